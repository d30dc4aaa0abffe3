"""The designs of the range-guard cases (tests/range_guard_cases.py), judged on the CPU in float64 before any kernel sees
them: every case that tests/test_gpu_range_guard_sites.py and tests/test_gpu_range_guard_loop.py launch meets the conditions of
range_guard_cases' docstring -- the intended operand at or beyond 7.0e4 (or the planted value itself) and every other split
operand within 6.0e4; the intended gates with a row of positive variance at most a quarter of the floor and every other
positive variance at least four times it -- so that a GPU test can neither pass nor fail for a reason other than the one
raise site it names.  The launch paths the cases claim (resident, lock-step with and without the operand preload, K in two
chunks, a second lock-step round of one live row) are asked of the library's host-side planner for a 256-CU device."""
import numpy as np
import pytest
import torch

import range_guard_cases as RG
from oracle import params as P
from oracle import torch_oracle as TO
from plan_replay import cell_fwd_plan

CUS = 256
NW = 4          # wavefronts per workgroup of a launch this small (asserted in test_launch_paths)
KEYS = sorted(RG.SITE_KEYS)
KEY_IDS = ["%d-%s-%d-%s" % (d, mode, dx, "mlp" if mlp else "cell") for d, mode, dx, mlp in KEYS]
ROWS = RG.row_cases(NW)


def judge(cases):
    n = 0
    for label, task, design in cases:
        bad = RG.design_faults(task.operands("cpu"), design)
        assert not bad, (label, design, bad)
        n += 1
    assert n > 0
    return n


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_launch_paths(key):
    d, mode, dx, mlp = key
    for rows, row in ROWS:
        p = cell_fwd_plan([RG.site_cell(d, mode, dx, mlp, rows, 1).plan()], d, CUS, "h2")
        t = p.tasks[0]
        assert p.nw == NW and RG.path_of(t) == RG.SITE_KEYS[key], (rows, p)
        if t.mode == "lockstep" and rows > 17:       # a second round whose only live wavefront holds one row
            assert t.lock_tiles == NW and t.rounds == 2 and t.tiles - NW == 1 and row == rows - 1 == 16 * NW


def test_operands_of_a_task_on_the_cpu():
    """FwdCell.operands: every tensor the launch splits, and the variance of each gate's z, from the reference's operands."""
    cell = RG.site_cell(64, "bias", 64, True, 17, 5)
    ops = cell.operands("cpu")
    assert sorted(ops) == ["h", "layer1", "layer2", "layer3", "layer4", "proj", "var", "x"]
    ref = cell.reference("cpu")
    assert torch.equal(ops["layer1"], ref["h"]) and torch.equal(ops["layer2"], ref["acts"][0])
    assert torch.equal(ops["proj"], ref["msg"]) and ops["var"].shape == (17, 4) and ops["x"].dtype == torch.float64
    z = np.concatenate([cell.x, cell.h], 1).astype(np.float64) @ cell.K.astype(np.float64) \
        + cell.zscale.astype(np.float64)[:, None] * cell.zbias.astype(np.float64)[None]
    assert np.allclose(ops["var"].numpy(), z.reshape(17, 4, 64).var(axis=2), rtol=1e-12)
    assert sorted(RG.site_cell(32, "gather", 0, False, 3, 5).operands("cpu")) == ["h", "var"]


# ---------------------------------------------------------------------------------------------------------------- bit 0
@pytest.mark.parametrize("rows,row", ROWS)
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_planted_x_and_h_designs(key, rows, row):
    d, mode, dx, mlp = key
    n = judge(RG.planted_cell_cases(d, mode, dx, mlp, rows, row))
    assert n == 3 * 2 * (dx + d) // 32


@pytest.mark.parametrize("rows", [1, 17, 16 * NW + 1])
@pytest.mark.parametrize("key", [k for k in KEYS if k[3]], ids=[i for k, i in zip(KEYS, KEY_IDS) if k[3]])
def test_fused_site_designs(key, rows):
    d, mode, dx, _ = key
    n = judge(RG.fused_site_cases(d, mode, dx, rows))
    assert n == (6 if dx else 4)     # h', every later layer's input (, the projection's), and the ordinary task


@pytest.mark.parametrize("rows,row", ROWS)
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("kind", sorted(RG.MLP_KINDS))
def test_plain_mlp_designs(kind, d, rows, row):
    assert judge(RG.planted_mlp_cases(kind, d, rows, row)) == 3 * 2 * d // 32
    assert judge(RG.chain_mlp_cases(kind, d, rows, row)) == {"plain": 3, "head": 3, "proj": 5}[kind]


# ---------------------------------------------------------------------------------------------------------------- bit 1
@pytest.mark.parametrize("centred", [False, True], ids=["plain_ln", "centred"])
@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_gate_designs(key, rows, centred):
    d, mode, dx, mlp = key
    assert judge(RG.gate_cases(d, mode, dx, mlp, rows, centred)) == 8


@pytest.mark.parametrize("centred", [False, True], ids=["plain_ln", "centred"])
@pytest.mark.parametrize("rows,row", ROWS)
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_one_row_designs(key, rows, row, centred):
    d, mode, dx, mlp = key
    cases = list(RG.one_row_cases(d, mode, dx, mlp, rows, row, centred))
    assert judge(cases) == 2
    zero = cases[1][1].operands("cpu")["var"][row]
    assert bool((zero == 0).all()), "the zero row's variance must be exactly 0 (the guard ignores only that)"


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_foreign_memory_designs(key):
    d, mode, dx, mlp = key
    cell = RG.pad_fill_cell(d, mode, dx, mlp)
    assert cell.in_blocked and cell.pad_fill == 1.0e30 and cell.rows % 16
    assert not RG.design_faults(cell.operands("cpu"), RG.QUIET_DESIGN)


@pytest.mark.parametrize("v_rows", [1, 17, 16 * NW + 1])
@pytest.mark.parametrize("d", [32, 64])
def test_companion_designs(d, v_rows):
    cells = RG.companion_cells(d, v_rows)
    p = cell_fwd_plan([c.plan() for c in cells], d, CUS, "h2")
    assert [t.mode for t in p.tasks] == ["resident", "lockstep"]
    v = p.tasks[1]
    assert v.tiles - (v.rounds - 1) * v.lock_tiles < p.nw, "no idle wavefront in the vertex task's last round"
    for c in cells:
        assert not RG.design_faults(c.operands("cpu"), RG.QUIET_DESIGN)
    assert RG.absmax(cells[1].operands("cpu"))["x"] == RG.SAFE == RG.absmax(cells[1].operands("cpu"))["h"]


# ------------------------------------------------------------------------------------------------------- the whole model
def test_the_collector_changes_nothing():
    """sites=None is the oracle as it was; a collector records and leaves every output bit for bit."""
    import tspgnn
    from conftest import batch_from_tuple
    batch = batch_from_tuple(tspgnn.synthetic_batch([9, 14], seed=2))
    params = TO.to_torch(P.init_params(64, seed=3, perturb=True), torch.float64)
    plain = TO.forward(params, batch, 2)
    sites = TO.RangeSites()
    seen = TO.forward(params, batch, 2, sites=sites)
    assert torch.equal(plain["predictions"], seen["predictions"]) and torch.equal(plain["loss"], seen["loss"])
    for var in ("E", "V"):
        for a, b in zip(plain["last_states"][var], seen["last_states"][var]):
            assert torch.equal(a, b)
    assert set(RG.MODEL_SPLIT) <= set(sites.absmax) and set(RG.MODEL_GATES) == set(sites.minvar)
    # the pushed operand: the row-sum of the LAST HIDDEN activation, so that x_pushed W + degree b is the cell's x
    Eh = TO.initial_embeddings(params, batch)[1]
    a = Eh
    for l in (1, 2, 3):
        a = torch.relu(a @ params["TSP/E_msg_V_MLP_layer_%d/kernel" % l] + params["TSP/E_msg_V_MLP_layer_%d/bias" % l])
    uv = torch.as_tensor(np.asarray(batch["ev_uv"]), dtype=torch.long)
    pushed = torch.zeros((23, 64), dtype=torch.float64).index_add(0, uv[:, 0], a).index_add(0, uv[:, 1], a)
    one = TO.RangeSites()
    TO.forward(params, batch, 1, sites=one)
    assert torch.equal(one.last["V_cell/x_pushed"], pushed)
    deg = torch.zeros(23, dtype=torch.float64).index_add(0, uv.reshape(-1), torch.ones(2 * uv.shape[0], dtype=torch.float64))
    x = pushed @ params["TSP/E_msg_V_MLP_layer_4/kernel"] + deg[:, None] * params["TSP/E_msg_V_MLP_layer_4/bias"]
    assert torch.allclose(one.last["V_cell/x"], x, rtol=1e-12, atol=1e-12)


MODEL_CASES = RG.model_cases()


@pytest.mark.parametrize("case", MODEL_CASES, ids=[c.label.replace(" ", "_") for c in MODEL_CASES])
def test_model_case_designs(case):
    import tspgnn
    from conftest import batch_from_tuple
    assert len(case.sizes) <= 3 and max(case.sizes) <= 40 and case.T in (1, 2, 3)
    sites = TO.RangeSites()
    out = TO.forward(TO.to_torch(case.params, torch.float64), batch_from_tuple(tspgnn.synthetic_batch(case.sizes, seed=3)), case.T,
                     sites=sites)
    assert bool(torch.isfinite(out["predictions"]).all())
    bad = RG.model_design_faults(case, sites)
    assert not bad, (case.label, bad)


def test_chain_cases_leave_the_messages_of_step_0_in_range():
    """What sets the "behind new h" cases apart from the bias cases: with T = 0 cell updates -- the message MLPs on the initial
    embeddings alone, which is all the plain MLP launch of step 0 computes -- every operand is within SAFE."""
    import tspgnn
    from conftest import batch_from_tuple
    n = 0
    for case in MODEL_CASES:
        if "behind new h" not in case.label:
            continue
        params = TO.to_torch(case.params, torch.float64)
        batch = batch_from_tuple(tspgnn.synthetic_batch(case.sizes, seed=3))
        V0, E0 = TO.initial_embeddings(params, batch)
        sites = TO.RangeSites()
        TO.mlp(E0, params, "TSP/E_msg_V", sites=sites)
        sites.operand("TSP/V_msg_E_out", TO.mlp(V0, params, "TSP/V_msg_E", sites=sites))
        assert max(sites.absmax.values()) <= RG.SAFE, (case.label, sites.absmax)
        n += 1
    assert n == 6
