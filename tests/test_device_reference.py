"""The every-row forward reference (oracle/device_reference.py) on the CPU: its trajectory is the oracle's forward bit for
bit, its bars keep the 1e-5 floor, and its row check catches what the anchors' sampled check lets through -- one wrong
entry in a row that anchor_rows does not pick.  Also the loop-plan table tests/test_gpu_forward_rows.py runs on."""
import numpy as np
import pytest
import torch

import tspgnn
from conftest import load_pack
from oracle import device_reference as DR
from oracle import params as P
from oracle import torch_oracle as TO
from oracle.anchors import ANCHORS, anchor_rows
from tspgnn import graphnn, resident_plan

REL_TOL = 1e-5


def pack_batch(name, seed=0):
    g = load_pack(name, seed)
    return {k: g[k] for k in ("ev_uv", "W", "C", "route_exists", "n_vertices", "n_edges")}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d", [64, 32])
def test_trajectory_reproduces_the_oracle_forward_bit_for_bit(d, bf16):
    """Every depth of one trajectory equals torch_oracle.forward run to that depth (bf16: with the inference forward's
    fold, at every width), and a trajectory started from the state at depth 2 reaches depth 4's state."""
    T = 4
    batch = pack_batch("ragged_B6")
    params = P.init_params(d, seed=3, perturb=True)
    traj = DR.trajectory(params, batch, range(T + 1), torch.float64, "cpu", bf16=bf16)
    assert sorted(traj) == list(range(T + 1))
    tp = TO.to_torch(params, torch.float64)
    with torch.no_grad():
        for t in range(T + 1):
            ref = TO.forward(tp, batch, t, bf16=bf16, fold=DR.INFERENCE_FOLD)
            got = traj[t]
            for v, k in (("V", 0), ("E", 0), ("V", 1), ("E", 1)):
                assert torch.equal(got["%s.%s" % (v, "hc"[k])], ref["last_states"][v][k]), (t, v, k)
            for k in ("predictions", "loss", "acc", "TP", "FP", "TN", "FN"):
                assert torch.equal(got[k], ref[k]), (t, k)
    mid = traj[2]
    again = DR.trajectory(params, batch, [2], torch.float64, "cpu", start=(mid["V.h"], mid["V.c"], mid["E.h"], mid["E.c"]),
                          bf16=bf16)
    for k in DR.OUTPUTS:
        assert torch.equal(again[2][k], traj[4][k]), k
    if bf16 and d != 64:   # fold=None: the training forward's form, which at d != 64 rounds the aggregate instead
        train = DR.trajectory(params, batch, [T], torch.float64, "cpu", bf16=True, fold=None)
        with torch.no_grad():
            ref = TO.forward(tp, batch, T, bf16=True, fold=False)
        assert torch.equal(train[T]["E.h"], ref["last_states"]["E"][0])
        assert not torch.equal(train[T]["E.h"], traj[T]["E.h"])


def test_no_cell_state_is_the_zero_state():
    batch = pack_batch("ragged_B6")
    params = P.init_params(64, seed=3, perturb=True)
    traj = DR.trajectory(params, batch, [0, 1], torch.float64, "cpu")
    s = traj[0]
    a = DR.trajectory(params, batch, [1], torch.float64, "cpu", start=(s["V.h"], None, s["E.h"], None))
    for k in DR.OUTPUTS:
        assert torch.equal(a[1][k], traj[1][k]), k


def sampled_check(got, ref):
    """tests/test_gpu_anchors.py's check of a state array: 512 evenly spaced rows within 1e-5 of the tensor's largest entry,
    the column sums within 1e-5 of it times the number of rows.  -> the larger of the two ratios to 1e-5."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    rows = anchor_rows(ref.shape[0])
    e_rows = np.abs(got[rows] - ref[rows]).max() / scale
    e_sum = np.abs(got.sum(0) - ref.sum(0)).max() / (scale * ref.shape[0])
    return max(e_rows, e_sum) / REL_TOL


@pytest.fixture(scope="module")
def n20_reference():
    """n20_B32 (32 x n=20, 6 080 edge rows: more than anchor_rows picks) at T=2, bars and all, on the CPU."""
    batch = pack_batch("n20_B32")
    params = P.init_params(64, seed=3, perturb=True)
    ref, bars = DR.reference(params, batch, [2], "cpu")
    return batch, ref[2], bars[2]


def test_row_check_catches_one_wrong_entry_the_sampled_check_misses(n20_reference):
    batch, ref, bars = n20_reference
    Eh, bar = ref["E.h"], bars["E.h"]
    M = Eh.shape[0]
    S = float(Eh.abs().max())
    sampled = set(anchor_rows(M).tolist())
    assert len(sampled) < M
    # a row the anchors never look at, deep inside an instance, whose own bar is the floor's neighbourhood
    r = next(r for r in range(3 * 190 + 77, M) if r not in sampled and float(bar[r]) < 2e-5 * S)
    got = Eh.clone()
    got[r, 13] += 3e-5 * S
    assert sampled_check(got.numpy(), Eh.numpy()) < 1.0          # the anchors' check passes ...
    res = DR.compare_rows(got, Eh, bar, batch, "E.h")               # ... the row check does not, and says where
    assert res["worst"] > 1.0 and res["over"] == 1 and res["row"] == r, res
    n_edges = np.asarray(batch["n_edges"])
    assert np.all(n_edges == 190)
    assert res["instance"] == r // 190 and res["local"] == r % 190 and res["tile_row"] == r % 16
    u, v = np.asarray(batch["ev_uv"])[r] - 20 * (r // 190)
    assert res["uv"] == (int(u), int(v))
    msg = DR.describe(res)
    assert ("row %d = instance %d row %d" % (r, r // 190, r % 190)) in msg and ("tile %d row %d" % (r // 16, r % 16)) in msg
    # and the reference against itself: nothing over
    for k in DR.STATES:
        assert DR.compare_rows(ref[k], ref[k], bars[k], batch, k)["worst"] == 0.0


def test_row_check_locates_vertex_rows_and_instances(n20_reference):
    batch, ref, bars = n20_reference
    got = ref["V.c"].clone()
    got[333, 5] = float("nan")
    res = DR.compare_rows(got, ref["V.c"], bars["V.c"], batch, "V.c")
    assert res["worst"] == float("inf") and res["over"] == 1 and (res["row"], res["instance"], res["local"]) == (333, 16, 13)
    p = ref["predictions"].clone()
    p[7] += 1e-3
    res = DR.compare_rows(p, ref["predictions"], bars["predictions"], batch, "predictions")
    assert res["worst"] > 1.0 and res["instance"] == 7


def test_every_bar_keeps_the_floor(n20_reference):
    _, ref, bars = n20_reference
    for k in DR.OUTPUTS:
        S = float(ref[k].abs().max())
        assert bars[k].shape[0] == (ref[k].shape[0] if ref[k].dim() else 1)
        assert bool(torch.all(bars[k] >= DR.FLOOR * S)) and bool(torch.all(torch.isfinite(bars[k]))), k
        # the conditioning terms stay below the floor's order almost everywhere at T=2: the floor is what most rows get
        assert float((bars[k] <= 2 * DR.FLOOR * S).double().mean()) > 0.9, k


def test_bars_stay_finite_on_zero_rows():
    ref = torch.randn(40, 8, dtype=torch.float64)
    ref[[0, 17, 39]] = 0.0
    f32 = ref.float()
    bar = DR.bar_of(ref, DR.row_err(f32, ref), torch.zeros(40, dtype=torch.float64))
    S = float(ref.abs().max())
    assert bool(torch.all(torch.isfinite(bar))) and bool(torch.all(bar >= DR.FLOOR * S))
    assert bool(torch.all(bar[[0, 17, 39]] == DR.FLOOR * S))
    res = DR.compare_rows(ref, ref, bar, {"n_vertices": [20, 20]}, "V.h")
    assert res["worst"] == 0.0 and res["over"] == 0
    zero = torch.zeros(5, 8, dtype=torch.float64)
    bz = DR.bar_of(zero, torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64))
    assert bool(torch.all(torch.isfinite(bz))) and bool(torch.all(bz > 0))


# The batches tests/test_gpu_forward_rows.py runs and the one-launch form the selector gives each (grid 256, MI355X's
# CUs): ``None`` = the stepwise launches.  Keys: default (TSPGNN_LOOP_KIND unset), "loop", "loop" with
# TSPGNN_LOOP_MAX_TILES=4, "resident".
PLAN_TABLE = {
    "c1": ([20] * 32, {"auto": "loop", "loop": "loop", "loop4": "loop", "resident": "resident"}),
    "c2": ([40] * 128, {"auto": None, "loop": None, "loop4": "loop", "resident": "resident"}),
    "192x40": ([40] * 192, {"auto": "resident", "loop": None, "loop4": None, "resident": "resident"}),
    "c4": (None, {"auto": None, "loop": None, "loop4": None, "resident": None}),
    "32x200": ([200] * 32, {"auto": None, "loop": None, "loop4": None, "resident": "resident"}),
}


def plan_kind(sizes, kind, monkeypatch):
    monkeypatch.delenv("TSPGNN_LOOP_MAX_TILES", raising=False)
    monkeypatch.delenv("TSPGNN_LOOP_KIND", raising=False)
    if kind != "auto":
        monkeypatch.setenv("TSPGNN_LOOP_KIND", kind.rstrip("4"))
    if kind == "loop4":
        monkeypatch.setenv("TSPGNN_LOOP_MAX_TILES", "4")
    ev = tspgnn.synthetic_batch(sizes, seed=1234)[0]
    built = graphnn.choose_loop_plan(ev.blocks[0], ev.blocks[1], 256)
    return None if built is None else built[1][2]


@pytest.mark.parametrize("name", sorted(PLAN_TABLE))
def test_loop_plan_table_of_the_row_tests(name, monkeypatch):
    sizes, want = PLAN_TABLE[name]
    sizes = sizes if sizes is not None else ANCHORS["c4"][0]()
    for kind, k in want.items():
        assert plan_kind(sizes, kind, monkeypatch) == k, (name, kind)
    if name == "32x200":   # degree 199: the resident kernel's row-sum leaves its LDS share for the general loop
        assert 199 > resident_plan.SHARE_CAP
