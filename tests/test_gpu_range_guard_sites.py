"""The f16x2 range guard (include/tspgnn.h, range_flag) at every site that raises it in the forward launches called
directly -- tspgnn_mlp_fwd_multi_h2 (with and without the projection second phase), tspgnn_mlp_head_fwd_h2,
tspgnn_lnlstm_fwd_multi_h2, tspgnn_lnlstm_mlp_fwd_multi_h2 (csrc/dense_h2.hip) -- one assertion per site:

  bit 0: the [x | h] operand of a cell in a resident task (kloop), in the preloaded lock-step path, in lock-step with K
  staged whole and in two chunks -- one planted entry in each 16-column half of every k-block of x and of h, in the first
  row, the last row of a partial last tile and the only live row of a second lock-step round: 65519 leaves the word 0 and
  the outputs within the bars of tests/test_gpu_cell_forward_edges.py, 65520 and -7e4 set bit 0 and only bit 0; h' into the
  fused MLP, the input of each later layer, the projection's input (one site each: range_guard_cases.plant_new_h,
  plant_bias, plant_chain); the plain MLP launches' X, hidden layers, second-phase projection and head variant;
  bit 1: each gate of the cell alone below the variance floor and alone above it, with and without the CENTERED LayerNorm;
  one row alone below it; a row whose z is exactly 0 (ignored, and its outputs correct);
  no raise from memory the task does not own: pad rows of blocked input states holding 1e30, idle lock-step wavefronts beside
  a last row that holds 6.0e4.

The cases are range_guard_cases' generators; tests/test_range_guard_cases_host.py has judged every one of them in float64
(the intended site beyond 7.0e4 or the floor / 4, every other within 6.0e4 and 4 floors), so an unexpected word here is the
kernel's.  Each test asserts its launch path through plan_replay.cell_fwd_plan before it launches.  A flagged launch's
outputs are not compared; it must still leave every row beyond the task's own untouched."""
import pytest
import torch

import range_guard_cases as RG
from cell_fwd_cases import ENTRY, t64
from lstm_bwd_cases import release
from plan_replay import cell_fwd_plan, mlp_fwd_plan
from test_gpu_cell_forward_edges import ROW_TOL, TOL, check, check_mlp, cus
from tspgnn import _lib

pytestmark = pytest.mark.gpu

KEYS = sorted(RG.SITE_KEYS)
KEY_IDS = ["%d-%s-%d-%s" % (d, mode, dx, "mlp" if mlp else "cell") for d, mode, dx, mlp in KEYS]
FUSED = [k for k in KEYS if k[3]]
FUSED_IDS = [i for k, i in zip(KEYS, KEY_IDS) if k[3]]
ROW_KINDS = ["one_row", "first_row", "last_row_of_partial_tile", "second_round_only_row"]


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def launch(cells, d, device):
    """A task without an MLP and with row-major states goes through tspgnn_lnlstm_fwd_multi_h2 (which wraps it into the
    fused launch), everything else through tspgnn_lnlstm_mlp_fwd_multi_h2."""
    tasks = [c.task(device) for c in cells]
    if all(c.L == 0 and c.P is None and not (c.in_blocked or c.out_blocked) for c in cells):
        _lib.call_multi("tspgnn_lnlstm_fwd_multi_h2", [t.cell for t in tasks], d)
    else:
        _lib.call_multi(ENTRY["h2"], tasks, d)
    torch.cuda.synchronize()


def rows_of(kind, key, device):
    """(rows, row) of a ROW_KINDS entry; the second round's size from the launch's own wavefront count."""
    d, mode, dx, mlp = key
    nw = cell_fwd_plan([RG.site_cell(d, mode, dx, mlp, 17, 1).plan()], d, cus(device), "h2").nw
    return RG.row_cases(nw)[ROW_KINDS.index(kind)]


def claim_path(key, cell, device, second_round=False):
    p = cell_fwd_plan([cell.plan()], cell.d, cus(device), "h2")
    t = p.tasks[0]
    assert RG.path_of(t) == RG.SITE_KEYS[key], (key, t)
    if second_round and t.mode == "lockstep":
        assert t.rounds == 2 and t.lock_tiles == p.nw and t.tiles - t.lock_tiles == 1 and cell.rows % 16 == 1, t


def check_head(case, y_ref, device, label):
    """The head's y[row] = <a, hw> + hb, a the last layer's output row.  check_mlp measures y against the largest |y| of
    the whole task, which for a task of one row is that row's own y -- a dot product that may cancel to any size, here of
    terms that a planted 65519 makes thousands of times larger.  Row by row instead, against what the other bars and fp32
    summation allow: a within ROW_TOL of its row's largest entry (the bar it has just passed), d products summed in fp32
    (d 2^-24 < TOL of the sum of their magnitudes):  |y - ref| <= ROW_TOL max|a| sum|hw| + TOL (sum|a hw| + |hb|)."""
    a = case.reference(device)["Y"]
    hw = t64(case.hw, device)[:, 0].abs()
    bar = ROW_TOL * a.abs().max(dim=1).values * hw.sum() + TOL * (a.abs() @ hw + abs(float(case.hb[0])))
    err = (case.buf["y"][:case.rows, 0].double() - y_ref[:, 0]).abs()
    print(" HEAD %s: worst |y - ref| / bar %.2e" % (label, float((err / bar).max())))
    assert bool((err <= bar).all()), (label, float((err / bar).max()))


def judge(label, case, design, device, what):
    """The launched case against its design: the exact word; quiet: the outputs within the bars; flagged: nothing written
    beyond the task's rows."""
    word = case.range_flag()
    print(" GUARD %s %s: word %d (design %d)" % (what, label, word, design.word))
    assert word == design.word, "%s, %s: range_flag %d, design %s" % (what, label, word, design)
    if design.word == 0:
        if isinstance(case, RG.MlpCase):
            case.buf["flag"] = case.flag
            ref = dict(case.reference(device))
            y = ref.pop("y", None)
            check_mlp("h2", case.rows, case.buf, ref, label)
            if y is not None:
                check_head(case, y, device, label)
        else:
            check(case, device, label)
    assert not case.untouched(), ("written beyond the task's rows", label, case.untouched())


# ------------------------------------------------------------------------------------------------ bit 0: the cell launch
@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_planted_entry_of_x_and_h(cuda_device, key, kind):
    """split2w of the [x | h] operand: kloop (resident; lock-step chunk by chunk) and the preloaded lock-step path."""
    d, mode, dx, mlp = key
    rows, row = rows_of(kind, key, cuda_device)
    n = 0
    for label, cell, design in RG.planted_cell_cases(d, mode, dx, mlp, rows, row):
        if n == 0:
            claim_path(key, cell, cuda_device, second_round=kind == "second_round_only_row")
        launch([cell], d, cuda_device)
        judge(label, cell, design, cuda_device, "%s %d rows" % (KEY_IDS[KEYS.index(key)], rows))
        release()
        n += 1
    assert n == 3 * 2 * (dx + d) // 32


@pytest.mark.parametrize("kind", ["one_row", "last_row_of_partial_tile", "second_round_only_row"])
@pytest.mark.parametrize("key", FUSED, ids=FUSED_IDS)
def test_fused_mlp_and_projection_operands(cuda_device, key, kind):
    """dense_layer_h2 per fused layer (resident and lock-step) and the fused projection's operand: h' into layer 1, each later
    layer's input, the projection's input, each the only site beyond the range; the same task untouched stays quiet."""
    d, mode, dx, _ = key
    rows, _ = rows_of(kind, key, cuda_device)
    n = 0
    for label, cell, design in RG.fused_site_cases(d, mode, dx, rows):
        if n == 0:
            claim_path(key, cell, cuda_device, second_round=kind == "second_round_only_row")
        launch([cell], d, cuda_device)
        judge(label, cell, design, cuda_device, "%s %d rows" % (FUSED_IDS[FUSED.index(key)], rows))
        release()
        n += 1
    assert n == (6 if dx else 4)


# ------------------------------------------------------------------------------------------- bit 0: the plain MLP launches
@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("entry", sorted(RG.MLP_KINDS))
def test_plain_mlp_operands(cuda_device, entry, d, kind):
    """mlp_fwd_h2_kernel: dense_layer_h2 per layer (X planted in each half of every k-block; each hidden layer's input
    through a one-column chain that only one row carries), the second-phase projection's operand, the head variant."""
    nw = mlp_fwd_plan([(17, 3, False)], cus(cuda_device)).nw
    rows, row = RG.row_cases(nw)[ROW_KINDS.index(kind)]
    n = 0
    for cases in (RG.planted_mlp_cases(entry, d, rows, row), RG.chain_mlp_cases(entry, d, rows, row)):
        for label, case, design in cases:
            case.launch(cuda_device)
            judge(label, case, design, cuda_device, "%s d=%d %d rows" % (entry, d, rows))
            release()
            n += 1
    assert n == 3 * 2 * d // 32 + {"plain": 3, "head": 3, "proj": 5}[entry]


# ----------------------------------------------------------------------------------------------------------------- bit 1
@pytest.mark.parametrize("centred", [False, True], ids=["plain_ln", "centred"])
@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_each_gate_tracks_its_variance(cuda_device, key, rows, centred):
    """ln_gate<..., TRACK> in each of the four gates, with and without CENTERED: one gate's z alone below the floor raises
    bit 1 and only bit 1, and so do the other three with this one left alone."""
    d, mode, dx, mlp = key
    n = 0
    for label, cell, design in RG.gate_cases(d, mode, dx, mlp, rows, centred):
        if n == 0:
            claim_path(key, cell, cuda_device)
            assert cell_fwd_plan([cell.plan()], d, cus(cuda_device), "h2").centered == centred
        launch([cell], d, cuda_device)
        judge(label, cell, design, cuda_device, "%s %d rows%s" % (KEY_IDS[KEYS.index(key)], rows, " centred" if centred else ""))
        release()
        n += 1
    assert n == 8


@pytest.mark.parametrize("centred", [False, True], ids=["plain_ln", "centred"])
@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_one_row_below_the_floor_and_one_exactly_zero(cuda_device, key, kind, centred):
    """One row's z at 2^-9 of its size raises bit 1 wherever the row sits; a row whose z is exactly 0 does not, and its
    outputs match float64."""
    d, mode, dx, mlp = key
    rows, row = rows_of(kind, key, cuda_device)
    n = 0
    for label, cell, design in RG.one_row_cases(d, mode, dx, mlp, rows, row, centred):
        if n == 0:
            claim_path(key, cell, cuda_device, second_round=kind == "second_round_only_row")
        launch([cell], d, cuda_device)
        judge(label, cell, design, cuda_device, "%s %d rows%s" % (KEY_IDS[KEYS.index(key)], rows, " centred" if centred else ""))
        release()
        n += 1
    assert n == 2


# ------------------------------------------------------------------------------------------ memory the task does not own
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_pad_rows_of_blocked_input_states_are_not_read(cuda_device, key):
    """17 rows in blocked states whose 15 pad rows hold 1e30: a lane beyond the task's rows that split them, or normalised
    by them, would raise the word."""
    d, mode, dx, mlp = key
    cell = RG.pad_fill_cell(d, mode, dx, mlp)
    claim_path(key, cell, cuda_device)
    launch([cell], d, cuda_device)
    judge("pad rows 1e30", cell, RG.QUIET_DESIGN, cuda_device, KEY_IDS[KEYS.index(key)])


@pytest.mark.parametrize("kind", ["one_row", "last_row_of_partial_tile", "second_round_only_row"])
@pytest.mark.parametrize("d", [32, 64])
def test_in_range_last_row_beside_idle_wavefronts(cuda_device, d, kind):
    """A lock-step vertex task beside an edge task: its last row, which every clamped lane of its partial tile reads again
    and which an idle wavefront would clamp to, holds 6.0e4 in x and h -- in range: the word of both tasks stays 0."""
    nw = cell_fwd_plan([c.plan() for c in RG.companion_cells(d, 17)], d, cus(cuda_device), "h2").nw
    v_rows = RG.row_cases(nw)[ROW_KINDS.index(kind)][0]
    cells = RG.companion_cells(d, v_rows)
    p = cell_fwd_plan([c.plan() for c in cells], d, cus(cuda_device), "h2")
    v = p.tasks[1]
    assert [t.mode for t in p.tasks] == ["resident", "lockstep"] and v.tiles - (v.rounds - 1) * v.lock_tiles < p.nw, p
    launch(cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        judge("6.0e4 in the last row", c, RG.QUIET_DESIGN, cuda_device, what)
