"""The fused forward cell launch, tspgnn_lnlstm_mlp_fwd_multi_h2 (csrc/dense_h2.hip: launch_cell_h2 /
lnlstm_mlp_fwd_h2_kernel) -- the launch the inference and the training forward are made of -- and, wherever its entry
accepts the task, tspgnn_lnlstm_mlp_fwd_multi_x3, called directly against float64 on the device at the launch's own edges:
every mode (plain dx, gather-init, bias-init; with and without the fused MLP) from 1 row to ROWS_DEEP = 16 * (12 * 2 * CUs)
+ 1 rows; both sides of the 4- and 8-wavefront thresholds with idle and one-row lock-step wavefronts; the fixed split, its
plain fallback, several rounds per lock-step workgroup, the write-through variant on and off; every remainder mod 8 of a
resident task's workgroup count (xcd_contiguous); the blocked state layouts, in-place states, c == NULL, strided mlp_acts,
a projection without mlp_out; the CENTERED variant and a mixed launch; bit-equality of a task alone and beside a companion.
The plain MLP launches (tspgnn_mlp_fwd_multi_{h2,x3}, tspgnn_mlp_head_fwd_h2) at their 8-wavefront plan come last.

Every test that claims a branch asserts it through plan_replay.cell_fwd_plan / mlp_fwd_plan with the device's CU count
BEFORE it launches: a changed launcher fails the claim instead of quietly testing something else.

Bars, all against float64: whole tensor rel_err < TOL = 5e-6 (the bar of test_gpu_split_kernels.py); row by row
lstm_bwd_cases.row_err < ROW_TOL = 2e-5 (the bar of the backward suite) on h', c', the messages, the saved activations and
the unpacked projection.  Every check also finds the rows beyond the task's own (16 spare rows; the pad rows of a blocked
or projected-message buffer's last tile; the other slot of a strided mlp_acts) untouched, every row of the task written,
and the f16x2 range_flag still 0 -- with idle lock-step wavefronts, dead tiles, zscale = 0 rows and the centred variant.
Each check prints its worst ratios.

Measured on the MI355X (256 CUs), worst over all cases, f16x2 / bf16x3 -- whole tensor: h' 6.3e-7 / 5.8e-7, c' 4.9e-7 /
6.0e-7, messages 5.3e-7 / 4.9e-7, saved activations 5.4e-7 / --, projection 5.5e-7 / 4.4e-7; row by row: h' 1.9e-6 / 2.2e-6,
c' 1.4e-6 / 1.7e-6, messages 1.3e-6 / 1.4e-6, activations 2.0e-6 / --, projection 1.1e-6 / 1.1e-6; the plain MLP launches
<= 3.3e-7 whole and <= 8.2e-7 row by row.  Row by row the worst are those at ROWS_DEEP (the maximum grows with the number of
rows it is taken over): rounding, a tenth of either bar, so neither was raised.  The whole file: 423 tests, 36 s, 1.8 GB peak
device memory ("The forward cell launches at their own edges", also for the mutations the tests were tried on)."""
import ctypes
import time

import numpy as np
import pytest
import torch

from cell_fwd_cases import ENTRY, FwdCell, draw_mlp, mlp64, mlp_blocks, packed, blocked_unpack, pad16, t64, wscale
from conftest import rel_err
from lstm_bwd_cases import SENTINEL, SPARE, dev, empty, release, row_err
from plan_replay import cell_fwd_plan, cell_task, mlp_fwd_plan
from tspgnn import _lib

pytestmark = pytest.mark.gpu

TOL = 5e-6
ROW_TOL = 2e-5
ARITHS = ["h2", "x3"]
ROWS = [1, 15, 16, 17, 333, "deep"]


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


@pytest.fixture(scope="module", autouse=True)
def _time_and_memory():
    t0 = time.time()
    yield
    if torch.cuda.is_available():
        print("\n[cell forward edges] wall %.1f s, peak device memory %.0f MiB" % (
            time.time() - t0, torch.cuda.max_memory_allocated() / 2.0 ** 20))


def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def rows_deep(device):
    """Alone in a launch at 12 wavefronts: a resident task's wavefronts take two or three tiles each, a lock-step task's
    workgroups two or three rounds, and the last tile holds one row (98 305 rows on 256 CUs)."""
    return 16 * (12 * 2 * cus(device)) + 1


def plan(cells, d, device, arith):
    return cell_fwd_plan([c.plan() for c in cells], d, cus(device), arith)


def launch(arith, cells, d, device):
    tasks = [c.task(device) for c in cells]
    _lib.call_multi(ENTRY[arith], tasks, d)
    torch.cuda.synchronize()


def check(cell, device, what=""):
    """Every output of the launched task against float64 -- whole tensor at TOL, row by row at ROW_TOL -- every row written,
    nothing written beyond them, the range guard quiet.  Prints the worst ratios before it asserts."""
    got, ref = cell.outputs(), cell.reference(device)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    whole, rowwise = {}, {}
    for n, a in got.items():
        a = a.reshape(-1, a.shape[-1]).cpu().numpy().astype(np.float64)
        b = ref[n].reshape(-1, ref[n].shape[-1]).cpu().numpy()
        whole[n], rowwise[n] = rel_err(a, b), row_err(a, b)
    print(" CELLFWD %s %s[%d rows] whole %s row %s" % (
        cell.arith, what, cell.rows, " ".join("%s %.1e" % kv for kv in whole.items()),
        " ".join("%s %.1e" % kv for kv in rowwise.items())))
    assert not cell.unwritten(), ("rows left unwritten", cell.unwritten())
    assert not cell.untouched(), ("written beyond the task's rows", cell.untouched())
    if cell.arith == "h2":
        assert cell.range_flag() == 0, "range_flag %d from ordinary operands" % cell.range_flag()
    over = [("whole", n, e) for n, e in whole.items() if not e < TOL] + \
        [("row", n, e) for n, e in rowwise.items() if not e < ROW_TOL]
    assert not over, over      # every measure that misses its bar, not only the first


def same_bits(a, b):
    ga, gb = a.outputs(), b.outputs()
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def edge_cell(arith, d, rows, seed, **kw):
    """The step's edge task: gather-init cell + 3 relu layers -> messages (h2: the activations saved, default stride)."""
    kw.setdefault("acts", "default" if arith == "h2" else None)
    return FwdCell(arith, d, rows, seed, mode="gather", mlp_layers=3, **kw)


def vertex_cell(arith, d, rows, seed, **kw):
    """The step's vertex task: bias-init cell on [x | h], dx = d, + 4 layers (the last linear) + projection (h2: the
    activations saved with an explicit layer stride)."""
    kw.setdefault("acts", "strided" if arith == "h2" else None)
    return FwdCell(arith, d, rows, seed, dx=d, mode="bias", mlp_layers=4, relu_mask=0b0111, proj=True, **kw)


# ---------------------------------------------------------------------------------------- every mode, 1 row ... deep
# (d, mode, dx) -> the task's mode per (arith, fused MLP): "r" resident, "lN" lock-step with N stagings of K per round
MODES = {(64, "plain", 0): "r r r r", (64, "plain", 64): "r l1 l2 l2", (64, "plain", 192): "l2 l2 l3 l3",
         (64, "gather", 0): "r r r r", (64, "bias", 64): "r l1 l2 l2",
         (32, "plain", 0): "r r r r", (32, "plain", 32): "r l1 r l2", (32, "plain", 96): "r l1 r l2",
         (32, "plain", 256): "r l1 l2 l2", (32, "plain", 320): "l2 l2 l2 l2",
         (32, "gather", 0): "r r r r", (32, "bias", 32): "r l1 r l2"}


def mode_cell(arith, d, mode, dx, mlp, rows, seed):
    if not mlp:
        return FwdCell(arith, d, rows, seed, dx=dx, mode=mode)
    acts = None if arith == "x3" else ("default" if mode == "gather" else "strided")
    if dx == 0:     # the edge form: 3 layers -> messages (plain dx = 0: an inner layer without relu)
        return FwdCell(arith, d, rows, seed, mode=mode, mlp_layers=3, relu_mask=0b111 if mode == "gather" else 0b101, acts=acts)
    return FwdCell(arith, d, rows, seed, dx=dx, mode=mode, mlp_layers=4, relu_mask=0b0111, proj=True, acts=acts)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("mlp", [False, True], ids=["cell", "mlp"])
@pytest.mark.parametrize("d,mode,dx", sorted(MODES))
@pytest.mark.parametrize("arith", ARITHS)
def test_every_mode_vs_float64(cuda_device, arith, d, mode, dx, mlp, rows):
    """One task alone.  The mode it runs in is asserted from MODES; at "deep" also that every wavefront of a resident task
    takes two or three tiles (and some three), that every workgroup of a lock-step task runs two or three rounds, and that
    the last tile -- the only live one of the last lock-step round -- holds one row."""
    seed = d * 7 + dx + (rows if isinstance(rows, int) else 98305) + 1000 * mlp
    rows = rows if isinstance(rows, int) else rows_deep(cuda_device)
    cell = mode_cell(arith, d, mode, dx, mlp, rows, seed)
    p = plan([cell], d, cuda_device, arith)
    t = p.tasks[0]
    want = MODES[(d, mode, dx)].split()[2 * ARITHS.index(arith) + int(mlp)]
    assert (t.mode[0] + (str(t.chunks) if t.mode == "lockstep" else "")) == want, (t, want)
    if arith == "h2" and t.mode == "lockstep":
        assert t.preload == ((dx + d) // 32 <= 4) and (cell.P is None or t.together == 1)
    if rows > 333:
        assert p.nw == 12 and rows % 16 == 1
        if t.mode == "resident":
            share = [e - b for b, e in t.ranges]
            assert min(share) // 12 >= 2 and -(-max(share) // 12) == 3, (min(share), max(share))
        else:
            assert t.rounds_per_wg == (2, 3) and t.tiles - (t.rounds - 1) * t.lock_tiles == 1, t
    launch(arith, [cell], d, cuda_device)
    check(cell, cuda_device, "%s dx=%d d=%d %s" % (mode, dx, d, "mlp" if mlp else "cell"))


# ------------------------------------------------------------------------------------------------- wavefront counts
@pytest.mark.parametrize("companion", ["alone", "one_row", "last_wavefront_one_row", "second_round_one_row"])
@pytest.mark.parametrize("per_cu,over", [(4, 0), (4, 1), (8, 0), (8, 1)])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("arith", ARITHS)
def test_wavefront_thresholds(cuda_device, arith, d, per_cu, over, companion):
    """Total tiles = 4 CUs, 4 CUs + 1, 8 CUs, 8 CUs + 1: 4, 8, 8 and 12 wavefronts per workgroup.  The edge task alone, and
    beside a lock-step vertex task of 1 row (idle wavefronts in its only round), of 16 (nw - 1) + 1 rows (its last wavefront
    holds one row) and of 16 nw + 1 rows (a second round with one live wavefront of one row)."""
    n = cus(cuda_device)
    total = per_cu * n + over
    nw = 4 if total <= 4 * n else (8 if total <= 8 * n else 12)
    v_rows = {"alone": 0, "one_row": 1, "last_wavefront_one_row": 16 * (nw - 1) + 1, "second_round_one_row": 16 * nw + 1}[companion]
    v_tiles = (v_rows + 15) // 16
    e_rows = 16 * (total - v_tiles) - 5          # the edge task's last tile is partial too
    blocked = arith == "h2"
    cells = [edge_cell(arith, d, e_rows, 11 + per_cu + over, in_blocked=blocked, out_blocked=blocked)]
    if v_rows:
        cells.append(vertex_cell(arith, d, v_rows, 13 + v_rows, in_blocked=blocked, out_blocked=blocked))
    p = plan(cells, d, cuda_device, arith)
    assert p.nw == nw and sum(t.tiles for t in p.tasks) == total, p
    assert p.tasks[0].mode == "resident"
    if v_rows:
        v = p.tasks[1]
        assert v.mode == "lockstep" and v.lock_tiles == nw and p.split == "fixed", p
        assert v.rounds == {1: 1, nw: 1, nw + 1: 2}[v_tiles] and v.blocks == v.rounds and v_rows % 16 == 1
        assert v.tiles - (v.rounds - 1) * nw == {1: 1, nw: nw, nw + 1: 1}[v_tiles]      # live wavefronts of the last round
    if arith == "h2":
        assert p.wt      # blocked states, messages: the loop's buffers, far below the footprint limit
    launch(arith, cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        check(c, cuda_device, "%s %d tiles nw=%d %s" % (what, total, nw, companion))


@pytest.mark.parametrize("companion", [False, True], ids=["alone", "beside_edges"])
@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("d", [32, 64])
def test_idle_lockstep_wavefronts_leave_the_range_guard_alone_h2(cuda_device, d, rounds, companion):
    """An idle wavefront of a lock-step round keeps z == 0 -- a variance of exactly 0, which the range guard ignores.  Were
    it to start from zscale[row] * zbias like a live one (its clamped row is the task's last), a folded bias of ordinary size
    for the model (|zbias| ~ 2^-8, far below [x | h] K) would be ALL of its z: a positive variance near 2^-16 < (2^-5)^2, bit
    1 of range_flag, and the model rerouted to bf16x3 with nothing failing.  The last round has one live wavefront of one row
    beside nw - 1 idle ones; the task's last row has degree 1."""
    n = cus(cuda_device)
    nw = 12 if companion else 4
    v_rows = 16 * nw * (rounds - 1) + 1
    cells = [vertex_cell("h2", d, v_rows, 140 + rounds, out_blocked=True, zbias_scale=2.0 ** -8)]
    if companion:
        cells.insert(0, edge_cell("h2", d, 16 * 8 * n + 100, 141, out_blocked=True, acts=None))
    p = plan(cells, d, cuda_device, "h2")
    v = p.tasks[-1]
    assert p.nw == nw and v.mode == "lockstep" and v.lock_tiles == nw and v.rounds == rounds, p._replace(tasks=None)
    assert v.tiles - (v.rounds - 1) * nw == 1 and float(cells[-1].zscale[-1]) == 1.0
    launch("h2", cells, d, cuda_device)
    for c in cells:
        check(c, cuda_device, "idle wavefronts, small zbias")


# ---------------------------------------------------------------------------------------------------------- the split
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("arith", ARITHS)
def test_fixed_share_beyond_half_the_grid_falls_back(cuda_device, arith, d):
    """100 edge rows beside 5000 vertex rows: one round of the vertex task would take nearly the whole grid, so
    split_blocks_fixed hands out the plain split by cost."""
    cells = [edge_cell(arith, d, 100, 5), vertex_cell(arith, d, 5000, 6)]
    p = plan(cells, d, cuda_device, arith)
    assert p.split == "plain" and p.tasks[1].mode == "lockstep" and p.tasks[0].blocks >= 1, p
    launch(arith, cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        check(c, cuda_device, what + " plain-split fallback")


def two_round_shape(d, n_cus):
    """The smallest (M, N) = (2 N, N), N a multiple of 1000 plus 1, at which launch_cell_h2 gives the vertex task two
    rounds per workgroup under the fixed split (at 256 CUs and d = 64: cost 22 * 6000 + 40 * 3000 > 960 * 256, N near
    48 000)."""
    for N in range(1001, 400000, 1000):
        p = cell_fwd_plan([cell_task(2 * N, 0, 3, False, True, True), cell_task(N, d, 4, True, True, True)], d, n_cus, "h2")
        if p.split == "fixed" and p.tasks[1].n_rounds >= 2:
            return 2 * N, N
    raise AssertionError("no two-round shape below 400 000 vertex rows")


@pytest.mark.parametrize("d", [32, 64])
def test_several_rounds_per_lockstep_workgroup_h2(cuda_device, d):
    """The n_rounds > 1 branch of the workgroup split, at the smallest two-task launch the plan query finds for this device (256
    CUs: 94 002 + 47 001 rows at either width -- which at d = 64 is already past the write-through footprint, at d = 32 not)."""
    M, N = two_round_shape(d, cus(cuda_device))
    cells = [edge_cell("h2", d, M, 21, in_blocked=True, out_blocked=True, acts=None),
             vertex_cell("h2", d, N, 22, in_blocked=True, out_blocked=True, acts=None)]
    p = plan(cells, d, cuda_device, "h2")
    v = p.tasks[1]
    assert p.split == "fixed" and p.nw == 12 and v.n_rounds >= 2 and v.rounds_per_wg[1] == v.n_rounds, p._replace(tasks=None)
    assert v.rounds_per_wg[0] >= 1
    print(" [two rounds: M = %d, N = %d, %d + %d workgroups, write-through %s]" % (M, N, p.tasks[0].blocks, v.blocks, p.wt))
    launch("h2", cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        check(c, cuda_device, what + " %d rounds" % v.n_rounds)


def test_footprint_beyond_the_infinity_cache_turns_write_through_off_h2(cuda_device):
    """2 x the launch's output bytes > 200 MiB (d = 64 with messages: more than 136 534 edge rows): the plain-store variant,
    although the launch writes blocked states and messages."""
    d, M, N = 64, 137001, 333
    cells = [edge_cell("h2", d, M, 31, in_blocked=True, out_blocked=True, acts=None),
             vertex_cell("h2", d, N, 32, in_blocked=True, out_blocked=True, acts=None)]
    p = plan(cells, d, cuda_device, "h2")
    assert not p.wt and not p.centered
    assert cell_fwd_plan([cell_task(136000, 0, 3, False, True, True)], d, cus(cuda_device), "h2").wt    # the limit's other side
    launch("h2", cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        check(c, cuda_device, what + " WT off")


@pytest.mark.parametrize("d", [32, 64])
def test_plain_cell_into_row_major_buffers_runs_without_write_through_h2(cuda_device, d):
    """No blocked state, no messages, no projection: nothing the next step's launch reads, so plain stores."""
    cells = [FwdCell("h2", d, 333, 41, dx=d), FwdCell("h2", d, 77, 42, mode="gather")]
    assert not plan(cells, d, cuda_device, "h2").wt
    launch("h2", cells, d, cuda_device)
    for c in cells:
        check(c, cuda_device, "row-major, WT off")


# ---------------------------------------------------------------------------------------------------- ticket coverage
@pytest.mark.parametrize("rem", [1, 2, 3, 4, 5, 6, 7, 0])
@pytest.mark.parametrize("d", [32, 64])
def test_resident_ticket_ranges_at_every_remainder_h2(cuda_device, d, rem):
    """A resident task alone on 24 + rem (rem = 0: 32) workgroups of 4 wavefronts: xcd_contiguous at every remainder mod 8.
    Every row must be written, and correctly."""
    blocks = 24 + (rem or 8)
    assert blocks <= cus(cuda_device)
    rows = 16 * (4 * blocks - 2) - 7
    cell = edge_cell("h2", d, rows, 50 + rem, out_blocked=True)
    p = plan([cell], d, cuda_device, "h2")
    t = p.tasks[0]
    assert t.mode == "resident" and p.nw == 4 and t.blocks == blocks and t.blocks % 8 == rem, p._replace(tasks=None)
    covered = sorted(t.ranges)
    assert covered[0][0] == 0 and covered[-1][1] == t.tiles and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    launch("h2", [cell], d, cuda_device)
    check(cell, cuda_device, "%d workgroups" % blocks)


# ------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("in_blocked,out_blocked", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("d", [32, 64])
def test_blocked_state_layouts_h2(cuda_device, d, in_blocked, out_blocked):
    """The four combinations of blocked input and output states, an edge and a vertex task in one launch; the pad rows of the
    blocked buffers and of the projected messages stay untouched (check)."""
    cells = [edge_cell("h2", d, 333, 61, in_blocked=in_blocked, out_blocked=out_blocked),
             vertex_cell("h2", d, 77, 62, in_blocked=in_blocked, out_blocked=out_blocked)]
    p = plan(cells, d, cuda_device, "h2")
    assert p.wt and [t.mode for t in p.tasks] == ["resident", "lockstep"]
    launch("h2", cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        check(c, cuda_device, "%s in %d out %d" % (what, in_blocked, out_blocked))


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("d", [32, 64])
def test_in_place_states_h2(cuda_device, d, blocked):
    """h_out == h and c_out == c (blocked both ways: the T-step loop's form): bit-equal to the out-of-place launch."""
    kw = dict(in_blocked=blocked, out_blocked=blocked)
    apart = [edge_cell("h2", d, 1501, 71, **kw), vertex_cell("h2", d, 205, 72, **kw)]
    place = [edge_cell("h2", d, 1501, 71, inplace=True, **kw), vertex_cell("h2", d, 205, 72, inplace=True, **kw)]
    assert plan(apart, d, cuda_device, "h2") == plan(place, d, cuda_device, "h2")
    launch("h2", apart, d, cuda_device)
    launch("h2", place, d, cuda_device)
    for a, b in zip(apart, place):
        assert b.h_out.data_ptr() != a.h_out.data_ptr()
        check(b, cuda_device, "in place")
        same_bits(a, b)


@pytest.mark.parametrize("d", [32, 64])
def test_null_c_is_a_zero_c_h2(cuda_device, d):
    zero = [edge_cell("h2", d, 333, 81), vertex_cell("h2", d, 77, 82)]
    null = [edge_cell("h2", d, 333, 81, null_c=True), vertex_cell("h2", d, 77, 82, null_c=True)]
    for c in zero:
        c.c[:] = 0.0
    launch("h2", zero, d, cuda_device)
    launch("h2", null, d, cuda_device)
    for a, b in zip(zero, null):
        check(b, cuda_device, "c == NULL")
        same_bits(a, b)


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("arith", ARITHS)
def test_projection_without_mlp_out(cuda_device, arith, d):
    cell = vertex_cell(arith, d, 333, 91, mlp_out=False, out_blocked=arith == "h2")
    assert plan([cell], d, cuda_device, arith).tasks[0].mode == "lockstep"
    launch(arith, [cell], d, cuda_device)
    assert cell.mlp_out is None and "proj" in cell.outputs() and "msg" not in cell.outputs()
    check(cell, cuda_device, "proj only")


# ----------------------------------------------------------------------------------------------------------- centring
@pytest.mark.parametrize("d", [32, 64])
def test_centred_launch_h2(cuda_device, d):
    """Every task promises z_centered (its K, projected messages and zbias centred per gate): the CENTERED variant, against
    the float64 cell of the same operands.  The range guard stays quiet."""
    cells = [edge_cell("h2", d, 1501, 101, out_blocked=True).centred(), vertex_cell("h2", d, 205, 102, out_blocked=True).centred(),
             FwdCell("h2", d, 333, 103, dx=d).centred()]
    p = plan(cells, d, cuda_device, "h2")
    assert p.centered and [t.mode for t in p.tasks] == ["resident", "lockstep", "resident"]
    launch("h2", cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex", "plain")):
        check(c, cuda_device, what + " centred")


@pytest.mark.parametrize("d", [32, 64])
def test_mixed_centred_launch_runs_uncentred_h2(cuda_device, d):
    """One centred task beside one that is not: the launcher must run the launch uncentred; both against float64.  (The
    centred task's bits alone and beside the other need not match: two variants of the LayerNorm.)"""
    cells = [edge_cell("h2", d, 1501, 111, out_blocked=True).centred(), vertex_cell("h2", d, 205, 112, out_blocked=True)]
    assert not plan(cells, d, cuda_device, "h2").centered
    launch("h2", cells, d, cuda_device)
    for c, what in zip(cells, ("edge centred", "vertex uncentred")):
        check(c, cuda_device, what + ", mixed launch")


# ------------------------------------------------------------------------------------------------------- independence
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("arith", ARITHS)
def test_a_task_alone_and_beside_a_companion_same_bits(cuda_device, arith, d):
    """The forward has no reduction across rows (the one-launch loops rely on it): the same launch twice gives the same
    bits, and a task's outputs do not depend on the wavefront count or the split a companion brings about."""
    blocked = arith == "h2"
    mk = lambda: [edge_cell(arith, d, 1501, 121, out_blocked=blocked), vertex_cell(arith, d, 205, 122, out_blocked=blocked)]
    first, again = mk(), mk()
    launch(arith, first, d, cuda_device)
    launch(arith, again, d, cuda_device)
    for a, b in zip(first, again):
        same_bits(a, b)
    n = cus(cuda_device)
    for k, what in ((0, "edge"), (1, "vertex")):
        alone = mk()[k]
        companion = FwdCell(arith, d, 16 * 8 * n + 100, 123, dx=0, mlp_layers=3)      # more than 8 CUs tiles: 12 wavefronts
        beside = [mk()[k], companion] if k == 0 else [companion, mk()[k]]
        pa, pb = plan([alone], d, cuda_device, arith), plan(beside, d, cuda_device, arith)
        assert (pa.nw, pb.nw) == (4, 12) and pa.tasks[0].blocks != pb.tasks[1 - (k == 0)].blocks, (pa, pb)
        launch(arith, [alone], d, cuda_device)
        launch(arith, beside, d, cuda_device)
        check(alone, cuda_device, what + " alone")
        same_bits(alone, beside[0 if k == 0 else 1])
        same_bits(alone, first[k])
        release()


# ------------------------------------------------------------------------------------------------ the plain MLP launch
def mlp_task(arith, d, rows, n_layers, mask, seed, device, proj=False, head=False):
    """-> (MlpTask, buffers {Y, acts, proj, y, flag}, float64 reference of the same names)."""
    rng = np.random.RandomState(seed)
    X = rng.randn(rows, d).astype(np.float32)
    layers = draw_mlp(rng, d, n_layers)
    P = (rng.randn(d, 4 * d) / np.sqrt(d)).astype(np.float32) if proj else None
    buf = {"Y": empty((rows + SPARE, d), device, SENTINEL),
           "acts": empty((max(n_layers - 1, 1), rows + SPARE, d), device, SENTINEL),
           "flag": torch.zeros(1, dtype=torch.int32, device=device)}
    if proj:
        buf["proj"] = empty(((pad16(rows) if arith == "h2" else rows) + SPARE, 4 * d), device, SENTINEL)
    task = _lib.MlpTask(_lib.ptr(dev(X, device)), _lib.ptr(mlp_blocks(arith, layers, device)), _lib.ptr(buf["Y"]),
                        _lib.ptr(buf["acts"]), (rows + SPARE) * d, rows, n_layers, mask,
                        _lib.ptr(packed(arith, P, device)) if proj else None, _lib.ptr(buf.get("proj")), _lib.ptr(buf["flag"]))
    outs = mlp64(t64(X, device), layers, mask, device)
    ref = {"Y": outs[-1]}
    if n_layers > 1:
        ref["acts"] = torch.stack(outs[:-1])
    if proj:
        ref["proj"] = outs[-1] @ t64(P, device)
    if head:
        hw, hb = (rng.randn(d, 1) / np.sqrt(d)).astype(np.float32), np.array([0.3], np.float32)
        buf["y"] = empty((rows + SPARE, 1), device, SENTINEL)
        buf["head"] = (dev(hw, device), dev(hb, device))
        ref["y"] = outs[-1] @ t64(hw, device) + 0.3
    return task, buf, ref


def check_mlp(arith, rows, buf, ref, what):
    got = {"Y": buf["Y"]}
    if "acts" in ref:
        got["acts"] = buf["acts"][:ref["acts"].shape[0]]
    if "proj" in ref:
        got["proj"] = blocked_unpack(buf["proj"]) / wscale("h2") if arith == "h2" else buf["proj"]
    if "y" in ref:
        got["y"] = buf["y"]
    whole, rowwise = {}, {}
    for n, t in got.items():
        raw = blocked_unpack(buf["proj"]) if (n == "proj" and arith == "h2") else t
        assert bool(raw[..., rows:, :].eq(SENTINEL).all()), n + ": written beyond the task's rows"
        a = t[..., :rows, :].reshape(-1, t.shape[-1]).cpu().numpy().astype(np.float64)
        b = ref[n].reshape(-1, ref[n].shape[-1]).cpu().numpy()
        whole[n] = rel_err(a, b)
        rowwise[n] = row_err(a, b) if n != "y" else whole[n]       # the head's one column: a row's own scale may be ~0
    print(" MLPFWD %s %s[%d rows] whole %s row %s" % (arith, what, rows, " ".join("%s %.1e" % kv for kv in whole.items()),
                                                      " ".join("%s %.1e" % kv for kv in rowwise.items())))
    assert int(buf["flag"].item()) == 0
    over = [("whole", n, e) for n, e in whole.items() if not e < TOL] + \
        [("row", n, e) for n, e in rowwise.items() if not e < ROW_TOL]
    assert not over, over


def mlp_rows(kind, n_cus):
    """Total tiles 4 CUs + 1 (the fewest that run 8 wavefronts) and 16 CUs (the most), the last tile partial."""
    return {"low": 16 * (4 * n_cus + 1) - 3, "high": 16 * 16 * n_cus - 3}[kind]


@pytest.mark.parametrize("kind", ["low", "high"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("arith", ARITHS)
def test_mlp_launch_at_eight_wavefronts(cuda_device, arith, d, kind):
    """One task with a projection, and two tasks (3 relu layers; 4 layers + projection) whose tiles sum to the same total."""
    n = cus(cuda_device)
    rows = mlp_rows(kind, n)
    assert mlp_fwd_plan([(rows, 4, True)], n).nw == 8
    task, buf, ref = mlp_task(arith, d, rows, 4, 0b0111, 200 + d, cuda_device, proj=True)
    _lib.call_multi("tspgnn_mlp_fwd_multi_" + arith, [task], d)
    torch.cuda.synchronize()
    check_mlp(arith, rows, buf, ref, "one task " + kind)
    release()
    rows_b = 16 * 40 + 1
    rows_a = rows - 16 * 41
    p = mlp_fwd_plan([(rows_a, 3, False), (rows_b, 4, True)], n)
    assert p.nw == 8 and sum(e - b for r in p.ranges for b, e in r) == (rows + 15) // 16
    ta, ba, ra = mlp_task(arith, d, rows_a, 3, 0b111, 201 + d, cuda_device)
    tb, bb, rb = mlp_task(arith, d, rows_b, 4, 0b0111, 202 + d, cuda_device, proj=True)
    _lib.call_multi("tspgnn_mlp_fwd_multi_" + arith, [ta, tb], d)
    torch.cuda.synchronize()
    check_mlp(arith, rows_a, ba, ra, "two tasks a " + kind)
    check_mlp(arith, rows_b, bb, rb, "two tasks b " + kind)


@pytest.mark.parametrize("kind", ["low", "high"])
@pytest.mark.parametrize("d", [32, 64])
def test_mlp_head_at_eight_wavefronts_h2(cuda_device, d, kind):
    n = cus(cuda_device)
    rows = mlp_rows(kind, n)
    assert mlp_fwd_plan([(rows, 3, False)], n).nw == 8
    task, buf, ref = mlp_task("h2", d, rows, 3, 0b111, 300 + d, cuda_device, head=True)
    hw, hb = buf["head"]
    _lib.call("tspgnn_mlp_head_fwd_h2", ctypes.cast(ctypes.pointer(task), ctypes.c_void_p), _lib.ptr(hw), _lib.ptr(hb),
              _lib.ptr(buf["y"]), d, None)
    torch.cuda.synchronize()
    check_mlp("h2", rows, buf, ref, "head " + kind)
