"""The fp32-MFMA forward, tspgnn_mlp_fwd_multi_f32 and tspgnn_lnlstm_fwd_multi_f32 (csrc/dense.hip: launch_mlp / mlp_fwd_kernel,
launch_lnlstm / lnlstm_fwd_kernel / lnlstm_fwd_chunked_kernel) -- the forward of every d = 128 and fp32-storage network, of
gemm="f32", and of whatever the split kernels decline -- and their one-task wrappers, called directly against float64 on the
device at the launches' own edges.

MLP: d 32, 64, 128 at every depth, relu masks 0, all, last layer only and inner layers only, from 1 row to both sides of the
4 / 8 and (d 32, 64) 8 / 16 wavefront thresholds with a one-row last tile; acts absent, dense and strided (the gap stays
SENTINEL), one layer with acts (nothing written); the projection phase, also on the small companion of a launch; 2, 3 and
4 tasks of very unequal rows and different depth, a task with fewer tiles than workgroups, an empty task in the middle.
Cell: the resident kernel in plain, gather-init (n_src = 37: every Zx row shared by many edges) and bias-init mode (zscale =
0 rows) up to the last input width that fits LDS at each d, from 1 row to both sides of the 4 / 8 wavefront threshold and a
deep task; the chunked kernel at the first width that does not fit, with a last chunk shorter than qc, a chunk that
straddles the x / h boundary, and round `CUs` of one live wavefront holding one row; the step's edge + vertex launch, four
tasks, a dropped empty task.  Bit claims: a task alone and beside a companion, the first R rows of a task and a task of
those R rows alone across every wavefront threshold, the one-task entries and the multi entry, and a resident and a
chunked run of the same rows (d = 64, dx = 80 against the same operands zero-padded to dx = 96: lstm_kloop adds the
k-steps of a tile into one MFMA accumulator chain in increasing order in both kernels -- a chunk boundary only restages
LDS -- and a zero block adds exact zeros, so the bits must agree, and the test asserts it).  Mixed launches: resident tasks
(gather-init and bias-init among them) together and only the tasks that do not fit chunked; a launch refused for a chunked
bias-init task leaves every buffer of every task untouched.

Every test that claims a branch asserts it through plan_replay.mlp_fwd_f32_plan / lstm_fwd_f32_plan with the device's CU
count BEFORE it launches.

Bars, all against float64: whole tensor rel_err < TOL = 5e-6 (the bar of test_gpu_split_kernels.py); row by row
lstm_bwd_cases.row_err < ROW_TOL = 2e-5 (the bar of the backward and forward edge suites).  Every check also finds every
row of the task written and nothing beyond them touched (16 spare rows, the other slot of a strided acts).  Each check
prints its worst ratios; the module prints the worst of all.

Measured on the MI355X (256 CUs), worst over all cases -- whole tensor: h' 7.4e-7, c' 8.5e-7 (17 % of the bar), MLP output
5.6e-7, saved activations 5.4e-7, projection 3.9e-7; row by row: h' 2.6e-6 (13 % of the bar), c' 1.8e-6, MLP output 9.8e-7,
activations 1.2e-6, projection 8.0e-7: rounding, so neither bar was raised.  The resident and the chunked run of the same
rows agreed bit for bit.  The whole file: 234 tests, 11 s, 0.8 GB peak device memory (the sibling
test_gpu_cell_forward_edges.py: 36 s, 1.8 GB).  DESIGN 2, "The fp32 forward launches at their own edges", also lists the
mutations the tests were weighed against."""
import time

import numpy as np
import pytest
import torch

from conftest import rel_err
from dense_fwd_cases import CellF32, MlpF32
from lstm_bwd_cases import release, row_err
from plan_replay import lstm_fwd_f32_plan, mlp_fwd_f32_plan, tiles16
from tspgnn import _lib

pytestmark = pytest.mark.gpu

TOL = 5e-6
ROW_TOL = 2e-5
MLP, CELL = "tspgnn_mlp_fwd_multi_f32", "tspgnn_lnlstm_fwd_multi_f32"
WORST = {}          # (kind, "whole" / "row", output) -> the worst ratio of all checks


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


@pytest.fixture(scope="module", autouse=True)
def _time_and_memory():
    t0 = time.time()
    yield
    if torch.cuda.is_available():
        print("\n[fp32 forward edges] worst %s" % " ".join("%s/%s/%s %.1e" % (k + (v,)) for k, v in sorted(WORST.items())))
        print("[fp32 forward edges] wall %.1f s, peak device memory %.0f MiB" % (
            time.time() - t0, torch.cuda.max_memory_allocated() / 2.0 ** 20))


def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def mlp_grid(d, device):
    """Workgroups of launch_mlp before its clamp: two per CU while four (d = 128: two) layers fit 80 KiB of LDS."""
    return cus(device) * (1 if d == 128 else 2)


def mlp_plan(tasks, d, device):
    return mlp_fwd_f32_plan([t.plan() for t in tasks], d, cus(device))


def cell_plan(cells, d, device):
    return lstm_fwd_f32_plan([c.plan() for c in cells], d, cus(device))


def launch(entry, cases, d, device):
    tasks = [c.task(device) for c in cases]
    _lib.call_multi(entry, tasks, d)
    torch.cuda.synchronize()


def check(case, device, what=""):
    """Every output of the launched task against float64 -- whole tensor at TOL, row by row at ROW_TOL -- every row written,
    nothing written beyond them.  Prints the worst ratios before it asserts."""
    kind = "mlp" if isinstance(case, MlpF32) else "cell"
    got, ref = case.outputs(), case.reference(device)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    whole, rowwise = {}, {}
    for n, a in got.items():
        a = a.reshape(-1, a.shape[-1]).cpu().numpy().astype(np.float64)
        b = ref[n].reshape(-1, ref[n].shape[-1]).cpu().numpy()
        whole[n], rowwise[n] = rel_err(a, b), row_err(a, b)
        for m, e in (("whole", whole[n]), ("row", rowwise[n])):
            WORST[(kind, m, n)] = max(WORST.get((kind, m, n), 0.0), e)
    print(" F32FWD %s d=%d %s[%d rows] whole %s row %s" % (
        kind, case.d, what, case.rows, " ".join("%s %.1e" % kv for kv in whole.items()),
        " ".join("%s %.1e" % kv for kv in rowwise.items())))
    assert not case.unwritten(), ("rows left unwritten", case.unwritten())
    assert not case.untouched(), ("written beyond the task's rows", case.untouched())
    over = [("whole", n, e) for n, e in whole.items() if not e < TOL] + \
        [("row", n, e) for n, e in rowwise.items() if not e < ROW_TOL]
    assert not over, over      # every measure that misses its bar, not only the first


def same_bits(a, b, rows=None):
    """The outputs of b equal, bit for bit, those of a (rows: the first `rows` rows of a)."""
    ga, gb = a.outputs(), b.outputs()
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert torch.equal(ga[n] if rows is None else ga[n][..., :rows, :], gb[n]), n


# =============================================================================================================== MLP
def masks(L):
    """No relu, every layer, the last layer only, the inner layers only."""
    return sorted({0, (1 << L) - 1, 1 << (L - 1), (1 << (L - 1)) - 1})


DEPTHS = [(d, L) for d in (32, 64, 128) for L in ((1, 2) if d == 128 else (1, 2, 3, 4))]


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 333])
@pytest.mark.parametrize("d,L", DEPTHS)
def test_mlp_every_depth_mask_and_acts_vs_float64(cuda_device, d, L, rows):
    """One task alone on four wavefronts, at every relu mask of masks(L) -- a bit on the last layer together with acts
    among them -- with acts absent, dense and strided; with one layer, acts must stay untouched."""
    assert mlp_fwd_f32_plan([(rows, L, False)], d, cus(cuda_device)).nw == 4
    for mask in masks(L):
        for acts in (None, "dense", "strided"):
            t = MlpF32(d, rows, 1000 * d + 10 * rows + L, n_layers=L, relu_mask=mask, acts=acts)
            launch(MLP, [t], d, cuda_device)
            assert ("acts" in t.outputs()) == (acts is not None and L > 1)
            check(t, cuda_device, "L=%d mask=%d acts=%s" % (L, mask, acts))
        release()


@pytest.mark.parametrize("d,per_grid", [(32, 4), (32, 16), (64, 4), (64, 16), (128, 4)])
def test_mlp_wavefront_thresholds_and_the_same_bits_either_side(cuda_device, d, per_grid):
    """rows = 16 * per_grid * grid: the last launch on 4 (8) wavefronts; one row more -- a last tile of one row -- the first
    on 8 (16).  Both against float64, and the first rows of the larger task equal, bit for bit, the smaller one."""
    rows = 16 * per_grid * mlp_grid(d, cuda_device)
    L = 2
    big = MlpF32(d, rows + 1, 31 * d + per_grid, n_layers=L, relu_mask=0b10, acts="dense")
    small = big.head(rows)
    nws = {4: (4, 8), 16: (8, 16)}[per_grid]
    assert (mlp_plan([small], d, cuda_device).nw, mlp_plan([big], d, cuda_device).nw) == nws
    assert tiles16(big.rows) == tiles16(small.rows) + 1
    launch(MLP, [small], d, cuda_device)
    launch(MLP, [big], d, cuda_device)
    check(small, cuda_device, "nw=%d" % nws[0])
    check(big, cuda_device, "nw=%d" % nws[1])
    same_bits(big, small, rows)


@pytest.mark.parametrize("rows", [1, 17, 333, "over_four"])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("d", [32, 64])
def test_mlp_projection_vs_float64(cuda_device, d, L, rows):
    """The second phase (LDS restaged behind a barrier, the ticket reset, a second loop over the workgroup's tiles), on 4
    wavefronts and -- one tile past 4 per workgroup -- on 8; proj_out against float64 Y64 P64."""
    rows = rows if isinstance(rows, int) else 16 * 4 * mlp_grid(d, cuda_device) + 1
    t = MlpF32(d, rows, 77 * d + L + rows, n_layers=L, relu_mask=(1 << (L - 1)) - 1, acts="strided", proj=True)
    assert mlp_plan([t], d, cuda_device).nw == (4 if rows <= 333 else 8)
    launch(MLP, [t], d, cuda_device)
    assert "proj" in t.outputs()
    check(t, cuda_device, "L=%d proj" % L)


def unequal_tasks(d, n, proj_ok):
    """n tasks of very unequal rows and different depth; the second is a one-row task, a projected one where d allows."""
    deep = 2 if d == 128 else 4
    tasks = [MlpF32(d, 40000, 500 + d, n_layers=2, acts="dense"),
             MlpF32(d, 1, 501 + d, n_layers=deep, relu_mask=0, proj=proj_ok, acts="strided"),
             MlpF32(d, 333, 502 + d, n_layers=1, acts="dense"),
             MlpF32(d, 4001, 503 + d, n_layers=deep - 1, relu_mask=1)]
    return tasks[:n]


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_mlp_unequal_tasks_in_one_launch(cuda_device, d, n):
    """1 row (projected, where d allows: the projection on the small companion) beside 40 000, then 333 rows of one layer
    and 4001 of another depth: every task gets at least one workgroup and its own tile range, and every task's bits equal
    those of the task launched alone."""
    tasks = unequal_tasks(d, n, d != 128)
    p = mlp_plan(tasks, d, cuda_device)
    assert len(p.blocks) == n and min(p.blocks) >= 1 and p.blocks[1] == 1, p.blocks
    for t, ranges in zip(tasks, p.ranges):
        assert ranges[0][0] == 0 and ranges[-1][1] == tiles16(t.rows) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    launch(MLP, tasks, d, cuda_device)
    for k, t in enumerate(tasks):
        check(t, cuda_device, "task %d of %d" % (k, n))
    for k in (1, n - 1):
        alone = unequal_tasks(d, n, d != 128)[k]
        assert mlp_plan([alone], d, cuda_device).nw != p.nw or mlp_plan([alone], d, cuda_device).blocks != [p.blocks[k]]
        launch(MLP, [alone], d, cuda_device)
        same_bits(tasks[k], alone)


@pytest.mark.parametrize("d", [32, 64])
def test_mlp_task_with_fewer_tiles_than_workgroups(cuda_device, d):
    """A projected one-layer task of 2 tiles beside 40 tiles of one plain layer: priced at six times its tiles it is handed
    more workgroups than it has tiles, so some of them own an empty range [t, t) -- in both phases."""
    small, large = MlpF32(d, 32, 610 + d, n_layers=1, proj=True), MlpF32(d, 16 * 40 - 3, 611 + d, n_layers=1)
    p = mlp_plan([small, large], d, cuda_device)
    assert p.blocks[0] > tiles16(small.rows) and any(b == e for b, e in p.ranges[0]), p
    launch(MLP, [small, large], d, cuda_device)
    check(small, cuda_device, "2 tiles on %d workgroups" % p.blocks[0])
    check(large, cuda_device, "companion")


@pytest.mark.parametrize("d", [32, 64, 128])
def test_mlp_empty_task_in_the_middle_is_dropped(cuda_device, d):
    """rows = 0 between two live tasks: filter_live drops it, and the launch equals the launch of the other two."""
    mk = lambda: [MlpF32(d, 5000, 700 + d, n_layers=2, acts="dense"), MlpF32(d, 0, 701 + d, n_layers=1, acts="dense"),
                  MlpF32(d, 77, 702 + d, n_layers=1, proj=d != 128)]
    three, two = mk(), [t for t in mk() if t.rows]
    assert mlp_plan(three, d, cuda_device) == mlp_plan(two, d, cuda_device) and len(mlp_plan(three, d, cuda_device).blocks) == 2
    launch(MLP, three, d, cuda_device)
    launch(MLP, two, d, cuda_device)
    assert three[1].all_sentinel()
    for a, b in zip([three[0], three[2]], two):
        check(a, cuda_device, "beside an empty task")
        same_bits(a, b)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_mlp_one_task_entry_equals_the_multi_entry(cuda_device, d):
    L = 2 if d == 128 else 3
    a, b = (MlpF32(d, 1501, 800 + d, n_layers=L, relu_mask=0b101, acts="strided") for _ in range(2))
    launch(MLP, [a], d, cuda_device)
    f = _lib.ptrs(b.fields(cuda_device))
    _lib.call("tspgnn_mlp_fwd_f32", f["X"], f["wb"], f["Y"], f["acts"], f["acts_stride"], b.rows, d, L, b.mask, None)
    torch.cuda.synchronize()
    check(b, cuda_device, "tspgnn_mlp_fwd_f32")
    same_bits(a, b)


# ============================================================================================================== cell
RESIDENT = [(32, 0, "plain"), (32, 16, "plain"), (32, 272, "plain"), (64, 0, "plain"), (64, 64, "plain"), (64, 80, "plain"),
            (32, 0, "gather"), (64, 0, "gather"), (32, 32, "bias"), (64, 64, "bias")]
CHUNKED = {(32, 288): [16, 4], (64, 96): [8, 2], (64, 192): [8, 8], (128, 0): [4, 4], (128, 32): [4, 4, 2], (128, 128): [4, 4, 4, 4]}
"""(d, dx) -> the stagings of K in 16-row blocks: (128, 32) ends on a chunk shorter than qc; at (64, 96) (blocks 0-5 are x)
and (128, 32) (blocks 0-1) a chunk straddles the x / h boundary."""
N_SRC = 37


def rows_deep(device):
    """Alone at 8 wavefronts: every wavefront takes two or three tiles and the last tile holds one row (65 537 rows on 256
    CUs)."""
    return 16 * (8 * 2 * cus(device)) + 1


def resident_rows(kind, device):
    n = cus(device)
    return {"four_per_cu": 16 * 4 * n, "four_per_cu+1": 16 * 4 * n + 1, "deep": rows_deep(device)}.get(kind, kind)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 333, "four_per_cu", "four_per_cu+1", "deep"])
@pytest.mark.parametrize("d,dx,mode", RESIDENT)
def test_resident_cell_vs_float64(cuda_device, d, dx, mode, rows):
    """One task alone in lnlstm_fwd_kernel: 4 wavefronts up to 4 tiles per CU, 8 beyond; at "deep" every wavefront takes two
    or three tiles."""
    seed = 13 * d + dx + (rows if isinstance(rows, int) else len(rows))
    rows = resident_rows(rows, cuda_device)
    cell = CellF32(d, rows, seed, dx=dx, mode=mode, n_src=N_SRC)
    p = cell_plan([cell], d, cuda_device)
    assert p.chunked == [False] and p.qc == [(dx + d) // 16] and p.nw == (4 if tiles16(rows) <= 4 * cus(cuda_device) else 8), p
    assert p.ranges[0][0][0] == 0 and p.ranges[0][-1][1] == tiles16(rows)
    if rows == rows_deep(cuda_device):
        share = [e - b for b, e in p.ranges[0]]
        assert min(share) // 8 >= 2 and -(-max(share) // 8) == 3 and rows % 16 == 1, (min(share), max(share))
    launch(CELL, [cell], d, cuda_device)
    check(cell, cuda_device, "%s dx=%d" % (mode, dx))


@pytest.mark.parametrize("rows", [1, 17, 127, 128, 129, "round_per_cu", "round_per_cu+1"])
@pytest.mark.parametrize("d,dx", sorted(CHUNKED))
def test_chunked_cell_vs_float64(cuda_device, d, dx, rows):
    """One task alone in lnlstm_fwd_chunked_kernel.  16 * 8 * CUs rows: one round per workgroup; one row more: round `CUs`
    exists, workgroup 0 strides to it, and its one live wavefront holds one valid row."""
    n = cus(cuda_device)
    seed = 17 * d + dx + (rows if isinstance(rows, int) else len(rows))
    rows = {"round_per_cu": 16 * 8 * n, "round_per_cu+1": 16 * 8 * n + 1}.get(rows, rows)
    cell = CellF32(d, rows, seed, dx=dx)
    p = cell_plan([cell], d, cuda_device)
    assert p.chunked == [True] and p.grid == 0 and p.chunks[0] == CHUNKED[(d, dx)] and p.qc[0] == CHUNKED[(d, dx)][0], p
    rounds = -(-tiles16(rows) // 8)
    assert p.chunk_grid[0] == min(n, rounds) and p.rounds_per_wg[0] == ((1, 2) if rounds > n else (1, 1))
    if rows == 16 * 8 * n + 1:
        assert rounds == n + 1 and tiles16(rows) - 8 * n == 1 and rows % 16 == 1
    launch(CELL, [cell], d, cuda_device)
    check(cell, cuda_device, "chunked dx=%d" % dx)


def step_cells(d, M, N):
    """The step's launch: the edge task (gather-init) and the vertex task (bias-init on [x | h], dx = d)."""
    return [CellF32(d, M, 900 + d, mode="gather", n_src=N), CellF32(d, N, 901 + d, dx=d, mode="bias")]


@pytest.mark.parametrize("M,N", [(7001, 333), (100, 5000), (1, 40000)])
@pytest.mark.parametrize("d", [32, 64])
def test_edge_and_vertex_tasks_in_one_launch(cuda_device, d, M, N):
    """As the training step launches them, at three very different splits of the workgroups; each task's bits equal those of
    the task launched alone."""
    cells = step_cells(d, M, N)
    p = cell_plan(cells, d, cuda_device)
    assert p.chunked == [False, False] and min(p.blocks) >= 1 and sum(p.blocks) == p.grid, p
    launch(CELL, cells, d, cuda_device)
    for c, what in zip(cells, ("edge", "vertex")):
        check(c, cuda_device, what + " of a step")
    for k in (0, 1):
        alone = step_cells(d, M, N)[k]
        launch(CELL, [alone], d, cuda_device)
        same_bits(cells[k], alone)


@pytest.mark.parametrize("d", [32, 64])
def test_four_cell_tasks_and_a_dropped_empty_one(cuda_device, d):
    """Four tasks of every mode and unequal rows in one resident launch; then the same with an empty task in the middle in
    place of the third: three live tasks, planned and computed as those three alone."""
    mk = lambda: [CellF32(d, 2000, 910 + d, dx=d), CellF32(d, 40000, 911 + d, mode="gather", n_src=N_SRC),
                  CellF32(d, 1, 912 + d, dx=16), CellF32(d, 300, 913 + d, dx=32, mode="bias")]
    four = mk()
    p = cell_plan(four, d, cuda_device)
    assert p.nw == 8 and not any(p.chunked) and min(p.blocks) >= 1 and p.blocks[2] == 1, p
    launch(CELL, four, d, cuda_device)
    for k, c in enumerate(four):
        check(c, cuda_device, "task %d of 4" % k)
    release()
    hole = mk()
    hole[2] = CellF32(d, 0, 912 + d, dx=16)
    three = [c for c in mk() if c.rows != 1]
    assert cell_plan(hole, d, cuda_device) == cell_plan(three, d, cuda_device)
    launch(CELL, hole, d, cuda_device)
    launch(CELL, three, d, cuda_device)
    assert hole[2].all_sentinel()
    for a, b in zip([hole[0], hole[1], hole[3]], three):
        check(a, cuda_device, "beside an empty task")
        same_bits(a, b)


@pytest.mark.parametrize("d,dx,mode", [(32, 0, "gather"), (64, 64, "bias"), (64, 80, "plain")])
def test_cell_rows_do_not_depend_on_the_wavefront_count(cuda_device, d, dx, mode):
    """16 * 4 * CUs rows run on 4 wavefronts, one row more on 8: the first rows of the larger task equal, bit for bit, the
    smaller one."""
    rows = 16 * 4 * cus(cuda_device)
    big = CellF32(d, rows + 1, 920 + d + dx, dx=dx, mode=mode, n_src=N_SRC)
    small = big.head(rows)
    assert (cell_plan([small], d, cuda_device).nw, cell_plan([big], d, cuda_device).nw) == (4, 8)
    launch(CELL, [small], d, cuda_device)
    launch(CELL, [big], d, cuda_device)
    check(small, cuda_device, "nw=4")
    same_bits(big, small, rows)


@pytest.mark.parametrize("d,dx", [(64, 64), (64, 192), (128, 32)])
def test_lnlstm_fwd_entry_equals_the_multi_entry(cuda_device, d, dx):
    a, b = (CellF32(d, 1501, 930 + d + dx, dx=dx) for _ in range(2))
    launch(CELL, [a], d, cuda_device)
    f = _lib.ptrs(b.fields(cuda_device))
    _lib.call("tspgnn_lnlstm_fwd_f32", f["x"], dx, f["h"], f["c"], f["K"], f["ln"], f["h_out"], f["c_out"], b.rows, d, None)
    torch.cuda.synchronize()
    check(b, cuda_device, "tspgnn_lnlstm_fwd_f32 dx=%d" % dx)
    same_bits(a, b)


@pytest.mark.parametrize("d", [32, 64])
def test_lnlstm_gather_fwd_entry_equals_the_multi_entry(cuda_device, d):
    a, b = (CellF32(d, 1501, 940 + d, mode="gather", n_src=N_SRC) for _ in range(2))
    launch(CELL, [a], d, cuda_device)
    f = _lib.ptrs(b.fields(cuda_device))
    _lib.call("tspgnn_lnlstm_gather_fwd_f32", f["uv"], f["Zx"], f["h"], f["c"], f["K"], f["ln"], f["h_out"], f["c_out"],
              b.rows, N_SRC, d, None)
    torch.cuda.synchronize()
    check(b, cuda_device, "tspgnn_lnlstm_gather_fwd_f32")
    same_bits(a, b)


@pytest.mark.parametrize("rows", [333, "round_per_cu+1"])
def test_resident_and_chunked_runs_of_the_same_rows_same_bits(cuda_device, rows):
    """d = 64, dx = 80 (resident) against the same operands zero-padded to dx = 96 (chunked, 8 + 2 blocks).  Both kernels add
    a tile's k-steps into one accumulator chain in increasing order and start it at zero; the padding block adds exact
    zeros: the same bits, by lstm_kloop's order."""
    rows = rows if isinstance(rows, int) else 16 * 8 * cus(cuda_device) + 1
    res = CellF32(64, rows, 950, dx=80)
    chk = res.padded(96)
    assert cell_plan([res], 64, cuda_device).chunked == [False] and cell_plan([chk], 64, cuda_device).chunked == [True]
    launch(CELL, [res], 64, cuda_device)
    launch(CELL, [chk], 64, cuda_device)
    check(res, cuda_device, "resident dx=80")
    check(chk, cuda_device, "chunked dx=80+16")
    same = all(torch.equal(a, b) for a, b in zip(res.outputs().values(), chk.outputs().values()))
    print(" F32FWD resident and chunked runs of the same rows agree bit for bit: %s" % same)
    same_bits(res, chk)


# ------------------------------------------------------------------------- launches whose tasks do not all fit LDS
MIXED = {"gather+chunked": lambda: [CellF32(64, 7001, 960, mode="gather", n_src=N_SRC), CellF32(64, 333, 961, dx=192)],
         "chunked+bias": lambda: [CellF32(64, 333, 962, dx=96), CellF32(64, 7001, 963, dx=64, mode="bias")]}


@pytest.mark.parametrize("which", sorted(MIXED))
def test_mixed_launch_runs_the_fitting_tasks_resident(cuda_device, which):
    """[gather dx = 0, plain dx = 192] and [plain dx = 96, bias-init dx = 64] at d = 64: the fitting task -- gather-init,
    bias-init -- in the resident launch, only the other one chunked; the fitting task's bits equal those of the task alone."""
    cells = MIXED[which]()
    fit = 0 if which == "gather+chunked" else 1
    p = cell_plan(cells, 64, cuda_device)
    assert p.chunked == [k != fit for k in (0, 1)] and p.blocks[1 - fit] == 0 and p.blocks[fit] == p.grid > 0, p
    launch(CELL, cells, 64, cuda_device)
    for c in cells:
        check(c, cuda_device, which)
    alone = MIXED[which]()[fit]
    assert cell_plan([alone], 64, cuda_device).blocks == [p.blocks[fit]]
    launch(CELL, [alone], 64, cuda_device)
    same_bits(cells[fit], alone)


REFUSED = {"d=64 bias dx=192": (64, lambda: [CellF32(64, 333, 970, dx=192), CellF32(64, 77, 971, dx=192, mode="bias")], -2),
           "d=128 bias dx=128": (128, lambda: [CellF32(128, 333, 972, dx=192), CellF32(128, 77, 973, dx=128, mode="bias")], -2),
           "d=64 bias first": (64, lambda: [CellF32(64, 77, 974, dx=96, mode="bias"), CellF32(64, 333, 975, mode="gather")], -2),
           "d=128 gather": (128, lambda: [CellF32(128, 333, 976, dx=192), CellF32(128, 77, 977, mode="gather")], -1)}


@pytest.mark.parametrize("which", sorted(REFUSED))
def test_refused_launch_writes_nothing(cuda_device, which):
    """A chunked task that could run, then a gather-init or bias-init task whose K does not fit LDS (a gather-init task at
    d = 128 -- the only width at which its K[d, 4d] does not fit -- is turned away by the entry's validation, TSPGNN_EINVAL;
    a bias-init one by the plan, TSPGNN_EUNSUPPORTED): the verdict comes before anything is launched, and every output
    buffer of every task is still all SENTINEL."""
    d, mk, status = REFUSED[which]
    cells = mk()
    if status == -2:
        with pytest.raises(ValueError):
            cell_plan(cells, d, cuda_device)
    tasks = [c.task(cuda_device) for c in cells]
    with pytest.raises(_lib.TspgnnError) as e:
        _lib.call_multi(CELL, tasks, d)
    torch.cuda.synchronize()
    assert e.value.status == status, e.value
    if status == -2:
        assert e.value.message == "lnlstm_fwd: gather-init / zbias need K[%d,%d] resident in LDS" % (d, 4 * d)
    assert all(c.all_sentinel() for c in cells), [c.all_sentinel() for c in cells]
