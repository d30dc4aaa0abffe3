"""The default arithmetic's LN-LSTM cell backward, tspgnn_lnlstm_bwd_multi_h2 (csrc/dense_bwd_h2.hip), and through the same
cases the fp32-MFMA one, tspgnn_lnlstm_bwd_multi_f32 (csrc/dense_bwd.hip), called directly against float64 autograd on the
device -- at the kernels' own edges: every mode (plain, gather-init, bias-init, the fused data gradients KT and KTg), 1 row
to ROWS_DEEP = 16 * 17 * CUs + 1 rows, where a single-task launch gives every wavefront two or three tiles (so the f16x2
kernel's software pipeline runs in its steady state, and its last, prefetched tile holds one row) and the fp32 kernel's
chunked-K path runs several rounds with dead tiles in the last.  Every test that claims such a depth asserts it through
lstm_bwd_cases.tiles_per_wavefront, which walks the launcher's own plan (tspgnn_plan_cell_bwd).

Bars, all against float64: whole tensor rel_err < TOL = 5e-6 (the bar of test_gpu_backward_kernels.py and the bf16 file);
row by row, max |got - ref| over a row by max |ref| over that row < ROW_TOL = 2e-5 (the bar of
test_lnlstm_gather_backward_h2_fused_dh) -- the measure that shows a wrong prefetched tile, a wrong row exponent or a
misplaced zscale among rows of larger scale; rows whose reference is all zero must be exactly zero.  Every check also finds
the 16 spare rows behind each output untouched.  Each test prints its worst ratios.

Measured on the MI355X (256 CUs), worst over all cases, f16x2 / fp32 -- whole tensor: dz 3.5e-7 / 4.6e-7, dc_in 2.3e-7 /
3.7e-7, ln_grad 3.4e-7 / 4.2e-7, dxh 4.6e-7 / 7.6e-7, dxg 3.6e-7 / --; row by row: dz 1.2e-6 / 1.3e-6, dc_in 6.9e-7 / 1.1e-6,
dxh 9.0e-7 / 1.9e-6, dxg 8.4e-7 / --.  The worst at ROWS_DEEP alone are within a factor of three of those at 1 ... 333 rows
(the row-wise maximum grows with the number of rows it is taken over), and spreading the rows' gradients over twelve decades
leaves them where they were: rounding, evenly spread, a tenth of either bar, so neither bar was raised.  The 2^-16 band of
quiet_kinks sufficed for the f16x2 recomputation of z; it quietened at most 0.36 % of the deep rows, and 2 of 333."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
from lstm_bwd_cases import (SENTINEL, Cell, dev, empty, k_resident_f32, plan_of, release, row_err, tiles_per_wavefront,
                            workspace)
from tspgnn import _lib

pytestmark = pytest.mark.gpu

TOL = 5e-6
ROW_TOL = 2e-5
ENTRY = {"h2": "tspgnn_lnlstm_bwd_multi_h2", "f32": "tspgnn_lnlstm_bwd_multi_f32"}
ROWS_SMALL = [1, 15, 16, 17, 333]
ROWS = ROWS_SMALL + ["deep"]                # "deep": ROWS_DEEP, known once the device is
ROWS_SPREAD = ROWS + ["deep_spread"]        # ... and once more with the rows' gradients spread over twelve decades


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def rows_of(rows, device):
    """A parametrised row count -> (rows, row_spread)."""
    if isinstance(rows, int):
        return rows, False
    return 16 * 17 * cus(device) + 1, rows == "deep_spread"      # ROWS_DEEP: 69 633 on 256 CUs


def assert_deep(cells, d, device, arith):
    """Every task of the launch gives each of its wavefronts at least two tiles, and some three."""
    for plan in tiles_per_wavefront([c.plan() for c in cells], d, cus(device), arith):
        if plan is not None:
            nw, blocks, lo, hi = plan
            assert lo >= 2 and hi >= 3, plan


def launch(arith, cells, d, device, **kw):
    _lib.call_multi(ENTRY[arith], [c.task(device, **kw) for c in cells], d)
    torch.cuda.synchronize()


def check(cell, device, what=""):
    """Every output of the launched cell against float64: whole tensor at TOL, row by row at ROW_TOL; the spare rows
    untouched.  Prints the worst ratios before it asserts."""
    got = cell.named_outputs()
    assert cell.untouched(), "rows beyond the task's were written"
    if cell.dh is None:     # no incoming gradient: every output is exactly zero
        for name, a in got.items():
            assert not a.any(), name
        return
    ref = cell.reference(device)
    whole = {n: rel_err(a, ref[n]) for n, a in got.items()}
    rowwise = {n: row_err(a, ref[n]) for n, a in got.items() if n != "ln_grad"}
    print(" %s[%d rows, %d quiet] whole %s row %s" % (
        what, cell.rows, cell.quietened, " ".join("%s %.1e" % kv for kv in whole.items()),
        " ".join("%s %.1e" % kv for kv in rowwise.items())), end="")
    over = [("whole", n, e) for n, e in whole.items() if not e < TOL] + \
        [("row", n, e) for n, e in rowwise.items() if not e < ROW_TOL]
    assert not over, over      # every measure that misses its bar, not only the first


def same_bits(a, b, names=("dz", "dc_in", "dxh", "dxg")):
    ga, gb = a.named_outputs(), b.named_outputs()
    for n in names:
        if n in ga or n in gb:
            assert np.array_equal(ga[n], gb[n]), n
    return ga, gb


H2_PLAIN = [(32, 32), (32, 64), (32, 256), (64, 0), (64, 32), (64, 64)]      # all that fits LDS (dx a multiple of 32)
F32_CHUNKED = [(128, 32), (128, 128), (64, 192)]                             # K streamed through LDS
PLAIN = [("h2",) + s for s in H2_PLAIN] + [("f32",) + s for s in H2_PLAIN + F32_CHUNKED]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("arith,d,dx", PLAIN)
def test_lnlstm_bwd_plain_vs_float64(cuda_device, arith, d, dx, rows):
    """Plain mode, z = [x | h] K: dz, dc_in and the LayerNorm gradients.  fp32 at (128, 32), (128, 128) and (64, 192) streams K
    in chunks: rounds of nw tiles, with dead tiles in the last round at every row count here but 16 * nw * k."""
    if arith == "f32":
        assert k_resident_f32(d, dx) == ((d, dx) not in F32_CHUNKED)
    seed = d * 7 + dx + (rows if isinstance(rows, int) else 70001)
    rows, _ = rows_of(rows, cuda_device)
    cell = Cell(arith, d, dx, rows, seed=seed)
    if rows > 333:
        assert_deep([cell], d, cuda_device, arith)
    launch(arith, [cell], d, cuda_device)
    check(cell, cuda_device)


@pytest.mark.parametrize("rows", ROWS_SPREAD)
@pytest.mark.parametrize("arith,d,fused", [(a, d, f) for a in ("h2", "f32") for d, f in ((32, False), (64, False), (64, True))])
def test_lnlstm_bwd_gather_init_vs_float64(cuda_device, arith, d, fused, rows):
    """Gather-init mode, z = Zx[u] + Zx[v] + h Kh; with KT, the fused dxh = dz Kh^T against autograd's d/dh.  At ROWS_DEEP
    the f16x2 kernel fetches the next tile's endpoints, h rows and projected messages inside the current tile (behind the
    KT k-blocks with KT, after the tile without), and its last tile, of one row, arrives prefetched."""
    if arith == "f32":
        assert k_resident_f32(d, 0, with_KT=fused)
    seed = d + (rows if isinstance(rows, int) else 70001) + fused
    rows, spread = rows_of(rows, cuda_device)
    cell = Cell(arith, d, 0, rows, seed=seed, gather=True, fused=fused, row_spread=spread)
    if rows > 333:
        assert_deep([cell], d, cuda_device, arith)
    launch(arith, [cell], d, cuda_device)
    check(cell, cuda_device)


@pytest.mark.parametrize("rows", ROWS_SPREAD)
@pytest.mark.parametrize("d,dx,fused", [(64, 64, True), (32, 32, False)])
def test_lnlstm_bwd_h2_bias_init_vs_float64(cuda_device, d, dx, fused, rows):
    """Bias-init mode (f16x2 only), z = zscale[row] zbias + [x | h] K, as the pushed vertex cell runs it; at d = dx = 64
    with KTg, the second phase's dxg | dxh = dz K^T against autograd's d/dx | d/dh."""
    seed = d + dx + (rows if isinstance(rows, int) else 70001)
    rows, spread = rows_of(rows, cuda_device)
    cell = Cell("h2", d, dx, rows, seed=seed, bias_init=True, fused=fused, row_spread=spread)
    if rows > 333:
        assert_deep([cell], d, cuda_device, "h2")
    launch("h2", [cell], d, cuda_device)
    check(cell, cuda_device)


def step_cells(arith, rows_v, rows_e, n_tasks, seed=11):
    """The training step's launch at d = 64: a vertex-style task (f16x2: bias-init with KTg; fp32: plain), an edge-style
    task (gather-init with KT) and, with three, an empty one."""
    vertex = dict(dx=64, bias_init=True, fused=True) if arith == "h2" else dict(dx=64)
    specs = [dict(rows=rows_v, **vertex), dict(rows=rows_e, dx=0, gather=True, fused=True)] + \
        ([dict(rows=0, dx=64)] if n_tasks == 3 else [])
    return [Cell(arith, 64, s.pop("dx"), s.pop("rows"), seed=seed + i, **s) for i, s in enumerate(specs)]


def step_plans(arith, rows_v, rows_e):
    """Cell.plan() of step_cells' two live tasks, without drawing them (the test asserts that it is)."""
    return [plan_of(rows_v, 64, fused=arith == "h2"), plan_of(rows_e, 0, gather=True, fused=True)]


def step_rows(arith, n_cus):
    """Beside 12 801 vertex rows, the smallest edge row count 16 k + 1 >= 70 001 at which tiles_per_wavefront reports two to
    three tiles per wavefront for BOTH tasks (the tasks share the grid by cost; on 256 CUs 70 001 edge rows leave the
    f16x2 vertex task's wavefronts one to two tiles).  Only the edge count is searched: the vertex count stays at 12 801,
    so the pair is the smallest in the edge count alone.  256 CUs: 70 769 edge rows for f16x2, 70 001 for fp32; 304 CUs:
    87 297 and 85 777."""
    rows_v = 12801
    for rows_e in range(70001, 200000, 16):
        plans = tiles_per_wavefront(step_plans(arith, rows_v, rows_e), 64, n_cus, arith)
        if all(lo >= 2 and hi >= 3 for _, _, lo, hi in plans):
            return rows_v, rows_e
    raise AssertionError("no row counts reach two to three tiles per wavefront in both tasks on %d CUs" % n_cus)


@pytest.mark.parametrize("n_tasks", [2, 3])
@pytest.mark.parametrize("arith", ["h2", "f32"])
def test_lnlstm_bwd_step_launch_equals_separate_launches(cuda_device, arith, n_tasks):
    """The vertex-style and the edge-style task in ONE launch, each wavefront of either with two to three tiles and neither
    row count a multiple of 16: dz, dc_in, dxh, dxg bit for bit those of separate launches; the LayerNorm gradients are sums
    over the task's share of the workgroups, which the table changes: they agree to fp32 rounding.  Each against float64."""
    rows_v, rows_e = step_rows(arith, cus(cuda_device))
    assert rows_v % 16 and rows_e % 16
    together, apart = (step_cells(arith, rows_v, rows_e, n_tasks) for _ in range(2))
    assert [c.plan() for c in together[:2]] == step_plans(arith, rows_v, rows_e)
    assert_deep(together, 64, cuda_device, arith)
    launch(arith, together, 64, cuda_device)
    for c in apart:
        launch(arith, [c], 64, cuda_device)
    for i, (a, b) in enumerate(zip(together, apart)):
        ga, gb = same_bits(a, b)
        if a.rows:
            assert rel_err(ga["ln_grad"], gb["ln_grad"]) < 1e-6
            check(a, cuda_device, what="task %d " % i)
        else:
            assert not ga["ln_grad"].any()


@pytest.mark.parametrize("arith,d,dx,mode", [("h2", 64, 0, "gather"), ("h2", 64, 64, "bias"), ("f32", 64, 0, "gather"),
                                             ("f32", 64, 64, "plain"), ("f32", 128, 128, "plain")])
def test_lnlstm_bwd_deferred_reduction_over_launches(cuda_device, arith, d, dx, mode):
    """defer_reduce: three launches (three time steps) ADD their LayerNorm-gradient partials to one zeroed workspace and
    leave ln_grad alone; tspgnn_lnlstm_bwd_finish_f32 then adds the fold to ln_grad.  Equal, to fp32 rounding, to the sum of
    three single-launch ln_grads (on top of what ln_grad held); the other outputs bit for bit those of the plain launches
    (gather-init with KT, bias-init with KTg: the forms of the training step)."""
    rows = [333, rows_of("deep", cuda_device)[0], 17]
    kw = dict(gather=True, fused=True) if mode == "gather" else dict(bias_init=True, fused=True) if mode == "bias" else {}
    deferred, single = ([Cell(arith, d, dx, r, seed=40 + i, **kw) for i, r in enumerate(rows)] for _ in range(2))
    assert_deep([deferred[1]], d, cuda_device, arith)
    ws = workspace(d, cuda_device)
    start = np.random.RandomState(0).randn(10 * d).astype(np.float32)
    ln_grad = dev(start, cuda_device)
    for c in deferred:
        launch(arith, [c], d, cuda_device, ws=ws, defer=True, ln_grad=ln_grad)
        assert np.array_equal(ln_grad.cpu().numpy(), start)
    _lib.call("tspgnn_lnlstm_bwd_finish_f32", _lib.ptr(ws), _lib.ptr(ln_grad), d, None)
    torch.cuda.synchronize()
    total = start.astype(np.float64)
    for a, b in zip(deferred, single):
        launch(arith, [b], d, cuda_device)
        assert a.untouched() and b.untouched()
        total = total + same_bits(a, b)[1]["ln_grad"]
    got = ln_grad.cpu().numpy().astype(np.float64)
    assert rel_err(got, total) < 1e-6
    e = rel_err(got - start, sum(b.reference(cuda_device)["ln_grad"] for b in single))
    print(" accumulated ln_grad %.1e" % e, end="")
    assert e < TOL


@pytest.mark.parametrize("arith,d,dx,mode", [("h2", 64, 0, "gather"), ("h2", 64, 64, "bias"), ("f32", 64, 0, "gather"),
                                             ("f32", 128, 128, "plain")])
def test_lnlstm_bwd_is_deterministic(cuda_device, arith, d, dx, mode):
    """Two identical launches at ROWS_DEEP (gather-init with KT, bias-init with KTg; fp32: gather-init with KT, chunked K)
    give identical outputs, the LayerNorm gradients included, bit for bit."""
    kw = dict(gather=True, fused=True) if mode == "gather" else dict(bias_init=True, fused=True) if mode == "bias" else {}
    cells = [Cell(arith, d, dx, rows_of("deep", cuda_device)[0], seed=9, **kw) for _ in range(2)]
    assert_deep(cells[:1], d, cuda_device, arith)
    for c in cells:
        launch(arith, [c], d, cuda_device)
    same_bits(*cells, names=("dz", "dc_in", "dxh", "dxg", "ln_grad"))


EDGE_FORMS = [("h2", 64, 0, "gather"), ("h2", 64, 64, "bias"), ("h2", 32, 64, "plain"), ("f32", 64, 0, "gather"),
              ("f32", 128, 32, "plain")]


@pytest.mark.parametrize("arith,d,dx,mode", EDGE_FORMS)
def test_lnlstm_bwd_without_incoming_gradients(cuda_device, arith, d, dx, mode):
    """dh_out and dc_out both NULL (= zero): dz, dc_in, the LayerNorm gradients, dxh and dxg are exactly zero."""
    kw = dict(gather=True, fused=True) if mode == "gather" else dict(bias_init=True, fused=True) if mode == "bias" else {}
    cell = Cell(arith, d, dx, 333, seed=3, null_grads=True, **kw)
    launch(arith, [cell], d, cuda_device)
    check(cell, cuda_device)
    assert set(cell.named_outputs()) == {"dz", "dc_in", "ln_grad"} | ({"dxh"} if kw else set()) | ({"dxg"} if mode == "bias" else set())


@pytest.mark.parametrize("rows", [1, 15, 17, "deep"])
@pytest.mark.parametrize("arith,d,dx,mode", EDGE_FORMS)
def test_lnlstm_bwd_leaves_rows_beyond_the_task_alone(cuda_device, arith, d, dx, mode, rows):
    """Every output is allocated with 16 spare rows holding a sentinel: the lanes of a partial last tile are clamped to the
    last row and masked (`valid`), on the direct path (a wavefront's first tile) and, at ROWS_DEEP, on the prefetched one
    -- the spare rows keep the sentinel, and every row of the task is written."""
    rows, _ = rows_of(rows, cuda_device)
    kw = dict(gather=True, fused=True) if mode == "gather" else dict(bias_init=True, fused=True) if mode == "bias" else {}
    cell = Cell(arith, d, dx, rows, seed=rows % 1000, **kw)
    if rows > 333:
        assert_deep([cell], d, cuda_device, arith)
    launch(arith, [cell], d, cuda_device)
    assert cell.untouched() and cell.written()


@pytest.mark.parametrize("case", ["lds", "d128", "KT_dx", "zbias_uv", "KTg_d32"])
def test_lnlstm_bwd_h2_refuses_what_it_does_not_implement(cuda_device, case):
    """Valid calls the f16x2 entry declines: a K that does not fit LDS (d = 64, dx = 96), d = 128, the fused dxh beside a
    dx > 0, bias-init beside gather-init, the streamed data gradient at d = 32 -- an error code, nothing launched, every
    output as it was."""
    d, rows = 64, 33
    if case == "lds":
        cell = Cell("h2", 64, 96, rows, seed=1)
    elif case == "zbias_uv":
        cell = Cell("h2", 64, 0, rows, seed=1, gather=True)
    elif case == "KTg_d32":
        d, cell = 32, Cell("h2", 32, 32, rows, seed=1)
    else:
        cell = Cell("h2", 64, 64, rows, seed=1)
    lg0 = np.random.RandomState(2).randn(10 * d).astype(np.float32)
    ln_grad = dev(lg0, cuda_device)
    t = cell.task(cuda_device, ln_grad=ln_grad)
    spare = empty((rows * 8 * d,), cuda_device, SENTINEL)       # stands in for KT / KTg / zbias / zscale and dxh / dxg
    fields = {"KT_dx": ("KT", "dxh"), "zbias_uv": ("zbias", "zscale"), "KTg_d32": ("KTg", "dxg", "dxh")}.get(case, ())
    for f in fields:
        setattr(t, f, _lib.ptr(spare))
    arr = (_lib.LstmBwdTask * 1)(t)
    rc = _lib.lib.tspgnn_lnlstm_bwd_multi_h2(ctypes.cast(arr, ctypes.c_void_p), 1, 128 if case == "d128" else d, None)
    torch.cuda.synchronize()
    assert rc != 0
    if case == "lds":
        assert "does not fit LDS" in _lib.lib.tspgnn_last_error().decode("utf-8", "replace")
    assert cell.untouched(whole=True) and bool(spare.eq(SENTINEL).all())
    assert np.array_equal(ln_grad.cpu().numpy(), lg0) and cell.workspace_clear()
