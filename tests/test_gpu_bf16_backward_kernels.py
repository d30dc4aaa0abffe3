"""The bf16-storage mode's backward kernels (csrc/dense_bwd_bf16.hip) called directly, against float64 references on the
device: tspgnn_lnlstm_bwd_multi_bf16 (with tspgnn_lnlstm_bwd_finish_f32 for its deferred LayerNorm gradients) and
tspgnn_linear_bf16w_f32.  The model reaches them only at the shapes its fixtures happen to have; these tests aim at the
kernels' own edges -- the chunked-K path, the column-block split, tiles left over after the last full round, several
tasks in one launch, accumulation across launches."""
import ctypes

import numpy as np
import pytest
import torch

import lstm_bwd_cases
from conftest import rel_err
from lstm_bwd_cases import dev, empty, k_chunked, packed_bf16, rb, release, workspace
from tspgnn import _lib

pytestmark = pytest.mark.gpu

TOL = 5e-6          # the fp32 backward kernels' bar (test_gpu_backward_kernels.py)


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


class Cell(lstm_bwd_cases.Cell):
    """One backward task's inputs (lstm_bwd_cases.Cell in the bf16 arithmetic): bf16-exact x, h, K (or the gather-init Zx,
    uv, Kh), fp32 c, dh', dc', LayerNorm."""

    def __init__(self, d, dx, rows, seed, gather=False, null_grads=False, n_src=257):
        super().__init__("bf16", d, dx, rows, seed, gather=gather, null_grads=null_grads, n_src=n_src)

    def reference(self, device):
        """float64 autograd of TO.lnlstm_cell with respect to z (z64) -> (dz, dc_in, ln_grad [10d])."""
        ref = super().reference(device)
        return [ref["dz"], ref["dc_in"], ref["ln_grad"]]


def launch(tasks, d):
    _lib.call_multi("tspgnn_lnlstm_bwd_multi_bf16", tasks, d)
    torch.cuda.synchronize()


def check(cell, device):
    got = cell.outputs()
    if cell.dh is None:     # no incoming gradient: all three are exactly zero
        for name, a in zip(("dz", "dc_in", "ln_grad"), got):
            assert not a.any(), name
        return
    for name, a, b in zip(("dz", "dc_in", "ln_grad"), got, cell.reference(device)):
        assert rel_err(a, b) < TOL, (name, rel_err(a, b))


ROWS = [1, 15, 16, 17, 333, 70001]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d,dx", [(32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 32), (128, 128), (128, 256)])
def test_lnlstm_bwd_bf16_plain_vs_autograd(cuda_device, d, dx, rows):
    """Plain mode, z = [x | h] K: dz, dc and the LayerNorm gradients at the fp32 kernels' bar (both GEMM operands are
    bf16-exact, so the recomputed z is the forward's own).  d = 128 with dx >= 128 streams K through LDS in chunks."""
    if d == 128 and dx >= 128:
        assert k_chunked(d, dx)
    cell = Cell(d, dx, rows, seed=d * 7 + dx + rows)
    launch([cell.task(cuda_device)], d)
    check(cell, cuda_device)
    print(" rows quietened at a relu kink: %d of %d" % (cell.quietened, rows), end="")
    assert cell.quietened <= 3 + 0.005 * rows     # (expected: ~4e-3 of the rows; measured at most 272 of 70 001)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [32, 64, 128])
def test_lnlstm_bwd_bf16_gather_init_vs_autograd(cuda_device, d, rows):
    """Gather-init mode, z = Zx[u] + Zx[v] + h Kh with the bf16 blocked Zx of Tape.ZX; Kh stays resident even at d = 128."""
    assert not k_chunked(d, 0)
    cell = Cell(d, 0, rows, seed=d + rows, gather=True)
    launch([cell.task(cuda_device)], d)
    check(cell, cuda_device)


def test_lnlstm_bwd_bf16_at_the_config5_edge_rows(cuda_device):
    """The benchmark's edge cell: gather-init, d = 128, M = 636 800 rows (32 graphs of n = 200), 6 400 source rows."""
    cell = Cell(128, 0, 636800, seed=5, gather=True, n_src=6400)
    launch([cell.task(cuda_device)], 128)
    check(cell, cuda_device)


@pytest.mark.parametrize("d,dx,gather", [(64, 64, False), (128, 128, False), (128, 0, True)])
def test_lnlstm_bwd_bf16_without_incoming_gradients(cuda_device, d, dx, gather):
    """dh_out and dc_out both NULL (= zero): every output is exactly zero."""
    cell = Cell(d, dx, 333, seed=3, gather=gather, null_grads=True)
    launch([cell.task(cuda_device)], d)
    check(cell, cuda_device)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("n_tasks", [2, 3])
def test_lnlstm_bwd_bf16_multi_task_equals_separate_launches(cuda_device, d, n_tasks):
    """A vertex-style task (plain, dx = d: chunked K at d = 128), an edge-style task (gather-init) and, with three, an
    empty one (rows = 0) in ONE launch: dz and dc bit for bit those of separate launches.  The LayerNorm gradients are sums
    over the task's share of the workgroups, which the table changes: they agree to fp32 rounding."""
    specs = [dict(dx=d, rows=6400, gather=False), dict(dx=0, rows=70001, gather=True)] + \
        ([dict(dx=d, rows=0, gather=False)] if n_tasks == 3 else [])
    together = [Cell(d, s["dx"], s["rows"], seed=11 + i, gather=s["gather"]) for i, s in enumerate(specs)]
    apart = [Cell(d, s["dx"], s["rows"], seed=11 + i, gather=s["gather"]) for i, s in enumerate(specs)]
    launch([c.task(cuda_device) for c in together], d)
    for c in apart:
        launch([c.task(cuda_device)], d)
    for a, b in zip(together, apart):
        ga, gb = a.outputs(), b.outputs()
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])
        if a.rows:
            assert rel_err(ga[2], gb[2]) < 1e-6
            check(a, cuda_device)
        else:
            assert not ga[2].any()


@pytest.mark.parametrize("d,dx,gather", [(64, 64, False), (128, 128, False), (128, 0, True)])
def test_lnlstm_bwd_bf16_deferred_reduction_over_launches(cuda_device, d, dx, gather):
    """defer_reduce: three launches (three time steps) ADD their LayerNorm-gradient partials to one zeroed workspace and
    leave ln_grad alone; tspgnn_lnlstm_bwd_finish_f32 then adds the fold to ln_grad.  Equal, to fp32 rounding, to the sum of
    three single-launch ln_grads (on top of what ln_grad held); dz and dc bit for bit those of the plain launches."""
    rows = [333, 70001, 17]
    deferred = [Cell(d, dx, r, seed=40 + i, gather=gather) for i, r in enumerate(rows)]
    single = [Cell(d, dx, r, seed=40 + i, gather=gather) for i, r in enumerate(rows)]
    ws = workspace(d, cuda_device)
    start = np.random.RandomState(0).randn(10 * d).astype(np.float32)
    ln_grad = dev(start, cuda_device)
    for c in deferred:
        launch([c.task(cuda_device, ws=ws, defer=True, ln_grad=ln_grad)], d)
        assert np.array_equal(ln_grad.cpu().numpy(), start)
    _lib.call("tspgnn_lnlstm_bwd_finish_f32", _lib.ptr(ws), _lib.ptr(ln_grad), d, None)
    total = start.astype(np.float64)
    for a, b in zip(deferred, single):
        launch([b.task(cuda_device)], d)
        ga, gb = a.outputs(), b.outputs()
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])
        total = total + gb[2]
    torch.cuda.synchronize()
    assert rel_err(ln_grad.cpu().numpy(), total) < 1e-6
    assert rel_err(ln_grad.cpu().numpy().astype(np.float64) - start, sum(b.reference(cuda_device)[2] for b in single)) < TOL


@pytest.mark.parametrize("d,dx,gather", [(128, 128, False), (128, 0, True), (32, 64, False)])
def test_lnlstm_bwd_bf16_is_deterministic(cuda_device, d, dx, gather):
    """Two identical launches give identical dz, dc and LayerNorm gradients, bit for bit."""
    outs = []
    for _ in range(2):
        c = Cell(d, dx, 70001, seed=9, gather=gather)
        launch([c.task(cuda_device)], d)
        outs.append(c.outputs())
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", ["KT", "dxh", "zbias", "KTg", "dx16", "d96"])
def test_lnlstm_bwd_bf16_rejects_what_it_does_not_implement(cuda_device, case):
    """The fused data gradient (KT / dxh, KTg), the bias-init start (zbias), a dx that is not a multiple of 32 and a width
    other than 32 / 64 / 128 are refused with an error code -- before anything is launched."""
    d = 64
    cell = Cell(d, 64, 33, seed=1)
    t = cell.task(cuda_device)
    spare = empty((33 * 4 * d,), cuda_device, 0.0)
    if case in ("KT", "dxh", "zbias", "KTg"):
        setattr(t, case, _lib.ptr(spare))
    elif case == "dx16":
        t.dx = 16
    arr = (_lib.LstmBwdTask * 1)(t)
    rc = _lib.lib.tspgnn_lnlstm_bwd_multi_bf16(ctypes.cast(arr, ctypes.c_void_p), 1, 96 if case == "d96" else d, None)
    torch.cuda.synchronize()
    assert rc != 0


# ------------------------------------------------------------------------------------------ tspgnn_linear_bf16w_f32
def linear_bar(X, W, kin):
    """|Y - X W| <= 2 * 2^-16 (|X| |W|) + fp32 accumulation: X enters as two bf16 pieces (16 significand bits: 2^-16
    relative per product), the products accumulate in fp32 over 2 kin / 32 MFMA steps."""
    return (2.0 * 2.0 ** -16 + (kin / 16 + 1) * 2.0 ** -24) * (X.abs() @ W.abs())


@pytest.mark.parametrize("rows", [1, 17, 333, 70001])
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n1,n2", [(128, 128), (64, 128), (16, 96), (48, 0), (0, 16)])
@pytest.mark.parametrize("kin", [32, 128, 256, 512, 1024])
def test_linear_bf16w_vs_float64(cuda_device, kin, n1, n2, acc, rows):
    """Y1 | Y2 = X W for an fp32 X and W = piece 0 of tspgnn_pack_weights_x3 of a bf16-exact W[kin, n1 + n2], against
    float64, elementwise at the two-piece bar -- which an emulation using only X's leading bf16 piece (8 bits) violates on
    the same data.  The column tiles split 8 + 8, 8 + 4, 4 + 2 + 1, 2 + 1 and 1 (4-tile blocks at kin = 1024, where an
    8-tile block exceeds the LDS gate), with the n1 | n2 boundary inside a block; Y2 pre-filled, added to with accumulate_y2."""
    rng = np.random.RandomState(kin + n1 + 3 * n2 + rows + acc)
    n = n1 + n2
    X = rng.randn(rows, kin).astype(np.float32) * np.float32(10.0) ** rng.randint(-3, 4, size=(rows, 1)).astype(np.float32)
    W = rb(rng.randn(kin, n) / np.sqrt(kin))
    Y2_0 = rng.randn(rows, max(n2, 1)).astype(np.float32)
    Y1 = empty((rows, max(n1, 1)), cuda_device)
    Y2 = dev(Y2_0, cuda_device)
    _lib.call("tspgnn_linear_bf16w_f32", _lib.ptr(dev(X, cuda_device)), kin, _lib.ptr(packed_bf16(W, cuda_device)),
              _lib.ptr(Y1) if n1 else None, n1, _lib.ptr(Y2) if n2 else None, n2, acc, rows, None)
    torch.cuda.synchronize()
    X64 = torch.tensor(X, dtype=torch.float64, device=cuda_device)
    W64 = torch.tensor(W, dtype=torch.float64, device=cuda_device)
    ref = X64 @ W64
    bar = linear_bar(X64, W64, kin)
    got = torch.empty_like(ref)
    if n1:
        got[:, :n1] = Y1.to(torch.float64)
    if n2:
        base = torch.tensor(Y2_0, dtype=torch.float64, device=cuda_device) if acc else 0.0
        got[:, n1:] = Y2.to(torch.float64) - base
        if acc:   # the final fp32 add of the pre-filled Y2
            bar[:, n1:] += 2.0 ** -24 * (Y2.to(torch.float64).abs() + base.abs())
    err = (got - ref).abs()
    assert bool((err <= bar).all()), float((err / bar.clamp_min(1e-300)).max())
    hi = torch.tensor(rb(X), dtype=torch.float64, device=cuda_device) @ W64   # the leading piece of X alone
    assert bool(((hi - ref).abs() > bar).any())
