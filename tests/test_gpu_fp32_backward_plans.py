"""The fp32 backward kernels of csrc/dense_bwd.hip called directly at their LARGE launch plans -- the ones every real batch
takes and the older direct tests (rows <= 1000) never reach -- against float64 on the device.  Every row count is derived
from the device's CU count, and every test asserts the branch and its depth through tests/plan_replay.py BEFORE it
launches.  The row counts named below are those at 256 CUs (MI355X).

tspgnn_linear_f32 (launch_linear), (kin, n1, n2) in (256, 0, 64) [64 KB of W in LDS, two workgroups per CU], (128, 64, 64)
[64 KB, two], (256, 64, 64) [131 KB, one: the training shape], (512, 128, 128) [W streamed through LDS 8 k-blocks at a
time], (256, 48, 16) [the n1 | n2 boundary inside a wavefront's tile group]:
  * linear_split_kernel at 1, 15, 16, 17 and 16 * 4 * CUs = 16 384 rows (its last row count);
  * linear_kernel with the ticket from 16 * 4 * CUs + 1 = 16 385 rows (its first): nw = 4 where two workgroups share a CU,
    nw = 8 at once where one does.  nw = 4 holds while tiles <= 4 * grid, so its deepest launch, 16 * 4 * grid - 15 =
    32 753 rows, gives every wavefront ONE tile (the last of one row); the row count 16 * (2 * grid * 4) + 1 = 65 537 that
    would give an nw = 4 launch two tiles per wavefront is by the same rule an nw = 8 launch -- it is run, and asserted to
    be one;
  * nw = 8 at 16 * (2 * grid * 8) + 1 = 131 073 rows (65 537 with one workgroup per CU): every workgroup's [t_beg, t_end)
    holds 16 or 17 tiles, two to three per wavefront through the ticket, the last tile of one row;
  * the streamed path at every row count above and at 16 * 8 * (2 * CUs) + 17 = 65 553 rows: 513 rounds of 8 tiles over 256
    workgroups (r += gridDim.x: two rounds each, three for the first), six dead tiles in the last round.
  Both accumulate_y2, Y2 pre-filled, the rows of X (and of the pre-filled Y2) times 10^k, k in -3 .. 3.

tspgnn_mlp_bwd_multi_f32 (launch_mlp_bwd), the (d, L, mask) of test_mlp_backward_and_wgrad at 1, 17 and
16 * (2 * grid * 8) + 1 = 131 073 rows (d = 128: 65 537; nw = 8, two to three tiles per wavefront); one task, two tasks of
333 and the deep row count in one launch, accumulate_dx 0 and 1, fp32 and bf16 saved activations (acts_bf16); dX and every
layer's dpre.  The saved activations only decide the relu masks, so they are drawn at random and the float64 chain uses the
masks of the very values the kernel reads.

tspgnn_wgrad_f32's generic kernel wgrad_kernel<AV, BV>, all nine (AV, BV) = kin in {16, 32, 64} x nout in {16, 32, 64}: at
70 001 rows (274 chunks of 256 rows, the last of 113; reduce_partials at S = 16) except (4, 4), which is run at 4095 rows,
the last on the generic kernel (16 chunks, the last of 255; S = 4), and at 4096, the first on wgrad_x3_kernel; with and
without db; accumulating onto a non-zero dW and db.

Bars, all against float64.  Inherited: whole tensor rel_err < TOL = 5e-6 (test_gpu_backward_kernels.py); row by row
lstm_bwd_cases.row_err < ROW_TOL = 2e-5 (test_gpu_h2_backward_kernels.py) for dX, dpre, Y1 and Y2.  Derived, for linear:
elementwise |Y - X W| <= (kin + 2) 2^-24 (|X| |W|) -- an fp32 FMA chain of kin terms plus the accumulate add (the
pre-filled Y2 is drawn at the scale of its row of X, so that its add stays inside the chain's allowance).  Every output
has 16 spare rows of SENTINEL behind it, found intact.  Each test prints its worst ratios.

Measured on the MI355X (256 CUs), worst over all cases -- linear: elementwise 0.06 of the derived bar (0.04 split, 0.05
ticket nw = 4, 0.06 ticket nw = 8, 0.01 streamed), whole tensor Y1 9.9e-7, Y2 1.0e-6, row by row Y1 2.1e-6, Y2 2.0e-6;
mlp_bwd: dpre 4.2e-7 whole, 1.1e-6 row by row, dX 3.5e-7 and 1.2e-6; wgrad: dW 3.9e-7 (generic), 3.2e-7 (x3 at 4096 rows),
db 1.9e-7.  Rounding, a fifth to a tenth of the inherited bars; no bar was moved.

Mutations, each on a scratch build, one run each: with `tile >= t_end - 1` in linear_kernel's ticket loop the older
direct tests (test_linear, the cell chains) still pass and exactly the 28 ticket cases here fail, the split and streamed
ones pass."""
import numpy as np
import pytest
import torch

import plan_replay as PR
from conftest import rel_err
from lstm_bwd_cases import SENTINEL, SPARE, empty, packed_f32, release, row_err
from tspgnn import _lib

pytestmark = pytest.mark.gpu

TOL = 5e-6          # test_gpu_backward_kernels.TOL
ROW_TOL = 2e-5      # test_gpu_h2_backward_kernels.ROW_TOL


@pytest.fixture(autouse=True)
def _release():
    yield
    release()


def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def generator(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=g.device, generator=g)


def row_scale(g, rows):
    """10^k per row, k in -3 .. 3."""
    return torch.pow(10.0, torch.randint(-3, 4, (rows, 1), device=g.device, generator=g).to(torch.float32))


def padded(t, device):
    """A copy of the [rows, n] tensor t with SPARE rows of SENTINEL behind it."""
    out = empty((t.shape[0] + SPARE,) + tuple(t.shape[1:]), device, SENTINEL)
    out[:t.shape[0]].copy_(t)
    return out


def host(t):
    return t.cpu().numpy().astype(np.float64)


def check_rows(name, got, ref, rows, what):
    """got [rows + SPARE, n] fp32 against ref [rows, n] float64: whole tensor at TOL, row by row at ROW_TOL, spare rows
    intact.  -> the measures that miss (all of them, not only the first)."""
    assert bool(got[rows:].eq(SENTINEL).all()), "%s: rows beyond the task's were written" % name
    g, r = host(got[:rows]), host(ref)
    whole, rowwise = rel_err(g, r), row_err(g, r)
    print(" %s %s whole %.1e row %.1e" % (what, name, whole, rowwise), end="")
    return [(name, "whole", whole)] * (not whole < TOL) + [(name, "row", rowwise)] * (not rowwise < ROW_TOL)


# ------------------------------------------------------------------------------------------------ tspgnn_linear_f32
LINEAR_SHAPES = [(256, 0, 64), (128, 64, 64), (256, 64, 64), (512, 128, 128), (256, 48, 16)]


def _linear_cases():
    out = []
    for kin, n1, n2 in LINEAR_SHAPES:
        p = PR.linear_plan(kin, n1, n2, 1, 256)        # per_cu and resident / streamed do not depend on the CU count
        streamed = p.path == "streamed"
        rows = [1, 15, 16, 17, "split_last", "ticket_first"]
        rows += ["streamed_deep"] if streamed else ["nw8_deep"]
        if not streamed and p.per_cu == 2:
            rows += ["nw4_deep", "nw4_formula"]
        out += [(kin, n1, n2, r) for r in rows]
    return out


def linear_rows(kin, n1, n2, rows, n_cus):
    """A parametrised row count -> (rows, check of the queried plan)."""
    p1 = PR.linear_plan(kin, n1, n2, 1, n_cus)
    streamed, full = p1.path == "streamed", n_cus * p1.per_cu
    small = "streamed" if streamed else "split"
    if isinstance(rows, int):
        return rows, lambda p: p.path == small
    if rows == "split_last":
        return 16 * 4 * n_cus, lambda p: p.path == small and p.tiles == 4 * n_cus
    if rows == "ticket_first":
        return 16 * 4 * n_cus + 1, lambda p: p.path == ("streamed" if streamed else "ticket") and p.tiles == 4 * n_cus + 1 and \
            p.nw == (4 if p1.per_cu == 2 and not streamed else 8)
    if rows == "nw4_deep":          # tiles == 4 * grid: one tile per wavefront, the last of one row
        return 16 * 4 * full - 15, lambda p: (p.path, p.nw, p.grid, p.lo, p.hi) == ("ticket", 4, full, 1, 1)
    if rows == "nw4_formula":       # two tiles per slot of an nw = 4 grid: by launch_linear's rule an nw = 8 launch
        return 16 * (2 * full * 4) + 1, lambda p: (p.path, p.nw, p.grid) == ("ticket", 8, full) and p.lo >= 1 and p.hi >= 2
    if rows == "nw8_deep":
        return 16 * (2 * full * 8) + 1, lambda p: (p.path, p.nw, p.grid) == ("ticket", 8, full) and p.lo >= 2 and p.hi >= 3
    assert rows == "streamed_deep" and streamed
    return 16 * 8 * (2 * n_cus * p1.per_cu) + 17, lambda p: (p.path, p.nw, p.grid) == ("streamed", 8, full) and \
        p.lo >= 2 and p.hi >= 3 and p.dead > 0 and p.qc < kin // 16


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("kin,n1,n2,rows", _linear_cases())
def test_linear_f32_every_path_vs_float64(cuda_device, kin, n1, n2, rows, acc):
    """Y1 | Y2 (+)= X W on linear_split_kernel, linear_kernel with the ticket (nw = 4, nw = 8) and linear_kernel with W
    streamed in rounds -- see the module docstring for the row counts; the path and its depth asserted through the plan query."""
    seed = kin + 3 * n1 + 7 * n2 + acc + (rows if isinstance(rows, int) else sum(map(ord, rows)))
    rows, expected = linear_rows(kin, n1, n2, rows, cus(cuda_device))
    plan = PR.linear_plan(kin, n1, n2, rows, cus(cuda_device))
    assert expected(plan), plan
    g = generator(cuda_device, seed)
    scale = row_scale(g, rows)
    X = randn(g, rows, kin) * scale
    W = (np.random.RandomState(seed).randn(kin, n1 + n2) / np.sqrt(kin)).astype(np.float32)
    Y2_0 = randn(g, rows, n2) * scale
    Y1 = empty((rows + SPARE, max(n1, 1)), cuda_device, SENTINEL)
    Y2 = padded(Y2_0, cuda_device)
    _lib.call("tspgnn_linear_f32", _lib.ptr(X), kin, _lib.ptr(packed_f32(W, cuda_device)), _lib.ptr(Y1) if n1 else None, n1,
              _lib.ptr(Y2), n2, acc, rows, None)
    torch.cuda.synchronize()
    X64, W64 = X.to(torch.float64), torch.tensor(W, dtype=torch.float64, device=cuda_device)
    ref = X64 @ W64
    bar = (kin + 2) * 2.0 ** -24 * (X64.abs() @ W64.abs())
    if acc:
        ref[:, n1:] += Y2_0.to(torch.float64)
    got = torch.cat([Y1[:rows, :n1].to(torch.float64), Y2[:rows].to(torch.float64)], dim=1)
    worst = float(((got - ref).abs() / bar.clamp_min(1e-300)).max())
    print(" linear %s nw=%d grid=%d [%d rows] elementwise %.2f of the bar" % (plan.path, plan.nw, plan.grid, rows, worst), end="")
    over = []
    if n1:
        over += check_rows("Y1", Y1[:, :n1], ref[:, :n1], rows, "linear")
    else:
        assert bool(Y1.eq(SENTINEL).all())
    over += check_rows("Y2", Y2, ref[:, n1:], rows, "linear")
    assert not over and worst <= 1.0, (over, worst)


# ----------------------------------------------------------------------------------------- tspgnn_mlp_bwd_multi_f32
MLP_SHAPES = [(64, 4, 0b0111), (64, 3, 0b111), (32, 4, 0b0111), (32, 2, 0b01), (128, 2, 0b11), (64, 1, 0)]


def mlp_deep_rows(d, n_cus):
    """16 * (2 * grid * 8) + 1 with launch_mlp_bwd's full grid: 131 073 rows on 256 CUs (d = 128: 65 537)."""
    full = n_cus * (1 if d >= 128 else 2)
    return 16 * (2 * full * 8) + 1


class MlpCase(object):
    """One tspgnn_mlp_bwd_task: dY and the pre-filled dX with rows times 10^k, saved activations and Yout drawn at random
    (only their signs matter), the weights W_l / sqrt(d); outputs with SPARE rows of SENTINEL behind them."""

    def __init__(self, d, L, mask, rows, acc, seed, device, bf16=False):
        self.d, self.L, self.mask, self.rows, self.acc, self.bf16 = d, L, mask, rows, acc, bf16
        g = generator(device, seed)
        scale = row_scale(g, rows)
        self.dY, self.dX0 = randn(g, rows, d) * scale, randn(g, rows, d) * scale
        self.acts, self.Yout = randn(g, max(L - 1, 1), rows, d), randn(g, rows, d)
        if bf16:
            self.acts, self.Yout = self.acts.to(torch.bfloat16), self.Yout.to(torch.bfloat16)
        rng = np.random.RandomState(seed)
        self.Ws = [(rng.randn(d, d) / np.sqrt(d)).astype(np.float32) for _ in range(L)]
        self.wt = torch.cat([packed_f32(w, device, transposed=1).view(-1) for w in self.Ws])
        self.dpre = empty((L, rows + SPARE, d), device, SENTINEL)
        self.dX = padded(self.dX0, device)

    def task(self):
        return _lib.MlpBwdTask(dY=_lib.ptr(self.dY), wt=_lib.ptr(self.wt), acts=_lib.ptr(self.acts) if self.L > 1 else None,
                               acts_stride=self.rows * self.d, Yout=_lib.ptr(self.Yout), dpre=_lib.ptr(self.dpre),
                               dpre_stride=(self.rows + SPARE) * self.d, dX=_lib.ptr(self.dX), accumulate_dx=self.acc,
                               rows=self.rows, n_layers=self.L, relu_mask=self.mask, acts_bf16=int(self.bf16))

    def check(self, device, what):
        """dX and every layer's dpre against the float64 chain with the masks of the stored activations."""
        G = self.dY.to(torch.float64)
        over = []
        for l in range(self.L - 1, -1, -1):
            if (self.mask >> l) & 1:
                A = self.Yout if l == self.L - 1 else self.acts[l]
                G = G * (A.to(torch.float32) > 0)
            over += check_rows("dpre%d" % l, self.dpre[l], G, self.rows, what)
            G = G @ torch.tensor(self.Ws[l], dtype=torch.float64, device=device).T
        if self.acc:
            G = G + self.dX0.to(torch.float64)
        over += check_rows("dX", self.dX, G, self.rows, what)
        return over


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("rows", [1, 17, "deep"])
@pytest.mark.parametrize("d,L,mask", MLP_SHAPES)
def test_mlp_bwd_f32_one_task_vs_float64(cuda_device, d, L, mask, rows, acc):
    """One task at 1 and 17 rows (nw = 4, one workgroup) and at 16 * (2 * grid * 8) + 1 rows (nw = 8, every workgroup 16 or
    17 tiles: two to three per wavefront through the ticket, the last tile of one row)."""
    n_cus = cus(cuda_device)
    deep = rows == "deep"
    rows = mlp_deep_rows(d, n_cus) if deep else rows
    plan = PR.mlp_bwd_plan([(rows, L)], d, n_cus)
    if deep:
        assert plan.nw == 8 and plan.grid == n_cus * (1 if d >= 128 else 2) and plan.lo[0] >= 2 and plan.hi[0] >= 3, plan
    else:
        assert plan.nw == 4 and plan.grid == 1, plan
    case = MlpCase(d, L, mask, rows, acc, seed=d * L + mask + acc + rows % 1000, device=cuda_device)
    _lib.call_multi("tspgnn_mlp_bwd_multi_f32", [case.task()], d)
    torch.cuda.synchronize()
    over = case.check(cuda_device, "mlp_bwd nw=%d [%d rows]" % (plan.nw, rows))
    assert not over, over


@pytest.mark.parametrize("d,L,mask", [(64, 4, 0b0111), (32, 2, 0b01), (128, 2, 0b11)])
def test_mlp_bwd_f32_two_unequal_tasks_in_one_launch(cuda_device, d, L, mask):
    """333 rows (accumulate_dx = 1) and the deep row count (accumulate_dx = 0) in ONE launch: the grid is shared by cost, the
    small task gets a handful of workgroups, the deep task's wavefronts still two tiles or more each."""
    n_cus = cus(cuda_device)
    rows = [333, mlp_deep_rows(d, n_cus)]
    plan = PR.mlp_bwd_plan([(r, L) for r in rows], d, n_cus)
    assert plan.nw == 8 and plan.blocks[0] >= 1 and plan.lo[1] >= 2 and plan.hi[1] >= 3, plan
    cases = [MlpCase(d, L, mask, r, acc, seed=900 + d + i, device=cuda_device) for i, (r, acc) in enumerate(zip(rows, (1, 0)))]
    _lib.call_multi("tspgnn_mlp_bwd_multi_f32", [c.task() for c in cases], d)
    torch.cuda.synchronize()
    over = sum((c.check(cuda_device, "mlp_bwd task %d of 2 [%d rows, %d workgroups]" % (i, c.rows, plan.blocks[i]))
                for i, c in enumerate(cases)), [])
    assert not over, over


@pytest.mark.parametrize("rows", [17, "deep"])
@pytest.mark.parametrize("d,L,mask", [(64, 4, 0b0111), (128, 2, 0b11)])
def test_mlp_bwd_f32_bf16_saved_activations(cuda_device, d, L, mask, rows):
    """acts_bf16: the saved activations and Yout are bf16 arrays (acts_stride in elements) that only decide the masks."""
    n_cus = cus(cuda_device)
    deep = rows == "deep"
    rows = mlp_deep_rows(d, n_cus) if deep else rows
    plan = PR.mlp_bwd_plan([(rows, L)], d, n_cus)
    assert (plan.nw == 8 and plan.lo[0] >= 2 and plan.hi[0] >= 3) if deep else plan.nw == 4, plan
    case = MlpCase(d, L, mask, rows, 1, seed=77 + d, device=cuda_device, bf16=True)
    _lib.call_multi("tspgnn_mlp_bwd_multi_f32", [case.task()], d)
    torch.cuda.synchronize()
    over = case.check(cuda_device, "mlp_bwd bf16 acts [%d rows]" % rows)
    assert not over, over


# ------------------------------------------------------------------------------------------------- tspgnn_wgrad_f32
def _wgrad_cases():
    out = []
    for kin in (16, 32, 64):
        for nout in (16, 32, 64):
            out += [(kin, nout, r) for r in ((4095, 4096) if kin == nout == 64 else (70001,))]
    return out


@pytest.mark.parametrize("with_db", [0, 1])
@pytest.mark.parametrize("kin,nout,rows", _wgrad_cases())
def test_wgrad_f32_generic_kernel_every_vector_width(cuda_device, kin, nout, rows, with_db):
    """wgrad_kernel<AV, BV> for all nine (AV, BV) at 70 001 rows ((4, 4): 4095, its last row count; 4096 goes to
    wgrad_x3_kernel and is held to the same bars): >= 3 row chunks with a partial last one, the partials folded by
    reduce_partials at S = 16 (S = 4 at 4095 rows), dW and db accumulated onto non-zero values (with db) or onto zero."""
    plan = PR.wgrad_plan(rows, kin, nout, cus(cuda_device))
    assert (plan.av, plan.bv) == (PR.pick_vec(kin), PR.pick_vec(nout))
    if rows == 4096:
        assert plan.kernel == "x3", plan
    else:
        assert plan.kernel == "generic" and plan.n_chunks >= 3 and 0 < plan.last_rows < plan.chunk_rows, plan
        assert PR.reduce_slices(plan.n_chunks) == (4 if rows == 4095 else 16)
    g = generator(cuda_device, kin * 3 + nout + rows + with_db)
    X, dY = randn(g, rows, kin), randn(g, rows, nout)
    dW0 = randn(g, kin, nout) if with_db else torch.zeros(kin, nout, device=cuda_device)
    db0 = randn(g, 1, nout)
    dW, db = padded(dW0, cuda_device), padded(db0.view(nout, 1), cuda_device)
    n_ws = int(_lib.lib.tspgnn_wgrad_workspace_floats(rows, kin, nout))
    assert n_ws == PR.wgrad_workspace_floats(rows, kin, nout, cus(cuda_device))
    ws = empty((n_ws + SPARE,), cuda_device, SENTINEL)
    _lib.call("tspgnn_wgrad_f32", _lib.ptr(X), _lib.ptr(dY), rows, kin, nout, _lib.ptr(dW), _lib.ptr(db) if with_db else None,
              _lib.ptr(ws), None)
    torch.cuda.synchronize()
    assert bool(dW[kin:].eq(SENTINEL).all()) and bool(db[nout:].eq(SENTINEL).all()) and bool(ws[n_ws:].eq(SENTINEL).all())
    e_w = rel_err(host(dW[:kin]), host(X.to(torch.float64).T @ dY.to(torch.float64) + dW0.to(torch.float64)))
    print(" wgrad %s<%d,%d> [%d rows, %d chunks] dW %.1e" % (plan.kernel, plan.av, plan.bv, rows, plan.n_chunks, e_w), end="")
    if with_db:
        e_b = rel_err(host(db[:nout, 0]), host(dY.to(torch.float64).sum(0) + db0.view(-1).to(torch.float64)))
        print(" db %.1e" % e_b, end="")
        assert e_b < TOL
    else:
        assert bool(db[:nout, 0].eq(db0.view(-1)).all())
    assert e_w < TOL
