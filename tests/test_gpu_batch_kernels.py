"""The once-per-batch kernels of csrc/prepost.hip and the training-tail kernels of csrc/train.hip called directly at the
sizes where their launch shape changes -- persistent workgroups that take a second chunk, capped grids that stride, the
reduction's slice counts, a single workgroup that strides over thousands of problems -- against float64 (or, for the
one-multiply kernels, bit for bit).  Row counts that depend on the CU count are derived from the device and the branch is
asserted through tests/plan_replay.py BEFORE the launch; the counts named below are those at 256 CUs (MI355X).

  tspgnn_einit_bwd_f32   d in {32, 64, 128}; M = 1, 63, 64, 65 (one workgroup per 64-edge chunk), 64 * grid = 32 768
                         (d = 128: 16 384; every persistent workgroup one chunk), 64 * grid + 1 (the first workgroup's
                         chunk += gridDim.x loop takes a second chunk of one edge; every other workgroup prefetches
                         a chunk that does not exist) and 64 * 2 * grid + 1 = 65 537 (32 769): two to three chunks each,
                         the register prefetch of dE0 and the accumulation over chunks in their steady state;
                         reduce_partials at S = 1 (grid < 8) and S = 16 (grid >= 64).  dwb pre-filled (the entry adds).
  tspgnn_wcolsum_f32     d in {4, 32, 64, 128, 256, 1024} (RS = 256, 32, 16, 8, 4, 1 rows in flight); rows 1, 1023, 1024
                         (one chunk, S = 1), 1025 (two chunks), 8 * 1024 + 1 (9 chunks, S = 4), 64 * 1024 + 1 (65 chunks,
                         S = 16) and, at d = 32, 1024 * 4 * CUs + 1 = 1 048 577 (the 4 * CUs chunk cap: 1024 chunks of 1025
                         rows, the last of 2); with and without wt and out_wsum, scale = 1/8, out pre-filled.
  tspgnn_tile_rows_f32, tspgnn_rowdot_bwd_f32   rows 1 x d 4, and 16 400 x 256 (1 049 600 float4s > 4096 * 256: the
                         grid-stride loop's second trip), bit for bit the NumPy float32 product.
  tspgnn_rowdot_f32      rowdot_kernel<8 / 16 / 32 / 64> (d = 32 / 64 / 128 / 256) and rowdot_generic_kernel (d = 4, 20,
                         48, 512) at 1, 3, 4, 5, 255, 256, 257 and 70 001 rows.
  tspgnn_einit_fwd_f32   M = 1, 15, 16, 17 (the 16-edge tile), 255, 256, 257 (the 256-edge workgroup), 70 001.
  tspgnn_segment_mean_f32, tspgnn_vote_grad_f32   one batch of segments 0, 1, 255, 256, 257, 767, 768, 769, 1023, 1024,
                         1025, 2047, 2048, 2049, 19 900, 0 (the four-chain loop switches at k + 768 < end; empty segments
                         first-adjacent and last), and B = 1.
  tspgnn_bce_metrics_f32 B = 1, 255, 256, 257, 1000, 4099: every thread of the one workgroup holds a partial from B = 256
                         on, so a wrong half of the tree cannot pass.
  tspgnn_bucket_pack_f32 / _unpack_f32   n = 2 * 1024 * 256 + 3: every thread of the 1024 capped workgroups two elements,
                         three of them three.

Bars.  Inherited: rel_err < TOL = 5e-6 (test_gpu_backward_kernels.py) for einit_bwd and wcolsum; F32_TOL = 2e-6 whole
tensor (test_gpu_kernels.py) and 2e-5 row by row (test_gpu_h2_backward_kernels.py) for einit_fwd; 1e-6 for vote_grad and
pred.  Derived from the kernels' operation counts and fp32's 2^-24: out_wsum within (chunk_rows / RS + RS + 2) 2^-24
sum |wt| (exact without wt); rowdot within (d + 2) 2^-24 (sum |x_k w_k| + |b|); segment mean within
(ceil(len / 1024) + 12) 2^-24 sum |vote| / len; the mean loss within ((ceil(B / 256) + 11) 2^-24 sum |term| + 4 ulp per
term) / B -- the 4 ulp for the device's expf / log1pf is a supposition; the five counts exactly.  Outputs carry SPARE
elements of SENTINEL behind (vote_grad: before, too), found intact.  Every test prints its worst ratio.

As in the LN-LSTM cell tests (lstm_bwd_cases.Cell.quiet_kinks) the einit_bwd edges where a relu input lies within 2^-16
of its terms' magnitude from zero get no incoming gradient: they pass through the kernel and contribute exactly zero on
both sides, instead of a legitimately different derivative.

Measured on the MI355X (256 CUs), worst over all cases -- einit_bwd 7.4e-7 (at most 1.6 % of the edges quietened: one
of 64); wcolsum out 1.5e-6, out_wsum below 0.005 of its bar; rowdot 0.41 of its bar (d = 4, where the bar is six
roundings wide); einit_fwd 3.4e-7 whole, 8.4e-7 row by row; segment mean 0.011 of its bar; mean loss 0.09 of its bar
(B = 257; 0.003 at B = 1, 0.036 at B = 4099), so the 4 ulp supposed for expf / log1pf were not needed; tile_rows,
rowdot_bwd and the bucket kernels bit for bit.  No bar was moved.

Mutations, each on a scratch build, one run each: einit_bwd with the next chunk's prefetch replaced by zeros --
test_einit_backward (M = 333) still passes, the six cases with more chunks than workgroups here fail (64 * grid + 1 too:
one missing edge of 32 769); bce_metrics with its tree started at off = 64 -- the older B = 1 and B = 6 tests still pass,
B = 255, 256, 257, 1000 and 4099 here fail."""
import numpy as np
import pytest
import torch

import plan_replay as PR
from conftest import rel_err
from lstm_bwd_cases import SENTINEL, SPARE, dev, empty, release, row_err
from tspgnn import _lib

pytestmark = pytest.mark.gpu

TOL = 5e-6          # test_gpu_backward_kernels.TOL
F32_TOL = 2e-6      # test_gpu_kernels.F32_TOL
ROW_TOL = 2e-5      # test_gpu_h2_backward_kernels.ROW_TOL
EPS = 2.0 ** -24


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


def host(t):
    return t.cpu().numpy().astype(np.float64)


def intact(t, n):
    """Do the SPARE elements (rows) behind the first n of t still hold SENTINEL?"""
    return t.shape[0] == n + SPARE and bool(t[n:].eq(SENTINEL).all())


# --------------------------------------------------------------------------------------------- E_init_MLP: parameters
def einit_params(d, seed, bias=0.3):
    """-> ([W_l], [b_l]) of the 2 -> d/8 -> d/4 -> d/2 -> d chain, and the flat wb the entries take."""
    rng = np.random.RandomState(seed)
    dims = [2, d // 8, d // 4, d // 2, d]
    Ws = [rng.randn(a, b).astype(np.float32) for a, b in zip(dims[:-1], dims[1:])]
    bs = [(bias * rng.randn(b)).astype(np.float32) for b in dims[1:]]
    return Ws, bs, np.concatenate([v.reshape(-1) for pair in zip(Ws, bs) for v in pair])


def einit_forward64(WC, Ws, bs):
    """The chain in float64 on WC's device -> (output, [pre-activation, band] of the three relu layers), band =
    2^-16 (|a| |W| + |b|): the distance from zero inside which fp32 may put a relu input on the other side."""
    a, pres = WC.to(torch.float64), []
    for l in range(4):
        pre = a @ Ws[l] + bs[l]
        if l < 3:
            pres.append((pre, 2.0 ** -16 * (a.abs() @ Ws[l].abs() + bs[l].abs())))
            pre = torch.relu(pre)
        a = pre
    return a, pres


# ------------------------------------------------------------------------------------------- tspgnn_einit_bwd_f32
def einit_bwd_M(M, d, n_cus):
    """A parametrised edge count -> (M, the plan expected of it)."""
    full = PR.einit_bwd_full_grid(d, n_cus)
    if isinstance(M, int):
        return M, PR.EinitBwdPlan((M + 63) // 64, (M + 63) // 64, 1, 1)
    return {"grid": (64 * full, PR.EinitBwdPlan(full, full, 1, 1)),
            "grid+1": (64 * full + 1, PR.EinitBwdPlan(full, full + 1, 1, 2)),
            "2grid+1": (64 * 2 * full + 1, PR.EinitBwdPlan(full, 2 * full + 1, 2, 3))}[M]


@pytest.mark.parametrize("M", [1, 63, 64, 65, "grid", "grid+1", "2grid+1"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_einit_bwd_persistent_workgroups_vs_float64(cuda_device, d, M):
    """dwb += the E_init_MLP parameter gradients: one chunk per workgroup, then the chunk += gridDim.x loop with its dE0
    prefetch and its accumulation over chunks (64 * grid + 1: a second chunk of ONE edge for the first workgroup only;
    64 * 2 * grid + 1: two to three chunks each) -- against float64 autograd, the grid asserted through the plan query."""
    n_cus = cus(cuda_device)
    seed = d + (M if isinstance(M, int) else len(M))
    deep = not isinstance(M, int)
    M, expected = einit_bwd_M(M, d, n_cus)
    plan = PR.einit_bwd_plan(M, d, n_cus)
    assert plan == expected, (plan, expected)
    assert PR.reduce_slices(plan.grid) == (16 if deep else 1)
    g = generator(cuda_device, seed)
    WC = torch.rand(M, 2, device=cuda_device, generator=g)
    dE0 = randn(g, M, d)
    Ws, bs, wb = einit_params(d, seed)
    tW = [torch.tensor(w, dtype=torch.float64, device=cuda_device, requires_grad=True) for w in Ws]
    tb = [torch.tensor(b, dtype=torch.float64, device=cuda_device, requires_grad=True) for b in bs]
    out, pres = einit_forward64(WC, tW, tb)
    kink = torch.zeros(M, dtype=torch.bool, device=cuda_device)
    for pre, band in pres:
        kink |= (pre.abs() < band).any(dim=1)
    quiet = int(kink.sum())
    assert quiet <= max(1, 1e-2 * M) and (M > 1 or quiet == 0), (quiet, M)
    dE0[kink] = 0.0
    grads = torch.autograd.grad((out * dE0.to(torch.float64)).sum(), [v for pair in zip(tW, tb) for v in pair])
    dwb0 = np.random.RandomState(seed + 1).randn(wb.size).astype(np.float32)
    ref = np.concatenate([host(gr).reshape(-1) for gr in grads]) + dwb0
    dwb = dev(np.concatenate([dwb0, np.full(SPARE, SENTINEL, np.float32)]), cuda_device)
    n_ws = int(_lib.lib.tspgnn_einit_bwd_workspace_floats(M, d))
    assert n_ws == PR.einit_bwd_workspace_floats(M, d) >= plan.grid * PR.einit_np(d)
    ws = empty((n_ws + SPARE,), cuda_device, SENTINEL)
    _lib.call("tspgnn_einit_bwd_f32", _lib.ptr(WC), _lib.ptr(dev(wb, cuda_device)), _lib.ptr(dE0), _lib.ptr(dwb), _lib.ptr(ws),
              M, d, None)
    torch.cuda.synchronize()
    assert intact(dwb, wb.size) and intact(ws, n_ws)
    e = rel_err(host(dwb[:wb.size]), ref)
    print(" einit_bwd d=%d [%d edges, %d quiet, grid %d, %d..%d chunks] %.1e" % (d, M, quiet, plan.grid, plan.lo, plan.hi, e), end="")
    assert e < TOL


# ---------------------------------------------------------------------------------------------- tspgnn_wcolsum_f32
COLSUM_S = {1: 1, 1023: 1, 1024: 1, 1025: 1, 8 * 1024 + 1: 4, 64 * 1024 + 1: 16, "cap": 16}


@pytest.mark.parametrize("d,rows", [(d, r) for d in (4, 32, 64, 128, 256, 1024) for r in list(COLSUM_S)[:-1]] + [(32, "cap")])
def test_wcolsum_chunks_and_slices_vs_float64(cuda_device, d, rows):
    """out += scale sum_r wt[r] X[r, :] and out_wsum += scale sum_r wt[r] over 1, 2, 9, 65 chunks (reduce_partials at S = 1,
    1, 4, 16) and, at d = 32, over the capped 4 * CUs chunks of 1025 rows; RS = 1024 / d rows in flight per workgroup; with
    and without wt, with and without out_wsum."""
    n_cus = cus(cuda_device)
    want_S = COLSUM_S[rows]
    rows = 1024 * 4 * n_cus + 1 if rows == "cap" else rows
    plan = PR.colsum_plan(rows, n_cus)
    assert PR.reduce_slices(plan.n_chunks) == want_S and plan.capped == (rows > 1024 * 4 * n_cus), plan
    if plan.capped:
        assert plan.n_chunks == 4 * n_cus and plan.chunk_rows == 1025 and plan.last_rows == 2, plan
    assert plan.n_chunks == (rows + plan.chunk_rows - 1) // plan.chunk_rows and 0 < plan.last_rows <= plan.chunk_rows
    RS = PR.colsum_rows_in_flight(d)
    g = generator(cuda_device, d + rows % 1000)
    X, wt = randn(g, rows, d), randn(g, rows)
    X64, wt64 = X.to(torch.float64), wt.to(torch.float64)
    out0 = np.random.RandomState(d).randn(d).astype(np.float32)
    scale = 0.125
    n_ws = int(_lib.lib.tspgnn_wcolsum_workspace_floats(rows, d))
    assert n_ws == PR.wcolsum_workspace_floats(rows, d, n_cus)
    for with_wt in (False, True):
        ref = out0 + scale * host(wt64 @ X64 if with_wt else X64.sum(0))
        for with_wsum in (False, True):
            out = dev(np.concatenate([out0, np.full(SPARE, SENTINEL, np.float32)]), cuda_device)
            wsum0 = 0.0 if with_wt else 0.25
            wsum = dev(np.concatenate([[wsum0], np.full(SPARE, SENTINEL)]), cuda_device)
            ws = empty((n_ws + SPARE,), cuda_device, SENTINEL)
            _lib.call("tspgnn_wcolsum_f32", _lib.ptr(X), _lib.ptr(wt) if with_wt else None, rows, d, scale, _lib.ptr(out),
                      _lib.ptr(wsum) if with_wsum else None, _lib.ptr(ws), None)
            torch.cuda.synchronize()
            assert intact(out, d) and intact(wsum, 1) and intact(ws, n_ws)
            e = rel_err(host(out[:d]), ref)
            print(" wcolsum d=%d [%d rows, %d chunks]%s%s %.1e" % (d, rows, plan.n_chunks, " wt" * with_wt, " wsum" * with_wsum, e), end="")
            assert e < TOL
            got = float(wsum[0].item())
            if not with_wsum:
                assert got == wsum0
            elif not with_wt:            # sums of ones: every step exact
                assert got == wsum0 + scale * rows, (got, rows)
            else:                        # (wsum0 = 0 and scale a power of two: got / scale is the kernel's sum itself)
                bar = ((plan.chunk_rows + RS - 1) // RS + RS + 2) * EPS * float(wt64.abs().sum())
                err = abs(got / scale - float(wt64.sum()))
                print(" wsum %.2f of the bar" % (err / bar), end="")
                assert err <= bar, (err, bar)


# ----------------------------------------------------------------- tspgnn_tile_rows_f32, tspgnn_rowdot_bwd_f32
@pytest.mark.parametrize("rows,d", [(1, 4), (16400, 256)])
def test_tile_rows_and_rowdot_bwd_bit_for_bit(cuda_device, rows, d):
    """Y[r, :] = scale v and dX[r, :] = dy[r] w: one fp32 multiply per element, so bit for bit the NumPy float32 product --
    at 16 400 x 256 through the second trip of the grid-stride loops (more than 4096 workgroups' worth of float4s)."""
    assert PR.strided_blocks(rows * (d // 4), 4096) == ((4096, True) if rows > 1 else (1, False))
    rng = np.random.RandomState(rows + d)
    v, w, dy = (rng.randn(n).astype(np.float32) for n in (d, d, rows))
    scale = 0.3
    Y, dX = empty((rows + SPARE, d), cuda_device, SENTINEL), empty((rows + SPARE, d), cuda_device, SENTINEL)
    _lib.call("tspgnn_tile_rows_f32", _lib.ptr(dev(v, cuda_device)), scale, _lib.ptr(Y), rows, d, None)
    _lib.call("tspgnn_rowdot_bwd_f32", _lib.ptr(dev(dy, cuda_device)), _lib.ptr(dev(w, cuda_device)), _lib.ptr(dX), rows, d, None)
    torch.cuda.synchronize()
    assert intact(Y, rows) and intact(dX, rows)
    assert np.array_equal(Y[:rows].cpu().numpy(), np.tile(v * np.float32(scale), (rows, 1)))
    assert np.array_equal(dX[:rows].cpu().numpy(), dy[:, None] * w[None, :])


# ------------------------------------------------------------------------------------------------ tspgnn_rowdot_f32
@pytest.mark.parametrize("d", [32, 64, 128, 256, 4, 20, 48, 512])
def test_rowdot_every_kernel_vs_float64(cuda_device, d):
    """y[r] = X[r, :] . w + b on rowdot_kernel<d / 4> (d = 32, 64, 128, 256: d / 4 lanes per row, the last row count of a
    workgroup and the first of the next) and on rowdot_generic_kernel (any other d), elementwise at the derived bar."""
    worst = 0.0
    for rows in (1, 3, 4, 5, 255, 256, 257, 70001):
        g = generator(cuda_device, d + rows)
        X, w = randn(g, rows, d), randn(g, d)
        b = dev(np.array([0.3], np.float32), cuda_device)
        y = empty((rows + SPARE,), cuda_device, SENTINEL)
        _lib.call("tspgnn_rowdot_f32", _lib.ptr(X), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), rows, d, None)
        torch.cuda.synchronize()
        assert intact(y, rows)
        X64, w64, b64 = X.to(torch.float64), w.to(torch.float64), float(b.item())
        bar = (d + 2) * EPS * (X64.abs() @ w64.abs() + abs(b64))
        ratio = float(((y[:rows].to(torch.float64) - (X64 @ w64 + b64)).abs() / bar).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (rows, ratio)
    print(" rowdot d=%d %.3f of the bar" % (d, worst), end="")


# --------------------------------------------------------------------------------------------- tspgnn_einit_fwd_f32
@pytest.mark.parametrize("M", [1, 15, 16, 17, 255, 256, 257, 70001])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_einit_fwd_tile_and_workgroup_edges_vs_float64(cuda_device, d, M):
    """E0 = E_init_MLP([W, C]) around the 16-edge tile and the 256-edge workgroup, and at 70 001 edges (274 workgroups, the
    last with 113 edges: seven full tiles and one of one edge); rows >= M are left alone."""
    g = generator(cuda_device, d + M)
    WC = torch.rand(M, 2, device=cuda_device, generator=g)
    Ws, bs, wb = einit_params(d, d + M, bias=0.1)
    E0 = empty((M + SPARE, d), cuda_device, SENTINEL)
    _lib.call("tspgnn_einit_fwd_f32", _lib.ptr(WC), _lib.ptr(dev(wb, cuda_device)), _lib.ptr(E0), M, d, None)
    torch.cuda.synchronize()
    assert intact(E0, M)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=cuda_device)
    ref = host(einit_forward64(WC, [t64(w) for w in Ws], [t64(b) for b in bs])[0])
    got = host(E0[:M])
    whole, rowwise = rel_err(got, ref), row_err(got, ref)
    print(" einit_fwd d=%d [%d edges] whole %.1e row %.1e" % (d, M, whole, rowwise), end="")
    assert whole < F32_TOL and rowwise < ROW_TOL, (whole, rowwise)


# --------------------------------------------------------------- tspgnn_segment_mean_f32, tspgnn_vote_grad_f32
SEGMENTS = [0, 1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 2047, 2048, 2049, 19900, 0]


@pytest.mark.parametrize("lengths", [SEGMENTS, [1000]], ids=["edges_of_the_four_chain_loop", "B1"])
def test_segment_mean_and_vote_grad_at_the_loop_edges(cuda_device, lengths):
    """Per-problem mean of the votes and its adjoint over segments one short of, at and one past 256, 768, 1024 and 2048 (the
    four-chain loop runs while k + 768 < end), an empty segment first and last (mean 0 / 0 = NaN; vote_grad writes nothing
    for it), and a single segment."""
    B = len(lengths)
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    total = int(seg[-1])
    g = generator(cuda_device, B)
    vote = randn(g, total)
    segd = dev(seg, cuda_device, np.int32)
    logits = empty((B + SPARE,), cuda_device, SENTINEL)
    _lib.call("tspgnn_segment_mean_f32", _lib.ptr(vote), _lib.ptr(segd), _lib.ptr(logits), B, None)
    torch.cuda.synchronize()
    assert intact(logits, B)
    got, v64 = host(logits[:B]), host(vote)
    worst = 0.0
    for p, n in enumerate(lengths):
        if n == 0:
            assert np.isnan(got[p]), (p, got[p])
            continue
        s = v64[seg[p]:seg[p + 1]]
        bar = ((n + 1023) // 1024 + 12) * EPS * np.abs(s).sum() / n
        worst = max(worst, abs(got[p] - s.mean()) / bar)
        assert abs(got[p] - s.mean()) <= bar, (p, n, got[p], s.mean(), bar)
    print(" segment_mean %.3f of the bar" % worst, end="")
    # the adjoint, from finite logits; SPARE sentinels before the first vote and behind the last
    # (|logit| ~ 0.5: sigmoid - label stays away from the cancellation that would turn the hardware sigmoid's 2e-7 into
    # more than the bar; the loops under test do not depend on the value)
    lg = (0.5 * np.random.RandomState(B).randn(B)).astype(np.float32)
    lab = (np.arange(B) % 2).astype(np.float32)
    buf = empty((SPARE + total + SPARE,), cuda_device, SENTINEL)
    _lib.call("tspgnn_vote_grad_f32", _lib.ptr(dev(lg, cuda_device)), _lib.ptr(dev(lab, cuda_device)), _lib.ptr(segd),
              _lib.ptr(buf[SPARE:]), B, None)
    torch.cuda.synchronize()
    assert bool(buf[:SPARE].eq(SENTINEL).all()) and bool(buf[SPARE + total:].eq(SENTINEL).all())
    dvote = host(buf[SPARE:SPARE + total])
    sig = 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))
    for p, n in enumerate(lengths):
        if n:
            want = (sig[p] - lab[p]) / (B * n)
            assert np.abs(dvote[seg[p]:seg[p + 1]] - want).max() < 1e-6 * abs(want), (p, n)


# ------------------------------------------------------------------------------------------- tspgnn_bce_metrics_f32
@pytest.mark.parametrize("B", [1, 255, 256, 257, 1000, 4099])
def test_bce_metrics_over_a_full_workgroup_and_more(cuda_device, B):
    """sigmoid, mean cross entropy and the confusion counts of B problems in the one workgroup: up to 17 problems per thread,
    every one of the 256 partials non-zero from B = 256 on.  Logits N(0, 2^2) kept 1e-3 away from zero (p = 0.5 +- 2.5e-4
    rounds the same way in fp32 and float64), plus exact zeros with both labels (p = 0.5 rounds half to even, to 0)."""
    rng = np.random.RandomState(B)
    x = (2.0 * rng.randn(B)).astype(np.float32)
    x = np.where(np.abs(x) < 1e-3, np.float32(1e-3) * np.where(x < 0, -1, 1), x).astype(np.float32)
    z = rng.randint(0, 2, B).astype(np.float32)
    nz = min(B, 6)
    x[:nz] = 0.0
    z[:nz] = [1, 0, 1, 0, 0, 1][:nz]
    pred = empty((B + SPARE,), cuda_device, SENTINEL)
    stats = empty((6 + SPARE,), cuda_device, SENTINEL)
    _lib.call("tspgnn_bce_metrics_f32", _lib.ptr(dev(x, cuda_device)), _lib.ptr(dev(z, cuda_device)), _lib.ptr(pred),
              _lib.ptr(stats), B, None)
    torch.cuda.synchronize()
    assert intact(pred, B) and intact(stats, 6)
    x64, z64 = x.astype(np.float64), z.astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-x64))
    eq = (z64 == np.rint(p)).astype(np.float64)
    counts = [eq.sum(), (z64 * eq).sum(), (z64 * (1 - eq)).sum(), ((1 - z64) * eq).sum(), ((1 - z64) * (1 - eq)).sum()]
    s = host(stats[:6])
    got_counts = [s[1] * B] + s[2:].tolist()
    assert abs(s[1] * B - counts[0]) <= 2 * EPS * max(counts[0], 1) and np.rint(s[1] * B) == counts[0], (s[1] * B, counts[0])
    assert s[2:].tolist() == counts[1:], (got_counts, counts)
    assert rel_err(host(pred[:B]), p) < 1e-6
    term = np.maximum(x64, 0) - x64 * z64 + np.log1p(np.exp(-np.abs(x64)))
    bar = (((B + 255) // 256 + 11) * EPS * np.abs(term).sum() + 4 * np.spacing(term.astype(np.float32)).astype(np.float64).sum()) / B
    err = abs(s[0] - term.mean())
    print(" bce B=%d loss %.3f of the bar" % (B, err / bar), end="")
    assert err <= bar, (err, bar)


# ------------------------------------------------------------------- tspgnn_bucket_pack_f32 / tspgnn_bucket_unpack_f32
@pytest.mark.parametrize("with_grad", [True, False])
def test_bucket_pack_unpack_beyond_the_grid_cap(cuda_device, with_grad):
    """The checks of test_gpu_kernels.test_bucket_pack_unpack at n = 2 * 1024 * 256 + 3: the grid is capped at 1024
    workgroups, so every thread scales two gradient elements and three threads a third."""
    n = 2 * 1024 * 256 + 3
    assert PR.strided_blocks(n, 1024) == (1024, True) and n > 2 * 1024 * 256
    rng = np.random.RandomState(n + 3)
    grads = [rng.randn(n).astype(np.float32) for _ in range(2)]
    stats = [np.array([0.7, 0.5, 3, 1, 2, 0], np.float32), np.array([0.4, 0.75, 1, 0, 5, 2], np.float32)]
    nb, flags = [6.0, 10.0], [4, 2]
    buckets = []
    for r in range(2):
        b = dev(np.concatenate([grads[r], np.full(10, 123.0, np.float32), np.full(SPARE, SENTINEL, np.float32)]), cuda_device)
        fl = dev(np.array([flags[r]], np.uint32), cuda_device, dtype=np.uint32)
        _lib.call("tspgnn_bucket_pack_f32", _lib.ptr(b), n, int(with_grad), nb[r], _lib.ptr(dev(stats[r], cuda_device)),
                  _lib.ptr(fl), None)
        torch.cuda.synchronize()
        assert intact(b, n + 10)
        got = b.cpu().numpy()[:n + 10]
        want_tail = np.array([nb[r], nb[r] * stats[r][0], nb[r] * stats[r][1], *stats[r][2:6],
                              flags[r] & 1, (flags[r] >> 1) & 1, (flags[r] >> 2) & 1], np.float32)
        assert np.array_equal(got[n:], want_tail)
        assert np.array_equal(got[:n], grads[r] * np.float32(nb[r]) if with_grad else grads[r])
        buckets.append(b)
    total = buckets[0][:n + 10] + buckets[1][:n + 10]
    total = dev(np.concatenate([total.cpu().numpy(), np.full(SPARE, SENTINEL, np.float32)]), cuda_device)
    st_out = dev(np.full(6, -1.0, np.float32), cuda_device)
    fl_out = dev(np.zeros(1, np.int32), cuda_device, dtype=np.int32)
    before = total.cpu().numpy()[:n + 10].copy()
    _lib.call("tspgnn_bucket_unpack_f32", _lib.ptr(total), n, int(with_grad), _lib.ptr(st_out), _lib.ptr(fl_out), None)
    torch.cuda.synchronize()
    assert intact(total, n + 10)
    got = total.cpu().numpy()[:n + 10]
    inv = np.float32(1.0) / np.float32(16.0)
    assert np.array_equal(got[:n], before[:n] * inv if with_grad else before[:n])
    assert np.array_equal(st_out.cpu().numpy(), np.concatenate([before[n + 1:n + 3] * inv, before[n + 3:n + 7]]))
    assert int(fl_out.item()) == 6
