"""Cases for the LN-LSTM cell backward kernels called directly (tests/test_gpu_h2_backward_kernels.py,
tests/test_gpu_bf16_backward_kernels.py): one task's inputs, its operands packed for an arithmetic, a float64 autograd
reference on the device, and the launchers' plans as the library answers them (tests/plan_replay.py), so that a test that
claims to reach a path (a second tile per wavefront, the chunked K) asserts that it does.  The device-buffer helpers (dev,
empty, release, SENTINEL, SPARE) and the row-by-row measure row_err also serve tests/test_gpu_fp32_backward_plans.py and tests/test_gpu_batch_kernels.py.

The arithmetic decides the packing of K / K^T, the form of the projected messages Zx, and the entry point:
  "h2"    tspgnn_lnlstm_bwd_multi_h2   (csrc/dense_bwd_h2.hip)    pack_weights_h2 of K and of K^T, Zx scaled and blocked
  "f32"   tspgnn_lnlstm_bwd_multi_f32  (csrc/dense_bwd.hip)       pack_weights_f32 (transposed=1 for K^T), Zx row-major
  "bf16"  tspgnn_lnlstm_bwd_multi_bf16 (csrc/dense_bwd_bf16.hip)  piece 0 of pack_weights_x3, bf16 x / h / blocked Zx
"""
import numpy as np
import torch

import plan_replay as PR
from conftest import h2_zx_pack
from oracle import torch_oracle as TO
from tspgnn import _lib

_KEEP = []          # device tensors the launched kernels still read or write; the test's fixture calls release()
GATES = ("input", "transform", "forget", "output", "state")
SENTINEL = 7.0      # what every output row holds before the launch
SPARE = 16          # rows allocated beyond `rows` in every output: a clamped lane must not write there
KINK = 2.0 ** -16


def release():
    torch.cuda.synchronize()
    del _KEEP[:]


def dev(a, device, dtype=np.float32):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
    _KEEP.append(t)
    return t


def dev_bf16(a, device):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(device)
    _KEEP.append(t)
    return t


def empty(shape, device, fill=None):
    t = torch.empty(shape, dtype=torch.float32, device=device) if fill is None else \
        torch.full(shape, fill, dtype=torch.float32, device=device)
    _KEEP.append(t)
    return t


def row_err(a, b):
    """max over the rows of max |a - b| / max |b| (each over the row); a row where b is all zero must be all zero in a."""
    scale = np.abs(b).max(axis=1)
    dead = scale == 0
    assert not a[dead].any(), "rows without a gradient: %d not exactly zero" % int(np.abs(a[dead]).max(axis=1).astype(bool).sum())
    if dead.all():
        return 0.0
    return float((np.abs(a - b).max(axis=1)[~dead] / scale[~dead]).max())


def rb(x):
    """Round to bf16 (nearest even), back in float32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def packed_f32(W, device, transposed=0):
    """tspgnn_pack_weights_f32 of W or, with transposed=1, of W^T straight from W as stored."""
    src = dev(W, device)
    out = empty(src.shape, device)
    kr, nc = (W.shape[1], W.shape[0]) if transposed else W.shape
    _lib.call("tspgnn_pack_weights_f32", _lib.ptr(src), _lib.ptr(out), kr, nc, transposed, None)
    return out


def packed_h2(W, device):
    """tspgnn_pack_weights_h2 (two fp16 pieces of 2^s W) as a byte tensor."""
    src = dev(W, device)
    out = torch.empty(4 * W.size, dtype=torch.uint8, device=device)
    _KEEP.append(out)
    _lib.call("tspgnn_pack_weights_h2", _lib.ptr(src), _lib.ptr(out), W.shape[0], W.shape[1], None, None)
    return out


def packed_bf16(W, device):
    """Piece 0 of tspgnn_pack_weights_x3 = W rounded to bf16 in MFMA fragment order (bytes)."""
    src = dev(W, device)
    out = torch.empty(3 * W.size * 2, dtype=torch.uint8, device=device)
    _KEEP.append(out)
    _lib.call("tspgnn_pack_weights_x3", _lib.ptr(src), _lib.ptr(out), W.shape[0], W.shape[1], None)
    return out[:W.size * 2]


def workspace(d, device):
    return empty((int(_lib.lib.tspgnn_lnlstm_bwd_workspace_floats(d)),), device, 0.0)


# ------------------------------------------------------------------------------ the launchers' plans, asked of the library
def k_chunked(d, dx):
    """Does tspgnn_lnlstm_bwd_multi_bf16 stream K through LDS in chunks (rather than keep it resident)?  The planner's answer
    (plan_replay.cell_bwd_plan); it does not depend on the rows or the CU count."""
    return PR.cell_bwd_plan([(16, dx, False, False)], d, 256, "bf16").chunked[0]


def k_resident_f32(d, dx, with_KT=False):
    """Does the whole of K stay in LDS in tspgnn_lnlstm_bwd_multi_f32 (else it is streamed in chunks of qc 16-row blocks, the
    tiles taken in rounds of nw)?  The planner's answer.  with_KT: K^T ([4d, dx + d] floats) has to fit beside a resident K,
    which the launcher grants only at d = 64, dx = 0 -- asserted: the planner accepts the task (it raises where the launch is
    refused) and answers a resident K."""
    chunked = PR.cell_bwd_plan([(16, dx, with_KT, False)], d, 256, "f32").chunked[0]
    if with_KT:
        assert not chunked
    return not chunked


def tiles_per_wavefront(tasks, d, cus, arith="h2"):
    """How many 16-row tiles each wavefront of a launch works through: -> per task (nw, workgroups, min, max), None for
    an empty task (dropped before the launch).  tasks: (rows, dx, with_KT, with_KTg) each -- Cell.plan().

    nw, the workgroups per task and whether K is chunked are the launcher's plan (plan_replay.cell_bwd_plan); what follows
    them here is the kernels' own walk: t_beg / t_end of a workgroup and the round-robin over its wavefronts (f32 with a
    chunked K: rounds of nw tiles, round r to workgroup r mod workgroups)."""
    assert arith in ("h2", "f32")
    live = [t for t in tasks if t[0] > 0]
    plan = PR.cell_bwd_plan(live, d, cus, arith)
    nw = plan.nw
    out = []
    for (rows, *_), blocks, ch in zip(live, plan.blocks, plan.chunked):
        n = PR.tiles16(rows)
        counts = []
        for b in range(blocks):
            if ch:
                rounds = range(b, (n + nw - 1) // nw, blocks)
                counts += [sum(1 for r in rounds if r * nw + w < n) for w in range(nw)]
            else:
                share = n * (b + 1) // blocks - n * b // blocks
                counts += [max(0, (share - w + nw - 1) // nw) for w in range(nw)]
        out.append((nw, blocks, min(counts), max(counts)))
    it = iter(out)
    return [next(it) if t[0] > 0 else None for t in tasks]


def plan_of(rows, dx, gather=False, fused=False):
    """One task for tiles_per_wavefront: (rows, dx, with_KT, with_KTg).  Cell.plan() is this of its own fields."""
    return (rows, dx, fused and gather, fused and not gather)


# --------------------------------------------------------------------------------------------------------- one task
class Cell(object):
    """One backward task: fp32 x, h, c, K, LayerNorm, dh', dc' (gather-init: Zx, uv and Kh in place of x and K; bias-init:
    zbias, zscale on top of x and K), drawn as the older direct tests draw them.  arith = "bf16" rounds x, h, K and Zx to
    bf16, which is what that kernel stores.

    fused: the data gradient formed in the launch -- gather-init: KT -> dxh = dz Kh^T; otherwise KTg -> dxg | dxh = dz K^T.
    row_spread: every row of dh', dc' times 10^U(-9, 3)."""

    def __init__(self, arith, d, dx, rows, seed, gather=False, bias_init=False, fused=False, null_grads=False, n_src=257,
                 row_spread=False):
        assert arith in ("h2", "f32", "bf16") and not (gather and (bias_init or dx))
        rng = np.random.RandomState(seed)
        self.arith, self.d, self.dx, self.rows = arith, d, dx, rows
        self.gather, self.bias_init, self.fused = gather, bias_init, fused
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        op = rb if arith == "bf16" else f32     # a GEMM operand as the arithmetic stores it
        self.h, self.c = op(rng.randn(rows, d)), f32(rng.randn(rows, d))
        if gather:
            self.n_src = n_src
            self.uv = np.stack([rng.randint(0, n_src, rows), rng.randint(0, n_src, rows)], 1).astype(np.int32)
            self.Zx = op(rng.randn(n_src, 4 * d))
            self.K = op(rng.randn(d, 4 * d) / np.sqrt(d))
        else:
            self.x = op(rng.randn(rows, dx))
            self.K = op(rng.randn(dx + d, 4 * d) / np.sqrt(dx + d))
        self.ln = f32(np.stack([np.stack([1 + 0.2 * rng.randn(d), 0.2 * rng.randn(d)]) for _ in range(5)]))
        self.dh, self.dc = (None, None) if null_grads else (f32(rng.randn(rows, d)), f32(rng.randn(rows, d)))
        if row_spread and not null_grads:
            row_scale = 10.0 ** rng.uniform(-9, 3, size=(rows, 1))
            self.dh, self.dc = f32(row_scale * self.dh), f32(row_scale * self.dc)
        if bias_init:
            self.zbias, self.zscale = f32(0.1 * rng.randn(1, 4 * d)), f32(rng.randint(1, 40, rows))

    def plan(self):
        """This task for tiles_per_wavefront."""
        return plan_of(self.rows, self.dx, self.gather, self.fused)

    def z64(self, device, x=None, h=None):
        """z = [x | h] K (+ Zx[u] + Zx[v], + zscale zbias) in float64 from the stored operand values themselves."""
        t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=device)
        h = t64(self.h) if h is None else h
        if self.gather:
            uv = torch.as_tensor(self.uv, dtype=torch.long, device=device)
            Zx = t64(self.Zx)
            return Zx[uv[:, 0]] + Zx[uv[:, 1]] + h @ t64(self.K)
        x = t64(self.x) if x is None else x
        z = torch.cat([x, h], dim=1) @ t64(self.K)
        if self.bias_init:
            z = z + t64(self.zscale)[:, None] * t64(self.zbias)
        return z

    def quiet_kinks(self, device):
        """Rows where a relu input -- the normalised transform gate j or the normalised cell state c' -- lies within 2^-16 of
        zero are a rounding away from the other side of the kink: the fp32 kernel and the float64 reference may take
        different derivatives there, and legitimately (measured: one row of 70 001 with |c'| = 3.7e-8 moved dz by 1e-2).
        Such rows get no incoming gradient (dh' = dc' = 0): they still pass through the kernel, and contribute exactly zero
        on both sides.  -> the number of rows quietened."""
        if self.dh is None:
            return 0
        d = self.d
        ln = torch.tensor(self.ln, dtype=torch.float64, device=device)
        i, j, f, o = torch.chunk(self.z64(device), 4, dim=1)
        i, j, f = (TO.layer_norm(g, ln[k, 0], ln[k, 1]) for k, g in enumerate((i, j, f)))
        c = torch.tensor(self.c, dtype=torch.float64, device=device)
        cn = TO.layer_norm(c * torch.sigmoid(f + TO.FORGET_BIAS) + torch.sigmoid(i) * torch.relu(j), ln[4, 0], ln[4, 1])
        kink = ((j.abs().min(dim=1).values < KINK) | (cn.abs().min(dim=1).values < KINK)).cpu().numpy()
        self.dh[kink] = 0.0
        self.dc[kink] = 0.0
        assert kink.sum() <= max(2, 1e-2 * self.rows), (d, int(kink.sum()))
        return int(kink.sum())

    def _operands(self, device):
        """-> the task's K, x, h, Zx, KT, KTg fields as this arithmetic wants them."""
        a, gather = self.arith, self.gather
        f = {}
        if a == "bf16":
            assert not (self.fused or self.bias_init)
            f["K"], f["h"] = packed_bf16(self.K, device), dev_bf16(self.h, device)
            if gather:    # the projected messages as Tape.ZX holds them: bf16, blocked by 16 rows
                f["Zx"] = dev_bf16(h2_zx_pack(self.Zx, 1.0), device)
            else:
                f["x"] = dev_bf16(self.x, device)
            return f
        f["h"] = dev(self.h, device)
        if not gather and self.dx:
            f["x"] = dev(self.x, device)
        if a == "h2":
            f["K"] = packed_h2(self.K, device)
            if gather:
                f["Zx"] = dev(h2_zx_pack(self.Zx, float(_lib.lib.tspgnn_h2_weight_scale())), device)
            if self.fused:
                f["KT" if gather else "KTg"] = packed_h2(np.ascontiguousarray(self.K.T), device)
        else:
            f["K"] = packed_f32(self.K, device)
            if gather:
                f["Zx"] = dev(self.Zx, device)
            if self.fused:
                assert gather
                f["KT"] = packed_f32(self.K, device, transposed=1)
        return f

    def task(self, device, ws=None, defer=False, ln_grad=None):
        """The tspgnn_lstm_bwd_task.  Every output is allocated with SPARE rows beyond `rows` and holds SENTINEL throughout
        (ln_grad, which a launch adds to: zeros, unless one is handed in)."""
        d, rows = self.d, self.rows
        if not hasattr(self, "quietened"):
            self.quietened = self.quiet_kinks(device)
        self.dz, self.dc_in = empty((rows + SPARE, 4 * d), device, SENTINEL), empty((rows + SPARE, d), device, SENTINEL)
        self.ln_grad = empty((10 * d,), device, 0.0) if ln_grad is None else ln_grad
        self.ws = workspace(d, device) if ws is None else ws
        self.dxh = empty((rows + SPARE, d), device, SENTINEL) if self.fused else None
        self.dxg = empty((rows + SPARE, self.dx), device, SENTINEL) if self.fused and not self.gather else None
        f = self._operands(device)
        f.update(dx=self.dx, c=dev(self.c, device), ln=dev(self.ln, device), rows=rows, defer_reduce=int(defer),
                 dh_out=None if self.dh is None else dev(self.dh, device),
                 dc_out=None if self.dc is None else dev(self.dc, device),
                 dz=self.dz, dc_in=self.dc_in, ln_grad=self.ln_grad, workspace=self.ws, dxh=self.dxh, dxg=self.dxg)
        if self.gather:
            f["uv"] = dev(self.uv, device, np.int32)
        if self.bias_init:
            f["zbias"], f["zscale"] = dev(self.zbias, device), dev(self.zscale, device)
        return _lib.LstmBwdTask(**_lib.ptrs({k: v for k, v in f.items() if v is not None}))

    def _outs(self):
        named = (("dz", self.dz), ("dc_in", self.dc_in), ("dxh", self.dxh), ("dxg", self.dxg))
        return [(n, t) for n, t in named if t is not None]

    def outputs(self):
        """-> [dz, dc_in, ln_grad] in float64 (the rows of the task)."""
        return [t.cpu().numpy().astype(np.float64) for t in (self.dz[:self.rows], self.dc_in[:self.rows], self.ln_grad)]

    def named_outputs(self):
        """-> {"dz", "dc_in", "ln_grad", and with the fused data gradient "dxh", "dxg"} in float64 (the rows of the task)."""
        out = {n: t[:self.rows].cpu().numpy().astype(np.float64) for n, t in self._outs()}
        out["ln_grad"] = self.ln_grad.cpu().numpy().astype(np.float64)
        return out

    def untouched(self, whole=False):
        """Do the SPARE rows beyond `rows` of every output (whole: all of every output) still hold SENTINEL?"""
        return all(bool((t if whole else t[self.rows:]).eq(SENTINEL).all()) for _, t in self._outs())

    def written(self):
        """Has the launch written every one of the task's rows in every output (none still holds SENTINEL)?"""
        return all(not bool(t[:self.rows].eq(SENTINEL).any()) for _, t in self._outs())

    def workspace_clear(self):
        """Is the LayerNorm-gradient workspace still all zero (nothing was launched)?"""
        return not bool(self.ws.any())

    def reference(self, device):
        """float64 autograd of TO.lnlstm_cell on z64 -> {dz, dc_in, ln_grad [10d], dxh = d/dh, dxg = d/dx (where dx > 0)}."""
        d = self.d
        t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=device)
        h = t64(self.h).requires_grad_(True)
        x = t64(self.x).requires_grad_(True) if not self.gather and self.dx else None
        z = self.z64(device, x=x, h=h)
        c, ln = t64(self.c).requires_grad_(True), t64(self.ln).requires_grad_(True)
        base = "TSP/Q_cell/layer_norm_basic_lstm_cell"
        params = {base + "/kernel": torch.eye(4 * d, dtype=torch.float64, device=device)}   # the cell's GEMM: z itself
        for i, g in enumerate(GATES):
            params[base + "/%s/gamma" % g] = ln[i, 0]
            params[base + "/%s/beta" % g] = ln[i, 1]
        nh, nc = TO.lnlstm_cell(z, torch.zeros((self.rows, 0), dtype=torch.float64, device=device), c, params, "Q")
        loss = (nh * t64(self.dh)).sum() + (nc * t64(self.dc)).sum()
        wrt = [z, c, ln, h] + ([x] if x is not None else [])
        g = [t.cpu().numpy() for t in torch.autograd.grad(loss, wrt)]
        ref = {"dz": g[0], "dc_in": g[1], "ln_grad": g[2].reshape(-1), "dxh": g[3]}
        if x is not None:
            ref["dxg"] = g[4]
        return ref
