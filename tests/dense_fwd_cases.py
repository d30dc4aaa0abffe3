"""Cases for the fp32-MFMA forward entries called directly (tests/test_gpu_fp32_forward_edges.py): tspgnn_mlp_fwd_multi_f32
and tspgnn_lnlstm_fwd_multi_f32 (csrc/dense.hip) and their one-task wrappers.  One task's operands -- the cell's drawn by
cell_fwd_cases.FwdCell, the MLP's by cell_fwd_cases.draw_mlp -- packed with lstm_bwd_cases.packed_f32; every output buffer
with SPARE rows of SENTINEL behind it (the other slot of a strided `acts` holds it too); a float64 reference on the device,
computed once per case.  The launchers' plans are asked of the library in tests/plan_replay.py (mlp_fwd_f32_plan,
lstm_fwd_f32_plan); plan() is the task's entry for them.

head(R) is the task of the first R rows alone, from the same operands: the kernels' per-row arithmetic must not depend on
the rows behind them or on the plan they bring about."""
import copy

import numpy as np
import torch

from cell_fwd_cases import FwdCell, draw_mlp, mlp64, t64
from lstm_bwd_cases import SENTINEL, SPARE, _KEEP, dev, empty, packed_f32
from tspgnn import _lib


class MlpF32(object):
    """One tspgnn_mlp_task of the fp32 entry: n_layers Dense layers of width d with relu_mask (default: every layer).
    acts: None, "dense" (stride 0 -> rows * d) or "strided" (slot 1 of a [layers - 1, 2, rows + SPARE, d] array); with one
    layer there is nothing to save and the whole buffer must stay SENTINEL.  proj: Y P, P [d, 4d], behind the last layer."""

    def __init__(self, d, rows, seed, n_layers=2, relu_mask=None, acts=None, proj=False):
        assert acts in (None, "dense", "strided")
        rng = np.random.RandomState(seed)
        self.d, self.rows, self.L = d, rows, n_layers
        self.mask = ((1 << n_layers) - 1) if relu_mask is None else relu_mask
        self.X = rng.randn(rows, d).astype(np.float32)
        self.layers = draw_mlp(rng, d, n_layers)
        self.P = (rng.randn(d, 4 * d) / np.sqrt(d)).astype(np.float32) if proj else None
        self.acts = acts
        self._ref = None

    def head(self, rows):
        """The first `rows` rows as a task of their own (same weights)."""
        t = copy.copy(self)
        t.rows, t.X, t._ref = rows, np.ascontiguousarray(self.X[:rows]), None
        return t

    def plan(self):
        """This task for plan_replay.mlp_fwd_f32_plan."""
        return (self.rows, self.L, self.P is not None)

    def fields(self, device):
        """The tspgnn_mlp_task's fields; every output allocated with SPARE rows beyond its own and filled with SENTINEL."""
        d, rows, L = self.d, self.rows, self.L
        wb = torch.cat([part for W, b in self.layers for part in (packed_f32(W, device).reshape(-1), dev(b, device))])
        _KEEP.append(wb)
        self.Y = empty((rows + SPARE, d), device, SENTINEL)
        f = dict(X=dev(self.X, device), wb=wb, Y=self.Y, rows=rows, n_layers=L, relu_mask=self.mask)
        self.acts_buf = self.proj_out = None
        if self.acts == "dense":
            self.acts_buf = empty((max(L - 1, 1) * rows + SPARE, d), device, SENTINEL)
            f["acts"], f["acts_stride"] = self.acts_buf, 0
        elif self.acts == "strided":
            self.acts_buf = empty((max(L - 1, 1), 2, rows + SPARE, d), device, SENTINEL)
            f["acts"], f["acts_stride"] = self.acts_buf[0, 1], 2 * (rows + SPARE) * d
        if self.P is not None:
            self.proj_out = empty((rows + SPARE, 4 * d), device, SENTINEL)
            f["proj_w"], f["proj_out"] = packed_f32(self.P, device), self.proj_out
        return f

    def task(self, device):
        return _lib.MlpTask(**_lib.ptrs(self.fields(device)))

    def _named(self):
        """-> [(name, tensor with its rows beyond the task's own, rows of the task in it)]."""
        out = [("Y", self.Y, self.rows)]
        if self.proj_out is not None:
            out.append(("proj", self.proj_out, self.rows))
        if self.acts == "dense":
            out.append(("acts", self.acts_buf, (self.L - 1) * self.rows))
        elif self.acts == "strided":
            out += [("acts%d" % l, self.acts_buf[l, 1], self.rows if l < self.L - 1 else 0) for l in range(max(self.L - 1, 1))]
        return out

    def outputs(self):
        """-> {name: the task's rows, float32 on the device}.  "acts": [layers - 1, rows, d], absent with one layer."""
        out = {}
        for n, t, rows in self._named():
            if not rows:
                continue
            if n == "acts":
                out[n] = t[:rows].reshape(self.L - 1, self.rows, self.d)
            elif n.startswith("acts"):
                out.setdefault("acts", []).append(t[:rows])
            else:
                out[n] = t[:rows]
        if isinstance(out.get("acts"), list):
            out["acts"] = torch.stack(out["acts"])
        return out

    def untouched(self):
        """Names of the buffers in which a row beyond the task's own -- the SPARE rows, the other slot of a strided acts, all
        of acts with one layer -- no longer holds SENTINEL."""
        bad = [n for n, t, rows in self._named() if not bool(t[rows:].eq(SENTINEL).all())]
        if self.acts == "strided" and not bool(self.acts_buf[:, 0].eq(SENTINEL).all()):
            bad.append("acts slot 0")
        return bad

    def unwritten(self):
        """Names of the outputs in which some row of the task still holds a SENTINEL (exactly 7.0 is no value of these
        operands)."""
        return [n for n, t in self.outputs().items() if bool(t.eq(SENTINEL).any())]

    def all_sentinel(self):
        """Does every output buffer still hold SENTINEL everywhere (nothing was launched)?"""
        return all(bool(t.eq(SENTINEL).all()) for t in (self.Y, self.acts_buf, self.proj_out) if t is not None)

    def reference(self, device):
        """float64 on the device, from the stored fp32 operands: {Y, acts, proj} as outputs().  Computed once."""
        if self._ref is None:
            outs = mlp64(t64(self.X, device), self.layers, self.mask, device)
            ref = {"Y": outs[-1]}
            if self.acts and self.L > 1:
                ref["acts"] = torch.stack(outs[:-1])
            if self.P is not None:
                ref["proj"] = outs[-1] @ t64(self.P, device)
            self._ref = ref
        return self._ref


class CellF32(FwdCell):
    """One tspgnn_lstm_task of the fp32 entry: FwdCell's draw, modes ("plain", "gather", "bias"; zscale = 0 on some rows) and
    float64 reference, the operands row-major fp32 and K through tspgnn_pack_weights_f32."""

    def __init__(self, d, rows, seed, dx=0, mode="plain", n_src=257):
        FwdCell.__init__(self, "f32", d, rows, seed, dx=dx, mode=mode, n_src=n_src)

    def head(self, rows):
        """The first `rows` rows as a task of their own (same K, LayerNorm, Zx, zbias)."""
        t = copy.copy(self)
        t.rows, t._ref, t._ops = rows, None, None
        for name in ("h", "c", "x", "uv", "zscale"):
            if hasattr(self, name):
                setattr(t, name, np.ascontiguousarray(getattr(self, name)[:rows]))
        return t

    def padded(self, dx):
        """The same rows with x widened to dx columns by zeros, and zero rows of K beneath x's: the same z."""
        t = copy.copy(self)
        extra = dx - self.dx
        t.dx, t._ref, t._ops = dx, None, None
        t.x = np.ascontiguousarray(np.concatenate([self.x, np.zeros((self.rows, extra), np.float32)], axis=1))
        t.K = np.ascontiguousarray(np.concatenate([self.K[:self.dx], np.zeros((extra, 4 * self.d), np.float32), self.K[self.dx:]]))
        return t

    def plan(self):
        """This task for plan_replay.lstm_fwd_f32_plan."""
        return (self.rows, self.dx, self.mode)

    def fields(self, device):
        """The tspgnn_lstm_task's fields; h_out and c_out allocated with SPARE rows beyond `rows`, filled with SENTINEL."""
        d, rows = self.d, self.rows
        self.h_out, self.c_out = empty((rows + SPARE, d), device, SENTINEL), empty((rows + SPARE, d), device, SENTINEL)
        self.mlp_out = self.proj_out = self.acts_buf = None
        f = dict(dx=self.dx, h=dev(self.h, device), c=dev(self.c, device), K=packed_f32(self.K, device), ln=dev(self.ln, device),
                 h_out=self.h_out, c_out=self.c_out, rows=rows)
        if self.dx:
            f["x"] = dev(self.x, device)
        if self.mode == "gather":
            f["uv"], f["Zx"] = dev(self.uv, device, np.int32), dev(self.Zx, device)
        if self.mode == "bias":
            f["zbias"], f["zscale"] = dev(self.zbias, device), dev(self.zscale, device)
        return f

    def task(self, device):
        return _lib.LstmTask(**_lib.ptrs(self.fields(device)))

    def all_sentinel(self):
        """Do h_out and c_out still hold SENTINEL everywhere (nothing was launched)?"""
        return bool(self.h_out.eq(SENTINEL).all()) and bool(self.c_out.eq(SENTINEL).all())
