"""Cases for the fused forward cell launches called directly (tests/test_gpu_cell_forward_edges.py):
tspgnn_lnlstm_mlp_fwd_multi_h2 (csrc/dense_h2.hip) and, wherever its entry accepts the task, tspgnn_lnlstm_mlp_fwd_multi_x3
(csrc/dense_x3.hip).  One task's operands, drawn as tests/test_gpu_split_kernels.py draws them, packed for the arithmetic;
every output buffer with SPARE rows of SENTINEL behind it (blocked and projected-message buffers: the pad rows of the last
16-row tile hold it too); a zeroed range_flag word; a float64 reference on the device.  The launchers' plan is asked of the library
in tests/plan_replay.py (cell_fwd_plan); FwdCell.plan() is the task's entry for it.

The blocked layouts are written from the comments of include/tspgnn.h, not from the kernels: the float4 (columns
16t + 4g .. +3) of row r of a [rows, W] array sits at float offset (((r/16) * W/16 + t) * 4 + g) * 64 + (r%16) * 4, in a
buffer of ceil(rows/16)*16 rows -- W = d for a blocked state, W = 4d for the projected messages (there written d/4 = W/16)."""
import numpy as np
import torch

from lstm_bwd_cases import GATES, SENTINEL, SPARE, _KEEP, dev, empty
from oracle import torch_oracle as TO
from plan_replay import cell_task
from tspgnn import _lib

ENTRY = {"h2": "tspgnn_lnlstm_mlp_fwd_multi_h2", "x3": "tspgnn_lnlstm_mlp_fwd_multi_x3"}
PIECES = {"h2": 2, "x3": 3}


def wscale(arith):
    """The factor the weights, a cell's z and the projected messages of this arithmetic carry."""
    return float(_lib.lib.tspgnn_h2_weight_scale()) if arith == "h2" else 1.0


def pad16(n):
    return (n + 15) // 16 * 16


def blocked_pack(a, fill=0.0):
    """Row-major [n, W] (device tensor) -> blocked by 16 rows, [pad16(n), W]; the pad rows hold `fill`."""
    n, w = a.shape
    flat = torch.full((pad16(n), w), fill, dtype=a.dtype, device=a.device)
    flat[:n] = a
    # (R, r, t, g, j) -> (R, t, g, r, j): offset (((R * W/16 + t) * 4 + g) * 16 + r) * 4 + j
    return flat.reshape(-1, 16, w // 16, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1, w).contiguous()


def blocked_unpack(b):
    """Inverse of blocked_pack: blocked [P, W], P a multiple of 16 -> row-major [P, W] (pad rows included)."""
    p, w = b.shape
    return b.reshape(p // 16, w // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(p, w).contiguous()


def packed(arith, W, device):
    """tspgnn_pack_weights_{h2,x3} of W as a byte tensor."""
    src = dev(W, device)
    out = torch.empty(PIECES[arith] * W.size * 2, dtype=torch.uint8, device=device)
    _KEEP.append(out)
    if arith == "h2":
        _lib.call("tspgnn_pack_weights_h2", _lib.ptr(src), _lib.ptr(out), W.shape[0], W.shape[1], None, None)
    else:
        _lib.call("tspgnn_pack_weights_x3", _lib.ptr(src), _lib.ptr(out), W.shape[0], W.shape[1], None)
    return out


def mlp_blocks(arith, layers, device):
    """{packed weights, bias (2^s b for h2)} per layer as one byte tensor: tspgnn_mlp_task.wb / tspgnn_cell_mlp_task.mlp_wb."""
    parts = []
    for W, b in layers:
        parts.append(packed(arith, W, device))
        parts.append(dev(wscale(arith) * b, device).view(torch.uint8))
    out = torch.cat(parts)
    _KEEP.append(out)
    return out


def t64(a, device):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=device)


def draw_mlp(rng, d, n_layers):
    return [((rng.randn(d, d) / np.sqrt(d)).astype(np.float32), (0.1 * rng.randn(d)).astype(np.float32))
            for _ in range(n_layers)]


def mlp64(x, layers, mask, device):
    """The Dense chain in float64 -> [output of every layer]."""
    outs = []
    for l, (W, b) in enumerate(layers):
        x = x @ t64(W, device) + t64(b, device)
        if (mask >> l) & 1:
            x = torch.relu(x)
        outs.append(x)
    return outs


class FwdCell(object):
    """One forward task.  mode: "plain" (z = [x | h] K), "gather" (z = Zx[u] + Zx[v] + h Kh, dx = 0) or "bias"
    (z = zscale zbias + [x | h] K, zscale = degrees 0 .. 39).  mlp_layers 0 .. 4 with relu_mask, mlp_out, a projection,
    mlp_acts ("default": dense, stride 0 -> rows * d; "strided": slot 1 of a [layers - 1, 2, rows + SPARE, d] array).
    in_blocked / out_blocked: the state layouts (h2).  null_c: c == NULL with the reference's c = 0.  inplace: h_out == h and
    c_out == c (the layouts of both sides must agree).  zbias_scale: zbias times this, and zscale = 1 on the last row."""

    def __init__(self, arith, d, rows, seed, dx=0, mode="plain", mlp_layers=0, relu_mask=None, mlp_out=True, proj=False,
                 acts=None, in_blocked=False, out_blocked=False, null_c=False, inplace=False, n_src=257, zbias_scale=1.0,
                 pad_fill=SENTINEL):
        # ("f32": tests/dense_fwd_cases.py builds the fp32 entry's task from the same draw and reference)
        assert arith in ("h2", "x3", "f32") and mode in ("plain", "gather", "bias") and not (mode == "gather" and dx)
        assert arith == "h2" or not (in_blocked or out_blocked or acts or null_c or inplace)
        assert not inplace or in_blocked == out_blocked
        rng = np.random.RandomState(seed)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.arith, self.d, self.dx, self.rows, self.mode = arith, d, dx, rows, mode
        self.h, self.c = f32(rng.randn(rows, d)), f32(rng.randn(rows, d))
        if null_c:
            self.c = np.zeros_like(self.c)
        self.K = f32(rng.randn(dx + d, 4 * d) / np.sqrt(dx + d))
        self.x = f32(rng.randn(rows, dx))
        self.ln = f32(np.stack([np.stack([1 + 0.2 * rng.randn(d), 0.2 * rng.randn(d)]) for _ in range(5)]))
        if mode == "gather":
            self.n_src = n_src
            self.uv = np.stack([rng.randint(0, n_src, rows), rng.randint(0, n_src, rows)], 1).astype(np.int32)
            self.Zx = f32(rng.randn(n_src, 4 * d))
        if mode == "bias":
            self.zbias, self.zscale = f32(rng.randn(4 * d)), f32(rng.randint(0, 40, rows))
            self.zscale[rows // 2] = 0.0          # a vertex without edges, at every row count
            if zbias_scale != 1.0:                # a folded bias far smaller than [x | h] K, and the last row of degree 1: what
                self.zbias, self.zscale[rows - 1] = f32(zbias_scale * self.zbias), 1.0     # a clamped lane would take as its z
        self.L = mlp_layers
        self.mask = ((1 << mlp_layers) - 1) if relu_mask is None else relu_mask
        self.layers = draw_mlp(rng, d, mlp_layers)
        self.P = f32(rng.randn(d, 4 * d) / np.sqrt(d)) if proj else None
        self.with_out = bool(mlp_out and mlp_layers)
        self.acts = acts if mlp_layers > 1 else None
        self.in_blocked, self.out_blocked, self.null_c, self.inplace = in_blocked, out_blocked, null_c, inplace
        self.z_centered, self.pad_fill = False, pad_fill
        self._ref = self._ops = None

    def centred(self):
        """Centres K, the projected messages (= the Kx behind them) and zbias per gate over its d columns, so that every
        row of z has zero mean over each gate and the task may truthfully promise z_centered.  The float64 reference of the
        centred operands is the same cell: LayerNorm subtracts the mean anyway."""
        d = self.d

        def per_gate(a):
            a = a.astype(np.float64).reshape(a.shape[0], 4, d)
            return np.ascontiguousarray((a - a.mean(axis=2, keepdims=True)).reshape(a.shape[0], 4 * d), dtype=np.float32)
        self.K = per_gate(self.K)
        if self.mode == "gather":
            self.Zx = per_gate(self.Zx)
        if self.mode == "bias":
            self.zbias = per_gate(self.zbias[None])[0]
        self.z_centered, self._ref, self._ops = True, None, None
        return self

    def plan(self):
        """This task for plan_replay.cell_fwd_plan."""
        return cell_task(self.rows, self.dx, self.L, self.P is not None, self.out_blocked, self.with_out, self.z_centered)

    # ------------------------------------------------------------------------------------------------------ the task
    def _state_in(self, a, device):
        t = dev(a, device)      # (SPARE rows behind an input too: in place it is the output)
        b = torch.cat([blocked_pack(t, self.pad_fill) if self.in_blocked else t, torch.full((SPARE, self.d), SENTINEL, device=device)])
        _KEEP.append(b)
        return b

    def _state_out(self, device):
        rows = pad16(self.rows) if self.out_blocked else self.rows
        return empty((rows + SPARE, self.d), device, SENTINEL)

    def task(self, device):
        """The tspgnn_cell_mlp_task; every output allocated with SPARE rows beyond its own and filled with SENTINEL."""
        d, rows, a = self.d, self.rows, self.arith
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        _KEEP.append(self.flag)
        h_in = self._state_in(self.h, device)
        c_in = None if self.null_c else self._state_in(self.c, device)
        if self.inplace:
            self.h_out, self.c_out = h_in, (c_in if c_in is not None else self._state_out(device))
        else:
            self.h_out, self.c_out = self._state_out(device), self._state_out(device)
        cell = dict(x=dev(self.x, device) if self.dx else None, dx=self.dx, h=h_in, c=c_in, K=packed(a, self.K, device),
                    ln=dev(self.ln, device), h_out=self.h_out, c_out=self.c_out, rows=rows, range_flag=self.flag,
                    z_centered=int(self.z_centered))
        if self.mode == "gather":
            Zx = dev(self.Zx, device)
            cell["uv"] = dev(self.uv, device, np.int32)
            cell["Zx"] = blocked_pack(Zx * wscale("h2")) if a == "h2" else Zx
            _KEEP.append(cell["Zx"])
        if self.mode == "bias":
            cell["zbias"], cell["zscale"] = dev(self.zbias, device), dev(self.zscale, device)
        f = dict(cell=_lib.LstmTask(**_lib.ptrs({k: v for k, v in cell.items() if v is not None})),
                 mlp_layers=self.L, relu_mask=self.mask, state_in_blocked=int(self.in_blocked),
                 state_out_blocked=int(self.out_blocked))
        self.mlp_out = self.proj_out = self.acts_buf = None
        if self.L:
            f["mlp_wb"] = mlp_blocks(a, self.layers, device)
            if self.with_out:
                f["mlp_out"] = self.mlp_out = empty((rows + SPARE, d), device, SENTINEL)
        if self.P is not None:
            f["proj_w"] = packed(a, self.P, device)
            f["proj_out"] = self.proj_out = empty(((pad16(rows) if a == "h2" else rows) + SPARE, 4 * d), device, SENTINEL)
        if self.acts == "default":
            self.acts_buf = empty(((self.L - 1) * rows + SPARE, d), device, SENTINEL)
            f["mlp_acts"], f["mlp_acts_stride"] = self.acts_buf, 0
        elif self.acts == "strided":
            self.acts_buf = empty((self.L - 1, 2, rows + SPARE, d), device, SENTINEL)
            f["mlp_acts"], f["mlp_acts_stride"] = self.acts_buf[0, 1], 2 * (rows + SPARE) * d
        return _lib.CellMlpTask(**_lib.ptrs({k: v for k, v in f.items() if v is not None}))

    # --------------------------------------------------------------------------------------------------- what came back
    def _state(self, t):
        """A state output as row-major rows (pad and spare rows included)."""
        return blocked_unpack(t) if self.out_blocked else t

    def _named(self):
        """-> [(name, row-major tensor with its rows beyond `rows`)] of everything the launch writes."""
        out = [("h", self._state(self.h_out)), ("c", self._state(self.c_out))]
        if self.mlp_out is not None:
            out.append(("msg", self.mlp_out))
        if self.proj_out is not None:
            out.append(("proj", blocked_unpack(self.proj_out) / wscale("h2") if self.arith == "h2" else self.proj_out))
        if self.acts == "default":
            out.append(("acts", self.acts_buf))
        elif self.acts == "strided":
            out += [("acts%d" % l, self.acts_buf[l, 1]) for l in range(self.L - 1)]
        return out

    def outputs(self):
        """-> {name: the task's rows, float32 on the device}.  "acts": [layers - 1, rows, d]."""
        out = {}
        for n, t in self._named():
            if n == "acts":
                out[n] = t[:(self.L - 1) * self.rows].reshape(self.L - 1, self.rows, self.d)
            elif n.startswith("acts"):
                out.setdefault("acts", []).append(t[:self.rows])
            else:
                out[n] = t[:self.rows]
        if isinstance(out.get("acts"), list):
            out["acts"] = torch.stack(out["acts"])
        return out

    def untouched(self):
        """Every row beyond the task's own -- the SPARE rows, the pad rows of a blocked or projected-message buffer's last
        tile, the other slot of a strided mlp_acts -- still holds SENTINEL (a projection's are stored unscaled: compared
        in the buffer itself)."""
        bad = []
        for n, t in self._named():
            rows = (self.L - 1) * self.rows if n == "acts" else self.rows
            if n == "proj" and self.arith == "h2":
                t = blocked_unpack(self.proj_out)
            if not bool(t[rows:].eq(SENTINEL).all()):
                bad.append(n)
        if self.acts == "strided" and not bool(self.acts_buf[:, 0].eq(SENTINEL).all()):
            bad.append("acts slot 0")
        return bad

    def unwritten(self):
        """Names of the outputs in which some row of the task still holds a SENTINEL (exactly 7.0 is no value of these
        operands)."""
        return [n for n, t in self.outputs().items() if bool(t.eq(SENTINEL).any())]

    def range_flag(self):
        return int(self.flag.item())

    # ------------------------------------------------------------------------------------------------------- reference
    def _z64(self, device):
        """z of every row in float64, from the stored fp32 operands."""
        z = torch.cat([t64(self.x, device), t64(self.h, device)], dim=1) @ t64(self.K, device)
        if self.mode == "gather":
            uv = torch.as_tensor(self.uv, dtype=torch.long, device=device)
            Zx = t64(self.Zx, device)
            z = z + Zx[uv[:, 0]] + Zx[uv[:, 1]]
        if self.mode == "bias":
            z = z + t64(self.zscale, device)[:, None] * t64(self.zbias, device)[None]
        return z

    def reference(self, device):
        """float64 on the device, from the stored fp32 operands: {h, c, msg, proj, acts} as outputs().  Computed once."""
        if self._ref is not None:
            return self._ref
        d = self.d
        z = self._z64(device)
        ln = t64(self.ln, device)
        base = "cell"
        params = {base + "/kernel": torch.eye(4 * d, dtype=torch.float64, device=device)}      # the cell's GEMM: z itself
        for i, g in enumerate(GATES):
            params[base + "/%s/gamma" % g], params[base + "/%s/beta" % g] = ln[i, 0], ln[i, 1]
        nh, nc = TO.lnlstm_cell(z, z[:, :0], t64(self.c, device), params, None, base=base)
        ref = {"h": nh, "c": nc}
        outs = mlp64(nh, self.layers, self.mask, device) if self.L else []
        if self.L:
            if self.with_out:
                ref["msg"] = outs[-1]
            if self.P is not None:
                ref["proj"] = outs[-1] @ t64(self.P, device)
            if self.acts:
                ref["acts"] = torch.stack(outs[:-1])
        # what the f16x2 range guard looks at (operands): every tensor a kernel splits, and the variance LayerNorm divides a
        # gate row by -- oracle/torch_oracle.layer_norm's, the biased one
        ops = {"h": t64(self.h, device)}
        if self.dx:
            ops["x"] = t64(self.x, device)
        for l, a in enumerate([nh] + outs[:-1] if self.L else []):
            ops["layer%d" % (l + 1)] = a          # layer 1 takes h', layer l + 1 the output of layer l
        if self.P is not None:
            ops["proj"] = outs[-1]
        zg = z.reshape(self.rows, 4, d)
        ops["var"] = ((zg - zg.mean(dim=2, keepdim=True)) ** 2).mean(dim=2)       # [rows, 4]: gates i, j, f, o
        self._ref, self._ops = ref, ops
        return ref

    def operands(self, device):
        """float64 (device "cpu" works), from the same stored fp32 operands as reference(): {site: tensor} of every tensor
        a kernel splits into fp16 pieces -- "x" (dx > 0), "h", "layer1" (h' into the fused MLP's first layer), "layer2" ..
        (the input of each later layer), "proj" (the projection's input) -- and "var": [rows, 4], per row the variance of z
        over each gate's d columns (i, j, f, o)."""
        self.reference(device)
        return self._ops
