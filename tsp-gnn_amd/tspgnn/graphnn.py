"""``GraphNN``: the typed-graph recurrent message-passing engine with the reference's
constructor / call contract (/root/reference/graphnn.py:4-272), running on hand-written HIP
kernels (libtspgnn.so) instead of TensorFlow ops.

Per time step and per variable v (graphnn.py:142-173), for each entry of loop[v]:
    y = states[var].h  ->  optional fun(y)  ->  optional msg MLP  ->  optional mat (x) y
the entries are concatenated on axis 1 and fed to v's LayerNorm-LSTM cell; every update reads
the OLD states (synchronous update, graphnn.py:143).  The adjacency product never touches a
dense matrix: matrices are kept as CSR (both orientations) on the device and multiplied by the
aggregation kernels; a 0/1 matrix with exactly two ones per row (the TSP EV matrix) takes the
gather path.
"""
from collections import namedtuple
from types import SimpleNamespace

import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import loop_plan
from . import resident_plan
from . import variables as V
from .instance_loader import SparseEV
from .mlp import Mlp, wgrad

# Field order of tf.contrib.rnn.LSTMStateTuple is (c, h); the reference constructs it by keyword
# (graphnn.py:138).
LSTMStateTuple = namedtuple("LSTMStateTuple", ("c", "h"))

LN_GATES = ("input", "transform", "forget", "output", "state")


# GraphNN.gemm -> suffix of the split-operand entry points (None: the fp32-MFMA kernels) and bytes per packed weight
GEMM_ARITH = {"f16x2": "h2", "bf16x3": "x3", "f32": None}
SPLIT_BYTES = {"x3": 6, "h2": 4}
# LayerNormBasicLSTMCell.packed: form -> (split arithmetic of the pack kernel, None = fp32 fragment order; transposed)
PACK_FORMS = {"f32": (None, False), "f32T": (None, True), "x3": ("x3", False), "h2": ("h2", False), "h2T": ("h2", True),
              "bf16": ("x3", False), "bf16T": ("x3", True)}


def _pad16(rows):
    """Row count of a projected-message buffer of the f16x2 kernels (blocked by 16 source rows, include/tspgnn.h)."""
    return (int(rows) + 15) // 16 * 16


def to_storage(x, dtype, out=None):
    """``x`` (fp32) in the storage type of the embeddings: itself for fp32, rounded to bf16 (nearest even) by the library's
    own kernel on the device (tspgnn_convert_f32_to_bf16) -- torch only converts on the CPU plumbing path."""
    if dtype == torch.float32 or x.dtype == dtype:
        x = x.contiguous()
        if out is None:
            return x
        out.copy_(x)
        return out
    if dtype == torch.bfloat16 and x.is_cuda and x.dtype == torch.float32:
        x = x.contiguous()
        if out is None:
            out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        _lib.call("tspgnn_convert_f32_to_bf16", _lib.ptr(x), _lib.ptr(out), x.numel(), _lib.current_stream())
        return out
    y = x.to(dtype).contiguous()
    if out is None:
        return y
    out.copy_(y)
    return out


def to_f32(x):
    """Stored embeddings as fp32 (bf16 storage: widened once by tspgnn_convert_bf16_to_f32)."""
    if x.dtype == torch.float32:
        return x
    if x.dtype == torch.bfloat16 and x.is_cuda and x.is_contiguous():
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _lib.call("tspgnn_convert_bf16_to_f32", _lib.ptr(x), _lib.ptr(out), x.numel(), _lib.current_stream())
        return out
    return x.to(torch.float32)


def _pack_split(store, arith, W, out, krows, ncols):
    """tspgnn_pack_weights_x3 / _h2 of W [krows, ncols] into the byte tensor ``out``; an f16x2 packing also raises the
    store's range guard's weight word to max |2^s W| (range_guard.py)."""
    if arith == "h2":
        _lib.call("tspgnn_pack_weights_h2", _lib.ptr(W), _lib.ptr(out), krows, ncols, store.guard.weight_ptr(),
                  _lib.current_stream())
    else:
        _lib.call("tspgnn_pack_weights_" + arith, _lib.ptr(W), _lib.ptr(out), krows, ncols, _lib.current_stream())


def _center_gates(K, d):
    """K [rows, 4d] with the mean over each gate's d columns subtracted per row (float64 arithmetic): LayerNorm's mean
    subtraction moved from every z row of every step into the weights (tspgnn_lstm_task.z_centered)."""
    k64 = K.to(torch.float64).reshape(K.shape[0], 4, d)
    return (k64 - k64.mean(dim=2, keepdim=True)).reshape(K.shape[0], 4 * d).to(torch.float32).contiguous()


def _check_cell_input(shape, rows, dx):
    if shape[0] != rows or shape[1] != dx:
        raise ValueError("cell input must be [%d,%d], got %s" % (rows, dx, tuple(shape)))


def _dev_i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


def loop_enabled():
    """The one-launch T-step loop (tspgnn_mp_loop_h2) is on unless TSPGNN_LOOP=0 (A/B runs, parity tests of the stepwise
    launches)."""
    return os.environ.get("TSPGNN_LOOP", "1") != "0"


def loop_kind():
    """Which one-launch form a batch may get: "auto" (default) = tspgnn_mp_loop_h2 (edge states in registers) for batches of
    <= loop_plan.max_edge_tiles() tiles per wavefront, tspgnn_mp_resident_h2 (edge states through memory, LDS ticket) for
    larger ones; TSPGNN_LOOP_KIND=loop / resident force one form (tests, A/B runs)."""
    return os.environ.get("TSPGNN_LOOP_KIND", "auto")


def choose_loop_plan(e_start, v_start, grid):
    """-> (plan int32 ndarray, meta) or None; meta = (n_groups, grid, kind, n_slots, lds_words, n_active), kind "loop"
    (loop_plan.py, tspgnn_mp_loop_h2) or "resident" (resident_plan.py, tspgnn_mp_resident_h2)."""
    kind = loop_kind()
    if kind in ("auto", "loop"):
        built = loop_plan.build(e_start, v_start, grid=grid)
        if built is not None:
            return built[0], (built[1], grid, "loop", 0, 0, 0)
    if kind in ("auto", "resident"):
        built = resident_plan.build(e_start, v_start, grid=grid)
        if built is not None and kind == "auto" and not resident_plan.in_auto_window(int(e_start[-1])):
            built = None
        if built is not None:
            return built["plan"], (built["n_groups"], grid, "resident", built["n_slots"], built["lds_words"],
                                   built["edge_wgs"] + built["vertex_wgs"])
    return None


def device_loop_plan(e_start, v_start, device):
    """choose_loop_plan at the grid of ``device``: its compute units, rounded down to a multiple of 8."""
    grid = torch.cuda.get_device_properties(device).multi_processor_count
    grid -= grid % 8
    return choose_loop_plan(e_start, v_start, grid)


def _make_loop_plan(ev, device):
    """Work plan of the one-launch T-step loop for a SparseEV on a GPU: built where the batch is packed (host side, cached
    per block structure), uploaded with the adjacency -- a captured forward then serves any batch copied into its buffers
    (DeviceBatch.copy_from copies the plan too).  None: no GPU, switched off, or the batch does not fit a resident
    design.  -> (int32 device tensor, n_groups, grid, kind, n_slots, lds_words, n_active)."""
    dev = torch.device(device)
    if dev.type != "cuda" or not loop_enabled() or ev.shape[0] == 0:
        return None
    blocks = getattr(ev, "blocks", None)
    if blocks is None:
        blocks = loop_plan.block_structure(ev.uv, ev.shape[1])
        if blocks is None:
            return None
    built = device_loop_plan(blocks[0], blocks[1], dev)
    if built is None:
        return None
    plan, meta = built
    return (torch.from_numpy(plan).to(dev),) + meta


class _States(dict):
    """{var: LSTMStateTuple} as returned by GraphNN.__call__, carrying the scratch buffers its launch plan points at:
    the task structures hold raw device pointers, so the buffers must live as long as anything that may replay those
    launches -- a captured HIP graph keeps the outputs (Session.capture_forward's closure), hence the buffers, alive,
    independently of later calls that build other plans."""

    def __init__(self, states, keep):
        dict.__init__(self, states)
        self._keep = keep


class _Ends(object):
    """Where one message-passing step reads and writes: all that a step builder (GraphNN._split_step, _fused_step,
    _bf16_step) knows of its driver.  Inference makes one per parity of its ping-pong buffers (and per first / last step
    where those differ), training one per step from the Tape (GraphNN._tape_ends).  What a dict does not name is the
    builder's to allocate; it puts the buffer into the dict (msg, zx) or into ``keep``, so whoever keeps the _Ends keeps
    every buffer the step's tasks point at.
      src, dst         {var: LSTMStateTuple} the step reads / writes (src c None: the zero cell state, as a null pointer)
      rows             {var: rows of its states} (a blocked buffer is padded beyond them)
      blk_in, blk_out  {var: the src / dst state buffers are blocked by 16 rows}; not named: row-major
      zx               {var: the projected messages Zx of a folded cell}
      x                {var: where the cell input goes} (training: the tape's X[v][t])
      msg              {(var, i): where loop entry i's message goes} (training: the tape's X or the extra acts slot).  Once
                       the messages are built it holds EVERY entry's rows -- the source h or 'fun' of it, the appended
                       matrix, the message -- which is what the cell inputs are made of
      acts             {(var, i): (hidden-activation slice [layers-1, rows, d], element stride between layers)}, training"""

    def __init__(self, src, dst, rows=None, blk_in=None, blk_out=None, zx=None, x=None, msg=None, acts=None):
        self.src, self.dst = src, dst
        self.rows = rows if rows is not None else {v: st.h.shape[0] for v, st in src.items()}
        self.blk_in, self.blk_out = blk_in or {}, blk_out or {}
        self.zx, self.x, self.acts = {} if zx is None else zx, x or {}, acts or {}
        self.msg = {} if msg is None else msg
        self.keep = []


def _launch_ops(name, by_width):
    """_lib.launches(by_width) of entry point ``name`` as (fn, args) operations, like the adjacency products between them."""
    return [(_lib.call_multi, (name, tasks, d)) for tasks, d in _lib.launches(by_width)]


def _run(parts):
    """Run a step: ``parts`` = lists of (fn, args) in order.  A builder (a generator) builds a part only when asked for it,
    so an eager driver, which hands the generator itself, has run a part before the next one is built -- the weight
    packings of the cell tasks are enqueued behind the adjacency products; a plan keeps list(builder) and replays it."""
    for ops in parts:
        for fn, args in ops:
            fn(*args)


class Tape(object):
    """What GraphNN.forward_train keeps for the backward pass: every step's states H, C ([T+1, rows, d]), cell inputs
    X (for a folded cell: the message y per SOURCE row, with ZX = y Kx), hidden MLP activations acts
    ([layers-1, T, rows, d]; one more slot for the output of a chain that ends in a relu and feeds an adjacency product,
    GraphNN._message_output_slot).  fp32 in the default mode; in the bf16-storage mode H, X, ZX, acts are the bf16 arrays
    the forward stored (C stays fp32) and the accessors below widen a step -- or a range of steps for the weight
    gradients -- to the fp32 operands the backward kernels take."""

    def __init__(self):
        self.arith = None    # the forward's arithmetic: "h2" (f16x2), "x3" (bf16x3), None (fp32 MFMA) or "bf16" (bf16 storage)
        self.folded = {}     # {var: its loop entry when the adjacency product is folded through the cell's kernel, else None}
        self.pushed = {}     # {var: the message MLP's last layer was pushed into the cell}
        self.rc = {}         # {(var, i): True when the backward recomputes this entry's hidden activations}
        self.fused = False   # the message MLPs of step t+1 ran in the cell launch of step t
        self.native = False  # bf16 tape consumed as it is by the bf16-reading backward kernels (no widened copies)

    def _f32(self, x):
        return x if (x.dtype == torch.float32 or self.native) else x.to(torch.float32)

    def h(self, v, t):
        return self._f32(self.H[v][t])

    def x(self, v, t):
        return self._f32(self.X[v][t])

    def zx(self, v, t):
        z = self.ZX[v][t]
        if z.dtype == torch.float32 or self.native:
            return z
        pad, w = z.shape     # bf16 projected messages, blocked by 16 rows (include/tspgnn.h) -> fp32 row-major
        return z.view(pad // 16, w // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(pad, w).to(torch.float32)

    def acts_at(self, key, t):
        """(hidden activations of step t [layers-1, rows, d], element stride between layers)."""
        a = self.acts[key]
        if a.dtype == torch.float32 or self.native:
            return a[:, t], a.stride(0)
        w = a[:, t].to(torch.float32)
        return w, w.stride(0)

    def h_steps(self, v, t0, t1):
        return self._f32(self.H[v][t0:t1]).reshape(-1, self.H[v].shape[2])

    def x_steps(self, v, t0, t1):
        return self._f32(self.X[v][t0:t1]).reshape(-1, self.X[v].shape[2])

    def acts_steps(self, key, layer, t0, t1):
        a = self.acts[key]
        return self._f32(a[layer, t0:t1]).reshape(-1, a.shape[3])


class DeviceAdjacency(object):
    """A sparse [R, C] matrix resident on the device in CSR, both orientations."""

    def __init__(self, shape, device, csr, csr_t, uv=None):
        self.shape = tuple(shape)
        self.device = device
        self.csr = csr      # (rowptr[R+1], col[nnz], val[nnz] or None)   rows of the matrix
        self.csr_t = csr_t  # same for the transpose
        self.uv = uv        # int32 [R,2] if the matrix is 0/1 with exactly two ones per row
        self._degrees = {}
        self.loop_plan = None   # (int32 device tensor, n_groups, grid, kind, n_slots, lds_words, n_active): _make_loop_plan

    def row_degrees(self, transpose=False):
        """Stored entries per row (of the transpose) as fp32, computed once per matrix."""
        if transpose not in self._degrees:
            rowptr = (self.csr_t if transpose else self.csr)[0]
            self._degrees[transpose] = (rowptr[1:] - rowptr[:-1]).to(torch.float32)
        return self._degrees[transpose]

    @staticmethod
    def from_sparse_ev(ev, device):
        rowptr, eid = ev.csr_by_vertex()
        M, N = ev.shape
        uv = _dev_i32(ev.uv, device)
        csr = (torch.arange(0, 2 * M + 1, 2, dtype=torch.int32, device=device), uv.view(-1), None)
        csr_t = (_dev_i32(rowptr, device), _dev_i32(eid, device), None)
        adj = DeviceAdjacency((M, N), device, csr, csr_t, uv=uv)
        adj.loop_plan = _make_loop_plan(ev, device)
        return adj

    @staticmethod
    def from_dense(mat, device):
        a = mat.detach().cpu().numpy() if torch.is_tensor(mat) else np.asarray(mat)
        if a.ndim != 2:
            raise ValueError("adjacency matrix must be 2-D")
        try:
            return DeviceAdjacency.from_sparse_ev(SparseEV.fromdense(a), device)
        except ValueError:
            pass

        def one(m):
            r, c = np.nonzero(m)
            vals = m[r, c].astype(np.float32)
            rowptr = np.zeros(m.shape[0] + 1, dtype=np.int64)
            np.cumsum(np.bincount(r, minlength=m.shape[0]), out=rowptr[1:])
            pattern = bool(np.all(vals == 1.0))
            v = None if pattern else torch.from_numpy(vals).to(device)
            return (_dev_i32(rowptr, device), _dev_i32(c, device), v)

        return DeviceAdjacency(a.shape, device, one(a), one(np.ascontiguousarray(a.T)))

    @staticmethod
    def wrap(mat, device):
        if isinstance(mat, DeviceAdjacency):
            return mat
        if isinstance(mat, SparseEV):
            return DeviceAdjacency.from_sparse_ev(mat, device)
        return DeviceAdjacency.from_dense(mat, device)

    def matmul(self, y, transpose=False, out=None):
        """mat (x) y  or  mat^T (x) y  (tf.matmul(..., adjoint_a=transpose), graphnn.py:156-160)."""
        R, C = self.shape
        rows_in = R if transpose else C
        rows_out = C if transpose else R
        if y.shape[0] != rows_in:
            raise ValueError("matrix/embedding size mismatch: %d vs %d" % (rows_in, y.shape[0]))
        d = y.shape[1]
        st = _lib.current_stream()
        if y.dtype == torch.bfloat16:   # bf16 rows, fp32 sums, one rounding at the store (pattern matrices only)
            if out is None:
                out = torch.empty((rows_out, d), dtype=torch.bfloat16, device=y.device)
            if not transpose and self.uv is not None:
                _lib.call("tspgnn_gather2_sum_bf16", _lib.ptr(self.uv), _lib.ptr(y), _lib.ptr(out), R, C, d, st)
                return out
            rowptr, col, val = self.csr_t if transpose else self.csr
            if val is not None:
                raise NotImplementedError("bf16 aggregation of a valued matrix")
            _lib.call("tspgnn_csr_rowsum_bf16", _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(y), _lib.ptr(out),
                      rows_out, rows_in, d, st)
            return out
        if d % 4 != 0:
            raise NotImplementedError("aggregation kernels need d %% 4 == 0 (got %d)" % d)
        if out is None:
            out = torch.empty((rows_out, d), dtype=torch.float32, device=y.device)
        if not transpose and self.uv is not None:
            _lib.call("tspgnn_gather2_sum_f32", _lib.ptr(self.uv), _lib.ptr(y), _lib.ptr(out), R, C, d, st)
            return out
        rowptr, col, val = self.csr_t if transpose else self.csr
        if val is None:
            _lib.call("tspgnn_csr_rowsum_f32", _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(y), _lib.ptr(out),
                      rows_out, rows_in, d, st)
        else:
            _lib.call("tspgnn_csr_spmm_f32", _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(y),
                      _lib.ptr(out), rows_out, rows_in, d, st)
        return out


class LayerNormBasicLSTMCell(object):
    """tf.contrib.rnn.LayerNormBasicLSTMCell(num_units, activation=relu) with its defaults
    (forget_bias=1, layer_norm=True, gain 1, shift 0, no dropout) -- graphnn.py:107-112.
    Variables: <scope>/layer_norm_basic_lstm_cell/kernel [dx+d,4d] (glorot uniform, TF's default
    initialiser), .../{input,transform,forget,output,state}/{gamma,beta}."""

    def __init__(self, num_units, input_size, scope, activation="relu", store=None):
        if getattr(activation, "__name__", activation) != "relu":
            raise NotImplementedError("LayerNormBasicLSTMCell: only activation=relu has a HIP kernel")
        self.d, self.dx = int(num_units), int(input_size)
        if self.d not in (32, 64, 128):
            raise NotImplementedError("LSTM width %d: HIP kernels exist for 32, 64, 128" % self.d)
        if self.dx % 16 != 0:
            raise NotImplementedError("LSTM input width %d must be a multiple of 16" % self.dx)
        self.store = store if store is not None else V.get_default_store()
        self.base = "%s/layer_norm_basic_lstm_cell" % scope
        self.store.declare(self.base + "/kernel", (self.dx + self.d, 4 * self.d), V.xavier_uniform)
        for g in LN_GATES:
            self.store.declare("%s/%s/gamma" % (self.base, g), (self.d,), V.ones_init)
            self.store.declare("%s/%s/beta" % (self.base, g), (self.d,), V.zeros_init)

    def kernel(self):
        return self.store.view(self.base + "/kernel")

    def packed(self, part, form, centered=False, pushed=None):
        """Kernel rows ``part`` ("K": all, "Kx": [0, dx), "Kh": [dx, dx+d)) in the byte layout ``form``, cached per weight
        version; the buffer is reused across versions (captured graphs hold its address).
          "f32": MFMA fragment order (tspgnn_pack_weights_f32); "f32T": of the transpose [4d, rows], by that kernel's flag
          "x3": three bf16 pieces (tspgnn_pack_weights_x3); "h2": two fp16 pieces of 2^s K (tspgnn_pack_weights_h2, which
                also raises the store's range guard word); "h2T": of the transposed rows
          "bf16" / "bf16T": rounded to bf16 in fragment order = piece 0 of the "x3" packing (of the transposed rows), a
                view of that buffer: one pack launch serves both
        ``centered``: each gate's columns centred first (_center_gates), a packing of its own.
        ``pushed`` = a message MLP: part "K" of the product K' = [W Kx ; Kh] (pushed_kernel) instead of the kernel."""
        arith, transposed = PACK_FORMS[form]
        lo, hi = {"K": (0, self.dx + self.d), "Kx": (0, self.dx), "Kh": (self.dx, self.dx + self.d)}[part]

        def build(out):
            K = self.kernel()[lo:hi] if pushed is None else self.pushed_kernel(pushed)[0]
            if centered:
                K = _center_gates(K, self.d)
            if arith is None:
                if out is None:
                    out = torch.empty_like(K)
                kr, nc = (4 * self.d, hi - lo) if transposed else (hi - lo, 4 * self.d)
                _lib.call("tspgnn_pack_weights_f32", _lib.ptr(K), _lib.ptr(out), kr, nc, int(transposed), _lib.current_stream())
                return out
            if transposed:
                K = K.t().contiguous()
            if out is None:
                out = torch.empty(SPLIT_BYTES[arith] * K.numel(), dtype=torch.uint8, device=K.device)
            _pack_split(self.store, arith, K, out, K.shape[0], K.shape[1])
            return out
        key = ("lstm", part, arith, transposed, centered, self.base, None if pushed is None else pushed.layer_names[-1])
        buf = self.store.packed(key, build)
        return buf[:buf.numel() // 3] if form.startswith("bf16") else buf

    def ln(self):
        return self.store.span(self.base + "/input/gamma", self.base + "/state/beta")

    def __call__(self, inputs, state, out=None):
        """Returns (new_h, LSTMStateTuple(new_c, new_h)) like the TF cell.  ``out`` = (h_out, c_out)
        lets the caller own the output buffers (training keeps every step's state)."""
        c, h = state.c, state.h
        rows = h.shape[0]
        _check_cell_input(inputs.shape, rows, self.dx)
        x = inputs if inputs.is_contiguous() else inputs.contiguous()
        h_out, c_out = out if out is not None else (torch.empty_like(h), torch.empty_like(c))
        _lib.call("tspgnn_lnlstm_fwd_f32", _lib.ptr(x), self.dx, _lib.ptr(h), _lib.ptr(c), _lib.ptr(self.packed("K", "f32")),
                  _lib.ptr(self.ln()), _lib.ptr(h_out), _lib.ptr(c_out), rows, self.d, _lib.current_stream())
        return h_out, LSTMStateTuple(c=c_out, h=h_out)

    # ------------------------------------------------------------------ backward
    def ln_grad(self):
        return self.store.grad_span(self.base + "/input/gamma", self.base + "/state/beta")

    # ------------------------------------------------------------------ folded adjacency product
    # (EV y) Kx = EV (y Kx): when the cell's only input is a gather over a two-ones-per-row matrix, the
    # x-half of the GEMM is applied on the (fewer) source rows and the cell kernel adds the two gathered
    # rows of Zx = y Kx to h Kh (tspgnn_lnlstm_gather_fwd_f32).
    def can_fold(self):
        return self.d == 64 and self.dx == 64

    def _forward_task(self, state, out, K, struct=_lib.LstmTask, **fields):
        """A tspgnn_lstm_task (``struct`` = _lib.LstmTaskB: tspgnn_lstm_task_bf16) over the rows of state.h, out = (h_out,
        c_out): the fields every form shares; the others by field name (tensors as their device pointers), zero where
        not named."""
        fields.setdefault("rows", state.h.shape[0])
        return struct(h=_lib.ptr(state.h), c=_lib.ptr(state.c), K=_lib.ptr(K), ln=_lib.ptr(self.ln()), h_out=_lib.ptr(out[0]),
                      c_out=_lib.ptr(out[1]), **_lib.ptrs(fields))

    def task_bf16(self, x, h, c, h_out, c_out, rows, adj=None, state_in_blocked=False, state_out_blocked=False):
        """tspgnn_lstm_task_bf16 over ``rows`` rows: x, h, h_out bf16; c, c_out fp32; the states blocked by 16 rows when
        flagged (padded buffers).  With adj, the gather-init form: x is the blocked bf16 Zx of the source rows, K = Kh."""
        form = dict(x=x, dx=self.dx) if adj is None else dict(uv=adj.uv, Zx=x)
        return self._forward_task(LSTMStateTuple(c=c, h=h), (h_out, c_out), self.packed("K" if adj is None else "Kh", "bf16"),
                                  struct=_lib.LstmTaskB, rows=rows, state_in_blocked=int(state_in_blocked),
                                  state_out_blocked=int(state_out_blocked), **form)

    def x3_ok(self):
        """The split-operand cell kernels cover this shape (tspgnn_lnlstm_fwd_multi_x3 / _h2)."""
        return self.d in (32, 64) and self.dx % 32 == 0

    def task(self, x, state, out, arith=None, centered=False):
        return self._forward_task(state, out, self.packed("K", arith or "f32", centered), x=x, dx=self.dx,
                                  range_flag=self._flag(arith), z_centered=int(centered))

    def gather_task(self, adj, zx, state, out, arith=None, centered=False):
        """``centered``: Kh AND the Kx behind zx were centred per gate (the caller projects with
        packed("Kx", arith, centered=True))."""
        return self._forward_task(state, out, self.packed("Kh", arith or "f32", centered), uv=adj.uv, Zx=zx,
                                  range_flag=self._flag(arith), z_centered=int(centered))

    def _flag(self, arith):
        """The range_flag of an f16x2 task (include/tspgnn.h): the store's guard's flags word."""
        return self.store.guard.flag_ptr() if arith == "h2" else None

    def pushed_kernel(self, mlp):
        """(K' = [W Kx ; Kh] as fp32 [dx+d, 4d], b Kx as [1, 4d], pack(K'^T) for the data gradient) of the message MLP's
        last (linear) layer W, b pushed through a row-sum aggregation and through Kx:
            (sum_e (a_e W + b)) Kx = (sum_e a_e) (W Kx) + degree (b Kx)."""
        d, dx = self.d, self.dx
        last = mlp.layer_names[-1]

        def build(out):
            W, b = self.store.view(last + "/kernel"), self.store.view(last + "/bias")
            if out is None:
                out = (torch.empty((dx + d, 4 * d), dtype=torch.float32, device=W.device),
                       torch.empty((1, 4 * d), dtype=torch.float32, device=W.device),
                       torch.empty((dx + d, 4 * d), dtype=torch.float32, device=W.device))
            kfull, zb, kt = out
            st = _lib.current_stream()
            kfull[dx:].copy_(self.kernel()[dx:])
            _lib.call("tspgnn_linear_f32", _lib.ptr(W), dx, _lib.ptr(self.packed("Kx", "f32")), None, 0, _lib.ptr(kfull[:dx]),
                      4 * d, 0, W.shape[0], st)
            _lib.call("tspgnn_linear_f32", _lib.ptr(b.view(1, -1)), dx, _lib.ptr(self.packed("Kx", "f32")), None, 0, _lib.ptr(zb),
                      4 * d, 0, 1, st)
            _lib.call("tspgnn_pack_weights_f32", _lib.ptr(kfull), _lib.ptr(kt), 4 * d, dx + d, 1, st)
            return (kfull, zb, kt)
        return self.store.packed(("lstm.pushed.kernel", self.base, last), build)

    def pushed_bias_pack(self, mlp, arith=None, centered=False):
        """For a cell whose input is a row-sum aggregation of ``mlp``'s output: (pack(K'), b Kx) of pushed_kernel in the
        packing of ``arith``.  The cell then takes the row-sum of the LAST HIDDEN activation as its input and starts z
        at degree * (b Kx).  One Dense(d) layer less on every edge row per step."""
        packed = self.packed("K", arith or "f32", centered, pushed=mlp)
        if not centered:
            return packed, self.pushed_kernel(mlp)[1]
        # (K' and b Kx centred per gate: tspgnn_lstm_task.z_centered)
        zb_c = self.store.packed(("lstm.pushed.zb.c", self.base, mlp.layer_names[-1]),
                                 lambda out: _center_gates(self.pushed_kernel(mlp)[1], self.d) if out is None
                                 else out.copy_(_center_gates(self.pushed_kernel(mlp)[1], self.d)))
        return packed, zb_c

    def _backward_task(self, h, c, K, dh_out, dc_out, dz, dc_in, ws, **fields):
        """A tspgnn_lstm_bwd_task over the rows of h: the fields every form shares; the others by field name (tensors as
        their device pointers), zero where not named."""
        return _lib.LstmBwdTask(h=_lib.ptr(h), c=_lib.ptr(c), K=_lib.ptr(K), ln=_lib.ptr(self.ln()), dh_out=_lib.ptr(dh_out),
                                dc_out=_lib.ptr(dc_out), dz=_lib.ptr(dz), dc_in=_lib.ptr(dc_in),
                                ln_grad=_lib.ptr(self.ln_grad()), workspace=_lib.ptr(ws), rows=h.shape[0], **_lib.ptrs(fields))

    def pushed_backward_task(self, x, h, c, dh_out, dc_out, dz, dc_in, ws, kp, zb, deg, defer=False, data=None):
        """Backward task (tspgnn_lnlstm_bwd_multi_h2) of pushed_task: K = pushed_bias_pack's f16x2 K', z restarts at
        deg * zb.  ``data`` = (f16x2 packing of K'^T, dx_out, dh_in): the data gradient [dx_out | dh_in] = dz K'^T formed in
        the same launch (tspgnn_lstm_bwd_task.KTg) instead of by pushed_backward_data."""
        ktg, dx_out, dh_in = data if data is not None else (None, None, None)
        return self._backward_task(h, c, kp, dh_out, dc_out, dz, dc_in, ws, x=x, dx=self.dx, dxh=dh_in,
                                   defer_reduce=int(defer), zbias=zb, zscale=deg, KTg=ktg, dxg=dx_out)

    def fuses_pushed_data_gradient(self):
        """The pushed cell's data gradient can ride in its backward launch (f16x2, d == dx == 64)."""
        return self.d == 64 and self.dx == 64

    def pushed_backward_data(self, mlp, dz, dx_out, dh_in):
        """[d(aggregate) | dh] = dz K'^T."""
        _lib.call("tspgnn_linear_f32", _lib.ptr(dz), 4 * self.d, _lib.ptr(self.pushed_kernel(mlp)[2]), _lib.ptr(dx_out),
                  self.dx, _lib.ptr(dh_in), self.d, 0, dz.shape[0], _lib.current_stream())

    def pushed_backward_weights(self, agg_all, h_all, dz_all, rows, deg_all, g_wkx, g_zb):
        """Over rows = steps * rows_per_step: g_wkx[dx,4d] += agg^T dz (gradient w.r.t. the product W Kx), dKh += h^T dz,
        g_zb[4d] += sum_r deg[r] dz[r] (gradient w.r.t. b Kx); pushed_backward_finish turns the first and the last
        into the gradients of W, b and Kx."""
        gK = self.store.grad_view(self.base + "/kernel")
        st = _lib.current_stream()
        ws = _lib.workspace("tspgnn_wgrad_workspace_floats", rows, max(self.dx, self.d), 4 * self.d, device=dz_all.device)
        _lib.call("tspgnn_wgrad_f32", _lib.ptr(agg_all), _lib.ptr(dz_all), rows, self.dx, 4 * self.d, _lib.ptr(g_wkx), None,
                  _lib.ptr(ws), st)
        _lib.call("tspgnn_wgrad_f32", _lib.ptr(h_all), _lib.ptr(dz_all), rows, self.d, 4 * self.d, _lib.ptr(gK[self.dx:]), None,
                  _lib.ptr(ws), st)
        ws = _lib.workspace("tspgnn_wcolsum_workspace_floats", rows, 4 * self.d, device=dz_all.device)
        _lib.call("tspgnn_wcolsum_f32", _lib.ptr(dz_all), _lib.ptr(deg_all), rows, 4 * self.d, 1.0, _lib.ptr(g_zb), None,
                  _lib.ptr(ws), st)

    def pushed_backward_finish(self, mlp, g_wkx, g_zb):
        """With P = W Kx and q = b Kx:  dW += dP Kx^T,  db += dq Kx^T,  dKx += W^T dP + b^T dq  (once per training step,
        on [dx, 4d]-sized operands)."""
        d, dx, st = self.d, self.dx, _lib.current_stream()
        last = mlp.layer_names[-1]
        W, b = self.store.view(last + "/kernel"), self.store.view(last + "/bias")
        f32 = dict(dtype=torch.float32, device=W.device)
        dW, db = torch.empty((W.shape[0], dx), **f32), torch.empty((1, dx), **f32)
        _lib.call("tspgnn_linear_f32", _lib.ptr(g_wkx), 4 * d, _lib.ptr(self.packed("Kx", "f32T")), _lib.ptr(dW), dx, None, 0, 0,
                  g_wkx.shape[0], st)
        _lib.call("tspgnn_linear_f32", _lib.ptr(g_zb), 4 * d, _lib.ptr(self.packed("Kx", "f32T")), _lib.ptr(db), dx, None, 0, 0, 1, st)
        self.store.grad_view(last + "/kernel").add_(dW)
        self.store.grad_view(last + "/bias").add_(db.view(-1))
        packed = torch.empty_like(g_wkx)
        _lib.call("tspgnn_pack_weights_f32", _lib.ptr(g_wkx), _lib.ptr(packed), g_wkx.shape[0], 4 * d, 0, st)
        wt = W.t().contiguous()
        dkx = torch.empty((dx, 4 * d), **f32)
        _lib.call("tspgnn_linear_f32", _lib.ptr(wt), wt.shape[1], _lib.ptr(packed), None, 0, _lib.ptr(dkx), 4 * d, 0, dx, st)
        dkx.addcmul_(b.view(-1, 1), g_zb.view(1, -1))
        self.store.grad_view(self.base + "/kernel")[:dx].add_(dkx)

    def pushed_task(self, x, state, out, kp, zb, deg, arith=None, centered=False):
        """Cell task whose kernel operand is pushed_bias_pack's K' (either packing) and z starts at deg * zb."""
        return self._forward_task(state, out, kp, x=x, dx=self.dx, zbias=zb, zscale=deg, range_flag=self._flag(arith),
                                  z_centered=int(centered))

    def premultiply(self, y, out=None, scale=None):
        """Zx = y Kx  ([n_src, 4d]); ``scale``: times 2^s for an f16x2 cell, whose z carries that factor."""
        if out is None:
            out = torch.empty((y.shape[0], 4 * self.d), dtype=torch.float32, device=y.device)
        if scale is None:
            _lib.call("tspgnn_linear_f32", _lib.ptr(y), self.dx, _lib.ptr(self.packed("Kx", "f32")), None, 0, _lib.ptr(out),
                      4 * self.d, 0, y.shape[0], _lib.current_stream())
            return out
        # the f16x2 cells' projected-message format: times 2^s, blocked by 16 source rows (include/tspgnn.h)
        n, d4 = y.shape[0], 4 * self.d
        flat = torch.zeros((_pad16(n), d4), dtype=torch.float32, device=y.device)
        _lib.call("tspgnn_linear_f32", _lib.ptr(y), self.dx, _lib.ptr(self.packed("Kx", "f32")), None, 0, _lib.ptr(flat), d4, 0, n,
                  _lib.current_stream())
        out.view(-1, d4 // 16, 4, 16, 4).copy_(flat.mul_(scale).view(-1, 16, d4 // 16, 4, 4).permute(0, 2, 3, 1, 4))
        return out

    def backward_task(self, x, h, c, dh_out, dc_out, dz, dc_in, ws, defer=False, arith=None):
        return self._backward_task(h, c, self.packed("K", "h2" if arith == "h2" else "f32"), dh_out, dc_out, dz, dc_in, ws,
                                   x=x, dx=self.dx, defer_reduce=int(defer))

    def gather_backward_task(self, adj, zx, h, c, dh_out, dc_out, dz, dc_in, ws, dh_in=None, defer=False, arith=None):
        """``dh_in`` given (d == 64): dh_in = dz Kh^T is formed in the same launch, from dz in registers.
        ``defer``: LayerNorm-gradient partials accumulate in ``ws`` (see backward_finish).
        ``arith`` = "h2": operands for tspgnn_lnlstm_bwd_multi_h2 (``zx`` as the f16x2 forward wrote it)."""
        fuse = dh_in is not None and self.d == 64
        form = "h2" if arith == "h2" else "f32"
        return self._backward_task(h, c, self.packed("Kh", form), dh_out, dc_out, dz, dc_in, ws, uv=adj.uv, Zx=zx,
                                   KT=self.packed("Kh", form + "T") if fuse else None, dxh=dh_in if fuse else None,
                                   defer_reduce=int(defer))

    # ---- bf16-storage tape (tspgnn_lnlstm_bwd_multi_bf16 and friends, include/tspgnn.h)

    def backward_task_bf16(self, x, h, c, dh_out, dc_out, dz, dc_in, ws, adj=None, zx=None):
        """tspgnn_lnlstm_bwd_multi_bf16 task: x / h (and zx: the blocked projected messages, gather-init mode with adj)
        are the tape's bf16 arrays."""
        form = dict(x=x, dx=self.dx) if adj is None else dict(uv=adj.uv, Zx=zx)
        return self._backward_task(h, c, self.packed("K" if adj is None else "Kh", "bf16"), dh_out, dc_out, dz, dc_in, ws,
                                   defer_reduce=1, **form)

    def backward_finish(self, ws):
        """Fold the LayerNorm-gradient partials that the deferred backward launches of all time steps left in ws."""
        _lib.call("tspgnn_lnlstm_bwd_finish_f32", _lib.ptr(ws), _lib.ptr(self.ln_grad()), self.d, _lib.current_stream())

    # data-gradient GEMMs by ``form``: the fp32 kernel, or on a bf16 tape read as it is the bf16-exact weights of that mode
    DATA_GEMM = {"f32": "tspgnn_linear_f32", "bf16": "tspgnn_linear_bf16w_f32"}

    def check_backward_data(self, form):
        if form == "f32" and (self.dx + self.d) not in (64, 128, 256):
            raise NotImplementedError("LSTM backward needs dx+d in {64,128,256} (got %d)" % (self.dx + self.d))

    def backward_data(self, dz, dx_out, dh_in, form="f32"):
        """[dx | dh] = dz K^T."""
        self.check_backward_data(form)
        _lib.call(self.DATA_GEMM[form], _lib.ptr(dz), 4 * self.d, _lib.ptr(self.packed("K", form + "T")), _lib.ptr(dx_out),
                  self.dx, _lib.ptr(dh_in), self.d, 0, dz.shape[0], _lib.current_stream())

    def gather_backward_data(self, adj, dz, dh_in, dzx, dy, form="f32"):
        """dh = dz Kh^T (unless the cell launch already formed it: dh_in None), dZx = EV^T dz, dy = dZx Kx^T (``dy`` None:
        left to the source MLP's backward launch)."""
        st = _lib.current_stream()
        if dh_in is not None:
            _lib.call(self.DATA_GEMM[form], _lib.ptr(dz), 4 * self.d, _lib.ptr(self.packed("Kh", form + "T")), None, 0,
                      _lib.ptr(dh_in), self.d, 0, dz.shape[0], st)
        adj.matmul(dz, transpose=True, out=dzx)
        if dy is not None:
            _lib.call(self.DATA_GEMM[form], _lib.ptr(dzx), 4 * self.d, _lib.ptr(self.packed("Kx", form + "T")), None, 0,
                      _lib.ptr(dy), self.dx, 0, dzx.shape[0], st)

    def backward_weights_folded(self, y_all, dzx_all, rows_src, h_all, dz_all, rows):
        """dKx += y^T dZx over T*n_src rows (instead of T*M), dKh += h^T dz over T*M rows."""
        gK = self.store.grad_view(self.base + "/kernel")
        ws = _lib.workspace("tspgnn_wgrad_workspace_floats", rows_src, self.dx, 4 * self.d, device=dz_all.device)
        wgrad(y_all, dzx_all, rows_src, self.dx, 4 * self.d, gK[:self.dx], None, ws)
        ws = _lib.workspace("tspgnn_wgrad_workspace_floats", rows, self.d, 4 * self.d, device=dz_all.device)
        wgrad(h_all, dz_all, rows, self.d, 4 * self.d, gK[self.dx:], None, ws)

    def backward_weights(self, x_all, h_all, dz_all, rows):
        """dK += [x|h]^T dz over all time steps at once (rows = T * rows_per_step)."""
        gK = self.store.grad_view(self.base + "/kernel")
        if self.dx:
            ws = _lib.workspace("tspgnn_wgrad_workspace_floats", rows, self.dx, 4 * self.d, device=dz_all.device)
            wgrad(x_all, dz_all, rows, self.dx, 4 * self.d, gK[:self.dx], None, ws)
        ws = _lib.workspace("tspgnn_wgrad_workspace_floats", rows, self.d, 4 * self.d, device=dz_all.device)
        wgrad(h_all, dz_all, rows, self.d, 4 * self.d, gK[self.dx:], None, ws)


class GraphNN(object):
    def __init__(self, var, mat, msg, loop, MLP_depth=3, MLP_weight_initializer=None, MLP_bias_initializer=None,
                 RNN_cell=LayerNormBasicLSTMCell, Cell_activation="relu", Msg_activation="relu",
                 Msg_last_activation=None, float_dtype=torch.float32, name="GraphNN", store=None):
        """Same four dictionaries as the reference (graphnn.py:21-48):
        var: name -> embedding size;  mat: name -> (row var, column var or int);
        msg: name -> (source var, target var);  loop: var -> list of update dicts with the
        optional keys 'mat', 'transpose?', 'fun', 'msg', 'var'."""
        self.var, self.mat, self.msg, self.loop, self.name = var, mat, msg, loop, name
        self.MLP_depth = MLP_depth
        # The reference initialises the message-MLP *biases* with the weight initialiser
        # (graphnn.py:121 passes MLP_weight_initializer() as bias_initializer).
        self.MLP_weight_initializer = MLP_weight_initializer or V.xavier_uniform
        self.MLP_bias_initializer = MLP_bias_initializer
        self.RNN_cell = RNN_cell
        self.Cell_activation = Cell_activation
        self.Msg_activation = Msg_activation
        self.Msg_last_activation = Msg_last_activation
        if float_dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError("GraphNN: float_dtype must be torch.float32 or torch.bfloat16 (bf16 storage of the "
                                      "embeddings with fp32 accumulation)")
        self.float_dtype = float_dtype
        self.store = store if store is not None else V.get_default_store()
        self.fold_adjacency = True   # (EV y) Kx = EV (y Kx) fast path; False = op-for-op reference order
        # f16x2 fused forward: LayerNorm's mean subtraction folded into the cell kernels (TSPGNN_CENTER_GATES=0: A/B)
        self.center_gates = os.environ.get("TSPGNN_CENTER_GATES", "1") != "0"
        # f16x2 inference forward: the whole T-step loop as ONE launch of resident workgroups (tspgnn_mp_loop_h2) where the
        # wiring and the batch allow it (_loop_launch); False / TSPGNN_LOOP=0 = one row-sum + one cell launch per step
        self.persistent_loop = True
        self._launched_loop = None   # launched_loop
        self._last_backward = None   # last_backward
        # training (f16x2): a message MLP's last linear layer pushed through the row-sum into the receiving cell, as in the
        # inference plan (one Dense layer less per edge row in the forward, the backward and the weight gradients)
        self.push_training = os.environ.get("TSPGNN_PUSH_TRAINING", "1") != "0"
        self.wgrad_chunk_bytes = 24 * 2 ** 30   # backward: budget for the pre-activation gradients kept per weight-gradient chunk
        # training forward: message MLPs of step t+1 inside the cell launch of step t (TSPGNN_FUSE_TRAINING=1).  Off by
        # default: the tape makes the training forward HBM-write-bound, and there the two plain launches at full occupancy
        # measured 0.2 ms per step FASTER than the fused one (C2: 11.75 vs 11.95 ms)
        self.fuse_training_messages = os.environ.get("TSPGNN_FUSE_TRAINING", "0") == "1"
        # training (f16x2 and bf16 storage, widths 64 / 128): the message MLPs' data gradient on the fp16 matrix cores
        # (tspgnn_mlp_bwd_multi_h2) instead of the fp32 matrix instruction (TSPGNN_MLP_BWD_H2=0: A/B)
        self.mlp_backward_h2 = os.environ.get("TSPGNN_MLP_BWD_H2", "1") != "0"
        # training (f16x2, pushed message MLPs of width 64), OPT-IN (TSPGNN_RECOMPUTE=1): the backward recomputes the MLP's
        # hidden activations and forms the MLP's weight gradients in the same launch (tspgnn_mlp_bwd_rc_h2), so that the
        # forward tapes only the messages and runs the message MLP inside the cell launch as the inference plan does.
        # Parity-green and deterministic; off by default because it does not pay at C2 (round 5, one box: taped 10.98-11.19 ms
        # per training step, this form 11.6-11.7 ms).  The variant that handed the recomputed activations to tspgnn_wgrad
        # instead (11.23-11.33 ms) was removed in round 6 -- DESIGN_HISTORY
        self.recompute_messages = os.environ.get("TSPGNN_RECOMPUTE", "0") == "1"
        # GEMM arithmetic of the inference forward, all fp32-class in accuracy: "f16x2" = fp16 matrix cores on
        # two-piece splits of the fp32 operands (csrc/dense_h2.hip, the default); "bf16x3" = bf16 matrix cores on
        # exact three-piece splits (csrc/dense_x3.hip); "f32" = fp32 MFMA.  TSPGNN_GEMM in the environment selects
        # one; shapes the split kernels do not cover fall back to "f32".
        self.gemm = os.environ.get("TSPGNN_GEMM", "f16x2")
        if self.gemm not in GEMM_ARITH:
            raise ValueError("TSPGNN_GEMM must be one of %s, got %r" % (sorted(GEMM_ARITH), self.gemm))
        self._mlp_h2_native_ok = False   # bf16-storage backward: the last eager pass found the MLP weights inside the f16x2 range
        self.check_model()
        self._init_parameters()

    # ---------------------------------------------------------------- static checks
    def check_model(self):
        """graphnn.py:72-103, same exception types and messages."""
        for v in self.var:
            if v not in self.loop:
                raise Warning("Variable {v} is not updated anywhere! Consider removing it from the model".format(v=v))
        for v in self.loop:
            if v not in self.var:
                raise Exception("Updating variable {v}, which has not been declared!".format(v=v))
        for mat, (v1, v2) in self.mat.items():
            if v1 not in self.var:
                raise Exception("Matrix {mat} definition depends on undeclared variable {v}".format(mat=mat, v=v1))
            if v2 not in self.var and type(v2) is not int:
                raise Exception("Matrix {mat} definition depends on undeclared variable {v}".format(mat=mat, v=v2))
        for msg, (v1, v2) in self.msg.items():
            if v1 not in self.var:
                raise Exception("Message {msg} maps from undeclared variable {v}".format(msg=msg, v=v1))
            if v2 not in self.var:
                raise Exception("Message {msg} maps to undeclared variable {v}".format(msg=msg, v=v2))

    def _update_width(self, update):
        """Number of columns one loop entry contributes to the cell input."""
        if "var" in update:
            width = self.var[update["var"]]
            if "msg" in update:
                width = self.var[self.msg[update["msg"]][1]]
            return width
        v2 = self.mat[update["mat"]][1]
        if type(v2) is not int:
            raise NotImplementedError("a loop entry without 'var' needs a matrix with an integer second "
                                      "dimension (graphnn.py:163-165)")
        return v2

    def _init_parameters(self):
        """graphnn.py:105-126: message MLPs ([d_in]*depth + [d_out], relu, xavier weights AND
        biases) and one LayerNorm-LSTM cell per variable."""
        self._msg_MLPs = {}
        for msg, (vin, vout) in self.msg.items():
            self._msg_MLPs[msg] = Mlp(
                layer_sizes=[self.var[vin] for _ in range(self.MLP_depth)],
                output_size=self.var[vout],
                activations=[self.Msg_activation for _ in range(self.MLP_depth)],
                output_activation=self.Msg_last_activation,
                kernel_initializer=self.MLP_weight_initializer,
                bias_initializer=self.MLP_weight_initializer,
                name="%s/%s" % (self.name, msg),
                name_internal_layers=True,
                input_size=self.var[vin],
                store=self.store,
            )
        self._RNN_cells = {}
        for v, d in self.var.items():
            dx = sum(self._update_width(u) for u in self.loop[v])
            self._RNN_cells[v] = self.RNN_cell(d, dx, "%s/%s_cell" % (self.name, v),
                                               activation=self.Cell_activation, store=self.store)

    # ---------------------------------------------------------------- run-time checks
    def check_run(self, adjacency_matrices, initial_embeddings, time_steps, LSTM_initial_states):
        """graphnn.py:185-271 (tf.assert_equal -> ValueError with the reference's messages)."""
        num_vars = {}
        for v, d in self.var.items():
            shape = tuple(initial_embeddings[v].shape)
            num_vars[v] = shape[0]
            if shape[1] != d:
                raise ValueError("Initial embedding of variable {v} doesn't have the same dimensionality {d} as "
                                 "declared".format(v=v, d=d))
            if v in LSTM_initial_states:
                ls = tuple(LSTM_initial_states[v].shape)
                if ls[1] != d:
                    raise ValueError("Initial hidden state of variable {v}'s LSTM doesn't have the same "
                                     "dimensionality {d} as declared".format(v=v, d=d))
                if ls != shape:
                    raise ValueError("Initial embeddings of variable {v} don't have the same shape as the its "
                                     "LSTM's initial hidden state".format(v=v))
        for mat, (v1, v2) in self.mat.items():
            ms = tuple(adjacency_matrices[mat].shape)
            if ms[0] != num_vars[v1]:
                raise ValueError("Matrix {m} doesn't have the same number of nodes as the initial embeddings of "
                                 "its variable {v}".format(v=v1, m=mat))
            if type(v2) is int:
                if ms[1] != v2:
                    raise ValueError("Matrix {m} doesn't have the same dimensionality {d} on the second variable "
                                     "as declared".format(m=mat, d=v2))
            elif ms[1] != num_vars[v2]:
                raise ValueError("Matrix {m} doesn't have the same number of nodes as the initial embeddings of "
                                 "its variable {v}".format(v=v2, m=mat))

    def _pushable(self, v, mats, folded):
        """True if v's cell input is a pattern (all-ones) adjacency product of a message MLP whose last
        layer is linear: that layer can be pushed through the row-sum into the cell (pushed_bias_pack)."""
        if not self.fold_adjacency or folded[v] is not None or len(self.loop[v]) != 1:
            return False
        u = self.loop[v][0]
        if "var" not in u or "fun" in u or "mat" not in u or "msg" not in u:
            return False
        mlp, cell = self._msg_MLPs[u["msg"]], self._RNN_cells[v]
        adj = mats[u["mat"]]
        csr = adj.csr_t if u.get("transpose?", False) else adj.csr
        if csr[2] is not None or mlp.relu[-1] or mlp.n_square < 2 or len(mlp._chunks()) != 1:
            return False
        return cell.d == 64 and cell.dx == 64 and mlp.sizes[-1] == cell.dx

    def _folded(self, v, mats, bf16_inference=False):
        """The loop entry of v if its cell input is a single gather over a two-ones-per-row matrix
        (then the adjacency product is folded through the cell's GEMM), else None.  The fp32-storage forward and every
        training forward fold at d == dx == 64 (can_fold), with or without a message MLP; ``bf16_inference``: the
        bf16-storage inference forward folds at every width, but only behind a message MLP of the cell's own width, whose
        launch then projects Zx = msg(y) Kx on the source rows."""
        if not self.fold_adjacency or len(self.loop[v]) != 1:
            return None
        u = self.loop[v][0]
        if "var" not in u or "fun" in u or "mat" not in u or u.get("transpose?", False) or mats[u["mat"]].uv is None:
            return None
        cell = self._RNN_cells[v]
        if bf16_inference:
            return u if "msg" in u and cell.dx == self._msg_MLPs[u["msg"]].sizes[-1] == self.var[v] else None
        return u if cell.can_fold() else None

    def _pushed_degrees(self, v, mats):
        """Stored entries per row of the adjacency product behind a pushed cell (the factor of its bias b Kx)."""
        u0 = self.loop[v][0]
        return mats[u0["mat"]].row_degrees(bool(u0.get("transpose?", False)))

    def _message_to_tape(self, v, i, folded):
        """The training forward writes loop entry (v, i)'s message straight into the tape's cell input X[v]: a folded
        cell keeps the message per source row, a cell whose only entry has no matrix takes it as it is."""
        return folded[v] is not None or (len(self.loop[v]) == 1 and "mat" not in self.loop[v][i])

    def _message_output_slot(self, v, i, folded):
        """Layer slot of the tape's acts[(v, i)] that keeps loop entry (v, i)'s message, or None.  The backward of a chain
        that ends in a relu masks by the chain's output (tspgnn_mlp_bwd_task.Yout); where that output is only a
        temporary of the forward -- it goes into an adjacency product or a concatenation -- the tape gets one more slot
        behind the hidden activations for it.  A linear last layer (the default) needs none."""
        mlp = self._msg_MLPs[self.loop[v][i]["msg"]]
        if not mlp.relu[-1] or self._message_to_tape(v, i, folded):
            return None
        return mlp.n_square - 1

    def _matrices(self, adjacency_matrices, device):
        """-> ({name: DeviceAdjacency} of the matrices that multiply an embedding, {name: dense fp32 tensor} of those a
        loop entry without 'var' appends to the cell input as they are), each converted once per call."""
        mats, dense = {}, {}
        for v in self.var:
            for update in self.loop[v]:
                m = update.get("mat")
                if m is None:
                    continue
                if "var" in update and m not in mats:
                    mats[m] = DeviceAdjacency.wrap(adjacency_matrices[m], device)
                elif "var" not in update and m not in dense:
                    # graphnn.py:163-165: the matrix itself joins the cell input -- a constant of the step (a placeholder:
                    # tf.gradients stops there); its columns only meet the cell kernel's rows
                    a = adjacency_matrices[m]
                    if isinstance(a, (SparseEV, DeviceAdjacency)):
                        raise NotImplementedError("a matrix appended as a cell input must be dense")
                    dense[m] = torch.as_tensor(a, dtype=torch.float32).to(device).contiguous()
        return mats, dense

    def _cell_input(self, v, msg_out, mats, rows, dtype, out=None):
        """The input of v's unfolded cell from msg_out = {(v, i): rows of loop entry i after 'fun' / the message MLP, or the
        appended matrix}: per entry with a matrix the adjacency product, several entries concatenated on axis 1.
        -> (x [rows, dx], ops): ``ops`` is the list of (fn, args) that fills x -- a plan replays it every step, an eager
        driver runs it on the spot.  ``out`` (training: the tape's slot of the step) becomes x: a single product writes
        straight into it, the concatenation writes into it, a single entry that lives elsewhere is copied."""
        single = len(self.loop[v]) == 1
        new = dict(dtype=dtype, device=self.store.theta.device)
        inputs, ops = [], []
        for i, u in enumerate(self.loop[v]):
            y = msg_out[(v, i)]
            if "var" in u and "mat" in u:
                adj, tr = mats[u["mat"]], u.get("transpose?", False)
                o = out if single and out is not None else torch.empty((adj.shape[1] if tr else adj.shape[0], y.shape[1]), **new)
                ops.append((adj.matmul, (y, tr, o)))
                y = o
            inputs.append(y)
        dx = self._RNN_cells[v].dx
        for y in inputs:    # every entry on the cell's rows, the widths adding up to the cell's input width
            _check_cell_input((y.shape[0], sum(z.shape[1] for z in inputs)), rows, dx)
        if not single:
            x = out if out is not None else torch.empty((rows, dx), **new)
            ops.append((lambda ins, o: torch.cat(ins, dim=1, out=o), (inputs, x)))
        elif out is not None and inputs[0].data_ptr() != out.data_ptr():
            x = out
            ops.append((out.copy_, (inputs[0],)))
        else:
            x = inputs[0]
        return x, ops

    def _cell_forward_task(self, v, x, st, out, folded, pushed, mats, arith=None, centered=False):
        """v's cell task in the form its selectors name: folded (x = the projected messages Zx of the source rows, gathered
        by the cell kernel), pushed (x = the row-sum of the message MLP's last hidden activation, K' = [W Kx ; Kh]) or plain."""
        cell = self._RNN_cells[v]
        if folded[v] is not None:
            return cell.gather_task(mats[folded[v]["mat"]], x, st, out, arith=arith, centered=centered)
        if pushed[v]:
            kp, zb = cell.pushed_bias_pack(self._msg_MLPs[self.loop[v][0]["msg"]], arith=arith, centered=centered)
            return cell.pushed_task(x, st, out, kp, zb, self._pushed_degrees(v, mats), arith=arith, centered=centered)
        return cell.task(x, st, out, arith=arith, centered=centered)

    def _prepack_cells(self, folded, pushed, arith, centered, with_kx_and_mlps=False):
        """The packings _cell_forward_task will take, made up front: the caller vets their range (check_h2_weights) before
        any kernel multiplies with them.  A folded cell multiplies with Kh, a pushed one with the PRODUCT [W Kx ; Kh] --
        which can leave the range on its own --, the others with the whole kernel.  ``with_kx_and_mlps`` (the training
        forward, whose message launches are not built yet): also the Kx a folded cell's message MLP projects with and the
        single-kernel message MLPs."""
        for v, cell in self._RNN_cells.items():
            if folded[v] is not None:
                cell.packed("Kh", arith, centered)
                if with_kx_and_mlps and "msg" in folded[v]:
                    cell.packed("Kx", arith, centered)
            elif pushed[v]:
                cell.pushed_bias_pack(self._msg_MLPs[self.loop[v][0]["msg"]], arith=arith, centered=centered)
            else:
                cell.packed("K", arith, centered)
        if with_kx_and_mlps:
            for mlp in self._msg_MLPs.values():
                if len(mlp._chunks()) == 1:
                    mlp.wb_packed(0, mlp.n_square - 1, mlp.sizes[-1], arith)

    def _check_bf16_wiring(self, folded=None):
        """What the bf16-storage kernels cover; ``folded`` (training, which folds by the fp32 rule): its folded cells must
        also be the ones the bf16 gather cell takes."""
        for v in self.var:
            cell = self._RNN_cells[v]
            if self.var[v] not in (32, 64, 128) or cell.dx % 32 != 0:
                raise NotImplementedError("bf16 storage needs widths 32/64/128 and cell inputs in multiples of 32")
            if folded is not None and folded[v] is not None and (
                    "msg" not in folded[v] or cell.dx != self._msg_MLPs[folded[v]["msg"]].sizes[-1] or cell.dx != self.var[v]):
                raise NotImplementedError("bf16 storage: a folded cell input needs a message MLP of the cell's width")
            for u in self.loop[v]:
                if "var" not in u or "fun" in u:
                    raise NotImplementedError("bf16 storage supports loop entries made of var / msg / mat only")
                if "msg" in u:
                    m = self._msg_MLPs[u["msg"]]
                    if m._plan[0] != "square" or m._plan[3] or not (1 <= m.n_square <= 4) or m.input_size != m.sizes[-1]:
                        raise NotImplementedError("bf16 storage needs square message MLPs of at most 4 layers")

    def _bf16_message_task(self, mlp, y, rows, out, proj, interleave=False, blocked=False, acts=None):
        """tspgnn_mlp_task_bf16 of ``mlp`` over ``rows`` rows of y (``blocked``: a state buffer blocked by 16 rows);
        proj = (bf16 Kx, Zx) of a folded receiver or (None, None); ``interleave``: the last layer's columns interleaved
        (y_interleaved); ``acts``: the tape's [layers-1, rows, d] slice for the hidden activations."""
        n, d = mlp.n_square, mlp.sizes[-1]
        return _lib.MlpTaskB(X=_lib.ptr(y), wb=_lib.ptr(mlp.wb_packed_bf16(0, n - 1, d, interleave_last=interleave)),
                             Y=_lib.ptr(out), rows=rows, n_layers=n, relu_mask=mlp.relu_mask(0, n), proj_w=_lib.ptr(proj[0]),
                             proj_out=_lib.ptr(proj[1]), acts=_lib.ptr(acts) if n > 1 else None,
                             acts_stride=0 if acts is None else acts.stride(0), x_blocked=int(blocked),
                             y_interleaved=int(interleave))

    # ---------------------------------------------------------------- step builders
    # One synchronous step (graphnn.py:142-173) in each of its three launch shapes, as a function of where it reads and
    # writes (_Ends).  The drivers decide the selectors (folded, pushed, arith, centered, rc, consumers, interleave) and
    # hand them in; the builders read no switch of their own.  Each is a generator of the step's parts in running order
    # -- message launches, adjacency products, cell launches --, see _run.  An eager driver must hand _run the generator
    # itself, not a list of it: a cell task's first use packs its weights, and tests/test_launch_trace.py pins those
    # packings BEHIND the adjacency products the driver has already run (the bf16 training forward: variable by variable,
    # which is why _bf16_step yields one part of products per variable).
    def _split_messages(self, ep, dense, folded, pushed, arith=None, centered=False, rc={}, project=True):
        """-> the message-MLP launches of a step (per width): every loop entry's MLP -- the whole chain, with Zx = msg(y) Kx
        riding behind it for a folded receiver (``project``), or for a pushed receiver all but the last layer, whose output
        is the last saved activation (``rc``: the backward recomputes them, none is saved).  Fills ep.msg (and ep.zx).
        What has no task runs while the step is built, which only an eager driver's wiring asks for: a Python 'fun'
        (graphnn.py:149-151; the backward differentiates it again: _fun_vjp) and a chain of several fp32 kernels."""
        f32 = dict(dtype=torch.float32, device=self.store.theta.device)
        tasks = {}
        for v in self.var:
            for i, u in enumerate(self.loop[v]):
                if "var" not in u:          # an appended matrix: joins the cell input as it is
                    ep.msg[(v, i)] = dense[u["mat"]]
                    continue
                y = h = ep.src[u["var"]].h
                if "fun" in u:
                    y = u["fun"](h)
                    if not torch.is_tensor(y) or y.shape != h.shape:
                        raise ValueError("loop entry 'fun' must map [rows, d] to a tensor of the same shape")
                    y = y.to(torch.float32).contiguous()
                    ep.keep.append(y)
                if "msg" in u:
                    mlp = self._msg_MLPs[u["msg"]]
                    out = ep.msg.get((v, i))
                    if out is None:
                        out = torch.empty((y.shape[0], mlp.sizes[-1]), **f32)
                    acts, stride = ep.acts.get((v, i), (None, 0))
                    proj = None
                    if pushed[v]:   # last hidden activation only; the last layer is folded into the cell
                        if rc.get((v, i)):
                            acts, stride = None, 0
                        task = mlp.prefix_task(y, out, mlp.n_square - 1, arith=arith, acts=acts, acts_stride=stride)
                    else:
                        if project and folded[v] is not None:   # Zx = msg(y) Kx rides in the MLP launch
                            if v not in ep.zx:
                                ep.zx[v] = torch.empty((_pad16(y.shape[0]), 4 * self.var[v]), **f32)
                            proj = (self._RNN_cells[v].packed("Kx", arith or "f32", centered), ep.zx[v])
                        task = mlp.task(y, out, acts, stride, proj=proj, arith=arith)
                    if task is not None:
                        tasks.setdefault(mlp.sizes[-1], []).append(task)
                    else:   # run here, once: never inside a plan, which declines such a wiring before it builds anything
                        assert not pushed[v] and (acts is not None or not project), "a replayed step needs single-kernel MLPs"
                        if acts is None:
                            out = mlp(y)
                        elif arith:
                            raise NotImplementedError("bf16x3 training forward needs single-kernel message MLPs")
                        else:
                            mlp.forward_saving(y, out, acts, stride)
                        if proj is not None:
                            self._RNN_cells[v].premultiply(out, out=proj[1])
                    y = out
                ep.msg[(v, i)] = y
        return _launch_ops("tspgnn_mlp_fwd_multi_" + (arith or "f32"), tasks)

    def _split_step(self, ep, mats, dense, folded, pushed, arith=None, centered=False, rc={}, project=True):
        """The split shape: (A) every message MLP, (B) the adjacency products / the projection Zx = y Kx of a folded
        cell that no MLP launch made, (C) every cell -- independent work of the same kind shares a launch per width."""
        yield self._split_messages(ep, dense, folded, pushed, arith, centered, rc, project)
        xs, mid = {}, []
        for v in self.var:
            u = folded[v]
            if u is None:
                xs[v], ops = self._cell_input(v, ep.msg, mats, ep.rows[v], torch.float32, out=ep.x.get(v))
                mid += ops
            elif project and "msg" in u:
                xs[v] = ep.zx[v]
            else:   # no message launch to project behind: Zx = y Kx by a launch of its own (f16x2: times 2^s, blocked)
                y, x = ep.msg[(v, 0)], ep.x.get(v)
                if x is not None and x.data_ptr() != y.data_ptr():   # (training: the tape keeps y per source row)
                    mid.append((x.copy_, (y,)))
                    y = x
                xs[v] = ep.zx[v] if v in ep.zx else torch.empty((_pad16(y.shape[0]), 4 * self.var[v]), dtype=torch.float32,
                                                                device=y.device)
                mid.append((self._RNN_cells[v].premultiply,
                            (y, xs[v], _lib.lib.tspgnn_h2_weight_scale() if arith == "h2" else None)))
        ep.keep.append(xs)
        yield mid
        tasks = {}
        for v, d in self.var.items():
            tasks.setdefault(d, []).append(self._cell_forward_task(v, xs[v], ep.src[v], (ep.dst[v].h, ep.dst[v].c), folded,
                                                                   pushed, mats, arith, centered))
        yield _launch_ops("tspgnn_lnlstm_fwd_multi_" + (arith or "f32"), tasks)

    def _fused_message(self, v, i, ep, folded, pushed, arith, centered):
        """(wb, n_layers, relu_mask, out, proj_w, proj_out) of loop entry (v, i)'s message MLP writing into ``ep``, as the
        fused cell + message launch and the one-launch loop take it; out None: a folded receiver only takes Zx."""
        mlp = self._msg_MLPs[self.loop[v][i]["msg"]]
        n = mlp.n_square - 1 if pushed[v] else mlp.n_square   # >= 1 (_pushable needs two square layers)
        pw = po = None
        if folded[v] is not None:
            pw, po = self._RNN_cells[v].packed("Kx", arith, centered), ep.zx[v]
        elif (v, i) not in ep.msg:
            ep.msg[(v, i)] = torch.empty((ep.rows[self.loop[v][i]["var"]], mlp.sizes[-1]), dtype=torch.float32,
                                         device=self.store.theta.device)
        return (mlp.wb_packed(0, n - 1, mlp.sizes[-1], arith), n, mlp.relu_mask(0, n), ep.msg.get((v, i)), pw, po)

    def _fused_step(self, ep, nxt, mats, folded, pushed, consumers, arith, centered=False, rc={}):
        """The fused shape (tspgnn_lnlstm_mlp_fwd_multi_x3 / _h2): the adjacency products over the messages in ep.msg, then
        ONE launch per width that updates the states and, on the rows of h' it still holds in registers, evaluates the
        message MLP that reads them in the next step, writing where ``nxt`` (that step's _Ends) says; nxt None: the last
        step, the cells alone.  consumers = _single_consumers()."""
        xs, mid = {}, []
        for v in self.var:
            if folded[v] is not None:
                xs[v] = ep.zx[v]
            else:
                xs[v], ops = self._cell_input(v, ep.msg, mats, ep.rows[v], torch.float32, out=ep.x.get(v))
                mid += ops
        ep.keep.append(xs)
        yield mid
        tasks = {}
        for v, d in self.var.items():
            n_v, c = ep.rows[v], ep.src[v].c
            st = LSTMStateTuple(c=c if c is None else c[:n_v], h=ep.src[v].h[:n_v])
            t = self._cell_forward_task(v, xs[v], st, (ep.dst[v].h, ep.dst[v].c), folded, pushed, mats, arith, centered)
            more = {}
            if nxt is not None:   # the message MLP that reads this variable's new h in the next step
                key = consumers[v]
                wb, n, mask, out, pw, po = self._fused_message(key[0], key[1], nxt, folded, pushed, arith, centered)
                saved, stride = nxt.acts.get(key, (None, 0))
                if rc.get(key) or n == 1:
                    saved = None
                more = dict(mlp_wb=_lib.ptr(wb), mlp_layers=n, relu_mask=mask, mlp_out=_lib.ptr(out), proj_w=_lib.ptr(pw),
                            proj_out=_lib.ptr(po), mlp_acts=_lib.ptr(saved), mlp_acts_stride=stride)
            tasks.setdefault(d, []).append(_lib.CellMlpTask(t, state_in_blocked=int(ep.blk_in.get(v, False)),
                                                            state_out_blocked=int(ep.blk_out.get(v, False)), **more))
        yield _launch_ops("tspgnn_lnlstm_mlp_fwd_multi_" + arith, tasks)

    def _bf16_step(self, ep, mats, folded, interleave=False):
        """The bf16-storage shape, three launches per step: message MLPs (a folded receiver's with its Kx projection),
        adjacency products, cells (a folded cell in gather-init mode).  ``interleave``: a plain message (no projection
        rides behind it) has its last layer's columns interleaved in the packing, 16-byte stores of Y
        (tspgnn_mlp_task_bf16.y_interleaved)."""
        bf = dict(dtype=torch.bfloat16, device=self.store.theta.device)
        mlp_tasks = {}
        for v in self.var:
            for i, u in enumerate(self.loop[v]):
                src = u["var"]
                y = ep.src[src].h
                if "msg" in u:
                    mlp = self._msg_MLPs[u["msg"]]
                    d, rows = mlp.sizes[-1], ep.rows[src]
                    out = ep.msg.get((v, i))
                    if out is None:
                        out = torch.empty((rows, d), **bf)
                    proj = (None, None)
                    if folded[v] is not None:
                        if v not in ep.zx:
                            ep.zx[v] = torch.empty((_pad16(rows), 4 * self.var[v]), **bf)
                        proj = (self._RNN_cells[v].packed("Kx", "bf16"), ep.zx[v])
                    mlp_tasks.setdefault(d, []).append(self._bf16_message_task(
                        mlp, y, rows, out, proj, interleave=interleave and proj[0] is None and d % 32 == 0,
                        blocked=ep.blk_in.get(src, False), acts=ep.acts.get((v, i), (None, 0))[0]))
                    y = out
                ep.msg[(v, i)] = y
        # tasks with a projection go to their own launch: without them the MLP kernel needs a third of the registers (the
        # projection's 4d accumulators) and the big edge task runs at twice the occupancy
        launches = []
        for d, ts in mlp_tasks.items():
            for group in ([t for t in ts if not t.proj_w], [t for t in ts if t.proj_w]):
                launches += _launch_ops("tspgnn_mlp_fwd_multi_bf16", {d: group})
        yield launches
        cell_tasks = {}
        for v, d in self.var.items():
            if folded[v] is not None:
                x, adj = ep.zx[v], mats[folded[v]["mat"]]
            else:
                x, ops = self._cell_input(v, ep.msg, mats, ep.rows[v], torch.bfloat16, out=ep.x.get(v))
                adj = None
                ep.keep.append(x)
                yield ops
            cell_tasks.setdefault(d, []).append(self._RNN_cells[v].task_bf16(
                x, ep.src[v].h, ep.src[v].c, ep.dst[v].h, ep.dst[v].c, ep.rows[v], adj=adj,
                state_in_blocked=ep.blk_in.get(v, False), state_out_blocked=ep.blk_out.get(v, False)))
        yield _launch_ops("tspgnn_lnlstm_fwd_multi_bf16", cell_tasks)

    def _tape_ends(self, tape):
        """-> ends(t), the _Ends of step t of a training forward: it reads slot t of the tape and writes slot t + 1; cell
        inputs, messages, projected messages and hidden activations go straight into the tape.  Which array and layer an
        entry's message goes to does not depend on t and is worked out once: the eager forward pays for every index."""
        H, C, X, ZX = tape.H, tape.C, tape.X, tape.ZX
        rows = {v: h.shape[1] for v, h in H.items()}
        # X[v] as the cell input's place: not for a folded cell behind a message MLP, whose X is that message's place
        own_x = [v for v in self.var if tape.folded[v] is None or "msg" not in tape.folded[v]]
        saved, where = [], []   # (key, acts or None, stride between layers), (key, array, layer or None)
        for (v, i), acts in tape.acts.items():
            rc = tape.rc.get((v, i))
            saved.append(((v, i), None if rc else acts, acts.stride(0)))   # (recomputed by the backward: none is saved)
            slot = self._message_output_slot(v, i, tape.folded)
            if tape.pushed[v]:   # the message is the last hidden activation
                where.append(((v, i), acts, 0 if rc else self._msg_MLPs[self.loop[v][i]["msg"]].n_square - 2))
            elif self._message_to_tape(v, i, tape.folded):
                where.append(((v, i), X[v], None))
            elif slot is not None:
                where.append(((v, i), acts, slot))

        def ends(t):
            return _Ends({v: LSTMStateTuple(C[v][t], H[v][t]) for v in rows}, {v: LSTMStateTuple(C[v][t + 1], H[v][t + 1]) for v in rows},
                         rows=rows, zx={v: zx[t] for v, zx in ZX.items()}, x={v: X[v][t] for v in own_x},
                         msg={key: a[t] if k is None else a[k, t] for key, a, k in where},
                         acts={key: (a if a is None else a[:, t], stride) for key, a, stride in saved})
        return ends

    # ---------------------------------------------------------------- forward
    def __call__(self, adjacency_matrices, initial_embeddings, time_steps, LSTM_initial_states={}):
        """-> {var: LSTMStateTuple(c, h)} after ``time_steps`` synchronous steps
        (graphnn.py:128-183).  Embeddings are fp32 device tensors; matrices may be SparseEV,
        DeviceAdjacency, or dense numpy / torch arrays (converted once per call)."""
        self.check_run(adjacency_matrices, initial_embeddings, time_steps, LSTM_initial_states)
        self._launched_loop = None
        some = next(iter(initial_embeddings.values()))
        device = some.device
        mats, dense_mats = self._matrices(adjacency_matrices, device)
        T = int(time_steps)
        h0 = {v: to_storage(init, self.float_dtype) for v, init in initial_embeddings.items()}   # storage type
        c0 = {v: LSTM_initial_states[v].to(torch.float32).contiguous() if v in LSTM_initial_states else None for v in h0}
        folded = {v: self._folded(v, mats) for v in self.var}
        if T > 0 and self.float_dtype == torch.float32:
            # (the fused plan reads the caller's embeddings in place and takes "no initial cell state" as such: no copies,
            # no zero fill)
            plan = self._plan_fused({v: LSTMStateTuple(c=c0[v], h=h0[v]) for v in h0}, mats, folded)
            if plan is not None and not self.check_h2_weights():   # (the plan's packings raised the guard: bf16x3 instead)
                plan = self._plan_fused({v: LSTMStateTuple(c=c0[v], h=h0[v]) for v in h0}, mats, folded)
            if plan is not None:
                return _States(plan(T), self._plan_keep)
        if self.float_dtype == torch.bfloat16:   # (no initial cell state = a null pointer to the bf16 cell kernel: no zero fill)
            return self._run_bf16({v: LSTMStateTuple(c=c0[v], h=h0[v]) for v in h0}, mats, dense_mats, T)
        states = {v: LSTMStateTuple(c=torch.zeros(h0[v].shape, dtype=torch.float32, device=h0[v].device) if c0[v] is None
                                    else c0[v], h=h0[v]) for v in h0}     # the cell state stays fp32
        if T > 0:
            plan = self._plan(states, mats, folded)
            if plan is not None and not self.check_h2_weights():
                plan = self._plan(states, mats, folded)
            if plan is not None:
                for t in range(T):
                    plan[t & 1]()
                return _States(plan[2][T & 1], self._plan_keep)
        for _ in range(T):
            states = self._step(states, mats, dense_mats, folded)
        return states

    def _run_bf16(self, states, mats, dense_mats, T):
        """bf16-storage forward (float_dtype=torch.bfloat16; BASELINE config 5): h, messages, aggregates and the
        projected messages Zx are bf16 in HBM, GEMMs are bf16 MFMA with fp32 accumulation, the cell state, LayerNorm
        and gate arithmetic fp32.  Three launches per step over ping-pong state buffers: message MLPs (vertex task
        with its Kx projection), adjacency products, cells (edge cell in gather-init mode)."""
        if dense_mats:
            raise NotImplementedError("bf16 storage: dense matrices appended as cell inputs")
        bf = dict(dtype=torch.bfloat16, device=self.store.theta.device)
        self._check_bf16_wiring()
        if T == 0:
            return {v: LSTMStateTuple(c=st.c if st.c is not None else torch.zeros(st.h.shape, dtype=torch.float32,
                                                                                    device=st.h.device), h=st.h)
                    for v, st in states.items()}
        # Between the steps the states live in two ping-pong buffers BLOCKED by 16 rows (include/tspgnn.h: the lstm
        # task's state_*_blocked, the mlp task's x_blocked) -- only the loop's own launches read them, and a tile is then
        # loaded and stored in contiguous runs instead of as pieces of 16 rows.  The first step reads the caller's
        # row-major states in place, the last one writes row-major results.  An h that a loop entry uses WITHOUT a message
        # MLP (it goes to an aggregation or straight into a cell input) stays row-major.
        f32 = dict(dtype=torch.float32, device=self.store.theta.device)
        blocked = {v: all("msg" in u for w in self.var for u in self.loop[w] if u["var"] == v) for v in self.var}
        rows = {v: st.h.shape[0] for v, st in states.items()}
        shape = {v: (_pad16(rows[v]) if blocked[v] else rows[v], d) for v, d in self.var.items()}
        buf = [{v: LSTMStateTuple(c=torch.empty(shape[v], **f32), h=torch.empty(shape[v], **bf)) for v in self.var}
               for _ in (0, 1)]
        last = {v: LSTMStateTuple(c=torch.empty(st.h.shape, **f32), h=torch.empty_like(st.h)) for v, st in states.items()}
        folded = {v: self._folded(v, mats, bf16_inference=True) for v in self.var}
        interleave = os.environ.get("TSPGNN_BF16_INTERLEAVE", "1") != "0"
        built = {}
        self._plan_keep = keep = [buf, last, states, built]
        for t in range(T):
            p, first, final = kind = (t & 1, t == 0, t == T - 1)
            if kind not in built:   # the step's _Ends and its parts: built once per kind, replayed
                ep = _Ends(states if first else buf[p], last if final else buf[1 - p], rows=rows,
                           blk_in={v: blocked[v] and not first for v in self.var},
                           blk_out={v: blocked[v] and not final for v in self.var})
                built[kind] = (ep, list(self._bf16_step(ep, mats, folded, interleave)))
            _run(built[kind][1])
        return _States(last, keep)

    def _split_arith(self, n_rows=None):
        """"h2" / "x3" when the selected split-operand kernels cover this network (widths 32/64, cell inputs in
        multiples of 32) and, when the row counts are given, this batch (they address rows with 32-bit element
        offsets: rows * 4d < 2^30); None = the fp32-MFMA kernels."""
        if n_rows is not None and any(int(n) * 4 * self.var[v] >= 2 ** 30 for v, n in n_rows.items()):
            return None
        if GEMM_ARITH[self.gemm] and all(c.x3_ok() for c in self._RNN_cells.values()) \
                and all(m.sizes[-1] in (32, 64) for m in self._msg_MLPs.values()):
            return self.active_arith()
        return None

    # ---- f16x2 range guard.  fp16 pieces cannot hold what fp32 -- the reference's type, graphnn.py:18 -- can: a weight
    # with 2^6 |w| >= 65504 or an activation >= 65504 overflows to inf.  Weights are checked where they are packed,
    # activations where the kernels split them; either way the network falls back to bf16x3, whose pieces have fp32's
    # exponent range.  The device words and the latches behind these methods are range_guard.RangeGuard's (store.guard).
    def active_arith(self):
        """Suffix of the split-operand entry points in force: "h2" / "x3" / None, after the range guard's say."""
        arith = GEMM_ARITH[self.gemm]
        return "x3" if arith == "h2" and self.store.guard.h2_off() else arith

    @property
    def launched_loop(self):
        """Which form the last call ran its T steps in: "loop" (one launch of tspgnn_mp_loop_h2), "resident" (one launch
        of tspgnn_mp_resident_h2) or None (the stepwise launches -- also when a batch had a loop plan but _loop_launch
        declined the wiring or the device declined the launch)."""
        return self._launched_loop

    @property
    def last_backward(self):
        """What the last backward pass ran (None before the first): {"forward": the tape's arithmetic -- "h2" (f16x2),
        "x3" (bf16x3), "f32" or "bf16" (bf16 storage); "backward": "h2" (the f16x2 cell kernels: only after an f16x2
        forward), "f32" (the fp32-MFMA kernels), "bf16-native" (the bf16-reading kernels on the tape as it is) or
        "bf16-widened" (fp32 kernels on widened tape slices); per variable "folded" (the cell's adjacency product folded
        through its kernel), "pushed" (the message MLP's last layer pushed into the cell), "fused_data" (the pushed cell's
        data gradient inside its backward launch) and "projected" (a folded cell's dy = dZx Kx^T inside the message MLP's
        launch); "chunk_steps" and "chunks": the weight gradients' chunking of the T steps}."""
        return self._last_backward

    def training_packs_h2(self):
        """A training step of this network packs weights into fp16 pieces (the f16x2 forward and backward, or the bf16-storage
        mode's message-MLP backward): a replayed training graph has to watch the range guard's weight word."""
        if self.float_dtype == torch.bfloat16:
            return bool(self.mlp_backward_h2 and self._mlp_h2_native_ok)
        return self.active_arith() == "h2"

    def forced_off_h2(self):
        """Context manager: f16x2 disabled inside (Session's re-run of a batch whose activations overflowed)."""
        return self.store.guard.forced_off()

    def leave_h2(self):
        """f16x2 is off for these variables, the bf16-native backward's message MLPs included, until they are assigned
        anew (a captured training step whose guard fired)."""
        self.store.guard.veto()
        self._mlp_h2_native_ok = False

    def check_h2_weights(self):
        """False if the weights just packed veto f16x2 (the caller rebuilds its launch plan: _split_arith now answers
        "x3"), True otherwise.  Takes the guard's weight word when packings were enqueued since the last look and the guard
        can look; past HALF the fp16 range the network is latched to bf16x3 until the variables are assigned anew."""
        guard = self.store.guard
        if GEMM_ARITH[self.gemm] != "h2" or guard.h2_off():
            return True    # (not in use, or already vetoed for these variables: the caller's plan stands)
        if guard.packs_pending and guard.can_look():
            return guard.vet_weights()
        return True

    def _single_consumers(self, own_width=False):
        """{source variable: (v, i)} when every variable's h feeds exactly one loop entry and that entry has a
        single-kernel message MLP (the wiring the fused cell + message launch covers), else None.  ``own_width`` (the
        training forward, whose tape keeps the hidden activations per SOURCE row): the MLP must also be square and of the
        source variable's own width."""
        consumers = {u: [] for u in self.var}
        for v in self.var:
            for i, u in enumerate(self.loop[v]):
                if "var" not in u or "fun" in u or "msg" not in u:
                    return None
                mlp = self._msg_MLPs[u["msg"]]
                if len(mlp._chunks()) != 1 or mlp.n_square < 1 or mlp._plan[3]:
                    return None
                if own_width and (mlp._plan[0] != "square" or mlp.sizes[-1] != self.var[u["var"]]):
                    return None
                consumers[u["var"]].append((v, i))
        if any(len(c) != 1 for c in consumers.values()):
            return None
        return {u: c[0] for u, c in consumers.items()}

    def _plan_fused(self, states, mats, folded):
        """bf16x3 plan with every message MLP fused behind the cell of its SOURCE variable: the launch that
        updates the states of step t also evaluates msg(h') -- the messages of step t+1 -- on the rows it
        still holds in registers (tspgnn_lnlstm_mlp_fwd_multi_x3), so a step is {adjacency products, one
        cell+message launch}.  The messages of step 0 come from one plain MLP launch, the last step runs
        the cells alone.  Applies when every variable's h feeds exactly one loop entry and that entry has a
        single-kernel message MLP; returns run(T) -> states, or None."""
        arith = self._split_arith({v: st.h.shape[0] for v, st in states.items()})
        if arith is None:
            return None
        consumers = self._single_consumers()
        if consumers is None:
            return None
        f32 = dict(dtype=torch.float32, device=self.store.theta.device)
        # f16x2: the states of a folded (edge-side) variable live BLOCKED by 16 rows between the steps (include/tspgnn.h,
        # tspgnn_cell_mlp_task.state_*_blocked): nothing but the variable's own cell task reads them -- the message MLP
        # takes h' from registers -- so the loop's ping-pong buffers are loaded and stored 1 KiB contiguous per
        # instruction; the first step reads the caller's row-major states, the last one writes row-major again.
        blocked = {v: arith == "h2" and folded[v] is not None for v in self.var}
        # f16x2: the cells' kernels (and with Kx the projected messages, and a pushed bias) are centred per gate, so that
        # the four gate LayerNorms of every row and step skip their mean pass (tspgnn_lstm_task.z_centered)
        cen = arith == "h2" and self.center_gates
        rows_of = {v: st.h.shape[0] for v, st in states.items()}

        def state_buffers():
            out = {}
            for v, st in states.items():
                rows = _pad16(rows_of[v]) if blocked[v] else rows_of[v]
                out[v] = LSTMStateTuple(c=torch.empty((rows, st.h.shape[1]), **f32), h=torch.empty((rows, st.h.shape[1]), **f32))
            return out
        # ping-pong buffers of the loop; the FIRST step reads the caller's states in place (row-major; c None = the zero
        # cell state, which the f16x2 kernels take as a null pointer: nothing is read), so nothing is copied or filled
        buf = [state_buffers(), state_buffers()]
        first_state = {v: LSTMStateTuple(c=st.c if st.c is not None or arith == "h2" else torch.zeros_like(st.h), h=st.h)
                       for v, st in states.items()}
        pushed = {v: self._pushable(v, mats, folded) for v in self.var}
        # message outputs / projected messages, double-buffered by step parity (a launch reads one set and
        # writes the other)
        mo = [{}, {}]
        zxs = [{}, {}]
        for v in self.var:
            for i, u in enumerate(self.loop[v]):
                rows, width = states[u["var"]].h.shape[0], self._msg_MLPs[u["msg"]].sizes[-1]
                for p in (0, 1):
                    if folded[v] is not None:
                        zxs[p][v] = torch.empty((_pad16(rows), 4 * self.var[v]), **f32)   # (fused plan: f16x2 / x3 only)
                    else:
                        mo[p][(v, i)] = torch.empty((rows, width), **f32)

        def ends(p, with_messages=True, first=False):
            """A step of parity p: it reads the messages of mo[p] / zxs[p]; ``first``: and the caller's (row-major) states;
            a step without messages is the last one and writes row-major states."""
            return _Ends(first_state if first else buf[p], buf[1 - p], rows=rows_of, zx=zxs[p], msg=mo[p],
                         blk_in={v: blocked[v] and not first for v in self.var},
                         blk_out={v: blocked[v] and with_messages for v in self.var})

        def message(v, i, p):
            """(wb, n_layers, relu_mask, out, proj_w, proj_out) of loop entry (v, i) writing parity-p buffers."""
            return self._fused_message(v, i, ends(p), folded, pushed, arith, cen)

        # messages of step 0 from the initial states (a folded receiver's message itself goes to a temporary of this launch)
        pre_ends = _Ends(first_state, None, zx=zxs[0], msg=dict(mo[0]))
        pre = [self._split_messages(pre_ends, {}, folded, pushed, arith, cen)]
        built = {}
        self._plan_keep = keep = [buf, mo, zxs, first_state, pre_ends, built]
        # the cells' packings are made here, not at the first step: the caller vets their range (check_h2_weights) between
        # the construction of the plan and its first launch
        self._prepack_cells(folded, pushed, arith, cen)

        loop_launch = self._loop_launch(states, mats, folded, pushed, consumers, message, first_state, arith, cen, keep) \
            if arith == "h2" else None

        def run(T):
            _run(pre)
            if loop_launch is not None:
                done = loop_launch(T)
                if done is not None:
                    return done
            for t in range(T):
                p, with_messages, first = kind = (t & 1, t < T - 1, t == 0)
                if kind not in built:   # the step's _Ends and its parts: built once per kind, replayed.  (The next step's
                    # _Ends is not kept: it names nothing but mo[1 - p] / zxs[1 - p], which _plan_keep holds.)
                    ep = ends(p, with_messages, first)
                    built[kind] = (ep, list(self._fused_step(ep, ends(1 - p) if with_messages else None, mats, folded, pushed,
                                                             consumers, arith, cen)))
                _run(built[kind][1])
            final = buf[T & 1]
            return {v: LSTMStateTuple(c=final[v].c[:rows_of[v]], h=final[v].h[:rows_of[v]]) for v in self.var}
        return run

    def _loop_launch(self, states, mats, folded, pushed, consumers, message, first_state, arith, cen, keep):
        """run(T) -> states through ONE launch of tspgnn_mp_loop_h2 (csrc/mp_loop_h2.hip: resident workgroups, edge
        states in registers, per-group synchronisation), or None when the wiring or the batch is not the one that kernel
        is written for: two variables of width 64, the "edge" one folded over a two-ones-per-row matrix that carries a
        work plan (DeviceAdjacency.loop_plan), the "vertex" one fed by the row-sum over the same matrix's transpose.
        Results are bit-identical to the stepwise launches of _plan_fused (tests/test_gpu_loop.py)."""
        if not loop_enabled() or not self.persistent_loop or len(self.var) != 2:
            return None
        ve = [v for v in self.var if folded[v] is not None]
        if len(ve) != 1:
            return None
        ve = ve[0]
        vv = [v for v in self.var if v != ve][0]
        if self.var[ve] != 64 or self.var[vv] != 64:
            return None
        ue, uvx = folded[ve], self.loop[vv]
        if len(uvx) != 1:
            return None
        uvx = uvx[0]
        if ue.get("var") != vv or uvx.get("var") != ve or uvx.get("mat") != ue["mat"] or not uvx.get("transpose?", False) \
                or "fun" in uvx or "msg" not in uvx or "msg" not in ue:
            return None
        adj = mats[ue["mat"]]
        if adj.loop_plan is None or adj.csr_t[2] is not None:
            return None
        plan_t, n_groups, grid, kind, n_slots, lds_words, n_active = adj.loop_plan
        cell_e, cell_v = self._RNN_cells[ve], self._RNN_cells[vv]
        if cell_v.dx != 64 or cell_e.dx != 64:
            return None
        M, N = states[ve].h.shape[0], states[vv].h.shape[0]
        f32 = dict(dtype=torch.float32, device=self.store.theta.device)
        # the edge side's message MLP (consumed by the vertex cell) and the vertex side's (consumed, projected, by the edge cell)
        e_wb, e_n, e_mask, e_out0, _, _ = message(vv, 0, 0)
        _, _, _, e_out1, _, _ = message(vv, 0, 1)
        v_wb, v_n, v_mask, _, v_pw, zx0 = message(ve, 0, 0)
        _, _, _, _, _, zx1 = message(ve, 0, 1)
        if e_out0 is None or zx0 is None or e_n > 3 or v_n > 4 or v_n < 1:   # (e_n <= 3: resident next to Kh in LDS)
            return None
        if pushed[vv]:
            mlp_e = self._msg_MLPs[uvx["msg"]]
            v_K, zb = cell_v.pushed_bias_pack(mlp_e, arith=arith, centered=cen)
            deg = adj.row_degrees(True)
        else:
            v_K, zb, deg = cell_v.packed("K", arith, cen), None, None
        e_K = cell_e.packed("Kh", arith, cen)
        out_e = LSTMStateTuple(c=torch.empty((M, 64), **f32), h=torch.empty((M, 64), **f32))
        out_v = LSTMStateTuple(c=torch.empty((N, 64), **f32), h=torch.empty((N, 64), **f32))
        vagg = [torch.empty((N, 64), **f32), torch.empty((N, 64), **f32)]
        counters = torch.zeros(4 * 32 * n_groups + 32, dtype=torch.int32, device=f32["device"])
        guard = self.store.guard
        fs_e, fs_v = first_state[ve], first_state[vv]
        resident = kind == "resident"
        a = _lib.MpResidentArgs() if resident else _lib.MpLoopArgs()
        if resident:   # the edge states between the steps, by tile slot (private to the launch)
            slots = [torch.empty((n_slots * 16, 64), **f32), torch.empty((n_slots * 16, 64), **f32)]
            a.e_hs, a.e_cs, a.n_slots, a.lds_words = _lib.ptr(slots[0]), _lib.ptr(slots[1]), n_slots, lds_words
            a.n_active = n_active
            a.flags = 1 if os.environ.get("TSPGNN_RES_SAFE") == "1" else 0   # (tests: the placement-independent acquire)
            vh = [torch.empty((N, 64), **f32), torch.empty((N, 64), **f32)]
            a.vh[0], a.vh[1] = _lib.ptr(vh[0]), _lib.ptr(vh[1])
            keep.extend([slots, vh])
        a.e_h0, a.e_c0, a.e_h, a.e_c = _lib.ptr(fs_e.h), _lib.ptr(fs_e.c), _lib.ptr(out_e.h), _lib.ptr(out_e.c)
        a.uv, a.e_K, a.e_ln = _lib.ptr(adj.uv), _lib.ptr(e_K), _lib.ptr(cell_e.ln())
        a.e_mlp_wb, a.e_mlp_layers, a.e_relu_mask = _lib.ptr(e_wb), e_n, e_mask
        a.msg[0], a.msg[1] = _lib.ptr(e_out0), _lib.ptr(e_out1)
        a.v_h0, a.v_c0, a.v_h, a.v_c = _lib.ptr(fs_v.h), _lib.ptr(fs_v.c), _lib.ptr(out_v.h), _lib.ptr(out_v.c)
        a.rowptr, a.eid = _lib.ptr(adj.csr_t[0]), _lib.ptr(adj.csr_t[1])
        a.v_K, a.v_ln, a.v_zbias, a.v_zscale = _lib.ptr(v_K), _lib.ptr(cell_v.ln()), _lib.ptr(zb), _lib.ptr(deg)
        a.v_mlp_wb, a.v_mlp_layers, a.v_relu_mask, a.v_proj_w = _lib.ptr(v_wb), v_n, v_mask, _lib.ptr(v_pw)
        a.zx[0], a.zx[1] = _lib.ptr(zx0), _lib.ptr(zx1)
        a.vagg[0], a.vagg[1] = _lib.ptr(vagg[0]), _lib.ptr(vagg[1])
        a.plan, a.counters, a.n_groups, a.grid = _lib.ptr(plan_t), _lib.ptr(counters), n_groups, grid
        a.M, a.N, a.z_centered = M, N, int(cen)
        a.range_flag, a.status = guard.flag_ptr(), guard.status_ptr()
        trace = None
        if os.environ.get("TSPGNN_LOOP_TRACE"):   # development: per-wavefront phase times (tools/loop_trace.py)
            trace = self.loop_trace = torch.zeros((grid, resident_plan.WAVES if resident else loop_plan.WAVES, 32 if resident else 16),
                                                  dtype=torch.int64, device=f32["device"])
        a.trace = _lib.ptr(trace)
        keep.extend([out_e, out_v, vagg, counters, plan_t, v_K, zb, deg, e_K, a, trace])

        unsupported = [False]

        def launch(T):
            """-> the final states, or None when the device cannot keep the launch's workgroups resident (the entry point
            asks the runtime before it launches anything and answers TSPGNN_EUNSUPPORTED): the caller then runs the
            stepwise launches."""
            if unsupported[0]:
                return None
            a.T = int(T)
            counters.zero_()
            try:
                _lib.call("tspgnn_mp_resident_h2" if resident else "tspgnn_mp_loop_h2", ctypes.byref(a), 64,
                          _lib.current_stream())
            except _lib.TspgnnError as e:
                if e.status != -2:
                    raise
                unsupported[0] = True
                return None
            self._launched_loop = kind
            return {ve: out_e, vv: out_v}
        return launch

    def _plan(self, states, mats, folded):
        """Pre-builds the launches of an even and an odd step over two ping-pong state buffers, so that
        the T-step loop is a handful of ctypes calls per step (the host stays ahead of the GPU even
        without HIP-graph replay).  Returns (run_even, run_odd, (states_if_T_even, states_if_T_odd)), or
        None when the wiring needs the general path (Python 'fun' entries, dense matrices, MLPs that do
        not fit one kernel)."""
        for v in self.var:
            for u in self.loop[v]:
                if "var" not in u or "fun" in u:
                    return None
                if "msg" in u and len(self._msg_MLPs[u["msg"]]._chunks()) != 1:
                    return None
        # buf[p] holds the states a step of parity p READS; it writes buf[1-p]
        buf = [{v: LSTMStateTuple(c=st.c.clone(), h=st.h.clone()) for v, st in states.items()},
               {v: LSTMStateTuple(c=torch.empty_like(st.c), h=torch.empty_like(st.h)) for v, st in states.items()}]
        arith = self._split_arith({v: st.h.shape[0] for v, st in states.items()})
        pushed = {v: self._pushable(v, mats, folded) for v in self.var}
        ends = [_Ends(buf[p], buf[1 - p]) for p in (0, 1)]
        steps = [list(self._split_step(ep, mats, {}, folded, pushed, arith)) for ep in ends]
        self._plan_keep = [ends, steps]   # buffers referenced by raw pointers inside the task structures
        return (lambda: _run(steps[0])), (lambda: _run(steps[1])), (buf[0], buf[1])

    def _step(self, states, mats, dense_mats, folded):
        """One synchronous step (graphnn.py:142-173) of the general path, built and run on the spot in the fp32 kernels: no
        cell is pushed, and a folded cell's Zx = y Kx is a launch of its own even behind a message MLP."""
        new_states = {v: LSTMStateTuple(c=torch.empty_like(st.c), h=torch.empty_like(st.h)) for v, st in states.items()}
        _run(self._split_step(_Ends(states, new_states), mats, dense_mats, folded, {v: False for v in self.var}, project=False))
        return new_states

    # ---------------------------------------------------------------- training: forward with a tape
    def check_training(self):
        """What forward_train / backward cover of this network's construction, asked before a training step launches or
        zeroes anything (Session.loss_and_grads, forward_train): NotImplementedError otherwise.  A message MLP trains
        with at most four layers (MLP_depth <= 3): the f16x2 / bf16x3 / bf16 training forwards and the fused backward
        tasks take single-kernel chains, and the several-kernel fp32 chain is only exercised at width 128."""
        if self.float_dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError("training runs with float_dtype torch.float32 or torch.bfloat16")
        for name, mlp in self._msg_MLPs.items():
            if mlp.n_square > 4:
                raise NotImplementedError("training: message MLP %s has %d layers, at most 4 (MLP_depth <= 3) are covered"
                                          % (name, mlp.n_square))

    def forward_train(self, adjacency_matrices, initial_embeddings, time_steps):
        """Same computation as __call__, keeping what the backward pass needs: every step's states,
        cell inputs and hidden MLP activations, each stored [T, rows, width] contiguous so that a
        variable's weight gradient is ONE reduction over all time steps (sized for 288 GB of HBM:
        ~10 GB at n=40, batch 128, T=32).  Returns (states, tape).

        float_dtype=torch.bfloat16 (bf16 storage, BASELINE config 5): the forward is the inference mode's (bf16 h,
        messages, aggregates, projected messages and hidden activations, bf16 MFMA with fp32 accumulation, fp32 c /
        LayerNorm / gates) and the tape holds those bf16 arrays -- half the bytes; see backward()."""
        T = int(time_steps)
        bf16 = self.float_dtype == torch.bfloat16
        self.check_training()
        self.check_run(adjacency_matrices, initial_embeddings, T, {})
        device = next(iter(initial_embeddings.values())).device
        f32 = dict(dtype=torch.float32, device=device)
        stored = dict(dtype=self.float_dtype, device=device)   # what the tape keeps of h, messages, activations
        if bf16 and any("fun" in u or "var" not in u for v in self.var for u in self.loop[v]):
            raise NotImplementedError("bf16-storage training supports loop entries made of var / msg / mat only")
        mats, dense = self._matrices(adjacency_matrices, device)
        tape = Tape()
        tape.T, tape.mats, tape.dense = T, mats, dense
        tape.folded = {v: self._folded(v, mats) for v in self.var}
        n = {v: initial_embeddings[v].shape[0] for v in self.var}
        tape.H = {v: torch.empty((T + 1, n[v], d), **stored) for v, d in self.var.items()}
        tape.C = {v: torch.empty((T + 1, n[v], d), **f32) for v, d in self.var.items()}
        # cell inputs; for a folded cell: the message y per SOURCE row and Zx = y Kx instead of the aggregate
        tape.X, tape.ZX = {}, {}
        for v in self.var:
            u = tape.folded[v]
            rows_x = n[v] if u is None else n[u["var"]]
            tape.X[v] = torch.empty((T, rows_x, self._RNN_cells[v].dx), **stored)
            if u is not None:
                tape.ZX[v] = torch.empty((T, _pad16(rows_x), 4 * self.var[v]), **stored)
        tape.acts = {}
        for v in self.var:
            to_storage(initial_embeddings[v], self.float_dtype, out=tape.H[v][0])   # (bf16 storage: rounded here, as the
                                                                                    # inference mode does)
            tape.C[v][0].zero_()
            for i, u in enumerate(self.loop[v]):
                if "msg" in u and "var" in u:
                    tape.acts[(v, i)] = None     # allocated below, once the arithmetic (hence the tape's form) is known

        def alloc_acts():
            for (v, i) in tape.acts:
                u = self.loop[v][i]
                mlp, src = self._msg_MLPs[u["msg"]], u["var"]
                layers = 1 if tape.rc.get((v, i)) else max(mlp.n_square - 1, 1)   # (recomputed: the messages only)
                if self._message_output_slot(v, i, tape.folded) is not None:
                    layers = mlp.n_square
                tape.acts[(v, i)] = torch.empty((layers, T, n[src], self.var[src]), **stored)
        if bf16:
            tape.arith = "bf16"
            tape.pushed = {v: False for v in self.var}
            alloc_acts()
            self._check_bf16_wiring(tape.folded)
            ends = self._tape_ends(tape)
            for t in range(T):   # (three launches per step as in _run_bf16, every output written into the tape)
                _run(self._bf16_step(ends(t), mats, tape.folded))
            return {v: LSTMStateTuple(c=tape.C[v][T], h=tape.H[v][T]) for v in self.var}, tape
        # forward GEMMs in the split-operand arithmetic selected by self.gemm (fp32-class accuracy).  With f16x2 the
        # cells' backward recomputes z in the same arithmetic (tspgnn_lnlstm_bwd_multi_h2; the tape's projected
        # messages ZX carry the factor 2^s both sides expect); with bf16x3 the backward is fp32 MFMA.
        arith = self._split_arith({v: initial_embeddings[v].shape[0] for v in self.var})
        pushable = {v: bool(self.push_training and not self.fuse_training_messages and self._pushable(v, mats, tape.folded))
                    for v in self.var}
        if arith == "h2":
            # the step's f16x2 packings up front (they are cached for the tasks below), so that the guard can veto them
            # before any kernel multiplies with them
            self._prepack_cells(tape.folded, pushable, "h2", False, with_kx_and_mlps=True)
            if not self.check_h2_weights():
                arith = self._split_arith({v: initial_embeddings[v].shape[0] for v in self.var})
        tape.arith = arith
        # pushed cells (f16x2): the tape's X[v] holds the row-sum of the message MLP's LAST HIDDEN activation and the cell
        # runs with K' = [W Kx ; Kh], z starting at degree * (b Kx) (LayerNormBasicLSTMCell.pushed_kernel)
        tape.pushed = {v: arith == "h2" and pushable[v] for v in self.var}
        # recomputed message MLPs (tspgnn_mlp_bwd_rc_h2): the pushed entries whose prefix the kernel covers
        for v in self.var:
            if tape.pushed[v] and self.recompute_messages:
                mlp = self._msg_MLPs[self.loop[v][0]["msg"]]
                tape.rc[(v, 0)] = mlp.recompute_ok(mlp.n_square - 1)
        alloc_acts()

        # f16x2, opt-in (fuse_training_messages): the message MLPs of step t+1 ride in the cell launch of step t, on the
        # rows of h' it still holds in registers (tspgnn_lnlstm_mlp_fwd_multi_h2 as in the inference plan, here writing
        # the tape: states, hidden activations, messages and projected messages of every step)
        consumers = self._single_consumers(own_width=True) \
            if arith == "h2" and (self.fuse_training_messages or any(tape.rc.values())) else None
        tape.fused = consumers is not None
        ends = self._tape_ends(tape)
        if consumers is not None:
            nxt = ends(0) if T > 0 else None
            if T > 0:   # the messages of step 0 from one plain launch
                _run([self._split_messages(nxt, dense, tape.folded, tape.pushed, arith, rc=tape.rc)])
            for t in range(T):
                ep, nxt = nxt, ends(t + 1) if t < T - 1 else None
                _run(self._fused_step(ep, nxt, mats, tape.folded, tape.pushed, consumers, arith, rc=tape.rc))
        else:
            for t in range(T):
                _run(self._split_step(ends(t), mats, dense, tape.folded, tape.pushed, arith, rc=tape.rc))
        states = {v: LSTMStateTuple(c=tape.C[v][T], h=tape.H[v][T]) for v in self.var}
        return states, tape

    def backward(self, tape, dstates):
        """Back-propagation through time of forward_train.  dstates: {var: (dh, dc)} gradients w.r.t. the
        final states (None = zero).  Parameter gradients are ADDED to the store's flat gradient buffer;
        returns {var: (d h0, d c0)} (gradients w.r.t. the initial embeddings / cell states).

        bf16-storage tape: gradients are fp32 throughout (the fp32-MFMA backward kernels on the widened tape), taken
        of the function the forward evaluated -- stored values as they were rounded, GEMM weights rounded to bf16,
        every rounding passed straight through -- and land on the fp32 master variables."""
        if tape.arith == "bf16":
            names = [c.base + "/kernel" for c in self._RNN_cells.values()]
            names += [ln + "/kernel" for m in self._msg_MLPs.values() for ln in m.layer_names]
            with self.store.rounded_to_bf16(names):
                return self._backward(tape, dstates)
        return self._backward(tape, dstates)

    @staticmethod
    def _fun_vjp(fun, h, g_out):
        """g_out (gradient w.r.t. fun(h)) pulled back to h.  A loop entry's 'fun' is the caller's own code (graphnn.py:149-151
        applies it to the states inside the TF graph, and tf.gradients differentiates it there): either it brings its
        vector-Jacobian product along -- ``fun.vjp(h, g_out) -> g_in`` -- or it is made of differentiable torch operations
        and is differentiated the same way TF would, by the framework's autograd on this one call."""
        vjp = getattr(fun, "vjp", None)
        if vjp is not None:
            return vjp(h, g_out).to(torch.float32)
        with torch.enable_grad():
            x = h.detach().to(torch.float32).requires_grad_(True)
            y = fun(x)
            if not y.requires_grad:       # a function that ignores its argument (or detaches): zero gradient
                return torch.zeros_like(x)
            (g_in,) = torch.autograd.grad(y, x, grad_outputs=g_out.to(y.dtype))
        return g_in

    def _vet_native_mlp_h2(self, tape):
        """bf16-native pass: -> the message MLPs' data gradient runs on tspgnn_mlp_bwd_multi_h2.  That kernel packs 2^s W^T
        into fp16 pieces, which the bf16 forward never vetted: pack up front and look at the guard's weight word (one
        4-byte read per backward pass) -- beyond half the fp16 range the pass uses tspgnn_mlp_bwd_multi_f32.  A pass being
        CAPTURED (or one without a device) cannot look: it follows the eager pass before it (Session.capture_train_step
        warms up eagerly) and its replays watch the word at the f16x2 guard's lag."""
        guard = self.store.guard
        can_look = guard.can_look()
        if not self.mlp_backward_h2 or not (can_look or self._mlp_h2_native_ok):
            return False
        for (v, i), acts in tape.acts.items():      # the packs the pass will use
            mlp = self._msg_MLPs[self.loop[v][i]["msg"]]
            if mlp.backward_h2_ok(acts):
                for l0, nl in mlp._chunks():
                    mlp.wt_packed(l0, l0 + nl - 1, mlp.sizes[-1], h2=True)
        if can_look:
            self._mlp_h2_native_ok = guard.vet_weights(latch=False)
        return self._mlp_h2_native_ok

    def _backward_plan(self, tape):
        """Every decision of a backward pass over ``tape``, taken before its first launch (the only reader of
        TSPGNN_BF16_BACKWARD and TSPGNN_FUSE_DATA_GRADIENTS); fills tape.native and last_backward.  -> a namespace of
          native: a bf16 tape read as it is by the bf16 kernels (widths 64 / 128; narrow widths widen slices of the tape for
          the fp32 kernels); cells: the cell kernels' arithmetic "bf16" / "h2" / "f32" (it follows the forward); form {var:
          "folded" | "pushed" | "plain"}; mlp_h2: the message MLPs' data gradient is f16x2 where the kernel covers the chain;
          fused_data / projected {var: its data-gradient GEMM rides in one of the step's launches -- a pushed cell's
          [d(aggregate) | dh] = dz K'^T as a second phase of its task, a folded cell's dy = dZx Kx^T as the head of its
          source MLP's chain}; n {var: rows}; per_step, CH: bytes of chunk buffers per step, steps per chunk."""
        T, rc, folded, device = tape.T, tape.rc, tape.folded, self.store.theta.device
        n = {v: tape.H[v].shape[1] for v in self.var}
        native = tape.arith == "bf16" and all(d in (64, 128) for d in self.var.values()) \
            and all(c.dx % 64 == 0 for c in self._RNN_cells.values()) \
            and os.environ.get("TSPGNN_BF16_BACKWARD", "native") == "native"
        tape.native = native
        cells = "bf16" if native else ("h2" if tape.arith == "h2" else "f32")
        form = {v: "folded" if folded[v] is not None else ("pushed" if tape.pushed[v] else "plain") for v in self.var}
        for v, cell in self._RNN_cells.items():
            if form[v] == "plain" and T > 0:
                cell.check_backward_data("bf16" if native else "f32")
        fuse_data = cells == "h2" and os.environ.get("TSPGNN_FUSE_DATA_GRADIENTS", "1") != "0"
        fused_data = {v: bool(fuse_data and form[v] == "pushed" and self._RNN_cells[v].fuses_pushed_data_gradient())
                      for v in self.var}
        projected = {}
        for v in self.var:
            u0 = self.loop[v][0]
            projected[v] = bool(
                fuse_data and form[v] == "folded" and "msg" in u0 and not rc.get((v, 0)) and self.mlp_backward_h2 and T > 0
                and self._msg_MLPs[u0["msg"]].backward_task_takes_projection(tape.acts_at((v, 0), 0)[0],
                                                                              4 * self._RNN_cells[v].d))
        per_step = sum(n[v] * 4 * d * 4 for v, d in self.var.items())
        per_step += sum(self._msg_MLPs[self.loop[v][i]["msg"]].n_square * n[self.loop[v][i]["var"]]
                        * self.var[self.loop[v][i]["var"]] * 4 * (0 if rc.get((v, i)) else 1)
                        for (v, i) in tape.acts)
        per_step += sum(tape.X[v].shape[1] * 4 * self.var[v] * 4 for v in self.var if form[v] == "folded")   # DZX
        per_step += sum(n[v] * 4 for v in self.var if form[v] == "pushed")          # degrees
        if tape.arith == "bf16" and not native:
            # widened fp32 copies of the chunk's tape slices (h, cell inputs, hidden activations) for the fp32 reductions
            per_step += sum(n[v] * d * 4 + tape.X[v].shape[1] * tape.X[v].shape[2] * 4 for v, d in self.var.items())
            per_step += sum(a.shape[0] * a.shape[2] * a.shape[3] * 4 for a in tape.acts.values())
        budget = self.wgrad_chunk_bytes
        if device.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            # never more than half of what is free next to the tape (smaller devices, other HBM sizes); memory the caching
            # allocator holds but has not handed out counts as free
            avail = torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
            budget = min(budget, avail // 2)
        # Weight gradients are one reduction per variable over a CHUNK of time steps: all T when the gradients w.r.t. the
        # pre-activations fit the budget (the C2 case, ~6 GB), else the largest chunk that does (a C5 shard: 84 GB for 64 steps)
        CH = max(1, min(T, int(budget // max(per_step, 1)))) if T > 0 else 1
        mlp_h2 = bool(self.mlp_backward_h2 and cells == "h2") or bool(native and self._vet_native_mlp_h2(tape))
        self._last_backward = {
            "forward": tape.arith or "f32", "backward": ("bf16-native" if native else "bf16-widened") if tape.arith == "bf16" else cells,
            "folded": {v: form[v] == "folded" for v in self.var}, "pushed": {v: form[v] == "pushed" for v in self.var},
            "fused_data": dict(fused_data), "projected": dict(projected), "chunk_steps": CH, "chunks": -(-T // CH)}
        return SimpleNamespace(n=n, native=native, cells=cells, form=form, mlp_h2=mlp_h2, fused_data=fused_data,
                               projected=projected, per_step=per_step, CH=CH)

    def _backward_buffers(self, tape, plan):
        """What a pass allocates once, from the plan -> a namespace of the chunk buffers DZ {var: dz [CH, rows, 4d]}, DZX
        (folded cells: dZx per source row), DPRE {(var, i): the message MLP's dpre [layers, CH, rows, d]}; RCP (recomputed
        entries: workgroup partials of {dW, db} over all T steps); ws (LayerNorm-gradient partials of all T steps, zeroed);
        push (pushed cells: message MLP, degrees, gradients w.r.t. W Kx [dx, 4d] and b Kx [4d]) -- folded after the loop."""
        n, CH = plan.n, plan.CH
        f32 = dict(dtype=torch.float32, device=self.store.theta.device)
        b = SimpleNamespace(DZX={}, DPRE={}, RCP={}, push={})
        b.DZ = {v: torch.empty((CH, n[v], 4 * d), **f32) for v, d in self.var.items()}
        for (v, i) in tape.acts:
            u = self.loop[v][i]
            mlp = self._msg_MLPs[u["msg"]]
            if tape.rc.get((v, i)):
                b.RCP[(v, i)] = mlp.backward_rc_partial(mlp.n_square - 1)
            else:       # (a pushed entry's last layer has its gradient formed on the receiving side)
                b.DPRE[(v, i)] = torch.empty((mlp.n_square - (plan.form[v] == "pushed"), CH, n[u["var"]], self.var[u["var"]]), **f32)
        b.ws = {v: _lib.workspace("tspgnn_lnlstm_bwd_workspace_floats", d, device=f32["device"]).zero_() for v, d in self.var.items()}
        for v, d in self.var.items():
            if plan.form[v] == "folded":
                b.DZX[v] = torch.empty((CH, tape.X[v].shape[1], 4 * d), **f32)
            if plan.form[v] == "pushed":
                deg = self._pushed_degrees(v, tape.mats)
                b.push[v] = dict(mlp=self._msg_MLPs[self.loop[v][0]["msg"]], deg=deg, deg_steps=deg.repeat(CH),
                                 g_wkx=torch.zeros((self._RNN_cells[v].dx, 4 * d), **f32), g_zb=torch.zeros((1, 4 * d), **f32))
        return b

    def _backward_weights(self, tape, plan, buf, t0, t1):
        """Weight gradients of steps [t0, t1): their dz / dpre sit in slots 0 .. t1-t0-1 of the chunk buffers."""
        steps, n = t1 - t0, plan.n
        for v, d in self.var.items():
            cell, push = self._RNN_cells[v], buf.push.get(v)
            x, h, dz = tape.x_steps(v, t0, t1), tape.h_steps(v, t0, t1), buf.DZ[v][:steps].view(-1, 4 * d)
            if plan.form[v] == "pushed":
                cell.pushed_backward_weights(x, h, dz, steps * n[v], push["deg_steps"], push["g_wkx"], push["g_zb"])
            elif plan.form[v] == "folded":
                cell.backward_weights_folded(x, buf.DZX[v][:steps].view(-1, 4 * d), steps * tape.X[v].shape[1], h, dz, steps * n[v])
            else:
                cell.backward_weights(x, h, dz, steps * n[v])
        for (v, i), dpre in buf.DPRE.items():
            u = self.loop[v][i]
            src, dsrc = u["var"], self.var[u["var"]]
            layers = dpre.shape[0]
            first = tape.h_steps(src, t0, t1)
            if "fun" in u:      # the MLP's input rows are fun(h), step by step as the forward formed them
                with torch.no_grad():
                    first = torch.cat([u["fun"](tape.h(src, t)).to(torch.float32) for t in range(t0, t1)], dim=0).contiguous()
            inputs = [first] + [tape.acts_steps((v, i), l, t0, t1) for l in range(layers - 1)]
            self._msg_MLPs[u["msg"]].backward_weights(inputs, [dpre[l, :steps].reshape(-1, dsrc) for l in range(layers)],
                                                      steps * n[src], n_layers=layers)

    def _cell_backward_task(self, v, t, tape, plan, buf, s):
        """v's task of step t's cell launch (recompute z, LayerNorm / gate gradients), in the plan's form."""
        cell, form = self._RNN_cells[v], plan.form[v]
        h_t, c_t = tape.h(v, t), tape.C[v][t]
        grads = (s.dH[v], s.dC[v], buf.DZ[v][s.k], s.ndC[v], buf.ws[v])
        if form == "folded":
            adj, zx_t = tape.mats[tape.folded[v]["mat"]], tape.zx(v, t)
            if plan.native:
                return cell.backward_task_bf16(None, h_t, c_t, *grads, adj=adj, zx=zx_t)
            s.keep += [h_t, zx_t]
            return cell.gather_backward_task(adj, zx_t, h_t, c_t, *grads, dh_in=s.ndH[v], defer=True, arith=plan.cells)
        if form == "pushed":
            push = buf.push[v]
            kp, zb = cell.pushed_bias_pack(push["mlp"], arith="h2")
            # (fused_data: [d(aggregate) | dh] = dz K'^T as a second phase of the task's workgroups, one launch less a step)
            data = (cell.packed("K", "h2T", pushed=push["mlp"]), s.dX[v], s.ndH[v]) if plan.fused_data[v] else None
            return cell.pushed_backward_task(tape.x(v, t), h_t, c_t, *grads, kp, zb, push["deg"], defer=True, data=data)
        x_t = tape.x(v, t)
        if plan.native:
            return cell.backward_task_bf16(x_t, h_t, c_t, *grads)
        s.keep += [h_t, x_t]
        return cell.backward_task(x_t, h_t, c_t, *grads, defer=True, arith=plan.cells)

    def _cell_backward_data(self, v, tape, plan, buf, s):
        """Data gradients of v's cell GEMMs: these WRITE dh (s.ndH[v]), the message paths ACCUMULATE into it.  s.dX[v] becomes
        the gradient w.r.t. the cell input -- folded: w.r.t. the message y (source rows); pushed: w.r.t. the aggregated last
        hidden activation."""
        cell, dz, gemm = self._RNN_cells[v], buf.DZ[v][s.k], "bf16" if plan.native else "f32"
        if plan.form[v] == "folded":
            # (fp32, d == 64: dh was formed by the cell launch; projected: dy = dZx Kx^T is left to the message MLP's launch)
            cell.gather_backward_data(tape.mats[tape.folded[v]["mat"]], dz, s.ndH[v] if plan.native or cell.d != 64 else None,
                                      buf.DZX[v][s.k], None if plan.projected[v] else s.dX[v], gemm)
        elif plan.form[v] == "plain":
            cell.backward_data(dz, s.dX[v], s.ndH[v], gemm)
        elif not plan.fused_data[v]:
            cell.pushed_backward_data(buf.push[v]["mlp"], dz, s.dX[v], s.ndH[v])

    def _message_backward(self, v, i, t, tape, plan, buf, s):
        """Loop entry (v, i) at step t, from the gradient w.r.t. its columns of v's cell input: the adjoint adjacency product
        (or its gather inside the MLP launch), the pull-back through 'fun', and the message MLP's data gradient -- as a task
        of the step's launch (s.mlp_tasks: plain, pushed prefix, or starting from the projection; s.rc_tasks: recomputed),
        else in launches of its own."""
        u = self.loop[v][i]
        if "var" not in u:      # an appended matrix is a constant of the graph: its columns' gradient ends here
            return
        off, w = sum(self._update_width(x) for x in self.loop[v][:i]), self._update_width(u)
        dy = s.dX[v] if len(self.loop[v]) == 1 else s.dX[v][:, off:off + w].contiguous()
        src, k, ndh = u["var"], s.k, s.ndH[u["var"]]
        mlp = self._msg_MLPs[u["msg"]] if "msg" in u else None
        adjoint = dict(transpose=not u.get("transpose?", False))    # of mat (x) y: mat^T (x) dy, and vice versa
        if mlp is not None and not tape.rc.get((v, i)):
            (acts_t, acts_stride), dpre = tape.acts_at((v, i), t), buf.DPRE[(v, i)]
            # the chain's forward output, read when its last layer has a relu (a pushed chain ends in a linear layer)
            y_out = None
            if mlp.relu[-1]:
                slot = self._message_output_slot(v, i, tape.folded)
                y_out = tape.x(v, t) if slot is None else acts_t[slot]
                s.keep.append(y_out)
            chain = (acts_t, acts_stride, y_out, dpre[:, k], dpre.stride(0))
        if "fun" in u:
            # graphnn.py:149-151: y = fun(h) ahead of the message MLP.  The gradient w.r.t. fun's OUTPUT is formed apart
            # (adjoint product, the MLP's backward on its own, never fused with another writer of dh), then pulled back
            # through fun (_fun_vjp) and added to dh of the source
            if "mat" in u:
                dy = tape.mats[u["mat"]].matmul(dy, **adjoint)
            if mlp is not None:
                g_out = torch.empty_like(ndh)
                mlp.backward_data(dy, *chain, g_out, accumulate=False, h2=False)
                dy = g_out
            ndh.add_(self._fun_vjp(u["fun"], tape.h(src, t), dy))
            return
        # The tasks of the step's launch accumulate into dh side by side: one per source.  A second writer of dh[src] runs
        # in launches of its own, ahead of it (a recomputed or pushed entry has no such form)
        first = src not in s.targets
        gather_uv = None
        if "mat" in u and plan.form[v] != "folded":
            adj = tape.mats[u["mat"]]
            if first and u.get("transpose?", False) and adj.uv is not None and mlp is not None \
                    and mlp.backward_task_fuses_gather(dy):
                gather_uv = adj.uv     # the adjoint of the row-sum is a two-row gather: the MLP launch forms it
            else:
                dy = adj.matmul(dy, **adjoint)
        if mlp is None:
            ndh.add_(dy)
            return
        if tape.rc.get((v, i)):     # the chain is recomputed from its input rows; data and weight gradients in one launch
            if not first:
                raise NotImplementedError("recomputed message MLP: a second writer of the source's gradient")
            h_src = tape.h(src, t)
            s.keep += [dy, h_src]
            s.rc_tasks.append((mlp, mlp.backward_rc_task(mlp.n_square - 1, h_src, tape.acts[(v, i)][0, t], dy, ndh, True,
                                                         gather_uv=gather_uv, partial=buf.RCP[(v, i)])))
            s.targets.append(src)
            return
        s.keep += [dy, acts_t]
        h2 = bool(plan.mlp_h2 and mlp.backward_h2_ok(acts_t))
        cell, task = self._RNN_cells[v], None
        if plan.form[v] == "pushed":   # the chain ends at the last hidden activation (a relu layer: masked by its output)
            if first:
                task = mlp.backward_prefix_task(dpre.shape[0], dy, acts_t, acts_stride, acts_t[dpre.shape[0] - 1], *chain[3:],
                                                ndh, True, gather_uv=gather_uv, h2=h2)
            if task is None:
                raise NotImplementedError("pushed training needs the message MLP's backward in one launch")
        elif plan.projected[v] and first:   # the chain starts from dZx Kx^T, formed inside the launch
            task = mlp.backward_task(None, *chain, ndh, True, h2=True, pre=(buf.DZX[v][k], cell.packed("Kx", "h2T")))
        else:
            if plan.projected[v]:
                _lib.call("tspgnn_linear_f32", _lib.ptr(buf.DZX[v][k]), 4 * cell.d, _lib.ptr(cell.packed("Kx", "f32T")), None, 0,
                          _lib.ptr(dy), cell.dx, 0, buf.DZX[v][k].shape[0], _lib.current_stream())
            if first:
                task = mlp.backward_task(dy, *chain, ndh, True, gather_uv=gather_uv, h2=h2)
        if task is None:    # several kernels, or a second writer
            mlp.backward_data(dy, *chain, ndh, accumulate=True, h2=h2)
        else:
            s.mlp_tasks.setdefault((self.var[src], h2), []).append(task)
            s.targets.append(src)

    def _backward(self, tape, dstates):
        """What _backward_plan decided, on _backward_buffers' arrays: per step, in reverse, the three launches (per width) of
        the builders above, the weight gradients flushed chunk by chunk, then the deferred reductions."""
        T, plan = tape.T, self._backward_plan(tape)
        buf = self._backward_buffers(tape, plan)
        f32 = dict(dtype=torch.float32, device=self.store.theta.device)
        dH = {v: (dstates.get(v, (None, None))[0]) for v in self.var}
        dC = {v: (dstates.get(v, (None, None))[1]) for v in self.var}
        for t in range(T - 1, -1, -1):
            # the step's own -- k: its slot in the chunk buffers (chunks start at multiples of CH); keep: what has to stay
            # alive until the step's launches are enqueued; targets: the sources whose dh a task of the message launch writes
            s = SimpleNamespace(k=t % plan.CH, dH=dH, dC=dC, keep=[], mlp_tasks={}, rc_tasks=[], targets=[])
            s.ndH = {v: torch.empty((plan.n[v], d), **f32) for v, d in self.var.items()}
            s.ndC = {v: torch.empty((plan.n[v], d), **f32) for v, d in self.var.items()}
            s.dX = {v: torch.empty((tape.X[v].shape[1], self._RNN_cells[v].dx), **f32) for v in self.var}
            # ---- 1: every cell's backward in one launch per width
            tasks = {}
            for v, d in self.var.items():
                tasks.setdefault(d, []).append(self._cell_backward_task(v, t, tape, plan, buf, s))
            _lib.call_by_width("tspgnn_lnlstm_bwd_multi_" + plan.cells, tasks)
            # ---- 2: data gradients of the cell GEMMs
            for v in self.var:
                self._cell_backward_data(v, tape, plan, buf, s)
            # ---- 3: adjoint adjacency products, then every message MLP's data gradient in one launch
            for v in self.var:
                for i in range(len(self.loop[v])):
                    self._message_backward(v, i, t, tape, plan, buf, s)
            for (d, h2), ts in s.mlp_tasks.items():
                _lib.call_by_width("tspgnn_mlp_bwd_multi_" + ("h2" if h2 else "f32"), {d: ts})
            for mlp, task in s.rc_tasks:
                _lib.call("tspgnn_mlp_bwd_rc_h2", ctypes.cast(ctypes.pointer(task), ctypes.c_void_p), mlp.sizes[-1],
                          _lib.current_stream())
            dH, dC = s.ndH, s.ndC
            if s.k == 0:      # the chunk [t, t + CH) is complete
                self._backward_weights(tape, plan, buf, t, min(t + plan.CH, T))
        for (v, i), part in buf.RCP.items():
            mlp = self._msg_MLPs[self.loop[v][i]["msg"]]
            mlp.backward_rc_finish(mlp.n_square - 1, part)
        for v in self.var:
            self._RNN_cells[v].backward_finish(buf.ws[v])      # LayerNorm parameters: the deferred per-step partials
            if plan.form[v] == "pushed":
                self._RNN_cells[v].pushed_backward_finish(buf.push[v]["mlp"], buf.push[v]["g_wkx"], buf.push[v]["g_zb"])
        return {v: (dH[v], dC[v]) for v in self.var}
