"""Cases for the f16x2 range guard (include/tspgnn.h, range_flag): one task per case whose operands are built so that
exactly one site of one kernel sees the event -- bit 0, an operand a kernel splits into fp16 pieces reaches 65520 in
magnitude (split2w, csrc/h2_tile.h); bit 1, a gate LayerNorm divides by a positive variance below (2^-5)^2 of the unscaled
z (ln_gate<..., TRACK>, csrc/mfma_tile.h) -- or that no site does.  tests/test_gpu_range_guard_sites.py launches them;
tests/test_range_guard_cases_host.py proves on the CPU, in float64, that every case is what it claims to be.

Two constants are the project's: QUIET = 65519 (the largest fp32 integer whose fp16 hi piece is finite) and RAISED = 65520
(rounds to inf), and the floor FLOOR = 2^-10.  Everything behind a GEMM cannot be planted exactly; there the designs keep
a factor of safety that no rounding of the kernels can bridge (design_faults, model_design_faults):
  bit 0 raised: the intended operand has an entry of magnitude >= BIG = 7.0e4;  quiet: every split operand <= SAFE = 6.0e4;
  bit 1 raised: the intended gate has a row of positive variance <= FLOOR / 4;  quiet: every positive row variance of every
  gate >= 4 FLOOR (the fp32 variance of an fp16-split z differs from the float64 one by far less than a factor of 4)."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from cell_fwd_cases import FwdCell, blocked_unpack, draw_mlp, mlp64, mlp_blocks, packed, pad16, t64, wscale
from lstm_bwd_cases import SENTINEL, SPARE, dev, empty
from tspgnn import _lib

QUIET, RAISED, NEGATIVE = 65519.0, 65520.0, -7.0e4
FLOOR = 2.0 ** -10
BIG, SAFE = 7.0e4, 6.0e4
BIAS_BIG = 73728.0          # 2^16 + 2^13: a bias that puts a whole column of a layer's output past BIG
GATE_NAMES = ("i", "j", "f", "o")

# (d, mode, dx, fused MLP) -> the f16x2 task's path, as MODES of tests/test_gpu_cell_forward_edges.py names it: "r" resident
# (kloop over a tile taken by ticket), "l1p" lock-step with the operand preload ((dx + d) / 32 <= 4), "l1" lock-step, K
# staged whole, without the preload, "l2" lock-step with K in two chunks
SITE_KEYS = {(64, "plain", 0, False): "r", (64, "gather", 0, True): "r", (64, "plain", 64, False): "r",
             (32, "gather", 0, False): "r", (32, "plain", 0, True): "r", (32, "bias", 32, False): "r",
             (64, "bias", 64, True): "l1p", (32, "plain", 32, True): "l1p", (32, "plain", 256, True): "l1",
             (64, "plain", 192, False): "l2", (64, "plain", 192, True): "l2", (32, "plain", 320, True): "l2"}


def path_of(task_plan):
    """A CellTaskPlan (tests/plan_replay.py) in the words of SITE_KEYS."""
    if task_plan.mode == "resident":
        return "r"
    return "l%d%s" % (task_plan.chunks, "p" if task_plan.preload else "")


def row_cases(nw):
    """(rows, row): the first row; the last row of a partial last tile; the only task of one row; the only live row of a
    second lock-step round (16 nw + 1 rows with nw tiles per round)."""
    return [(1, 0), (17, 0), (17, 16), (16 * nw + 1, 16 * nw)]


def operand_columns(width):
    """One column in each 16-column half of every 32-column k-block of an operand."""
    return [32 * kb + 16 * half + 5 for kb in range(width // 32) for half in (0, 1)]


def site_cell(d, mode, dx, mlp, rows, seed, **kw):
    """The f16x2 task of a SITE_KEYS entry, shaped as mode_cell of tests/test_gpu_cell_forward_edges.py shapes it."""
    if not mlp:
        return FwdCell("h2", d, rows, seed, dx=dx, mode=mode, **kw)
    acts = "default" if mode == "gather" else "strided"
    if dx == 0:
        return FwdCell("h2", d, rows, seed, mode=mode, mlp_layers=3, relu_mask=0b111 if mode == "gather" else 0b101, acts=acts, **kw)
    return FwdCell("h2", d, rows, seed, dx=dx, mode=mode, mlp_layers=4, relu_mask=0b0111, proj=True, acts=acts, **kw)


# ------------------------------------------------------------------------------------------------- the design conditions
Design = namedtuple("Design", "word site exact gates")
"""What a case claims.  word: the range_flag it must leave (0, 1 or 2).  site: the one operand meant to cross (bit 0), with
exact = its planted largest magnitude (QUIET for a planted value that must NOT raise) or None (behind a GEMM: >= BIG).
gates: the gates (0 .. 3 = i, j, f, o) meant to hold a row of positive variance below the floor (bit 1)."""

QUIET_DESIGN = Design(0, None, None, ())


def absmax(ops):
    return {s: float(t.abs().max()) if t.numel() else 0.0 for s, t in ops.items() if s != "var"}


def min_positive_variance(ops):
    """Per gate, the smallest positive row variance (inf where every row's is exactly 0)."""
    if "var" not in ops:
        return None
    var = ops["var"]
    big = torch.full_like(var, float("inf"))
    return [float(v) for v in torch.where(var > 0, var, big).min(dim=0).values]


def design_faults(ops, design):
    """-> the conditions of the module docstring that the float64 operands of a case miss (empty: the case is what it claims)."""
    bad = []
    for s, m in absmax(ops).items():
        if s == design.site:
            if design.exact is not None and m != abs(design.exact):
                bad.append("%s: largest magnitude %r, planted %r" % (s, m, design.exact))
            if design.exact is None and not m >= BIG:
                bad.append("%s: largest magnitude %.4g < %.4g" % (s, m, BIG))
        elif not m <= SAFE:
            bad.append("%s: largest magnitude %.4g > %.4g and not the intended site" % (s, m, SAFE))
    if design.site is not None and design.site not in ops:
        bad.append("no operand %s" % design.site)
    if (design.word & 1) != int(design.site is not None and design.exact != QUIET):
        bad.append("bit 0 of the expected word does not follow from the site")
    mv = min_positive_variance(ops)
    if mv is None:
        if design.gates:
            bad.append("gates named for a task without a cell")
    else:
        for g, v in enumerate(mv):
            if g in design.gates and not v <= FLOOR / 4:
                bad.append("gate %s: smallest positive variance %.3g > floor / 4" % (GATE_NAMES[g], v))
            if g not in design.gates and not v >= 4 * FLOOR:
                bad.append("gate %s: smallest positive variance %.3g < 4 floor and not an intended gate" % (GATE_NAMES[g], v))
    if bool(design.word & 2) != bool(design.gates):
        bad.append("bit 1 of the expected word does not follow from the gates")
    return bad


# --------------------------------------------------------------------------------------------------------- bit 0: cells
def plant(case, site, row, col, value):
    """One entry of x, of h (a cell) or of the input X (a plain MLP task, site "layer1")."""
    field = {"x": "x", "h": "h", "layer1": "X"}[site]
    getattr(case, field)[row, col] = value
    return Design(int(abs(value) >= RAISED), site, value, ())


def planted_sites(cell):
    """(site, width) of the operands of a cell task an entry can be planted in."""
    return ([("x", cell.dx)] if cell.dx else []) + [("h", cell.d)]


def plant_bias(cell, layer, col=11):
    """Fused launch: the bias entry `col` of layer `layer` (1-based) at BIAS_BIG, the row `col` of what consumes that
    layer's output -- the next layer's weights, the projection matrix behind the last layer -- zero: the column overflows at
    exactly one site, in every row, and the float64 reference stays finite and of ordinary size."""
    cell.layers[layer - 1][1][col] = BIAS_BIG
    if layer < cell.L:
        cell.layers[layer][0][col, :] = 0.0
        return Design(1, "layer%d" % (layer + 1), None, ())
    assert cell.P is not None, "nothing splits the last layer's output of this task"
    cell.P[col, :] = 0.0
    return Design(1, "proj", None, ())


def bias_sites(cell):
    """The layers whose output something in the launch splits."""
    return [l for l in range(1, cell.L + 1) if l < cell.L or cell.P is not None]


def plant_new_h(cell, col=11):
    """Fused launch: h' itself, the first MLP layer's operand.  LayerNorm bounds c' only through its own parameters: state
    beta[col] = 1e5 puts c'[:, col] near 1e5, output gamma[col] = 0 with beta[col] = 20 opens the output gate (sigmoid(20) =
    1 - 2e-9), so h'[:, col] ~ 1e5 in every row; row `col` of layer 1's weights is zero."""
    assert cell.L > 0
    cell.ln[4, 1, col] = 1.0e5
    cell.ln[3, 0, col], cell.ln[3, 1, col] = 0.0, 20.0
    cell.layers[0][0][col, :] = 0.0
    return Design(1, "layer1", None, ())


# ------------------------------------------------------------------------------------------------ bit 0: the plain MLPs
class MlpCase(object):
    """One task of tspgnn_mlp_fwd_multi_h2 (proj: with the projection second phase) or tspgnn_mlp_head_fwd_h2 (head), drawn
    as tests/test_gpu_split_kernels.py draws it: X, layers, P, hw / hb are NumPy fields, changed before launch()."""

    def __init__(self, d, rows, n_layers, mask, seed, proj=False, head=False):
        assert not (proj and head)
        rng = np.random.RandomState(seed)
        self.d, self.rows, self.L, self.mask, self.head = d, rows, n_layers, mask, head
        self.X = rng.randn(rows, d).astype(np.float32)
        self.layers = draw_mlp(rng, d, n_layers)
        self.P = (rng.randn(d, 4 * d) / np.sqrt(d)).astype(np.float32) if proj else None
        self.hw, self.hb = (rng.randn(d, 1) / np.sqrt(d)).astype(np.float32), np.array([0.3], np.float32)
        self._ref = None

    def plan(self):
        return (self.rows, self.L, self.P is not None)

    def launch(self, device):
        d, rows = self.d, self.rows
        self.buf = {"Y": empty((rows + SPARE, d), device, SENTINEL),
                    "acts": empty((max(self.L - 1, 1), rows + SPARE, d), device, SENTINEL)}
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        if self.P is not None:
            self.buf["proj"] = empty((pad16(rows) + SPARE, 4 * d), device, SENTINEL)
        task = _lib.MlpTask(_lib.ptr(dev(self.X, device)), _lib.ptr(mlp_blocks("h2", self.layers, device)), _lib.ptr(self.buf["Y"]),
                            _lib.ptr(self.buf["acts"]), (rows + SPARE) * d, rows, self.L, self.mask,
                            _lib.ptr(packed("h2", self.P, device)) if self.P is not None else None,
                            _lib.ptr(self.buf.get("proj")), _lib.ptr(self.flag))
        if self.head:
            self.buf["y"] = empty((rows + SPARE, 1), device, SENTINEL)
            _lib.call("tspgnn_mlp_head_fwd_h2", ctypes.cast(ctypes.pointer(task), ctypes.c_void_p), _lib.ptr(dev(self.hw, device)),
                      _lib.ptr(dev(self.hb, device)), _lib.ptr(self.buf["y"]), d, None)
        else:
            _lib.call_multi("tspgnn_mlp_fwd_multi_h2", [task], d)
        torch.cuda.synchronize()

    def range_flag(self):
        return int(self.flag.item())

    def _named(self):
        """-> [(name, buffer as row-major rows, the same unscaled)]."""
        out = [("Y", self.buf["Y"], self.buf["Y"])]
        if self.L > 1:
            out.append(("acts", self.buf["acts"], self.buf["acts"]))
        if self.P is not None:
            raw = blocked_unpack(self.buf["proj"])
            out.append(("proj", raw, raw / wscale("h2")))
        if self.head:
            out.append(("y", self.buf["y"], self.buf["y"]))
        return out

    def outputs(self):
        return {n: t[..., :self.rows, :] for n, _, t in self._named()}

    def untouched(self):
        return [n for n, raw, _ in self._named() if not bool(raw[..., self.rows:, :].eq(SENTINEL).all())]

    def reference(self, device):
        if self._ref is None:
            outs = mlp64(t64(self.X, device), self.layers, self.mask, device)
            ref = {"Y": outs[-1]}
            if self.L > 1:
                ref["acts"] = torch.stack(outs[:-1])
            if self.P is not None:
                ref["proj"] = outs[-1] @ t64(self.P, device)
            if self.head:
                ref["y"] = outs[-1] @ t64(self.hw, device) + t64(self.hb, device)
            ops = {"layer%d" % (l + 1): a for l, a in enumerate([t64(self.X, device)] + outs[:-1])}
            if self.P is not None:
                ops["proj"] = outs[-1]
            self._ref, self._ops = ref, ops
        return self._ref

    def operands(self, device):
        """{site: float64 tensor} of what the launch splits: "layer1" (X) .. "layerL", "proj" (the projection's input)."""
        self.reference(device)
        return self._ops


def plant_chain(case, target, row, col=13):
    """Plain MLP launch, row-specific: X[row, col] = 6.0e4 (in range) travels down column `col` alone -- row `col` of every
    weight matrix on the way is zero but for its diagonal entry -- and leaves layer `target` (1-based) as 7.5e4: through
    1.25 at target = 1, through 0.5 (3.0e4), ones, and 2.5 otherwise.  Row `col` of what consumes layer `target`'s output
    (layer target + 1, or P behind the last layer) is zero.  Only `row` overflows, and only at that one site."""
    gains = [1.25] if target == 1 else [0.5] + [1.0] * (target - 2) + [2.5]
    case.X[row, col] = SAFE
    for l, gain in enumerate(gains):
        W = case.layers[l][0]
        W[col, :] = 0.0
        W[col, col] = gain
    if target < case.L:
        case.layers[target][0][col, :] = 0.0
        return Design(1, "layer%d" % (target + 1), None, ())
    assert case.P is not None
    case.P[col, :] = 0.0
    return Design(1, "proj", None, ())


def chain_targets(case):
    return [t for t in range(1, case.L + 1) if t < case.L or case.P is not None]


MLP_KINDS = {"plain": dict(n_layers=3, mask=0b111), "proj": dict(n_layers=4, mask=0b0111, proj=True),
             "head": dict(n_layers=3, mask=0b111, head=True)}


def mlp_case(kind, d, rows, seed):
    return MlpCase(d, rows, seed=seed, **MLP_KINDS[kind])


# ----------------------------------------------------------------------------------------------------------------- bit 1
def gate_factor(cell):
    """The power of two that takes a gate's z below the floor: the variance of a row of z is ~1 in plain mode and ~3 in
    gather mode (2^-18 of it <= FLOOR / 4 = 2^-12), up to ~39^2 in bias mode (degrees 0 .. 39 times a unit zbias: 2^-24)."""
    return 2.0 ** -12 if cell.mode == "bias" else 2.0 ** -9


def scale_gates(cell, gates, factor=None):
    """The columns of the named gates of K -- and of Zx (gather) or zbias (bias): everything that feeds those gates' z."""
    f, d = np.float32(factor or gate_factor(cell)), cell.d
    for g in gates:
        cols = slice(g * d, (g + 1) * d)
        cell.K[:, cols] *= f
        if cell.mode == "gather":
            cell.Zx[:, cols] *= f
        if cell.mode == "bias":
            cell.zbias[cols] *= f
    return Design(2, None, None, tuple(sorted(gates)))


def private_sources(cell, row):
    """gather mode: `row` gets the last two rows of Zx for itself (no other row gathers them)."""
    assert cell.mode == "gather" and cell.n_src > 2
    cell.uv %= cell.n_src - 2
    cell.uv[row] = (cell.n_src - 2, cell.n_src - 1)


def scale_row(cell, row, factor):
    """Everything that feeds z of one row times `factor` (a power of two, or 0): its x, its h, in gather mode its two private
    source rows, in bias mode its degree 0 (no bias term).  factor = 0: z is exactly 0, a variance the guard ignores."""
    f = np.float32(factor)
    cell.h[row] *= f
    if cell.dx:
        cell.x[row] *= f
    if cell.mode == "gather":
        private_sources(cell, row)
        cell.Zx[cell.n_src - 2:] *= f
    if cell.mode == "bias":
        cell.zscale[row] = 0.0
    return Design(2, None, None, (0, 1, 2, 3)) if factor else QUIET_DESIGN


# ------------------------------------------------------------------------------------------ the cases, one generator each
# Every generator yields (label, task, Design) with a freshly drawn task per case; the GPU test launches exactly what the
# host test has judged.
def _seed(*key):
    return 1000 + sum(int(k) * w for k, w in zip(key, (1, 3, 7, 11, 13)))


def planted_cell_cases(d, mode, dx, mlp, rows, row):
    """One entry of x or h at QUIET, RAISED, NEGATIVE, in each half of every k-block."""
    for site, width in planted_sites(site_cell(d, mode, dx, mlp, 1, 0)):
        for col in operand_columns(width):
            for value in (QUIET, RAISED, NEGATIVE):
                cell = site_cell(d, mode, dx, mlp, rows, _seed(d, dx, rows, mlp))
                yield "%s[%d, %d] = %g" % (site, row, col, value), cell, plant(cell, site, row, col, value)


def fused_site_cases(d, mode, dx, rows):
    """Fused launch: h' into layer 1, the input of each later layer, the projection's input."""
    cell = site_cell(d, mode, dx, True, rows, _seed(d, dx, rows, 1))
    yield "h' into layer 1", cell, plant_new_h(cell)
    for layer in bias_sites(cell):
        cell = site_cell(d, mode, dx, True, rows, _seed(d, dx, rows, 1))
        yield "bias of layer %d" % layer, cell, plant_bias(cell, layer)
    yield "ordinary operands", site_cell(d, mode, dx, True, rows, _seed(d, dx, rows, 1)), QUIET_DESIGN


def planted_mlp_cases(kind, d, rows, row):
    for col in operand_columns(d):
        for value in (QUIET, RAISED, NEGATIVE):
            case = mlp_case(kind, d, rows, _seed(d, 0, rows))
            yield "X[%d, %d] = %g" % (row, col, value), case, plant(case, "layer1", row, col, value)


def chain_mlp_cases(kind, d, rows, row):
    for target in chain_targets(mlp_case(kind, d, 1, 0)):
        case = mlp_case(kind, d, rows, _seed(d, 0, rows))
        yield "layer %d's output[%d]" % (target, row), case, plant_chain(case, target, row)
    case = mlp_case(kind, d, rows, _seed(d, 0, rows))
    case.X[row, 13] = SAFE          # the chain's start alone: in range at every site
    yield "X[%d, 13] = 6.0e4 alone" % row, case, QUIET_DESIGN


def gate_cases(d, mode, dx, mlp, rows, centred):
    """Each gate alone below the floor, and each gate alone above it."""
    for g in range(4):
        for gates in ((g,), tuple(k for k in range(4) if k != g)):
            cell = site_cell(d, mode, dx, mlp, rows, _seed(d, dx, rows, mlp))
            design = scale_gates(cell, gates)
            yield "gates %s scaled" % "".join(GATE_NAMES[k] for k in gates), (cell.centred() if centred else cell), design


def one_row_cases(d, mode, dx, mlp, rows, row, centred):
    """One row's z at 2^-9 of its size (raises), and exactly 0 (does not)."""
    for factor in (2.0 ** -9, 0.0):
        cell = site_cell(d, mode, dx, mlp, rows, _seed(d, dx, rows, mlp))
        design = scale_row(cell, row, factor)
        yield "row %d times %g" % (row, factor), (cell.centred() if centred else cell), design


def pad_fill_cell(d, mode, dx, mlp, rows=17):
    """Blocked input states whose pad rows hold 1e30: memory the task does not own."""
    return site_cell(d, mode, dx, mlp, rows, _seed(d, dx, rows, mlp), in_blocked=True, out_blocked=True, pad_fill=1.0e30)


def companion_cells(d, v_rows):
    """An edge task (resident) beside a lock-step vertex task of v_rows rows whose LAST row -- the row the clamped lanes of
    its partial tile read again -- holds 6.0e4 in x and in h: in range."""
    edge = FwdCell("h2", d, 100, _seed(d, 0, 100), mode="gather", mlp_layers=3, acts="default", out_blocked=True)
    vertex = FwdCell("h2", d, v_rows, _seed(d, d, v_rows), dx=d, mode="bias", mlp_layers=4, relu_mask=0b0111, proj=True,
                     acts="strided", out_blocked=True)
    vertex.x[v_rows - 1, 21] = SAFE
    vertex.h[v_rows - 1, 37 % d] = SAFE
    return [edge, vertex]


# ---------------------------------------------------------------------------------------------------- the whole model
# tests/test_gpu_range_guard_loop.py: the same events through Session.forward_device on the stepwise launches, tspgnn_mp_loop_h2
# and tspgnn_mp_resident_h2.  What the f16x2 forward of the d = 64 network splits, in the names of
# oracle/torch_oracle.RangeSites: the edge cell is folded (z = Zx[u] + Zx[v] + h Kh: it splits h only), the vertex cell pushed
# (it splits the row-sum of E_msg_V's last hidden activation, and h), V_msg_E's output is the projection's operand, the
# vote head's last layer is an fp32 dot product.
MODEL_SPLIT = ["TSP/E_msg_V_MLP_layer_1", "TSP/E_msg_V_MLP_layer_2", "TSP/E_msg_V_MLP_layer_3", "V_cell/x_pushed", "V_cell/h",
               "TSP/V_msg_E_MLP_layer_1", "TSP/V_msg_E_MLP_layer_2", "TSP/V_msg_E_MLP_layer_3", "TSP/V_msg_E_MLP_layer_4",
               "TSP/V_msg_E_out", "E_cell/h", "E_vote_MLP_layer_1", "E_vote_MLP_layer_2", "E_vote_MLP_layer_3"]
MODEL_GATES = [(c, g) for c in ("E", "V") for g in ("input", "transform", "forget", "output")]
CELL = "TSP/%s_cell/layer_norm_basic_lstm_cell/"
MSG_DEPTH = {"E_msg_V": 4, "V_msg_E": 4}
# h' of a cell feeds: its own Kh, the message MLP that reads it, and (E) the vote head
H_SITES = {"E": ["E_cell/h", "TSP/E_msg_V_MLP_layer_1", "E_vote_MLP_layer_1"], "V": ["V_cell/h", "TSP/V_msg_E_MLP_layer_1"]}
READER = {"E": "E_msg_V", "V": "V_msg_E"}

ModelCase = namedtuple("ModelCase", "label params sizes T word sites gates")
"""params: the variables (oracle/params.py names); sizes, T: tspgnn.synthetic_batch(sizes, seed=3) and the step count;
word: the guard word an unguarded f16x2 forward must leave; sites: the MODEL_SPLIT operands meant to reach BIG (every other
stays within SAFE); gates: the MODEL_GATES meant to hold a row of positive variance <= FLOOR / 4 (every other >= 4 FLOOR)."""


def model_params(seed):
    from oracle import params as P
    return {k: np.array(v, copy=True) for k, v in P.init_params(64, seed=seed, perturb=True).items()}


def _layer(msg, l, what):
    return "TSP/%s_MLP_layer_%d/%s" % (msg, l, what)


def _zero_consumers_of_message(p, msg, layer, j):
    """Row j of what reads the output of layer `layer` of `msg`: the next layer; behind V_msg_E's last one the x half of the
    edge cell's kernel (the projection multiplies with it)."""
    if layer < MSG_DEPTH[msg]:
        p[_layer(msg, layer + 1, "kernel")][j, :] = 0.0
        return "TSP/%s_MLP_layer_%d" % (msg, layer + 1)
    assert msg == "V_msg_E", "E_msg_V's output is summed over a vertex's edges: the aggregate case"
    p[CELL % "E" + "kernel"][j, :] = 0.0
    return "TSP/V_msg_E_out"


def model_bias_case(msg, layer, sizes, T, seed, j=11):
    """One bias entry of a message MLP's layer at BIAS_BIG, the consumer's row j zero: that layer's output column j is beyond
    the range in every row and at every evaluation -- the launch of step 0's messages included."""
    p = model_params(seed)
    p[_layer(msg, layer, "bias")][j] = BIAS_BIG
    site = _zero_consumers_of_message(p, msg, layer, j)
    return ModelCase("%s layer %d bias" % (msg, layer), p, sizes, T, 1, (site,), ())


def _open_state_column(p, cell, j, value):
    """h'[:, j] ~ value in every row and step: state beta[j] = value, the output gate's gamma[j] = 0 and beta[j] = 20
    (sigmoid(20) = 1 - 2e-9); row j of the cell's own Kh half and (E) of the vote head's first layer zero."""
    base = CELL % cell
    p[base + "state/beta"][j] = value
    p[base + "output/gamma"][j], p[base + "output/beta"][j] = 0.0, 20.0
    p[base + "kernel"][64 + j, :] = 0.0
    if cell == "E":
        p["E_vote_MLP_layer_1/kernel"][j, :] = 0.0


def model_new_h_case(cell, sizes, T, seed, j=11):
    """A cell's h' beyond the range (T >= 2: the next step's cell splits it as well); row j of the reading MLP's first
    layer zero."""
    assert T >= 2
    p = model_params(seed)
    _open_state_column(p, cell, j, 1.0e5)
    p[_layer(READER[cell], 1, "kernel")][j, :] = 0.0
    return ModelCase("%s cell new h" % cell, p, sizes, T, 1, tuple(H_SITES[cell]), ())


def model_chain_case(cell, target, sizes, T, seed, j=11):
    """The overflow only where the launches BEHIND step 0's messages can see it: h'[:, j] = 3.0e4 (in range; the initial
    embeddings are of ordinary size), carried down column j of the reading MLP alone -- ones on the diagonal, 2.5 in layer
    `target` -- so that layer `target`'s output column j is 7.5e4 whenever the MLP reads a cell's output and ordinary when it
    reads the initial embeddings; the consumer's row j zero.  The plain MLP launch of step 0 stays in range: what raises the
    word is the fused cell launch, or the one-launch loop."""
    assert T >= 2
    msg = READER[cell]
    p = model_params(seed)
    _open_state_column(p, cell, j, 3.0e4)
    for l in range(1, target + 1):
        W = p[_layer(msg, l, "kernel")]
        W[j, :] = 0.0
        W[j, j] = 2.5 if l == target else 1.0
    site = _zero_consumers_of_message(p, msg, target, j)
    return ModelCase("%s layer %d behind new h" % (msg, target), p, sizes, T, 1, (site,), ())


def model_aggregate_case(sizes, T, seed):
    """E_msg_V's last hidden layer with a bias of 3000: a vertex of a 40-vertex graph sums 39 of them (117 000), of a
    20-vertex graph 19 (57 000)."""
    p = model_params(seed)
    p[_layer("E_msg_V", 3, "bias")][:] = 3000.0
    big = max(sizes) - 1 > BIG / 3000.0
    return ModelCase("aggregate %s" % "+".join(str(n) for n in sizes), p, sizes, T, int(big), ("V_cell/x_pushed",) if big else (), ())


def model_gate_case(cell, gate, sizes, T, seed):
    """One gate's columns of a cell's kernel -- both halves: everything that gate's z is made of -- times 2^-9 (E: a row's
    variance is ~0.1) or 2^-12 (V: it is up to ~10^2, the sum over a vertex's edges)."""
    p = model_params(seed)
    g = ("input", "transform", "forget", "output").index(gate)
    p[CELL % cell + "kernel"][:, 64 * g:64 * (g + 1)] *= np.float32(2.0 ** -9 if cell == "E" else 2.0 ** -12)
    return ModelCase("%s cell gate %s" % (cell, gate), p, sizes, T, 2, (), ((cell, gate),))


def model_cases():
    """Every case of tests/test_gpu_range_guard_loop.py: batches of at most three graphs of at most 40 vertices, T <= 3."""
    cases = [ModelCase("ordinary", model_params(40), [12, 40, 25], 3, 0, (), ())]
    shapes = [([20, 40], 2), ([40, 7, 33], 1), ([31], 3), ([12, 40, 25], 2), ([40, 40], 3), ([9, 21], 1)]
    k = 0
    for msg, layers in (("E_msg_V", (1, 2)), ("V_msg_E", (1, 2, 3, 4))):
        for layer in layers:
            cases.append(model_bias_case(msg, layer, *shapes[k % len(shapes)], seed=41 + k))
            k += 1
    for cell in ("E", "V"):
        cases.append(model_new_h_case(cell, [20, 40] if cell == "E" else [33, 8, 40], 2 if cell == "E" else 3, seed=50 + len(cell)))
    for cell, targets in (("E", (1, 2)), ("V", (1, 2, 3, 4))):
        for target in targets:
            cases.append(model_chain_case(cell, target, [17, 40] if target % 2 else [40, 5, 22], 2 + target % 2, seed=60 + target))
    for sizes in ([40, 20], [20, 40], [20, 40, 20], [20, 20]):
        cases.append(model_aggregate_case(sizes, 3, seed=5))
    k = 0
    for cell in ("E", "V"):
        for gate in ("input", "transform", "forget", "output"):
            cases.append(model_gate_case(cell, gate, *shapes[k % len(shapes)], seed=70 + k))
            k += 1
    return cases


def model_design_faults(case, sites):
    """The conditions of the module docstring on an oracle/torch_oracle.RangeSites of the case's float64 forward."""
    bad = []
    for s in MODEL_SPLIT:
        m = sites.absmax[s]
        if s in case.sites and not m >= BIG:
            bad.append("%s: largest magnitude %.4g < %.4g" % (s, m, BIG))
        if s not in case.sites and not m <= SAFE:
            bad.append("%s: largest magnitude %.4g > %.4g and not an intended site" % (s, m, SAFE))
    for cg in MODEL_GATES:
        v = sites.minvar.get(cg, float("inf"))
        if cg in case.gates and not v <= FLOOR / 4:
            bad.append("%s: smallest positive variance %.3g > floor / 4" % (cg, v))
        if cg not in case.gates and not v >= 4 * FLOOR:
            bad.append("%s: smallest positive variance %.3g < 4 floor and not an intended gate" % (cg, v))
    if case.word != int(bool(case.sites)) + 2 * int(bool(case.gates)):
        bad.append("the expected word does not follow from the sites and gates")
    return bad
