"""CPU restatement of the TSP-GNN hot path in torch (TEST INFRASTRUCTURE -- see oracle/__init__.py).

PARITY UNPINNED: the reference's arithmetic lives in TensorFlow 1.x (tf.contrib), which
is neither vendored nor installable here and the reference holds no
golden vectors for this path (O5).  What this file restates, line by line:

* Mlp.__call__                      /root/reference/mlp.py:57-63
* GraphNN.__call__ / while_body      /root/reference/graphnn.py:134-179
* build_network pre-loop             /root/reference/model.py:33-51
* build_network post-loop            /root/reference/model.py:107-157
* L2 / clip / Adam                   /root/reference/model.py:160-167
* tf.contrib.rnn.LayerNormBasicLSTMCell, tf.contrib.layers.layer_norm, tf.layers.Dense,
  tf.nn.sigmoid_cross_entropy_with_logits, tf.clip_by_global_norm, tf.train.AdamOptimizer:
  restated from the published TF-1.x semantics.

Two variants of the adjacency product (graphnn.py:156-160):
``dense=True``  multiplies by the dense block-diagonal EV[M,N] exactly like tf.matmul does
                (op-for-op; this is what ``bench.py``'s cpu_baseline times), and
``dense=False`` uses the endpoint list (index_add / gather) -- same mathematics, no zeros.
Gradients come from torch autograd on this restatement (float64 for the oracle).
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import params as P

LN_EPS = 1e-12  # tf.contrib.layers.layer_norm: variance_epsilon = 1e-12
FORGET_BIAS = 1.0  # LayerNormBasicLSTMCell default
LEARNING_RATE = 2e-5  # model.py:13
L2NORM_SCALING = 1e-10  # model.py:14
CLIP_NORM = 0.65  # model.py:15
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8  # tf.train.AdamOptimizer defaults


def to_torch(params, dtype=torch.float64, requires_grad=False, device=None):
    out = OrderedDict()
    for k, v in params.items():
        t = torch.tensor(np.asarray(v), dtype=dtype, device=device)
        t.requires_grad_(requires_grad)
        out[k] = t
    return out


class RangeSites(object):
    """Optional collector for mlp, lnlstm_cell, step, message_passing and forward (their ``sites`` argument; None, the
    default, records nothing and changes nothing): what the f16x2 range guard of the build looks at, in the oracle's own
    precision.  absmax[site]: the largest magnitude of a GEMM operand -- "<prefix>_MLP_layer_<l>" the input of that
    Dense layer, "<cell>_cell/x" and "<cell>_cell/h" the two halves of a cell's operand, "<cell>_cell/x_pushed" the row-sum
    of the sending MLP's LAST HIDDEN activation (the operand of the build's pushed form, z = rowsum(a) (W Kx) + degree (b Kx)
    + h Kh), "<prefix>_out" the output of a message MLP (the operand of the projection through the receiving cell's Kx).
    minvar[(cell, gate)]: the smallest positive variance (layer_norm's, biased) of a row of that gate's z; gate in
    "input", "transform", "forget", "output".  Both over every call since the collector was made."""

    def __init__(self):
        self.absmax, self.minvar, self.last = {}, {}, {}

    def operand(self, site, x):
        self.last[site] = x
        if x.numel():
            self.absmax[site] = max(self.absmax.get(site, 0.0), float(x.detach().abs().max()))

    def gates(self, cell, z):
        for name, zg in zip(("input", "transform", "forget", "output"), torch.chunk(z.detach(), 4, dim=1)):
            var = ((zg - zg.mean(dim=-1, keepdim=True)) ** 2).mean(dim=-1)
            var = var[var > 0]
            if var.numel():
                self.minvar[(cell, name)] = min(self.minvar.get((cell, name), float("inf")), float(var.min()))


def mlp(x, params, prefix, n_layers=4, last_activation=False, sites=None):
    """mlp.py:57-63 with activations [relu]*3 + [None] (graphnn.py:116-119, model.py:34-37)."""
    for i in range(n_layers):
        if sites is not None:
            sites.operand("%s_MLP_layer_%d" % (prefix, i + 1), x)
        W = params["%s_MLP_layer_%d/kernel" % (prefix, i + 1)]
        b = params["%s_MLP_layer_%d/bias" % (prefix, i + 1)]
        x = x @ W + b  # tf.layers.Dense: x @ kernel + bias, kernel[in,out]
        if i < n_layers - 1 or last_activation:
            x = torch.relu(x)
    return x


def layer_norm(x, gamma, beta):
    """tf.contrib.layers.layer_norm over the last axis: nn.moments (biased variance) +
    nn.batch_normalization evaluated as x*inv + (beta - mean*inv), inv = rsqrt(var+eps)*gamma."""
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    inv = torch.rsqrt(var + LN_EPS) * gamma
    return x * inv + (beta - mean * inv)


def lnlstm_cell(x, h, c, params, cell, activation=torch.relu, base=None, sites=None):
    """tf.contrib.rnn.LayerNormBasicLSTMCell.call with activation=relu (graphnn.py:110,168-170).
    args = concat([inputs, h]); no bias; gates i,j,f,o; forget bias added after LN;
    the *normalised* new_c is both stored and fed to the output.
    ``activation`` (the cell's own constructor argument; the hot path always passes relu) exists so that the
    cell can be checked against the one vector TensorFlow itself publishes for it, which uses the default tanh
    (tests/test_oracle.py::test_lnlstm_cell_reproduces_tensorflow_unit_test_constants)."""
    base = base if base is not None else "TSP/%s_cell/layer_norm_basic_lstm_cell" % cell
    z = torch.cat([x, h], dim=1) @ params[base + "/kernel"]
    if sites is not None:
        sites.operand("%s_cell/x" % cell, x)
        sites.operand("%s_cell/h" % cell, h)
        sites.gates(cell, z)
    i, j, f, o = torch.chunk(z, 4, dim=1)
    i = layer_norm(i, params[base + "/input/gamma"], params[base + "/input/beta"])
    j = layer_norm(j, params[base + "/transform/gamma"], params[base + "/transform/beta"])
    f = layer_norm(f, params[base + "/forget/gamma"], params[base + "/forget/beta"])
    o = layer_norm(o, params[base + "/output/gamma"], params[base + "/output/beta"])
    g = activation(j)
    new_c = c * torch.sigmoid(f + FORGET_BIAS) + torch.sigmoid(i) * g
    new_c = layer_norm(new_c, params[base + "/state/gamma"], params[base + "/state/beta"])
    new_h = activation(new_c) * torch.sigmoid(o)
    return new_h, new_c


def dense_ev(ev_uv, n_total, dtype):
    """The block-diagonal dense EV[M,N] of instance_loader.py:45,63-66 (exactly two ones per row)."""
    M = ev_uv.shape[0]
    EV = torch.zeros((M, n_total), dtype=dtype)
    idx = torch.arange(M)
    uv = torch.as_tensor(np.asarray(ev_uv), dtype=torch.long)
    EV[idx, uv[:, 0]] = 1
    EV[idx, uv[:, 1]] = 1
    return EV


def msg_layers(params, msg="V_msg_E"):
    """Dense layers of the message MLP ``msg``, counted from the variables' names (GraphNN's MLP_depth + 1)."""
    n = 0
    while "TSP/%s_MLP_layer_%d/kernel" % (msg, n + 1) in params:
        n += 1
    return n


def message_passing(params, ev_uv, V0, E0, time_steps, dense=False, EV=None, trace=None, msg_last_relu=False, sites=None):
    """GraphNN.__call__ for the TSP wiring (graphnn.py:134-179, model.py:57-94): ``time_steps`` iterations of ``step``.
    ``msg_last_relu``: GraphNN's Msg_last_activation is relu (graphnn.py:119), not the default None."""
    N = V0.shape[0]
    uv = torch.as_tensor(np.asarray(ev_uv), dtype=torch.long, device=V0.device)
    if dense and EV is None:
        EV = dense_ev(ev_uv, N, V0.dtype).to(V0.device)
    Vh, Vc = V0, torch.zeros_like(V0)  # graphnn.py:135-138
    Eh, Ec = E0, torch.zeros_like(E0)
    for t in range(int(time_steps)):
        Vh, Vc, Eh, Ec = step(params, uv, Vh, Vc, Eh, Ec, EV=EV if dense else None, msg_last_relu=msg_last_relu, sites=sites)
        if trace is not None:
            trace.append((Vh.detach().clone(), Eh.detach().clone()))
    return {"V": (Vh, Vc), "E": (Eh, Ec)}


def step(params, uv, Vh, Vc, Eh, Ec, EV=None, msg_last_relu=False, sites=None):
    """One message-passing step of message_passing (graphnn.py:143-170): -> the next (Vh, Vc, Eh, Ec).  Both updates
    read the *old* states (new_states is a fresh dict, graphnn.py:143).  uv: long tensor [M,2]; EV given: the
    adjacency products by the dense block-diagonal matrix (tf.matmul op for op) instead of index_add / gather.
    The message MLPs have as many layers as ``params`` names (msg_layers); ``msg_last_relu``: relu on their last one."""
    # V <- LSTM_V( EV^T x E_msg_V(E.h) )
    y = mlp(Eh, params, "TSP/E_msg_V", msg_layers(params, "E_msg_V"), msg_last_relu, sites=sites)
    if EV is not None:
        vagg = EV.t() @ y  # tf.matmul(..., adjoint_a=True)
    else:
        vagg = torch.zeros_like(Vh).index_add(0, uv[:, 0], y).index_add(0, uv[:, 1], y)
    # E <- LSTM_E( EV x V_msg_E(V.h) )
    y2 = mlp(Vh, params, "TSP/V_msg_E", msg_layers(params, "V_msg_E"), msg_last_relu, sites=sites)
    if sites is not None:
        a = sites.last["TSP/E_msg_V_MLP_layer_%d" % msg_layers(params, "E_msg_V")]      # the last hidden activation
        sites.operand("V_cell/x_pushed", torch.zeros((Vh.shape[0], a.shape[1]), dtype=a.dtype, device=a.device)
                      .index_add(0, uv[:, 0], a).index_add(0, uv[:, 1], a))
        sites.operand("TSP/E_msg_V_out", y)
        sites.operand("TSP/V_msg_E_out", y2)
    if EV is not None:
        eagg = EV @ y2
    else:
        eagg = y2[uv[:, 0]] + y2[uv[:, 1]]
    nVh, nVc = lnlstm_cell(vagg, Vh, Vc, params, "V", sites=sites)
    nEh, nEc = lnlstm_cell(eagg, Eh, Ec, params, "E", sites=sites)
    return nVh, nVc, nEh, nEc


def _rb(x):
    """Round to bf16 (nearest even) and return in the original dtype.  Straight-through for autograd: the gradient
    passes unchanged and in the working precision (a plain .to(bfloat16) round trip would also round the gradient
    flowing back through it) -- the mixed-precision convention the build's bf16 training follows."""
    return x + (x.to(torch.bfloat16).to(x.dtype) - x).detach()


def message_passing_bf16(params, ev_uv, V0, E0, time_steps, fold=True, msg_last_relu=False):
    """The build's bf16-storage mode (BASELINE config 5: "bf16 embeddings with fp32 accumulate"; the reference has
    no reduced-precision path, this restates where tsp-gnn_amd rounds): embeddings h, every stored MLP activation,
    the V<-E aggregate and the projected vertex messages Zx = V_msg_E(V.h) Kx are rounded to bf16, GEMM weights are
    the variables rounded to bf16, sums accumulate in the working precision; the cell state c, LayerNorm, biases
    and gates are not rounded.  The edge cell is evaluated in the folded form (EV y) Kx = EV (y Kx) (``fold``: see step_bf16)."""
    uv = torch.as_tensor(np.asarray(ev_uv), dtype=torch.long, device=V0.device)
    Vh, Vc = _rb(V0), torch.zeros_like(V0)
    Eh, Ec = _rb(E0), torch.zeros_like(E0)
    for t in range(int(time_steps)):
        Vh, Vc, Eh, Ec = step_bf16(params, uv, Vh, Vc, Eh, Ec, fold=fold, msg_last_relu=msg_last_relu)
    return {"V": (Vh, Vc), "E": (Eh, Ec)}


def step_bf16(params, uv, Vh, Vc, Eh, Ec, stored=None, fold=True, msg_last_relu=False):
    """One message-passing step of message_passing_bf16 on stored (bf16-valued) h and fp32-class c: -> the next
    (Vh, Vc, Eh, Ec), h rounded for storage.  uv: long tensor [M,2].
    ``fold``: the edge cell's input in the folded form, z = Zx[u] + Zx[v] + h Kh with Zx = bf16(y Kx) -- what the build runs
    at d = 64 (LayerNormBasicLSTMCell.can_fold) --, or (False) op for op, z = [bf16(y[u] + y[v]) | h] K -- what it runs at
    the other widths: the two round at different points.
    ``stored`` (optional): values a device stored for this step's bf16-rounded intermediates, used IN PLACE of the
    oracle's own rounding (straight through, like it): "E_msg_V" / "V_msg_E" the hidden activations of the message MLPs
    [layers - 1 or more, rows, d], "vagg" the V<-E aggregate [N, d], "y2" the vertex messages [N, d], "zx" the projected
    messages [N, 4d].
    The message MLPs have as many layers as ``params`` names (msg_layers); ``msg_last_relu``: relu on their last one."""
    d = Vh.shape[1]
    stored = stored or {}

    def pin(x, s):
        return _rb(x) if s is None else x + (s.to(x.dtype) - x).detach()

    def mlp_b(x, prefix, acts=None, out=None):
        n = msg_layers(params, prefix[len("TSP/"):])
        for i in range(n):
            W = _rb(params["%s_MLP_layer_%d/kernel" % (prefix, i + 1)])
            x = x @ W + params["%s_MLP_layer_%d/bias" % (prefix, i + 1)]
            if i < n - 1:
                x = pin(torch.relu(x), None if acts is None else acts[i])
            else:
                x = pin(torch.relu(x) if msg_last_relu else x, out)
        return x

    def cell_b(z, c, cell):
        base = "TSP/%s_cell/layer_norm_basic_lstm_cell" % cell
        i, j, f, o = torch.chunk(z, 4, dim=1)
        i = layer_norm(i, params[base + "/input/gamma"], params[base + "/input/beta"])
        j = layer_norm(j, params[base + "/transform/gamma"], params[base + "/transform/beta"])
        f = layer_norm(f, params[base + "/forget/gamma"], params[base + "/forget/beta"])
        o = layer_norm(o, params[base + "/output/gamma"], params[base + "/output/beta"])
        new_c = c * torch.sigmoid(f + FORGET_BIAS) + torch.sigmoid(i) * torch.relu(j)
        new_c = layer_norm(new_c, params[base + "/state/gamma"], params[base + "/state/beta"])
        return _rb(torch.relu(new_c) * torch.sigmoid(o)), new_c
    KV = _rb(params["TSP/V_cell/layer_norm_basic_lstm_cell/kernel"])
    KE = _rb(params["TSP/E_cell/layer_norm_basic_lstm_cell/kernel"])
    y = mlp_b(Eh, "TSP/E_msg_V", acts=stored.get("E_msg_V"))
    vagg = pin(torch.zeros_like(Vh).index_add(0, uv[:, 0], y).index_add(0, uv[:, 1], y), stored.get("vagg"))
    y2 = mlp_b(Vh, "TSP/V_msg_E", acts=stored.get("V_msg_E"), out=stored.get("y2"))
    nVh, nVc = cell_b(torch.cat([vagg, Vh], dim=1) @ KV, Vc, "V")
    if fold:
        zx = pin(y2 @ KE[:d], stored.get("zx"))
        nEh, nEc = cell_b(zx[uv[:, 0]] + zx[uv[:, 1]] + Eh @ KE[d:], Ec, "E")
    else:
        eagg = pin(y2[uv[:, 0]] + y2[uv[:, 1]], stored.get("eagg"))
        nEh, nEc = cell_b(torch.cat([eagg, Eh], dim=1) @ KE, Ec, "E")
    return nVh, nVc, nEh, nEc


def forward(params, batch, time_steps, dense=False, trace=None, bf16=False, fold=True, msg_last_relu=False, sites=None):
    """build_network forward (model.py:18-157) on a packed batch.

    batch: dict with ev_uv int[M,2], W[M], C[M], route_exists[B], n_vertices[B], n_edges[B].
    bf16=True: the message passing in the build's bf16-storage mode (message_passing_bf16).
    """
    V0, E0 = initial_embeddings(params, batch)
    if bf16:
        last = message_passing_bf16(params, batch["ev_uv"], V0, E0, time_steps, fold=fold, msg_last_relu=msg_last_relu)
    else:
        last = message_passing(params, batch["ev_uv"], V0, E0, time_steps, dense=dense, trace=trace,
                               msg_last_relu=msg_last_relu, sites=sites)
    out = vote_head(params, batch, last["E"][0], sites=sites)
    out["last_states"] = last
    return out


def initial_embeddings(params, batch):
    """(V0, E0) of model.py:33-51: V_init / sqrt(d) tiled over the vertices, E_init_MLP([W, C])."""
    some = params["V_init"]
    dtype = some.dtype
    d = some.shape[1]
    W = torch.as_tensor(np.asarray(batch["W"]), dtype=dtype, device=some.device).reshape(-1, 1)
    C = torch.as_tensor(np.asarray(batch["C"]), dtype=dtype, device=some.device).reshape(-1, 1)
    N = int(np.asarray(batch["n_vertices"]).astype(np.int64).sum())
    # model.py:43
    E0 = mlp(torch.cat([W, C], dim=1), params, "E_init_MLP")
    # model.py:48-51
    V0 = (params["V_init"] / math.sqrt(float(d))).repeat(N, 1)
    return V0, E0


def vote_head(params, batch, E_n, sites=None):
    """model.py:107-157 from the final edge embeddings: votes, per-problem mean, predictions, metrics, loss."""
    dtype = E_n.dtype
    labels = torch.as_tensor(np.asarray(batch["route_exists"]), dtype=dtype, device=E_n.device)
    n_edges = np.asarray(batch["n_edges"]).astype(np.int64)
    # model.py:128
    E_vote = mlp(E_n, params, "E_vote", sites=sites).reshape(-1)
    # model.py:134-145: mean of each problem's edge-vote segment
    offs = np.concatenate([[0], np.cumsum(n_edges)])
    logits = torch.stack([E_vote[offs[i]:offs[i + 1]].mean() for i in range(len(n_edges))])
    pred = torch.sigmoid(logits)
    # tf.round = half-to-even; torch.round too
    rp = torch.round(pred)
    eq = (labels == rp).to(dtype)
    ne = (labels != rp).to(dtype)
    out = {
        "E_vote": E_vote,
        "logits": logits,
        "predictions": pred,
        # formulas kept verbatim, including the FP/FN mislabelling (model.py:150-153)
        "TP": (labels * eq).sum(),
        "FP": (labels * ne).sum(),
        "TN": ((1 - labels) * eq).sum(),
        "FN": ((1 - labels) * ne).sum(),
        "acc": eq.mean(),
    }
    out["loss"] = sigmoid_cross_entropy_with_logits(logits, labels).mean()
    return out


def sigmoid_cross_entropy_with_logits(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits (model.py:147): z * -log(sigmoid(x)) + (1 - z) * -log(1 - sigmoid(x)) in the
    form TensorFlow documents and evaluates, max(x, 0) - x * z + log(1 + exp(-|x|))."""
    return torch.clamp(x, min=0) - x * z + torch.log1p(torch.exp(-x.abs()))


def loss_and_grads(params_np, batch, time_steps, dtype=torch.float64, dense=False, bf16=False, fold=True,
                   msg_last_relu=False):
    """tf.gradients(loss + 1e-10 * sum l2_loss(var)) (model.py:163-166), unclipped.  bf16=True: of the bf16-storage
    forward (message_passing_bf16), roundings passed straight through, gradients w.r.t. the unrounded variables."""
    params = to_torch(params_np, dtype=dtype, requires_grad=True)
    out = forward(params, batch, time_steps, dense=dense, bf16=bf16, fold=fold, msg_last_relu=msg_last_relu)
    vars_cost = sum((p ** 2).sum() / 2 for p in params.values())
    total = out["loss"] + L2NORM_SCALING * vars_cost
    grads = torch.autograd.grad(total, list(params.values()))
    g = OrderedDict((k, gi.detach().numpy().copy()) for k, gi in zip(params.keys(), grads))
    return out, g


def clip_by_global_norm(grads, clip_norm=CLIP_NORM):
    """tf.clip_by_global_norm: g * clip / max(global_norm, clip)."""
    gn = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values()))
    scale = clip_norm / max(gn, clip_norm)
    return OrderedDict((k, g * scale) for k, g in grads.items()), gn


def adam_step(params, grads, m, v, step, lr=LEARNING_RATE):
    """tf.train.AdamOptimizer._apply_dense: lr_t = lr*sqrt(1-b2^t)/(1-b1^t);
    m,v EMA; p -= lr_t * m / (sqrt(v) + eps).  ``step`` is 1-based."""
    lr_t = lr * math.sqrt(1 - ADAM_B2 ** step) / (1 - ADAM_B1 ** step)
    new_p, new_m, new_v = OrderedDict(), OrderedDict(), OrderedDict()
    for k in params:
        g = grads[k]
        new_m[k] = ADAM_B1 * m[k] + (1 - ADAM_B1) * g
        new_v[k] = ADAM_B2 * v[k] + (1 - ADAM_B2) * g * g
        new_p[k] = params[k] - lr_t * new_m[k] / (np.sqrt(new_v[k]) + ADAM_EPS)
    return new_p, new_m, new_v


def train_step(params_np, batch, time_steps, m, v, step, dtype=torch.float64):
    """One ``sess.run(train_step)`` (model.py:160-167)."""
    out, g = loss_and_grads(params_np, batch, time_steps, dtype=dtype)
    g, gn = clip_by_global_norm(g)
    p, m, v = adam_step(params_np, g, m, v, step)
    return out, p, m, v, gn


def time_dense_forward(d, batch, time_steps, threads, warm=1, iters=1, seed=0):
    """cpu_baseline leg of bench.py: fp32, dense EV matmuls both directions, unfused Dense
    layers and LayerNorm-LSTM -- the FLOPs and memory traffic of the TF CPU graph
    (SURVEY.md §8d M5).  Returns (median seconds per forward, threads used)."""
    import time

    torch.set_num_threads(int(threads))
    params = to_torch(P.init_params(d, seed=seed), dtype=torch.float32)
    N = int(np.asarray(batch["n_vertices"]).sum())
    EV = dense_ev(batch["ev_uv"], N, torch.float32)
    times = []
    with torch.no_grad():
        W = torch.as_tensor(np.asarray(batch["W"]), dtype=torch.float32).reshape(-1, 1)
        C = torch.as_tensor(np.asarray(batch["C"]), dtype=torch.float32).reshape(-1, 1)
        E0 = mlp(torch.cat([W, C], dim=1), params, "E_init_MLP")
        V0 = (params["V_init"] / math.sqrt(float(d))).repeat(N, 1)
        for it in range(warm + iters):
            t0 = time.perf_counter()
            message_passing(params, batch["ev_uv"], V0, E0, time_steps, dense=True, EV=EV)
            dt = time.perf_counter() - t0
            if it >= warm:
                times.append(dt)
    return float(np.median(times)), torch.get_num_threads()
