"""float64 restatement of the route head (build_network(d, route_head=True)) on top of the oracle: TEST INFRASTRUCTURE.

The oracle (oracle/torch_oracle.py) is imported, not copied: its forward gives the final edge states and the decision loss;
this module adds E_route = mlp(last E.h, params, "E_route"), the weighted per-edge cross entropy

    route_loss = (1/B) sum_p (1/m_p) sum_{e in p} w_e sce(x_e, y_e),   w_e = 1 (y = 0) | pos_weight (y = 1),
    pos_weight None: w_e = (m_p - k_p) / max(k_p, 1) on the k_p marked edges of problem p,

the edge statistics at threshold logit > 0, and torch-autograd gradients of loss + lam * route_loss + L2.
"""
from collections import OrderedDict

import numpy as np
import torch

from oracle import params as P
from oracle import torch_oracle as TO
from oracle.torch_oracle import L2NORM_SCALING, forward, mlp, sigmoid_cross_entropy_with_logits


def route_params(d, seed=0, perturb=True):
    """The oracle's parameters (oracle.params.init_params) plus E_route/*: E_vote's shapes, xavier kernels, and -- with
    ``perturb`` -- random biases instead of the zeros they start from; every value a float32."""
    params = P.init_params(d, seed=seed, perturb=perturb)
    rng = np.random.RandomState(seed + 7919)
    for i, (a, b) in enumerate(P.mlp_layer_sizes(d)["E_vote"]):
        lim = np.sqrt(6.0 / (a + b))
        params["E_route_MLP_layer_%d/kernel" % (i + 1)] = rng.uniform(-lim, lim, size=(a, b)).astype(np.float32).astype(np.float64)
        bias = 0.1 * rng.randn(b) if perturb else np.zeros(b)
        params["E_route_MLP_layer_%d/bias" % (i + 1)] = bias.astype(np.float32).astype(np.float64)
    return params


def segments(n_edges):
    return np.concatenate([[0], np.cumsum(np.asarray(n_edges).astype(np.int64))])


def edge_weights(marks, n_edges, pos_weight):
    """w_e of the loss above as a float64 array (marks: 0 / 1 per edge)."""
    y = np.asarray(marks, dtype=np.float64)
    w = np.ones_like(y)
    seg = segments(n_edges)
    for p in range(len(seg) - 1):
        s = slice(seg[p], seg[p + 1])
        k, m = y[s].sum(), seg[p + 1] - seg[p]
        pw = (m - k) / max(k, 1.0) if pos_weight is None else float(pos_weight)
        w[s] = np.where(y[s] != 0, pw, 1.0)
    return w


def edge_bce(logits, marks, n_edges, pos_weight, scale=1.0):
    """float64 (stats[6], dlogit) of tspgnn_edge_bce_f32: route loss, mean per-problem edge accuracy, TP, FP, TN, FN at
    logit > 0, and scale * w_e (sigmoid(x_e) - y_e) / (B m_p)."""
    x, y = np.asarray(logits, dtype=np.float64), np.asarray(marks, dtype=np.float64)
    w, seg = edge_weights(y, n_edges, pos_weight), segments(n_edges)
    B = len(seg) - 1
    term = w * (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x))))
    yes, on = x > 0, y != 0
    loss = acc = 0.0
    dlogit = np.zeros_like(x)
    for p in range(B):
        s = slice(seg[p], seg[p + 1])
        m = seg[p + 1] - seg[p]
        if m == 0:
            continue
        loss += term[s].sum() / m
        acc += (yes[s] == on[s]).sum() / m
        dlogit[s] = scale * w[s] * (1.0 / (1.0 + np.exp(-x[s])) - y[s]) / (B * m)
    stats = np.array([loss / B, acc / B, (yes & on).sum(), (yes & ~on).sum(), (~yes & ~on).sum(), (~yes & on).sum()],
                     dtype=np.float64)
    return stats, dlogit


def route_loss_torch(E_route, marks, n_edges, pos_weight):
    y = torch.as_tensor(np.asarray(marks, dtype=np.float64), dtype=E_route.dtype)
    w = torch.as_tensor(edge_weights(marks, n_edges, pos_weight), dtype=E_route.dtype)
    term = w * sigmoid_cross_entropy_with_logits(E_route, y)
    seg = segments(n_edges)
    return torch.stack([term[seg[p]:seg[p + 1]].mean() for p in range(len(seg) - 1)]).mean()


def loss_and_grads(params_np, batch, marks, time_steps, lam=1.0, pos_weight=None, dtype=torch.float64, bf16=False,
                   fold=True, dense=False):
    """-> (out, grads): out the oracle's forward outputs plus "E_route" and "route_loss"; grads the autograd gradients of
    loss + lam * route_loss + 1e-10 * sum l2_loss(var) over every variable, E_route/* included (name -> float64 array).
    ``bf16``: through the oracle's bf16-storage forward, as oracle.torch_oracle.loss_and_grads(bf16=True); ``dense``: the
    adjacency products by the dense matrix, op for op (the fp32 error budget of tests/test_gpu_model.py)."""
    params = TO.to_torch(params_np, dtype=dtype, requires_grad=True)
    out = forward(params, batch, time_steps, dense=dense, bf16=bf16, fold=fold)
    out["E_route"] = mlp(out["last_states"]["E"][0], params, "E_route").reshape(-1)
    out["route_loss"] = route_loss_torch(out["E_route"], marks, batch["n_edges"], pos_weight)
    l2 = sum((p ** 2).sum() / 2 for p in params.values())
    total = out["loss"] + lam * out["route_loss"] + L2NORM_SCALING * l2
    grads = torch.autograd.grad(total, list(params.values()))
    return out, OrderedDict((k, g.detach().numpy().copy()) for k, g in zip(params.keys(), grads))


# ------------------------------------------------------------------------------------------------ the launch-name fixture
# tests/golden/route_head_launch_names.json: the library calls, by name, of Session.forward_device and
# Session.loss_and_grads as the code stood BEFORE the route head existed, recorded with tests/test_launch_trace.recording on
# the batch below (d = 32 and 64, T = 3, the one-launch loop off as in that test).  A network built without the head must
# still make exactly these.
LAUNCH_SIZES, LAUNCH_T = (5, 6, 8, 12), 3


def launch_case(d, device, route_head=False):
    """(model, session, resident batch, its instances) of the fixture's case."""
    import tspgnn
    rng = np.random.RandomState(3)
    instances = [tspgnn.random_instance(n, rng) for n in LAUNCH_SIZES]
    model = tspgnn.build_network(d, store=tspgnn.VariableStore(), route_head=route_head)
    sess = tspgnn.Session(model, device=device)
    sess.run(tspgnn.global_variables_initializer())
    model["gnn"].persistent_loop = False
    t = tspgnn.InstanceLoader.create_batch(instances)
    feed = {model[k]: v for k, v in zip(("EV", "W", "C", "route_exists", "n_vertices", "n_edges"), t)}
    feed[model["time_steps"]] = LAUNCH_T
    if route_head:
        feed[model["route_edges"]] = tspgnn.route_edge_marks_host(instances)[0]
    return model, sess, sess.prepare(feed), instances


def launch_names(trace):
    return [c[0] if isinstance(c, list) else c["multi"] for c in trace]
