"""Every-row references of the inference forward (TEST INFRASTRUCTURE -- the package never imports this).

trajectory() runs the oracle's message passing (torch_oracle.step / step_bf16, initial_embeddings, vote_head) on whatever
device is asked for, and keeps the states, predictions and loss at the requested depths -- from the initial embeddings,
or from a given state (a teacher-forced window).  reference() adds a bar to every ROW of every state array, so that a
badly conditioned row gets its own allowance while every other row keeps the 1e-5 floor (BASELINE.json):

    bar[r] = max(1e-5 S,  2 max_col |f32 - f64|[r],  2 max over 8 draws max_col |f64(w (1 +- 2^-22)) - f64|[r])

S the largest entry of the float64 tensor; f32 the same trajectory in float32 (what fp32 arithmetic loses on that row);
the draws move every weight by 2^-22 relative, random signs (the f16x2 packing's weight precision: a kernel computes the
exact forward of a network that far off) -- the per-variable bars of tests/test_gpu_forced_gradients.py, row by row.
compare_rows() checks a device array against them and says where the worst row sits: instance, row within it, tile row.
"""
import contextlib

import numpy as np
import torch

from . import teacher_forced as TF
from . import torch_oracle as TO

FLOOR = 1e-5                # BASELINE.json's relative tolerance
SPREAD_DRAWS = 8
SPREAD_REL = 2.0 ** -22     # the f16x2 packing's weight precision
STATES = ("V.h", "V.c", "E.h", "E.c")
OUTPUTS = STATES + ("predictions", "loss")
# bf16 storage: the INFERENCE forward (GraphNN._run_bf16) folds the edge cell's adjacency product through its kernel,
# z = Zx[u] + Zx[v] + h Kh with Zx = bf16(y Kx), at every width whose message width is the cell's -- all of this network's;
# the training forward does so only at d = 64 (LayerNormBasicLSTMCell.can_fold, teacher_forced._step_fn)
INFERENCE_FOLD = True


def spread_draw(params, draw):
    """Every entry of every variable moved by 2^-22 relative, signs from a generator seeded by ``draw``."""
    rng = np.random.RandomState(104729 + draw)
    return {k: np.asarray(v, dtype=np.float64) * (1.0 + (rng.randint(0, 2, size=np.shape(v)) * 2 - 1) * SPREAD_REL)
            for k, v in params.items()}


def trajectory(params, batch, depths, dtype, device, start=None, bf16=False, fold=INFERENCE_FOLD, msg_last_relu=False):
    """The forward at each depth of ``depths`` (steps taken): {t: {"V.h", "V.c", "E.h", "E.c": state [rows, d],
    "predictions", "loss", "acc", "TP", "FP", "TN", "FN": vote head on E.h}}, tensors of ``dtype`` on ``device``, no
    autograd.  ``params``: the variables (NumPy).  ``start``: (Vh, Vc, Eh, Ec) to step from instead of the initial
    embeddings (a cell state of None is the zero state).  ``bf16``: in the build's bf16-storage semantics (step_bf16 with
    the edge cell in the inference forward's form, ``fold``; None: the training forward's, teacher_forced._step_fn); from
    the initial embeddings their h is rounded for storage, as in message_passing_bf16."""
    depths = sorted(set(int(t) for t in depths))
    tp = TO.to_torch(params, dtype, device=device)
    d = tp["V_init"].shape[1]
    step = TF._step_fn(bf16, d, fold, msg_last_relu)
    uv = torch.as_tensor(np.asarray(batch["ev_uv"]), dtype=torch.long, device=device)
    out = {}
    with torch.no_grad():
        if start is None:
            V0, E0 = TO.initial_embeddings(tp, batch)
            if bf16:
                V0, E0 = TO._rb(V0), TO._rb(E0)
            state = (V0, torch.zeros_like(V0), E0, torch.zeros_like(E0))
        else:
            w = lambda a: torch.as_tensor(a).to(device=device, dtype=dtype)
            Vh, Vc, Eh, Ec = start
            state = (w(Vh), torch.zeros_like(w(Vh)) if Vc is None else w(Vc), w(Eh), torch.zeros_like(w(Eh)) if Ec is None else w(Ec))
        for t in range(depths[-1] + 1 if depths else 0):
            if t > 0:
                state = step(tp, uv, *state)
            if t in depths:
                head = TO.vote_head(tp, batch, state[2])
                out[t] = dict(zip(STATES, state))
                out[t].update((k, head[k]) for k in ("predictions", "loss", "acc", "TP", "FP", "TN", "FN"))
    return out


def row_err(got, ref):
    """max over the columns of |got - ref| per row, in float64 ([rows]; a vector or a scalar: per entry)."""
    got = torch.as_tensor(got).to(device=ref.device, dtype=torch.float64)
    diff = (got - ref.to(torch.float64)).abs()
    return diff.amax(dim=1) if diff.dim() == 2 else diff.reshape(-1)


def bar_of(ref, err32, spread):
    """Per-row bar from the float64 tensor, the float32 run's per-row error and the draws' per-row spread: at least 1e-5 of
    the tensor's largest entry (of the smallest positive double when the tensor is all zeros: the bar stays finite)."""
    S = max(float(ref.abs().max()) if ref.numel() else 0.0, np.finfo(np.float64).tiny)
    return torch.clamp(torch.maximum(2.0 * err32, 2.0 * spread), min=FLOOR * S)


@contextlib.contextmanager
def no_tf32():
    """float32 matrix products in float32: TF32 / XF32 off inside (asserted), the previous setting restored after."""
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        assert not torch.backends.cuda.matmul.allow_tf32
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32


def reference(params, batch, depths, device, start=None, msg_last_relu=False):
    """-> (float64 trajectory, {t: {"V.h" | "V.c" | "E.h" | "E.c" | "predictions" | "loss": bar per row}}).  The float32
    run must not use TF32 / XF32 on the matrix cores (asserted).  Its index_add sums in atomic order on the GPU, so the
    float32 term moves slightly from run to run."""
    kw = dict(start=start, msg_last_relu=msg_last_relu)
    ref = trajectory(params, batch, depths, torch.float64, device, **kw)
    with no_tf32():
        f32 = trajectory(params, batch, depths, torch.float32, device, **kw)
    err32 = {t: {k: row_err(f32[t][k], ref[t][k]) for k in OUTPUTS} for t in ref}
    del f32
    spread = {t: {k: torch.zeros_like(err32[t][k]) for k in OUTPUTS} for t in ref}
    for draw in range(SPREAD_DRAWS):
        fd = trajectory(spread_draw(params, draw), batch, depths, torch.float64, device, **kw)
        for t in ref:
            for k in OUTPUTS:
                spread[t][k] = torch.maximum(spread[t][k], row_err(fd[t][k], ref[t][k]))
        del fd
    bars = {t: {k: bar_of(ref[t][k], err32[t][k], spread[t][k]) for k in OUTPUTS} for t in ref}
    return ref, bars


def _segment(counts, r):
    offs = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    i = int(np.searchsorted(offs, r, side="right") - 1)
    return i, int(r - offs[i]), offs


def compare_rows(got, ref, bar, batch, kind):
    """Every row of ``got`` (device result, NumPy or torch) against ``ref`` (float64) with per-row ``bar``.  ``kind``: "E.h",
    "E.c", "V.h", "V.c" (edge or vertex rows), "predictions" (one row per instance) or "loss".
    -> {"worst": largest err/bar (a NaN counts as infinite), "over": rows at or over their bar, "rows": rows compared,
        "array": kind, "row", "err", "bar": the worst row, its error and bar, "instance", "local": its instance and row
        within it, "tile", "tile_row": its 16-row tile and row % 16, "uv": endpoints (u, v) of an edge row, numbered
        within the instance (None for other rows)}."""
    err = row_err(got, ref)
    ratio = torch.nan_to_num(err / bar, nan=float("inf"))
    r = int(torch.argmax(ratio))
    out = {"worst": float(ratio[r]), "over": int((ratio >= 1.0).sum()), "rows": int(ratio.numel()), "array": kind,
           "row": r, "err": float(err[r]), "bar": float(bar[r]), "tile": r // 16, "tile_row": r % 16, "uv": None,
           "instance": None, "local": None}
    if kind[0] == "E":
        i, out["local"], _ = _segment(batch["n_edges"], r)
        _, _, voffs = _segment(batch["n_vertices"], 0)
        u, v = (int(x) - int(voffs[i]) for x in np.asarray(batch["ev_uv"])[r])
        out["instance"], out["uv"] = i, (u, v)
    elif kind[0] == "V":
        out["instance"], out["local"], _ = _segment(batch["n_vertices"], r)
    elif kind == "predictions":
        out["instance"], out["local"] = r, 0
    return out


def describe(res):
    """One line for a compare_rows result: where the worst row sits."""
    where = "row %d" % res["row"]
    if res["instance"] is not None and res["array"] != "predictions":
        where += " = instance %d row %d" % (res["instance"], res["local"])
        if res["uv"] is not None:
            where += " (edge %d-%d)" % res["uv"]
    elif res["array"] == "predictions":
        where = "instance %d" % res["row"]
    if res["array"] in STATES:
        where += ", tile %d row %d" % (res["tile"], res["tile_row"])
    return "%s: worst err/bar %.3f at %s (err %.2e, bar %.2e); %d of %d rows at or over the bar" % (
        res["array"], res["worst"], where, res["err"], res["bar"], res["over"], res["rows"])
