"""Teacher-forced references of the training step (TEST INFRASTRUCTURE -- the package never imports this).

A backward pass that reads a tape differentiates each message-passing step AT THE STATES THE FORWARD STORED.  The
references here do the same with the oracle: one oracle step (torch_oracle.step / step_bf16) per time step, evaluated at
the tape's (H[t], C[t]) and differentiated by autograd, the vector-Jacobian products chained from the last step back to the
initial embeddings.  Unlike the end-to-end oracle gradient -- whose own forward takes other rounding decisions, amplified over
the recurrence -- such a reference differs from the device's gradient only by the arithmetic inside one step, so its bar can
be far tighter; and when the tape is the oracle's own trajectory it IS the end-to-end gradient (tests/test_oracle.py).

H, C: {"V": [T+1, rows, d], "E": [T+1, rows, d]} -- the layout of graphnn.Tape.H / Tape.C, bf16 or fp32, on any device.  A
step is widened to ``dtype`` on ``device`` only when it is used: the peak memory is one step's graph, not the whole tape.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import torch_oracle as TO


def _step_fn(bf16, d, fold=None, msg_last_relu=False):
    """The oracle step of the semantics; bf16: with the edge cell folded exactly where the build's TRAINING forward folds it
    (d = 64, LayerNormBasicLSTMCell.can_fold), or as ``fold`` says: the two forms round at different points
    (torch_oracle.step_bf16).  The inference forward folds at every width (oracle/device_reference.INFERENCE_FOLD).
    ``msg_last_relu``: the message MLPs end in a relu (GraphNN's Msg_last_activation)."""
    if not bf16:
        return TO.step if not msg_last_relu else (lambda *a, **kw: TO.step(*a, msg_last_relu=True, **kw))
    fold = (d == 64) if fold is None else bool(fold)
    return lambda *a, **kw: TO.step_bf16(*a, fold=fold, msg_last_relu=msg_last_relu, **kw)


def _uv(batch, device):
    return torch.as_tensor(np.asarray(batch["ev_uv"]), dtype=torch.long, device=device)


def bf16_tape_intermediates(tape):
    """-> stored(t): the bf16-rounded intermediates a bf16-storage graphnn.Tape kept for step t, in the form of
    torch_oracle.step_bf16's ``stored`` -- the message MLPs' hidden activations (Tape.acts: the vertex cell's entry holds
    E_msg_V over the edges, the edge cell's V_msg_E over the vertices), the V<-E aggregate (Tape.X["V"]), the vertex
    messages (Tape.X["E"]) and the projected messages (Tape.ZX["E"], bf16 blocked by 16 rows -> row-major) of a folded edge
    cell, or the E<-V aggregate (Tape.X["E"]) of one that is not."""
    N = tape.H["V"].shape[1]

    def stored(t):
        common = {"E_msg_V": tape.acts[("V", 0)][:, t], "vagg": tape.X["V"][t], "V_msg_E": tape.acts[("E", 0)][:, t]}
        if "E" not in tape.ZX:
            return dict(common, eagg=tape.X["E"][t])
        z = tape.ZX["E"][t]
        pad, w = z.shape
        zx = z.view(pad // 16, w // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(pad, w)[:N]
        return dict(common, y2=tape.X["E"][t], zx=zx)
    return stored


def _stored_at(stored, t, device, dtype):
    if stored is None:
        return None
    return {k: v.to(device=device, dtype=dtype) for k, v in stored(t).items()}


def forced_grads(params, batch, T, H, C, *, bf16, device, dtype, weights=None, stored=None, msg_last_relu=False):
    """Back-propagation through time of the message passing (bf16=True: in the bf16-storage semantics, roundings passed
    straight through), one step at a time at the stored states H[t], C[t], then through the initial embeddings and the vote
    head.  ``params``: the variables (NumPy); ``weights`` (default: params): the values the graph is evaluated at -- e.g. a
    perturbed copy of the variables, on the same tape.  ``stored`` (bf16 only; e.g. bf16_tape_intermediates(tape)): the
    step's rounded intermediates are the device's too, not re-rounded by the oracle.
    -> {name: gradient (NumPy float64)} WITHOUT the L2 term."""
    tp = TO.to_torch(params if weights is None else weights, dtype, requires_grad=True, device=device)
    names, plist = list(params.keys()), [tp[k] for k in params]
    total = [torch.zeros_like(p) for p in plist]
    uv = _uv(batch, device)
    step = _step_fn(bf16, H["V"].shape[2], msg_last_relu=msg_last_relu)

    def leaf(a):
        return a.to(device=device, dtype=dtype).detach().requires_grad_(True)

    def vjp(scalar, leaves):
        g = torch.autograd.grad(scalar, leaves + plist, allow_unused=True)
        for k, gk in enumerate(g[len(leaves):]):
            if gk is not None:
                total[k] += gk
        return [torch.zeros_like(l) if gi is None else gi for l, gi in zip(leaves, g[:len(leaves)])]
    Eh = leaf(H["E"][T])
    dEh, = vjp(TO.vote_head(tp, batch, Eh)["loss"], [Eh])
    shape = lambda x: (x.shape[1], x.shape[2])
    dVh = torch.zeros(shape(H["V"]), dtype=dtype, device=device)
    dVc = torch.zeros(shape(C["V"]), dtype=dtype, device=device)
    dEc = torch.zeros(shape(C["E"]), dtype=dtype, device=device)
    for t in range(T - 1, -1, -1):
        leaves = [leaf(H["V"][t]), leaf(C["V"][t]), leaf(H["E"][t]), leaf(C["E"][t])]
        kw = {"stored": _stored_at(stored, t, device, dtype)} if stored is not None else {}
        nVh, nVc, nEh, nEc = step(tp, uv, *leaves, **kw)
        scalar = (nVh * dVh).sum() + (nVc * dVc).sum() + (nEh * dEh).sum() + (nEc * dEc).sum()
        del nVh, nVc, nEh, nEc
        dVh, dVc, dEh, dEc = vjp(scalar, leaves)
        del leaves, scalar
    V0, E0 = TO.initial_embeddings(tp, batch)      # (their rounding for storage passes the gradient through)
    vjp((V0 * dVh).sum() + (E0 * dEh).sum(), [])
    return OrderedDict((k, g.detach().to(torch.float64).cpu().numpy()) for k, g in zip(names, total))


def forced_step_errors(params, batch, T, H, C, *, bf16, device, dtype=torch.float64, stored=None, fold=None,
                       msg_last_relu=False):
    """Every row of every stored state H[t+1], C[t+1] against one oracle step from the stored (H[t], C[t]), t = 0..T-1.
    -> {"V.h" | "V.c" | "E.h" | "E.c": statistics over all rows of all steps}:
         max    largest |stored - oracle|,            sumsq  sum of the squared differences,   n  entries compared,
         scale  largest |oracle| entry,
         ulps   largest |stored - oracle| in bf16 ulps of the entry's own binade (2^(floor(log2 max(|stored|, |oracle|)) - 7)),
         whole  entries that differ by at least one such ulp,
         ulps_top  ``ulps`` over the entries at or above 2^-8 of the step's largest |oracle| entry (bf16's own range).
    ``stored``: as in forced_grads.  ``fold``: the bf16 edge cell's form (default: the training forward's, _step_fn)."""
    tp = TO.to_torch(params, dtype, device=device)
    uv = _uv(batch, device)
    step = _step_fn(bf16, H["V"].shape[2], fold, msg_last_relu)
    keys = (("V", "h"), ("V", "c"), ("E", "h"), ("E", "c"))
    acc = {"%s.%s" % k: {"max": 0.0, "sumsq": 0.0, "n": 0, "scale": 0.0, "ulps": 0.0, "whole": 0, "ulps_top": 0.0}
           for k in keys}
    w = lambda a: a.to(device=device, dtype=dtype)
    with torch.no_grad():
        for t in range(T):
            kw = {"stored": _stored_at(stored, t, device, dtype)} if stored is not None else {}
            nxt = step(tp, uv, w(H["V"][t]), w(C["V"][t]), w(H["E"][t]), w(C["E"][t]), **kw)
            for (v, part), ref in zip(keys, nxt):
                got = w((H if part == "h" else C)[v][t + 1])
                a = acc["%s.%s" % (v, part)]
                diff = (got - ref).abs()
                ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(got.abs(), ref.abs()).clamp_min(1e-30))) - 7)
                units = diff / ulp
                a["max"] = max(a["max"], float(diff.max()))
                a["sumsq"] += float((diff.to(torch.float64) ** 2).sum())
                a["n"] += diff.numel()
                a["scale"] = max(a["scale"], float(ref.abs().max()))
                a["ulps"] = max(a["ulps"], float(units.max()))
                a["whole"] += int((units >= 1).sum())
                top = ref.abs() >= 2.0 ** -8 * float(ref.abs().max())
                a["ulps_top"] = max(a["ulps_top"], float(units[top].max()) if bool(top.any()) else 0.0)
                del got, diff, ulp, units
            del nxt
    return acc


# ---------------------------------------------------------------- the bars (tests/test_gpu_forced_gradients.py)
FP32_FLOOR = 1e-5               # BASELINE.json's relative tolerance
BF16_L2 = 3e-3                  # bf16 storage: the gradient's L2 distance, relative to its L2 norm
BF16_WORST = 8e-3               # ... the worst variable's largest error, relative to max(its largest entry, 1e-2 of all)
BF16_ROW_RMS = 0.1 * 2.0 ** -8  # ... every stored row: rms of the error, relative to the tensor's largest entry
BF16_C_MAX = 2.0 ** -7          # ... the fp32 cell states: the largest error, relative to the same
BF16_H_ULPS = 2.0               # ... the bf16 h (pinned reference): ulps of the entry's own binade, in bf16's range


def _norm(a):
    return float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))


def fp32_gradient_check(g, f64, f32, draws, rows):
    """The bar of an fp32-class training backward (any GEMM arithmetic of the fp32 mode, no arithmetic-specific slack), per
    variable, with scale = max(its largest entry, 1e-3 of the largest entry overall):
        max(1e-5 scale,  2 x |f32 - f64| (what the same teacher-forced reference loses in float32 on the variable),
            2 x max over the draws |draw - f64| (the float64 reference at weights moved by 2^-22: an f16x2-packed weight is
            that far off, and the kernel computes the exact gradient of such a network)),
    the same bar for the variable's 2-norm, and every stored row within 1e-5 of its tensor's scale.
    g: the device's gradients; f64, f32: forced_grads in float64 / float32; draws: forced_grads in float64 at
    device_reference.spread_draw weights; rows: forced_step_errors.  All gradients {name: array}.
    -> {"ratios": [(err / bar, name, err / scale, bar / scale, norm err / norm bar)], worst first,
        "rows": {state: largest error / scale}, "failures": [what exceeds its bar]}."""
    gscale = max(float(np.abs(v).max()) for v in f64.values())
    ratios = []
    for k in f64:
        spread = max([float(np.abs(d[k] - f64[k]).max()) for d in draws], default=0.0)
        spread_norm = max([abs(_norm(d[k]) - _norm(f64[k])) for d in draws], default=0.0)
        scale = max(float(np.abs(f64[k]).max()), 1e-3 * gscale)
        bar = max(FP32_FLOOR * scale, 2.0 * float(np.abs(f32[k] - f64[k]).max()), 2.0 * spread)
        err = float(np.abs(g[k] - f64[k]).max())
        nscale = max(_norm(f64[k]), 1e-3 * gscale)
        nbar = max(FP32_FLOOR * nscale, 2.0 * abs(_norm(f32[k]) - _norm(f64[k])), 2.0 * spread_norm)
        nerr = abs(_norm(g[k]) - _norm(f64[k]))
        ratios.append((err / bar, k, err / scale, bar / scale, nerr / nbar))
    ratios.sort(reverse=True)
    fwd = {k: e["max"] / e["scale"] for k, e in rows.items()}
    failures = [(k, "err %.3e bar %.3e (relative to scale), norm ratio %.3f" % (e, b, nr))
                for r, k, e, b, nr in ratios if not (r < 1.0 and nr < 1.0)]
    failures += [(k, "row error %.3e of the scale" % e) for k, e in fwd.items() if not e < FP32_FLOOR]
    return {"ratios": ratios, "rows": fwd, "failures": failures}


def _l2_dist(a, b):
    return float(np.sqrt(sum(((a[k] - b[k]) ** 2).sum() for k in b) / sum((b[k] ** 2).sum() for k in b)))


def gradient_report(g, ref):
    """-> (L2 distance of g from ref relative to ref's L2 norm, [(largest error / max(largest entry, 1e-2 of the largest
    overall), name)] worst first)."""
    gscale = max(float(np.abs(v).max()) for v in ref.values())
    per = sorted(((float(np.abs(g[k] - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-2 * gscale), k) for k in ref),
                 reverse=True)
    return _l2_dist(g, ref), per


def bf16_gradient_check(g, pinned, rerounded, rows, rows_rr):
    """The bars of the bf16-storage training backward (tests/test_gpu_model.py::test_bf16_storage_training_gradients sets
    and explains them) against the teacher-forced bf16 reference, pinned (forced_grads / forced_step_errors with the tape's
    stored intermediates) and re-rounded (without):
        the gradient against either: L2 < 3e-3, worst variable < 8e-3 (gradient_report);
        every stored row against either: rms below 0.1 bf16 ulp (2^-8) of the tensor's largest entry, and the fp32 c
            no entry more than 2^-7 of that scale off;
        the bf16 h against the pinned one: no entry in bf16's range more than 2 ulps of its own binade off, none more
            than 2 ulps of the tensor's scale.
    -> {"pinned": (L2, per-variable), "rerounded": (L2, per-variable), "failures": [what exceeds its bar]}."""
    out = {"pinned": gradient_report(g, pinned), "rerounded": gradient_report(g, rerounded), "failures": []}
    for name in ("rerounded", "pinned"):
        l2, per = out[name]
        if not (l2 < BF16_L2 and per[0][0] < BF16_WORST):
            out["failures"].append((name, "gradient L2 %.2e, worst %s" % (l2, per[:5])))
    for name, errs in (("pinned", rows), ("re-rounded", rows_rr)):
        for k, e in errs.items():
            if not np.sqrt(e["sumsq"] / e["n"]) / e["scale"] < BF16_ROW_RMS:
                out["failures"].append((name, k, "row rms", e))
            if k.endswith(".c") and not e["max"] / e["scale"] < BF16_C_MAX:
                out["failures"].append((name, k, "c max", e))
    for k in ("V.h", "E.h"):
        if not (rows[k]["ulps_top"] <= BF16_H_ULPS and rows[k]["max"] / rows[k]["scale"] <= BF16_H_ULPS * 2.0 ** -8):
            out["failures"].append(("pinned", k, "h ulps", rows[k]))
    return out
