"""The training step's gradients at the benchmark's own size and depth, against TEACHER-FORCED float64 references
(oracle/teacher_forced.py): back-propagation through time of the oracle, one step at a time at the states the device
stored on its tape, computed on the GPU in torch.  Every entry of every variable is compared -- no samples -- and every row
of every stored step is checked against one oracle step from the step before: C2 (128 x n=40, d=64) at T=32, the depth
`bench.py --mode train` runs, in every GEMM arithmetic of the fp32 mode.

The end-to-end float64 anchors (test_gpu_anchors.py) stop at T=8 for the gradients: their bar must cover how much the
forward amplifies rounding over the recurrence.  A teacher-forced reference does not see that amplification -- it is the
end-to-end gradient whenever the tape is exact (tests/test_oracle.py) -- so its bars are the per-step ones."""
import time

import numpy as np
import pytest
import torch

from oracle import params as P
from oracle import teacher_forced as TF
from oracle.device_reference import SPREAD_DRAWS, spread_draw as _spread_draw

pytestmark = pytest.mark.gpu

C2_T = 32


def _batch_dict(t):
    return {"ev_uv": t[0].uv, "W": t[1], "C": t[2], "route_exists": t[3], "n_vertices": t[4], "n_edges": t[5]}


def _train_with_tape(t, params, d, T, gemm=None, bf16=False):
    """One sess.loss_and_grads on the device with the tape kept -> (gradients {name: fp64 array}, tape, loss)."""
    import tspgnn
    model = tspgnn.build_network(d, float_dtype=torch.bfloat16) if bf16 else tspgnn.build_network(d)
    if gemm is not None:
        model["gnn"].gemm = gemm
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(params)
    EV, W, C, route_exists, n_vertices, n_edges = t
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    out = sess.loss_and_grads(feed, keep_tape=True)
    torch.cuda.synchronize()
    g = {k: np.asarray(v, dtype=np.float64) for k, v in model.store.grad_dict().items()}
    return g, out["tape"], float(out["stats"][0].item())


def _norm(a):
    return float(np.sqrt((a ** 2).sum()))


@pytest.fixture
def measured():
    """Wall time and peak device memory of the test, printed; the tape and the cache are released afterwards."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("  wall %.1f s, peak device memory %.1f GB" % (time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 1e9))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "f32"])
def test_c2_gradients_at_training_depth_match_teacher_forced_float64(cuda_device, measured, gemm):
    """C2 at T=32, whole gradient of every variable.  ONE bar for every arithmetic (no arithmetic-specific slack), per
    variable, with scale = max(its largest entry, 1e-3 of the largest entry overall):
        max(1e-5 scale,
            2 x what the same teacher-forced reference loses in float32 on that variable  (fp32 arithmetic on the same
                operands: the error budget of an fp32 backward),
            2 x the largest change of the float64 reference over 8 draws of w (1 +- 2^-22), random signs  (an f16x2-packed
                weight is a 2^-22 rounding away: the kernel computes the exact gradient of a network that far off)),
    and the same bar for the variable's 2-norm.  Plus the forward: every row of every stored step within 1e-5 of the
    tensor's scale of one float64 oracle step from the stored step before."""
    from oracle.anchors import grad_anchor_inputs
    t, params, _, _ = grad_anchor_inputs("c2")
    batch = _batch_dict(t)
    g, tape, loss = _train_with_tape(t, params, 64, C2_T, gemm=gemm)
    H, C = tape.H, tape.C
    assert H["E"].dtype == torch.float32 and H["E"].shape[0] == C2_T + 1
    t0 = time.perf_counter()
    f64 = TF.forced_grads(params, batch, C2_T, H, C, bf16=False, device=cuda_device, dtype=torch.float64)
    t_f64 = time.perf_counter() - t0
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        assert not torch.backends.cuda.matmul.allow_tf32
        f32 = TF.forced_grads(params, batch, C2_T, H, C, bf16=False, device=cuda_device, dtype=torch.float32)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    spread = {k: 0.0 for k in params}
    spread_norm = {k: 0.0 for k in params}
    for draw in range(SPREAD_DRAWS):
        fd = TF.forced_grads(params, batch, C2_T, H, C, bf16=False, device=cuda_device, dtype=torch.float64,
                             weights=_spread_draw(params, draw))
        for k in params:
            spread[k] = max(spread[k], float(np.abs(fd[k] - f64[k]).max()))
            spread_norm[k] = max(spread_norm[k], abs(_norm(fd[k]) - _norm(f64[k])))
    errs = TF.forced_step_errors(params, batch, C2_T, H, C, bf16=False, device=cuda_device)
    del tape, H, C
    gscale = max(float(np.abs(v).max()) for v in f64.values())
    ratios = []
    for k in params:
        scale = max(float(np.abs(f64[k]).max()), 1e-3 * gscale)
        bar = max(1e-5 * scale, 2.0 * float(np.abs(f32[k] - f64[k]).max()), 2.0 * spread[k])
        err = float(np.abs(g[k] - f64[k]).max())
        nscale = max(_norm(f64[k]), 1e-3 * gscale)
        nbar = max(1e-5 * nscale, 2.0 * abs(_norm(f32[k]) - _norm(f64[k])), 2.0 * spread_norm[k])
        nerr = abs(_norm(g[k]) - _norm(f64[k]))
        ratios.append((err / bar, k, err / scale, bar / scale, nerr / nbar))
    ratios.sort(reverse=True)
    fwd = {k: e["max"] / e["scale"] for k, e in errs.items()}
    print("\n[C2 T=%d %s] loss %.6f; gradient vs teacher-forced float64: worst ratio to the bar %.2f (%s: %.2e against %.2e), "
          "worst norm ratio %.2f; forward rows: %s; float64 reference %.1f s"
          % (C2_T, gemm, loss, ratios[0][0], ratios[0][1], ratios[0][2], ratios[0][3], max(r[4] for r in ratios),
             "  ".join("%s %.1e" % kv for kv in fwd.items()), t_f64), end="")
    for r, k, e, b, nr in ratios:
        assert r < 1.0 and nr < 1.0, (k, "err %.3e bar %.3e (relative to scale), norm ratio %.3f" % (e, b, nr))
    for k, e in fwd.items():
        assert e < 1e-5, (k, e)


def _l2_dist(a, b):
    return float(np.sqrt(sum(((a[k] - b[k]) ** 2).sum() for k in b) / sum((b[k] ** 2).sum() for k in b)))


def _grad_report(g, ref):
    gscale = max(float(np.abs(v).max()) for v in ref.values())
    per = sorted(((float(np.abs(g[k] - ref[k]).max()) / max(float(np.abs(ref[k]).max()), 1e-2 * gscale), k) for k in ref),
                 reverse=True)
    return _l2_dist(g, ref), per


def _rows_report(errs):
    return "  ".join("%s rms %.1e max %.1e (%.1f ulp own binade, %.1f in range; %.2e of entries a whole ulp off)"
                     % (k, np.sqrt(e["sumsq"] / e["n"]) / e["scale"], e["max"] / e["scale"], e["ulps"], e["ulps_top"],
                        e["whole"] / e["n"]) for k, e in errs.items())


@pytest.mark.parametrize("T", [8, 64])
def test_config5_bf16_gradients_match_teacher_forced_float64(cuda_device, measured, T):
    """The config-5 shard in the bf16-storage mode (M = 636 800 edge rows, d=128) at T=8 and at T=64 -- what
    `bench.py --workload c5 --mode train` runs -- against the teacher-forced bf16 reference in float64, with the bars
    test_gpu_model.py::test_bf16_storage_training_gradients sets and explains (L2 < 3e-3, worst variable < 8e-3 relative to
    max(its largest entry, 1e-2 of the largest overall)), and every stored row of every step against one bf16 oracle step:
        h and c: rms below 0.1 bf16 ulp (2^-8) of the tensor's largest entry;  h (bf16): no entry more than 2 ulps of its own
        binade off;  c (fp32, from bf16-rounded aggregates): no entry more than 2^-7 of the tensor's scale off.
    Two references.  The plain one re-rounds every bf16 intermediate itself (the bars above apply to the gradient, the rms and
    c bars to the rows).  The pinned one takes the device's stored intermediates (message MLP activations, both aggregates:
    bf16_tape_intermediates); against it every bar applies.  At d = 128 the build does NOT fold the edge cell's adjacency
    product through its kernel (LayerNormBasicLSTMCell.can_fold: d = 64 only), so its E<-V aggregate is rounded to bf16
    before the GEMM: the oracle step follows it (teacher_forced._step_fn).  With the folded form instead -- the oracle's
    default -- the plain reference rounded Zx = y Kx where the device rounds y[u] + y[v], and 10 % of the edge h entries
    landed a whole ulp away (L2 3.0e-3, worst 9.4e-3).  The 2-ulp bar on h counts the entries in bf16's range of the step
    (at least 2^-8 of its largest); below that an entry's own ulp is smaller than the fp32 error of the cell state it comes
    from, and the entry is held to 2 ulps of the tensor's scale."""
    from oracle.anchors import bf16_anchor_inputs
    t, _, d, _, _ = bf16_anchor_inputs("c5shard")
    params = P.init_params(d, seed=3, perturb=True)
    batch = _batch_dict(t)
    t0 = time.perf_counter()
    g, tape, loss = _train_with_tape(t, params, d, T, bf16=True)
    t_dev = time.perf_counter() - t0
    H, C = tape.H, tape.C
    assert H["E"].dtype == torch.bfloat16 and C["E"].dtype == torch.float32 and tuple(H["E"].shape) == (T + 1, 636800, d)
    assert tuple(tape.acts[("V", 0)].shape) == (3, T, 636800, d) and tuple(tape.acts[("E", 0)].shape) == (3, T, 6400, d)
    tape_gb = sum(x.numel() * x.element_size() for x in list(H.values()) + list(C.values()) + list(tape.X.values())
                  + list(tape.ZX.values()) + list(tape.acts.values())) / 1e9
    stored = TF.bf16_tape_intermediates(tape)
    t0 = time.perf_counter()
    pinned = TF.forced_grads(params, batch, T, H, C, bf16=True, device=cuda_device, dtype=torch.float64, stored=stored)
    t_ref = time.perf_counter() - t0
    rows = TF.forced_step_errors(params, batch, T, H, C, bf16=True, device=cuda_device, stored=stored)
    rerounded = TF.forced_grads(params, batch, T, H, C, bf16=True, device=cuda_device, dtype=torch.float64)
    rows_rr = TF.forced_step_errors(params, batch, T, H, C, bf16=True, device=cuda_device)
    del tape, H, C, stored
    l2, per = _grad_report(g, pinned)
    l2_rr, per_rr = _grad_report(g, rerounded)
    print("\n[config-5 shard bf16 T=%d] loss %.6f; gradient vs teacher-forced float64: L2 %.2e, worst variable %.2e (%s; next %s); "
          "forward rows: %s\n  re-rounded reference: L2 %.2e, worst %.2e (%s; next %s); rows: %s\n  device step %.1f s (tape %.1f GB), "
          "reference %.1f s"
          % (T, loss, l2, per[0][0], per[0][1], ", ".join("%s %.1e" % (k, r) for r, k in per[1:4]), _rows_report(rows),
             l2_rr, per_rr[0][0], per_rr[0][1], ", ".join("%s %.1e" % (k, r) for r, k in per_rr[1:4]), _rows_report(rows_rr),
             t_dev, tape_gb, t_ref), end="")
    assert l2_rr < 3e-3 and per_rr[0][0] < 8e-3, per_rr[:5]
    assert l2 < 3e-3 and per[0][0] < 8e-3, per[:5]
    for name, errs in (("pinned", rows), ("re-rounded", rows_rr)):
        for k, e in errs.items():
            assert np.sqrt(e["sumsq"] / e["n"]) / e["scale"] < 0.1 * 2.0 ** -8, (name, k, e)
            if k.endswith(".c"):
                assert e["max"] / e["scale"] < 2.0 ** -7, (name, k, e)
    for k in ("V.h", "E.h"):
        assert rows[k]["ulps_top"] <= 2.0 and rows[k]["max"] / rows[k]["scale"] <= 2 * 2.0 ** -8, (k, rows[k])
