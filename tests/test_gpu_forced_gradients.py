"""The training step's gradients at the benchmark's own size and depth, against TEACHER-FORCED float64 references
(oracle/teacher_forced.py): back-propagation through time of the oracle, one step at a time at the states the device
stored on its tape, computed on the GPU in torch.  Every entry of every variable is compared -- no samples -- and every row
of every stored step is checked against one oracle step from the step before: C2 (128 x n=40, d=64) at T=32, the depth
`bench.py --mode train` runs, in every GEMM arithmetic of the fp32 mode; C4 at T=32 (two weight-gradient chunks) and T=8;
32 x n=200 (vertex degree 199); d=32 and d=128, whose backward takes other kernels (unfolded edge cell, <32> templates, the
fp32-MFMA backward at d=128); bf16 storage at config 5's shard and at d=64 (folded, native) and d=32 (widened).  Each case
asserts the path its backward took (GraphNN.last_backward).  The bars live in oracle/teacher_forced.py (fp32_gradient_check,
bf16_gradient_check) and are the same for every case of a storage mode.

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
    """One sess.loss_and_grads on the device with the tape kept -> (gradients {name: fp64 array}, tape, loss, the backward's
    path record: GraphNN.last_backward)."""
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
    return g, out["tape"], float(out["stats"][0].item()), model["gnn"].last_backward


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


def _path(rec):
    """The path record (GraphNN.last_backward) in one line."""
    flags = " ".join("%s=%s" % (f, "".join(v for v, on in sorted(rec[f].items()) if on) or "-")
                     for f in ("folded", "pushed", "fused_data", "projected"))
    return "forward %s, backward %s, %s, %d chunk(s) of %d steps" % (rec["forward"], rec["backward"], flags, rec["chunks"],
                                                                     rec["chunk_steps"])


def _assert_path(rec, expect):
    """``expect``: {"forward", "backward", "folded", "pushed", "fused_data": the variables that are, "chunks": a number,
    or (lo, None) for at least lo}: the path the selector must give the case."""
    for f in ("forward", "backward"):
        assert rec[f] == expect[f], (f, _path(rec))
    for f in ("folded", "pushed", "fused_data"):
        assert {v for v, on in rec[f].items() if on} == set(expect[f]), (f, _path(rec))
    lo = expect["chunks"][0] if isinstance(expect["chunks"], tuple) else expect["chunks"]
    assert rec["chunks"] >= lo if isinstance(expect["chunks"], tuple) else rec["chunks"] == lo, ("chunks", _path(rec))


def _fp32_case(label, t, params, d, T, gemm, device, expect=None):
    """The fp32-storage training step of one batch against the teacher-forced float64 reference: every entry of every
    variable and every stored row, under TF.fp32_gradient_check's bar (the same for every arithmetic); ``expect``: the
    path the backward must take (_assert_path)."""
    batch = _batch_dict(t)
    g, tape, loss, rec = _train_with_tape(t, params, d, T, gemm=gemm)
    H, C = tape.H, tape.C
    assert H["E"].dtype == torch.float32 and tuple(H["E"].shape) == (T + 1, t[0].shape[0], d)
    t0 = time.perf_counter()
    f64 = TF.forced_grads(params, batch, T, H, C, bf16=False, device=device, dtype=torch.float64)
    t_f64 = time.perf_counter() - t0
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        assert not torch.backends.cuda.matmul.allow_tf32
        f32 = TF.forced_grads(params, batch, T, H, C, bf16=False, device=device, dtype=torch.float32)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    draws = [TF.forced_grads(params, batch, T, H, C, bf16=False, device=device, dtype=torch.float64,
                             weights=_spread_draw(params, draw)) for draw in range(SPREAD_DRAWS)]
    errs = TF.forced_step_errors(params, batch, T, H, C, bf16=False, device=device)
    del tape, H, C
    res = TF.fp32_gradient_check(g, f64, f32, draws, errs)
    ratios = res["ratios"]
    print("\n[%s T=%d %s] loss %.6f; gradient vs teacher-forced float64: worst ratio to the bar %.2f (%s: %.2e against "
          "%.2e), worst norm ratio %.2f; forward rows: %s; float64 reference %.1f s\n  path: %s"
          % (label, T, gemm, loss, ratios[0][0], ratios[0][1], ratios[0][2], ratios[0][3], max(r[4] for r in ratios),
             "  ".join("%s %.1e" % kv for kv in res["rows"].items()), t_f64, _path(rec)), end="")
    if expect is not None:
        _assert_path(rec, expect)
    assert not res["failures"], res["failures"]


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
    tensor's scale of one float64 oracle step from the stored step before.  (TF.fp32_gradient_check)"""
    from oracle.anchors import grad_anchor_inputs
    t, params, _, _ = grad_anchor_inputs("c2")
    _fp32_case("C2", t, params, 64, C2_T, gemm, cuda_device)


# ---------------------------------------------------------------- the other widths, depths and degrees
# The backward picks its kernels by width, storage and shape: at d = 64 the edge cell is folded (can_fold) and, in f16x2, the
# vertex cell takes the message MLP's last layer (pushed) with its data gradient in the cell's launch; d = 32 runs the
# f16x2 / bf16x3 <32> templates unfolded, with no fused data gradient; d = 128 has no split-operand kernels (x3_ok) and
# runs the fp32-MFMA forward and backward whatever the arithmetic asked for.  C4 at T = 32 is what `bench.py --workload c4`
# trains, and it needs two weight-gradient chunks; n = 200 gives vertex degree 199 (C2: 39, C4: up to 79).
def _inputs(name, d):
    """-> (create_batch tuple, params) of a case's batch at width d."""
    import tspgnn
    if name == "c4":
        from oracle.anchors import grad_anchor_inputs
        t, params, _, _ = grad_anchor_inputs("c4")
        assert d == 64
        return t, params
    if name == "128x40":     # C2's batch
        return tspgnn.synthetic_batch([40] * 128, seed=1234), P.init_params(d, seed=11, perturb=True)
    if name == "32x200":     # a config-5 shard
        return tspgnn.synthetic_batch([200] * 32, seed=7), P.init_params(d, seed=9, perturb=True)
    raise KeyError(name)


def _expect(forward, backward, folded=(), pushed=(), fused_data=(), chunks=1):
    return dict(forward=forward, backward=backward, folded=folded, pushed=pushed, fused_data=fused_data, chunks=chunks)


D64_H2 = dict(folded=("E",), pushed=("V",), fused_data=("V",))
FP32_CASES = [
    ("c4", 64, 32, "f16x2", _expect("h2", "h2", chunks=(2, None), **D64_H2)),
    ("c4", 64, 8, "bf16x3", _expect("x3", "f32", folded=("E",))),
    ("c4", 64, 8, "f32", _expect("f32", "f32", folded=("E",))),
    ("32x200", 64, 8, "f16x2", _expect("h2", "h2", **D64_H2)),
    ("32x200", 64, 8, "f32", _expect("f32", "f32", folded=("E",))),
    ("128x40", 32, 32, "f16x2", _expect("h2", "h2")),
    ("128x40", 32, 32, "bf16x3", _expect("x3", "f32")),
    ("128x40", 32, 32, "f32", _expect("f32", "f32")),
    ("32x200", 32, 8, "f16x2", _expect("h2", "h2")),
    ("128x40", 128, 32, "f16x2", _expect("f32", "f32")),
    ("128x40", 128, 32, "f32", _expect("f32", "f32")),
    ("32x200", 128, 8, "f32", _expect("f32", "f32")),
]


@pytest.mark.parametrize("name,d,T,gemm,expect", FP32_CASES,
                         ids=["%s-d%d-T%d-%s" % c[:4] for c in FP32_CASES])
def test_fp32_gradients_match_teacher_forced_float64(cuda_device, measured, name, d, T, gemm, expect):
    """Every entry of every variable and every stored row against the teacher-forced float64 reference, under C2's bar
    unchanged (TF.fp32_gradient_check); the path the backward took (GraphNN.last_backward) is asserted, so that a changed
    selector fails the case instead of quietly testing another path."""
    t, params = _inputs(name, d)
    _fp32_case("%s d=%d" % (name, d), t, params, d, T, gemm, cuda_device, expect)


def _rows_report(errs):
    return "  ".join("%s rms %.1e max %.1e (%.1f ulp own binade, %.1f in range; %.2e of entries a whole ulp off)"
                     % (k, np.sqrt(e["sumsq"] / e["n"]) / e["scale"], e["max"] / e["scale"], e["ulps"], e["ulps_top"],
                        e["whole"] / e["n"]) for k, e in errs.items())


def _bf16_case(label, t, params, d, T, device, expect=None):
    """The bf16-storage training step of one batch against the teacher-forced bf16 reference in float64, pinned to the
    tape's stored intermediates and re-rounded, under TF.bf16_gradient_check's bars; ``expect``: the path (_assert_path)."""
    batch = _batch_dict(t)
    M, N = t[0].shape
    t0 = time.perf_counter()
    g, tape, loss, rec = _train_with_tape(t, params, d, T, bf16=True)
    t_dev = time.perf_counter() - t0
    H, C = tape.H, tape.C
    assert H["E"].dtype == torch.bfloat16 and C["E"].dtype == torch.float32 and tuple(H["E"].shape) == (T + 1, M, d)
    assert tuple(tape.acts[("V", 0)].shape) == (3, T, M, d) and tuple(tape.acts[("E", 0)].shape) == (3, T, N, d)
    tape_gb = sum(x.numel() * x.element_size() for x in list(H.values()) + list(C.values()) + list(tape.X.values())
                  + list(tape.ZX.values()) + list(tape.acts.values())) / 1e9
    stored = TF.bf16_tape_intermediates(tape)
    t0 = time.perf_counter()
    pinned = TF.forced_grads(params, batch, T, H, C, bf16=True, device=device, dtype=torch.float64, stored=stored)
    t_ref = time.perf_counter() - t0
    rows = TF.forced_step_errors(params, batch, T, H, C, bf16=True, device=device, stored=stored)
    rerounded = TF.forced_grads(params, batch, T, H, C, bf16=True, device=device, dtype=torch.float64)
    rows_rr = TF.forced_step_errors(params, batch, T, H, C, bf16=True, device=device)
    del tape, H, C, stored
    res = TF.bf16_gradient_check(g, pinned, rerounded, rows, rows_rr)
    (l2, per), (l2_rr, per_rr) = res["pinned"], res["rerounded"]
    print("\n[%s bf16 T=%d] loss %.6f; gradient vs teacher-forced float64: L2 %.2e, worst variable %.2e (%s; next %s); "
          "forward rows: %s\n  re-rounded reference: L2 %.2e, worst %.2e (%s; next %s); rows: %s\n  device step %.1f s (tape %.1f GB), "
          "reference %.1f s\n  path: %s"
          % (label, T, loss, l2, per[0][0], per[0][1], ", ".join("%s %.1e" % (k, r) for r, k in per[1:4]), _rows_report(rows),
             l2_rr, per_rr[0][0], per_rr[0][1], ", ".join("%s %.1e" % (k, r) for r, k in per_rr[1:4]), _rows_report(rows_rr),
             t_dev, tape_gb, t_ref, _path(rec)), end="")
    if expect is not None:
        _assert_path(rec, expect)
    assert not res["failures"], res["failures"]


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
    from, and the entry is held to 2 ulps of the tensor's scale.  (TF.bf16_gradient_check)"""
    from oracle.anchors import bf16_anchor_inputs
    t, _, d, _, _ = bf16_anchor_inputs("c5shard")
    params = P.init_params(d, seed=3, perturb=True)
    assert t[0].shape[0] == 636800
    _bf16_case("config-5 shard", t, params, d, T, cuda_device)


BF16_CASES = [
    # d = 64: the edge cell folded, the bf16-reading backward kernels with Kh resident
    ("128x40", 64, 32, _expect("bf16", "bf16-native", folded=("E",))),
    # d = 32: no bf16-reading kernels at this width -- the fp32 kernels on widened slices of the tape, unfolded
    ("128x40", 32, 8, _expect("bf16", "bf16-widened")),
]


@pytest.mark.parametrize("name,d,T,expect", BF16_CASES, ids=["%s-d%d-T%d" % c[:3] for c in BF16_CASES])
def test_bf16_gradients_match_teacher_forced_float64(cuda_device, measured, name, d, T, expect):
    """bf16 storage at the widths config 5 does not run, under config 5's bars unchanged (TF.bf16_gradient_check), the
    pinned reference from the tape's own intermediates; the path is asserted."""
    t, params = _inputs(name, d)
    _bf16_case("%s d=%d" % (name, d), t, params, d, T, cuda_device, expect)
