"""Message MLPs of every depth, with and without a relu on their last layer (GraphNN's MLP_depth and Msg_last_activation,
build_network's keywords of the same names): every other file runs three hidden layers and a linear last one.  The two
values decide whether the vertex cell is pushed, the layers and relu masks of every message launch, of the fused cell +
message launches, of the one-launch loops and of the recomputing backward, the tape's acts, and how many kernels a chain
takes (four layers each, two at d = 128).  Here each (depth, last activation) runs

  (a) the inference forward against float64, every row under device_reference.reference's bars (bf16 storage: under the bars
      of test_gpu_model.py::test_bf16_storage_mode);
  (b) the one-launch loops against the stepwise launches, bit for bit;
  (c) a training step's gradients against the teacher-forced float64 reference at the tape's states, under
      teacher_forced.fp32_gradient_check / bf16_gradient_check, with the backward's path asserted;
  (d) the refusals: message MLPs of five layers do not train, and bf16 storage does not run them at all.

(3, None) is the control: the configuration of every other file, through this file's harness.  One small batch serves
everything: 8 instances of 3 to 40 vertices, 1754 edge rows and 138 vertices, partial 16-row tiles on both sides."""
import time

import numpy as np
import pytest
import torch

import tspgnn
from conftest import batch_from_tuple, rel_err
from oracle import device_reference as DR
from oracle import params as P
from oracle import teacher_forced as TF
from oracle import torch_oracle as TO
from test_gpu_forced_gradients import _assert_path, _path
from test_gpu_loop import assert_bit_equal

pytestmark = pytest.mark.gpu

SIZES = [7, 33, 12, 40, 5, 3, 17, 21]
CASES = [(0, None), (0, "relu"), (1, None), (1, "relu"), (2, None), (2, "relu"), (3, "relu"), (3, None)]
UP_TO_DEPTH_2 = [c for c in CASES if c[0] <= 2]
ARITH = {"f16x2": "h2", "bf16x3": "x3", "f32": None}
FORWARD_T = (1, 4)
TRAIN_T = 3
BF16 = torch.bfloat16


def _id(case):
    return "depth%d-%s" % (case[0], case[1] or "linear")


def _ids(cases):
    return [_id(c) for c in cases]


@pytest.fixture(scope="module", autouse=True)
def file_measured():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\n[message depth] file wall %.1f s" % (time.perf_counter() - t0))


@pytest.fixture(autouse=True)
def default_selectors(monkeypatch):
    for k in ("TSPGNN_LOOP", "TSPGNN_LOOP_KIND", "TSPGNN_LOOP_MAX_TILES", "TSPGNN_GEMM", "TSPGNN_PUSH_TRAINING",
              "TSPGNN_FUSE_TRAINING", "TSPGNN_RECOMPUTE", "TSPGNN_MLP_BWD_H2", "TSPGNN_BF16_BACKWARD",
              "TSPGNN_FUSE_DATA_GRADIENTS"):
        monkeypatch.delenv(k, raising=False)


class Shared(object):
    """The batch, and per (d, depth[, last]) the weights and the float64 forward reference with its per-row bars: computed
    once, on first use, and left unchanged."""

    def __init__(self, device):
        self.device = device
        self.t = tspgnn.synthetic_batch(SIZES, seed=5)
        self.batch = batch_from_tuple(self.t)
        assert self.t[0].shape == (1754, 138)
        self._params, self._refs = {}, {}

    def params(self, d, depth):
        if (d, depth) not in self._params:
            self._params[(d, depth)] = P.init_params(d, seed=31 + depth, perturb=True, msg_layers=depth + 1)
        return self._params[(d, depth)]

    def reference(self, d, case):
        if (d, case) not in self._refs:
            self._refs[(d, case)] = DR.reference(self.params(d, case[0]), self.batch, [1, 2, 4], self.device,
                                                 msg_last_relu=case[1] == "relu")
        return self._refs[(d, case)]


@pytest.fixture(scope="module")
def shared(cuda_device):
    s = Shared(cuda_device)
    yield s
    s._refs.clear()
    torch.cuda.empty_cache()


def _session(shared, d, case, gemm=None, float_dtype=torch.float32, **attrs):
    model = tspgnn.build_network(d, float_dtype=float_dtype, MLP_depth=case[0], Msg_last_activation=case[1])
    gnn = model["gnn"]
    if gemm is not None:
        gnn.gemm = gemm
    for k, v in attrs.items():
        setattr(gnn, k, v)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(shared.params(d, case[0]))
    assert all(m.n_square == case[0] + 1 and m.relu[-1] == (case[1] == "relu") for m in gnn._msg_MLPs.values())
    return model, sess


def _feed(model, t, T):
    EV, W, C, route_exists, n_vertices, n_edges = t
    return {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}


def _forward(model, sess, shared, T):
    """-> (predictions, last states, the form the loop ran in, the guard's status word) of one inference forward."""
    pred, last = sess.run([model["predictions"], model["last_states"]], feed_dict=_feed(model, shared.t, T))
    return pred, last, model["gnn"].launched_loop, int(model.store.guard.peek().status)


def _rows_under_their_bars(shared, d, case, T, pred, last, what):
    """(a): predictions and every row of the four state arrays under device_reference.reference's per-row bars; -> the
    worst err / bar."""
    ref, bars = shared.reference(d, case)
    res = [DR.compare_rows(pred, ref[T]["predictions"], bars[T]["predictions"], shared.batch, "predictions")]
    for k in DR.STATES:
        v, part = k.split(".")
        res.append(DR.compare_rows(getattr(last[v], part), ref[T][k], bars[T][k], shared.batch, k))
    worst = max(res, key=lambda r: r["worst"])
    print("\n[message depth forward] d=%d %s %s: worst %s" % (d, _id(case), what, DR.describe(worst)), end="")
    bad = [DR.describe(r) for r in res if r["over"]]
    assert not bad, "%s:\n  %s" % (what, "\n  ".join(bad))
    return worst["worst"]


# ---------------------------------------------------------------- a. inference forward, every row against float64
FORWARD_CASES = [(64, g, c) for g in ("f16x2", "bf16x3", "f32") for c in CASES] + [(32, "f16x2", c) for c in CASES] \
    + [(128, "f16x2", c) for c in UP_TO_DEPTH_2]


@pytest.mark.parametrize("d,gemm,case", FORWARD_CASES, ids=["d%d-%s-%s" % (d, g, _id(c)) for d, g, c in FORWARD_CASES])
def test_forward_rows_match_float64(shared, d, gemm, case):
    """T = 1 (the last-step launches alone) and T = 4, as the selector routes the batch: V.h, V.c, E.h, E.c and the
    predictions, every row under its bar (float64 oracle, its float32 run, the 2^-22 weight draws; floor 1e-5)."""
    model, sess = _session(shared, d, case, gemm)
    gnn = model["gnn"]
    for T in FORWARD_T:
        pred, last, launched, status = _forward(model, sess, shared, T)
        assert status == 0 and sess.last_range_bits == 0
        assert gnn.active_arith() == ARITH[gemm]
        _rows_under_their_bars(shared, d, case, T, pred, last, "%s T=%d launched_loop=%s" % (gemm, T, launched))


BF16_FORWARD_CASES = [(64, c) for c in CASES] + [(128, c) for c in UP_TO_DEPTH_2]


@pytest.mark.parametrize("d,case", BF16_FORWARD_CASES, ids=["d%d-%s" % (d, _id(c)) for d, c in BF16_FORWARD_CASES])
def test_bf16_storage_forward(shared, d, case):
    """bf16 storage against the oracle that rounds at the same points and against the fp32 semantics, under the bars of
    test_gpu_model.py::test_bf16_storage_mode unchanged."""
    model, sess = _session(shared, d, case, float_dtype=BF16)
    relu = case[1] == "relu"
    params64 = TO.to_torch(shared.params(d, case[0]), torch.float64)
    for T in FORWARD_T:
        pred, last, loss = sess.run([model["predictions"], model["last_states"], model["loss"]],
                                    feed_dict=_feed(model, shared.t, T))
        assert model["gnn"].launched_loop is None
        ref = TO.forward(params64, shared.batch, T, bf16=True, msg_last_relu=relu)
        full = TO.forward(params64, shared.batch, T, msg_last_relu=relu)
        ref_h = ref["last_states"]["E"][0].numpy()
        e_h = rel_err(last["E"].h, ref_h)
        e_c = rel_err(last["V"].c, ref["last_states"]["V"][1].numpy())
        e_p = rel_err(pred, ref["predictions"].numpy())
        a_h = rel_err(last["E"].h, full["last_states"]["E"][0].numpy())
        a_p = rel_err(pred, full["predictions"].numpy())
        r_h = float(np.sqrt(((np.asarray(last["E"].h, dtype=np.float64) - ref_h) ** 2).mean()) / np.abs(ref_h).max())
        e_l = abs(float(loss) - ref["loss"].item())
        print("\n[message depth forward bf16] d=%d %s T=%d: vs bf16 oracle E.h %.2e (rms %.2e) V.c %.2e pred %.2e loss %.1e | "
              "vs fp32 semantics E.h %.2e pred %.2e" % (d, _id(case), T, e_h, r_h, e_c, e_p, e_l, a_h, a_p), end="")
        assert e_h < 2e-2 and e_c < 1e-2 and r_h < 2e-3 and e_p < 1e-3
        assert a_h < 4e-2 and a_p < 1e-2
        assert e_l < 5e-4


# ---------------------------------------------------------------- b. the one-launch loops
@pytest.mark.parametrize("kind", ["loop", "resident"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_one_launch_loop_equals_stepwise_launches(shared, monkeypatch, case, kind):
    """tspgnn_mp_loop_h2 / tspgnn_mp_resident_h2 with the edge side's message MLP of one to three layers, pushed
    (v_zbias) or not, against the stepwise launches: the same bits, the form asked for, the guard's status word 0.  The
    unpushed four-layer edge-side MLP of (3, relu) does not fit beside Kh in LDS: the selector falls back, and what ran
    instead is held to the float64 bars like every other."""
    monkeypatch.setenv("TSPGNN_LOOP_MAX_TILES", "4")
    monkeypatch.setenv("TSPGNN_LOOP_KIND", kind)
    T = 4
    got = {}
    for loop in (True, False):
        model, sess = _session(shared, 64, case, "f16x2", persistent_loop=loop)
        b = sess.prepare(_feed(model, shared.t, T))
        assert b.adj.loop_plan is not None and b.adj.loop_plan[3] == kind
        got[loop] = _forward(model, sess, shared, T)
        assert got[loop][3] == 0 and sess.last_range_bits == 0 and model["gnn"].active_arith() == "h2"
    assert got[True][2] == (None if case == (3, "relu") else kind), got[True][2]
    assert got[False][2] is None
    assert_bit_equal(got[True][:3], got[False][:3])
    _rows_under_their_bars(shared, 64, case, T, got[True][0], got[True][1], "%s T=%d launched_loop=%s" % (kind, T, got[True][2]))


# ---------------------------------------------------------------- c. training gradients
def _expected_path(d, gemm, case, bf16=False, pushes=True):
    if bf16:
        forward, backward = "bf16", "bf16-native" if d == 64 else "bf16-widened"
    elif d == 128:
        forward, backward = "f32", "f32"
    else:
        forward, backward = ARITH[gemm] or "f32", "h2" if gemm == "f16x2" else "f32"
    pushed = ("V",) if (pushes and not bf16 and d == 64 and gemm == "f16x2" and case[1] is None and case[0] >= 1) else ()
    return dict(forward=forward, backward=backward, folded=("E",) if d == 64 else (), pushed=pushed, fused_data=pushed, chunks=1)


def _train(shared, d, case, gemm=None, float_dtype=torch.float32, **attrs):
    model, sess = _session(shared, d, case, gemm, float_dtype, **attrs)
    out = sess.loss_and_grads(_feed(model, shared.t, TRAIN_T), keep_tape=True)
    torch.cuda.synchronize()
    assert sess.store.guard.peek().activation == 0
    g = {k: np.asarray(v, dtype=np.float64) for k, v in model.store.grad_dict().items()}
    return g, out["tape"], model["gnn"].last_backward


def _fp32_gradients(shared, d, case, gemm, pushes=True, **attrs):
    """Every entry of every variable against the teacher-forced float64 reference at the tape's states, every stored row
    against one oracle step: TF.fp32_gradient_check's bars; the path the backward took asserted."""
    params, batch, device, T = shared.params(d, case[0]), shared.batch, shared.device, TRAIN_T
    g, tape, rec = _train(shared, d, case, gemm, **attrs)
    H, C = tape.H, tape.C
    assert H["E"].dtype == torch.float32 and tuple(H["E"].shape) == (T + 1, 1754, d)
    kw = dict(bf16=False, device=device, msg_last_relu=case[1] == "relu")
    f64 = TF.forced_grads(params, batch, T, H, C, dtype=torch.float64, **kw)
    assert sorted(f64) == sorted(g)
    with DR.no_tf32():
        f32 = TF.forced_grads(params, batch, T, H, C, dtype=torch.float32, **kw)
    draws = [TF.forced_grads(params, batch, T, H, C, dtype=torch.float64, weights=DR.spread_draw(params, draw), **kw)
             for draw in range(DR.SPREAD_DRAWS)]
    errs = TF.forced_step_errors(params, batch, T, H, C, **kw)
    res = TF.fp32_gradient_check(g, f64, f32, draws, errs)
    r = res["ratios"]
    print("\n[message depth gradients] d=%d %s %s %s: worst ratio to the bar %.3f (%s), worst norm ratio %.3f; rows %s; path: %s"
          % (d, gemm, _id(case), attrs or "", r[0][0], r[0][1], max(x[4] for x in r),
             " ".join("%s %.1e" % kv for kv in res["rows"].items()), _path(rec)), end="")
    _assert_path(rec, _expected_path(d, gemm, case, pushes=pushes))
    assert not res["failures"], res["failures"]
    return tape


FP32_CASES = [(64, g, c) for g in ("f16x2", "bf16x3", "f32") for c in CASES] + [(d, "f16x2", c) for d in (32, 128) for c in CASES]


@pytest.mark.parametrize("d,gemm,case", FP32_CASES, ids=["d%d-%s-%s" % (d, g, _id(c)) for d, g, c in FP32_CASES])
def test_fp32_gradients_match_teacher_forced_float64(shared, d, gemm, case):
    _fp32_gradients(shared, d, case, gemm)


SWITCHES = [("unpushed", dict(push_training=False), False), ("recompute", dict(recompute_messages=True), True),
            ("fused", dict(fuse_training_messages=True), False)]


@pytest.mark.parametrize("label,attrs,pushes", SWITCHES, ids=[s[0] for s in SWITCHES])
@pytest.mark.parametrize("case", [(1, None), (2, None)], ids=_ids([(1, None), (2, None)]))
def test_fp32_gradients_of_pushable_cases_under_the_training_switches(shared, case, label, attrs, pushes):
    """Where the vertex cell is pushed by default: the same chains unpushed, recomputed in the backward (a pushed prefix of
    one layer leaves nothing to save) and inside the cell launches of the training forward."""
    tape = _fp32_gradients(shared, 64, case, "f16x2", pushes=pushes, **attrs)
    assert tape.rc == ({("V", 0): True} if label == "recompute" else {}) and tape.fused == (label != "unpushed")


BF16_TRAIN_CASES = [(d, c) for d in (64, 32) for c in CASES]


@pytest.mark.parametrize("d,case", BF16_TRAIN_CASES, ids=["d%d-%s" % (d, _id(c)) for d, c in BF16_TRAIN_CASES])
def test_bf16_gradients_match_teacher_forced_float64(shared, d, case):
    """bf16 storage, d = 64 (the bf16-reading backward on the tape as it is) and d = 32 (fp32 kernels on widened slices):
    TF.bf16_gradient_check's bars against the teacher-forced bf16 reference, pinned to the tape's intermediates and
    re-rounded."""
    params, batch, device, T = shared.params(d, case[0]), shared.batch, shared.device, TRAIN_T
    g, tape, rec = _train(shared, d, case, float_dtype=BF16)
    H, C = tape.H, tape.C
    assert H["E"].dtype == BF16 and C["E"].dtype == torch.float32
    stored = TF.bf16_tape_intermediates(tape)
    kw = dict(bf16=True, device=device, msg_last_relu=case[1] == "relu")
    pinned = TF.forced_grads(params, batch, T, H, C, dtype=torch.float64, stored=stored, **kw)
    rows = TF.forced_step_errors(params, batch, T, H, C, stored=stored, **kw)
    rerounded = TF.forced_grads(params, batch, T, H, C, dtype=torch.float64, **kw)
    rows_rr = TF.forced_step_errors(params, batch, T, H, C, **kw)
    res = TF.bf16_gradient_check(g, pinned, rerounded, rows, rows_rr)
    (l2, per), (l2_rr, per_rr) = res["pinned"], res["rerounded"]
    print("\n[message depth gradients bf16] d=%d %s: pinned L2 %.2e (%.3f of its bar), worst variable %.2e (%.3f of its bar, %s); "
          "re-rounded L2 %.2e worst %.2e; path: %s" % (d, _id(case), l2, l2 / TF.BF16_L2, per[0][0], per[0][0] / TF.BF16_WORST,
                                                      per[0][1], l2_rr, per_rr[0][0], _path(rec)), end="")
    _assert_path(rec, _expected_path(d, None, case, bf16=True))
    assert not res["failures"], res["failures"]


# ---------------------------------------------------------------- d. refusals
DEPTH_4 = (4, None)
REFUSED_TRAINING = [(64, "f16x2", torch.float32), (64, "bf16x3", torch.float32), (64, "f32", torch.float32),
                    (32, "f16x2", torch.float32), (128, "f16x2", torch.float32), (64, "f16x2", BF16), (128, "f16x2", BF16)]


@pytest.mark.parametrize("d,gemm,dtype", REFUSED_TRAINING,
                         ids=["d%d-%s-%s" % (d, g, "bf16" if t == BF16 else "fp32") for d, g, t in REFUSED_TRAINING])
def test_five_layer_message_mlps_do_not_train(shared, d, gemm, dtype):
    """MLP_depth = 4: NotImplementedError before anything is launched or zeroed -- not an error code from the library in the
    middle of a pass -- and the variables and the gradient buffer are as they were."""
    model, sess = _session(shared, d, DEPTH_4, gemm, dtype)
    store = model.store
    store.zero_grad().fill_(1.0)
    theta = store.theta.clone()
    with pytest.raises(NotImplementedError):
        sess.loss_and_grads(_feed(model, shared.t, TRAIN_T))
    with pytest.raises(NotImplementedError):
        sess.run(model["train_step"], feed_dict=_feed(model, shared.t, TRAIN_T))
    torch.cuda.synchronize()
    assert torch.equal(store.theta, theta) and bool((store.grad == 1.0).all())


@pytest.mark.parametrize("d", [64, 128])
def test_bf16_storage_refuses_five_layer_message_mlps_in_inference(shared, d):
    model, sess = _session(shared, d, DEPTH_4, float_dtype=BF16)
    store = model.store
    store.zero_grad().fill_(1.0)
    theta = store.theta.clone()
    with pytest.raises(NotImplementedError):
        sess.run(model["predictions"], feed_dict=_feed(model, shared.t, 2))
    torch.cuda.synchronize()
    assert torch.equal(store.theta, theta) and bool((store.grad == 1.0).all())


def test_fp32_inference_runs_five_layer_message_mlps_on_the_general_path(shared):
    """fp32 storage at d = 64: a five-layer chain is two kernels (4 + 1), so neither launch plan takes it and the forward
    goes step by step through the fp32 kernels; every row under its bar at T = 2."""
    model, sess = _session(shared, 64, DEPTH_4, "f16x2")
    gnn = model["gnn"]
    assert all(m._chunks() == [(0, 4), (4, 1)] for m in gnn._msg_MLPs.values())
    pred, last, launched, status = _forward(model, sess, shared, 2)
    assert launched is None and status == 0 and getattr(gnn, "_plan_keep", None) is None
    _rows_under_their_bars(shared, 64, DEPTH_4, 2, pred, last, "general path T=2")
