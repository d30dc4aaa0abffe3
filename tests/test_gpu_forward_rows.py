"""Every row of the inference forward at full size against a float64 reference computed on the GPU
(oracle/device_reference.py) -- the anchors (test_gpu_anchors.py) keep 512 sampled rows and column sums of the last
states; here every row of V.h, V.c, E.h and E.c is held to its own bar at depths 1, 2, 8 and T, each depth its own
forward (so each also runs the last-step code), on every path the selector can give these batches: the stepwise launches
in each GEMM arithmetic, the register-resident loop (tspgnn_mp_loop_h2) and the memory-resident one (tspgnn_mp_resident_h2).
The path that actually ran is asserted (GraphNN.launched_loop, active_arith, the range guard), not inferred from the plan.

Per-row bar (device_reference.reference): max(1e-5 S, 2x what float32 loses on the row, 2x how far the row moves when every
weight moves by 2^-22).  Teacher-forced windows (k = 1, 3 steps from the float64 state rounded to fp32, through
GraphNN.__call__ with supplied states) check the same kernels without the recurrence's amplification.  BASELINE config 5's
bf16-storage mode at its shard (32 x n=200, d=128) is held to test_gpu_anchors.py's and test_gpu_forced_gradients.py's
bf16 bars over all rows."""
import os
import time

import numpy as np
import pytest
import torch

import tspgnn
from conftest import GOLDEN, batch_from_tuple
from oracle import device_reference as DR
from oracle import params as P
from oracle import teacher_forced as TF
from oracle.anchors import anchor_inputs, anchor_rows

pytestmark = pytest.mark.gpu

ARITH = {"f16x2": "h2", "bf16x3": "x3", "f32": None}
LOOP_ENV = ("TSPGNN_LOOP", "TSPGNN_LOOP_KIND", "TSPGNN_LOOP_MAX_TILES")
STEPS = {"TSPGNN_LOOP": "0"}
LOOP4 = {"TSPGNN_LOOP_KIND": "loop", "TSPGNN_LOOP_MAX_TILES": "4"}
RESIDENT = {"TSPGNN_LOOP_KIND": "resident"}


def _inputs(name):
    """-> (create_batch tuple, params, d, T): the anchors' batches and weights for c1 / c2 / c4, perturbed weights otherwise."""
    if name in ("c1", "c2", "c4"):
        t, params, T, _ = anchor_inputs(name)
        return t, params, 64, T
    if name == "192x40":
        return tspgnn.synthetic_batch([40] * 192, seed=5), P.init_params(64, seed=9, perturb=True), 64, 32
    if name == "32x200":
        return tspgnn.synthetic_batch([200] * 32, seed=7), P.init_params(64, seed=9, perturb=True), 64, 8
    if name == "32x200d128":
        return tspgnn.synthetic_batch([200] * 32, seed=7), P.init_params(128, seed=3, perturb=True), 128, 8
    if name == "128x40d32":
        return tspgnn.synthetic_batch([40] * 128, seed=5), P.init_params(32, seed=9, perturb=True), 32, 32
    if name == "32x200d32":
        return tspgnn.synthetic_batch([200] * 32, seed=7), P.init_params(32, seed=9, perturb=True), 32, 8
    raise KeyError(name)


WINDOWED = ("c2", "192x40", "32x200")


def _e2e_depths(T):
    return sorted({1, 2, 8, T})


def _window_starts(T):
    return (0, T // 2, T - 1)


class Ref(object):
    def __init__(self, name, device):
        self.name, self.device = name, device
        self.t, self.params, self.d, self.T = _inputs(name)
        self.batch = batch_from_tuple(self.t)
        depths = set(_e2e_depths(self.T)) | (set(_window_starts(self.T)) if name in WINDOWED else set())
        self.ref, self.bars = DR.reference(self.params, self.batch, depths, device)
        self.windows = {}

    def window(self, t0):
        """Float64 reference (and bars) of k = 1 and 3 steps from the float64 state at depth t0 rounded to fp32 -> (start
        state in fp32, {k: trajectory}, {k: bars}); at t0 = 0 the cell states are None (no initial cell state)."""
        if t0 not in self.windows:
            s = self.ref[t0]
            start = tuple(s[k].to(torch.float32) for k in DR.STATES)
            if t0 == 0:
                start = (start[0], None, start[2], None)
            r, b = DR.reference(self.params, self.batch, [1, 3], self.device, start=start)
            self.windows[t0] = (start, r, b)
        return self.windows[t0]


@pytest.fixture(scope="module", autouse=True)
def file_measured():
    """Wall time and peak device memory of the whole file."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\n[forward rows] file wall %.1f s, peak device memory %.1f GB" % (time.perf_counter() - t0,
                                                                             torch.cuda.max_memory_allocated() / 1e9))


@pytest.fixture(scope="module")
def refs(cuda_device):
    """{configuration name: Ref}, each configuration's float64 trajectory and per-row bars computed once, on first use, and
    freed at the end of the file."""
    class Refs(dict):
        def __missing__(self, name):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = self[name] = Ref(name, cuda_device)
            torch.cuda.synchronize()
            print("\n[reference %s] M=%d N=%d d=%d T=%d: float64 trajectory + bars %.1f s, %.1f GB held, peak so far %.1f GB"
                  % (name, r.t[0].shape[0], r.t[0].shape[1], r.d, r.T, time.perf_counter() - t0,
                     torch.cuda.memory_allocated() / 1e9, torch.cuda.max_memory_allocated() / 1e9))
            return r
    cache = Refs()
    yield cache
    cache.clear()
    torch.cuda.empty_cache()


def _session(d, gemm, float_dtype=torch.float32):
    model = tspgnn.build_network(d, float_dtype=float_dtype)
    if gemm is not None:
        model["gnn"].gemm = gemm
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    return model, sess


def _feed(model, t, T):
    EV, W, C, route_exists, n_vertices, n_edges = t
    return {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}


def _set_env(monkeypatch, env):
    for k in LOOP_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _plan_kind(b):
    return None if b.adj.loop_plan is None else b.adj.loop_plan[3]


def _check(results, what):
    worst = max(results, key=lambda r: r["worst"])
    print("  %s: worst %s" % (what, DR.describe(worst)))
    bad = [DR.describe(r) for r in results if r["over"]]
    assert not bad, "%s:\n  %s" % (what, "\n  ".join(bad))
    return worst["worst"]


# ---------------------------------------------------------------- a. the device reference is the committed anchors'
@pytest.mark.parametrize("name", ["c1", "c2", "c4"])
def test_device_reference_reproduces_the_committed_anchor(refs, name):
    """The in-test float64 reference (GPU) against the anchor generated on the host (tests/golden/anchor_*.npz):
    predictions, loss, sampled rows and column sums within 1e-10 relative."""
    ref = refs[name]
    z = np.load(os.path.join(GOLDEN, "anchor_%s.npz" % ref.name))
    _, _, T, finger = anchor_inputs(ref.name)
    assert T == ref.T == int(z["T"]) and np.array_equal(finger, z["fingerprint"])
    r = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in ref.ref[T].items()}
    worst = {"predictions": np.abs(r["predictions"] - z["predictions"]).max() / np.abs(z["predictions"]).max(),
             "loss": abs(float(r["loss"]) - float(z["loss"])) / abs(float(z["loss"]))}
    assert float(r["acc"]) == float(z["acc"])
    for v in ("E", "V"):
        for part in ("h", "c"):
            a = r["%s.%s" % (v, part)]
            scale = float(z["%s%s_absmax" % (v, part)])
            worst["%s.%s absmax" % (v, part)] = abs(np.abs(a).max() - scale) / scale
            worst["%s.%s rows" % (v, part)] = np.abs(a[anchor_rows(a.shape[0])] - z["%s%s_rows" % (v, part)]).max() / scale
            cs = z["%s%s_colsum" % (v, part)]
            worst["%s.%s colsum" % (v, part)] = np.abs(a.sum(0) - cs).max() / np.abs(cs).max()
    print("\n  anchor %s: device float64 vs host float64: %s" % (ref.name, "  ".join("%s %.1e" % kv for kv in worst.items())))
    for k, e in worst.items():
        assert e <= 1e-10, (k, e)


# ---------------------------------------------------------------- b. end to end, every row
# per configuration: (label, environment, GEMM arithmetic, loop plan the batch gets, form that must run)
E2E = {
    "c1": [("steps", STEPS, g, None, None) for g in ARITH] + [("default", {}, "f16x2", "loop", "loop"),
                                                              ("resident", RESIDENT, "f16x2", "resident", "resident")],
    "c2": [("default", {}, g, None, None) for g in ARITH] + [("loop", LOOP4, "f16x2", "loop", "loop"),
                                                             ("resident", RESIDENT, "f16x2", "resident", "resident")],
    "192x40": [("default", {}, "f16x2", "resident", "resident"), ("steps", STEPS, "f16x2", None, None)],
    "c4": [("default", {}, g, None, None) for g in ARITH],
    "32x200": [("resident", RESIDENT, "f16x2", "resident", "resident"), ("default", {}, "f16x2", None, None)],
    "32x200d128": [("default", {}, "f32", None, None)],
    # d = 32: the one-launch loops are d = 64 only, so the stepwise launches run the <32> templates at size
    "128x40d32": [("default", {}, g, None, None) for g in ARITH],
    "32x200d32": [("default", {}, g, None, None) for g in ARITH],
}


def _each_path(ref, paths, monkeypatch, run):
    """run(label, gemm, plan, launched, model, sess) -> worst err/bar, for every path of the configuration, each in its own
    session (the adjacency and its loop plan are made under the path's environment); every path runs, the failures are
    reported together."""
    failed, summary = [], []
    for label, env, gemm, plan, launched in paths:
        _set_env(monkeypatch, env)
        model, sess = _session(ref.d, gemm)
        model.store.load(ref.params)
        print("\n[%s %s %s]" % (ref.name, label, gemm))
        try:
            summary.append("%s/%s %.3f" % (label, gemm, run(label, gemm, plan, launched, model, sess)))
        except AssertionError as e:
            failed.append("%s %s %s: %s" % (ref.name, label, gemm, e))
            summary.append("%s/%s FAILED" % (label, gemm))
    return failed, summary


@pytest.mark.parametrize("name", list(E2E))
def test_forward_every_row_matches_float64(refs, name, monkeypatch):
    """Each path of the configuration, end to end at depths 1, 2, 8 and T: the plan the batch gets and the form and
    arithmetic that ran are asserted; predictions, loss and every row of the four state arrays are held to their per-row
    bars; acc, TP, FP, TN and FN are the float64 reference's exactly."""
    ref = refs[name]
    def run(label, gemm, plan, launched, model, sess):
        gnn = model["gnn"]
        worst = 0.0
        for t in _e2e_depths(ref.T):
            feed = _feed(model, ref.t, t)
            b = sess.prepare(feed)
            assert _plan_kind(b) == plan, "loop plan %r, expected %r" % (_plan_kind(b), plan)
            pred, loss, acc, TP, FP, TN, FN, last = sess.run(
                [model[k] for k in ("predictions", "loss", "acc", "TP", "FP", "TN", "FN", "last_states")], feed_dict=feed)
            assert gnn.launched_loop == launched, "T=%d: %r ran, expected %r" % (t, gnn.launched_loop, launched)
            assert gnn.active_arith() == ARITH[gemm] and sess.last_range_bits == 0, (gnn.active_arith(), sess.last_range_bits)
            r, bars = ref.ref[t], ref.bars[t]
            for k, got in (("acc", acc), ("TP", TP), ("FP", FP), ("TN", TN), ("FN", FN)):
                assert float(got) == float(np.float32(float(r[k]))), (t, k, float(got), float(r[k]))
            res = [DR.compare_rows(pred, r["predictions"], bars["predictions"], ref.batch, "predictions"),
                   DR.compare_rows(np.float64(loss), r["loss"], bars["loss"], ref.batch, "loss")]
            for k in DR.STATES:
                v, part = k.split(".")
                res.append(DR.compare_rows(getattr(last[v], part), r[k], bars[k], ref.batch, k))
            del last
            worst = max(worst, _check(res, "T=%d plan %s ran %s arith %s" % (t, plan, gnn.launched_loop, gnn.active_arith())))
        return worst
    failed, summary = _each_path(ref, E2E[ref.name], monkeypatch, run)
    print("[rows] %s end to end, worst err/bar: %s" % (ref.name, ", ".join(summary)))
    assert not failed, "\n".join(failed)


def test_no_loop_plan_takes_c4(cuda_device, monkeypatch):
    """C4's 512 ragged instances (695 849 edge rows) fit neither one-launch form, whichever is forced."""
    t, params, _, T = _inputs("c4")
    for env in ({}, LOOP4, RESIDENT):
        _set_env(monkeypatch, env)
        model, sess = _session(64, "f16x2")
        assert sess.prepare(_feed(model, t, T)).adj.loop_plan is None, env


# ---------------------------------------------------------------- c. teacher-forced windows through the inference kernels
WINDOWS = {
    "c2": E2E["c2"],
    "192x40": [("default", {}, "f16x2", "resident", "resident")],
    "32x200": [("resident", RESIDENT, "f16x2", "resident", "resident")],
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_teacher_forced_windows_match_float64(refs, name, monkeypatch):
    """k = 1 and 3 steps of GraphNN.__call__ from the float64 state at t0 in {0, T/2, T-1} rounded to fp32 (t0 = 0: no
    initial cell state), on the prepared batch's DeviceAdjacency (its loop plan applies), against k float64 steps from the
    same state, every row, with the same per-row bars over the window.  A path that does not take supplied states fails
    the launched-form assertion instead of testing the stepwise launches twice."""
    ref = refs[name]
    def run(label, gemm, plan, launched, model, sess):
        gnn = model["gnn"]
        b = sess.prepare(_feed(model, ref.t, ref.T))
        assert _plan_kind(b) == plan, "loop plan %r, expected %r" % (_plan_kind(b), plan)
        worst = 0.0
        for t0 in _window_starts(ref.T):
            (Vh, Vc, Eh, Ec), wr, wb = ref.window(t0)
            cells = {} if t0 == 0 else {"V": Vc, "E": Ec}
            for k in (1, 3):
                out = gnn({"EV": b.adj}, {"V": Vh, "E": Eh}, k, LSTM_initial_states=cells)
                torch.cuda.synchronize()
                assert gnn.launched_loop == launched, "from supplied states (t0=%d, %s cell state) %r ran, not %r" % (
                    t0, "no" if t0 == 0 else "a", gnn.launched_loop, launched)
                assert gnn.active_arith() == ARITH[gemm] and not sess.range_exceeded()
                res = [DR.compare_rows(getattr(out[key[0]], key[2]), wr[k][key], wb[k][key], ref.batch, key)
                       for key in DR.STATES]
                del out
                worst = max(worst, _check(res, "t0=%d k=%d ran %s" % (t0, k, gnn.launched_loop)))
        return worst
    failed, summary = _each_path(ref, WINDOWS[ref.name], monkeypatch, run)
    print("[rows] %s windows, worst err/bar: %s" % (ref.name, ", ".join(summary)))
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------- d. bf16 storage at config 5's shard
@pytest.fixture(scope="module")
def bf16_ref(cuda_device):
    t, params, d, _ = _inputs("32x200d128")
    batch = batch_from_tuple(t)
    t0 = time.perf_counter()
    r = DR.trajectory(params, batch, [0, 1, 2, 4, 7, 8], torch.float64, cuda_device, bf16=True)
    torch.cuda.synchronize()
    print("\n[reference bf16 32x200 d=128] float64 bf16-storage trajectory %.1f s" % (time.perf_counter() - t0))
    yield t, params, d, batch, r
    del r
    torch.cuda.empty_cache()


def test_bf16_storage_every_row_at_config5_shard(cuda_device, bf16_ref):
    """End to end at T = 1, 2, 8 against the float64 bf16-storage oracle (the inference forward's fold), every row, with
    test_gpu_anchors.py::test_bf16_storage_at_config5_depth's bars: max < 2e-2 and rms < 1.5e-3 of the tensor's largest
    entry; predictions within 5e-4, loss within 2e-4."""
    t, params, d, batch, r = bf16_ref
    model, sess = _session(d, None, torch.bfloat16)
    model.store.load(params)
    print()
    for T in (1, 2, 8):
        pred, loss, last = sess.run([model["predictions"], model["loss"], model["last_states"]], feed_dict=_feed(model, t, T))
        assert model["gnn"].launched_loop is None
        rep = []
        for k in DR.STATES:
            v, part = k.split(".")
            ref = r[T][k]
            scale = float(ref.abs().max())
            e = (torch.as_tensor(getattr(last[v], part)).to(ref.device, torch.float64) - ref).abs() / scale
            mx, rms = float(e.max()), float(torch.sqrt((e ** 2).mean()))
            row = int(torch.argmax(e.amax(dim=1)))
            rep.append("%s max %.1e (row %d) rms %.1e" % (k, mx, row, rms))
            assert mx < 2e-2 and rms < 1.5e-3, (T, k, mx, rms, row)
        e_pred = float(np.abs(pred - r[T]["predictions"].cpu().numpy()).max() / r[T]["predictions"].abs().max().item())
        e_loss = abs(float(loss) - float(r[T]["loss"]))
        print("  [bf16 T=%d] pred %.1e loss %.1e  %s" % (T, e_pred, e_loss, "  ".join(rep)))
        assert e_pred < 5e-4 and e_loss < 2e-4


def test_bf16_storage_one_step_windows(cuda_device, bf16_ref):
    """One step of GraphNN.__call__ in bf16 storage from the float64 bf16-storage state at t0 in {0, 4, 7} (h bf16-valued,
    c rounded to fp32; t0 = 0: no initial cell state) against one float64 step_bf16 from the same state -- with the edge
    cell in the inference forward's folded form (device_reference.INFERENCE_FOLD) --, every row, with the stored-row bars of
    test_gpu_forced_gradients.py for a reference that re-decides the roundings: rms < 0.1 * 2^-8 of the scale, c max < 2^-7,
    and h max within 2 * 2^-8 of the scale (or 2x what the same oracle step in float32 misses by, if more).  The 2-ulp bar on
    h there holds only against the device's OWN rounded intermediates, which the inference forward does not keep: re-decided,
    the vertex cell's input -- the bf16-rounded sum of 199 edge messages -- and the projected messages Zx land an ulp apart
    wherever an fp32 sum and the float64 one straddle a rounding boundary, and the oracle step in float32 itself misses h by
    up to 40 ulps of an entry's own binade (printed).  The training forward's form (the aggregate rounded instead of Zx, at
    d = 128) is printed next to it."""
    t, params, d, batch, r = bf16_ref
    model, sess = _session(d, None, torch.bfloat16)
    model.store.load(params)
    b = sess.prepare(_feed(model, t, 1))
    gnn = model["gnn"]

    def report(errs):
        return "  ".join("%s rms %.1e max %.1e (%.1f ulp in range, %.1e of entries a whole ulp off)"
                         % (k, np.sqrt(e["sumsq"] / e["n"]) / e["scale"], e["max"] / e["scale"], e["ulps_top"], e["whole"] / e["n"])
                         for k, e in errs.items())
    print()
    for t0 in (0, 4, 7):
        s = {k: r[t0][k].to(torch.float32) for k in DR.STATES}
        cells = {} if t0 == 0 else {"V": s["V.c"], "E": s["E.c"]}
        start = (s["V.h"], s["V.c"] if cells else None, s["E.h"], s["E.c"] if cells else None)
        with DR.no_tf32():
            f32 = DR.trajectory(params, batch, [1], torch.float32, cuda_device, start=start, bf16=True)[1]
        f32_errs = TF.forced_step_errors(params, batch, 1, {v: torch.stack([s[v + ".h"], f32[v + ".h"]]) for v in ("V", "E")},
                                         {v: torch.stack([s[v + ".c"], f32[v + ".c"]]) for v in ("V", "E")}, bf16=True,
                                         device=cuda_device, fold=DR.INFERENCE_FOLD)
        del f32
        out = gnn({"EV": b.adj}, {"V": s["V.h"], "E": s["E.h"]}, 1, LSTM_initial_states=cells)
        torch.cuda.synchronize()
        assert out["E"].h.dtype == torch.bfloat16 and gnn.launched_loop is None
        H = {v: torch.stack([s[v + ".h"], out[v].h.to(torch.float32)]) for v in ("V", "E")}
        C = {v: torch.stack([s[v + ".c"], out[v].c]) for v in ("V", "E")}
        del out
        errs = TF.forced_step_errors(params, batch, 1, H, C, bf16=True, device=cuda_device, fold=DR.INFERENCE_FOLD)
        other = TF.forced_step_errors(params, batch, 1, H, C, bf16=True, device=cuda_device, fold=not DR.INFERENCE_FOLD)
        del H, C
        print("  [bf16 window t0=%d] %s\n    (the oracle step in float32: %s)\n    (training forward's form: %s)"
              % (t0, report(errs), report(f32_errs), report(other)))
        for k, e in errs.items():
            assert np.sqrt(e["sumsq"] / e["n"]) / e["scale"] < 0.1 * 2.0 ** -8, (t0, k, e)
            if k.endswith(".c"):
                assert e["max"] / e["scale"] < 2.0 ** -7, (t0, k, e)
            else:
                f = f32_errs[k]
                assert e["max"] / e["scale"] <= max(2 * 2.0 ** -8, 2 * f["max"] / f["scale"]), (t0, k, e, f)
