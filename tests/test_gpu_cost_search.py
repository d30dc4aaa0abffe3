"""tspgnn.get_costs -- the batched tour-cost binary search -- on the MI355X: the search kernel bitwise against a NumPy
float64 restatement of get_cost's rule, the whole search against get_cost and against the float64 oracle, its trace,
determinism across calls and chunkings, and the f16x2 range guard."""
import numpy as np
import pytest
import torch

import tspgnn
from tspgnn import _lib
from tspgnn.binary_search import cost_bounds
from oracle import params as P
from oracle import torch_oracle as TO

pytestmark = pytest.mark.gpu

NEAR = 1e-5     # a probe whose prediction is this close to the threshold may legitimately branch either way


# ---------------------------------------------------------------------------- get_cost's rule, restated in NumPy
def host_active(lo, hi, delta):
    w = (hi + lo) / 2
    return bool(lo < w * (1 - delta) or w * (1 + delta) < hi)


def host_probes(lo, hi, k):
    if k == 1:
        return np.array([(hi + lo) / 2])
    return lo + (hi - lo) * (np.arange(1, k + 1) / (k + 1.0))


def host_update(lo, hi, preds, threshold, k):
    """binary_search.py get_cost's loop body: preds float32[k] -> (lo, hi, pred)."""
    if k == 1:
        w = (hi + lo) / 2
        if preds[0:1] < threshold:
            lo = w
        else:
            hi = w
        return lo, hi, preds[0]
    probes = host_probes(lo, hi, k)
    accept = np.nonzero(preds >= threshold)[0]
    first = accept[0] if len(accept) else k
    nlo = lo if first == 0 else probes[first - 1]
    nhi = hi if first == k else probes[first]
    return float(nlo), float(nhi), preds[min(first, k - 1)]


def model_session(d, params, float_dtype=torch.float32, gemm=None):
    model = tspgnn.build_network(d, float_dtype=float_dtype)
    if gemm is not None:
        model["gnn"].gemm = gemm
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(params)
    return model, sess


def near_threshold(trace, threshold=0.5):
    return any(np.any(np.abs(r["preds"].astype(np.float64) - threshold) < NEAR) for r in trace["rounds"])


def assert_same_results(got, want, traces, label):
    """Equal wpred / iterations / route_cost, pred within 1e-6 -- except where a probe's prediction sits within NEAR of
    the threshold.  Returns the number of exempted instances."""
    exempt = 0
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[2] == float(w[2]), (label, i)
        if g[0] == float(w[0]) and g[3] == w[3]:
            if w[1] is None:
                assert g[1] is None, (label, i)
            else:
                assert g[1].dtype == np.float32 and g[1].shape == (1,)
                assert abs(float(g[1][0]) - float(w[1][0])) < 1e-6, (label, i, g[1], w[1])
            continue
        assert traces is not None and near_threshold(traces[i]), (label, i, g, w)
        exempt += 1
    return exempt


# ---------------------------------------------------------------------------- 1. the kernel, bitwise
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("threshold", [0.5, 0.7])
def test_search_kernel_matches_the_host_rule(cuda_device, k, threshold):
    rng = np.random.RandomState(100 + k)
    n, delta = 37, 0.01
    G = n * k
    m = rng.randint(1, 60, size=G)                 # ragged graphs
    seg = np.concatenate([[0], np.cumsum(m)]).astype(np.int32)
    M = int(seg[-1])
    WC0 = rng.rand(M, 2).astype(np.float32)
    lo = rng.rand(n) * 0.3
    hi = lo + rng.rand(n) * 0.5 + 1e-3
    hi[3] = lo[3] * (1 + 1e-4) if lo[3] > 0 else 1e-9   # already converged
    lo[5] = hi[5] = 0.25                                 # lo == hi
    hi[7] = lo[7] * (1 + 0.019)                          # one step from converging
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]

    def preds_for(step):
        p = rng.rand(n, k).astype(np.float32)
        thr32 = np.float32(threshold)
        p[0, :] = np.nan                                 # NaN everywhere
        p[1, :] = thr32                                  # exactly the threshold
        p[2, :] = np.float32(threshold + 0.2)            # accept at the first probe
        p[4, :] = np.float32(threshold - 0.3)            # accept none
        p[6, :] = np.sort(p[6, :])                       # monotone, crossing somewhere
        if k > 1:
            p[8, 0] = np.nan                             # NaN before an accepted probe
            p[8, 1:] = thr32
            p[9, :] = np.nextafter(thr32, np.float32(0))  # one ulp below
        return p.reshape(-1)

    dev = cuda_device
    t_lo = torch.tensor(lo, dtype=torch.float64, device=dev)
    t_hi = torch.tensor(hi, dtype=torch.float64, device=dev)
    t_it = torch.zeros(n, dtype=torch.int32, device=dev)
    t_po = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    t_na = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    t_wc = torch.from_numpy(WC0.copy()).to(dev)
    t_seg = torch.from_numpy(seg).to(dev)
    guard = torch.zeros(4, dtype=torch.int32, device=dev)

    def launch(mode, pred):
        _lib.call("tspgnn_cost_search_step", _lib.ptr(t_lo), _lib.ptr(t_hi), _lib.ptr(t_it), _lib.ptr(t_po),
                  _lib.ptr(t_na), _lib.ptr(pred), _lib.ptr(t_wc), _lib.ptr(t_seg), _lib.ptr(guard), n, k, threshold,
                  delta, mode, _lib.current_stream())
        torch.cuda.synchronize()

    # host state
    h_lo, h_hi, h_it, h_po = list(lo), list(hi), [0] * n, [np.float32(np.nan)] * n
    h_wc = WC0.copy()

    def host_write():
        for i in range(n):
            if host_active(h_lo[i], h_hi[i], delta):
                pr = host_probes(h_lo[i], h_hi[i], k).astype(np.float32)
                for j in range(k):
                    g = i * k + j
                    h_wc[seg[g]:seg[g + 1], 1] = pr[j]

    def check():
        assert np.array_equal(t_lo.cpu().numpy(), np.array(h_lo)), "lo"
        assert np.array_equal(t_hi.cpu().numpy(), np.array(h_hi)), "hi"
        assert np.array_equal(t_it.cpu().numpy(), np.array(h_it)), "iters"
        assert np.array_equal(t_po.cpu().numpy(), np.array(h_po, dtype=np.float32), equal_nan=True), "pred_out"
        wc = t_wc.cpu().numpy()
        assert np.array_equal(wc[:, 0], WC0[:, 0]), "W column written"
        assert np.array_equal(wc[:, 1], h_wc[:, 1]), "probe costs"
        assert int(t_na.item()) == sum(host_active(a, b, delta) for a, b in zip(h_lo, h_hi)), "n_active"

    launch(0, None)
    host_write()
    check()
    assert not host_active(h_lo[3], h_hi[3], delta) and not host_active(h_lo[5], h_hi[5], delta)
    for step in range(6):
        preds = preds_for(step)
        t_pred = torch.from_numpy(preds).to(dev)
        if step == 2:                  # a flagged round (range bits, then a loop timeout) changes nothing
            for word, val in ((0, 1), (0, 2), (2, 5)):
                guard.zero_()
                guard[word] = val
                launch(1, t_pred)
                check()
            guard.zero_()
        before_inactive = [i for i in range(n) if not host_active(h_lo[i], h_hi[i], delta)]
        launch(1, t_pred)
        p = preds.reshape(n, k)
        for i in range(n):
            if host_active(h_lo[i], h_hi[i], delta):
                h_lo[i], h_hi[i], h_po[i] = host_update(h_lo[i], h_hi[i], p[i], threshold, k)
                h_it[i] += 1
        host_write()
        check()
        for i in before_inactive:      # inactive instances are never touched again
            assert h_it[i] == int(t_it[i].item())
    assert h_it[3] == 0 and h_it[5] == 0 and max(h_it) >= 2


# ---------------------------------------------------------------------------- 2. end to end against get_cost
def small_instances(count, seed, n_lo=9, n_hi=40):
    rng = np.random.RandomState(seed)
    sizes = np.linspace(n_lo, n_hi, count).astype(int)
    return [tspgnn.random_instance(int(s), rng) for s in sizes]


@pytest.mark.parametrize("parallel", [1, 4])
def test_get_costs_matches_get_cost(cuda_device, parallel):
    d, T = 32, 3
    model, sess = model_session(d, P.init_params(d, seed=12, perturb=True))
    insts = small_instances(24, seed=5)
    got, traces = tspgnn.get_costs(sess, model, insts, T, parallel=parallel, trace=True)
    want = [tspgnn.get_cost(sess, model, x, T, parallel=parallel) for x in insts]
    exempt = assert_same_results(got, want, traces, "parallel=%d" % parallel)
    print("get_costs vs get_cost, parallel=%d: %d of %d instances exempted (a prediction within %g of the threshold)"
          % (parallel, exempt, len(insts), NEAR))
    assert exempt <= 3
    assert all(r[3] > 0 for r in got)


# ---------------------------------------------------------------------------- 3. the trace
@pytest.mark.parametrize("parallel", [1, 3])
def test_trace_is_consistent(cuda_device, parallel):
    d, T, k = 32, 3, parallel
    model, sess = model_session(d, P.init_params(d, seed=12, perturb=True))
    insts = small_instances(10, seed=8)
    got, traces = tspgnn.get_costs(sess, model, insts, T, parallel=parallel, trace=True)
    for (Ma, Mw, route), res, tr in zip(insts, got, traces):
        lo, hi = [float(x) for x in cost_bounds(Mw, Ma.shape[0])]
        assert tr["bounds"] == (lo, hi)
        pred = None
        for r in tr["rounds"]:
            assert host_active(lo, hi, 0.01)
            assert np.array_equal(r["probes"], host_probes(lo, hi, k).astype(np.float32))
            lo, hi, pred = host_update(lo, hi, r["preds"], 0.5, k)
            assert (r["lo"], r["hi"]) == (lo, hi)
        assert not host_active(lo, hi, 0.01)
        assert res[3] == len(tr["rounds"]) and res[0] == (hi + lo) / 2
        assert res[1] is not None and res[1][0] == pred
    # the recorded predictions are what a plain forward of the recorded probe costs gives
    for i in (0, 4, 9):
        Ma = insts[i][0]
        m = len(np.nonzero(Ma)[0])
        for r in traces[i]["rounds"]:
            EV, W, _, re_, nv, ne = tspgnn.InstanceLoader.create_batch([insts[i]] * k, target_cost=0.0)
            C = np.repeat(r["probes"].astype(np.float64), m).reshape(-1, 1)
            feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: re_,
                    model["n_vertices"]: nv, model["n_edges"]: ne}
            p = sess.run(model["predictions"], feed_dict=feed)
            assert np.abs(p.astype(np.float64) - r["preds"]).max() < 1e-6


# ---------------------------------------------------------------------------- 4. determinism, chunking, max_rounds
def test_deterministic_and_chunk_independent(cuda_device):
    d, T, k = 32, 3, 4
    model, sess = model_session(d, P.init_params(d, seed=12, perturb=True))
    insts = small_instances(24, seed=11)
    a, traces = tspgnn.get_costs(sess, model, insts, T, parallel=k, trace=True)
    b = tspgnn.get_costs(sess, model, insts, T, parallel=k)

    def same(x, y):
        return all(p[0] == q[0] and p[2] == q[2] and p[3] == q[3]
                   and ((p[1] is None and q[1] is None) or np.array_equal(p[1], q[1])) for p, q in zip(x, y))

    assert same(a, b)
    chunked = tspgnn.get_costs(sess, model, insts, T, parallel=k, max_graphs=32)   # 8 instances per chunk: 3 chunks
    assert len(tspgnn.binary_search.plan_chunks(len(insts), k, 32)) >= 3
    assert assert_same_results(chunked, a, traces, "chunked") == 0
    assert same(tspgnn.get_costs(sess, model, insts, T, parallel=k, max_rounds=500), a)
    with pytest.raises(RuntimeError, match="still open after max_rounds=1"):
        tspgnn.get_costs(sess, model, insts, T, parallel=k, max_rounds=1)


# ---------------------------------------------------------------------------- 5. the f16x2 range guard
def test_range_guard_runs_the_search_on_bf16x3(cuda_device):
    d, T = 64, 3
    params = P.init_params(d, seed=5, perturb=True)
    key = [x for x in params if x.endswith("E_msg_V_MLP_layer_3/bias")]
    assert len(key) == 1
    params[key[0]] = np.full_like(params[key[0]], 3000.0)
    rng = np.random.RandomState(0)
    insts = [tspgnn.random_instance(n, rng) for n in (20, 40, 20, 40, 20, 40)]
    model, sess = model_session(d, params)
    assert model["gnn"].active_arith() == "h2"
    got = tspgnn.get_costs(sess, model, insts, T, parallel=2)
    assert sess.last_range_bits & 1
    assert not sess.range_exceeded()
    model_x3, sess_x3 = model_session(d, params, gemm="bf16x3")
    want = tspgnn.get_costs(sess_x3, model_x3, insts, T, parallel=2)
    assert sess_x3.last_range_bits == 0
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[2] == w[2] and g[3] == w[3] and np.array_equal(g[1], w[1])
        assert np.all(np.isfinite(g[1]))


# ---------------------------------------------------------------------------- 6. the float64 oracle
def test_matches_the_float64_oracle_loop(cuda_device):
    d, T = 32, 3
    params = P.init_params(d, seed=12, perturb=True)
    model, sess = model_session(d, params)
    rng = np.random.RandomState(5)
    insts = [tspgnn.random_instance(n, rng) for n in (9, 11, 12)]
    got = tspgnn.get_costs(sess, model, insts, T)
    tp = TO.to_torch(params, torch.float64)
    for inst, res in zip(insts, got):
        Ma, Mw, route = inst
        n = Ma.shape[0]
        wmin, wmax = cost_bounds(Mw, n)
        EV, W, _, r, nv, ne = tspgnn.InstanceLoader.create_batch([inst], target_cost=0.0)
        w, it = (wmin + wmax) / 2, 0
        while wmin < w * 0.99 or w * 1.01 < wmax:
            b = {"ev_uv": EV.uv, "W": W, "C": np.ones_like(W) * w, "route_exists": r, "n_vertices": nv, "n_edges": ne}
            p = TO.forward(tp, b, T)["predictions"].item()
            if p < 0.5:
                wmin = w
            else:
                wmax = w
            w, it = (wmin + wmax) / 2, it + 1
        assert res[3] == it and abs(res[0] - w) < 1e-12 and 0 < it < 40


# ---------------------------------------------------------------------------- 7. the experiment's shape
def test_experiment_shape(cuda_device):
    """experiments/binary_search.py's shape: d = 64, T = 32, n in [20, 40]."""
    d, T = 64, 32
    model, sess = model_session(d, P.init_params(d, seed=3, perturb=True))
    rng = np.random.RandomState(21)
    insts = [tspgnn.random_instance(int(n), rng) for n in rng.randint(20, 41, size=64)]
    got, traces = tspgnn.get_costs(sess, model, insts, T, trace=True)
    assert len(got) == 64 and all(r[3] > 0 and np.isfinite(r[0]) for r in got)
    idx = list(range(0, 64, 8))
    want = [tspgnn.get_cost(sess, model, insts[i], T) for i in idx]
    exempt = assert_same_results([got[i] for i in idx], want, [traces[i] for i in idx], "d=64 T=32")
    print("experiment shape: %d of %d exempted" % (exempt, len(idx)))
    assert exempt <= 2


def test_bf16_storage_model(cuda_device):
    d, T = 128, 4
    # (seed 3: an untrained network whose answer crosses the threshold inside the bracket -- one that says "yes" to every
    # cost drives the upper end to the bracket's lower end, 0, through ~1 000 bisections, as get_cost would)
    model, sess = model_session(d, P.init_params(d, seed=3, perturb=True), float_dtype=torch.bfloat16)
    rng = np.random.RandomState(22)
    insts = [tspgnn.random_instance(n, rng) for n in (20, 27, 33, 40)]
    got, traces = tspgnn.get_costs(sess, model, insts, T, parallel=2, trace=True)
    want = [tspgnn.get_cost(sess, model, x, T, parallel=2) for x in insts]
    exempt = assert_same_results(got, want, traces, "bf16 storage")
    print("bf16 storage: %d of %d exempted" % (exempt, len(insts)))
    assert exempt <= 2
