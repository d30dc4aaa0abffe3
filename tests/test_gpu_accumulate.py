"""Gradient accumulation on the device: tspgnn_bucket_accumulate_f32 bit for bit against a NumPy
float32 restatement, the accumulated gradient and three accumulated optimiser steps against the float64 oracle of the UNION
batch, and the step's own contracts -- K = 1 is train_step where the scalings are exact, the captured form equals the
eager one, a flagged micro-batch repeats the whole step.  The arithmetic without a GPU: tests/test_accumulate_host.py."""
import functools

import numpy as np
import pytest
import torch

import tspgnn
from tspgnn import _lib
from conftest import load_pack
from oracle import params as P
from oracle import torch_oracle as TO
from test_dp_gloo import _shard
from test_gpu_model import MOVE_TOL, MOVE_TOL_BY_CLASS, REL_TOL, _low_end_params

pytestmark = pytest.mark.gpu

TAIL = 10
STAT_KEYS = ("loss", "acc", "TP", "FP", "TN", "FN")


# --------------------------------------------------------------------------------- 1. tspgnn_bucket_accumulate_f32
def _tail_of(B, stats, flag):
    """The ten tail values bucket_pack_kernel writes for a rank (here: a micro-batch) of B graphs, in float32."""
    v = np.zeros(TAIL, dtype=np.float32)
    v[0] = B
    if stats is not None:
        v[1:3] = np.float32(B) * stats[0:2]
        v[3:7] = stats[2:6]
    if flag is not None:
        v[7:10] = [(flag >> k) & 1 for k in range(3)]
    return v


@pytest.mark.parametrize("with_flag", [False, True], ids=["flag-null", "flag-0b101-in-call-2"])
@pytest.mark.parametrize("with_stats", [False, True], ids=["stats-null", "stats"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 115529, 262147])
def test_accumulate_kernel_bit_for_bit(cuda_device, n, with_stats, with_flag):
    """Three calls with batch sizes 2, 3, 5 (not all powers of two: the product's rounding matters, and so does its being
    rounded apart from the sum).  n = 115 529 is d = 64's parameter count, 262 147 lies past 1024 workgroups x 256 threads:
    the grid-stride loop's second trip.  The restatement: acc = acc + np.float32(B) * g on float32 arrays."""
    rng = np.random.RandomState(n % 1000 + 2 * with_stats + with_flag)
    accum = torch.full((n + TAIL,), float("nan"), device=cuda_device)           # `first` must WRITE
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    want = np.full(n + TAIL, np.nan, dtype=np.float32)
    for call, B in enumerate((2.0, 3.0, 5.0)):
        g = (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-4, 4, size=n)).astype(np.float32)
        stats = np.array([rng.uniform(0.3, 0.9), rng.uniform(0.2, 1.0)] + list(rng.randint(0, 7, size=4)),
                         dtype=np.float32) if with_stats else None
        word = (0b101 if call == 1 else 0) if with_flag else None
        if with_flag:
            flag.fill_(word)
        g_dev = torch.from_numpy(g).to(cuda_device)
        s_dev = torch.from_numpy(stats).to(cuda_device) if with_stats else None
        _lib.call("tspgnn_bucket_accumulate_f32", _lib.ptr(accum), _lib.ptr(g_dev) if n else None, n, int(call == 0), B,
                  _lib.ptr(s_dev), _lib.ptr(flag) if with_flag else None, _lib.current_stream())
        term = np.concatenate([np.float32(B) * g, _tail_of(B, stats, word)])
        want = term if call == 0 else want + term
        assert want.dtype == np.float32
        got = accum.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (call, np.flatnonzero(got != want)[:5])
        assert np.array_equal(g_dev.cpu().numpy().view(np.uint32), g.view(np.uint32))     # grad is only read
    # tspgnn_bucket_unpack_f32 finishes the step: inv = 1.0f / tail[0], then a multiply
    st_out = torch.full((6,), -1.0, device=cuda_device)
    fl_out = torch.full((1,), 7, dtype=torch.int32, device=cuda_device)
    _lib.call("tspgnn_bucket_unpack_f32", _lib.ptr(accum), n, 1, _lib.ptr(st_out), _lib.ptr(fl_out), _lib.current_stream())
    assert want[n] == 10.0
    inv = np.float32(1) / np.float32(10)
    got = accum.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), (want[:n] * inv).view(np.uint32))
    assert np.array_equal(st_out.cpu().numpy(), np.concatenate([want[n + 1:n + 3] * inv, want[n + 3:n + 7]]))
    assert int(fl_out.item()) == (0b101 if with_flag else 0)


def test_accumulate_kernel_argument_checks(cuda_device):
    """TSPGNN_EINVAL, and nothing launched: a NULL accumulator, a negative n, a NULL gradient with n > 0, and the
    accumulator as its own gradient."""
    n = 300
    accum = torch.full((n + TAIL,), 3.0, device=cuda_device)
    grad = torch.full((n,), 1.0, device=cuda_device)
    fn = _lib.lib.tspgnn_bucket_accumulate_f32
    for a, g, count in ((None, grad, n), (accum, grad, -1), (accum, None, n), (accum, accum, n)):
        assert fn(_lib.ptr(a), _lib.ptr(g), count, 0, 2.0, None, None, _lib.current_stream()) == -1
        assert b"bucket_accumulate" in _lib.lib.tspgnn_last_error()
    torch.cuda.synchronize()
    assert bool((accum == 3.0).all()) and bool((grad == 1.0).all())
    assert fn(_lib.ptr(accum), None, 0, 1, 2.0, None, None, _lib.current_stream()) == 0       # n == 0: the tail only
    torch.cuda.synchronize()
    assert accum[:TAIL].tolist() == [2.0] + [0.0] * 9 and bool((accum[TAIL:] == 3.0).all())


# --------------------------------------------------------------------------------- the step
def _tuple(g, lo, hi):
    s = _shard(g, lo, hi)
    return (tspgnn.SparseEV(s["ev_uv"], int(s["n_vertices"].sum())), s["W"], s["C"], s["route_exists"], s["n_vertices"],
            s["n_edges"])


def _feed(model, t, T):
    EV, W, C, route_exists, n_vertices, n_edges = t
    return {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}


def _session(d, params, float_dtype=torch.float32):
    model = tspgnn.build_network(d, float_dtype=float_dtype)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(params)
    return model, sess


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, pack_seed, d, param_seed, T, lo, hi):
    """Of graphs lo .. hi-1 of a golden pack: (float64 outputs, float64 gradients less the L2 term, the op-for-op fp32
    autograd run's distance from float64 per variable) -- the two ingredients of test_gradient_parity's bar."""
    params = P.init_params(d, seed=param_seed, perturb=True)
    batch = _shard(load_pack(name, pack_seed), lo, hi)
    out, g64 = TO.loss_and_grads(params, batch, T, dtype=torch.float64)
    _, g32 = TO.loss_and_grads(params, batch, T, dtype=torch.float32, dense=True)
    ref = {k: g64[k] - TO.L2NORM_SCALING * params[k] for k in g64}
    dist32 = {k: float(np.abs(g32[k] - g64[k]).max()) for k in g64}
    return {k: float(out[k].detach()) for k in STAT_KEYS}, ref, dist32


@pytest.mark.parametrize("name,d,T,split", [("ragged_B6", 64, 4, [0, 2, 6]), ("ragged_B6", 64, 4, [0, 1, 4, 6]),
                                            ("n5_B2", 32, 3, [0, 1, 2])])
def test_accumulated_gradient_against_the_union_batch_oracle(cuda_device, name, d, T, split):
    """HIP backward per micro-batch + accumulate + unpack against the float64 oracle of the whole batch.  The bar is
    test_gradient_parity_with_autograd_oracle's, carried through the linear combination g = Σ_k (B_k / B) g_k, plus the
    accumulation's own roundings: with scale_k and err32_k formed per micro-batch as that test forms them,
        |g[v] - ref[v]| < Σ_k (B_k / B) max(1e-5, 2 err32_k[v]) scale_k[v] + K 2^-23 Σ_k (B_k / B) max|g_k[v]|."""
    pack = load_pack(name, 1)
    params = P.init_params(d, seed=21, perturb=True)
    model, sess = _session(d, params)
    bounds = list(zip(split[:-1], split[1:]))
    K, B = len(bounds), split[-1]
    bar = {k: 0.0 for k in params}
    rounding = {k: 0.0 for k in params}
    for k, (lo, hi) in enumerate(bounds):
        out = sess.loss_and_grads(_feed(model, _tuple(pack, lo, hi), T))
        sess.accumulate_grads(hi - lo, out["stats"], first=(k == 0))
        _, ref_k, dist32 = _oracle_grads(name, 1, d, 21, T, lo, hi)
        gscale = max(np.abs(r).max() for r in ref_k.values())
        for v in ref_k:
            scale = max(np.abs(ref_k[v]).max(), 1e-3 * gscale)
            bar[v] += (hi - lo) / B * max(1e-5, 2 * dist32[v] / scale) * scale
            rounding[v] += (hi - lo) / B * np.abs(ref_k[v]).max()
    stats = out["stats"]
    sess.reduce_accumulated(stats)
    torch.cuda.synchronize()
    got = model.store.grad_dict()
    want_out, want, _ = _oracle_grads(name, 1, d, 21, T, 0, B)
    worst = 0.0
    for v in want:
        err = np.abs(got[v] - want[v]).max()
        limit = bar[v] + K * 2.0 ** -23 * rounding[v]
        worst = max(worst, err / limit)
        assert err < limit, (v, err, limit)
    print("\n[%s d=%d T=%d split %s] worst accumulated-gradient error / bar: %.2f" % (name, d, T, split, worst))
    stats = stats.cpu().numpy()
    assert abs(float(stats[0]) - want_out["loss"]) < REL_TOL
    for i, key in enumerate(STAT_KEYS[1:], 1):
        assert float(stats[i]) == want_out[key], key


def test_three_accumulated_steps_follow_the_oracle(cuda_device):
    """test_train_steps_follow_the_oracle with every step taken over the split [0, 2, 6] of its batch: the oracle's
    train_step sees the whole batch."""
    d, T = 64, 4
    pack = load_pack("ragged_B6", 0)
    params = P.init_params(d, seed=2, perturb=True)
    model, sess = _session(d, params)
    feeds = [_feed(model, _tuple(pack, lo, hi), T) for lo, hi in ((0, 2), (2, 6))]
    batch = _shard(pack, 0, 6)
    p = {k: v.copy() for k, v in params.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(v) for k, v in p.items()}
    for step in (1, 2, 3):
        out = sess.train_step_accumulated(feeds)
        ref_out, p, m, v, gn = TO.train_step(p, batch, T, m, v, step)
        assert abs(float(out["stats"][0].item()) - ref_out["loss"].item()) < REL_TOL
        assert abs(float(out["global_norm"].item()) - gn) < 2e-5 * gn
        assert len(out["predictions"]) == 2 and [b.B for b in out["batches"]] == [2, 4]
    assert int(sess._adam["t"].item()) == 3 and sess._adam["step"] == 3
    now = model.store.state_dict()
    for k in p:
        moved_ref = p[k] - params[k]
        moved = now[k].astype(np.float64) - params[k]
        klass = k.rsplit("/", 1)[-1] if "/" in k else k
        ratio = np.abs(moved - moved_ref).max() / np.abs(moved_ref).max()
        assert np.abs(moved - moved_ref).max() < 2e-7 + MOVE_TOL_BY_CLASS.get(klass, MOVE_TOL) * np.abs(moved_ref).max(), (k, ratio)


@pytest.mark.parametrize("float_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16-storage"])
def test_one_micro_batch_is_train_step_at_a_power_of_two(cuda_device, float_dtype):
    """K = 1, B = 4: B * g and the product with 1 / B are exact, so the accumulated step IS train_step -- variables, losses
    and Adam's moments bit for bit after two steps."""
    d, T = 64, 3
    t = _tuple(load_pack("sparse_B4", 0), 0, 4)
    params = P.init_params(d, seed=7, perturb=True)
    ends = []
    for accumulated in (False, True):
        model, sess = _session(d, params, float_dtype)
        b = sess.prepare(_feed(model, t, T))
        assert b.B == 4
        before = model.store.theta.clone()
        losses = []
        for _ in range(2):
            out = sess.train_step_accumulated([b]) if accumulated else sess.train_step(b)
            losses.append(float(out["stats"][0].item()))
        torch.cuda.synchronize()
        ends.append((model.store.theta.clone(), losses, sess._adam["m"].clone(), sess._adam["v"].clone(),
                     int(sess._adam["t"].item()), sess._adam["step"]))
    plain, acc = ends
    assert plain[1] == acc[1] and plain[4] == acc[4] == 2 and plain[5] == acc[5] == 2
    for i in (0, 2, 3):
        assert torch.equal(plain[i], acc[i]), i
    assert not torch.equal(plain[0], before)


def test_captured_accumulation_equals_eager_with_refilled_micro_batches(cuda_device):
    """capture_train_step(b, micro_batches=3): graph A three times over batches written into b's buffers, one accumulate
    launch behind each, then hand-over, unpack and graph B -- the trajectory of eager train_step_accumulated on freshly
    gathered batches, bit for bit.  A refill of another shape is refused by batch(out=) before anything is applied."""
    d, T = 32, 3
    rng = np.random.RandomState(12)
    ds = tspgnn.DeviceDataset([tspgnn.random_instance(6, rng) for _ in range(8)], device=cuda_device)
    ids = ([0, 0, 1, 1], [2, 2, 3, 3], [4, 4, 5, 5])
    params = P.init_params(d, seed=3, perturb=True)
    ends = []
    for captured in (False, True):
        model, sess = _session(d, params)
        losses = []
        if captured:
            b = ds.batch(ids[0], time_steps=T)
            step = sess.capture_train_step(b, micro_batches=3)
            refill = lambda k: ds.batch(ids[k], time_steps=T, out=b)     # noqa: E731
        for _ in range(3):
            out = step(refill) if captured else sess.train_step_accumulated([ds.batch(i, time_steps=T) for i in ids])
            losses.append(float(out["stats"][0].item()))
        torch.cuda.synchronize()
        ends.append((model.store.theta.clone(), losses, int(sess._adam["t"].item()), sess._adam["step"]))
    assert ends[0][2] == ends[1][2] == 3 and ends[0][3] == ends[1][3] == 3
    assert ends[0][1] == ends[1][1]
    assert torch.equal(ends[0][0], ends[1][0])
    assert len(set(ends[0][1])) == 3              # (the steps moved the variables: three different losses)
    with pytest.raises(ValueError, match="instance sizes"):
        step(lambda k: ds.batch([0, 0, 1], time_steps=T, out=b))
    torch.cuda.synchronize()
    assert int(sess._adam["t"].item()) == 3 and sess._adam["step"] == 3 and torch.equal(model.store.theta, ends[1][0])


def test_a_flagged_micro_batch_repeats_the_whole_step(cuda_device):
    """Variables whose cell inputs sit under the f16x2 split's variance floor (test_variance_floor_routes_a_tiny_z_to_bf16x3):
    the optimiser kernel skips the accumulated step, train_step_accumulated repeats it from its first micro-batch on
    bf16x3 -- ONE step is applied, and it is the step a session takes that was on bf16x3 from the start."""
    d, T = 64, 6
    pack = load_pack("ragged_B6", 1)
    params = _low_end_params("d", d, 31)
    ends = []
    for forced in (False, True):
        model, sess = _session(d, params)
        feeds = [_feed(model, _tuple(pack, lo, hi), T) for lo, hi in ((0, 2), (2, 6))]
        before = model.store.theta.clone()
        if forced:
            with model["gnn"].forced_off_h2():
                sess.train_step_accumulated(feeds)
            assert sess.last_range_bits == 0
        else:
            assert model["gnn"].active_arith() == "h2"
            sess.train_step_accumulated(feeds)
            assert sess.last_range_bits != 0
        torch.cuda.synchronize()
        assert int(sess._adam["t"].item()) == 1 and sess._adam["step"] == 1
        ends.append(model.store.theta.clone())
    assert torch.equal(ends[0], ends[1]) and not torch.equal(ends[0], before)
