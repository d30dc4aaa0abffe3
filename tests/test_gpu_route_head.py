"""The route head on the GPU (csrc/route_head.hip, tspgnn/route_head.py, build_network(d, route_head=True)).

  1. tspgnn_route_edge_marks against route_edge_marks_host, exactly, on one ragged batch and at the LDS table's limit.
  2. tspgnn_edge_bce_f32 against the float64 restatement, with the bars tests/test_gpu_kernels.py puts on tspgnn_bce_metrics_f32
     (np.allclose(rtol=1e-6, atol=1e-7) on the statistics) and tests/test_gpu_backward_kernels.py on tspgnn_vote_grad_f32
     (rel_err < 1e-6 on the gradient): the same arithmetic, the same bars.  Two launches bit for bit.
  3. Every variable's gradient and both losses against tests/route_head_reference.py (the oracle plus the head), with the bars
     of tests/test_gpu_model.py: fp32 storage -- per variable max(1e-5, twice what an op-for-op fp32 autograd run loses), both
     losses within 1e-5; bf16 storage -- both losses within 5e-4 and the gradient's L2 distance from the oracle's own bf16
     forward within 3 max(spread under a 1e-6 nudge, 1e-2) (test_bf16_storage_training_gradients' end-to-end bar; its
     teacher-forced bar needs oracle/teacher_forced.py, which knows no second head, and is not restated here).
  4. A network without the head is what it was: bit-identical gradients next to route_head=True, route_loss=0, and the
     launches of tests/golden/route_head_launch_names.json.
  5. capture_train_step, DeviceDataset(routes=True), train_step_accumulated.
  6. Forty steps on one batch lower the route loss; the decoders take votes="route".
"""
import json
import os

import numpy as np
import pytest
import torch

import tspgnn
from conftest import GOLDEN, batch_from_tuple, rel_err
from tspgnn import _lib, route_edge_marks_host
from tspgnn import route_head as RH

import route_head_reference as REF
from test_route_head_host import sparse_n12

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5     # tests/test_gpu_model.py
FEED_KEYS = ("EV", "W", "C", "route_exists", "n_vertices", "n_edges")


def dev(a, device, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def feed_of(model, t, T, marks=None):
    feed = {model[k]: v for k, v in zip(FEED_KEYS, t)}
    feed[model["time_steps"]] = T
    if marks is not None:
        feed[model["route_edges"]] = marks
    return feed


def complete_instance(n, rng):
    Ma, Mw, _ = tspgnn.random_instance(n, rng)
    return Ma, Mw, [int(v) for v in rng.permutation(n)]


# ------------------------------------------------------------------------------------------- 1. tspgnn_route_edge_marks
def ragged_instances():
    rng = np.random.RandomState(17)
    out = [complete_instance(n, rng) for n in (3, 4, 5, 7)]
    Ma, Mw, _ = sparse_n12()
    out.append((Ma, Mw, [int(v) for v in rng.permutation(12)]))          # a random tour on the sparse graph: pairs missing
    out += [complete_instance(n, rng) for n in (40, 256)]
    return out


def resident(instances, device, T=2):
    model = tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=True)
    sess = tspgnn.Session(model, device=device)
    return sess, sess.prepare(feed_of(model, tspgnn.InstanceLoader.create_batch(instances), T))


def test_marks_kernel_equals_the_host_function(cuda_device):
    instances = ragged_instances()
    want, want_missing = route_edge_marks_host(instances)
    assert [int(np.count_nonzero(i[0])) for i in instances] == [3, 6, 10, 21, 15, 780, 32640]
    assert want_missing[4] > 0 and not want_missing[[0, 1, 2, 3, 5, 6]].any()
    sess, b = resident(instances, cuda_device)
    b.route_edges = torch.full((b.M,), float("nan"), device=cuda_device)      # every entry must be written
    marks_buffer = b.route_edges
    missing = sess.mark_routes(b, [i[2] for i in instances])
    assert b.route_edges is marks_buffer
    got = b.route_edges.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(missing, want_missing)
    # the (array, offsets) form, into the same buffer
    flat = np.concatenate([i[2] for i in instances]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(i[2]) for i in instances])])
    b.route_edges.fill_(float("nan"))
    assert np.array_equal(sess.mark_routes(b, (flat, off)), want_missing)
    assert np.array_equal(b.route_edges.cpu().numpy(), want)


def test_marks_refuse_a_non_permutation_by_name(cuda_device):
    instances = ragged_instances()[:4]
    sess, b = resident(instances, cuda_device)
    tours = [i[2] for i in instances]
    bad = [list(t) for t in tours]
    bad[2][4] = bad[2][0]                                   # instance 2 visits a vertex twice
    with pytest.raises(ValueError, match="instance 2"):
        sess.mark_routes(b, bad)
    # the kernel's own answer to the same tour (its status word; no table entry is written twice, nothing out of bounds):
    # the problem's marks are zeros, the others are unaffected
    flat = torch.from_numpy(np.concatenate(bad).astype(np.int32)).to(cuda_device)
    b.route_edges = torch.full((b.M,), float("nan"), device=cuda_device)
    n_missing, status = RH.launch_marks(b, flat)
    want, want_missing = route_edge_marks_host(instances[:2] + [(instances[2][0], instances[2][1], tours[2])] + instances[3:])
    seg = np.concatenate([[0], np.cumsum(b.n_edges)])
    want[seg[2]:seg[3]] = 0
    want_missing[2] = -1
    assert status.cpu().tolist() == [0, 0, 1, 0]
    assert np.array_equal(b.route_edges.cpu().numpy(), want) and np.array_equal(n_missing.cpu().numpy(), want_missing)


def test_marks_kernel_at_the_table_limit(cuda_device):
    """n = 16384, the largest position table (64 KB of LDS plus the pair bits: the launch raises its dynamic-LDS limit), on a
    sparse graph -- a ring and 4n random chords -- beside a small instance; one more vertex is refused before any launch."""
    n, rng = RH.MAX_N, np.random.RandomState(4)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    chords = rng.randint(0, n, size=(4 * n, 2))
    uv_big = np.concatenate([ring, chords[chords[:, 0] != chords[:, 1]]])
    uv_big = uv_big[rng.permutation(len(uv_big))]
    small = complete_instance(5, rng)
    su, sv = np.nonzero(small[0])
    uv = np.concatenate([uv_big, np.stack([su, sv], axis=1) + n]).astype(np.int32)
    n_edges, n_vertices = np.array([len(uv_big), len(su)]), np.array([n, 5])
    model = tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=True)
    sess = tspgnn.Session(model, device=cuda_device)
    M = len(uv)
    t = (tspgnn.SparseEV(uv, n + 5), rng.rand(M, 1), rng.rand(M, 1), np.array([0, 1]), n_vertices, n_edges)
    b = sess.prepare(feed_of(model, t, 1), remember_adjacency=False)
    # the tour: the ring with a random rotation and a few transpositions, so that most of its pairs are edges and some not
    tour = np.roll(np.arange(n), 1234)
    for i in rng.randint(0, n - 1, size=50):
        tour[[i, i + 1]] = tour[[i + 1, i]]
    pairs = {frozenset((int(a), int(c))) for a, c in zip(tour, np.roll(tour, -1))}
    edges = [frozenset((int(a), int(c))) for a, c in uv_big]
    want_big = np.array([1.0 if e in pairs and len(e) == 2 else 0.0 for e in edges], dtype=np.float32)
    want_missing = len(pairs - set(edges))
    small_marks, small_missing = route_edge_marks_host([small])
    b.route_edges = torch.full((b.M,), float("nan"), device=cuda_device)
    missing = sess.mark_routes(b, [tour, small[2]])
    got = b.route_edges.cpu().numpy()
    assert 0 < want_missing < n and want_big.sum() >= n - want_missing
    assert np.array_equal(got[:len(uv_big)], want_big) and np.array_equal(got[len(uv_big):], small_marks)
    assert missing.tolist() == [want_missing, int(small_missing[0])]
    with pytest.raises(_lib.TspgnnError, match="n_max=16385 exceeds 16384"):
        _lib.call("tspgnn_route_edge_marks", 1, 1, 1, 1, None, 1, RH.MAX_N + 1, 1, 1, 1, None)
    with pytest.raises(_lib.TspgnnError, match="at least 3"):
        _lib.call("tspgnn_route_edge_marks", 1, 1, 1, 1, None, 1, 2, 1, 1, 1, None)


# ------------------------------------------------------------------------------------------------ 2. tspgnn_edge_bce_f32
def bce_case():
    rng = np.random.RandomState(23)
    n_edges = np.array([1, 6, 255, 256, 780])
    seg = REF.segments(n_edges)
    M = int(seg[-1])
    x = rng.uniform(-8, 8, size=M).astype(np.float32)
    y = (rng.rand(M) < 0.15).astype(np.float32)
    y[0] = 1.0                      # m = 1, its one edge marked: balanced weight (1 - 1) / 1 = 0
    y[seg[2]:seg[3]] = 0.0          # a problem without a marked edge: k = 0
    at = seg[4] + np.arange(6)      # planted: +-40 and 0 on marked and unmarked edges
    x[at] = [40.0, -40.0, 0.0, 40.0, -40.0, 0.0]
    y[at] = [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    return n_edges, seg.astype(np.int32), x, y


@pytest.mark.parametrize("pos_weight", [3.0, None], ids=["pos_weight-3", "balanced"])
def test_edge_bce_kernel_against_float64(cuda_device, pos_weight):
    n_edges, seg, x, y = bce_case()
    B, M, scale = len(n_edges), len(x), 0.25
    want_stats, want_d = REF.edge_bce(x, y, n_edges, pos_weight, scale)
    xd, yd, sd = dev(x, cuda_device), dev(y, cuda_device), dev(seg, cuda_device, np.int32)
    runs = []
    for _ in range(2):
        buf = torch.full((M + 8,), float("nan"), device=cuda_device)
        dlogit = buf[4:4 + M]
        stats = torch.full((6,), float("nan"), device=cuda_device)
        ws = _lib.workspace("tspgnn_edge_bce_workspace_floats", B, device=cuda_device)
        _lib.call("tspgnn_edge_bce_f32", _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(sd), B, 0.0 if pos_weight is None else pos_weight,
                  scale, _lib.ptr(dlogit), _lib.ptr(stats), _lib.ptr(ws), None)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + M:]).all())
        runs.append((stats.cpu().numpy(), dlogit.cpu().numpy()))
    (stats, dlogit), (stats2, dlogit2) = runs
    print("\n[edge_bce %s] stats %s\n  float64 %s\n  dlogit rel err %.2e" % (pos_weight, stats, want_stats,
                                                                          rel_err(dlogit, want_d)))
    assert np.array_equal(stats.view(np.uint32), stats2.view(np.uint32))
    assert np.array_equal(dlogit.view(np.uint32), dlogit2.view(np.uint32))
    assert np.allclose(stats, want_stats, rtol=1e-6, atol=1e-7)
    assert rel_err(dlogit, want_d) < 1e-6
    assert stats[2] + stats[3] + stats[4] + stats[5] == M and np.array_equal(stats[2:], want_stats[2:])
    # the statistics alone (dlogit NULL) are the same numbers
    only = torch.empty(6, device=cuda_device)
    _lib.call("tspgnn_edge_bce_f32", _lib.ptr(xd), _lib.ptr(yd), _lib.ptr(sd), B, 0.0 if pos_weight is None else pos_weight,
              scale, None, _lib.ptr(only), _lib.ptr(ws), None)
    assert np.array_equal(only.cpu().numpy().view(np.uint32), stats.view(np.uint32))


# --------------------------------------------------------------------------------------- 3. gradient parity end to end
def parity_case():
    rng = np.random.RandomState(31)
    instances = [tspgnn.random_instance(n, rng) for n in (5, 6, 8, 12)]
    t = tspgnn.InstanceLoader.create_batch(instances)
    return instances, t, route_edge_marks_host(instances)[0]


def route_session(d, params, float_dtype=torch.float32, **kw):
    model = tspgnn.build_network(d, store=tspgnn.VariableStore(), float_dtype=float_dtype, route_head=True, **kw)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(params)
    return model, sess


@pytest.mark.parametrize("lam", [1.0, 0.25])
@pytest.mark.parametrize("d", [32, 64])
def test_gradient_parity_with_the_reference(cuda_device, d, lam):
    T = 3
    _, t, marks = parity_case()
    params = REF.route_params(d, seed=21)
    model, sess = route_session(d, params, route_loss=lam)
    out = sess.loss_and_grads(feed_of(model, t, T, marks))
    torch.cuda.synchronize()
    g = model.store.grad_dict()
    batch = batch_from_tuple(t)
    ref_out, ref_g = REF.loss_and_grads(params, batch, marks, T, lam=lam)
    _, f32_g = REF.loss_and_grads(params, batch, marks, T, lam=lam, dtype=torch.float32, dense=True)
    stats, rstats = out["stats"].cpu().numpy(), out["route_stats"].cpu().numpy()
    print("\n[d=%d lam=%g] loss %.7f (ref %.7f)  route_loss %.7f (ref %.7f)"
          % (d, lam, stats[0], ref_out["loss"].item(), rstats[0], ref_out["route_loss"].item()))
    assert abs(float(stats[0]) - ref_out["loss"].item()) < REL_TOL
    assert abs(float(rstats[0]) - ref_out["route_loss"].item()) < REL_TOL
    assert rel_err(out["E_route"].cpu().numpy(), ref_out["E_route"].detach().numpy()) < REL_TOL
    want_stats = REF.edge_bce(ref_out["E_route"].detach().numpy(), marks, t[5], None)[0]
    assert np.array_equal(rstats[2:], want_stats[2:]) and abs(rstats[1] - want_stats[1]) < 1e-6
    assert set(g) == set(ref_g) and any(k.startswith("E_route") for k in g)
    l2 = {k: REF.L2NORM_SCALING * params[k] for k in params}          # the reference's gradients include the L2 term
    gscale = max(np.abs(ref_g[k] - l2[k]).max() for k in ref_g)
    worst = worst32 = 0.0
    for k in ref_g:
        ref = ref_g[k] - l2[k]
        scale = max(np.abs(ref).max(), 1e-3 * gscale)
        err = np.abs(g[k] - ref).max() / scale
        err32 = np.abs(f32_g[k] - ref_g[k]).max() / scale
        worst, worst32 = max(worst, err), max(worst32, err32)
        assert err < max(1e-5, 2 * err32), (k, err, err32)
    print("[d=%d lam=%g] worst per-variable gradient rel err: HIP %.2e, fp32 restatement %.2e" % (d, lam, worst, worst32))


@pytest.mark.parametrize("lam", [1.0, 0.25])
@pytest.mark.parametrize("d", [32, 64])
def test_gradient_parity_in_bf16_storage(cuda_device, d, lam):
    T = 3
    _, t, marks = parity_case()
    params = REF.route_params(d, seed=21)
    model, sess = route_session(d, params, float_dtype=torch.bfloat16, route_loss=lam)
    out = sess.loss_and_grads(feed_of(model, t, T, marks))
    torch.cuda.synchronize()
    g = model.store.grad_dict()
    batch = batch_from_tuple(t)
    fold = d == 64         # (what the build runs at that width: oracle.torch_oracle.step_bf16)

    def l2_dist(a, b):
        return float(np.sqrt(sum(((a[k] - b[k]) ** 2).sum() for k in b) / sum((b[k] ** 2).sum() for k in b)))
    ref_out, ref_g = REF.loss_and_grads(params, batch, marks, T, lam=lam, bf16=True, fold=fold)
    l2 = {k: REF.L2NORM_SCALING * params[k] for k in params}
    ref = {k: ref_g[k] - l2[k] for k in ref_g}
    nudged = {k: (v * (1 + 1e-6 * np.random.RandomState(1).randn(*v.shape))).astype(v.dtype) for k, v in params.items()}
    _, ref2 = REF.loss_and_grads(nudged, batch, marks, T, lam=lam, bf16=True, fold=fold)
    spread = l2_dist({k: ref2[k] - l2[k] for k in ref2}, ref)
    end_to_end = l2_dist(g, ref)
    stats, rstats = out["stats"].cpu().numpy(), out["route_stats"].cpu().numpy()
    print("\n[d=%d lam=%g bf16] loss %.6f (ref %.6f) route_loss %.6f (ref %.6f); gradient vs the oracle's own forward: L2 %.2e "
          "(its spread under a 1e-6 nudge: %.2e)" % (d, lam, stats[0], ref_out["loss"].item(), rstats[0],
                                                    ref_out["route_loss"].item(), end_to_end, spread))
    assert abs(float(stats[0]) - ref_out["loss"].item()) < 5e-4
    assert abs(float(rstats[0]) - ref_out["route_loss"].item()) < 5e-4
    assert end_to_end < 3 * max(spread, 1e-2)


# -------------------------------------------------------------------------------------- 4. no existing behaviour changes
def test_route_loss_zero_leaves_every_other_gradient_bit_identical(cuda_device):
    """Two stores with the same weights; route_head=True with route_loss=0 adds exact zeros to dE.h, so the gradient of
    every variable the plain network has is the plain network's, bit for bit (+0 and -0 compare equal).  After one
    train_step the variables are compared as well: the clip norm then also sums E_route's L2 term (1e-10 theta, ~1e-21 of
    the squared norm, far below its last bit) but over a longer buffer, whose reduction is cut differently -- so the step
    is compared bit for bit only when the two norms came out equal, and the gradients before the clip are what is pinned."""
    d, T = 64, 3
    _, t, marks = parity_case()
    params = REF.route_params(d, seed=5)
    plain_params = {k: v for k, v in params.items() if not k.startswith("E_route")}
    model0 = tspgnn.build_network(d, store=tspgnn.VariableStore())
    sess0 = tspgnn.Session(model0)
    sess0.run(tspgnn.global_variables_initializer())
    model0.store.load(plain_params)
    model1, sess1 = route_session(d, params, route_loss=0.0)
    b0, b1 = sess0.prepare(feed_of(model0, t, T)), sess1.prepare(feed_of(model1, t, T, marks))
    out0, out1 = sess0.loss_and_grads(b0), sess1.loss_and_grads(b1)
    torch.cuda.synchronize()
    g0, g1 = model0.store.grad_dict(), model1.store.grad_dict()
    assert torch.equal(out0["stats"], out1["stats"]) and torch.equal(out0["E_vote"], out1["E_vote"])
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    assert all(not g1[k].any() for k in g1 if k.startswith("E_route"))
    assert float(out1["route_stats"][0]) > 0
    o0, o1 = sess0.train_step(b0), sess1.train_step(b1)
    n0, n1 = float(o0["global_norm"].item()), float(o1["global_norm"].item())
    s0, s1 = model0.store.state_dict(), model1.store.state_dict()
    print("\nglobal norms %.9g / %.9g" % (n0, n1))
    assert abs(n0 - n1) <= 2.0 ** -22 * n0
    assert any(not np.array_equal(s0[k], plain_params[k]) for k in s0)      # (the step moved the variables)
    for k in s0:
        if n0 == n1:
            assert np.array_equal(s0[k], s1[k]), k
        else:       # one rounding of the clip scale apart: a variable moves by at most its last bit
            assert np.all(np.abs(s0[k] - s1[k]) <= np.spacing(np.abs(s0[k]).astype(np.float32))), k


@pytest.mark.parametrize("d", [32, 64])
def test_launches_without_the_head_are_the_recorded_ones(cuda_device, d):
    """tests/test_launch_trace.py's recorder around launches that really run: Session.forward_device and loss_and_grads of a
    network built without the head name the calls recorded before the head existed."""
    from test_launch_trace import recording
    want = json.load(open(os.path.join(GOLDEN, "route_head_launch_names.json")))
    model, sess, b, _ = REF.launch_case(d, cuda_device, route_head=False)
    with recording(True) as trace:
        sess.forward_device(b)
    assert REF.launch_names(trace) == want["forward_d%d" % d]
    with recording(True) as trace:
        sess.loss_and_grads(b)
    assert REF.launch_names(trace) == want["loss_and_grads_d%d" % d]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ 5. plumbing
def test_captured_training_step_matches_eager_with_the_head(cuda_device):
    d, T = 64, 3
    _, t, marks = parity_case()
    params = REF.route_params(d, seed=9)
    ends = []
    for captured in (False, True):
        model, sess = route_session(d, params, route_loss=0.5)
        b = sess.prepare(feed_of(model, t, T, marks))
        step = sess.capture_train_step(b) if captured else (lambda: sess.train_step(b))
        seen = []
        for _ in range(3):
            out = step()
            seen.append((out["stats"].clone(), out["route_stats"].clone()))
        torch.cuda.synchronize()
        ends.append((model.store.theta.clone(), seen, int(sess._adam["t"].item())))
    assert ends[0][2] == ends[1][2] == 3
    for (s0, r0), (s1, r1) in zip(ends[0][1], ends[1][1]):
        assert torch.equal(s0, s1) and torch.equal(r0, r1)
    assert len({float(r[0]) for _, r in ends[0][1]}) == 3       # (the steps moved the route loss)
    assert torch.equal(ends[0][0], ends[1][0])


def test_device_dataset_marks_its_batches(cuda_device):
    rng = np.random.RandomState(6)
    instances = [tspgnn.random_instance(n, rng) for n in (5, 9, 7, 5, 9, 7, 6)]
    Ma, Mw, _ = sparse_n12()
    instances.append((Ma, Mw, [int(v) for v in rng.permutation(12)]))
    ds = tspgnn.DeviceDataset(instances, device=cuda_device, routes=True)
    ids = [2, 0, 1, 7]
    b = ds.batch(ids, time_steps=2)
    want = route_edge_marks_host([instances[i] for i in ids])[0]
    assert np.array_equal(b.route_edges.cpu().numpy(), want) and want.sum() < 7 + 5 + 9 + 12
    buffer = b.route_edges
    ids2 = [5, 3, 4, 7]                                          # the same sizes in the same order: refilled in place
    assert ds.batch(ids2, time_steps=2, out=b) is b and b.route_edges is buffer
    want2 = route_edge_marks_host([instances[i] for i in ids2])[0]
    assert np.array_equal(b.route_edges.cpu().numpy(), want2) and not np.array_equal(want, want2)
    plain = tspgnn.DeviceDataset(instances, device=cuda_device).batch(ids, time_steps=2)
    assert getattr(plain, "route_edges", None) is None
    assert [x.shape for x in plain.tensors()] == [x.shape for x in b.tensors() if x is not b.route_edges]


def test_datasets_read_and_generated_with_routes_mark_their_batches(cuda_device, tmp_path):
    """from_directory(routes=True) on both readers and generate(routes=True): the marks of a batch are the host function's
    on the same instances; without routes= a batch carries none."""
    import random
    rng = np.random.RandomState(11)
    instances = [tspgnn.random_instance(n, rng) for n in (6, 9, 6, 12)]
    for k, (Ma, Mw, route) in enumerate(instances):
        tspgnn.write_graph(np.triu(Ma), Mw, str(tmp_path / ("%d.graph" % k)), route=route)
    ids = [3, 0, 2, 1]
    for reader in ("host", "device"):
        ds = tspgnn.DeviceDataset.from_directory(str(tmp_path), device=cuda_device, reader=reader, routes=True)
        read = [tspgnn.read_graph(str(tmp_path / ("%d.graph" % k))) for k in range(4)]     # (sorted file order: 0 .. 3)
        b = ds.batch(ids, time_steps=2)
        assert np.array_equal(b.route_edges.cpu().numpy(), route_edge_marks_host([read[i] for i in ids])[0]), reader
        plain = tspgnn.DeviceDataset.from_directory(str(tmp_path), device=cuda_device, reader=reader)
        assert plain._routes is None and getattr(plain.batch(ids, time_steps=2), "route_edges", None) is None
    random.seed(3)
    np.random.seed(3)
    ds = tspgnn.DeviceDataset.generate(6, 6, 9, device=cuda_device, routes=True)
    made = ds.to_instances()
    b = ds.batch([5, 1, 4], time_steps=2)
    want, missing = route_edge_marks_host([made[i] for i in (5, 1, 4)])
    assert np.array_equal(b.route_edges.cpu().numpy(), want) and not missing.any()
    assert want.sum() == sum(len(made[i][2]) for i in (5, 1, 4))


def test_accumulated_step_equals_the_union_batch_reference(cuda_device):
    """Two micro-batches through loss_and_grads + accumulate_grads + reduce_accumulated against the float64 reference of
    their union, with the bar of tests/test_gpu_accumulate.py: per variable sum_k (B_k / B) max(1e-5, 2 err32_k) scale_k
    + K 2^-23 sum_k (B_k / B) max |g_k|, err32_k and scale_k formed per micro-batch as the gradient-parity test forms them."""
    d, T, lam = 64, 3, 0.5
    instances, _, _ = parity_case()
    params = REF.route_params(d, seed=21)
    model, sess = route_session(d, params, route_loss=lam)
    union = tspgnn.InstanceLoader.create_batch(instances)
    union_marks = route_edge_marks_host(instances)[0]
    e0, v0 = REF.segments(union[5]), REF.segments(union[4])

    def shard(lo, hi):
        """Graphs lo .. hi-1 of the union batch, with the labels and target costs they have THERE, and their marks."""
        es, vs = slice(e0[lo], e0[hi]), slice(v0[lo], v0[hi])
        ev = tspgnn.SparseEV(union[0].uv[es] - v0[lo], int(v0[hi] - v0[lo]))
        return (ev, union[1][es], union[2][es], union[3][lo:hi], union[4][lo:hi], union[5][lo:hi]), union_marks[es]
    parts, B, K = [shard(0, 1), shard(1, 4)], len(instances), 2
    bar = {k: 0.0 for k in params}
    rounding = {k: 0.0 for k in params}
    l2 = {k: REF.L2NORM_SCALING * params[k] for k in params}
    for k, (t, marks) in enumerate(parts):
        part = t[3]
        out = sess.loss_and_grads(feed_of(model, t, T, marks))
        sess.accumulate_grads(len(part), out["stats"], first=(k == 0))
        batch = batch_from_tuple(t)
        _, g64 = REF.loss_and_grads(params, batch, marks, T, lam=lam)
        _, g32 = REF.loss_and_grads(params, batch, marks, T, lam=lam, dtype=torch.float32, dense=True)
        ref_k = {v: g64[v] - l2[v] for v in g64}
        gscale = max(np.abs(r).max() for r in ref_k.values())
        for v in ref_k:
            scale = max(np.abs(ref_k[v]).max(), 1e-3 * gscale)
            bar[v] += len(part) / B * max(1e-5, 2 * float(np.abs(g32[v] - g64[v]).max()) / scale) * scale
            rounding[v] += len(part) / B * np.abs(ref_k[v]).max()
    sess.reduce_accumulated(out["stats"])
    torch.cuda.synchronize()
    got = model.store.grad_dict()
    want_out, want = REF.loss_and_grads(params, batch_from_tuple(union), union_marks, T, lam=lam)
    worst = 0.0
    for v in want:
        err = np.abs(got[v] - (want[v] - l2[v])).max()
        limit = bar[v] + K * 2.0 ** -23 * rounding[v]
        worst = max(worst, err / limit)
        assert err < limit, (v, err, limit)
    print("\nworst accumulated-gradient error / bar: %.2f" % worst)
    assert abs(float(out["stats"][0].item()) - want_out["loss"].item()) < REL_TOL
    # and the one call: an optimiser step over the two micro-batches runs and moves the head
    before = model.store.state_dict()
    out = sess.train_step_accumulated([feed_of(model, t, T, marks) for t, marks in parts])
    assert "route_stats" in out and int(sess._adam["t"].item()) == 1
    after = model.store.state_dict()
    assert not np.array_equal(before["E_route_MLP_layer_1/kernel"], after["E_route_MLP_layer_1/kernel"])


# ------------------------------------------------------------------------------------------------------------ 6. it learns
def test_forty_steps_lower_the_route_loss_and_the_decoders_take_the_head(cuda_device, capsys):
    rng = np.random.RandomState(40)
    graphs = [tspgnn.random_instance(10, rng) for _ in range(8)]
    labels = tspgnn.label_tours([(Ma, Mw) for Ma, Mw, _ in graphs], init_tours=[r for _, _, r in graphs], lower_bound=False,
                                device=cuda_device)
    instances = [(Ma, Mw, [int(v) for v in r.tour]) for (Ma, Mw, _), r in zip(graphs, labels)]
    model = tspgnn.build_network(32, store=tspgnn.VariableStore(), route_head=True)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer(seed=2))
    t = tspgnn.InstanceLoader.create_batch(instances)
    marks = route_edge_marks_host(instances)[0]
    assert marks.sum() == 8 * 10
    b = sess.prepare(feed_of(model, t, 4, marks))
    before = float(sess.forward(b)["route_stats"][0].item())
    for _ in range(40):
        sess.train_step(b)
    after = float(sess.forward(b)["route_stats"][0].item())
    print("\nroute loss %.6f -> %.6f after 40 steps" % (before, after))
    assert after < before
    # the fetches, and run_batch's line
    feed = feed_of(model, t, 4, marks)
    route_loss, acc, logits = sess.run([model["route_loss"], model["route_acc"], model["E_route"]], feed_dict=feed)
    assert abs(float(route_loss) - after) < 1e-6 and 0.0 <= float(acc) <= 1.0 and logits.shape == (len(marks),)
    counts = sess.run([model[k] for k in ("route_TP", "route_FP", "route_TN", "route_FN")], feed_dict=feed)
    assert sum(float(c) for c in counts) == len(marks)
    capsys.readouterr()
    tspgnn.run_batch(sess, model, t + (marks,), 0, 0, 4, train=False)
    assert "route_loss=%.4f" % after in capsys.readouterr().out
    for kw in ({}, {"beam": 8}):
        res = tspgnn.decode_tours(sess, model, instances, 4, target_costs=[1.0] * 8, votes="route", **kw)
        assert all(sorted(r.tour) == list(range(10)) for r in res)
    with pytest.raises(ValueError, match="route_head=True"):
        plain = tspgnn.build_network(32, store=tspgnn.VariableStore())
        tspgnn.decode_tours(tspgnn.Session(plain), plain, instances, 4, target_costs=[1.0] * 8, votes="route")
