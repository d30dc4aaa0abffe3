"""GPU labelling of instances with up to 256 vertices (tspgnn.dataset.label_tours on tspgnn_tour_search_tri /
tspgnn_tour_lower_bound_tri, csrc/tour_search.hip): bit-identity with the square kernels for n <= 128 (which
test_gpu_tour_solver.py ties to exact Held-Karp optima), exact optima on points in convex position for n 129-256, planted
and non-Hamiltonian sparse graphs, determinism, the certified fraction at n = 200 and create_dataset end to end."""
import filecmp
import os
import random

import numpy as np
import pytest
import torch

import tspgnn
from tspgnn import _lib, dataset

pytestmark = pytest.mark.gpu

# Measured 0.898 on the MI355X with the n > 128 defaults (8 x 384); 0.83 leaves ~3.5 binomial standard
# deviations at 256 instances for changes of the solver or its defaults.
CERTIFIED_MIN_N200 = 0.83


def _instances(rng, sizes, kind):
    out, inits = [], []
    for n in sizes:
        p = rng.rand(n, 2)
        Mw = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        Ma = np.triu(np.ones((n, n)), 1)
        perm = None
        if kind == "metric":
            W = np.triu(rng.rand(n, n), 1)
            Mw = dataset.floyd_warshall(W + W.T)
        elif kind == "sparse":
            Ma = np.triu((rng.rand(n, n) < 0.3).astype(float), 1)
            perm = [int(x) for x in rng.permutation(n)]
            for i, j in zip(perm, perm[1:] + perm[:1]):
                Ma[min(i, j), max(i, j)] = 1
        out.append((Ma, Mw))
        inits.append(perm)
    return out, inits


def _run_kernels(insts, inits, tri, seed, restarts, kicks, lb_iters):
    """Both kernels of one layout on one launch each, straight through the C ABI: (tours, fp32 costs, fp64 bounds)."""
    ns = np.array([m.shape[0] for m, _ in insts], dtype=np.int32)
    sizes = ns.astype(np.int64) * (ns - 1) // 2 if tri else ns.astype(np.int64) ** 2
    w_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    t_off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    packs = []
    for (Ma, Mw) in insts:
        A = dataset._edge_mask(Ma)[None]
        W = np.asarray(Mw, dtype=np.float64)[None]
        packs.append((dataset._penalised_tri if tri else dataset._penalised)(A, W).reshape(-1))
    init = np.concatenate([np.arange(n) if it is None else np.asarray(it) for n, it in zip(ns, inits)]).astype(np.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("W", np.concatenate(packs)), ("w_off", w_off), ("t_off", t_off), ("n", ns), ("init", init))}
    B = len(insts)
    tours = torch.empty(int(ns.sum()), dtype=torch.int32, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    lb = torch.empty(B, dtype=torch.float64, device=dev)
    suffix = "_tri" if tri else ""
    st = _lib.current_stream()
    _lib.call("tspgnn_tour_search" + suffix, _lib.ptr(d["W"]), _lib.ptr(d["w_off"]), _lib.ptr(d["n"]), _lib.ptr(d["init"]),
              _lib.ptr(d["t_off"]), None, B, int(ns.max()), restarts, kicks, seed, _lib.ptr(tours), _lib.ptr(costs), st)
    _lib.call("tspgnn_tour_lower_bound" + suffix, _lib.ptr(d["W"]), _lib.ptr(d["w_off"]), _lib.ptr(d["n"]),
              _lib.ptr(costs), B, int(ns.max()), lb_iters, _lib.ptr(lb), st)
    torch.cuda.synchronize()
    return tours.cpu().numpy(), costs.cpu().numpy(), lb.cpu().numpy()


def test_tri_kernels_bitwise_equal_to_square_kernels_up_to_n128(cuda_device):
    rng = np.random.RandomState(30)
    sizes = list(rng.randint(4, 129, size=96)) + [4, 64, 65, 127, 128]
    insts, inits = [], []
    for kind, part in (("euc", sizes[0::3]), ("metric", sizes[1::3]), ("sparse", sizes[2::3])):
        a, b = _instances(rng, part, kind)
        insts += a
        inits += b
    for restarts, kicks in ((8, 16), (3, 5)):
        sq = _run_kernels(insts, inits, False, 5, restarts, kicks, 120)
        tr = _run_kernels(insts, inits, True, 5, restarts, kicks, 120)
        assert np.array_equal(sq[0], tr[0])
        assert np.array_equal(sq[1].view(np.uint32), tr[1].view(np.uint32))
        assert np.array_equal(sq[2].view(np.uint64), tr[2].view(np.uint64))
        assert np.all(np.isfinite(tr[2])) and np.all(tr[2] <= tr[1] * (1 + 1e-6))
    # label_tours is solve_tours for n <= 128
    assert dataset.label_tours(insts, init_tours=inits, seed=9) == dataset.solve_tours(insts, init_tours=inits, seed=9)


def _convex(rng, n, ax, ay):
    """n points at random angles (every gap at least a third of the mean) on an ellipse, labels shuffled.  Returns the
    instance and the hull order as a canonical tour."""
    gaps = 0.5 + rng.rand(n)
    th = 2 * np.pi * np.cumsum(gaps) / gaps.sum()
    pts = np.stack([ax * np.cos(th), ay * np.sin(th)], 1)
    lab = rng.permutation(n)
    P = np.empty_like(pts)
    P[lab] = pts                       # vertex lab[k] sits at angle th[k]
    Mw = np.sqrt(((P[:, None] - P[None]) ** 2).sum(-1))
    hull = list(lab)
    k0 = hull.index(0)
    hull = hull[k0:] + hull[:k0]
    if hull[1] > hull[-1]:
        hull = [0] + hull[1:][::-1]
    return (np.triu(np.ones((n, n)), 1), Mw), [int(x) for x in hull]


def _fp64_cost(Mw, tour):
    up = np.triu(np.asarray(Mw, dtype=np.float64), 1)
    c = 0.0
    for a, b in zip(tour, tour[1:] + tour[:1]):
        c += up[min(a, b), max(a, b)]
    return c


def test_convex_position_exact_optimum_n129_256(cuda_device):
    rng = np.random.RandomState(31)
    cases = [_convex(rng, n, 1.0, 1.0) for n in (129, 150, 200, 256)]
    cases += [_convex(rng, n, 1.0, 0.55) for n in (140, 201, 255, 256)]
    res = dataset.label_tours([c[0] for c in cases], seed=3)
    for (inst, hull), r in zip(cases, res):
        opt = _fp64_cost(inst[1], hull)
        assert r.feasible
        assert r.tour == hull, len(hull)
        assert r.cost == opt
        assert r.lb <= opt


def test_planted_and_non_hamiltonian_n200(cuda_device):
    rng = np.random.RandomState(32)
    n = 200
    insts, inits = [], []
    for _ in range(6):
        p = rng.rand(n, 2)
        Mw = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
        perm = [int(x) for x in rng.permutation(n)]
        Ma = np.zeros((n, n))
        for i, j in zip(perm, perm[1:] + perm[:1]):
            Ma[min(i, j), max(i, j)] = 1
        for _ in range(3 * n):        # a few chords
            i, j = rng.randint(n, size=2)
            if i != j:
                Ma[min(i, j), max(i, j)] = 1
        insts.append((Ma, Mw))
        inits.append(perm)
    res = dataset.label_tours(insts, init_tours=inits, seed=4)
    for (Ma, Mw), r in zip(insts, res):
        assert r.feasible and sorted(r.tour) == list(range(n))
        assert r.tour[0] == 0 and r.tour[1] < r.tour[-1]
        assert r.cost == _fp64_cost(Mw, r.tour)
        assert r.lb <= r.cost
    # a path plus chords that never touch vertex n-1's neighbourhood: vertex n-1 has degree 1, so no tour exists
    Ma = np.zeros((n, n))
    for v in range(n - 1):
        Ma[v, v + 1] = 1
    for i in range(0, n - 3, 7):
        Ma[i, i + 2] = 1
    Mw = rng.rand(n, n)
    (r,) = dataset.label_tours([(Ma, Mw)], seed=4)
    assert not r.feasible
    assert dataset.solve(Ma, Mw) is None


def test_determinism_chunks_subsets_and_mixing(cuda_device):
    rng = np.random.RandomState(33)
    sizes = [129, 160, 200, 231, 256, 140, 190, 256]
    insts, inits = _instances(rng, sizes[:5], "euc")
    a, b = _instances(rng, sizes[5:], "sparse")
    insts += a
    inits += b
    kw = dict(init_tours=inits, seed=6, restarts=4, kicks=24, lb_iters=200)
    r1 = dataset.label_tours(insts, **kw)
    r2 = dataset.label_tours(insts, **kw)
    r3 = dataset.label_tours(insts, chunk=3, **kw)
    assert r1 == r2 == r3
    for (Ma, Mw), r in zip(insts, r1):
        assert sorted(r.tour) == list(range(Ma.shape[0])) and r.lb <= r.cost
    half = dataset.label_tours(insts[4:], index=np.arange(4, 8), **dict(kw, init_tours=inits[4:]))
    assert half == r1[4:]
    # n = 30 and n = 200 in one call: each result is the one it gets alone, under the same index
    small, _ = _instances(rng, [30], "euc")
    mixed = dataset.label_tours([small[0], insts[2]], seed=6, restarts=4, kicks=24, lb_iters=200)
    alone_s = dataset.label_tours([small[0]], seed=6, restarts=4, kicks=24, lb_iters=200)
    alone_b = dataset.label_tours([insts[2]], index=[1], seed=6, restarts=4, kicks=24, lb_iters=200)
    assert mixed == alone_s + alone_b


def test_certified_fraction_n200(cuda_device):
    np.random.seed(34)
    random.seed(34)
    graphs = dataset.draw_instances(200, 200, samples=256)
    res = dataset.label_tours([(g[0], g[1]) for g in graphs], init_tours=[g[2] for g in graphs])
    c = dataset.certify(res, 0.02)
    gap = np.array([(r.cost - r.lb) / r.cost for r in res])
    print("n=200 certified fraction at dev=0.02: %.4f (label0 %.4f, label1 %.4f); gap median %.5f p90 %.5f max %.5f"
          % (c["fraction"], c["label0"].mean(), c["label1"].mean(), np.median(gap), np.percentile(gap, 90), gap.max()))
    assert all(r.feasible for r in res)
    assert np.all(gap >= 0)
    assert c["fraction"] >= CERTIFIED_MIN_N200


def test_create_dataset_n200_end_to_end(cuda_device, tmp_path):
    def make(path, nmin, nmax, samples):
        random.seed(8)
        np.random.seed(8)
        return dataset.create_dataset(str(path), nmin, nmax, samples=samples)

    s1 = make(tmp_path / "a", 200, 200, 16)
    s2 = make(tmp_path / "b", 200, 200, 16)
    assert np.all(s1["feasible"]) and np.all(s1["n"] == 200)
    assert np.array_equal(s1["cost"], s2["cost"]) and np.array_equal(s1["lb"], s2["lb"])
    assert np.all(s1["lb"] <= s1["cost"])
    names = sorted(os.listdir(tmp_path / "a"))
    assert len(names) == 16
    _, mismatch, errors = filecmp.cmpfiles(tmp_path / "a", tmp_path / "b", names, shallow=False)
    assert not mismatch and not errors
    Ma, Mw, route = tspgnn.read_graph(str(tmp_path / "a" / "3.graph"))
    assert route[0] == 0 and sorted(route) == list(range(200))
    # config 5's network (d = 128, bf16 storage) on a batch of the labelled instances
    loader = tspgnn.InstanceLoader(str(tmp_path / "a"))
    batch = next(loader.get_batches(4, 0.02))
    model = tspgnn.build_network(128, float_dtype=torch.bfloat16)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    out = tspgnn.run_batch(sess, model, batch, 0, 0, 4, train=False, verbose=False)
    assert np.isfinite(out[0])
    # a range across n = 128 uses both kernel layouts
    s3 = make(tmp_path / "c", 100, 160, 24)
    assert np.any(s3["n"] <= 128) and np.any(s3["n"] > 128)
    assert np.all(s3["feasible"]) and np.all(s3["lb"] <= s3["cost"])
