"""GPU candidate-list tour search (neighbors=K; tspgnn_tour_search_knn / _knn_tri, csrc/tour_search.hip): with every edge
in the candidate set it is the full-scan kernel bit for bit (which test_gpu_tour_solver.py ties to exact optima); with a
restricted set it equals the NumPy restatement of tests/knn_search_reference.py tour for tour; the two layouts agree;
validity, determinism and quality at n 160-200; create_dataset end to end."""
import random

import numpy as np
import pytest
import torch

import knn_search_reference as ref
import tspgnn
from baseline_reference import cost64, euclidean, packed, sparse_planted
from tspgnn import _lib, dataset

pytestmark = pytest.mark.gpu

# test_quality_against_full_scan_n160: mean cost with neighbors=8 over mean cost of the full scan, measured on the MI355X
# (32 Euclidean instances, 4 x 48 kicks).
MEASURED_RATIO_N160 = 0.9981   # 9.720764 / 9.739238


def _search(insts, inits, tri, neighbors, seed, restarts, kicks):
    """One launch of the search of one layout straight through the C ABI: (tours split per instance, fp32 costs).
    neighbors=None: the full-scan entry point.  inits=None: no init_tours (every chain starts at random)."""
    ns = np.array([m.shape[0] for m, _ in insts], dtype=np.int32)
    sizes = ns.astype(np.int64) * (ns - 1) // 2 if tri else ns.astype(np.int64) ** 2
    w_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    t_off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    packs = []
    for (Ma, Mw) in insts:
        A = dataset._edge_mask(Ma)[None]
        W = np.asarray(Mw, dtype=np.float64)[None]
        packs.append((dataset._penalised_tri if tri else dataset._penalised)(A, W).reshape(-1))
    dev = torch.device("cuda", torch.cuda.current_device())
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("W", np.concatenate(packs)), ("w_off", w_off), ("t_off", t_off), ("n", ns))}
    init = None
    if inits is not None:
        init = torch.from_numpy(np.concatenate([np.asarray(it) for it in inits]).astype(np.int32)).to(dev)
    tours = torch.empty(int(ns.sum()), dtype=torch.int32, device=dev)
    costs = torch.empty(len(insts), dtype=torch.float32, device=dev)
    name = "tspgnn_tour_search" + ("" if neighbors is None else "_knn") + ("_tri" if tri else "")
    knn = () if neighbors is None else (neighbors,)
    _lib.call(name, _lib.ptr(d["W"]), _lib.ptr(d["w_off"]), _lib.ptr(d["n"]), _lib.ptr(init), _lib.ptr(d["t_off"]), None,
              len(insts), int(ns.max()), restarts, kicks, *knn, seed, _lib.ptr(tours), _lib.ptr(costs),
              _lib.current_stream())
    torch.cuda.synchronize()
    return np.split(tours.cpu().numpy(), np.cumsum(ns)[:-1]), costs.cpu().numpy()


def _integer(rng, n):
    """Weights from {1, 2, 3}: many moves tie in delta, so the smaller code decides."""
    W = np.triu(rng.randint(1, 4, size=(n, n)).astype(np.float64), 1)
    return np.triu(np.ones((n, n)), 1), W + W.T


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and \
        np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("tri", [False, True], ids=["square", "tri"])
def test_full_neighbourhood_equals_full_scan_bitwise(cuda_device, tri):
    rng = np.random.RandomState(60)
    insts, inits = [], []
    for make in (euclidean, sparse_planted, _integer):
        for n in (4, 5, 7, 12, 17, 24, 33):
            insts.append(make(rng, n))
            inits.append(rng.permutation(n))
    for given in (inits, None):
        full = _search(insts, given, tri, None, 21, 2, 4)
        knn = _search(insts, given, tri, 32, 21, 2, 4)
        assert _same(full, knn)
        for (Ma, _), t in zip(insts, knn[0]):
            assert sorted(t) == list(range(Ma.shape[0]))


@pytest.mark.parametrize("K", ref.KS)
@pytest.mark.parametrize("layout", ["square", "tri"])
def test_restricted_neighbourhood_equals_restatement(cuda_device, layout, K):
    sizes = ref.TRI_N if layout == "tri" else ref.SQUARE_N
    cases = [ref.instance(layout, n) for n in sizes]
    insts, inits = [(Ma, Mw) for Ma, Mw, _ in cases], [init for _, _, init in cases]
    for kicks in ref.KICKS:
        tours, costs = _search(insts, inits, layout == "tri", K, ref.SEED, 1, kicks)
        for n, (Ma, Mw), t, c in zip(sizes, insts, tours, costs):
            want = ref.expected(layout, n, K)[0][kicks]
            assert t.tolist() == want, (n, kicks)
            c64 = cost64(packed(Ma, Mw), want)
            assert abs(float(c) - c64) <= n * 2.0 ** -23 * c64, (n, kicks, float(c), c64)


def test_tri_equals_square_bitwise_with_neighbors_8(cuda_device):
    rng = np.random.RandomState(61)
    sizes = [4, 5, 9, 64, 65, 127, 128] + [int(v) for v in rng.randint(6, 128, size=9)]
    insts, inits = [], []
    for k, n in enumerate(sizes):
        insts.append((euclidean, sparse_planted, _integer)[k % 3](rng, n))
        inits.append(rng.permutation(n))
    assert len(insts) == 16
    for restarts, kicks in ((4, 6), (1, 0)):
        assert _same(_search(insts, inits, False, 8, 22, restarts, kicks), _search(insts, inits, True, 8, 22, restarts, kicks))


def test_validity_and_determinism_n200(cuda_device):
    rng = np.random.RandomState(62)
    n = 200
    insts, inits, planted = [], [], []
    for k in range(23):
        if k % 3 == 2:
            Ma, Mw = euclidean(rng, n)
            perm = [int(x) for x in rng.permutation(n)]
            Ma = np.triu((rng.rand(n, n) < 0.05).astype(float), 1)
            for i, j in zip(perm, perm[1:] + perm[:1]):
                Ma[min(i, j), max(i, j)] = 1
            insts.append((Ma, Mw))
            inits.append(perm)
            planted.append(k)
        else:
            insts.append(euclidean(rng, n))
            inits.append(None)
    # a path plus short chords: vertex n-1 has degree 1, so no tour exists
    Ma = np.zeros((n, n))
    for v in range(n - 1):
        Ma[v, v + 1] = 1
    for i in range(0, n - 3, 7):
        Ma[i, i + 2] = 1
    insts.append((Ma, rng.rand(n, n)))
    inits.append(None)
    kw = dict(neighbors=8, restarts=4, kicks=16, seed=8, lower_bound=False)
    r1 = dataset.label_tours(insts, init_tours=inits, **kw)
    assert len(r1) == 24
    for r in r1:
        assert sorted(r.tour) == list(range(n)) and r.tour[0] == 0 and r.tour[1] < r.tour[-1]
    assert all(r1[k].feasible for k in planted)
    assert all(r.feasible for r in r1[:23])
    assert not r1[23].feasible
    assert dataset.solve(*insts[23], neighbors=8, restarts=4, kicks=16, seed=8) is None
    strip = lambda rs: [(r.tour, r.cost, r.feasible) for r in rs]   # noqa: E731  (lb is nan without the bound)
    assert strip(dataset.label_tours(insts, init_tours=inits, chunk=5, **kw)) == strip(r1)
    assert strip(dataset.label_tours(insts, init_tours=inits, chunk=24, **kw)) == strip(r1)
    sub = [3, 8, 23]
    alone = dataset.label_tours([insts[k] for k in sub], init_tours=[inits[k] for k in sub], index=sub, **kw)
    assert strip(alone) == strip([r1[k] for k in sub])
    # the restriction is real: the full scan finds other tours on these instances
    assert strip(dataset.label_tours(insts[:4], init_tours=inits[:4], **dict(kw, neighbors=None))) != strip(r1[:4])


def test_quality_against_full_scan_n160(cuda_device):
    """Measured on the MI355X: see MEASURED_RATIO_N160.  One percent is half of dev = 0.02, the scale at which a label
    changes."""
    rng = np.random.RandomState(63)
    insts = [euclidean(rng, 160) for _ in range(32)]
    kw = dict(restarts=4, kicks=48, seed=9, lower_bound=False)
    full = np.mean([r.cost for r in dataset.label_tours(insts, **kw)])
    knn = np.mean([r.cost for r in dataset.label_tours(insts, neighbors=8, **kw)])
    print("n=160 mean cost: neighbors=8 %.6f, full scan %.6f, ratio %.5f" % (knn, full, knn / full))
    assert knn / full <= max(MEASURED_RATIO_N160, 1.0) + 0.01


def test_create_dataset_end_to_end_with_neighbors(cuda_device, tmp_path):
    random.seed(12)
    np.random.seed(12)
    s = dataset.create_dataset(str(tmp_path), 136, 136, samples=6, neighbors=8)
    assert np.all(s["feasible"]) and np.all(s["n"] == 136) and np.all(s["lb"] <= s["cost"])
    for i in range(6):
        Ma, Mw, route = tspgnn.read_graph(str(tmp_path / ("%d.graph" % i)))
        route = [int(v) for v in route]
        assert route[0] == 0 and sorted(route) == list(range(136))
        A = dataset._edge_mask(Ma)
        assert all(A[a, b] for a, b in zip(route, route[1:] + route[:1]))
    # create_graph hands neighbors to the search as well
    np.random.seed(13)
    Ma, Mw, route, _ = dataset.create_graph(30, 0.4, neighbors=5)
    assert sorted(route) == list(range(30)) and all(dataset._edge_mask(Ma)[a, b] for a, b in zip(route, route[1:] + route[:1]))
