"""Host side of the dataset module (tspgnn/dataset.py): the reference's instance stream, the metric closure, the
certification arithmetic and the argument checks of the two tour kernels' entry points.  No GPU.

Fixture recipe (tests/golden/dataset_create_graph.npz): run the reference's dataset.py with a stub ``concorde.tsp``
module (TSPSolver = object) inserted into sys.modules and ``dataset.solve`` replaced by ``lambda Ma, Mw: [0]``, so
that no RNG is consumed beyond create_graph's own draws, then
  - np.random.seed(11); create_graph(12, 1.0, 'euc_2D')  -> euc_full_{Ma,Mw}, then np.random.rand(4) -> euc_full_state
  - np.random.seed(12); create_graph(15, 0.3, 'euc_2D')  -> euc_sparse_*
  - np.random.seed(13); create_graph(10, 1.0, 'random', metric=True) -> rand_metric_* (networkx closure)
  - random.seed(5); np.random.seed(5); create_dataset(path, 6, 9, conn_min=0.3, conn_max=0.9, samples=20) with
    dataset.write_graph replaced by a recorder of its (Ma, Mw) arguments -> ds_{i}_{Ma,Mw}.
"""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from tspgnn import _lib, dataset
from tspgnn.instance_loader import route_cost

FIX = os.path.join(GOLDEN, "dataset_create_graph.npz")


def _ulps(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 1e-300)


@pytest.mark.parametrize("name,n,conn,dist,seed", [("euc_full", 12, 1.0, "euc_2D", 11),
                                                    ("euc_sparse", 15, 0.3, "euc_2D", 12),
                                                    ("rand_metric", 10, 1.0, "random", 13)])
def test_create_graph_draws_match_reference(name, n, conn, dist, seed):
    z = np.load(FIX)
    np.random.seed(seed)
    Ma, Mw, perm, nodes = dataset._draw_graph(n, conn, distances=dist, metric=True)
    assert np.array_equal(np.triu(Ma), z[name + "_Ma"])
    if dist == "euc_2D":
        assert np.array_equal(Mw, z[name + "_Mw"])
        assert nodes.shape == (n, 2)
    else:
        assert _ulps(Mw, z[name + "_Mw"]).max() <= 4
    assert np.array_equal(np.random.rand(4), z[name + "_state"])   # the same number of draws
    assert sorted(perm) == list(range(n))
    for i, j in zip(perm, perm[1:] + perm[:1]):
        assert Ma[i, j] == 1 and Ma[j, i] == 1


def test_create_dataset_instance_stream_matches_reference():
    z = np.load(FIX)
    random.seed(5)
    np.random.seed(5)
    graphs = dataset.draw_instances(6, 9, conn_min=0.3, conn_max=0.9, samples=20, distances="euc_2D")
    assert len(graphs) == int(z["ds_count"])
    for i, (Ma, Mw, perm, nodes) in enumerate(graphs):
        assert np.array_equal(np.triu(Ma), z["ds_%d_Ma" % i])
        assert np.array_equal(Mw, z["ds_%d_Mw" % i])


def test_floyd_warshall_matches_networkx():
    nx = pytest.importorskip("networkx")
    rng = np.random.RandomState(3)
    n = 14
    W = rng.rand(n, n)
    W = np.triu(W, 1)
    W = W + W.T
    D = dataset.floyd_warshall(W)
    G = nx.Graph()
    G.add_edges_from([(i, j, {"weight": W[i, j]}) for i in range(n) for j in range(n)])
    for i in range(n):
        for j in range(n):
            ref = 0.0 if i == j else nx.shortest_path_length(G, source=i, target=j, weight="weight")
            assert _ulps(np.array(D[i, j]), np.array(ref)) <= 4
    assert np.array_equal(D, D.T)
    # the closure is metric
    for k in range(n):
        assert np.all(D <= D[:, k:k + 1] + D[k:k + 1, :] + 1e-15)


def test_penalty_and_rounding_direction():
    Ma = np.triu(np.ones((5, 5)), 1)
    Ma[0, 2] = 0
    Mw = np.random.RandomState(0).rand(5, 5)
    A = dataset._edge_mask(Ma)
    W = dataset._penalised(A[None], Mw[None])[0]
    up = np.triu(Mw, 1)
    w = up + up.T
    real = w[A]
    assert W.dtype == np.float32
    assert np.all(W[A].astype(np.float64) <= real) and np.all(real - W[A] < 1e-7)
    pen = 5 * real.max() + 1
    assert W[0, 2] == W[2, 0] and W[0, 2] <= pen and pen - W[0, 2] < 1e-5
    assert np.all(np.diag(W) == 0)


def test_host_small_instances_and_certification_quirk():
    # n < 4 is solved on the host: the tour, its cost and a bound equal to it
    Ma = np.array([[0, 1, 1], [0, 0, 1], [0, 0, 0]])
    Mw = np.array([[0, 0.5, 0.25], [0.5, 0, 0.125], [0.25, 0.125, 0]])
    (r,) = dataset.solve_tours([(Ma, Mw)])
    assert r.tour == [0, 1, 2] and r.feasible and r.cost == r.lb == 0.875
    # the quirk target: pairs (r0,r1), (r1,r2), then (r[-1], r[1]) -- here (2,1): 0.5 + 0.125 + 0.125
    assert r.target == 3 * route_cost(np.triu(Mw, 1), [0, 1, 2])
    assert abs(r.target - 3 * (0.75 / 3)) < 1e-15
    Ma[0, 2] = 0
    (r,) = dataset.solve_tours([(Ma, Mw)])
    assert not r.feasible and r.lb == float("inf")
    assert dataset.solve(Ma, Mw) is None


def test_certify_arithmetic():
    R = dataset.TourResult
    Q = 10.0
    rs = [R([0], 10.0, 9.9, True, Q),      # both: lb 9.9 > 9.8, cost 10 <= 10.2
          R([0], 10.0, 9.8, True, Q),      # lb == (1-dev) Q: label 0 not certified (strict)
          R([0], 10.2, 9.9, True, Q),      # cost == (1+dev) Q: label 1 certified
          R([0], 10.3, 10.25, True, Q),    # the tour is longer than (1+dev) Q
          R([0], 10.0, 9.9, False, Q)]     # infeasible tour: label 1 not certified
    c = dataset.certify(rs, 0.02)
    assert list(c["label0"]) == [True, False, True, True, True]
    assert list(c["label1"]) == [True, True, True, False, False]
    assert list(c["both"]) == [True, False, True, False, False]
    assert c["fraction"] == pytest.approx(0.4)
    summ = {"cost": [r.cost for r in rs], "lb": [r.lb for r in rs], "target": [Q] * 5,
            "feasible": [r.feasible for r in rs]}
    assert list(dataset.certify(summ, 0.02)["both"]) == list(c["both"])


def test_quirk_target_on_sparse_file_matrix():
    # read_graph's Mw is zero off the edge set: the quirk's closing pair (route[-1], route[1]) can weigh 0
    n = 5
    Ma = np.zeros((n, n))
    for i in range(n):
        Ma[i, (i + 1) % n] = Ma[(i + 1) % n, i] = 1
    Mw = np.arange(n * n, dtype=np.float64).reshape(n, n) / 100.0
    Mw = Mw + Mw.T
    tour = [0, 1, 2, 3, 4]
    t = dataset._target(Ma, Mw, tour)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4)]
    expect = sum(Mw[a, b] for a, b in pairs) + 0.0   # (4, 1) is no edge: 0 in the file
    assert t == pytest.approx(expect, rel=1e-15)


def test_entry_points_reject_bad_arguments_without_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(16)
    # n_max > 128: EUNSUPPORTED before anything is launched
    assert L.tspgnn_tour_search(p, p, p, None, p, None, 4, 129, 4, 8, 0, p, p, None) == -2
    assert L.tspgnn_tour_lower_bound(p, p, p, p, 4, 129, 10, p, None) == -2
    # bad sizes and null pointers: EINVAL
    assert L.tspgnn_tour_search(None, p, p, None, p, None, 4, 20, 4, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search(p, p, p, None, p, None, 4, 20, 0, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search(p, p, p, None, p, None, 4, 20, 17, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search(p, p, p, None, p, None, 4, 20, 4, -1, 0, p, p, None) == -1
    assert L.tspgnn_tour_search(p, p, p, None, p, None, 4, 3, 4, 8, 0, p, p, None) == -1
    assert L.tspgnn_tour_search(p, p, p, None, p, None, -1, 20, 4, 8, 0, p, p, None) == -1
    assert b"restarts" in L.tspgnn_last_error() or b"n_inst" in L.tspgnn_last_error()
    assert L.tspgnn_tour_lower_bound(p, p, p, None, 4, 20, 10, p, None) == -1
    assert L.tspgnn_tour_lower_bound(p, p, p, p, 4, 20, 0, p, None) == -1
    assert L.tspgnn_tour_lower_bound(p, p, p, p, 4, 2, 10, p, None) == -1
    # empty batches are a no-op
    assert L.tspgnn_tour_search(None, None, None, None, None, None, 0, 0, 1, 0, 0, None, None, None) == 0
    assert L.tspgnn_tour_lower_bound(None, None, None, None, 0, 0, 1, None, None) == 0


def test_solve_tours_rejects_bad_instances_without_gpu():
    big = np.ones((129, 129))
    with pytest.raises(ValueError, match="129"):
        dataset.solve_tours([(big, big)])
    with pytest.raises(ValueError):
        dataset.solve_tours([(np.ones((5, 5)), np.ones((4, 4)))])
    with pytest.raises(ValueError):
        dataset.solve_tours([(np.ones((5, 5)), -np.ones((5, 5)))])
    with pytest.raises(ValueError):
        dataset.solve_tours([(np.ones((5, 5)), np.ones((5, 5)))], restarts=17)
    with pytest.raises(ValueError):
        dataset.solve_tours([(np.ones((5, 5)), np.ones((5, 5)))], init_tours=[[0, 1, 2, 3, 3]])


def _search(n_inst, n_max, restarts, kicks, W=16):
    p = ctypes.c_void_p(16)
    return (ctypes.c_void_p(W), p, p, None, p, None, n_inst, n_max, restarts, kicks, 0, p, p, None)


def _knn(n_inst, n_max, restarts, kicks, neighbors):
    p = ctypes.c_void_p(16)
    return (p, p, p, None, p, None, n_inst, n_max, restarts, kicks, neighbors, 0, p, p, None)


def _cand(n_inst, n_max, restarts, kicks, columns, W=16, cand=16):
    p = ctypes.c_void_p(16)
    return (ctypes.c_void_p(W), p, p, None, p, None, ctypes.c_void_p(cand), p, n_inst, n_max, restarts, kicks, columns, 0,
            p, p, None)


def _bound(n_inst, n_max, iters, W=16):
    p = ctypes.c_void_p(16)
    return (ctypes.c_void_p(W), p, p, p, n_inst, n_max, iters, p, None)


# Two arguments wrong at once: which one an entry point names is the order of its checks.  Codes and messages as the
# library gave them before the entry points shared check_layout (csrc/tour_common.h).
TWO_FAULTS = [
    ("tspgnn_tour_search", _search(4, 129, 0, 8), -2, "tour_search: n_max=129 exceeds 128"),
    ("tspgnn_tour_search", _search(4, 3, 17, 8), -1, "tour_search: n_max=3 must be at least 4"),
    ("tspgnn_tour_search", _search(4, 20, 17, -1), -1, "tour_search: restarts=17 not in [1, 16]"),
    ("tspgnn_tour_search", _search(-1, 129, 4, 8, W=0), -1, "tour_search: n_inst=-1"),
    ("tspgnn_tour_search", _search(4, 20, 4, -1, W=0), -1, "tour_search: kicks=-1"),
    ("tspgnn_tour_search_tri", _search(4, 257, 0, 8), -2, "tour_search_tri: n_max=257 exceeds 256"),
    ("tspgnn_tour_search_tri", _search(4, 256, 11, -1), -1,
     "tour_search_tri: restarts=11: at n_max=256 at most 10 chains fit in LDS"),
    ("tspgnn_tour_search_tri", _search(4, 3, 0, -1), -1, "tour_search_tri: n_max=3 must be at least 4"),
    ("tspgnn_tour_search_knn", _knn(4, 129, 4, 8, 0), -1, "tour_search_knn: neighbors=0 not in [1, 32]"),
    ("tspgnn_tour_search_knn", _knn(4, 129, 0, 8, 8), -2, "tour_search_knn: n_max=129 exceeds 128"),
    ("tspgnn_tour_search_knn", _knn(-1, 20, 4, 8, 33), -1, "tour_search_knn: n_inst=-1"),
    ("tspgnn_tour_search_knn_tri", _knn(4, 3, 4, 8, 33), -1, "tour_search_knn_tri: neighbors=33 not in [1, 32]"),
    ("tspgnn_tour_search_knn_tri", _knn(4, 256, 10, -1, 8), -1,
     "tour_search_knn_tri: restarts=10: at n_max=256 at most 9 chains fit in LDS"),
    ("tspgnn_tour_search_knn_tri", _knn(4, 257, 17, 8, 8), -2, "tour_search_knn_tri: n_max=257 exceeds 256"),
    ("tspgnn_tour_search_cand", _cand(4, 300, 4, 8, 33), -1, "tour_search_cand: columns=33 not in [1, 32]"),
    ("tspgnn_tour_search_cand", _cand(4, 20, 4, -1, 8, cand=0), -1, "tour_search_cand: kicks=-1"),
    ("tspgnn_tour_search_cand", _cand(4, 20, 4, 8, 8, W=0, cand=0), -1, "tour_search_cand: null pointer"),
    ("tspgnn_tour_search_cand_tri", _cand(4, 257, 4, 8, 0), -1, "tour_search_cand_tri: columns=0 not in [1, 32]"),
    ("tspgnn_tour_search_cand_tri", _cand(4, 256, 10, 8, 8, cand=0), -1,
     "tour_search_cand_tri: restarts=10: at n_max=256 at most 9 chains fit in LDS"),
    ("tspgnn_tour_search_cand_tri", _cand(4, 3, 0, 8, 8), -1, "tour_search_cand_tri: n_max=3 must be at least 4"),
    ("tspgnn_tour_lower_bound", _bound(4, 129, 0), -2, "tour_lower_bound: n_max=129 exceeds 128"),
    ("tspgnn_tour_lower_bound", _bound(4, 3, 0), -1, "tour_lower_bound: n_max=3 must be at least 4"),
    ("tspgnn_tour_lower_bound", _bound(4, 20, 0, W=0), -1, "tour_lower_bound: iters=0"),
    ("tspgnn_tour_lower_bound", _bound(-1, 129, 0, W=0), -1, "tour_lower_bound: n_inst=-1"),
    ("tspgnn_tour_lower_bound_tri", _bound(4, 257, 0), -2, "tour_lower_bound_tri: n_max=257 exceeds 256"),
    ("tspgnn_tour_lower_bound_tri", _bound(4, 3, 0, W=0), -1, "tour_lower_bound_tri: n_max=3 must be at least 4"),
    ("tspgnn_tour_lower_bound_tri", _bound(4, 256, 0, W=0), -1, "tour_lower_bound_tri: iters=0"),
]


@pytest.mark.parametrize("entry,args,code,message", TWO_FAULTS, ids=["%s-%d" % (t[0][12:], k) for k, t in enumerate(TWO_FAULTS)])
def test_two_faults_at_once_name_the_first_check(entry, args, code, message):
    assert getattr(_lib.lib, entry)(*args) == code
    assert _lib.lib.tspgnn_last_error().decode() == message
