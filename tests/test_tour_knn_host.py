"""Host side of the candidate-list tour search (neighbors=K; tspgnn_tour_search_knn / _knn_tri): the NumPy restatement
of tests/knn_search_reference.py against itself, the stop-rule margin of every instance the GPU comparison uses, the LDS
budget, and the argument checks that come before any launch.  No GPU."""
import ctypes

import numpy as np
import pytest

import knn_search_reference as ref
from baseline_reference import euclidean, packed, sparse_planted
from tspgnn import _lib, dataset


def _small(rng, n, kind):
    if kind == "int":   # weights from {1, 2, 3}: deltas tie, so the code decides
        W = np.triu(rng.randint(1, 4, size=(n, n)).astype(np.float64), 1)
        return np.triu(np.ones((n, n)), 1), W + W.T
    return (sparse_planted if kind == "sparse" else euclidean)(rng, n)


def test_neighbor_sets_rank_by_weight_then_id():
    W = np.array([[0, 2, 1, 2, 1], [2, 0, 5, 5, 5], [1, 5, 0, 3, 3], [2, 5, 3, 0, 9], [1, 5, 3, 9, 0]], dtype=np.float32)
    N = ref.neighbor_sets(W, 2)
    assert N.tolist() == [[2, 4], [0, 2], [0, 3], [0, 2], [0, 2]]
    assert ref.neighbor_sets(W, 32).shape == (5, 4)            # K_eff = n - 1
    S = ref.pair_mask(W, 1)
    assert np.array_equal(S, S.T) and not S.diagonal().any()
    assert sorted(map(tuple, np.argwhere(np.triu(S)))) == [(0, 1), (0, 2), (0, 3), (0, 4)]
    assert ref.pair_mask(W, 4)[~np.eye(5, dtype=bool)].all()


def test_full_neighbourhood_restatement_equals_its_unmasked_form():
    rng = np.random.RandomState(50)
    for k, n in enumerate((4, 5, 6, 7, 9, 12, 17, 24, 33)):
        Ma, Mw = _small(rng, n, ("euc", "sparse", "int")[k % 3])
        W = packed(Ma, Mw)
        init = [int(v) for v in rng.permutation(n)]
        masked, _ = ref.chain0(W, n - 1, init, 4, 3, k)
        assert masked == ref.chain0(W, 32, init, 4, 3, k)[0]
        assert masked == ref.chain0(W, None, init, 4, 3, k)[0]


def test_restricted_restatement_finds_permutations_and_never_beats_nothing():
    rng = np.random.RandomState(51)
    for k in range(32):
        n = int(rng.randint(5, 11))
        Ma, Mw = _small(rng, n, ("euc", "sparse", "int")[k % 3])
        W = packed(Ma, Mw)
        init = [int(v) for v in rng.permutation(n)]
        for K in (1, 2, 3):
            tours, log = ref.chain0(W, K, init, 2, 7, k)
            for t in tours:
                assert sorted(t) == list(range(n)) and t[0] == 0 and t[1] < t[-1]
            costs = [ref.cost32(W, t) for t in tours]
            assert costs[-1] <= ref.cost32(W, init) and all(b <= a for a, b in zip(costs, costs[1:]))


def test_scan_masks_by_the_added_edges_only():
    """One tour, K = 1: every candidate the scan keeps adds a pair of S, and a 2-opt move whose added pairs are outside S
    is not kept although the full scan has it."""
    rng = np.random.RandomState(52)
    Ma, Mw = euclidean(rng, 9)
    W = packed(Ma, Mw)
    S = ref.pair_mask(W, 1)
    t = [int(v) for v in rng.permutation(9)]
    full, restricted = ref.scan(W, None, t), ref.scan(W, S, t)
    assert restricted[0] >= full[0]
    code = restricted[1]
    i, j = (code >> 8) & 0xff, code & 0xff
    if not code & ref.OR_OPT:
        assert S[t[i], t[j]] or S[t[i + 1], t[(j + 1) % 9]]
    else:
        L, rv = (code >> 26) & 3, (code >> 29) & 1
        s0, sl, a, b = t[i], t[(i + L - 1) % 9], t[j], t[(j + 1) % 9]
        assert (S[a, sl] or S[s0, b]) if rv else (S[a, s0] or S[sl, b])


@pytest.mark.parametrize("layout,n", [("square", n) for n in ref.SQUARE_N] + [("tri", n) for n in ref.TRI_N])
def test_margin_of_the_gpu_comparison_instances(layout, n):
    """The stop rule compares fp32 quantities on the GPU and an fp64 cost here, about 1e-6 apart: each instance of the
    GPU comparison keeps |best + thr| / thr >= 1e-3 over all its scans, so both sides stop at the same move."""
    for K in ref.KS:
        tours, log = ref.expected(layout, n, K)
        assert log["margin"] >= 1e-3, (K, log)
        assert len(tours) == max(ref.KICKS) + 1 and all(sorted(t) == list(range(n)) for t in tours)


def test_lds_budget_matches_the_kernel():
    fit = dataset.tri_chains_fit
    assert [fit(129, K) for K in (1, 8, 32)] == [16, 16, 16]
    assert [fit(242, K) for K in (1, 8, 32)] == [14, 14, 12]
    assert [fit(256, K) for K in (1, 8, 32)] == [9, 9, 7]
    assert fit(256) == 10 and fit(242) == 16 and fit(256, None) == 10          # unchanged without neighbors
    for n, K in ((129, 8), (242, 8), (242, 32), (256, 1), (256, 8), (256, 32)):
        r = fit(n, K)
        assert 2 * n * (n - 1) + n * K + 13 * r * n <= 163712
        assert r == 16 or 2 * n * (n - 1) + n * K + 13 * (r + 1) * n > 163712
    L = _lib.lib
    p = ctypes.c_void_p(16)
    assert L.tspgnn_tour_search_knn_tri(p, p, p, None, p, None, 4, 256, 10, 8, 8, 0, p, p, None) == -1
    msg = L.tspgnn_last_error()
    assert b"restarts=10" in msg and b"at most 9" in msg
    assert L.tspgnn_tour_search_knn_tri(p, p, p, None, p, None, 4, 256, 8, 8, 32, 0, p, p, None) == -1
    assert b"at most 7" in L.tspgnn_last_error()
    assert L.tspgnn_tour_search_knn_tri(p, p, p, None, p, None, 4, 242, 13, 8, 32, 0, p, p, None) == -1
    assert b"at most 12" in L.tspgnn_last_error()


def test_chains_fit_query_is_the_closed_form():
    """tspgnn_tour_chains_fit against this file's own statement of the budget (above), for every n of both layouts and
    every table width: the weights, n K bytes of table, and per chain 12 n bytes of tours plus n of positions with a
    table, in 163 712 bytes; 16 chains at the most."""
    q = _lib.lib.tspgnn_tour_chains_fit
    for tri, top in ((0, 128), (1, 256)):
        for n in range(4, 257):
            weights = 2 * n * (n - 1) if tri else 4 * n * (n | 1)
            for K in range(0, 33):
                want = min(16, (163712 - weights - n * K) // ((13 if K else 12) * n)) if n <= top else 0
                assert q(tri, n, K) == want, (tri, n, K)
                if want:
                    assert weights + n * K + (13 if K else 12) * want * n <= 163712
        for n, K in ((3, 0), (0, 8), (-1, 0), (top + 1, 0), (top + 1, 8), (20, -1), (20, 33), (top, 33)):
            assert q(tri, n, K) == 0, (tri, n, K)
    assert q(1, 256, 0) == 10 and q(1, 256, 8) == 9 and q(1, 256, 32) == 7 and q(0, 128, 32) == 16
    for n in (129, 200, 242, 243, 256):
        assert dataset.tri_chains_fit(n) == dataset.tri_chains_fit(n, None) == q(1, n, 0)
        for K in (1, 8, 32):
            assert dataset.tri_chains_fit(n, K) == q(1, n, K)


def test_knn_entry_points_reject_bad_arguments_without_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(16)
    for fn, top in ((L.tspgnn_tour_search_knn, 128), (L.tspgnn_tour_search_knn_tri, 256)):
        for bad in (0, -1, 33):
            assert fn(p, p, p, None, p, None, 4, 20, 4, 8, bad, 0, p, p, None) == -1
            assert b"neighbors=%d" % bad in L.tspgnn_last_error()
        assert fn(p, p, p, None, p, None, 4, top + 1, 4, 8, 8, 0, p, p, None) == -2
        assert fn(None, p, p, None, p, None, 4, 20, 4, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, 4, 20, 0, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, 4, 20, 17, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, 4, 20, 4, -1, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, 4, 3, 4, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, -1, 20, 4, 8, 8, 0, p, p, None) == -1
        assert fn(None, None, None, None, None, None, 0, 0, 1, 0, 8, 0, None, None, None) == 0


@pytest.mark.parametrize("bad", [0, 33, 2.5, -3, True, "8"])
def test_python_rejects_bad_neighbors_before_any_launch(bad):
    inst = [(np.triu(np.ones((6, 6)), 1), np.ones((6, 6)))]
    for call in (lambda: dataset.solve_tours(inst, neighbors=bad), lambda: dataset.label_tours(inst, neighbors=bad),
                 lambda: dataset.solve(inst[0][0], inst[0][1], neighbors=bad)):
        with pytest.raises(ValueError, match="neighbors"):
            call()


def test_python_rejects_restarts_over_the_knn_budget_before_any_launch():
    big = [(np.triu(np.ones((256, 256)), 1), np.ones((256, 256)))]
    with pytest.raises(ValueError, match="restarts=10: at n=256 at most 9 chains"):
        dataset.label_tours(big, restarts=10, neighbors=8)
    with pytest.raises(ValueError, match="restarts=8: at n=256 at most 7 chains"):
        dataset.label_tours(big, neighbors=32)              # the n > 128 default of 8 restarts does not fit K = 32
    with pytest.raises(ValueError, match="restarts=11: at n=256 at most 10 chains"):
        dataset.label_tours(big, restarts=11)               # unchanged without neighbors
