"""Host side of the vote-guided tour search (tspgnn_vote_neighbors, tspgnn_tour_search_cand / _cand_tri,
label_tours(candidates=), decode_tours(guide=)): the NumPy restatements of tests/guided_reference.py against
knn_search_reference and against rows written out by hand, and every argument check that comes before device work.
No GPU."""
import ctypes

import numpy as np
import pytest

import decode_cases as cases
import guided_reference as gref
import knn_search_reference as ref
import tspgnn
from baseline_reference import euclidean, packed, sparse_planted
from tspgnn import _lib, dataset, decode


def _knn_table(W, K):
    """knn_search_reference.neighbor_sets as a table of exactly K columns: rows padded with the vertex itself."""
    n = W.shape[0]
    N = ref.neighbor_sets(W, K)
    tab = np.repeat(np.arange(n)[:, None], K, axis=1)
    tab[:, :N.shape[1]] = N
    return tab.astype(np.uint8)


def test_pair_mask_from_the_knn_table_is_the_knn_pair_mask():
    rng = np.random.RandomState(70)
    for k, n in enumerate((4, 5, 8, 13, 40)):
        W = packed(*(sparse_planted if k % 2 else euclidean)(rng, n))
        for K in (1, 3, 5, 32):
            assert np.array_equal(gref.pair_mask_from_table(ref.neighbor_sets(W, K), n), ref.pair_mask(W, K))
            assert np.array_equal(gref.pair_mask_from_table(_knn_table(W, K), n), ref.pair_mask(W, K))
    # entries >= n, self entries and duplicates add nothing
    S = gref.pair_mask_from_table(np.array([[1, 1, 9], [1, 5, 255], [2, 2, 2], [0, 3, 4], [4, 4, 4]]), 5)
    assert sorted(map(tuple, np.argwhere(np.triu(S)))) == [(0, 1), (0, 3), (3, 4)]


@pytest.mark.parametrize("n", [8, 40])
def test_chain0_table_with_the_knn_table_is_chain0(n):
    Ma, Mw, init = ref.instance("square", n)
    W = packed(Ma, Mw)
    index = ref.SQUARE_N.index(n)
    for K in (1, 5):
        want = ref.expected("square", n, K)[0]
        got, log = gref.chain0_table(W, _knn_table(W, K), init, max(ref.KICKS), ref.SEED, index)
        assert got == want
        assert log["margin"] >= 1e-3


def test_chain0_table_with_an_empty_set_keeps_the_start():
    Ma, Mw, init = ref.instance("square", 8)
    W = packed(Ma, Mw)
    skip = np.repeat(np.arange(8)[:, None], 3, axis=1)
    tours, log = gref.chain0_table(W, skip, init, 3, ref.SEED, 0)
    assert tours[0] == ref.canonical(init) and "margin" not in log
    costs = [ref.cost32(W, t) for t in tours]
    assert all(b <= a for a, b in zip(costs, costs[1:]))


# ---------------------------------------------------------------------------------------------- vote_rows by hand
def _one(n, edges, w, votes):
    case = cases.batch([(n, np.asarray(edges, dtype=np.int32).reshape(-1, 2), np.asarray(w, dtype=np.float32),
                         np.asarray(votes, dtype=np.float32))])
    return lambda kv, kn: gref.case_rows(case, kv, kn).tolist()


def test_vote_rows_on_a_path_pad_with_the_vertex_itself():
    rows = _one(5, [[0, 1], [1, 2], [2, 3], [3, 4]], [1, 2, 3, 4], [0.5, -1.0, 2.0, 0.0])
    assert rows(2, 0) == [[1, 0], [0, 2], [3, 1], [2, 4], [3, 4]]        # the ends have one neighbour
    assert rows(0, 2) == [[1, 0], [0, 2], [1, 3], [2, 4], [3, 4]]        # by weight
    assert rows(1, 1) == [[1, 0], [0, 2], [3, 1], [2, 4], [3, 4]]        # the near phase takes what the votes left
    assert rows(3, 1) == [[1, 0, 0, 0], [0, 2, 1, 1], [3, 1, 2, 2], [2, 4, 3, 3], [3, 4, 4, 4]]


def test_vote_rows_take_a_multi_edge_pair_from_its_smaller_edge_id():
    # the pair {0, 1} twice: edge 0 (vote -3, weight 9) decides, not edge 3 (vote +9, weight 0.1)
    rows = _one(4, [[0, 1], [0, 2], [0, 3], [1, 0], [1, 2], [2, 3]], [9, 2, 3, 0.1, 1, 1], [-3, 1, 2, 9, 0, 0])
    assert rows(3, 0)[0] == [3, 2, 1] and rows(0, 3)[0] == [2, 3, 1]
    assert rows(2, 0)[1] == [2, 0] and rows(0, 2)[1] == [2, 0]           # seen from vertex 1: the same edge 0


def test_vote_rows_order_special_votes_and_weights():
    inf, nan = np.inf, np.nan
    # the star at vertex 0: leaves 1..5 with votes NaN, -inf, -0.0, +0.0, +inf and weights NaN, +inf, +0.0, -0.0, 1
    star = [[0, 1], [0, 2], [0, 3], [0, 4], [0, 5]]
    rows = _one(6, star, [nan, inf, 0.0, -0.0, 1.0], [nan, -inf, -0.0, 0.0, inf])
    assert rows(5, 0)[0] == [5, 4, 3, 2, 1]          # +inf > +0 > -0 > -inf > NaN
    assert rows(0, 5)[0] == [4, 3, 5, 2, 1]          # -0 < +0 < 1 < +inf < NaN
    assert rows(2, 3)[0] == [5, 4, 3, 2, 1]          # votes take 5 and 4; by weight 3 (+0), then 2 (inf), then 1 (NaN)
    assert rows(1, 1)[3] == [0, 3]                   # a leaf: its one neighbour, then itself


def test_vote_rows_break_equal_votes_by_vertex_id():
    n, uv, w, _ = cases.complete(np.random.RandomState(3), 6)
    rows = _one(n, uv, np.ones(len(uv)), np.full(len(uv), 0.25))
    assert rows(3, 0) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 2]]
    assert rows(1, 2) == rows(3, 0) == rows(0, 3)


def test_vote_rows_ignore_the_order_of_a_csr_row_and_foreign_edges():
    case = cases.odd_case()
    rowptr, eid = gref.vertex_csr(case)
    args = (case["uv"], case["wc"], case["seg"], case["vseg"])
    want = gref.vote_rows(*args, rowptr, eid, case["vote"], 3, 2)
    rev = eid.copy()
    for g in range(len(rowptr) - 1):
        rev[rowptr[g]:rowptr[g + 1]] = eid[rowptr[g]:rowptr[g + 1]][::-1]
    assert np.array_equal(gref.vote_rows(*args, rowptr, rev, case["vote"], 3, 2), want)
    v = case["vseg"]
    assert want[v[0] + 3].tolist() == [3] * 5                             # the vertex no edge touches
    assert (want[v[1]:v[2]] == np.arange(6)[:, None]).all()               # the instance without edges
    assert want[v[2]:v[3]].tolist() == [[1, 0, 0, 0, 0], [0, 1, 1, 1, 1], [2] * 5, [3] * 5]   # only (0, 1) is an edge


# ---------------------------------------------------------------------------------------------- argument checks
def _inst(n):
    return np.triu(np.ones((n, n)), 1), np.ones((n, n))


def _tab(n, K):
    return np.repeat(np.arange(n)[:, None], K, axis=1)


@pytest.mark.parametrize("fn", [dataset.label_tours, dataset.solve_tours])
def test_python_rejects_bad_candidates_before_any_device_work(fn):
    insts = [_inst(6), _inst(8)]
    for bad, match in (([_tab(6, 3)], "one .* per instance"),
                       ([_tab(6, 3), _tab(7, 3)], r"candidates\[1\] has shape"),
                       ([_tab(6, 3).reshape(-1), _tab(8, 3)], r"candidates\[0\] has shape"),
                       ([_tab(6, 0), _tab(8, 0)], "K=0"),
                       ([_tab(6, 33), _tab(8, 33)], "K=33"),
                       ([_tab(6, 3), _tab(8, 4)], "one K for all"),
                       ([_tab(6, 3), _tab(8, 3) + 300], "0..255"),
                       ([_tab(6, 3) - 7, _tab(8, 3)], "0..255"),
                       ([_tab(6, 3) * 0.5, _tab(8, 3)], "integers")):
        with pytest.raises(ValueError, match=match):
            fn(insts, candidates=bad)
    with pytest.raises(ValueError, match="exclusive"):
        fn(insts, candidates=[_tab(6, 3), _tab(8, 3)], neighbors=3)


def test_python_checks_restarts_against_the_budget_of_the_table_width():
    big = [_inst(256)]
    with pytest.raises(ValueError, match="restarts=10: at n=256 at most 9 chains"):
        dataset.label_tours(big, restarts=10, candidates=[_tab(256, 8)])
    with pytest.raises(ValueError, match="restarts=8: at n=256 at most 7 chains"):
        dataset.label_tours(big, candidates=[_tab(256, 32)])


def test_candidates_of_host_solved_instances_are_checked_and_not_used():
    r = dataset.label_tours([_inst(3)], candidates=[_tab(3, 2)], lower_bound=False)
    assert r[0].tour == [0, 1, 2]
    with pytest.raises(ValueError, match="shape"):
        dataset.label_tours([_inst(3)], candidates=[_tab(4, 2)])


def test_decode_tours_rejects_guide_without_polish_and_with_neighbors():
    with pytest.raises(TypeError, match="guide only applies with polish=True"):
        decode.decode_tours(None, None, [], 4, guide=4)
    with pytest.raises(ValueError, match="exclusive"):
        decode.decode_tours(None, None, [], 4, polish=True, guide=(4, 4), neighbors=8)
    for bad in (0, 33, (0, 0), (30, 3), (-1, 4), (4, 4, 4), 2.5, True, "4"):
        with pytest.raises(ValueError, match="guide"):
            decode.decode_tours(None, None, [], 4, polish=True, guide=bad)


def test_entry_points_refuse_bad_arguments_without_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(16)
    for fn, top in ((L.tspgnn_tour_search_cand, 128), (L.tspgnn_tour_search_cand_tri, 256)):
        for bad in (0, -1, 33):
            assert fn(p, p, p, None, p, None, p, p, 4, 20, 4, 8, bad, 0, p, p, None) == -1
            assert b"columns=%d" % bad in L.tspgnn_last_error()
        assert fn(p, p, p, None, p, None, p, p, 4, top + 1, 4, 8, 8, 0, p, p, None) == -2
        assert fn(p, p, p, None, p, None, None, p, 4, 20, 4, 8, 8, 0, p, p, None) == -1
        assert b"null pointer" in L.tspgnn_last_error()
        assert fn(p, p, p, None, p, None, p, None, 4, 20, 4, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, p, p, 4, 20, 17, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, p, p, 4, 3, 4, 8, 8, 0, p, p, None) == -1
        assert fn(p, p, p, None, p, None, p, p, -1, 20, 4, 8, 8, 0, p, p, None) == -1
        assert fn(None, None, None, None, None, None, None, None, 0, 0, 1, 0, 8, 0, None, None, None) == 0
    assert L.tspgnn_tour_search_cand_tri(p, p, p, None, p, None, p, p, 4, 256, 10, 8, 8, 0, p, p, None) == -1
    msg = L.tspgnn_last_error()
    assert b"restarts=10" in msg and b"at most 9" in msg
    f = L.tspgnn_vote_neighbors
    assert f(None, None, None, None, None, None, None, 0, 0, 0, 0, None, None) == 0         # B == 0: a no-op
    assert f(p, p, p, p, p, p, p, 3, 257, 4, 4, p, None) == -2
    for n_max, kv, kn in ((3, 4, 4), (8, -1, 4), (8, 4, -1), (8, 0, 0), (8, 33, 0), (8, 17, 16), (8, 2 ** 31 - 1, 1)):
        assert f(p, p, p, p, p, p, p, 3, n_max, kv, kn, p, None) == -1, (n_max, kv, kn)
    assert f(p, p, p, p, p, p, p, -1, 8, 4, 4, p, None) == -1
    for k in (0, 1, 2, 3, 4, 5, 6, 11):
        args = [p, p, p, p, p, p, p, 3, 8, 4, 4, p, None]
        args[k] = None
        assert f(*args) == -1, k
        assert b"null pointer" in L.tspgnn_last_error()


def test_the_surface_is_exported():
    assert "vote_neighbors" in tspgnn.__all__ and tspgnn.vote_neighbors is decode.vote_neighbors
    assert tspgnn.DecodedTour._fields[-2:] == ("polished_tour", "polished_cost")


@pytest.mark.parametrize("layout,n", [("square", n) for n in ref.SQUARE_N] + [("tri", n) for n in ref.TRI_N])
def test_margin_of_the_gpu_comparison_tables(layout, n):
    """As test_tour_knn_host.py's margin test, for the tables of the arbitrary-table GPU comparison: the restatement's
    fp64 stop rule and the kernel's fp32 one decide alike while |best + thr| / thr stays far above 1e-6."""
    for kind in gref.TABLES:
        tab = gref.table(layout, n, kind)
        assert tab.dtype == np.uint8 and tab.shape[0] == n
        tours, log = gref.expected(layout, n, kind)
        assert log.get("margin", np.inf) >= 1e-3, (kind, log)
        assert len(tours) == max(gref.KICKS) + 1 and all(sorted(t) == list(range(n)) for t in tours)
    S = gref.pair_mask_from_table(gref.table(layout, n, "random"), n)
    assert S.any() and not gref.pair_mask_from_table(gref.table(layout, n, "skip"), n).any()
