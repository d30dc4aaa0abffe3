"""The vote decoder's definition without a GPU: the NumPy restatement (tests/decode_reference.py) against an independent
brute-force enumeration on small complete graphs, the key order stated literally, the equivalence of "arg-max per round"
and "one sorted pass", what the chosen sparse seeds produce, and the entry point's refusals before any launch."""
import functools
import itertools

import numpy as np
import pytest

import decode_cases as cases
import decode_reference as ref
from tspgnn import _lib
from tspgnn.decode import vote_key


def brute_force(n, votes):
    """The greedy on a complete graph, written independently of the restatement: Python floats compared directly (no
    key; the votes here are finite, distinct or tied, never NaN or -0), the fragments kept as explicit vertex lists."""
    edges = list(itertools.combinations(range(n), 2))
    order = sorted(range(len(edges)), key=lambda e: (-float(votes[e]), e))
    frags = [[v] for v in range(n)]
    picked = []
    for e in order:
        a, b = edges[e]
        fa = next(f for f in frags if a in f)
        fb = next(f for f in frags if b in f)
        if fa is fb or a not in (fa[0], fa[-1]) or b not in (fb[0], fb[-1]):
            continue        # a cycle, or an interior vertex (degree 2 already)
        if len(fa) > 1 and fa[0] == a:
            fa.reverse()
        if len(fb) > 1 and fb[-1] == b:
            fb.reverse()
        frags.remove(fb)
        fa.extend(fb)
        picked.append(e)
    return edges, picked, frags


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_restatement_against_brute_force(n):
    rng = np.random.RandomState(n)
    for trial in range(20):
        votes = rng.randn(n * (n - 1) // 2).astype(np.float32)
        if trial % 4 == 3:
            votes = np.round(votes)     # plenty of ties
            votes[votes == 0] = 0.0     # (no -0: brute_force compares floats)
        edges, picked, frags = brute_force(n, votes)
        uv = np.array(edges)
        assert ref.greedy_sorted(n, uv, votes) == picked
        deg = np.bincount(uv[picked].reshape(-1), minlength=n)
        assert deg.max() <= 2 and len(picked) == n - 1      # a Hamiltonian path: no premature cycle
        assert len(frags) == 1
        tour, missing, cost, fragments = ref.decode_instance(n, uv, np.ones(len(uv)), votes)
        assert sorted(tour) == list(range(n))
        assert tour[0] == 0 and tour[1] < tour[-1]
        assert missing == 0 and fragments == 1 and cost == np.float32(n)
        path = frags[0]
        assert tour == ref.canonical(path)


def test_key_order_literally():
    votes = cases.SPECIAL
    # index:   0    1     2    3     4    5      6      7    8    9     10     11    12   13
    # value: +0.0 -0.0  +inf -inf   nan 1e-45 -1e-45   1.0  1.0 -1.0  5e-39  -nan   3.5 -2.0
    key = vote_key(votes)
    assert key.dtype == np.uint32
    assert [int(k) for k in key] == [0x80000000, 0x7FFFFFFF, 0xFF800000, 0x007FFFFF, 0, 0x80000001, 0x7FFFFFFE, 0xBF800000,
                                     0xBF800000, 0x407FFFFF, 0x803671F7, 0, 0xC0600000, 0x3FFFFFFF]
    assert [int(e) for e in ref.edge_order(votes)] == [2, 12, 7, 8, 10, 5, 0, 1, 6, 9, 13, 3, 4, 11]


@pytest.mark.parametrize("seed", range(6))
def test_argmax_per_round_equals_sorted_pass(seed):
    rng = np.random.RandomState(100 + seed)
    n = int(rng.randint(5, 40))
    n, uv, w, votes = cases.sparse_planted(rng, n, rng.uniform(0.1, 0.5))
    if seed % 2:
        votes = cases.SPECIAL[rng.randint(0, len(cases.SPECIAL), size=len(votes))]
    assert ref.greedy_rounds(n, uv, votes) == ref.greedy_sorted(n, uv, votes)
    assert ref.decode_instance(n, uv, w, votes, rounds=True)[:2] == ref.decode_instance(n, uv, w, votes)[:2]


@functools.lru_cache(maxsize=None)
def sparse_results():
    return ref.decode_batch(cases.sparse_case())


def test_the_sparse_seeds_strand():
    """What decode_cases.SPARSE_OUTCOME records: the chosen seeds leave several paths on three instances and one
    unclosed Hamiltonian path on the fourth; every stitched tour needs pairs that are no edges."""
    got = tuple((missing, fragments) for _, missing, _, fragments in sparse_results())
    assert got == cases.SPARSE_OUTCOME == ((2, 2), (1, 1), (6, 6), (7, 7))
    for (tour, _, _, _), n in zip(sparse_results(), cases.sparse_case()["n"]):
        assert sorted(tour) == list(range(n)) and tour[0] == 0 and tour[1] < tour[-1]


def test_odd_instances():
    lonely, empty, junk, multi = ref.decode_batch(cases.odd_case())
    assert lonely[1] == 2 and lonely[3] == 2            # vertex 3 is a path of its own: two pairs without an edge
    assert empty[0] == list(range(6)) and empty[1] == 6 and empty[2] == 0 and empty[3] == 6
    assert junk[0] == [0, 1, 2, 3] and junk[1] == 3     # only (0, 1) is an edge
    assert multi[1] == 0 and multi[3] == 1


def test_the_surface_is_exported():
    import tspgnn
    for name in ("tours_from_votes", "decode_tours", "DecodedBatch", "DecodedTour"):
        assert name in tspgnn.__all__ and getattr(tspgnn, name) is getattr(tspgnn.decode, name)
    assert callable(tspgnn.experiments.decoded_tour_curve)
    assert tspgnn.DecodedTour._fields == ("tour", "cost", "n_missing", "feasible", "prediction", "target_cost",
                                          "polished_tour", "polished_cost")


def test_refusals_before_any_launch():
    f = _lib.lib.tspgnn_tour_from_votes
    p = 64      # never dereferenced: the call returns before a launch
    assert f(None, None, None, None, None, 0, 0, None, None, None, None) == 0          # B == 0: a no-op
    assert f(p, p, p, p, p, 3, 257, p, p, p, None) == -2
    assert b"257" in _lib.lib.tspgnn_last_error()
    assert f(p, p, p, p, p, 3, 3, p, p, p, None) == -1
    assert f(p, p, p, p, p, -1, 8, p, p, p, None) == -1
    for k in (0, 1, 2, 3, 4, 7, 8, 9):
        args = [p, p, p, p, p, 3, 8, p, p, p, None]
        args[k] = None
        assert f(*args) == -1, k
        assert b"null pointer" in _lib.lib.tspgnn_last_error()
