"""The beam decoder's definition without a GPU: the NumPy restatement (tests/beam_reference.py) against an independently
written walk at beam = 1 and a brute force over all cycles at an exhaustive beam, what the sparse seeds produce, q(v) on
the special votes, and the entry points' refusals before any launch."""
import functools
import itertools

import numpy as np
import pytest

import beam_cases as bc
import beam_reference as ref
import decode_cases as cases
from tspgnn import _lib


def instance_of(case, b):
    e0, e1 = case["seg"][b], case["seg"][b + 1]
    return int(case["n"][b]), case["uv"][e0:e1] - case["vseg"][b], case["wc"][e0:e1, 0], slice(e0, e1)


def walk(n, uv, score):
    """beam = 1 written on its own: from vertex 0 to the unvisited neighbour of best clamped score (the smallest edge id
    of a pair speaks for it), ties to the smaller vertex, until no neighbour is left; then the rest in ascending id."""
    first = {}
    for e, (a, b) in enumerate(np.asarray(uv).tolist()):
        if 0 <= a < n and 0 <= b < n and a != b:
            first.setdefault((min(a, b), max(a, b)), e)
    path, total = [0], 0
    while len(path) < n:
        best = None
        for u in range(n):
            e = first.get((min(path[-1], u), max(path[-1], u)))
            if u in path or e is None:
                continue
            q = min(max(int(score[e]), -(1 << 22)), 0)
            if best is None or q > best[0]:
                best = (q, u)
        if best is None:
            return path + [u for u in range(n) if u not in path], total, True
        total += best[0]
        path.append(best[1])
    e = first.get((0, path[-1]))
    if e is not None:
        total += min(max(int(score[e]), -(1 << 22)), 0)
    return path, total, False


@pytest.mark.parametrize("name", ["sparse_case", "ragged_case", "odd_case", "ties_case", "special_case"])
def test_beam_one_is_the_best_neighbour_walk(name):
    case, scores = getattr(cases, name)(), bc.scores_of(name)
    for b in range(len(case["n"])):
        n, uv, w, sl = instance_of(case, b)
        path, total, stranded = walk(n, uv, scores[sl])
        got = ref.beam_instance(n, uv, w, scores[sl], 1, "score")
        assert got["tour"] == ref.canonical(path) and got["score"] == total
        assert (got["stranded"] is not None) == stranded
        assert ref.beam_instance(n, uv, w, scores[sl], 1, "cost") == got      # one entry: nothing to choose


@functools.lru_cache(maxsize=None)
def brute_force_cycles():
    """[(fp32 cost, canonical tour)] of all 360 cycles of the exhaustive case, cheapest first."""
    case = bc.exhaustive_case()
    n, uv, w, _ = instance_of(case, 0)
    W = np.zeros((n, n), dtype=np.float32)
    W[uv[:, 0], uv[:, 1]] = w
    W += W.T
    out = []
    for perm in itertools.permutations(range(1, n)):
        if perm[0] > perm[-1]:
            continue
        tour = [0] + list(perm)
        c = np.float32(0)
        for a, b in zip(tour, tour[1:] + tour[:1]):
            c = np.float32(c + W[a, b])
        out.append((c, tour))
    return sorted(out, key=lambda x: x[0])


def test_an_exhaustive_beam_returns_the_brute_force_optimum():
    cycles = brute_force_cycles()
    assert len(cycles) == 360
    assert cycles[0][0] == bc.EXHAUSTIVE_COST and cycles[0][1] == bc.EXHAUSTIVE_TOUR
    assert cycles[1][0] == bc.EXHAUSTIVE_RUNNER_UP > cycles[0][0]                            # the optimum is unique
    case = bc.exhaustive_case()
    n, uv, w, sl = instance_of(case, 0)
    scores = ref.q_scores(case["vote"])
    a, b = (ref.beam_instance(n, uv, w, scores, beam, "cost") for beam in (720, 1024))
    assert a == b
    assert a["tour"] == bc.EXHAUSTIVE_TOUR and a["cost"] == bc.EXHAUSTIVE_COST and a["n_closed"] == 720
    assert a["n_missing"] == 0 and a["stranded"] is None
    by_score = [ref.beam_instance(n, uv, w, scores, beam, "score") for beam in (720, 1024)]
    assert by_score[0] == by_score[1] and by_score[0]["n_closed"] == 720
    # the best score over all Hamiltonian paths closed, found independently
    Q = np.zeros((n, n), dtype=np.int64)
    Q[uv[:, 0], uv[:, 1]] = scores
    Q += Q.T
    best = max(sum(int(Q[x, y]) for x, y in zip((0,) + p, p + (0,))) for p in itertools.permutations(range(1, n)))
    assert by_score[0]["score"] == best


# (stranded at step, n_closed, n_missing) per graph of decode_cases.SPARSE, per beam of bc.SPARSE_BEAMS
SPARSE_BEAM_OUTCOME = (((6, 0, 6), (27, 0, 3), (55, 0, 13), (110, 0, 18)),
                       ((9, 0, 2), (26, 0, 4), (57, 0, 11), (116, 0, 14)),
                       ((None, 10, 0), (27, 0, 3), (62, 0, 7), (120, 0, 9)))


def test_the_sparse_seeds_under_the_beam():
    case, scores = cases.sparse_case(), bc.scores_of("sparse_case")
    stranded = 0
    for beam, want in zip(bc.SPARSE_BEAMS, SPARSE_BEAM_OUTCOME):
        for select in ("score", "cost"):
            got = ref.beam_batch(case, scores, beam, select)
            assert tuple((r["stranded"], r["n_closed"], r["n_missing"]) for r in got) == want
            for r, n in zip(got, case["n"]):
                assert sorted(r["tour"]) == list(range(n)) and r["tour"][0] == 0 and r["tour"][1] < r["tour"][-1]
                if r["stranded"] is not None:
                    assert r["stranded"] < n - 1
                    stranded += select == "score"
    assert stranded == 11


def test_scores_of_the_special_votes():
    # index:   0    1     2    3     4    5      6      7    8    9     10     11    12   13
    # value: +0.0 -0.0  +inf -inf   nan 1e-45 -1e-45   1.0  1.0 -1.0  5e-39  -nan   3.5 -2.0
    q = ref.q_scores(cases.SPECIAL)
    assert q.dtype == np.int32
    half = int(np.rint(65536.0 * np.log(0.5)))        # logsigmoid(0) = -log 2: -45426
    assert half == -45426
    assert [int(x) for x in q] == [half, half, 0, -(1 << 22), -(1 << 22), half, half, -20530, -20530, -86066, half,
                                   -(1 << 22), -1950, -139390]
    votes = np.sort(np.concatenate([np.random.RandomState(3).randn(20000).astype(np.float32) * 30,
                                    cases.SPECIAL[np.isfinite(cases.SPECIAL)]]))
    q = ref.q_scores(votes)
    assert (np.diff(q.astype(np.int64)) >= 0).all()
    assert q.min() == -(1 << 22) and q.max() == 0      # both clamps are reached: logsigmoid(-64) < -64
    assert np.array_equal(ref.q_scores_second(cases.SPECIAL), ref.q_scores(cases.SPECIAL))


def test_the_surface_is_exported():
    import tspgnn
    for name in ("edge_scores", "beam_tours", "BeamBatch", "BeamTour", "decode_tours"):
        assert name in tspgnn.__all__ and getattr(tspgnn, name) is getattr(tspgnn.decode, name)
    assert tspgnn.BeamTour._fields == tspgnn.DecodedTour._fields + ("score", "n_closed")
    assert tspgnn.BeamBatch._fields == ("tours", "costs", "n_missing", "scores", "n_closed", "vseg")
    assert tspgnn.decode.DEFAULT_BEAM_WORKSPACE_BYTES == 256 << 20


def test_workspace_query_and_refusals_before_any_launch():
    ws = _lib.lib.tspgnn_tour_beam_workspace_bytes
    assert ws(1, 256, 1024) == 2 * 256 * 256 * 4 + 256 * 1024 * 4 + 256 * 1024
    assert ws(3, 40, 7) == 3 * ws(1, 40, 7) and ws(1, 40, 7) % 16 == 0 and ws(1, 40, 7) >= 2 * 40 * 40 * 4 + 5 * 40 * 7
    assert ws(0, 40, 7) == ws(1, 257, 7) == ws(1, 3, 7) == ws(1, 40, 0) == ws(1, 40, 1025) == 0
    f = _lib.lib.tspgnn_tour_beam
    p, big = 64, 1 << 40      # never dereferenced: the call returns before a launch
    args = [p, p, p, p, p, 3, 8, 4, 0, p, big, p, p, p, p, p, None]
    assert f(None, None, None, None, None, 0, 0, 0, 7, None, 0, None, None, None, None, None, None) == 0   # B == 0
    for at, value, code, word in ((6, 257, -2, b"257"), (7, 1025, -2, b"1025"), (6, 3, -1, b"n_max"), (7, 0, -1, b"beam"),
                                  (8, 2, -1, b"select"), (8, -1, -1, b"select"), (5, -1, -1, b"B=-1"),
                                  (10, ws(3, 8, 4) - 1, -1, b"workspace"), (9, 72, -1, b"aligned")):
        bad = list(args)
        bad[at] = value
        assert f(*bad) == code, (at, value)
        assert word in _lib.lib.tspgnn_last_error(), (at, value, _lib.lib.tspgnn_last_error())
    for k in (0, 1, 2, 3, 4, 9, 11, 12, 13, 14, 15):
        bad = list(args)
        bad[k] = None
        assert f(*bad) == -1, k
        assert b"null pointer" in _lib.lib.tspgnn_last_error()
    g = _lib.lib.tspgnn_vote_scores_i32
    assert g(None, 0, None, None) == 0
    assert g(p, -1, p, None) == -1 and g(None, 5, p, None) == -1 and g(p, 5, None, None) == -1
