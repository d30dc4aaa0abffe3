"""Host side of the decision-TSP baselines: the argument checks of the four tspgnn_tour_nearest_neighbor / _anneal entry
points, the limits tspgnn.baselines enforces before anything is launched, ``decide`` and the curve arithmetic, and the
tests' own reference of the two algorithms.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import baseline_reference as ref
from tspgnn import _lib, baselines, dataset, experiments
from tspgnn.dataset import TourResult


def test_entry_points_reject_bad_arguments_without_gpu():
    L = _lib.lib
    p = ctypes.c_void_p(16)
    for sfx, cap in (("", 128), ("_tri", 256)):
        nn = getattr(L, "tspgnn_tour_nearest_neighbor" + sfx)
        sa = getattr(L, "tspgnn_tour_anneal" + sfx)
        # n_max beyond the layout: EUNSUPPORTED, with the limit in the message
        assert nn(p, p, p, p, 4, cap + 1, 0, p, p, None) == -2
        assert str(cap).encode() in L.tspgnn_last_error()
        assert sa(p, p, p, None, p, None, p, p, 4, cap + 1, 4, 8, 0, p, p, None) == -2
        assert str(cap).encode() in L.tspgnn_last_error()
        # n_max below 4, negative counts, a start below -1: EINVAL
        assert nn(p, p, p, p, 4, 3, 0, p, p, None) == -1
        assert b"at least 4" in L.tspgnn_last_error()
        assert sa(p, p, p, None, p, None, p, p, 4, 3, 4, 8, 0, p, p, None) == -1
        assert nn(p, p, p, p, -1, 20, 0, p, p, None) == -1
        assert sa(p, p, p, None, p, None, p, p, -1, 20, 4, 8, 0, p, p, None) == -1
        assert nn(p, p, p, p, 4, 20, -2, p, p, None) == -1
        assert sa(p, p, p, None, p, None, p, p, 4, 20, 4, -1, 0, p, p, None) == -1
        # chains 0 and 17
        assert sa(p, p, p, None, p, None, p, p, 4, 20, 0, 8, 0, p, p, None) == -1
        assert sa(p, p, p, None, p, None, p, p, 4, 20, 17, 8, 0, p, p, None) == -1
        assert b"chains=17" in L.tspgnn_last_error() and b"16" in L.tspgnn_last_error()
        # null pointers: each required one in turn
        for k in range(6):
            a = [p] * 6
            a[k] = None
            assert nn(a[0], a[1], a[2], a[3], 4, 20, 0, a[4], a[5], None) == -1
            assert b"null pointer" in L.tspgnn_last_error()
        for k in range(8):
            a = [p] * 8
            a[k] = None
            assert sa(a[0], a[1], a[2], None, a[3], None, a[4], a[5], 4, 20, 4, 8, 0, a[6], a[7], None) == -1
            assert b"null pointer" in L.tspgnn_last_error()
        # empty batches are a no-op
        assert nn(None, None, None, None, 0, 0, 0, None, None, None) == 0
        assert sa(None, None, None, None, None, None, None, None, 0, 0, 1, 0, 0, None, None, None) == 0
    # chains over the LDS budget: 10 fit at n_max = 256, 16 at n_max = 242 (the rule of tspgnn_tour_search_tri)
    assert L.tspgnn_tour_anneal_tri(p, p, p, None, p, None, p, p, 4, 256, 11, 8, 0, p, p, None) == -1
    msg = L.tspgnn_last_error()
    assert b"chains=11" in msg and b"at most 10" in msg
    assert L.tspgnn_tour_anneal_tri(p, p, p, None, p, None, p, p, 4, 243, 16, 8, 0, p, p, None) == -1


def _inst(n, seed=0):
    return ref.euclidean(np.random.RandomState(seed), n)


def test_baselines_raise_before_any_launch():
    """None of these reaches a kernel: on a machine without a GPU a launch would fail with another error."""
    ok = _inst(5)
    big = (np.ones((257, 257)), np.ones((257, 257)))
    with pytest.raises(ValueError, match="instance 1: n=257 .* 256"):
        baselines.nearest_neighbor_tours([ok, big])
    with pytest.raises(ValueError, match="instance 1: n=257 .* 256"):
        baselines.anneal_tours([ok, big])
    for bad in (dict(chains=0), dict(chains=17), dict(chunk=0), dict(levels=-1), dict(sweeps=-1), dict(sweeps=float("nan")),
                dict(t_hot=-0.1), dict(t_hot=float("nan")), dict(t_cold=float("nan")), dict(t_cold=-1.0),
                dict(t_hot=0.01, t_cold=0.1), dict(t_cold=0.0), dict(t_hot=float("inf")),
                dict(inv_temp=[1.0, -1.0]), dict(inv_temp=[1.0, float("nan")]), dict(inv_temp=np.ones((2, 3))),
                dict(per_level=-1), dict(per_level=[1, 2]), dict(index=[0, 1]), dict(index=[-1]),
                dict(init_tours=[[0, 1, 2, 3, 3]]), dict(init_tours=[None, None])):
        with pytest.raises(ValueError):
            baselines.anneal_tours([ok], **bad)
    # the proposal budget: levels * per_level may not pass 2^31 - 1
    with pytest.raises(ValueError, match="2147483647"):
        baselines.anneal_tours([ok], levels=2 ** 11, per_level=2 ** 20)
    with pytest.raises(ValueError, match="2147483647"):
        baselines.anneal_tours([ok], inv_temp=np.ones(2 ** 12), per_level=2 ** 19)
    with pytest.raises(ValueError, match="2147483647"):
        baselines.anneal_tours([_inst(256)], levels=2 ** 10, sweeps=32)
    # chains that do not fit at the largest n
    with pytest.raises(ValueError, match="at most 10 chains"):
        baselines.anneal_tours([_inst(256)], chains=11)
    for bad in ("worst", -1, 1.5, 2 ** 31):
        with pytest.raises(ValueError):
            baselines.nearest_neighbor_tours([ok], start=bad)
    with pytest.raises(ValueError):
        baselines.nearest_neighbor_tours([ok], chunk=0)
    # n < 4 is solved on the host, with no device needed, and lb is nan
    Ma = np.array([[0, 1, 1], [0, 0, 1], [0, 0, 0]])
    Mw = np.array([[0, 0.5, 0.25], [0.5, 0, 0.125], [0.25, 0.125, 0]])
    want = dataset.label_tours([(Ma, Mw)])[0]
    for r in (baselines.nearest_neighbor_tours([(Ma, Mw)])[0], baselines.anneal_tours([(Ma, Mw)])[0],
              baselines.nearest_neighbor_tours([(Ma, Mw)], start="best")[0]):
        assert (r.tour, r.cost, r.feasible, r.target) == (want.tour, want.cost, want.feasible, want.target)
        assert np.isnan(r.lb)
    assert baselines.anneal_tours([]) == [] and baselines.nearest_neighbor_tours([]) == []


def test_geometric_schedule():
    t = baselines.geometric_schedule(5, 0.4, 0.025)
    assert t[0] == 0.4 and abs(t[-1] - 0.025) < 1e-15
    assert np.allclose(t[1:] / t[:-1], 0.5)
    assert list(baselines.geometric_schedule(1, 0.3, 0.1)) == [0.3]
    assert list(baselines.geometric_schedule(3, 0.0, 0.0)) == [0.0, 0.0, 0.0]
    assert baselines.geometric_schedule(0, 0.3, 0.1).shape == (0,)


def test_decide_and_curve_arithmetic():
    nan = float("nan")
    res = [TourResult([0, 1, 2, 3], 10.0, nan, True, 9.0), TourResult([0, 1, 2, 3], 10.0, nan, False, 9.0),
           TourResult([0, 2, 1, 3], 4.0, nan, True, 4.0), TourResult([0, 1, 3, 2], 7.0, nan, True, 8.0)]
    assert list(baselines.decide(res, [10.0, 10.0, 3.999, 7.0])) == [True, False, False, True]
    assert list(baselines.decide(res, 9.0)) == [False, False, True, True]
    assert baselines.decide(res, [r.target for r in res]).dtype == np.bool_
    assert baselines.decide([], []).shape == (0,)
    # costs 10 / 10 (infeasible) / 4 / 7 against Q = 9 / 9 / 4 / 8
    c = experiments.curve_from_costs([r.cost for r in res], [r.feasible for r in res], [r.target for r in res],
                                     [0.0, 0.1, 0.2, 0.5])
    #   dev 0: yes at (1+0)Q for instances 2, 3 -> tpr 1/2; the (1-0)Q copies get the same answers -> fpr 1/2
    #   dev 0.1: (1.1 Q = 9.9, 9.9, 4.4, 8.8) -> 2, 3 -> 1/2; (0.9 Q = 8.1, 8.1, 3.6, 7.2) -> 3 -> 1/4
    #   dev 0.2: (10.8, ., 4.8, 9.6) -> 0, 2, 3 -> 3/4; (7.2, ., 3.2, 6.4) -> none -> 0
    assert list(c["tpr"]) == [0.5, 0.5, 0.75, 0.75]
    assert list(c["fpr"]) == [0.5, 0.25, 0.0, 0.0]
    assert list(c["acc"]) == [0.5, 0.625, 0.875, 0.875]
    with pytest.raises(ValueError, match="method"):
        experiments.baseline_curve([], [0.02], method="ils")


def test_reference_generator_and_nearest_neighbour():
    """The tests' own reference: splitmix64's published first outputs, and nearest neighbour against a plain loop."""
    # splitmix64 from state 0: the finaliser applied to the first increment
    assert ref.mix64(0) == 0xE220A8397B1DCDAF
    assert ref.draw(1, 2, 3, 4, 0) != ref.draw(1, 2, 3, 5, 0) != ref.draw(1, 2, 4, 4, 0)
    rng = np.random.RandomState(3)
    for make, n in itertools.product((ref.euclidean, ref.grid, ref.sparse_planted), (4, 9, 70)):
        W = ref.packed(*make(rng, n))
        for s in (0, n - 1):
            t, seen = [s], {s}
            while len(t) < n:
                cand = [(W[t[-1], v], v) for v in range(n) if v not in seen]
                t.append(min(cand)[1])
                seen.add(t[-1])
            assert ref.nn_tour(W, s) == t
        assert [list(x) for x in ref.nn_tours(W, [0, n - 1])] == [ref.nn_tour(W, 0), ref.nn_tour(W, n - 1)]
    assert ref.canonical([2, 0, 3, 1]) == [0, 2, 1, 3] and ref.canonical([3, 0, 1, 2]) == [0, 1, 2, 3]


def test_reference_chain_at_zero_temperature_is_a_descent():
    rng = np.random.RandomState(4)
    W = ref.packed(*ref.euclidean(rng, 12))
    start = ref.nn_tour(W, 0)
    best, near = ref.chain(W, start, 1, 0, 0, np.array([np.inf], dtype=np.float32), 3000)
    assert near == 0 and sorted(best) == list(range(12))
    assert ref.cost64(W, best) <= ref.cost64(W, start)
    # no budget: the start itself
    assert ref.chain(W, start, 1, 0, 0, np.zeros(0, dtype=np.float32), 100)[0] == start


def _nn(n_inst, n_max, start, W=16):
    p = ctypes.c_void_p(16)
    return (ctypes.c_void_p(W), p, p, p, n_inst, n_max, start, p, p, None)


def _sa(n_inst, n_max, chains, levels, W=16):
    p = ctypes.c_void_p(16)
    return (ctypes.c_void_p(W), p, p, None, p, None, p, p, n_inst, n_max, chains, levels, 0, p, p, None)


# Two arguments wrong at once: which one an entry point names is the order of its checks.  Codes and messages as the
# library gave them before check_layout moved to csrc/tour_common.h.
TWO_FAULTS = [
    ("tspgnn_tour_nearest_neighbor", _nn(4, 129, -2), -2, "tour_nearest_neighbor: n_max=129 exceeds 128"),
    ("tspgnn_tour_nearest_neighbor", _nn(4, 3, -2), -1, "tour_nearest_neighbor: n_max=3 must be at least 4"),
    ("tspgnn_tour_nearest_neighbor", _nn(4, 20, -2, W=0), -1,
     "tour_nearest_neighbor: start=-2 must be a vertex (>= 0) or -1 for every start"),
    ("tspgnn_tour_nearest_neighbor", _nn(-1, 0, -2, W=0), -1, "tour_nearest_neighbor: n_inst=-1"),
    ("tspgnn_tour_nearest_neighbor_tri", _nn(4, 257, -2, W=0), -2, "tour_nearest_neighbor_tri: n_max=257 exceeds 256"),
    ("tspgnn_tour_nearest_neighbor_tri", _nn(4, 256, -5, W=0), -1,
     "tour_nearest_neighbor_tri: start=-5 must be a vertex (>= 0) or -1 for every start"),
    ("tspgnn_tour_anneal", _sa(4, 129, 0, -1), -2, "tour_anneal: n_max=129 exceeds 128"),
    ("tspgnn_tour_anneal", _sa(4, 3, 17, -1), -1, "tour_anneal: n_max=3 must be at least 4"),
    ("tspgnn_tour_anneal", _sa(4, 20, 17, -1), -1, "tour_anneal: chains=17 not in [1, 16]"),
    ("tspgnn_tour_anneal", _sa(4, 20, 4, -1, W=0), -1, "tour_anneal: levels=-1"),
    ("tspgnn_tour_anneal", _sa(-1, 129, 0, -1, W=0), -1, "tour_anneal: n_inst=-1"),
    ("tspgnn_tour_anneal_tri", _sa(4, 257, 0, -1), -2, "tour_anneal_tri: n_max=257 exceeds 256"),
    ("tspgnn_tour_anneal_tri", _sa(4, 256, 11, -1), -1, "tour_anneal_tri: chains=11: at n_max=256 at most 10 chains fit in LDS"),
    ("tspgnn_tour_anneal_tri", _sa(4, 256, 17, -1, W=0), -1, "tour_anneal_tri: chains=17 not in [1, 16]"),
]


@pytest.mark.parametrize("entry,args,code,message", TWO_FAULTS, ids=["%s-%d" % (t[0][12:], k) for k, t in enumerate(TWO_FAULTS)])
def test_two_faults_at_once_name_the_first_check(entry, args, code, message):
    assert getattr(_lib.lib, entry)(*args) == code
    assert _lib.lib.tspgnn_last_error().decode() == message
