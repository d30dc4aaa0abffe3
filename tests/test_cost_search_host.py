"""Batched tour-cost search (tspgnn.get_costs) without a GPU: the C entry point's argument validation answers before
any launch, and the chunk planner keeps instances in order, never splits an instance's probe copies and respects
max_graphs."""
import ctypes

import pytest

import tspgnn
from tspgnn import _lib
from tspgnn.binary_search import DEFAULT_MAX_GRAPHS, plan_chunks

_FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: validation rejects the call before any launch


def _step(n_inst, k, mode, ptrs=None, pred=_FAKE):
    p = [_FAKE] * 8 if ptrs is None else ptrs
    lo, hi, iters, pred_out, n_active, WC, seg, guard = p
    return _lib.lib.tspgnn_cost_search_step(lo, hi, iters, pred_out, n_active, pred, WC, seg, guard, n_inst, k, 0.5,
                                            0.01, mode, None)


def test_no_instances_is_a_no_op():
    assert _step(0, 1, 1, ptrs=[None] * 8, pred=None) == 0
    assert _step(0, 0, 7, ptrs=[None] * 8, pred=None) == 0


@pytest.mark.parametrize("k", [0, -3])
def test_k_below_one_is_rejected(k):
    assert _step(4, k, 1) == -1
    assert b"k=%d" % k in _lib.lib.tspgnn_last_error()


@pytest.mark.parametrize("mode", [-1, 2, 9])
def test_bad_mode_is_rejected(mode):
    assert _step(4, 2, mode) == -1
    assert b"mode=%d" % mode in _lib.lib.tspgnn_last_error()


@pytest.mark.parametrize("which", range(8))
def test_null_state_pointers_are_rejected(which):
    ptrs = [_FAKE] * 8
    ptrs[which] = None
    for mode in (0, 1):
        assert _step(5, 3, mode, ptrs=ptrs) == -1
        assert b"null pointer" in _lib.lib.tspgnn_last_error()


def test_predictions_are_required_by_a_step_only():
    assert _step(5, 3, 1, pred=None) == -1
    assert b"null pointer" in _lib.lib.tspgnn_last_error()
    with pytest.raises(_lib.TspgnnError) as e:
        _lib.call("tspgnn_cost_search_step", *([_FAKE] * 5), None, *([_FAKE] * 3), 5, 3, 0.5, 0.01, 1, None)
    assert e.value.status == -1


def test_negative_instance_count_is_rejected():
    assert _step(-1, 1, 0) == -1
    assert b"n_inst=-1" in _lib.lib.tspgnn_last_error()


@pytest.mark.parametrize("n,k,max_graphs", [(1, 1, 1), (7, 1, 3), (512, 8, 1024), (513, 1, 1024), (24, 4, 32),
                                            (10, 3, 10), (100, 7, 50), (3, 5, 5)])
def test_chunk_plan(n, k, max_graphs):
    plan = plan_chunks(n, k, max_graphs)
    assert plan[0][0] == 0 and plan[-1][1] == n
    for (a, b), (c, _) in zip(plan, plan[1:]):
        assert b == c                               # in order, contiguous, nothing dropped or repeated
    sizes = [b - a for a, b in plan]
    assert all(s >= 1 and s * k <= max_graphs for s in sizes)
    assert max(sizes) - min(sizes) <= 1                 # balanced
    assert len(plan) == -(-n // (max_graphs // k))  # no more chunks than whole instances per chunk force


def test_chunk_plan_edges():
    assert plan_chunks(0, 4) == []
    assert plan_chunks(512, 8) == [(0, 128), (128, 256), (256, 384), (384, 512)]
    assert plan_chunks(5, 1, DEFAULT_MAX_GRAPHS) == [(0, 5)]
    with pytest.raises(ValueError):
        plan_chunks(4, 9, 8)                        # one instance's copies do not fit
    with pytest.raises(ValueError):
        plan_chunks(4, 0, 8)


def test_get_costs_is_exported():
    assert tspgnn.get_costs is tspgnn.binary_search.get_costs
    assert "get_costs" in tspgnn.__all__


def test_get_costs_refuses_a_plumbing_session():
    model = tspgnn.build_network(32)
    sess = tspgnn.Session(model, device="cpu")
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        tspgnn.get_costs(sess, model, [tspgnn.random_instance(5, __import__("numpy").random.RandomState(0))], 2)
