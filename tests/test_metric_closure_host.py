"""Host side of the device metric closure (tspgnn.metric_closure, closure='host' | 'device'; tspgnn_metric_closure,
csrc/tour_closure.hip): the argument checks that come before any launch, in Python and in the C entry point, and the
paths on which closure= changes nothing.  No GPU."""
import ctypes
import random

import numpy as np
import pytest

import tspgnn
from tspgnn import _lib, dataset


@pytest.fixture
def no_launch(monkeypatch):
    """Any call into the library's launch path, or any look at the device, fails the test."""
    def boom(*a, **k):
        raise AssertionError("reached the launch path")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "current_stream", boom)


def test_limits_and_export():
    assert dataset.CLOSURE_MAX_N == 256
    L = dataset.CLOSURE_LDS_MAX_N
    assert 8 * L * L <= 160 * 1024 < 8 * (L + 1) * (L + 1)      # kLdsBytes: the whole fp64 matrix in LDS
    assert tspgnn.metric_closure is dataset.metric_closure and "metric_closure" in tspgnn.__all__


def test_bogus_closure_raises_on_all_three(tmp_path, no_launch):
    with pytest.raises(ValueError, match="closure"):
        dataset.create_graph(6, 1.0, closure="bogus")
    with pytest.raises(ValueError, match="closure"):
        dataset.draw_instances(5, 6, samples=2, closure="bogus")
    with pytest.raises(ValueError, match="closure"):
        dataset.create_dataset(str(tmp_path / "d"), 5, 6, samples=2, closure="bogus")
    with pytest.raises(ValueError, match="closure"):
        dataset.draw_instances(5, 6, samples=2, distances="random", closure=None)


def _bad_inputs():
    ok = np.ones((4, 4))
    nan, neg, inf = ok.copy(), ok.copy(), ok.copy()
    nan[1, 2], neg[3, 0], inf[0, 3] = np.nan, -1e-300, np.inf
    return {"n257": (np.ones((257, 257)), "n=257"), "nan": (nan, "finite"), "negative": (neg, "non-negative"),
            "inf": (inf, "finite"), "nonsquare": (np.ones((4, 5)), "square"), "empty": (np.ones((0, 0)), "n=0"),
            "vector": (np.ones(4), "square")}


@pytest.mark.parametrize("case", sorted(_bad_inputs()))
def test_metric_closure_refuses_before_any_launch(case, no_launch):
    bad, word = _bad_inputs()[case]
    with pytest.raises(ValueError, match="instance 2: .*" + word):
        dataset.metric_closure([np.ones((3, 3)), np.ones((5, 5)), bad])


def test_metric_closure_of_nothing_and_bad_chunk(no_launch):
    assert dataset.metric_closure([]) == []
    with pytest.raises(ValueError, match="chunk_bytes"):
        dataset.metric_closure([np.ones((3, 3))], chunk_bytes=0)


def test_c_entry_refuses_before_any_launch():
    fn = _lib.lib.tspgnn_metric_closure
    p = ctypes.c_void_p(16)
    assert fn(p, p, p, 1, 257, None) == -1           # TSPGNN_EINVAL
    assert b"n_max=257" in _lib.lib.tspgnn_last_error()
    assert fn(p, p, p, 1, 0, None) == -1
    assert b"n_max=0" in _lib.lib.tspgnn_last_error()
    assert fn(p, p, p, -1, 20, None) == -1
    assert b"count=-1" in _lib.lib.tspgnn_last_error()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert fn(*args, 1, 20, None) == -1
        assert b"null pointer" in _lib.lib.tspgnn_last_error()
    assert fn(None, None, None, 0, 20, None) == 0    # count == 0: a no-op
    assert fn(p, p, p, 0, 256, None) == 0
    with pytest.raises(_lib.TspgnnError) as e:
        _lib.call("tspgnn_metric_closure", 16, 16, 16, 1, 257, None)
    assert e.value.status == -1


def _same(a, b):
    assert len(a) == len(b)
    for (Ma, Mw, perm, nodes), (Mb, Wb, pb, nb) in zip(a, b):
        assert np.array_equal(Ma, Mb) and np.array_equal(Mw, Wb) and perm == pb
        assert (nodes is None and nb is None) or np.array_equal(nodes, nb)


@pytest.mark.parametrize("distances,metric", [("euc_2D", True), ("euc_2D", False), ("random", False)])
def test_closure_device_changes_nothing_where_nothing_is_closed(distances, metric, no_launch):
    """euc_2D, or metric=False: no closure is taken, so closure='device' is the default call and needs no GPU."""
    def draw(**kw):
        random.seed(3)
        np.random.seed(3)
        tm = {}
        g = dataset.draw_instances(5, 9, conn_min=0.4, conn_max=0.9, samples=6, distances=distances, metric=metric,
                                   timings=tm, **kw)
        assert "closure" not in tm
        return g, np.random.rand(3), random.random()
    g0, r0, p0 = draw()
    g1, r1, p1 = draw(closure="device")
    _same(g0, g1)
    assert np.array_equal(r0, r1) and p0 == p1


def test_host_closure_is_todays_draw_and_is_timed():
    """closure='host' (the default) is floyd_warshall inside the draw, as before; timings['closure'] counts it."""
    random.seed(4)
    np.random.seed(4)
    tm = {}
    g = dataset.draw_instances(6, 9, conn_min=0.3, conn_max=0.9, samples=4, distances="random", timings=tm)
    assert tm["closure"] > 0
    random.seed(4)
    np.random.seed(4)
    for Ma, Mw, perm, nodes in g:
        n = random.randint(6, 9)
        Mb, Wb, pb, _ = dataset._draw_graph(n, np.random.uniform(0.3, 0.9), distances="random", close=False)
        assert np.array_equal(Ma, Mb) and perm == pb and nodes is None       # the open draw: same stream
        assert np.array_equal(Mw, dataset.floyd_warshall(Wb)) and not np.array_equal(Mw, Wb)
