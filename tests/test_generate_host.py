"""Host side of DeviceDataset.generate (tspgnn/device_dataset.py; csrc/dataset_build.hip): dataset.draw_streams makes
draw_instances' draws and leaves the global generators where draw_instances leaves them; a NumPy restatement of
tspgnn_build_instances rebuilds draw_instances' matrices and planted cycles from the streams bit for bit; the three entry
points and generate refuse bad arguments before any launch.  No GPU."""
import ctypes
import random

import numpy as np
import pytest

import tspgnn
from tspgnn import _lib, dataset
from tspgnn.device_dataset import DeviceDataset

from generate_reference import build_instance

CASES = [(d, c) for d in ("euc_2D", "random") for c in ((1, 1), (0.3, 0.9))]
P = 64   # a non-null, 8-byte aligned stand-in for a device pointer: every call below is refused before it is used


@pytest.fixture
def no_launch(monkeypatch):
    """Any call into the library's launch path, or any look at the device, fails the test."""
    def boom(*a, **k):
        raise AssertionError("reached the launch path")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "current_stream", boom)


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _same_state(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


@pytest.mark.parametrize("distances,conn", CASES)
def test_draw_streams_consumes_the_generators_like_draw_instances(distances, conn):
    _seed(11)
    graphs = dataset.draw_instances(4, 30, conn[0], conn[1], samples=50, distances=distances, metric=False)
    after_instances = (random.getstate(), np.random.get_state())
    _seed(11)
    S = dataset.draw_streams(4, 30, conn[0], conn[1], samples=50, distances=distances)
    assert _same_state((random.getstate(), np.random.get_state()), after_instances)
    n = np.array([g[0].shape[0] for g in graphs])
    assert S["n"].dtype == np.int32 and np.array_equal(S["n"], n) and n.min() >= 4 and n.max() <= 30
    assert S["conn"].dtype == np.float64 and S["conn"].shape == (50,)
    pairs = n * (n - 1) // 2
    assert np.array_equal(S["pair_off"], np.concatenate([[0], np.cumsum(pairs)]))
    assert np.array_equal(S["vert_off"], np.concatenate([[0], np.cumsum(n)]))
    assert S["adj_u"].shape == (pairs.sum(),) and S["perm"].dtype == np.int32 and S["perm"].shape == (n.sum(),)
    second = S["pts"] if distances == "euc_2D" else S["wts"]
    assert second.dtype == np.float64 and second.shape == ((2 * n.sum(),) if distances == "euc_2D" else (pairs.sum(),))
    assert ("wts" in S) != ("pts" in S)
    assert all(np.ndim(v) <= 1 for v in S.values())   # no n x n array anywhere


@pytest.mark.parametrize("distances,conn", CASES)
def test_restated_build_kernel_rebuilds_the_matrices_bit_for_bit(distances, conn):
    _seed(5)
    graphs = dataset.draw_instances(4, 30, conn[0], conn[1], samples=50, distances=distances, metric=False)
    _seed(5)
    S = dataset.draw_streams(4, 30, conn[0], conn[1], samples=50, distances=distances)
    sparse = 0
    for i, (Ma, Mw, perm, _) in enumerate(graphs):
        A, W, p = build_instance(S, i)
        assert np.array_equal(A, Ma) and p == perm, i
        assert W.tobytes() == np.ascontiguousarray(Mw).tobytes(), i
        sparse += int(np.count_nonzero(np.triu(A, 1)) < len(p) * (len(p) - 1) // 2)
    assert (sparse > 0) == (conn != (1, 1))


def test_draw_streams_arguments_and_export():
    assert tspgnn.draw_streams is dataset.draw_streams and "draw_streams" in tspgnn.__all__
    with pytest.raises(ValueError, match="distances"):
        dataset.draw_streams(4, 5, samples=1, distances="manhattan")
    _seed(0)
    S = dataset.draw_streams(4, 5, samples=0)
    assert S["n"].shape == (0,) and S["adj_u"].shape == (0,) and np.array_equal(S["pair_off"], [0])


# ------------------------------------------------------------------------------------------------- the entry points
def _build_args(**kw):
    a = dict(tab=P, d_tab=P, conn=P, adj_u=P, coord=P, perm=P, random_weights=0, count=1, n_max=8, n_pairs=28, n_verts=8,
             n_cells=64, Mw=P, A=P, m=P, stream=None)
    a.update(kw)
    return list(a.values())


def _pen_args(**kw):
    a = dict(tab=P, d_tab=P, A=P, Mw=P, count=1, n_max=8, triangle=0, n_cells=64, n_floats=64, W=P, stream=None)
    a.update(kw)
    return list(a.values())


def _pack_args(**kw):
    a = dict(tab=P, d_tab=P, A=P, Mw=P, tours=P, count=1, n_max=8, n_cells=64, n_tour=8, n_edges=28, n_rowptr=9, n_inst=1,
             uv=P, w=P, rowptr=P, eid=P, cost=P, file_cost=P, cycle_cost=P, feasible=P, stream=None)
    a.update(kw)
    return list(a.values())


ENTRY = {"tspgnn_build_instances": (_build_args, ["tab", "d_tab", "conn", "adj_u", "coord", "perm", "Mw", "A", "m"]),
         "tspgnn_penalise_instances": (_pen_args, ["tab", "d_tab", "A", "Mw", "W"]),
         "tspgnn_pack_dataset": (_pack_args, ["tab", "d_tab", "A", "Mw", "tours", "uv", "w", "rowptr", "eid", "cost",
                                              "file_cost", "cycle_cost", "feasible"])}


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_entry_points_refuse_before_any_launch(name):
    fn, (args, pointers) = getattr(_lib.lib, name), ENTRY[name]
    err = _lib.lib.tspgnn_last_error
    for p in pointers:
        assert fn(*args(**{p: None})) == -1 and b"null" in err(), p
    for n_max in (3, 257):
        assert fn(*args(n_max=n_max)) == -1 and b"n_max" in err()
    assert fn(*args(count=-1)) == -1 and b"count" in err()
    # an empty count is a no-op that looks at nothing else
    assert fn(*args(count=0, **{p: None for p in pointers})) == 0
    with pytest.raises(_lib.TspgnnError, match="n_max=257"):
        _lib.call(name, *args(n_max=257))


def test_entry_points_check_every_table_row_on_the_host():
    """n outside [4, n_max], an offset that leaves its array, a misaligned array: refused from the host table alone (the
    device pointers are stand-ins that a launch would fault on)."""
    err = _lib.lib.tspgnn_last_error
    row = lambda *v: np.array([v], dtype=np.int64)
    L = _lib.lib
    good = row(8, 0, 0, 0)
    for tab, word in ((row(3, 0, 0, 0), b"n=3"), (row(9, 0, 0, 0), b"n=9"), (row(8, 1, 0, 0), b"leave"),
                      (row(8, 0, 1, 0), b"leave"), (row(8, 0, 0, 1), b"leave"), (row(8, -1, 0, 0), b"leave")):
        assert L.tspgnn_build_instances(*_build_args(tab=tab.ctypes.data)) == -1 and word in err(), tab
    assert L.tspgnn_build_instances(*_build_args(tab=good.ctypes.data, Mw=P + 4)) == -1 and b"misaligned" in err()
    for tab, word in ((row(2, 0, 0), b"n=2"), (row(8, 1, 0), b"leave"), (row(8, 0, 1), b"leave")):
        assert L.tspgnn_penalise_instances(*_pen_args(tab=tab.ctypes.data)) == -1 and word in err(), tab
    assert L.tspgnn_penalise_instances(*_pen_args(tab=row(8, 0, 0).ctypes.data, triangle=1, n_floats=27)) == -1
    assert L.tspgnn_penalise_instances(*_pen_args(n_max=129)) == -1 and b"square" in err()
    for tab, word in ((row(300, 0, 0, 28, 0, 0, 0), b"n=300"), (row(8, 1, 0, 28, 0, 0, 0), b"leave"),
                      (row(8, 0, 1, 28, 0, 0, 0), b"leave"), (row(8, 0, 0, 29, 0, 0, 0), b"leave"),
                      (row(8, 0, 0, 28, 1, 0, 0), b"leave"), (row(8, 0, 0, 28, 0, 1, 0), b"leave"),
                      (row(8, 0, 0, 28, 0, 0, 1), b"leave")):
        assert L.tspgnn_pack_dataset(*_pack_args(tab=tab.ctypes.data)) == -1 and word in err(), tab
    assert L.tspgnn_pack_dataset(*_pack_args(tab=row(8, 0, 0, 28, 0, 0, 0).ctypes.data, uv=P + 4)) == -1
    assert b"misaligned" in err()
    assert L.tspgnn_pack_dataset(*_pack_args(n_edges=2 ** 30)) == -1 and b"2^31" in err()


@pytest.mark.parametrize("kw,word", [(dict(nmin=3), "nmin"), (dict(nmax=257), "nmax"), (dict(nmin=9, nmax=8), "nmin"),
                                     (dict(restarts=17), "restarts"), (dict(restarts=0), "restarts"),
                                     (dict(kicks=-1), "kicks"), (dict(lb_iters=0), "lb_iters"),
                                     (dict(neighbors=33), "neighbors"), (dict(exact=True, max_nodes=0), "max_nodes"),
                                     (dict(distances="manhattan"), "distances"), (dict(chunk_bytes=0), "chunk_bytes"),
                                     (dict(samples=-1), "samples"), (dict(device="cpu"), "device")])
def test_generate_refuses_before_any_launch(kw, word, no_launch):
    args = dict(samples=2, nmin=5, nmax=8, device="cuda:0")
    args.update(kw)
    state = (random.getstate(), np.random.get_state())
    with pytest.raises(ValueError, match=word):
        DeviceDataset.generate(**args)
    assert _same_state((random.getstate(), np.random.get_state()), state)   # and before any draw


def test_generate_takes_label_tours_keywords_only(no_launch):
    with pytest.raises(TypeError, match="chunk"):
        DeviceDataset.generate(2, 5, 8, device="cuda:0", chunk=4)


def test_generate_checks_the_chains_that_fit_at_the_largest_n_drawn(no_launch):
    _seed(1)
    with pytest.raises(ValueError, match="chains fit"):
        DeviceDataset.generate(1, 256, 256, device="cuda:0", restarts=11)


def test_to_instances_needs_a_generated_dataset():
    ds = DeviceDataset([(np.triu(np.ones((4, 4)), 1), np.ones((4, 4)), [0, 1, 2, 3])], device="cpu")
    assert ds.summary is None and ds.tours is None
    with pytest.raises(RuntimeError, match="generate"):
        ds.to_instances()
