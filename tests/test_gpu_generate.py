"""DeviceDataset.generate on the GPU (tspgnn/device_dataset.py; csrc/dataset_build.hip): the dataset it makes from the
random streams equals, byte for byte, the one the host route makes from the same seeds -- draw_instances (closure
included), label_tours(init_tours=planted cycles, index=arange), DeviceDataset([(np.triu(Ma), Mw, tour)]) -- in all six
device arrays, n, m, the summary's cost / lb / target / feasible, the tours and the state the global generators are left
in.  The search runs restarts=2, kicks=4, lb_iters=20: its quality is not under test, only that both routes feed it the
same bits."""
import random

import numpy as np
import pytest
import torch

from tspgnn import dataset
from tspgnn.device_dataset import DeviceDataset

pytestmark = pytest.mark.gpu

KW = dict(restarts=2, kicks=4, lb_iters=20)
ARRAYS = ("_inst", "_uv", "_w", "_rowptr", "_eid", "_cost")

# name: (samples, nmin, nmax, (conn_min, conn_max), distances, metric)
CASES = {
    "sparse_ragged": (24, 4, 12, (0.3, 0.9), "euc_2D", True),
    "n63": (3, 63, 63, (1, 1), "euc_2D", True),
    "n64": (3, 64, 64, (1, 1), "euc_2D", True),
    "n65": (3, 65, 65, (1, 1), "euc_2D", True),
    "n128": (3, 128, 128, (1, 1), "euc_2D", True),
    "tri_n129": (2, 129, 129, (1, 1), "euc_2D", True),
    "tri_n140": (2, 140, 140, (0.5, 0.9), "euc_2D", True),
    "both_classes": (6, 126, 131, (1, 1), "euc_2D", True),
    "random_closed_lds": (16, 5, 20, (0.4, 1.0), "random", True),
    "random_closed_global": (2, 144, 144, (1, 1), "random", True),
    "random_open": (8, 5, 20, (0.4, 1.0), "random", False),
}


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _state():
    return random.getstate(), np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def host_route(case, rng_seed, exact=False, **kw):
    """-> (instances [(np.triu(Ma), Mw, tour)], results, stats, DeviceDataset, generator state afterwards)."""
    samples, nmin, nmax, conn, distances, metric = case
    _seed(rng_seed)
    graphs = dataset.draw_instances(nmin, nmax, conn[0], conn[1], samples, distances, metric, closure="device")
    state = _state()
    stats = {}
    res = dataset.label_tours([(g[0], g[1]) for g in graphs], init_tours=[g[2] for g in graphs],
                              index=np.arange(samples), exact=exact, stats=stats, **kw)
    inst = [(np.triu(g[0]), g[1], r.tour) for g, r in zip(graphs, res)]
    return inst, res, stats, DeviceDataset(inst), state


def generated(case, rng_seed, **kw):
    samples, nmin, nmax, conn, distances, metric = case
    _seed(rng_seed)
    ds = DeviceDataset.generate(samples, nmin, nmax, conn[0], conn[1], distances=distances, metric=metric, **kw)
    return ds, _state()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_same_dataset(a, b):
    assert np.array_equal(a.n, b.n) and np.array_equal(a.m, b.m) and a.n.dtype == b.n.dtype and a.m.dtype == b.m.dtype
    for name in ARRAYS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, name
        assert bits(x.cpu().numpy()) == bits(y.cpu().numpy()), name


def assert_same_labels(ds, res):
    s = ds.summary
    assert s["samples"] == len(res) and np.array_equal(s["n"], ds.n)
    assert bits(s["cost"]) == bits(np.array([r.cost for r in res]))
    assert bits(s["lb"]) == bits(np.array([r.lb for r in res]))
    assert bits(s["target"]) == bits(np.array([r.target for r in res]))
    assert s["feasible"].dtype == bool and np.array_equal(s["feasible"], [r.feasible for r in res])
    cost, lb = s["cost"], s["lb"]
    assert bits(s["gap"]) == bits((cost - lb) / np.where(cost > 0, cost, 1.0))
    assert s["certified_fraction"] == dataset.certify(res, 0.02)["fraction"]
    tours, off = ds.tours
    assert tours.dtype == np.int32 and np.array_equal(off, np.concatenate([[0], np.cumsum(ds.n)]))
    assert np.array_equal(tours, np.concatenate([r.tour for r in res]))
    assert {"draw", "build", "search", "pack"} <= set(s["times"]) and all(v >= 0 for v in s["times"].values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_generate_equals_the_host_route(name):
    case = CASES[name]
    inst, res, _, host, host_state = host_route(case, 3, **KW)
    ds, state = generated(case, 3, **KW)
    assert _same_state(state, host_state)
    assert_same_dataset(ds, host)
    assert_same_labels(ds, res)
    assert ("closure" in ds.summary["times"]) == (case[4] == "random" and case[5])
    assert "bound" in ds.summary["times"] and "exact" not in ds.summary["times"]
    if name == "sparse_ragged":   # where a prefix sum or the CSR order would go wrong
        full = ds.n * (ds.n - 1) // 2
        assert (ds.m < full).any() and len(set(ds.m.tolist())) > 4
        degrees = np.concatenate([np.diff(p) for p in np.split(host._rowptr.cpu().numpy(), np.cumsum(ds.n + 1)[:-1])])
        assert degrees.min() == 2 and degrees.sum() == 2 * ds.m.sum()
    if name == "both_classes":
        assert ds.n.min() <= 128 < ds.n.max()
    got = ds.to_instances()
    assert len(got) == len(inst)
    for (Ma, Mw, tour), (Ha, Hw, htour) in zip(got, inst):
        assert np.array_equal(Ma, Ha) and bits(Mw) == bits(Hw) and tour == htour


def test_result_does_not_depend_on_chunk_bytes():
    case = CASES["sparse_ragged"]
    whole, state = generated(case, 7, **KW)
    chunk_bytes = 2000
    assert 8 * int((whole.n ** 2).sum()) > 2 * chunk_bytes   # so at least three chunks, each at most chunk_bytes
    parts, state2 = generated(case, 7, chunk_bytes=chunk_bytes, **KW)
    assert _same_state(state, state2)
    assert_same_dataset(parts, whole)
    for key in ("cost", "lb", "target", "feasible"):
        assert bits(parts.summary[key]) == bits(whole.summary[key]), key
    assert np.array_equal(parts.tours[0], whole.tours[0])
    one_each, _ = generated(CASES["both_classes"], 7, chunk_bytes=1, **KW)   # every instance its own chunk
    assert_same_dataset(one_each, generated(CASES["both_classes"], 7, **KW)[0])


def test_exact_labels_equal_label_tours_exact():
    case = (8, 8, 12, (0.5, 1.0), "euc_2D", True)
    _, res, stats, host, host_state = host_route(case, 9, exact=True, **KW)
    ds, state = generated(case, 9, exact=True, **KW)
    assert _same_state(state, host_state)
    assert_same_dataset(ds, host)
    assert_same_labels(ds, res)
    assert np.array_equal(ds.summary["proved"], stats["status"] == "proved") and ds.summary["proved"].any()
    assert np.array_equal(ds.summary["nodes"], stats["nodes"])
    assert "exact" in ds.summary["times"] and "bound" not in ds.summary["times"]


def test_batches_of_a_generated_dataset_equal_the_host_built_ones():
    case = CASES["sparse_ragged"]
    _, _, _, host, _ = host_route(case, 5, **KW)
    ds, _ = generated(case, 5, **KW)
    ids = [3, 3, 0, 23, 7, 7, 7, 11]
    a, b = ds.batch(ids, dev=0.02), host.batch(ids, dev=0.02)
    torch.cuda.synchronize()
    from tspgnn.parallel import stage_layout
    assert list(a._offsets) == list(b._offsets) and a._buf.numel() == b._buf.numel()
    sizes = stage_layout(a.M, a.N, a.B, 0)[1]
    for k in range(7):   # the seven arrays of the staged batch (between them the buffer holds padding nobody writes)
        o = a._offsets[k]
        assert torch.equal(a._buf[o:o + sizes[k]], b._buf[o:o + sizes[k]]), k
    assert np.array_equal(a.n_edges, b.n_edges) and np.array_equal(a.n_vertices, b.n_vertices)


def test_seed_and_neighbors_reach_the_search():
    case = CASES["n65"]
    _, res, _, host, _ = host_route(case, 2, seed=5, neighbors=6, **KW)
    ds, _ = generated(case, 2, seed=5, neighbors=6, **KW)
    assert_same_dataset(ds, host)
    assert_same_labels(ds, res)
