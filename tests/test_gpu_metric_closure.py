"""The metric closure on the GPU (tspgnn.metric_closure on csrc/tour_closure.hip; closure='device' in create_graph,
draw_instances and create_dataset) against its definition, dataset.floyd_warshall on the same input.  The definition is
exact -- fp64 sums rounded once, minima, k ascending -- so every comparison is np.array_equal: there is no tolerance."""
import os
import random

import numpy as np
import pytest
import torch

from tspgnn import _lib, dataset

pytestmark = pytest.mark.gpu

L = dataset.CLOSURE_LDS_MAX_N
SIZES = (1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 127, 128, 129, L - 1, L, L + 1, 200, 255, 256)
FAMILIES = ("symmetric", "asymmetric", "integer", "path")


def make(family, n, rng):
    """symmetric / asymmetric: U[0, 1) off the diagonal; integer: weights from {1, .., 4}, so sums tie; path: a random
    Hamiltonian path of U(0, 1) edges and 1000 + U(0, 1) for every other pair -- the shortest paths run along the path, and
    the order in which their edges are added (k ascending) decides the last bits."""
    if family == "asymmetric":
        M = rng.rand(n, n)
    elif family == "integer":
        M = np.triu(rng.randint(1, 5, size=(n, n)).astype(np.float64), 1)
        M = M + M.T
    else:
        M = np.triu(rng.rand(n, n), 1)
        if family == "path":
            M = np.triu(1000.0 + rng.rand(n, n), 1)
            p = rng.permutation(n)
            for a, b in zip(p[:-1], p[1:]):
                M[min(a, b), max(a, b)] = rng.rand()
        M = M + M.T
    np.fill_diagonal(M, 0.0)
    return M


@pytest.fixture(scope="module")
def batch():
    """The ragged batch, unsorted, every size once per family, with the host closures: computed once, never changed."""
    rng = np.random.RandomState(20)
    items = [(f, n, make(f, n, rng)) for f in FAMILIES for n in SIZES]
    items = [items[k] for k in rng.permutation(len(items))]
    mats = [m for _, _, m in items]
    want = [dataset.floyd_warshall(m) for m in mats]
    for m in mats + want:
        m.setflags(write=False)
    return items, mats, want


def test_ragged_mixed_batch_equals_the_host(batch, cuda_device):
    items, mats, want = batch
    got = dataset.metric_closure(mats, device=cuda_device)
    assert len(got) == len(want)
    for (family, n, m), g, w in zip(items, got, want):
        assert g.dtype == np.float64 and g.shape == (n, n), (family, n)
        assert np.array_equal(g, w), (family, n, int((g != w).sum()))
        if n >= 16:
            assert (w != m).mean() > 0.3, (family, n)        # the closure changes these: an identity kernel fails


def test_result_is_independent_of_batch_chunk_and_repeats(batch, cuda_device):
    items, mats, want = batch
    pick = [k for k, (f, n, _) in enumerate(items) if f in ("path", "asymmetric") and n in (5, 17, 65, L, L + 1, 200)]
    assert len(pick) == 12
    for k in pick:                                            # alone
        assert np.array_equal(dataset.metric_closure([mats[k]], device=cuda_device)[0], want[k]), items[k][:2]
    sub = [mats[k] for k in pick]
    one_each = dataset.metric_closure(sub, device=cuda_device, chunk_bytes=1)     # one instance per launch
    twice = dataset.metric_closure(sub + sub[::-1], device=cuda_device)          # listed twice
    for j, k in enumerate(pick):
        assert np.array_equal(one_each[j], want[k]), items[k][:2]
        assert np.array_equal(twice[j], want[k]) and np.array_equal(twice[-1 - j], want[k]), items[k][:2]


def _call(buf, off, ns, n_max, dev):
    d = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(np.asarray(off, dtype=np.int64)).to(dev)
    d_n = torch.from_numpy(np.asarray(ns, dtype=np.int32)).to(dev)
    with torch.cuda.device(dev):
        _lib.call("tspgnn_metric_closure", _lib.ptr(d), _lib.ptr(d_off), _lib.ptr(d_n), len(ns), int(n_max),
                  _lib.current_stream())
        return d.cpu().numpy()


@pytest.mark.parametrize("n", [5, 17, 64])
def test_both_tiers_on_small_n(n, cuda_device):
    """n_max = 256 sends a small instance through the global tier, n_max = n through LDS: both are the host's matrix."""
    rng = np.random.RandomState(21 + n)
    mats = [make(f, n, rng) for f in FAMILIES]
    want = np.concatenate([dataset.floyd_warshall(m).reshape(-1) for m in mats])
    flat = np.concatenate([m.reshape(-1) for m in mats])
    off = [k * n * n for k in range(len(mats))]
    for n_max in (256, n):
        got = _call(flat.copy(), off, [n] * len(mats), n_max, cuda_device)
        assert np.array_equal(got, want), (n, n_max, int((got != want).sum()))


@pytest.mark.parametrize("n_max", [L, 256])
def test_memory_outside_the_matrices_is_untouched(n_max, cuda_device):
    """Gaps between the instances and a tail, filled with a NaN bit pattern; offsets out of order."""
    rng = np.random.RandomState(22)
    ns = [17, 1, 64, 5, 33]
    mats = [make(FAMILIES[k % 4], n, rng) for k, n in enumerate(ns)]
    place = [3, 0, 4, 1, 2]                                   # instance b sits at slot place[b]
    sizes = [n * n for n in ns]
    off, at = [0] * len(ns), 7
    for slot in range(len(ns)):
        b = place.index(slot)
        off[b] = at
        at += sizes[b] + 5 + slot
    fill = np.uint64(0x7FF8DEADBEEF0123)
    bits = np.full(at + 11, fill, dtype=np.uint64)
    buf = bits.view(np.float64)
    inside = np.zeros(bits.size, dtype=bool)
    for m, o, s in zip(mats, off, sizes):
        buf[o:o + s] = m.reshape(-1)
        inside[o:o + s] = True
    assert 0 < (~inside).sum() and off != sorted(off)
    got = _call(buf.copy(), off, ns, n_max, cuda_device)
    assert np.array_equal(got.view(np.uint64)[~inside], bits[~inside])
    for m, o, s in zip(mats, off, sizes):
        assert np.array_equal(got[o:o + s].reshape(m.shape), dataset.floyd_warshall(m))


def _draw(closure, **kw):
    random.seed(5)
    np.random.seed(5)
    tm = {}
    g = dataset.draw_instances(8, 12, conn_min=0.3, conn_max=0.9, samples=12, distances="random", closure=closure,
                               timings=tm, **kw)
    return g, np.random.rand(4), random.random(), tm


def test_draw_instances_device_equals_host(cuda_device):
    gh, rh, ph, th = _draw("host")
    gd, rd, pd, td = _draw("device", device=cuda_device)
    assert len(gh) == len(gd) == 12
    for (Ma, Mw, perm, nodes), (Mb, Wb, pb, nb) in zip(gh, gd):
        assert np.array_equal(Ma, Mb) and np.array_equal(Mw, Wb) and perm == pb and nodes is None and nb is None
    assert np.array_equal(rh, rd) and ph == pd               # the global generators are left in the same state
    assert th["closure"] > 0 and td["closure"] > 0


def test_create_graph_device_equals_host(cuda_device):
    out = []
    for closure in ("host", "device"):
        random.seed(6)
        np.random.seed(6)
        out.append(dataset.create_graph(11, 0.6, distances="random", closure=closure, kicks=4, device=cuda_device))
    (Ma, Mw, route, nodes), (Mb, Wb, rb, nb) = out
    assert np.array_equal(Ma, Mb) and np.array_equal(Mw, Wb) and route == rb and nodes is None and nb is None


def test_create_dataset_writes_the_same_bytes(tmp_path, cuda_device):
    summ = {}
    for closure in ("host", "device"):
        random.seed(5)
        np.random.seed(5)
        summ[closure] = dataset.create_dataset(str(tmp_path / closure), 8, 12, conn_min=0.3, conn_max=0.9, samples=6,
                                               distances="random", closure=closure, kicks=8, lb_iters=50,
                                               device=cuda_device)
        assert summ[closure]["times"]["closure"] > 0
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted("%d.graph" % i for i in range(6)) == sorted(os.listdir(tmp_path / "device"))
    for name in names:
        assert (tmp_path / "host" / name).read_bytes() == (tmp_path / "device" / name).read_bytes(), name
    assert np.array_equal(summ["host"]["cost"], summ["device"]["cost"])
    # euc_2D closes nothing: no 'closure' time, whatever the argument
    random.seed(5)
    np.random.seed(5)
    s = dataset.create_dataset(str(tmp_path / "euc"), 8, 12, samples=3, closure="device", kicks=4, lb_iters=20,
                               device=cuda_device)
    assert "closure" not in s["times"]


def test_redraw_rounds_close_on_the_device_too(tmp_path, cuda_device):
    """require_certified redraws through the same closure setting: some of the 8 instances are redrawn, and
    the two settings still redraw the same ones and write the same files."""
    summ = {}
    for closure in ("host", "device"):
        random.seed(7)
        np.random.seed(7)
        summ[closure] = dataset.create_dataset(str(tmp_path / closure), 9, 12, conn_min=0.3, conn_max=0.9, samples=8,
                                               distances="random", closure=closure, require_certified=0.1,
                                               device=cuda_device)
    assert summ["host"]["redrawn"] == summ["device"]["redrawn"] > 0
    for i in range(8):
        name = "%d.graph" % i
        assert (tmp_path / "host" / name).read_bytes() == (tmp_path / "device" / name).read_bytes(), name
