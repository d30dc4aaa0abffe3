"""Host half of tspgnn.DeviceDataset (no GPU): the once-per-instance preprocessing reproduces what create_batch +
csr_by_vertex give for each instance alone, plan_batch gives create_batch's prefix sums, the epoch order mirrors
InstanceLoader's, and malformed input raises what create_batch raises."""
import numpy as np
import pytest

from conftest import load_pack
import tspgnn
from tspgnn import device_dataset as DD
from tspgnn.instance_loader import route_cost

PACKS = [(name, seed) for name in ("n5_B2", "ragged_B6", "sparse_B4") for seed in (0, 1, 2)]


@pytest.mark.parametrize("name,seed", PACKS)
def test_preprocessing_equals_create_batch_of_each_instance_alone(name, seed):
    inst = load_pack(name, seed)["instances"]
    host = DD.preprocess(inst)
    assert host["n"].dtype == host["m"].dtype == np.int64
    assert host["uv"].dtype == host["rowptr"].dtype == host["eid"].dtype == np.int32
    assert host["w"].dtype == np.float32 and host["cost"].dtype == np.float64
    e0, v0 = host["e0"], host["v0"]
    assert len(host["uv"]) == len(host["w"]) == e0[-1] and len(host["eid"]) == 2 * e0[-1]
    assert len(host["rowptr"]) == v0[-1] + len(inst)
    for i, one in enumerate(inst):
        EV, W, _, _, nv, ne = tspgnn.InstanceLoader.create_batch([one], dev=0.0)
        rowptr, eid = EV.csr_by_vertex()
        n, m = int(nv[0]), int(ne[0])
        assert (host["n"][i], host["m"][i]) == (n, m)
        assert np.array_equal(host["uv"][e0[i]:e0[i + 1]], EV.uv)
        assert np.array_equal(host["w"][e0[i]:e0[i + 1]], W.reshape(-1).astype(np.float32))
        assert np.array_equal(host["rowptr"][v0[i] + i:v0[i + 1] + i + 1], rowptr)
        assert np.array_equal(host["eid"][2 * e0[i]:2 * e0[i + 1]], eid)
        assert host["cost"][i] == route_cost(one[1], one[2])


def _single_vertex():
    return np.zeros((1, 1), dtype=int), np.zeros((1, 1)), [0]


def test_plan_batch_equals_the_prefix_sums_of_create_batch():
    inst = load_pack("ragged_B6", 0)["instances"] + [_single_vertex()]
    host = DD.preprocess(inst)
    n, m = host["n"], host["m"]
    assert (n[-1], m[-1]) == (1, 0)
    for idx in (list(range(6)), [3, 3, 0, 0, 5, 5], [5, 0, 5], [2, 6, 6, 1], [6], []):
        EV, _, _, r, nv, ne = tspgnn.InstanceLoader.create_batch([inst[i] for i in idx], dev=0.02)
        e_start, v_start, M, N, labels = DD.plan_batch(n, m, idx)
        assert e_start.dtype == v_start.dtype == np.int32
        assert np.array_equal(e_start, EV.blocks[0]) and np.array_equal(v_start, EV.blocks[1])
        assert (M, N) == EV.shape
        assert np.array_equal(labels, r) and labels.dtype == np.int64   # (create_batch's is int64 unless the list is empty)
        assert np.array_equal(n[idx], nv) and np.array_equal(m[idx], ne)


def test_epoch_order_mirrors_the_instance_loader():
    a = DD.epoch_indices(10, 3, shuffle=True, rng=np.random.RandomState(5))
    b = DD.epoch_indices(10, 3, shuffle=True, rng=np.random.RandomState(5))
    assert len(a) == 10 // 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    for idx in a:
        assert idx.shape == (6,) and np.array_equal(idx[0::2], idx[1::2])       # each id twice in a row
    assert len(set(np.concatenate(a)[0::2].tolist())) == 9                      # ... and no id in two batches
    c = DD.epoch_indices(10, 3, shuffle=True, rng=np.random.RandomState(6))
    assert any(not np.array_equal(x, y) for x, y in zip(a, c))
    rng = np.random.RandomState(5)                                              # the order is drawn per call
    first, second = DD.epoch_indices(10, 3, rng=rng), DD.epoch_indices(10, 3, rng=rng)
    assert all(np.array_equal(x, y) for x, y in zip(a, first))
    assert any(not np.array_equal(x, y) for x, y in zip(first, second))
    plain = DD.epoch_indices(10, 3, shuffle=False)
    assert np.array_equal(np.concatenate(plain), np.repeat(np.arange(9), 2))


def test_every_index_of_an_epoch_appears_exactly_twice():
    batches = DD.epoch_indices(12, 4, shuffle=True, rng=np.random.RandomState(1))
    assert len(batches) == 3
    assert np.array_equal(np.bincount(np.concatenate(batches), minlength=12), np.full(12, 2))


def test_a_cpu_dataset_is_plumbing_only():
    inst = load_pack("n5_B2", 0)["instances"]
    ds = tspgnn.DeviceDataset(inst, device="cpu")
    assert len(ds) == 2 and ds.n.dtype == ds.m.dtype == np.int64
    with pytest.raises(RuntimeError):
        ds.batch([0, 1])
    with pytest.raises(IndexError):
        ds.batch([0, 2])


def test_errors():
    inst = load_pack("ragged_B6", 0)["instances"]
    host = DD.preprocess(inst)
    for bad in ([6], [-1], [0, 1, 99]):
        with pytest.raises(IndexError):
            DD.plan_batch(host["n"], host["m"], bad)
    Ma, Mw, route = inst[0]
    with pytest.raises(ValueError):
        DD.preprocess([inst[1], (Ma[:, :-1], Mw, route)])            # non-square adjacency
    with pytest.raises(ValueError):
        DD.preprocess([(Ma, Mw[:-1, :-1], route)])                   # weight matrix of another shape
    with pytest.raises(IndexError):
        DD.preprocess([inst[1], (Ma, Mw, [0, 1, len(Ma)])])          # a route that leaves its graph
    # the same three through create_batch: the dataset raises what the loader raises
    with pytest.raises(ValueError):
        tspgnn.InstanceLoader.create_batch([(Ma[:, :-1], Mw, route)])
    with pytest.raises(ValueError):
        tspgnn.InstanceLoader.create_batch([(Ma, Mw[:-1, :-1], route)])
    with pytest.raises(IndexError):
        tspgnn.InstanceLoader.create_batch([(Ma, Mw, [0, 1, len(Ma)])])
    # int32 limit: 2 * sum(m) < 2^31, through the size function
    DD.check_size(2 ** 30 - 1)
    with pytest.raises(ValueError, match="2\\^31"):
        DD.check_size(2 ** 30)


def test_from_directory_reads_the_graph_files_in_sorted_order(tmp_path):
    rng = np.random.RandomState(2)
    inst = [tspgnn.random_instance(n, rng) for n in (6, 4, 5)]
    for name, (Ma, Mw, route) in zip(("b", "a", "c"), inst):
        tspgnn.write_graph(Ma, Mw, str(tmp_path / (name + ".graph")), route=route)
    ds = tspgnn.DeviceDataset.from_directory(str(tmp_path), device="cpu")
    assert np.array_equal(ds.n, [4, 6, 5])
    assert np.array_equal(ds.m, [np.count_nonzero(inst[k][0]) for k in (1, 0, 2)])
