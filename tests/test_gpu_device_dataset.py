"""tspgnn.DeviceDataset on the GPU: tspgnn_gather_batch writes, byte for byte, what tspgnn_host_stage_batch writes for the
same instance list (which tests/test_packer.py pins to the reference-generated fixtures) and nothing else; batches made of
it feed the forward pass, run_batch, the training step and a captured forward exactly as create_batch's do."""
import numpy as np
import pytest
import torch

import tspgnn
from conftest import load_pack
from oracle import params as P
from tspgnn import device_dataset as DD
from tspgnn import parallel as PL

pytestmark = pytest.mark.gpu

PLAN_INTS = 11   # a plan slot behind the seven arrays that the kernel must leave alone


def single_vertex():
    return np.zeros((1, 1), dtype=int), np.zeros((1, 1)), [0]


def assert_gather_equals_host_stage(ds, inst, idx, dev, target):
    """The bar: every byte of the buffer -- the seven arrays, the alignment padding between them and the plan's slot, all
    0xAB beforehand -- equals the host stager's over the same instance list."""
    e_start, v_start, M, N, _ = DD.plan_batch(ds.n, ds.m, idx)
    B = len(idx)
    off, sizes, total = PL.stage_layout(M, N, B, PLAN_INTS)
    want = np.full(total, 0xAB, dtype=np.uint8)
    PL.stage_instances([inst[i] for i in idx], dev, target, M, N, want.ctypes.data, off)
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device=ds.device)
    ds.gather(idx, dev, target, buf, off)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    names = ("uv", "eid", "rowptr", "wc", "labels", "seg", "n_edges")
    for k, name in enumerate(names):
        assert np.array_equal(got[off[k]:off[k] + sizes[k]], want[off[k]:off[k] + sizes[k]]), (name, idx)
    covered = np.zeros(total, dtype=bool)
    for k in range(7):
        covered[off[k]:off[k] + sizes[k]] = True
    assert np.all(got[~covered] == 0xAB), ("padding / plan slot written", idx)
    assert np.all(got[off[7]:off[7] + 4 * PLAN_INTS] == 0xAB)
    return got, off, sizes


@pytest.fixture(scope="module")
def ragged(cuda_device):
    rng = np.random.RandomState(3)
    inst = [tspgnn.random_instance(n, rng) for n in (5, 9, 3, 12, 12, 7)]
    return inst, tspgnn.DeviceDataset(inst, device=cuda_device)


@pytest.mark.parametrize("target", [None, 0.4321])
def test_ragged_list(ragged, target):
    inst, ds = ragged
    assert_gather_equals_host_stage(ds, inst, list(range(6)), 0.03, target)


@pytest.mark.parametrize("idx", [[3, 3, 0, 0, 5, 5], [5, 0, 5], [2]])
def test_out_of_order_repeats_and_a_single_instance(ragged, idx):
    inst, ds = ragged
    assert_gather_equals_host_stage(ds, inst, idx, 0.03, None)


def test_single_vertex_instances(cuda_device):
    rng = np.random.RandomState(4)
    inst = [tspgnn.random_instance(6, rng), single_vertex(), single_vertex(), tspgnn.random_instance(4, rng)]
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    assert_gather_equals_host_stage(ds, inst, [0, 1, 2, 3], 0.02, None)
    assert_gather_equals_host_stage(ds, inst, [1, 0, 3, 2], 0.02, None)        # ... first and last in the batch
    got, off, sizes = assert_gather_equals_host_stage(ds, inst, [1, 2, 1], 0.02, None)   # M = 0: nothing launched
    assert not got[off[2]:off[2] + sizes[2]].any() and not got[off[5]:off[5] + sizes[5]].any()
    assert sizes[2] == 4 * 4 and sizes[5] == 4 * 4


def test_sparse_instances(cuda_device):
    inst = load_pack("sparse_B4", 0)["instances"]
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    assert_gather_equals_host_stage(ds, inst, [0, 1, 2, 3], 0.02, None)
    assert_gather_equals_host_stage(ds, inst, [2, 0, 3, 3, 1], 0.02, 1.5)


def test_an_instance_over_several_workgroups(cuda_device):
    rng = np.random.RandomState(5)
    inst = [tspgnn.random_instance(64, rng), tspgnn.random_instance(3, rng)]
    assert int(np.count_nonzero(inst[0][0])) == 2016
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    assert_gather_equals_host_stage(ds, inst, [0, 1], 0.02, None)
    assert_gather_equals_host_stage(ds, inst, [1, 0, 1, 0], 0.02, None)


def test_the_largest_instance_alone(cuda_device):
    inst = [tspgnn.random_instance(256, np.random.RandomState(6))]
    assert int(np.count_nonzero(inst[0][0])) == 32640
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    assert_gather_equals_host_stage(ds, inst, [0], 0.02, None)


def test_more_slots_than_the_lds_search_table_holds(cuda_device):
    """Above 8191 slots the kernel searches e_start / v_start in global memory: both sides of that threshold."""
    rng = np.random.RandomState(7)
    inst = [tspgnn.random_instance(3, rng), single_vertex(), tspgnn.random_instance(4, rng)]
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    for B in (8191, 8192):
        assert_gather_equals_host_stage(ds, inst, list(np.arange(B) % 3), 0.02, None)


def test_argument_checks(ragged):
    from tspgnn import _lib
    import ctypes
    inst, ds = ragged
    buf = torch.zeros(4096, dtype=torch.uint8, device=ds.device)
    off = (ctypes.c_longlong * 7)(*range(0, 7 * 256, 256))
    p = buf.data_ptr()
    args = lambda B, dst, o: (p, p, p, p, p, p, p, p, p, B, 4, 4, 0.02, 0, 0.0, dst, o, None)
    assert _lib.lib.tspgnn_gather_batch(*args(-1, p, off)) == -1
    assert _lib.lib.tspgnn_gather_batch(*args(2, None, off)) == -1 and b"null" in _lib.lib.tspgnn_last_error()
    odd = (ctypes.c_longlong * 7)(0, 256, 516, 768, 1024, 1280, 1536)
    assert _lib.lib.tspgnn_gather_batch(*args(2, p, odd)) == -1 and b"multiple of 8" in _lib.lib.tspgnn_last_error()
    assert _lib.lib.tspgnn_gather_batch(*args(0, None, None)) == 0
    with pytest.raises(IndexError):
        ds.batch([0, 6])


def test_batch_into_an_earlier_batch(ragged):
    inst, ds = ragged
    first = ds.batch([3, 0, 5], dev=0.03, time_steps=3)
    ptrs = [t.data_ptr() for t in first.tensors()]
    again = ds.batch([4, 0, 5], dev=0.03, time_steps=3, out=first)     # instances 3 and 4 are both n = 12
    assert again is first and [t.data_ptr() for t in first.tensors()] == ptrs
    fresh = ds.batch([4, 0, 5], dev=0.03, time_steps=3)
    torch.cuda.synchronize()
    for a, b in zip(first.tensors(), fresh.tensors()):
        assert torch.equal(a, b)
    assert not torch.equal(first.WC, ds.batch([3, 0, 5], dev=0.03).WC)
    with pytest.raises(ValueError):
        ds.batch([0, 4, 5], out=first)
    with pytest.raises(ValueError):
        ds.batch([4, 0], out=first)


def _session(d, params):
    model = tspgnn.build_network(d)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(params)
    return model, sess


def _feed(model, t, T):
    EV, W, C, route_exists, n_vertices, n_edges = t
    return {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}


def test_end_to_end_equals_the_create_batch_path(cuda_device):
    d, T = 32, 3
    rng = np.random.RandomState(8)
    inst = [tspgnn.random_instance(n, rng) for n in (5, 9, 12, 7)]
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    t = tspgnn.InstanceLoader.create_batch(inst, dev=0.02)
    params = P.init_params(d, seed=5, perturb=True)
    model, sess = _session(d, params)
    host = sess.prepare(_feed(model, t, T))
    devb = ds.batch([0, 1, 2, 3], dev=0.02, time_steps=T)
    assert (devb.M, devb.N, devb.B, devb.T) == (host.M, host.N, host.B, host.T)
    for a, b in ((devb.adj.uv, host.adj.uv), (devb.adj.csr_t[0], host.adj.csr_t[0]), (devb.adj.csr_t[1], host.adj.csr_t[1]),
                 (devb.WC, host.WC), (devb.labels, host.labels), (devb.seg, host.seg)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert (devb.adj.loop_plan is None) == (host.adj.loop_plan is None)
    for k, want in ((devb.route_exists, t[3]), (devb.n_vertices, t[4]), (devb.n_edges, t[5])):
        assert k.dtype == np.int64 and np.array_equal(k, want)
    oh, od = sess.forward(host), sess.forward(devb)
    for key in ("predictions", "E_vote"):
        assert np.array_equal(oh[key].cpu().numpy(), od[key].cpu().numpy()), key
    rh = tspgnn.run_batch(sess, model, t, 0, 0, T, train=False, verbose=False)
    rd = tspgnn.run_batch(sess, model, devb, 0, 0, T, train=False, verbose=False)
    assert len(rd) == 8 and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(rh, rd))
    finals = []
    for use_device in (False, True):
        model, sess = _session(d, params)
        sess.train_step(ds.batch([0, 1, 2, 3], dev=0.02, time_steps=T) if use_device else _feed(model, t, T))
        torch.cuda.synchronize()
        finals.append(model.store.theta.cpu().numpy().copy())
    assert np.array_equal(finals[0], finals[1])
    assert not np.array_equal(finals[0], np.zeros_like(finals[0]))


def test_a_captured_forward_serves_batches_written_into_its_buffer(cuda_device):
    d, T = 32, 3
    rng = np.random.RandomState(9)
    inst = [tspgnn.random_instance(n, rng) for n in (5, 5, 9, 9, 7, 7)]
    ds = tspgnn.DeviceDataset(inst, device=cuda_device)
    model, sess = _session(d, P.init_params(d, seed=6, perturb=True))
    lists = ([0, 2, 4, 4], [1, 3, 5, 4], [1, 2, 5, 5])
    want = [sess.forward(ds.batch(idx, dev=0.02, time_steps=T))["predictions"].clone() for idx in lists]
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    bound = ds.batch(lists[2], dev=0.02, time_steps=T)
    replay = sess.capture_forward(bound)
    for idx, w in zip(lists, want):
        assert ds.batch(idx, dev=0.02, time_steps=T, out=bound) is bound
        assert torch.equal(replay()["predictions"], w), idx
    assert not sess.range_exceeded()
