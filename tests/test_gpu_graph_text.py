"""The device writer of .graph files (csrc/graph_text.hip, tspgnn/graph_text.py) against instance_loader.write_graph:
the formatter against the host build of the same routine, the two file kernels on a hand-made instance, whole generated
datasets file by file, the chunking, create_dataset's two writers, and the kernels' guards.  Every comparison is exact."""
import os
import random

import numpy as np
import pytest
import torch

import graph_text_cases as cases
from tspgnn import _lib, dataset
from tspgnn.device_dataset import DeviceDataset
from tspgnn.graph_text import REPR_BYTES, host_f64_repr
from tspgnn.instance_loader import read_graph, write_graph

pytestmark = pytest.mark.gpu

KW = dict(restarts=2, kicks=4, lb_iters=20)   # the labels' quality is not under test


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def host_bytes(tmp_path, inst, name="host.graph"):
    Ma, Mw, tour = inst
    p = str(tmp_path / name)
    write_graph(np.triu(Ma), Mw, p, route=tour)
    with open(p, "rb") as f:
        return f.read()


def directory(path):
    out = {}
    for name in os.listdir(path):
        with open(os.path.join(path, name), "rb") as f:
            out[name] = f.read()
    return out


class Launch(object):
    """The two kernels over a list of (Ma, Mw, tour), called directly: ``sizes`` after size(), ``text`` / ``status`` after
    write(); the text buffer is pre-filled with '#' and ``slack`` bytes longer than the files."""

    def __init__(self, insts, dev, slack=16):
        self.dev = dev
        self.n = np.array([len(t) for _, _, t in insts], dtype=np.int64)
        self.c_off = np.cumsum(self.n ** 2) - self.n ** 2
        self.t_off = np.cumsum(self.n) - self.n
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.A = up(np.concatenate([(np.triu(Ma) != 0).astype(np.uint8).reshape(-1) for Ma, _, _ in insts]))
        self.Mw = up(np.concatenate([np.asarray(Mw, dtype=np.float64).reshape(-1) for _, Mw, _ in insts]))
        self.tours = up(np.concatenate([np.asarray(t, dtype=np.int32) for _, _, t in insts]))
        self.up, self.slack = up, slack

    def size(self):
        tab = np.ascontiguousarray(np.stack([self.n, self.c_off, self.t_off], axis=1))
        self.d_bytes = torch.zeros(len(self.n), dtype=torch.int64, device=self.dev)
        d_tab = self.up(tab)   # named: the launch reads it
        _lib.call("tspgnn_graph_text_sizes", tab.ctypes.data, _lib.ptr(d_tab), _lib.ptr(self.A), _lib.ptr(self.Mw),
                  _lib.ptr(self.tours), len(self.n), int(self.n.max()), self.A.numel(), self.tours.numel(),
                  _lib.ptr(self.d_bytes), _lib.current_stream())
        self.sizes = self.d_bytes.cpu().numpy()
        return self.sizes

    def write(self, sizes=None, n_text=None):
        """``sizes``: what the kernel is told instead of its own sizes; -> the status array."""
        sizes = self.sizes if sizes is None else np.asarray(sizes, dtype=np.int64)
        self.b0 = np.cumsum(self.sizes) - self.sizes   # the files keep their true places
        n_text = int(self.sizes.sum()) + self.slack if n_text is None else n_text
        tab = np.ascontiguousarray(np.stack([self.n, self.c_off, self.t_off, self.b0], axis=1))
        self.d_text = torch.full((int(self.sizes.sum()) + self.slack,), ord("#"), dtype=torch.uint8, device=self.dev)
        d_status = torch.full((len(self.n),), -7, dtype=torch.int32, device=self.dev)
        d_tab, d_sizes = self.up(tab), self.up(sizes)   # named: the launch reads them
        _lib.call("tspgnn_graph_text_write", tab.ctypes.data, _lib.ptr(d_tab), _lib.ptr(self.A), _lib.ptr(self.Mw),
                  _lib.ptr(self.tours), len(self.n), int(self.n.max()), self.A.numel(), self.tours.numel(),
                  _lib.ptr(d_sizes), sizes.ctypes.data, _lib.ptr(self.d_text), n_text, _lib.ptr(d_status),
                  _lib.current_stream())
        self.text = self.d_text.cpu().numpy().tobytes()
        return d_status.cpu().numpy()

    def file(self, k):
        return self.text[int(self.b0[k]):int(self.b0[k] + self.sizes[k])]


def hand_made():
    """n = 4: a set pair of weight 0.0, the exponent forms, a 17-digit weight and an unset pair (1, 2)."""
    Ma = np.array([[0, 1, 1, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0]])
    Mw = np.array([[0.0, 0.0, 1e-05, 5e-324], [9.0, 0.0, 0.7071067811865476, 1e16],
                   [9.0, 9.0, 0.0, 0.30000000000000004], [9.0, 9.0, 9.0, 7.0]])
    return Ma, Mw, [0, 2, 3, 1]


def test_device_formatter_equals_the_host_entry(cuda_device):
    values = np.concatenate([np.array(cases.FIXED), cases.powers_of_two(), cases.powers_of_ten(),
                             cases.bit_patterns(100000)])
    want, want_len = host_f64_repr(values)
    d_x = torch.from_numpy(values).to(cuda_device)
    d_text = torch.full((REPR_BYTES * values.size,), 0x7E, dtype=torch.uint8, device=cuda_device)
    d_len = torch.zeros(values.size, dtype=torch.uint8, device=cuda_device)
    _lib.call("tspgnn_f64_repr", _lib.ptr(d_x), values.size, _lib.ptr(d_text), _lib.ptr(d_len), _lib.current_stream())
    length = d_len.cpu().numpy()
    assert np.array_equal(length, want_len)
    cells = d_text.cpu().numpy().reshape(-1, REPR_BYTES)
    keep = np.arange(REPR_BYTES)[None, :] < length[:, None]
    host = np.full_like(cells, 0x7E)
    host[keep] = np.frombuffer("".join(want).encode(), dtype=np.uint8)
    wrong = np.flatnonzero((cells != host).any(axis=1))   # the bytes past a value stay as they were
    assert wrong.size == 0, [(values[i].hex(), cells[i].tobytes(), want[i]) for i in wrong[:5]]
    _lib.call("tspgnn_f64_repr", None, 0, None, None, _lib.current_stream())   # count == 0: no-op


def test_hand_made_instance_through_the_two_kernels(cuda_device, tmp_path):
    inst = hand_made()
    want = host_bytes(tmp_path, inst)
    assert b"\n0 0.0 1e-05 5e-324 \n0 0 0 1e+16 \n0 0 0 0.30000000000000004 \n0 0 0 0 \n" in want   # what the case is for
    run = Launch([inst], cuda_device)
    assert run.size().tolist() == [len(want)]
    assert run.write().tolist() == [0]
    assert run.file(0) == want and run.text[len(want):] == b"#" * run.slack


GENERATED = {
    # name: (samples, nmin, nmax, (conn_min, conn_max), distances)
    "euclidean": (24, 4, 12, (1, 1), "euc_2D"),
    "sparse": (8, 4, 9, (0.3, 0.8), "euc_2D"),
    "random_metric": (8, 5, 10, (1, 1), "random"),
    "triangle_class": (2, 129, 140, (1, 1), "euc_2D"),
    "n256": (1, 256, 256, (1, 1), "euc_2D"),
}
_made = {}


def generated(name):
    """The dataset of a case, generated once, with its instances."""
    if name not in _made:
        samples, nmin, nmax, conn, distances = GENERATED[name]
        _seed(21)
        ds = DeviceDataset.generate(samples, nmin, nmax, conn[0], conn[1], distances=distances, metric=True, **KW)
        _made[name] = ds, ds.to_instances()
    return _made[name]


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_dataset_is_written_as_write_graph_writes_it(name, cuda_device, tmp_path):
    ds, insts = generated(name)
    out = tmp_path / "device"
    report = ds.write_directory(str(out))
    got = directory(str(out))
    assert sorted(got) == sorted("%d.graph" % i for i in range(len(ds)))
    for i, inst in enumerate(insts):
        assert got["%d.graph" % i] == host_bytes(tmp_path, inst), i
        Ma, Mw, route = read_graph(str(out / ("%d.graph" % i)))
        assert np.array_equal(Ma, inst[0]) and [int(x) for x in route] == inst[2]
        assert np.where(Ma != 0, Mw, 0.0).tobytes() == np.where(inst[0] != 0, inst[1], 0.0).tobytes()
    assert report["bytes"] == sum(len(b) for b in got.values())
    assert {"format", "download", "files"} <= set(report["times"]) and all(v >= 0 for v in report["times"].values())
    if name == "sparse":   # many "0" cells, and pairs that are not edges
        assert (ds.m < ds.n * (ds.n - 1) // 2).any()
    if name == "n256":
        assert b"\n254 255\n" in got["0.graph"]


def test_result_does_not_depend_on_text_bytes(cuda_device, tmp_path):
    ds, _ = generated("euclidean")
    whole, parts = tmp_path / "whole", tmp_path / "parts"
    ds.write_directory(str(whole))
    ds.write_directory(str(parts), text_bytes=1)   # every instance its own chunk
    assert directory(str(whole)) == directory(str(parts)) and len(directory(str(whole))) == len(ds)
    with pytest.raises(ValueError):
        ds.write_directory(str(parts), text_bytes=0)


def test_only_generated_datasets_write_directories(cuda_device, tmp_path):
    _, insts = generated("sparse")
    with pytest.raises(RuntimeError):
        DeviceDataset(insts).write_directory(str(tmp_path / "none"))


def test_create_dataset_writers_write_identical_directories(cuda_device, tmp_path):
    summaries = {}
    for writer in ("host", "device"):
        _seed(33)
        summaries[writer] = dataset.create_dataset(str(tmp_path / writer), 6, 10, 0.5, 1.0, samples=16, writer=writer, **KW)
        assert summaries[writer]["times"]["write"] > 0
    host = directory(str(tmp_path / "host"))
    assert len(host) == 16 and host == directory(str(tmp_path / "device"))
    assert np.array_equal(summaries["host"]["cost"], summaries["device"]["cost"])
    with pytest.raises(ValueError):
        dataset.create_dataset(str(tmp_path / "bad"), 6, 10, samples=1, writer="gpu", **KW)


def test_device_writer_refuses_what_it_cannot_print_before_any_launch(cuda_device, tmp_path):
    from tspgnn.graph_text import write_instances
    Ma, Mw, tour = hand_made()
    two = Ma.copy()
    two[0, 1] = 2
    for bad in ((two, Mw, tour), (Ma, Mw, tour[:3]), (Ma, Mw, tour + [0])):
        with pytest.raises(ValueError):
            write_instances(str(tmp_path / "refused"), [(Ma, Mw, tour), bad], cuda_device)
        assert not os.path.exists(str(tmp_path / "refused"))
    write_instances(str(tmp_path / "ok"), [(Ma, Mw, tour)], cuda_device)
    assert directory(str(tmp_path / "ok")) == {"0.graph": host_bytes(tmp_path, (Ma, Mw, tour))}


def test_guards(cuda_device, tmp_path):
    _, insts = generated("sparse")
    insts = insts[:3]
    want = [host_bytes(tmp_path, inst) for inst in insts]
    run = Launch(insts, cuda_device)
    assert run.size().tolist() == [len(b) for b in want]
    for delta in (-1, 1):   # a size that is off by one: that file's range stays as it was, its neighbours are written
        told = run.sizes.copy()
        told[1] += delta
        assert run.write(sizes=told).tolist() == [0, 1, 0]
        assert run.file(0) == want[0] and run.file(2) == want[2]
        assert run.file(1) == b"#" * len(want[1]) and run.text[-run.slack:] == b"#" * run.slack
    # a tour entry equal to n
    Ma, Mw, tour = insts[1]
    out = Launch([insts[0], (Ma, Mw, tour[:-1] + [len(tour)]), insts[2]], cuda_device)
    out.size()
    assert out.write().tolist() == [0, 2, 0]
    assert out.file(0) == want[0] and out.file(2) == want[2] and set(out.file(1)) == {ord("#")}
    # a text buffer that is one byte short: refused before any launch
    with pytest.raises(_lib.TspgnnError) as err:
        run.write(n_text=int(run.sizes.sum()) - 1)
    assert err.value.status == -1
    assert set(run.d_text.cpu().numpy().tolist()) == {ord("#")}
    # count == 0
    _lib.call("tspgnn_graph_text_sizes", None, None, None, None, None, 0, 8, 0, 0, None, _lib.current_stream())
    _lib.call("tspgnn_graph_text_write", None, None, None, None, None, 0, 8, 0, 0, None, None, None, 0, None,
              _lib.current_stream())
