"""``.graph`` files formatted on the GPU (csrc/graph_text.hip): the bytes instance_loader.write_graph(np.triu(Ma), Mw,
path, route=tour) writes, without a Python pass over the cells.

``write_files`` is the driver both public routes share -- DeviceDataset.write_directory, whose masks, fp64 matrices and
tours are on the device already, and create_dataset(writer='device'), which uploads them in ``write_instances``.  Per
group of instances (one set of flat device arrays): tspgnn_graph_text_sizes gives every file its length, the host takes
the prefix sums and cuts the group into chunks of at most ``text_bytes`` of text, and per chunk tspgnn_graph_text_write
formats the files side by side into one device buffer, which comes down in one copy to a pinned buffer; every file is
then one slice of that buffer handed to ``write``.  Pinned layout: file k of the chunk at [b0[k], b0[k] + bytes[k]), b0 the
exclusive prefix sums of bytes inside the chunk, no padding.
"""
import os
import time

import numpy as np
import torch

from . import _lib

DEFAULT_TEXT_BYTES = 1 << 28
REPR_BYTES = 24   # the longest repr(float): '-2.2250738585072014e-308'


def host_f64_repr(x):
    """[repr(float(v)) for v in x] through tspgnn_host_f64_repr: -> (list of str, uint8 lengths)."""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    text = np.zeros(REPR_BYTES * x.size, dtype=np.uint8)
    length = np.zeros(x.size, dtype=np.uint8)
    status = _lib.lib.tspgnn_host_f64_repr(x.ctypes.data, x.size, text.ctypes.data, length.ctypes.data)
    if status != 0:
        raise _lib.TspgnnError("tspgnn_host_f64_repr", status, _lib.lib.tspgnn_last_error().decode("utf-8", "replace"))
    raw = text.tobytes()
    return [raw[REPR_BYTES * i:REPR_BYTES * i + int(length[i])].decode("ascii") for i in range(x.size)], length


def _text_chunks(sizes, text_bytes):
    """(lo, hi) runs of consecutive files with at most text_bytes of text, and at least one file each."""
    runs, lo, acc = [], 0, 0
    for k, b in enumerate(sizes):
        if k > lo and acc + int(b) > text_bytes:
            runs.append((lo, k))
            lo, acc = k, 0
        acc += int(b)
    if len(sizes) > lo:
        runs.append((lo, len(sizes)))
    return runs


class _Buffers(object):
    """The device text buffer and its pinned twin, grown to the largest chunk seen (pinning is the expensive part)."""

    def __init__(self, dev):
        self.dev, self.text, self.pinned = dev, None, None

    def get(self, nbytes):
        if self.text is None or self.text.numel() < nbytes:
            self.text = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            self.pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return self.text, self.pinned


def _sync(dev):
    torch.cuda.synchronize(dev)
    return time.perf_counter()


def write_files(path, names, nc, c_off, t_off, n_cells, n_verts, d_A, d_Mw, d_tours, dev, text_bytes, times, buffers=None):
    """Writes ``{path}/{names[k]}.graph`` for the instances k of one group: nc[k] vertices, mask and fp64 matrix at cell
    c_off[k] of the flat device arrays d_A (uint8) / d_Mw (n_cells entries), tour at t_off[k] of d_tours (int32, n_verts
    entries).  Adds the seconds to times['sizes'], ['write'] (the two launches, synchronised), ['format'] (their sum),
    ['download'] and ['files'].  -> bytes written.  RuntimeError when the write kernel refuses an instance (a tour entry
    outside [0, n))."""
    C = len(nc)
    if C == 0:
        return 0
    if text_bytes < 1:
        raise ValueError("text_bytes=%r must be positive" % (text_bytes,))
    buffers = _Buffers(dev) if buffers is None else buffers
    nc = np.asarray(nc, dtype=np.int64)
    n_max = int(nc.max())
    with torch.cuda.device(dev):
        st = _lib.current_stream()
        t0 = _sync(dev)
        tab = np.ascontiguousarray(np.stack([nc, c_off, t_off], axis=1).astype(np.int64))
        d_tab = torch.from_numpy(tab).to(dev)
        d_bytes = torch.empty(C, dtype=torch.int64, device=dev)
        _lib.call("tspgnn_graph_text_sizes", tab.ctypes.data, _lib.ptr(d_tab), _lib.ptr(d_A), _lib.ptr(d_Mw),
                  _lib.ptr(d_tours), C, n_max, int(n_cells), int(n_verts), _lib.ptr(d_bytes), st)
        sizes = d_bytes.cpu().numpy()
        t1 = _sync(dev)
        times["sizes"] = times.get("sizes", 0.0) + t1 - t0
        times["format"] = times.get("format", 0.0) + t1 - t0
        for lo, hi in _text_chunks(sizes, text_bytes):
            t0 = _sync(dev)
            size = np.ascontiguousarray(sizes[lo:hi])
            b0 = np.cumsum(size) - size
            total = int(size.sum())
            d_text, pinned = buffers.get(total)
            tab4 = np.ascontiguousarray(np.stack([nc[lo:hi], c_off[lo:hi], t_off[lo:hi], b0], axis=1).astype(np.int64))
            d_tab4 = torch.from_numpy(tab4).to(dev)
            d_status = torch.empty(hi - lo, dtype=torch.int32, device=dev)
            _lib.call("tspgnn_graph_text_write", tab4.ctypes.data, _lib.ptr(d_tab4), _lib.ptr(d_A), _lib.ptr(d_Mw),
                      _lib.ptr(d_tours), hi - lo, int(nc[lo:hi].max()), int(n_cells), int(n_verts),
                      _lib.ptr(d_bytes[lo:hi]), size.ctypes.data, _lib.ptr(d_text), total, _lib.ptr(d_status), st)
            t1 = _sync(dev)
            pinned[:total].copy_(d_text[:total], non_blocking=True)
            status = d_status.cpu().numpy()
            t2 = _sync(dev)
            if status.any():
                k = int(np.flatnonzero(status)[0])
                raise RuntimeError("graph text: instance %s refused (status %d: %s)" % (
                    names[lo + k], status[k], "its tour leaves [0, n)" if status[k] == 2 else "its size changed"))
            view = memoryview(pinned.numpy())
            for k in range(hi - lo):
                with open(os.path.join(path, "%s.graph" % names[lo + k]), "wb") as out:
                    out.write(view[int(b0[k]):int(b0[k] + size[k])])
            t3 = time.perf_counter()
            for key, dt in (("write", t1 - t0), ("format", t1 - t0), ("download", t2 - t1), ("files", t3 - t2)):
                times[key] = times.get(key, 0.0) + dt
    return int(sizes.sum())


def check_instances(instances):
    """What the device route cannot print as write_graph does, found before any launch: ValueError for a mask whose upper
    triangle holds a non-zero entry other than 1 (write_graph lists the pair and prints 0 for it) or an entry on the
    diagonal, and for a tour that is not n entries long."""
    for k, (Ma, Mw, tour) in enumerate(instances):
        Ma = np.asarray(Ma)
        n = Ma.shape[0]
        if Ma.ndim != 2 or Ma.shape[1] != n or np.shape(Mw) != Ma.shape:
            raise ValueError("instance %d: Ma %s and Mw %s must be the same square shape" % (k, Ma.shape, np.shape(Mw)))
        up = np.triu(Ma)
        if np.any((up != 0) & (up != 1)):
            raise ValueError("instance %d: the mask holds a non-zero entry other than 1" % k)
        if np.any(np.diagonal(up) != 0):
            raise ValueError("instance %d: the mask has an entry on the diagonal" % k)
        if tour is None or len(tour) != n:
            raise ValueError("instance %d: the tour must have n=%d entries, got %s" % (
                k, n, "none" if tour is None else len(tour)))


def write_instances(path, instances, dev, text_bytes=DEFAULT_TEXT_BYTES, chunk_bytes=1 << 28, times=None):
    """``{path}/{i}.graph`` for instance i of the list of (Ma, Mw, tour), as write_graph(np.triu(Ma), Mw, .., route=tour)
    writes them: np.triu(Ma) as uint8, the fp64 Mw and the tours go up in chunks of at most chunk_bytes of matrices and
    write_files does the rest (times['upload']: packing and copying them).  Every instance is checked first
    (check_instances).  -> bytes written."""
    instances = list(instances)
    check_instances(instances)
    times = {} if times is None else times
    os.makedirs(path, exist_ok=True)
    ns = np.array([np.shape(Ma)[0] for Ma, _, _ in instances], dtype=np.int64)
    buffers, written, lo = _Buffers(dev), 0, 0
    while lo < len(ns):
        hi, acc = lo, 0
        while hi < len(ns) and (hi == lo or acc + 8 * int(ns[hi]) ** 2 <= chunk_bytes):
            acc += 8 * int(ns[hi]) ** 2
            hi += 1
        t0 = time.perf_counter()
        nc = ns[lo:hi]
        c_off = np.cumsum(nc * nc) - nc * nc
        t_off = np.cumsum(nc) - nc
        A = np.concatenate([(np.triu(np.asarray(Ma)) != 0).astype(np.uint8).reshape(-1) for Ma, _, _ in instances[lo:hi]])
        Mw = np.concatenate([np.asarray(Mw, dtype=np.float64).reshape(-1) for _, Mw, _ in instances[lo:hi]])
        tours = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for _, _, t in instances[lo:hi]])
        if tours.size and (tours.min() < -(2 ** 31) or tours.max() >= 2 ** 31):
            raise ValueError("a tour entry does not fit int32")
        d_A, d_Mw, d_tours = (torch.from_numpy(a).to(dev) for a in (A, Mw, tours.astype(np.int32)))
        times["upload"] = times.get("upload", 0.0) + _sync(dev) - t0
        written += write_files(path, list(range(lo, hi)), nc, c_off, t_off, A.size, tours.size, d_A, d_Mw, d_tours, dev,
                               text_bytes, times, buffers)
        lo = hi
    return written
