"""``.graph`` files formatted on the GPU (csrc/graph_text.hip): the bytes instance_loader.write_graph(np.triu(Ma), Mw,
path, route=tour) writes, without a Python pass over the cells.

``write_files`` is the driver both public routes share -- DeviceDataset.write_directory, whose masks, fp64 matrices and
tours are on the device already, and create_dataset(writer='device'), which uploads them in ``write_instances``.  Per
group of instances (one set of flat device arrays): tspgnn_graph_text_sizes gives every file its length, the host takes
the prefix sums and cuts the group into chunks of at most ``text_bytes`` of text, and per chunk tspgnn_graph_text_write
formats the files side by side into one device buffer, which comes down in one copy to a pinned buffer; every file is
then one slice of that buffer handed to ``write``.  Pinned layout: file k of the chunk at [b0[k], b0[k] + bytes[k]), b0 the
exclusive prefix sums of bytes inside the chunk, no padding.

``read_files`` is the way back (csrc/graph_parse.hip), behind DeviceDataset.from_directory(reader='device'): per chunk of
at most ``text_bytes`` of text the raw bytes of the files go into a pinned buffer (each file on a 16-byte border) and up
in one copy, tspgnn_graph_text_scan gives every file its n, the host takes the prefix sums, and
tspgnn_graph_text_parse fills the uint8 masks, fp64 matrices and int32 tours tspgnn_pack_dataset takes.  The host makes no
pass over cells, tokens or lines.
"""
import collections
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


def token_arrays(tokens):
    """The arguments of tspgnn_f64_parse for a list of tokens (bytes or str): -> (uint8 buffer, the tokens end to end; int64
    offsets; int32 lengths)."""
    raw = [t if isinstance(t, bytes) else t.encode("utf-8") for t in tokens]
    length = np.array([len(t) for t in raw], dtype=np.int32)
    off = np.cumsum(length, dtype=np.int64) - length
    return np.frombuffer(bytearray(b"".join(raw) + b"\0"), dtype=np.uint8)[:-1], off, length


def host_f64_parse(tokens, mode=0):
    """float(t) of every token (bytes or str) through tspgnn_host_f64_parse: -> (uint64 bits, uint8 status); status 0
    parsed, 1 malformed, 2 outside the device grammar (include/tspgnn.h)."""
    buf, off, length = token_arrays(tokens)
    bits = np.zeros(len(off), dtype=np.uint64)
    status = np.zeros(len(off), dtype=np.uint8)
    rc = _lib.lib.tspgnn_host_f64_parse(buf.ctypes.data, buf.size, off.ctypes.data, length.ctypes.data, len(off),
                                        int(mode), bits.ctypes.data, status.ctypes.data)
    if rc != 0:
        raise _lib.TspgnnError("tspgnn_host_f64_parse", rc, _lib.lib.tspgnn_last_error().decode("utf-8", "replace"))
    return bits, status


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


# ---------------------------------------------------------------------------------------------------------- reading
MAX_FILE_BYTES = 1 << 24   # the longest file write_graph makes at n = 256 is below 2 MiB
READ_STATUS = {
    3: "no DIMENSION, or n <= 0",
    4: "a section is missing",
    5: "a pair outside [0, n)",
    6: "fewer than n^2 weight tokens, or a malformed one",
    7: "a tour entry outside [0, n)",
    8: "n outside [4, 256]",
    9: "a pair with i >= j",
    10: "the tour does not have n entries",
    11: "a weight token outside the device grammar",
}
# One chunk of read_files: the files [lo, hi) of the list; nc: their n (int64); c_off / t_off: a file's first cell in A / Mw
# and first entry in tours, with the totals n_cells / n_verts; the device arrays A (uint8 mask, symmetric), Mw (fp64), tours (int32);
# the host array m (set pairs, int64).
ReadChunk = collections.namedtuple("ReadChunk", "lo hi nc c_off t_off n_cells n_verts A Mw tours m")


def _refuse(paths, lo, status):
    """ValueError for the first file of a chunk with a non-zero status."""
    k = int(np.flatnonzero(status)[0])
    code = int(status[k])
    raise ValueError("graph text: %s: status %d: %s%s" % (
        paths[lo + k], code, READ_STATUS.get(code, "refused"),
        " (reader='host' reads such a file)" if 8 <= code <= 11 else ""))


def read_files(paths, dev, text_bytes=DEFAULT_TEXT_BYTES, times=None):
    """Reads the ``.graph`` files ``paths`` on the GPU ``dev``: yields one ReadChunk per run of consecutive files with at
    most ``text_bytes`` of text (at least one file).  A chunk's text dies with the iteration; its arrays are the
    caller's.  Adds the seconds to times['files'] (reading the bytes), ['upload'], ['scan'] and ['parse'] (each launch
    with the download of its result, synchronised).  ValueError before anything is yielded for a chunk: a file above
    MAX_FILE_BYTES (before any file is read), a file either launch refuses -- the first such file and its status in
    words."""
    paths = list(paths)
    if text_bytes < 1:
        raise ValueError("text_bytes=%r must be positive" % (text_bytes,))
    times = {} if times is None else times
    sizes = np.array([os.path.getsize(p) for p in paths], dtype=np.int64)
    for p, b in zip(paths, sizes):
        if b > MAX_FILE_BYTES:
            raise ValueError("graph text: %s: %d bytes, more than the %d a file may have" % (p, b, MAX_FILE_BYTES))
    padded = (sizes + 15) // 16 * 16   # every file begins on a 16-byte border of the buffer
    buffers = _Buffers(dev)
    with torch.cuda.device(dev):
        st = _lib.current_stream()
        for lo, hi in _text_chunks(padded, text_bytes):
            t0 = time.perf_counter()
            C = hi - lo
            size = np.ascontiguousarray(sizes[lo:hi])
            b0 = np.cumsum(padded[lo:hi]) - padded[lo:hi]
            total = max(int(padded[lo:hi].sum()), 16)
            d_text, pinned = buffers.get(total)
            view = memoryview(pinned.numpy())
            for k in range(C):
                with open(paths[lo + k], "rb") as f:
                    if f.readinto(view[int(b0[k]):int(b0[k] + size[k])]) != size[k] or f.read(1):
                        raise ValueError("graph text: %s changed while it was read" % paths[lo + k])
            t1 = time.perf_counter()
            d_text[:total].copy_(pinned[:total], non_blocking=True)
            tab2 = np.ascontiguousarray(np.stack([b0, size], axis=1).astype(np.int64))
            d_tab2 = torch.from_numpy(tab2).to(dev)
            t2 = _sync(dev)
            d_info = torch.empty((C, 8), dtype=torch.int32, device=dev)
            _lib.call("tspgnn_graph_text_scan", tab2.ctypes.data, _lib.ptr(d_tab2), _lib.ptr(d_text), total, C,
                      _lib.ptr(d_info), st)
            info = d_info.cpu().numpy()
            t3 = _sync(dev)
            if info[:, 0].any():
                _refuse(paths, lo, info[:, 0])
            nc = info[:, 1].astype(np.int64)
            c_off = np.cumsum(nc * nc) - nc * nc
            t_off = np.cumsum(nc) - nc
            n_cells, n_verts = int((nc * nc).sum()), int(nc.sum())
            tab5 = np.ascontiguousarray(np.stack([b0, size, nc, c_off, t_off], axis=1).astype(np.int64))
            d_tab5 = torch.from_numpy(tab5).to(dev)
            d_A = torch.empty(n_cells, dtype=torch.uint8, device=dev)
            d_Mw = torch.empty(n_cells, dtype=torch.float64, device=dev)
            d_tours = torch.empty(n_verts, dtype=torch.int32, device=dev)
            d_ms = torch.empty((2, C), dtype=torch.int32, device=dev)
            _lib.call("tspgnn_graph_text_parse", tab5.ctypes.data, _lib.ptr(d_tab5), _lib.ptr(d_text), total, C,
                      int(nc.max()), n_cells, n_verts, _lib.ptr(d_A), _lib.ptr(d_Mw), _lib.ptr(d_tours), _lib.ptr(d_ms[0]),
                      _lib.ptr(d_ms[1]), st)
            ms = d_ms.cpu().numpy()
            t4 = _sync(dev)
            for key, dt in (("files", t1 - t0), ("upload", t2 - t1), ("scan", t3 - t2), ("parse", t4 - t3)):
                times[key] = times.get(key, 0.0) + dt
            times["bytes"] = times.get("bytes", 0) + int(size.sum())
            if ms[1].any():
                _refuse(paths, lo, ms[1])
            yield ReadChunk(lo, hi, nc, c_off, t_off, n_cells, n_verts, d_A, d_Mw, d_tours, ms[0].astype(np.int64))
