"""Device-resident datasets: the instances are uploaded once, a batch is a list of instance ids and one launch.

What a batch needs from an instance does not depend on the batch, apart from two offsets and one factor: the edge list in
np.nonzero order, the fp32 weights, the CSR by vertex and the tour cost are properties of the INSTANCE; the vertex offset,
the edge offset and (1 -/+ dev) are properties of the BATCH.  ``DeviceDataset`` packs every instance once on the host with
the native packers (tspgnn_host_stage_batch / tspgnn_host_route_cost: edge order and arithmetic are the ones
tests/test_packer.py pins), keeps the concatenation in HBM, and ``batch(indices)`` runs tspgnn_gather_batch
(csrc/batch_gather.hip) over it: the bytes tspgnn_host_stage_batch would write for the same instance list, without a host
pass over the matrices and without the upload.

Layout (device, int32 offsets -- ``MAX_CSR_ENTRIES``):
    inst   int32[I][4]       n, m, first edge, first vertex of instance i (prefix sums)
    uv     int32[sum m][2]   local endpoint ids          w    float[sum m]     (float)Mw[i, j]
    rowptr int32[sum (n+1)]  local CSR by vertex         eid  int32[2 sum m]   ascending edge ids inside a vertex
    cost   double[I]         route_cost, closing-pair quirk included
The host keeps ``n`` and ``m`` (int64): a batch's e_start / v_start are their prefix sums over the index list
(``plan_batch``), uploaded with the ids as one small pinned buffer.

``DeviceDataset.generate`` fills the same arrays without the host pass: the reference's random draws stay on the host as
flat streams (dataset.draw_streams) and csrc/dataset_build.hip builds, penalises and packs the instances around the
existing closure, search and bound kernels.
"""
import collections
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib
from . import dataset as D
from . import graph_text as G
from .instance_loader import read_graph, route_cost
from .parallel import stage_instances, stage_layout, staged_batch

MAX_CSR_ENTRIES = 2 ** 31   # 2 * sum(m) must stay below: CSR positions and edge ids are int32 on the device
_CHUNK = 1024               # instances per host packing call (bounds the scratch of the one-off preprocessing)
_PLAN_CACHE = 64            # work plans kept per dataset (an epoch of fixed-size batches needs one)
_RING = 4                   # pinned (ids, e_start, v_start) buffers in flight


def check_size(total_edges):
    """Raises ValueError when a dataset of ``total_edges`` edges does not fit the int32 offsets of the device layout."""
    if 2 * int(total_edges) >= MAX_CSR_ENTRIES:
        raise ValueError("DeviceDataset: %d edges: 2 * sum(m) must stay below 2^31 (int32 CSR offsets); split the dataset"
                         % int(total_edges))


def preprocess(instances):
    """Packs every (Ma, Mw, route) once: -> dict of NumPy arrays ``n``, ``m`` (int64), ``e0``, ``v0`` (int64 prefix sums,
    I + 1 entries), ``uv`` int32[sum m, 2] (local ids), ``w`` float32[sum m], ``rowptr`` int32[sum (n + 1)], ``eid``
    int32[2 sum m] (local ids), ``cost`` float64[I].  Raises like create_batch: ValueError for a non-square adjacency or a
    weight matrix of another shape, IndexError for a route that leaves its graph."""
    instances = list(instances)
    I = len(instances)
    for k, (Ma, Mw, _) in enumerate(instances):
        sa, sw = np.shape(Ma), np.shape(Mw)
        if len(sa) != 2 or sa[0] != sa[1]:
            raise ValueError("DeviceDataset: instance %d: the adjacency matrix must be square, got %s" % (k, sa))
        if sw != sa:
            raise ValueError("DeviceDataset: instance %d: weight matrix %s does not match adjacency matrix %s" % (k, sw, sa))
    n = np.array([np.shape(Ma)[0] for Ma, _, _ in instances], dtype=np.int64)
    m = np.array([int(np.count_nonzero(Ma)) for Ma, _, _ in instances], dtype=np.int64)
    check_size(m.sum())
    e0 = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    v0 = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    uv = np.empty((int(e0[-1]), 2), dtype=np.int32)
    w = np.empty(int(e0[-1]), dtype=np.float32)
    eid = np.empty(2 * int(e0[-1]), dtype=np.int32)
    rowptr = np.empty(int(v0[-1]) + I, dtype=np.int32)
    cost = np.empty(I, dtype=np.float64)
    for lo, hi in D._spans(I, _CHUNK):
        # one tspgnn_host_stage_batch call over the chunk with dev = 0: its endpoints, CSR and (float)Mw are the batch's up
        # to the chunk-relative offsets taken off below (the cost column is not used: the fp64 cost is kept instead)
        Mc, Nc, Bc = int(e0[hi] - e0[lo]), int(v0[hi] - v0[lo]), hi - lo
        off, sizes, total = stage_layout(Mc, Nc, Bc, 0)
        buf = np.empty(total, dtype=np.uint8)
        stage_instances(instances[lo:hi], 0.0, None, Mc, Nc, buf.ctypes.data, off)
        g = lambda k, dt: buf[off[k]:off[k] + sizes[k]].view(dt)
        el, vl = (e0[lo:hi] - e0[lo]).astype(np.int32), (v0[lo:hi] - v0[lo]).astype(np.int32)   # chunk-relative starts
        mc, nc = m[lo:hi], n[lo:hi]
        uv[e0[lo]:e0[hi]] = g(0, np.int32).reshape(Mc, 2) - np.repeat(vl, mc)[:, None]
        w[e0[lo]:e0[hi]] = g(3, np.float32).reshape(Mc, 2)[:, 0]
        eid[2 * e0[lo]:2 * e0[hi]] = g(1, np.int32) - np.repeat(el, 2 * mc)
        # n + 1 row pointers per instance: the chunk's rowptr[v_start[b] .. v_start[b] + n], less 2 * e_start[b]
        take = np.arange(Nc + Bc) - np.repeat(np.arange(Bc), nc + 1)
        rowptr[v0[lo] + lo:v0[hi] + hi] = g(2, np.int32)[take] - np.repeat(2 * el, nc + 1)
        for k in range(lo, hi):
            cost[k] = route_cost(instances[k][1], instances[k][2])
    return {"n": n, "m": m, "e0": e0, "v0": v0, "uv": uv, "w": w, "rowptr": rowptr, "eid": eid, "cost": cost}


def plan_batch(n, m, indices):
    """The batch-side half of a gather: -> (e_start int32[B + 1], v_start int32[B + 1], M, N, labels int64[B]) for the
    instance list ``indices`` -- the prefix sums create_batch returns as EV.blocks, and its route_exists.  IndexError for
    an id outside the dataset."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= len(n)):
        raise IndexError("DeviceDataset: instance id outside [0, %d)" % len(n))
    e_start = np.concatenate([[0], np.cumsum(np.asarray(m, dtype=np.int64)[idx])])
    v_start = np.concatenate([[0], np.cumsum(np.asarray(n, dtype=np.int64)[idx])])
    check_size(e_start[-1])
    return (e_start.astype(np.int32), v_start.astype(np.int32), int(e_start[-1]), int(v_start[-1]),
            np.arange(idx.size, dtype=np.int64) % 2)


def epoch_indices(n_instances, batch_size, shuffle=True, rng=None):
    """Index lists of one epoch, as InstanceLoader.get_instances / get_batches visit a directory: n_instances //
    batch_size lists of 2 * batch_size ids, every instance twice in a row (labels 0, 1); with ``shuffle`` the order is
    drawn from ``rng`` (a numpy.random.RandomState; None: numpy's global one)."""
    order = np.arange(n_instances, dtype=np.int64)
    if shuffle:
        order = (np.random if rng is None else rng).permutation(n_instances).astype(np.int64)
    bs = int(batch_size)
    return [np.repeat(order[k * bs:(k + 1) * bs], 2) for k in range(n_instances // bs)]


def _segments(flat, starts, lens):
    """flat[starts[k]:starts[k] + lens[k]] for every k, concatenated (one fancy-indexing pass over a 1-D stream)."""
    lens = np.asarray(lens, dtype=np.int64)
    first = np.cumsum(lens) - lens
    return flat[np.arange(int(lens.sum()), dtype=np.int64) + np.repeat(np.asarray(starts, dtype=np.int64) - first, lens)]


def _prefix(lens):
    """Exclusive prefix sums of ``lens`` (int64, one entry per element) and their total."""
    lens = np.asarray(lens, dtype=np.int64)
    ends = np.cumsum(lens)
    return ends - lens, int(ends[-1]) if len(lens) else 0


def _default_device(device):
    """``device``, or the current HIP device when it is None."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceDataset needs an MI355X (no HIP device visible)")
        device = "cuda:%d" % torch.cuda.current_device()
    return torch.device(device)


def _clock(dev):
    torch.cuda.synchronize(dev)
    return time.perf_counter()


# ---------------------------------------------------------------------------------------------- the phases of generate
_GENERATE_KW = ("restarts", "kicks", "lb_iters", "seed", "neighbors", "max_nodes")

# generate's checked arguments: small / large / bb as dataset._label_settings returns them, the search's seed and
# neighbors, random_w (distances == 'random'), closes (the weights get their metric closure), dev.
_Settings = collections.namedtuple("_Settings", "small large bb seed neighbors random_w closes dev")
# One labelled chunk of generate.  pos: its stream positions (int64); nc: their n; c_off / t_off: an instance's first cell
# in A / Mw and first vertex in tours, with the totals n_cells / n_verts; the device arrays A (uint8 mask), Mw (fp64) and
# tours (int32); the host arrays m (edges), lb and, with the branch and bound, status / nodes (else None).
_Chunk = collections.namedtuple("_Chunk", "pos nc c_off t_off n_cells n_verts n_max A Mw tours m lb status nodes")
# What a generated dataset keeps of a chunk for to_instances() and write_directory(): the first seven fields of _Chunk
# and its device arrays A, Mw and tours.
_Kept = collections.namedtuple("_Kept", "pos nc c_off t_off n_cells n_verts A Mw tours")


def _generate_settings(samples, nmin, nmax, distances, metric, device, exact, chunk_bytes, solve_kw):
    """Every check of generate that needs no draw -> _Settings."""
    unknown = sorted(set(solve_kw) - set(_GENERATE_KW))
    if unknown:
        raise TypeError("DeviceDataset.generate: unexpected keyword %s (label_tours' %s)" % (unknown, list(_GENERATE_KW)))
    if not 4 <= nmin <= nmax <= D.MAX_N_TRI:
        raise ValueError("DeviceDataset.generate: 4 <= nmin <= nmax <= %d, got nmin=%r nmax=%r" % (D.MAX_N_TRI, nmin, nmax))
    if samples < 0 or chunk_bytes < 1:
        raise ValueError("DeviceDataset.generate: samples=%r must be >= 0 and chunk_bytes=%r positive" % (samples, chunk_bytes))
    if distances not in ("euc_2D", "random"):
        raise ValueError("distances=%r must be 'euc_2D' or 'random'" % (distances,))
    small, large, bb = D._label_settings(solve_kw.get("restarts"), solve_kw.get("kicks"), solve_kw.get("lb_iters"),
                                         solve_kw.get("neighbors"), exact, solve_kw.get("max_nodes"))
    dev = _default_device(device)
    if dev.type != "cuda":
        raise ValueError("DeviceDataset.generate: device=%r: the instances are made by HIP kernels" % str(dev))
    return _Settings(small, large, bb, solve_kw.get("seed", 0), solve_kw.get("neighbors"), distances == "random",
                     D._closes(distances, metric), dev)


def _plan_chunks(ns, chunk_bytes):
    """[(tri, stream positions int64)] in launch order: by n, the two size classes apart (as label_tours), each chunk at
    most chunk_bytes of fp64 matrices."""
    order = np.argsort(ns, kind="stable")
    return [(tri, np.array(run, dtype=np.int64)) for tri, sel in D._split(ns[order])
            for run in D._byte_chunks(order[sel], ns, chunk_bytes)]


def _label_chunk(S, tri, pos, cfg, st, times):
    """One chunk of generate, from the streams ``S`` at positions ``pos``: build the instances, close their weights (the
    tiers apart), penalise them for the layout ``tri`` and label them.  -> _Chunk.  The seconds go to times['build'],
    ['closure'], ['search'] and ['bound'] | ['exact'].  The streams' device copies and the search input die with the call."""
    dev = cfg.dev
    t0 = _clock(dev)
    nc = S["n"][pos].astype(np.int64)
    C, n_max = len(pos), int(nc.max())
    pairs = nc * (nc - 1) // 2
    p_off, n_pairs = _prefix(pairs)
    t_off, n_verts = _prefix(nc)
    c_off, n_cells = _prefix(nc * nc)
    w_off, n_floats = _prefix(pairs if tri else nc * nc)
    d_adj = D._to_device(_segments(S["adj_u"], S["pair_off"][pos], pairs), dev)
    d_coord = D._to_device(_segments(S["wts"], S["pair_off"][pos], pairs) if cfg.random_w else
                           _segments(S["pts"], 2 * S["vert_off"][pos], 2 * nc), dev)
    d_perm = D._to_device(_segments(S["perm"], S["vert_off"][pos], nc), dev)
    d_conn = D._to_device(S["conn"][pos], dev)
    tab = np.ascontiguousarray(np.stack([nc, p_off, t_off, c_off], axis=1))
    d_tab = D._to_device(tab, dev)
    d_Mw = torch.empty(n_cells, dtype=torch.float64, device=dev)
    d_A = torch.empty(n_cells, dtype=torch.uint8, device=dev)
    d_m = torch.empty(C, dtype=torch.int32, device=dev)
    _lib.call("tspgnn_build_instances", tab.ctypes.data, _lib.ptr(d_tab), _lib.ptr(d_conn), _lib.ptr(d_adj),
              _lib.ptr(d_coord), _lib.ptr(d_perm), int(cfg.random_w), C, n_max, n_pairs, n_verts, n_cells,
              _lib.ptr(d_Mw), _lib.ptr(d_A), _lib.ptr(d_m), st)
    d_coff, d_n = D._to_device(c_off, dev), D._to_device(nc.astype(np.int32), dev)
    t1 = _clock(dev)
    D._add_time(times, "build", t1 - t0)
    if cfg.closes:   # the tiers apart, as metric_closure: a small instance is closed in LDS
        cut = int(np.searchsorted(nc, D.CLOSURE_LDS_MAX_N, side="right"))
        for lo, hi in ((0, cut), (cut, C)):
            if hi > lo:
                _lib.call("tspgnn_metric_closure", _lib.ptr(d_Mw), _lib.ptr(d_coff[lo:hi]), _lib.ptr(d_n[lo:hi]),
                          hi - lo, int(nc[lo:hi].max()), st)
        t0 = _clock(dev)
        D._add_time(times, "closure", t0 - t1)
        t1 = t0
    ptab = np.ascontiguousarray(np.stack([nc, c_off, w_off], axis=1))
    d_ptab = D._to_device(ptab, dev)
    d_W = torch.empty(n_floats, dtype=torch.float32, device=dev)
    _lib.call("tspgnn_penalise_instances", ptab.ctypes.data, _lib.ptr(d_ptab), _lib.ptr(d_A), _lib.ptr(d_Mw), C,
              n_max, int(tri), n_cells, n_floats, _lib.ptr(d_W), st)
    arrays = D.LabelArrays(nc.astype(np.int32), d_W, D._to_device(w_off, dev), D._to_device(t_off, dev), d_n,
                           D._to_device(pos, dev), d_perm, torch.empty(n_verts, dtype=torch.int32, device=dev),
                           torch.empty(C, dtype=torch.float32, device=dev),
                           torch.empty(C, dtype=torch.float64, device=dev))
    (restarts, kicks, lb_iters), bb = (cfg.large if tri else cfg.small), (None if tri else cfg.bb)
    t1b, t2, t3, d_stat, d_nodes = D._launch_labels(dev, arrays, restarts=restarts, kicks=kicks, seed=cfg.seed,
                                                    lb_iters=lb_iters, chunk=D.DEFAULT_CHUNK, tri=tri,
                                                    neighbors=cfg.neighbors, exact=bb)
    D._add_time(times, "build", t1b - t1)
    D._add_time(times, "search", t2 - t1b)
    D._add_time(times, "bound" if bb is None else "exact", t3 - t2)
    return _Chunk(pos, nc, c_off, t_off, n_cells, n_verts, n_max, d_A, d_Mw, arrays.tours, d_m.cpu().numpy(),
                  arrays.lb.cpu().numpy(), None if bb is None else d_stat.cpu().numpy(),
                  None if bb is None else d_nodes.cpu().numpy())


def _summary(n64, chunks, file_cost, cyc, feas, exact, times):
    """create_dataset's summary dict from the labelled chunks and tspgnn_pack_dataset's per-instance outputs."""
    I = len(n64)
    lb = np.full(I, np.nan)
    status, nodes = np.full(I, 2, dtype=np.int64), np.zeros(I, dtype=np.int64)
    for c in chunks:
        lb[c.pos] = c.lb
        if c.status is not None:
            status[c.pos], nodes[c.pos] = c.status, c.nodes
    summary = {"samples": I, "n": n64.copy(), "cost": cyc, "lb": lb, "target": n64 * file_cost, "feasible": feas,
               "times": times}
    if exact:
        summary["proved"], summary["nodes"] = status == 0, nodes
    summary["gap"] = (cyc - lb) / np.where(cyc > 0, cyc, 1.0)
    summary["certified_fraction"] = D.certify(summary, 0.02)["fraction"]
    return summary


class DeviceDataset(object):
    """A list of (Ma, Mw, route) -- as read_graph returns them -- resident on one GPU; ``DeviceDataset.generate`` makes
    the set draw_instances + label_tours would make without a host pass over the matrices.

        ds = DeviceDataset(instances)                        # or DeviceDataset.generate(2 ** 15, 20, 40)
        for batch in ds.get_batches(64, dev=0.02, time_steps=32, rng=np.random.RandomState(0)):
            run_batch(sess, model, batch, ...)               # or sess.forward(batch) / sess.train_step(batch)

        b = ds.batch(ids, time_steps=32)                     # serving: one buffer, one captured graph
        replay = sess.capture_forward(b)
        for ids in stream_of_index_lists_of_that_shape:
            ds.batch(ids, time_steps=32, out=b); out = replay()

    ``device='cpu'`` is plumbing only (host tests): the arrays stay on the host and batch() raises."""

    def __init__(self, instances, device=None, routes=False):
        """``routes=True`` keeps the instances' tours on the device as well (int32, 4 sum n bytes): ``batch`` then adds one
        tspgnn_route_edge_marks launch and the batch carries ``route_edges``, the marks a route-head network trains on
        (build_network(d, route_head=True)); every route must be a permutation of its instance's vertices (ValueError)."""
        self.device = _default_device(device)
        instances = list(instances)
        host = preprocess(instances)
        self.n, self.m = host["n"], host["m"]
        I = len(self.n)
        inst = np.stack([self.n, self.m, host["e0"][:-1], host["v0"][:-1]], axis=1).astype(np.int32).reshape(I, 4)
        self._inst, self._uv, self._w, self._rowptr, self._eid, self._cost = (
            D._to_device(a, self.device) for a in (inst, host["uv"], host["w"], host["rowptr"], host["eid"], host["cost"]))
        self._init_batching()
        if routes:
            from .route_head import check_tour
            tours = [check_tour(k, r, int(self.n[k])) for k, (_, _, r) in enumerate(instances)]
            self._keep_routes(np.concatenate(tours) if tours else np.zeros(0, dtype=np.int64))

    def _init_batching(self):
        self._plans = {}     # (e_start bytes, v_start bytes) -> (device int32 plan or None, meta or None)
        self._ring, self._next = [None] * _RING, 0   # [pinned int32 buffer, its device copy, event of the launch that read it]
        self.summary = self.tours = self._matrices = None   # generate() fills these
        self._routes = self._route_v0 = None                # routes=True: the tours on the device, their int32 offsets (host)

    def _keep_routes(self, flat, on_device=None):
        """routes=True: ``flat`` -- every instance's tour in local ids, concatenated in instance order (host array) -- is
        checked (a permutation per instance; ValueError naming the first that is not, before anything is kept) and kept on
        the device as int32; ``on_device``: the same values already there."""
        from .route_head import MAX_N, MIN_N, check_tour
        flat = np.asarray(flat).reshape(-1)
        v0, N = _prefix(self.n)
        if len(self.n) and (self.n.min() < MIN_N or self.n.max() > MAX_N):
            raise ValueError("DeviceDataset(routes=True): instances of %d..%d vertices; the marks take %d <= n <= %d"
                             % (self.n.min(), self.n.max(), MIN_N, MAX_N))
        if flat.shape[0] != N:
            raise ValueError("DeviceDataset(routes=True): the routes hold %d entries for %d vertices: every route is a "
                             "permutation of its instance's vertices" % (flat.shape[0], N))
        for k in range(len(self.n)):
            check_tour(k, flat[v0[k]:v0[k] + self.n[k]], int(self.n[k]))
        self._routes = on_device if on_device is not None else D._to_device(flat.astype(np.int32), self.device)
        self._route_v0 = v0.astype(np.int32)

    @classmethod
    def _adopt(cls, device, n, m, inst, uv, w, rowptr, eid, cost):
        """A dataset over arrays that are already on ``device`` in the layout of the module docstring (generate);
        n, m: the host copies (int64)."""
        self = cls.__new__(cls)
        self.device = torch.device(device)
        self.n, self.m = np.asarray(n, dtype=np.int64), np.asarray(m, dtype=np.int64)
        self._inst, self._uv, self._w, self._rowptr, self._eid, self._cost = inst, uv, w, rowptr, eid, cost
        self._init_batching()
        return self

    def __len__(self):
        return len(self.n)

    @classmethod
    def from_directory(cls, path, device=None, reader="host", text_bytes=G.DEFAULT_TEXT_BYTES, keep_matrices=False,
                       routes=False):
        """Every file of a ``.graph`` directory, in sorted order.  reader='host': read_graph per file and the host packers
        (text_bytes and keep_matrices are not used).  reader='device': the raw bytes go up in chunks of at most
        ``text_bytes`` of text and the files are taken apart (csrc/graph_parse.hip, graph_text.read_files) and packed
        (tspgnn_pack_dataset) on the GPU: the same dataset arrays, without a host pass over cells, tokens or lines; the
        result does not depend on text_bytes.  That route reads the files write_graph(np.triu(Ma), Mw, ...) makes -- 4 <= n
        <= 256, pairs with i < j, a tour of n entries, weights in the spellings of repr -- and raises ValueError, naming the
        first file and why, for a file it cannot read, before the dataset exists.  keep_matrices: the masks, fp64
        matrices and tours stay on the device as generate keeps them, for to_instances() and write_directory().
        ``read_times`` then holds the seconds of 'files', 'upload', 'scan', 'parse' and 'pack' and the 'bytes' of text.
        routes=True, with either reader: the files' tours stay on the device for the route marks (see __init__)."""
        if reader not in ("host", "device"):
            raise ValueError("DeviceDataset.from_directory: reader=%r must be 'host' or 'device'" % (reader,))
        if reader == "host":
            return cls([read_graph(os.path.join(path, f)) for f in sorted(os.listdir(path))], device=device, routes=routes)
        dev = _default_device(device)
        if dev.type != "cuda":
            raise ValueError("DeviceDataset.from_directory: device=%r: the files are read by HIP kernels" % str(dev))
        return cls._read(path, dev, text_bytes, keep_matrices, routes)

    @classmethod
    def _read(cls, path, dev, text_bytes, keep, routes=False):
        """from_directory(reader='device'): one tspgnn_pack_dataset launch per chunk of read_files into chunk-sized arrays
        (uv, eid and rowptr are instance-local, so the dataset's arrays are the chunks' concatenated), ``inst`` from the
        host prefix sums."""
        paths = [os.path.join(path, f) for f in sorted(os.listdir(path))]
        times = {"files": 0.0, "upload": 0.0, "scan": 0.0, "parse": 0.0, "pack": 0.0, "bytes": 0}
        parts, kept, ns, ms, read_tours = [], [], [], [], []
        with torch.cuda.device(dev):
            st = _lib.current_stream()
            for c in G.read_files(paths, dev, text_bytes, times):
                t0 = _clock(dev)
                C = c.hi - c.lo
                ns.append(c.nc)
                ms.append(c.m)
                check_size(sum(int(m.sum()) for m in ms))
                e0, M = _prefix(c.m)
                v0, N = _prefix(c.nc)
                tab = np.ascontiguousarray(np.stack([c.nc, c.c_off, c.t_off, c.m, e0, v0, np.arange(C)], axis=1)
                                           .astype(np.int64))
                d_tab = D._to_device(tab, dev)
                d_uv = torch.empty((M, 2), dtype=torch.int32, device=dev)
                d_w = torch.empty(M, dtype=torch.float32, device=dev)
                d_eid = torch.empty(2 * M, dtype=torch.int32, device=dev)
                d_rowptr = torch.empty(N + C, dtype=torch.int32, device=dev)
                d_rc, d_fc, d_cyc = (torch.empty(C, dtype=torch.float64, device=dev) for _ in range(3))
                d_feas = torch.empty(C, dtype=torch.int32, device=dev)
                _lib.call("tspgnn_pack_dataset", tab.ctypes.data, _lib.ptr(d_tab), _lib.ptr(c.A), _lib.ptr(c.Mw),
                          _lib.ptr(c.tours), C, int(c.nc.max()), c.n_cells, c.n_verts, M, N + C, C,
                          _lib.ptr(d_uv) if M else None, _lib.ptr(d_w) if M else None, _lib.ptr(d_rowptr),
                          _lib.ptr(d_eid) if M else None, _lib.ptr(d_rc), _lib.ptr(d_fc), _lib.ptr(d_cyc), _lib.ptr(d_feas),
                          st)
                parts.append((d_uv, d_w, d_rowptr, d_eid, d_rc))
                if routes:
                    read_tours.append(c.tours)    # int32 [n_verts], the chunk's tours in file order
                if keep:
                    kept.append(_Kept(np.arange(c.lo, c.hi, dtype=np.int64), c.nc, c.c_off, c.t_off, c.n_cells, c.n_verts,
                                      c.A, c.Mw, c.tours))
                D._add_time(times, "pack", _clock(dev) - t0)
            n64 = np.concatenate(ns) if ns else np.zeros(0, dtype=np.int64)
            m64 = np.concatenate(ms) if ms else np.zeros(0, dtype=np.int64)
            I = len(n64)
            e0, M = _prefix(m64)
            v0, N = _prefix(n64)
            inst = np.stack([n64, m64, e0, v0], axis=1).astype(np.int32).reshape(I, 4)
            cat = lambda k, dtype, shape: (torch.cat([p[k] for p in parts]) if parts else
                                           torch.empty(shape, dtype=dtype, device=dev))
            ds = cls._adopt(dev, n64, m64, D._to_device(inst, dev), cat(0, torch.int32, (0, 2)), cat(1, torch.float32, 0),
                            cat(2, torch.int32, 0), cat(3, torch.int32, 0), cat(4, torch.float64, 0))
            if keep:
                tours = (np.concatenate([k.tours.cpu().numpy() for k in kept]) if kept else np.zeros(0, dtype=np.int32))
                ds.tours = (tours, np.concatenate([v0, [N]]).astype(np.int64))
                ds._matrices = kept
            if routes:
                flat = torch.cat(read_tours) if read_tours else torch.zeros(0, dtype=torch.int32, device=dev)
                ds._keep_routes(flat.cpu().numpy(), on_device=flat.to(torch.int32).contiguous())
        ds.read_times = times
        return ds

    # ------------------------------------------------------------------ made on the device
    @classmethod
    def generate(cls, samples, nmin, nmax, conn_min=1, conn_max=1, distances="euc_2D", metric=True, device=None,
                 exact=False, chunk_bytes=1 << 30, routes=False, **solve_kw):
        """The dataset DeviceDataset([(np.triu(Ma), Mw, tour)]) of draw_instances(nmin, nmax, conn_min, conn_max, samples,
        distances, metric) labelled by label_tours(init_tours=planted cycles, index=arange(samples), exact=exact,
        **solve_kw) -- byte for byte, the global ``random`` / ``np.random`` consumed exactly alike -- with only the 1-D
        random draws made on the host (dataset.draw_streams).  The matrices (tspgnn_build_instances), the metric closure
        of 'random' weights (tspgnn_metric_closure), the search input (tspgnn_penalise_instances), the labels (the tour
        kernels) and the dataset arrays (tspgnn_pack_dataset) are made on the GPU.

        4 <= nmin <= nmax <= 256.  solve_kw: restarts, kicks, lb_iters, seed, neighbors, max_nodes as label_tours takes
        them (None: its defaults for n <= 128 and for n 129-256).  exact: the branch and bound for n <= 128.  chunk_bytes:
        most bytes of fp64 matrices built and labelled together (the search input and the streams of a chunk are dropped
        after it; its mask and matrix stay on the device, 9 sum n^2 bytes in all); the result does not depend on it.
        Every argument is checked before the first launch (ValueError).

        Instance i is the i-th draw.  ``summary`` is create_dataset's dict: samples, n, cost, lb, target, feasible, gap,
        certified_fraction (at dev 0.02), with ``exact`` proved and nodes, and times {'draw', 'build', 'closure' when one
        ran, 'search', 'bound' | 'exact', 'pack'} in device-synchronised seconds plus 'total', the call's wall seconds.
        ``tours`` is (int32 host array of all tours, int64 offsets[samples + 1]).  The device array ``_cost`` is
        tspgnn_host_route_cost on Mw, as DeviceDataset(instances) keeps it; summary['target'] is n times that cost on the
        file form of Mw, as create_dataset reports it (they differ only when the closing pair (route[-1], route[1]) is no
        edge).  The fp64 weight matrices, the uint8 masks and the int32 tours of every chunk stay on the device (9 sum n^2 +
        4 sum n bytes) for to_instances() and write_directory().  routes=True: the labels also serve as the batches' route
        marks (see __init__): one more int32 copy of them in instance order, made after the summary's clock stops."""
        t_begin = time.perf_counter()
        cfg = _generate_settings(samples, nmin, nmax, distances, metric, device, exact, chunk_bytes, solve_kw)
        t0 = time.perf_counter()
        S = D.draw_streams(nmin, nmax, conn_min, conn_max, samples, distances)
        times = {"draw": time.perf_counter() - t0}
        ns = S["n"]
        D._check_chains_fit(cfg.large[0], int(ns[ns > D.MAX_N].max(initial=0)), cfg.neighbors)
        with torch.cuda.device(cfg.dev):
            st = _lib.current_stream()
            chunks = [_label_chunk(S, tri, pos, cfg, st, times) for tri, pos in _plan_chunks(ns, chunk_bytes)]
            t0 = _clock(cfg.dev)
            ds, file_cost, cyc, feas = cls._from_chunks(chunks, ns.astype(np.int64), cfg.dev, st)
            D._add_time(times, "pack", _clock(cfg.dev) - t0)
        if not feas.all():
            raise Exception("Unsolvable")
        summary = _summary(ds.n, chunks, file_cost, cyc, feas, exact, times)
        times["total"] = time.perf_counter() - t_begin
        ds.summary = summary
        if routes:
            ds._keep_routes(ds.tours[0])
        return ds

    @classmethod
    def _from_chunks(cls, chunks, n64, dev, st):
        """generate's last phase, once every chunk's edge counts are known: the dataset's prefix sums, then one
        tspgnn_pack_dataset launch per chunk into the final arrays.  -> (the dataset, with ``tours`` and the chunks' fp64
        matrices; then per instance: the route cost on the file form of Mw, the cycle cost, the tour's feasibility)."""
        I = len(n64)
        m = np.zeros(I, dtype=np.int64)
        for c in chunks:
            m[c.pos] = c.m
        check_size(m.sum())
        e0, M = _prefix(m)
        v0, N = _prefix(n64)
        inst = np.stack([n64, m, e0, v0], axis=1).astype(np.int32).reshape(I, 4)
        d_uv = torch.empty((M, 2), dtype=torch.int32, device=dev)
        d_w = torch.empty(M, dtype=torch.float32, device=dev)
        d_eid = torch.empty(2 * M, dtype=torch.int32, device=dev)
        d_rowptr = torch.empty(N + I, dtype=torch.int32, device=dev)
        d_rc, d_fc, d_cyc = (torch.empty(I, dtype=torch.float64, device=dev) for _ in range(3))
        d_feas = torch.empty(I, dtype=torch.int32, device=dev)
        tours = np.empty(N, dtype=np.int32)
        for c in chunks:
            tab = np.ascontiguousarray(np.stack([c.nc, c.c_off, c.t_off, m[c.pos], e0[c.pos], v0[c.pos], c.pos], axis=1))
            d_tab = D._to_device(tab, dev)
            _lib.call("tspgnn_pack_dataset", tab.ctypes.data, _lib.ptr(d_tab), _lib.ptr(c.A), _lib.ptr(c.Mw),
                      _lib.ptr(c.tours), len(c.pos), c.n_max, c.n_cells, c.n_verts, M, N + I, I, _lib.ptr(d_uv),
                      _lib.ptr(d_w), _lib.ptr(d_rowptr), _lib.ptr(d_eid), _lib.ptr(d_rc), _lib.ptr(d_fc), _lib.ptr(d_cyc),
                      _lib.ptr(d_feas), st)
            tours[np.arange(c.n_verts, dtype=np.int64) + np.repeat(v0[c.pos] - c.t_off, c.nc)] = c.tours.cpu().numpy()
        ds = cls._adopt(dev, n64, m, D._to_device(inst, dev), d_uv, d_w, d_rowptr, d_eid, d_rc)
        ds.tours = (tours, np.concatenate([v0, [N]]).astype(np.int64))
        ds._matrices = [_Kept(c.pos, c.nc, c.c_off, c.t_off, c.n_cells, c.n_verts, c.A, c.Mw, c.tours) for c in chunks]
        return ds, d_fc.cpu().numpy(), d_cyc.cpu().numpy(), d_feas.cpu().numpy().astype(bool)

    def to_instances(self):
        """A generated dataset as the list of (np.triu(Ma), Mw, route) DeviceDataset(...) and write_graph take, downloaded
        from the device: Ma from the edge list, Mw the fp64 matrices generate kept, route the label."""
        if self._matrices is None:
            raise RuntimeError("DeviceDataset.to_instances: only a dataset made by generate() keeps its fp64 matrices "
                               "(or read with reader='device', keep_matrices=True)")
        I = len(self.n)
        uv = self._uv.cpu().numpy()
        e0 = np.concatenate([[0], np.cumsum(self.m)])
        tours, t_off = self.tours
        Mw = [None] * I
        for kept in self._matrices:
            flat = kept.Mw.cpu().numpy()
            for p, o in zip(kept.pos, kept.c_off):
                n = int(self.n[p])
                Mw[p] = flat[o:o + n * n].reshape(n, n).copy()
        out = []
        for i in range(I):
            n = int(self.n[i])
            Ma = np.zeros((n, n))
            e = uv[e0[i]:e0[i + 1]]
            Ma[e[:, 0], e[:, 1]] = 1.0
            out.append((Ma, Mw[i], [int(x) for x in tours[t_off[i]:t_off[i + 1]]]))
        return out

    def write_directory(self, path, text_bytes=G.DEFAULT_TEXT_BYTES):
        """``{path}/{i}.graph`` for every instance i of a generated dataset, byte for byte the files write_graph(*inst,
        ...) writes over to_instances(), formatted on the GPU (csrc/graph_text.hip) from the masks, fp64 matrices and
        tours generate kept there.  Per chunk of at most ``text_bytes`` of text: the sizes launch (per generate chunk),
        the prefix sums on the host, the write launch, one download into a pinned buffer and one write per file; the
        result does not depend on text_bytes.  -> {'bytes': bytes written, 'times': {'format', 'download', 'files'
        seconds, and 'sizes' / 'write', the two launches 'format' is the sum of}}."""
        if self._matrices is None:
            raise RuntimeError("DeviceDataset.to_instances: only a dataset made by generate() keeps its fp64 matrices "
                               "(or read with reader='device', keep_matrices=True)")
        self._require_gpu()
        os.makedirs(path, exist_ok=True)
        times = {"sizes": 0.0, "write": 0.0, "format": 0.0, "download": 0.0, "files": 0.0}
        buffers, written = G._Buffers(self.device), 0
        for kept in self._matrices:
            written += G.write_files(path, [int(p) for p in kept.pos], kept.nc, kept.c_off, kept.t_off, kept.n_cells,
                                     kept.n_verts, kept.A, kept.Mw, kept.tours, self.device, text_bytes, times, buffers)
        return {"bytes": written, "times": times}

    def _require_gpu(self):
        if self.device.type != "cuda":
            raise RuntimeError("DeviceDataset(device=%r) is plumbing only: a batch is assembled by a HIP kernel and needs "
                               "an MI355X" % str(self.device))

    # ------------------------------------------------------------------ the launch
    def _small(self, idx, e_start, v_start):
        """ids, e_start, v_start as one pinned buffer and its (asynchronous) device copy: three int32 device views.  A
        ring of buffers that grow to the largest batch seen: pinning is the expensive part, and a slot is reused only once
        the launch that read it has run."""
        B = idx.size
        k = self._next
        self._next = (k + 1) % _RING
        slot = self._ring[k]
        if slot is not None and slot[2] is not None:
            slot[2].synchronize()
        if slot is None or slot[0].numel() < 3 * B + 2:
            cap = max(3 * B + 2, 1024)
            slot = self._ring[k] = [torch.empty(cap, dtype=torch.int32).pin_memory(),
                                    torch.empty(cap, dtype=torch.int32, device=self.device), None]
        pinned, dev = slot[0][:3 * B + 2], slot[1][:3 * B + 2]
        host = pinned.numpy()
        host[:B], host[B:2 * B + 1], host[2 * B + 1:] = idx, e_start, v_start
        dev.copy_(pinned, non_blocking=True)
        return slot, dev[:B], dev[B:2 * B + 1], dev[2 * B + 1:]

    def gather(self, indices, dev, target_cost, buf, offsets):
        """tspgnn_gather_batch of the instance list ``indices`` into the uint8 device tensor ``buf`` at the byte offsets
        ``offsets`` (parallel.stage_layout), on the current stream.  -> plan_batch(indices).  Writes the seven arrays and
        nothing else.  A batch without edges launches nothing: it is all offsets, filled from the host."""
        self._require_gpu()
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        plan = plan_batch(self.n, self.m, idx)
        e_start, v_start, M, N, _ = plan
        B = idx.size
        if buf.device != self.device or buf.dtype != torch.uint8 or not buf.is_contiguous():
            raise ValueError("DeviceDataset.gather: the destination is a contiguous uint8 tensor on %s" % self.device)
        sizes = stage_layout(M, N, B, 0)[1]
        if any(o < 0 or o + s > buf.numel() for o, s in zip(offsets[:7], sizes[:7])):
            raise ValueError("DeviceDataset.gather: the destination is too small for %d edges / %d vertices / %d graphs"
                             % (M, N, B))
        if B == 0:
            return plan
        if M == 0:   # all offsets, no edge anywhere: row pointers, segment offsets and edge counts are zeros
            part = lambda k, dtype: buf[offsets[k]:offsets[k] + sizes[k]].view(dtype)
            for k in (2, 5, 6):
                part(k, torch.int32).zero_()
            part(4, torch.float32).copy_(torch.arange(B, device=self.device) % 2)
            return plan
        slot, ids_d, es_d, vs_d = self._small(idx.astype(np.int32), e_start, v_start)
        off = (ctypes.c_longlong * 7)(*[int(o) for o in offsets[:7]])
        _lib.call("tspgnn_gather_batch", _lib.ptr(self._inst), _lib.ptr(self._uv), _lib.ptr(self._w), _lib.ptr(self._rowptr),
                  _lib.ptr(self._eid), _lib.ptr(self._cost), _lib.ptr(ids_d), _lib.ptr(es_d), _lib.ptr(vs_d), B, M, N,
                  float(dev), 0 if target_cost is None else 1, 0.0 if target_cost is None else float(target_cost),
                  buf.data_ptr(), off, _lib.current_stream())
        ev = torch.cuda.Event()
        ev.record()
        slot[2] = ev
        return plan

    # ------------------------------------------------------------------ batches
    def _plan_for(self, e_start, v_start, M):
        """The one-launch loop's work plan for a block structure, built once (device tensor, meta) or (None, None)."""
        from .graphnn import device_loop_plan, loop_enabled
        if not loop_enabled() or M == 0:
            return None, None
        key = (e_start.tobytes(), v_start.tobytes())
        if key not in self._plans:
            built = device_loop_plan(e_start.astype(np.int64), v_start.astype(np.int64), self.device)
            if len(self._plans) >= _PLAN_CACHE:
                self._plans.clear()
            self._plans[key] = (None, None) if built is None else (torch.from_numpy(built[0]).to(self.device), built[1])
        return self._plans[key]

    def batch(self, indices, dev=0.02, target_cost=None, time_steps=32, out=None):
        """-> DeviceBatch of the instance list ``indices`` (labels 0, 1, 0, 1, ...; target cost (1 -/+ dev) * tour cost, or
        ``target_cost``), as Session.prepare(feed of create_batch) makes it, plus the host arrays ``route_exists``,
        ``n_vertices``, ``n_edges`` (int64).  ``out``: a batch this dataset returned earlier for index lists of the same
        shape (the same instance sizes in the same order): the kernel writes into THAT batch's buffer, so a graph captured
        on it serves the new batch; ValueError when the shapes differ."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        e_start, v_start, M, N, labels = plan_batch(self.n, self.m, idx)
        B = idx.size
        if out is not None:
            if getattr(out, "_dataset", None) is not self:
                raise ValueError("DeviceDataset.batch: out= takes a batch this dataset returned")
            if not (np.array_equal(out._blocks[0], e_start) and np.array_equal(out._blocks[1], v_start)):
                raise ValueError("DeviceDataset.batch: the instance sizes of the index list differ from those of out=")
            b = out
        else:
            self._require_gpu()
            plan, meta = self._plan_for(e_start, v_start, M)
            offsets, nbytes, total = stage_layout(M, N, B, 0 if plan is None else plan.numel())
            buf = torch.empty(total, dtype=torch.uint8, device=self.device)
            b = staged_batch(buf, offsets, nbytes, M, N, B, meta)
            if plan is not None:
                b.adj.loop_plan[0].copy_(plan, non_blocking=True)
            b._dataset, b._buf, b._offsets, b._blocks = self, buf, offsets, (e_start, v_start)
        self.gather(idx, dev, target_cost, b._buf, b._offsets)
        b.T = int(time_steps)
        b.route_exists, b.n_vertices, b.n_edges = labels, self.n[idx], self.m[idx]
        if self._routes is not None and B:
            # one more launch: the marks of the instances' tours, into the batch's own route_edges (under out=: in place)
            from .route_head import launch_marks
            tour_off = torch.from_numpy(self._route_v0[idx]).to(self.device)
            launch_marks(b, self._routes, tour_off)
        return b

    def get_batches(self, batch_size, dev, time_steps, shuffle=True, rng=None):
        """One epoch, as InstanceLoader.get_batches: len(self) // batch_size batches of 2 * batch_size graphs, every
        instance twice in a row; the order is drawn per call (epoch_indices)."""
        for idx in epoch_indices(len(self), batch_size, shuffle, rng):
            yield self.batch(idx, dev=dev, time_steps=time_steps)
