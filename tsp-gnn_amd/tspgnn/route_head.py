"""The route head's supervision: which edges of a batch lie on the instances' labelled tours.

``build_network(d, route_head=True)`` adds a second per-edge head, ``E_route``, trained with a sigmoid cross entropy against
the marks "this edge lies on the labelled tour" (Session.loss_and_grads).  The marks of a batch come from

* ``route_edge_marks_host(instances)``: NumPy, in create_batch's edge order -- the feed of ``model['route_edges']`` for a
  create_batch 6-tuple, and what the kernel is tested against;
* ``mark_routes(batch, tours)`` / ``Session.mark_routes``: tspgnn_route_edge_marks (csrc/route_head.hip) on a resident
  DeviceBatch, which is what ``DeviceDataset(..., routes=True).batch`` launches.

The tour is the true cycle: the pairs (tour[k], tour[k+1]) and the closing pair (tour[n-1], tour[0]) -- not the
(route[-1], route[1]) of the reference's cost sum (instance_loader.route_cost).
"""
import numpy as np
import torch

from . import _lib

MIN_N, MAX_N = 3, 16384    # tspgnn_route_edge_marks: an int32 position table in LDS


def check_tour(k, tour, n):
    """The tour of instance ``k`` as an int64 array, once it is a permutation of 0 .. n-1 (ValueError naming k otherwise)."""
    t = np.asarray(tour, dtype=np.int64).reshape(-1)
    if t.shape[0] != n or not np.array_equal(np.sort(t), np.arange(n)):
        raise ValueError("route marks: the tour of instance %d is not a permutation of its %d vertices" % (k, n))
    return t


def route_edge_marks_host(instances):
    """(marks float32[M], n_missing int64[B]) of a list of (Ma, Mw, route): marks in create_batch's edge order
    (np.nonzero(Ma) per instance, instances concatenated), 1.0 where the edge's endpoints are cyclically consecutive in the
    route, the closing pair included; n_missing[b] the route's pairs that are no edge of the graph.  ValueError for a route
    that is no permutation of the instance's vertices, or an instance of fewer than three."""
    marks, missing = [], []
    for k, (Ma, _, route) in enumerate(instances):
        Ma = np.asarray(Ma)
        n = Ma.shape[0]
        if n < MIN_N:
            raise ValueError("route marks: instance %d has %d vertices; a tour takes at least %d" % (k, n, MIN_N))
        t = check_tour(k, route, n)
        pos = np.empty(n, dtype=np.int64)
        pos[t] = np.arange(n)
        u, v = np.nonzero(Ma)
        dist = np.abs(pos[u] - pos[v])
        on = ((dist == 1) | (dist == n - 1)) & (u != v)
        # the pair an edge joins: k = the smaller position, the closing pair k = n - 1 (n >= 3: never both)
        pair = np.where(dist == 1, np.minimum(pos[u], pos[v]), n - 1)[on]
        marks.append(on.astype(np.float32))
        missing.append(n - np.unique(pair).size)
    flat = np.concatenate(marks) if marks else np.zeros(0, dtype=np.float32)
    return flat, np.asarray(missing, dtype=np.int64)


def _vseg(batch):
    """(device int32 vertex prefix sums, largest n) of a batch that carries its host n_vertices; remembered on the batch."""
    nv = getattr(batch, "n_vertices", None)
    if nv is None:
        raise ValueError("mark_routes: this batch does not carry n_vertices")
    nv = np.asarray(nv, dtype=np.int64).reshape(-1)
    cached = getattr(batch, "_route_vseg", None)
    if cached is not None and np.array_equal(cached[0], nv):
        return cached[1], cached[2]
    if nv.size and (nv.min() < MIN_N or nv.max() > MAX_N):
        raise ValueError("mark_routes: instances of %d..%d vertices; the marks take %d <= n <= %d"
                         % (nv.min(), nv.max(), MIN_N, MAX_N))
    vseg = torch.from_numpy(np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)).to(batch.seg.device)
    batch._route_vseg = (nv.copy(), vseg, int(nv.max()) if nv.size else MIN_N)
    return vseg, batch._route_vseg[2]


def launch_marks(batch, tours, tour_off=None):
    """tspgnn_route_edge_marks on the current stream: ``tours`` an int32 device tensor of local vertex ids, problem p's at
    ``tour_off[p]`` (int32 device tensor) or, without offsets, at the batch's vertex offset.  Writes ``batch.route_edges``
    (float32 [M], made on first use and refilled in place afterwards: a captured graph keeps reading it) and returns the
    device tensors (n_missing, status).  Nothing here waits for the device."""
    vseg, n_max = _vseg(batch)
    dev = batch.seg.device
    marks = getattr(batch, "route_edges", None)
    if marks is None or marks.numel() != batch.M:
        marks = batch.route_edges = torch.empty(batch.M, dtype=torch.float32, device=dev)
    n_missing = torch.empty(batch.B, dtype=torch.int32, device=dev)
    status = torch.empty(batch.B, dtype=torch.int32, device=dev)
    if batch.B == 0:
        return n_missing, status
    uv = batch.adj.uv if batch.M else batch.adj.uv.new_zeros((1, 2))
    out = marks if batch.M else marks.new_zeros(1)
    with torch.cuda.device(dev):
        _lib.call("tspgnn_route_edge_marks", _lib.ptr(uv), _lib.ptr(batch.seg), _lib.ptr(vseg), _lib.ptr(tours),
                  _lib.ptr(tour_off), batch.B, n_max, _lib.ptr(out), _lib.ptr(n_missing), _lib.ptr(status),
                  _lib.current_stream())
    return n_missing, status


def mark_routes(batch, tours):
    """Session.mark_routes: the marks of a resident batch from its instances' tours.  ``tours``: one sequence of local
    vertex ids per instance, or (int32 array of all of them, offsets[B + 1]).  Sets ``batch.route_edges``; returns n_missing
    (int64 host array).  ValueError, naming the instance, for a tour that is no permutation of its instance's vertices:
    checked on the host before the launch, and read back from the kernel's status words after it."""
    nv = np.asarray(batch.n_vertices, dtype=np.int64).reshape(-1)
    if isinstance(tours, tuple):     # (a tuple is always the (array, offsets) form; a list holds one sequence per instance)
        if len(tours) != 2 or len(tours[1]) != len(nv) + 1:
            raise ValueError("mark_routes: tours as a tuple is (int32 array, offsets[%d])" % (len(nv) + 1))
        flat, off = np.asarray(tours[0]).reshape(-1), np.asarray(tours[1], dtype=np.int64).reshape(-1)
        tours = [flat[off[k]:off[k + 1]] for k in range(len(nv))]
    tours = list(tours)
    if len(tours) != len(nv):
        raise ValueError("mark_routes: %d tours for a batch of %d instances" % (len(tours), len(nv)))
    checked = [check_tour(k, t, int(nv[k])) for k, t in enumerate(tours)]
    flat = np.concatenate(checked).astype(np.int32) if checked else np.zeros(0, dtype=np.int32)
    dev = batch.seg.device
    d_tours = torch.from_numpy(flat).to(dev) if flat.size else torch.zeros(1, dtype=torch.int32, device=dev)
    n_missing, status = launch_marks(batch, d_tours)
    status = status.cpu().numpy()
    if status.any():
        k = int(np.nonzero(status)[0][0])
        raise ValueError("mark_routes: the tour of instance %d is not a permutation of its %d vertices (status %d)"
                         % (k, int(nv[k]), int(status[k])))
    return n_missing.cpu().numpy().astype(np.int64)


def edge_bce(logits, marks, seg, B, pos_weight, scale, want_grad):
    """tspgnn_edge_bce_f32 on the current stream -> (dlogit or None, stats float32[6]): see include/tspgnn.h."""
    dev = logits.device
    dlogit = torch.empty_like(logits) if want_grad else None
    stats = torch.empty(6, dtype=torch.float32, device=dev)
    ws = _lib.workspace("tspgnn_edge_bce_workspace_floats", B, device=dev)
    _lib.call("tspgnn_edge_bce_f32", _lib.ptr(logits), _lib.ptr(marks), _lib.ptr(seg), B, float(pos_weight), float(scale),
              _lib.ptr(dlogit), _lib.ptr(stats), _lib.ptr(ws), _lib.current_stream())
    return dlogit, stats
