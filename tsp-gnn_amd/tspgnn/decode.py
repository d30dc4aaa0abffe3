"""Tours from the network's edge votes.

The network answers "is there a tour of cost at most C?"; it never produces a route.  Yet one logit per edge is exactly
what it computes -- ``E_vote`` of the reference's model.py:106-128, which the reference only averages, and which its
figures/route-examples.png draws over the optimal route.  ``tspgnn_tour_from_votes`` (csrc/tour_decode.hip) turns the votes
of a resident batch into one tour per instance on the device: the edges in descending vote order, each taken when both
endpoints still have degree < 2 and lie in different fragments, the fragments stitched by vertex id, the tour written in
the canonical form of ``TourResult``.  include/tspgnn.h states the process in full; tests/decode_reference.py restates
it in NumPy.

``tours_from_votes`` is the launch alone, ``decode_tours`` the pipeline from instances to records, with the network's own
cost estimate (``get_costs``) as the target when none is given and an optional descent of the existing tour search from
the decoded tour (``polish=True``).  How good the decoded tours are is an observation, not a guarantee.
"""
import collections

import numpy as np
import torch

from . import _lib
from .binary_search import DEFAULT_MAX_GRAPHS, get_costs, plan_chunks
from .instance_loader import InstanceLoader

MIN_N = 4      # tspgnn_tour_from_votes: 4 <= n <= 256
MAX_N = 256

DecodedBatch = collections.namedtuple("DecodedBatch", ["tours", "costs", "n_missing", "vseg"])
DecodedBatch.__doc__ = """tours_from_votes' device tensors: tours int32 [N] (instance b at vseg[b], local vertex ids,
canonical form), costs float32 [B], n_missing int32 [B], vseg int32 [B+1] (the vertex prefix sums)."""

DecodedTour = collections.namedtuple("DecodedTour", ["tour", "cost", "n_missing", "feasible", "prediction", "target_cost",
                                                     "polished_tour", "polished_cost"])
DecodedTour.__doc__ = """One decoded instance.
tour: list of vertex ids, canonical (starts at 0, tour[1] < tour[-1]); cost: the kernel's fp32 sum of the weights of the
tour's pairs that are edges, unnormalised; n_missing: the pairs that are not edges; feasible: n_missing == 0;
prediction: the network's answer at target_cost; target_cost: the per-vertex target the instance was packed at (the unit
get_costs returns); polished_tour / polished_cost: label_tours' tour and fp64 cost from the decoded tour (None without
polish=True)."""


def vote_key(votes):
    """The key the decoder orders edges by, as a uint32 array: 0 for a NaN vote, otherwise the order-preserving image of
    the fp32 bits (all bits flipped when the sign bit is set, else the sign bit set).  Larger key first; -0.0 < +0.0, -inf
    is the lowest number and NaN lies below everything."""
    bits = np.ascontiguousarray(votes, dtype=np.float32).view(np.uint32)
    key = np.where((bits & np.uint32(0x80000000)) != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    key[(bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = 0
    return key


def _vseg(batch, n_vertices):
    """(device prefix sums of n_vertices, largest n), remembered on the batch: the upload then happens once, ahead of the
    forward whose votes the launch will read."""
    if n_vertices is None:
        n_vertices = getattr(batch, "n_vertices", None)
        if n_vertices is None:
            raise ValueError("tours_from_votes: this batch does not carry n_vertices; pass it")
    nv = np.asarray(n_vertices, dtype=np.int64).reshape(-1)
    if nv.shape[0] != batch.B or int(nv.sum()) != batch.N:
        raise ValueError("tours_from_votes: n_vertices must hold one entry per graph and sum to the batch's %d vertices"
                         % batch.N)
    if nv.size and (nv.min() < MIN_N or nv.max() > MAX_N):
        raise ValueError("tours_from_votes: instances of %d..%d vertices; the decoder takes %d <= n <= %d"
                         % (nv.min(), nv.max(), MIN_N, MAX_N))
    cached = getattr(batch, "_decode_vseg", None)
    if cached is not None and np.array_equal(cached[0], nv):
        return cached[1], cached[2]
    dev = batch.seg.device
    vseg = torch.from_numpy(np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)).to(dev)
    batch._decode_vseg = (nv.copy(), vseg, int(nv.max()) if nv.size else MIN_N)
    return vseg, batch._decode_vseg[2]


def tours_from_votes(batch, votes, n_vertices=None):
    """tspgnn_tour_from_votes on a resident batch (Session.prepare / DeviceDataset.batch) and its vote tensor
    (``forward_device(batch)["E_vote"]``, float32 [M] on the batch's device), on the current stream.  -> DecodedBatch of
    device tensors.  n_vertices: the batch's own when it carries them.  Nothing here waits for the device, so the launch
    may follow forward_device directly; only the first call on a batch uploads the B + 1 vertex prefix sums."""
    if not torch.is_tensor(votes) or votes.dtype != torch.float32 or votes.device != batch.seg.device:
        raise ValueError("tours_from_votes: votes must be a float32 tensor on the batch's device")
    votes = votes.reshape(-1)
    if votes.numel() != batch.M or not votes.is_contiguous():
        raise ValueError("tours_from_votes: one contiguous vote per edge (%d), got %d" % (batch.M, votes.numel()))
    vseg, n_max = _vseg(batch, n_vertices)
    dev = batch.seg.device
    tours = torch.empty(batch.N, dtype=torch.int32, device=dev)
    costs = torch.empty(batch.B, dtype=torch.float32, device=dev)
    n_missing = torch.empty(batch.B, dtype=torch.int32, device=dev)
    uv, wc = batch.adj.uv, batch.WC
    if batch.M == 0:   # no edge anywhere: the kernel reads none of the three, but refuses null pointers
        votes = torch.zeros(1, dtype=torch.float32, device=dev)
        uv = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        wc = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("tspgnn_tour_from_votes", _lib.ptr(votes), _lib.ptr(uv), _lib.ptr(wc), _lib.ptr(batch.seg),
                  _lib.ptr(vseg), batch.B, n_max, _lib.ptr(tours), _lib.ptr(costs), _lib.ptr(n_missing),
                  _lib.current_stream())
    return DecodedBatch(tours, costs, n_missing, vseg)


def _decode_chunk(sess, model, chunk, targets, time_steps):
    """[(tour, cost, n_missing, prediction)] of one batch: pack at the targets, forward, decode, one read-back."""
    EV, W, C, route_exists, n_vertices, n_edges = InstanceLoader.create_batch(chunk, target_cost=0.0)
    C[:, 0] = np.repeat(np.asarray(targets, dtype=np.float64), n_edges)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: time_steps,
            model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    b = sess.prepare(feed, remember_adjacency=False)
    _vseg(b, n_vertices)   # uploaded before the forward is enqueued

    def run():
        out = sess.forward_device(b)
        return tours_from_votes(b, out["E_vote"], n_vertices), out["predictions"]

    dec, pred = sess._on_bf16x3_if_flagged(run)   # (one synchronising look at the f16x2 range guard)
    tours, costs = dec.tours.cpu().numpy(), dec.costs.cpu().numpy()
    missing, pred = dec.n_missing.cpu().numpy(), pred.cpu().numpy()
    v0 = np.concatenate([[0], np.cumsum(n_vertices)])
    return [([int(v) for v in tours[v0[i]:v0[i + 1]]], float(costs[i]), int(missing[i]), float(pred[i]))
            for i in range(len(chunk))]


def decode_tours(sess, model, instances, time_steps, target_costs=None, polish=False, max_graphs=None, **search_kw):
    """A tour per instance from the network's edge votes.

    instances: list of (Ma, Mw, route) as for get_costs (4 <= n <= 256; the route is not used by the decoder).
    target_costs: one per-vertex target cost per instance, the unit get_costs returns; None runs get_costs first and
    decodes at the network's own estimate, so the whole pipeline needs no label.  The instances are packed at their
    targets in chunks of at most ``max_graphs`` graphs (plan_chunks, default DEFAULT_MAX_GRAPHS), each one forward and one
    tspgnn_tour_from_votes launch.
    polish=True hands the decoded tours to the tour search as its starting tours (label_tours with restarts=1, kicks=0,
    lower_bound=False: one descent from the network's tour on the penalised weights, which repairs an infeasible stitch
    where the graph allows); ``search_kw`` go to label_tours and may raise the restart and kick counts.
    Returns a list of DecodedTour in input order."""
    sess._require_gpu("decode_tours")
    instances = list(instances)
    for k, inst in enumerate(instances):
        n = np.asarray(inst[0]).shape[0]
        if not MIN_N <= n <= MAX_N:
            raise ValueError("decode_tours: instance %d has %d vertices; the decoder takes %d <= n <= %d"
                             % (k, n, MIN_N, MAX_N))
    if search_kw and not polish:
        raise TypeError("decode_tours: %s only apply with polish=True" % ", ".join(sorted(search_kw)))
    if target_costs is None:
        targets = [r[0] for r in get_costs(sess, model, instances, time_steps, max_graphs=max_graphs)]
    else:
        targets = [float(c) for c in np.asarray(target_costs, dtype=np.float64).reshape(-1)]
        if len(targets) != len(instances):
            raise ValueError("decode_tours: target_costs must hold one cost per instance")
    rows = []
    for start, stop in plan_chunks(len(instances), 1, DEFAULT_MAX_GRAPHS if max_graphs is None else max_graphs):
        rows += _decode_chunk(sess, model, instances[start:stop], targets[start:stop], time_steps)
    polished = [(None, None)] * len(instances)
    if polish and instances:
        from .dataset import label_tours
        kw = dict(restarts=1, kicks=0, lower_bound=False)
        kw.update(search_kw)
        res = label_tours([(x[0], x[1]) for x in instances], init_tours=[r[0] for r in rows], device=sess.device, **kw)
        polished = [(r.tour, r.cost) for r in res]
    return [DecodedTour(tour, cost, missing, missing == 0, pred, target, p[0], p[1])
            for (tour, cost, missing, pred), target, p in zip(rows, targets, polished)]
