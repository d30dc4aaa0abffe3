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

``decode_tours(..., beam=K)`` decodes by beam search instead: ``edge_scores`` turns the votes into integer
log-probabilities (tspgnn_vote_scores_i32), ``beam_tours`` keeps the K best partial paths from vertex 0 under their sum
(tspgnn_tour_beam, csrc/tour_beam.hip) and returns the best-scoring closed tour of the last list, or with
``select="cost"`` the cheapest.  tests/beam_reference.py restates it in NumPy.

``vote_neighbors`` turns the same votes into per-vertex candidate rows (tspgnn_vote_neighbors, csrc/tour_guided.hip): the
k_vote neighbours the network ranks highest, then the k_near nearest of the rest.  ``decode_tours(..., polish=True,
guide=K | (k_vote, k_near))`` hands those rows to the polish, whose descent then adds only edges the rows name
(label_tours(candidates=), tspgnn_tour_search_cand).  tests/guided_reference.py restates the rows in NumPy.
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

MAX_GUIDE = 32                                # tspgnn_vote_neighbors: 1 <= k_vote + k_near <= 32
MAX_BEAM = 1024                               # tspgnn_tour_beam: 1 <= beam <= 1024
SELECT = {"score": 0, "cost": 1}
DEFAULT_BEAM_WORKSPACE_BYTES = 256 << 20      # beam_tours splits a batch into launches whose workspace stays below this

BeamBatch = collections.namedtuple("BeamBatch", ["tours", "costs", "n_missing", "scores", "n_closed", "vseg"])
BeamBatch.__doc__ = """beam_tours' device tensors: tours, costs, n_missing and vseg as DecodedBatch; scores int32 [B], the
integer score of the chosen entry; n_closed int32 [B], the entries of the last list that an edge closes (0: stranded)."""

BeamTour = collections.namedtuple("BeamTour", DecodedTour._fields + ("score", "n_closed"))
BeamTour.__doc__ = """One instance decoded by beam search: the fields of DecodedTour, then score: the tour's integer score
(65536 x the sum of its edges' log-probabilities, each rounded and clamped to [-2^22, 0]); n_closed: how many entries of
the final list an edge closes (0: the search stranded and the tour was filled up by vertex id)."""


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


_PER_EDGE = {torch.float32: ("vote", "a float32"), torch.int32: ("score", "an int32")}


def _per_edge(who, batch, values, dtype):
    """The votes (float32) or scores (int32) of a launch, flat: a tensor of ``dtype`` on the batch's device, one
    contiguous value per edge."""
    word, kind = _PER_EDGE[dtype]
    if not torch.is_tensor(values) or values.dtype != dtype or values.device != batch.seg.device:
        raise ValueError("%s: %ss must be %s tensor on the batch's device" % (who, word, kind))
    values = values.reshape(-1)
    if values.numel() != batch.M or not values.is_contiguous():
        raise ValueError("%s: one contiguous %s per edge (%d), got %d" % (who, word, batch.M, values.numel()))
    return values


def _edge_inputs(batch, values, csr=False):
    """(values, uv, wc[, eid]) as a launch takes them.  Without an edge anywhere the kernel reads none of them but refuses
    null pointers: each is then a placeholder of one row."""
    inputs = (values, batch.adj.uv, batch.WC) + ((batch.adj.csr_t[1],) if csr else ())
    if batch.M == 0:
        inputs = tuple(t.new_zeros((1,) + tuple(t.shape[1:])) for t in inputs)
    return inputs


def tours_from_votes(batch, votes, n_vertices=None):
    """tspgnn_tour_from_votes on a resident batch (Session.prepare / DeviceDataset.batch) and its vote tensor
    (``forward_device(batch)["E_vote"]``, float32 [M] on the batch's device), on the current stream.  -> DecodedBatch of
    device tensors.  n_vertices: the batch's own when it carries them.  Nothing here waits for the device, so the launch
    may follow forward_device directly; only the first call on a batch uploads the B + 1 vertex prefix sums."""
    votes = _per_edge("tours_from_votes", batch, votes, torch.float32)
    vseg, n_max = _vseg(batch, n_vertices)
    dev = batch.seg.device
    tours = torch.empty(batch.N, dtype=torch.int32, device=dev)
    costs = torch.empty(batch.B, dtype=torch.float32, device=dev)
    n_missing = torch.empty(batch.B, dtype=torch.int32, device=dev)
    votes, uv, wc = _edge_inputs(batch, votes)
    with torch.cuda.device(dev):
        _lib.call("tspgnn_tour_from_votes", _lib.ptr(votes), _lib.ptr(uv), _lib.ptr(wc), _lib.ptr(batch.seg),
                  _lib.ptr(vseg), batch.B, n_max, _lib.ptr(tours), _lib.ptr(costs), _lib.ptr(n_missing),
                  _lib.current_stream())
    return DecodedBatch(tours, costs, n_missing, vseg)


def _guide_counts(guide, what):
    """guide=K | (k_vote, k_near) -> (k_vote, k_near), checked against tspgnn_vote_neighbors' limits."""
    pair = (guide, 0) if isinstance(guide, (int, np.integer)) and not isinstance(guide, bool) else guide
    try:
        k_vote, k_near = pair
        ok = all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in (k_vote, k_near))
    except (TypeError, ValueError):
        ok = False
    if not ok or k_vote < 0 or k_near < 0 or not 1 <= k_vote + k_near <= MAX_GUIDE:
        raise ValueError("%s: %r; the rows take k_vote >= 0 and k_near >= 0 with 1 <= k_vote + k_near <= %d"
                         % (what, guide, MAX_GUIDE))
    return int(k_vote), int(k_near)


def vote_neighbors(batch, votes, k_vote, k_near=0, n_vertices=None):
    """tspgnn_vote_neighbors on a resident batch and its vote tensor, as tours_from_votes takes them, on the current
    stream -> a uint8 device tensor [N, k_vote + k_near]: row vseg[b] + x holds, for local vertex x of instance b, the
    k_vote neighbours of highest vote (ties to the smaller id), then the k_near nearest by weight among the rest, in local
    ids; a vertex with fewer neighbours pads its row with x itself, which the search ignores.  include/tspgnn.h states the
    process in full.  The batch must carry its vertex CSR (``batch.adj.csr_t``, as every prepared batch does).  Nothing
    here waits for the device, so the launch may follow forward_device directly."""
    k_vote, k_near = _guide_counts((k_vote, k_near), "vote_neighbors: k_vote, k_near")
    votes = _per_edge("vote_neighbors", batch, votes, torch.float32)
    vseg, n_max = _vseg(batch, n_vertices)
    dev = batch.seg.device
    tab = torch.empty((batch.N, k_vote + k_near), dtype=torch.uint8, device=dev)
    votes, uv, wc, eid = _edge_inputs(batch, votes, csr=True)
    with torch.cuda.device(dev):
        _lib.call("tspgnn_vote_neighbors", _lib.ptr(votes), _lib.ptr(uv), _lib.ptr(wc), _lib.ptr(batch.seg),
                  _lib.ptr(vseg), _lib.ptr(batch.adj.csr_t[0]), _lib.ptr(eid), batch.B, n_max, k_vote, k_near,
                  _lib.ptr(tab), _lib.current_stream())
    return tab


def edge_scores(votes):
    """tspgnn_vote_scores_i32 on a float32 device tensor of votes, on the current stream: q(v) = clamp(rint(65536
    logsigmoid(v)), -2^22, 0) -> int32 tensor of the same length (NaN -> -2^22).  Does not wait for the device."""
    if not torch.is_tensor(votes) or votes.dtype != torch.float32 or not votes.is_cuda:
        raise ValueError("edge_scores: votes must be a float32 tensor on a GPU")
    votes = votes.reshape(-1)
    if not votes.is_contiguous():
        raise ValueError("edge_scores: the votes must be contiguous")
    scores = torch.empty(votes.numel(), dtype=torch.int32, device=votes.device)
    with torch.cuda.device(votes.device):
        _lib.call("tspgnn_vote_scores_i32", _lib.ptr(votes), votes.numel(), _lib.ptr(scores), _lib.current_stream())
    return scores


def beam_ranges(B, n_max, beam, workspace_bytes=None):
    """The instance ranges [(start, stop)] beam_tours launches one after the other, and the bytes of workspace they share:
    as many instances per launch as tspgnn_tour_beam_workspace_bytes allows under the cap (at least one)."""
    cap = DEFAULT_BEAM_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    per = int(_lib.lib.tspgnn_tour_beam_workspace_bytes(1, n_max, beam))
    if per <= 0:
        raise ValueError("beam_tours: no workspace for n_max=%d, beam=%d" % (n_max, beam))
    g = max(1, min(B, cap // per))
    return [(s, min(s + g, B)) for s in range(0, B, g)], int(_lib.lib.tspgnn_tour_beam_workspace_bytes(g, n_max, beam))


def _beam_width(who, beam, select, shown="%d"):
    """beam as the int tspgnn_tour_beam takes, once select and its range are checked.  shown: how a refusal prints the
    width, "%d" (the int) or "%r" (the caller's value)."""
    if select not in SELECT:
        raise ValueError("%s: select must be 'score' or 'cost', got %r" % (who, select))
    width = int(beam)
    if not 1 <= width <= MAX_BEAM:
        raise ValueError("%s: beam=%s; the decoder takes 1 <= beam <= %d"
                         % (who, shown % (width if shown == "%d" else beam,), MAX_BEAM))
    return width


def beam_tours(batch, scores, beam, select="score", n_vertices=None, workspace_bytes=None):
    """tspgnn_tour_beam on a resident batch and its integer edge scores (``edge_scores(forward_device(batch)["E_vote"])``,
    int32 [M] on the batch's device), on the current stream -> BeamBatch of device tensors.  beam: 1 .. 1024; select:
    "score" or "cost".  Nothing here waits for the device, so the launch may follow forward_device and edge_scores
    directly.  The workspace is sized by the library's query; when a batch would need more than ``workspace_bytes``
    (default DEFAULT_BEAM_WORKSPACE_BYTES, 256 MiB) it is decoded in several launches over instance ranges that share one
    workspace -- instances are independent, so the ranges change nothing."""
    beam = _beam_width("beam_tours", beam, select)
    scores = _per_edge("beam_tours", batch, scores, torch.int32)
    vseg, n_max = _vseg(batch, n_vertices)
    dev = batch.seg.device
    tours = torch.empty(batch.N, dtype=torch.int32, device=dev)
    costs = torch.empty(batch.B, dtype=torch.float32, device=dev)
    n_missing, out_scores, n_closed = (torch.empty(batch.B, dtype=torch.int32, device=dev) for _ in range(3))
    scores, uv, wc = _edge_inputs(batch, scores)
    if batch.B == 0:
        return BeamBatch(tours, costs, n_missing, out_scores, n_closed, vseg)
    ranges, ws_bytes = beam_ranges(batch.B, n_max, beam, workspace_bytes)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for start, stop in ranges:      # seg and vseg hold global offsets: a range is the same arrays from `start` on
            _lib.call("tspgnn_tour_beam", _lib.ptr(scores), _lib.ptr(uv), _lib.ptr(wc), _lib.ptr(batch.seg) + 4 * start,
                      _lib.ptr(vseg) + 4 * start, stop - start, n_max, beam, SELECT[select], _lib.ptr(ws), ws_bytes,
                      _lib.ptr(tours), _lib.ptr(costs) + 4 * start, _lib.ptr(n_missing) + 4 * start,
                      _lib.ptr(out_scores) + 4 * start, _lib.ptr(n_closed) + 4 * start, _lib.current_stream())
    return BeamBatch(tours, costs, n_missing, out_scores, n_closed, vseg)


_Decoded = collections.namedtuple("_Decoded", ["tour", "cost", "n_missing", "prediction", "score", "n_closed", "table"])


VOTE_SOURCES = {"decision": "E_vote", "route": "E_route"}   # decode_tours(votes=...): the forward output the decoders read


def _decode_chunk(sess, model, chunk, targets, time_steps, beam=None, select="score", workspace_bytes=None, guide=None,
                  votes="decision"):
    """One _Decoded per instance of one batch: pack at the targets, forward, decode, one read-back.  beam None: the
    greedy decoder, score and n_closed None.  guide = (k_vote, k_near): vote_neighbors follows the forward on the same
    stream and table is the instance's uint8 [n, K] rows; otherwise None.  votes: the key of VOTE_SOURCES."""
    key = VOTE_SOURCES[votes]
    EV, W, C, route_exists, n_vertices, n_edges = InstanceLoader.create_batch(chunk, target_cost=0.0)
    C[:, 0] = np.repeat(np.asarray(targets, dtype=np.float64), n_edges)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: time_steps,
            model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    b = sess.prepare(feed, remember_adjacency=False)
    _vseg(b, n_vertices)   # uploaded before the forward is enqueued

    def run():
        out = sess.forward_device(b)
        tab = None if guide is None else vote_neighbors(b, out[key], guide[0], guide[1], n_vertices)
        if beam is None:
            return tours_from_votes(b, out[key], n_vertices), out["predictions"], tab
        return (beam_tours(b, edge_scores(out[key]), beam, select, n_vertices, workspace_bytes), out["predictions"],
                tab)

    dec, pred, tab = sess._on_bf16x3_if_flagged(run)   # (one synchronising look at the f16x2 range guard)
    tours, costs = dec.tours.cpu().numpy(), dec.costs.cpu().numpy()
    missing, pred = dec.n_missing.cpu().numpy(), pred.cpu().numpy()
    v0 = np.concatenate([[0], np.cumsum(n_vertices)])
    scores = closed = tabs = [None] * len(chunk)
    if beam is not None:
        scores, closed = dec.scores.cpu().numpy().tolist(), dec.n_closed.cpu().numpy().tolist()
    if tab is not None:
        tab = tab.cpu().numpy()
        tabs = [tab[v0[i]:v0[i + 1]] for i in range(len(chunk))]
    return [_Decoded(tour=tours[v0[i]:v0[i + 1]].tolist(), cost=float(costs[i]), n_missing=int(missing[i]),
                     prediction=float(pred[i]), score=scores[i], n_closed=closed[i], table=tabs[i])
            for i in range(len(chunk))]


def decode_tours(sess, model, instances, time_steps, target_costs=None, polish=False, max_graphs=None, beam=None,
                 select="score", workspace_bytes=None, guide=None, votes="decision", **search_kw):
    """A tour per instance from the network's edge votes.

    instances: list of (Ma, Mw, route) as for get_costs (4 <= n <= 256; the route is not used by the decoder).
    target_costs: one per-vertex target cost per instance, the unit get_costs returns; None runs get_costs first and
    decodes at the network's own estimate, so the whole pipeline needs no label.  The instances are packed at their
    targets in chunks of at most ``max_graphs`` graphs (plan_chunks, default DEFAULT_MAX_GRAPHS), each one forward and one
    tspgnn_tour_from_votes launch.
    polish=True hands the decoded tours to the tour search as its starting tours (label_tours with restarts=1, kicks=0,
    lower_bound=False: one descent from the network's tour on the penalised weights, which repairs an infeasible stitch
    where the graph allows); ``search_kw`` go to label_tours and may raise the restart and kick counts.
    guide=K or (k_vote, k_near), with polish=True: the polish descends over candidate rows made from the votes --
    vote_neighbors per chunk behind the forward, the rows read back with the tours, label_tours(candidates=rows) -- so it
    may add only edges among a vertex's k_vote best-voted neighbours and the k_near nearest of the rest.  Exclusive with
    ``neighbors`` in search_kw.  The records are unchanged.
    beam=None decodes by greedy edge insertion (tspgnn_tour_from_votes).  beam=K, 1 .. 1024, decodes by beam search
    instead: edge_scores and beam_tours per chunk, ``select`` "score" (the best-scoring closed tour of the last list) or
    "cost" (its cheapest), ``workspace_bytes`` beam_tours' cap; the records are then BeamTour, DecodedTour's fields
    followed by score and n_closed.
    votes="decision" (the default) decodes from E_vote, the per-edge logits the decision averages; votes="route" from
    E_route, the head trained on the labelled tours' edges (build_network(d, route_head=True)) -- it selects what goes to
    tours_from_votes, edge_scores / beam_tours and vote_neighbors, and nothing else.
    Returns a list of DecodedTour (BeamTour with a beam) in input order."""
    if votes not in VOTE_SOURCES:
        raise ValueError("decode_tours: votes must be 'decision' or 'route', got %r" % (votes,))
    if votes == "route" and not getattr(model, "route_head", False):
        raise ValueError("decode_tours: votes='route' needs a network built with route_head=True")
    if guide is not None:
        if not polish:
            raise TypeError("decode_tours: guide only applies with polish=True")
        if search_kw.get("neighbors") is not None or search_kw.get("candidates") is not None:
            raise ValueError("decode_tours: guide and neighbors / candidates are exclusive: the polish descends over "
                             "one candidate table")
        guide = _guide_counts(guide, "decode_tours: guide")
    sess._require_gpu("decode_tours")
    instances = list(instances)
    for k, inst in enumerate(instances):
        n = np.asarray(inst[0]).shape[0]
        if not MIN_N <= n <= MAX_N:
            raise ValueError("decode_tours: instance %d has %d vertices; the decoder takes %d <= n <= %d"
                             % (k, n, MIN_N, MAX_N))
    if beam is None and (select != "score" or workspace_bytes is not None):
        raise TypeError("decode_tours: select and workspace_bytes only apply with beam=K")
    if beam is not None:
        _beam_width("decode_tours", beam, select, shown="%r")
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
        rows += _decode_chunk(sess, model, instances[start:stop], targets[start:stop], time_steps, beam, select,
                              workspace_bytes, guide, votes)
    polished = [(None, None)] * len(instances)
    if polish and instances:
        from .dataset import label_tours
        kw = dict(restarts=1, kicks=0, lower_bound=False)
        kw.update(search_kw)
        if guide is not None:
            kw["candidates"] = [r.table for r in rows]
        res = label_tours([(x[0], x[1]) for x in instances], init_tours=[r.tour for r in rows], device=sess.device, **kw)
        polished = [(p.tour, p.cost) for p in res]
    records = []
    for r, target, (polished_tour, polished_cost) in zip(rows, targets, polished):
        fields = dict(tour=r.tour, cost=r.cost, n_missing=r.n_missing, feasible=r.n_missing == 0,
                      prediction=r.prediction, target_cost=target, polished_tour=polished_tour,
                      polished_cost=polished_cost)
        records.append(DecodedTour(**fields) if beam is None else BeamTour(score=r.score, n_closed=r.n_closed, **fields))
    return records
