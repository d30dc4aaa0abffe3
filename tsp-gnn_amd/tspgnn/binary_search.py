"""Binary search on the target cost with the decision network -- the inference caller of the hot path
in the reference (/root/reference/experiments/binary_search.py:13-78, ``get_cost``).

``get_cost(sess, model, instance, time_steps)`` keeps the reference's signature, return tuple and loop
(one ``sess.run(model['predictions'])`` per probe, same bracket updates and stopping rule).
``parallel=k`` (k > 1) is the MI355X-shaped variant: every round packs k copies of the instance with k
target costs spread over the bracket into ONE batch -- the graphs are independent blocks of EV -- and
narrows the bracket by a factor k+1 per forward pass instead of 2.
"""
import numpy as np

from .instance_loader import InstanceLoader


def cost_bounds(Mw, n):
    """Bracket of the per-vertex tour cost the search starts from, as the reference forms it
    (experiments/binary_search.py:21-33): each triangle of the weight matrix is laid out as a full n x n array
    (the other triangle zero-filled -- the zeros take part in the ranking, so for non-negative weights the lower
    end of the bracket is 0), its n smallest and n largest entries are summed, and the looser of the two
    triangles wins on either side.  Returned per vertex (divided by n)."""
    lows, highs = [], []
    for triangle in (np.triu(Mw), np.tril(Mw)):
        ranked = np.sort(triangle, axis=None)
        lows.append(ranked[:n].sum())
        highs.append(ranked[ranked.size - n:].sum())
    return min(lows) / n, max(highs) / n


def get_cost(sess, model, instance, time_steps, threshold=0.5, stopping_delta=0.01, parallel=1):
    Ma, Mw, route = instance
    n = Ma.shape[0]
    m = len(np.nonzero(Ma)[0])
    wmin, wmax = cost_bounds(Mw, n)
    wpred = (wmin + wmax) / 2
    # the true closing edge, unlike create_batch's quirk (binary_search.py:40 vs instance_loader.py:70)
    route_cost = sum(Mw[min(i, j), max(i, j)] for (i, j) in zip(route, route[1:] + route[:1])) / n
    k = max(1, int(parallel))
    EV, W, _, route_exists, n_vertices, n_edges = InstanceLoader.create_batch([(Ma, Mw, route)] * k, target_cost=wpred)
    feed_dict = {model["EV"]: EV, model["W"]: W, model["C"]: None, model["time_steps"]: time_steps,
                 model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    iterations, pred = 0, None
    while wmin < wpred * (1 - stopping_delta) or wpred * (1 + stopping_delta) < wmax:
        if k == 1:
            feed_dict[model["C"]] = np.ones((m, 1)) * wpred
            pred = sess.run(model["predictions"], feed_dict=feed_dict)
            if pred < threshold:
                wmin = wpred
            else:
                wmax = wpred
        else:
            probes = wmin + (wmax - wmin) * (np.arange(1, k + 1) / (k + 1.0))
            feed_dict[model["C"]] = np.repeat(probes, m).reshape(-1, 1)
            preds = sess.run(model["predictions"], feed_dict=feed_dict)
            # the answer is monotone in the target cost for a trained model: keep the bracket around
            # the first probe the network accepts
            accept = np.nonzero(preds >= threshold)[0]
            first = accept[0] if len(accept) else k
            lo = wmin if first == 0 else probes[first - 1]
            hi = wmax if first == k else probes[first]
            wmin, wmax = lo, hi
            pred = preds[min(first, k - 1):min(first, k - 1) + 1]
        wpred = (wmax + wmin) / 2
        iterations += 1
    return wpred, pred, route_cost, iterations


# ---------------------------------------------------------------------------- every instance of a test set at once
# get_cost above bisects one instance with one forward pass (and one host round trip) per probe; the reference calls it
# for every instance of a test set in turn (experiments/binary_search.py:108-130).  get_costs runs all of them together:
# one batch holds every instance's k probe copies, each instance keeps its bracket in device memory, and
# tspgnn_cost_search_step applies get_cost's update after each forward and writes the next probe costs straight into the
# batch's WC column.  One round -- E_init, the T-step loop, vote, segment mean, sigmoid, bracket update -- is one
# captured graph, replayed until every bracket has closed, with one small read-back per round.

# Graphs per chunk (one batch, one captured round).  1 024 graphs of the reference's test sizes (n = 20..40, ~450 edges
# on average) are ~0.5 M edge rows: the size of BASELINE C4's batch, which keeps every compute unit busy, while the
# captured round's activations stay at a few GB at d = 64.  A larger test set is split into balanced chunks.
DEFAULT_MAX_GRAPHS = 1024


def plan_chunks(n_instances, k, max_graphs=DEFAULT_MAX_GRAPHS):
    """Instance ranges [(start, stop), ...] of the chunks get_costs runs: in input order, an instance's k probe copies
    never split, every chunk at most ``max_graphs`` graphs, as few chunks as that allows, their sizes within one instance."""
    n_instances, k, max_graphs = int(n_instances), int(k), int(max_graphs)
    if k < 1:
        raise ValueError("plan_chunks: k=%d must be at least 1" % k)
    per = max_graphs // k
    if per < 1:
        raise ValueError("max_graphs=%d cannot hold the %d probe copies of one instance" % (max_graphs, k))
    if n_instances <= 0:
        return []
    n_chunks = -(-n_instances // per)
    base, extra = divmod(n_instances, n_chunks)     # the first `extra` chunks take one instance more
    bounds = np.cumsum([0] + [base + (c < extra) for c in range(n_chunks)])
    return [(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]


def _tour_cost(Mw, route, n):
    """get_cost's route_cost: the true closing edge, per vertex."""
    return sum(Mw[min(i, j), max(i, j)] for (i, j) in zip(route, route[1:] + route[:1])) / n


def get_costs(sess, model, instances, time_steps, threshold=0.5, stopping_delta=0.01, parallel=1, max_graphs=None,
              max_rounds=64, trace=False):
    """``get_cost`` for every instance of ``instances`` at once.  Returns, in input order, the four values get_cost
    returns for that instance -- (wpred, pred, route_cost, iterations): floats, a float32 array of shape (1,) (None when
    iterations == 0), and an int.  Given the same predictions the brackets are bit-identical to get_cost's.

    ``parallel=k`` packs k probe copies of each instance as get_cost's parallel variant does.  Instances are split into
    chunks of at most ``max_graphs`` graphs (default DEFAULT_MAX_GRAPHS), each with its own captured round.  More than
    ``max_rounds`` rounds in a chunk raise.  If a round's f16x2 forward leaves the fp16 range, the search kernel leaves
    that round's brackets alone and the rest of the chunk runs on bf16x3 (``sess.last_range_bits`` records the bits).

    ``trace=True`` returns ``(results, traces)``: per instance {"bounds": (lo, hi), "rounds": [{"probes": float32[k],
    "preds": float32[k], "lo": float, "hi": float}, ...]} -- the probe costs the forward consumed, its predictions, and
    the bracket after the update, for every round the instance took part in.

    Rank-local (no collective): each rank of a data-parallel session may search its own instances.  The variables must
    not change during the call (the captured round refuses to replay)."""
    sess._require_gpu("get_costs")
    k = max(1, int(parallel))
    instances = list(instances)
    plan = plan_chunks(len(instances), k, DEFAULT_MAX_GRAPHS if max_graphs is None else max_graphs)
    results, traces = [], []
    for start, stop in plan:
        r, t = _search_chunk(sess, model, instances[start:stop], time_steps, float(threshold), float(stopping_delta), k,
                             int(max_rounds), trace)
        results += r
        traces += t
    return (results, traces) if trace else results


def _search_chunk(sess, model, chunk, time_steps, threshold, stopping_delta, k, max_rounds, trace):
    import torch
    from . import _lib
    from .range_guard import decode

    n = len(chunk)
    bounds, route_costs = [], []
    for Ma, Mw, route in chunk:
        nv = Ma.shape[0]
        wmin, wmax = cost_bounds(Mw, nv)
        bounds.append((float(wmin), float(wmax)))
        route_costs.append(float(_tour_cost(Mw, route, nv)))
    # k adjacent copies per instance; the init launch writes the real probe costs into C
    EV, W, C, route_exists, n_vertices, n_edges = InstanceLoader.create_batch([x for x in chunk for _ in range(k)],
                                                                              target_cost=0.0)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: time_steps,
            model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    b = sess.prepare(feed, remember_adjacency=False)
    dev = sess.device
    lo = torch.tensor([x[0] for x in bounds], dtype=torch.float64, device=dev)
    hi = torch.tensor([x[1] for x in bounds], dtype=torch.float64, device=dev)
    iters = torch.zeros(n, dtype=torch.int32, device=dev)
    pred_out = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    n_active = torch.zeros(1, dtype=torch.int32, device=dev)
    guard = sess.store.guard
    host = torch.zeros(5, dtype=torch.int32).pin_memory()
    seg_h = np.concatenate([[0], np.cumsum(n_edges)]).astype(np.int64)

    def launch(mode, pred):
        _lib.call("tspgnn_cost_search_step", _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(iters), _lib.ptr(pred_out),
                  _lib.ptr(n_active), _lib.ptr(pred), _lib.ptr(b.WC), _lib.ptr(b.seg), _lib.ptr(guard.words), n, k,
                  threshold, stopping_delta, mode, _lib.current_stream())

    def read_status():
        """(active instances, the guard's words decoded) with one synchronisation."""
        host[0:1].copy_(n_active, non_blocking=True)
        host[1:].copy_(guard.words, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        status = host.tolist()
        return status[0], decode(status[1:])

    sess.range_exceeded()               # a flag left by an earlier, unchecked forward must not skip this search's rounds
    launch(0, None)
    active = read_status()[0]
    tr = [{"bounds": x, "rounds": []} for x in bounds] if trace else []
    forced = False
    replay = sess.capture_forward(b, epilogue=lambda out: launch(1, out["predictions"])) if active else None
    rounds = 0
    while active:
        if rounds >= max_rounds:
            raise RuntimeError("get_costs: %d of %d instances still open after max_rounds=%d" % (active, n, max_rounds))
        if trace:
            probes = b.WC[:, 1].cpu().numpy()[seg_h[:-1]].reshape(n, k)   # (every graph has at least one edge)
            it0 = iters.cpu().numpy()
        out = replay()
        still_active, words = read_status()
        if words.status or words.activation:
            sess.range_exceeded()       # raises on a loop timeout; clears the range bits, records sess.last_range_bits
            if forced:
                raise RuntimeError("get_costs: the range guard flagged a bf16x3 round (bits %d)" % words.activation)
            # the search kernel left this round's brackets alone: repeat it, and the rest of the chunk, on bf16x3
            del replay, out
            forced = True
            with model["gnn"].forced_off_h2():
                replay = sess.capture_forward(b, epilogue=lambda out: launch(1, out["predictions"]))
            continue
        rounds += 1
        active = still_active
        if trace:
            preds = out["predictions"].cpu().numpy().reshape(n, k)
            it1, lo_h, hi_h = iters.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
            for i in np.nonzero(it1 != it0)[0]:
                tr[i]["rounds"].append({"probes": probes[i].copy(), "preds": preds[i].copy(), "lo": float(lo_h[i]),
                                        "hi": float(hi_h[i])})
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    it_h, po_h = iters.cpu().numpy(), pred_out.cpu().numpy()
    results = []
    for i in range(n):
        wpred = float((hi_h[i] + lo_h[i]) / 2)
        pred = None if it_h[i] == 0 else np.array([po_h[i]], dtype=np.float32)
        results.append((wpred, pred, route_costs[i], int(it_h[i])))
    return results, tr
