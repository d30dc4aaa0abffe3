"""Labelled TSP instances: the counterpart of the reference's ``dataset.py`` (create_graph, create_dataset, solve).

The reference labels every instance with Concorde (dataset.py:9-50).  Here the label comes from HIP kernels:
``tspgnn_tour_search`` (csrc/tour_search.hip), a batched multi-start iterated local search that returns a short tour;
``tspgnn_tour_lower_bound``, the Held-Karp 1-tree bound that certifies how far that tour can be from the optimum; and
``tspgnn_tour_branch_bound`` (csrc/tour_exact.hip), a branch and bound on that bound which starts from the search's tour
and either proves it optimal, replaces it by a better one and proves that, or runs out of its node budget and says so
(``prove_tours``, ``label_tours(exact=True)``, ``create_dataset(exact=True)``; n <= 128).  Without ``exact`` a label is
trusted when ``certify`` says the bound and the tour settle it for the target cost ``create_batch`` will feed
(DESIGN.md §12).

Instance generation (create_graph, create_dataset) draws from the global ``random`` / ``np.random`` in exactly the
reference's order, so a script that seeds them as the reference's train.py does gets the reference's instances.
"""
import collections
import os
import random
import time

import numpy as np
import torch

from . import _lib
from .instance_loader import route_cost, write_graph

MAX_N = 128
MAX_N_TRI = 256   # label_tours: the triangle kernels (n 129-256)
MAX_NEIGHBORS = 32   # neighbors=K: the widest neighbour table of tspgnn_tour_search_knn
CLOSURE_MAX_N = 256       # metric_closure: the largest matrix tspgnn_metric_closure takes
CLOSURE_LDS_MAX_N = 143   # ... and the largest it closes in LDS: 8 n^2 <= 160 KiB (kClosureLdsMaxN, csrc/tour_closure.hip)

# Defaults measured on the MI355X at the reference's training shape (n 20-40): 8 chains of 96 kicks label
# 2^15 instances in a few seconds, and on n 5-13 they match exact optima; 400 subgradient steps bring the median
# (cost - lb) / cost under 1 %.  More restarts and kicks only pay at larger n.
DEFAULT_RESTARTS = 8
DEFAULT_KICKS = 96
DEFAULT_LB_ITERS = 400
# n 129-256 (label_tours on the triangle kernels; DESIGN.md §12, 2^10 instances at n 200 and 256): the search, not the
# bound, limits certification there, and it keeps gaining with kicks (certified at dev 0.02, n 200: 0.36 / 0.87 / 0.94 at
# 96 / 384 / 768 kicks; n 256: 0.11 / 0.68 / 0.92), while 1 000 bound steps change nothing.  384 kicks cost 11 s of
# search per 2^10 instances at n 200, 18 s at n 256.
DEFAULT_RESTARTS_LARGE = 8
DEFAULT_KICKS_LARGE = 384
DEFAULT_LB_ITERS_LARGE = 400
DEFAULT_CHUNK = 8192
# Branch and bound (prove_tours; DESIGN.md §12 has the measured table): nodes per instance and ascent steps per node.
# One launch runs at most max_nodes * (node_iters + 1) + root_iters 1-trees per instance.
DEFAULT_BB_NODES = 2048
DEFAULT_BB_ITERS = 30
BB_WORKSPACE_BYTES = 1 << 30   # most workspace of one branch-and-bound launch; larger chunks are split
BB_STATUS = ("proved", "budget", "skipped")   # TSPGNN_BB_PROVED, TSPGNN_BB_BUDGET; 'skipped': no launch for it

TourResult = collections.namedtuple("TourResult", ["tour", "cost", "lb", "feasible", "target"])
TourResult.__doc__ = """One solved instance.
tour: list of vertex ids, canonical (starts at 0, tour[1] < tour[-1]); cost: fp64 cycle cost with w(i,j) = Mw[min, max];
lb: a lower bound on every tour that uses real edges only (nan when not computed, inf when no such tour exists for n < 4);
feasible: the tour uses real edges only; target: Q = n * route_cost(Mw_file, tour), the cost create_batch derives from the
written file (instance_loader.py:70 pairs route[-1] with route[1]; Mw_file is zero off the upper-triangular edge set)."""


def _edge_mask(Ma):
    A = np.asarray(Ma) != 0
    A = A | A.T
    np.fill_diagonal(A, False)
    return A


def _check(k, Ma, Mw, max_n=MAX_N):
    Ma = np.asarray(Ma)
    Mw = np.asarray(Mw, dtype=np.float64)
    if Ma.ndim != 2 or Ma.shape[0] != Ma.shape[1] or Mw.shape != Ma.shape:
        raise ValueError("instance %d: Ma %s and Mw %s must be the same square shape" % (k, Ma.shape, Mw.shape))
    n = Ma.shape[0]
    if n < 1:
        raise ValueError("instance %d: empty graph" % k)
    if n > max_n:
        raise ValueError("instance %d: n=%d exceeds the tour kernels' limit of %d vertices" % (k, n, max_n))
    w = np.triu(Mw, 1)[np.triu(_edge_mask(Ma), 1)]
    if w.size and (not np.all(np.isfinite(w)) or w.min() < 0):
        raise ValueError("instance %d: edge weights must be finite and non-negative" % k)
    return Ma, Mw, n


def _penalised(A, Mw):
    """[b,n,n] fp32 matrices for the kernels: w(i,j) = Mw[min, max] on edges, n * max(real weight) + 1 off them, rounded
    towards -inf so that the lower bound computed on them is a lower bound for the fp64 weights too."""
    b, n, _ = Mw.shape
    up = np.triu(Mw, 1)
    w = up + up.transpose(0, 2, 1)
    mx = np.where(A, w, 0.0).reshape(b, -1).max(axis=1)
    pen = n * mx + 1.0
    W = np.where(A, w, pen[:, None, None])
    idx = np.arange(n)
    W[:, idx, idx] = 0.0
    W32 = W.astype(np.float32)
    over = W32.astype(np.float64) > W
    W32[over] = np.nextafter(W32[over], np.float32(-np.inf))
    return W32


def _penalised_tri(A, Mw):
    """[b, n(n-1)/2] fp32 strict upper triangles, row-major, for the _tri kernels: the values of _penalised at (i < j),
    with the same penalty and the same rounding towards -inf."""
    b, n, _ = Mw.shape
    iu = np.triu_indices(n, 1)
    w = Mw[:, iu[0], iu[1]] + 0.0   # as _penalised's up + up.T: -0 becomes +0
    a = A[:, iu[0], iu[1]]
    mx = np.where(a, w, 0.0).max(axis=1) if w.shape[1] else np.zeros(b)
    pen = n * mx + 1.0
    W = np.where(a, w, pen[:, None])
    W32 = W.astype(np.float32)
    over = W32.astype(np.float64) > W
    W32[over] = np.nextafter(W32[over], np.float32(-np.inf))
    return W32


def _cycle_cost(Mw, tours):
    """fp64 cost of [b,n] tours under w(i,j) = Mw[min(i,j), max(i,j)], summed in tour order."""
    nxt = np.roll(tours, -1, axis=1)
    lo, hi = np.minimum(tours, nxt), np.maximum(tours, nxt)
    b = np.arange(tours.shape[0])[:, None]
    w = Mw[b, lo, hi]
    out = np.zeros(tours.shape[0])
    for k in range(tours.shape[1]):   # sequential, as the host computes any tour cost
        out += w[:, k]
    return out


def _host_small(Ma, Mw, n):
    """n < 4: there is one tour (0, 1, ..., n-1); its cost is exact, so it is its own bound."""
    tour = list(range(n))
    A = _edge_mask(Ma)
    pairs = list(zip(tour, tour[1:] + tour[:1])) if n > 1 else []
    feasible = all(A[a, b] for a, b in pairs)
    cost = float(sum(Mw[min(a, b), max(a, b)] for a, b in pairs))
    return tour, cost, (cost if feasible else float("inf")), feasible


def _target(Ma, Mw, tour):
    n = len(tour)
    mw_file = np.where(np.triu(_edge_mask(Ma), 1), np.asarray(Mw, dtype=np.float64), 0.0)
    return n * route_cost(mw_file, tour) if n > 1 else 0.0


def solve_tours(instances, restarts=DEFAULT_RESTARTS, kicks=DEFAULT_KICKS, seed=0, init_tours=None, lower_bound=True,
                device=None, lb_iters=DEFAULT_LB_ITERS, chunk=DEFAULT_CHUNK, index=None, timings=None, neighbors=None,
                candidates=None):
    """Solve symmetric TSP instances on the GPU, many at once.

    instances: list of (Ma, Mw); Ma upper-triangular or symmetric (nonzero = edge), Mw [n,n] with w(i,j) = Mw[min, max].
    Edges absent from Ma cost n * max(real weight) + 1, more than any tour over real edges.
    restarts: wave64 chains per instance (1..16); kicks: double-bridge kicks per chain; seed: the generator's key.
    init_tours: optional list (None entries allowed) of starting tours for chain 0 -- create_dataset passes the planted
    cycle, so a planted graph always gets a feasible tour.
    lower_bound: also run the Held-Karp bound (lb_iters subgradient steps).  chunk: instances per launch.
    index: the key of each instance in the generator (default: its position in ``instances``); results depend on
    (seed, index, restarts, kicks, neighbors) only, never on ``chunk``.
    neighbors: None = every descent step scans the whole 2-opt + Or-opt neighbourhood (tspgnn_tour_search).  K in 1..32 =
    it scans only the moves that add an edge {x, y} with y among the K nearest vertices of x or x among y's
    (tspgnn_tour_search_knn): many times fewer evaluations per step, so more kicks in the same time.
    candidates: None, or one array-like [n, K] per instance, the same K in 1..32 for all, values 0..255: the caller's own
    candidate table in place of the K nearest (tspgnn_tour_search_cand).  Entry (x, s) = y lets the descent add the edge
    {x, y} when y < n and y != x; any other value (x itself by convention) stands for nothing.  Rows may be asymmetric,
    repeat a vertex or be empty of pairs; results then depend on (seed, index, restarts, kicks, candidates) only.
    Exclusive with ``neighbors``.  The tables of instances with n < 4 are checked and not used.
    timings: optional dict that receives the seconds spent in 'pack', 'search' and 'bound' (device-synchronised).
    n < 4 is solved on the host; n > 128 raises ValueError before anything is launched.

    Returns a list of TourResult (tour, cost, lb, feasible, target).
    """
    t0 = time.perf_counter()
    _check_neighbors(neighbors, candidates)
    checked, index = _validate(instances, restarts, kicks, lb_iters, chunk, index, init_tours, MAX_N)
    candidates = _check_candidates(candidates, checked)
    return _solve(checked, index, tri=False, restarts=restarts, kicks=kicks, seed=seed, init_tours=init_tours,
                  lower_bound=lower_bound, device=device, lb_iters=lb_iters, chunk=chunk, timings=timings, t0=t0,
                  neighbors=neighbors, candidates=candidates)[0]


def _check_counts(restarts, kicks, lb_iters, chunk):
    if not 1 <= restarts <= 16:
        raise ValueError("restarts=%d must be in [1, 16]" % restarts)
    if kicks < 0 or lb_iters < 1 or chunk < 1:
        raise ValueError("kicks, lb_iters and chunk must be non-negative / positive")


def _check_neighbors(neighbors, candidates=None):
    if neighbors is not None and candidates is not None:
        raise ValueError("neighbors and candidates are exclusive: the search descends over one candidate table")
    if neighbors is None:
        return
    if isinstance(neighbors, bool) or not isinstance(neighbors, (int, np.integer)) or not 1 <= neighbors <= MAX_NEIGHBORS:
        raise ValueError("neighbors=%r must be None or an int in [1, %d]" % (neighbors, MAX_NEIGHBORS))


def _validate(instances, restarts, kicks, lb_iters, chunk, index, init_tours, max_n):
    _check_counts(restarts, kicks, lb_iters, chunk)
    checked = [_check(k, Ma, Mw, max_n) for k, (Ma, Mw) in enumerate(instances)]
    B = len(checked)
    index = np.arange(B, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64).reshape(-1)
    if index.shape[0] != B or (B and index.min() < 0):
        raise ValueError("index must hold one non-negative key per instance")
    if init_tours is not None and len(init_tours) != B:
        raise ValueError("init_tours must hold one entry (or None) per instance")
    return checked, index


def _check_candidates(candidates, checked):
    """candidates=: None, or one [n, K] table per checked instance -> a list of uint8 arrays, K the same for all."""
    if candidates is None:
        return None
    candidates = list(candidates)
    if len(candidates) != len(checked):
        raise ValueError("candidates must hold one [n, K] table per instance")
    out, K = [], None
    for k, (tab, (_, _, n)) in enumerate(zip(candidates, checked)):
        raw = np.asarray(tab)
        if raw.ndim != 2 or raw.shape[0] != n:
            raise ValueError("candidates[%d] has shape %s; an instance of %d vertices takes [%d, K]"
                             % (k, raw.shape, n, n))
        if K is None:
            K = raw.shape[1]
            if not 1 <= K <= MAX_NEIGHBORS:
                raise ValueError("candidates: K=%d columns; the search takes 1 <= K <= %d" % (K, MAX_NEIGHBORS))
        if raw.shape[1] != K:
            raise ValueError("candidates[%d] has %d columns, candidates[0] has %d: one K for all"
                             % (k, raw.shape[1], K))
        if raw.dtype.kind not in "iu" or (raw.size and (raw.min() < 0 or raw.max() > 255)):
            raise ValueError("candidates[%d] must hold integers in 0..255" % k)
        out.append(np.ascontiguousarray(raw, dtype=np.uint8))
    return out


def _cand_columns(candidates):
    return None if not candidates else candidates[0].shape[1]


def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _to_device(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _add_time(timings, key, seconds):
    if timings is not None:
        timings[key] = timings.get(key, 0.0) + seconds


def _spans(count, chunk):
    """(c0, c1) of every launch over ``count`` instances, ``chunk`` at a time; the last one may be shorter."""
    for c0 in range(0, count, chunk):
        yield c0, min(count, c0 + chunk)


def _split(ns):
    """[(tri, positions)] of the non-empty size classes of the vertex counts ``ns``: n <= 128 on the square kernels, above
    on the triangle kernels."""
    above = np.asarray(ns) > MAX_N
    return [(tri, sel) for tri, sel in ((False, np.flatnonzero(~above)), (True, np.flatnonzero(above))) if len(sel)]


def _byte_chunks(order, ns, chunk_bytes):
    """The positions ``order`` (into the vertex counts ``ns``) cut greedily into runs of at most chunk_bytes of fp64
    n x n matrices, and at least one instance each."""
    runs, cur, size = [], [], 0
    for p in order:
        b = 8 * int(ns[p]) ** 2
        if cur and size + b > chunk_bytes:
            runs.append(cur)
            cur, size = [], 0
        cur.append(int(p))
        size += b
    if cur:
        runs.append(cur)
    return runs


# The instances of one kernel layout, packed (_pack).  out: per instance the TourResult where n < 4, else None; checked:
# the (Ma, Mw, n) it was made from; big: the positions of the n >= 4 instances in launch order.  Per launched instance: ns
# int32, w_off / t_off (its first float in W, its first vertex in init and the kernels' tours), mean_w (None unless asked
# for).  W: the penalised fp32 matrices, flat; init: the starting tours, -1 where there is none; has_init: some instance
# came with one.  groups: {n: positions in big}; stacked: {n: (edge masks, fp64 weights)} of a group.  cand / c_off: the
# candidate tables of the launched instances, flat uint8, each one's first byte and their column count (None without
# candidates=).
Packed = collections.namedtuple("Packed", ["out", "checked", "big", "ns", "w_off", "t_off", "W", "init", "has_init",
                                           "mean_w", "groups", "stacked", "cand", "c_off", "columns"],
                            defaults=(None, None, None))
# What the tour kernels read and write for G instances of one layout: ns, the host copy of n, then the device arrays (init
# None: no starting tours; cost None: prove_tours; idx and lb None for the baselines, which take neither; cand, c_off and
# columns None unless the search descends over the caller's tables).
LabelArrays = collections.namedtuple("LabelArrays", "ns W w_off t_off n idx init tours cost lb cand c_off columns",
                                     defaults=(None, None, None))


def _pack(checked, tri, init_tours=None, lower_bound=False, incumbents=None, mean_weight=False, candidates=None):
    """Checked instances -> Packed: n < 4 solved on the host (lb = nan unless lower_bound), the rest packed for the square
    (tri=False) or triangle kernels, grouped by n so that the penalties, costs and targets are array operations.
    incumbents: one tour per instance, taken as its starting tour unchecked (prove_tours has checked them).
    mean_weight: also the mean real edge weight per instance (annealing's temperature unit).
    candidates: _check_candidates' tables, one per checked instance; they are laid out in launch order beside the tours."""
    out = [None] * len(checked)
    for k, (Ma, Mw, n) in enumerate(checked):
        if n < 4:
            tour, cost, lb, feas = _host_small(Ma, Mw, n)
            out[k] = TourResult(tour, cost, lb if lower_bound else float("nan"), feas, _target(Ma, Mw, tour))
    big = [k for k, c in enumerate(checked) if c[2] >= 4]
    ns = np.array([checked[k][2] for k in big], dtype=np.int32)
    order = np.argsort(ns, kind="stable")            # launch order: by n (similar work per workgroup)
    big = [big[k] for k in order]
    ns = ns[order]
    sq = ns.astype(np.int64) * (ns - 1) // 2 if tri else ns.astype(np.int64) ** 2   # floats per instance
    w_off = np.concatenate([[0], np.cumsum(sq)[:-1]]).astype(np.int64)
    t_off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    Wflat = np.empty(int(sq.sum()), dtype=np.float32)
    init = np.full(int(ns.sum()), -1, dtype=np.int32)
    mean_w = np.zeros(len(big)) if mean_weight else None
    groups, stacked = {}, {}
    for pos in range(len(big)):
        groups.setdefault(int(ns[pos]), []).append(pos)
    for n, poss in groups.items():
        A = np.stack([_edge_mask(checked[big[p]][0]) for p in poss])
        Mw = np.stack([checked[big[p]][1] for p in poss])
        W32 = (_penalised_tri if tri else _penalised)(A, Mw)
        if mean_weight:
            up = np.triu(A, 1)
            mean_w[poss] = np.where(up, Mw, 0.0).sum(axis=(1, 2)) / np.maximum(up.sum(axis=(1, 2)), 1)
        for g, p in enumerate(poss):
            Wflat[w_off[p]:w_off[p] + sq[p]] = W32[g].reshape(-1)
            if incumbents is not None:
                init[t_off[p]:t_off[p] + n] = incumbents[big[p]]
            elif init_tours is not None and init_tours[big[p]] is not None:
                it = np.asarray(init_tours[big[p]], dtype=np.int64).reshape(-1)
                if it.shape[0] != n or not np.array_equal(np.sort(it), np.arange(n)):
                    raise ValueError("init_tours[%d] is not a permutation of 0..%d" % (big[p], n - 1))
                init[t_off[p]:t_off[p] + n] = it
        stacked[n] = (A, Mw)
    has_init = init_tours is not None and any(t is not None for t in init_tours)
    cand = c_off = K = None
    if candidates:
        K = _cand_columns(candidates)
        c_off = (t_off * K).astype(np.int64)
        cand = np.concatenate([candidates[k].reshape(-1) for k in big]) if big else np.zeros(0, dtype=np.uint8)
    return Packed(out, checked, big, ns, w_off, t_off, Wflat, init, has_init, mean_w, groups, stacked, cand, c_off, K)


def _upload(pk, dev, index=None, bound=False):
    """Packed -> LabelArrays on ``dev``.  index: the generator key of every packed instance (idx); bound: allocate lb."""
    G = len(pk.big)
    return LabelArrays(pk.ns, _to_device(pk.W, dev), _to_device(pk.w_off, dev), _to_device(pk.t_off, dev),
                       _to_device(pk.ns, dev), None if index is None else _to_device(index[pk.big], dev),
                       _to_device(pk.init, dev) if pk.has_init else None,
                       torch.empty(int(pk.ns.sum()), dtype=torch.int32, device=dev),
                       torch.empty(G, dtype=torch.float32, device=dev),
                       torch.empty(G, dtype=torch.float64, device=dev) if bound else None,
                       None if pk.cand is None else _to_device(pk.cand, dev),
                       None if pk.cand is None else _to_device(pk.c_off, dev),
                       pk.columns)


def _finish(pk, tours, lbs=None):
    """TourResults of the packed instances from the kernels' tours (fp64 cycle cost, feasibility, target Q) and, per
    launched instance, the bounds ``lbs`` (None: nan)."""
    out, big, t_off = pk.out, pk.big, pk.t_off
    for n, poss in pk.groups.items():
        A, Mw = pk.stacked[n]
        T = np.stack([tours[t_off[p]:t_off[p] + n] for p in poss])
        cost = _cycle_cost(Mw, T)
        feas = A[np.arange(len(poss))[:, None], T, np.roll(T, -1, axis=1)].all(axis=1)
        for g, p in enumerate(poss):
            k = big[p]
            tour = [int(x) for x in T[g]]
            out[k] = TourResult(tour, float(cost[g]), float("nan") if lbs is None else float(lbs[p]), bool(feas[g]),
                                _target(pk.checked[k][0], pk.checked[k][1], tour))
    return out


def _launch_labels(dev, a, *, restarts, kicks, seed, lb_iters, chunk, tri, neighbors=None, lower_bound=True, exact=None,
                   search=True):
    """The launches of one size class over the LabelArrays ``a``, already on ``dev`` (inside torch.cuda.device(dev)): the
    search, ``chunk`` instances per launch, then the branch and bound (exact = (max_nodes, node_iters, opt_tol), tri=False
    only) or the bound (lower_bound).  search=False: a.tours already holds the incumbents (a.cost None: the root's step
    then aims at the incumbent's own cost).  a.cand: the search is the _cand entry point over the caller's tables of
    a.columns columns, a launch reading its instances' tables through a.c_off.  -> (t1, t2, t3, d_stat, d_nodes):
    perf_counter before the search, after it and after the bound, each device-synchronised, and the branch and bound's
    int32 device arrays (None without exact)."""
    ns, d_W, d_woff, d_toff, d_n, d_idx, d_init, d_tours, d_cost, d_lb = a[:10]
    G = len(ns)
    search_fn, bound_fn = ("tspgnn_tour_search_tri", "tspgnn_tour_lower_bound_tri") if tri else \
        ("tspgnn_tour_search", "tspgnn_tour_lower_bound")
    knn = ()
    if neighbors is not None:
        search_fn, knn = search_fn.replace("_search", "_search_knn"), (int(neighbors),)
    if a.cand is not None:
        search_fn, knn = search_fn.replace("_search", "_search_cand"), (int(a.columns),)
    d_stat = d_nodes = None
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    st = _lib.current_stream()
    for c0, c1 in _spans(G if search else 0, chunk):
        _lib.call(search_fn, _lib.ptr(d_W), _lib.ptr(d_woff[c0:c1]), _lib.ptr(d_n[c0:c1]),
                  _lib.ptr(d_init), _lib.ptr(d_toff[c0:c1]), _lib.ptr(d_idx[c0:c1]),
                  *(() if a.cand is None else (_lib.ptr(a.cand), _lib.ptr(a.c_off[c0:c1]))), c1 - c0,
                  int(ns[c0:c1].max()), int(restarts), int(kicks), *knn, int(seed) & 0xFFFFFFFFFFFFFFFF,
                  _lib.ptr(d_tours), _lib.ptr(d_cost[c0:c1]), st)
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    if exact is not None:
        # results do not depend on the launch size, so a chunk whose stack would not fit BB_WORKSPACE_BYTES is split
        per = int(_lib.lib.tspgnn_tour_branch_bound_ws(1, int(ns.max())))
        step = max(1, min(chunk, G, BB_WORKSPACE_BYTES // per))
        d_ws = torch.empty(per * step, dtype=torch.uint8, device=dev)
        d_nodes = torch.empty(G, dtype=torch.int32, device=dev)
        d_stat = torch.empty(G, dtype=torch.int32, device=dev)
        for c0, c1 in _spans(G, step):
            _lib.call("tspgnn_tour_branch_bound", _lib.ptr(d_W), _lib.ptr(d_woff[c0:c1]), _lib.ptr(d_n[c0:c1]),
                      _lib.ptr(d_toff[c0:c1]), _lib.ptr(None if d_cost is None else d_cost[c0:c1]), c1 - c0,
                      int(ns[c0:c1].max()), int(lb_iters), int(exact[1]), int(exact[0]), float(exact[2]),
                      _lib.ptr(d_ws), _lib.ptr(d_tours), _lib.ptr(d_lb[c0:c1]), _lib.ptr(d_nodes[c0:c1]),
                      _lib.ptr(d_stat[c0:c1]), st)
    elif lower_bound:
        for c0, c1 in _spans(G, chunk):
            _lib.call(bound_fn, _lib.ptr(d_W), _lib.ptr(d_woff[c0:c1]), _lib.ptr(d_n[c0:c1]),
                      _lib.ptr(d_cost[c0:c1]), c1 - c0, int(ns[c0:c1].max()), int(lb_iters), _lib.ptr(d_lb[c0:c1]), st)
    torch.cuda.synchronize(dev)
    t3 = time.perf_counter()
    return t1, t2, t3, d_stat, d_nodes


def _solve(checked, index, *, tri, lb_iters, chunk, t0, restarts=1, kicks=0, seed=0, init_tours=None, lower_bound=True,
           device=None, timings=None, exact=None, incumbents=None, neighbors=None, candidates=None):
    """solve_tours on checked instances, n < 4 on the host and the rest on the square kernels (tri=False, n <= 128) or
    the triangle kernels (tri=True, n <= 256); neighbors=K: the search is the _knn entry point of that layout;
    candidates (one checked table per instance): its _cand entry point.
    exact = (max_nodes, node_iters, opt_tol): the branch and bound takes the place of the bound launch (tri=False only).
    incumbents: one tour per instance; the search is skipped and the branch and bound starts from these.  t0: perf_counter
    where timings['pack'] begins.  -> (results, status, nodes): with exact the branch and bound's int64 status and node
    count per instance (n < 4: proved, 0 nodes), otherwise None."""
    pk = _pack(checked, tri, init_tours, lower_bound=lower_bound, incumbents=incumbents, candidates=candidates)
    status = nodes = None
    if exact is not None:
        status, nodes = np.zeros(len(checked), dtype=np.int64), np.zeros(len(checked), dtype=np.int64)
    if not pk.big:
        return pk.out, status, nodes
    dev = _device(device)
    with torch.cuda.device(dev):
        a = _upload(pk, dev, index, bound=True)
        if incumbents is not None:
            a.tours.copy_(torch.from_numpy(pk.init))
            a = a._replace(cost=None)   # the root's step then aims at the incumbent's own cost
        t1, t2, t3, d_stat, d_nodes = _launch_labels(dev, a, restarts=restarts, kicks=kicks, seed=seed, lb_iters=lb_iters,
                                                     chunk=chunk, tri=tri, neighbors=neighbors, lower_bound=lower_bound,
                                                     exact=exact, search=incumbents is None)
        if exact is not None:
            status[pk.big] = d_stat.cpu().numpy()
            nodes[pk.big] = d_nodes.cpu().numpy()
        tours = a.tours.cpu().numpy().astype(np.int64)
        lbs = a.lb.cpu().numpy() if lower_bound or exact is not None else None
    _add_time(timings, "pack", t1 - t0)
    _add_time(timings, "search", t2 - t1)
    _add_time(timings, "bound" if exact is None else "exact", t3 - t2)
    return _finish(pk, tours, lbs), status, nodes


def _label_settings(restarts, kicks, lb_iters, neighbors, exact, max_nodes, chunk=1, candidates=None):
    """label_tours' settings, checked in label_tours' order (None: DEFAULT_* / DEFAULT_*_LARGE): -> ((restarts, kicks,
    lb_iters) for n <= 128, the same for n 129-256, the branch and bound's (max_nodes, node_iters, opt_tol) or None)."""
    _check_neighbors(neighbors, candidates)
    bb = None
    if exact:
        bb = (DEFAULT_BB_NODES if max_nodes is None else max_nodes, DEFAULT_BB_ITERS, 1e-9)
        _check_bb(*bb)
    small = (DEFAULT_RESTARTS if restarts is None else restarts, DEFAULT_KICKS if kicks is None else kicks,
             DEFAULT_LB_ITERS if lb_iters is None else lb_iters)
    large = (DEFAULT_RESTARTS_LARGE if restarts is None else restarts,
             DEFAULT_KICKS_LARGE if kicks is None else kicks, DEFAULT_LB_ITERS_LARGE if lb_iters is None else lb_iters)
    _check_counts(*large, chunk)
    _check_counts(*small, chunk)
    return small, large, bb


def _check_chains_fit(restarts, n_big, neighbors, word="restarts"):
    """n_big: the largest n above MAX_N among the instances (0: none), where ``restarts`` chains must fit in LDS;
    ``word``: what the caller calls its chains."""
    if n_big and restarts > tri_chains_fit(n_big, neighbors):
        raise ValueError("%s=%d: at n=%d at most %d chains fit in LDS"
                         % (word, restarts, n_big, tri_chains_fit(n_big, neighbors)))


def tri_chains_fit(n, neighbors=None):
    """The most restarts tspgnn_tour_search_tri takes at n_max = n (10 at n = 256), or with neighbors=K
    tspgnn_tour_search_knn_tri (9 at n = 256 with K = 8): the library's own rule, tspgnn_tour_chains_fit (the LDS layout
    behind it: include/tspgnn.h, tspgnn_tour_search_tri)."""
    return int(_lib.lib.tspgnn_tour_chains_fit(1, int(n), 0 if neighbors is None else int(neighbors)))


def _bb_stats(stats, status, nodes, seconds):
    if stats is not None:
        stats["status"] = np.array([BB_STATUS[s] for s in status])
        stats["nodes"] = np.asarray(nodes, dtype=np.int64)
        stats["seconds"] = float(seconds)


def _check_bb(max_nodes, node_iters, opt_tol):
    if not 1 <= max_nodes <= 65536:
        raise ValueError("max_nodes=%d must be in [1, 65536]" % max_nodes)
    if node_iters < 1:
        raise ValueError("node_iters=%d must be positive" % node_iters)
    if not (np.isfinite(opt_tol) and opt_tol >= 0):
        raise ValueError("opt_tol=%r must be finite and non-negative" % (opt_tol,))


def prove_tours(instances, results, max_nodes=DEFAULT_BB_NODES, node_iters=DEFAULT_BB_ITERS, root_iters=DEFAULT_LB_ITERS,
                opt_tol=1e-9, device=None, chunk=DEFAULT_CHUNK, stats=None):
    """Exact labels: prove the tours of solve_tours / label_tours optimal, or improve them, by branch and bound on the
    Held-Karp 1-tree bound (tspgnn_tour_branch_bound, csrc/tour_exact.hip) -- Concorde's role in the reference
    (dataset.py:9-50).

    instances: as solve_tours; results: one TourResult per instance, whose tour is the incumbent.
    max_nodes: nodes per instance (1..65536); node_iters / root_iters: ascent steps per node / at the root; opt_tol: a
    node is pruned when its bound reaches (1 - opt_tol) times the incumbent's cost.  chunk: instances per launch.
    stats: optional dict that receives 'status' (array of 'proved' / 'budget' / 'skipped'), 'nodes' (per instance) and
    'seconds' (of the launches, device-synchronised).

    Returns a list of TourResult: lb is the branch and bound's, and tour, cost, feasible and target are those of the best
    tour it holds at the end (the incumbent, or a cheaper one it met).  'proved' means: under the fp64 weights no tour is
    cheaper than ``cost`` by more than (opt_tol + n * 2**-24) * cost -- the kernel sees fp32 weights, each rounded down by
    at most one ulp.  (Concorde in the reference sees int(10**6 * w), exact only to 10**-6 per edge, which is coarser.)
    'budget' means max_nodes ran out: lb is still a valid bound and the tour the best found.  Instances with n < 4 (their
    host bound is already exact: 'proved'), with n > 128, or whose incumbent is infeasible ('skipped') pass through
    unchanged.  Results never depend on chunk or on which other instances share the call.
    """
    if len(instances) != len(results):
        raise ValueError("prove_tours: %d instances but %d results" % (len(instances), len(results)))
    _check_counts(1, 0, root_iters, chunk)
    _check_bb(max_nodes, node_iters, opt_tol)
    checked = [_check(k, Ma, Mw, MAX_N_TRI) for k, (Ma, Mw) in enumerate(instances)]
    B = len(checked)
    status = np.full(B, 2, dtype=np.int64)
    nodes = np.zeros(B, dtype=np.int64)
    sel = []
    for k, ((_, _, n), r) in enumerate(zip(checked, results)):
        if sorted(r.tour) != list(range(n)):
            raise ValueError("prove_tours: results[%d].tour is not a permutation of 0..%d" % (k, n - 1))
        if n < 4:
            status[k] = 0
        elif n <= MAX_N and r.feasible:
            sel.append(k)
    out = list(results)
    times = {}
    if sel:
        res, status[sel], nodes[sel] = _solve(
            [checked[k] for k in sel], np.arange(len(sel), dtype=np.int64), tri=False, device=device, lb_iters=root_iters,
            chunk=chunk, timings=times, t0=time.perf_counter(), exact=(max_nodes, node_iters, opt_tol),
            incumbents=[results[k].tour for k in sel])
        for j, k in enumerate(sel):
            out[k] = res[j]
    _bb_stats(stats, status, nodes, times.get("exact", 0.0))
    return out


def label_tours(instances, restarts=None, kicks=None, lb_iters=None, seed=0, init_tours=None, lower_bound=True,
                device=None, chunk=DEFAULT_CHUNK, index=None, timings=None, exact=False, max_nodes=None, stats=None,
                neighbors=None, candidates=None):
    """solve_tours for instances of up to MAX_N_TRI = 256 vertices, split by n: n < 4 on the host, 4-128 on the square
    kernels (exactly solve_tours), 129-256 on the packed-triangle kernels (tspgnn_tour_search_tri /
    tspgnn_tour_lower_bound_tri); n > 256 raises ValueError before anything is launched.

    restarts, kicks, lb_iters: None takes DEFAULT_* for n <= 128 and DEFAULT_*_LARGE for n > 128; a value applies to both.
    For n > 128 restarts may not exceed tri_chains_fit(largest n, neighbors) (10 at n = 256; 9 with neighbors=8).  The
    other arguments are solve_tours'.  Results come back in input order; each depends on (seed, its index, restarts, kicks,
    neighbors) only, never on chunk or on which other instances share the call.
    exact=True: for n <= 128 the branch and bound (prove_tours, with max_nodes or DEFAULT_BB_NODES, DEFAULT_BB_ITERS
    steps per node and lb_iters at the root) takes the place of the bound launch: lb is its bound and the tour the best it
    holds.  stats then receives prove_tours' 'status', 'nodes' and 'seconds'; n > 128 is 'skipped' and keeps the plain
    bound.  timings gets the launch under 'exact'.
    candidates: solve_tours' (tspgnn_tour_search_cand / _cand_tri), exclusive with neighbors; for n > 128 restarts may not
    exceed tri_chains_fit(largest n, K).  Everything about them is checked before any device work.
    """
    t0 = time.perf_counter()
    small, large, bb = _label_settings(restarts, kicks, lb_iters, neighbors, exact, max_nodes, chunk, candidates)
    if bb is not None:
        timings = {} if timings is None else timings
        before = timings.get("exact", 0.0)
    checked, index = _validate(instances, *small, chunk, index, init_tours, MAX_N_TRI)
    ns = [c[2] for c in checked]
    candidates = _check_candidates(candidates, checked)
    _check_chains_fit(large[0], max([n for n in ns if n > MAX_N], default=0),
                      neighbors if candidates is None else _cand_columns(candidates))
    out = [None] * len(checked)
    status, nodes = np.full(len(checked), 2, dtype=np.int64), np.zeros(len(checked), dtype=np.int64)
    for tri, sel in _split(ns):
        r, k, it = large if tri else small
        res, st, nd = _solve([checked[i] for i in sel], index[sel], tri=tri, restarts=r, kicks=k, seed=seed,
                             init_tours=None if init_tours is None else [init_tours[i] for i in sel],
                             lower_bound=lower_bound, device=device, lb_iters=it, chunk=chunk, timings=timings,
                             t0=t0 if not tri else time.perf_counter(), exact=None if tri else bb, neighbors=neighbors,
                             candidates=None if candidates is None else [candidates[i] for i in sel])
        for i, x in zip(sel, res):
            out[i] = x
        if st is not None:
            status[sel], nodes[sel] = st, nd
    if bb is not None:
        _bb_stats(stats, status, nodes, timings.get("exact", 0.0) - before)
    return out


def solve(Ma, Mw, **kw):
    """The reference's contract (dataset.py:9-50): the tour as a list, or None when the best tour found needs an edge
    absent from Ma.  Keyword arguments (restarts, kicks, seed, neighbors, ...) go to label_tours."""
    r = label_tours([(Ma, Mw)], lower_bound=False, **kw)[0]
    return r.tour if r.feasible else None


def certify(results, dev=0.02):
    """Which labels are provably right for the target create_batch feeds (instance_loader.py:70-73).

    results: a list of TourResult, or create_dataset's summary (its 'cost', 'lb', 'target', 'feasible' arrays).
    With Q = target: the label-0 copy, fed (1-dev) Q, is certified iff lb > (1-dev) Q (no tour is that short); the
    label-1 copy, fed (1+dev) Q, iff the tour is feasible and cost <= (1+dev) Q.
    Returns a dict of bool arrays 'label0', 'label1', 'both' and the float 'fraction' (of 'both')."""
    if isinstance(results, dict):
        cost, lb, Q, feas = (np.asarray(results[k], dtype=np.float64) for k in ("cost", "lb", "target", "feasible"))
        feas = feas.astype(bool)
    else:
        cost = np.array([r.cost for r in results], dtype=np.float64)
        lb = np.array([r.lb for r in results], dtype=np.float64)
        Q = np.array([r.target for r in results], dtype=np.float64)
        feas = np.array([r.feasible for r in results], dtype=bool)
    label0 = lb > (1.0 - dev) * Q
    label1 = feas & (cost <= (1.0 + dev) * Q)
    both = label0 & label1
    return {"label0": label0, "label1": label1, "both": both, "fraction": float(both.mean()) if both.size else 1.0}


def floyd_warshall(Mw):
    """All-pairs shortest-path lengths of the complete graph with weights Mw (the reference's networkx closure,
    dataset.py:87-101); the diagonal is 0."""
    D = np.array(Mw, dtype=np.float64, copy=True)
    n = D.shape[0]
    np.fill_diagonal(D, 0.0)
    for k in range(n):
        np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :], out=D)
    np.fill_diagonal(D, 0.0)
    return D


def metric_closure(matrices, device=None, chunk_bytes=1 << 30):
    """floyd_warshall on the GPU, many matrices at once (tspgnn_metric_closure, csrc/tour_closure.hip): the closure the
    reference takes with networkx for 'random' distances (dataset.py:85-101).

    matrices: a list of square arrays, 1 <= n <= CLOSURE_MAX_N = 256, entries finite and >= 0, not necessarily symmetric.
    Everything is checked on the host before the first launch; a failure raises ValueError naming the instance.
    The instances are sorted by n; those of n <= CLOSURE_LDS_MAX_N and the larger ones go to separate launches, so a small
    instance is closed in LDS whatever its neighbours, and a launch holds at most chunk_bytes of matrices (and at least
    one).  Each result equals floyd_warshall of its matrix bit for bit; it never depends on the other instances, on
    chunk_bytes or on the kernel's tier.

    Returns a list of fp64 [n, n] arrays in input order.
    """
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes=%r must be positive" % (chunk_bytes,))
    mats = []
    for k, m in enumerate(matrices):
        a = np.asarray(m, dtype=np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("instance %d: a weight matrix must be square, not %s" % (k, a.shape))
        n = a.shape[0]
        if not 1 <= n <= CLOSURE_MAX_N:
            raise ValueError("instance %d: n=%d is outside the closure kernel's range [1, %d]" % (k, n, CLOSURE_MAX_N))
        if not np.all(np.isfinite(a)) or a.min() < 0:
            raise ValueError("instance %d: weights must be finite and non-negative" % k)
        mats.append(a)
    out = [None] * len(mats)
    if not mats:
        return out
    ns = np.array([a.shape[0] for a in mats], dtype=np.int32)
    order = np.argsort(ns, kind="stable")
    # lists of positions in `mats`: one tier each, ascending n, at most chunk_bytes
    launches = (_byte_chunks(order[ns[order] <= CLOSURE_LDS_MAX_N], ns, chunk_bytes)
                + _byte_chunks(order[ns[order] > CLOSURE_LDS_MAX_N], ns, chunk_bytes))
    dev = _device(device)
    with torch.cuda.device(dev):
        st = _lib.current_stream()
        for sel in launches:
            n_sel = ns[sel]
            sq = n_sel.astype(np.int64) ** 2
            off = np.concatenate([[0], np.cumsum(sq)[:-1]]).astype(np.int64)
            d_D = torch.from_numpy(np.concatenate([mats[p].reshape(-1) for p in sel])).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            d_n = torch.from_numpy(np.ascontiguousarray(n_sel)).to(dev)
            _lib.call("tspgnn_metric_closure", _lib.ptr(d_D), _lib.ptr(d_off), _lib.ptr(d_n), len(sel),
                      int(n_sel.max()), st)
            flat = d_D.cpu().numpy()
            for p, o, n in zip(sel, off, n_sel):
                out[p] = flat[o:o + int(n) * int(n)].reshape(int(n), int(n)).copy()
    return out


def _check_closure(closure):
    if closure not in ("host", "device"):
        raise ValueError("closure=%r must be 'host' or 'device'" % (closure,))


def _closes(distances, metric):
    """Whether create_graph takes the metric closure of these weights (dataset.py:85)."""
    return bool(metric) and distances != "euc_2D"


def _close_on_device(graphs, idx, device, timings):
    """closure='device': close the weights of graphs[i], i in idx, which _draw_graph left open, in one metric_closure
    call; its wall seconds (transfers included, device-synchronised) are added to timings['closure']."""
    if not len(idx):
        return
    t0 = time.perf_counter()
    closed = metric_closure([graphs[i][1] for i in idx], device=device)
    for i, Mw in zip(idx, closed):
        graphs[i] = (graphs[i][0], Mw) + tuple(graphs[i][2:])
    _add_time(timings, "closure", time.perf_counter() - t0)


def _draw_graph(n, connectivity, distances="euc_2D", metric=True, close=True, timings=None):
    """create_graph's draws (dataset.py:52-108) in the reference's order on the global np.random: the adjacency pairs,
    then the points or the weights, then the planted permutation.  Returns (symmetric Ma, Mw, permutation, nodes).
    close=False leaves the metric closure of Mw to the caller (closure='device'); it draws no random numbers, so the
    stream is the same.  timings: optional dict; the closure's seconds are added to its 'closure'."""
    Ma = np.zeros((n, n))
    Mw = np.zeros((n, n))
    iu = np.triu_indices(n, 1)   # the (i, j > i) loop order of dataset.py:60-64 and :77-81
    adj = (np.random.rand(iu[0].size) < connectivity).astype(np.float64)
    Ma[iu] = adj
    Ma[iu[1], iu[0]] = adj
    nodes = None
    if distances == "euc_2D":
        nodes = np.random.rand(n, 2)
        d = nodes[:, None, :] - nodes[None, :, :]
        sq = d ** 2
        Mw = np.sqrt(sq[..., 0] + sq[..., 1])   # sum() of a 2-vector: (0 + x0) + x1
        np.fill_diagonal(Mw, 0.0)
    elif distances == "random":
        w = np.random.rand(iu[0].size)
        Mw[iu] = w
        Mw[iu[1], iu[0]] = w
    if close and _closes(distances, metric):
        t0 = time.perf_counter()
        Mw = floyd_warshall(Mw)
        _add_time(timings, "closure", time.perf_counter() - t0)
    permutation = [int(x) for x in np.random.permutation(n)]
    for i, j in zip(permutation, permutation[1:] + permutation[:1]):
        Ma[i, j] = Ma[j, i] = 1
    return Ma, Mw, permutation, nodes


def create_graph(n, connectivity, distances="euc_2D", metric=True, closure="host", **solve_kw):
    """dataset.py:52-116: a random graph with a planted Hamiltonian cycle, labelled with the best tour found.
    Returns (np.triu(Ma), Mw, route, nodes); raises Exception('Unsolvable') as the reference does when that tour needs an
    absent edge (it cannot here: the planted cycle is the search's first start).  closure: 'host' takes the metric
    closure of non-Euclidean weights with floyd_warshall, 'device' with metric_closure -- the same draws and the same
    bits.  solve_kw go to label_tours."""
    _check_closure(closure)
    graphs = [_draw_graph(n, connectivity, distances, metric, close=closure == "host")]
    if closure == "device" and _closes(distances, metric):
        _close_on_device(graphs, [0], solve_kw.get("device"), None)
    Ma, Mw, perm, nodes = graphs[0]
    solve_kw.setdefault("lower_bound", False)
    r = label_tours([(Ma, Mw)], init_tours=[perm], **solve_kw)[0]
    if not r.feasible:
        raise Exception("Unsolvable")
    return np.triu(Ma), Mw, r.tour, nodes


def draw_instances(nmin, nmax, conn_min=1, conn_max=1, samples=1000, distances="euc_2D", metric=True, closure="host",
                   timings=None, device=None):
    """The instance stream of create_dataset (dataset.py:126-133): per sample random.randint(nmin, nmax), then
    np.random.uniform(conn_min, conn_max), then create_graph's draws.  Returns a list of (Ma, Mw, permutation, nodes).
    closure: where the metric closure of non-Euclidean weights is taken.  'host': floyd_warshall inside each draw.
    'device': the draws run as before with the closure left out -- it consumes no random numbers -- and one
    metric_closure call on ``device`` closes them all afterwards: the same instances bit for bit, the global generators
    in the same state.  With euc_2D or metric=False nothing is closed and the argument changes nothing.
    timings: optional dict; when a closure ran, its wall seconds are added to timings['closure']."""
    _check_closure(closure)
    out = []
    for _ in range(samples):
        n = random.randint(nmin, nmax)
        out.append(_draw_graph(n, np.random.uniform(conn_min, conn_max), distances=distances, metric=metric,
                               close=closure == "host", timings=timings))
    if closure == "device" and _closes(distances, metric):
        _close_on_device(out, range(samples), device, timings)
    return out


def draw_streams(nmin, nmax, conn_min=1, conn_max=1, samples=1000, distances="euc_2D"):
    """draw_instances' random draws without its matrices: per sample random.randint(nmin, nmax), then
    np.random.uniform(conn_min, conn_max), then rand(n (n-1) / 2) (the adjacency pairs, row-major i < j), then
    rand(n, 2) (euc_2D: the points) or rand(n (n-1) / 2) (random: the weights of the pairs), then permutation(n) (the
    planted cycle) -- the same calls in the same order on the same global generators, which it leaves in the state
    draw_instances leaves them.  Builds no n x n array: DeviceDataset.generate turns the streams into matrices on the GPU
    (tspgnn_build_instances).

    Returns a dict of flat arrays: 'n' int32[I]; 'conn' float64[I]; 'adj_u' float64[sum pairs]; 'pts' float64[sum 2 n]
    (x, y interleaved; euc_2D) or 'wts' float64[sum pairs] (random); 'perm' int32[sum n]; and the prefix offsets
    'pair_off' / 'vert_off' int64[I + 1] of an instance's pairs and vertices; 'distances'."""
    if distances not in ("euc_2D", "random"):
        raise ValueError("distances=%r must be 'euc_2D' or 'random'" % (distances,))
    ns = np.empty(samples, dtype=np.int32)
    conn = np.empty(samples, dtype=np.float64)
    adj, second, perm = [], [], []
    for s in range(samples):
        n = random.randint(nmin, nmax)
        ns[s], conn[s] = n, np.random.uniform(conn_min, conn_max)
        pairs = n * (n - 1) // 2
        adj.append(np.random.rand(pairs))
        second.append(np.random.rand(n, 2).reshape(-1) if distances == "euc_2D" else np.random.rand(pairs))
        perm.append(np.random.permutation(n))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.empty(0, dtype=dt)
    n64 = ns.astype(np.int64)
    return {"n": ns, "conn": conn, "adj_u": cat(adj, np.float64),
            "pts" if distances == "euc_2D" else "wts": cat(second, np.float64), "perm": cat(perm, np.int32),
            "pair_off": np.concatenate([[0], np.cumsum(n64 * (n64 - 1) // 2)]).astype(np.int64),
            "vert_off": np.concatenate([[0], np.cumsum(n64)]).astype(np.int64), "distances": distances}


def create_dataset(path, nmin, nmax, conn_min=1, conn_max=1, samples=1000, distances="euc_2D", metric=True,
                   require_certified=None, max_redraw_rounds=20, verbose=False, exact=False, closure="host", writer="host",
                   **solve_kw):
    """dataset.py:118-143: draw ``samples`` instances (the reference's stream), label them on the GPU in batches with
    the planted cycle as a starting tour, and write ``{path}/{i}.graph`` with write_graph.

    require_certified=None | dev: redraw (from the same global RNG, after the whole stream) every instance whose labels
    ``certify(.., dev)`` cannot prove, for at most max_redraw_rounds rounds, then raise RuntimeError if any remain.
    Redrawing BIASES the distribution: it drops the instances whose optimum sits close to the quirk target, which are the
    hardest ones, and the set no longer matches the reference's stream from the first redrawn index on.
    exact=True: label with label_tours(exact=True), the branch and bound for n <= 128 (prove_tours).
    closure: 'host' | 'device', as draw_instances: where the metric closure of non-Euclidean weights is taken, for the
    stream and for every redraw round (one metric_closure call each); the files are the same bytes either way.
    writer: 'host' | 'device': who formats the files.  'host' is the write_graph loop; 'device' uploads each instance's
    np.triu(Ma) as uint8, the fp64 Mw and the tours in chunks and formats the same bytes on the GPU (graph_text.py,
    csrc/graph_text.hip; n >= 4).  It raises ValueError before any launch of the writer when a mask holds a non-zero entry
    other than 1 or a tour is not n entries long.  times['write'] is filled either way; 'device' adds its stages as
    times['write_upload'], ['write_format'] (the two launches), ['write_download'] and ['write_files'].
    solve_kw go to label_tours (restarts, kicks, seed, lb_iters, chunk, device, max_nodes, neighbors); n up to 256.

    Returns a summary dict: samples, n (per instance), cost, lb, target, feasible, gap = (cost - lb) / cost,
    certified_fraction (at require_certified, else 0.02), redrawn (count) and times {'pack', 'search', 'bound', 'write'},
    plus times['closure'] when a metric closure ran (wall seconds; for 'device' synchronised, transfers included);
    with exact=True also proved (per instance: the written tour is proved optimal), nodes (per instance) and
    times['exact'].
    """
    _check_closure(closure)
    if writer not in ("host", "device"):
        raise ValueError("writer=%r must be 'host' or 'device'" % (writer,))
    os.makedirs(path, exist_ok=True)
    times = {}
    graphs = draw_instances(nmin, nmax, conn_min, conn_max, samples, distances, metric, closure=closure, timings=times,
                            device=solve_kw.get("device"))
    solve_kw.setdefault("lower_bound", True)
    proved, nodes = np.zeros(samples, dtype=bool), np.zeros(samples, dtype=np.int64)

    def label(idx, keys):
        if exact:
            stats = {}
            solve_kw.update(exact=True, stats=stats)
        res = label_tours([(graphs[i][0], graphs[i][1]) for i in idx], init_tours=[graphs[i][2] for i in idx],
                          index=keys, timings=times, **solve_kw)
        if exact:
            proved[idx], nodes[idx] = stats["status"] == "proved", stats["nodes"]
        for r in res:
            if not r.feasible:
                raise Exception("Unsolvable")
        return res

    results = label(list(range(samples)), np.arange(samples))
    redrawn = 0
    if require_certified is not None:
        for rnd in range(1, max_redraw_rounds + 1):
            bad = np.nonzero(~certify(results, require_certified)["both"])[0]
            if bad.size == 0:
                break
            for i in bad:
                n = graphs[i][0].shape[0]
                graphs[i] = _draw_graph(n, np.random.uniform(conn_min, conn_max), distances=distances, metric=metric,
                                        close=closure == "host", timings=times)
            if closure == "device" and _closes(distances, metric):
                _close_on_device(graphs, [int(i) for i in bad], solve_kw.get("device"), times)
            redrawn += int(bad.size)
            new = label(list(bad), rnd * samples + bad)
            for i, r in zip(bad, new):
                results[i] = r
        else:
            if not certify(results, require_certified)["both"].all():
                raise RuntimeError("create_dataset: instances still uncertified after %d redraw rounds" % max_redraw_rounds)
    t0 = time.perf_counter()
    if writer == "device":
        from . import graph_text
        stages = {}
        graph_text.write_instances(path, [(g[0], g[1], r.tour) for g, r in zip(graphs, results)],
                                   _device(solve_kw.get("device")), times=stages)
        times.update(("write_" + k, stages.get(k, 0.0)) for k in ("upload", "format", "download", "files"))
    else:
        for i, (g, r) in enumerate(zip(graphs, results)):
            write_graph(np.triu(g[0]), g[1], filepath="{}/{}.graph".format(path, i), route=r.tour)
            if verbose and samples >= 20 and (i + 1) % (samples // 20) == 0:
                print("Dataset creation {}% complete".format(int(100 * (i + 1) / samples)), flush=True)
    times["write"] = time.perf_counter() - t0
    summary = {
        "samples": samples,
        "n": np.array([g[0].shape[0] for g in graphs]),
        "cost": np.array([r.cost for r in results]),
        "lb": np.array([r.lb for r in results]),
        "target": np.array([r.target for r in results]),
        "feasible": np.array([r.feasible for r in results]),
        "redrawn": redrawn,
        "times": times,
    }
    if exact:
        summary["proved"], summary["nodes"] = proved, nodes
    summary["gap"] = (summary["cost"] - summary["lb"]) / np.where(summary["cost"] > 0, summary["cost"], 1.0)
    summary["certified_fraction"] = certify(summary, 0.02 if require_certified is None else require_certified)["fraction"]
    return summary
