"""Classical baselines for the decision TSP: a nearest-neighbour tour and simulated annealing over 2-exchange moves.

The reference compares its trained model with "a predictor for the decision TSP obtained from the solutions yielded by 1) a
Nearest Neighbor strategy and 2) a Simulated Annealing strategy (2-exchange)" (figures/test_varying_dev_baseline.png) and
ships no code for either.  Here both are HIP kernels (csrc/tour_baselines.hip: ``tspgnn_tour_nearest_neighbor`` and
``tspgnn_tour_anneal``, with ``_tri`` entry points for n 129-256), and the predictor is ``decide``: answer yes iff the
heuristic's tour is feasible and costs no more than the target.  ``experiments.baseline_curve`` draws the curve.

Both solvers take what ``dataset.label_tours`` takes -- the same checks, the same penalised packing, n < 4 on the host,
the split at 128 between the square and the triangle kernels -- and return ``TourResult``s with ``lb = nan``.
"""
import time

import numpy as np
import torch

from . import _lib
from .dataset import (DEFAULT_CHUNK, MAX_N, MAX_N_TRI, _add_time, _check_chains_fit, _device, _finish, _pack, _spans,
                      _split, _upload, _validate)

# Annealing defaults, chosen from the t_hot x sweeps grid of DESIGN.md §12 (2^10 instances at n 20-40, 80 and 200 on the
# MI355X).  Temperatures are multiples of the instance's mean real edge weight, and a level runs sweeps * n^2 proposals.
# t_hot = 0.1 with sweeps = 4 had the highest tpr at dev 0.02 at every shape (0.984 / 0.995 / 0.990) and the smallest
# median gap to label_tours (0 / 0.28 % / 0.92 %); halving either loses 1-9 points at n 200.  The kernel time, 4 ms /
# 16 ms / 0.22 s per 2^10 instances, stays below the host's packing time, so the cheaper settings buy nothing.
DEFAULT_CHAINS = 4
DEFAULT_LEVELS = 32
DEFAULT_SWEEPS = 4
DEFAULT_T_HOT = 0.1
DEFAULT_T_COLD = 0.002
MAX_PROPOSALS = 2 ** 31 - 1


def nearest_neighbor_tours(instances, start=0, device=None, chunk=DEFAULT_CHUNK):
    """The nearest-neighbour tour of every instance: from the start vertex, always on to the closest unvisited vertex
    (ties to the smaller id; an edge absent from Ma costs the penalty of label_tours, so it is taken last).

    instances: list of (Ma, Mw) as for label_tours, n up to 256.  start: a vertex id (taken modulo n), or "best" to run
    every start vertex and keep the shortest tour (fp32 cost, ties to the smaller start).  chunk: instances per launch.
    Returns a list of TourResult with lb = nan."""
    if isinstance(start, str):
        if start != "best":
            raise ValueError("start=%r must be a vertex id or 'best'" % (start,))
        s = -1
    else:
        s = int(start)
        if s != start or not 0 <= s < 2 ** 31:
            raise ValueError("start=%r must be a non-negative vertex id or 'best'" % (start,))
    checked, _ = _validate(instances, 1, 0, 1, chunk, None, None, MAX_N_TRI)
    out = [None] * len(checked)
    for tri, sel in _split([c[2] for c in checked]):
        pk = _pack([checked[i] for i in sel], tri)
        res = pk.out
        if pk.big:
            dev = _device(device)
            entry = "tspgnn_tour_nearest_neighbor_tri" if tri else "tspgnn_tour_nearest_neighbor"
            with torch.cuda.device(dev):
                d = _upload(pk, dev)
                st = _lib.current_stream()
                for c0, c1 in _spans(len(pk.big), chunk):
                    _lib.call(entry, _lib.ptr(d.W), _lib.ptr(d.w_off[c0:c1]), _lib.ptr(d.n[c0:c1]),
                              _lib.ptr(d.t_off[c0:c1]), c1 - c0, int(pk.ns[c0:c1].max()), s, _lib.ptr(d.tours),
                              _lib.ptr(d.cost[c0:c1]), st)
                tours = d.tours.cpu().numpy().astype(np.int64)
            res = _finish(pk, tours)
        for i, x in zip(sel, res):
            out[i] = x
    return out


def geometric_schedule(levels, t_hot, t_cold):
    """[levels] temperatures from t_hot down to t_cold in equal ratios (levels = 1: t_hot alone)."""
    if levels < 0:
        raise ValueError("levels=%d must not be negative" % levels)
    for name, t in (("t_hot", t_hot), ("t_cold", t_cold)):
        if not (t >= 0 and np.isfinite(t)):   # NaN fails the comparison
            raise ValueError("%s=%r must be a finite, non-negative temperature" % (name, t))
    if t_cold > t_hot:
        raise ValueError("t_cold=%r exceeds t_hot=%r" % (t_cold, t_hot))
    if t_cold == 0 and t_hot > 0 and levels > 1:
        raise ValueError("a geometric schedule cannot reach t_cold = 0; pass inv_temp with inf entries for T = 0")
    if levels == 0:
        return np.zeros(0)
    if levels == 1 or t_hot == 0:
        return np.full(levels, float(t_hot))
    return t_hot * (t_cold / t_hot) ** (np.arange(levels) / (levels - 1.0))


def anneal_tours(instances, chains=DEFAULT_CHAINS, levels=DEFAULT_LEVELS, sweeps=DEFAULT_SWEEPS, t_hot=DEFAULT_T_HOT,
                 t_cold=DEFAULT_T_COLD, seed=0, init_tours=None, index=None, inv_temp=None, per_level=None, device=None,
                 chunk=DEFAULT_CHUNK, timings=None):
    """Simulated annealing over 2-exchange moves (Metropolis acceptance), many instances at once.

    instances, init_tours, index, seed, device, chunk: as for label_tours (n up to 256).  chains: wave64 chains per
    instance (1..16; for n > 128 at most dataset.tri_chains_fit(largest n)).  Chain 0 starts from the instance's init_tours entry
    when there is one, otherwise from the nearest-neighbour tour from vertex 0; chain c from the one from vertex c % n.
    The default schedule has ``levels`` temperatures, geometric from t_hot to t_cold, both multiples of the instance's mean
    real edge weight, and sweeps * n^2 proposals per level.  inv_temp ([levels] or [len(instances), levels], 1 / T, inf
    for T = 0) and per_level (an int or one per instance) override it.  levels * per_level may not exceed 2^31 - 1.
    A result depends on (seed, its index, chains, its schedule) only.  timings: optional dict that receives the seconds of
    'pack' and 'anneal'.  Returns a list of TourResult with lb = nan; the tour is the best any chain has seen."""
    t0 = time.perf_counter()
    if chains != int(chains) or not 1 <= chains <= 16:
        raise ValueError("chains=%r must be in [1, 16]" % (chains,))
    chains = int(chains)
    checked, index = _validate(instances, 1, 0, 1, chunk, index, init_tours, MAX_N_TRI)
    B = len(checked)
    _check_chains_fit(chains, max([c[2] for c in checked if c[2] > MAX_N], default=0), None, "chains")
    if inv_temp is None:
        temps = geometric_schedule(int(levels), t_hot, t_cold)
        inv = None
    else:
        inv = np.asarray(inv_temp, dtype=np.float64)
        if inv.ndim == 1:
            inv = np.broadcast_to(inv, (B, inv.shape[0]))
        if inv.ndim != 2 or inv.shape[0] != B:
            raise ValueError("inv_temp must be [levels] or [len(instances), levels]")
        if np.isnan(inv).any() or (inv < 0).any():
            raise ValueError("inv_temp holds a negative or NaN inverse temperature")
    L = len(temps) if inv is None else inv.shape[1]
    ns_all = np.array([c[2] for c in checked], dtype=np.int64)
    if per_level is None:
        if not (sweeps >= 0 and np.isfinite(sweeps)):
            raise ValueError("sweeps=%r must be finite and non-negative" % (sweeps,))
        per = np.floor(sweeps * ns_all.astype(np.float64) ** 2).astype(np.int64)
    else:
        per = np.broadcast_to(np.asarray(per_level, dtype=np.int64), (B,)).copy()
        if (per < 0).any():
            raise ValueError("per_level must not be negative")
    if B and int(per.max()) * L > MAX_PROPOSALS:
        raise ValueError("levels * per_level = %d exceeds the limit of %d proposals per chain"
                         % (int(per.max()) * L, MAX_PROPOSALS))
    out = [None] * B
    for tri, sel in _split(ns_all):
        t_pack = time.perf_counter()
        pk = _pack([checked[i] for i in sel], tri, None if init_tours is None else [init_tours[i] for i in sel],
                   mean_weight=inv is None)
        res = pk.out
        if pk.big:
            big = np.array(sel)[pk.big]          # positions in `instances`, in launch order
            G = len(big)
            if inv is None:
                with np.errstate(divide="ignore"):
                    inv32 = (1.0 / (pk.mean_w[:, None] * temps[None, :])).astype(np.float32)
            else:
                inv32 = inv[big].astype(np.float32)
            inv32 = np.ascontiguousarray(inv32).reshape(G, L)
            dev = _device(device)
            entry = "tspgnn_tour_anneal_tri" if tri else "tspgnn_tour_anneal"
            with torch.cuda.device(dev):
                d = _upload(pk, dev, index[sel])
                d_inv = torch.from_numpy(inv32).to(dev)
                d_per = torch.from_numpy(per[big].astype(np.int32)).to(dev)
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                st = _lib.current_stream()
                for c0, c1 in _spans(G, chunk):
                    _lib.call(entry, _lib.ptr(d.W), _lib.ptr(d.w_off[c0:c1]), _lib.ptr(d.n[c0:c1]),
                              _lib.ptr(d.init), _lib.ptr(d.t_off[c0:c1]), _lib.ptr(d.idx[c0:c1]),
                              _lib.ptr(d_inv[c0:c1]) if L else None, _lib.ptr(d_per[c0:c1]), c1 - c0,
                              int(pk.ns[c0:c1].max()), chains, L, int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(d.tours),
                              _lib.ptr(d.cost[c0:c1]), st)
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                tours = d.tours.cpu().numpy().astype(np.int64)
            res = _finish(pk, tours)
            _add_time(timings, "pack", t1 - t_pack)
            _add_time(timings, "anneal", t2 - t1)
        for i, x in zip(sel, res):
            out[i] = x
    for key, seconds in (("pack", 0.0), ("anneal", 0.0), ("total", time.perf_counter() - t0)):   # every key, always
        _add_time(timings, key, seconds)
    return out


def decide(results, targets):
    """The baseline's answer to "is there a tour of cost at most C?": yes iff its tour is feasible and costs no more than
    C.  results: a list of TourResult; targets: one C per result (or one for all).  Returns a bool array."""
    cost = np.array([r.cost for r in results], dtype=np.float64)
    feas = np.array([r.feasible for r in results], dtype=bool)
    C = np.broadcast_to(np.asarray(targets, dtype=np.float64), cost.shape)
    return feas & (cost <= C)
