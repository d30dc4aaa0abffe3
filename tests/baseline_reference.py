"""NumPy / Python-int reference of the two decision-TSP baselines (csrc/tour_baselines.hip), for the tests.

Both run on the packed fp32 matrix the kernels get (dataset._penalised).  The nearest-neighbour reference is exact: it
only compares fp32 values.  The annealing reference is the sequential chain of include/tspgnn.h, one proposal after the
other, with fp32 d, d * inv_temp and rel; its one inexact step is exp(), so it also counts the near ties -- uphill
decisions with |exp(-x) - u| <= 1e-5 max(exp(-x), u), about 40 times expf's error bound -- and a test asserts that its
seeds have none."""
import math

import numpy as np

from tspgnn import dataset

M64 = (1 << 64) - 1
NEAR_TIE = 1e-5


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, inst, chain, kick, k):
    h = mix64((seed & M64) ^ mix64(inst & M64))
    h = mix64(h ^ (((chain & 0xffffffff) << 32) | (kick & 0xffffffff)))
    return mix64(h ^ (k & 0xffffffff))


def packed(Ma, Mw):
    """The dense fp32 matrix of one instance, as the kernels see it (both layouts hold these values)."""
    A = dataset._edge_mask(Ma)[None]
    return dataset._penalised(A, np.asarray(Mw, dtype=np.float64)[None])[0]


def canonical(tour):
    tour = [int(v) for v in tour]
    k = tour.index(0)
    t = tour[k:] + tour[:k]
    if t[1] > t[-1]:
        t = [0] + t[1:][::-1]
    return t


def cost64(W32, tour):
    """fp64 cost of a tour under the packed fp32 weights."""
    t = np.asarray(tour)
    return float(W32[t, np.roll(t, -1)].astype(np.float64).sum())


def nn_tours(W32, starts):
    """Nearest-neighbour tours from every vertex of ``starts`` at once (not yet canonical): to the unvisited vertex of
    smallest W(cur, v), ties to the smaller id (np.argmin returns the first minimum)."""
    n = W32.shape[0]
    starts = np.asarray(starts, dtype=np.int64)
    S = np.arange(len(starts))
    tours = np.empty((len(starts), n), dtype=np.int64)
    seen = np.zeros((len(starts), n), dtype=bool)
    cur = starts.copy()
    tours[:, 0] = cur
    seen[S, cur] = True
    for k in range(1, n):
        rows = np.where(seen, np.float32(np.inf), W32[cur])
        cur = rows.argmin(axis=1)
        tours[:, k] = cur
        seen[S, cur] = True
    return tours


def nn_tour(W32, start):
    return [int(v) for v in nn_tours(W32, [start])[0]]


def chain(W32, start_tour, seed, index, chain_id, inv_temp, per_level):
    """The sequential annealing chain.  Returns (its best tour, not yet canonical; the count of near ties)."""
    n = W32.shape[0]
    t = [int(v) for v in start_tour]
    best = list(t)
    inv_temp = np.asarray(inv_temp, dtype=np.float32)
    rel = np.float32(0)
    best_rel = np.float32(0)
    near = 0
    with np.errstate(over="ignore"):
        for p in range(len(inv_temp) * int(per_level)):
            r = draw(seed, index, chain_id, p, 0)
            i, j = (r & 0xffff) % n, ((r >> 16) & 0xffff) % n
            if i > j:
                i, j = j, i
            if not (j > i + 1 and not (i == 0 and j == n - 1)):
                continue
            a, b, c, e = t[i], t[i + 1], t[j], t[(j + 1) % n]
            d = np.float32(np.float32(W32[a, c] + W32[b, e]) - np.float32(W32[a, b] + W32[c, e]))
            if not d <= 0:
                u = (((r >> 40) & 0x7fffff) + 0.5) * 2.0 ** -23
                x = np.float32(d * inv_temp[p // per_level])
                ex = math.exp(-float(x))
                if abs(ex - u) <= NEAR_TIE * max(ex, u):
                    near += 1
                if not u < ex:
                    continue
            t[i + 1:j + 1] = t[i + 1:j + 1][::-1]
            rel = np.float32(rel + d)
            if rel < best_rel:
                best_rel = rel
                best = list(t)
    return best, near


def anneal(W32, seed, index, chains, inv_temp, per_level, init=None):
    """Every chain's best tour, canonical, and the total count of near ties.  Chain 0 starts from ``init`` when given,
    otherwise from the nearest-neighbour tour from vertex 0; chain c from the one from vertex c % n."""
    n = W32.shape[0]
    tours, near = [], 0
    for c in range(chains):
        start = list(init) if (c == 0 and init is not None) else nn_tour(W32, c % n)
        best, k = chain(W32, start, seed, index, c, inv_temp, per_level)
        tours.append(canonical(best))
        near += k
    return tours, near


def euclidean(rng, n):
    p = rng.rand(n, 2)
    return np.triu(np.ones((n, n)), 1), np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))


def grid(rng, n):
    """Integer-grid points: many pairs at exactly the same distance, so the tie rules act."""
    side = max(3, int(math.ceil(math.sqrt(n))))
    p = rng.randint(0, side, size=(n, 2)).astype(np.float64)
    return np.triu(np.ones((n, n)), 1), np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))


def sparse_planted(rng, n):
    """A sparse graph with a planted Hamiltonian cycle: most pairs carry the penalty weight."""
    Ma, Mw = euclidean(rng, n)
    Ma = np.triu((rng.rand(n, n) < 0.3).astype(float), 1)
    perm = [int(x) for x in rng.permutation(n)]
    for i, j in zip(perm, perm[1:] + perm[:1]):
        Ma[min(i, j), max(i, j)] = 1
    return Ma, Mw
