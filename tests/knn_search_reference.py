"""NumPy restatement of the candidate-list tour search (tspgnn_tour_search_knn, csrc/tour_search.hip), for the tests.

It works on the packed fp32 matrix the kernels get and restates the definition of include/tspgnn.h as sets: the
neighbour sets N(x) by the key (w(x, y), y), the pair set S, every move of the full neighbourhood with its fp32 delta
(the kernel's parenthesisation) and its 32-bit code over whole (i, j) grids, a mask from S, and the argmin of
(delta, code).  Nothing here follows the kernel's enumeration.  The chain around it (double-bridge kicks keyed on the
generator, acceptance on the fp32 cost summed in the kernel's order) is restated exactly.

The one inexact step is the stop rule best < -1e-6 * cost / n: the kernel's cost is fp32, this one's fp64, about 1e-6
apart.  Every scan records margin = |best + thr| / thr; while the smallest stays far above 1e-6 both sides decide alike.
"""
import functools

import numpy as np

from baseline_reference import canonical, cost64, draw, euclidean, nn_tour, packed, sparse_planted

EPS_REL = float(np.float32(1e-6))
OR_OPT = 1 << 30


def neighbor_sets(W32, K):
    """[n, min(K, n-1)] ids: row x = the vertices y != x smallest by (w(x, y), y)."""
    n = W32.shape[0]
    kk = min(K, n - 1)
    out = np.empty((n, kk), dtype=np.int64)
    ids = np.arange(n)
    for x in range(n):
        order = np.lexsort((ids, W32[x]))
        out[x] = order[order != x][:kk]
    return out


def pair_mask(W32, K):
    """S as a symmetric [n, n] bool matrix."""
    n = W32.shape[0]
    S = np.zeros((n, n), dtype=bool)
    S[np.arange(n)[:, None], neighbor_sets(W32, K)] = True
    return S | S.T


def scan(W, S, t):
    """The best candidate of tour t: (fp32 delta, code), or (inf, None) when there is none.  S=None: every move."""
    n = len(t)
    t = np.asarray(t)
    I, J = np.arange(n)[:, None], np.arange(n)[None, :]
    t1 = np.roll(t, -1)
    ds, cs = [], []

    def keep(d, code, valid, e1, e2):
        m = valid if S is None else valid & (S[e1] | S[e2])
        ds.append(d[m])
        cs.append(np.broadcast_to(code, d.shape)[m])

    a, b, c, e = t[I], t1[I], t[J], t1[J]
    d = (W[a, c] + W[b, e]) - (W[a, b] + W[c, e])
    keep(d, (I << 8) | J, (J > I + 1) & ~((I == 0) & (J == n - 1)), (a, c), (b, e))
    for L in range(1, min(3, n - 3) + 1):
        rel = (J - I) % n
        valid = (rel >= L) & (rel <= n - 2)
        prev, s0, sl, nx = t[(I - 1) % n], t[I], t[(I + L - 1) % n], t[(I + L) % n]
        a, b = t[J], t1[J]
        gain = W[prev, nx] - (W[prev, s0] + W[sl, nx])
        ab = W[a, b]
        code = OR_OPT | (L << 26) | (I << 8) | J
        keep(gain + ((W[a, s0] + W[sl, b]) - ab), code, valid, (a, s0), (sl, b))
        if L > 1:
            keep(gain + ((W[a, sl] + W[s0, b]) - ab), code | (1 << 29), valid, (a, sl), (s0, b))
    d, c = np.concatenate(ds), np.concatenate(cs)
    assert d.dtype == np.float32
    if d.size == 0:
        return np.float32(np.inf), None
    best = d.min()
    return best, int(c[d == best].min())


def apply_move(t, code):
    n = len(t)
    i, j = (code >> 8) & 0xff, code & 0xff
    if not code & OR_OPT:
        return t[:i + 1] + t[i + 1:j + 1][::-1] + t[j + 1:]
    L, rv = (code >> 26) & 3, (code >> 29) & 1
    seg = [t[(i + k) % n] for k in range(L)]
    rel = (j - i) % n
    head = [t[(i + L + k) % n] for k in range(rel - L + 1)]
    tail = [t[(i + k) % n] for k in range(rel + 1, n)]
    return head + (seg[::-1] if rv else seg) + tail


def cost32(W, t):
    """The kernel's fp32 tour cost: lane l sums the edges l, l + 64, ... in order, then a xor butterfly over the lanes."""
    t = np.asarray(t)
    w = W[t, np.roll(t, -1)]
    acc = np.zeros(64, dtype=np.float32)
    for r in range(0, len(t), 64):
        part = w[r:r + 64]
        acc[:len(part)] = acc[:len(part)] + part
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
    return acc[0]


def descend(W, S, t, log):
    """The descent from tour t (a list); log['margin'] keeps the smallest |best + thr| / thr, log['scans'] counts."""
    n = len(t)
    for _ in range(4 * n * n):
        best, code = scan(W, S, t)
        thr = EPS_REL * cost64(W, t) / n
        log["scans"] = log.get("scans", 0) + 1
        if np.isfinite(best):
            log["margin"] = min(log.get("margin", np.inf), abs(float(best) + thr) / thr)
        if not float(best) < -thr:
            break
        t = apply_move(t, code)
    return t


def double_bridge(t, r):
    n = len(t)
    x1 = 1 + (r & 0xffffff) % (n - 1)
    x2 = 1 + ((r >> 24) & 0xffffff) % (n - 2)
    x3 = 1 + ((r >> 48) & 0xffff) % (n - 3)
    if x2 >= x1:
        x2 += 1
    lo, hi = min(x1, x2), max(x1, x2)
    if x3 >= lo:
        x3 += 1
    if x3 >= hi:
        x3 += 1
    p1, p2, p3 = sorted((lo, hi, x3))
    return t[:p1] + t[p2:p3] + t[p1:p2] + t[p3:]


def chain0(W, K, init, kicks, seed, index):
    """Chain 0 of the search from the tour ``init``: [canonical best tour after 0, 1, ..., kicks kicks], and the log.
    K=None is the full scan."""
    S = None if K is None else pair_mask(W, K)
    log = {}
    cur = descend(W, S, [int(v) for v in init], log)
    best = cost32(W, cur)
    out = [canonical(cur)]
    for kick in range(kicks):
        work = descend(W, S, double_bridge(cur, draw(seed, index, 0, kick, 0)), log)
        c = cost32(W, work)
        if c <= best:
            cur, best = work, c
        out.append(canonical(cur))
    return out, log


# ---------------------------------------------------------------- the instances of the restricted-neighbourhood GPU test
SQUARE_N = (8, 40, 64, 65, 128)
TRI_N = (65, 129, 200, 256)
KS = (1, 5, 10)
KICKS = (0, 3)
SEED = 11


@functools.lru_cache(maxsize=None)
def instance(layout, n):
    """(Ma, Mw, init tour) of the case (layout, n): Euclidean, the square n = 40 a sparse planted graph; from a random
    permutation up to n = 65, from the nearest-neighbour tour above (a shorter descent for the host side)."""
    rng = np.random.RandomState(1000 * (layout == "tri") + n)
    Ma, Mw = sparse_planted(rng, n) if (layout, n) == ("square", 40) else euclidean(rng, n)
    init = [int(v) for v in rng.permutation(n)] if n <= 65 else nn_tour(packed(Ma, Mw), int(rng.randint(n)))
    return Ma, Mw, init


@functools.lru_cache(maxsize=None)
def expected(layout, n, K):
    """The restatement's tours after each kick count of 0..max(KICKS) for the case, and its log.  A layout's instances
    share a launch in the order of SQUARE_N / TRI_N, which is their generator index."""
    Ma, Mw, init = instance(layout, n)
    return chain0(packed(Ma, Mw), K, init, max(KICKS), SEED, (TRI_N if layout == "tri" else SQUARE_N).index(n))
