"""NumPy restatements for the vote-guided tour search, written from the definitions in include/tspgnn.h:

vote_rows             tspgnn_vote_neighbors: per vertex the pairs its CSR row joins (the smallest edge id per pair), then
                      k_vote picks by (vote key descending, y ascending) and k_near picks by (weight ascending, y ascending)
                      among the rest, rows padded with the vertex itself.  Plain loops and Python's sort; the vote key is
                      the package's (tspgnn.decode.vote_key, one owner), the weight order is restated here.
pair_mask_from_table  the pair set S of tspgnn_tour_search_cand from a table.
chain0_table          chain 0 of that search: knn_search_reference's descend / double_bridge / cost32 over that S.

vertex_csr builds the vertex CSR of a decode_cases batch from the valid endpoints, as the tests feed it to the kernel.
table / expected are the tables and the restatement's tours of the GPU comparison, on knn_search_reference's instances.
"""
import functools

import numpy as np

import decode_cases
import knn_search_reference as knn
from baseline_reference import canonical, draw, packed
from knn_search_reference import cost32, descend, double_bridge
from tspgnn import dataset
from tspgnn.decode import vote_key


def weight_key(w):
    """Ascending order of fp32 weights as uint32: the order-preserving image of the bits, a NaN after everything."""
    bits = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)
    key = np.where((bits & np.uint32(0x80000000)) != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    key[(bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return key


def vertex_csr(case):
    """(rowptr [N+1], eid) int32 of a decode_cases batch: row g lists, ascending, the edges one of whose endpoints is the
    global vertex g (an endpoint outside 0..N-1 is listed nowhere; a self-loop is listed once)."""
    N = int(case["vseg"][-1])
    rows = [[] for _ in range(N)]
    for e, (a, b) in enumerate(np.asarray(case["uv"]).reshape(-1, 2)):
        for g in sorted({int(a), int(b)}):
            if 0 <= g < N:
                rows[g].append(e)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    eid = np.array([e for r in rows for e in r], dtype=np.int32)
    return rowptr, eid


def vote_rows(uv, wc, seg, vseg, rowptr, eid, vote, k_vote, k_near):
    """uint8 [N, k_vote + k_near]: tspgnn_vote_neighbors on the batch arrays (global endpoint ids, wc column 0 the
    weight).  An instance with n outside [4, 256] gets zero rows."""
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    wc = np.asarray(wc, dtype=np.float32).reshape(-1, 2)
    vk = vote_key(np.asarray(vote, dtype=np.float32).reshape(-1)).astype(np.int64) if len(uv) else np.zeros(0, np.int64)
    wk = weight_key(wc[:, 0]).astype(np.int64) if len(uv) else np.zeros(0, np.int64)
    K = k_vote + k_near
    tab = np.zeros((int(vseg[-1]), K), dtype=np.uint8)
    for b in range(len(seg) - 1):
        v0, n = int(vseg[b]), int(vseg[b + 1] - vseg[b])
        if not 4 <= n <= 256:
            continue
        for x in range(n):
            first = {}      # y -> e(x, y)
            for e in eid[rowptr[v0 + x]:rowptr[v0 + x + 1]]:
                e = int(e)
                if not seg[b] <= e < seg[b + 1]:
                    continue
                a, c = int(uv[e][0]) - v0, int(uv[e][1]) - v0
                y = c if a == x else a if c == x else None
                if y is None or y == x or not 0 <= y < n:
                    continue
                first[y] = min(first.get(y, e), e)
            # both orders are strict and total, so "the first of those left, K times" is a prefix of the sorted list
            by_vote = sorted(first, key=lambda y: (-vk[first[y]], y))[:k_vote]
            by_weight = [y for y in sorted(first, key=lambda y: (wk[first[y]], y)) if y not in by_vote][:k_near]
            row = by_vote + [x] * (k_vote - len(by_vote)) + by_weight + [x] * (k_near - len(by_weight))
            tab[v0 + x] = row
    return tab


def case_rows(case, k_vote, k_near):
    """vote_rows of a decode_cases batch, with the CSR of vertex_csr."""
    rowptr, eid = vertex_csr(case)
    return vote_rows(case["uv"], case["wc"], case["seg"], case["vseg"], rowptr, eid, case["vote"], k_vote, k_near)


def pair_mask_from_table(tab, n):
    """S as a symmetric [n, n] bool matrix: entry (x, s) = y puts {x, y} into S iff y < n and y != x."""
    tab = np.asarray(tab).reshape(n, -1)
    S = np.zeros((n, n), dtype=bool)
    for x in range(n):
        for y in tab[x]:
            y = int(y)
            if y < n and y != x:
                S[x, y] = S[y, x] = True
    return S


def chain0_table(W, tab, init, kicks, seed, index):
    """Chain 0 of tspgnn_tour_search_cand from the tour ``init``: [canonical best tour after 0, 1, ..., kicks kicks], and
    the log -- knn_search_reference.chain0 with S taken from the table."""
    S = pair_mask_from_table(tab, W.shape[0])
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


# ------------------------------------------------------------------ the tables of the arbitrary-table GPU comparison
TABLES = ("votes_5_0", "votes_3_2", "random", "skip")
KICKS = knn.KICKS
SEED = knn.SEED


def instance_case(Ma, Mw, votes):
    """One (Ma, Mw) instance as a decode_cases batch: its edges in create_batch's order, with the given votes."""
    A = np.triu(dataset._edge_mask(Ma), 1)
    uv = np.stack(np.nonzero(A), axis=1).astype(np.int32)
    w = np.asarray(Mw, dtype=np.float64)[uv[:, 0], uv[:, 1]].astype(np.float32)
    return decode_cases.batch([(Ma.shape[0], uv, w, np.asarray(votes, dtype=np.float32))])


@functools.lru_cache(maxsize=None)
def table(layout, n, kind):
    """uint8 [n, K] for the case (layout, n) of knn_search_reference.instance: the vote rows of random votes at
    (k_vote, k_near) = (5, 0) and (3, 2); a random table of 6 columns with entries >= n, self entries and duplicates
    inside a row; 4 columns of skips."""
    Ma, Mw, _ = knn.instance(layout, n)
    rng = np.random.RandomState(7000 + 10 * n + (layout == "tri"))
    if kind == "skip":
        return np.repeat(np.arange(n, dtype=np.uint8)[:, None], 4, axis=1)
    if kind == "random":
        tab = rng.randint(0, n, size=(n, 6))
        tab[:, 2] = tab[:, 1]                                       # a duplicate in every row
        own = rng.rand(n) < 0.5
        tab[own, 3] = np.arange(n)[own]                             # self entries
        if n < 256:
            tab[:, 4] = rng.randint(n, 256, size=n)                 # entries >= n
        return tab.astype(np.uint8)
    m = int(np.triu(dataset._edge_mask(Ma), 1).sum())
    kv, kn = (5, 0) if kind == "votes_5_0" else (3, 2)
    return case_rows(instance_case(Ma, Mw, rng.randn(m)), kv, kn)


@functools.lru_cache(maxsize=None)
def expected(layout, n, kind):
    """chain0_table's tours after 0 .. max(KICKS) kicks for the case and table, and its log.  A layout's instances share
    a launch in the order of SQUARE_N / TRI_N, which is their generator index."""
    Ma, Mw, init = knn.instance(layout, n)
    index = (knn.TRI_N if layout == "tri" else knn.SQUARE_N).index(n)
    return chain0_table(packed(Ma, Mw), table(layout, n, kind), init, max(KICKS), SEED, index)
