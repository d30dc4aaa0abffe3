"""A plain NumPy restatement of tspgnn_tour_from_votes (include/tspgnn.h): key, sort, one union-find pass over the sorted
edges, stitch, canonical form, n_missing, and the fp32 cost summed in tour order with np.float32 additions.  It shares
one thing with the package, the key (tspgnn.decode.vote_key), so that the key has one owner; test_decode_host.py states
the key's outcomes literally."""
import numpy as np

from tspgnn.decode import vote_key


def edge_order(votes):
    """Edge ids in the decoder's order: larger key first, equal keys by ascending id."""
    key = vote_key(votes).astype(np.int64)
    return np.lexsort((np.arange(len(key)), -key))


def greedy_sorted(n, uv, votes):
    """The chosen edges (ids, in the order chosen): one pass over the sorted list with a union-find."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    deg = [0] * n
    chosen = []
    for e in edge_order(votes):
        a, b = int(uv[e][0]), int(uv[e][1])
        if not (0 <= a < n and 0 <= b < n) or a == b:
            continue
        if deg[a] >= 2 or deg[b] >= 2:
            continue
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        parent[rb] = ra
        deg[a] += 1
        deg[b] += 1
        chosen.append(int(e))
    return chosen


def greedy_rounds(n, uv, votes):
    """The same edges by the definition itself: per round the first edge, in the order, that is eligible NOW (components
    by relabelling, no union-find, no sorted pass)."""
    key = vote_key(votes)
    comp = list(range(n))
    deg = [0] * n
    chosen = []
    while True:
        best = None
        for e in range(len(key)):
            a, b = int(uv[e][0]), int(uv[e][1])
            if not (0 <= a < n and 0 <= b < n) or a == b:
                continue
            if deg[a] >= 2 or deg[b] >= 2 or comp[a] == comp[b]:
                continue
            if best is None or key[e] > key[best]:   # ascending e: a strict > keeps the smaller id
                best = e
        if best is None:
            return chosen
        a, b = int(uv[best][0]), int(uv[best][1])
        ca, cb = comp[a], comp[b]
        comp = [ca if c == cb else c for c in comp]
        deg[a] += 1
        deg[b] += 1
        chosen.append(best)


def stitch(n, uv, chosen):
    """The paths of the chosen edges (each from its smaller endpoint, ordered by smallest vertex), and their
    concatenation."""
    nb = [[] for _ in range(n)]
    for e in chosen:
        a, b = int(uv[e][0]), int(uv[e][1])
        nb[a].append(b)
        nb[b].append(a)
    paths = []
    seen = [False] * n
    for s in range(n):          # ascending: an endpoint met first is the smaller one of its path
        if seen[s] or len(nb[s]) == 2:
            continue
        path, prev, cur = [s], -1, s
        seen[s] = True
        while True:
            nxt = [x for x in nb[cur] if x != prev]
            if not nxt:
                break
            prev, cur = cur, nxt[0]
            seen[cur] = True
            path.append(cur)
        paths.append(path)
    assert all(seen), "the chosen edges hold a cycle"
    paths.sort(key=min)
    return paths, [v for p in paths for v in p]


def canonical(seq):
    n = len(seq)
    p0 = seq.index(0)
    rot = seq[p0:] + seq[:p0]
    if rot[1] > rot[n - 1]:
        rot = [rot[0]] + rot[1:][::-1]
    return rot


def decode_instance(n, uv, w, votes, rounds=False):
    """-> (tour list, n_missing, cost np.float32, fragments) of one instance: uv [m, 2] local ids, w [m] weights."""
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    votes = np.asarray(votes, dtype=np.float32).reshape(-1)
    chosen = (greedy_rounds if rounds else greedy_sorted)(n, uv, votes)
    paths, seq = stitch(n, uv, chosen)
    tour = canonical(seq)
    first = {}
    for e in range(len(uv)):    # ascending: the smallest edge id joining a pair
        a, b = int(uv[e][0]), int(uv[e][1])
        if 0 <= a < n and 0 <= b < n and a != b:
            first.setdefault((min(a, b), max(a, b)), e)
    cost, missing = np.float32(0), 0
    for a, b in zip(tour, tour[1:] + tour[:1]):
        e = first.get((min(a, b), max(a, b)))
        if e is None:
            missing += 1
        else:
            cost = np.float32(cost + w[e])
    return tour, missing, cost, len(paths)


def decode_batch(case):
    """Per instance of a decode_cases case -> [(tour, n_missing, cost, fragments)]."""
    out = []
    for b in range(len(case["n"])):
        e0, e1 = case["seg"][b], case["seg"][b + 1]
        out.append(decode_instance(int(case["n"][b]), case["uv"][e0:e1] - case["vseg"][b], case["wc"][e0:e1, 0],
                                   case["vote"][e0:e1]))
    return out
