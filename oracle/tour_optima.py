"""Exact optima of symmetric TSP instances with integer weights, on the host: the truth that the tour kernels' bounds and
exact labels are tested against beyond the reach of the Held-Karp DP (tests/test_gpu_tour_optima.py, n up to 256).

TEST INFRASTRUCTURE, host only; scipy is imported inside the functions, so that importing this module needs NumPy alone.

``solve_exact`` is a degree-2 integer program with lazily added subtour cuts on scipy.optimize.milp (HiGHS).  HiGHS stops
at an absolute gap of 1e-6, which scipy does not expose; with integer weights two tours differ by at least 1, so what it
returns is the optimum.

``generate`` writes tests/golden/tour_optima.npz for the cases of tests/tour_optima_cases.py (``python
oracle/gen_golden.py tour_optima``), and ``select`` is the seed search that chose them.  Both run the NumPy restatement
of the branch and bound (tests/test_tour_exact_host.py) with a vectorised 1-tree that picks the same edges in the same
order; neither is run by a test.
"""
import contextlib
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(ROOT, "tests", "golden", "tour_optima.npz")

FREE, FORCED, FORBIDDEN = 0, 1, 2


def _components(n, pairs):
    """Vertex sets of the connected components of the graph (0..n-1, pairs)."""
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for a, b in pairs:
        root[find(a)] = find(b)
    comps = {}
    for v in range(n):
        comps.setdefault(find(v), []).append(v)
    return list(comps.values())


def canonical(tour):
    """The cycle started at vertex 0 with tour[1] < tour[-1], as the kernels write theirs."""
    tour = [int(x) for x in tour]
    k = tour.index(0)
    tour = tour[k:] + tour[:k]
    if len(tour) > 2 and tour[1] > tour[-1]:
        tour = [0] + tour[:0:-1]
    return tour


def solve_exact(K, mask):
    """The shortest Hamiltonian cycle over the edges of ``mask`` (symmetric bool [n, n]) under the integer weights
    K[min(i, j), max(i, j)].  -> (optimum as int, tour as a canonical list), or (None, None) when there is no cycle."""
    from scipy import sparse
    from scipy.optimize import Bounds, LinearConstraint, milp

    K = np.asarray(K)
    if K.dtype.kind not in "iu":
        raise ValueError("solve_exact needs integer weights (dtype %s): only then is the MILP's answer exact" % K.dtype)
    mask = np.asarray(mask, dtype=bool)
    n = K.shape[0]
    iu, ju = np.nonzero(np.triu(mask | mask.T, 1))
    m = len(iu)
    cost = K[iu, ju].astype(np.float64)
    col = np.arange(m)
    degree = sparse.csr_matrix((np.ones(2 * m), (np.concatenate([iu, ju]), np.concatenate([col, col]))), shape=(n, m))
    cons = [LinearConstraint(degree, 2, 2)]
    cut_rows, cut_cols, cut_rhs = [], [], []
    while True:
        if cut_rhs:
            cuts = sparse.csr_matrix((np.ones(len(cut_rows)), (cut_rows, cut_cols)), shape=(len(cut_rhs), m))
            extra = [LinearConstraint(cuts, -np.inf, np.array(cut_rhs, dtype=np.float64))]
        else:
            extra = []
        res = milp(cost, constraints=cons + extra, integrality=np.ones(m), bounds=Bounds(0, 1))
        if res.status == 2:
            return None, None
        assert res.status == 0, res.message
        chosen = np.flatnonzero(res.x > 0.5)
        assert len(chosen) == n and np.all(np.abs(res.x - np.round(res.x)) < 1e-6)
        comps = _components(n, zip(iu[chosen], ju[chosen]))
        if len(comps) == 1:
            break
        for S in comps:                       # sum x(E(S)) <= |S| - 1 for every subtour's vertex set
            inS = np.zeros(n, bool)
            inS[S] = True
            inside = np.flatnonzero(inS[iu] & inS[ju])
            cut_rows += [len(cut_rhs)] * len(inside)
            cut_cols += list(inside)
            cut_rhs.append(len(S) - 1)
    adj = {v: [] for v in range(n)}
    for e in chosen:
        adj[int(iu[e])].append(int(ju[e]))
        adj[int(ju[e])].append(int(iu[e]))
    tour, prev, cur = [0], 0, min(adj[0])
    while cur != 0:
        tour.append(cur)
        prev, cur = cur, (adj[cur][1] if adj[cur][0] == prev else adj[cur][0])
    assert sorted(tour) == list(range(n))
    own = int(sum(int(K[min(a, b), max(a, b)]) for a, b in zip(tour, tour[1:] + tour[:1])))
    assert abs(res.fun - round(res.fun)) < 1e-6 and int(round(res.fun)) == own, (res.fun, own)
    return own, canonical(tour)


# ------------------------------------------------------------- the restatement, with a 1-tree that is quick at n > 64

def one_tree_fast(w, pi, cls):
    """tests/test_tour_exact_host.py's one_tree with its inner loops as array operations: the same picks, the same edge
    order and the same sequential sum, so the same bits."""
    n = w.shape[0]
    c = w + pi[:, None] + pi[None, :]
    rank = np.where(cls == FORCED, 0, np.where(cls == FORBIDDEN, 2, 1))
    done = np.zeros(n, bool)
    done[:2] = True
    kr, kc, par = rank[1].copy(), c[1].copy(), np.ones(n, int)
    edges = []
    for _ in range(n - 2):
        r = np.where(done, 3, kr)
        rmin = r.min()
        if rmin >= 2:
            return None
        u = int(np.argmin(np.where(r == rmin, kc, np.inf)))      # smallest (rank, cost), ties to the smaller vertex
        done[u] = True
        edges.append((u, int(par[u])))
        ru, cu = rank[u], c[u]
        upd = ~done & (ru < 2) & ((ru < kr) | ((ru == kr) & (cu < kc)))
        kr[upd], kc[upd], par[upd] = ru[upd], cu[upd], u
    vs = np.arange(1, n)
    vs = vs[rank[0, 1:] < 2]
    if len(vs) < 2:
        return None
    order = np.lexsort((vs, c[0, vs], rank[0, vs]))
    edges += [(0, int(vs[order[0]])), (0, int(vs[order[1]]))]
    deg = np.zeros(n, int)
    val = 0.0
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
        val += c[a, b]
    return val - 2 * pi.sum(), deg, edges


@contextlib.contextmanager
def _tests_on_path():
    sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        yield
    finally:
        del sys.path[:2]


def restate(w, tour, max_nodes):
    """test_tour_exact_host.branch_bound(w, tour, max_nodes=max_nodes) on one_tree_fast -> (cost, tour, lb, nodes,
    proved)."""
    with _tests_on_path():
        import test_tour_exact_host as host
    slow = host.one_tree
    host.one_tree = one_tree_fast
    try:
        return host.branch_bound(w, [int(x) for x in tour], max_nodes=max_nodes)
    finally:
        host.one_tree = slow


def _check_fast_one_tree():
    """one_tree_fast against the restatement's own, bit for bit, on constrained random instances."""
    with _tests_on_path():
        import test_tour_exact_host as host
    rng = np.random.RandomState(0)
    for n in (5, 9, 17, 30):
        for _ in range(20):
            w = np.triu(rng.randint(1, 5, size=(n, n)).astype(np.float64) / 4, 1)
            w = w + w.T
            cls = np.triu(rng.choice([FREE, FREE, FREE, FORCED, FORBIDDEN], size=(n, n)), 1)
            cls = cls + cls.T
            pi = rng.randn(n) * rng.choice([0.0, 0.3])
            a, b = host.one_tree(w, pi, cls), one_tree_fast(w, pi, cls)
            assert (a is None) == (b is None)
            if a is not None:
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _run_variants(cases, case, inst, opt, tour):
    """The restatement from every incumbent of ``case`` -> [(incumbent name, nodes, proved and at the optimum)]."""
    out = []
    w = cases.kernel_weights(inst)
    for name in cases.incumbents(case):
        start = cases.incumbent(inst, tour, name)
        cost, _, lb, nodes, proved = restate(w, start, cases.restatement_cap(case[1]))
        ok = bool(proved and cost * cases.SCALE == opt and lb <= cost)
        out.append((name, int(nodes), ok))
    return out


def select(families=None, tries=12):
    """The seed search behind tour_optima_cases.CASES: per (family, n) the first seed whose restatement runs meet the
    rule of tour_optima_cases.kind_of for every incumbent, else the first where the main incumbent does; prints them."""
    with _tests_on_path():
        import tour_optima_cases as cases
    _check_fast_one_tree()
    for family, n in cases.SIZES:
        if families and family not in families:
            continue
        if n > cases.BB_MAX_N:
            print('    ("%s", %d, 0),' % (family, n), flush=True)
            continue
        first = None
        for seed in range(tries if n <= 64 else max(2, tries // 3)):
            case = (family, n, seed)
            inst = cases.build(*case)
            opt, tour = solve_exact(inst.K, inst.mask)
            runs = _run_variants(cases, case, inst, opt, tour)
            kinds = [cases.kind_of(family, n, nodes, ok) for _, nodes, ok in runs]
            print("#   %s n=%d seed=%d: %s" % (family, n, seed, list(zip(runs, kinds))), flush=True)
            if kinds[0] == "proving" and first is None:
                first = seed
            if all(k == "proving" for k in kinds):
                first = seed
                break
            if family == "clustered":          # budget_expected whatever the restatement says: the first seed
                break
        print('    ("%s", %d, %d),' % (family, n, 0 if first is None else first), flush=True)


def generate(path=FIXTURE):
    """tests/golden/tour_optima.npz for tour_optima_cases.CASES: per case family, n, seed, CRC32 of K and of the mask,
    the optimum, one optimal tour, and per branch-and-bound run its incumbent, the restatement's node count, whether it
    proved the optimum, and the kind that follows."""
    with _tests_on_path():
        import tour_optima_cases as cases
    _check_fast_one_tree()
    fam, ns, seeds, crc_k, crc_m, opts, tours = [], [], [], [], [], [], []
    bb_case, bb_inc, bb_nodes, bb_proved, bb_kind = [], [], [], [], []
    for k, case in enumerate(cases.CASES):
        family, n, seed = case
        inst = cases.build(*case)
        opt, tour = solve_exact(inst.K, inst.mask)
        fam.append(family)
        ns.append(n)
        seeds.append(seed)
        crc_k.append(zlib.crc32(np.ascontiguousarray(inst.K, dtype=np.int64).tobytes()))
        crc_m.append(zlib.crc32(np.ascontiguousarray(inst.mask, dtype=np.uint8).tobytes()))
        opts.append(opt)
        tours.append(np.asarray(tour, dtype=np.int16))
        line = "%s n=%d seed=%d: optimum %d" % (family, n, seed, opt)
        if n <= cases.BB_MAX_N:
            for name, nodes, ok in _run_variants(cases, case, inst, opt, tour):
                kind = cases.kind_of(family, n, nodes, ok)
                bb_case.append(k)
                bb_inc.append(name)
                bb_nodes.append(nodes)
                bb_proved.append(ok)
                bb_kind.append(kind)
                line += "; %s: %d nodes, %s -> %s" % (name, nodes, "proved" if ok else "not proved", kind)
        print(line, flush=True)
    np.savez_compressed(
        path, family=np.array(fam), n=np.array(ns, dtype=np.int32), seed=np.array(seeds, dtype=np.int32),
        crc_k=np.array(crc_k, dtype=np.uint32), crc_mask=np.array(crc_m, dtype=np.uint32),
        optimum=np.array(opts, dtype=np.int64), tours=np.concatenate(tours),
        bb_case=np.array(bb_case, dtype=np.int32), bb_incumbent=np.array(bb_inc), bb_nodes=np.array(bb_nodes, dtype=np.int32),
        bb_proved=np.array(bb_proved, dtype=bool), bb_kind=np.array(bb_kind))
    print("wrote %s: %d cases, %d branch-and-bound runs, %d bytes" % (path, len(fam), len(bb_case), os.path.getsize(path)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["select"]:
        select(sys.argv[2:])
    else:
        generate()
