"""Exact tour labels without a GPU: the argument checks of tspgnn_tour_branch_bound and its workspace query answer before
any launch, prove_tours routes what it does not launch, and a NumPy branch and bound under the branching rules that
include/tspgnn.h states for the kernel agrees with the Held-Karp DP (it pins the rules; it is not compared bit for bit
with the kernel, whose ascent runs in fp32)."""
import ctypes

import numpy as np
import pytest

from test_gpu_tour_solver import _w, held_karp
from tspgnn import _lib, dataset

FREE, FORCED, FORBIDDEN = 0, 1, 2


def int_family(rng, sizes, conn=0.35):
    """Weights from {1, 2, 3} on a sparse graph with a planted cycle: many ties, so the 1-tree bound has to branch.
    Returns [(Ma, Mw)] and the planted permutations."""
    out, perms = [], []
    for n in sizes:
        Mw = np.triu(rng.randint(1, 4, size=(n, n)).astype(np.float64), 1)
        Ma = np.triu((rng.rand(n, n) < conn).astype(float), 1)
        perm = [int(x) for x in rng.permutation(n)]
        for i, j in zip(perm, perm[1:] + perm[:1]):
            Ma[min(i, j), max(i, j)] = 1
        out.append((Ma, Mw))
        perms.append(perm)
    return out, perms


# ---------------------------------------------------------------------------- the kernel's rules, in NumPy and fp64

def one_tree(w, pi, cls):
    """Minimum 1-tree by (class, cost): Prim on 1..n-1 from vertex 1, then vertex 0's two best edges; a forced edge goes
    before any free one, a forbidden one is never picked, ties to the smaller vertex.  None when there is none."""
    n = w.shape[0]
    c = w + pi[:, None] + pi[None, :]
    rank = np.where(cls == FORCED, 0, np.where(cls == FORBIDDEN, 2, 1))
    done = np.zeros(n, bool)
    done[:2] = True
    kr, kc, par = rank[1].copy(), c[1].copy(), np.ones(n, int)
    edges = []
    for _ in range(n - 2):
        cand = [(kr[v], kc[v], v) for v in range(2, n) if not done[v] and kr[v] < 2]
        if not cand:
            return None
        u = min(cand)[2]
        done[u] = True
        edges.append((u, int(par[u])))
        for v in range(2, n):
            if not done[v] and rank[u, v] < 2 and (rank[u, v], c[u, v]) < (kr[v], kc[v]):
                kr[v], kc[v], par[v] = rank[u, v], c[u, v], u
    at0 = sorted((rank[0, v], c[0, v], v) for v in range(1, n) if rank[0, v] < 2)
    if len(at0) < 2:
        return None
    edges += [(0, at0[0][2]), (0, at0[1][2])]
    deg = np.zeros(n, int)
    val = 0.0
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
        val += c[a, b]
    return val - 2 * pi.sum(), deg, edges


def ascend(w, pi, cls, ub, iters):
    """tour_common.h's schedule: Polyak steps towards ub, lambda = 2 halved after 8 steps without a new best."""
    best, bp, lam, stall = -np.inf, pi.copy(), 2.0, 0
    for _ in range(iters):
        t = one_tree(w, pi, cls)
        if t is None:
            return None
        L, deg, _ = t
        if L > best:
            best, bp, stall = L, pi.copy(), 0
        else:
            stall += 1
            if stall >= 8:
                lam, stall = lam * 0.5, 0
        g = deg - 2
        gg = int((g * g).sum())
        if gg == 0 or lam < 1e-6:
            break
        pi = pi + lam * max(ub - L, 1e-4 * abs(L) + 1e-30) / gg * g
    return bp


def classes(n, path):
    """The class matrix after the path's decisions (v, e1, e2 or -1, child), or None for an infeasible node."""
    cls = np.zeros((n, n), int)
    for v, e1, e2, child in path:
        if e2 >= 0:
            sets = [((e1, FORCED), (e2, FORCED)), ((e1, FORCED), (e2, FORBIDDEN)), ((e1, FORBIDDEN),)][child]
        else:
            sets = [((e1, FORCED),), ((e1, FORBIDDEN),)][child]
        for x, c in sets:
            cls[v, x] = cls[x, v] = c
    nf = (cls == FORCED).sum(1)
    if (nf > 2).any():
        return None
    for v in np.nonzero(nf == 2)[0]:
        for x in range(n):
            if x != v and cls[v, x] == FREE:
                cls[v, x] = cls[x, v] = FORBIDDEN
    if (n - 1 - (cls == FORBIDDEN).sum(1) < 2).any():
        return None
    return cls


def cycle_cost(w, t):
    s = 0.0
    for a, b in zip(t, t[1:] + t[:1]):
        s += w[a, b]
    return s


def branch_bound(w, tour, root_iters=400, node_iters=30, max_nodes=2048, opt_tol=1e-9):
    """Depth-first branch and bound as include/tspgnn.h describes it.  Returns (cost, tour, lb, nodes, proved)."""
    n = w.shape[0]
    inc, best_t = cycle_cost(w, tour), list(tour)
    lbmin, left_open, stack, nodes = np.inf, False, [], 1
    cls = np.zeros((n, n), int)
    bp, plr = ascend(w, np.zeros(n), cls, inc, root_iters), -np.inf
    while True:
        if bp is not None:
            Lr, deg, edges = one_tree(w, bp, cls)
            Lr = max(Lr, plr)
            if Lr >= inc * (1 - opt_tol):
                lbmin = min(lbmin, Lr)
            elif (deg == 2).all():
                adj = {v: [] for v in range(n)}
                for a, b in edges:
                    adj[a].append(b)
                    adj[b].append(a)
                t, prev, cur = [0], 0, min(adj[0])
                while cur != 0:
                    t.append(cur)
                    prev, cur = cur, (adj[cur][1] if adj[cur][0] == prev else adj[cur][0])
                if cycle_cost(w, t) < inc:
                    inc, best_t = cycle_cost(w, t), t
                lbmin = min(lbmin, Lr)
            elif nodes >= max_nodes:
                lbmin, left_open = min(lbmin, Lr), True
            else:
                v = int(np.argmax(deg))                                     # largest degree, ties to the smaller id
                xs = sorted(((w[v, b if a == v else a], b if a == v else a) for a, b in edges
                             if v in (a, b) and cls[v, b if a == v else a] == FREE))   # free tree edges by weight, id
                e2 = xs[1][1] if (cls[v] == FORCED).sum() == 0 else -1
                stack.append([v, xs[0][1], e2, 0, Lr, bp])
        bp = None
        while stack and bp is None:
            top = stack[-1]
            if top[3] >= (3 if top[2] >= 0 else 2):
                stack.pop()
            elif nodes >= max_nodes:
                lbmin, left_open = min(lbmin, top[4]), True
                stack.pop()
            elif top[4] >= inc * (1 - opt_tol):
                lbmin = min(lbmin, top[4])
                stack.pop()
            else:
                top[3] += 1
                cls = classes(n, [(s[0], s[1], s[2], s[3] - 1) for s in stack])
                if cls is None:
                    continue
                nodes += 1
                plr = top[4]
                bp = ascend(w, top[5], cls, inc, node_iters)
                if bp is None:
                    continue
        if bp is None:
            break
    return inc, best_t, min(inc, lbmin), nodes, not left_open


def test_numpy_branch_bound_under_the_kernels_rules_matches_the_dp():
    rng = np.random.RandomState(5)
    insts, perms = int_family(rng, rng.randint(5, 14, size=24))
    branched = 0
    for (Ma, Mw), perm in zip(insts, perms):
        n = Ma.shape[0]
        A = dataset._edge_mask(Ma)
        w = dataset._penalised(A[None], Mw[None])[0].astype(np.float64)
        opt = held_karp(_w(Ma, Mw))
        cost, tour, lb, nodes, proved = branch_bound(w, perm)
        assert proved and sorted(tour) == list(range(n))
        assert abs(cost - opt) <= 1e-9 * opt, (cost, opt)
        assert lb <= opt and opt - lb <= 2e-6 * opt
        branched += nodes > 1
    assert branched >= 8   # a third of the family: otherwise this says nothing about the branching rules


# ---------------------------------------------------------------------------------- entry points, before any launch

def _bb(**kw):
    p = ctypes.c_void_p(16)
    a = dict(W=p, w_off=p, n=p, t_off=p, upper=None, n_inst=4, n_max=20, root_iters=400, node_iters=30, max_nodes=64,
             opt_tol=1e-9, workspace=p, tours=p, lb=p, nodes=p, status=p, stream=None)
    a.update(kw)
    return _lib.lib.tspgnn_tour_branch_bound(*a.values())


def test_branch_bound_rejects_bad_arguments_without_gpu():
    for name in ("W", "w_off", "n", "t_off", "workspace", "tours", "lb", "nodes", "status"):
        assert _bb(**{name: None}) == -1, name
        assert b"null pointer" in _lib.lib.tspgnn_last_error()
    assert _bb(n_max=3) == -1
    assert _bb(n_max=129) == -2
    assert _bb(max_nodes=0) == -1 and _bb(max_nodes=65537) == -1
    assert _bb(node_iters=0) == -1 and _bb(root_iters=0) == -1
    assert _bb(opt_tol=-1e-9) == -1 and _bb(opt_tol=float("nan")) == -1 and _bb(opt_tol=float("inf")) == -1
    assert _bb(n_inst=-1) == -1
    # an empty batch is a no-op, whatever else is passed
    assert _bb(n_inst=0, W=None, w_off=None, n=None, t_off=None, workspace=None, tours=None, lb=None, nodes=None,
               status=None, n_max=0) == 0


def test_workspace_query_grows_with_both_arguments():
    q = _lib.lib.tspgnn_tour_branch_bound_ws
    assert q(0, 20) == 0 and q(4, 3) == 0 and q(4, 129) == 0
    assert 0 < q(1, 4) < q(2, 4) < q(2, 5) < q(2, 128) < q(8192, 128)
    assert q(8192, 128) == 8192 * 128 * 128 * 4    # TSPGNN_BB_MAX_DEPTH levels of n_max floats: beyond 2^31


def test_prove_tours_routes_without_touching_the_library():
    R = dataset.TourResult
    tri = (np.triu(np.ones((3, 3)), 1), np.triu(np.ones((3, 3)), 1))
    (small,) = dataset.solve_tours([tri])                       # n < 4: solved on the host
    n = 130
    big = (np.triu(np.ones((n, n)), 1), np.random.RandomState(0).rand(n, n))
    big_r = R(list(range(n)), 1.0, 0.5, True, 1.0)
    path = np.zeros((5, 5))
    for i in range(4):
        path[i, i + 1] = 1                                      # no Hamiltonian cycle: the incumbent is infeasible
    bad = (path, np.ones((5, 5)))
    bad_r = R([0, 1, 2, 3, 4], 5.0, 4.0, False, 5.0)
    stats = {}
    out = dataset.prove_tours([tri, big, bad], [small, big_r, bad_r], stats=stats)
    assert out == [small, big_r, bad_r]
    assert list(stats["status"]) == ["proved", "skipped", "skipped"]
    assert list(stats["nodes"]) == [0, 0, 0] and stats["seconds"] == 0.0
    assert dataset.prove_tours([], [], stats=stats) == [] and len(stats["status"]) == 0


def test_prove_tours_rejects_bad_arguments_without_gpu():
    tri = (np.triu(np.ones((3, 3)), 1), np.triu(np.ones((3, 3)), 1))
    (r,) = dataset.solve_tours([tri])
    with pytest.raises(ValueError, match="2 instances but 1 results"):
        dataset.prove_tours([tri, tri], [r])
    with pytest.raises(ValueError, match="max_nodes"):
        dataset.prove_tours([tri], [r], max_nodes=0)
    with pytest.raises(ValueError, match="max_nodes"):
        dataset.prove_tours([tri], [r], max_nodes=65537)
    with pytest.raises(ValueError, match="node_iters"):
        dataset.prove_tours([tri], [r], node_iters=0)
    with pytest.raises(ValueError, match="opt_tol"):
        dataset.prove_tours([tri], [r], opt_tol=float("nan"))
    with pytest.raises(ValueError, match="permutation"):
        dataset.prove_tours([tri], [r._replace(tour=[0, 1, 1])])
    with pytest.raises(ValueError, match="max_nodes"):
        dataset.label_tours([tri], exact=True, max_nodes=0)


# Two arguments wrong at once: which one the entry point names is the order of its checks.  Codes and messages as the
# library gave them before the entry point took check_layout of csrc/tour_common.h.
@pytest.mark.parametrize("kw,code,message", [
    (dict(n_max=129, root_iters=0, node_iters=0, max_nodes=0, opt_tol=-1.0), -2, "n_max=129 exceeds 128"),
    (dict(n_max=3, root_iters=0, max_nodes=0), -1, "n_max=3 must be at least 4"),
    (dict(root_iters=0, node_iters=1, max_nodes=0), -1, "root_iters=0, node_iters=1"),
    (dict(root_iters=1, node_iters=0, max_nodes=70000, opt_tol=-1.0), -1, "root_iters=1, node_iters=0"),
    (dict(max_nodes=70000, opt_tol=-1.0), -1, "max_nodes=70000 not in [1, 65536]"),
    (dict(opt_tol=-1.0, W=None), -1, "opt_tol=-1 must be finite and >= 0"),
    (dict(n_inst=-1, n_max=129, root_iters=0, W=None), -1, "n_inst=-1"),
])
def test_two_faults_at_once_name_the_first_check(kw, code, message):
    assert _bb(**kw) == code
    assert _lib.lib.tspgnn_last_error().decode() == "tour_branch_bound: " + message
