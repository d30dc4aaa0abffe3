"""A NumPy restatement of tspgnn_vote_scores_i32 and tspgnn_tour_beam, written from the definition in include/tspgnn.h:
the integer scores q(v), the pair tables (smallest edge id per pair), the lists L_0 .. L_{n-1} with the candidates of a
step ordered by one lexsort over (score descending, i, u), the stranded fill, the final choice by score or by cost, the
canonical form, n_missing and the fp32 cost summed in tour order with np.float32 additions.  It keeps whole paths per
entry (no parent trace, no radix select, no tables in a workspace): nothing of the kernel's layout is in here."""
import numpy as np

SCORE_MIN = -(1 << 22)


def q_scores(votes):
    """q(v) = clamp(rint(65536 logsigmoid(v)), -2^22, 0) as int32, in float64, NaN -> -2^22."""
    v = np.asarray(votes, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.rint(65536.0 * (np.minimum(v, 0.0) - np.log1p(np.exp(-np.abs(v)))))
    s = np.where(np.isnan(s), float(SCORE_MIN), s)
    return np.clip(s, float(SCORE_MIN), 0.0).astype(np.int32)


def q_scores_second(votes):
    """The same number by another route: logsigmoid(v) = -logaddexp(0, -v)."""
    v = np.asarray(votes, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.rint(-65536.0 * np.logaddexp(0.0, -v))
    s = np.where(np.isnan(s), float(SCORE_MIN), s)
    return np.clip(s, float(SCORE_MIN), 0.0).astype(np.int32)


def pair_tables(n, uv, w, score):
    """has [n, n] bool, Q [n, n] int64 (the clamped score of the smallest edge id joining the pair), Wt [n, n] float32."""
    uv = np.asarray(uv, dtype=np.int64).reshape(-1, 2)
    ok = (uv[:, 0] >= 0) & (uv[:, 0] < n) & (uv[:, 1] >= 0) & (uv[:, 1] < n) & (uv[:, 0] != uv[:, 1])
    ids = np.nonzero(ok)[0][::-1]           # descending: of repeated indices the last assignment stands, the smallest id
    E = np.full((n, n), -1, dtype=np.int64)
    E[uv[ids, 0], uv[ids, 1]] = ids
    E[uv[ids, 1], uv[ids, 0]] = ids
    has = E >= 0
    sc = np.clip(np.asarray(score, dtype=np.int64).reshape(-1), SCORE_MIN, 0)
    Q = np.where(has, sc[np.maximum(E, 0)] if len(sc) else 0, 0).astype(np.int64)
    wt = np.asarray(w, dtype=np.float32).reshape(-1)
    Wt = np.where(has, wt[np.maximum(E, 0)] if len(wt) else 0, 0).astype(np.float32)
    return has, Q, Wt


def canonical(seq):
    seq = [int(v) for v in seq]
    assert seq[0] == 0
    return seq if seq[1] < seq[-1] else [0] + seq[1:][::-1]


def cost_key(c):
    """fp32 costs -> uint32 keys in ascending order of the numbers: -0.0 before +0.0, a NaN after everything."""
    b = np.ascontiguousarray(c, dtype=np.float32).view(np.uint32)
    key = np.where((b & np.uint32(0x80000000)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return key


def tour_cost(tour, has, Wt):
    """(n_missing, fp32 cost) of one cyclic tour: one running sum from 0, the closing pair last."""
    cost, missing = np.float32(0), 0
    for a, b in zip(tour, tour[1:] + tour[:1]):
        if has[a, b]:
            cost = np.float32(cost + Wt[a, b])
        else:
            missing += 1
    return missing, cost


def entry_costs(paths, has, Wt):
    """C_i of every Hamiltonian path of a final list, all entries at once: the additions run position by position."""
    L, n = paths.shape
    rev = paths[:, 1] > paths[:, n - 1]
    tours = paths.copy()
    tours[rev, 1:] = paths[rev, :0:-1]
    c = np.zeros(L, dtype=np.float32)
    for k in range(n):
        a, b = tours[:, k], tours[:, (k + 1) % n]
        c = np.where(has[a, b], (c + Wt[a, b]).astype(np.float32), c).astype(np.float32)
    return c


def beam_instance(n, uv, w, score, beam, select):
    """-> dict(tour, n_missing, cost, score, n_closed, stranded, n_final) of one instance: uv [m, 2] local ids, w [m]
    weights, score [m] integers (clamped here), select "score" or "cost".  stranded: the step k at which L_{k+1} came out
    empty, else None; n_final: the entries of L_{n-1} (0 when stranded)."""
    assert select in ("score", "cost") and beam >= 1
    has, Q, Wt = pair_tables(n, uv, w, score)
    paths = np.zeros((1, 1), dtype=np.int64)
    S = np.zeros(1, dtype=np.int64)
    visited = np.zeros((1, n), dtype=bool)
    visited[0, 0] = True
    for k in range(n - 1):
        last = paths[:, -1]
        ii, uu = np.nonzero(has[last] & ~visited)          # row-major: i ascending, then u ascending
        if len(ii) == 0:
            seq = [int(v) for v in paths[0]] + [v for v in range(n) if not visited[0, v]]
            tour = canonical(seq)
            missing, cost = tour_cost(tour, has, Wt)
            return {"tour": tour, "n_missing": missing, "cost": cost, "score": int(S[0]), "n_closed": 0, "stranded": k,
                    "n_final": 0}
        sc = S[ii] + Q[last[ii], uu]
        keep = np.lexsort((uu, ii, -sc))[:beam]
        ii, uu, S = ii[keep], uu[keep], sc[keep]
        paths = np.concatenate([paths[ii], uu[:, None]], axis=1)
        visited = visited[ii]
        visited[np.arange(len(ii)), uu] = True
    last = paths[:, -1]
    closed = has[last, 0]
    F = S + np.where(closed, Q[last, 0], 0)
    idx = np.arange(len(S))
    if select == "score":
        best = int(np.lexsort((idx, -F, ~closed))[0])
    else:
        best = int(np.lexsort((idx, cost_key(entry_costs(paths, has, Wt)).astype(np.int64), ~closed))[0])
    tour = canonical(paths[best])
    missing, cost = tour_cost(tour, has, Wt)
    return {"tour": tour, "n_missing": missing, "cost": cost, "score": int(F[best]), "n_closed": int(closed.sum()),
            "stranded": None, "n_final": len(S)}


def beam_batch(case, scores, beam, select):
    """Per instance of a decode_cases batch (scores [M] in place of its votes) -> [beam_instance(...)]."""
    out = []
    for b in range(len(case["n"])):
        e0, e1 = case["seg"][b], case["seg"][b + 1]
        out.append(beam_instance(int(case["n"][b]), case["uv"][e0:e1] - case["vseg"][b], case["wc"][e0:e1, 0],
                                 scores[e0:e1], beam, select))
    return out
