"""Seeded launches of the tour chain kernels (csrc/tour_search.hip, tour_baselines.hip, tour_exact.hip) for
tools/record_tour_bits.py and tests/test_gpu_tour_chain_bits.py: the smallest shapes at which the chain workspace in LDS,
the starting-tour check, the chain winner, the refusal of an instance the host never sends and the 2-exchange move can go
wrong.  Inputs come from NumPy generators seeded by the case's data name, so a square case and its _tri twin see the same
weights, starting tours and candidate tables.  Every entry point is called directly through _lib with sentinel-filled
outputs; tours come back as int32, costs and bounds as raw bit patterns, node counts and statuses as int32."""
import zlib

import numpy as np

SENT_TOUR, SENT_I32 = -7, -99
SENT_COST, SENT_LB = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
NAN32, NAN64 = 0x7FC00000, 0x7FF8000000000000
BB_BAD = 2

SMALL = [4, 5, 63, 64, 65, 128]          # the per-lane vertex ownership and the position strider wrap at 64
RAGGED = [5, 64, 100, 64, 100]           # under n_max = 100: the carve uses n_max, the tours use n
RAGGED_STARTS = ["valid", "n", "repeat", "fill", "valid"]
KEYS = [2 ** 40 + 17, 3, 2 ** 33, 10 ** 12 + 5, 77, 2 ** 50]   # `index`: large, not consecutive


def _case(name, entry, ns, tri, data=None, **kw):
    c = dict(name=name, entry=entry, ns=list(ns), tri=tri, data=data or name, n_max=max(ns), unit=False, starts=None,
             index=None, refused=[], bad=[])
    c.update(kw)
    return c


def cases():
    """The launches, in recording order.  A name ending in /sq or /tri has a twin of the other layout on the same data;
    for n <= 128 the two must give the same bits (twins())."""
    out = []

    def both(name, entry, ns, **kw):
        for tri in (False, True):
            out.append(_case("%s/%s" % (name, "tri" if tri else "sq"), entry, ns, tri, data=name, **kw))

    tabs = (("search", {}), ("search_knn", {"neighbors": 8}), ("search_cand", {"neighbors": 8}))
    for entry, kw in tabs:
        both(entry + "/small", entry, SMALL, restarts=3, kicks=2, **kw)
        both(entry + "/ragged", entry, RAGGED, restarts=16, kicks=0, starts=RAGGED_STARTS, index=KEYS[:5], **kw)
        both(entry + "/refuse", entry, [6, 3, 7], restarts=3, kicks=2, refused=[1], **kw)
    out.append(_case("search/129", "search", [129], True, restarts=1, kicks=0))
    # the largest chain count the launcher admits at n_max = 256: the last chain's third tour ends at the LDS budget
    out.append(_case("search/256x10", "search", [256], True, restarts=10, kicks=0))
    out.append(_case("search_knn/256x9", "search_knn", [256], True, restarts=9, kicks=0, neighbors=8))
    out.append(_case("search_cand/256x9", "search_cand", [256], True, restarts=9, kicks=0, neighbors=8))

    both("bound/small", "lower_bound", [4, 65, 128], iters=60)
    out.append(_case("bound/256", "lower_bound", [4, 65, 256], True, iters=30))
    both("bound/refuse", "lower_bound", [6, 3, 7], iters=30, refused=[1])

    both("nn/start0", "nearest_neighbor", SMALL, start=0)
    both("nn/start200", "nearest_neighbor", SMALL, start=200)            # above n: taken modulo n
    both("nn/best4_5", "nearest_neighbor", [4, 5], start=-1)             # most of the 16 waves have no start
    both("nn/best65", "nearest_neighbor", [65, 64], start=-1)
    both("nn/unit", "nearest_neighbor", [6, 65], start=-1, unit=True)     # every start ties: start 0 must win
    both("nn/refuse", "nearest_neighbor", [6, 3, 7], start=-1, refused=[1])
    out.append(_case("nn/256", "nearest_neighbor", [129, 256], True, start=-1))

    both("anneal/levels0", "anneal", [4, 5, 64, 65, 128], chains=3, levels=0, starts=["valid", "n", "repeat", "fill", "valid"])
    both("anneal/short", "anneal", RAGGED, chains=4, levels=3, starts=RAGGED_STARTS, index=KEYS[:5])
    both("anneal/no_init", "anneal", SMALL, chains=16, levels=2, index=KEYS)
    both("anneal/refuse", "anneal", [6, 3, 7], chains=4, levels=2, refused=[1])
    out.append(_case("anneal/256x10", "anneal", [256], True, chains=10, levels=2))

    # the branch and bound: one launch that proves its instances (three of its incumbents are no permutations), one with
    # max_nodes = 1, one with an n = 3 inside
    out.append(_case("bb/prove", "branch_bound", [4, 5, 8, 9, 10, 12, 9, 10], False, max_nodes=2048,
                     starts=["id", "valid", "id", "n", "valid", "id", "repeat", "fill"], bad=[3, 6, 7], upper=False))
    out.append(_case("bb/root", "branch_bound", [4, 63, 64, 65, 128], False, max_nodes=1, starts=["id"] * 5, upper=True))
    out.append(_case("bb/refuse", "branch_bound", [6, 3, 7], False, max_nodes=64, starts=["id"] * 3, bad=[1], upper=False))
    return out


def twins(cs):
    """(square case, tri case) pairs of one data name."""
    by = {c["name"]: c for c in cs}
    return [(c, by[c["name"][:-2] + "tri"]) for c in cs if c["name"].endswith("/sq")]


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))[:-1]]).astype(np.int64)


def _weights(rng, n, unit):
    """A symmetric fp32 matrix with a zero diagonal: unit weights, or the distances of n points of the unit square."""
    if unit:
        return np.ones((n, n), dtype=np.float32) - np.eye(n, dtype=np.float32)
    p = rng.rand(n, 2)
    return np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1)).astype(np.float32)


def _start(rng, n, kind):
    """A starting tour: a permutation ("valid", or "id" = 0..n-1), one with an id equal to n, one with a repeated id, or
    the -1 filler that dataset._pack writes for "none"."""
    t = np.arange(n, dtype=np.int32) if kind == "id" else rng.permutation(n).astype(np.int32)
    if kind == "n":
        t[n // 2] = n
    elif kind == "repeat":
        t[n - 1] = t[0]
    elif kind == "fill":
        t[:] = -1
    return t


def build(c):
    """The host arrays of case c: W (packed for its layout), w_off, t_off, n, and what its entry point reads beside."""
    rng = np.random.RandomState(zlib.crc32(c["data"].encode()))
    ns = np.array(c["ns"], dtype=np.int32)
    mats = [_weights(rng, int(n), c["unit"]) for n in ns]
    parts = [m[np.triu_indices(len(m), 1)] if c["tri"] else m.reshape(-1) for m in mats]
    h = {"n": ns, "W": np.concatenate(parts).astype(np.float32), "w_off": _offsets([p.size for p in parts]),
         "t_off": _offsets(ns), "mats": mats}
    h["starts"] = None if c["starts"] is None else \
        np.concatenate([_start(rng, int(n), k) for n, k in zip(ns, c["starts"])]).astype(np.int32)
    h["index"] = None if c["index"] is None else np.array(c["index"], dtype=np.int64)
    if c["entry"] == "search_cand":   # rows with ids past n (skipped), repeats and asymmetric pairs
        tabs = []
        for n in ns:
            tab = rng.randint(0, 256, size=(int(n), c["neighbors"]))
            tab[::2] %= int(n)
            tabs.append(tab.astype(np.uint8).reshape(-1))
        h["cand"], h["c_off"] = np.concatenate(tabs), _offsets([t.size for t in tabs])
    if c["entry"] in ("lower_bound", "branch_bound"):   # the fp32 cost of the tour 0..n-1
        h["upper"] = np.array([np.float32(m[np.arange(len(m)), np.roll(np.arange(len(m)), -1)].astype(np.float64).sum())
                               for m in mats], dtype=np.float32)
    if c["entry"] == "anneal":
        L = c["levels"]
        mean = np.array([m.sum() / max(m.size - len(m), 1) for m in mats], dtype=np.float64)
        temps = 0.1 * (0.02 ** (np.arange(L) / max(L - 1.0, 1.0)))
        h["inv_temp"] = np.ascontiguousarray((1.0 / (mean[:, None] * temps[None, :])).astype(np.float32)).reshape(len(ns), L)
        h["per_level"] = (ns.astype(np.int64) ** 2 // 2).astype(np.int32)
    return h


def run_case(c, device):
    """Launch case c on `device` -> {output name: array}."""
    import torch
    from tspgnn import _lib
    h = build(c)
    G, total = len(c["ns"]), int(h["n"].sum())

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)

    d = {k: dev(h[k]) for k in ("W", "w_off", "t_off", "n", "starts", "index")}
    p = {k: _lib.ptr(v) for k, v in d.items()}
    tours = torch.full((total,), SENT_TOUR, dtype=torch.int32, device=device)
    cost = torch.full((G,), SENT_COST, dtype=torch.int32, device=device)
    lb = torch.full((G,), SENT_LB, dtype=torch.int64, device=device)
    name = "tspgnn_tour_" + c["entry"] + ("_tri" if c["tri"] else "")
    seed = zlib.crc32(c["data"].encode()) * 2654435761 & 0xFFFFFFFFFFFFFFFF
    st = _lib.current_stream()
    out = {}
    with torch.cuda.device(device):
        if c["entry"].startswith("search"):
            table, cols = (), ()
            if c["entry"] == "search_cand":
                d_cand, d_coff = dev(h["cand"]), dev(h["c_off"])
                table = (_lib.ptr(d_cand), _lib.ptr(d_coff))
            if "neighbors" in c:
                cols = (c["neighbors"],)
            _lib.call(name, p["W"], p["w_off"], p["n"], p["starts"], p["t_off"], p["index"], *table, G, c["n_max"],
                      c["restarts"], c["kicks"], *cols, seed, _lib.ptr(tours), _lib.ptr(cost), st)
            out = {"tours": tours, "cost": cost}
        elif c["entry"] == "lower_bound":
            d_up = dev(h["upper"])
            _lib.call(name, p["W"], p["w_off"], p["n"], _lib.ptr(d_up), G, c["n_max"], c["iters"], _lib.ptr(lb), st)
            out = {"lb": lb}
        elif c["entry"] == "nearest_neighbor":
            _lib.call(name, p["W"], p["w_off"], p["n"], p["t_off"], G, c["n_max"], c["start"], _lib.ptr(tours),
                      _lib.ptr(cost), st)
            out = {"tours": tours, "cost": cost}
        elif c["entry"] == "anneal":
            d_inv, d_per = dev(h["inv_temp"]), dev(h["per_level"])
            _lib.call(name, p["W"], p["w_off"], p["n"], p["starts"], p["t_off"], p["index"],
                      _lib.ptr(d_inv) if c["levels"] else None, _lib.ptr(d_per), G, c["n_max"], c["chains"], c["levels"],
                      seed, _lib.ptr(tours), _lib.ptr(cost), st)
            out = {"tours": tours, "cost": cost}
        else:
            d_up = dev(h["upper"]) if c["upper"] else None
            tours.copy_(d["starts"])                     # in: the incumbents
            nodes = torch.full((G,), SENT_I32, dtype=torch.int32, device=device)
            status = torch.full((G,), SENT_I32, dtype=torch.int32, device=device)
            ws = torch.empty(int(_lib.lib.tspgnn_tour_branch_bound_ws(G, c["n_max"])), dtype=torch.uint8, device=device)
            _lib.call(name, p["W"], p["w_off"], p["n"], p["t_off"], _lib.ptr(d_up), G, c["n_max"], 100, 30, c["max_nodes"],
                      1e-9, _lib.ptr(ws), _lib.ptr(tours), _lib.ptr(lb), _lib.ptr(nodes), _lib.ptr(status), st)
            out = {"tours": tours, "lb": lb, "nodes": nodes, "status": status}
        torch.cuda.synchronize(device)
    views = {"cost": np.uint32, "lb": np.uint64}
    return {k: v.cpu().numpy().view(views.get(k, np.int32)) for k, v in out.items()}


def slots(c):
    """Per instance, its slice of the case's tours array."""
    off = _offsets(c["ns"])
    return [slice(int(o), int(o) + int(n)) for o, n in zip(off, c["ns"])]


def check_shape_of_answers(c, h, out):
    """What a recording or a run must show whatever the bits: a refused instance has a NaN cost or bound and an untouched
    tour slot, a bad incumbent of the branch and bound comes back as TSPGNN_BB_BAD with a NaN bound, 0 nodes and its tour
    untouched, and every other instance has a canonical permutation and a number."""
    bb = c["entry"] == "branch_bound"
    for i, (n, sl) in enumerate(zip(c["ns"], slots(c))):
        refused = i in c["refused"] or i in c["bad"]
        if "cost" in out:
            assert (int(out["cost"][i]) == NAN32) == refused, (c["name"], i, hex(int(out["cost"][i])))
        if "lb" in out:
            assert (int(out["lb"][i]) == NAN64) == refused, (c["name"], i, hex(int(out["lb"][i])))
            assert int(out["lb"][i]) != SENT_LB
        if bb:
            assert (int(out["status"][i]) == BB_BAD) == refused and (int(out["nodes"][i]) == 0) == refused, (c["name"], i)
            assert c["max_nodes"] > 1 or refused or int(out["nodes"][i]) == 1
        if "tours" in out:
            t = out["tours"][sl]
            if refused:
                want = h["starts"][sl] if bb else np.full(n, SENT_TOUR, dtype=np.int32)
                assert np.array_equal(t, want), (c["name"], i, t)
            else:
                assert sorted(t.tolist()) == list(range(n)) and t[0] == 0 and t[1] < t[n - 1], (c["name"], i, t)
