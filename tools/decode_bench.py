"""Times the vote decoder (tspgnn_tour_from_votes) beside the forward pass that produces its votes, in one process, at
C2 (128 x n=40), the C4 ragged batch (512 graphs, n 20-80) and one n=200 batch (32 graphs), all at d = 64, T = 32.

Per shape, after a warm-up of both: the forward as a replayed captured graph and as eager launches, and the decode launch
alone, each as the median and the minimum over --reps windows of --inner back-to-back calls between two device events
(tools/baseline_bench.py's rule -- a timing ends in a device synchronise -- with events, because a decode launch is far
shorter than a host clock resolves).  One JSON line per shape, also written to --out.

--beam K[,K...] times the beam decoder as well (tspgnn_vote_scores_i32 once, then tspgnn_tour_beam per width and per
select, at the default workspace cap), adds its columns to the shape's line and appends to --out instead of replacing it.

--guide K[,KN] (repeatable) times tspgnn_vote_neighbors at (k_vote, k_near) = (K, KN) beside the forward, then polishes
the greedy decoder's tours -- label_tours from the decoded tour at --restarts / --kicks -- three ways at equal settings:
the full scan, neighbors = K + KN, and the guide's rows as candidates; per way the search seconds label_tours reports
(second of two calls) and the mean polished cost.  The shape "trained" (the five n = 20 instances and the checkpoint of
tests/golden/trained_d64.npz, T = 8) is added to the shapes; the lines go to --out, appended.

    python tools/decode_bench.py [--shapes c2,c4,n200] [--reps 20] [--inner 10] [--beam 1,16,128,1024]
                                 [--guide 8 --guide 4,4 [--restarts 1] [--kicks 0]] [--out profiles/decode_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsp-gnn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tspgnn  # noqa: E402
from oracle import params as P  # noqa: E402

SHAPES = {"c2": [40] * 128, "c4": list(np.random.RandomState(0).randint(20, 81, size=512)), "n200": [200] * 32}


def windows(fn, reps, inner):
    """Milliseconds per call of fn over `reps` windows of `inner` calls: (median, min)."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out)), float(np.min(out))


def polish_ways(instances, decoded, tab, v0, guide, restarts, kicks):
    """{way: {"search_ms", "mean_cost"}} of the polish from the decoded tours: full scan, neighbors=K, guide rows."""
    pairs = [(Ma, Mw) for Ma, Mw, _ in instances]
    tables = [tab[v0[i]:v0[i + 1]] for i in range(len(pairs))]
    K = guide[0] + guide[1]
    out = {}
    for way, kw in (("full", {}), ("neighbors=%d" % K, {"neighbors": K}), ("guide=%d,%d" % guide, {"candidates": tables})):
        for _ in range(2):      # the first call warms the kernel up
            t = {}
            res = tspgnn.label_tours(pairs, init_tours=decoded, restarts=restarts, kicks=kicks, lower_bound=False,
                                     timings=t, **kw)
        out[way] = {"search_ms": round(1e3 * t["search"], 3), "mean_cost": round(float(np.mean([r.cost for r in res])), 4),
                    "feasible": int(sum(r.feasible for r in res))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c4,n200")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--timesteps", type=int, default=32)
    ap.add_argument("--beam", default="", help="beam widths to time, comma-separated (none: the greedy decoder only)")
    ap.add_argument("--guide", action="append", default=[], help="K[,KN]: time vote_neighbors and the guided polish")
    ap.add_argument("--restarts", type=int, default=1, help="of the --guide polish")
    ap.add_argument("--kicks", type=int, default=0, help="of the --guide polish")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench needs an MI355X"
    d = 64
    model = tspgnn.build_network(d)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    lines = []
    guides = [tuple(int(k) for k in (g + ",0").split(",")[:2]) for g in a.guide]
    for name in a.shapes.split(",") + (["trained"] if guides else []):
        if name == "trained":
            z = np.load(os.path.join(ROOT, "tests", "golden", "trained_d64.npz"))
            model.store.load({k: z[k].astype(np.float64) for k in z.files})
            rng, sizes, a.timesteps = np.random.RandomState(5), [20] * 5, 8
            instances = [tspgnn.random_instance(20, rng) for _ in sizes]
            EV, W, C, route_exists, n_vertices, n_edges = tspgnn.InstanceLoader.create_batch(instances, target_cost=0.2)
        else:
            model.store.load(P.init_params(d, seed=1, perturb=True))
            sizes = SHAPES[name]
            EV, W, C, route_exists, n_vertices, n_edges = tspgnn.synthetic_batch(sizes, seed=1234)
        feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: a.timesteps,
                model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
        b = sess.prepare(feed)
        replay = sess.capture_forward(b)            # (warms the forward up, f16x2 range guard included)
        votes = replay()["E_vote"]
        for _ in range(3):
            dec = tspgnn.tours_from_votes(b, votes)
        torch.cuda.synchronize()
        assert int((dec.n_missing != 0).sum()) == 0    # complete graphs: every decoded tour is feasible
        graph = windows(replay, a.reps, a.inner)
        eager = windows(lambda: sess.forward_device(b), a.reps, max(1, a.inner // 5))
        decode = windows(lambda: tspgnn.tours_from_votes(b, votes), a.reps, a.inner)
        rounds = int(max(sizes)) - 1                 # greedy rounds of the largest instance: the launch's critical path
        row = {"shape": name, "graphs": len(sizes), "n": [int(min(sizes)), int(max(sizes))], "M": int(b.M), "d": d,
               "T": a.timesteps, "arith": model["gnn"].active_arith(),
               "forward_graph_ms": round(graph[0], 4), "forward_graph_min_ms": round(graph[1], 4),
               "forward_eager_ms": round(eager[0], 4), "decode_ms": round(decode[0], 4),
               "decode_min_ms": round(decode[1], 4), "decode_us_per_round": round(1e3 * decode[0] / rounds, 3),
               "decode_over_forward": round(decode[0] / graph[0], 4)}
        if a.beam:
            scores = tspgnn.edge_scores(votes)
            row["scores_ms"] = round(windows(lambda: tspgnn.edge_scores(votes), a.reps, a.inner)[0], 4)
            row["beam"] = {}
            for width in (int(k) for k in a.beam.split(",")):
                launches = len(tspgnn.decode.beam_ranges(len(sizes), int(max(sizes)), width)[0])
                inner = max(1, a.inner // (1 + width // 64))     # wide beams run for milliseconds: shorter windows
                for select in ("score", "cost"):
                    for _ in range(2):
                        out = tspgnn.beam_tours(b, scores, width, select)
                    torch.cuda.synchronize()
                    assert int((out.n_missing != 0).sum()) == 0 and int((out.n_closed <= 0).sum()) == 0
                    t = windows(lambda: tspgnn.beam_tours(b, scores, width, select), a.reps, inner)
                    row["beam"]["%d/%s" % (width, select)] = {"ms": round(t[0], 4), "min_ms": round(t[1], 4),
                                                              "launches": launches,
                                                              "over_forward": round(t[0] / graph[0], 3),
                                                              "mean_cost": round(float(out.costs.mean()), 4)}
            row["greedy_mean_cost"] = round(float(dec.costs.mean()), 4)
        if guides:
            if name != "trained":       # synthetic_batch's own instances
                rng = np.random.RandomState(1234)
                instances = [tspgnn.random_instance(int(n), rng) for n in sizes]
            v0 = np.concatenate([[0], np.cumsum(n_vertices)])
            tours = dec.tours.cpu().numpy()
            decoded = [[int(v) for v in tours[v0[i]:v0[i + 1]]] for i in range(len(sizes))]
            row["greedy_mean_cost"] = round(float(dec.costs.mean()), 4)
            row["polish"] = {"restarts": a.restarts, "kicks": a.kicks}
            row["guide"] = {}
            for g in guides:
                for _ in range(3):
                    tab = tspgnn.vote_neighbors(b, votes, g[0], g[1])
                torch.cuda.synchronize()
                t = windows(lambda: tspgnn.vote_neighbors(b, votes, g[0], g[1]), a.reps, a.inner)
                row["guide"]["%d,%d" % g] = {"rows_ms": round(t[0], 4), "rows_min_ms": round(t[1], 4),
                                             "rows_over_forward": round(t[0] / graph[0], 4),
                                             "polish": polish_ways(instances, decoded, tab.cpu().numpy(), v0, g,
                                                                   a.restarts, a.kicks)}
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.beam or guides else "w") as out:
        out.write("# tools/decode_bench.py --shapes %s --reps %d --inner %d%s%s: ms per call, median and min over the windows\n"
                  % (a.shapes, a.reps, a.inner, " --beam " + a.beam if a.beam else "",
                     "".join(" --guide " + g for g in a.guide)
                     + (" --restarts %d --kicks %d" % (a.restarts, a.kicks) if guides else "")))
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
