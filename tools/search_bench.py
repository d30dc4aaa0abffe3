#!/usr/bin/env python
"""Tour-cost search throughput: the sequential get_cost loop of experiments/binary_search.py against the batched
tspgnn.get_costs, on that experiment's shape (512 instances, n in [20, 40], d = 64, T = 32), for parallel = 1 and 8.

    python tools/search_bench.py [--instances 512] [--prefix 32] [--parallel 1 8]

The sequential figure is measured on a fixed prefix of --prefix instances and reported per instance (it is not
extrapolated to the whole set).  get_costs is timed over the whole set after one warm-up call (the warm-up call builds
the packed-weight caches); its time includes packing, upload and capturing each chunk's round.  "rounds" is the sum
over chunks of the chunk's largest iteration count (= replays), "ms/round" the timed call divided by it, and "forward
ms" one replay of a bare captured forward over the first chunk's batch -- the part of a round that is the network.
Untrained (random, perturbed) weights: the numbers measure the mechanics, not the costs found.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsp-gnn_amd")):
    sys.path.insert(0, p)
import tspgnn  # noqa: E402
from tspgnn.binary_search import DEFAULT_MAX_GRAPHS, plan_chunks  # noqa: E402
from oracle import params as P  # noqa: E402


def forward_ms(sess, model, chunk, T, k, reps=20):
    EV, W, C, r, nv, ne = tspgnn.InstanceLoader.create_batch([x for x in chunk for _ in range(k)], target_cost=0.0)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: r,
            model["n_vertices"]: nv, model["n_edges"]: ne}
    replay = sess.capture_forward(sess.prepare(feed))
    replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=512)
    ap.add_argument("--prefix", type=int, default=32)
    ap.add_argument("--parallel", type=int, nargs="+", default=[1, 8])
    ap.add_argument("-d", type=int, default=64)
    ap.add_argument("-T", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0, help="instances")
    ap.add_argument("--param-seed", type=int, default=3,
                    help="untrained weights whose answer crosses the threshold inside the bracket")
    a = ap.parse_args()
    rng = np.random.RandomState(a.seed)
    insts = [tspgnn.random_instance(int(n), rng) for n in rng.randint(20, 41, size=a.instances)]
    model = tspgnn.build_network(a.d)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer())
    model.store.load(P.init_params(a.d, seed=a.param_seed, perturb=True))
    summary = {"instances": a.instances, "d": a.d, "T": a.T, "prefix": a.prefix, "param_seed": a.param_seed, "runs": []}
    for k in a.parallel:
        prefix = insts[:a.prefix]
        tspgnn.get_cost(sess, model, prefix[0], a.T, parallel=k)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = [tspgnn.get_cost(sess, model, x, a.T, parallel=k) for x in prefix]
        seq_s = (time.perf_counter() - t0) / len(prefix)
        tspgnn.get_costs(sess, model, insts, a.T, parallel=k)                 # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tspgnn.get_costs(sess, model, insts, a.T, parallel=k)
        bat_s = time.perf_counter() - t0
        plan = plan_chunks(len(insts), k, DEFAULT_MAX_GRAPHS)
        iters = np.array([r[3] for r in res])
        rounds = int(sum(iters[s:e].max() for s, e in plan))
        same = sum(r[0] == float(q[0]) and r[3] == q[3] for r, q in zip(res[:a.prefix], seq))
        fwd = forward_ms(sess, model, insts[plan[0][0]:plan[0][1]], a.T, k)
        run = {"parallel": k, "chunks": len(plan), "graphs_per_chunk": (plan[0][1] - plan[0][0]) * k,
               "sequential_ms_per_instance": round(seq_s * 1e3, 3), "sequential_instances_per_s": round(1 / seq_s, 1),
               "batched_s": round(bat_s, 4), "batched_instances_per_s": round(len(insts) / bat_s, 1),
               "speedup": round(len(insts) / bat_s * seq_s, 1), "rounds": rounds,
               "ms_per_round": round(bat_s * 1e3 / rounds, 3), "forward_ms": round(fwd, 3),
               "iterations_min": int(iters.min()), "iterations_max": int(iters.max()),
               "iterations_hist": {int(v): int(c) for v, c in zip(*np.unique(iters, return_counts=True))},
               "prefix_equal_to_get_cost": "%d/%d" % (same, len(prefix))}
        summary["runs"].append(run)
        print("parallel=%d: sequential %.2f ms/instance (%.1f inst/s, %d-instance prefix) | get_costs %.1f inst/s over "
              "%d instances, %d chunk(s) of %d graphs, %d rounds, %.2f ms/round (bare forward %.2f ms) | x%.1f | "
              "iterations %d..%d | prefix equal %s"
              % (k, seq_s * 1e3, 1 / seq_s, len(prefix), len(insts) / bat_s, len(insts), len(plan),
                 run["graphs_per_chunk"], rounds, run["ms_per_round"], fwd, run["speedup"], iters.min(), iters.max(),
                 run["prefix_equal_to_get_cost"]), flush=True)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
