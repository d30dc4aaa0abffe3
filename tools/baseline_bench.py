"""Times the decision-TSP baselines (tspgnn.baselines) at the shapes of tools/dataset_bench.py: the test set (2^10
instances, n 20-40), n = 80 and n = 200.  Per shape the instances are labelled once with label_tours; then nearest
neighbour (from vertex 0 and the best start) and annealing over a grid of t_hot x sweeps are timed and scored: seconds,
the median relative gap of the tour to label_tours' cost, and tpr at dev = 0.02 (the share of instances whose tour is
feasible and costs at most 1.02 Q, Q the label's target).  One JSON line per row.

    python tools/baseline_bench.py [--shapes test,n80,n200] [--samples N] [--t-hot 0.05,0.1] [--sweeps 1,2,4]
                                   [--t-cold-ratio 0.02] [--levels L] [--chains C]

Without --t-hot / --sweeps the annealing runs its defaults alone.
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tspgnn import baselines, dataset  # noqa: E402

SHAPES = {"test": (2 ** 10, 20, 40), "n80": (2 ** 10, 80, 80), "n200": (2 ** 10, 200, 200), "n256": (2 ** 10, 256, 256)}


def score(res, labels, dev=0.02):
    cost = np.array([r.cost for r in res])
    ref = np.array([r.cost for r in labels])
    Q = np.array([r.target for r in labels])
    return {"gap_median": float(np.median(cost / ref - 1.0)), "gap_p90": float(np.percentile(cost / ref - 1.0, 90)),
            "feasible": float(np.mean([r.feasible for r in res])),
            "tpr_%g" % dev: float(baselines.decide(res, (1.0 + dev) * Q).mean())}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="test,n80,n200")
    ap.add_argument("--samples", type=int, default=0, help="override the instance count of every shape")
    ap.add_argument("--t-hot", default=None, help="comma-separated multiples of the mean edge weight")
    ap.add_argument("--sweeps", default=None, help="comma-separated proposals per level in units of n^2")
    ap.add_argument("--t-cold-ratio", type=float, default=None, help="t_cold = ratio * t_hot (default: the default pair's)")
    ap.add_argument("--levels", type=int, default=baselines.DEFAULT_LEVELS)
    ap.add_argument("--chains", type=int, default=baselines.DEFAULT_CHAINS)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "baseline_bench needs an MI355X"
    ratio = a.t_cold_ratio if a.t_cold_ratio is not None else baselines.DEFAULT_T_COLD / baselines.DEFAULT_T_HOT
    t_hots = [float(x) for x in a.t_hot.split(",")] if a.t_hot else [baselines.DEFAULT_T_HOT]
    sweeps = [float(x) for x in a.sweeps.split(",")] if a.sweeps else [baselines.DEFAULT_SWEEPS]
    # warm-up: load the code objects outside the timed runs
    for n in (20, 130):
        warm = [(np.triu(np.ones((n, n)), 1), np.random.RandomState(0).rand(n, n))]
        baselines.nearest_neighbor_tours(warm, start="best")
        baselines.anneal_tours(warm, levels=1, sweeps=1)
        dataset.label_tours(warm, kicks=1, lower_bound=False)
    for name in a.shapes.split(","):
        samples, nmin, nmax = SHAPES[name]
        samples = a.samples or samples
        random.seed(1)
        np.random.seed(1)
        graphs = dataset.draw_instances(nmin, nmax, samples=samples)
        insts = [(g[0], g[1]) for g in graphs]
        labels, t_label = timed(lambda: dataset.label_tours(insts, init_tours=[g[2] for g in graphs], lower_bound=False))
        head = {"shape": name, "samples": samples, "n": [nmin, nmax]}
        print(json.dumps(dict(head, method="label_tours", seconds=round(t_label, 3))), flush=True)
        for start in (0, "best"):
            res, t = timed(lambda: baselines.nearest_neighbor_tours(insts, start=start))
            print(json.dumps(dict(head, method="nn", start=start, seconds=round(t, 3), **score(res, labels))), flush=True)
        for th in t_hots:
            for sw in sweeps:
                tm = {}
                res, t = timed(lambda: baselines.anneal_tours(insts, chains=a.chains, levels=a.levels, sweeps=sw, t_hot=th,
                                                              t_cold=ratio * th, seed=a.seed, timings=tm))
                print(json.dumps(dict(head, method="sa", chains=a.chains, levels=a.levels, sweeps=sw, t_hot=th,
                                      t_cold=ratio * th, seconds=round(t, 3), kernel_s=round(tm["anneal"], 3),
                                      **score(res, labels))), flush=True)


if __name__ == "__main__":
    main()
