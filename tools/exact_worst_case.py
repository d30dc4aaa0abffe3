"""Worst-case seconds of one tspgnn_tour_branch_bound launch at the default budget: complete graphs with weights from
{1, 2, 3} are all ties, so a large share of the instances exhausts max_nodes and the longest of them sets the launch's
time.  Prints the launch seconds, the share that ran out of budget and the nodes per shape.

    python tools/exact_worst_case.py [--shapes 20:1024,40:1024,128:256,128:1024] [--max-nodes N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))

import numpy as np  # noqa: E402

from tspgnn import dataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20:1024,40:1024,128:256,128:1024", help="n:count, comma-separated")
    ap.add_argument("--max-nodes", type=int, default=dataset.DEFAULT_BB_NODES)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        n, count = (int(x) for x in shape.split(":"))
        rng = np.random.RandomState(n)
        insts = [(np.triu(np.ones((n, n)), 1), np.triu(rng.randint(1, 4, size=(n, n)).astype(float), 1))
                 for _ in range(count)]
        incs = [dataset.TourResult(list(range(n)), 0.0, 0.0, True, 0.0) for _ in range(count)]
        for rep in range(2):   # the first repetition loads the code object
            stats = {}
            t0 = time.perf_counter()
            dataset.prove_tours(insts, incs, max_nodes=a.max_nodes, stats=stats)
            wall = time.perf_counter() - t0
            nd = stats["nodes"]
            print("n=%d count=%d rep=%d: launch %.3f s (wall %.2f); budget fraction %.3f; nodes mean %.0f max %d"
                  % (n, count, rep, stats["seconds"], wall, np.mean(stats["status"] == "budget"), nd.mean(), nd.max()),
                  flush=True)


if __name__ == "__main__":
    main()
