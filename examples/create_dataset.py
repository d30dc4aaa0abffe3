"""Create a labelled dataset of .graph files on the GPU: the reference's dataset.py command line (dataset.py:189-214).

    python examples/create_dataset.py -path instances/train -samples 32768 -nmin 20 -nmax 40 [-seed 42]
        [-distances euc_2D|random] [--metric] [-cmin 1] [-cmax 1] [--require-certified DEV] [-exact] [-neighbors K]
        [-closure host|device] [-writer host|device]

Unlike the reference's __main__, -seed is applied: random and np.random are seeded with it before the first draw, so
the instance stream is the one the reference's train.py gets after its own seeding (train.py seeds both the same way).
Instances of up to 256 vertices are labelled (tspgnn.label_tours).
-exact proves every tour of up to 128 vertices optimal by branch and bound (tspgnn.prove_tours), or improves it first,
and reports how many it proved within its node budget.
-neighbors K restricts the search's descent to moves between K nearest neighbours (1..32; tspgnn.label_tours).
--metric, as in the reference, turns the metric closure OFF for random distances.
-closure device takes that closure on the GPU (tspgnn.metric_closure) instead of in NumPy: the same files, byte for byte.
-writer device formats the .graph files on the GPU instead of in write_graph: the same files, byte for byte.
"""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tsp-gnn_amd"))

import numpy as np  # noqa: E402

from tspgnn import dataset  # noqa: E402


def main():
    p = argparse.ArgumentParser(description="Create labelled TSP instances (GPU tour search + Held-Karp bounds).")
    p.add_argument("-seed", type=int, default=42, help="RNG seed for Python and NumPy")
    p.add_argument("-distances", default="euc_2D", help="What type of distances? (euc_2D or random)")
    p.add_argument("--metric", const=False, default=True, action="store_const", help="Create metric instances?")
    p.add_argument("-samples", default=2 ** 10, type=int, help="How many samples?")
    p.add_argument("-path", help="Save path", required=True)
    p.add_argument("-nmin", default=20, type=int, help="Min. number of vertices")
    p.add_argument("-nmax", default=40, type=int, help="Max. number of vertices")
    p.add_argument("-cmin", default=1, type=float, help="Min. connectivity")
    p.add_argument("-cmax", default=1, type=float, help="Max. connectivity")
    p.add_argument("--require-certified", type=float, default=None, metavar="DEV",
                   help="redraw instances whose labels cannot be certified at this dev (biases the distribution)")
    p.add_argument("-exact", action="store_true",
                   help="prove the tours optimal by branch and bound (n <= 128), as Concorde does for the reference")
    p.add_argument("-neighbors", type=int, default=None, metavar="K",
                   help="candidate-list descent over the K nearest neighbours (1..32; default: the full scan)")
    p.add_argument("-closure", default="host", choices=("host", "device"),
                   help="where the metric closure of random distances is taken (the files are the same bytes)")
    p.add_argument("-writer", default="host", choices=("host", "device"),
                   help="who formats the .graph files: write_graph, or the GPU (the files are the same bytes)")
    a = p.parse_args()
    random.seed(a.seed)
    np.random.seed(a.seed)
    print("Creating {} instances".format(a.samples), flush=True)
    s = dataset.create_dataset(a.path, a.nmin, a.nmax, a.cmin, a.cmax, samples=a.samples, distances=a.distances,
                               metric=a.metric, require_certified=a.require_certified, verbose=True, exact=a.exact,
                               neighbors=a.neighbors, closure=a.closure, writer=a.writer)
    t = s["times"]
    if "closure" in t:
        print("closure (%s) %.2f s" % (a.closure, t["closure"]), flush=True)
    print("search %.2f s, bound %.2f s, write %.2f s; certified fraction %.4f; gap median %.5f max %.5f; redrawn %d"
          % (t["search"], t.get("bound", 0.0), t["write"], s["certified_fraction"], float(np.median(s["gap"])),
             float(s["gap"].max()), s["redrawn"]), flush=True)
    if a.exact:
        print("exact %.2f s; proved optimal %d of %d; nodes median %d max %d"
              % (t.get("exact", 0.0), int(s["proved"].sum()), a.samples, int(np.median(s["nodes"])),
                 int(s["nodes"].max())), flush=True)


if __name__ == "__main__":
    main()
