#!/usr/bin/env python
"""Tour-cost estimation with a decision network: every instance's target cost bisected until its bracket is within
``-delta`` (the experiment of the reference's experiments/binary_search.py), all instances at once with
tspgnn.get_costs.

    python examples/binary_search.py --synthetic 512 --out results/binary-search.dat
    python examples/binary_search.py --instances instances/test --checkpoint training/dev=0.02/checkpoints/epoch=100

Instances come from a directory of .graph files (InstanceLoader) or are synthetic Euclidean graphs (n in [20, 40]);
weights from a TensorFlow-format checkpoint (load_weights) or a random initialisation -- untrained weights exercise the
mechanics only, their costs mean nothing.  One line per instance, tab-separated: n, predicted cost, prediction at the
final bracket, real (route) cost, relative deviation, iterations; the mean |deviation| is printed at the end.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
from tspgnn import (InstanceLoader, Session, build_network, get_costs, global_variables_initializer,  # noqa: E402
                    load_weights, random_instance, read_graph)


def load_instances(a):
    if a.instances:
        loader = InstanceLoader(a.instances)
        names = sorted(loader.filenames)
        if a.limit:
            names = names[:a.limit]
        return [read_graph(f) for f in names]
    rng = np.random.RandomState(a.seed)
    return [random_instance(int(n), rng) for n in rng.randint(20, 41, size=a.synthetic)]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-d", default=64, type=int)
    p.add_argument("-timesteps", default=32, type=int)
    p.add_argument("-threshold", default=0.5, type=float)
    p.add_argument("-delta", default=0.01, type=float, help="stopping_delta: relative width of the final bracket")
    p.add_argument("--parallel", default=1, type=int, help="probe copies of each instance per round")
    p.add_argument("--instances", default=None, help="directory of .graph files")
    p.add_argument("--limit", default=0, type=int, help="first N files of --instances (0: all)")
    p.add_argument("--synthetic", default=64, type=int, help="number of synthetic instances without --instances")
    p.add_argument("--checkpoint", default=None, help="TensorFlow-format checkpoint directory .../epoch=N")
    p.add_argument("--max-rounds", default=1100, type=int,
                   help="bisection rounds before giving up (untrained weights that accept every cost drive the bracket's "
                        "upper end down to its lower end, 0: ~1 075 halvings)")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--out", default="binary-search.dat")
    a = p.parse_args(argv)

    instances = load_instances(a)
    model = build_network(a.d)
    sess = Session(model)
    sess.run(global_variables_initializer(seed=a.seed))
    if a.checkpoint:
        load_weights(sess, a.checkpoint)
    t0 = time.perf_counter()
    results = get_costs(sess, model, instances, a.timesteps, threshold=a.threshold, stopping_delta=a.delta,
                        parallel=a.parallel, max_rounds=a.max_rounds)
    elapsed = time.perf_counter() - t0
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    total_dev = 0.0
    with open(a.out, "w") as out:
        for (Ma, _, _), (pred_cost, pred, real_cost, iterations) in zip(instances, results):
            deviation = (pred_cost - real_cost) / real_cost
            total_dev += abs(deviation)
            prob = float("nan") if pred is None else float(pred[0])
            out.write("{}\t{}\t{}\t{}\t{}\t{}\n".format(Ma.shape[0], pred_cost, prob, real_cost, deviation, iterations))
    iters = [r[3] for r in results]
    print("%d instances in %.3f s (%.1f instances/s), iterations %d..%d; mean |deviation| %.4f%%; wrote %s"
          % (len(results), elapsed, len(results) / elapsed, min(iters), max(iters),
             100 * total_dev / max(len(results), 1), a.out))
    return results


if __name__ == "__main__":
    main()
