#!/usr/bin/env python
"""Accuracy of two classical heuristics as decision-TSP predictors, per target-cost deviation: the measurement behind
the reference's figures/test_varying_dev_baseline.png (nearest neighbour and simulated annealing over 2-exchange moves
beside the trained model).  A heuristic answers "is there a tour of cost at most C?" with yes iff its own tour is
feasible and costs at most C.

    python examples/baseline_curve.py --synthetic 256 -devs 0.01,0.02,0.05,0.1
    python examples/baseline_curve.py --instances instances/test -checkpoint training/dev=0.02/checkpoints/epoch=100

Instances come from a directory of .graph files or are synthetic Euclidean graphs (n in [20, 40]) labelled with
label_tours.  One line per deviation, tab-separated: dev, then tpr / fpr / acc of nearest neighbour, then of annealing;
with -checkpoint a last column has the network's accuracy at that deviation (experiments.get_accuracy, as the
reference's test_varying_dev.py measures it), and with -decoded one more: the accuracy of the tour decoded from the
network's edge votes at its own cost estimate, scored like the two heuristics (experiments.decoded_tour_curve); -beam K
decodes that tour by beam search of width K instead of greedy edge insertion.
"""
import argparse
import os
import sys
import tempfile
from itertools import islice

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
from tspgnn import (InstanceLoader, Session, build_network, experiments, global_variables_initializer,  # noqa: E402
                    label_tours, load_weights, random_instance, read_graph, write_graph)


def load_instances(a):
    if a.instances:
        names = sorted(InstanceLoader(a.instances).filenames)
        return [read_graph(f) for f in (names[:a.limit] if a.limit else names)]
    rng = np.random.RandomState(a.seed)
    graphs = [random_instance(int(n), rng) for n in rng.randint(20, 41, size=a.synthetic)]
    labels = label_tours([(Ma, Mw) for Ma, Mw, _ in graphs], init_tours=[r for _, _, r in graphs], lower_bound=False)
    return [(Ma, Mw, r.tour) for (Ma, Mw, _), r in zip(graphs, labels)]


def network_accuracy(a, instances, devs):
    """The network's accuracy per deviation through experiments.get_accuracy, on the instances written to a directory."""
    model = build_network(a.d)
    sess = Session(model)
    sess.run(global_variables_initializer(seed=a.seed))
    load_weights(sess, a.checkpoint)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, (Ma, Mw, route) in enumerate(instances):
            write_graph(np.triu(Ma), Mw, filepath=os.path.join(tmp, "%d.graph" % k), route=route)
        loader = InstanceLoader(tmp)
        for dev in devs:
            loader.reset()
            accs = [experiments.get_accuracy(sess, model, b, a.timesteps)
                    for b in islice(loader.get_batches(a.batch_size, dev), len(instances) // a.batch_size)]
            out.append(float(np.mean(accs)) if accs else float("nan"))
    return out


def decoded_curve(a, instances, devs):
    """The tour decoded from the network's edge votes as a decision-TSP predictor (experiments.decoded_tour_curve)."""
    model = build_network(a.d, route_head=a.votes == "route")
    sess = Session(model)
    sess.run(global_variables_initializer(seed=a.seed))
    load_weights(sess, a.checkpoint, missing_ok=a.votes == "route")
    beam_kw = {} if a.beam is None else {"beam": a.beam}
    if a.votes != "decision":
        beam_kw["votes"] = a.votes     # (decoded from E_route, the head trained on the tours' edges)
    return experiments.decoded_tour_curve(sess, model, instances, a.timesteps, devs, **beam_kw)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-devs", default="0.001,0.002,0.005,0.01,0.02,0.05,0.1,0.2", help="comma-separated deviations")
    p.add_argument("-d", default=64, type=int)
    p.add_argument("-timesteps", default=32, type=int)
    p.add_argument("-checkpoint", default=None, help="TensorFlow-format checkpoint directory .../epoch=N")
    p.add_argument("-decoded", action="store_true",
                   help="with -checkpoint: one more column, the accuracy of the tour decoded from the network's edge votes")
    p.add_argument("-beam", default=None, type=int,
                   help="with -decoded: decode by beam search of this width, 1 .. 1024 (default: greedy edge insertion)")
    p.add_argument("-votes", default="decision", choices=["decision", "route"],
                   help="with -decoded: decode from E_vote (decision) or from the route head's E_route")
    p.add_argument("--batch-size", default=16, type=int)
    p.add_argument("--instances", default=None, help="directory of .graph files")
    p.add_argument("--limit", default=0, type=int, help="first N files of --instances (0: all)")
    p.add_argument("--synthetic", default=256, type=int, help="number of synthetic instances without --instances")
    p.add_argument("--nn-start", default="0", help="nearest neighbour's start vertex, or 'best'")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--out", default="baseline-curve.dat")
    a = p.parse_args(argv)
    if a.decoded and not a.checkpoint:
        p.error("-decoded needs -checkpoint")
    if a.beam is not None and not a.decoded:
        p.error("-beam needs -decoded")

    devs = [float(x) for x in a.devs.split(",")]
    instances = load_instances(a)
    start = "best" if a.nn_start == "best" else int(a.nn_start)
    nn = experiments.baseline_curve(instances, devs, method="nn", start=start)
    sa = experiments.baseline_curve(instances, devs, method="sa", seed=a.seed)
    net = network_accuracy(a, instances, devs) if a.checkpoint else None
    decoded = decoded_curve(a, instances, devs) if a.decoded else None
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as out:
        for k, dev in enumerate(devs):
            cols = [dev] + [c[key][k] for c in (nn, sa) for key in ("tpr", "fpr", "acc")] + ([net[k]] if net else []) \
                + ([decoded["acc"][k]] if decoded else [])
            out.write("\t".join(str(x) for x in cols) + "\n")
    print("%d instances, %d deviations; accuracy at dev %g: nearest neighbour %.4f, annealing %.4f; wrote %s"
          % (len(instances), len(devs), devs[len(devs) // 2], nn["acc"][len(devs) // 2], sa["acc"][len(devs) // 2], a.out))
    return (nn, sa, net, decoded) if a.decoded else (nn, sa, net)


if __name__ == "__main__":
    main()
