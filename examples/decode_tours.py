#!/usr/bin/env python
"""A tour per instance from the network's edge votes (tspgnn.decode_tours): the network's own cost estimate from
get_costs, a forward at that target, the greedy decoder on the GPU, and optionally one descent of the tour search from
the decoded tour.

    python examples/decode_tours.py --synthetic 64 --polish --out results/decoded-tours.dat
    python examples/decode_tours.py --instances instances/test --checkpoint training/dev=0.02/checkpoints/epoch=100 \\
                                    --write-graphs decoded/

Instances come from a directory of .graph files or are synthetic Euclidean graphs (n in [20, 40]); weights from a
TensorFlow-format checkpoint or a random initialisation -- untrained weights exercise the mechanics only, their tours
mean nothing.  One line per instance, tab-separated: n, the cost of the route the instance carries (nan when it has
none), the network's cost estimate, the decoded tour's cost, its pairs that are not edges (n_missing), and the polished
cost (nan without --polish); all costs unnormalised.  --write-graphs DIR writes every instance back as DIR/k.graph with
the decoded (or polished) tour in its TOUR_SECTION.  How good a decoded tour is, is an observation, not a guarantee.

-beam K decodes by beam search of width K (1 .. 1024) instead of greedy edge insertion, -select cost keeps the cheapest
closed tour of the last beam instead of the best-scoring one; two more columns then follow: the tour's integer score and
the number of closed entries of the last beam.

    python examples/decode_tours.py --synthetic 32 -beam 128 -select cost --polish

-guide K[,KN] (with -polish) lets the polish add only edges that the votes rank: per vertex its K best-voted neighbours,
then the KN nearest of the rest (tspgnn.vote_neighbors; decode_tours(guide=(K, KN))).

    python examples/decode_tours.py --synthetic 32 -polish -guide 4,4

-votes route decodes from E_route, the head trained on the labelled tours' edges, instead of the decision's E_vote: the
network is then built with route_head=True, and a checkpoint without the head leaves it as initialised.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
from tspgnn import (InstanceLoader, Session, build_network, decode_tours, get_costs,  # noqa: E402
                    global_variables_initializer, load_weights, random_instance, read_graph, write_graph)


def load_instances(a):
    if a.instances:
        names = sorted(InstanceLoader(a.instances).filenames)
        return [read_graph(f) for f in (names[:a.limit] if a.limit else names)]
    rng = np.random.RandomState(a.seed)
    return [random_instance(int(n), rng) for n in rng.randint(20, 41, size=a.synthetic)]


def cycle_cost(Mw, route):
    if len(route) != Mw.shape[0]:
        return float("nan")
    return float(sum(Mw[min(i, j), max(i, j)] for i, j in zip(route, route[1:] + route[:1])))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-d", default=64, type=int)
    p.add_argument("-timesteps", default=32, type=int)
    p.add_argument("--instances", default=None, help="directory of .graph files")
    p.add_argument("--limit", default=0, type=int, help="first N files of --instances (0: all)")
    p.add_argument("--synthetic", default=64, type=int, help="number of synthetic instances without --instances")
    p.add_argument("--checkpoint", default=None, help="TensorFlow-format checkpoint directory .../epoch=N")
    p.add_argument("-beam", default=None, type=int, help="beam width, 1 .. 1024 (default: the greedy decoder)")
    p.add_argument("-select", default="score", choices=["score", "cost"], help="with -beam: what the last beam is chosen by")
    p.add_argument("--polish", "-polish", action="store_true", help="one descent of the tour search from every decoded tour")
    p.add_argument("-guide", default=None, help="K[,KN]: with -polish, candidate rows from the votes (K + KN <= 32)")
    p.add_argument("-votes", default="decision", choices=["decision", "route"],
                   help="which per-edge logits the decoders read: E_vote (decision) or the route head's E_route")
    p.add_argument("--max-rounds", default=1100, type=int, help="bisection rounds of the cost estimate (see binary_search.py)")
    p.add_argument("--write-graphs", default=None, help="directory for the instances with their decoded tours")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--out", default="decoded-tours.dat")
    a = p.parse_args(argv)

    instances = load_instances(a)
    model = build_network(a.d, route_head=a.votes == "route")
    sess = Session(model)
    sess.run(global_variables_initializer(seed=a.seed))
    if a.checkpoint:
        load_weights(sess, a.checkpoint, missing_ok=a.votes == "route")
    # decode_tours(target_costs=None) runs this same search with its default round limit; untrained weights need more
    estimates = [r[0] for r in get_costs(sess, model, instances, a.timesteps, max_rounds=a.max_rounds)]
    beam_kw = {} if a.beam is None else {"beam": a.beam, "select": a.select}
    if a.guide is not None:
        beam_kw["guide"] = tuple(int(k) for k in (a.guide + ",0").split(",")[:2])
    if a.votes != "decision":
        beam_kw["votes"] = a.votes
    res = decode_tours(sess, model, instances, a.timesteps, target_costs=estimates, polish=a.polish, **beam_kw)
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as out:
        for (Ma, Mw, route), r in zip(instances, res):
            n = Ma.shape[0]
            polished = float("nan") if r.polished_cost is None else r.polished_cost
            more = "" if a.beam is None else "\t{}\t{}".format(r.score, r.n_closed)
            out.write("{}\t{}\t{}\t{}\t{}\t{}{}\n".format(n, cycle_cost(Mw, [int(v) for v in route]), n * r.target_cost,
                                                            r.cost, r.n_missing, polished, more))
    if a.write_graphs:
        os.makedirs(a.write_graphs, exist_ok=True)
        for k, ((Ma, Mw, _), r) in enumerate(zip(instances, res)):
            write_graph(np.triu(Ma), Mw, os.path.join(a.write_graphs, "%d.graph" % k),
                        route=r.polished_tour if a.polish else r.tour)
    feasible = sum(r.feasible for r in res)
    print("%d instances, %d decoded tours feasible; wrote %s" % (len(res), feasible, a.out))
    carried = np.array([cycle_cost(Mw, [int(v) for v in route]) for _, Mw, route in instances])
    if np.isfinite(carried).any():      # the observation of DESIGN section 12: cost over the cost of the carried route
        ratio = np.array([r.cost for r in res]) / carried
        line = "decoded / carried route: mean %.3f, min %.3f, max %.3f" % (np.nanmean(ratio), np.nanmin(ratio),
                                                                          np.nanmax(ratio))
        if a.polish:
            line += "; polished: mean %.3f" % np.nanmean(np.array([r.polished_cost for r in res]) / carried)
        print(line)
    return res


if __name__ == "__main__":
    main()
