"""The measurement routines of the reference's experiment scripts on the MI355X path, without the plotting:
``get_predictions`` (/root/reference/experiments/acceptance_curve.py:19-37), ``get_accuracy``
(experiments/test_varying_sizes.py:20-38, test_varying_dev.py) and the two sweeps built on them.  Each keeps the
reference's feed / fetch; the sweeps call them exactly like the scripts' loops (acceptance_curve.py:87-99,
test_varying_sizes.py:82-114).  ``baseline_curve`` is the measurement behind figures/test_varying_dev_baseline.png, for
which the reference has no script: the decision-TSP predictor built on a nearest-neighbour or annealing tour
(tspgnn/baselines.py); ``decoded_tour_curve`` is the same measurement on the tour decoded from the network's own edge
votes (tspgnn/decode.py)."""
from itertools import islice

import numpy as np


def _feed(model, batch, time_steps):
    EV, W, C, route_exists, n_vertices, n_edges = batch[0], batch[1], batch[2], batch[-3], batch[-2], batch[-1]
    return {model['EV']: EV, model['W']: W, model['C']: C, model['time_steps']: time_steps,
            model['route_exists']: route_exists, model['n_vertices']: n_vertices, model['n_edges']: n_edges}


def get_predictions(sess, model, batch, time_steps):
    """``batch``: the 6-tuple of create_batch (a 7-tuple with an edges_mask in fourth place is accepted, as in
    acceptance_curve.py:21)."""
    return sess.run(model['predictions'], feed_dict=_feed(model, batch, time_steps))


def get_accuracy(sess, model, batch, time_steps):
    return np.mean(sess.run(model['acc'], feed_dict=_feed(model, batch, time_steps)))


def acceptance_curve(sess, model, loader, time_steps, deviations, batch_size=16, max_batches=64):
    """Mean prediction as a function of the target-cost deviation (acceptance_curve.py:87-99): for every deviation
    the loader is rewound and up to ``max_batches`` batches (every instance twice: (1-dev) and (1+dev) times its
    tour cost) are scored.  Returns an array of len(deviations) means."""
    out = np.zeros(len(deviations))
    for i, dev in enumerate(deviations):
        loader.reset()
        preds = [get_predictions(sess, model, b, time_steps) for b in islice(loader.get_batches(batch_size, dev), max_batches)]
        out[i] = np.mean(np.concatenate(preds)) if preds else np.nan
    return out


def accuracy_by_size(sess, model, loaders, time_steps, dev, batch_size=16, max_batches=64):
    """{n: accuracy} over per-size instance loaders (test_varying_sizes.py:82-114)."""
    result = {}
    for n, loader in loaders.items():
        loader.reset()
        accs = [get_accuracy(sess, model, b, time_steps) for b in islice(loader.get_batches(batch_size, dev), max_batches)]
        result[n] = float(np.mean(accs)) if accs else float('nan')
    return result


def curve_from_costs(cost, feasible, Q, deviations):
    """The arithmetic of baseline_curve: a predictor that answers yes iff its tour is feasible and costs at most C, scored
    on the two copies create_batch makes of every instance, C = (1 + dev) Q (label 1) and C = (1 - dev) Q (label 0).
    Returns {'tpr', 'fpr', 'acc'} arrays over the deviations, acc = (tpr + 1 - fpr) / 2."""
    cost, Q = np.asarray(cost, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    feasible = np.asarray(feasible, dtype=bool)
    tpr, fpr = np.zeros(len(deviations)), np.zeros(len(deviations))
    for i, dev in enumerate(deviations):
        tpr[i] = np.mean(feasible & (cost <= (1.0 + dev) * Q)) if cost.size else np.nan
        fpr[i] = np.mean(feasible & (cost <= (1.0 - dev) * Q)) if cost.size else np.nan
    return {"tpr": tpr, "fpr": fpr, "acc": (tpr + 1.0 - fpr) / 2.0}


def baseline_curve(instances_or_loader, deviations, method="nn", **solver_kw):
    """Accuracy of a classical heuristic as a decision-TSP predictor, per target-cost deviation.

    instances_or_loader: a list of (Ma, Mw, route) as read_graph returns them, or an InstanceLoader (every file once).
    method: "nn" (baselines.nearest_neighbor_tours) or "sa" (baselines.anneal_tours); solver_kw go to the solver.  Every
    instance is solved once; for each deviation the tour is thresholded against C = (1 +/- dev) Q, with Q the target cost
    create_batch derives from the file's route (dataset._target).  Returns {'tpr', 'fpr', 'acc', 'deviations'}: tpr is
    the share of the (1 + dev) copies answered yes, fpr the share of the (1 - dev) copies answered yes -- nonzero only
    through the closing-pair quirk of Q or a label that is not optimal -- and acc = (tpr + 1 - fpr) / 2."""
    from . import baselines, dataset
    from .instance_loader import read_graph
    if hasattr(instances_or_loader, "filenames"):
        instances = [read_graph(f) for f in instances_or_loader.filenames]
    else:
        instances = list(instances_or_loader)
    if method not in ("nn", "sa"):
        raise ValueError("method=%r must be 'nn' or 'sa'" % (method,))
    solve = baselines.nearest_neighbor_tours if method == "nn" else baselines.anneal_tours
    res = solve([(Ma, Mw) for Ma, Mw, _ in instances], **solver_kw)
    Q = np.array([dataset._target(Ma, Mw, [int(v) for v in route]) for Ma, Mw, route in instances])
    out = curve_from_costs([r.cost for r in res], [r.feasible for r in res], Q, deviations)
    out["deviations"] = np.asarray(deviations, dtype=np.float64)
    return out


def decoded_tour_curve(sess, model, instances_or_loader, time_steps, deviations, polish=False, **decode_kw):
    """baseline_curve with the network as the constructive heuristic: the tour decoded from its edge votes at its own cost
    estimate (decode.decode_tours with target_costs=None, so no label enters), or with polish=True that tour after one
    descent of the tour search, thresholded against C = (1 +/- dev) Q like a nearest-neighbour or annealing tour.  The
    decoded cost counts only when the tour is feasible (n_missing == 0).  decode_kw go to decode_tours -- votes="route"
    among them: the curve of the tours decoded from the route head's E_route instead of E_vote.  Returns
    {'tpr', 'fpr', 'acc', 'deviations'} as baseline_curve does."""
    from . import dataset, decode
    from .instance_loader import read_graph
    if hasattr(instances_or_loader, "filenames"):
        instances = [read_graph(f) for f in instances_or_loader.filenames]
    else:
        instances = list(instances_or_loader)
    res = decode.decode_tours(sess, model, instances, time_steps, polish=polish, **decode_kw)
    Q = np.array([dataset._target(Ma, Mw, [int(v) for v in route]) for Ma, Mw, route in instances])
    if polish:
        edge = [dataset._edge_mask(Ma) for Ma, _, _ in instances]
        cost = [r.polished_cost for r in res]
        feasible = [all(A[a, b] for a, b in zip(r.polished_tour, r.polished_tour[1:] + r.polished_tour[:1]))
                    for A, r in zip(edge, res)]
    else:
        cost, feasible = [r.cost for r in res], [r.feasible for r in res]
    out = curve_from_costs(cost, feasible, Q, deviations)
    out["deviations"] = np.asarray(deviations, dtype=np.float64)
    return out
