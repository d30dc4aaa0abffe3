"""Per-batch driver of the MI355X path with the calling contract of the reference's ``run_batch`` /
``summarize_epoch`` (/root/reference/train.py:17-76): same argument lists, and ``run_batch`` returns the
8-tuple ``(loss, acc, mean label, mean prediction, TP, FP, TN, FN)`` a training script written against the
reference unpacks.  Everything else -- how the feed is assembled, what is logged and how -- is this
package's own.

In a data-parallel session (``Session(..., process_group=...)``) the statistics that come back are the ones
of the GLOBAL batch (``Session`` reduces them across ranks); the label / prediction means of
the tuple are reduced here the same way, so every rank returns identical numbers.
"""
import sys

import numpy as np

_FEED_ORDER = ("EV", "W", "C", "route_exists", "n_vertices", "n_edges")
_STAT_KEYS = ("loss", "acc", "predictions", "TP", "FP", "TN", "FN")


_ROUTE_KEYS = ("route_loss", "route_acc")


def _route_model(model):
    return bool(getattr(model, "route_head", False))


def _feed_for(model, batch, time_steps):
    """feed_dict of one ``InstanceLoader`` batch (a 6-tuple in ``_FEED_ORDER``).  For a route-head network the tuple may
    carry a seventh item, the per-edge route marks (tspgnn.route_edge_marks_host of the batch's instances): it feeds
    ``model['route_edges']``."""
    marked = _route_model(model) and len(batch) == len(_FEED_ORDER) + 1
    if len(batch) != len(_FEED_ORDER) and not marked:
        raise ValueError("run_batch: a batch is the 6-tuple (%s), got %d items" % (", ".join(_FEED_ORDER), len(batch)))
    feed = {model[key]: value for key, value in zip(_FEED_ORDER, batch)}
    feed[model["time_steps"]] = time_steps
    if marked:
        feed[model["route_edges"]] = batch[len(_FEED_ORDER)]
    return feed


def _route_fields(route_stats):
    """The log fields of a route-head batch: the local batch's route loss and edge accuracy (None: no marks, no fields)."""
    if route_stats is None:
        return ()
    return (("route_loss", "%.4f" % route_stats[0]), ("route_acc", "%.4f" % route_stats[1]))


def _batch_means(sess, labels, predictions):
    """(mean label, mean prediction): of this batch, or -- in a data-parallel session -- of the global batch
    (local sums and counts summed over the session's process group)."""
    if getattr(sess, "world_size", 1) <= 1:
        return np.mean(labels), np.mean(predictions)
    sums = sess.allreduce_host_sums(np.array(
        [np.sum(labels, dtype=np.float64), np.sum(predictions, dtype=np.float64), float(len(labels))]))
    count = max(sums[2], 1.0)
    return sums[0] / count, sums[1] / count


def _log(kind, epoch_i, fields):
    sys.stdout.write("[%s] epoch %d  %s\n" % (kind, epoch_i, "  ".join("%s=%s" % kv for kv in fields)))
    sys.stdout.flush()


def _run_device_batch(sess, batch, time_steps, train):
    """The fetches of run_batch over a batch that is already on the device (DeviceDataset.batch): what Session.run
    does with a feed -- the training step looks after the f16x2 range flag itself, a flagged forward is repeated on
    bf16x3, the statistics are those of the global batch -- without a feed to convert."""
    batch.T = int(time_steps)
    if train:
        out = sess.train_step(batch)
    else:
        out = sess._on_bf16x3_if_flagged(lambda: sess.forward(batch, global_stats=True))
    stats = out["stats"].cpu().numpy()
    values = {key: np.float32(stats[k]) for k, key in enumerate(("loss", "acc", "TP", "FP", "TN", "FN"))}
    values["predictions"] = out["predictions"].cpu().numpy()
    if "route_stats" in out:
        values["route_stats"] = out["route_stats"].cpu().numpy()
    return values


def run_batch(sess, model, batch, batch_i, epoch_i, time_steps, train=False, verbose=True):
    """One ``sess.run`` over ``batch``; with ``train`` the optimiser step is fetched first (train.py:36-42).  ``batch``:
    the create_batch 6-tuple, or a DeviceBatch of DeviceDataset.batch / get_batches (labels and counts from its host
    arrays).  A route-head network is fed the marks the batch has -- a DeviceBatch's ``route_edges``
    (DeviceDataset(routes=True), Session.mark_routes) or the tuple's seventh item -- and the line then shows the route loss
    and edge accuracy of this rank's batch beside the existing fields; the returned tuple is unchanged."""
    from .model import DeviceBatch
    if isinstance(batch, DeviceBatch):
        stats = _run_device_batch(sess, batch, time_steps, train)
        labels, n_vertices, n_edges = batch.route_exists, batch.n_vertices, batch.n_edges
    else:
        feed = _feed_for(model, batch, time_steps)
        keys = _STAT_KEYS + (_ROUTE_KEYS if _route_model(model) and model["route_edges"] in feed else ())
        fetches = [model[key] for key in keys]
        if train:
            fetches.insert(0, model["train_step"])
        values = sess.run(fetches, feed_dict=feed)
        stats = dict(zip(keys, values[len(values) - len(keys):]))
        if len(keys) > len(_STAT_KEYS):
            stats["route_stats"] = [stats[k] for k in _ROUTE_KEYS]
        labels, n_vertices, n_edges = batch[3], batch[4], batch[5]
    mean_label, mean_pred = _batch_means(sess, labels, stats["predictions"])
    if verbose:
        _log("train" if train else "test", epoch_i, (
            ("batch", batch_i),
            ("vertices", int(np.sum(n_vertices))), ("edges", int(np.sum(n_edges))), ("graphs", len(n_vertices)),
            ("loss", "%.4f" % stats["loss"]), ("acc", "%.4f" % stats["acc"]),
            ("label_mean", "%.4f" % mean_label),
            ("decided_yes", "%.4f" % float(np.mean(np.round(stats["predictions"])))),
        ) + _route_fields(stats.get("route_stats")))
    return (stats["loss"], stats["acc"], mean_label, mean_pred,
            stats["TP"], stats["FP"], stats["TN"], stats["FN"])


def run_batches_accumulated(sess, model, batches, batch_i, epoch_i, time_steps, verbose=True):
    """ONE optimiser step over ``batches`` (Session.train_step_accumulated): create_batch 6-tuples or DeviceBatches, each
    a micro-batch whose gradient counts with weight B_k / B.  Returns run_batch's 8-tuple for their union: loss and acc
    are the B-weighted means, TP .. FN the sums, the label / prediction means are taken over all graphs (reduced across
    ranks as run_batch's are).  With a route head: marks as in run_batch, and the line shows the route loss and edge
    accuracy of the LAST micro-batch (of this rank)."""
    from .model import DeviceBatch
    feeds, labels, n_vertices, n_edges = [], [], [], []
    for batch in batches:
        if isinstance(batch, DeviceBatch):
            batch.T = int(time_steps)
            feeds.append(batch)
            host = (batch.route_exists, batch.n_vertices, batch.n_edges)
        else:
            feeds.append(_feed_for(model, batch, time_steps))
            host = batch[3:6]
        for dest, part in zip((labels, n_vertices, n_edges), host):
            dest.append(np.asarray(part).reshape(-1))
    out = sess.train_step_accumulated(feeds)
    values = out["stats"].cpu().numpy()
    stats = {key: np.float32(values[k]) for k, key in enumerate(("loss", "acc", "TP", "FP", "TN", "FN"))}
    predictions = np.concatenate([p.cpu().numpy() for p in out["predictions"]])
    labels, n_vertices, n_edges = (np.concatenate(x) for x in (labels, n_vertices, n_edges))
    mean_label, mean_pred = _batch_means(sess, labels, predictions)
    if verbose:
        _log("train", epoch_i, (
            ("batch", batch_i), ("micro_batches", len(feeds)),
            ("vertices", int(np.sum(n_vertices))), ("edges", int(np.sum(n_edges))), ("graphs", len(n_vertices)),
            ("loss", "%.4f" % stats["loss"]), ("acc", "%.4f" % stats["acc"]),
            ("label_mean", "%.4f" % mean_label),
            ("decided_yes", "%.4f" % float(np.mean(np.round(predictions)))),
        ) + _route_fields(out["route_stats"].cpu().numpy() if "route_stats" in out else None))
    return (stats["loss"], stats["acc"], mean_label, mean_pred,
            stats["TP"], stats["FP"], stats["TN"], stats["FN"])


def summarize_epoch(epoch_i, loss, acc, sat, pred, train=False):
    """Epoch line: the means of the per-batch values ``run_batch`` returned (train.py:66-76)."""
    _log("train" if train else "test", epoch_i, (
        ("batches", len(loss)),
        ("loss", "%.4f" % float(np.mean(loss))), ("acc", "%.4f" % float(np.mean(acc))),
        ("label_mean", "%.4f" % float(np.mean(sat))), ("pred_mean", "%.4f" % float(np.mean(pred))),
    ))
