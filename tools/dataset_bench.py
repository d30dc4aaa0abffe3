"""Times GPU labelling (tspgnn.dataset) at the reference's dataset shapes: the training set (2^15 instances, n 20-40),
the test set (2^10), n = 80, and n = 200 and 256 (label_tours on the triangle kernels).  Reports the closure, search, bound and file-writing seconds separately, the certified fraction
at dev = 0.02 and the gap (cost - lb) / cost distribution; one JSON line per shape.

    python tools/dataset_bench.py [--shapes train,test,n80,n200,n256] [--restarts R] [--kicks K] [--lb-iters I] [--out DIR]
        [--exact [--max-nodes N]] [--neighbors K] [--distances euc_2D|random] [--closure host|device] [--resident]
        [--writer host|device|both] [--reader host|device|both]

Without --restarts / --kicks / --lb-iters each shape runs label_tours' defaults for its n.
--exact labels with the branch and bound (label_tours(exact=True), n <= 128) and adds the proved fraction, the nodes per
instance (p50 / p90 / max) and the seconds of that launch; bound_s is then 0.
--neighbors K runs the candidate-list descent (label_tours(neighbors=K)); the JSON line then carries "neighbors".
--distances random draws the reference's random metric instances; --closure says where their metric closure is taken
(draw_instances(closure=...)): "closure_s" is its wall seconds (for device: synchronised, transfers included) and
"draw_s" the rest of the drawing.
--resident times, per shape, the two routes to a device-resident dataset, alternated twice in one process: "host" is
draw_instances -> label_tours -> DeviceDataset(...), "generate" is DeviceDataset.generate; one JSON line per run with the
wall seconds from the seeding to the synchronised dataset ("total_s") and the stages each route can name.
--writer says who formats the .graph files, as create_dataset(writer=...): "host" is the write_graph loop, "device" the
GPU writer (graph_text.write_instances, the call create_dataset makes) and "both" alternates the two twice over the same
labelled instances; a device run adds one JSON line with its wall seconds ("total_s") and its stages (upload, the sizes
and write launches, their sum "format_s", the download, the file writes).  With --resident every generated dataset is also written twice by DeviceDataset.write_directory and
twice by to_instances() + write_graph, alternated, one JSON line each ("writer").
--reader times DeviceDataset.from_directory over directories written first by write_directory -- 2^14 files with n 20-40
and 256 files with n = 200 (--samples overrides both counts) -- and does nothing else: "host" is read_graph per file and
the host packers, "device" the GPU reader (graph_text.read_files), "both" alternates the two twice over the same
directory.  The page cache is warm for both: every file is read once, untimed, after it is written.  One JSON line per run
with the wall seconds to the synchronised dataset ("total_s") and the MB/s of text; a device run adds its stages (file
I/O, upload, the scan and parse launches with their downloads, the packing launch).
"""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tspgnn import dataset, graph_text  # noqa: E402
from tspgnn.device_dataset import DeviceDataset  # noqa: E402

SHAPES = {"train": (2 ** 15, 20, 40), "test": (2 ** 10, 20, 40), "n80": (2 ** 10, 80, 80), "n200": (2 ** 10, 200, 200),
          "n256": (2 ** 10, 256, 256)}


def _scratch_dir(a):
    out = a.out or tempfile.mkdtemp(prefix="dsbench_")
    os.makedirs(out, exist_ok=True)
    return out


def _stage_columns(stages):
    """The device writer's stages as JSON columns; its two launches are named for their kernels."""
    names = {"sizes": "sizes_kernel_s", "write": "write_kernel_s"}
    return {names.get(k, k + "_s"): round(v, 3) for k, v in stages.items()}


def write_files(a, name, samples, instances):
    """The files of one labelled shape by the writer(s) of --writer: -> seconds of the first run (the "write_s" column);
    one JSON line per device run, and per run at all with --writer both."""
    order = {"host": ["host"], "device": ["device"], "both": ["host", "device"] * 2}[a.writer]
    first = None
    for rep, writer in enumerate(order):
        out = _scratch_dir(a)
        stages = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if writer == "host":
            for i, (Ma, Mw, tour) in enumerate(instances):
                dataset.write_graph(np.triu(Ma), Mw, filepath=os.path.join(out, "%d.graph" % i), route=tour)
        else:
            graph_text.write_instances(out, instances, torch.device("cuda", torch.cuda.current_device()), times=stages)
        seconds = time.perf_counter() - t0
        first = seconds if first is None else first
        if writer == "device" or a.writer == "both":
            print(json.dumps({"shape": name, "samples": samples, "writer": writer, "rep": rep // 2,
                              "total_s": round(seconds, 3), **_stage_columns(stages)}), flush=True)
        if a.out is None:
            shutil.rmtree(out)
    return first


def write_resident(a, name, samples, ds):
    """A generated dataset to files: write_directory against to_instances() + write_graph, alternated twice."""
    for rep in range(2):
        for writer in ("to_instances+write_graph", "write_directory"):
            out = _scratch_dir(a)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if writer == "write_directory":
                report = ds.write_directory(out)
                stages = dict(_stage_columns(report["times"]), bytes=report["bytes"])
            else:
                instances = ds.to_instances()
                t1 = time.perf_counter()
                for i, (Ma, Mw, tour) in enumerate(instances):
                    dataset.write_graph(Ma, Mw, filepath=os.path.join(out, "%d.graph" % i), route=tour)
                stages = {"to_instances_s": round(t1 - t0, 3), "write_graph_s": round(time.perf_counter() - t1, 3)}
            print(json.dumps({"shape": name, "samples": samples, "writer": writer, "rep": rep,
                              "total_s": round(time.perf_counter() - t0, 3), **stages}), flush=True)
            if a.out is None:
                shutil.rmtree(out)


def resident(a, name, samples, nmin, nmax):
    """The two routes to a resident dataset of one shape, alternated twice; one JSON line per run."""
    kw = dict(restarts=a.restarts, kicks=a.kicks, lb_iters=a.lb_iters, neighbors=a.neighbors)
    r3 = lambda d: {k + "_s": round(v, 3) for k, v in d.items()}
    for rep in range(2):
        for route in ("host", "generate"):
            random.seed(1)
            np.random.seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "host":
                tc, tm = {}, {}
                graphs = dataset.draw_instances(nmin, nmax, samples=samples, distances=a.distances, closure=a.closure,
                                                timings=tc)
                t_draw = time.perf_counter() - t0 - tc.get("closure", 0.0)
                res = dataset.label_tours([(g[0], g[1]) for g in graphs], init_tours=[g[2] for g in graphs], timings=tm,
                                          exact=a.exact, max_nodes=a.max_nodes, **kw)
                t1 = time.perf_counter()
                ds = DeviceDataset([(np.triu(g[0]), g[1], r.tour) for g, r in zip(graphs, res)])
                torch.cuda.synchronize()
                stages = dict(draw=t_draw, **tc, **tm, resident=time.perf_counter() - t1)
                certified = dataset.certify(res, 0.02)["fraction"]
            else:
                ds = DeviceDataset.generate(samples, nmin, nmax, distances=a.distances, exact=a.exact,
                                            **({} if a.max_nodes is None else {"max_nodes": a.max_nodes}), **kw)
                torch.cuda.synchronize()
                stages = {k: v for k, v in ds.summary["times"].items() if k != "total"}
                certified = ds.summary["certified_fraction"]
            total = time.perf_counter() - t0
            print(json.dumps({"shape": name, "samples": samples, "n": [nmin, nmax], "resident": route, "rep": rep,
                              "distances": a.distances, **({} if a.neighbors is None else {"neighbors": a.neighbors}),
                              "total_s": round(total, 3), **r3(stages), "edges": int(ds.m.sum()),
                              "certified_0.02": round(certified, 4)}), flush=True)
            if route == "generate" and rep == 1 and not a.no_write:
                write_resident(a, name, samples, ds)
            del ds


READ_SHAPES = {"files_train": (2 ** 14, 20, 40), "files_n200": (2 ** 8, 200, 200)}


def readers(a):
    """--reader: the two readers of a .graph directory per shape of READ_SHAPES; one JSON line per run."""
    order = {"host": ["host"], "device": ["device"], "both": ["host", "device"] * 2}[a.reader]
    dev = torch.device("cuda", torch.cuda.current_device())
    warm = tempfile.mkdtemp(prefix="dsbench_warm_")   # the reader's code objects and the pinned allocator, untimed
    DeviceDataset.generate(4, 20, 20, kicks=1, lb_iters=1, restarts=1).write_directory(warm)
    for reader in order:
        DeviceDataset.from_directory(warm, device=dev, reader=reader)
    shutil.rmtree(warm)
    for name, (samples, nmin, nmax) in READ_SHAPES.items():
        samples = a.samples or samples
        random.seed(1)
        np.random.seed(1)
        out = _scratch_dir(a) if a.out is None else os.path.join(a.out, name)
        made = DeviceDataset.generate(samples, nmin, nmax, kicks=1, lb_iters=1, restarts=1)
        written = made.write_directory(out)["bytes"]
        del made
        for f in os.listdir(out):   # warm page cache for both readers
            with open(os.path.join(out, f), "rb") as fh:
                fh.read()
        for rep, reader in enumerate(order):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = DeviceDataset.from_directory(out, device=dev, reader=reader)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            stages = {}
            if reader == "device":
                stages = {k + "_s": round(v, 3) for k, v in ds.read_times.items() if k != "bytes"}
            print(json.dumps({"shape": name, "files": samples, "n": [nmin, nmax], "reader": reader, "rep": rep // 2,
                              "text_bytes": written, "total_s": round(total, 3),
                              "MB_per_s": round(written / total / 1e6, 1), **stages, "edges": int(ds.m.sum())}),
                  flush=True)
            del ds
        if a.out is None:
            shutil.rmtree(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="train,test,n80")
    ap.add_argument("--restarts", type=int, default=None)
    ap.add_argument("--kicks", type=int, default=None)
    ap.add_argument("--lb-iters", type=int, default=None)
    ap.add_argument("--exact", action="store_true", help="label with the branch and bound (n <= 128)")
    ap.add_argument("--max-nodes", type=int, default=None, help="--exact: nodes per instance")
    ap.add_argument("--neighbors", type=int, default=None, help="candidate-list descent over K nearest neighbours")
    ap.add_argument("--distances", default="euc_2D", choices=("euc_2D", "random"))
    ap.add_argument("--closure", default="host", choices=("host", "device"),
                    help="--distances random: where the metric closure is taken")
    ap.add_argument("--samples", type=int, default=0, help="override the instance count of every shape")
    ap.add_argument("--resident", action="store_true",
                    help="time the host route and DeviceDataset.generate to a device-resident dataset, alternated twice")
    ap.add_argument("--writer", default="host", choices=("host", "device", "both"),
                    help="who formats the .graph files (create_dataset's writer=); both: alternated twice")
    ap.add_argument("--reader", default=None, choices=("host", "device", "both"),
                    help="time DeviceDataset.from_directory(reader=) over written directories, and nothing else")
    ap.add_argument("--no-write", action="store_true", help="solve only (no .graph files)")
    ap.add_argument("--out", default=None, help="directory for the .graph files (default: a temporary one)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dataset_bench needs an MI355X"
    if a.reader is not None:
        return readers(a)
    # warm-up: load the code objects outside the timed runs
    for n in (20, 130):
        dataset.label_tours([(np.triu(np.ones((n, n)), 1), np.random.RandomState(0).rand(n, n))], kicks=1, lb_iters=1,
                            neighbors=a.neighbors)
    if a.closure == "device" and a.distances != "euc_2D":
        for n in (20, 40, 80, 140, 200):   # one launch per kernel instantiation
            dataset.metric_closure([np.ones((n, n))])
    if a.exact:
        dataset.label_tours([(np.triu(np.ones((20, 20)), 1), np.random.RandomState(0).rand(20, 20))], kicks=1, lb_iters=1,
                            exact=True, max_nodes=1)
    if a.resident:   # generate's kernels and the gather-free constructor path, outside the timed runs
        state = random.getstate(), np.random.get_state()
        for n in (20, 130):
            DeviceDataset.generate(2, n, n, distances=a.distances, kicks=1, lb_iters=1, neighbors=a.neighbors)
        random.setstate(state[0])
        np.random.set_state(state[1])
    for name in a.shapes.split(","):
        samples, nmin, nmax = SHAPES[name]
        samples = a.samples or samples
        if a.resident:
            resident(a, name, samples, nmin, nmax)
            continue
        random.seed(1)
        np.random.seed(1)
        t0 = time.perf_counter()
        tc = {}
        graphs = dataset.draw_instances(nmin, nmax, samples=samples, distances=a.distances, closure=a.closure, timings=tc)
        t_draw = time.perf_counter() - t0 - tc.get("closure", 0.0)
        closure = {} if "closure" not in tc else {"closure": a.closure, "closure_s": round(tc["closure"], 3)}
        tm, stats = {}, {}
        res = dataset.label_tours([(g[0], g[1]) for g in graphs], init_tours=[g[2] for g in graphs],
                                  restarts=a.restarts, kicks=a.kicks, lb_iters=a.lb_iters, timings=tm,
                                  exact=a.exact, max_nodes=a.max_nodes, stats=stats, neighbors=a.neighbors)
        large = nmax > dataset.MAX_N
        restarts = a.restarts or (dataset.DEFAULT_RESTARTS_LARGE if large else dataset.DEFAULT_RESTARTS)
        kicks = a.kicks if a.kicks is not None else (dataset.DEFAULT_KICKS_LARGE if large else dataset.DEFAULT_KICKS)
        lb_iters = a.lb_iters or (dataset.DEFAULT_LB_ITERS_LARGE if large else dataset.DEFAULT_LB_ITERS)
        t_write = None
        if not a.no_write:
            t_write = write_files(a, name, samples, [(g[0], g[1], r.tour) for g, r in zip(graphs, res)])
        c = dataset.certify(res, 0.02)
        gap = np.array([(r.cost - r.lb) / r.cost for r in res])
        exact = {}
        if a.exact:
            nd = stats["nodes"]
            exact = {"exact_s": round(tm.get("exact", 0.0), 3),
                     "max_nodes": a.max_nodes or dataset.DEFAULT_BB_NODES, "node_iters": dataset.DEFAULT_BB_ITERS,
                     "proved": round(float(np.mean(stats["status"] == "proved")), 4),
                     "nodes": {"p50": int(np.percentile(nd, 50)), "p90": int(np.percentile(nd, 90)), "max": int(nd.max())},
                     "proved_gap_max": float(gap[stats["status"] == "proved"].max(initial=0.0))}
        print(json.dumps({
            "shape": name, "samples": samples, "n": [nmin, nmax], "restarts": restarts, "kicks": kicks,
            "lb_iters": lb_iters, **({} if a.neighbors is None else {"neighbors": a.neighbors}), "distances": a.distances, "draw_s": round(t_draw, 3), **closure, "pack_s": round(tm["pack"], 3),
            "search_s": round(tm["search"], 3), "bound_s": round(tm.get("bound", 0.0), 3), **exact,
            "write_s": None if t_write is None else round(t_write, 3),
            "feasible": float(np.mean([r.feasible for r in res])),
            "certified_0.02": round(c["fraction"], 4), "label0": round(float(c["label0"].mean()), 4),
            "label1": round(float(c["label1"].mean()), 4),
            "gap": {"median": float(np.median(gap)), "p90": float(np.percentile(gap, 90)),
                    "p99": float(np.percentile(gap, 99)), "max": float(gap.max()),
                    "zero": float(np.mean(gap <= 1e-9))},
        }), flush=True)


if __name__ == "__main__":
    main()
