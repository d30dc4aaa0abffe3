#!/usr/bin/env python
"""End-to-end forward-only serving rate at C2 (host instances -> packed batch -> upload -> forward), i.e. the
PCIe- and packer-inclusive number next to bench.py's resident-batch headline.  Fresh instances every batch:
BatchPrefetcher packs and uploads batch i+1 on a worker thread / side stream while the GPU runs batch i."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
import tspgnn  # noqa: E402


def device_dataset_bench():
    """--device-dataset: the serving rate at C2 (128 x n = 40, T = 32) with batches assembled on the GPU from instance ids
    (DeviceDataset.batch(out=...) + replay), next to the BatchStager rate and the resident replay of the same process, the
    three legs alternated ROUNDS times; then a ragged leg (n 20-40, eager launches) against BatchPrefetcher.  Prints a
    text report (kept as profiles/device_dataset_bench.txt)."""
    B, n, T = 128, 40, 32
    nb, rounds = int(os.environ.get("BATCHES", 200)), int(os.environ.get("ROUNDS", 5))
    rng = np.random.RandomState(0)
    pool = [tspgnn.random_instance(n, rng) for _ in range(3 * B)]
    lists = [[(i * 37 + j) % len(pool) for j in range(B)] for i in range(nb)]
    model = tspgnn.build_network(64)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer(seed=0))
    t0 = time.perf_counter()
    ds = tspgnn.DeviceDataset(pool)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    stager = tspgnn.BatchStager(sess, [pool[k] for k in lists[0]], T)
    replay_s = sess.capture_forward(stager.batch)
    bound = ds.batch(lists[0], time_steps=T)
    replay_d = sess.capture_forward(bound)
    # same bytes in, same graph: the two paths must agree before their times mean anything
    same = True
    for k, _ in enumerate(stager.feed([pool[j] for j in idx] for idx in lists[:3])):
        want = replay_s()["predictions"].clone()
        ds.batch(lists[k], time_steps=T, out=bound)
        same = same and torch.equal(replay_d()["predictions"], want)

    def timed(run):
        torch.cuda.synchronize()
        t = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / nb

    def leg_resident():
        for _ in range(nb):
            replay_d()

    def leg_stager():
        for _ in stager.feed([pool[k] for k in idx] for idx in lists):
            replay_s()

    def leg_device():
        for idx in lists:
            ds.batch(idx, time_steps=T, out=bound)
            replay_d()

    def leg_gather_only():
        for idx in lists:
            ds.batch(idx, time_steps=T, out=bound)

    legs = (("resident replay", leg_resident), ("BatchStager + replay", leg_stager),
            ("DeviceDataset.batch(out=) + replay", leg_device), ("DeviceDataset.batch(out=) alone", leg_gather_only))
    for _, run in legs:     # warm-up of every leg
        run()
    times = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, run in legs:
            times[name].append(timed(run))
    print("device-resident dataset at C2: %d x n = %d, T = %d, d = 64; %d batches per leg, %d alternated rounds; dataset of "
          "%d instances built in %.1f ms; predictions equal to the stager path's: %s"
          % (B, n, T, nb, rounds, len(pool), 1e3 * build_s, same))
    base = float(np.median(times["resident replay"]))
    for name, _ in legs:
        v = times[name]
        print("  %-36s ms/batch median %.4f  min %.4f  max %.4f   x%.3f of resident   mp-steps/s %.0f"
              % (name, np.median(v), min(v), max(v), np.median(v) / base, T / (1e-3 * np.median(v))))
    # ---- ragged: every batch another shape, eager launches; the prefetcher packs and uploads on its worker thread
    nbr = int(os.environ.get("RAGGED_BATCHES", 40))
    sizes = rng.randint(20, 41, size=256)
    rpool = [tspgnn.random_instance(int(k), rng) for k in sizes]
    rds = tspgnn.DeviceDataset(rpool)
    rlists = [list(rng.randint(0, len(rpool), size=B)) for _ in range(nbr)]
    pack = lambda inst: tspgnn.InstanceLoader.create_batch(inst, dev=0.02)

    def ragged_prefetcher():
        for b in tspgnn.BatchPrefetcher(sess, ([rpool[k] for k in idx] for idx in rlists), T, pack=pack):
            sess.forward_device(b)

    def ragged_device():
        for idx in rlists:
            sess.forward_device(rds.batch(idx, time_steps=T))

    rlegs = (("BatchPrefetcher + forward", ragged_prefetcher), ("DeviceDataset.batch + forward", ragged_device))
    rtimes = {name: [] for name, _ in rlegs}
    for _ in range(rounds + 1):     # first pass: the work plans of the block structures are built (both paths cache them)
        for name, run in rlegs:
            rtimes[name].append(timed(run) * nb / nbr)
    print("ragged: %d graphs per batch, n uniform in 20..40, %d batches of different shapes, eager launches" % (B, nbr))
    for name, _ in rlegs:
        v = rtimes[name]
        print("  %-36s ms/batch first pass %.4f | later passes median %.4f  min %.4f  max %.4f"
              % (name, v[0], np.median(v[1:]), min(v[1:]), max(v[1:])))
    print("  range guard bits: %d" % (sess.last_range_bits if sess.range_exceeded() else 0))


if "--device-dataset" in sys.argv[1:]:
    device_dataset_bench()
    sys.exit(0)

B, n, T, nb =128, 40, 32, int(os.environ.get("BATCHES", 60))
rng = np.random.RandomState(0)
pool = [tspgnn.random_instance(n, rng) for _ in range(4 * B)]


def batches():
    for i in range(nb):
        k = (i * 37) % (3 * B)
        yield tspgnn.InstanceLoader.create_batch(pool[k:k + B], dev=0.02)


pool_batch = tspgnn.InstanceLoader.create_batch(pool[:B], dev=0.02)
model = tspgnn.build_network(64)
sess = tspgnn.Session(model)
sess.run(tspgnn.global_variables_initializer(seed=0))
out = None
for b in tspgnn.BatchPrefetcher(sess, batches(), T):      # warm-up pass (allocator, weight packs)
    out = sess.forward_device(b)
torch.cuda.synchronize()
t0 = time.perf_counter()
preds = []
for b in tspgnn.BatchPrefetcher(sess, batches(), T):
    preds.append(sess.forward_device(b)["predictions"])
torch.cuda.synchronize()
dt = time.perf_counter() - t0
t1 = time.perf_counter()
for _ in batches():
    pass
pack = (time.perf_counter() - t1) / nb
# same-shaped batches through ONE captured graph: each prefetched batch is copied into the graph's resident buffers
static = sess.prepare({model["EV"]: pool_batch[0], model["W"]: pool_batch[1], model["C"]: pool_batch[2],
                       model["time_steps"]: T, model["route_exists"]: pool_batch[3], model["n_vertices"]: pool_batch[4],
                       model["n_edges"]: pool_batch[5]})
replay = sess.capture_forward(static)
torch.cuda.synchronize()
t3 = time.perf_counter()
for b in tspgnn.BatchPrefetcher(sess, batches(), T):
    static.copy_from(b)
    preds.append(replay()["predictions"].clone())
torch.cuda.synchronize()
graphed = (time.perf_counter() - t3) / nb
# the same without the worker thread: pack, upload and launch from one thread
m = model
torch.cuda.synchronize()
t2 = time.perf_counter()
for t in batches():
    EV, W, C, r, nv, ne = t
    b = sess.prepare({m["EV"]: EV, m["W"]: W, m["C"]: C, m["time_steps"]: T, m["route_exists"]: r, m["n_vertices"]: nv,
                      m["n_edges"]: ne})
    preds.append(sess.forward_device(b)["predictions"])
torch.cuda.synchronize()
inline = (time.perf_counter() - t2) / nb
print(json.dumps({"workload": "c2 serving: fresh instances every batch, pack + upload + forward (eager launches)",
                  "batches": nb, "ms_per_batch_end_to_end": round(1e3 * dt / nb, 3),
                  "mp_steps_per_s_end_to_end": round(nb * T / dt, 1), "host_pack_ms_per_batch": round(1e3 * pack, 3),
                  "ms_per_batch_single_thread": round(1e3 * inline, 3),
                  "ms_per_batch_graph_replay": round(1e3 * graphed, 3),
                  "mp_steps_per_s_graph_replay": round(T / graphed, 1)}))
