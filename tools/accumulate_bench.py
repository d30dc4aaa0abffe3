"""Times gradient accumulation at C2 (128 x n=40, d=64, T=32), captured, one process per run: milliseconds per optimiser step
and per micro-batch of capture_train_step(batch, micro_batches=K) for K in {1, 2, 4, 8}, beside the PLAIN captured training
step of this tree and of another checkout of the project (the parent commit, built in its own directory).

    python tools/accumulate_bench.py --parent PATH [--rounds 3] [--steps 30] [--warmup 5]

The two trees alternate as tools/ab.sh alternates two libraries -- parent, this tree, parent, this tree, ... -- each run a
fresh process that imports its own tree's package and library.  The spread of a column over the rounds is the margin the
comparison has; it is printed beside the medians.  What is expected: an accumulated step of K micro-batches costs no more
than K plain steps of the parent (it takes K - 1 fewer optimiser launches; the captured graph A still re-packs the weights
with every micro-batch -- the eager path packs once per step -- and each micro-batch adds one accumulate launch and the
step one bucket copy and one unpack).  Without a refill the resident batch is taken K times: timing only.

    python tools/accumulate_bench.py --child ROOT [--plain-only]      (one run; prints one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 4, 8)
SIZES, D, T = [40] * 128, 64, 32          # bench.py's workload c2


def child(root, plain_only, steps, warmup):
    sys.path.insert(0, os.path.join(root, "tsp-gnn_amd"))
    import torch
    import tspgnn

    def timed(step, count):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count

    model = tspgnn.build_network(D)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer(seed=0))
    EV, W, C, route_exists, n_vertices, n_edges = tspgnn.synthetic_batch(SIZES, seed=1234)
    b = sess.prepare({model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T,
                      model["route_exists"]: route_exists, model["n_vertices"]: n_vertices, model["n_edges"]: n_edges})
    res = {"plain_ms": round(timed(sess.capture_train_step(b), steps), 4)}
    if not plain_only:
        for K in KS:
            res["k%d_ms" % K] = round(timed(sess.capture_train_step(b, micro_batches=K), max(steps // K, 5)), 4)
    res["steps_applied"] = int(sess._adam["t"].item())
    print(json.dumps(res), flush=True)


def run(root, plain_only, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    out = subprocess.run(cmd + (["--plain-only"] if plain_only else []), check=True, stdout=subprocess.PIPE,
                         timeout=a.timeout).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def column(name, values):
    values = sorted(values)
    med = values[len(values) // 2]
    return "%-28s median %8.3f ms   min %8.3f   max %8.3f   spread %.3f ms (%.1f %%)" % (
        name, med, values[0], values[-1], values[-1] - values[0], 100.0 * (values[-1] - values[0]) / med), med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its plain captured step)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    ap.add_argument("--child", default=None, metavar="ROOT")
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.plain_only, a.steps, a.warmup)
    parent, mine = [], []
    for r in range(a.rounds):
        if a.parent is not None:
            parent.append(run(os.path.abspath(a.parent), True, a))
            print("round %d  parent     %s" % (r, json.dumps(parent[-1])), flush=True)
        mine.append(run(HERE, False, a))
        print("round %d  this tree  %s" % (r, json.dumps(mine[-1])), flush=True)
    print("\nC2 (128 x n=40, d=64, T=32), captured training step, one GPU, %d rounds of %d timed steps, trees alternating"
          % (a.rounds, a.steps))
    ref = None
    if parent:
        line, ref = column("parent: plain step", [p["plain_ms"] for p in parent])
        print(line)
    line, plain = column("this tree: plain step", [m["plain_ms"] for m in mine])
    print(line)
    ref = plain if ref is None else ref
    for K in KS:
        line, med = column("this tree: K=%d, per step" % K, [m["k%d_ms" % K] for m in mine])
        print(line)
        print("%-28s median %8.3f ms   K plain steps of the %s: %8.3f ms   difference %+.3f ms (%+.1f %%)" % (
            "           per micro-batch", med / K, "parent" if parent else "same tree", K * ref, med - K * ref,
            100.0 * (med - K * ref) / (K * ref)))
    print("\nnot measured: C5's global batch (n=200, B=256, d=128, T=64, bf16 storage) on one GPU, and any multi-GPU run")


if __name__ == "__main__":
    main()
