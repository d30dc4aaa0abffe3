"""What the route head costs at C2 (128 x n=40, d=64, T=32), captured, one process per run: milliseconds per training step
(capture_train_step) and per forward (capture_forward) of build_network(64) and of build_network(64, route_head=True) on the
same batch, the second with the marks of the instances' tours.

    python tools/route_head_bench.py [--rounds 3] [--steps 30] [--warmup 5] [--out profiles/route_head_bench.txt]

The two networks alternate as tools/ab.sh alternates two libraries -- without, with, without, with, ... -- each run a fresh
process; the spread of a column over the rounds is the margin the comparison has and is printed beside the medians.  The
head adds, per training step: one three-layer MLP forward with saved activations, a row-dot, tspgnn_edge_bce_f32, and the
backward of those (data gradient, four weight gradients); per forward: one tspgnn_mlp_head_fwd_h2 launch and the statistics.

    python tools/route_head_bench.py --child 0|1      (one run; prints one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PAIRS, D, T = 40, 64, 64, 32          # bench.py's workload c2: 128 graphs of 40 vertices, every instance twice


def child(head, steps, warmup):
    sys.path.insert(0, os.path.join(HERE, "tsp-gnn_amd"))
    import numpy as np
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

    rng = np.random.RandomState(1234)
    instances = [inst for inst in (tspgnn.random_instance(N, rng) for _ in range(PAIRS)) for _ in (0, 1)]
    model = tspgnn.build_network(D, route_head=head)
    sess = tspgnn.Session(model)
    sess.run(tspgnn.global_variables_initializer(seed=0))
    EV, W, C, route_exists, n_vertices, n_edges = tspgnn.InstanceLoader.create_batch(instances)
    feed = {model["EV"]: EV, model["W"]: W, model["C"]: C, model["time_steps"]: T, model["route_exists"]: route_exists,
            model["n_vertices"]: n_vertices, model["n_edges"]: n_edges}
    if head:
        feed[model["route_edges"]] = tspgnn.route_edge_marks_host(instances)[0]
    b = sess.prepare(feed)
    res = {"head": int(head), "forward_ms": round(timed(sess.capture_forward(b), steps), 4)}
    res["train_ms"] = round(timed(sess.capture_train_step(b), steps), 4)
    res["steps_applied"] = int(sess._adam["t"].item())
    print(json.dumps(res), flush=True)


def run(head, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(head), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.timeout).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def column(name, values):
    values = sorted(values)
    med = values[len(values) // 2]
    return "%-34s median %8.3f ms   min %8.3f   max %8.3f   spread %.3f ms (%.1f %%)" % (
        name, med, values[0], values[-1], values[-1] - values[0], 100.0 * (values[-1] - values[0]) / med), med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "route_head_bench.txt"))
    ap.add_argument("--child", default=None, type=int, metavar="HEAD")
    a = ap.parse_args()
    if a.child is not None:
        return child(bool(a.child), a.steps, a.warmup)
    runs = {0: [], 1: []}
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for r in range(a.rounds):
        for head in (0, 1):
            runs[head].append(run(head, a))
            say("round %d  route_head=%d  %s" % (r, head, json.dumps(runs[head][-1])))
    say("\nC2 (128 x n=40, d=64, T=32), captured, one GPU, %d rounds of %d timed steps, the two networks alternating"
        % (a.rounds, a.steps))
    for key, what in (("train_ms", "training step"), ("forward_ms", "forward")):
        line, off = column("%s, without the head" % what, [m[key] for m in runs[0]])
        say(line)
        line, on = column("%s, route_head=True" % what, [m[key] for m in runs[1]])
        say(line)
        say("%-34s %+.3f ms (%+.1f %%)" % ("    the head adds", on - off, 100.0 * (on - off) / off))
    say("\nnot measured: other shapes than C2, bf16 storage, and any multi-GPU run")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
