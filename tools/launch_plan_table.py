#!/usr/bin/env python3
"""The table of launch plans, tests/golden/launch_plans.json: every planner of csrc/launch_plan.h asked through
tests/plan_replay.py (the tspgnn_plan_* queries) over a grid that crosses its thresholds -- CU counts 1, 104 and 256, row counts at,
one below and one above the boundaries derived from the CU count, the LDS modes of the forward cell launchers, K resident
and chunked in the cell backward and bf16 forward launchers.  No device
is needed.

    python tools/launch_plan_table.py            compare the library with the committed table (exit status 1: it moved)
    python tools/launch_plan_table.py --write    rewrite the table: how a deliberate launcher change records itself

tests/test_launch_plan_table.py holds the library to the committed table."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "launch_plans.json")

CUS = (1, 104, 256)      # (the first recording crossed 1, 8, 64, 104, 256 and 304 with more row counts: the table is its thinning)


def around(*bounds):
    """Each boundary, one below and one above (positive values, ascending, once each)."""
    return sorted({v for b in bounds for v in (b - 1, b, b + 1) if v > 0})


def linear_cases():
    for kin, n1, n2, per_cu in ((128, 64, 64, 2), (256, 64, 64, 1), (512, 128, 128, 1)):
        for cus in CUS:
            full = cus * per_cu
            for r in around(16 * 4 * cus, 16 * 4 * full) + [16 * 4 * full - 15, 16 * 8 * (2 * full) + 17, 16 * (2 * full * 8) + 1]:
                yield (kin, n1, n2, r, cus)


def mlp_bwd_cases():
    for d, per_cu in ((64, 2), (128, 1)):
        for cus in CUS:
            full = cus * per_cu
            deep = 16 * (2 * full * 8) + 1
            for r in around(16 * 4 * full) + [17, deep]:
                yield ([(r, 2)], d, cus)
            yield ([(333, 2), (deep, 2)], d, cus)
            yield ([(5000, 2), (5000, 1), (100, 2), (16 * 8 * cus + 1, 1)], d, cus)


def wgrad_cases():
    for cus in CUS:
        for kin in (16, 32, 64):
            for nout in (16, 32, 64):
                for r in ((255, 4095, 4096, 70001) if kin == nout else (257, 70001)):
                    yield (r, kin, nout, cus)
        for kin, nout in ((32, 128), (512, 512), (48, 96)):
            for r in (1, 99840, 256 * cus * 8 + 1):
                yield (r, kin, nout, cus)


def colsum_cases():
    for cus in CUS:
        for r in around(1024, 1024 * 4 * cus) + [1, 64 * 1024 + 1, 5094400]:
            yield (r, cus)


def einit_bwd_cases():
    for d, per_cu in ((64, 2), (128, 1)):
        for cus in CUS:
            full = cus * per_cu
            for M in around(64 * full) + [1, 333, 64 * 2 * full + 1]:
                yield (M, d, cus)


def mlp_fwd_cases():
    for cus in CUS:
        for tiles in around(4 * cus, 16 * cus):
            yield ([(16 * tiles, 3, False)], cus)
        yield ([(9000, 3, False), (700, 4, True)], cus)
        yield ([(5000, 2, False), (5000, 1, True), (100, 4, True), (16 * 16 * cus + 1, 3, False)], cus)


def cell_fwd_cases(task):
    """task: plan_replay.cell_task."""
    for arith in ("h2", "x3"):
        for d in (32, 64):
            # the LDS modes: one task, among the shapes the entries accept (a projection needs an MLP layer)
            for dx in (0, 64, 96, 192, 320, 512):
                for L, proj in ((0, False), (1, True), (3, False), (4, False), (4, True)):
                    yield ([task(333, dx, L, proj, proj, bool(L))], d, 256, arith)
            for cus in CUS if d == 64 else ():       # (the split does not look at d)
                edge = lambda rows: task(rows, 0, 3, False, True, True)
                vert = lambda rows, zc=False: task(rows, d, 4, True, True, True, zc)
                # the wavefront thresholds of a resident and of a lock-step task, and the vertex task's deep count
                for tiles in around(4 * cus, 8 * cus):
                    yield ([edge(16 * tiles)], d, cus, arith)
                yield ([vert(16 * 4 * cus + 1)], d, cus, arith)
                yield ([vert(16 * (12 * 2 * cus) + 1)], d, cus, arith)
                # a step's launch: edge gather cell + 3 layers, vertex cell + 4 layers + projection
                for M, N in ((7001, 333), (99840, 5120), (695849, 25362), (100, 5000)):
                    yield ([edge(M), vert(N)], d, cus, arith)
                yield ([vert(5120, True), task(99840, 0, 0, z_centered=True)], d, cus, arith)
                yield ([task(2000, 64), edge(99840), vert(5120)], d, cus, arith)
                yield ([task(2000, 64, 2), edge(40000), vert(5120), task(300, 192, 1, True)], d, cus, arith)


STEPS = ((12801, 70001), (333, 7001))     # (vertex rows, edge rows) of a training step's cell launch


def cell_bwd_cases():
    """(tasks, d, cus, arith); tasks: plan_replay.cell_bwd_plan's (rows, dx, with_KT, with_KTg[, gather])."""
    plain = lambda rows, dx: (rows, dx, False, False)
    kt = lambda rows, dx=0, gather=True: (rows, dx, True, False, gather)
    # fp32 residency either side of the boundary (d = 128 streams K even at dx = 0, four 16-row blocks at a time), K^T beside
    # K only at d = 64 and dx = 0, and a gather-init task at d = 128, which the entry's validation turns away first
    for d, dx in ((32, 256), (32, 272), (64, 64), (64, 80), (128, 0)):
        yield ([plain(333, dx)], d, 256, "f32")
    for d, dx, gather in ((64, 0, True), (64, 64, False), (32, 0, True)):
        yield ([kt(333, dx, gather)], d, 256, "f32")
    yield ([(333, 0, False, False, True)], 128, 256, "f32")
    # f16x2: every K it offers, the fused data gradients, and at d = 64 the last dx that fits LDS and the first that does not
    # (in steps of 32; with K^T the entry wants dx = 0, so no dx beyond it reaches the planner)
    for d in (32, 64):
        for dx in (0, d, 4 * d):
            yield ([plain(333, dx)], d, 256, "h2")
        yield ([kt(333)], d, 256, "h2")
    yield ([(333, 64, False, True)], 64, 256, "h2")
    for task in (plain(333, 96), kt(333, 32, False)):           # (dx = 64 above is the last that fits)
        yield ([task], 64, 256, "h2")
    # bf16: resident and chunked K at each d (a chunked task's tiles cost twice: blk_end beside a resident task of equal rows)
    for d, dx in ((128, 0), (128, 32), (64, 192), (64, 224), (32, 544), (32, 576)):
        yield ([plain(333, dx)], d, 256, "bf16")
    for cus in CUS:
        # four wavefronts up to 4 tiles per CU: f16x2 and a resident fp32 K; never beside a chunked fp32 task
        for tiles in around(4 * cus):
            yield ([plain(16 * tiles, 64)], 64, cus, "h2")
            yield ([plain(16 * tiles, 64)], 64, cus, "f32")
            yield ([plain(16 * tiles - 16, 64), plain(16, 128)], 64, cus, "f32")
        yield ([plain(5000, 0), plain(5000, 32)], 128, cus, "bf16")
        for N, M in STEPS:
            yield ([(N, 64, False, True), kt(M)], 64, cus, "h2")
            yield ([plain(N, 64), kt(M)], 64, cus, "f32")
            yield ([plain(N, 128), plain(M, 0)], 128, cus, "f32")
            for d in (64, 128):
                yield ([plain(N, d), (M, 0, False, False, True)], d, cus, "bf16")
        for arith in ("h2", "f32", "bf16"):
            yield ([plain(2000, 64), plain(40000, 0), plain(5120, 64), plain(300, 32)], 64, cus, arith)
            yield ([plain(5120, 64), plain(0, 64), plain(40000, 0)], 64, cus, arith)


def lstm_fwd_bf16_cases(nws):
    """(tasks, d, cus, nw); nws: plan_replay.LSTM_FWD_BF16_NW, every NW the entry dispatches at a d."""
    for d, fits, chunked in ((32, 576, 608), (64, 224, 256), (128, 0, 32)):       # under the forward's own 156 KB budget
        for nw in nws[d]:
            for dx in (fits, chunked):
                yield ([(333, dx)], d, 256, nw)
            for cus in CUS:
                for N, M in STEPS:
                    yield ([(M, 0), (N, d)], d, cus, nw)
                yield ([(5000, fits), (5000, chunked)], d, cus, nw)
                yield ([(2000, 64), (40000, 0), (5120, d), (300, 32)], d, cus, nw)
                yield ([(5120, d), (0, 32), (40000, 0)], d, cus, nw)


def mlp_fwd_bf16_cases():
    for d in (32, 64, 128):
        for L in (1, 2, 3, 4):
            for proj in (False, True):
                yield ([(333, L, proj)], d, 256)
        for cus in CUS:
            for N, M in STEPS:
                yield ([(M, 3, False), (N, 4, True)], d, cus)
                yield ([(M, 3, False), (N, 4, False)], d, cus)
            yield ([(5000, 2, False), (5000, 1, True), (100, 4, True), (16 * 16 * cus + 1, 3, False)], d, cus)


def mlp_fwd_f32_cases():
    """(tasks, d, cus); tasks: plan_replay.mlp_fwd_f32_plan's (rows, n_layers, has_proj).  Two workgroups per CU at d = 32 and
    64 (4, 8, then ONE of 16 wavefronts), one at d = 128 (4, 8); the shapes the entry's validation turns away come last."""
    for d, per_cu, L in ((32, 2, 4), (64, 2, 3), (128, 1, 2)):
        for cus in CUS:
            full = cus * per_cu
            for tiles in around(4 * full, 16 * full):
                yield ([(16 * tiles - 15, L, False)], d, cus)
            proj = d != 128
            yield ([(1, 1, False), (40000, L, False)], d, cus)
            yield ([(9000, L, False), (700, 2, proj)], d, cus)
            yield ([(40000, 2, False), (17, L, proj), (333, 1, False)], d, cus)
            yield ([(5000, 2, False), (5000, 1, proj), (100, L, proj), (16 * 16 * full + 1, 2, False)], d, cus)
    yield ([(333, 3, False)], 128, 256)
    yield ([(333, 2, True)], 128, 256)


def lstm_fwd_f32_cases():
    """(tasks, d, cus); tasks: plan_replay.lstm_fwd_f32_plan's (rows, dx, mode)."""
    # the last resident and the first chunked input width at each d (d = 128 streams K even at dx = 0), a chunk shorter than
    # qc, gather-init and bias-init where they fit
    for d, dx in ((32, 0), (32, 272), (32, 288), (64, 0), (64, 80), (64, 96), (64, 192), (128, 0), (128, 32), (128, 128)):
        yield ([(333, dx, "plain")], d, 256)
    for d in (32, 64):
        yield ([(333, 0, "gather")], d, 256)
        yield ([(333, d, "bias")], d, 256)
    for cus in CUS:
        # four wavefronts up to 4 tiles per CU of the resident launch; a chunked task's rounds at, below and above the CUs
        for tiles in around(4 * cus):
            yield ([(16 * tiles - 15, 64, "plain")], 64, cus)
            yield ([(16 * tiles - 31, 0, "gather"), (16, 64, "bias")], 64, cus)
        for rounds in around(cus):
            yield ([(16 * 8 * rounds - 15, 128, "plain")], 128, cus)
        for N, M in STEPS:
            yield ([(M, 0, "gather"), (N, 64, "bias")], 64, cus)
            yield ([(M, 0, "plain"), (N, 128, "plain")], 128, cus)
        # mixed launches: the resident tasks together, the chunked ones on their own
        yield ([(7001, 0, "gather"), (333, 192, "plain")], 64, cus)
        yield ([(333, 96, "plain"), (7001, 64, "bias")], 64, cus)
        yield ([(5120, 64, "plain"), (0, 64, "plain"), (40000, 0, "gather")], 64, cus)
        yield ([(2000, 64, "bias"), (300, 192, "plain"), (40000, 0, "gather")], 64, cus)
        yield ([(2000, 64, "plain"), (40000, 0, "gather"), (5120, 96, "plain"), (300, 32, "bias")], 64, cus)
    # refused: a bias-init task whose K does not fit (alone, and behind a task that could run), gather-init at d = 128
    yield ([(333, 192, "bias")], 64, 256)
    yield ([(333, 192, "plain"), (333, 96, "bias")], 64, 256)
    yield ([(333, 128, "bias")], 128, 256)
    yield ([(333, 0, "gather")], 128, 256)


def answer(plan, *args):
    """A plan as a list, or how the query declined: "unsupported" (the launch is refused) or "invalid" (the entry's
    validation)."""
    try:
        return list(plan(*args))
    except ValueError:
        return "unsupported"
    except RuntimeError as e:
        if getattr(e, "status", None) != -1:
            raise
        return "invalid"


def mlp_fwd_f32_record(PR, *a):
    p = PR.mlp_fwd_f32_plan(*a)
    return [p.nw, p.grid, p.blocks]


def lstm_fwd_f32_record(PR, *a):
    p = PR.lstm_fwd_f32_plan(*a)
    return [p.nw, p.grid, p.blocks, p.qc, p.chunked, p.lds_bytes, p.chunks, p.chunk_grid, p.rounds_per_wg]


def table(PR):
    """{planner: [[arguments, answer]]} from a module with tests/plan_replay.py's functions."""
    cell = []
    for tasks, d, cus, arith in cell_fwd_cases(PR.cell_task):
        try:
            p = PR.cell_fwd_plan(tasks, d, cus, arith)
            got = [p.nw, p.grid, p.blk_end, p.split, p.centered, p.wt, p.lds_bytes,
                   [[t.mode, t.kbc, t.chunks, t.preload, t.together, t.lock_tiles, t.n_rounds, t.blocks, t.rounds,
                     t.rounds_per_wg] for t in p.tasks]]
        except ValueError:
            got = "unsupported"
        cell.append([[tasks, d, cus, arith], got])
    mlp_fwd = []
    for tasks, cus in mlp_fwd_cases():
        p = PR.mlp_fwd_plan(tasks, cus)
        mlp_fwd.append([[tasks, cus], [p.nw, p.grid, p.blocks]])
    return {
        "linear": [[list(a), list(PR.linear_plan(*a))] for a in linear_cases()],
        "mlp_bwd": [[list(a), list(PR.mlp_bwd_plan(*a))] for a in mlp_bwd_cases()],
        "wgrad": [[list(a), list(PR.wgrad_plan(*a))] for a in wgrad_cases()],
        "wcolsum": [[list(a), list(PR.colsum_plan(*a))] for a in colsum_cases()],
        "einit_bwd": [[list(a), list(PR.einit_bwd_plan(*a)) + [PR.einit_bwd_full_grid(a[1], a[2])]] for a in einit_bwd_cases()],
        "mlp_fwd": mlp_fwd,
        "cell_fwd": cell,
        "cell_bwd": [[list(a), answer(PR.cell_bwd_plan, *a)] for a in cell_bwd_cases()],
        "lstm_fwd_bf16": [[list(a), answer(PR.lstm_fwd_bf16_plan, *a)] for a in lstm_fwd_bf16_cases(PR.LSTM_FWD_BF16_NW)],
        "mlp_fwd_bf16": [[list(a), answer(PR.mlp_fwd_bf16_plan, *a)] for a in mlp_fwd_bf16_cases()],
        "reduce_slices": [[n, PR.reduce_slices(n)] for n in (1, 7, 8, 63, 64, 2048)],
        "strided_blocks": [[[t, cap], list(PR.strided_blocks(t, cap))] for cap in (1024, 4096) for t in around(256 * cap) + [1]],
        "mlp_fwd_f32": [[list(a), answer(mlp_fwd_f32_record, PR, *a)] for a in mlp_fwd_f32_cases()],
        "lstm_fwd_f32": [[list(a), answer(lstm_fwd_f32_record, PR, *a)] for a in lstm_fwd_f32_cases()],
    }


def dumps(tab):
    """One record per line, no spaces: the committed form."""
    out = ["{"]
    for i, (name, recs) in enumerate(tab.items()):
        out.append('"%s":[' % name)
        out += [json.dumps(json.loads(json.dumps(r)), separators=(",", ":")) + ("," if j + 1 < len(recs) else "")
                for j, r in enumerate(recs)]
        out.append("]" + ("," if i + 1 < len(tab) else ""))
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tsp-gnn_amd")]
    import plan_replay
    text = dumps(table(plan_replay))
    if "--write" in sys.argv[1:]:
        with open(TABLE, "w") as f:
            f.write(text)
        print("wrote %s: %d bytes" % (TABLE, len(text)))
        return 0
    same = os.path.exists(TABLE) and open(TABLE).read() == text
    print("the library %s %s" % ("answers" if same else "does NOT answer", TABLE))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
