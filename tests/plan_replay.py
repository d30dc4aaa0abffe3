"""Replay of the host-side launch plans of the fp32 backward kernels (csrc/dense_bwd.hip) and the training-tail kernels
(csrc/train.hip): plain functions of (shape, cus) that follow the C++ line by line and answer the branch taken and its
grid.  The GPU tests that claim a branch (tests/test_gpu_fp32_backward_plans.py, tests/test_gpu_batch_kernels.py) derive
their row counts from the device's CU count and assert the branch and its depth through these functions BEFORE they
launch; tests/test_plan_replay_host.py pins the functions against the library wherever the library exposes a plan (the
workspace-size queries).  A launcher that changes must be changed here too -- the host test, or a "deep" test's own
assertion, then fails instead of the test going shallow without notice.

Nothing here touches a device."""
from collections import namedtuple


def ceil_div(a, b):
    return (a + b - 1) // b


def tiles16(rows):
    """tiles16 (csrc/launch_plan.h)."""
    return (rows + 15) // 16


def clamp_grid(grid, tiles_all, nw):
    """clamp_grid (csrc/launch_plan.h): min(grid, ceil(tiles_all / nw))."""
    return min(grid, ceil_div(tiles_all, nw))


def split_blocks(cost, grid):
    """split_blocks (csrc/launch_plan.h): workgroups per task, proportional to cost, at least one each."""
    cost = [c if c > 0 else 1 for c in cost]
    total = sum(cost)
    grid = max(grid, len(cost))
    return [max(1, (c * grid + total // 2) // total) for c in cost]


# ---------------------------------------------------------------------------------------------- tspgnn_linear_f32
LinearPlan = namedtuple("LinearPlan", "path nw grid qc per_cu tiles rounds lo hi dead")
"""path: "split" (linear_split_kernel: W resident, the columns of a tile over four wavefronts, two tiles per workgroup),
"ticket" (linear_kernel, W resident, tiles pulled through a ticket inside the workgroup's [t_beg, t_end)) or "streamed"
(linear_kernel, W through LDS qc 16-row blocks at a time, rounds of nw tiles, round r to workgroup r mod grid).
rounds: streamed only, all rounds of the launch.  lo / hi: the fewest / most tiles a workgroup hands to one wavefront SLOT
(ticket: its share of tiles over nw, rounded down / up; streamed: its rounds; split: 1).  dead: streamed only, the tiles of
the last round that do not exist."""


def linear_plan(kin, n1, n2, rows, cus):
    """launch_linear<NT> (csrc/dense_bwd.hip)."""
    nt = (n1 + n2) // 16
    tiles = tiles16(rows)
    qt = kin // 16
    per_q = 16 * nt * 16 * 4
    qc = qt
    if qt * per_q + 16 > 150 * 1024:
        qc = (128 * 1024) // per_q
    lds_bytes = qc * per_q + 16
    per_cu = 1 if lds_bytes > 80 * 1024 else 2
    grid = cus * per_cu
    if nt % 4 == 0 and qc >= qt and tiles <= cus * 4:
        return LinearPlan("split", 8, (tiles + 1) // 2, qc, per_cu, tiles, None, 1, 1, None)
    nw = 4 if (qc >= qt and tiles <= grid * 4) else 8
    grid = clamp_grid(grid, tiles, nw)
    if qc >= qt:
        share = [tiles * (b + 1) // grid - tiles * b // grid for b in range(grid)]
        return LinearPlan("ticket", nw, grid, qc, per_cu, tiles, None, min(share) // nw, ceil_div(max(share), nw), None)
    rounds = ceil_div(tiles, nw)
    per_wg = [len(range(b, rounds, grid)) for b in range(grid)]
    return LinearPlan("streamed", nw, grid, qc, per_cu, tiles, rounds, min(per_wg), max(per_wg), rounds * nw - tiles)


# ---------------------------------------------------------------------------------------- tspgnn_mlp_bwd_multi_f32
MlpBwdPlan = namedtuple("MlpBwdPlan", "nw grid blocks lo hi")
"""blocks: workgroups per task; lo / hi: per task, the fewest / most tiles of a workgroup per wavefront slot (share over
nw, rounded down / up)."""


def mlp_bwd_plan(tasks, d, cus):
    """launch_mlp_bwd<D, MAXL> (csrc/dense_bwd.hip).  tasks: [(rows, n_layers)] of the live tasks (rows > 0)."""
    maxl = 2 if d >= 128 else 4
    tiles = [tiles16(rows) for rows, _ in tasks]
    cost = [t * n_layers for t, (_, n_layers) in zip(tiles, tasks)]
    tiles_all = sum(tiles)
    lds_bytes = maxl * d * d * 4 + 16
    per_cu = 1 if lds_bytes > 80 * 1024 else 2
    grid = cus * per_cu
    nw = 4 if tiles_all <= grid * 4 else 8
    blocks = split_blocks(cost, clamp_grid(grid, tiles_all, nw))
    lo, hi = [], []
    for n, nb in zip(tiles, blocks):
        share = [n * (b + 1) // nb - n * b // nb for b in range(nb)]
        lo.append(min(share) // nw)
        hi.append(ceil_div(max(share), nw))
    return MlpBwdPlan(nw, sum(blocks), blocks, lo, hi)


# ------------------------------------------------------------------------------------------------ tspgnn_wgrad_f32
WgradPlan = namedtuple("WgradPlan", "kernel av bv nob n_chunks chunk_rows last_rows")
"""kernel: "x3" (wgrad_x3_kernel) or "generic" (wgrad_kernel<av, bv>); last_rows: rows of the last chunk."""


def pick_vec(width):
    return 4 if width % 64 == 0 else (2 if width % 32 == 0 else 1)


def wgrad_plan(rows, kin, nout, cus):
    """wgrad_plan and the kernel choice of tspgnn_wgrad_f32 (csrc/dense_bwd.hip)."""
    av, bv = pick_vec(kin), pick_vec(nout)
    nob = (kin // (16 * av)) * (nout // (16 * bv))
    target = max(cus * 8 // nob, 1)
    by_rows = (rows + 255) // 256
    nc = max(min(target, by_rows), 1)
    cr = ceil_div(rows, nc)
    cr = max((cr + 15) // 16 * 16, 16)
    nc = max(ceil_div(rows, cr), 1)
    kernel = "x3" if (av == 4 and bv == 4 and rows >= 4096) else "generic"
    return WgradPlan(kernel, av, bv, nob, nc, cr, rows - (nc - 1) * cr)


def wgrad_workspace_floats(rows, kin, nout, cus):
    """tspgnn_wgrad_workspace_floats."""
    if rows <= 0 or kin <= 0 or nout <= 0 or kin % 16 or nout % 16:
        return 0
    return wgrad_plan(rows, kin, nout, cus).n_chunks * (kin * nout + nout)


# ----------------------------------------------------------------------------------------------- tspgnn_wcolsum_f32
ColsumPlan = namedtuple("ColsumPlan", "n_chunks chunk_rows last_rows capped")
"""capped: the 4 * CUs cap on the chunk count took effect (chunks of more than 1024 rows)."""


def colsum_plan(rows, cus):
    """colsum_plan (csrc/train.hip)."""
    nc = (rows + 1023) // 1024
    cap = cus * 4
    capped = nc > cap
    nc = max(min(nc, cap), 1)
    cr = ceil_div(rows, nc)
    nc = max(ceil_div(rows, cr), 1)
    cr = max(cr, 1)
    return ColsumPlan(nc, cr, rows - (nc - 1) * cr, capped)


def wcolsum_workspace_floats(rows, d, cus):
    """tspgnn_wcolsum_workspace_floats."""
    return colsum_plan(max(rows, 1), cus).n_chunks * (d + 1)


def colsum_rows_in_flight(d):
    """RS of wcolsum_kernel: rows in flight per workgroup."""
    return 256 // (d // 4)


# --------------------------------------------------------------------------------------------- tspgnn_einit_bwd_f32
EinitBwdPlan = namedtuple("EinitBwdPlan", "grid n_chunks lo hi")
"""lo / hi: the fewest / most 64-edge chunks of a (persistent) workgroup."""


def einit_np(d):
    h1, h2, h3 = d // 8, d // 4, d // 2
    return 2 * h1 + h1 + h1 * h2 + h2 + h2 * h3 + h3 + h3 * d + d


def einit_bwd_full_grid(d, cus):
    """The persistent grid of tspgnn_einit_bwd_f32 before the clamp to the chunk count."""
    return cus * (1 if d >= 128 else 2)


def einit_bwd_plan(M, d, cus):
    """The grid of tspgnn_einit_bwd_f32 (csrc/train.hip) and the kernel's chunk += gridDim.x walk."""
    n_chunks = (M + 63) // 64
    grid = min(einit_bwd_full_grid(d, cus), n_chunks)
    per_wg = [len(range(b, n_chunks, grid)) for b in range(grid)]
    return EinitBwdPlan(grid, n_chunks, min(per_wg), max(per_wg))


def einit_bwd_workspace_floats(M, d):
    """tspgnn_einit_bwd_workspace_floats: one partial row per chunk (at least one per workgroup)."""
    return ((M + 63) // 64) * einit_np(d)


# ------------------------------------------------------------------------------------------------- reduce_partials2
def reduce_slices(n_chunks):
    """S of reduce_partials2 (csrc/dense_bwd.hip): slices of the chunk range per workgroup."""
    return 16 if n_chunks >= 64 else (4 if n_chunks >= 8 else 1)


# ------------------------------------------------------------------------------------ capped grid-stride launches
def strided_blocks(total, cap, per_block=256):
    """(workgroups, does a thread take a second element) of the launches that cap their grid and stride over the rest:
    tspgnn_tile_rows_f32 / tspgnn_rowdot_bwd_f32 (float4s, cap 4096), tspgnn_bucket_pack_f32 / _unpack_f32 (floats, 1024)."""
    blocks = max(min(ceil_div(total, per_block), cap), 1)
    return blocks, total > blocks * per_block
