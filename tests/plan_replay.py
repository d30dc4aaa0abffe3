"""Replay of the host-side launch plans of the fp32 backward kernels (csrc/dense_bwd.hip), the training-tail kernels
(csrc/train.hip) and -- last section -- the forward cell and MLP launchers (csrc/dense_h2.hip, csrc/dense_x3.hip): plain
functions of (shape, cus) that follow the C++ line by line and answer the branch taken and its grid.  The GPU tests that
claim a branch (tests/test_gpu_fp32_backward_plans.py, tests/test_gpu_batch_kernels.py,
tests/test_gpu_cell_forward_edges.py) derive their row counts from the device's CU count and assert the branch and its
depth through these functions BEFORE they launch; tests/test_plan_replay_host.py pins the functions against the library
wherever the library exposes a plan (the workspace-size queries), tests/test_cell_fwd_replay_host.py the forward launchers
at the shapes the project runs.  A launcher that changes must be changed here too -- the host test, or a "deep" test's own
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


# ------------------------------------------------------- tspgnn_lnlstm_mlp_fwd_multi_{h2,x3}, tspgnn_mlp_fwd_multi_{h2,x3}
# The forward cell launchers launch_cell_h2 (csrc/dense_h2.hip) and launch_cell_x3 (csrc/dense_x3.hip), the MLP launchers
# launch_mlp_h2 / launch_mlp_x3, split_blocks_fixed (csrc/launch_plan.h) and xcd_contiguous (csrc/common.h), restated.
# They must follow the launchers and the kernels' own tile ranges: a change there has to be made here too, or the tests
# that assert a branch through them (tests/test_gpu_cell_forward_edges.py) stop knowing what they reach --
# tests/test_cell_fwd_replay_host.py pins the figures of the shapes the project runs.
LDS_BUDGET = 160 * 1024
H2_LOCK_TILES = 16      # h2_lock_tiles() without its development switch
WT_FOOTPRINT = 200 * 1024 * 1024


def split_blocks_fixed(cost, fixed, grid):
    """split_blocks_fixed (csrc/launch_plan.h) -> (workgroups per task, "fixed" or "plain": which split ran)."""
    fixed_sum = sum(fixed)
    res = [c for c, f in zip(cost, fixed) if not f]
    if not res or fixed_sum == 0 or fixed_sum > grid // 2:
        return split_blocks(cost, grid), "plain"
    it = iter(split_blocks(res, grid - fixed_sum))
    return [f if f else next(it) for f in fixed], "fixed"


def xcd_contiguous(b, n):
    """xcd_contiguous (csrc/common.h): workgroup b of n -> its position, the workgroups of one XCD (b mod 8) consecutive."""
    per, rem, x = n >> 3, n & 7, b & 7
    return x * per + min(x, rem) + (b >> 3)


def ticket_ranges(tiles, my_grid, xcd=True):
    """[t_beg, t_end) of every workgroup of a resident task (lnlstm_mlp_fwd_h2_kernel through xcd_contiguous; the x3 kernel
    and the MLP kernels by the plain workgroup index)."""
    pos = [xcd_contiguous(b, my_grid) if xcd else b for b in range(my_grid)]
    return [(tiles * p // my_grid, tiles * (p + 1) // my_grid) for p in pos]


CellTaskPlan = namedtuple("CellTaskPlan", "mode kbc chunks preload together lock_tiles n_rounds blocks tiles rounds "
                                          "rounds_per_wg ranges")
"""mode: "resident" (K and the MLP staged once, tiles by ticket) or "lockstep" (one tile per working wavefront and round).
kbc: k-blocks per LDS chunk; chunks: stagings of K per round; preload: the lock-step operand preload (KBT <= 4, h2 only).
together: MLP layers and projection matrix in one residency (h2 lock-step).  lock_tiles: working wavefronts per workgroup.
n_rounds: the launcher's rounds per workgroup behind the task's fixed share (None: resident).  blocks: its workgroups.
rounds: all lock-step rounds, ceil(tiles / lock_tiles); rounds_per_wg: (fewest, most) rounds of a workgroup, the kernel's
r = my_blk; r < rounds; r += my_grid.  ranges: resident, every workgroup's [t_beg, t_end)."""

CellLaunchPlan = namedtuple("CellLaunchPlan", "nw grid blk_end split centered wt lds_bytes tasks")
"""split: "fixed" or "plain" (split_blocks_fixed).  centered / wt: the template variant (h2; always False for x3).
tasks: a CellTaskPlan per task."""


def cell_fwd_plan(tasks, d, cus, arith="h2"):
    """launch_cell_h2<D> / launch_cell_x3<D>.  tasks: (rows, dx, mlp_layers, has_proj, out_blocked, has_mlp_out, z_centered)
    of the live tasks (rows > 0), in order.  Raises ValueError where the launcher answers TSPGNN_EUNSUPPORTED."""
    assert arith in ("h2", "x3") and d in (32, 64) and 1 <= len(tasks) <= 4
    pieces = 2 if arith == "h2" else 3
    head = (10 * d + 4) * 4
    per_kb = pieces * 32 * 4 * d * 2
    budget = LDS_BUDGET - head
    layer_all = pieces * d * d * 2 + d * 4
    proj_bytes = pieces * d * 4 * d * 2
    mode, kbcs, together, cost, tiles, lds_w = [], [], [], [], [], 0
    for rows, dx, L, proj, _, _, _ in tasks:
        assert rows > 0 and dx % 32 == 0 and 0 <= L <= 4 and (not proj or L > 0)
        KBT = (dx + d) // 32
        k_bytes = KBT * per_kb
        tog = 0
        if arith == "h2":
            if k_bytes + L * layer_all <= budget and not proj:
                kbc, lock, need = KBT, False, k_bytes + L * layer_all
            else:
                kbc = KBT if k_bytes <= budget else budget // per_kb
                if kbc < 1 or L * layer_all > budget or (proj and proj_bytes > budget):
                    raise ValueError("dx=%d, d=%d, %d MLP layers do not fit LDS" % (dx, d, L))
                lock, need, second = True, kbc * per_kb, L * layer_all
                if proj:
                    if L * layer_all + proj_bytes <= budget:
                        tog = 1
                        second += proj_bytes
                    elif proj_bytes > second:
                        second = proj_bytes
                need = max(need, second)
        else:
            layer_hm, layer_lo = 2 * d * d * 2, d * d * 2
            mlp_min = L * (layer_hm + d * 4)          # resident: hi, mid and the biases must be in LDS
            if k_bytes + mlp_min <= budget and not proj:
                n_lo = min((budget - k_bytes - mlp_min) // layer_lo, L)
                kbc, lock, need = KBT, False, k_bytes + mlp_min + n_lo * layer_lo
            else:
                kbc = KBT if k_bytes <= budget else budget // per_kb
                if kbc >= KBT:
                    kbc = KBT - 1                     # lock-step mode is selected by kbc < KBT
                if kbc < 1 or L * layer_all > budget or (proj and proj_bytes > budget):
                    raise ValueError("dx=%d, d=%d, %d MLP layers do not fit LDS" % (dx, d, L))
                lock, need = True, max(kbc * per_kb, L * layer_all, proj_bytes if proj else 0)
        lds_w = max(lds_w, need)
        n = tiles16(rows)
        mode.append("lockstep" if lock else "resident")
        kbcs.append(kbc)
        together.append(tog)
        tiles.append(n)
        cost.append(n * (KBT * 4 + 2 * L + (8 if proj else 0) + (8 if arith == "h2" else 6)))
    tiles_all = sum(tiles)
    nw = 4 if tiles_all <= cus * 4 else (8 if tiles_all <= cus * 8 else 12)
    grid = clamp_grid(cus, tiles_all, nw)
    total_cost = sum(c if c > 0 else 1 for c in cost)
    fixed, lock_tiles, n_rounds = [], [], []
    for k, m in enumerate(mode):
        if m != "lockstep":
            fixed.append(0), lock_tiles.append(0), n_rounds.append(None)
        elif arith == "h2":
            lw = min(nw, H2_LOCK_TILES)
            per_round = ceil_div(tiles[k], lw)
            share = max(ceil_div(2 * cost[k] * grid, total_cost), 1)     # twice the proportional share
            nr = ceil_div(per_round, share)
            fixed.append(ceil_div(per_round, nr)), lock_tiles.append(lw), n_rounds.append(nr)
        else:
            fixed.append(ceil_div(tiles[k], nw)), lock_tiles.append(nw), n_rounds.append(1)
    blocks, split = split_blocks_fixed(cost, fixed, grid)
    centered = arith == "h2" and all(t[6] for t in tasks)
    out_bytes = sum(rows * d * 4 * (3 if mlp_out else 2) for rows, _, _, _, _, mlp_out, _ in tasks)
    loop_buffers = any(out_blk or mlp_out or proj for _, _, _, proj, out_blk, mlp_out, _ in tasks)
    wt = arith == "h2" and loop_buffers and 2 * out_bytes <= WT_FOOTPRINT
    plans = []
    for k, (rows, dx, L, proj, _, _, _) in enumerate(tasks):
        KBT = (dx + d) // 32
        if mode[k] == "resident":
            plans.append(CellTaskPlan("resident", kbcs[k], 1, False, 0, 0, None, blocks[k], tiles[k], None, None,
                                      ticket_ranges(tiles[k], blocks[k], xcd=arith == "h2")))
        else:
            rounds = ceil_div(tiles[k], lock_tiles[k])
            per_wg = [len(range(b, rounds, blocks[k])) for b in range(blocks[k])]
            plans.append(CellTaskPlan("lockstep", kbcs[k], ceil_div(KBT, kbcs[k]), arith == "h2" and KBT <= 4, together[k],
                                      lock_tiles[k], n_rounds[k], blocks[k], tiles[k], rounds, (min(per_wg), max(per_wg)),
                                      None))
    blk_end = [sum(blocks[:k + 1]) for k in range(len(blocks))]
    return CellLaunchPlan(nw, blk_end[-1], blk_end, split, centered, wt, lds_w + head, plans)


def cell_task(rows, dx=0, mlp_layers=0, proj=False, out_blocked=False, mlp_out=False, z_centered=False):
    """One task for cell_fwd_plan."""
    return (rows, dx, mlp_layers, bool(proj), bool(out_blocked), bool(mlp_out), bool(z_centered))


MlpFwdPlan = namedtuple("MlpFwdPlan", "nw grid blocks ranges")
"""blocks: workgroups per task; ranges: per task, every workgroup's [t_beg, t_end)."""


def mlp_fwd_plan(tasks, cus):
    """launch_mlp_h2<D> / launch_mlp_x3<D> (the same arithmetic; tspgnn_mlp_head_fwd_h2 is the one-task launch).
    tasks: [(rows, n_layers, has_proj)] of the live tasks."""
    tiles = [tiles16(rows) for rows, _, _ in tasks]
    cost = [n * (L + (5 if proj else 0)) for n, (_, L, proj) in zip(tiles, tasks)]
    tiles_all = sum(tiles)
    nw = 16
    if tiles_all <= cus * 16:
        nw = 4 if tiles_all <= cus * 4 else 8
    blocks = split_blocks(cost, clamp_grid(cus, tiles_all, nw))
    return MlpFwdPlan(nw, sum(blocks), blocks, [ticket_ranges(n, b, xcd=False) for n, b in zip(tiles, blocks)])
