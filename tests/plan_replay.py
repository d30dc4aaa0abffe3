"""The launch plans of the fp32 backward kernels (csrc/dense_bwd.hip), the training-tail kernels (csrc/train.hip), the
forward cell and MLP launchers (csrc/dense.hip, csrc/dense_h2.hip, csrc/dense_x3.hip, csrc/bf16.hip) and the three cell backward launchers
(csrc/dense_bwd.hip, csrc/dense_bwd_h2.hip, csrc/dense_bwd_bf16.hip), asked of the library: every launcher-level figure
here -- path, wavefronts, grid, blk_end, LDS chunking, mode, variant, chunk counts -- is what the tspgnn_plan_* queries
answer, and those run the planner the launcher itself calls (csrc/launch_plan.h).  The GPU tests that claim a branch
(tests/test_gpu_fp32_backward_plans.py, tests/test_gpu_batch_kernels.py, tests/test_gpu_cell_forward_edges.py, tests/test_gpu_fp32_forward_edges.py, and through
tests/lstm_bwd_cases.py tests/test_gpu_h2_backward_kernels.py and tests/test_gpu_bf16_backward_kernels.py) derive
their row counts from the device's CU count and assert the branch and its depth through these functions BEFORE they
launch.  What remains in Python follows a KERNEL's own loop from the plan -- a workgroup's ticket range, its rounds, the
rows of a last chunk -- and names the line it follows.  tests/golden/launch_plans.json records the answers across the
thresholds (tools/launch_plan_table.py).

Nothing here touches a device."""
from collections import namedtuple

from tspgnn import _lib


def ceil_div(a, b):
    return (a + b - 1) // b


def tiles16(rows):
    """tiles_total of the tiled kernels: 16 rows per MFMA tile."""
    return (rows + 15) // 16


def blocks_of(plan):
    """Workgroups per task from blk_end[] (the kernels' my_grid = blk_end[k] - blk_end[k - 1])."""
    end = list(plan.blk_end[:plan.n])
    return [e - b for b, e in zip([0] + end, end)]


def ticket_shares(tiles, my_grid):
    """Tiles of every workgroup of a ticket task: t_end - t_beg with t_beg = tiles * b / my_grid (linear_kernel,
    mlp_bwd_kernel)."""
    return [tiles * (b + 1) // my_grid - tiles * b // my_grid for b in range(my_grid)]


def strided_walk(n, my_grid):
    """Iterations of every workgroup of a loop `r = my_blk; r < n; r += my_grid`."""
    return [len(range(b, n, my_grid)) for b in range(my_grid)]


# ---------------------------------------------------------------------------------------------- tspgnn_linear_f32
LinearPlan = namedtuple("LinearPlan", "path nw grid qc per_cu tiles rounds lo hi dead")
"""path: "split" (linear_split_kernel: W resident, the columns of a tile over four wavefronts, two tiles per workgroup),
"ticket" (linear_kernel, W resident, tiles pulled through a ticket inside the workgroup's [t_beg, t_end)) or "streamed"
(linear_kernel, W through LDS qc 16-row blocks at a time, rounds of nw tiles, round r to workgroup r mod grid).
rounds: streamed only, all rounds of the launch.  lo / hi: the fewest / most tiles a workgroup hands to one wavefront SLOT
(ticket: its share of tiles over nw, rounded down / up; streamed: its rounds; split: 1).  dead: streamed only, the tiles of
the last round that do not exist."""


def linear_plan(kin, n1, n2, rows, cus):
    """tspgnn_plan_linear, and linear_kernel's walk of its tiles."""
    p = _lib.plan("tspgnn_plan_linear", kin, n1, n2, rows, cus)
    path = ("split", "ticket", "streamed")[p.path]
    if path == "split":
        return LinearPlan(path, p.nw, p.grid, p.qc, p.per_cu, p.tiles, None, 1, 1, None)
    if path == "ticket":
        share = ticket_shares(p.tiles, p.grid)
        return LinearPlan(path, p.nw, p.grid, p.qc, p.per_cu, p.tiles, None, min(share) // p.nw, ceil_div(max(share), p.nw), None)
    rounds = ceil_div(p.tiles, p.nw)                  # linear_kernel: rounds = (tiles_total + nw - 1) / nw
    per_wg = strided_walk(rounds, p.grid)             # r = blockIdx.x; r < rounds; r += gridDim.x
    return LinearPlan(path, p.nw, p.grid, p.qc, p.per_cu, p.tiles, rounds, min(per_wg), max(per_wg), rounds * p.nw - p.tiles)


# ---------------------------------------------------------------------------------------- tspgnn_mlp_bwd_multi_f32
MlpBwdPlan = namedtuple("MlpBwdPlan", "nw grid blocks lo hi")
"""blocks: workgroups per task; lo / hi: per task, the fewest / most tiles of a workgroup per wavefront slot (share over
nw, rounded down / up)."""


def mlp_bwd_plan(tasks, d, cus):
    """tspgnn_plan_mlp_bwd.  tasks: [(rows, n_layers)] of the live tasks (rows > 0)."""
    p = _lib.plan("tspgnn_plan_mlp_bwd", [_lib.MlpBwdTask(rows=rows, n_layers=L) for rows, L in tasks], len(tasks), d, cus)
    blocks = blocks_of(p)
    shares = [ticket_shares(tiles16(rows), nb) for (rows, _), nb in zip(tasks, blocks)]
    return MlpBwdPlan(p.nw, p.grid, blocks, [min(s) // p.nw for s in shares], [ceil_div(max(s), p.nw) for s in shares])


# ------------------------------------------------------------------------------------------------ tspgnn_wgrad_f32
WgradPlan = namedtuple("WgradPlan", "kernel av bv nob n_chunks chunk_rows last_rows")
"""kernel: "x3" (wgrad_x3_kernel) or "generic" (wgrad_kernel<av, bv>); last_rows: rows of the last chunk."""


def pick_vec(width):
    """AV (= BV) of wgrad_kernel for a feature width: what the planner answers for it."""
    return _lib.plan("tspgnn_plan_wgrad", 1, width, width, 0, 1).av


def wgrad_plan(rows, kin, nout, cus):
    """tspgnn_plan_wgrad for tspgnn_wgrad_f32; the kernels' chunk c covers rows [c * chunk_rows, min(rows, ...))."""
    p = _lib.plan("tspgnn_plan_wgrad", rows, kin, nout, 0, cus)
    return WgradPlan(("generic", "x3")[p.kernel], p.av, p.bv, p.nob, p.n_chunks, p.chunk_rows, rows - (p.n_chunks - 1) * p.chunk_rows)


def wgrad_workspace_floats(rows, kin, nout, cus):
    """tspgnn_wgrad_workspace_floats: a [kin, nout] partial and a bias row per chunk; 0 for a shape the entry rejects."""
    try:
        return _lib.plan("tspgnn_plan_wgrad", rows, kin, nout, 0, cus).n_chunks * (kin * nout + nout)
    except _lib.TspgnnError:
        return 0


# ----------------------------------------------------------------------------------------------- tspgnn_wcolsum_f32
ColsumPlan = namedtuple("ColsumPlan", "n_chunks chunk_rows last_rows capped")
"""capped: the 4 * CUs cap on the chunk count took effect (chunks of more than 1024 rows)."""


def colsum_plan(rows, cus):
    """tspgnn_plan_wcolsum; wcolsum_kernel's workgroup c covers rows [c * chunk_rows, min(rows, ...))."""
    p = _lib.plan("tspgnn_plan_wcolsum", rows, 4, cus)
    return ColsumPlan(p.n_chunks, p.chunk_rows, rows - (p.n_chunks - 1) * p.chunk_rows, bool(p.capped))


def wcolsum_workspace_floats(rows, d, cus):
    """tspgnn_wcolsum_workspace_floats: d column partials and a weight sum per chunk."""
    return colsum_plan(max(rows, 1), cus).n_chunks * (d + 1)


def colsum_rows_in_flight(d):
    """RS of wcolsum_kernel: rows in flight per workgroup."""
    return 256 // (d // 4)


# --------------------------------------------------------------------------------------------- tspgnn_einit_bwd_f32
EinitBwdPlan = namedtuple("EinitBwdPlan", "grid n_chunks lo hi")
"""lo / hi: the fewest / most 64-edge chunks of a (persistent) workgroup."""


def einit_np(d):
    """einit_np (csrc/train.hip): parameters of the E_init MLP 2 -> d/8 -> d/4 -> d/2 -> d, a partial row's length."""
    h1, h2, h3 = d // 8, d // 4, d // 2
    return 2 * h1 + h1 + h1 * h2 + h2 + h2 * h3 + h3 + h3 * d + d


def einit_bwd_full_grid(d, cus):
    """The persistent grid of tspgnn_einit_bwd_f32 before the clamp to the chunk count."""
    return _lib.plan("tspgnn_plan_einit_bwd", 1, d, cus).full_grid


def einit_bwd_plan(M, d, cus):
    """tspgnn_plan_einit_bwd and einit_bwd_kernel's chunk += gridDim.x walk."""
    p = _lib.plan("tspgnn_plan_einit_bwd", M, d, cus)
    per_wg = strided_walk(p.n_chunks, p.grid)
    return EinitBwdPlan(p.grid, p.n_chunks, min(per_wg), max(per_wg))


def einit_bwd_workspace_floats(M, d):
    """tspgnn_einit_bwd_workspace_floats: one partial row per chunk (at least one per workgroup)."""
    return _lib.plan("tspgnn_plan_einit_bwd", M, d, 1).n_chunks * einit_np(d)


# ------------------------------------------------------------------------------------------------- reduce_partials2
def reduce_slices(n_chunks):
    """S of reduce_partials2 (csrc/dense_bwd.hip): slices of the chunk range per workgroup."""
    return _lib.lib.tspgnn_plan_reduce_slices(n_chunks)


# ------------------------------------------------------------------------------------ capped grid-stride launches
def strided_blocks(total, cap, per_block=256):
    """(workgroups, does a thread take a second element) of the launches that cap their grid and stride over the rest:
    tspgnn_tile_rows_f32 / tspgnn_rowdot_bwd_f32 (float4s, cap 4096), tspgnn_bucket_pack_f32 / _unpack_f32 (floats, 1024)."""
    blocks = _lib.lib.tspgnn_plan_strided_blocks(total, per_block, cap)
    return blocks, total > blocks * per_block


# ------------------------------------------------------- tspgnn_lnlstm_mlp_fwd_multi_{h2,x3}, tspgnn_mlp_fwd_multi_{h2,x3}
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
"""split: "fixed" (the lock-step tasks kept their set share of the workgroups) or "plain" (all by cost).  centered / wt: the template variant (h2; always False for x3).
tasks: a CellTaskPlan per task."""


def cell_fwd_plan(tasks, d, cus, arith="h2"):
    """tspgnn_plan_cell_fwd.  tasks: (rows, dx, mlp_layers, has_proj, out_blocked, has_mlp_out, z_centered) of the live
    tasks (rows > 0), in order.  Raises ValueError where the launcher answers TSPGNN_EUNSUPPORTED."""
    assert arith in ("h2", "x3") and d in (32, 64) and 1 <= len(tasks) <= 4
    structs = [_lib.CellMlpTask(cell=_lib.LstmTask(rows=rows, dx=dx, z_centered=int(zc)), mlp_layers=L, proj_w=int(proj),
                                proj_out=int(proj), mlp_out=int(mlp_out), state_out_blocked=int(out_blk))
               for rows, dx, L, proj, out_blk, mlp_out, zc in tasks]
    try:
        p = _lib.plan("tspgnn_plan_cell_fwd", structs, len(tasks), d, ("h2", "x3").index(arith), cus)
    except _lib.TspgnnError as e:
        if e.status != -2:
            raise
        raise ValueError(e.message)
    blocks = blocks_of(p)
    plans = []
    for k, (rows, dx, *_) in enumerate(tasks):
        tiles, KBT = tiles16(rows), (dx + d) // 32            # the kernels' tiles_total and KBT
        if not p.lockstep[k]:
            plans.append(CellTaskPlan("resident", p.kbc[k], 1, False, 0, 0, None, blocks[k], tiles, None, None,
                                      ticket_ranges(tiles, blocks[k], xcd=arith == "h2")))
            continue
        rounds = ceil_div(tiles, p.lock_tiles[k])             # rounds = (tiles_total + lw - 1) / lw
        per_wg = strided_walk(rounds, blocks[k])              # r = my_blk; r < rounds; r += my_grid
        plans.append(CellTaskPlan("lockstep", p.kbc[k], ceil_div(KBT, p.kbc[k]),        # kb0 = 0; kb0 < KBT; kb0 += kbc
                                  arith == "h2" and KBT <= 4,                           # pre = KBT <= KBP
                                  p.together[k], p.lock_tiles[k], p.n_rounds[k], blocks[k], tiles, rounds,
                                  (min(per_wg), max(per_wg)), None))
    return CellLaunchPlan(p.nw, p.grid, list(p.blk_end[:p.n]), "fixed" if p.split_fixed else "plain", bool(p.centered),
                          bool(p.wt), p.lds_bytes, plans)


def cell_task(rows, dx=0, mlp_layers=0, proj=False, out_blocked=False, mlp_out=False, z_centered=False):
    """One task for cell_fwd_plan."""
    return (rows, dx, mlp_layers, bool(proj), bool(out_blocked), bool(mlp_out), bool(z_centered))


MlpFwdPlan = namedtuple("MlpFwdPlan", "nw grid blocks ranges")
"""blocks: workgroups per task; ranges: per task, every workgroup's [t_beg, t_end)."""


def mlp_fwd_plan(tasks, cus):
    """tspgnn_plan_mlp_fwd (launch_mlp_h2 and launch_mlp_x3 share the planner; tspgnn_mlp_head_fwd_h2 is the one-task
    launch).  tasks: [(rows, n_layers, has_proj)] of the live tasks."""
    p = _lib.plan("tspgnn_plan_mlp_fwd", [_lib.MlpTask(rows=rows, n_layers=L, proj_w=int(proj)) for rows, L, proj in tasks],
                  len(tasks), 64, cus)
    blocks = blocks_of(p)
    return MlpFwdPlan(p.nw, p.grid, blocks, [ticket_ranges(tiles16(rows), b, xcd=False) for (rows, _, _), b in zip(tasks, blocks)])


# ------------------------------------------------- tspgnn_lnlstm_bwd_multi_{f32,h2,bf16}, tspgnn_{lnlstm,mlp}_fwd_multi_bf16
def unsupported_as_value_error(query, *args):
    """_lib.plan, with ValueError where the launcher answers TSPGNN_EUNSUPPORTED."""
    try:
        return _lib.plan(query, *args)
    except _lib.TspgnnError as e:
        if e.status != -2:
            raise
        raise ValueError(e.message)


CellChunkPlan = namedtuple("CellChunkPlan", "nw grid blocks qc chunked lds_bytes")
"""blocks: workgroups per task; qc: units of K per LDS chunk (16-row blocks for the fp32 backward, 32-row k-blocks for bf16,
0 for the f16x2 backward, which never chunks); chunked: K streamed through LDS rather than resident, per task."""


def _chunk_plan(p):
    return CellChunkPlan(p.nw, p.grid, blocks_of(p), list(p.qc[:p.n]), [bool(c) for c in p.chunked[:p.n]], p.lds_bytes)


def cell_bwd_plan(tasks, d, cus, arith):
    """tspgnn_plan_cell_bwd.  tasks: (rows, dx, with_KT, with_KTg[, gather]) of the live tasks (rows > 0), in order; a task
    with K^T is a gather-init task unless said otherwise.  The outputs each mode wants (dxh, dxg) and Zx count as given.
    Raises ValueError where the launcher answers TSPGNN_EUNSUPPORTED."""
    structs = []
    for rows, dx, kt, ktg, *gather in tasks:
        gather = bool(gather[0]) if gather else bool(kt)
        structs.append(_lib.LstmBwdTask(rows=rows, dx=dx, KT=int(bool(kt)), KTg=int(bool(ktg)), dxh=int(bool(kt or ktg)),
                                        dxg=int(bool(ktg)), uv=int(gather), Zx=int(gather)))
    arith = {"h2": 0, "f32": 2, "bf16": 3}[arith]           # TSPGNN_ARITH_*
    return _chunk_plan(unsupported_as_value_error("tspgnn_plan_cell_bwd", structs, len(tasks), d, arith, cus))


LSTM_FWD_BF16_NW = {32: (8,), 64: (12, 8), 128: (8,)}
"""NW of the kernel tspgnn_lnlstm_fwd_multi_bf16 dispatches to, per d (csrc/bf16.hip); the first is the default, the second
the all-gates kernel behind the development switch TSPGNN_BF16_CELL=0."""


def lstm_fwd_bf16_plan(tasks, d, cus, nw=None):
    """tspgnn_plan_lstm_fwd_bf16.  tasks: (rows, dx) of the live tasks."""
    nw = LSTM_FWD_BF16_NW[d][0] if nw is None else nw
    structs = [_lib.LstmTaskB(rows=rows, dx=dx) for rows, dx in tasks]
    return _chunk_plan(unsupported_as_value_error("tspgnn_plan_lstm_fwd_bf16", structs, len(tasks), d, nw, cus))


MlpFwdBf16Plan = namedtuple("MlpFwdBf16Plan", "nw grid blocks lds_bytes")


def mlp_fwd_bf16_plan(tasks, d, cus):
    """tspgnn_plan_mlp_fwd_bf16 at the NW of the entry's dispatch (csrc/bf16.hip: 16 at d = 128 when no task has a projection,
    else 8).  tasks: [(rows, n_layers, has_proj)] of the live tasks."""
    nw = 16 if d == 128 and not any(proj for _, _, proj in tasks) else 8
    structs = [_lib.MlpTaskB(rows=rows, n_layers=L, proj_w=int(proj)) for rows, L, proj in tasks]
    p = unsupported_as_value_error("tspgnn_plan_mlp_fwd_bf16", structs, len(tasks), d, nw, cus)
    return MlpFwdBf16Plan(p.nw, p.grid, blocks_of(p), p.lds_bytes)


# ------------------------------------------------------------------- tspgnn_mlp_fwd_multi_f32, tspgnn_lnlstm_fwd_multi_f32
def mlp_fwd_f32_plan(tasks, d, cus):
    """tspgnn_plan_mlp_fwd_f32 -> MlpFwdPlan over the live tasks (rows > 0; the entry drops the others).  tasks: [(rows,
    n_layers, has_proj)]; mlp_fwd_kernel walks [t_beg, t_end) by the plain workgroup index."""
    structs = [_lib.MlpTask(rows=rows, n_layers=L, proj_w=int(proj), proj_out=int(proj)) for rows, L, proj in tasks]
    p = _lib.plan("tspgnn_plan_mlp_fwd_f32", structs, len(tasks), d, cus)
    blocks, live = blocks_of(p), [t for t in tasks if t[0] > 0]
    assert len(blocks) == len(live)
    return MlpFwdPlan(p.nw, p.grid, blocks, [ticket_ranges(tiles16(rows), b, xcd=False) for (rows, _, _), b in zip(live, blocks)])


LstmFwdF32Plan = namedtuple("LstmFwdF32Plan", "nw grid blocks qc chunked lds_bytes ranges chunks chunk_grid rounds_per_wg")
"""nw, grid, blocks, lds_bytes: the ONE launch of the resident tasks (lnlstm_fwd_kernel; grid 0: none; a chunked task has 0
blocks there).  qc / chunked: per task.  ranges: per resident task every workgroup's [t_beg, t_end) (None: chunked).  Per
chunked task (None: resident), its own launch of lnlstm_fwd_chunked_kernel at 8 wavefronts: chunks, the lengths in 16-row
blocks of the stagings of K (q0 = 0; q0 < QT; q0 += qc); chunk_grid, its workgroups min(cus, rounds) with rounds =
ceil(tiles / 8); rounds_per_wg, the (fewest, most) rounds of a workgroup (r = blockIdx.x; r < rounds; r += gridDim.x)."""


def lstm_fwd_f32_plan(tasks, d, cus):
    """tspgnn_plan_lstm_fwd_f32, over the live tasks (rows > 0; the entry drops the others).  tasks: (rows, dx, mode), mode
    "plain", "gather" or "bias".  Raises ValueError where the launch answers TSPGNN_EUNSUPPORTED."""
    structs = [_lib.LstmTask(rows=rows, dx=dx, uv=int(mode == "gather"), Zx=int(mode == "gather"), zbias=int(mode == "bias"),
                             zscale=int(mode == "bias")) for rows, dx, mode in tasks]
    p = unsupported_as_value_error("tspgnn_plan_lstm_fwd_f32", structs, len(tasks), d, cus)
    c, live = _chunk_plan(p), [t for t in tasks if t[0] > 0]
    assert len(c.blocks) == len(live)
    ranges, chunks, grids, per_wg = [], [], [], []
    for (rows, dx, _), blocks, qc, chunked in zip(live, c.blocks, c.qc, c.chunked):
        tiles, QT = tiles16(rows), (dx + d) // 16
        if not chunked:
            ranges.append(ticket_ranges(tiles, blocks, xcd=False))
            chunks.append(None), grids.append(None), per_wg.append(None)
            continue
        rounds = ceil_div(tiles, 8)                          # rounds = (tiles_total + 7) / 8
        grid = min(cus, rounds)                              # launch_lnlstm: lstm_fwd_chunked_grid
        walk = strided_walk(rounds, grid)
        ranges.append(None)
        chunks.append([min(QT, q0 + qc) - q0 for q0 in range(0, QT, qc)])
        grids.append(grid)
        per_wg.append((min(walk), max(walk)))
    return LstmFwdF32Plan(c.nw, c.grid, c.blocks, c.qc, c.chunked, c.lds_bytes, ranges, chunks, grids, per_wg)
