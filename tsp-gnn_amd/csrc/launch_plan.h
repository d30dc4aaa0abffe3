// Host side of the launches, in one place: validating the tasks and dropping the empty ones, pricing them in 16-row tiles,
// clamping the grid, handing each task a contiguous share of the workgroups (blk_end[]) -- and the PLANNERS: per kernel, a
// pure function of (task shapes, which pointers are null, width, CUs) that fills the plan structure of include/tspgnn.h with
// everything the launcher decides before its <<<>>>.  A launcher calls its planner with n_cus() taken once, copies the plan
// into the kernel's task table and launches (the three cell backward launchers through one frame, launch_cell_bwd); the
// tspgnn_plan_* queries answer the same planner to the tests.  What is
// measured per kernel -- wavefronts per workgroup, workgroups per CU, LDS budgets, the cost formulas -- stands in that
// kernel's planner.  Host-only: nothing here is seen by device code.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace tspgnn {

// 16-row tiles of a task
inline long long tiles16(int rows) { return ((long long)rows + 15) / 16; }

// min(grid, ceil(tiles_all / nw)): at least one tile per wavefront
inline int clamp_grid(int grid, long long tiles_all, int nw) {
    const long long max_grid = (tiles_all + nw - 1) / nw;
    return grid > max_grid ? (int)max_grid : grid;
}

// Workgroups per task, proportional to cost[k] (at least one each); grid = sum.
inline int split_blocks(const long long* cost, int n, int grid, int* blk_end) {
    long long total = 0;
    for (int k = 0; k < n; ++k) total += cost[k] > 0 ? cost[k] : 1;
    if (grid < n) grid = n;
    int used = 0;
    for (int k = 0; k < n; ++k) {
        const long long ck = cost[k] > 0 ? cost[k] : 1;
        int bk = (int)((ck * grid + total / 2) / total);
        if (bk < 1) bk = 1;
        used += bk;
        blk_end[k] = used;
    }
    return used;
}

// The same with some tasks at a set size: a task with fixed[k] > 0 gets exactly that many workgroups, the others share
// grid - sum(fixed) by cost.  The plain split when no task or every task is fixed, or the fixed ones would take more than
// half the grid; *kept_fixed says which of the two ran.
inline int split_blocks_fixed(const long long* cost, const int* fixed, int n, int grid, int* blk_end, int* kept_fixed) {
    int fixed_sum = 0, n_res = 0;
    long long res_cost[kMaxTasks];
    for (int k = 0; k < n; ++k) {
        fixed_sum += fixed[k];
        if (!fixed[k]) res_cost[n_res++] = cost[k];
    }
    *kept_fixed = !(n_res == 0 || fixed_sum == 0 || fixed_sum > grid / 2);
    if (!*kept_fixed) return split_blocks(cost, n, grid, blk_end);
    int res_end[kMaxTasks];
    split_blocks(res_cost, n_res, grid - fixed_sum, res_end);
    int used = 0, j = 0;
    for (int k = 0; k < n; ++k) {
        used += fixed[k] ? fixed[k] : res_end[j] - (j ? res_end[j - 1] : 0);
        if (!fixed[k]) ++j;
        blk_end[k] = used;
    }
    return used;
}

// Raises a kernel's dynamic-LDS limit to `bytes`; 0 or the positive hipError_t (message recorded under `what`, with the
// byte count where say_bytes).
template <class Kernel>
int set_dynamic_lds(Kernel* kernel, size_t bytes, const char* what, bool say_bytes = false) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) return TSPGNN_OK;
    if (say_bytes) return fail((int)e, "%s: hipFuncSetAttribute(%d B): %s", what, (int)bytes, hipGetErrorString(e));
    return fail((int)e, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
}

// Second stage of an LN-LSTM backward launch: folds each task's per-workgroup LayerNorm-gradient partials (one row per
// workgroup of blk_end[]) into its ln_grad, unless the task defers that to tspgnn_lnlstm_bwd_finish_f32.
inline int reduce_ln_partials(const tspgnn_lstm_bwd_task* tasks, int n, const int* blk_end, int D, hipStream_t st,
                              const char* what) {
    for (int k = 0; k < n; ++k) {
        if (tasks[k].defer_reduce) continue;
        const int nblk = blk_end[k] - (k ? blk_end[k - 1] : 0);
        reduce_partials(tasks[k].workspace, nblk, 10 * D, tasks[k].ln_grad, 10 * D, 1.0f, 1, st);
        const int rc = launched(what);
        if (rc) return rc;
    }
    return TSPGNN_OK;
}

// ------------------------------------------------------------------------------------------------------ validation
// Every check takes the prefix of its messages (`p`: an entry's name, or its historic short form) and answers TSPGNN_OK
// for a task with rows == 0 once the requirements that hold for empty tasks too have passed.

inline int task_rows(const tspgnn_cell_mlp_task& t) { return t.cell.rows; }
template <class Task>
int task_rows(const Task& t) { return t.rows; }

// live[0..*n) = copies of the tasks with rows > 0, in order; check(copy) validates a task (every task, empty ones too) and
// may fill in defaults.  live[] holds kMaxTasks tasks and n_tasks <= kMaxTasks.
template <class Task, class Check>
int filter_live(const Task* tasks, int n_tasks, Task* live, int* n, Check check) {
    *n = 0;
    for (int k = 0; k < n_tasks; ++k) {
        Task& t = live[*n];
        t = tasks[k];
        const int rc = check(t);
        if (rc) return rc;
        if (task_rows(t) > 0) ++*n;
    }
    return TSPGNN_OK;
}

// a stride of 0 beside a non-null array: the array is dense, layer after layer of [rows, d]
inline void default_stride(const void* array, long long* stride, int rows, int d) {
    if (array && *stride == 0) *stride = (long long)rows * d;
}

// tspgnn_mlp_task, tspgnn_mlp_task_bf16, tspgnn_mlp_bwd_task: what holds for an empty task too
template <class Task>
int check_mlp_shape(const Task& t, const char* p) {
    TSPGNN_REQUIRE(t.rows >= 0, "%s: rows=%d", p, t.rows);
    TSPGNN_REQUIRE(t.n_layers >= 1 && t.n_layers <= 4, "%s: n_layers=%d must be in 1..4", p, t.n_layers);
    return TSPGNN_OK;
}

// tspgnn_mlp_task / tspgnn_mlp_task_bf16 of the matrix-core forward entries (f16x2, bf16x3, bf16)
template <class Task>
int check_mlp_task(Task& t, int d, const char* p) {
    const int rc = check_mlp_shape(t, p);
    if (rc || t.rows == 0) return rc;
    TSPGNN_REQUIRE(t.X && t.wb && t.Y, "%s: null pointer", p);
    TSPGNN_REQUIRE(!t.proj_w || t.proj_out, "%s: projection needs proj_out", p);
    default_stride(t.acts, &t.acts_stride, t.rows, d);
    return TSPGNN_OK;
}

// tspgnn_mlp_bwd_task: what holds for an empty task too
inline int check_mlp_bwd_shape(const tspgnn_mlp_bwd_task& t, int d, const char* p) {
    const int rc = check_mlp_shape(t, p);
    if (rc) return rc;
    if (d == 128 && t.n_layers > 2) return fail(TSPGNN_EUNSUPPORTED, "%s: d=128 holds at most 2 layers in LDS (got %d)", p, t.n_layers);
    return TSPGNN_OK;
}

// tspgnn_mlp_bwd_task; first_live: the launch's first task with rows > 0 so far (NULL: none).  A task with pre_X may come
// without dY (the f16x2 entry; the fp32 entry rejects pre_X itself).
inline int check_mlp_bwd_task(tspgnn_mlp_bwd_task& t, int d, const tspgnn_mlp_bwd_task* first_live, const char* p) {
    const int rc = check_mlp_bwd_shape(t, d, p);
    if (rc || t.rows == 0) return rc;
    TSPGNN_REQUIRE((t.dY || t.pre_X) && t.wt, "%s: null pointer", p);
    const unsigned inner = t.relu_mask & ((1u << (t.n_layers - 1)) - 1u);
    TSPGNN_REQUIRE(!inner || t.acts, "%s: relu layers need the saved activations", p);
    TSPGNN_REQUIRE(!((t.relu_mask >> (t.n_layers - 1)) & 1u) || t.Yout, "%s: relu on the last layer needs Yout", p);
    TSPGNN_REQUIRE(!first_live || (t.acts_bf16 != 0) == (first_live->acts_bf16 != 0), "%s: the tasks of a launch share acts_bf16", p);
    default_stride(t.acts, &t.acts_stride, t.rows, d);
    default_stride(t.dpre, &t.dpre_stride, t.rows, d);
    return TSPGNN_OK;
}

// rows * max(4d, dx) < 2^30: the f16x2 / bf16x3 cell kernels and the f16x2 backward index rows with 32-bit offsets
inline int check_rows_32bit(int rows, int dx, int d, const char* p) {
    TSPGNN_REQUIRE((long long)rows * (4 * d > dx ? 4 * d : dx) < (1ll << 30), "%s: rows=%d too large for 32-bit offsets", p, rows);
    return TSPGNN_OK;
}

// tspgnn_cell_mlp_task (f16x2, bf16x3): the shape fields, what holds for an empty task too
inline int check_cell_mlp_shape(const tspgnn_cell_mlp_task& ct, int d, const char* p) {
    const tspgnn_lstm_task& t = ct.cell;
    TSPGNN_REQUIRE(t.rows >= 0, "%s: rows=%d", p, t.rows);
    const int rc = check_rows_32bit(t.rows, t.dx, d, p);
    if (rc) return rc;
    TSPGNN_REQUIRE(t.dx >= 0 && t.dx % 32 == 0, "%s: dx=%d must be a non-negative multiple of 32", p, t.dx);
    TSPGNN_REQUIRE(ct.mlp_layers >= 0 && ct.mlp_layers <= 4, "%s: mlp_layers=%d must be in 0..4", p, ct.mlp_layers);
    return TSPGNN_OK;
}

// tspgnn_cell_mlp_task (f16x2, bf16x3).  c == NULL passes here: the zero cell state of a run's first step for the f16x2
// kernel, which reads nothing then; so do outputs that alias the inputs.
inline int check_cell_mlp_task(const tspgnn_cell_mlp_task& ct, int d, const char* p) {
    const tspgnn_lstm_task& t = ct.cell;
    const int rc = check_cell_mlp_shape(ct, d, p);
    if (rc || t.rows == 0) return rc;
    TSPGNN_REQUIRE(t.h && t.K && t.ln && t.h_out && t.c_out && (t.dx == 0 || t.x), "%s: null pointer", p);
    TSPGNN_REQUIRE(!t.uv || (t.dx == 0 && t.Zx), "%s: gather-init mode needs dx == 0 and Zx", p);
    TSPGNN_REQUIRE(!t.zbias || (t.zscale && !t.uv), "%s: zbias needs zscale and excludes gather-init mode", p);
    TSPGNN_REQUIRE(ct.mlp_layers == 0 || ct.mlp_wb, "%s: mlp_layers > 0 needs mlp_wb", p);
    TSPGNN_REQUIRE(!ct.proj_w || (ct.proj_out && ct.mlp_layers > 0), "%s: a projection needs proj_out and at least one MLP layer", p);
    return TSPGNN_OK;
}

// tspgnn_lstm_bwd_task of the three cell backward entries and of their plan query (arith: TSPGNN_ARITH_F32 / _H2 / _BF16):
// the shape fields, the operands, and what each arithmetic offers.  The fp32 kernels step K by 16 rows (dx a multiple of 16,
// else 32) and gather only at d in {32, 64}; the f16x2 backward indexes rows with 32-bit offsets.  operands = false (the
// query, which reads no pointer as more than null or non-null) skips the null-pointer requirement alone.
inline int check_cell_bwd_mode(const tspgnn_lstm_bwd_task& t, int d, int arith, const char* p, bool operands = true) {
    const bool f32 = arith == TSPGNN_ARITH_F32;
    if (arith == TSPGNN_ARITH_H2) {
        const int rc = check_rows_32bit(t.rows, t.dx, d, p);
        if (rc) return rc;
    }
    TSPGNN_REQUIRE(t.rows >= 0, "%s: rows=%d", p, t.rows);
    const int step = f32 ? 16 : 32;
    TSPGNN_REQUIRE(t.dx >= 0 && t.dx % step == 0, "%s: dx=%d must be a non-negative multiple of %d", p, t.dx, step);
    if (t.rows == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(!operands || (t.h && t.c && t.K && t.ln && t.dz && t.dc_in && t.ln_grad && t.workspace && (t.dx == 0 || t.x)),
                   "%s: null pointer", p);
    if (f32)
        TSPGNN_REQUIRE(!t.uv || (t.dx == 0 && t.Zx && (d == 32 || d == 64)), "%s: gather-init mode needs dx == 0, Zx and d in {32,64}", p);
    else
        TSPGNN_REQUIRE(!t.uv || (t.dx == 0 && t.Zx), "%s: gather-init mode needs dx == 0 and Zx", p);
    if (f32) {
        TSPGNN_REQUIRE(!t.zbias && !t.KTg,
                       "%s: a bias-init z / a streamed data gradient are f16x2 features (tspgnn_lnlstm_bwd_multi_h2)", p);
    } else if (arith == TSPGNN_ARITH_H2) {
        TSPGNN_REQUIRE(!t.KT || (t.dxh && t.dx == 0), "%s: the fused data gradient needs dxh and dx == 0", p);
        TSPGNN_REQUIRE(!t.zbias || (t.zscale && !t.uv), "%s: zbias needs zscale and excludes gather-init mode", p);
        TSPGNN_REQUIRE(!t.KTg || (d == 64 && t.dx == 64 && t.dxg && t.dxh && !t.KT && !t.uv),
                       "%s: the streamed data gradient needs d == dx == 64, dxg, dxh and excludes KT / gather-init mode", p);
    } else {
        TSPGNN_REQUIRE(!t.KT && !t.dxh && !t.zbias && !t.KTg, "%s: no fused data gradient / bias-init in this mode", p);
    }
    return TSPGNN_OK;
}

// -------------------------------------------------------------------------------------------------------- planners
// Pure: no HIP call, no allocation, no global state but the two development switches below (read once).  `tasks` are the
// live tasks (rows > 0) of a launch, validated; `cus` the CU count.

// S of reduce_partials2: slices of the chunk range per workgroup (blockDim.x * S == 256)
inline int reduce_slices(int n_chunks) { return n_chunks >= 64 ? 16 : (n_chunks >= 8 ? 4 : 1); }

// Workgroups of a launch that caps its grid and strides over the rest: clamp(ceil(total / per_block), 1, cap)
inline int strided_blocks(long long total, int per_block, int cap) {
    const long long blocks = (total + per_block - 1) / per_block;
    return blocks > cap ? cap : (blocks < 1 ? 1 : (int)blocks);
}

// blk_end[] of the tasks by cost over the clamped grid: the tail of the planners that only share out workgroups
inline void plan_tasks(const long long* cost, long long tiles_all, int n, int grid, int nw, tspgnn_tasks_plan* p) {
    p->nw = nw;
    p->n = n;
    p->grid = split_blocks(cost, n, clamp_grid(grid, tiles_all, nw), p->blk_end);
    p->lds_bytes = 0;
}

// tspgnn_linear_f32; nt = (n1 + n2) / 16
inline void plan_linear(int kin, int nt, int rows, int cus, tspgnn_linear_plan* p) {
    const int tiles = (rows + 15) / 16;
    const int QT = kin / 16;
    const size_t per_q = (size_t)16 * nt * 16 * sizeof(float);
    int qc = QT;
    if ((size_t)QT * per_q + 16 > 150 * 1024) qc = (int)((128 * 1024) / per_q);
    const size_t lds_bytes = (size_t)qc * per_q + 16;
    p->qc = qc;
    p->tiles = tiles;
    p->lds_bytes = (int)lds_bytes;
    p->per_cu = lds_bytes > 80 * 1024 ? 1 : 2;
    const int grid = cus * p->per_cu;
    if (nt % 4 == 0 && qc >= QT && tiles <= cus * 4) {   // few tiles: split each tile's columns over four wavefronts
        p->path = TSPGNN_LINEAR_SPLIT;
        p->nw = 8;
        p->grid = (tiles + 1) / 2;
        return;
    }
    p->path = qc >= QT ? TSPGNN_LINEAR_TICKET : TSPGNN_LINEAR_STREAMED;
    p->nw = (qc >= QT && tiles <= grid * 4) ? 4 : 8;
    p->grid = clamp_grid(grid, tiles, p->nw);
}

// tspgnn_mlp_bwd_multi_f32 (d = 128 holds two layers in LDS, else four)
inline void plan_mlp_bwd(const tspgnn_mlp_bwd_task* tasks, int n, int d, int cus, tspgnn_tasks_plan* p) {
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    for (int k = 0; k < n; ++k) {
        const long long tiles = tiles16(tasks[k].rows);
        cost[k] = tiles * tasks[k].n_layers;
        tiles_all += tiles;
    }
    const int lds_bytes = (d >= 128 ? 2 : 4) * d * d * 4 + 16;
    const int grid = cus * (lds_bytes > 80 * 1024 ? 1 : 2);
    plan_tasks(cost, tiles_all, n, grid, tiles_all <= (long long)grid * 4 ? 4 : 8, p);
}

// tspgnn_mlp_fwd_multi_h2 / _x3, tspgnn_mlp_head_fwd_h2
inline void plan_mlp_fwd(const tspgnn_mlp_task* tasks, int n, int cus, tspgnn_tasks_plan* p) {
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    for (int k = 0; k < n; ++k) {
        cost[k] = tiles16(tasks[k].rows) * (tasks[k].n_layers + (tasks[k].proj_w ? 5 : 0));
        tiles_all += tiles16(tasks[k].rows);
    }
    int nw = 16;
    if (tiles_all <= (long long)cus * 16) nw = tiles_all <= (long long)cus * 4 ? 4 : 8;
    plan_tasks(cost, tiles_all, n, cus, nw, p);
}

// tspgnn_mlp_fwd_multi_f32 (d = 128 holds two layers in LDS, else four).  The LDS of a workgroup decides how many fit a CU:
// d = 64 -> 65 KiB -> two of 8 wavefronts.  Few tiles: one wavefront per SIMD and more workgroups.  Many tiles, two per CU:
// ONE workgroup of 16 wavefronts per CU instead -- the whole CU shares one ticket counter, so its four SIMDs finish within
// one tile of each other.
inline void plan_mlp_fwd_f32(const tspgnn_mlp_task* tasks, int n, int d, int cus, tspgnn_tasks_plan* p) {
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    for (int k = 0; k < n; ++k) {
        cost[k] = tiles16(tasks[k].rows) * (tasks[k].n_layers + (tasks[k].proj_w ? 5 : 0));
        tiles_all += tiles16(tasks[k].rows);
    }
    const int lds_bytes = (d >= 128 ? 2 : 4) * (d * d + d) * 4 + 16;
    const int per_cu = lds_bytes > 80 * 1024 ? 1 : 2;
    int grid = cus * per_cu;
    int nw = tiles_all <= (long long)grid * 4 ? 4 : 8;
    if (per_cu == 2 && tiles_all > (long long)grid * 16) {
        grid = cus;
        nw = 16;
    }
    plan_tasks(cost, tiles_all, n, grid, nw, p);
}

inline int pick_vec(int width) { return width % 64 == 0 ? 4 : (width % 32 == 0 ? 2 : 1); }

// tspgnn_wgrad_f32 / tspgnn_wgrad_bf16x_f32 (and the workspace size): the split of the row range, the kernel, its grid
inline void plan_wgrad(long long rows, int kin, int nout, bool bf16x, int cus, tspgnn_wgrad_plan* p) {
    const int av = pick_vec(kin), bv = pick_vec(nout);
    const int nob = (kin / (16 * av)) * (nout / (16 * bv));
    long long target = (long long)cus * 8 / nob;  // ~8 wavefronts per CU in total (HBM-bound: loads in flight)
    if (target < 1) target = 1;
    long long by_rows = (rows + 255) / 256;       // at least 256 rows per chunk
    long long nc = target < by_rows ? target : by_rows;
    if (nc < 1) nc = 1;
    long long cr = (rows + nc - 1) / nc;
    cr = (cr + 15) / 16 * 16;
    if (cr < 16) cr = 16;
    nc = (rows + cr - 1) / cr;
    if (nc < 1) nc = 1;
    p->av = av;
    p->bv = bv;
    p->nob = nob;
    p->n_chunks = (int)nc;
    p->chunk_rows = cr;
    if (bf16x) {   // (kin a multiple of 128: two X blocks per wavefront, every dY value is split once per 128 features)
        p->kernel = kin % 128 == 0 ? TSPGNN_WGRAD_X3_PAIR : TSPGNN_WGRAD_X3;
        p->launch_nob = (kin / (kin % 128 == 0 ? 128 : 64)) * (nout / 64);
    } else if (av == 4 && bv == 4 && rows >= 4096) {   // the big reductions over T*rows: bf16 matrix cores, fp32-class accuracy
        p->kernel = TSPGNN_WGRAD_X3;
        p->launch_nob = (kin / 64) * (nout / 64);
    } else {
        p->kernel = TSPGNN_WGRAD_GENERIC;
        p->launch_nob = nob;
    }
    p->grid = (int)((nc * p->launch_nob + 3) / 4);
}

// tspgnn_wcolsum_f32 (and the workspace size): chunks of about 1024 rows, at most 4 per CU
inline void plan_wcolsum(long long rows, int cus, tspgnn_wcolsum_plan* p) {
    long long nc = (rows + 1023) / 1024;
    const long long cap = (long long)cus * 4;
    p->capped = nc > cap;
    if (nc > cap) nc = cap;
    if (nc < 1) nc = 1;
    long long cr = (rows + nc - 1) / nc;
    nc = (rows + cr - 1) / cr;
    p->n_chunks = (int)(nc < 1 ? 1 : nc);
    p->chunk_rows = cr < 1 ? 1 : cr;
}

// tspgnn_einit_bwd_f32: persistent workgroups (LDS: 1 / 2 per CU) over 64-edge chunks
inline void plan_einit_bwd(int M, int d, int cus, tspgnn_einit_bwd_plan* p) {
    p->n_chunks = (M + 63) / 64;
    p->full_grid = cus * (d >= 128 ? 1 : 2);
    p->grid = p->full_grid > p->n_chunks ? p->n_chunks : p->full_grid;
}

// Working wavefronts per workgroup of a lock-step f16x2 cell task (development switch TSPGNN_H2_LOCK_TILES; default: all of
// them -- 8 / 6 / 4 measured 40.3 / 54.1 / 52.3 us per C2 launch against 37.9: the edge task misses the CUs more than the
// vertex chain gains from emptier matrix pipes).
inline int h2_lock_tiles() {
    static const int v = [] {
        const char* e = getenv("TSPGNN_H2_LOCK_TILES");
        const int x = e ? atoi(e) : 0;
        return (x >= 1 && x <= 16) ? x : 16;
    }();
    return v;
}

// Development switch TSPGNN_H2_WT=0/1 forces the write-through variant of the f16x2 cell launch off / on (-1: not set).
inline int h2_wt_forced() {
    static const int v = [] {
        const char* e = getenv("TSPGNN_H2_WT");
        return e ? atoi(e) : -1;
    }();
    return v;
}

// LDS residency of one f16x2 cell task: K and the MLP resident together, or lock-step rounds (K whole or in chunks of kbc
// k-blocks, then the MLP layers and -- `together`, where both fit -- the projection matrix).  false: does not fit.
inline bool cell_h2_residency(int KBT, int L, bool proj, int d, size_t per_kb, size_t budget, tspgnn_cell_fwd_plan* p, int k,
                              size_t* need) {
    const size_t layer_all = 2 * d * d * 2 + d * 4, proj_bytes = (size_t)2 * d * 4 * d * 2;
    const size_t k_bytes = (size_t)KBT * per_kb;
    if (k_bytes + L * layer_all <= budget && !proj) {
        p->kbc[k] = KBT;
        *need = k_bytes + L * layer_all;
        return true;
    }
    const int kbc = k_bytes <= budget ? KBT : (int)(budget / per_kb);
    if (kbc < 1 || L * layer_all > budget || (proj && proj_bytes > budget)) return false;
    p->kbc[k] = kbc;
    p->lockstep[k] = 1;
    *need = (size_t)kbc * per_kb;
    size_t second = L * layer_all;
    if (proj) {
        if (L * layer_all + proj_bytes <= budget) {
            p->together[k] = 1;
            second += proj_bytes;
        } else if (proj_bytes > second) {
            second = proj_bytes;
        }
    }
    if (second > *need) *need = second;
    return true;
}

// The same for a bf16x3 task: resident needs hi, mid and the biases of every MLP layer in LDS beside K (the lo pieces of
// n_lo_lds layers where they fit); the kernel selects the lock step by kbc < KBT, so a K that would fit whole goes in
// chunks of KBT - 1 there.
inline bool cell_x3_residency(int KBT, int L, bool proj, int d, size_t per_kb, size_t budget, tspgnn_cell_fwd_plan* p, int k,
                              size_t* need) {
    const size_t layer_hm = (size_t)2 * d * d * 2, layer_lo = (size_t)d * d * 2, layer_all = 3 * d * d * 2 + d * 4;
    const size_t proj_bytes = (size_t)3 * d * 4 * d * 2;
    const size_t k_bytes = (size_t)KBT * per_kb;
    const size_t mlp_min = L * (layer_hm + d * 4);
    if (k_bytes + mlp_min <= budget && !proj) {
        p->kbc[k] = KBT;
        int n_lo = (int)((budget - k_bytes - mlp_min) / layer_lo);
        if (n_lo > L) n_lo = L;
        p->n_lo_lds[k] = n_lo;
        *need = k_bytes + mlp_min + n_lo * layer_lo;
        return true;
    }
    int kbc = k_bytes <= budget ? KBT : (int)(budget / per_kb);
    if (kbc >= KBT) kbc = KBT - 1;
    if (kbc < 1 || L * layer_all > budget || (proj && proj_bytes > budget)) return false;
    p->kbc[k] = kbc;
    p->lockstep[k] = 1;
    p->n_lo_lds[k] = L;
    *need = (size_t)kbc * per_kb;
    if (L * layer_all > *need) *need = L * layer_all;
    if (proj && proj_bytes > *need) *need = proj_bytes;
    return true;
}

// tspgnn_lnlstm_mlp_fwd_multi_h2 / _x3 (arith: TSPGNN_ARITH_*; d in {32, 64}).  -1, or the index of the (first) task whose
// K chunk, MLP or projection matrix does not fit LDS: TSPGNN_EUNSUPPORTED.
inline int plan_cell_fwd(const tspgnn_cell_mlp_task* tasks, int n, int d, int arith, int cus, tspgnn_cell_fwd_plan* p) {
    const bool h2 = arith == TSPGNN_ARITH_H2;
    const size_t head = (10 * d + 4) * sizeof(float);
    const size_t per_kb = (size_t)(h2 ? 2 : 3) * 32 * 4 * d * 2;  // bytes of one k-block, two / three pieces
    const size_t budget = 160 * 1024 - head;
    *p = tspgnn_cell_fwd_plan{};
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    size_t lds_w = 0;
    for (int k = 0; k < n; ++k) {
        const int L = tasks[k].mlp_layers;
        const bool proj = tasks[k].proj_w != nullptr;
        const int KBT = (tasks[k].cell.dx + d) / 32;
        size_t need;
        if (!(h2 ? cell_h2_residency : cell_x3_residency)(KBT, L, proj, d, per_kb, budget, p, k, &need)) return k;
        if (need > lds_w) lds_w = need;
        const long long tiles = tiles16(tasks[k].cell.rows);
        cost[k] = tiles * (KBT * 4 + 2 * L + (proj ? 8 : 0) + (h2 ? 8 : 6));
        tiles_all += tiles;
    }
    p->n = n;
    p->lds_bytes = (int)(lds_w + head);
    const int nw = tiles_all <= (long long)cus * 4 ? 4 : (tiles_all <= (long long)cus * 8 ? 8 : 12);
    const int grid = clamp_grid(cus, tiles_all, nw);
    p->nw = nw;
    // A lock-step task is a latency chain (LDS re-stagings every round) that the resident tasks of the launch hide.  It
    // gets the workgroups of a whole number of rounds; the resident tasks share the rest by cost.
    // bf16x3: exactly ONE round (more workgroups would idle, fewer would double the chain), capped at half the grid.
    // f16x2: ONE round while that stays within about twice its share of the grid by cost (C2's 320 vertex tiles take 27
    // of 256), otherwise as many rounds as bring it back to its share (C4's 1 586 vertex tiles: 5 rounds on 27 workgroups
    // instead of starving the edge task of 133).  (Figures at 256 CUs and 12 working wavefronts: tspgnn_plan_cell_fwd.)
    long long total_cost = 0;
    for (int k = 0; k < n; ++k) total_cost += cost[k] > 0 ? cost[k] : 1;
    int fixed[kMaxTasks];
    for (int k = 0; k < n; ++k) {
        fixed[k] = 0;
        if (!p->lockstep[k]) continue;
        const long long tiles = tiles16(tasks[k].cell.rows);
        const int lw = h2 && h2_lock_tiles() < nw ? h2_lock_tiles() : nw;
        const long long per_round = (tiles + lw - 1) / lw;
        long long n_rounds = 1;
        if (h2) {
            long long share = (2 * cost[k] * grid + total_cost - 1) / total_cost;  // twice the proportional share
            if (share < 1) share = 1;
            n_rounds = (per_round + share - 1) / share;
        }
        p->lock_tiles[k] = lw;
        p->n_rounds[k] = (int)n_rounds;
        fixed[k] = (int)((per_round + n_rounds - 1) / n_rounds);
    }
    p->grid = split_blocks_fixed(cost, fixed, n, grid, p->blk_end, &p->split_fixed);
    if (!h2) return -1;
    bool centered = true, loop_buffers = false;
    long long out_bytes = 0;   // h', c' of every task and its messages: what the launch stores (and the next ones re-read)
    for (int k = 0; k < n; ++k) {
        centered = centered && tasks[k].cell.z_centered != 0;
        out_bytes += (long long)tasks[k].cell.rows * d * 4 * (tasks[k].mlp_out ? 3 : 2);
        loop_buffers = loop_buffers || tasks[k].state_out_blocked != 0 || tasks[k].mlp_out != nullptr || tasks[k].proj_out != nullptr;
    }
    // write-through output stores while the loop's arrays (two copies of the states, two of the messages: ~2x out_bytes)
    // stay inside the 256 MB Infinity Cache; plain stores beyond (see st4o) -- and for a launch that writes nothing the next
    // step's launch reads from these buffers (no blocked state, no messages: the training forward's cell launch stores
    // into the tape, which the backward reads much later -- C2 training step 10.25-10.27 -> 10.12-10.16 ms)
    p->centered = centered;
    p->wt = h2_wt_forced() >= 0 ? h2_wt_forced() != 0 : (loop_buffers && 2 * out_bytes <= (long long)200 * 1024 * 1024);
    return -1;
}

// what plan_cell_fwd's caller answers for the task it names
inline int cell_does_not_fit(const tspgnn_cell_mlp_task& t, int d, const char* what) {
    return fail(TSPGNN_EUNSUPPORTED, "%s: dx=%d, d=%d, %d MLP layers do not fit LDS", what, t.cell.dx, d, t.mlp_layers);
}

// ------------------------------------------------------------ cell launches that keep K resident or stream it in chunks
// The LayerNorm tail of a cell backward workgroup's LDS: the 10 d parameters, nw wavefront slabs of 10 d partials, 4 words.
inline size_t ln_tail_bytes(int d, int nw) { return (size_t)(10 * d + nw * 10 * d + 4) * sizeof(float); }

// Units of K (per_unit bytes each: a 16-row block of fp32, a 32-row k-block of bf16) per LDS chunk under `budget`: all
// `total` of them where they fit (resident), else as many as fit (0: not even one).
inline int k_units_per_chunk(int total, size_t per_unit, size_t budget) {
    return (size_t)total * per_unit > budget ? (int)(budget / per_unit) : total;
}

// bf16 K, shared by the bf16 backward and the bf16 forward cell: task k's k-blocks per chunk into p (false: none fits), its
// bytes into *lds_k (the launch's maximum), and its tiles priced per_tile + KBT each, twice where K is streamed.
inline bool plan_bf16_k(int rows, int dx, int d, size_t budget, int per_tile, tspgnn_cell_chunk_plan* p, int k, size_t* lds_k,
                        long long* cost) {
    const size_t per_kb = (size_t)32 * 4 * d * 2;
    const int KBT = (dx + d) / 32;
    const int kbc = k_units_per_chunk(KBT, per_kb, budget);
    if (kbc < 1) return false;
    p->qc[k] = kbc;
    p->chunked[k] = kbc < KBT;
    if ((size_t)kbc * per_kb > *lds_k) *lds_k = (size_t)kbc * per_kb;
    *cost = tiles16(rows) * (KBT + per_tile) * (kbc < KBT ? 2 : 1);
    return true;
}

// Most wavefronts per workgroup of the cell backward kernels = their NWMAX template argument.  fp32 and bf16: D = 128 keeps
// 4D/16 + temporaries > 256 registers live, one wavefront per SIMD (512-register budget).
#ifndef H2_BWD_NW
#define H2_BWD_NW 8
#endif
constexpr int cell_bwd_nwmax(int d, int arith) { return arith == TSPGNN_ARITH_H2 ? H2_BWD_NW : (d >= 128 ? 4 : 8); }

// tspgnn_lnlstm_bwd_multi_f32 / _h2 / _bf16 (arith: TSPGNN_ARITH_F32 / _H2 / _BF16).  TSPGNN_EUNSUPPORTED, by the first task
// that does not fit, where the launch is refused.
inline int plan_cell_bwd(const tspgnn_lstm_bwd_task* tasks, int n, int d, int arith, int cus, tspgnn_cell_chunk_plan* p) {
    const int nwmax = cell_bwd_nwmax(d, arith);
    const size_t budget = 160 * 1024 - ln_tail_bytes(d, nwmax);
    *p = tspgnn_cell_chunk_plan{};
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    size_t lds_k = 0;
    bool any_chunked = false;
    for (int k = 0; k < n; ++k) {
        const tspgnn_lstm_bwd_task& t = tasks[k];
        const long long tiles = tiles16(t.rows);
        if (arith == TSPGNN_ARITH_BF16) {
            if (!plan_bf16_k(t.rows, t.dx, d, budget, 12, p, k, &lds_k, &cost[k]))
                return fail(TSPGNN_EUNSUPPORTED, "lnlstm_bwd_bf16: d=%d does not fit LDS", d);
        } else if (arith == TSPGNN_ARITH_H2) {   // never chunked (qc = 0)
            size_t need = (size_t)(t.dx + d) * 4 * d * 4;               // two fp16 pieces
            if (t.KT != nullptr) need += (size_t)4 * d * d * 4;
            if (need > budget)
                return fail(TSPGNN_EUNSUPPORTED, "lnlstm_bwd_h2: dx=%d, d=%d%s does not fit LDS", t.dx, d,
                            t.KT ? " with K^T" : "");
            if (need > lds_k) lds_k = need;
            cost[k] = tiles * ((t.dx + d) / 32 + (t.KT ? 2 : 0) + (t.KTg ? 5 : 0) + 10);
        } else {
            const size_t per_q = (size_t)16 * 4 * d * sizeof(float);
            const int QT = (t.dx + d) / 16;
            const int qc = k_units_per_chunk(QT, per_q, budget);
            if (qc < QT && (qc < 1 || t.uv)) return fail(TSPGNN_EUNSUPPORTED, "lnlstm_bwd: d=%d does not fit LDS", d);
            size_t need = (size_t)qc * per_q;
            if (t.KT != nullptr) {
                need += (size_t)4 * d * (t.dx + d) * sizeof(float);
                if (d != 64 || t.dx != 0 || qc < QT || need > budget)
                    return fail(TSPGNN_EUNSUPPORTED,
                                "lnlstm_bwd: the fused data gradient needs d=64, dx=0 and K, K^T resident in LDS");
            }
            p->qc[k] = qc;
            p->chunked[k] = qc < QT;
            if (need > lds_k) lds_k = need;
            cost[k] = tiles * (QT + 8);  // k-blocks + ~8 blocks' worth of elementwise backward
        }
        any_chunked = any_chunked || p->chunked[k];
        tiles_all += tiles;
    }
    // four wavefronts while every one of them still has a tile -- the fp32 rounds of a chunked K and the bf16 kernel
    // always run all of them
    const bool few = arith != TSPGNN_ARITH_BF16 && !any_chunked && tiles_all <= (long long)cus * 4;
    p->n = n;
    p->nw = few ? 4 : nwmax;
    p->lds_bytes = (int)(lds_k + ln_tail_bytes(d, p->nw));
    p->grid = split_blocks(cost, n, clamp_grid(cus, tiles_all, p->nw), p->blk_end);
    return TSPGNN_OK;
}

// The frame of the three cell backward launchers: plan, the kernel's table from the plan, the launch, and the second stage
// over the LayerNorm-gradient partials.  (The workspace holds one row of partials per workgroup of a task: n_cus + 8 rows,
// tspgnn_lnlstm_bwd_workspace_floats.)  p: the prefix of the LDS message; what / what_reduce: the launches' names.
template <class Table>
int launch_cell_bwd(void (*kernel)(Table), const tspgnn_lstm_bwd_task* tasks, int n, int d, int arith, hipStream_t st,
                    const char* p, const char* what, const char* what_reduce) {
    tspgnn_cell_chunk_plan pl;
    int rc = plan_cell_bwd(tasks, n, d, arith, n_cus(), &pl);
    if (rc) return rc;
    Table tt;
    for (int k = 0; k < n; ++k) {
        tt.task[k] = tasks[k];
        tt.qc[k] = pl.qc[k];
        tt.blk_end[k] = pl.blk_end[k];
    }
    tt.n = n;
    if ((rc = set_dynamic_lds(kernel, pl.lds_bytes, p))) return rc;
    kernel<<<pl.grid, pl.nw * 64, pl.lds_bytes, st>>>(tt);
    if ((rc = launched(what))) return rc;
    return reduce_ln_partials(tasks, n, pl.blk_end, d, st, what_reduce);
}

// Workgroups of lnlstm_fwd_chunked_kernel for one task: its 8 wavefronts take one tile each per round, round r goes to
// workgroup r mod grid.
inline int lstm_fwd_chunked_grid(int rows, int cus) {
    const long long rounds = (tiles16(rows) + 7) / 8;
    return cus > rounds ? (int)rounds : cus;
}

// tspgnn_lnlstm_fwd_multi_f32.  A task whose K ([dx + d, 4d] floats) fits 160 KiB of LDS beside the LayerNorm parameters is
// RESIDENT: all of them share one launch of lnlstm_fwd_kernel, which nw, grid, blk_end[] and lds_bytes describe (blk_end[k]
// runs over the resident tasks in order; a chunked task owns no workgroup there, blk_end[k] == blk_end[k - 1]; grid 0: no
// resident task).  A task whose K does not fit is CHUNKED: a launch of its own of lnlstm_fwd_chunked_kernel, 8 wavefronts,
// K in chunks of qc[k] 16-row blocks (as many as fit 128 KiB), lstm_fwd_chunked_grid workgroups.  That kernel starts z at
// zero: a chunked gather-init or bias-init task is TSPGNN_EUNSUPPORTED -- for the whole launch, before anything runs.
inline int plan_lstm_fwd_f32(const tspgnn_lstm_task* tasks, int n, int d, int cus, tspgnn_cell_chunk_plan* p) {
    const size_t extra = (10 * d + 4) * sizeof(float);
    const size_t per_q = (size_t)16 * 4 * d * sizeof(float);
    *p = tspgnn_cell_chunk_plan{};
    long long cost[kMaxTasks];
    int res[kMaxTasks];
    int n_res = 0;
    long long tiles_all = 0;
    size_t resident = 0;
    for (int k = 0; k < n; ++k) {
        const int QT = (tasks[k].dx + d) / 16;
        const size_t r = (size_t)QT * per_q + extra;
        p->chunked[k] = r > 160 * 1024;
        p->qc[k] = p->chunked[k] ? (int)((128 * 1024) / per_q) : QT;
        if (p->chunked[k]) {
            if (tasks[k].uv || tasks[k].zbias)
                return fail(TSPGNN_EUNSUPPORTED, "lnlstm_fwd: gather-init / zbias need K[%d,%d] resident in LDS", d, 4 * d);
            continue;
        }
        const long long tiles = tiles16(tasks[k].rows);
        cost[n_res] = tiles * (QT + 3);  // k-blocks + ~3 blocks' worth of epilogue
        res[n_res++] = k;
        tiles_all += tiles;
        if (r > resident) resident = r;
    }
    p->n = n;
    // Few tiles (a lone vertex-side task): one wavefront per SIMD and more, smaller workgroups, so every tile gets a matrix
    // pipe to itself; many tiles: one workgroup per CU, two wavefronts per SIMD.
    p->nw = n_res && tiles_all <= (long long)cus * 4 ? 4 : 8;
    if (n_res == 0) return TSPGNN_OK;
    int end[kMaxTasks];
    p->grid = split_blocks(cost, n_res, clamp_grid(cus, tiles_all, p->nw), end);
    p->lds_bytes = (int)resident;
    for (int k = 0, j = 0, used = 0; k < n; ++k) {
        if (j < n_res && res[j] == k) used = end[j++];
        p->blk_end[k] = used;
    }
    return TSPGNN_OK;
}

// tspgnn_lnlstm_fwd_multi_bf16 at the nw wavefronts per workgroup of the kernel its dispatch chose
inline int plan_lstm_fwd_bf16(const tspgnn_lstm_task_bf16* tasks, int n, int d, int nw, int cus, tspgnn_cell_chunk_plan* p) {
    const size_t head = (10 * d + 4) * sizeof(float);
    *p = tspgnn_cell_chunk_plan{};
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    size_t lds_w = 0;
    for (int k = 0; k < n; ++k) {
        if (!plan_bf16_k(tasks[k].rows, tasks[k].dx, d, 156 * 1024 - head, 4, p, k, &lds_w, &cost[k]))
            return fail(TSPGNN_EUNSUPPORTED, "lnlstm_fwd_bf16: d=%d does not fit LDS", d);
        tiles_all += tiles16(tasks[k].rows);
    }
    p->n = n;
    p->nw = nw;
    p->lds_bytes = (int)(lds_w + head);
    p->grid = split_blocks(cost, n, clamp_grid(cus, tiles_all, nw), p->blk_end);
    return TSPGNN_OK;
}

// tspgnn_mlp_fwd_multi_bf16, likewise: LDS holds the layers of the deepest task or a projection matrix, whichever is larger
inline int plan_mlp_fwd_bf16(const tspgnn_mlp_task_bf16* tasks, int n, int d, int nw, int cus, tspgnn_tasks_plan* p) {
    long long cost[kMaxTasks];
    long long tiles_all = 0;
    size_t lds_w = 0;
    for (int k = 0; k < n; ++k) {
        const size_t need = tasks[k].proj_w ? (size_t)d * 4 * d * 2 : 0;
        const size_t lay = (size_t)tasks[k].n_layers * (d * d * 2 + d * 4);
        lds_w = lds_w > need ? lds_w : need;
        lds_w = lds_w > lay ? lds_w : lay;
        cost[k] = tiles16(tasks[k].rows) * (tasks[k].n_layers + (tasks[k].proj_w ? 5 : 0));
        tiles_all += tiles16(tasks[k].rows);
    }
    const size_t lds_bytes = lds_w + 16;
    if (lds_bytes > 160 * 1024) return fail(TSPGNN_EUNSUPPORTED, "mlp_fwd_bf16: %zu bytes of weights do not fit LDS", lds_bytes);
    plan_tasks(cost, tiles_all, n, cus, nw, p);
    p->lds_bytes = (int)lds_bytes;
    return TSPGNN_OK;
}

}  // namespace tspgnn
