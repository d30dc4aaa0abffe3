// Host side of the multi-task launches (tspgnn_*_multi_*), in one place: validating the tasks and dropping the empty ones,
// pricing them in 16-row tiles, clamping the grid and handing each task a contiguous share of the workgroups (blk_end[]).
// What is measured per kernel -- wavefronts per workgroup, workgroups per CU, LDS budgets, the cost formulas -- stays in
// the launcher beside that kernel.  Host-only: nothing here is seen by device code.
#pragma once
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
// half the grid.
inline int split_blocks_fixed(const long long* cost, const int* fixed, int n, int grid, int* blk_end) {
    int fixed_sum = 0, n_res = 0;
    long long res_cost[kMaxTasks];
    for (int k = 0; k < n; ++k) {
        fixed_sum += fixed[k];
        if (!fixed[k]) res_cost[n_res++] = cost[k];
    }
    if (n_res == 0 || fixed_sum == 0 || fixed_sum > grid / 2) return split_blocks(cost, n, grid, blk_end);
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

// tspgnn_mlp_bwd_task; first_live: the launch's first task with rows > 0 so far (NULL: none).  A task with pre_X may come
// without dY (the f16x2 entry; the fp32 entry rejects pre_X itself).
inline int check_mlp_bwd_task(tspgnn_mlp_bwd_task& t, int d, const tspgnn_mlp_bwd_task* first_live, const char* p) {
    const int rc = check_mlp_shape(t, p);
    if (rc) return rc;
    if (d == 128 && t.n_layers > 2) return fail(TSPGNN_EUNSUPPORTED, "%s: d=128 holds at most 2 layers in LDS (got %d)", p, t.n_layers);
    if (t.rows == 0) return TSPGNN_OK;
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

// tspgnn_cell_mlp_task (f16x2, bf16x3).  c == NULL passes here: the zero cell state of a run's first step for the f16x2
// kernel, which reads nothing then; so do outputs that alias the inputs.
inline int check_cell_mlp_task(const tspgnn_cell_mlp_task& ct, int d, const char* p) {
    const tspgnn_lstm_task& t = ct.cell;
    TSPGNN_REQUIRE(t.rows >= 0, "%s: rows=%d", p, t.rows);
    const int rc = check_rows_32bit(t.rows, t.dx, d, p);
    if (rc) return rc;
    TSPGNN_REQUIRE(t.dx >= 0 && t.dx % 32 == 0, "%s: dx=%d must be a non-negative multiple of 32", p, t.dx);
    TSPGNN_REQUIRE(ct.mlp_layers >= 0 && ct.mlp_layers <= 4, "%s: mlp_layers=%d must be in 0..4", p, ct.mlp_layers);
    if (t.rows == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(t.h && t.K && t.ln && t.h_out && t.c_out && (t.dx == 0 || t.x), "%s: null pointer", p);
    TSPGNN_REQUIRE(!t.uv || (t.dx == 0 && t.Zx), "%s: gather-init mode needs dx == 0 and Zx", p);
    TSPGNN_REQUIRE(!t.zbias || (t.zscale && !t.uv), "%s: zbias needs zscale and excludes gather-init mode", p);
    TSPGNN_REQUIRE(ct.mlp_layers == 0 || ct.mlp_wb, "%s: mlp_layers > 0 needs mlp_wb", p);
    TSPGNN_REQUIRE(!ct.proj_w || (ct.proj_out && ct.mlp_layers > 0), "%s: a projection needs proj_out and at least one MLP layer", p);
    return TSPGNN_OK;
}

// tspgnn_lstm_bwd_task.  fp32_mfma: the fp32 kernels step K by 16 rows (dx a multiple of 16, else 32) and gather only at
// d in {32, 64}.  KT / KTg / zbias are per arithmetic: at the entries.
inline int check_lstm_bwd_task(const tspgnn_lstm_bwd_task& t, int d, bool fp32_mfma, const char* p) {
    const int step = fp32_mfma ? 16 : 32;
    TSPGNN_REQUIRE(t.rows >= 0, "%s: rows=%d", p, t.rows);
    TSPGNN_REQUIRE(t.dx >= 0 && t.dx % step == 0, "%s: dx=%d must be a non-negative multiple of %d", p, t.dx, step);
    if (t.rows == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(t.h && t.c && t.K && t.ln && t.dz && t.dc_in && t.ln_grad && t.workspace && (t.dx == 0 || t.x),
                   "%s: null pointer", p);
    if (fp32_mfma)
        TSPGNN_REQUIRE(!t.uv || (t.dx == 0 && t.Zx && (d == 32 || d == 64)), "%s: gather-init mode needs dx == 0, Zx and d in {32,64}", p);
    else
        TSPGNN_REQUIRE(!t.uv || (t.dx == 0 && t.Zx), "%s: gather-init mode needs dx == 0 and Zx", p);
    return TSPGNN_OK;
}

}  // namespace tspgnn
