/*
 * tspgnn.h -- C ABI of libtspgnn.so: the MI355X (gfx950) implementation of the TSP-GNN
 * message-passing hot path.
 *
 * The reference (machine-reasoning-ufrgs/TSP-GNN) has no FFI of its own: the boundary of this
 * path is the TensorFlow op set its Python graph lowers to.  Each entry point below replaces
 * one such op group; the reference line it replaces is cited on the declaration
 * (paths are relative to the reference repository root).  INTEGRATION.md shows the ctypes
 * binding a maintainer adds on the reference side.
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is retained or freed;
 *   - every function takes the HIP stream to enqueue on (hipStream_t passed as void*;
 *     NULL = the default stream), launches asynchronously, never synchronises, never
 *     allocates, keeps no mutable global state (re-entrant across streams and devices);
 *   - return value: 0 = OK, <0 = TSPGNN_E* below, >0 = the hipError_t of a failed launch;
 *     nothing throws across the ABI; tspgnn_last_error() returns a thread-local message;
 *   - matrices are row-major contiguous fp32, rows of d floats; d must be 32, 64 or 128
 *     for the MFMA kernels (mlp, lnlstm), any multiple of 4 for the aggregation kernels;
 *   - index arrays are int32.
 */
#ifndef TSPGNN_H
#define TSPGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSPGNN_OK 0
#define TSPGNN_EINVAL (-1)      /* bad argument (null pointer, negative size, unsupported d) */
#define TSPGNN_EUNSUPPORTED (-2) /* valid request this build has no kernel for */

#define TSPGNN_ABI_VERSION 5   /* 2: range_flag in the task structures, pack_weights_h2 / adam_clip_step arguments;
                                  3: tspgnn_mp_loop_h2 (the whole T-step loop as one launch);
                                  4: tspgnn_mp_resident_h2 (the loop as one launch, states through memory);
                                  5: tspgnn_lstm_bwd_task.KTg / dxg, tspgnn_mlp_bwd_task.pre_X / pre_wt / pre_k (the vertex
                                     side's data-gradient GEMMs inside the step's two backward launches) */

/* ABI version of the loaded library (== TSPGNN_ABI_VERSION of the header it was built from). */
int tspgnn_version(void);

/* Thread-local description of the last non-zero status returned on this thread ("" if none). */
const char* tspgnn_last_error(void);

/* ------------------------------------------------------------------ aggregation (the SpMM) */

/*
 * Y[e,:] = X[uv[e,0],:] + X[uv[e,1],:]                                 e in [0,M)
 * Replaces tf.matmul(EV, y) at graphnn.py:156-160 (E update, adjoint_a=False) for an EV whose
 * rows hold exactly two ones (instance_loader.py:63-66).  X:[N,d]  Y:[M,d]  uv:[M,2].
 */
int tspgnn_gather2_sum_f32(const int32_t* uv, const float* X, float* Y,
                           int M, int N, int d, void* stream);

/*
 * Y[v,:] = sum_{k in [rowptr[v],rowptr[v+1])} X[eid[k],:]               v in [0,N)
 * Replaces tf.matmul(EV, y, adjoint_a=True) at graphnn.py:156-160 (V update): EV^T in
 * pattern-only CSR (all stored values are 1).  Summation order is ascending k
 * (deterministic).  X:[M,d]  Y:[N,d]  rowptr:[N+1]  eid:[nnz].
 */
int tspgnn_csr_rowsum_f32(const int32_t* rowptr, const int32_t* eid, const float* X, float* Y,
                          int N, int M, int d, void* stream);

/*
 * Both aggregations of one message-passing step in one launch (they are independent: every update
 * reads the OLD states, graphnn.py:143):  Ye = EV Xv  (gather, as tspgnn_gather2_sum_f32)  and
 * Yv = EV^T Xe  (row-sum, as tspgnn_csr_rowsum_f32).  Xv:[N,d] Ye:[M,d] Xe:[M,d] Yv:[N,d]; d in
 * {32,64,128,256}.  Shares the chip between the two streams instead of two launch latencies.
 */
int tspgnn_spmm_pair_f32(const int32_t* uv, const float* Xv, float* Ye, const int32_t* rowptr,
                         const int32_t* eid, const float* Xe, float* Yv, int M, int N, int d, void* stream);

/*
 * Y[r,:] = sum_k val[k] * X[col[k],:], k in [rowptr[r],rowptr[r+1])     r in [0,R)
 * General valued CSR product for GraphNN matrices that are not 0/1 patterns
 * (graphnn.py:156-160 with an arbitrary `mat`).  X:[C,d]  Y:[R,d].
 */
int tspgnn_csr_spmm_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                        const float* X, float* Y, int R, int C, int d, void* stream);

/* ------------------------------------------------------------------ dense updates (MFMA) */

/*
 * P = W reordered into the MFMA A-fragment order the dense kernels stage into LDS (layout
 * documented in csrc/dense.hip).  W:[krows,ncols] row-major; krows % 16 == 0; ncols == 32 or
 * ncols % 64 == 0.  transposed != 0: W is stored [ncols,krows] and P packs W^T (the backward
 * kernels multiply by the transposed weights).  Run once per weight update (the reference re-reads its tf.Variables every
 * sess.run; here the packed copy is refreshed after initialisation / restore / Adam).
 */
int tspgnn_pack_weights_f32(const float* W, float* P, int krows, int ncols, int transposed, void* stream);

/*
 * n_layers (1..4) chained tf.layers.Dense(d) layers: x <- act_l(x W_l + b_l); layer l applies
 * relu iff bit l of relu_mask is set.  Replaces Mlp.__call__ (mlp.py:57-63) as instantiated
 * for the message MLPs (graphnn.py:114-125,153) and the hidden part of E_vote
 * (model.py:107-115).  X,Y:[rows,d].  wb: per layer pack_weights(W[d,d] (in x out)) followed
 * by b[d], layers back to back ((d*d+d) floats each).  If acts != NULL the post-activation
 * output of every layer but the last is stored at acts + l*acts_stride + row*d (backward);
 * acts_stride (floats) = 0 means rows*d.
 */
int tspgnn_mlp_fwd_f32(const float* X, const float* wb, float* Y, float* acts, long long acts_stride,
                       int rows, int d, int n_layers, unsigned relu_mask, void* stream);

/*
 * One tf.contrib.rnn.LayerNormBasicLSTMCell(d, activation=relu) step, the cell call at
 * graphnn.py:168-170:  z=[x,h]K; i,j,f,o = LN_k(split(z)); c'=LN_s(c*sig(f+1)+sig(i)*relu(j));
 * h'=relu(c')*sig(o).  x:[rows,dx]  h,c,h_out,c_out:[rows,d]  K: pack_weights(kernel[dx+d,4d])
 * ln: [5][2][d] = (gamma,beta) for input, transform, forget, output, state.
 * h_out/c_out may not alias h/c.  dx must be a multiple of 16.
 */
int tspgnn_lnlstm_fwd_f32(const float* x, int dx, const float* h, const float* c,
                          const float* K, const float* ln, float* h_out, float* c_out,
                          int rows, int d, void* stream);

/*
 * The same cell step with the adjacency product folded through the GEMM (fast path of the E update,
 * graphnn.py:156-170): z = Zx[uv[e,0]] + Zx[uv[e,1]] + h Kh, where Zx = V_msg_E(V.h) Kx is formed once
 * per VERTEX by tspgnn_linear_f32 ((EV y) Kx = EV (y Kx): the x-half of the GEMM moves from the M edge
 * rows to the N vertex rows).  Zx:[n_src,4d]  Kh: pack_weights(kernel[dx:, :]) = [d,4d].
 */
int tspgnn_lnlstm_gather_fwd_f32(const int32_t* uv, const float* Zx, const float* h, const float* c,
                                 const float* Kh, const float* ln, float* h_out, float* c_out,
                                 int rows, int n_src, int d, void* stream);

/*
 * Several independent tasks in ONE launch (<= 4): the workgroups are divided among the tasks in
 * proportion to their work and each stages its own task's weights.  One message-passing step runs the
 * edge-side and vertex-side MLPs as one launch and the two cells as another, so the small vertex-side
 * problems do not pay their own launch, weight staging and tail (graphnn.py:144-171 iterates the
 * variables; the updates of one step are mutually independent because they all read the OLD states).
 * The task arrays live in HOST memory; all pointers inside are device pointers.
 */
typedef struct tspgnn_mlp_task {
    const float* X; const float* wb; float* Y; float* acts; long long acts_stride;
    int rows; int n_layers; unsigned relu_mask;
    const float* proj_w; float* proj_out;  /* optional: proj_out[rows,4d] = Y * P, proj_w = pack_weights(P[d,4d]) */
    unsigned* range_flag;  /* _h2 entry points only (optional, others ignore it): device word, |= 1 when an activation
                              left the fp16 range of the f16x2 split at the top, |= 2 (cell entry points) when a gate row's
                              spread fell below the split's absolute error at the bottom (see tspgnn_pack_weights_h2) */
} tspgnn_mlp_task;   /* fields as the arguments of tspgnn_mlp_fwd_f32 */

typedef struct tspgnn_lstm_task {
    const float* x; int dx; const float* h; const float* c; const float* K; const float* ln;
    float* h_out; float* c_out; int rows;
    const int32_t* uv; const float* Zx;   /* gather-init mode when uv != NULL: dx == 0, K = Kh */
    const float* zbias; const float* zscale; /* optional: z starts at zscale[row] * zbias[4d] (a bias folded
                                                through a row-sum aggregation: degree * (b Kx)) */
    unsigned* range_flag;                    /* as tspgnn_mlp_task.range_flag */
    int z_centered;                          /* a promise, not a request: every row of z = [x|h] K (+ Zx[u] + Zx[v], + zscale
                                                * zbias) has zero mean over each gate's d columns, because the caller centred
                                                the columns of K (and of the Kx behind Zx, and zbias) per gate -- LayerNorm
                                                subtracts that mean anyway, and the subtraction commutes with the product.
                                                The f16x2 cell kernels then skip the mean pass of the four gate LayerNorms;
                                                every other entry point ignores the field. */
} tspgnn_lstm_task;  /* fields as the arguments of tspgnn_lnlstm_fwd_f32 / tspgnn_lnlstm_gather_fwd_f32 */

int tspgnn_mlp_fwd_multi_f32(const tspgnn_mlp_task* tasks, int n_tasks, int d, void* stream);
/* The tasks whose K[dx + d, 4d] fits LDS (160 KiB with the LayerNorm parameters) share one launch; each of the others streams
 * its K through LDS in a launch of its own, which starts z at zero: TSPGNN_EUNSUPPORTED -- before any task is launched -- where
 * such a task is in gather-init or bias-init mode (tspgnn_plan_lstm_fwd_f32 answers the same). */
int tspgnn_lnlstm_fwd_multi_f32(const tspgnn_lstm_task* tasks, int n_tasks, int d, void* stream);

/*
 * The same two launches on the bf16 matrix cores with fp32-class accuracy ("bf16x3": every fp32 operand is
 * split exactly into three bf16 pieces, six piece products accumulate in fp32; dropped terms <= 2^-24
 * relative).  d in {32, 64}.  Weight operands are bf16x3 packings made by tspgnn_pack_weights_x3:
 *   mlp task:  wb = n_layers blocks of { packed[3*d*d] bf16, bias[d] float };  proj_w = packed [d,4d].
 *   lstm task: K  = packed [dx+d, 4d] (dx a multiple of 32; a kernel larger than LDS is streamed in k-block
 *              chunks with the workgroup in lock step);  every other field as in the _f32 functions.
 * tspgnn_pack_weights_x3: W:[krows,ncols] row-major fp32 (krows % 32 == 0, ncols % 16 == 0) ->
 *   P: 3*krows*ncols bf16 (2 bytes each), piece-major, each piece in MFMA fragment order.
 */
int tspgnn_pack_weights_x3(const float* W, void* P, int krows, int ncols, void* stream);
int tspgnn_mlp_fwd_multi_x3(const tspgnn_mlp_task* tasks, int n_tasks, int d, void* stream);
int tspgnn_lnlstm_fwd_multi_x3(const tspgnn_lstm_task* tasks, int n_tasks, int d, void* stream);

/*
 * Cell update fused with the message MLP that consumes the new h in the NEXT time step (graphnn.py:150-170 read
 * across the step boundary: msg(h') is the same value whether it is computed at the end of step t or at the start
 * of step t+1).  Per task: the cell exactly as in tspgnn_lnlstm_fwd_multi_x3, then, on the same rows,
 *   Y = Dense chain (mlp_layers <= 4 square layers, weights/bias blocks as in tspgnn_mlp_fwd_multi_x3) of h';
 *   mlp_out:[rows,d] = Y (optional);  proj_out:[rows,4d] = Y P (optional, P = pack_weights_x3 of [d,4d]).
 * mlp_layers == 0: plain cell.
 */
typedef struct tspgnn_cell_mlp_task {
    tspgnn_lstm_task cell;
    const void* mlp_wb; int mlp_layers; unsigned relu_mask; float* mlp_out;
    const void* proj_w; float* proj_out;
    /* _h2 entry points only (the others require 0): the states h, c are read / h_out, c_out are written BLOCKED by 16
     * rows -- float4 (columns 16t + 4g .. +3) of row r at (((r/16) * d/16 + t) * 4 + g) * 64 + (r%16) * 4, buffers of
     * ceil(rows/16)*16 rows -- instead of row-major.  A state that only this launch sequence reads (the T-step loop's
     * ping-pong buffers) is then loaded and stored 1 KiB contiguous per instruction instead of as 16-byte pieces of 16
     * different rows. */
    int state_in_blocked; int state_out_blocked;
    /* _h2 entry points only (the others require NULL): training forward -- the MLP's hidden activations (outputs of its
     * layers 0 .. mlp_layers-2, after the ReLU) are also stored, layer l of row r at mlp_acts[l*mlp_acts_stride + r*d],
     * exactly what tspgnn_mlp_task.acts receives from the plain MLP launch (the backward's tape). */
    float* mlp_acts; long long mlp_acts_stride;
} tspgnn_cell_mlp_task;
int tspgnn_lnlstm_mlp_fwd_multi_x3(const tspgnn_cell_mlp_task* tasks, int n_tasks, int d, void* stream);

/*
 * The same three launches on the fp16 matrix cores with fp32-class accuracy ("f16x2": every fp32 operand is split
 * into two fp16 pieces hi + lo = x to 2^-24 relative, three piece products accumulate in fp32; see
 * csrc/dense_h2.hip) -- half the matrix instructions and less than half the split arithmetic of bf16x3; the
 * default arithmetic of the inference forward.  d in {32, 64}.  Operands as for the _x3 functions, except:
 *   tspgnn_pack_weights_h2: W:[krows,ncols] -> P: 2*krows*ncols fp16, piece-major, the pieces of 2^s * W with
 *     s = TSPGNN_H2_WEIGHT_SCALE_LOG2 (keeps the lo piece of a typical weight out of the fp16 subnormals).
 *     RANGE: the hi piece is an fp16, so 2^s |W| must stay below 65504 (|W| < 1023.5) -- fp32, the reference's type
 *     (graphnn.py:18), has no such limit.  absmax_bits (optional device word, caller-zeroed): atomically raised to
 *     the IEEE bit pattern of max |2^s W| over the matrix (0x7f800000 or above: a non-finite entry).  A caller
 *     that gets >= the bits of 65504.0f (0x477fe000) must run that network on the _x3 / _f32 entry points, which
 *     have fp32's range.  Activations: an operand row of a GEMM (h, a message MLP's hidden activation, an aggregate)
 *     with an entry >= 65504 in magnitude overflows the same way; the kernels detect it where they split the operand
 *     and set bit 0 of the task's range_flag (then the launch's outputs are not to be used: re-run on _x3 / _f32);
 *     the LOW end: the lo piece of an operand below 2^-3 is an fp16 subnormal, so the split of a small value carries an
 *     ABSOLUTE error up to 2^-25 where fp32 carries a relative one -- immaterial next to a z of ordinary size, but
 *     LayerNorm divides by the row's spread.  The cell kernels therefore keep the smallest positive variance they
 *     normalise a gate row by and set bit 1 of range_flag when it is below (2^-5)^2 in units of the unscaled z (a row
 *     of exactly zero variance -- exact operands -- does not count): same consequence as bit 0;
 *   mlp task:  wb = n_layers blocks of { packed[2*d*d] fp16, 2^s * bias[d] float }; Y comes back unscaled;
 *              proj_out = the PROJECTED-MESSAGE FORMAT of this family: 2^s * (Y P), blocked by 16 source rows -- the
 *              float4 (columns 16t + 4g .. 4g+3) of row v at float offset (((v/16) * d/4 + t) * 4 + g) * 64 + (v%16) * 4;
 *              buffer of ceil(rows/16)*16 rows x 4d floats.  It only ever feeds the z of an f16x2 cell (Zx of
 *              gather-init mode): producer tiles store 1 KiB contiguous, and the edges' gathers find consecutive
 *              vertices in one 64-byte segment;
 *   lstm task: K packed [dx+d, 4d]; Zx in the projected-message format above; zbias unscaled; c may be NULL = the
 *     zero cell state (LSTM_initial_states' default at the first step of a run): nothing is read for it (the same in
 *     tspgnn_lstm_task_bf16).
 *     The cell normalises the scaled z with epsilon 2^2s * 1e-12, which reproduces the gates of the unscaled z
 *     bit for bit (power-of-two scaling commutes with rounding).
 */
#define TSPGNN_H2_WEIGHT_SCALE_LOG2 6
float tspgnn_h2_weight_scale(void);   /* 2^TSPGNN_H2_WEIGHT_SCALE_LOG2 */
int tspgnn_pack_weights_h2(const float* W, void* P, int krows, int ncols, unsigned* absmax_bits, void* stream);
/* Every square layer of an MLP in one launch, from the variables' own layout wb = n_layers blocks {W[d,d], b[d]} (mlp.py:57-63's
 * Dense layers as a flat parameter vector holds them): transposed == 0 -> out = n_layers blocks {tspgnn_pack_weights_h2(W_l)
 * [4 d d bytes], 2^s b_l [4 d bytes]} = tspgnn_mlp_task.wb of the _h2 entry points; transposed != 0 -> out = n_layers blocks
 * tspgnn_pack_weights_h2(W_l^T) [4 d d bytes] = tspgnn_mlp_bwd_task.wt.  absmax_bits as tspgnn_pack_weights_h2.  A training
 * step repacks after every optimiser step: one launch per MLP and direction instead of three per layer. */
int tspgnn_pack_mlp_h2(const float* wb, void* out, int d, int n_layers, int transposed, unsigned* absmax_bits, void* stream);
int tspgnn_mlp_fwd_multi_h2(const tspgnn_mlp_task* tasks, int n_tasks, int d, void* stream);
/* One task followed by a Dense(1) head on the rows in hand (the vote MLP of model.py:107-115,128: three relu layers and
 * a linear d -> 1): y[r] = <out row r, head_w[d]> + head_b[0] in fp32, where `out` is what tspgnn_mlp_fwd_multi_h2
 * would have written to task->Y.  task->Y may be NULL (the rows are then never written); task->proj_w must be NULL. */
int tspgnn_mlp_head_fwd_h2(const tspgnn_mlp_task* task, const float* head_w, const float* head_b, float* y, int d,
                           void* stream);
int tspgnn_lnlstm_fwd_multi_h2(const tspgnn_lstm_task* tasks, int n_tasks, int d, void* stream);
int tspgnn_lnlstm_mlp_fwd_multi_h2(const tspgnn_cell_mlp_task* tasks, int n_tasks, int d, void* stream);

/*
 * The WHOLE T-step loop of graphnn.py:175-179 (tf.while_loop over while_body, graphnn.py:142-173) as ONE launch, for the
 * wiring of model.py:53-104: two variables, the "edge" one updated from a two-ones-per-row matrix (rows of EV,
 * instance_loader.py:63-66) and the "vertex" one from its transpose.  Arithmetic, operand formats and summation orders
 * are those of tspgnn_lnlstm_mlp_fwd_multi_h2 + tspgnn_csr_rowsum_f32 launched T times (bit-identical results); what
 * changes is where the data lives and how steps are ordered:
 *   - one workgroup per compute unit, resident for all T steps; EV is block-diagonal by instance
 *     (instance_loader.py:56-66), so a step's dependences never leave a GROUP of consecutive instances: workgroups
 *     synchronise per group through device counters (arrivals of message tiles, of aggregated vertex rows, of projected
 *     vertex tiles) instead of per step through kernel boundaries, and run ahead where their inputs are ready;
 *   - the edge states h, c stay IN REGISTERS between the steps (a wavefront owns <= 4 tiles of 16 edge rows for the whole
 *     loop); per step an edge row only reads the projected messages of its two endpoints and writes its message row;
 *   - the V<-E row-sum of a group is shared by the wavefronts that produced its messages; the vertex cells run on a few
 *     workgroups of their own, one LDS residency for the cell kernel and one for the message MLP + projection per step.
 * All buffers are caller-owned device memory; `plan` (int32, built by the host from the batch's instance sizes, see
 * tspgnn/loop_plan.py) tells every wavefront its role, its tiles, its groups and the counts it waits for:
 * TSPGNN_LOOP_DESC_INTS ints per (workgroup, wavefront), grid * TSPGNN_LOOP_WAVES descriptors in all -- the layout is
 * documented where it is written (loop_plan._build) and read (mp_loop_h2.hip).  `counters` = 3 * 32 * n_groups unsigned
 * words + 32 (three counters per group, each split by step parity), ZEROED by the caller before every launch
 * (stream-ordered).  status (optional device word): |= 1 when a wait timed out (the
 * launch's outputs are then garbage; cannot happen unless fewer than `grid` workgroups are resident).
 * msg[0] / zx[0] hold the messages / projected messages of step 0 on entry (tspgnn_mlp_fwd_multi_h2).  T >= 1.
 */
#define TSPGNN_LOOP_WAVES 8
#define TSPGNN_LOOP_DESC_INTS 24
typedef struct tspgnn_mp_loop_args {
    /* edge variable: rows M, gather-init cell (Kh, projected messages of the two endpoints), message MLP */
    const float* e_h0; const float* e_c0;   /* [M,d] row-major initial states; e_c0 NULL = zeros */
    float* e_h; float* e_c;                 /* [M,d] final states */
    const int32_t* uv;                      /* [M,2] */
    const void* e_K; const float* e_ln;     /* tspgnn_pack_weights_h2(Kh[d,4d]); LayerNorm block [10d] */
    const void* e_mlp_wb; int e_mlp_layers; unsigned e_relu_mask;
    float* msg[2];                          /* [M,d] message rows, by step parity */
    /* vertex variable: rows N, cell over [row-sum of messages | h], message MLP, projection through the edge cell's Kx */
    const float* v_h0; const float* v_c0; float* v_h; float* v_c;
    const int32_t* rowptr; const int32_t* eid;   /* CSR of EV^T: [N+1], [2M] */
    const void* v_K; const float* v_ln;     /* tspgnn_pack_weights_h2(K[2d,4d]) */
    const float* v_zbias; const float* v_zscale;   /* optional, as tspgnn_lstm_task */
    const void* v_mlp_wb; int v_mlp_layers; unsigned v_relu_mask;
    const void* v_proj_w;                   /* tspgnn_pack_weights_h2(Kx[d,4d]) */
    float* zx[2];                           /* projected messages (blocked format), by step parity */
    float* vagg[2];                         /* [N,d] scratch: the row-sums, by step parity */
    const int32_t* plan; unsigned* counters; int n_groups; int grid;
    int M; int N; int T; int z_centered;
    unsigned* range_flag; unsigned* status;
    unsigned long long* trace;              /* optional (development): 16 words per (workgroup, wavefront), sums of
                                               s_memrealtime ticks per phase of the loop (tools/loop_trace.py) */
} tspgnn_mp_loop_args;
int tspgnn_mp_loop_h2(const tspgnn_mp_loop_args* args, int d, void* stream);

/*
 * The same loop (graphnn.py:175-179 over while_body, graphnn.py:142-173; wiring of model.py:53-104) as ONE launch of
 * resident workgroups with the edge states kept in MEMORY between the steps -- the form for batches whose edge tiles
 * outnumber what tspgnn_mp_loop_h2 holds in registers (BASELINE's n=40, batch=128 and beyond).  Arithmetic, operand
 * formats and summation orders are again those of tspgnn_lnlstm_mlp_fwd_multi_h2 + tspgnn_csr_rowsum_f32 launched T
 * times (bit-identical results).  Per compute unit one workgroup of TSPGNN_RESIDENT_WAVES wavefronts:
 *   - EDGE workgroups keep Kh and the message MLP in LDS for the whole loop and hand out WORK ITEMS -- 16-row edge tiles
 *     and shares of the V<-E row-sum -- through one LDS ticket that runs through all T steps: item k is item k mod W of
 *     step k div W.  A tile's states live in private slot arrays (`e_hs`, `e_cs`: [slots * 16, d], blocked by tile,
 *     updated in place, write-through stores and L1-bypassing loads: they never leave the Infinity Cache at C2 sizes);
 *     a tile of step t waits for its own step t-1 (an LDS word per tile) and for its group's projected messages;
 *   - the items of a step are ordered by CLASS (the groups of an XCD are cut into classes, tspgnn/resident_plan.py): while
 *     the vertex chain of one class runs -- row-sum, vertex cells, message MLP, projection: ~25 us that nothing else of
 *     that class can overlap -- the workgroup's wavefronts work on the tiles of the other class;
 *   - VERTEX workgroups come in two kinds, neither with a barrier or a second LDS residency inside the loop: CELL workgroups
 *     (K[2d,4d] resident) and MESSAGE workgroups (message MLP + projection resident); h' crosses between them through `vh`.
 * Synchronisation is per group of consecutive instances through the three parity-split counters of tspgnn_mp_loop_h2
 * (message tiles arrived, vertex rows aggregated, vertex tiles projected) and a fourth (vertex tiles updated): the
 * ordering argument is the same.  `counters` = 4 * 32 * n_groups + 32 words here (the last 32: the placement check).
 * The kernel's one dependence on WHERE workgroups run -- an L1-only invalidate before re-gathering projected messages, valid
 * when a group's producers and consumers share an XCD's L2 -- is verified inside the launch and replaced by an agent-scope
 * acquire when it does not hold.
 * `plan`: int32 -- grid headers of TSPGNN_RESIDENT_HDR_INTS, then items of TSPGNN_RESIDENT_ITEM_INTS (layout documented in
 * tspgnn/resident_plan.py and csrc/mp_resident_h2.hip).  `counters` as for tspgnn_mp_loop_h2, zeroed by the caller before
 * every launch.  `lds_words`: LDS words the plan's largest edge workgroup needs behind the weights (one per tile, and
 * TSPGNN_RESIDENT_SHARE_ROWS * (1 + TSPGNN_RESIDENT_SHARE_CAP / 2) per row-sum share whose edge lists it keeps there)).
 */
#define TSPGNN_RESIDENT_WAVES 12
#define TSPGNN_RESIDENT_HDR_INTS 8
#define TSPGNN_RESIDENT_ITEM_INTS 8
#define TSPGNN_RESIDENT_SHARE_ROWS 8   /* vertex rows per row-sum share */
#define TSPGNN_RESIDENT_SHARE_CAP 48   /* edge ids (16-bit offsets from the group's first edge) per vertex row of a share kept in LDS */
typedef struct tspgnn_mp_resident_args {
    const float* e_h0; const float* e_c0;   /* [M,d] row-major initial states; e_c0 NULL = zeros */
    float* e_h; float* e_c;                 /* [M,d] final states */
    float* e_hs; float* e_cs;               /* [n_slots*16, d] scratch: the states between the steps, by tile slot */
    const int32_t* uv;
    const void* e_K; const float* e_ln;
    const void* e_mlp_wb; int e_mlp_layers; unsigned e_relu_mask;
    float* msg[2];
    const float* v_h0; const float* v_c0; float* v_h; float* v_c;
    const int32_t* rowptr; const int32_t* eid;
    const void* v_K; const float* v_ln;
    const float* v_zbias; const float* v_zscale;
    const void* v_mlp_wb; int v_mlp_layers; unsigned v_relu_mask;
    const void* v_proj_w;
    float* zx[2];
    float* vagg[2];
    float* vh[2];                           /* [N,d] scratch: the vertex states h between the steps, by step parity */
    const int32_t* plan; unsigned* counters; int n_groups; int grid; int n_slots; int lds_words;
    int n_active;                           /* workgroups of the plan with work (edge + cell + message) */
    int flags;                              /* bit 0: take the placement-independent acquire (tests; see PLACEMENT in the kernel) */
    int M; int N; int T; int z_centered;
    unsigned* range_flag; unsigned* status;
    unsigned long long* trace;              /* optional (development), as tspgnn_mp_loop_args */
} tspgnn_mp_resident_args;
int tspgnn_mp_resident_h2(const tspgnn_mp_resident_args* args, int d, void* stream);

/* ------------------------------------------------------------------ bf16 storage, fp32 accumulate
 *
 * BASELINE config 5 ("bf16 embeddings with fp32 accumulate"): the same forward operators with
 * the embeddings h, the messages, the aggregates and the projected messages Zx stored as bf16 (void* = bf16
 * rows, row-major, 16-byte aligned), GEMMs as bf16 MFMA products accumulated in fp32, and the cell state c, the
 * LayerNorm statistics / parameters, the biases and the gate arithmetic in fp32.  Weight operands are the fp32
 * variables rounded to bf16: piece 0 (the first krows*ncols bf16) of tspgnn_pack_weights_x3.
 *   tspgnn_gather2_sum_bf16 / tspgnn_csr_rowsum_bf16: tf.matmul(EV, y [, adjoint_a]) (graphnn.py:156-160), sums in
 *     fp32, one rounding at the store; d % 8 == 0 (gather), d in {32..512} (row-sum).
 *   mlp task:  wb = n_layers blocks of { bf16 packed[d*d], float bias[d] }, hidden activations rounded to bf16
 *     between layers (what a stored embedding would be); proj_w = bf16 packed [d,4d], proj_out = the bf16 projected
 *     messages Zx in the blocked format of the f16x2 family (unscaled): [rows padded to 16, 4d] bf16, the four
 *     values (cols 16t+4g..+3) of row v at element (((v/16)*(4d/16) + t)*4 + g)*64 + (v%16)*4.
 *   lstm task: x, h, h_out bf16 row-major, Zx in the blocked format above; c, c_out, ln fp32; K = bf16 packed
 *     kernel[dx+d,4d] (Kh[d,4d] in gather-init mode, uv != NULL); a kernel larger than LDS is streamed in k-block
 *     chunks.  d in {32, 64, 128}.  state_in_blocked / state_out_blocked: h and c / h_out and c_out are stored
 *     [rows padded to 16, d] blocked by 16 rows (element (((r/16)*(d/16) + t)*4 + g)*64 + (r%16)*4 for cols
 *     16t+4g..+3) instead of row-major -- for the ping-pong state buffers inside a T-step loop, which only this
 *     kernel and the message MLP (mlp task: x_blocked) read.
 */
int tspgnn_gather2_sum_bf16(const int32_t* ev_uv, const void* X, void* Y, int M, int N, int d, void* stream);
int tspgnn_csr_rowsum_bf16(const int32_t* rowptr, const int32_t* eid, const void* X, void* Y, int N, int M, int d,
                           void* stream);
typedef struct tspgnn_mlp_task_bf16 {
    const void* X; const void* wb; void* Y; int rows; int n_layers; unsigned relu_mask;
    const void* proj_w; void* proj_out;
    void* acts; long long acts_stride;   /* optional (training): the stored (bf16) hidden activations, layer l of row r
                                            at acts[l*acts_stride + r*d] (elements); stride 0 = rows*d */
    int x_blocked;                       /* X is a loop state h stored blocked by 16 rows (see the lstm task) */
    int y_interleaved;                   /* the LAST layer's packed weights and bias have their output columns permuted --
                                            packed column 16t + 4g + j (t < d/16, g, j < 4) holds true column
                                            32(t/2) + 8g + 4(t%2) + j -- so that a lane's eight results of a tile pair are
                                            eight CONSECUTIVE columns of Y: one 16-byte store, 64-byte runs per row and
                                            instruction, instead of two 8-byte stores in 32-byte runs.  Y itself is the
                                            ordinary row-major [rows, d].  Not with a projection or saved activations. */
} tspgnn_mlp_task_bf16;
typedef struct tspgnn_lstm_task_bf16 {
    const void* x; int dx; const void* h; const float* c; const void* K; const float* ln;
    void* h_out; float* c_out; int rows;
    const int32_t* uv; const void* Zx;
    int state_in_blocked; int state_out_blocked;
} tspgnn_lstm_task_bf16;
int tspgnn_mlp_fwd_multi_bf16(const tspgnn_mlp_task_bf16* tasks, int n_tasks, int d, void* stream);
int tspgnn_lnlstm_fwd_multi_bf16(const tspgnn_lstm_task_bf16* tasks, int n_tasks, int d, void* stream);

/* ------------------------------------------------------------------ pre / post loop */

/*
 * E0 = E_init_MLP(concat([W, C], 1)): Dense 2 -> d/8 -> d/4 -> d/2 -> d, relu x3 + linear
 * (model.py:33-43).  WC:[M,2] = (edge weight, target cost) per edge, E0:[M,d].
 * wb: the four layers back to back, each W[in,out] then b[out].
 */
int tspgnn_einit_fwd_f32(const float* WC, const float* wb, float* E0, int M, int d, void* stream);

/* Y[r,:] = v[:] for r in [0,rows): tf.tile(V_init/sqrt(d), [N,1]) (model.py:48-51), with
 * scale applied: Y = scale * v. */
int tspgnn_tile_rows_f32(const float* v, float scale, float* Y, int rows, int d, void* stream);

/* y[r] = dot(X[r,:], w) + b[0]: the final Dense(1) of E_vote (model.py:107-115,128).
 * b is a device pointer to one float. */
int tspgnn_rowdot_f32(const float* X, const float* w, const float* b, float* y,
                      int rows, int d, void* stream);

/*
 * logits[p] = mean(vote[seg[p]:seg[p+1]]) (model.py:134-145);  seg:[B+1] exclusive prefix
 * sums of n_edges.  An empty segment yields NaN like tf.reduce_mean of an empty slice.
 */
int tspgnn_segment_mean_f32(const float* vote, const int32_t* seg, float* logits,
                            int B, void* stream);

/*
 * predictions = sigmoid(logits); loss = mean(sigmoid_cross_entropy_with_logits);
 * TP/FP/TN/FN/acc with tf.round (half-to-even), formulas verbatim from model.py:147-157.
 * pred:[B]   stats:[6] = loss, acc, TP, FP, TN, FN.
 */
int tspgnn_bce_metrics_f32(const float* logits, const float* labels, float* pred, float* stats,
                           int B, void* stream);

/*
 * One bracket update of the tour-cost binary search for n_inst instances at once (get_cost's loop,
 * experiments/binary_search.py:53-75).  Instance i owns the k graphs g = i*k + j of the batch; seg:[n_inst*k+1] is the
 * batch's edge offsets.  State: lo, hi:[n_inst] fp64 bracket, iters:[n_inst], pred_out:[n_inst] (the prediction
 * get_cost would return).  An instance is active while lo < w*(1-stopping_delta) || w*(1+stopping_delta) < hi,
 * w = (hi+lo)/2, evaluated in fp64 as Python does.
 *   mode 0 (init): writes the first probes of every active instance; reads no predictions (pred may be NULL).
 *   mode 1 (step): every active instance reads its k predictions pred:[n_inst*k] and applies get_cost's k == 1 rule
 *                  (p < threshold moves lo, anything else -- NaN included -- moves hi) or its k > 1 rule (probes
 *                  lo + (hi-lo)*((j+1)/(k+1.0)), bracket around the first p >= threshold, pred_out = preds[min(first,
 *                  k-1)]); iters += 1; then writes its next probes.  Inactive instances are never touched.
 * Probe write: WC[e*2+1] = (float)probe (round to nearest) for every edge e of every active graph; column 0 is never
 * written.  The threshold is compared in fp32, as NumPy compares a float32 prediction with a Python float.
 * n_active:[1] = number of instances active after the launch (zeroed on `stream` first, so a captured round recounts).
 * guard: the f16x2 range guard word (VariableStore.h2_guard): if guard[0] & 3 or guard[2] is set, the launch changes
 * no state and no probe (it still counts the active instances).  Bit-identical to the host loop for the same
 * predictions.  n_inst == 0 is a no-op.
 */
int tspgnn_cost_search_step(double* lo, double* hi, int* iters, float* pred_out, int* n_active, const float* pred,
                            float* WC, const int32_t* seg, const int* guard, int n_inst, int k, double threshold,
                            double stopping_delta, int mode, void* stream);

/* ------------------------------------------------------------------ tour labelling (dataset.py:9-50, Concorde's role) */

/*
 * Batched multi-start iterated local search for symmetric TSP instances (tspgnn/dataset.py solve_tours).  Instance i has
 * n[i] vertices (4 <= n[i] <= n_max <= 128) and a dense fp32 weight matrix W + w_off[i] of n[i] x n[i] (row-major,
 * symmetric; absent edges carry a penalty weight chosen by the caller).  One workgroup per instance holds the matrix in
 * LDS; each of its `restarts` (1..16) wave64 chains runs a best-improvement descent (2-opt, and Or-opt moves of 1-3
 * vertices in either orientation; a move must gain more than 1e-6 * cost / n; at most 4 n^2 moves per descent), then
 * `kicks` double-bridge kicks, each followed by a descent and accepted when no worse.  Chain 0 starts from
 * init_tours + t_off[i] when init_tours is not NULL and that tour is a permutation of 0..n[i]-1; every other start is a
 * random permutation.  Randomness is keyed on (seed, index[i], chain, kick) only -- index[i] is the instance's position
 * in the caller's list (index == NULL: i) -- so a result does not depend on how the caller splits its batch into launches.
 * Out: tours + t_off[i] (n[i] int32) = the best chain's tour in canonical form (tour[0] = 0, tour[1] < tour[n-1]);
 * costs[i] = its fp32 cost under W.  n_inst == 0 is a no-op; n_max > 128: TSPGNN_EUNSUPPORTED.
 */
int tspgnn_tour_search(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                       const long long* t_off, const long long* index, int n_inst, int n_max, int restarts, int kicks,
                       unsigned long long seed, int32_t* tours, float* costs, void* stream);

/*
 * Held-Karp 1-tree lower bound by subgradient ascent, one wave64 per instance, same W / w_off / n layout as
 * tspgnn_tour_search.  Each of at most `iters` steps builds the minimum 1-tree under W[u][v] + pi_u + pi_v (Prim on
 * vertices 1..n-1, plus the two cheapest edges at vertex 0) and moves pi along (degree - 2) with the Polyak step
 * lambda * (upper[i] - L) / |g|^2, lambda = 2 halved after 8 steps without a new best.  The best multipliers' 1-tree is
 * rebuilt in fp64 and lb[i] = its value less 8 n DBL_EPSILON times the sum of its terms' magnitudes: a lower bound on
 * every tour's cost under W, rounding included.
 */
int tspgnn_tour_lower_bound(const float* W, const long long* w_off, const int* n, const float* upper, int n_inst,
                            int n_max, int iters, double* lb, void* stream);

/*
 * tspgnn_tour_search for instances of up to 256 vertices (dataset.py:9-50): the same search, moves, kicks, keys and
 * canonical output, on the packed strict upper triangle.  W + w_off[i] holds n[i] (n[i] - 1) / 2 fp32 values, row-major:
 * w(a, b) for a < b sits at a (2 n - 3 - a) / 2 - 1 + b.  4 <= n[i] <= n_max <= 256; n_max > 256: TSPGNN_EUNSUPPORTED.
 * The LDS of every chain kernel (the searches, tspgnn_tour_nearest_neighbor, tspgnn_tour_anneal; csrc/tour_common.h,
 * ChainLds): the weights (4 n_max (n_max | 1) bytes dense, 2 n_max (n_max - 1) packed), per chain three tours of n_max
 * int32 ids, and for a search with a table of K columns (_knn: neighbors, _cand: columns) n_max K bytes of table and
 * n_max more bytes per chain -- weights + K n_max + chains (12 + [K > 0]) n_max bytes, which must fit 163 712 (160 KiB
 * less 128 static).  The dense layout always holds all 16 chains; the triangle holds 16 up to n_max = 242 and 10 at
 * n_max = 256 (9 with K = 8).  tspgnn_tour_chains_fit gives the limit; a larger restarts is TSPGNN_EINVAL, and the message
 * names the limit.  For n <= 128 the tours and costs equal tspgnn_tour_search's bit for bit, given the same seed, index,
 * restarts and kicks.
 */
int tspgnn_tour_search_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                           const long long* t_off, const long long* index, int n_inst, int n_max, int restarts, int kicks,
                           unsigned long long seed, int32_t* tours, float* costs, void* stream);

/*
 * tspgnn_tour_search with a candidate-list descent (dataset.py:9-50): same starts, kicks, keys, acceptance and canonical
 * output, but a descent step looks only at the moves that add an edge between near neighbours.  With kk = min(neighbors,
 * n[i] - 1), N(x) = the kk vertices y != x smallest by (W[x][y], y) and S = the pairs {x, y} with y in N(x) or x in N(y).
 * The moves, their fp32 deltas and their order are tspgnn_tour_search's, the two orientations of an Or-opt move counted
 * as two moves.  A 2-opt move (reverse positions i+1..j) is a candidate iff {t[i], t[j]} or {t[i+1], t[j+1]} is in S; an
 * Or-opt move (segment s0..sl between a and b) iff {a, s0} or {sl, b} is (reversed: {a, sl} or {s0, b}); the edge that
 * closes the gap the segment leaves does not count.  A step applies the best candidate when it gains more than
 * 1e-6 * cost / n.  The result is defined by that set, not by an enumeration order.  neighbors in 1..32, else
 * TSPGNN_EINVAL before any launch; neighbors >= n[i] - 1 gives tspgnn_tour_search's tours and costs bit for bit.  LDS holds
 * n_max * neighbors bytes of neighbour table and n_max more bytes per chain; at n_max <= 128 all 16 chains still fit.
 * n_inst == 0 is a no-op; n_max > 128: TSPGNN_EUNSUPPORTED.
 */
int tspgnn_tour_search_knn(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                           const long long* t_off, const long long* index, int n_inst, int n_max, int restarts, int kicks,
                           int neighbors, unsigned long long seed, int32_t* tours, float* costs, void* stream);

/*
 * tspgnn_tour_search_knn on the packed strict upper triangle of tspgnn_tour_search_tri, n_max <= 256 (above:
 * TSPGNN_EUNSUPPORTED) (dataset.py:9-50).  restarts <= tspgnn_tour_chains_fit(1, n_max, neighbors) (the LDS layout:
 * tspgnn_tour_search_tri); a larger restarts is TSPGNN_EINVAL, and the message names the limit.  For n <= 128 the tours
 * and costs equal tspgnn_tour_search_knn's bit for bit.
 */
int tspgnn_tour_search_knn_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                               const long long* t_off, const long long* index, int n_inst, int n_max, int restarts,
                               int kicks, int neighbors, unsigned long long seed, int32_t* tours, float* costs,
                               void* stream);

/*
 * tspgnn_tour_search_knn with the candidate table handed in by the caller instead of built from the weights: the same
 * starts, kicks, random keys, moves, fp32 deltas, codes, candidate rule, threshold, move cap, acceptance and canonical
 * output; only S differs.  cand + c_off[i] holds instance i's table, n[i] x columns bytes, row-major, on the device.
 * Entry (x, s) = y puts the pair {x, y} into S iff y < n[i] and y != x; any other entry contributes nothing (x itself is
 * the conventional "skip").  Duplicate entries, asymmetric rows and an empty S are all legal: the result is a function of
 * the set S.  With an empty S every descent stops at once, and a chain keeps the cheapest of its start and kicked tours.
 * With the table N(x) of tspgnn_tour_search_knn (the neighbors nearest by (W[x][y], y), rows padded with x) the tours and
 * costs equal tspgnn_tour_search_knn's bit for bit.  Any candidate rule -- the network's edge votes
 * (tspgnn_vote_neighbors), alpha-nearness, quadrant neighbours, a union of rules -- is thus a table, with no new kernel.
 * LDS and chain limits are tspgnn_tour_search_knn's with neighbors = columns.  columns outside [1, 32], restarts above what
 * fits (the message names the limit) or a null cand / c_off: TSPGNN_EINVAL; n_max > 128: TSPGNN_EUNSUPPORTED; all before
 * any launch, the outputs untouched.  n_inst == 0 is a no-op.
 */
int tspgnn_tour_search_cand(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                            const long long* t_off, const long long* index, const uint8_t* cand, const long long* c_off,
                            int n_inst, int n_max, int restarts, int kicks, int columns, unsigned long long seed,
                            int32_t* tours, float* costs, void* stream);

/*
 * tspgnn_tour_search_cand on the packed strict upper triangle of tspgnn_tour_search_tri, n_max <= 256 (above:
 * TSPGNN_EUNSUPPORTED).  restarts <= tspgnn_tour_chains_fit(1, n_max, columns), as for tspgnn_tour_search_knn_tri.  For
 * n <= 128 the tours and costs equal tspgnn_tour_search_cand's bit for bit.
 */
int tspgnn_tour_search_cand_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                const long long* t_off, const long long* index, const uint8_t* cand,
                                const long long* c_off, int n_inst, int n_max, int restarts, int kicks, int columns,
                                unsigned long long seed, int32_t* tours, float* costs, void* stream);

/*
 * tspgnn_tour_lower_bound on the packed triangle of tspgnn_tour_search_tri (dataset.py:9-50): the same subgradient
 * ascent, fp64 re-evaluation and margin; a lane owns the vertices l, l+64, l+128 and l+192.  n_max <= 256
 * (above: TSPGNN_EUNSUPPORTED).  For n <= 128, lb[i] equals tspgnn_tour_lower_bound's bit for bit.
 */
int tspgnn_tour_lower_bound_tri(const float* W, const long long* w_off, const int* n, const float* upper, int n_inst,
                                int n_max, int iters, double* lb, void* stream);

/* ------------------------------------------------------------------ exact tour labels (dataset.py:9-50, Concorde's role) */

#define TSPGNN_BB_PROVED 0   /* the search finished: no tour is cheaper than the one returned, up to opt_tol */
#define TSPGNN_BB_BUDGET 1   /* max_nodes or the depth limit left nodes open: lb is valid, the tour is the best found */
#define TSPGNN_BB_BAD 2      /* n[i] outside [4, n_max], or the incumbent is no permutation: lb = NaN, tour untouched */
#define TSPGNN_BB_MAX_DEPTH 128   /* stack levels of the depth-first search (sizes the workspace) */

/*
 * Depth-first branch and bound on the Held-Karp 1-tree bound (tspgnn/dataset.py prove_tours): what Concorde does for the
 * reference's labels (dataset.py:9-50).  One wave64 per instance; W / w_off / n / t_off as tspgnn_tour_search (dense
 * matrices, 4 <= n[i] <= n_max <= 128; n_max > 128: TSPGNN_EUNSUPPORTED).  The workgroup keeps the weights and an int8
 * edge-class matrix (free / forced / forbidden) in LDS.
 * In/out: tours + t_off[i] holds an incumbent tour on entry and the best tour found on exit, in canonical form.
 * upper: NULL, or float[n_inst], the fp32 cost that steers the root's Polyak step; NULL takes the incumbent's cost.
 * Out: lb[i], a lower bound on every tour's cost under W, rounding included; nodes[i], the nodes whose ascent ran;
 * status[i], TSPGNN_BB_*.  workspace: tspgnn_tour_branch_bound_ws(n_inst, n_max) bytes on the device, the stack's
 * multipliers (n_max floats per level and instance; the decisions and bounds of the levels sit in LDS).
 * Root: tspgnn_tour_lower_bound's ascent (pi = 0, lambda = 2, root_iters steps) and fp64 rebuild; with max_nodes = 1 and
 * the same upper, lb[i] equals that kernel's bit for bit.  With inc = the incumbent's fp64 cost under the fp32 weights,
 * summed in tour order, a node is:
 *   infeasible  when a vertex has more than two forced edges or fewer than two edges that are not forbidden (a vertex
 *               with two forced edges forbids its others first), or when the allowed edges hold no 1-tree;
 *   bounded     by node_iters fp32 ascent steps from its parent's best multipliers (lambda = 2 again), the best
 *               multipliers' 1-tree rebuilt in fp64 less 8 n DBL_EPSILON times its magnitude, and not below the parent's
 *               bound: Lr.  The constrained 1-tree picks by (class, cost), a forced edge before any free one, a forbidden
 *               one never; its value is summed from the true W + pi_u + pi_v;
 *   pruned      when Lr >= inc (1 - opt_tol);
 *   a tour      when all fp64 1-tree degrees are 2: it becomes the incumbent when its cost is below inc;
 *   branched    otherwise, at the vertex v of largest degree (ties: smaller id) on its free tree edges e1, e2 of smallest
 *               and second smallest W(v, .) (ties: smaller id).  No forced edge at v: children force e1 and e2 / force
 *               e1, forbid e2 / forbid e1, visited in this order; one forced edge at v: force e1 / forbid e1.
 * A node that would be branched after max_nodes ascents or at depth TSPGNN_BB_MAX_DEPTH stays open, as does a node whose
 * children were not all visited; each counts with its own Lr.  lb[i] = min(inc, Lr of every pruned, tour and open
 * node): valid whether or not the search finished.  status[i] = TSPGNN_BB_PROVED exactly when nothing stayed open.
 * 1 <= max_nodes <= 65 536, node_iters >= 1, root_iters >= 1, opt_tol finite and >= 0 (relative), else TSPGNN_EINVAL
 * before any launch; n_inst == 0 is a no-op.  At most max_nodes * (node_iters + 1) + root_iters 1-trees per instance.
 */
int tspgnn_tour_branch_bound(const float* W, const long long* w_off, const int* n, const long long* t_off,
                             const float* upper, int n_inst, int n_max, int root_iters, int node_iters, int max_nodes,
                             double opt_tol, void* workspace, int32_t* tours, double* lb, int32_t* nodes, int32_t* status,
                             void* stream);

/* Bytes of workspace tspgnn_tour_branch_bound needs for n_inst instances at n_max (dataset.py:9-50): n_inst *
 * TSPGNN_BB_MAX_DEPTH * n_max floats; 0 for an empty or unsupported request. */
long long tspgnn_tour_branch_bound_ws(int n_inst, int n_max);

/* The chains (restarts of the searches, chains of tspgnn_tour_anneal, waves of tspgnn_tour_nearest_neighbor's every-start
 * run) that fit in LDS at n_max, 16 at the most: tri != 0 the packed triangle (n_max <= 256), else the dense matrix
 * (n_max <= 128); neighbors = 0 the full scan, 1..32 the columns of the _knn / _cand table.  0 for an n_max outside
 * [4, the layout's limit] or neighbors outside [0, 32].  Host only: touches no device.  The layout behind it is stated
 * at tspgnn_tour_search_tri. */
long long tspgnn_tour_chains_fit(int tri, int n_max, int neighbors);

/*
 * Metric closure of `count` weight matrices, in place: batched Floyd-Warshall in fp64, one workgroup per instance.
 * Replaces the networkx closure of the reference's 'random' distances (dataset.py:85-101).  Instance b is a row-major
 * fp64 n[b] x n[b] matrix at D + off[b] (off in doubles, in any order, gaps allowed; nothing outside the matrices is
 * written); 1 <= n[b] <= n_max <= 256.  Entries are finite and >= 0; the matrix need not be symmetric.
 * The result is exactly this process: the diagonal is set to 0; for k = 0 .. n-1 in ascending order
 * D[i][j] = min(D[i][j], D[i][k] + D[k][j]), the sum rounded once in fp64; the diagonal is set to 0.  It depends on the
 * instance alone, never on n_max, on the other instances or on the launch.
 * n_max <= 143 (8 n_max^2 bytes fit the 160 KiB of LDS): the matrix is closed in LDS; above, in place in global memory.
 * n_max > 256, n_max < 1, count < 0 or a null pointer with count > 0: TSPGNN_EINVAL before any launch.  count == 0 is a
 * no-op.
 */
int tspgnn_metric_closure(double* D, const long long* off, const int* n, int count, int n_max, void* stream);

/* ------------------------------------------------------------------ decision-TSP baselines (tspgnn/baselines.py) */

/*
 * Nearest-neighbour tours, one workgroup per instance, W / w_off / n / t_off as tspgnn_tour_search (dense matrices,
 * 4 <= n[i] <= n_max <= 128; n_max > 128: TSPGNN_EUNSUPPORTED).  From the start vertex the tour moves repeatedly to the
 * unvisited vertex v of smallest W(cur, v), ties to the smaller vertex id.  start >= 0: the one tour from vertex
 * start % n[i].  start == -1: the tour from every start vertex, the waves of the workgroup striding over the starts, and
 * of those the tour of smallest fp32 cost, ties to the smaller start.  start < -1: TSPGNN_EINVAL.
 * Out: tours + t_off[i] in canonical form (tour[0] = 0, tour[1] < tour[n-1]); costs[i] = its fp32 cost under W.
 * n_inst == 0 is a no-op.
 */
int tspgnn_tour_nearest_neighbor(const float* W, const long long* w_off, const int* n, const long long* t_off, int n_inst,
                                 int n_max, int start, int32_t* tours, float* costs, void* stream);

/*
 * tspgnn_tour_nearest_neighbor on the packed strict upper triangle of tspgnn_tour_search_tri, n_max <= 256 (above:
 * TSPGNN_EUNSUPPORTED).  For n <= 128 the tours and costs equal tspgnn_tour_nearest_neighbor's bit for bit.
 */
int tspgnn_tour_nearest_neighbor_tri(const float* W, const long long* w_off, const int* n, const long long* t_off,
                                     int n_inst, int n_max, int start, int32_t* tours, float* costs, void* stream);

/*
 * Metropolis annealing over 2-exchange moves: one workgroup per instance, one wave64 per chain, `chains` in [1, 16] and
 * at most what fits in LDS beside the weights (the rule of tspgnn_tour_search's restarts; TSPGNN_EINVAL names the limit).
 * W / w_off / n / init_tours / t_off / index as tspgnn_tour_search.  inv_temp:[n_inst, levels] fp32 on the device holds
 * 1 / T per level (+inf: T = 0); per_level:[n_inst] int on the device; levels >= 0.  Instance i runs
 * levels * per_level[i] proposals per chain, which must be at most 2^31 - 1: the arrays live on the device, so this entry
 * point cannot see them, and an instance that breaks the rule (or has per_level[i] < 0) gets costs[i] = NaN and no tour.
 * Chain 0 starts from init_tours + t_off[i] when that is given and a permutation, otherwise from the nearest-neighbour
 * tour from vertex 0; chain c > 0 from the nearest-neighbour tour from vertex c % n[i].
 * A chain is this sequential process over proposal numbers p = 0, 1, ...:
 *   r = the generator's draw for (seed, index[i], chain, p, 0);  i = (r & 0xffff) % n, j = ((r >> 16) & 0xffff) % n,
 *   swapped if i > j;  u = (((r >> 40) & 0x7fffff) + 0.5) * 2^-23;
 *   the proposal is void (a rejection) unless j > i + 1 and not (i == 0 and j == n - 1);
 *   d = (W(a,c) + W(b,e)) - (W(a,b) + W(c,e)) in fp32, a = t[i], b = t[i+1], c = t[j], e = t[(j+1) % n];
 *   accepted iff d <= 0 or u < expf(-(d * inv_temp[i][p / per_level[i]]));  acceptance reverses positions i+1..j;
 *   rel, the fp32 running sum of the accepted d, starts at 0, and the tour is kept as the chain's best whenever rel falls
 *   below its smallest value so far.
 * The wave evaluates 64 consecutive proposals against the current tour at once and applies the first that accepts, which
 * is the same process.  Out: of the chains' best tours the one of smallest fp32 cost (recomputed from the tour), ties to
 * the lower chain, in canonical form; costs[i] = that cost.  Results depend on (seed, index[i], chains, the schedule)
 * only.  n_inst == 0 is a no-op; n_max > 128: TSPGNN_EUNSUPPORTED.
 */
int tspgnn_tour_anneal(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                       const long long* t_off, const long long* index, const float* inv_temp, const int* per_level,
                       int n_inst, int n_max, int chains, int levels, unsigned long long seed, int32_t* tours,
                       float* costs, void* stream);

/*
 * tspgnn_tour_anneal on the packed strict upper triangle of tspgnn_tour_search_tri, n_max <= 256 (above:
 * TSPGNN_EUNSUPPORTED); at n_max = 256 chains <= 10.  For n <= 128 the tours and costs equal tspgnn_tour_anneal's bit
 * for bit.
 */
int tspgnn_tour_anneal_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                           const long long* t_off, const long long* index, const float* inv_temp, const int* per_level,
                           int n_inst, int n_max, int chains, int levels, unsigned long long seed, int32_t* tours,
                           float* costs, void* stream);

/* ------------------------------------------------------------------ tours from the edge votes (tspgnn/decode.py) */

/*
 * tspgnn_tour_from_votes, tspgnn_tour_beam and tspgnn_vote_neighbors read the network's per-edge logits (E_vote,
 * model.py:106-128) of a batch as Session.prepare / DeviceDataset.batch leave it on the device, one workgroup per
 * instance.  What the three have in common is stated here once:
 *   Batch.  vote:[M] fp32; uv:[M][2] the global endpoint ids; wc:[M][2], column 0 the edge weight; seg:[B+1] the edge
 *           prefix sums; vseg:[B+1] the vertex prefix sums.  Instance b has n = vseg[b+1] - vseg[b] vertices and the edges
 *           e = 0 .. m-1 of seg[b] .. seg[b+1], endpoints in local ids uv - vseg[b].  4 <= n <= n_max <= 256.
 *   Pairs.  An edge joins its local endpoints a and b only when both lie in [0, n) and a != b; any other edge joins
 *           nothing.  For an unordered pair {a, b}: e(a,b) is the smallest edge id joining it, or none, and
 *           w(a,b) = wc[e(a,b)][0].
 *   Key.    The order-preserving uint32 image of an fp32 value: all bits flipped when the sign bit is set, else the sign
 *           bit set, so -0.0 < +0.0 and -inf is the lowest number.  The vote key gives a NaN the image 0, below
 *           everything; the ascending key of costs and weights gives it 0xffffffff, after every number.
 *   Tour.   tours + vseg[b]: the cyclic sequence in canonical form (tour[0] = 0, tour[1] < tour[n-1]), local ids.
 *           n_missing[b]: the cyclically consecutive pairs that no edge joins (0: a feasible tour).  costs[b]: one running
 *           fp32 sum from 0 in canonical tour order, the closing pair last, of w over the pairs that are edges; additions
 *           only, no FMA.
 *   Checks. B == 0 is a no-op; n_max > 256: TSPGNN_EUNSUPPORTED; B < 0, n_max < 4 or a null pointer with B > 0:
 *           TSPGNN_EINVAL; all before any launch, the outputs untouched.  The arrays live on the device, so an entry point
 *           cannot see them: what an instance with n outside [4, n_max] gets is said with each.
 * A result depends on the instance and its votes (and the arguments named) alone: never on n_max, on the other instances
 * or on the launch.  No kernel communicates between workgroups.
 */

/*
 * A tour per instance from the votes by greedy edge insertion.  The result is exactly this sequential process:
 *   Order.   Edge e precedes edge f iff its vote key is larger, or the keys are equal and e < f.
 *   Greedy.  Every vertex starts with degree 0 in a component of its own.  Until no edge is eligible: take the first
 *            eligible edge in the order above, add it, raise both degrees, merge the components.  Eligible: the edge joins
 *            its endpoints (Pairs), both have degree < 2 and they lie in different components.  Eligibility only shrinks,
 *            so this equals one pass over the sorted list; the kernel takes a workgroup-wide arg-max over (key, edge id)
 *            per round and sorts nothing.
 *   Stitch.  The chosen edges form vertex-disjoint paths, an untouched vertex being a path of one.  Each path starts at
 *            its endpoint of smaller id; the paths are ordered by their smallest vertex id and concatenated.
 *   Output.  tours, n_missing and costs as under Tour.
 * An instance with m == 0 gets the identity tour, n_missing = n and cost 0; one with n outside [4, 256] gets
 * costs[b] = NaN, n_missing[b] = -1 and no tour.
 */
int tspgnn_tour_from_votes(const float* vote, const int32_t* uv, const float* wc, const int32_t* seg, const int32_t* vseg,
                           int B, int n_max, int32_t* tours, float* costs, int32_t* n_missing, void* stream);

/*
 * Integer edge scores for tspgnn_tour_beam: score[e] = q(vote[e]) for the M votes of a batch, one launch, both arrays on
 * the device.  q(v) = clamp(rint(65536 * logsigmoid(v)), -2^22, 0) as int32, with logsigmoid(v) = min(v, 0) -
 * log1p(exp(-|v|)) evaluated in fp64 and rint rounding half to even; a NaN vote gives -2^22.  So +inf gives 0 and -inf
 * gives -2^22, and q never decreases as the vote rises.  The fixed point is chosen so that the sum over a tour of at most
 * 256 edges lies in [-2^30, 0]: every score sum of the beam search is exact int32 arithmetic.
 * M == 0 is a no-op; M < 0 or a null pointer with M > 0: TSPGNN_EINVAL before any launch.
 */
int tspgnn_vote_scores_i32(const float* vote, long long M, int32_t* score, void* stream);

/* Bytes of workspace tspgnn_tour_beam needs for B instances at n_max and beam: per instance two n_max x n_max int32
 * tables, n_max x beam words of parent trace and n_max x beam bytes of paths; 0 for an empty or unsupported request. */
long long tspgnn_tour_beam_workspace_bytes(int B, int n_max, int beam);

/*
 * A tour per instance by beam search over integer edge scores: the batch as above, with score:[M] int32 in place of the
 * votes (tspgnn_vote_scores_i32, or any integers: they are clamped to [-2^22, 0] on input, q(a,b) =
 * clamp(score[e(a,b)], -2^22, 0)).  beam: the width, 1 .. 1024; select: 0 = by score, 1 = by cost.  The result is exactly
 * this sequential process on instance b:
 *   Lists.    L_0 = [(path [0], S = 0)].  For k = 0 .. n-2 the candidates of L_k are all (i, u) with i an index into L_k,
 *             u not on path i, and e(last_i, u) existing; candidate (i, u) carries the score S_i + q(last_i, u).
 *             Candidates are ordered by score descending, then i ascending, then u ascending (a strict total order);
 *             L_{k+1} is the first min(beam, #candidates) candidates in that order, in that order, entry (i, u) being
 *             path i extended by u.
 *   Stranded. If L_{k+1} is empty (only on incomplete graphs), the tour is the path of L_k[0] followed by the unvisited
 *             vertices in ascending id; scores[b] = S of that entry and n_closed[b] = 0.
 *   Final.    Otherwise every entry i of L_{n-1} is a Hamiltonian path.  closed_i: e(last_i, 0) exists.
 *             F_i = S_i + q(last_i, 0) if closed, else S_i.  C_i = the fp32 cost of the entry's tour in canonical form,
 *             summed as costs[b].  select = 0: the chosen entry is the first by (closed first, F descending, i
 *             ascending); select = 1: the first by (closed first, ascending key of C, i ascending).  scores[b] = F of the
 *             chosen entry; n_closed[b] = the number of closed entries.
 *   Output.   tours, n_missing and costs as under Tour.
 * The result depends on beam and select as well, but not on the workgroup shape (256 / 512 / 1024 threads for n_max <= 64
 * / 128 / 256) or on what the workspace held before the launch.  beam = 1 is the walk from vertex 0 to the best-scoring
 * unvisited neighbour; an instance with m == 0 gets the identity tour, n_missing = n, cost 0 and score 0.  The kernel
 * takes an exact top-`beam` per step: a radix select on the composite key (-score, i, u) and a sort of the survivors; it
 * runs n - 1 steps.
 * workspace: 16-byte aligned device memory of at least tspgnn_tour_beam_workspace_bytes(B, n_max, beam) bytes, contents
 * irrelevant.  An instance with n outside [4, n_max] gets costs[b] = NaN, n_missing[b] = -1, scores[b] = 0,
 * n_closed[b] = -1 and no tour.
 * Beyond Checks: beam > 1024: TSPGNN_EUNSUPPORTED; beam < 1, select outside {0, 1} or a workspace that is short or
 * misaligned: TSPGNN_EINVAL.
 */
int tspgnn_tour_beam(const int32_t* score, const int32_t* uv, const float* wc, const int32_t* seg, const int32_t* vseg,
                     int B, int n_max, int beam, int select, void* workspace, long long workspace_bytes, int32_t* tours,
                     float* costs, int32_t* n_missing, int32_t* scores, int32_t* n_closed, void* stream);

/*
 * Candidate rows for tspgnn_tour_search_cand from the votes: the batch as above, and with it the vertex CSR the batch
 * carries: rowptr:[N+1] int32, and eid row g = the ids of the edges that list global vertex g as an endpoint.  tab: uint8
 * [N][K], K = k_vote + k_near; row vseg[b] + x is the candidate row of local vertex x of instance b.  The result is exactly
 * this sequential process on instance b and its vertex x:
 *   Row.    Pairs, read through CSR row x: e(x,y) is the smallest id in the row that joins x and y.  An id joins nothing
 *           when it lies outside seg[b] .. seg[b+1] or when the edge does not list x.  Only the set of ids in the row
 *           matters, not their order.  v(x,y) = vote[e(x,y)]; the neighbours of x are the y for which e(x,y) exists.
 *   Vote.   For s = 0 .. k_vote-1: among the neighbours of x not yet in the row, take the first by (vote key of v(x,y)
 *           descending, y ascending).  Write y to slot s.  If no neighbour is left, write x ("skip", which
 *           tspgnn_tour_search_cand ignores).
 *   Near.   For s = k_vote .. K-1: among the neighbours not yet in the row, take the first by (ascending key of w(x,y), y
 *           ascending), a NaN weight coming last.  Write y to slot s; if no neighbour is left, write x.
 * The kernel resolves multi-edges by an atomic minimum in LDS, then takes K wave-wide arg-max rounds per vertex; it sorts
 * nothing and needs no workspace.  An instance with n outside [4, n_max] gets its rows zero-filled.
 * Beyond Checks: k_vote < 0, k_near < 0 or K outside [1, 32]: TSPGNN_EINVAL.
 */
int tspgnn_vote_neighbors(const float* vote, const int32_t* uv, const float* wc, const int32_t* seg, const int32_t* vseg,
                          const int32_t* rowptr, const int32_t* eid, int B, int n_max, int k_vote, int k_near,
                          uint8_t* tab, void* stream);

/* ------------------------------------------------------------------ backward (tf.gradients, model.py:166) */

/*
 * Y = X W for a weight matrix resident in LDS: X:[rows,kin], Wp = pack_weights(W[kin,n1+n2]);
 * columns [0,n1) are written to Y1:[rows,n1], the rest to Y2:[rows,n2] (added to Y2 when
 * accumulate2 != 0).  n1+n2 in {64,128,256}; kin % 16 == 0.  Used for the data gradient of the LSTM
 * GEMM: [dx | dh] = dz K^T with Wp = pack_weights(K, transposed=1).
 */
int tspgnn_linear_f32(const float* X, int kin, const float* Wp, float* Y1, int n1, float* Y2, int n2,
                      int accumulate2, int rows, void* stream);

/* Workspace (floats) tspgnn_lnlstm_bwd_f32 needs for width d. */
long long tspgnn_lnlstm_bwd_workspace_floats(int d);

/*
 * Backward of one LayerNormBasicLSTMCell step (the gradient of graphnn.py:168-170).  Inputs are the
 * forward inputs (x,h,c,K packed,ln) plus dh_out/dc_out = gradients w.r.t. the step's outputs
 * (h', c'); either may be NULL (= zero).  Recomputes z, then writes dz:[rows,4d] (gradient w.r.t.
 * z = [x,h]K, consumed by tspgnn_linear_f32 and tspgnn_wgrad_f32), dc_in:[rows,d], and ADDS the
 * LayerNorm parameter gradients to ln_grad ([5][2][d], same layout as ln).
 */
int tspgnn_lnlstm_bwd_f32(const float* x, int dx, const float* h, const float* c, const float* K,
                          const float* ln, const float* dh_out, const float* dc_out, float* dz,
                          float* dc_in, float* ln_grad, float* workspace, int rows, int d, void* stream);

/* Backward of tspgnn_lnlstm_gather_fwd_f32: same outputs as tspgnn_lnlstm_bwd_f32 (dz, dc_in, LN grads);
 * the caller turns dz into dh = dz Kh^T (tspgnn_linear_f32), dZx = EV^T dz (tspgnn_csr_rowsum_f32, d=4d)
 * and the vertex-side gradients. */
int tspgnn_lnlstm_gather_bwd_f32(const int32_t* uv, const float* Zx, const float* h, const float* c,
                                 const float* Kh, const float* ln, const float* dh_out, const float* dc_out,
                                 float* dz, float* dc_in, float* ln_grad, float* workspace, int rows, int d,
                                 void* stream);

/*
 * Data gradient of tspgnn_mlp_fwd_f32: g = dY; for l = n_layers-1..0: mask by the saved activation of
 * layer l if it had relu (acts as written by mlp_fwd; Yout = forward output, only read when the
 * last layer has relu); dpre + l*dpre_stride <- g (gradient w.r.t. the layer's pre-activation; NULL
 * to skip); g <- g W_l^T.  Finally dX (+)= g (NULL to skip).  wt: per layer
 * pack_weights(W_l, transposed=1), d*d floats each, back to back.
 */
int tspgnn_mlp_bwd_f32(const float* dY, const float* wt, const float* acts, long long acts_stride,
                       const float* Yout, float* dpre, long long dpre_stride, float* dX,
                       int accumulate_dx, int rows, int d, int n_layers, unsigned relu_mask, void* stream);

/* Several independent backward tasks in one launch (see tspgnn_mlp_fwd_multi_f32): the edge-side and
 * vertex-side cells / message MLPs of one step.  Task arrays live in HOST memory. */
typedef struct tspgnn_lstm_bwd_task {
    const float* x; int dx; const float* h; const float* c; const float* K; const float* ln;
    const float* dh_out; const float* dc_out; float* dz; float* dc_in; float* ln_grad; float* workspace;
    int rows;
    const int32_t* uv; const float* Zx;   /* gather-init mode when uv != NULL: dx == 0, K = Kh */
    const float* KT; float* dxh;          /* optional (d == 64, gather-init mode): dxh[rows,d] = dz Kh^T in the same launch,
                                             KT = tspgnn_pack_weights_f32(Kh, 4d, d, transposed=1); dz is not re-read */
    int defer_reduce;                     /* != 0: ADD the workgroups' LayerNorm-gradient partials to `workspace` (zeroed by
                                             the caller before the first launch) and leave ln_grad alone; one
                                             tspgnn_lnlstm_bwd_finish_f32 after the last time step folds them -- one
                                             reduction per cell instead of one per time step */
    const float* zbias; const float* zscale; /* _h2 entry point only (the others require NULL): the forward's z started at
                                             zscale[row] * zbias[4d] (tspgnn_lstm_task: a bias folded through a row-sum
                                             aggregation); the recomputation of z starts there too */
    const void* KTg; float* dxg;          /* _h2 entry point only (the others require NULL), d == dx == 64, no KT, no uv: the
                                             data gradient [dxg[rows,dx] | dxh[rows,d]] = dz K^T in the same launch for a cell
                                             whose K^T cannot stay in LDS beside K: KTg = tspgnn_pack_weights_h2(K^T[4d, dx+d])
                                             in device memory, its fragments streamed through the L2 (few rows: the vertex
                                             cell).  Replaces one tspgnn_linear_f32 launch per time step */
} tspgnn_lstm_bwd_task;   /* fields as the arguments of tspgnn_lnlstm_bwd_f32 / tspgnn_lnlstm_gather_bwd_f32 */

typedef struct tspgnn_mlp_bwd_task {
    const float* dY; const float* wt; const float* acts; long long acts_stride; const float* Yout;
    float* dpre; long long dpre_stride; float* dX; int accumulate_dx; int rows; int n_layers; unsigned relu_mask;
    const int32_t* uv;                    /* optional, [rows,2]: gather-init mode -- dY is an [n_src,d] array and the chain
                                             starts from dY[uv[r][0]] + dY[uv[r][1]], i.e. the adjoint of the V<-E row-sum
                                             (EV x dY, graphnn.py:156-160 with adjoint_a) without materialising it */
    int acts_bf16;                        /* != 0: acts (and Yout) are bf16 arrays -- the tape of the bf16-storage mode; they
                                             only decide the relu masks.  The tasks of one launch share the flag */
    const float* pre_X; const void* pre_wt; int pre_k;
                                          /* _h2 entry point only (the others require NULL), d == 64, no uv: the chain starts
                                             from dY = pre_X[rows, pre_k] P^T instead of reading dY (then unused, may be
                                             NULL): pre_wt = tspgnn_pack_weights_h2(P^T[pre_k, d]) in device memory, fragments
                                             streamed through the L2; pre_k a multiple of 32, at most 256.  The vertex side of
                                             a folded cell input: dY = dZx Kx^T without its own tspgnn_linear_f32 launch */
} tspgnn_mlp_bwd_task;    /* fields as the arguments of tspgnn_mlp_bwd_f32 (uv = NULL there) */

int tspgnn_lnlstm_bwd_multi_f32(const tspgnn_lstm_bwd_task* tasks, int n_tasks, int d, void* stream);

/*
 * Training in the bf16-storage mode (model.py:160-167 with graphnn.py:18's float_dtype): backward kernels that read the
 * bf16 TAPE the forward wrote -- no widened copies -- and multiply on the bf16 matrix cores.  Gradients are fp32.
 *   tspgnn_lnlstm_bwd_multi_bf16: tspgnn_lstm_bwd_task with x, h (row-major) and Zx (projected-message format above) as
 *     bf16 arrays and K = the bf16 packing of the kernel (piece 0 of tspgnn_pack_weights_x3; Kh in gather-init mode);
 *     c, dh_out, dc_out, dz, dc_in, ln, ln_grad, workspace fp32 as in tspgnn_lnlstm_bwd_multi_f32.  z is recomputed with
 *     one bf16 MFMA per product (both operands are bf16-exact: the forward's own z).  KT / dxh / zbias must be NULL.
 *     d in {32, 64, 128}; at d = 128 Kh[128,512] is resident in LDS (128 KB).
 *   tspgnn_linear_bf16w_f32: tspgnn_linear_f32 with Wp = the bf16 packing of a bf16-exact W[kin, n1+n2] (e.g. K^T for
 *     [dx | dh] = dz K^T); X fp32, split into two bf16 pieces (16 significand bits), two MFMAs per product.
 *   tspgnn_wgrad_bf16x_f32: tspgnn_wgrad_f32 with X a bf16 array (h, messages, hidden activations of the tape): two
 *     bf16 MFMA terms per product (X exact, dY in two pieces = 16 significand bits, like the fp32 operand of
 *     tspgnn_linear_bf16w_f32); kin and nout multiples of 64 (else TSPGNN_EUNSUPPORTED).
 */
int tspgnn_lnlstm_bwd_multi_bf16(const tspgnn_lstm_bwd_task* tasks, int n_tasks, int d, void* stream);
int tspgnn_linear_bf16w_f32(const float* X, int kin, const void* Wp, float* Y1, int n1, float* Y2, int n2,
                            int accumulate_y2, int rows, void* stream);
int tspgnn_wgrad_bf16x_f32(const void* X, const float* dY, long long rows, int kin, int nout, float* dW, float* db,
                           float* workspace, void* stream);
/*
 * tspgnn_lnlstm_bwd_multi_f32 with both GEMMs (the recomputation of z and dh = dz Kh^T) on the fp16 matrix cores
 * (f16x2, csrc/dense_bwd_h2.hip).  Same task structure; d in {32, 64}, dx a multiple of 32, K (and K^T) resident in LDS:
 *   K  = tspgnn_pack_weights_h2 of kernel[dx+d, 4d] (Kh[d,4d] in gather-init mode);
 *   KT = tspgnn_pack_weights_h2 of Kh^T laid out [4d, d] (row-major transpose of Kh), dx == 0;
 *   Zx = the projected messages as the f16x2 forward wrote them (its projected-message format: scaled, blocked).
 * dz, dc_in, dxh and the LayerNorm gradients come back unscaled, exactly as from the _f32 function.
 */
int tspgnn_lnlstm_bwd_multi_h2(const tspgnn_lstm_bwd_task* tasks, int n_tasks, int d, void* stream);
/* ln_grad[10d] += fixed-order sum of the deferred partials in `workspace` (tspgnn_lnlstm_bwd_workspace_floats(d)). */
int tspgnn_lnlstm_bwd_finish_f32(const float* workspace, float* ln_grad, int d, void* stream);
int tspgnn_mlp_bwd_multi_f32(const tspgnn_mlp_bwd_task* tasks, int n_tasks, int d, void* stream);
/* tspgnn_mlp_bwd_multi_f32 with the data gradient on the fp16 matrix cores (f16x2: every row of dpre_l normalised by a
 * power of two, second piece scaled into fp16's normal range and accumulated apart -- csrc/mlp_bwd_rc.hip): the same task
 * structure with wt = n_layers blocks tspgnn_pack_weights_h2(W_l^T) (4 d d bytes each); d = 64, fp32 tapes, <= 4 tasks. */
int tspgnn_mlp_bwd_multi_h2(const tspgnn_mlp_bwd_task* tasks, int n_tasks, int d, void* stream);

/*
 * Backward of a message MLP's square layers that RECOMPUTES the hidden activations instead of reading a forward tape
 * (csrc/mlp_bwd_rc.hip) -- the data gradient of graphnn.py:150-155's `msg(h)` under model.py:160-167 from nothing but the
 * chain's input, its output and the incoming gradient; both GEMM chains on the fp16 matrix cores (f16x2):
 *   a_0 = X,  a_{l+1} = act_l(a_l W_l + b_l)  (recomputed as the f16x2 forward forms them; a_L = Yout is read),
 *   dpre_l = G_{l+1} * [a_{l+1} > 0]  (G_L = dY, or dY[uv[r][0]] + dY[uv[r][1]]),   G_l = dpre_l W_l^T,   dX (+)= G_0.
 * The weight gradients { a_l^T dpre_l, colsum(dpre_l) } are formed in the same launch (`partial`).  d = 64, 1 <= n_layers <= 3.
 * Opt-in (TSPGNN_RECOMPUTE=1): parity-green, slower than the taped backward at C2.
 */
typedef struct tspgnn_mlp_bwd_rc_task {
    const float* X;          /* [rows, d]: the chain's input rows */
    const void* wb;          /* the f16x2 forward's blocks {tspgnn_pack_weights_h2(W_l), 2^s b_l} (tspgnn_mlp_task.wb) */
    const void* wt;          /* n_layers blocks tspgnn_pack_weights_h2(W_l^T), 2 d d fp16 each */
    const float* Yout;       /* [rows, d]: the chain's output as the forward wrote it (needed if the last layer has relu) */
    const float* dY;         /* gradient w.r.t. the output: [rows, d], or [n_src, d] with uv */
    const int32_t* uv;       /* optional, [rows, 2]: gather-init mode as in tspgnn_mlp_bwd_task */
    float* dX; int accumulate_dx;
    int rows; int n_layers; unsigned relu_mask;
    float* acts; long long acts_stride;      /* must be NULL / 0 (ABI 4: the form that handed the recomputed activations and */
    float* dpre; long long dpre_stride;      /* pre-activation gradients to tspgnn_wgrad_f32 was removed; layout kept)        */
    float* partial;          /* required: the weight gradients are formed in the launch --
                                partial[workgroup] += { a_l^T dpre_l , colsum(dpre_l) }_l, per workgroup [W_0, b_0, W_1, ...];
                                tspgnn_mlp_bwd_rc_partial_floats(d, n_layers) floats, zeroed by the caller before the first
                                launch of a backward pass, ACCUMULATED by every launch, folded in a fixed order by
                                tspgnn_mlp_bwd_rc_finish_f32 into the flat [W,b,W,b,...] gradient slice.  Deterministic:
                                rows, LDS slots and the order of the sums are assigned statically */
} tspgnn_mlp_bwd_rc_task;
int tspgnn_mlp_bwd_rc_h2(const tspgnn_mlp_bwd_rc_task* task, int d, void* stream);
long long tspgnn_mlp_bwd_rc_partial_floats(int d, int n_layers);
int tspgnn_mlp_bwd_rc_finish_f32(const float* partial, float* grad_wb, int d, int n_layers, void* stream);

/* Workspace (floats) tspgnn_wgrad_f32 needs. */
long long tspgnn_wgrad_workspace_floats(long long rows, int kin, int nout);

/*
 * dW[kin,nout] += X^T dY and (db != NULL) db[nout] += colsum(dY); X:[rows,kin], dY:[rows,nout],
 * kin and nout multiples of 16.  rows may span all time steps of a batch (the per-step
 * activations and pre-activation gradients are stored contiguously), so each tf.Variable gets ONE
 * reduction.  Deterministic: fixed row chunks, partials in the workspace, one pass over chunks.
 */
int tspgnn_wgrad_f32(const float* X, const float* dY, long long rows, int kin, int nout, float* dW,
                     float* db, float* workspace, void* stream);

/* dvote[e] = (sigmoid(logits[p]) - labels[p]) / (B * n_edges[p]) for e in problem p: the gradient of
 * model.py:134-157 (mean cross entropy of per-problem mean votes) w.r.t. every edge vote. */
int tspgnn_vote_grad_f32(const float* logits, const float* labels, const int32_t* seg, float* dvote,
                         int B, void* stream);

/* dX[r,:] = dy[r] * w: backward of tspgnn_rowdot_f32 through X. */
int tspgnn_rowdot_bwd_f32(const float* dy, const float* w, float* dX, int rows, int d, void* stream);

long long tspgnn_wcolsum_workspace_floats(long long rows, int d);

/*
 * out[f] += scale * sum_r wt[r] * X[r,f]  (wt == NULL: plain column sums) and, if out_wsum != NULL,
 * out_wsum[0] += scale * sum_r wt[r].  Used for the gradients of the vote head's Dense(1) kernel /
 * bias and of V_init (model.py:47-51).  Deterministic two-stage reduction.
 */
int tspgnn_wcolsum_f32(const float* X, const float* wt, long long rows, int d, float scale, float* out,
                       float* out_wsum, float* workspace, void* stream);

long long tspgnn_einit_bwd_workspace_floats(int M, int d);

/* dwb += gradient of the E_init_MLP parameters (layout of tspgnn_einit_fwd_f32's wb) given
 * dE0:[M,d]; recomputes the forward chain per edge. */
int tspgnn_einit_bwd_f32(const float* WC, const float* wb, const float* dE0, float* dwb, float* workspace,
                         int M, int d, void* stream);

long long tspgnn_adam_workspace_floats(void);

/*
 * One optimiser step on the flat parameter buffer (model.py:160-167): g += l2_scale*theta (gradient
 * of l2_scale * sum l2_loss(var)); global_norm = ||g||; g *= clip/max(global_norm, clip)
 * (clip_norm <= 0: no clipping); Adam with the bias-corrected step lr_t.  gnorm_out[0] = global_norm.
 * step_counter == NULL: lr_t is the already bias-corrected rate lr*sqrt(1-b2^t)/(1-b1^t).
 * step_counter != NULL (device int): the counter is incremented to t and lr_t is the BASE rate, corrected on
 * the device -- no host value changes between steps, so the whole training step can be replayed as a HIP graph.
 * In data-parallel training g is the all-reduced (averaged) gradient.
 * skip_flag (optional device word): when non-zero at execution time the step is NOT applied -- theta, m, v and the
 * step counter stay as they are, gnorm_out is still written.  It is the range_flag of the step's f16x2 launches: a
 * gradient computed from an overflowed forward never reaches the variables, the caller repeats the step on the
 * _x3 / _f32 entry points.
 */
int tspgnn_adam_clip_step_f32(float* theta, float* g, float* m, float* v, int n, float l2_scale,
                              float clip_norm, float lr_t, float beta1, float beta2, float eps,
                              float* gnorm_out, float* workspace, int* step_counter, const unsigned* skip_flag,
                              void* stream);

/* ------------------------------------------------------------------ route head (csrc/route_head.hip, tspgnn/route_head.py) */

/*
 * Which edges of a resident batch lie on the instances' labelled tours.  The batch as under "tours from the edge votes":
 * uv:[M][2] global endpoint ids, seg:[B+1] edge prefix sums, vseg:[B+1] vertex prefix sums.  tours: int32 local vertex ids;
 * problem p's tour is the n_p = vseg[p+1] - vseg[p] entries from tours + tour_off[p], or from tours + vseg[p] when
 * tour_off is NULL (the tours concatenated in batch order).  3 <= n_p <= n_max <= 16384 (an int32 position table in LDS).
 *   marks[e]     1.0 where the edge joins its endpoints (both local ids in [0, n), different) and they are cyclically
 *                consecutive in the tour -- |pos[a] - pos[b]| in {1, n - 1}, the closing pair (tour[n-1], tour[0])
 *                included --, else 0.0.  Every entry of seg[0] .. seg[B] is written.
 *   n_missing[p] the tour's n pairs that no edge joins (a pair joined by several edges counts once).
 *   status[p]    0; 1 when the tour is no permutation of 0 .. n-1, 2 when n is outside [3, n_max]: then the problem's
 *                marks are zeros and n_missing[p] = -1.
 * One workgroup per problem; no floating-point arithmetic.  B == 0 is a no-op; n_max > 16384: TSPGNN_EUNSUPPORTED; B < 0,
 * n_max < 3 or a null pointer (tour_off aside): TSPGNN_EINVAL, before any launch.
 */
int tspgnn_route_edge_marks(const int32_t* uv, const int32_t* seg, const int32_t* vseg, const int32_t* tours,
                            const int32_t* tour_off, int B, int n_max, float* marks, int32_t* n_missing, int32_t* status,
                            void* stream);

/*
 * Per-edge sigmoid cross entropy of logits:[M] against marks:[M] (0 / 1), a mean over each problem's m_p edges and then
 * over the B problems:
 *   route_loss = (1/B) sum_p (1/m_p) sum_{e in p} w_e sce(x_e, y_e),   sce(x, y) = max(x, 0) - x y + log1p(exp(-|x|)),
 *   w_e = 1 for y_e = 0 and pos_weight for y_e = 1; pos_weight == 0 is the balanced rule w_e = (m_p - k_p) / max(k_p, 1),
 *   k_p the problem's marked edges.
 *   dlogit[e] = scale w_e (sigmoid(x_e) - y_e) / (B m_p)      (dlogit NULL: the statistics alone)
 *   stats[6]  = route_loss; the mean over the problems of (TP_p + TN_p) / m_p; TP, FP, TN, FN over the batch, an edge
 *               counted as predicted where x_e > 0 (TP: predicted and marked, FP: predicted and not marked, ...).
 * A problem without edges adds nothing.  Deterministic: one workgroup per problem, a thread's edges in ascending order, a
 * fixed tree over the workgroup, then the problems' partials in problem order; no floating-point atomics.  workspace:
 * tspgnn_edge_bce_workspace_floats(B) floats.  B < 1, pos_weight < 0 or a null pointer: TSPGNN_EINVAL.
 */
long long tspgnn_edge_bce_workspace_floats(int B);
int tspgnn_edge_bce_f32(const float* logits, const float* marks, const int32_t* seg, int B, float pos_weight, float scale,
                        float* dlogit, float* stats, float* workspace, void* stream);

/* ------------------------------------------------------------------ batches from a device-resident dataset */

/*
 * One batch, assembled on the device from a dataset that was uploaded once (tspgnn/device_dataset.py): writes exactly
 * the bytes tspgnn_host_stage_batch (below) writes for the instance list ids[0..B), in ONE launch.
 * The dataset, all DEVICE arrays, instance i of I:
 *   inst   int32[I][4]        n, m, first edge e0, first vertex v0 of the instance in the arrays below (prefix sums)
 *   uv     int32[sum m][2]    LOCAL endpoint ids of its edges in np.nonzero(Ma) order, at e0
 *   w      float[sum m]       (float)Mw[i,j] of those edges, at e0
 *   rowptr int32[sum (n+1)]   its local CSR by vertex, n + 1 entries at v0 + i
 *   eid    int32[2 sum m]     ... and its 2 m local edge ids, ascending inside a vertex, at 2 e0
 *   cost   double[I]          tspgnn_host_route_cost of its tour (may be NULL with use_target)
 * The batch: ids int32[B] on the DEVICE, each in [0, I) -- checked by the caller, not here; e_start / v_start
 * int32[B+1] on the DEVICE, the prefix sums of m[ids[b]] / n[ids[b]]; M = e_start[B], N = v_start[B].
 * Out, at dst + off[k] (dst on the DEVICE, off[7] a HOST array, the order of parallel.stage_layout):
 *   uv int32[M][2] local endpoint + v_start[b] | eid int32[2M] local edge id + e_start[b] | rowptr int32[N+1] local row
 *   pointer + 2 e_start[b], rowptr[N] = 2M | wc float[M][2] (weight, (float)c_b) | labels float[B] b mod 2 |
 *   seg int32[B+1] = e_start | n_edges int32[B].
 * c_b = target_cost if use_target, else (1.0 - dev) * cost for even b and (1.0 + dev) * cost for odd b, in fp64 with
 * two roundings like the host code.  Nothing outside the seven arrays is written.
 * B, M or N < 0, a null pointer with B > 0, dst or an offset not 8-byte aligned: TSPGNN_EINVAL before any launch.
 * B == 0 or M == 0 launches nothing and returns 0 (a batch without edges is all offsets: the caller fills it).
 */
int tspgnn_gather_batch(const int32_t* inst, const int32_t* uv, const float* w, const int32_t* rowptr,
                        const int32_t* eid, const double* cost, const int32_t* ids, const int32_t* e_start,
                        const int32_t* v_start, int B, int M, int N, double dev, int use_target, double target_cost,
                        unsigned char* dst, const long long* off, void* stream);

/* ------------------------------------------------------------------ datasets made on the device (DeviceDataset.generate) */

/*
 * The three stages between the reference's random draws (dataset.draw_streams, host) and a device-resident dataset
 * (csrc/dataset_build.hip).  One workgroup per instance, 4 <= n <= n_max <= 256.  An instance is a row of an int64 table
 * that is passed twice: `tab` on the HOST, checked row by row against the array sizes given, and `d_tab`, the same bytes
 * on the DEVICE, which the kernels read.  All other arrays are DEVICE arrays.  For each of the three: count < 0, n_max
 * outside [4, 256], a null pointer, an array not aligned to its element (uv: to 8 bytes), an n outside [4, n_max] or an
 * offset that leaves its array: TSPGNN_EINVAL before any launch.  count == 0 is a no-op that looks at nothing else.
 *
 * tspgnn_build_instances: tab[count][4] = n, first pair p0, first vertex t0, first matrix cell c0.  In: conn
 * double[count]; adj_u double[n_pairs], the instance's n (n-1) / 2 uniform draws at p0; coord: random_weights == 0:
 * double[2 n_verts], its points (x, y) at 2 t0, else double[n_pairs], its weights at p0; perm int32[n_verts], the
 * planted permutation at t0.  Out: Mw double[n_cells] and A uint8[n_cells], row-major n x n at c0; m int32[count].
 *   Pair k is the k-th (i, j > i) in row-major order.  A[i][j] = A[j][i] = adj_u[k] < conn, or {i, j} is an edge
 *   perm[t] - perm[t+1 mod n] of the planted cycle.  Points: Mw[i][j] = sqrt((x_i - x_j) (x_i - x_j) + (y_i - y_j)
 *   (y_i - y_j)), each subtraction, product, sum and the root rounded once to nearest (no FMA); weights: Mw[i][j] =
 *   Mw[j][i] = coord[p0 + k].  Both diagonals are 0.  m = the number of set pairs i < j.
 */
int tspgnn_build_instances(const long long* tab, const long long* d_tab, const double* conn, const double* adj_u,
                           const double* coord, const int32_t* perm, int random_weights, int count, int n_max,
                           long long n_pairs, long long n_verts, long long n_cells, double* Mw, unsigned char* A,
                           int32_t* m, void* stream);

/*
 * tspgnn_penalise_instances: tab[count][3] = n, first matrix cell c0, first output float f0.  (A, Mw) as above -> the
 * input of the tour kernels at W + f0: triangle == 0 the row-major n x n matrix of tspgnn_tour_search (n_max <= 128),
 * else the packed strict upper triangle of tspgnn_tour_search_tri; n_floats is the extent of W.
 *   w(i, j) = Mw[min][max] + 0.0; mx = the fp64 maximum of 0 and w over the set pairs; pen = n * mx + 1.0 with two
 *   roundings; the value is 0 on the diagonal, w(i, j) where A is set and pen elsewhere; each is converted to fp32 to
 *   nearest and then stepped down one ulp when the fp32 value exceeds the fp64 one (dataset._penalised bit for bit).
 */
int tspgnn_penalise_instances(const long long* tab, const long long* d_tab, const unsigned char* A, const double* Mw,
                              int count, int n_max, int triangle, long long n_cells, long long n_floats, float* W,
                              void* stream);

/*
 * tspgnn_pack_dataset: tab[count][7] = n, first matrix cell c0, first tour entry t0, m, first edge e0, first vertex v0,
 * position i of the instance in the dataset.  (A, Mw) as above and its tour tours[t0 .. t0 + n) -> the arrays of
 * tspgnn_gather_batch's dataset: uv / w at e0, eid at 2 e0, rowptr (n + 1 entries) at v0 + i, and cost[i],
 * file_cost[i], cycle_cost[i], feasible[i].  n_tour, n_edges, n_rowptr, n_inst are the extents of tours, of uv / w (eid:
 * twice), of rowptr and of the four per-instance arrays; uv, w and eid may be NULL when n_edges == 0.
 *   Edges are the set pairs i < j in row-major order (np.nonzero(np.triu(A))); uv holds (i, j), w = (float)Mw[i][j];
 *   rowptr / eid are the CSR by vertex with ascending edge ids inside a vertex (tspgnn_host_csr_by_vertex).
 *   cost = tspgnn_host_route_cost of the tour on Mw: one lane sums Mw[min][max] in route order, the closing pair is
 *   (route[n-1], route[1]), the sum is divided by n; this is the cost array of the dataset, what DeviceDataset keeps for
 *   an instance (Ma, Mw, route) held in memory.  file_cost = the same on the file form of Mw, which is Mw on the set
 *   pairs i < j and 0 elsewhere -- what a .graph file of the instance would give (n * file_cost is dataset._target); the
 *   two differ only when the closing pair or a tour edge is absent from A.  cycle_cost = the fp64 sum of Mw[min][max]
 *   along the closed tour, in tour order.  feasible = every tour edge is set in A.  A tour entry outside [0, n) makes
 *   the costs NaN.  An m that is not the mask's count writes the row pointers and the scalars only.
 */
int tspgnn_pack_dataset(const long long* tab, const long long* d_tab, const unsigned char* A, const double* Mw,
                        const int32_t* tours, int count, int n_max, long long n_cells, long long n_tour,
                        long long n_edges, long long n_rowptr, long long n_inst, int32_t* uv, float* w, int32_t* rowptr,
                        int32_t* eid, double* cost, double* file_cost, double* cycle_cost, int32_t* feasible,
                        void* stream);

/* ------------------------------------------------------------------ ".graph" text made on the device (csrc/graph_text.hip)
 *
 * Python's repr(float) of count doubles: the shortest digit string that reads back to the same bits (of those the one
 * nearest the value, a tie to the even digit), positional for 1e-4 <= |x| < 1e16 with ".0" on integers, d[.ddd]e+XX /
 * e-XX otherwise, and "0.0", "-0.0", "inf", "-inf", "nan".  Value i goes to text[24 i .. 24 i + len[i]), len[i] <= 24; the
 * rest of its 24 bytes is left alone.  Integer arithmetic only, the same routine on host and device.
 * tspgnn_host_f64_repr takes HOST pointers and launches nothing; tspgnn_f64_repr takes device arrays (one thread per
 * value).  NULL or count < 0: TSPGNN_EINVAL before any launch; count == 0: no-op.
 */
int tspgnn_host_f64_repr(const double* x, long long count, char* text, unsigned char* len);
int tspgnn_f64_repr(const double* x, long long count, char* text, unsigned char* len, void* stream);

/*
 * The bytes tspgnn.write_graph(np.triu(A), Mw, path, route=tour) writes for each of count instances, one 256-thread
 * workgroup per instance, 4 <= n <= n_max <= 256.  (A, Mw, tours) as tspgnn_pack_dataset takes them: A uint8[n][n] and Mw
 * double[n][n] at cell c0, the tour of n int32 entries at t0; n_cells and n_tour are the extents.  Only the cells j > i of
 * A are read: a pair is set when its byte is non-zero, every other cell prints "0".  tab is passed twice, on the HOST
 * (every row is checked against the extents before anything launches) and on the device (d_tab).
 *
 * tspgnn_graph_text_sizes: tab[count][3] = n, c0, t0 -> bytes[i] (device) = the exact length of file i.  A tour entry
 * outside [0, n) counts as one character; tspgnn_graph_text_write refuses such an instance.
 *
 * tspgnn_graph_text_write: tab[count][4] = n, c0, t0, b0 -> file i in text[b0 .. b0 + bytes[i]), where bytes is the
 * DEVICE array the sizes launch filled and host_bytes its copy on the HOST: the host check of row i is b0 >= 0 and
 * b0 + host_bytes[i] <= n_text (the kernel reads bytes, never host_bytes).  Every store is guarded by the instance's
 * extent.  status[i] (device) = 0 written; 1 the kernel's own size differs from bytes[i], nothing written; 2 a tour entry
 * outside [0, n), nothing written.  Both passes format the weights (the sizes pass keeps only the lengths): no scratch
 * table travels between them.
 *
 * TSPGNN_EINVAL before any launch: a NULL pointer, count < 0, n_max outside [4, 256], an n outside [4, n_max], an
 * offset that leaves its array.  count == 0: no-op.
 */
int tspgnn_graph_text_sizes(const long long* tab, const long long* d_tab, const unsigned char* A, const double* Mw,
                            const int32_t* tours, int count, int n_max, long long n_cells, long long n_tour,
                            long long* bytes, void* stream);
int tspgnn_graph_text_write(const long long* tab, const long long* d_tab, const unsigned char* A, const double* Mw,
                            const int32_t* tours, int count, int n_max, long long n_cells, long long n_tour,
                            const long long* bytes, const long long* host_bytes, char* text, long long n_text,
                            int32_t* status, void* stream);

/* ------------------------------------------------------------------ ".graph" text read on the device (csrc/graph_parse.hip)
 *
 * Python's float(token) of count tokens: token i is the len[i] (int32) bytes at off[i] (int64) of buf, n_buf the extent of
 * buf.  -> bits[i], the double as uint64, and status[i] (uint8): 0 parsed; 1 malformed, float(token) would raise too (also:
 * a token that leaves buf); 2 well-formed for strtod or float() but outside the device grammar -- the host reader can
 * still read a file with such a token.  bits[i] is 0 unless status[i] is 0.
 *   Grammar: [+-]? ( digits [. digits?] | . digits ) ( [eE] [+-]? digits )?, or [+-]?inf, or nan, lower case only: the
 * spellings tspgnn_f64_repr emits.  After its leading zeros the mantissa holds at most 19 digits, integer and fraction
 * digits together; the exponent field may have any number of digits and saturates (1e9999 is inf, 1e-9999 is 0.0); a
 * token is at most 48 bytes.  Status 2: more than 19 digits, 0x..., Infinity, NaN and every other case of inf / nan, a
 * signed nan, '_' between digits, more than 48 bytes.
 *   For status 0 the result is float(token) bit for bit: to nearest, ties to even, through subnormals, underflow to
 * +-0.0 and overflow to +-inf, the sign of zero kept.  Integer arithmetic only, the same routine on host and device:
 * mode 0 rounds from the 192-bit product with a 128-bit power of ten wherever that decides it and by exact multi-word
 * comparison with the midpoint elsewhere; mode 1 sends every token through the exact comparison (for tests).
 * tspgnn_host_f64_parse takes HOST pointers and launches nothing; tspgnn_f64_parse takes device arrays (one thread per
 * token).  NULL, count < 0 or n_buf < 0: TSPGNN_EINVAL before any launch; count == 0: no-op.
 */
int tspgnn_host_f64_parse(const unsigned char* buf, long long n_buf, const long long* off, const int32_t* len,
                          long long count, int mode, unsigned long long* bits, unsigned char* status);
int tspgnn_f64_parse(const unsigned char* buf, long long n_buf, const long long* off, const int32_t* len, long long count,
                     int mode, unsigned long long* bits, unsigned char* status, void* stream);

/*
 * count ".graph" files side by side in the device byte buffer text (n_text bytes), file i in [b0, b0 + bytes), read as
 * tspgnn_host_read_graph reads them (instance_loader.py:95-127), one 256-thread workgroup per file.  tab is passed twice,
 * on the HOST (every row is checked against the extents before anything launches) and on the device (d_tab); every load
 * and store of a kernel is guarded by the file's extent and the row's.
 *   The first DIMENSION; n the integer after it, past ':', blanks and tabs; EDGE_DATA_SECTION, EDGE_WEIGHT_SECTION and
 * TOUR_SECTION each the first occurrence at or after the previous section's first line; pair lines "i j" until the first
 * line that contains the two bytes "-1" (or does not begin with an integer); the weights the first n^2 tokens of the
 * weight section separated by blank, tab, CR, LF, VT, FF, later tokens ignored; the tour the integers on the line after
 * TOUR_SECTION, separated by blanks and tabs.  Unlike strtol this reader stays on a line: a pair line with one integer
 * is status 5 and a blank pair line is skipped.
 *
 * tspgnn_graph_text_scan: tab[count][2] = b0, bytes -> info[i][8] (device, int32) = status, n, tour length, the offsets
 * in the file of the first lines of the three sections (-1: absent), the number of pair lines, 0.  It reads everything
 * but the weights.
 *
 * tspgnn_graph_text_parse: tab[count][5] = b0, bytes, n, c0, t0 with n what the scan gave -> the uint8 mask A[c0 .. c0 +
 * n^2), all of it, zeros included, symmetric as tspgnn_build_instances makes it (a pair i < j sets [i][j] and [j][i]);
 * Mw[c0 ..) in fp64 (tspgnn_f64_parse, mode 0); tours[t0 .. t0 + n) in int32; m[i], the number of set pairs
 * (tspgnn_build_instances' m); status[i] (int32).  n_cells and n_tour are the extents.
 *
 * status: 0 read; 3 no DIMENSION, or n <= 0 (parse: n differs from the row's); 4 a section is missing; 5 a pair outside
 * [0, n); 6 fewer than n^2 weight tokens, or a malformed one; 7 a tour entry outside [0, n); 8 n outside [4, 256],
 * tspgnn_pack_dataset's range; 9 a pair with i >= j (tspgnn_pack_dataset lists the pairs of np.triu(A)); 10 tour length
 * != n; 11 a weight token outside the device grammar.  3 to 7 mirror the host reader's codes; the lowest that applies is
 * reported.  A non-zero status in either launch means the caller uses nothing of that file.
 *
 * TSPGNN_EINVAL before any launch: a NULL pointer, count < 0, n_max outside [4, 256] or an n outside [4, n_max] (parse), a
 * file above 2^30 bytes, an offset that leaves its array.  count == 0: no-op.
 */
int tspgnn_graph_text_scan(const long long* tab, const long long* d_tab, const char* text, long long n_text, int count,
                           int32_t* info, void* stream);
int tspgnn_graph_text_parse(const long long* tab, const long long* d_tab, const char* text, long long n_text, int count,
                            int n_max, long long n_cells, long long n_tour, unsigned char* A, double* Mw, int32_t* tours,
                            int32_t* m, int32_t* status, void* stream);

/* ------------------------------------------------------------------ host-side batch packing (no GPU work) */

/*
 * Appends the edges of one instance to a batch under construction: for every non-zero Ma[i,j] in np.nonzero
 * (row-major) order writes uv = (v_off+i, v_off+j) and W = Mw[i,j] (instance_loader.py:56-67, without the dense
 * EV).  Ma:[n,n] of kind 0=int8/bool 1=int32 2=int64 3=float32 4=float64; Mw:[n,n] float64.  HOST pointers.
 * Returns the number of edges written, or -1 on a bad argument.
 */
long long tspgnn_host_pack_instance(const void* Ma, int ma_kind, const double* Mw, int n, int v_off,
                                    int32_t* uv, double* W);

/* Tour cost per vertex exactly as instance_loader.py:70 (closing pair (route[-1], route[1])). HOST pointers. */
double tspgnn_host_route_cost(const double* Mw, int n, const int64_t* route, int len);

/* CSR of EV^T (rowptr:[N+1], eid:[2M], ascending edge ids per vertex) from the endpoint list; HOST pointers.
 * 0 = OK, -2 = endpoint out of range. */
int tspgnn_host_csr_by_vertex(const int32_t* uv, long long M, int N, int32_t* rowptr, int32_t* eid);
/* Whole-batch packing (one call instead of one per instance): per-instance host pointers / sizes in arrays.
 * tspgnn_host_count_edges fills n_edges[B] (= count_nonzero(Ma)); tspgnn_host_pack_batch then fills uv[M,2], W[M]
 * and C[M] (target_cost if use_target, else (1 -/+ dev) * tour cost for even / odd instances) and returns M. */
int tspgnn_host_count_edges(const void* const* Ma, const int* ma_kind, const int* n, int B, int64_t* n_edges);
long long tspgnn_host_pack_batch(const void* const* Ma, const int* ma_kind, const double* const* Mw, const int* n,
                                 const int64_t* const* route, const int* route_len, int B, double dev, int use_target,
                                 double target_cost, int32_t* uv, double* W, double* C);
/*
 * Parser of the reference's ".graph" instance files (dataset.py:145-187 / instance_loader.py:95-127).  Call with
 * Ma == Mw == NULL to get n and the tour length, then with Ma[n*n] (int64 0/1), Mw[n*n] (double), route[len].
 * Returns 0, or <0: -1 bad arguments, -2 cannot open, -3 no/invalid DIMENSION, -4 missing section, -5 edge out of
 * range, -6 malformed weight matrix.
 */
/* One device batch's worth of arrays packed by one call into one caller-owned (pinned) buffer: off[7] = byte offsets of
 * uv int32[M][2], eid int32[2M], rowptr int32[N+1], wc float[M][2], labels float[B], seg int32[B+1], n_edges int32[B]
 * (instance_loader.py:29-80 + the conversions of the feed, train.py:25-33).  Returns M; -1 malformed, -2 a route leaves
 * its graph, -3 M / N differ from M_expected / N_expected.  Thread-safe (thread-local scratch). */
long long tspgnn_host_stage_batch(const void* const* Ma, const int* ma_kind, const double* const* Mw, const int* n,
                                  const int64_t* const* route, const int* route_len, int B, double dev, int use_target,
                                  double target_cost, long long M_expected, int N_expected, unsigned char* stage,
                                  const long long* off);
int tspgnn_host_read_graph(const char* path, int* n_out, int* route_len_out, int64_t* Ma, double* Mw, int64_t* route);

/*
 * Storage conversions of the bf16-storage mode (BASELINE config 5; graphnn.py:18 float_dtype): y[i] = bf16(x[i]), round to
 * nearest even / y[i] = float(x[i]), n elements, both pointers 16-byte aligned.  The mode needs them at its two ends -- the
 * caller's fp32 initial embeddings in, E.h out to the fp32 vote head (model.py:118-128).
 */
int tspgnn_convert_f32_to_bf16(const float* x, void* y, long long n, void* stream);
int tspgnn_convert_bf16_to_f32(const void* x, float* y, long long n, void* stream);

/*
 * The data-parallel bucket of a training step (the reference has no counterpart: model.py:157-167 run in
 * one process).  bucket = [ gradient of the rank's mean loss (n floats) | 8-float tail ].  pack: gradient *= local_batch
 * (with_grad != 0), tail = { local_batch, local_batch * stats[0] (loss), local_batch * stats[1] (acc), stats[2..5] (TP,
 * FP, TN, FN), (float) *range_flag }; stats / range_flag may be NULL (zeros).  After ONE all-reduce(sum) of the bucket --
 * of the tail alone when only statistics are reduced: with_grad == 0 and the gradient part is not touched -- unpack
 * divides the gradient and the two means by the reduced batch size tail[0], copies the four counts, and sets
 * *range_flag = (reduced flag != 0): every rank's optimiser launch then skips or applies the step together.
 */
int tspgnn_bucket_pack_f32(float* bucket, int n, int with_grad, float local_batch, const float* stats,
                           const unsigned* range_flag, void* stream);
int tspgnn_bucket_unpack_f32(float* bucket, int n, int with_grad, float* stats, unsigned* range_flag, void* stream);

/*
 * Gradient accumulation: one optimiser step over several micro-batches (a micro-batch is a rank that runs later).  accum
 * has the bucket's layout, n floats and the 10 tail slots; grad (n floats, the gradient of the micro-batch's mean loss) is
 * only read.  For i < n: t = local_batch * grad[i], accum[i] = first ? t : accum[i] + t, the product and the sum each
 * rounded to fp32 (no fma).  For tail slot k: v = what tspgnn_bucket_pack_f32 writes there from local_batch, stats and
 * range_flag (NULL: zeros), accum[n + k] = first ? v : accum[n + k] + v -- a guard slot counts the flagged micro-batches.
 * first != 0 WRITES: whatever accum held, NaN included, is gone.  n == 0 touches the tail only.  TSPGNN_EINVAL: accum NULL,
 * n < 0, grad NULL with n > 0, accum == grad.  tspgnn_bucket_unpack_f32 on the accumulated (and, across ranks, once
 * all-reduced) bucket finishes the step: it divides by the summed batch size, copies the counts, rebuilds the flag word.
 */
int tspgnn_bucket_accumulate_f32(float* accum, const float* grad, int n, int first, float local_batch,
                                 const float* stats, const unsigned* range_flag, void* stream);

/*
 * Launch plans: what an entry's launcher decides in host code from the task shapes and the CU count, answered by the
 * same planner the launcher calls (csrc/launch_plan.h).  Host only -- nothing is launched, no device is needed, and no
 * pointer is dereferenced: a pointer field of a task counts as null or non-null.  Every query takes the arguments that
 * shape the plan of the entry it describes plus `cus` (0: the device's count, the one the launcher uses; 256 without a
 * device), validates the shape fields as the entry does, answers TSPGNN_EUNSUPPORTED exactly where the launch would, and
 * fills a zeroed plan (grid 0) where the entry would launch nothing (no rows).  The tests claim a branch through these
 * before they launch (tests/plan_replay.py); tests/golden/launch_plans.json records them across their thresholds.
 */
enum { TSPGNN_LINEAR_SPLIT = 0, TSPGNN_LINEAR_TICKET = 1, TSPGNN_LINEAR_STREAMED = 2 };
typedef struct tspgnn_linear_plan {   /* tspgnn_linear_f32 */
    int path;       /* TSPGNN_LINEAR_*: linear_split_kernel / linear_kernel with W resident / W streamed through LDS */
    int nw, grid;   /* wavefronts per workgroup, workgroups */
    int qc;         /* 16-row blocks of W per LDS staging (>= kin / 16: resident) */
    int per_cu;     /* workgroups per CU the LDS size allows */
    int tiles;      /* 16-row tiles */
    int lds_bytes;
} tspgnn_linear_plan;
int tspgnn_plan_linear(int kin, int n1, int n2, int rows, int cus, tspgnn_linear_plan* out);

typedef struct tspgnn_tasks_plan {    /* the ticket launches that only share out workgroups */
    int nw, grid, n;                  /* n: live tasks (rows > 0), in order */
    int blk_end[4];                   /* task k owns the workgroups [blk_end[k-1], blk_end[k]) */
    int lds_bytes;                    /* dynamic LDS of the launch (0: none) */
} tspgnn_tasks_plan;
int tspgnn_plan_mlp_bwd(const tspgnn_mlp_bwd_task* tasks, int n_tasks, int d, int cus, tspgnn_tasks_plan* out); /* tspgnn_mlp_bwd_multi_f32 */
int tspgnn_plan_mlp_fwd(const tspgnn_mlp_task* tasks, int n_tasks, int d, int cus, tspgnn_tasks_plan* out);     /* tspgnn_mlp_fwd_multi_h2 / _x3, tspgnn_mlp_head_fwd_h2 */
int tspgnn_plan_mlp_fwd_f32(const tspgnn_mlp_task* tasks, int n_tasks, int d, int cus, tspgnn_tasks_plan* out); /* tspgnn_mlp_fwd_multi_f32 */
/* tspgnn_mlp_fwd_multi_bf16; nw: the wavefronts per workgroup its dispatch chooses (16 at d = 128 without a projection, else 8) */
int tspgnn_plan_mlp_fwd_bf16(const tspgnn_mlp_task_bf16* tasks, int n_tasks, int d, int nw, int cus, tspgnn_tasks_plan* out);

enum { TSPGNN_WGRAD_GENERIC = 0, TSPGNN_WGRAD_X3 = 1, TSPGNN_WGRAD_X3_PAIR = 2 };
typedef struct tspgnn_wgrad_plan {    /* tspgnn_wgrad_f32 (bf16x == 0), tspgnn_wgrad_bf16x_f32 (bf16x != 0) */
    int kernel;             /* TSPGNN_WGRAD_*: wgrad_kernel<av, bv> / wgrad_x3_kernel / the same, two X blocks per wavefront */
    int av, bv;             /* 16-wide feature blocks of X / dY per wavefront of the generic kernel */
    int nob;                /* output blocks the chunking counts with: kin / (16 av) * nout / (16 bv) */
    int n_chunks;           /* row chunks = partial results in the workspace = terms of the second stage's sums */
    int launch_nob, grid;   /* output blocks (wavefronts per chunk) of the chosen kernel, its workgroups */
    long long chunk_rows;
} tspgnn_wgrad_plan;
int tspgnn_plan_wgrad(long long rows, int kin, int nout, int bf16x, int cus, tspgnn_wgrad_plan* out);

typedef struct tspgnn_wcolsum_plan {  /* tspgnn_wcolsum_f32 */
    int n_chunks, capped;   /* capped: the 4 per CU cap on the chunk count took effect */
    long long chunk_rows;
} tspgnn_wcolsum_plan;
int tspgnn_plan_wcolsum(long long rows, int d, int cus, tspgnn_wcolsum_plan* out);

typedef struct tspgnn_einit_bwd_plan {   /* tspgnn_einit_bwd_f32 */
    int grid, n_chunks;     /* persistent workgroups, 64-edge chunks */
    int full_grid;          /* the grid before the clamp to the chunk count */
} tspgnn_einit_bwd_plan;
int tspgnn_plan_einit_bwd(int M, int d, int cus, tspgnn_einit_bwd_plan* out);

enum { TSPGNN_ARITH_H2 = 0, TSPGNN_ARITH_X3 = 1, TSPGNN_ARITH_F32 = 2, TSPGNN_ARITH_BF16 = 3 };
typedef struct tspgnn_cell_fwd_plan {    /* tspgnn_lnlstm_mlp_fwd_multi_h2 / _x3 (arith: TSPGNN_ARITH_*) */
    int nw, grid, n;
    int blk_end[4];
    int lockstep[4];        /* 0: K and the MLP resident, tiles by ticket; 1: lock-step rounds */
    int kbc[4];             /* k-blocks (32 rows of K) per LDS chunk */
    int together[4];        /* h2, lock step: MLP layers and projection matrix in one residency */
    int lock_tiles[4];      /* lock step: working wavefronts per workgroup (0: resident) */
    int n_lo_lds[4];        /* x3: MLP layers whose lo piece is in LDS */
    int n_rounds[4];        /* lock step: rounds per workgroup behind the task's fixed share (0: resident) */
    int split_fixed;        /* 1: the lock-step tasks kept their fixed share; 0: the plain split by cost */
    int centered, wt;       /* h2: the template variant */
    int lds_bytes;
} tspgnn_cell_fwd_plan;
int tspgnn_plan_cell_fwd(const tspgnn_cell_mlp_task* tasks, int n_tasks, int d, int arith, int cus, tspgnn_cell_fwd_plan* out);

typedef struct tspgnn_cell_chunk_plan {  /* the cell launches whose only LDS decision is K resident or in chunks */
    int nw, grid, n;
    int blk_end[4];
    int qc[4];          /* units of K per LDS chunk: 16-row blocks (f32 backward), 32-row k-blocks (bf16), 0 (h2 backward: always resident) */
    int chunked[4];     /* K streamed through LDS rather than resident */
    int lds_bytes;
} tspgnn_cell_chunk_plan;
/* tspgnn_lnlstm_bwd_multi_f32 / _h2 / _bf16 (arith: TSPGNN_ARITH_F32 / _H2 / _BF16) */
int tspgnn_plan_cell_bwd(const tspgnn_lstm_bwd_task* tasks, int n_tasks, int d, int arith, int cus, tspgnn_cell_chunk_plan* out);
/* tspgnn_lnlstm_fwd_multi_bf16; nw: the wavefronts per workgroup its dispatch chooses (12 for the staged kernel at d = 64, else 8) */
int tspgnn_plan_lstm_fwd_bf16(const tspgnn_lstm_task_bf16* tasks, int n_tasks, int d, int nw, int cus, tspgnn_cell_chunk_plan* out);
/* tspgnn_lnlstm_fwd_multi_f32: nw, grid, blk_end and lds_bytes describe the ONE launch of the resident tasks (chunked[k] == 0;
 * grid 0: there is none), in which a chunked task owns no workgroup (blk_end[k] == blk_end[k-1]).  Every chunked task runs in
 * a launch of its own: 8 wavefronts, K in chunks of qc[k] 16-row blocks, min(cus, ceil(tiles / 8)) workgroups, round r of 8
 * tiles to workgroup r mod that.  qc[k] of a resident task: all (dx + d) / 16 blocks.  TSPGNN_EUNSUPPORTED: a gather-init or
 * bias-init task whose K does not fit LDS -- the entry answers it before it launches any task. */
int tspgnn_plan_lstm_fwd_f32(const tspgnn_lstm_task* tasks, int n_tasks, int d, int cus, tspgnn_cell_chunk_plan* out);

/* Slices of the chunk range per workgroup in the second stage of the split reductions (wgrad, wcolsum). */
int tspgnn_plan_reduce_slices(int n_chunks);
/* Workgroups of the launches that cap their grid and stride over the rest: clamp(ceil(total / per_block), 1, cap). */
int tspgnn_plan_strided_blocks(long long total, int per_block, int cap);

#ifdef __cplusplus
}
#endif
#endif /* TSPGNN_H */
