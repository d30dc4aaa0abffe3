// The route head's once-per-batch kernels (tspgnn/route_head.py, Session.loss_and_grads): which edges of a resident batch
// lie on the instances' labelled tours (tspgnn_route_edge_marks), and the per-edge sigmoid cross entropy of the head's
// logits against those marks with its gradient and statistics (tspgnn_edge_bce_f32).  include/tspgnn.h, "route head",
// states both.  Both are memory-trivial next to the message-passing loop: one workgroup per problem, plain loads and
// stores, integer LDS atomics only (their result does not depend on the order), every floating-point sum in a fixed order.
#include "common.h"
#include "launch_plan.h"

namespace tspgnn {
namespace {

constexpr int kRouteThreads = 256;
constexpr int kRouteMinN = 3, kRouteMaxN = 16384;   // an int32 position table of 64 KB

__device__ __forceinline__ int lds_words_of_bits(int n) { return (n + 31) >> 5; }

// One workgroup per problem.  LDS: pos[n] the position of a vertex in the tour, then one bit per tour pair k -- the pair
// (tour[k], tour[k+1]), k = n - 1 the closing pair -- set when an edge joins it.
__global__ __launch_bounds__(kRouteThreads) void route_edge_marks_kernel(const int32_t* __restrict__ uv,
                                                                         const int32_t* __restrict__ seg,
                                                                         const int32_t* __restrict__ vseg,
                                                                         const int32_t* __restrict__ tours,
                                                                         const int32_t* __restrict__ tour_off, int n_max,
                                                                         float* __restrict__ marks,
                                                                         int32_t* __restrict__ n_missing,
                                                                         int32_t* __restrict__ status) {
    extern __shared__ int32_t route_lds[];
    __shared__ int s_bad, s_pairs;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int v0 = vseg[p], n = vseg[p + 1] - v0;
    const long long e0 = seg[p], m = (long long)seg[p + 1] - e0;
    float* out = marks + e0;
    // what the host never sends: no table is built, the problem's marks are zeros
    if (n < kRouteMinN || n > n_max || n > kRouteMaxN) {
        for (long long e = tid; e < m; e += kRouteThreads) out[e] = 0.f;
        if (tid == 0) {
            n_missing[p] = -1;
            status[p] = 2;
        }
        return;
    }
    int32_t* pos = route_lds;
    uint32_t* pair_bits = reinterpret_cast<uint32_t*>(route_lds + n_max);
    const int n_words = lds_words_of_bits(n);
    const int32_t* tour = tours + (tour_off ? tour_off[p] : v0);
    if (tid == 0) s_bad = 0, s_pairs = 0;
    for (int v = tid; v < n; v += kRouteThreads) pos[v] = -1;
    for (int w = tid; w < n_words; w += kRouteThreads) pair_bits[w] = 0u;
    __syncthreads();
    // n entries, each in [0, n), none twice: a permutation
    bool bad = false;
    for (int k = tid; k < n; k += kRouteThreads) {
        const int v = tour[k];
        if (v < 0 || v >= n) bad = true;
        else if (atomicExch(&pos[v], k) != -1) bad = true;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (s_bad) {   // workgroup-uniform
        for (long long e = tid; e < m; e += kRouteThreads) out[e] = 0.f;
        if (tid == 0) {
            n_missing[p] = -1;
            status[p] = 1;
        }
        return;
    }
    for (long long e = tid; e < m; e += kRouteThreads) {
        const int a = uv[2 * (e0 + e)] - v0, b = uv[2 * (e0 + e) + 1] - v0;
        float mark = 0.f;
        if (a >= 0 && a < n && b >= 0 && b < n && a != b) {
            const int pa = pos[a], pb = pos[b];
            const int lo = min(pa, pb), dist = max(pa, pb) - lo;
            // n >= 3: dist 1 and dist n - 1 are different pairs, so a pair is counted once (n = 3: pairs 0, 1 and 2)
            const int k = dist == 1 ? lo : dist == n - 1 ? n - 1 : -1;
            if (k >= 0) {
                mark = 1.f;
                atomicOr(&pair_bits[k >> 5], 1u << (k & 31));
            }
        }
        out[e] = mark;
    }
    __syncthreads();
    int found = 0;
    for (int w = tid; w < n_words; w += kRouteThreads) found += __popc(pair_bits[w]);
    if (found) atomicAdd(&s_pairs, found);
    __syncthreads();
    if (tid == 0) {
        n_missing[p] = n - s_pairs;
        status[p] = 0;
    }
}

// tf.nn.sigmoid_cross_entropy_with_logits, the form bce_metrics_kernel evaluates (prepost.hip)
__device__ __forceinline__ float sce(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }

// Fixed-order tree over the workgroup's 256 partials of `v` in LDS scratch `red`; every thread returns the total.
template <class T>
__device__ __forceinline__ T block_tree_sum(T v, T* red) {
    const int tid = threadIdx.x;
    __syncthreads();   // (the scratch may still be read from an earlier sum)
    red[tid] = v;
    __syncthreads();
    for (int off = kRouteThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per problem: part[p][0..5] = sum_e w_e sce(x_e, y_e) / m_p, (TP + TN) / m_p, TP, FP, TN, FN.  A thread sums
// its edges tid, tid + 256, ... in that order (the terms are fp32, their running sum fp64), then the tree.
__global__ __launch_bounds__(kRouteThreads) void edge_bce_kernel(const float* __restrict__ logits,
                                                                 const float* __restrict__ marks,
                                                                 const int32_t* __restrict__ seg, int B, float pos_weight,
                                                                 float scale, float* __restrict__ dlogit,
                                                                 float* __restrict__ part) {
    __shared__ double red_f[kRouteThreads];
    __shared__ int red_i[kRouteThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int beg = seg[p], end = seg[p + 1], m = end - beg;
    float w_pos = pos_weight;
    if (pos_weight == 0.f) {   // balanced: (m - k) / max(k, 1), k the problem's marked edges
        int k = 0;
        for (int e = beg + tid; e < end; e += kRouteThreads) k += marks[e] != 0.f ? 1 : 0;
        k = block_tree_sum(k, red_i);
        w_pos = (float)(m - k) / (float)max(k, 1);
    }
    const float inv = 1.0f / ((float)B * (float)max(m, 1));
    double loss = 0.0;
    int tp = 0, fp = 0, tn = 0, fn = 0;
    for (int e = beg + tid; e < end; e += kRouteThreads) {
        const float x = logits[e], y = marks[e];
        const bool on = y != 0.f, yes = x > 0.f;
        const float w = on ? w_pos : 1.0f;
        loss += (double)(w * sce(x, y));
        tp += (yes && on) ? 1 : 0;
        fp += (yes && !on) ? 1 : 0;
        tn += (!yes && !on) ? 1 : 0;
        fn += (!yes && on) ? 1 : 0;
        if (dlogit) dlogit[e] = scale * w * (sigmoidf_(x) - y) * inv;
    }
    loss = block_tree_sum(loss, red_f);
    tp = block_tree_sum(tp, red_i);
    fp = block_tree_sum(fp, red_i);
    tn = block_tree_sum(tn, red_i);
    fn = block_tree_sum(fn, red_i);
    if (tid == 0) {
        float* o = part + 6 * (size_t)p;
        const double inv_m = m > 0 ? 1.0 / (double)m : 0.0;   // a problem without edges adds nothing
        o[0] = (float)(loss * inv_m);
        o[1] = (float)((double)(tp + tn) * inv_m);
        o[2] = (float)tp, o[3] = (float)fp, o[4] = (float)tn, o[5] = (float)fn;
    }
}

// Last stage: the problems' partials in problem order; loss and accuracy are means over the problems.
__global__ __launch_bounds__(64) void edge_bce_finish_kernel(const float* __restrict__ part, int B,
                                                             float* __restrict__ stats) {
    const int k = threadIdx.x;
    if (k >= 6) return;
    double s = 0.0;
    for (int p = 0; p < B; ++p) s += (double)part[6 * (size_t)p + k];
    stats[k] = (float)(k < 2 ? s / (double)B : s);
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_route_edge_marks(const int32_t* uv, const int32_t* seg, const int32_t* vseg, const int32_t* tours,
                                       const int32_t* tour_off, int B, int n_max, float* marks, int32_t* n_missing,
                                       int32_t* status, void* stream) {
    TSPGNN_REQUIRE(B >= 0, "route_edge_marks: B=%d", B);
    if (B == 0) return TSPGNN_OK;
    if (n_max > kRouteMaxN)
        return fail(TSPGNN_EUNSUPPORTED, "route_edge_marks: n_max=%d exceeds %d", n_max, kRouteMaxN);
    TSPGNN_REQUIRE(n_max >= kRouteMinN, "route_edge_marks: n_max=%d must be at least %d", n_max, kRouteMinN);
    TSPGNN_REQUIRE(uv && seg && vseg && tours && marks && n_missing && status, "route_edge_marks: null pointer");
    const size_t lds = sizeof(int32_t) * ((size_t)n_max + (size_t)((n_max + 31) >> 5));
    if (lds > 32 * 1024) {
        if (int rc = set_dynamic_lds(route_edge_marks_kernel, lds, "route_edge_marks", true)) return rc;
    }
    route_edge_marks_kernel<<<(unsigned)B, kRouteThreads, lds, as_stream(stream)>>>(uv, seg, vseg, tours, tour_off, n_max,
                                                                                   marks, n_missing, status);
    return launched("tspgnn_route_edge_marks");
}

extern "C" long long tspgnn_edge_bce_workspace_floats(int B) { return B > 0 ? 6ll * B : 0ll; }

extern "C" int tspgnn_edge_bce_f32(const float* logits, const float* marks, const int32_t* seg, int B, float pos_weight,
                                   float scale, float* dlogit, float* stats, float* workspace, void* stream) {
    TSPGNN_REQUIRE(B >= 1, "edge_bce: B=%d must be at least 1", B);
    TSPGNN_REQUIRE(pos_weight >= 0.f, "edge_bce: pos_weight=%g must be positive, or 0 for the balanced rule",
                   (double)pos_weight);
    TSPGNN_REQUIRE(logits && marks && seg && stats && workspace, "edge_bce: null pointer");
    hipStream_t st = as_stream(stream);
    edge_bce_kernel<<<(unsigned)B, kRouteThreads, 0, st>>>(logits, marks, seg, B, pos_weight, scale, dlogit, workspace);
    if (int rc = launched("tspgnn_edge_bce_f32")) return rc;
    edge_bce_finish_kernel<<<1, 64, 0, st>>>(workspace, B, stats);
    return launched("tspgnn_edge_bce_f32");
}
