// Batches assembled on the device from a resident dataset (tspgnn/device_dataset.py):
//   tspgnn_gather_batch   one launch writes the seven arrays of a staged batch -- byte for byte what
//                         tspgnn_host_stage_batch (host_pack.hip) writes for the same instance list.
// What an instance contributes does not depend on the batch it lands in apart from two offsets and one factor: its edges
// in np.nonzero order with LOCAL endpoint ids, their fp32 weights, its local CSR by vertex and its fp64 tour cost sit in
// the dataset arrays once; a batch adds v_start[b] to the endpoints, e_start[b] to the edge ids, 2 e_start[b] to the row
// pointers and scales the cost by (1 -/+ dev).  So the kernel is a segmented copy with offsets: ~2.4 MB at 128 x n = 40,
// latency-bound, nothing to reuse.
//
// Mapping.  Three regions of whole 256-thread workgroups, so that the region is uniform over a workgroup:
//   edges     one thread per OUTPUT edge k in [0, M): uv[k] (8 B), wc[k] (8 B) and the CSR entries eid[2k], eid[2k+1]
//             (8 B; an instance's entries start at 2 e_start[b], so a pair never straddles two instances);
//   vertices  one thread per PAIR of row pointers 2j, 2j+1 in [0, N]: one 8-byte store (4 bytes for an odd tail);
//   slots     one thread per batch slot: labels, seg, n_edges (4-byte stores: B + 1 values in all).
// An element finds its slot by a binary search over e_start / v_start, which every workgroup copies to LDS first (8 (B+1)
// bytes; above kGatherLdsSlots slots the search reads the arrays where they are, L2-resident).  Work is shared out by
// output element, never by instance: a batch of one 32 640-edge instance beside an empty one loads every thread alike.
// Every store is a plain per-lane store to an address owned by exactly one thread; nothing is read back, no atomics, no
// inter-workgroup communication, one __syncthreads() that all threads of a workgroup reach.
#include "common.h"

namespace tspgnn {
namespace {

constexpr int kGatherThreads = 256;
constexpr int kGatherLdsSlots = 8191;   // 8 (B + 1) bytes of LDS <= 64 KiB, the limit of a launch that asks for no more

struct GatherArgs {
    const int32_t* inst;      // [I][4]: n, m, first edge, first vertex in the dataset arrays
    const int32_t* uv;        // [sum m][2] local endpoints
    const float* w;           // [sum m]
    const int32_t* rowptr;    // [sum (n + 1)]: instance i's n[i] + 1 local row pointers start at first vertex + i
    const int32_t* eid;       // [2 sum m] local edge ids, instance i's start at 2 * first edge
    const double* cost;       // [I]
    const int32_t* ids;       // [B]
    const int32_t* e_start;   // [B + 1]
    const int32_t* v_start;   // [B + 1]
    int B, M, N;
    double dev, target_cost;
    int use_target;
    int2* o_uv;
    int2* o_eid;
    int32_t* o_rowptr;
    float2* o_wc;
    float* o_labels;
    int32_t* o_seg;
    int32_t* o_ne;
    int edge_wgs, vertex_wgs;
};

// largest b in [0, B) with start[b] <= k, given start[0] = 0 <= k < start[B]: the slot that owns element k (empty slots
// repeat a value and are skipped: of equal starts the last one qualifies)
__device__ __forceinline__ int slot_of(const int32_t* start, int B, int k) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool kLds>
__global__ __launch_bounds__(kGatherThreads) void gather_batch_kernel(const GatherArgs a) {
    extern __shared__ int32_t gather_lds[];
    const int tid = threadIdx.x, B = a.B;
    const int32_t *es = a.e_start, *vs = a.v_start;
    if constexpr (kLds) {
        for (int i = tid; i <= B; i += kGatherThreads) {
            gather_lds[i] = a.e_start[i];
            gather_lds[B + 1 + i] = a.v_start[i];
        }
        __syncthreads();
        es = gather_lds;
        vs = gather_lds + B + 1;
    }
    int wg = blockIdx.x;
    if (wg < a.edge_wgs) {
        const int k = wg * kGatherThreads + tid;
        if (k >= a.M) return;
        const int b = slot_of(es, B, k);
        const int e0b = es[b], v0b = vs[b];
        const int id = a.ids[b];
        const long long src = (long long)a.inst[4 * id + 2] + (k - e0b);
        const int2 ends = reinterpret_cast<const int2*>(a.uv)[src];
        const int2 ce = reinterpret_cast<const int2*>(a.eid)[src];
        double c = a.target_cost;
        if (!a.use_target) {   // two roundings, as the host's (1.0 -/+ dev) * cost
            const double f = (b & 1) ? __dadd_rn(1.0, a.dev) : __dsub_rn(1.0, a.dev);
            c = __dmul_rn(f, a.cost[id]);
        }
        a.o_uv[k] = make_int2(ends.x + v0b, ends.y + v0b);
        a.o_eid[k] = make_int2(ce.x + e0b, ce.y + e0b);
        a.o_wc[k] = make_float2(a.w[src], (float)c);
        return;
    }
    wg -= a.edge_wgs;
    if (wg < a.vertex_wgs) {
        const int v = 2 * (wg * kGatherThreads + tid);
        if (v > a.N) return;
        int32_t val[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int x = v + s;
            val[s] = 2 * a.M;      // rowptr[N]; x == N + 1 is not stored
            if (x < a.N) {
                const int b = slot_of(vs, B, x);
                const int id = a.ids[b];
                const long long src = (long long)a.inst[4 * id + 3] + id + (x - vs[b]);
                val[s] = a.rowptr[src] + 2 * es[b];
            }
        }
        if (v + 1 <= a.N)
            reinterpret_cast<int2*>(a.o_rowptr)[v >> 1] = make_int2(val[0], val[1]);
        else
            a.o_rowptr[v] = val[0];
        return;
    }
    wg -= a.vertex_wgs;
    const int b = wg * kGatherThreads + tid;
    if (b > B) return;
    a.o_seg[b] = es[b];
    if (b < B) {
        a.o_labels[b] = (float)(b & 1);
        a.o_ne[b] = es[b + 1] - es[b];
    }
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_gather_batch(const int32_t* inst, const int32_t* uv, const float* w, const int32_t* rowptr,
                                   const int32_t* eid, const double* cost, const int32_t* ids, const int32_t* e_start,
                                   const int32_t* v_start, int B, int M, int N, double dev, int use_target,
                                   double target_cost, unsigned char* dst, const long long* off, void* stream) {
    TSPGNN_REQUIRE(B >= 0 && M >= 0 && N >= 0, "gather_batch: B=%d M=%d N=%d", B, M, N);
    if (B == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(inst && uv && w && rowptr && eid && ids && e_start && v_start && dst && off && (use_target || cost),
                   "gather_batch: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 8 == 0, "gather_batch: the destination is not 8-byte aligned");
    for (int k = 0; k < 7; ++k)
        TSPGNN_REQUIRE(off[k] >= 0 && off[k] % 8 == 0, "gather_batch: offset %d (%lld) is not a non-negative multiple of 8",
                       k, off[k]);
    if (M == 0) return TSPGNN_OK;   // nothing to launch: a batch without edges is all offsets, which the caller has
    GatherArgs a;
    a.inst = inst, a.uv = uv, a.w = w, a.rowptr = rowptr, a.eid = eid, a.cost = cost;
    a.ids = ids, a.e_start = e_start, a.v_start = v_start;
    a.B = B, a.M = M, a.N = N, a.dev = dev, a.target_cost = target_cost, a.use_target = use_target != 0;
    a.o_uv = reinterpret_cast<int2*>(dst + off[0]);
    a.o_eid = reinterpret_cast<int2*>(dst + off[1]);
    a.o_rowptr = reinterpret_cast<int32_t*>(dst + off[2]);
    a.o_wc = reinterpret_cast<float2*>(dst + off[3]);
    a.o_labels = reinterpret_cast<float*>(dst + off[4]);
    a.o_seg = reinterpret_cast<int32_t*>(dst + off[5]);
    a.o_ne = reinterpret_cast<int32_t*>(dst + off[6]);
    const auto wgs = [](long long items) { return (int)((items + kGatherThreads - 1) / kGatherThreads); };
    a.edge_wgs = wgs(M);
    a.vertex_wgs = wgs(((long long)N + 2) / 2);   // pairs covering the N + 1 row pointers
    const unsigned grid = (unsigned)(a.edge_wgs + a.vertex_wgs + wgs((long long)B + 1));
    hipStream_t st = as_stream(stream);
    if (B <= kGatherLdsSlots)
        gather_batch_kernel<true><<<grid, kGatherThreads, 2 * ((size_t)B + 1) * sizeof(int32_t), st>>>(a);
    else
        gather_batch_kernel<false><<<grid, kGatherThreads, 0, st>>>(a);
    return launched("tspgnn_gather_batch");
}
