// tspgnn_vote_neighbors (tspgnn/decode.py): per-vertex candidate rows from the network's per-edge logits, the table
// tspgnn_tour_search_cand (tour_search.hip) descends over.  One workgroup per instance, reading the batch and the vertex
// CSR it carries: rowptr[N+1], eid row g = the ids of the edges that list global vertex g as an endpoint.
// include/tspgnn.h DEFINES the rows as a sequential process: the batch, the pair rule and the two keys under "tours from
// the edge votes", then this entry point's Row, Vote and Near.  A row depends on the instance, its votes and weights
// alone: never on n_max, on the other instances or on the launch.
//
// A wave takes the vertices wave, wave + waves, ...  Per vertex it resolves multi-edges in its own LDS array best_e[y]
// (atomic-min over the CSR row), then a lane holds the <= 4 neighbours lane + 64 j with their two keys in registers and
// the wave takes K arg-max rounds over (key, y) packed into one 64-bit word.  Lane s keeps slot s, so a row leaves in
// one store of K consecutive bytes.  No sort, no workspace, no communication between workgroups; every loop has a fixed
// trip count (the row length, K, n / waves).
#include "vote_common.h"

namespace tspgnn {
namespace {

constexpr int kGuideSlots = kVoteMaxN / kWave;   // neighbours a lane holds
constexpr int kGuideMaxK = 32;

// Wave-wide maximum of a 64-bit word; every lane gets it.
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

template <int NT>
__global__ __launch_bounds__(NT) void vote_neighbors_kernel(const float* __restrict__ vote, const int32_t* __restrict__ uv,
                                                            const float* __restrict__ wc, const int32_t* __restrict__ seg,
                                                            const int32_t* __restrict__ vseg,
                                                            const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ eid, int n_max, int k_vote,
                                                            int k_near, uint8_t* __restrict__ tab) {
    constexpr int kWaves = NT / kWave;
    __shared__ int s_best[kWaves][kVoteMaxN];
    const int inst = blockIdx.x;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const VoteInstance I(uv, seg, vseg, inst);
    const int v0 = I.v0, n = I.n;
    const int K = k_vote + k_near;
    if (n < 4 || n > n_max) {   // the host module never sends these: zero rows, and every LDS index stays in bounds
        const long long bytes = n > 0 ? (long long)n * K : 0;
        uint8_t* out = tab + (long long)v0 * K;
        for (long long k = threadIdx.x; k < bytes; k += NT) out[k] = 0;
        return;
    }
    int* best_e = s_best[wave];
    for (int x = wave; x < n; x += kWaves) {
        for (int y = lane; y < n; y += kWave) best_e[y] = INT_MAX;
        wave_sync();
        const int r0 = rowptr[v0 + x], r1 = rowptr[v0 + x + 1];
        for (int r = r0 + lane; r < r1; r += kWave) {
            const int e = eid[r];
            int y;
            if (I.other_end(e, x, y)) atomicMin(&best_e[y], e);
        }
        wave_sync();
        // this lane's neighbours: the arg-max words of the two phases, 0 = not a neighbour (or taken)
        unsigned long long kv[kGuideSlots], kw[kGuideSlots];
#pragma unroll
        for (int j = 0; j < kGuideSlots; ++j) {
            const int y = lane + j * kWave;
            const int e = y < n ? best_e[y] : INT_MAX;
            kv[j] = kw[j] = 0;
            if (e != INT_MAX) {
                const unsigned long long tie = 0xffffffffu - (unsigned)y;   // the smaller y wins a tie
                kv[j] = ((unsigned long long)vote_key(vote[e]) << 32) | tie;
                // the smallest weight makes the largest word
                kw[j] = ((unsigned long long)(~ordered_key(wc[2 * (long long)e], kNanHighest)) << 32) | tie;
            }
        }
        wave_sync();   // best_e is read: the next vertex may clear it
        int mine = x;
        for (int s = 0; s < K; ++s) {
            const bool by_w = s >= k_vote;
            unsigned long long m = 0;
#pragma unroll
            for (int j = 0; j < kGuideSlots; ++j) {
                const unsigned long long c = by_w ? kw[j] : kv[j];
                m = c > m ? c : m;
            }
            m = wave_max_u64(m);
            int y = x;
            if (m != 0) {   // wave-uniform
                y = (int)(0xffffffffu - (unsigned)(m & 0xffffffffu));
#pragma unroll
                for (int j = 0; j < kGuideSlots; ++j)
                    if (lane + j * kWave == y) kv[j] = kw[j] = 0;
            }
            if (lane == s) mine = y;
        }
        if (lane < K) tab[(long long)(v0 + x) * K + lane] = (uint8_t)mine;
    }
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_vote_neighbors(const float* vote, const int32_t* uv, const float* wc, const int32_t* seg,
                                     const int32_t* vseg, const int32_t* rowptr, const int32_t* eid, int B, int n_max,
                                     int k_vote, int k_near, uint8_t* tab, void* stream) {
    if (int rc = vote_entry("vote_neighbors", B, n_max)) return rc;
    if (B == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(k_vote >= 0 && k_near >= 0, "vote_neighbors: k_vote=%d, k_near=%d", k_vote, k_near);
    TSPGNN_REQUIRE(k_vote <= kGuideMaxK && k_near <= kGuideMaxK && k_vote + k_near >= 1 && k_vote + k_near <= kGuideMaxK,
                   "vote_neighbors: k_vote + k_near = %d + %d not in [1, %d]", k_vote, k_near, kGuideMaxK);
    TSPGNN_REQUIRE(vote && uv && wc && seg && vseg && rowptr && eid && tab, "vote_neighbors: null pointer");
    hipStream_t st = as_stream(stream);
    // the waves stride over the vertices, so the workgroup's size changes no row
    if (n_max <= 64)
        vote_neighbors_kernel<256><<<(unsigned)B, 256, 0, st>>>(vote, uv, wc, seg, vseg, rowptr, eid, n_max, k_vote, k_near,
                                                                tab);
    else
        vote_neighbors_kernel<1024><<<(unsigned)B, 1024, 0, st>>>(vote, uv, wc, seg, vseg, rowptr, eid, n_max, k_vote,
                                                                  k_near, tab);
    return launched("tspgnn_vote_neighbors");
}
