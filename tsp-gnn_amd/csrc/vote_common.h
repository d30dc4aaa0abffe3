// What the kernels that read a resident batch's per-edge votes share (tour_decode.hip, tour_beam.hip, tour_guided.hip;
// include/tspgnn.h, "tours from the edge votes", states the layout, the pair rule and the key): the view of one instance
// with its endpoint rule, the ordered fp32 key, the tail of a decoded tour and the entry points' first checks.
#pragma once
#include "tour_common.h"

namespace tspgnn {
namespace {

constexpr int kVoteMaxN = 256;   // vertices per instance, every vote kernel's limit (MAX_N of tspgnn/decode.py)

// Instance `inst` of the batch: n vertices from global id v0, the m edges e = 0 .. m-1 from global edge id e0; uv the
// batch's endpoint ids, ep those of edge 0 of the instance.
struct VoteInstance {
    int v0, n;
    long long e0, m;
    const int32_t *uv, *ep;

    __device__ __forceinline__ VoteInstance(const int32_t* uv_, const int32_t* seg, const int32_t* vseg, int inst)
        : v0(vseg[inst]), n(vseg[inst + 1] - v0), e0(seg[inst]), m((long long)seg[inst + 1] - e0), uv(uv_),
          ep(uv_ + 2 * e0) {}

    // f(a, b) with the local endpoints of edge e in [0, m), when the edge joins them: only when both lie in [0, n) and
    // differ.  (A callback, not a predicate: the body then sits under the same branches as a spelled-out test, and the
    // kernels compile to the code they had.)
    template <class F>
    __device__ __forceinline__ void with_ends(long long e, F&& f) const {
        const int a = ep[2 * e] - v0, b = ep[2 * e + 1] - v0;
        if (a >= 0 && a < n && b >= 0 && b < n && a != b) f(a, b);
    }

    // The rule read through the vertex CSR's row of local vertex x in [0, n): whether the row's global edge id g is an
    // edge of this instance that joins x to another vertex, y.
    __device__ __forceinline__ bool other_end(int g, int x, int& y) const {
        if (g < (int)e0 || g >= (int)(e0 + m)) return false;
        const int a = uv[2 * (long long)g] - v0, b = uv[2 * (long long)g + 1] - v0;
        y = a == x ? b : b == x ? a : -1;
        return y >= 0 && y < n && y != x;
    }
};

// The order-preserving uint32 image of an fp32 value: all bits flipped when the sign bit is set, else the sign bit set,
// so -0.0 < +0.0 and -inf is the lowest number; a NaN gets `nan`.
constexpr uint32_t kNanLowest = 0u, kNanHighest = 0xffffffffu;
__device__ __forceinline__ uint32_t ordered_key(float x, uint32_t nan) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return nan;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// The key the votes are ordered by: larger key = larger vote, a NaN below everything.
__device__ __forceinline__ uint32_t vote_key(float vote) { return ordered_key(vote, kNanLowest); }

// What an instance the host module never sends (n outside the kernel's range, m < 0) gets: no tour.
__device__ __forceinline__ void refuse_tour(float* cost, int32_t* n_missing) {
    *cost = __int_as_float(0x7fc00000);
    *n_missing = -1;
}

// One lane: the cost of a tour of n vertices whose pair k -- (tour[k], tour[k+1]), k = n - 1 the closing pair -- is an
// edge of weight w[k] iff is_edge(k), and the number of pairs that are not.  One running fp32 sum from 0 in tour order,
// additions only.
template <class IsEdge>
__device__ __forceinline__ float sum_tour_pairs(int n, IsEdge&& is_edge, const float* w, int& missing) {
    float cost = 0.f;
    missing = 0;
    for (int k = 0; k < n; ++k) {
        if (is_edge(k)) cost += w[k];
        else ++missing;
    }
    return cost;
}

// What every vote entry point checks first, in this order: B >= 0; B == 0, nothing to do (the caller returns TSPGNN_OK);
// n_max <= 256 and, at the same rank, a launch limit of the entry point's own (`limit_name`: value <= limit); n_max >= 4.
inline int vote_entry(const char* who, int B, int n_max, const char* limit_name = nullptr, int value = 0, int limit = 0) {
    TSPGNN_REQUIRE(B >= 0, "%s: B=%d", who, B);
    if (B == 0) return TSPGNN_OK;
    if (n_max > kVoteMaxN) return fail(TSPGNN_EUNSUPPORTED, "%s: n_max=%d exceeds %d", who, n_max, kVoteMaxN);
    if (limit_name && value > limit) return fail(TSPGNN_EUNSUPPORTED, "%s: %s=%d exceeds %d", who, limit_name, value, limit);
    TSPGNN_REQUIRE(n_max >= 4, "%s: n_max=%d must be at least 4", who, n_max);
    return TSPGNN_OK;
}

}  // namespace
}  // namespace tspgnn
