// Device and host helpers shared by the tour kernels (tour_search.hip, tour_baselines.hip): the two LDS layouts of an
// instance's weights, the counter-based generator, the wave reductions, the canonical write-out and the LDS budget.
#pragma once
#include "common.h"

#include <float.h>
#include <limits.h>

namespace tspgnn {
namespace {

constexpr int kMaxChains = 16;
constexpr size_t kLdsBytes = 160 * 1024;   // gfx950: LDS per workgroup, static and dynamic together

// Intra-wave LDS hand-off: lanes of one wave write, other lanes of the same wave read.  A wave executes its LDS
// operations in order; this only keeps the compiler from moving accesses across the point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The dense layout: row stride n | 1, odd, so a column read by 32 consecutive rows touches 32 distinct banks.
struct SquareW {
    static constexpr int kMaxN = 128;
    const float* w;
    int s;
    __host__ __device__ static size_t floats(int n) { return (size_t)n * (size_t)(n | 1); }
    __device__ static SquareW stage(float* lds, const float* src, int n, int tid, int nt) {
        const int s = n | 1;
        for (int e = tid; e < n * n; e += nt) lds[(e / n) * s + e % n] = src[e];
        return {lds, s};
    }
    __device__ __forceinline__ float operator()(int a, int b) const { return w[a * s + b]; }
};

// The packed strict upper triangle, row-major: w(a, b) = w[off(min) + max], off(r) = r (2n - 3 - r) / 2 - 1 (r (2n-3-r)
// is even).  Callers never ask for the diagonal, which the layout does not hold.
struct TriW {
    static constexpr int kMaxN = 256;
    const float* w;
    int k;   // 2n - 3
    __host__ __device__ static size_t floats(int n) { return (size_t)n * (size_t)(n - 1) / 2; }
    __device__ static TriW stage(float* lds, const float* src, int n, int tid, int nt) {
        const int m = n * (n - 1) / 2;
        for (int e = tid; e < m; e += nt) lds[e] = src[e];
        return {lds, 2 * n - 3};
    }
    __device__ __forceinline__ float operator()(int a, int b) const {
        const int lo = min(a, b), hi = max(a, b);
        return w[hi - 1 + (int)(__umul24((unsigned)lo, (unsigned)(k - lo)) >> 1)];
    }
};

// The move codes of tour_search.hip keep a tour position in 8 bits, and a lane owns kMaxN / 64 vertices (one_tree,
// nearest_neighbor).
static_assert(SquareW::kMaxN - 1 <= 0xff && TriW::kMaxN - 1 <= 0xff, "move codes hold positions 0..255");
static_assert(SquareW::kMaxN % kWave == 0 && TriW::kMaxN % kWave == 0, "one_tree's vertices per lane");

// Counter-based generator: splitmix64 finaliser over (seed, instance index in the caller's list, chain, kick, draw).
// Nothing depends on blockIdx, so results do not depend on how the caller chunks its batch.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t draw(uint64_t seed, long long inst, int chain, int kick, int k) {
    uint64_t h = mix64(seed ^ mix64((uint64_t)inst));
    h = mix64(h ^ (((uint64_t)(unsigned)chain << 32) | (unsigned)kick));
    return mix64(h ^ (uint64_t)(unsigned)k);
}

// Wave-wide argmin of (value, code), ties to the smaller code.  The butterfly leaves every lane with the same pair.
template <typename T>
__device__ __forceinline__ void wave_argmin(T& v, int& c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T ov = __shfl_xor(v, off);
        const int oc = __shfl_xor(c, off);
        if (ov < v || (ov == v && oc < c)) {
            v = ov;
            c = oc;
        }
    }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);   // commutative pairs: every lane gets the same sum
    return v;
}

template <class WA>
__device__ __forceinline__ float tour_cost(const WA& W, const int* t, int n, int lane) {
    float acc = 0.f;
    for (int k = lane; k < n; k += kWave) acc += W(t[k], t[k + 1 < n ? k + 1 : 0]);
    return wave_sum(acc);
}

// One wave writes tour t (LDS) to out in canonical form: starts at vertex 0, tour[1] < tour[n-1].
__device__ __forceinline__ void write_canonical(const int* t, int n, int32_t* out, int lane) {
    int p0 = 0;
    for (int k = lane; k < n; k += kWave)
        if (t[k] == 0) p0 = k;
    p0 = wave_sum(p0);   // exactly one lane holds the position of vertex 0
    const int nxt = t[p0 + 1 < n ? p0 + 1 : 0], prv = t[p0 > 0 ? p0 - 1 : n - 1];
    const bool fwd = nxt < prv;
    for (int k = lane; k < n; k += kWave) {
        int q = fwd ? p0 + k : p0 - k;
        if (q >= n) q -= n;
        if (q < 0) q += n;
        out[k] = t[q];
    }
}

template <class K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return TSPGNN_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e != hipSuccess) return fail((int)e, "tour kernels: hipFuncSetAttribute: %s", hipGetErrorString(e));
    return TSPGNN_OK;
}

// Static LDS of a chain kernel (per chain one float and one int: s_cost, s_tour); the dynamic part must fit beside it.
constexpr size_t kSearchStaticLds = kMaxChains * (sizeof(float) + sizeof(int));

// The chains that fit at n_max: the weights plus three tours of n_max int32 ids per chain.
template <class WA>
int chains_fit(int n_max) {
    const size_t free_bytes = kLdsBytes - kSearchStaticLds - WA::floats(n_max) * sizeof(float);
    const size_t c = free_bytes / ((size_t)3 * n_max * sizeof(int));
    return c < (size_t)kMaxChains ? (int)c : kMaxChains;
}

}  // namespace
}  // namespace tspgnn
