// Device and host helpers shared by the tour kernels (tour_search.hip, tour_baselines.hip, tour_exact.hip): the two LDS
// layouts of an instance's weights, the counter-based generator, the wave reductions, the canonical form and its
// write-out, the Held-Karp 1-tree with its subgradient ascent (the bound kernel and the branch and bound), the entry
// points' n_max check, the refusal of an instance the host never sends, the starting-tour check, the 2-exchange move, and
// the chain kernels' workspace in LDS with its budget and the chain winner.  What only the readers of the edge votes
// share sits on top of this header, in vote_common.h.
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

// Canonical form of a cyclic sequence of n vertices (starts at vertex 0, tour[1] < tour[n-1]): where its entry k sits in
// the sequence, p0 being the position of vertex 0 and fwd saying that p0's successor is smaller than its predecessor.
__device__ __forceinline__ int canonical_index(int p0, bool fwd, int k, int n) {
    int q = fwd ? p0 + k : p0 - k;
    if (q >= n) q -= n;
    if (q < 0) q += n;
    return q;
}

// The same for a sequence that starts at vertex 0 (p0 = 0), k in [1, n); entry 0 is entry 0.
__device__ __forceinline__ int canonical_index_from0(bool fwd, int k, int n) { return fwd ? k : n - k; }

// One wave writes tour t (LDS) to out in canonical form.
__device__ __forceinline__ void write_canonical(const int* t, int n, int32_t* out, int lane) {
    int p0 = 0;
    for (int k = lane; k < n; k += kWave)
        if (t[k] == 0) p0 = k;
    p0 = wave_sum(p0);   // exactly one lane holds the position of vertex 0
    const int nxt = t[p0 + 1 < n ? p0 + 1 : 0], prv = t[p0 > 0 ? p0 - 1 : n - 1];
    const bool fwd = nxt < prv;
    for (int k = lane; k < n; k += kWave) out[k] = t[canonical_index(p0, fwd, k, n)];
}

// Wave-wide minimum of an int; every lane gets it.
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

// ------------------------------------------------------------------------------------------------- Held-Karp 1-tree
// Edge classes of a branch-and-bound node (tour_exact.hip).  A 1-tree picks its edges by (rank, cost): rank 0 = forced,
// before any free edge (rank 1); a forbidden edge (rank 2) is never picked.  The classes never touch the costs.
constexpr int kEdgeFree = 0, kEdgeForced = 1, kEdgeForbidden = 2;

// No constraints (the bound kernel, the root node): every edge is free and the class code compiles away.
struct NoCons {
    static constexpr bool kActive = false;
    __device__ __forceinline__ int rank(int, int) const { return 1; }
};

// The n x n int8 class matrix of a node in LDS, row stride s bytes, symmetric.
struct LdsCons {
    static constexpr bool kActive = true;
    int8_t* c;
    int s;
    __device__ __forceinline__ int operator()(int a, int b) const { return c[a * s + b]; }
    __device__ __forceinline__ int rank(int a, int b) const {
        const int x = c[a * s + b];
        return x == kEdgeForced ? 0 : x == kEdgeFree ? 1 : 2;
    }
};

// Minimum 1-tree under the costs c(u,v) = W(u,v) + pi_u + pi_v, evaluated in T: Prim's tree on vertices 1..n-1 plus the two
// cheapest edges at vertex 0, both by (rank, cost) under the classes C.  Lane l owns the K vertices l, l+64, ... (pi[j] is
// vertex l + 64 j's).  Returns sum c(edges) - 2 sum pi; deg[] (LDS) gets the 1-tree degrees; *mag gets sum |c(edges)| +
// 2 sum |pi| (the scale of the rounding error).  Vertices past n take no part and add nothing to a lane's sums, so the
// result does not depend on K.  tp (LDS, optional) gets the tree's edges: (u, tp[u]) for u >= 2, (0, tp[0]) and (0, tp[1]).
// When the allowed edges hold no 1-tree (constraints only) the result is not below FLT_MAX; deg and tp are then partial.
template <typename T, int K, class WA, class CA>
__device__ T one_tree(const WA& W, const CA& C, int n, const T (&pi)[K], int lane, int* deg, T* mag, int* tp = nullptr) {
    const T inf = (T)FLT_MAX * (T)4;
    int v[K];
    bool ok[K], in[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        v[j] = lane + j * kWave;
        ok[j] = v[j] < n;
        if (ok[j]) deg[v[j]] = 0;
        in[j] = !ok[j] || v[j] <= 1;
    }
    wave_sync();
    const T pir = __shfl(pi[0], 1);
    T key[K];
    int par[K], rk[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        key[j] = in[j] ? inf : (T)W(1, v[j]) + pir + pi[j];
        par[j] = 1;
        rk[j] = 1;
        if constexpr (CA::kActive) {
            rk[j] = in[j] ? 2 : C.rank(1, v[j]);
            if (rk[j] == 2) key[j] = inf;
        }
    }
    T tree = 0, amag = 0;
    for (int step = 0; step < n - 2; ++step) {
        T k = inf;
        int who = INT_MAX;
        if constexpr (!CA::kActive) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (!in[j] && (j == 0 || key[j] < k)) {
                    k = key[j];
                    who = v[j];
                }
            }
        } else {
            int r = 2;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (!in[j] && (rk[j] < r || (rk[j] == r && key[j] < k))) {
                    r = rk[j];
                    k = key[j];
                    who = v[j];
                }
            }
            const int rmin = wave_min(r);
            if (rmin == 2) {   // wave-uniform: the allowed edges do not connect 1..n-1
                *mag = 0;
                return inf;
            }
            if (r != rmin) {
                k = inf;
                who = INT_MAX;
            }
        }
        wave_argmin(k, who);
        const int u = who;
        tree += k;
        amag += k < 0 ? -k : k;
        T pu = __shfl(pi[0], u & (kWave - 1));
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (v[j] == u) {
                in[j] = true;
                atomicAdd(&deg[par[j]], 1);
                atomicAdd(&deg[u], 1);
                if (tp) tp[u] = par[j];
            }
            if (j > 0) {
                const T x = __shfl(pi[j], u & (kWave - 1));
                if (u / kWave == j) pu = x;
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (!in[j]) {
                if constexpr (!CA::kActive) {
                    const T c = (T)W(u, v[j]) + pu + pi[j];
                    if (c < key[j]) {
                        key[j] = c;
                        par[j] = u;
                    }
                } else {
                    const int r = C.rank(u, v[j]);
                    const T c = (T)W(u, v[j]) + pu + pi[j];
                    if (r < 2 && (r < rk[j] || (r == rk[j] && c < key[j]))) {
                        rk[j] = r;
                        key[j] = c;
                        par[j] = u;
                    }
                }
            }
        }
    }
    // the two cheapest edges at vertex 0 (pi_0 is lane 0's pi[0]); per lane the smallest, ties to the smaller vertex
    const T piz = __shfl(pi[0], 0);
    T c[K];
#pragma unroll
    for (int j = 0; j < K; ++j) c[j] = (ok[j] && v[j] >= 1) ? (T)W(0, v[j]) + piz + pi[j] : inf;
    T m1, m2;
    int e1, e2;
    if constexpr (!CA::kActive) {
        m1 = c[0];
        e1 = v[0];
#pragma unroll
        for (int j = 1; j < K; ++j) {
            if (c[j] < m1) {
                m1 = c[j];
                e1 = v[j];
            }
        }
        wave_argmin(m1, e1);
        m2 = inf;
        e2 = INT_MAX;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (v[j] != e1 && c[j] < m2) {
                m2 = c[j];
                e2 = v[j];
            }
        }
        if (m2 == inf) e2 = INT_MAX;
        wave_argmin(m2, e2);
    } else {
        int r0[K];
#pragma unroll
        for (int j = 0; j < K; ++j) r0[j] = (ok[j] && v[j] >= 1) ? C.rank(0, v[j]) : 2;
        e1 = INT_MAX;
#pragma unroll
        for (int pick = 0; pick < 2; ++pick) {   // the first edge, then the second among the rest
            int r = 2, e = INT_MAX;
            T m = inf;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (v[j] != e1 && (r0[j] < r || (r0[j] == r && c[j] < m))) {
                    r = r0[j];
                    m = c[j];
                    e = v[j];
                }
            }
            const int rmin = wave_min(r);
            if (rmin == 2) {   // wave-uniform: vertex 0 has fewer than two allowed edges
                *mag = 0;
                return inf;
            }
            if (r != rmin) {
                m = inf;
                e = INT_MAX;
            }
            wave_argmin(m, e);
            if (pick == 0) {
                m1 = m;
                e1 = e;
            } else {
                m2 = m;
                e2 = e;
            }
        }
    }
    wave_sync();
    if (lane == 0) {
        deg[0] = 2;
        atomicAdd(&deg[e1], 1);
        atomicAdd(&deg[e2], 1);
        if (tp) {
            tp[0] = e1;
            tp[1] = e2;
        }
    }
    T psum = (ok[0] ? pi[0] : (T)0) + (ok[1] ? pi[1] : (T)0);
    T pmag = (ok[0] ? (pi[0] < 0 ? -pi[0] : pi[0]) : (T)0) + (ok[1] ? (pi[1] < 0 ? -pi[1] : pi[1]) : (T)0);
#pragma unroll
    for (int j = 2; j < K; ++j) {
        if (ok[j]) {
            psum += pi[j];
            pmag += pi[j] < 0 ? -pi[j] : pi[j];
        }
    }
    psum = wave_sum(psum);
    pmag = wave_sum(pmag);
    wave_sync();
    *mag = amag + (m1 < 0 ? -m1 : m1) + (m2 < 0 ? -m2 : m2) + 2 * pmag;
    return tree + m1 + m2 - 2 * psum;
}

// Subgradient ascent on the 1-tree bound from the multipliers pi: at most `iters` steps, each a 1-tree under pi and a
// Polyak step lambda * (ub - L) / |g|^2 along g = degree - 2, lambda = 2 halved after 8 steps without a new best.  Returns
// the best fp32 value and leaves its multipliers in bp; a value not below FLT_MAX says that the classes allow no 1-tree.
template <int K, class WA, class CA>
__device__ float ascend(const WA& W, const CA& C, int n, float ub, int iters, int lane, int* deg, float (&pi)[K],
                        float (&bp)[K]) {
    float best = -FLT_MAX, lambda = 2.f, mag;
#pragma unroll
    for (int j = 0; j < K; ++j) bp[j] = pi[j];
    int stall = 0;
    for (int it = 0; it < iters; ++it) {
        const float L = one_tree<float>(W, C, n, pi, lane, deg, &mag);
        if constexpr (CA::kActive) {
            if (!(L < FLT_MAX)) return L;
        }
        if (L > best) {
            best = L;
#pragma unroll
            for (int j = 0; j < K; ++j) bp[j] = pi[j];
            stall = 0;
        } else if (++stall >= 8) {   // halving schedule: no improvement in 8 steps
            lambda *= 0.5f;
            stall = 0;
        }
        int g[K], g2 = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            g[j] = lane + j * kWave < n ? deg[lane + j * kWave] - 2 : 0;
            g2 += g[j] * g[j];
        }
        const int gg = wave_sum(g2);
        if (gg == 0 || lambda < 1e-6f) break;   // the 1-tree is a tour (optimal), or the step has vanished
        const float gap = fmaxf(ub - L, 1e-4f * fabsf(L) + 1e-30f);
        const float t = lambda * gap / (float)gg;   // Polyak step towards the upper bound
#pragma unroll
        for (int j = 0; j < K; ++j) pi[j] += t * (float)g[j];
        wave_sync();
    }
    return best;
}

// The 1-tree of the multipliers bp again from scratch in fp64 (the fp32 Prim of the ascent may pick a non-minimal tree
// under rounding), less a margin for the fp64 rounding of the c(u,v) sums and the accumulation: a lower bound on every
// tour that the classes allow, rounding included.  deg and tp as one_tree; not below FLT_MAX when there is no 1-tree.
template <int K, class WA, class CA>
__device__ double rebuilt_bound(const WA& W, const CA& C, int n, const float (&bp)[K], int lane, int* deg,
                                int* tp = nullptr) {
    double dpi[K], dmag;
#pragma unroll
    for (int j = 0; j < K; ++j) dpi[j] = (double)bp[j];
    const double L = one_tree<double>(W, C, n, dpi, lane, deg, &dmag, tp);
    return L - 8.0 * (double)n * DBL_EPSILON * dmag;
}

template <class K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return TSPGNN_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e != hipSuccess) return fail((int)e, "tour kernels: hipFuncSetAttribute: %s", hipGetErrorString(e));
    return TSPGNN_OK;
}

// What every tour entry point checks of n_max, in this order: the layout's limit, then the smallest instance.
template <class WA>
int check_layout(const char* what, int n_max) {
    if (n_max > WA::kMaxN) return fail(TSPGNN_EUNSUPPORTED, "%s: n_max=%d exceeds %d", what, n_max, WA::kMaxN);
    TSPGNN_REQUIRE(n_max >= 4, "%s: n_max=%d must be at least 4", what, n_max);
    return TSPGNN_OK;
}

// An instance the host never sends (n outside [4, n_max]) is refused before the first LDS access, which keeps every LDS
// index in bounds: one thread puts a NaN in place of its cost, or of its bound, and nothing else is written.  (The vote
// kernels' form is vote_common.h's refuse_tour.)
__device__ __forceinline__ bool never_sent(int n, int n_max) { return n < 4 || n > n_max; }
__device__ __forceinline__ void refuse(float* cost) { *cost = __int_as_float(0x7fc00000); }
__device__ __forceinline__ void refuse(double* lb) { *lb = __longlong_as_double(0x7ff8000000000000ll); }

// One wave copies n vertex ids from global memory into the LDS tour t and says whether they are a permutation of
// 0..n-1 (cnt: n ints of LDS scratch).  The callers take every later LDS index from t: on "no" they replace or drop it.
__device__ __forceinline__ bool load_permutation(const int32_t* src, int* t, int* cnt, int n, int lane) {
    for (int k = lane; k < n; k += kWave) cnt[k] = 0;
    wave_sync();
    int bad = 0;
    for (int k = lane; k < n; k += kWave) {
        const int v = src[k];
        t[k] = v;
        if (v < 0 || v >= n) bad = 1;
        else atomicAdd(&cnt[v], 1);
    }
    wave_sync();
    for (int k = lane; k < n; k += kWave) bad |= cnt[k] != 1;
    return wave_sum(bad) == 0;
}

// The 2-exchange move (i, j) of tour t, i <= j: reverse positions i+1..j.  It is a move when i + 1 < j <= n - 1 and the
// segment is not the whole cycle; f(d) then gets its fp32 cost change.  (A callback, as vote_common.h's with_ends: the
// body sits under the same branches as a spelled-out test.)
template <class WA, class F>
__device__ __forceinline__ void two_exchange(const WA& W, const int* t, int n, int i, int j, F&& f) {
    if (j > i + 1 && !(i == 0 && j == n - 1)) {
        const int a = t[i], b = t[i + 1], c = t[j], e = t[j + 1 < n ? j + 1 : 0];
        f((W(a, c) + W(b, e)) - (W(a, b) + W(c, e)));
    }
}

// ------------------------------------------------------------------------------------------------ chain workspace
// A chain kernel (the searches, nearest neighbour, the annealing) runs one workgroup per instance and one wave64 per
// chain.  Its static LDS is what the chains post for the pick of the winner: a cost and a tag (chain_winner below: the
// tie-break; the search: where the chain's best tour lies).
struct ChainPosts {
    float cost[kMaxChains];
    int tag[kMaxChains];
};
static_assert(sizeof(ChainPosts) == kMaxChains * (sizeof(float) + sizeof(int)), "the static LDS beside ChainLds::bytes()");

// Its dynamic LDS -- THE statement of the layout (include/tspgnn.h and DESIGN.md §12 give the byte formula):
//   the weights, WA::floats(n_max) fp32;
//   per chain three tours of n_max int32 vertex ids;
//   with a candidate table (neighbors > 0) the workgroup's byte table [n_max][neighbors], then per chain a byte position
//   array [n_max].
// Together with ChainPosts it must fit kLdsBytes.  The carve uses n_max, never an instance's own n.
constexpr int kMaxNeighbors = 32;
template <class WA>
struct ChainLds {
    float* lds;                      // the workgroup's dynamic LDS (host: null)
    int n_max, chains, neighbors;    // neighbors = 0: no table, no positions

    static size_t weight_bytes(int n_max) { return WA::floats(n_max) * sizeof(float); }
    static size_t chain_bytes(int n_max, int neighbors) { return (size_t)3 * n_max * sizeof(int) + (neighbors ? n_max : 0); }
    // the dynamic LDS bytes of a launch
    size_t bytes() const {
        return weight_bytes(n_max) + (size_t)n_max * neighbors + (size_t)chains * chain_bytes(n_max, neighbors);
    }
    // the chains that fit at n_max, kMaxChains at the most
    static int fit(int n_max, int neighbors) {
        const size_t free_bytes = kLdsBytes - sizeof(ChainPosts) - weight_bytes(n_max) - (size_t)n_max * (size_t)neighbors;
        const size_t c = free_bytes / chain_bytes(n_max, neighbors);
        return c < (size_t)kMaxChains ? (int)c : kMaxChains;
    }

    __device__ __forceinline__ int* tour(int chain, int slot) const {
        return reinterpret_cast<int*>(lds + WA::floats(n_max)) + (chain * 3 + slot) * n_max;
    }
    __device__ __forceinline__ uint8_t* table() const { return reinterpret_cast<uint8_t*>(tour(chains, 0)); }
    __device__ __forceinline__ uint8_t* positions(int chain) const { return table() + n_max * neighbors + chain * n_max; }
};

// The chain winner of nearest neighbour and the annealing.  Every wave of the workgroup calls this once: its chain's best
// tour is tour 1 of its workspace, of fp32 cost `cost`.  Wave 0 takes the smallest (cost, tie), equal pairs to the lower
// chain, and writes that tour to tour_out in canonical form and its cost to *cost_out.  (The search keeps its own pick:
// its best tour is any of the chain's three, and this routine in its place cost the full scan 1.6 % at n = 200,
// profiles/chain_refactor_ab.txt.)
template <class WA>
__device__ __forceinline__ void chain_winner(const ChainLds<WA>& ws, ChainPosts& post, int wave, int lane, float cost,
                                             int tie, int n, int32_t* tour_out, float* cost_out) {
    if (lane == 0) {
        post.cost[wave] = cost;
        post.tag[wave] = tie;
    }
    __syncthreads();
    if (wave != 0) return;
    float bc = post.cost[0];
    int bw = 0;
    for (int c = 1; c < ws.chains; ++c) {
        if (post.cost[c] < bc || (post.cost[c] == bc && post.tag[c] < post.tag[bw])) {
            bc = post.cost[c];
            bw = c;
        }
    }
    write_canonical(ws.tour(bw, 1), n, tour_out, lane);
    if (lane == 0) *cost_out = bc;
}

}  // namespace
}  // namespace tspgnn
