// Batched TSP tour labelling (tspgnn/dataset.py, the counterpart of the reference's Concorde call in dataset.py:9-50):
//   tspgnn_tour_search       multi-start iterated local search (2-opt + Or-opt, double-bridge kicks), one workgroup per
//                            instance, one wave64 per chain, the instance's weight matrix resident in LDS;
//   tspgnn_tour_lower_bound  the Held-Karp 1-tree bound by subgradient ascent, one wave64 per instance, the final 1-tree
//                            re-evaluated in fp64 so that the reported value is a lower bound under rounding.
// Both are issue-bound on LDS reads and VALU work: an instance reads its n*n weights from memory once.
//
// Termination: every loop below has a fixed trip-count bound.  A descent accepts a move only on a strict improvement of
// more than kEpsRel * cost / n and makes at most 4 n^2 moves; the kick and subgradient counts are arguments.  There is no
// inter-workgroup communication.
#include "common.h"

#include <float.h>
#include <limits.h>

namespace tspgnn {
namespace {

constexpr int kMaxN = 128;
constexpr int kMaxChains = 16;
constexpr float kEpsRel = 1e-6f;   // a move must gain more than kEpsRel * (cost / n): ~16 ulp of a mean edge

// Intra-wave LDS hand-off: lanes of one wave write, other lanes of the same wave read.  A wave executes its LDS
// operations in order; this only keeps the compiler from moving accesses across the point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Row stride of the LDS weight matrix: odd, so a column read by 32 consecutive rows touches 32 distinct banks.
__device__ __forceinline__ int lds_stride(int n) { return n | 1; }

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

__device__ __forceinline__ float tour_cost(const float* W, int s, const int* t, int n, int lane) {
    float acc = 0.f;
    for (int k = lane; k < n; k += kWave) acc += W[t[k] * s + t[k + 1 < n ? k + 1 : 0]];
    return wave_sum(acc);
}

// Move codes: bit 30 = Or-opt; Or-opt: bit 29 = reversed segment, bits 26..27 = segment length, bits 8..15 = segment
// start position i, bits 0..7 = insertion position p; 2-opt: bits 8..15 = i, bits 0..7 = j.
constexpr int kOrOpt = 1 << 30;

// Positions (i, j) of an n x n enumeration strided by the wave: lane starts at lane, steps by 64.
struct Strider {
    int i, j, q, r, n;
    __device__ Strider(int n_, int lane) : i(lane / n_), j(lane % n_), q(kWave / n_), r(kWave % n_), n(n_) {}
    __device__ __forceinline__ void step() {
        j += r;
        i += q;
        if (j >= n) {
            j -= n;
            ++i;
        }
    }
};

// Best-improvement descent on tour *t (scratch *u; the two are swapped per applied move).  Returns the tour's cost.
__device__ float descend(const float* W, int s, int*& t, int*& u, int n, int lane) {
    float cost = tour_cost(W, s, t, n, lane);
    const int cap = 4 * n * n;
    for (int mv = 0; mv < cap; ++mv) {
        float best = FLT_MAX;
        int code = INT_MAX;
        // 2-opt: reverse positions i+1..j (0 <= i, i+1 < j <= n-1, not the whole cycle)
        for (Strider p(n, lane); p.i < n; p.step()) {
            const int i = p.i, j = p.j;
            if (j > i + 1 && !(i == 0 && j == n - 1)) {
                const int a = t[i], b = t[i + 1], c = t[j], e = t[j + 1 < n ? j + 1 : 0];
                const float d = (W[a * s + c] + W[b * s + e]) - (W[a * s + b] + W[c * s + e]);
                const int cd = (i << 8) | j;
                if (d < best || (d == best && cd < code)) {
                    best = d;
                    code = cd;
                }
            }
        }
        // Or-opt: move the segment t[i..i+L-1] (cyclic) between t[p] and t[p+1], either orientation
        for (int L = 1; L <= 3 && L <= n - 3; ++L) {
            for (Strider p(n, lane); p.i < n; p.step()) {
                const int i = p.i, q = p.j;
                int rel = q - i;
                if (rel < 0) rel += n;
                if (rel < L || rel > n - 2) continue;
                int ie = i + L - 1, in = i + L, ip = i - 1, q1 = q + 1;
                if (ie >= n) ie -= n;
                if (in >= n) in -= n;
                if (ip < 0) ip += n;
                if (q1 >= n) q1 -= n;
                const int prev = t[ip], s0 = t[i], sl = t[ie], nx = t[in], a = t[q], b = t[q1];
                const float gain = W[prev * s + nx] - (W[prev * s + s0] + W[sl * s + nx]);
                const float ab = W[a * s + b];
                const float fwd = (W[a * s + s0] + W[sl * s + b]) - ab;
                const float rev = (W[a * s + sl] + W[s0 * s + b]) - ab;
                const bool use_rev = L > 1 && rev < fwd;
                const float d = gain + (use_rev ? rev : fwd);
                const int cd = kOrOpt | (use_rev ? 1 << 29 : 0) | (L << 26) | (i << 8) | q;
                if (d < best || (d == best && cd < code)) {
                    best = d;
                    code = cd;
                }
            }
        }
        wave_argmin(best, code);
        if (!(best < -kEpsRel * cost / (float)n)) break;   // wave-uniform: every lane holds the same pair
        const int i = (code >> 8) & 0xff, j = code & 0xff;
        if (!(code & kOrOpt)) {
            for (int k = lane; k < n; k += kWave) u[k] = (k <= i || k > j) ? t[k] : t[i + 1 + j - k];
        } else {
            const int L = (code >> 26) & 3, rv = (code >> 29) & 1;
            int rel = j - i;
            if (rel < 0) rel += n;
            const int A = rel - L + 1;   // t[i+L .. p] come first, then the segment, then t[p+1 .. i-1]
            for (int k = lane; k < n; k += kWave) {
                int src;
                if (k < A) src = i + L + k;
                else if (k < A + L) src = i + (rv ? L - 1 - (k - A) : k - A);
                else src = i + k;
                u[k] = t[src % n];
            }
        }
        wave_sync();
        int* x = t;
        t = u;
        u = x;
        cost = tour_cost(W, s, t, n, lane);
    }
    return cost;
}

// dst = double-bridge kick of src: cut at positions 1 <= p1 < p2 < p3 <= n-1, A B C D -> A C B D.  n >= 4.
__device__ void double_bridge(const int* src, int* dst, int n, uint64_t r, int lane) {
    int x1 = 1 + (int)((r & 0xffffffull) % (unsigned)(n - 1));
    int x2 = 1 + (int)(((r >> 24) & 0xffffffull) % (unsigned)(n - 2));
    int x3 = 1 + (int)(((r >> 48) & 0xffffull) % (unsigned)(n - 3));
    if (x2 >= x1) ++x2;                       // three distinct values of [1, n-1]
    const int lo = x1 < x2 ? x1 : x2, hi = x1 < x2 ? x2 : x1;
    if (x3 >= lo) ++x3;
    if (x3 >= hi) ++x3;
    const int p1 = min(lo, x3), p3 = max(hi, x3), p2 = lo + hi + x3 - p1 - p3;
    const int C = p3 - p2;
    for (int k = lane; k < n; k += kWave) {
        int q;
        if (k < p1 || k >= p3) q = k;
        else if (k < p1 + C) q = p2 + (k - p1);
        else q = p1 + (k - p1 - C);
        dst[k] = src[q];
    }
    wave_sync();
}

__global__ __launch_bounds__(kWave* kMaxChains) void tour_search_kernel(
    const float* __restrict__ Wg, const long long* __restrict__ w_off, const int* __restrict__ n_arr,
    const int32_t* __restrict__ init, const long long* __restrict__ t_off, const long long* __restrict__ index, int n_max,
    int kicks, unsigned long long seed, int32_t* __restrict__ tours, float* __restrict__ costs) {
    extern __shared__ float lds[];
    __shared__ float s_cost[kMaxChains];
    __shared__ int s_tour[kMaxChains];
    const int inst = blockIdx.x;
    const long long gi = index ? index[inst] : inst;
    const int n = n_arr[inst];
    const int chains = blockDim.x / kWave;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (n < 4 || n > n_max) {   // the host never sends these; a defensive no-op keeps every LDS index in bounds
        if (threadIdx.x == 0) costs[inst] = __int_as_float(0x7fc00000);
        return;
    }
    const int s = lds_stride(n);
    const float* W = lds;
    {
        const float* src = Wg + w_off[inst];
        for (int e = threadIdx.x; e < n * n; e += blockDim.x) lds[(e / n) * s + e % n] = src[e];
    }
    // per chain: three tours of n vertex ids (current, work, scratch) after the matrix
    int* base = reinterpret_cast<int*>(lds + n_max * lds_stride(n_max)) + wave * 3 * n_max;
    int* cur = base;
    int* work = base + n_max;
    int* scr = base + 2 * n_max;
    __syncthreads();

    // starting tour: chain 0 takes init_tours when given and a permutation of 0..n-1; otherwise Fisher-Yates
    bool have = false;
    if (wave == 0 && init) {
        const int32_t* it = init + t_off[inst];
        for (int k = lane; k < n; k += kWave) scr[k] = 0;
        wave_sync();
        int bad = 0;
        for (int k = lane; k < n; k += kWave) {
            const int v = it[k];
            cur[k] = v;
            if (v < 0 || v >= n) bad = 1;
            else atomicAdd(&scr[v], 1);
        }
        wave_sync();
        for (int k = lane; k < n; k += kWave) bad |= scr[k] != 1;
        have = wave_sum(bad) == 0;
    }
    if (!have) {
        for (int k = lane; k < n; k += kWave) cur[k] = k;
        wave_sync();
        if (lane == 0) {
            for (int k = n - 1; k > 0; --k) {
                const int j = (int)(draw(seed, gi, wave, -1, k) % (unsigned)(k + 1));
                const int x = cur[k];
                cur[k] = cur[j];
                cur[j] = x;
            }
        }
        wave_sync();
    }
    float best = descend(W, s, cur, scr, n, lane);
    for (int kick = 0; kick < kicks; ++kick) {
        double_bridge(cur, work, n, draw(seed, gi, wave, kick, 0), lane);
        const float c = descend(W, s, work, scr, n, lane);
        if (c <= best) {   // no worse: accept (the chain's current tour is always its best)
            int* x = cur;
            cur = work;
            work = x;
            best = c;
        }
    }
    if (lane == 0) {
        s_cost[wave] = best;
        s_tour[wave] = (int)(cur - reinterpret_cast<int*>(lds));
    }
    __syncthreads();
    if (wave != 0) return;
    float bc = s_cost[0];
    int bw = 0;
    for (int c = 1; c < chains; ++c) {
        if (s_cost[c] < bc) {
            bc = s_cost[c];
            bw = c;
        }
    }
    const int* t = reinterpret_cast<const int*>(lds) + s_tour[bw];
    // canonical form: starts at vertex 0, tour[1] < tour[n-1]
    int p0 = 0;
    for (int k = lane; k < n; k += kWave)
        if (t[k] == 0) p0 = k;
    p0 = wave_sum(p0);   // exactly one lane holds the position of vertex 0
    const int nxt = t[p0 + 1 < n ? p0 + 1 : 0], prv = t[p0 > 0 ? p0 - 1 : n - 1];
    const bool fwd = nxt < prv;
    int32_t* out = tours + t_off[inst];
    for (int k = lane; k < n; k += kWave) {
        int q = fwd ? p0 + k : p0 - k;
        if (q >= n) q -= n;
        if (q < 0) q += n;
        out[k] = t[q];
    }
    if (lane == 0) costs[inst] = bc;
}

// ---------------------------------------------------------------------------------------------------------- lower bound

// Minimum 1-tree under the costs c(u,v) = W[u][v] + pi_u + pi_v, evaluated in T: Prim's tree on vertices 1..n-1 plus the two
// cheapest edges at vertex 0.  Lane l owns vertices l and l+64.  Returns sum c(edges) - 2 sum pi; deg[] (LDS) gets the
// 1-tree degrees; *mag gets sum |c(edges)| + 2 sum |pi| (the scale of the rounding error).
template <typename T>
__device__ T one_tree(const float* W, int s, int n, T pi0, T pi1, int lane, int* deg, T* mag) {
    const T inf = (T)FLT_MAX * (T)4;
    const int v0 = lane, v1 = lane + kWave;
    const bool ok0 = v0 < n, ok1 = v1 < n;
    if (ok0) deg[v0] = 0;
    if (ok1) deg[v1] = 0;
    wave_sync();
    bool in0 = !ok0 || v0 <= 1, in1 = !ok1;
    const T pir = __shfl(pi0, 1);
    T key0 = in0 ? inf : (T)W[s + v0] + pir + pi0;
    T key1 = in1 ? inf : (T)W[s + v1] + pir + pi1;
    int par0 = 1, par1 = 1;
    T tree = 0, amag = 0;
    for (int step = 0; step < n - 2; ++step) {
        T k = inf;
        int who = INT_MAX;
        if (!in0) {
            k = key0;
            who = v0;
        }
        if (!in1 && key1 < k) {
            k = key1;
            who = v1;
        }
        wave_argmin(k, who);
        const int u = who;
        tree += k;
        amag += k < 0 ? -k : k;
        if (v0 == u) {
            in0 = true;
            atomicAdd(&deg[par0], 1);
            atomicAdd(&deg[u], 1);
        }
        if (v1 == u) {
            in1 = true;
            atomicAdd(&deg[par1], 1);
            atomicAdd(&deg[u], 1);
        }
        const T pu = u < kWave ? __shfl(pi0, u) : __shfl(pi1, u - kWave);
        if (!in0) {
            const T c = (T)W[u * s + v0] + pu + pi0;
            if (c < key0) {
                key0 = c;
                par0 = u;
            }
        }
        if (!in1) {
            const T c = (T)W[u * s + v1] + pu + pi1;
            if (c < key1) {
                key1 = c;
                par1 = u;
            }
        }
    }
    // the two cheapest edges at vertex 0 (pi_0 is lane 0's pi0)
    const T piz = __shfl(pi0, 0);
    const T c0 = (ok0 && v0 >= 1) ? (T)W[v0] + piz + pi0 : inf;
    const T c1 = ok1 ? (T)W[v1] + piz + pi1 : inf;
    T m1 = c0 < c1 || (c0 == c1) ? c0 : c1;
    int e1 = c0 <= c1 ? v0 : v1;
    wave_argmin(m1, e1);
    T m2 = (v0 == e1) ? c1 : (v1 == e1 ? c0 : (c0 <= c1 ? c0 : c1));
    int e2 = (v0 == e1) ? v1 : (v1 == e1 ? v0 : (c0 <= c1 ? v0 : v1));
    if (m2 == inf) e2 = INT_MAX;
    wave_argmin(m2, e2);
    wave_sync();
    if (lane == 0) {
        deg[0] = 2;
        atomicAdd(&deg[e1], 1);
        atomicAdd(&deg[e2], 1);
    }
    T psum = (ok0 ? pi0 : (T)0) + (ok1 ? pi1 : (T)0);
    T pmag = (ok0 ? (pi0 < 0 ? -pi0 : pi0) : (T)0) + (ok1 ? (pi1 < 0 ? -pi1 : pi1) : (T)0);
    psum = wave_sum(psum);
    pmag = wave_sum(pmag);
    wave_sync();
    *mag = amag + (m1 < 0 ? -m1 : m1) + (m2 < 0 ? -m2 : m2) + 2 * pmag;
    return tree + m1 + m2 - 2 * psum;
}

__global__ __launch_bounds__(kWave) void tour_lower_bound_kernel(const float* __restrict__ Wg,
                                                                 const long long* __restrict__ w_off,
                                                                 const int* __restrict__ n_arr,
                                                                 const float* __restrict__ upper, int n_max, int iters,
                                                                 double* __restrict__ lb) {
    extern __shared__ float lds[];
    __shared__ int deg[kMaxN];
    const int inst = blockIdx.x, lane = threadIdx.x;
    const int n = n_arr[inst];
    if (n < 4 || n > n_max) {
        if (lane == 0) lb[inst] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int s = lds_stride(n);
    {
        const float* src = Wg + w_off[inst];
        for (int e = lane; e < n * n; e += kWave) lds[(e / n) * s + e % n] = src[e];
    }
    __syncthreads();
    const float ub = upper[inst];
    const int v0 = lane, v1 = lane + kWave;
    float pi0 = 0.f, pi1 = 0.f, bp0 = 0.f, bp1 = 0.f, best = -FLT_MAX, lambda = 2.f, mag;
    int stall = 0;
    for (int it = 0; it < iters; ++it) {
        const float L = one_tree<float>(lds, s, n, pi0, pi1, lane, deg, &mag);
        if (L > best) {
            best = L;
            bp0 = pi0;
            bp1 = pi1;
            stall = 0;
        } else if (++stall >= 8) {   // halving schedule: no improvement in 8 steps
            lambda *= 0.5f;
            stall = 0;
        }
        const int g0 = v0 < n ? deg[v0] - 2 : 0, g1 = v1 < n ? deg[v1] - 2 : 0;
        const int gg = wave_sum(g0 * g0 + g1 * g1);
        if (gg == 0 || lambda < 1e-6f) break;   // the 1-tree is a tour (optimal), or the step has vanished
        const float gap = fmaxf(ub - L, 1e-4f * fabsf(L) + 1e-30f);
        const float t = lambda * gap / (float)gg;   // Polyak step towards the tour-search upper bound
        pi0 += t * (float)g0;
        pi1 += t * (float)g1;
        wave_sync();
    }
    // the best multipliers' 1-tree, again from scratch in fp64 (the fp32 Prim above may pick a non-minimal tree under
    // rounding), less a margin for the fp64 rounding of the c(u,v) sums and the accumulation
    double dmag;
    const double L = one_tree<double>(lds, s, n, (double)bp0, (double)bp1, lane, deg, &dmag);
    if (lane == 0) lb[inst] = L - 8.0 * (double)n * DBL_EPSILON * dmag;
}

template <typename K>
int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return TSPGNN_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e != hipSuccess) return fail((int)e, "tour kernels: hipFuncSetAttribute: %s", hipGetErrorString(e));
    return TSPGNN_OK;
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_tour_search(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                  const long long* t_off, const long long* index, int n_inst, int n_max, int restarts,
                                  int kicks, unsigned long long seed, int32_t* tours, float* costs, void* stream) {
    TSPGNN_REQUIRE(n_inst >= 0, "tour_search: n_inst=%d", n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    if (n_max > kMaxN) return fail(TSPGNN_EUNSUPPORTED, "tour_search: n_max=%d exceeds %d", n_max, kMaxN);
    TSPGNN_REQUIRE(n_max >= 4, "tour_search: n_max=%d must be at least 4", n_max);
    TSPGNN_REQUIRE(restarts >= 1 && restarts <= kMaxChains, "tour_search: restarts=%d not in [1, %d]", restarts,
                   kMaxChains);
    TSPGNN_REQUIRE(kicks >= 0, "tour_search: kicks=%d", kicks);
    TSPGNN_REQUIRE(W && w_off && n && t_off && tours && costs, "tour_search: null pointer");
    const size_t lds = ((size_t)n_max * (n_max | 1) + (size_t)3 * restarts * n_max) * sizeof(float);
    int rc = allow_lds(tour_search_kernel, lds);
    if (rc) return rc;
    tour_search_kernel<<<(unsigned)n_inst, kWave * restarts, lds, as_stream(stream)>>>(
        W, w_off, n, init_tours, t_off, index, n_max, kicks, seed, tours, costs);
    return launched("tspgnn_tour_search");
}

extern "C" int tspgnn_tour_lower_bound(const float* W, const long long* w_off, const int* n, const float* upper,
                                       int n_inst, int n_max, int iters, double* lb, void* stream) {
    TSPGNN_REQUIRE(n_inst >= 0, "tour_lower_bound: n_inst=%d", n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    if (n_max > kMaxN) return fail(TSPGNN_EUNSUPPORTED, "tour_lower_bound: n_max=%d exceeds %d", n_max, kMaxN);
    TSPGNN_REQUIRE(n_max >= 4, "tour_lower_bound: n_max=%d must be at least 4", n_max);
    TSPGNN_REQUIRE(iters >= 1, "tour_lower_bound: iters=%d", iters);
    TSPGNN_REQUIRE(W && w_off && n && upper && lb, "tour_lower_bound: null pointer");
    const size_t lds = (size_t)n_max * (n_max | 1) * sizeof(float);
    int rc = allow_lds(tour_lower_bound_kernel, lds);
    if (rc) return rc;
    tour_lower_bound_kernel<<<(unsigned)n_inst, kWave, lds, as_stream(stream)>>>(W, w_off, n, upper, n_max, iters, lb);
    return launched("tspgnn_tour_lower_bound");
}
