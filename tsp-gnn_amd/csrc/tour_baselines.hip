// Classical baselines for the decision TSP (tspgnn/baselines.py; the reference's figures/test_varying_dev_baseline.png
// compares the network with them and ships no code for either):
//   tspgnn_tour_nearest_neighbor  the nearest-neighbour tour from one start vertex, or the best over every start;
//   tspgnn_tour_anneal            Metropolis annealing over 2-exchange moves, one wave64 per chain.
// Both run one workgroup per instance with the instance's weights resident in LDS, and both have the two layouts of
// tour_common.h behind one device body (dense matrix, n <= 128; packed strict upper triangle, the _tri entry points,
// n <= 256).  The bodies read a weight only through W(a, b) and both layouts hold the same fp32 values, so for n <= 128
// the two give the same bits.
//
// The annealing chain is DEFINED as a sequential process over proposal numbers p = 0 .. levels * per_level - 1 (see
// include/tspgnn.h).  A wave runs it speculatively: lane l evaluates proposal p0 + l against the current tour, the first
// accepting lane a is applied, and p0 advances by a + 1 (by 64 when no lane accepts).  Every proposal before a was
// rejected against the very tour it was evaluated on, so this is the sequential chain exactly.
//
// Termination: every loop below has a fixed trip-count bound.  A nearest-neighbour tour takes n - 1 steps per start and
// there are at most n starts; every wave step of a chain consumes at least one proposal, so its loop runs at most
// levels * per_level <= 2^31 - 1 times.  There is no inter-workgroup communication.
#include "tour_common.h"

#include <math.h>

namespace tspgnn {
namespace {

// Nearest-neighbour tour from `start` into t[0..n-1] (LDS): from the current vertex move to the unvisited vertex of
// smallest W(cur, v), ties to the smaller vertex id.  Lane l owns the vertices l, l+64, ... as one_tree does.
template <class WA>
__device__ void nearest_neighbor(const WA& W, int n, int start, int* t, int lane) {
    constexpr int K = WA::kMaxN / kWave;
    bool seen[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int v = lane + j * kWave;
        seen[j] = v >= n || v == start;
    }
    int cur = start;
    if (lane == 0) t[0] = start;
    for (int k = 1; k < n; ++k) {
        float best = FLT_MAX;
        int who = INT_MAX;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (!seen[j]) {
                const int v = lane + j * kWave;
                const float w = W(cur, v);
                if (who == INT_MAX || w < best) {   // v ascends: a strict < keeps the smaller id on a tie
                    best = w;
                    who = v;
                }
            }
        }
        wave_argmin(best, who);
        cur = who;
#pragma unroll
        for (int j = 0; j < K; ++j) seen[j] = seen[j] || lane + j * kWave == cur;
        if (lane == 0) t[k] = cur;
    }
    wave_sync();
}

template <class WA>
__global__ __launch_bounds__(kWave* kMaxChains) void nearest_neighbor_kernel(
    const float* __restrict__ Wg, const long long* __restrict__ w_off, const int* __restrict__ n_arr,
    const long long* __restrict__ t_off, int n_max, int start, int32_t* __restrict__ tours, float* __restrict__ costs) {
    extern __shared__ float lds[];
    __shared__ ChainPosts post;
    const int inst = blockIdx.x;
    const int n = n_arr[inst];
    const int waves = blockDim.x / kWave;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (never_sent(n, n_max)) {
        if (threadIdx.x == 0) refuse(&costs[inst]);
        return;
    }
    const WA W = WA::stage(lds, Wg + w_off[inst], n, threadIdx.x, blockDim.x);
    const ChainLds<WA> ws{lds, n_max, waves, 0};
    // per wave: the tour under construction and the wave's best (the third tour of the chain layout stays unused)
    int* cur = ws.tour(wave, 0);
    int* best = ws.tour(wave, 1);
    __syncthreads();

    float bc = FLT_MAX;
    int bs = INT_MAX;
    if (start >= 0) {   // one wave, one start
        bs = start % n;
        nearest_neighbor(W, n, bs, best, lane);
        bc = tour_cost(W, best, n, lane);
    } else {            // every start, the waves striding over them; a wave's starts ascend, so < keeps the smaller
        for (int s = wave; s < n; s += waves) {
            nearest_neighbor(W, n, s, cur, lane);
            const float c = tour_cost(W, cur, n, lane);
            if (bs == INT_MAX || c < bc) {
                bc = c;
                bs = s;
                for (int k = lane; k < n; k += kWave) best[k] = cur[k];
                wave_sync();
            }
        }
    }
    // ties to the smaller start.  Wave 0 always has start 0 (or the one start); a wave past n has none and posts
    // (+inf, INT_MAX), which is below no pair that wave 0 can post
    if (bs == INT_MAX) bc = __int_as_float(0x7f800000);
    chain_winner(ws, post, wave, lane, bc, bs, n, tours + t_off[inst], &costs[inst]);
}

template <class WA>
__global__ __launch_bounds__(kWave* kMaxChains) void tour_anneal_kernel(
    const float* __restrict__ Wg, const long long* __restrict__ w_off, const int* __restrict__ n_arr,
    const int32_t* __restrict__ init, const long long* __restrict__ t_off, const long long* __restrict__ index,
    const float* __restrict__ inv_temp, const int* __restrict__ per_level_arr, int n_max, int levels,
    unsigned long long seed, int32_t* __restrict__ tours, float* __restrict__ costs) {
    extern __shared__ float lds[];
    __shared__ ChainPosts post;
    const int inst = blockIdx.x;
    const long long gi = index ? index[inst] : inst;
    const int n = n_arr[inst];
    const int per_level = per_level_arr[inst];
    const long long budget = (long long)levels * (long long)per_level;
    const int chains = blockDim.x / kWave;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    // the host module never sends these; a defensive no-op keeps every LDS index in bounds and the trip count bounded
    if (never_sent(n, n_max) || per_level < 0 || budget > (long long)INT_MAX) {
        if (threadIdx.x == 0) refuse(&costs[inst]);
        return;
    }
    const WA W = WA::stage(lds, Wg + w_off[inst], n, threadIdx.x, blockDim.x);
    const ChainLds<WA> ws{lds, n_max, chains, 0};
    // the chain's three tours: current, best, scratch
    int* cur = ws.tour(wave, 0);
    int* best = ws.tour(wave, 1);
    int* scr = ws.tour(wave, 2);
    __syncthreads();

    // starting tour: chain 0 takes init_tours when given and a permutation of 0..n-1; otherwise nearest neighbour from
    // vertex chain % n
    const bool have = wave == 0 && init && load_permutation(init + t_off[inst], cur, scr, n, lane);
    if (!have) nearest_neighbor(W, n, wave % n, cur, lane);
    for (int k = lane; k < n; k += kWave) best[k] = cur[k];
    wave_sync();

    const float* it = inv_temp + (long long)inst * levels;
    const unsigned P = (unsigned)budget, per = (unsigned)per_level;
    unsigned p0 = 0, off0 = 0;   // p0 = lev0 * per + off0, off0 < per
    int lev0 = 0;
    float it0 = P ? it[0] : 0.f;
    float rel = 0.f, best_rel = 0.f;
    while (p0 < P) {
        const unsigned p = p0 + (unsigned)lane;   // < 2^31 + 63
        bool acc = false;
        int i = 0, j = 0;
        float d = 0.f;
        if (p < P) {
            const uint64_t r = draw(seed, gi, wave, (int)p, 0);
            i = (int)((unsigned)(r & 0xffff) % (unsigned)n);
            j = (int)((unsigned)((r >> 16) & 0xffff) % (unsigned)n);
            if (i > j) {
                const int x = i;
                i = j;
                j = x;
            }
            two_exchange(W, cur, n, i, j, [&](float dm) {   // anything else is void
                d = dm;
                if (d <= 0.f) {
                    acc = true;
                } else {
                    const unsigned o = off0 + (unsigned)lane;
                    const float itl = o < per ? it0 : it[lev0 + (int)(o / per)];
                    const float u = ((float)(unsigned)((r >> 40) & 0x7fffff) + 0.5f) * 0x1p-23f;
                    acc = u < expf(-(d * itl));
                }
            });
        }
        const unsigned long long m = __ballot(acc);
        unsigned adv = kWave;
        if (m != 0) {   // wave-uniform
            const int a = __ffsll((long long)m) - 1;
            const int ai = __shfl(i, a), aj = __shfl(j, a);
            const float ad = __shfl(d, a);
            const int half = (aj - ai) >> 1;   // pairs to swap in the segment ai+1..aj; a lane's pairs are disjoint
            for (int k = lane; k < half; k += kWave) {
                const int x = cur[ai + 1 + k], y = cur[aj - k];
                cur[ai + 1 + k] = y;
                cur[aj - k] = x;
            }
            wave_sync();
            rel += ad;
            if (rel < best_rel) {
                best_rel = rel;
                for (int k = lane; k < n; k += kWave) best[k] = cur[k];
            }
            adv = (unsigned)a + 1u;
        }
        p0 += adv;
        off0 += adv;
        if (off0 >= per) {
            lev0 += (int)(off0 / per);
            off0 %= per;
            if (p0 < P) it0 = it[lev0];
        }
    }
    wave_sync();
    chain_winner(ws, post, wave, lane, tour_cost(W, best, n, lane), 0, n, tours + t_off[inst], &costs[inst]);
}

template <class WA>
int nearest(const char* entry, const char* what, const float* W, const long long* w_off, const int* n, const long long* t_off,
            int n_inst, int n_max, int start, int32_t* tours, float* costs, void* stream) {
    TSPGNN_REQUIRE(n_inst >= 0, "%s: n_inst=%d", what, n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    int rc = check_layout<WA>(what, n_max);
    if (rc) return rc;
    TSPGNN_REQUIRE(start >= -1, "%s: start=%d must be a vertex (>= 0) or -1 for every start", what, start);
    TSPGNN_REQUIRE(W && w_off && n && t_off && tours && costs, "%s: null pointer", what);
    const int waves = start >= 0 ? 1 : ChainLds<WA>::fit(n_max, 0);
    const size_t lds = ChainLds<WA>{nullptr, n_max, waves, 0}.bytes();
    rc = allow_lds(nearest_neighbor_kernel<WA>, lds);
    if (rc) return rc;
    nearest_neighbor_kernel<WA><<<(unsigned)n_inst, kWave * waves, lds, as_stream(stream)>>>(W, w_off, n, t_off, n_max, start,
                                                                                            tours, costs);
    return launched(entry);
}

template <class WA>
int anneal(const char* entry, const char* what, const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
           const long long* t_off, const long long* index, const float* inv_temp, const int* per_level, int n_inst, int n_max,
           int chains, int levels, unsigned long long seed, int32_t* tours, float* costs, void* stream) {
    TSPGNN_REQUIRE(n_inst >= 0, "%s: n_inst=%d", what, n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    int rc = check_layout<WA>(what, n_max);
    if (rc) return rc;
    TSPGNN_REQUIRE(chains >= 1 && chains <= kMaxChains, "%s: chains=%d not in [1, %d]", what, chains, kMaxChains);
    const int fit = ChainLds<WA>::fit(n_max, 0);
    TSPGNN_REQUIRE(chains <= fit, "%s: chains=%d: at n_max=%d at most %d chains fit in LDS", what, chains, n_max, fit);
    TSPGNN_REQUIRE(levels >= 0, "%s: levels=%d", what, levels);
    TSPGNN_REQUIRE(W && w_off && n && t_off && per_level && tours && costs && (inv_temp || levels == 0),
                   "%s: null pointer", what);
    const size_t lds = ChainLds<WA>{nullptr, n_max, chains, 0}.bytes();
    rc = allow_lds(tour_anneal_kernel<WA>, lds);
    if (rc) return rc;
    tour_anneal_kernel<WA><<<(unsigned)n_inst, kWave * chains, lds, as_stream(stream)>>>(
        W, w_off, n, init_tours, t_off, index, inv_temp, per_level, n_max, levels, seed, tours, costs);
    return launched(entry);
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_tour_nearest_neighbor(const float* W, const long long* w_off, const int* n, const long long* t_off,
                                            int n_inst, int n_max, int start, int32_t* tours, float* costs, void* stream) {
    return nearest<SquareW>("tspgnn_tour_nearest_neighbor", "tour_nearest_neighbor", W, w_off, n, t_off, n_inst, n_max, start,
                            tours, costs, stream);
}

extern "C" int tspgnn_tour_nearest_neighbor_tri(const float* W, const long long* w_off, const int* n, const long long* t_off,
                                                int n_inst, int n_max, int start, int32_t* tours, float* costs,
                                                void* stream) {
    return nearest<TriW>("tspgnn_tour_nearest_neighbor_tri", "tour_nearest_neighbor_tri", W, w_off, n, t_off, n_inst, n_max,
                         start, tours, costs, stream);
}

extern "C" int tspgnn_tour_anneal(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                  const long long* t_off, const long long* index, const float* inv_temp, const int* per_level,
                                  int n_inst, int n_max, int chains, int levels, unsigned long long seed, int32_t* tours,
                                  float* costs, void* stream) {
    return anneal<SquareW>("tspgnn_tour_anneal", "tour_anneal", W, w_off, n, init_tours, t_off, index, inv_temp, per_level,
                           n_inst, n_max, chains, levels, seed, tours, costs, stream);
}

extern "C" int tspgnn_tour_anneal_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                      const long long* t_off, const long long* index, const float* inv_temp,
                                      const int* per_level, int n_inst, int n_max, int chains, int levels,
                                      unsigned long long seed, int32_t* tours, float* costs, void* stream) {
    return anneal<TriW>("tspgnn_tour_anneal_tri", "tour_anneal_tri", W, w_off, n, init_tours, t_off, index, inv_temp,
                        per_level, n_inst, n_max, chains, levels, seed, tours, costs, stream);
}
