// Batched TSP tour labelling (tspgnn/dataset.py, the counterpart of the reference's Concorde call in dataset.py:9-50):
//   tspgnn_tour_search       multi-start iterated local search (2-opt + Or-opt, double-bridge kicks), one workgroup per
//                            instance, one wave64 per chain, the instance's weight matrix resident in LDS;
//   tspgnn_tour_lower_bound  the Held-Karp 1-tree bound by subgradient ascent, one wave64 per instance, the final 1-tree
//                            re-evaluated in fp64 so that the reported value is a lower bound under rounding.
//   tspgnn_tour_search_knn   the same search with its descent restricted to the moves that add an edge between near
//                            neighbours (descend_knn below): about 13 n K evaluations per applied move, not 5.3 n^2.
//   tspgnn_tour_search_cand  that search with the candidate table handed in by the caller, one row of `columns` vertex
//                            ids per vertex, instead of built from the weights (stage_candidates below).
// All are issue-bound on LDS reads and VALU work: an instance reads its n*n weights from memory once.
// Each has two layouts of the weights, one device body: the dense matrix (tspgnn_tour_search / _lower_bound, n <= 128)
// and the packed strict upper triangle (the _tri entry points, n <= 256, 130 560 B at n = 256).  The bodies read a weight
// only through the layout's W(a, b), and both layouts hold the same fp32 value for w(a, b), so for n <= 128 the two give
// the same bits.
//
// Termination: every loop below has a fixed trip-count bound.  A descent accepts a move only on a strict improvement of
// more than kEpsRel * cost / n and makes at most 4 n^2 moves; the kick and subgradient counts are arguments.  There is no
// inter-workgroup communication.
#include "tour_common.h"

namespace tspgnn {
namespace {

constexpr float kEpsRel = 1e-6f;   // a move must gain more than kEpsRel * (cost / n): ~16 ulp of a mean edge

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

// u = tour t after the move `code`; then the two are swapped, so that t is the new tour.
__device__ __forceinline__ void apply_move(int*& t, int*& u, int n, int code, int lane) {
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
}

// Best-improvement descent on tour *t (scratch *u; the two are swapped per applied move).  Returns the tour's cost.
template <class WA>
__device__ float descend(const WA& W, int*& t, int*& u, int n, int lane) {
    float cost = tour_cost(W, t, n, lane);
    const int cap = 4 * n * n;
    for (int mv = 0; mv < cap; ++mv) {
        float best = FLT_MAX;
        int code = INT_MAX;
        // 2-opt: reverse positions i+1..j (0 <= i, i+1 < j <= n-1, not the whole cycle)
        for (Strider p(n, lane); p.i < n; p.step()) {
            const int i = p.i, j = p.j;
            two_exchange(W, t, n, i, j, [&](float d) {
                const int cd = (i << 8) | j;
                if (d < best || (d == best && cd < code)) {
                    best = d;
                    code = cd;
                }
            });
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
                const float gain = W(prev, nx) - (W(prev, s0) + W(sl, nx));
                const float ab = W(a, b);
                const float fwd = (W(a, s0) + W(sl, b)) - ab;
                const float rev = (W(a, sl) + W(s0, b)) - ab;
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
        apply_move(t, u, n, code, lane);
        cost = tour_cost(W, t, n, lane);
    }
    return cost;
}

// ------------------------------------------------------------------------------------- candidate-list descent (_knn)
// N(x) = the kk = min(K, n-1) vertices y != x smallest by (w(x, y), y); S = the pairs {x, y} with y in N(x) or x in N(y).
// A move of descend() is a candidate iff one of the edges it adds -- 2-opt: {t[i], t[j]}, {t[i+1], t[j+1]}; Or-opt: the
// two insertion edges of its orientation, not the closing edge {prev, nx} -- is in S.  A step takes the argmin of
// (delta, code) over the candidates, with descend()'s deltas, codes, threshold and cap, where the two orientations of an
// Or-opt (L, i, q) are two moves (descend()'s "reverse iff rev < fwd" is that argmin: the forward code is the smaller).
// The result is a function of the candidate SET, so the enumeration below may meet a move more than once.
struct Knn {
    uint8_t* tab;   // [n][kk] vertex ids: row x = N(x), less the entries (x, y) with y < x and x in N(y), which hold x
                    // itself ("skip"): every pair of S is then met once, from its smaller vertex when both rows have it
    uint8_t* pos;   // this chain's pos[v] = position of vertex v in the tour being descended
    int kk;
};

// Every thread drops the second copy of a mutual pair: entry (x, y) with y < x and x in row y becomes x ("skip").  A
// thread meets at most n kk / 64 <= 128 entries, whose verdicts wait in two 64-bit masks for the barrier between the
// reading and the writing of the table.  The table is complete on entry (a barrier behind its last write); ends with a
// barrier.
template <class WA>
__device__ void dedup_neighbors(uint8_t* tab, int n, int kk, int wave, int waves, int lane) {
    static_assert(WA::kMaxN * 32 / kWave <= 128, "the two dedup masks hold a thread's entries");
    const int tid = wave * kWave + lane, nt = waves * kWave, m = n * kk;
    uint64_t dup0 = 0, dup1 = 0;
    int it = 0;
    for (int e = tid; e < m; e += nt, ++it) {
        const int x = e / kk, y = tab[e];
        bool dup = false;
        if (y < x)
            for (int s = 0; s < kk; ++s) dup |= tab[y * kk + s] == x;
        if (dup) {
            if (it < 64) dup0 |= 1ull << it;
            else dup1 |= 1ull << (it - 64);
        }
    }
    __syncthreads();
    it = 0;
    for (int e = tid; e < m; e += nt, ++it)
        if ((it < 64 ? dup0 >> it : dup1 >> (it - 64)) & 1) tab[e] = (uint8_t)(e / kk);
    __syncthreads();
}

// The workgroup builds the table: wave `wave` of `waves` selects rows wave, wave + waves, ... by kk rounds of argmin
// over (w, y), a lane holding vertices lane, lane + 64, ...; then dedup_neighbors.  Ends with a barrier.
template <class WA>
__device__ void build_neighbors(const WA& W, uint8_t* tab, int n, int kk, int wave, int waves, int lane) {
    constexpr int V = WA::kMaxN / kWave;
    for (int x = wave; x < n; x += waves) {
        float key[V];
        bool avail[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int y = lane + j * kWave;
            avail[j] = y < n && y != x;
            key[j] = avail[j] ? W(x, y) : FLT_MAX;
        }
        for (int s = 0; s < kk; ++s) {
            float bv = FLT_MAX;
            int bc = INT_MAX;
#pragma unroll
            for (int j = 0; j < V; ++j) {   // ascending y: a strict < keeps the smaller id on a tie
                if (avail[j] && (bc == INT_MAX || key[j] < bv)) {
                    bv = key[j];
                    bc = lane + j * kWave;
                }
            }
            wave_argmin(bv, bc);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (lane + j * kWave == bc) avail[j] = false;
            if (lane == 0) tab[x * kk + s] = (uint8_t)(bc == INT_MAX ? x : bc);   // kk <= n - 1: bc is a vertex
        }
    }
    __syncthreads();
    dedup_neighbors<WA>(tab, n, kk, wave, waves, lane);
}

// _cand: the caller's table in place of build_neighbors'.  Entry (x, s) = y stands for the pair {x, y} when y < n and
// y != x; any other entry becomes x ("skip").  Rows may be asymmetric, repeat an entry or hold nothing: descend_knn's
// result is a function of the pair set.  Then dedup_neighbors, which keeps that set.  Ends with a barrier.
template <class WA>
__device__ void stage_candidates(const uint8_t* __restrict__ src, uint8_t* tab, int n, int columns, int wave, int waves,
                                 int lane) {
    const int tid = wave * kWave + lane, nt = waves * kWave, m = n * columns;
    for (int e = tid; e < m; e += nt) {
        const int x = e / columns, y = src[e];
        tab[e] = (uint8_t)(y < n && y != x ? y : x);
    }
    __syncthreads();
    dedup_neighbors<WA>(tab, n, columns, wave, waves, lane);
}

// One lane's running best over the candidates it generates.
template <class WA>
struct KnnScan {
    const WA& W;
    const int* t;
    int n;
    float best = FLT_MAX;
    int code = INT_MAX;
    __device__ __forceinline__ void take(float d, int cd) {
        if (d < best || (d == best && cd < code)) {
            best = d;
            code = cd;
        }
    }
    __device__ __forceinline__ int wrap(int p) const { return p < 0 ? p + n : p >= n ? p - n : p; }
    // descend()'s 2-opt move (i, j), when it is one
    __device__ __forceinline__ void two_opt(int i, int j) {
        if (i >= 0) two_exchange(W, t, n, i, j, [&](float d) { take(d, (i << 8) | j); });
    }
    // descend()'s Or-opt move (L, i, q) in the orientation rv, when it is one; i and q in [0, n)
    __device__ __forceinline__ void or_opt(int L, int i, int q, int rv) {
        const int rel = wrap(q - i);
        if (rel < L || rel > n - 2) return;
        const int prev = t[wrap(i - 1)], s0 = t[i], sl = t[wrap(i + L - 1)], nx = t[wrap(i + L)], a = t[q],
                  b = t[wrap(q + 1)];
        const float gain = W(prev, nx) - (W(prev, s0) + W(sl, nx));
        const float ab = W(a, b);
        const float ins = rv ? (W(a, sl) + W(s0, b)) - ab : (W(a, s0) + W(sl, b)) - ab;
        take(gain + ins, kOrOpt | (rv << 29) | (L << 26) | (i << 8) | q);
    }
};

// descend() over the candidates.  Work item 2 e + h: table entry e = (x, y), h = which of the two is u in the ordered
// roles below; eleven moves per item.  Lanes 2 k and 2 k + 1 read one table byte, a wave 32 consecutive ones.
template <class WA>
__device__ float descend_knn(const WA& W, const Knn& K, int*& t, int*& u, int n, int lane) {
    float cost = tour_cost(W, t, n, lane);
    const int cap = 4 * n * n, items = 2 * n * K.kk;
    for (int mv = 0; mv < cap; ++mv) {
        for (int k = lane; k < n; k += kWave) K.pos[t[k]] = (uint8_t)k;
        wave_sync();
        KnnScan<WA> sc{W, t, n};
        for (int item = lane; item < items; item += kWave) {
            const int e = item >> 1, h = item & 1;
            const int x = e / K.kk, y = K.tab[e];
            if (y == x) continue;
            const int pu = K.pos[h ? y : x], pv = K.pos[h ? x : y];
            const int lo = min(pu, pv), hi = max(pu, pv);
            if (!h) sc.two_opt(lo, hi);                      // {t[i], t[j]} = {x, y}
            else if (lo >= 1) sc.two_opt(lo - 1, hi - 1);    // {t[i+1], t[j+1]} = {x, y}
            else sc.two_opt(hi - 1, n - 1);                  // ... with j + 1 = n, which is position 0
            for (int L = 1; L <= 3 && L <= n - 3; ++L) {
                sc.or_opt(L, pv, pu, 0);                                   // a = u, s0 = v
                sc.or_opt(L, sc.wrap(pu - L + 1), sc.wrap(pv - 1), 0);     // sl = u, b = v
                if (L > 1) {
                    sc.or_opt(L, sc.wrap(pv - L + 1), pu, 1);              // a = u, sl = v
                    sc.or_opt(L, pu, sc.wrap(pv - 1), 1);                  // s0 = u, b = v
                }
            }
        }
        float best = sc.best;
        int code = sc.code;
        wave_argmin(best, code);
        if (!(best < -kEpsRel * cost / (float)n)) break;   // wave-uniform: every lane holds the same pair
        apply_move(t, u, n, code, lane);
        cost = tour_cost(W, t, n, lane);
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

// Where the descent's candidate table comes from: none (descend(), the whole neighbourhood), the `neighbors` nearest by
// weight (build_neighbors), or the caller's rows of `neighbors` columns (stage_candidates).
enum TabSrc { kTabNone = 0, kTabNearest = 1, kTabGiven = 2 };

// kTab != kTabNone: the chains descend by descend_knn over a table of `neighbors` columns; otherwise by descend().
// cand / c_off are read by kTabGiven alone; they come last, so the other instantiations read their arguments where they
// always did.
template <class WA, TabSrc kTab>
__global__ __launch_bounds__(kWave* kMaxChains) void tour_search_kernel(
    const float* __restrict__ Wg, const long long* __restrict__ w_off, const int* __restrict__ n_arr,
    const int32_t* __restrict__ init, const long long* __restrict__ t_off, const long long* __restrict__ index, int n_max,
    int kicks, int neighbors, unsigned long long seed, int32_t* __restrict__ tours, float* __restrict__ costs,
    const uint8_t* __restrict__ cand, const long long* __restrict__ c_off) {
    constexpr bool kKnn = kTab != kTabNone;
    extern __shared__ float lds[];
    __shared__ ChainPosts post;
    const int inst = blockIdx.x;
    const long long gi = index ? index[inst] : inst;
    const int n = n_arr[inst];
    const int chains = blockDim.x / kWave;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (never_sent(n, n_max)) {
        if (threadIdx.x == 0) refuse(&costs[inst]);
        return;
    }
    const WA W = WA::stage(lds, Wg + w_off[inst], n, threadIdx.x, blockDim.x);
    const ChainLds<WA> ws{lds, n_max, chains, kKnn ? neighbors : 0};
    // the chain's three tours: current, work, scratch
    int* cur = ws.tour(wave, 0);
    int* work = ws.tour(wave, 1);
    int* scr = ws.tour(wave, 2);
    __syncthreads();
    Knn nb{};
    if constexpr (kKnn) {
        nb.tab = ws.table();
        nb.pos = ws.positions(wave);
        if constexpr (kTab == kTabGiven) {
            nb.kk = neighbors;
            stage_candidates<WA>(cand + c_off[inst], nb.tab, n, nb.kk, wave, chains, lane);
        } else {
            nb.kk = min(neighbors, n - 1);
            build_neighbors(W, nb.tab, n, nb.kk, wave, chains, lane);
        }
    }

    // starting tour: chain 0 takes init_tours when given and a permutation of 0..n-1; otherwise Fisher-Yates
    const bool have = wave == 0 && init && load_permutation(init + t_off[inst], cur, scr, n, lane);
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
    float best;
    if constexpr (kKnn) best = descend_knn(W, nb, cur, scr, n, lane);
    else best = descend(W, cur, scr, n, lane);
    for (int kick = 0; kick < kicks; ++kick) {
        double_bridge(cur, work, n, draw(seed, gi, wave, kick, 0), lane);
        float c;
        if constexpr (kKnn) c = descend_knn(W, nb, work, scr, n, lane);
        else c = descend(W, work, scr, n, lane);
        if (c <= best) {   // no worse: accept (the chain's current tour is always its best)
            int* x = cur;
            cur = work;
            work = x;
            best = c;
        }
    }
    // the winner, ties to the lower chain (the descents have swapped cur among the chain's three tours)
    if (lane == 0) {
        post.cost[wave] = best;
        post.tag[wave] = (int)(cur - reinterpret_cast<int*>(lds));
    }
    __syncthreads();
    if (wave != 0) return;
    float bc = post.cost[0];
    int bw = 0;
    for (int c = 1; c < chains; ++c) {
        if (post.cost[c] < bc) {
            bc = post.cost[c];
            bw = c;
        }
    }
    write_canonical(reinterpret_cast<const int*>(lds) + post.tag[bw], n, tours + t_off[inst], lane);
    if (lane == 0) costs[inst] = bc;
}

// ---------------------------------------------------------------------------------------------------------- lower bound

template <class WA>
__global__ __launch_bounds__(kWave) void tour_lower_bound_kernel(const float* __restrict__ Wg,
                                                                 const long long* __restrict__ w_off,
                                                                 const int* __restrict__ n_arr,
                                                                 const float* __restrict__ upper, int n_max, int iters,
                                                                 double* __restrict__ lb) {
    constexpr int K = WA::kMaxN / kWave;
    extern __shared__ float lds[];
    __shared__ int deg[WA::kMaxN];
    const int inst = blockIdx.x, lane = threadIdx.x;
    const int n = n_arr[inst];
    if (never_sent(n, n_max)) {
        if (lane == 0) refuse(&lb[inst]);
        return;
    }
    const WA W = WA::stage(lds, Wg + w_off[inst], n, lane, kWave);
    __syncthreads();
    float pi[K], bp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) pi[j] = 0.f;
    ascend(W, NoCons{}, n, upper[inst], iters, lane, deg, pi, bp);
    const double L = rebuilt_bound(W, NoCons{}, n, bp, lane, deg);
    if (lane == 0) lb[inst] = L;
}

// neighbors: 0 = the full-scan kernel (kTabNone); the _knn entry points pass their 1..32, the _cand entry points their
// columns with the table (cand, c_off), which the others leave null.
template <class WA, TabSrc kTab>
int search(const char* entry, const char* what, const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
           const long long* t_off, const long long* index, int n_inst, int n_max, int restarts, int kicks, int neighbors,
           unsigned long long seed, int32_t* tours, float* costs, void* stream, const uint8_t* cand = nullptr,
           const long long* c_off = nullptr) {
    constexpr bool kKnn = kTab != kTabNone;
    TSPGNN_REQUIRE(n_inst >= 0, "%s: n_inst=%d", what, n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    if constexpr (kKnn)
        TSPGNN_REQUIRE(neighbors >= 1 && neighbors <= kMaxNeighbors, "%s: %s=%d not in [1, %d]", what,
                       kTab == kTabGiven ? "columns" : "neighbors", neighbors, kMaxNeighbors);
    int rc = check_layout<WA>(what, n_max);
    if (rc) return rc;
    TSPGNN_REQUIRE(restarts >= 1 && restarts <= kMaxChains, "%s: restarts=%d not in [1, %d]", what, restarts,
                   kMaxChains);
    const int fit = ChainLds<WA>::fit(n_max, neighbors);
    TSPGNN_REQUIRE(restarts <= fit, "%s: restarts=%d: at n_max=%d at most %d chains fit in LDS", what, restarts, n_max, fit);
    TSPGNN_REQUIRE(kicks >= 0, "%s: kicks=%d", what, kicks);
    TSPGNN_REQUIRE(W && w_off && n && t_off && tours && costs, "%s: null pointer", what);
    if constexpr (kTab == kTabGiven) TSPGNN_REQUIRE(cand && c_off, "%s: null pointer", what);
    const size_t lds = ChainLds<WA>{nullptr, n_max, restarts, neighbors}.bytes();
    rc = allow_lds(tour_search_kernel<WA, kTab>, lds);
    if (rc) return rc;
    tour_search_kernel<WA, kTab><<<(unsigned)n_inst, kWave * restarts, lds, as_stream(stream)>>>(
        W, w_off, n, init_tours, t_off, index, n_max, kicks, neighbors, seed, tours, costs, cand, c_off);
    return launched(entry);
}

template <class WA>
int lower_bound(const char* entry, const char* what, const float* W, const long long* w_off, const int* n, const float* upper, int n_inst,
                int n_max, int iters, double* lb, void* stream) {
    TSPGNN_REQUIRE(n_inst >= 0, "%s: n_inst=%d", what, n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    int rc = check_layout<WA>(what, n_max);
    if (rc) return rc;
    TSPGNN_REQUIRE(iters >= 1, "%s: iters=%d", what, iters);
    TSPGNN_REQUIRE(W && w_off && n && upper && lb, "%s: null pointer", what);
    const size_t lds = WA::floats(n_max) * sizeof(float);
    rc = allow_lds(tour_lower_bound_kernel<WA>, lds);
    if (rc) return rc;
    tour_lower_bound_kernel<WA><<<(unsigned)n_inst, kWave, lds, as_stream(stream)>>>(W, w_off, n, upper, n_max, iters, lb);
    return launched(entry);
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_tour_search(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                  const long long* t_off, const long long* index, int n_inst, int n_max, int restarts,
                                  int kicks, unsigned long long seed, int32_t* tours, float* costs, void* stream) {
    return search<SquareW, kTabNone>("tspgnn_tour_search", "tour_search", W, w_off, n, init_tours, t_off, index, n_inst,
                                  n_max, restarts, kicks, 0, seed, tours, costs, stream);
}

extern "C" int tspgnn_tour_lower_bound(const float* W, const long long* w_off, const int* n, const float* upper,
                                       int n_inst, int n_max, int iters, double* lb, void* stream) {
    return lower_bound<SquareW>("tspgnn_tour_lower_bound", "tour_lower_bound", W, w_off, n, upper, n_inst, n_max, iters,
                                lb, stream);
}

extern "C" int tspgnn_tour_search_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                      const long long* t_off, const long long* index, int n_inst, int n_max, int restarts,
                                      int kicks, unsigned long long seed, int32_t* tours, float* costs, void* stream) {
    return search<TriW, kTabNone>("tspgnn_tour_search_tri", "tour_search_tri", W, w_off, n, init_tours, t_off, index, n_inst,
                               n_max, restarts, kicks, 0, seed, tours, costs, stream);
}

extern "C" int tspgnn_tour_lower_bound_tri(const float* W, const long long* w_off, const int* n, const float* upper,
                                           int n_inst, int n_max, int iters, double* lb, void* stream) {
    return lower_bound<TriW>("tspgnn_tour_lower_bound_tri", "tour_lower_bound_tri", W, w_off, n, upper, n_inst, n_max,
                             iters, lb, stream);
}

extern "C" int tspgnn_tour_search_knn(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                      const long long* t_off, const long long* index, int n_inst, int n_max, int restarts,
                                      int kicks, int neighbors, unsigned long long seed, int32_t* tours, float* costs,
                                      void* stream) {
    return search<SquareW, kTabNearest>("tspgnn_tour_search_knn", "tour_search_knn", W, w_off, n, init_tours, t_off, index, n_inst,
                                 n_max, restarts, kicks, neighbors, seed, tours, costs, stream);
}

extern "C" int tspgnn_tour_search_knn_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                          const long long* t_off, const long long* index, int n_inst, int n_max,
                                          int restarts, int kicks, int neighbors, unsigned long long seed, int32_t* tours,
                                          float* costs, void* stream) {
    return search<TriW, kTabNearest>("tspgnn_tour_search_knn_tri", "tour_search_knn_tri", W, w_off, n, init_tours, t_off, index,
                              n_inst, n_max, restarts, kicks, neighbors, seed, tours, costs, stream);
}

extern "C" int tspgnn_tour_search_cand(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                       const long long* t_off, const long long* index, const uint8_t* cand,
                                       const long long* c_off, int n_inst, int n_max, int restarts, int kicks, int columns,
                                       unsigned long long seed, int32_t* tours, float* costs, void* stream) {
    return search<SquareW, kTabGiven>("tspgnn_tour_search_cand", "tour_search_cand", W, w_off, n, init_tours, t_off,
                                      index, n_inst, n_max, restarts, kicks, columns, seed, tours, costs, stream, cand,
                                      c_off);
}

extern "C" int tspgnn_tour_search_cand_tri(const float* W, const long long* w_off, const int* n, const int32_t* init_tours,
                                           const long long* t_off, const long long* index, const uint8_t* cand,
                                           const long long* c_off, int n_inst, int n_max, int restarts, int kicks,
                                           int columns, unsigned long long seed, int32_t* tours, float* costs,
                                           void* stream) {
    return search<TriW, kTabGiven>("tspgnn_tour_search_cand_tri", "tour_search_cand_tri", W, w_off, n, init_tours, t_off,
                                   index, n_inst, n_max, restarts, kicks, columns, seed, tours, costs, stream, cand,
                                   c_off);
}

template <class WA>
static long long chains_fit_query(int n_max, int neighbors) {
    if (n_max < 4 || n_max > WA::kMaxN || neighbors < 0 || neighbors > kMaxNeighbors) return 0;
    return ChainLds<WA>::fit(n_max, neighbors);
}

extern "C" long long tspgnn_tour_chains_fit(int tri, int n_max, int neighbors) {
    return tri ? chains_fit_query<TriW>(n_max, neighbors) : chains_fit_query<SquareW>(n_max, neighbors);
}
