// tspgnn_tour_from_votes (tspgnn/decode.py): a tour per instance from the network's per-edge logits, E_vote of
// model.py:106-128, which the reference only ever averages (figures/route-examples.png draws them over the optimal
// route).  One workgroup per instance, reading the batch as it lies on the device after Session.prepare /
// DeviceDataset.batch.  No dense matrix, no host pass.  include/tspgnn.h DEFINES the result as a sequential process: the
// batch, the pair rule, the key and the tour's outputs under "tours from the edge votes", then this entry point's Order,
// Greedy and Stitch.  It depends on the instance and its votes alone: never on n_max, on the other instances or on the
// launch.
//
// Eligibility only ever shrinks -- degrees rise, components merge -- so "the first eligible edge in a fixed order,
// repeated" is one pass over the sorted list, and equally a workgroup-wide arg-max over (key, edge id) per round: no
// sort, and no LDS for 32 640 keys at n = 256.  A thread keeps its first kSlots edges (key, endpoints, a live bit) in
// registers, dropping an edge for good the first time it finds it ineligible; edges past that (only a multigraph has
// them) are re-read from memory every round.  Degrees and component ids sit in LDS, one word per vertex; the winner's
// endpoints and their component ids travel with the arg-max, and the vertices relabel the merged component in parallel.
// The workgroup is 64, 256 or 1024 threads for n_max <= 64, <= 128, <= 256 (kSlots * threads covers n (n-1) / 2): the
// arg-max is exact, so the shape changes nothing.
//
// Termination: the greedy loop runs at most n rounds (each but the last adds an edge, and a forest has at most n - 1);
// every path walk takes at most n steps.  There is no inter-workgroup communication.  Costs are plain fp32 additions
// (no products, and contraction is off as in dataset_build.hip).
#include "vote_common.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace tspgnn {
namespace {

constexpr int kSlots = 32;   // edges a thread keeps in registers

// f(integral_constant<int, j>) for j = J .. N-1.  The slot arrays below are indexed by these compile-time constants
// alone: behind a loop that is only unrolled later they stay one 32-word vector each, and every conditional update of
// one element makes another copy of the whole vector (6 KB of scratch per lane).
template <int J, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>{});
        static_for<J + 1, N>(f);
    }
}

// (key, edge id) as one word whose maximum is the first edge in the order: the id enters complemented.  0 = no edge.
__device__ __forceinline__ unsigned long long candidate(uint32_t key, uint32_t e) {
    return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - e);
}

// state word of a vertex: component id in bits 0-7, degree in bits 8-9
__device__ __forceinline__ int comp_of(int s) { return s & 0xff; }
__device__ __forceinline__ int deg_of(int s) { return s >> 8; }

template <int NT>
__global__ __launch_bounds__(NT) void tour_from_votes_kernel(const float* __restrict__ vote,
                                                             const int32_t* __restrict__ uv,
                                                             const float* __restrict__ wc,
                                                             const int32_t* __restrict__ seg,
                                                             const int32_t* __restrict__ vseg,
                                                             int32_t* __restrict__ tours, float* __restrict__ costs,
                                                             int32_t* __restrict__ n_missing) {
    constexpr int kWaves = NT / kWave;
    __shared__ int s_state[kVoteMaxN];
    __shared__ int s_nb[2][kVoteMaxN];     // the chosen edges: a vertex's neighbours, -1 = none
    __shared__ int s_len[kVoteMaxN];       // of the path that starts at this vertex; 0 = no path starts here
    __shared__ int s_min[kVoteMaxN];       // that path's smallest vertex id
    __shared__ int s_seq[kVoteMaxN];       // the stitched sequence
    __shared__ int s_tour[kVoteMaxN];      // ... in canonical form
    __shared__ int s_pos[kVoteMaxN];       // position of a vertex in s_seq, then in s_tour
    __shared__ int s_edge[kVoteMaxN];      // smallest edge id joining tour[k] and tour[k+1]; INT_MAX = none
    __shared__ float s_w[kVoteMaxN];
    __shared__ unsigned long long s_best[kWaves];
    __shared__ uint32_t s_pay[kWaves];

    const int inst = blockIdx.x;
    const int tid = threadIdx.x;
    const VoteInstance I(uv, seg, vseg, inst);
    const int v0 = I.v0, n = I.n;
    const long long e0 = I.e0, m = I.m;
    // the host module never sends these; a defensive no-op keeps every LDS index in bounds
    if (n < 4 || n > kVoteMaxN || m < 0) {
        if (tid == 0) refuse_tour(costs + inst, n_missing + inst);
        return;
    }
    const float* vt = vote + e0;

    for (int w = tid; w < n; w += NT) {
        s_state[w] = w;
        s_nb[0][w] = -1;
        s_nb[1][w] = -1;
        s_len[w] = 0;
        s_edge[w] = INT_MAX;
    }

    // this thread's edges tid, tid + NT, ...: key and endpoints in registers
    uint32_t key[kSlots], ends[kSlots / 2], live = 0;   // ends: a | b << 8, two slots to a word
    static_for<0, kSlots>([&](auto J) {
        constexpr int j = decltype(J)::value;
        const long long e = tid + (long long)j * NT;
        key[j] = 0;
        if (j % 2 == 0) ends[j / 2] = 0;
        if (e < m) {
            I.with_ends(e, [&](int a, int b) {
                key[j] = vote_key(vt[e]);
                ends[j / 2] |= ((uint32_t)a | ((uint32_t)b << 8)) << (16 * (j % 2));
                live |= 1u << j;
            });
        }
    });
    __syncthreads();

    // ---- greedy: one arg-max over the eligible edges per round
    for (int round = 0; round < n; ++round) {
        // this thread's first eligible edge: (bk, be), be = 0xffffffff while there is none; its edges ascend with the slot,
        // so a later one wins on a larger key alone
        uint32_t bk = 0, be = 0xffffffffu;
        uint32_t pay = 0;   // the winner's a | b << 8 | comp(a) << 16 | comp(b) << 24
        // Everything a slot derives from ends[j] and tid (LDS addresses, the complemented edge id) is invariant over the
        // rounds, and the compiler would keep all of it in registers beside the 48 of key and ends, which 1 024 threads
        // (128 registers each) cannot afford.  The empty asm statements make the two sources opaque once per use, so the
        // derived values are recomputed.
        uint32_t t = (uint32_t)tid;
        asm volatile("" : "+v"(t));
        static_for<0, kSlots>([&](auto J) {
            constexpr int j = decltype(J)::value;
            if (live & (1u << j)) {
                uint32_t en = ends[j / 2];
                asm volatile("" : "+v"(en));
                en = (en >> (16 * (j % 2))) & 0xffffu;
                const int a = en & 0xff, b = en >> 8;
                const int sa = s_state[a], sb = s_state[b];
                if (deg_of(sa) < 2 && deg_of(sb) < 2 && comp_of(sa) != comp_of(sb)) {
                    if (be == 0xffffffffu || key[j] > bk) {
                        bk = key[j];
                        be = t + (uint32_t)(j * NT);
                        pay = en | ((uint32_t)comp_of(sa) << 16) | ((uint32_t)comp_of(sb) << 24);
                    }
                } else {
                    live &= ~(1u << j);   // for good: eligibility never comes back
                }
            }
        });
        for (long long e = tid + (long long)kSlots * NT; e < m; e += NT) {   // a multigraph's surplus, from memory
            I.with_ends(e, [&](int a, int b) {
                const int sa = s_state[a], sb = s_state[b];
                if (deg_of(sa) < 2 && deg_of(sb) < 2 && comp_of(sa) != comp_of(sb)) {
                    const uint32_t k = vote_key(vt[e]);
                    if (be == 0xffffffffu || k > bk) {
                        bk = k;
                        be = (uint32_t)e;
                        pay = (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)comp_of(sa) << 16) |
                              ((uint32_t)comp_of(sb) << 24);
                    }
                }
            });
        }
        unsigned long long best = be == 0xffffffffu ? 0ull : candidate(bk, be);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {   // butterfly: every lane ends with the wave's winner
            const unsigned long long ob = __shfl_xor(best, off);
            const uint32_t op = __shfl_xor(pay, off);
            if (ob > best) {
                best = ob;
                pay = op;
            }
        }
        if constexpr (kWaves > 1) {
            if ((tid & (kWave - 1)) == 0) {
                s_best[tid / kWave] = best;
                s_pay[tid / kWave] = pay;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kWaves; ++k) {
                const unsigned long long ob = s_best[k];
                if (ob > best) {
                    best = ob;
                    pay = s_pay[k];
                }
            }
        }
        if (best == 0) break;   // workgroup-uniform: nothing is eligible any more
        const int a = pay & 0xff, b = (pay >> 8) & 0xff, ca = (pay >> 16) & 0xff, cb = pay >> 24;
        for (int w = tid; w < n; w += NT) {
            int s = s_state[w];
            if (comp_of(s) == cb) s = (s & ~0xff) | ca;
            if (w == a || w == b) {
                s_nb[deg_of(s)][w] = w == a ? b : a;
                s += 0x100;
            }
            s_state[w] = s;
        }
        __syncthreads();   // the new states before the next scan (and s_best / s_pay free again)
    }
    __syncthreads();

    // ---- stitch: every path from its smaller endpoint, the paths by their smallest vertex
    for (int w = tid; w < n; w += NT) {
        if (deg_of(s_state[w]) < 2) {
            int prev = -1, cur = w, len = 1, mn = w;
            for (int step = 1; step < n; ++step) {
                const int x = s_nb[0][cur], nxt = x != prev ? x : s_nb[1][cur];
                if (nxt < 0) break;
                prev = cur;
                cur = nxt;
                ++len;
                mn = min(mn, cur);
            }
            if (w <= cur) {   // w is the smaller endpoint (or the path's only vertex)
                s_len[w] = len;
                s_min[w] = mn;
            }
        }
    }
    __syncthreads();
    for (int w = tid; w < n; w += NT) {
        const int len = s_len[w];
        if (len > 0) {
            const int mine = s_min[w];
            int at = 0;
            for (int x = 0; x < n; ++x)
                if (s_len[x] > 0 && s_min[x] < mine) at += s_len[x];
            int prev = -1, cur = w;
            for (int k = 0; k < len; ++k) {
                s_seq[at + k] = cur;
                s_pos[cur] = at + k;
                const int x = s_nb[0][cur], nxt = x != prev ? x : s_nb[1][cur];
                prev = cur;
                cur = nxt;
            }
        }
    }
    __syncthreads();

    // ---- canonical form: from vertex 0 towards its smaller neighbour in the cycle
    const int p0 = s_pos[0];
    const bool fwd = s_seq[p0 + 1 < n ? p0 + 1 : 0] < s_seq[p0 > 0 ? p0 - 1 : n - 1];
    __syncthreads();   // s_pos is rewritten below
    int32_t* out = tours + v0;
    for (int k = tid; k < n; k += NT) {
        const int v = s_seq[canonical_index(p0, fwd, k, n)];
        s_tour[k] = v;
        s_pos[v] = k;
        out[k] = v;
    }
    __syncthreads();

    // ---- the pairs that are edges: pair k = (tour[k], tour[k+1]), the closing pair k = n - 1
    for (long long e = tid; e < m; e += NT) {
        I.with_ends(e, [&](int a, int b) {
            const int pa = s_pos[a], pb = s_pos[b];
            if (pb == (pa + 1 < n ? pa + 1 : 0)) atomicMin(&s_edge[pa], (int)e);
            else if (pa == (pb + 1 < n ? pb + 1 : 0)) atomicMin(&s_edge[pb], (int)e);
        });
    }
    __syncthreads();
    for (int k = tid; k < n; k += NT) {
        const int e = s_edge[k];
        s_w[k] = e != INT_MAX ? wc[2 * (e0 + e)] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        int missing;
        costs[inst] = sum_tour_pairs(n, [&](int k) { return s_edge[k] != INT_MAX; }, s_w, missing);
        n_missing[inst] = missing;
    }
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_tour_from_votes(const float* vote, const int32_t* uv, const float* wc, const int32_t* seg,
                                      const int32_t* vseg, int B, int n_max, int32_t* tours, float* costs,
                                      int32_t* n_missing, void* stream) {
    if (int rc = vote_entry("tour_from_votes", B, n_max)) return rc;
    if (B == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(vote && uv && wc && seg && vseg && tours && costs && n_missing, "tour_from_votes: null pointer");
    hipStream_t st = as_stream(stream);
    if (n_max <= 64)
        tour_from_votes_kernel<64><<<(unsigned)B, 64, 0, st>>>(vote, uv, wc, seg, vseg, tours, costs, n_missing);
    else if (n_max <= 128)
        tour_from_votes_kernel<256><<<(unsigned)B, 256, 0, st>>>(vote, uv, wc, seg, vseg, tours, costs, n_missing);
    else
        tour_from_votes_kernel<1024><<<(unsigned)B, 1024, 0, st>>>(vote, uv, wc, seg, vseg, tours, costs, n_missing);
    return launched("tspgnn_tour_from_votes");
}
