// tspgnn_vote_scores_i32 and tspgnn_tour_beam (tspgnn/decode.py): beam search over the network's per-edge logits.  Where
// tspgnn_tour_from_votes (tour_decode.hip) commits to one edge at a time, this keeps the `beam` best partial paths from
// vertex 0 under the sum of the edges' integer log-probabilities and closes the best, or the cheapest, of the survivors.
//
// Scores.  q(v) = clamp(rint(65536 * logsigmoid(v)), -2^22, 0) as int32, logsigmoid(v) = min(v, 0) - log1p(exp(-|v|))
// in fp64, rounded half to even; NaN gives -2^22.  A tour has at most 256 edges, so every sum of scores lies in
// [-2^30, 0]: exact integer arithmetic that a restatement reproduces bit for bit.
//
// include/tspgnn.h DEFINES the result of tspgnn_tour_beam as a sequential process: the batch, the pairs e(a,b), the
// ascending key and the tour's outputs under "tours from the edge votes", then this entry point's Lists, Stranded and
// Final.  It depends on the instance, its scores, beam and select alone: never on n_max, on the other instances, on the
// workgroup shape or on what the workspace held.
//
// Layout.  One workgroup per instance: 256 / 512 / 1024 threads and visited masks of 1 / 2 / 4 64-bit words for
// n_max <= 64 / 128 / 256.  The workspace holds, per instance, two dense n_max x n_max tables -- q(a,b) (INT_MIN = no
// edge) and w(a,b) -- built once from the edge list through an atomicMin over edge ids (a minimum: the arrival order
// never reaches it), the parent trace (n_max x beam words: parent index and vertex of every list entry) and a path
// buffer of n_max x beam bytes for the costs of select = 1.  LDS holds the two lists (S, last vertex, mask per entry,
// double-buffered), the 2 048-bin histogram of the radix select and the at most `beam` keys of the chosen candidates.
// A step is an exact top-`beam` under the composite key (-score) << 18 | i << 8 | u (49 bits, ascending = the order
// of Lists, all keys distinct).  The candidates are never stored: every pass recomputes them from the lists and the q table,
// a wave taking entries and its lanes the vertices.  The first pass finds their number and the smallest and largest key
// (register minima, one LDS atomic each per wave).  With more candidates than `beam`, a radix select of 11 bits per pass
// on key - smallest, starting at the digit that holds the highest bit of the span, finds the threshold; it ends as soon
// as the bin it lands in holds exactly the entries still wanted.  (Digits from the top of the 49 bits would put every
// candidate of the early passes into one bin, and 64 lanes adding to one LDS word serialise.)  The candidates at or
// below the threshold are gathered through an LDS counter, in arrival order, and then sorted by a bitonic network,
// which removes that order.  A list of one entry (beam = 1) needs neither: its survivor is the smallest key.
//
// Termination: n - 1 steps of at most 7 passes over the candidates; every loop is bounded by n, beam, m or the 2 048
// bins; the trace walks take at most n steps.  No communication between workgroups.  Contraction is off as in
// tour_decode.hip.
#include "vote_common.h"

#pragma clang fp contract(off)

namespace tspgnn {
namespace {

constexpr int kBeamMax = 1024;
constexpr int kScoreMin = -(1 << 22);
constexpr int kNoPair = INT_MIN;      // q table: no edge joins the pair
constexpr int kBins = 2048;           // 11 bits per radix pass
constexpr int kIdBits = 18;           // i << 8 | u below the score

__global__ __launch_bounds__(256) void vote_scores_kernel(const float* __restrict__ vote, long long M,
                                                          int32_t* __restrict__ score) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= M) return;
    const double v = (double)vote[e];
    int q = kScoreMin;
    if (v == v) {
        const double ls = fmin(v, 0.0) - log1p(exp(-fabs(v)));
        const double s = rint(65536.0 * ls);
        q = s < (double)kScoreMin ? kScoreMin : (s > 0.0 ? 0 : (int)s);
    }
    score[e] = q;
}

__host__ __device__ inline int clamp_score(int s) { return s < kScoreMin ? kScoreMin : (s > 0 ? 0 : s); }

// per-instance workspace: the q table, the w table, the trace, the path buffer, each from a 16-byte boundary
struct BeamWs {
    size_t table, trace, path, total;
};
inline BeamWs beam_ws(int n_max, int beam) {
    BeamWs w;
    w.table = (size_t)n_max * n_max * 4;
    w.trace = (size_t)n_max * beam * 4;
    w.path = ((size_t)n_max * beam + 15) & ~(size_t)15;
    w.total = 2 * w.table + w.trace + w.path;
    return w;
}

// LDS: keys [P] u64, masks [2][P][W] u64, S [2][P], last [2][P], hist [kBins], then the fixed tail
inline int pow2_at_least(int x) {
    int p = 2;
    while (p < x) p <<= 1;
    return p;
}
inline size_t beam_lds_bytes(int P, int W) {
    return (size_t)P * 8 + (size_t)2 * P * W * 8 + (size_t)4 * P * 4 + kBins * 4 + 3 * kVoteMaxN * 4;
}

template <int NT, int W>
__global__ __launch_bounds__(NT) void tour_beam_kernel(const int32_t* __restrict__ score, const int32_t* __restrict__ uv,
                                                       const float* __restrict__ wc, const int32_t* __restrict__ seg,
                                                       const int32_t* __restrict__ vseg, int stride, int beam, int P,
                                                       int select, unsigned char* __restrict__ workspace,
                                                       size_t ws_table, size_t ws_trace, size_t ws_total,
                                                       int32_t* __restrict__ tours, float* __restrict__ costs,
                                                       int32_t* __restrict__ n_missing, int32_t* __restrict__ scores,
                                                       int32_t* __restrict__ n_closed) {
    constexpr int kWaves = NT / kWave;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(lds);
    unsigned long long* s_mask = s_key + P;                              // [2][P][W]
    int* s_S = reinterpret_cast<int*>(s_mask + (size_t)2 * P * W);      // [2][P]
    int* s_last = s_S + 2 * P;                                          // [2][P]
    unsigned* s_hist = reinterpret_cast<unsigned*>(s_last + 2 * P);     // [kBins]
    int* s_seq = reinterpret_cast<int*>(s_hist + kBins);                // [256] the chosen path, then the tour
    float* s_w = reinterpret_cast<float*>(s_seq + kVoteMaxN);           // [256] weight of pair k
    int* s_ex = reinterpret_cast<int*>(s_w + kVoteMaxN);                // [256] pair k is an edge
    __shared__ int s_ctl[3];                                            // bin, below, count of a pass
    __shared__ unsigned s_cnt;
    __shared__ unsigned long long s_best, s_worst;
    __shared__ int s_nclosed;

    const int inst = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const VoteInstance I(uv, seg, vseg, inst);
    const int v0 = I.v0, n = I.n;
    const long long e0 = I.e0, m = I.m;
    // the host module never sends these; a defensive no-op keeps every LDS and workspace index in bounds
    if (n < 4 || n > kVoteMaxN || n > stride || n > 64 * W || m < 0) {
        if (tid == 0) {
            refuse_tour(costs + inst, n_missing + inst);
            scores[inst] = 0;
            n_closed[inst] = -1;
        }
        return;
    }
    unsigned char* ws = workspace + (size_t)inst * ws_total;
    int* qtab = reinterpret_cast<int*>(ws);
    int* etab = reinterpret_cast<int*>(ws + ws_table);       // edge ids while the tables are built, then the weights
    float* wtab = reinterpret_cast<float*>(ws + ws_table);
    uint32_t* trace = reinterpret_cast<uint32_t*>(ws + 2 * ws_table);
    unsigned char* pathbuf = ws + 2 * ws_table + ws_trace;

    // ---- the pair tables: smallest edge id per pair, then its clamped score and its weight
    for (int x = tid; x < n * n; x += NT) etab[(x / n) * stride + x % n] = INT_MAX;
    __threadfence();
    __syncthreads();
    for (long long e = tid; e < m; e += NT) {
        I.with_ends(e, [&](int a, int b) {
            atomicMin(&etab[a * stride + b], (int)e);
            atomicMin(&etab[b * stride + a], (int)e);
        });
    }
    __threadfence();
    __syncthreads();
    __threadfence();   // the atomics ran in the L2: no stale line of the table may answer the reads below
    for (int x = tid; x < n * n; x += NT) {
        const int at = (x / n) * stride + x % n;
        const int e = etab[at];
        qtab[at] = e != INT_MAX ? clamp_score(score[e0 + e]) : kNoPair;
        wtab[at] = e != INT_MAX ? wc[2 * (e0 + e)] : 0.f;
    }
    if (tid == 0) {
        s_S[0] = 0;
        s_last[0] = 0;
        for (int w = 0; w < W; ++w) s_mask[w] = w == 0 ? 1ull : 0ull;
    }
    __syncthreads();

    // f(key) for every candidate of the list `cur` of L entries: a wave per entry, a lane per vertex (u = lane + 64 w
    // lies in mask word w at bit `lane`).  A wave takes kEntries entries at once, so that a lane has up to 8 reads of the q
    // table in flight before the first key is formed; a visited vertex costs no read.
    int cur = 0, L = 1;
    constexpr int kEntries = 8 / W;
    auto for_candidates = [&](auto&& f) {
        for (int i0 = wave; i0 < L; i0 += kEntries * kWaves) {
            int q[kEntries][W], S[kEntries];
#pragma unroll
            for (int x = 0; x < kEntries; ++x) {
                const bool have = i0 + x * kWaves < L;
                const int at = cur * P + (have ? i0 + x * kWaves : 0);
                S[x] = s_S[at];
                const int* qrow = qtab + s_last[at] * stride;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const int u = lane + kWave * w;
                    const bool open = have && u < n && !((s_mask[(size_t)at * W + w] >> lane) & 1ull);
                    q[x][w] = open ? qrow[u] : kNoPair;
                }
            }
#pragma unroll
            for (int x = 0; x < kEntries; ++x) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (q[x][w] != kNoPair)
                        f(((unsigned long long)(unsigned)(-(S[x] + q[x][w])) << kIdBits) |
                          (unsigned long long)(((i0 + x * kWaves) << 8) | (lane + kWave * w)));
                }
            }
        }
    };

    int steps = 0;   // lists built: cur holds L_steps
    bool stranded = false;
    for (int k = 0; k < n - 1; ++k) {
        // ---- the range of the candidate keys and their number: per lane, per wave, then one LDS atomic each per wave
        if (tid == 0) {
            s_best = ~0ull;
            s_worst = 0;
            s_cnt = 0;
        }
        __syncthreads();
        {
            unsigned long long lo = ~0ull, hi = 0;
            int c = 0;
            for_candidates([&](unsigned long long key) {
                lo = key < lo ? key : lo;
                hi = key > hi ? key : hi;
                ++c;
            });
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
                lo = ol < lo ? ol : lo;
                hi = oh > hi ? oh : hi;
                c += __shfl_xor(c, off);
            }
            if (lane == 0 && c > 0) {
                atomicMin(&s_best, lo);
                atomicMax(&s_worst, hi);
                atomicAdd(&s_cnt, (unsigned)c);
            }
        }
        __syncthreads();
        const unsigned long long kmin = s_best, span = s_worst - kmin;
        const int total = (int)s_cnt;
        if (total == 0) {   // workgroup-uniform
            stranded = true;
            break;
        }
        const int newL = min(beam, total);
        __syncthreads();   // s_cnt is read: the gather below counts from 0 again
        if (newL == 1) {
            if (tid == 0) s_key[0] = kmin;   // the one survivor is the smallest key
        } else {
            if (tid == 0) s_cnt = 0;
            // ---- radix select on key - kmin, from the digit that holds the highest bit of the span: the threshold T
            // with exactly newL candidates at or below it.  (total <= beam: every candidate survives, T stays all ones.)
            unsigned long long prefix = 0, T = ~0ull;
            int want = newL;
            const int passes = total <= beam ? 0 : (64 - __clzll((long long)(span | 1ull)) + 10) / 11;
            for (int pass = 0; pass < passes; ++pass) {
                const int shift = 11 * (passes - 1 - pass);
                for (int x = tid; x < kBins; x += NT) s_hist[x] = 0;
                __syncthreads();
                for_candidates([&](unsigned long long key) {
                    const unsigned long long rel = key - kmin;
                    if (pass == 0 || (rel >> (shift + 11)) == prefix)
                        atomicAdd(&s_hist[(rel >> shift) & (kBins - 1)], 1u);
                });
                __syncthreads();
                if (wave == 0) {   // the bin in which the running count reaches `want`
                    int part = 0;
                    for (int x = 0; x < kBins / kWave; ++x)   // rotated by the lane: the lanes read distinct banks
                        part += (int)s_hist[lane * (kBins / kWave) + ((x + lane) & (kBins / kWave - 1))];
                    int incl = part;
#pragma unroll
                    for (int off = 1; off < kWave; off <<= 1) {
                        const int o = __shfl_up(incl, off);
                        if (lane >= off) incl += o;
                    }
                    const unsigned long long bal = __ballot(incl >= want);
                    if (bal != 0 && lane == __ffsll((long long)bal) - 1) {
                        int run = incl - part;
                        for (int x = 0; x < kBins / kWave; ++x) {
                            const int c = (int)s_hist[lane * (kBins / kWave) + x];
                            if (run + c >= want) {
                                s_ctl[0] = lane * (kBins / kWave) + x;
                                s_ctl[1] = run;
                                s_ctl[2] = c;
                                break;
                            }
                            run += c;
                        }
                    }
                }
                __syncthreads();
                const int bin = s_ctl[0], below = s_ctl[1], cnt = s_ctl[2];
                prefix = (prefix << 11) | (unsigned long long)bin;
                const int left = want - below;   // entries wanted from this bin
                if (cnt == left || pass == passes - 1) {
                    T = shift == 0 ? prefix : (((prefix + 1) << shift) - 1);   // the whole bin
                    break;
                }
                want = left;
            }

            // ---- gather the survivors and sort them
            const int P2 = min(P, 1 << (32 - __clz(newL - 1)));   // power of two >= newL >= 2
            for (int x = tid; x < P2; x += NT) s_key[x] = ~0ull;
            __syncthreads();
            for_candidates([&](unsigned long long key) {
                if (key - kmin <= T) {
                    const unsigned at = atomicAdd(&s_cnt, 1u);
                    if (at < (unsigned)P) s_key[at] = key;
                }
            });
            __syncthreads();
            for (int k2 = 2; k2 <= P2; k2 <<= 1) {
                for (int j = k2 >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < P2; t += NT) {
                        const int o = t ^ j;
                        if (o > t) {
                            const unsigned long long a = s_key[t], b = s_key[o];
                            if ((a > b) == ((t & k2) == 0)) {
                                s_key[t] = b;
                                s_key[o] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        // ---- build L_{k+1}
        const int nxt = cur ^ 1;
        for (int j = tid; j < newL; j += NT) {
            const unsigned long long key = s_key[j];
            const int i = (int)((key >> 8) & 1023u), u = (int)(key & 255u);
            s_S[nxt * P + j] = -(int)(unsigned)(key >> kIdBits);
            s_last[nxt * P + j] = u;
            for (int w = 0; w < W; ++w)
                s_mask[((size_t)nxt * P + j) * W + w] =
                    s_mask[((size_t)cur * P + i) * W + w] | (w == (u >> 6) ? 1ull << (u & 63) : 0ull);
            trace[(size_t)k * beam + j] = (uint32_t)(key & ((1u << kIdBits) - 1));
        }
        __syncthreads();
        cur = nxt;
        L = newL;
        steps = k + 1;
    }

    // vertices 1 .. steps of entry j of L_steps, read back through the trace; put(position, vertex)
    auto walk = [&](int j, auto&& put) {
        for (int pos = steps; pos >= 1; --pos) {
            const uint32_t t = trace[(size_t)(pos - 1) * beam + j];
            put(pos, (int)(t & 255u));
            j = (int)(t >> 8);
        }
    };

    int score_out = 0, closed_out = 0;
    if (stranded) {
        if (tid == 0) {
            s_seq[0] = 0;
            walk(0, [&](int pos, int v) { s_seq[pos] = v; });
            int at = steps + 1;
            const unsigned long long* mk = s_mask + (size_t)cur * P * W;
            for (int v = 0; v < n; ++v)
                if (!((mk[v >> 6] >> (v & 63)) & 1ull) && at < n) s_seq[at++] = v;
        }
        score_out = s_S[cur * P];
    } else {
        if (tid == 0) {
            s_best = ~0ull;
            s_nclosed = 0;
        }
        __syncthreads();
        for (int j = tid; j < L; j += NT) {
            const int q0 = qtab[s_last[cur * P + j] * stride];
            const bool closed = q0 != kNoPair;
            unsigned long long key = closed ? 0ull : 1ull << 62;
            if (select == 0) {
                key |= (unsigned long long)(unsigned)(-(s_S[cur * P + j] + (closed ? q0 : 0))) << 10;
            } else {
                pathbuf[j] = 0;
                walk(j, [&](int pos, int v) { pathbuf[(size_t)pos * beam + j] = (unsigned char)v; });
                const bool fwd = pathbuf[(size_t)beam + j] < pathbuf[(size_t)(n - 1) * beam + j];
                float c = 0.f;
                int a = 0;
                for (int p = 1; p < n; ++p) {
                    const int b = pathbuf[(size_t)canonical_index_from0(fwd, p, n) * beam + j];
                    if (qtab[a * stride + b] != kNoPair) c += wtab[a * stride + b];
                    a = b;
                }
                if (qtab[a * stride] != kNoPair) c += wtab[a * stride];
                key |= (unsigned long long)ordered_key(c, kNanHighest) << 10;   // ascending, a NaN after every number
            }
            atomicMin(&s_best, key | (unsigned long long)j);
            if (closed) atomicAdd(&s_nclosed, 1);
        }
        __syncthreads();
        const int js = (int)(s_best & 1023u);
        const int q0 = qtab[s_last[cur * P + js] * stride];
        score_out = s_S[cur * P + js] + (q0 != kNoPair ? q0 : 0);
        closed_out = s_nclosed;
        if (select == 0) {
            if (tid == 0) {
                s_seq[0] = 0;
                walk(js, [&](int pos, int v) { s_seq[pos] = v; });
            }
        } else {
            for (int p = tid; p < n; p += NT) s_seq[p] = pathbuf[(size_t)p * beam + js];
        }
    }
    __syncthreads();

    // ---- canonical form (the path starts at vertex 0), the pairs that are edges, the cost
    const bool fwd = s_seq[1] < s_seq[n - 1];
    int mine[kVoteMaxN / 64];   // tour[tid], tour[tid + NT], ...: at most 256 / 256 = 1 .. 4 entries for NT >= 256
    int cnt = 0;
    for (int p = tid; p < n; p += NT) mine[cnt++] = s_seq[p == 0 ? 0 : canonical_index_from0(fwd, p, n)];
    __syncthreads();
    cnt = 0;
    int32_t* out = tours + v0;
    for (int p = tid; p < n; p += NT) {
        s_seq[p] = mine[cnt];
        out[p] = mine[cnt++];
    }
    __syncthreads();
    for (int p = tid; p < n; p += NT) {
        const int at = s_seq[p] * stride + s_seq[p + 1 < n ? p + 1 : 0];
        s_ex[p] = qtab[at] != kNoPair;
        s_w[p] = wtab[at];
    }
    __syncthreads();
    if (tid == 0) {
        int missing;
        costs[inst] = sum_tour_pairs(n, [&](int p) { return s_ex[p] != 0; }, s_w, missing);
        n_missing[inst] = missing;
        scores[inst] = score_out;
        n_closed[inst] = closed_out;
    }
}

template <int NT, int W>
int launch_beam(const int32_t* score, const int32_t* uv, const float* wc, const int32_t* seg, const int32_t* vseg, int B,
                int n_max, int beam, int select, void* workspace, int32_t* tours, float* costs, int32_t* n_missing,
                int32_t* scores, int32_t* n_closed, hipStream_t st) {
    const int P = pow2_at_least(beam);
    const size_t lds = beam_lds_bytes(P, W);
    if (int rc = allow_lds(tour_beam_kernel<NT, W>, lds)) return rc;
    const BeamWs w = beam_ws(n_max, beam);
    tour_beam_kernel<NT, W><<<(unsigned)B, NT, lds, st>>>(score, uv, wc, seg, vseg, n_max, beam, P, select,
                                                          static_cast<unsigned char*>(workspace), w.table, w.trace,
                                                          w.total, tours, costs, n_missing, scores, n_closed);
    return launched("tspgnn_tour_beam");
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_vote_scores_i32(const float* vote, long long M, int32_t* score, void* stream) {
    TSPGNN_REQUIRE(M >= 0, "vote_scores: M=%lld", M);
    if (M == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(vote && score, "vote_scores: null pointer");
    TSPGNN_REQUIRE(M <= 0x7fffffffLL * 256, "vote_scores: M=%lld", M);
    vote_scores_kernel<<<(unsigned)((M + 255) / 256), 256, 0, as_stream(stream)>>>(vote, M, score);
    return launched("tspgnn_vote_scores_i32");
}

extern "C" long long tspgnn_tour_beam_workspace_bytes(int B, int n_max, int beam) {
    if (B <= 0 || n_max < 4 || n_max > kVoteMaxN || beam < 1 || beam > kBeamMax) return 0;
    return (long long)B * (long long)beam_ws(n_max, beam).total;
}

extern "C" int tspgnn_tour_beam(const int32_t* score, const int32_t* uv, const float* wc, const int32_t* seg,
                                const int32_t* vseg, int B, int n_max, int beam, int select, void* workspace,
                                long long workspace_bytes, int32_t* tours, float* costs, int32_t* n_missing,
                                int32_t* scores, int32_t* n_closed, void* stream) {
    if (int rc = vote_entry("tour_beam", B, n_max, "beam", beam, kBeamMax)) return rc;
    if (B == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(beam >= 1, "tour_beam: beam=%d must be at least 1", beam);
    TSPGNN_REQUIRE(select == 0 || select == 1, "tour_beam: select=%d is neither 0 (score) nor 1 (cost)", select);
    TSPGNN_REQUIRE(score && uv && wc && seg && vseg && workspace && tours && costs && n_missing && scores && n_closed,
                   "tour_beam: null pointer");
    const long long need = tspgnn_tour_beam_workspace_bytes(B, n_max, beam);
    TSPGNN_REQUIRE(workspace_bytes >= need, "tour_beam: workspace of %lld bytes, %lld needed", workspace_bytes, need);
    TSPGNN_REQUIRE(((uintptr_t)workspace & 15) == 0, "tour_beam: the workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (n_max <= 64)
        return launch_beam<256, 1>(score, uv, wc, seg, vseg, B, n_max, beam, select, workspace, tours, costs, n_missing,
                                   scores, n_closed, st);
    if (n_max <= 128)
        return launch_beam<512, 2>(score, uv, wc, seg, vseg, B, n_max, beam, select, workspace, tours, costs, n_missing,
                                   scores, n_closed, st);
    return launch_beam<1024, 4>(score, uv, wc, seg, vseg, B, n_max, beam, select, workspace, tours, costs, n_missing,
                                scores, n_closed, st);
}
