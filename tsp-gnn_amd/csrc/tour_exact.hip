// Exact tour labels (tspgnn/dataset.py prove_tours, the counterpart of the reference's Concorde call in dataset.py:9-50):
//   tspgnn_tour_branch_bound  depth-first branch and bound on the Held-Karp 1-tree bound, one wave64 (one workgroup) per
//                             instance, the weight matrix and an int8 edge-class matrix resident in LDS.
// The 1-tree, the ascent and the fp64 rebuild with its margin are tour_common.h's, shared with tspgnn_tour_lower_bound;
// the root node is that kernel's computation, so with max_nodes = 1 the two give the same bits.
//
// A node is the list of decisions on its path.  Its class matrix is rebuilt from that list (O(depth + n^2 / 64) LDS
// operations, far below one ascent), so nothing is undone on the way back up.  Rules, all ties to the smaller id:
//   classes      an edge is free, forced or forbidden.  After the path's decisions are applied, a vertex with two forced
//                edges forbids its other edges; a vertex with more than two forced edges, or with fewer than two edges that
//                are not forbidden, makes the node infeasible.  A class matrix that holds no 1-tree does so as well.
//   bound        node_iters ascent steps in fp32 from the parent's best multipliers (lambda = 2 again, the Polyak step
//                towards the incumbent's cost), then Lr = the best multipliers' 1-tree in fp64 less the margin, and not below
//                the parent's Lr (a bound of the parent holds for the child).
//   leaf         Lr >= inc (1 - opt_tol): pruned.  Otherwise, all degrees 2: the 1-tree is a tour, which replaces the
//                incumbent when its cost (fp64, summed in tour order under the fp32 weights) is below inc.
//   branching    at the vertex v of largest 1-tree degree (> 2); e1, e2 = its free tree edges of smallest and second
//                smallest weight W(v, .).  No forced edge at v: children "force e1 and e2", "force e1, forbid e2",
//                "forbid e1", visited in that order.  One forced edge at v: "force e1", "forbid e1".
//   budget       a node that would be branched when max_nodes ascents have run, or at depth kDepth, stays open; so does a
//                node with unvisited children when the budget runs out.  An open node counts with its own Lr.
//   result       lb = min(inc, Lr of every pruned, tour and open node); proved iff no node stayed open.
//
// Termination: the outer loop runs one ascent per trip and stops at max_nodes; the walk to the next child makes at most
// 4 (kDepth + 1) trips (three children or a pop per level); every other loop is bounded by n, node_iters or root_iters.
// There is no inter-workgroup communication.
#include "tour_common.h"

namespace tspgnn {
namespace {

constexpr int kDepth = TSPGNN_BB_MAX_DEPTH;
constexpr int kN = SquareW::kMaxN;
constexpr int K = kN / kWave;
constexpr int kMaxNodes = 65536;

// Row stride of the class matrix in bytes: an odd number of words, so the rows a wave's lanes scan sit on distinct banks.
__host__ __device__ inline int cons_stride(int n_max) { return 4 * (((n_max + 3) / 4) | 1); }

// fp64 cost of tour t under the fp32 weights, summed in tour order; every lane computes the same sum.
__device__ double seq_cost(const SquareW& W, const int* t, int n) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += (double)W(t[k], t[k + 1 < n ? k + 1 : 0]);
    return s;
}

// Decision word of a stack level: v | e1 << 8 | e2 << 16 | children visited << 24; e2 = 0xff: the two-child kind.
__device__ __forceinline__ int dec_v(int d) { return d & 0xff; }
__device__ __forceinline__ int dec_e1(int d) { return (d >> 8) & 0xff; }
__device__ __forceinline__ int dec_e2(int d) { return (d >> 16) & 0xff; }
__device__ __forceinline__ int dec_next(int d) { return (d >> 24) & 0xff; }

// The class matrix of the node whose path is dec[0..depth): every level's last visited child.  nf gets the forced edges
// per vertex.  Returns false when the node is infeasible by the degree rules.
__device__ bool build_classes(const LdsCons& C, int n, const int* dec, int depth, int* nf, int lane) {
    int* words = reinterpret_cast<int*>(C.c);
    for (int e = lane; e < n * (C.s / 4); e += kWave) words[e] = 0;
    wave_sync();
    if (lane == 0) {
        for (int d = 0; d < depth; ++d) {
            const int w = dec[d], v = dec_v(w), e1 = dec_e1(w), e2 = dec_e2(w), child = dec_next(w) - 1;
            int c1, c2 = -1;
            if (e2 != 0xff) {
                c1 = child == 2 ? kEdgeForbidden : kEdgeForced;
                if (child < 2) c2 = child == 0 ? kEdgeForced : kEdgeForbidden;
            } else {
                c1 = child == 0 ? kEdgeForced : kEdgeForbidden;
            }
            C.c[v * C.s + e1] = (int8_t)c1;
            C.c[e1 * C.s + v] = (int8_t)c1;
            if (c2 >= 0) {
                C.c[v * C.s + e2] = (int8_t)c2;
                C.c[e2 * C.s + v] = (int8_t)c2;
            }
        }
    }
    wave_sync();
    int cnt[K], bad = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int v = lane + j * kWave;
        cnt[j] = 0;
        if (v < n) {
            for (int x = 0; x < n; ++x) cnt[j] += C(v, x) == kEdgeForced;
            nf[v] = cnt[j];
            bad |= cnt[j] > 2;
        }
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int v = lane + j * kWave;
        if (v < n && cnt[j] == 2) {   // both tour edges of v are fixed: the others go (two owners may write the same 2)
            for (int x = 0; x < n; ++x) {
                if (x != v && C(v, x) == kEdgeFree) {
                    C.c[v * C.s + x] = (int8_t)kEdgeForbidden;
                    C.c[x * C.s + v] = (int8_t)kEdgeForbidden;
                }
            }
        }
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int v = lane + j * kWave;
        if (v < n) {
            int forb = 0;
            for (int x = 0; x < n; ++x) forb += C(v, x) == kEdgeForbidden;
            bad |= n - 1 - forb < 2;
        }
    }
    return wave_sum(bad) == 0;
}

// The 1-tree tp with all degrees 2 is a Hamiltonian cycle (connected, n edges): t gets it from vertex 0 towards 0's
// smaller neighbour, which is the canonical form.  adj (2 n ints) and cnt (n ints) are scratch.
__device__ void tree_tour(const int* tp, int n, int* adj, int* cnt, int* t, int lane) {
    for (int k = lane; k < n; k += kWave) cnt[k] = 0;
    wave_sync();
    for (int k = lane; k < n; k += kWave) {
        const int a = k < 2 ? 0 : k, b = tp[k];
        adj[2 * a + (atomicAdd(&cnt[a], 1) & 1)] = b;
        adj[2 * b + (atomicAdd(&cnt[b], 1) & 1)] = a;
    }
    wave_sync();
    int prev = 0, cur = min(adj[0], adj[1]);
    for (int i = 1; i < n; ++i) {   // every lane walks the same cycle; lane 0 records it
        if (lane == 0) t[i] = cur;
        const int nx = adj[2 * cur] == prev ? adj[2 * cur + 1] : adj[2 * cur];
        prev = cur;
        cur = nx;
    }
    if (lane == 0) t[0] = 0;
    wave_sync();
}

__global__ __launch_bounds__(kWave) void tour_branch_bound_kernel(
    const float* __restrict__ Wg, const long long* __restrict__ w_off, const int* __restrict__ n_arr,
    const long long* __restrict__ t_off, const float* __restrict__ upper, int n_max, int root_iters, int node_iters,
    int max_nodes, double opt_tol, float* __restrict__ ws, int32_t* __restrict__ tours, double* __restrict__ lb,
    int32_t* __restrict__ nodes_out, int32_t* __restrict__ status_out) {
    extern __shared__ float lds[];
    __shared__ int deg[kN], tp[kN], nf[kN], cnt[kN], adj[2 * kN], inc_t[kN], new_t[kN], s_dec[kDepth];
    __shared__ double s_lr[kDepth];
    const int inst = blockIdx.x, lane = threadIdx.x;
    const int n = n_arr[inst];
    const double dinf = __longlong_as_double(0x7ff0000000000000ll);
    int32_t* tg = tours + t_off[inst];
    // the incumbent must be a permutation of 0..n-1: every later LDS index comes from it
    if (never_sent(n, n_max) || !load_permutation(tg, inc_t, cnt, n, lane)) {
        if (lane == 0) {
            refuse(&lb[inst]);
            nodes_out[inst] = 0;
            status_out[inst] = TSPGNN_BB_BAD;
        }
        return;
    }
    const SquareW W = SquareW::stage(lds, Wg + w_off[inst], n, lane, kWave);
    const LdsCons C = {reinterpret_cast<int8_t*>(lds + SquareW::floats(n_max)), cons_stride(n_max)};
    float* pst = ws + (size_t)inst * kDepth * n_max;   // level d's multipliers: pst[d * n_max + vertex]
    __syncthreads();
    build_classes(C, n, s_dec, 0, nf, lane);           // all free: what the root branches on
    double inc = seq_cost(W, inc_t, n);

    // root: the bound kernel's ascent and rebuild
    float pi[K], bp[K];
#pragma unroll
    for (int j = 0; j < K; ++j) pi[j] = 0.f;
    ascend(W, NoCons{}, n, upper ? upper[inst] : (float)inc, root_iters, lane, deg, pi, bp);
    double Lr = rebuilt_bound(W, NoCons{}, n, bp, lane, deg, tp);
    bool feasible = true, open = false;
    double lbmin = dinf;
    int depth = 0, nodes = 1;

    for (int trip = 0; trip < max_nodes; ++trip) {
        // ---- the node just bounded: leaf, or one more stack level
        if (feasible) {
            int g2 = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int g = lane + j * kWave < n ? deg[lane + j * kWave] - 2 : 0;
                g2 += g * g;
            }
            int e1 = INT_MAX, e2 = INT_MAX, bv = INT_MAX;
            if (Lr >= inc * (1.0 - opt_tol)) {
                lbmin = fmin(lbmin, Lr);
            } else if (wave_sum(g2) == 0) {
                tree_tour(tp, n, adj, cnt, new_t, lane);
                const double c = seq_cost(W, new_t, n);
                if (c < inc) {
                    inc = c;
                    for (int k = lane; k < n; k += kWave) inc_t[k] = new_t[k];
                    wave_sync();
                }
                lbmin = fmin(lbmin, Lr);
            } else {
                if (nodes < max_nodes && depth < kDepth) {
                    int nd = 0;   // minus the largest degree, then the smallest such vertex
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const int v = lane + j * kWave;
                        if (v < n && -deg[v] < nd) {
                            nd = -deg[v];
                            bv = v;
                        }
                    }
                    wave_argmin(nd, bv);
                    // its free tree edges (edge k of the 1-tree is (k < 2 ? 0 : k, tp[k])), by weight
                    float cw[K];
                    int cx[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        const int k = lane + j * kWave;
                        cw[j] = FLT_MAX;
                        cx[j] = INT_MAX;
                        if (k < n) {
                            const int a = k < 2 ? 0 : k, b = tp[k];
                            if (a == bv || b == bv) {
                                const int x = a == bv ? b : a;
                                if (C(bv, x) == kEdgeFree) {
                                    cw[j] = W(bv, x);
                                    cx[j] = x;
                                }
                            }
                        }
                    }
                    float m = FLT_MAX;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if (cx[j] != INT_MAX && (cw[j] < m || (cw[j] == m && cx[j] < e1))) {
                            m = cw[j];
                            e1 = cx[j];
                        }
                    }
                    wave_argmin(m, e1);
                    m = FLT_MAX;
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if (cx[j] != INT_MAX && cx[j] != e1 && (cw[j] < m || (cw[j] == m && cx[j] < e2))) {
                            m = cw[j];
                            e2 = cx[j];
                        }
                    }
                    wave_argmin(m, e2);
                }
                const int forced = bv != INT_MAX ? nf[bv] : 0;
                if (e1 == INT_MAX || (forced == 0 && e2 == INT_MAX)) {   // out of budget or depth: the node stays open
                    lbmin = fmin(lbmin, Lr);
                    open = true;
                } else {
                    if (lane == 0) {
                        s_dec[depth] = bv | (e1 << 8) | ((forced == 0 ? e2 : 0xff) << 16);
                        s_lr[depth] = Lr;
                    }
#pragma unroll
                    for (int j = 0; j < K; ++j)
                        if (lane + j * kWave < n) pst[(size_t)depth * n_max + lane + j * kWave] = bp[j];
                    ++depth;
                    wave_sync();
                }
            }
        }
        // ---- walk to the next child that has a class matrix, and bound it
        bool have = false;
        for (int s = 0; s < 4 * (kDepth + 1) && depth > 0; ++s) {
            const int w = s_dec[depth - 1], next = dec_next(w);
            const double plr = s_lr[depth - 1];
            if (next >= (dec_e2(w) != 0xff ? 3 : 2)) {
                --depth;
                continue;
            }
            if (nodes >= max_nodes) {   // children left unvisited: the node counts with its own bound
                lbmin = fmin(lbmin, plr);
                open = true;
                --depth;
                continue;
            }
            if (plr >= inc * (1.0 - opt_tol)) {   // the incumbent has improved since: the rest of the node is pruned
                lbmin = fmin(lbmin, plr);
                --depth;
                continue;
            }
            wave_sync();
            if (lane == 0) s_dec[depth - 1] = w + (1 << 24);
            wave_sync();
            if (!build_classes(C, n, s_dec, depth, nf, lane)) continue;
#pragma unroll
            for (int j = 0; j < K; ++j)
                pi[j] = lane + j * kWave < n ? pst[(size_t)(depth - 1) * n_max + lane + j * kWave] : 0.f;
            const float best = ascend(W, C, n, (float)inc, node_iters, lane, deg, pi, bp);
            ++nodes;
            feasible = best < FLT_MAX;
            if (feasible) {
                Lr = rebuilt_bound(W, C, n, bp, lane, deg, tp);
                feasible = Lr < (double)FLT_MAX;
                Lr = fmax(Lr, plr);
            }
            have = true;
            break;
        }
        if (!have) break;
    }
    // (not reached with the bounds above: levels still on the stack count as open)
    for (int d = 0; d < depth; ++d) {
        lbmin = fmin(lbmin, s_lr[d]);
        open = true;
    }
    write_canonical(inc_t, n, tg, lane);
    if (lane == 0) {
        lb[inst] = fmin(inc, lbmin);
        nodes_out[inst] = nodes;
        status_out[inst] = open ? TSPGNN_BB_BUDGET : TSPGNN_BB_PROVED;
    }
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" long long tspgnn_tour_branch_bound_ws(int n_inst, int n_max) {
    if (n_inst <= 0 || n_max < 4 || n_max > kN) return 0;
    return (long long)n_inst * kDepth * n_max * (long long)sizeof(float);
}

extern "C" int tspgnn_tour_branch_bound(const float* W, const long long* w_off, const int* n, const long long* t_off,
                                        const float* upper, int n_inst, int n_max, int root_iters, int node_iters,
                                        int max_nodes, double opt_tol, void* workspace, int32_t* tours, double* lb,
                                        int32_t* nodes, int32_t* status, void* stream) {
    const char* what = "tour_branch_bound";
    TSPGNN_REQUIRE(n_inst >= 0, "%s: n_inst=%d", what, n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    int rc = check_layout<SquareW>(what, n_max);
    if (rc) return rc;
    TSPGNN_REQUIRE(root_iters >= 1 && node_iters >= 1, "%s: root_iters=%d, node_iters=%d", what, root_iters, node_iters);
    TSPGNN_REQUIRE(max_nodes >= 1 && max_nodes <= kMaxNodes, "%s: max_nodes=%d not in [1, %d]", what, max_nodes,
                   kMaxNodes);
    TSPGNN_REQUIRE(opt_tol >= 0.0 && opt_tol < (double)FLT_MAX, "%s: opt_tol=%g must be finite and >= 0", what, opt_tol);
    TSPGNN_REQUIRE(W && w_off && n && t_off && workspace && tours && lb && nodes && status, "%s: null pointer", what);
    const size_t lds = SquareW::floats(n_max) * sizeof(float) + (size_t)n_max * cons_stride(n_max);
    rc = allow_lds(tour_branch_bound_kernel, lds);
    if (rc) return rc;
    tour_branch_bound_kernel<<<(unsigned)n_inst, kWave, lds, as_stream(stream)>>>(
        W, w_off, n, t_off, upper, n_max, root_iters, node_iters, max_nodes, opt_tol, static_cast<float*>(workspace), tours,
        lb, nodes, status);
    return launched("tspgnn_tour_branch_bound");
}
