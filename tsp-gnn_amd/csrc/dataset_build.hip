// Labelled instances made on the device from the reference's random streams (tspgnn/device_dataset.py,
// DeviceDataset.generate; dataset.draw_streams makes the 1-D draws on the host, in the reference's order):
//   tspgnn_build_instances     the streams -> per instance the fp64 weight matrix, the symmetric edge mask and m;
//   tspgnn_penalise_instances  (mask, weights) -> the fp32 input of the tour kernels, square or packed triangle;
//   tspgnn_pack_dataset        (mask, weights, tours) -> the arrays of a DeviceDataset and the label's scalars.
// Each result is DEFINED by host code the tests pin: dataset._draw_graph (the matrices), dataset._penalised /
// _penalised_tri (the search input), device_dataset.preprocess (tspgnn_host_stage_batch's edge order and CSR,
// tspgnn_host_route_cost), dataset._cycle_cost.  All of it is element-wise arithmetic, exact reductions (an fp64 maximum,
// integer counts) or a sum one lane takes in the host's order, so the bits do not depend on the mapping:
//   pair k of (i, j > i) in row-major order is k = i (2n - i - 1) / 2 + (j - i - 1);
//   A[i][j] = A[j][i] = adj_u[k] < conn, or {i, j} is an edge of the planted cycle perm[t] - perm[t + 1 mod n];
//   euc_2D: Mw[i][j] = sqrt((x_i - x_j) (x_i - x_j) + (y_i - y_j) (y_i - y_j)), every operation rounded once (the file is
//   compiled with contraction off, so no product joins the sum in an FMA), the square root correctly rounded;
//   random: Mw[i][j] = Mw[j][i] = wts[k];  the diagonal of A and Mw is 0;
//   penalty = n * max(real-edge weight, 0) + 1.0 with two roundings; fp64 -> fp32 rounds to nearest, then steps down one
//   ulp when the result exceeds the fp64 value (written out below: no directed-rounding conversion is relied on).
//
// Mapping: one workgroup of 256 threads per instance, n <= 256.  Instances are described by a table of int64 rows that
// the caller passes twice: on the HOST, where every row is checked against the array sizes before anything is launched,
// and on the DEVICE, where the kernels read it.  Every loop is bounded by n or n^2; every barrier is reached by all
// threads of a workgroup (the only early return is workgroup-uniform, for an n the host check never lets through); no
// inter-workgroup communication; plain per-lane stores to addresses owned by one thread, and in the packing kernel every
// store into the shared dataset arrays is also guarded by the instance's own extent (m edges from e0).
#include "tour_common.h"

#pragma clang fp contract(off)

namespace tspgnn {
namespace {

// One rounding per operation.  The header's __dadd_rn / __dmul_rn are plain operators compiled where contraction is
// allowed, so a product and a sum taken through them may still meet in an FMA; these are compiled under the pragma above.
__device__ __forceinline__ double rn_add(double a, double b) { return a + b; }
__device__ __forceinline__ double rn_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double rn_mul(double a, double b) { return a * b; }

constexpr int kDsMinN = 4;
constexpr int kDsMaxN = 256;
constexpr int kDsThreads = 256;
constexpr int kDsWaves = kDsThreads / kWave;
static_assert(kDsThreads >= kDsMaxN, "the packing kernel gives every vertex a thread");

constexpr int kBuildCols = 4;   // n, first pair, first vertex, first matrix cell
constexpr int kPenCols = 3;     // n, first matrix cell, first output float
constexpr int kPackCols = 7;    // n, first matrix cell, first tour entry, m, first edge e0, first vertex v0, position

__device__ __forceinline__ int pair_index(int lo, int hi, int n) { return lo * (2 * n - lo - 1) / 2 + (hi - lo - 1); }

// ------------------------------------------------------------------------------------------------- 1. the matrices
__global__ __launch_bounds__(kDsThreads) void build_instances_kernel(
    const long long* __restrict__ tab, const double* __restrict__ conn, const double* __restrict__ adj_u,
    const double* __restrict__ coord, const int32_t* __restrict__ perm, int random_w, int n_max, double* __restrict__ Mw,
    uint8_t* __restrict__ A, int32_t* __restrict__ m_out) {
    __shared__ int s_pos[kDsMaxN];     // position of a vertex in the planted cycle
    __shared__ int s_cnt[kDsWaves];
    const long long* row = tab + (long long)kBuildCols * blockIdx.x;
    const int n = (int)row[0];
    if (n < kDsMinN || n > n_max) return;   // workgroup-uniform; the host check never sends these
    const double* u = adj_u + row[1];
    const double* c = coord + (random_w ? row[1] : 2 * row[2]);
    const int32_t* p = perm + row[2];
    double* mw = Mw + row[3];
    uint8_t* a = A + row[3];
    const double cn = conn[blockIdx.x];
    const int tid = threadIdx.x;
    for (int t = tid; t < n; t += kDsThreads) s_pos[t] = -2;
    __syncthreads();
    for (int t = tid; t < n; t += kDsThreads) {
        const int v = p[t];
        if ((unsigned)v < (unsigned)n) s_pos[v] = t;   // a stream that is no permutation plants fewer edges, nothing else
    }
    __syncthreads();
    int cnt = 0;
    for (int e = tid; e < n * n; e += kDsThreads) {
        const int i = e / n, j = e - i * n;
        uint8_t bit = 0;
        double w = 0.0;
        if (i != j) {
            const int lo = min(i, j), hi = max(i, j);
            const int k = pair_index(lo, hi, n);
            const int pi = s_pos[i], pj = s_pos[j];
            const int d = pi > pj ? pi - pj : pj - pi;
            const bool planted = pi >= 0 && pj >= 0 && (d == 1 || d == n - 1);
            bit = (u[k] < cn || planted) ? 1 : 0;
            if (random_w) {
                w = c[k];
            } else {
                const double dx = rn_sub(c[2 * i], c[2 * j]), dy = rn_sub(c[2 * i + 1], c[2 * j + 1]);
                w = __dsqrt_rn(rn_add(rn_mul(dx, dx), rn_mul(dy, dy)));
            }
            cnt += (i < j) ? bit : 0;
        }
        a[e] = bit;
        mw[e] = w;
    }
    cnt = wave_sum(cnt);
    if ((tid & (kWave - 1)) == 0) s_cnt[tid / kWave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int k = 0; k < kDsWaves; ++k) m += s_cnt[k];
        m_out[blockIdx.x] = m;
    }
}

// ------------------------------------------------------------------------------------------------- 2. the search input
// dataset._penalised's conversion: to nearest, then one ulp towards -inf when that went up.
__device__ __forceinline__ float to_float_down(double v) {
    float f = (float)v;
    if ((double)f > v) {
        const unsigned b = __float_as_uint(f);
        f = f > 0.f ? __uint_as_float(b - 1) : f < 0.f ? __uint_as_float(b + 1) : __uint_as_float(0x80000001u);
    }
    return f;
}

template <bool kTri>
__global__ __launch_bounds__(kDsThreads) void penalise_instances_kernel(const long long* __restrict__ tab,
                                                                        const uint8_t* __restrict__ A,
                                                                        const double* __restrict__ Mw, int n_max,
                                                                        float* __restrict__ W) {
    __shared__ double s_max[kDsWaves];
    const long long* row = tab + (long long)kPenCols * blockIdx.x;
    const int n = (int)row[0];
    if (n < kDsMinN || n > n_max) return;   // workgroup-uniform; the host check never sends these
    const uint8_t* a = A + row[1];
    const double* mw = Mw + row[1];
    float* out = W + row[2];
    const int tid = threadIdx.x;
    double mx = 0.0;   // the host's maximum is taken over where(A, w, 0.0)
    for (int e = tid; e < n * n; e += kDsThreads) {
        const int i = e / n, j = e - i * n;
        if (i < j && a[e]) mx = fmax(mx, rn_add(mw[e], 0.0));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
    if ((tid & (kWave - 1)) == 0) s_max[tid / kWave] = mx;
    __syncthreads();
    mx = s_max[0];
    for (int k = 1; k < kDsWaves; ++k) mx = fmax(mx, s_max[k]);
    const double pen = rn_add(rn_mul((double)n, mx), 1.0);
    for (int e = tid; e < n * n; e += kDsThreads) {
        const int i = e / n, j = e - i * n;
        if (kTri && i >= j) continue;
        const int lo = min(i, j), hi = max(i, j);
        const double v = i == j ? 0.0 : a[e] ? rn_add(mw[lo * n + hi], 0.0) : pen;   // + 0.0: -0 becomes +0
        out[kTri ? pair_index(i, j, n) : e] = to_float_down(v);
    }
}

// ------------------------------------------------------------------------------------------------- 3. the dataset arrays
// Exclusive prefix sum of one int per thread over the workgroup (kDsThreads threads, all of them call); *total gets the sum.
__device__ __forceinline__ int block_scan(int v, int* s_w, int tid, int* total) {
    const int lane = tid & (kWave - 1), wv = tid / kWave;
    int x = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == kWave - 1) s_w[wv] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < kDsWaves; ++k) {
        if (k < wv) base += s_w[k];
        tot += s_w[k];
    }
    __syncthreads();   // s_w is free again
    *total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(kDsThreads) void pack_dataset_kernel(
    const long long* __restrict__ tab, const uint8_t* __restrict__ A, const double* __restrict__ Mw,
    const int32_t* __restrict__ tours, int n_max, int2* __restrict__ uv, float* __restrict__ w,
    int32_t* __restrict__ rowptr, int32_t* __restrict__ eid, double* __restrict__ cost, double* __restrict__ file_cost,
    double* __restrict__ cycle_cost, int32_t* __restrict__ feasible) {
    extern __shared__ int32_t pack_lds[];
    __shared__ int s_w[kDsWaves];
    int* s_row = pack_lds;            // [n_max]: edges of the rows above row i, the id of row i's first edge
    int* s_ptr = s_row + n_max;       // [n_max]: the row pointer of vertex v
    int* s_low = s_ptr + n_max;       // [n_max]: neighbours of v below v
    uint8_t* s_rank = reinterpret_cast<uint8_t*>(s_low + n_max);   // [n][n]: rank of edge (i, j > i) inside row i (< 255)
    const long long* row = tab + (long long)kPackCols * blockIdx.x;
    const int n = (int)row[0];
    if (n < kDsMinN || n > n_max) return;   // workgroup-uniform; the host check never sends these
    const uint8_t* a = A + row[1];
    const double* mw = Mw + row[1];
    const int32_t* t = tours + row[2];
    const int m = (int)row[3];
    const long long e0 = row[4], r0 = row[5] + row[6], pos = row[6];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;

    // per vertex: neighbours above and below, read down the column (A is symmetric), which the lanes of a wave share
    int up = 0, low = 0;
    if (tid < n) {
        for (int x = 0; x < n; ++x) {
            const int bit = a[x * n + tid] != 0;
            low += x < tid ? bit : 0;
            up += x > tid ? bit : 0;
        }
    }
    int total, total2;
    const int first = block_scan(up, s_w, tid, &total);
    const int ptr = block_scan(up + low, s_w, tid, &total2);
    if (tid < n) {
        s_row[tid] = first;
        s_ptr[tid] = ptr;
        s_low[tid] = low;
        rowptr[r0 + tid] = ptr;
    }
    if (tid == 0) rowptr[r0 + n] = total2;
    __syncthreads();
    const bool fits = total == m && total2 == 2 * m;   // else the table's m is not this mask's: nothing more is written

    // edges in np.nonzero(np.triu(A)) order: a wave per row, the rank inside the row from a ballot
    for (int i = wv; i < n && fits; i += kDsWaves) {
        int base = 0;
        for (int j0 = i + 1; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            const bool bit = j < n && a[i * n + j] != 0;
            const unsigned long long mask = __ballot(bit);
            if (bit) {
                const int r = base + __popcll(mask & ((1ull << lane) - 1ull));
                const int e = s_row[i] + r, q = s_ptr[i] + s_low[i] + r;
                if (e < m && q < 2 * m) {   // always, for a symmetric mask
                    uv[e0 + e] = make_int2(i, j);
                    w[e0 + e] = (float)mw[i * n + j];
                    eid[2 * e0 + q] = e;   // vertex i: after its edges to lower vertices
                }
                s_rank[i * n + j] = (uint8_t)r;
            }
            base += __popcll(mask);
        }
    }
    __syncthreads();
    // vertex v's edges to lower vertices u, ascending u: ascending edge id, and all of them below row v's own edges
    for (int v = wv; v < n && fits; v += kDsWaves) {
        int base = 0;
        for (int u0 = 0; u0 < v; u0 += kWave) {
            const int x = u0 + lane;
            const bool bit = x < v && a[v * n + x] != 0;
            const unsigned long long mask = __ballot(bit);
            if (bit) {
                const int q = base + __popcll(mask & ((1ull << lane) - 1ull));
                if (q < s_low[v]) eid[2 * e0 + s_ptr[v] + q] = s_row[x] + s_rank[x * n + v];
            }
            base += __popcll(mask);
        }
    }

    // the label's scalars: each a sum one lane takes in the host's order
    if (tid == 0 || tid == 2 * kWave) {   // tspgnn_host_route_cost: on Mw as it is, and on the file form of Mw
        const bool file = tid != 0;          // ... which is zero off the upper-triangular edge set
        double s = 0.0;
        bool bad = false;
        for (int k = 0; k < n; ++k) {
            const int x = t[k], y = k + 1 < n ? t[k + 1] : t[1];
            if ((unsigned)x >= (unsigned)n || (unsigned)y >= (unsigned)n) {
                bad = true;
                break;
            }
            const int lo = min(x, y), hi = max(x, y);
            s = rn_add(s, !file || a[lo * n + hi] ? mw[lo * n + hi] : 0.0);
        }
        (file ? file_cost : cost)[pos] = bad ? __builtin_nan("") : s / (double)n;
    }
    if (tid == kWave) {   // dataset._cycle_cost, and whether every tour edge is real
        double s = 0.0;
        bool bad = false, feas = true;
        for (int k = 0; k < n; ++k) {
            const int x = t[k], y = t[k + 1 < n ? k + 1 : 0];
            if ((unsigned)x >= (unsigned)n || (unsigned)y >= (unsigned)n) {
                bad = true;
                break;
            }
            const int lo = min(x, y), hi = max(x, y);
            s = rn_add(s, mw[lo * n + hi]);
            feas = feas && a[x * n + y] != 0;
        }
        cycle_cost[pos] = bad ? __builtin_nan("") : s;
        feasible[pos] = !bad && feas;
    }
}

size_t pack_lds_bytes(int n_max) { return (size_t)3 * n_max * sizeof(int32_t) + (size_t)n_max * n_max; }
static_assert((size_t)3 * kDsMaxN * sizeof(int32_t) + (size_t)kDsMaxN * kDsMaxN + kDsWaves * sizeof(int) <= kLdsBytes,
              "the packing kernel's LDS at n_max = 256");

// rows [lo, lo + len) must lie in [0, size): the host half of every offset check
bool inside(long long lo, long long len, long long size) { return lo >= 0 && len >= 0 && lo <= size - len; }

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

#define DS_COMMON(name, count, n_max)                                                                        \
    TSPGNN_REQUIRE((count) >= 0, name ": count=%d", (count));                                              \
    TSPGNN_REQUIRE((n_max) >= kDsMinN && (n_max) <= kDsMaxN, name ": n_max=%d not in [%d, %d]", (n_max), kDsMinN, \
                   kDsMaxN);                                                                                 \
    if ((count) == 0) return TSPGNN_OK

extern "C" int tspgnn_build_instances(const long long* tab, const long long* d_tab, const double* conn,
                                      const double* adj_u, const double* coord, const int32_t* perm, int random_weights,
                                      int count, int n_max, long long n_pairs, long long n_verts, long long n_cells,
                                      double* Mw, unsigned char* A, int32_t* m, void* stream) {
    DS_COMMON("build_instances", count, n_max);
    TSPGNN_REQUIRE(tab && d_tab && conn && adj_u && coord && perm && Mw && A && m, "build_instances: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(Mw) % 8 == 0 && reinterpret_cast<uintptr_t>(adj_u) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(coord) % 8 == 0 && reinterpret_cast<uintptr_t>(conn) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 && reinterpret_cast<uintptr_t>(perm) % 4 == 0 &&
                       reinterpret_cast<uintptr_t>(m) % 4 == 0,
                   "build_instances: misaligned array");
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kBuildCols * b;
        TSPGNN_REQUIRE(r[0] >= kDsMinN && r[0] <= n_max, "build_instances: instance %d: n=%lld not in [%d, %d]", b, r[0],
                       kDsMinN, n_max);
        const long long n = r[0];
        TSPGNN_REQUIRE(inside(r[1], n * (n - 1) / 2, n_pairs) && inside(r[2], n, n_verts) && inside(r[3], n * n, n_cells),
                       "build_instances: instance %d: offsets (%lld, %lld, %lld) leave the arrays", b, r[1], r[2], r[3]);
    }
    build_instances_kernel<<<(unsigned)count, kDsThreads, 0, as_stream(stream)>>>(
        d_tab, conn, adj_u, coord, perm, random_weights != 0, n_max, Mw, A, m);
    return launched("tspgnn_build_instances");
}

extern "C" int tspgnn_penalise_instances(const long long* tab, const long long* d_tab, const unsigned char* A,
                                         const double* Mw, int count, int n_max, int triangle, long long n_cells,
                                         long long n_floats, float* W, void* stream) {
    DS_COMMON("penalise_instances", count, n_max);
    TSPGNN_REQUIRE(tab && d_tab && A && Mw && W, "penalise_instances: null pointer");
    TSPGNN_REQUIRE(triangle || n_max <= SquareW::kMaxN, "penalise_instances: the square layout ends at n_max=%d",
                   SquareW::kMaxN);
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(Mw) % 8 == 0 && reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(W) % 4 == 0,
                   "penalise_instances: misaligned array");
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kPenCols * b;
        TSPGNN_REQUIRE(r[0] >= kDsMinN && r[0] <= n_max, "penalise_instances: instance %d: n=%lld not in [%d, %d]", b,
                       r[0], kDsMinN, n_max);
        const long long n = r[0];
        TSPGNN_REQUIRE(inside(r[1], n * n, n_cells) && inside(r[2], triangle ? n * (n - 1) / 2 : n * n, n_floats),
                       "penalise_instances: instance %d: offsets (%lld, %lld) leave the arrays", b, r[1], r[2]);
    }
    if (triangle)
        penalise_instances_kernel<true><<<(unsigned)count, kDsThreads, 0, as_stream(stream)>>>(d_tab, A, Mw, n_max, W);
    else
        penalise_instances_kernel<false><<<(unsigned)count, kDsThreads, 0, as_stream(stream)>>>(d_tab, A, Mw, n_max, W);
    return launched("tspgnn_penalise_instances");
}

extern "C" int tspgnn_pack_dataset(const long long* tab, const long long* d_tab, const unsigned char* A, const double* Mw,
                                   const int32_t* tours, int count, int n_max, long long n_cells, long long n_tour,
                                   long long n_edges, long long n_rowptr, long long n_inst, int32_t* uv, float* w,
                                   int32_t* rowptr, int32_t* eid, double* cost, double* file_cost, double* cycle_cost,
                                   int32_t* feasible, void* stream) {
    DS_COMMON("pack_dataset", count, n_max);
    TSPGNN_REQUIRE(tab && d_tab && A && Mw && tours && rowptr && cost && file_cost && cycle_cost && feasible &&
                       (n_edges == 0 || (uv && w && eid)),
                   "pack_dataset: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(Mw) % 8 == 0 && reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(uv) % 8 == 0 && reinterpret_cast<uintptr_t>(cost) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(file_cost) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(cycle_cost) % 8 == 0 && reinterpret_cast<uintptr_t>(w) % 4 == 0 &&
                       reinterpret_cast<uintptr_t>(rowptr) % 4 == 0 && reinterpret_cast<uintptr_t>(eid) % 4 == 0 &&
                       reinterpret_cast<uintptr_t>(tours) % 4 == 0 && reinterpret_cast<uintptr_t>(feasible) % 4 == 0,
                   "pack_dataset: misaligned array");
    TSPGNN_REQUIRE(n_edges >= 0 && 2 * n_edges < (1ll << 31), "pack_dataset: %lld edges: 2 * sum(m) must stay below 2^31",
                   n_edges);
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kPackCols * b;
        TSPGNN_REQUIRE(r[0] >= kDsMinN && r[0] <= n_max, "pack_dataset: instance %d: n=%lld not in [%d, %d]", b, r[0],
                       kDsMinN, n_max);
        const long long n = r[0];
        TSPGNN_REQUIRE(inside(r[1], n * n, n_cells) && inside(r[2], n, n_tour) && r[3] >= 0 && r[3] <= n * (n - 1) / 2 &&
                           inside(r[4], r[3], n_edges) && r[5] >= 0 && inside(r[6], 1, n_inst) &&
                           inside(r[5] + r[6], n + 1, n_rowptr),
                       "pack_dataset: instance %d: offsets (%lld, %lld, %lld, %lld, %lld, %lld) leave the arrays", b, r[1],
                       r[2], r[3], r[4], r[5], r[6]);
    }
    const size_t lds = pack_lds_bytes(n_max);
    const int rc = allow_lds(pack_dataset_kernel, lds);
    if (rc) return rc;
    pack_dataset_kernel<<<(unsigned)count, kDsThreads, lds, as_stream(stream)>>>(
        d_tab, A, Mw, tours, n_max, reinterpret_cast<int2*>(uv), w, rowptr, eid, cost, file_cost, cycle_cost, feasible);
    return launched("tspgnn_pack_dataset");
}
