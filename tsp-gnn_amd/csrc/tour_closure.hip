// Metric closure of random weight matrices (tspgnn/dataset.py metric_closure; the reference closes its 'random'
// distances under shortest paths with networkx, dataset.py:85-101):
//   tspgnn_metric_closure   batched Floyd-Warshall in fp64, in place, one workgroup per instance.
// The result is DEFINED as dataset.floyd_warshall on the host: diagonal 0, then for k = 0 .. n-1 in ascending order
// D[i][j] = min(D[i][j], D[i][k] + D[k][j]) with the sum rounded once in fp64, then diagonal 0.  There is no multiply, so
// nothing contracts into an FMA, and a minimum of two finite numbers is exact: the bits do not depend on how the elements
// of a step are shared out, so both tiers below, any workgroup size and any neighbours in the batch give the same matrix.
//
// Two tiers, picked by the launch's n_max:
//   LDS     8 n_max^2 <= kLdsBytes (n_max <= kClosureLdsMaxN = 143): the whole matrix is staged into dynamic LDS, closed
//           there and written back once;
//   global  larger n_max, up to kClosureMaxN = 256 (512 KB at n = 256, more than a CU's LDS or registers hold): the matrix
//           stays where it is.  A workgroup's waves run on one CU and share its vector L1, and __syncthreads() orders
//           their global accesses at workgroup scope, so the hand-off between steps needs nothing beyond the barrier.
//
// Termination: every thread of a workgroup runs the k loop exactly n[b] times with one barrier per step; the only return
// before it is taken by the whole workgroup at once (an n the host never sends).  No inter-workgroup communication.
#include "tour_common.h"

namespace tspgnn {
namespace {

constexpr int kClosureMaxN = 256;
constexpr int kClosureThreads = 1024;

constexpr int closure_lds_max_n() {
    int n = 1;
    while ((size_t)(n + 1) * (size_t)(n + 1) * sizeof(double) <= kLdsBytes) ++n;
    return n;
}
constexpr int kClosureLdsMaxN = closure_lds_max_n();   // the kernel has no static LDS: all of kLdsBytes is the matrix's
static_assert(kClosureLdsMaxN == 143, "dataset.CLOSURE_LDS_MAX_N mirrors this");
static_assert((size_t)kClosureLdsMaxN * kClosureLdsMaxN * sizeof(double) <= kLdsBytes &&
                  (size_t)(kClosureLdsMaxN + 1) * (kClosureLdsMaxN + 1) * sizeof(double) > kLdsBytes,
              "the LDS tier's limit is the largest n whose fp64 matrix fits kLdsBytes");

// JPL: columns per lane, ceil(n_max / 64).  A group of G = 64, 32 or 16 lanes (the smallest that covers n, so small
// instances keep their lanes busy) takes whole rows i = r0, r0 + rs, ...; its lanes stride over the columns j.  D[i][k]
// is uniform over the group (an LDS broadcast, one global fetch); a lane's D[k][j] stay in registers across its rows.
template <int JPL, bool kLds>
__global__ __launch_bounds__(kClosureThreads) void metric_closure_kernel(double* Dg, const long long* __restrict__ off,
                                                                         const int* __restrict__ n_arr, int n_max) {
    extern __shared__ double closure_lds[];
    const int n = n_arr[blockIdx.x];
    if (n < 1 || n > n_max) return;   // workgroup-uniform; the host never sends these (every index below stays in bounds)
    double* const g = Dg + off[blockIdx.x];
    double* const D = kLds ? closure_lds : g;
    const int tid = threadIdx.x, nt = blockDim.x;
    if constexpr (kLds) {
        for (int e = tid; e < n * n; e += nt) D[e] = e / n == e % n ? 0.0 : g[e];
    } else {
        for (int i = tid; i < n; i += nt) D[i * n + i] = 0.0;
    }
    __syncthreads();

    const int lg = n > 32 ? 6 : n > 16 ? 5 : 4;
    const int G = 1 << lg;
    const int r0 = tid >> lg, rs = nt >> lg, j0 = tid & (G - 1);
    // One barrier per step.  D[k][k] = 0 and every weight is >= 0, so step k cannot lower an element of row k or of
    // column k (D[k][j] against D[k][k] + D[k][j], D[i][k] against D[i][k] + D[k][k]): threads skip i == k and j == k.
    // What a thread reads from other threads' elements in step k, D[k][j] and D[i][k], is then written by nobody in step
    // k, and the barrier separates step k's reads from step k + 1's writes (and step k's writes from step k + 1's reads
    // of row and column k + 1).  The diagonal is skipped the same way: it is 0 and no sum of weights is below 0, which is
    // also why the definition's second "diagonal to 0" has nothing left to do here.
    for (int k = 0; k < n; ++k) {
        double rk[JPL];
#pragma unroll
        for (int c = 0; c < JPL; ++c) {
            const int j = j0 + c * G;
            rk[c] = j < n ? D[k * n + j] : 0.0;
        }
        for (int i = r0; i < n; i += rs) {
            if (i == k) continue;
            const double dik = D[i * n + k];
#pragma unroll
            for (int c = 0; c < JPL; ++c) {
                const int j = j0 + c * G;
                if (j < n && j != k && j != i) {
                    const double s = dik + rk[c];
                    if (s < D[i * n + j]) D[i * n + j] = s;
                }
            }
        }
        __syncthreads();
    }

    if constexpr (kLds) {   // the loop's last barrier stands between the last step's writes and these reads
        for (int e = tid; e < n * n; e += nt) g[e] = D[e];
    }
}

template <int JPL, bool kLds>
int launch_closure(double* D, const long long* off, const int* n, int count, int n_max, int threads, hipStream_t st) {
    const size_t lds = kLds ? (size_t)n_max * (size_t)n_max * sizeof(double) : 0;
    const int rc = allow_lds(metric_closure_kernel<JPL, kLds>, lds);
    if (rc) return rc;
    metric_closure_kernel<JPL, kLds><<<(unsigned)count, threads, lds, st>>>(D, off, n, n_max);
    return launched("tspgnn_metric_closure");
}

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_metric_closure(double* D, const long long* off, const int* n, int count, int n_max, void* stream) {
    TSPGNN_REQUIRE(count >= 0, "metric_closure: count=%d", count);
    TSPGNN_REQUIRE(n_max >= 1 && n_max <= kClosureMaxN, "metric_closure: n_max=%d not in [1, %d]", n_max, kClosureMaxN);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(D && off && n, "metric_closure: null pointer");
    hipStream_t st = as_stream(stream);
    // workgroup size: enough 16-, 32- or 64-lane groups to share out n_max rows, no more waves than that at the barrier
    if (n_max <= 32) return launch_closure<1, true>(D, off, n, count, n_max, 256, st);
    if (n_max <= 64) return launch_closure<1, true>(D, off, n, count, n_max, 512, st);
    if (n_max <= 128) return launch_closure<2, true>(D, off, n, count, n_max, kClosureThreads, st);
    if (n_max <= kClosureLdsMaxN) return launch_closure<3, true>(D, off, n, count, n_max, kClosureThreads, st);
    return launch_closure<4, false>(D, off, n, count, n_max, kClosureThreads, st);
}
