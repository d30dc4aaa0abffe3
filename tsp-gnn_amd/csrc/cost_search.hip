// Batched tour-cost binary search: the bracket update of experiments/binary_search.py:53-75 (get_cost's loop) for many
// instances at once, applied on the device after each forward pass so that a whole search round -- forward, vote,
// sigmoid, bracket update, next probe costs -- is one captured graph (tspgnn/binary_search.py, get_costs).
#include "common.h"

namespace tspgnn {

// The probe and stop-test arithmetic must round exactly as the host loop's float64 Python / NumPy does, one IEEE
// operation at a time.  HIP device code contracts a + b*c into an FMA by default (NumPy never does), so contraction is
// off for everything below; fp64 division is IEEE-exact without -ffast-math.
#pragma clang fp contract(off)

// get_cost's loop condition, with w = (hi + lo) / 2.  A NaN bracket compares false: inactive.
__device__ __forceinline__ bool search_active(double lo, double hi, double below, double above) {
    const double w = (hi + lo) / 2.0;
    return lo < w * below || w * above < hi;
}

// Probe cost of graph j of an instance with k probe copies: the midpoint for k == 1 (wpred), else
// lo + (hi - lo) * ((j + 1) / (k + 1.0))  (np.arange(1, k + 1) / (k + 1.0), evaluated per element).
__device__ __forceinline__ double search_probe(double lo, double hi, int j, int k) {
    if (k == 1) return (hi + lo) / 2.0;
    const double frac = (double)(j + 1) / ((double)k + 1.0);
    return lo + (hi - lo) * frac;
}

// One workgroup per instance.  Thread 0 applies the rule; the workgroup then writes the instance's next probe costs
// into column 1 of WC for each of its k graphs' edges.
__global__ __launch_bounds__(256) void cost_search_kernel(double* __restrict__ lo_, double* __restrict__ hi_,
                                                          int* __restrict__ iters, float* __restrict__ pred_out,
                                                          int* __restrict__ n_active, const float* __restrict__ pred,
                                                          float* __restrict__ WC, const int32_t* __restrict__ seg,
                                                          const int* __restrict__ guard, int k, float thr,
                                                          double below, double above, int mode) {
    __shared__ double s_lo, s_hi;
    __shared__ int s_write;
    const int i = blockIdx.x;
    if (threadIdx.x == 0) {
        double lo = lo_[i], hi = hi_[i];
        bool write = false;
        const bool was_active = search_active(lo, hi, below, above);
        // the round's f16x2 forward left the fp16 range, or the one-launch loop timed out: its predictions are not
        // to be trusted -- leave the state alone (the host repeats the round on bf16x3 / raises)
        const bool skip = (guard[0] & 3) != 0 || guard[2] != 0;
        bool active = was_active;
        if (was_active && !skip) {
            if (mode == 1) {
                const float* p = pred + (size_t)i * k;
                if (k == 1) {
                    const double w = (hi + lo) / 2.0;
                    const float p0 = p[0];
                    if (p0 < thr) lo = w;      // a NaN prediction is not below the threshold: hi moves, as in Python
                    else hi = w;
                    pred_out[i] = p0;
                } else {
                    int first = k;             // the first probe the network accepts (NaN never does)
                    for (int j = 0; j < k; ++j) {
                        if (p[j] >= thr) { first = j; break; }
                    }
                    const double nlo = first == 0 ? lo : search_probe(lo, hi, first - 1, k);
                    const double nhi = first == k ? hi : search_probe(lo, hi, first, k);
                    pred_out[i] = p[first < k - 1 ? first : k - 1];
                    lo = nlo;
                    hi = nhi;
                }
                lo_[i] = lo;
                hi_[i] = hi;
                iters[i] += 1;
                active = search_active(lo, hi, below, above);
            }
            write = active;
        }
        if (active) atomicAdd(n_active, 1);   // integer count: order-independent
        s_lo = lo;
        s_hi = hi;
        s_write = write ? 1 : 0;
    }
    __syncthreads();
    if (!s_write) return;
    const double lo = s_lo, hi = s_hi;
    for (int j = 0; j < k; ++j) {
        const float c = (float)search_probe(lo, hi, j, k);   // round to nearest, as Session.prepare's float32 feed
        const int g = i * k + j;
        const int end = seg[g + 1];
        for (int e = seg[g] + (int)threadIdx.x; e < end; e += (int)blockDim.x) WC[2 * (size_t)e + 1] = c;
    }
}

}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_cost_search_step(double* lo, double* hi, int* iters, float* pred_out, int* n_active,
                                       const float* pred, float* WC, const int32_t* seg, const int* guard, int n_inst,
                                       int k, double threshold, double stopping_delta, int mode, void* stream) {
    TSPGNN_REQUIRE(n_inst >= 0, "cost_search_step: n_inst=%d", n_inst);
    if (n_inst == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(k >= 1, "cost_search_step: k=%d must be at least 1", k);
    TSPGNN_REQUIRE((long long)n_inst * k < (1LL << 31) - 1, "cost_search_step: n_inst*k=%lld graphs exceed int32",
                   (long long)n_inst * k);
    TSPGNN_REQUIRE(mode == 0 || mode == 1, "cost_search_step: mode=%d must be 0 (init) or 1 (step)", mode);
    TSPGNN_REQUIRE(lo && hi && iters && pred_out && n_active && WC && seg && guard,
                   "cost_search_step: null pointer");
    TSPGNN_REQUIRE(mode == 0 || pred, "cost_search_step: null pointer (pred, mode 1)");
    hipStream_t st = as_stream(stream);
    // zeroed on the launch's own stream: a captured round recounts from zero on every replay
    hipError_t e = hipMemsetAsync(n_active, 0, sizeof(int), st);
    if (e != hipSuccess)
        return fail(static_cast<int>(e), "cost_search_step: hipMemsetAsync failed: %s", hipGetErrorString(e));
    // the threshold is compared in fp32: NumPy compares a float32 prediction with a Python float in float32
    const float thr = (float)threshold;
    const double below = 1.0 - stopping_delta, above = 1.0 + stopping_delta;
    cost_search_kernel<<<(unsigned)n_inst, 256, 0, st>>>(lo, hi, iters, pred_out, n_active, pred, WC, seg, guard, k,
                                                         thr, below, above, mode);
    return launched("tspgnn_cost_search_step");
}
