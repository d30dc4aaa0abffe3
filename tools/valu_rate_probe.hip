// Development probe: issue cost (cycles per wave64 instruction per SIMD) of the VALU / MFMA instructions the
// fused cell kernel is made of, on gfx950.  One workgroup per CU, W waves per SIMD, each wave runs `rounds` x 64
// instances of ONE instruction over 8 independent register chains; cycles = wall time x clock / instructions.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/valu_rate_probe.hip -o /tmp/valu_probe
// `valu_probe` prints the single-instruction table; `valu_probe mixed` the MFMA-beside-VALU co-issue table (below).
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define REP8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define BODY(NAME, ASM)                                                                        \
    __device__ __forceinline__ void NAME(float (&v)[8], float (&w)[8], float a, float b) {     \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                        \
            _Pragma("unroll") for (int i = 0; i < 8; ++i) { ASM; }                             \
        }                                                                                      \
    }

BODY(b_fma, asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(a), "v"(b)))
BODY(b_max, asm volatile("v_max_f32 %0, %0, %1" : "+v"(v[i]) : "v"(b)))
BODY(b_exp, asm volatile("v_exp_f32 %0, %0" : "+v"(v[i])))
BODY(b_rcp, asm volatile("v_rcp_f32 %0, %0" : "+v"(v[i])))
BODY(b_rsq, asm volatile("v_rsq_f32 %0, %0" : "+v"(v[i])))
BODY(b_shl, asm volatile("v_lshlrev_b32 %0, 16, %0" : "+v"(v[i])))
BODY(b_cvtbf, asm volatile("v_cvt_pk_bf16_f32 %0, %0, %1" : "+v"(v[i]) : "v"(w[i])))
BODY(b_cvtf16, asm volatile("v_cvt_pk_f16_f32 %0, %0, %1" : "+v"(v[i]) : "v"(w[i])))
BODY(b_cvtrtz, asm volatile("v_cvt_pkrtz_f16_f32 %0, %0, %1" : "+v"(v[i]) : "v"(w[i])))
BODY(b_cvtf32, asm volatile("v_cvt_f32_f16 %0, %0" : "+v"(v[i])))
BODY(b_mix, asm volatile("v_fma_mix_f32 %0, %0, %1, %2 op_sel_hi:[0,0,1]" : "+v"(v[i]) : "v"(a), "v"(w[i])))
BODY(b_mixlo, asm volatile("v_fma_mixlo_f16 %0, %1, %2, %0 op_sel_hi:[0,0,0]" : "+v"(v[i]) : "v"(w[i]), "v"(a)))
BODY(b_dpp, asm volatile("v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf" : "+v"(v[i])))
BODY(b_perm, asm volatile("ds_bpermute_b32 %0, %1, %0\n s_waitcnt lgkmcnt(0)" : "+v"(v[i]) : "v"(w[i])))

__device__ __forceinline__ void b_pkfma(float (&v)[8], float (&w)[8], float a, float b) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 x[4], aa = {a, a}, bb = {b, b};
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = f32x2{v[2 * i], v[2 * i + 1]};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(x[i]) : "v"(aa), "v"(bb));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = x[i][0]; v[2 * i + 1] = x[i][1]; }
}

template <int KIND>
__global__ __launch_bounds__(1024) void probe(float* __restrict__ out, int rounds) {
    const int tid = threadIdx.x, lane = tid & 63;
    float v[8], w[8];
    for (int i = 0; i < 8; ++i) { v[i] = 1.0f + 0.001f * (lane + i); w[i] = 0.5f + 0.002f * (lane - i); }
    const float a = 0.9999f, b = 0.0001f;
    f32x4 acc[8];
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    f16x8 ha, hb;
    bf16x8 ba, bb;
    for (int i = 0; i < 8; ++i) {
        ha[i] = (_Float16)(0.01f * (lane + i)); hb[i] = (_Float16)(0.02f * (lane - i));
        ba[i] = (__bf16)(0.01f * (lane + i)); bb[i] = (__bf16)(0.02f * (lane - i));
    }
    for (int r = 0; r < rounds; ++r) {
        if constexpr (KIND == 0) b_fma(v, w, a, b);
        if constexpr (KIND == 1) b_pkfma(v, w, a, b);
        if constexpr (KIND == 2) b_exp(v, w, a, b);
        if constexpr (KIND == 3) b_rcp(v, w, a, b);
        if constexpr (KIND == 4) b_rsq(v, w, a, b);
        if constexpr (KIND == 5) b_max(v, w, a, b);
        if constexpr (KIND == 6) b_shl(v, w, a, b);
        if constexpr (KIND == 7) b_cvtbf(v, w, a, b);
        if constexpr (KIND == 8) b_cvtf16(v, w, a, b);
        if constexpr (KIND == 9) b_cvtrtz(v, w, a, b);
        if constexpr (KIND == 10) b_cvtf32(v, w, a, b);
        if constexpr (KIND == 11) b_mix(v, w, a, b);
        if constexpr (KIND == 12) b_mixlo(v, w, a, b);
        if constexpr (KIND == 13) b_dpp(v, w, a, b);
        if constexpr (KIND == 14) b_perm(v, w, a, b);
        if constexpr (KIND == 15) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[t], 0, 0, 0);
        }
        if constexpr (KIND == 16) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ba, bb, acc[t], 0, 0, 0);
        }
        if constexpr (KIND >= 20 && KIND <= 23) {  // dependent chains: 1, 2, 4 accumulators in rotation; 23: 3-chains per acc
            constexpr int NA = KIND == 20 ? 1 : (KIND == 21 ? 2 : 4);
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const int t = KIND == 23 ? (k / 3) % 8 : k % NA;
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[t], 0, 0, 0);
            }
        }
        if constexpr (KIND == 17) {  // 8 MFMA + 8 v_exp interleaved
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[t], 0, 0, 0);
                    asm volatile("v_exp_f32 %0, %0" : "+v"(v[t]));
                }
            }
        }
        if constexpr (KIND == 18) {  // 8 MFMA + 8 v_fma interleaved
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[t], 0, 0, 0);
                    asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(v[t]) : "v"(a), "v"(b));
                }
            }
        }
        if constexpr (KIND == 19) {  // 1 MFMA : 4 v_fma
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, acc[t], 0, 0, 0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(v[(t + j) & 7]) : "v"(a), "v"(b));
                }
            }
        }
    }
    float res = 0.f;
    for (int t = 0; t < 8; ++t) res += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
    for (int i = 0; i < 8; ++i) res += v[i];
    out[blockIdx.x * blockDim.x + tid] = res;
}

template <int KIND>
static void run(const char* name, float* out, int per_round) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int rounds = 4000;
    printf("%-34s", name);
    for (int wps = 1; wps <= 4; wps *= 2) {  // waves per SIMD
        probe<KIND><<<256, wps * 256>>>(out, rounds);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        probe<KIND><<<256, wps * 256>>>(out, rounds);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        // cycles per instruction per SIMD at a nominal 2.4 GHz
        const double cyc = ms * 1e-3 * 2.4e9 / ((double)rounds * per_round * wps);
        printf("  %dw/SIMD: %6.2f cyc (%.3f ms)", wps, cyc, ms);
    }
    printf("\n");
}

// ------------------------------------------------------------------------------------------------------- mixed mode
// `valu_probe mixed`: does the gate phase's f32 arithmetic issue beside ANOTHER wavefront's MFMAs?  One workgroup of 12
// wavefronts per CU (100 KB of LDS keeps a second one away), three per SIMD -- the cell launch's occupancy; wavefront w runs
// on SIMD w % 4, so w / 4 is its slot on the SIMD.  Slots below n_mfma run the K GEMM's shape: 16 accumulators, three
// dependent v_mfma_f32_16x16x32_f16 each, `rm` rounds.  The other slots run `rv` rounds of the gate mix of one edge tile, 192
// pair operations in the tile's proportions (96 fma : 60 mul : 36 add, plus 24 v_max_f32 for the relus) over four
// independent pair chains, either PACKED (v_pk_fma/mul/add_f32) or SINGLE (the same element operations as v_fma / v_mul /
// v_add_f32), with or without the tile's transcendentals (48 v_exp, 48 v_rcp, 12 v_rsq per 192).  Every loop is bounded.
// A role that is switched off leaves at once, so each role is also timed alone; hidden = (alone_m + alone_v - together) /
// min(alone_m, alone_v) from the launches' wall times.  Per-wavefront s_memtime ticks are reported beside them.
typedef float f32x2m __attribute__((ext_vector_type(2)));

template <bool PACKED, bool TRANS>
__device__ __forceinline__ void gate_mix(float (&x)[8], float (&u)[8], const float (&w)[8], float a, float b) {
    f32x2m p[4], aa = {a, a}, bb = {b, b};
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = f32x2m{x[2 * i], x[2 * i + 1]};
#pragma unroll
    for (int unit = 0; unit < 12; ++unit) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {   // 8 fma, 5 mul, 3 add per unit, round-robin over the four pair chains
            const int i = k & 3;
            if constexpr (PACKED) {
                if (k < 8) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(p[i]) : "v"(aa), "v"(bb));
                else if (k < 13) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(p[i]) : "v"(aa));
                else asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(p[i]) : "v"(bb));
            } else {
                float &lo = x[2 * i], &hi = x[2 * i + 1];
                if (k < 8) {
                    asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(lo) : "v"(a), "v"(b));
                    asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(hi) : "v"(a), "v"(b));
                } else if (k < 13) {
                    asm volatile("v_mul_f32 %0, %0, %1" : "+v"(lo) : "v"(a));
                    asm volatile("v_mul_f32 %0, %0, %1" : "+v"(hi) : "v"(a));
                } else {
                    asm volatile("v_add_f32 %0, %0, %1" : "+v"(lo) : "v"(b));
                    asm volatile("v_add_f32 %0, %0, %1" : "+v"(hi) : "v"(b));
                }
            }
        }
        asm volatile("v_max_f32 %0, %1, %1" : "=v"(u[0]) : "v"(w[0]));
        asm volatile("v_max_f32 %0, %1, %1" : "=v"(u[1]) : "v"(w[1]));
        if constexpr (TRANS) {   // results are not chained: the operands stay finite whatever the round count
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("v_exp_f32 %0, %1" : "=v"(u[k]) : "v"(w[k]));
#pragma unroll
            for (int k = 0; k < 4; ++k) asm volatile("v_rcp_f32 %0, %1" : "=v"(u[4 + k]) : "v"(w[4 + k]));
            asm volatile("v_rsq_f32 %0, %1" : "=v"(u[unit & 7]) : "v"(w[unit & 7]));
        }
    }
    if constexpr (PACKED) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { x[2 * i] = p[i][0]; x[2 * i + 1] = p[i][1]; }
    }
}

template <bool PACKED, bool TRANS>
__global__ __launch_bounds__(768) void mixed(float* __restrict__ out, long long* __restrict__ ticks, int n_mfma, int mfma_on,
                                             int valu_on, int rm, int rv) {
    extern __shared__ float pad[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slot = wave >> 2;
    const bool is_mfma = slot < n_mfma;
    long long dt = 0;
    float res = 0.f;
    if (is_mfma && mfma_on) {
        f32x4 acc[16];
        for (int t = 0; t < 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        f16x8 ha, hb;
        for (int i = 0; i < 8; ++i) { ha[i] = (_Float16)(0.01f * (lane + i)); hb[i] = (_Float16)(0.001f * (lane - i)); }
        const long long t0 = clock64();
        for (int r = 0; r < rm; ++r) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                f32x4 c = acc[t];
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(hb, ha, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ha, hb, c, 0, 0, 0);
                acc[t] = c;
            }
        }
        for (int t = 0; t < 16; ++t) res += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
        dt = clock64() - t0;
    } else if (!is_mfma && valu_on) {
        float x[8], u[8], w[8];
        for (int i = 0; i < 8; ++i) { x[i] = 1.0f + 0.001f * (lane + i); w[i] = 0.5f + 0.002f * (lane + i); u[i] = 0.f; }
        const float a = 0.99999f, b = 0.00001f;
        const long long t0 = clock64();
        for (int r = 0; r < rv; ++r) gate_mix<PACKED, TRANS>(x, u, w, a, b);
        for (int i = 0; i < 8; ++i) res += x[i] + u[i];
        dt = clock64() - t0;
    }
    if (res == 123.456f) pad[tid] = res;   // (keeps the LDS allocation and the results alive)
    out[blockIdx.x * 768 + tid] = res;
    if (lane == 0) ticks[blockIdx.x * 12 + wave] = dt;
}

template <bool PACKED, bool TRANS>
static void run_mixed(const char* name, float* out, long long* ticks, int n_mfma, int rm, int rv) {
    const int grid = 256, lds = 100 * 1024;
    hipFuncSetAttribute(reinterpret_cast<const void*>(&mixed<PACKED, TRANS>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    static long long host[256 * 12];
    double ms[3], tk_m[3], tk_v[3];
    for (int mode = 0; mode < 3; ++mode) {   // 0: MFMA wavefronts alone, 1: VALU wavefronts alone, 2: together
        const int m_on = mode != 1, v_on = mode != 0;
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {   // first launch warms up; best of the other three
            hipEventRecord(e0);
            mixed<PACKED, TRANS><<<grid, 768, lds>>>(out, ticks, n_mfma, m_on, v_on, rm, rv);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float t;
            hipEventElapsedTime(&t, e0, e1);
            if (rep > 0 && t < best) best = t;
        }
        ms[mode] = best;
        hipMemcpy(host, ticks, sizeof(host), hipMemcpyDeviceToHost);
        double sm = 0, sv = 0;
        int nm = 0, nv = 0;
        for (int i = 0; i < grid * 12; ++i) {
            if ((i % 12) / 4 < n_mfma) { sm += host[i]; ++nm; } else { sv += host[i]; ++nv; }
        }
        tk_m[mode] = nm ? sm / nm : 0;
        tk_v[mode] = nv ? sv / nv : 0;
    }
    const double lo = ms[0] < ms[1] ? ms[0] : ms[1];
    printf("%-18s %d MFMA + %d VALU wavefronts/SIMD | alone: mfma %7.1f us (%9.0f ticks/wave)  valu %7.1f us (%9.0f) | together %7.1f us "
           "(mfma %9.0f, valu %9.0f ticks/wave) | serial sum %7.1f us  hidden %5.1f %%\n",
           name, n_mfma, 3 - n_mfma, ms[0] * 1e3, tk_m[0], ms[1] * 1e3, tk_v[1], ms[2] * 1e3, tk_m[2], tk_v[2],
           (ms[0] + ms[1]) * 1e3, 100.0 * (ms[0] + ms[1] - ms[2]) / lo);
}

static int main_mixed() {
    float* out;
    long long* ticks;
    hipMalloc(&out, 256 * 768 * sizeof(float));
    hipMalloc(&ticks, 256 * 12 * sizeof(long long));
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    printf("# %s, %d CUs; 256 workgroups x 12 wavefronts; per VALU round: 192 pair ops (96 fma, 60 mul, 36 add) + 24 v_max"
           " [+ 48 v_exp, 48 v_rcp, 12 v_rsq]; per MFMA round: 48 v_mfma_f32_16x16x32_f16 (16 accumulators x 3 dependent)\n",
           prop.name, prop.multiProcessorCount);
    for (int n_mfma = 1; n_mfma <= 2; ++n_mfma) {
        // rounds sized so that both roles alone take a few hundred microseconds
        const int rv = n_mfma == 1 ? 150 : 300, rm = n_mfma == 1 ? 600 : 300;
        run_mixed<true, false>("packed", out, ticks, n_mfma, rm, rv);
        run_mixed<false, false>("single", out, ticks, n_mfma, rm, rv);
        run_mixed<true, true>("packed + trans", out, ticks, n_mfma, rm, rv);
        run_mixed<false, true>("single + trans", out, ticks, n_mfma, rm, rv);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && argv[1][0] == 'm') return main_mixed();
    float* out;
    hipMalloc(&out, 1024 * 1024 * 4);
    run<0>("v_fma_f32", out, 64);
    run<1>("v_pk_fma_f32", out, 64);
    run<2>("v_exp_f32", out, 64);
    run<3>("v_rcp_f32", out, 64);
    run<4>("v_rsq_f32", out, 64);
    run<5>("v_max_f32", out, 64);
    run<6>("v_lshlrev_b32", out, 64);
    run<7>("v_cvt_pk_bf16_f32", out, 64);
    run<8>("v_cvt_pk_f16_f32", out, 64);
    run<9>("v_cvt_pkrtz_f16_f32", out, 64);
    run<10>("v_cvt_f32_f16", out, 64);
    run<11>("v_fma_mix_f32", out, 64);
    run<12>("v_fma_mixlo_f16", out, 64);
    run<13>("v_add_f32_dpp row_ror", out, 64);
    run<14>("ds_bpermute_b32 + wait", out, 64);
    run<15>("v_mfma_f32_16x16x32_f16", out, 64);
    run<16>("v_mfma_f32_16x16x32_bf16", out, 64);
    run<17>("mfma_f16 + v_exp (per pair)", out, 64);
    run<18>("mfma_f16 + v_fma (per pair)", out, 64);
    run<19>("mfma_f16 + 4 v_fma (per group)", out, 64);
    run<20>("mfma_f16 dependent chain (1 acc)", out, 64);
    run<21>("mfma_f16 2 accs alternating", out, 64);
    run<22>("mfma_f16 4 accs alternating", out, 64);
    run<23>("mfma_f16 3-chains, 8 accs", out, 64);
    return 0;
}
