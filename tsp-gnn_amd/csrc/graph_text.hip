// ".graph" text on the device: the bytes instance_loader.write_graph(np.triu(A), Mw, path, route=tour) writes.
//   tspgnn_host_f64_repr / tspgnn_f64_repr   Python's repr(float) of an array of doubles, on the host / on the device;
//   tspgnn_graph_text_sizes                  per instance the exact length of its file;
//   tspgnn_graph_text_write                  the files, each into its own byte range of one buffer.
//
// 1. repr(float).  A finite double is v = c 2^q (c < 2^53, q >= -1074); the doubles that round to it fill the interval
// [v - 2^(q-1), v + 2^(q-1)] -- from v - 2^(q-2) when c = 2^52 and v is not the smallest normal, where the spacing below v
// is half the spacing above -- with its ends inside exactly when c is even (round-half-even reads them back as v).  repr
// prints the decimal d 10^E with the fewest digits inside the interval, the nearest to v among those, a tie to the even d.
// With k = floor(log10 2^q) (floor(log10 (3/4) 2^q) for the short side) the interval is at least 10^k and less than 10^(k+1)
// wide: it holds a multiple of 10^k and at most one multiple of 10^(k+1).  Every decimal with fewer digits than the
// multiples of 10^k in it is a multiple of 10^(k+1), so the answer is that one multiple when it exists (its trailing
// zeros come off afterwards) and else the nearer of the two multiples of 10^k around v: s = floor(v 10^-k) or s + 1.
// All of it is decided on three integers, V(x) = x 2^q 10^-k for x = 4c - 2 | 4c - 1, 4c, 4c + 2: four times the lower end,
// v and the upper end in units of 10^k.  V is taken as the product with a 128-bit ceiling of 10^-k (graph_text_pow10.inc,
// tools/gen_pow10_table.py), floored, with bit 0 set when the next 64 bits of the fraction are not zero ("round to
// odd"): since every comparison is against a multiple of 4, the bit keeps "below", "at" and "above" apart.  The table's
// relative error is below 2^-127, the products below 2^60: an error below 2^-67 of a unit, which cannot carry V past
// an integer or hide a fraction because x 2^q 10^-k with x < 2^55 either is an integer or stays 2^-64 and more away from
// every integer (the known bound behind 128-bit tables for binary64 shortest printing; tests/test_graph_text_host.py
// compares 5 10^5 sampled values and every power of two and of ten with repr).  Integer arithmetic only: no floating-point operation
// touches the value, so host and device agree by construction.  Every loop has a fixed trip count (17 digits, 16 zeros).
//
// 2. The files.  One workgroup of 256 threads per instance (dataset_build.hip's conventions: the table on the host and
// on the device, n <= 256, workgroup-uniform early returns only).  A wave takes a row: the lengths of its edge lines and
// weight cells, summed over the wave, go to LDS; workgroup prefix sums over the rows and over the tour entries give
// every row and entry its first byte.  The write kernel measures in the same way, compares its total with bytes[i], and
// then walks the rows again: a wave scan of the lengths places each line and cell.  The weights are formatted in both
// passes and nothing but bytes[] travels between the launches: a conversion is ~10^2 integer operations against the
// 8-byte load it follows, and a table of cell lengths would be one more array of n^2 bytes per instance to size, check
// and keep alive between two calls.  Every store goes through Sink::put, which drops a byte outside [0, bytes[i]).
#include "tour_common.h"

#include <string.h>

namespace tspgnn {
namespace {

constexpr int kPow10Min = -292, kPow10Max = 324;
[[maybe_unused]] const uint64_t kPow10Host[kPow10Max - kPow10Min + 1][2] = {
#include "graph_text_pow10.inc"
};
[[maybe_unused]] __constant__ uint64_t kPow10Dev[kPow10Max - kPow10Min + 1][2] = {
#include "graph_text_pow10.inc"
};

constexpr int kReprMax = 24;   // "-2.2250738585072014e-308"

// A double in decimal: kind 0: d 10^e10 with nd digits in d, no trailing zero; 1: zero; 2: infinity; 3: NaN.
struct Dec {
    uint64_t d;
    int nd, e10, kind;
    bool neg;
};

// floor(y g / 2^128), g = g1 2^64 + g0, with bit 0 set when bits 64..127 of the product are not all zero.  y < 2^60.
__host__ __device__ __forceinline__ uint64_t scaled_odd(uint64_t g1, uint64_t g0, uint64_t y) {
    const unsigned __int128 lo = (unsigned __int128)g0 * y;
    const unsigned __int128 hi = (unsigned __int128)g1 * y + (uint64_t)(lo >> 64);
    return (uint64_t)(hi >> 64) | ((uint64_t)hi != 0 ? 1ull : 0ull);
}

__host__ __device__ __forceinline__ int count_digits(uint64_t d) {   // d < 10^17
    int nd = 1;
    uint64_t p = 10;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        nd += d >= p ? 1 : 0;
        p *= 10;
    }
    return nd;
}

__host__ __device__ inline Dec shortest(uint64_t bits) {
    Dec r;
    r.neg = (bits >> 63) != 0;
    r.d = 0;
    r.nd = 1;
    r.e10 = 0;
    const int be = (int)((bits >> 52) & 0x7ff);
    const uint64_t f = bits & ((1ull << 52) - 1);
    if (be == 0x7ff) {
        r.kind = f ? 3 : 2;
        return r;
    }
    if (be == 0 && f == 0) {
        r.kind = 1;
        return r;
    }
    r.kind = 0;
    const uint64_t c = be ? (f | (1ull << 52)) : f;
    const int q = be ? be - 1075 : -1074;
    const bool shortside = f == 0 && be > 1;
    // floor(log10 2^q), floor(log10 (3/4) 2^q), floor(log2 10^e) in fixed point; exact over the whole range
    // (tools/gen_pow10_table.py checks all three).  Negative products: an arithmetic shift, spelled as a floor division.
    const int num = q * 1262611 - (shortside ? 524031 : 0);
    const int k = num >= 0 ? num >> 22 : -((-num + (1 << 22) - 1) >> 22);
    const int l2n = -k * 1741647;
    const int l2 = l2n >= 0 ? l2n >> 19 : -((-l2n + (1 << 19) - 1) >> 19);
    const int h = q + l2 + 1;   // 1 .. 4
#ifdef __HIP_DEVICE_COMPILE__
    const uint64_t g1 = kPow10Dev[-k - kPow10Min][0], g0 = kPow10Dev[-k - kPow10Min][1];
#else
    const uint64_t g1 = kPow10Host[-k - kPow10Min][0], g0 = kPow10Host[-k - kPow10Min][1];
#endif
    const uint64_t cb = c << 2;
    const uint64_t vl = scaled_odd(g1, g0, (cb - (shortside ? 1 : 2)) << h);
    const uint64_t vb = scaled_odd(g1, g0, cb << h);
    const uint64_t vr = scaled_odd(g1, g0, (cb + 2) << h);
    const uint64_t open = c & 1;   // an odd c: the ends are outside
    const uint64_t s = vb >> 2;
    const uint64_t s10 = (s / 10) * 10, t10 = s10 + 10;
    const bool lo10 = vl + open <= (s10 << 2), hi10 = (t10 << 2) + open <= vr;
    uint64_t d;
    int e10;
    if (lo10 != hi10) {   // the one multiple of 10^(k+1) inside
        d = lo10 ? s10 : t10;
        e10 = k;
    } else {
        const bool lo1 = vl + open <= (s << 2), hi1 = ((s + 1) << 2) + open <= vr;
        const uint64_t mid = (2 * s + 1) << 1;   // four times s + 1/2
        const bool up = lo1 != hi1 ? hi1 : vb > mid || (vb == mid && (s & 1));
        d = up ? s + 1 : s;
        e10 = k;
    }
#pragma unroll 1
    for (int i = 0; i < 17; ++i) {   // trailing zeros; d < 10^18 has at most 17 of them
        const uint64_t t = d / 10;
        if (d != 0 && t * 10 == d) {
            d = t;
            ++e10;
        }
    }
    r.d = d;
    r.e10 = e10;
    r.nd = count_digits(d);
    return r;
}

// repr's layout: positional when the decimal point sits -3 .. 16 places after the first digit's left edge
__host__ __device__ __forceinline__ int repr_len(const Dec& r) {
    if (r.kind == 3) return 3;
    if (r.kind) return 3 + (r.neg ? 1 : 0);
    const int sign = r.neg ? 1 : 0, pt = r.nd + r.e10;
    if (pt > -4 && pt <= 16) return sign + (pt <= 0 ? 2 - pt + r.nd : pt < r.nd ? r.nd + 1 : pt + 2);
    const int x = pt - 1 < 0 ? 1 - pt : pt - 1;
    return sign + r.nd + (r.nd > 1 ? 1 : 0) + 2 + (x >= 100 ? 3 : 2);
}

// put(position, character) for every byte of the text; returns repr_len(r)
template <class Put>
__host__ __device__ inline int repr_put(const Dec& r, Put put) {
    int p = 0;
    if (r.neg && r.kind != 3) put(p++, '-');
    if (r.kind == 1) {
        put(p, '0'), put(p + 1, '.'), put(p + 2, '0');
        return p + 3;
    }
    if (r.kind == 2) {
        put(p, 'i'), put(p + 1, 'n'), put(p + 2, 'f');
        return p + 3;
    }
    if (r.kind == 3) {
        put(p, 'n'), put(p + 1, 'a'), put(p + 2, 'n');
        return p + 3;
    }
    const int nd = r.nd, pt = nd + r.e10;
    const bool positional = pt > -4 && pt <= 16;
    // digit i (from the left) sits at p + shift + i, one further right once a point stands before it
    int shift = 0, point = -1;   // point: digits before the '.', or -1 when no '.' splits the digits
    if (positional) {
        if (pt <= 0) {
            put(p, '0'), put(p + 1, '.');
#pragma unroll 1
            for (int z = 0; z < 3; ++z)
                if (z < -pt) put(p + 2 + z, '0');
            shift = 2 - pt;
        } else if (pt < nd) {
            point = pt;
        }
    } else if (nd > 1) {
        point = 1;
    }
    uint64_t d = r.d;
#pragma unroll 1
    for (int i = 16; i >= 0; --i) {
        if (i < nd) {
            const uint64_t t = d / 10;
            put(p + shift + i + (point >= 0 && i >= point ? 1 : 0), (char)('0' + (int)(d - t * 10)));
            d = t;
        }
    }
    if (point >= 0) put(p + point, '.');
    p += shift + nd + (point >= 0 ? 1 : 0);
    if (positional) {
        if (pt >= nd) {
#pragma unroll 1
            for (int z = 0; z < 16; ++z)
                if (z < pt - nd) put(p + z, '0');
            p += pt - nd;
            put(p, '.'), put(p + 1, '0');
            p += 2;
        }
        return p;
    }
    int x = pt - 1;
    put(p++, 'e');
    put(p++, x < 0 ? '-' : '+');
    x = x < 0 ? -x : x;
    if (x >= 100) put(p++, (char)('0' + x / 100));
    put(p++, (char)('0' + x / 10 % 10));
    put(p++, (char)('0' + x % 10));
    return p;
}

struct RawPut {
    char* out;
    __host__ __device__ __forceinline__ void operator()(int p, char ch) const { out[p] = ch; }
};

__global__ __launch_bounds__(256) void f64_repr_kernel(const unsigned long long* __restrict__ x, long long count,
                                                       char* __restrict__ text, unsigned char* __restrict__ len) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    len[i] = (unsigned char)repr_put(shortest(x[i]), RawPut{text + kReprMax * i});
}

// ------------------------------------------------------------------------------------------------------- the files
constexpr int kGtMinN = 4;
constexpr int kGtMaxN = 256;
constexpr int kGtThreads = 256;
constexpr int kGtWaves = kGtThreads / kWave;
static_assert(kGtThreads >= kGtMaxN, "every row and every tour entry has a thread");
constexpr int kSizeCols = 3;    // n, first matrix cell, first tour entry
constexpr int kWriteCols = 4;   // ... and the file's first byte

__constant__ const char kHead1[] = "TYPE : TSP\nDIMENSION: ";
__constant__ const char kHead2[] =
    "\nEDGE_DATA_FORMAT: EDGE_LIST\nEDGE_WEIGHT_TYPE: EXPLICIT\nEDGE_WEIGHT_FORMAT: FULL_MATRIX \nEDGE_DATA_SECTION:\n";
__constant__ const char kMid[] = "-1\nEDGE_WEIGHT_SECTION:\n";
__constant__ const char kTourHead[] = "TOUR_SECTION:\n";
__constant__ const char kTail[] = "EOF\n";
constexpr int kHead1Len = sizeof(kHead1) - 1, kHead2Len = sizeof(kHead2) - 1, kMidLen = sizeof(kMid) - 1,
              kTourHeadLen = sizeof(kTourHead) - 1, kTailLen = sizeof(kTail) - 1;

__device__ __forceinline__ int id_len(int x) { return 1 + (x >= 10 ? 1 : 0) + (x >= 100 ? 1 : 0); }   // 0 <= x < 1000

// The bytes of one file: the only door to the text buffer.
struct Sink {
    char* base;
    int size;
    __device__ __forceinline__ void put(int p, char ch) const {
        if ((unsigned)p < (unsigned)size) base[p] = ch;
    }
    __device__ __forceinline__ void text(int p, const char* s, int len, int tid) const {
        for (int k = tid; k < len; k += kGtThreads) put(p + k, s[k]);
    }
    __device__ __forceinline__ int id(int p, int x) const {   // 0 <= x < 1000; returns the position after it
        const int len = id_len(x);
        if (len > 2) put(p, (char)('0' + x / 100));
        if (len > 1) put(p + len - 2, (char)('0' + x / 10 % 10));
        put(p + len - 1, (char)('0' + x % 10));
        return p + len;
    }
};
struct SinkPut {
    Sink s;
    int at;
    __device__ __forceinline__ void operator()(int p, char ch) const { s.put(at + p, ch); }
};

// Exclusive prefix sum of one int per thread over the workgroup (all kGtThreads threads call); *total gets the sum.
__device__ __forceinline__ int group_scan(int v, int* s_w, int tid, int* total) {
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
    for (int k = 0; k < kGtWaves; ++k) {
        if (k < wv) base += s_w[k];
        tot += s_w[k];
    }
    __syncthreads();   // s_w is free again
    *total = tot;
    return base + x - v;
}

// Exclusive prefix sum over the wave; *total gets the wave's sum.
__device__ __forceinline__ int wave_scan(int v, int lane, int* total) {
    int x = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    *total = __shfl(x, kWave - 1);
    return x - v;
}

// The lengths of cell (i, j): its edge line "{i} {j}\n" (0 when the pair is not set) and its weight with the blank.
__device__ __forceinline__ void cell_lengths(const uint8_t* a, const unsigned long long* mw, int n, int i, int j, int* edge,
                                             int* weight) {
    const bool set = j > i && j < n && a[i * n + j] != 0;
    *edge = set ? id_len(i) + id_len(j) + 2 : 0;
    *weight = j >= n ? 0 : set ? repr_len(shortest(mw[i * n + j])) + 1 : 2;
}

// First bytes of the sections of a file, relative to its start, and its length.
struct Layout {
    int edges, mid, weights, tour_head, tour, tail, total;
    bool bad_tour;
};

// All threads of the workgroup call.  s_edge[i] / s_row[i] get the first byte of row i's edge lines / weight line inside
// their sections; *tour_at gets the first byte of this thread's tour entry inside the tour line (tid < n).
__device__ Layout measure(int n, const uint8_t* a, const unsigned long long* mw, const int32_t* t, int* s_edge, int* s_row,
                          int* s_w, int* tour_at) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    for (int i = wv; i < n; i += kGtWaves) {
        int e = 0, w = 0;
        for (int j = lane; j < n; j += kWave) {
            int ce, cw;
            cell_lengths(a, mw, n, i, j, &ce, &cw);
            e += ce;
            w += cw;
        }
        e = wave_sum(e);
        w = wave_sum(w);
        if (lane == 0) {
            s_edge[i] = e;
            s_row[i] = w + 1;   // the line end
        }
    }
    __syncthreads();
    int bad = 0, tlen = 0;
    if (tid < n) {
        const int x = t[tid];
        bad = (unsigned)x >= (unsigned)n;
        tlen = (bad ? 1 : id_len(x)) + 1;   // a blank, or the line end after the last entry
    }
    int tot_e, tot_w, tot_t;
    const int at_e = group_scan(tid < n ? s_edge[tid] : 0, s_w, tid, &tot_e);
    const int at_w = group_scan(tid < n ? s_row[tid] : 0, s_w, tid, &tot_w);
    *tour_at = group_scan(tlen, s_w, tid, &tot_t);
    if (tid < n) {
        s_edge[tid] = at_e;
        s_row[tid] = at_w;
    }
    Layout L;
    L.bad_tour = __syncthreads_or(bad) != 0;   // also: the offsets in LDS are visible
    L.edges = kHead1Len + id_len(n) + kHead2Len;
    L.mid = L.edges + tot_e;
    L.weights = L.mid + kMidLen;
    L.tour_head = L.weights + tot_w;
    L.tour = L.tour_head + kTourHeadLen;
    L.tail = L.tour + tot_t;
    L.total = L.tail + kTailLen;
    return L;
}

__global__ __launch_bounds__(kGtThreads) void graph_text_sizes_kernel(const long long* __restrict__ tab,
                                                                      const uint8_t* __restrict__ A,
                                                                      const unsigned long long* __restrict__ Mw,
                                                                      const int32_t* __restrict__ tours, int n_max,
                                                                      long long* __restrict__ bytes) {
    __shared__ int s_edge[kGtMaxN], s_row[kGtMaxN], s_w[kGtWaves];
    const long long* row = tab + (long long)kSizeCols * blockIdx.x;
    const int n = (int)row[0];
    if (n < kGtMinN || n > n_max) return;   // workgroup-uniform; the host check never sends these
    int tour_at;
    const Layout L = measure(n, A + row[1], Mw + row[1], tours + row[2], s_edge, s_row, s_w, &tour_at);
    if (threadIdx.x == 0) bytes[blockIdx.x] = L.total;
}

__global__ __launch_bounds__(kGtThreads) void graph_text_write_kernel(
    const long long* __restrict__ tab, const uint8_t* __restrict__ A, const unsigned long long* __restrict__ Mw,
    const int32_t* __restrict__ tours, int n_max, const long long* __restrict__ bytes, char* __restrict__ text,
    long long n_text, int32_t* __restrict__ status) {
    __shared__ int s_edge[kGtMaxN], s_row[kGtMaxN], s_w[kGtWaves];
    const long long* row = tab + (long long)kWriteCols * blockIdx.x;
    const int n = (int)row[0];
    if (n < kGtMinN || n > n_max) return;   // workgroup-uniform; the host check never sends these
    const uint8_t* a = A + row[1];
    const unsigned long long* mw = Mw + row[1];
    const int32_t* t = tours + row[2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    int tour_at;
    const Layout L = measure(n, a, mw, t, s_edge, s_row, s_w, &tour_at);
    const long long want = bytes[blockIdx.x];
    const bool fits = row[3] >= 0 && row[3] <= n_text - want;   // the host checked its own copy of bytes; this is ours
    const int verdict = L.bad_tour ? 2 : (long long)L.total != want || !fits ? 1 : 0;   // workgroup-uniform
    if (tid == 0) status[blockIdx.x] = verdict;
    if (verdict) return;
    const Sink out{text + row[3], L.total};

    out.text(0, kHead1, kHead1Len, tid);
    if (tid == 0) out.id(kHead1Len, n);
    out.text(kHead1Len + id_len(n), kHead2, kHead2Len, tid);
    out.text(L.mid, kMid, kMidLen, tid);
    out.text(L.tour_head, kTourHead, kTourHeadLen, tid);
    out.text(L.tail, kTail, kTailLen, tid);
    if (tid < n) out.put(out.id(L.tour + tour_at, t[tid]), tid == n - 1 ? '\n' : ' ');

    for (int i = wv; i < n; i += kGtWaves) {
        int at_e = L.edges + s_edge[i], at_w = L.weights + s_row[i];
        for (int j0 = 0; j0 < n; j0 += kWave) {
            const int j = j0 + lane;
            int ce, cw, sum_e, sum_w;
            cell_lengths(a, mw, n, i, j, &ce, &cw);
            const int pe = at_e + wave_scan(ce, lane, &sum_e), pw = at_w + wave_scan(cw, lane, &sum_w);
            if (ce) {
                out.put(out.id(pe, i), ' ');
                out.put(out.id(pe + id_len(i) + 1, j), '\n');
            }
            if (j < n) {
                if (ce)
                    repr_put(shortest(mw[i * n + j]), SinkPut{out, pw});
                else
                    out.put(pw, '0');
                out.put(pw + cw - 1, ' ');
                if (j == n - 1) out.put(pw + cw, '\n');
            }
            at_e += sum_e;
            at_w += sum_w;
        }
    }
}

// rows [lo, lo + len) must lie in [0, size): the host half of every offset check
bool inside(long long lo, long long len, long long size) { return lo >= 0 && len >= 0 && lo <= size - len; }

// The longest file at n: every pair set, every weight 24 characters, three-digit ids.  Keeps the int positions honest.
constexpr long long kLongestFile =
    200 + (long long)kGtMaxN * kGtMaxN / 2 * 8 + (long long)kGtMaxN * (kGtMaxN * (kReprMax + 1) + 1) + 4 * kGtMaxN;
static_assert(kLongestFile < (1ll << 31), "file positions are int");

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_host_f64_repr(const double* x, long long count, char* text, unsigned char* len) {
    TSPGNN_REQUIRE(count >= 0, "host_f64_repr: count=%lld", count);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(x && text && len, "host_f64_repr: null pointer");
    for (long long i = 0; i < count; ++i) {
        uint64_t bits;
        memcpy(&bits, x + i, sizeof bits);
        len[i] = (unsigned char)repr_put(shortest(bits), RawPut{text + kReprMax * i});
    }
    return TSPGNN_OK;
}

extern "C" int tspgnn_f64_repr(const double* x, long long count, char* text, unsigned char* len, void* stream) {
    TSPGNN_REQUIRE(count >= 0, "f64_repr: count=%lld", count);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(x && text && len, "f64_repr: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(x) % 8 == 0, "f64_repr: misaligned array");
    const long long blocks = (count + 255) / 256;
    TSPGNN_REQUIRE(blocks < (1ll << 31), "f64_repr: count=%lld is more than one launch holds", count);
    f64_repr_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(reinterpret_cast<const unsigned long long*>(x), count,
                                                                    text, len);
    return launched("tspgnn_f64_repr");
}

#define GT_COMMON(name, count, n_max)                                                                                \
    TSPGNN_REQUIRE((count) >= 0, name ": count=%d", (count));                                                      \
    TSPGNN_REQUIRE((n_max) >= kGtMinN && (n_max) <= kGtMaxN, name ": n_max=%d not in [%d, %d]", (n_max), kGtMinN, kGtMaxN); \
    if ((count) == 0) return TSPGNN_OK

extern "C" int tspgnn_graph_text_sizes(const long long* tab, const long long* d_tab, const unsigned char* A,
                                       const double* Mw, const int32_t* tours, int count, int n_max, long long n_cells,
                                       long long n_tour, long long* bytes, void* stream) {
    GT_COMMON("graph_text_sizes", count, n_max);
    TSPGNN_REQUIRE(tab && d_tab && A && Mw && tours && bytes, "graph_text_sizes: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(Mw) % 8 == 0 && reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(bytes) % 8 == 0 && reinterpret_cast<uintptr_t>(tours) % 4 == 0,
                   "graph_text_sizes: misaligned array");
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kSizeCols * b;
        TSPGNN_REQUIRE(r[0] >= kGtMinN && r[0] <= n_max, "graph_text_sizes: instance %d: n=%lld not in [%d, %d]", b, r[0],
                       kGtMinN, n_max);
        TSPGNN_REQUIRE(inside(r[1], r[0] * r[0], n_cells) && inside(r[2], r[0], n_tour),
                       "graph_text_sizes: instance %d: offsets (%lld, %lld) leave the arrays", b, r[1], r[2]);
    }
    graph_text_sizes_kernel<<<(unsigned)count, kGtThreads, 0, as_stream(stream)>>>(
        d_tab, A, reinterpret_cast<const unsigned long long*>(Mw), tours, n_max, bytes);
    return launched("tspgnn_graph_text_sizes");
}

extern "C" int tspgnn_graph_text_write(const long long* tab, const long long* d_tab, const unsigned char* A,
                                       const double* Mw, const int32_t* tours, int count, int n_max, long long n_cells,
                                       long long n_tour, const long long* bytes, const long long* host_bytes, char* text,
                                       long long n_text, int32_t* status, void* stream) {
    GT_COMMON("graph_text_write", count, n_max);
    TSPGNN_REQUIRE(tab && d_tab && A && Mw && tours && bytes && host_bytes && text && status,
                   "graph_text_write: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(Mw) % 8 == 0 && reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(bytes) % 8 == 0 && reinterpret_cast<uintptr_t>(tours) % 4 == 0 &&
                       reinterpret_cast<uintptr_t>(status) % 4 == 0,
                   "graph_text_write: misaligned array");
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kWriteCols * b;
        TSPGNN_REQUIRE(r[0] >= kGtMinN && r[0] <= n_max, "graph_text_write: instance %d: n=%lld not in [%d, %d]", b, r[0],
                       kGtMinN, n_max);
        TSPGNN_REQUIRE(inside(r[1], r[0] * r[0], n_cells) && inside(r[2], r[0], n_tour),
                       "graph_text_write: instance %d: offsets (%lld, %lld) leave the arrays", b, r[1], r[2]);
        TSPGNN_REQUIRE(host_bytes[b] >= 0 && host_bytes[b] < (1ll << 31) && inside(r[3], host_bytes[b], n_text),
                       "graph_text_write: instance %d: bytes [%lld, %lld + %lld) leave the text of %lld", b, r[3], r[3],
                       host_bytes[b], n_text);
    }
    graph_text_write_kernel<<<(unsigned)count, kGtThreads, 0, as_stream(stream)>>>(
        d_tab, A, reinterpret_cast<const unsigned long long*>(Mw), tours, n_max, bytes, text, n_text, status);
    return launched("tspgnn_graph_text_write");
}
