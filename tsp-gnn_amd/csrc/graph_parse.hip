// ".graph" text read on the device: the arrays instance_loader.read_graph gives for a file, without a host pass over it.
//   tspgnn_host_f64_parse / tspgnn_f64_parse   Python's float(token) of an array of tokens, on the host / on the device;
//   tspgnn_graph_text_scan                     per file its status, n, tour length and section offsets;
//   tspgnn_graph_text_parse                    per file the uint8 mask, the fp64 weights and the tour tspgnn_pack_dataset takes.
//
// 1. float(token).  The inverse of graph_text.hip's repr: a token is a sign, a mantissa w of at most 19 digits (w < 10^19
// < 2^64) and a decimal exponent e, its value v = w 10^e.  w = 0 is a signed zero; e < -342 gives v < 10^19 10^-343 <
// 2^-1075, half the smallest subnormal: zero; e > 308 gives v >= 10^309 > 2^1024: infinity.  Otherwise the table
// (graph_parse_pow10.inc, tools/gen_parse_table.py) holds t = floor(10^e / 2^p), p = floor(log2 10^e) - 127, so 10^e =
// (t + theta) 2^p with 0 <= theta < 1 and 2^127 <= t < 2^128.  With w' = w 2^z the mantissa shifted to 2^63 <= w' < 2^64,
// the 192-bit product P = w' t is exact, and v = X 2^(p - z + 64) with X = (P + w' theta) / 2^64.  H = floor(P / 2^64)
// has 127 or 128 bits and H <= X < H + 2: the fraction of P adds less than 1 and w' theta / 2^64 adds less than 1.
//   "Conclusive."  When H + 2 > 2^bits(H) the power of two above H may lie below X and the binary exponent is not
// known: not conclusive.  Otherwise floor(log2 v) = bits(H) - 1 + p - z + 64 is certain, and so is the number `kept` of
// mantissa bits the double holds there (53, fewer for a subnormal, none or less below 2^-1074).  kept < 0: v <
// 2^-1075, zero.  Else the double is H without its lowest drop = bits(H) - kept >= 74 bits, rounded: with r those bits of H
// and half = 2^(drop-1), the dropped part of X lies in [r, r + 2).  r + 2 <= half: it is below the midpoint, round down.
// r > half: it is above the midpoint, and if it passes 2^drop it passes it by less than 2 < half, which also rounds to
// q + 1: round up.  Only half - 2 < r <= half leaves the midpoint inside the interval: not conclusive.  A token that is not
// conclusive -- a share of 2^-72 of random ones, every exact tie -- is decided exactly: the truncation q of H is the
// double below v or that double's lower neighbour, and in both cases v rounds up from q exactly when v is above the
// midpoint (2q + 1) 2^(E-1) (when q is the lower neighbour v lies above q + 1, a fortiori), a tie going to the even q.
// The two sides of w 10^e <> (2q + 1) 2^(E-1) are brought to integers by moving the negative powers of five and two
// across, then compared word by word: at most 5^342 times a 56-bit integer, or w 5^308 2^308 -- under 1280 bits, 40
// words (the generator checks both).  mode 1 sends every token down that path.  Integer arithmetic only: no
// floating-point operation touches the value, so host and device agree by construction.  Every loop has a fixed trip
// count (48 bytes, 13 multiplications by 5^27, 40 words); nothing recurses or allocates.
//
// 2. The files.  One workgroup of 256 threads per file (graph_text.hip's conventions: the table on the host and on the
// device, workgroup-uniform early returns only).  The text is walked in tiles of 256 slabs of 16 bytes, slab borders on
// 16-byte addresses: a slab that lies inside the file is one 16-byte load, one that crosses an end is read byte by byte
// under the guard.  Sections are found as tspgnn_host_read_graph finds them, each key searched from where the last
// section began, the search ending with the first tile that holds a hit.  A per-byte flag marks line starts (pair lines)
// and token starts (weights, tour); a workgroup prefix sum of the slabs' counts plus a base carried from tile to tile
// numbers them, and the thread that owns a start handles the whole line or token, reading ahead across slab and tile
// borders through File::at, the only door to the text, which returns 0 outside [0, bytes[i]).  Pairs are set in a bitmap
// in LDS (atomicOr: a duplicated line counts once; both (i, j) and (j, i), the symmetric mask tspgnn_pack_dataset reads), from
// which the whole mask is written, zeros included.  Both kernels
// walk the sections; scan keeps only what the host needs to lay out the outputs.  Where the host reader lets strtol run
// on into the next line (a pair line with one integer, a blank line before the -1 line), this reader stays on the line:
// a line with one integer is status 5, a blank pair line is skipped.  A NUL byte is an ordinary character here.
#include "tour_common.h"


namespace tspgnn {
namespace {

typedef unsigned __int128 u128;

constexpr int kParseMin = -342, kParseMax = 308;
[[maybe_unused]] const uint64_t kParsePow10Host[kParseMax - kParseMin + 1][2] = {
#include "graph_parse_pow10.inc"
};
[[maybe_unused]] __constant__ uint64_t kParsePow10Dev[kParseMax - kParseMin + 1][2] = {
#include "graph_parse_pow10.inc"
};

constexpr int kTokenMax = 48;      // bytes of a token the device grammar reads
constexpr int kDigitsMax = 19;     // 10^19 < 2^64
constexpr int kWords = 40;         // 32-bit words of an exact comparison's operands
constexpr int kPow5Step = 27;      // 5^27 < 2^63
constexpr uint64_t kPow5_27 = 7450580596923828125ull;
constexpr uint64_t kInfBits = 0x7ff0000000000000ull, kNanBits = 0x7ff8000000000000ull;

enum { kTokOk = 0, kTokMalformed = 1, kTokOutside = 2 };

// ------------------------------------------------------------------------------------------ the exact comparison
struct Big {
    uint32_t w[kWords];
};

__host__ __device__ inline void big_set(Big& x, uint64_t v) {
    for (int i = 0; i < kWords; ++i) x.w[i] = 0;
    x.w[0] = (uint32_t)v;
    x.w[1] = (uint32_t)(v >> 32);
}

__host__ __device__ inline void big_mul(Big& x, uint64_t m) {   // what does not fit kWords words is dropped
    u128 carry = 0;
    for (int i = 0; i < kWords; ++i) {
        carry += (u128)x.w[i] * m;
        x.w[i] = (uint32_t)carry;
        carry >>= 32;
    }
}

__host__ __device__ inline void big_mul_pow5(Big& x, int a) {   // 0 <= a <= 13 * 27
    const int full = a / kPow5Step, rest = a % kPow5Step;
    uint64_t last = 1;
    for (int j = 0; j < kPow5Step - 1; ++j) last *= j < rest ? 5 : 1;
    for (int i = 0; i < 13; ++i) {
        if (i < full)
            big_mul(x, kPow5_27);
        else if (i == full && rest)
            big_mul(x, last);
    }
}

__host__ __device__ inline void big_shl(Big& x, int s) {   // s >= 0; bits shifted past the top are dropped
    const int ws = s >> 5, bs = s & 31;
    for (int i = kWords - 1; i >= 0; --i) {
        const int a = i - ws;
        const uint32_t hi = a >= 0 ? x.w[a] : 0u, lo = a >= 1 ? x.w[a - 1] : 0u;
        x.w[i] = bs ? (hi << bs) | (lo >> (32 - bs)) : hi;
    }
}

__host__ __device__ inline int big_cmp(const Big& a, const Big& b) {
    int c = 0;
    for (int i = 0; i < kWords; ++i) c = a.w[i] > b.w[i] ? 1 : a.w[i] < b.w[i] ? -1 : c;   // the highest difference wins
    return c;
}

// Does w 10^e round up from q 2^E2 -- is it above the midpoint (2q + 1) 2^(E2-1), or on it with q odd?
__host__ __device__ inline bool above_midpoint(uint64_t w, int e, uint64_t q, int E2) {
    Big V, S;
    big_set(V, w);
    big_set(S, 1);
    big_mul_pow5(e >= 0 ? V : S, e >= 0 ? e : -e);
    const int t = e - (E2 - 1);   // w 5^e 2^t <> 2q + 1
    big_shl(t >= 0 ? V : S, t >= 0 ? t : -t);
    big_mul(S, 2 * q + 1);
    const int c = big_cmp(V, S);
    return c > 0 || (c == 0 && (q & 1));
}

__host__ __device__ __forceinline__ int clz64(uint64_t x) {   // x != 0
#ifdef __HIP_DEVICE_COMPILE__
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// The double nearest to (neg ? -1 : 1) w 10^e, ties to even, as its bits.  mode != 0: every rounding by above_midpoint.
__host__ __device__ inline uint64_t decimal_bits(bool neg, uint64_t w, int e, int mode) {
    const uint64_t sign = neg ? 1ull << 63 : 0ull;
    if (w == 0 || e < kParseMin) return sign;
    if (e > kParseMax) return sign | kInfBits;
    const int z = clz64(w);
    const uint64_t wn = w << z;
#ifdef __HIP_DEVICE_COMPILE__
    const uint64_t t1 = kParsePow10Dev[e - kParseMin][0], t0 = kParsePow10Dev[e - kParseMin][1];
#else
    const uint64_t t1 = kParsePow10Host[e - kParseMin][0], t0 = kParsePow10Host[e - kParseMin][1];
#endif
    const u128 lo = (u128)wn * t0;
    const u128 H = (u128)wn * t1 + (uint64_t)(lo >> 64);   // < 2^128: wn t < 2^192
    // floor(log2 10^e) in fixed point, exact over the table (tools/gen_parse_table.py); an arithmetic shift, spelled as a
    // floor division
    const int l2n = e * 1741647;
    const int l2 = l2n >= 0 ? l2n >> 19 : -((-l2n + (1 << 19) - 1) >> 19);
    const int off = l2 - 127 - z + 64;   // v = X 2^off
    const int hb = (uint64_t)(H >> 127) ? 128 : 127;
    const int exp2 = hb - 1 + off;
    if (exp2 > 1023) return sign | kInfBits;   // H is a lower bound
    const int kept = exp2 >= -1022 ? 53 : exp2 + 1075;
    bool exact = mode != 0, up = false;
    if (!exact) {
        const u128 top = hb == 128 ? ~(u128)0 : (((u128)1 << 127) - 1);   // 2^hb - 1
        if (top - H < 2) {
            exact = true;
        } else if (kept < 0) {
            return sign;
        } else {
            const int drop = hb - kept;   // 74 .. 128
            const u128 r = drop == 128 ? H : H & (((u128)1 << drop) - 1), half = (u128)1 << (drop - 1);
            if (r <= half && r + 2 > half)
                exact = true;
            else
                up = r > half;
        }
    }
    const uint64_t q = kept <= 0 ? 0ull : (uint64_t)(H >> (hb - kept));
    if (exact) up = above_midpoint(w, e, q, kept <= 0 ? -1074 : off + hb - kept);
    const uint64_t m = q + (up ? 1 : 0);   // a carry out of the mantissa lands in the exponent field, up to infinity
    return sign | (exp2 >= -1022 ? ((uint64_t)(exp2 + 1022) << 52) + m : m);
}

// --------------------------------------------------------------------------------------------------- the grammar
__host__ __device__ __forceinline__ bool is_digit(int c) { return c >= '0' && c <= '9'; }
__host__ __device__ __forceinline__ int lower(int c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }

// get(i), 0 <= i < len, is byte i of the token.  -> kTok*, and *bits when kTokOk.
template <class Get>
__host__ __device__ inline int parse_token(Get get, int len, int mode, uint64_t* bits) {
    *bits = 0;
    if (len <= 0) return kTokMalformed;
    if (len > kTokenMax) return kTokOutside;
    int i = 0;
    bool neg = false;
    const int c0 = get(0);
    if (c0 == '+' || c0 == '-') {
        neg = c0 == '-';
        i = 1;
    }
    const int body = len - i;
    {   // inf, infinity, nan in any case; lower-case [+-]inf and unsigned nan are the device's
        const char* names[3] = {"inf", "infinity", "nan"};
        const int lens[3] = {3, 8, 3};
        for (int k = 0; k < 3; ++k) {
            if (body != lens[k]) continue;
            bool same = true, exact = true;
            for (int j = 0; j < lens[k]; ++j) {
                const int c = get(i + j);
                same = same && lower(c) == names[k][j];
                exact = exact && c == names[k][j];
            }
            if (!same) continue;
            if (!exact || k == 1 || (k == 2 && i)) return kTokOutside;
            *bits = k == 2 ? kNanBits : (neg ? 1ull << 63 : 0ull) | kInfBits;
            return kTokOk;
        }
    }
    if (body >= 3 && get(i) == '0' && lower(get(i + 1)) == 'x') {   // strtod reads hexadecimal, float() does not
        const int c = lower(get(i + 2));
        return is_digit(c) || (c >= 'a' && c <= 'f') ? kTokOutside : kTokMalformed;
    }
    // [digits][.digits][(e|E)[+-]digits], a digit on one side of the point at least; '_' between two digits is Python's
    uint64_t w = 0;
    int nd = 0, fd = 0, ex = 0, digits = 0, xdigits = 0;
    int state = 0;   // 0 integer part, 1 fraction, 2 exponent sign allowed, 3 exponent digits
    bool xneg = false, underscore = false, bad = false;
    int prev = 0;
    for (int p = 0; p < kTokenMax; ++p) {
        if (p < i || p >= len || bad) continue;
        const int c = get(p);
        if (is_digit(c)) {
            if (state <= 1) {
                ++digits;
                fd += state;
                if (nd || c != '0') {
                    if (nd < kDigitsMax) w = w * 10 + (uint64_t)(c - '0');
                    ++nd;
                }
            } else {
                state = 3;
                ++xdigits;
                ex = ex < 100000 ? ex * 10 + (c - '0') : ex;
            }
        } else if (c == '_') {
            const int nx = p + 1 < len ? get(p + 1) : 0;
            if (!is_digit(prev) || !is_digit(nx)) bad = true;
            underscore = true;
        } else if (c == '.' && state == 0) {
            state = 1;
        } else if ((c == 'e' || c == 'E') && state <= 1 && digits) {
            state = 2;
        } else if ((c == '+' || c == '-') && state == 2 && lower(prev) == 'e') {
            xneg = c == '-';
        } else {
            bad = true;
        }
        prev = c;
    }
    if (bad || !digits || (state >= 2 && !xdigits)) return kTokMalformed;
    if (underscore || nd > kDigitsMax) return kTokOutside;
    *bits = decimal_bits(neg, w, (xneg ? -ex : ex) - fd, mode);
    return kTokOk;
}

struct BufGet {
    const unsigned char* p;
    __host__ __device__ __forceinline__ int operator()(int i) const { return p[i]; }
};

__host__ __device__ inline void parse_one(const unsigned char* buf, long long n_buf, long long off, int len, int mode,
                                          unsigned long long* bits, unsigned char* status) {
    uint64_t b = 0;
    int s = kTokMalformed;   // a token that leaves the buffer
    if (off >= 0 && len >= 0 && off <= n_buf - len) s = parse_token(BufGet{buf + off}, len, mode, &b);
    *bits = b;
    *status = (unsigned char)s;
}

__global__ __launch_bounds__(256) void f64_parse_kernel(const unsigned char* __restrict__ buf, long long n_buf,
                                                        const long long* __restrict__ off, const int32_t* __restrict__ len,
                                                        long long count, int mode, unsigned long long* __restrict__ bits,
                                                        unsigned char* __restrict__ status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    parse_one(buf, n_buf, off[i], len[i], mode, bits + i, status + i);
}

// ------------------------------------------------------------------------------------------------------- the files
constexpr int kGpMinN = 4;
constexpr int kGpMaxN = 256;
constexpr int kGpThreads = 256;
constexpr int kGpWaves = kGpThreads / kWave;
constexpr int kSlab = 16;
constexpr int kScanCols = 2;    // the file's first byte, its length
constexpr int kParseCols = 5;   // ... n, first matrix cell, first tour entry
constexpr int kInfoCols = 8;    // status, n, tour length, edges, weights, tour (offsets), pair lines, 0
constexpr int kNSat = 1 << 20;  // integers saturate here, the host reader's limit on n
constexpr long long kFileMax = 1ll << 30;   // file positions are int
constexpr int kNone = INT_MAX;

enum {
    kStNoDimension = 3, kStNoSection = 4, kStPair = 5, kStWeights = 6, kStTour = 7, kStRange = 8, kStLower = 9,
    kStTourLength = 10, kStGrammar = 11
};

__device__ __forceinline__ bool is_space(int c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // \t \n \v \f \r
__device__ __forceinline__ bool is_blank(int c) { return c == ' ' || c == '\t'; }

// The bytes of one file: the only door to the text.
struct File {
    const unsigned char* f;
    int size;
    int skew;   // the file's first byte inside its 16-byte line
    __device__ __forceinline__ int at(int p) const { return (unsigned)p < (unsigned)size ? f[p] : 0; }
    __device__ __forceinline__ int first_slab(int p) const { return (p + skew) / kSlab; }
    __device__ __forceinline__ int slab_pos(int s) const { return s * kSlab - skew; }
    // the 16 bytes from slab_pos(s) on, 0 outside the file
    __device__ __forceinline__ void slab(int s, uint32_t w[4]) const {
        const int p = slab_pos(s);
        if (p >= 0 && p <= size - kSlab) {
            const uint4 v = *reinterpret_cast<const uint4*>(f + p);   // f + p is a multiple of 16
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        } else {
            w[0] = w[1] = w[2] = w[3] = 0;
            if (p + kSlab > 0 && p < size)
                for (int b = 0; b < kSlab; ++b) w[b >> 2] |= (uint32_t)at(p + b) << (8 * (b & 3));
        }
    }
};
__device__ __forceinline__ int slab_byte(const uint32_t w[4], int b) { return (w[b >> 2] >> (8 * (b & 3))) & 0xff; }

// Exclusive prefix sum of one int per thread over the workgroup (all kGpThreads threads call); *total gets the sum.
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
    for (int k = 0; k < kGpWaves; ++k) {
        if (k < wv) base += s_w[k];
        tot += s_w[k];
    }
    __syncthreads();   // s_w is free again
    *total = tot;
    return base + x - v;
}

// The smallest of one int per thread over the workgroup (all threads call).
__device__ __forceinline__ int group_min(int v, int* s_w, int tid) {
    const int lane = tid & (kWave - 1), wv = tid / kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
    int r = s_w[0];
    for (int k = 1; k < kGpWaves; ++k) r = min(r, s_w[k]);
    __syncthreads();
    return r;
}

// The bitwise or of one word per thread over the workgroup (all threads call).
__device__ __forceinline__ unsigned group_or(unsigned v, int* s_w, int tid) {
    const int lane = tid & (kWave - 1), wv = tid / kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v |= (unsigned)__shfl_xor((int)v, off);
    if (lane == 0) s_w[wv] = (int)v;
    __syncthreads();
    unsigned r = 0;
    for (int k = 0; k < kGpWaves; ++k) r |= (unsigned)s_w[k];
    __syncthreads();
    return r;
}

// The first position p >= from at which hit(p, byte at p) holds, or kNone.  All threads call; the result is uniform.
template <class Hit>
__device__ int first_at(const File& F, int from, int* s_w, Hit hit) {
    const int tid = threadIdx.x;
    if (from >= F.size) return kNone;   // uniform
    for (int s0 = F.first_slab(from); F.slab_pos(s0) < F.size; s0 += kGpThreads) {
        uint32_t w[4];
        F.slab(s0 + tid, w);
        const int p0 = F.slab_pos(s0 + tid);
        int mine = kNone;
#pragma unroll
        for (int b = kSlab - 1; b >= 0; --b) {
            const int p = p0 + b;
            if (p >= from && p < F.size && hit(p, slab_byte(w, b))) mine = p;
        }
        const int r = group_min(mine, s_w, tid);
        if (r != kNone) return r;
    }
    return kNone;
}

// The first `key` at or after `from`, or kNone.
__device__ int find_key(const File& F, int from, const char* key, int klen, int* s_w) {
    return first_at(F, from, s_w, [&](int p, int c) {
        if (c != key[0]) return false;
        for (int i = 1; i < klen; ++i)
            if (F.at(p + i) != key[i]) return false;
        return true;
    });
}

// The first byte after the line that holds the first `key` at or after `from` (the file's end when that line is the
// last), or kNone without the key.
__device__ int after_line_with(const File& F, int from, const char* key, int klen, int* s_w) {
    const int k = find_key(F, from, key, klen, s_w);
    if (k == kNone) return kNone;
    const int nl = first_at(F, k, s_w, [](int, int c) { return c == '\n'; });
    return nl == kNone ? F.size : nl + 1;
}

// strtol's integer at p, confined to [p, end): blanks and tabs, a sign, digits.  -> the position after it, or -1 when no
// digit stands there; the value saturates beyond +-kNSat.
__device__ __forceinline__ int read_int(const File& F, int p, int end, int* value) {
    while (p < end && is_blank(F.at(p))) ++p;
    bool neg = false;
    if (p < end && (F.at(p) == '+' || F.at(p) == '-')) neg = F.at(p++) == '-';
    if (p >= end || !is_digit(F.at(p))) return -1;
    int v = 0;
    while (p < end && is_digit(F.at(p))) {
        v = min(v * 10 + (F.at(p) - '0'), kNSat + 1);
        ++p;
    }
    *value = neg ? -v : v;
    return p;
}

__constant__ const char kKeyDim[] = "DIMENSION";
__constant__ const char kKeyEdges[] = "EDGE_DATA_SECTION";
__constant__ const char kKeyWeights[] = "EDGE_WEIGHT_SECTION";
__constant__ const char kKeyTour[] = "TOUR_SECTION";

struct Sections {
    int n, edges, weights, tour;   // positions: the first byte of each section's first line
    unsigned bad;                  // bit s: status s applies
};

// All threads call; everything returned is workgroup-uniform.
__device__ Sections locate(const File& F, int* s_w, int* s_n) {
    Sections L;
    L.n = 0, L.edges = L.weights = L.tour = 0, L.bad = 0;
    const int dim = find_key(F, 0, kKeyDim, (int)sizeof(kKeyDim) - 1, s_w);
    if (dim == kNone) {
        L.bad = 1u << kStNoDimension;
        return L;
    }
    if (threadIdx.x == 0) {   // strtol after the key, past ':', blanks and tabs; strtol itself skips any white space
        int p = dim + (int)sizeof(kKeyDim) - 1;
        while (p < F.size && (F.at(p) == ':' || is_blank(F.at(p)))) ++p;
        while (p < F.size && is_space(F.at(p))) ++p;
        int v = 0;
        *s_n = read_int(F, p, F.size, &v) < 0 ? 0 : v;
    }
    __syncthreads();
    L.n = *s_n;
    __syncthreads();
    if (L.n <= 0 || L.n > kNSat) {
        L.bad = 1u << kStNoDimension;
        return L;
    }
    L.edges = after_line_with(F, dim, kKeyEdges, (int)sizeof(kKeyEdges) - 1, s_w);
    L.weights = L.edges == kNone ? kNone : after_line_with(F, L.edges, kKeyWeights, (int)sizeof(kKeyWeights) - 1, s_w);
    L.tour = L.weights == kNone ? kNone : after_line_with(F, L.weights, kKeyTour, (int)sizeof(kKeyTour) - 1, s_w);
    if (L.tour == kNone) L.bad = 1u << kStNoSection;
    if (L.n < kGpMinN || L.n > kGpMaxN) L.bad |= 1u << kStRange;
    return L;
}

// One pair line [p, its '\n' or the file's end).  -> 0 a blank line, 1 the line that ends the list (it holds "-1", or
// does not begin with an integer), 2 a pair (*i, *j; *j is kNone when the line holds one integer only).
__device__ int pair_line(const File& F, int p, int* i, int* j) {
    int end = p;
    bool minus_one = false, blank = true;
    while (end < F.size && F.at(end) != '\n') {
        minus_one = minus_one || (F.at(end) == '-' && F.at(end + 1) == '1');
        blank = blank && is_space(F.at(end));
        ++end;
    }
    if (minus_one) return 1;
    if (blank) return 0;
    const int q = read_int(F, p, end, i);
    if (q < 0) return 1;
    if (read_int(F, q, end, j) < 0) *j = kNone;
    return 2;
}

// The pair lines from L.edges on, up to the line that ends the list.  bitmap (LDS, n^2 bits, zeroed by the caller) gets
// the pairs when it is not NULL.  -> the number of pair lines; *set: the number of distinct pairs; bad: status bits.
__device__ int read_pairs(const File& F, const Sections& L, uint32_t* bitmap, int* s_w, int* set, unsigned* bad) {
    const int tid = threadIdx.x, n = L.n;
    int lines = 0, fresh = 0;
    if (L.edges < L.weights) {   // uniform
        for (int s0 = F.first_slab(L.edges); F.slab_pos(s0) < L.weights; s0 += kGpThreads) {
            uint32_t w[4];
            F.slab(s0 + tid, w);
            const int p0 = F.slab_pos(s0 + tid);
            int prev = F.at(p0 - 1);
            unsigned starts = 0;
            int stop = kNone;
#pragma unroll
            for (int b = 0; b < kSlab; ++b) {
                const int p = p0 + b;
                if (p >= L.edges && p < L.weights && (p == L.edges || prev == '\n')) starts |= 1u << b;
                prev = slab_byte(w, b);
            }
            for (unsigned rest = starts; rest; rest &= rest - 1) {
                int i, j;
                const int p = p0 + __ffs(rest) - 1;
                if (pair_line(F, p, &i, &j) == 1) stop = min(stop, p);
            }
            stop = group_min(stop, s_w, tid);
            for (unsigned rest = starts; rest; rest &= rest - 1) {
                int i = 0, j = 0;
                const int p = p0 + __ffs(rest) - 1;
                if (p >= stop || pair_line(F, p, &i, &j) != 2) continue;
                ++lines;
                if (j == kNone || (unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n) {
                    *bad |= 1u << kStPair;
                } else if (i >= j) {
                    *bad |= 1u << kStLower;
                } else if (bitmap) {
                    const int cell = i * n + j;
                    const uint32_t bit = 1u << (cell & 31);
                    fresh += (atomicOr(&bitmap[cell >> 5], bit) & bit) ? 0 : 1;
                    const int mirror = j * n + i;   // the mask is symmetric, as tspgnn_build_instances makes it
                    atomicOr(&bitmap[mirror >> 5], 1u << (mirror & 31));
                }
            }
            if (stop != kNone) break;   // uniform
        }
    }
    int total;
    group_scan(fresh, s_w, tid, set);
    group_scan(lines, s_w, tid, &total);
    return total;
}

// The tour: the integers on the line at L.tour, separated by blanks and tabs, up to the first token that is none
// (strtol's prefix of such a token still counts).  tours: NULL, or where the first n entries go.  -> its length.
__device__ int read_tour(const File& F, const Sections& L, int32_t* tours, int* s_w, unsigned* bad) {
    const int tid = threadIdx.x, n = L.n;
    const int eol = first_at(F, L.tour, s_w, [](int, int c) { return c == '\n' || c == '\r'; });
    const int end = eol == kNone ? F.size : eol;
    int base = 0, length = kNone;
    if (L.tour < end) {   // uniform
        for (int s0 = F.first_slab(L.tour); F.slab_pos(s0) < end; s0 += kGpThreads) {
            uint32_t w[4];
            F.slab(s0 + tid, w);
            const int p0 = F.slab_pos(s0 + tid);
            int prev = F.at(p0 - 1);
            unsigned starts = 0;
#pragma unroll
            for (int b = 0; b < kSlab; ++b) {
                const int p = p0 + b, c = slab_byte(w, b);
                if (p >= L.tour && p < end && !is_blank(c) && (p == L.tour || is_blank(prev))) starts |= 1u << b;
                prev = c;
            }
            int total;
            const int first = base + group_scan(__popc(starts), s_w, tid, &total);
            int stop = kNone, k = first;
            for (unsigned rest = starts; rest; rest &= rest - 1, ++k) {
                int v;
                const int q = read_int(F, p0 + __ffs(rest) - 1, end, &v);
                if (q < 0 || (q < end && !is_blank(F.at(q)))) stop = min(stop, k + (q < 0 ? 0 : 1));
            }
            stop = group_min(stop, s_w, tid);
            k = first;
            for (unsigned rest = starts; rest; rest &= rest - 1, ++k) {
                int v = 0;
                if (k >= stop || read_int(F, p0 + __ffs(rest) - 1, end, &v) < 0) continue;
                if ((unsigned)v >= (unsigned)n)
                    *bad |= 1u << kStTour;
                else if (tours && k < n)
                    tours[k] = v;
            }
            base += total;
            if (stop != kNone) {   // uniform
                length = stop;
                break;
            }
        }
    }
    return length == kNone ? base : length;
}

struct FileGet {
    File F;
    int at;
    __device__ __forceinline__ int operator()(int i) const { return F.at(at + i); }
};

// The first n^2 white-space separated tokens from L.weights on -> mw (NULL: counted only).
__device__ void read_weights(const File& F, const Sections& L, unsigned long long* mw, int* s_w, unsigned* bad) {
    const int tid = threadIdx.x, cells = L.n * L.n;
    int base = 0;
    if (L.weights < F.size) {   // uniform
        for (int s0 = F.first_slab(L.weights); F.slab_pos(s0) < F.size && base < cells; s0 += kGpThreads) {
            uint32_t w[4];
            F.slab(s0 + tid, w);
            const int p0 = F.slab_pos(s0 + tid);
            int prev = F.at(p0 - 1);
            unsigned starts = 0;
#pragma unroll
            for (int b = 0; b < kSlab; ++b) {
                const int p = p0 + b, c = slab_byte(w, b);
                if (p >= L.weights && p < F.size && !is_space(c) && (p == L.weights || is_space(prev))) starts |= 1u << b;
                prev = c;
            }
            int total;
            int k = base + group_scan(__popc(starts), s_w, tid, &total);
            for (unsigned rest = starts; rest && k < cells; rest &= rest - 1, ++k) {
                const int p = p0 + __ffs(rest) - 1;
                int len = 0;
                while (len <= kTokenMax && p + len < F.size && !is_space(F.at(p + len))) ++len;
                uint64_t bits;
                const int s = parse_token(FileGet{F, p}, len, 0, &bits);
                if (s) *bad |= 1u << (s == kTokOutside ? kStGrammar : kStWeights);
                if (mw) mw[k] = bits;
            }
            base += total;
        }
    }
    if (base < cells) *bad |= 1u << kStWeights;   // uniform
}

__device__ __forceinline__ int first_status(unsigned bad) { return bad ? __ffs(bad) - 1 : 0; }

__device__ __forceinline__ File open_file(const char* text, long long n_text, long long b0, long long bytes, bool* ok) {
    *ok = b0 >= 0 && bytes >= 0 && bytes <= kFileMax && b0 <= n_text - bytes;   // the host checked its own copy
    File F;
    F.f = reinterpret_cast<const unsigned char*>(text) + (*ok ? b0 : 0);
    F.size = *ok ? (int)bytes : 0;
    F.skew = (int)(reinterpret_cast<uintptr_t>(F.f) & (kSlab - 1));
    return F;
}

__global__ __launch_bounds__(kGpThreads) void graph_text_scan_kernel(const long long* __restrict__ tab,
                                                                     const char* __restrict__ text, long long n_text,
                                                                     int32_t* __restrict__ info) {
    __shared__ int s_w[kGpWaves], s_n;
    const long long* row = tab + (long long)kScanCols * blockIdx.x;
    int32_t* out = info + (long long)kInfoCols * blockIdx.x;
    const int tid = threadIdx.x;
    bool ok;
    const File F = open_file(text, n_text, row[0], row[1], &ok);
    Sections L = locate(F, s_w, &s_n);
    int lines = 0, tour_len = 0, set;
    unsigned bad = 0;
    if (!L.bad) {   // uniform
        lines = read_pairs(F, L, nullptr, s_w, &set, &bad);
        tour_len = read_tour(F, L, nullptr, s_w, &bad);
        if (tour_len != L.n) bad |= 1u << kStTourLength;
    }
    bad = group_or(bad | L.bad, s_w, tid);
    if (tid == 0) {
        out[0] = first_status(bad), out[1] = L.n, out[2] = tour_len, out[3] = L.edges == kNone ? -1 : L.edges;
        out[4] = L.weights == kNone ? -1 : L.weights, out[5] = L.tour == kNone ? -1 : L.tour, out[6] = lines, out[7] = 0;
    }
}

__global__ __launch_bounds__(kGpThreads) void graph_text_parse_kernel(
    const long long* __restrict__ tab, const char* __restrict__ text, long long n_text, int n_max, long long n_cells,
    long long n_tour, unsigned char* __restrict__ A, unsigned long long* __restrict__ Mw, int32_t* __restrict__ tours,
    int32_t* __restrict__ m, int32_t* __restrict__ status) {
    __shared__ int s_w[kGpWaves], s_n;
    __shared__ uint32_t s_bits[kGpMaxN * kGpMaxN / 32];
    const long long* row = tab + (long long)kParseCols * blockIdx.x;
    const int tid = threadIdx.x;
    const int n = (int)row[2];
    const long long c0 = row[3], t0 = row[4];
    // workgroup-uniform; the host check never sends these
    if (n < kGpMinN || n > n_max || n_max > kGpMaxN || c0 < 0 || c0 > n_cells - (long long)n * n || t0 < 0 || t0 > n_tour - n)
        return;
    bool ok;
    const File F = open_file(text, n_text, row[0], row[1], &ok);
    Sections L = locate(F, s_w, &s_n);
    if (!L.bad && L.n != n) L.bad = 1u << kStNoDimension;   // not the n the scan of this file gave
    unsigned bad = 0;
    int set = 0;
    if (!L.bad) {   // uniform
        for (int k = tid; k < (n * n + 31) / 32; k += kGpThreads) s_bits[k] = 0;
        __syncthreads();
        read_pairs(F, L, s_bits, s_w, &set, &bad);   // its scans are the barrier behind the atomics
        for (int k = tid; k < n * n; k += kGpThreads) A[c0 + k] = (unsigned char)((s_bits[k >> 5] >> (k & 31)) & 1u);
        if (read_tour(F, L, tours + t0, s_w, &bad) != n) bad |= 1u << kStTourLength;
        read_weights(F, L, Mw + c0, s_w, &bad);
    }
    bad = group_or(bad | L.bad, s_w, tid);
    if (tid == 0) {
        status[blockIdx.x] = first_status(bad);
        m[blockIdx.x] = set;
    }
}

// rows [lo, lo + len) must lie in [0, size): the host half of every offset check
bool inside(long long lo, long long len, long long size) { return lo >= 0 && len >= 0 && lo <= size - len; }

}  // namespace
}  // namespace tspgnn

using namespace tspgnn;

extern "C" int tspgnn_host_f64_parse(const unsigned char* buf, long long n_buf, const long long* off, const int32_t* len,
                                     long long count, int mode, unsigned long long* bits, unsigned char* status) {
    TSPGNN_REQUIRE(count >= 0 && n_buf >= 0, "host_f64_parse: count=%lld n_buf=%lld", count, n_buf);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(buf && off && len && bits && status, "host_f64_parse: null pointer");
    for (long long i = 0; i < count; ++i) parse_one(buf, n_buf, off[i], len[i], mode, bits + i, status + i);
    return TSPGNN_OK;
}

extern "C" int tspgnn_f64_parse(const unsigned char* buf, long long n_buf, const long long* off, const int32_t* len,
                                long long count, int mode, unsigned long long* bits, unsigned char* status, void* stream) {
    TSPGNN_REQUIRE(count >= 0 && n_buf >= 0, "f64_parse: count=%lld n_buf=%lld", count, n_buf);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(buf && off && len && bits && status, "f64_parse: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(off) % 8 == 0 && reinterpret_cast<uintptr_t>(bits) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(len) % 4 == 0,
                   "f64_parse: misaligned array");
    const long long blocks = (count + 255) / 256;
    TSPGNN_REQUIRE(blocks < (1ll << 31), "f64_parse: count=%lld is more than one launch holds", count);
    f64_parse_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(buf, n_buf, off, len, count, mode, bits, status);
    return launched("tspgnn_f64_parse");
}

extern "C" int tspgnn_graph_text_scan(const long long* tab, const long long* d_tab, const char* text, long long n_text,
                                      int count, int32_t* info, void* stream) {
    TSPGNN_REQUIRE(count >= 0, "graph_text_scan: count=%d", count);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(tab && d_tab && text && info, "graph_text_scan: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 && reinterpret_cast<uintptr_t>(info) % 4 == 0,
                   "graph_text_scan: misaligned array");
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kScanCols * b;
        TSPGNN_REQUIRE(r[1] <= kFileMax && inside(r[0], r[1], n_text),
                       "graph_text_scan: file %d: bytes [%lld, %lld + %lld) leave the text of %lld", b, r[0], r[0], r[1],
                       n_text);
    }
    graph_text_scan_kernel<<<(unsigned)count, kGpThreads, 0, as_stream(stream)>>>(d_tab, text, n_text, info);
    return launched("tspgnn_graph_text_scan");
}

extern "C" int tspgnn_graph_text_parse(const long long* tab, const long long* d_tab, const char* text, long long n_text,
                                       int count, int n_max, long long n_cells, long long n_tour, unsigned char* A,
                                       double* Mw, int32_t* tours, int32_t* m, int32_t* status, void* stream) {
    TSPGNN_REQUIRE(count >= 0, "graph_text_parse: count=%d", count);
    TSPGNN_REQUIRE(n_max >= kGpMinN && n_max <= kGpMaxN, "graph_text_parse: n_max=%d not in [%d, %d]", n_max, kGpMinN,
                   kGpMaxN);
    if (count == 0) return TSPGNN_OK;
    TSPGNN_REQUIRE(tab && d_tab && text && A && Mw && tours && m && status, "graph_text_parse: null pointer");
    TSPGNN_REQUIRE(reinterpret_cast<uintptr_t>(d_tab) % 8 == 0 && reinterpret_cast<uintptr_t>(Mw) % 8 == 0 &&
                       reinterpret_cast<uintptr_t>(tours) % 4 == 0 && reinterpret_cast<uintptr_t>(m) % 4 == 0 &&
                       reinterpret_cast<uintptr_t>(status) % 4 == 0,
                   "graph_text_parse: misaligned array");
    for (int b = 0; b < count; ++b) {
        const long long* r = tab + (long long)kParseCols * b;
        TSPGNN_REQUIRE(r[1] <= kFileMax && inside(r[0], r[1], n_text),
                       "graph_text_parse: file %d: bytes [%lld, %lld + %lld) leave the text of %lld", b, r[0], r[0], r[1],
                       n_text);
        TSPGNN_REQUIRE(r[2] >= kGpMinN && r[2] <= n_max, "graph_text_parse: file %d: n=%lld not in [%d, %d]", b, r[2],
                       kGpMinN, n_max);
        TSPGNN_REQUIRE(inside(r[3], r[2] * r[2], n_cells) && inside(r[4], r[2], n_tour),
                       "graph_text_parse: file %d: offsets (%lld, %lld) leave the arrays", b, r[3], r[4]);
    }
    graph_text_parse_kernel<<<(unsigned)count, kGpThreads, 0, as_stream(stream)>>>(
        d_tab, text, n_text, n_max, n_cells, n_tour, A, reinterpret_cast<unsigned long long*>(Mw), tours, m, status);
    return launched("tspgnn_graph_text_parse");
}
