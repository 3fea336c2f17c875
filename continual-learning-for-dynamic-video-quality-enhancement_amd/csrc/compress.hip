// Compressed client updates on the client matrix: top-k sparsification with error feedback and QSGD
// stochastic quantisation, in place, per row.
//
//   nvq_fed_compress   a = (x - base) + e; keep the k largest |a| of the row (ties kept), quantise the kept ones to `levels`
//                      uniform steps of max |a| with Philox rounding; x' = base + c or base, e' = a - (x' - base)
//
// The k-th largest magnitude of a row is exact: a radix select on the 31 magnitude bits (digits of 11, 10 and 10 bits), one
// streaming pass per digit.  A workgroup counts its share of the row in an LDS histogram and adds the bins that are not empty to
// the row's histogram in the workspace with integer atomics; every workgroup of the next pass finds the digit of the k-th key in
// that histogram again by itself, so there is no host step and no launch between the passes.  Integers only: the counts, and so
// every value, are the same on every call.  All K rows go in each launch (grid.y = K); a thread owns whole quads in the 16-byte
// and in the scalar form alike, and the n % 4 tail belongs to threads 0 .. 2 of block 0 (flat.h).
#include "fed.h"

namespace nvq {

constexpr int kCompressQuads = 2048;                   // quads of a row per workgroup before the grid stops growing: 8 trips
constexpr int kCompressMaxBlocks = 512;                // workgroups per row at most
constexpr int kBins0 = 2048, kBins1 = 1024, kBins2 = 1024;
constexpr int kRowWords = kBins0 + kBins1 + kBins2 + 4;   // a row's workspace: three histograms, then the largest key

inline int compress_blocks(long n) {
    int nb = ceil_div(n >> 2, (long)kCompressQuads);
    if (nb > kCompressMaxBlocks) nb = kCompressMaxBlocks;
    return nb < 1 ? 1 : nb;
}

// where the accumulated update of a pass comes from
constexpr int SRC_DELTA = 0;                           // x - b: no residual
constexpr int SRC_ACCUMULATE = 1;                      // (x - b) + e, and the pass stores it into the residual row
constexpr int SRC_STORED = 2;                          // the residual row holds it already

// what a counting pass counts
constexpr int PASS_DIGIT0 = 0, PASS_DIGIT1 = 1, PASS_DIGIT2 = 2, PASS_MAX = 3;

// the 31 magnitude bits; every NaN is the largest key, after inf
__device__ __forceinline__ unsigned magnitude_key(float a) {
    const unsigned m = __float_as_uint(a) & 0x7fffffffu;
    return m > 0x7f800000u ? 0x7fffffffu : m;
}

__device__ __forceinline__ float accumulate(float x, float b, float e) {
    return (float)(((double)x - (double)b) + (double)e);
}

template <bool VEC, bool HAS_BASE, int SRC>
__device__ __forceinline__ float4 update_quad(const float* x, const float* base, float* res, long q) {
    if (SRC == SRC_STORED) return ldq<VEC>(res + 4 * q);
    const float4 xv = ldq<VEC>(x + 4 * q);
    const float4 b = HAS_BASE ? ldq<VEC>(base + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 e = SRC == SRC_ACCUMULATE ? ldq<VEC>(res + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(accumulate(xv.x, b.x, e.x), accumulate(xv.y, b.y, e.y), accumulate(xv.z, b.z, e.z),
                       accumulate(xv.w, b.w, e.w));
}

template <bool HAS_BASE, int SRC>
__device__ __forceinline__ float update_tail(const float* x, const float* base, float* res, long t) {
    if (SRC == SRC_STORED) return res[t];
    return accumulate(x[t], HAS_BASE ? base[t] : 0.f, SRC == SRC_ACCUMULATE ? res[t] : 0.f);
}

// The digit of the kth largest key (kth >= 1) from a histogram of nbins = 256 * per bins: `digit` has fewer than kth keys above
// it and at least kth with it; `rem` = kth less the keys above it, `at` = the keys in it.  256 threads; thread t owns the per
// bins below nbins - t * per, so an inclusive scan over t counts from the top.  sh: 8 words of LDS.  Ends with a barrier after
// which sh may be used again.
__device__ __forceinline__ void select_digit(const unsigned* __restrict__ hist, int nbins, unsigned kth, unsigned* sh,
                                             unsigned& digit, unsigned& rem, unsigned& at) {
    const int per = nbins >> 8, t = threadIdx.x, top = nbins - 1 - t * per;
    unsigned c[8], s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        c[j] = j < per ? hist[top - j] : 0u;
        s += c[j];
    }
    unsigned incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if ((t & 63) >= o) incl += up;
    }
    if (t < 3) sh[4 + t] = 0u;
    if ((t & 63) == 63) sh[t >> 6] = incl;
    __syncthreads();
    for (int w = 0; w < (t >> 6); ++w) incl += sh[w];
    unsigned above = incl - s;
    if (above < kth && kth <= incl) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < per && above < kth) {
                if (above + c[j] >= kth) {
                    sh[4] = (unsigned)(top - j);
                    sh[5] = kth - above;
                    sh[6] = c[j];
                    above = kth;                       // found: the lower bins are not looked at
                } else {
                    above += c[j];
                }
            }
        }
    }
    __syncthreads();
    digit = sh[4];
    rem = sh[5];
    at = sh[6];
    __syncthreads();
}

// One counting pass over row blockIdx.y.  PASS_DIGIT0: the histogram of the leading 11 bits and the row's largest key;
// PASS_DIGIT1 / 2: the next 10 bits among the keys that share the digits found so far; PASS_MAX: the largest key only (no top-k).
// With SRC_ACCUMULATE the pass leaves the accumulated update in the residual row for the passes that follow.
template <bool VEC, bool HAS_BASE, int SRC>
__global__ __launch_bounds__(256) void compress_count_kernel(const float* clients, long stride, const float* base, long n,
                                                             long kth, float* residual, long residual_stride,
                                                             const int* __restrict__ slots, int pass, unsigned* workspace) {
    __shared__ unsigned bins[kBins0];
    __shared__ unsigned sh[8];
    const int r = blockIdx.y;
    const float* x = clients + r * stride;
    float* res = SRC == SRC_DELTA ? nullptr : residual + (slots != nullptr ? slots[r] : r) * residual_stride;
    unsigned* hist = workspace + (long)r * kRowWords;
    unsigned prefix = 0, shift = 20, mask = kBins0 - 1, match = 31;   // key >> 31 == 0: every key matches
    unsigned* out = hist;
    if (pass == PASS_DIGIT1 || pass == PASS_DIGIT2) {
        unsigned d0, d1, rem, at;
        select_digit(hist, kBins0, (unsigned)kth, sh, d0, rem, at);
        prefix = d0, match = 20, shift = 10, mask = kBins1 - 1, out = hist + kBins0;
        if (pass == PASS_DIGIT2) {
            select_digit(hist + kBins0, kBins1, rem, sh, d1, rem, at);
            prefix = d0 << 10 | d1, match = 10, shift = 0, out = hist + kBins0 + kBins1;
        }
    }
    const bool count = pass != PASS_MAX;
    if (count)
        for (int b = threadIdx.x; b < kBins0; b += 256) bins[b] = 0u;
    __syncthreads();
    unsigned largest = 0;
    const auto take = [&](float a) {
        const unsigned key = magnitude_key(a);
        largest = max(largest, key);
        if (count && (key >> match) == prefix) atomicAdd(&bins[(key >> shift) & mask], 1u);
    };
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 a = update_quad<VEC, HAS_BASE, SRC>(x, base, res, q);
        if (SRC == SRC_ACCUMULATE) stq<VEC>(res + 4 * q, a);
        take(a.x);
        take(a.y);
        take(a.z);
        take(a.w);
    }
    const long t = 4 * nq + threadIdx.x;
    if (flat_tail(n, t)) {
        const float a = update_tail<HAS_BASE, SRC>(x, base, res, t);
        if (SRC == SRC_ACCUMULATE) res[t] = a;
        take(a);
    }
    __syncthreads();
    if (count)
        for (int b = threadIdx.x; b <= (int)mask; b += 256)
            if (bins[b] != 0u) atomicAdd(&out[b], bins[b]);
    if (pass == PASS_DIGIT0 || pass == PASS_MAX) {
        for (int o = 32; o > 0; o >>= 1) largest = max(largest, (unsigned)__shfl_xor((int)largest, o, 64));
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = largest;
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(&hist[kBins0 + kBins1 + kBins2], max(max(sh[0], sh[1]), max(sh[2], sh[3])));
    }
}

// xi = floor(|a| s / scale + u), c = sgn(a) xi scale / s: every operation a single IEEE rounding in double, or exact
__device__ __forceinline__ float quantise(float a, unsigned w, double scale, double s) {
    const double t = __ddiv_rn(__dmul_rn((double)fabsf(a), s), scale);
    const double u = ((double)(w >> 8) + 0.5) * 0x1p-24;
    const double xi = floor(__dadd_rn(t, u));
    const double c = __ddiv_rn(__dmul_rn(xi, scale), s);
    return (float)(a < 0.f ? -c : c);
}

// one coordinate: a and b in, x' returned, e' in `e`
__device__ __forceinline__ float compress_one(float a, float b, unsigned threshold, bool quant, unsigned w, double scale, double s,
                                              float& e) {
    float xn = b;
    if (magnitude_key(a) >= threshold) {
        const float c = quant ? quantise(a, w, scale, s) : a;
        xn = (float)((double)b + (double)c);
    }
    e = (float)((double)a - ((double)xn - (double)b));
    if ((__float_as_uint(e) & 0x7f800000u) == 0x7f800000u) e = 0.f;    // inf or NaN: one bad update does not stay for ever
    return xn;
}

// The last sweep of row blockIdx.y: the threshold from the three histograms (kth > 0), the scale from the largest key
// (levels > 0), then x' into the matrix and, with a residual, e' into its row.  Block 0 writes kept[r].
template <bool VEC, bool HAS_BASE, int SRC>
__global__ __launch_bounds__(256) void compress_sweep_kernel(float* clients, long stride, const float* base, long n, long kth,
                                                             int levels, float* residual, long residual_stride,
                                                             const int* __restrict__ slots, long seed, long offset,
                                                             int* __restrict__ kept, const unsigned* __restrict__ workspace) {
    __shared__ unsigned sh[8];
    const int r = blockIdx.y;
    float* x = clients + r * stride;
    float* res = SRC == SRC_DELTA ? nullptr : residual + (slots != nullptr ? slots[r] : r) * residual_stride;
    unsigned threshold = 0;
    long keep = n;
    if (kth > 0) {
        const unsigned* hist = workspace + (long)r * kRowWords;
        unsigned d0, d1, d2, rem, at;
        select_digit(hist, kBins0, (unsigned)kth, sh, d0, rem, at);
        select_digit(hist + kBins0, kBins1, rem, sh, d1, rem, at);
        select_digit(hist + kBins0 + kBins1, kBins2, rem, sh, d2, rem, at);
        threshold = d0 << 20 | d1 << 10 | d2;
        keep = kth - rem + at;                         // the keys above the threshold and every key equal to it
    }
    if (kept != nullptr && blockIdx.x == 0 && threadIdx.x == 0) kept[r] = (int)keep;
    bool quant = false;
    double scale = 0.0;
    if (levels > 0) {
        const unsigned top = workspace[(long)r * kRowWords + kBins0 + kBins1 + kBins2];
        quant = top != 0u && top < 0x7f800000u;        // a row of zeros, or one with inf or NaN, is not quantised
        scale = (double)__uint_as_float(top);
    }
    const double s = (double)levels;
    const long off = offset + r;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 a = update_quad<VEC, HAS_BASE, SRC>(x, base, res, q);
        const float4 b = HAS_BASE ? ldq<VEC>(base + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (quant && max(max(magnitude_key(a.x), magnitude_key(a.y)), max(magnitude_key(a.z), magnitude_key(a.w))) >= threshold)
            philox4x32_10((unsigned)q, (unsigned)((unsigned long)q >> 32), (unsigned)off, (unsigned)((unsigned long)off >> 32),
                          (unsigned)seed, (unsigned)((unsigned long)seed >> 32), w);
        float4 v, e;
        v.x = compress_one(a.x, b.x, threshold, quant, w[0], scale, s, e.x);
        v.y = compress_one(a.y, b.y, threshold, quant, w[1], scale, s, e.y);
        v.z = compress_one(a.z, b.z, threshold, quant, w[2], scale, s, e.z);
        v.w = compress_one(a.w, b.w, threshold, quant, w[3], scale, s, e.w);
        stq<VEC>(x + 4 * q, v);
        if (SRC != SRC_DELTA) stq<VEC>(res + 4 * q, e);
    }
    const long t = 4 * nq + threadIdx.x;
    if (flat_tail(n, t)) {
        const float a = update_tail<HAS_BASE, SRC>(x, base, res, t);
        const float b = HAS_BASE ? base[t] : 0.f;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (quant)
            philox4x32_10((unsigned)nq, (unsigned)((unsigned long)nq >> 32), (unsigned)off, (unsigned)((unsigned long)off >> 32),
                          (unsigned)seed, (unsigned)((unsigned long)seed >> 32), w);
        float e;
        x[t] = compress_one(a, b, threshold, quant, threadIdx.x == 0 ? w[0] : (threadIdx.x == 1 ? w[1] : w[2]), scale, s, e);
        if (SRC != SRC_DELTA) res[t] = e;
    }
}

__global__ __launch_bounds__(64) void compress_fill_kept_kernel(int* __restrict__ kept, int K, int n) {
    if ((int)threadIdx.x < K) kept[threadIdx.x] = n;
}

}  // namespace nvq

using namespace nvq;

extern "C" {

size_t nvq_fed_compress_workspace_bytes(int K, long n) {
    if (K < 1 || n < 0) return 0;
    return (size_t)K * kRowWords * sizeof(unsigned);
}

int nvq_fed_compress(float* clients, long stride, int K, const float* base, long n, long k, int levels, float* residual,
                     long residual_stride, const int* slots, long seed, long offset, int* kept, void* workspace,
                     size_t workspace_bytes, void* stream) {
    int rc = fed_check("fed_compress", clients, stride, K, n, seed, offset);
    if (rc) return rc;
    NVQ_REQUIRE(k >= 0, "fed_compress: k = %ld (0: no top-k)", k);
    NVQ_REQUIRE(levels >= 0 && levels <= 32767, "fed_compress: levels = %d outside 0 .. 32767", levels);
    NVQ_REQUIRE(n <= 0x7fffffffL, "fed_compress: n = %ld does not fit the 32-bit counters", n);
    NVQ_REQUIRE(residual == nullptr || residual_stride >= n, "fed_compress: residual_stride %ld < n %ld", residual_stride, n);
    NVQ_REQUIRE(residual != nullptr || slots == nullptr, "fed_compress: slots without a residual");
    NVQ_REQUIRE(aligned4(slots) && aligned4(kept) && aligned4(workspace), "fed_compress: slots / kept / workspace alignment");
    hipStream_t s = (hipStream_t)stream;
    if (k >= n) k = 0;                                 // everything is kept
    const bool select = k > 0, quant = levels > 0;
    if (n == 0 || (!select && !quant && residual == nullptr)) {        // nothing to change
        if (kept != nullptr) {
            hipLaunchKernelGGL(compress_fill_kept_kernel, dim3(1), dim3(64), 0, s, kept, K, (int)n);
            return check_launch("fed_compress");
        }
        return NVQ_OK;
    }
    unsigned* ws = (unsigned*)workspace;
    if (select || quant) {
        const size_t need = nvq_fed_compress_workspace_bytes(K, n);
        if (workspace == nullptr || workspace_bytes < need) {
            set_error("fed_compress: the workspace has %zu bytes, %zu are needed", workspace_bytes, need);
            return NVQ_EWORKSPACE;
        }
        if (hipMemsetAsync(ws, 0, need, s) != hipSuccess) return check_launch("fed_compress");
    }
    const bool vec = fed_vec(clients, stride, base, residual) && (residual_stride & 3) == 0;
    const dim3 grid(compress_blocks(n), K), block(256);
    const bool has_res = residual != nullptr;
    const auto count = [&](int src, int pass) {
        return with_consts("fed_compress", [&](auto SRC, auto V, auto B) {
            hipLaunchKernelGGL((compress_count_kernel<V(), B(), SRC()>), grid, block, 0, s, clients, stride, base, n, k, residual,
                               residual_stride, slots, pass, ws);
        }, one_of<SRC_DELTA, SRC_ACCUMULATE, SRC_STORED>(src), vec, base != nullptr);
    };
    const int later = has_res ? SRC_STORED : SRC_DELTA;
    int src = has_res ? SRC_ACCUMULATE : SRC_DELTA;    // of the next pass: the first one with a residual accumulates into it
    if (select) {
        if ((rc = count(src, PASS_DIGIT0)) || (rc = count(later, PASS_DIGIT1)) || (rc = count(later, PASS_DIGIT2))) return rc;
        src = later;
    } else if (quant) {
        if ((rc = count(src, PASS_MAX))) return rc;
        src = later;
    }
    rc = with_consts("fed_compress", [&](auto SRC, auto V, auto B) {
        hipLaunchKernelGGL((compress_sweep_kernel<V(), B(), SRC()>), grid, block, 0, s, clients, stride, base, n, k, levels, residual,
                           residual_stride, slots, seed, offset, kept, ws);
    }, one_of<SRC_DELTA, SRC_ACCUMULATE, SRC_STORED>(src), vec, base != nullptr);
    if (rc) return rc;
    return check_launch("fed_compress");
}

}  // extern "C"
