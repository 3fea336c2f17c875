// Two-sample Kolmogorov-Smirnov test per feature on device-resident samples: every feature's values sorted
// in LDS, the two-sided statistic as an exact integer from upper-bound ranks, and scipy's exact p-value as a hypergeometric
// walk over the lattice of draws that only ever adds positive terms.  No float atomics: every p-value is a function of
// (n1, n2, h) only.
#include <cmath>

#include "flat.h"

namespace nvq {

constexpr int KS_MAX_N = 4096;    // rows of one set: a column is sorted in LDS (16 KiB of keys)
constexpr int KS_SLAB = 4;        // neighbouring features staged and sorted by one workgroup: 16-byte runs of every input row

// ------------------------------------------------------------------------------------------------------------ sort
// Features [4 blockIdx.x, + 4) of the row-major (rows x d) matrix x, rows gathered through idx when given, as ascending
// columns of the feature-major (d x n) matrix out.  A bitonic network over npad = 2^lp >= n keys per feature; the padding is
// +inf, lives in LDS only and sorts behind every value (a real +inf equals it), so the first n keys are the column.  -0.0 is
// stored as +0.0.  An index outside [0, rows) reads as 0, as in the Gram kernel.  A NaN makes comparisons false and the order
// of its column meaningless, but a compare-exchange only ever swaps two LDS cells of its own column.
__global__ __launch_bounds__(256) void sort_columns_kernel(const float* __restrict__ x, const int* __restrict__ idx, int n, int rows,
                                                           int d, int lp, float* __restrict__ out) {
    __shared__ float keys[KS_SLAB * KS_MAX_N];
    const int npad = 1 << lp;
    const int f0 = blockIdx.x * KS_SLAB;
    const int nf = d - f0 < KS_SLAB ? d - f0 : KS_SLAB;
    for (int e = threadIdx.x; e < npad * KS_SLAB; e += 256) {
        const int i = e / KS_SLAB, f = e % KS_SLAB;
        float v = INFINITY;
        if (i < n && f < nf) {
            const int src = idx ? idx[i] : i;
            v = 0.f;
            if (src >= 0 && src < rows) v = x[(size_t)src * d + f0 + f];
            if (v == 0.f) v = 0.f;                                      // -0.0 ties with +0.0: one representation
        }
        keys[f * npad + i] = v;
    }
    __syncthreads();
    const int lh = lp > 0 ? lp - 1 : 0;                                 // npad = 1: no stage runs
    const int pairs = nf << lh;                                         // npad / 2 compare-exchanges per feature and stage
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = threadIdx.x; e < pairs; e += 256) {
                const int f = e >> lh, p = e & ((1 << lh) - 1);
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));    // bit j of i is clear
                const int l = i | j;
                float* col = keys + f * npad;
                const float lo = col[i], hi = col[l];
                if ((lo > hi) == ((i & k) == 0)) {
                    col[i] = hi;
                    col[l] = lo;
                }
            }
            __syncthreads();
        }
    }
    for (int e = threadIdx.x; e < nf * n; e += 256) {
        const int f = e / n, i = e - f * n;
        out[(size_t)(f0 + f) * n + i] = keys[f * npad + i];
    }
}

// ------------------------------------------------------------------------------------------------------------ statistic
// #{col[0 .. n) <= v} for an ascending column: numpy's searchsorted(side='right').  lo and hi stay in [0, n] whatever v is.
__device__ __forceinline__ int upper_bound(const float* col, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One workgroup per feature.  h = max over every value v of either sample of |a #{ref <= v} - b #{cur <= v}| with
// a = n2 / gcd, b = n1 / gcd: lcm(n1, n2) times the largest distance between the two empirical distribution functions, taken
// after all copies of v.  Integers throughout (a n1 = lcm <= 2^24).
__global__ __launch_bounds__(256) void ks_statistic_kernel(const float* __restrict__ ref, const float* __restrict__ cur, int n1, int n2,
                                                           int a, int b, double lcm, int* __restrict__ h_out,
                                                           double* __restrict__ d_out) {
    __shared__ float rs[KS_MAX_N];
    __shared__ float cs[KS_MAX_N];
    __shared__ int wmax[4];
    const size_t f = blockIdx.x;
    for (int i = threadIdx.x; i < n1; i += 256) rs[i] = ref[f * n1 + i];
    for (int i = threadIdx.x; i < n2; i += 256) cs[i] = cur[f * n2 + i];
    __syncthreads();
    int h = 0;
    for (int e = threadIdx.x; e < n1 + n2; e += 256) {
        const float v = e < n1 ? rs[e] : cs[e - n1];
        const int t = a * upper_bound(rs, n1, v) - b * upper_bound(cs, n2, v);
        h = max(h, t < 0 ? -t : t);
    }
    for (int o = 32; o > 0; o >>= 1) h = max(h, __shfl_xor(h, o, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        h = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        h_out[f] = h;
        d_out[f] = (double)h / lcm;
    }
}

// ------------------------------------------------------------------------------------------------------------ p-value
// The walk.  Draw the pooled sample without replacement: after s - 1 draws, x of them from the first sample and y from the
// second, the next one comes from the first with probability (n1 - x) / rem and from the second with (n2 - y) / rem,
// rem = n1 + n2 - (s - 1).  The empirical distribution functions differ by (a x - b y) / lcm at (x, y), so a path stays
// strictly below the observed distance while |a x - b y| < h: the band.  Mass that steps out of the band is the p-value's and
// leaves the walk.  Only positive terms are ever added, so a p-value of 1e-35 is as accurate, relatively, as one of 0.5.
//
// Cells of one anti-diagonal x + y = s are indexed by x; with A = a + b the band is |A x - b s| < h, and both its ends move
// up by at most one per step (b < A), so they are kept incrementally.  [lo, hi] are the live cells of the previous
// anti-diagonal, clipped to the lattice; the cells they can reach are [lo, hi + 1].  Two buffers, one barrier per step.
// SINGLE: the band never holds more than 63 cells, one wave walks it alone and a step needs no barrier.
template <bool SINGLE>
__device__ __forceinline__ void step_sync() {
    if (SINGLE) {
        __threadfence_block();                                          // the wave's own LDS writes, in order, before its reads
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <bool SINGLE, int CAP>
__device__ __forceinline__ double ks_walk(double (*cell)[CAP], int h, int n1, int n2, int a, int b, int blo, int bhi) {
    constexpr int NT = SINGLE ? 64 : 256;
    const int A = a + b, N = n1 + n2;
    if (threadIdx.x == 0) cell[0][0] = 1.0;
    step_sync<SINGLE>();
    int lo = 0, hi = 0, buf = 0, bs = 0;
    double acc = 0.0;
    for (int s = 1; s <= N; ++s) {
        bs += b;
        if (A * blo - bs <= -h) ++blo;
        if (A * (bhi + 1) - bs < h) ++bhi;
        const int nlo = max(blo, max(0, s - n2)), nhi = min(bhi, min(n1, s));
        const double rem = (double)(N - s + 1);
        const double* old = cell[buf];
        double* nw = cell[buf ^ 1];
        for (int x = lo + (int)threadIdx.x; x <= hi + 1; x += NT) {
            double m = 0.0;
            if (x > lo) m = old[x - 1] * (double)(n1 - x + 1);          // from (x - 1, y): a draw from the first sample
            if (x <= hi) m += old[x] * (double)(n2 - (s - 1 - x));      // from (x, y - 1): a draw from the second
            m /= rem;
            if (x >= nlo && x <= nhi) nw[x] = m;
            else acc += m;
        }
        lo = nlo;
        hi = nhi;
        buf ^= 1;
        if (lo > hi) break;                                             // nothing left inside the band (block-uniform)
        step_sync<SINGLE>();
    }
    return acc;
}

template <int CAP>
__global__ __launch_bounds__(256) void ks_pvalue_kernel(const int* __restrict__ h_in, int n1, int n2, int a, int b, int lcm,
                                                        double* __restrict__ p_out) {
    __shared__ double cell[2][CAP];
    __shared__ double scratch[4];
    const int h = h_in[blockIdx.x];
    if (h <= 0 || h > lcm) {                                            // no distance at all: p = 1; beyond the largest possible: 0
        if (threadIdx.x == 0) p_out[blockIdx.x] = h <= 0 ? 1.0 : 0.0;
        return;
    }
    const int w0 = (h + a + b - 1) / (a + b);                           // the band at s = 0 is |x| < h / A: x in [1 - w0, w0 - 1]
    double p;
    if (2 * w0 + 1 <= 64) {                                             // at most 2 w0 live cells, 2 w0 + 1 reachable ones
        if (threadIdx.x >= 64) return;
        p = wave_sum(ks_walk<true, CAP>(cell, h, n1, n2, a, b, 1 - w0, w0 - 1));
    } else {
        p = wave_sum(ks_walk<false, CAP>(cell, h, n1, n2, a, b, 1 - w0, w0 - 1));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = p;
        __syncthreads();
        p = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    }
    if (threadIdx.x == 0) p_out[blockIdx.x] = p < 1.0 ? p : 1.0;
}

// One block: score = d min_i p_i (the reference's Bonferroni correction, not clamped), flag = score < threshold.
__global__ __launch_bounds__(256) void ks_finish_kernel(const double* __restrict__ p, int d, double threshold, double* __restrict__ score,
                                                        unsigned char* __restrict__ flag) {
    __shared__ double wmin[4];
    double m = INFINITY;
    for (int i = threadIdx.x; i < d; i += 256) m = fmin(m, p[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = fmin(fmin(wmin[0], wmin[1]), fmin(wmin[2], wmin[3])) * (double)d;
        score[0] = s;
        flag[0] = s < threshold ? 1 : 0;
    }
}

static int gcd_int(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_sort_columns(const float* x, const int* index, int n, int rows, int d, float* out, void* stream) {
    NVQ_REQUIRE(x != nullptr && out != nullptr, "sort_columns: x / out");
    NVQ_REQUIRE(n >= 1 && n <= KS_MAX_N && d >= 1, "sort_columns: n must be in [1, %d] and d >= 1 (got %d, %d)", KS_MAX_N, n, d);
    NVQ_REQUIRE(rows >= 1 && (index != nullptr || n <= rows), "sort_columns: %d rows asked of a matrix with %d rows", n, rows);
    int lp = 0;
    while ((1 << lp) < n) ++lp;
    hipLaunchKernelGGL(sort_columns_kernel, dim3((unsigned)ceil_div(d, KS_SLAB)), dim3(256), 0, (hipStream_t)stream, x, index, n, rows,
                       d, lp, out);
    return check_launch("sort_columns");
}

int nvq_ks_statistic(const float* ref_sorted, const float* cur_sorted, int n1, int n2, int d, int* h_out, double* d_out,
                     void* stream) {
    NVQ_REQUIRE(ref_sorted != nullptr && cur_sorted != nullptr && h_out != nullptr && d_out != nullptr,
                "ks_statistic: ref_sorted / cur_sorted / h_out / d_out");
    NVQ_REQUIRE(n1 >= 1 && n1 <= KS_MAX_N && n2 >= 1 && n2 <= KS_MAX_N && d >= 1,
                "ks_statistic: n1, n2 must be in [1, %d] and d >= 1 (got %d, %d, %d)", KS_MAX_N, n1, n2, d);
    NVQ_REQUIRE(aligned8(d_out), "ks_statistic: d_out must be 8-byte aligned");
    const int g = gcd_int(n1, n2), a = n2 / g, b = n1 / g;
    hipLaunchKernelGGL(ks_statistic_kernel, dim3((unsigned)d), dim3(256), 0, (hipStream_t)stream, ref_sorted, cur_sorted, n1, n2, a, b,
                       (double)a * (double)n1, h_out, d_out);
    return check_launch("ks_statistic");
}

int nvq_ks_pvalue(const int* h, int n1, int n2, int d, double* p_out, void* stream) {
    NVQ_REQUIRE(h != nullptr && p_out != nullptr, "ks_pvalue: h / p_out");
    NVQ_REQUIRE(n1 >= 1 && n1 <= KS_MAX_N && n2 >= 1 && n2 <= KS_MAX_N && d >= 1,
                "ks_pvalue: n1, n2 must be in [1, %d] and d >= 1 (got %d, %d, %d)", KS_MAX_N, n1, n2, d);
    NVQ_REQUIRE(aligned8(p_out), "ks_pvalue: p_out must be 8-byte aligned");
    const int g = gcd_int(n1, n2), a = n2 / g, b = n1 / g;
    hipStream_t s = (hipStream_t)stream;
    if (n1 <= 1024) hipLaunchKernelGGL(ks_pvalue_kernel<1025>, dim3((unsigned)d), dim3(256), 0, s, h, n1, n2, a, b, a * n1, p_out);
    else hipLaunchKernelGGL(ks_pvalue_kernel<KS_MAX_N + 1>, dim3((unsigned)d), dim3(256), 0, s, h, n1, n2, a, b, a * n1, p_out);
    return check_launch("ks_pvalue");
}

int nvq_ks_finish(const double* p, int d, const double* threshold_host, double* score_out, unsigned char* flag_out, void* stream) {
    NVQ_REQUIRE(p != nullptr && threshold_host != nullptr && score_out != nullptr && flag_out != nullptr,
                "ks_finish: p / threshold_host / score_out / flag_out");
    NVQ_REQUIRE(d >= 1, "ks_finish: d must be >= 1 (got %d)", d);
    NVQ_REQUIRE(aligned8(p) && aligned8(score_out), "ks_finish: p and score_out must be 8-byte aligned");
    hipLaunchKernelGGL(ks_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p, d, threshold_host[0], score_out, flag_out);
    return check_launch("ks_finish");
}

}  // extern "C"
