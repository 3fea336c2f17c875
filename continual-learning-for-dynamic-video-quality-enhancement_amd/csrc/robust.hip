// Byzantine-robust aggregation on the client matrix.
//
//   nvq_fed_trimmed_aggregate  out = base + lr * trimmed mean_k (x_k - base) (+ Gaussian noise) per coordinate: trim = 0 is the
//                              unweighted mean of the live rows, a large trim the coordinate-wise median (Yin et al. 2018)
//   nvq_fed_krum_select        Krum / multi-Krum scores, order and 0/1 selection weights from the update Gram (Blanchard et al.
//                              2017), one workgroup
//
// A row is live when weights == NULL or weights[k] > 0; a row that is not live is never read.  The flat-buffer rule of flat.h: no
// atomics, a grid that depends on n only, whole quads per thread in the vector and in the scalar form alike, sums in double in a
// fixed order: the same bits on every call and at every pointer alignment.
#include <utility>

#include "fed.h"

namespace nvq {

// ------------------------------------------------------------------ keys and the sorting network
// Order-preserving key of a float: negative values flip every bit, the others the sign bit; every NaN, whatever its sign, becomes
// the largest key (after +inf, as np.sort orders it).  fminf / fmaxf drop NaNs; unsigned min / max on the keys do not.
__device__ __forceinline__ unsigned order_key(float x) {
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {               // 0xffffffff comes back as a NaN
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Batcher's odd-even merge sort for N = 2^j keys as a list of compare-exchange pairs built at compile time (63 pairs for 16
// keys, 543 for 64).  Every index is a template argument, so the keys stay in registers (no runtime-indexed array).
template <int N>
struct SortNet {
    int a[N * 12], b[N * 12], count;
    constexpr SortNet() : a{}, b{}, count(0) {
        for (int p = 1; p < N; p <<= 1)
            for (int s = p; s >= 1; s >>= 1)
                for (int j = s % p; j + s < N; j += 2 * s)
                    for (int i = 0; i < s && i + j + s < N; ++i)
                        if ((i + j) / (2 * p) == (i + j + s) / (2 * p)) {
                            a[count] = i + j;
                            b[count] = i + j + s;
                            ++count;
                        }
    }
};
template <int N>
inline constexpr SortNet<N> kSortNet{};

template <int A, int B, int N>
__device__ __forceinline__ int compare_exchange(unsigned (&k)[N]) {
    const unsigned lo = min(k[A], k[B]), hi = max(k[A], k[B]);
    k[A] = lo;
    k[B] = hi;
    return 0;
}
template <int N, size_t... Is>
__device__ __forceinline__ void sort_keys(unsigned (&k)[N], std::index_sequence<Is...>) {
    const int done[] = {compare_exchange<kSortNet<N>.a[Is], kSortNet<N>.b[Is]>(k)...};
    (void)done;
}
template <int N>
__device__ __forceinline__ void sort_keys(unsigned (&k)[N]) {
    sort_keys(k, std::make_index_sequence<kSortNet<N>.count>{});
}

// The next row's address from this one's.  The empty asm hides the chain from the optimiser, which otherwise forms all KMAX row
// addresses ahead of the loads and keeps them live across the sort: two registers instead of 2 KMAX.
__device__ __forceinline__ const float* next_row(const float* p, long stride) {
    p += stride;
    asm volatile("" : "+v"(p));
    return p;
}

// Sorts the keys and adds d = value - base over the sorted positions lo .. hi - 1, ascending, in double.
template <int KMAX>
__device__ __forceinline__ double trimmed_sum(unsigned (&k)[KMAX], float b, int lo, int hi) {
    sort_keys(k);
    // the KMAX range tests are made per lane, where they are used: as uniform tests they are kept as KMAX lane masks across the
    // whole sweep and spill scalar registers
    int first = lo;
    unsigned span = hi - lo;
    asm volatile("" : "+v"(first), "+v"(span));
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        const double d = (double)key_value(k[j]) - (double)b;
        a += (unsigned)(j - first) < span ? d : 0.0;  // a is never -0.0, so adding +0.0 changes nothing
    }
    return a;
}

// The same for one element e.  A row that is not live takes the padding key 0xffffffff without being read: with the NaNs it
// sorts behind the m live values, and the positions below m hold exactly those.  The live rows' values are read as scalars
// (the wide forms and the n % 4 tail).
template <int KMAX>
__device__ __forceinline__ double trimmed_element(const float* __restrict__ clients, long stride, unsigned long live, long e,
                                                  float b, int lo, int hi) {
    unsigned k[KMAX];
    const float* p = clients + e;
    asm volatile("" : "+s"(live));                    // the KMAX liveness tests are made here, not once for the whole sweep
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        k[j] = (live >> j) & 1 ? order_key(*p) : 0xffffffffu;
        p = next_row(p, stride);
    }
    return trimmed_sum(k, b, lo, hi);
}

__device__ __forceinline__ float robust_mix(double sum, int cnt, float b, double lr) {
    const double a = cnt > 0 ? sum / (double)cnt : 0.0;
    return fed_mix(a, b, lr);
}

// KMAX <= 16: the quad's four columns of keys live in registers at once (one 16-byte load per row).  KMAX >= 32: one column at a
// time, the rows read again for the next column (the same 16 bytes per lane: cache hits), so at most KMAX keys are live.
template <bool VEC, bool HAS_BASE, bool NOISE, int KMAX>
__global__ __launch_bounds__(256) void fed_trimmed_kernel(const float* __restrict__ clients, long stride, int K, const float* base,
                                                          const double* __restrict__ weights, int trim, float server_lr,
                                                          float noise_std, long seed, long offset, long n, float* out) {
    unsigned long live = 0;                            // bit k: row k is live.  Uniform: the keys of the other rows are padding
    for (int k = 0; k < K; ++k)
        if (weights == nullptr || weights[k] > 0.0) live |= 1ul << k;
    const int m = __popcll(live);
    const int t = min(trim, (m - 1) / 2);
    const int lo = t, hi = m - t, cnt = m > 0 ? m - 2 * t : 0;
    const double lr = (double)server_lr;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 b = HAS_BASE ? ldq<VEC>(base + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (KMAX <= 16) {
            unsigned kx[KMAX], ky[KMAX], kz[KMAX], kw[KMAX];
            const float* p = clients + 4 * q;
            unsigned long lv = live;
            asm volatile("" : "+s"(lv));
#pragma unroll
            for (int j = 0; j < KMAX; ++j, p = next_row(p, stride)) {
                kx[j] = ky[j] = kz[j] = kw[j] = 0xffffffffu;
                if ((lv >> j) & 1) {
                    const float4 x = ldq<VEC>(p);
                    kx[j] = order_key(x.x);
                    ky[j] = order_key(x.y);
                    kz[j] = order_key(x.z);
                    kw[j] = order_key(x.w);
                }
            }
            v.x = robust_mix(trimmed_sum(kx, b.x, lo, hi), cnt, b.x, lr);
            v.y = robust_mix(trimmed_sum(ky, b.y, lo, hi), cnt, b.y, lr);
            v.z = robust_mix(trimmed_sum(kz, b.z, lo, hi), cnt, b.z, lr);
            v.w = robust_mix(trimmed_sum(kw, b.w, lo, hi), cnt, b.w, lr);
        } else {
#pragma unroll 1
            for (int c = 0; c < 4; ++c) {              // not unrolled: the four columns must not share the register file
                const float bc = c == 0 ? b.x : (c == 1 ? b.y : (c == 2 ? b.z : b.w));
                const float r = robust_mix(trimmed_element<KMAX>(clients, stride, live, 4 * q + c, bc, lo, hi), cnt, bc, lr);
                v.x = c == 0 ? r : v.x;
                v.y = c == 1 ? r : v.y;
                v.z = c == 2 ? r : v.z;
                v.w = c == 3 ? r : v.w;
            }
        }
        fed_noise<NOISE>(v, noise_std, q, seed, offset);
        stq<VEC>(out + 4 * q, v);
    }
    const long e = 4 * nq + threadIdx.x;              // the n % 4 last floats: threads 0..2 of block 0
    if (blockIdx.x == 0 && threadIdx.x < 3 && e < n) {
        const float b = HAS_BASE ? base[e] : 0.f;
        float v = robust_mix(trimmed_element<KMAX>(clients, stride, live, e, b, lo, hi), cnt, b, lr);
        fed_noise_tail<NOISE>(v, noise_std, nq, seed, offset);
        out[e] = v;
    }
}

// ------------------------------------------------------------------ Krum
// (score, index) ascending with NaN scores last
__device__ __forceinline__ bool krum_before(double sa, int a, double sb, int b) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return sa < sb;
    return a < b;
}

// One wave: thread i owns row i.  Its distances to the other live rows go to its row of an LDS table, are sorted there by
// insertion (at most 63 values) and the c smallest are added in ascending order.
__global__ __launch_bounds__(64) void fed_krum_select_kernel(const double* __restrict__ gram, int K,
                                                             const double* __restrict__ weights, int f, int q,
                                                             double* __restrict__ out_weights, double* __restrict__ scores,
                                                             int* __restrict__ order) {
    __shared__ double dist[64][65];
    __shared__ double score[64];
    __shared__ int alive[64];
    const int i = threadIdx.x;
    alive[i] = i < K && (weights == nullptr || weights[i] > 0.0);
    __syncthreads();
    int m = 0, dead_before = 0;
    for (int j = 0; j < K; ++j) {
        m += alive[j];
        if (j < i) dead_before += !alive[j];
    }
    const bool mine = alive[i] != 0;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    int c = m - f - 2;
    c = c < 1 ? 1 : c;
    c = c > m - 1 ? m - 1 : c;
    double s = inf;
    if (mine) {
        const double gii = gram[i * K + i];
        double* row = dist[i];
        int cnt = 0;
        for (int j = 0; j < K; ++j) {
            if (j == i || !alive[j]) continue;
            double d = gii + gram[j * K + j] - 2.0 * gram[i * K + j];
            if (d != d) d = inf;                      // a NaN distance counts as the largest
            else if (d < 0.0) d = 0.0;
            int p = cnt++;
            for (; p > 0 && row[p - 1] > d; --p) row[p] = row[p - 1];
            row[p] = d;
        }
        s = 0.0;
        for (int p = 0; p < c; ++p) s += row[p];
    }
    score[i] = s;
    __syncthreads();
    if (i >= K) return;
    scores[i] = s;
    int rank;
    if (mine) {
        rank = 0;
        for (int j = 0; j < K; ++j)
            if (j != i && alive[j] && krum_before(score[j], j, s, i)) ++rank;
    } else {
        rank = m + dead_before;
    }
    order[rank] = i;
    out_weights[i] = mine && rank < q ? 1.0 : 0.0;
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_fed_trimmed_aggregate(const float* clients, long stride, int K, const float* base, const double* weights, int trim,
                              float server_lr, float noise_std, long seed, long offset, long n, float* out, void* stream) {
    int rc = fed_check("fed_trimmed_aggregate", clients, stride, K, n, seed, offset, noise_std);
    if (rc) return rc;
    NVQ_REQUIRE(out != nullptr && trim >= 0, "fed_trimmed_aggregate: out / trim = %d", trim);
    NVQ_REQUIRE(aligned8(weights), "fed_trimmed_aggregate: weights must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = fed_vec(clients, stride, base, out);
    const dim3 grid(flat_blocks(n)), block(256);
    const int kmax = K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64;
    rc = with_consts("fed_trimmed_aggregate", [&](auto KM, auto V, auto B, auto N) {
        hipLaunchKernelGGL((fed_trimmed_kernel<V(), B(), N(), KM()>), grid, block, 0, s, clients, stride, K, base, weights, trim,
                           server_lr, noise_std, seed, offset, n, out);
    }, one_of<8, 16, 32, 64>(kmax), vec, base != nullptr, noise_std != 0.f);
    if (rc) return rc;
    return check_launch("fed_trimmed_aggregate");
}

int nvq_fed_krum_select(const double* gram, int K, const double* weights, int num_byzantine, int num_selected,
                        double* out_weights, double* scores, int* order, void* stream) {
    NVQ_REQUIRE(gram != nullptr && out_weights != nullptr && scores != nullptr && order != nullptr, "fed_krum_select: null pointer");
    NVQ_REQUIRE(K >= 1 && K <= 64, "fed_krum_select: K = %d outside 1 .. 64", K);
    NVQ_REQUIRE(num_byzantine >= 0 && num_selected >= 1, "fed_krum_select: num_byzantine = %d, num_selected = %d", num_byzantine,
                num_selected);
    NVQ_REQUIRE(aligned8(gram) && aligned8(weights) && aligned8(out_weights) && aligned8(scores) && aligned4(order),
                "fed_krum_select: alignment");
    hipLaunchKernelGGL(fed_krum_select_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gram, K, weights, num_byzantine,
                       num_selected, out_weights, scores, order);
    return check_launch("fed_krum_select");
}

}  // extern "C"
