// Federated rounds and differential privacy on flat fp32 buffers.
//
//   nvq_fed_delta_norms   sq[k] = |x_k - base|^2 for the K rows of a client matrix, one pass
//   nvq_fed_aggregate     out = base + lr * sum_k c_k (x_k - base) (+ Gaussian noise): FedAvg, clipped updates, server step
//   nvq_dp_segment_norms  sq[s] = |g_s|^2 per slot of a gradient bucket
//   nvq_dp_clip_noise     g_s = g_s * min(1, C / (|g_s| + 1e-6)) + sigma z per slot, padding kept at zero
//
// No atomics; every grid depends on the sizes only; every thread owns whole quads (4 consecutive floats) in the vector and
// in the scalar form alike and adds in one order, so a result depends neither on pointer alignment nor on the call.  The
// noise is Philox4x32-10 keyed by (seed), counted by (quad index, offset): a function of (seed, offset, element) alone.
#include "fed.h"

namespace nvq {

// ------------------------------------------------------------------ client-update norms
#define NVQ_SQDIFF(acc, xv, bv)                                \
    do {                                                       \
        const double d_ = (double)(xv) - (double)(bv);         \
        acc = fma(d_, d_, acc);                                \
    } while (0)

// part[blockIdx.x * K + k] = this block's share of |x_k - base|^2.  KMAX accumulators live in registers (fully unrolled).
template <bool VEC, bool HAS_BASE, int KMAX>
__global__ __launch_bounds__(256) void fed_delta_norms_kernel(const float* __restrict__ clients, long stride, int K,
                                                              const float* __restrict__ base, long n, double* __restrict__ part) {
    __shared__ double scratch[4 * KMAX];
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 b = HAS_BASE ? ldq<VEC>(base + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K) {
                const float4 x = ldq<VEC>(clients + k * stride + 4 * q);
                NVQ_SQDIFF(acc[k], x.x, b.x);
                NVQ_SQDIFF(acc[k], x.y, b.y);
                NVQ_SQDIFF(acc[k], x.z, b.z);
                NVQ_SQDIFF(acc[k], x.w, b.w);
            }
        }
    }
    const long t = 4 * nq + threadIdx.x;              // the n % 4 last floats: threads 0..2 of block 0
    if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) {
        const float b = HAS_BASE ? base[t] : 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) NVQ_SQDIFF(acc[k], clients[k * stride + t], b);
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            const double v = wave_sum(acc[k]);
            if ((threadIdx.x & 63) == 0) scratch[wave * KMAX + k] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x;
        part[(long)blockIdx.x * K + k] = scratch[k] + scratch[KMAX + k] + scratch[2 * KMAX + k] + scratch[3 * KMAX + k];
    }
}

// block k: sq[k] = sum over the blocks' partials, thread t takes blocks t, t + 256, ..., then the block sum: a fixed order
__global__ __launch_bounds__(256) void fed_delta_norms_final_kernel(const double* __restrict__ part, int nblk, int K,
                                                                    double* __restrict__ sq) {
    __shared__ double scratch[4];
    const int k = blockIdx.x;
    double v = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) v += part[(long)b * K + k];
    block_wave_sum_256(scratch, v);
    if (threadIdx.x == 0) sq[k] = v;
}

// ------------------------------------------------------------------ aggregate
// fed_mean_quad / fed_mean_tail (fed.h) over all K rows in index order
template <bool VEC, bool HAS_BASE, bool NOISE>
__global__ __launch_bounds__(256) void fed_aggregate_kernel(const float* __restrict__ clients, long stride, int K,
                                                            const float* base, const double* __restrict__ weights,
                                                            const double* __restrict__ sq, float clip_norm, float server_lr,
                                                            float noise_std, long seed, long offset, long n, float* out) {
    __shared__ double coef[64];
    fed_coefficients(coef, weights, sq, clip_norm, K);
    const auto row = [](int m) { return m; };
    const double lr = (double)server_lr;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 b = HAS_BASE ? ldq<VEC>(base + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        stq<VEC>(out + 4 * q, fed_mean_quad<VEC, NOISE>(clients, stride, q, b, coef, row, 0, K, lr, noise_std, seed, offset));
    }
    const long t = 4 * nq + threadIdx.x;
    if (flat_tail(n, t)) {
        const float b = HAS_BASE ? base[t] : 0.f;
        out[t] = fed_mean_tail<NOISE>(clients, stride, t, nq, b, coef, row, 0, K, lr, noise_std, seed, offset);
    }
}

// ------------------------------------------------------------------ per-slot DP on a gradient bucket
// chunks[c] = {slot, first quad of the bucket, quads}: one block per chunk, sorted by slot.  A chunk that does not lie inside
// its slot is skipped (the tables are device memory: the host side cannot check them).
__device__ __forceinline__ bool dp_chunk(const int* __restrict__ chunks, const long* __restrict__ seg_off,
                                         const long* __restrict__ seg_numel, int S, int& s, long& q0, long& q1, long& e0,
                                         long& e1) {
    s = chunks[3 * blockIdx.x];
    if (s < 0 || s >= S) return false;
    q0 = chunks[3 * blockIdx.x + 1];
    q1 = q0 + chunks[3 * blockIdx.x + 2];
    e0 = seg_off[s];
    e1 = e0 + seg_numel[s];
    return q0 >= 0 && q1 >= q0 && (e0 & 3) == 0 && e0 >= 0 && 4 * q0 >= e0 && 4 * q1 <= ((e1 + 3) & ~3L);
}

__global__ __launch_bounds__(256) void dp_segment_norms_kernel(const float* __restrict__ g, const long* __restrict__ seg_off,
                                                               const long* __restrict__ seg_numel, int S,
                                                               const int* __restrict__ chunks, double* __restrict__ part) {
    __shared__ double scratch[4];
    int s;
    long q0, q1, e0, e1;
    double v = 0.0;
    if (dp_chunk(chunks, seg_off, seg_numel, S, s, q0, q1, e0, e1)) {
        for (long q = q0 + threadIdx.x; q < q1; q += 256) {
            const float4 a = ld4(g + 4 * q);
            const long e = 4 * q;
            const double x = (double)a.x, y = e + 1 < e1 ? (double)a.y : 0.0, z = e + 2 < e1 ? (double)a.z : 0.0,
                         w = e + 3 < e1 ? (double)a.w : 0.0;
            if (e < e1) v = fma(x, x, v);
            v = fma(y, y, v);
            v = fma(z, z, v);
            v = fma(w, w, v);
        }
    }
    block_wave_sum_256(scratch, v);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// thread s: sq[s] = the sum of slot s's chunks in table order (its first chunk by bisection: the table is sorted by slot)
__global__ __launch_bounds__(256) void dp_segment_norms_final_kernel(const double* __restrict__ part,
                                                                     const int* __restrict__ chunks, int n_chunks, int S,
                                                                     double* __restrict__ sq) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int lo = 0, hi = n_chunks;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (chunks[3 * mid] < s) lo = mid + 1;
        else hi = mid;
    }
    double v = 0.0;
    for (int c = lo; c < n_chunks && chunks[3 * c] == s; ++c) v += part[c];
    sq[s] = v;
}

template <bool NOISE>
__global__ __launch_bounds__(256) void dp_clip_noise_kernel(float* __restrict__ g, const long* __restrict__ seg_off,
                                                            const long* __restrict__ seg_numel, int S,
                                                            const int* __restrict__ chunks, const double* __restrict__ sq,
                                                            float max_norm, float noise_scale, long seed, long offset) {
    int s;
    long q0, q1, e0, e1;
    if (!dp_chunk(chunks, seg_off, seg_numel, S, s, q0, q1, e0, e1)) return;
    double coef = (double)max_norm / (sqrt(sq[s]) + 1e-6);
    if (!(coef < 1.0)) coef = 1.0;
    const float cf = (float)coef;
    if (!NOISE && cf == 1.0f) return;                 // a slot under the bound keeps its bits
    for (long q = q0 + threadIdx.x; q < q1; q += 256) {
        float4 a = ld4(g + 4 * q);
        a.x = __fmul_rn(a.x, cf);
        a.y = __fmul_rn(a.y, cf);
        a.z = __fmul_rn(a.z, cf);
        a.w = __fmul_rn(a.w, cf);
        fed_noise<NOISE>(a, noise_scale, q, seed, offset);
        const long e = 4 * q;                          // the slot's padding stays exactly zero: those draws are dropped
        if (e + 1 >= e1) a.y = 0.f;
        if (e + 2 >= e1) a.z = 0.f;
        if (e + 3 >= e1) a.w = 0.f;
        if (e >= e1) a.x = 0.f;
        st4(g + 4 * q, a);
    }
}

static int dp_check(const char* what, const float* g, const long* seg_off, const long* seg_numel, int S, const int* chunks,
                    int n_chunks, const double* sq) {
    NVQ_REQUIRE(g != nullptr && seg_off != nullptr && seg_numel != nullptr && chunks != nullptr && sq != nullptr,
                "%s: null pointer", what);
    NVQ_REQUIRE(S >= 1 && n_chunks >= 1, "%s: S = %d, n_chunks = %d", what, S, n_chunks);
    NVQ_REQUIRE(aligned16(g), "%s: the bucket must be 16-byte aligned (slots are whole quads)", what);
    NVQ_REQUIRE(aligned8(seg_off) && aligned8(seg_numel) && aligned8(sq) && aligned4(chunks), "%s: table alignment", what);
    return NVQ_OK;
}

}  // namespace nvq

using namespace nvq;

extern "C" {

size_t nvq_fed_workspace_bytes(int K, long n) {
    if (K < 1 || n < 0) return 0;
    return (size_t)flat_blocks(n) * (size_t)K * sizeof(double);
}

int nvq_fed_delta_norms(const float* clients, long stride, int K, const float* base, long n, double* sq, float* workspace,
                        size_t workspace_bytes, void* stream) {
    int rc = fed_check("fed_delta_norms", clients, stride, K, n);
    if (rc) return rc;
    NVQ_REQUIRE(sq != nullptr && aligned8(sq) && aligned8(workspace), "fed_delta_norms: sq / 8-byte alignment");
    const int nb = flat_blocks(n);
    if (workspace == nullptr || (size_t)nb * K * sizeof(double) > workspace_bytes) {
        set_error("fed_delta_norms: workspace");
        return NVQ_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    const bool vec = fed_vec(clients, stride, base);
    const dim3 grid(nb), block(256);
    with_bools([&](auto V, auto B) {
        const auto kernel = K <= 8    ? fed_delta_norms_kernel<V(), B(), 8>
                            : K <= 16 ? fed_delta_norms_kernel<V(), B(), 16>
                                      : fed_delta_norms_kernel<V(), B(), 64>;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, clients, stride, K, base, n, part);
    }, vec, base != nullptr);
    rc = check_launch("fed_delta_norms");
    if (rc) return rc;
    hipLaunchKernelGGL(fed_delta_norms_final_kernel, dim3(K), dim3(256), 0, s, part, nb, K, sq);
    return check_launch("fed_delta_norms_final");
}

int nvq_fed_aggregate(const float* clients, long stride, int K, const float* base, const double* weights, const double* sq,
                      float clip_norm, float server_lr, float noise_std, long seed, long offset, long n, float* out,
                      void* stream) {
    int rc = fed_check("fed_aggregate", clients, stride, K, n, seed, offset, noise_std);
    if (rc) return rc;
    NVQ_REQUIRE(weights != nullptr && out != nullptr, "fed_aggregate: weights / out");
    NVQ_REQUIRE(sq == nullptr || clip_norm >= 0.f, "fed_aggregate: clip_norm");
    NVQ_REQUIRE(aligned8(weights) && aligned8(sq), "fed_aggregate: weights and sq must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = fed_vec(clients, stride, base, out);
    const dim3 grid(flat_blocks(n)), block(256);
    with_bools([&](auto V, auto B, auto N) {
        hipLaunchKernelGGL((fed_aggregate_kernel<V(), B(), N()>), grid, block, 0, s, clients, stride, K, base, weights, sq,
                           clip_norm, server_lr, noise_std, seed, offset, n, out);
    }, vec, base != nullptr, noise_std != 0.f);
    return check_launch("fed_aggregate");
}

int nvq_dp_segment_norms(const float* g, const long* seg_off, const long* seg_numel, int S, const int* chunks, int n_chunks,
                         double* sq, float* workspace, size_t workspace_bytes, void* stream) {
    int rc = dp_check("dp_segment_norms", g, seg_off, seg_numel, S, chunks, n_chunks, sq);
    if (rc) return rc;
    NVQ_REQUIRE(aligned8(workspace), "dp_segment_norms: workspace must be 8-byte aligned");
    if (workspace == nullptr || (size_t)n_chunks * sizeof(double) > workspace_bytes) {
        set_error("dp_segment_norms: workspace");
        return NVQ_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(dp_segment_norms_kernel, dim3(n_chunks), dim3(256), 0, s, g, seg_off, seg_numel, S, chunks, part);
    rc = check_launch("dp_segment_norms");
    if (rc) return rc;
    hipLaunchKernelGGL(dp_segment_norms_final_kernel, dim3(ceil_div(S, 256)), dim3(256), 0, s, part, chunks, n_chunks, S, sq);
    return check_launch("dp_segment_norms_final");
}

int nvq_dp_clip_noise(float* g, const long* seg_off, const long* seg_numel, int S, const int* chunks, int n_chunks,
                      const double* sq, float max_norm, float noise_scale, long seed, long offset, void* stream) {
    int rc = dp_check("dp_clip_noise", g, seg_off, seg_numel, S, chunks, n_chunks, sq);
    if (rc) return rc;
    NVQ_REQUIRE(seed >= 0 && offset >= 0, "dp_clip_noise: seed and offset are non-negative");
    NVQ_REQUIRE(max_norm >= 0.f && noise_scale >= 0.f, "dp_clip_noise: max_norm / noise_scale");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(n_chunks), block(256);
    with_bools([&](auto N) {
        hipLaunchKernelGGL(dp_clip_noise_kernel<N()>, grid, block, 0, s, g, seg_off, seg_numel, S, chunks, sq, max_norm,
                           noise_scale, seed, offset);
    }, noise_scale != 0.f);
    return check_launch("dp_clip_noise");
}

}  // extern "C"
