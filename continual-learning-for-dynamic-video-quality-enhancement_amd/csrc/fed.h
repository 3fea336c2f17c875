// What the sweeps over a [K, n] client matrix share (DESIGN.md sections 23, 25, 28): the server step, the clip coefficient, the
// Gaussian-noise epilogue of a quad and of the n % 4 tail, the weighted mean of a set of rows around a base, and the host-side
// argument checks of the nvq_fed_* entry points.  federated.hip, cluster.hip, robust.hip and fedopt.hip include this header in
// place of flat.h and philox.h; a further aggregation rule includes it too and writes only what is its own.
#pragma once
#include "flat.h"
#include "philox.h"

namespace nvq {

// the server step: base + lr * (aggregated update), rounded to fp32 once
__device__ __forceinline__ float fed_mix(double a, float b, double lr) { return (float)fma(lr, a, (double)b); }

// min(1, clip_norm / (|x_k - base| + 1e-6)) from the squared norms, 1 without them.  !(s < 1): a NaN norm does not clip.
__device__ __forceinline__ double fed_clip(const double* __restrict__ sq, int k, float clip_norm) {
    if (sq == nullptr) return 1.0;
    double s = (double)clip_norm / (sqrt(sq[k]) + 1e-6);
    if (!(s < 1.0)) s = 1.0;
    return s;
}

// v += noise_std * z for quad q of the Philox stream (seed, offset)
template <bool NOISE>
__device__ __forceinline__ void fed_noise(float4& v, float noise_std, long q, long seed, long offset) {
    if (!NOISE) return;
    const float4 z = quad_normals(q, seed, offset);
    v.x = fmaf(noise_std, z.x, v.x);
    v.y = fmaf(noise_std, z.y, v.y);
    v.z = fmaf(noise_std, z.z, v.z);
    v.w = fmaf(noise_std, z.w, v.w);
}

// the same for tail element 4 nq + threadIdx.x (flat_tail): lane threadIdx.x of quad nq's draws
template <bool NOISE>
__device__ __forceinline__ void fed_noise_tail(float& v, float noise_std, long nq, long seed, long offset) {
    if (!NOISE) return;
    const float4 z = quad_normals(nq, seed, offset);
    v = fmaf(noise_std, threadIdx.x == 0 ? z.x : (threadIdx.x == 1 ? z.y : z.z), v);
}

// Quad q of the aggregated update sum_m coef[row(m)] (x_row(m) - b) over m0 <= m < m1, in double and not rounded: m ascending,
// one fma chain per lane of the quad.
template <bool VEC, class Row>
__device__ __forceinline__ double4 fed_delta_quad(const float* __restrict__ clients, long stride, long q, float4 b,
                                                  const double* coef, Row row, int m0, int m1) {
    double ax = 0.0, ay = 0.0, az = 0.0, aw = 0.0;
    for (int m = m0; m < m1; ++m) {
        const int k = row(m);
        const float4 x = ldq<VEC>(clients + k * stride + 4 * q);
        const double c = coef[k];
        ax = fma(c, (double)x.x - (double)b.x, ax);
        ay = fma(c, (double)x.y - (double)b.y, ay);
        az = fma(c, (double)x.z - (double)b.z, az);
        aw = fma(c, (double)x.w - (double)b.w, aw);
    }
    return make_double4(ax, ay, az, aw);
}

// The same for tail element t = 4 nq + threadIdx.x.
template <class Row>
__device__ __forceinline__ double fed_delta_tail(const float* __restrict__ clients, long stride, long t, float b,
                                                 const double* coef, Row row, int m0, int m1) {
    double a = 0.0;
    for (int m = m0; m < m1; ++m) {
        const int k = row(m);
        a = fma(coef[k], (double)clients[k * stride + t] - (double)b, a);
    }
    return a;
}

// Quad q of b + lr * (fed_delta_quad), plus noise.
template <bool VEC, bool NOISE, class Row>
__device__ __forceinline__ float4 fed_mean_quad(const float* __restrict__ clients, long stride, long q, float4 b,
                                                const double* coef, Row row, int m0, int m1, double lr, float noise_std,
                                                long seed, long offset) {
    const double4 a = fed_delta_quad<VEC>(clients, stride, q, b, coef, row, m0, m1);
    float4 v = make_float4(fed_mix(a.x, b.x, lr), fed_mix(a.y, b.y, lr), fed_mix(a.z, b.z, lr), fed_mix(a.w, b.w, lr));
    fed_noise<NOISE>(v, noise_std, q, seed, offset);
    return v;
}

// The same for tail element t = 4 nq + threadIdx.x.
template <bool NOISE, class Row>
__device__ __forceinline__ float fed_mean_tail(const float* __restrict__ clients, long stride, long t, long nq, float b,
                                               const double* coef, Row row, int m0, int m1, double lr, float noise_std,
                                               long seed, long offset) {
    float v = fed_mix(fed_delta_tail(clients, stride, t, b, coef, row, m0, m1), b, lr);
    fed_noise_tail<NOISE>(v, noise_std, nq, seed, offset);
    return v;
}

// coef[k] = weights[k] / W * fed_clip(sq, k, clip_norm) in shared memory, W the sum of the K weights in index order; ends with
// the barrier after which every thread may read coef.
__device__ __forceinline__ void fed_coefficients(double* coef, const double* __restrict__ weights, const double* __restrict__ sq,
                                                 float clip_norm, int K) {
    if ((int)threadIdx.x < K) {
        double W = 0.0;
        for (int k = 0; k < K; ++k) W += weights[k];
        const int k = threadIdx.x;
        coef[k] = weights[k] / W * fed_clip(sq, k, clip_norm);
    }
    __syncthreads();
}

// ------------------------------------------------------------------ host side
// The client matrix of the entry point `what`: K rows (1 .. 64) of n floats, `stride` floats apart; an aggregate passes its Philox
// stream and noise level too.
inline int fed_check(const char* what, const float* clients, long stride, int K, long n, long seed = 0, long offset = 0,
                     float noise_std = 0.f) {
    NVQ_REQUIRE(clients != nullptr && n >= 0, "%s: clients / n", what);
    NVQ_REQUIRE(K >= 1 && K <= 64, "%s: K = %d outside 1 .. 64", what, K);
    NVQ_REQUIRE(stride >= n, "%s: stride %ld < n %ld", what, stride, n);
    NVQ_REQUIRE(seed >= 0 && offset >= 0, "%s: seed and offset are non-negative", what);
    NVQ_REQUIRE(noise_std >= 0.f, "%s: noise_std", what);
    return NVQ_OK;
}

// 16-byte loads and stores are in order when the matrix and every vector that is given are aligned
inline bool fed_vec(const float* clients, long stride, const float* base, const float* out = nullptr) {
    return aligned16(clients) && (stride & 3) == 0 && aligned16(base) && aligned16(out);
}

}  // namespace nvq
