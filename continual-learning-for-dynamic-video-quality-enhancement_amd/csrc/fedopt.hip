// Federated optimisation for clients that differ: what the server does with the aggregated update, and
// what a client's local steps are pulled towards.
//
//   nvq_fed_server_opt   FedOpt: D = sum_k c_k (x_k - base) as a pseudo-gradient for server momentum, Adagrad, Adam or Yogi;
//                        out = base + lr * step(D, m, v) (+ Gaussian noise), m and v stepped in place.  One launch.
//   nvq_fed_prox_grad    FedProx: grad += mu * (theta - anchor).  One launch.
//
// The sweep is fed_aggregate_kernel's (federated.hip): no atomics, no workspace, a grid that depends on n only, whole quads per
// thread in the vector and in the scalar form alike, the n % 4 tail in block 0.  All arithmetic of an element is one double
// chain; out, m and v are each that chain rounded to fp32 once, so no stored value carries the rounding of another.
#include "fed.h"

namespace nvq {

// One element.  D: the aggregated update; mp, vp: the stored moments, widened.  Returns the step that fed_mix scales; m1 and v1
// are the new moments before rounding (v1 = vp for AVGM, which has none).
template <int RULE>
__device__ __forceinline__ double fed_opt_step(double D, double mp, double vp, double b1, double b2, double tau, double& m1,
                                               double& v1) {
    if (RULE == NVQ_FED_OPT_AVGM) {
        m1 = fma(b1, mp, D);
        v1 = vp;
        return m1;
    }
    m1 = fma(b1, mp, (1.0 - b1) * D);
    const double d2 = __dmul_rn(D, D);                 // rounded on its own: the sign below is that of vp - round(D^2)
    if (RULE == NVQ_FED_OPT_ADAGRAD) {
        v1 = vp + d2;
    } else if (RULE == NVQ_FED_OPT_ADAM) {
        v1 = fma(b2, vp, (1.0 - b2) * d2);
    } else {
        const double s = vp - d2;
        const double sign = s > 0.0 ? 1.0 : (s < 0.0 ? -1.0 : 0.0);
        v1 = vp - (1.0 - b2) * d2 * sign;
    }
    return m1 / (sqrt(v1) + tau);
}

// fed_delta_quad / fed_delta_tail (fed.h) over all K rows in index order, then the server step.  `out` may be `base`: a thread
// reads its quad of base before it writes that quad of out.
template <bool VEC, bool NOISE, int RULE>
__global__ __launch_bounds__(256) void fed_server_opt_kernel(const float* __restrict__ clients, long stride, int K,
                                                             const float* base, const double* __restrict__ weights,
                                                             const double* __restrict__ sq, float clip_norm, float server_lr,
                                                             float beta1, float beta2, float tau, float* __restrict__ m,
                                                             float* __restrict__ v, float noise_std, long seed, long offset,
                                                             long n, float* out) {
    constexpr bool ADAPTIVE = RULE != NVQ_FED_OPT_AVGM;
    __shared__ double coef[64];
    fed_coefficients(coef, weights, sq, clip_norm, K);
    const auto row = [](int i) { return i; };
    const double lr = (double)server_lr, b1 = (double)beta1, b2 = (double)beta2, tu = (double)tau;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 b = ldq<VEC>(base + 4 * q);
        const float4 mp = ldq<VEC>(m + 4 * q);
        const float4 vp = ADAPTIVE ? ldq<VEC>(v + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        const double4 D = fed_delta_quad<VEC>(clients, stride, q, b, coef, row, 0, K);
        double4 m1, v1;
        const double sx = fed_opt_step<RULE>(D.x, (double)mp.x, (double)vp.x, b1, b2, tu, m1.x, v1.x);
        const double sy = fed_opt_step<RULE>(D.y, (double)mp.y, (double)vp.y, b1, b2, tu, m1.y, v1.y);
        const double sz = fed_opt_step<RULE>(D.z, (double)mp.z, (double)vp.z, b1, b2, tu, m1.z, v1.z);
        const double sw = fed_opt_step<RULE>(D.w, (double)mp.w, (double)vp.w, b1, b2, tu, m1.w, v1.w);
        float4 o = make_float4(fed_mix(sx, b.x, lr), fed_mix(sy, b.y, lr), fed_mix(sz, b.z, lr), fed_mix(sw, b.w, lr));
        fed_noise<NOISE>(o, noise_std, q, seed, offset);
        stq<VEC>(out + 4 * q, o);
        stq<VEC>(m + 4 * q, make_float4((float)m1.x, (float)m1.y, (float)m1.z, (float)m1.w));
        if (ADAPTIVE) stq<VEC>(v + 4 * q, make_float4((float)v1.x, (float)v1.y, (float)v1.z, (float)v1.w));
    }
    const long t = 4 * nq + threadIdx.x;
    if (flat_tail(n, t)) {
        const float b = base[t];
        const double D = fed_delta_tail(clients, stride, t, b, coef, row, 0, K);
        double m1, v1;
        const double s = fed_opt_step<RULE>(D, (double)m[t], ADAPTIVE ? (double)v[t] : 0.0, b1, b2, tu, m1, v1);
        float o = fed_mix(s, b, lr);
        fed_noise_tail<NOISE>(o, noise_std, nq, seed, offset);
        out[t] = o;
        m[t] = (float)m1;
        if (ADAPTIVE) v[t] = (float)v1;
    }
}

// grad += mu * (theta - anchor): the difference, the product and the sum in double (one fma), rounded to fp32 once
__device__ __forceinline__ float prox_one(float g, float th, float an, double mu) {
    return (float)fma(mu, (double)th - (double)an, (double)g);
}

template <bool VEC>
__global__ __launch_bounds__(256) void fed_prox_grad_kernel(float* __restrict__ grad, const float* __restrict__ theta,
                                                            const float* __restrict__ anchor, long n, float mu_) {
    const double mu = (double)mu_;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 g = ldq<VEC>(grad + 4 * q), th = ldq<VEC>(theta + 4 * q), an = ldq<VEC>(anchor + 4 * q);
        stq<VEC>(grad + 4 * q, make_float4(prox_one(g.x, th.x, an.x, mu), prox_one(g.y, th.y, an.y, mu),
                                           prox_one(g.z, th.z, an.z, mu), prox_one(g.w, th.w, an.w, mu)));
    }
    const long t = 4 * nq + threadIdx.x;
    if (flat_tail(n, t)) grad[t] = prox_one(grad[t], theta[t], anchor[t], mu);
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_fed_server_opt(const float* clients, long stride, int K, const float* base, const double* weights, const double* sq,
                       float clip_norm, int rule, float server_lr, float beta1, float beta2, float tau, float* m, float* v,
                       float noise_std, long seed, long offset, long n, float* out, void* stream) {
    int rc = fed_check("fed_server_opt", clients, stride, K, n, seed, offset, noise_std);
    if (rc) return rc;
    NVQ_REQUIRE(rule >= NVQ_FED_OPT_AVGM && rule <= NVQ_FED_OPT_YOGI, "fed_server_opt: rule %d outside 0 .. 3", rule);
    const bool adaptive = rule != NVQ_FED_OPT_AVGM;
    NVQ_REQUIRE(base != nullptr && weights != nullptr && out != nullptr, "fed_server_opt: base / weights / out");
    NVQ_REQUIRE(m != nullptr && (v != nullptr || !adaptive), "fed_server_opt: m, and v with an adaptive rule");
    NVQ_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "fed_server_opt: 0 <= beta < 1");
    NVQ_REQUIRE(!adaptive || tau > 0.f, "fed_server_opt: tau > 0 with an adaptive rule");
    NVQ_REQUIRE(sq == nullptr || clip_norm >= 0.f, "fed_server_opt: clip_norm");
    NVQ_REQUIRE(aligned8(weights) && aligned8(sq), "fed_server_opt: weights and sq must be 8-byte aligned");
    NVQ_REQUIRE(aligned4(m) && aligned4(v), "fed_server_opt: m / v alignment");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = fed_vec(clients, stride, base, out) && aligned16(m) && aligned16(v);
    const dim3 grid(flat_blocks(n)), block(256);
    rc = with_consts("fed_server_opt", [&](auto V, auto N, auto R) {
        hipLaunchKernelGGL((fed_server_opt_kernel<V(), N(), R()>), grid, block, 0, s, clients, stride, K, base, weights, sq,
                           clip_norm, server_lr, beta1, beta2, tau, m, v, noise_std, seed, offset, n, out);
    }, vec, noise_std != 0.f, one_of<NVQ_FED_OPT_AVGM, NVQ_FED_OPT_ADAGRAD, NVQ_FED_OPT_ADAM, NVQ_FED_OPT_YOGI>(rule));
    if (rc) return rc;
    return check_launch("fed_server_opt");
}

int nvq_fed_prox_grad(float* grad, const float* theta, const float* anchor, long n, float mu, void* stream) {
    NVQ_REQUIRE(grad != nullptr && theta != nullptr && anchor != nullptr && n >= 0, "fed_prox_grad: grad / theta / anchor / n");
    NVQ_REQUIRE(mu >= 0.f, "fed_prox_grad: mu");
    NVQ_REQUIRE(aligned4(grad) && aligned4(theta) && aligned4(anchor), "fed_prox_grad: alignment");
    if (mu == 0.f) return NVQ_OK;                      // nothing to add: grad keeps its bits, a -0.0 included
    const bool vec = aligned16(grad) && aligned16(theta) && aligned16(anchor);
    with_bools([&](auto V) {
        hipLaunchKernelGGL(fed_prox_grad_kernel<V()>, dim3(flat_blocks(n)), dim3(256), 0, (hipStream_t)stream, grad, theta,
                           anchor, n, mu);
    }, vec);
    return check_launch("fed_prox_grad");
}

}  // extern "C"
