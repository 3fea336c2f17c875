// Adam / AdamW on flat fp32 buffers: the update, optional global-norm clipping of the gradient and an optional exponential
// moving average of the weights in one pass over theta, grad, exp_avg, exp_avg_sq (and ema) - DESIGN.md section 20.
//
// Shaped like bucket_ops.hip: the grid depends on n only, every thread owns whole quads (4 consecutive floats) in both the
// float4 and the scalar form, the n % 4 last floats go to threads 0..2 of block 0.  Every fma is spelled out and contraction is
// off in the element function, so the compiler cannot contract the two forms differently: an element's result depends on its
// inputs only, never on the alignment of the pointers or on its position.  No atomics, no LDS.
#include "flat.h"

#include <math.h>

namespace nvq {

struct AdamArgs {
    float neg_step;      // -(lr / bias1)
    float theta_scale;   // decoupled: 1 - lr * weight_decay
    float l2;            // not decoupled: weight_decay
    float omb1;          // 1 - beta1
    float beta2, omb2;   // beta2, 1 - beta2
    float bias2_sqrt;    // sqrt(1 - beta2^t)
    float eps;
    float ome;           // 1 - ema_decay
    float max_norm;
    int decoupled;
};

struct AdamOut {
    float theta, m, v, ema;
};

// torch.optim.Adam / AdamW (amsgrad = False, maximize = False), single-tensor form, one element
template <bool HAS_EMA>
__device__ __forceinline__ AdamOut adam_element(float theta, float g, float m, float v, float ema, const AdamArgs& a, bool clip,
                                                float cf) {
    // plain operators below are single roundings: no contraction into fma other than the ones spelled out
#pragma clang fp contract(off)
    if (clip) g = g * cf;
    if (a.decoupled) theta = theta * a.theta_scale;
    else g = fmaf(a.l2, theta, g);
    m = fmaf(g - m, a.omb1, m);
    const float v_old = a.beta2 * v;
    v = fmaf(a.omb2 * g, g, v_old);
    const float denom = sqrtf(v) / a.bias2_sqrt + a.eps;      // correctly rounded sqrt and division (the hipcc default)
    theta = fmaf(a.neg_step, m / denom, theta);
    if (HAS_EMA) ema = fmaf(theta - ema, a.ome, ema);
    AdamOut o;
    o.theta = theta; o.m = m; o.v = v; o.ema = ema;
    return o;
}

#define NVQ_ADAM_LANE(c)                                                                  \
    do {                                                                                  \
        const AdamOut o = adam_element<HAS_EMA>(t.c, g.c, m.c, v.c, e.c, a, clip, cf);     \
        t.c = o.theta; m.c = o.m; v.c = o.v; e.c = o.ema;                                  \
    } while (0)

template <bool VEC, bool HAS_EMA>
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ theta, const float* __restrict__ grad,
                                                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                        float* __restrict__ ema, long n, AdamArgs a,
                                                        const double* __restrict__ acc) {
    // the decision of nvq_bucket_clip: scale only when coef < 1 (a NaN compares false)
    bool clip = false;
    float cf = 1.f;
    if (acc != nullptr) {
        const double coef = (double)a.max_norm / (sqrt(acc[2]) + 1e-6);
        clip = coef < 1.0;
        cf = (float)coef;
    }
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        float4 t = ldq<VEC>(theta + 4 * q);
        const float4 g = ldq<VEC>(grad + 4 * q);
        float4 m = ldq<VEC>(exp_avg + 4 * q);
        float4 v = ldq<VEC>(exp_avg_sq + 4 * q);
        float4 e = HAS_EMA ? ldq<VEC>(ema + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        NVQ_ADAM_LANE(x);
        NVQ_ADAM_LANE(y);
        NVQ_ADAM_LANE(z);
        NVQ_ADAM_LANE(w);
        stq<VEC>(theta + 4 * q, t);
        stq<VEC>(exp_avg + 4 * q, m);
        stq<VEC>(exp_avg_sq + 4 * q, v);
        if (HAS_EMA) stq<VEC>(ema + 4 * q, e);
    }
    const long i = 4 * nq + threadIdx.x;              // the n % 4 last floats: threads 0..2 of block 0
    if (blockIdx.x == 0 && threadIdx.x < 3 && i < n) {
        const AdamOut o = adam_element<HAS_EMA>(theta[i], grad[i], exp_avg[i], exp_avg_sq[i], HAS_EMA ? ema[i] : 0.f, a, clip, cf);
        theta[i] = o.theta;
        exp_avg[i] = o.m;
        exp_avg_sq[i] = o.v;
        if (HAS_EMA) ema[i] = o.ema;
    }
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_adam_step(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, long n, float lr, float beta1,
                  float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay, int decoupled,
                  float bias1, float bias2_sqrt, float ema_decay, const double* acc, float max_norm, void* stream) {
    NVQ_REQUIRE(n >= 0, "adam_step: n = %ld", n);
    if (n == 0) return NVQ_OK;
    NVQ_REQUIRE(theta != nullptr && grad != nullptr && exp_avg != nullptr && exp_avg_sq != nullptr,
                "adam_step: theta / grad / exp_avg / exp_avg_sq must not be NULL");
    NVQ_REQUIRE(aligned4(theta) && aligned4(grad) && aligned4(exp_avg) && aligned4(exp_avg_sq) && aligned4(ema),
                "adam_step: pointers must be 4-byte aligned");
    NVQ_REQUIRE(aligned8(acc), "adam_step: acc must be 8-byte aligned");
    NVQ_REQUIRE(bias1 > 0.f && bias2_sqrt > 0.f, "adam_step: bias1 = %g, bias2_sqrt = %g (step count < 1?)", (double)bias1,
                (double)bias2_sqrt);
    NVQ_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam_step: betas = (%g, %g)", (double)beta1,
                (double)beta2);
    AdamArgs a;
    a.neg_step = -(float)((double)lr / (double)bias1);
    a.theta_scale = (float)(1.0 - (double)lr * (double)weight_decay);
    a.l2 = weight_decay;
    a.omb1 = one_minus_beta1;
    a.beta2 = beta2;
    a.omb2 = one_minus_beta2;
    a.bias2_sqrt = bias2_sqrt;
    a.eps = eps;
    a.ome = (float)(1.0 - (double)ema_decay);
    a.max_norm = max_norm;
    a.decoupled = decoupled != 0;
    const bool vec = aligned16(theta) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) &&
                     (ema == nullptr || aligned16(ema));
    const dim3 grid(flat_blocks(n)), block(256);
    hipStream_t s = (hipStream_t)stream;
    with_bools([&](auto V, auto E) {
        hipLaunchKernelGGL((adam_step_kernel<V(), E()>), grid, block, 0, s, theta, grad, exp_avg, exp_avg_sq, ema, n, a, acc);
    }, vec, ema != nullptr);
    return check_launch("adam_step");
}

}  // extern "C"
