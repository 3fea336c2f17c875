// Distillation losses on fp32 tensors, the gradient with respect to the student only.
//
// distill: d = mean (s - t)^2 and m = mean (s - y)^2 of the student output s against the teacher output t and the target y
// in ONE pass over the three tensors, out = wt d + wy m; the backward writes ds = go (2 / per) (wt (s - t) + wy (s - y)) once.
// The pixel_loss pattern of quality.hip with two sums: grid (nbs, groups), fp32 block partials in the workspace, a final
// kernel per group that adds them in double in a fixed order.
//
// cosine: 1 - cos(s_p, t_p) over the channels of every position p of two NCHW feature tensors, averaged over the positions.
// A thread owns one position (four adjacent ones as a float4 when hw % 4 == 0) and walks the channels with stride hw, so the
// loads of a wave are contiguous in every channel.  The backward recomputes the three moments (sum s^2, sum t^2, sum s t) in
// a first sweep over the channels and writes ds in a second one: nothing is saved besides the two inputs.
//
// HBM-bound VALU kernels, no LDS beyond the block reduction, no float atomics: two identical calls give the same bits.
#include "flat.h"

namespace nvq {

namespace {

// ------------------------------------------------------------------------------------------------------------ distill

__device__ __forceinline__ float sq(float v) { return v * v; }

// grid (nbs, G): part[(g * nbs + k) * 2 + {0, 1}] = block k's share of sum (s - t)^2 and of sum (s - y)^2 over group g
template <bool VEC, bool HAS_Y>
__global__ __launch_bounds__(256) void distill_partial_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                              const float* __restrict__ y, long per, float* __restrict__ part) {
    __shared__ float scratch[4];
    const long base = (long)blockIdx.y * per;
    const float* ss = s + base;
    const float* ts = t + base;
    const float* ys = HAS_Y ? y + base : nullptr;
    float d = 0.f, m = 0.f;
    if (VEC) {
        const long n4 = per >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const float4 u = ld4(ss + 4 * i), v = ld4(ts + 4 * i);
            d += (sq(u.x - v.x) + sq(u.y - v.y)) + (sq(u.z - v.z) + sq(u.w - v.w));
            if (HAS_Y) {
                const float4 w = ld4(ys + 4 * i);
                m += (sq(u.x - w.x) + sq(u.y - w.y)) + (sq(u.z - w.z) + sq(u.w - w.w));
            }
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
            const float u = ss[i];
            d += sq(u - ts[i]);
            if (HAS_Y) m += sq(u - ys[i]);
        }
    }
    d = block_sum_256(d, scratch);
    if (HAS_Y) m = block_sum_256(m, scratch);
    if (threadIdx.x == 0) {
        float* p = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        p[0] = d;
        p[1] = m;
    }
}

// grid (G): out[g] = wt d + wy m, out[G + g] = d, out[2 G + g] = m; the partials are added in double in a fixed order
__global__ __launch_bounds__(256) void distill_final_kernel(const float* __restrict__ part, int nblk, double inv_per, float wt,
                                                            float wy, float* __restrict__ out) {
    __shared__ double scratch[256];
    const float* p = part + (long)blockIdx.x * nblk * 2;
    double d = 0.0, m = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) {
        d += (double)p[2 * k];
        m += (double)p[2 * k + 1];
    }
    d = block_tree_sum_256(d, scratch);
    m = block_tree_sum_256(m, scratch);
    if (threadIdx.x == 0) {
        d *= inv_per;
        m *= inv_per;
        const int G = gridDim.x;
        out[blockIdx.x] = (float)((double)wt * d + (double)wy * m);
        out[G + blockIdx.x] = (float)d;
        out[2 * G + blockIdx.x] = (float)m;
    }
}

// ds = go[g] (2 / per) (wt (s - t) + wy (s - y))
template <bool VEC, bool HAS_Y>
__global__ __launch_bounds__(256) void distill_backward_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                               const float* __restrict__ y, long per, float wt, float wy,
                                                               const float* __restrict__ go, float two_inv_per,
                                                               float* __restrict__ ds) {
    const long base = (long)blockIdx.y * per;
    const float* ss = s + base;
    const float* ts = t + base;
    const float* ys = HAS_Y ? y + base : nullptr;
    float* out = ds + base;
    const float sc = two_inv_per * (go ? go[blockIdx.y] : 1.f);
    const float ct = sc * wt, cy = sc * wy;
    if (VEC) {
        const long n4 = per >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const float4 u = ld4(ss + 4 * i), v = ld4(ts + 4 * i);
            float4 r = make_float4(ct * (u.x - v.x), ct * (u.y - v.y), ct * (u.z - v.z), ct * (u.w - v.w));
            if (HAS_Y) {
                const float4 w = ld4(ys + 4 * i);
                r = make_float4(fmaf(cy, u.x - w.x, r.x), fmaf(cy, u.y - w.y, r.y), fmaf(cy, u.z - w.z, r.z),
                                fmaf(cy, u.w - w.w, r.w));
            }
            st4(out + 4 * i, r);
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
            const float u = ss[i];
            float r = ct * (u - ts[i]);
            if (HAS_Y) r = fmaf(cy, u - ys[i], r);
            out[i] = r;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- cosine

// V positions of one thread: float (V = 1) or float4 (V = 4)
template <int V> struct Lanes;
template <> struct Lanes<1> {
    float v[1];
    __device__ __forceinline__ static Lanes load(const float* p) { return {{*p}}; }
    __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <> struct Lanes<4> {
    float v[4];
    __device__ __forceinline__ static Lanes load(const float* p) {
        const float4 u = ld4(p);
        return {{u.x, u.y, u.z, u.w}};
    }
    __device__ __forceinline__ void store(float* p) const { st4(p, make_float4(v[0], v[1], v[2], v[3])); }
};

// a = sum_c s^2, b = sum_c t^2, ab = sum_c s t of V positions; sp, tp point at channel 0 of the first one
template <int V>
__device__ __forceinline__ void cosine_moments(const float* __restrict__ sp, const float* __restrict__ tp, int C, long hw,
                                               float (&a)[V], float (&b)[V], float (&ab)[V]) {
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = b[j] = ab[j] = 0.f;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        const Lanes<V> u = Lanes<V>::load(sp + c * hw), w = Lanes<V>::load(tp + c * hw);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            a[j] = fmaf(u.v[j], u.v[j], a[j]);
            b[j] = fmaf(w.v[j], w.v[j], b[j]);
            ab[j] = fmaf(u.v[j], w.v[j], ab[j]);
        }
    }
}

// grid (nbx, B): part[b * nbx + k] = block k's share of sum_p (1 - cos_p) over sample b
template <int V>
__global__ __launch_bounds__(256) void cosine_partial_kernel(const float* __restrict__ s, const float* __restrict__ t, int C,
                                                             long hw, float eps, float* __restrict__ part) {
    __shared__ float scratch[4];
    const long base = (long)blockIdx.y * C * hw;
    const long items = hw / V;
    float sum = 0.f;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        float a[V], b[V], ab[V];
        cosine_moments<V>(s + base + i * V, t + base + i * V, C, hw, a, b, ab);
#pragma unroll
        for (int j = 0; j < V; ++j) sum += 1.f - ab[j] / (fmaxf(sqrtf(a[j]), eps) * fmaxf(sqrtf(b[j]), eps));
    }
    sum = block_sum_256(sum, scratch);
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// ds_c = -(go / N) (t_c - [sqrt(a) > eps] (ab / a) s_c) / (ns nt): with r = ab / a the bracket is one fma per element, and for
// parallel s and t (C = 1 always) it cancels to a few ulp of t_c
template <int V>
__global__ __launch_bounds__(256) void cosine_backward_kernel(const float* __restrict__ s, const float* __restrict__ t, int C,
                                                              long hw, float eps, const float* __restrict__ go,
                                                              int go_per_sample, float inv_n, float* __restrict__ ds) {
    const long base = (long)blockIdx.y * C * hw;
    const long items = hw / V;
    const float sc = -inv_n * (go ? go[go_per_sample ? blockIdx.y : 0] : 1.f);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        const float* sp = s + base + i * V;
        const float* tp = t + base + i * V;
        float* dp = ds + base + i * V;
        float a[V], b[V], ab[V], k[V], r[V];
        cosine_moments<V>(sp, tp, C, hw, a, b, ab);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float ns = sqrtf(a[j]);
            k[j] = sc / (fmaxf(ns, eps) * fmaxf(sqrtf(b[j]), eps));
            r[j] = ns > eps ? ab[j] / a[j] : 0.f;
        }
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const Lanes<V> u = Lanes<V>::load(sp + c * hw), w = Lanes<V>::load(tp + c * hw);
            Lanes<V> d;
#pragma unroll
            for (int j = 0; j < V; ++j) d.v[j] = k[j] * fmaf(-r[j], u.v[j], w.v[j]);
            d.store(dp + c * hw);
        }
    }
}

// blocks per sample of the cosine kernels: one item (V positions) per thread, capped (the rest by the grid-stride loop)
int cosine_blocks(long hw, int V) {
    const int nb = ceil_div(hw / V, 256L);
    return nb > 1024 ? 1024 : nb;
}

}  // namespace

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_distill_forward(const float* s, const float* t, const float* y, int groups, long per, float wt, float wy, float* out,
                        float* workspace, size_t workspace_bytes, void* stream) {
    NVQ_REQUIRE(groups > 0 && groups <= 65535 && per > 0 && s && t && out && aligned16(s) && aligned16(t) && aligned16(y),
                "distill_forward: 0 < groups <= 65535, per > 0, 16-byte aligned tensors");
    const int nbs = group_blocks(per, groups);
    if ((size_t)groups * nbs * 2 * sizeof(float) > workspace_bytes) { set_error("distill_forward: workspace"); return NVQ_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (per & 3) == 0;
    const dim3 grid(nbs, groups);
    with_bools([&](auto V, auto Y) {
        hipLaunchKernelGGL((distill_partial_kernel<V(), Y()>), grid, dim3(256), 0, st, s, t, y, per, workspace);
    }, vec, y != nullptr);
    int rc = check_launch("distill_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(distill_final_kernel, dim3(groups), dim3(256), 0, st, workspace, nbs, 1.0 / (double)per, wt, wy, out);
    return check_launch("distill_final");
}

int nvq_distill_backward(const float* s, const float* t, const float* y, int groups, long per, float wt, float wy,
                         const float* grad_out_dev, float* ds, void* stream) {
    NVQ_REQUIRE(groups > 0 && groups <= 65535 && per > 0 && s && t && ds && aligned16(s) && aligned16(t) && aligned16(y) &&
                    aligned16(ds),
                "distill_backward: 0 < groups <= 65535, per > 0, 16-byte aligned tensors");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (per & 3) == 0;
    const dim3 grid(group_blocks(per, groups), groups);
    with_bools([&](auto V, auto Y) {
        hipLaunchKernelGGL((distill_backward_kernel<V(), Y()>), grid, dim3(256), 0, st, s, t, y, per, wt, wy, grad_out_dev,
                           (float)(2.0 / (double)per), ds);
    }, vec, y != nullptr);
    return check_launch("distill_backward");
}

int nvq_cosine_distill_forward(const float* s, const float* t, int B, int C, int hw, float eps, int per_sample, float* out,
                               float* workspace, size_t workspace_bytes, void* stream) {
    NVQ_REQUIRE(B > 0 && B <= 65535 && C > 0 && hw > 0 && eps > 0.f && s && t && out && aligned16(s) && aligned16(t),
                "cosine_distill_forward: 0 < B <= 65535, C, hw > 0, eps > 0, 16-byte aligned tensors");
    const int V = (hw & 3) == 0 ? 4 : 1;
    const int nbx = cosine_blocks(hw, V);
    if ((size_t)B * nbx * sizeof(float) > workspace_bytes) { set_error("cosine_distill_forward: workspace"); return NVQ_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nbx, B);
    if (V == 4)
        hipLaunchKernelGGL(cosine_partial_kernel<4>, grid, dim3(256), 0, st, s, t, C, (long)hw, eps, workspace);
    else
        hipLaunchKernelGGL(cosine_partial_kernel<1>, grid, dim3(256), 0, st, s, t, C, (long)hw, eps, workspace);
    int rc = check_launch("cosine_distill_partial");
    if (rc) return rc;
    const int groups = per_sample ? B : 1;
    launch_group_final(workspace, per_sample ? nbx : B * nbx, groups, 1.0 / ((double)(per_sample ? 1 : B) * (double)hw), 0.0, out,
                       st);
    return check_launch("cosine_distill_final");
}

int nvq_cosine_distill_backward(const float* s, const float* t, int B, int C, int hw, float eps, const float* grad_out_dev,
                                int per_sample, float* ds, void* stream) {
    NVQ_REQUIRE(B > 0 && B <= 65535 && C > 0 && hw > 0 && eps > 0.f && s && t && ds && aligned16(s) && aligned16(t) &&
                    aligned16(ds),
                "cosine_distill_backward: 0 < B <= 65535, C, hw > 0, eps > 0, 16-byte aligned tensors");
    const int V = (hw & 3) == 0 ? 4 : 1;
    const dim3 grid(cosine_blocks(hw, V), B);
    const float inv_n = (float)(1.0 / ((double)(per_sample ? 1 : B) * (double)hw));
    hipStream_t st = (hipStream_t)stream;
    if (V == 4)
        hipLaunchKernelGGL(cosine_backward_kernel<4>, grid, dim3(256), 0, st, s, t, C, (long)hw, eps, grad_out_dev, per_sample,
                           inv_n, ds);
    else
        hipLaunchKernelGGL(cosine_backward_kernel<1>, grid, dim3(256), 0, st, s, t, C, (long)hw, eps, grad_out_dev, per_sample,
                           inv_n, ds);
    return check_launch("cosine_distill_backward");
}

}  // extern "C"
