// Gradient projection (A-GEM, Chaudhry et al. 2019) and global-norm clipping on flat fp32 gradient buckets: the inner
// products g.r, r.r, g.g in one pass, the decision and the coefficient on the device, then one axpy / scale.  No host
// read anywhere: the step's `if (g.r < 0)` is a uniform early return of the update kernel.
//
// Every thread owns whole quads (4 consecutive floats) in both the vector and the scalar form of a kernel, so the two
// forms add the same products in the same order: the sums do not depend on the alignment of the pointers, only on n.
#include "flat.h"

namespace nvq {

// acc slots (float64, device): g.r, r.r, g.g, projection coefficient c, number of projections so far
enum { ACC_GR = 0, ACC_RR = 1, ACC_GG = 2, ACC_C = 3, ACC_COUNT = 4 };

#define NVQ_MOMENT(gv, rv)                                 \
    do {                                                   \
        const double gd = (double)(gv), rd = (double)(rv); \
        gr += gd * rd;                                     \
        rr += rd * rd;                                     \
        gg += gd * gd;                                     \
    } while (0)

// part[blockIdx.x * 3 + {0,1,2}] = this block's share of g.r, r.r, g.g; exact products, double sums
template <bool VEC, bool HAS_R>
__global__ __launch_bounds__(256) void bucket_moments_kernel(const float* __restrict__ g, const float* __restrict__ r, long n,
                                                             double* __restrict__ part) {
    __shared__ double scratch[12];
    double gr = 0.0, rr = 0.0, gg = 0.0;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 a = ldq<VEC>(g + 4 * q);
        const float4 b = HAS_R ? ldq<VEC>(r + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        NVQ_MOMENT(a.x, b.x);
        NVQ_MOMENT(a.y, b.y);
        NVQ_MOMENT(a.z, b.z);
        NVQ_MOMENT(a.w, b.w);
    }
    const long t = 4 * nq + threadIdx.x;              // the n % 4 last floats: threads 0..2 of block 0
    if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) NVQ_MOMENT(g[t], HAS_R ? r[t] : 0.f);
    block_wave_sum_256(scratch, gr, rr, gg);
    if (threadIdx.x == 0) {
        part[blockIdx.x * 3 + 0] = gr;
        part[blockIdx.x * 3 + 1] = rr;
        part[blockIdx.x * 3 + 2] = gg;
    }
}

// One block: acc[0..2] (+)= sum over the blocks' partials in a fixed order; with `coefficient` the A-GEM decision:
// c = g.r / r.r when g.r < 0 and r.r > 0 (a NaN compares false), else 0; acc[4] counts the non-zero ones.
__global__ __launch_bounds__(256) void bucket_moments_final_kernel(const double* __restrict__ part, int nblk, int has_r,
                                                                   int accumulate, int coefficient, double* __restrict__ acc) {
    __shared__ double scratch[12];
    double gr = 0.0, rr = 0.0, gg = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) {
        gr += part[b * 3 + 0];
        rr += part[b * 3 + 1];
        gg += part[b * 3 + 2];
    }
    block_wave_sum_256(scratch, gr, rr, gg);
    if (threadIdx.x != 0) return;
    if (accumulate) {
        if (has_r) {
            gr += acc[ACC_GR];
            rr += acc[ACC_RR];
        }
        gg += acc[ACC_GG];
    }
    if (has_r || !accumulate) {
        acc[ACC_GR] = gr;
        acc[ACC_RR] = rr;
    } else {
        gr = acc[ACC_GR];
        rr = acc[ACC_RR];
    }
    acc[ACC_GG] = gg;
    if (coefficient) {
        const double c = (gr < 0.0 && rr > 0.0) ? gr / rr : 0.0;
        acc[ACC_C] = c;
        if (c != 0.0) acc[ACC_COUNT] += 1.0;
    }
}

// g -= c r with c = acc[3] read by every thread; c == 0 (no conflict) returns before g is touched
template <bool VEC>
__global__ __launch_bounds__(256) void bucket_project_kernel(float* __restrict__ g, const float* __restrict__ r, long n,
                                                             const double* __restrict__ acc) {
    const double c = acc[ACC_C];
    if (c == 0.0) return;
    const float mc = -(float)c;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        float4 a = ldq<VEC>(g + 4 * q);
        const float4 b = ldq<VEC>(r + 4 * q);
        a.x = fmaf(mc, b.x, a.x);
        a.y = fmaf(mc, b.y, a.y);
        a.z = fmaf(mc, b.z, a.z);
        a.w = fmaf(mc, b.w, a.w);
        stq<VEC>(g + 4 * q, a);
    }
    const long t = 4 * nq + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) g[t] = fmaf(mc, r[t], g[t]);
}

// torch.nn.utils.clip_grad_norm_ (2-norm): coef = max_norm / (norm + 1e-6); g *= coef only when coef < 1
template <bool VEC>
__global__ __launch_bounds__(256) void bucket_clip_kernel(float* __restrict__ g, long n, const double* __restrict__ acc,
                                                          float max_norm, float* __restrict__ norm_out) {
    const double norm = sqrt(acc[ACC_GG]);
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
    const double coef = (double)max_norm / (norm + 1e-6);
    if (!(coef < 1.0)) return;
    const float cf = (float)coef;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        float4 a = ldq<VEC>(g + 4 * q);
        a.x *= cf;
        a.y *= cf;
        a.z *= cf;
        a.w *= cf;
        stq<VEC>(g + 4 * q, a);
    }
    const long t = 4 * nq + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 3 && t < n) g[t] *= cf;
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_bucket_moments(const float* g, const float* r, long n, double* acc, int accumulate, int coefficient,
                       float* workspace, size_t workspace_bytes, void* stream) {
    NVQ_REQUIRE(g != nullptr && acc != nullptr && n >= 0, "bucket_moments: g / acc / n");
    NVQ_REQUIRE(aligned8(acc) && aligned8(workspace), "bucket_moments: acc and workspace must be 8-byte aligned");
    const int nb = flat_blocks(n);
    if (workspace == nullptr || (size_t)nb * 3 * sizeof(double) > workspace_bytes) {
        set_error("bucket_moments: workspace");
        return NVQ_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    const bool vec = aligned16(g) && (r == nullptr || aligned16(r));
    const dim3 grid(nb), block(256);
    with_bools([&](auto V, auto R) { hipLaunchKernelGGL((bucket_moments_kernel<V(), R()>), grid, block, 0, s, g, r, n, part); },
               vec, r != nullptr);
    int rc = check_launch("bucket_moments");
    if (rc) return rc;
    hipLaunchKernelGGL(bucket_moments_final_kernel, dim3(1), dim3(256), 0, s, part, nb, r != nullptr ? 1 : 0, accumulate,
                       coefficient, acc);
    return check_launch("bucket_moments_final");
}

int nvq_bucket_project(float* g, const float* r, long n, const double* acc, void* stream) {
    NVQ_REQUIRE(g != nullptr && r != nullptr && acc != nullptr && n >= 0, "bucket_project: g / r / acc / n");
    const dim3 grid(flat_blocks(n)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(g) && aligned16(r)) hipLaunchKernelGGL(bucket_project_kernel<true>, grid, block, 0, s, g, r, n, acc);
    else hipLaunchKernelGGL(bucket_project_kernel<false>, grid, block, 0, s, g, r, n, acc);
    return check_launch("bucket_project");
}

int nvq_bucket_clip(float* g, long n, const double* acc, float max_norm, float* norm_out, void* stream) {
    NVQ_REQUIRE(g != nullptr && acc != nullptr && n >= 0, "bucket_clip: g / acc / n");
    const dim3 grid(flat_blocks(n)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(g)) hipLaunchKernelGGL(bucket_clip_kernel<true>, grid, block, 0, s, g, n, acc, max_norm, norm_out);
    else hipLaunchKernelGGL(bucket_clip_kernel<false>, grid, block, 0, s, g, n, acc, max_norm, norm_out);
    return check_launch("bucket_clip");
}

}  // extern "C"
