// Second-stage kernels of the flat-buffer losses that more than one translation unit launches.  The build has no relocatable
// device code, so each lives here once behind a host launcher.  Every one adds the first stage's fp32 partials in double in a
// fixed order.  (launch_reduce_partials, the K-output second stage of the convolution paths, stays in conv_igemm.hip:
// tests/test_launch_forms_cpu.py mirrors its lane loop there.)
#include "flat.h"

namespace nvq {

// grid (G): out[g] = bias + alpha * sum_k part[g * nblk + k], in double in a fixed order
__global__ __launch_bounds__(256) void group_final_kernel(const float* __restrict__ part, int nblk, double alpha, double bias,
                                                          float* __restrict__ out) {
    __shared__ double scratch[256];
    const float* p = part + (long)blockIdx.x * nblk;
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) s += (double)p[k];
    s = block_tree_sum_256(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(bias + alpha * s);
}

// bias = 0.0 gives (float)(alpha * s) bit for bit: s is a sum started from +0.0 and alpha > 0, so alpha * s is never -0.0
void launch_group_final(const float* part, int nblk, int groups, double alpha, double bias, float* out, hipStream_t s) {
    hipLaunchKernelGGL(group_final_kernel, dim3(groups), dim3(256), 0, s, part, nblk, alpha, bias, out);
}

// A serial sum, not a tree: the results of nvq_mse_forward and nvq_ewc_penalty are defined by this order.
__global__ void serial_final_kernel(const float* __restrict__ part, int nblk, double alpha, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < nblk; ++k) s += (double)part[k];
        *out = (float)(alpha * s);
    }
}

void launch_serial_final(const float* part, int nblk, double alpha, float* out, hipStream_t s) {
    hipLaunchKernelGGL(serial_final_kernel, dim3(1), dim3(64), 0, s, part, nblk, alpha, out);
}

}  // namespace nvq
