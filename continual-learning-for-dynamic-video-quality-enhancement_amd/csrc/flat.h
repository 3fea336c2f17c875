// The flat-buffer rule, in one place.  A kernel that sweeps a flat fp32 buffer
//   - runs on a grid that depends on the sizes only (flat_blocks / group_blocks),
//   - gives every thread whole quads (4 consecutive floats) in the vector and in the scalar form alike (ldq / stq),
//   - adds in double in a fixed order (wave_sum, then one of the block sums below),
// so its results depend neither on the alignment of the pointers nor on the call: they are bit-reproducible.
// A new flat kernel includes this header instead of copying from a neighbour.
#pragma once
#include "common.h"

namespace nvq {

// one quad per thread and trip, at most 1024 blocks, at least 1: a function of n only
inline int flat_blocks(long n) {
    int nb = ceil_div(n, 256L * 4);
    if (nb > 1024) nb = 1024;
    return nb < 1 ? 1 : nb;
}

// blocks per group of the grouped elementwise passes (grid (nb, groups)): 16 elements per thread, capped
inline int group_blocks(long per, int groups) {
    int nb = ceil_div(per, 256L * 16);
    const int cap = groups == 1 ? 2048 : 1024;
    if (nb > cap) nb = cap;
    return nb < 1 ? 1 : nb;
}

template <bool VEC>
__device__ __forceinline__ float4 ldq(const float* p) {
    if (VEC) return ld4(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

template <bool VEC>
__device__ __forceinline__ void stq(float* p, float4 v) {
    if (VEC) {
        st4(p, v);
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

// The n % 4 last floats belong to threads 0 .. 2 of block 0: whether this thread owns tail element t = 4 * (n >> 2) + threadIdx.x.
__device__ __forceinline__ bool flat_tail(long n, long t) { return blockIdx.x == 0 && threadIdx.x < 3 && t < n; }

// Sum over the 64 lanes of a wave, the 32, 16, ..., 1 xor-shuffle tree; valid in every lane.
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sums of doubles over 256 threads: wave_sum, then the four wave sums left to right, ((w0 + w1) + w2) + w3.
// Valid in every thread.  scratch: >= 4 doubles of LDS per value.
template <class... D>
__device__ __forceinline__ void block_wave_sum_256(double* scratch, D&... v) {
    constexpr int N = sizeof...(D);
    ((v = wave_sum(v)), ...);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        int i = wave * N;
        ((scratch[i++] = v), ...);
    }
    __syncthreads();
    int i = 0;
    ((v = scratch[i] + scratch[N + i] + scratch[2 * N + i] + scratch[3 * N + i], ++i), ...);
}

// Block-wide sum of a double over 256 threads as a halving tree in LDS (thread t adds t + 128, then t + 64, ...): another
// order than block_wave_sum_256, kept by the second stages that were written with it.  Valid in thread 0.  scratch: 256 doubles.
__device__ __forceinline__ double block_tree_sum_256(double v, double* scratch) {
    __syncthreads();
    scratch[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) scratch[threadIdx.x] += scratch[threadIdx.x + o];
        __syncthreads();
    }
    return scratch[0];
}

// Second stages shared between translation units (reduce.hip).  Both only
// enqueue: the caller checks the launch under its own name.
// grid (groups): out[g] = bias + alpha * sum_k part[g * nblk + k], in double, block_tree_sum_256 order
void launch_group_final(const float* part, int nblk, int groups, double alpha, double bias, float* out, hipStream_t s);
// one thread: out[0] = alpha * sum_k part[k], in double in index order
void launch_serial_final(const float* part, int nblk, double alpha, float* out, hipStream_t s);

}  // namespace nvq
