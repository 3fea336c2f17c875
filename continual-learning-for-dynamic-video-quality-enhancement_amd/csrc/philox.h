// Philox4x32-10 and the four standard normals of one quad (include/nvq.h, "Noise"), shared by the kernels that add Gaussian
// noise to a flat buffer (federated.hip, cluster.hip): a function of (seed, offset, quad index) alone.
#pragma once
#include "common.h"

namespace nvq {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned r[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// u = (m + 0.5) 2^-24 for the 24-bit m.  m + 0.5 is exact in fp32 only below 2^23; above, 1 - u = (2^24 - m - 0.5) 2^-24 is,
// so ln u = log1p(-(1 - u)) and the angle 2 pi u = -2 pi (1 - u) (mod 2 pi) are formed from the exact complement.
__device__ __forceinline__ float philox_neg2ln(unsigned w) {
    const unsigned m = w >> 8;
    if (m < 0x800000u) return -2.0f * logf(((float)m + 0.5f) * 0x1p-24f);
    return -2.0f * log1pf(-(((float)(0x1000000u - m) - 0.5f) * 0x1p-24f));
}
__device__ __forceinline__ float philox_turns(unsigned w) {          // 2 u in (-1, 1], for sincospif
    const unsigned m = w >> 8;
    if (m < 0x800000u) return ((float)m + 0.5f) * 0x1p-23f;
    return -(((float)(0x1000000u - m) - 0.5f) * 0x1p-23f);
}

__device__ __forceinline__ float4 quad_normals(long q, long seed, long offset) {
    unsigned r[4];
    philox4x32_10((unsigned)q, (unsigned)((unsigned long)q >> 32), (unsigned)offset, (unsigned)((unsigned long)offset >> 32),
                  (unsigned)seed, (unsigned)((unsigned long)seed >> 32), r);
    float s0, c0, s1, c1;
    sincospif(philox_turns(r[1]), &s0, &c0);
    sincospif(philox_turns(r[3]), &s1, &c1);
    const float m0 = sqrtf(philox_neg2ln(r[0])), m1 = sqrtf(philox_neg2ln(r[2]));
    return make_float4(m0 * c0, m0 * s0, m1 * c1, m1 * s1);
}

}  // namespace nvq
