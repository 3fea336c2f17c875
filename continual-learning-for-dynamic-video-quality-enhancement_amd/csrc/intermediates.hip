// SuperResolutionNet's return_intermediate tensors (reference nerve_cl/models/super_resolution.py:384-389) between the engine's
// NHWC channel slices and the fp32 NCHW tensors of the module boundary: the forward's gather (a widening copy, all 2T + 1
// tensors in one launch) and the backward's inject (their upstream gradients added into the gradient slices).
//
// Both move a tile of 64 pixels (linear within the image) x TC = min(C, 64) channels through LDS, so that each side moves
// 16-B pieces: 4 fp32 or 8 bf16 channels of a pixel on the NHWC side, 4 consecutive pixels of a channel on the NCHW side
// (scalar on that side when H*W % 4 != 0 or an NCHW base is not 16-B aligned: its rows then do not start on 16 B).
// LDS tile: fp32 [TC][64], element (c, p) at c*64 + (p ^ sw(c)), sw(c) = ((c >> 2) & 15) << 2 (an XOR of whole 16-B
// slots, so a pixel quad stays one aligned 16-B piece).  NCHW side: ds_read_b128 / ds_write_b128, a wave covers channels
// 4k .. 4k+3 (one sw value), each row a permutation of its 16 slots: conflict-free.  NHWC side: scalar accesses, lanes with
// the pixel piece fastest; banks (p ^ sw(c)) mod 32: at most 2-way (free for the gather's ds_write_b32, twice the cycles of
// the inject's ds_read_b32; neither is near the bound of these HBM-bound copies).
#include "common.h"

namespace nvq {

constexpr int IL_TP = 64;    // pixels per tile

struct GatherJobs { nvq_gather_job j[NVQ_LAYOUT_MAX_JOBS]; };
struct InjectJobs { nvq_inject_job j[NVQ_LAYOUT_MAX_JOBS]; };

__device__ __forceinline__ int il_idx(int c, int p) { return c * IL_TP + (p ^ (((c >> 2) & 15) << 2)); }

// tile (c, p) for the TC x 64 tile at channel c0, pixel p0 of image n of an NHWC slice -> LDS (fp32 values)
template <bool BF16>
__device__ __forceinline__ void il_nhwc_to_lds(float* tile, const void* base, int ld, int coff, int n, long HW, long p0, int c0,
                                               int TC) {
    constexpr int V = BF16 ? 8 : 4;
    const int pp = TC / V;                               // pieces per pixel
    for (int q = threadIdx.x; q < IL_TP * pp; q += 256) {
        const int piece = q % pp, p = q / pp;
        if (p0 + p >= HW) continue;
        const size_t e = ((size_t)n * HW + p0 + p) * ld + coff + c0 + piece * V;
        const int c = piece * V;
        if (BF16) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(base) + e);
#pragma unroll
            for (int k = 0; k < 8; ++k) tile[il_idx(c + k, p)] = (float)v[k];
        } else {
            const float4 v = ld4(reinterpret_cast<const float*>(base) + e);
            tile[il_idx(c + 0, p)] = v.x;
            tile[il_idx(c + 1, p)] = v.y;
            tile[il_idx(c + 2, p)] = v.z;
            tile[il_idx(c + 3, p)] = v.w;
        }
    }
}

// dst[n, c0 + c, p0 + p] = tile (c, p), for every pixel < HW
__device__ __forceinline__ void il_lds_to_nchw(const float* tile, float* dst, int C, int n, long HW, long p0, int c0, int TC,
                                               int vec) {
    for (int q = threadIdx.x; q < TC * (IL_TP / 4); q += 256) {
        const int p4 = q & 15, c = q >> 4;
        const long p = p0 + p4 * 4;
        if (p >= HW) continue;
        const float4 v = *reinterpret_cast<const float4*>(tile + il_idx(c, p4 * 4));
        float* row = dst + ((size_t)n * C + c0 + c) * HW + p;
        if (vec) {
            st4(row, v);                                  // HW % 4 == 0: the quad is whole
        } else {
            row[0] = v.x;
            if (p + 1 < HW) row[1] = v.y;
            if (p + 2 < HW) row[2] = v.z;
            if (p + 3 < HW) row[3] = v.w;
        }
    }
}

// tile (c, p) = src[n, c0 + c, p0 + p] (pixels >= HW: 0)
__device__ __forceinline__ void il_nchw_to_lds(float* tile, const float* src, int C, int n, long HW, long p0, int c0, int TC,
                                               int vec) {
    for (int q = threadIdx.x; q < TC * (IL_TP / 4); q += 256) {
        const int p4 = q & 15, c = q >> 4;
        const long p = p0 + p4 * 4;
        const float* row = src + ((size_t)n * C + c0 + c) * HW + p;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec) {
            if (p < HW) v = ld4(row);
        } else {
            if (p < HW) v.x = row[0];
            if (p + 1 < HW) v.y = row[1];
            if (p + 2 < HW) v.z = row[2];
            if (p + 3 < HW) v.w = row[3];
        }
        *reinterpret_cast<float4*>(tile + il_idx(c, p4 * 4)) = v;
    }
}

// grid (pixel tiles, C / TC, njobs * N)
__global__ __launch_bounds__(256) void gather_nchw_kernel(GatherJobs jobs, int N, int C, long HW, int TC, int vec) {
    __shared__ float tile[64 * IL_TP];
    const nvq_gather_job& jb = jobs.j[blockIdx.z / N];
    const int n = blockIdx.z % N, c0 = blockIdx.y * TC;
    const long p0 = (long)blockIdx.x * IL_TP;
    if (jb.src_bf16)
        il_nhwc_to_lds<true>(tile, jb.src, jb.src_ld, jb.src_coff, n, HW, p0, c0, TC);
    else
        il_nhwc_to_lds<false>(tile, jb.src, jb.src_ld, jb.src_coff, n, HW, p0, c0, TC);
    __syncthreads();
    il_lds_to_nchw(tile, jb.dst, C, n, HW, p0, c0, TC, vec);
}

// The NHWC side of the inject kernel: a thread keeps the destination pieces it owns in registers (at most 4 fp32 or 2 bf16
// pieces of 16 B: 64 pixels x 64 channels / 256 threads), adds each staged source tile, and stores once.
template <bool BF16>
__device__ __forceinline__ void il_inject(float* tile, const nvq_inject_job& jb, int C, int n, long HW, long p0, int c0, int TC,
                                          int vec) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr int IT = IL_TP * 64 / V / 256;             // pieces per thread at TC = 64
    const int pp = TC / V;
    float acc[IT][V];
    size_t e[IT];
    bool live[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int q = threadIdx.x + 256 * i;
        const int piece = q % pp, p = q / pp;
        live[i] = q < IL_TP * pp && p0 + p < HW;
        e[i] = ((size_t)n * HW + p0 + p) * jb.dst_ld + jb.dst_coff + c0 + piece * V;
        if (live[i]) {
            if (BF16) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(jb.dst) + e[i]);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[i][k] = (float)v[k];
            } else {
                const float4 v = ld4(reinterpret_cast<const float*>(jb.dst) + e[i]);
                acc[i][0] = v.x; acc[i][1] = v.y; acc[i][2] = v.z; acc[i][3] = v.w;
            }
        }
    }
    for (int s = 0; s < NVQ_INJECT_MAX_SRC; ++s) {       // in the given order: ((dst + src0) + src1) + ...
        const float* src = jb.src[s];
        if (src == nullptr) continue;
        __syncthreads();                                  // the previous source's tile has been read
        il_nchw_to_lds(tile, src, C, n, HW, p0, c0, TC, vec);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int q = threadIdx.x + 256 * i;
            const int piece = q % pp, p = q / pp;
            if (live[i]) {
#pragma unroll
                for (int k = 0; k < V; ++k) acc[i][k] += tile[il_idx(piece * V + k, p)];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        if (!live[i]) continue;
        if (BF16) {
            bf16x8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (__bf16)acc[i][k];      // one RNE rounding of the fp32 sum
            *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(jb.dst) + e[i]) = v;
        } else {
            st4(reinterpret_cast<float*>(jb.dst) + e[i], make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
        }
    }
}

__global__ __launch_bounds__(256) void inject_nchw_kernel(InjectJobs jobs, int N, int C, long HW, int TC, int vec) {
    __shared__ float tile[64 * IL_TP];
    const nvq_inject_job& jb = jobs.j[blockIdx.z / N];
    const int n = blockIdx.z % N, c0 = blockIdx.y * TC;
    const long p0 = (long)blockIdx.x * IL_TP;
    if (jb.dst_bf16)
        il_inject<true>(tile, jb, C, n, HW, p0, c0, TC, vec);
    else
        il_inject<false>(tile, jb, C, n, HW, p0, c0, TC, vec);
}

static int il_check_slice(const void* base, int ld, int coff, int C, int bf16, const char* what) {
    const int v = bf16 ? 8 : 4;
    NVQ_REQUIRE(base != nullptr && aligned16(base) && ld % v == 0 && coff % v == 0 && coff >= 0 && coff + C <= ld,
                "%s: NHWC slice needs a 16-B aligned base, ld and coff multiples of %d and coff + C <= ld (ld %d coff %d C %d)",
                what, v, ld, coff, C);
    return NVQ_OK;
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_gather_nchw(const nvq_gather_job* jobs, int njobs, int N, int C, int H, int W, void* stream) {
    NVQ_REQUIRE(njobs > 0 && njobs <= NVQ_LAYOUT_MAX_JOBS && N > 0 && H > 0 && W > 0 && (long)N * njobs <= 65535,
                "gather_nchw: njobs %d N %d H %d W %d", njobs, N, H, W);
    NVQ_REQUIRE(C >= 16 && C <= 256 && (C & (C - 1)) == 0, "gather_nchw: C %d is not a power of two in [16, 256]", C);
    const long HW = (long)H * W;
    GatherJobs a;
    int vec = HW % 4 == 0;
    for (int i = 0; i < njobs; ++i) {
        const nvq_gather_job& j = jobs[i];
        const int rc = il_check_slice(j.src, j.src_ld, j.src_coff, C, j.src_bf16, "gather_nchw");
        if (rc != NVQ_OK) return rc;
        NVQ_REQUIRE(j.dst != nullptr, "gather_nchw: job %d has no destination", i);
        vec = vec && aligned16(j.dst);
        a.j[i] = j;
    }
    const int TC = C < 64 ? C : 64;
    hipLaunchKernelGGL(gather_nchw_kernel, dim3(ceil_div(HW, IL_TP), C / TC, N * njobs), dim3(256), 0, (hipStream_t)stream, a, N,
                       C, HW, TC, vec);
    return check_launch("gather_nchw");
}

int nvq_inject_nchw(const nvq_inject_job* jobs, int njobs, int N, int C, int H, int W, void* stream) {
    NVQ_REQUIRE(njobs > 0 && njobs <= NVQ_LAYOUT_MAX_JOBS && N > 0 && H > 0 && W > 0 && (long)N * njobs <= 65535,
                "inject_nchw: njobs %d N %d H %d W %d", njobs, N, H, W);
    NVQ_REQUIRE(C >= 16 && C <= 256 && (C & (C - 1)) == 0, "inject_nchw: C %d is not a power of two in [16, 256]", C);
    const long HW = (long)H * W;
    InjectJobs a;
    int vec = HW % 4 == 0;
    for (int i = 0; i < njobs; ++i) {
        const nvq_inject_job& j = jobs[i];
        const int rc = il_check_slice(j.dst, j.dst_ld, j.dst_coff, C, j.dst_bf16, "inject_nchw");
        if (rc != NVQ_OK) return rc;
        for (int s = 0; s < NVQ_INJECT_MAX_SRC; ++s) vec = vec && (j.src[s] == nullptr || aligned16(j.src[s]));
        a.j[i] = j;
    }
    const int TC = C < 64 ? C : 64;
    hipLaunchKernelGGL(inject_nchw_kernel, dim3(ceil_div(HW, IL_TP), C / TC, N * njobs), dim3(256), 0, (hipStream_t)stream, a, N,
                       C, HW, TC, vec);
    return check_launch("inject_nchw");
}

size_t nvq_sizeof_gather_job(void) { return sizeof(nvq_gather_job); }
size_t nvq_sizeof_inject_job(void) { return sizeof(nvq_inject_job); }

}  // extern "C"
