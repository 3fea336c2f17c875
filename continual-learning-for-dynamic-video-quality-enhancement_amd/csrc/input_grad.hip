// Input gradients of the SR networks: the head conv's input gradient (nvq_head_dgrad) and the adjoint of the bicubic skip
// (nvq_bicubic_adjoint); of FrameRecoveryNet: the first temporal conv's input gradient in the time-in-channels layout
// (nvq_head_dgrad_tc), the 7x7 stride-2 stem's input gradient (nvq_stem7_dgrad) and the blend's frame / mask gradient
// (nvq_mask_blend_backward_ex).  All are gather kernels: every output element is owned by one thread and summed in a fixed
// order (no atomics), so the inputs' gradient is bit-identical from run to run.
#include "common.h"

namespace nvq {

// ------------------------------------------------------------------ head conv input gradient
// dframes[b, t, ci, y, x] = sum_{f, ky, kx} g[slot*B + b, y + 1 - ky, x + 1 - kx, f] * W[f, ci, ky, kx]
// g = dout (pre-masked, act == NULL) or (dout + dout2) where act > 0.
// One workgroup: a DG_TH x DG_TW tile of one image, one thread per output pixel.  g is staged chunk by chunk (DG_CC
// channels) with its one-pixel halo in LDS, channel-major, so that the lanes of a wave read consecutive words; the weights
// of the chunk sit in LDS too and are read as broadcasts.
constexpr int DG_TW = 32, DG_TH = 8;
constexpr int DG_HW = DG_TW + 2, DG_HH = DG_TH + 2, DG_HP = DG_HW * DG_HH;   // halo tile: 34 x 10 = 340 pixels
constexpr int DG_CC = 16;                                                     // channels per LDS chunk

// slot s: frame t[s] of dframes, read from images s * slot_images + b of g at channel offset c[s]
struct DgSlots { int t[NVQ_MAX_T]; int c[NVQ_MAX_T]; };

// 8 channels at element `idx` (16-B aligned in either storage type) as fp32
__device__ __forceinline__ void ld8(const float* base, size_t idx, int is_bf16, float v[8]) {
    if (is_bf16) {
        const bf16x8 q = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(base) + idx);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (float)q[k];
    } else {
        const float4 a = ld4(base + idx), b = ld4(base + idx + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}

template <int CIN>
__global__ __launch_bounds__(256) void head_dgrad_kernel(const float* __restrict__ dout, int dout_ld, int dout_bf16,
                                                         const float* __restrict__ dout2, int dout2_ld,
                                                         const float* __restrict__ act, int act_ld, int act_bf16,
                                                         const float* __restrict__ weight, int F, int B, int T, int H,
                                                         int W, DgSlots sm, int slot_images, float* __restrict__ dframes,
                                                         int accumulate, int tilesX) {
    __shared__ float gs[DG_CC][DG_HP];
    __shared__ float ws[DG_CC][CIN][9];
    const int tid = threadIdx.x;
    const int img = blockIdx.y;                  // slot * B + b
    const int tx0 = (blockIdx.x % tilesX) * DG_TW, ty0 = (blockIdx.x / tilesX) * DG_TH;
    const int slot = img / B, b = img - slot * B;
    const int ty = tid / DG_TW, tx = tid - ty * DG_TW;
    float acc[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
    const size_t pix0 = ((size_t)slot * slot_images + b) * H * W;
    const int cofs = sm.c[slot];
    for (int f0 = 0; f0 < F; f0 += DG_CC) {
        __syncthreads();                         // the previous chunk's readers are done
        // stage: unit = (halo pixel, 8-channel half of the chunk); 680 units over 256 threads
        for (int u = tid; u < DG_HP * 2; u += 256) {
            const int p = u >> 1, h8 = (u & 1) * 8;
            const int hy = p / DG_HW, hx = p - hy * DG_HW;
            const int y = ty0 - 1 + hy, x = tx0 - 1 + hx;
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = 0.f;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const size_t q = pix0 + (size_t)y * W + x;
                ld8(dout, q * dout_ld + cofs + f0 + h8, dout_bf16, v);
                if (act) {
                    float a[8];
                    ld8(act, q * act_ld + f0 + h8, act_bf16, a);
                    if (dout2) {
                        float d2[8];
                        ld8(dout2, q * dout2_ld + f0 + h8, 0, d2);
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] += d2[k];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = a[k] > 0.f ? v[k] : 0.f;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) gs[h8 + k][p] = v[k];
        }
        for (int e = tid; e < DG_CC * CIN * 9; e += 256) {
            const int f = e / (CIN * 9), r = e - f * (CIN * 9);
            ws[f][r / 9][r % 9] = weight[(size_t)(f0 + f) * CIN * 9 + r];
        }
        __syncthreads();
#pragma unroll 4
        for (int f = 0; f < DG_CC; ++f) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float gv = gs[f][(ty + 2 - ky) * DG_HW + tx + 2 - kx];
#pragma unroll
                    for (int c = 0; c < CIN; ++c) acc[c] = fmaf(gv, ws[f][c][ky * 3 + kx], acc[c]);
                }
        }
    }
    const int y = ty0 + ty, x = tx0 + tx;
    if (y < H && x < W) {
        const int t = sm.t[slot];
#pragma unroll
        for (int c = 0; c < CIN; ++c) {
            float* o = dframes + (((size_t)(b * T + t) * CIN + c) * H + y) * W + x;
            *o = accumulate ? *o + acc[c] : acc[c];
        }
    }
}

// ------------------------------------------------------------------ adjoint of the bicubic skip
// Keys cubic taps, A = -0.75, align_corners=False: the same arithmetic as cubic_taps in upsample.hip, so that the adjoint
// weights are exactly the forward's.
__device__ __forceinline__ float ka1(float x) { const float A = -0.75f; return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float ka2(float x) { const float A = -0.75f; return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

__device__ __forceinline__ void adj_taps(int dst, float scale, int size, int idx[4], float w[4]) {
    const float real = scale * ((float)dst + 0.5f) - 0.5f;
    const float fl = floorf(real);
    const float t = real - fl;
    const int i0 = (int)fl;
    w[0] = ka2(t + 1.f);
    w[1] = ka1(t);
    w[2] = ka1(1.f - t);
    w[3] = ka2((1.f - t) + 1.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(i0 - 1 + k, 0), size - 1);
}

// An HR column ox reaches LR column x only if ox is in [(x - 2) s, (x + 3) s) (interior taps i0 - 1 .. i0 + 2 with
// i0 = floor((ox + 0.5) / s - 0.5); the clamped border taps land on x = 0 / W - 1 from inside the same range).
constexpr int BA_TW = 32, BA_TH = 8, BA_SMAX = 4;
constexpr int BA_XW = (BA_TW + 5) * BA_SMAX, BA_YH = (BA_TH + 5) * BA_SMAX;   // 148 x 52 HR elements at s = 4

// One workgroup: a BA_TH x BA_TW LR tile of one (b, c) plane.  (1) the masked HR gradient of the tile's reach is staged in
// LDS with coalesced row loads, (2) row pass: R[oy][x] = sum_ox wx(ox -> x) g[oy][ox], (3) column pass:
// d[y][x] = sum_oy wy(oy -> y) R[oy][x], one thread per LR pixel, in a fixed order.
__global__ __launch_bounds__(256) void bicubic_adjoint_kernel(const float* __restrict__ dout,
                                                              const uint8_t* __restrict__ pass, int C, int H, int W,
                                                              int s, float scale, int T, int t_center, float coef,
                                                              float* __restrict__ dframes, int accumulate, int tilesX) {
    __shared__ float gs[BA_YH][BA_XW];
    __shared__ float rs[BA_YH][BA_TW];
    __shared__ float xw[BA_XW][4], yw[BA_YH][4];
    __shared__ int xi[BA_XW][4], yi[BA_YH][4];
    const int tid = threadIdx.x;
    const int plane = blockIdx.y;                // b * C + c
    const int x0 = (blockIdx.x % tilesX) * BA_TW, y0 = (blockIdx.x / tilesX) * BA_TH;
    const int OW = W * s, OH = H * s;
    const int oxa = max(0, (x0 - 2) * s), oxb = min(OW, (x0 + BA_TW + 3) * s);
    const int oya = max(0, (y0 - 2) * s), oyb = min(OH, (y0 + BA_TH + 3) * s);
    const int nx = oxb - oxa, ny = oyb - oya;
    for (int e = tid; e < nx; e += 256) adj_taps(oxa + e, scale, W, xi[e], xw[e]);
    for (int e = tid; e < ny; e += 256) adj_taps(oya + e, scale, H, yi[e], yw[e]);
    const size_t hr0 = (size_t)plane * OH * OW;
    for (int e = tid; e < ny * nx; e += 256) {
        const int r = e / nx, q = e - r * nx;
        const size_t o = hr0 + (size_t)(oya + r) * OW + oxa + q;
        const float g = dout[o];
        gs[r][q] = (pass == nullptr || pass[o]) ? g : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < ny * BA_TW; e += 256) {
        const int r = e / BA_TW, xl = e - r * BA_TW, x = x0 + xl;
        float acc = 0.f;
        if (x < W) {
            const int qa = max(oxa, (x - 2) * s) - oxa, qb = min(oxb, (x + 3) * s) - oxa;
            for (int q = qa; q < qb; ++q) {
                float w = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) w += xi[q][k] == x ? xw[q][k] : 0.f;
                acc = fmaf(w, gs[r][q], acc);
            }
        }
        rs[r][xl] = acc;
    }
    __syncthreads();
    const int yl = tid / BA_TW, xl = tid - yl * BA_TW;
    const int y = y0 + yl, x = x0 + xl;
    if (y >= H || x >= W) return;
    const int ra = max(oya, (y - 2) * s) - oya, rb = min(oyb, (y + 3) * s) - oya;
    float acc = 0.f;
    for (int r = ra; r < rb; ++r) {
        float w = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) w += yi[r][k] == y ? yw[r][k] : 0.f;
        acc = fmaf(w, rs[r][xl], acc);
    }
    const int b = plane / C, c = plane - b * C;
    float* o = dframes + (((size_t)(b * T + t_center) * C + c) * H + y) * W + x;
    *o = accumulate ? *o + coef * acc : coef * acc;
}

// ------------------------------------------------------------------ FrameRecoveryNet: stem input gradient
// Adjoint of nn.Conv2d(4, Co, 7, 2, 3): dx[n, iy, ix, ci] = sum_{co, ky, kx} dy[n, oy, ox, co] * w[co, ci, ky, kx] over
// oy = (iy + 3 - ky) / 2, ox = (ix + 3 - kx) / 2 where those are integers in range, i.e. only the taps with
// ky = iy + 3 (mod 2) (3 or 4 per dimension).
// One workgroup: an SD_TH x SD_TW input tile of one image, one thread per input pixel (all 4 channels).  dy is staged chunk
// by chunk (SD_CC channels) with its halo in LDS, channel-major; the chunk's weights sit in LDS as [f][tap] float4s (the 4
// input channels) and are read as broadcasts.  Lanes are mapped so that every wave owns pixels of one (row, column)
// parity: the tap loops are then the same for all lanes of a wave.  Sum order: chunks ascending, f, ky, kx.
constexpr int SD_TW = 32, SD_TH = 8;
constexpr int SD_HW = SD_TW / 2 + 3, SD_HH = SD_TH / 2 + 3, SD_HP = SD_HW * SD_HH;   // halo tile: 19 x 7 = 133 pixels
constexpr int SD_CC = 16;

__global__ __launch_bounds__(256) void stem7_dgrad_kernel(const float* __restrict__ dy, int dy_ld, int dy_bf16,
                                                          const float* __restrict__ weight, int Co, int H, int W, int OH,
                                                          int OW, float* __restrict__ dframe, float* __restrict__ dmask,
                                                          int accumulate, int tilesX) {
    __shared__ float gs[SD_CC][SD_HP];
    __shared__ float4 ws[SD_CC][49];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n = blockIdx.y;
    const int ix0 = (blockIdx.x % tilesX) * SD_TW, iy0 = (blockIdx.x / tilesX) * SD_TH;
    const int oy0 = iy0 / 2 - 1, ox0 = ix0 / 2 - 1;            // halo origin (iy0, ix0 even)
    const int ty = 2 * (lane >> 4) + (wave >> 1), tx = 2 * (lane & 15) + (wave & 1);
    const int kyp = ((wave >> 1) + 1) & 1, kxp = ((wave & 1) + 1) & 1;   // first tap of the pixel's parity (wave-uniform)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const size_t pix0 = (size_t)n * OH * OW;
    for (int f0 = 0; f0 < Co; f0 += SD_CC) {
        __syncthreads();                         // the previous chunk's readers are done
        // stage: unit = (halo pixel, 8-channel half of the chunk); 266 units over 256 threads
        for (int u = tid; u < SD_HP * 2; u += 256) {
            const int p = u >> 1, h8 = (u & 1) * 8;
            const int hy = p / SD_HW, hx = p - hy * SD_HW;
            const int oy = oy0 + hy, ox = ox0 + hx;
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = 0.f;
            if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) ld8(dy, (pix0 + (size_t)oy * OW + ox) * dy_ld + f0 + h8, dy_bf16, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) gs[h8 + k][p] = v[k];
        }
        for (int e = tid; e < SD_CC * 49; e += 256) {
            const int f = e / 49, t = e - f * 49;
            const float* wr = weight + (size_t)(f0 + f) * 196 + t;
            ws[f][t] = make_float4(wr[0], wr[49], wr[98], wr[147]);
        }
        __syncthreads();
#pragma unroll 2
        for (int f = 0; f < SD_CC; ++f) {
#pragma unroll
            for (int jy = 0; jy < 4; ++jy) {
                const int ky = kyp + 2 * jy;
                if (ky < 7) {
                    const int ry = (ty + 5 - ky) >> 1;
#pragma unroll
                    for (int jx = 0; jx < 4; ++jx) {
                        const int kx = kxp + 2 * jx;
                        if (kx < 7) {
                            const float gv = gs[f][ry * SD_HW + ((tx + 5 - kx) >> 1)];
                            const float4 w4 = ws[f][ky * 7 + kx];
                            acc[0] = fmaf(gv, w4.x, acc[0]);
                            acc[1] = fmaf(gv, w4.y, acc[1]);
                            acc[2] = fmaf(gv, w4.z, acc[2]);
                            acc[3] = fmaf(gv, w4.w, acc[3]);
                        }
                    }
                }
            }
        }
    }
    const int iy = iy0 + ty, ix = ix0 + tx;
    if (iy < H && ix < W) {
        const size_t hw = (size_t)H * W, q = (size_t)iy * W + ix;
        if (dframe) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* o = dframe + ((size_t)n * 3 + c) * hw + q;
                *o = accumulate ? *o + acc[c] : acc[c];
            }
        }
        if (dmask) {
            float* o = dmask + (size_t)n * hw + q;
            *o = accumulate ? *o + acc[3] : acc[3];
        }
    }
}

// ------------------------------------------------------------------ FrameRecoveryNet: blend backward with input gradients
// out = frame * (1 - m) + rec * m: drec[n, p, c] = dout * m (channels [C, ld) = 0), dframe = dout * (1 - m),
// dmask[n, p] = sum_c dout * (rec - frame) (c ascending, one thread per pixel)
__global__ __launch_bounds__(256) void mask_blend_bwd_ex_kernel(const float* __restrict__ dout, const float* __restrict__ frame,
                                                                const float* __restrict__ rec, const float* __restrict__ mask,
                                                                int C, long HW, long total, float* __restrict__ drec, int ld,
                                                                float* __restrict__ dframe, float* __restrict__ dmask) {
    const long gid = blockIdx.x * 256L + threadIdx.x;
    if (gid >= total) return;                       // total = N * HW
    const long n = gid / HW, p = gid % HW;
    const float m = mask[gid];
    float dm = 0.f;
    for (int c = 0; c < ld; ++c) {
        if (c < C) {
            const long e = (n * C + c) * HW + p;
            const float d = dout[e];
            drec[gid * ld + c] = d * m;
            if (dframe) dframe[e] = d * (1.f - m);
            if (dmask) dm = fmaf(d, rec[gid * ld + c] - frame[e], dm);
        } else {
            drec[gid * ld + c] = 0.f;
        }
    }
    if (dmask) dmask[gid] = dm;
}

}  // namespace nvq

using namespace nvq;

namespace {

int launch_head_dgrad(const char* what, const float* dout, int dout_ld, int dout_bf16, const float* dout2, int dout2_ld,
                      const float* act, int act_ld, int act_bf16, const float* weight, int F, int B, int T, int Cin, int H,
                      int W, const DgSlots& sm, int nslots, int slot_images, float* dframes, int accumulate, void* stream) {
    const int tilesX = (W + DG_TW - 1) / DG_TW, tilesY = (H + DG_TH - 1) / DG_TH;
    const long ntiles = (long)tilesX * tilesY, nimg = (long)nslots * B;
    NVQ_REQUIRE(ntiles < ((long)1 << 31) && nimg <= 65535, "%s: grid too large", what);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ntiles, (unsigned)nimg);
    if (Cin == 3)
        hipLaunchKernelGGL((head_dgrad_kernel<3>), grid, dim3(256), 0, s, dout, dout_ld, dout_bf16, dout2, dout2_ld, act,
                           act_ld, act_bf16, weight, F, B, T, H, W, sm, slot_images, dframes, accumulate, tilesX);
    else
        hipLaunchKernelGGL((head_dgrad_kernel<1>), grid, dim3(256), 0, s, dout, dout_ld, dout_bf16, dout2, dout2_ld, act,
                           act_ld, act_bf16, weight, F, B, T, H, W, sm, slot_images, dframes, accumulate, tilesX);
    return check_launch(what);
}

}  // namespace

extern "C" {

int nvq_head_dgrad(const float* dout, int dout_ld, int dout_bf16, const float* dout2, int dout2_ld, const float* act,
                   int act_ld, int act_bf16, const float* weight, int F, int B, int T, int Cin, int H, int W,
                   const int* t_of_slot_host, int nslots, float* dframes, int accumulate, void* stream) {
    NVQ_REQUIRE(Cin == 3 || Cin == 1, "head_dgrad: in_channels %d not supported (1 or 3)", Cin);
    NVQ_REQUIRE(F >= DG_CC && F <= 256 && F % DG_CC == 0, "head_dgrad: F %d (a multiple of %d in [16, 256])", F, DG_CC);
    NVQ_REQUIRE(B >= 1 && H >= 1 && W >= 1, "head_dgrad: B %d H %d W %d", B, H, W);
    NVQ_REQUIRE(nslots >= 1 && nslots <= NVQ_MAX_T && T >= 1 && T <= NVQ_MAX_T, "head_dgrad: T %d slots %d", T, nslots);
    NVQ_REQUIRE(dout && weight && dframes, "head_dgrad: NULL dout / weight / dframes");
    NVQ_REQUIRE(act || !dout2, "head_dgrad: dout2 needs act (the pre-masked form takes one gradient)");
    NVQ_REQUIRE(dout_ld >= F && dout_ld % 8 == 0 && aligned16(dout), "head_dgrad: dout ld %d / alignment", dout_ld);
    NVQ_REQUIRE(!act || (act_ld >= F && act_ld % 8 == 0 && aligned16(act)), "head_dgrad: act ld %d / alignment", act_ld);
    NVQ_REQUIRE(!dout2 || (dout2_ld >= F && dout2_ld % 8 == 0 && aligned16(dout2)), "head_dgrad: dout2 ld %d / alignment",
                dout2_ld);
    DgSlots sm;
    for (int i = 0; i < NVQ_MAX_T; ++i) {
        sm.t[i] = i < nslots ? t_of_slot_host[i] : 0;
        sm.c[i] = 0;
        NVQ_REQUIRE(sm.t[i] >= 0 && sm.t[i] < T, "head_dgrad: slot %d maps to frame %d of %d", i, sm.t[i], T);
    }
    return launch_head_dgrad("head_dgrad", dout, dout_ld, dout_bf16, dout2, dout2_ld, act, act_ld, act_bf16, weight, F, B,
                             T, Cin, H, W, sm, nslots, B, dframes, accumulate, stream);
}

int nvq_head_dgrad_tc(const float* dout, int dout_ld, int dout_bf16, const float* weight, int F, int B, int T, int Cin,
                      int H, int W, const int* t_of_slot_host, const int* coff_of_slot_host, int nslots, int slot_images,
                      float* dframes, int accumulate, void* stream) {
    NVQ_REQUIRE(Cin == 3 || Cin == 1, "head_dgrad_tc: in_channels %d not supported (1 or 3)", Cin);
    NVQ_REQUIRE(F >= DG_CC && F <= 256 && F % DG_CC == 0, "head_dgrad_tc: F %d (a multiple of %d in [16, 256])", F, DG_CC);
    NVQ_REQUIRE(B >= 1 && H >= 1 && W >= 1, "head_dgrad_tc: B %d H %d W %d", B, H, W);
    NVQ_REQUIRE(nslots >= 1 && nslots <= NVQ_MAX_T && T >= 1 && T <= NVQ_MAX_T, "head_dgrad_tc: T %d slots %d", T, nslots);
    NVQ_REQUIRE(slot_images == 0 || slot_images == B, "head_dgrad_tc: slot_images %d (0 or B = %d)", slot_images, B);
    NVQ_REQUIRE(dout && weight && dframes, "head_dgrad_tc: NULL dout / weight / dframes");
    NVQ_REQUIRE(dout_ld % 8 == 0 && aligned16(dout), "head_dgrad_tc: dout ld %d / alignment", dout_ld);
    DgSlots sm;
    for (int i = 0; i < NVQ_MAX_T; ++i) {
        sm.t[i] = i < nslots ? t_of_slot_host[i] : 0;
        sm.c[i] = i < nslots ? coff_of_slot_host[i] : 0;
        NVQ_REQUIRE(sm.t[i] >= 0 && sm.t[i] < T, "head_dgrad_tc: slot %d maps to frame %d of %d", i, sm.t[i], T);
        NVQ_REQUIRE(sm.c[i] >= 0 && sm.c[i] % 8 == 0 && sm.c[i] + F <= dout_ld,
                    "head_dgrad_tc: slot %d channel offset %d (a multiple of 8, + F %d <= ld %d)", i, sm.c[i], F, dout_ld);
    }
    return launch_head_dgrad("head_dgrad_tc", dout, dout_ld, dout_bf16, nullptr, 0, nullptr, 0, 0, weight, F, B, T, Cin, H,
                             W, sm, nslots, slot_images, dframes, accumulate, stream);
}

int nvq_stem7_dgrad(const float* dy, int dy_ld, int dy_bf16, const float* weight, int N, int H, int W, int Co,
                    float* dframe, float* dmask, int accumulate, void* stream) {
    NVQ_REQUIRE(Co >= SD_CC && Co <= 64 && Co % SD_CC == 0, "stem7_dgrad: Co %d (a multiple of %d in [16, 64])", Co, SD_CC);
    NVQ_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "stem7_dgrad: N %d H %d W %d", N, H, W);
    NVQ_REQUIRE(dy && weight, "stem7_dgrad: NULL dy / weight");
    NVQ_REQUIRE(dframe || dmask, "stem7_dgrad: NULL dframe and dmask (nothing to write)");
    NVQ_REQUIRE(dy_ld >= Co && dy_ld % 8 == 0 && aligned16(dy), "stem7_dgrad: dy ld %d / alignment", dy_ld);
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int tilesX = (W + SD_TW - 1) / SD_TW, tilesY = (H + SD_TH - 1) / SD_TH;
    const long ntiles = (long)tilesX * tilesY;
    NVQ_REQUIRE(ntiles < ((long)1 << 31), "stem7_dgrad: grid too large");
    hipLaunchKernelGGL(stem7_dgrad_kernel, dim3((unsigned)ntiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, dy, dy_ld,
                       dy_bf16, weight, Co, H, W, OH, OW, dframe, dmask, accumulate, tilesX);
    return check_launch("stem7_dgrad");
}

int nvq_mask_blend_backward_ex(const float* dout, const float* frame, const float* rec, int rec_ld, const float* mask, int N,
                               int C, int H, int W, float* drec, float* dframe, float* dmask, void* stream) {
    NVQ_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1 && C <= rec_ld, "mask_blend_backward_ex: N %d C %d H %d W %d ld %d", N,
                C, H, W, rec_ld);
    NVQ_REQUIRE(dout && mask && drec, "mask_blend_backward_ex: NULL dout / mask / drec");
    NVQ_REQUIRE(!dmask || (frame && rec), "mask_blend_backward_ex: dmask needs frame and rec");
    const long HW = (long)H * W, total = (long)N * HW;
    hipLaunchKernelGGL(mask_blend_bwd_ex_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, dout, frame,
                       rec, mask, C, HW, total, drec, rec_ld, dframe, dmask);
    return check_launch("mask_blend_backward_ex");
}

int nvq_bicubic_adjoint(const float* dout, const uint8_t* pass, int B, int Cimg, int H, int W, int s, int T, int t_center,
                        float coef, float* dframes, int accumulate, void* stream) {
    NVQ_REQUIRE(s >= 1 && s <= BA_SMAX, "bicubic_adjoint: scale factor %d (1..%d)", s, BA_SMAX);
    NVQ_REQUIRE(B >= 1 && Cimg >= 1 && H >= 1 && W >= 1, "bicubic_adjoint: B %d C %d H %d W %d", B, Cimg, H, W);
    NVQ_REQUIRE(t_center >= 0 && t_center < T, "bicubic_adjoint: t_center %d of %d frames", t_center, T);
    NVQ_REQUIRE(dout && dframes, "bicubic_adjoint: NULL dout / dframes");
    const int tilesX = (W + BA_TW - 1) / BA_TW, tilesY = (H + BA_TH - 1) / BA_TH;
    const long ntiles = (long)tilesX * tilesY, nplanes = (long)B * Cimg;
    NVQ_REQUIRE(ntiles < ((long)1 << 31) && nplanes <= 65535, "bicubic_adjoint: grid too large");
    hipLaunchKernelGGL(bicubic_adjoint_kernel, dim3((unsigned)ntiles, (unsigned)nplanes), dim3(256), 0, (hipStream_t)stream,
                       dout, pass, Cimg, H, W, s, (float)(1.0 / (double)s), T, t_center, coef, dframes, accumulate, tilesX);
    return check_launch("bicubic_adjoint");
}

}  // extern "C"
