// Image-quality sums, pixel losses (L1 / Charbonnier / MSE with per-sample reduction) and the windowed SSIM
// (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, valid positions only) with its gradient, on fp32 NCHW tensors.
// Everything is fp32 on the VALU with two-stage reductions (fp32 per block, double in fixed order across blocks): no float
// atomics anywhere, so two runs give the same bits.
//
// quality_sums / pixel_loss: the two-stage pattern of loss.hip with blockIdx.y = sample (a workgroup never
// straddles two samples).  HBM-bound: two reads per element (+ one write for the pixel-loss backward).
//
// SSIM: one workgroup per (image plane, tile).  `moments_tile` stages the x and y tiles with their halo in LDS, runs the
// horizontal 11-tap pass of (x, y, x^2, y^2, xy) into LDS and the vertical pass in registers, and hands the five local
// moments of every position to a functor: the forward sums the SSIM map value (never stored), the backward turns them into
// the map's derivatives A, B, C with respect to mu_x, E[x^2], E[xy], keeps those in LDS and applies the adjoint filter in
// gather form (one owner thread per dx element, fixed tap order): dx = G^T[A] + 2 x G^T[B] + y G^T[C].
//
// Multi-scale SSIM: the same two kernels per scale of a 2 x 2 mean pyramid with a contrast-structure
// functor, one launch that pools x and y together, and a finalize that forms the clamped weighted product and its derivatives.
#include "flat.h"

namespace nvq {

namespace {

constexpr int kTaps = 11, kHalo = kTaps - 1;
struct Taps { float g[kTaps]; };

// Gaussian taps, sigma 1.5, normalised to sum 1 in fp32
Taps gaussian_taps() {
    Taps t;
    float s = 0.f;
    for (int i = 0; i < kTaps; ++i) {
        const float d = (float)(i - kTaps / 2);
        t.g[i] = expf(-(d * d) / (2.f * 1.5f * 1.5f));
        s += t.g[i];
    }
    for (int i = 0; i < kTaps; ++i) t.g[i] /= s;
    return t;
}

// ------------------------------------------------------------------------------------------------ sums and pixel losses

constexpr int kSums = 7;   // sum x, y, x^2, y^2, xy, |x-y|, (x-y)^2

struct SumAcc {
    float s[kSums];
    __device__ __forceinline__ void add(float x, float y) {
        const float d = x - y;
        s[0] += x; s[1] += y; s[2] += x * x; s[3] += y * y; s[4] += x * y; s[5] += fabsf(d); s[6] += d * d;
    }
};

// grid (nbs, B): block (k, b) covers a strided share of sample b; part[(b * nbs + k) * 7 + q]
template <bool VEC>
__global__ __launch_bounds__(256) void quality_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, long per,
                                                           float* __restrict__ part) {
    __shared__ float scratch[4];
    const float* xs = x + (long)blockIdx.y * per;
    const float* ys = y + (long)blockIdx.y * per;
    SumAcc a;
#pragma unroll
    for (int q = 0; q < kSums; ++q) a.s[q] = 0.f;
    if (VEC) {
        const long n4 = per >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const float4 u = ld4(xs + 4 * i), v = ld4(ys + 4 * i);
            a.add(u.x, v.x); a.add(u.y, v.y); a.add(u.z, v.z); a.add(u.w, v.w);
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < per; i += (long)gridDim.x * 256) a.add(xs[i], ys[i]);
    }
    float* p = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * kSums;
#pragma unroll
    for (int q = 0; q < kSums; ++q) {
        const float s = block_sum_256(a.s[q], scratch);
        if (threadIdx.x == 0) p[q] = s;
    }
}

// grid (B): out[b * 8 + ...] = n, then the seven sums, added in double in a fixed order
__global__ __launch_bounds__(256) void quality_sums_final_kernel(const float* __restrict__ part, int nbs, long per,
                                                                 double* __restrict__ out) {
    __shared__ double scratch[256];
    const float* p = part + (long)blockIdx.x * nbs * kSums;
#pragma unroll 1
    for (int q = 0; q < kSums; ++q) {
        double s = 0.0;
        for (int k = threadIdx.x; k < nbs; k += 256) s += (double)p[(long)k * kSums + q];
        s = block_tree_sum_256(s, scratch);
        if (threadIdx.x == 0) out[blockIdx.x * 8 + 1 + q] = s;
    }
    if (threadIdx.x == 0) out[blockIdx.x * 8] = (double)per;
}

template <int KIND>
__device__ __forceinline__ float pixel_value(float d, float eps2) {
    if (KIND == NVQ_LOSS_L1) return fabsf(d);
    if (KIND == NVQ_LOSS_CHARBONNIER) return sqrtf(d * d + eps2);
    return d * d;
}
template <int KIND>
__device__ __forceinline__ float pixel_slope(float d, float eps2) {
    if (KIND == NVQ_LOSS_L1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    if (KIND == NVQ_LOSS_CHARBONNIER) return d / sqrtf(d * d + eps2);
    return 2.f * d;
}

// grid (nbs, G): part[g * nbs + k] = block k's share of sum f(x - y) over group g
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void pixel_loss_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 long per, float eps2, float* __restrict__ part) {
    __shared__ float scratch[4];
    const float* xs = x + (long)blockIdx.y * per;
    const float* ys = y + (long)blockIdx.y * per;
    float s = 0.f;
    if (VEC) {
        const long n4 = per >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const float4 u = ld4(xs + 4 * i), v = ld4(ys + 4 * i);
            s += (pixel_value<KIND>(u.x - v.x, eps2) + pixel_value<KIND>(u.y - v.y, eps2)) +
                 (pixel_value<KIND>(u.z - v.z, eps2) + pixel_value<KIND>(u.w - v.w, eps2));
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < per; i += (long)gridDim.x * 256)
            s += pixel_value<KIND>(xs[i] - ys[i], eps2);
    }
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// dx = go[g] * f'(x - y) / per
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void pixel_loss_backward_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  long per, float eps2, const float* __restrict__ go,
                                                                  float inv_per, float* __restrict__ dx) {
    const long base = (long)blockIdx.y * per;
    const float* xs = x + base;
    const float* ys = y + base;
    float* ds = dx + base;
    const float sc = inv_per * (go ? go[blockIdx.y] : 1.f);
    if (VEC) {
        const long n4 = per >> 2;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            const float4 u = ld4(xs + 4 * i), v = ld4(ys + 4 * i);
            st4(ds + 4 * i, make_float4(sc * pixel_slope<KIND>(u.x - v.x, eps2), sc * pixel_slope<KIND>(u.y - v.y, eps2),
                                        sc * pixel_slope<KIND>(u.z - v.z, eps2), sc * pixel_slope<KIND>(u.w - v.w, eps2)));
        }
    } else {
        for (long i = blockIdx.x * 256L + threadIdx.x; i < per; i += (long)gridDim.x * 256)
            ds[i] = sc * pixel_slope<KIND>(xs[i] - ys[i], eps2);
    }
}

// ------------------------------------------------------------------------------------------------------ windowed SSIM

// Geometry of one moments tile: MH x MW positions (MW a multiple of 4) need (MH + 10) x (MW + 10) inputs; the staged input
// tile is IW = MW + 12 wide so that every row is whole float4s.
template <int MH_, int MW_>
struct TileGeom {
    static constexpr int MH = MH_, MW = MW_, IH = MH_ + kHalo, IW = MW_ + 12;
    static constexpr int XY_FLOATS = 2 * IH * IW;   // staged x and y
    static constexpr int HP_FLOATS = 5 * IH * MW;   // horizontal pass of x, y, x^2, y^2, xy
};

// The five local moments of the MH x MW positions whose top-left input pixel is (r0, c0) of the H x W planes xp, yp.
// Inputs outside the plane read as 0 (such positions are not valid ones; the callers mask them).  c0 is a multiple of 4.
// xy: XY_FLOATS of LDS, hp: HP_FLOATS of LDS.  emit(mr, mc, mu_x, mu_y, E[x^2], E[y^2], E[xy]) runs once per position.
// xy is dead once the vertical pass starts (emit may overwrite it); hp is still being read when this returns:
// synchronise before reusing it.
// CENTRE (the multi-scale kernels): the moments are those of x - centre and y - centre.  Variances and the covariance do not
// depend on the centre, and with it at mid-range E[x^2] - mu^2 no longer cancels; the caller adds it back to the means.
template <class G, int RV, bool CENTRE = false, class Emit>
__device__ __forceinline__ void moments_tile(const float* __restrict__ xp, const float* __restrict__ yp, int H, int W,
                                             int r0, int c0, bool vec, const Taps& t, float* xy, float* hp, Emit emit,
                                             float centre = 0.f) {
    constexpr int MH = G::MH, MW = G::MW, IH = G::IH, IW = G::IW;
    float* xs = xy;
    float* ys = xy + IH * IW;
    // 1. stage
    for (int ch = threadIdx.x; ch < IH * (IW / 4); ch += 256) {
        const int row = ch / (IW / 4), col = 4 * (ch % (IW / 4));
        const int gr = r0 + row, gc = c0 + col;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
        if (gr >= 0 && gr < H) {
            const long o = (long)gr * W + gc;
            if (vec && gc >= 0 && gc + 3 < W) {
                u = ld4(xp + o);
                v = ld4(yp + o);
            } else {
                if (gc >= 0 && gc < W) { u.x = xp[o]; v.x = yp[o]; }
                if (gc + 1 >= 0 && gc + 1 < W) { u.y = xp[o + 1]; v.y = yp[o + 1]; }
                if (gc + 2 >= 0 && gc + 2 < W) { u.z = xp[o + 2]; v.z = yp[o + 2]; }
                if (gc + 3 >= 0 && gc + 3 < W) { u.w = xp[o + 3]; v.w = yp[o + 3]; }
            }
            if (CENTRE) {   // columns outside the plane become -centre: only masked positions read them
                u = make_float4(u.x - centre, u.y - centre, u.z - centre, u.w - centre);
                v = make_float4(v.x - centre, v.y - centre, v.z - centre, v.w - centre);
            }
        }
        st4(xs + row * IW + col, u);
        st4(ys + row * IW + col, v);
    }
    __syncthreads();
    // 2. horizontal pass: four neighbouring positions of one row per item
    for (int it = threadIdx.x; it < IH * (MW / 4); it += 256) {
        const int row = it / (MW / 4), col = 4 * (it % (MW / 4));
        float a[16], b[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 u = ld4(xs + row * IW + col + 4 * k), v = ld4(ys + row * IW + col + 4 * k);
            a[4 * k] = u.x; a[4 * k + 1] = u.y; a[4 * k + 2] = u.z; a[4 * k + 3] = u.w;
            b[4 * k] = v.x; b[4 * k + 1] = v.y; b[4 * k + 2] = v.z; b[4 * k + 3] = v.w;
        }
        float acc[5][4];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[q][o] = 0.f;
#pragma unroll
        for (int i = 0; i < 14; ++i) {
            const float xx = a[i] * a[i], yy = b[i] * b[i], xv = a[i] * b[i];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int k = i - o;
                if (k >= 0 && k < kTaps) {
                    acc[0][o] = fmaf(t.g[k], a[i], acc[0][o]);
                    acc[1][o] = fmaf(t.g[k], b[i], acc[1][o]);
                    acc[2][o] = fmaf(t.g[k], xx, acc[2][o]);
                    acc[3][o] = fmaf(t.g[k], yy, acc[3][o]);
                    acc[4][o] = fmaf(t.g[k], xv, acc[4][o]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 5; ++q)
            st4(hp + (q * IH + row) * MW + col, make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]));
    }
    __syncthreads();
    // 3. vertical pass: RV positions of one column per item
    constexpr int NG = (MH + RV - 1) / RV;
    for (int it = threadIdx.x; it < NG * MW; it += 256) {
        const int col = it % MW, rb = (it / MW) * RV;
        float acc[RV][5];
#pragma unroll
        for (int o = 0; o < RV; ++o)
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[o][q] = 0.f;
#pragma unroll
        for (int r = 0; r < RV + kHalo; ++r) {
            float v[5];
            const bool in = rb + r < IH;
#pragma unroll
            for (int q = 0; q < 5; ++q) v[q] = in ? hp[(q * IH + rb + r) * MW + col] : 0.f;
#pragma unroll
            for (int o = 0; o < RV; ++o) {
                const int k = r - o;
                if (k >= 0 && k < kTaps) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) acc[o][q] = fmaf(t.g[k], v[q], acc[o][q]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < RV; ++o)
            if (rb + o < MH) emit(rb + o, col, acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4]);
    }
}

// forward tile: 32 x 64 valid positions per workgroup
constexpr int kFTH = 32, kFTW = 64;
using FwdGeom = TileGeom<kFTH, kFTW>;

__global__ __launch_bounds__(256) void ssim_forward_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                           int W, int tiles_x, int tiles_y, int vec, float c1, float c2,
                                                           Taps t, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float xy[FwdGeom::XY_FLOATS];
    __shared__ __attribute__((aligned(16))) float hp[FwdGeom::HP_FLOATS];
    __shared__ float scratch[4];
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, plane = tile / (tiles_x * tiles_y);
    const int r0 = ty * kFTH, c0 = tx * kFTW, OH = H - kHalo, OW = W - kHalo;
    const long po = (long)plane * H * W;
    float s = 0.f;
    moments_tile<FwdGeom, 8>(x + po, y + po, H, W, r0, c0, vec != 0, t, xy, hp,
                             [&](int mr, int mc, float mx, float my, float exx, float eyy, float exy) {
                                 const float mxy = mx * my, m2 = mx * mx + my * my;
                                 const float sxy = exy - mxy, s2 = (exx - mx * mx) + (eyy - my * my);
                                 const float v = ((2.f * mxy + c1) * (2.f * sxy + c2)) / ((m2 + c1) * (s2 + c2));
                                 if (r0 + mr < OH && c0 + mc < OW) s += v;
                             });
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) part[tile] = s;
}

// backward tile: 16 x 64 elements of dx per workgroup.  They gather from the 26 x 74 positions above and to the left; the
// moments tile starts 12 (not 10) columns to the left so that its rows stay float4-aligned: 26 x 76 positions.
constexpr int kBTH = 16, kBTW = 64, kBLead = 12;
using BwdGeom = TileGeom<kBTH + kHalo, kBTW + kBLead>;
constexpr int kAbcFloats = 3 * BwdGeom::MH * BwdGeom::MW;
constexpr int kBwdR1 = BwdGeom::XY_FLOATS > kAbcFloats ? BwdGeom::XY_FLOATS : kAbcFloats;

__global__ __launch_bounds__(256) void ssim_backward_kernel(const float* __restrict__ x, const float* __restrict__ y, int C,
                                                            int H, int W, int tiles_x, int tiles_y, int vec, float c1, float c2,
                                                            Taps t, const float* __restrict__ go, int go_per_sample,
                                                            float scale, float* __restrict__ dx) {
    constexpr int MH = BwdGeom::MH, MW = BwdGeom::MW;
    __shared__ __attribute__((aligned(16))) float r1[kBwdR1];               // staged x, y; then A, B, C
    __shared__ __attribute__((aligned(16))) float r2[BwdGeom::HP_FLOATS];   // horizontal pass; then that of the adjoint
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, plane = tile / (tiles_x * tiles_y);
    const int r0 = ty * kBTH - kHalo, c0 = tx * kBTW - kBLead, OH = H - kHalo, OW = W - kHalo;
    const long po = (long)plane * H * W;
    const float sc = scale * (go ? go[go_per_sample ? plane / C : 0] : 1.f);

    // nothing reads the staged x, y after the barrier that ends the horizontal pass: A, B, C overwrite them in place
    moments_tile<BwdGeom, 9>(x + po, y + po, H, W, r0, c0, vec != 0, t, r1, r2,
                             [&](int mr, int mc, float mx, float my, float exx, float eyy, float exy) {
                                 const int pr = r0 + mr, pc = c0 + mc;
                                 float a = 0.f, b = 0.f, c = 0.f;
                                 if (pr >= 0 && pr < OH && pc >= 0 && pc < OW) {
                                     const float a1 = 2.f * mx * my + c1, a2 = 2.f * (exy - mx * my) + c2;
                                     const float b1 = mx * mx + my * my + c1, b2 = (exx - mx * mx) + (eyy - my * my) + c2;
                                     const float ib1 = 1.f / b1, ib2 = 1.f / b2, ib = ib1 * ib2, S = a1 * a2 * ib;
                                     a = sc * (2.f * my * (a2 - a1) * ib + 2.f * mx * S * (ib2 - ib1));
                                     b = -sc * S * ib2;
                                     c = sc * 2.f * a1 * ib;
                                 }
                                 r1[(0 * MH + mr) * MW + mc] = a;
                                 r1[(1 * MH + mr) * MW + mc] = b;
                                 r1[(2 * MH + mr) * MW + mc] = c;
                             });
    __syncthreads();
    // adjoint, horizontal: element column j gathers positions m = j + 2 .. j + 12 with tap (j + 12 - m)
    for (int it = threadIdx.x; it < MH * (kBTW / 4); it += 256) {
        const int row = it / (kBTW / 4), col = 4 * (it % (kBTW / 4));
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float a[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 u = ld4(r1 + (q * MH + row) * MW + col + 4 * k);
                a[4 * k] = u.x; a[4 * k + 1] = u.y; a[4 * k + 2] = u.z; a[4 * k + 3] = u.w;
            }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kTaps; ++k)
#pragma unroll
                for (int o = 0; o < 4; ++o) acc[o] = fmaf(t.g[k], a[o + kBLead - k], acc[o]);
            st4(r2 + (q * MH + row) * kBTW + col, make_float4(acc[0], acc[1], acc[2], acc[3]));
        }
    }
    __syncthreads();
    // adjoint, vertical: element row i gathers position rows i .. i + 10 (tile-relative) with tap (i + 10 - row)
    {
        constexpr int RO = kBTH / 4;
        const int col = threadIdx.x & 63, ib = (threadIdx.x >> 6) * RO;
        float acc[RO][3];
#pragma unroll
        for (int o = 0; o < RO; ++o) acc[o][0] = acc[o][1] = acc[o][2] = 0.f;
#pragma unroll
        for (int r = 0; r < RO + kHalo; ++r) {
            float v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = r2[(q * MH + ib + r) * kBTW + col];
#pragma unroll
            for (int o = 0; o < RO; ++o) {
                const int k = o + kHalo - r;
                if (k >= 0 && k < kTaps) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc[o][q] = fmaf(t.g[k], v[q], acc[o][q]);
                }
            }
        }
        const int gc = tx * kBTW + col;
#pragma unroll
        for (int o = 0; o < RO; ++o) {
            const int gr = ty * kBTH + ib + o;
            if (gr < H && gc < W) {
                const long e = po + (long)gr * W + gc;
                dx[e] = acc[o][0] + 2.f * x[e] * acc[o][1] + y[e] * acc[o][2];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ multi-scale SSIM
// Scale j of the pyramid (x_1 = x, x_{j+1} = 2 x 2 mean of x_j) contributes the plane mean of cs = (2 s_xy + C2) / (s_xx + s_yy
// + C2) (j < M) or of the SSIM map l * cs (j = M).  The kernels below are the SSIM pair with that functor, a per-plane upstream
// factor and the pooling adjoint folded into the backward's store.  They take their moments about the centre 0.5 L (see
// moments_tile): a coarse scale has few positions, down to a single one, so the cancellation error of E[x^2] - mu^2 is not
// averaged away there as it is over a full-size plane, and the weights put most of the product on those scales.

constexpr int kMaxScales = 8;

// tiles of one plane of every scale's forward pass, where its partials start in the workspace, 1 / valid positions
struct ScaleGeom {
    int tpp[kMaxScales];
    long off[kMaxScales];
    double inv_count[kMaxScales];
    long total;
};

ScaleGeom scale_geom(int planes, int H, int W, int scales) {
    ScaleGeom g;
    long off = 0;
    for (int j = 0; j < kMaxScales; ++j) {
        const int h = H >> j, w = W >> j;
        const bool on = j < scales && h >= kTaps && w >= kTaps;
        g.tpp[j] = on ? ceil_div(h - kHalo, 32) * ceil_div(w - kHalo, 64) : 0;
        g.off[j] = off;
        g.inv_count[j] = on ? 1.0 / ((double)(h - kHalo) * (double)(w - kHalo)) : 0.0;
        off += (long)planes * g.tpp[j];
    }
    g.total = off;
    return g;
}

// PyTorch's avg_pool2d order: ((a + b) + c) + d over the window's rows, then / 4
__device__ __forceinline__ float pool4(float a, float b, float c, float d) { return (((a + b) + c) + d) * 0.25f; }

// 2 x 2 mean, stride 2, of the H x W planes of x and y in one launch (an odd last row or column is dropped).  Workgroup
// blockIdx.x covers a strided share of plane blockIdx.x / nbp: it never straddles two planes.  VEC (W % 4 == 0): an item is
// two neighbouring outputs from two 16-byte loads per tensor.
template <bool VEC>
__global__ __launch_bounds__(256) void avgpool2_pair_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                            int W, int nbp, float* __restrict__ px, float* __restrict__ py) {
    const int plane = blockIdx.x / nbp, blk = blockIdx.x % nbp;
    const int OH = H >> 1, OW = W >> 1;
    const long pi = (long)plane * H * W, po = (long)plane * OH * OW;
    const float* xs = x + pi;
    const float* ys = y + pi;
    float* pxs = px + po;
    float* pys = py + po;
    if (VEC) {
        const int hw = OW >> 1, n2 = OH * hw;
        for (int i = blk * 256 + threadIdx.x; i < n2; i += nbp * 256) {
            const int r = i / hw, c = i % hw;
            const long o = (long)(2 * r) * W + 4 * c;
            const float4 a = ld4(xs + o), b = ld4(xs + o + W), u = ld4(ys + o), v = ld4(ys + o + W);
            const long e = (long)r * OW + 2 * c;
            *reinterpret_cast<float2*>(pxs + e) = make_float2(pool4(a.x, a.y, b.x, b.y), pool4(a.z, a.w, b.z, b.w));
            *reinterpret_cast<float2*>(pys + e) = make_float2(pool4(u.x, u.y, v.x, v.y), pool4(u.z, u.w, v.z, v.w));
        }
    } else {
        const int n = OH * OW;
        for (int i = blk * 256 + threadIdx.x; i < n; i += nbp * 256) {
            const int r = i / OW, c = i % OW;
            const long o = (long)(2 * r) * W + 2 * c;
            pxs[i] = pool4(xs[o], xs[o + 1], xs[o + W], xs[o + W + 1]);
            pys[i] = pool4(ys[o], ys[o + 1], ys[o + W], ys[o + W + 1]);
        }
    }
}

// ssim_forward_kernel on centred moments: part[tile] = sum over the tile's valid positions of cs (CS) or of l * cs
template <bool CS>
__global__ __launch_bounds__(256) void msssim_forward_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                             int W, int tiles_x, int tiles_y, int vec, float c1, float c2,
                                                             float centre, Taps t, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float xy[FwdGeom::XY_FLOATS];
    __shared__ __attribute__((aligned(16))) float hp[FwdGeom::HP_FLOATS];
    __shared__ float scratch[4];
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, plane = tile / (tiles_x * tiles_y);
    const int r0 = ty * kFTH, c0 = tx * kFTW, OH = H - kHalo, OW = W - kHalo;
    const long po = (long)plane * H * W;
    float s = 0.f;
    moments_tile<FwdGeom, 8, true>(x + po, y + po, H, W, r0, c0, vec != 0, t, xy, hp,
                                   [&](int mr, int mc, float mx, float my, float exx, float eyy, float exy) {
                                       const float sxy = exy - mx * my, s2 = (exx - mx * mx) + (eyy - my * my);
                                       float v;
                                       if (CS) {
                                           v = (2.f * sxy + c2) / (s2 + c2);
                                       } else {
                                           const float ux = mx + centre, uy = my + centre;
                                           const float mxy = ux * uy, m2 = ux * ux + uy * uy;
                                           v = ((2.f * mxy + c1) * (2.f * sxy + c2)) / ((m2 + c1) * (s2 + c2));
                                       }
                                       if (r0 + mr < OH && c0 + mc < OW) s += v;
                                   },
                                   centre);
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) part[tile] = s;
}

// One workgroup of 16 waves; a wave owns whole samples (b = wave, wave + 16, ...).  Per plane and scale it adds the tile
// partials in double (lane-strided, then a butterfly: a fixed order), lane j keeps m_j; the clamp, the powers, the product and
// its derivatives are formed in double by lanes 0 .. M-1.  mt[j][plane] = m_j, dt[j][plane] = d ms(b) / d m_j(b, c) (0 where a
// term is clamped: never 0 * inf).  out: (B,) or (1,), the value or 1 - value.
__global__ __launch_bounds__(1024) void msssim_finalize_kernel(const float* __restrict__ part, ScaleGeom g, int M, int B, int C,
                                                               const float* __restrict__ w, int per_sample, int as_loss,
                                                               float* __restrict__ out, float* __restrict__ mt,
                                                               float* __restrict__ dt) {
    __shared__ double wave_acc[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long planes = (long)B * C;
    const double wj = lane < M ? (double)w[lane] : 0.0;
    double acc = 0.0;
    for (int b = wave; b < B; b += 16) {
        double vs = 0.0;
        for (int c = 0; c < C; ++c) {
            const long plane = (long)b * C + c;
            double m = 1.0;
            for (int j = 0; j < M; ++j) {
                const int n = g.tpp[j];
                const float* q = part + g.off[j] + plane * n;
                double s = 0.0;
                for (int k = lane; k < n; k += 64) s += (double)q[k];
                s = wave_sum(s);
                if (lane == j) m = s * g.inv_count[j];
            }
            const double pw = lane < M ? (m > 0.0 ? pow(m, wj) : 0.0) : 1.0;
            double v = 1.0, others = 1.0;
            for (int k = 0; k < M; ++k) {
                const double pk = __shfl(pw, k, 64);
                v *= pk;
                if (k != lane) others *= pk;
            }
            if (lane < M) {
                mt[lane * planes + plane] = (float)m;
                dt[lane * planes + plane] = m > 0.0 ? (float)(wj * (pw / m) * others / (double)C) : 0.f;
            }
            vs += v;
        }
        const double ms = vs / (double)C;
        if (per_sample) {
            if (lane == 0) out[b] = (float)(as_loss ? 1.0 - ms : ms);
        } else {
            acc += ms;
        }
    }
    if (per_sample) return;
    if (lane == 0) wave_acc[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += wave_acc[k];
        s /= (double)B;
        out[0] = (float)(as_loss ? 1.0 - s : s);
    }
}

// ssim_backward_kernel for one scale of the pyramid.  The upstream factor is per plane: scale * go[b or 0] * dplane[plane]
// (dplane: this scale's row of the finalize's derivative table); CS selects the contrast-structure functor
//   d cs / d mu_x = (2 mu_x cs - 2 mu_y) / b2,  d cs / d E[x^2] = -cs / b2,  d cs / d E[xy] = 2 / b2,  b2 = s_xx + s_yy + C2
// and the store adds the pooling adjoint of the next coarser scale's gradient dxc (HC x WC planes, may be NULL):
// dx[r][c] = own + 0.25 dxc[r / 2][c / 2] wherever that element exists.  The moments are centred: the derivatives are those
// with respect to x - centre, which are those with respect to x; only the luminance term sees the uncentred means.
template <bool CS>
__global__ __launch_bounds__(256) void msssim_backward_kernel(const float* __restrict__ x, const float* __restrict__ y, int C,
                                                              int H, int W, int tiles_x, int tiles_y, int vec, float c1, float c2,
                                                              float centre, Taps t, const float* __restrict__ dplane,
                                                              const float* __restrict__ go, int go_per_sample, float scale,
                                                              const float* __restrict__ dxc, int HC, int WC,
                                                              float* __restrict__ dx) {
    constexpr int MH = BwdGeom::MH, MW = BwdGeom::MW;
    __shared__ __attribute__((aligned(16))) float r1[kBwdR1];               // staged x, y; then A, B, C
    __shared__ __attribute__((aligned(16))) float r2[BwdGeom::HP_FLOATS];   // horizontal pass; then that of the adjoint
    const int tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, plane = tile / (tiles_x * tiles_y);
    const int r0 = ty * kBTH - kHalo, c0 = tx * kBTW - kBLead, OH = H - kHalo, OW = W - kHalo;
    const long po = (long)plane * H * W;
    const float sc = scale * (go ? go[go_per_sample ? plane / C : 0] : 1.f) * dplane[plane];

    moments_tile<BwdGeom, 9, true>(x + po, y + po, H, W, r0, c0, vec != 0, t, r1, r2,
                                   [&](int mr, int mc, float mx, float my, float exx, float eyy, float exy) {
                                       const int pr = r0 + mr, pc = c0 + mc;
                                       float a = 0.f, b = 0.f, c = 0.f;
                                       if (pr >= 0 && pr < OH && pc >= 0 && pc < OW) {
                                           const float a2 = 2.f * (exy - mx * my) + c2;
                                           const float b2 = (exx - mx * mx) + (eyy - my * my) + c2, ib2 = 1.f / b2;
                                           if (CS) {
                                               const float cs = a2 * ib2;
                                               a = sc * (2.f * mx * cs - 2.f * my) * ib2;
                                               b = -sc * cs * ib2;
                                               c = sc * 2.f * ib2;
                                           } else {
                                               // l = a1 / b1 in the uncentred means ux, uy; cs = a2 / b2 in the centred ones
                                               const float ux = mx + centre, uy = my + centre;
                                               const float a1 = 2.f * ux * uy + c1, b1 = ux * ux + uy * uy + c1;
                                               const float ib1 = 1.f / b1, ib = ib1 * ib2, S = a1 * a2 * ib;
                                               a = sc * (2.f * (uy * a2 - my * a1) * ib + 2.f * S * (mx * ib2 - ux * ib1));
                                               b = -sc * S * ib2;
                                               c = sc * 2.f * a1 * ib;
                                           }
                                       }
                                       r1[(0 * MH + mr) * MW + mc] = a;
                                       r1[(1 * MH + mr) * MW + mc] = b;
                                       r1[(2 * MH + mr) * MW + mc] = c;
                                   },
                                   centre);
    __syncthreads();
    // adjoint, horizontal: element column j gathers positions m = j + 2 .. j + 12 with tap (j + 12 - m)
    for (int it = threadIdx.x; it < MH * (kBTW / 4); it += 256) {
        const int row = it / (kBTW / 4), col = 4 * (it % (kBTW / 4));
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float a[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 u = ld4(r1 + (q * MH + row) * MW + col + 4 * k);
                a[4 * k] = u.x; a[4 * k + 1] = u.y; a[4 * k + 2] = u.z; a[4 * k + 3] = u.w;
            }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kTaps; ++k)
#pragma unroll
                for (int o = 0; o < 4; ++o) acc[o] = fmaf(t.g[k], a[o + kBLead - k], acc[o]);
            st4(r2 + (q * MH + row) * kBTW + col, make_float4(acc[0], acc[1], acc[2], acc[3]));
        }
    }
    __syncthreads();
    // adjoint, vertical: element row i gathers position rows i .. i + 10 (tile-relative) with tap (i + 10 - row)
    {
        constexpr int RO = kBTH / 4;
        const int col = threadIdx.x & 63, ib = (threadIdx.x >> 6) * RO;
        float acc[RO][3];
#pragma unroll
        for (int o = 0; o < RO; ++o) acc[o][0] = acc[o][1] = acc[o][2] = 0.f;
#pragma unroll
        for (int r = 0; r < RO + kHalo; ++r) {
            float v[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) v[q] = r2[(q * MH + ib + r) * kBTW + col];
#pragma unroll
            for (int o = 0; o < RO; ++o) {
                const int k = o + kHalo - r;
                if (k >= 0 && k < kTaps) {
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc[o][q] = fmaf(t.g[k], v[q], acc[o][q]);
                }
            }
        }
        const int gc = tx * kBTW + col;
        const long pc = (long)plane * HC * WC;
#pragma unroll
        for (int o = 0; o < RO; ++o) {
            const int gr = ty * kBTH + ib + o;
            if (gr < H && gc < W) {
                const long e = po + (long)gr * W + gc;
                float d = acc[o][0] + 2.f * (x[e] - centre) * acc[o][1] + (y[e] - centre) * acc[o][2];
                if (dxc && (gr >> 1) < HC && (gc >> 1) < WC) d += 0.25f * dxc[pc + (long)(gr >> 1) * WC + (gc >> 1)];
                dx[e] = d;
            }
        }
    }
}

}  // namespace

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_quality_sums(const float* x, const float* y, int B, long per, double* out, float* workspace, size_t workspace_bytes,
                     void* stream) {
    NVQ_REQUIRE(B > 0 && B <= 65535 && per > 0 && aligned16(x) && aligned16(y) && aligned8(out),
                "quality_sums: 0 < B <= 65535, per > 0, 16-byte aligned tensors");
    const int nbs = group_blocks(per, B);
    if ((size_t)B * nbs * kSums * sizeof(float) > workspace_bytes) { set_error("quality_sums: workspace"); return NVQ_EWORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    if ((per & 3) == 0)
        hipLaunchKernelGGL(quality_sums_kernel<true>, dim3(nbs, B), dim3(256), 0, s, x, y, per, workspace);
    else
        hipLaunchKernelGGL(quality_sums_kernel<false>, dim3(nbs, B), dim3(256), 0, s, x, y, per, workspace);
    int rc = check_launch("quality_sums");
    if (rc) return rc;
    hipLaunchKernelGGL(quality_sums_final_kernel, dim3(B), dim3(256), 0, s, workspace, nbs, per, out);
    return check_launch("quality_sums_final");
}

#define NVQ_PIXEL_DISPATCH(KERNEL, ...)                                                                                  \
    with_bools([&](auto V) {                                                                                             \
        if (kind == NVQ_LOSS_L1) hipLaunchKernelGGL((KERNEL<NVQ_LOSS_L1, V()>), grid, dim3(256), 0, s, __VA_ARGS__);     \
        else if (kind == NVQ_LOSS_CHARBONNIER)                                                                           \
            hipLaunchKernelGGL((KERNEL<NVQ_LOSS_CHARBONNIER, V()>), grid, dim3(256), 0, s, __VA_ARGS__);                 \
        else hipLaunchKernelGGL((KERNEL<NVQ_LOSS_MSE, V()>), grid, dim3(256), 0, s, __VA_ARGS__);                        \
    }, vec)

int nvq_pixel_loss_forward(const float* x, const float* y, int groups, long per, int kind, float eps, float* out,
                           float* workspace, size_t workspace_bytes, void* stream) {
    NVQ_REQUIRE(groups > 0 && groups <= 65535 && per > 0 && aligned16(x) && aligned16(y),
                "pixel_loss_forward: 0 < groups <= 65535, per > 0, 16-byte aligned tensors");
    NVQ_REQUIRE(kind == NVQ_LOSS_L1 || kind == NVQ_LOSS_CHARBONNIER || kind == NVQ_LOSS_MSE, "pixel_loss_forward: kind %d", kind);
    const int nbs = group_blocks(per, groups);
    if ((size_t)groups * nbs * sizeof(float) > workspace_bytes) { set_error("pixel_loss_forward: workspace"); return NVQ_EWORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (per & 3) == 0;
    const dim3 grid(nbs, groups);
    NVQ_PIXEL_DISPATCH(pixel_loss_partial_kernel, x, y, per, eps * eps, workspace);
    int rc = check_launch("pixel_loss_partial");
    if (rc) return rc;
    launch_group_final(workspace, nbs, groups, 1.0 / (double)per, 0.0, out, s);
    return check_launch("pixel_loss_final");
}

int nvq_pixel_loss_backward(const float* x, const float* y, int groups, long per, int kind, float eps,
                            const float* grad_out_dev, float* dx, void* stream) {
    NVQ_REQUIRE(groups > 0 && groups <= 65535 && per > 0 && aligned16(x) && aligned16(y) && aligned16(dx),
                "pixel_loss_backward: 0 < groups <= 65535, per > 0, 16-byte aligned tensors");
    NVQ_REQUIRE(kind == NVQ_LOSS_L1 || kind == NVQ_LOSS_CHARBONNIER || kind == NVQ_LOSS_MSE, "pixel_loss_backward: kind %d", kind);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (per & 3) == 0;
    const dim3 grid(group_blocks(per, groups), groups);
    NVQ_PIXEL_DISPATCH(pixel_loss_backward_kernel, x, y, per, eps * eps, grad_out_dev, (float)(1.0 / (double)per), dx);
    return check_launch("pixel_loss_backward");
}

static int ssim_check(const char* what, const void* x, const void* y, int B, int C, int H, int W, float data_range, int th,
                      int tw, int full, long* tiles) {
    NVQ_REQUIRE(B > 0 && C > 0 && H >= kTaps && W >= kTaps && data_range > 0.f && aligned16(x) && aligned16(y),
                "%s: B, C > 0, H, W >= 11, data_range > 0, 16-byte aligned tensors", what);
    const long tx = ceil_div(full ? W : W - kHalo, tw), ty = ceil_div(full ? H : H - kHalo, th);
    *tiles = (long)B * C * tx * ty;
    NVQ_REQUIRE(*tiles <= 0x7fffffffL && (long)B * C * H * W > 0, "%s: too many tiles", what);
    return NVQ_OK;
}

int nvq_ssim_forward(const float* x, const float* y, int B, int C, int H, int W, float data_range, int per_sample,
                     int as_loss, float* out, float* workspace, size_t workspace_bytes, void* stream) {
    long tiles;
    int rc = ssim_check("ssim_forward", x, y, B, C, H, W, data_range, kFTH, kFTW, 0, &tiles);
    if (rc) return rc;
    if ((size_t)tiles * sizeof(float) > workspace_bytes) { set_error("ssim_forward: workspace"); return NVQ_EWORKSPACE; }
    hipStream_t s = (hipStream_t)stream;
    const int tx = ceil_div(W - kHalo, kFTW), ty = ceil_div(H - kHalo, kFTH);
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    hipLaunchKernelGGL(ssim_forward_kernel, dim3((unsigned)tiles), dim3(256), 0, s, x, y, H, W, tx, ty, (int)((W & 3) == 0), c1,
                       c2, gaussian_taps(), workspace);
    rc = check_launch("ssim_forward");
    if (rc) return rc;
    const int groups = per_sample ? B : 1;
    const double count = (double)(tiles / groups) / ((double)tx * ty) * (double)(H - kHalo) * (double)(W - kHalo);
    launch_group_final(workspace, (int)(tiles / groups), groups, (as_loss ? -1.0 : 1.0) / count, as_loss ? 1.0 : 0.0, out, s);
    return check_launch("ssim_final");
}

int nvq_ssim_backward(const float* x, const float* y, int B, int C, int H, int W, float data_range,
                      const float* grad_out_dev, int grad_per_sample, float scale, float* dx, void* stream) {
    long tiles;
    int rc = ssim_check("ssim_backward", x, y, B, C, H, W, data_range, kBTH, kBTW, 1, &tiles);
    if (rc) return rc;
    NVQ_REQUIRE(aligned16(dx), "ssim_backward: 16-byte aligned dx");
    const int tx = ceil_div(W, kBTW), ty = ceil_div(H, kBTH);
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    const double count = (double)(grad_per_sample ? 1 : B) * C * (double)(H - kHalo) * (double)(W - kHalo);
    hipLaunchKernelGGL(ssim_backward_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, x, y, C, H, W, tx, ty,
                       (int)((W & 3) == 0), c1, c2, gaussian_taps(), grad_out_dev, grad_per_sample, (float)(scale / count), dx);
    return check_launch("ssim_backward");
}

int nvq_avgpool2_pair(const float* x, const float* y, int planes, int H, int W, float* px, float* py, void* stream) {
    NVQ_REQUIRE(planes > 0 && H >= 2 && W >= 2 && (long)H * W <= 0x7fffffffL && aligned16(x) && aligned16(y) && aligned16(px) &&
                    aligned16(py),
                "avgpool2_pair: planes > 0, H, W >= 2, H * W < 2^31, 16-byte aligned tensors");
    const bool vec = (W & 3) == 0;
    const long items = (long)(H >> 1) * (vec ? W >> 2 : W >> 1);
    int nbp = ceil_div(items, 256L * 4);
    if (nbp > 1024) nbp = 1024;
    NVQ_REQUIRE((long)planes * nbp <= 0x7fffffffL, "avgpool2_pair: too many planes");
    const dim3 grid((unsigned)(planes * nbp));
    if (vec)
        hipLaunchKernelGGL(avgpool2_pair_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, y, H, W, nbp, px, py);
    else
        hipLaunchKernelGGL(avgpool2_pair_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, y, H, W, nbp, px, py);
    return check_launch("avgpool2_pair");
}

static int msssim_check(const char* what, long planes, int H, int W, int scales, int scale, float data_range) {
    NVQ_REQUIRE(planes > 0 && planes <= 0x7fffffffL && scales >= 1 && scales <= kMaxScales && scale >= 0 && scale < scales &&
                    data_range > 0.f,
                "%s: planes > 0, 1 <= scales <= 8, 0 <= scale < scales, data_range > 0", what);
    NVQ_REQUIRE(H > 0 && W > 0 && (H >> (scales - 1)) >= kTaps && (W >> (scales - 1)) >= kTaps,
                "%s: the coarsest of %d scales of %d x %d holds no 11 x 11 window", what, scales, H, W);
    return NVQ_OK;
}

size_t nvq_msssim_workspace_bytes(int planes, int H, int W, int scales) {
    if (planes <= 0 || H <= 0 || W <= 0 || scales < 1 || scales > kMaxScales) return 0;
    return (size_t)scale_geom(planes, H, W, scales).total * sizeof(float);
}

int nvq_msssim_scale_forward(const float* xs, const float* ys, int planes, int H, int W, int scales, int scale,
                             float data_range, float* workspace, size_t workspace_bytes, void* stream) {
    int rc = msssim_check("msssim_scale_forward", planes, H, W, scales, scale, data_range);
    if (rc) return rc;
    NVQ_REQUIRE(aligned16(xs) && aligned16(ys), "msssim_scale_forward: 16-byte aligned tensors");
    const ScaleGeom g = scale_geom(planes, H, W, scales);
    if ((size_t)g.total * sizeof(float) > workspace_bytes) { set_error("msssim_scale_forward: workspace"); return NVQ_EWORKSPACE; }
    const int h = H >> scale, w = W >> scale;
    const long tiles = (long)planes * g.tpp[scale];
    NVQ_REQUIRE(tiles <= 0x7fffffffL, "msssim_scale_forward: too many tiles");
    const int tx = ceil_div(w - kHalo, kFTW), ty = ceil_div(h - kHalo, kFTH);
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    float* part = workspace + g.off[scale];
    if (scale + 1 < scales)
        hipLaunchKernelGGL(msssim_forward_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, xs, ys, h, w, tx,
                           ty, (int)((w & 3) == 0), c1, c2, 0.5f * data_range, gaussian_taps(), part);
    else
        hipLaunchKernelGGL(msssim_forward_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, xs, ys, h, w, tx,
                           ty, (int)((w & 3) == 0), c1, c2, 0.5f * data_range, gaussian_taps(), part);
    return check_launch("msssim_scale_forward");
}

int nvq_msssim_finalize(const float* workspace, int B, int C, int H, int W, int scales, const float* weights, int per_sample,
                        int as_loss, float* out, float* mtable, float* dtable, void* stream) {
    NVQ_REQUIRE(B > 0 && C > 0, "msssim_finalize: B, C > 0");
    int rc = msssim_check("msssim_finalize", (long)B * C, H, W, scales, 0, 1.f);
    if (rc) return rc;
    NVQ_REQUIRE(workspace && weights && out && mtable && dtable, "msssim_finalize: NULL argument");
    hipLaunchKernelGGL(msssim_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, workspace,
                       scale_geom(B * C, H, W, scales), scales, B, C, weights, per_sample, as_loss, out, mtable, dtable);
    return check_launch("msssim_finalize");
}

int nvq_msssim_scale_backward(const float* xs, const float* ys, int B, int C, int H, int W, int scales, int scale,
                              float data_range, const float* dtable, const float* grad_out_dev, int grad_per_sample,
                              float sign, const float* dx_coarser, float* dx, void* stream) {
    NVQ_REQUIRE(B > 0 && C > 0, "msssim_scale_backward: B, C > 0");
    const long planes = (long)B * C;
    int rc = msssim_check("msssim_scale_backward", planes, H, W, scales, scale, data_range);
    if (rc) return rc;
    NVQ_REQUIRE(aligned16(xs) && aligned16(ys) && aligned16(dx) && dtable, "msssim_scale_backward: 16-byte aligned tensors");
    NVQ_REQUIRE(dx_coarser == nullptr || scale + 1 < scales, "msssim_scale_backward: the coarsest scale has no coarser gradient");
    const int h = H >> scale, w = W >> scale;
    const int tx = ceil_div(w, kBTW), ty = ceil_div(h, kBTH);
    const long tiles = planes * tx * ty;
    NVQ_REQUIRE(tiles <= 0x7fffffffL, "msssim_scale_backward: too many tiles");
    const float c1 = (0.01f * data_range) * (0.01f * data_range), c2 = (0.03f * data_range) * (0.03f * data_range);
    const double count = (double)(grad_per_sample ? 1 : B) * (double)(h - kHalo) * (double)(w - kHalo);
    const float* dplane = dtable + (long)scale * planes;
    const dim3 grid((unsigned)tiles);
    hipStream_t s = (hipStream_t)stream;
    if (scale + 1 < scales)
        hipLaunchKernelGGL(msssim_backward_kernel<true>, grid, dim3(256), 0, s, xs, ys, C, h, w, tx, ty, (int)((w & 3) == 0), c1,
                           c2, 0.5f * data_range, gaussian_taps(), dplane, grad_out_dev, grad_per_sample, (float)(sign / count), dx_coarser, h >> 1,
                           w >> 1, dx);
    else
        hipLaunchKernelGGL(msssim_backward_kernel<false>, grid, dim3(256), 0, s, xs, ys, C, h, w, tx, ty, (int)((w & 3) == 0), c1,
                           c2, 0.5f * data_range, gaussian_taps(), dplane, grad_out_dev, grad_per_sample, (float)(sign / count), dx_coarser, h >> 1,
                           w >> 1, dx);
    return check_launch("msssim_scale_backward");
}

}  // extern "C"
