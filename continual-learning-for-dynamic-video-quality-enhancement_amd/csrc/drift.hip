// Drift detection on device-resident samples: the RBF Gram sums of the biased MMD estimator in float64
// on v_mfma_f64_16x16x4_f64, np.histogram-exact counts and the population stability index, per-cell mean / standard deviation
// clip descriptors, and the sliding metric window of the performance monitor.  No float atomics anywhere: every sum is a
// function of the shapes only, so a score is bit-reproducible.
#include "flat.h"

namespace nvq {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GT = 64;            // output tile (rows of a x rows of b) of one workgroup
constexpr int GK = 32;            // features staged per chunk
constexpr int GLD = GK + 4;       // LDS row stride in floats: 36 r + k (r < 16, k < 4) covers 64 distinct banks
constexpr int KLD = GT + 1;       // row stride in doubles of the finished tile

// Sum over 256 threads in a fixed order; valid in thread 0.  scratch: >= 4 doubles of LDS.  The wave sums meet pairwise,
// (w0 + w1) + (w2 + w3), not left to right as in flat.h's block_wave_sum_256: the order is part of the scores' bits.
__device__ __forceinline__ double block_sum_f64_256(double v, double* scratch) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// Index of tile (lo, hi), lo <= hi, among the upper-triangle tiles of a T x T grid, row-major.
__device__ __forceinline__ int tri_index(int lo, int hi, int T) { return lo * T - lo * (lo - 1) / 2 + (hi - lo); }

// Rows [row0, row0 + 64) x features [k0, k0 + 32) of a row-major (rows x d) matrix, gathered through idx when given, into
// dst[64][GLD]; rows past n, indices outside [0, rows) and features past d are zeros.
__device__ __forceinline__ void stage_rows(const float* __restrict__ x, const int* __restrict__ idx, int n, int rows, int d,
                                           int row0, int k0, float* dst) {
    const int c = threadIdx.x & 31;
    const int k = k0 + c;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int r = (threadIdx.x >> 5) + 8 * m;
        const int i = row0 + r;
        float v = 0.f;
        if (i < n && k < d) {
            const int src = idx ? idx[i] : i;
            if (src >= 0 && src < rows) v = x[(size_t)src * d + k];
        }
        dst[r * GLD + c] = v;
    }
}

// One 64 x 64 tile of K[i][j] = exp(-gamma (|a_i|^2 + |b_j|^2 - 2 a_i.b_j)), summed into part[blockIdx.x].
//
// Four waves, each a 32 x 32 quarter as 2 x 2 MFMA tiles.  Per k-step of 4 a wave issues 8 v_mfma_f64_16x16x4_f64: four for
// a.b, two for the row norms (A = a^2, B = 1: D[i][j] = |a_i|^2 for every j) and two for the column norms (A = 1, B = b^2), so
// the three terms arrive in the same accumulator layout and meet without a lane exchange.  fp32 inputs are widened on the way
// out of LDS (exact), and a^2 of an fp32 value is exact in double.
//
// The tile sum is formed so that it does not change under transposition: the finished tile goes to LDS and the sum runs over
// K[r][c] + K[c][r] (r < c) and K[r][r] in index order.  Tile (j, i) of a symmetric problem holds the transposed values of
// tile (i, j) bit for bit (same products, same k order, commutative additions), hence the same partial: the symmetric form
// may skip it.
__global__ __launch_bounds__(256) void rbf_gram_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const int* __restrict__ ia, const int* __restrict__ ib, int na,
                                                            int nb, int a_rows, int b_rows, int d,
                                                            const double* __restrict__ gamma_dev, int symmetric, int Tb,
                                                            double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double smem[GT * KLD];      // 33 KiB; the two staged chunks (18 KiB) live in it first
    __shared__ double scratch[4];
    float* As = reinterpret_cast<float*>(smem);
    float* Bs = As + GT * GLD;

    int ti, tj;
    if (symmetric) {
        int rem = blockIdx.x;
        ti = 0;
        while (rem >= Tb - ti) {
            rem -= Tb - ti;
            ++ti;
        }
        tj = ti + rem;
    } else {
        ti = blockIdx.x / Tb;
        tj = blockIdx.x - ti * Tb;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int lr = lane & 15, lk = lane >> 4;

    f64x4 xy[2][2], xx[2], yy[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        xx[m] = (f64x4){0.0, 0.0, 0.0, 0.0};
        yy[m] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int n = 0; n < 2; ++n) xy[m][n] = (f64x4){0.0, 0.0, 0.0, 0.0};
    }

    for (int k0 = 0; k0 < d; k0 += GK) {
        __syncthreads();
        stage_rows(a, ia, na, a_rows, d, ti * GT, k0, As);
        stage_rows(b, ib, nb, b_rows, d, tj * GT, k0, Bs);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                av[m] = (double)As[(wr + 16 * m + lr) * GLD + kk + lk];
                bv[m] = (double)Bs[(wc + 16 * m + lr) * GLD + kk + lk];
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                xx[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m] * av[m], 1.0, xx[m], 0, 0, 0);
                yy[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, bv[m] * bv[m], yy[m], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < 2; ++n) xy[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[n], xy[m][n], 0, 0, 0);
            }
        }
    }

    const double gamma = gamma_dev ? gamma_dev[0] : 1.0 / (double)d;
    __syncthreads();                                                    // the staged chunks are dead: smem becomes the tile
    // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = wr + 16 * m + lk + 4 * reg, c = wc + 16 * n + lr;
                const double dist = (xx[m][reg] + yy[n][reg]) - 2.0 * xy[m][n][reg];
                const bool live = ti * GT + r < na && tj * GT + c < nb;
                smem[r * KLD + c] = live ? exp(-gamma * dist) : 0.0;
            }
    __syncthreads();
    double s = 0.0;
#pragma unroll 4
    for (int e = threadIdx.x; e < GT * GT; e += 256) {
        const int r = e >> 6, c = e & 63;
        if (r < c) s += smem[r * KLD + c] + smem[c * KLD + r];
        else if (r == c) s += smem[r * KLD + r];
    }
    s = block_sum_f64_256(s, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One block: out = sum over the Ta x Tb tile slots in slot order; the symmetric form reads slot (i, j) from tile
// (min, max), so an off-diagonal tile counts twice and the additions are those of the rectangular form on (a, a).
__global__ __launch_bounds__(256) void rbf_gram_final_kernel(const double* __restrict__ part, int Ta, int Tb, int symmetric,
                                                             double* __restrict__ out) {
    __shared__ double scratch[4];
    double s = 0.0;
    const int slots = Ta * Tb;
    for (int e = threadIdx.x; e < slots; e += 256) {
        int idx = e;
        if (symmetric) {
            const int i = e / Tb, j = e - i * Tb;
            idx = tri_index(i < j ? i : j, i < j ? j : i, Tb);
        }
        s += part[idx];
    }
    s = block_sum_f64_256(s, scratch);
    if (threadIdx.x == 0) out[0] = s;
}

// sums = {sum K(ref, ref), sum K(cur, cur), sum K(ref, cur)}: the biased estimator, diagonals included
__global__ void mmd_finish_kernel(const double* __restrict__ sums, int na, int nb, float threshold, double* __restrict__ score,
                                  unsigned char* __restrict__ flag) {
    const double n = (double)na, m = (double)nb;
    const double mmd = sums[0] / (n * n) + sums[1] / (m * m) - 2.0 * sums[2] / (n * m);
    score[0] = mmd;
    flag[0] = mmd > (double)threshold ? 1 : 0;
}

constexpr int PSI_MAX_EDGES = 11;

// np.histogram(x, bins=edges): bin i = [e_i, e_{i+1}), the last bin closed on the right, values outside [e_0, e_last] (and
// NaN) uncounted; comparisons in double.  Counts in LDS, then one global integer atomic per bin and block.
__global__ __launch_bounds__(256) void psi_counts_kernel(const float* __restrict__ x, long n, const double* __restrict__ edges,
                                                         int nedges, int* __restrict__ counts) {
    __shared__ int local[PSI_MAX_EDGES];
    __shared__ double e[PSI_MAX_EDGES];
    if (threadIdx.x < PSI_MAX_EDGES) {
        local[threadIdx.x] = 0;
        e[threadIdx.x] = threadIdx.x < nedges ? edges[threadIdx.x] : 0.0;
    }
    __syncthreads();
    const int nbins = nedges - 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const double v = (double)x[i];
        if (!(v >= e[0] && v <= e[nbins])) continue;
        int bin = 0;
        for (int j = 1; j < nbins; ++j) bin += v >= e[j] ? 1 : 0;
        atomicAdd(&local[bin], 1);
    }
    __syncthreads();
    if (threadIdx.x < nbins && local[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], local[threadIdx.x]);
}

__global__ void psi_finish_kernel(const int* __restrict__ cur, const int* __restrict__ ref, int nbins, long len_cur, long len_ref,
                                  double* __restrict__ score, unsigned char* __restrict__ flag) {
    double psi = 0.0;
    for (int i = 0; i < nbins; ++i) {
        const double rp = (double)ref[i] / (double)len_ref + 1e-10;
        const double cp = (double)cur[i] / (double)len_cur + 1e-10;
        psi += (cp - rp) * log(cp / rp);
    }
    score[0] = psi;
    flag[0] = psi > 0.2 ? 1 : 0;
}

// One wave per (image, channel, cell).  A lane owns whole quads (4 consecutive columns of one cell row, the last quad of a row
// may be short) in both forms, and adds their elements in column order: the vector form only changes how a full, aligned quad
// is fetched, so both forms give the same bits.  Two passes over the cell (the second one hits the cache): mean, then the
// mean of squared deviations, both summed in double.
template <bool VEC>
__global__ __launch_bounds__(256) void cell_descriptor_kernel(const float* __restrict__ x, int B, int C, int H, int W, int gh,
                                                              int gw, float* __restrict__ out) {
    const long cell = blockIdx.x * 4L + (threadIdx.x >> 6);
    const long cells = (long)B * C * gh * gw;
    if (cell >= cells) return;                                          // wave-uniform
    const int lane = threadIdx.x & 63;
    const int j = (int)(cell % gw);
    const int i = (int)((cell / gw) % gh);
    const long bc = cell / ((long)gw * gh);
    const int c = (int)(bc % C);
    const long bimg = bc / C;
    const int h0 = (int)((long)i * H / gh), h1 = (int)(((long)(i + 1) * H + gh - 1) / gh);
    const int w0 = (int)((long)j * W / gw), w1 = (int)(((long)(j + 1) * W + gw - 1) / gw);
    const int cw = w1 - w0, ch = h1 - h0;
    const int qpr = (cw + 3) >> 2;                                      // quads per cell row
    const int nq = ch * qpr;
    const float* base = x + (size_t)bc * H * W;
    const bool vec = VEC && (w0 & 3) == 0;
    const double cnt = (double)ch * (double)cw;

    double mean = 0.0, dev = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        double s = 0.0;
        for (int q = lane; q < nq; q += 64) {
            const int r = q / qpr, qc = q - r * qpr;
            const int col = w0 + 4 * qc;
            const int len = w1 - col < 4 ? w1 - col : 4;
            const float* p = base + (size_t)(h0 + r) * W + col;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec && len == 4) {
                const float4 t = ld4(p);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                for (int k = 0; k < len; ++k) v[k] = p[k];
            }
            for (int k = 0; k < len; ++k) {
                const double t = (double)v[k] - mean;                   // pass 0: mean == 0
                s += pass == 0 ? t : t * t;
            }
        }
        s = wave_sum(s);
        if (pass == 0) mean = s / cnt;
        else dev = s / cnt;
    }
    if (lane == 0) {
        const long per = (long)C * gh * gw;
        const long o = bimg * 2 * per + ((long)c * gh + i) * gw + j;
        out[o] = (float)mean;
        out[o + per] = (float)sqrt(dev);
    }
}

// state[0] = next ring position, state[1] = values held (<= window)
__global__ __launch_bounds__(256) void metric_window_kernel(const float* __restrict__ value, float* __restrict__ ring,
                                                            int* __restrict__ state, int window, float baseline, float threshold,
                                                            double* __restrict__ mean_out, unsigned char* __restrict__ flag) {
    __shared__ double scratch[4];
    __shared__ int filled_s;
    if (threadIdx.x == 0) {
        int pos = state[0];
        int filled = state[1];
        if (pos < 0 || pos >= window) pos = 0;                          // a state the caller did not zero never indexes past the ring
        if (filled < 0) filled = 0;
        ring[pos] = value[0];
        state[0] = pos + 1 == window ? 0 : pos + 1;
        if (filled < window) ++filled;
        state[1] = filled;
        filled_s = filled;
        __threadfence_block();
    }
    __syncthreads();
    const int filled = filled_s;
    double s = 0.0;
    for (int i = threadIdx.x; i < filled; i += 256) s += (double)ring[i];
    s = block_sum_f64_256(s, scratch);
    if (threadIdx.x == 0) {
        const double mean = s / (double)filled;
        mean_out[0] = mean;
        const double b = (double)baseline;
        flag[0] = (filled >= window && (b - mean) / b > (double)threshold) ? 1 : 0;
    }
}

}  // namespace nvq

using namespace nvq;

extern "C" {

size_t nvq_rbf_gram_workspace_bytes(int na, int nb, int symmetric) {
    if (na < 1 || nb < 1) return 0;
    const size_t Ta = (size_t)ceil_div(na, GT), Tb = (size_t)ceil_div(nb, GT);
    return (symmetric ? Ta * (Ta + 1) / 2 : Ta * Tb) * sizeof(double);
}

int nvq_rbf_gram_sum(const float* a, const float* b, const int* a_index, const int* b_index, int na, int nb, int a_rows,
                     int b_rows, int d, const double* gamma_dev, int symmetric, double* out, float* workspace,
                     size_t workspace_bytes, void* stream) {
    NVQ_REQUIRE(a != nullptr && b != nullptr && out != nullptr, "rbf_gram_sum: a / b / out");
    NVQ_REQUIRE(na >= 1 && nb >= 1 && d >= 1, "rbf_gram_sum: na, nb, d must be >= 1 (got %d, %d, %d)", na, nb, d);
    NVQ_REQUIRE(a_rows >= 1 && b_rows >= 1 && (a_index != nullptr || na <= a_rows) && (b_index != nullptr || nb <= b_rows),
                "rbf_gram_sum: %d / %d rows asked of matrices with %d / %d rows", na, nb, a_rows, b_rows);
    NVQ_REQUIRE(!symmetric || (a == b && a_index == b_index && na == nb && a_rows == b_rows),
                "rbf_gram_sum: symmetric needs the same matrix, index array and count on both sides");
    NVQ_REQUIRE(aligned8(out) && aligned8(workspace) && aligned8(gamma_dev), "rbf_gram_sum: out, workspace and gamma must be 8-byte aligned");
    const long Ta = ceil_div(na, GT), Tb = ceil_div(nb, GT);
    const long nblk = symmetric ? Ta * (Ta + 1) / 2 : Ta * Tb;
    NVQ_REQUIRE(Ta * Tb <= 0x7fffffffL, "rbf_gram_sum: too many tiles");
    if (workspace == nullptr || (size_t)nblk * sizeof(double) > workspace_bytes) {
        set_error("rbf_gram_sum: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)nblk * sizeof(double));
        return NVQ_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(rbf_gram_tile_kernel, dim3((unsigned)nblk), dim3(256), 0, s, a, b, a_index, b_index, na, nb, a_rows, b_rows,
                       d, gamma_dev, symmetric ? 1 : 0, (int)Tb, part);
    int rc = check_launch("rbf_gram_tile");
    if (rc) return rc;
    hipLaunchKernelGGL(rbf_gram_final_kernel, dim3(1), dim3(256), 0, s, part, (int)Ta, (int)Tb, symmetric ? 1 : 0, out);
    return check_launch("rbf_gram_final");
}

int nvq_mmd_finish(const double* sums, int na, int nb, float threshold, double* score_out, unsigned char* flag_out, void* stream) {
    NVQ_REQUIRE(sums != nullptr && score_out != nullptr && flag_out != nullptr, "mmd_finish: sums / score_out / flag_out");
    NVQ_REQUIRE(na >= 1 && nb >= 1, "mmd_finish: na, nb must be >= 1");
    NVQ_REQUIRE(aligned8(sums) && aligned8(score_out), "mmd_finish: sums and score_out must be 8-byte aligned");
    hipLaunchKernelGGL(mmd_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sums, na, nb, threshold, score_out, flag_out);
    return check_launch("mmd_finish");
}

int nvq_psi_counts(const float* x, long n, const double* edges, int nedges, int* counts, void* stream) {
    NVQ_REQUIRE(x != nullptr && edges != nullptr && counts != nullptr, "psi_counts: x / edges / counts");
    NVQ_REQUIRE(n >= 1 && n <= 0x7fffffffL, "psi_counts: n must be in [1, 2^31)");
    NVQ_REQUIRE(nedges >= 2 && nedges <= PSI_MAX_EDGES, "psi_counts: %d edges (2 .. %d)", nedges, PSI_MAX_EDGES);
    NVQ_REQUIRE(aligned8(edges), "psi_counts: edges must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)(nedges - 1) * sizeof(int), s) != hipSuccess) return check_launch("psi_counts memset");
    int nblk = ceil_div(n, 256L * 8);
    if (nblk > 1024) nblk = 1024;
    hipLaunchKernelGGL(psi_counts_kernel, dim3(nblk), dim3(256), 0, s, x, n, edges, nedges, counts);
    return check_launch("psi_counts");
}

int nvq_psi_finish(const int* cur_counts, const int* ref_counts, int nbins, long len_cur, long len_ref, double* score_out,
                   unsigned char* flag_out, void* stream) {
    NVQ_REQUIRE(cur_counts != nullptr && ref_counts != nullptr && score_out != nullptr && flag_out != nullptr,
                "psi_finish: counts / score_out / flag_out");
    NVQ_REQUIRE(nbins >= 1 && nbins < PSI_MAX_EDGES && len_cur >= 1 && len_ref >= 1, "psi_finish: nbins / lengths");
    NVQ_REQUIRE(aligned8(score_out), "psi_finish: score_out must be 8-byte aligned");
    hipLaunchKernelGGL(psi_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cur_counts, ref_counts, nbins, len_cur, len_ref,
                       score_out, flag_out);
    return check_launch("psi_finish");
}

int nvq_cell_descriptor(const float* x, int B, int C, int H, int W, int gh, int gw, float* out, void* stream) {
    NVQ_REQUIRE(x != nullptr && out != nullptr, "cell_descriptor: x / out");
    NVQ_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "cell_descriptor: B, C, H, W must be >= 1");
    NVQ_REQUIRE(gh >= 1 && gw >= 1 && gh <= H && gw <= W, "cell_descriptor: grid %d x %d on %d x %d frames", gh, gw, H, W);
    const long cells = (long)B * C * gh * gw;
    NVQ_REQUIRE(cells <= 4L * 0x7fffffffL, "cell_descriptor: too many cells");
    const dim3 grid((unsigned)((cells + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(x) && (W & 3) == 0) hipLaunchKernelGGL(cell_descriptor_kernel<true>, grid, block, 0, s, x, B, C, H, W, gh, gw, out);
    else hipLaunchKernelGGL(cell_descriptor_kernel<false>, grid, block, 0, s, x, B, C, H, W, gh, gw, out);
    return check_launch("cell_descriptor");
}

int nvq_metric_window_update(const float* value, float* ring, int* state, int window, float baseline, float threshold,
                             double* mean_out, unsigned char* flag_out, void* stream) {
    NVQ_REQUIRE(value != nullptr && ring != nullptr && state != nullptr && mean_out != nullptr && flag_out != nullptr,
                "metric_window_update: value / ring / state / mean_out / flag_out");
    NVQ_REQUIRE(window >= 1, "metric_window_update: window must be >= 1");
    NVQ_REQUIRE(aligned8(mean_out), "metric_window_update: mean_out must be 8-byte aligned");
    hipLaunchKernelGGL(metric_window_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, value, ring, state, window, baseline,
                       threshold, mean_out, flag_out);
    return check_launch("metric_window_update");
}

}  // extern "C"
