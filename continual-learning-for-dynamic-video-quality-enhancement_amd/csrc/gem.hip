// Gradient Episodic Memory (GEM, Lopez-Paz & Ranzato 2017) on flat fp32 gradient buckets.
//
//   nvq_gem_gram     the 16 x 16 float64 Gram matrix of the T <= 15 reference rows and the gradient g (index T): one pass
//   nvq_gem_solve    v = argmin 1/2 v'Pv + q'v, v >= margin, with P = R R' + ridge I and q = R g: one workgroup, active set
//   nvq_gem_project  g <- g + R' v, added in double in row order and rounded once
//
// Nothing is read back: "no q_t < 0" leaves v = 0, and the projection returns on v == 0 before g is touched.  The flat-buffer
// rule of flat.h: no atomics, grids that depend on the sizes only, whole quads per lane in the vector and in the scalar form
// alike, sums in double in a fixed order: the same bits on every call and at every pointer alignment.
#include "flat.h"

namespace nvq {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GEM_ROWS = 16;          // 15 references and g: the rows of one v_mfma_f64_16x16x4_f64 tile
constexpr int GEM_MAX_T = GEM_ROWS - 1;
constexpr int GEM_U = 4;              // groups of 4 quads per wave and trip
constexpr int GEM_MAX_ITER = 64;      // Cholesky solves of the active-set method

// stats slots (float64, device)
enum { GS_VIOLATED = 0, GS_ACTIVE = 1, GS_ITER = 2, GS_STATUS = 3, GS_COUNT = 4, GS_GG = 5, GS_GG_AFTER = 6, GS_MIN_COS = 7 };

// ------------------------------------------------------------------ Gram
// The scheme of fed_update_gram_kernel (cluster.hip) with one tile.  A wave takes groups of 4 consecutive quads: lane (lr = lane
// & 15, lk = lane >> 4) fetches quad 4 p + lk of row lr - reference lr for lr < T, g for lr == T, nothing for lr > T - and
// component c of the quads, widened to double, is one k-step: A and B are the same register, the tile gains 4 elements per
// instruction.  Dead lanes (row past T, quad past n / 4) enter as zeros and are not read.  A trip covers GEM_U groups and the
// next trip's quads are fetched before this trip's MFMAs.  The n % 4 last floats are one more k-step in wave 0 of block 0,
// k-lanes 0 .. 2.  The four waves' tiles are added in wave order in LDS; part[block][reg * 64 + lane] holds the block's share.
template <bool VEC>
struct GemFetch {
    float4 x[GEM_U];
    __device__ __forceinline__ void load(const float* __restrict__ row, bool alive, long nq, long p0, int lk) {
#pragma unroll
        for (int u = 0; u < GEM_U; ++u) {
            const long q = 4 * (p0 + u) + lk;
            x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (alive && q < nq) x[u] = ldq<VEC>(row + 4 * q);
        }
    }
};

template <bool VEC>
__global__ __launch_bounds__(256) void gem_gram_kernel(const float* __restrict__ refs, long stride, int T,
                                                       const float* __restrict__ g, long n, double* __restrict__ part) {
    __shared__ double red[256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lk = lane >> 4;
    const bool alive = lr <= T;
    const float* __restrict__ row = lr < T ? refs + lr * stride : g;      // only dereferenced by live lanes

    f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
    const long nq = n >> 2;
    const long ng = (nq + 3) >> 2;
    const long step = (long)gridDim.x * 4 * GEM_U;
    long p0 = (blockIdx.x * 4L + wave) * GEM_U;
    GemFetch<VEC> cur, nxt;
    if (p0 < ng) cur.load(row, alive, nq, p0, lk);
    while (p0 < ng) {
        nxt.load(row, alive, nq, p0 + step, lk);                          // past the end: every lane is dead, nothing is read
#pragma unroll
        for (int u = 0; u < GEM_U; ++u) {
            const double a0 = (double)cur.x[u].x, a1 = (double)cur.x[u].y, a2 = (double)cur.x[u].z, a3 = (double)cur.x[u].w;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, a2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, a3, acc, 0, 0, 0);
        }
        cur = nxt;
        p0 += step;
    }
    if (blockIdx.x == 0 && wave == 0 && (n & 3) != 0) {                   // the n % 4 last floats: element 4 nq + lk, lk < 3
        const long e = 4 * nq + lk;
        const double a = (alive && lk < 3 && e < n) ? (double)row[e] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
    }

    // ((w0 + w1) + w2) + w3, element by element
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int e = reg * 64 + lane;
                red[e] = w == 0 ? acc[reg] : red[e] + acc[reg];
            }
        }
        __syncthreads();
    }
    part[(long)blockIdx.x * 256 + threadIdx.x] = red[threadIdx.x];
}

// grid (16): block x owns the 16 entries x * 16 .. x * 16 + 15.  Thread (entry = threadIdx.x & 15, s = threadIdx.x >> 4) adds the
// blocks s, s + 16, ... in order, then the sixteen strands meet left to right.  Entry e = reg * 64 + lane of the f64 C/D map:
// col = lane & 15, row = (lane >> 4) + 4 reg.  Entries with row <= col are written, to (row, col) and to (col, row): the matrix is
// symmetric bit for bit.  Outside (T + 1) x (T + 1) it is zero, whatever the rows held (0 * NaN of a dead row is not kept).
__global__ __launch_bounds__(256) void gem_gram_final_kernel(const double* __restrict__ part, int nblk, int T, int accumulate,
                                                             double* __restrict__ gram) {
    __shared__ double strand[16][16];
    const int el = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    const double* src = part + e;
    double v = 0.0;
#pragma unroll 8
    for (int b = s; b < nblk; b += 16) v += src[(long)b * 256];
    strand[s][el] = v;
    __syncthreads();
    if (s != 0) return;
    v = strand[0][el];
#pragma unroll
    for (int k = 1; k < 16; ++k) v += strand[k][el];
    const int reg = e >> 6, lane = e & 63;
    const int row = (lane >> 4) + 4 * reg, col = lane & 15;
    if (row > col) return;
    if (col > T) v = 0.0;
    else if (accumulate) v += gram[row * GEM_ROWS + col];
    gram[row * GEM_ROWS + col] = v;
    gram[col * GEM_ROWS + row] = v;
}

// ------------------------------------------------------------------ the quadratic program
// One workgroup; the threads load P, q into LDS and thread 0 runs the active-set method in double.  With u = v - margin >= 0 and
// c = q + margin P 1 the problem is min 1/2 u'Pu + c'u, u >= 0, its multiplier w = P u + c.  Lawson-Hanson: free the bound
// index with the most negative w, solve the free block P_FF s = -c_F by Cholesky; while some free s_i <= 0 step from u towards s
// up to the boundary, bind what reached it, solve again.  Every iterate is feasible, the objective falls strictly with every
// freed index, so no free set returns and the method is finite; GEM_MAX_ITER solves are the cap.
struct GemShared {
    double P[GEM_MAX_T][GEM_MAX_T];
    double L[GEM_MAX_T][GEM_MAX_T];
    double q[GEM_MAX_T], c[GEM_MAX_T], u[GEM_MAX_T], s[GEM_MAX_T], w[GEM_MAX_T], rr[GEM_MAX_T];
    int idx[GEM_MAX_T];
    int bad;
};

// P_FF s_F = -c_F over the free indices sh.idx[0 .. m); false when a pivot is not positive
__device__ bool gem_free_solve(GemShared& sh, int m) {
    for (int j = 0; j < m; ++j) {
        double d = sh.P[sh.idx[j]][sh.idx[j]];
        for (int k = 0; k < j; ++k) d -= sh.L[j][k] * sh.L[j][k];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        sh.L[j][j] = d;
        for (int i = j + 1; i < m; ++i) {
            double a = sh.P[sh.idx[i]][sh.idx[j]];
            for (int k = 0; k < j; ++k) a -= sh.L[i][k] * sh.L[j][k];
            sh.L[i][j] = a / d;
        }
    }
    for (int i = 0; i < m; ++i) {                                         // L y = -c_F
        double a = -sh.c[sh.idx[i]];
        for (int k = 0; k < i; ++k) a -= sh.L[i][k] * sh.s[k];
        sh.s[i] = a / sh.L[i][i];
    }
    for (int i = m - 1; i >= 0; --i) {                                    // L' s = y
        double a = sh.s[i];
        for (int k = i + 1; k < m; ++k) a -= sh.L[k][i] * sh.s[k];
        sh.s[i] = a / sh.L[i][i];
    }
    return true;
}

__global__ __launch_bounds__(64) void gem_solve_kernel(const double* __restrict__ gram, int T, float margin_f, float eps_f,
                                                       int eps_relative, double* __restrict__ v, double* __restrict__ stats) {
    __shared__ GemShared sh;
    const int tid = threadIdx.x;
    if (tid == 0) sh.bad = 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < (T + 1) * (T + 1); e += 64) {
        const int i = e / (T + 1), j = e - i * (T + 1);
        const double x = gram[i * GEM_ROWS + j];
        if (!(fabs(x) <= 1.79769313486231570815e308)) bad = true;          // NaN or infinity
        if (i < T && j < T) sh.P[i][j] = x;
        if (i < T && j == T) sh.q[i] = x;
    }
    if (bad) sh.bad = 1;                                                   // every writer stores the same value
    __syncthreads();
    if (tid != 0) return;
    for (int t = 0; t < GEM_ROWS; ++t) v[t] = 0.0;                         // the result when nothing is to be projected

    const double gg = gram[T * GEM_ROWS + T];
    stats[GS_VIOLATED] = 0.0;
    stats[GS_ACTIVE] = 0.0;
    stats[GS_ITER] = 0.0;
    stats[GS_GG] = gg;
    stats[GS_GG_AFTER] = gg;
    stats[GS_MIN_COS] = 0.0;
    if (sh.bad) {
        stats[GS_STATUS] = 2.0;
        return;
    }
    stats[GS_STATUS] = 0.0;
    if (T == 0) return;

    int violated = 0;
    double min_cos = INFINITY, rr_max = 0.0;
    for (int t = 0; t < T; ++t) {
        violated += sh.q[t] < 0.0;
        const double den = sqrt(gg * sh.P[t][t]);
        const double cs = den > 0.0 ? sh.q[t] / den : 0.0;
        if (cs < min_cos) min_cos = cs;
        if (sh.P[t][t] > rr_max) rr_max = sh.P[t][t];
    }
    stats[GS_VIOLATED] = (double)violated;
    stats[GS_MIN_COS] = min_cos;
    if (violated == 0) return;

    const double margin = (double)margin_f;
    const double ridge = eps_relative ? (double)eps_f * rr_max : (double)eps_f;
    for (int t = 0; t < T; ++t) {
        sh.rr[t] = sh.P[t][t];
        sh.P[t][t] += ridge;
    }
    double cmax = 0.0;
    for (int i = 0; i < T; ++i) {
        double a = 0.0;
        for (int j = 0; j < T; ++j) a += sh.P[i][j];
        sh.c[i] = sh.q[i] + margin * a;
        sh.u[i] = 0.0;
        if (fabs(sh.c[i]) > cmax) cmax = fabs(sh.c[i]);
    }
    const double tol = 1e-13 * cmax;                                      // a multiplier within rounding of 0 is not negative

    unsigned free_mask = 0;
    int iter = 0, status = 0;
    bool running = true;
    while (running) {
        int pick = -1;
        double worst = -tol;
        for (int i = 0; i < T; ++i) {
            if (free_mask >> i & 1) continue;
            double a = sh.c[i];
            for (int j = 0; j < T; ++j) a += sh.P[i][j] * sh.u[j];
            if (a < worst) {
                worst = a;
                pick = i;
            }
        }
        if (pick < 0) break;                                              // w >= 0 on the bound set: the optimum
        free_mask |= 1u << pick;
        for (;;) {
            if (iter == GEM_MAX_ITER) {
                status = 1;
                running = false;
                break;
            }
            int m = 0;
            for (int i = 0; i < T; ++i)
                if (free_mask >> i & 1) sh.idx[m++] = i;
            ++iter;
            if (!gem_free_solve(sh, m)) {                                 // P is positive definite: only rounding gets here
                status = 1;
                running = false;
                break;
            }
            double alpha = 1.0;
            int leave = -1;
            for (int k = 0; k < m; ++k) {
                if (sh.s[k] > 0.0) continue;
                const double ui = sh.u[sh.idx[k]];
                const double a = ui / (ui - sh.s[k]);                     // ui >= 0 >= s: in [0, 1]; ui == 0 == s gives NaN -> 0
                const double al = a >= 0.0 ? a : 0.0;
                if (leave < 0 || al < alpha) {
                    alpha = al;
                    leave = sh.idx[k];
                }
            }
            if (leave < 0) {
                for (int k = 0; k < m; ++k) sh.u[sh.idx[k]] = sh.s[k];
                break;
            }
            for (int k = 0; k < m; ++k) {
                const int i = sh.idx[k];
                const double ui = sh.u[i] + alpha * (sh.s[k] - sh.u[i]);
                sh.u[i] = ui;
                if (i == leave || !(ui > 0.0)) {
                    sh.u[i] = 0.0;
                    free_mask &= ~(1u << i);
                }
            }
            if (free_mask == 0) break;
        }
    }

    int active = 0;
    double lin = 0.0, quad = 0.0;
    for (int i = 0; i < T; ++i) {
        sh.w[i] = sh.u[i] + margin;
        active += sh.u[i] > 0.0;
    }
    for (int i = 0; i < T; ++i) {
        double a = 0.0;
        for (int j = 0; j < T; ++j) a += (i == j ? sh.rr[i] : sh.P[i][j]) * sh.w[j];
        quad += sh.w[i] * a;
        lin += sh.w[i] * sh.q[i];
        v[i] = sh.w[i];
    }
    stats[GS_ACTIVE] = (double)active;
    stats[GS_ITER] = (double)iter;
    stats[GS_STATUS] = (double)status;
    stats[GS_COUNT] += 1.0;
    stats[GS_GG_AFTER] = gg + 2.0 * lin + quad;
}

// ------------------------------------------------------------------ projection
template <bool VEC>
__global__ __launch_bounds__(256) void gem_project_kernel(float* __restrict__ g, const float* __restrict__ refs, long stride,
                                                          int T, long n, const double* __restrict__ v) {
    __shared__ double vs[GEM_MAX_T];
    __shared__ int any;
    if (threadIdx.x == 0) {
        int a = 0;
        for (int t = 0; t < T; ++t) {
            vs[t] = v[t];
            a |= vs[t] != 0.0;
        }
        any = a;
    }
    __syncthreads();
    if (!any) return;                                                      // uniform: an agreeing gradient is never touched
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 a = ldq<VEC>(g + 4 * q);
        double x = a.x, y = a.y, z = a.z, w = a.w;
        for (int t = 0; t < T; ++t) {
            const double vt = vs[t];
            if (vt == 0.0) continue;                                       // uniform: the row is not read
            const float4 b = ldq<VEC>(refs + t * stride + 4 * q);
            x = fma(vt, (double)b.x, x);
            y = fma(vt, (double)b.y, y);
            z = fma(vt, (double)b.z, z);
            w = fma(vt, (double)b.w, w);
        }
        stq<VEC>(g + 4 * q, make_float4((float)x, (float)y, (float)z, (float)w));
    }
    const long e = 4 * nq + threadIdx.x;
    if (flat_tail(n, e)) {
        double x = g[e];
        for (int t = 0; t < T; ++t) {
            const double vt = vs[t];
            if (vt == 0.0) continue;
            x = fma(vt, (double)refs[t * stride + e], x);
        }
        g[e] = (float)x;
    }
}

static int gem_check(const char* what, const float* refs, long stride, int T, const float* g, long n) {
    NVQ_REQUIRE(T >= 0 && T <= GEM_MAX_T, "%s: T = %d outside 0 .. %d", what, T, GEM_MAX_T);
    NVQ_REQUIRE(g != nullptr && n >= 0 && aligned4(g), "%s: g / n", what);
    NVQ_REQUIRE(T == 0 || (refs != nullptr && aligned4(refs) && stride >= n), "%s: refs / stride %ld < n %ld", what, stride, n);
    return NVQ_OK;
}

static bool gem_vec(const float* refs, long stride, int T, const float* g) {
    return aligned16(g) && (T == 0 || (aligned16(refs) && (stride & 3) == 0));
}

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_gem_gram(const float* refs, long stride, int T, const float* g, long n, double* gram, int accumulate, float* workspace,
                 size_t workspace_bytes, void* stream) {
    int rc = gem_check("gem_gram", refs, stride, T, g, n);
    if (rc) return rc;
    NVQ_REQUIRE(T >= 1, "gem_gram: T = %d outside 1 .. %d", T, GEM_MAX_T);
    NVQ_REQUIRE(gram != nullptr && aligned8(gram) && aligned8(workspace), "gem_gram: gram / 8-byte alignment");
    const int nb = flat_blocks(n);
    if (workspace == nullptr || (size_t)nb * 256 * sizeof(double) > workspace_bytes) {
        set_error("gem_gram: workspace");
        return NVQ_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    const dim3 grid(nb), block(256);
    with_bools([&](auto V) { hipLaunchKernelGGL(gem_gram_kernel<V()>, grid, block, 0, s, refs, stride, T, g, n, part); },
               gem_vec(refs, stride, T, g));
    rc = check_launch("gem_gram");
    if (rc) return rc;
    hipLaunchKernelGGL(gem_gram_final_kernel, dim3(16), dim3(256), 0, s, part, nb, T, accumulate, gram);
    return check_launch("gem_gram_final");
}

int nvq_gem_solve(const double* gram, int T, float margin, float eps, int eps_relative, double* v, double* stats, void* stream) {
    NVQ_REQUIRE(gram != nullptr && v != nullptr && stats != nullptr, "gem_solve: null pointer");
    NVQ_REQUIRE(aligned8(gram) && aligned8(v) && aligned8(stats), "gem_solve: 8-byte alignment");
    NVQ_REQUIRE(T >= 0 && T <= GEM_MAX_T, "gem_solve: T = %d outside 0 .. %d", T, GEM_MAX_T);
    NVQ_REQUIRE(margin >= 0.f && eps > 0.f, "gem_solve: margin %g must be >= 0 and eps %g > 0", (double)margin, (double)eps);
    hipLaunchKernelGGL(gem_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gram, T, margin, eps, eps_relative, v, stats);
    return check_launch("gem_solve");
}

int nvq_gem_project(float* g, const float* refs, long stride, int T, long n, const double* v, void* stream) {
    int rc = gem_check("gem_project", refs, stride, T, g, n);
    if (rc) return rc;
    NVQ_REQUIRE(v != nullptr && aligned8(v), "gem_project: v");
    if (T == 0) return NVQ_OK;
    const dim3 grid(flat_blocks(n)), block(256);
    with_bools([&](auto V) { hipLaunchKernelGGL(gem_project_kernel<V()>, grid, block, 0, (hipStream_t)stream, g, refs, stride, T, n, v); },
               gem_vec(refs, stride, T, g));
    return check_launch("gem_project");
}

}  // extern "C"
