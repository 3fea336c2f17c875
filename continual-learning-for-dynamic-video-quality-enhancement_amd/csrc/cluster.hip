// Clustered federated learning on the client matrix.
//
//   nvq_fed_update_gram         G[i][j] = (x_i - base).(x_j - base) for the K rows of a client matrix: one pass, fp64 MFMA
//   nvq_cluster_gram_kmeans     Lloyd's algorithm in the update space from G alone (kernel k-means), one workgroup
//   nvq_fed_aggregate_clusters  out[c] = base_c + lr * sum_{k in S_c} c_k (x_k - base_c) (+ noise): C models in one pass
//
// The flat-buffer rule of flat.h: no atomics, grids that depend on the sizes only, whole quads per lane in the vector and in
// the scalar form alike, sums in double in a fixed order: the same bits on every call and at every pointer alignment.
#include "fed.h"

namespace nvq {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int CLUSTER_MAX = 8;

__host__ __device__ constexpr int gram_tiles(int T) { return T * (T + 1) / 2; }

// ------------------------------------------------------------------ update Gram
// A wave takes groups of 4 consecutive quads (16 floats): lane (lr = lane & 15, lk = lane >> 4) fetches quad 4 p + lk of the
// rows 16 i + lr, i < T, and widens (x - base) to double.  Component c of the quads is one k-step of v_mfma_f64_16x16x4_f64:
// A[row lr][k lk] = u_{16 i + lr}[4 (4 p + lk) + c], B the same register of row tile j, so tile (i, j) of the partial Gram
// gains 4 elements per instruction.  Only the tiles i <= j are kept (a diagonal tile multiplies a register by itself).  Rows
// past K and quads past n / 4 enter as zeros.  A trip covers U = 4 / T groups (T = 1, 2) or one, and the next trip's quads are
// fetched before this trip's MFMAs, so several loads per lane are in flight while the matrix cores work.  The n % 4 last
// floats are one more k-step in wave 0 of block 0, k-lanes 0 .. 2.  The four waves' tiles are added in wave order in LDS;
// part[block][tile][reg * 64 + lane] holds the block's share.
template <bool VEC, bool HAS_BASE, int T, int U>
struct GramFetch {
    float4 b[U];
    float4 x[U][T];
    // the quads of the groups p0 .. p0 + U - 1; a dead lane (row past K, quad past nq) holds x = b, so x - b = 0
    __device__ __forceinline__ void load(const float* __restrict__ clients, long stride, int K, const float* __restrict__ base,
                                         long nq, long p0, int lr, int lk) {
#pragma unroll
        for (int g = 0; g < U; ++g) {
            const long q = 4 * (p0 + g) + lk;
            const bool in = q < nq;
            b[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (HAS_BASE && in) b[g] = ldq<VEC>(base + 4 * q);
#pragma unroll
            for (int i = 0; i < T; ++i) {
                const int r = 16 * i + lr;
                x[g][i] = b[g];
                if (in && r < K) x[g][i] = ldq<VEC>(clients + r * stride + 4 * q);
            }
        }
    }
};

template <bool VEC, bool HAS_BASE, int T>
__global__ __launch_bounds__(256) void fed_update_gram_kernel(const float* __restrict__ clients, long stride, int K,
                                                              const float* __restrict__ base, long n, double* __restrict__ part) {
    constexpr int NT = gram_tiles(T);
    constexpr int U = T == 1 ? 4 : (T == 2 ? 2 : 1);
    __shared__ double red[NT * 256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lr = lane & 15, lk = lane >> 4;

    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};

    const long nq = n >> 2;
    const long ng = (nq + 3) >> 2;
    const long step = (long)gridDim.x * 4 * U;
    long p0 = (blockIdx.x * 4L + wave) * U;
    GramFetch<VEC, HAS_BASE, T, U> cur, nxt;
    if (p0 < ng) cur.load(clients, stride, K, base, nq, p0, lr, lk);
    while (p0 < ng) {
        nxt.load(clients, stride, K, base, nq, p0 + step, lr, lk);     // past the end: every lane is dead, nothing is read
#pragma unroll
        for (int g = 0; g < U; ++g) {
            double u[T][4];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                u[i][0] = (double)cur.x[g][i].x - (double)cur.b[g].x;
                u[i][1] = (double)cur.x[g][i].y - (double)cur.b[g].y;
                u[i][2] = (double)cur.x[g][i].z - (double)cur.b[g].z;
                u[i][3] = (double)cur.x[g][i].w - (double)cur.b[g].w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                int t = 0;
#pragma unroll
                for (int i = 0; i < T; ++i)
#pragma unroll
                    for (int j = i; j < T; ++j, ++t)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[i][c], u[j][c], acc[t], 0, 0, 0);
            }
        }
        cur = nxt;
        p0 += step;
    }
    if (blockIdx.x == 0 && wave == 0 && (n & 3) != 0) {                // the n % 4 last floats: element 4 nq + lk, lk < 3
        const long e = 4 * nq + lk;
        const bool in = lk < 3 && e < n;
        const float b = (HAS_BASE && in) ? base[e] : 0.f;
        double u[T];
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const int r = 16 * i + lr;
            const float x = (in && r < K) ? clients[r * stride + e] : b;
            u[i] = (double)x - (double)b;
        }
        int t = 0;
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = i; j < T; ++j, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[i], u[j], acc[t], 0, 0, 0);
    }

    // ((w0 + w1) + w2) + w3, element by element
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int e = t * 256 + reg * 64 + lane;
                    red[e] = w == 0 ? acc[t][reg] : red[e] + acc[t][reg];
                }
        }
        __syncthreads();
    }
    double* dst = part + (long)blockIdx.x * (NT * 256);
    for (int e = threadIdx.x; e < NT * 256; e += 256) dst[e] = red[e];
}

// grid (16, tiles): block (x, t) owns the 16 entries x * 16 .. x * 16 + 15 of tile t.  Thread (entry = threadIdx.x & 15, s =
// threadIdx.x >> 4) adds the blocks s, s + 16, ... in order, then the sixteen strands meet left to right.  Entry e = reg * 64 +
// lane of the f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg.  Entries with global row <= col are written, to (row, col)
// and to (col, row): G is symmetric bit for bit.
__global__ __launch_bounds__(256) void fed_update_gram_final_kernel(const double* __restrict__ part, int nblk, int K, int T,
                                                                    double* __restrict__ gram) {
    __shared__ double strand[16][16];
    const int t = blockIdx.y, NT = gram_tiles(T);
    const int el = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    const double* src = part + (long)t * 256 + e;
    double v = 0.0;
#pragma unroll 8
    for (int b = s; b < nblk; b += 16) v += src[(long)b * (NT * 256)];
    strand[s][el] = v;
    __syncthreads();
    if (s != 0) return;
    v = strand[0][el];
#pragma unroll
    for (int k = 1; k < 16; ++k) v += strand[k][el];
    int ti = 0, rem = t;
    while (rem >= T - ti) {
        rem -= T - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int reg = e >> 6, lane = e & 63;
    const int row = 16 * ti + (lane >> 4) + 4 * reg, col = 16 * tj + (lane & 15);
    if (row <= col && col < K) {
        gram[row * K + col] = v;
        gram[col * K + row] = v;
    }
}

// ------------------------------------------------------------------ kernel k-means on the Gram
// One workgroup.  With S_c the members of cluster c, A[k][c] = sum_{j in S_c} G[k][j] (j ascending) and B[c] = sum_{i in S_c}
// A[i][c] (i ascending), d(k, c) = G[k][k] - (2 / |S_c|) A[k][c] + B[c] / |S_c|^2, +inf for an empty cluster.
struct KMeansShared {
    double G[64 * 64];
    double A[64 * CLUSTER_MAX];
    double B[CLUSTER_MAX];
    double mind[64];
    int labels[64];
    int counts[CLUSTER_MAX];
    int seeds[CLUSTER_MAX];
    int changed;
};

__device__ __forceinline__ void kmeans_stats(KMeansShared& sh, int K, int C) {
    __syncthreads();
    if ((int)threadIdx.x < C) {
        int m = 0;
        for (int k = 0; k < K; ++k) m += sh.labels[k] == (int)threadIdx.x;
        sh.counts[threadIdx.x] = m;
    }
    for (int e = threadIdx.x; e < K * C; e += 256) {
        const int k = e / C, c = e - k * C;
        double a = 0.0;
        for (int j = 0; j < K; ++j)
            if (sh.labels[j] == c) a += sh.G[k * K + j];
        sh.A[k * CLUSTER_MAX + c] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        double b = 0.0;
        for (int i = 0; i < K; ++i)
            if (sh.labels[i] == c) b += sh.A[i * CLUSTER_MAX + c];
        sh.B[c] = b;
    }
    __syncthreads();
}

__device__ __forceinline__ double kmeans_dist(const KMeansShared& sh, int K, int k, int c) {
    const int m = sh.counts[c];
    if (m == 0) return INFINITY;
    const double dm = (double)m;
    return sh.G[k * K + k] - (2.0 / dm) * sh.A[k * CLUSTER_MAX + c] + sh.B[c] / (dm * dm);
}

__global__ __launch_bounds__(256) void cluster_gram_kmeans_kernel(const double* __restrict__ gram, int K, int C,
                                                                  const int* __restrict__ init, int max_iter,
                                                                  int* __restrict__ labels, int* __restrict__ counts,
                                                                  double* __restrict__ inertia, int* __restrict__ n_iter) {
    __shared__ KMeansShared sh;
    const int tid = threadIdx.x;
    for (int e = tid; e < K * K; e += 256) sh.G[e] = gram[e];
    if (tid < C) sh.seeds[tid] = init ? init[tid] : -1;
    __syncthreads();

    if (init == nullptr) {                                             // farthest-first, ties to the lowest index
        if (tid == 0) {
            int best = 0;
            for (int k = 1; k < K; ++k)
                if (sh.G[k * K + k] > sh.G[best * K + best]) best = k;
            sh.seeds[0] = best;
        }
        if (tid < K) sh.mind[tid] = INFINITY;
        __syncthreads();
        for (int c = 1; c < C; ++c) {
            if (tid < K) {
                const int s = sh.seeds[c - 1];
                const double d = sh.G[tid * K + tid] - 2.0 * sh.G[tid * K + s] + sh.G[s * K + s];
                if (d < sh.mind[tid]) sh.mind[tid] = d;
            }
            __syncthreads();
            if (tid == 0) {
                int best = 0;
                for (int k = 1; k < K; ++k)
                    if (sh.mind[k] > sh.mind[best]) best = k;
                sh.seeds[c] = best;
            }
            __syncthreads();
        }
    }

    // the seed assignment: the nearest seed row, ties to the lowest cluster; a seed outside [0, K) is an empty cluster
    if (tid < K) {
        int best = 0;
        double bd = INFINITY;
        for (int c = 0; c < C; ++c) {
            const int s = sh.seeds[c];
            if (s < 0 || s >= K) continue;
            const double d = sh.G[tid * K + tid] - 2.0 * sh.G[tid * K + s] + sh.G[s * K + s];
            if (d < bd) {
                bd = d;
                best = c;
            }
        }
        sh.labels[tid] = best;
    }

    int it = 0;
    while (it < max_iter) {
        kmeans_stats(sh, K, C);
        if (tid == 0) sh.changed = 0;
        __syncthreads();
        if (tid < K) {
            int best = 0;
            double bd = INFINITY;
            for (int c = 0; c < C; ++c) {
                const double d = kmeans_dist(sh, K, tid, c);
                if (d < bd) {
                    bd = d;
                    best = c;
                }
            }
            if (best != sh.labels[tid]) {
                sh.labels[tid] = best;
                sh.changed = 1;                                        // every writer stores the same value
            }
        }
        ++it;
        __syncthreads();
        if (sh.changed == 0) break;                                    // uniform; kmeans_stats' first barrier precedes the next clear
    }

    kmeans_stats(sh, K, C);
    if (tid < K) labels[tid] = sh.labels[tid];
    if (tid < C) counts[tid] = sh.counts[tid];
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += kmeans_dist(sh, K, k, sh.labels[k]);
        inertia[0] = s;
        n_iter[0] = it;
    }
}

// ------------------------------------------------------------------ one model per cluster
// order[start[c] .. start[c + 1]) = the members of cluster c in ascending k; per quad the clusters are taken in turn, each
// the fed_mean_quad / fed_mean_tail (fed.h) of its members, so every client row is read once and C rows are written.
template <bool VEC, bool HAS_BASE, bool NOISE>
__global__ __launch_bounds__(256) void fed_aggregate_clusters_kernel(const float* __restrict__ clients, long stride, int K,
                                                                     const int* __restrict__ labels, int C, const float* bases,
                                                                     long base_stride, const double* __restrict__ weights,
                                                                     const double* __restrict__ sq, float clip_norm,
                                                                     float server_lr, float noise_std, long seed, long offset,
                                                                     long n, float* out, long out_stride) {
    __shared__ double coef[64];
    __shared__ int lab[64], order[64], start[CLUSTER_MAX + 1];
    const int tid = threadIdx.x;
    if (tid < K) {
        const int l = labels[tid];
        lab[tid] = (l >= 0 && l < C) ? l : -1;
    }
    __syncthreads();
    if (tid < K && lab[tid] >= 0) {
        const int l = lab[tid];
        int before = 0, rank = 0;
        double W = 0.0;
        for (int k = 0; k < K; ++k) {
            before += lab[k] >= 0 && lab[k] < l;
            rank += k < tid && lab[k] == l;
            if (lab[k] == l) W += weights[k];
        }
        order[before + rank] = tid;
        coef[tid] = weights[tid] / W * fed_clip(sq, tid, clip_norm);
    }
    if (tid <= C) {
        int m = 0;
        for (int k = 0; k < K; ++k) m += lab[k] >= 0 && lab[k] < tid;
        start[tid] = m;
    }
    __syncthreads();

    const auto row = [&](int m) { return order[m]; };
    const double lr = (double)server_lr;
    const long nq = n >> 2;
    for (long q = blockIdx.x * 256L + tid; q < nq; q += (long)gridDim.x * 256) {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (HAS_BASE && base_stride == 0) b = ldq<VEC>(bases + 4 * q);  // a shared base: once, before any row is written
        for (int c = 0; c < C; ++c) {
            if (HAS_BASE && base_stride != 0) b = ldq<VEC>(bases + c * base_stride + 4 * q);
            stq<VEC>(out + c * out_stride + 4 * q, fed_mean_quad<VEC, NOISE>(clients, stride, q, b, coef, row, start[c], start[c + 1],
                                                                              lr, noise_std, seed, offset + c));
        }
    }
    const long t = 4 * nq + tid;
    if (flat_tail(n, t)) {
        float b = (HAS_BASE && base_stride == 0) ? bases[t] : 0.f;
        for (int c = 0; c < C; ++c) {
            if (HAS_BASE && base_stride != 0) b = bases[c * base_stride + t];
            out[c * out_stride + t] = fed_mean_tail<NOISE>(clients, stride, t, nq, b, coef, row, start[c], start[c + 1], lr,
                                                           noise_std, seed, offset + c);
        }
    }
}

}  // namespace nvq

using namespace nvq;

extern "C" {

size_t nvq_fed_gram_workspace_bytes(int K, long n) {
    if (K < 1 || K > 64 || n < 0) return 0;
    return (size_t)flat_blocks(n) * (size_t)gram_tiles(ceil_div(K, 16)) * 256 * sizeof(double);
}

int nvq_fed_update_gram(const float* clients, long stride, int K, const float* base, long n, double* gram, float* workspace,
                        size_t workspace_bytes, void* stream) {
    int rc = fed_check("fed_update_gram", clients, stride, K, n);
    if (rc) return rc;
    NVQ_REQUIRE(gram != nullptr && aligned8(gram) && aligned8(workspace), "fed_update_gram: gram / 8-byte alignment");
    const int nb = flat_blocks(n), T = ceil_div(K, 16);
    if (workspace == nullptr || nvq_fed_gram_workspace_bytes(K, n) > workspace_bytes) {
        set_error("fed_update_gram: workspace");
        return NVQ_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(workspace);
    const bool vec = fed_vec(clients, stride, base);
    const dim3 grid(nb), block(256);
    with_bools([&](auto V, auto B) {
        const auto kernel = T == 1   ? fed_update_gram_kernel<V(), B(), 1>
                            : T == 2 ? fed_update_gram_kernel<V(), B(), 2>
                            : T == 3 ? fed_update_gram_kernel<V(), B(), 3>
                                     : fed_update_gram_kernel<V(), B(), 4>;
        hipLaunchKernelGGL(kernel, grid, block, 0, s, clients, stride, K, base, n, part);
    }, vec, base != nullptr);
    rc = check_launch("fed_update_gram");
    if (rc) return rc;
    hipLaunchKernelGGL(fed_update_gram_final_kernel, dim3(16, gram_tiles(T)), dim3(256), 0, s, part, nb, K, T, gram);
    return check_launch("fed_update_gram_final");
}

int nvq_cluster_gram_kmeans(const double* gram, int K, int C, const int* init, int max_iter, int* labels, int* counts,
                            double* inertia, int* n_iter, void* stream) {
    NVQ_REQUIRE(gram != nullptr && labels != nullptr && counts != nullptr && inertia != nullptr && n_iter != nullptr,
                "cluster_gram_kmeans: null pointer");
    NVQ_REQUIRE(K >= 1 && K <= 64, "cluster_gram_kmeans: K = %d outside 1 .. 64", K);
    NVQ_REQUIRE(C >= 1 && C <= CLUSTER_MAX && C <= K, "cluster_gram_kmeans: C = %d outside 1 .. min(%d, K = %d)", C, CLUSTER_MAX, K);
    NVQ_REQUIRE(max_iter >= 0, "cluster_gram_kmeans: max_iter = %d", max_iter);
    NVQ_REQUIRE(aligned8(gram) && aligned8(inertia) && aligned4(init) && aligned4(labels) && aligned4(counts) && aligned4(n_iter),
                "cluster_gram_kmeans: alignment");
    hipLaunchKernelGGL(cluster_gram_kmeans_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, gram, K, C, init, max_iter, labels,
                       counts, inertia, n_iter);
    return check_launch("cluster_gram_kmeans");
}

int nvq_fed_aggregate_clusters(const float* clients, long stride, int K, const int* labels, int C, const float* bases,
                               long base_stride, const double* weights, const double* sq, float clip_norm, float server_lr,
                               float noise_std, long seed, long offset, long n, float* out, long out_stride, void* stream) {
    int rc = fed_check("fed_aggregate_clusters", clients, stride, K, n, seed, offset, noise_std);
    if (rc) return rc;
    NVQ_REQUIRE(labels != nullptr && weights != nullptr && out != nullptr, "fed_aggregate_clusters: labels / weights / out");
    NVQ_REQUIRE(C >= 1 && C <= CLUSTER_MAX, "fed_aggregate_clusters: C = %d outside 1 .. %d", C, CLUSTER_MAX);
    NVQ_REQUIRE(out_stride >= n, "fed_aggregate_clusters: out_stride %ld < n %ld", out_stride, n);
    NVQ_REQUIRE(base_stride == 0 || (bases != nullptr && base_stride >= n), "fed_aggregate_clusters: base_stride %ld", base_stride);
    NVQ_REQUIRE(sq == nullptr || clip_norm >= 0.f, "fed_aggregate_clusters: clip_norm");
    NVQ_REQUIRE(sq == nullptr || base_stride == 0, "fed_aggregate_clusters: clipping needs one shared base");
    NVQ_REQUIRE(bases == nullptr || base_stride != 0 || C == 1 || out != bases,
                "fed_aggregate_clusters: out may be bases only with one base per cluster");
    NVQ_REQUIRE(out != bases || C == 1 || out_stride == base_stride, "fed_aggregate_clusters: in place needs out_stride == base_stride");
    NVQ_REQUIRE(aligned8(weights) && aligned8(sq) && aligned4(labels), "fed_aggregate_clusters: table alignment");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = fed_vec(clients, stride, bases, out) && (base_stride & 3) == 0 && (out_stride & 3) == 0;
    const dim3 grid(flat_blocks(n)), block(256);
    with_bools([&](auto V, auto B, auto N) {
        hipLaunchKernelGGL((fed_aggregate_clusters_kernel<V(), B(), N()>), grid, block, 0, s, clients, stride, K, labels, C, bases,
                           base_stride, weights, sq, clip_norm, server_lr, noise_std, seed, offset, n, out, out_stride);
    }, vec, bases != nullptr, noise_std != 0.f);
    return check_launch("fed_aggregate_clusters");
}

}  // extern "C"
