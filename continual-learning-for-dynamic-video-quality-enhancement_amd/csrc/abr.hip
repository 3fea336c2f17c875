// The ABR agent on the device (include/nvq.h "ABR agent"): the vectorised streaming environment (one thread
// per environment, float64, the reference's order of operations, no contraction), the actor-critic forward with inverse-CDF
// sampling in one launch on the exact-fp32 MFMA, the GAE scan and the clipped-surrogate loss with its gradient.  No atomics
// anywhere: every sum is taken in double in a fixed order, so each result is the same bits on every call.
#include "flat.h"
#include "philox.h"

namespace nvq {

constexpr int ABR_MAX_Q = 16;        // quality levels of the ladder
constexpr int ABR_STATE = 8;         // doubles per environment
constexpr int ABR_OBS = 7;
constexpr int ACT_ROWS = 16;         // observation rows per workgroup: one MFMA M tile
constexpr int ACT_MAX_OUT = 32;      // head outputs including the value
constexpr int ACT_MAX_HEADS = 4;
constexpr int ACT_MAX_LAYERS = 3;
constexpr int ACT_HO_LD = ACT_MAX_OUT + 1;
constexpr int PPO_MAX_OUT = 64;

struct EnvCfg {
    int bitrate[ABR_MAX_Q];
    int nq, enh_levels, max_steps;
};

// the four uniforms of (environment e, draw counter t) on `stream`, u = ((w >> 8) + 0.5) 2^-24, exact in double
__device__ __forceinline__ void abr_words(long e, long t, unsigned stream, long seed, unsigned r[4]) {
    philox4x32_10((unsigned)e, (unsigned)((unsigned long)e >> 32), (unsigned)t,
                  ((unsigned)((unsigned long)t >> 32) & 0xFFFFFFu) | (stream << 24), (unsigned)seed,
                  (unsigned)((unsigned long)seed >> 32), r);
}
__device__ __forceinline__ double abr_u(unsigned w) { return ((double)(w >> 8) + 0.5) * 0x1p-24; }

__device__ __forceinline__ void env_obs(const double* s, double cx, double buffer_size, const EnvCfg& c, float* obs) {
#pragma clang fp contract(off)
    const double bw = s[1] / 20.0;
    obs[0] = (float)(s[0] / buffer_size);
    obs[1] = (float)(bw < 1.0 ? bw : 1.0);
    obs[2] = (float)s[2];
    obs[3] = (float)(s[3] / (double)c.nq);
    obs[4] = (float)(s[4] / 100.0);
    obs[5] = (float)cx;
    obs[6] = (float)(s[5] / (double)c.max_steps);
}

__device__ __forceinline__ void env_fresh(double* s, double bw0) {
    s[0] = 10.0; s[1] = bw0; s[2] = 1.0; s[3] = 2.0; s[4] = 70.0; s[5] = 0.0; s[6] = 0.0; s[7] = 0.0;
}

__global__ __launch_bounds__(256) void abr_env_reset_kernel(double* __restrict__ state, long* __restrict__ counters,
                                                            float* __restrict__ obs, const double* __restrict__ params, EnvCfg c,
                                                            long seed, int N) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const long t = counters[e];
    unsigned r[4];
    abr_words(e, t, 0u, seed, r);
    double s[ABR_STATE];
    env_fresh(s, 2.0 + 13.0 * abr_u(r[2]));
    float o[ABR_OBS];
    env_obs(s, 0.3 + 0.5 * abr_u(r[3]), params[1], c, o);
    for (int i = 0; i < ABR_STATE; ++i) state[(long)e * ABR_STATE + i] = s[i];
    for (int i = 0; i < ABR_OBS; ++i) obs[(long)e * ABR_OBS + i] = o[i];
    counters[e] = t + 1;
}

__global__ __launch_bounds__(256) void abr_env_step_kernel(double* __restrict__ state, long* __restrict__ counters,
                                                           const int* __restrict__ actions, const double* __restrict__ params,
                                                           EnvCfg c, long seed, int N, float* __restrict__ obs,
                                                           double* __restrict__ reward, unsigned char* __restrict__ terminated,
                                                           unsigned char* __restrict__ truncated, double* __restrict__ info,
                                                           float* __restrict__ reward_f32, float* __restrict__ done_f32,
                                                           double* __restrict__ finished) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    const double seg = params[0], buffer_size = params[1];
    double s[ABR_STATE];
    for (int i = 0; i < ABR_STATE; ++i) s[i] = state[(long)e * ABR_STATE + i];
    const long t = counters[e];
    unsigned r[4];
    abr_words(e, t, 0u, seed, r);

    int q = actions[2 * e], lvl = actions[2 * e + 1];
    q = q < 0 ? 0 : (q >= c.nq ? c.nq - 1 : q);
    lvl = lvl < 0 ? 0 : (lvl >= c.enh_levels ? c.enh_levels - 1 : lvl);
    const double enh = (double)lvl / (double)(c.enh_levels - 1);
    int bitrate = c.bitrate[0];
    for (int i = 1; i < ABR_MAX_Q; ++i) bitrate = i == q ? c.bitrate[i] : bitrate;     // (no dynamic index into the arguments)

    const double chunk = (double)bitrate * seg;
    const double download = chunk / (s[1] * 1000.0);
    const double level = s[0] - download;
    const double rebuffer = -level > 0.0 ? -level : 0.0;
    s[6] = s[6] + rebuffer;
    double lv = (level > 0.0 ? level : 0.0) + seg;
    s[0] = lv < buffer_size ? lv : buffer_size;
    const double base = 50.0 + ((double)q / (double)c.nq) * 40.0;
    const double enhanced = base + enh * 10.0;
    s[4] = enhanced < 100.0 ? enhanced : 100.0;
    const double cost = 0.01 + enh * 0.02;
    const double bat = s[2] - cost;
    s[2] = bat > 0.0 ? bat : 0.0;
    const int dq = q - (int)s[3];
    const double rew = s[4] / 100.0 - rebuffer * 10.0 - (double)(dq < 0 ? -dq : dq) * 0.1 + s[2] * 0.1;
    s[3] = (double)q;
    s[5] = s[5] + 1.0;
    double bw = s[1] * (0.8 + 0.4 * abr_u(r[0]));
    bw = bw > 0.5 ? bw : 0.5;
    s[1] = bw < 50.0 ? bw : 50.0;
    s[7] = s[7] + rew;
    const bool term = s[5] >= (double)c.max_steps, trunc = s[2] <= 0.0;
    const bool done = term || trunc;

    reward[e] = rew;
    terminated[e] = term;
    truncated[e] = trunc;
    if (info != nullptr) {
        info[e] = s[4];
        info[(long)N + e] = rebuffer;
        info[2L * N + e] = s[1];
        info[3L * N + e] = s[0];
        info[4L * N + e] = s[7];
    }
    if (reward_f32 != nullptr) reward_f32[e] = (float)rew;
    if (done_f32 != nullptr) done_f32[e] = done ? 1.f : 0.f;
    double cx = 0.3 + 0.5 * abr_u(r[1]);
    if (done) {
        if (finished != nullptr) {
            finished[2L * e] = finished[2L * e] + s[7];
            finished[2L * e + 1] = finished[2L * e + 1] + 1.0;
        }
        env_fresh(s, 2.0 + 13.0 * abr_u(r[2]));
        cx = 0.3 + 0.5 * abr_u(r[3]);
    }
    float o[ABR_OBS];
    env_obs(s, cx, buffer_size, c, o);
    for (int i = 0; i < ABR_STATE; ++i) state[(long)e * ABR_STATE + i] = s[i];
    for (int i = 0; i < ABR_OBS; ++i) obs[(long)e * ABR_OBS + i] = o[i];
    counters[e] = t + 1;
}

// ---------------------------------------------------------------------------------------------------------------- act
// One workgroup = 16 observation rows (one MFMA M tile), four waves.  The activations of a layer are a [16][LD] fp32 image in LDS
// (two images, in and out); a wave owns output tiles of 16 columns, four at a time so that four accumulator chains are in flight,
// and reads its B operand straight from the nn.Linear weight [out][in] in global memory as one float4 per lane and 16-wide K
// chunk: the weights (280 KB for 7-256-256) stay in L2 for every workgroup and nothing is packed or staged.  Within a chunk lane
// (r, g) holds k = k0 + 4 g + s for MFMA s in A and B alike: a permutation of the chunk's sixteen products.
struct ActArgs {
    const float* obs;
    int B, obs_dim;
    const float* W[ACT_MAX_LAYERS];
    const float* b[ACT_MAX_LAYERS];
    int width[ACT_MAX_LAYERS];
    int nl;
    const float* colW[ACT_MAX_OUT];     // the weight row behind each head output column (the value last), null past P
    const float* colB[ACT_MAX_OUT];
    int hn[ACT_MAX_HEADS];
    int nh, P, LD;
    const long* counters;
    long seed;
    int deterministic;
    int* actions;
    float* log_prob;
    float* value;
    float* head_out;
};

__device__ __forceinline__ float4 act_ldw(const float* row, int k, int in_dim, bool vec) {
    if (row == nullptr) return make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) return ld4(row + k);
    return make_float4(k < in_dim ? row[k] : 0.f, k + 1 < in_dim ? row[k + 1] : 0.f, k + 2 < in_dim ? row[k + 2] : 0.f,
                       k + 3 < in_dim ? row[k + 3] : 0.f);
}

__device__ __forceinline__ f32x4 act_mfma4(float4 a, float4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

__global__ __launch_bounds__(256) void abr_act_kernel(const ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float act_lds[];
    const int LD = a.LD;
    float* cur = act_lds;
    float* nxt = act_lds + ACT_ROWS * LD;
    float* ho = act_lds + 2 * ACT_ROWS * LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long row0 = (long)blockIdx.x * ACT_ROWS;

    for (int i = tid; i < ACT_ROWS * 32; i += 256) {
        const int rr = i >> 5, cc = i & 31;
        cur[rr * LD + cc] = (row0 + rr < a.B && cc < a.obs_dim) ? a.obs[(row0 + rr) * a.obs_dim + cc] : 0.f;
    }
    __syncthreads();

    int K = 32, in_dim = a.obs_dim;
    for (int l = 0; l < a.nl; ++l) {
        const int wout = a.width[l], ntiles = wout >> 4;
        const float* W = a.W[l];
        const float* bias = a.b[l];
        const bool vec = in_dim == K;          // (whole float4s of a 16-byte aligned row: the host checks the tensors)
        for (int t0 = wave; t0 < ntiles; t0 += 16) {
            f32x4 acc[4];
            const float* wrow[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                wrow[q] = t0 + 4 * q < ntiles ? W + (long)((t0 + 4 * q) * 16 + r) * in_dim : nullptr;
            }
            for (int k0 = 0; k0 < K; k0 += 16) {
                const float4 av = ld4(cur + r * LD + k0 + 4 * g);
                float4 bv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) bv[q] = act_ldw(wrow[q], k0 + 4 * g, in_dim, vec);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = act_mfma4(av, bv[q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (t0 + 4 * q < ntiles) {
                    const int col = (t0 + 4 * q) * 16 + r;
                    const float bc = bias[col];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = acc[q][i] + bc;
                        nxt[(4 * g + i) * LD + col] = v > 0.f ? v : 0.f;
                    }
                }
            }
        }
        __syncthreads();
        float* tmp = cur; cur = nxt; nxt = tmp;
        K = in_dim = wout;
    }

    if (wave * 16 < a.P) {                                   // heads: output columns [16 wave, 16 wave + 16)
        const int col = wave * 16 + r;
        const float* wrow = a.colW[col];
        const bool vec = in_dim == K;                        // (nn.Linear rows of a width that is a multiple of 32: 16-byte aligned
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};             //  whenever the tensor is, which the host checks)
        for (int k0 = 0; k0 < K; k0 += 16)
            acc = act_mfma4(ld4(cur + r * LD + k0 + 4 * g), act_ldw(wrow, k0 + 4 * g, in_dim, vec), acc);
        const float bc = wrow != nullptr ? *a.colB[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) ho[(4 * g + i) * ACT_HO_LD + col] = acc[i] + bc;
    }
    __syncthreads();

    const long row = row0 + tid;
    if (tid < ACT_ROWS && row < a.B) {
        const float* x = ho + tid * ACT_HO_LD;
        const bool det = a.deterministic || a.counters == nullptr;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (!det) abr_words(row, a.counters[row], 1u, a.seed, w);
        int off = 0;
        float lp_sum = 0.f;
        for (int j = 0; j < a.nh; ++j) {
            const int n = a.hn[j];
            float m = x[off];
            int best = 0;
            for (int k = 1; k < n; ++k)
                if (x[off + k] > m) { m = x[off + k]; best = k; }
            float s = 0.f;
            for (int k = 0; k < n; ++k) s += expf(x[off + k] - m);
            const float lse = m + logf(s);
            int pick = best;
            if (!det) {
                const float u = (float)abr_u(w[j]);
                float cdf = 0.f;
                pick = n - 1;
                for (int k = 0; k < n; ++k) {
                    cdf += expf(x[off + k] - lse);
                    if (u < cdf) { pick = k; break; }
                }
            }
            lp_sum += x[off + pick] - lse;
            a.actions[row * a.nh + j] = pick;
            off += n;
        }
        a.log_prob[row] = lp_sum;
        a.value[row] = x[off];
        if (a.head_out != nullptr)
            for (int k = 0; k < a.P; ++k) a.head_out[row * a.P + k] = x[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- GAE
__global__ __launch_bounds__(256) void abr_gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values,
                                                      const float* __restrict__ dones, const float* __restrict__ last_values,
                                                      float gamma, float lam, int T, int N, float* __restrict__ returns,
                                                      float* __restrict__ advantages) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    float gae = 0.f, next = last_values[e];
    for (int t = T - 1; t >= 0; --t) {
        const long i = (long)t * N + e;
        const float nd = 1.f - dones[i], v = values[i];
        const float delta = rewards[i] + gamma * next * nd - v;
        gae = delta + gamma * lam * nd * gae;
        advantages[i] = gae;
        returns[i] = gae + v;
        next = v;
    }
}

// stats = {mean, unbiased standard deviation} of adv[0 .. M), two passes in double, one workgroup: thread t adds elements
// t, t + 256, ... in order, then block_wave_sum_256
__global__ __launch_bounds__(256) void abr_adv_stats_kernel(const float* __restrict__ adv, long M, double* __restrict__ stats) {
    __shared__ double scratch[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < M; i += 256) s += (double)adv[i];
    block_wave_sum_256(scratch, s);
    const double mean = s / (double)M;
    double q = 0.0;
    for (long i = threadIdx.x; i < M; i += 256) {
        const double d = (double)adv[i] - mean;
        q += d * d;
    }
    block_wave_sum_256(scratch, q);
    if (threadIdx.x == 0) {
        stats[0] = mean;
        stats[1] = sqrt(q / (double)(M - 1));
    }
}

// ---------------------------------------------------------------------------------------------------------------- PPO loss
struct PpoCfg {
    int hn[ACT_MAX_HEADS];
    int nh, P;
    double clip, value_coef, entropy_coef;
};

constexpr int PPO_SUMS = 5;          // policy surrogate, squared value error, entropy, approximate KL, clipped count

// One thread per sample, everything per sample in double (about 3 P exponentials: nothing next to the network's GEMMs), the
// gradient rounded once to fp32.  part[b * 5 + i]: the block's five sums.
__global__ __launch_bounds__(256) void ppo_loss_kernel(const float* __restrict__ x, const int* __restrict__ actions,
                                                       const float* __restrict__ old_lp, const float* __restrict__ adv,
                                                       const double* __restrict__ adv_stats, const float* __restrict__ returns,
                                                       long M, PpoCfg c, float* __restrict__ grad, double* __restrict__ part) {
    __shared__ double scratch[4 * PPO_SUMS];
    const double mean = adv_stats[0], denom = adv_stats[1] + 1e-8, invM = 1.0 / (double)M;
    double s_pol = 0.0, s_val = 0.0, s_ent = 0.0, s_kl = 0.0, s_clip = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long)gridDim.x * 256) {
        const float* xi = x + i * c.P;
        float* gi = grad + i * c.P;
        double lse[ACT_MAX_HEADS], ent[ACT_MAX_HEADS];
        double new_lp = 0.0;
        int off = 0;
#pragma unroll
        for (int j = 0; j < ACT_MAX_HEADS; ++j) {
            if (j < c.nh) {
                const int n = c.hn[j];
                double m = (double)xi[off];
                for (int k = 1; k < n; ++k) m = fmax(m, (double)xi[off + k]);
                double s = 0.0;
                for (int k = 0; k < n; ++k) s += exp((double)xi[off + k] - m);
                lse[j] = m + log(s);
                double h = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double lp = (double)xi[off + k] - lse[j];
                    h -= exp(lp) * lp;
                }
                ent[j] = h;
                s_ent += h;
                const int act = min(max(actions[i * c.nh + j], 0), n - 1);
                new_lp += (double)xi[off + act] - lse[j];
                off += n;
            }
        }
        const double A = ((double)adv[i] - mean) / denom;
        const double lr = new_lp - (double)old_lp[i];
        const double ratio = exp(lr);
        const double clipped = fmin(fmax(ratio, 1.0 - c.clip), 1.0 + c.clip);
        const double s1 = ratio * A, s2 = clipped * A;
        s_pol += fmin(s1, s2);
        // d min(s1, s2) / d new_lp: s1's branch (A ratio) when it is the smaller one or the two coincide (ratio inside the clip
        // range, where clamp passes the gradient); the clamped branch is constant
        const double dlp = (s1 <= s2) ? -A * ratio * invM : 0.0;
        const double verr = (double)xi[off] - (double)returns[i];
        s_val += verr * verr;
        s_kl += (ratio - 1.0) - lr;
        s_clip += fabs(ratio - 1.0) > c.clip ? 1.0 : 0.0;
        off = 0;
#pragma unroll
        for (int j = 0; j < ACT_MAX_HEADS; ++j) {
            if (j < c.nh) {
                const int n = c.hn[j], act = min(max(actions[i * c.nh + j], 0), n - 1);
                for (int k = 0; k < n; ++k) {
                    const double lp = (double)xi[off + k] - lse[j], p = exp(lp);
                    gi[off + k] = (float)(dlp * ((k == act ? 1.0 : 0.0) - p) + c.entropy_coef * invM * p * (lp + ent[j]));
                }
                off += n;
            }
        }
        gi[off] = (float)(2.0 * c.value_coef * invM * verr);
    }
    block_wave_sum_256(scratch, s_pol, s_val, s_ent, s_kl, s_clip);
    if (threadIdx.x == 0) {
        double* p = part + (long)blockIdx.x * PPO_SUMS;
        p[0] = s_pol; p[1] = s_val; p[2] = s_ent; p[3] = s_kl; p[4] = s_clip;
    }
}

// out = {loss, policy loss, value loss, entropy, approximate KL, clip fraction}: the blocks' sums added in index order
__global__ void ppo_loss_final_kernel(const double* __restrict__ part, int nb, long M, PpoCfg c, double* __restrict__ out) {
    __shared__ double sums[PPO_SUMS];
    if (threadIdx.x < PPO_SUMS) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += part[(long)b * PPO_SUMS + threadIdx.x];
        sums[threadIdx.x] = s / (double)M;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double pol = -sums[0];
        out[0] = pol + c.value_coef * sums[1] - c.entropy_coef * sums[2];
        out[1] = pol; out[2] = sums[1]; out[3] = sums[2]; out[4] = sums[3]; out[5] = sums[4];
    }
}

inline int ppo_blocks(long M) {
    int nb = ceil_div(M, 256L);
    if (nb > 1024) nb = 1024;
    return nb < 1 ? 1 : nb;
}

}  // namespace nvq

using namespace nvq;

static int env_cfg(EnvCfg& c, const int* bitrates_host, int nq, int enh_levels, int max_steps, const char* what) {
    NVQ_REQUIRE(nq >= 1 && nq <= ABR_MAX_Q, "%s: %d quality levels outside 1 .. %d", what, nq, ABR_MAX_Q);
    NVQ_REQUIRE(enh_levels >= 2 && max_steps >= 1, "%s: enh_levels = %d / max_steps = %d", what, enh_levels, max_steps);
    for (int i = 0; i < ABR_MAX_Q; ++i) c.bitrate[i] = bitrates_host != nullptr && i < nq ? bitrates_host[i] : 0;
    c.nq = nq;
    c.enh_levels = enh_levels;
    c.max_steps = max_steps;
    return NVQ_OK;
}

extern "C" {

int nvq_abr_env_reset(double* state, long* counters, float* obs, const double* params, int nq, int max_steps, long seed, int N,
                      void* stream) {
    NVQ_REQUIRE(state != nullptr && counters != nullptr && obs != nullptr && params != nullptr, "abr_env_reset: null pointer");
    NVQ_REQUIRE(N >= 1 && seed >= 0, "abr_env_reset: N = %d, seed = %ld", N, seed);
    NVQ_REQUIRE(aligned8(state) && aligned8(counters) && aligned8(params) && aligned4(obs), "abr_env_reset: alignment");
    EnvCfg c;
    int rc = env_cfg(c, nullptr, nq, 2, max_steps, "abr_env_reset");
    if (rc) return rc;
    hipLaunchKernelGGL(abr_env_reset_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, state, counters, obs, params,
                       c, seed, N);
    return check_launch("abr_env_reset");
}

int nvq_abr_env_step(double* state, long* counters, const int* actions, const int* bitrates_host, int nq, int enh_levels,
                     int max_steps, const double* params, long seed, int N, float* obs, double* reward,
                     unsigned char* terminated, unsigned char* truncated, double* info, float* reward_f32, float* done_f32,
                     double* finished, void* stream) {
    NVQ_REQUIRE(state != nullptr && counters != nullptr && actions != nullptr && bitrates_host != nullptr && params != nullptr &&
                    obs != nullptr && reward != nullptr && terminated != nullptr && truncated != nullptr,
                "abr_env_step: null pointer");
    NVQ_REQUIRE(N >= 1 && seed >= 0, "abr_env_step: N = %d, seed = %ld", N, seed);
    NVQ_REQUIRE(aligned8(state) && aligned8(counters) && aligned8(params) && aligned8(reward) && aligned8(info) &&
                    aligned8(finished) && aligned4(actions) && aligned4(obs) && aligned4(reward_f32) && aligned4(done_f32),
                "abr_env_step: alignment");
    EnvCfg c;
    int rc = env_cfg(c, bitrates_host, nq, enh_levels, max_steps, "abr_env_step");
    if (rc) return rc;
    hipLaunchKernelGGL(abr_env_step_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, state, counters, actions,
                       params, c, seed, N, obs, reward, terminated, truncated, info, reward_f32, done_f32, finished);
    return check_launch("abr_env_step");
}

int nvq_abr_act_supported(int obs_dim, const int* dims_host) {
    if (dims_host == nullptr || obs_dim < 1 || obs_dim > 32) return 0;
    const int nl = dims_host[0], nh = dims_host[1 + ACT_MAX_LAYERS];
    if (nl < 1 || nl > ACT_MAX_LAYERS || nh < 1 || nh > ACT_MAX_HEADS) return 0;
    for (int l = 0; l < nl; ++l) {
        const int w = dims_host[1 + l];
        if (w < 32 || w > 512 || (w & 31)) return 0;
    }
    int P = 1;
    for (int j = 0; j < nh; ++j) {
        const int n = dims_host[2 + ACT_MAX_LAYERS + j];
        if (n < 1) return 0;
        P += n;
    }
    return P <= ACT_MAX_OUT;
}

int nvq_abr_act(const float* obs, int B, int obs_dim, const void* params_host, const int* dims_host, const long* counters,
                long seed, int deterministic, int* actions, float* log_prob, float* value, float* head_out, void* stream) {
    NVQ_REQUIRE(obs != nullptr && params_host != nullptr && dims_host != nullptr && actions != nullptr && log_prob != nullptr &&
                    value != nullptr, "abr_act: null pointer");
    NVQ_REQUIRE(B >= 1 && seed >= 0, "abr_act: B = %d, seed = %ld", B, seed);
    NVQ_REQUIRE(nvq_abr_act_supported(obs_dim, dims_host),
                "abr_act: unsupported network (obs_dim <= 32, 1 .. 3 hidden layers of a width % 32 == 0 in [32, 512], <= 4 heads, "
                "<= 32 head outputs with the value)");
    NVQ_REQUIRE(aligned4(obs) && aligned8(counters) && aligned4(actions) && aligned4(log_prob) && aligned4(value) && aligned4(head_out),
                "abr_act: alignment");
    const float* const* pp = reinterpret_cast<const float* const*>(params_host);
    ActArgs a;
    a.obs = obs; a.B = B; a.obs_dim = obs_dim;
    a.nl = dims_host[0];
    a.nh = dims_host[1 + ACT_MAX_LAYERS];
    int maxw = 32;
    for (int l = 0; l < ACT_MAX_LAYERS; ++l) {
        a.W[l] = l < a.nl ? pp[2 * l] : nullptr;
        a.b[l] = l < a.nl ? pp[2 * l + 1] : nullptr;
        a.width[l] = l < a.nl ? dims_host[1 + l] : 0;
        if (l < a.nl) {
            NVQ_REQUIRE(a.W[l] != nullptr && a.b[l] != nullptr && aligned16(a.W[l]) && aligned4(a.b[l]), "abr_act: layer %d weights", l);
            if (a.width[l] > maxw) maxw = a.width[l];
        }
    }
    const int last = a.width[a.nl - 1];
    for (int k = 0; k < ACT_MAX_OUT; ++k) a.colW[k] = a.colB[k] = nullptr;
    int col = 0;
    for (int j = 0; j <= a.nh; ++j) {                         // j == nh: the value head
        const int n = j < a.nh ? dims_host[2 + ACT_MAX_LAYERS + j] : 1;
        const int slot = j < a.nh ? j : ACT_MAX_HEADS;
        const float* W = pp[2 * ACT_MAX_LAYERS + 2 * slot];
        const float* bias = pp[2 * ACT_MAX_LAYERS + 2 * slot + 1];
        NVQ_REQUIRE(W != nullptr && bias != nullptr && aligned16(W) && aligned4(bias), "abr_act: head %d weights", j);
        if (j < a.nh) a.hn[j] = n;
        for (int k = 0; k < n; ++k, ++col) {
            a.colW[col] = W + (long)k * last;
            a.colB[col] = bias + k;
        }
    }
    for (int j = a.nh; j < ACT_MAX_HEADS; ++j) a.hn[j] = 0;
    a.P = col;
    a.LD = maxw + 4;
    a.counters = counters; a.seed = seed; a.deterministic = deterministic;
    a.actions = actions; a.log_prob = log_prob; a.value = value; a.head_out = head_out;
    const size_t lds = (size_t)(2 * ACT_ROWS * a.LD + ACT_ROWS * ACT_HO_LD) * sizeof(float);
    if (lds > 48 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(abr_act_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
            (void)hipGetLastError();
            set_error("abr_act: %zu bytes of LDS refused", lds);
            return NVQ_ELAUNCH;
        }
    }
    hipLaunchKernelGGL(abr_act_kernel, dim3(ceil_div(B, ACT_ROWS)), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch("abr_act");
}

int nvq_abr_gae(const float* rewards, const float* values, const float* dones, const float* last_values, float gamma, float lam,
                int T, int N, float* returns, float* advantages, void* stream) {
    NVQ_REQUIRE(rewards != nullptr && values != nullptr && dones != nullptr && last_values != nullptr && returns != nullptr &&
                    advantages != nullptr, "abr_gae: null pointer");
    NVQ_REQUIRE(T >= 1 && N >= 1, "abr_gae: T = %d, N = %d", T, N);
    NVQ_REQUIRE(aligned4(rewards) && aligned4(values) && aligned4(dones) && aligned4(last_values) && aligned4(returns) &&
                    aligned4(advantages), "abr_gae: alignment");
    hipLaunchKernelGGL(abr_gae_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream, rewards, values, dones, last_values,
                       gamma, lam, T, N, returns, advantages);
    return check_launch("abr_gae");
}

int nvq_abr_adv_stats(const float* adv, long M, double* stats, void* stream) {
    NVQ_REQUIRE(adv != nullptr && stats != nullptr && M >= 1, "abr_adv_stats: adv / stats / M");
    NVQ_REQUIRE(aligned4(adv) && aligned8(stats), "abr_adv_stats: alignment");
    hipLaunchKernelGGL(abr_adv_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, adv, M, stats);
    return check_launch("abr_adv_stats");
}

size_t nvq_ppo_loss_workspace_bytes(long M) {
    return M < 1 ? 0 : (size_t)ppo_blocks(M) * PPO_SUMS * sizeof(double);
}

int nvq_ppo_loss(const float* head_outputs, const int* actions, const float* old_log_probs, const float* advantages,
                 const double* adv_stats, const float* returns, long M, const int* heads_host, int n_heads, float clip_ratio,
                 float value_coef, float entropy_coef, float* grad, double* out, double* workspace, size_t workspace_bytes,
                 void* stream) {
    NVQ_REQUIRE(head_outputs != nullptr && actions != nullptr && old_log_probs != nullptr && advantages != nullptr &&
                    adv_stats != nullptr && returns != nullptr && heads_host != nullptr && grad != nullptr && out != nullptr,
                "ppo_loss: null pointer");
    NVQ_REQUIRE(M >= 1 && n_heads >= 1 && n_heads <= ACT_MAX_HEADS, "ppo_loss: M = %ld, %d heads (1 .. %d)", M, n_heads, ACT_MAX_HEADS);
    PpoCfg c;
    c.nh = n_heads;
    c.P = 1;
    for (int j = 0; j < ACT_MAX_HEADS; ++j) {
        c.hn[j] = j < n_heads ? heads_host[j] : 0;
        NVQ_REQUIRE(j >= n_heads || c.hn[j] >= 1, "ppo_loss: head %d has %d outputs", j, c.hn[j]);
        c.P += c.hn[j];
    }
    NVQ_REQUIRE(c.P <= PPO_MAX_OUT, "ppo_loss: %d head outputs with the value, at most %d", c.P, PPO_MAX_OUT);
    NVQ_REQUIRE(aligned4(head_outputs) && aligned4(actions) && aligned4(old_log_probs) && aligned4(advantages) && aligned8(adv_stats) &&
                    aligned4(returns) && aligned4(grad) && aligned8(out) && aligned8(workspace), "ppo_loss: alignment");
    if (workspace == nullptr || nvq_ppo_loss_workspace_bytes(M) > workspace_bytes) {
        set_error("ppo_loss: workspace");
        return NVQ_EWORKSPACE;
    }
    c.clip = (double)clip_ratio;
    c.value_coef = (double)value_coef;
    c.entropy_coef = (double)entropy_coef;
    const int nb = ppo_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_loss_kernel, dim3(nb), dim3(256), 0, s, head_outputs, actions, old_log_probs, advantages, adv_stats, returns,
                       M, c, grad, workspace);
    int rc = check_launch("ppo_loss");
    if (rc) return rc;
    hipLaunchKernelGGL(ppo_loss_final_kernel, dim3(1), dim3(64), 0, s, workspace, nb, M, c, out);
    return check_launch("ppo_loss_final");
}

}  // extern "C"
