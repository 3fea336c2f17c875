// Device-resident episodic memory (nerve_cl.continual.DeviceEpisodicMemory): the slot tables live in HBM, these kernels
// move samples in and out of them and keep the small per-slot tables (importance, time, access count, type id, LR mean).
//
// store / gather: streaming copies, grid (LR chunks + HR chunks, sample): the first chunks_lr workgroups of a sample copy
// its LR tensor, the rest its HR tensor, each tensor with as many chunks as its own length, element type and path need, so
// no workgroup is idle and none straddles two samples or tensors.  A workgroup owns one contiguous chunk of kChunk stored
// 16-byte items (scalar path: kChunk * 4 elements) and issues its loads before its stores.  16 bytes per lane on both
// sides when rows allow it (fp32: row length a multiple of 4 elements, bf16: of 8, bases 16-byte aligned); otherwise the
// guarded scalar path of the same kernel.  bf16 storage rounds to nearest
// even with integer arithmetic (the bits of x.to(torch.bfloat16), subnormals kept, NaN -> 0x7fc0) and widens exactly.
// mean: one workgroup per (channel, sample), double accumulators and a fixed tree: two runs give the same bits.
// sample_weighted / nearest: one workgroup, block arg-max / arg-min in a fixed order, ties to the lower index.
// No atomics and no workspace anywhere; every per-slot word has one owner thread.
#include "common.h"

namespace nvq {

namespace {

constexpr int kItems = 4;                 // 16-byte items per thread
constexpr int kChunk = 256 * kItems;      // per workgroup

__device__ __forceinline__ unsigned short bf16_rne(float x) {
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_widen(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned pack2(float lo, float hi) { return (unsigned)bf16_rne(lo) | ((unsigned)bf16_rne(hi) << 16); }

// src rows [n][per] fp32 -> store row slots[j]
template <bool BF16>
__global__ __launch_bounds__(256) void replay_store_kernel(const float* __restrict__ src_lr, const float* __restrict__ src_hr,
                                                           long lr_per, long hr_per, int vec_lr, int vec_hr, int chunks_lr,
                                                           const int* __restrict__ slots, void* __restrict__ lr_store,
                                                           void* __restrict__ hr_store, int capacity,
                                                           const float* __restrict__ s_imp, const int* __restrict__ s_time,
                                                           const int* __restrict__ s_type, float* __restrict__ importance,
                                                           int* __restrict__ time, int* __restrict__ access,
                                                           int* __restrict__ type_id) {
    const int j = blockIdx.y, hr = (int)blockIdx.x >= chunks_lr;
    const long chunk = hr ? blockIdx.x - chunks_lr : blockIdx.x;
    const int slot = slots[j];
    if ((unsigned)slot >= (unsigned)capacity) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        importance[slot] = s_imp[j];
        time[slot] = s_time[j];
        type_id[slot] = s_type[j];
        access[slot] = 0;
    }
    const long per = hr ? hr_per : lr_per;
    const float* s = (hr ? src_hr : src_lr) + (long)j * per;
    void* store = hr ? hr_store : lr_store;
    const long row = (long)slot * per;
    if (hr ? vec_hr : vec_lr) {
        if (BF16) {
            const long n8 = per >> 3, i0 = chunk * kChunk + threadIdx.x;
            uint4* d = reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(store) + row);
            float4 a[kItems], b[kItems];
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                if (i < n8) { a[q] = ld4(s + 8 * i); b[q] = ld4(s + 8 * i + 4); }
            }
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                if (i < n8) d[i] = make_uint4(pack2(a[q].x, a[q].y), pack2(a[q].z, a[q].w), pack2(b[q].x, b[q].y), pack2(b[q].z, b[q].w));
            }
        } else {
            const long n4 = per >> 2, i0 = chunk * kChunk + threadIdx.x;
            float* d = reinterpret_cast<float*>(store) + row;
            float4 a[kItems];
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                if (i < n4) a[q] = ld4(s + 4 * i);
            }
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                if (i < n4) st4(d + 4 * i, a[q]);
            }
        }
    } else {
        const long e0 = chunk * kChunk * 4;
        for (long i = e0 + threadIdx.x; i < e0 + kChunk * 4 && i < per; i += 256) {
            if (BF16) reinterpret_cast<unsigned short*>(store)[row + i] = bf16_rne(s[i]);
            else reinterpret_cast<float*>(store)[row + i] = s[i];
        }
    }
}

// grid (channels, n): means[slots[j]][c] = mean of plane c of LR sample j, summed in double in a fixed order
template <bool VEC>
__global__ __launch_bounds__(256) void replay_mean_kernel(const float* __restrict__ src_lr, long lr_per, long plane,
                                                          const int* __restrict__ slots, int capacity,
                                                          float* __restrict__ means) {
    __shared__ double scratch[256];
    const int c = blockIdx.x, j = blockIdx.y;
    const int slot = slots[j];
    if ((unsigned)slot >= (unsigned)capacity) return;
    const float* s = src_lr + (long)j * lr_per + (long)c * plane;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (VEC) {
        for (long i = threadIdx.x; i < (plane >> 2); i += 256) {
            const float4 v = ld4(s + 4 * i);
            a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
        }
    } else {
        for (long i = threadIdx.x; i < plane; i += 256) a0 += (double)s[i];
    }
    scratch[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) scratch[threadIdx.x] += scratch[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) means[(long)slot * gridDim.x + c] = (float)(scratch[0] / (double)plane);
}

// store row idx[j] -> rows row0 + j of the fp32 batches; idx[j] < 0 (a draw that found no eligible slot): a row of zeros
template <bool BF16>
__global__ __launch_bounds__(256) void replay_gather_kernel(const void* __restrict__ lr_store, const void* __restrict__ hr_store,
                                                            int capacity, long lr_per, long hr_per, int vec_lr, int vec_hr,
                                                            int chunks_lr, const int* __restrict__ idx, float* __restrict__ lr_batch,
                                                            float* __restrict__ hr_batch, int row0, int* __restrict__ access) {
    const int j = blockIdx.y, hr = (int)blockIdx.x >= chunks_lr;
    const long chunk = hr ? blockIdx.x - chunks_lr : blockIdx.x;
    int slot = idx[j];
    if (slot >= capacity) slot = -1;
    const bool have = slot >= 0;
    if (have && blockIdx.x == 0 && threadIdx.x == 0) access[slot] += 1;
    const long per = hr ? hr_per : lr_per;
    const void* store = hr ? hr_store : lr_store;
    float* d = (hr ? hr_batch : lr_batch) + (long)(row0 + j) * per;
    const long row = have ? (long)slot * per : 0;
    if (hr ? vec_hr : vec_lr) {
        if (BF16) {
            const long n8 = per >> 3, i0 = chunk * kChunk + threadIdx.x;
            const uint4* s = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(store) + row);
            uint4 a[kItems];
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                a[q] = make_uint4(0, 0, 0, 0);
                if (have && i < n8) a[q] = s[i];
            }
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                if (i < n8) {
                    st4(d + 8 * i, make_float4(__uint_as_float(a[q].x << 16), __uint_as_float(a[q].x & 0xffff0000u),
                                               __uint_as_float(a[q].y << 16), __uint_as_float(a[q].y & 0xffff0000u)));
                    st4(d + 8 * i + 4, make_float4(__uint_as_float(a[q].z << 16), __uint_as_float(a[q].z & 0xffff0000u),
                                                   __uint_as_float(a[q].w << 16), __uint_as_float(a[q].w & 0xffff0000u)));
                }
            }
        } else {
            const long n4 = per >> 2, i0 = chunk * kChunk + threadIdx.x;
            const float* s = reinterpret_cast<const float*>(store) + row;
            float4 a[kItems];
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (have && i < n4) a[q] = ld4(s + 4 * i);
            }
#pragma unroll
            for (int q = 0; q < kItems; ++q) {
                const long i = i0 + q * 256L;
                if (i < n4) st4(d + 4 * i, a[q]);
            }
        }
    } else {
        const long e0 = chunk * kChunk * 4;
        for (long i = e0 + threadIdx.x; i < e0 + kChunk * 4 && i < per; i += 256) {
            float v = 0.f;
            if (have) v = BF16 ? bf16_widen(reinterpret_cast<const unsigned short*>(store)[row + i])
                               : reinterpret_cast<const float*>(store)[row + i];
            d[i] = v;
        }
    }
}

constexpr int kWide = 1024;   // threads of the one-workgroup kernels

struct Pick { float key; int idx; };

// a ranks before b: larger key, then lower index (idx < 0 = nothing, ranks last)
__device__ __forceinline__ bool before(Pick a, Pick b) {
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.key > b.key || (a.key == b.key && a.idx < b.idx);
}

// the first Pick in `before` order over the workgroup; valid in every thread.  scratch: kWide / 64 Picks of LDS.
__device__ __forceinline__ Pick block_first(Pick p, Pick* scratch) {
    for (int o = 32; o > 0; o >>= 1) {
        Pick q;
        q.key = __shfl_xor(p.key, o, 64);
        q.idx = __shfl_xor(p.idx, o, 64);
        if (before(q, p)) p = q;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = p;
    __syncthreads();
    Pick best = scratch[0];
    for (int w = 1; w < kWide / 64; ++w)
        if (before(scratch[w], best)) best = scratch[w];
    return best;
}

constexpr int kKeys = 65536 / kWide;   // slots per thread at the largest capacity

// Efraimidis-Spirakis: the k largest keys log(u_i) / w_i over the eligible slots, one round of block arg-max per draw.
// Every thread computes the keys of its (at most kKeys) slots once and keeps them in registers (-inf: not eligible, never
// drawn).  Round r takes the first slot in (key descending, index ascending) order that ranks after round r - 1's pick, so
// no list of the slots already drawn is kept.
__global__ __launch_bounds__(kWide) void replay_sample_kernel(const float* __restrict__ importance, const int* __restrict__ time,
                                                              const int* __restrict__ type_id, int capacity, int now, float rw,
                                                              int type_filter, const float* __restrict__ u, int k,
                                                              int* __restrict__ out) {
    __shared__ Pick scratch[kWide / 64];
    float key[kKeys];
#pragma unroll
    for (int q = 0; q < kKeys; ++q) {
        const int i = q * kWide + threadIdx.x;
        key[q] = -INFINITY;
        if (i < capacity) {
            const int t = type_id[i];
            const float w = (1.f - rw) * importance[i] + rw / (1.f + (float)(now - time[i]));
            const float ui = u[i];
            if (t >= 0 && (type_filter < 0 || t == type_filter) && w > 0.f && ui > 0.f) key[q] = logf(ui) / w;
        }
    }
    Pick prev;
    prev.key = INFINITY;
    prev.idx = -1;
    for (int r = 0; r < k; ++r) {
        Pick mine;
        mine.key = 0.f;
        mine.idx = -1;
        if (r == 0 || prev.idx >= 0) {
#pragma unroll
            for (int q = 0; q < kKeys; ++q) {
                Pick c;
                c.key = key[q];
                c.idx = q * kWide + threadIdx.x;
                if (!(c.key > -INFINITY)) continue;
                if (r > 0 && !before(prev, c)) continue;   // drawn in an earlier round
                if (before(c, mine)) mine = c;
            }
        }
        prev = block_first(mine, scratch);
        if (threadIdx.x == 0) out[r] = prev.idx;
    }
}

__global__ __launch_bounds__(256) void replay_update_kernel(float* __restrict__ importance, int capacity,
                                                            const int* __restrict__ idx, const float* __restrict__ value, int k,
                                                            float m) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const int i = idx[j];
    const float v = value[j];
    if ((unsigned)i >= (unsigned)capacity || !isfinite(v)) return;
    // two products and one sum, each rounded (no fused multiply-add): the arithmetic a caller can write out
    importance[i] = __fadd_rn(__fmul_rn(m, importance[i]), __fmul_rn(1.f - m, v));
}

// arg-min over the valid slots of |table[i] - query| (Euclidean over `channels`), or of table[i] itself without a query
__global__ __launch_bounds__(kWide) void replay_nearest_kernel(const float* __restrict__ query, const float* __restrict__ table,
                                                               const int* __restrict__ type_id, int capacity, int channels,
                                                               int* __restrict__ out_idx, float* __restrict__ out_dist) {
    __shared__ Pick scratch[kWide / 64];
    Pick mine;
    mine.key = 0.f;
    mine.idx = -1;
    for (int i = threadIdx.x; i < capacity; i += kWide) {
        if (type_id[i] < 0) continue;
        float d;
        if (query) {
            float s = 0.f;
            for (int c = 0; c < channels; ++c) {
                const float e = table[(long)i * channels + c] - query[c];
                s = fmaf(e, e, s);
            }
            d = sqrtf(s);
        } else {
            d = table[i];
        }
        if (d != d) continue;
        Pick c;
        c.key = -d;
        c.idx = i;
        if (before(c, mine)) mine = c;
    }
    const Pick best = block_first(mine, scratch);
    if (threadIdx.x == 0) {
        *out_idx = best.idx;
        *out_dist = best.idx >= 0 ? -best.key : INFINITY;
    }
}

// workgroups one tensor of one sample needs: kChunk items of 16 stored bytes (vector path) or kChunk * 4 elements (scalar)
long copy_chunks(long per, int vec, int bf16) { return (per + (long)kChunk * (vec && bf16 ? 8 : 4) - 1) / ((long)kChunk * (vec && bf16 ? 8 : 4)); }

bool vec_ok(const void* a, const void* b, long per, int bf16) { return aligned16(a) && aligned16(b) && per % (bf16 ? 8 : 4) == 0; }

}  // namespace

}  // namespace nvq

using namespace nvq;

extern "C" {

int nvq_replay_store(const float* src_lr, const float* src_hr, int n, long lr_per, long hr_per, int channels,
                     const int* slots, const float* sample_importance, const int* sample_time, const int* sample_type,
                     void* lr_store, void* hr_store, int store_bf16, int capacity, float* means, float* importance,
                     int* time, int* access_count, int* type_id, int flags, void* stream) {
    NVQ_REQUIRE(n > 0 && n <= 65535 && capacity > 0 && capacity <= 65536 && lr_per > 0 && hr_per > 0 && channels > 0 &&
                    channels <= 65535 && lr_per % channels == 0,
                "replay_store: 0 < n <= 65535, 0 < capacity <= 65536, per > 0, lr_per a multiple of channels");
    NVQ_REQUIRE((flags & ~NVQ_REPLAY_MEANS_ONLY) == 0 && src_lr && slots && means, "replay_store: flags / NULL argument");
    NVQ_REQUIRE(((uintptr_t)src_lr & 3) == 0 && ((uintptr_t)src_hr & 3) == 0 && ((uintptr_t)lr_store & (store_bf16 ? 1 : 3)) == 0 &&
                    ((uintptr_t)hr_store & (store_bf16 ? 1 : 3)) == 0, "replay_store: element-aligned tensors");
    hipStream_t s = (hipStream_t)stream;
    if (!(flags & NVQ_REPLAY_MEANS_ONLY)) {
        NVQ_REQUIRE(src_hr && lr_store && hr_store && sample_importance && sample_time && sample_type && importance && time &&
                        access_count && type_id, "replay_store: NULL argument");
        const int vl = vec_ok(src_lr, lr_store, lr_per, store_bf16), vh = vec_ok(src_hr, hr_store, hr_per, store_bf16);
        const long cl = copy_chunks(lr_per, vl, store_bf16), chunks = cl + copy_chunks(hr_per, vh, store_bf16);
        NVQ_REQUIRE(chunks <= 0x7fffffffL, "replay_store: sample too large");
        const dim3 grid((unsigned)chunks, n);
        if (store_bf16)
            hipLaunchKernelGGL(replay_store_kernel<true>, grid, dim3(256), 0, s, src_lr, src_hr, lr_per, hr_per, vl, vh, (int)cl, slots,
                               lr_store, hr_store, capacity, sample_importance, sample_time, sample_type, importance, time,
                               access_count, type_id);
        else
            hipLaunchKernelGGL(replay_store_kernel<false>, grid, dim3(256), 0, s, src_lr, src_hr, lr_per, hr_per, vl, vh, (int)cl, slots,
                               lr_store, hr_store, capacity, sample_importance, sample_time, sample_type, importance, time,
                               access_count, type_id);
        int rc = check_launch("replay_store");
        if (rc) return rc;
    }
    const long plane = lr_per / channels;
    if (aligned16(src_lr) && (plane & 3) == 0)
        hipLaunchKernelGGL(replay_mean_kernel<true>, dim3(channels, n), dim3(256), 0, s, src_lr, lr_per, plane, slots, capacity, means);
    else
        hipLaunchKernelGGL(replay_mean_kernel<false>, dim3(channels, n), dim3(256), 0, s, src_lr, lr_per, plane, slots, capacity, means);
    return check_launch("replay_mean");
}

int nvq_replay_gather(const void* lr_store, const void* hr_store, int store_bf16, int capacity, long lr_per, long hr_per,
                      const int* idx, int k, float* lr_batch, float* hr_batch, int row0, int* access_count, void* stream) {
    NVQ_REQUIRE(k > 0 && k <= 65535 && capacity > 0 && capacity <= 65536 && lr_per > 0 && hr_per > 0 && row0 >= 0,
                "replay_gather: 0 < k <= 65535, 0 < capacity <= 65536, per > 0, row0 >= 0");
    NVQ_REQUIRE(lr_store && hr_store && idx && lr_batch && hr_batch && access_count, "replay_gather: NULL argument");
    NVQ_REQUIRE(((uintptr_t)lr_batch & 3) == 0 && ((uintptr_t)hr_batch & 3) == 0 && ((uintptr_t)lr_store & (store_bf16 ? 1 : 3)) == 0 &&
                    ((uintptr_t)hr_store & (store_bf16 ? 1 : 3)) == 0, "replay_gather: element-aligned tensors");
    // (row0 * per keeps a 16-byte aligned batch base aligned whenever the row length allows the vector path)
    const int vl = vec_ok(lr_store, lr_batch, lr_per, store_bf16), vh = vec_ok(hr_store, hr_batch, hr_per, store_bf16);
    const long cl = copy_chunks(lr_per, vl, store_bf16), chunks = cl + copy_chunks(hr_per, vh, store_bf16);
    NVQ_REQUIRE(chunks <= 0x7fffffffL, "replay_gather: sample too large");
    const dim3 grid((unsigned)chunks, k);
    hipStream_t s = (hipStream_t)stream;
    if (store_bf16)
        hipLaunchKernelGGL(replay_gather_kernel<true>, grid, dim3(256), 0, s, lr_store, hr_store, capacity, lr_per, hr_per, vl, vh,
                           (int)cl, idx, lr_batch, hr_batch, row0, access_count);
    else
        hipLaunchKernelGGL(replay_gather_kernel<false>, grid, dim3(256), 0, s, lr_store, hr_store, capacity, lr_per, hr_per, vl, vh,
                           (int)cl, idx, lr_batch, hr_batch, row0, access_count);
    return check_launch("replay_gather");
}

int nvq_replay_sample_weighted(const float* importance, const int* time, const int* type_id, int capacity, int now,
                               float recency_weight, int type_filter, const float* uniforms, int k, int* out_idx,
                               void* stream) {
    NVQ_REQUIRE(capacity > 0 && capacity <= 65536 && k > 0 && k <= 256, "replay_sample_weighted: 0 < capacity <= 65536, 0 < k <= 256");
    NVQ_REQUIRE(importance && time && type_id && uniforms && out_idx && recency_weight >= 0.f && recency_weight <= 1.f,
                "replay_sample_weighted: NULL argument or recency_weight outside [0, 1]");
    hipLaunchKernelGGL(replay_sample_kernel, dim3(1), dim3(kWide), 0, (hipStream_t)stream, importance, time, type_id, capacity,
                       now, recency_weight, type_filter, uniforms, k, out_idx);
    return check_launch("replay_sample_weighted");
}

int nvq_replay_update_importance(float* importance, int capacity, const int* idx, const float* value, int k, float momentum,
                                 void* stream) {
    NVQ_REQUIRE(capacity > 0 && capacity <= 65536 && k > 0 && importance && idx && value,
                "replay_update_importance: 0 < capacity <= 65536, k > 0, non-NULL tensors");
    hipLaunchKernelGGL(replay_update_kernel, dim3(ceil_div(k, 256)), dim3(256), 0, (hipStream_t)stream, importance, capacity, idx,
                       value, k, momentum);
    return check_launch("replay_update_importance");
}

int nvq_replay_nearest(const float* query, const float* table, const int* type_id, int capacity, int channels, int* out_idx,
                       float* out_dist, void* stream) {
    NVQ_REQUIRE(capacity > 0 && capacity <= 65536 && channels > 0 && table && type_id && out_idx && out_dist,
                "replay_nearest: 0 < capacity <= 65536, channels > 0, non-NULL tensors");
    NVQ_REQUIRE(query || channels == 1, "replay_nearest: without a query the table has one value per slot");
    hipLaunchKernelGGL(replay_nearest_kernel, dim3(1), dim3(kWide), 0, (hipStream_t)stream, query, table, type_id, capacity,
                       channels, out_idx, out_dist);
    return check_launch("replay_nearest");
}

}  // extern "C"
