// What the fold-in kernels share (foldin.hip: tgcn_foldin_two_layer; foldin_levels.hip: tgcn_foldin_levels): a document's
// scalars, the 4-column row accesses of a lane, the wave-local LDS sync, the u W2 epilogue and the launch (launch_fold).
// Both kernels run THIS code, so a document's deg_d, dis_d, a_j, a_dd and its level-1 sums carry the same bits in either.
// The pass over a document's words is NOT here: each kernel spells its own out (one body for both measured slower in
// either kernel).
#pragma once

#include <algorithm>
#include <atomic>
#include <climits>

#include "common.h"

namespace tgcn {
namespace fold {

constexpr int kFoldWaves = TGCN_FOLDIN_DOCS_PER_WORKGROUP;
constexpr int kFoldMaxH = 256;      // 64 lanes x 4 columns
constexpr int kFoldMaxC = 128;      // W2 at 256 x 128 fp32 = 128 KiB of the 160 KiB of LDS, 24 KiB for the waves' slices
static_assert(kFoldWaves * 64 <= 1024, "one workgroup");

__device__ __forceinline__ int lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float lane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// columns c0 .. c0+3 of a row of n columns: zeros beyond n; a 16-byte load where the four exist
template <bool TAIL>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int c0, int n) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 + 4 <= n) {
        v = *reinterpret_cast<const float4 *>(row + c0);
    } else if (TAIL && c0 < n) {
        v.x = row[c0];
        if (c0 + 1 < n) v.y = row[c0 + 1];
        if (c0 + 2 < n) v.z = row[c0 + 2];
    }
    return v;
}

template <bool TAIL>
__device__ __forceinline__ void store4(float *__restrict__ row, int c0, int n, const float4 v) {
    if (c0 + 4 <= n) {
        *reinterpret_cast<float4 *>(row + c0) = v;
    } else if (TAIL && c0 < n) {
        row[c0] = v.x;
        if (c0 + 1 < n) row[c0 + 1] = v.y;
        if (c0 + 2 < n) row[c0 + 2] = v.z;
    }
}

__device__ __forceinline__ void fma4(float4 &acc, const float a, const float4 x) {
    acc.x = fmaf(a, x.x, acc.x);
    acc.y = fmaf(a, x.y, acc.y);
    acc.z = fmaf(a, x.z, acc.z);
    acc.w = fmaf(a, x.w, acc.w);
}

__device__ __forceinline__ float act1(const float v, const int act) {
    return (act == TGCN_ACT_RELU && v < 0.f) ? 0.f : v;       // a NaN goes through, as torch.relu does
}

// act(v + b), column by column
__device__ __forceinline__ float4 bias_act4(const float4 v, const float4 b, const int act) {
    return make_float4(act1(v.x + b.x, act), act1(v.y + b.y, act), act1(v.z + b.z, act), act1(v.w + b.w, act));
}

// deg_d and from it dis_d, in the plan's own rules (plan.hip: k_deg_sum_seq / k_deg_sum_f64, k_deg_finish)
__device__ __forceinline__ float doc_dis(const float *__restrict__ val, const int64_t beg, const int64_t end, const int lane,
                                         const int reference) {
#pragma clang fp contract(off)
    float deg;
    if (reference) {
        float s = 0.f;
        for (int64_t b = beg; b < end; b += 64) {
            const float v = b + lane < end ? val[b + lane] : 0.f;
            const int cnt = static_cast<int>(min(int64_t(64), end - b));
            for (int i = 0; i < cnt; ++i) s += lane_f(v, i);
        }
        deg = s + 1.0f;
    } else {
        double s = 0.0;
        for (int64_t j = beg + lane; j < end; j += 64) s += static_cast<double>(val[j]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        deg = static_cast<float>(s + 1.0);
    }
    float d = 1.0f / sqrtf(deg);
    if (isinf(d)) d = 0.0f;
    return d;
}

// a_dd = dis_d * dis_d, the self loop's weight 1.0 between them as gcn_norm multiplies it
__device__ __forceinline__ float doc_self_weight(const float dd) {
#pragma clang fp contract(off)
    return (dd * 1.0f) * dd;
}

// This lane's entry b + lane of the row [.., end): its column id (-1: none, or outside [0, n_vocab)) and its a_j
__device__ __forceinline__ void doc_entry(const int32_t *__restrict__ col, const float *__restrict__ val,
                                          const float *__restrict__ dis, const int n_vocab, const int64_t b, const int64_t end,
                                          const int lane, const float dd, const int reference, int &c, float &a) {
#pragma clang fp contract(off)
    c = -1;
    a = 0.f;
    if (b + lane < end) {
        const int cj = col[b + lane];
        const float t = val[b + lane];
        if (cj >= 0 && cj < n_vocab) {
            const float dw = dis[cj];
            a = reference ? (dw * t) * dd : t * (dw * dd);
            c = cj;
        }
    }
}

// A wave's LDS slice belongs to that wave alone: its LDS operations run in order, so a wave-local fence and barrier stand
// between the slice's stores and the loads that follow them
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// y = u W2 for the columns `lane` (y0) and, WIDE, `lane + 64` (y1): u [h] in the wave's LDS slice, w0 / w1 point at the
// lane's column of the tight [h, C] copy of W2 in LDS; k = 0 .. h-1 in order, one FMA per term
template <bool WIDE>
__device__ __forceinline__ void u_times_w2(const float *__restrict__ us, const float *__restrict__ w0,
                                           const float *__restrict__ w1, const int h, const int C, float &y0, float &y1) {
    y0 = 0.f;
    y1 = 0.f;
    int k = 0;
#pragma unroll 2
    for (; k + 4 <= h; k += 4) {
        const float4 uu = *reinterpret_cast<const float4 *>(us + k);
        const float *r0 = w0 + k * C;
        y0 = fmaf(uu.x, r0[0], y0);
        y0 = fmaf(uu.y, r0[C], y0);
        y0 = fmaf(uu.z, r0[2 * C], y0);
        y0 = fmaf(uu.w, r0[3 * C], y0);
        if (WIDE) {
            const float *r1 = w1 + k * C;
            y1 = fmaf(uu.x, r1[0], y1);
            y1 = fmaf(uu.y, r1[C], y1);
            y1 = fmaf(uu.z, r1[2 * C], y1);
            y1 = fmaf(uu.w, r1[3 * C], y1);
        }
    }
    for (; k < h; ++k) {
        const float uk = us[k];
        y0 = fmaf(uk, w0[k * C], y0);
        if (WIDE) y1 = fmaf(uk, w1[k * C], y1);
    }
}

// The row maximum over the lanes' z0 / z1 (-inf where a lane holds no column) and the first column that holds it, as
// tgcn_masked_ce_pred breaks ties (0 for a row without one: all NaN)
__device__ __forceinline__ int first_argmax(const float z0, const float z1, const bool on0, const bool on1, const int lane,
                                            float &m) {
    m = fmaxf(z0, z1);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    int bi = INT_MAX;
    if (on0 && z0 == m)
        bi = lane;
    else if (on1 && z1 == m)
        bi = lane + 64;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bi = min(bi, __shfl_xor(bi, off, 64));
    return bi == INT_MAX ? 0 : bi;
}

inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// The launch of a fold-in leaf `Kernel` (one wave per document, grid-stride, at most TGCN_FOLDIN_WORKGROUP_CAP workgroups)
// with `lds_bytes` of dynamic LDS.  The leaf's LDS ceiling is raised to `lds_ceiling` once per device, not per launch: the
// call is host work on a path whose cost is the host's (a device ordinal beyond the table asks every time).
template <auto Kernel, class Args>
int launch_fold(const Args &A, int64_t n_docs, int lds_ceiling, size_t lds_bytes, hipStream_t s) {
    static std::atomic<bool> raised[64] = {};            // (one table per kernel symbol)
    int dev = -1;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (!known || !raised[dev].load(std::memory_order_acquire)) {
        TGCN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           lds_ceiling));
        if (known) raised[dev].store(true, std::memory_order_release);
    }
    const int grid =
        static_cast<int>(std::min<int64_t>((n_docs + kFoldWaves - 1) / kFoldWaves, int64_t(TGCN_FOLDIN_WORKGROUP_CAP)));
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(64 * kFoldWaves), lds_bytes, s, A);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // namespace fold
}  // namespace tgcn
