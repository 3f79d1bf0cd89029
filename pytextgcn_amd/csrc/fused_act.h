// What the fused-activation products (embed.hip; mlp.hip and mlp_grouped.hip through mlp_products.h) and the other
// matrix-core kernels of the model layers (jk.hip, hier.hip's entry points) share: the accumulator map of
// v_mfma_f32_32x32x2_f32, SELU, the dropout decision of one element, the argument checks of the entry points, the cut of a
// reduction into slices and the sum over the slices (reduce_slices: the body of k_reduce_slices and of k_gmlp_reduce_w).
// Everything here is inline, a template or in an unnamed namespace: a translation unit holds a copy of what it uses.
#pragma once

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "drop_hash.h"

namespace tgcn {

// v_mfma_f32_32x32x2_f32 (exact fp32), the fragment maps as in dense.hip: lane l feeds A[l & 31][l >> 5] and
// B[l >> 5][l & 31]; register r of lane l is C[acc_row(r, l >> 5)][l & 31].
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// torch's constants (aten/src/ATen/native/Activation.cpp: selu)
constexpr float kSeluScale = 1.0507009873554805f;
constexpr float kSeluNeg = static_cast<float>(1.0507009873554805 * 1.6732632423543772);   // scale * alpha

__device__ __forceinline__ float selu_f(float x) { return x > 0.f ? kSeluScale * x : kSeluNeg * expm1f(x); }
__device__ __forceinline__ float selu_grad_f(float x) { return x > 0.f ? kSeluScale : kSeluNeg * expf(x); }

// The dropout of a row-indexed activation: keep(i, col) is the decision of tgcn_gemm_*_dropout (drop_hash.h) for mask row
// i + row0 and column col.
struct RowDrop {
    const uint64_t *seed;  // device pointer (read by the kernels: safe under HIP-graph capture)
    uint32_t thresh;       // keep iff hash >= thresh
    float scale;           // 1 / (1 - p)
    int64_t row0;          // row i is mask row i + row0
};

template <bool DROP>
__device__ __forceinline__ uint32_t row_key(const RowDrop &d, int64_t i) {
    if constexpr (DROP) {
        const uint64_t seed = *d.seed;
        return drop_row_key(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), i + d.row0);
    }
    return 0u;
}

// s * keep * selu(z); `key` is the row's key, `col_term` the column's term of the hash
template <bool DROP>
__device__ __forceinline__ float act(float z, uint32_t key, uint32_t col_term, const RowDrop &d) {
    const float a = selu_f(z);
    if constexpr (DROP) return drop_hash_keep(key, col_term, d.thresh) ? a * d.scale : 0.f;
    return a;
}

// A bias that depends on the ROW (tgcn_mlp_act_linear_cls*): row i carries S <= 2 ids into a small table T [Fh, k], and the
// pre-activation of (i, j) is ((Z[i, j] + T[cls[i, 0], j]) + T[cls[i, 1], j]) + b[j].  An id outside [0, Fh) selects nothing.
// The table is read through the caches, where its at most Fh lines of a 32-column chunk stay; the products without the
// term (CLS false) compile to what they were.
constexpr int kClassRowsMax = 128;   // the cap on Fh (tgcn_hier_max_features has the same)

struct ClassTerm {
    const int32_t *cls;   // [N, S], row stride ldcls
    int64_t ldcls;
    const float *T;       // [Fh, k], row stride ldt
    int64_t ldt;
    int S, Fh;
};

// the ids of row i: -1 where the row selects nothing
template <bool CLS>
__device__ __forceinline__ void class_ids(const ClassTerm &t, int64_t i, bool live, int32_t &id0, int32_t &id1) {
    id0 = id1 = -1;
    if constexpr (CLS) {
        if (live) {
            const int32_t *row = t.cls + i * t.ldcls;
            const int32_t a = row[0], b = t.S > 1 ? row[1] : -1;
            id0 = (a >= 0 && a < t.Fh) ? a : -1;
            id1 = (b >= 0 && b < t.Fh) ? b : -1;
        }
    }
}

// (z + T[id0, j]) + T[id1, j]; j < k is the caller's.  Without a branch (in an unrolled loop over a lane's rows the
// compiler would keep one exec mask per row alive): an id of -1 loads from row 0, which exists, and the sum is dropped,
// so z comes back as it was, its bits untouched.
template <bool CLS>
__device__ __forceinline__ float plus_class_rows(float z, const ClassTerm &t, int32_t id0, int32_t id1, int j) {
    if constexpr (CLS) {
        const float t0 = t.T[(id0 < 0 ? 0 : id0) * t.ldt + j];
        z = id0 < 0 ? z : z + t0;
        if (t.S > 1) {                                     // (uniform)
            const float t1 = t.T[(id1 < 0 ? 0 : id1) * t.ldt + j];
            z = id1 < 0 ? z : z + t1;
        }
    }
    return z;
}

// two ids in one register (Fh <= 128): what a lane that keeps the ids of 16 rows holds
__device__ __forceinline__ uint32_t pack_ids(int32_t id0, int32_t id1) {
    return (static_cast<uint32_t>(id0) & 0xffffu) | (static_cast<uint32_t>(id1) << 16);
}
__device__ __forceinline__ int32_t packed_id(uint32_t both, int slot) {
    return static_cast<int16_t>(slot ? both >> 16 : both & 0xffffu);
}

inline int make_row_drop(const char *fn, double p, const uint64_t *seed, int64_t mask_row0, RowDrop &d, bool &on) {
    if (!(p >= 0.0 && p < 1.0)) {
        set_error("%s: p must be in [0, 1) (p=%g)", fn, p);
        return TGCN_E_INVALID;
    }
    if (mask_row0 < 0) {
        set_error("%s: mask_row0 must be >= 0 (%lld)", fn, (long long)mask_row0);
        return TGCN_E_INVALID;
    }
    on = p > 0.0 && seed != nullptr;
    d.seed = seed;
    d.thresh = on ? drop_threshold(p) : 0u;
    d.scale = on ? static_cast<float>(1.0 / (1.0 - p)) : 1.f;
    d.row0 = mask_row0;
    return TGCN_OK;
}

// The argument checks of the entry points, used under TGCN_CHECK.
inline int check_ld(const char *fn, const char *name, int64_t ld, int64_t extent) {
    if (ld < extent) {
        set_error("%s: %s (%lld) is smaller than the extent %lld", fn, name, (long long)ld, (long long)extent);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

inline int check_ptr(const char *fn, const char *name, const void *ptr) {
    if (!ptr) {
        set_error("%s: %s is NULL", fn, name);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

// `k`: how the entry point's signature spells the activation's width ("K" or "k")
inline int check_sizes(const char *fn, const char *k, int64_t N, int K, int n) {
    if (N < 0 || K <= 0 || n <= 0) {
        set_error("%s: need N >= 0, %s >= 1 and n >= 1 (N=%lld, %s=%d, n=%d)", fn, k, (long long)N, k, K, n);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

// f(std::integral_constant<int, T>) for the first T of the ascending ladder TS... with t <= T (the last one when there is
// none): how a launcher picks the instantiation for a run-time tile count
template <int T, int... TS, class F>
inline void with_tiles(int t, F &&f) {
    if constexpr (sizeof...(TS) == 0) {
        f(std::integral_constant<int, T>{});
    } else {
        if (t <= T) f(std::integral_constant<int, T>{});
        else with_tiles<TS...>(t, f);
    }
}

// A reduction over N rows for a result of ceil(K / 32) tiles, cut into slices of whole chunks of kWChunk rows: about
// `target_workgroups` workgroups in all, at most 256 slices.  The slices' partial sums go to a workspace and
// k_reduce_slices adds them in slice order: no atomics, the same bits every run.
constexpr int kWChunk = 128;   // rows per staged tile

inline void grad_w_split(int64_t N, int K, int target_workgroups, int64_t &slices, int64_t &chunks_per_slice) {
    const int64_t chunks = std::max<int64_t>(1, (N + kWChunk - 1) / kWChunk);
    const int64_t ktiles = (int64_t(K) + 31) / 32;
    const int64_t want = std::min<int64_t>(256, std::max<int64_t>(1, target_workgroups / ktiles));
    chunks_per_slice = (chunks + want - 1) / want;
    slices = (chunks + chunks_per_slice - 1) / chunks_per_slice;
}

// How the fused SELU + dropout products of the MLP (mlp.hip, mlp_grouped.hip) cut a wide operand into launches.
constexpr int kFwdGroup = 256;   // result columns of one forward launch (8 tiles)
constexpr int kGzGroup = 128;    // reduction length of one dZ launch (4 tiles: 64 registers of G per lane)
constexpr int kWGroup = 256;     // rows of dW of one dW launch (4 waves x 2 tiles)
constexpr int kWTarget = 512;    // workgroups of a dW launch, about (grad_w_split)

namespace {   // (a kernel in a header: every translation unit that launches it has its own; as a template, no other has one)

// out[r, j] = sum over the slices q, in order, of part[q * slice_stride + r * row_stride + j]
template <class T>
__device__ __forceinline__ void reduce_slices(const T *__restrict__ part, int slices, int64_t slice_stride, int row_stride,
                                              int rows, int cols, T *__restrict__ out, int64_t ld) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= int64_t(rows) * cols) return;
    const int r = static_cast<int>(e / cols), j = static_cast<int>(e % cols);
    const T *p = part + int64_t(r) * row_stride + j;
    T s = 0;
    for (int q = 0; q < slices; ++q) s += p[q * slice_stride];
    out[int64_t(r) * ld + j] = s;
}

template <class T>
__global__ __launch_bounds__(256) void k_reduce_slices(const T *__restrict__ part, int slices, int64_t slice_stride,
                                                       int row_stride, int rows, int cols, T *__restrict__ out, int64_t ld) {
    reduce_slices(part, slices, slice_stride, row_stride, rows, cols, out, ld);
}

template <class T>
void launch_reduce_slices(const T *part, int64_t slices, int64_t slice_stride, int row_stride, int rows, int cols, T *out,
                          int64_t ld, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((int64_t(rows) * cols + 255) / 256);
    hipLaunchKernelGGL(k_reduce_slices<T>, dim3(grid), dim3(256), 0, s, part, static_cast<int>(slices), slice_stride,
                       row_stride, rows, cols, out, ld);
}

}  // namespace

}  // namespace tgcn
