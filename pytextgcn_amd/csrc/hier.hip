// The first GCNConv's x @ W on [I_N | H] features for plain GCN (the per-level scripts: perlevel_amazon.py:122,156 train a
// GCN on them, text2graph.py:226-246 builds them).  W is the layer's whole weight [N + Fh, F]; with Wh = W[N:]
//     X @ W = W[:N] + H @ Wh,        H zero on the rows below h_row0 (the word rows).
// Composed (conv.features_times on the sparse tensor) that is a SpMM on a second plan, an add pass and, backwards, two
// zero-filled gradients of W's size.  Here the hierarchy block is an operand of its own:
//     tgcn_hier_xw        C[i, :] = W[i, :] + t(i, :)
//                           ONEHOT  t(i, :) = Wh[cls[i - h_row0], :]                     (training: H is the one-hot top label)
//                           DENSE   t(i, c) = sum_f Hd[i - h_row0, f] Wh[f, c]           (test time: H is a softmax)
//     tgcn_hier_xw_grad   dW[0:N] = G,   ONEHOT: dW[N + f, :] = sum of G[i, :] over the rows i >= h_row0 with cls = f
// Streaming kernels: W (G) is read once and C (dW) written once, in float4 lanes where F, the strides and the pointers
// allow and in dword lanes with the same results otherwise.
//   k_hier_rows        rows in blocks of 64, a lane per (row, float4): the copy of W's rows and the ONEHOT term (one more
//                      read of a row of Wh, which is at most 128 rows and sits in the caches).
//   k_hier_dense       a 64 x 64 tile of the document rows per workgroup, 4 x 4 results per lane; Wh and Hd go through
//                      LDS in chunks of 32 features (the whole of Wh, 128 x 300 floats, would not fit), one fmaf per
//                      feature in ascending order from t = 0, then C = W + t.  The ONEHOT kernel forms t as Wh + 0, so a
//                      one-hot Hd gives its bits exactly.
//   k_hier_class_sums  the grouped column sum.  A lane OWNS one (class, float4 of columns) accumulator and walks the rows of
//                      its slice in order; it loads a row of G only where the row's class is its own, so G is still read
//                      once.  The document rows are cut into a fixed number of slices, whose partial sums [slice, Fh, F]
//                      go to the workspace (its size does not grow with N) and are added in slice order by
//                      k_hier_reduce: no atomics, the same bits every run, exact zeros for a class without a row.
// A class id outside [0, Fh) selects nothing (the rule of tgcn_rows_gather: skipped on the device, never read through).
#include <algorithm>

#include "fused_act.h"

namespace tgcn {
namespace {

constexpr int kHierMax = 128;      // the cap on Fh (tgcn_embed_xw_h_max_features has the same)
constexpr int kRowBlock = 64;      // rows per workgroup of k_hier_rows

template <bool VEC>
struct Lane;
template <>
struct Lane<true> {
    using type = float4;
    static constexpr int width = 4;
    static __device__ __forceinline__ type zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ type add(const type &a, const type &b) {
        return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
};
template <>
struct Lane<false> {
    using type = float;
    static constexpr int width = 1;
    static __device__ __forceinline__ type zero() { return 0.f; }
    static __device__ __forceinline__ type add(const type &a, const type &b) { return a + b; }
};

// dst[i, :] = src[i, :] (+ Wh[cls[i - h0], :] for i >= h0 with a class id in [0, Fh)), i in [0, n_rows).  cls == nullptr:
// a plain copy of the rows.
template <bool VEC>
__global__ __launch_bounds__(256) void k_hier_rows(const float *__restrict__ src, int64_t lds_, const float *__restrict__ Wh,
                                                   int64_t ldwh, const int32_t *__restrict__ cls, int64_t h0, int Fh,
                                                   float *__restrict__ dst, int64_t ldd, int64_t n_rows, int F) {
    using L = Lane<VEC>;
    using vec_t = typename L::type;
    const int lanes = F / L::width;                            // per row (VEC: F % 4 == 0)
    const int64_t r0 = int64_t(blockIdx.x) * kRowBlock;
    const int nr = static_cast<int>(n_rows - r0 < kRowBlock ? n_rows - r0 : kRowBlock);
    for (int e = threadIdx.x; e < nr * lanes; e += 256) {
        const int r = e / lanes, c = (e - r * lanes) * L::width;
        const int64_t i = r0 + r;
        vec_t v = *reinterpret_cast<const vec_t *>(src + i * lds_ + c);
        if (cls != nullptr && i >= h0) {
            const int32_t k = cls[i - h0];
            if (k >= 0 && k < Fh) {
                // t = Wh + 0: what the DENSE form's fmaf(1, Wh, 0) gives, signed zeros included
                const vec_t t = L::add(*reinterpret_cast<const vec_t *>(Wh + int64_t(k) * ldwh + c), L::zero());
                v = L::add(v, t);
            }
        }
        *reinterpret_cast<vec_t *>(dst + i * ldd + c) = v;
    }
}

constexpr int kTile = 64;          // rows and columns of a k_hier_dense tile
constexpr int kFChunk = 32;        // features staged at a time
constexpr int kHsLd = kTile + 4;   // row stride of the transposed chunk of Hd (a multiple of 4: float4 reads)

// C[i, :] = W[i, :] + sum_f Hd[i - h0, f] Wh[f, :] for the rows i in [h0, N)
template <bool VEC>
__global__ __launch_bounds__(256) void k_hier_dense(const float *__restrict__ W, int64_t ldw, const float *__restrict__ Wh,
                                                    const float *__restrict__ Hd, int64_t ldh, float *__restrict__ C,
                                                    int64_t ldc, int64_t N, int F, int Fh, int64_t h0) {
    __shared__ __attribute__((aligned(16))) float Ws[kFChunk * kTile];
    __shared__ __attribute__((aligned(16))) float Hs[kFChunk * kHsLd];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t row0 = h0 + int64_t(blockIdx.x) * kTile;
    const int col0 = blockIdx.y * kTile;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;

    for (int f0 = 0; f0 < Fh; f0 += kFChunk) {
        const int nf = Fh - f0 < kFChunk ? Fh - f0 : kFChunk;
        __syncthreads();                                       // the previous chunk has been read
        for (int e = tid; e < kFChunk * kTile; e += 256) {
            const int ff = e / kTile, cc = e % kTile;
            Ws[e] = (ff < nf && col0 + cc < F) ? Wh[int64_t(f0 + ff) * ldw + col0 + cc] : 0.f;
        }
        for (int e = tid; e < kFChunk * kTile; e += 256) {
            const int rr = e / kFChunk, ff = e % kFChunk;
            const int64_t row = row0 + rr;
            Hs[ff * kHsLd + rr] = (ff < nf && row < N) ? Hd[(row - h0) * ldh + f0 + ff] : 0.f;
        }
        __syncthreads();
        for (int ff = 0; ff < nf; ++ff) {                      // f ascending, one fmaf each
            const float4 h = *reinterpret_cast<const float4 *>(Hs + ff * kHsLd + 4 * ty);
            const float4 w = *reinterpret_cast<const float4 *>(Ws + ff * kTile + 4 * tx);
            const float hr[4] = {h.x, h.y, h.z, h.w}, wc[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(hr[r], wc[c], acc[r][c]);
        }
    }
    const int col = col0 + 4 * tx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 4 * ty + r;
        if (row >= N) continue;
        if constexpr (VEC) {
            if (col < F) {                                     // F % 4 == 0: a float4 is inside or outside as a whole
                const float4 w = *reinterpret_cast<const float4 *>(W + row * ldw + col);
                *reinterpret_cast<float4 *>(C + row * ldc + col) =
                    make_float4(w.x + acc[r][0], w.y + acc[r][1], w.z + acc[r][2], w.w + acc[r][3]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (col + c < F) C[row * ldc + col + c] = W[row * ldw + col + c] + acc[r][c];
        }
    }
}

constexpr int kSumLanes = 32;      // column lanes per class in a k_hier_class_sums workgroup
constexpr int kSumClasses = 8;     // classes per workgroup (32 x 8 = 256 lanes)

// part[slice, k, :] = sum over the rows j of the slice, in order, with cls[j] == k, of Gd[j, :]   (Gd = G from row h0 on)
// grid: x the tile of columns, y the tile of classes, z the slice
template <bool VEC>
__global__ __launch_bounds__(256) void k_hier_class_sums(const float *__restrict__ Gd, int64_t ldg,
                                                         const int32_t *__restrict__ cls, int64_t n_doc, int F, int Fh,
                                                         int64_t rows_per_slice, float *__restrict__ part, int Fp) {
    using L = Lane<VEC>;
    using vec_t = typename L::type;
    const int k = blockIdx.y * kSumClasses + (threadIdx.x >> 5);
    const int c = (blockIdx.x * kSumLanes + (threadIdx.x & 31)) * L::width;
    const bool owner = k < Fh && c < F;
    const int64_t j0 = int64_t(blockIdx.z) * rows_per_slice;
    const int64_t j1 = j0 + rows_per_slice < n_doc ? j0 + rows_per_slice : n_doc;
    vec_t acc = L::zero();
    for (int64_t j = j0; j < j1; j += 4) {
        bool mine[4];
        vec_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            mine[u] = owner && j + u < j1 && cls[j + u < j1 ? j + u : j] == k;
            v[u] = mine[u] ? *reinterpret_cast<const vec_t *>(Gd + (j + u) * ldg + c) : L::zero();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (mine[u]) acc = L::add(acc, v[u]);
    }
    if (owner) *reinterpret_cast<vec_t *>(part + (int64_t(blockIdx.z) * Fh + k) * Fp + c) = acc;
}

// dWh[k, c] = sum over the slices, in slice order, of part[slice, k, c]
__global__ __launch_bounds__(256) void k_hier_reduce(const float *__restrict__ part, int slices, int Fh, int F, int Fp,
                                                     float *__restrict__ dWh, int64_t lddw) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Fh * F) return;
    const int k = e / F, c = e - k * F;
    const float *p = part + int64_t(k) * Fp + c;
    const int64_t stride = int64_t(Fh) * Fp;
    float s = 0.f;
    for (int q = 0; q < slices; ++q) s += p[q * stride];
    dWh[int64_t(k) * lddw + c] = s;
}

// How the document rows are cut for the grouped sum: slices of at least 64 rows, at most 1024 of them and at most
// 4 M floats of partial sums (16 MB at the widest Fh x F; for Fh = 6, F = 100 the count is what bounds it).
void class_sum_split(int64_t n_doc, int F, int Fh, int64_t &slices, int64_t &rows_per_slice) {
    const int64_t per_slice = int64_t(Fh) * round_up4(F);
    const int64_t most = std::min<int64_t>(1024, std::max<int64_t>(16, (int64_t(1) << 22) / per_slice));
    rows_per_slice = std::max<int64_t>(64, (n_doc + most - 1) / most);
    slices = (n_doc + rows_per_slice - 1) / rows_per_slice;
}

size_t class_sum_bytes(int64_t n_doc, int F, int Fh) {
    if (n_doc <= 0) return 0;
    int64_t slices, rps;
    class_sum_split(n_doc, F, Fh, slices, rps);
    return static_cast<size_t>(slices * Fh * round_up4(F)) * sizeof(float);
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int check_hier(const char *fn, int64_t N, int F, int Fh, int64_t h_row0, int form) {
    if (N < 0 || F <= 0) {
        set_error("%s: need N >= 0 and F >= 1 (N=%lld, F=%d)", fn, (long long)N, F);
        return TGCN_E_INVALID;
    }
    if (Fh < 1 || Fh > kHierMax) {
        set_error("%s: Fh must be in [1, %d] (tgcn_hier_max_features) (Fh=%d)", fn, kHierMax, Fh);
        return TGCN_E_INVALID;
    }
    if (h_row0 < 0 || h_row0 > N) {
        set_error("%s: h_row0 must be in [0, N] (h_row0=%lld, N=%lld)", fn, (long long)h_row0, (long long)N);
        return TGCN_E_INVALID;
    }
    if (form != TGCN_HIER_ONEHOT && form != TGCN_HIER_DENSE) {
        set_error("%s: unknown form %d (TGCN_HIER_ONEHOT or TGCN_HIER_DENSE)", fn, form);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

unsigned row_blocks(int64_t n) { return static_cast<unsigned>((n + kRowBlock - 1) / kRowBlock); }

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_hier_max_features(void) { return tgcn::kHierMax; }

int tgcn_hier_xw(const float *W, int64_t ldw, int form, const int32_t *cls, const float *Hd, int64_t ldh, int64_t h_row0,
                 int Fh, float *C, int64_t ldc, int64_t N, int F, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_hier_xw";
    TGCN_CHECK(check_hier(fn, N, F, Fh, h_row0, form));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, F));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, F));
    if (form == TGCN_HIER_DENSE) TGCN_CHECK(check_ld(fn, "ldh", ldh, Fh));
    if (N == 0) return TGCN_OK;                // (an empty tensor's pointer may be NULL)
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "C", C));
    if (h_row0 < N) {
        if (form == TGCN_HIER_ONEHOT) TGCN_CHECK(check_ptr(fn, "cls", cls));
        if (form == TGCN_HIER_DENSE) TGCN_CHECK(check_ptr(fn, "Hd", Hd));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float *Wh = W + N * ldw;
    const bool vec = F % 4 == 0 && ldw % 4 == 0 && ldc % 4 == 0 && aligned16(W) && aligned16(C);
    // ONEHOT: every row in one launch.  DENSE: the rows below h_row0 are a copy, the others a tile product.
    const int64_t n_rows = form == TGCN_HIER_ONEHOT ? N : h_row0;
    const int32_t *ids = form == TGCN_HIER_ONEHOT ? cls : nullptr;
    if (n_rows > 0) {
        if (vec)
            hipLaunchKernelGGL(k_hier_rows<true>, dim3(row_blocks(n_rows)), dim3(256), 0, s, W, ldw, Wh, ldw, ids, h_row0, Fh, C,
                               ldc, n_rows, F);
        else
            hipLaunchKernelGGL(k_hier_rows<false>, dim3(row_blocks(n_rows)), dim3(256), 0, s, W, ldw, Wh, ldw, ids, h_row0, Fh,
                               C, ldc, n_rows, F);
    }
    if (form == TGCN_HIER_DENSE && h_row0 < N) {
        const dim3 grid(static_cast<unsigned>((N - h_row0 + kTile - 1) / kTile), static_cast<unsigned>((F + kTile - 1) / kTile));
        if (vec)
            hipLaunchKernelGGL(k_hier_dense<true>, grid, dim3(256), 0, s, W, ldw, Wh, Hd, ldh, C, ldc, N, F, Fh, h_row0);
        else
            hipLaunchKernelGGL(k_hier_dense<false>, grid, dim3(256), 0, s, W, ldw, Wh, Hd, ldh, C, ldc, N, F, Fh, h_row0);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

size_t tgcn_hier_xw_grad_workspace_bytes(int64_t N, int F, int Fh, int64_t h_row0, int form) {
    if (N < 0 || F <= 0 || Fh < 1 || Fh > tgcn::kHierMax || h_row0 < 0 || h_row0 > N || form != TGCN_HIER_ONEHOT) return 0;
    return tgcn::class_sum_bytes(N - h_row0, F, Fh);
}

int tgcn_hier_xw_grad(const float *G, int64_t ldg, int form, const int32_t *cls, int64_t h_row0, int Fh, float *dW,
                      int64_t lddw, int64_t N, int F, void *workspace, size_t workspace_bytes, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_hier_xw_grad";
    TGCN_CHECK(check_hier(fn, N, F, Fh, h_row0, form));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, F));
    TGCN_CHECK(check_ld(fn, "lddw", lddw, F));
    TGCN_CHECK(check_ptr(fn, "dW", dW));
    if (N > 0) TGCN_CHECK(check_ptr(fn, "G", G));
    const int64_t n_doc = N - h_row0;
    const bool sums = form == TGCN_HIER_ONEHOT;            // DENSE: dW[N:] is the caller's tgcn_gemm_tn
    const size_t need = sums ? class_sum_bytes(n_doc, F, Fh) : 0;
    if (sums && n_doc > 0) {
        TGCN_CHECK(check_ptr(fn, "cls", cls));
        if (!workspace || workspace_bytes < need) {        // before anything is enqueued
            set_error("%s: workspace of %zu bytes, tgcn_hier_xw_grad_workspace_bytes() asks for %zu", fn, workspace_bytes, need);
            return TGCN_E_INVALID;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *dWh = dW + N * lddw;
    if (sums && n_doc == 0)                                // nobody has a class: empty sums (and no kernel when N == 0)
        TGCN_HIP_CHECK(hipMemset2DAsync(dWh, sizeof(float) * lddw, 0, sizeof(float) * F, Fh, s));
    if (N == 0) return TGCN_OK;
    const bool vec = F % 4 == 0 && ldg % 4 == 0 && lddw % 4 == 0 && aligned16(G) && aligned16(dW);
    if (vec)
        hipLaunchKernelGGL(k_hier_rows<true>, dim3(row_blocks(N)), dim3(256), 0, s, G, ldg, static_cast<const float *>(nullptr),
                           int64_t(0), static_cast<const int32_t *>(nullptr), N, 0, dW, lddw, N, F);
    else
        hipLaunchKernelGGL(k_hier_rows<false>, dim3(row_blocks(N)), dim3(256), 0, s, G, ldg, static_cast<const float *>(nullptr),
                           int64_t(0), static_cast<const int32_t *>(nullptr), N, 0, dW, lddw, N, F);
    if (sums && n_doc > 0) {
        int64_t slices, rps;
        class_sum_split(n_doc, F, Fh, slices, rps);
        float *part = static_cast<float *>(workspace);
        const int Fp = static_cast<int>(round_up4(F));
        const float *Gd = G + h_row0 * ldg;
        const bool vsum = F % 4 == 0 && ldg % 4 == 0 && aligned16(G) && aligned16(part);
        const int cols_per_tile = kSumLanes * (vsum ? 4 : 1);
        const dim3 grid(static_cast<unsigned>((F + cols_per_tile - 1) / cols_per_tile),
                        static_cast<unsigned>((Fh + kSumClasses - 1) / kSumClasses), static_cast<unsigned>(slices));
        if (vsum)
            hipLaunchKernelGGL(k_hier_class_sums<true>, grid, dim3(256), 0, s, Gd, ldg, cls, n_doc, F, Fh, rps, part, Fp);
        else
            hipLaunchKernelGGL(k_hier_class_sums<false>, grid, dim3(256), 0, s, Gd, ldg, cls, n_doc, F, Fh, rps, part, Fp);
        hipLaunchKernelGGL(k_hier_reduce, dim3(static_cast<unsigned>((Fh * F + 255) / 256)), dim3(256), 0, s, part,
                           static_cast<int>(slices), Fh, F, Fp, dWh, lddw);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // extern "C"
