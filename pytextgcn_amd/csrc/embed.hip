// The front end of EGCN (reference: textgcn/lib/models.py:28-52) on one-hot features, fused into the first GCNConv's
// x @ W:   Linear(N -> K) on the identity is E^T + b (E = the Linear's [K, N] weight), then SELU, then dropout, then the
// product with W [K, n].  Composed from separate ops that is three N x K fp32 activations (and their gradients) that exist
// only to be contracted against W straight away; here element a(i, k) = s * keep(i, k) * selu(E[k, i] + b[k]) is formed in
// registers on its way into the matrix cores and never stored:
//     tgcn_embed_xw        C[i, :]  = sum_k a(i, k) W[k, :]
//     tgcn_embed_xw_grad   dE[k, i] = s keep(i, k) selu'(E[k, i] + b[k]) sum_j G[i, j] W[k, j],   db[k] = sum_i dE[k, i],
//                          dW[k, j] = sum_i a(i, k) G[i, j]                          (a recomputed, the same mask)
// keep(i, k) is the decision of tgcn_gemm_*_dropout (drop_hash.h) for mask row i, column k.
// tgcn_embed_xw_h / tgcn_embed_xw_h_grad (second half of this file) are the same products on [I | H] features: the nodes
// from h_row0 on gain sum_f H[i, f] Eh[k, f] inside the SELU, and dEh joins the gradients.
//
// All three products run on v_mfma_f32_32x32x2_f32 (exact fp32; fragment maps as in dense.hip: lane l feeds A[l & 31][l >> 5]
// and B[l >> 5][l & 31], register r of lane l is C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]).  E's layout suits them: for a
// fixed k the 32 nodes of a tile are contiguous, so a wave's operand load is two 128-byte runs and no transpose is needed;
// the loads are scalar dwords because a contiguous [K, N] parameter has 16-byte rows only when N % 4 == 0.
#include <algorithm>

#include "common.h"
#include "drop_hash.h"

namespace tgcn {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// torch's constants (aten/src/ATen/native/Activation.cpp: selu)
constexpr float kSeluScale = 1.0507009873554805f;
constexpr float kSeluNeg = static_cast<float>(1.0507009873554805 * 1.6732632423543772);   // scale * alpha

struct EmbedDrop {
    const uint64_t *seed;  // device pointer (read by the kernels: safe under HIP-graph capture)
    uint32_t thresh;       // keep iff hash >= thresh
    float scale;           // 1 / (1 - p)
    int64_t row0;          // node i is mask row i + row0
};

__device__ __forceinline__ float selu_f(float x) { return x > 0.f ? kSeluScale * x : kSeluNeg * expm1f(x); }
__device__ __forceinline__ float selu_grad_f(float x) { return x > 0.f ? kSeluScale : kSeluNeg * expf(x); }

// a(i, k) from z = E[k, i] + b[k]
template <bool DROP>
__device__ __forceinline__ float embed_act(float z, uint32_t key, int k, const EmbedDrop &d) {
    const float a = selu_f(z);
    if constexpr (DROP) return drop_hash_keep(key, drop_col_term(k), d.thresh) ? a * d.scale : 0.f;
    return a;
}

template <bool DROP>
__device__ __forceinline__ uint32_t embed_row_key(const EmbedDrop &d, int64_t i) {
    if constexpr (DROP) {
        const uint64_t seed = *d.seed;
        return drop_row_key(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), i + d.row0);
    }
    return 0u;
}

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// ---------------------------------------------------------------------------------------------
// Forward.  A wave owns 32 nodes and all 32 NT result columns; the workgroup's 4 waves share the k chunk of W in LDS
// (W does not fit: 2000 x 200 floats are 1.6 MB, so it goes through 32 rows at a time).  Per MFMA step a lane forms ONE
// element a(i, k) -- its node i is fixed, so the row key of the hash is paid once per lane -- and spends it on NT tiles.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP>
__global__ __launch_bounds__(256, 2) void k_embed_fwd(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                      const float *__restrict__ W, int64_t ldw, float *__restrict__ C,
                                                      int64_t ldc, int64_t N, int K, int n, const EmbedDrop d) {
    constexpr int KC = 32, NP = 32 * NT;
    __shared__ float Ws[KC * NP];
    __shared__ float bs[KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = (int64_t(blockIdx.x) * 4 + wave) * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    const uint32_t key = embed_row_key<DROP>(d, i);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();                                   // the previous chunk has been read
        for (int e = tid; e < KC * NP; e += 256) {
            const int kk = e / NP, j = e % NP;
            Ws[e] = (k0 + kk < K && j < n) ? W[int64_t(k0 + kk) * ldw + j] : 0.f;
        }
        if (tid < KC) bs[tid] = k0 + tid < K ? b[k0 + tid] : 0.f;
        float z[KC / 2];
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int k = k0 + 2 * s + half;
            z[s] = (live && k < K) ? E[int64_t(k) * lde + ic] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int kk = 2 * s + half, k = k0 + kk;
            const float a = (live && k < K) ? embed_act<DROP>(z[s] + bs[kk], key, k, d) : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Ws[kk * NP + 32 * t + c], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = 32 * t + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, half);
            if (row < N && col < n) C[row * ldc + col] = acc[t][r];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dE, in E's layout.  The tile is computed transposed, T[k, i] = sum_j W[k, j] G[i, j], so that the 32 nodes of a tile are
// the lanes of a store (two 128-byte runs per register).  A wave keeps its 32 rows of G in registers (the B operand; loaded
// once, reused over all K / 32 tiles of k), the workgroup shares the 32 rows of W in LDS, transposed with an odd stride so
// that neither the staging writes nor the operand reads conflict.  `accum`: the reduction over j is longer than one launch
// covers (n > 256) and this is not its first piece: the masked, scaled partial sum is added to what dE holds.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP>
__global__ __launch_bounds__(256, 2) void k_embed_grad_e(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                         const float *__restrict__ W, int64_t ldw,
                                                         const float *__restrict__ G, int64_t ldg, float *__restrict__ dE,
                                                         int64_t ldde, int64_t N, int K, int n, int accum, const EmbedDrop d) {
    constexpr int NP = 32 * NT, LDW = 33;
    __shared__ float Ws[NP * LDW];
    __shared__ float bs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t i = (int64_t(blockIdx.x) * 4 + wave) * 32 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    const uint32_t key = embed_row_key<DROP>(d, i);
    float g[16 * NT];
#pragma unroll
    for (int s = 0; s < 16 * NT; ++s) {
        const int j = 2 * s + half;
        g[s] = (live && j < n) ? G[ic * ldg + j] : 0.f;
    }
    for (int k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();
        for (int e = tid; e < 32 * NP; e += 256) {
            const int kk = e / NP, j = e % NP;
            Ws[j * LDW + kk] = (k0 + kk < K && j < n) ? W[int64_t(k0 + kk) * ldw + j] : 0.f;
        }
        if (tid < 32) bs[tid] = k0 + tid < K ? b[k0 + tid] : 0.f;
        float z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + acc_row(r, half);
            z[r] = (live && k < K) ? E[int64_t(k) * lde + ic] : 0.f;
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16 * NT; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[(2 * s + half) * LDW + c], g[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = acc_row(r, half), k = k0 + kk;
            if (live && k < K) {
                float v = acc[r] * selu_grad_f(z[r] + bs[kk]);
                if constexpr (DROP) v = drop_hash_keep(key, drop_col_term(k), d.thresh) ? v * d.scale : 0.f;
                float *out = dE + int64_t(k) * ldde + ic;
                *out = accum ? *out + v : v;
            }
        }
    }
}

// db[k] = sum_i dE[k, i]: one workgroup per row of dE, a fixed summation order (no atomics: reproducible run to run)
__global__ __launch_bounds__(256) void k_embed_rowsum(const float *__restrict__ dE, int64_t ldde, int64_t N,
                                                      float *__restrict__ db) {
    __shared__ float red[256];
    const float *row = dE + int64_t(blockIdx.x) * ldde;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int64_t i = threadIdx.x;
    for (; i + 768 < N; i += 1024) {
        s0 += row[i];
        s1 += row[i + 256];
        s2 += row[i + 512];
        s3 += row[i + 768];
    }
    for (; i < N; i += 256) s0 += row[i];
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) db[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------------------------------------
// dW[k, j] = sum_i a(i, k) G[i, j]: the reduction runs over the nodes.  The node index is the contiguous one of E, and an
// MFMA step takes only two reduction indices across the lanes, so the tile of a goes through LDS: the workgroup reads 32
// rows of E x 128 nodes coalesced, forms a(i, k) ONCE per element and stores it with an odd row stride; the matrix cores
// then read it as the A operand (row k per lane) without conflicts.  The 4 waves split the result columns (TW tiles of 32
// each) and read their slab of G straight from memory, 128 bytes per half wave.  blockIdx.x is the tile of k, blockIdx.y a
// slice of the nodes; the slices' partial sums go to the workspace and are added in a fixed order by k_embed_reduce_w.
// ---------------------------------------------------------------------------------------------
constexpr int kWChunk = 128;   // nodes per staged tile

template <int TW, bool DROP>
__global__ __launch_bounds__(256, 2) void k_embed_grad_w(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                         const float *__restrict__ G, int64_t ldg, float *__restrict__ part,
                                                         int64_t N, int K, int n, int64_t chunks_per_slice,
                                                         const EmbedDrop d) {
    constexpr int LDA = kWChunk + 1, NP = 128 * TW;
    __shared__ float As[32 * LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int k0 = blockIdx.x * 32;
    const int kpad = gridDim.x * 32;
    const int64_t i_begin = int64_t(blockIdx.y) * chunks_per_slice * kWChunk;
    const int64_t i_stop = i_begin + chunks_per_slice * kWChunk;
    const int64_t i_end = i_stop < N ? i_stop : N;
    const bool computes = wave * TW * 32 < n;             // a wave whose columns are all padding only helps staging
    float bk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) bk[u] = k0 + wave * 8 + u < K ? b[k0 + wave * 8 + u] : 0.f;
    f32x16 acc[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int64_t i0 = i_begin; i0 < i_end; i0 += kWChunk) {
        float z[2][8];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int64_t i = i0 + lane + 64 * v;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + wave * 8 + u;
                z[v][u] = (i < i_end && k < K) ? E[int64_t(k) * lde + i] : 0.f;
            }
        }
        __syncthreads();                                   // the previous tile has been read
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int64_t i = i0 + lane + 64 * v;
            const uint32_t key = embed_row_key<DROP>(d, i);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int kk = wave * 8 + u, k = k0 + kk;
                As[kk * LDA + lane + 64 * v] = (i < i_end && k < K) ? embed_act<DROP>(z[v][u] + bk[u], key, k, d) : 0.f;
            }
        }
        __syncthreads();
        if (computes) {
#pragma unroll 8
            for (int s = 0; s < kWChunk / 2; ++s) {
                const int ii = 2 * s + half;
                const int64_t i = i0 + ii;
                const float a = As[c * LDA + ii];
#pragma unroll
                for (int t = 0; t < TW; ++t) {
                    const int j = (wave * TW + t) * 32 + c;
                    const float gv = (i < i_end && j < n) ? G[i * ldg + j] : 0.f;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gv, acc[t], 0, 0, 0);
                }
            }
        }
    }
    float *out = part + (int64_t(blockIdx.y) * kpad + k0) * NP;
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[int64_t(acc_row(r, half)) * NP + (wave * TW + t) * 32 + c] = acc[t][r];
}

__global__ __launch_bounds__(256) void k_embed_reduce_w(const float *__restrict__ part, int slices, int kpad, int np, int K,
                                                        int n, float *__restrict__ dW, int64_t lddw) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= int64_t(K) * n) return;
    const int k = static_cast<int>(e / n), j = static_cast<int>(e % n);
    const float *p = part + int64_t(k) * np + j;
    const int64_t stride = int64_t(kpad) * np;
    float s = 0.f;
    for (int q = 0; q < slices; ++q) s += p[q * stride];
    dW[int64_t(k) * lddw + j] = s;
}

constexpr int kFwdGroup = 256;   // result columns of one forward launch / reduction length of one dE launch (8 tiles)
constexpr int kWGroup = 256;     // result columns of one dW launch (4 waves x 2 tiles)

// how the nodes are cut into slices for dW: about 1024 workgroups in all, at most 256 slices
void grad_w_split(int64_t N, int K, int64_t &slices, int64_t &chunks_per_slice) {
    const int64_t chunks = std::max<int64_t>(1, (N + kWChunk - 1) / kWChunk);
    const int64_t ktiles = (int64_t(K) + 31) / 32;
    const int64_t want = std::min<int64_t>(256, std::max<int64_t>(1, 1024 / ktiles));
    chunks_per_slice = (chunks + want - 1) / want;
    slices = (chunks + chunks_per_slice - 1) / chunks_per_slice;
}

size_t grad_w_bytes(int64_t N, int K, int n) {
    int64_t slices, cps;
    grad_w_split(N, K, slices, cps);
    const int64_t kpad = (int64_t(K) + 31) / 32 * 32;
    const int64_t np = std::min(n, kWGroup) > 128 ? 256 : 128;
    return static_cast<size_t>(slices * kpad * np) * sizeof(float);
}

int make_embed_drop(const char *fn, double p, const uint64_t *seed, int64_t mask_row0, EmbedDrop &d, bool &on) {
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

int check_sizes(const char *fn, int64_t N, int K, int n) {
    if (N < 0 || K <= 0 || n <= 0) {
        set_error("%s: need N >= 0, K >= 1 and n >= 1 (N=%lld, K=%d, n=%d)", fn, (long long)N, K, n);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

#define TGCN_EMBED_LD(name, ld, extent)                                                                     \
    if ((ld) < (extent)) {                                                                                  \
        set_error("%s: " name " (%lld) is smaller than the extent %lld", fn, (long long)(ld), (long long)(extent)); \
        return TGCN_E_INVALID;                                                                              \
    }
#define TGCN_EMBED_PTR(name, ptr)                            \
    if (!(ptr)) {                                            \
        set_error("%s: " name " is NULL", fn);               \
        return TGCN_E_INVALID;                               \
    }

template <bool DROP>
int launch_fwd(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
               int K, int n, const EmbedDrop &d, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup), nt = (ng + 31) / 32;
#define TGCN_EMBED_FWD(NT)                                                                                             \
    hipLaunchKernelGGL((k_embed_fwd<NT, DROP>), dim3(grid), dim3(256), 0, s, E, lde, b, W + col0, ldw, C + col0, ldc, N, K, \
                       ng, d)
        if (nt <= 1) TGCN_EMBED_FWD(1);
        else if (nt <= 2) TGCN_EMBED_FWD(2);
        else if (nt <= 4) TGCN_EMBED_FWD(4);
        else if (nt <= 7) TGCN_EMBED_FWD(7);
        else TGCN_EMBED_FWD(8);
#undef TGCN_EMBED_FWD
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_grad_e(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, const float *G, int64_t ldg,
                  float *dE, int64_t ldde, float *db, int64_t N, int K, int n, const EmbedDrop &d, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup), nt = (ng + 31) / 32, accum = col0 > 0;
#define TGCN_EMBED_GE(NT)                                                                                                \
    hipLaunchKernelGGL((k_embed_grad_e<NT, DROP>), dim3(grid), dim3(256), 0, s, E, lde, b, W + col0, ldw, G + col0, ldg, dE, \
                       ldde, N, K, ng, accum, d)
        if (nt <= 1) TGCN_EMBED_GE(1);
        else if (nt <= 2) TGCN_EMBED_GE(2);
        else if (nt <= 4) TGCN_EMBED_GE(4);
        else if (nt <= 7) TGCN_EMBED_GE(7);
        else TGCN_EMBED_GE(8);
#undef TGCN_EMBED_GE
    }
    hipLaunchKernelGGL(k_embed_rowsum, dim3(K), dim3(256), 0, s, dE, ldde, N, db);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_grad_w(const float *E, int64_t lde, const float *b, const float *G, int64_t ldg, float *dW, int64_t lddw,
                  int64_t N, int K, int n, const EmbedDrop &d, float *part, hipStream_t s) {
    int64_t slices, cps;
    grad_w_split(N, K, slices, cps);
    const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
    for (int col0 = 0; col0 < n; col0 += kWGroup) {
        const int ng = std::min(n - col0, kWGroup);
        const dim3 grid(ktiles, static_cast<unsigned>(slices));
        if (ng > 128)
            hipLaunchKernelGGL((k_embed_grad_w<2, DROP>), grid, dim3(256), 0, s, E, lde, b, G + col0, ldg, part, N, K, ng, cps, d);
        else
            hipLaunchKernelGGL((k_embed_grad_w<1, DROP>), grid, dim3(256), 0, s, E, lde, b, G + col0, ldg, part, N, K, ng, cps, d);
        const int np = ng > 128 ? 256 : 128;
        const unsigned rgrid = static_cast<unsigned>((int64_t(K) * ng + 255) / 256);
        hipLaunchKernelGGL(k_embed_reduce_w, dim3(rgrid), dim3(256), 0, s, part, static_cast<int>(slices), kpad, np, K, ng,
                           dW + col0, lddw);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// =============================================================================================
// [I | H] features (the hierarchy features of the per-level scripts; text2graph.py:226-246): the Linear's weight is
// [K, N + Fh], E its first N columns, Eh the last Fh, and for the nodes i >= h0 (the document rows)
//     z(i, k) = (E[k, i] + b[k]) + t(i, k),      t(i, k) = sum_f H[i, f] Eh[k, f]   (f ascending, one fma each).
// t is itself a small product, so it runs on the matrix cores as well: per chunk of 32 k a wave forms the 32 x 32 tile
// T[k, node] = Ehs[k, :] H[node, :]^T in ceil(Fh / 2) MFMA steps (against 16 NT for the main product).  Its accumulator
// registers hold, for the lane's node, 16 values of k -- exactly the 16 pre-activations the lane needs next; the forward
// kernel reads the rows of Ehs through a permutation so that register r of half-wave `half` is k = 2 r + half, the A
// operand order of its own MFMA steps.  The workgroup's chunk of Eh sits in LDS beside the chunk of W (odd row stride:
// the 32 rows a half-wave reads fall into 32 banks).  The lane's node is fixed, so its H values are loaded once: the
// first 2 kHReg features into registers, the rest (Fh > 16) again per chunk from the caches -- H is [N_doc, Fh], far
// below the L2's size.  A wave whose nodes all lie below h0 -- the word rows, two thirds of a TextGCN graph -- skips the
// term through a wave-uniform branch and computes what k_embed_* compute, bit for bit.
// =============================================================================================
constexpr int kHMax = 128;        // the cap on Fh
constexpr int kHLd = kHMax + 1;   // row stride of the chunk of Eh in LDS
constexpr int kHReg = 8;          // MFMA steps (pairs of features) whose H operand stays in registers

struct EmbedH {
    const float *Eh;   // [K, Fh], row stride ldeh
    int64_t ldeh;
    const float *Hd;   // [N - h0, Fh], row stride ldh: the rows of H from node h0 on
    int64_t ldh;
    int64_t h0;
    int Fh;
};

__device__ __forceinline__ float h_load(const EmbedH &h, int64_t i, int64_t N, int f) {
    return (i >= h.h0 && i < N && f < h.Fh) ? h.Hd[(i - h.h0) * h.ldh + f] : 0.f;
}

// rows k0 .. k0 + 31 of Eh, zero-padded to an even number of features
__device__ __forceinline__ void stage_eh(float *Ehs, const EmbedH &h, int k0, int K, int tid) {
    const int fp = (h.Fh + 1) & ~1;
    for (int e = tid; e < 32 * fp; e += 256) {
        const int kk = e / fp, f = e % fp;
        Ehs[kk * kHLd + f] = (k0 + kk < K && f < h.Fh) ? h.Eh[int64_t(k0 + kk) * h.ldeh + f] : 0.f;
    }
}

// the tile of t for the lane's node i: register r is k = k0 + 2 r + half (PAIRED, the forward's operand order) or
// k = k0 + acc_row(r, half) (the order of a transposed result tile)
template <bool PAIRED>
__device__ __forceinline__ f32x16 h_term(const float *Ehs, const float (&hreg)[kHReg], const EmbedH &h, int64_t i, int64_t N,
                                         int c, int half) {
    const int m = PAIRED ? 2 * ((c & 3) + 4 * (c >> 3)) + ((c >> 2) & 1) : c;   // acc_row(r, half) == m  <=>  k = 2 r + half
    const float *row = Ehs + m * kHLd + half;
    const int pairs = (h.Fh + 1) >> 1;
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll
    for (int sp = 0; sp < kHReg; ++sp)
        if (sp < pairs) t = __builtin_amdgcn_mfma_f32_32x32x2f32(row[2 * sp], hreg[sp], t, 0, 0, 0);
    for (int sp = kHReg; sp < pairs; ++sp)
        t = __builtin_amdgcn_mfma_f32_32x32x2f32(row[2 * sp], h_load(h, i, N, 2 * sp + half), t, 0, 0, 0);
    return t;
}

template <int NT, bool DROP>
__global__ __launch_bounds__(256, 2) void k_embed_h_fwd(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                        const float *__restrict__ W, int64_t ldw, float *__restrict__ C,
                                                        int64_t ldc, int64_t N, int K, int n, const EmbedH h,
                                                        const EmbedDrop d) {
    constexpr int KC = 32, NP = 32 * NT;
    __shared__ float Ws[KC * NP];
    __shared__ float Ehs[KC * kHLd];
    __shared__ float bs[KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = (int64_t(blockIdx.x) * 4 + wave) * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    const bool wg_h = (int64_t(blockIdx.x) + 1) * 128 > h.h0;      // some node of the workgroup may have an H row
    const bool wave_h = row0 + 32 > h.h0 && row0 < N;              // wave-uniform
    const uint32_t key = embed_row_key<DROP>(d, i);
    float hreg[kHReg];
#pragma unroll
    for (int sp = 0; sp < kHReg; ++sp) hreg[sp] = wave_h ? h_load(h, i, N, 2 * sp + half) : 0.f;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();                                   // the previous chunk has been read
        for (int e = tid; e < KC * NP; e += 256) {
            const int kk = e / NP, j = e % NP;
            Ws[e] = (k0 + kk < K && j < n) ? W[int64_t(k0 + kk) * ldw + j] : 0.f;
        }
        if (tid < KC) bs[tid] = k0 + tid < K ? b[k0 + tid] : 0.f;
        if (wg_h) stage_eh(Ehs, h, k0, K, tid);
        float z[KC / 2];
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int k = k0 + 2 * s + half;
            z[s] = (live && k < K) ? E[int64_t(k) * lde + ic] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) z[s] = z[s] + bs[2 * s + half];
        if (wave_h) {
            const f32x16 t = h_term<true>(Ehs, hreg, h, i, N, c, half);
#pragma unroll
            for (int s = 0; s < KC / 2; ++s) z[s] = z[s] + t[s];
        }
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int kk = 2 * s + half, k = k0 + kk;
            const float a = (live && k < K) ? embed_act<DROP>(z[s], key, k, d) : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Ws[kk * NP + 32 * t + c], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = 32 * t + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, half);
            if (row < N && col < n) C[row * ldc + col] = acc[t][r];
        }
    }
}

// dE as k_embed_grad_e forms it, with z = (E + b) + t.  (dEh needs the FINISHED dE -- with n > 256 it is the sum of
// several launches -- so it is a product of its own: k_embed_h_grad_eh.)
template <int NT, bool DROP>
__global__ __launch_bounds__(256, 2) void k_embed_h_grad_e(const float *__restrict__ E, int64_t lde,
                                                           const float *__restrict__ b, const float *__restrict__ W,
                                                           int64_t ldw, const float *__restrict__ G, int64_t ldg,
                                                           float *__restrict__ dE, int64_t ldde, int64_t N, int K, int n,
                                                           int accum, const EmbedH h, const EmbedDrop d) {
    constexpr int NP = 32 * NT, LDW = 33;
    __shared__ float Ws[NP * LDW];
    __shared__ float Ehs[32 * kHLd];
    __shared__ float bs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = (int64_t(blockIdx.x) * 4 + wave) * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    const bool wg_h = (int64_t(blockIdx.x) + 1) * 128 > h.h0;
    const bool wave_h = row0 + 32 > h.h0 && row0 < N;
    const uint32_t key = embed_row_key<DROP>(d, i);
    float hreg[kHReg];
#pragma unroll
    for (int sp = 0; sp < kHReg; ++sp) hreg[sp] = wave_h ? h_load(h, i, N, 2 * sp + half) : 0.f;
    float g[16 * NT];
#pragma unroll
    for (int s = 0; s < 16 * NT; ++s) {
        const int j = 2 * s + half;
        g[s] = (live && j < n) ? G[ic * ldg + j] : 0.f;
    }
    for (int k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();
        for (int e = tid; e < 32 * NP; e += 256) {
            const int kk = e / NP, j = e % NP;
            Ws[j * LDW + kk] = (k0 + kk < K && j < n) ? W[int64_t(k0 + kk) * ldw + j] : 0.f;
        }
        if (tid < 32) bs[tid] = k0 + tid < K ? b[k0 + tid] : 0.f;
        if (wg_h) stage_eh(Ehs, h, k0, K, tid);
        float z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + acc_row(r, half);
            z[r] = (live && k < K) ? E[int64_t(k) * lde + ic] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = z[r] + bs[acc_row(r, half)];
        if (wave_h) {
            const f32x16 t = h_term<false>(Ehs, hreg, h, i, N, c, half);
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = z[r] + t[r];
        }
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16 * NT; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[(2 * s + half) * LDW + c], g[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + acc_row(r, half);
            if (live && k < K) {
                float v = acc[r] * selu_grad_f(z[r]);
                if constexpr (DROP) v = drop_hash_keep(key, drop_col_term(k), d.thresh) ? v * d.scale : 0.f;
                float *out = dE + int64_t(k) * ldde + ic;
                *out = accum ? *out + v : v;
            }
        }
    }
}

// dW as k_embed_grad_w forms it, with a from z = (E + b) + t.  Here the nodes change from tile to tile, so the tile is
// staged by (node = wave * 32 + c, k = acc_row(r, half)) -- the layout in which the matrix cores deliver t -- and the H
// operand of a tile is read once, where the tile is formed.  The workgroup's k tile is fixed: its rows of Eh are staged once.
template <int TW, bool DROP>
__global__ __launch_bounds__(256, 2) void k_embed_h_grad_w(const float *__restrict__ E, int64_t lde,
                                                           const float *__restrict__ b, const float *__restrict__ G,
                                                           int64_t ldg, float *__restrict__ part, int64_t N, int K, int n,
                                                           int64_t chunks_per_slice, const EmbedH h, const EmbedDrop d) {
    constexpr int LDA = kWChunk + 1, NP = 128 * TW;
    __shared__ float As[32 * LDA];
    __shared__ float Ehs[32 * kHLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int k0 = blockIdx.x * 32;
    const int kpad = gridDim.x * 32;
    const int64_t i_begin = int64_t(blockIdx.y) * chunks_per_slice * kWChunk;
    const int64_t i_stop = i_begin + chunks_per_slice * kWChunk;
    const int64_t i_end = i_stop < N ? i_stop : N;
    const bool computes = wave * TW * 32 < n;
    const int pairs = (h.Fh + 1) >> 1;
    float bk[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bk[r] = k0 + acc_row(r, half) < K ? b[k0 + acc_row(r, half)] : 0.f;
    const bool slice_h = i_end > h.h0;                     // some node of the slice has an H row
    if (slice_h) stage_eh(Ehs, h, k0, K, tid);             // (read after the first barrier of the loop)
    f32x16 acc[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int64_t i0 = i_begin; i0 < i_end; i0 += kWChunk) {
        const int64_t w0 = i0 + wave * 32, i = w0 + c;
        const bool live = i < i_end;
        float z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + acc_row(r, half);
            z[r] = (live && k < K) ? E[int64_t(k) * lde + i] : 0.f;
        }
        __syncthreads();                                   // the previous tile has been read (and Ehs is staged)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = z[r] + bk[r];
        if (slice_h && w0 + 32 > h.h0 && w0 < i_end) {     // wave-uniform
            f32x16 t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.f;
            for (int sp = 0; sp < pairs; ++sp)
                t = __builtin_amdgcn_mfma_f32_32x32x2f32(Ehs[c * kHLd + 2 * sp + half], h_load(h, i, i_end, 2 * sp + half), t,
                                                         0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = z[r] + t[r];
        }
        const uint32_t key = embed_row_key<DROP>(d, i);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kk = acc_row(r, half), k = k0 + kk;
            As[kk * LDA + wave * 32 + c] = (live && k < K) ? embed_act<DROP>(z[r], key, k, d) : 0.f;
        }
        __syncthreads();
        if (computes) {
#pragma unroll 8
            for (int s = 0; s < kWChunk / 2; ++s) {
                const int ii = 2 * s + half;
                const int64_t in = i0 + ii;
                const float a = As[c * LDA + ii];
#pragma unroll
                for (int t = 0; t < TW; ++t) {
                    const int j = (wave * TW + t) * 32 + c;
                    const float gv = (in < i_end && j < n) ? G[in * ldg + j] : 0.f;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gv, acc[t], 0, 0, 0);
                }
            }
        }
    }
    float *out = part + (int64_t(blockIdx.y) * kpad + k0) * NP;
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[int64_t(acc_row(r, half)) * NP + (wave * TW + t) * 32 + c] = acc[t][r];
}

// dEh[k, f] = sum_{i >= h0} dE[k, i] H[i, f]: the reduction over the nodes that the kernels above do not have.  The shape
// of k_embed_grad_w with the finished dE in the place of the activation: blockIdx.x is the tile of k, blockIdx.y one of a
// FIXED number of slices of the nodes from h0 on; the workgroup stages 32 rows of dE x 128 nodes, the 4 waves take the
// (at most 4) tiles of 32 features and read their rows of H straight from memory.  The slices' partial sums [32, 128] go
// to the workspace and k_embed_reduce_w adds them in slice order: no atomics, the same bits every run.
__global__ __launch_bounds__(256, 2) void k_embed_h_grad_eh(const float *__restrict__ dE, int64_t ldde, float *__restrict__ part,
                                                            int64_t N, int K, int64_t chunks_per_slice, const EmbedH h) {
    constexpr int LDA = kWChunk + 1, NP = kHMax;
    __shared__ float As[32 * LDA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int k0 = blockIdx.x * 32;
    const int kpad = gridDim.x * 32;
    const int64_t i_begin = h.h0 + int64_t(blockIdx.y) * chunks_per_slice * kWChunk;
    const int64_t i_stop = i_begin + chunks_per_slice * kWChunk;
    const int64_t i_end = i_stop < N ? i_stop : N;
    const int f = wave * 32 + c;
    const bool computes = wave * 32 < h.Fh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int64_t i0 = i_begin; i0 < i_end; i0 += kWChunk) {
        float v[2][8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t i = i0 + lane + 64 * q;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + wave * 8 + u;
                v[q][u] = (i < i_end && k < K) ? dE[int64_t(k) * ldde + i] : 0.f;
            }
        }
        __syncthreads();                                   // the previous tile has been read
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int u = 0; u < 8; ++u) As[(wave * 8 + u) * LDA + lane + 64 * q] = v[q][u];
        __syncthreads();
        if (computes) {
#pragma unroll 8
            for (int s = 0; s < kWChunk / 2; ++s) {
                const int ii = 2 * s + half;
                const int64_t in = i0 + ii;
                const float hv = (in < i_end && f < h.Fh) ? h.Hd[(in - h.h0) * h.ldh + f] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[c * LDA + ii], hv, acc, 0, 0, 0);
            }
        }
    }
    float *out = part + (int64_t(blockIdx.y) * kpad + k0) * NP;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[int64_t(acc_row(r, half)) * NP + f] = acc[r];
}

// the workspace of tgcn_embed_xw_h_grad: the partial sums of dW and those of dEh use it one after the other.  dEh's nodes
// are cut with the chunks-per-slice that the whole N would get, so that a later h0 only means fewer slices.
size_t grad_eh_bytes(int64_t N, int K) {
    int64_t slices, cps;
    grad_w_split(N, K, slices, cps);
    const int64_t kpad = (int64_t(K) + 31) / 32 * 32;
    return static_cast<size_t>(slices * kpad * kHMax) * sizeof(float);
}

int check_h(const char *fn, int64_t N, int Fh, int64_t h_row0) {
    if (Fh < 1 || Fh > kHMax) {
        set_error("%s: Fh must be in [1, %d] (tgcn_embed_xw_h_max_features) (Fh=%d)", fn, kHMax, Fh);
        return TGCN_E_INVALID;
    }
    if (h_row0 < 0 || h_row0 > N) {
        set_error("%s: h_row0 must be in [0, N] (h_row0=%lld, N=%lld)", fn, (long long)h_row0, (long long)N);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

template <bool DROP>
int launch_h_fwd(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
                 int K, int n, const EmbedH &h, const EmbedDrop &d, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup), nt = (ng + 31) / 32;
#define TGCN_EMBED_FWD(NT)                                                                                               \
    hipLaunchKernelGGL((k_embed_h_fwd<NT, DROP>), dim3(grid), dim3(256), 0, s, E, lde, b, W + col0, ldw, C + col0, ldc, N, K, \
                       ng, h, d)
        if (nt <= 1) TGCN_EMBED_FWD(1);
        else if (nt <= 2) TGCN_EMBED_FWD(2);
        else if (nt <= 4) TGCN_EMBED_FWD(4);
        else if (nt <= 7) TGCN_EMBED_FWD(7);
        else TGCN_EMBED_FWD(8);
#undef TGCN_EMBED_FWD
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_h_grad_e(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, const float *G, int64_t ldg,
                    float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, int64_t N, int K, int n, const EmbedH &h,
                    const EmbedDrop &d, float *part, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup), nt = (ng + 31) / 32, accum = col0 > 0;
#define TGCN_EMBED_GE(NT)                                                                                                  \
    hipLaunchKernelGGL((k_embed_h_grad_e<NT, DROP>), dim3(grid), dim3(256), 0, s, E, lde, b, W + col0, ldw, G + col0, ldg, dE, \
                       ldde, N, K, ng, accum, h, d)
        if (nt <= 1) TGCN_EMBED_GE(1);
        else if (nt <= 2) TGCN_EMBED_GE(2);
        else if (nt <= 4) TGCN_EMBED_GE(4);
        else if (nt <= 7) TGCN_EMBED_GE(7);
        else TGCN_EMBED_GE(8);
#undef TGCN_EMBED_GE
    }
    hipLaunchKernelGGL(k_embed_rowsum, dim3(K), dim3(256), 0, s, dE, ldde, N, db);
    if (h.h0 == N) {                           // nobody has an H row: an empty sum
        TGCN_HIP_CHECK(hipMemset2DAsync(dEh, sizeof(float) * lddeh, 0, sizeof(float) * h.Fh, K, s));
    } else {
        int64_t slices, cps;
        grad_w_split(N, K, slices, cps);
        const int64_t chunks = (N - h.h0 + kWChunk - 1) / kWChunk;
        slices = (chunks + cps - 1) / cps;     // <= the slices of the whole N, which the workspace is sized for
        const int ktiles = (K + 31) / 32;
        hipLaunchKernelGGL(k_embed_h_grad_eh, dim3(ktiles, static_cast<unsigned>(slices)), dim3(256), 0, s, dE, ldde, part, N, K,
                           cps, h);
        const unsigned rgrid = static_cast<unsigned>((int64_t(K) * h.Fh + 255) / 256);
        hipLaunchKernelGGL(k_embed_reduce_w, dim3(rgrid), dim3(256), 0, s, part, static_cast<int>(slices), ktiles * 32, kHMax, K,
                           h.Fh, dEh, lddeh);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_h_grad_w(const float *E, int64_t lde, const float *b, const float *G, int64_t ldg, float *dW, int64_t lddw,
                    int64_t N, int K, int n, const EmbedH &h, const EmbedDrop &d, float *part, hipStream_t s) {
    int64_t slices, cps;
    grad_w_split(N, K, slices, cps);
    const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
    for (int col0 = 0; col0 < n; col0 += kWGroup) {
        const int ng = std::min(n - col0, kWGroup);
        const dim3 grid(ktiles, static_cast<unsigned>(slices));
        if (ng > 128)
            hipLaunchKernelGGL((k_embed_h_grad_w<2, DROP>), grid, dim3(256), 0, s, E, lde, b, G + col0, ldg, part, N, K, ng, cps,
                               h, d);
        else
            hipLaunchKernelGGL((k_embed_h_grad_w<1, DROP>), grid, dim3(256), 0, s, E, lde, b, G + col0, ldg, part, N, K, ng, cps,
                               h, d);
        const int np = ng > 128 ? 256 : 128;
        const unsigned rgrid = static_cast<unsigned>((int64_t(K) * ng + 255) / 256);
        hipLaunchKernelGGL(k_embed_reduce_w, dim3(rgrid), dim3(256), 0, s, part, static_cast<int>(slices), kpad, np, K, ng,
                           dW + col0, lddw);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_embed_xw(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, float *C, int64_t ldc,
                  int64_t N, int K, int n, double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_embed_xw";
    TGCN_CHECK(check_sizes(fn, N, K, n));
    EmbedDrop d{};
    bool drop = false;
    TGCN_CHECK(make_embed_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_EMBED_LD("lde", lde, N);
    TGCN_EMBED_LD("ldw", ldw, n);
    TGCN_EMBED_LD("ldc", ldc, n);
    if (N == 0) return TGCN_OK;                // (an empty tensor's pointer may be NULL)
    TGCN_EMBED_PTR("E", E);
    TGCN_EMBED_PTR("b", b);
    TGCN_EMBED_PTR("W", W);
    TGCN_EMBED_PTR("C", C);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return drop ? launch_fwd<true>(E, lde, b, W, ldw, C, ldc, N, K, n, d, s)
                : launch_fwd<false>(E, lde, b, W, ldw, C, ldc, N, K, n, d, s);
}

size_t tgcn_embed_xw_grad_workspace_bytes(int64_t N, int K, int n) {
    if (N < 0 || K <= 0 || n <= 0) return 0;
    return tgcn::grad_w_bytes(N, K, n);
}

int tgcn_embed_xw_grad(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, const float *G,
                       int64_t ldg, float *dE, int64_t ldde, float *db, float *dW, int64_t lddw, int64_t N, int K, int n,
                       double p, const uint64_t *seed, int64_t mask_row0, void *workspace, size_t workspace_bytes,
                       tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_embed_xw_grad";
    TGCN_CHECK(check_sizes(fn, N, K, n));
    EmbedDrop d{};
    bool drop = false;
    TGCN_CHECK(make_embed_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_EMBED_LD("lde", lde, N);
    TGCN_EMBED_LD("ldw", ldw, n);
    TGCN_EMBED_LD("ldg", ldg, n);
    if (dE) {
        TGCN_EMBED_LD("ldde", ldde, N);
    }
    if (dW) {
        TGCN_EMBED_LD("lddw", lddw, n);
    }
    if ((dE == nullptr) != (db == nullptr) && N > 0) {
        set_error("%s: dE and db are computed together: pass both or neither (db is the row sum of dE)", fn);
        return TGCN_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {                              // empty sums; there is no element of dE
        if (db) TGCN_HIP_CHECK(hipMemsetAsync(db, 0, sizeof(float) * K, s));
        if (dW) TGCN_HIP_CHECK(hipMemset2DAsync(dW, sizeof(float) * lddw, 0, sizeof(float) * n, K, s));
        return TGCN_OK;
    }
    TGCN_EMBED_PTR("E", E);
    TGCN_EMBED_PTR("b", b);
    TGCN_EMBED_PTR("W", W);
    TGCN_EMBED_PTR("G", G);
    if (!dE && !dW) {
        set_error("%s: dE (with db) and dW are both NULL: nothing to compute", fn);
        return TGCN_E_INVALID;
    }
    if (dE) {
        TGCN_CHECK(drop ? launch_grad_e<true>(E, lde, b, W, ldw, G, ldg, dE, ldde, db, N, K, n, d, s)
                        : launch_grad_e<false>(E, lde, b, W, ldw, G, ldg, dE, ldde, db, N, K, n, d, s));
    }
    if (dW) {
        const size_t need = grad_w_bytes(N, K, n);
        if (!workspace || workspace_bytes < need) {
            set_error("%s: workspace of %zu bytes, tgcn_embed_xw_grad_workspace_bytes() asks for %zu", fn, workspace_bytes, need);
            return TGCN_E_WORKSPACE;
        }
        float *part = static_cast<float *>(workspace);
        TGCN_CHECK(drop ? launch_grad_w<true>(E, lde, b, G, ldg, dW, lddw, N, K, n, d, part, s)
                        : launch_grad_w<false>(E, lde, b, G, ldg, dW, lddw, N, K, n, d, part, s));
    }
    return TGCN_OK;
}

int tgcn_embed_xw_h_max_features(void) { return tgcn::kHMax; }

int tgcn_embed_xw_h(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd, int64_t ldh,
                    int64_t h_row0, int Fh, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N, int K, int n,
                    double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_embed_xw_h";
    TGCN_CHECK(check_sizes(fn, N, K, n));
    TGCN_CHECK(check_h(fn, N, Fh, h_row0));
    EmbedDrop d{};
    bool drop = false;
    TGCN_CHECK(make_embed_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_EMBED_LD("lde", lde, N);
    TGCN_EMBED_LD("ldeh", ldeh, Fh);
    TGCN_EMBED_LD("ldh", ldh, Fh);
    TGCN_EMBED_LD("ldw", ldw, n);
    TGCN_EMBED_LD("ldc", ldc, n);
    if (N == 0) return TGCN_OK;                // (an empty tensor's pointer may be NULL)
    TGCN_EMBED_PTR("E", E);
    TGCN_EMBED_PTR("b", b);
    TGCN_EMBED_PTR("Eh", Eh);
    if (h_row0 < N) TGCN_EMBED_PTR("Hd", Hd);
    TGCN_EMBED_PTR("W", W);
    TGCN_EMBED_PTR("C", C);
    const EmbedH h{Eh, ldeh, Hd, ldh, h_row0, Fh};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return drop ? launch_h_fwd<true>(E, lde, b, W, ldw, C, ldc, N, K, n, h, d, s)
                : launch_h_fwd<false>(E, lde, b, W, ldw, C, ldc, N, K, n, h, d, s);
}

size_t tgcn_embed_xw_h_grad_workspace_bytes(int64_t N, int K, int n, int Fh) {
    if (N < 0 || K <= 0 || n <= 0 || Fh < 1 || Fh > tgcn::kHMax) return 0;
    return std::max(tgcn::grad_w_bytes(N, K, n), tgcn::grad_eh_bytes(N, K));
}

int tgcn_embed_xw_h_grad(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd,
                         int64_t ldh, int64_t h_row0, int Fh, const float *W, int64_t ldw, const float *G, int64_t ldg,
                         float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, float *dW, int64_t lddw, int64_t N,
                         int K, int n, double p, const uint64_t *seed, int64_t mask_row0, void *workspace,
                         size_t workspace_bytes, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_embed_xw_h_grad";
    TGCN_CHECK(check_sizes(fn, N, K, n));
    TGCN_CHECK(check_h(fn, N, Fh, h_row0));
    EmbedDrop d{};
    bool drop = false;
    TGCN_CHECK(make_embed_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_EMBED_LD("lde", lde, N);
    TGCN_EMBED_LD("ldeh", ldeh, Fh);
    TGCN_EMBED_LD("ldh", ldh, Fh);
    TGCN_EMBED_LD("ldw", ldw, n);
    TGCN_EMBED_LD("ldg", ldg, n);
    if (dE) {
        TGCN_EMBED_LD("ldde", ldde, N);
    }
    if (dEh) {
        TGCN_EMBED_LD("lddeh", lddeh, Fh);
    }
    if (dW) {
        TGCN_EMBED_LD("lddw", lddw, n);
    }
    if ((dE == nullptr) != (dEh == nullptr) || ((dE == nullptr) != (db == nullptr) && N > 0)) {
        set_error("%s: dE, db and dEh are computed together: pass all three or none (db and dEh are sums over dE)", fn);
        return TGCN_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {                              // empty sums; there is no element of dE
        if (db) TGCN_HIP_CHECK(hipMemsetAsync(db, 0, sizeof(float) * K, s));
        if (dEh) TGCN_HIP_CHECK(hipMemset2DAsync(dEh, sizeof(float) * lddeh, 0, sizeof(float) * Fh, K, s));
        if (dW) TGCN_HIP_CHECK(hipMemset2DAsync(dW, sizeof(float) * lddw, 0, sizeof(float) * n, K, s));
        return TGCN_OK;
    }
    TGCN_EMBED_PTR("E", E);
    TGCN_EMBED_PTR("b", b);
    TGCN_EMBED_PTR("Eh", Eh);
    if (h_row0 < N) TGCN_EMBED_PTR("Hd", Hd);
    TGCN_EMBED_PTR("W", W);
    TGCN_EMBED_PTR("G", G);
    if (!dE && !dW) {
        set_error("%s: dE (with db and dEh) and dW are both NULL: nothing to compute", fn);
        return TGCN_E_INVALID;
    }
    const size_t need = std::max(dW ? grad_w_bytes(N, K, n) : 0, dE ? grad_eh_bytes(N, K) : 0);
    if (!workspace || workspace_bytes < need) {            // before anything is enqueued
        set_error("%s: workspace of %zu bytes, tgcn_embed_xw_h_grad_workspace_bytes() asks for %zu", fn, workspace_bytes, need);
        return TGCN_E_INVALID;
    }
    const EmbedH h{Eh, ldeh, Hd, ldh, h_row0, Fh};
    float *part = static_cast<float *>(workspace);
    if (dE) {
        TGCN_CHECK(drop ? launch_h_grad_e<true>(E, lde, b, W, ldw, G, ldg, dE, ldde, db, dEh, lddeh, N, K, n, h, d, part, s)
                        : launch_h_grad_e<false>(E, lde, b, W, ldw, G, ldg, dE, ldde, db, dEh, lddeh, N, K, n, h, d, part, s));
    }
    if (dW) {
        TGCN_CHECK(drop ? launch_h_grad_w<true>(E, lde, b, G, ldg, dW, lddw, N, K, n, h, d, part, s)
                        : launch_h_grad_w<false>(E, lde, b, G, ldg, dW, lddw, N, K, n, h, d, part, s));
    }
    return TGCN_OK;
}

}  // extern "C"
