// The front end of EGCN (reference: textgcn/lib/models.py:28-52) on one-hot features, fused into the first GCNConv's
// x @ W:   Linear(N -> K) on the identity is E^T + b (E = the Linear's [K, N] weight), then SELU, then dropout, then the
// product with W [K, n].  Composed from separate ops that is three N x K fp32 activations (and their gradients) that exist
// only to be contracted against W straight away; here element a(i, k) = s * keep(i, k) * selu(E[k, i] + b[k]) is formed in
// registers on its way into the matrix cores and never stored:
//     tgcn_embed_xw        C[i, :]  = sum_k a(i, k) W[k, :]
//     tgcn_embed_xw_grad   dE[k, i] = s keep(i, k) selu'(E[k, i] + b[k]) sum_j G[i, j] W[k, j],   db[k] = sum_i dE[k, i],
//                          dW[k, j] = sum_i a(i, k) G[i, j]                          (a recomputed, the same mask)
// keep(i, k) is the decision of tgcn_gemm_*_dropout (drop_hash.h) for mask row i, column k.
//
// tgcn_embed_xw_h / tgcn_embed_xw_h_grad are the same products on [I | H] features (the hierarchy features of the
// per-level scripts; text2graph.py:226-246): the Linear's weight is [K, N + Fh], E its first N columns, Eh the last Fh,
// and for the nodes i >= h0 (the document rows)
//     z(i, k) = (E[k, i] + b[k]) + t(i, k),      t(i, k) = sum_f H[i, f] Eh[k, f]   (f ascending, one fma each),
// and dEh joins the gradients.  They are the HIER = true instantiations of the same kernels.
//
// tgcn_embed_xw_members / tgcn_embed_xw_members_grad run the same kernel bodies for M networks of equal widths whose
// parameters are stacked by rows (the EGCN members of a sweep cell): the member is one more grid dimension.
//
// All products run on v_mfma_f32_32x32x2_f32 (fragment maps: fused_act.h).  E's layout suits them: for a fixed k the 32
// nodes of a tile are contiguous, so a wave's operand load is two 128-byte runs and no transpose is needed; the loads are
// scalar dwords because a contiguous [K, N] parameter has 16-byte rows only when N % 4 == 0.
#include <algorithm>

#include "fused_act.h"

namespace tgcn {
namespace {

// ---------------------------------------------------------------------------------------------
// The H term.  t is itself a small product, so it runs on the matrix cores as well: per chunk of 32 k a wave forms the
// 32 x 32 tile T[k, node] = Ehs[k, :] H[node, :]^T in ceil(Fh / 2) MFMA steps (against 16 NT for the main product).  Its
// accumulator registers hold, for the lane's node, 16 values of k -- exactly the 16 pre-activations the lane needs next;
// the forward kernel reads the rows of Ehs through a permutation so that register r of half-wave `half` is k = 2 r + half,
// the A operand order of its own MFMA steps.  The workgroup's chunk of Eh sits in LDS beside the chunk of W (odd row
// stride: the 32 rows a half-wave reads fall into 32 banks).  In the forward and dE the lane's node is fixed, so its H
// values are loaded once: the first 2 kHReg features into registers, the rest (Fh > 16) again per chunk from the caches --
// H is [N_doc, Fh], far below the L2's size.  A wave whose nodes all lie below h0 -- the word rows, two thirds of a TextGCN
// graph -- skips the term through a wave-uniform branch and computes what HIER = false computes, bit for bit.
// ---------------------------------------------------------------------------------------------
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

// The trailing kernel argument: only a HIER kernel is handed an EmbedH.
template <bool HIER>
struct EmbedTail;
template <>
struct EmbedTail<false> {
    RowDrop d;
};
template <>
struct EmbedTail<true> {
    EmbedH h;
    RowDrop d;
};

template <bool HIER>
EmbedTail<HIER> make_tail(const EmbedH *h, const RowDrop &d) {
    if constexpr (HIER) return {*h, d};
    else return {d};
}

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

// ---------------------------------------------------------------------------------------------
// Forward.  A wave owns 32 nodes and all 32 NT result columns; the workgroup's 4 waves share the k chunk of W in LDS
// (W does not fit: 2000 x 200 floats are 1.6 MB, so it goes through 32 rows at a time).  Per MFMA step a lane forms ONE
// element a(i, k) -- its node i is fixed, so the row key of the hash is paid once per lane -- and spends it on NT tiles.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP, bool HIER>
__device__ __forceinline__ void embed_fwd(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                          const float *__restrict__ W, int64_t ldw, float *__restrict__ C, int64_t ldc,
                                          int64_t N, int K, int n, const EmbedTail<HIER> &a) {
    constexpr int KC = 32, NP = 32 * NT;
    __shared__ float Ws[KC * NP];
    __shared__ float Ehs[HIER ? KC * kHLd : 1];            // (HIER = false: never referenced, not allocated)
    __shared__ float bs[KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = (int64_t(blockIdx.x) * 4 + wave) * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    bool wg_h = false, wave_h = false;
    if constexpr (HIER) {
        wg_h = (int64_t(blockIdx.x) + 1) * 128 > a.h.h0;   // some node of the workgroup may have an H row
        wave_h = row0 + 32 > a.h.h0 && row0 < N;           // wave-uniform
    }
    const uint32_t key = row_key<DROP>(a.d, i);
    float hreg[kHReg];
    if constexpr (HIER) {
#pragma unroll
        for (int sp = 0; sp < kHReg; ++sp) hreg[sp] = wave_h ? h_load(a.h, i, N, 2 * sp + half) : 0.f;
    }
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
        if constexpr (HIER) {
            if (wg_h) stage_eh(Ehs, a.h, k0, K, tid);
        }
        float z[KC / 2];
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int k = k0 + 2 * s + half;
            z[s] = (live && k < K) ? E[int64_t(k) * lde + ic] : 0.f;
        }
        __syncthreads();
        if constexpr (HIER) {
#pragma unroll
            for (int s = 0; s < KC / 2; ++s) z[s] = z[s] + bs[2 * s + half];
            if (wave_h) {
                const f32x16 t = h_term<true>(Ehs, hreg, a.h, i, N, c, half);
#pragma unroll
                for (int s = 0; s < KC / 2; ++s) z[s] = z[s] + t[s];
            }
        }
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int kk = 2 * s + half, k = k0 + kk;
            const float av = (live && k < K) ? act<DROP>(HIER ? z[s] : z[s] + bs[kk], key, drop_col_term(k), a.d) : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Ws[kk * NP + 32 * t + c], acc[t], 0, 0, 0);
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

template <int NT, bool DROP, bool HIER>
__global__ __launch_bounds__(256, 2) void k_embed_fwd(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                      const float *__restrict__ W, int64_t ldw, float *__restrict__ C,
                                                      int64_t ldc, int64_t N, int K, int n, const EmbedTail<HIER> a) {
    embed_fwd<NT, DROP, HIER>(E, lde, b, W, ldw, C, ldc, N, K, n, a);
}

// ---------------------------------------------------------------------------------------------
// M members in one launch (tgcn_embed_xw_members*): E, b, Eh, W and their gradients are stacked by rows -- member m owns
// the rows [m K, (m + 1) K) -- and C / G by columns, member m owning [m nm, (m + 1) nm).  The member is one more grid
// dimension: it moves the operands to the member's blocks, selects the member's seed, threshold and scale, and runs the
// kernel body above on them -- the same arithmetic in the same order as the single call with that member's slices, so
// the same bits.  A member at rate 0 has threshold 0 and scale 1: every element is kept and x * 1.f is x.
// ---------------------------------------------------------------------------------------------
constexpr int kMaxMembers = 64;

struct MemberDrop {
    uint32_t thresh[kMaxMembers];
    float scale[kMaxMembers];
};

template <bool DROP, bool HIER>
__device__ __forceinline__ EmbedTail<HIER> member_tail(const EmbedTail<HIER> &a, const MemberDrop &md, int m, int K) {
    EmbedTail<HIER> t = a;
    if constexpr (HIER) t.h.Eh += int64_t(m) * K * t.h.ldeh;
    if constexpr (DROP) {
        t.d.seed += m;
        t.d.thresh = md.thresh[m];
        t.d.scale = md.scale[m];
    }
    return t;
}

template <int NT, bool DROP, bool HIER>
__global__ __launch_bounds__(256, 2) void k_embed_fwd_members(const float *__restrict__ E, int64_t lde,
                                                              const float *__restrict__ b, const float *__restrict__ W,
                                                              int64_t ldw, float *__restrict__ C, int64_t ldc, int64_t N,
                                                              int K, int n, int nm, const EmbedTail<HIER> a,
                                                              const MemberDrop md) {
    const int m = blockIdx.y;
    const int64_t r0 = int64_t(m) * K;
    embed_fwd<NT, DROP, HIER>(E + r0 * lde, lde, b + r0, W + r0 * ldw, ldw, C + int64_t(m) * nm, ldc, N, K, n,
                              member_tail<DROP, HIER>(a, md, m, K));
}

// ---------------------------------------------------------------------------------------------
// dE, in E's layout.  The tile is computed transposed, T[k, i] = sum_j W[k, j] G[i, j], so that the 32 nodes of a tile are
// the lanes of a store (two 128-byte runs per register).  A wave keeps its 32 rows of G in registers (the B operand; loaded
// once, reused over all K / 32 tiles of k), the workgroup shares the 32 rows of W in LDS, transposed with an odd stride so
// that neither the staging writes nor the operand reads conflict.  `accum`: the reduction over j is longer than one launch
// covers (n > 256) and this is not its first piece: the masked, scaled partial sum is added to what dE holds.
// (dEh needs the FINISHED dE -- with n > 256 it is the sum of several launches -- so it is a product of its own:
// k_embed_h_grad_eh.)
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP, bool HIER>
__device__ __forceinline__ void embed_grad_e(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                             const float *__restrict__ W, int64_t ldw, const float *__restrict__ G,
                                             int64_t ldg, float *__restrict__ dE, int64_t ldde, int64_t N, int K, int n,
                                             int accum, const EmbedTail<HIER> &a) {
    constexpr int NP = 32 * NT, LDW = 33;
    __shared__ float Ws[NP * LDW];
    __shared__ float Ehs[HIER ? 32 * kHLd : 1];
    __shared__ float bs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = (int64_t(blockIdx.x) * 4 + wave) * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    bool wg_h = false, wave_h = false;
    if constexpr (HIER) {
        wg_h = (int64_t(blockIdx.x) + 1) * 128 > a.h.h0;
        wave_h = row0 + 32 > a.h.h0 && row0 < N;
    }
    const uint32_t key = row_key<DROP>(a.d, i);
    float hreg[kHReg];
    if constexpr (HIER) {
#pragma unroll
        for (int sp = 0; sp < kHReg; ++sp) hreg[sp] = wave_h ? h_load(a.h, i, N, 2 * sp + half) : 0.f;
    }
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
        if constexpr (HIER) {
            if (wg_h) stage_eh(Ehs, a.h, k0, K, tid);
        }
        float z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + acc_row(r, half);
            z[r] = (live && k < K) ? E[int64_t(k) * lde + ic] : 0.f;
        }
        __syncthreads();
        if constexpr (HIER) {
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = z[r] + bs[acc_row(r, half)];
            if (wave_h) {
                const f32x16 t = h_term<false>(Ehs, hreg, a.h, i, N, c, half);
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = z[r] + t[r];
            }
        }
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
                float v = acc[r] * selu_grad_f(HIER ? z[r] : z[r] + bs[kk]);
                if constexpr (DROP) v = drop_hash_keep(key, drop_col_term(k), a.d.thresh) ? v * a.d.scale : 0.f;
                float *out = dE + int64_t(k) * ldde + ic;
                *out = accum ? *out + v : v;
            }
        }
    }
}

template <int NT, bool DROP, bool HIER>
__global__ __launch_bounds__(256, 2) void k_embed_grad_e(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                         const float *__restrict__ W, int64_t ldw,
                                                         const float *__restrict__ G, int64_t ldg, float *__restrict__ dE,
                                                         int64_t ldde, int64_t N, int K, int n, int accum,
                                                         const EmbedTail<HIER> a) {
    embed_grad_e<NT, DROP, HIER>(E, lde, b, W, ldw, G, ldg, dE, ldde, N, K, n, accum, a);
}

template <int NT, bool DROP, bool HIER>
__global__ __launch_bounds__(256, 2) void k_embed_grad_e_members(const float *__restrict__ E, int64_t lde,
                                                                 const float *__restrict__ b, const float *__restrict__ W,
                                                                 int64_t ldw, const float *__restrict__ G, int64_t ldg,
                                                                 float *__restrict__ dE, int64_t ldde, int64_t N, int K,
                                                                 int n, int nm, int accum, const EmbedTail<HIER> a,
                                                                 const MemberDrop md) {
    const int m = blockIdx.y;
    const int64_t r0 = int64_t(m) * K;
    embed_grad_e<NT, DROP, HIER>(E + r0 * lde, lde, b + r0, W + r0 * ldw, ldw, G + int64_t(m) * nm, ldg, dE + r0 * ldde, ldde,
                                 N, K, n, accum, member_tail<DROP, HIER>(a, md, m, K));
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
// MFMA step takes only two reduction indices across the lanes, so the tile of a goes through LDS: the workgroup forms
// a(i, k) ONCE per element for 32 rows of k x 128 nodes and stores it with an odd row stride; the matrix cores then read it
// as the A operand (row k per lane) without conflicts.  The tile is staged in one of two ways:
//   plain  the workgroup reads its 32 rows of E coalesced: a lane takes nodes lane and lane + 64 of 8 rows of k.
//   HIER   the nodes change from tile to tile, so the tile is staged by (node = wave * 32 + c, k = acc_row(r, half)) --
//          the layout in which the matrix cores deliver t -- and the H operand of a tile is read once, where the tile is
//          formed.  The workgroup's k tile is fixed: its rows of Eh are staged once.
// The 4 waves split the result columns (TW tiles of 32 each) and read their slab of G straight from memory, 128 bytes per
// half wave.  blockIdx.x is the tile of k, blockIdx.y a slice of the nodes; the slices' partial sums go to the workspace
// and are added in a fixed order by k_reduce_slices.
// ---------------------------------------------------------------------------------------------
template <int TW, bool DROP, bool HIER>
__device__ __forceinline__ void embed_grad_w(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                             const float *__restrict__ G, int64_t ldg, float *__restrict__ part, int64_t N,
                                             int K, int n, int64_t chunks_per_slice, const EmbedTail<HIER> &a) {
    constexpr int LDA = kWChunk + 1, NP = 128 * TW;
    __shared__ float As[32 * LDA];
    __shared__ float Ehs[HIER ? 32 * kHLd : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int k0 = blockIdx.x * 32, kpad = gridDim.x * 32;
    const int64_t i_begin = int64_t(blockIdx.y) * chunks_per_slice * kWChunk;
    const int64_t i_stop = i_begin + chunks_per_slice * kWChunk;
    const int64_t i_end = i_stop < N ? i_stop : N;
    const bool computes = wave * TW * 32 < n;             // a wave whose columns are all padding only helps staging
    float bk[HIER ? 16 : 8];                               // b at the lane's values of k
    int pairs = 0;
    bool slice_h = false;
    if constexpr (HIER) {
        pairs = (a.h.Fh + 1) >> 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) bk[r] = k0 + acc_row(r, half) < K ? b[k0 + acc_row(r, half)] : 0.f;
        slice_h = i_end > a.h.h0;                          // some node of the slice has an H row
        if (slice_h) stage_eh(Ehs, a.h, k0, K, tid);       // (read after the first barrier of the loop)
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) bk[u] = k0 + wave * 8 + u < K ? b[k0 + wave * 8 + u] : 0.f;
    }
    f32x16 acc[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int64_t i0 = i_begin; i0 < i_end; i0 += kWChunk) {
        if constexpr (HIER) {
            const int64_t w0 = i0 + wave * 32, i = w0 + c;
            const bool live = i < i_end;
            float z[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + acc_row(r, half);
                z[r] = (live && k < K) ? E[int64_t(k) * lde + i] : 0.f;
            }
            __syncthreads();                               // the previous tile has been read (and Ehs is staged)
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = z[r] + bk[r];
            if (slice_h && w0 + 32 > a.h.h0 && w0 < i_end) {   // wave-uniform
                f32x16 t;
#pragma unroll
                for (int r = 0; r < 16; ++r) t[r] = 0.f;
                for (int sp = 0; sp < pairs; ++sp)
                    t = __builtin_amdgcn_mfma_f32_32x32x2f32(Ehs[c * kHLd + 2 * sp + half],
                                                             h_load(a.h, i, i_end, 2 * sp + half), t, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = z[r] + t[r];
            }
            const uint32_t key = row_key<DROP>(a.d, i);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kk = acc_row(r, half), k = k0 + kk;
                As[kk * LDA + wave * 32 + c] = (live && k < K) ? act<DROP>(z[r], key, drop_col_term(k), a.d) : 0.f;
            }
        } else {
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
            __syncthreads();                               // the previous tile has been read
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int64_t i = i0 + lane + 64 * v;
                const uint32_t key = row_key<DROP>(a.d, i);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int kk = wave * 8 + u, k = k0 + kk;
                    As[kk * LDA + lane + 64 * v] =
                        (i < i_end && k < K) ? act<DROP>(z[v][u] + bk[u], key, drop_col_term(k), a.d) : 0.f;
                }
            }
        }
        __syncthreads();
        if (computes) {
#pragma unroll 8
            for (int s = 0; s < kWChunk / 2; ++s) {
                const int ii = 2 * s + half;
                const int64_t i = i0 + ii;
                const float av = As[c * LDA + ii];
#pragma unroll
                for (int t = 0; t < TW; ++t) {
                    const int j = (wave * TW + t) * 32 + c;
                    const float gv = (i < i_end && j < n) ? G[i * ldg + j] : 0.f;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, gv, acc[t], 0, 0, 0);
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

template <int TW, bool DROP, bool HIER>
__global__ __launch_bounds__(256, 2) void k_embed_grad_w(const float *__restrict__ E, int64_t lde, const float *__restrict__ b,
                                                         const float *__restrict__ G, int64_t ldg, float *__restrict__ part,
                                                         int64_t N, int K, int n, int64_t chunks_per_slice,
                                                         const EmbedTail<HIER> a) {
    embed_grad_w<TW, DROP, HIER>(E, lde, b, G, ldg, part, N, K, n, chunks_per_slice, a);
}

// blockIdx.z is the member; `part_stride`: the floats of one member's partial sums (the single call's workspace)
template <int TW, bool DROP, bool HIER>
__global__ __launch_bounds__(256, 2) void k_embed_grad_w_members(const float *__restrict__ E, int64_t lde,
                                                                 const float *__restrict__ b, const float *__restrict__ G,
                                                                 int64_t ldg, float *__restrict__ part, int64_t part_stride,
                                                                 int64_t N, int K, int n, int nm, int64_t chunks_per_slice,
                                                                 const EmbedTail<HIER> a, const MemberDrop md) {
    const int m = blockIdx.z;
    const int64_t r0 = int64_t(m) * K;
    embed_grad_w<TW, DROP, HIER>(E + r0 * lde, lde, b + r0, G + int64_t(m) * nm, ldg, part + m * part_stride, N, K, n,
                                 chunks_per_slice, member_tail<DROP, HIER>(a, md, m, K));
}

// dEh[k, f] = sum_{i >= h0} dE[k, i] H[i, f]: the reduction over the nodes that the kernels above do not have.  The shape
// of k_embed_grad_w with the finished dE in the place of the activation: blockIdx.x is the tile of k, blockIdx.y one of a
// FIXED number of slices of the nodes from h0 on; the workgroup stages 32 rows of dE x 128 nodes, the 4 waves take the
// (at most 4) tiles of 32 features and read their rows of H straight from memory.  The slices' partial sums [32, 128] go
// to the workspace and k_reduce_slices adds them in slice order: no atomics, the same bits every run.
__device__ __forceinline__ void embed_h_grad_eh(const float *__restrict__ dE, int64_t ldde, float *__restrict__ part,
                                                int64_t N, int K, int64_t chunks_per_slice, const EmbedH &h) {
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

__global__ __launch_bounds__(256, 2) void k_embed_h_grad_eh(const float *__restrict__ dE, int64_t ldde, float *__restrict__ part,
                                                            int64_t N, int K, int64_t chunks_per_slice, const EmbedH h) {
    embed_h_grad_eh(dE, ldde, part, N, K, chunks_per_slice, h);
}

// blockIdx.z is the member (Eh is not read here: H and h0 are the members' common ones)
__global__ __launch_bounds__(256, 2) void k_embed_h_grad_eh_members(const float *__restrict__ dE, int64_t ldde,
                                                                    float *__restrict__ part, int64_t part_stride, int64_t N,
                                                                    int K, int64_t chunks_per_slice, const EmbedH h) {
    const int m = blockIdx.z;
    embed_h_grad_eh(dE + int64_t(m) * K * ldde, ldde, part + m * part_stride, N, K, chunks_per_slice, h);
}

// k_reduce_slices for every member: blockIdx.y is the member, whose rows of `out` follow those of the member before
__global__ __launch_bounds__(256) void k_reduce_slices_members(const float *__restrict__ part, int64_t part_stride, int slices,
                                                               int64_t slice_stride, int row_stride, int rows, int cols,
                                                               float *__restrict__ out, int64_t ld) {
    const int m = blockIdx.y;
    reduce_slices(part + m * part_stride, slices, slice_stride, row_stride, rows, cols, out + int64_t(m) * rows * ld, ld);
}

constexpr int kFwdGroup = 256;   // result columns of one forward launch / reduction length of one dE launch (8 tiles)
constexpr int kWGroup = 256;     // result columns of one dW launch (4 waves x 2 tiles)
constexpr int kWTarget = 1024;   // workgroups of a dW launch, about (grad_w_split)

size_t grad_w_bytes(int64_t N, int K, int n) {
    int64_t slices, cps;
    grad_w_split(N, K, kWTarget, slices, cps);
    const int64_t kpad = (int64_t(K) + 31) / 32 * 32;
    const int64_t np = std::min(n, kWGroup) > 128 ? 256 : 128;
    return static_cast<size_t>(slices * kpad * np) * sizeof(float);
}

// the partial sums of dEh use the workspace after those of dW.  dEh's nodes are cut with the chunks-per-slice that the
// whole N would get, so that a later h0 only means fewer slices.
size_t grad_eh_bytes(int64_t N, int K) {
    int64_t slices, cps;
    grad_w_split(N, K, kWTarget, slices, cps);
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

// The launchers: h == nullptr runs the HIER = false kernels.
template <class F>
void with_hier(const EmbedH *h, const RowDrop &d, F &&f) {
    if (!h) f(std::false_type{}, make_tail<false>(h, d));
    else f(std::true_type{}, make_tail<true>(h, d));
}

template <bool DROP>
int launch_fwd(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
               int K, int n, const EmbedH *h, const RowDrop &d, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup);
        with_tiles<1, 2, 4, 7, 8>((ng + 31) / 32, [&](auto nt) {
            with_hier(h, d, [&](auto hier, const auto &tail) {
                hipLaunchKernelGGL((k_embed_fwd<decltype(nt)::value, DROP, decltype(hier)::value>), dim3(grid), dim3(256), 0,
                                   s, E, lde, b, W + col0, ldw, C + col0, ldc, N, K, ng, tail);
            });
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// dE and db, and with h also dEh (through `part`, which only that one needs)
template <bool DROP>
int launch_grad_e(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, const float *G, int64_t ldg,
                  float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, int64_t N, int K, int n, const EmbedH *h,
                  const RowDrop &d, float *part, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup), accum = col0 > 0;
        with_tiles<1, 2, 4, 7, 8>((ng + 31) / 32, [&](auto nt) {
            with_hier(h, d, [&](auto hier, const auto &tail) {
                hipLaunchKernelGGL((k_embed_grad_e<decltype(nt)::value, DROP, decltype(hier)::value>), dim3(grid), dim3(256),
                                   0, s, E, lde, b, W + col0, ldw, G + col0, ldg, dE, ldde, N, K, ng, accum, tail);
            });
        });
    }
    hipLaunchKernelGGL(k_embed_rowsum, dim3(K), dim3(256), 0, s, dE, ldde, N, db);
    if (h && h->h0 == N) {                     // nobody has an H row: an empty sum
        TGCN_HIP_CHECK(hipMemset2DAsync(dEh, sizeof(float) * lddeh, 0, sizeof(float) * h->Fh, K, s));
    } else if (h) {
        int64_t slices, cps;
        grad_w_split(N, K, kWTarget, slices, cps);
        const int64_t chunks = (N - h->h0 + kWChunk - 1) / kWChunk;
        slices = (chunks + cps - 1) / cps;     // <= the slices of the whole N, which the workspace is sized for
        const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
        hipLaunchKernelGGL(k_embed_h_grad_eh, dim3(ktiles, static_cast<unsigned>(slices)), dim3(256), 0, s, dE, ldde, part, N, K,
                           cps, *h);
        launch_reduce_slices(part, slices, int64_t(kpad) * kHMax, kHMax, K, h->Fh, dEh, lddeh, s);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_grad_w(const float *E, int64_t lde, const float *b, const float *G, int64_t ldg, float *dW, int64_t lddw,
                  int64_t N, int K, int n, const EmbedH *h, const RowDrop &d, float *part, hipStream_t s) {
    int64_t slices, cps;
    grad_w_split(N, K, kWTarget, slices, cps);
    const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
    const dim3 grid(ktiles, static_cast<unsigned>(slices));
    for (int col0 = 0; col0 < n; col0 += kWGroup) {
        const int ng = std::min(n - col0, kWGroup);
        with_hier(h, d, [&](auto hier, const auto &tail) {
            constexpr bool HIER = decltype(hier)::value;
            if (ng > 128)
                hipLaunchKernelGGL((k_embed_grad_w<2, DROP, HIER>), grid, dim3(256), 0, s, E, lde, b, G + col0, ldg, part, N,
                                   K, ng, cps, tail);
            else
                hipLaunchKernelGGL((k_embed_grad_w<1, DROP, HIER>), grid, dim3(256), 0, s, E, lde, b, G + col0, ldg, part, N,
                                   K, ng, cps, tail);
        });
        const int np = ng > 128 ? 256 : 128;
        launch_reduce_slices(part, slices, int64_t(kpad) * np, np, K, ng, dW + col0, lddw, s);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// tgcn_embed_xw (h == nullptr) and tgcn_embed_xw_h
int embed_xw(const char *fn, const float *E, int64_t lde, const float *b, const EmbedH *h, const float *W, int64_t ldw,
             float *C, int64_t ldc, int64_t N, int K, int n, double p, const uint64_t *seed, int64_t mask_row0,
             tgcn_stream stream) {
    TGCN_CHECK(check_sizes(fn, "K", N, K, n));
    if (h) TGCN_CHECK(check_h(fn, N, h->Fh, h->h0));
    RowDrop d{};
    bool drop = false;
    TGCN_CHECK(make_row_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_CHECK(check_ld(fn, "lde", lde, N));
    if (h) {
        TGCN_CHECK(check_ld(fn, "ldeh", h->ldeh, h->Fh));
        TGCN_CHECK(check_ld(fn, "ldh", h->ldh, h->Fh));
    }
    TGCN_CHECK(check_ld(fn, "ldw", ldw, n));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, n));
    if (N == 0) return TGCN_OK;                // (an empty tensor's pointer may be NULL)
    TGCN_CHECK(check_ptr(fn, "E", E));
    TGCN_CHECK(check_ptr(fn, "b", b));
    if (h) {
        TGCN_CHECK(check_ptr(fn, "Eh", h->Eh));
        if (h->h0 < N) TGCN_CHECK(check_ptr(fn, "Hd", h->Hd));
    }
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "C", C));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return drop ? launch_fwd<true>(E, lde, b, W, ldw, C, ldc, N, K, n, h, d, s)
                : launch_fwd<false>(E, lde, b, W, ldw, C, ldc, N, K, n, h, d, s);
}

// tgcn_embed_xw_grad (h == nullptr; dEh is not looked at) and tgcn_embed_xw_h_grad.  The two differ in when the workspace
// is checked and in the status of a short one: the plain gradient checks it where dW needs it, after dE has been enqueued,
// and returns TGCN_E_WORKSPACE; the H gradient checks before anything is enqueued and returns TGCN_E_INVALID.
int embed_xw_grad(const char *fn, const float *E, int64_t lde, const float *b, const EmbedH *h, const float *W, int64_t ldw,
                  const float *G, int64_t ldg, float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, float *dW,
                  int64_t lddw, int64_t N, int K, int n, double p, const uint64_t *seed, int64_t mask_row0, void *workspace,
                  size_t workspace_bytes, tgcn_stream stream) {
    TGCN_CHECK(check_sizes(fn, "K", N, K, n));
    if (h) TGCN_CHECK(check_h(fn, N, h->Fh, h->h0));
    RowDrop d{};
    bool drop = false;
    TGCN_CHECK(make_row_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_CHECK(check_ld(fn, "lde", lde, N));
    if (h) {
        TGCN_CHECK(check_ld(fn, "ldeh", h->ldeh, h->Fh));
        TGCN_CHECK(check_ld(fn, "ldh", h->ldh, h->Fh));
    }
    TGCN_CHECK(check_ld(fn, "ldw", ldw, n));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, n));
    if (dE) TGCN_CHECK(check_ld(fn, "ldde", ldde, N));
    if (h && dEh) TGCN_CHECK(check_ld(fn, "lddeh", lddeh, h->Fh));
    if (dW) TGCN_CHECK(check_ld(fn, "lddw", lddw, n));
    const bool db_apart = (dE == nullptr) != (db == nullptr) && N > 0;
    if (h && ((dE == nullptr) != (dEh == nullptr) || db_apart)) {
        set_error("%s: dE, db and dEh are computed together: pass all three or none (db and dEh are sums over dE)", fn);
        return TGCN_E_INVALID;
    }
    if (!h && db_apart) {
        set_error("%s: dE and db are computed together: pass both or neither (db is the row sum of dE)", fn);
        return TGCN_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {                              // empty sums; there is no element of dE
        if (db) TGCN_HIP_CHECK(hipMemsetAsync(db, 0, sizeof(float) * K, s));
        if (h && dEh) TGCN_HIP_CHECK(hipMemset2DAsync(dEh, sizeof(float) * lddeh, 0, sizeof(float) * h->Fh, K, s));
        if (dW) TGCN_HIP_CHECK(hipMemset2DAsync(dW, sizeof(float) * lddw, 0, sizeof(float) * n, K, s));
        return TGCN_OK;
    }
    TGCN_CHECK(check_ptr(fn, "E", E));
    TGCN_CHECK(check_ptr(fn, "b", b));
    if (h) {
        TGCN_CHECK(check_ptr(fn, "Eh", h->Eh));
        if (h->h0 < N) TGCN_CHECK(check_ptr(fn, "Hd", h->Hd));
    }
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "G", G));
    if (!dE && !dW) {
        set_error("%s: dE (with %s) and dW are both NULL: nothing to compute", fn, h ? "db and dEh" : "db");
        return TGCN_E_INVALID;
    }
    const auto workspace_holds = [&](size_t need) {
        if (workspace && workspace_bytes >= need) return true;
        set_error("%s: workspace of %zu bytes, %s_workspace_bytes() asks for %zu", fn, workspace_bytes, fn, need);
        return false;
    };
    if (h && !workspace_holds(std::max(dW ? grad_w_bytes(N, K, n) : 0, dE ? grad_eh_bytes(N, K) : 0))) return TGCN_E_INVALID;
    float *part = static_cast<float *>(workspace);
    if (dE) {
        TGCN_CHECK(drop ? launch_grad_e<true>(E, lde, b, W, ldw, G, ldg, dE, ldde, db, dEh, lddeh, N, K, n, h, d, part, s)
                        : launch_grad_e<false>(E, lde, b, W, ldw, G, ldg, dE, ldde, db, dEh, lddeh, N, K, n, h, d, part, s));
    }
    if (dW) {
        if (!h && !workspace_holds(grad_w_bytes(N, K, n))) return TGCN_E_WORKSPACE;
        TGCN_CHECK(drop ? launch_grad_w<true>(E, lde, b, G, ldg, dW, lddw, N, K, n, h, d, part, s)
                        : launch_grad_w<false>(E, lde, b, G, ldg, dW, lddw, N, K, n, h, d, part, s));
    }
    return TGCN_OK;
}

// ---------------------------------------------------------------------------------------------
// The member-batched calls.  Every launch below is the single call's with the member as one more grid dimension, so
// the number of launches does not depend on M.
// ---------------------------------------------------------------------------------------------
size_t members_part_bytes(int64_t N, int K, int n, int Fh) {   // one member's partial sums: the single call's workspace
    return Fh > 0 ? std::max(grad_w_bytes(N, K, n), grad_eh_bytes(N, K)) : grad_w_bytes(N, K, n);
}

struct MembersArgs {
    const float *E;
    int64_t lde;
    const float *b;
    const float *W;
    int64_t ldw;
    int64_t N;
    int K, n, M;
    const EmbedH *h;           // nullptr: identity features
    RowDrop d;                 // seed: the members' seeds [M]; thresh and scale are the member's (MemberDrop)
    MemberDrop md;
    hipStream_t s;
};

template <bool DROP>
int launch_fwd_members(const MembersArgs &a, float *C, int64_t ldc) {
    const dim3 grid(static_cast<unsigned>((a.N + 127) / 128), a.M);
    for (int col0 = 0; col0 < a.n; col0 += kFwdGroup) {
        const int ng = std::min(a.n - col0, kFwdGroup);
        with_tiles<1, 2, 4, 7, 8>((ng + 31) / 32, [&](auto nt) {
            with_hier(a.h, a.d, [&](auto hier, const auto &tail) {
                hipLaunchKernelGGL((k_embed_fwd_members<decltype(nt)::value, DROP, decltype(hier)::value>), grid, dim3(256), 0,
                                   a.s, a.E, a.lde, a.b, a.W + col0, a.ldw, C + col0, ldc, a.N, a.K, ng, a.n, tail, a.md);
            });
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_grad_e_members(const MembersArgs &a, const float *G, int64_t ldg, float *dE, int64_t ldde, float *db, float *dEh,
                          int64_t lddeh, float *part, int64_t part_stride) {
    const dim3 grid(static_cast<unsigned>((a.N + 127) / 128), a.M);
    const int rows = a.M * a.K;
    for (int col0 = 0; col0 < a.n; col0 += kFwdGroup) {
        const int ng = std::min(a.n - col0, kFwdGroup), accum = col0 > 0;
        with_tiles<1, 2, 4, 7, 8>((ng + 31) / 32, [&](auto nt) {
            with_hier(a.h, a.d, [&](auto hier, const auto &tail) {
                hipLaunchKernelGGL((k_embed_grad_e_members<decltype(nt)::value, DROP, decltype(hier)::value>), grid,
                                   dim3(256), 0, a.s, a.E, a.lde, a.b, a.W + col0, a.ldw, G + col0, ldg, dE, ldde, a.N, a.K,
                                   ng, a.n, accum, tail, a.md);
            });
        });
    }
    hipLaunchKernelGGL(k_embed_rowsum, dim3(rows), dim3(256), 0, a.s, dE, ldde, a.N, db);   // the members' rows are stacked
    const EmbedH *h = a.h;
    if (h && h->h0 == a.N) {
        TGCN_HIP_CHECK(hipMemset2DAsync(dEh, sizeof(float) * lddeh, 0, sizeof(float) * h->Fh, rows, a.s));
    } else if (h) {
        int64_t slices, cps;
        grad_w_split(a.N, a.K, kWTarget, slices, cps);
        const int64_t chunks = (a.N - h->h0 + kWChunk - 1) / kWChunk;
        slices = (chunks + cps - 1) / cps;
        const int ktiles = (a.K + 31) / 32, kpad = ktiles * 32;
        hipLaunchKernelGGL(k_embed_h_grad_eh_members, dim3(ktiles, static_cast<unsigned>(slices), a.M), dim3(256), 0, a.s, dE,
                           ldde, part, part_stride, a.N, a.K, cps, *h);
        const dim3 rgrid(static_cast<unsigned>((int64_t(a.K) * h->Fh + 255) / 256), a.M);
        hipLaunchKernelGGL(k_reduce_slices_members, rgrid, dim3(256), 0, a.s, part, part_stride, static_cast<int>(slices),
                           int64_t(kpad) * kHMax, kHMax, a.K, h->Fh, dEh, lddeh);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_grad_w_members(const MembersArgs &a, const float *G, int64_t ldg, float *dW, int64_t lddw, float *part,
                          int64_t part_stride) {
    int64_t slices, cps;
    grad_w_split(a.N, a.K, kWTarget, slices, cps);
    const int ktiles = (a.K + 31) / 32, kpad = ktiles * 32;
    const dim3 grid(ktiles, static_cast<unsigned>(slices), a.M);
    for (int col0 = 0; col0 < a.n; col0 += kWGroup) {
        const int ng = std::min(a.n - col0, kWGroup);
        with_hier(a.h, a.d, [&](auto hier, const auto &tail) {
            constexpr bool HIER = decltype(hier)::value;
            if (ng > 128)
                hipLaunchKernelGGL((k_embed_grad_w_members<2, DROP, HIER>), grid, dim3(256), 0, a.s, a.E, a.lde, a.b, G + col0,
                                   ldg, part, part_stride, a.N, a.K, ng, a.n, cps, tail, a.md);
            else
                hipLaunchKernelGGL((k_embed_grad_w_members<1, DROP, HIER>), grid, dim3(256), 0, a.s, a.E, a.lde, a.b, G + col0,
                                   ldg, part, part_stride, a.N, a.K, ng, a.n, cps, tail, a.md);
        });
        const int np = ng > 128 ? 256 : 128;
        const dim3 rgrid(static_cast<unsigned>((int64_t(a.K) * ng + 255) / 256), a.M);
        hipLaunchKernelGGL(k_reduce_slices_members, rgrid, dim3(256), 0, a.s, part, part_stride, static_cast<int>(slices),
                           int64_t(kpad) * np, np, a.K, ng, dW + col0, lddw);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// the checks the two member calls share; fills `a` (but for the stream) and `drop`
int members_args(const char *fn, const float *E, int64_t lde, const float *b, const EmbedH &h, const float *W, int64_t ldw,
                 int64_t N, int K, int n, int M, const double *p_host, const uint64_t *seeds, int64_t mask_row0, MembersArgs &a,
                 bool &drop) {
    TGCN_CHECK(check_sizes(fn, "K", N, K, n));
    if (M < 1 || M > kMaxMembers) {
        set_error("%s: n_members must be in [1, %d] (n_members=%d)", fn, kMaxMembers, M);
        return TGCN_E_INVALID;
    }
    if (int64_t(M) * K > INT32_MAX || int64_t(M) * n > INT32_MAX) {
        set_error("%s: n_members * K and n_members * n must fit 32 bits", fn);
        return TGCN_E_INVALID;
    }
    if (h.Fh < 0 || h.Fh > kHMax) {
        set_error("%s: Fh must be in [0, %d] (tgcn_embed_xw_h_max_features; 0: identity features) (Fh=%d)", fn, kHMax, h.Fh);
        return TGCN_E_INVALID;
    }
    if (h.h0 < 0 || h.h0 > N) {
        set_error("%s: h_row0 must be in [0, N] (h_row0=%lld, N=%lld)", fn, (long long)h.h0, (long long)N);
        return TGCN_E_INVALID;
    }
    TGCN_CHECK(check_ptr(fn, "p_host", p_host));
    if (mask_row0 < 0) {
        set_error("%s: mask_row0 must be >= 0 (%lld)", fn, (long long)mask_row0);
        return TGCN_E_INVALID;
    }
    a = MembersArgs{};
    drop = false;
    for (int m = 0; m < M; ++m) {
        const double p = p_host[m];
        if (!(p >= 0.0 && p < 1.0)) {
            set_error("%s: every member's p must be in [0, 1) (p[%d]=%g)", fn, m, p);
            return TGCN_E_INVALID;
        }
        const bool on = p > 0.0 && seeds != nullptr;      // (make_row_drop's values, member by member)
        a.md.thresh[m] = on ? drop_threshold(p) : 0u;
        a.md.scale[m] = on ? static_cast<float>(1.0 / (1.0 - p)) : 1.f;
        drop = drop || on;
    }
    TGCN_CHECK(check_ld(fn, "lde", lde, N));
    if (h.Fh > 0) {
        TGCN_CHECK(check_ld(fn, "ldeh", h.ldeh, h.Fh));
        TGCN_CHECK(check_ld(fn, "ldh", h.ldh, h.Fh));
    }
    TGCN_CHECK(check_ld(fn, "ldw", ldw, n));
    a.E = E, a.lde = lde, a.b = b, a.W = W, a.ldw = ldw, a.N = N, a.K = K, a.n = n, a.M = M;
    a.h = h.Fh > 0 ? &h : nullptr;
    a.d = RowDrop{seeds, 0u, 1.f, mask_row0};
    return TGCN_OK;
}

int members_ptrs(const char *fn, const MembersArgs &a) {
    TGCN_CHECK(check_ptr(fn, "E", a.E));
    TGCN_CHECK(check_ptr(fn, "b", a.b));
    if (a.h) {
        TGCN_CHECK(check_ptr(fn, "Eh", a.h->Eh));
        if (a.h->h0 < a.N) TGCN_CHECK(check_ptr(fn, "Hd", a.h->Hd));
    }
    TGCN_CHECK(check_ptr(fn, "W", a.W));
    return TGCN_OK;
}

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_embed_xw(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, float *C, int64_t ldc,
                  int64_t N, int K, int n, double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream) {
    return tgcn::embed_xw("tgcn_embed_xw", E, lde, b, nullptr, W, ldw, C, ldc, N, K, n, p, seed, mask_row0, stream);
}

size_t tgcn_embed_xw_grad_workspace_bytes(int64_t N, int K, int n) {
    if (N < 0 || K <= 0 || n <= 0) return 0;
    return tgcn::grad_w_bytes(N, K, n);
}

int tgcn_embed_xw_grad(const float *E, int64_t lde, const float *b, const float *W, int64_t ldw, const float *G,
                       int64_t ldg, float *dE, int64_t ldde, float *db, float *dW, int64_t lddw, int64_t N, int K, int n,
                       double p, const uint64_t *seed, int64_t mask_row0, void *workspace, size_t workspace_bytes,
                       tgcn_stream stream) {
    return tgcn::embed_xw_grad("tgcn_embed_xw_grad", E, lde, b, nullptr, W, ldw, G, ldg, dE, ldde, db, nullptr, 0, dW, lddw, N,
                               K, n, p, seed, mask_row0, workspace, workspace_bytes, stream);
}

int tgcn_embed_xw_h_max_features(void) { return tgcn::kHMax; }

int tgcn_embed_xw_h(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd, int64_t ldh,
                    int64_t h_row0, int Fh, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N, int K, int n,
                    double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream) {
    const tgcn::EmbedH h{Eh, ldeh, Hd, ldh, h_row0, Fh};
    return tgcn::embed_xw("tgcn_embed_xw_h", E, lde, b, &h, W, ldw, C, ldc, N, K, n, p, seed, mask_row0, stream);
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
    const tgcn::EmbedH h{Eh, ldeh, Hd, ldh, h_row0, Fh};
    return tgcn::embed_xw_grad("tgcn_embed_xw_h_grad", E, lde, b, &h, W, ldw, G, ldg, dE, ldde, db, dEh, lddeh, dW, lddw, N, K,
                               n, p, seed, mask_row0, workspace, workspace_bytes, stream);
}

int tgcn_embed_xw_members(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd,
                          int64_t ldh, int64_t h_row0, int Fh, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
                          int K, int n, int n_members, const double *p_host, const uint64_t *seeds, int64_t mask_row0,
                          tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_embed_xw_members";
    const EmbedH h{Eh, ldeh, Hd, ldh, h_row0, Fh};
    MembersArgs a;
    bool drop = false;
    TGCN_CHECK(members_args(fn, E, lde, b, h, W, ldw, N, K, n, n_members, p_host, seeds, mask_row0, a, drop));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, int64_t(n_members) * n));
    if (N == 0) return TGCN_OK;
    TGCN_CHECK(members_ptrs(fn, a));
    TGCN_CHECK(check_ptr(fn, "C", C));
    a.s = static_cast<hipStream_t>(stream);
    return drop ? launch_fwd_members<true>(a, C, ldc) : launch_fwd_members<false>(a, C, ldc);
}

size_t tgcn_embed_xw_members_grad_workspace_bytes(int64_t N, int K, int n, int Fh, int n_members) {
    if (N < 0 || K <= 0 || n <= 0 || Fh < 0 || Fh > tgcn::kHMax || n_members < 1 || n_members > tgcn::kMaxMembers) return 0;
    return tgcn::members_part_bytes(N, K, n, Fh) * static_cast<size_t>(n_members);
}

int tgcn_embed_xw_members_grad(const float *E, int64_t lde, const float *b, const float *Eh, int64_t ldeh, const float *Hd,
                               int64_t ldh, int64_t h_row0, int Fh, const float *W, int64_t ldw, const float *G, int64_t ldg,
                               float *dE, int64_t ldde, float *db, float *dEh, int64_t lddeh, float *dW, int64_t lddw,
                               int64_t N, int K, int n, int n_members, const double *p_host, const uint64_t *seeds,
                               int64_t mask_row0, void *workspace, size_t workspace_bytes, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_embed_xw_members_grad";
    const EmbedH h{Eh, ldeh, Hd, ldh, h_row0, Fh};
    MembersArgs a;
    bool drop = false;
    TGCN_CHECK(members_args(fn, E, lde, b, h, W, ldw, N, K, n, n_members, p_host, seeds, mask_row0, a, drop));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, int64_t(n_members) * n));
    if (dE) TGCN_CHECK(check_ld(fn, "ldde", ldde, N));
    if (a.h && dEh) TGCN_CHECK(check_ld(fn, "lddeh", lddeh, Fh));
    if (dW) TGCN_CHECK(check_ld(fn, "lddw", lddw, n));
    const bool db_apart = (dE == nullptr) != (db == nullptr) && N > 0;
    if (a.h && ((dE == nullptr) != (dEh == nullptr) || db_apart)) {
        set_error("%s: dE, db and dEh are computed together: pass all three or none (db and dEh are sums over dE)", fn);
        return TGCN_E_INVALID;
    }
    if (!a.h && db_apart) {
        set_error("%s: dE and db are computed together: pass both or neither (db is the row sum of dE)", fn);
        return TGCN_E_INVALID;
    }
    a.s = static_cast<hipStream_t>(stream);
    const int rows = n_members * K;
    if (N == 0) {                              // empty sums; there is no element of dE
        if (db) TGCN_HIP_CHECK(hipMemsetAsync(db, 0, sizeof(float) * rows, a.s));
        if (a.h && dEh) TGCN_HIP_CHECK(hipMemset2DAsync(dEh, sizeof(float) * lddeh, 0, sizeof(float) * Fh, rows, a.s));
        if (dW) TGCN_HIP_CHECK(hipMemset2DAsync(dW, sizeof(float) * lddw, 0, sizeof(float) * n, rows, a.s));
        return TGCN_OK;
    }
    TGCN_CHECK(members_ptrs(fn, a));
    TGCN_CHECK(check_ptr(fn, "G", G));
    if (!dE && !dW) {
        set_error("%s: dE (with %s) and dW are both NULL: nothing to compute", fn, a.h ? "db and dEh" : "db");
        return TGCN_E_INVALID;
    }
    const size_t one = members_part_bytes(N, K, n, Fh), need = one * static_cast<size_t>(n_members);
    if ((dW || (dE && a.h && h.h0 < N)) && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace of %zu bytes, %s_workspace_bytes() asks for %zu", fn, workspace_bytes, fn, need);
        return TGCN_E_WORKSPACE;
    }
    float *part = static_cast<float *>(workspace);
    const int64_t part_stride = static_cast<int64_t>(one / sizeof(float));
    if (dE) {
        TGCN_CHECK(drop ? launch_grad_e_members<true>(a, G, ldg, dE, ldde, db, dEh, lddeh, part, part_stride)
                        : launch_grad_e_members<false>(a, G, ldg, dE, ldde, db, dEh, lddeh, part, part_stride));
    }
    if (dW) {
        TGCN_CHECK(drop ? launch_grad_w_members<true>(a, G, ldg, dW, lddw, part, part_stride)
                        : launch_grad_w_members<false>(a, G, ldg, dW, lddw, part, part_stride));
    }
    return TGCN_OK;
}

}  // extern "C"
