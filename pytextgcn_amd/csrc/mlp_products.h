// The three fused SELU + dropout products of the MLP, ONCE: the bodies of k_mlp_fwd / k_mlp_grad_z / k_mlp_grad_w (mlp.hip)
// and of k_gmlp_fwd / k_gmlp_grad_z / k_gmlp_grad_w (mlp_grouped.hip).  A kernel only says where its rows are -- rows
// 128 blockIdx.x ... of the whole operand, or one tile / slice of the grouped layout table -- and hands in the operand
// pointers already moved to its group's W, b, G, C and c; the arithmetic, its summation order and every MFMA of these
// products stand here, so a group's slice of the grouped results has the bits of the flat kernels by construction
// (embed.hip's idiom: __shared__ arrays inside the body, an unnamed namespace, one copy per translation unit).
//
// Z [N, K] is a layer's stored pre-activation WITHOUT its bias b [K], W [n, K] the next nn.Linear's weight in torch's
// [out, in] layout.  Element a(i, j) = s * keep(i, j) * selu(Z[i, j] + b[j]) is formed in registers on its way into the
// matrix cores and never stored; CLS adds the rows of T that the row's ids select to the pre-activation where Z is loaded
// (ClassTerm, fused_act.h; only the flat kernels have it, and for dW it is in k_mlp_grad_w at the end of this file).  All three run on v_mfma_f32_32x32x2_f32 (fragment maps: fused_act.h).  Z, W and G are
// row-major, so every global load here has the lanes of a half wave on 32 consecutive floats of one row (one 128-byte
// run); they are plain dword loads, which ask nothing of the strides or the alignment.  Where the matrix cores want an
// operand with the ROW on the lane (the forward's activation and weight tiles, dZ's tile of G), the tile goes through LDS
// with an odd row stride.
#pragma once

#include "fused_act.h"

namespace tgcn {
namespace {

// ---------------------------------------------------------------------------------------------
// Forward: C[i, m] = sum_j a(i, j) W[m, j] (+ cb[m]) for the rows [blk0, min(blk0 + 128, N)).  A workgroup owns 128 rows,
// a wave 32 of them and all 32 NT result columns.  Per chunk of 32 reduction indices the workgroup stages its 128 x 32
// tile of Z and the NT 32 x 32 tiles of W in LDS, both as [row][33]: the staging writes (lanes along a row) and the
// operand reads (lanes down a column, 33 floats apart) are conflict-free.  Per MFMA step a lane forms ONE element
// a(i, j) -- its row i is fixed, so the row key of the hash is paid once per lane -- and spends it on NT tiles.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP, bool CLS>
__device__ __forceinline__ void mlp_fwd(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                        const float *__restrict__ W, int64_t ldw, const float *__restrict__ cb,
                                        float *__restrict__ C, int64_t ldc, int64_t blk0, int64_t N, int K, int n,
                                        const RowDrop &d, const ClassTerm &ct) {
    constexpr int KC = 32, NP = 32 * NT, LD = KC + 1;
    __shared__ float Ws[NP * LD];
    __shared__ float Zs[128 * LD];
    __shared__ float bs[KC];
    __shared__ int32_t cs[CLS ? 2 * 128 : 2];              // the ids of the workgroup's rows (-1: nothing selected)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = blk0 + wave * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const uint32_t key = row_key<DROP>(d, i);
    const int skk = tid & 31, sr = tid >> 5;               // staging: this thread's column of the chunk and its first row
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    if constexpr (CLS) {
        if (tid < 128) class_ids<CLS>(ct, blk0 + tid, blk0 + tid < N, cs[2 * tid], cs[2 * tid + 1]);
    }

    for (int k0 = 0; k0 < K; k0 += KC) {
        const bool kin = k0 + skk < K;
        __syncthreads();                                   // the previous chunk has been read (and the ids are written)
#pragma unroll 4
        for (int u = 0; u < 4 * NT; ++u) {
            const int m = sr + 8 * u;
            Ws[m * LD + skk] = (kin && m < n) ? W[int64_t(m) * ldw + k0 + skk] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = sr + 8 * u;
            float z = (kin && blk0 + r < N) ? Z[(blk0 + r) * ldz + k0 + skk] : 0.f;
            if constexpr (CLS) {
                if (kin) z = plus_class_rows<CLS>(z, ct, cs[2 * r], cs[2 * r + 1], k0 + skk);
            }
            Zs[r * LD + skk] = z;
        }
        if (tid < KC) bs[tid] = kin ? b[k0 + tid] : 0.f;
        __syncthreads();
        const float *zr = Zs + (wave * 32 + c) * LD;
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int kk = 2 * s + half, k = k0 + kk;
            const float a = (live && k < K) ? act<DROP>(zr[kk] + bs[kk], key, drop_col_term(k), d) : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Ws[(32 * t + c) * LD + kk], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = 32 * t + c;
        const float bias = (cb != nullptr && col < n) ? cb[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, half);
            if (row < N && col < n) C[row * ldc + col] = acc[t][r] + bias;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dZ, in Z's layout, for the rows [blk0, min(blk0 + 128, N)): dZ[i, j] = s keep(i, j) selu'(.) sum_m G[i, m] W[m, j].  A
// wave (rows blk0 + 32 wave ...) keeps its 32 rows of G in registers (the A operand, the row on the lane: read once with
// the lanes along a row, turned through the wave's own [32][33] tile in LDS, then reused over all K / 32 tiles of j); the
// workgroup shares the NT x 32 rows of W for the tile in LDS as they lie in memory (the B operand has the lanes along a
// row: no transpose, no conflict).  A lane's 16 results are 16 rows of one column, so it pays 16 row keys, once, before
// the loop over the tiles.  `accum`: the reduction over m is longer than one launch covers (n > 128: more rows of G than
// a lane has registers for beside the keys) and this is not its first piece: the masked, scaled partial sum is added to
// what dZ holds.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP, bool CLS>
__device__ __forceinline__ void mlp_grad_z(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                           const float *__restrict__ W, int64_t ldw, const float *__restrict__ G,
                                           int64_t ldg, float *__restrict__ dZ, int64_t lddz, int64_t blk0, int64_t N, int K,
                                           int n, int accum, const RowDrop &d, const ClassTerm &ct) {
    constexpr int NP = 32 * NT;
    __shared__ float Ws[NP * 32];
    __shared__ float Gs[4 * 32 * 33];
    __shared__ float bs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = blk0 + wave * 32;
    const int sj = tid & 31, sr = tid >> 5;
    float *gw = Gs + wave * (32 * 33);                     // this wave's 32 x 32 tile of G, [row][33]
    float g[16 * NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int m = 32 * t + c;
#pragma unroll
        for (int u = 0; u < 16; ++u) {                     // lanes along a row of G: 128 bytes per half wave
            const int r = 2 * u + half;
            gw[r * 33 + c] = (row0 + r < N && m < n) ? G[(row0 + r) * ldg + m] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) g[16 * t + s] = gw[c * 33 + 2 * s + half];   // lane c takes row c, column 2 s + half
        __syncthreads();
    }
    uint32_t keys[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) keys[r] = row_key<DROP>(d, row0 + acc_row(r, half));
    // The ids of the workgroup's 128 rows (pack_ids), in LDS and read again for every tile: held in registers, the
    // compiler keeps 32 row addresses of T per lane alive across the loop and the widest instantiation spills.
    __shared__ uint32_t cs[CLS ? 128 : 1];
    if constexpr (CLS) {
        if (lane < 32) {
            int32_t id0, id1;
            class_ids<CLS>(ct, row0 + lane, row0 + lane < N, id0, id1);
            cs[wave * 32 + lane] = pack_ids(id0, id1);
        }
    }

    for (int j0 = 0; j0 < K; j0 += 32) {
        __syncthreads();                                   // the previous tile has been read
#pragma unroll 4
        for (int u = 0; u < 4 * NT; ++u) {
            const int m = sr + 8 * u;
            Ws[m * 32 + sj] = (j0 + sj < K && m < n) ? W[int64_t(m) * ldw + j0 + sj] : 0.f;
        }
        if (tid < 32) bs[tid] = j0 + tid < K ? b[j0 + tid] : 0.f;
        const int j = j0 + c;
        float z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, half);
            z[r] = (row < N && j < K) ? Z[row * ldz + j] : 0.f;
            if constexpr (CLS) {
                const uint32_t ids = cs[wave * 32 + acc_row(r, half)];
                if (j < K) z[r] = plus_class_rows<CLS>(z[r], ct, packed_id(ids, 0), packed_id(ids, 1), j);
            }
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16 * NT; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g[s], Ws[(2 * s + half) * 32 + c], acc, 0, 0, 0);
        const float bj = bs[c];
        const uint32_t col_term = drop_col_term(j);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, half);
            if (row < N && j < K) {
                float v = acc[r] * selu_grad_f(z[r] + bj);
                if constexpr (DROP) v = drop_hash_keep(keys[r], col_term, d.thresh) ? v * d.scale : 0.f;
                float *out = dZ + row * lddz + j;
                *out = accum ? *out + v : v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dW[m, j] = sum_i G[i, m] a(i, j), in W's layout, over the rows [i_begin, i_end) of one slice: the reduction runs over
// the rows, and both operands have the lanes along a row as they lie in memory.  blockIdx.x is a tile of 32 columns j,
// blockIdx.y the slice (where its partial sums go in `part`).  The workgroup reads 128 rows x 32 columns of Z, forms
// a(i, j) ONCE per element and leaves it in LDS (the row keys of the tile are computed once, by 128 threads, and shared
// through LDS); the 4 waves split the rows m of dW (TW tiles of 32 each) and read their slab of G straight from memory,
// 128 bytes per half wave.  The slices' partial sums go to the workspace and are added in a fixed order by
// reduce_slices (fused_act.h).
// ---------------------------------------------------------------------------------------------
template <int TW, bool DROP>
__device__ __forceinline__ void mlp_grad_w(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                           const float *__restrict__ G, int64_t ldg, float *__restrict__ part,
                                           int64_t i_begin, int64_t i_end, int K, int n, const RowDrop &d) {
    constexpr int NP = 128 * TW;
    __shared__ float As[kWChunk * 32];
    __shared__ uint32_t ks[kWChunk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int j0 = blockIdx.x * 32;
    const int kpad = gridDim.x * 32;
    const bool computes = wave * TW * 32 < n;             // a wave whose rows of dW are all padding only helps staging
    const int sj = tid & 31, sr = tid >> 5;                // staging: this thread's column of the tile and its first row
    const int j = j0 + sj;
    const float bj = j < K ? b[j] : 0.f;
    const uint32_t col_term = drop_col_term(j);
    f32x16 acc[TW];
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int64_t i0 = i_begin; i0 < i_end; i0 += kWChunk) {
        float z[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int64_t i = i0 + sr + 8 * u;
            z[u] = (i < i_end && j < K) ? Z[i * ldz + j] : 0.f;
        }
        __syncthreads();                                   // the previous tile has been read
        if constexpr (DROP) {
            if (tid < kWChunk) ks[tid] = row_key<DROP>(d, i0 + tid);
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = sr + 8 * u;
            const int64_t i = i0 + r;
            const uint32_t key = DROP ? ks[r] : 0u;
            As[r * 32 + sj] = (i < i_end && j < K) ? act<DROP>(z[u] + bj, key, col_term, d) : 0.f;
        }
        __syncthreads();
        if (computes) {
#pragma unroll 8
            for (int s = 0; s < kWChunk / 2; ++s) {
                const int ii = 2 * s + half;
                const int64_t i = i0 + ii;
                const float a = As[ii * 32 + c];
#pragma unroll
                for (int t = 0; t < TW; ++t) {
                    const int m = (wave * TW + t) * 32 + c;
                    const float gv = (i < i_end && m < n) ? G[i * ldg + m] : 0.f;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, a, acc[t], 0, 0, 0);
                }
            }
        }
    }
    float *out = part + int64_t(blockIdx.y) * NP * kpad + j0 + c;
#pragma unroll
    for (int t = 0; t < TW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[int64_t((wave * TW + t) * 32 + acc_row(r, half)) * kpad] = acc[t][r];
}

// ---------------------------------------------------------------------------------------------
// The flat dW kernel of mlp.hip (blockIdx.y: a slice of `chunks_per_slice` chunks of kWChunk rows of the whole operand).
// Without the class term it calls mlp_grad_w, as k_gmlp_grad_w (mlp_grouped.hip) does.  WITH the class term, which only
// this kernel has and no other kernel must agree with, the row loop stands in the kernel: inlined from a body, the
// compiler places the first use of the tile's loads of Z and T inside the 16 guarded blocks that stage a(i, j) and waits
// in each of them (16 s_waitcnt per 128-row chunk, +0.3 % on the call; profiles/r21_shared_bodies_isa.md).  The loop is
// mlp_grad_w's with `(z + T[id0, j]) + T[id1, j]` where Z is loaded; it is here, not in mlp.hip, so that every MFMA of
// these products is in this file.
// ---------------------------------------------------------------------------------------------
template <int TW, bool DROP, bool CLS>
__global__ __launch_bounds__(256, 2) void k_mlp_grad_w(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                       const float *__restrict__ G, int64_t ldg, float *__restrict__ part,
                                                       int64_t N, int K, int n, int64_t chunks_per_slice, const RowDrop d,
                                                       const ClassTerm ct) {
    if constexpr (!CLS) {
        const int64_t i_begin = int64_t(blockIdx.y) * chunks_per_slice * kWChunk;
        const int64_t i_stop = i_begin + chunks_per_slice * kWChunk;
        mlp_grad_w<TW, DROP>(Z, ldz, b, G, ldg, part, i_begin, i_stop < N ? i_stop : N, K, n, d);
    } else {
        constexpr int NP = 128 * TW;
        __shared__ float As[kWChunk * 32];
        __shared__ uint32_t ks[kWChunk];
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
        const int j0 = blockIdx.x * 32;
        const int kpad = gridDim.x * 32;
        const int64_t i_begin = int64_t(blockIdx.y) * chunks_per_slice * kWChunk;
        const int64_t i_stop = i_begin + chunks_per_slice * kWChunk;
        const int64_t i_end = i_stop < N ? i_stop : N;
        const bool computes = wave * TW * 32 < n;             // a wave whose rows of dW are all padding only helps staging
        const int sj = tid & 31, sr = tid >> 5;                // staging: this thread's column of the tile and its first row
        const int j = j0 + sj;
        const float bj = j < K ? b[j] : 0.f;
        const uint32_t col_term = drop_col_term(j);
        f32x16 acc[TW];
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

        for (int64_t i0 = i_begin; i0 < i_end; i0 += kWChunk) {
            float z[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int64_t i = i0 + sr + 8 * u;
                z[u] = (i < i_end && j < K) ? Z[i * ldz + j] : 0.f;
                if constexpr (CLS) {
                    int32_t id0, id1;
                    class_ids<CLS>(ct, i, i < i_end && j < K, id0, id1);
                    if (j < K) z[u] = plus_class_rows<CLS>(z[u], ct, id0, id1, j);
                }
            }
            __syncthreads();                                   // the previous tile has been read
            if constexpr (DROP) {
                if (tid < kWChunk) ks[tid] = row_key<DROP>(d, i0 + tid);
                __syncthreads();
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int r = sr + 8 * u;
                const int64_t i = i0 + r;
                const uint32_t key = DROP ? ks[r] : 0u;
                As[r * 32 + sj] = (i < i_end && j < K) ? act<DROP>(z[u] + bj, key, col_term, d) : 0.f;
            }
            __syncthreads();
            if (computes) {
#pragma unroll 8
                for (int s = 0; s < kWChunk / 2; ++s) {
                    const int ii = 2 * s + half;
                    const int64_t i = i0 + ii;
                    const float a = As[ii * 32 + c];
#pragma unroll
                    for (int t = 0; t < TW; ++t) {
                        const int m = (wave * TW + t) * 32 + c;
                        const float gv = (i < i_end && m < n) ? G[i * ldg + m] : 0.f;
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(gv, a, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        float *out = part + int64_t(blockIdx.y) * NP * kpad + j0 + c;
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[int64_t((wave * TW + t) * 32 + acc_row(r, half)) * kpad] = acc[t][r];
    }
}

}  // namespace
}  // namespace tgcn
