// The middle of the reference's MLP (textgcn/lib/models.py:83-102): x = dropout(selu(Linear(x))) feeding the next Linear.
// Z [N, k] is a layer's stored pre-activation WITHOUT its bias b [k]; W [n, k] is the next nn.Linear's weight in torch's
// [out, in] layout, c [n] its bias.  Element a(i, j) = s * keep(i, j) * selu(Z[i, j] + b[j]) is formed in registers on its
// way into the matrix cores and never stored:
//     tgcn_mlp_act_linear        C[i, m]  = sum_j a(i, j) W[m, j] (+ c[m])
//     tgcn_mlp_act_linear_grad   dZ[i, j] = s keep(i, j) selu'(Z[i, j] + b[j]) sum_m G[i, m] W[m, j],   db[j] = sum_i dZ[i, j],
//                                dW[m, j] = sum_i G[i, m] a(i, j)                       (a recomputed, the same mask)
// keep(i, j) is the decision of tgcn_gemm_*_dropout (drop_hash.h) for mask row mask_row0 + i, column j.
//
// tgcn_mlp_act_linear_cls* are the same three kernels with CLS = true: the pre-activation is then
// ((Z[i, j] + T[cls[i, 0], j]) + T[cls[i, 1], j]) + b[j], a bias that depends on the row (ClassTerm, fused_act.h) -- the
// one-hot class columns that MLP_level.py appends to the TF-IDF features, as rows of the first layer's weight.  Each kernel
// adds the rows of T where it loads Z, so no N x k sum is stored; dT is a grouped column sum of the finished dZ
// (k_mlp_class_sums), computed next to db.
//
// All three products run on v_mfma_f32_32x32x2_f32 (fragment maps: fused_act.h).  Z, W and G are row-major, so every
// global load here has the lanes of a half wave on 32 consecutive floats of one row (one 128-byte run); they are plain
// dword loads, which ask nothing of the strides or the alignment.  Where the matrix cores want an operand with the ROW
// on the lane (the forward's activation and weight tiles, dZ's tile of G), the tile goes through LDS with an odd row
// stride.
#include <algorithm>

#include "fused_act.h"

namespace tgcn {
namespace {

// ---------------------------------------------------------------------------------------------
// Forward.  A workgroup owns 128 rows, a wave 32 of them and all 32 NT result columns.  Per chunk of 32 reduction
// indices the workgroup stages its 128 x 32 tile of Z and the NT 32 x 32 tiles of W in LDS, both as [row][33]: the
// staging writes (lanes along a row) and the operand reads (lanes down a column, 33 floats apart) are conflict-free.
// Per MFMA step a lane forms ONE element a(i, j) -- its row i is fixed, so the row key of the hash is paid once per
// lane -- and spends it on NT tiles.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP, bool CLS>
__global__ __launch_bounds__(256, 2) void k_mlp_fwd(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                    const float *__restrict__ W, int64_t ldw, const float *__restrict__ cb,
                                                    float *__restrict__ C, int64_t ldc, int64_t N, int K, int n,
                                                    const RowDrop d, const ClassTerm ct) {
    constexpr int KC = 32, NP = 32 * NT, LD = KC + 1;
    __shared__ float Ws[NP * LD];
    __shared__ float Zs[128 * LD];
    __shared__ float bs[KC];
    __shared__ int32_t cs[CLS ? 2 * 128 : 2];              // the ids of the workgroup's rows (-1: nothing selected)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t blk0 = int64_t(blockIdx.x) * 128;
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
// dZ, in Z's layout: T[i, j] = sum_m G[i, m] W[m, j].  A wave keeps its 32 rows of G in registers (the A operand, the row
// on the lane: read once with the lanes along a row, turned through the wave's own [32][33] tile in LDS, then reused over
// all K / 32 tiles of j); the workgroup shares the NT x 32 rows of W for the tile in LDS as they lie in
// memory (the B operand has the lanes along a row: no transpose, no conflict).  A lane's 16 results are 16 rows of one
// column, so it pays 16 row keys, once, before the loop over the tiles.  `accum`: the reduction over m is longer than one
// launch covers (n > 128: more rows of G than a lane has registers for beside the keys) and this is not its first piece:
// the masked, scaled partial sum is added to what dZ holds.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP, bool CLS>
__global__ __launch_bounds__(256, 2) void k_mlp_grad_z(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                       const float *__restrict__ W, int64_t ldw,
                                                       const float *__restrict__ G, int64_t ldg, float *__restrict__ dZ,
                                                       int64_t lddz, int64_t N, int K, int n, int accum, const RowDrop d,
                                                       const ClassTerm ct) {
    constexpr int NP = 32 * NT;
    __shared__ float Ws[NP * 32];
    __shared__ float Gs[4 * 32 * 33];
    __shared__ float bs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = (int64_t(blockIdx.x) * 4 + wave) * 32;
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
// dW[m, j] = sum_i G[i, m] a(i, j), in W's layout: the reduction runs over the rows, and both operands have the lanes
// along a row as they lie in memory.  blockIdx.x is a tile of 32 columns j, blockIdx.y a slice of the rows.  The workgroup
// reads 128 rows x 32 columns of Z, forms a(i, j) ONCE per element and leaves it in LDS (the row keys of the tile are
// computed once, by 128 threads, and shared through LDS); the 4 waves split the rows m of dW (TW tiles of 32 each) and
// read their slab of G straight from memory, 128 bytes per half wave.  The slices' partial sums go to the workspace and
// are added in a fixed order by k_reduce_slices.
// ---------------------------------------------------------------------------------------------
template <int TW, bool DROP, bool CLS>
__global__ __launch_bounds__(256, 2) void k_mlp_grad_w(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                       const float *__restrict__ G, int64_t ldg, float *__restrict__ part,
                                                       int64_t N, int K, int n, int64_t chunks_per_slice, const RowDrop d,
                                                       const ClassTerm ct) {
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

// ---------------------------------------------------------------------------------------------
// dT[f, j] = the sum of dZ[i, j] over the rows i and slots s with cls[i, s] == f: a grouped column sum of the finished dZ.
// A workgroup is ONE wave: blockIdx.x is a tile of 64 columns, blockIdx.y a slice of the rows.  It keeps a table
// [Fh][64] of sums in LDS (dynamic: Fh x 256 bytes, at most 32 KB), lane c owning column c of it, and walks the rows of
// its slice in order: the row's ids are the same for the whole wave, the 64 lanes load 256 consecutive bytes of dZ and
// each adds its element to its column of the id's row.  A lane touches no other lane's sums, so there is no barrier and
// the order of the additions is the row order; the cost does not grow with Fh (hier.hip's k_hier_class_sums, which has a
// lane per (class, column), walks the ids once per 8 classes).  k_reduce_slices adds the slices in order.  A row of T
// that no id selects gets exact zeros; a row whose two slots name the same id counts twice, as the sum says.
// ---------------------------------------------------------------------------------------------
constexpr int kSumCols = 64;

__global__ __launch_bounds__(64) void k_mlp_class_sums(const float *__restrict__ dZ, int64_t lddz, const ClassTerm ct,
                                                       int64_t N, int K, int64_t rows_per_slice, float *__restrict__ part,
                                                       int kpad) {
    extern __shared__ float tab[];                         // [Fh][kSumCols]
    const int c = threadIdx.x, j = blockIdx.x * kSumCols + c;
    const bool in = j < K;
    for (int f = 0; f < ct.Fh; ++f) tab[f * kSumCols + c] = 0.f;
    const int64_t i0 = int64_t(blockIdx.y) * rows_per_slice;
    const int64_t i1 = i0 + rows_per_slice < N ? i0 + rows_per_slice : N;
    for (int64_t i = i0; i < i1; i += 4) {
        int32_t id0[4], id1[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            class_ids<true>(ct, i + u, i + u < i1, id0[u], id1[u]);
            id0[u] = __builtin_amdgcn_readfirstlane(id0[u]);   // (the same in every lane)
            id1[u] = __builtin_amdgcn_readfirstlane(id1[u]);
            v[u] = (in && (id0[u] >= 0 || id1[u] >= 0)) ? dZ[(i + u) * lddz + j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (id0[u] >= 0) tab[id0[u] * kSumCols + c] += v[u];
            if (id1[u] >= 0) tab[id1[u] * kSumCols + c] += v[u];
        }
    }
    if (in)
        for (int f = 0; f < ct.Fh; ++f) part[(int64_t(blockIdx.y) * ct.Fh + f) * kpad + j] = tab[f * kSumCols + c];
}

// How the rows are cut for dT: slices of at least 64 rows, at most 1024 of them and at most 4 M floats of partial sums
// (hier.hip's class_sum_split).
void class_sum_split(int64_t N, int K, int Fh, int64_t &slices, int64_t &rows_per_slice) {
    const int64_t per_slice = int64_t(Fh) * ((int64_t(K) + 31) / 32 * 32);
    const int64_t most = std::min<int64_t>(1024, std::max<int64_t>(16, (int64_t(1) << 22) / per_slice));
    rows_per_slice = std::max<int64_t>(64, (N + most - 1) / most);
    slices = (N + rows_per_slice - 1) / rows_per_slice;
}

// the workspace: the column-sum partials of db first, the slices' partial sums of dW after them, those of dT last
size_t db_floats(int64_t N, int K) { return static_cast<size_t>(colsum_blocks(N)) * static_cast<size_t>(K); }

size_t dt_floats(int64_t N, int K, int Fh) {
    if (N <= 0) return 0;
    int64_t slices, rps;
    class_sum_split(N, K, Fh, slices, rps);
    return static_cast<size_t>(slices * Fh * ((int64_t(K) + 31) / 32 * 32));
}

size_t dw_floats(int64_t N, int K, int n) {
    int64_t slices, cps;
    grad_w_split(N, K, kWTarget, slices, cps);
    const int64_t kpad = (int64_t(K) + 31) / 32 * 32;
    const int64_t np = std::min(n, kWGroup) > 128 ? 256 : 128;
    return static_cast<size_t>(slices * np * kpad);
}

template <bool DROP, bool CLS>
int launch_fwd(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *cb, float *C,
               int64_t ldc, int64_t N, int K, int n, const RowDrop &d, const ClassTerm &ct, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kFwdGroup) {
        const int ng = std::min(n - col0, kFwdGroup), nt = (ng + 31) / 32;
        const float *cg = cb ? cb + col0 : nullptr;
        with_tiles<1, 2, 4, 8>(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_mlp_fwd<decltype(NT)::value, DROP, CLS>), dim3(grid), dim3(256), 0, s, Z, ldz, b,
                               W + int64_t(col0) * ldw, ldw, cg, C + col0, ldc, N, K, ng, d, ct);
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP, bool CLS>
int launch_grad_z(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *G, int64_t ldg,
                  float *dZ, int64_t lddz, float *db, int64_t N, int K, int n, const RowDrop &d, const ClassTerm &ct,
                  float *part, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((N + 127) / 128);
    for (int col0 = 0; col0 < n; col0 += kGzGroup) {
        const int ng = std::min(n - col0, kGzGroup), nt = (ng + 31) / 32, accum = col0 > 0;
        with_tiles<1, 2, 4>(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_mlp_grad_z<decltype(NT)::value, DROP, CLS>), dim3(grid), dim3(256), 0, s, Z, ldz, b,
                               W + int64_t(col0) * ldw, ldw, G + col0, ldg, dZ, lddz, N, K, ng, accum, d, ct);
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    // db[j] = sum_i dZ[i, j]: tgcn_colsum's two passes (colsum.hip), a fixed summation order
    return launch_colsum(dZ, lddz, N, K, db, part, colsum_blocks(N), s);
}

// dT from the finished dZ: the slices' grouped column sums, then their sum in slice order
int launch_grad_t(const float *dZ, int64_t lddz, const ClassTerm &ct, float *dT, int64_t lddt, int64_t N, int K, float *part,
                  hipStream_t s) {
    int64_t slices, rps;
    class_sum_split(N, K, ct.Fh, slices, rps);
    const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
    const dim3 grid((K + kSumCols - 1) / kSumCols, static_cast<unsigned>(slices));
    hipLaunchKernelGGL(k_mlp_class_sums, grid, dim3(kSumCols), sizeof(float) * ct.Fh * kSumCols, s, dZ, lddz, ct, N, K, rps,
                       part, kpad);
    launch_reduce_slices(part, slices, int64_t(ct.Fh) * kpad, kpad, ct.Fh, K, dT, lddt, s);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP, bool CLS>
int launch_grad_w(const float *Z, int64_t ldz, const float *b, const float *G, int64_t ldg, float *dW, int64_t lddw,
                  int64_t N, int K, int n, const RowDrop &d, const ClassTerm &ct, float *part, hipStream_t s) {
    int64_t slices, cps;
    grad_w_split(N, K, kWTarget, slices, cps);
    const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
    for (int m0 = 0; m0 < n; m0 += kWGroup) {
        const int ng = std::min(n - m0, kWGroup);
        const dim3 grid(ktiles, static_cast<unsigned>(slices));
        if (ng > 128)
            hipLaunchKernelGGL((k_mlp_grad_w<2, DROP, CLS>), grid, dim3(256), 0, s, Z, ldz, b, G + m0, ldg, part, N, K, ng, cps,
                               d, ct);
        else
            hipLaunchKernelGGL((k_mlp_grad_w<1, DROP, CLS>), grid, dim3(256), 0, s, Z, ldz, b, G + m0, ldg, part, N, K, ng, cps,
                               d, ct);
        const int np = ng > 128 ? 256 : 128;
        launch_reduce_slices(part, slices, int64_t(np) * kpad, kpad, ng, K, dW + int64_t(m0) * lddw, lddw, s);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// f(DROP, CLS) with the two switches as integral constants
template <class F>
int with_variant(bool drop, bool cls, F &&f) {
    using Y = std::true_type;
    using No = std::false_type;
    return drop ? (cls ? f(Y{}, Y{}) : f(Y{}, No{})) : (cls ? f(No{}, Y{}) : f(No{}, No{}));
}

// the checks of the class term; `dT` / `lddt`: the backward's (nullptr in the forward)
int check_class_term(const char *fn, const ClassTerm &ct, int64_t N, int k, const float *dT, int64_t lddt) {
    if (ct.S != 1 && ct.S != 2) {
        set_error("%s: S must be 1 or 2 (S=%d)", fn, ct.S);
        return TGCN_E_INVALID;
    }
    if (ct.Fh < 1 || ct.Fh > kClassRowsMax) {
        set_error("%s: Fh must be in [1, %d] (tgcn_hier_max_features) (Fh=%d)", fn, kClassRowsMax, ct.Fh);
        return TGCN_E_INVALID;
    }
    TGCN_CHECK(check_ld(fn, "ldcls", ct.ldcls, ct.S));
    TGCN_CHECK(check_ld(fn, "ldt", ct.ldt, k));
    if (dT) TGCN_CHECK(check_ld(fn, "lddt", lddt, k));
    if (N > 0) {
        TGCN_CHECK(check_ptr(fn, "cls", ct.cls));
        TGCN_CHECK(check_ptr(fn, "T", ct.T));
    }
    return TGCN_OK;
}

// the two entry points with and without the class term (`term` NULL: without)
int act_linear(const char *fn, const float *Z, int64_t ldz, const ClassTerm *term, const float *b, const float *W,
               int64_t ldw, const float *c, float *C, int64_t ldc, int64_t N, int k, int n, double p, const uint64_t *seed,
               int64_t mask_row0, tgcn_stream stream) {
    TGCN_CHECK(check_sizes(fn, "k", N, k, n));
    RowDrop d{};
    bool drop = false;
    TGCN_CHECK(make_row_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_CHECK(check_ld(fn, "ldz", ldz, k));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, k));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, n));
    if (term) TGCN_CHECK(check_class_term(fn, *term, N, k, nullptr, 0));
    if (N == 0) return TGCN_OK;                // (an empty tensor's pointer may be NULL)
    TGCN_CHECK(check_ptr(fn, "Z", Z));
    TGCN_CHECK(check_ptr(fn, "b", b));
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "C", C));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ClassTerm ct = term ? *term : ClassTerm{};
    return with_variant(drop, term != nullptr, [&](auto DROP, auto CLS) {
        return launch_fwd<decltype(DROP)::value, decltype(CLS)::value>(Z, ldz, b, W, ldw, c, C, ldc, N, k, n, d, ct, s);
    });
}

size_t grad_workspace_floats(int64_t N, int k, int n, int Fh) {
    return db_floats(N, k) + dw_floats(N, k, n) + (Fh > 0 ? dt_floats(N, k, Fh) : 0);
}

int act_linear_grad(const char *fn, const float *Z, int64_t ldz, const ClassTerm *term, const float *b, const float *W,
                    int64_t ldw, const float *G, int64_t ldg, float *dZ, int64_t lddz, float *db, float *dT, int64_t lddt,
                    float *dW, int64_t lddw, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                    void *workspace, size_t workspace_bytes, tgcn_stream stream) {
    TGCN_CHECK(check_sizes(fn, "k", N, k, n));
    RowDrop d{};
    bool drop = false;
    TGCN_CHECK(make_row_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_CHECK(check_ld(fn, "ldz", ldz, k));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, k));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, n));
    if (dZ) TGCN_CHECK(check_ld(fn, "lddz", lddz, k));
    if (dW) TGCN_CHECK(check_ld(fn, "lddw", lddw, k));
    if (term) TGCN_CHECK(check_class_term(fn, *term, N, k, dT, lddt));
    if ((dZ == nullptr) != (db == nullptr) && N > 0) {     // (N == 0: dZ has no element and its pointer may be NULL)
        set_error("%s: dZ and db are computed together: pass both or neither (db is the column sum of dZ)", fn);
        return TGCN_E_INVALID;
    }
    if (dT && !dZ && N > 0) {
        set_error("%s: dT is requested without dZ (dT is a grouped column sum of dZ)", fn);
        return TGCN_E_INVALID;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (N == 0) {                              // empty sums; there is no element of dZ
        if (db) TGCN_HIP_CHECK(hipMemsetAsync(db, 0, sizeof(float) * k, s));
        if (dW) TGCN_HIP_CHECK(hipMemset2DAsync(dW, sizeof(float) * lddw, 0, sizeof(float) * k, n, s));
        if (dT) TGCN_HIP_CHECK(hipMemset2DAsync(dT, sizeof(float) * lddt, 0, sizeof(float) * k, term->Fh, s));
        return TGCN_OK;
    }
    TGCN_CHECK(check_ptr(fn, "Z", Z));
    TGCN_CHECK(check_ptr(fn, "b", b));
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "G", G));
    if (!dZ && !dW) {
        set_error("%s: dZ (with db) and dW are both NULL: nothing to compute", fn);
        return TGCN_E_INVALID;
    }
    const size_t need = grad_workspace_floats(N, k, n, term ? term->Fh : 0) * sizeof(float);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %s_workspace_bytes() asks for %zu", fn, workspace ? workspace_bytes : size_t(0),
                  fn, need);
        return TGCN_E_INVALID;
    }
    float *part_b = static_cast<float *>(workspace);
    float *part_w = part_b + db_floats(N, k);
    float *part_t = part_w + dw_floats(N, k, n);
    const ClassTerm ct = term ? *term : ClassTerm{};
    return with_variant(drop, term != nullptr, [&](auto DROP, auto CLS) {
        constexpr bool kDrop = decltype(DROP)::value, kCls = decltype(CLS)::value;
        if (dZ) {
            TGCN_CHECK((launch_grad_z<kDrop, kCls>(Z, ldz, b, W, ldw, G, ldg, dZ, lddz, db, N, k, n, d, ct, part_b, s)));
            if (dT) TGCN_CHECK(launch_grad_t(dZ, lddz, ct, dT, lddt, N, k, part_t, s));
        }
        if (dW) TGCN_CHECK((launch_grad_w<kDrop, kCls>(Z, ldz, b, G, ldg, dW, lddw, N, k, n, d, ct, part_w, s)));
        return int(TGCN_OK);
    });
}

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_mlp_act_linear(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *c, float *C,
                        int64_t ldc, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                        tgcn_stream stream) {
    return tgcn::act_linear("tgcn_mlp_act_linear", Z, ldz, nullptr, b, W, ldw, c, C, ldc, N, k, n, p, seed, mask_row0, stream);
}

size_t tgcn_mlp_act_linear_grad_workspace_bytes(int64_t N, int k, int n) {
    if (N < 0 || k <= 0 || n <= 0) return 0;
    return tgcn::grad_workspace_floats(N, k, n, 0) * sizeof(float);
}

int tgcn_mlp_act_linear_grad(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *G,
                             int64_t ldg, float *dZ, int64_t lddz, float *db, float *dW, int64_t lddw, int64_t N, int k,
                             int n, double p, const uint64_t *seed, int64_t mask_row0, void *workspace,
                             size_t workspace_bytes, tgcn_stream stream) {
    return tgcn::act_linear_grad("tgcn_mlp_act_linear_grad", Z, ldz, nullptr, b, W, ldw, G, ldg, dZ, lddz, db, nullptr, 0, dW,
                                 lddw, N, k, n, p, seed, mask_row0, workspace, workspace_bytes, stream);
}

int tgcn_mlp_act_linear_cls(const float *Z, int64_t ldz, const int32_t *cls, int64_t ldcls, int S, const float *T,
                            int64_t ldt, int Fh, const float *b, const float *W, int64_t ldw, const float *c, float *C,
                            int64_t ldc, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                            tgcn_stream stream) {
    const tgcn::ClassTerm ct{cls, ldcls, T, ldt, S, Fh};
    return tgcn::act_linear("tgcn_mlp_act_linear_cls", Z, ldz, &ct, b, W, ldw, c, C, ldc, N, k, n, p, seed, mask_row0, stream);
}

size_t tgcn_mlp_act_linear_cls_grad_workspace_bytes(int64_t N, int k, int n, int Fh) {
    if (N < 0 || k <= 0 || n <= 0 || Fh < 1 || Fh > tgcn::kClassRowsMax) return 0;
    return tgcn::grad_workspace_floats(N, k, n, Fh) * sizeof(float);
}

int tgcn_mlp_act_linear_cls_grad(const float *Z, int64_t ldz, const int32_t *cls, int64_t ldcls, int S, const float *T,
                                 int64_t ldt, int Fh, const float *b, const float *W, int64_t ldw, const float *G,
                                 int64_t ldg, float *dZ, int64_t lddz, float *db, float *dT, int64_t lddt, float *dW,
                                 int64_t lddw, int64_t N, int k, int n, double p, const uint64_t *seed, int64_t mask_row0,
                                 void *workspace, size_t workspace_bytes, tgcn_stream stream) {
    const tgcn::ClassTerm ct{cls, ldcls, T, ldt, S, Fh};
    return tgcn::act_linear_grad("tgcn_mlp_act_linear_cls_grad", Z, ldz, &ct, b, W, ldw, G, ldg, dZ, lddz, db, dT, lddt, dW,
                                 lddw, N, k, n, p, seed, mask_row0, workspace, workspace_bytes, stream);
}

}  // extern "C"

