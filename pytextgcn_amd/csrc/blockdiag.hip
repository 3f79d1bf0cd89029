// The layer-2 products of the grouped GCNs (PerLabelGCN, CrossValGCN) for ALL K members in one launch each, with a dropout
// rate and a seed per member.  X [N, K h] is the concatenated hidden activation (member k: columns [k h, (k + 1) h)), W
// [h, n_cols] holds W_k in the column segment [col0_k, col0_k + n_k); with a(i, j) = s_k keep_k(i, j) X[i, k h + j]:
//     tgcn_blockdiag_xw        C[i, col0_k + m]  = sum_j a(i, j) W[j, col0_k + m]                 (pad columns: 0)
//     tgcn_blockdiag_xw_grad   dX[i, k h + j]    = s_k keep_k(i, j) sum_m G[i, col0_k + m] W[j, col0_k + m]
//                              colsum[k h + j]   = sum_i dX[i, k h + j]
//                              dW[j, col0_k + m] = sum_i a(i, j) G[i, col0_k + m]                 (pad columns: 0)
// keep_k(i, j) is the decision of drop_hash.h for seeds[k], mask row mask_row0 + i and column j INSIDE the member's block,
// at the threshold of p_k: what tgcn_gemm_*_dropout decides on the member's slice.  The mask is regenerated from the seed
// in all three products; nothing is recorded.
//
// The kernels are those of mlp_grouped.hip turned to this layout (W is [h, n], not [n, h]) with blockIdx.y = the member:
// a workgroup of the forward and of dX owns 128 rows of ONE member (4 waves x 32 rows, v_mfma_f32_32x32x2_f32), so X and
// G are read once per launch; dW gives a workgroup one slice of rows of one member and ALL h rows of that member's dW
// (which is where the cap on h comes from: 2 x 4 j-tiles per workgroup), so X and G are again read once.  The member table
// (col0, n, threshold, scale, the columns it zero-fills) is a blob built on the host (tgcn_blockdiag_layout), as in
// mlp_grouped.hip.  Partial sums (dW per slice, the column sums per row tile) go to the workspace and are added in a fixed
// order: no atomics.  The launch count depends on max n_k only (column groups of kFwdGroup, kGzGroup and kBdWGroup).
#include <algorithm>
#include <climits>
#include <cstring>

#include "fused_act.h"

namespace tgcn {
namespace {

constexpr int64_t kBdMagic = 0x31474449424b4c42ll;
constexpr int kBdMaxMembers = 128;
constexpr int kBdMaxH = 256;      // dW: one workgroup holds all h rows of a member's dW (4 waves x 2 tiles of 32)
constexpr int kBdRows = 128;      // the row tile of the forward and of dX
constexpr int kBdWRows = 32;      // rows of X and G that dW stages at a time
constexpr int kBdWGroup = 128;    // columns of a member's dW of one dW launch (4 tiles)
constexpr int64_t kBdMaxTiles = (int64_t(1) << 24) - 1;   // row tiles: a grid of 256-thread workgroups stays below 2^32 threads along x

// The layout blob: BdHeader | BdMember [K], the same bytes on the host and the device.
struct BdHeader {
    int64_t magic, bytes, K, h, n_cols, n_max, own_max, any_drop;
};
struct BdMember {
    int32_t col0, n;        // the segment
    int32_t own0, own1;     // the columns this member writes: its segment and the pad columns around it (zeros)
    uint32_t thresh;        // keep iff hash >= thresh
    float scale;            // 1 / (1 - p)
    int32_t drop, pad;      // p > 0
};

struct BdDrop {   // per workgroup: the member's dropout, off when the call has no seeds
    bool on;
    uint32_t s_lo, s_hi, thresh;
    float scale;
};

__device__ __forceinline__ BdDrop drop_of(const BdMember &m, const uint64_t *seeds, int k) {
    BdDrop d;
    d.on = seeds != nullptr && m.drop != 0;
    const uint64_t seed = d.on ? seeds[k] : 0ull;
    d.s_lo = static_cast<uint32_t>(seed);
    d.s_hi = static_cast<uint32_t>(seed >> 32);
    d.thresh = m.thresh;
    d.scale = m.scale;
    return d;
}

__device__ __forceinline__ uint32_t key_of(const BdDrop &d, int64_t mask_row) {
    return d.on ? drop_row_key(d.s_lo, d.s_hi, mask_row) : 0u;
}

__device__ __forceinline__ float dropped(float v, const BdDrop &d, uint32_t key, int col) {
    if (d.on) return drop_hash_keep(key, drop_col_term(col), d.thresh) ? v * d.scale : 0.f;
    return v;
}

// ---------------------------------------------------------------------------------------------
// Forward: 128 rows (blockIdx.x) of member blockIdx.y.  `cg0`: the first column of this launch inside every segment
// (groups of kFwdGroup); the launch with cg0 = 0 also writes the zeros of the member's pad columns.
// ---------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256, 2) void k_bd_fwd(const BdMember *__restrict__ members, const uint64_t *__restrict__ seeds,
                                                   const float *__restrict__ X, int64_t ldx, const float *__restrict__ W,
                                                   int64_t ldw, float *__restrict__ C, int64_t ldc, int64_t N, int h, int cg0,
                                                   int64_t mask_row0) {
    constexpr int KC = 32, NP = 32 * NT, LDW = NP + 32, LDX = KC + 1;
    __shared__ float Ws[KC * LDW];                         // [kk][m]
    __shared__ float Xs[kBdRows * LDX];
    const int member = blockIdx.y;
    const BdMember mem = members[member];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t blk0 = int64_t(blockIdx.x) * kBdRows;
    if (cg0 == 0) {
        const int lo = mem.col0 - mem.own0, padw = lo + mem.own1 - (mem.col0 + mem.n);
        const int rows = static_cast<int>(min(int64_t(kBdRows), N - blk0));
        for (int e = tid; e < rows * padw; e += 256) {
            const int r = e / padw, q = e % padw;
            C[(blk0 + r) * ldc + (q < lo ? mem.own0 + q : mem.col0 + mem.n + (q - lo))] = 0.f;
        }
    }
    const int n = min(mem.n - cg0, kFwdGroup);
    if (n <= 0) return;                                    // (the whole workgroup: no barrier has been reached)
    const BdDrop d = drop_of(mem, seeds, member);
    X += int64_t(member) * h;
    W += mem.col0 + cg0;
    C += mem.col0 + cg0;
    const int64_t row0 = blk0 + wave * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const uint32_t key = key_of(d, i + mask_row0);
    const int skk = tid & 31, sr = tid >> 5;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int k0 = 0; k0 < h; k0 += KC) {
        __syncthreads();                                   // the previous chunk has been read
#pragma unroll 4
        for (int u = 0; u < 4 * NT; ++u) {                 // lanes along a row of W
            const int e = tid + 256 * u, kk = e / NP, m = e % NP;
            Ws[kk * LDW + m] = (k0 + kk < h && m < n) ? W[int64_t(k0 + kk) * ldw + m] : 0.f;
        }
        const bool kin = k0 + skk < h;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = sr + 8 * u;
            Xs[r * LDX + skk] = (kin && blk0 + r < N) ? X[(blk0 + r) * ldx + k0 + skk] : 0.f;
        }
        __syncthreads();
        const float *xr = Xs + (wave * 32 + c) * LDX;
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int kk = 2 * s + half, k = k0 + kk;
            const float a = (live && k < h) ? dropped(xr[kk], d, key, k) : 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Ws[kk * LDW + 32 * t + c], acc[t], 0, 0, 0);
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
// dX: 128 rows of member blockIdx.y.  `mg0`: the first index m of this launch's piece of the reduction (pieces of
// kGzGroup; a later piece adds to what dX holds).  The launch that holds a member's LAST piece also leaves the column sums
// of the stored dX over the tile's rows at part[tile][k h + j]: thread-local over the lane's 16 rows in register order,
// then over the 8 half waves in order.
// ---------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256, 2) void k_bd_grad_x(const BdMember *__restrict__ members, const uint64_t *__restrict__ seeds,
                                                      const float *__restrict__ W, int64_t ldw, const float *__restrict__ G,
                                                      int64_t ldg, float *__restrict__ dX, int64_t lddx,
                                                      float *__restrict__ part, int64_t N, int h, int mg0, int64_t mask_row0) {
    constexpr int NP = 32 * NT;
    __shared__ float Ws[NP * 33];                          // [m][j]
    __shared__ float Gs[4 * 32 * 33];
    __shared__ float cs[8 * 32];
    const int member = blockIdx.y;
    const BdMember mem = members[member];
    const int n = min(mem.n - mg0, kGzGroup);
    if (n <= 0) return;                                    // (mg0 > 0: what dX and part hold is already the whole sum)
    const bool accum = mg0 > 0, last = mg0 + kGzGroup >= mem.n;
    const BdDrop d = drop_of(mem, seeds, member);
    W += mem.col0 + mg0;
    G += mem.col0 + mg0;
    dX += int64_t(member) * h;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t row0 = int64_t(blockIdx.x) * kBdRows + wave * 32;
    float *gw = Gs + wave * (32 * 33);                     // this wave's 32 x 32 tile of G, [row][33]
    float g[16 * NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int m = 32 * t + c;
#pragma unroll
        for (int u = 0; u < 16; ++u) {                     // lanes along a row of G
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
    for (int r = 0; r < 16; ++r) keys[r] = key_of(d, row0 + acc_row(r, half) + mask_row0);

    for (int j0 = 0; j0 < h; j0 += 32) {
        __syncthreads();                                   // the previous tile has been read
#pragma unroll 4
        for (int u = 0; u < 4 * NT; ++u) {                 // lanes along a row of W
            const int e = tid + 256 * u, jj = e / NP, m = e % NP;
            Ws[m * 33 + jj] = (j0 + jj < h && m < n) ? W[int64_t(j0 + jj) * ldw + m] : 0.f;
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16 * NT; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g[s], Ws[(2 * s + half) * 33 + c], acc, 0, 0, 0);
        const int j = j0 + c;
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + acc_row(r, half);
            if (row < N && j < h) {
                float v = dropped(acc[r], d, keys[r], j);
                float *out = dX + row * lddx + j;
                if (accum) v += *out;
                *out = v;
                sum += v;
            }
        }
        if (last && part != nullptr) {                     // (uniform)
            cs[(2 * wave + half) * 32 + c] = sum;
            __syncthreads();
            if (tid < 32 && j0 + tid < h) {
                float v = 0.f;
#pragma unroll
                for (int q = 0; q < 8; ++q) v += cs[q * 32 + tid];
                part[(int64_t(blockIdx.x) * gridDim.y + member) * h + j0 + tid] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dW: slice blockIdx.x of the rows (whole chunks of kWChunk rows, grad_w_split) for member blockIdx.y.  Wave w owns the
// tiles w, w + 4 (TJ = 2) of the h rows of dW and NT tiles of columns; `cg0`: the first column of this launch inside every
// segment (groups of kBdWGroup = `ng` columns at most).  The partial sums of slice q lie at part[q][k][j][m], stride ng.
// ---------------------------------------------------------------------------------------------
template <int TJ, int NT>
__global__ __launch_bounds__(256, 2) void k_bd_grad_w(const BdMember *__restrict__ members, const uint64_t *__restrict__ seeds,
                                                      const float *__restrict__ X, int64_t ldx, const float *__restrict__ G,
                                                      int64_t ldg, float *__restrict__ part, int64_t N, int h, int cg0, int ng,
                                                      int64_t rows_per_slice, int64_t mask_row0) {
    constexpr int HP = 128 * TJ, NP = 32 * NT, LDA = HP + 32, LDG = NP + 32;
    __shared__ float As[kBdWRows * LDA];
    __shared__ float Gs[kBdWRows * LDG];
    __shared__ uint32_t ks[kBdWRows];
    const int member = blockIdx.y;
    const BdMember mem = members[member];
    const int n = min(mem.n - cg0, kBdWGroup);
    if (n <= 0) return;                                    // (k_bd_reduce_w reads nothing of this member in this launch)
    const BdDrop d = drop_of(mem, seeds, member);
    X += int64_t(member) * h;
    G += mem.col0 + cg0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int64_t i_begin = min(N, int64_t(blockIdx.x) * rows_per_slice), i_end = min(N, i_begin + rows_per_slice);
    f32x16 acc[TJ][NT];
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tj][t][r] = 0.f;

    for (int64_t i0 = i_begin; i0 < i_end; i0 += kBdWRows) {
        __syncthreads();                                   // the previous chunk has been read
        if (tid < kBdWRows) ks[tid] = key_of(d, i0 + tid + mask_row0);
        __syncthreads();
#pragma unroll 4
        for (int u = 0; u < 16 * TJ; ++u) {                // lanes along a row of X
            const int e = tid + 256 * u, r = e / HP, j = e % HP;
            const int64_t i = i0 + r;
            As[r * LDA + j] = (i < i_end && j < h) ? dropped(X[i * ldx + j], d, ks[r], j) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4 * NT; ++u) {
            const int e = tid + 256 * u, r = e / NP, m = e % NP;
            const int64_t i = i0 + r;
            Gs[r * LDG + m] = (i < i_end && m < n) ? G[i * ldg + m] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj) {
            const int jt = wave + 4 * tj;
            if (jt * 32 < h) {                             // (per wave: a tile of padding adds nothing)
#pragma unroll
                for (int s = 0; s < kBdWRows / 2; ++s) {
                    const int ii = 2 * s + half;
                    const float a = As[ii * LDA + jt * 32 + c];
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[tj][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Gs[ii * LDG + 32 * t + c], acc[tj][t], 0, 0, 0);
                }
            }
        }
    }
    float *out = part + (int64_t(blockIdx.x) * gridDim.y + member) * h * ng;
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (wave + 4 * tj) * 32 + acc_row(r, half), m = 32 * t + c;
                if (j < h && m < n) out[int64_t(j) * ng + m] = acc[tj][t][r];
            }
}

// dW[j, col] for the columns member blockIdx.y owns: the sum over the slices, in order, inside this launch's piece of the
// segment; exact zeros in the pad columns (written by the launch with cg0 = 0).
__global__ __launch_bounds__(256) void k_bd_reduce_w(const BdMember *__restrict__ members, const float *__restrict__ part,
                                                     int slices, int h, int cg0, int ng, int own_max, float *__restrict__ dW,
                                                     int64_t lddw) {
    const BdMember mem = members[blockIdx.y];
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= int64_t(h) * own_max) return;
    const int j = static_cast<int>(e / own_max), col = mem.own0 + static_cast<int>(e % own_max);
    if (col >= mem.own1) return;
    if (col < mem.col0 || col >= mem.col0 + mem.n) {
        if (cg0 == 0) dW[int64_t(j) * lddw + col] = 0.f;
        return;
    }
    const int m = col - mem.col0 - cg0;
    if (m < 0 || m >= ng) return;
    const int64_t slice_stride = int64_t(gridDim.y) * h * ng;
    const float *p = part + (int64_t(blockIdx.y) * h + j) * ng + m;
    float s = 0.f;
    for (int q = 0; q < slices; ++q) s += p[q * slice_stride];
    dW[int64_t(j) * lddw + col] = s;
}

int64_t row_tiles(int64_t N) { return (N + kBdRows - 1) / kBdRows; }

void dw_split(const BdHeader &hd, int64_t N, int64_t &slices, int64_t &rows_per_slice) {
    int64_t cps;
    grad_w_split(N, 32 * static_cast<int>(hd.K), kWTarget, slices, cps);   // about kWTarget workgroups over K members
    rows_per_slice = cps * kWChunk;
}

size_t colsum_floats(const BdHeader &hd, int64_t N) { return static_cast<size_t>(row_tiles(N) * hd.K * hd.h); }

size_t dw_floats(const BdHeader &hd, int64_t N) {
    int64_t slices, rps;
    dw_split(hd, N, slices, rps);
    return static_cast<size_t>(slices * hd.K * hd.h * std::min<int64_t>(hd.n_max, kBdWGroup));
}

int read_header(const char *fn, const void *layout_host, const void *layout_dev, BdHeader &hd) {
    TGCN_CHECK(check_ptr(fn, "layout_host", layout_host));
    std::memcpy(&hd, layout_host, sizeof(BdHeader));
    if (hd.magic != kBdMagic) {
        set_error("%s: layout_host is not a blob of tgcn_blockdiag_layout", fn);
        return TGCN_E_INVALID;
    }
    return check_ptr(fn, "layout_dev", layout_dev);
}

int check_rows(const char *fn, int64_t N, int64_t mask_row0) {
    if (N < 0 || row_tiles(N) > kBdMaxTiles) {
        set_error("%s: N must be in [0, 128 * (2^24 - 1)] (N=%lld)", fn, (long long)N);
        return TGCN_E_INVALID;
    }
    if (mask_row0 < 0) {
        set_error("%s: mask_row0 must be >= 0 (%lld)", fn, (long long)mask_row0);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_blockdiag_max_hidden(void) { return tgcn::kBdMaxH; }

size_t tgcn_blockdiag_layout_bytes(int K) {
    using namespace tgcn;
    return (K < 1 || K > kBdMaxMembers) ? 0 : sizeof(BdHeader) + sizeof(BdMember) * static_cast<size_t>(K);
}

int tgcn_blockdiag_layout(int K, int h, int64_t n_cols, const int32_t *col0, const int32_t *n, const double *p, void *out,
                          size_t out_bytes) {
    using namespace tgcn;
    const char *fn = "tgcn_blockdiag_layout";
    if (K < 1 || K > kBdMaxMembers) {
        set_error("%s: K must be in [1, %d] (K=%d)", fn, kBdMaxMembers, K);
        return TGCN_E_INVALID;
    }
    if (h < 1 || h > kBdMaxH) {
        set_error("%s: h must be in [1, %d] (h=%d)", fn, kBdMaxH, h);
        return TGCN_E_INVALID;
    }
    if (n_cols < 1 || n_cols > INT_MAX) {
        set_error("%s: n_cols must be in [1, 2^31) (n_cols=%lld)", fn, (long long)n_cols);
        return TGCN_E_INVALID;
    }
    TGCN_CHECK(check_ptr(fn, "col0", col0));
    TGCN_CHECK(check_ptr(fn, "n", n));
    TGCN_CHECK(check_ptr(fn, "out", out));
    int64_t at = 0;
    int n_max = 0;
    bool any = false;
    for (int k = 0; k < K; ++k) {
        if (n[k] < 1) {
            set_error("%s: member %d has n = %d columns, need >= 1", fn, k, n[k]);
            return TGCN_E_INVALID;
        }
        if (col0[k] < at) {
            set_error("%s: the segment of member %d starts at column %d, before the end %lld of the one before it (segments "
                      "must increase and must not overlap)", fn, k, col0[k], (long long)at);
            return TGCN_E_INVALID;
        }
        at = int64_t(col0[k]) + n[k];
        if (at > n_cols) {
            set_error("%s: columns [%d, %lld) of member %d are outside the %lld columns", fn, col0[k], (long long)at, k,
                      (long long)n_cols);
            return TGCN_E_INVALID;
        }
        const double pk = p ? p[k] : 0.0;
        if (!(pk >= 0.0 && pk < 1.0)) {
            set_error("%s: the rate of member %d must be in [0, 1) (p=%g)", fn, k, pk);
            return TGCN_E_INVALID;
        }
        any = any || pk > 0.0;
        n_max = std::max(n_max, n[k]);
    }
    const size_t need = tgcn_blockdiag_layout_bytes(K);
    if (out_bytes < need) {
        set_error("%s: out of %zu bytes, tgcn_blockdiag_layout_bytes() asks for %zu", fn, out_bytes, need);
        return TGCN_E_INVALID;
    }
    std::memset(out, 0, need);
    BdHeader hd{};
    hd.magic = kBdMagic;
    hd.bytes = static_cast<int64_t>(need);
    hd.K = K;
    hd.h = h;
    hd.n_cols = n_cols;
    hd.n_max = n_max;
    hd.any_drop = any;
    BdMember *mm = reinterpret_cast<BdMember *>(static_cast<char *>(out) + sizeof(BdHeader));
    for (int k = 0; k < K; ++k) {
        const double pk = p ? p[k] : 0.0;
        BdMember &m = mm[k];
        m.col0 = col0[k];
        m.n = n[k];
        m.own0 = k == 0 ? 0 : col0[k];
        m.own1 = k + 1 < K ? col0[k + 1] : static_cast<int32_t>(n_cols);
        m.drop = pk > 0.0;
        m.thresh = m.drop ? drop_threshold(pk) : 0u;
        m.scale = m.drop ? static_cast<float>(1.0 / (1.0 - pk)) : 1.f;
        hd.own_max = std::max<int64_t>(hd.own_max, m.own1 - m.own0);
    }
    std::memcpy(out, &hd, sizeof(BdHeader));
    return TGCN_OK;
}

int tgcn_blockdiag_xw(const float *X, int64_t ldx, const float *W, int64_t ldw, float *C, int64_t ldc, int64_t N,
                      const void *layout_host, const void *layout_dev, const uint64_t *seeds, int64_t mask_row0,
                      tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_blockdiag_xw";
    BdHeader hd;
    TGCN_CHECK(read_header(fn, layout_host, layout_dev, hd));
    TGCN_CHECK(check_rows(fn, N, mask_row0));
    TGCN_CHECK(check_ld(fn, "ldx", ldx, hd.K * hd.h));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, hd.n_cols));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, hd.n_cols));
    if (N == 0) return TGCN_OK;                // C has no row
    TGCN_CHECK(check_ptr(fn, "X", X));
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "C", C));
    const BdMember *members = reinterpret_cast<const BdMember *>(static_cast<const char *>(layout_dev) + sizeof(BdHeader));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int h = static_cast<int>(hd.h), n = static_cast<int>(hd.n_max);
    const dim3 grid(static_cast<unsigned>(row_tiles(N)), static_cast<unsigned>(hd.K));
    for (int cg0 = 0; cg0 < n; cg0 += kFwdGroup) {
        const int nt = (std::min(n - cg0, kFwdGroup) + 31) / 32;
        with_tiles<1, 2, 4, 8>(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_bd_fwd<decltype(NT)::value>), grid, dim3(256), 0, s, members, seeds, X, ldx, W, ldw, C, ldc,
                               N, h, cg0, mask_row0);
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

size_t tgcn_blockdiag_xw_grad_workspace_bytes(const void *layout_host, int64_t N) {
    using namespace tgcn;
    if (!layout_host || N < 0 || row_tiles(N) > kBdMaxTiles) return 0;
    BdHeader hd;
    std::memcpy(&hd, layout_host, sizeof(BdHeader));
    if (hd.magic != kBdMagic) return 0;
    return (colsum_floats(hd, N) + dw_floats(hd, N)) * sizeof(float);
}

int tgcn_blockdiag_xw_grad(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *G, int64_t ldg, float *dX,
                           int64_t lddx, float *colsum, float *dW, int64_t lddw, int64_t N, const void *layout_host,
                           const void *layout_dev, const uint64_t *seeds, int64_t mask_row0, void *workspace,
                           size_t workspace_bytes, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_blockdiag_xw_grad";
    BdHeader hd;
    TGCN_CHECK(read_header(fn, layout_host, layout_dev, hd));
    TGCN_CHECK(check_rows(fn, N, mask_row0));
    TGCN_CHECK(check_ld(fn, "ldx", ldx, hd.K * hd.h));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, hd.n_cols));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, hd.n_cols));
    if (dX) TGCN_CHECK(check_ld(fn, "lddx", lddx, hd.K * hd.h));
    if (dW) TGCN_CHECK(check_ld(fn, "lddw", lddw, hd.n_cols));
    if ((dX == nullptr) != (colsum == nullptr) && !(N == 0 && colsum != nullptr)) {   // (N = 0: dX has no element)
        set_error("%s: dX and colsum are computed together: pass both or neither (colsum is the column sum of dX)", fn);
        return TGCN_E_INVALID;
    }
    if (!colsum && !dW) {
        set_error("%s: dX (with colsum) and dW are both NULL: nothing to compute", fn);
        return TGCN_E_INVALID;
    }
    if (N > 0) {
        TGCN_CHECK(check_ptr(fn, "G", G));
        if (colsum) TGCN_CHECK(check_ptr(fn, "W", W));
        if (dW) TGCN_CHECK(check_ptr(fn, "X", X));
    }
    const size_t need = tgcn_blockdiag_xw_grad_workspace_bytes(layout_host, N);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace of %zu bytes, tgcn_blockdiag_xw_grad_workspace_bytes() asks for %zu", fn,
                  workspace ? workspace_bytes : size_t(0), need);
        return TGCN_E_WORKSPACE;
    }
    const BdMember *members = reinterpret_cast<const BdMember *>(static_cast<const char *>(layout_dev) + sizeof(BdHeader));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int h = static_cast<int>(hd.h), n = static_cast<int>(hd.n_max), K = static_cast<int>(hd.K);
    float *part_c = static_cast<float *>(workspace);
    float *part_w = part_c + colsum_floats(hd, N);
    if (colsum) {
        const int64_t tiles = row_tiles(N);
        if (tiles > 0) {
            const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(K));
            for (int mg0 = 0; mg0 < n; mg0 += kGzGroup) {
                const int nt = (std::min(n - mg0, kGzGroup) + 31) / 32;
                with_tiles<1, 2, 4>(nt, [&](auto NT) {
                    hipLaunchKernelGGL((k_bd_grad_x<decltype(NT)::value>), grid, dim3(256), 0, s, members, seeds, W, ldw, G, ldg,
                                       dX, lddx, part_c, N, h, mg0, mask_row0);
                });
            }
        }
        launch_reduce_slices<float>(part_c, tiles, int64_t(K) * h, 0, 1, K * h, colsum, int64_t(K) * h, s);
    }
    if (dW) {
        int64_t slices, rps;
        dw_split(hd, N, slices, rps);
        const dim3 grid(static_cast<unsigned>(slices), static_cast<unsigned>(K));
        const int own_max = static_cast<int>(hd.own_max);
        const dim3 rgrid(static_cast<unsigned>((int64_t(h) * own_max + 255) / 256), static_cast<unsigned>(K));
        for (int cg0 = 0; cg0 < n; cg0 += kBdWGroup) {
            const int ng = std::min(n - cg0, kBdWGroup), nt = (ng + 31) / 32;
            with_tiles<1, 2, 4>(nt, [&](auto NT) {
                if (h > 128)
                    hipLaunchKernelGGL((k_bd_grad_w<2, decltype(NT)::value>), grid, dim3(256), 0, s, members, seeds, X, ldx, G,
                                       ldg, part_w, N, h, cg0, ng, rps, mask_row0);
                else
                    hipLaunchKernelGGL((k_bd_grad_w<1, decltype(NT)::value>), grid, dim3(256), 0, s, members, seeds, X, ldx, G,
                                       ldg, part_w, N, h, cg0, ng, rps, mask_row0);
            });
            hipLaunchKernelGGL(k_bd_reduce_w, rgrid, dim3(256), 0, s, members, part_w, static_cast<int>(slices), h, cg0, ng,
                               own_max, dW, lddw);
        }
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // extern "C"
