// The per-label strategy of the reference's MLP baseline (MLP_label.py: one MLP per top-level label, each trained on that
// label's documents) as ONE network: the products of mlp.hip with a weight that depends on the row's group.  The rows lie
// in grouped order -- the rows of group 0, then group 1, ... (row_ptr [K + 1]); rows at or past row_ptr[K] belong to
// nobody and are never touched.  For row i of group g, with a(i, j) = s * keep(i, j) * selu(Z[i, j] + b[b_off_g + j]):
//     tgcn_mlp_grouped_act_linear        C[i, col0_g + m] = sum_j a(i, j) W[w_row0_g + m, j] (+ c[col0_g + m]),  m < n_g
//     tgcn_mlp_grouped_act_linear_grad   dZ[i, j] = s keep selu'(.) sum_m G[i, col0_g + m] W[w_row0_g + m, j]
//                                        db[b_off_g + j] = sum over the rows i of group g of dZ[i, j]
//                                        dW[w_row0_g + m, j] = sum over the rows i of group g of G[i, col0_g + m] a(i, j)
//                                        dc[col0_g + m] = sum over the rows i of group g of G[i, col0_g + m]
// keep(i, j) is the hash of drop_hash.h for mask row mask_row0 + i (i the row's index in grouped order) and column j.
//
// The kernels run the bodies of mlp.hip's (mlp_products.h: mlp_fwd and mlp_grad_z with CLS = false, mlp_grad_w) with one
// indirection: a workgroup does not own rows 128 blockIdx.x ... but one TILE of a table built on the host
// (tgcn_mlp_grouped_layout): at most 128 rows that all belong to one group, so the W / b tiles it stages in LDS are that
// group's, and the rows past the tile's count are masked as the rows past N are.  A kernel here reads its tile or slice
// and its group, moves W, b, G, C and c to the group's and calls the body.  The sums of an element run over k (forward)
// and over m (dZ) in the one body, whatever the row tiling: group g's slice of C and dZ has the bits of
// tgcn_mlp_act_linear* on Z[row_ptr[g] : row_ptr[g + 1]] with mask_row0 + row_ptr[g].  dW is cut into slices of whole
// chunks of kWChunk rows inside one group and reduced per group in slice order, db is a column sum per tile reduced per
// group in tile order: no atomics, the host never loops over the groups, and the launch count depends on n and k only.
#include <algorithm>
#include <cstring>

#include "mlp_products.h"

namespace tgcn {
namespace {

// The layout blob: GHeader | GGroup [K] | GTile [n_tiles] | GSlice [n_slices], the same bytes on the host and the device.
constexpr int64_t kGMagic = 0x4c50524754474e31ll;
constexpr int kMaxGroups = 128;

struct GHeader {
    int64_t magic, bytes, K, N, k, w_rows, c_cols, b_len, n_max, n_tiles, n_slices, chunks_per_slice;
};
struct GGroup {
    int64_t row0, rows;
    int32_t w_row0, n, col0, b_off;
    int32_t tile0, n_tiles, slice0, n_slices;
};
struct GTile {
    int64_t row0;
    int32_t group, count;
};
struct GSlice {
    int64_t row0, row_end;
    int32_t group, pad;
};

struct GTables {   // the blob's parts in device memory
    const GGroup *groups;
    const GTile *tiles;
    const GSlice *slices;
};

inline GTables tables_of(const void *blob, const GHeader &h) {
    const char *p = static_cast<const char *>(blob) + sizeof(GHeader);
    GTables t;
    t.groups = reinterpret_cast<const GGroup *>(p);
    t.tiles = reinterpret_cast<const GTile *>(p + sizeof(GGroup) * h.K);
    t.slices = reinterpret_cast<const GSlice *>(p + sizeof(GGroup) * h.K + sizeof(GTile) * h.n_tiles);
    return t;
}

// ---------------------------------------------------------------------------------------------
// Forward: mlp_fwd on one tile of the table.  `cg0`: the first result column of this launch inside every group's n_g
// columns (groups of kFwdGroup); a group that is narrower than cg0 has nothing here.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP>
__global__ __launch_bounds__(256, 2) void k_gmlp_fwd(const GTile *__restrict__ tiles, const GGroup *__restrict__ groups,
                                                     const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                     const float *__restrict__ W, int64_t ldw, const float *__restrict__ cb,
                                                     float *__restrict__ C, int64_t ldc, int K, int cg0, const RowDrop d) {
    const GTile tile = tiles[blockIdx.x];
    const GGroup grp = groups[tile.group];
    const int n = min(grp.n - cg0, kFwdGroup);
    if (n <= 0) return;                                    // (the whole workgroup: no barrier has been reached)
    mlp_fwd<NT, DROP, false>(Z, ldz, b + grp.b_off, W + int64_t(grp.w_row0 + cg0) * ldw, ldw,
                             cb != nullptr ? cb + grp.col0 + cg0 : nullptr, C + grp.col0 + cg0, ldc, tile.row0,
                             tile.row0 + tile.count, K, n, d, ClassTerm{});
}

// ---------------------------------------------------------------------------------------------
// dZ: mlp_grad_z on one tile of the table.  `mg0`: the first index m of this launch's piece of the reduction (pieces of
// kGzGroup; `accum` on every piece but the first, as in mlp.hip); a group with n_g <= mg0 adds nothing.
// ---------------------------------------------------------------------------------------------
template <int NT, bool DROP>
__global__ __launch_bounds__(256, 2) void k_gmlp_grad_z(const GTile *__restrict__ tiles, const GGroup *__restrict__ groups,
                                                        const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                        const float *__restrict__ W, int64_t ldw,
                                                        const float *__restrict__ G, int64_t ldg, float *__restrict__ dZ,
                                                        int64_t lddz, int K, int mg0, const RowDrop d) {
    const GTile tile = tiles[blockIdx.x];
    const GGroup grp = groups[tile.group];
    const int n = min(grp.n - mg0, kGzGroup);
    if (n <= 0) return;                                    // (mg0 > 0: what dZ holds is already the whole sum)
    mlp_grad_z<NT, DROP, false>(Z, ldz, b + grp.b_off, W + int64_t(grp.w_row0 + mg0) * ldw, ldw, G + grp.col0 + mg0, ldg, dZ,
                                lddz, tile.row0, tile.row0 + tile.count, K, n, mg0 > 0, d, ClassTerm{});
}

// ---------------------------------------------------------------------------------------------
// dW: mlp_grad_w on one slice of the table (blockIdx.y): whole chunks of kWChunk rows of ONE group, so the bias and the
// columns of G are that group's.  `m0`: the first row of dW of this launch inside every group's n_g rows (groups of
// kWGroup).  The partial sums of slice q lie at part[q], as in mlp.hip; k_gmlp_reduce_w adds a group's slices.
// ---------------------------------------------------------------------------------------------
template <int TW, bool DROP>
__global__ __launch_bounds__(256, 2) void k_gmlp_grad_w(const GSlice *__restrict__ slices, const GGroup *__restrict__ groups,
                                                        const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                        const float *__restrict__ G, int64_t ldg, float *__restrict__ part,
                                                        int K, int m0, const RowDrop d) {
    const GSlice slice = slices[blockIdx.y];
    const GGroup grp = groups[slice.group];
    const int n = min(grp.n - m0, kWGroup);
    if (n <= 0) return;                                    // (k_gmlp_reduce_w reads no row of this group in this launch)
    mlp_grad_w<TW, DROP>(Z, ldz, b + grp.b_off, G + grp.col0 + m0, ldg, part, slice.row0, slice.row_end, K, n, d);
}

// dW[w_row0_g + m0 + r, j] = the sum over the slices of group g (blockIdx.y), in order, of their partial sums: reduce_slices
// (fused_act.h) on the slice range taken from the table.  A group without rows has no slice: exact zeros.
__global__ __launch_bounds__(256) void k_gmlp_reduce_w(const float *__restrict__ part, const GGroup *__restrict__ groups,
                                                       int64_t slice_stride, int row_stride, int cols, int m0,
                                                       float *__restrict__ dW, int64_t lddw) {
    const GGroup grp = groups[blockIdx.y];
    const int rows = min(grp.n - m0, kWGroup);
    if (rows <= 0) return;
    reduce_slices(part + int64_t(grp.slice0) * slice_stride, grp.n_slices, slice_stride, row_stride, rows, cols,
                  dW + int64_t(grp.w_row0 + m0) * lddw, lddw);
}

// db, first pass: the column sums of dZ over one tile (blockIdx.x) for 32 columns (blockIdx.y).  Thread (sr, c) adds rows
// sr, sr + 8, ... of column c; the 8 partial sums are added in the order of sr.
__global__ __launch_bounds__(256) void k_gmlp_colsum_tiles(const GTile *__restrict__ tiles, const float *__restrict__ dZ,
                                                           int64_t lddz, int K, float *__restrict__ part) {
    __shared__ float red[8 * 32];
    const GTile tile = tiles[blockIdx.x];
    const int c = threadIdx.x & 31, sr = threadIdx.x >> 5;
    const int j = blockIdx.y * 32 + c;
    float s = 0.f;
#pragma unroll 4
    for (int u = 0; u < 16; ++u) {
        const int r = sr + 8 * u;
        if (r < tile.count && j < K) s += dZ[(tile.row0 + r) * lddz + j];
    }
    red[sr * 32 + c] = s;
    __syncthreads();
    if (sr == 0 && j < K) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += red[q * 32 + c];
        part[int64_t(blockIdx.x) * K + j] = v;
    }
}

// db, second pass: db[b_off_g + j] = the sum over the tiles of group g (blockIdx.y), in order; no tile: an exact zero.
// OWN_COLS (dc, the column sums of G): only the group's own columns [col0_g, col0_g + n_g), written in place.
template <bool OWN_COLS>
__global__ __launch_bounds__(256) void k_gmlp_colsum_groups(const GGroup *__restrict__ groups, const float *__restrict__ part,
                                                            int K, float *__restrict__ out) {
    const GGroup grp = groups[blockIdx.y];
    int j = blockIdx.x * 256 + threadIdx.x;
    if (OWN_COLS ? j >= grp.n : j >= K) return;
    if (OWN_COLS) j += grp.col0;
    const float *p = part + int64_t(grp.tile0) * K + j;
    float s = 0.f;
    for (int q = 0; q < grp.n_tiles; ++q) s += p[int64_t(q) * K];
    out[OWN_COLS ? j : grp.b_off + j] = s;
}

// the workspace: the tiles' column sums (of dZ for db, of G for dc) first, the slices' partial sums of dW after them
size_t gdb_floats(const GHeader &h) { return static_cast<size_t>(h.n_tiles) * static_cast<size_t>(std::max(h.k, h.c_cols)); }

size_t gdw_floats(const GHeader &h) {
    const int64_t kpad = (h.k + 31) / 32 * 32;
    const int64_t np = std::min<int64_t>(h.n_max, kWGroup) > 128 ? 256 : 128;
    return static_cast<size_t>(h.n_slices * np * kpad);
}

template <bool DROP>
int launch_gfwd(const GHeader &h, const GTables &t, const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw,
                const float *cb, float *C, int64_t ldc, const RowDrop &d, hipStream_t s) {
    const int K = static_cast<int>(h.k), n = static_cast<int>(h.n_max);
    const unsigned grid = static_cast<unsigned>(h.n_tiles);
    for (int cg0 = 0; cg0 < n; cg0 += kFwdGroup) {
        const int nt = (std::min(n - cg0, kFwdGroup) + 31) / 32;
        with_tiles<1, 2, 4, 8>(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_gmlp_fwd<decltype(NT)::value, DROP>), dim3(grid), dim3(256), 0, s, t.tiles, t.groups, Z, ldz,
                               b, W, ldw, cb, C, ldc, K, cg0, d);
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_ggrad_z(const GHeader &h, const GTables &t, const float *Z, int64_t ldz, const float *b, const float *W,
                   int64_t ldw, const float *G, int64_t ldg, float *dZ, int64_t lddz, const RowDrop &d, hipStream_t s) {
    const int K = static_cast<int>(h.k), n = static_cast<int>(h.n_max);
    const unsigned grid = static_cast<unsigned>(h.n_tiles);
    for (int mg0 = 0; mg0 < n; mg0 += kGzGroup) {
        const int nt = (std::min(n - mg0, kGzGroup) + 31) / 32;
        with_tiles<1, 2, 4>(nt, [&](auto NT) {
            hipLaunchKernelGGL((k_gmlp_grad_z<decltype(NT)::value, DROP>), dim3(grid), dim3(256), 0, s, t.tiles, t.groups, Z,
                               ldz, b, W, ldw, G, ldg, dZ, lddz, K, mg0, d);
        });
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

template <bool DROP>
int launch_ggrad_w(const GHeader &h, const GTables &t, const float *Z, int64_t ldz, const float *b, const float *G,
                   int64_t ldg, float *dW, int64_t lddw, const RowDrop &d, float *part, hipStream_t s) {
    const int K = static_cast<int>(h.k), n = static_cast<int>(h.n_max);
    const int ktiles = (K + 31) / 32, kpad = ktiles * 32;
    const int np = std::min(n, kWGroup) > 128 ? 256 : 128;
    for (int m0 = 0; m0 < n; m0 += kWGroup) {
        const int ng = std::min(n - m0, kWGroup);
        if (h.n_slices > 0) {
            const dim3 grid(ktiles, static_cast<unsigned>(h.n_slices));
            if (np == 256)
                hipLaunchKernelGGL((k_gmlp_grad_w<2, DROP>), grid, dim3(256), 0, s, t.slices, t.groups, Z, ldz, b, G, ldg, part,
                                   K, m0, d);
            else
                hipLaunchKernelGGL((k_gmlp_grad_w<1, DROP>), grid, dim3(256), 0, s, t.slices, t.groups, Z, ldz, b, G, ldg, part,
                                   K, m0, d);
        }
        const dim3 rgrid(static_cast<unsigned>((int64_t(ng) * K + 255) / 256), static_cast<unsigned>(h.K));
        hipLaunchKernelGGL(k_gmlp_reduce_w, rgrid, dim3(256), 0, s, part, t.groups, int64_t(np) * kpad, kpad, K, m0, dW, lddw);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// the grouped column sums of X [N, cols]: db from dZ (every column, at b_off_g) or dc from G (the group's own columns)
template <bool OWN_COLS>
int launch_gcolsum(const GHeader &h, const GTables &t, const float *X, int64_t ldx, int cols, float *out, float *part,
                   hipStream_t s) {
    if (h.n_tiles > 0)
        hipLaunchKernelGGL(k_gmlp_colsum_tiles, dim3(static_cast<unsigned>(h.n_tiles), (cols + 31) / 32), dim3(256), 0, s,
                           t.tiles, X, ldx, cols, part);
    hipLaunchKernelGGL(k_gmlp_colsum_groups<OWN_COLS>, dim3((cols + 255) / 256, static_cast<unsigned>(h.K)), dim3(256), 0, s,
                       t.groups, part, cols, out);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

// the header of a blob that tgcn_mlp_grouped_layout filled, checked against the call's N and k
int read_header(const char *fn, const void *layout_host, const void *layout_dev, int64_t N, int k, GHeader &h) {
    TGCN_CHECK(check_ptr(fn, "layout_host", layout_host));
    std::memcpy(&h, layout_host, sizeof(GHeader));
    if (h.magic != kGMagic) {
        set_error("%s: layout_host is not a blob of tgcn_mlp_grouped_layout", fn);
        return TGCN_E_INVALID;
    }
    if (h.N != N || h.k != k) {
        set_error("%s: the layout was built for N=%lld, k=%lld, the call has N=%lld, k=%d", fn, (long long)h.N, (long long)h.k,
                  (long long)N, k);
        return TGCN_E_INVALID;
    }
    return check_ptr(fn, "layout_dev", layout_dev);
}

size_t layout_bytes(int64_t K, int64_t tiles) {
    return sizeof(GHeader) + sizeof(GGroup) * static_cast<size_t>(K) + (sizeof(GTile) + sizeof(GSlice)) * static_cast<size_t>(tiles);
}

// tiles (= chunks of kWChunk rows) of all segments; -1: K or row_ptr is not valid
int64_t count_tiles(int K, const int64_t *row_ptr) {
    if (K < 1 || K > kMaxGroups || row_ptr == nullptr || row_ptr[0] < 0) return -1;
    int64_t tiles = 0;
    for (int g = 0; g < K; ++g) {
        if (row_ptr[g + 1] < row_ptr[g]) return -1;
        tiles += (row_ptr[g + 1] - row_ptr[g] + 127) / 128;
    }
    return tiles;
}

}  // namespace
}  // namespace tgcn

extern "C" {

size_t tgcn_mlp_grouped_layout_bytes(int K, const int64_t *row_ptr) {
    const int64_t tiles = tgcn::count_tiles(K, row_ptr);
    return tiles < 0 ? 0 : tgcn::layout_bytes(K, tiles);
}

int tgcn_mlp_grouped_layout(int K, const int64_t *row_ptr, const int32_t *w_row0, const int32_t *n, const int32_t *col0,
                            const int32_t *b_off, int64_t N, int k, int64_t w_rows, int64_t c_cols, int64_t b_len, void *out,
                            size_t out_bytes) {
    using namespace tgcn;
    const char *fn = "tgcn_mlp_grouped_layout";
    static_assert(kWChunk == 128, "a tile of the forward table and a chunk of the dW table are both 128 rows");
    if (K < 1 || K > kMaxGroups) {
        set_error("%s: K must be in [1, %d] (K=%d)", fn, kMaxGroups, K);
        return TGCN_E_INVALID;
    }
    TGCN_CHECK(check_ptr(fn, "row_ptr", row_ptr));
    TGCN_CHECK(check_ptr(fn, "w_row0", w_row0));
    TGCN_CHECK(check_ptr(fn, "n", n));
    TGCN_CHECK(check_ptr(fn, "col0", col0));
    TGCN_CHECK(check_ptr(fn, "b_off", b_off));
    TGCN_CHECK(check_ptr(fn, "out", out));
    if (N < 0 || k < 1) {
        set_error("%s: need N >= 0 and k >= 1 (N=%lld, k=%d)", fn, (long long)N, k);
        return TGCN_E_INVALID;
    }
    if (row_ptr[0] < 0) {
        set_error("%s: row_ptr[0] is negative (%lld)", fn, (long long)row_ptr[0]);
        return TGCN_E_INVALID;
    }
    for (int g = 0; g < K; ++g) {
        if (row_ptr[g + 1] < row_ptr[g]) {
            set_error("%s: row_ptr decreases at group %d (%lld after %lld)", fn, g, (long long)row_ptr[g + 1],
                      (long long)row_ptr[g]);
            return TGCN_E_INVALID;
        }
    }
    if (row_ptr[K] > N) {
        set_error("%s: row_ptr[K] (%lld) is past the N = %lld rows", fn, (long long)row_ptr[K], (long long)N);
        return TGCN_E_INVALID;
    }
    int n_max = 0;
    for (int g = 0; g < K; ++g) {
        if (n[g] < 1) {
            set_error("%s: group %d has n = %d result columns, need >= 1", fn, g, n[g]);
            return TGCN_E_INVALID;
        }
        if (w_row0[g] < 0 || int64_t(w_row0[g]) + n[g] > w_rows) {
            set_error("%s: rows [%d, %lld) of W for group %d are outside its %lld rows", fn, w_row0[g],
                      (long long)w_row0[g] + n[g], g, (long long)w_rows);
            return TGCN_E_INVALID;
        }
        if (col0[g] < 0 || int64_t(col0[g]) + n[g] > c_cols) {
            set_error("%s: columns [%d, %lld) of C for group %d are outside its %lld columns", fn, col0[g],
                      (long long)col0[g] + n[g], g, (long long)c_cols);
            return TGCN_E_INVALID;
        }
        if (b_off[g] < 0 || int64_t(b_off[g]) + k > b_len) {
            set_error("%s: entries [%d, %lld) of b for group %d are outside its %lld entries", fn, b_off[g],
                      (long long)b_off[g] + k, g, (long long)b_len);
            return TGCN_E_INVALID;
        }
        n_max = std::max(n_max, n[g]);
    }
    const int64_t tiles = count_tiles(K, row_ptr);
    const size_t need = layout_bytes(K, tiles);
    if (out_bytes < need) {
        set_error("%s: out of %zu bytes, tgcn_mlp_grouped_layout_bytes() asks for %zu", fn, out_bytes, need);
        return TGCN_E_INVALID;
    }
    int64_t slices_flat, cps;
    grad_w_split(tiles * kWChunk, k, kWTarget, slices_flat, cps);
    GHeader h{};
    h.magic = kGMagic;
    h.bytes = static_cast<int64_t>(need);
    h.K = K;
    h.N = N;
    h.k = k;
    h.w_rows = w_rows;
    h.c_cols = c_cols;
    h.b_len = b_len;
    h.n_max = n_max;
    h.n_tiles = tiles;
    h.chunks_per_slice = cps;
    std::memset(out, 0, need);
    char *base = static_cast<char *>(out);
    GGroup *groups = reinterpret_cast<GGroup *>(base + sizeof(GHeader));
    GTile *tt = reinterpret_cast<GTile *>(base + sizeof(GHeader) + sizeof(GGroup) * K);
    int64_t n_tiles = 0, n_slices = 0;
    // first the tiles (the slice table starts behind them), then the slices
    for (int g = 0; g < K; ++g) {
        GGroup &gr = groups[g];
        gr.row0 = row_ptr[g];
        gr.rows = row_ptr[g + 1] - row_ptr[g];
        gr.w_row0 = w_row0[g];
        gr.n = n[g];
        gr.col0 = col0[g];
        gr.b_off = b_off[g];
        gr.tile0 = static_cast<int32_t>(n_tiles);
        for (int64_t r = row_ptr[g]; r < row_ptr[g + 1]; r += 128) {
            GTile &t = tt[n_tiles++];
            t.row0 = r;
            t.group = g;
            t.count = static_cast<int32_t>(std::min<int64_t>(128, row_ptr[g + 1] - r));
        }
        gr.n_tiles = static_cast<int32_t>(n_tiles) - gr.tile0;
    }
    GSlice *ss = reinterpret_cast<GSlice *>(reinterpret_cast<char *>(tt) + sizeof(GTile) * n_tiles);
    const int64_t slice_rows = cps * kWChunk;
    for (int g = 0; g < K; ++g) {
        GGroup &gr = groups[g];
        gr.slice0 = static_cast<int32_t>(n_slices);
        for (int64_t r = row_ptr[g]; r < row_ptr[g + 1]; r += slice_rows) {
            GSlice &sl = ss[n_slices++];
            sl.row0 = r;
            sl.row_end = std::min(r + slice_rows, row_ptr[g + 1]);
            sl.group = g;
        }
        gr.n_slices = static_cast<int32_t>(n_slices) - gr.slice0;
    }
    h.n_slices = n_slices;
    std::memcpy(out, &h, sizeof(GHeader));
    return TGCN_OK;
}

int tgcn_mlp_grouped_act_linear(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *c,
                                float *C, int64_t ldc, int64_t N, int k, const void *layout_host, const void *layout_dev,
                                double p, const uint64_t *seed, int64_t mask_row0, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_mlp_grouped_act_linear";
    GHeader h;
    TGCN_CHECK(read_header(fn, layout_host, layout_dev, N, k, h));
    RowDrop d{};
    bool drop = false;
    TGCN_CHECK(make_row_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_CHECK(check_ld(fn, "ldz", ldz, k));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, k));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, h.c_cols));
    if (h.n_tiles == 0) return TGCN_OK;        // no routed row: nothing is written
    TGCN_CHECK(check_ptr(fn, "Z", Z));
    TGCN_CHECK(check_ptr(fn, "b", b));
    TGCN_CHECK(check_ptr(fn, "W", W));
    TGCN_CHECK(check_ptr(fn, "C", C));
    const GTables t = tables_of(layout_dev, h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return drop ? launch_gfwd<true>(h, t, Z, ldz, b, W, ldw, c, C, ldc, d, s)
                : launch_gfwd<false>(h, t, Z, ldz, b, W, ldw, c, C, ldc, d, s);
}

size_t tgcn_mlp_grouped_act_linear_grad_workspace_bytes(const void *layout_host) {
    using namespace tgcn;
    if (!layout_host) return 0;
    GHeader h;
    std::memcpy(&h, layout_host, sizeof(GHeader));
    if (h.magic != kGMagic) return 0;
    return (gdb_floats(h) + gdw_floats(h)) * sizeof(float);
}

int tgcn_mlp_grouped_act_linear_grad(const float *Z, int64_t ldz, const float *b, const float *W, int64_t ldw, const float *G,
                                     int64_t ldg, float *dZ, int64_t lddz, float *db, float *dW, int64_t lddw, float *dc,
                                     int64_t N, int k, const void *layout_host, const void *layout_dev, double p, const uint64_t *seed,
                                     int64_t mask_row0, void *workspace, size_t workspace_bytes, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_mlp_grouped_act_linear_grad";
    GHeader h;
    TGCN_CHECK(read_header(fn, layout_host, layout_dev, N, k, h));
    RowDrop d{};
    bool drop = false;
    TGCN_CHECK(make_row_drop(fn, p, seed, mask_row0, d, drop));
    TGCN_CHECK(check_ld(fn, "ldz", ldz, k));
    TGCN_CHECK(check_ld(fn, "ldw", ldw, k));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, h.c_cols));
    if (dZ) TGCN_CHECK(check_ld(fn, "lddz", lddz, k));
    if (dW) TGCN_CHECK(check_ld(fn, "lddw", lddw, k));
    if ((dZ == nullptr) != (db == nullptr) && !(h.n_tiles == 0 && db != nullptr)) {   // (no routed row: dZ has no element)
        set_error("%s: dZ and db are computed together: pass both or neither (db is the column sum of dZ)", fn);
        return TGCN_E_INVALID;
    }
    if (!db && !dW && !dc) {
        set_error("%s: dZ (with db), dW and dc are all NULL: nothing to compute", fn);
        return TGCN_E_INVALID;
    }
    if (h.n_tiles > 0) {
        TGCN_CHECK(check_ptr(fn, "Z", Z));
        TGCN_CHECK(check_ptr(fn, "b", b));
        TGCN_CHECK(check_ptr(fn, "W", W));
        TGCN_CHECK(check_ptr(fn, "G", G));
    }
    const size_t need = tgcn_mlp_grouped_act_linear_grad_workspace_bytes(layout_host);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace of %zu bytes, tgcn_mlp_grouped_act_linear_grad_workspace_bytes() asks for %zu", fn,
                  workspace ? workspace_bytes : size_t(0), need);
        return TGCN_E_INVALID;
    }
    const GTables t = tables_of(layout_dev, h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part_b = static_cast<float *>(workspace);
    float *part_w = part_b + gdb_floats(h);
    if (dc) TGCN_CHECK(launch_gcolsum<true>(h, t, G, ldg, static_cast<int>(h.c_cols), dc, part_b, s));
    if (db) {
        if (h.n_tiles > 0)
            TGCN_CHECK(drop ? launch_ggrad_z<true>(h, t, Z, ldz, b, W, ldw, G, ldg, dZ, lddz, d, s)
                            : launch_ggrad_z<false>(h, t, Z, ldz, b, W, ldw, G, ldg, dZ, lddz, d, s));
        TGCN_CHECK(launch_gcolsum<false>(h, t, dZ, lddz, k, db, part_b, s));
    }
    if (dW) {
        TGCN_CHECK(drop ? launch_ggrad_w<true>(h, t, Z, ldz, b, G, ldg, dW, lddw, d, part_w, s)
                        : launch_ggrad_w<false>(h, t, Z, ldz, b, G, ldg, dW, lddw, d, part_w, s));
    }
    return TGCN_OK;
}

}  // extern "C"
