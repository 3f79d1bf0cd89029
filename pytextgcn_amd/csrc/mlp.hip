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
// The three products themselves -- mlp_fwd, mlp_grad_z and mlp_grad_w, every MFMA of them -- stand in mlp_products.h, which
// mlp_grouped.hip includes too; the kernels say which rows a workgroup owns: rows 128 blockIdx.x ... of the whole operand
// (forward, dZ), or slice blockIdx.y of `chunks_per_slice` chunks of kWChunk rows (dW; that kernel is in the header too).
#include <algorithm>

#include "mlp_products.h"

namespace tgcn {
namespace {

template <int NT, bool DROP, bool CLS>
__global__ __launch_bounds__(256, 2) void k_mlp_fwd(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                    const float *__restrict__ W, int64_t ldw, const float *__restrict__ cb,
                                                    float *__restrict__ C, int64_t ldc, int64_t N, int K, int n,
                                                    const RowDrop d, const ClassTerm ct) {
    mlp_fwd<NT, DROP, CLS>(Z, ldz, b, W, ldw, cb, C, ldc, int64_t(blockIdx.x) * 128, N, K, n, d, ct);
}

template <int NT, bool DROP, bool CLS>
__global__ __launch_bounds__(256, 2) void k_mlp_grad_z(const float *__restrict__ Z, int64_t ldz, const float *__restrict__ b,
                                                       const float *__restrict__ W, int64_t ldw,
                                                       const float *__restrict__ G, int64_t ldg, float *__restrict__ dZ,
                                                       int64_t lddz, int64_t N, int K, int n, int accum, const RowDrop d,
                                                       const ClassTerm ct) {
    mlp_grad_z<NT, DROP, CLS>(Z, ldz, b, W, ldw, G, ldg, dZ, lddz, int64_t(blockIdx.x) * 128, N, K, n, accum, d, ct);
}

// k_mlp_grad_w<TW, DROP, CLS> stands in mlp_products.h, next to mlp_grad_w: with the class term it keeps the row loop in the
// kernel itself.

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

