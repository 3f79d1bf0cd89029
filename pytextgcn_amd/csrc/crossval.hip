// One cell of the reference's hyper-parameter sweeps (old/h_o_train.py and its siblings: len(lrs) x KFold(k) two-layer GCNs
// on ONE graph) trained as one network of K equal-width members (pytextgcn_amd/crossval.py).  The network side is
// PerLabelGCN's; the two kernels here are what a sweep cell needs beyond it.
//
//   k_member_ce      masked CrossEntropyLoss('mean') of K members in one pass.  Member k owns the columns
//                    [k * S, k * S + C) of the logits (S = seg_stride >= C, the columns behind C are pad) and selects row r
//                    where bit k of bits[r] is set: in cross-validation a document is a training row of k - 1 members and a
//                    validation row of the remaining one, so EVERY row meets EVERY segment (tgcn_grouped_ce trains a row on
//                    the segment of its one group).  The members are uniform, so the logits are N * K "virtual rows" of C
//                    columns: the row body of k_masked_ce (ce_rows of masked_ce.h, the one text both kernels run) under the
//                    view MemberRows with blockIdx.y = member -- base offset k * S, mask = bit k, divisor inv_count[k], one
//                    partial slot per (workgroup, member), pad columns [C, S).
//   k_adam_members   tgcn_adam_step on a [n_rows, K * member_width] tensor whose column block k takes the rate lr[k]: the
//                    members are column blocks of shared tensors and Adam is elementwise, so block k after a step is bit for
//                    bit what tgcn_adam_step with lr[k] gives on a contiguous copy of it: k_adam's sweep (adam_sweep of adam.h)
//                    under a rate policy that looks the step size up by column block.
//   k_adam_member_rows  the same with the members as contiguous ROW blocks of a flat tensor (the stacked tensors of a
//                    CrossValEGCN), every index 64-bit: such a tensor passes 2^31 elements.
// All are deterministic (fixed-order two-stage reductions, no atomics) and only enqueue on the caller's stream.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "adam.h"
#include "common.h"
#include "masked_ce.h"

namespace tgcn {
namespace {

constexpr int kMceBlocks = 2048;       // workgroups of one launch, shared by the members: gridDim.x <= mce_cap(K)
constexpr int kMceMinBlocks = 32;
constexpr int kMaxMembers = kMaxRates;        // one bit of bits[r] per member, one step size per member (adam.h)

int mce_cap(int K) { return std::max(kMceMinBlocks, kMceBlocks / K); }

struct MceArgs {
    const float *logits;
    int64_t ld;
    int C;                      // classes of a member
    int S;                      // columns from one member's segment to the next
    int K;
    const int64_t *target;
    const uint64_t *bits;
    const float *inv_counts;    // [K]
    int64_t n_rows;
    float *dlogits;
    int64_t ldd;
    float *partial;             // [K][gridDim.x]
    int32_t *pred;              // [n_rows][K]
    float *colpart;             // [gridDim.x][K][C] or nullptr
};

// Member blockIdx.y of the launch as the rows of ce_rows (masked_ce.h): its segment of every row, its bit, its divisor,
// its slots.  kPadded: the workgroup writes the zeros of its member's pad columns [C, S) itself, and with V4 (S, ld, ldd
// multiples of 4, 16-byte aligned bases -- whatever C is) reads and writes 16 bytes at a time up to the stride.
struct MemberRows : MceArgs {
    static constexpr bool kPadded = true;
    const int member;
    const int64_t base;         // first column of the member's segment
    const float inv_count;
    __device__ explicit MemberRows(const MceArgs &a)
        : MceArgs(a), member(blockIdx.y), base(int64_t(member) * a.S), inv_count(a.inv_counts[member]) {}
    __device__ int width() const { return S; }
    __device__ bool selected(int64_t r) const { return ((bits[r] >> member) & 1) != 0; }
    __device__ const float *row(int64_t r) const { return logits + r * ld + base; }
    __device__ float *drow(int64_t r) const { return dlogits + r * ldd + base; }
    __device__ bool want_pred() const { return pred != nullptr; }
    __device__ void set_pred(int64_t r, int c) const { pred[r * K + member] = c; }
    __device__ float *partial_slot() const { return partial + int64_t(member) * gridDim.x + blockIdx.x; }
    __device__ float *colpart_row() const { return colpart + (int64_t(blockIdx.x) * K + member) * C; }
};

template <int LPR, bool V4, int KPL = 4>
__global__ __launch_bounds__(256) void k_member_ce(const MceArgs a) {
    ce_rows<LPR, V4, KPL>(MemberRows(a));
}

// Members wider than 256 classes: the column sums of the gradient take a pass of their own over the member's segment,
// into the same partial rows the register path leaves.  Thread t owns the columns t, t + 256, ...
__global__ __launch_bounds__(256) void k_member_colsum_wide(const float *__restrict__ d, int64_t ldd, int64_t n_rows, int C,
                                                            int S, int K, float *__restrict__ colpart) {
    const int member = blockIdx.y;
    float *out = colpart + (int64_t(blockIdx.x) * K + member) * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float *p = d + int64_t(member) * S + c;
        float s = 0.f;
        for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) s += p[r * ldd];
        out[c] = s;
    }
}

// dbias[k * S + c] = the sum of the partial rows in a fixed order (k_colsum_final's: 16 waves take every 16th row, then the
// 16 sums in wave order), exactly 0 in the pad columns
__global__ __launch_bounds__(1024) void k_member_colsum_final(const float *__restrict__ colpart, int nb, int C, int S, int K,
                                                              float *__restrict__ dbias) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = blockIdx.x * 64 + lane;
    const int member = f / S, c = f % S;
    const bool live = f < K * S && c < C;
    float s = 0.f;
    if (live) {
        const float *p = colpart + int64_t(member) * C + c;
        const int64_t ldp = int64_t(K) * C;
        for (int b = wave; b < nb; b += 16) s += p[b * ldp];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && f < K * S) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += red[w][lane];
        dbias[f] = live ? t : 0.f;
    }
}

// loss_k[k] = inv_count[k] * sum of the member's workgroup partials (NaN for a member without a selected row: torch's mean
// over nothing), loss = the sum of the others, member by member in index order
__global__ __launch_bounds__(256) void k_member_ce_final(const float *__restrict__ partial, int n_part, int K,
                                                         const float *__restrict__ inv_count, float *__restrict__ loss,
                                                         float *__restrict__ loss_k) {
    __shared__ float red[256];
    float total = 0.f;                                // (thread 0's copy is the one that is stored)
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
        for (int i = threadIdx.x; i < n_part; i += 256) s += partial[int64_t(k) * n_part + i];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (static_cast<int>(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float ic = inv_count[k];
            const float mean = red[0] * ic;
            if (ic != 0.f) total += mean;
            if (loss_k != nullptr) loss_k[k] = ic != 0.f ? mean : NAN;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = total;
}

// ---- Adam with one learning rate per member: the sweep of adam.h under a rate policy --------------------------------
// The members as COLUMN blocks of a [n_rows, n_cols] tensor (ColumnBlockRates: V4, IDX32).
template <bool AMSGRAD, bool NT, bool V4, bool IDX32>
__global__ __launch_bounds__(256) void k_adam_members(float *__restrict__ p, const float *__restrict__ g,
                                                      float *__restrict__ m, float *__restrict__ v,
                                                      float *__restrict__ vmax, int64_t n, uint32_t n_cols, uint32_t width,
                                                      int K, float w1 /* 1-b1 */, float b2, float w2 /* 1-b2 */, float eps,
                                                      float wd, const AdamRates host, float inv_bc2_sqrt,
                                                      const float *__restrict__ dev_scalars) {
    const float *rate = member_rate_table(host, K, dev_scalars, inv_bc2_sqrt);
    adam_sweep<AMSGRAD, NT>(p, g, m, v, vmax, n, AdamCoef{w1, b2, w2, eps, wd, inv_bc2_sqrt},
                            ColumnBlockRates<V4, IDX32>{rate, n_cols, width});
}

// The members as ROW blocks (the stacked embedding weight [M D, in] of a CrossValEGCN): a flat tensor of n = K * block
// elements (RowBlockRates: V4).
template <bool AMSGRAD, bool NT, bool V4>
__global__ __launch_bounds__(256) void k_adam_member_rows(float *__restrict__ p, const float *__restrict__ g,
                                                          float *__restrict__ m, float *__restrict__ v,
                                                          float *__restrict__ vmax, int64_t n, int64_t block, int K,
                                                          float w1 /* 1-b1 */, float b2, float w2 /* 1-b2 */, float eps,
                                                          float wd, const AdamRates host, float inv_bc2_sqrt,
                                                          const float *__restrict__ dev_scalars) {
    const float *rate = member_rate_table(host, K, dev_scalars, inv_bc2_sqrt);
    adam_sweep<AMSGRAD, NT>(p, g, m, v, vmax, n, AdamCoef{w1, b2, w2, eps, wd, inv_bc2_sqrt}, RowBlockRates<V4>{rate, block});
}

}  // namespace
}  // namespace tgcn

extern "C" {

size_t tgcn_member_ce_workspace_bytes(int64_t n_rows, int n_members, int n_classes) {
    if (n_rows < 0 || n_members < 1 || n_members > tgcn::kMaxMembers || n_classes < 1) return 0;
    // per (workgroup, member): one loss partial and one row of C column sums
    return sizeof(float) * static_cast<size_t>(tgcn::mce_cap(n_members)) * static_cast<size_t>(n_members) *
           (static_cast<size_t>(n_classes) + 1);
}

int tgcn_member_ce(const float *logits, int64_t ld, int64_t n_rows, int n_members, int n_classes, int seg_stride,
                   const int64_t *target, const uint64_t *bits, const float *inv_count, float *loss, float *loss_k,
                   float *dlogits, int64_t ldd, float *dbias, int32_t *pred, void *workspace, size_t workspace_bytes,
                   tgcn_stream stream) {
    using namespace tgcn;
    const char *who = "tgcn_member_ce";
    const int K = n_members, C = n_classes, S = seg_stride;
    if (K < 1 || K > kMaxMembers || C < 1) {
        set_error("%s: n_members=%d must lie in 1..%d and n_classes=%d must be >= 1", who, K, kMaxMembers, C);
        return TGCN_E_INVALID;
    }
    if (S < C) {
        set_error("%s: seg_stride=%d is less than n_classes=%d", who, S, C);
        return TGCN_E_INVALID;
    }
    const int64_t n_cols = int64_t(K) * S;
    if (ld < n_cols || (dlogits && ldd < n_cols)) {
        set_error("%s: ld=%lld / ldd=%lld is less than n_members * seg_stride = %lld", who, (long long)ld, (long long)ldd,
                  (long long)n_cols);
        return TGCN_E_INVALID;
    }
    if (dbias && !dlogits) {
        set_error("%s: dbias is the column sums of dlogits: it needs dlogits", who);
        return TGCN_E_INVALID;
    }
    // (an empty matrix may come with NULL row arrays: torch hands out no storage for zero rows)
    if (n_rows < 0 || n_cols > INT32_MAX || !inv_count || !loss || (n_rows > 0 && (!logits || !target || !bits))) {
        set_error("%s: bad argument (n_rows=%lld, NULL logits / target / bits / inv_count / loss, or more than 2^31 columns)",
                  who, (long long)n_rows);
        return TGCN_E_INVALID;
    }
    const size_t need = tgcn_member_ce_workspace_bytes(n_rows, K, C);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes given, %zu needed", who, workspace_bytes, need);
        return TGCN_E_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cap = mce_cap(K);
    float *partial = static_cast<float *>(workspace);
    float *colws = partial + static_cast<size_t>(cap) * K;
    const bool regs = C <= 256;
    const bool v4 = ce_v4(S, logits, ld, dlogits, ldd);
    MceArgs a{logits, ld, C, S, K, target, bits, inv_count, n_rows, dlogits, ldd, partial, pred,
              (dbias && regs) ? colws : nullptr};
    int gx = 0;
    // lanes per row and logits per lane by class count: the leaves of masked_ce_impl (train.hip), one grid column per member
    ce_dispatch(C, v4, [&](auto lpr, auto kpl, auto vec) {
        gx = ce_grid(n_rows, lpr, cap);
        k_member_ce<lpr, vec, kpl><<<dim3(gx, K), 256, 0, s>>>(a);
    });
    TGCN_HIP_CHECK(hipGetLastError());
    k_member_ce_final<<<1, 256, 0, s>>>(partial, gx, K, inv_count, loss, loss_k);
    TGCN_HIP_CHECK(hipGetLastError());
    if (dbias) {
        int nb = gx;
        if (!regs) {
            nb = std::min(cap, colsum_blocks(n_rows));
            k_member_colsum_wide<<<dim3(nb, K), 256, 0, s>>>(dlogits, ldd, n_rows, C, S, K, colws);
            TGCN_HIP_CHECK(hipGetLastError());
        }
        k_member_colsum_final<<<static_cast<int>((n_cols + 63) / 64), 1024, 0, s>>>(colws, nb, C, S, K, dbias);
        TGCN_HIP_CHECK(hipGetLastError());
    }
    return TGCN_OK;
}

static int adam_members_impl(const char *who, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                             float *max_exp_avg_sq, int64_t n_rows, int64_t n_cols, int member_width, int n_members,
                             const double *lr_host, double beta1, double beta2, double eps, double weight_decay,
                             int64_t step, int64_t *step_dev, float *scalars_dev, tgcn_stream stream) {
    using namespace tgcn;
    const int K = n_members;
    if (K < 1 || K > kMaxMembers || !lr_host || n_rows < 0 || n_cols < 0 || member_width < 0 ||
        n_cols != int64_t(K) * member_width || n_cols > INT32_MAX || step < 1) {
        set_error("%s: bad argument (n_rows=%lld n_cols=%lld must be n_members=%d (1..%d) * member_width=%d; lr_host=%s "
                  "step=%lld)", who, (long long)n_rows, (long long)n_cols, K, kMaxMembers, member_width,
                  lr_host ? "given" : "NULL", (long long)step);
        return TGCN_E_INVALID;
    }
    if (n_rows > 0 && n_cols > INT64_MAX / n_rows) {
        set_error("%s: n_rows * n_cols overflows", who);
        return TGCN_E_INVALID;
    }
    const int64_t n = n_rows * n_cols;
    if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) {
        set_error("%s: NULL param / grad / exp_avg / exp_avg_sq", who);
        return TGCN_E_INVALID;
    }
    if (n > 0 && !adam_aligned(who, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq)) return TGCN_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool v4 = member_width % 4 == 0 && n_cols % 4 == 0;
    const bool i32 = n <= INT32_MAX;
    const uint32_t nc = static_cast<uint32_t>(n_cols), mw = static_cast<uint32_t>(member_width);
    return adam_launch(n, max_exp_avg_sq != nullptr, lr_host, K, beta1, beta2, eps, weight_decay, step, step_dev, scalars_dev, s,
                       [&](auto ams, auto nt, const AdamLaunch &a) {
                           auto go = [&](auto vec, auto idx32) {
                               k_adam_members<ams, nt, vec, idx32><<<a.grid, 256, 0, s>>>(
                                   param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, nc, mw, K, a.c.w1, a.c.b2, a.c.w2,
                                   a.c.eps, a.c.wd, a.rates, a.c.inv_bc2_sqrt, scalars_dev);
                           };
                           if (v4 && i32)
                               go(std::true_type{}, std::true_type{});
                           else if (v4)
                               go(std::true_type{}, std::false_type{});
                           else if (i32)
                               go(std::false_type{}, std::true_type{});
                           else
                               go(std::false_type{}, std::false_type{});
                       });
}

int tgcn_adam_members(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                      int64_t n_rows, int64_t n_cols, int member_width, int n_members, const double *lr_host, double beta1,
                      double beta2, double eps, double weight_decay, int64_t step, tgcn_stream stream) {
    return adam_members_impl("tgcn_adam_members", param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n_rows, n_cols,
                             member_width, n_members, lr_host, beta1, beta2, eps, weight_decay, step, nullptr, nullptr,
                             stream);
}

int tgcn_adam_members_capturable(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                                 int64_t n_rows, int64_t n_cols, int member_width, int n_members, const double *lr_host,
                                 double beta1, double beta2, double eps, double weight_decay, int64_t *step_dev,
                                 float *scalars_dev, tgcn_stream stream) {
    if (!step_dev || !scalars_dev) {
        tgcn::set_error("tgcn_adam_members_capturable: step_dev / scalars_dev must be device pointers");
        return TGCN_E_INVALID;
    }
    return adam_members_impl("tgcn_adam_members_capturable", param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n_rows,
                             n_cols, member_width, n_members, lr_host, beta1, beta2, eps, weight_decay, 1, step_dev,
                             scalars_dev, stream);
}

static int adam_member_rows_impl(const char *who, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                 float *max_exp_avg_sq, int64_t n, int64_t block, int n_members, const double *lr_host,
                                 double beta1, double beta2, double eps, double weight_decay, int64_t step, int64_t *step_dev,
                                 float *scalars_dev, tgcn_stream stream) {
    using namespace tgcn;
    const int K = n_members;
    if (K < 1 || K > kMaxMembers || !lr_host || n < 0 || block < 0 || block > INT64_MAX / K || n != int64_t(K) * block ||
        step < 1) {
        set_error("%s: bad argument (n=%lld must be n_members=%d (1..%d) * block=%lld; lr_host=%s step=%lld)", who,
                  (long long)n, K, kMaxMembers, (long long)block, lr_host ? "given" : "NULL", (long long)step);
        return TGCN_E_INVALID;
    }
    if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) {
        set_error("%s: NULL param / grad / exp_avg / exp_avg_sq", who);
        return TGCN_E_INVALID;
    }
    if (n > 0 && !adam_aligned(who, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq)) return TGCN_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return adam_launch(n, max_exp_avg_sq != nullptr, lr_host, K, beta1, beta2, eps, weight_decay, step, step_dev, scalars_dev, s,
                       [&](auto ams, auto nt, const AdamLaunch &a) {
                           auto go = [&](auto vec) {
                               k_adam_member_rows<ams, nt, vec><<<a.grid, 256, 0, s>>>(
                                   param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, block, K, a.c.w1, a.c.b2, a.c.w2,
                                   a.c.eps, a.c.wd, a.rates, a.c.inv_bc2_sqrt, scalars_dev);
                           };
                           if (block % 4 == 0)
                               go(std::true_type{});
                           else
                               go(std::false_type{});
                       });
}

int tgcn_adam_member_rows(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq,
                          int64_t n, int64_t block, int n_members, const double *lr_host, double beta1, double beta2,
                          double eps, double weight_decay, int64_t step, tgcn_stream stream) {
    return adam_member_rows_impl("tgcn_adam_member_rows", param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, block,
                                 n_members, lr_host, beta1, beta2, eps, weight_decay, step, nullptr, nullptr, stream);
}

int tgcn_adam_member_rows_capturable(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                     float *max_exp_avg_sq, int64_t n, int64_t block, int n_members, const double *lr_host,
                                     double beta1, double beta2, double eps, double weight_decay, int64_t *step_dev,
                                     float *scalars_dev, tgcn_stream stream) {
    if (!step_dev || !scalars_dev) {
        tgcn::set_error("tgcn_adam_member_rows_capturable: step_dev / scalars_dev must be device pointers");
        return TGCN_E_INVALID;
    }
    return adam_member_rows_impl("tgcn_adam_member_rows_capturable", param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n,
                                 block, n_members, lr_host, beta1, beta2, eps, weight_decay, 1, step_dev, scalars_dev, stream);
}

}  // extern "C"
