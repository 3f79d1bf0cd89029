// Device-side scores of the K-member networks (pytextgcn_amd/metrics.py): what the reference computes per member on the
// host with sklearn's f1_score(average="macro") and accuracy_score (old/h_o_train.py:116-122) from three numbers per
// class -- tp[c], n_pred[c], n_true[c] -- instead of a C x C confusion matrix.
//
//   k_class_counts<MEMBERS>   counts [K][3][C] (planes tp, n_pred, n_true) of up to two row sets in one pass over the
//                    predictions.  Workgroup (x, y, z) owns the row tiles x, x + gridDim.x, ... (kRows rows each), the
//                    members [y * kt, (y + 1) * kt) and, when both sets do not fit the LDS budget side by side, the set z.
//                    It counts with LDS integer adds into a zeroed table and stores the table to its own slice of the
//                    workspace: no global atomics, nothing shared between workgroups.
//                      MEMBERS = true   pred int32 [n_rows, K]; row r counts for member k of set s where bit k of
//                                       bits_s[r] is set (tgcn_member_ce's selection and prediction)
//                      MEMBERS = false  pred int64 [n_rows]; row r belongs to member group[r] (-1: none; no group array:
//                                       member 0), its class is pred[r] - pred_offset[group[r]], set s takes it where
//                                       mask_s[r] != 0 (tgcn_grouped_ce's prediction; the flat network without groups)
//                    The target is compared with [0, C) BEFORE it is used as an index (a row outside counts nowhere: the
//                    Python side raises for it before the launch); a prediction outside [0, C) counts in n_true only.
//   k_class_counts_final      counts_s[j] = sum over the workgroups' partial tables, in workgroup order; writes every entry.
//   k_class_scores            per member: accuracy, macro-F1 (sklearn's: the mean of 2 tp / (n_pred + n_true) over the
//                    classes with n_pred + n_true > 0), rows, labels -- in double, fixed-order tree reduction.
// Everything only enqueues on the caller's stream.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace tgcn {
namespace {

constexpr int kRows = TGCN_CLASS_COUNTS_ROWS_PER_WORKGROUP;    // rows of one tile
constexpr int kCap = TGCN_CLASS_COUNTS_WORKGROUP_CAP;          // gridDim.x at most
constexpr int kLdsBytes = TGCN_CLASS_COUNTS_LDS_BYTES;         // LDS table of a workgroup at most
constexpr int64_t kPartialBytes = TGCN_CLASS_COUNTS_PARTIAL_BYTES;   // the workgroups' partial tables together at most
constexpr int kMaxClasses = TGCN_CLASS_COUNTS_MAX_CLASSES;
constexpr int kMaxMembers = 64;
static_assert(kRows == 256, "k_class_counts walks a tile with one 256-thread workgroup");
static_assert(3 * kMaxClasses * 4 <= kLdsBytes && kLdsBytes <= 64 * 1024, "one member's table of one set fits the budget");

struct Tiling {
    int sets_per_wg;    // 2: a workgroup counts both sets; 1: one set (gridDim.z walks the sets)
    int kt;             // members per workgroup
    int n_ktiles;       // gridDim.y
    int gx;             // gridDim.x: row-tile walkers = partial tables per (member, set)
};

int row_walkers(int64_t n_rows, int K, int C) {
    const int64_t tiles = (n_rows + kRows - 1) / kRows;
    const int64_t per_wg = int64_t(2) * K * 3 * C * 4;          // both sets of every member
    const int64_t by_ws = std::max<int64_t>(1, kPartialBytes / per_wg);
    return static_cast<int>(std::min<int64_t>(std::min<int64_t>(kCap, tiles), by_ws));
}

Tiling tiling(int64_t n_rows, int K, int C, bool two_sets) {
    Tiling t;
    const int per_member = 3 * C * 4;
    t.sets_per_wg = (two_sets && 2 * per_member <= kLdsBytes) ? 2 : 1;
    t.kt = std::min(K, std::max(1, kLdsBytes / (t.sets_per_wg * per_member)));
    t.n_ktiles = (K + t.kt - 1) / t.kt;
    t.gx = row_walkers(n_rows, K, C);
    return t;
}

struct CountArgs {
    const void *pred;             // MEMBERS: int32 [n_rows][ldp]; else int64 [n_rows]
    int64_t ldp;
    const int64_t *target;
    const uint64_t *bits_a, *bits_b;   // MEMBERS
    const int32_t *pred_offset;   // groups form, [K] or nullptr
    const int32_t *group;         // groups form, [n_rows] or nullptr
    const uint8_t *mask_a, *mask_b;    // groups form
    int64_t n_rows;
    int K, C, kt, sets_per_wg;
    int32_t *partial;             // [gridDim.x][2][K][3][C]
};

template <bool MEMBERS>
__global__ __launch_bounds__(256) void k_class_counts(const CountArgs a) {
    extern __shared__ int32_t table[];            // [sets of this workgroup][kt][3][C]
    const int C = a.C, K = a.K, plane = 3 * a.C;
    const int k0 = blockIdx.y * a.kt;
    const int kt = min(a.kt, K - k0);
    const int nsets = a.sets_per_wg;
    const int set0 = nsets == 2 ? 0 : static_cast<int>(blockIdx.z);
    const int n_slots = nsets * kt * plane;
    // the first (and, with both sets in one workgroup, the second) set of this workgroup: table slots 0 and 1
    const bool second = nsets == 1 && set0 == 1;
    const uint64_t *bits0 = second ? a.bits_b : a.bits_a, *bits1 = nsets == 2 ? a.bits_b : nullptr;
    const uint8_t *mask0 = second ? a.mask_b : a.mask_a, *mask1 = nsets == 2 ? a.mask_b : nullptr;
    for (int i = threadIdx.x; i < n_slots; i += 256) table[i] = 0;
    __syncthreads();
    auto count = [&](int s, int kl, int64_t t, int64_t p) {
        int32_t *base = table + (s * kt + kl) * plane;
        atomicAdd(&base[2 * C + static_cast<int>(t)], 1);
        if (p >= 0 && p < C) {
            atomicAdd(&base[C + static_cast<int>(p)], 1);
            if (p == t) atomicAdd(&base[static_cast<int>(t)], 1);
        }
    };
    const int64_t n_tiles = (a.n_rows + kRows - 1) / kRows;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kRows;
        const int rows_here = static_cast<int>(min(int64_t(kRows), a.n_rows - row0));
        if constexpr (MEMBERS) {
            const int32_t *pred = static_cast<const int32_t *>(a.pred);
            const int n_el = rows_here * kt;            // (row, member) pairs, the member fastest: pred is read in row order
            for (int e = threadIdx.x; e < n_el; e += 256) {
                const int rl = e / kt, kl = e - rl * kt;
                const int64_t r = row0 + rl;
                const int k = k0 + kl;
                const bool on0 = ((bits0[r] >> k) & 1) != 0;
                const bool on1 = bits1 != nullptr && ((bits1[r] >> k) & 1) != 0;
                if (!(on0 || on1)) continue;
                const int64_t t = a.target[r];
                if (t < 0 || t >= C) continue;          // never an index
                const int64_t p = pred[r * a.ldp + k];
                if (on0) count(0, kl, t, p);
                if (on1) count(1, kl, t, p);
            }
        } else {
            const int64_t *pred = static_cast<const int64_t *>(a.pred);
            for (int rl = threadIdx.x; rl < rows_here; rl += 256) {
                const int64_t r = row0 + rl;
                const int g = a.group != nullptr ? a.group[r] : 0;
                if (g < k0 || g >= k0 + kt) continue;    // (-1, another tile's member, or no member at all)
                const bool on0 = mask0[r] != 0;
                const bool on1 = mask1 != nullptr && mask1[r] != 0;
                if (!(on0 || on1)) continue;
                const int64_t t = a.target[r];
                if (t < 0 || t >= C) continue;
                const int64_t p = pred[r] - (a.pred_offset != nullptr ? a.pred_offset[g] : 0);
                if (on0) count(0, g - k0, t, p);
                if (on1) count(1, g - k0, t, p);
            }
        }
    }
    __syncthreads();
    for (int s = 0; s < nsets; ++s) {
        int32_t *dst = a.partial + ((int64_t(blockIdx.x) * 2 + (set0 + s)) * K + k0) * plane;
        const int32_t *src = table + s * kt * plane;
        for (int i = threadIdx.x; i < kt * plane; i += 256) dst[i] = src[i];
    }
}

__global__ __launch_bounds__(256) void k_class_counts_final(const int32_t *__restrict__ partial, int nb, int per_set,
                                                            int n_sets, int32_t *__restrict__ counts_a,
                                                            int32_t *__restrict__ counts_b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sets * per_set) return;
    const int set = i / per_set, j = i - set * per_set;
    int32_t s = 0;
    for (int b = 0; b < nb; ++b) s += partial[(int64_t(b) * 2 + set) * per_set + j];
    (set ? counts_b : counts_a)[j] = s;
}

__global__ __launch_bounds__(256) void k_class_scores(const int32_t *__restrict__ counts, int C, double *__restrict__ scores) {
    __shared__ double red_f[256];
    __shared__ long long red_tp[256], red_nt[256];
    __shared__ int red_l[256];
    const int32_t *tp = counts + int64_t(blockIdx.x) * 3 * C, *np = tp + C, *nt = np + C;
    double f = 0.0;
    long long s_tp = 0, s_nt = 0;
    int labels = 0;
    for (int c = threadIdx.x; c < C; c += 256) {
        const long long den = static_cast<long long>(np[c]) + nt[c];
        if (den > 0) {
            ++labels;
            f += 2.0 * static_cast<double>(tp[c]) / static_cast<double>(den);
        }
        s_tp += tp[c];
        s_nt += nt[c];
    }
    red_f[threadIdx.x] = f;
    red_tp[threadIdx.x] = s_tp;
    red_nt[threadIdx.x] = s_nt;
    red_l[threadIdx.x] = labels;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) {
            red_f[threadIdx.x] += red_f[threadIdx.x + off];
            red_tp[threadIdx.x] += red_tp[threadIdx.x + off];
            red_nt[threadIdx.x] += red_nt[threadIdx.x + off];
            red_l[threadIdx.x] += red_l[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *out = scores + int64_t(blockIdx.x) * 4;
        out[0] = red_nt[0] > 0 ? static_cast<double>(red_tp[0]) / static_cast<double>(red_nt[0]) : NAN;
        out[1] = red_l[0] > 0 ? red_f[0] / static_cast<double>(red_l[0]) : NAN;
        out[2] = static_cast<double>(red_nt[0]);
        out[3] = static_cast<double>(red_l[0]);
    }
}

bool sizes_ok(const char *who, int64_t n_rows, int K, int C) {
    if (K < 1 || K > kMaxMembers || C < 1 || C > kMaxClasses || n_rows < 0 || n_rows > INT32_MAX) {
        set_error("%s: n_members=%d must lie in 1..%d, n_classes=%d in 1..%d and n_rows=%lld in 0..2^31-1", who, K,
                  kMaxMembers, C, kMaxClasses, (long long)n_rows);
        return false;
    }
    return true;
}

template <bool MEMBERS>
int launch_counts(const char *who, CountArgs a, int32_t *counts_a, int32_t *counts_b, void *workspace,
                  size_t workspace_bytes, hipStream_t s) {
    const int K = a.K, C = a.C;
    const size_t need = tgcn_class_counts_workspace_bytes(a.n_rows, K, C);
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        set_error("%s: workspace of %zu bytes given, %zu needed", who, workspace_bytes, need);
        return TGCN_E_WORKSPACE;
    }
    const bool two = counts_b != nullptr;
    const Tiling t = tiling(a.n_rows, K, C, two);
    a.kt = t.kt;
    a.sets_per_wg = t.sets_per_wg;
    a.partial = static_cast<int32_t *>(workspace);
    if (t.gx > 0) {
        const dim3 grid(t.gx, t.n_ktiles, two && t.sets_per_wg == 1 ? 2 : 1);
        const size_t lds = size_t(t.sets_per_wg) * t.kt * 3 * C * 4;
        k_class_counts<MEMBERS><<<grid, 256, lds, s>>>(a);
        TGCN_HIP_CHECK(hipGetLastError());
    }
    const int per_set = K * 3 * C, n_sets = two ? 2 : 1;
    k_class_counts_final<<<(n_sets * per_set + 255) / 256, 256, 0, s>>>(a.partial, t.gx, per_set, n_sets, counts_a, counts_b);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // namespace
}  // namespace tgcn

extern "C" {

size_t tgcn_class_counts_workspace_bytes(int64_t n_rows, int n_members, int n_classes) {
    using namespace tgcn;
    if (n_rows < 0 || n_rows > INT32_MAX || n_members < 1 || n_members > kMaxMembers || n_classes < 1 ||
        n_classes > kMaxClasses)
        return 0;
    return size_t(row_walkers(n_rows, n_members, n_classes)) * 2 * n_members * 3 * n_classes * sizeof(int32_t);
}

int tgcn_class_counts_members(const int32_t *pred, int64_t ldp, const int64_t *target, const uint64_t *bits_a,
                              const uint64_t *bits_b, int64_t n_rows, int n_members, int n_classes, int32_t *counts_a,
                              int32_t *counts_b, void *workspace, size_t workspace_bytes, tgcn_stream stream) {
    using namespace tgcn;
    const char *who = "tgcn_class_counts_members";
    if (!sizes_ok(who, n_rows, n_members, n_classes)) return TGCN_E_INVALID;
    if (ldp < n_members) {
        set_error("%s: ldp=%lld is less than n_members=%d", who, (long long)ldp, n_members);
        return TGCN_E_INVALID;
    }
    if (!counts_a || (bits_b != nullptr) != (counts_b != nullptr) || (n_rows > 0 && (!pred || !target || !bits_a))) {
        set_error("%s: NULL pred / target / bits_a / counts_a, or one of bits_b and counts_b without the other", who);
        return TGCN_E_INVALID;
    }
    CountArgs a{};
    a.pred = pred;
    a.ldp = ldp;
    a.target = target;
    a.bits_a = bits_a;
    a.bits_b = bits_b;
    a.n_rows = n_rows;
    a.K = n_members;
    a.C = n_classes;
    return launch_counts<true>(who, a, counts_a, counts_b, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int tgcn_class_counts_groups(const int64_t *pred, const int32_t *pred_offset, const int64_t *target, const int32_t *group,
                             const uint8_t *mask_a, const uint8_t *mask_b, int64_t n_rows, int n_members, int n_classes,
                             int32_t *counts_a, int32_t *counts_b, void *workspace, size_t workspace_bytes,
                             tgcn_stream stream) {
    using namespace tgcn;
    const char *who = "tgcn_class_counts_groups";
    if (!sizes_ok(who, n_rows, n_members, n_classes)) return TGCN_E_INVALID;
    if (!counts_a || (mask_b != nullptr) != (counts_b != nullptr) || (n_rows > 0 && (!pred || !target || !mask_a))) {
        set_error("%s: NULL pred / target / mask_a / counts_a, or one of mask_b and counts_b without the other", who);
        return TGCN_E_INVALID;
    }
    CountArgs a{};
    a.pred = pred;
    a.target = target;
    a.pred_offset = pred_offset;
    a.group = group;
    a.mask_a = mask_a;
    a.mask_b = mask_b;
    a.n_rows = n_rows;
    a.K = n_members;
    a.C = n_classes;
    return launch_counts<false>(who, a, counts_a, counts_b, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int tgcn_class_scores(const int32_t *counts, int n_members, int n_classes, double *scores, tgcn_stream stream) {
    using namespace tgcn;
    const char *who = "tgcn_class_scores";
    if (!sizes_ok(who, 0, n_members, n_classes)) return TGCN_E_INVALID;
    if (!counts || !scores) {
        set_error("%s: NULL counts / scores", who);
        return TGCN_E_INVALID;
    }
    k_class_scores<<<n_members, 256, 0, static_cast<hipStream_t>(stream)>>>(counts, n_classes, scores);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // extern "C"
