// Grouped masked cross-entropy: the loss of the per-label strategy (perlabel_amazon.py:90-155) for ALL of its classifiers
// in one pass.
//
// The reference trains one two-layer GCN per top-level label k: it restricts the masks to that label's documents
// (perlabel_amazon.py:130-132), relabels their classes to 0..C_k-1 (:104-109) and takes CrossEntropyLoss('mean') of
// `gcn(g)[train_mask]` (:136-137).  With the K classifiers concatenated along the class axis (pytextgcn_amd/perlabel.py)
// the K losses are one matrix [N, sum C_k] in which row r is trained on the column segment of ITS group only:
//
//   loss_k  = mean over the selected rows r of group k of  lse(logits[r, seg_k]) - logits[r, seg_k.start + target[r]]
//   loss    = sum of loss_k over the groups that have a selected row
//   dlogits = (softmax over seg_k - one-hot) * inv_count[k] inside the row's segment, exactly 0.0f everywhere else
// computed as ce_rows (masked_ce.h) computes the flat loss: with m the segment's maximum, e_c = exp(x_c - m) and `others`
// the sum of the e_c without the target's e_t, a row's term is log(others + e_t) - (x_t - m) and its gradient is
// e_c / sum off the target and -(others / sum) at it -- no `p_t - 1.f`, no `m + log(sum)`, which round a confident row's
// gradient and a large row's loss away (tests/test_gpu_grouped_ce.py).
//   pred[r] = seg_q.start + argmax logits[r, seg_q],  q = route[r]  (eval_perlabel.py:71-78: routed by the top label)
//
// k_grouped_ce (n_cols <= 256): LPR lanes hold one row, each lane four ABSOLUTE columns of it, whatever the row's segment:
// a segment is a predicate on the lane's columns.  So the 16-byte path depends on the buffers (n_cols, ld, ldd multiples of
// 4, aligned bases), not on where the segments start, and the column sums of the gradient (the bias gradient of the layer
// that produced the logits) are taken from the registers that hold the rows, as k_masked_ce does.  Only the 16-byte chunks
// that meet the row's training or routing segment are read.
// k_grouped_ce_wide (wider rows): one wave per row walks the segment; the column sums take a pass of their own.
// Both are deterministic: per-group loss terms meet in LDS slots that one sub-group owns (no atomics), workgroup partials
// are summed in a fixed order by k_grouped_ce_final.  Every launch goes to the caller's stream and nothing else is done,
// so the call is legal under HIP-graph capture.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace tgcn {
namespace {

constexpr int kGceBlocks = 1024;
constexpr int kGceMaxGroups = 128;      // LDS: (4 * 64 / LPR) sub-groups x K floats <= 32 KB

struct GceArgs {
    const float *logits;
    int64_t ld;
    int n_cols;
    int K;
    const int32_t *seg_start;
    const int32_t *seg_width;
    const int32_t *group;
    const int32_t *route;       // nullptr: the group
    const int64_t *target;
    const uint8_t *mask;
    const float *inv_count;
    const int64_t *class_map;   // nullptr: the column itself
    int64_t n_rows;
    float *dlogits;
    int64_t ldd;
    float *part_k;              // [gridDim.x][K]
    int64_t *pred;
    float *colpart;             // [gridDim.x][n_cols] or nullptr
};

// the segment [s0, s1) of group g, empty for "none" and for anything outside [0, K); cut to the row
__device__ __forceinline__ void segment_of(const GceArgs &a, int g, int &s0, int &s1) {
    s0 = s1 = 0;
    if (g >= 0 && g < a.K) {
        s0 = max(0, min(a.seg_start[g], a.n_cols));
        s1 = max(s0, min(s0 + a.seg_width[g], a.n_cols));
    }
}

// the per-sub-group LDS slots [n_sub][K] of the per-group loss terms -> part_k[blockIdx.x][0..K), in a fixed order
__device__ __forceinline__ void flush_group_terms(const volatile float *lk, int n_sub, int K, float *part_k) {
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float s = 0.f;
        for (int i = 0; i < n_sub; ++i) s += lk[i * K + k];
        part_k[int64_t(blockIdx.x) * K + k] = s;
    }
}

template <int LPR, bool V4>
__global__ __launch_bounds__(256) void k_grouped_ce(const GceArgs a) {
    constexpr int KPL = 4, RPW = 64 / LPR, UN = 2;
    extern __shared__ float lk_raw[];                 // [4 * RPW][K]
    volatile float *lk = lk_raw;
    __shared__ float cred[4][LPR * KPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const int C = a.n_cols, K = a.K;
    for (int i = threadIdx.x; i < 4 * RPW * K; i += 256) lk[i] = 0.f;
    __syncthreads();
    volatile float *mine = lk + (wave * RPW + sub) * K;      // written by the lanes of this sub-group only
    auto col = [&](int k) { return V4 ? sl * KPL + k : sl + k * LPR; };
    const bool want_pred = a.pred != nullptr;
    const int64_t rows_per_iter = int64_t(gridDim.x) * 4 * RPW * UN;
    float cs[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) cs[k] = 0.f;
    for (int64_t r0 = (int64_t(blockIdx.x) * 4 + wave) * RPW * UN; r0 < a.n_rows; r0 += rows_per_iter) {
        float x[UN][KPL];
        bool on[UN], valid[UN];
        int64_t r[UN];
        int g[UN], s0[UN], s1[UN], q0[UN], q1[UN], tc[UN], rt[UN];
        bool bad[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            r[u] = r0 + u * RPW + sub;
            valid[u] = r[u] < a.n_rows;
            g[u] = valid[u] ? a.group[r[u]] : -1;
            on[u] = valid[u] && a.mask[r[u]] != 0 && g[u] >= 0 && g[u] < K;
            segment_of(a, on[u] ? g[u] : -1, s0[u], s1[u]);
            rt[u] = -1;
            if (want_pred && valid[u]) rt[u] = a.route != nullptr ? a.route[r[u]] : g[u];
            segment_of(a, rt[u], q0[u], q1[u]);
            const int64_t t = on[u] ? a.target[r[u]] : 0;
            bad[u] = on[u] && (t < 0 || t >= s1[u] - s0[u]);      // (also: a segment the row cut short)
            tc[u] = (on[u] && !bad[u]) ? s0[u] + static_cast<int>(t) : -1;
            const float *row = a.logits + (valid[u] ? r[u] : 0) * a.ld;
            if constexpr (V4) {
                const int c0 = sl * KPL;
                float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                if (c0 < C && ((c0 < s1[u] && c0 + 4 > s0[u]) || (c0 < q1[u] && c0 + 4 > q0[u])))
                    v = *reinterpret_cast<const float4 *>(row + c0);
                x[u][0] = v.x, x[u][1] = v.y, x[u][2] = v.z, x[u][3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < KPL; ++k) {
                    const int c = col(k);
                    x[u][k] = (c < C && ((c >= s0[u] && c < s1[u]) || (c >= q0[u] && c < q1[u]))) ? row[c] : -INFINITY;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            bool in_t[KPL];
            float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < KPL; ++k) {
                in_t[k] = col(k) >= s0[u] && col(k) < s1[u];
                if (in_t[k]) m = fmaxf(m, x[u][k]);
            }
#pragma unroll
            for (int off = LPR / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
            if (want_pred) {
                // arg-max inside the ROUTE's segment (first index on ties), for every row, masked or not
                float mp = -INFINITY;
#pragma unroll
                for (int k = 0; k < KPL; ++k)
                    if (col(k) >= q0[u] && col(k) < q1[u]) mp = fmaxf(mp, x[u][k]);
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) mp = fmaxf(mp, __shfl_xor(mp, off, 64));
                int bi = INT32_MAX;
#pragma unroll
                for (int k = KPL - 1; k >= 0; --k)
                    if (col(k) >= q0[u] && col(k) < q1[u] && x[u][k] == mp) bi = min(bi, col(k));
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) bi = min(bi, __shfl_xor(bi, off, 64));
                if (valid[u] && sl == 0) {
                    int64_t p = -1;
                    if (q1[u] > q0[u]) {
                        const int c = bi == INT32_MAX ? q0[u] : bi;       // (a row of NaNs: the segment's first class)
                        p = a.class_map != nullptr ? a.class_map[c] : c;
                    }
                    a.pred[r[u]] = p;
                }
            }
            // The arithmetic of ce_rows (masked_ce.h), restated for a segment of the row: the target's term is kept out of
            // the sum of the others -- the gradient at the target is p_t - 1 = -(sum of the others) / sum, which
            // `e_t / sum - 1.f` would round to a multiple of 2^-24, the size of the whole gradient row of a confident sample.
            float e[KPL], others = 0.f, et = 0.f;
#pragma unroll
            for (int k = 0; k < KPL; ++k) {
                e[k] = in_t[k] ? expf(x[u][k] - m) : 0.f;
                if (col(k) == tc[u])
                    et = e[k];
                else
                    others += e[k];
            }
#pragma unroll
            for (int off = LPR / 2; off > 0; off >>= 1) others += __shfl_xor(others, off, 64);
            // e_t from the lane that holds the target column (0 from any lane when there is no valid target)
            et = __shfl(et, lane - sl + (tc[u] < 0 ? 0 : V4 ? tc[u] / KPL : tc[u] % LPR), 64);
            const float sum = others + et;
            if (on[u]) {
                // the lane that holds the target logit adds the row's term, log(sum) - (x_t - m), to its sub-group's slot of
                // the row's group: the difference first, so that a row at +-1e4 does not round its term to fp32's spacing there
                // (one update of the slot behind the column loop: hipcc 7 rejects its own code for the 16-byte
                // instantiations when the update sits inside it)
                const float lsum = logf(sum);
                float term = 0.f;
                bool mine_t = false;
#pragma unroll
                for (int k = 0; k < KPL; ++k)
                    if (col(k) == tc[u]) term = lsum - (x[u][k] - m), mine_t = true;
                if (mine_t) mine[g[u]] += term;
                // a class index outside the segment poisons the group's loss instead of being dropped silently
                // (torch raises; the Python wrapper checks the labels once per tensor)
                if (bad[u] && sl == 0) mine[g[u]] = NAN;
            }
            if (a.dlogits != nullptr && valid[u]) {
                float *drow = a.dlogits + r[u] * a.ldd;
                const float inv = on[u] ? 1.f / sum : 0.f;
                const float ic = on[u] ? a.inv_count[g[u]] : 0.f;
                float d[KPL];
#pragma unroll
                for (int k = 0; k < KPL; ++k) {
                    d[k] = in_t[k] ? (col(k) == tc[u] ? -(others * inv) : e[k] * inv) * ic : 0.f;
                    cs[k] += d[k];
                }
                if constexpr (V4) {
                    if (sl * KPL < C) *reinterpret_cast<float4 *>(drow + sl * KPL) = make_float4(d[0], d[1], d[2], d[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < KPL; ++k)
                        if (col(k) < C) drow[col(k)] = d[k];
                }
            }
        }
    }
    if (a.colpart != nullptr) {
        // column sums of the gradient rows: the sub-groups of a wave, then the four waves, in a fixed order
#pragma unroll
        for (int k = 0; k < KPL; ++k) {
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) cs[k] += __shfl_xor(cs[k], off, 64);
            if (sub == 0) cred[wave][sl * KPL + k] = cs[k];
        }
    }
    flush_group_terms(lk, 4 * RPW, K, a.part_k);           // (its barrier also covers cred)
    if (a.colpart != nullptr && wave == 0 && sub == 0) {
#pragma unroll
        for (int k = 0; k < KPL; ++k) {
            const int c = col(k), i = sl * KPL + k;
            if (c < C) a.colpart[int64_t(blockIdx.x) * C + c] = (cred[0][i] + cred[1][i]) + (cred[2][i] + cred[3][i]);
        }
    }
}

// Rows wider than 256 columns: one wave per row, the lanes stride over the segment.
__global__ __launch_bounds__(256) void k_grouped_ce_wide(const GceArgs a) {
    constexpr int UN = 2;
    extern __shared__ float lk_raw[];                 // [4][K]
    volatile float *lk = lk_raw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.n_cols, K = a.K;
    for (int i = threadIdx.x; i < 4 * K; i += 256) lk[i] = 0.f;
    __syncthreads();
    volatile float *mine = lk + wave * K;
    const bool want_pred = a.pred != nullptr;
    const int64_t rows_per_iter = int64_t(gridDim.x) * 4 * UN;
    for (int64_t r0 = (int64_t(blockIdx.x) * 4 + wave) * UN; r0 < a.n_rows; r0 += rows_per_iter) {
        for (int u = 0; u < UN; ++u) {
            const int64_t r = r0 + u;                 // wave-uniform
            if (r >= a.n_rows) break;
            const int g = a.group[r];
            const bool on = a.mask[r] != 0 && g >= 0 && g < K;
            int s0, s1, q0, q1;
            segment_of(a, on ? g : -1, s0, s1);
            const float *row = a.logits + r * a.ld;
            if (want_pred) {
                const int rt = a.route != nullptr ? a.route[r] : g;
                segment_of(a, rt, q0, q1);
                float mp = -INFINITY;
                for (int c = q0 + lane; c < q1; c += 64) mp = fmaxf(mp, row[c]);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) mp = fmaxf(mp, __shfl_xor(mp, off, 64));
                int bi = INT32_MAX;
                for (int c = q0 + lane; c < q1; c += 64)
                    if (row[c] == mp) {
                        bi = c;
                        break;
                    }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) bi = min(bi, __shfl_xor(bi, off, 64));
                if (lane == 0) {
                    int64_t p = -1;
                    if (q1 > q0) {
                        const int c = bi == INT32_MAX ? q0 : bi;
                        p = a.class_map != nullptr ? a.class_map[c] : c;
                    }
                    a.pred[r] = p;
                }
            }
            float m = -INFINITY;
            for (int c = s0 + lane; c < s1; c += 64) m = fmaxf(m, row[c]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
            // as on the register path: the target's term apart from the sum of the others, differences from the row
            // maximum before anything is added to log(sum)
            const int64_t t = on ? a.target[r] : 0;
            const bool bad = on && (t < 0 || t >= s1 - s0);
            const int tc = (on && !bad) ? s0 + static_cast<int>(t) : -1;      // (no read outside the segment)
            const float xt = tc >= 0 ? row[tc] - m : 0.f;
            float s = 0.f;
            for (int c = s0 + lane; c < s1; c += 64)
                if (c != tc) s += expf(row[c] - m);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            const float sum = s + (tc >= 0 ? expf(xt) : 0.f);
            if (on && lane == 0) {
                if (bad)
                    mine[g] = NAN;
                else
                    mine[g] += logf(sum) - xt;
            }
            if (a.dlogits != nullptr) {
                float *drow = a.dlogits + r * a.ldd;
                const float ic = on ? a.inv_count[g] : 0.f;
                const float inv = on ? 1.f / sum : 0.f;
                for (int c = lane; c < C; c += 64)
                    drow[c] = (c >= s0 && c < s1) ? (c == tc ? -(s * inv) : expf(row[c] - m) * inv) * ic : 0.f;
            }
        }
    }
    flush_group_terms(lk, 4, K, a.part_k);
}

// loss_k[k] = inv_count[k] * sum of the workgroup partials (NaN for a group without a selected row: torch's mean over
// nothing), loss = sum of the others, group by group in index order.
__global__ __launch_bounds__(256) void k_grouped_ce_final(const float *__restrict__ part_k, int n_part, int K,
                                                          const float *__restrict__ inv_count, float *__restrict__ loss,
                                                          float *__restrict__ loss_k) {
    __shared__ float red[256];
    float total = 0.f;                                // (thread 0's copy is the one that is stored)
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
        for (int i = threadIdx.x; i < n_part; i += 256) s += part_k[int64_t(i) * K + k];
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

int lanes_per_row(int n_cols) { return n_cols <= 16 ? 4 : n_cols <= 32 ? 8 : n_cols <= 64 ? 16 : n_cols <= 128 ? 32 : 64; }

}  // namespace
}  // namespace tgcn

extern "C" {

size_t tgcn_grouped_ce_workspace_bytes(int64_t n_rows, int n_cols, int n_groups) {
    if (n_rows < 0 || n_cols <= 0 || n_groups <= 0) return 0;
    const size_t rows = std::max<size_t>(tgcn::kGceBlocks, static_cast<size_t>(tgcn::colsum_blocks(n_rows)));
    return sizeof(float) * (static_cast<size_t>(tgcn::kGceBlocks) * static_cast<size_t>(n_groups) +
                            rows * static_cast<size_t>(n_cols));
}

int tgcn_grouped_ce(const float *logits, int64_t ld, int64_t n_rows, int n_cols, int n_groups,
                    const int32_t *seg_start_host, const int32_t *seg_width_host, const int32_t *seg_start,
                    const int32_t *seg_width, const int32_t *group, const int32_t *route, const int64_t *target,
                    const uint8_t *mask, const float *inv_count, const int64_t *class_map, float *loss, float *loss_k,
                    float *dlogits, int64_t ldd, float *dbias, int64_t *pred, void *workspace, size_t workspace_bytes,
                    tgcn_stream stream) {
    using namespace tgcn;
    const char *who = "tgcn_grouped_ce";
    // (an empty matrix may come with NULL row arrays: torch hands out no storage for zero rows)
    if ((n_rows > 0 && (!logits || !group || !target || !mask || (dbias && !dlogits))) || !seg_start_host || !seg_width_host ||
        !seg_start || !seg_width || !inv_count || !loss || n_rows < 0 || n_cols <= 0 || n_groups <= 0 ||
        n_groups > kGceMaxGroups || ld < n_cols || ((dlogits || dbias) && ldd < n_cols)) {
        set_error("%s: bad argument (n_rows=%lld n_cols=%d n_groups=%d (at most %d) ld=%lld ldd=%lld)", who,
                  (long long)n_rows, n_cols, n_groups, kGceMaxGroups, (long long)ld, (long long)ldd);
        return TGCN_E_INVALID;
    }
    int64_t end = 0;
    for (int k = 0; k < n_groups; ++k) {
        const int64_t s = seg_start_host[k], w = seg_width_host[k];
        if (s < end || w < 1 || s + w > n_cols) {
            set_error("%s: segment %d = [%lld, %lld) must have a width >= 1, start at or after the end of segment %d (%lld) "
                      "and end inside the %d columns", who, k, (long long)s, (long long)(s + w), k - 1, (long long)end, n_cols);
            return TGCN_E_INVALID;
        }
        end = s + w;
    }
    const size_t need = tgcn_grouped_ce_workspace_bytes(n_rows, n_cols, n_groups);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes given, %zu needed", who, workspace_bytes, need);
        return TGCN_E_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part_k = static_cast<float *>(workspace);
    float *colws = part_k + static_cast<size_t>(kGceBlocks) * n_groups;
    const bool regs = n_cols <= 256;
    const int lpr = lanes_per_row(n_cols);
    const int64_t rows_per_block = regs ? 2 * 4 * (64 / lpr) : 2 * 4;
    const int grid = static_cast<int>(std::min<int64_t>(kGceBlocks, std::max<int64_t>(1, (n_rows + rows_per_block - 1) / rows_per_block)));
    GceArgs a{logits, ld, n_cols, n_groups, seg_start, seg_width, group, route, target, mask, inv_count, class_map, n_rows,
              dlogits, ldd, part_k, pred, (dbias && regs) ? colws : nullptr};
    if (regs) {
        const bool v4 = n_cols % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
                        (!dlogits || (ldd % 4 == 0 && reinterpret_cast<uintptr_t>(dlogits) % 16 == 0));
        const size_t lds = sizeof(float) * 4 * (64 / lpr) * static_cast<size_t>(n_groups);
#define TGCN_GCE(LPR)                                                  \
    do {                                                               \
        if (v4)                                                        \
            k_grouped_ce<LPR, true><<<grid, 256, lds, s>>>(a);         \
        else                                                           \
            k_grouped_ce<LPR, false><<<grid, 256, lds, s>>>(a);        \
    } while (0)
        if (lpr == 4)
            TGCN_GCE(4);
        else if (lpr == 8)
            TGCN_GCE(8);
        else if (lpr == 16)
            TGCN_GCE(16);
        else if (lpr == 32)
            TGCN_GCE(32);
        else
            TGCN_GCE(64);
#undef TGCN_GCE
    } else {
        k_grouped_ce_wide<<<grid, 256, sizeof(float) * 4 * static_cast<size_t>(n_groups), s>>>(a);
    }
    TGCN_HIP_CHECK(hipGetLastError());
    k_grouped_ce_final<<<1, 256, 0, s>>>(part_k, grid, n_groups, inv_count, loss, loss_k);
    TGCN_HIP_CHECK(hipGetLastError());
    if (dbias) {
        if (regs) return launch_colsum_final(colws, grid, n_cols, dbias, s);
        return launch_colsum(dlogits, ldd, n_rows, n_cols, dbias, colws, colsum_blocks(n_rows), s);
    }
    return TGCN_OK;
}

}  // extern "C"
