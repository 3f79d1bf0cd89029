// One cell of the reference's hyper-parameter sweeps (old/h_o_train.py and its siblings: len(lrs) x KFold(k) two-layer GCNs
// on ONE graph) trained as one network of K equal-width members (pytextgcn_amd/crossval.py).  The network side is
// PerLabelGCN's; the two kernels here are what a sweep cell needs beyond it.
//
//   k_member_ce      masked CrossEntropyLoss('mean') of K members in one pass.  Member k owns the columns
//                    [k * S, k * S + C) of the logits (S = seg_stride >= C, the columns behind C are pad) and selects row r
//                    where bit k of bits[r] is set: in cross-validation a document is a training row of k - 1 members and a
//                    validation row of the remaining one, so EVERY row meets EVERY segment (tgcn_grouped_ce trains a row on
//                    the segment of its one group).  The members are uniform, so the logits are N * K "virtual rows" of C
//                    columns: the row scheme of k_masked_ce (train.hip) with blockIdx.y = member -- base offset k * S, mask =
//                    bit k, divisor inv_count[k], one partial slot per (workgroup, member).  Its arithmetic is k_masked_ce's:
//                    the target's term is kept out of the sum of the others, differences from the row maximum come first.
//   k_adam_members   tgcn_adam_step on a [n_rows, K * member_width] tensor whose column block k takes the rate lr[k]: the
//                    members are column blocks of shared tensors and Adam is elementwise, so block k after a step is bit for
//                    bit what tgcn_adam_step with lr[k] gives on a contiguous copy of it (the same adam_element).
//   k_adam_member_rows  the same with the members as contiguous ROW blocks of a flat tensor (the stacked tensors of a
//                    CrossValEGCN), every index 64-bit: such a tensor passes 2^31 elements.
// All are deterministic (fixed-order two-stage reductions, no atomics) and only enqueue on the caller's stream.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace tgcn {
namespace {

constexpr int kMceBlocks = 2048;       // workgroups of one launch, shared by the members: gridDim.x <= mce_cap(K)
constexpr int kMceMinBlocks = 32;
constexpr int kMaxMembers = 64;        // one bit of bits[r] per member

int mce_cap(int K) { return std::max(kMceMinBlocks, kMceBlocks / K); }

struct MceArgs {
    const float *logits;
    int64_t ld;
    int C;                      // classes of a member
    int S;                      // columns from one member's segment to the next
    int K;
    const int64_t *target;
    const uint64_t *bits;
    const float *inv_count;     // [K]
    int64_t n_rows;
    float *dlogits;
    int64_t ldd;
    float *partial;             // [K][gridDim.x]
    int32_t *pred;              // [n_rows][K]
    float *colpart;             // [gridDim.x][K][C] or nullptr
};

// LPR lanes cooperate on one row of one member (blockIdx.y); everything else is the scheme of k_masked_ce (train.hip).
// V4 (S, ld, ldd multiples of 4, 16-byte aligned bases -- whatever C is): a lane's KPL logits are CONSECUTIVE columns of
// the segment, read and written 16 bytes at a time up to the stride; the lanes predicate the pad columns to -inf.
// Otherwise they are LPR columns apart (4-byte accesses).  The workgroup writes the zeros of its member's pad columns
// and of the rows its member does not select itself.
template <int LPR, bool V4, int KPL = 4>
__global__ __launch_bounds__(256) void k_member_ce(const MceArgs a) {
    constexpr int RPW = 64 / LPR;
    static_assert(KPL == 4 || KPL == 8, "logits per lane on the register path");
    constexpr int UN = 2;        // row groups in flight per wave
    __shared__ float red[4];
    __shared__ float cred[4][LPR * KPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const int C = a.C, S = a.S, K = a.K;
    const int member = blockIdx.y;
    const int64_t base = int64_t(member) * S;
    const float inv_count = a.inv_count[member];
    const int64_t rows_per_iter = int64_t(gridDim.x) * 4 * RPW * UN;
    const bool in_regs = C <= KPL * LPR;
    const bool want_pred = a.pred != nullptr;
    auto col = [&](int k) { return V4 ? sl * KPL + k : sl + k * LPR; };
    float loss = 0.f;
    float cs[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) cs[k] = 0.f;
    for (int64_t r0 = (int64_t(blockIdx.x) * 4 + wave) * RPW * UN; r0 < a.n_rows; r0 += rows_per_iter) {
        if (in_regs) {
            float x[UN][KPL];
            bool on[UN], valid[UN];
            int64_t r[UN], t[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                r[u] = r0 + u * RPW + sub;
                valid[u] = r[u] < a.n_rows;
                on[u] = valid[u] && ((a.bits[r[u]] >> member) & 1) != 0;
                const float *row = a.logits + (valid[u] ? r[u] : 0) * a.ld + base;
                t[u] = on[u] ? a.target[r[u]] : 0;
                const bool need = on[u] || (want_pred && valid[u]);
                if constexpr (V4) {
#pragma unroll
                    for (int q = 0; q < KPL / 4; ++q) {
                        const int c0 = sl * KPL + 4 * q;
                        float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                        if (need && c0 < C) v = *reinterpret_cast<const float4 *>(row + c0);   // (c0 + 3 < S: S % 4 == 0)
                        x[u][4 * q] = v.x;
                        x[u][4 * q + 1] = c0 + 1 < C ? v.y : -INFINITY;
                        x[u][4 * q + 2] = c0 + 2 < C ? v.z : -INFINITY;
                        x[u][4 * q + 3] = c0 + 3 < C ? v.w : -INFINITY;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < KPL; ++k) {
                        const int c = col(k);
                        x[u][k] = (need && c < C) ? row[c] : -INFINITY;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                float m = fmaxf(fmaxf(x[u][0], x[u][1]), fmaxf(x[u][2], x[u][3]));
#pragma unroll
                for (int q = 1; q < KPL / 4; ++q)
                    m = fmaxf(m, fmaxf(fmaxf(x[u][4 * q], x[u][4 * q + 1]), fmaxf(x[u][4 * q + 2], x[u][4 * q + 3])));
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
                if (want_pred) {
                    // local arg-max of the segment (first index on ties), for every row, selected or not
                    int bi = INT32_MAX;
#pragma unroll
                    for (int k = KPL - 1; k >= 0; --k)
                        if (x[u][k] == m && col(k) < C) bi = col(k);
#pragma unroll
                    for (int off = LPR / 2; off > 0; off >>= 1) bi = min(bi, __shfl_xor(bi, off, 64));
                    if (valid[u] && sl == 0) a.pred[r[u] * K + member] = bi == INT32_MAX ? 0 : bi;
                }
                // The target's term is kept out of the sum of the others (k_masked_ce): the gradient at the target is
                // p_t - 1 = -(sum of the others) / sum, which `e_t / sum - 1.f` would round to a multiple of 2^-24.
                float e[KPL], others = 0.f, et = 0.f;
#pragma unroll
                for (int k = 0; k < KPL; ++k) {
                    e[k] = on[u] ? expf(x[u][k] - m) : 0.f;   // exp(-inf) = 0 for the padding
                    if (col(k) == t[u])
                        et = e[k];
                    else
                        others += e[k];
                }
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) others += __shfl_xor(others, off, 64);
                {
                    // e_t from the lane that holds the target column (0 from any lane when the target is invalid)
                    const int tc = static_cast<int>(t[u] < 0 ? 0 : t[u] >= C ? C - 1 : t[u]);
                    et = __shfl(et, lane - sl + (V4 ? tc / KPL : tc % LPR), 64);
                }
                const float sum = others + et;
                if (on[u]) {
                    // the lane that holds the target logit adds the row's term, log(sum) - (x_t - m): the difference first
                    const float lsum = logf(sum);
#pragma unroll
                    for (int k = 0; k < KPL; ++k)
                        if (col(k) == t[u]) loss += lsum - (x[u][k] - m);
                    // a class index outside [0, C) poisons the member's loss instead of being dropped silently
                    if (sl == 0 && (t[u] < 0 || t[u] >= C)) loss = NAN;
                }
                if (a.dlogits != nullptr && valid[u]) {
                    float *drow = a.dlogits + r[u] * a.ldd + base;
                    const float inv = on[u] ? 1.f / sum : 0.f;
                    float d[KPL];
#pragma unroll
                    for (int k = 0; k < KPL; ++k) {
                        const int c = col(k);
                        d[k] = (on[u] && c < C) ? (c == t[u] ? -(others * inv) : e[k] * inv) * inv_count : 0.f;
                        cs[k] += d[k];
                    }
                    if constexpr (V4) {
#pragma unroll
                        for (int q = 0; q < KPL / 4; ++q)
                            if (sl * KPL + 4 * q < S)
                                *reinterpret_cast<float4 *>(drow + sl * KPL + 4 * q) =
                                    make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
                        for (int c = LPR * KPL + 4 * sl; c < S; c += 4 * LPR)          // pad beyond the lanes' columns
                            *reinterpret_cast<float4 *>(drow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
                    } else {
#pragma unroll
                        for (int k = 0; k < KPL; ++k)
                            if (col(k) < S) drow[col(k)] = d[k];
                        for (int c = LPR * KPL + sl; c < S; c += LPR) drow[c] = 0.f;
                    }
                }
            }
        } else {
            for (int u = 0; u < UN; ++u) {
                const int64_t r = r0 + u * RPW + sub;
                const bool valid = r < a.n_rows;
                const bool on = valid && ((a.bits[r] >> member) & 1) != 0;
                const float *row = a.logits + (valid ? r : 0) * a.ld + base;
                float m = -INFINITY;
                if (on || (want_pred && valid))
                    for (int c = sl; c < C; c += LPR) m = fmaxf(m, row[c]);
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
                if (want_pred) {
                    int bi = INT32_MAX;
                    if (valid)
                        for (int c = sl; c < C; c += LPR)
                            if (row[c] == m) {
                                bi = c;
                                break;
                            }
#pragma unroll
                    for (int off = LPR / 2; off > 0; off >>= 1) bi = min(bi, __shfl_xor(bi, off, 64));
                    if (valid && sl == 0) a.pred[r * K + member] = bi == INT32_MAX ? 0 : bi;
                }
                const int64_t t = on ? a.target[r] : 0;
                const bool t_ok = on && t >= 0 && t < C;   // no read outside the segment
                const float xt = t_ok ? row[t] - m : 0.f;
                float s = 0.f;
                if (on)
                    for (int c = sl; c < C; c += LPR)
                        if (c != t) s += expf(row[c] - m);
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
                const float sum = s + (t_ok ? expf(xt) : 0.f);
                if (on && sl == 0) loss += t_ok ? logf(sum) - xt : NAN;
                if (a.dlogits != nullptr && valid) {
                    float *drow = a.dlogits + r * a.ldd + base;
                    const float inv = on ? 1.f / sum : 0.f;
                    for (int c = sl; c < C; c += LPR)
                        drow[c] = on ? (c == t ? -(s * inv) : expf(row[c] - m) * inv) * inv_count : 0.f;
                    for (int c = C + sl; c < S; c += LPR) drow[c] = 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) loss += __shfl_xor(loss, off, 64);
    if (lane == 0) red[wave] = loss;
    if (a.colpart != nullptr) {
        // column sums of the gradient rows: the sub-groups of a wave, then the four waves, in a fixed order
#pragma unroll
        for (int k = 0; k < KPL; ++k) {
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) cs[k] += __shfl_xor(cs[k], off, 64);
            if (sub == 0) cred[wave][sl * KPL + k] = cs[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) a.partial[int64_t(member) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (a.colpart != nullptr && wave == 0 && sub == 0) {
        float *out = a.colpart + (int64_t(blockIdx.x) * K + member) * C;
#pragma unroll
        for (int k = 0; k < KPL; ++k) {
            const int c = col(k), i = sl * KPL + k;
            if (c < C) out[c] = (cred[0][i] + cred[1][i]) + (cred[2][i] + cred[3][i]);
        }
    }
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

// ---- Adam with one learning rate per column block --------------------------------------------------------------------
struct MemberRates {
    float step_size[kMaxMembers];      // lr[k] / (1 - beta1^t), derived in double and rounded once (adam_impl)
};
struct MemberLrs {
    double lr[kMaxMembers];
};

// Capturable form (k_adam_scalars of train.hip with K rates): thread 0 advances the device step; thread k < K leaves
// lr[k] / bc1 in scalars[k], thread 0 1 / sqrt(bc2) in scalars[K] -- all in double, as the host path derives them.
__global__ __launch_bounds__(64) void k_adam_member_scalars(int64_t *step, const MemberLrs lrs, int K, double b1, double b2,
                                                            float *scalars) {
    const int64_t s = *step + 1;
    __syncthreads();                    // every thread has read the step before thread 0 advances it
    const double bc1 = 1.0 - pow(b1, static_cast<double>(s));
    if (static_cast<int>(threadIdx.x) < K) scalars[threadIdx.x] = static_cast<float>(lrs.lr[threadIdx.x] / bc1);
    if (threadIdx.x == 0) {
        *step = s;
        const double bc2 = 1.0 - pow(b2, static_cast<double>(s));
        scalars[K] = static_cast<float>(1.0 / sqrt(bc2));
    }
}

// NT: state and gradient are touched once per step and stream past the caches; the parameter keeps plain accesses
// (train.hip: k_adam).
typedef float member_f4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float *q) {
    if constexpr (NT) {
        const member_f4 t = __builtin_nontemporal_load(reinterpret_cast<const member_f4 *>(q));
        return make_float4(t.x, t.y, t.z, t.w);
    } else {
        return *reinterpret_cast<const float4 *>(q);
    }
}
template <bool NT>
__device__ __forceinline__ void st4(float *q, const float4 &a) {
    if constexpr (NT) {
        member_f4 t = {a.x, a.y, a.z, a.w};
        __builtin_nontemporal_store(t, reinterpret_cast<member_f4 *>(q));
    } else {
        *reinterpret_cast<float4 *>(q) = a;
    }
}

// V4 (member_width and n_cols multiples of 4): the four elements of a 16-byte body lie in one member.  Otherwise every
// element looks its member up (4-byte accesses).  IDX32: the flat index fits 32 bits (its division is the cheaper one).
template <bool AMSGRAD, bool NT, bool V4, bool IDX32>
__global__ __launch_bounds__(256) void k_adam_members(float *__restrict__ p, const float *__restrict__ g,
                                                      float *__restrict__ m, float *__restrict__ v,
                                                      float *__restrict__ vmax, int64_t n, uint32_t n_cols, uint32_t width,
                                                      int K, float w1 /* 1-b1 */, float b2, float w2 /* 1-b2 */, float eps,
                                                      float wd, const MemberRates host, float inv_bc2_sqrt,
                                                      const float *__restrict__ dev_scalars) {
    __shared__ float rate[kMaxMembers];
    if (static_cast<int>(threadIdx.x) < K)
        rate[threadIdx.x] = dev_scalars != nullptr ? dev_scalars[threadIdx.x] : host.step_size[threadIdx.x];
    if (dev_scalars != nullptr) inv_bc2_sqrt = dev_scalars[K];
    __syncthreads();
    auto col_of = [&](int64_t i) {
        return IDX32 ? static_cast<uint32_t>(i) % n_cols : static_cast<uint32_t>(static_cast<uint64_t>(i) % n_cols);
    };
    const int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
    for (int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if constexpr (V4) {                       // (n is a multiple of 4: no tail)
            const float step_size = rate[col_of(i) / width];
            float4 pp = *reinterpret_cast<float4 *>(p + i);
            const float4 gg = ld4<NT>(g + i);
            float4 mm = ld4<NT>(m + i);
            float4 vv = ld4<NT>(v + i);
            float4 xx = make_float4(0.f, 0.f, 0.f, 0.f);
            if (AMSGRAD) xx = ld4<NT>(vmax + i);
            float *P = &pp.x, *M = &mm.x, *V = &vv.x, *X = &xx.x;
            const float *G = &gg.x;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                adam_element(P[k], G[k], M[k], V[k], X[k], AMSGRAD, w1, b2, w2, eps, wd, step_size, inv_bc2_sqrt);
            *reinterpret_cast<float4 *>(p + i) = pp;
            st4<NT>(m + i, mm);
            st4<NT>(v + i, vv);
            if (AMSGRAD) st4<NT>(vmax + i, xx);
        } else {
            uint32_t c = col_of(i);
            const int64_t end = i + 4 < n ? i + 4 : n;
            for (int64_t j = i; j < end; ++j) {
                float pj = p[j], mj = m[j], vj = v[j], xj = AMSGRAD ? vmax[j] : 0.f;
                adam_element(pj, g[j], mj, vj, xj, AMSGRAD, w1, b2, w2, eps, wd, rate[c / width], inv_bc2_sqrt);
                p[j] = pj;
                m[j] = mj;
                v[j] = vj;
                if (AMSGRAD) vmax[j] = xj;
                if (++c == n_cols) c = 0;
            }
        }
    }
}

// The members as ROW blocks (the stacked embedding weight [M D, in] of a CrossValEGCN): a flat tensor of n = K * block
// elements, element i takes the rate of member i / block.  Such a tensor passes 2^31 elements (12 members at 100 000
// nodes and D = 2000 are 2.4e9), so every index here is 64-bit.  V4 (block a multiple of 4, hence n too): the four
// elements of a 16-byte body lie in one member and there is no tail.  Otherwise every element looks its member up.
template <bool AMSGRAD, bool NT, bool V4>
__global__ __launch_bounds__(256) void k_adam_member_rows(float *__restrict__ p, const float *__restrict__ g,
                                                          float *__restrict__ m, float *__restrict__ v,
                                                          float *__restrict__ vmax, int64_t n, int64_t block, int K,
                                                          float w1 /* 1-b1 */, float b2, float w2 /* 1-b2 */, float eps,
                                                          float wd, const MemberRates host, float inv_bc2_sqrt,
                                                          const float *__restrict__ dev_scalars) {
    __shared__ float rate[kMaxMembers];
    if (static_cast<int>(threadIdx.x) < K)
        rate[threadIdx.x] = dev_scalars != nullptr ? dev_scalars[threadIdx.x] : host.step_size[threadIdx.x];
    if (dev_scalars != nullptr) inv_bc2_sqrt = dev_scalars[K];
    __syncthreads();
    const int64_t stride = int64_t(gridDim.x) * blockDim.x * 4;
    for (int64_t i = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if constexpr (V4) {
            const float step_size = rate[i / block];
            float4 pp = *reinterpret_cast<float4 *>(p + i);
            const float4 gg = ld4<NT>(g + i);
            float4 mm = ld4<NT>(m + i);
            float4 vv = ld4<NT>(v + i);
            float4 xx = make_float4(0.f, 0.f, 0.f, 0.f);
            if (AMSGRAD) xx = ld4<NT>(vmax + i);
            float *P = &pp.x, *M = &mm.x, *V = &vv.x, *X = &xx.x;
            const float *G = &gg.x;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                adam_element(P[k], G[k], M[k], V[k], X[k], AMSGRAD, w1, b2, w2, eps, wd, step_size, inv_bc2_sqrt);
            *reinterpret_cast<float4 *>(p + i) = pp;
            st4<NT>(m + i, mm);
            st4<NT>(v + i, vv);
            if (AMSGRAD) st4<NT>(vmax + i, xx);
        } else {
            int64_t k = i / block, left = (k + 1) * block - i;     // elements of member k from i on
            const int64_t end = i + 4 < n ? i + 4 : n;
            for (int64_t j = i; j < end; ++j) {
                float pj = p[j], mj = m[j], vj = v[j], xj = AMSGRAD ? vmax[j] : 0.f;
                adam_element(pj, g[j], mj, vj, xj, AMSGRAD, w1, b2, w2, eps, wd, rate[k], inv_bc2_sqrt);
                p[j] = pj;
                m[j] = mj;
                v[j] = vj;
                if (AMSGRAD) vmax[j] = xj;
                if (--left == 0) {
                    ++k;
                    left = block;
                }
            }
        }
    }
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
    // lanes per row and logits per lane by class count, as masked_ce_impl (train.hip) chooses them
    const int lpr = C <= 32 ? 4 : C <= 64 ? 8 : C <= 128 ? 16 : C <= 256 ? 32 : 64;
    const int64_t rows_per_block = 2 * 4 * (64 / lpr);
    const int gx = static_cast<int>(std::min<int64_t>(cap, std::max<int64_t>(1, (n_rows + rows_per_block - 1) / rows_per_block)));
    const bool regs = C <= 256;
    const bool v4 = S % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
                    (!dlogits || (ldd % 4 == 0 && reinterpret_cast<uintptr_t>(dlogits) % 16 == 0));
    const MceArgs a{logits, ld, C, S, K, target, bits, inv_count, n_rows, dlogits, ldd, partial, pred,
                    (dbias && regs) ? colws : nullptr};
    const dim3 grid(gx, K);
#define TGCN_MCE(LPR, KPL)                                          \
    do {                                                            \
        if (v4)                                                     \
            k_member_ce<LPR, true, KPL><<<grid, 256, 0, s>>>(a);    \
        else                                                        \
            k_member_ce<LPR, false, KPL><<<grid, 256, 0, s>>>(a);   \
    } while (0)
    if (C <= 16)
        TGCN_MCE(4, 4);
    else if (C <= 32)
        TGCN_MCE(4, 8);
    else if (C <= 64)
        TGCN_MCE(8, 8);
    else if (C <= 128)
        TGCN_MCE(16, 8);
    else if (C <= 256)
        TGCN_MCE(32, 8);
    else
        TGCN_MCE(64, 4);
#undef TGCN_MCE
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
    const uintptr_t al = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                         reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq) |
                         reinterpret_cast<uintptr_t>(max_exp_avg_sq);
    if (n > 0 && al % 16 != 0) {
        set_error("%s: buffers must be 16-byte aligned", who);
        return TGCN_E_INVALID;
    }
    if (n == 0 && step_dev == nullptr) return TGCN_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every constant in double, rounded once (adam_impl of train.hip)
    const double bc1 = 1.0 - std::pow(beta1, static_cast<double>(step));
    const double bc2 = 1.0 - std::pow(beta2, static_cast<double>(step));
    MemberRates rates{};
    for (int k = 0; k < K; ++k) rates.step_size[k] = static_cast<float>(lr_host[k] / bc1);
    const float w1 = static_cast<float>(1.0 - beta1), w2 = static_cast<float>(1.0 - beta2);
    const float b2f = static_cast<float>(beta2), epsf = static_cast<float>(eps), wdf = static_cast<float>(weight_decay);
    const float inv_bc2_sqrt = static_cast<float>(1.0 / std::sqrt(bc2));
    if (step_dev != nullptr) {
        MemberLrs lrs{};
        for (int k = 0; k < K; ++k) lrs.lr[k] = lr_host[k];
        k_adam_member_scalars<<<1, 64, 0, s>>>(step_dev, lrs, K, beta1, beta2, scalars_dev);
        TGCN_HIP_CHECK(hipGetLastError());
        if (n == 0) return TGCN_OK;
    }
    const int grid = static_cast<int>(std::min<int64_t>(8192, (n / 4 + 255) / 256 + 1));
    const bool nt = n >= (int64_t(1) << 24);
    const bool v4 = member_width % 4 == 0 && n_cols % 4 == 0;
    const bool i32 = n <= INT32_MAX;
    const uint32_t nc = static_cast<uint32_t>(n_cols), mw = static_cast<uint32_t>(member_width);
#define TGCN_MADAM4(AMS, NTV, V4V, I32)                                                                                  \
    k_adam_members<AMS, NTV, V4V, I32><<<grid, 256, 0, s>>>(param, grad, exp_avg, exp_avg_sq,                             \
                                                            AMS ? max_exp_avg_sq : nullptr, n, nc, mw, K, w1, b2f, w2,    \
                                                            epsf, wdf, rates, inv_bc2_sqrt, scalars_dev)
#define TGCN_MADAM2(AMS, NTV)                                       \
    do {                                                            \
        if (v4 && i32)                                              \
            TGCN_MADAM4(AMS, NTV, true, true);                      \
        else if (v4)                                                \
            TGCN_MADAM4(AMS, NTV, true, false);                     \
        else if (i32)                                               \
            TGCN_MADAM4(AMS, NTV, false, true);                     \
        else                                                        \
            TGCN_MADAM4(AMS, NTV, false, false);                    \
    } while (0)
    if (max_exp_avg_sq) {
        if (nt) TGCN_MADAM2(true, true); else TGCN_MADAM2(true, false);
    } else {
        if (nt) TGCN_MADAM2(false, true); else TGCN_MADAM2(false, false);
    }
#undef TGCN_MADAM2
#undef TGCN_MADAM4
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
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
    const uintptr_t al = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                         reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq) |
                         reinterpret_cast<uintptr_t>(max_exp_avg_sq);
    if (n > 0 && al % 16 != 0) {
        set_error("%s: buffers must be 16-byte aligned", who);
        return TGCN_E_INVALID;
    }
    if (n == 0 && step_dev == nullptr) return TGCN_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every constant in double, rounded once (adam_impl of train.hip)
    const double bc1 = 1.0 - std::pow(beta1, static_cast<double>(step));
    const double bc2 = 1.0 - std::pow(beta2, static_cast<double>(step));
    MemberRates rates{};
    for (int k = 0; k < K; ++k) rates.step_size[k] = static_cast<float>(lr_host[k] / bc1);
    const float w1 = static_cast<float>(1.0 - beta1), w2 = static_cast<float>(1.0 - beta2);
    const float b2f = static_cast<float>(beta2), epsf = static_cast<float>(eps), wdf = static_cast<float>(weight_decay);
    const float inv_bc2_sqrt = static_cast<float>(1.0 / std::sqrt(bc2));
    if (step_dev != nullptr) {
        MemberLrs lrs{};
        for (int k = 0; k < K; ++k) lrs.lr[k] = lr_host[k];
        k_adam_member_scalars<<<1, 64, 0, s>>>(step_dev, lrs, K, beta1, beta2, scalars_dev);
        TGCN_HIP_CHECK(hipGetLastError());
        if (n == 0) return TGCN_OK;
    }
    const int grid = static_cast<int>(std::min<int64_t>(8192, (n / 4 + 255) / 256 + 1));
    const bool nt = n >= (int64_t(1) << 24);
    const bool v4 = block % 4 == 0;
#define TGCN_RADAM3(AMS, NTV, V4V)                                                                                        \
    k_adam_member_rows<AMS, NTV, V4V><<<grid, 256, 0, s>>>(param, grad, exp_avg, exp_avg_sq,                              \
                                                           AMS ? max_exp_avg_sq : nullptr, n, block, K, w1, b2f, w2, epsf, \
                                                           wdf, rates, inv_bc2_sqrt, scalars_dev)
#define TGCN_RADAM2(AMS, NTV)                                       \
    do {                                                            \
        if (v4)                                                     \
            TGCN_RADAM3(AMS, NTV, true);                            \
        else                                                        \
            TGCN_RADAM3(AMS, NTV, false);                           \
    } while (0)
    if (max_exp_avg_sq) {
        if (nt) TGCN_RADAM2(true, true); else TGCN_RADAM2(true, false);
    } else {
        if (nt) TGCN_RADAM2(false, true); else TGCN_RADAM2(false, false);
    }
#undef TGCN_RADAM2
#undef TGCN_RADAM3
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
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
