// The row body of the masked cross-entropy kernels and the table that picks its instantiation, shared by k_masked_ce
// (train.hip: one [N, C] matrix, one mask) and k_member_ce (crossval.hip: K members side by side, one bit per member).
// The arithmetic -- the target's term kept out of the sum of the others, differences from the row maximum before logf --
// stands here once; a kernel supplies a `Rows` view that says where a row, its selection bit, its divisor and its output
// slots are, and nothing else.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace tgcn {

// ---- host: the leaf by class count ---------------------------------------------------------------------------------
// f(LPR, KPL, V4) as std::integral_constant / std::bool_constant, by class count.
// Logits per lane on the register path: 8 (half the lanes per row, one shuffle level less in each of the three row
// reductions) measured 0.247 -> 0.149 ms without and 0.308 -> 0.232 ms with the gradient at c4 (2 M x 64); 16 was slower
// again (0.17 / 0.28 ms).  Four per lane remains for C <= 16, and for the wide path (C > 256: the row is streamed).
template <class F>
void ce_dispatch(int C, bool v4, F &&f) {
    auto leaf = [&](auto lpr, auto kpl) {
        if (v4)
            f(lpr, kpl, std::true_type{});
        else
            f(lpr, kpl, std::false_type{});
    };
    using std::integral_constant;
    if (C <= 16)
        leaf(integral_constant<int, 4>{}, integral_constant<int, 4>{});
    else if (C <= 32)
        leaf(integral_constant<int, 4>{}, integral_constant<int, 8>{});
    else if (C <= 64)
        leaf(integral_constant<int, 8>{}, integral_constant<int, 8>{});
    else if (C <= 128)
        leaf(integral_constant<int, 16>{}, integral_constant<int, 8>{});
    else if (C <= 256)
        leaf(integral_constant<int, 32>{}, integral_constant<int, 8>{});
    else
        leaf(integral_constant<int, 64>{}, integral_constant<int, 4>{});
}

// workgroups of a launch: one per rows_per_block = UN (2 row groups) x 4 waves x 64 / LPR rows, at most `cap`
inline int ce_grid(int64_t n_rows, int lpr, int cap) {
    const int64_t rows_per_block = 2 * 4 * (64 / lpr);
    return static_cast<int>(std::min<int64_t>(cap, std::max<int64_t>(1, (n_rows + rows_per_block - 1) / rows_per_block)));
}

// 16-byte accesses: every row of the logits (and of the gradient, when there is one) starts on a 16-byte boundary;
// `width` is what a lane's consecutive columns must tile (the class count, or the segment stride of a member)
inline bool ce_v4(int width, const float *logits, int64_t ld, const float *dlogits, int64_t ldd) {
    return width % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
           (!dlogits || (ldd % 4 == 0 && reinterpret_cast<uintptr_t>(dlogits) % 16 == 0));
}

// ---- device: the rows of one workgroup -----------------------------------------------------------------------------
// LPR lanes cooperate on one row; a wave handles 64/LPR rows at a time, two such groups per loop
// iteration (independent dependency chains: the kernel is instruction- and latency-bound, not bandwidth-bound).
// For C <= KPL * LPR (the launcher's choice for C <= 256) a lane keeps its <= KPL logits in registers: one read
// of the row, one expf per element, shared by the loss and the gradient.
// V4 (16-byte aligned rows whose width is a multiple of 4): the lane's KPL logits are CONSECUTIVE columns -- 16-byte
// loads and stores; otherwise they are LPR columns apart (4-byte accesses).
// rows.colpart != nullptr (register path only): the workgroup also leaves the column sums of the gradient rows it
// wrote -- the bias gradient of the layer that produced the logits -- in rows.colpart_row()[0..C).
//
// `Rows` supplies
//   C, n_rows, target, inv_count, dlogits, colpart      the class count, the row count, the labels, the divisor of the
//                                                       mean, and whether a gradient / its column sums are wanted
//   selected(r), row(r), drow(r)                        is row r part of the loss; its C logits; its gradient row
//   want_pred(), set_pred(r, c)                         the arg-max of every row, selected or not
//   partial_slot(), colpart_row()                       where the workgroup leaves its loss partial and column sums
//   kPadded, width()                                    kPadded: the row owns width() >= C columns, those in [C, width())
//                                                       are pad -- read as -inf (a 16-byte load may straddle C), never
//                                                       the arg-max, zero in the gradient.  Otherwise width() == C and
//                                                       none of that is compiled.
template <int LPR, bool V4, int KPL, class Rows>
__device__ __forceinline__ void ce_rows(const Rows &rows) {
    constexpr int RPW = 64 / LPR;
    static_assert(KPL == 4 || KPL == 8, "logits per lane on the register path");
    constexpr int UN = 2;        // row groups in flight per wave
    constexpr bool kPadded = Rows::kPadded;
    __shared__ float red[4];
    __shared__ float cred[4][LPR * KPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPR, sl = lane % LPR;
    const int C = rows.C;
    const int64_t n_rows = rows.n_rows;
    const float inv_count = rows.inv_count;
    const int64_t rows_per_iter = int64_t(gridDim.x) * 4 * RPW * UN;
    const bool in_regs = C <= KPL * LPR;
    const bool want_pred = rows.want_pred();
    auto col = [&](int k) { return V4 ? sl * KPL + k : sl + k * LPR; };
    float loss = 0.f;
    float cs[KPL];
#pragma unroll
    for (int k = 0; k < KPL; ++k) cs[k] = 0.f;
    for (int64_t r0 = (int64_t(blockIdx.x) * 4 + wave) * RPW * UN; r0 < n_rows; r0 += rows_per_iter) {
        if (in_regs) {
            float x[UN][KPL];
            bool on[UN], valid[UN];
            int64_t r[UN], t[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                r[u] = r0 + u * RPW + sub;
                valid[u] = r[u] < n_rows;
                on[u] = valid[u] && rows.selected(r[u]);
                const float *row = rows.row(valid[u] ? r[u] : 0);
                t[u] = on[u] ? rows.target[r[u]] : 0;
                const bool need = on[u] || (want_pred && valid[u]);
                if constexpr (V4) {
#pragma unroll
                    for (int q = 0; q < KPL / 4; ++q) {
                        const int c0 = sl * KPL + 4 * q;
                        float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                        if (need && c0 < C) v = *reinterpret_cast<const float4 *>(row + c0);   // (c0 + 3 < width(): a multiple of 4)
                        if constexpr (kPadded) {
                            if (c0 + 1 >= C) v.y = -INFINITY;
                            if (c0 + 2 >= C) v.z = -INFINITY;
                            if (c0 + 3 >= C) v.w = -INFINITY;
                        }
                        x[u][4 * q] = v.x, x[u][4 * q + 1] = v.y, x[u][4 * q + 2] = v.z, x[u][4 * q + 3] = v.w;
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
                    // arg-max of the row (first index on ties), for every row, selected or not
                    int bi = INT32_MAX;
#pragma unroll
                    for (int k = KPL - 1; k >= 0; --k)
                        if (x[u][k] == m && (!kPadded || col(k) < C)) bi = col(k);
#pragma unroll
                    for (int off = LPR / 2; off > 0; off >>= 1) bi = min(bi, __shfl_xor(bi, off, 64));
                    if (valid[u] && sl == 0) rows.set_pred(r[u], bi == INT32_MAX ? 0 : bi);
                }
                // The target's term is kept out of the sum of the others: the gradient at the target is
                // p_t - 1 = -(sum of the others) / sum, which `e_t / sum - 1.f` would round to a multiple of 2^-24 --
                // the whole gradient row of a confident sample (p_t -> 1) is of that size or smaller.
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
                    // the lane that holds the target logit adds the row's loss term, log(sum) - (x_t - m): the
                    // difference first, so that a row at +-1e4 does not round its loss to the spacing of fp32 there
                    const float lsum = logf(sum);
#pragma unroll
                    for (int k = 0; k < KPL; ++k)
                        if (col(k) == t[u]) loss += lsum - (x[u][k] - m);
                    // a class index outside [0, C) poisons the loss instead of being dropped silently
                    // (torch raises; the Python wrapper checks the labels once per tensor)
                    if (sl == 0 && (t[u] < 0 || t[u] >= C)) loss = NAN;
                }
                if (rows.dlogits != nullptr && valid[u]) {
                    float *drow = rows.drow(r[u]);
                    const int W = rows.width();
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
                            if (sl * KPL + 4 * q < W)
                                *reinterpret_cast<float4 *>(drow + sl * KPL + 4 * q) =
                                    make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
                        if constexpr (kPadded)
                            for (int c = LPR * KPL + 4 * sl; c < W; c += 4 * LPR)          // pad beyond the lanes' columns
                                *reinterpret_cast<float4 *>(drow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
                    } else {
#pragma unroll
                        for (int k = 0; k < KPL; ++k)
                            if (col(k) < W) drow[col(k)] = d[k];
                        if constexpr (kPadded)
                            for (int c = LPR * KPL + sl; c < W; c += LPR) drow[c] = 0.f;
                    }
                }
            }
        } else {
            for (int u = 0; u < UN; ++u) {
                const int64_t r = r0 + u * RPW + sub;
                const bool valid = r < n_rows;
                const bool on = valid && rows.selected(r);
                const float *row = rows.row(valid ? r : 0);
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
                    if (valid && sl == 0) rows.set_pred(r, bi == INT32_MAX ? 0 : bi);
                }
                // as on the register path: the target's term apart from the sum of the others, differences from the
                // row maximum before anything is added to log(sum)
                const int64_t t = on ? rows.target[r] : 0;
                const bool t_ok = on && t >= 0 && t < C;   // no read outside the row (see above)
                const float xt = t_ok ? row[t] - m : 0.f;
                float s = 0.f;
                if (on)
                    for (int c = sl; c < C; c += LPR)
                        if (c != t) s += expf(row[c] - m);
#pragma unroll
                for (int off = LPR / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
                const float sum = s + (t_ok ? expf(xt) : 0.f);
                // an invalid class index poisons the loss
                if (on && sl == 0) loss += t_ok ? logf(sum) - xt : NAN;
                if (rows.dlogits != nullptr && valid) {
                    float *drow = rows.drow(r);
                    const float inv = on ? 1.f / sum : 0.f;
                    for (int c = sl; c < C; c += LPR)
                        drow[c] = on ? (c == t ? -(s * inv) : expf(row[c] - m) * inv) * inv_count : 0.f;
                    if constexpr (kPadded)
                        for (int c = C + sl; c < rows.width(); c += LPR) drow[c] = 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) loss += __shfl_xor(loss, off, 64);
    if (lane == 0) red[wave] = loss;
    if (rows.colpart != nullptr) {
        // column sums of the gradient rows: the sub-groups of a wave, then the four waves, in a fixed order
#pragma unroll
        for (int k = 0; k < KPL; ++k) {
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) cs[k] += __shfl_xor(cs[k], off, 64);
            if (sub == 0) cred[wave][sl * KPL + k] = cs[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *rows.partial_slot() = (red[0] + red[1]) + (red[2] + red[3]);
    if (rows.colpart != nullptr && wave == 0 && sub == 0) {
        float *out = rows.colpart_row();
#pragma unroll
        for (int k = 0; k < KPL; ++k) {
            const int c = col(k), i = sl * KPL + k;
            if (c < C) out[c] = (cred[0][i] + cred[1][i]) + (cred[2][i] + cred[3][i]);
        }
    }
}

}  // namespace tgcn
