// JumpingKnowledge(mode="lstm") of the reference's JumpingKnowledgeNetwork (textgcn/lib/models.py:64,75; PyG 1.6.3
// jumping_knowledge.py): a bidirectional LSTM (hidden width H = L C / 2) over the L per-layer activations x_t [N, C] of every
// node, a Linear(2 H -> 1) on [h_fwd_t | h_bwd_t], a softmax over the layers and the weighted sum
//     alpha[i, :] = softmax_t(att_w . [h_fwd_t(i) | h_bwd_t(i)] + att_b),      out[i, :] = sum_t alpha[i, t] x_t[i, :].
// torch's parameter layout throughout: W_ih [4 H, C], W_hh [4 H, H], gate order i, f, g, o.
//
//   tgcn_jk_lstm_forward   the whole step as ONE kernel: a wave owns 32 nodes and carries them through both directions and
//                          all L steps on v_mfma_f32_32x32x2_f32 (exact fp32; fragment maps: fused_act.h).
//                          Only out [N, C] and alpha [N, L] reach memory: no gate, cell or hidden value does.
//   tgcn_jk_cell, tgcn_jk_attention                          the same arithmetic as pointwise pieces around the library's
//   tgcn_jk_attention_grad, tgcn_jk_cell_grad,               tall-skinny products: the composed forward and the backward by
//   tgcn_jk_input_grad                                       recomputation in row chunks (pytextgcn_amd/jk.py).
// No atomics anywhere: every sum has a fixed order.
#include <algorithm>
#include <type_traits>

#include "fused_act.h"

namespace tgcn {
namespace {

struct JkInputs {
    const float *x[TGCN_JK_MAX_LAYERS];
    int64_t ld[TGCN_JK_MAX_LAYERS];
};

struct JkDir {
    const float *wih, *whh, *bih, *bhh;
};

// the accurate forms: expf / tanhf, no fast-math intrinsics (the bar is 1e-5 against float64 through L recurrent steps)
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// f(integral_constant<0>) ... f(integral_constant<N - 1>): a loop whose index is a constant in every copy of the body (the
// cell state is a register array indexed by it; an `unroll` pragma the compiler may decline would put it in scratch)
template <int J, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>{});
        static_for<J + 1, N>(f);
    }
}

constexpr int kGateCols = 128;   // one block of 32 hidden units x the 4 gates
constexpr int kLdW = 33;         // odd stride of the staged weight chunk: neither the staging writes nor the operand reads conflict
constexpr int kMaxHiddenBlocks = 8;

// ---------------------------------------------------------------------------------------------
// The fused forward.  The 4 H gate columns do not fit the registers at H = 200 (25 accumulator tiles), so they go in
// passes of 32 hidden units: the i, f, g and o tiles of those units (4 accumulators), reduced over [x_t | h_{t-1}], then
// the cell update of exactly those units.  c lives in registers in the accumulator layout (NHB x 16 per lane); h_t is
// needed as the A operand of the next step (row = node per lane), which is the transpose of the accumulator layout, so
// it goes through the wave's own LDS, double buffered (every pass of step t reads all of h_{t-1}).  The weights do not
// fit LDS (4 x 640 KB at C = H = 200): the workgroup's waves walk (direction, step, pass, k chunk) in lockstep and share a
// staged [128 gate columns x 32 k] chunk.  The attention score of (node, t) is summed from the h_t that was just written
// to LDS, forward direction first, then the reverse one: a fixed order.
// ---------------------------------------------------------------------------------------------
template <int NHB>
__global__ __launch_bounds__(256, 1) void k_jk_fwd(const JkInputs xs, int L, int64_t N, int C, int H, const JkDir d0,
                                                   const JkDir d1, int64_t ldwi, int64_t ldwh, const float *__restrict__ aw,
                                                   const float *__restrict__ ab, float *__restrict__ out, int64_t ldo,
                                                   float *__restrict__ alpha, int64_t lda, int relu) {
    extern __shared__ float jk_lds[];
    const int tid = threadIdx.x, nthreads = blockDim.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, c = lane & 31;
    const int HS = H | 1;                                   // odd row stride of the h tiles
    float *Ws = jk_lds;                                     // [128][33]
    float *mine = jk_lds + kGateCols * kLdW + wave * (2 * 32 * HS + 32 * TGCN_JK_MAX_LAYERS);
    float *hprev = mine, *hnew = mine + 32 * HS;
    float *sc = mine + 2 * 32 * HS;                         // [32 nodes][8]: scores, then alpha
    const int64_t row0 = (int64_t(blockIdx.x) * (nthreads >> 6) + wave) * 32;
    const int64_t i = row0 + c;
    const bool live = i < N;
    const int64_t ic = live ? i : 0;
    float cst[NHB * 16];
#pragma unroll
    for (int q = 0; q < NHB * 16; ++q) cst[q] = 0.f;
    const int cx = (C + 31) / 32, ch = (H + 31) / 32;

    for (int dir = 0; dir < 2; ++dir) {
        const JkDir w = dir ? d1 : d0;
        for (int step = 0; step < L; ++step) {
            const int t = dir ? L - 1 - step : step;
            const float *x = xs.x[t];
            const int64_t ldx = xs.ld[t];
            const bool first = step == 0;                   // h = c = 0: no recurrent product
            const int chunks = first ? cx : cx + ch;
            static_for<0, NHB>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                f32x16 acc[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
                for (int q = 0; q < chunks; ++q) {
                    const bool xpart = q < cx;
                    const int k0 = 32 * (xpart ? q : q - cx), K = xpart ? C : H;
                    const float *W = xpart ? w.wih : w.whh;
                    const int64_t ldw = xpart ? ldwi : ldwh;
                    __syncthreads();                        // the previous chunk has been read
                    for (int e = tid; e < kGateCols * 32; e += nthreads) {
                        const int col = e >> 5, kk = e & 31, hcol = j * 32 + (col & 31), k = k0 + kk;
                        Ws[col * kLdW + kk] = (hcol < H && k < K) ? W[(int64_t(col >> 5) * H + hcol) * ldw + k] : 0.f;
                    }
                    float a[16];
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const int k = k0 + 2 * s + half;
                        if (xpart) a[s] = (live && k < C) ? x[ic * ldx + k] : 0.f;
                        else a[s] = k < H ? hprev[c * HS + k] : 0.f;
                    }
                    __syncthreads();
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const int kk = 2 * s + half;
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], Ws[(g * 32 + c) * kLdW + kk], acc[g], 0, 0, 0);
                    }
                }
                // the cell update of hidden units [32 j, 32 j + 32): lane (c, half) holds 16 nodes of unit 32 j + c
                const int col = j * 32 + c;
                const bool colok = col < H;
                const int cc = colok ? col : 0;
                const float bi = w.bih[cc] + w.bhh[cc], bf = w.bih[H + cc] + w.bhh[H + cc];
                const float bg = w.bih[2 * H + cc] + w.bhh[2 * H + cc], bo = w.bih[3 * H + cc] + w.bhh[3 * H + cc];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float ig = sigmoid_f(acc[0][r] + bi), fg = sigmoid_f(acc[1][r] + bf);
                    const float gg = tanhf(acc[2][r] + bg), og = sigmoid_f(acc[3][r] + bo);
                    const float cn = (first ? 0.f : fg * cst[j * 16 + r]) + ig * gg;
                    cst[j * 16 + r] = cn;
                    if (colok) hnew[acc_row(r, half) * HS + col] = og * tanhf(cn);
                }
            });
            __syncthreads();                                // h_t is complete
            float p = 0.f;
            for (int k = half; k < H; k += 2) p += hnew[c * HS + k] * aw[dir * H + k];
            p += __shfl_xor(p, 32);
            if (half == 0) sc[c * TGCN_JK_MAX_LAYERS + t] = dir == 0 ? p : sc[c * TGCN_JK_MAX_LAYERS + t] + p;
            float *swap = hprev;
            hprev = hnew;
            hnew = swap;
        }
    }
    __syncthreads();
    if (half == 0) {                                        // softmax over the layers of node c
        float *s = sc + c * TGCN_JK_MAX_LAYERS;
        const float b = ab[0];
        float m = -INFINITY, sum = 0.f;
        for (int t = 0; t < L; ++t) m = fmaxf(m, s[t] + b);
        for (int t = 0; t < L; ++t) sum += expf(s[t] + b - m);
        for (int t = 0; t < L; ++t) {
            const float av = expf(s[t] + b - m) / sum;
            s[t] = av;
            if (live) alpha[i * lda + t] = av;
        }
    }
    __syncthreads();
    for (int row = 0; row < 32; ++row) {
        const int64_t node = row0 + row;
        if (node >= N) break;
        for (int col = lane; col < C; col += 64) {
            float v = 0.f;
            for (int t = 0; t < L; ++t) v += sc[row * TGCN_JK_MAX_LAYERS + t] * xs.x[t][node * xs.ld[t] + col];
            out[node * ldo + col] = relu ? fmaxf(v, 0.f) : v;
        }
    }
}

size_t fwd_lds_bytes(int H, int waves) {
    return sizeof(float) * (size_t(kGateCols) * kLdW + size_t(waves) * (2 * 32 * size_t(H | 1) + 32 * TGCN_JK_MAX_LAYERS));
}

constexpr size_t kLdsLimit = 160 * 1024;

// waves per workgroup of the fused forward for hidden width H (0: the kernel does not take this width)
int fwd_waves(int H) {
    if ((H + 31) / 32 > kMaxHiddenBlocks) return 0;
    for (int w = 4; w >= 1; w >>= 1)
        if (fwd_lds_bytes(H, w) <= kLdsLimit) return w;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The pointwise pieces.  One thread per (row, hidden unit) / (row, column); one wave per row where a row is reduced.
// ---------------------------------------------------------------------------------------------
// gates <- (sigmoid, sigmoid, tanh, sigmoid)(pre_x + pre_h + b_ih + b_hh), c = f c_prev + i g, h = o tanh(c).  `gates` may
// be `pre_x` itself: a thread reads its four pre-activations before it writes them.
__global__ __launch_bounds__(256) void k_jk_cell(const float *pre_x, int64_t ldpx, const float *pre_h, int64_t ldph,
                                                 const float *__restrict__ bih, const float *__restrict__ bhh,
                                                 const float *__restrict__ c_prev, int64_t ldcp, float *gates, int64_t ldg,
                                                 float *__restrict__ cout, int64_t ldc, float *__restrict__ hout, int64_t ldh,
                                                 int64_t R, int H) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= R * H) return;
    const int64_t row = e / H;
    const int col = static_cast<int>(e % H);
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        z[g] = pre_x[row * ldpx + g * H + col] + (bih[g * H + col] + bhh[g * H + col]);
        if (pre_h) z[g] += pre_h[row * ldph + g * H + col];
    }
    const float ig = sigmoid_f(z[0]), fg = sigmoid_f(z[1]), gg = tanhf(z[2]), og = sigmoid_f(z[3]);
    const float cn = (c_prev ? fg * c_prev[row * ldcp + col] : 0.f) + ig * gg;
    float *gr = gates + row * ldg + col;
    gr[0] = ig;
    gr[H] = fg;
    gr[2 * H] = gg;
    gr[3 * H] = og;
    cout[row * ldc + col] = cn;
    hout[row * ldh + col] = og * tanhf(cn);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// scores, softmax and the weighted sum for stored hidden states: hf / hb + t * hstep is h_t [R, H] of the direction
__global__ __launch_bounds__(256) void k_jk_attention(const JkInputs xs, int L, int64_t R, int C, int H,
                                                      const float *__restrict__ hf, const float *__restrict__ hb, int64_t ldh,
                                                      int64_t hstep, const float *__restrict__ aw, const float *__restrict__ ab,
                                                      float *__restrict__ out, int64_t ldo, float *__restrict__ alpha,
                                                      int64_t lda, int relu) {
    __shared__ float sc[4][TGCN_JK_MAX_LAYERS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = int64_t(blockIdx.x) * 4 + wave;
    if (row >= R) return;                                   // (whole waves leave; no barrier below)
    const float b = ab[0];
    float m = -INFINITY;
    for (int t = 0; t < L; ++t) {
        const float *f = hf + t * hstep + row * ldh, *r = hb + t * hstep + row * ldh;
        float p = 0.f, q = 0.f;
        for (int k = lane; k < H; k += 64) {
            p += f[k] * aw[k];
            q += r[k] * aw[H + k];
        }
        const float s = wave_sum(p) + wave_sum(q) + b;
        m = fmaxf(m, s);
        if (lane == 0) sc[wave][t] = s;
    }
    float sum = 0.f;
    for (int t = 0; t < L; ++t) sum += expf(sc[wave][t] - m);
    for (int t = 0; t < L; ++t) {
        const float av = expf(sc[wave][t] - m) / sum;       // (every lane computes the same value)
        if (lane == 0) alpha[row * lda + t] = av;
    }
    for (int col = lane; col < C; col += 64) {
        float v = 0.f;
        for (int t = 0; t < L; ++t) v += (expf(sc[wave][t] - m) / sum) * xs.x[t][row * xs.ld[t] + col];
        out[row * ldo + col] = relu ? fmaxf(v, 0.f) : v;
    }
}

// G' = G where out > 0 (relu) or G;  d alpha_t = G' . x_t;  d score_t = alpha_t (d alpha_t - sum_s alpha_s d alpha_s)
__global__ __launch_bounds__(256) void k_jk_attention_grad(const JkInputs xs, int L, int64_t R, int C,
                                                           const float *__restrict__ G, int64_t ldg,
                                                           const float *__restrict__ out, int64_t ldo,
                                                           const float *__restrict__ alpha, int64_t lda,
                                                           float *__restrict__ dscore, int64_t ldds) {
    __shared__ float da[4][TGCN_JK_MAX_LAYERS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = int64_t(blockIdx.x) * 4 + wave;
    if (row >= R) return;
    float dot = 0.f;
    for (int t = 0; t < L; ++t) {
        float p = 0.f;
        for (int col = lane; col < C; col += 64) {
            const float g = (!out || out[row * ldo + col] > 0.f) ? G[row * ldg + col] : 0.f;
            p += g * xs.x[t][row * xs.ld[t] + col];
        }
        p = wave_sum(p);
        dot += alpha[row * lda + t] * p;
        if (lane == 0) da[wave][t] = p;
    }
    if (lane < L) dscore[row * ldds + lane] = alpha[row * lda + lane] * (da[wave][lane] - dot);
}

// One step of the LSTM's backward at the pre-activations.  d h_t = dh_rec + d score_t att_w (the attention reads h_t);
// dc holds d c_t coming from step t + 1 (`dc_zero`: nothing yet) and leaves as d c_{t-1}.
__global__ __launch_bounds__(256) void k_jk_cell_grad(const float *__restrict__ gates, int64_t ldg, const float *__restrict__ cs,
                                                      int64_t ldc, const float *__restrict__ c_prev, int64_t ldcp,
                                                      const float *__restrict__ dh_rec, int64_t lddh,
                                                      const float *__restrict__ dscore, int64_t ldds,
                                                      const float *__restrict__ aw, float *__restrict__ dc, int64_t lddc,
                                                      int dc_zero, float *__restrict__ dgates, int64_t lddg, int64_t R, int H) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= R * H) return;
    const int64_t row = e / H;
    const int col = static_cast<int>(e % H);
    const float *gr = gates + row * ldg + col;
    const float ig = gr[0], fg = gr[H], gg = gr[2 * H], og = gr[3 * H];
    const float dh = (dh_rec ? dh_rec[row * lddh + col] : 0.f) + dscore[row * ldds] * aw[col];
    const float tc = tanhf(cs[row * ldc + col]);
    const float dcn = (dc_zero ? 0.f : dc[row * lddc + col]) + dh * og * (1.f - tc * tc);
    const float cp = c_prev ? c_prev[row * ldcp + col] : 0.f;
    float *dg = dgates + row * lddg + col;
    dg[0] = dcn * gg * ig * (1.f - ig);
    dg[H] = dcn * cp * fg * (1.f - fg);
    dg[2 * H] = dcn * ig * (1.f - gg * gg);
    dg[3 * H] = dh * tc * og * (1.f - og);
    dc[row * lddc + col] = dcn * fg;
}

// d x_t = alpha_t G' + T   (T: the LSTM's part, d gates_t @ W_ih of both directions)
__global__ __launch_bounds__(256) void k_jk_input_grad(float *__restrict__ dx, int64_t lddx, const float *__restrict__ T,
                                                       int64_t ldt, const float *__restrict__ G, int64_t ldg,
                                                       const float *__restrict__ out, int64_t ldo,
                                                       const float *__restrict__ alpha, int64_t lda, int64_t R, int C) {
    const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (e >= R * C) return;
    const int64_t row = e / C;
    const int col = static_cast<int>(e % C);
    const float g = (!out || out[row * ldo + col] > 0.f) ? G[row * ldg + col] : 0.f;
    dx[row * lddx + col] = alpha[row * lda] * g + T[row * ldt + col];
}

int check_widths(const char *fn, int64_t R, int a, int b) {
    if (R < 0 || a <= 0 || b <= 0) {
        set_error("%s: need a row count >= 0 and widths >= 1 (rows=%lld, widths %d, %d)", fn, (long long)R, a, b);
        return TGCN_E_INVALID;
    }
    return TGCN_OK;
}

// the L inputs: host arrays of device pointers and leading dimensions
int gather_inputs(const char *fn, const float *const *xs, const int64_t *ldxs, int L, int64_t R, int C, JkInputs &in) {
    if (L < 1 || L > TGCN_JK_MAX_LAYERS) {
        set_error("%s: %d layers; 1 .. TGCN_JK_MAX_LAYERS = %d are taken", fn, L, TGCN_JK_MAX_LAYERS);
        return TGCN_E_INVALID;
    }
    TGCN_CHECK(check_ptr(fn, "xs", xs));
    TGCN_CHECK(check_ptr(fn, "ldxs", ldxs));
    for (int t = 0; t < TGCN_JK_MAX_LAYERS; ++t) {
        in.x[t] = nullptr;
        in.ld[t] = 0;
    }
    for (int t = 0; t < L; ++t) {
        TGCN_CHECK(check_ld(fn, "ldxs[t]", ldxs[t], C));
        if (R > 0) TGCN_CHECK(check_ptr(fn, "xs[t]", xs[t]));
        in.x[t] = xs[t];
        in.ld[t] = ldxs[t];
    }
    return TGCN_OK;
}

unsigned grid_of(int64_t elements) { return static_cast<unsigned>((elements + 255) / 256); }

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_jk_lstm_forward_supported(int H) { return tgcn::fwd_waves(H) > 0 ? 1 : 0; }

int tgcn_jk_lstm_forward(const float *const *xs, const int64_t *ldxs, int L, int64_t N, int C, int H,
                         const float *const *lstm, int64_t ldwi, int64_t ldwh, const float *att_w, const float *att_b,
                         float *out, int64_t ldo, float *alpha, int64_t lda, int relu, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_jk_lstm_forward";
    TGCN_CHECK(check_widths(fn, N, C, H));
    JkInputs in;
    TGCN_CHECK(gather_inputs(fn, xs, ldxs, L, N, C, in));
    TGCN_CHECK(check_ld(fn, "ldwi", ldwi, C));
    TGCN_CHECK(check_ld(fn, "ldwh", ldwh, H));
    TGCN_CHECK(check_ld(fn, "ldo", ldo, C));
    TGCN_CHECK(check_ld(fn, "lda", lda, L));
    const int waves = fwd_waves(H);
    if (waves == 0) {
        set_error("%s: hidden width %d is beyond the fused kernel (at most %d); run the composed pieces", fn, H,
                  32 * kMaxHiddenBlocks);
        return TGCN_E_INVALID;
    }
    if (N == 0) return TGCN_OK;
    TGCN_CHECK(check_ptr(fn, "lstm", lstm));
    for (int q = 0; q < 8; ++q) TGCN_CHECK(check_ptr(fn, "lstm[q]", lstm[q]));
    TGCN_CHECK(check_ptr(fn, "att_w", att_w));
    TGCN_CHECK(check_ptr(fn, "att_b", att_b));
    TGCN_CHECK(check_ptr(fn, "out", out));
    TGCN_CHECK(check_ptr(fn, "alpha", alpha));
    const JkDir d0{lstm[0], lstm[1], lstm[2], lstm[3]}, d1{lstm[4], lstm[5], lstm[6], lstm[7]};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = fwd_lds_bytes(H, waves);
    const unsigned grid = static_cast<unsigned>((N + 32 * waves - 1) / (32 * waves));
#define TGCN_JK_FWD(NHB)                                                                                              \
    do {                                                                                                              \
        TGCN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_jk_fwd<NHB>),                            \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsLimit))); \
        hipLaunchKernelGGL((k_jk_fwd<NHB>), dim3(grid), dim3(64 * waves), lds, s, in, L, N, C, H, d0, d1, ldwi, ldwh, \
                           att_w, att_b, out, ldo, alpha, lda, relu);                                                 \
    } while (0)
    switch ((H + 31) / 32) {
        case 1: TGCN_JK_FWD(1); break;
        case 2: TGCN_JK_FWD(2); break;
        case 3: TGCN_JK_FWD(3); break;
        case 4: TGCN_JK_FWD(4); break;
        case 5: TGCN_JK_FWD(5); break;
        case 6: TGCN_JK_FWD(6); break;
        case 7: TGCN_JK_FWD(7); break;
        default: TGCN_JK_FWD(8); break;
    }
#undef TGCN_JK_FWD
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

int tgcn_jk_cell(const float *pre_x, int64_t ldpx, const float *pre_h, int64_t ldph, const float *b_ih, const float *b_hh,
                 const float *c_prev, int64_t ldcp, float *gates, int64_t ldg, float *c, int64_t ldc, float *h, int64_t ldh,
                 int64_t R, int H, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_jk_cell";
    TGCN_CHECK(check_widths(fn, R, H, H));
    TGCN_CHECK(check_ld(fn, "ldpx", ldpx, 4 * int64_t(H)));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, 4 * int64_t(H)));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, H));
    TGCN_CHECK(check_ld(fn, "ldh", ldh, H));
    if (pre_h) TGCN_CHECK(check_ld(fn, "ldph", ldph, 4 * int64_t(H)));
    if (c_prev) TGCN_CHECK(check_ld(fn, "ldcp", ldcp, H));
    if (R == 0) return TGCN_OK;
    TGCN_CHECK(check_ptr(fn, "pre_x", pre_x));
    TGCN_CHECK(check_ptr(fn, "b_ih", b_ih));
    TGCN_CHECK(check_ptr(fn, "b_hh", b_hh));
    TGCN_CHECK(check_ptr(fn, "gates", gates));
    TGCN_CHECK(check_ptr(fn, "c", c));
    TGCN_CHECK(check_ptr(fn, "h", h));
    hipLaunchKernelGGL(k_jk_cell, dim3(grid_of(R * H)), dim3(256), 0, static_cast<hipStream_t>(stream), pre_x, ldpx, pre_h,
                       ldph, b_ih, b_hh, c_prev, ldcp, gates, ldg, c, ldc, h, ldh, R, H);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

int tgcn_jk_attention(const float *const *xs, const int64_t *ldxs, int L, int64_t R, int C, int H, const float *h_fwd,
                      const float *h_bwd, int64_t ldh, int64_t hstep, const float *att_w, const float *att_b, float *out,
                      int64_t ldo, float *alpha, int64_t lda, int relu, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_jk_attention";
    TGCN_CHECK(check_widths(fn, R, C, H));
    JkInputs in;
    TGCN_CHECK(gather_inputs(fn, xs, ldxs, L, R, C, in));
    TGCN_CHECK(check_ld(fn, "ldh", ldh, H));
    TGCN_CHECK(check_ld(fn, "ldo", ldo, C));
    TGCN_CHECK(check_ld(fn, "lda", lda, L));
    if (hstep < 0) {
        set_error("%s: hstep must be >= 0", fn);
        return TGCN_E_INVALID;
    }
    if (R == 0) return TGCN_OK;
    TGCN_CHECK(check_ptr(fn, "h_fwd", h_fwd));
    TGCN_CHECK(check_ptr(fn, "h_bwd", h_bwd));
    TGCN_CHECK(check_ptr(fn, "att_w", att_w));
    TGCN_CHECK(check_ptr(fn, "att_b", att_b));
    TGCN_CHECK(check_ptr(fn, "out", out));
    TGCN_CHECK(check_ptr(fn, "alpha", alpha));
    hipLaunchKernelGGL(k_jk_attention, dim3(static_cast<unsigned>((R + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       in, L, R, C, H, h_fwd, h_bwd, ldh, hstep, att_w, att_b, out, ldo, alpha, lda, relu);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

int tgcn_jk_attention_grad(const float *const *xs, const int64_t *ldxs, int L, int64_t R, int C, const float *G, int64_t ldg,
                           const float *out, int64_t ldo, const float *alpha, int64_t lda, float *dscore, int64_t ldds,
                           tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_jk_attention_grad";
    TGCN_CHECK(check_widths(fn, R, C, C));
    JkInputs in;
    TGCN_CHECK(gather_inputs(fn, xs, ldxs, L, R, C, in));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, C));
    if (out) TGCN_CHECK(check_ld(fn, "ldo", ldo, C));
    TGCN_CHECK(check_ld(fn, "lda", lda, L));
    TGCN_CHECK(check_ld(fn, "ldds", ldds, L));
    if (R == 0) return TGCN_OK;
    TGCN_CHECK(check_ptr(fn, "G", G));
    TGCN_CHECK(check_ptr(fn, "alpha", alpha));
    TGCN_CHECK(check_ptr(fn, "dscore", dscore));
    hipLaunchKernelGGL(k_jk_attention_grad, dim3(static_cast<unsigned>((R + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), in, L, R, C, G, ldg, out, ldo, alpha, lda, dscore, ldds);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

int tgcn_jk_cell_grad(const float *gates, int64_t ldg, const float *c, int64_t ldc, const float *c_prev, int64_t ldcp,
                      const float *dh_rec, int64_t lddh, const float *dscore_t, int64_t ldds, const float *att_w_dir, float *dc,
                      int64_t lddc, int dc_zero, float *dgates, int64_t lddg, int64_t R, int H, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_jk_cell_grad";
    TGCN_CHECK(check_widths(fn, R, H, H));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, 4 * int64_t(H)));
    TGCN_CHECK(check_ld(fn, "lddg", lddg, 4 * int64_t(H)));
    TGCN_CHECK(check_ld(fn, "ldc", ldc, H));
    TGCN_CHECK(check_ld(fn, "lddc", lddc, H));
    TGCN_CHECK(check_ld(fn, "ldds", ldds, 1));
    if (c_prev) TGCN_CHECK(check_ld(fn, "ldcp", ldcp, H));
    if (dh_rec) TGCN_CHECK(check_ld(fn, "lddh", lddh, H));
    if (R == 0) return TGCN_OK;
    TGCN_CHECK(check_ptr(fn, "gates", gates));
    TGCN_CHECK(check_ptr(fn, "c", c));
    TGCN_CHECK(check_ptr(fn, "dscore_t", dscore_t));
    TGCN_CHECK(check_ptr(fn, "att_w_dir", att_w_dir));
    TGCN_CHECK(check_ptr(fn, "dc", dc));
    TGCN_CHECK(check_ptr(fn, "dgates", dgates));
    hipLaunchKernelGGL(k_jk_cell_grad, dim3(grid_of(R * H)), dim3(256), 0, static_cast<hipStream_t>(stream), gates, ldg, c, ldc,
                       c_prev, ldcp, dh_rec, lddh, dscore_t, ldds, att_w_dir, dc, lddc, dc_zero, dgates, lddg, R, H);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

int tgcn_jk_input_grad(float *dx, int64_t lddx, const float *T, int64_t ldt, const float *G, int64_t ldg, const float *out,
                       int64_t ldo, const float *alpha_t, int64_t lda, int64_t R, int C, tgcn_stream stream) {
    using namespace tgcn;
    const char *fn = "tgcn_jk_input_grad";
    TGCN_CHECK(check_widths(fn, R, C, C));
    TGCN_CHECK(check_ld(fn, "lddx", lddx, C));
    TGCN_CHECK(check_ld(fn, "ldt", ldt, C));
    TGCN_CHECK(check_ld(fn, "ldg", ldg, C));
    if (out) TGCN_CHECK(check_ld(fn, "ldo", ldo, C));
    TGCN_CHECK(check_ld(fn, "lda", lda, 1));
    if (R == 0) return TGCN_OK;
    TGCN_CHECK(check_ptr(fn, "dx", dx));
    TGCN_CHECK(check_ptr(fn, "T", T));
    TGCN_CHECK(check_ptr(fn, "G", G));
    TGCN_CHECK(check_ptr(fn, "alpha_t", alpha_t));
    hipLaunchKernelGGL(k_jk_input_grad, dim3(grid_of(R * C)), dim3(256), 0, static_cast<hipStream_t>(stream), dx, lddx, T, ldt,
                       G, ldg, out, ldo, alpha_t, lda, R, C);
    TGCN_HIP_CHECK(hipGetLastError());
    return TGCN_OK;
}

}  // extern "C"
