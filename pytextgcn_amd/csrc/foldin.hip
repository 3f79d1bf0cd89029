// tgcn_foldin_two_layer -- the logits of documents that are not nodes of the training graph (include/tgcn.h; DESIGN.md
// 4.2m).  Nothing in the reference corresponds: its Text2GraphTransformer has fit_transform only (flat_amazon.py:57-71).
//
// One wavefront per document, kFoldWaves documents per workgroup pass, grid-stride over the batch.  Per document:
//   1. deg_d: the row's weights 64 at a time (coalesced), summed in the degree mode's order -- reference: the wave adds them
//      one after the other through v_readlane, as plan.hip's k_deg_sum_seq does; accurate: float64 per lane + butterfly.
//   2. the two gathers: every lane turns its own entry into a_j (one load of dis[w_j]); column id and a_j are then handed
//      out through v_readlane, so a gathered row is addressed from SGPRs; lane l holds columns 4l .. 4l+3 of the T1 row
//      (h <= 256) and of the P row (C <= 128), one 16-byte load each, four entries in flight; fp32 FMA in CSR order.
//   3. u = act(. + a_dd s1 + b1) goes to the wave's LDS slice (and to `hidden`), the gathered P sum next to it; then
//      u W2 from the workgroup's LDS copy of W2: lane l owns the columns l and l + 64, k in order; z, the store, arg-max.
// A document's arithmetic is a function of (h, C) and its own row: the leaf never depends on the batch or the row length.
// The document scalars, the row accesses, the wave-local LDS sync, the u W2 epilogue and the launch live in foldin.h:
// foldin_levels.hip runs the same code.  The pass over the words is written out in both kernels.
// Leaves (template): TAIL = h or C is not a multiple of 4 (the last lane of a row loads and stores scalars),
//                    WIDE = C > 64 (a second column per lane in the epilogue).
#include "foldin.h"

namespace tgcn {
namespace {

using namespace fold;

struct FoldArgs {
    int64_t n_docs;
    const int64_t *rowptr;
    const int32_t *col;
    const float *val;
    int n_vocab;
    const float *dis;
    int reference;
    const float *T1;
    int64_t ldt1;
    int h;
    const float *s1;
    const float *b1;
    int act;
    const float *P;
    int64_t ldp;
    int C;
    const float *W2;
    int64_t ldw2;
    const float *b2;
    float *logits;
    int64_t ldl;
    int32_t *pred;
    float *hidden;
    int64_t ldh;
};

template <bool TAIL, bool WIDE>
__global__ __launch_bounds__(64 * kFoldWaves) void k_foldin(const FoldArgs A) {
    extern __shared__ float4 lds4[];
    float *const W2s = reinterpret_cast<float *>(lds4);        // [h, C], tight
    const int h = A.h, C = A.C;
    const int H4 = (h + 3) & ~3, C4 = (C + 3) & ~3;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    float *const us = W2s + ((h * C + 3) & ~3) + wave * (H4 + C4);   // this wave's u [H4] ...
    float *const zs = us + H4;                                        // ... and its gathered P sum [C4]

    for (int i = threadIdx.x; i < h * C; i += 64 * kFoldWaves) {
        const int k = i / C;
        W2s[i] = A.W2[int64_t(k) * A.ldw2 + (i - k * C)];
    }
    __syncthreads();

    const int c0 = 4 * lane;
    const float4 b1v = load4<TAIL>(A.b1, c0, h);
    const float4 s1v = A.s1 ? load4<TAIL>(A.s1, c0, h) : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool on0 = lane < C, on1 = WIDE && lane + 64 < C;
    const float b2v0 = on0 ? A.b2[lane] : 0.f;
    const float b2v1 = on1 ? A.b2[lane + 64] : 0.f;
    const float *const w0 = W2s + (on0 ? lane : 0);
    const float *const w1 = W2s + (on1 ? lane + 64 : 0);
    const int reference = A.reference;

    const int64_t stride = int64_t(gridDim.x) * kFoldWaves;
    for (int64_t d = int64_t(blockIdx.x) * kFoldWaves + wave; d < A.n_docs; d += stride) {
        const int64_t beg = A.rowptr[d], end = A.rowptr[d + 1];
        const float dd = doc_dis(A.val, beg, end, lane, reference);
        const float a_dd = doc_self_weight(dd);
        float4 accT = make_float4(0.f, 0.f, 0.f, 0.f), accP = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t b = beg; b < end; b += 64) {
            int c;
            float a;
            doc_entry(A.col, A.val, A.dis, A.n_vocab, b, end, lane, dd, reference, c, a);
            const int cnt = static_cast<int>(min(int64_t(64), end - b));
            const bool clean = __ballot(lane < cnt && c < 0) == 0;      // no entry of the chunk is skipped
            int i = 0;
            if (clean) {
                for (; i + 4 <= cnt; i += 4) {
                    float4 xt[4], xp[4];
                    float av[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int cq = lane_i(c, i + q);
                        av[q] = lane_f(a, i + q);
                        xt[q] = load4<TAIL>(A.T1 + int64_t(cq) * A.ldt1, c0, h);
                        xp[q] = load4<TAIL>(A.P + int64_t(cq) * A.ldp, c0, C);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        fma4(accT, av[q], xt[q]);
                        fma4(accP, av[q], xp[q]);
                    }
                }
            }
            for (; i < cnt; ++i) {
                const int cq = lane_i(c, i);
                if (cq < 0) continue;                                     // wave-uniform
                const float aq = lane_f(a, i);
                const float4 xt = load4<TAIL>(A.T1 + int64_t(cq) * A.ldt1, c0, h);
                const float4 xp = load4<TAIL>(A.P + int64_t(cq) * A.ldp, c0, C);
                fma4(accT, aq, xt);
                fma4(accP, aq, xp);
            }
        }
        // u = act((sum + a_dd s1) + b1); columns at and beyond h are zero (zero loads, zero sums)
        float4 u = accT;
        if (A.s1) fma4(u, a_dd, s1v);
        u = bias_act4(u, b1v, A.act);
        if (c0 < H4) *reinterpret_cast<float4 *>(us + c0) = u;
        if (c0 < C4) *reinterpret_cast<float4 *>(zs + c0) = accP;
        if (A.hidden) store4<TAIL>(A.hidden + d * A.ldh, c0, h, u);
        wave_lds_sync();

        float y0, y1;
        u_times_w2<WIDE>(us, w0, w1, h, C, y0, y1);
        float z0 = -INFINITY, z1 = -INFINITY;
        float *const out = A.logits + d * A.ldl;
        if (on0) {
            z0 = fmaf(a_dd, y0, zs[lane]) + b2v0;
            out[lane] = z0;
        }
        if (on1) {
            z1 = fmaf(a_dd, y1, zs[lane + 64]) + b2v1;
            out[lane + 64] = z1;
        }
        if (A.pred) {
            float m;
            const int bi = first_argmax(z0, z1, on0, on1, lane, m);
            if (lane == 0) A.pred[d] = bi;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                 // the next document's stores follow this one's loads
    }
}

size_t foldin_lds_bytes(int h, int C) {
    const size_t H4 = (h + 3) & ~3, C4 = (C + 3) & ~3;
    return sizeof(float) * (((size_t(h) * C + 3) & ~size_t(3)) + kFoldWaves * (H4 + C4));
}

template <bool TAIL, bool WIDE>
int launch_foldin(const FoldArgs &A, hipStream_t s) {
    // the leaf's LDS ceiling is that of the largest shape
    return launch_fold<k_foldin<TAIL, WIDE>>(A, A.n_docs, static_cast<int>(foldin_lds_bytes(kFoldMaxH, kFoldMaxC)),
                                             foldin_lds_bytes(A.h, A.C), s);
}

}  // namespace
}  // namespace tgcn

extern "C" {

int tgcn_foldin_max_hidden(void) { return tgcn::kFoldMaxH; }
int tgcn_foldin_max_classes(void) { return tgcn::kFoldMaxC; }

int tgcn_foldin_two_layer(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                          const float *dis, int degree_sum, const float *T1, int64_t ldt1, int h, const float *s1,
                          const float *b1, int act, const float *P, int64_t ldp, int C, const float *W2, int64_t ldw2,
                          const float *b2, float *logits, int64_t ldl, int32_t *pred, float *hidden, int64_t ldh,
                          tgcn_stream stream) {
    using namespace tgcn;
    if (n_docs < 0 || n_vocab < 1 || n_vocab > INT32_MAX || h < 1 || h > kFoldMaxH || C < 1 || C > kFoldMaxC) {
        set_error("tgcn_foldin_two_layer: bad size (n_docs=%lld n_vocab=%lld h=%d, 1..%d; C=%d, 1..%d)", (long long)n_docs,
                  (long long)n_vocab, h, kFoldMaxH, C, kFoldMaxC);
        return TGCN_E_INVALID;
    }
    if ((act != TGCN_ACT_NONE && act != TGCN_ACT_RELU) ||
        (degree_sum != TGCN_DEGREE_ACCURATE && degree_sum != TGCN_DEGREE_REFERENCE)) {
        set_error("tgcn_foldin_two_layer: unknown act %d or degree_sum %d", act, degree_sum);
        return TGCN_E_INVALID;
    }
    if (ldt1 < h || ldp < C || ldw2 < C || ldl < C || (hidden && ldh < h) ||
        ((ldt1 | ldp | ldw2 | ldl | (hidden ? ldh : 0)) & 3) != 0) {
        set_error("tgcn_foldin_two_layer: leading dimensions must cover their rows and be multiples of 4 (ldt1=%lld ldp=%lld "
                  "ldw2=%lld ldl=%lld ldh=%lld for h=%d C=%d)", (long long)ldt1, (long long)ldp, (long long)ldw2,
                  (long long)ldl, (long long)ldh, h, C);
        return TGCN_E_INVALID;
    }
    if (n_docs == 0) return TGCN_OK;
    if (!rowptr || !col || !val || !dis || !T1 || !b1 || !P || !W2 || !b2 || !logits) {
        set_error("tgcn_foldin_two_layer: NULL pointer (only s1, pred and hidden may be NULL)");
        return TGCN_E_INVALID;
    }
    if (!aligned16(T1) || !aligned16(P) || !aligned16(W2) || !aligned16(b1) || !aligned16(b2) || !aligned16(s1) ||
        !aligned16(logits) || !aligned16(hidden)) {
        set_error("tgcn_foldin_two_layer: T1, P, W2, s1, b1, b2, logits and hidden must be 16-byte aligned");
        return TGCN_E_INVALID;
    }
    FoldArgs A{n_docs, rowptr, col, val, static_cast<int>(n_vocab), dis, degree_sum == TGCN_DEGREE_REFERENCE, T1, ldt1, h,
               s1, b1, act, P, ldp, C, W2, ldw2, b2, logits, ldl, pred, hidden, ldh};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool tail = (h % 4) != 0 || (C % 4) != 0, wide = C > 64;
    if (tail)
        return wide ? launch_foldin<true, true>(A, s) : launch_foldin<true, false>(A, s);
    return wide ? launch_foldin<false, true>(A, s) : launch_foldin<false, false>(A, s);
}

}  // extern "C"
