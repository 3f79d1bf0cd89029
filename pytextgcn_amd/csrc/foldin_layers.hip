// tgcn_foldin_layers -- documents outside the training graph through a chain of L = 2, 3 or 4 GCNConv layers (include/tgcn.h;
// DESIGN.md 4.2p): the deep GCN / EGCN (models.py: n_gcn) and the layers of the JumpingKnowledgeNetwork, whose row-wise
// aggregation then runs on the L outputs.  The reference runs these models on graph nodes only.
//
// One wavefront per document, kFoldWaves documents per workgroup pass, grid-stride over the batch, as foldin.hip -- and the
// document's scalars, row accesses, wave-local LDS sync, x W epilogue and the launch ARE foldin.hip's (foldin.h).  The pass
// over the words is written out here as it is there and in foldin_levels.hip (one body for several kernels measured slower,
// DESIGN.md 7).  Per document:
//   1. deg_d, dis_d, a_dd once.
//   2. ONE pass over the words: column id and a_j through v_readlane, then the word's row of the combined table, which
//      holds the L segments T^l[w] (one scalar row address, one loop-invariant lane offset per segment); lane i holds
//      columns 4i .. 4i+3 of each segment, L float4 accumulators, kFlight entries in flight: 4 L loads of 16 bytes per lane
//      at L <= 3 and 2 L at L = 4, 48 registers at the most next to the 16 of the accumulators -- what the 128 registers of
//      a 1024-thread workgroup hold (foldin_levels.hip carries 64 + 16 at its L = 2).
//   3. the sums of the layers 2 .. L go to the wave's LDS slice [ x^1 (r4 w_1) | x^2 | .. | x^L ], so that no accumulator
//      is alive across the layers (the x W loop wants the registers); W_2 .. W_L and the biases were staged in LDS once per
//      workgroup.  Layer 1 is resolved in the lane's registers (columns 4i .. 4i+3, as foldin.hip's u) and stored to the
//      slice; then the layers in order: x^{l-1} W_l from the LDS copy of W_l (lane i owns the columns i and i + 64), the
//      sum, the bias, the activation; x^l overwrites the layer's sum in place (each lane what it alone has read).
// Leaves (template): L in {2, 3, 4}; TAIL = some w_l is not a multiple of 4; WIDE = some w_l, l >= 2, above 64.  act is per
// layer and read at run time.  A document's arithmetic is a function of the widths and its own row.
#include "foldin.h"

namespace tgcn {
namespace {

using namespace fold;

constexpr int kMaxLayers = TGCN_FOLDIN_MAX_LAYERS;

struct LayerK {
    const float *W, *b;
    float *out;
    int64_t ldw, ldo;
    int width, act;
    int t_col;                 // where the layer's segment begins in a row of the table
    int w_off, b_off;          // floats from the start of LDS: W_l (tight [w_{l-1}, w_l]), b_l (r4 w_l, zero pad)
    int x_off;                 // floats from the start of a wave's slice: x^l (r4 w_l)
};

struct LayersArgs {
    int64_t n_docs;
    const int64_t *rowptr;
    const int32_t *col;
    const float *val;
    const float *dis;
    const float *table;
    int64_t ldt;
    const float *s1;
    int32_t *pred;
    int n_vocab;
    int reference;
    int slice_off, slice;      // floats: the first wave's slice, and a slice's size
    LayerK ly[kMaxLayers];
};

template <int L, bool TAIL, bool WIDE>
__global__ __launch_bounds__(64 * kFoldWaves) void k_foldin_layers(const LayersArgs A) {
    constexpr int kFlight = L == 4 ? 2 : 4;
    extern __shared__ float4 lds4[];
    float *const lds = reinterpret_cast<float *>(lds4);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));

#pragma unroll
    for (int l = 0; l < L; ++l) {
        const LayerK &V = A.ly[l];
        const int w = V.width;
        if (l > 0) {
            const int n = A.ly[l - 1].width * w;
            float *const Ws = lds + V.w_off;                              // [w_{l-1}, w_l], tight
            for (int i = threadIdx.x; i < n; i += 64 * kFoldWaves) {
                const int k = i / w;
                Ws[i] = V.W[int64_t(k) * V.ldw + (i - k * w)];
            }
        }
        const int W4 = (w + 3) & ~3;
        for (int i = threadIdx.x; i < W4; i += 64 * kFoldWaves) lds[V.b_off + i] = i < w ? V.b[i] : 0.f;
    }
    __syncthreads();

    float *const us = lds + A.slice_off + wave * A.slice;
    const int c0 = 4 * lane;
    const int reference = A.reference;
    const int w1 = A.ly[0].width;
    const int W41 = (w1 + 3) & ~3;
    const float4 s1v = A.s1 ? load4<TAIL>(A.s1, c0, w1) : make_float4(0.f, 0.f, 0.f, 0.f);

    const int64_t stride = int64_t(gridDim.x) * kFoldWaves;
    for (int64_t d = int64_t(blockIdx.x) * kFoldWaves + wave; d < A.n_docs; d += stride) {
        const int64_t beg = A.rowptr[d], end = A.rowptr[d + 1];
        const float dd = doc_dis(A.val, beg, end, lane, reference);
        const float a_dd = doc_self_weight(dd);
        float4 acc[L];
#pragma unroll
        for (int l = 0; l < L; ++l) acc[l] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t b = beg; b < end; b += 64) {
            int c;
            float a;
            doc_entry(A.col, A.val, A.dis, A.n_vocab, b, end, lane, dd, reference, c, a);
            const int cnt = static_cast<int>(min(int64_t(64), end - b));
            const bool clean = __ballot(lane < cnt && c < 0) == 0;      // no entry of the chunk is skipped
            int i = 0;
            if (clean) {
                for (; i + kFlight <= cnt; i += kFlight) {
                    float4 x[kFlight][L];
                    float av[kFlight];
#pragma unroll
                    for (int q = 0; q < kFlight; ++q) {
                        const float *const row = A.table + int64_t(lane_i(c, i + q)) * A.ldt;
                        av[q] = lane_f(a, i + q);
#pragma unroll
                        for (int l = 0; l < L; ++l) x[q][l] = load4<TAIL>(row + A.ly[l].t_col, c0, A.ly[l].width);
                    }
#pragma unroll
                    for (int q = 0; q < kFlight; ++q) {
#pragma unroll
                        for (int l = 0; l < L; ++l) fma4(acc[l], av[q], x[q][l]);
                    }
                }
            }
            for (; i < cnt; ++i) {
                const int cq = lane_i(c, i);
                if (cq < 0) continue;                                     // wave-uniform
                const float aq = lane_f(a, i);
                const float *const row = A.table + int64_t(cq) * A.ldt;
                float4 x[L];
#pragma unroll
                for (int l = 0; l < L; ++l) x[l] = load4<TAIL>(row + A.ly[l].t_col, c0, A.ly[l].width);
#pragma unroll
                for (int l = 0; l < L; ++l) fma4(acc[l], aq, x[l]);
            }
        }

        // the sums of the layers 2 .. L leave the registers: the layers below work from the slice
#pragma unroll
        for (int l = 1; l < L; ++l)
            if (c0 < ((A.ly[l].width + 3) & ~3)) *reinterpret_cast<float4 *>(us + A.ly[l].x_off + c0) = acc[l];

        // x^1 = act((sum + a_dd s1) + b_1), as foldin.hip's u; columns at and beyond w_1 are zero (zero loads, zero sums,
        // zero pad of the bias)
        {
            float4 u = acc[0];
            if (A.s1) fma4(u, a_dd, s1v);
            if (c0 < W41) {
                u = bias_act4(u, *reinterpret_cast<const float4 *>(lds + A.ly[0].b_off + c0), A.ly[0].act);
                *reinterpret_cast<float4 *>(us + A.ly[0].x_off + c0) = u;
            }
            if (A.ly[0].out) store4<TAIL>(A.ly[0].out + d * A.ly[0].ldo, c0, w1, u);
        }
        wave_lds_sync();

        // ONE loop body for the layers 2 .. L (not unrolled, as in foldin_levels.hip: a layer's parameters are scalar
        // loads by l)
#pragma unroll 1
        for (int l = 1; l < L; ++l) {
            const LayerK &V = A.ly[l];
            const int w = V.width, hp = A.ly[l - 1].width;
            float *const xs = us + V.x_off;
            const bool on0 = lane < w, on1 = WIDE && lane + 64 < w;
            float y0, y1;
            u_times_w2<WIDE>(us + A.ly[l - 1].x_off, lds + V.w_off + (on0 ? lane : 0), lds + V.w_off + (on1 ? lane + 64 : 0),
                             hp, w, y0, y1);
            float z0 = -INFINITY, z1 = -INFINITY;
            if (on0) {
                z0 = act1(fmaf(a_dd, y0, xs[lane]) + lds[V.b_off + lane], V.act);
                xs[lane] = z0;                                   // each lane overwrites what it alone has read
            }
            if (on1) {
                z1 = act1(fmaf(a_dd, y1, xs[lane + 64]) + lds[V.b_off + lane + 64], V.act);
                xs[lane + 64] = z1;
            }
            if (V.out) {
                float *const out = V.out + d * V.ldo;
                if (on0) out[lane] = z0;
                if (on1) out[lane + 64] = z1;
            }
            if (l == L - 1 && A.pred) {
                float m;
                const int bi = first_argmax(z0, z1, on0, on1, lane, m);
                if (lane == 0) A.pred[d] = bi;
            }
            wave_lds_sync();                                     // the next layer's (document's) accesses follow these
        }
    }
}

inline size_t r4(size_t v) { return (v + 3) & ~size_t(3); }

// floats; fills the offsets of `A` when given
size_t layers_lds_floats(int L, const int32_t *w, LayersArgs *A) {
    size_t at = 0, slice = 0;
    for (int l = 1; l < L; ++l) {
        if (A) A->ly[l].w_off = static_cast<int>(at);
        at += r4(size_t(w[l - 1]) * w[l]);
    }
    for (int l = 0; l < L; ++l) {
        if (A) A->ly[l].b_off = static_cast<int>(at), A->ly[l].x_off = static_cast<int>(slice);
        at += r4(w[l]);
        slice += r4(w[l]);
    }
    if (A) {
        A->ly[0].w_off = 0;
        A->slice_off = static_cast<int>(at);
        A->slice = static_cast<int>(slice);
    }
    return at + size_t(kFoldWaves) * slice;
}

bool widths_ok(int L, const int32_t *w) {
    if (L < 2 || L > kMaxLayers || !w) return false;
    for (int l = 0; l < L; ++l)
        if (w[l] < 1 || w[l] > (l == 0 ? kFoldMaxH : kFoldMaxC)) return false;
    return true;
}

template <int L, bool TAIL, bool WIDE>
int launch_layers(const LayersArgs &A, size_t lds_bytes, hipStream_t s) {
    return launch_fold<k_foldin_layers<L, TAIL, WIDE>>(A, A.n_docs, TGCN_FOLDIN_LEVELS_LDS_LIMIT, lds_bytes, s);
}

template <int L>
int launch_layers_of(const LayersArgs &A, bool tail, bool wide, size_t lds_bytes, hipStream_t s) {
    if (tail)
        return wide ? launch_layers<L, true, true>(A, lds_bytes, s) : launch_layers<L, true, false>(A, lds_bytes, s);
    return wide ? launch_layers<L, false, true>(A, lds_bytes, s) : launch_layers<L, false, false>(A, lds_bytes, s);
}

}  // namespace
}  // namespace tgcn

extern "C" {

int64_t tgcn_foldin_layers_lds_bytes(int n_layers, const int32_t *width) {
    using namespace tgcn;
    if (!widths_ok(n_layers, width)) return -1;
    return static_cast<int64_t>(sizeof(float) * layers_lds_floats(n_layers, width, nullptr));
}

int tgcn_foldin_layers(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                       const float *dis, int degree_sum, const float *table, int64_t ldt, const float *s1, int n_layers,
                       const tgcn_foldin_layer *layers, int32_t *pred, tgcn_stream stream) {
    using namespace tgcn;
    if (n_layers < 2 || n_layers > kMaxLayers || !layers) {
        set_error("tgcn_foldin_layers: n_layers=%d (2..%d) with a non-NULL `layers`", n_layers, kMaxLayers);
        return TGCN_E_INVALID;
    }
    if (n_docs < 0 || n_vocab < 1 || n_vocab > INT32_MAX || ldt < 4 || ldt > INT32_MAX || (ldt & 3) != 0) {
        set_error("tgcn_foldin_layers: bad size (n_docs=%lld n_vocab=%lld; ldt=%lld, a multiple of 4)", (long long)n_docs,
                  (long long)n_vocab, (long long)ldt);
        return TGCN_E_INVALID;
    }
    if (degree_sum != TGCN_DEGREE_ACCURATE && degree_sum != TGCN_DEGREE_REFERENCE) {
        set_error("tgcn_foldin_layers: unknown degree_sum %d", degree_sum);
        return TGCN_E_INVALID;
    }
    int32_t ws[kMaxLayers];
    bool tail = false, wide = false;
    for (int l = 0; l < n_layers; ++l) {
        const tgcn_foldin_layer &v = layers[l];
        const int wmax = l == 0 ? kFoldMaxH : kFoldMaxC;
        if (v.width < 1 || v.width > wmax) {
            set_error("tgcn_foldin_layers: layer %d: bad size (width=%d, 1..%d)", l + 1, v.width, wmax);
            return TGCN_E_INVALID;
        }
        if (v.act != TGCN_ACT_NONE && v.act != TGCN_ACT_RELU) {
            set_error("tgcn_foldin_layers: layer %d: unknown act %d", l + 1, v.act);
            return TGCN_E_INVALID;
        }
        if (v.t_col < 0 || (v.t_col & 3) != 0 || int64_t(v.t_col) + v.width > ldt) {
            set_error("tgcn_foldin_layers: layer %d: the segment must begin at a multiple of 4 and end inside a table row "
                      "(t_col=%d width=%d ldt=%lld)", l + 1, v.t_col, v.width, (long long)ldt);
            return TGCN_E_INVALID;
        }
        const int64_t ldw = l > 0 ? v.ldw : 0, ldo = v.out ? v.ldo : 0;
        if ((l > 0 && ldw < v.width) || (v.out && ldo < v.width) || ((ldw | ldo) & 3) != 0) {
            set_error("tgcn_foldin_layers: layer %d: leading dimensions must cover their rows and be multiples of 4 (ldw=%lld "
                      "ldo=%lld for width=%d)", l + 1, (long long)ldw, (long long)ldo, v.width);
            return TGCN_E_INVALID;
        }
        ws[l] = v.width;
        tail = tail || (v.width % 4) != 0;
        wide = wide || (l > 0 && v.width > 64);
    }
    LayersArgs A{};
    const size_t lds_bytes = sizeof(float) * layers_lds_floats(n_layers, ws, &A);
    if (lds_bytes > size_t(TGCN_FOLDIN_LEVELS_LDS_LIMIT)) {
        set_error("tgcn_foldin_layers: the staged W_2 .. W_L, the biases and the waves' slices need %zu bytes of LDS, a CU has "
                  "%d (tgcn_foldin_layers_lds_bytes)", lds_bytes, TGCN_FOLDIN_LEVELS_LDS_LIMIT);
        return TGCN_E_INVALID;
    }
    if (n_docs == 0) return TGCN_OK;
    if (!rowptr || !col || !val || !dis || !table || !aligned16(table) || !aligned16(s1)) {
        set_error("tgcn_foldin_layers: NULL pointer (rowptr, col, val, dis, table), or a table or s1 that is not 16-byte "
                  "aligned");
        return TGCN_E_INVALID;
    }
    for (int l = 0; l < n_layers; ++l) {
        const tgcn_foldin_layer &v = layers[l];
        if (!v.b || (l > 0 && !v.W)) {
            set_error("tgcn_foldin_layers: layer %d: NULL pointer (only s1, out and pred may be NULL)", l + 1);
            return TGCN_E_INVALID;
        }
        if ((l > 0 && !aligned16(v.W)) || !aligned16(v.b) || !aligned16(v.out)) {
            set_error("tgcn_foldin_layers: layer %d: W, b and out must be 16-byte aligned", l + 1);
            return TGCN_E_INVALID;
        }
        LayerK &K = A.ly[l];
        K.W = l > 0 ? v.W : nullptr, K.b = v.b, K.out = v.out, K.ldw = l > 0 ? v.ldw : 0, K.ldo = v.out ? v.ldo : 0;
        K.width = v.width, K.act = v.act, K.t_col = v.t_col;
    }
    A.n_docs = n_docs, A.rowptr = rowptr, A.col = col, A.val = val, A.dis = dis, A.table = table, A.ldt = ldt;
    A.s1 = s1, A.pred = pred;
    A.n_vocab = static_cast<int>(n_vocab), A.reference = degree_sum == TGCN_DEGREE_REFERENCE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (n_layers) {
        case 2: return launch_layers_of<2>(A, tail, wide, lds_bytes, s);
        case 3: return launch_layers_of<3>(A, tail, wide, lds_bytes, s);
        default: return launch_layers_of<4>(A, tail, wide, lds_bytes, s);
    }
}

}  // extern "C"
