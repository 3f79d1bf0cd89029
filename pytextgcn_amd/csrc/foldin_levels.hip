// tgcn_foldin_levels -- documents outside the training graph through the per-level hierarchy (include/tgcn.h; DESIGN.md
// 4.2n): L = 2 or 3 two-layer networks on one graph, level l >= 2 fed the link (softmax or one-hot) of level l-1's logits.
// The reference runs the strategy on graph nodes only (perlevel_amazon.py, perlevel_dbpedia.py).
//
// One wavefront per document, kFoldWaves documents per workgroup pass, grid-stride over the batch, as foldin.hip -- and the
// document's scalars, row accesses, wave-local LDS sync, u W2 epilogue and the launch ARE foldin.hip's (foldin.h).  The pass
// over the words is written out here as it is there: one body for both (2 segments of two tables, 2L segments of one) gave
// the same bits but measured slower in leaves of either kernel (profiles/r21_shared_bodies_isa.md).
// Per document:
//   1. deg_d, dis_d, a_dd once.
//   2. ONE pass over the words: column id and a_j through v_readlane, then the word's row of the combined table, which
//      holds the 2L segments T1^l[w], P^l[w] (one scalar row address, one loop-invariant lane offset per segment); lane i
//      holds columns 4i .. 4i+3 of each segment, 2L float4
//      accumulators, kFlight entries in flight (4 at L = 2, 2 at L = 3: 16 resp. 12 loads of 16 bytes per lane, which is
//      what the 128 registers of a 1024-thread workgroup hold next to the accumulators).
//   3. the 2L sums go to the wave's LDS slice  [ u^1 (H4_1) | zs^1 (C4_1) | .. | u^L | zs^L ], so that no accumulator is
//      alive across the levels (the u W2 loop wants the registers); W2^l, Wh^l and the biases were staged in LDS once per
//      workgroup.  Then the levels in order:
//      s^l from p^l (which overwrote zs^{l-1} in place) and the LDS copy of Wh^l, rows padded to H4_l, float4 reads;
//      u^l -> slice; u^l W2^l from the LDS copy of W2^l; z^l; arg-max; the next level's link.
// Leaves (template): L in {2, 3}; TAIL = some h_l or C_l is not a multiple of 4; WIDE = some C_l > 64.  act and link are
// per level and read at run time.  A document's arithmetic is a function of the widths and its own row.
#include "foldin.h"

namespace tgcn {
namespace {

using namespace fold;

constexpr int kMaxLevels = TGCN_FOLDIN_MAX_LEVELS;

struct LevelK {
    const float *W2, *Wh, *b1, *b2;
    float *logits, *hidden, *link_out;
    int32_t *pred;
    int64_t ldw2, ldwh, ldl, ldh, ldk;
    int h, C, act, link;
    int t1_col, p_col;                    // where the level's T1 and P segments begin in a row of the table
    int w2_off, wh_off, b1_off, b2_off;   // floats from the start of LDS: W2^l, Wh^l, b1^l (H4_l, zero pad), b2^l (C4_l)
    int us_off, zs_off;                   // floats from the start of a wave's slice: u^l (H4_l), zs^l (C4_l)
};

struct LevelsArgs {
    int64_t n_docs;
    const int64_t *rowptr;
    const int32_t *col;
    const float *val;
    const float *dis;
    const float *table;
    int64_t ldt;
    int n_vocab;
    int reference;
    int slice_off, slice;            // floats: the first wave's slice, and a slice's size
    LevelK lv[kMaxLevels];
};

template <int L, bool TAIL, bool WIDE>
__global__ __launch_bounds__(64 * kFoldWaves) void k_foldin_levels(const LevelsArgs A) {
    constexpr int kFlight = L == 2 ? 4 : 2;
    extern __shared__ float4 lds4[];
    float *const lds = reinterpret_cast<float *>(lds4);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));

#pragma unroll
    for (int l = 0; l < L; ++l) {
        const LevelK &V = A.lv[l];
        const int h = V.h, C = V.C;
        float *const W2s = lds + V.w2_off;                            // [h, C], tight
        for (int i = threadIdx.x; i < h * C; i += 64 * kFoldWaves) {
            const int k = i / C;
            W2s[i] = V.W2[int64_t(k) * V.ldw2 + (i - k * C)];
        }
        const int H4 = (h + 3) & ~3;
        for (int i = threadIdx.x; i < H4; i += 64 * kFoldWaves) lds[V.b1_off + i] = i < h ? V.b1[i] : 0.f;
        for (int i = threadIdx.x; i < C; i += 64 * kFoldWaves) lds[V.b2_off + i] = V.b2[i];
        if (l > 0) {
            const int n = A.lv[l - 1].C * H4;
            float *const Whs = lds + V.wh_off;                        // [C_{l-1}, H4], zeros beyond h
            for (int i = threadIdx.x; i < n; i += 64 * kFoldWaves) {
                const int c = i / H4, k = i - c * H4;
                Whs[i] = k < h ? V.Wh[int64_t(c) * V.ldwh + k] : 0.f;
            }
        }
    }
    __syncthreads();

    float *const us = lds + A.slice_off + wave * A.slice;
    const int c0 = 4 * lane;
    const int reference = A.reference;

    const int64_t stride = int64_t(gridDim.x) * kFoldWaves;
    for (int64_t d = int64_t(blockIdx.x) * kFoldWaves + wave; d < A.n_docs; d += stride) {
        const int64_t beg = A.rowptr[d], end = A.rowptr[d + 1];
        const float dd = doc_dis(A.val, beg, end, lane, reference);
        const float a_dd = doc_self_weight(dd);
        float4 accT[L], accP[L];
#pragma unroll
        for (int l = 0; l < L; ++l) accT[l] = accP[l] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t b = beg; b < end; b += 64) {
            int c;
            float a;
            doc_entry(A.col, A.val, A.dis, A.n_vocab, b, end, lane, dd, reference, c, a);
            const int cnt = static_cast<int>(min(int64_t(64), end - b));
            const bool clean = __ballot(lane < cnt && c < 0) == 0;      // no entry of the chunk is skipped
            int i = 0;
            if (clean) {
                for (; i + kFlight <= cnt; i += kFlight) {
                    float4 xt[kFlight][L], xp[kFlight][L];
                    float av[kFlight];
#pragma unroll
                    for (int q = 0; q < kFlight; ++q) {
                        const float *const row = A.table + int64_t(lane_i(c, i + q)) * A.ldt;
                        av[q] = lane_f(a, i + q);
#pragma unroll
                        for (int l = 0; l < L; ++l) {
                            xt[q][l] = load4<TAIL>(row + A.lv[l].t1_col, c0, A.lv[l].h);
                            xp[q][l] = load4<TAIL>(row + A.lv[l].p_col, c0, A.lv[l].C);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < kFlight; ++q) {
#pragma unroll
                        for (int l = 0; l < L; ++l) {
                            fma4(accT[l], av[q], xt[q][l]);
                            fma4(accP[l], av[q], xp[q][l]);
                        }
                    }
                }
            }
            for (; i < cnt; ++i) {
                const int cq = lane_i(c, i);
                if (cq < 0) continue;                                     // wave-uniform
                const float aq = lane_f(a, i);
                const float *const row = A.table + int64_t(cq) * A.ldt;
                float4 xt[L], xp[L];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    xt[l] = load4<TAIL>(row + A.lv[l].t1_col, c0, A.lv[l].h);
                    xp[l] = load4<TAIL>(row + A.lv[l].p_col, c0, A.lv[l].C);
                }
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    fma4(accT[l], aq, xt[l]);
                    fma4(accP[l], aq, xp[l]);
                }
            }
        }

        // the sums leave the registers: the levels below work from the slice, with no accumulator alive across them
#pragma unroll
        for (int l = 0; l < L; ++l) {
            if (c0 < ((A.lv[l].h + 3) & ~3)) *reinterpret_cast<float4 *>(us + A.lv[l].us_off + c0) = accT[l];
            if (c0 < ((A.lv[l].C + 3) & ~3)) *reinterpret_cast<float4 *>(us + A.lv[l].zs_off + c0) = accP[l];
        }

        // ONE loop body for all levels (not unrolled: L copies of it, each with its own loop-invariant addresses hoisted
        // out of the document loop, do not fit the registers); a level's parameters are scalar loads by l
        int kprev = 0;                                   // the previous level's first arg-max (wave-uniform)
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            const LevelK &V = A.lv[l];
            const int h = V.h, C = V.C;
            const int H4 = (h + 3) & ~3;
            float *const ul = us + V.us_off, *const zs = us + V.zs_off;
            // u = act((sum + a_dd s) + b1); columns at and beyond h are zero (zero loads, zero sums, zero pad of Wh)
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 < H4) u = *reinterpret_cast<const float4 *>(ul + c0);        // (this lane's own store)
            if (l > 0) {
                const float *const Whs = lds + V.wh_off;
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 < H4) {
                    if (V.link == TGCN_FOLDIN_LINK_ONE_HOT) {
                        s = *reinterpret_cast<const float4 *>(Whs + kprev * H4 + c0);
                    } else {
                        const float *const ps = us + A.lv[l - 1].zs_off;    // p^l, where the previous level's P sum was
                        const int Cp = A.lv[l - 1].C;
                        for (int cc = 0; cc < Cp; ++cc)
                            fma4(s, ps[cc], *reinterpret_cast<const float4 *>(Whs + cc * H4 + c0));
                    }
                }
                fma4(u, a_dd, s);
            }
            if (c0 < H4) {
                u = bias_act4(u, *reinterpret_cast<const float4 *>(lds + V.b1_off + c0), V.act);
                *reinterpret_cast<float4 *>(ul + c0) = u;
            }
            if (V.hidden) store4<TAIL>(V.hidden + d * V.ldh, c0, h, u);
            wave_lds_sync();

            const bool on0 = lane < C, on1 = WIDE && lane + 64 < C;
            float y0, y1;
            u_times_w2<WIDE>(ul, lds + V.w2_off + (on0 ? lane : 0), lds + V.w2_off + (on1 ? lane + 64 : 0), h, C, y0, y1);
            float z0 = -INFINITY, z1 = -INFINITY;
            if (on0) z0 = fmaf(a_dd, y0, zs[lane]) + lds[V.b2_off + lane];
            if (on1) z1 = fmaf(a_dd, y1, zs[lane + 64]) + lds[V.b2_off + lane + 64];
            if (V.logits) {
                float *const out = V.logits + d * V.ldl;
                if (on0) out[lane] = z0;
                if (on1) out[lane + 64] = z1;
            }
            if (V.pred || l + 1 < L) {
                float m;
                const int bi = first_argmax(z0, z1, on0, on1, lane, m);
                if (V.pred && lane == 0) V.pred[d] = bi;
                if (l + 1 < L) {
                    const LevelK &Nx = A.lv[l + 1];
                    float p0, p1;
                    if (Nx.link == TGCN_FOLDIN_LINK_ONE_HOT) {
                        kprev = bi;
                        p0 = (on0 && lane == bi) ? 1.f : 0.f;
                        p1 = (on1 && lane + 64 == bi) ? 1.f : 0.f;
                    } else {
                        const float e0 = on0 ? expf(z0 - m) : 0.f;
                        const float e1 = on1 ? expf(z1 - m) : 0.f;
                        float S = on1 ? e0 + e1 : e0;                      // (the order of include/tgcn.h)
#pragma unroll
                        for (int off = 32; off > 0; off >>= 1) S += __shfl_xor(S, off, 64);
                        p0 = e0 / S;
                        p1 = e1 / S;
                        if (on0) zs[lane] = p0;                            // each lane overwrites what it alone has read
                        if (on1) zs[lane + 64] = p1;
                    }
                    if (Nx.link_out) {
                        float *const out = Nx.link_out + d * Nx.ldk;
                        if (on0) out[lane] = p0;
                        if (on1) out[lane + 64] = p1;
                    }
                }
            }
            wave_lds_sync();                             // the next level's (document's) stores follow this one's loads
        }
    }
}

inline size_t r4(size_t v) { return (v + 3) & ~size_t(3); }

// floats; fills the offsets of `A` when given
size_t levels_lds_floats(int L, const int32_t *h, const int32_t *C, LevelsArgs *A) {
    size_t at = 0, slice = 0;
    for (int l = 0; l < L; ++l) {
        if (A) A->lv[l].w2_off = static_cast<int>(at);
        at += r4(size_t(h[l]) * C[l]);
    }
    for (int l = 1; l < L; ++l) {
        if (A) A->lv[l].wh_off = static_cast<int>(at);
        at += size_t(C[l - 1]) * r4(h[l]);
    }
    for (int l = 0; l < L; ++l) {
        if (A) {
            A->lv[l].b1_off = static_cast<int>(at), A->lv[l].b2_off = static_cast<int>(at + r4(h[l]));
            A->lv[l].us_off = static_cast<int>(slice), A->lv[l].zs_off = static_cast<int>(slice + r4(h[l]));
        }
        at += r4(h[l]) + r4(C[l]);
        slice += r4(h[l]) + r4(C[l]);
    }
    if (A) {
        A->lv[0].wh_off = 0;
        A->slice_off = static_cast<int>(at);
        A->slice = static_cast<int>(slice);
    }
    return at + size_t(kFoldWaves) * slice;
}

bool widths_ok(int L, const int32_t *h, const int32_t *C) {
    if (L < 2 || L > kMaxLevels || !h || !C) return false;
    for (int l = 0; l < L; ++l)
        if (h[l] < 1 || h[l] > kFoldMaxH || C[l] < 1 || C[l] > kFoldMaxC) return false;
    return true;
}

template <int L, bool TAIL, bool WIDE>
int launch_levels(const LevelsArgs &A, size_t lds_bytes, hipStream_t s) {
    return launch_fold<k_foldin_levels<L, TAIL, WIDE>>(A, A.n_docs, TGCN_FOLDIN_LEVELS_LDS_LIMIT, lds_bytes, s);
}

template <int L>
int launch_levels_of(const LevelsArgs &A, bool tail, bool wide, size_t lds_bytes, hipStream_t s) {
    if (tail)
        return wide ? launch_levels<L, true, true>(A, lds_bytes, s) : launch_levels<L, true, false>(A, lds_bytes, s);
    return wide ? launch_levels<L, false, true>(A, lds_bytes, s) : launch_levels<L, false, false>(A, lds_bytes, s);
}

}  // namespace
}  // namespace tgcn

extern "C" {

int64_t tgcn_foldin_levels_lds_bytes(int n_levels, const int32_t *h, const int32_t *C) {
    using namespace tgcn;
    if (!widths_ok(n_levels, h, C)) return -1;
    return static_cast<int64_t>(sizeof(float) * levels_lds_floats(n_levels, h, C, nullptr));
}

int tgcn_foldin_levels(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                       const float *dis, int degree_sum, const float *table, int64_t ldt, int n_levels,
                       const tgcn_foldin_level *levels, tgcn_stream stream) {
    using namespace tgcn;
    if (n_levels < 2 || n_levels > kMaxLevels || !levels) {
        set_error("tgcn_foldin_levels: n_levels=%d (2..%d) with a non-NULL `levels`", n_levels, kMaxLevels);
        return TGCN_E_INVALID;
    }
    if (n_docs < 0 || n_vocab < 1 || n_vocab > INT32_MAX || ldt < 4 || ldt > INT32_MAX || (ldt & 3) != 0) {
        set_error("tgcn_foldin_levels: bad size (n_docs=%lld n_vocab=%lld; ldt=%lld, a multiple of 4)", (long long)n_docs,
                  (long long)n_vocab, (long long)ldt);
        return TGCN_E_INVALID;
    }
    if (degree_sum != TGCN_DEGREE_ACCURATE && degree_sum != TGCN_DEGREE_REFERENCE) {
        set_error("tgcn_foldin_levels: unknown degree_sum %d", degree_sum);
        return TGCN_E_INVALID;
    }
    int32_t hs[kMaxLevels], Cs[kMaxLevels];
    bool tail = false, wide = false;
    for (int l = 0; l < n_levels; ++l) {
        const tgcn_foldin_level &v = levels[l];
        if (v.h < 1 || v.h > kFoldMaxH || v.C < 1 || v.C > kFoldMaxC) {
            set_error("tgcn_foldin_levels: level %d: bad size (h=%d, 1..%d; C=%d, 1..%d)", l + 1, v.h, kFoldMaxH, v.C, kFoldMaxC);
            return TGCN_E_INVALID;
        }
        if ((v.act != TGCN_ACT_NONE && v.act != TGCN_ACT_RELU) ||
            (l > 0 && v.link != TGCN_FOLDIN_LINK_SOFTMAX && v.link != TGCN_FOLDIN_LINK_ONE_HOT)) {
            set_error("tgcn_foldin_levels: level %d: unknown act %d or link %d", l + 1, v.act, v.link);
            return TGCN_E_INVALID;
        }
        const int Cp = l > 0 ? levels[l - 1].C : 0;
        const int64_t ldwh = l > 0 ? v.ldwh : 0, ldl = v.logits ? v.ldl : 0, ldh = v.hidden ? v.ldh : 0,
                      ldk = (l > 0 && v.link_out) ? v.ldk : 0;
        if (v.t1_col < 0 || v.p_col < 0 || ((v.t1_col | v.p_col) & 3) != 0 || v.t1_col + v.h > ldt || v.p_col + v.C > ldt) {
            set_error("tgcn_foldin_levels: level %d: the segments must begin at multiples of 4 and end inside a table row "
                      "(t1_col=%lld h=%d p_col=%lld C=%d ldt=%lld)", l + 1, (long long)v.t1_col, v.h, (long long)v.p_col, v.C,
                      (long long)ldt);
            return TGCN_E_INVALID;
        }
        if (v.ldw2 < v.C || (l > 0 && ldwh < v.h) || (v.logits && ldl < v.C) ||
            (v.hidden && ldh < v.h) || (l > 0 && v.link_out && ldk < Cp) ||
            ((v.ldw2 | ldwh | ldl | ldh | ldk) & 3) != 0) {
            set_error("tgcn_foldin_levels: level %d: leading dimensions must cover their rows and be multiples of 4 ("
                      "ldw2=%lld ldwh=%lld ldl=%lld ldh=%lld ldk=%lld for h=%d C=%d, %d link columns)", l + 1,
                      (long long)v.ldw2, (long long)ldwh, (long long)ldl, (long long)ldh,
                      (long long)ldk, v.h, v.C, Cp);
            return TGCN_E_INVALID;
        }
        if (l == 0 && v.link_out) {
            set_error("tgcn_foldin_levels: level 1 has no link: its link_out must be NULL");
            return TGCN_E_INVALID;
        }
        hs[l] = v.h;
        Cs[l] = v.C;
        tail = tail || (v.h % 4) != 0 || (v.C % 4) != 0;
        wide = wide || v.C > 64;
    }
    LevelsArgs A{};
    const size_t lds_bytes = sizeof(float) * levels_lds_floats(n_levels, hs, Cs, &A);
    if (lds_bytes > size_t(TGCN_FOLDIN_LEVELS_LDS_LIMIT)) {
        set_error("tgcn_foldin_levels: the staged W2 / Wh and the waves' slices need %zu bytes of LDS, a CU has %d "
                  "(tgcn_foldin_levels_lds_bytes)", lds_bytes, TGCN_FOLDIN_LEVELS_LDS_LIMIT);
        return TGCN_E_INVALID;
    }
    if (n_docs == 0) return TGCN_OK;
    if (!rowptr || !col || !val || !dis || !table || !aligned16(table)) {
        set_error("tgcn_foldin_levels: NULL pointer (rowptr, col, val, dis, table), or a table that is not 16-byte aligned");
        return TGCN_E_INVALID;
    }
    for (int l = 0; l < n_levels; ++l) {
        const tgcn_foldin_level &v = levels[l];
        if (!v.W2 || !v.b1 || !v.b2 || (l > 0 && !v.Wh)) {
            set_error("tgcn_foldin_levels: level %d: NULL pointer (only logits, pred, hidden and link_out may be NULL)", l + 1);
            return TGCN_E_INVALID;
        }
        if (!aligned16(v.W2) || (l > 0 && !aligned16(v.Wh)) || !aligned16(v.b1) ||
            !aligned16(v.b2) || !aligned16(v.logits) || !aligned16(v.hidden) || !aligned16(v.link_out)) {
            set_error("tgcn_foldin_levels: level %d: W2, Wh, b1, b2, logits, hidden and link_out must be 16-byte aligned",
                      l + 1);
            return TGCN_E_INVALID;
        }
        LevelK &K = A.lv[l];
        K.t1_col = static_cast<int>(v.t1_col), K.p_col = static_cast<int>(v.p_col), K.W2 = v.W2, K.Wh = l > 0 ? v.Wh : nullptr, K.b1 = v.b1, K.b2 = v.b2;
        K.logits = v.logits, K.hidden = v.hidden, K.link_out = v.link_out, K.pred = v.pred;
        K.ldw2 = v.ldw2, K.ldwh = v.ldwh, K.ldl = v.ldl, K.ldh = v.ldh, K.ldk = v.ldk;
        K.h = v.h, K.C = v.C, K.act = v.act, K.link = l > 0 ? v.link : TGCN_FOLDIN_LINK_SOFTMAX;
    }
    A.n_docs = n_docs, A.rowptr = rowptr, A.col = col, A.val = val, A.dis = dis, A.table = table, A.ldt = ldt;
    A.n_vocab = static_cast<int>(n_vocab), A.reference = degree_sum == TGCN_DEGREE_REFERENCE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return n_levels == 2 ? launch_levels_of<2>(A, tail, wide, lds_bytes, s) : launch_levels_of<3>(A, tail, wide, lds_bytes, s);
}

}  // extern "C"
