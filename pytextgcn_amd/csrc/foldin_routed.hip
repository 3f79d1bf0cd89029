// tgcn_foldin_routed -- documents outside the training graph through the per-label strategy (include/tgcn.h; DESIGN.md
// 4.2o): a top-level two-layer network picks the top label k, the document goes to label k's own two-layer network
// (perlabel_amazon.py, eval_perlabel.py:57-78).  The reference runs the strategy on graph nodes only.
//
// One wavefront per document, kFoldWaves documents per workgroup pass, grid-stride over the batch, as foldin.hip -- and the
// document's scalars, row accesses, wave-local LDS sync, u W2 epilogue, arg-max and the launch ARE foldin.hip's (foldin.h).
// The pass over the words is written out here as it is there: ONE body, run once per network the document
// meets -- the top network (TOP leaves), then the routed member -- in a loop that is not unrolled, so that nothing of the
// first run but the route is alive in the second.  Per document:
//   1. deg_d, dis_d, a_dd once.
//   2. TOP: the pass over the words gathers the top network's two segments of the combined table (16-byte loads, four
//      entries in flight, ids and a_j through v_readlane), u^0 -> the wave's LDS slice, u^0 W2^0 from LDS, z^0, the first
//      arg-max: the route.  Without TOP the route is read from `route_in` and no top segment is touched.
//   3. the route is wave-uniform and taken through readfirstlane: the member's column offsets, LDS offsets and C_k are
//      scalars.  A route outside [0, K) writes its "nobody" row and reads no table row.
//   4. the same pass over the same words with the member's column offsets; a_j is recomputed by doc_entry (its re-read of
//      col / val / dis hits the cache).  The arithmetic is that of step 2: fp32 FMA in CSR order.
//   5. u^k, u^k W2^k from LDS, z^k, the -inf fill behind C_k, the arg-max and the class map.
// W2 and b2 of the top network and of ALL K members are staged in LDS once per workgroup: any document may route anywhere.
// b1 is read from memory (one 16-byte load per lane and network, a cache hit): with it in LDS too the shape
// h = 256, C = {128, 4} would not fit the 160 KiB.
// Leaves (template): TOP = the top network is evaluated; TAIL = some h or C of a network that takes part is not a multiple
// of 4; WIDE = some such C > 64.  A document's arithmetic is a function of the widths, its own row and its route.
#include "foldin.h"

namespace tgcn {
namespace {

using namespace fold;

constexpr int kMaxMembers = TGCN_FOLDIN_MAX_MEMBERS;

struct MemberK {                          // network m: 0 = the top network, 1 + k = member k
    const float *W2, *b1, *b2;
    int ldw2;
    int t1_col, p_col;                    // where the network's T1 and P segments begin in a row of the table
    int w2_off;                           // floats from the start of LDS: W2 [r4(h C)], then b2 [r4(C)]
    int C_act;                            // C | act << 8
    int seg;                              // where the member's columns begin in class_map
};

struct RoutedArgs {
    int64_t n_docs;
    const int64_t *rowptr;
    const int32_t *col;
    const float *val;
    const float *dis;
    const float *table;
    const int32_t *route_in;
    const int64_t *class_map;
    int32_t *route_out;
    float *top_logits, *logits, *hidden;
    int64_t *pred;
    int64_t ldt, ldtl, ldl, ldh;
    int n_vocab, reference;
    int K, h_top, h_mem, c_max;           // c_max: the widest member, the width of a `logits` row
    int slice_off, slice, zs_off;         // floats: the first wave's slice, a slice's size, and zs inside a slice
    MemberK mb[kMaxMembers + 1];
};
static_assert(sizeof(RoutedArgs) <= 4096, "kernel arguments");

template <bool TOP, bool TAIL, bool WIDE>
__global__ __launch_bounds__(64 * kFoldWaves) void k_foldin_routed(const RoutedArgs A) {
    extern __shared__ float4 lds4[];
    float *const lds = reinterpret_cast<float *>(lds4);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));

    for (int m = TOP ? 0 : 1; m <= A.K; ++m) {
        const MemberK &V = A.mb[m];
        const int h = m ? A.h_mem : A.h_top, C = V.C_act & 255;
        float *const W2s = lds + V.w2_off;                            // [h, C], tight
        for (int i = threadIdx.x; i < h * C; i += 64 * kFoldWaves) {
            const int k = i / C;
            W2s[i] = V.W2[int64_t(k) * V.ldw2 + (i - k * C)];
        }
        float *const b2s = W2s + ((h * C + 3) & ~3);
        for (int i = threadIdx.x; i < ((C + 3) & ~3); i += 64 * kFoldWaves) b2s[i] = i < C ? V.b2[i] : 0.f;
    }
    __syncthreads();

    float *const us = lds + A.slice_off + wave * A.slice;            // this wave's u ...
    float *const zs = us + A.zs_off;                                  // ... and its gathered P sum
    const int c0 = 4 * lane;
    const int reference = A.reference;
    const int K = A.K;

    const int64_t stride = int64_t(gridDim.x) * kFoldWaves;
    for (int64_t d = int64_t(blockIdx.x) * kFoldWaves + wave; d < A.n_docs; d += stride) {
        const int64_t beg = A.rowptr[d], end = A.rowptr[d + 1];
        const float dd = doc_dis(A.val, beg, end, lane, reference);
        const float a_dd = doc_self_weight(dd);
        int route = 0;                                  // wave-uniform
#pragma unroll 1
        for (int run = TOP ? 0 : 1; run < 2; ++run) {
            if (!TOP) {
                route = __builtin_amdgcn_readfirstlane(A.route_in[d]);
                if (A.route_out && lane == 0) A.route_out[d] = route;
            }
            if (run == 1 && (route < 0 || route >= K)) {    // nobody: no table row is read
                if (A.logits) {
                    float *const out = A.logits + d * A.ldl;
                    if (lane < A.c_max) out[lane] = -INFINITY;
                    if (WIDE && lane + 64 < A.c_max) out[lane + 64] = -INFINITY;
                }
                if (A.hidden) store4<TAIL>(A.hidden + d * A.ldh, c0, A.h_mem, make_float4(0.f, 0.f, 0.f, 0.f));
                if (A.pred && lane == 0) A.pred[d] = -1;
                break;
            }
            const MemberK &V = A.mb[run ? 1 + route : 0];
            const int h = run ? A.h_mem : A.h_top, C = V.C_act & 255, act = V.C_act >> 8;
            const int H4 = (h + 3) & ~3, C4 = (C + 3) & ~3;
            const float *const tabT = A.table + V.t1_col, *const tabP = A.table + V.p_col;

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
                            const int64_t at = int64_t(lane_i(c, i + q)) * A.ldt;
                            av[q] = lane_f(a, i + q);
                            xt[q] = load4<TAIL>(tabT + at, c0, h);
                            xp[q] = load4<TAIL>(tabP + at, c0, C);
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
                    const int64_t at = int64_t(cq) * A.ldt;
                    const float4 xt = load4<TAIL>(tabT + at, c0, h);
                    const float4 xp = load4<TAIL>(tabP + at, c0, C);
                    fma4(accT, aq, xt);
                    fma4(accP, aq, xp);
                }
            }
            // u = act(sum + b1); columns at and beyond h are zero (zero loads, zero sums)
            const float4 u = bias_act4(accT, load4<TAIL>(V.b1, c0, h), act);
            if (c0 < H4) *reinterpret_cast<float4 *>(us + c0) = u;
            if (c0 < C4) *reinterpret_cast<float4 *>(zs + c0) = accP;
            if (run && A.hidden) store4<TAIL>(A.hidden + d * A.ldh, c0, h, u);
            wave_lds_sync();

            const bool on0 = lane < C, on1 = WIDE && lane + 64 < C;
            const float *const W2s = lds + V.w2_off, *const b2s = W2s + ((h * C + 3) & ~3);
            float y0, y1;
            u_times_w2<WIDE>(us, W2s + (on0 ? lane : 0), W2s + (on1 ? lane + 64 : 0), h, C, y0, y1);
            float z0 = -INFINITY, z1 = -INFINITY;
            if (on0) z0 = fmaf(a_dd, y0, zs[lane]) + b2s[lane];
            if (on1) z1 = fmaf(a_dd, y1, zs[lane + 64]) + b2s[lane + 64];
            float *const out = run ? A.logits : A.top_logits;
            if (out) {                                   // a member's row is -inf from C_k to the widest member's end
                const int wr = run ? A.c_max : C;
                float *const row = out + d * (run ? A.ldl : A.ldtl);
                if (lane < wr) row[lane] = z0;
                if (WIDE && lane + 64 < wr) row[lane + 64] = z1;
            }
            if (!run || A.pred) {
                float mx;
                const int bi = first_argmax(z0, z1, on0, on1, lane, mx);
                if (!run) {
                    route = __builtin_amdgcn_readfirstlane(bi);
                    if (A.route_out && lane == 0) A.route_out[d] = bi;
                } else if (lane == 0) {
                    A.pred[d] = A.class_map ? A.class_map[V.seg + bi] : int64_t(bi);
                }
            }
            wave_lds_sync();                             // the next run's (document's) stores follow this one's loads
        }
    }
}

inline size_t r4(size_t v) { return (v + 3) & ~size_t(3); }

// floats; h[0] == 0: no top network.  Fills the offsets of `A` when given.
size_t routed_lds_floats(int K, const int32_t *h, const int32_t *C, RoutedArgs *A) {
    size_t at = 0, hmax = 0, cmax = 0;
    for (int m = h[0] ? 0 : 1; m <= K; ++m) {
        if (A) A->mb[m].w2_off = static_cast<int>(at);
        at += r4(size_t(h[m]) * C[m]) + r4(C[m]);
        hmax = std::max(hmax, r4(h[m]));
        cmax = std::max(cmax, r4(C[m]));
    }
    if (A) {
        A->slice_off = static_cast<int>(at);
        A->slice = static_cast<int>(hmax + cmax);
        A->zs_off = static_cast<int>(hmax);
    }
    return at + size_t(kFoldWaves) * (hmax + cmax);
}

bool routed_widths_ok(int K, const int32_t *h, const int32_t *C) {
    if (K < 1 || K > kMaxMembers || !h || !C) return false;
    for (int m = 0; m <= K; ++m) {
        if (m == 0 && h[0] == 0) continue;
        if (h[m] < 1 || h[m] > kFoldMaxH || C[m] < 1 || C[m] > kFoldMaxC) return false;
        if (m > 1 && h[m] != h[1]) return false;
    }
    return true;
}

template <bool TOP, bool TAIL, bool WIDE>
int launch_routed(const RoutedArgs &A, size_t lds_bytes, hipStream_t s) {
    return launch_fold<k_foldin_routed<TOP, TAIL, WIDE>>(A, A.n_docs, TGCN_FOLDIN_LEVELS_LDS_LIMIT, lds_bytes, s);
}

template <bool TOP>
int launch_routed_of(const RoutedArgs &A, bool tail, bool wide, size_t lds_bytes, hipStream_t s) {
    if (tail)
        return wide ? launch_routed<TOP, true, true>(A, lds_bytes, s) : launch_routed<TOP, true, false>(A, lds_bytes, s);
    return wide ? launch_routed<TOP, false, true>(A, lds_bytes, s) : launch_routed<TOP, false, false>(A, lds_bytes, s);
}

}  // namespace
}  // namespace tgcn

extern "C" {

int64_t tgcn_foldin_routed_lds_bytes(int n_members, const int32_t *h, const int32_t *C) {
    using namespace tgcn;
    if (!routed_widths_ok(n_members, h, C)) return -1;
    return static_cast<int64_t>(sizeof(float) * routed_lds_floats(n_members, h, C, nullptr));
}

int tgcn_foldin_routed(int64_t n_docs, const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_vocab,
                       const float *dis, int degree_sum, const float *table, int64_t ldt, int n_members,
                       const tgcn_foldin_member *members, const int32_t *route_in, const int64_t *class_map,
                       int32_t *route_out, float *top_logits, int64_t ldtl, float *logits, int64_t ldl, int64_t *pred,
                       float *hidden, int64_t ldh, tgcn_stream stream) {
    using namespace tgcn;
    const int K = n_members;
    if (K < 1 || K > kMaxMembers || !members) {
        set_error("tgcn_foldin_routed: n_members=%d (1..%d) with a non-NULL `members`", K, kMaxMembers);
        return TGCN_E_INVALID;
    }
    if (n_docs < 0 || n_vocab < 1 || n_vocab > INT32_MAX || ldt < 4 || ldt > INT32_MAX || (ldt & 3) != 0) {
        set_error("tgcn_foldin_routed: bad size (n_docs=%lld n_vocab=%lld; ldt=%lld, a multiple of 4)", (long long)n_docs,
                  (long long)n_vocab, (long long)ldt);
        return TGCN_E_INVALID;
    }
    if (degree_sum != TGCN_DEGREE_ACCURATE && degree_sum != TGCN_DEGREE_REFERENCE) {
        set_error("tgcn_foldin_routed: unknown degree_sum %d", degree_sum);
        return TGCN_E_INVALID;
    }
    const bool top = route_in == nullptr;
    if (!route_out && !top_logits && !logits && !pred && !hidden) {
        set_error("tgcn_foldin_routed: no output is asked for (route_out, top_logits, logits, pred, hidden are all NULL)");
        return TGCN_E_INVALID;
    }
    if (!top && top_logits) {
        set_error("tgcn_foldin_routed: with route_in the top network is not evaluated: top_logits must be NULL");
        return TGCN_E_INVALID;
    }
    int32_t hs[kMaxMembers + 1], Cs[kMaxMembers + 1];
    bool tail = false, wide = false;
    int c_max = 0;
    for (int m = 0; m <= K; ++m) {
        const tgcn_foldin_member &v = members[m];
        hs[m] = v.h, Cs[m] = v.C;
        if (m == 0 && !top) {
            hs[0] = 0;                                   // entry 0 is not looked at
            continue;
        }
        if (v.h < 1 || v.h > kFoldMaxH || v.C < 1 || v.C > kFoldMaxC) {
            set_error("tgcn_foldin_routed: member %d: bad size (h=%d, 1..%d; C=%d, 1..%d)", m, v.h, kFoldMaxH, v.C, kFoldMaxC);
            return TGCN_E_INVALID;
        }
        if (m == 0 && v.C != K) {
            set_error("tgcn_foldin_routed: member 0 (the top network) has C=%d classes for %d routed members", v.C, K);
            return TGCN_E_INVALID;
        }
        if (m > 1 && v.h != members[1].h) {
            set_error("tgcn_foldin_routed: member %d: h=%d, the routed members share one hidden width (member 1: h=%d)", m, v.h,
                      members[1].h);
            return TGCN_E_INVALID;
        }
        if (v.act != TGCN_ACT_NONE && v.act != TGCN_ACT_RELU) {
            set_error("tgcn_foldin_routed: member %d: unknown act %d", m, v.act);
            return TGCN_E_INVALID;
        }
        if (v.t1_col < 0 || v.p_col < 0 || ((v.t1_col | v.p_col) & 3) != 0 || v.t1_col + v.h > ldt || v.p_col + v.C > ldt) {
            set_error("tgcn_foldin_routed: member %d: the segments must begin at multiples of 4 and end inside a table row "
                      "(t1_col=%lld h=%d p_col=%lld C=%d ldt=%lld)", m, (long long)v.t1_col, v.h, (long long)v.p_col, v.C,
                      (long long)ldt);
            return TGCN_E_INVALID;
        }
        if (v.ldw2 < v.C || v.ldw2 > INT32_MAX || (v.ldw2 & 3) != 0) {
            set_error("tgcn_foldin_routed: member %d: ldw2=%lld must cover C=%d and be a multiple of 4", m, (long long)v.ldw2,
                      v.C);
            return TGCN_E_INVALID;
        }
        tail = tail || (v.h % 4) != 0 || (v.C % 4) != 0;
        wide = wide || v.C > 64;
        if (m) c_max = std::max(c_max, v.C);
    }
    const int h_mem = members[1].h;
    const int64_t ltl = top_logits ? ldtl : 0, ll = logits ? ldl : 0, lh = hidden ? ldh : 0;
    if ((top_logits && ldtl < K) || (logits && ldl < c_max) || (hidden && ldh < h_mem) || ((ltl | ll | lh) & 3) != 0) {
        set_error("tgcn_foldin_routed: leading dimensions must cover their rows and be multiples of 4 (ldtl=%lld for %d top "
                  "classes, ldl=%lld for %d classes of the widest member, ldh=%lld for h=%d)", (long long)ltl, K, (long long)ll,
                  c_max, (long long)lh, h_mem);
        return TGCN_E_INVALID;
    }
    RoutedArgs A{};
    const size_t lds_bytes = sizeof(float) * routed_lds_floats(K, hs, Cs, &A);
    if (lds_bytes > size_t(TGCN_FOLDIN_LEVELS_LDS_LIMIT)) {
        set_error("tgcn_foldin_routed: the staged W2 / b2 of every member and the waves' slices need %zu bytes of LDS, a CU "
                  "has %d (tgcn_foldin_routed_lds_bytes)", lds_bytes, TGCN_FOLDIN_LEVELS_LDS_LIMIT);
        return TGCN_E_INVALID;
    }
    if (n_docs == 0) return TGCN_OK;
    if (!rowptr || !col || !val || !dis || !table || !aligned16(table)) {
        set_error("tgcn_foldin_routed: NULL pointer (rowptr, col, val, dis, table), or a table that is not 16-byte aligned");
        return TGCN_E_INVALID;
    }
    if (!aligned16(top_logits) || !aligned16(logits) || !aligned16(hidden)) {
        set_error("tgcn_foldin_routed: top_logits, logits and hidden must be 16-byte aligned");
        return TGCN_E_INVALID;
    }
    int seg = 0;
    for (int m = top ? 0 : 1; m <= K; ++m) {
        const tgcn_foldin_member &v = members[m];
        if (!v.W2 || !v.b1 || !v.b2) {
            set_error("tgcn_foldin_routed: member %d: NULL pointer (W2, b1, b2)", m);
            return TGCN_E_INVALID;
        }
        if (!aligned16(v.W2) || !aligned16(v.b1) || !aligned16(v.b2)) {
            set_error("tgcn_foldin_routed: member %d: W2, b1 and b2 must be 16-byte aligned", m);
            return TGCN_E_INVALID;
        }
        MemberK &M = A.mb[m];
        M.W2 = v.W2, M.b1 = v.b1, M.b2 = v.b2, M.ldw2 = static_cast<int>(v.ldw2);
        M.t1_col = static_cast<int>(v.t1_col), M.p_col = static_cast<int>(v.p_col);
        M.C_act = v.C | (v.act << 8);
        M.seg = seg;
        if (m) seg += static_cast<int>(r4(v.C));
    }
    A.n_docs = n_docs, A.rowptr = rowptr, A.col = col, A.val = val, A.dis = dis, A.table = table, A.ldt = ldt;
    A.route_in = route_in, A.class_map = class_map, A.route_out = route_out, A.top_logits = top_logits, A.logits = logits;
    A.hidden = hidden, A.pred = pred, A.ldtl = ldtl, A.ldl = ldl, A.ldh = ldh;
    A.n_vocab = static_cast<int>(n_vocab), A.reference = degree_sum == TGCN_DEGREE_REFERENCE;
    A.K = K, A.h_top = top ? members[0].h : 0, A.h_mem = h_mem, A.c_max = c_max;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return top ? launch_routed_of<true>(A, tail, wide, lds_bytes, s) : launch_routed_of<false>(A, tail, wide, lds_bytes, s);
}

}  // extern "C"
