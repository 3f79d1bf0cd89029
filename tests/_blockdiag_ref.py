"""The one-launch block-diagonal products of pytextgcn_amd/csrc/blockdiag.hip restated in float64 with the mask of
tests/_dropout_hash.py, a pure-Python restatement of what the launchers choose, and the case lists the kernel tests share.
CPU only.  Test infrastructure; nothing under pytextgcn_amd/ imports this.

The restated choices are written from `tgcn_blockdiag_xw` and `tgcn_blockdiag_xw_grad`; they exist so that the tests can
say "every template instantiation and column group" about their case lists -- no test asks them what the right answer
is."""
import zlib
from functools import lru_cache

import numpy as np

import _dropout_hash as DH

FILL = 7.0                                      # what every output buffer holds before a call

# ---- the launchers' choices ------------------------------------------------------------------------------------------
T = 128                                         # kBdRows: the row tile of the forward and of dX
H_MAX = 256                                     # kBdMaxH
K_MAX = 128                                     # kBdMaxMembers
FWD_GROUP, FWD_LADDER = 256, (1, 2, 4, 8)       # kFwdGroup and with_tiles<1, 2, 4, 8>
DX_GROUP, DX_LADDER = 128, (1, 2, 4)            # kGzGroup
DW_GROUP, DW_LADDER = 128, (1, 2, 4)            # kBdWGroup
W_CHUNK, W_TARGET = 128, 512                    # kWChunk, kWTarget (fused_act.h: grad_w_split)
MAX_TILES = (1 << 24) - 1                       # kBdMaxTiles: 256-thread workgroups, fewer than 2^32 threads along x
# The grids: (row tiles, K) forward and dX -- a workgroup there never takes a second tile, and past MAX_TILES tiles the
# entry points refuse the call (no operand of that size exists) -- and (slices, K) for dW, where the slices ARE capped:
# grad_w_split(N, 32 K, kWTarget) hands out at most min(256, kWTarget / K) slices, so past that many 128-row chunks a
# workgroup walks more than one chunk (chunks_per_slice > 1) and the slice boundaries stop being the chunk boundaries.


def dw_slice_cap(K):
    """the most slices a dW launch has for K members"""
    return min(256, max(1, W_TARGET // K))


def dw_rows_past_cap(K):
    """the smallest row count at which a workgroup of dW takes a second chunk of rows"""
    return dw_slice_cap(K) * W_CHUNK + 1


def _ladder(tiles, ladder):
    return next((t for t in ladder if tiles <= t), ladder[-1])


def launches(h, widths):
    """The kernel instantiations one call of each product launches: {"fwd": [NT per column group], "dx": [...],
    "dw": [(TJ, NT) per column group]}."""
    n = max(widths)
    tj = 2 if h > 128 else 1
    return {"fwd": [_ladder((min(n - c, FWD_GROUP) + 31) // 32, FWD_LADDER) for c in range(0, n, FWD_GROUP)],
            "dx": [_ladder((min(n - c, DX_GROUP) + 31) // 32, DX_LADDER) for c in range(0, n, DX_GROUP)],
            "dw": [(tj, _ladder((min(n - c, DW_GROUP) + 31) // 32, DW_LADDER)) for c in range(0, n, DW_GROUP)]}


ALL_INSTANTIATIONS = ({("fwd", nt) for nt in FWD_LADDER} | {("dx", nt) for nt in DX_LADDER}
                      | {("dw", tj, nt) for tj in (1, 2) for nt in DW_LADDER})


def instantiations(h, widths):
    l = launches(h, widths)
    return {("fwd", nt) for nt in l["fwd"]} | {("dx", nt) for nt in l["dx"]} | {("dw",) + v for v in l["dw"]}


def dw_slices(N, K):
    """(slices, rows per slice) of the dW reduction: grad_w_split(N, 32 K, kWTarget)"""
    chunks = max(1, (N + W_CHUNK - 1) // W_CHUNK)
    want = dw_slice_cap(K)
    cps = (chunks + want - 1) // want
    return (chunks + cps - 1) // cps, cps * W_CHUNK


# ---- the layout ------------------------------------------------------------------------------------------------------
def layout(widths, lead=0, gap=0):
    """(starts, n_cols): segments at multiples of 4 columns as `perlabel.segment_layout` lays them, after `lead` pad
    columns and with `gap` more pad columns behind every segment"""
    starts, at = [], lead
    for c in widths:
        starts.append(at)
        at += ((c + 3) & ~3) + gap
    return starts, at


# ---- the float64 reference -------------------------------------------------------------------------------------------
def keep_scale(N, h, rate, seed, mask_row0):
    """s_k keep_k [N, h] in float64: the decisions of `dense.xw_dropout` on the member's own [N, h] block"""
    if rate == 0.0 or seed is None:
        return np.ones((N, h))
    rows = (np.arange(N, dtype=np.uint64) + np.uint64(mask_row0))[:, None]
    cols = np.arange(h, dtype=np.uint64)[None, :]
    return DH.keep_mask(int(seed), rows, cols, rate).astype(np.float64) / (1.0 - rate)


def products(X, W, G, h, starts, widths, rates, seeds, mask_row0=0):
    """(C [N, n_cols], dX [N, K h], colsum [K h], dW [h, n_cols]) in float64; `seeds` None: nobody drops anything.  Pad
    columns of C and dW are 0."""
    X, W, G = (np.asarray(a, dtype=np.float64) for a in (X, W, G))
    N, n_cols = X.shape[0], W.shape[1]
    C, dX, dW = np.zeros((N, n_cols)), np.zeros_like(X), np.zeros((h, n_cols))
    for k, (s, c) in enumerate(zip(starts, widths)):
        m = keep_scale(N, h, rates[k], None if seeds is None else seeds[k], mask_row0)
        a = m * X[:, k * h:(k + 1) * h]
        C[:, s:s + c] = a @ W[:, s:s + c]
        dX[:, k * h:(k + 1) * h] = m * (G[:, s:s + c] @ W[:, s:s + c].T)
        dW[:, s:s + c] = a.T @ G[:, s:s + c]
    return C, dX, dX.sum(0), dW


# ---- the cases -------------------------------------------------------------------------------------------------------
ROWS = (0, 1, 31, 33, T - 1, T, T + 1, 2 * T + 1)   # (the first row count past dW's slice cap depends on K: PAST_SLICE_CAP)
HIDDEN = (1, 3, 31, 32, 33, 100, 200, H_MAX)
# the lists of test_gpu_perlabel.py (they cross the 32-, 128- and 256-column edges) and one with 33..64 columns, the only
# width at which the ladders pick their two-tile instantiations
WIDTHS = ([1], [3, 4], [5] * 12, [64, 65, 1, 7], [257, 2], [40, 33])
EXACT_RATES = (0.0, 0.5, 0.75)                  # scales 1, 2 and 4
SEEDS = (0x1234567890ABCDE, -77, (1 << 40) + 12345, 5, -(1 << 62), 99, -1, -(1 << 63), (1 << 63) - 1, 0)
MASK_ROW0 = (0, (1 << 32) + 5)
OUTPUTS = ("all", "no-dx", "no-dw")


def _crc(*v):
    return zlib.crc32(repr(v).encode())


def seeds_for(K, salt=0):
    """K 64-bit seeds as Python ints in int64 range: the fixed list (negative ones, all 64 bits in use) and then hashes"""
    out = list(SEEDS[salt % len(SEEDS):] + SEEDS[:salt % len(SEEDS)])[:K]
    gen = np.random.default_rng(_crc("seeds", K, salt))
    out += [int(v) for v in gen.integers(-(1 << 63), (1 << 63) - 1, size=K - len(out), dtype=np.int64)]
    return out


def exact_cases(widths):
    """The exact cases of one width list: every h at a row count that cycles through ROWS, every row count at an h <= 128 and
    at an h > 128 (dW's two row tilings) that cycle through HIDDEN; mask_row0, the optional outputs, the lead / gap pad
    columns and seeds-or-none cycle with the case number.  Each: dict(N, h, widths, lead, gap, rates, salt, mask_row0,
    outputs, eval)."""
    K, out = len(widths), []
    low, high = [h for h in HIDDEN if h <= 128], [h for h in HIDDEN if h > 128]
    pairs = [(ROWS[(i + 3) % len(ROWS)], h) for i, h in enumerate(HIDDEN)] + \
            [(N, low[(i + 2) % len(low)]) for i, N in enumerate(ROWS)] + \
            [(N, high[i % len(high)]) for i, N in enumerate(ROWS)]
    for i, (N, h) in enumerate(pairs):
        rates = [EXACT_RATES[(k + i) % 3] for k in range(K)]
        out.append(dict(N=N, h=h, widths=list(widths), lead=(0, 4, 3)[i % 3], gap=(0, 0, 5)[i % 3], rates=rates, salt=i,
                        mask_row0=MASK_ROW0[i % 2], outputs=OUTPUTS[i % 3], eval=i % 7 == 6))
    return out


# more members than CrossValGCN's 64 allows (PerLabelGCN's case), and the cap
MANY_MEMBERS = (dict(N=33, h=3, widths=[5] * 64, lead=0, gap=0, rates=[EXACT_RATES[k % 3] for k in range(64)], salt=1,
                     mask_row0=0, outputs="all", eval=False),
                dict(N=T + 1, h=32, widths=[1] * K_MAX, lead=0, gap=0, rates=[EXACT_RATES[(k + 1) % 3] for k in range(K_MAX)],
                     salt=2, mask_row0=MASK_ROW0[1], outputs="all", eval=False))


def _past_cap(widths, h, i):
    K = len(widths)
    return dict(N=dw_rows_past_cap(K), h=h, widths=widths, lead=(0, 4)[i % 2], gap=(0, 5)[i % 2],
                rates=[EXACT_RATES[(k + i) % 3] for k in range(K)], salt=10 + i, mask_row0=MASK_ROW0[i % 2], outputs="all",
                eval=False)


# The first row count past dW's slice cap (a second chunk per workgroup) for every instantiation of k_bd_grad_w -- many
# members keep that row count small: 513 rows at K = 128, 1025 at K = 64 -- and the sweep's own K = 12 at 5377 rows.
PAST_SLICE_CAP = tuple(_past_cap(w, h, i) for i, (w, h) in enumerate((
    ([1] * 128, 8), ([1] * 128, 200), ([33] + [1] * 63, 100), ([33] + [1] * 63, H_MAX), ([65] + [1] * 63, 3),
    ([65] + [1] * 63, 200), ([5] * 12, 33))))


def all_exact_cases():
    return [c for w in WIDTHS for c in exact_cases(w)] + list(MANY_MEMBERS) + list(PAST_SLICE_CAP)


def partial_sum_bound(c):
    """an upper bound on |any partial sum| of the case with |X|, |W|, |G| <= 2 and s <= 4: 16 h in C, 16 n in dX, 16 N in
    dW and 16 n N in the column sums of dX"""
    n = max(c["widths"])
    return 16 * max(c["h"], n * max(c["N"], 1))


@lru_cache(maxsize=8)
def operands(N, h, K, n_cols, kind, salt=0):
    """(X [N, K h], W [h, n_cols], G [N, n_cols]) float32 on the CPU, left unchanged: small integers in [-2, 2] ("int") or
    `randn`"""
    gen = np.random.default_rng(_crc("ops", N, h, K, n_cols, kind, salt))
    if kind == "int":
        f = lambda *s: gen.integers(-2, 3, size=s).astype(np.float32)
    else:
        f = lambda *s: gen.standard_normal(s).astype(np.float32)
    return f(N, K * h), f(h, n_cols), f(N, n_cols)
