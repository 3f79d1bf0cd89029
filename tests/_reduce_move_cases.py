"""Cases of the exact sweeps over csrc/colsum.hip (`tgcn_colsum`, `tgcn_act_grad`) and csrc/rows.hip (`tgcn_rows_gather`,
`tgcn_rows_scatter`, `tgcn_rows_reduce_ranked`) of tests/test_gpu_reduce_move_exact.py: a pure-Python restatement of what
the launchers choose, the case lists, integer operands and int64 references.  CPU only: numpy; nothing here imports
torch.cuda or the library.  Test infrastructure; tests/test_reduce_move_cases.py keeps the lists honest.

Operands are integers in [-7, 7] and every case has 7 * n_rows < 2^24, so every partial sum in any order is an integer that
fp32 holds exactly: the kernels are compared bit for bit, whatever their summation order."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

FILL = 7.0                                      # what every output buffer holds before a call (the arenas of tests/_arena.py)
ACT_NONE, ACT_RELU = 0, 1                       # include/tgcn.h TGCN_ACT_NONE / TGCN_ACT_RELU


def _seed(*v):
    return zlib.crc32(repr(v).encode())


# ---- colsum.hip: the launchers' choice -------------------------------------------------------------------------------
COLSUM_MAX_BLOCKS = 2048                        # colsum.hip:219 `if (nb > 2048) nb = 2048`
COLSUM_ROWS_PER_BLOCK = 256                     # colsum.hip:217 `nb = (n_rows + 255) / 256`
COLSUM_LEAVES = ((4, 16), (4, 32), (4, 64), (1, 64))       # (VEC, LPR) of k_colsum_partial / k_relu_grad
COLSUM_EDGES = ((64, 68), (128, 132), (256, 260))          # F: 16 | 32 lanes, 32 | 64 lanes, one | two column tiles of 64 lanes


def colsum_blocks(n):
    """colsum.hip:216-221 `nb = (n_rows + 255) / 256`, clamped to [1, 2048]"""
    return min(COLSUM_MAX_BLOCKS, max(1, (n + 255) // 256))


def colsum_leaf(F, vec4):
    """(VEC, LPR, column tiles) of launch_colsum (colsum.hip:225-238) and launch_relu_grad (:248-262): `vec4 && F <= 64` ->
    <4, 16>, `vec4 && F <= 128` -> <4, 32>, `vec4` -> <4, 64> with (F + 255) / 256 tiles, else <1, 64> with (F + 63) / 64"""
    if vec4 and F <= 64:
        return 4, 16, 1
    if vec4 and F <= 128:
        return 4, 32, 1
    if vec4:
        return 4, 64, (F + 255) // 256
    return 1, 64, (F + 63) // 64


def pass_rows(leaf):
    """rows of one pass of a workgroup, `4 * RPW` with RPW = 64 / LPR; the unrolled loop strides UN = 4 of them"""
    return 4 * (64 // leaf[1])


def final_unrolled(nb):
    """(does any wave of k_colsum_final run its eight-deep loop, does any run the tail behind it): colsum.hip:195-202 `for (;
    b + 7 * 16 < nb; b += 8 * 16)` from b = wave, then `for (; b < nb; b += 16)`"""
    deep = nb > 112
    tail = any((w + ((nb - w - 113) // 128 + 1) * 128 if w + 112 < nb else w) < nb for w in range(16))
    return deep, tail


ColCase = namedtuple("ColCase", "F n pad off")
ColCase.__doc__ = """tgcn_colsum of an [n, F] matrix with rows of F + pad floats that starts `off` floats into a 16-byte aligned buffer"""
ActCase = namedtuple("ActCase", "act F n pada offa padg offg sums")
ActCase.__doc__ = """tgcn_act_grad: A [n, F + pada] at `offa`, G [n, F + padg] at `offg`, with the column sums or without"""

COL_F = (1, 3, 4, 64, 68, 128, 132, 256, 260, 65, 129, 516)
COL_BLOCKS = (1, 16, 17, 112, 113, 128, 129, 2048)          # k_colsum_final's eight-deep unroll and its tail
COL_OVER = COLSUM_MAX_BLOCKS * COLSUM_ROWS_PER_BLOCK + 1    # 524 289: a workgroup owns 257 rows
LEAF_F = {(4, 16): 64, (4, 32): 128, (4, 64): 260, (1, 64): 65}


def col_is_vec4(c):
    return c.F % 4 == 0 and (c.F + c.pad) % 4 == 0 and c.off % 4 == 0


def col_layouts(F):
    """(pad, off): for F % 4 == 0 two that keep 16-byte rows, one odd stride, one shifted base; otherwise dense, padded to
    16-byte rows (F alone forces the scalar leaf) and odd"""
    return ((0, 0), (4, 0), (1, 0), (0, 1)) if F % 4 == 0 else ((0, 0), (-F % 4, 0), (5, 1))


def row_counts(leaf):
    """0, 1, one pass +- 1, the unrolled loop's stride (four passes) +- 1, two strides and one row, three passes and one row
    (the unrolled loop's own condition `r + 3 * pass < r_end`), and two workgroups"""
    p = pass_rows(leaf)
    return (0, 1, p - 1, p, p + 1, 3 * p, 3 * p + 1, 4 * p - 1, 4 * p, 4 * p + 1, 8 * p + 1, 257)


def rows_for_blocks(nb):
    return nb * COLSUM_ROWS_PER_BLOCK - 5 if nb > 1 else 251


@lru_cache(maxsize=None)
def col_cases():
    out = []
    for F in COL_F:
        for pad, off in col_layouts(F):
            leaf = colsum_leaf(F, col_is_vec4(ColCase(F, 1, pad, off)))[:2]
            ns = row_counts(leaf) if F == LEAF_F[leaf] or F in (3, 4) else (1, 4 * pass_rows(leaf) + 1, 257)
            out += [ColCase(F, n, pad, off) for n in ns]
    for F in (4, 3):
        out += [ColCase(F, rows_for_blocks(nb), 0, 0) for nb in COL_BLOCKS] + [ColCase(F, COL_OVER, 0, 0)]
    out += [ColCase(F, rows_for_blocks(129), pad, 0) for F, pad in ((64, 0), (128, 4), (260, 0), (65, 0))]
    return tuple(dict.fromkeys(out))


def act_is_vec4(c):
    return c.F % 4 == 0 and (c.F + c.pada) % 4 == 0 and (c.F + c.padg) % 4 == 0 and c.offa % 4 == 0 and c.offg % 4 == 0


def act_layouts(F):
    """(pada, offa, padg, offg): A's stride and base apart from G's"""
    if F % 4 == 0:
        return ((0, 0, 0, 0), (4, 0, 8, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0, 1, 0, 0), (0, 0, 0, 1))
    return ((0, 0, 0, 0), (-F % 4, 0, -F % 4, 0), (5, 1, 2, 3))


@lru_cache(maxsize=None)
def act_cases():
    out = []
    for F in COL_F:
        for lay in act_layouts(F):
            leaf = colsum_leaf(F, act_is_vec4(ActCase(ACT_RELU, F, 1, *lay, True)))[:2]
            ns = row_counts(leaf) if F == LEAF_F[leaf] or F in (3, 4) else (1, 4 * pass_rows(leaf) + 1, 257)
            out += [ActCase(ACT_RELU, F, n, *lay, sums) for n in ns for sums in (True, False)]
        out += [ActCase(ACT_NONE, F, n, *act_layouts(F)[1], sums) for n in (0, 1, 257) for sums in (True, False)]
    for F in (4, 3):
        out += [ActCase(ACT_RELU, F, rows_for_blocks(nb), 0, 0, 0, 0, True) for nb in COL_BLOCKS]
        out += [ActCase(ACT_RELU, F, COL_OVER, 0, 0, 0, 0, sums) for sums in (True, False)]
    return tuple(dict.fromkeys(out))


def col_leaf_of(c):
    return colsum_leaf(c.F, act_is_vec4(c) if isinstance(c, ActCase) else col_is_vec4(c))[:2]


def by_col_leaf(cases):
    out = {leaf: [] for leaf in COLSUM_LEAVES}
    for c in cases:
        out[col_leaf_of(c)].append(c)
    return out


def col_leaf_id(leaf):
    return f"lpr{leaf[1]}-{'v4' if leaf[0] == 4 else 'scalar'}"


@lru_cache(maxsize=2)
def _ints(n, F, tag):
    return np.random.default_rng(_seed(tag, n, F)).integers(-7, 8, size=(n, F)).astype(np.float32)


def col_operand(c):
    """G: integers in [-7, 7]; the reference: their int64 column sums"""
    assert 7 * c.n < 2 ** 24
    G = _ints(c.n, c.F, "colsum")
    return G, G.astype(np.int64).sum(0)


def act_operands(c):
    """A: integers in [-7, 7] with -0.0 and NaN sprinkled in (0, -0.0 and NaN keep the gate closed); G: integers, NaN exactly
    where the gate is closed (TGCN_ACT_RELU; no NaN under TGCN_ACT_NONE, whose gate is always open).  Returns (A, G, gated
    G -- +0.0 where the gate is closed --, its int64 column sums)"""
    assert 7 * c.n < 2 ** 24
    gen = np.random.default_rng(_seed("act", c.n, c.F))
    A = _ints(c.n, c.F, "act-a").copy()
    what = gen.integers(0, 8, size=A.shape)
    A[what == 0] = np.float32(-0.0)
    A[what == 1] = np.float32(np.nan)
    G = _ints(c.n, c.F, "act-g").copy()
    if c.act == ACT_NONE:
        return A, G, G, G.astype(np.int64).sum(0)
    open_ = A > 0
    want = np.where(open_, G, np.float32(0.0)).astype(np.float32)
    G[~open_] = np.float32(np.nan)
    return A, G, want, want.astype(np.int64).sum(0)


# ---- rows.hip: the launchers' choice ---------------------------------------------------------------------------------
ROW_WAVES = 4                                   # rows.hip:38 `constexpr int kRowWaves = 4` (rows per workgroup)
ROWS_MAX_BLOCKS = 256 * 32                      # rows.hip:81 `min((n + kRowWaves - 1) / kRowWaves, 256 * 32)`
ROWS_CAP = ROWS_MAX_BLOCKS * ROW_WAVES          # 32 768 rows: above it a wave takes a second row
ROW_OPS = ("gather", "scatter", "reduce")
ROW_LEAVES = tuple((op, v4) for op in ROW_OPS for v4 in (True, False))
ROW_F = (1, 3, 4, 252, 256, 260, 516)
ROW_N = (0, 1, 5)
ROW_BIG_F = (4, 7)
BAD_INDEX = (-1, "n", 1 << 40)                  # "n": the row count of the indexed buffer


def rows_grid(n):
    """rows.hip:80-82 `max(1, min((n + kRowWaves - 1) / kRowWaves, 256 * 32))`"""
    return max(1, min((n + ROW_WAVES - 1) // ROW_WAVES, ROWS_MAX_BLOCKS))


def rows_vec4(F, lda, ldb, offa, offb):
    """rows.hip:84-87 `F % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && ((a | b) % 16) == 0`"""
    return F % 4 == 0 and lda % 4 == 0 and ldb % 4 == 0 and offa % 4 == 0 and offb % 4 == 0


RowCase = namedtuple("RowCase", "op F n pads offs padd offd skip W step")
RowCase.__doc__ = """one call of tgcn_rows_<op>: n moved rows of F floats; the source rows ([n_src, F + pads] at `offs`: x, or
recv) and the destination rows (F + padd at `offd`: out, or y); `skip`: out-of-range indices at the first, a middle and the
last position; W ranks and the row step of the ranked reduction (0 elsewhere)"""


def row_layouts(F):
    """(pads, offs, padd, offd): source and destination strided and misaligned apart from each other"""
    if F % 4 == 0:
        return ((0, 0, 0, 0), (4, 0, 8, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))
    return ((0, 0, 0, 0), (-F % 4, 0, -F % 4, 0), (1, 1, 2, 3))


def row_is_vec4(c):
    return rows_vec4(c.F, c.F + c.pads, c.F + c.padd, c.offs, c.offd)


@lru_cache(maxsize=None)
def row_cases():
    out = []
    for F in ROW_F:
        for lay in row_layouts(F):
            for n in ROW_N:
                for skip in (False, True):
                    out += [RowCase(op, F, n, *lay, skip, 0, 0) for op in ("gather", "scatter")]
                    out += [RowCase("reduce", F, n, *lay, skip, W, step) for W, step in ((1, 1), (2, 3), (8, 1))]
    for F in ROW_BIG_F:
        lay = (4, 0, 4, 0) if F % 4 == 0 else (0, 0, 0, 0)
        for n in (ROWS_CAP, ROWS_CAP + 1):
            out += [RowCase(op, F, n, *lay, True, 0, 0) for op in ("gather", "scatter")] + [RowCase("reduce", F, n, *lay, True, 2, 3)]
    return tuple(dict.fromkeys(out))


def by_row_leaf(cases):
    out = {leaf: [] for leaf in ROW_LEAVES}
    for c in cases:
        out[(c.op, row_is_vec4(c))].append(c)
    return out


def row_leaf_id(leaf):
    return f"{leaf[0]}-{'v4' if leaf[1] else 'scalar'}"


ROW0 = 2                                        # first row of y that the ranked reduction adds to
SPARE = 3                                       # rows of an indexed buffer that no index names


def _with_bad(idx, n_indexed, skip):
    """out-of-range values at the first, the last and a middle position (fewer where n is smaller)"""
    idx = idx.astype(np.int64)
    bad = np.zeros(len(idx), dtype=bool)
    if skip and len(idx):
        for pos, v in zip(dict.fromkeys((0, len(idx) - 1, len(idx) // 2)), BAD_INDEX):
            idx[pos] = n_indexed if v == "n" else v
            bad[pos] = True
    return idx, bad


def move_operands(c):
    """gather: (x [n + 3, F], idx descending with duplicates, out-of-range where `skip`, want [n, F] with FILL in the skipped
    rows).  scatter: (x [n, F], idx a partial permutation of n + 3 rows, want [n + 3, F] with FILL in the rows nobody names)"""
    gen = np.random.default_rng(_seed("move", *c))
    n_indexed = c.n + SPARE
    if c.op == "gather":
        x = _ints(n_indexed, c.F, "rows").copy()
        idx = np.sort(gen.integers(0, n_indexed, size=c.n))[::-1].copy()
        if c.n >= 2:
            idx[1] = idx[0]
        idx, bad = _with_bad(idx, n_indexed, c.skip)
        want = np.full((c.n, c.F), FILL, dtype=np.float32)
        want[~bad] = x[idx[~bad]]
    else:
        x = _ints(c.n, c.F, "rows").copy()
        idx, bad = _with_bad(gen.permutation(n_indexed)[:c.n], n_indexed, c.skip)
        want = np.full((n_indexed, c.F), FILL, dtype=np.float32)
        want[idx[~bad]] = x[~bad]
    return x, idx, want, n_indexed


def reduce_operands(c, floats=False):
    """(recv [n_recv, F], inv int32 [W, n], y [n_y, F], want [n_y, F], n_recv): table entries of -1, n_recv and n_recv + 5
    are skipped; every third row has no rank at all.  Integer operands with an int64 reference -- or, with `floats`, random
    fp32 operands and the documented order evaluated in fp32: zero, plus the ranks in order, then one add into y.
    y holds -0.0 here and there: y + 0 is +0.0 there."""
    gen = np.random.default_rng(_seed("reduce", *c, floats))
    n_recv = c.n * c.W // 2 + 1 if c.n else 0
    n_y = ROW0 + max(c.n - 1, 0) * c.step + 1 + SPARE
    draw = (lambda r: gen.standard_normal((r, c.F), dtype=np.float32)) if floats else (lambda r: gen.integers(-7, 8, size=(r, c.F)).astype(np.float32))
    recv, y = draw(n_recv), draw(n_y)
    y[gen.random(y.shape) < 0.1] = np.float32(-0.0)
    inv = gen.integers(0, max(n_recv, 1), size=(c.W, c.n)).astype(np.int64)
    inv[gen.random(inv.shape) < 0.3] = -1
    inv[:, 2::3] = -1                                           # rows that no rank has
    if c.skip and c.n:
        inv[0, 0], inv[-1, -1] = n_recv, n_recv + 5
    inv = inv.astype(np.int32)
    ok = (inv >= 0) & (inv < n_recv)
    rows = ROW0 + np.arange(c.n) * c.step
    want = y.copy()
    if floats:
        acc = np.zeros((c.n, c.F), dtype=np.float32)
        for q in range(c.W):
            acc[ok[q]] = acc[ok[q]] + recv[inv[q][ok[q]]]
        want[rows] = y[rows] + acc
        assert want.dtype == np.float32
    else:
        acc = np.zeros((c.n, c.F), dtype=np.int64)
        for q in range(c.W):
            acc[ok[q]] += recv[inv[q][ok[q]]].astype(np.int64)
        want[rows] = (y[rows].astype(np.int64) + acc).astype(np.float32)       # (+0.0 where the total is zero)
    return recv, inv, y, want, n_recv
