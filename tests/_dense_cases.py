"""Cases of the exact sweep over the dense kernels (tests/test_gpu_dense_exact.py): operands of small integers stored as
fp32, the independent reference (float64 on the host), the strided layouts and the generated case list.  CPU only: numpy
and tests/_dropout_hash.py; nothing here imports torch.cuda or the library.  Test infrastructure.

Why the comparison may be bit for bit: a product of small integers and every partial sum of such products is an integer
of magnitude <= max|a| * max|b| * (reduction length) * (dropout scale, a power of two); below 2^24 every such integer IS
an fp32 value, so no addition rounds and ANY summation order (MFMA steps, k chunks, partial tiles, column sums over
workgroups) returns the same bits.  `exact_bound` states that bound per case; tests/test_dense_cases.py asserts it for
the whole list.

The boundaries are NAMED here (from the dispatch of csrc/dense.hip as include/tgcn.h documents it); the C++ predicate
is deliberately not restated."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from _dropout_hash import keep_mask

EXACT_LIMIT = 1 << 24
SEED = 0x9E3779B97F4A7C15                       # the 64-bit dropout seed of every case (upper bit set: a negative int64)

# ---- named boundaries -----------------------------------------------------------------------------------------------
# result width n: the 32-column tiles (1..8 of them in one launch) and the one-launch limit of 256 columns
N_EDGES = ((32, 33), (64, 65), (96, 97), (128, 129), (192, 193), (224, 225), (256, 257))
# reduction length k (nn / nt) = width of A: k % 8 (the generic loop's last step), the unrolled k = 200 kernels, the nt
# kernel of 216 < k <= 224, one k chunk (256), two chunks and a ragged third (512 / 513)
K_MOD8 = tuple(range(1, 9))
K_EDGES = ((199, 200), (200, 201), (216, 217), (224, 225), (256, 257), (512, 513))
# the LDS threshold of one launch: k = 160, n = 256 is 160 KB to the byte; with column sums it moves by 4 * n_pad floats
LDS_EDGE = ((160, 256), (168, 256))
LDS_EDGE_COLSUM = ((152, 256), (160, 256))
# shapes the library has special kernels or column groups for (GCN layers; DBpedia's 219 classes)
SPECIAL_PAIRS = ((200, 64), (64, 200), (64, 219), (200, 219), (219, 200), (217, 96), (224, 65), (220, 128), (513, 257),
                 (257, 129), (260, 131), (100, 91))
K_PIVOTS = (7, 64, 200)      # generic loop with a ragged last step / the block-pipelined candidates / the unrolled kernels
N_PIVOTS = (33, 97, 224)     # two tiles / four tiles (the column-group kernels) / seven tiles

FORMS = {"nn": ("plain", "hashed", "recorded"),
         "nt": ("plain", "hashed", "colsum", "colsum_hashed", "colsum_recorded"),
         "tn": ("plain", "hashed", "recorded")}
LAYOUTS = ("tight", "pad", "odd", "shift")
N_AXIS_ROWS = (0, 1, 31, 32, 33, 127, 129, 1024, 1025)        # every row count at every (k, n), form and layout of the sweep
# One pass of a persistent nn / nt grid covers 4 blocks of 32 rows per workgroup, and a grid is at most 256 CUs x 4
# resident workgroups: 4 * 256 * 4 * 32 = 131 072 rows.  Beyond that the grid loop runs whatever the occupancy.
ROWS_OF_ONE_GRID_PASS = 4 * 256 * 4 * 32
N_PERSISTENT = 200_003
# the nt product that masks from the record runs two workgroups per CU (a grid of 512: one pass covers 65 536 rows); its
# column sums stay exact only while 64 * 2 * N < 2^24, so that case sits at 130 001 rows: two passes of ITS grid
ROWS_OF_ONE_RECORD_GRID_PASS = 4 * 256 * 2 * 32
N_PERSISTENT_RECORD = 130_001
N_TN_SATURATED = 600_001     # past 512 * 1024 rows: tn_blocks stays at 512 partial tiles

Case = namedtuple("Case", "family form N k n layout p amax keys foreign", defaults=(False,))
Case.__doc__ = """family nn / nt / tn, form (FORMS), the call's N, k, n, the layout (LAYOUTS), the dropout rate (None without
dropout), the largest |entry| of both operands, the dropout row keys (split, key0, key1) or None, and `foreign`: the record
handed to a consumer holds the mask of ANOTHER seed (FOREIGN_SEED) and the reference follows the record, not the hash."""
FOREIGN_SEED = 0x0123456789ABCDEF


def case_id(c):
    s = f"{c.family}-{c.form}-N{c.N}-k{c.k}-n{c.n}-{c.layout}"
    if c.p is not None and c.p not in (0.5, 0.75):
        s += f"-p{c.p:g}"
    return s + ("-keyed" if c.keys else "") + ("-foreign" if c.foreign else "")


def _h(*v):
    return zlib.crc32(repr(v).encode())


def has_drop(form):
    return form in ("hashed", "recorded", "colsum_hashed", "colsum_recorded")


def has_colsum(form):
    return form.startswith("colsum")


def scale_of(p):
    return 1.0 if p is None else (0.0 if p >= 1.0 else 1.0 / (1.0 - p))


def exact_bound(c):
    """An upper bound of every intermediate and final value of the case: max|a| * max|b| * reduction length * dropout
    scale (reduction k for nn / nt, N for tn), times N again for the column sums of an nn / nt result."""
    red = c.k if c.family in ("nn", "nt") else c.N
    b = c.amax * c.amax * max(red, 1) * max(scale_of(c.p), 1.0)
    if has_colsum(c.form):
        b *= max(c.N, 1)
    return b


def make_case(family, form, N, k, n, layout, p="auto", keys=None, foreign=False):
    """p = "auto": 0.5 or 0.75 (scales 2 and 4, both exact) by a hash of the shape; entries as wide as the bound allows."""
    if not has_drop(form):
        p = None
    elif p == "auto":
        p = 0.75 if _h(family, k, n) % 3 == 0 else 0.5
    for amax in (3, 2, 1):
        c = Case(family, form, N, k, n, layout, p, amax, keys, foreign)
        if exact_bound(c) < EXACT_LIMIT:
            return c
    raise ValueError(f"no exact operands for {family} {form} N={N} k={k} n={n}: bound {exact_bound(c):.3g} >= 2^24")


# ---- operands and reference ----------------------------------------------------------------------------------------
def _ints(gen, rows, cols, amax):
    """integers in [-amax, amax] as float64, asymmetric (no structure a transposed fragment map would keep), with no
    all-zero row or column (a dropped k step or row then changes the result)"""
    m = gen.integers(-amax, amax + 1, size=(rows, cols)).astype(np.float64)
    if rows and cols:
        zr = np.flatnonzero(~m.any(1))
        m[zr, zr % cols] = 1.0
        zc = np.flatnonzero(~m.any(0))
        m[zc % rows, zc] = 1.0
    return m


def shapes(c):
    """(rows, width) of A, of the second operand (B of nn: [k, n]; B of nt: [n, k]; G of tn: [N, n]) and of the result"""
    if c.family == "nn":
        return (c.N, c.k), (c.k, c.n), (c.N, c.n)
    if c.family == "nt":
        return (c.N, c.k), (c.n, c.k), (c.N, c.n)
    return (c.N, c.k), (c.N, c.n), (c.k, c.n)


def mask_shape(c):
    """the matrix the dropout masks: A [N x k] for nn and tn, the result [N x n] for nt"""
    return (c.N, c.n) if c.family == "nt" else (c.N, c.k)


def keep_of(N, width, p, keys=None, seed=SEED):
    """keep decisions of the documented hash (tests/_dropout_hash.py) over [N x width]; row i of the matrix is mask row
    i + key0 below `split`, i + key1 from there on (tgcn_set_dropout_row_keys)"""
    rows = np.arange(N, dtype=np.uint64)
    if keys:
        split, key0, key1 = keys
        rows = rows + np.where(rows < np.uint64(split), np.uint64(key0), np.uint64(key1))
    return keep_mask(seed, rows[:, None], np.arange(width, dtype=np.uint64)[None, :], p)


@lru_cache(maxsize=8)
def _reference(family, form, N, k, n, p, amax, keys, foreign):
    c = Case(family, form, N, k, n, "tight", p, amax, keys, foreign)
    gen = np.random.default_rng(_h(family, N, k, n, amax))
    sa, sb, _ = shapes(c)
    a, b = _ints(gen, sa[0], sa[1], amax), _ints(gen, sb[0], sb[1], amax)
    s = scale_of(p)
    keep = keep_of(*mask_shape(c), p, keys, FOREIGN_SEED if foreign else SEED) if p is not None else None
    if family == "nn":
        res = (np.where(keep, a, 0.0) * s if p is not None else a) @ b
    elif family == "nt":
        res = a @ b.T
        if p is not None:
            res = np.where(keep, res, 0.0) * s
    else:
        res = (np.where(keep, a, 0.0) if p is not None else a).T @ b
        if p is not None:
            res = res * s
    res = res + 0.0                                                   # no negative zeros in the reference
    out = {"a": a.astype(np.float32), "b": b.astype(np.float32), "keep": keep, "colsum": None}
    vals = [res]
    if has_colsum(form):
        out["colsum"] = res.sum(0) + 0.0
        vals.append(out["colsum"])
    for v in vals:                                                    # the stated condition, checked on the actual numbers
        assert v.size == 0 or np.abs(v).max() < EXACT_LIMIT, "reference leaves the exact fp32 integers"
        assert np.array_equal(v, np.rint(v))
    out["c"] = res.astype(np.float32)
    if out["colsum"] is not None:
        out["colsum"] = out["colsum"].astype(np.float32)
    return out


def reference(c):
    """dict: a, b (fp32 operands), c (fp32 result), colsum (fp32 [n] or None), keep (bool mask or None); cached, the
    layouts of one shape share it"""
    return _reference(c.family, c.form, c.N, c.k, c.n, c.p, c.amax, c.keys, c.foreign)


# ---- the recorded mask (layout of include/tgcn.h) ---------------------------------------------------------------
def mask_words(width):
    """32-bit words per row of the record of a [N x width] operand: 2 * ceil(ceil(width / 8) / 8)"""
    return 2 * (((width + 7) // 8 + 7) // 8)


def _word_bit(width):
    c = np.arange(width)
    return ((c // 4) & 1) * (mask_words(width) // 2) + c // 64, 4 * ((c // 8) % 8) + (c & 3)


def encode_record(keep):
    """uint32 [N x mask_words] from a bool mask: column c is bit 4 ((c / 8) % 8) + (c & 3) of word ((c / 4) & 1) * (words /
    2) + c / 64; bits of columns that do not exist stay 0"""
    N, width = keep.shape
    word, bit = _word_bit(width)
    rec = np.zeros((N, mask_words(width)), dtype=np.uint32)
    np.bitwise_or.at(rec, (np.arange(N)[:, None], word[None, :]), keep.astype(np.uint32) << bit[None, :].astype(np.uint32))
    return rec


def decode_record(rec, width):
    word, bit = _word_bit(width)
    return ((rec[:, word] >> bit[None, :].astype(np.uint32)) & 1).astype(bool)


# ---- layouts --------------------------------------------------------------------------------------------------------
Layout = namedtuple("Layout", "lda off_a ldb off_b ldc off_c mask_stride off_mask")


def _r4(v):
    return (v + 3) // 4 * 4


def layout(c):
    """Leading dimensions (elements) and base misalignments (elements past a 16-byte boundary) of a case's buffers.
    tight: ld == width;  pad: width rounded up to 4, plus 4;  odd: NOT a multiple of 4 and a base that is 4-byte but not
    16-byte aligned;  shift: pad's leading dimensions (multiples of 4) on a base 4 bytes past a 16-byte boundary, so that the
    base alignment ALONE decides -- the last two for the arguments include/tgcn.h leaves free (ldb, ldc everywhere; lda, ldg
    of tn; the mask record).  A of nn / nt keeps the header's contract (lda % 4 == 0, 16-byte aligned): tight is then
    round_up(k, 4) (the NaN gap sits right behind a row whose k is not a multiple of 4), odd is round_up(k, 4) + 8."""
    (_, wa), (_, wb), (_, wc) = shapes(c)
    free_a = c.family == "tn"
    words = mask_words(mask_shape(c)[1])

    def ld(width, free):
        if c.layout == "tight":
            return width if free else _r4(width)
        if c.layout in ("pad", "shift"):
            return _r4(width) + 4
        return _r4(width) + (5 if free else 8)

    mis = 1 if c.layout in ("odd", "shift") else 0
    stride = {"tight": words, "pad": _r4(words) + 4, "odd": words + 1, "shift": _r4(words) + 4}[c.layout]
    return Layout(ld(wa, free_a), mis if free_a else 0, ld(wb, True), mis, ld(wc, True), mis, stride, mis)


# ---- the generated case list ----------------------------------------------------------------------------------------
def k_axis():
    return tuple(sorted(set(K_MOD8) | {v for e in K_EDGES for v in e} | {63, 64, 65, 219, 220}))


def n_axis():
    return tuple(sorted({1, 3, 200, 219} | {v for e in N_EDGES for v in e}))


def shape_pairs():
    """(k, n): every k of the k axis at the pivot widths, every n of the n axis at the pivot reductions, the LDS threshold
    (both forms of it) and the special shapes -- the cross product thinned to the pairs that reach a leaf of their own"""
    pairs = {(k, n) for k in k_axis() for n in N_PIVOTS} | {(k, n) for k in K_PIVOTS for n in n_axis()}
    pairs |= set(LDS_EDGE) | set(LDS_EDGE_COLSUM) | set(SPECIAL_PAIRS)
    return tuple(sorted(pairs))


def sweep_cases(family):
    out = []
    for k, n in shape_pairs():
        for form in FORMS[family]:
            if family == "nn" and form == "recorded" and k > 256:
                continue                      # nothing to record (tgcn_dropout_mask_words == 0): REFUSED_RECORD_SHAPES
            for N in N_AXIS_ROWS:
                for lay in LAYOUTS:
                    out.append(make_case(family, form, N, k, n, lay))
    return out


REFUSED_RECORD_SHAPES = ((257, 64), (512, 33), (513, 257), (1000, 64))      # k > 256: no record, the _mask entry refuses
RECORDED_AT_THE_EDGE = ((256, 64), (256, 257))                               # k = 256 still records (8 words)


def big_cases():
    """A handful of leaves at an N that makes the persistent grid loop, and tn past the saturation of its partial tiles"""
    P, T, R = N_PERSISTENT, N_TN_SATURATED, N_PERSISTENT_RECORD
    spec = [("nn", "plain", P, 200, 64, "tight"), ("nn", "hashed", P, 64, 33, "pad"), ("nn", "recorded", P, 36, 8, "odd"),
            ("nt", "plain", P, 64, 224, "tight"), ("nt", "colsum", P, 64, 224, "pad"), ("nt", "hashed", P, 8, 97, "odd"),
            ("nt", "colsum_recorded", R, 64, 200, "pad"),
            ("tn", "plain", T, 200, 64, "tight"), ("tn", "hashed", T, 8, 33, "odd"), ("tn", "recorded", T, 32, 32, "pad"),
            ("tn", "plain", 512 * 1024 + 1, 7, 3, "tight")]
    return [make_case(*s, p=0.5) for s in spec]


def edge_rate_cases():
    """p = 0 (identity) and p = 1 (zeros) once per dropout form"""
    out = []
    for family, forms in FORMS.items():
        for form in forms:
            if has_drop(form):
                for p in (0.0, 1.0):
                    out.append(make_case(family, form, 129, 64, 200 if family == "nt" else 40, "pad", p=p))
    return out


ROW_KEYS = (20, 1000, 5000)          # rows [0, 20) are mask rows 1000.., the rest 5020..


def keyed_cases():
    """one shape per dropout form with row keys (split, key0, key1) through tgcn_set_dropout_row_keys"""
    out = []
    for family, forms in FORMS.items():
        for form in forms:
            if has_drop(form):
                out.append(make_case(family, form, 129, 64, 200 if family == "nt" else 36, "pad", keys=ROW_KEYS))
    return out


def zero_row_cases():
    """N = 0 for every form: the call succeeds, nn / nt store nothing, column sums of zero rows are zeros, tn is zeros"""
    return [make_case(f, form, 0, k, n, lay) for f, forms in FORMS.items() for form in forms
            for (k, n) in ((64, 200), (200, 64)) for lay in ("tight", "odd")]


# the split-bf16 mode: the shapes it claims and their neighbours it must not claim (all exact: integers up to 3 and their
# doubles are bf16 values, the low split terms are zero)
SPLIT_SHAPES = {"nn": [(200, n) for n in (32, 33, 48, 64, 65)],
                "nt": [(64, n) for n in (192, 193, 200, 224, 225)],
                "tn": [(200, n) for n in (32, 36, 64, 68)]}


def split_cases():
    out = []
    for family, pairs in SPLIT_SHAPES.items():
        forms = [f for f in FORMS[family] if "recorded" not in f]        # nothing records in this mode
        for k, n in pairs:
            for form in forms:
                for N in (1, 33, 1025):
                    for lay in LAYOUTS:
                        out.append(make_case(family, form, N, k, n, lay))
    return out


def foreign_record_cases():
    """Consumers of the record, handed the mask of ANOTHER seed, at shapes whose kernel is documented to take the record (tn:
    one LDS-staged launch covers all k; nt: k = 64, 193 <= n <= 224, aligned record): the result must follow the record.  A
    kernel that quietly hashes again would pass every other recorded case, whose record equals the hash."""
    spec = [("tn", "recorded", 1025, 200, 64, "pad"), ("tn", "recorded", 129, 64, 32, "tight"),
            ("tn", "recorded", 1024, 256, 128, "pad"), ("tn", "recorded", 33, 8, 4, "pad"),
            ("nt", "colsum_recorded", 1025, 64, 200, "pad"), ("nt", "colsum_recorded", 129, 64, 224, "tight"),
            ("nt", "colsum_recorded", 33, 64, 193, "pad")]
    return [make_case(*s, p=0.5, foreign=True) for s in spec]


def grouped(cases, by_k=True):
    """the cases as lists of one (family, form, k) -- or of one (family, form) -- each, in their order: the unit of one
    pytest item (a failure still names every failing case by its case_id)"""
    groups = {}
    for c in cases:
        groups.setdefault((c.family, c.form, c.k if by_k else None), []).append(c)
    return list(groups.values())


def all_cases():
    out = []
    for family in FORMS:
        out += sweep_cases(family)
    return out + big_cases() + edge_rate_cases() + keyed_cases() + zero_row_cases() + split_cases() + foreign_record_cases()
