"""Case table of the fold-in kernel's sweep (tests/test_gpu_foldin.py runs it through the C ABI; tests/test_foldin_host.py
keeps it complete on the CPU).  Test infrastructure.

`leaf_of` restates the dispatch of csrc/foldin.hip: the kernel is instantiated on
    tail   h or C is not a multiple of 4 (the last lane of a row loads and stores scalars) -- else `vec`
    wide   C > 64 (a second column per lane in the epilogue)                               -- else `narrow`
and inside a leaf the arithmetic of a document depends on nothing but (h, C) and its own row.

Exact family: dis entries are powers of two, TF-IDF values multiples of 2^-8 with sum + 1 in {1, 4, 16} (dis_d in {1, 1/2,
1/4}), tables, W2, s1 and the biases small integers.  Every product and every partial sum is then a dyadic rational; `operands`
returns the sums of absolute values in units of the finest one, and while they stay below 2^24 ANY fp32 evaluation in ANY
order -- fused or not -- equals the float64 evaluation bit for bit (the bound is asserted per case)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _foldin_ref as R

DOCS_PER_WORKGROUP, WORKGROUP_CAP = 16, 512          # TGCN_FOLDIN_DOCS_PER_WORKGROUP / _WORKGROUP_CAP of include/tgcn.h
MAX_HIDDEN, MAX_CLASSES = 256, 128                   # tgcn_foldin_max_hidden() / _max_classes()
LEAVES = ("vec-narrow", "vec-wide", "tail-narrow", "tail-wide")
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 129, 1100)
T_UNIT_LOG2 = 8                                       # TF-IDF values are multiples of 2^-8

# layout: "tight" = leading dimensions rounded up to 4, "padded" = 8 more, "shared" = T1 and P are two views of one row-padded table
Case = namedtuple("Case", "family h C n_docs n_vocab layout s1 act mode pred hidden seed")


def leaf_of(h, C):
    return ("vec" if h % 4 == 0 and C % 4 == 0 else "tail") + "-" + ("wide" if C > 64 else "narrow")


def case_id(c):
    return (f"{c.family}-h{c.h}-C{c.C}-B{c.n_docs}-V{c.n_vocab}-{c.layout}-{'s1' if c.s1 else 'nos1'}-"
            f"{'relu' if c.act else 'lin'}-{c.mode[:3]}-{'p' if c.pred else ''}{'h' if c.hidden else ''}")


_SHAPES = ((1, 1), (4, 2), (4, 8), (63, 63), (64, 64), (63, 65), (64, 65), (100, 8), (100, 128), (200, 64), (200, 65),
           (256, 128), (256, 1), (1, 128))
_LAYOUTS = ("tight", "padded", "shared")


def _variant(family, i, h, C, n_docs, n_vocab=37):
    """Option values cycle with the case index at co-prime periods, so that every pair of options meets somewhere."""
    return Case(family, h, C, n_docs, n_vocab, _LAYOUTS[i % 3], bool(i % 2), (i // 2) % 2,
                (R.REFERENCE, R.ACCURATE)[(i // 3) % 2], bool((i // 2) % 2) ^ bool(i % 5 == 0), bool(i % 4 in (1, 2)), 100 + i)


def int_cases():
    cases, i = [], 0
    for h, C in _SHAPES:                              # every row length in every shape: 8 documents + 9 short ones = a tile + 1
        for _ in range(2):
            cases.append(_variant("int", i, h, C, DOCS_PER_WORKGROUP + 1))
            i += 1
    # the batch sizes: none, one, a tile - 1, a tile, and two grid strides + 1 (short rows)
    for n_docs in (0, 1, DOCS_PER_WORKGROUP - 1, DOCS_PER_WORKGROUP, 2 * DOCS_PER_WORKGROUP * WORKGROUP_CAP + 1):
        for h, C in ((4, 8), (5, 65)):
            cases.append(_variant("int", i, h, C, n_docs))
            i += 1
    # pred x hidden in every combination on one shape per leaf, both activations
    for h, C in ((8, 4), (8, 68), (7, 5), (9, 70)):
        for pred in (False, True):
            for hidden in (False, True):
                cases.append(_variant("int", i, h, C, 9)._replace(pred=pred, hidden=hidden, act=int(pred ^ hidden)))
                i += 1
    return cases


def float_cases():
    shapes = ((64, 64), (200, 64), (100, 128), (63, 7), (200, 65), (256, 128))
    return [_variant("float", i, h, C, DOCS_PER_WORKGROUP + 1, n_vocab=301) for i, (h, C) in enumerate(shapes * 2)]


def row_lengths(c):
    """The number of entries of every document: the first eight documents walk ROW_LENGTHS, the rest are short -- except in
    the large batch, which is short rows throughout."""
    if c.n_docs > 4 * DOCS_PER_WORKGROUP:
        return [(d * 7) % 3 for d in range(c.n_docs)]
    return [ROW_LENGTHS[d] if d < len(ROW_LENGTHS) else (d % 3) for d in range(c.n_docs)]


def _dyadic_row(rng, n):
    """n positive multiples of 2^-8 with sum 3 or 15 (sum + 1 = 4 or 16)."""
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    total = 15 if (n > 700 or rng.integers(2)) else 3
    units = total << T_UNIT_LOG2
    r = rng.integers(1, max(2, units // n), size=n)
    r[-1] = units - int(r[:-1].sum())
    assert r.min() >= 1 and int(r.sum()) == units
    return (r.astype(np.float64) / (1 << T_UNIT_LOG2)).astype(np.float32)


@lru_cache(maxsize=4)
def operands(c):
    """dict of host arrays: rowptr, col, val, dis, T1, s1 (or None), b1, P, W2, b2 -- and for the exact family `units`, the
    largest sum of absolute values of a case in units of its finest dyadic step (must stay below 2^24)."""
    rng = np.random.default_rng(c.seed)
    V, h, C, B = c.n_vocab, c.h, c.C, c.n_docs
    lens = row_lengths(c)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols, vals = [], []
    for d, n in enumerate(lens):
        cj = rng.integers(0, V, size=n).astype(np.int32)
        if n >= 1 and d % 2 == 0:
            cj[0] = 0                                  # the first column ...
        if n >= 2:
            cj[-1] = V - 1                             # ... the last one ...
        if n >= 3 and d % 2:
            cj[1] = cj[2]                              # ... and a duplicate next to itself
        cols.append(cj)
        vals.append(_dyadic_row(rng, n) if c.family == "int" else (rng.random(n) * 0.9 + 0.05).astype(np.float32))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, dtype=np.int32)
    val = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, dtype=np.float32)
    if c.family == "int":
        dis = (2.0 ** -rng.integers(0, 4, size=V)).astype(np.float32)
        T1 = rng.integers(-1, 2, size=(V, h))
        P = rng.integers(-2, 3, size=(V, C))
        W2 = rng.integers(-1, 2, size=(h, C)) * (rng.random((h, C)) < 0.5)
        s1, b1, b2 = rng.integers(-2, 3, size=h), rng.integers(-2, 3, size=h), rng.integers(-2, 3, size=C)
    else:
        dis = (rng.random(V) * 0.95 + 0.05).astype(np.float32)
        T1, P, W2 = rng.standard_normal((V, h)), rng.standard_normal((V, C)), rng.standard_normal((h, C)) / np.sqrt(h)
        s1, b1, b2 = rng.standard_normal(h), rng.standard_normal(h), rng.standard_normal(C)
    out = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in
           dict(dis=dis, T1=T1, P=P, W2=W2, s1=s1, b1=b1, b2=b2).items()}
    if not c.s1:
        out["s1"] = None
    out.update(rowptr=rowptr, col=col, val=val)
    return out


@lru_cache(maxsize=4)
def reference(c):
    """dict: z, u (float64 evaluation of the definition), pred; `units` (exact family) or bu, bz (float family)."""
    o = operands(c)
    z, u, U, Zp = R.foldin(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["T1"], o["s1"], o["b1"], c.act, o["P"],
                           o["W2"], o["b2"], np.float64, want_abs=True)
    a, a_dd, dis_d = R.doc_scalars(o["rowptr"], o["col"].astype(np.int64), o["val"], o["dis"], c.mode)
    ref = {"z": z, "u": u, "a_dd": a_dd, "dis_d": dis_d}
    if c.family == "int":
        # finest step of a document: a_j = t (2^-8) * dis (>= 2^-3) * dis_d and u shares it (a_dd s1 and b1 are coarser); a
        # document without entries has integer u.  z = ... + a_dd (u W2) is a_dd = dis_d^2 finer.  The degree sum itself
        # stays below 16 in steps of 2^-8.
        assert set(np.unique(dis_d).tolist()) <= {1.0, 0.5, 0.25}
        n = np.diff(o["rowptr"])
        step_u = np.where(n > 0, 2.0 ** -(T_UNIT_LOG2 + 3) * dis_d.astype(np.float64), 1.0)[:, None]
        step_z = step_u * a_dd.astype(np.float64)[:, None]
        zabs = Zp + np.abs(a_dd.astype(np.float64))[:, None] * (np.abs(u) @ np.abs(o["W2"].astype(np.float64))) \
            + np.abs(o["b2"].astype(np.float64))[None, :]
        ref["units"] = max(float((U / step_u).max(initial=0.0)), float((zabs / step_z).max(initial=0.0)))
        # the float64 values are the exact ones and fit fp32: the cast changes nothing
        assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    else:
        ref["bu"], ref["bz"] = R.float_bounds(o["rowptr"], a_dd, c.h, u, U, Zp, o["W2"], o["b2"])
    ref["pred"] = R.first_argmax(z.astype(np.float32))
    return ref
