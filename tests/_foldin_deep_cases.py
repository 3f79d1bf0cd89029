"""Case table of the layer-chain fold-in kernel's sweep (tests/test_gpu_foldin_deep.py runs it through the C ABI;
tests/test_foldin_deep_host.py keeps it complete on the CPU).  Test infrastructure.

`leaf_of` restates the dispatch of csrc/foldin_layers.hip: the kernel is instantiated on
    L2 / L3 / L4   the number of layers
    tail           some w_l is not a multiple of 4 (the last lane of a segment loads and stores scalars) -- else `vec`
    wide           some w_l, l >= 2, above 64 (a second column per lane in the x W epilogue)               -- else `narrow`
Exact family: dis powers of two, TF-IDF multiples of 2^-8 with sum + 1 = 4 (dis_d = 1/2, a_dd = 1/4; a document without
entries has dis_d = a_dd = 1), tables, s1 and the biases small integers, W_l with at most four entries of +-1 per column.
Every partial sum is then a dyadic rational whose finest step shrinks by a_dd per layer: 2^-12 at layer 1, 2^-18 at layer 4.
While the sums of absolute values stay below 2^24 units of the layer's step (asserted per case), ANY fp32 evaluation in ANY
order equals the float64 evaluation bit for bit.  dis_d = 1/4 (sum + 1 = 16) would put layer 4 at 2^-25, where a bias of
1 already breaks the condition, so the rows of 1100 entries (which need sum >= 1100 / 256) live in the float family and in
the bit-equality tests; the exact family has rows of 0, 1, 2, 63, 64, 65 and 129 entries at every L."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _foldin_cases as fc
import _foldin_deep_ref as DR
import _foldin_ref as R

DOCS_PER_WORKGROUP, WORKGROUP_CAP = fc.DOCS_PER_WORKGROUP, fc.WORKGROUP_CAP
MAX_FIRST, MAX_NEXT, MAX_LAYERS, LDS_LIMIT = 256, 128, 4, 163840
LEAVES = tuple(f"L{L}-{t}-{w}" for L in (2, 3, 4) for t in ("vec", "tail") for w in ("narrow", "wide"))
EXACT_ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 129)
ROW_LENGTHS = fc.ROW_LENGTHS                       # the float family's: 129 and 1100 entries too
LAYOUTS = ("tight", "padded", "reversed")          # segments back to back | 8 columns of gap after each | the layers reversed

# widths: (w_1, .., w_L);  acts: one per layer;  outs: which layers' `out` is given (one bool per layer);  pred: asked or not
Case = namedtuple("Case", "family widths n_docs n_vocab layout s1 acts mode outs pred seed")

WIDTHS = ((1, 1), (4, 8), (64, 128), (5, 63), (63, 65), (100, 64), (200, 100), (256, 128),
          (4, 64, 4), (100, 100, 64), (5, 1, 63), (65, 65, 5), (200, 64, 128),
          (4, 4, 4, 4), (100, 100, 100, 100), (5, 4, 63, 1), (64, 65, 128, 5), (64, 128, 64, 4))
OVER_THE_LIMIT = (128, 128, 128, 128)


def leaf_of(widths):
    tail = any(w % 4 for w in widths)
    return f"L{len(widths)}-{'tail' if tail else 'vec'}-{'wide' if any(w > 64 for w in widths[1:]) else 'narrow'}"


def case_id(c):
    return (f"{c.family}-{'x'.join(str(w) for w in c.widths)}-B{c.n_docs}-{c.layout}-{'s1' if c.s1 else 'nos1'}-"
            f"{''.join('r' if a else 'l' for a in c.acts)}-{c.mode[:3]}-{''.join('o' if o else '_' for o in c.outs)}"
            f"{'p' if c.pred else ''}")


def _variant(family, i, widths, n_docs, n_vocab=37):
    """Option values cycle with the case index at co-prime periods."""
    L = len(widths)
    acts = tuple((i >> l) & 1 for l in range(L))
    return Case(family, tuple(widths), n_docs, n_vocab, LAYOUTS[i % 3], bool(i % 2), acts, (R.REFERENCE, R.ACCURATE)[(i // 3) % 2],
                (True,) * L, True, 500 + i)


# one shape per leaf for the output combinations
_OUT_SHAPES = ((8, 4), (8, 68), (7, 5), (9, 70), (8, 4, 8), (8, 68, 4), (7, 5, 3), (9, 70, 5),
               (8, 4, 8, 4), (8, 4, 68, 4), (7, 5, 3, 2), (9, 5, 70, 5))


def int_cases():
    cases, i = [], 0
    for widths in WIDTHS:                              # every row length in every shape: 7 documents + 10 short ones = a tile + 1
        for _ in range(2):
            cases.append(_variant("int", i, widths, DOCS_PER_WORKGROUP + 1))
            i += 1
    # the batch sizes: none, one, a tile - 1, a tile, and two grid strides + 1 (short rows)
    for n_docs in (0, 1, DOCS_PER_WORKGROUP - 1, DOCS_PER_WORKGROUP, 2 * DOCS_PER_WORKGROUP * WORKGROUP_CAP + 1):
        for widths in ((4, 8), (5, 68, 3), (4, 4, 5, 8)):
            if n_docs > 4 * DOCS_PER_WORKGROUP and len(widths) == 3:
                continue
            cases.append(_variant("int", i, widths, n_docs))
            i += 1
    # every `out` and pred present or absent in every combination, on one shape per leaf
    for widths in _OUT_SHAPES:
        L = len(widths)
        for bits in range(1 << (L + 1)):
            outs = tuple(bool((bits >> l) & 1) for l in range(L))
            cases.append(_variant("int", i, widths, 9)._replace(outs=outs, pred=bool((bits >> L) & 1)))
            i += 1
    return cases


def float_cases():
    shapes = ((64, 64), (200, 128), (63, 7), (200, 65), (256, 128), (100, 100),
              (100, 100, 64), (64, 4, 8), (63, 5, 7), (65, 100, 5),
              (100, 100, 100, 100), (64, 64, 4, 8), (63, 5, 7, 1), (200, 65, 128, 5))
    return [_variant("float", i, widths, DOCS_PER_WORKGROUP + 1, n_vocab=301) for i, widths in enumerate(shapes * 2)]


def row_lengths(c):
    """The number of entries of every document: the first documents walk the family's row lengths, the rest are short --
    except in the large batch, which is short rows throughout."""
    if c.n_docs > 4 * DOCS_PER_WORKGROUP:
        return [(d * 7) % 3 for d in range(c.n_docs)]
    walk = EXACT_ROW_LENGTHS if c.family == "int" else ROW_LENGTHS
    return [walk[d] if d < len(walk) else (d % 3) for d in range(c.n_docs)]


def _dyadic_row(rng, n):
    """n positive multiples of 2^-8 with sum 3 (sum + 1 = 4)."""
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    units = 3 << fc.T_UNIT_LOG2
    r = rng.integers(1, max(2, units // n), size=n)
    r[-1] = units - int(r[:-1].sum())
    assert r.min() >= 1 and int(r.sum()) == units
    return (r.astype(np.float64) / (1 << fc.T_UNIT_LOG2)).astype(np.float32)


def _sparse_pm1(rng, rows, cols, per_col=4):
    """[rows, cols] with at most `per_col` entries of +-1 in every column, at random rows."""
    W = np.zeros((rows, cols))
    for c in range(cols):
        ks = rng.choice(rows, size=min(per_col, rows), replace=False)
        W[ks, c] = rng.choice((-1.0, 1.0), size=ks.size)
    return W


@lru_cache(maxsize=4)
def operands(c):
    """dict of host arrays: rowptr, col, val, dis, s1 (or None) and `layers` (dicts as tests/_foldin_deep_ref.py takes them).
    Documents carry first / last / duplicate columns and, every fourth one, a column outside [0, V) (skipped in the sums)."""
    rng = np.random.default_rng(c.seed)
    V = c.n_vocab
    lens = row_lengths(c)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols, vals = [], []
    for d, n in enumerate(lens):
        cj = rng.integers(0, V, size=n).astype(np.int32)
        if n >= 1 and d % 2 == 0:
            cj[0] = 0
        if n >= 2:
            cj[-1] = V - 1
        if n >= 3 and d % 2:
            cj[1] = cj[2]
        if n >= 4 and d % 4 == 3:
            cj[n // 2] = V + 5 if d % 8 == 3 else -1
        cols.append(cj)
        vals.append(_dyadic_row(rng, n) if c.family == "int" else (rng.random(n) * 0.9 + 0.05).astype(np.float32))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, dtype=np.int32)
    val = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, dtype=np.float32)
    exact = c.family == "int"
    dis = (2.0 ** -rng.integers(0, 4, size=V)) if exact else (rng.random(V) * 0.95 + 0.05)
    layers, wp = [], 0
    for li, w in enumerate(c.widths):
        if exact:
            T = rng.integers(-1, 2, size=(V, w)) if li == 0 else rng.integers(-2, 3, size=(V, w))
            W = _sparse_pm1(rng, wp, w) if li else None
            b = rng.integers(-2, 3, size=w)
        else:
            T = rng.standard_normal((V, w))
            W = rng.standard_normal((wp, w)) / np.sqrt(wp) if li else None
            b = rng.standard_normal(w)
        ly = dict(T=np.ascontiguousarray(T, dtype=np.float32), b=np.ascontiguousarray(b, dtype=np.float32),
                  W=None if W is None else np.ascontiguousarray(W, dtype=np.float32), act=c.acts[li])
        layers.append(ly)
        wp = w
    s1 = None
    if c.s1:
        s1 = (rng.integers(-2, 3, size=c.widths[0]) if exact else rng.standard_normal(c.widths[0])).astype(np.float32)
    return dict(rowptr=rowptr, col=col, val=val, dis=np.ascontiguousarray(dis, dtype=np.float32), s1=s1, layers=layers)


@lru_cache(maxsize=4)
def reference(c):
    """The float64 evaluation per layer (`layers`), the first arg-max of the last one (`pred`), and for the exact family
    `units`: the largest sum of absolute values in units of the document's finest dyadic step at that layer (must stay below
    2^24)."""
    o = operands(c)
    res = DR.foldin_layers(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["layers"], o["s1"], np.float64, want_abs=True)
    out = {"layers": res, "pred": R.first_argmax(res[-1]["x"].astype(np.float32))}
    if c.family == "int":
        _, _, dis_d = R.doc_scalars(o["rowptr"], np.clip(o["col"].astype(np.int64), 0, c.n_vocab - 1), o["val"], o["dis"], c.mode)
        n = np.diff(o["rowptr"])
        assert set(np.unique(dis_d).tolist()) <= {1.0, 0.5} and bool((dis_d[n == 0] == 1.0).all())
        units = 0.0
        # finest step of layer 1: a_j = t (2^-8) dis (>= 2^-3) dis_d; a document without entries has integers throughout.
        # Every further layer multiplies by a_dd = dis_d^2.
        step = np.where(n > 0, 2.0 ** -(fc.T_UNIT_LOG2 + 3) * dis_d.astype(np.float64), 1.0)[:, None] if len(n) else np.ones((0, 1))
        for li, r in enumerate(res):
            if li:
                step = step * r["a_dd"].astype(np.float64)[:, None]
            units = max(units, float((r["A"] / step).max(initial=0.0)))
            assert np.array_equal(r["x"].astype(np.float32).astype(np.float64), r["x"])
        out["units"] = units
    else:
        out["bounds"] = DR.float_bounds(o["rowptr"], res, o["layers"])
    return out
