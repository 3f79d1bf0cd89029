"""Case table of the per-level fold-in kernel's sweep (tests/test_gpu_foldin_levels.py runs it through the C ABI;
tests/test_foldin_levels_host.py keeps it complete on the CPU).  Test infrastructure.

`leaf_of` restates the dispatch of csrc/foldin_levels.hip: the kernel is instantiated on
    L2 / L3   the number of levels
    tail      some h_l or C_l is not a multiple of 4 (the last lane of a segment loads and stores scalars) -- else `vec`
    wide      some C_l > 64 (a second column per lane in the epilogue)                                     -- else `narrow`
Exact family: as tests/_foldin_cases.py -- dis powers of two, TF-IDF multiples of 2^-8 with dis_d in {1, 1/2, 1/4}, tables,
W2, Wh and the biases small integers, link = one_hot (so s^l is a row of Wh); every partial sum is a dyadic rational and,
while the sums of absolute values stay below 2^24 units of the finest step (asserted per case), ANY fp32 evaluation in ANY
order equals the float64 evaluation bit for bit."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _foldin_cases as fc
import _foldin_levels_ref as LR
import _foldin_ref as R

DOCS_PER_WORKGROUP, WORKGROUP_CAP = fc.DOCS_PER_WORKGROUP, fc.WORKGROUP_CAP
MAX_HIDDEN, MAX_CLASSES, MAX_LEVELS, LDS_LIMIT = 256, 128, 3, 163840
LEAVES = tuple(f"L{L}-{t}-{w}" for L in (2, 3) for t in ("vec", "tail") for w in ("narrow", "wide"))
ROW_LENGTHS = fc.ROW_LENGTHS
LAYOUTS = ("tight", "padded", "reversed")      # segments back to back | 8 columns of gap after each | P segments first, levels reversed
OUTS = ("logits", "pred", "hidden", "link")

# widths: ((h_1, C_1), (h_2, C_2)[, (h_3, C_3)]);  acts / links: one per level (links[0] is unused);  outs: which outputs are asked
Case = namedtuple("Case", "family widths n_docs n_vocab layout acts links mode outs seed")

WIDTHS = (((1, 1), (1, 1)), ((4, 2), (4, 8)), ((63, 63), (64, 65)), ((100, 6), (100, 64)),
          ((100, 9), (100, 70), (100, 128)), ((256, 128), (8, 4)),
          ((4, 4), (8, 8)), ((8, 4), (4, 8), (12, 4)), ((8, 4), (4, 68), (4, 8)), ((5, 3), (4, 2), (3, 5)))
OVER_THE_LIMIT = ((256, 128), (256, 128))       # two W2 of 128 KiB


def leaf_of(widths):
    tail = any(h % 4 or C % 4 for h, C in widths)
    return f"L{len(widths)}-{'tail' if tail else 'vec'}-{'wide' if any(C > 64 for _, C in widths) else 'narrow'}"


def case_id(c):
    w = "_".join(f"{h}x{C}" for h, C in c.widths)
    return (f"{c.family}-{w}-B{c.n_docs}-{c.layout}-{''.join('r' if a else 'l' for a in c.acts)}-"
            f"{''.join(k[0] for k in c.links[1:])}-{c.mode[:3]}-{''.join(o[0] for o in c.outs)}")


def _variant(family, i, widths, n_docs, n_vocab=37):
    """Option values cycle with the case index at co-prime periods."""
    L = len(widths)
    acts = tuple((i >> l) & 1 for l in range(L))
    if family == "int":
        links = (None,) + (LR.ONE_HOT,) * (L - 1)
    else:
        links = (None,) + tuple((LR.SOFTMAX, LR.ONE_HOT)[(i >> l) & 1] for l in range(L - 1))
    outs = tuple(o for k, o in enumerate(OUTS) if k == 0 or (i + k) % 2)
    return Case(family, widths, n_docs, n_vocab, LAYOUTS[i % 3], acts, links, (R.REFERENCE, R.ACCURATE)[(i // 3) % 2], outs,
                300 + i)


def int_cases():
    cases, i = [], 0
    for widths in WIDTHS:                              # every row length in every shape: 8 documents + 9 short ones = a tile + 1
        for _ in range(2):
            cases.append(_variant("int", i, widths, DOCS_PER_WORKGROUP + 1))
            i += 1
    # the batch sizes: none, one, a tile - 1, a tile, and two grid strides + 1 (short rows)
    for n_docs in (0, 1, DOCS_PER_WORKGROUP - 1, DOCS_PER_WORKGROUP, 2 * DOCS_PER_WORKGROUP * WORKGROUP_CAP + 1):
        for widths in (((4, 2), (4, 8)), ((5, 3), (4, 68), (3, 5))):
            cases.append(_variant("int", i, widths, n_docs))
            i += 1
    # every optional output off and on (logits too) on one shape per number of levels
    for widths in (((8, 4), (4, 8)), ((5, 3), (4, 68), (3, 5))):
        for outs in ((), ("logits",), ("pred",), ("hidden",), ("link",), OUTS):
            cases.append(_variant("int", i, widths, 9)._replace(outs=outs))
            i += 1
    return cases


def float_cases():
    """link = softmax on some level of every case; both links and both activations on every level across the family."""
    shapes = (((64, 64), (64, 64)), ((100, 6), (100, 64)), ((63, 7), (200, 65)), ((100, 128), (64, 8)),
              ((100, 9), (100, 70), (100, 128)), ((8, 4), (4, 8), (12, 4)), ((8, 4), (4, 68), (4, 8)), ((5, 3), (4, 2), (3, 5)))
    out = []
    for i, widths in enumerate(shapes * 2):
        c = _variant("float", i, widths, DOCS_PER_WORKGROUP + 1, n_vocab=301)
        if all(k != LR.SOFTMAX for k in c.links[1:]):
            c = c._replace(links=(None, LR.SOFTMAX) + c.links[2:])
        out.append(c._replace(outs=OUTS))
    return out


def row_lengths(c):
    return fc.row_lengths(fc.Case(c.family, 1, 1, c.n_docs, c.n_vocab, "tight", False, 0, c.mode, False, False, 0))


@lru_cache(maxsize=4)
def operands(c):
    """dict of host arrays: rowptr, col, val, dis and `levels` (dicts as tests/_foldin_levels_ref.py takes them).  Documents
    carry first / last / duplicate columns and, every fourth one, a column outside [0, V) (skipped in the sums)."""
    rng = np.random.default_rng(c.seed)
    V, B = c.n_vocab, c.n_docs
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
        vals.append(fc._dyadic_row(rng, n) if c.family == "int" else (rng.random(n) * 0.9 + 0.05).astype(np.float32))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, dtype=np.int32)
    val = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, dtype=np.float32)
    exact = c.family == "int"
    dis = (2.0 ** -rng.integers(0, 4, size=V)) if exact else (rng.random(V) * 0.95 + 0.05)
    levels, Cp = [], 0
    for li, (h, C) in enumerate(c.widths):
        if exact:
            T1, P = rng.integers(-1, 2, size=(V, h)), rng.integers(-2, 3, size=(V, C))
            W2 = rng.integers(-1, 2, size=(h, C)) * (rng.random((h, C)) < 0.5)
            Wh, b1, b2 = rng.integers(-2, 3, size=(Cp, h)), rng.integers(-2, 3, size=h), rng.integers(-2, 3, size=C)
        else:
            T1, P, W2 = rng.standard_normal((V, h)), rng.standard_normal((V, C)), rng.standard_normal((h, C)) / np.sqrt(h)
            Wh, b1, b2 = rng.standard_normal((Cp, h)), rng.standard_normal(h), rng.standard_normal(C)
            if li == 0 and c.seed % 2:
                P, b2 = P * 30.0, b2 * 30.0            # level-1 logits spread to +-80 and beyond: the softmax saturates
        lv = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in dict(T1=T1, P=P, W2=W2, b1=b1, b2=b2).items()}
        lv["Wh"] = np.ascontiguousarray(Wh, dtype=np.float32) if li else None
        lv["act"], lv["link"] = c.acts[li], c.links[li]
        levels.append(lv)
        Cp = C
    return dict(rowptr=rowptr, col=col, val=val, dis=np.ascontiguousarray(dis, dtype=np.float32), levels=levels)


@lru_cache(maxsize=4)
def reference(c):
    """The float64 evaluation per level, and for the exact family `units`: the largest sum of absolute values in units of
    the document's finest dyadic step (must stay below 2^24)."""
    o = operands(c)
    res = LR.foldin_levels(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["levels"], np.float64, want_abs=True)
    if c.family == "int":
        _, _, dis_d = R.doc_scalars(o["rowptr"], np.clip(o["col"].astype(np.int64), 0, c.n_vocab - 1), o["val"], o["dis"], c.mode)
        assert set(np.unique(dis_d).tolist()) <= {1.0, 0.5, 0.25}
        n = np.diff(o["rowptr"])
        units = 0.0
        for r, lv in zip(res, o["levels"]):
            a_dd = r["a_dd"].astype(np.float64)[:, None]
            # finest step: a_j = t (2^-8) dis (>= 2^-3) dis_d; a_dd s (level >= 2) is a multiple of dis_d^2 >= 2^-3 dis_d
            step_u = (2.0 ** -(fc.T_UNIT_LOG2 + 3) * dis_d.astype(np.float64))[:, None] if len(n) else np.ones((0, 1))
            step_z = step_u * a_dd
            zabs = r["Zp"] + a_dd * (np.abs(r["u"]) @ np.abs(lv["W2"].astype(np.float64))) + np.abs(lv["b2"].astype(np.float64))[None, :]
            units = max(units, float((r["U"] / step_u).max(initial=0.0)), float((zabs / step_z).max(initial=0.0)))
            assert np.array_equal(r["z"].astype(np.float32).astype(np.float64), r["z"])
            assert np.array_equal(r["u"].astype(np.float32).astype(np.float64), r["u"])
        return {"levels": res, "units": units}
    return {"levels": res}
