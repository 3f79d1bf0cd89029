"""Cases of the sweep over the grouped masked cross-entropy of csrc/perlabel.hip (tests/test_gpu_grouped_ce.py):
k_grouped_ce<LPR, V4>, k_grouped_ce_wide and k_grouped_ce_final behind `tgcn_grouped_ce`.  The case lists, a pure-Python
restatement of what the launcher chooses, the inputs, the float64 reference and an fp32 restatement of the arithmetic the
kernel is meant to use.  CPU only: numpy; nothing here imports torch.cuda or the library.  Test infrastructure;
tests/test_grouped_ce_cases.py keeps the lists honest.

The restated choices are written from `tgcn_grouped_ce` (csrc/perlabel.hip); the lines are cited where they are restated.
They exist so that the host test can say "every leaf, both sides of every boundary, one case above each launch cap" about
the LIST -- the GPU test never asks them what the right answer is."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from _train_cases import FILL, N_SMALL, TINY_ROW, _frozen   # noqa: F401  (FILL, TINY_ROW: re-exported to the GPU test)

# ---- the launcher's choice -------------------------------------------------------------------------------------------
GCE_BLOCKS = 1024                               # perlabel.hip:32 `constexpr int kGceBlocks = 1024`
GCE_MAX_GROUPS = 128                            # perlabel.hip:33 `constexpr int kGceMaxGroups = 128`
GCE_EDGES = ((16, 17), (32, 33), (64, 65), (128, 129), (256, 257))
WIDE = 0                                        # the "lanes per row" of k_grouped_ce_wide in a leaf tuple


def gce_lanes(n_cols):
    """perlabel.hip:322 `lanes_per_row`: `n_cols <= 16 ? 4 : n_cols <= 32 ? 8 : n_cols <= 64 ? 16 : n_cols <= 128 ? 32 : 64`"""
    return 4 if n_cols <= 16 else 8 if n_cols <= 32 else 16 if n_cols <= 64 else 32 if n_cols <= 128 else 64


def gce_rows_per_block(n_cols):
    """perlabel.hip:370-372 `regs = n_cols <= 256; rows_per_block = regs ? 2 * 4 * (64 / lpr) : 2 * 4`"""
    return 2 * 4 * (64 // gce_lanes(n_cols)) if n_cols <= 256 else 2 * 4


def gce_grid(n_cols, n):
    """perlabel.hip:373 `min(kGceBlocks, max(1, (n_rows + rows_per_block - 1) / rows_per_block))`"""
    rpb = gce_rows_per_block(n_cols)
    return min(GCE_BLOCKS, max(1, -(-n // rpb)))


def gce_v4(n_cols, ld, ldd, off, offd, has_grad):
    """perlabel.hip:377-378 `n_cols % 4 == 0 && ld % 4 == 0 && logits % 16 == 0 && (!dlogits || (ldd % 4 == 0 && dlogits % 16
    == 0))`, asked only when `regs`; for buffers that start `off` / `offd` floats into a 16-byte aligned allocation."""
    return n_cols <= 256 and n_cols % 4 == 0 and ld % 4 == 0 and off % 4 == 0 and (not has_grad or (ldd % 4 == 0 and offd % 4 == 0))


def scalar_causes(C, ld, ldd, off, offd, has_grad):
    """which of the five terms of the `v4` test fail"""
    return frozenset(name for name, bad in (("n_cols", C % 4), ("ld", ld % 4), ("base", off % 4), ("ldd", has_grad and ldd % 4),
                                            ("dbase", has_grad and offd % 4)) if bad)


LEAVES = tuple((lpr, v4) for v4 in (True, False) for lpr in (4, 8, 16, 32, 64)) + ((WIDE, False),)


def leaf_id(leaf):
    return "wide" if leaf[0] == WIDE else f"lpr{leaf[0]}-{'v4' if leaf[1] else 'scalar'}"


# ---- segment layouts -------------------------------------------------------------------------------------------------
_PATTERN = (3, 6, 1, 5, 9, 2, 7, 13, 4, 33)
SEG_LAYOUTS = ("packed", "gaps", "one", "full")                 # the four of every leaf
GROUP_EDGE_LAYOUTS = ("ones", "ones_spread", "alt13")           # K = min(n_cols, 128) / 128 / 128 groups
N_GROUP_EDGE = 2049                                             # rows of those: some ten selected rows in each of 128 groups


@lru_cache(maxsize=None)
def segments(C, seg):
    """(starts, widths) of a named layout in a row of C columns
      packed       back to back from column 0 at any residue, the last one cut at C: segments straddle a lane's four
                   columns and a sub-group's lanes; one of 70 columns in rows that have the room (more than one pass of
                   the wide kernel's 64 lanes)
      gaps         starts at multiples of 4, four more pad columns in front of every odd segment, pad at the tail
      one          a width-1 segment in the middle of the row between two that fill the rest
      full         one segment over the whole row
      ones         min(C, 128) width-1 segments back to back;  ones_spread: 128 of them at the odd columns
      alt13        128 segments of widths 1, 3, 1, 3, ... back to back"""
    pat = _PATTERN[:4] + (70,) + _PATTERN[4:] if C > 140 else _PATTERN
    starts, widths = [], []
    if seg == "packed":
        at, i = 0, 0
        while at < C:
            w = min(pat[i % len(pat)], C - at)
            starts.append(at), widths.append(w)
            at, i = at + w, i + 1
    elif seg == "gaps":
        at, i = 0, 0
        while True:
            s = (at + 3) // 4 * 4 + (4 if i % 2 else 0)
            w = pat[i % len(pat)]
            if s + w > C:
                break
            starts.append(s), widths.append(w)
            at, i = s + w, i + 1
        if not starts:                                          # rows too narrow for the first segment
            starts, widths = [0], [max(1, C - 1)]
    elif seg == "one":
        h = C // 2
        for s, w in ((0, h), (h, 1), (h + 1, C - h - 1)):
            if w > 0:
                starts.append(s), widths.append(w)
    elif seg == "full":
        starts, widths = [0], [C]
    elif seg == "ones":
        starts, widths = list(range(min(C, GCE_MAX_GROUPS))), [1] * min(C, GCE_MAX_GROUPS)
    elif seg == "ones_spread":
        starts, widths = [2 * k + 1 for k in range(GCE_MAX_GROUPS)], [1] * GCE_MAX_GROUPS
    elif seg == "alt13":
        widths = [1, 3] * (GCE_MAX_GROUPS // 2)
        starts = [int(v) for v in np.cumsum([0] + widths[:-1])]
    else:
        raise ValueError(seg)
    assert starts and len(starts) <= GCE_MAX_GROUPS and starts[-1] + widths[-1] <= C, (C, seg)
    assert all(w >= 1 for w in widths) and all(a + w <= b for a, w, b in zip(starts, widths, starts[1:]))
    return tuple(starts), tuple(widths)


# ---- the cases -------------------------------------------------------------------------------------------------------
OUTPUTS = ("loss", "grad", "dbias")
# (pred, route, class_map): `route` and `class_map` are read by the arg-max alone
PRED_COMBOS = ((False, False, False), (True, False, False), (True, True, False), (True, False, True), (True, True, True))
GceCase = namedtuple("GceCase", "C n seg pad pad2 off offd out pred route cmap values")
GceCase.__doc__ = """C columns, n rows, segment layout `seg`; logits are [n, C + pad] starting `off` floats into a 16-byte
aligned buffer, dlogits [n + 3, C + pad2] starting `offd` floats in; `out` (OUTPUTS); `pred` (arg-max wanted), with a `route`
array or in the row's own group, through a `class_map` or as the column; `values` (VALUES)."""

V4_WIDTHS = {4: (4, 16), 8: (20, 32), 16: (36, 64), 32: (68, 128), 64: (132, 256)}
SCALAR_WIDTHS = {4: (1, 3, 7, 16), 8: (17, 32), 16: (33, 64), 32: (65, 128), 64: (129, 219, 256), WIDE: (257, 259, 260, 300)}
# (pad, pad2, off, offd)
V4_LAYOUTS = ((0, 0, 0, 0), (4, 4, 0, 0), (0, 4, 0, 0), (4, 0, 0, 0))
ODD_LAYOUTS = ((1, 3, 0, 0), (0, 0, 1, 1), (4, 4, 1, 0), (0, 4, 0, 1), (3, 4, 0, 0), (4, 1, 0, 0))   # for C % 4 == 0


def any_layouts(C):
    """for C % 4 != 0: the last one pads both rows to a multiple of 4 floats, which leaves n_cols as the only cause"""
    return ((0, 0, 0, 0), (1, 3, 0, 0), (5, 0, 0, 0), (-C % 4, -C % 4, 0, 0))


VALUES = ("randn", "at+80", "at-80", "at+1e4", "at-1e4", "x80", "x1e4", "neginf", "equal", "onemask", "ties", "onehot",
          "argmax", "nanrow")
EDGE_VALUES = VALUES[1:]
# one width per leaf for the full cross of layouts and outputs, the value edges and the grid-stride cases
LEAF_WIDTH = {(4, True): 16, (8, True): 32, (16, True): 64, (32, True): 128, (64, True): 256,
              (4, False): 7, (8, False): 17, (16, False): 33, (32, False): 65, (64, False): 129, (WIDE, False): 257}


def case_is_v4(c):
    return gce_v4(c.C, c.C + c.pad, c.C + c.pad2, c.off, c.offd, c.out != "loss")


def leaf_of(c):
    return (gce_lanes(c.C) if c.C <= 256 else WIDE, case_is_v4(c))


def case_id(c):
    return (f"C{c.C}-n{c.n}-{c.seg}-pad{c.pad}.{c.pad2}-off{c.off}.{c.offd}-{c.out}"
            f"{'-pred' if c.pred else ''}{'-route' if c.route else ''}{'-map' if c.cmap else ''}-{c.values}")


def _leaf_layout(leaf, C):
    return (4, 4, 0, 0) if leaf[1] else ((1, 3, 0, 0) if C % 4 else (0, 0, 1, 1))


def _leaf_case(leaf, n, values, seg="packed", out="dbias", combo=(True, True, True)):
    C = LEAF_WIDTH[leaf]
    return GceCase(C, n, seg, *_leaf_layout(leaf, C), out, *combo, values)


_SHORT = (("dbias", (True, True, True)), ("loss", (False, False, False)), ("grad", (True, False, False)))


@lru_cache(maxsize=None)
def small_cases():
    """per leaf: its own width x the four segment layouts x the three outputs x the five arg-max combinations; every
    other width and buffer layout that keeps the case on the leaf with the segment layouts in turn; the group edges
    (K = 128, K = 16) where the width belongs to the leaf; a few row counts below one workgroup"""
    out = []
    for leaf in LEAVES:
        out += [_leaf_case(leaf, N_SMALL, "randn", seg, o, combo) for seg in SEG_LAYOUTS for o in OUTPUTS for combo in PRED_COMBOS]
        i = 0
        if leaf[1]:
            spread = [(C, lay) for C in V4_WIDTHS[leaf[0]] for lay in V4_LAYOUTS]
        else:
            spread = [(C, lay) for C in SCALAR_WIDTHS[leaf[0]] for lay in (ODD_LAYOUTS if C % 4 == 0 else any_layouts(C))]
            if leaf[0] == WIDE:                                 # (no 16-byte leaf to leave: the aligned layouts as well)
                spread += [(C, lay) for C in SCALAR_WIDTHS[WIDE] if C % 4 == 0 for lay in V4_LAYOUTS]
        for C, lay in spread:
            for o, combo in _SHORT:
                c = GceCase(C, N_SMALL, SEG_LAYOUTS[i % 4], *lay, o, *combo, "randn")
                if leaf_of(c) == leaf:                          # (a shifted dlogits does not move the loss-alone call)
                    out.append(c)
            i += 1
    for C, seg in ((16, "ones"), (128, "ones"), (300, "ones_spread"), (300, "alt13")):
        for lay in ((4, 4, 0, 0), (1, 3, 0, 0)):
            out += [GceCase(C, N_GROUP_EDGE, seg, *lay, o, *combo, "randn") for o, combo in _SHORT]
    out += [GceCase(C, n, "packed", 0, 0, 0, 0, "dbias", True, True, True, "randn") for C in (2, 16, 64, 300) for n in (1, 37)]
    return tuple(dict.fromkeys(out))             # (the spread meets the full cross at the leaf's own width and layout)


@lru_cache(maxsize=None)
def edge_cases():
    """the value edges, at N_SMALL rows per leaf, on the packed segments"""
    return tuple(_leaf_case(leaf, N_SMALL, v) for leaf in LEAVES for v in EDGE_VALUES)


@lru_cache(maxsize=None)
def stride_cases():
    """per leaf the smallest n at which a workgroup takes a second stride of rows, 1024 * rows_per_block + 1, with random
    values and with one-hot rows that name themselves; and the largest n at which none does"""
    out = []
    for leaf in LEAVES:
        cap = GCE_BLOCKS * gce_rows_per_block(LEAF_WIDTH[leaf])
        out += [_leaf_case(leaf, cap + 1, "randn"), _leaf_case(leaf, cap + 1, "onehot", out="grad"),
                _leaf_case(leaf, cap, "onehot", out="loss")]
    return tuple(out)


def all_cases():
    return small_cases() + edge_cases() + stride_cases()


def by_leaf(cases):
    out = {leaf: [] for leaf in LEAVES}
    for c in cases:
        out[leaf_of(c)].append(c)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------
BAD_GROUPS = (-1, -5)                            # ... and K: selected rows of these groups contribute nothing


def _seed(*v):
    return zlib.crc32(repr(v).encode())


def tie_pairs(C, s, w):
    """the column pairs of segment [s, s + w) that hold a tied maximum, by row class: 0 -- the segment's first and last
    column; 1 -- the first two neighbours inside it where a lane's four consecutive columns hand over to the next lane's
    (a multiple of 4); 2 -- the same for the strided column map (a multiple of LPR).  None where the segment has no such
    pair."""
    lpr = gce_lanes(C) if C <= 256 else 64

    def hand_over(step):
        b = -(-(s + 1) // step) * step
        return (b - 1, b) if b < s + w else None
    return ((s, s + w - 1) if w >= 2 else None, hand_over(4), hand_over(lpr))


@lru_cache(maxsize=4)
def gce_inputs(C, n, seg, values):
    """{"x": float32 [n, C] (finite numbers in every column; see `poisoned`), "target", "mask", "group", "route",
    "class_map", "inv_count" float32 [K], "starts", "widths"}; shared by the cases of one (C, n, seg, values), read-only.

    Groups are uniform over the K segments, with one row in eight in K, -1 or -5 (selected or not); with K >= 2 group K // 2
    has rows but none selected; `route` is drawn independently, with one in eight out of range."""
    gen = np.random.default_rng(_seed("gce", C, n, seg, values))
    starts, widths = (np.asarray(v, dtype=np.int64) for v in segments(C, seg))
    K = len(starts)
    r = np.arange(n)

    def ids():
        g = gen.integers(0, K, size=n)
        odd = gen.random(n) < 0.125
        return np.where(odd, np.asarray((K,) + BAD_GROUPS)[gen.integers(0, 3, size=n)], g).astype(np.int32)
    group, route = ids(), ids()
    mask = gen.random(n) < 0.6
    for b in (K,) + BAD_GROUPS:                   # (at least one SELECTED row of each group that is none)
        mask[np.flatnonzero(group == b)[:1]] = True
    x = gen.standard_normal((n, C), dtype=np.float32) * np.float32(3.0)
    if values == "onehot":
        group = (r % K).astype(np.int32)
        route, mask = group.copy(), np.ones(n, dtype=bool)
    valid = (group >= 0) & (group < K)
    gs, gw = starts[np.where(valid, group, 0)], widths[np.where(valid, group, 0)]
    target = np.where(valid, (gen.random(n) * gw).astype(np.int64) % gw, -1)
    if values == "onehot":
        hot = (r // K) % gw
        x = np.zeros((n, C), dtype=np.float32)
        x[r, gs + hot] = 40.0
        # the hot class on every other row of a group, never it on the rest
        target = np.where(((r // K) % 2 == 0) | (gw == 1), hot, (hot + 1 + (r // 3) % np.maximum(gw - 1, 1)) % gw)
    elif K >= 2:
        mask &= group != K // 2
    trainable = np.flatnonzero(valid & ((group != K // 2) | (K < 2) | (values == "onehot")))
    if values == "onemask":
        mask = np.zeros(n, dtype=bool)
        mask[trainable[len(trainable) // 2]] = True
    elif n and trainable.size and not mask[trainable].any():
        mask[trainable[0]] = True
    if values.startswith("at"):                   # rows AT +-L
        x = x + np.float32(float(values[2:]))
    elif values in ("x80", "x1e4"):               # every segment of every row SCALED to +-L
        for s, w in zip(starts, widths):
            x[:, s:s + w] = x[:, s:s + w] / np.abs(x[:, s:s + w]).max(1, keepdims=True) * np.float32(float(values[1:]))
    elif values == "neginf":
        drop = gen.random((n, C)) < 1.0 / 3.0
        drop[r[valid], (gs + target)[valid]] = False
        x = np.where(drop, np.float32(-np.inf), x)
    elif values == "equal":
        x = np.repeat(np.asarray([0.0, 5.0, -80.0, 1e4, -1e4], dtype=np.float32)[r % 5][:, None], C, axis=1)
    elif values == "ties":
        x = np.minimum(x, np.float32(4.0))
        for s, w in zip(starts, widths):
            for cls, pair in enumerate(tie_pairs(C, int(s), int(w))):
                if pair is not None:
                    x[cls::4, pair[0]] = x[cls::4, pair[1]] = np.float32(6.0)
        x[3::4] = np.round(x[3::4])               # (the remaining rows: their own maximum, several times over)
    elif values == "argmax":                      # the confident rows: the target is the segment's largest logit
        for k, (s, w) in enumerate(zip(starts, widths)):
            rows = group == k
            target[rows] = x[rows, s:s + w].argmax(1)
    elif values == "nanrow":
        x[1::4] = np.float32(np.nan)
        mask[1::4] = False
    counts = np.asarray([int((mask & (group == k)).sum()) for k in range(K)])
    inv = np.where(counts > 0, 1.0 / np.maximum(counts, 1), 0.0).astype(np.float32)
    class_map = 1000 + 3 * np.arange(C - 1, -1, -1, dtype=np.int64)
    return _frozen(x=np.ascontiguousarray(x, dtype=np.float32), target=np.ascontiguousarray(target, dtype=np.int64), mask=mask,
                   group=group, route=route, class_map=class_map, inv_count=inv, starts=starts, widths=widths)


def own_columns(inp, pred, route):
    """bool [n, C]: the columns of a row's own training segment (of its group, selected or not) and, when the arg-max is
    wanted, of its routing segment (`route`, or the group again)"""
    n, C = inp["x"].shape
    K = len(inp["starts"])
    own = np.zeros((n, C), dtype=bool)
    col = np.arange(C)[None, :]
    for ids in (inp["group"],) + (((inp["route"] if route else inp["group"]),) if pred else ()):
        ok = (ids >= 0) & (ids < K)
        s = np.where(ok, inp["starts"][np.where(ok, ids, 0)], 0)[:, None]
        w = np.where(ok, inp["widths"][np.where(ok, ids, 0)], 0)[:, None]
        own |= (col >= s) & (col < s + w)
    return own


def poisoned(inp, pred, route):
    """the logits with NaN in every column outside the row's own segments, pad columns included"""
    return np.where(own_columns(inp, pred, route), inp["x"], np.float32(np.nan)).astype(np.float32)


# ---- the reference, and the fp32 restatement of the intended arithmetic ----------------------------------------------
def grouped_ce_of(x, target, mask, group, starts, widths, inv_count, dtype=np.float64):
    """loss_k = inv_count[k] * sum over the selected rows of group k of log(sum) - (x_t - m) inside the group's segment
    (NaN for a group without a selected row, and for one with a selected row whose target is outside [0, width)); loss = their
    sum over the groups that have a selected row; grad = softmax * inv_count[k] inside the segment of a selected row, the entry
    at the target as -(sum of the OTHER terms) / sum so that it does not cancel, 0 everywhere else; its column sums.

    dtype = float64 is the reference.  dtype = float32 is the arithmetic the kernel is meant to use, operation for operation
    (the target kept out of the sum, differences from the row maximum before the logarithm) -- what fp32 can reach."""
    f = dtype
    x = np.asarray(x).astype(f)
    n, C = x.shape
    K = len(starts)
    grad = np.zeros((n, C), dtype=f)
    loss_k = np.full(K, np.nan, dtype=f)
    loss = f(0.0)
    for k in range(K):
        rows = np.flatnonzero(mask & (group == k))
        if inv_count[k] == 0 or rows.size == 0:
            continue
        s, w = int(starts[k]), int(widths[k])
        ic = f(inv_count[k])
        seg, t = x[rows, s:s + w], target[rows]
        ok = (t >= 0) & (t < w)
        tc, i = np.where(ok, t, 0), np.arange(rows.size)
        m = seg.max(1, keepdims=True)
        with np.errstate(invalid="ignore"):
            d = seg - m
        e = np.exp(d)
        et = np.where(ok, e[i, tc], f(0.0))
        e_others = e.copy()
        e_others[i[ok], tc[ok]] = 0.0
        others = e_others.sum(1, dtype=f)
        tot = others + et
        terms = np.where(ok, np.log(tot) - d[i, tc], f(np.nan))
        loss_k[k] = terms.sum(dtype=f) * ic
        loss = loss + loss_k[k]
        inv = f(1.0) / tot
        g = e * inv[:, None]
        g[i[ok], tc[ok]] = -(others * inv)[ok]
        grad[rows, s:s + w] = g * ic
    return dict(loss=f(loss), loss_k=loss_k, grad=grad, dbias=grad.sum(0, dtype=np.float64))


def blocked_sum(a, block=64):
    """column sums of a float32 matrix in float32, 64 rows at a time and then 64 of those, as a fixed-order tree like the
    kernel's (lanes, sub-groups, waves, workgroup partials) adds them -- not one running sum over all the rows"""
    a = np.asarray(a, dtype=np.float32)
    while a.shape[0] > 1:
        pad = -a.shape[0] % block
        a = np.concatenate([a, np.zeros((pad, a.shape[1]), np.float32)]).reshape(-1, block, a.shape[1]).sum(1, dtype=np.float32)
    return a[0] if a.shape[0] else np.zeros(a.shape[1], np.float32)


def routed_pred(x, ids, starts, widths, class_map=None):
    """int64 [n]: start_q + argmax(x[r, seg_q]), q = ids[r] (the first index on ties; of a row of NaN the segment's first
    column), through `class_map` when given; -1 where q is outside [0, K)"""
    out = np.full(x.shape[0], -1, dtype=np.int64)
    for k, (s, w) in enumerate(zip(starts, widths)):
        rows = np.flatnonzero(ids == k)
        if rows.size:
            seg = x[rows, s:s + w]
            out[rows] = s + np.where(np.isnan(seg).all(1), 0, np.argmax(np.where(np.isnan(seg), -np.inf, seg), axis=1))
    if class_map is not None:
        out = np.where(out >= 0, class_map[np.maximum(out, 0)], -1)
    return out


@lru_cache(maxsize=4)
def gce_reference(C, n, seg, values):
    i = gce_inputs(C, n, seg, values)
    ref = grouped_ce_of(i["x"], i["target"], i["mask"], i["group"], i["starts"], i["widths"], i["inv_count"])
    ref["pred"] = {(route, cmap): routed_pred(i["x"], i["route"] if route else i["group"], i["starts"], i["widths"],
                                              i["class_map"] if cmap else None) for route in (False, True) for cmap in (False, True)}
    for p in ref["pred"].values():
        p.setflags(write=False)
    return _frozen(**ref)


def trained_columns(inp):
    """bool [C]: the columns of the segments that have a selected row -- everywhere else the bias gradient is exactly 0"""
    on = np.zeros(inp["x"].shape[1], dtype=bool)
    for k, (s, w) in enumerate(zip(inp["starts"], inp["widths"])):
        if inp["inv_count"][k] != 0:
            on[s:s + w] = True
    return on


def selected_rows(inp):
    K = len(inp["starts"])
    return inp["mask"] & (inp["group"] >= 0) & (inp["group"] < K)


# ---- the measure -----------------------------------------------------------------------------------------------------
def scalar_err(got, ref):
    """|got - ref| / |ref|, or |got| against a reference of exactly 0 (a group of width-1 segments)"""
    return abs(float(got) - float(ref)) / abs(float(ref)) if float(ref) != 0 else abs(float(got))


def row_err(got, ref):
    """every row of `got` against its own largest entry in `ref` (float64); a row whose largest entry is below TINY_ROW
    against that scale (see tests/_train_cases.py); an all-zero row must be all zero.  This is test_gpu_parity's
    `row_rel_err` under test_gpu_train_kernels' TINY_ROW rule, in numpy: the host test holds the fp32 restatement to it too"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.shape[0] == 0:
        return 0.0
    num, den = np.abs(got - ref).max(1), np.abs(ref).max(1)
    assert (num[den == 0] == 0).all()
    den = np.where(den == 0, 1.0, np.maximum(den, TINY_ROW))
    return float((num / den).max())


def errors(got, ref, inp):
    """{"loss", "loss_k", "row", "dbias"}: the figures one result is held to, whichever of them `got` has"""
    out = {"loss": scalar_err(got["loss"], ref["loss"])}
    fin = ~np.isnan(ref["loss_k"])
    assert np.array_equal(np.isnan(got["loss_k"]), ~fin)
    out["loss_k"] = max([scalar_err(a, b) for a, b in zip(got["loss_k"][fin], ref["loss_k"][fin])], default=0.0)
    if "grad" in got:
        sel = selected_rows(inp)
        out["row"] = row_err(got["grad"][sel], ref["grad"][sel])
    if "dbias" in got:
        out["dbias"] = float(np.abs(got["dbias"] - ref["dbias"]).max()) / max(float(np.abs(ref["dbias"]).max()), 1e-30)
    return out
