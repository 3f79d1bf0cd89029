"""Case table of the routed (per-label) fold-in kernel's sweep (tests/test_gpu_foldin_routed.py runs it through the C ABI;
tests/test_foldin_routed_host.py keeps it complete on the CPU).  Test infrastructure.

`leaf_of` restates the dispatch of csrc/foldin_routed.hip: the kernel is instantiated on
    top / given   the top network is evaluated, or the route is handed in (then the top network takes no part at all)
    tail          some h or C of a network that takes part is not a multiple of 4          -- else `vec`
    wide          some such C > 64 (a second column per lane in the epilogue)              -- else `narrow`
Exact family: as tests/_foldin_cases.py -- dis powers of two, TF-IDF multiples of 2^-8 with dis_d in {1, 1/2, 1/4}, tables, W2
and the biases small integers; every partial sum is a dyadic rational and, while the sums of absolute values stay below 2^24
units of the finest step (asserted per case), ANY fp32 evaluation in ANY order equals the float64 evaluation bit for bit --
so the top arg-max, and with it the route, is exact too.  The top b2 is chosen so that a document WITHOUT entries has equal
top logits in several columns, the first of which is not column 0: the first-arg-max rule decides its route.
Float family: random operands; the top network's P and b2 are scaled up so that every document's float64 top-logit margin
exceeds twice the top logits' forward-error bound (asserted on the CPU: zero documents excluded)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import _foldin_cases as fc
import _foldin_ref as R
import _foldin_routed_ref as RR

DOCS_PER_WORKGROUP, WORKGROUP_CAP = fc.DOCS_PER_WORKGROUP, fc.WORKGROUP_CAP
MAX_HIDDEN, MAX_CLASSES, MAX_MEMBERS, LDS_LIMIT = 256, 128, 64, 163840
LEAVES = tuple(f"{r}-{t}-{w}" for r in ("top", "given") for t in ("vec", "tail") for w in ("narrow", "wide"))
ROW_LENGTHS = fc.ROW_LENGTHS
LAYOUTS = ("tight", "padded", "reversed")      # networks back to back | 8 columns of gap after each segment | members reversed, P first
OUTS = ("route", "top", "logits", "pred", "hidden")
ROUTES = ("top", "given", "given_bad")         # the top network routes | route_in | route_in with -1 and K entries

# top: (h_0, K);  h: the members' hidden width;  Cs: the members' class counts;  acts: one per network (top first)
Case = namedtuple("Case", "family top h Cs n_docs n_vocab layout acts mode outs class_map route seed")

WIDTHS = (((1, 1), 1, (1,)), ((4, 2), 4, (8, 3)), ((8, 3), 4, (2, 68, 5)), ((100, 6), 100, (10, 11, 11, 10, 11, 11)),
          ((63, 5), 64, (65, 1, 4, 7, 9)), ((5, 64), 8, tuple(1 + k % 4 for k in range(64))), ((256, 2), 256, (128, 4)),
          ((8, 4), 4, (8, 4, 12, 4)), ((8, 4), 8, (68, 4, 8, 72)))
OVER_THE_LIMIT = ((256, 2), 256, (128, 128))    # two W2 of 128 KiB


def nets_of(c):
    """[(h, C)] of the networks that take part."""
    return ([c.top] if c.route == "top" else []) + [(c.h, C) for C in c.Cs]


def leaf_of(c):
    nets = nets_of(c)
    tail = any(h % 4 or C % 4 for h, C in nets)
    return f"{'top' if c.route == 'top' else 'given'}-{'tail' if tail else 'vec'}-{'wide' if any(C > 64 for _, C in nets) else 'narrow'}"


def widths_arrays(c, with_top=True):
    """(h [K + 1], C [K + 1]) as tgcn_foldin_routed_lds_bytes takes them."""
    top = c.top if with_top else (0, 0)
    return [top[0]] + [c.h] * len(c.Cs), [top[1]] + list(c.Cs)


def case_id(c):
    cs = "_".join(str(v) for v in c.Cs) if len(c.Cs) <= 6 else f"{len(c.Cs)}members"
    return (f"{c.family}-{c.top[0]}x{c.top[1]}-h{c.h}-{cs}-B{c.n_docs}-{c.layout}-a{sum(c.acts)}-{c.mode[:3]}-"
            f"{''.join(o[0] for o in c.outs)}-{'map' if c.class_map else 'local'}-{c.route}-s{c.seed}")


def _variant(family, i, widths, n_docs, n_vocab=37, route=None):
    """Option values cycle with the case index at co-prime periods."""
    top, h, Cs = widths
    acts = tuple((i + m + (m * m) // 3) % 2 for m in range(len(Cs) + 1))
    route = route or ROUTES[i % 3]
    outs = tuple(o for k, o in enumerate(OUTS) if (k == 2 or (i + k) % 2) and not (o == "top" and route != "top"))
    return Case(family, top, h, tuple(Cs), n_docs, n_vocab, LAYOUTS[(i // 2) % 3], acts, (R.REFERENCE, R.ACCURATE)[(i // 3) % 2],
                outs, bool((i // 2) % 2), route, 500 + i)


def int_cases():
    cases, i = [], 0
    for widths in WIDTHS:                              # every row length in every shape: 8 documents + 9 short ones = a tile + 1
        for route in ("top", "given"):
            cases.append(_variant("int", i, widths, DOCS_PER_WORKGROUP + 1, route=route))
            i += 1
        cases.append(_variant("int", i, widths, DOCS_PER_WORKGROUP + 1))
        i += 1
    # the batch sizes: none, one, a tile - 1, a tile, and two grid strides + 1 (short rows)
    for n_docs in (0, 1, DOCS_PER_WORKGROUP - 1, DOCS_PER_WORKGROUP, 2 * DOCS_PER_WORKGROUP * WORKGROUP_CAP + 1):
        for widths in (((4, 2), 4, (8, 3)), ((8, 3), 4, (2, 68, 5))):
            cases.append(_variant("int", i, widths, n_docs))
            i += 1
    # every output off and on, alone and together, with and without the class map, on a top and a given leaf
    for widths, route in ((((4, 2), 4, (8, 3)), "top"), (((8, 3), 4, (2, 68, 5)), "given_bad")):
        for outs in (("route",), ("top",), ("logits",), ("pred",), ("hidden",), OUTS):
            if route != "top":
                outs = tuple(o for o in outs if o != "top") or ("pred", "hidden")
            for cm in (False, True):
                cases.append(_variant("int", i, widths, 9, route=route)._replace(outs=outs, class_map=cm))
                i += 1
    return cases


FLOAT_SHAPES = (((64, 4), 64, (64, 8, 4, 12)), ((100, 6), 100, (10, 11, 11, 10, 11, 11)), ((63, 5), 64, (65, 1, 4, 7, 9)),
                ((8, 4), 8, (68, 4, 8, 72)))


def float_cases():
    out = []
    for i, widths in enumerate(FLOAT_SHAPES * 4):
        route = ("top", "given", "top", "given_bad")[i // len(FLOAT_SHAPES)]
        c = _variant("float", i, widths, DOCS_PER_WORKGROUP + 1, n_vocab=301, route=route)
        out.append(c._replace(outs=tuple(o for o in OUTS if o != "top" or route == "top")))
    return out


def row_lengths(c):
    return fc.row_lengths(fc.Case(c.family, 1, 1, c.n_docs, c.n_vocab, "tight", False, 0, c.mode, False, False, 0))


def route_given(c):
    """The route handed in (None when the top network routes): every member in turn; `given_bad` also names nobody."""
    if c.route == "top":
        return None
    K = len(c.Cs)
    r = np.array([(d * 7 + 3) % K for d in range(c.n_docs)], dtype=np.int32)
    if c.route == "given_bad":
        r[1::5] = -1
        r[2::5] = K
        r[4::11] = -(2 ** 31)
    return r


def class_map_of(c):
    """K lists of distinct global classes (ascending inside a member, as `relabel` returns them), or None."""
    if not c.class_map:
        return None
    rng = np.random.default_rng(c.seed + 7)
    return [np.sort(rng.choice(1000, size=C, replace=False)).tolist() for C in c.Cs]


def _net(rng, V, h, C, exact, act):
    if exact:
        T1, P = rng.integers(-1, 2, size=(V, h)), rng.integers(-2, 3, size=(V, C))
        W2 = rng.integers(-1, 2, size=(h, C)) * (rng.random((h, C)) < 0.5)
        b1, b2 = rng.integers(-2, 3, size=h), rng.integers(-2, 3, size=C)
    else:
        T1, P, W2 = rng.standard_normal((V, h)), rng.standard_normal((V, C)), rng.standard_normal((h, C)) / np.sqrt(h)
        b1, b2 = rng.standard_normal(h), rng.standard_normal(C)
    net = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in dict(T1=T1, P=P, W2=W2, b1=b1, b2=b2).items()}
    net["act"] = act
    return net


@lru_cache(maxsize=4)
def operands(c):
    """dict of host arrays: rowptr, col, val, dis and `nets` (dicts as tests/_foldin_routed_ref.py takes them; nets[0] is the
    top network and is there in every case -- a `given` case must not read it).  Documents carry first / last / duplicate
    columns and, every fourth one, a column outside [0, V) (skipped in the sums)."""
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
        vals.append(fc._dyadic_row(rng, n) if c.family == "int" else (rng.random(n) * 0.9 + 0.05).astype(np.float32))
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, dtype=np.int32)
    val = np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, dtype=np.float32)
    exact = c.family == "int"
    dis = (2.0 ** -rng.integers(0, 4, size=V)) if exact else (rng.random(V) * 0.95 + 0.05)
    K = len(c.Cs)
    top = _net(rng, V, c.top[0], K, exact, c.acts[0])
    if exact:
        # a document without entries has u = act(b1), a_dd = 1 and z = u W2 + b2: with b2 = t - u W2 its top logits are t,
        # whose maximum 1 sits in column 1 first (K >= 3: and again in the last column)
        u = top["b1"].astype(np.float64)
        if top["act"]:
            u = np.maximum(u, 0.0)
        t = rng.integers(0, 2, size=K)
        t[0] = 0
        t[1 % K] = 1 if K > 1 else 0
        t[-1] = 1 if K > 1 else 0
        top["b2"] = (t - u @ top["W2"].astype(np.float64)).astype(np.float32)
    else:
        top["P"] *= np.float32(8.0)                     # the margins of the top logits: far above their rounding error
        top["b2"] *= np.float32(8.0)
    nets = [top] + [_net(rng, V, c.h, C, exact, c.acts[1 + k]) for k, C in enumerate(c.Cs)]
    return dict(rowptr=rowptr, col=col, val=val, dis=np.ascontiguousarray(dis, dtype=np.float32), nets=nets)


@lru_cache(maxsize=4)
def reference(c):
    """The float64 evaluation (tests/_foldin_routed_ref.py:foldin_routed with the bounds) and, for the exact family, `units`:
    the largest sum of absolute values in units of the document's finest dyadic step (must stay below 2^24)."""
    o = operands(c)
    ref = RR.foldin_routed(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["nets"], route_given(c), np.float64,
                           want_bounds=True)
    if c.family == "int":
        _, _, dis_d = R.doc_scalars(o["rowptr"], np.clip(o["col"].astype(np.int64), 0, c.n_vocab - 1), o["val"], o["dis"], c.mode)
        assert set(np.unique(dis_d).tolist()) <= {1.0, 0.5, 0.25}
        # finest step of a document: a_j = t (2^-8) dis (>= 2^-3) dis_d; z is a_dd = dis_d^2 finer
        step_u = (2.0 ** -(fc.T_UNIT_LOG2 + 3) * dis_d.astype(np.float64))[:, None] if c.n_docs else np.ones((0, 1))
        step_z = step_u * (dis_d.astype(np.float64) ** 2)[:, None] if c.n_docs else step_u
        units = max(float((ref["absu"] / step_u).max(initial=0.0)), float((ref["absz"] / step_z).max(initial=0.0)))
        top = ref["top"]
        if top is not None:
            n0 = o["nets"][0]
            zabs = top["Zp"] + top["a_dd"].astype(np.float64)[:, None] * (np.abs(top["u"]) @ np.abs(n0["W2"].astype(np.float64))) \
                + np.abs(n0["b2"].astype(np.float64))[None, :]
            units = max(units, float((top["U"] / step_u).max(initial=0.0)), float((zabs / step_z).max(initial=0.0)))
            assert np.array_equal(top["z"].astype(np.float32).astype(np.float64), top["z"])
        ok = np.isfinite(ref["z"])
        assert np.array_equal(ref["z"][ok].astype(np.float32).astype(np.float64), ref["z"][ok])
        assert np.array_equal(ref["u"].astype(np.float32).astype(np.float64), ref["u"])
        ref["units"] = units
    return ref
