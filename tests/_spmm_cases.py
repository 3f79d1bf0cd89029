"""Cases of the exact sweep over the SpMM kernels (tests/test_gpu_spmm_exact.py): operators as host COO triplets with the
partition knobs they are built under, integer operands, the independent reference (scipy.sparse, int64, from the triplets --
never from tgcn_plan_export), the strided layouts, the generated case list and the dispatch of csrc/spmm.hip /
csrc/plan.hip RESTATED, so that a case names the kernel leaves it launches.  CPU only: numpy and scipy; nothing here imports
torch or the library.  Test infrastructure; tests/test_spmm_cases.py keeps the list complete.

Why the comparison may be bit for bit: operator values are integers in +-{1, 2, 3}, X holds integers in [-7, 7], bias and
the accumulate form's initial Y integers in [-50, 50].  Every partial sum of any summation order is then an integer of
magnitude <= `exact_bound` = max over rows of (sum |m|) * 7 + 50 + 50 (an upper bound of sum |m||x| + |bias| + |y0|);
below 2^24 every such integer IS an fp32 value, no addition rounds, and ANY correct kernel -- segment sums, the
sub-group shuffles, the MFMA hot block with its pre-summed duplicates, k_spmm_fix in any grouping -- returns the same bits.

The restated lines (cited where they stand): `launch_spmm` (the vec4 test), `launch_vec` (which kernel, `buf_ok`, `nt`,
tiles) in csrc/spmm.hip; pass 1 of `build_items`, the hot-block condition, `cpw` / `hot_parts`, `emit_piece` (segments
without column cuts) and `item_weight_for` in csrc/plan.hip."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np
from scipy import sparse

EXACT_LIMIT = 1 << 24
INT32_MAX = (1 << 31) - 1
BUF_LIMIT = 0xFFFF0000                          # launch_vec: `x_extent <= 0xFFFF0000ull`
K_HOT_ROWS = 32                                 # common.h: kHotRows
HOT_MIN_COLS = 4096                             # build_items: `b.n_cols >= 4096`
X_MAX, B_MAX, M_MAX = 7, 50, 3
BYTES_CAP = 64 << 20                            # operands + results + workspace of one case (hot_cpw72 at F = 32: 17 MB of X)
KNOB_NAMES = ("TGCN_ITEM_WEIGHT", "TGCN_COL_BLOCK", "TGCN_MIN_PIECE", "TGCN_HOT_RATIO", "TGCN_HOT_ROWS")

FLOAT4_WIDTHS = (4, 8, 32, 36, 60, 64, 68, 96, 124, 128, 132, 160, 192, 196, 224, 228, 256, 260, 512, 516)
SCALAR_WIDTHS = (1, 2, 3, 5, 63, 65, 127, 129, 130)
PIVOTS = (8, 64, 128, 200, 260)
SCALAR_PIVOTS = (5, 130)                        # tight / pad cases of the scalar leaves in every form
FORMS = ("plain", "relu", "acc", "split", "adam")
LAYOUTS = ("tight", "pad", "odd_ldx", "odd_ldy", "x_off", "y_off", "bias_off", "x2_off", "odd_ldx2")
SCALAR_CAUSES = LAYOUTS[2:]
SEGS_COUNTS = (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 70)        # slots per long row of `segs` (item weight 64, no column cuts)
ADAM_LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8

GATHER_LEAVES = ("gather<4,P3>", "gather<4,P1,acc>", "gather<4,P3,relu>", "gather<1,P0>", "gather<1,P0,acc>", "gather<1,P0,relu>")
SUBB_LEAVES = tuple(f"subb<{g}{f}>" for g in (16, 32) for f in ("", ",acc", ",relu"))
HOT_LEAVES = tuple(f"hot<{k}>" for k in range(1, 9))
FIX_LEAVES = ("fix<4>", "fix<4,adam>", "fix<4,acc>", "fix<4,relu>", "fix<1>", "fix<1,acc>", "fix<1,relu>")
LEAVES = GATHER_LEAVES + ("gather_adam<4>",) + SUBB_LEAVES + HOT_LEAVES + FIX_LEAVES
SCALAR_LEAVES = tuple(l for l in LEAVES if l.startswith(("gather<1", "fix<1")))

Op = namedtuple("Op", "name n_cols knobs swap values")
Op.__doc__ = """An operator and the knob set it is built under: structure `name` (at `n_cols` columns for the hot ones), knobs as
((env name, value), ...), `swap`: the plan is created from the TRANSPOSED triplets, so that transpose = 1 applies the
structure itself through the plan's backward block (hot block included); values "int" or "float"."""
Adam = namedtuple("Adam", "amsgrad wd dev")
Case = namedtuple("Case", "op t form F layout bias split adam")
Case.__doc__ = """operator, transpose flag of the call, form (FORMS), width, layout (LAYOUTS), bias given, split position of
the operand (None: one operand), Adam(amsgrad, weight decay, scalars on the device) for the adam form"""
Layout = namedtuple("Layout", "ldx ldy ldx2 ldp off_x off_y off_b off_x2")


def _h(*v):
    return zlib.crc32(repr(v).encode())


# ---- operators ------------------------------------------------------------------------------------------------------
_DEFAULT_KNOBS = {"short": (), "segs": (("TGCN_ITEM_WEIGHT", "64"), ("TGCN_COL_BLOCK", "0"))}
_HOT_KNOBS = (("TGCN_HOT_RATIO", "0.5"), ("TGCN_COL_BLOCK", "0"))
_HOT_COLS = {"hot12": 4096, "hot40": 4096, "hot_parts34": 16897, "hot_cpw72": 131080}


def make_op(name, n_cols=None, knobs=(), swap=False, values="int"):
    """`knobs` are set ON TOP of the structure's own set"""
    base = dict(_DEFAULT_KNOBS.get(name, _HOT_KNOBS))
    base.update(dict(knobs))
    if n_cols is None:
        n_cols = {"short": 700, "segs": 900}.get(name) or _HOT_COLS[name]
    return Op(name, n_cols, tuple(sorted(base.items())), swap, values)


def op_id(op):
    s = op.name + (f"_{op.n_cols}" if op.name in ("hot12", "hot40") else "")
    own = dict(_DEFAULT_KNOBS.get(op.name, _HOT_KNOBS))
    extra = [f"{k[5:].lower()}{v}" for k, v in op.knobs if own.get(k) != v]
    return s + "".join("_" + e for e in extra) + ("_swap" if op.swap else "") + ("_float" if op.values == "float" else "")


def _fill_rows(gen, n_cols, degrees, dup_every=5):
    rows, cols = [], []
    for r, d in enumerate(degrees):
        if d == 0:
            continue
        c = gen.choice(n_cols, d, replace=(d > n_cols or r % dup_every == 0))
        rows.append(np.full(d, r))
        cols.append(c)
    return rows, cols


def _short(gen, n_cols):
    """700 x 700 at the default item weight (128): 70 leading empty rows in a block that goes on past its 64th row; a row
    of degree 127, which closes its block, then a run of 200 empty rows (a block of 128 of them); a row of degree 127 again,
    then 63 empty rows and three of degree 1 at positions 63, 64, 65 of the next block; degrees 1..12 elsewhere; trailing empty rows"""
    deg = [0] * 70 + [1 + i % 12 for i in range(120)] + [127] + [0] * 200 + [127] + [0] * 63 + [1, 1, 1] + [0] * 40
    deg += [1 + (i * 5) % 12 for i in range(150)]
    deg += [0] * (700 - len(deg))
    return 700, _fill_rows(gen, n_cols, deg)


def _segs(gen, n_cols):
    """600 x 900 at item weight 64: long rows of degree 65, 129, 900 (every column once) next to one of 64 (not long); rows
    of 2 .. 70 segments (degrees above 900 hold duplicates); a long first and last row; 40 empty rows; three hub columns
    (0, 450, 899) that make long rows of the transposed operator"""
    special = {0: 65, 7: 129, 8: 900, 9: 64, 20: 128, 21: 256, 22: 320, 60: 1024, 61: 1088, 200: 1984, 201: 2048, 300: 2112,
               301: 4480, 599: 193}
    deg = [special.get(r, 0 if 100 <= r < 140 else (r * 7) % 13) for r in range(600)]
    rows, cols = _fill_rows(gen, n_cols, deg)
    for i, r in enumerate(np.unique(np.concatenate(rows))):
        if deg[r] == 900:
            cols[i] = np.arange(900)
    hub_rows = np.array([r for r in range(600) if r % 3 and not 100 <= r < 140 and r not in special])
    for hub in (0, 450, 899):
        rows.append(hub_rows)
        cols.append(np.full(hub_rows.size, hub))
    return 600, (rows, cols)


def _hot(n_long, n_rows, deg0, step):
    def build(gen, n_cols):
        """`n_long` long rows of distinct degrees with duplicate columns, column 0 and column n_cols - 1 (four times each)
        and the columns around the last workgroup's start; the other rows short (0 .. 10 entries), the last ten empty"""
        long_at = {3 + (n_rows - 20) // n_long * i: deg0 + step * i for i in range(n_long)}
        deg = [long_at.get(r, 0 if r >= n_rows - 10 else (r * 5) % 11) for r in range(n_rows)]
        rows, cols = _fill_rows(gen, n_cols, deg)
        edge = np.array([0] * 4 + [n_cols - 1] * 4 + [n_cols - 2, min(4095, n_cols - 1), min(4096, n_cols - 1), 511, 512])
        for i, r in enumerate(sorted(r for r in range(n_rows) if deg[r])):
            if r in long_at:
                cols[i] = np.concatenate([gen.choice(n_cols, deg[r], replace=True), edge])
                rows[i] = np.full(cols[i].size, r)
        for i in range(len(cols)):              # columns 1000 .. 1019 stay unused: empty rows of the transposed operator
            cols[i] = np.where((cols[i] >= 1000) & (cols[i] < 1020), cols[i] + 20, cols[i])
        return n_rows, (rows, cols)
    return build


_STRUCTURES = {"short": _short, "segs": _segs, "hot12": _hot(12, 300, 300, 37), "hot40": _hot(40, 300, 300, 37),
               "hot_parts34": _hot(34, 200, 400, 13), "hot_cpw72": _hot(34, 64, 1800, 40)}


@lru_cache(maxsize=None)
def _structure(name, n_cols):
    gen = np.random.default_rng(_h("structure", name, n_cols))
    n_rows, (rows, cols) = _STRUCTURES[name](gen, n_cols)
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    perm = gen.permutation(rows.size)                       # COO order is the caller's: the plan sorts
    rows, cols = rows[perm], cols[perm]
    ints = gen.choice(np.array([-3, -2, -1, 1, 2, 3]), rows.size)
    floats = (gen.random(rows.size) - 0.3).astype(np.float32)
    return n_rows, rows, cols, ints, floats


def structure(op):
    """(n_rows, n_cols, rows, cols, vals) of the structure itself"""
    n_rows, rows, cols, ints, floats = _structure(op.name, op.n_cols)
    return n_rows, op.n_cols, rows, cols, ints if op.values == "int" else floats


def plan_coo(op):
    """what tgcn_plan_create_coo is given: (n_rows, n_cols, row, col, val)"""
    n_rows, n_cols, rows, cols, vals = structure(op)
    return (n_cols, n_rows, cols, rows, vals) if op.swap else (n_rows, n_cols, rows, cols, vals)


def applied(op, t):
    """(n_out, n_in, rows, cols, vals) of the matrix a call with transpose = t multiplies by"""
    n_rows, n_cols, rows, cols, vals = plan_coo(op)
    return (n_cols, n_rows, cols, rows, vals) if t else (n_rows, n_cols, rows, cols, vals)


# ---- csrc/plan.hip restated -----------------------------------------------------------------------------------------
def item_weight(op, t):
    """item_weight_for: `if (v >= 64 && v <= (1 << 20)) return v; return b.nnz + b.n_rows < (24 << 20) ? 128 : 384`"""
    v = int(dict(op.knobs).get("TGCN_ITEM_WEIGHT", 0))
    if 64 <= v <= 1 << 20:
        return v
    n_out, _, rows, _, _ = applied(op, t)
    return 128 if rows.size + n_out < 24 << 20 else 384


def partition(deg, T):
    """pass 1 of build_items: rows of degree <= T packed into blocks that close at weight (degree + 1 per row) >= T, a row
    of degree > T is long and closes the block before it.  Returns ([(row_begin, row_end)], [long rows])."""
    blocks, long_rows, r0, w = [], [], 0, 0
    for r, d in enumerate(deg):
        if d > T:
            if r > r0:
                blocks.append((r0, r))
            long_rows.append(r)
            r0, w = r + 1, 0
        else:
            w += d + 1
            if w >= T:
                blocks.append((r0, r + 1))
                r0, w = r + 1, 0
    if r0 < len(deg):
        blocks.append((r0, len(deg)))
    return blocks, long_rows


Facts = namedtuple("Facts", "T deg blocks long_rows n_hot hot_rows hot_cpw hot_parts exact_segments seg_counts segments "
                            "segments_all n_items n_items_all")


@lru_cache(maxsize=None)
def facts(op, t):
    """The partition of the applied block as build_items makes it.  n_hot: `kn.hot_rows > 0 && n_long > 0 && b.n_cols >=
    4096`, the k = min(32, n_long) longest long rows (ties: the earlier row), `sum >= hot_ratio * n_cols`.  cpw / parts:
    `cpw = max(64, round_up8(ceil(n_cols / 2048)))`, `hot_parts = ceil(n_cols / (8 cpw))`.  Without column cuts (`n_cb == 0`:
    TGCN_COL_BLOCK = 0 or one column block) a long row of degree d is `nseg = (d + T - 1) / T` slots (emit_piece); the list
    next to the hot block leaves the hot rows out and appends n_hot * hot_parts slots."""
    kn = dict(op.knobs)
    n_out, n_in, rows, _, _ = applied(op, t)
    deg = np.bincount(rows, minlength=n_out)
    T = item_weight(op, t)
    blocks, long_rows = partition(deg.tolist(), T)
    n_hot, hot_rows, cpw, parts = 0, (), 0, 0
    if int(kn.get("TGCN_HOT_ROWS", 1)) > 0 and long_rows and n_in >= HOT_MIN_COLS:
        order = sorted(range(len(long_rows)), key=lambda i: (-deg[long_rows[i]], i))[:K_HOT_ROWS]
        if float(sum(deg[long_rows[i]] for i in order)) >= float(kn.get("TGCN_HOT_RATIO", 2.0)) * float(n_in):
            hot_rows = tuple(long_rows[i] for i in order)
            n_hot = len(hot_rows)
            cpw = max(64, ((n_in + 2047) // 2048 + 7) // 8 * 8)
            parts = (n_in + 8 * cpw - 1) // (8 * cpw)
    col_block = int(kn.get("TGCN_COL_BLOCK", 8192))
    n_cb = (n_in + col_block - 1) // col_block if long_rows and col_block > 0 else 0
    exact = not 1 < n_cb <= 8192
    counts = {r: -(-int(deg[r]) // T) for r in long_rows}
    seg_all = sum(counts.values())
    seg_main = sum(c for r, c in counts.items() if r not in hot_rows) + n_hot * parts
    return Facts(T, deg, tuple(blocks), tuple(long_rows), n_hot, hot_rows, cpw, parts, exact, counts,
                 seg_main if exact else None, (seg_all if n_hot else 0) if exact else None,
                 len(blocks) + (seg_main - n_hot * parts) if exact else None, len(blocks) + seg_all if exact else None)


def workspace_floats(c):
    """tgcn_spmm_workspace_bytes / 4: `max(b.n_segments, b.n_segments_all) * round_up4(F)` (known without column cuts)"""
    f = facts(c.op, c.t)
    return None if not f.exact_segments else max(f.segments, f.segments_all) * ((c.F + 3) // 4 * 4)


# ---- layouts and csrc/spmm.hip restated ------------------------------------------------------------------------------
def layout(c):
    """tight: every leading dimension F.  pad: ldx, ldx2 = F + 4 or F + 12, ldy the other one, ldp = F + 8.  The others
    force the scalar kernels at F % 4 == 0, one cause each: a leading dimension of F + 1, or a base 4 bytes past 16."""
    F = c.F
    pad = 4 if _h(c.op.name, c.F, c.form) % 2 else 12
    ld = {"x": F, "y": F, "x2": F, "p": F}
    off = {"x": 0, "y": 0, "b": 0, "x2": 0}
    if c.layout == "pad":
        ld = {"x": F + pad, "y": F + 16 - pad, "x2": F + pad, "p": F + 8}
    elif c.layout.startswith("odd_ld"):
        ld[c.layout[6:]] = F + 1
    elif c.layout.endswith("_off"):
        off[{"bias": "b"}.get(c.layout[:-4], c.layout[:-4])] = 1
    return Layout(ld["x"], ld["y"], ld["x2"], ld["p"], off["x"], off["y"], off["b"], off["x2"])


def applies(form, lay, bias, split):
    """whether a layout names a buffer the call has"""
    if form == "adam":
        return lay in ("tight", "pad")
    if lay == "bias_off":
        return bias
    if lay in ("x2_off", "odd_ldx2"):
        return split is not None
    return True


def is_vec4(c):
    """launch_spmm: `(F % 4 == 0) && (ldx % 4 == 0) && (ldx2 % 4 == 0) && (ldy % 4 == 0) && (align % 16 == 0)` over X, X2, Y,
    bias, carry (one operand: X2 = X); tgcn_spmm_adam refuses anything else"""
    if c.form == "adam":
        return True
    L = layout(c)
    ok = c.F % 4 == 0 and L.ldx % 4 == 0 and L.ldy % 4 == 0 and not L.off_x and not L.off_y and not (c.bias and L.off_b)
    if c.split is not None:
        ok = ok and L.ldx2 % 4 == 0 and not L.off_x2
    return ok


def buf_ok(c):
    """launch_vec: `split == INT32_MAX && x_extent <= 0xFFFF0000`, x_extent = ((n_cols - 1) * ldx + F) * 4"""
    n_in = applied(c.op, c.t)[1]
    return c.split is None and ((n_in - 1) * layout(c).ldx + c.F) * 4 <= BUF_LIMIT


def hot_nt(F):
    """launch_vec: `nt = min(8, (F + 31) / 32)`; launch_hot: grid.y = ceil(F / (32 nt))"""
    nt = min(8, (F + 31) // 32)
    return nt, (F + 32 * nt - 1) // (32 * nt)


def tiles(c):
    """launch_vec: `tiles = (F + 64 * VEC - 1) / (64 * VEC)`"""
    w = 256 if is_vec4(c) else 64
    return (c.F + w - 1) // w


def leaf_of(c):
    """the kernels launch_vec<VEC> launches for the case"""
    f = facts(c.op, c.t)
    vec = 4 if is_vec4(c) else 1
    acc, relu, adam = c.form == "acc", c.form == "relu", c.form == "adam"
    tag = ",adam" if adam else ",acc" if acc else ",relu" if relu else ""
    leaves = set()
    if vec == 4 and f.n_hot > 0:
        leaves.add(f"hot<{hot_nt(c.F)[0]}>")
    use_all = vec == 1 and f.n_hot > 0                        # the scalar kernels take the complete partition
    n_items = len(f.blocks) + (len(f.long_rows) if use_all else len(f.long_rows) - f.n_hot)      # > 0 is all that matters
    if n_items > 0:
        if adam:
            leaves.add("gather_adam<4>")
        elif vec == 4 and c.F <= 128 and buf_ok(c):
            leaves.add(f"subb<{16 if c.F <= 64 else 32}{tag}>")
        else:
            leaves.add(f"gather<{vec},P{(1 if acc else 3) if vec == 4 else 0}{tag}>")
    if f.long_rows:
        leaves.add(f"fix<{vec}{tag}>")
    return leaves


# ---- cases -----------------------------------------------------------------------------------------------------------
def case_id(c):
    s = f"{op_id(c.op)}-{'T' if c.t else 'N'}-{c.form}-F{c.F}-{c.layout}"
    s += ("-bias" if c.bias else "") + (f"-s{c.split}" if c.split is not None else "")
    if c.adam:
        s += f"-{'ams' if c.adam.amsgrad else 'noams'}-wd{c.adam.wd:g}-{'dev' if c.adam.dev else 'host'}"
    return s


def _split_positions(op, t):
    n_in = applied(op, t)[1]
    pos = [0, 1, n_in // 2, n_in - 1]
    if facts(op, t).n_hot:
        pos.append(700)                         # inside workgroup 1 (columns 512 .. 1023), wave 2, not on a load stage
    return pos


_ADAMS = (Adam(True, 0.0, False), Adam(False, 0.01, False), Adam(True, 0.01, True), Adam(False, 0.0, True))


def _forms(op, t, F, lay):
    """every variant of every form that a layout applies to, at one width"""
    n_in = applied(op, t)[1]
    mid = 700 if facts(op, t).n_hot else n_in // 2
    out = []
    full = lay in ("tight", "pad")
    for bias in ((True, False) if full else (True,)):
        out += [("plain", bias, None, None), ("relu", bias, None, None)]
    out += [("acc", False, None, None), ("acc", False, mid, None)]
    out += [("split", True, s, None) for s in (_split_positions(op, t) if full else (mid,))]
    if F % 4 == 0 and full:
        out += [("adam", False, None, a) for a in _ADAMS] + [("adam", False, mid, Adam(True, 0.01, False))]
    return [Case(op, t, form, F, lay, bias, split, adam) for form, bias, split, adam in out if applies(form, lay, bias, split)]


@lru_cache(maxsize=None)
def int_cases():
    segs, short = make_op("segs"), make_op("short")
    hot40, hot12 = make_op("hot40", 4097), make_op("hot12", 4100)
    cases = []
    # every width, both directions, on segments and on the hot block
    for op in (segs, hot40):
        for t in (0, 1):
            for F in FLOAT4_WIDTHS + SCALAR_WIDTHS:
                cases += [Case(op, t, "plain", F, "tight", True, None, None), Case(op, t, "relu", F, "tight", True, None, None),
                          Case(op, t, "plain", F, "pad", True, None, None)]
    # every form and layout at the pivot widths
    for op in (short, segs, hot12):
        for F in PIVOTS:
            for lay in LAYOUTS:
                cases += _forms(op, 0, F, lay)
        for F in SCALAR_PIVOTS:
            for lay in ("tight", "pad"):
                cases += _forms(op, 0, F, lay)
    # the cut, merge and short-tail paths of the long rows
    for knobs in ((("TGCN_COL_BLOCK", "16"), ("TGCN_MIN_PIECE", "4")), (("TGCN_COL_BLOCK", "7"), ("TGCN_MIN_PIECE", "1"))):
        op = make_op("segs", knobs=knobs)
        for t in (0, 1):
            for F in (8, 64, 200, 5):
                cases += [Case(op, t, "plain", F, "tight", True, None, None), Case(op, t, "relu", F, "pad", True, None, None),
                          Case(op, 0, "acc", F, "tight", False, None, None)]      # (the transpose has no empty row)
                if F % 4 == 0:
                    cases.append(Case(op, t, "adam", F, "pad", False, None, _ADAMS[0]))
    # the hot block at every column count, its transposes, the same rows as segments, the block of the backward plan
    hot_ops = [make_op(n, nc) for n in ("hot12", "hot40") for nc in (4096, 4097, 4100)]
    hot_ops += [make_op(n, 4097, knobs=(("TGCN_HOT_ROWS", "0"),)) for n in ("hot12", "hot40")]
    for op in hot_ops + [make_op("hot40", 4096, swap=True)]:
        for t in ((1,) if op.swap else (0, 1)):
            for F in (8, 64, 200, 260):
                mid = 700 if facts(op, t).n_hot else applied(op, t)[1] // 2
                cases += [Case(op, t, "plain", F, "tight", True, None, None), Case(op, t, "relu", F, "pad", True, None, None),
                          Case(op, t, "acc", F, "tight", False, None, None), Case(op, t, "split", F, "pad", True, mid, None),
                          Case(op, t, "adam", F, "tight", False, None, _ADAMS[2])]
    parts34 = make_op("hot_parts34")
    for F in (4, 8, 32, 36, 60, 64, 5):
        cases += [Case(parts34, 0, "plain", F, "tight", True, None, None), Case(parts34, 0, "relu", F, "pad", True, None, None),
                  Case(parts34, 0, "acc", F, "pad", False, None, None), Case(parts34, 0, "split", F, "tight", True, 700, None)]
        if F % 4 == 0:
            cases.append(Case(parts34, 0, "adam", F, "pad", False, None, _ADAMS[1]))
    cpw72 = make_op("hot_cpw72")
    for F in (8, 32):
        cases += [Case(cpw72, 0, "plain", F, "tight", True, None, None), Case(cpw72, 0, "relu", F, "tight", True, None, None),
                  Case(cpw72, 0, "acc", F, "tight", False, None, None)]
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return tuple(out)


@lru_cache(maxsize=None)
def float_cases():
    """The integer sweep cannot see a change that lowers precision (small integers are exact in bf16 too): random fp32
    values, float64 reference, the forward-error bound of `float_bound`"""
    out = []
    for op in (make_op("segs", values="float"), make_op("hot40", 4097, values="float"), make_op("short", values="float")):
        for F in PIVOTS:
            out += [Case(op, 0, "plain", F, "tight", True, None, None), Case(op, 0, "acc", F, "tight", False, None, None),
                    Case(op, 0, "relu", F, "tight", True, None, None)]
    return tuple(out)


def grouped(cases):
    """[(operator, form)] -> cases, in order of first appearance: one pytest item each"""
    groups = {}
    for c in cases:
        groups.setdefault((op_id(c.op), c.form), []).append(c)
    return list(groups.values())


def needs_transpose(op):
    return any(c.t for c in int_cases() + float_cases() if c.op == op)


# ---- operands and reference ------------------------------------------------------------------------------------------
@lru_cache(maxsize=4)
def _product(op, t, F):
    """X, M X and |M| |X| from the triplets: int64 for the integer family, float64 for the float one"""
    n_out, n_in, rows, cols, vals = applied(op, t)
    gen = np.random.default_rng(_h("x", op.name, op.n_cols, t, F))
    if op.values == "int":
        X = gen.integers(-X_MAX, X_MAX + 1, size=(n_in, F)).astype(np.int64)
        vals = vals.astype(np.int64)
    else:
        X = gen.standard_normal((n_in, F)).astype(np.float32).astype(np.float64)
        vals = vals.astype(np.float64)
    M = sparse.csr_matrix((vals, (rows, cols)), shape=(n_out, n_in))           # (duplicates add up)
    MX = np.asarray(M @ X)
    ABS = np.zeros_like(MX)
    if op.values == "float":
        ABS = np.asarray(sparse.csr_matrix((np.abs(vals), (rows, cols)), shape=(n_out, n_in)) @ np.abs(X))
    return X, MX, ABS


def exact_bound(c):
    """(largest sum of |m| over a row) * max|x| + max|bias| + max|y0|: an upper bound of max over rows of
    sum |m||x| + |bias| + |y0|, hence of every partial sum in any order"""
    n_out, _, rows, _, vals = applied(c.op, c.t)
    row_abs = np.bincount(rows, weights=np.abs(vals), minlength=n_out)
    return float(row_abs.max()) * X_MAX + (B_MAX if c.bias else 0) + (B_MAX if c.form == "acc" else 0)


def reference(c):
    """operands and expected result of a case (float32-exact arrays):
    x, bias (or None), y0 (acc), pre = M X + bias (+ y0), want (relu applied), has = rows with stored entries, and for the
    float family bound = gamma_{d+2} (sum |m||x| + |bias| + |y0|) per element; adam: p, m, v, vmax and grad = M X"""
    X, MX, ABS = _product(c.op, c.t, c.F)
    n_out = MX.shape[0]
    fl = c.op.values == "float"
    gen = np.random.default_rng(_h("operands", case_id(c)))
    draw = (lambda shape: gen.standard_normal(shape).astype(np.float32).astype(np.float64)) if fl else \
           (lambda shape: gen.integers(-B_MAX, B_MAX + 1, size=shape).astype(np.int64))
    out = {"x": X.astype(np.float32), "bias": None, "y0": None, "has": facts(c.op, c.t).deg > 0}
    pre, mag = MX, ABS
    if c.bias:
        # (relu: a bias no larger than a short row's sum, so that pre-activations fall on both sides of zero at F = 1 too)
        b = draw((c.F,)) if fl or c.form != "relu" else gen.integers(-6, 7, size=(c.F,)).astype(np.int64)
        out["bias"] = b.astype(np.float32)
        pre, mag = pre + b[None, :], mag + np.abs(b)[None, :]
    if c.form == "acc":
        y0 = draw((n_out, c.F))
        out["y0"] = y0.astype(np.float32)
        pre, mag = pre + y0, mag + np.abs(y0)
    out["pre"] = pre
    out["want"] = (np.maximum(pre, 0) if c.form == "relu" else pre).astype(np.float64 if fl else np.float32)
    if fl:
        k = facts(c.op, c.t).deg.astype(np.float64)[:, None] + 2.0
        u = 2.0 ** -24
        out["bound"] = k * u / (1.0 - k * u) * mag
    if c.form == "adam":
        f = lambda: gen.standard_normal((n_out, c.F), dtype=np.float32)
        out["p"], out["m"] = f(), f()
        out["v"] = gen.random((n_out, c.F), dtype=np.float32) + np.float32(0.1)
        out["vmax"] = out["v"] * (np.float32(0.5) + gen.random((n_out, c.F), dtype=np.float32))
        out["grad"] = MX.astype(np.float32)
    return out


def operand_bytes(c):
    n_out, n_in = applied(c.op, c.t)[:2]
    L = layout(c)
    ws = workspace_floats(c)
    if ws is None:                              # column cuts: at most one slot more per column block and long row
        ws = (len(facts(c.op, c.t).long_rows) * 200 + sum(facts(c.op, c.t).seg_counts.values())) * (c.F + 3)
    return 4 * (n_in * max(L.ldx, L.ldx2) + n_out * (4 * L.ldp if c.form == "adam" else L.ldy) + ws + c.F)
