"""Case table and placement arithmetic of tests/test_gpu_extents_families.py: the kernel families added since
tests/test_gpu_extents.py, each with ONE 2-D operand of the call placed in a float32 pool so that its row offsets pass
2^31 bytes, 2^32 bytes, 2^31 elements and 2^32 elements.  Host arithmetic only: tests/test_extent_cases.py checks the
table on any machine, and against include/tgcn.h that no entry point with a leading dimension is left out.

The layout of a placed operand is `pool[MARGIN:].view(rows, ld)[:, :width]`, the pool full of NaN:
  * MARGIN = 2^31 elements lie in front of row 0, so an element index that wraps to a negative int, a byte offset that
    wraps either way as 32 bits and an unsigned index that wraps to a small value all stay INSIDE the pool: a wrong read
    returns NaN and a wrong write lands in a gap the test counts -- never outside the allocation;
  * ld is a multiple of 4 and MARGIN keeps the base 16-byte aligned: the alignment class of the compact run (whose
    operands are rows of width rounded up to 4 in a fresh allocation);
  * "tall" operands (the activations, logits and gradients, one row per node) take ld = 2^24 and 273 rows -- two 128-row
    tiles and a partial third, not a multiple of 4 (an operand tied to another one's shape may have a few rows fewer, never
    fewer than 257, so that a row starts in every window);
  * "short" operands (weights, embedding tables, weight gradients: 3 .. 63 rows) take the smallest ld, a multiple of 4, that
    puts the start of the last row at or past 2^32 elements;
  * "planes" is tgcn_jk_attention's h_fwd / h_bwd: L planes of `rows` rows, plane t at t * hstep, hstep = rows * ld >= 2^31
    so that (L - 1) * hstep itself passes 2^32 elements (the fixed ld = 2^24 would ask for 2^31 + 3 * 273 * 2^24 floats,
    59 GiB, against the 32 GiB every case has to fit in); both directions share ldh and hstep, so they sit side by side in the
    same rows.
Integer operands that index something (`cls`, `pred`) live in an int32 view of the same pool whose gaps hold GAP ids: valid
for the call, used by no real row, and pointing at a NaN row of the table (or a class nobody predicts)."""
import os
import re
from collections import namedtuple

GiB = 1 << 30
MARGIN = 1 << 31                     # elements in front of row 0
TALL_LD = 1 << 24
TALL_ROWS = 273
TALL_MIN_ROWS = 257                  # row 256 starts at 2^32 elements
SHORT_MAX_ROWS = 63
POOL_LIMIT_BYTES = 32 * GiB
WINDOWS = ("[2^31 B, 2^32 B)", "[2^32 B, 2^31 el)", "[2^31 el, 2^32 el)", ">= 2^32 el")

Placement = namedtuple("Placement", "kind rows width ld hstep planes pool_elems")


def _r4(v):
    return (v + 3) & ~3


def windows_hit(rows, ld):
    """the WINDOWS in which at least one row of the view starts (element offset r * ld from row 0)"""
    hit = set()
    for r in range(rows):
        el = r * ld
        if (1 << 31) <= 4 * el < (1 << 32):
            hit.add(WINDOWS[0])
        elif (1 << 32) <= 4 * el and el < (1 << 31):
            hit.add(WINDOWS[1])
        elif (1 << 31) <= el < (1 << 32):
            hit.add(WINDOWS[2])
        elif el >= (1 << 32):
            hit.add(WINDOWS[3])
    return tuple(w for w in WINDOWS if w in hit)


def place(kind, rows, width, planes=1):
    """The Placement of an operand, with the assertions that make its name true."""
    assert MARGIN >= (1 << 31) and MARGIN % 4 == 0
    assert width >= 1
    if kind == "tall":
        assert TALL_MIN_ROWS <= rows <= TALL_ROWS and planes == 1, (rows, planes)
        ld, hstep = TALL_LD, 0
        assert width <= ld and windows_hit(rows, ld) == WINDOWS, windows_hit(rows, ld)
        pool = MARGIN + rows * ld
    elif kind == "short":
        assert 3 <= rows <= SHORT_MAX_ROWS and planes == 1, (rows, planes)
        ld, hstep = _r4(-(-(1 << 32) // (rows - 1))), 0
        assert ld % 4 == 0 and (rows - 1) * ld >= (1 << 32) > (rows - 1) * (ld - 4) and width <= ld
        pool = MARGIN + rows * ld
    else:
        assert kind == "planes" and planes >= 2 and TALL_MIN_ROWS <= rows <= TALL_ROWS
        ld = _r4(-(-(1 << 31) // rows))
        hstep = rows * ld
        assert hstep >= (1 << 31) > rows * (ld - 4) and (planes - 1) * hstep >= (1 << 32) and width <= ld
        pool = MARGIN + (planes - 1) * hstep + (rows - 1) * ld + width        # (the last plane ends with its last row)
    assert ld % 4 == 0 and (4 * MARGIN) % 16 == 0
    assert 4 * pool <= POOL_LIMIT_BYTES, (kind, rows, width, 4 * pool / GiB)
    return Placement(kind, rows, width, ld, hstep, planes, pool)


# ----------------------------------------------------------------------------------------------------------------------
# the shapes (shared with the GPU tests, which build their operands from them)
# ----------------------------------------------------------------------------------------------------------------------
R = TALL_ROWS
BD = dict(h=12, widths=(7, 64, 100), starts=(0, 8, 72), n_cols=172)         # K = 3 members of unequal width
MCE = dict(K=3, C=7, S=8)                                                    # tgcn_member_ce: logits [R, 24]
CNT = dict(K=3, C=8)                                                         # class counts: class 7 is the gap id
EMB = dict(K=12, n=7)                                                        # tgcn_embed_xw*: E [12, R], W [12, 7]
EMBH = dict(K=12, n=100, Fh=5, h_row0=10)                                    # ..._h*: Hd [R - 10, 5]
EMBM = dict(M=3, K=4, n=64, Fh=5, h_row0=10)                                 # ..._members*: E [12, R], C [R, 192]
HIER = dict(N=265, Fh=8, h_row0=5, F=100)                                    # W [273, 100], Hd [260, 8]
MLP = dict(k=100, n=7)                                                       # Z [R, 100], W [7, 100]
MLPC = dict(k=100, n=7, S=2, Fh=6)                                           # cls [R, 2], T [6, 100]; id 5 is the gap id
MLPG = dict(k=20, n=(5, 7, 12), row_ptr=(0, 90, 200, R), w_rows=24, c_cols=24)
JKF = dict(L=3, C=5, H=7)                                                    # the fused forward: H = L C // 2
JKC = dict(H=25)                                                             # the cell: gates [R, 100]
JKA = dict(L=3, C=7, H=10)                                                   # attention and its backward
GCE = dict(widths=(7, 64, 100), n_cols=176)                               # _perlabel_ref.layout(widths, aligned=True)
ACT = dict(F=100)

Operand = namedtuple("Operand", "name params kind rows width io dtype planes")


def _op(name, params, kind, rows, width, io="in", dtype="f32", planes=1):
    return Operand(name, tuple(params.split()), kind, rows, width, io, dtype, planes)


def _tall(name, params, width, io="in", rows=R, dtype="f32"):
    return _op(name, params, "tall", rows, width, io, dtype)


def _short(name, params, rows, width, io="in"):
    return _op(name, params, "short", rows, width, io)


_bdK = len(BD["widths"])
_embh_rows = R - EMBH["h_row0"]
_jk_xs = lambda C: [_tall(f"xs{t}", "ldxs", C) for t in range(3)]

# entry point -> (dropout rates the case runs at, its placed operands).  `io`: "in", "out" (the view stays NaN before the call:
# the call writes every element), "inout" (the view starts as the compact operand does).
ENTRIES = {
    "tgcn_blockdiag_xw": ((0.0, 0.5), [
        _tall("X", "ldx", _bdK * BD["h"]), _short("W", "ldw", BD["h"], BD["n_cols"]), _tall("C", "ldc", BD["n_cols"], "out")]),
    "tgcn_blockdiag_xw_grad": ((0.0, 0.5), [
        _tall("X", "ldx", _bdK * BD["h"]), _short("W", "ldw", BD["h"], BD["n_cols"]), _tall("G", "ldg", BD["n_cols"]),
        _tall("dX", "lddx", _bdK * BD["h"], "out"), _short("dW", "lddw", BD["h"], BD["n_cols"], "out")]),
    "tgcn_member_ce": ((None,), [
        _tall("logits", "ld", MCE["K"] * MCE["S"]), _tall("dlogits", "ldd", MCE["K"] * MCE["S"], "out")]),
    "tgcn_class_counts_members": ((None,), [_tall("pred", "ldp", CNT["K"], dtype="i32")]),
    "tgcn_embed_xw": ((0.0, 0.5), [
        _short("E", "lde", EMB["K"], R), _short("W", "ldw", EMB["K"], EMB["n"]), _tall("C", "ldc", EMB["n"], "out")]),
    "tgcn_embed_xw_grad": ((0.0, 0.5), [
        _short("E", "lde", EMB["K"], R), _short("W", "ldw", EMB["K"], EMB["n"]), _tall("G", "ldg", EMB["n"]),
        _short("dE", "ldde", EMB["K"], R, "out"), _short("dW", "lddw", EMB["K"], EMB["n"], "out")]),
    "tgcn_embed_xw_h": ((0.0, 0.5), [
        _short("E", "lde", EMBH["K"], R), _short("Eh", "ldeh", EMBH["K"], EMBH["Fh"]),
        _tall("Hd", "ldh", EMBH["Fh"], rows=_embh_rows), _short("W", "ldw", EMBH["K"], EMBH["n"]),
        _tall("C", "ldc", EMBH["n"], "out")]),
    "tgcn_embed_xw_h_grad": ((0.0, 0.5), [
        _short("E", "lde", EMBH["K"], R), _short("Eh", "ldeh", EMBH["K"], EMBH["Fh"]),
        _tall("Hd", "ldh", EMBH["Fh"], rows=_embh_rows), _short("W", "ldw", EMBH["K"], EMBH["n"]),
        _tall("G", "ldg", EMBH["n"]), _short("dE", "ldde", EMBH["K"], R, "out"),
        _short("dEh", "lddeh", EMBH["K"], EMBH["Fh"], "out"), _short("dW", "lddw", EMBH["K"], EMBH["n"], "out")]),
    "tgcn_embed_xw_members": ((0.0, 0.5), [
        _short("E", "lde", EMBM["M"] * EMBM["K"], R), _short("Eh", "ldeh", EMBM["M"] * EMBM["K"], EMBM["Fh"]),
        _tall("Hd", "ldh", EMBM["Fh"], rows=R - EMBM["h_row0"]), _short("W", "ldw", EMBM["M"] * EMBM["K"], EMBM["n"]),
        _tall("C", "ldc", EMBM["M"] * EMBM["n"], "out")]),
    "tgcn_embed_xw_members_grad": ((0.0, 0.5), [
        _short("E", "lde", EMBM["M"] * EMBM["K"], R), _short("Eh", "ldeh", EMBM["M"] * EMBM["K"], EMBM["Fh"]),
        _tall("Hd", "ldh", EMBM["Fh"], rows=R - EMBM["h_row0"]), _short("W", "ldw", EMBM["M"] * EMBM["K"], EMBM["n"]),
        _tall("G", "ldg", EMBM["M"] * EMBM["n"]), _short("dE", "ldde", EMBM["M"] * EMBM["K"], R, "out"),
        _short("dEh", "lddeh", EMBM["M"] * EMBM["K"], EMBM["Fh"], "out"),
        _short("dW", "lddw", EMBM["M"] * EMBM["K"], EMBM["n"], "out")]),
    "tgcn_hier_xw": ((None,), [
        _tall("W", "ldw", HIER["F"], rows=HIER["N"] + HIER["Fh"]),
        _tall("Hd", "ldh", HIER["Fh"], rows=HIER["N"] - HIER["h_row0"]), _tall("C", "ldc", HIER["F"], "out", rows=HIER["N"])]),
    "tgcn_hier_xw_grad": ((None,), [
        _tall("G", "ldg", HIER["F"], rows=HIER["N"]), _tall("dW", "lddw", HIER["F"], "out", rows=HIER["N"] + HIER["Fh"])]),
    "tgcn_mlp_act_linear": ((0.0, 0.5), [
        _tall("Z", "ldz", MLP["k"]), _short("W", "ldw", MLP["n"], MLP["k"]), _tall("C", "ldc", MLP["n"], "out")]),
    "tgcn_mlp_act_linear_grad": ((0.0, 0.5), [
        _tall("Z", "ldz", MLP["k"]), _short("W", "ldw", MLP["n"], MLP["k"]), _tall("G", "ldg", MLP["n"]),
        _tall("dZ", "lddz", MLP["k"], "out"), _short("dW", "lddw", MLP["n"], MLP["k"], "out")]),
    "tgcn_mlp_act_linear_cls": ((0.0, 0.5), [
        _tall("Z", "ldz", MLPC["k"]), _tall("cls", "ldcls", MLPC["S"], dtype="i32"), _short("T", "ldt", MLPC["Fh"], MLPC["k"]),
        _short("W", "ldw", MLPC["n"], MLPC["k"]), _tall("C", "ldc", MLPC["n"], "out")]),
    "tgcn_mlp_act_linear_cls_grad": ((0.0, 0.5), [
        _tall("Z", "ldz", MLPC["k"]), _tall("cls", "ldcls", MLPC["S"], dtype="i32"), _short("T", "ldt", MLPC["Fh"], MLPC["k"]),
        _short("W", "ldw", MLPC["n"], MLPC["k"]), _tall("G", "ldg", MLPC["n"]), _tall("dZ", "lddz", MLPC["k"], "out"),
        _short("dT", "lddt", MLPC["Fh"], MLPC["k"], "out"), _short("dW", "lddw", MLPC["n"], MLPC["k"], "out")]),
    # a row of the grouped C holds its own group's columns only; the others keep what they held: "inout"
    "tgcn_mlp_grouped_act_linear": ((0.0, 0.5), [
        _tall("Z", "ldz", MLPG["k"]), _short("W", "ldw", MLPG["w_rows"], MLPG["k"]), _tall("C", "ldc", MLPG["c_cols"], "inout")]),
    "tgcn_mlp_grouped_act_linear_grad": ((0.0, 0.5), [
        _tall("Z", "ldz", MLPG["k"]), _short("W", "ldw", MLPG["w_rows"], MLPG["k"]), _tall("G", "ldg", MLPG["c_cols"]),
        _tall("dZ", "lddz", MLPG["k"], "out"), _short("dW", "lddw", MLPG["w_rows"], MLPG["k"], "out")]),
    # ldwi / ldwh are shared by the two directions: their weights are placed as one stack of 8 H rows
    "tgcn_jk_lstm_forward": ((None,), _jk_xs(JKF["C"]) + [
        _short("Wih", "ldwi", 8 * JKF["H"], JKF["C"]), _short("Whh", "ldwh", 8 * JKF["H"], JKF["H"]),
        _tall("out", "ldo", JKF["C"], "out"), _tall("alpha", "lda", JKF["L"], "out")]),
    "tgcn_jk_cell": ((None,), [
        _tall("pre_x", "ldpx", 4 * JKC["H"]), _tall("pre_h", "ldph", 4 * JKC["H"]), _tall("c_prev", "ldcp", JKC["H"]),
        _tall("gates", "ldg", 4 * JKC["H"], "out"), _tall("c", "ldc", JKC["H"], "out"), _tall("h", "ldh", JKC["H"], "out")]),
    "tgcn_jk_attention": ((None,), _jk_xs(JKA["C"]) + [
        _op("h", "ldh hstep", "planes", R, _r4(JKA["H"]) + JKA["H"], planes=JKA["L"]),
        _tall("out", "ldo", JKA["C"], "out"), _tall("alpha", "lda", JKA["L"], "out")]),
    "tgcn_jk_attention_grad": ((None,), _jk_xs(JKA["C"]) + [
        _tall("G", "ldg", JKA["C"]), _tall("out", "ldo", JKA["C"]), _tall("alpha", "lda", JKA["L"]),
        _tall("dscore", "ldds", JKA["L"], "out")]),
    "tgcn_jk_cell_grad": ((None,), [
        _tall("gates", "ldg", 4 * JKC["H"]), _tall("c", "ldc", JKC["H"]), _tall("c_prev", "ldcp", JKC["H"]),
        _tall("dh_rec", "lddh", JKC["H"]), _tall("dscore_t", "ldds", 1), _tall("dc", "lddc", JKC["H"], "inout"),
        _tall("dgates", "lddg", 4 * JKC["H"], "out")]),
    "tgcn_jk_input_grad": ((None,), [
        _tall("dx", "lddx", JKA["C"], "out"), _tall("T", "ldt", JKA["C"]), _tall("G", "ldg", JKA["C"]),
        _tall("out", "ldo", JKA["C"]), _tall("alpha_t", "lda", 1)]),
    "tgcn_grouped_ce": ((None,), [_tall("logits", "ld", GCE["n_cols"]), _tall("dlogits", "ldd", GCE["n_cols"], "out")]),
    "tgcn_act_grad": ((None,), [_tall("A", "lda", ACT["F"]), _tall("G", "ldg", ACT["F"], "inout")]),
}

Case = namedtuple("Case", "entry operand p")
CASES = [Case(entry, op.name, p) for entry, (rates, ops) in ENTRIES.items() for op in ops for p in rates]


def case_id(c):
    return f"{c.entry[5:]}-{c.operand}" + ("" if c.p is None else f"-p{c.p}")


def operand(entry, name):
    return next(op for op in ENTRIES[entry][1] if op.name == name)


def placement_of(op):
    return place(op.kind, op.rows, op.width, op.planes)


def pool_elems():
    """the pool every case fits in"""
    return max(placement_of(op).pool_elems for _, ops in ENTRIES.values() for op in ops)


# ----------------------------------------------------------------------------------------------------------------------
# entry points that take a leading dimension and are NOT placed here, each with its reason
# ----------------------------------------------------------------------------------------------------------------------
_THERE = "placed past 2^31 bytes, 4 GiB and 2^31 elements by tests/test_gpu_extents.py"
_FOLDIN = ("its large operands are gathered tables whose leading dimension is capped at 2^31 - 1 and whose sizes are far from "
           "2^31 elements in every configuration: a follow-up")
EXEMPT = {
    **{e: "the SpMM family: " + _THERE for e in (
        "tgcn_spmm", "tgcn_spmm_split", "tgcn_spmm_acc", "tgcn_spmm_act", "tgcn_spmm_adam", "tgcn_spmm_adam_split")},
    **{e: "the dense products: " + _THERE for e in (
        "tgcn_gemm_nn", "tgcn_gemm_nt", "tgcn_gemm_tn", "tgcn_gemm_nn_dropout", "tgcn_gemm_nt_dropout", "tgcn_gemm_tn_dropout",
        "tgcn_gemm_nn_dropout_mask", "tgcn_gemm_tn_dropout_mask", "tgcn_gemm_nt_colsum_mask", "tgcn_gemm_nt_colsum")},
    **{e: "the row movement: " + _THERE for e in ("tgcn_rows_gather", "tgcn_rows_scatter", "tgcn_rows_reduce_ranked")},
    **{e: "the flat loss and the column sums: " + _THERE for e in (
        "tgcn_colsum", "tgcn_masked_ce", "tgcn_masked_ce_pred", "tgcn_masked_ce_grad")},
    **{e: "fold-in: " + _FOLDIN for e in (
        "tgcn_foldin_two_layer", "tgcn_foldin_levels", "tgcn_foldin_routed", "tgcn_foldin_layers")},
}

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tgcn.h")


def declared_leading_dimensions(text=None):
    """{entry point: [its `int64_t ld*` / `hstep` parameters]} of include/tgcn.h (`const int64_t *ldxs`, the host array of
    leading dimensions of the JK inputs, counts too); entry points without one are left out."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(tgcn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = re.findall(r"\bint64_t\s*\*?\s*(ld[a-z0-9_]*|hstep)\b", args)
        if params:
            out[name] = params
    return out


def uncovered(entries=None, exempt=None, declared=None):
    """the (entry point, parameter) pairs of the header that no case places and no exemption names"""
    entries = ENTRIES if entries is None else entries
    exempt = EXEMPT if exempt is None else exempt
    declared = declared_leading_dimensions() if declared is None else declared
    missing = []
    for entry, params in declared.items():
        if entry in exempt:
            continue
        placed = {p for op in entries.get(entry, ((), []))[1] for p in op.params}
        missing += [(entry, p) for p in params if p not in placed]
    return missing
