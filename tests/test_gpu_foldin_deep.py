"""Layer-chain fold-in on the GPU through the C ABI (csrc/foldin_layers.hip, `tgcn_foldin_layers`).

On guarded buffers (tests/_arena.py): every operand is a strided view into a pool of NaN -- the gaps of the combined table,
of W_l and of the biases included -- every result a view into a pool of a sentinel.
  * exact family -- dyadic operands (tests/_foldin_deep_cases.py): every layer's row and pred equal the float64 evaluation
    bit for bit; every leaf, table layout, output combination, batch size, both degree modes, columns outside the vocabulary.
  * float family -- every element within the derived forward-error bound of tests/_foldin_deep_ref.py:float_bounds:
    _foldin_ref's bound extended layer by layer.  Layer 1 is its `bu` (n FMAs, one FMA for a_dd s1, one add for b_1:
    gamma_{n+2} A^1).  Layer l >= 2 adds w_{l-1} + 2 roundings to the n of the gathered sum (w_{l-1} FMAs of x^{l-1} W_l, one
    FMA a_dd y + sum, one add of b_l): gamma_{n + w_{l-1} + 3} on the sum of the absolute values of its terms, evaluated on
    the COMPUTED x^{l-1}, whose own bound dx^{l-1} passes through a_dd |W_l|:
        |dx^l| <= gamma_{n + w_{l-1} + 3} (A^l + a_dd (dx^{l-1} |W_l|)) + a_dd (dx^{l-1} |W_l|).
    The ReLU is 1-Lipschitz.  Nothing in the bound is measured.
  * consistency with the flat kernel: at L = 2 with act_2 = none, out_1 / out_2 / pred are `tgcn_foldin_two_layer`'s hidden /
    logits / pred bit for bit on float operands, all of _foldin_cases.ROW_LENGTHS.
  * prefix property: the first l outputs of an L-layer call are the l-layer call's, bit for bit.
  * a document's results do not depend on the batch: alone, first and last among 2 * 16 * 512 + 1 short rows.
  * a shape over the LDS limit is refused with every sentinel in place."""
import numpy as np
import pytest
import torch

import _foldin_cases as fc
import _foldin_deep_cases as dc
import _foldin_deep_ref as DR
import _foldin_ref as R
from _arena import _Arena
from pytextgcn_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 0.15625
PRED_SENTINEL = -7
F32 = torch.float32


class _Pools:
    def __init__(self, dev):
        self.dev = dev
        self.nan = self.out = self.ints = None


@pytest.fixture(scope="module")
def pools(cuda):
    p = _Pools(cuda)
    yield p
    p.nan = p.out = p.ints = None
    dc.operands.cache_clear()
    dc.reference.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture
def lib(cuda):
    return _lib.load()


def _r4(v):
    return (v + 3) & ~3


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table_layout(widths, layout):
    """(t_col [L], ldt) of the combined table."""
    gap = 8 if layout == "padded" else 0
    order = list(range(len(widths)))
    if layout == "reversed":
        order.reverse()
    t_col, at = [0] * len(widths), 0
    for l in order:
        t_col[l] = at
        at += _r4(widths[l]) + gap
    return t_col, at + gap


def call_kernel(lib, pools, c, o):
    """One call of tgcn_foldin_layers on guarded, strided buffers; returns (status, [x per layer or None], pred or None,
    arenas)."""
    dev, B, V, L = pools.dev, c.n_docs, c.n_vocab, len(c.widths)
    pad = 8 if c.layout == "padded" else 0
    nnz = int(o["col"].size)
    t_col, ldt = table_layout(c.widths, c.layout)
    ins = _Arena(pools, "nan", F32)
    itab = ins.take(V, ldt, ldt, 0)
    iW, ib = [], []
    for l, w in enumerate(c.widths):
        iW.append(ins.take(c.widths[l - 1], w, _r4(w) + pad, 0) if l else None)
        ib.append(ins.take(1, w, _r4(w), 0))
    is1 = ins.take(1, c.widths[0], _r4(c.widths[0]), 0) if o["s1"] is not None else None
    idis, ival = ins.take(1, V, _r4(V), 0), ins.take(1, nnz, _r4(nnz), 0)
    ins.fill(float("nan"))
    tab = ins.view(itab)
    for l, (w, ly) in enumerate(zip(c.widths, o["layers"])):
        tab[:, t_col[l]:t_col[l] + w].copy_(_dev(ly["T"], dev))
        if l:
            ins.view(iW[l]).copy_(_dev(ly["W"], dev))
        ins.view(ib[l]).copy_(_dev(ly["b"], dev)[None, :])
    if is1 is not None:
        ins.view(is1).copy_(_dev(o["s1"], dev)[None, :])
    ins.view(idis).copy_(_dev(o["dis"], dev)[None, :])
    if nnz:
        ins.view(ival).copy_(_dev(o["val"], dev)[None, :])
    rowptr = _dev(o["rowptr"], dev)
    col = _dev(o["col"], dev) if nnz else torch.zeros(1, dtype=torch.int32, device=dev)

    outs = _Arena(pools, "out", F32)
    ints = _Arena(pools, "ints", torch.int32)
    io = [outs.take(B, w, _r4(w) + pad, 0) if on else None for w, on in zip(c.widths, c.outs)]
    ip = ints.take(1, B, _r4(B), 0) if c.pred else None
    outs.fill(SENTINEL)
    ints.fill(PRED_SENTINEL)
    ly = (_lib.FoldinLayer * L)()
    for l, w in enumerate(c.widths):
        ly[l] = _lib.FoldinLayer(ins.ptr(iW[l]) if l else None, _r4(w) + pad if l else 0, ins.ptr(ib[l]),
                                 outs.ptr(io[l]) if io[l] is not None else None, _r4(w) + pad, t_col[l], w, o["layers"][l]["act"], 0)
    st = lib.tgcn_foldin_layers(B, rowptr.data_ptr(), col.data_ptr(), ins.ptr(ival), V, ins.ptr(idis), _lib.DEGREE_SUMS[c.mode],
                                ins.ptr(itab), ldt, ins.ptr(is1) if is1 is not None else None, L, ly,
                                ints.ptr(ip) if ip is not None else None, None)
    torch.cuda.synchronize()
    xs = [outs.view(i).contiguous().cpu().numpy() if i is not None else None for i in io]
    pred = ints.view(ip).contiguous().cpu().numpy().reshape(-1) if ip is not None else None
    return st, xs, pred, (outs, ints)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), f"{what}: non-finite values (an operand gap or a guard row reached it)"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = bad[0]
        pytest.fail(f"{what} differs at {bad.shape[0]} of {got.size} elements in {np.unique(bad[:, 0]).size} rows, first "
                    f"[{r}, {k}]: {got[r, k]!r} != {want[r, k]!r}")


def _within(got, want, bound, what):
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    err = np.abs(got.astype(np.float64) - want)
    over = err > bound
    if over.any():
        r, k = np.argwhere(over)[0]
        pytest.fail(f"{what} beyond the forward-error bound at {int(over.sum())} elements, first [{r}, {k}]: error "
                    f"{err[r, k]:.3e}, bound {bound[r, k]:.3e}")


def run_case(lib, pools, c):
    o, ref = dc.operands(c), dc.reference(c)
    st, xs, pred, (outs, ints) = call_kernel(lib, pools, c, o)
    assert st == _lib.OK, (st, lib.tgcn_last_error().decode())
    if c.family == "int":
        assert ref["units"] < 2 ** 24, ref["units"]                    # the bound that makes fp32 exact, per case
        for l, (got, want) in enumerate(zip(xs, ref["layers"])):
            if got is not None:
                _same(got, want["x"].astype(np.float32), f"layer {l + 1}")
        if pred is not None:
            assert np.array_equal(pred, ref["pred"]), "pred is not the first arg-max of the exact last layer"
    else:
        for l, (got, want, bound) in enumerate(zip(xs, ref["layers"], ref["bounds"])):
            _within(got, want["x"], bound, f"layer {l + 1}")
        assert np.array_equal(pred, R.first_argmax(xs[-1])), "pred is not the first arg-max of the stored last layer"
    assert outs.untouched(), "a store outside the result views (gap columns / rows before or behind)"
    assert ints.untouched(), "a store outside pred"


def run_group(lib, pools, cases):
    failures = []
    for c in cases:
        try:
            run_case(lib, pools, c)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(f"{dc.case_id(c)} [{dc.leaf_of(c.widths)}]: {str(e)[:300]}")
    if failures:
        pytest.fail(f"{len(failures)} of {len(cases)} cases fail:\n" + "\n".join(failures), pytrace=False)


def _by_leaf(cases):
    return [[c for c in cases if dc.leaf_of(c.widths) == leaf] for leaf in dc.LEAVES]


@pytest.mark.parametrize("cases", _by_leaf(dc.int_cases()), ids=dc.LEAVES)
def test_foldin_layers_exact(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("cases", _by_leaf(dc.float_cases()), ids=dc.LEAVES)
def test_foldin_layers_float_within_the_derived_bound(lib, pools, cases):
    run_group(lib, pools, cases)


def test_a_shape_over_the_lds_limit_is_refused_with_every_sentinel_intact(lib, pools):
    c = dc._variant("int", 1, dc.OVER_THE_LIMIT, 3)
    st, xs, pred, (outs, ints) = call_kernel(lib, pools, c, dc.operands(c))
    assert st == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert str(DR.lds_bytes(dc.OVER_THE_LIMIT)) in msg and "LDS" in msg, msg
    assert all((x == SENTINEL).all() for x in xs) and (pred == PRED_SENTINEL).all()
    assert outs.untouched() and ints.untouched()


INVALID = [
    (dict(n_layers=5), "n_layers"), (dict(n_docs=-1), "bad size"), (dict(n_vocab=0), "bad size"), (dict(ldt=6), "bad size"),
    (dict(degree_sum=7), "degree_sum"), (dict(width=0), "bad size"), (dict(width=129), "bad size"), (dict(act=3), "unknown act"),
    (dict(t_col=2), "multiple of 4"), (dict(t_col=1 << 20), "inside a table row"), (dict(ldw=-4), "leading dimensions"),
    (dict(ldo=2), "leading dimensions"), (dict(rowptr=None), "NULL pointer"), (dict(table=None), "NULL pointer"),
    (dict(misalign_table=True), "16-byte aligned"), (dict(b=None), "NULL pointer"), (dict(W=None), "NULL pointer"),
    (dict(misalign_out=True), "16-byte aligned"),
]


@pytest.mark.parametrize("kw,word", INVALID, ids=[f"{list(k)[0]}-{i}" for i, (k, _) in enumerate(INVALID)])
def test_every_invalid_cause_returns_before_a_launch(lib, cuda, kw, word):
    """The cause is named in the error text and the output pool keeps its sentinel: nothing was enqueued."""
    B, V, widths = 5, 11, (8, 8, 8)
    tab = torch.zeros(V, 32, dtype=F32, device=cuda)
    W, b = torch.zeros(8, 8, dtype=F32, device=cuda), torch.zeros(8, dtype=F32, device=cuda)
    out = torch.full((3, B, 8), SENTINEL, dtype=F32, device=cuda)
    pred = torch.full((B,), PRED_SENTINEL, dtype=torch.int32, device=cuda)
    rowptr = torch.arange(B + 1, dtype=torch.int64, device=cuda)
    col, val = torch.zeros(B, dtype=torch.int32, device=cuda), torch.ones(B, dtype=F32, device=cuda)
    dis = torch.ones(V, dtype=F32, device=cuda)
    ly = (_lib.FoldinLayer * 3)()
    for l in range(3):
        f = dict(W=W.data_ptr() if l else None, ldw=8 if l else 0, b=b.data_ptr(), out=out[l].data_ptr(), ldo=8, t_col=8 * l,
                 width=8, act=0, reserved=0)
        if l == 1:
            f.update({k: v for k, v in kw.items() if k in f})
            if kw.get("misalign_out"):
                f["out"] += 4
        ly[l] = _lib.FoldinLayer(**f)
    a = dict(n_docs=B, rowptr=rowptr.data_ptr(), n_vocab=V, degree_sum=0, table=tab.data_ptr(), ldt=32, n_layers=3)
    a.update({k: v for k, v in kw.items() if k in a})
    if kw.get("misalign_table"):
        a["table"] += 4
    st = lib.tgcn_foldin_layers(a["n_docs"], a["rowptr"], col.data_ptr(), val.data_ptr(), a["n_vocab"], dis.data_ptr(),
                                a["degree_sum"], a["table"], a["ldt"], None, a["n_layers"], ly, pred.data_ptr(), None)
    torch.cuda.synchronize()
    assert st == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert "tgcn_foldin_layers" in msg and word in msg, msg
    assert bool((out == SENTINEL).all()) and bool((pred == PRED_SENTINEL).all())


# ---- consistency with the flat kernel -----------------------------------------------------------------------------------
def _plain(lib, dev, o, widths, mode, acts, want_pred=True):
    """tgcn_foldin_layers on plain, tight device tensors: ([x per layer], pred) as numpy."""
    L, B, V = len(widths), len(o["rowptr"]) - 1, o["layers"][0]["T"].shape[0]
    t_col, ldt = table_layout(widths, "tight")
    tab = torch.zeros(V, ldt, dtype=F32, device=dev)
    keep = []
    for l, w in enumerate(widths):
        tab[:, t_col[l]:t_col[l] + w] = _dev(o["layers"][l]["T"], dev)
    xs = [torch.full((B, _r4(w)), SENTINEL, dtype=F32, device=dev) for w in widths]
    pred = torch.full((max(B, 1),), PRED_SENTINEL, dtype=torch.int32, device=dev)
    ly = (_lib.FoldinLayer * L)()
    for l, w in enumerate(widths):
        Wt = None
        if l:
            Wt = torch.zeros(widths[l - 1], _r4(w), dtype=F32, device=dev)
            Wt[:, :w] = _dev(o["layers"][l]["W"], dev)
        bt = torch.zeros(_r4(w), dtype=F32, device=dev)
        bt[:w] = _dev(o["layers"][l]["b"], dev)
        keep += [Wt, bt]
        ly[l] = _lib.FoldinLayer(Wt.data_ptr() if l else None, _r4(w) if l else 0, bt.data_ptr(), xs[l].data_ptr(), _r4(w), t_col[l], w,
                                 acts[l], 0)
    s1 = None
    if o["s1"] is not None:
        s1 = torch.zeros(_r4(widths[0]), dtype=F32, device=dev)
        s1[:widths[0]] = _dev(o["s1"], dev)
    rp, cj, vj, dis = _dev(o["rowptr"], dev), _dev(o["col"], dev), _dev(o["val"], dev), _dev(o["dis"], dev)
    if cj.numel() == 0:
        cj, vj = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=F32, device=dev)
    st = lib.tgcn_foldin_layers(B, rp.data_ptr(), cj.data_ptr(), vj.data_ptr(), V, dis.data_ptr(), _lib.DEGREE_SUMS[mode],
                                tab.data_ptr(), ldt, s1.data_ptr() if s1 is not None else None, L, ly,
                                pred.data_ptr() if want_pred else None, None)
    torch.cuda.synchronize()
    assert st == _lib.OK, lib.tgcn_last_error().decode()
    return [x[:, :w].cpu().numpy() for x, w in zip(xs, widths)], pred[:B].cpu().numpy()


def _flat(lib, dev, o, mode):
    """tgcn_foldin_two_layer on the same operands (two layers); (z, u, pred) as numpy."""
    l1, l2 = o["layers"]
    h, C = l1["T"].shape[1], l2["T"].shape[1]
    B = len(o["rowptr"]) - 1

    def padded(a, w):
        t = torch.zeros(a.shape[0], _r4(w), dtype=F32, device=dev)
        t[:, :w] = _dev(a, dev)
        return t
    T1, P, W2 = padded(l1["T"], h), padded(l2["T"], C), padded(l2["W"], C)
    b1, b2 = padded(l1["b"][None, :], h), padded(l2["b"][None, :], C)
    s1t = padded(o["s1"][None, :], h) if o["s1"] is not None else None
    z = torch.full((B, _r4(C)), SENTINEL, dtype=F32, device=dev)
    u = torch.full((B, _r4(h)), SENTINEL, dtype=F32, device=dev)
    pred = torch.full((B,), PRED_SENTINEL, dtype=torch.int32, device=dev)
    rp, cj, vj, dis = _dev(o["rowptr"], dev), _dev(o["col"], dev), _dev(o["val"], dev), _dev(o["dis"], dev)
    st = lib.tgcn_foldin_two_layer(B, rp.data_ptr(), cj.data_ptr(), vj.data_ptr(), l1["T"].shape[0], dis.data_ptr(),
                                   _lib.DEGREE_SUMS[mode], T1.data_ptr(), _r4(h), h, s1t.data_ptr() if s1t is not None else None,
                                   b1.data_ptr(), l1["act"], P.data_ptr(), _r4(C), C, W2.data_ptr(), _r4(C), b2.data_ptr(),
                                   z.data_ptr(), _r4(C), pred.data_ptr(), u.data_ptr(), _r4(h), None)
    torch.cuda.synchronize()
    assert st == _lib.OK, lib.tgcn_last_error().decode()
    return z[:, :C].cpu().numpy(), u[:, :h].cpu().numpy(), pred.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("widths,s1,act1,mode", [((100, 64), False, 1, R.REFERENCE), ((63, 65), True, 0, R.ACCURATE),
                                                 ((256, 128), True, 1, R.REFERENCE), ((200, 5), False, 0, R.ACCURATE)],
                         ids=["vec-narrow", "tail-wide", "widest", "tail-narrow"])
def test_two_layers_are_the_flat_kernel_bit_for_bit(lib, pools, widths, s1, act1, mode):
    """Float operands, every row length of _foldin_cases.ROW_LENGTHS (the flat kernel skips out-of-range columns the same way)."""
    c = dc.Case("float", widths, dc.DOCS_PER_WORKGROUP + 1, 301, "tight", s1, (act1, 0), mode, (True, True), True, 61)
    assert dc.row_lengths(c)[:8] == list(fc.ROW_LENGTHS)
    o = dc.operands(c)
    xs, pred = _plain(lib, pools.dev, o, widths, mode, c.acts)
    z, u, pred_flat = _flat(lib, pools.dev, o, mode)
    assert np.isfinite(z).all() and np.isfinite(u).all()
    assert np.array_equal(_bits(xs[0]), _bits(u)), "out_1 differs from the flat kernel's hidden"
    assert np.array_equal(_bits(xs[1]), _bits(z)), "out_2 differs from the flat kernel's logits"
    assert np.array_equal(pred, pred_flat)


@pytest.mark.parametrize("widths", [(100, 100, 100, 100), (63, 5, 65, 7), (200, 128, 64, 4)], ids=["jkn", "tail", "mixed"])
def test_the_first_layers_of_a_deeper_call_are_the_shallower_call(lib, pools, widths):
    c = dc.Case("float", widths, dc.DOCS_PER_WORKGROUP + 1, 301, "tight", True, (1, 0, 1, 0), R.REFERENCE, (True,) * 4, True, 67)
    o = dc.operands(c)
    full, _ = _plain(lib, pools.dev, o, widths, c.mode, c.acts)
    for L in (2, 3):
        part, _ = _plain(lib, pools.dev, dict(o, layers=o["layers"][:L]), widths[:L], c.mode, c.acts[:L])
        for l in range(L):
            assert np.array_equal(_bits(part[l]), _bits(full[l])), (L, l)


def test_a_document_does_not_depend_on_its_batch(lib, pools):
    """Bit-equal rows alone, first and last in a batch of 2 * 16 * 512 + 1 short rows."""
    widths = (100, 70, 64, 5)
    base = dc.Case("float", widths, dc.DOCS_PER_WORKGROUP + 1, 301, "tight", True, (0, 1, 0, 0), R.REFERENCE, (True,) * 4, True, 91)
    o = dict(dc.operands(base))
    rp, probe = o["rowptr"], 6                                              # the 129-entry document
    mine = slice(int(rp[probe]), int(rp[probe + 1]))
    assert mine.stop - mine.start == 129
    n_other = 2 * dc.DOCS_PER_WORKGROUP * dc.WORKGROUP_CAP
    rng = np.random.default_rng(5)
    other_len = rng.integers(0, 3, size=n_other)
    other_col = rng.integers(0, base.n_vocab, size=int(other_len.sum())).astype(np.int32)
    other_val = (rng.random(other_col.size) * 0.9 + 0.05).astype(np.float32)

    def batch(pos):
        if pos is None:
            lens, col, val = [129], o["col"][mine], o["val"][mine]
        else:
            lens = list(other_len[:pos]) + [129] + list(other_len[pos:])
            cut = int(other_len[:pos].sum())
            col = np.concatenate([other_col[:cut], o["col"][mine], other_col[cut:]])
            val = np.concatenate([other_val[:cut], o["val"][mine], other_val[cut:]])
        ob = dict(o, rowptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col=col.astype(np.int32),
                  val=val.astype(np.float32))
        xs, pred = _plain(lib, pools.dev, ob, widths, base.mode, base.acts)
        at = 0 if pos is None else pos
        return [x[at].copy() for x in xs] + [pred[at:at + 1].astype(np.float32)]

    alone = batch(None)
    assert all(np.isfinite(a).all() for a in alone)
    for pos in (0, n_other):
        for a, b in zip(alone, batch(pos)):
            assert np.array_equal(_bits(a), _bits(b)), pos
