"""Per-level fold-in on the GPU (csrc/foldin_levels.hip, pytextgcn_amd/inductive.py `FoldInLevels`).

Through the C ABI, on guarded buffers (tests/_arena.py): every operand is a strided view into a pool of NaN -- the gaps of
the combined table, of W2, Wh and the biases included -- every result a view into a pool of a sentinel.
  * exact family -- dyadic operands, link = one_hot (tests/_foldin_levels_cases.py): every level's logits, hidden, pred and
    link rows equal the float64 evaluation bit for bit; every leaf, table layout, output combination, batch size; a shape over
    the LDS limit is refused with every sentinel in place.
  * consistency with the flat kernel: level 1 bit-equal to `tgcn_foldin_two_layer` on the same tables; with link = one_hot
    level l >= 2 equal to `tgcn_foldin_two_layer` on the documents grouped by their arg-max one level up, s1 = Wh[k].
  * float family, link = softmax somewhere, in two parts so that no undocumented expf error enters a bound:
      (i)  a link row against the float64 softmax of the kernel's OWN previous-level fp32 logits, `row_rel_err` < TOL, the
           project's bar for the cross-entropy kernels (tests/test_gpu_parity.py);
      (ii) a level's hidden and logits against the float64 evaluation that takes the kernel's OWN fp32 link rows as p, every
           element within the forward-error bound of tests/_foldin_levels_ref.py:float_bounds -- _foldin_ref's bound with
           C_{l-1} more FMAs for s^l, passed through a_dd: |du| <= gamma_{n + C_{l-1} + 2} U.
  * a document's results do not depend on the batch; HIP-graph capture.
At module level: `FoldInLevels` against the CPU oracle run level by level on `extended_graph(..., hierarchy=softmax)`."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import _foldin_levels_cases as lc
import _foldin_levels_ref as LR
import _foldin_ref as R
from _arena import _Arena
from oracle import gcn_oracle as O
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, synth
from pytextgcn_amd.inductive import FoldIn, FoldInLevels, enable_fused_foldin, extended_graph
from pytextgcn_amd.perlevel import one_hot_hierarchy, with_hierarchy
from test_gpu_parity import TOL, row_rel_err

pytestmark = pytest.mark.gpu

SENTINEL = 0.15625
PRED_SENTINEL = -7
PARITY = 1e-5
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
    lc.operands.cache_clear()
    lc.reference.cache_clear()
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
    """(t1_col [L], p_col [L], ldt) of the combined table."""
    gap = 8 if layout == "padded" else 0
    segs = [("t", l, _r4(h)) for l, (h, _) in enumerate(widths)] + [("p", l, _r4(C)) for l, (_, C) in enumerate(widths)]
    if layout == "reversed":
        segs = [s for s in reversed(segs)]                      # P segments first, the levels from the last to the first
    else:
        segs = sorted(segs, key=lambda s: (s[1], s[0] == "p"))   # T1^1 P^1 T1^2 P^2 ...
    t1, p, at = [0] * len(widths), [0] * len(widths), 0
    for kind, l, w in segs:
        (t1 if kind == "t" else p)[l] = at
        at += w + gap
    return t1, p, at + gap


def call_kernel(lib, pools, c, o):
    """One call of tgcn_foldin_levels on guarded, strided buffers; returns (status, per-level dicts of numpy results, arenas)."""
    dev, B, V, L = pools.dev, c.n_docs, c.n_vocab, len(c.widths)
    pad = 8 if c.layout == "padded" else 0
    nnz = int(o["col"].size)
    t1_col, p_col, ldt = table_layout(c.widths, c.layout)
    ins = _Arena(pools, "nan", F32)
    itab = ins.take(V, ldt, ldt, 0)
    iW, iWh, ib1, ib2 = [], [], [], []
    for l, (h, C) in enumerate(c.widths):
        iW.append(ins.take(h, C, _r4(C) + pad, 0))
        iWh.append(ins.take(c.widths[l - 1][1], h, _r4(h) + pad, 0) if l else None)
        ib1.append(ins.take(1, h, _r4(h), 0))
        ib2.append(ins.take(1, C, _r4(C), 0))
    idis, ival = ins.take(1, V, _r4(V), 0), ins.take(1, nnz, _r4(nnz), 0)
    ins.fill(float("nan"))
    tab = ins.view(itab)
    for l, ((h, C), lv) in enumerate(zip(c.widths, o["levels"])):
        tab[:, t1_col[l]:t1_col[l] + h].copy_(_dev(lv["T1"], dev))
        tab[:, p_col[l]:p_col[l] + C].copy_(_dev(lv["P"], dev))
        ins.view(iW[l]).copy_(_dev(lv["W2"], dev))
        if l:
            ins.view(iWh[l]).copy_(_dev(lv["Wh"], dev))
        ins.view(ib1[l]).copy_(_dev(lv["b1"], dev)[None, :])
        ins.view(ib2[l]).copy_(_dev(lv["b2"], dev)[None, :])
    ins.view(idis).copy_(_dev(o["dis"], dev)[None, :])
    if nnz:
        ins.view(ival).copy_(_dev(o["val"], dev)[None, :])
    rowptr = _dev(o["rowptr"], dev)
    col = _dev(o["col"], dev) if nnz else torch.zeros(1, dtype=torch.int32, device=dev)

    outs = _Arena(pools, "out", F32)
    ints = _Arena(pools, "ints", torch.int32)
    want = {k: k in c.outs for k in lc.OUTS}
    iz, ih, ik, ip = [], [], [], []
    for l, (h, C) in enumerate(c.widths):
        Cp = c.widths[l - 1][1] if l else 0
        iz.append(outs.take(B, C, _r4(C) + pad, 0) if want["logits"] else None)
        ih.append(outs.take(B, h, _r4(h) + pad, 0) if want["hidden"] else None)
        ik.append(outs.take(B, Cp, _r4(Cp) + pad, 0) if (want["link"] and l) else None)
        ip.append(ints.take(1, B, _r4(B), 0) if want["pred"] else None)
    outs.fill(SENTINEL)
    ints.fill(PRED_SENTINEL)

    def optr(arena, i):
        return arena.ptr(i) if i is not None else None
    lv = (_lib.FoldinLevel * L)()
    for l, (h, C) in enumerate(c.widths):
        Cp = c.widths[l - 1][1] if l else 0
        lv[l] = _lib.FoldinLevel(t1_col[l], p_col[l], ins.ptr(iW[l]), _r4(C) + pad, ins.ptr(iWh[l]) if l else None,
                                 _r4(h) + pad if l else 0, ins.ptr(ib1[l]), ins.ptr(ib2[l]), optr(outs, iz[l]), _r4(C) + pad,
                                 optr(ints, ip[l]), optr(outs, ih[l]), _r4(h) + pad, optr(outs, ik[l]), _r4(Cp) + pad if l else 0,
                                 h, C, c.acts[l], LR.LINK_ID[c.links[l]] if l else 0)
    st = lib.tgcn_foldin_levels(B, rowptr.data_ptr(), col.data_ptr(), ins.ptr(ival), V, ins.ptr(idis), _lib.DEGREE_SUMS[c.mode],
                                ins.ptr(itab), ldt, L, lv, None)
    torch.cuda.synchronize()

    def host(arena, i):
        return arena.view(i).contiguous().cpu().numpy() if i is not None else None
    res = [dict(z=host(outs, iz[l]), u=host(outs, ih[l]), p=host(outs, ik[l]),
                pred=host(ints, ip[l]).reshape(-1) if ip[l] is not None else None) for l in range(L)]
    return st, res, (outs, ints)


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
    o = lc.operands(c)
    st, res, (outs, ints) = call_kernel(lib, pools, c, o)
    assert st == _lib.OK, (st, lib.tgcn_last_error().decode())
    if c.family == "int":
        ref = lc.reference(c)
        assert ref["units"] < 2 ** 24, ref["units"]                    # the bound that makes fp32 exact, per case
        for l, (got, want) in enumerate(zip(res, ref["levels"])):
            if got["z"] is not None:
                _same(got["z"], want["z"].astype(np.float32), f"level {l + 1} logits")
            if got["u"] is not None:
                _same(got["u"], want["u"].astype(np.float32), f"level {l + 1} hidden")
            if got["p"] is not None:
                _same(got["p"], want["p"], f"level {l + 1} link")
            if got["pred"] is not None:
                assert np.array_equal(got["pred"], want["pred"]), f"level {l + 1} pred is not the first arg-max of the exact logits"
    else:
        # (i) the link rows against the kernel's own logits one level up
        for l in range(1, len(res)):
            z_up, p = res[l - 1]["z"], res[l]["p"]
            assert np.isfinite(p).all()
            if c.links[l] == LR.SOFTMAX:
                want = LR.softmax_rows(z_up, np.float64)
                e = row_rel_err(torch.from_numpy(p), torch.from_numpy(want))
                assert e < TOL, f"level {l + 1} link rows: {e:.3e} from the float64 softmax of the kernel's own logits"
            else:
                assert np.array_equal(p, LR.one_hot_rows(z_up)), f"level {l + 1}: not the one-hot of the first arg-max"
        # (ii) every level against float64 on the kernel's own link rows
        ref = LR.foldin_levels(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["levels"], np.float64,
                               links_given=[r["p"] for r in res[1:]], want_abs=True)
        for l, (got, want, lv) in enumerate(zip(res, ref, o["levels"])):
            bu, bz = LR.float_bounds(o["rowptr"], want, lv)
            _within(got["u"], want["u"], bu, f"level {l + 1} hidden")
            _within(got["z"], want["z"], bz, f"level {l + 1} logits")
            assert np.array_equal(got["pred"], R.first_argmax(got["z"])), f"level {l + 1} pred"
    assert outs.untouched(), "a store outside the result views (gap columns / rows before or behind)"
    assert ints.untouched(), "a store outside pred"


def run_group(lib, pools, cases):
    failures = []
    for c in cases:
        try:
            run_case(lib, pools, c)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(f"{lc.case_id(c)} [{lc.leaf_of(c.widths)}]: {str(e)[:300]}")
    if failures:
        pytest.fail(f"{len(failures)} of {len(cases)} cases fail:\n" + "\n".join(failures), pytrace=False)


def _by_leaf(cases):
    return [[c for c in cases if lc.leaf_of(c.widths) == leaf] for leaf in lc.LEAVES]


@pytest.mark.parametrize("cases", _by_leaf(lc.int_cases()), ids=lc.LEAVES)
def test_foldin_levels_exact(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("cases", _by_leaf(lc.float_cases()), ids=lc.LEAVES)
def test_foldin_levels_float_link_and_forward_error_bound(lib, pools, cases):
    run_group(lib, pools, cases)


def test_a_shape_over_the_lds_limit_is_refused_with_every_sentinel_intact(lib, pools):
    c = lc._variant("int", 1, lc.OVER_THE_LIMIT, 3)._replace(outs=lc.OUTS)
    st, res, (outs, ints) = call_kernel(lib, pools, c, lc.operands(c))
    assert st == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert str(LR.lds_bytes(*zip(*lc.OVER_THE_LIMIT))) in msg and "LDS" in msg, msg
    for r in res:
        assert (r["z"] == SENTINEL).all() and (r["u"] == SENTINEL).all() and (r["pred"] == PRED_SENTINEL).all()
    assert outs.untouched() and ints.untouched()


# ---- consistency with the flat kernel -----------------------------------------------------------------------------------
def _flat(lib, dev, o, lv, mode, rowptr, col, val, s1):
    """tgcn_foldin_two_layer on plain device tensors; (z, u, pred) as numpy."""
    h, C = lv["T1"].shape[1], lv["P"].shape[1]
    B = len(rowptr) - 1

    def padded(a, w):
        t = torch.zeros(a.shape[0], _r4(w), dtype=F32, device=dev)
        t[:, :w] = _dev(a, dev)
        return t
    T1, P, W2 = padded(lv["T1"], h), padded(lv["P"], C), padded(lv["W2"], C)
    b1, b2 = padded(lv["b1"][None, :], h), padded(lv["b2"][None, :], C)
    s1t = padded(np.asarray(s1, dtype=np.float32)[None, :], h) if s1 is not None else None
    z = torch.full((B, _r4(C)), SENTINEL, dtype=F32, device=dev)
    u = torch.full((B, _r4(h)), SENTINEL, dtype=F32, device=dev)
    pred = torch.full((B,), PRED_SENTINEL, dtype=torch.int32, device=dev)
    rp, cj, vj, dis = _dev(rowptr, dev), _dev(col, dev), _dev(val, dev), _dev(o["dis"], dev)
    if cj.numel() == 0:
        cj, vj = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=F32, device=dev)
    st = lib.tgcn_foldin_two_layer(B, rp.data_ptr(), cj.data_ptr(), vj.data_ptr(), lv["T1"].shape[0], dis.data_ptr(),
                                   _lib.DEGREE_SUMS[mode], T1.data_ptr(), _r4(h), h, s1t.data_ptr() if s1t is not None else None,
                                   b1.data_ptr(), lv["act"], P.data_ptr(), _r4(C), C, W2.data_ptr(), _r4(C), b2.data_ptr(),
                                   z.data_ptr(), _r4(C), pred.data_ptr(), u.data_ptr(), _r4(h), None)
    torch.cuda.synchronize()
    assert st == _lib.OK, lib.tgcn_last_error().decode()
    return z[:, :C].cpu().numpy(), u[:, :h].cpu().numpy(), pred.cpu().numpy()


@pytest.mark.parametrize("widths", [((100, 6), (100, 64)), ((63, 63), (64, 65)), ((100, 9), (100, 70), (100, 128))],
                         ids=["amazon", "tail-wide", "three-levels"])
def test_levels_agree_with_the_flat_kernel(lib, pools, widths):
    """Random operands (the flat kernel skips the out-of-range columns the same way).  Level 1: bit for bit.  Level l >= 2 under one_hot: the flat kernel on the documents of each arg-max class k with s1 = Wh[k], equal by
    value (`==`: the same operations in the same order; only the sign of a zero may differ)."""
    L = len(widths)
    c = lc.Case("float", widths, lc.DOCS_PER_WORKGROUP + 1, 301, "tight", (1, 0, 1)[:L], (None,) + (LR.ONE_HOT,) * (L - 1),
                R.ACCURATE if L == 3 else R.REFERENCE, lc.OUTS, 77)
    o = lc.operands(c)
    st, res, _ = call_kernel(lib, pools, c, o)
    assert st == _lib.OK
    z, u, pred = _flat(lib, pools.dev, o, o["levels"][0], c.mode, o["rowptr"], o["col"], o["val"], None)
    for name, got, want in (("logits", res[0]["z"], z), ("hidden", res[0]["u"], u)):
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"level 1 {name} differs from the flat kernel's bits"
    assert np.array_equal(res[0]["pred"], pred)
    rp = o["rowptr"]
    for l in range(1, L):
        ks = res[l - 1]["pred"]
        assert np.array_equal(res[l]["p"], LR.one_hot_rows(res[l - 1]["z"]))
        for k in np.unique(ks):
            docs = np.nonzero(ks == k)[0]
            lens = np.diff(rp)[docs]
            sel = np.concatenate([np.arange(rp[d], rp[d + 1]) for d in docs]).astype(np.int64) if lens.sum() else np.zeros(0, dtype=np.int64)
            sub_rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            z, u, pred = _flat(lib, pools.dev, o, o["levels"][l], c.mode, sub_rp, o["col"][sel], o["val"][sel],
                               o["levels"][l]["Wh"][k])
            assert (res[l]["z"][docs] == z).all() and (res[l]["u"][docs] == u).all(), (l, k)
            assert np.array_equal(res[l]["pred"][docs], pred), (l, k)


def test_a_document_does_not_depend_on_its_batch(lib, pools):
    """Bit-equal logits, hidden and link rows alone, first, last and in the middle of a batch of 300 other documents."""
    widths = ((100, 9), (100, 70), (64, 128))
    base = lc.Case("float", widths, lc.DOCS_PER_WORKGROUP + 1, 301, "padded", (0, 1, 0), (None, LR.SOFTMAX, LR.SOFTMAX),
                   R.REFERENCE, lc.OUTS, 91)
    o = dict(lc.operands(base))
    rp, probe = o["rowptr"], 6                                              # the 129-entry document
    mine = slice(int(rp[probe]), int(rp[probe + 1]))
    rng = np.random.default_rng(5)
    other_len = rng.integers(0, 40, size=299)
    other_col = rng.integers(0, base.n_vocab, size=int(other_len.sum())).astype(np.int32)
    other_val = (rng.random(other_col.size) * 0.9 + 0.05).astype(np.float32)

    def batch(pos):
        lens = [mine.stop - mine.start] if pos is None else list(other_len[:pos]) + [mine.stop - mine.start] + list(other_len[pos:])
        cut = 0 if pos is None else int(other_len[:pos].sum())
        col = np.concatenate([other_col[:cut], o["col"][mine], other_col[cut:]]) if pos is not None else o["col"][mine]
        val = np.concatenate([other_val[:cut], o["val"][mine], other_val[cut:]]) if pos is not None else o["val"][mine]
        ob = dict(o, rowptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col=col.astype(np.int32),
                  val=val.astype(np.float32))
        st, res, _ = call_kernel(lib, pools, base._replace(n_docs=len(lens)), ob)
        assert st == _lib.OK
        at = 0 if pos is None else pos
        return [r[k][at].copy() for r in res for k in ("z", "u", "p") if r[k] is not None]

    alone = batch(None)
    assert all(np.isfinite(a).all() for a in alone)
    for pos in (0, 299, 150):
        for a, b in zip(alone, batch(pos)):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), pos


# ---- module level --------------------------------------------------------------------------------------------------------
N_HOLD, C1, C2, C3 = 150, 7, 12, 5


@pytest.fixture(scope="module")
def corpus(cuda):
    full = synth.word_doc_graph(2150, 60000, seed=7, device=cuda, n_classes=C1, vocab_frac=0.28)
    g, tfidf, _ = synth.hold_out_documents(full, N_HOLD)
    V, N = int(g.n_vocab), g.x.size(0)
    y = g.y[V:]
    g2 = with_hierarchy(g, one_hot_hierarchy(g, y, C1))
    g3 = with_hierarchy(g, one_hot_hierarchy(g, (y * 5 + 1) % C2, C2))
    return g, g2, g3, tfidf


def _bias_noise(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return model


def _models(g, dev, relu, levels=2):
    N = g.x.size(0)
    torch.manual_seed(11)
    dims = [(N, C1, 100), (N + C1, C2, 64), (N + C2, C3, 36)][:levels]
    return [_bias_noise(pkg.GCN(i, o, n_hidden_gcn=h, dropout=0.5, apply_activation=relu).to(dev).float(), 13 + k).eval()
            for k, (i, o, h) in enumerate(dims)]


def _cpu_graph(g):
    out = copy.copy(g)
    out.x = g.x.to_sparse().cpu() if isinstance(g.x, pkg.HierarchyFeatures) else g.x.cpu()
    for k in ("edge_index", "edge_attr", "y", "train_mask", "val_mask", "test_mask"):
        setattr(out, k, getattr(g, k).cpu())
    return out


def _oracle_levels(models, graphs, tfidf, relu):
    """The CPU oracle level by level: (new rows' logits per level, softmax rows handed down, old rows unchanged)."""
    zs, links, H_new = [], [], None
    for model, g in zip(models, graphs):
        gc = _cpu_graph(g)
        N = gc.x.size(0)
        state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref = O.GCNOracle(gc.x.size(1), state["layers.1.bias"].numel(), n_hidden_gcn=state["layers.0.bias"].numel())
        ref.load_state_dict(state)
        with torch.no_grad():
            ext = R.gcn_forward(ref.eval(), extended_graph(gc, tfidf, hierarchy=H_new), relu)[0]
            base = R.gcn_forward(ref, gc, relu)[0]
        assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))        # the exactness claim: old rows as they were
        zs.append(ext[N:].numpy())
        H_new = torch.softmax(ext[N:], dim=1)
        links.append(H_new.numpy())
    return zs, links[:-1]


@pytest.mark.parametrize("relu,levels", [(False, 2), (True, 2), (True, 3)], ids=["linear", "relu", "relu-three-levels"])
def test_foldin_levels_matches_the_oracle_on_the_extended_graphs(cuda, corpus, relu, levels):
    g, g2, g3, tfidf = corpus
    graphs = [g, g2, g3][:levels]
    models = _models(g, cuda, relu, levels)
    fold = FoldInLevels(models, graphs)
    z = fold.logits(tfidf)
    want, want_links = _oracle_levels(models, graphs, tfidf, relu)
    assert [tuple(t.shape) for t in z] == [(N_HOLD, c) for c in (C1, C2, C3)[:levels]]
    for l, (a, b) in enumerate(zip(z, want)):
        e = R.rel_err(a.cpu().numpy(), b)
        print(f"FoldInLevels level {l + 1} against the oracle on the extended graph: {e:.3e}")
        assert e < PARITY, (l, e)
    for a, b in zip(fold.probabilities(tfidf), want_links):
        assert R.rel_err(a.cpu().numpy(), b) < PARITY
    pred = fold.predict(tfidf)
    assert pred.dtype == torch.int64 and tuple(pred.shape) == (N_HOLD, levels)
    assert torch.equal(pred, torch.stack([t.argmax(dim=1) for t in z], dim=1))
    # fused against composed, with equal predictions wherever the top-two gap exceeds the bound
    was = enable_fused_foldin(False)
    try:
        zc, pc = fold.logits(tfidf), fold.predict(tfidf)
    finally:
        enable_fused_foldin(was)
    for l, (a, b) in enumerate(zip(z, zc)):
        e = R.rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"FoldInLevels level {l + 1} fused against composed: {e:.3e}")
        assert e < PARITY, (l, e)
        top = torch.topk(a, 2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 2 * PARITY * float(a.abs().max())
        assert torch.equal(pred[clear, l], pc[clear, l]) and bool(clear.any())
    # device CSR tensors are the same call; an empty batch; documents without a known word
    dev_csr = tuple(torch.from_numpy(x).to(cuda) for x in (tfidf.indptr.astype(np.int64), tfidf.indices.astype(np.int32),
                                                           tfidf.data.astype(np.float32)))
    assert all(torch.equal(a, b) for a, b in zip(fold.logits(dev_csr), z))
    import scipy.sparse as sp
    assert [tuple(t.shape) for t in fold.logits(sp.csr_matrix((0, fold.n_vocab), dtype=np.float32))] == \
        [(0, c) for c in (C1, C2, C3)[:levels]]
    assert tuple(fold.predict(sp.csr_matrix((0, fold.n_vocab), dtype=np.float32)).shape) == (0, levels)
    z0 = fold.logits(sp.csr_matrix((2, fold.n_vocab), dtype=np.float32))[-1]
    assert torch.equal(z0[0], z0[1]) and bool(torch.isfinite(z0).all())


def test_one_hot_link_and_refresh_follow_the_models(cuda, corpus):
    g, g2, _, tfidf = corpus
    models = _models(g, cuda, True)
    fold = FoldInLevels(models, [g, g2], link="one_hot")
    z, p = fold.logits(tfidf), fold.probabilities(tfidf)[0]
    assert torch.equal(p.argmax(dim=1), z[0].argmax(dim=1)) and bool(((p == 0) | (p == 1)).all()) and bool((p.sum(dim=1) == 1).all())
    soft = FoldInLevels(models, [g, g2])
    before = [t.clone() for t in soft.logits(tfidf)]
    models[1].train()
    opt = torch.optim.SGD(models[1].parameters(), lr=0.5)
    loss = nn.functional.cross_entropy(models[1](g2)[g2.train_mask], g2.y[g2.train_mask] % C2)
    opt.zero_grad()
    loss.backward()
    opt.step()
    models[1].eval()
    assert all(torch.equal(a, b) for a, b in zip(soft.logits(tfidf), before))      # frozen until refresh()
    assert soft.refresh() is soft and models[1].training is False
    after = soft.logits(tfidf)
    want, _ = _oracle_levels(models, [g, g2], tfidf, True)
    assert torch.equal(after[0], before[0])                                           # level 1 did not train
    assert R.rel_err(after[1].cpu().numpy(), want[1]) < PARITY
    assert R.rel_err(before[1].cpu().numpy(), want[1]) > 1e-3                         # the step did move the logits


def test_what_is_refused(cuda, corpus):
    g, g2, g3, _ = corpus
    N, V = g.x.size(0), int(g.n_vocab)
    m1, m2 = pkg.GCN(N, C1, n_hidden_gcn=8).to(cuda), pkg.GCN(N + C1, C2, n_hidden_gcn=8).to(cuda)

    def refused(models, graphs, word, exc=(NotImplementedError, ValueError), **kw):
        with pytest.raises(exc, match=word):
            FoldInLevels(models, graphs, **kw)

    refused([m1], [g], "levels")
    refused([m1, m2], [g], "one graph per model")
    refused([m1, m2], [g, g2], "link is one of", link="sigmoid")
    refused([m1, m2], [g2, g2], "level 1 takes sparse identity")
    refused([m1, m2], [g, g], "HierarchyFeatures")
    refused([m1, m2], [g, with_hierarchy(g, g2.x.to_sparse())], "HierarchyFeatures")
    refused([m1, m2], [g, g3], "n_features")
    moved = pkg.HierarchyFeatures(N, V - 1, classes=torch.zeros(N - V + 1, dtype=torch.int64, device=cuda), n_classes=C1)
    refused([m1, m2], [g, with_hierarchy(g, moved)], "h_row0")
    other = copy.copy(g2)
    other.edge_attr = g.edge_attr * 2
    refused([m1, m2], [g, other], "edge_attr")
    other = copy.copy(g2)
    other.n_vocab = V - 1
    refused([m1, m2], [g, other], "n_vocab")
    same = copy.copy(g2)
    same.edge_attr = g.edge_attr.clone()                                  # equal tensors are the same graph
    FoldInLevels([m1, m2], [g, same])
    refused([pkg.EGCN(N, C1, embedding_dim=16).to(cuda), m2], [g, g2], "EGCN")
    refused([m1, pkg.GCN(N + C1, C2, n_gcn=3).to(cuda)], [g, g2], "n_gcn != 2")
    refused([m1, pkg.GCN(N + C1, C2, activation=nn.Tanh, apply_activation=True).to(cuda)], [g, g2], "other activations")
    refused([m1, pkg.GCN(N + C1, C2, n_hidden_gcn=512).to(cuda)], [g, g2], "exceed")
    refused([pkg.GCN(N, 128, n_hidden_gcn=256).to(cuda), pkg.GCN(N + 128, 128, n_hidden_gcn=256).to(cuda)],
            [g, with_hierarchy(g, one_hot_hierarchy(g, g.y[V:], 128))], "bytes of LDS")
    # FoldIn itself still refuses the hierarchy graph
    with pytest.raises(NotImplementedError, match="HierarchyFeatures"):
        FoldIn(m2, g2)


def test_foldin_levels_under_hip_graph_capture(cuda, corpus):
    """One `FoldInLevels.logits` call on device CSR tensors captured on a single stream, replayed twice with the buffers
    refilled: bit for bit the eager results."""
    g, g2, g3, tfidf = corpus
    fold = FoldInLevels(_models(g, cuda, True, 3), [g, g2, g3])
    a, b = tfidf[:64], tfidf[64:128][::-1]
    nnz = max(a.nnz, b.nnz)

    def parts(m):
        col, val = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.float32)
        col[:m.nnz], val[:m.nnz] = m.indices, m.data
        return [torch.from_numpy(x).to(cuda) for x in (m.indptr.astype(np.int64), col, val)]

    pa, pb = parts(a.tocsr()), parts(b.tocsr())
    eager_a = [t.clone() for t in fold.logits(tuple(pa))]
    eager_b = [t.clone() for t in fold.logits(tuple(pb))]
    static = [t.clone() for t in pa]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fold.logits(tuple(static))
    for src, want in ((pb, eager_b), (pa, eager_a)):
        for s, t in zip(static, src):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        for o, w in zip(out, want):
            assert torch.equal(o.view(torch.int32), w.view(torch.int32))
