"""Per-level fold-in on the CPU: the numpy restatement (tests/_foldin_levels_ref.py) in fp32 against float64 and against the
CPU oracle on `extended_graph(..., hierarchy=...)`, the completeness of the kernel sweep's case table
(tests/_foldin_levels_cases.py), the header's constants and LDS arithmetic, and the argument checks of `tgcn_foldin_levels`,
which need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import sparse as sp

import _foldin_levels_cases as lc
import _foldin_levels_ref as LR
import _foldin_ref as R
from oracle import gcn_oracle as O
from pytextgcn_amd import _lib, synth
from pytextgcn_amd.inductive import extended_graph

PARITY = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the case table ----------------------------------------------------------------------------------------------------
def test_every_leaf_and_every_option_of_the_sweep_is_hit():
    ints, floats = lc.int_cases(), lc.float_cases()
    for c in ints + floats:
        assert 2 <= len(c.widths) <= lc.MAX_LEVELS and leaf_ok(c)
        assert all(1 <= h <= lc.MAX_HIDDEN and 1 <= C <= lc.MAX_CLASSES for h, C in c.widths)
        assert LR.lds_bytes(*zip(*c.widths)) <= lc.LDS_LIMIT
    assert len(lc.LEAVES) == 8
    for family in (ints, floats):
        hit = {lc.leaf_of(c.widths) for c in family}
        skipped = [leaf for leaf in lc.LEAVES if leaf not in hit]
        assert len(skipped) <= 0, f"leaves without a case: {skipped}"              # cap: zero skipped
    assert len({lc.case_id(c) for c in ints + floats}) == len(ints + floats)
    assert {c.widths for c in ints} >= set(lc.WIDTHS)
    assert {c.layout for c in ints} == set(lc.LAYOUTS) == {c.layout for c in floats}
    assert {c.mode for c in ints} == {R.REFERENCE, R.ACCURATE} == {c.mode for c in floats}
    for L in (2, 3):
        for level in range(L):
            mine = [c for c in ints + floats if len(c.widths) == L]
            assert {c.acts[level] for c in mine} == {0, 1}, (L, level)
            if level:
                assert {c.links[level] for c in mine} == {LR.SOFTMAX, LR.ONE_HOT}, (L, level)
        for o in lc.OUTS:
            asked = {o in c.outs for c in ints if len(c.widths) == L}
            assert asked == {False, True}, (L, o)
    assert all(all(k == LR.ONE_HOT for k in c.links[1:]) for c in ints)
    assert all(LR.SOFTMAX in c.links for c in floats)
    full = [c for c in ints if c.n_docs == lc.DOCS_PER_WORKGROUP + 1]
    assert all(lc.row_lengths(c)[:8] == list(lc.ROW_LENGTHS) for c in full)
    tile, stride = lc.DOCS_PER_WORKGROUP, lc.DOCS_PER_WORKGROUP * lc.WORKGROUP_CAP
    assert {0, 1, tile - 1, tile, tile + 1, 2 * stride + 1} <= {c.n_docs for c in ints}


def leaf_ok(c):
    return lc.leaf_of(c.widths) in lc.LEAVES


def test_exact_family_keeps_every_partial_sum_below_2_to_24():
    seen = dict(dup=False, first=False, last=False, outside=False)
    for c in lc.int_cases():
        if c.n_docs > 4 * lc.DOCS_PER_WORKGROUP:
            continue                                   # (checked where it runs, on the GPU: its rows are the short ones)
        o, ref = lc.operands(c), lc.reference(c)
        assert ref["units"] < 2 ** 24, (lc.case_id(c), ref["units"])
        for d in range(c.n_docs):
            cj = o["col"][o["rowptr"][d]:o["rowptr"][d + 1]]
            seen["dup"] |= cj.size != np.unique(cj).size
            seen["first"] |= bool(cj.size and cj[0] == 0)
            seen["last"] |= bool(cj.size and cj[-1] == c.n_vocab - 1)
            seen["outside"] |= bool(cj.size and (cj.min() < 0 or cj.max() >= c.n_vocab))
    assert all(seen.values()), seen


def test_fp32_restatement_against_float64():
    """The fp32 evaluation of the definition (multiply, then add) stays within the derived bound of the float64 one, level by
    level, when both take the same link rows; the fp32 softmax in the header's order agrees with float64's."""
    for c in lc.float_cases()[:4]:
        o = lc.operands(c)
        f32 = LR.foldin_levels(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["levels"], np.float32)
        links = [r["p"] for r in f32[1:]]
        f64 = LR.foldin_levels(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["levels"], np.float64, links_given=links,
                               want_abs=True)
        for li, (a, b, lv) in enumerate(zip(f32, f64, o["levels"])):
            bu, bz = LR.float_bounds(o["rowptr"], b, lv)
            # (an unfused multiply-add rounds twice where the FMA rounds once: twice the bound covers it)
            assert (np.abs(a["u"].astype(np.float64) - b["u"]) <= 2 * bu).all(), (lc.case_id(c), li)
            assert (np.abs(a["z"].astype(np.float64) - b["z"]) <= 2 * bz).all(), (lc.case_id(c), li)
            if li and lv["link"] == LR.SOFTMAX:
                want = LR.softmax_rows(f32[li - 1]["z"].astype(np.float32), np.float64)
                assert np.abs(a["p"] - want).max() < 1e-6 and np.allclose(a["p"].sum(axis=1), 1.0, atol=1e-5)


def test_one_hot_link_breaks_ties_at_the_first_maximum():
    z = np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [-1.0, -5.0, -1.0]], dtype=np.float32)
    assert LR.one_hot_rows(z).tolist() == [[0, 1, 0], [1, 0, 0], [1, 0, 0]]
    p = LR.softmax_rows(np.array([[80.0, -80.0, 0.0]], dtype=np.float32), np.float32)
    assert p[0, 0] == 1.0 and p[0, 1] == 0.0 and np.isfinite(p).all()


# ---- the restatement against the CPU oracle on the extended graphs ------------------------------------------------------
def test_restatement_matches_the_oracle_through_two_levels():
    g = synth.word_doc_graph(70, 600, seed=5, device="cpu", n_classes=3, vocab_frac=0.58)
    V, N, C1, C2 = int(g.n_vocab), 70, 3, 5
    rng = np.random.default_rng(11)
    rows = []
    for n in (0, 1, 3, 17, 40):
        cols = np.sort(rng.choice(V, size=n, replace=False))
        v = rng.random(n) * 0.95 + 0.05
        rows.append((cols, (v / max(np.sqrt((v * v).sum()), 1e-30)).astype(np.float32)))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])])
    tfidf = sp.csr_matrix((np.concatenate([v for _, v in rows]), np.concatenate([c for c, _ in rows]), indptr),
                          shape=(len(rows), V), dtype=np.float32)
    B = len(rows)
    torch.manual_seed(2)
    m1, m2 = O.GCNOracle(N, C1, n_hidden_gcn=16).eval(), O.GCNOracle(N + C1, C2, n_hidden_gcn=12).eval()
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for m in (m1, m2):
            for p in m.parameters():
                if p.dim() == 1:
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
        from pytextgcn_amd import HierarchyFeatures
        g2 = type(g)()
        g2.__dict__.update(g.__dict__)
        g2.x = HierarchyFeatures(N, V, classes=g.y[V:] % C1, n_classes=C1).to_sparse()
        ge1 = extended_graph(g, tfidf)
        z1, h1 = R.gcn_forward(m1, ge1, False)
        assert torch.equal(z1[:N].view(torch.int32), m1(g).view(torch.int32))              # the old rows do not move
        H_new = torch.softmax(z1[N:], dim=1)
        ge2 = extended_graph(g2, tfidf, hierarchy=H_new)
        assert tuple(ge2.x.shape) == (N + B, N + C1)
        assert torch.equal(ge2.x.to_dense()[N:, N:], H_new) and not ge2.x.to_dense()[N:, :N].any()
        assert torch.equal(ge2.x.to_dense()[:N], g2.x.to_dense())
        z2, _ = R.gcn_forward(m2, ge2, True)
        base2, h2 = R.gcn_forward(m2, g2, True)
        assert torch.equal(z2[:N].view(torch.int32), base2.view(torch.int32))
        # the default keeps the empty rows
        assert not extended_graph(g2, tfidf).x.to_dense()[N:].any()
        with pytest.raises(ValueError, match="hierarchy"):
            extended_graph(g, tfidf, hierarchy=H_new)
        with pytest.raises(ValueError, match="float32"):
            extended_graph(g2, tfidf, hierarchy=H_new[:, :2])
        W1a, W2a = m1.layers[0].weight, m1.layers[1].weight
        W1b, W2b = m2.layers[0].weight, m2.layers[1].weight
        _, h1g = R.gcn_forward(m1, g, False)
        levels = [dict(T1=W1a[:V].numpy(), P=(h1g @ W2a)[:V].numpy(), W2=W2a.numpy(), Wh=None, b1=m1.layers[0].bias.numpy(),
                       b2=m1.layers[1].bias.numpy(), act=R.ACT_NONE, link=None),
                  dict(T1=W1b[:V].numpy(), P=(h2 @ W2b)[:V].numpy(), W2=W2b.numpy(), Wh=W1b[N:N + C1].numpy(),
                       b1=m2.layers[0].bias.numpy(), b2=m2.layers[1].bias.numpy(), act=R.ACT_RELU, link=LR.SOFTMAX)]
    res = LR.foldin_levels(tfidf.indptr, tfidf.indices, tfidf.data, R.word_dis(g), R.REFERENCE, levels, np.float32)
    e1, e2 = R.rel_err(res[0]["z"], z1[N:].numpy()), R.rel_err(res[1]["z"], z2[N:].numpy())
    print(f"restatement against the oracle's new rows: level 1 {e1:.2e}, level 2 {e2:.2e}")
    assert e1 < PARITY and e2 < PARITY
    assert R.rel_err(res[1]["p"], H_new.numpy()) < PARITY


# ---- the header's constants and the LDS arithmetic ----------------------------------------------------------------------
def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_header_constants_and_lds_bytes():
    header = open(os.path.join(ROOT, "include", "tgcn.h")).read()
    assert int(re.search(r"#define TGCN_FOLDIN_LEVELS_LDS_LIMIT (\d+)", header).group(1)) == lc.LDS_LIMIT == 160 * 1024
    assert int(re.search(r"#define TGCN_FOLDIN_MAX_LEVELS (\d+)", header).group(1)) == lc.MAX_LEVELS == _lib.FOLDIN_MAX_LEVELS
    assert int(re.search(r"#define TGCN_FOLDIN_LINK_SOFTMAX (\d+)", header).group(1)) == _lib.LINK_SOFTMAX == LR.LINK_ID[LR.SOFTMAX]
    assert int(re.search(r"#define TGCN_FOLDIN_LINK_ONE_HOT (\d+)", header).group(1)) == _lib.LINK_ONE_HOT == LR.LINK_ID[LR.ONE_HOT]
    assert _lib.FOLDIN_LEVELS_LDS_LIMIT == lc.LDS_LIMIT
    lib = _lib.load()
    for widths in lc.WIDTHS + (lc.OVER_THE_LIMIT, ((100, 6), (100, 64)), ((100, 9), (100, 70))):
        hs, Cs = zip(*widths)
        assert lib.tgcn_foldin_levels_lds_bytes(len(hs), _i32(hs), _i32(Cs)) == LR.lds_bytes(hs, Cs, lc.DOCS_PER_WORKGROUP), widths
    assert LR.lds_bytes((100, 100), (6, 64)) < 48 * 1024                         # Amazon
    assert LR.lds_bytes((100, 100, 100), (9, 70, 128)) < lc.LDS_LIMIT            # three levels
    assert lc.LDS_LIMIT - 4096 < LR.lds_bytes((256, 8), (128, 4)) <= lc.LDS_LIMIT  # near the limit
    assert LR.lds_bytes(*zip(*lc.OVER_THE_LIMIT)) > lc.LDS_LIMIT
    for hs, Cs in (((4,), (4,)), ((4, 4, 4, 4), (4, 4, 4, 4)), ((0, 4), (4, 4)), ((257, 4), (4, 4)), ((4, 4), (4, 129)), ((4, 4), (0, 4))):
        assert lib.tgcn_foldin_levels_lds_bytes(len(hs), _i32(hs), _i32(Cs)) == -1, (hs, Cs)
    assert lib.tgcn_foldin_levels_lds_bytes(2, None, None) == -1


# ---- argument errors need no GPU ----------------------------------------------------------------------------------------
A = 1 << 20                                          # a 16-byte aligned address nothing will ever dereference


def _level(**kw):
    d = dict(t1_col=0, p_col=64, W2=A, ldw2=8, Wh=A, ldwh=64, b1=A, b2=A, logits=A, ldl=8, pred=None, hidden=None, ldh=0,
             link_out=None, ldk=0, h=64, C=8, act=_lib.ACT_NONE, link=_lib.LINK_SOFTMAX)
    d.update(kw)
    return _lib.FoldinLevel(**d)


def _call(lib, levels, **kw):
    a = dict(n_docs=3, rowptr=A, col=A, val=A, n_vocab=10, dis=A, degree_sum=_lib.DEGREE_REFERENCE, table=A, ldt=160,
             n_levels=len(levels))
    a.update(kw)
    arr = (_lib.FoldinLevel * max(len(levels), 1))(*levels)
    return lib.tgcn_foldin_levels(a["n_docs"], a["rowptr"], a["col"], a["val"], a["n_vocab"], a["dis"], a["degree_sum"],
                                  a["table"], a["ldt"], a["n_levels"], arr, None)


def test_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    first = dict(Wh=None, ldwh=0)
    second = dict(t1_col=72, p_col=136)
    bad_calls = [dict(rowptr=None), dict(col=None), dict(val=None), dict(dis=None), dict(table=None), dict(table=A + 4),
                 dict(n_docs=-1), dict(n_vocab=0), dict(n_vocab=1 << 31), dict(degree_sum=2), dict(degree_sum=-1),
                 dict(ldt=162), dict(ldt=0), dict(ldt=140), dict(n_levels=1), dict(n_levels=4)]
    for kw in bad_calls:
        assert _call(lib, [_level(**first), _level(**second)], **kw) == _lib.E_INVALID, kw
        assert b"tgcn_foldin_levels" in lib.tgcn_last_error()
    bad_levels = [dict(h=0), dict(h=lc.MAX_HIDDEN + 1), dict(C=0), dict(C=lc.MAX_CLASSES + 1), dict(act=2), dict(act=-1),
                  dict(t1_col=2), dict(p_col=-4), dict(p_col=156), dict(ldw2=6), dict(ldw2=10), dict(ldl=4), dict(ldl=9),
                  dict(hidden=A, ldh=60), dict(hidden=A, ldh=66), dict(W2=None), dict(b1=None), dict(b2=None), dict(W2=A + 4),
                  dict(b1=A + 8), dict(b2=A + 4), dict(logits=A + 4), dict(hidden=A + 4, ldh=64)]
    for kw in bad_levels:
        for at in (0, 1):
            lv = [dict(first), dict(second)]
            lv[at].update(kw)
            assert _call(lib, [_level(**lv[0]), _level(**lv[1])]) == _lib.E_INVALID, (at, kw)
            assert b"tgcn_foldin_levels: level %d" % (at + 1) in lib.tgcn_last_error(), (at, kw, lib.tgcn_last_error())
    for kw in (dict(link=2), dict(link=-1), dict(Wh=None), dict(Wh=A + 4), dict(ldwh=60), dict(ldwh=66),
               dict(link_out=A, ldk=4), dict(link_out=A, ldk=10), dict(link_out=A + 4, ldk=8)):
        assert _call(lib, [_level(**first), _level(**dict(second, **kw))]) == _lib.E_INVALID, kw
    assert _call(lib, [_level(**dict(first, link_out=A, ldk=8)), _level(**second)]) == _lib.E_INVALID       # level 1 has no link
    # what is fine: every output NULL, the level-1 Wh / link ignored, an empty batch whatever the pointers are
    assert _call(lib, [_level(**first), _level(**second)], n_docs=0, rowptr=None, col=None, val=None, table=None) == _lib.OK
    assert _call(lib, [_level(**dict(first, logits=None, link=77)), _level(**dict(second, logits=None))], n_docs=0) == _lib.OK
    # the LDS need is checked before anything else is looked at, and named
    hs, Cs = zip(*lc.OVER_THE_LIMIT)
    big = [_level(h=256, C=128, t1_col=0, p_col=256, ldw2=128, ldl=128, **first),
           _level(h=256, C=128, t1_col=384, p_col=640, ldw2=128, ldl=128, ldwh=256)]
    assert _call(lib, big, ldt=768, n_docs=0) == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert str(LR.lds_bytes(hs, Cs)) in msg and str(lc.LDS_LIMIT) in msg, msg
    with pytest.raises(ValueError):
        _lib.check(_call(lib, [_level(**first), _level(**second)], n_levels=1))
