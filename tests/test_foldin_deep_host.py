"""Layer-chain fold-in on the CPU: the completeness of the kernel sweep's case table (tests/_foldin_deep_cases.py), the
exactness condition of its exact family, the numpy restatement (tests/_foldin_deep_ref.py) against the CPU oracles on
`extended_graph` at depth 2, 3 and 4 -- GCN, EGCN and the JumpingKnowledgeNetwork -- the header's constants and LDS
arithmetic, and the argument checks of `tgcn_foldin_layers`, which need no GPU.

Recorded: the float64 restatement against the oracles' new rows at BASELINE's rel_err <= 1e-5 -- GCNOracle n_gcn = 3 / 4
1.6e-7 / 1.8e-7, EGCNRef n_gcn = 3 1.3e-7, JKNRef n_gcn = 2 / 3 1.1e-7 / 6.1e-8; the exact family's largest sum of absolute
values in units of the finest step 2^17.0 / 2^19.1 / 2^21.3 at L = 2 / 3 / 4, against the 2^24 it must stay below."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import sparse as sp

import _foldin_deep_cases as dc
import _foldin_deep_ref as DR
import _foldin_ref as R
from _egcn_ref import EGCNRef
from _jkn_ref import JKNRef
from oracle import gcn_oracle as O
from pytextgcn_amd import _lib, synth
from pytextgcn_amd.inductive import extended_graph

PARITY = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the case table ----------------------------------------------------------------------------------------------------
def test_every_leaf_and_every_option_of_the_sweep_is_hit():
    ints, floats = dc.int_cases(), dc.float_cases()
    for c in ints + floats:
        assert 2 <= len(c.widths) <= dc.MAX_LAYERS and dc.leaf_of(c.widths) in dc.LEAVES
        assert 1 <= c.widths[0] <= dc.MAX_FIRST and all(1 <= w <= dc.MAX_NEXT for w in c.widths[1:])
        assert DR.lds_bytes(c.widths) <= dc.LDS_LIMIT, c.widths
    assert len(dc.LEAVES) == 12
    for family in (ints, floats):
        hit = {dc.leaf_of(c.widths) for c in family}
        assert not [leaf for leaf in dc.LEAVES if leaf not in hit]
    assert len({dc.case_id(c) for c in ints + floats}) == len(ints + floats)
    assert {c.widths for c in ints} >= set(dc.WIDTHS)
    first, further = {c.widths[0] for c in ints}, {w for c in ints for w in c.widths[1:]}
    assert first >= {1, 4, 5, 63, 64, 65, 100, 200, 256} and further >= {1, 4, 5, 63, 64, 65, 100, 128}
    assert {c.layout for c in ints} == set(dc.LAYOUTS) == {c.layout for c in floats}
    assert {c.mode for c in ints} == {R.REFERENCE, R.ACCURATE} == {c.mode for c in floats}
    assert {c.s1 for c in ints} == {False, True} == {c.s1 for c in floats}
    for L in (2, 3, 4):
        mine = [c for c in ints + floats if len(c.widths) == L]
        for layer in range(L):
            assert {c.acts[layer] for c in mine} == {0, 1}, (L, layer)
        for leaf in (l for l in dc.LEAVES if l.startswith(f"L{L}-")):
            combos = {c.outs + (c.pred,) for c in ints if dc.leaf_of(c.widths) == leaf}
            assert len(combos) == 1 << (L + 1), leaf                    # every `out` and pred, present and absent
    full = [c for c in ints if c.n_docs == dc.DOCS_PER_WORKGROUP + 1]
    assert all(dc.row_lengths(c)[:7] == list(dc.EXACT_ROW_LENGTHS) for c in full)
    assert all(dc.row_lengths(c)[:8] == list(dc.ROW_LENGTHS) for c in floats)
    tile, stride = dc.DOCS_PER_WORKGROUP, dc.DOCS_PER_WORKGROUP * dc.WORKGROUP_CAP
    assert {0, 1, tile - 1, tile, tile + 1, 2 * stride + 1} <= {c.n_docs for c in ints}
    assert {c.n_vocab for c in ints} == {37} and {c.n_vocab for c in floats} == {301}


def test_exact_family_keeps_every_partial_sum_below_2_to_24():
    seen = dict(dup=False, first=False, last=False, outside=False)
    worst = {2: 0.0, 3: 0.0, 4: 0.0}
    for c in dc.int_cases():
        if c.n_docs > 4 * dc.DOCS_PER_WORKGROUP:
            continue                                   # (checked where it runs, on the GPU: its rows are the short ones)
        o, ref = dc.operands(c), dc.reference(c)
        assert ref["units"] < 2 ** 24, (dc.case_id(c), ref["units"])
        worst[len(c.widths)] = max(worst[len(c.widths)], ref["units"])
        for d in range(c.n_docs):
            cj = o["col"][o["rowptr"][d]:o["rowptr"][d + 1]]
            seen["dup"] |= cj.size != np.unique(cj).size
            seen["first"] |= bool(cj.size and cj[0] == 0)
            seen["last"] |= bool(cj.size and cj[-1] == c.n_vocab - 1)
            seen["outside"] |= bool(cj.size and (cj.min() < 0 or cj.max() >= c.n_vocab))
    print("largest sum of absolute values in units of the finest step, per depth:", {k: f"2^{np.log2(max(v, 1)):.1f}" for k, v in worst.items()})
    assert all(seen.values()), seen


def test_fp32_restatement_against_float64():
    """The fp32 evaluation of the definition (multiply, then add) stays within the derived bound of the float64 one, layer by
    layer (an unfused multiply-add rounds twice where the FMA rounds once: twice the bound covers it)."""
    for c in [c for c in dc.float_cases() if c.widths[0] <= 100][:5]:
        o, ref = dc.operands(c), dc.reference(c)
        f32 = DR.foldin_layers(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["layers"], o["s1"], np.float32)
        for li, (a, b, bound) in enumerate(zip(f32, ref["layers"], ref["bounds"])):
            assert a["x"].dtype == np.float32
            assert (np.abs(a["x"].astype(np.float64) - b["x"]) <= 2 * bound).all(), (dc.case_id(c), li)


def test_the_two_layer_chain_is_the_two_layer_definition():
    """At L = 2 the restatement is _foldin_ref.foldin's, value for value, and the bound is its bound."""
    c = [c for c in dc.float_cases() if len(c.widths) == 2 and c.s1][0]
    o, ref = dc.operands(c), dc.reference(c)
    l1, l2 = o["layers"]
    keep = (o["col"] >= 0) & (o["col"] < c.n_vocab)
    assert not keep.all()
    # (the two-layer restatement has no skipped columns: drop them, and give the row its degree back through a zero entry)
    col, val = np.where(keep, o["col"], 0), o["val"]
    T1 = l1["T"].copy()
    z, u, U, Zp = R.foldin(o["rowptr"], col, val, o["dis"], c.mode, T1, o["s1"], l1["b"], l1["act"], l2["T"], l2["W"], l2["b"],
                           np.float64, want_abs=True)
    full = keep.reshape(-1)
    docs = [d for d in range(c.n_docs) if full[o["rowptr"][d]:o["rowptr"][d + 1]].all()]
    assert len(docs) >= 10
    assert np.array_equal(ref["layers"][0]["x"][docs], u[docs])
    if l2["act"] == R.ACT_NONE:
        assert np.array_equal(ref["layers"][1]["x"][docs], z[docs])
    bu, _ = R.float_bounds(o["rowptr"], ref["layers"][0]["a_dd"], c.widths[0], u, U, Zp, l2["W"], l2["b"])
    assert np.allclose(ref["bounds"][0][docs], bu[docs], rtol=1e-12, atol=0)


# ---- the restatement against the CPU oracles on the extended graph -----------------------------------------------------
@pytest.fixture(scope="module")
def small():
    g = synth.word_doc_graph(70, 600, seed=5, device="cpu", n_classes=3, vocab_frac=0.58)
    V = int(g.n_vocab)
    rng = np.random.default_rng(11)
    rows = []
    for n in (0, 1, 3, 17, 40):
        cols = np.sort(rng.choice(V, size=n, replace=False))
        v = rng.random(n) * 0.95 + 0.05
        rows.append((cols, (v / max(np.sqrt((v * v).sum()), 1e-30)).astype(np.float32)))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])])
    tfidf = sp.csr_matrix((np.concatenate([v for _, v in rows]), np.concatenate([c for c, _ in rows]), indptr),
                          shape=(len(rows), V), dtype=np.float32)
    return g, tfidf


def _noise(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
    return model.eval()


def _layers_of(convs, g, first_operand, acts=None):
    """The frozen operands of the chain from an oracle's GCNConv layers, run layer by layer on `g`: (layers, activations)."""
    V = int(g.n_vocab)
    layers, hs, h = [], [], None
    for l, conv in enumerate(convs):
        xw = first_operand if l == 0 else h @ conv.weight
        layers.append(dict(T=xw[:V].numpy(), W=None if l == 0 else conv.weight.numpy(), b=conv.bias.numpy(), act=R.ACT_NONE))
        h = O.gcn_conv(xw, g.edge_index, g.edge_attr, torch.eye(xw.size(1)), conv.bias, True)
        hs.append(h)
    return layers, hs


def _restated(g, tfidf, layers, s1=None):
    return DR.foldin_layers(tfidf.indptr, tfidf.indices, tfidf.data, R.word_dis(g), R.REFERENCE, layers, s1, np.float64)


WORST = {}


@pytest.mark.parametrize("n_gcn", [3, 4])
def test_restatement_matches_the_gcn_oracle_and_the_old_rows_do_not_move(small, n_gcn):
    g, tfidf = small
    N = g.x.size(0)
    torch.manual_seed(2 + n_gcn)
    m = _noise(O.GCNOracle(N, 5, n_gcn=n_gcn, n_hidden_gcn=16), 7)
    with torch.no_grad():
        ext, base = m(extended_graph(g, tfidf)), m(g)
        # (d) what the exactness claim rests on at depth 3 and 4: no old node's row changes
        assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))
        layers, _ = _layers_of(list(m.layers), g, m.layers[0].weight)
    res = _restated(g, tfidf, layers)
    e = R.rel_err(res[-1]["x"], ext[N:].numpy())
    WORST[f"GCN n_gcn={n_gcn}"] = e
    print(f"restatement (float64) against GCNOracle(n_gcn={n_gcn})'s new rows: {e:.2e}")
    assert e <= PARITY


def test_restatement_matches_the_egcn_oracle(small):
    g, tfidf = small
    N = g.x.size(0)
    torch.manual_seed(9)
    m = _noise(EGCNRef(N, 5, embedding_dim=24, n_gcn=3, n_hidden_gcn=16), 8)
    with torch.no_grad():
        ext, base = m(extended_graph(g, tfidf)), m(g)
        assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))
        lin, convs = m.layers[0], list(m.layers[1:])
        emb = torch.selu(torch.sparse.mm(g.x, lin.weight.t()) + lin.bias)
        layers, _ = _layers_of(convs, g, emb @ convs[0].weight)
        s1 = (torch.selu(lin.bias) @ convs[0].weight).numpy()          # a new document's feature row is empty
    res = _restated(g, tfidf, layers, s1)
    e = R.rel_err(res[-1]["x"], ext[N:].numpy())
    WORST["EGCN n_gcn=3"] = e
    print(f"restatement (float64) against EGCNRef(n_gcn=3)'s new rows: {e:.2e}")
    assert e <= PARITY


@pytest.mark.parametrize("n_gcn", [2, 3])
def test_restatement_matches_the_jkn_oracle(small, n_gcn):
    """The chain's L rows, then the reference's own row-wise tail (JK-LSTM, attention, activation, lin) on them."""
    g, tfidf = small
    N = g.x.size(0)
    torch.manual_seed(20 + n_gcn)
    m = _noise(JKNRef(N, 5, n_gcn=n_gcn, n_hidden_gcn=12), 9)
    with torch.no_grad():
        ext, base = m(extended_graph(g, tfidf)), m(g)
        assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))
        layers, _ = _layers_of(list(m.layers), g, m.layers[0].weight)
        res = _restated(g, tfidf, layers)
        xs = [torch.from_numpy(r["x"]).float() for r in res]
        z = m.lin(m.activation(m.jk(xs)))
    e = R.rel_err(z.numpy(), ext[N:].numpy())
    WORST[f"JKN n_gcn={n_gcn}"] = e
    print(f"restatement (float64 chain) against JKNRef(n_gcn={n_gcn})'s new rows: {e:.2e}")
    assert e <= PARITY


# ---- the header's constants and the LDS arithmetic ----------------------------------------------------------------------
def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_header_constants_and_lds_bytes():
    header = open(os.path.join(ROOT, "include", "tgcn.h")).read()
    assert int(re.search(r"#define TGCN_FOLDIN_MAX_LAYERS (\d+)", header).group(1)) == dc.MAX_LAYERS == _lib.FOLDIN_MAX_LAYERS
    assert _lib.FOLDIN_LEVELS_LDS_LIMIT == dc.LDS_LIMIT
    assert ctypes.sizeof(_lib.FoldinLayer) == 56
    lib = _lib.load()
    for widths in dc.WIDTHS + (dc.OVER_THE_LIMIT, (100, 100), (100, 100, 64), (128, 128, 128)):
        assert lib.tgcn_foldin_layers_lds_bytes(len(widths), _i32(widths)) == DR.lds_bytes(widths, dc.DOCS_PER_WORKGROUP), widths
    assert 53 * 1024 > DR.lds_bytes((100, 100)) > 52 * 1024                          # JKN h = 100, L = 2
    assert DR.lds_bytes((100, 100, 64)) == 83552                                     # GCN 100 -> 100 -> 64
    assert dc.LDS_LIMIT >= DR.lds_bytes((100, 100, 100, 100)) > 140 * 1024           # JKN h = 100, L = 4: fits
    assert DR.lds_bytes(dc.OVER_THE_LIMIT) > dc.LDS_LIMIT                            # JKN h = 128, L = 4: refused
    for widths in ((4,), (4, 4, 4, 4, 4), (0, 4), (257, 4), (4, 129), (4, 0), (4, 4, 129), (256, 4, 4, 200)):
        assert lib.tgcn_foldin_layers_lds_bytes(len(widths), _i32(widths)) == -1, widths
    assert lib.tgcn_foldin_layers_lds_bytes(2, None) == -1
    assert lib.tgcn_foldin_layers_lds_bytes(2, _i32((256, 128))) > 0


# ---- argument errors need no GPU ----------------------------------------------------------------------------------------
A = 1 << 20                                          # a 16-byte aligned address nothing will ever dereference


def _layer(**kw):
    d = dict(W=A, ldw=8, b=A, out=A, ldo=8, t_col=64, width=8, act=_lib.ACT_NONE, reserved=0)
    d.update(kw)
    return _lib.FoldinLayer(**d)


FIRST = dict(W=None, ldw=0, t_col=0, width=64, ldo=64)


def _call(lib, layers, **kw):
    a = dict(n_docs=3, rowptr=A, col=A, val=A, n_vocab=10, dis=A, degree_sum=_lib.DEGREE_REFERENCE, table=A, ldt=80, s1=None,
             n_layers=len(layers), pred=None)
    a.update(kw)
    arr = (_lib.FoldinLayer * max(len(layers), 1))(*layers)
    return lib.tgcn_foldin_layers(a["n_docs"], a["rowptr"], a["col"], a["val"], a["n_vocab"], a["dis"], a["degree_sum"],
                                  a["table"], a["ldt"], a["s1"], a["n_layers"], arr, a["pred"], None)


def test_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    third = dict(t_col=72)
    bad_calls = [dict(rowptr=None), dict(col=None), dict(val=None), dict(dis=None), dict(table=None), dict(table=A + 4),
                 dict(s1=A + 4), dict(n_docs=-1), dict(n_vocab=0), dict(n_vocab=1 << 31), dict(degree_sum=2), dict(degree_sum=-1),
                 dict(ldt=82), dict(ldt=0), dict(ldt=68), dict(n_layers=1), dict(n_layers=5)]
    for kw in bad_calls:
        assert _call(lib, [_layer(**FIRST), _layer(), _layer(**third)], **kw) == _lib.E_INVALID, kw
        assert b"tgcn_foldin_layers" in lib.tgcn_last_error()
    bad_layers = [dict(width=0), dict(act=2), dict(act=-1), dict(t_col=2), dict(t_col=-4), dict(t_col=76), dict(ldo=4),
                  dict(ldo=66), dict(b=None), dict(b=A + 8), dict(out=A + 4)]
    for kw in bad_layers:
        for at in (0, 1, 2):
            ly = [dict(FIRST), dict(), dict(third)]
            ly[at].update(kw)
            assert _call(lib, [_layer(**v) for v in ly]) == _lib.E_INVALID, (at, kw)
            assert b"tgcn_foldin_layers: layer %d" % (at + 1) in lib.tgcn_last_error(), (at, kw, lib.tgcn_last_error())
    assert _call(lib, [_layer(**dict(FIRST, width=dc.MAX_FIRST + 1, ldo=260)), _layer()], ldt=264) == _lib.E_INVALID
    assert b"layer 1" in lib.tgcn_last_error() and b"256" in lib.tgcn_last_error()
    for kw in (dict(width=dc.MAX_NEXT + 1, ldw=132, ldo=132, t_col=64), dict(W=None), dict(W=A + 4), dict(ldw=4), dict(ldw=10)):
        assert _call(lib, [_layer(**FIRST), _layer(**kw)], ldt=200) == _lib.E_INVALID, kw
        assert b"layer 2" in lib.tgcn_last_error(), kw
    # what is fine: every output NULL, layer 1's W and ldw ignored, an empty batch whatever the pointers are
    assert _call(lib, [_layer(**FIRST), _layer()], n_docs=0, rowptr=None, col=None, val=None, table=None) == _lib.OK
    assert _call(lib, [_layer(**dict(FIRST, W=A + 4, ldw=3, out=None, ldo=1)), _layer(out=None, ldo=0)], n_docs=0) == _lib.OK
    # the LDS need is checked before anything is looked at behind the sizes, and named
    w = dc.OVER_THE_LIMIT
    big = [_layer(W=None if l == 0 else A, ldw=128, ldo=128, t_col=128 * l, width=128) for l in range(4)]
    assert _call(lib, big, ldt=512, n_docs=0) == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert str(DR.lds_bytes(w)) in msg and str(dc.LDS_LIMIT) in msg and "LDS" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(_call(lib, [_layer(**FIRST), _layer()], n_layers=1))
