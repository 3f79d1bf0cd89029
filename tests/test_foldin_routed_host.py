"""Routed (per-label) fold-in on the CPU: the completeness of the kernel sweep's case table (tests/_foldin_routed_cases.py),
the exact family's 2^24 bound and its top-logit ties, the float family's zero-exclusion margin condition, the numpy
restatement (tests/_foldin_routed_ref.py) in fp32 against float64 and against the CPU oracle on `extended_graph` member by
member, the header's constants and LDS arithmetic, and the argument checks of `tgcn_foldin_routed`, which need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import sparse as sp

import _foldin_ref as R
import _foldin_routed_cases as rc
import _foldin_routed_ref as RR
from oracle import gcn_oracle as O
from pytextgcn_amd import _lib, synth
from pytextgcn_amd.inductive import extended_graph

PARITY = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the case table ----------------------------------------------------------------------------------------------------
def test_every_leaf_and_every_option_of_the_sweep_is_hit():
    ints, floats = rc.int_cases(), rc.float_cases()
    for c in ints + floats:
        K = len(c.Cs)
        assert 1 <= K <= rc.MAX_MEMBERS and c.top[1] == K and len(c.acts) == K + 1
        assert all(1 <= h <= rc.MAX_HIDDEN and 1 <= C <= rc.MAX_CLASSES for h, C in [c.top] + [(c.h, C) for C in c.Cs])
        assert RR.lds_bytes(*rc.widths_arrays(c, c.route == "top")) <= rc.LDS_LIMIT
        assert c.outs and ("top" not in c.outs or c.route == "top")
    assert len(rc.LEAVES) == 8
    for family in (ints, floats):
        hit = {rc.leaf_of(c) for c in family}
        skipped = [leaf for leaf in rc.LEAVES if leaf not in hit]
        assert len(skipped) <= 0, f"leaves without a case: {skipped}"              # cap: zero skipped
    assert len({rc.case_id(c) for c in ints + floats}) == len(ints + floats)
    assert {(c.top, c.h, c.Cs) for c in ints} >= set(rc.WIDTHS)
    assert {K for K in (len(c.Cs) for c in ints)} >= {1, 2, 64}
    for family in (ints, floats):
        assert {c.layout for c in family} == set(rc.LAYOUTS)
        assert {c.mode for c in family} == {R.REFERENCE, R.ACCURATE}
        assert {c.route for c in family} == set(rc.ROUTES)
        assert {c.class_map for c in family} == {False, True}
        assert {c.acts[0] for c in family if c.route == "top"} == {0, 1}
        assert {a for c in family for a in c.acts[1:]} == {0, 1}
        assert any(len(set(c.acts[1:])) == 2 for c in family)                      # activations differ between members
    for route in ("top", "given_bad"):
        for o in rc.OUTS:
            if o == "top" and route != "top":
                continue
            asked = {o in c.outs for c in ints if c.route == route}
            assert asked == {False, True}, (route, o)
    full = [c for c in ints if c.n_docs == rc.DOCS_PER_WORKGROUP + 1]
    assert all(rc.row_lengths(c)[:8] == list(rc.ROW_LENGTHS) for c in full)
    tile, stride = rc.DOCS_PER_WORKGROUP, rc.DOCS_PER_WORKGROUP * rc.WORKGROUP_CAP
    assert {0, 1, tile - 1, tile, tile + 1, 2 * stride + 1} <= {c.n_docs for c in ints}
    for c in ints + floats:
        r = rc.route_given(c)
        K = len(c.Cs)
        if c.route == "given" and c.n_docs >= K:
            assert set(r.tolist()) == set(range(K))                                # every member is met
        if c.route == "given_bad" and c.n_docs >= 9:
            assert -1 in r and K in r and ((r >= 0) & (r < K)).any()


def test_exact_family_keeps_every_partial_sum_below_2_to_24_and_breaks_a_tie():
    seen = dict(dup=False, first=False, last=False, outside=False, tie=False, routes=set())
    for c in rc.int_cases():
        if c.n_docs > 4 * rc.DOCS_PER_WORKGROUP:
            continue                                   # (checked where it runs, on the GPU: its rows are the short ones)
        o, ref = rc.operands(c), rc.reference(c)
        assert ref["units"] < 2 ** 24, (rc.case_id(c), ref["units"])
        for d in range(c.n_docs):
            cj = o["col"][o["rowptr"][d]:o["rowptr"][d + 1]]
            seen["dup"] |= cj.size != np.unique(cj).size
            seen["first"] |= bool(cj.size and cj[0] == 0)
            seen["last"] |= bool(cj.size and cj[-1] == c.n_vocab - 1)
            seen["outside"] |= bool(cj.size and (cj.min() < 0 or cj.max() >= c.n_vocab))
        if ref["top"] is not None and c.n_docs and len(c.Cs) >= 3:
            z = ref["top"]["z"]
            tied = (z == z.max(axis=1, keepdims=True)).sum(axis=1) > 1
            late = tied & (ref["route"] > 0)            # a tie whose first maximum is not column 0
            seen["tie"] |= bool(late.any())
            empty = np.diff(o["rowptr"]) == 0
            assert (ref["route"][empty] == 1).all() and tied[empty].all(), rc.case_id(c)
            seen["routes"] |= set(ref["route"].tolist())
    routes = seen.pop("routes")
    assert all(seen.values()), seen
    assert len(routes) > 3


def test_float_family_excludes_no_document():
    """A document enters the routed comparison only if its float64 top-logit margin exceeds twice the top logits' bound:
    every document of every case does (cap: zero excluded)."""
    excluded, total = 0, 0
    for c in rc.float_cases():
        ref = rc.reference(c)
        if ref["top"] is None:
            continue
        z = np.sort(ref["top"]["z"], axis=1)
        margin = z[:, -1] - z[:, -2] if z.shape[1] > 1 else np.full(z.shape[0], np.inf)
        excluded += int((margin <= 2 * ref["top_bz"].max(axis=1)).sum())
        total += z.shape[0]
    assert total >= 100 and excluded <= 0, (excluded, total)


def test_fp32_restatement_against_float64():
    """The fp32 evaluation of the definition (multiply, then add) picks the float64 route and stays within the derived bound
    of the float64 evaluation (an unfused multiply-add rounds twice where the FMA rounds once: twice the bound covers it)."""
    for c in rc.float_cases()[:6]:
        o, ref = rc.operands(c), rc.reference(c)
        f32 = RR.foldin_routed(o["rowptr"], o["col"], o["val"], o["dis"], c.mode, o["nets"], rc.route_given(c), np.float32)
        assert np.array_equal(f32["route"], ref["route"]), rc.case_id(c)
        assert np.array_equal(np.isneginf(f32["z"]), np.isneginf(ref["z"]))
        ok = np.isfinite(ref["z"])
        assert (np.abs(f32["z"][ok].astype(np.float64) - ref["z"][ok]) <= 2 * ref["bz"][ok]).all(), rc.case_id(c)
        assert (np.abs(f32["u"].astype(np.float64) - ref["u"]) <= 2 * ref["bu"]).all(), rc.case_id(c)
        if ref["top"] is not None:
            assert (np.abs(f32["top"]["z"].astype(np.float64) - ref["top"]["z"]) <= 2 * ref["top_bz"]).all()
        nobody = (ref["route"] < 0) | (ref["route"] >= len(c.Cs))
        assert (ref["pred"][nobody] == -1).all() and np.isneginf(ref["z"][nobody]).all() and not ref["u"][nobody].any()
        assert (ref["pred"][~nobody] >= 0).all()


def test_global_pred_follows_column_class_map():
    from pytextgcn_amd.perlabel import column_class_map
    lists = [[5, 9, 11], [2], [7, 8, 30, 31, 40]]
    cm = column_class_map(lists).numpy()
    pred, route = np.array([2, 0, 4, -1, 1]), np.array([0, 1, 2, -1, 0])
    assert RR.global_pred(pred, route, cm, [3, 1, 5]).tolist() == [11, 2, 40, -1, 9]


# ---- the restatement against the CPU oracle on the extended graph, member by member -------------------------------------
def test_restatement_matches_the_oracle_member_by_member():
    g = synth.word_doc_graph(70, 600, seed=5, device="cpu", n_classes=3, vocab_frac=0.58)
    V, N, K, Cs, h = int(g.n_vocab), 70, 3, (4, 2, 5), 12
    rng = np.random.default_rng(11)
    rows = []
    for n in (0, 1, 3, 17, 40, 9, 2):
        cols = np.sort(rng.choice(V, size=n, replace=False))
        v = rng.random(n) * 0.95 + 0.05
        rows.append((cols, (v / max(np.sqrt((v * v).sum()), 1e-30)).astype(np.float32)))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])])
    tfidf = sp.csr_matrix((np.concatenate([v for _, v in rows]), np.concatenate([c for c, _ in rows]), indptr),
                          shape=(len(rows), V), dtype=np.float32)
    torch.manual_seed(2)
    models = [O.GCNOracle(N, K, n_hidden_gcn=16).eval()] + [O.GCNOracle(N, C, n_hidden_gcn=h).eval() for C in Cs]
    gen = torch.Generator().manual_seed(7)
    relu = [True, False, False, False]
    nets, want = [], []
    with torch.no_grad():
        ge = extended_graph(g, tfidf)
        for m, r in zip(models, relu):
            for p in m.parameters():
                if p.dim() == 1:
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
            z, _ = R.gcn_forward(m, ge, r)
            base, h1 = R.gcn_forward(m, g, r)
            assert torch.equal(z[:N].view(torch.int32), base.view(torch.int32))               # the old rows do not move
            want.append(z[N:].numpy())
            W1, W2 = m.layers[0].weight, m.layers[1].weight
            nets.append(dict(T1=W1[:V].numpy(), P=(h1 @ W2)[:V].numpy(), W2=W2.numpy(), b1=m.layers[0].bias.numpy(),
                             b2=m.layers[1].bias.numpy(), act=R.ACT_RELU if r else R.ACT_NONE))
    dis = R.word_dis(g)
    res = RR.foldin_routed(tfidf.indptr, tfidf.indices, tfidf.data, dis, R.REFERENCE, nets, None, np.float32)
    e = R.rel_err(res["top"]["z"], want[0])
    print(f"restatement against the oracle's new rows: top {e:.2e}")
    assert e < PARITY
    assert np.array_equal(res["route"], np.argmax(want[0], axis=1))
    for k in range(K):                                  # every member on every document, by a given route
        r = RR.foldin_routed(tfidf.indptr, tfidf.indices, tfidf.data, dis, R.REFERENCE, nets, np.full(len(rows), k), np.float32)
        e = R.rel_err(r["z"][:, :Cs[k]], want[1 + k])
        print(f"restatement against the oracle's new rows: member {k} {e:.2e}")
        assert e < PARITY and np.isneginf(r["z"][:, Cs[k]:]).all()
        mine = res["route"] == k
        assert np.array_equal(res["z"][mine].view(np.int32), r["z"][mine].view(np.int32))


# ---- the header's constants and the LDS arithmetic ----------------------------------------------------------------------
def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _lds(lib, hs, Cs):
    return lib.tgcn_foldin_routed_lds_bytes(len(hs) - 1, _i32(hs), _i32(Cs))


def test_header_constants_and_lds_bytes():
    header = open(os.path.join(ROOT, "include", "tgcn.h")).read()
    assert int(re.search(r"#define TGCN_FOLDIN_MAX_MEMBERS (\d+)", header).group(1)) == rc.MAX_MEMBERS == _lib.FOLDIN_MAX_MEMBERS
    assert int(re.search(r"#define TGCN_FOLDIN_LEVELS_LDS_LIMIT (\d+)", header).group(1)) == rc.LDS_LIMIT
    assert int(re.search(r"#define TGCN_FOLDIN_DOCS_PER_WORKGROUP (\d+)", header).group(1)) == rc.DOCS_PER_WORKGROUP
    assert int(re.search(r"#define TGCN_FOLDIN_WORKGROUP_CAP (\d+)", header).group(1)) == rc.WORKGROUP_CAP
    lib = _lib.load()
    assert (lib.tgcn_foldin_max_hidden(), lib.tgcn_foldin_max_classes()) == (rc.MAX_HIDDEN, rc.MAX_CLASSES)
    for top, h, Cs in rc.WIDTHS + (rc.OVER_THE_LIMIT,):
        for with_top in (True, False):
            hs, cs = [top[0] if with_top else 0] + [h] * len(Cs), [top[1] if with_top else 0] + list(Cs)
            assert _lds(lib, hs, cs) == RR.lds_bytes(hs, cs, rc.DOCS_PER_WORKGROUP), (top, h, Cs, with_top)
    amazon = ([100] * 65, [64] + [1] * 64)              # 6 -> 64 classes at h = 100 needs far less than a CU has
    assert RR.lds_bytes([100] * 7, [6, 10, 11, 11, 10, 11, 11]) < 48 * 1024
    assert RR.lds_bytes(*amazon) < rc.LDS_LIMIT
    assert rc.LDS_LIMIT - 4096 < RR.lds_bytes([256, 256, 256], [2, 128, 4]) <= rc.LDS_LIMIT     # near the limit
    top, h, Cs = rc.OVER_THE_LIMIT
    assert RR.lds_bytes([top[0], h, h], [top[1]] + list(Cs)) > rc.LDS_LIMIT
    for hs, cs in (((4,), (4,)), ((4, 4, 8), (2, 4, 4)), ((4, 0), (1, 4)), ((4, 257), (1, 4)), ((4, 4), (1, 129)),
                   ((4, 4), (1, 0)), ((257, 4), (1, 4)), ([4] * 66, [65] + [1] * 65)):
        assert _lds(lib, list(hs), list(cs)) == -1, (hs, cs)
    assert lib.tgcn_foldin_routed_lds_bytes(2, None, None) == -1


# ---- argument errors need no GPU ----------------------------------------------------------------------------------------
A = 1 << 20                                          # a 16-byte aligned address nothing will ever dereference


def _member(**kw):
    d = dict(t1_col=0, p_col=64, W2=A, ldw2=8, b1=A, b2=A, h=64, C=8, act=_lib.ACT_NONE, reserved=0)
    d.update(kw)
    return _lib.FoldinMember(**d)


TOP = dict(t1_col=0, p_col=32, h=32, C=2, ldw2=4)
M1, M2 = dict(t1_col=40, p_col=104), dict(t1_col=112, p_col=176)


def _call(lib, members, **kw):
    a = dict(n_docs=3, rowptr=A, col=A, val=A, n_vocab=10, dis=A, degree_sum=_lib.DEGREE_REFERENCE, table=A, ldt=184,
             n_members=len(members) - 1, route_in=None, class_map=None, route_out=A, top_logits=A, ldtl=4, logits=A, ldl=8,
             pred=A, hidden=A, ldh=64)
    a.update(kw)
    arr = (_lib.FoldinMember * max(len(members), 1))(*members)
    return lib.tgcn_foldin_routed(a["n_docs"], a["rowptr"], a["col"], a["val"], a["n_vocab"], a["dis"], a["degree_sum"],
                                  a["table"], a["ldt"], a["n_members"], arr, a["route_in"], a["class_map"], a["route_out"],
                                  a["top_logits"], a["ldtl"], a["logits"], a["ldl"], a["pred"], a["hidden"], a["ldh"], None)


def test_argument_errors_do_not_need_a_gpu():
    lib = _lib.load()
    good = [_member(**TOP), _member(**M1), _member(**M2)]
    bad_calls = [dict(rowptr=None), dict(col=None), dict(val=None), dict(dis=None), dict(table=None), dict(table=A + 4),
                 dict(n_docs=-1), dict(n_vocab=0), dict(n_vocab=1 << 31), dict(degree_sum=2), dict(degree_sum=-1),
                 dict(ldt=186), dict(ldt=0), dict(ldt=180), dict(n_members=0), dict(n_members=65),
                 dict(ldtl=0), dict(ldtl=6), dict(ldl=4), dict(ldl=10), dict(ldh=60), dict(ldh=66),
                 dict(top_logits=A + 4), dict(logits=A + 8), dict(hidden=A + 4),
                 dict(route_out=None, top_logits=None, logits=None, pred=None, hidden=None),
                 dict(route_in=A)]                                            # (top_logits goes with the top network only)
    for kw in bad_calls:
        assert _call(lib, good, **kw) == _lib.E_INVALID, kw
        assert b"tgcn_foldin_routed" in lib.tgcn_last_error(), kw
    bad_members = [dict(h=0), dict(h=rc.MAX_HIDDEN + 1), dict(C=0), dict(C=rc.MAX_CLASSES + 1), dict(act=2), dict(act=-1),
                   dict(t1_col=2), dict(p_col=-4), dict(p_col=184), dict(ldw2=10), dict(ldw2=0), dict(W2=None), dict(b1=None),
                   dict(b2=None), dict(W2=A + 4), dict(b1=A + 8), dict(b2=A + 4)]
    for kw in bad_members:
        for at, base in enumerate((TOP, M1, M2)):
            mb = [dict(TOP), dict(M1), dict(M2)]
            mb[at].update(kw)
            assert _call(lib, [_member(**m) for m in mb]) == _lib.E_INVALID, (at, kw)
            assert b"tgcn_foldin_routed: member %d" % at in lib.tgcn_last_error(), (at, kw, lib.tgcn_last_error())
    assert _call(lib, [_member(**dict(TOP, C=3)), _member(**M1), _member(**M2)]) == _lib.E_INVALID     # the top's C is not K
    assert b"top network" in lib.tgcn_last_error()
    assert _call(lib, [_member(**TOP), _member(**M1), _member(**dict(M2, h=60))]) == _lib.E_INVALID     # unequal member h
    assert b"share one hidden width" in lib.tgcn_last_error()
    # what is fine: an empty batch whatever the pointers are; with route_in, entry 0 is not looked at
    assert _call(lib, good, n_docs=0, rowptr=None, col=None, val=None, table=None) == _lib.OK
    junk = _member(h=0, C=-3, W2=None, b1=None, b2=None, t1_col=-1, p_col=7, ldw2=0, act=9)
    assert _call(lib, [junk, _member(**M1), _member(**M2)], n_docs=0, route_in=A, top_logits=None) == _lib.OK
    assert _call(lib, good, n_docs=0, route_out=None, top_logits=None, logits=None, hidden=None) == _lib.OK     # pred alone
    # the LDS need is checked before anything is enqueued, and named
    top, h, Cs = rc.OVER_THE_LIMIT
    big = [_member(t1_col=0, p_col=256, h=256, C=2, ldw2=4), _member(t1_col=260, p_col=516, h=256, C=128, ldw2=128),
           _member(t1_col=644, p_col=900, h=256, C=128, ldw2=128)]
    assert _call(lib, big, ldt=1028, ldl=128, ldh=256, n_docs=0) == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert str(RR.lds_bytes([256, 256, 256], [2, 128, 128])) in msg and str(rc.LDS_LIMIT) in msg and "LDS" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(_call(lib, good, n_members=0))
