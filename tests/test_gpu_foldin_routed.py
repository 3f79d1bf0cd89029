"""Routed (per-label) fold-in on the GPU (csrc/foldin_routed.hip, pytextgcn_amd/inductive.py `FoldInPerLabel`).

Through the C ABI, on guarded buffers (tests/_arena.py): every operand is a strided view into a pool of NaN -- the gaps of
the combined table, of W2 and of the biases included, and in the `given` cases the top network's whole segment, so that any
read of it shows -- every result a view into a pool of a sentinel.
  * exact family -- dyadic operands (tests/_foldin_routed_cases.py): route, top logits, logits with their -inf fill, hidden
    and pred equal the float64 evaluation bit for bit, ties of the top logits included; every leaf, table layout, output
    combination, batch size, route form; a shape over the LDS limit is refused with every sentinel in place.
  * float family: every element within the forward-error bound of tests/_foldin_levels_ref.py:float_bounds; the route is the
    float64 one for every document (the margin condition is asserted on the CPU, tests/test_foldin_routed_host.py).
  * bit-equality with the flat kernel on the top tables and on member `route`'s tables; a document's bits do not depend on
    its batch or its neighbours' routes; the kernel's own route handed back as route_in gives the same bits.
At module level: `FoldInPerLabel` against the CPU oracle on `extended_graph` member by member, fused against composed,
`predict` against `PerLabelGCN.predict` on the extended graph, `from_members`, `refresh()`, the refusals, HIP-graph capture."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import _foldin_ref as R
import _foldin_routed_cases as rc
import _foldin_routed_ref as RR
from _arena import _Arena
from oracle import gcn_oracle as O
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, perlabel, synth
from pytextgcn_amd.inductive import FoldIn, FoldInPerLabel, enable_fused_foldin, extended_graph

pytestmark = pytest.mark.gpu

SENTINEL = 0.15625
INT_SENTINEL = -7
PARITY = 1e-5
F32 = torch.float32


class _Pools:
    def __init__(self, dev):
        self.dev = dev
        self.nan = self.out = self.ints = self.longs = None


@pytest.fixture(scope="module")
def pools(cuda):
    p = _Pools(cuda)
    yield p
    p.nan = p.out = p.ints = p.longs = None
    rc.operands.cache_clear()
    rc.reference.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture
def lib(cuda):
    return _lib.load()


def _r4(v):
    return (v + 3) & ~3


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table_layout(c):
    """(t1_col [K + 1], p_col [K + 1], ldt) of the combined table; network 0 is the top one."""
    nets = [c.top] + [(c.h, C) for C in c.Cs]
    gap = 8 if c.layout == "padded" else 0
    segs = [(kind, m, _r4(w)) for m, (h, C) in enumerate(nets) for kind, w in (("t", h), ("p", C))]
    if c.layout == "reversed":
        segs = [s for s in reversed(segs)]                       # P before T1, the members from the last to the top network
    t1, p, at = [0] * len(nets), [0] * len(nets), 0
    for kind, m, w in segs:
        (t1 if kind == "t" else p)[m] = at
        at += w + gap
    return t1, p, at + gap


def call_kernel(lib, pools, c, o, route_in="case"):
    """One call of tgcn_foldin_routed on guarded, strided buffers; returns (status, dict of numpy results, arenas)."""
    dev, B, V, K = pools.dev, c.n_docs, c.n_vocab, len(c.Cs)
    pad = 8 if c.layout == "padded" else 0
    nnz = int(o["col"].size)
    if isinstance(route_in, str):
        route_in = rc.route_given(c)
    with_top = route_in is None
    nets = [c.top] + [(c.h, C) for C in c.Cs]
    t1_col, p_col, ldt = table_layout(c)
    ins = _Arena(pools, "nan", F32)
    itab = ins.take(V, ldt, ldt, 0)
    iW, ib1, ib2 = [], [], []
    for h, C in nets:
        iW.append(ins.take(h, C, _r4(C) + pad, 0))
        ib1.append(ins.take(1, h, _r4(h), 0))
        ib2.append(ins.take(1, C, _r4(C), 0))
    idis, ival = ins.take(1, V, _r4(V), 0), ins.take(1, nnz, _r4(nnz), 0)
    ins.fill(float("nan"))
    tab = ins.view(itab)
    for m, ((h, C), net) in enumerate(zip(nets, o["nets"])):
        if m == 0 and not with_top:
            continue                                             # the top network stays NaN: nothing of it may be read
        tab[:, t1_col[m]:t1_col[m] + h].copy_(_dev(net["T1"], dev))
        tab[:, p_col[m]:p_col[m] + C].copy_(_dev(net["P"], dev))
        ins.view(iW[m]).copy_(_dev(net["W2"], dev))
        ins.view(ib1[m]).copy_(_dev(net["b1"], dev)[None, :])
        ins.view(ib2[m]).copy_(_dev(net["b2"], dev)[None, :])
    ins.view(idis).copy_(_dev(o["dis"], dev)[None, :])
    if nnz:
        ins.view(ival).copy_(_dev(o["val"], dev)[None, :])
    rowptr = _dev(o["rowptr"], dev)
    col = _dev(o["col"], dev) if nnz else torch.zeros(1, dtype=torch.int32, device=dev)
    route_dev = _dev(route_in, dev) if (route_in is not None and B) else None
    cmap = rc.class_map_of(c)
    cmap_dev = perlabel.column_class_map(cmap, dev) if cmap is not None else None

    cmax = max(c.Cs)
    outs, ints, longs = _Arena(pools, "out", F32), _Arena(pools, "ints", torch.int32), _Arena(pools, "longs", torch.int64)
    want = {k: k in c.outs for k in rc.OUTS}
    itop = outs.take(B, K, _r4(K) + pad, 0) if want["top"] else None
    iz = outs.take(B, cmax, _r4(cmax) + pad, 0) if want["logits"] else None
    ih = outs.take(B, c.h, _r4(c.h) + pad, 0) if want["hidden"] else None
    ir = ints.take(1, B, _r4(B), 0) if want["route"] else None
    ip = longs.take(1, B, _r4(B), 0) if want["pred"] else None
    outs.fill(SENTINEL)
    ints.fill(INT_SENTINEL)
    longs.fill(INT_SENTINEL)

    def optr(arena, i):
        return arena.ptr(i) if i is not None else None
    mb = (_lib.FoldinMember * (K + 1))()
    for m, (h, C) in enumerate(nets):
        if m == 0 and not with_top:
            mb[0] = _lib.FoldinMember(-1, 3, None, 0, None, None, 0, -5, 9, 0)      # not looked at
            continue
        mb[m] = _lib.FoldinMember(t1_col[m], p_col[m], ins.ptr(iW[m]), _r4(C) + pad, ins.ptr(ib1[m]), ins.ptr(ib2[m]), h, C,
                                  c.acts[m], 0)
    st = lib.tgcn_foldin_routed(B, rowptr.data_ptr(), col.data_ptr(), ins.ptr(ival), V, ins.ptr(idis), _lib.DEGREE_SUMS[c.mode],
                                ins.ptr(itab), ldt, K, mb, route_dev.data_ptr() if route_dev is not None else
                                (None if with_top else rowptr.data_ptr()),
                                cmap_dev.data_ptr() if cmap_dev is not None else None, optr(ints, ir), optr(outs, itop),
                                _r4(K) + pad, optr(outs, iz), _r4(cmax) + pad, optr(longs, ip), optr(outs, ih), _r4(c.h) + pad,
                                None)
    torch.cuda.synchronize()

    def host(arena, i, flat=False):
        if i is None:
            return None
        a = arena.view(i).contiguous().cpu().numpy()
        return a.reshape(-1) if flat else a
    res = dict(top=host(outs, itop), z=host(outs, iz), u=host(outs, ih), route=host(ints, ir, True), pred=host(longs, ip, True))
    return st, res, (outs, ints, longs)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert not np.isnan(got).any(), f"{what}: NaN (an operand gap, a guard row or the unread top segment reached it)"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = bad[0]
        pytest.fail(f"{what} differs at {bad.shape[0]} of {got.size} elements in {np.unique(bad[:, 0]).size} rows, first "
                    f"[{r}, {k}]: {got[r, k]!r} != {want[r, k]!r}")


def _within(got, want, bound, what):
    assert not np.isnan(got).any(), f"{what}: NaN"
    fill = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), fill), f"{what}: the -inf fill is not where the definition has it"
    err = np.where(fill, 0.0, np.abs(got.astype(np.float64) - np.where(fill, 0.0, want)))
    over = err > bound
    if over.any():
        r, k = np.argwhere(over)[0]
        pytest.fail(f"{what} beyond the forward-error bound at {int(over.sum())} elements, first [{r}, {k}]: error "
                    f"{err[r, k]:.3e}, bound {bound[r, k]:.3e}")


def _want_pred(c, ref):
    cmap = rc.class_map_of(c)
    if cmap is None:
        return ref["pred"]
    return RR.global_pred(ref["pred"], ref["route"], perlabel.column_class_map(cmap).numpy(), c.Cs)


def run_case(lib, pools, c):
    o = rc.operands(c)
    st, res, arenas = call_kernel(lib, pools, c, o)
    assert st == _lib.OK, (st, lib.tgcn_last_error().decode())
    ref = rc.reference(c)
    if res["route"] is not None:
        assert np.array_equal(res["route"], ref["route"]), "route"
    if c.family == "int":
        assert ref["units"] < 2 ** 24, ref["units"]                    # the bound that makes fp32 exact, per case
        if res["top"] is not None:
            _same(res["top"], ref["top"]["z"].astype(np.float32), "top logits")
        if res["z"] is not None:
            _same(res["z"], ref["z"].astype(np.float32), "logits")
        if res["u"] is not None:
            _same(res["u"], ref["u"].astype(np.float32), "hidden")
        if res["pred"] is not None:
            assert np.array_equal(res["pred"], _want_pred(c, ref)), "pred is not the (mapped) first arg-max of the exact logits"
    else:
        if res["top"] is not None:
            _within(res["top"], ref["top"]["z"], ref["top_bz"], "top logits")
        _within(res["z"], ref["z"], ref["bz"], "logits")
        _within(res["u"], ref["u"], ref["bu"], "hidden")
        K = len(c.Cs)
        ok = (ref["route"] >= 0) & (ref["route"] < K)
        local = np.where(ok, np.argmax(np.where(np.isnan(res["z"]), -np.inf, res["z"]), axis=1), -1)
        mine = dict(ref, pred=local)
        assert np.array_equal(res["pred"], _want_pred(c, mine)), "pred is not the (mapped) first arg-max of the kernel's logits"
    for a, what in zip(arenas, ("a float result", "route_out", "pred")):
        assert a.untouched(), f"a store outside the views of {what} (gap columns / rows before or behind)"


def run_group(lib, pools, cases):
    failures = []
    for c in cases:
        try:
            run_case(lib, pools, c)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(f"{rc.case_id(c)} [{rc.leaf_of(c)}]: {str(e)[:300]}")
    if failures:
        pytest.fail(f"{len(failures)} of {len(cases)} cases fail:\n" + "\n".join(failures), pytrace=False)


def _by_leaf(cases):
    return [[c for c in cases if rc.leaf_of(c) == leaf] for leaf in rc.LEAVES]


@pytest.mark.parametrize("cases", _by_leaf(rc.int_cases()), ids=rc.LEAVES)
def test_foldin_routed_exact(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("cases", _by_leaf(rc.float_cases()), ids=rc.LEAVES)
def test_foldin_routed_float_forward_error_bound(lib, pools, cases):
    run_group(lib, pools, cases)


def test_a_shape_over_the_lds_limit_is_refused_with_every_sentinel_intact(lib, pools):
    c = rc._variant("int", 1, rc.OVER_THE_LIMIT, 3, route="top")._replace(outs=rc.OUTS)
    st, res, arenas = call_kernel(lib, pools, c, rc.operands(c))
    assert st == _lib.E_INVALID
    msg = lib.tgcn_last_error().decode()
    assert str(RR.lds_bytes(*rc.widths_arrays(c))) in msg and "LDS" in msg, msg
    assert all((res[k] == SENTINEL).all() for k in ("top", "z", "u")) and (res["route"] == INT_SENTINEL).all()
    assert (res["pred"] == INT_SENTINEL).all() and all(a.untouched() for a in arenas)


# ---- consistency with the flat kernel -----------------------------------------------------------------------------------
def _flat(lib, dev, o, net, mode, rowptr, col, val):
    """tgcn_foldin_two_layer on plain device tensors; (z, u, pred) as numpy."""
    h, C = net["T1"].shape[1], net["P"].shape[1]
    B = len(rowptr) - 1

    def padded(a, w):
        t = torch.zeros(a.shape[0], _r4(w), dtype=F32, device=dev)
        t[:, :w] = _dev(a, dev)
        return t
    T1, P, W2 = padded(net["T1"], h), padded(net["P"], C), padded(net["W2"], C)
    b1, b2 = padded(net["b1"][None, :], h), padded(net["b2"][None, :], C)
    z = torch.full((B, _r4(C)), SENTINEL, dtype=F32, device=dev)
    u = torch.full((B, _r4(h)), SENTINEL, dtype=F32, device=dev)
    pred = torch.full((B,), INT_SENTINEL, dtype=torch.int32, device=dev)
    rp, cj, vj, dis = _dev(rowptr, dev), _dev(col, dev), _dev(val, dev), _dev(o["dis"], dev)
    if cj.numel() == 0:
        cj, vj = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=F32, device=dev)
    st = lib.tgcn_foldin_two_layer(B, rp.data_ptr(), cj.data_ptr(), vj.data_ptr(), net["T1"].shape[0], dis.data_ptr(),
                                   _lib.DEGREE_SUMS[mode], T1.data_ptr(), _r4(h), h, None, b1.data_ptr(), net["act"],
                                   P.data_ptr(), _r4(C), C, W2.data_ptr(), _r4(C), b2.data_ptr(), z.data_ptr(), _r4(C),
                                   pred.data_ptr(), u.data_ptr(), _r4(h), None)
    torch.cuda.synchronize()
    assert st == _lib.OK, lib.tgcn_last_error().decode()
    return z[:, :C].cpu().numpy(), u[:, :h].cpu().numpy(), pred.cpu().numpy()


def _spread_routes(o):
    """`o` with a top network whose b2 is zero: the top arg-max then follows the document and the routes spread."""
    nets = list(o["nets"])
    nets[0] = dict(nets[0], b2=np.zeros_like(nets[0]["b2"]))
    return dict(o, nets=nets)


def _mixed_batch(c, n_docs, seed):
    """The operands of `c` with a batch of `n_docs` random documents of 0 .. 70 entries in place of its own."""
    o = _spread_routes(rc.operands(c))
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 71, size=n_docs)
    o["rowptr"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    o["col"] = rng.integers(0, c.n_vocab, size=int(lens.sum())).astype(np.int32)
    o["val"] = (rng.random(o["col"].size) * 0.9 + 0.05).astype(np.float32)
    return o


@pytest.mark.parametrize("widths", [((100, 6), 100, (10, 11, 11, 10, 11, 11)), ((63, 5), 64, (65, 1, 4, 7, 9))],
                         ids=["amazon", "tail-wide"])
def test_routed_agrees_with_the_flat_kernel_bit_for_bit(lib, pools, widths):
    """300 documents with mixed routes: the top logits are `tgcn_foldin_two_layer`'s on the top tables, a document's logits
    those of `tgcn_foldin_two_layer` on member `route`'s tables, -inf behind them, and pred follows."""
    top, h, Cs = widths
    K = len(Cs)
    c = rc.Case("float", top, h, Cs, 300, 301, "padded", (1,) + tuple(k % 2 for k in range(K)), R.REFERENCE, rc.OUTS, False,
                "top", 77)
    o = _mixed_batch(c, 300, 3)
    st, res, _ = call_kernel(lib, pools, c, o)
    assert st == _lib.OK
    z, _, pred = _flat(lib, pools.dev, o, o["nets"][0], c.mode, o["rowptr"], o["col"], o["val"])
    assert np.array_equal(res["top"].view(np.int32), z.view(np.int32)), "the top logits differ from the flat kernel's bits"
    assert np.array_equal(res["route"], pred)
    assert len(np.unique(res["route"])) >= min(K, 4)                        # the routes are mixed
    for k in np.unique(res["route"]):
        docs = np.nonzero(res["route"] == k)[0]
        rp, cj, vj = RR.sub_csr(o["rowptr"], o["col"], o["val"], docs)
        z, u, pred = _flat(lib, pools.dev, o, o["nets"][1 + k], c.mode, rp, cj, vj)
        C = Cs[k]
        assert np.array_equal(res["z"][docs, :C].view(np.int32), z.view(np.int32)), k
        assert np.isneginf(res["z"][docs, C:]).all(), k
        assert np.array_equal(res["u"][docs].view(np.int32), u.view(np.int32)), k
        assert np.array_equal(res["pred"][docs], pred), k


def test_a_document_does_not_depend_on_its_batch_or_its_neighbours_routes(lib, pools):
    """Bit-equal top logits, logits and hidden alone, first, last and in the middle of 300 documents routed elsewhere."""
    top, h, Cs = (100, 6), 100, (10, 70, 11, 10, 128, 11)
    base = rc.Case("float", top, h, Cs, 1, 301, "padded", (0, 1, 0, 1, 0, 1, 0), R.REFERENCE, rc.OUTS, True, "top", 91)
    o = _spread_routes(rc.operands(base._replace(n_docs=rc.DOCS_PER_WORKGROUP + 1)))
    rp, probe = o["rowptr"], 6                                              # the 129-entry document
    mine = slice(int(rp[probe]), int(rp[probe + 1]))
    other = _mixed_batch(base, 299, 5)
    other_len = np.diff(other["rowptr"])

    def batch(pos):
        n = mine.stop - mine.start
        lens = [n] if pos is None else list(other_len[:pos]) + [n] + list(other_len[pos:])
        cut = 0 if pos is None else int(other_len[:pos].sum())
        col = o["col"][mine] if pos is None else np.concatenate([other["col"][:cut], o["col"][mine], other["col"][cut:]])
        val = o["val"][mine] if pos is None else np.concatenate([other["val"][:cut], o["val"][mine], other["val"][cut:]])
        ob = dict(o, rowptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col=col.astype(np.int32),
                  val=val.astype(np.float32))
        st, res, _ = call_kernel(lib, pools, base._replace(n_docs=len(lens)), ob)
        assert st == _lib.OK
        at = 0 if pos is None else pos
        if pos is not None:
            assert len(np.unique(res["route"])) > 2                        # the neighbours go elsewhere
        return [res[k][at].copy() for k in ("top", "z", "u")] + [res["route"][at:at + 1].astype(np.float32),
                                                                  res["pred"][at:at + 1].astype(np.float32)]

    alone = batch(None)
    assert not any(np.isnan(a).any() for a in alone)
    for pos in (0, 299, 150):
        for a, b in zip(alone, batch(pos)):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), pos


@pytest.mark.parametrize("widths", [((8, 4), 4, (8, 4, 12, 4)), ((8, 4), 8, (68, 4, 8, 72)), ((100, 6), 100, (10, 11, 11, 10, 11, 11)),
                                    ((63, 5), 64, (65, 1, 4, 7, 9))], ids=["vec-narrow", "vec-wide", "tail-narrow", "tail-wide"])
def test_the_kernels_own_route_handed_back_gives_the_same_bits(lib, pools, widths):
    """route_in = the route_out of a run with the top network: bit-equal logits, hidden and pred -- from the leaves without
    the top network, on a table whose top segment is NaN."""
    top, h, Cs = widths
    c = rc.Case("float", top, h, Cs, 120, 301, "tight", (1,) + (0, 1) * (len(Cs) // 2) + (0,) * (len(Cs) % 2), R.ACCURATE,
                rc.OUTS, True, "top", 33)
    o = _mixed_batch(c, 120, 8)
    st, with_top, _ = call_kernel(lib, pools, c, o)
    assert st == _lib.OK
    given = c._replace(route="given", outs=tuple(k for k in rc.OUTS if k != "top"))
    assert rc.leaf_of(given).startswith("given")
    st, res, _ = call_kernel(lib, pools, given, o, route_in=with_top["route"].astype(np.int32))
    assert st == _lib.OK
    assert np.array_equal(res["route"], with_top["route"]) and np.array_equal(res["pred"], with_top["pred"])
    for k in ("z", "u"):
        assert not np.isnan(res[k]).any(), "a NaN of the top segment was read"
        assert np.array_equal(res[k].view(np.int32), with_top[k].view(np.int32)), k


# ---- module level --------------------------------------------------------------------------------------------------------
N_HOLD, K_TOP, CS, H = 150, 4, (5, 3, 6, 2), 36


@pytest.fixture(scope="module")
def corpus(cuda):
    full = synth.word_doc_graph(2150, 60000, seed=7, device=cuda, n_classes=K_TOP, vocab_frac=0.28)
    g, tfidf, _ = synth.hold_out_documents(full, N_HOLD)
    return g, tfidf


def _bias_noise(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return model


def _models(g, dev, relu):
    N = g.x.size(0)
    torch.manual_seed(11)
    top = _bias_noise(pkg.GCN(N, K_TOP, n_hidden_gcn=100, dropout=0.5, apply_activation=relu).to(dev).float(), 13).eval()
    net = _bias_noise(pkg.PerLabelGCN(N, CS, n_hidden_gcn=H, dropout=0.5).to(dev).float(), 17).eval()
    return top, net


def _class_map():
    return [[100 * k + 7 * j for j in range(C)] for k, C in enumerate(CS)]


def _cpu_graph(g):
    out = copy.copy(g)
    out.x = g.x.cpu()
    for k in ("edge_index", "edge_attr", "y", "train_mask", "val_mask", "test_mask"):
        setattr(out, k, getattr(g, k).cpu())
    return out


def _oracle_rows(model, gc, tfidf, relu):
    """The CPU oracle's logits of the new nodes of `extended_graph(gc, tfidf)` for the package model `model`."""
    N = gc.x.size(0)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = O.GCNOracle(gc.x.size(1), state["layers.1.bias"].numel(), n_hidden_gcn=state["layers.0.bias"].numel())
    ref.load_state_dict(state)
    with torch.no_grad():
        ext = R.gcn_forward(ref.eval(), extended_graph(gc, tfidf), relu)[0]
        base = R.gcn_forward(ref, gc, relu)[0]
    assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))            # the exactness claim: old rows as they were
    return ext[N:].numpy()


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_foldin_perlabel_matches_the_oracle_member_by_member(cuda, corpus, relu):
    g, tfidf = corpus
    top, net = _models(g, cuda, relu)
    fold = FoldInPerLabel(top, net, g, _class_map())
    gc = _cpu_graph(g)
    z0 = fold.top_logits(tfidf)
    e = R.rel_err(z0.cpu().numpy(), _oracle_rows(top, gc, tfidf, relu))
    print(f"FoldInPerLabel top logits against the oracle on the extended graph: {e:.3e}")
    assert tuple(z0.shape) == (N_HOLD, K_TOP) and e < PARITY
    assert torch.equal(z0, FoldIn(top, g).logits(tfidf))                             # the flat fold-in of the top model, bit for bit
    route, z = fold.logits(tfidf)
    assert route.dtype == torch.int64 and torch.equal(route, z0.argmax(dim=1)) and tuple(z.shape) == (N_HOLD, max(CS))
    members = net.export_members()
    for k, (m, C) in enumerate(zip(members, CS)):
        want = _oracle_rows(m.eval(), gc, tfidf, False)
        forced = fold.logits(tfidf, route=torch.full((N_HOLD,), k))                  # every document through member k
        e = R.rel_err(forced[1][:, :C].cpu().numpy(), want)
        print(f"FoldInPerLabel member {k} against the oracle on the extended graph: {e:.3e}")
        assert e < PARITY and bool(torch.isneginf(forced[1][:, C:]).all()) and bool((forced[0] == k).all())
        mine = route == k
        assert torch.equal(z[mine], forced[1][mine])                                 # the routed rows are member k's, bit for bit
    # predictions: local arg-max through the class map; both levels from one launch
    cm = perlabel.column_class_map(_class_map(), cuda)
    local = z.argmax(dim=1)
    want_pred = cm[torch.tensor(net.seg_start, device=cuda)[route] + local]
    assert torch.equal(fold.predict(tfidf), want_pred)
    assert torch.equal(fold.predict_levels(tfidf), torch.stack([route, want_pred], dim=1))
    assert torch.equal(FoldInPerLabel(top, net, g).predict(tfidf), local)
    r = route.clone()
    r[::3] = -1
    p = fold.predict(tfidf, route=r)
    assert bool((p[::3] == -1).all()) and torch.equal(p[r >= 0], want_pred[r >= 0])
    # fused against composed
    was = enable_fused_foldin(False)
    try:
        zc0, (rc_, zc), pc = fold.top_logits(tfidf), fold.logits(tfidf), fold.predict(tfidf, route=r)
    finally:
        enable_fused_foldin(was)
    assert R.rel_err(z0.cpu().numpy(), zc0.cpu().numpy()) < PARITY
    top2 = torch.topk(z0, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * PARITY * float(z0.abs().max())
    assert bool(clear.any()) and torch.equal(rc_[clear], route[clear])
    same = clear & (rc_ == route)
    fin = torch.isfinite(z[same])
    assert torch.equal(fin, torch.isfinite(zc[same]))
    e = R.rel_err(z[same][fin].cpu().numpy(), zc[same][fin].cpu().numpy())
    print(f"FoldInPerLabel fused against composed: {e:.3e}")
    assert e < PARITY and bool((pc[::3] == -1).all())
    # device CSR tensors are the same call; an empty batch; documents without a known word
    dev_csr = tuple(torch.from_numpy(x).to(cuda) for x in (tfidf.indptr.astype(np.int64), tfidf.indices.astype(np.int32),
                                                           tfidf.data.astype(np.float32)))
    assert torch.equal(fold.logits(dev_csr)[1], z)
    import scipy.sparse as sp
    empty = sp.csr_matrix((0, fold.n_vocab), dtype=np.float32)
    assert tuple(fold.logits(empty)[1].shape) == (0, max(CS)) and tuple(fold.predict_levels(empty).shape) == (0, 2)
    z2 = fold.logits(sp.csr_matrix((2, fold.n_vocab), dtype=np.float32))[1]
    assert torch.equal(z2[0], z2[1]) and not bool(torch.isnan(z2).any())


def test_predict_agrees_with_perlabelgcn_on_the_extended_graph(cuda, corpus):
    """`FoldInPerLabel.predict` with a class map against `PerLabelGCN.predict` on `extended_graph` for the same documents,
    wherever the member's top-two gap is clear."""
    g, tfidf = corpus
    top, net = _models(g, cuda, True)
    cm_lists = _class_map()
    fold = FoldInPerLabel(top, net, g, cm_lists)
    route, z = fold.logits(tfidf)
    N = g.x.size(0)
    ge = extended_graph(g, tfidf)
    full_route = torch.full((N + N_HOLD,), -1, dtype=torch.int32, device=cuda)
    full_route[N:] = route.to(torch.int32)
    want = net.predict(ge, full_route, perlabel.column_class_map(cm_lists, cuda))[N:]
    got = fold.predict(tfidf)
    zz = torch.where(torch.isfinite(z), z, torch.full_like(z, -1e30))
    top2 = torch.topk(zz, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * PARITY * float(zz[torch.isfinite(z)].abs().max())
    assert int(clear.sum()) > N_HOLD // 2 and torch.equal(got[clear], want[clear])


def test_members_refresh_and_route_only(cuda, corpus):
    g, tfidf = corpus
    top, net = _models(g, cuda, False)
    members = net.export_members()
    a, b = FoldInPerLabel(top, net, g), FoldInPerLabel(top, members, g)
    assert torch.equal(a.logits(tfidf)[1], b.logits(tfidf)[1])                      # from_members: the same bits
    # no top model: every call needs a route, and gives what the routed call gives
    route = a.logits(tfidf)[0]
    c = FoldInPerLabel(None, net, g)
    with pytest.raises(ValueError, match="route="):
        c.predict(tfidf)
    assert torch.equal(c.logits(tfidf, route=route)[1], a.logits(tfidf)[1])
    with pytest.raises(ValueError, match="one entry per document"):
        a.predict(tfidf, route=route[:-1])
    # frozen until refresh() (every member in turn, by a given route)
    route = torch.arange(N_HOLD, device=cuda) % K_TOP
    before = a.logits(tfidf, route=route)[1].clone()
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    z = net(g)
    loss = nn.functional.cross_entropy(z[g.train_mask][:, :CS[0]], g.y[g.train_mask] % CS[0])
    opt.zero_grad()
    loss.backward()
    opt.step()
    net.eval()
    assert torch.equal(a.logits(tfidf, route=route)[1], before)
    assert a.refresh() is a and net.training is False
    after = a.logits(tfidf, route=route)[1]
    m0 = route == 0
    assert bool(m0.any()) and not torch.equal(after[m0], before[m0])                 # member 0 trained
    assert torch.equal(after[~m0], before[~m0])                                       # the others did not
    want = _oracle_rows(net.export_members()[0].eval(), _cpu_graph(g), tfidf, False)
    assert R.rel_err(after[m0][:, :CS[0]].cpu().numpy(), want[m0.cpu().numpy()]) < PARITY


def test_what_is_refused(cuda, corpus):
    g, tfidf = corpus
    N = g.x.size(0)
    top, net = pkg.GCN(N, 2, n_hidden_gcn=8).to(cuda), pkg.PerLabelGCN(N, (3, 4), n_hidden_gcn=8).to(cuda)

    def refused(word, top_model=top, network=net, graph=g, exc=(NotImplementedError, ValueError), **kw):
        with pytest.raises(exc, match=word):
            FoldInPerLabel(top_model, network, graph, **kw)

    FoldInPerLabel(top, net, g)
    refused("EGCN", top_model=pkg.EGCN(N, 2, embedding_dim=16).to(cuda))
    refused("JKN|JumpingKnowledge", top_model=pkg.JumpingKnowledgeNetwork(N, 2).to(cuda))
    refused("EGCN", network=[pkg.GCN(N, 3, n_hidden_gcn=8).to(cuda), pkg.EGCN(N, 4, embedding_dim=16).to(cuda)])
    refused("MLP", network=[pkg.GCN(N, 3, n_hidden_gcn=8).to(cuda), pkg.MLP(N, 4, [8]).to(cuda)])
    refused("n_gcn != 2", top_model=pkg.GCN(N, 2, n_gcn=3).to(cuda))
    refused("n_gcn != 2", network=[pkg.GCN(N, 3, n_gcn=3).to(cuda), pkg.GCN(N, 4, n_gcn=3).to(cuda)])
    refused("other activations", top_model=pkg.GCN(N, 2, activation=nn.Tanh, apply_activation=True).to(cuda))
    refused("other activations", network=[pkg.GCN(N, 3, n_hidden_gcn=8, apply_activation=True).to(cuda),
                                          pkg.GCN(N, 4, n_hidden_gcn=8).to(cuda)])
    refused("K = 2 members", top_model=pkg.GCN(N, 3, n_hidden_gcn=8).to(cuda))
    refused("exceed", top_model=pkg.GCN(N, 2, n_hidden_gcn=512).to(cuda))
    refused("exceed", network=pkg.PerLabelGCN(N, (3, 200), n_hidden_gcn=8).to(cuda))
    refused("kernel takes 64", top_model=None, network=pkg.PerLabelGCN(N, (1,) * 65, n_hidden_gcn=4).to(cuda))
    refused("bytes of LDS", network=pkg.PerLabelGCN(N, (128, 128), n_hidden_gcn=256).to(cuda))
    refused("PerLabelMLP.predict", network=pkg.PerLabelMLP(16, (3, 4), [8]).to(cuda))
    refused("class_map lists", class_map=[[1, 2, 3], [4, 5]])
    from pytextgcn_amd.perlevel import one_hot_hierarchy, with_hierarchy
    refused("hierarchy", graph=with_hierarchy(g, one_hot_hierarchy(g, g.y[int(g.n_vocab):], K_TOP)))
    dense_g = copy.copy(g)
    dense_g.x = torch.zeros(4, 4, device=cuda)
    refused("dense features", graph=dense_g)
    # FoldIn itself still refuses the K-member network, and now says where to go
    with pytest.raises(NotImplementedError, match="K-member networks.*FoldInPerLabel"):
        FoldIn(net, g)


def test_foldin_perlabel_under_hip_graph_capture(cuda, corpus):
    """One `FoldInPerLabel.predict` call on device CSR tensors captured on a single stream, replayed twice with the buffers
    refilled: the eager results."""
    g, tfidf = corpus
    top, net = _models(g, cuda, True)
    fold = FoldInPerLabel(top, net, g, _class_map())
    a, b = tfidf[:64], tfidf[64:128][::-1]
    nnz = max(a.nnz, b.nnz)

    def parts(m):
        col, val = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.float32)
        col[:m.nnz], val[:m.nnz] = m.indices, m.data
        return [torch.from_numpy(x).to(cuda) for x in (m.indptr.astype(np.int64), col, val)]

    pa, pb = parts(a.tocsr()), parts(b.tocsr())
    eager_a, eager_b = fold.predict(tuple(pa)).clone(), fold.predict(tuple(pb)).clone()
    static = [t.clone() for t in pa]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fold.predict(tuple(static))
    for src, want in ((pb, eager_b), (pa, eager_a)):
        for s, t in zip(static, src):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
