"""Fold-in on the GPU (csrc/foldin.hip, pytextgcn_amd/inductive.py).

Through the C ABI, on guarded buffers (tests/_arena.py): every operand is a strided view into a pool of NaN, every result a
view into a pool of a sentinel no result can equal.
  * exact family -- dyadic operands (tests/_foldin_cases.py): the fp32 result of ANY correct kernel in any summation order
    is the float64 evaluation of the definition bit for bit; no tolerance.  Rows of 0 .. 1100 entries with first / last /
    duplicate columns, every leaf, padded / tight / shared tables, s1, activation, both degree modes, pred and hidden in
    every combination, batches from none to two grid strides + 1, every sentinel in place afterwards.
  * float family -- random operands against float64, every element within the derived forward-error bound of
    tests/_foldin_ref.py:float_bounds.
  * a document's logits do not depend on the batch: bit-equal alone, first, last and in the middle of 300.
At module level: `FoldIn` of GCN (linear and ReLU) and of EGCN against the CPU oracles on `extended_graph` at the project's
parity bar (1e-5 max-norm relative), fused against composed, `refresh`, what is refused, and HIP-graph capture."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import _foldin_cases as fc
import _foldin_ref as R
from _arena import _Arena
from _egcn_ref import EGCNRef
from oracle import gcn_oracle as O
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, synth
from pytextgcn_amd.inductive import FoldIn, enable_fused_foldin, extended_graph

pytestmark = pytest.mark.gpu

SENTINEL = 0.15625               # finite, exact in fp32, not a value the exact family can produce next to NaN operands
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
    fc.operands.cache_clear()
    fc.reference.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture
def lib(cuda):
    return _lib.load()


def _r4(v):
    return (v + 3) & ~3


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def call_kernel(lib, pools, c, o):
    """One call of tgcn_foldin_two_layer on guarded, strided buffers; returns (status, logits, hidden, pred, arenas)."""
    dev, B, V, h, C = pools.dev, c.n_docs, c.n_vocab, c.h, c.C
    H4, C4 = _r4(h), _r4(C)
    pad = 8 if c.layout == "padded" else 0
    nnz = int(o["col"].size)
    ins = _Arena(pools, "nan", F32)
    if c.layout == "shared":                       # T1 and P are two views of one row-padded table
        itab = ins.take(V, H4 + C4, H4 + C4, 0)
        ldt1 = ldp = H4 + C4
    else:
        iT, iP = ins.take(V, h, H4 + pad, 0), ins.take(V, C, C4 + pad, 0)
        ldt1, ldp = H4 + pad, C4 + pad
    iW = ins.take(h, C, C4 + pad, 0)
    ib1, ib2 = ins.take(1, h, H4, 0), ins.take(1, C, C4, 0)
    is1 = ins.take(1, h, H4, 0) if o["s1"] is not None else None
    idis, ival = ins.take(1, V, _r4(V), 0), ins.take(1, nnz, _r4(nnz), 0)
    ins.fill(float("nan"))
    if c.layout == "shared":
        tab = ins.view(itab)
        tab[:, :h].copy_(_dev(o["T1"], dev))
        tab[:, H4:H4 + C].copy_(_dev(o["P"], dev))
        T1p, Pp = ins.ptr(itab), ins.ptr(itab) + 4 * H4
    else:
        ins.view(iT).copy_(_dev(o["T1"], dev))
        ins.view(iP).copy_(_dev(o["P"], dev))
        T1p, Pp = ins.ptr(iT), ins.ptr(iP)
    ins.view(iW).copy_(_dev(o["W2"], dev))
    ins.view(ib1).copy_(_dev(o["b1"], dev)[None, :])
    ins.view(ib2).copy_(_dev(o["b2"], dev)[None, :])
    if is1 is not None:
        ins.view(is1).copy_(_dev(o["s1"], dev)[None, :])
    ins.view(idis).copy_(_dev(o["dis"], dev)[None, :])
    if nnz:
        ins.view(ival).copy_(_dev(o["val"], dev)[None, :])
    rowptr = _dev(o["rowptr"], dev)
    col = _dev(o["col"], dev) if nnz else torch.zeros(1, dtype=torch.int32, device=dev)

    outs = _Arena(pools, "out", F32)
    iz = outs.take(B, C, C4 + pad, 0)
    ih = outs.take(B, h, H4 + pad, 0) if c.hidden else None
    outs.fill(SENTINEL)
    ints = _Arena(pools, "ints", torch.int32)
    ip = ints.take(1, B, _r4(B), 0) if c.pred else None
    ints.fill(PRED_SENTINEL)

    st = lib.tgcn_foldin_two_layer(B, rowptr.data_ptr(), col.data_ptr(), ins.ptr(ival), V, ins.ptr(idis),
                                   _lib.DEGREE_SUMS[c.mode], T1p, ldt1, h, ins.ptr(is1) if is1 is not None else None,
                                   ins.ptr(ib1), c.act, Pp, ldp, C, ins.ptr(iW), C4 + pad, ins.ptr(ib2), outs.ptr(iz), C4 + pad,
                                   ints.ptr(ip) if c.pred else None, outs.ptr(ih) if c.hidden else None,
                                   H4 + pad if c.hidden else 0, None)
    torch.cuda.synchronize()
    z = outs.view(iz).contiguous().cpu().numpy()
    hid = outs.view(ih).contiguous().cpu().numpy() if c.hidden else None
    pred = ints.view(ip).contiguous().cpu().numpy().reshape(-1) if c.pred else None
    return st, z, hid, pred, (outs, ints)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), f"{what}: non-finite values (an operand gap or a guard row reached it)"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, k = bad[0]
        pytest.fail(f"{what} differs at {bad.shape[0]} of {got.size} elements in {np.unique(bad[:, 0]).size} rows, first "
                    f"[{r}, {k}]: {got[r, k]!r} != {want[r, k]!r}")


def run_case(lib, pools, c):
    o, ref = fc.operands(c), fc.reference(c)
    if c.family == "int":
        assert ref["units"] < 2 ** 24, ref["units"]                    # the bound that makes fp32 exact, per case
    st, z, hid, pred, (outs, ints) = call_kernel(lib, pools, c, o)
    assert st == _lib.OK, (st, lib.tgcn_last_error().decode())
    if c.family == "int":
        _same(z, ref["z"].astype(np.float32), "logits")
        if c.hidden:
            _same(hid, ref["u"].astype(np.float32), "hidden")
        if c.pred:
            assert np.array_equal(pred, ref["pred"]), "pred is not the first arg-max of the exact logits"
    else:
        for name, got, want, bound in (("logits", z, ref["z"], ref["bz"]),) + ((("hidden", hid, ref["u"], ref["bu"]),) if c.hidden else ()):
            assert np.isfinite(got).all(), f"{name}: non-finite values"
            err = np.abs(got.astype(np.float64) - want)
            over = err > bound
            if over.any():
                r, k = np.argwhere(over)[0]
                pytest.fail(f"{name} beyond the forward-error bound at {int(over.sum())} elements, first [{r}, {k}]: error "
                            f"{err[r, k]:.3e}, bound {bound[r, k]:.3e}")
        if c.pred:
            assert np.array_equal(pred, R.first_argmax(z)), "pred is not the first arg-max of the stored logits"
    assert outs.untouched(), "a store outside the result views (gap columns / rows before or behind)"
    assert ints.untouched(), "a store outside pred"


def run_group(lib, pools, cases):
    failures = []
    for c in cases:
        try:
            run_case(lib, pools, c)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(f"{fc.case_id(c)} [{fc.leaf_of(c.h, c.C)}]: {str(e)[:300]}")
    if failures:
        pytest.fail(f"{len(failures)} of {len(cases)} cases fail:\n" + "\n".join(failures), pytrace=False)


def _by_leaf(cases):
    return [[c for c in cases if fc.leaf_of(c.h, c.C) == leaf] for leaf in fc.LEAVES]


@pytest.mark.parametrize("cases", _by_leaf(fc.int_cases()), ids=fc.LEAVES)
def test_foldin_exact(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("cases", _by_leaf(fc.float_cases()), ids=fc.LEAVES)
def test_foldin_float_within_the_forward_error_bound(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("h,C", [(200, 64), (63, 65)], ids=["vec-narrow", "tail-wide"])
def test_a_document_does_not_depend_on_its_batch(lib, pools, h, C):
    """Bit-equal logits alone, first, last and in the middle of a batch of 300 other documents."""
    base = fc._variant("float", 3, h, C, fc.DOCS_PER_WORKGROUP + 1, n_vocab=301)._replace(hidden=False, pred=False)
    o = dict(fc.operands(base))
    rp, probe = o["rowptr"], 6                                              # the 129-entry document
    mine = slice(int(rp[probe]), int(rp[probe + 1]))
    rng = np.random.default_rng(5)
    other_len = rng.integers(0, 40, size=299)
    other_col = rng.integers(0, base.n_vocab, size=int(other_len.sum())).astype(np.int32)
    other_val = (rng.random(other_col.size) * 0.9 + 0.05).astype(np.float32)

    def batch(pos):
        """the 299 others with the probe at `pos` (None: the probe alone)"""
        lens = [mine.stop - mine.start] if pos is None else list(other_len[:pos]) + [mine.stop - mine.start] + list(other_len[pos:])
        cut = 0 if pos is None else int(other_len[:pos].sum())
        col = np.concatenate([other_col[:cut], o["col"][mine], other_col[cut:]]) if pos is not None else o["col"][mine]
        val = np.concatenate([other_val[:cut], o["val"][mine], other_val[cut:]]) if pos is not None else o["val"][mine]
        ob = dict(o, rowptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col=col.astype(np.int32),
                  val=val.astype(np.float32))
        st, z, _, _, _ = call_kernel(lib, pools, base._replace(n_docs=len(lens)), ob)
        assert st == _lib.OK
        return z[0 if pos is None else pos].copy()

    alone = batch(None)
    assert np.isfinite(alone).all()
    for pos in (0, 299, 150):
        assert np.array_equal(alone.view(np.int32), batch(pos).view(np.int32)), pos


# ---- module level --------------------------------------------------------------------------------------------------------
N_HOLD = 150


@pytest.fixture(scope="module")
def corpus(cuda):
    """About 2 000 nodes; the last 150 documents are held out of the graph and become the new rows."""
    full = synth.word_doc_graph(2150, 60000, seed=7, device=cuda, n_classes=7, vocab_frac=0.28)
    g, tfidf, _ = synth.hold_out_documents(full, N_HOLD)
    assert g.x.size(0) == 2000 and tfidf.shape == (N_HOLD, int(g.n_vocab)) and tfidf.nnz > N_HOLD
    return g, tfidf, extended_graph(copy.copy(g).cpu(), tfidf)       # (Data.to moves in place: a shallow copy goes to the host)


def _bias_noise(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return model


def _oracle_logits(model, kind, ge, relu=False):
    """The CPU oracle with the model's parameters on the extended graph: its new rows."""
    N = ge.x.size(1)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        if kind == "egcn":
            ref = EGCNRef(N, state["layers.2.bias"].numel(), embedding_dim=state["layers.0.weight"].size(0),
                          n_hidden_gcn=state["layers.1.bias"].numel())
            ref.load_state_dict(state)
            return ref.eval()(ge)[N:].numpy()
        ref = O.GCNOracle(N, state["layers.1.bias"].numel(), n_hidden_gcn=state["layers.0.bias"].numel())
        ref.load_state_dict(state)
        return R.gcn_forward(ref.eval(), ge, relu)[0][N:].numpy()


def _model(kind, g, dev):
    N, C = g.x.size(0), 7
    torch.manual_seed(11)
    if kind == "egcn":
        m = pkg.EGCN(N, C, embedding_dim=96, n_hidden_gcn=64, dropout=0.5)
    else:
        m = pkg.GCN(N, C, n_hidden_gcn=100, dropout=0.5, apply_activation=(kind == "relu"))
    return _bias_noise(m.to(dev).float(), 13).eval()


@pytest.mark.parametrize("kind", ["linear", "relu", "egcn"])
def test_foldin_matches_the_oracle_on_the_extended_graph(cuda, corpus, kind):
    g, tfidf, ge = corpus
    model = _model(kind, g, cuda)
    fold = FoldIn(model, g)
    z = fold.logits(tfidf)
    assert tuple(z.shape) == (N_HOLD, 7) and z.dtype == torch.float32
    want = _oracle_logits(model, kind, ge, relu=(kind == "relu"))
    e = R.rel_err(z.cpu().numpy(), want)
    print(f"FoldIn({kind}) against the oracle on the extended graph: {e:.3e}")
    assert e < PARITY, e
    # ... and the model's own forward on the extended graph (the package against itself)
    with torch.no_grad():
        own = model(copy.copy(ge).to(cuda))[g.x.size(0):]
    assert R.rel_err(z.cpu().numpy(), own.cpu().numpy()) < PARITY
    pred = fold.predict(tfidf)
    assert pred.dtype == torch.int64 and torch.equal(pred, z.argmax(dim=1))
    # fused against composed
    was = enable_fused_foldin(False)
    try:
        assert was is True
        zc = fold.logits(tfidf)
        pc = fold.predict(tfidf)
    finally:
        assert enable_fused_foldin(was) is False
    ec = R.rel_err(z.cpu().numpy(), zc.cpu().numpy())
    print(f"FoldIn({kind}) fused against composed: {ec:.3e}")
    assert ec < PARITY, ec
    assert torch.equal(pc, zc.argmax(dim=1))
    # device CSR tensors are the same call
    dev_csr = tuple(torch.from_numpy(a).to(cuda) for a in (tfidf.indptr.astype(np.int64), tfidf.indices.astype(np.int32),
                                                           tfidf.data.astype(np.float32)))
    assert torch.equal(fold.logits(dev_csr), z)
    # an empty batch and a document without a known word
    import scipy.sparse as sp
    assert tuple(fold.logits(sp.csr_matrix((0, fold.n_vocab), dtype=np.float32)).shape) == (0, 7)
    z0 = fold.logits(sp.csr_matrix((2, fold.n_vocab), dtype=np.float32))
    assert torch.equal(z0[0], z0[1]) and bool(torch.isfinite(z0).all())


def test_accurate_degree_mode_follows_the_plan(cuda, corpus):
    g, tfidf, ge = corpus
    prev = pkg.set_degree_sum("accurate")
    try:
        pkg.clear_plan_cache()
        model = _model("linear", g, cuda)
        fold = FoldIn(model, g)
        assert fold.degree_sum == "accurate"
        z = fold.logits(tfidf)
        with torch.no_grad():
            own = model(copy.copy(ge).to(cuda))[g.x.size(0):]
    finally:
        pkg.set_degree_sum(prev)
        pkg.clear_plan_cache()
    assert R.rel_err(z.cpu().numpy(), own.cpu().numpy()) < PARITY
    assert R.rel_err(z.cpu().numpy(), _oracle_logits(model, "linear", ge)) < PARITY


@pytest.mark.parametrize("kind", ["linear", "relu", "egcn"])
def test_refresh_follows_the_model(cuda, corpus, kind):
    g, tfidf, ge = corpus
    model = _model(kind, g, cuda)
    fold = FoldIn(model, g)
    before = fold.logits(tfidf).clone()
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    loss = nn.functional.cross_entropy(model(g)[g.train_mask], g.y[g.train_mask])
    opt.zero_grad()
    loss.backward()
    opt.step()
    model.eval()
    assert torch.equal(fold.logits(tfidf), before)          # the tables are frozen: nothing moves until refresh()
    assert fold.refresh() is fold
    after = fold.logits(tfidf)
    want = _oracle_logits(model, kind, ge, relu=(kind == "relu"))
    e_after, e_before = R.rel_err(after.cpu().numpy(), want), R.rel_err(before.cpu().numpy(), want)
    print(f"refresh({kind}): {e_after:.3e} from the new oracle after refresh(), {e_before:.3e} before")
    assert e_after < PARITY
    assert e_before > 1e-3                                   # the step did move the logits
    assert model.training is False


@pytest.mark.parametrize("mode", [R.REFERENCE, R.ACCURATE])
def test_degree_mode_and_association_bit_for_bit(lib, pools, mode):
    """The two `degree_sum` modes told apart on the device.  T1 is the identity and b1 zero, so `hidden` holds the a_j
    themselves: document 0 has the weights [2^24, 1, 1, 1], whose fp32 sum in order absorbs the ones (deg 2^24) and whose
    float64 sum does not (deg 2^24 + 4); document 1 has 64 entries under irregular word factors, where (dis t) dis_d and
    t (dis dis_d) round differently.  Bit for bit the restatement's a_j of the mode, and not the other mode's."""
    V = h = 64
    rng = np.random.default_rng(17)
    rowptr = np.array([0, 4, 68], dtype=np.int64)
    col = np.concatenate([np.arange(4), rng.permutation(64)]).astype(np.int32)
    val = np.concatenate([[2.0 ** 24, 1.0, 1.0, 1.0], rng.random(64) * 0.9 + 0.05]).astype(np.float32)
    dis = (rng.random(V) * 0.9 + 0.05).astype(np.float32)
    o = dict(rowptr=rowptr, col=col, val=val, dis=dis, T1=np.eye(V, dtype=np.float32), s1=None,
             b1=np.zeros(h, dtype=np.float32), P=rng.standard_normal((V, 4)).astype(np.float32),
             W2=rng.standard_normal((h, 4)).astype(np.float32), b2=np.zeros(4, dtype=np.float32))
    c = fc.Case("float", h, 4, 2, V, "tight", False, 0, mode, False, True, 0)
    st, _, hid, _, (outs, ints) = call_kernel(lib, pools, c, o)
    assert st == _lib.OK and outs.untouched() and ints.untouched()
    want = {}
    for m in (R.REFERENCE, R.ACCURATE):
        a, _, dis_d = R.doc_scalars(rowptr, col.astype(np.int64), val, dis, m)
        w = np.zeros((2, h), dtype=np.float32)
        w[0, col[:4]], w[1, col[4:]] = a[:4], a[4:]
        want[m] = (w, dis_d)
    other = R.ACCURATE if mode == R.REFERENCE else R.REFERENCE
    assert want[R.REFERENCE][1][0] == np.float32(2.0 ** -12) != want[R.ACCURATE][1][0]            # the operands tell the sums apart ...
    assert not np.array_equal(want[mode][0][1], want[other][0][1])                                # ... and the associations
    assert np.array_equal(hid.view(np.int32), want[mode][0].view(np.int32)), "a_j are not the mode's bits"
    assert not np.array_equal(hid[0], want[other][0][0]) and not np.array_equal(hid[1], want[other][0][1])


def test_unsupported_models_and_features_are_refused(cuda, corpus):
    g, _, _ = corpus
    N = g.x.size(0)

    def refused(model, graph, word, move=True):
        with pytest.raises(NotImplementedError, match=word):
            FoldIn(model.to(cuda) if move else model, graph)

    refused(pkg.GCN(N, 7, n_gcn=3), g, "n_gcn != 2")
    refused(pkg.EGCN(N, 7, embedding_dim=16, n_gcn=3), g, "n_gcn != 2")
    refused(pkg.GCN(N, 7, activation=nn.Tanh, apply_activation=True), g, "other activations")
    refused(pkg.JumpingKnowledgeNetwork(N, 7), g, "JKN")
    refused(pkg.MLP(N, 7, hidden=[8]), g, "MLP")
    refused(pkg.GCN(N, 7, n_hidden_gcn=512), g, "exceed")
    # the K-member networks and the multi-GPU model: each names its cause
    from pytextgcn_amd.crossval import CrossValEGCN, CrossValGCN
    from pytextgcn_amd.sharded import ShardedGCN
    refused(CrossValGCN(N, 7, 3, n_hidden_gcn=8), g, "K-member")
    refused(CrossValEGCN(N, 7, 2, embedding_dim=8, n_hidden_gcn=8), g, "K-member")
    refused(pkg.PerLabelGCN(N, [3, 4], n_hidden_gcn=8), g, "K-member")
    refused(pkg.PerLabelMLP(N, [3, 4], [8]), g, "K-member")
    refused(ShardedGCN.__new__(ShardedGCN), g, "ShardedGCN", move=False)      # (its type is all FoldIn looks at)
    small = synth.word_doc_graph(60, 400, seed=1, device=cuda, n_classes=3, vocab_frac=0.5)
    dense = pkg.Data(x=torch.eye(60, device=cuda), edge_index=small.edge_index, edge_attr=small.edge_attr, n_vocab=small.n_vocab)
    refused(pkg.GCN(60, 3), dense, "dense")
    ar = torch.arange(60, device=cuda)
    ih = torch.sparse_coo_tensor(torch.stack([torch.cat([ar, ar[30:]]), torch.cat([ar, ar[30:] * 0 + 61])]),
                                 torch.ones(90, device=cuda), (60, 63)).coalesce()
    refused(pkg.GCN(63, 3), pkg.Data(x=ih, edge_index=small.edge_index, edge_attr=small.edge_attr, n_vocab=small.n_vocab),
            r"\[I \| H\]")
    held = pkg.HierarchyFeatures(60, 30, classes=torch.zeros(30, dtype=torch.int64), n_classes=3)
    refused(pkg.GCN(63, 3), pkg.Data(x=held, edge_index=small.edge_index, edge_attr=small.edge_attr, n_vocab=small.n_vocab),
            "HierarchyFeatures")
    scaled = torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.full((60,), 2.0, device=cuda), (60, 60)).coalesce()
    refused(pkg.GCN(60, 3), pkg.Data(x=scaled, edge_index=small.edge_index, edge_attr=small.edge_attr, n_vocab=small.n_vocab),
            "non-identity")
    # host input is checked before the copy
    import scipy.sparse as sp
    fold = FoldIn(pkg.GCN(60, 3).to(cuda), small)
    with pytest.raises(ValueError, match="columns"):
        fold.logits(sp.csr_matrix((2, fold.n_vocab + 1), dtype=np.float32))
    with pytest.raises(TypeError):
        fold.logits(np.zeros((2, fold.n_vocab), dtype=np.float32))
    bad = sp.csr_matrix((2, fold.n_vocab), dtype=np.float32)
    bad.indices, bad.data, bad.indptr = np.array([fold.n_vocab + 5], dtype=np.int32), np.ones(1, dtype=np.float32), \
        np.array([0, 1, 1], dtype=np.int32)                  # a matrix whose column id lies outside its width
    with pytest.raises(IndexError):
        fold.logits(bad)


def test_foldin_under_hip_graph_capture(cuda, corpus):
    """One `FoldIn.logits` call on device CSR tensors captured on a single stream, replayed twice with the buffers
    refilled: bit for bit the eager results."""
    g, tfidf, _ = corpus
    fold = FoldIn(_model("relu", g, cuda), g)
    a = tfidf[:64]
    b = tfidf[64:128][::-1]                                   # other documents
    nnz = max(a.nnz, b.nnz)

    def parts(m):
        col = np.zeros(nnz, dtype=np.int32)
        val = np.zeros(nnz, dtype=np.float32)
        col[:m.nnz], val[:m.nnz] = m.indices, m.data
        return [torch.from_numpy(x).to(cuda) for x in (m.indptr.astype(np.int64), col, val)]

    pa, pb = parts(a.tocsr()), parts(b.tocsr())
    eager_a, eager_b = fold.logits(tuple(pa)).clone(), fold.logits(tuple(pb)).clone()
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
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
