"""`FoldInDeep` on the GPU (pytextgcn_amd/inductive.py): GCN and EGCN at n_gcn 3 and 4 and the JumpingKnowledgeNetwork
against the package's own eval forward on `extended_graph(g, tfidf)` and against the CPU oracles with the same state dict, at
BASELINE's rel_err <= 1e-5; the fused chain and the composed one (`enable_fused_foldin(False)`) against the float64
restatement of the frozen tables within the derived bound of tests/_foldin_deep_ref.py; predict, predict_text, refresh,
HIP-graph capture, and every refusal by its cause."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import _foldin_deep_ref as DR
import _foldin_ref as R
from _egcn_ref import EGCNRef
from _jkn_ref import JKNRef
from oracle import gcn_oracle as O
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, synth
from pytextgcn_amd.inductive import FoldIn, FoldInDeep, enable_fused_foldin, extended_graph

pytestmark = pytest.mark.gpu

PARITY = 1e-5
N_HOLD, C = 60, 7


@pytest.fixture(scope="module")
def corpus(cuda):
    """500 nodes; the last 60 documents are held out of the graph and become the new rows."""
    full = synth.word_doc_graph(560, 14000, seed=7, device=cuda, n_classes=C, vocab_frac=0.3)
    g, tfidf, _ = synth.hold_out_documents(full, N_HOLD)
    assert g.x.size(0) == 500 and tfidf.shape == (N_HOLD, int(g.n_vocab)) and tfidf.nnz > N_HOLD
    return g, tfidf, extended_graph(copy.copy(g).cpu(), tfidf)


def _bias_noise(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(p.device))
    return model


KINDS = {
    "gcn3-linear": lambda N: pkg.GCN(N, C, n_gcn=3, n_hidden_gcn=100),
    "gcn3-relu": lambda N: pkg.GCN(N, C, n_gcn=3, n_hidden_gcn=100, apply_activation=True),
    "gcn4": lambda N: pkg.GCN(N, C, n_gcn=4, n_hidden_gcn=64),
    "egcn3": lambda N: pkg.EGCN(N, C, embedding_dim=96, n_gcn=3, n_hidden_gcn=64),
    "jkn2": lambda N: pkg.JumpingKnowledgeNetwork(N, C, n_gcn=2, n_hidden_gcn=100),
    "jkn3": lambda N: pkg.JumpingKnowledgeNetwork(N, C, n_gcn=3, n_hidden_gcn=64),
}


def _model(kind, g, dev):
    torch.manual_seed(11)
    return _bias_noise(KINDS[kind](g.x.size(0)).to(dev).float(), 13).eval()


def _oracle(model, kind, ge):
    """The CPU oracle with the model's parameters on the extended graph: (its new rows, alpha of the new rows or None)."""
    N = ge.x.size(1)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    L = len(FoldInDeep._convs(model))
    with torch.no_grad():
        if kind.startswith("egcn"):
            ref = EGCNRef(N, C, embedding_dim=state["layers.0.weight"].size(0), n_gcn=L, n_hidden_gcn=state["layers.1.bias"].numel())
            ref.load_state_dict(state)
            return ref.eval()(ge)[N:].numpy(), None
        if kind.startswith("jkn"):
            ref = JKNRef(N, C, n_gcn=L, n_hidden_gcn=state["layers.0.bias"].numel())
            ref.load_state_dict(state)
            ref.eval()
            x, acts = ge.x, []
            for layer in ref.layers:
                x = layer(x, ge.edge_index, ge.edge_attr)
                acts.append(x)
            out, alpha = ref.jk.forward_with_alpha(acts)
            return ref.lin(ref.activation(out))[N:].numpy(), alpha[N:].numpy()
        ref = O.GCNOracle(N, C, n_gcn=L, n_hidden_gcn=state["layers.0.bias"].numel())
        ref.load_state_dict(state)
        x = ge.x
        for i, layer in enumerate(ref.eval().layers):
            x = layer(x, ge.edge_index, ge.edge_attr)
            if kind.endswith("relu") and i < L - 1:
                x = torch.relu(x)
        return x[N:].numpy(), None


def _frozen(fold):
    """The frozen tables of a FoldInDeep as tests/_foldin_deep_ref.py takes them."""
    tab = fold._tab.cpu().numpy()
    layers = []
    for l, w in enumerate(fold.widths):
        layers.append(dict(T=tab[:, fold.t_col[l]:fold.t_col[l] + w], W=fold.W[l][:, :w].cpu().numpy() if l else None,
                           b=fold.b[l].cpu().numpy(), act=fold.act[l]))
    return layers, (None if fold.s1 is None else fold.s1.cpu().numpy()), fold.dis.cpu().numpy()


@pytest.mark.parametrize("kind", list(KINDS))
def test_foldin_deep_matches_the_model_and_the_oracle_on_the_extended_graph(cuda, corpus, kind):
    g, tfidf, ge = corpus
    N = g.x.size(0)
    model = _model(kind, g, cuda)
    fold = FoldInDeep(model, g)
    z = fold.logits(tfidf)
    assert tuple(z.shape) == (N_HOLD, C) and z.dtype == torch.float32
    want, want_alpha = _oracle(model, kind, ge)
    e = R.rel_err(z.cpu().numpy(), want)
    with torch.no_grad():
        own = model(copy.copy(ge).to(cuda))[N:]
    e_own = R.rel_err(z.cpu().numpy(), own.cpu().numpy())
    print(f"FoldInDeep({kind}): {e:.3e} from the oracle on the extended graph, {e_own:.3e} from the model's own forward on it")
    assert e <= PARITY and e_own <= PARITY, (e, e_own)
    if kind.startswith("jkn"):
        alpha = fold.alpha(tfidf)
        assert tuple(alpha.shape) == (N_HOLD, len(fold.widths))
        e_alpha = R.rel_err(alpha.cpu().numpy(), want_alpha)
        print(f"FoldInDeep({kind}) alpha against the oracle: {e_alpha:.3e}")
        assert e_alpha <= PARITY, e_alpha
    else:
        with pytest.raises(TypeError, match="JumpingKnowledgeNetwork"):
            fold.alpha(tfidf)
    pred = fold.predict(tfidf)
    assert pred.dtype == torch.int64 and torch.equal(pred, z.argmax(dim=1))

    # the chain, fused and composed, against the float64 restatement of the frozen tables: any fp32 evaluation with one
    # rounding per term stays within the derived bound (a gamma bound holds in every order of summation); the composed
    # path multiplies and adds a_dd s1 and a_dd y in two roundings where the kernel's FMA takes one: twice the bound
    acts = fold.activations(tfidf)
    assert [tuple(a.shape) for a in acts] == [(N_HOLD, w) for w in fold.widths]
    assert torch.equal(acts[-1], z) or kind.startswith("jkn")
    layers, s1, dis = _frozen(fold)
    ref = DR.foldin_layers(tfidf.indptr, tfidf.indices, tfidf.data, dis, fold.degree_sum, layers, s1, np.float64, want_abs=True)
    bounds = DR.float_bounds(tfidf.indptr, ref, layers)
    was = enable_fused_foldin(False)
    try:
        assert was is True
        acts_c, zc, pc = fold.activations(tfidf), fold.logits(tfidf), fold.predict(tfidf)
    finally:
        assert enable_fused_foldin(was) is False
    for l, (a, b, r, bound) in enumerate(zip(acts, acts_c, ref, bounds)):
        ea = np.abs(a.cpu().numpy().astype(np.float64) - r["x"])
        eb = np.abs(b.cpu().numpy().astype(np.float64) - r["x"])
        print(f"  layer {l + 1}: fused {float((ea / np.maximum(bound, 1e-300)).max()):.3f} of the bound, composed "
              f"{float((eb / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (ea <= bound).all(), (kind, l)
        assert (eb <= 2 * bound).all(), (kind, l)
    assert R.rel_err(z.cpu().numpy(), zc.cpu().numpy()) <= PARITY
    assert torch.equal(pc, zc.argmax(dim=1))

    # device CSR tensors are the same call; an empty batch; documents without a known word
    dev_csr = tuple(torch.from_numpy(a).to(cuda) for a in (tfidf.indptr.astype(np.int64), tfidf.indices.astype(np.int32),
                                                           tfidf.data.astype(np.float32)))
    assert torch.equal(fold.logits(dev_csr), z)
    import scipy.sparse as sp
    assert tuple(fold.logits(sp.csr_matrix((0, fold.n_vocab), dtype=np.float32)).shape) == (0, C)
    assert tuple(fold.predict(sp.csr_matrix((0, fold.n_vocab), dtype=np.float32)).shape) == (0,)
    z0 = fold.logits(sp.csr_matrix((2, fold.n_vocab), dtype=np.float32))
    assert torch.equal(z0[0], z0[1]) and bool(torch.isfinite(z0).all())


def test_a_two_layer_gcn_is_foldin_bit_for_bit(cuda, corpus):
    g, tfidf, _ = corpus
    torch.manual_seed(3)
    model = _bias_noise(pkg.GCN(g.x.size(0), C, n_hidden_gcn=100, apply_activation=True).to(cuda).float(), 5).eval()
    a, b = FoldInDeep(model, g), FoldIn(model, g)
    assert torch.equal(a.logits(tfidf).view(torch.int32), b.logits(tfidf).view(torch.int32))
    assert torch.equal(a.predict(tfidf), b.predict(tfidf))


@pytest.mark.parametrize("kind", ["gcn3-relu", "jkn2"])
def test_refresh_follows_the_model(cuda, corpus, kind):
    g, tfidf, ge = corpus
    model = _model(kind, g, cuda)
    fold = FoldInDeep(model, g)
    before = fold.logits(tfidf).clone()
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    loss = nn.functional.cross_entropy(model(g)[g.train_mask], g.y[g.train_mask])
    opt.zero_grad()
    loss.backward()
    opt.step()
    model.eval()
    assert torch.equal(fold.logits(tfidf), before)          # everything is frozen: nothing moves until refresh()
    assert fold.refresh() is fold and model.training is False
    after = fold.logits(tfidf)
    want, _ = _oracle(model, kind, ge)
    e_after, e_before = R.rel_err(after.cpu().numpy(), want), R.rel_err(before.cpu().numpy(), want)
    print(f"refresh({kind}): {e_after:.3e} from the new oracle after refresh(), {e_before:.3e} before")
    assert e_after <= PARITY
    assert e_before > 1e-3                                   # the step did move the logits


def test_predict_text_round_trip(cuda):
    docs, y = synth.synthetic_corpus(260, 300, n_classes=4, seed=3)
    inside, new_docs = docs[:220], docs[220:]
    t2g = pkg.Text2GraphTransformer(n_jobs=1, min_df=2, window_size=10, rm_stopwords=False)
    g = t2g.fit_transform(inside, list(y[:220]), val_idx=np.arange(20)).to(cuda)
    torch.manual_seed(5)
    model = _bias_noise(pkg.GCN(g.x.size(1), 4, n_gcn=3, n_hidden_gcn=32).to(cuda).float(), 6).eval()
    fold = FoldInDeep(model, g)
    tfidf = t2g.transform(new_docs)
    assert tfidf.shape == (40, fold.n_vocab) and tfidf.nnz > 40
    pred = fold.predict_text(t2g, new_docs)
    assert torch.equal(pred, fold.predict(tfidf)) and torch.equal(pred, fold.logits(tfidf).argmax(dim=1))
    with torch.no_grad():
        own = model(extended_graph(g, tfidf))[g.x.size(0):]
    assert R.rel_err(fold.logits(tfidf).cpu().numpy(), own.cpu().numpy()) <= PARITY


def test_foldin_deep_under_hip_graph_capture(cuda, corpus):
    """One `FoldInDeep.logits` call on device CSR tensors captured on a single stream (one linear chain of launches, no
    parallel branches), replayed twice with the buffers refilled: bit for bit the eager results."""
    g, tfidf, _ = corpus
    fold = FoldInDeep(_model("gcn3-relu", g, cuda), g)
    a, b = tfidf[:24], tfidf[24:48][::-1]
    nnz = max(a.nnz, b.nnz)

    def parts(m):
        col, val = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.float32)
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


def test_what_is_refused_is_refused_by_its_cause(cuda, corpus):
    g, _, _ = corpus
    N = g.x.size(0)

    def refused(model, graph, word, move=True):
        with pytest.raises(NotImplementedError, match=word):
            FoldInDeep(model.to(cuda) if move else model, graph)

    refused(pkg.GCN(N, C, n_gcn=5), g, "n_gcn outside 2..4")
    refused(pkg.JumpingKnowledgeNetwork(N, C, n_gcn=5, n_hidden_gcn=8), g, "n_gcn outside 2..4")
    refused(pkg.GCN(N, C, n_gcn=3, activation=nn.Tanh, apply_activation=True), g, "other activations than nn.ReLU")
    FoldInDeep(pkg.GCN(N, C, n_gcn=3, activation=nn.Tanh).to(cuda), g)               # constructed, never applied: linear
    FoldInDeep(pkg.JumpingKnowledgeNetwork(N, C, n_hidden_gcn=8, activation=nn.Tanh).to(cuda), g)   # row-wise, after the chain
    odd = pkg.GCN(N, C, n_gcn=3)
    odd.layers[1].improved = True
    refused(odd, g, "improved=False")
    refused(pkg.GCN(N, C, n_gcn=3, n_hidden_gcn=200), g, "exceed")
    refused(pkg.GCN(N, C, n_hidden_gcn=512), g, "exceed")
    refused(pkg.JumpingKnowledgeNetwork(N, C, n_gcn=4, n_hidden_gcn=128), g, f"{DR.lds_bytes((128,) * 4)} bytes of LDS")
    refused(pkg.MLP(N, C, hidden=[8]), g, "MLP")
    from pytextgcn_amd.crossval import CrossValEGCN, CrossValGCN
    from pytextgcn_amd.sharded import ShardedGCN
    refused(CrossValGCN(N, C, 3, n_hidden_gcn=8), g, "K-member")
    refused(CrossValEGCN(N, C, 2, embedding_dim=8, n_hidden_gcn=8), g, "K-member")
    refused(pkg.PerLabelGCN(N, [3, 4], n_hidden_gcn=8), g, "K-member")
    refused(pkg.PerLabelMLP(N, [3, 4], [8]), g, "K-member")
    refused(ShardedGCN.__new__(ShardedGCN), g, "ShardedGCN", move=False)
    small = synth.word_doc_graph(60, 400, seed=1, device=cuda, n_classes=3, vocab_frac=0.5)
    parts = dict(edge_index=small.edge_index, edge_attr=small.edge_attr, n_vocab=small.n_vocab)
    refused(pkg.GCN(60, 3, n_gcn=3), pkg.Data(x=torch.eye(60, device=cuda), **parts), "dense")
    held = pkg.HierarchyFeatures(60, 30, classes=torch.zeros(30, dtype=torch.int64), n_classes=3)
    refused(pkg.JumpingKnowledgeNetwork(63, 3), pkg.Data(x=held, **parts), "HierarchyFeatures")
    ar = torch.arange(60, device=cuda)
    scaled = torch.sparse_coo_tensor(torch.stack([ar, ar]), torch.full((60,), 2.0, device=cuda), (60, 60)).coalesce()
    refused(pkg.GCN(60, 3, n_gcn=4), pkg.Data(x=scaled, **parts), "non-identity")
    # the two-layer classes keep refusing what they refused, in their own words
    with pytest.raises(NotImplementedError, match="JKN"):
        FoldIn(pkg.JumpingKnowledgeNetwork(N, C).to(cuda), g)
    with pytest.raises(NotImplementedError, match="n_gcn != 2"):
        FoldIn(pkg.GCN(N, C, n_gcn=3).to(cuda), g)
