"""Fold-in on the CPU: `Text2GraphTransformer.transform`, the numpy restatement of the definition (tests/_foldin_ref.py)
against the CPU oracles on `extended_graph`, the completeness of the kernel sweep's case table (tests/_foldin_cases.py) and
the argument checks of `tgcn_foldin_two_layer`, which need no GPU."""
import os
import re

import numpy as np
import pytest
import torch
from scipy import sparse as sp

import _foldin_cases as fc
import _foldin_ref as R
from _egcn_ref import EGCNRef
from oracle import gcn_oracle as O
import pytextgcn_amd as pkg
from pytextgcn_amd import synth, text2graph
from pytextgcn_amd.inductive import extended_graph

PARITY = 1e-5                     # the project's parity bar (BASELINE.json): max-norm relative


# ---- Text2GraphTransformer.transform -----------------------------------------------------------------------------------
def _fitted(monkeypatch, docs):
    """fit_transform without a GPU: the word-word builder is replaced by one that finds no pair (the document-word edges
    and their TF-IDF weights, which `transform` is held against, do not depend on it)."""
    monkeypatch.setattr(text2graph.graphbuilder, "compute_word_word_edges",
                        lambda *a, **k: (np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.float32)))
    t = pkg.Text2GraphTransformer(min_df=5, window_size=20)
    return t, t.fit_transform(docs, y=[0] * len(docs))


def test_transform_of_the_corpus_is_the_document_word_edge_weights_bit_for_bit(monkeypatch):
    docs, _ = synth.synthetic_corpus(n_docs=1000, vocab_size=2000, n_classes=4, seed=44)      # config c1's corpus
    t, g = _fitted(monkeypatch, docs)
    m = t.transform(docs)
    V, D = t.n_vocabs_, len(docs)
    assert sp.isspmatrix_csr(m) and m.shape == (D, V) and m.dtype == np.float32 and m.has_sorted_indices
    n_dw = g.edge_index.size(1) // 2                    # [doc -> word | word -> doc], no word-word edges here
    src, dst = g.edge_index[0, :n_dw].numpy(), g.edge_index[1, :n_dw].numpy()
    assert np.array_equal(src - V, np.repeat(np.arange(D), np.diff(m.indptr))) and np.array_equal(dst, m.indices)
    assert np.array_equal(g.edge_attr[:n_dw].numpy().view(np.int32), m.data.view(np.int32))
    assert np.array_equal(g.edge_attr[n_dw:].numpy().view(np.int32), m.data.view(np.int32))
    # a subset, in another order, is the same rows: a document's weights do not depend on its batch
    pick = [7, 3, 500]
    sub = t.transform([docs[i] for i in pick])
    assert (sub != m[pick]).nnz == 0


def test_transform_drops_unknown_words_and_needs_a_fit(monkeypatch):
    from sklearn.exceptions import NotFittedError
    with pytest.raises(NotFittedError):
        pkg.Text2GraphTransformer().transform(["a document"])
    docs, _ = synth.synthetic_corpus(n_docs=200, vocab_size=300, n_classes=2, seed=3)
    t, _ = _fitted(monkeypatch, docs)
    known = sorted(t.vocabulary)[0]
    m = t.transform(["zzzunknownzzz qqqneverseenqqq", f"{known} zzzunknownzzz", ""])
    assert m.shape == (3, t.n_vocabs_) and np.diff(m.indptr).tolist() == [0, 1, 0]
    assert m.indices.tolist() == [t.vocabulary[known]] and m.data.tolist() == [1.0]      # one word: unit L2 norm


# ---- the restatement against the CPU oracles on the extended graph ------------------------------------------------------
NEW_ROW_WORDS = (0, 1, 3, 17, 40)


@pytest.fixture(scope="module")
def small():
    g = synth.word_doc_graph(70, 600, seed=5, device="cpu", n_classes=3, vocab_frac=0.58)
    V = int(g.n_vocab)
    assert V == 40 and g.x.size(0) == 70
    rng = np.random.default_rng(11)
    rows = []
    for n in NEW_ROW_WORDS:
        cols = np.sort(rng.choice(V, size=n, replace=False))
        v = rng.random(n) * 0.95 + 0.05
        rows.append((cols, (v / max(np.sqrt((v * v).sum()), 1e-30)).astype(np.float32)))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])])
    tfidf = sp.csr_matrix((np.concatenate([v for _, v in rows]), np.concatenate([c for c, _ in rows]), indptr),
                          shape=(len(rows), V), dtype=np.float32)
    return g, tfidf, extended_graph(g, tfidf)


def test_extended_graph_is_the_definition_as_a_graph(small):
    g, tfidf, ge = small
    N, B, V, E = 70, len(NEW_ROW_WORDS), 40, g.edge_index.size(1)
    assert ge.x.is_sparse and tuple(ge.x.shape) == (N + B, N) and ge.x._nnz() == N
    assert torch.equal(ge.x.to_dense()[:N], torch.eye(N)) and not ge.x.to_dense()[N:].any()
    assert torch.equal(ge.edge_index[:, :E], g.edge_index) and torch.equal(ge.edge_attr[:E], g.edge_attr)
    new = ge.edge_index[:, E:]
    assert new.size(1) == tfidf.nnz and bool((new[0] < V).all())                        # word -> new document only
    assert new[1].tolist() == (np.repeat(np.arange(B), np.diff(tfidf.indptr)) + N).tolist()
    assert new[0].tolist() == tfidf.indices.tolist() and torch.equal(ge.edge_attr[E:], torch.from_numpy(tfidf.data))
    for k in ("train_mask", "val_mask", "test_mask"):
        assert torch.equal(getattr(ge, k)[:N], getattr(g, k)) and not getattr(ge, k)[N:].any()
    assert torch.equal(ge.y[:N], g.y) and not ge.y[N:].any() and ge.n_vocab == V


def _randomise(model, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:                           # biases start at zero: give them a value the test can see
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
    return model.eval()


def _check_rows(z, want):
    print(f"restatement against the oracle's new rows: {R.rel_err(z, want):.2e} max-norm relative; row by row "
          f"{[f'{R.rel_err(z[i], want[i]):.1e}' for i in range(len(NEW_ROW_WORDS))]}")
    assert R.rel_err(z, want) < PARITY
    for i, n in enumerate(NEW_ROW_WORDS):              # and row by row: a short row must not hide behind a long one
        assert R.rel_err(z[i], want[i]) < PARITY, (n, R.rel_err(z[i], want[i]))


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_restatement_matches_the_gcn_oracle_on_the_extended_graph(small, relu):
    g, tfidf, ge = small
    N, V = 70, 40
    torch.manual_seed(2)
    model = _randomise(O.GCNOracle(N, 3, n_hidden_gcn=16), 7)
    with torch.no_grad():
        base, h1 = R.gcn_forward(model, g, relu)
        ext, _ = R.gcn_forward(model, ge, relu)
        if not relu:
            assert torch.equal(base, model(g))
        # the one-directional edges leave every old row as it was: bit for bit
        assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))
        W1, W2 = model.layers[0].weight, model.layers[1].weight
        P = (h1 @ W2)[:V]
        z, _ = R.foldin(tfidf.indptr, tfidf.indices, tfidf.data, R.word_dis(g), R.REFERENCE, W1[:V].numpy(), None,
                        model.layers[0].bias.numpy(), R.ACT_RELU if relu else R.ACT_NONE, P.numpy(), W2.numpy(),
                        model.layers[1].bias.numpy(), sum_dtype=np.float32)
    _check_rows(z, ext[N:].numpy())


def test_restatement_matches_the_egcn_reference_on_the_extended_graph(small):
    g, tfidf, ge = small
    N, V = 70, 40
    torch.manual_seed(3)
    model = _randomise(EGCNRef(N, 3, embedding_dim=24, n_hidden_gcn=16), 9)
    with torch.no_grad():
        base, ext = model(g), model(ge)
        assert torch.equal(ext[:N].view(torch.int32), base.view(torch.int32))
        lin, first, second = model.layers
        act = torch.selu(lin.weight.t() + lin.bias)                    # the Linear on identity features, [N, K]
        T1 = (act @ first.weight)[:V]
        s1 = torch.selu(lin.bias) @ first.weight                         # a new document's feature row is empty
        h1 = first(act, g.edge_index, g.edge_attr)
        P = (h1 @ second.weight)[:V]
        z, _ = R.foldin(tfidf.indptr, tfidf.indices, tfidf.data, R.word_dis(g), R.REFERENCE, T1.numpy(), s1.numpy(),
                        first.bias.numpy(), R.ACT_NONE, P.numpy(), second.weight.numpy(), second.bias.numpy(),
                        sum_dtype=np.float32)
    _check_rows(z, ext[N:].numpy())


def test_degree_rules_of_the_restatement():
    """reference: one fp32 accumulator in order, the 1.0 last -- a sum whose order matters shows it; accurate: float64."""
    t = np.array([2.0 ** 24, 1.0, 1.0, 1.0], dtype=np.float32)
    assert R.doc_dis(t, R.REFERENCE) == np.float32(1.0) / np.sqrt(np.float32(2.0 ** 24))          # the ones are absorbed
    assert R.doc_dis(t, R.ACCURATE) == np.float32(1.0) / np.sqrt(np.float32(2.0 ** 24 + 4.0))
    assert R.doc_dis(np.zeros(0, dtype=np.float32), R.REFERENCE) == 1.0 == R.doc_dis(np.zeros(0, dtype=np.float32), R.ACCURATE)
    assert R.doc_dis(np.array([3.0], dtype=np.float32), R.REFERENCE) == 0.5
    long = np.full(1100, 15.0 / 1100, dtype=np.float64).astype(np.float32)
    assert abs(float(R.doc_dis(long, R.ACCURATE)) - 0.25) < 1e-6


# ---- the case table ----------------------------------------------------------------------------------------------------
def test_every_leaf_and_every_option_of_the_sweep_is_hit():
    ints, floats = fc.int_cases(), fc.float_cases()
    for c in ints + floats:
        assert 1 <= c.h <= fc.MAX_HIDDEN and 1 <= c.C <= fc.MAX_CLASSES and fc.leaf_of(c.h, c.C) in fc.LEAVES
    for family in (ints, floats):
        hit = {fc.leaf_of(c.h, c.C) for c in family}
        skipped = [leaf for leaf in fc.LEAVES if leaf not in hit]
        assert len(skipped) <= 0, f"leaves without a case: {skipped}"              # cap: zero skipped
    assert len({fc.case_id(c) for c in ints + floats}) == len(ints + floats)
    for leaf in fc.LEAVES:
        mine = [c for c in ints if fc.leaf_of(c.h, c.C) == leaf]
        assert {c.layout for c in mine} == {"tight", "padded", "shared"}, leaf
        assert {c.s1 for c in mine} == {False, True} and {c.act for c in mine} == {0, 1}, leaf
        assert {c.mode for c in mine} == {R.REFERENCE, R.ACCURATE}, leaf
        assert {(c.pred, c.hidden) for c in mine} == {(False, False), (False, True), (True, False), (True, True)}, leaf
        full = [c for c in mine if c.n_docs == fc.DOCS_PER_WORKGROUP + 1]
        assert full and all(fc.row_lengths(c)[:8] == list(fc.ROW_LENGTHS) for c in full), leaf
    tile, stride = fc.DOCS_PER_WORKGROUP, fc.DOCS_PER_WORKGROUP * fc.WORKGROUP_CAP
    assert {0, 1, tile - 1, tile, tile + 1, 2 * stride + 1} <= {c.n_docs for c in ints}
    assert {(c.h, c.C) for c in ints} >= {(1, 1), (256, 128), (63, 65), (200, 64), (100, 128), (64, 64)}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tgcn.h")).read()
    assert int(re.search(r"#define TGCN_FOLDIN_DOCS_PER_WORKGROUP (\d+)", header).group(1)) == tile
    assert int(re.search(r"#define TGCN_FOLDIN_WORKGROUP_CAP (\d+)", header).group(1)) == fc.WORKGROUP_CAP


def test_exact_family_keeps_every_partial_sum_below_2_to_24():
    """... in units of the document's finest dyadic step, so that fp32 in any order is exact; rows hold first / last /
    duplicate columns.  (The large batch is checked where it runs, on the GPU: its rows are the short ones checked here.)"""
    seen_dup = seen_first = seen_last = False
    for c in fc.int_cases():
        if c.n_docs > 4 * fc.DOCS_PER_WORKGROUP:
            continue
        o, ref = fc.operands(c), fc.reference(c)
        assert ref["units"] < 2 ** 24, (fc.case_id(c), ref["units"])
        assert set(np.unique(ref["dis_d"]).tolist()) <= {1.0, 0.5, 0.25}
        assert o["col"].size == 0 or (0 <= o["col"].min() and o["col"].max() < c.n_vocab)
        for d in range(c.n_docs):
            cj = o["col"][o["rowptr"][d]:o["rowptr"][d + 1]]
            seen_dup |= cj.size != np.unique(cj).size
            seen_first |= bool(cj.size and cj[0] == 0)
            seen_last |= bool(cj.size and cj[-1] == c.n_vocab - 1)
    assert seen_dup and seen_first and seen_last


# ---- argument errors need no GPU ----------------------------------------------------------------------------------------
def test_argument_errors_do_not_need_a_gpu():
    from pytextgcn_amd import _lib
    lib = _lib.load()
    assert lib.tgcn_foldin_max_hidden() == fc.MAX_HIDDEN >= 256 and lib.tgcn_foldin_max_classes() == fc.MAX_CLASSES >= 128
    A = 1 << 20                                          # a 16-byte aligned address nothing will ever dereference
    good = dict(n_docs=3, rowptr=A, col=A, val=A, n_vocab=10, dis=A, degree_sum=_lib.DEGREE_REFERENCE, T1=A, ldt1=64, h=64,
                s1=None, b1=A, act=_lib.ACT_NONE, P=A, ldp=8, C=8, W2=A, ldw2=8, b2=A, logits=A, ldl=8, pred=None,
                hidden=None, ldh=0, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.tgcn_foldin_two_layer(*[a[k] for k in good])

    bad = [dict(rowptr=None), dict(col=None), dict(val=None), dict(dis=None), dict(T1=None), dict(b1=None), dict(P=None),
           dict(W2=None), dict(b2=None), dict(logits=None),
           dict(h=0), dict(h=fc.MAX_HIDDEN + 1, ldt1=512), dict(C=0), dict(C=fc.MAX_CLASSES + 1, ldp=256, ldw2=256, ldl=256),
           dict(ldt1=66), dict(ldt1=60), dict(ldp=6), dict(ldp=4), dict(ldw2=10), dict(ldl=9), dict(ldl=4),
           dict(hidden=A, ldh=60), dict(hidden=A, ldh=66),
           dict(T1=A + 4), dict(P=A + 8), dict(W2=A + 4), dict(b1=A + 4), dict(b2=A + 12), dict(s1=A + 4), dict(logits=A + 4),
           dict(hidden=A + 4, ldh=64),
           dict(act=2), dict(act=-1), dict(degree_sum=2), dict(degree_sum=-1), dict(n_docs=-1), dict(n_vocab=0),
           dict(n_vocab=1 << 31)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        assert b"tgcn_foldin_two_layer" in lib.tgcn_last_error()
    # an empty batch launches nothing, whatever the pointers are
    assert call(n_docs=0, rowptr=None, col=None, val=None, logits=None) == _lib.OK
    with pytest.raises(ValueError):
        _lib.check(call(h=0))
