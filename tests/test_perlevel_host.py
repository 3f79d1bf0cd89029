"""The hierarchy features of the per-level strategy as far as a host without a GPU can see them: `HierarchyFeatures` and
its sparse form, the helpers of `pytextgcn_amd.perlevel`, the routing of `conv.features_times`, the argument checks of
`tgcn_hier_xw*`.  The arithmetic is tested on the GPU (tests/test_gpu_perlevel.py)."""
import pytest
import torch

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, hier, perlevel, synth
from pytextgcn_amd.hier import HierarchyFeatures

import _perlevel_ref as R


def _transformer(n_vocab, n_docs):
    t2g = pkg.Text2GraphTransformer()
    t2g.n_vocabs_, t2g.n_docs_, t2g.n_nodes_ = n_vocab, n_docs, n_vocab + n_docs
    return t2g


def _same_sparse(a, b):
    assert a.is_sparse and a.is_coalesced() and a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values())


def test_to_sparse_is_node_feats_entry_for_entry():
    n_vocab, n_docs, Fh = 7, 5, 3
    t2g = _transformer(n_vocab, n_docs)
    cls = torch.tensor([2, 0, 1, 1, 2])
    onehot = HierarchyFeatures(n_vocab + n_docs, n_vocab, classes=cls, n_classes=Fh)
    _same_sparse(onehot.to_sparse(), t2g.node_feats(R.one_hot(cls, Fh).numpy()))
    assert onehot.to_sparse() is onehot.to_sparse()                     # built once
    Hd = torch.softmax(torch.randn(n_docs, Fh, generator=torch.Generator().manual_seed(1)), dim=1)
    Hd[1, 2] = 0.0                                                      # an exact zero is no entry, as th.nonzero has it
    dense = HierarchyFeatures(n_vocab + n_docs, n_vocab, dense=Hd)
    _same_sparse(dense.to_sparse(), t2g.node_feats(Hd.numpy()))
    # ids that select nothing leave their rows empty; the densified rows say the same
    holes = HierarchyFeatures(n_vocab + n_docs, n_vocab, classes=torch.tensor([2, -1, 1, Fh, 0]), n_classes=Fh)
    want = R.one_hot(torch.tensor([2, -1, 1, Fh, 0]), Fh)
    _same_sparse(holes.to_sparse(), t2g.node_feats(want.numpy()))
    assert torch.equal(holes.dense_block(), want) and holes.dense_block() is holes.dense_block()
    assert torch.equal(conv.split_identity_block(holes.to_sparse()).to_dense()[n_vocab:], want)


def test_shape_protocol():
    f = HierarchyFeatures(12, 7, classes=torch.tensor([0, 1, 2, 1, 0]), n_classes=4)
    assert f.shape == (12, 16) and f.size() == (12, 16) and f.size(0) == 12 and f.size(1) == 16 and f.dim() == 2
    assert f.is_sparse is False and f.is_cuda is False and f.device == torch.device("cpu") and f.dtype == torch.float32
    assert f.n_features == f.n_classes == 4 and f.classes.dtype == torch.int32 and f.dense is None
    assert HierarchyFeatures(12, 7, classes=[0, 1, 2, 1, 0]).n_features == 3          # the largest id + 1
    d = HierarchyFeatures(12, 7, dense=torch.zeros(5, 6))
    assert d.shape == (12, 18) and d.classes is None and d.n_features == 6
    assert f.to("cpu") is f and d.to(torch.device("cpu")) is d
    assert HierarchyFeatures(4, 4, classes=torch.empty(0, dtype=torch.long), n_classes=2).size(1) == 6   # nobody has a row


def test_constructor_refusals():
    cls, Hd = torch.tensor([0, 1, 0]), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="exactly one"):
        HierarchyFeatures(5, 2, classes=cls, dense=Hd)
    with pytest.raises(ValueError, match="exactly one"):
        HierarchyFeatures(5, 2)
    for kw in ({"classes": cls}, {"dense": Hd}):
        with pytest.raises(ValueError, match="rows given"):
            HierarchyFeatures(6, 2, **kw)                                # N - h_row0 = 4 rows expected
    for h_row0 in (-1, 6):
        with pytest.raises(ValueError, match="h_row0"):
            HierarchyFeatures(5, h_row0, classes=cls)
    with pytest.raises(TypeError):
        HierarchyFeatures(5, 2, classes=torch.tensor([0.0, 1.0, 0.0]))
    with pytest.raises(TypeError):
        HierarchyFeatures(5, 2, dense=torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(TypeError):
        HierarchyFeatures(5, 2, dense=torch.zeros(3))


def test_data_moves_the_features_and_the_helpers_share_the_graph():
    g = synth.word_doc_graph(60, 400, seed=3, n_classes=6)
    n_docs = 60 - g.n_vocab
    y_top = (g.y[g.n_vocab:] // 3)
    feats = perlevel.one_hot_hierarchy(g, y_top, n_classes=2)
    assert feats.h_row0 == g.n_vocab and feats.shape == (60, 62) and feats.classes.numel() == n_docs
    g2 = perlevel.with_hierarchy(g, feats, y=g.y + 0)
    assert g2.x is feats and g2.edge_index is g.edge_index and g2.edge_attr is g.edge_attr and g2.train_mask is g.train_mask
    assert g2.y is not g.y and g.x is not feats and g2.n_vocab == g.n_vocab and g2.num_nodes == 60
    assert perlevel.with_hierarchy(g, feats).y is g.y
    moved = g2.to("cpu")
    assert moved is g2 and isinstance(g2.x, HierarchyFeatures)          # `Data.apply` goes through the features' own `to`
    with pytest.raises(ValueError, match="documents"):
        perlevel.one_hot_hierarchy(g, y_top[:-1])
    with pytest.raises(ValueError, match="rows"):
        perlevel.with_hierarchy(g, HierarchyFeatures(61, g.n_vocab, classes=torch.zeros(61 - g.n_vocab, dtype=torch.long)))
    assert "different vocabularies" in perlevel.__doc__


def test_which_weights_take_the_kernels_and_no_cpu_fallback():
    f = HierarchyFeatures(10, 6, classes=torch.tensor([0, 1, 2, 1]), n_classes=3)
    w = torch.zeros(13, 8)
    assert hier.takes(f, w) and hier.takes(f, torch.zeros(13, 12)[:, :8])                 # row-major, any row stride
    assert not hier.takes(f, torch.zeros(8, 13).t())                                      # an nn.Linear weight, transposed
    assert not hier.takes(f, torch.zeros(12, 8)) and not hier.takes(f, w.double())
    wide = HierarchyFeatures(10, 6, dense=torch.zeros(4, hier.max_features() + 1))
    assert not hier.takes(wide, torch.zeros(10 + hier.max_features() + 1, 8))             # above the cap: the composition
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hier.xw(f, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.features_times(f, w, 13)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv.features_times(f, torch.zeros(8, 13).t(), 13)                                # the sparse road, same error
    with pytest.raises(ValueError, match="features"):
        conv.features_times(f, w, 14)
    with pytest.raises(TypeError):
        hier.xw(f.to_sparse(), w)
    m = pkg.EGCN(13, 3, embedding_dim=16, n_hidden_gcn=8, dropout=0.5).eval()
    assert pkg.models._FUSED_HIERARCHY is False and m.takes_fused_path(f)                 # the type selects the product
    assert not m.train().takes_fused_path(f)                                              # torch's random stream unless asked
    assert not pkg.EGCN(10 + 129, 3, embedding_dim=16).eval().takes_fused_path(HierarchyFeatures(10, 6, dense=torch.zeros(4, 129)))
    assert pkg.enable_fused_embedding(False) is True
    try:
        assert not m.eval().takes_fused_path(f)
    finally:
        pkg.enable_fused_embedding(True)


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.tgcn_abi_version() == 7       # the addition is purely additive
    assert lib.tgcn_hier_max_features() == 128 == hier.max_features() == lib.tgcn_embed_xw_h_max_features()
    P = 0x1000                                                          # a non-NULL pointer nobody dereferences
    ONEHOT, DENSE = _lib.HIER_ONEHOT, _lib.HIER_DENSE

    def fwd(W=P, ldw=4, form=ONEHOT, cls=P, Hd=P, ldh=3, h0=2, Fh=3, C=P, ldc=4, N=8, F=4):
        return lib.tgcn_hier_xw(W, ldw, form, cls, Hd, ldh, h0, Fh, C, ldc, N, F, None)

    def bwd(G=P, ldg=4, form=ONEHOT, cls=P, h0=2, Fh=3, dW=P, lddw=4, N=8, F=4, ws=P, ws_bytes=1 << 30):
        return lib.tgcn_hier_xw_grad(G, ldg, form, cls, h0, Fh, dW, lddw, N, F, ws, ws_bytes, None)

    def refused(status, *words):
        msg = lib.tgcn_last_error()
        assert status == _lib.E_INVALID, (status, msg)
        assert all(w in msg for w in words), msg
    for call, name in ((fwd, b"tgcn_hier_xw"), (bwd, b"tgcn_hier_xw_grad")):
        refused(call(cls=None), name, b"cls is NULL")
        refused(call(N=-1), name, b"N >= 0")
        refused(call(F=0), name, b"F >= 1")
        for Fh in (0, -2, 129):
            refused(call(Fh=Fh), name, b"Fh must be in")
        for h0 in (-1, 9):
            refused(call(h0=h0), name, b"h_row0 must be in [0, N]")
        for form in (-1, 2, 7):
            refused(call(form=form), name, b"unknown form")
    refused(fwd(W=None), b"W is NULL")
    refused(fwd(C=None), b"C is NULL")
    refused(fwd(form=DENSE, Hd=None), b"Hd is NULL")
    refused(fwd(ldw=3), b"ldw")
    refused(fwd(ldc=3), b"ldc")
    refused(fwd(form=DENSE, ldh=2), b"ldh")
    refused(bwd(G=None), b"G is NULL")
    refused(bwd(dW=None), b"dW is NULL")
    refused(bwd(ldg=3), b"ldg")
    refused(bwd(lddw=3), b"lddw")
    need = lib.tgcn_hier_xw_grad_workspace_bytes(8, 4, 3, 2, ONEHOT)
    assert need > 0
    refused(bwd(ws_bytes=need - 1), b"workspace")
    refused(bwd(ws=None), b"workspace")
    with pytest.raises(ValueError):
        _lib.check(fwd(F=0))
    # partial sums of [slices, Fh, F]: their size does not follow N
    big = lib.tgcn_hier_xw_grad_workspace_bytes(2_000_000, 100, 6, 200_000, ONEHOT)
    assert 0 < big <= (1 << 24) + 1024 * 6 * 100 * 4 and big < 2_000_000 * 100 * 4 // 16
    assert lib.tgcn_hier_xw_grad_workspace_bytes(8, 4, 3, 2, DENSE) == 0           # dW[N:] is the caller's gemm_tn
    assert lib.tgcn_hier_xw_grad_workspace_bytes(8, 4, 3, 8, ONEHOT) == 0          # nobody has a class
    assert lib.tgcn_hier_xw_grad_workspace_bytes(8, 4, 129, 2, ONEHOT) == 0
    assert fwd(N=0, h0=0, W=None, cls=None, C=None) == _lib.OK          # an empty product: nothing is enqueued
    refused(fwd(h0=8, cls=None, W=None), b"W is NULL")                  # h_row0 == N: cls is not looked at
    refused(fwd(form=ONEHOT, Hd=None, ldh=0, W=None), b"W is NULL")     # ONEHOT: Hd and ldh are not looked at
    refused(bwd(form=DENSE, cls=None, ws=None, ws_bytes=0, G=None), b"G is NULL")   # DENSE: neither cls nor a workspace
