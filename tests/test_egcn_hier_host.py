"""EGCN's fused front end on [I_N | H] features as far as a host without a GPU can see it: the switch, `embed_xw`'s
keywords, the dense-block helper, the argument checks of `tgcn_embed_xw_h*`.  The arithmetic is tested on the GPU
(tests/test_gpu_egcn_hier.py)."""
import inspect

import pytest
import torch

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, embed


def test_the_switch_exists_is_off_by_default_and_returns_the_previous_setting():
    assert pkg.enable_fused_hierarchy_embedding is pkg.models.enable_fused_hierarchy_embedding
    assert "enable_fused_hierarchy_embedding" in pkg.__all__
    assert pkg.models._FUSED_HIERARCHY is False
    assert pkg.enable_fused_hierarchy_embedding() is False
    try:
        assert pkg.enable_fused_hierarchy_embedding(False) is True
    finally:
        pkg.enable_fused_hierarchy_embedding(False)
    assert inspect.signature(pkg.enable_fused_hierarchy_embedding).parameters["on"].default is True


def test_embed_xw_has_the_trailing_keywords_with_their_defaults():
    for fn in (embed.embed_xw, embed.embed_xw_forward, embed.embed_xw_backward):
        params = list(inspect.signature(fn).parameters.values())
        assert [(q.name, q.default) for q in params[-2:]] == [("h", None), ("h_row0", 0)], fn
    assert [q.name for q in inspect.signature(embed.embed_xw).parameters.values()][:5] == ["E", "b", "W", "p", "seed"]


def _ih(n, entries, fh):
    ar = torch.arange(n)
    rows = torch.tensor([e[0] for e in entries], dtype=torch.long)
    cols = torch.tensor([e[1] for e in entries], dtype=torch.long)
    vals = torch.tensor([e[2] for e in entries], dtype=torch.float32)
    return torch.sparse_coo_tensor(torch.cat([torch.stack([ar, ar]), torch.stack([rows, cols + n])], 1),
                                   torch.cat([torch.ones(n), vals]), (n, n + fh))


def test_dense_block_helper():
    n, fh = 7, 3
    for entries, row0 in (([], n), ([(6, 2, 0.5), (6, 0, 0.25)], 6), ([(0, 1, 1.0), (4, 2, 0.5)], 0),
                          ([(3, 0, 0.125), (5, 1, 1.0)], 3)):
        h = conv.split_identity_block(_ih(n, entries, fh))
        assert h is not None and tuple(h.shape) == (n, fh)
        hd, got = conv.dense_hierarchy_block(h)
        assert got == row0 and tuple(hd.shape) == (n - row0, fh) and hd.dtype == torch.float32
        assert torch.equal(hd, h.to_dense()[row0:])
        assert conv.dense_hierarchy_block(h)[0] is hd        # cached per tensor object


def test_which_features_take_the_fused_path():
    n, fh = 10, 3
    x = _ih(n, [(8, 0, 1.0), (9, 2, 1.0)], fh)
    m = pkg.EGCN(n + fh, 3, embedding_dim=16, n_hidden_gcn=8, dropout=0.5).eval()
    assert not m.takes_fused_path(x)                         # off by default: the composition, as before
    was = pkg.enable_fused_hierarchy_embedding(True)
    try:
        assert m.takes_fused_path(x)
        assert not m.takes_fused_path(x.to_dense())
        assert not m.takes_fused_path(_ih(n, [(8, 0, 1.0)], embed.max_hierarchy_features() + 1))      # (also the wrong width)
        wide = pkg.EGCN(n + 129, 3, embedding_dim=16, n_hidden_gcn=8).eval()
        assert not wide.takes_fused_path(_ih(n, [(8, 0, 1.0)], 129))                                  # above the cap
        assert not pkg.EGCN(n + fh + 1, 3, embedding_dim=16).eval().takes_fused_path(x)               # in_features != N + Fh
        m.train()
        assert not m.takes_fused_path(x)                     # torch's random stream unless asked otherwise
        pkg.enable_fused_dropout(True)
        try:
            assert m.takes_fused_path(x)
        finally:
            pkg.enable_fused_dropout(False)
        m.eval()
        assert pkg.enable_fused_embedding(False) is True     # the master switch
        try:
            assert not m.takes_fused_path(x)
        finally:
            pkg.enable_fused_embedding(True)
    finally:
        pkg.enable_fused_hierarchy_embedding(was)


def test_cpu_features_raise_the_no_cpu_fallback_error():
    n, fh = 10, 3
    x = _ih(n, [(8, 0, 1.0)], fh)
    m = pkg.EGCN(n + fh, 3, embedding_dim=16, n_hidden_gcn=8).eval()
    ei = torch.tensor([[0, 1], [1, 0]])
    for on in (True, False):
        was = pkg.enable_fused_hierarchy_embedding(on)
        try:
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                m(pkg.Data(x=x, edge_index=ei, edge_attr=None))
        finally:
            pkg.enable_fused_hierarchy_embedding(was)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        embed.embed_xw(torch.zeros(6, 8 + fh), torch.zeros(6), torch.zeros(6, 4), h=torch.zeros(8, fh), h_row0=0)


def test_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.tgcn_abi_version() == 7       # the addition is purely additive
    cap = lib.tgcn_embed_xw_h_max_features()
    assert cap >= 128 and embed.max_hierarchy_features() == cap
    P = 0x1000                                                          # a non-NULL pointer nobody dereferences

    def fwd(E=P, lde=11, b=P, Eh=P, ldeh=11, Hd=P, ldh=3, h0=2, Fh=3, W=P, ldw=4, C=P, ldc=4, N=8, K=6, n=4, p=0.0, seed=None,
            row0=0):
        return lib.tgcn_embed_xw_h(E, lde, b, Eh, ldeh, Hd, ldh, h0, Fh, W, ldw, C, ldc, N, K, n, p, seed, row0, None)

    def bwd(E=P, lde=11, b=P, Eh=P, ldeh=11, Hd=P, ldh=3, h0=2, Fh=3, W=P, ldw=4, G=P, ldg=4, dE=P, ldde=11, db=P, dEh=P,
            lddeh=11, dW=P, lddw=4, N=8, K=6, n=4, p=0.0, seed=None, row0=0, ws=P, ws_bytes=1 << 30):
        return lib.tgcn_embed_xw_h_grad(E, lde, b, Eh, ldeh, Hd, ldh, h0, Fh, W, ldw, G, ldg, dE, ldde, db, dEh, lddeh, dW,
                                        lddw, N, K, n, p, seed, row0, ws, ws_bytes, None)

    def refused(status, *words):
        msg = lib.tgcn_last_error()
        assert status == _lib.E_INVALID, (status, msg)
        assert all(w in msg for w in words), msg
    for call, name in ((fwd, b"tgcn_embed_xw_h"), (bwd, b"tgcn_embed_xw_h_grad")):
        for arg in ("E", "b", "Eh", "Hd", "W"):
            refused(call(**{arg: None}), name, arg.encode() + b" is NULL")
        refused(call(K=0), name, b"K")
        refused(call(n=0), name, b"n >= 1")
        refused(call(N=-1), name, b"N >= 0")
        for Fh in (0, -2, cap + 1):
            refused(call(Fh=Fh, ldeh=1000, ldh=1000), name, b"Fh must be in")
        for h0 in (-1, 9):
            refused(call(h0=h0), name, b"h_row0 must be in [0, N]")
        for p in (-0.1, 1.0, 1.5, float("nan")):
            refused(call(p=p, seed=P), name, b"p must be in [0, 1)")
        refused(call(lde=7), name, b"lde")
        refused(call(ldeh=2), name, b"ldeh")
        refused(call(ldh=2), name, b"ldh")
        refused(call(ldw=3), name, b"ldw")
        refused(call(row0=-1), name, b"mask_row0")
    refused(fwd(C=None), b"C is NULL")
    refused(fwd(ldc=3), b"ldc")
    refused(bwd(G=None), b"G is NULL")
    refused(bwd(ldg=3), b"ldg")
    refused(bwd(ldde=7), b"ldde")
    refused(bwd(lddeh=2), b"lddeh")
    refused(bwd(lddw=3), b"lddw")
    refused(bwd(db=None), b"dE, db and dEh")
    refused(bwd(dEh=None), b"dE, db and dEh")
    refused(bwd(dE=None, db=None, dEh=None, dW=None), b"nothing to compute")
    need = lib.tgcn_embed_xw_h_grad_workspace_bytes(8, 6, 4, 3)
    assert need > 0
    refused(bwd(ws_bytes=need - 1), b"workspace")
    refused(bwd(ws=None), b"workspace")
    refused(bwd(dW=None, ws_bytes=0), b"workspace")          # dEh's partial sums need it as well
    with pytest.raises(ValueError):
        _lib.check(fwd(K=0))
    big = lib.tgcn_embed_xw_h_grad_workspace_bytes(20000, 2000, 100, 6)
    assert 0 < big < 20000 * 2000 * 4 // 8                   # partial sums: far from an N x K matrix
    assert big >= lib.tgcn_embed_xw_grad_workspace_bytes(20000, 2000, 100)
    assert lib.tgcn_embed_xw_h_grad_workspace_bytes(100, 5, 3, 0) == 0
    assert lib.tgcn_embed_xw_h_grad_workspace_bytes(100, 5, 3, cap + 1) == 0
    assert fwd(N=0, h0=0, E=None, Hd=None, C=None) == _lib.OK           # an empty product: nothing is enqueued
    refused(fwd(h0=8, Hd=None, E=None), b"E is NULL")                   # h_row0 == N: Hd is not looked at
