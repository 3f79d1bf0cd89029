"""CPU tests of `crossval.CrossValEGCN` (layout, initialisation, the bridge to M `EGCN`s, what it refuses), of the argument
checks of `tgcn_embed_xw_members*` and `tgcn_adam_member_rows*` -- every one returns before anything is enqueued, so no GPU
is needed -- and of the block map `MemberAdam` takes from the two network classes."""
import ctypes
import math

import pytest
import torch

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib
from pytextgcn_amd.crossval import CrossValEGCN, CrossValGCN, MemberAdam
from pytextgcn_amd.lib.models import CrossValEGCN as FromLibModels

N_IN, C, M, D, H = 50, 5, 3, 7, 6


def _net(**kw):
    torch.manual_seed(0)
    return CrossValEGCN(N_IN, C, M, embedding_dim=D, n_hidden_gcn=H, **kw)


def test_layout_and_init_bounds_per_member():
    assert FromLibModels is CrossValEGCN
    net = _net(dropout=[0.0, 0.3, 0.7])
    emb, first, second = net.layers
    assert isinstance(emb, pkg.models.EmbeddingLinear) and emb.in_features == N_IN and emb.out_features == M * D
    assert emb.weight.shape == (M * D, N_IN) and emb.bias.shape == (M * D,)
    assert first.weight.shape == (M * D, H) and first.bias.shape == (M * H,) and callable(first.plan)
    assert second.weight.shape == (H, M * 8) and second.class_counts == (C,) * M
    assert net.n_members == M and net.seg_stride == 8 and net.dropout == (0.0, 0.3, 0.7)
    assert [n for n, _ in net.named_parameters()] == [f"layers.{i}.{w}" for i in range(3) for w in ("weight", "bias")]
    lin = 1.0 / math.sqrt(N_IN)                  # nn.Linear(in, D): kaiming_uniform(a = sqrt 5) is U(-1/sqrt(in), 1/sqrt(in))
    glorot1, glorot2 = math.sqrt(6.0 / (D + H)), math.sqrt(6.0 / (H + C))
    for m in range(M):
        rows = slice(m * D, (m + 1) * D)
        for t, bound in ((emb.weight[rows], lin), (emb.bias[rows], lin), (first.weight[rows], glorot1),
                         (second.weight[:, m * 8:m * 8 + C], glorot2)):
            assert float(t.abs().max()) <= bound and float(t.abs().max()) > 0.5 * bound
        assert bool((second.weight[:, m * 8 + C:(m + 1) * 8] == 0).all())
    assert bool((first.bias == 0).all()) and bool((second.bias == 0).all())
    # a stacked glorot over [M D, h] would have the smaller bound sqrt(6 / (M D + h)): the members' is per member
    assert float(first.weight.abs().max()) > math.sqrt(6.0 / (M * D + H))


def test_round_trip_through_m_egcns_is_bit_exact():
    net = _net(dropout=[0.0, 0.3, 0.7])
    with torch.no_grad():
        net.layers[1].bias.uniform_(-1, 1)
        net.layers[2].bias.view(M, 8)[:, :C].uniform_(-1, 1)
    members = net.export_members()
    assert len(members) == M and all(isinstance(m, pkg.EGCN) and len(m.layers) == 3 for m in members)
    assert [m.dropout for m in members] == [0.0, 0.3, 0.7]
    assert members[1].layers[0].weight.shape == (D, N_IN) and members[1].layers[1].weight.shape == (D, H)
    back = CrossValEGCN.from_members(members)
    assert back.dropout == (0.0, 0.3, 0.7)
    for (n1, a), (n2, b) in zip(net.named_parameters(), back.named_parameters()):
        assert n1 == n2 and torch.equal(a, b), n1
    with torch.no_grad():                        # copies, not views
        members[0].layers[0].weight.add_(1.0)
    assert not torch.equal(net.layers[0].weight[:D], members[0].layers[0].weight)
    assert CrossValEGCN.from_members(members, dropout=0.25).dropout == 0.25


def test_what_it_refuses():
    for bad in (0, 65):
        with pytest.raises(ValueError, match="1..64 members"):
            CrossValEGCN(N_IN, C, bad, embedding_dim=D, n_hidden_gcn=H)
    with pytest.raises(ValueError, match="n_gcn"):
        CrossValEGCN(N_IN, C, M, embedding_dim=D, n_hidden_gcn=H, n_gcn=3)
    with pytest.raises(ValueError):
        CrossValEGCN(N_IN, C, M, embedding_dim=D, n_hidden_gcn=H, dropout=[0.1, 0.2])
    a = pkg.EGCN(N_IN, C, embedding_dim=D, n_hidden_gcn=H)
    for other in (pkg.EGCN(N_IN, C, embedding_dim=D + 1, n_hidden_gcn=H), pkg.EGCN(N_IN, C, embedding_dim=D, n_hidden_gcn=H + 1),
                  pkg.EGCN(N_IN, C + 1, embedding_dim=D, n_hidden_gcn=H), pkg.EGCN(N_IN + 1, C, embedding_dim=D, n_hidden_gcn=H)):
        with pytest.raises(ValueError, match="equal input, embedding, hidden and class width"):
            CrossValEGCN.from_members([a, other])
    with pytest.raises(ValueError, match="two-layer EGCNs"):
        CrossValEGCN.from_members([a, pkg.EGCN(N_IN, C, embedding_dim=D, n_gcn=3, n_hidden_gcn=H)])
    with pytest.raises(ValueError, match="no member"):
        CrossValEGCN.from_members([])
    from pytextgcn_amd.sharded import ShardedGraph
    with pytest.raises(ValueError, match="ShardedGraph"):
        _net()(object.__new__(ShardedGraph))     # the graph of ShardedGCN: refused before anything of it is read


def test_member_adam_block_map_for_both_network_classes():
    net = _net()
    emb, first, second = net.layers
    opt = MemberAdam(net, [0.1, 0.05, 0.01])
    assert opt._block == {id(emb.weight): D * N_IN, id(emb.bias): D, id(first.weight): D * H}
    assert opt._width == {id(first.bias): H, id(second.weight): 8, id(second.bias): 8}
    for p in net.parameters():                   # every tensor is M whole blocks
        if id(p) in opt._block:
            assert p.numel() == M * opt._block[id(p)]
        else:
            assert p.size(-1) == M * opt._width[id(p)]
    gcn = CrossValGCN(N_IN, C, M, n_hidden_gcn=H)
    opt = MemberAdam(gcn, 0.1)
    assert opt._block == {}
    assert opt._width == {id(gcn.layers[0].weight): H, id(gcn.layers[0].bias): H, id(gcn.layers[1].weight): 8,
                          id(gcn.layers[1].bias): 8}
    with pytest.raises(TypeError, match="MemberAdam updates a CrossValGCN"):
        MemberAdam(pkg.EGCN(N_IN, C, embedding_dim=D, n_hidden_gcn=H), 0.1)
    with pytest.raises(ValueError, match="2 learning rates for 3 members"):
        MemberAdam(net, [0.1, 0.2])


# ----------------------------------------------------------------------------------------------------------------------
# the argument checks of the C ABI: TGCN_E_INVALID / TGCN_E_WORKSPACE before anything is enqueued
# ----------------------------------------------------------------------------------------------------------------------
N, K, n, MM = 10, 4, 3, 2
_HOST = (ctypes.c_float * 64)()
P = ctypes.addressof(_HOST)                      # a non-NULL pointer that no call reads: every call below is refused


def _rates(*v):
    return (ctypes.c_double * len(v))(*v)


def _fwd(**kw):
    a = dict(E=P, lde=N, b=P, Eh=None, ldeh=0, Hd=None, ldh=0, h_row0=0, Fh=0, W=P, ldw=n, C=P, ldc=MM * n, N=N, K=K, n=n,
             M=MM, p=_rates(0.0, 0.5), seeds=None, row0=0)
    a.update(kw)
    return _lib.load().tgcn_embed_xw_members(a["E"], a["lde"], a["b"], a["Eh"], a["ldeh"], a["Hd"], a["ldh"], a["h_row0"],
                                             a["Fh"], a["W"], a["ldw"], a["C"], a["ldc"], a["N"], a["K"], a["n"], a["M"],
                                             a["p"], a["seeds"], a["row0"], None)


def _grad(**kw):
    a = dict(E=P, lde=N, b=P, Eh=None, ldeh=0, Hd=None, ldh=0, h_row0=0, Fh=0, W=P, ldw=n, G=P, ldg=MM * n, dE=P, ldde=N, db=P,
             dEh=None, lddeh=0, dW=P, lddw=n, N=N, K=K, n=n, M=MM, p=_rates(0.0, 0.5), seeds=None, row0=0, ws=P, ws_bytes=0)
    a.update(kw)
    return _lib.load().tgcn_embed_xw_members_grad(
        a["E"], a["lde"], a["b"], a["Eh"], a["ldeh"], a["Hd"], a["ldh"], a["h_row0"], a["Fh"], a["W"], a["ldw"], a["G"],
        a["ldg"], a["dE"], a["ldde"], a["db"], a["dEh"], a["lddeh"], a["dW"], a["lddw"], a["N"], a["K"], a["n"], a["M"], a["p"],
        a["seeds"], a["row0"], a["ws"], a["ws_bytes"], None)


HIER = dict(Eh=P, ldeh=N + 2, Hd=P, ldh=2, Fh=2, h_row0=3, lde=N + 2)
BAD = [("n_members=0", dict(M=0)), ("n_members=65", dict(M=65, p=_rates(*[0.0] * 65))),
       ("rate=1", dict(p=_rates(0.0, 1.0))), ("rate<0", dict(p=_rates(-0.1, 0.0))), ("rate nan", dict(p=_rates(0.0, float("nan")))),
       ("p_host NULL", dict(p=None)), ("lde", dict(lde=N - 1)), ("ldw", dict(ldw=n - 1)),
       ("E NULL", dict(E=None)), ("b NULL", dict(b=None)), ("W NULL", dict(W=None)),
       ("Fh=-1", dict(HIER, Fh=-1)), ("Fh=129", dict(HIER, Fh=129, ldeh=N + 129, ldh=129, lde=N + 129)),
       ("h_row0=-1", dict(HIER, h_row0=-1)), ("h_row0=N+1", dict(HIER, h_row0=N + 1)),
       ("Eh NULL", dict(HIER, Eh=None)), ("Hd NULL", dict(HIER, Hd=None)), ("ldeh", dict(HIER, ldeh=1)), ("ldh", dict(HIER, ldh=1)),
       ("N<0", dict(N=-1)), ("K=0", dict(K=0)), ("n=0", dict(n=0)), ("mask_row0<0", dict(row0=-1))]


@pytest.mark.parametrize("what,kw", BAD, ids=[w for w, _ in BAD])
def test_invalid_arguments_of_both_member_calls(what, kw):
    lib = _lib.load()
    assert _fwd(**kw) == _lib.E_INVALID, what
    assert b"tgcn_embed_xw_members" in lib.tgcn_last_error()
    grad_kw = dict(kw)
    if grad_kw.get("Fh", 0) != 0:
        grad_kw.setdefault("dEh", P)
        grad_kw.setdefault("lddeh", N + 2)
    assert _grad(**grad_kw) == _lib.E_INVALID, what
    assert b"tgcn_embed_xw_members_grad" in lib.tgcn_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.E_INVALID)


def test_invalid_arguments_of_one_call_alone():
    lib = _lib.load()
    assert _fwd(ldc=MM * n - 1) == _lib.E_INVALID and b"ldc" in lib.tgcn_last_error()
    assert _fwd(ldc=n) == _lib.E_INVALID                                    # one member's width is not enough
    assert _fwd(C=None) == _lib.E_INVALID and b"C is NULL" in lib.tgcn_last_error()
    assert _grad(ldg=MM * n - 1) == _lib.E_INVALID and b"ldg" in lib.tgcn_last_error()
    assert _grad(G=None) == _lib.E_INVALID
    assert _grad(ldde=N - 1) == _lib.E_INVALID and _grad(lddw=n - 1) == _lib.E_INVALID
    assert _grad(db=None) == _lib.E_INVALID and b"dE and db" in lib.tgcn_last_error()           # dE without db
    assert _grad(dE=None) == _lib.E_INVALID                                                      # db without dE
    assert _grad(dE=None, db=None, dW=None) == _lib.E_INVALID and b"nothing to compute" in lib.tgcn_last_error()
    hier = dict(HIER, dEh=P, lddeh=N + 2, ldde=N + 2)
    assert _grad(**dict(hier, dEh=None)) == _lib.E_INVALID and b"dEh" in lib.tgcn_last_error()   # dE without dEh
    assert _grad(**dict(hier, lddeh=1)) == _lib.E_INVALID
    # a short workspace has a status of its own
    need = lib.tgcn_embed_xw_members_grad_workspace_bytes(N, K, n, 0, MM)
    assert need > 0 and need == MM * lib.tgcn_embed_xw_grad_workspace_bytes(N, K, n)
    assert lib.tgcn_embed_xw_members_grad_workspace_bytes(N, K, n, 2, MM) == MM * lib.tgcn_embed_xw_h_grad_workspace_bytes(N, K, n, 2)
    assert _grad(ws_bytes=need - 1) == _lib.E_WORKSPACE and _grad(ws=None, ws_bytes=need) == _lib.E_WORKSPACE
    assert _grad(**dict(hier, ws_bytes=16)) == _lib.E_WORKSPACE
    for bad in (dict(N=-1), dict(K=0), dict(n=0), dict(Fh=-1), dict(Fh=129), dict(M=0), dict(M=65)):
        a = dict(N=N, K=K, n=n, Fh=0, M=MM)
        a.update(bad)
        assert lib.tgcn_embed_xw_members_grad_workspace_bytes(a["N"], a["K"], a["n"], a["Fh"], a["M"]) == 0
    assert lib.tgcn_abi_version() == 7


def test_adam_member_rows_argument_errors():
    lib = _lib.load()
    lr = _rates(0.1, 0.1, 0.1)
    A = (P + 15) & ~15                           # 16-byte aligned
    args = lambda n_, block, k, lrs=lr, p=A: (p, A, A, A, None, n_, block, k, lrs, 0.9, 0.999, 1e-8, 0.0)
    for bad in (args(13, 4, 3), args(12, 4, 0), args(12, 4, 65), args(12, 4, 3, None), args(-3, -1, 3), args(12, 4, 3, lr, A + 4),
                args(12, 4, 3, lr, None)):
        assert lib.tgcn_adam_member_rows(*bad, 1, None) == _lib.E_INVALID
        assert b"tgcn_adam_member_rows" in lib.tgcn_last_error()
    assert lib.tgcn_adam_member_rows(*args(12, 4, 3), 0, None) == _lib.E_INVALID                 # step < 1
    assert lib.tgcn_adam_member_rows_capturable(*args(12, 4, 3), None, None, None) == _lib.E_INVALID
    assert lib.tgcn_adam_member_rows(None, None, None, None, None, 0, 0, 3, lr, 0.9, 0.999, 1e-8, 0.0, 1, None) == _lib.OK
