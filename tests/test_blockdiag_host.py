"""Host tests of the one-launch block-diagonal products and of the dropout rate per member: the argument checks of
`tgcn_blockdiag_*` through ctypes (no GPU), `crossval.grid_members`, the rates of `PerLabelGCN` / `CrossValGCN` and their
round trip through `from_members` / `export_members`, the float64 reference against the product written out directly, and
the completeness of the case lists of tests/_blockdiag_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

import _blockdiag_ref as B
import _dropout_hash as DH
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, perlabel
from pytextgcn_amd.crossval import MAX_MEMBERS, CrossValGCN, fold_bits, grid_members
from pytextgcn_amd.perlabel import BlockDiagLayout, PerLabelGCN


def _layout_status(K, h, n_cols, col0, n, p, out_bytes=None):
    lib = _lib.load()
    a = np.asarray(col0, dtype=np.int32)
    b = np.asarray(n, dtype=np.int32)
    r = None if p is None else np.asarray(p, dtype=np.float64)
    size = 64 + 32 * max(K, 1) if out_bytes is None else out_bytes
    out = np.zeros(64 + 32 * 200, dtype=np.uint8)
    return lib.tgcn_blockdiag_layout(K, h, n_cols, a.ctypes.data, b.ctypes.data, None if r is None else r.ctypes.data,
                                     out.ctypes.data, size), lib.tgcn_last_error()


def test_layout_refuses_what_the_header_says_it_refuses():
    lib = _lib.load()
    ok = dict(K=2, h=8, n_cols=16, col0=[0, 8], n=[5, 7], p=[0.0, 0.5])
    assert _layout_status(**ok)[0] == _lib.OK
    assert lib.tgcn_blockdiag_max_hidden() == B.H_MAX >= 256
    bad = [dict(K=0, col0=[], n=[], p=[]), dict(K=B.K_MAX + 1, col0=[4 * k for k in range(B.K_MAX + 1)],
                                                 n=[1] * (B.K_MAX + 1), p=[0.0] * (B.K_MAX + 1), n_cols=1024),
           dict(h=0), dict(h=B.H_MAX + 1), dict(n=[0, 7]), dict(n=[5, -1]),
           dict(col0=[0, 4]),                      # overlapping: member 0 ends at 5
           dict(col0=[8, 0]),                      # decreasing
           dict(n=[5, 9]),                         # past n_cols
           dict(col0=[-4, 8]), dict(p=[1.0, 0.0]), dict(p=[0.0, -0.1]), dict(p=[float("nan"), 0.0]), dict(n_cols=0)]
    for change in bad:
        st, msg = _layout_status(**{**ok, **change})
        assert st == _lib.E_INVALID and b"tgcn_blockdiag_layout" in msg, change
    st, msg = _layout_status(**ok, out_bytes=lib.tgcn_blockdiag_layout_bytes(2) - 1)
    assert st == _lib.E_INVALID and b"out of" in msg
    assert lib.tgcn_blockdiag_layout_bytes(0) == 0 and lib.tgcn_blockdiag_layout_bytes(B.K_MAX + 1) == 0
    assert lib.tgcn_blockdiag_layout_bytes(B.K_MAX) == 64 + 32 * B.K_MAX
    assert _layout_status(B.K_MAX, B.H_MAX, 4 * B.K_MAX, [4 * k for k in range(B.K_MAX)], [1] * B.K_MAX, None)[0] == _lib.OK
    with pytest.raises(ValueError, match="overlap"):
        BlockDiagLayout([0, 4], [5, 7], 8, 16)


def test_layout_blob_holds_the_table_the_kernels_read():
    lay = BlockDiagLayout([4, 12, 24], [5, 7, 1], 8, 32, [0.0, 0.5, 0.999])
    assert lay.dev is None and lay.header["K"] == 3 and lay.header["h"] == 8 and lay.header["n_cols"] == 32
    assert lay.header["n_max"] == 7 and lay.header["any_drop"] == 1
    m = lay.members()
    assert m["col0"].tolist() == [4, 12, 24] and m["n"].tolist() == [5, 7, 1]
    assert m["own0"].tolist() == [0, 12, 24] and m["own1"].tolist() == [12, 24, 32]      # every column has one writer
    assert lay.header["own_max"] == 12
    assert m["drop"].tolist() == [0, 1, 1] and m["scale"].tolist() == [1.0, 2.0, np.float32(1.0 / (1.0 - 0.999))]
    assert m["thresh"].tolist() == [0, 1 << 31, min(int(0.999 * 4294967296.0), 4294967295)]
    assert BlockDiagLayout([0], [3], 4, 4).header["any_drop"] == 0


def test_layouts_live_as_long_as_their_weight_and_are_never_evicted():
    """a captured graph holds the device blob's raw pointer: the cache may not drop a layout while the weight -- the
    network -- exists, however many other layouts are built meanwhile"""
    import gc
    w = torch.zeros(8, 16)
    first = perlabel._bd_layout(w, (0, 8), (5, 7), (0.0, 0.5))
    ptr = first.dev.data_ptr()
    others = [torch.zeros(8, 16) for _ in range(200)]
    for i, o in enumerate(others):
        perlabel._bd_layout(o, (0, 8), (5, 7), (0.0, (i + 1) / 300.0))
    assert perlabel._bd_layout(w, (0, 8), (5, 7), (0.0, 0.5)) is first and first.dev.data_ptr() == ptr
    assert perlabel._bd_layout(w, (0, 8), (5, 7), (0.0, 0.25)) is not first                  # another description: its own
    assert perlabel._bd_layout(w, (0, 8), (5, 7), (0.0, 0.5)) is first
    n = len(perlabel._BD_LAYOUTS)
    key = id(w)
    del others, o, w
    gc.collect()
    assert len(perlabel._BD_LAYOUTS) == n - 201 and key not in perlabel._BD_LAYOUTS          # entries go with their weights


def _host_blob(K=2, h=8):
    return BlockDiagLayout([0, 8], [5, 7], h, 16, [0.0, 0.5])


def test_products_refuse_bad_arguments_without_a_gpu():
    """every refusal comes before anything is enqueued: the pointers are never followed, no device is needed"""
    lib = _lib.load()
    lay = _host_blob()
    hp, dp = lay.host.ctypes.data, lay.host.ctypes.data      # (the "device" copy is never read on a refused call)
    P = 4096                                                  # a non-NULL value that nothing dereferences
    N = 10
    junk = np.zeros(128, dtype=np.uint8)
    fwd = lambda **kw: lib.tgcn_blockdiag_xw(*[{**dict(X=P, ldx=16, W=P, ldw=16, C=P, ldc=16, N=N, lh=hp, ld=dp, seeds=None,
                                                       row0=0, stream=None), **kw}[k] for k in
                                               ("X", "ldx", "W", "ldw", "C", "ldc", "N", "lh", "ld", "seeds", "row0", "stream")])
    for kw, word in ((dict(ldx=15), b"ldx"), (dict(ldw=15), b"ldw"), (dict(ldc=15), b"ldc"), (dict(X=None), b"X is NULL"),
                     (dict(W=None), b"W is NULL"), (dict(C=None), b"C is NULL"), (dict(N=-1), b"N must"),
                     (dict(row0=-1), b"mask_row0"), (dict(lh=None), b"layout_host"), (dict(ld=None), b"layout_dev"),
                     (dict(lh=junk.ctypes.data), b"not a blob")):
        assert fwd(**kw) == _lib.E_INVALID and word in lib.tgcn_last_error(), kw
    assert fwd(N=0, X=None, W=None, C=None) == _lib.OK       # no row: nothing to enqueue
    assert fwd(N=B.T * B.MAX_TILES + 1) == _lib.E_INVALID and b"N must" in lib.tgcn_last_error()   # more tiles than a grid takes
    assert lib.tgcn_blockdiag_xw_grad_workspace_bytes(hp, B.T * B.MAX_TILES + 1) == 0
    need = lib.tgcn_blockdiag_xw_grad_workspace_bytes(hp, N)
    assert need >= 4 * (1 * 2 * 8 + 1 * 2 * 8 * 7)
    assert lib.tgcn_blockdiag_xw_grad_workspace_bytes(None, N) == 0 and lib.tgcn_blockdiag_xw_grad_workspace_bytes(hp, -1) == 0
    names = ("X", "ldx", "W", "ldw", "G", "ldg", "dX", "lddx", "colsum", "dW", "lddw", "N", "lh", "ld", "seeds", "row0", "ws",
             "ws_bytes", "stream")
    base = dict(X=P, ldx=16, W=P, ldw=16, G=P, ldg=16, dX=P, lddx=16, colsum=P, dW=P, lddw=16, N=N, lh=hp, ld=dp, seeds=None,
                row0=0, ws=P, ws_bytes=need, stream=None)
    grad = lambda **kw: lib.tgcn_blockdiag_xw_grad(*[{**base, **kw}[k] for k in names])
    for kw, word in ((dict(ldx=15), b"ldx"), (dict(ldw=15), b"ldw"), (dict(ldg=15), b"ldg"), (dict(lddx=15), b"lddx"),
                     (dict(lddw=15), b"lddw"), (dict(G=None), b"G is NULL"), (dict(W=None), b"W is NULL"),
                     (dict(X=None), b"X is NULL"), (dict(colsum=None), b"together"), (dict(dX=None), b"together"),
                     (dict(dX=None, colsum=None, dW=None), b"nothing to compute"), (dict(N=-1), b"N must"),
                     (dict(row0=-2), b"mask_row0"), (dict(lh=None), b"layout_host")):
        assert grad(**kw) == _lib.E_INVALID and word in lib.tgcn_last_error(), kw
    for kw in (dict(ws_bytes=need - 1), dict(ws=None)):
        assert grad(**kw) == _lib.E_WORKSPACE and b"workspace" in lib.tgcn_last_error(), kw


def test_grid_members_order_agrees_with_fold_bits():
    lrs, dos, k = [0.1, 0.05, 0.01, 0.001], [0.5, 0.7], 3
    mlr, mdo = grid_members(lrs, dos, k)
    assert len(mlr) == len(mdo) == 24
    for d in range(2):
        for l in range(4):
            for f in range(3):
                m = (d * 4 + l) * 3 + f
                assert mlr[m] == lrs[l] and mdo[m] == dos[d]
    docs = np.arange(5, 17)
    folds = [np.arange(f, 12, 3) for f in range(k)]
    train, val = fold_bits(docs, folds, 20, n_repeats=len(dos) * len(lrs))
    for m in range(24):                                     # member m validates on fold m % k, whatever its rate and dropout
        rows = torch.nonzero((val >> m) & 1).flatten().numpy()
        assert rows.tolist() == docs[folds[m % k]].tolist()
        assert int(((train >> m) & 1).sum()) == 12 - 4
    with pytest.raises(ValueError, match="members"):
        grid_members([0.1] * 11, [0.5, 0.7], 3)              # 66 > MAX_MEMBERS
    assert len(grid_members([0.1] * 16, [0.5, 0.7], 2)[0]) == MAX_MEMBERS
    with pytest.raises(ValueError):
        grid_members([], [0.5], 3)


def test_constructors_validate_the_rates():
    net = CrossValGCN(10, 3, 4, n_hidden_gcn=8, dropout=[0.0, 0.1, 0.5, 0.9])
    assert net.dropout == (0.0, 0.1, 0.5, 0.9) and net.member_dropout(2) == 0.5
    assert CrossValGCN(10, 3, 4, n_hidden_gcn=8, dropout=0.3).dropout == 0.3
    assert PerLabelGCN(10, [2, 3], n_hidden_gcn=8, dropout=(0.2, 0.0)).dropout == (0.2, 0.0)
    for bad in ([0.1, 0.2, 0.3], [0.1, 0.2, 0.3, 1.0], [0.1, -0.2, 0.3, 0.0], [0.1] * 5):
        with pytest.raises(ValueError):
            CrossValGCN(10, 3, 4, n_hidden_gcn=8, dropout=bad)
    with pytest.raises(ValueError):
        PerLabelGCN(10, [2, 3], n_hidden_gcn=8, dropout=[0.5])


def test_members_round_trip_their_rates():
    torch.manual_seed(0)
    rates = [0.0, 0.5, 0.5, 0.7]
    members = [pkg.GCN(12, 3, n_hidden_gcn=8, dropout=p) for p in rates]
    for cls in (CrossValGCN, PerLabelGCN):
        net = cls.from_members(members)
        assert net.dropout == tuple(rates)
        back = net.export_members()
        assert [m.dropout for m in back] == rates
        for a, b in zip(members, back):
            for pa, pb in zip(a.parameters(), b.parameters()):
                assert torch.equal(pa, pb)
        assert cls.from_members(back).dropout == tuple(rates)
        same = cls.from_members([pkg.GCN(12, 3, n_hidden_gcn=8, dropout=0.4) for _ in range(3)])
        assert same.dropout == 0.4 and isinstance(same.dropout, float)            # equal rates stay a float
        assert [m.dropout for m in same.export_members()] == [0.4] * 3
        assert cls.from_members(members, dropout=0.25).dropout == 0.25
        assert cls.from_members(members, dropout=[0.1, 0.2, 0.3, 0.4]).dropout == (0.1, 0.2, 0.3, 0.4)
        with pytest.raises(ValueError):
            cls.from_members(members, dropout=[0.1, 0.2])


def test_switch_returns_the_previous_setting_and_is_off_by_default():
    assert perlabel._FUSED_BLOCK_DIAG is False
    assert perlabel.enable_fused_block_diag() is False
    assert perlabel.enable_fused_block_diag(False) is True
    assert perlabel._FUSED_BLOCK_DIAG is False


def test_reference_with_one_member_is_the_masked_product_written_out():
    N, h, n, p, seed, row0 = 37, 33, 5, 0.3, -77, (1 << 32) + 5
    X, W, G = B.operands(N, h, 1, 8, "randn")
    C, dX, cs, dW = B.products(X, W, G, h, [0], [n], [p], [seed], row0)
    keep = DH.keep_mask(seed, (np.arange(N, dtype=np.uint64) + np.uint64(row0))[:, None], np.arange(h, dtype=np.uint64)[None, :], p)
    assert 0.55 < keep.mean() < 0.85
    a = np.where(keep, X.astype(np.float64) / (1.0 - p), 0.0)
    W64, G64 = W.astype(np.float64)[:, :n], G.astype(np.float64)[:, :n]
    close = lambda u, v: np.allclose(u, v, rtol=0, atol=1e-13 * np.abs(v).max())     # (x / (1 - p) against x * (1 / (1 - p)))
    assert close(C[:, :n], a @ W64) and not C[:, n:].any()
    want_dx = np.where(keep, (G64 @ W64.T) / (1.0 - p), 0.0)
    assert close(dX, want_dx) and np.array_equal(cs, dX.sum(0)) and np.array_equal(dX == 0, ~keep)
    assert close(dW[:, :n], a.T @ G64) and not dW[:, n:].any()
    # no seeds, or rate 0: the plain product
    C0 = B.products(X, W, G, h, [0], [n], [p], None)[0]
    assert np.array_equal(C0[:, :n], X.astype(np.float64) @ W64)
    assert np.array_equal(B.products(X, W, G, h, [0], [n], [0.0], [seed])[0], C0)


def test_case_lists_cover_every_instantiation_column_group_and_axis_value():
    cases = B.all_exact_cases()
    seen = set()
    by_inst = {}
    for c in cases:
        assert B.partial_sum_bound(c) < 2 ** 24, c
        assert all(r in B.EXACT_RATES for r in c["rates"]) and len(c["rates"]) == len(c["widths"])
        for inst in B.instantiations(c["h"], c["widths"]):
            seen.add(inst)
            d = by_inst.setdefault(inst, dict(N=set(), h=set(), row0=set(), outputs=set(), widths=set()))
            d["N"].add(c["N"]); d["h"].add(c["h"]); d["row0"].add(c["mask_row0"]); d["outputs"].add(c["outputs"])
            d["widths"].add(tuple(c["widths"]))
    assert seen == B.ALL_INSTANTIATIONS
    for inst, d in by_inst.items():
        assert d["N"] >= set(B.ROWS), (inst, sorted(set(B.ROWS) - d["N"]))
        # the dW instantiations are picked by h itself: TJ = 1 serves h <= 128, TJ = 2 the rest
        hs = {h for h in B.HIDDEN if inst[0] != "dw" or (h > 128) == (inst[1] == 2)}
        assert d["h"] >= hs, (inst, sorted(hs - d["h"]))
        assert d["row0"] == set(B.MASK_ROW0) and d["outputs"] == set(B.OUTPUTS), inst
    # dW's slice grid is capped: every instantiation of k_bd_grad_w meets the first row count at which a workgroup takes a
    # second chunk (and so does the reduction over slices that are no longer single chunks)
    past = {inst: False for inst in B.ALL_INSTANTIATIONS if inst[0] == "dw"}
    for c in cases:
        K = len(c["widths"])
        slices, rows_per_slice = B.dw_slices(c["N"], K)
        if c["N"] == B.dw_rows_past_cap(K) and c["outputs"] != "no-dw":
            assert rows_per_slice == 2 * B.W_CHUNK and slices <= B.dw_slice_cap(K)
            assert B.dw_slices(c["N"] - 1, K) == (B.dw_slice_cap(K), B.W_CHUNK)      # one row fewer: still a chunk each
            for inst in B.instantiations(c["h"], c["widths"]):
                if inst[0] == "dw":
                    past[inst] = True
        elif c not in B.PAST_SLICE_CAP:
            assert rows_per_slice == B.W_CHUNK                                       # (what the other cases never reach)
    assert all(past.values()), past
    assert (B.dw_rows_past_cap(128), B.dw_rows_past_cap(64), B.dw_rows_past_cap(12), B.dw_rows_past_cap(1)) == \
        (513, 1025, 5377, 256 * 128 + 1)
    # the forward and dX give every row tile a workgroup of its own: no second stride; past MAX_TILES the call is refused
    assert B.MAX_TILES * 256 < 2 ** 32 <= (B.MAX_TILES + 1) * 256
    # column groups: a second forward group past 256 columns, second and third dX / dW groups past 128 and 256
    l = B.launches(8, [257, 2])
    assert l["fwd"] == [8, 1] and l["dx"] == [4, 4, 1] and l["dw"] == [(1, 4), (1, 4), (1, 1)]
    assert B.launches(200, [64, 65, 1, 7]) == {"fwd": [4], "dx": [4], "dw": [(2, 4)]}
    assert B.launches(8, [40, 33]) == {"fwd": [2], "dx": [2], "dw": [(1, 2)]}
    assert {tuple(w) for w in B.WIDTHS} >= {(1,), (3, 4), (5,) * 12, (64, 65, 1, 7), (257, 2)}
    assert set(B.ROWS) >= {0, 1, 31, 33, B.T - 1, B.T, B.T + 1, 2 * B.T + 1}
    assert set(B.HIDDEN) == {1, 3, 31, 32, 33, 100, 200, B.H_MAX}
    assert any(len(c["widths"]) == 64 for c in cases) and any(c["widths"] == [1] * 128 for c in cases)
    every_seed = {s for c in cases for s in B.seeds_for(len(c["widths"]), c["salt"])}
    assert any(s < 0 for s in every_seed) and -(1 << 63) in every_seed and -1 in every_seed
    assert any(c["eval"] for c in cases) and any(c["lead"] for c in cases) and any(c["gap"] for c in cases)
    assert B.dw_slices(0, 3) == (1, 128) and B.dw_slices(257, 2)[0] == 3 and B.dw_slices(1000, 128) == (4, 256)
