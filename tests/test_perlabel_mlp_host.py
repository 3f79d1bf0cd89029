"""Host tests of the grouped MLP products' layout and argument checks (`tgcn_mlp_grouped_*`,
pytextgcn_amd/csrc/mlp_grouped.hip), of `perlabel.GroupedRows` and of `PerLabelMLP`'s bridge to K ordinary `MLP`s.  No GPU:
nothing is enqueued here."""
import ctypes

import numpy as np
import pytest
import torch

import _perlabel_mlp_ref as P

# (row_ptr, N): an empty group in the middle; a group of one row behind a full one; one group of three tiles; seven groups,
# the last one empty, and five rows without a group
TABLES = [([0, 33, 33, 162], 162), ([0, 127, 128], 128), ([0, 257], 257), ([0, 1, 32, 64, 97, 161, 256, 256], 261)]


def _layout(row_ptr, rows, width=33, cols=5, **over):
    """Hidden style: K members of `cols` result columns on activations of `width` columns; `over` replaces arguments."""
    from pytextgcn_amd import mlp
    K = len(row_ptr) - 1
    kw = dict(w_row0=[g * cols for g in range(K)], n=[cols] * K, col0=[0] * K, b_off=[g * width for g in range(K)], N=rows,
              k=width, w_rows=K * cols, c_cols=cols, b_len=K * width)
    kw.update(over)
    return mlp.GroupedLayout(row_ptr, **kw)


@pytest.mark.parametrize("k", [32, 515, 4096])
@pytest.mark.parametrize("row_ptr,N", TABLES + [([0, 4100, 4230], 4230)])
def test_layout_blob_is_the_python_restatement(row_ptr, N, k):
    lay = _layout(row_ptr, N, width=k)
    groups, tiles, slices = lay.tables()
    want_tiles, want_slices, cps = P.tables(row_ptr, k)
    K = len(row_ptr) - 1
    assert lay.header["K"] == K and lay.header["N"] == N and lay.header["k"] == k and lay.n_routed == row_ptr[K]
    assert lay.header["chunks_per_slice"] == cps and lay.header["bytes"] <= lay.host.size
    assert [(int(t["group"]), int(t["row0"]), int(t["count"])) for t in tiles] == want_tiles
    assert [(int(s["group"]), int(s["row0"]), int(s["row_end"])) for s in slices] == want_slices
    # tiles: at most 128 rows, inside one group, every row of a segment exactly once, none for an empty group
    covered = np.zeros(N, dtype=np.int64)
    for t in tiles:
        g, r0, cnt = int(t["group"]), int(t["row0"]), int(t["count"])
        assert 1 <= cnt <= 128 and row_ptr[g] <= r0 and r0 + cnt <= row_ptr[g + 1]
        covered[r0:r0 + cnt] += 1
    assert (covered[:row_ptr[K]] == 1).all() and (covered[row_ptr[K]:] == 0).all()
    # slices: whole chunks inside one group (only a group's last slice may end early), in order, covering the segment
    for g in range(K):
        rec = groups[g]
        assert (int(rec["row0"]), int(rec["rows"])) == (row_ptr[g], row_ptr[g + 1] - row_ptr[g])
        mine_t = tiles[int(rec["tile0"]):int(rec["tile0"]) + int(rec["n_tiles"])]
        mine_s = slices[int(rec["slice0"]):int(rec["slice0"]) + int(rec["n_slices"])]
        assert all(int(t["group"]) == g for t in mine_t) and all(int(s["group"]) == g for s in mine_s)
        assert sum(int(t["count"]) for t in mine_t) == row_ptr[g + 1] - row_ptr[g]
        if row_ptr[g] == row_ptr[g + 1]:
            assert len(mine_t) == 0 and len(mine_s) == 0
            continue
        at = row_ptr[g]
        for i, s in enumerate(mine_s):
            assert int(s["row0"]) == at and (int(s["row0"]) - row_ptr[g]) % 128 == 0
            assert int(s["row_end"]) - at == cps * 128 or (i == len(mine_s) - 1 and int(s["row_end"]) == row_ptr[g + 1])
            at = int(s["row_end"])
        assert at == row_ptr[g + 1]
    assert len(tiles) == sum(int(r["n_tiles"]) for r in groups) and len(slices) == sum(int(r["n_slices"]) for r in groups)


def test_dw_slices_of_the_multi_chunk_case():
    """[0, 4100, 4230] at k = 515: 35 chunks for 30 wanted slices, so two chunks per slice; group 0 has 16 full slices and
    a last one of a single chunk of 4 rows, group 1 one slice of two chunks (128 + 2 rows)."""
    _, _, slices = _layout([0, 4100, 4230], 4230, width=515, cols=3).tables()
    assert len(slices) == 18 and (int(slices[16]["row0"]), int(slices[16]["row_end"])) == (4096, 4100)
    assert (int(slices[17]["row0"]), int(slices[17]["row_end"]), int(slices[17]["group"])) == (4100, 4230, 1)


def test_layout_refuses_what_does_not_fit_without_a_device():
    from pytextgcn_amd import _lib
    lib = _lib.load()
    rp, N = [0, 33, 33, 162], 162
    for over, word in (({"N": 161}, "row_ptr[K]"), ({"n": [5, 0, 5]}, "need >= 1"), ({"w_rows": 14}, "of W"),
                       ({"w_row0": [0, -1, 10]}, "of W"), ({"c_cols": 4}, "columns"), ({"col0": [0, 1, 0]}, "columns"),
                       ({"b_len": 98}, "of b"), ({"k": 0}, "k >= 1")):
        with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
            _layout(rp, N, **over)
    with pytest.raises(ValueError, match="decreases"):
        _layout([0, 33, 32, 162], N)
    with pytest.raises(ValueError, match="negative"):
        _layout([-1, 33, 33, 162], N)
    with pytest.raises(ValueError, match=r"\[1, 128\]"):
        _layout(list(range(130)), 129)
    assert _layout(list(range(129)), 128).K == 128
    one = np.zeros(2, dtype=np.int64)
    assert lib.tgcn_mlp_grouped_layout_bytes(0, one.ctypes.data) == 0
    assert lib.tgcn_mlp_grouped_layout_bytes(129, one.ctypes.data) == 0
    assert lib.tgcn_mlp_grouped_layout_bytes(1, None) == 0
    bad = np.array([5, 3], dtype=np.int64)
    assert lib.tgcn_mlp_grouped_layout_bytes(1, bad.ctypes.data) == 0
    i32 = np.zeros(1, dtype=np.int32)
    out = np.zeros(64, dtype=np.uint8)
    a = i32.ctypes.data
    assert lib.tgcn_mlp_grouped_layout(0, one.ctypes.data, a, a, a, a, 0, 1, 1, 1, 1, out.ctypes.data, 64) == _lib.E_INVALID
    assert b"K must be" in lib.tgcn_last_error()
    assert lib.tgcn_mlp_grouped_layout(1, None, a, a, a, a, 0, 1, 1, 1, 1, out.ctypes.data, 64) == _lib.E_INVALID
    assert b"row_ptr is NULL" in lib.tgcn_last_error()
    i32[0] = 0
    n1 = np.ones(1, dtype=np.int32)
    assert lib.tgcn_mlp_grouped_layout(1, one.ctypes.data, a, n1.ctypes.data, a, a, 0, 1, 1, 1, 1, out.ctypes.data,
                                       8) == _lib.E_INVALID
    assert b"tgcn_mlp_grouped_layout_bytes" in lib.tgcn_last_error()


def test_products_refuse_bad_arguments_without_a_device():
    from pytextgcn_amd import _lib
    lib = _lib.load()
    N, k, n, K = 162, 33, 5, 3
    lay = _layout([0, 33, 33, 162], N, width=k, cols=n)
    blob = lay.host.ctypes.data
    host = ctypes.create_string_buffer(4096)        # an address that is never read: every call returns before it enqueues
    a = ctypes.addressof(host)

    def fwd(Z=a, b=a, W=a, C=a, p=0.5, ldz=k, ldw=k, ldc=n, N=N, k=k, lh=blob, ld=a, row0=0):
        return lib.tgcn_mlp_grouped_act_linear(Z, ldz, b, W, ldw, None, C, ldc, N, k, lh, ld, p, None, row0, None)

    for kw, word in (({"Z": None}, b"Z is NULL"), ({"b": None}, b"b is NULL"), ({"W": None}, b"W is NULL"),
                     ({"C": None}, b"C is NULL"), ({"p": 1.0}, b"[0, 1)"), ({"ldz": k - 1}, b"ldz"), ({"ldw": k - 1}, b"ldw"),
                     ({"ldc": n - 1}, b"ldc"), ({"N": N + 1}, b"layout was built"), ({"k": k + 1, "ldz": k + 1, "ldw": k + 1},
                                                                                    b"layout was built"),
                     ({"lh": None}, b"layout_host is NULL"), ({"ld": None}, b"layout_dev is NULL"),
                     ({"lh": a}, b"not a blob"), ({"row0": -1}, b"mask_row0")):
        assert fwd(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())
    with pytest.raises(ValueError):
        _lib.check(fwd(p=1.0))

    need = lib.tgcn_mlp_grouped_act_linear_grad_workspace_bytes(blob)
    assert need > 0 and lib.tgcn_mlp_grouped_act_linear_grad_workspace_bytes(None) == 0
    assert lib.tgcn_mlp_grouped_act_linear_grad_workspace_bytes(a) == 0

    def grad(Z=a, b=a, W=a, G=a, dZ=a, db=a, dW=a, dc=None, p=0.5, ws=a, ws_bytes=need, ldg=n, lddz=k, lddw=k):
        return lib.tgcn_mlp_grouped_act_linear_grad(Z, k, b, W, k, G, ldg, dZ, lddz, db, dW, lddw, dc, N, k, blob, a, p, None,
                                                    0, ws, ws_bytes, None)

    for kw, word in (({"Z": None}, b"Z is NULL"), ({"b": None}, b"b is NULL"), ({"W": None}, b"W is NULL"),
                     ({"G": None}, b"G is NULL"), ({"p": 1.0}, b"[0, 1)"), ({"ws_bytes": need - 1}, b"workspace"),
                     ({"ws": None}, b"workspace"), ({"db": None}, b"both or neither"), ({"dZ": None}, b"both or neither"),
                     ({"dZ": None, "db": None, "dW": None}, b"nothing to compute"), ({"ldg": n - 1}, b"ldg"),
                     ({"lddz": k - 1}, b"lddz"), ({"lddw": k - 1}, b"lddw")):
        assert grad(**kw) == _lib.E_INVALID, kw
        assert word in lib.tgcn_last_error(), (kw, lib.tgcn_last_error())


def test_grouped_rows_order_take_restore():
    from pytextgcn_amd.perlabel import GroupedRows
    group = torch.tensor([2, -1, 0, 2, 1, -1, 0, 2, 3, 0], dtype=torch.int32)
    rows = GroupedRows(group, 5)
    assert rows.order.tolist() == [2, 6, 9, 4, 0, 3, 7, 8, 1, 5]           # stable inside a group, -1 last
    assert rows.row_ptr == [0, 3, 4, 7, 8, 8] and rows.n_routed == 8 and rows.n_rows == 10 and rows.n_groups == 5
    assert rows.group_sorted.dtype == torch.int32 and rows.group_sorted.tolist() == [0, 0, 0, 1, 2, 2, 2, 3, -1, -1]
    t = torch.arange(10) * 10
    assert rows.take(t).tolist() == [20, 60, 90, 40, 0, 30, 70, 80, 10, 50]
    back = rows.restore(rows.take(t))
    assert back.tolist() == [0, -1, 20, 30, 40, -1, 60, 70, 80, 90]         # rows without a group: `fill`
    assert rows.restore(rows.take(t), fill=7)[1].item() == 7
    m = torch.randn(10, 3)
    routed = group >= 0
    assert torch.equal(rows.restore(rows.take(m), fill=0.0)[routed], m[routed])
    full = GroupedRows(torch.tensor([1, 0, 1, 0]), 2)
    assert torch.equal(full.restore(full.take(t[:4])), t[:4])               # every row has a group: the identity
    for bad in ([0, 5], [-2, 0]):
        with pytest.raises(ValueError, match="groups must lie"):
            GroupedRows(torch.tensor(bad), 5)
    with pytest.raises(ValueError, match="rows"):
        rows.take(torch.zeros(9))


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_grouped_rows_features_against_scipy(layout):
    sp = pytest.importorskip("scipy.sparse")
    from pytextgcn_amd.perlabel import GroupedRows
    rng = np.random.default_rng(3)
    N, F, K = 23, 11, 4
    group = rng.integers(-1, K, size=N)
    x = sp.random(N, F, density=0.3, random_state=5, format="csr", dtype=np.float32)
    rows = GroupedRows(torch.from_numpy(group), K)
    coo = x.tocoo()
    xt = torch.sparse_coo_tensor(np.stack([coo.row, coo.col]), coo.data, (N, F))
    got = rows.features(xt.to_sparse_csr() if layout == "csr" else xt)
    assert got.layout == torch.sparse_coo and got.is_coalesced() and tuple(got.shape) == (N, K * F)
    order = rows.order.numpy()
    want = sp.lil_matrix((N, K * F), dtype=np.float32)
    for new, old in enumerate(order):
        g = group[old]
        if g >= 0:
            want[new, g * F:(g + 1) * F] = x[old].toarray()
    want = want.tocoo()
    want.sum_duplicates()
    want = sp.coo_matrix(want.tocsr().tocoo())                             # row-major entry order, as coalesce gives
    assert got.indices()[0].tolist() == want.row.tolist() and got.indices()[1].tolist() == want.col.tolist()
    assert got.values().tolist() == want.data.tolist()
    with pytest.raises(TypeError, match="sparse"):
        rows.features(torch.zeros(N, F))


def test_members_round_trip_bit_for_bit():
    from pytextgcn_amd.lib.models import MLP, PerLabelMLP
    import pytextgcn_amd as pkg
    assert PerLabelMLP is pkg.PerLabelMLP is pkg.perlabel.PerLabelMLP
    torch.manual_seed(9)
    counts, F, hidden = [2, 5, 3], 13, [7, 6]
    members = [MLP(F, c, hidden, dropout=0.3) for c in counts]
    net = PerLabelMLP.from_members(members)
    assert net.class_counts == (2, 5, 3) and net.seg_start == (0, 4, 12) and net.n_cols == 16 and net.seg_width == (2, 5, 3)
    assert net.dropout.p == 0.3 and net.hidden == (7, 6) and net.in_channels == F
    assert [tuple(layer.weight.shape) for layer in net.layers] == [(7, 3 * F), (3 * 6, 7), (16, 6)]
    assert [tuple(layer.bias.shape) for layer in net.layers] == [(3 * 7,), (3 * 6,), (16,)]
    pad = [i for i in range(16) if not any(s <= i < s + c for s, c in zip(net.seg_start, counts))]
    assert float(net.layers[2].weight.detach()[pad].abs().sum()) == 0.0 and float(net.layers[2].bias.detach()[pad].abs().sum()) == 0.0
    back = net.export_members()
    for m, b in zip(members, back):
        assert sorted(m.state_dict()) == sorted(b.state_dict())
        assert all(torch.equal(v, b.state_dict()[key]) for key, v in m.state_dict().items())
        fresh = MLP(F, m.layers[-1].out_features, hidden)
        fresh.load_state_dict(b.state_dict(), strict=True)
    # copies, not views
    with torch.no_grad():
        net.layers[0].weight.add_(1.0)
    assert all(torch.equal(v, b.state_dict()[key]) for m, b in zip(members, back) for key, v in m.state_dict().items())
    # and the other way round
    again = PerLabelMLP.from_members(back)
    with torch.no_grad():
        net.layers[0].weight.sub_(1.0)
    assert all(torch.equal(p, q) for p, q in zip(PerLabelMLP.from_members(members).parameters(), again.parameters()))


def test_members_of_other_shapes_are_refused():
    from pytextgcn_amd.lib.models import MLP, PerLabelMLP
    with pytest.raises(ValueError, match="no member"):
        PerLabelMLP.from_members([])
    for other in (MLP(14, 3, [7, 6]), MLP(13, 3, [7, 5]), MLP(13, 3, [7]), MLP(13, 3, [8, 6])):
        with pytest.raises(ValueError, match="equal"):
            PerLabelMLP.from_members([MLP(13, 2, [7, 6]), other])
    with pytest.raises(ValueError):
        PerLabelMLP(13, [], [7])
    with pytest.raises(ValueError):
        PerLabelMLP(13, [2, 0], [7])
    with pytest.raises(ValueError, match="128"):
        PerLabelMLP(2, [1] * 129, [2])


def test_default_init_keeps_each_members_bounds():
    from pytextgcn_amd.lib.models import PerLabelMLP
    torch.manual_seed(1)
    net = PerLabelMLP(50, [3, 4], [20, 10])
    for layer, fan_in in zip(net.layers, (50, 20, 10)):
        a = fan_in ** -0.5
        assert float(layer.weight.abs().max()) <= a and float(layer.bias.abs().max()) <= a
        assert float(layer.weight.abs().max()) > 0.9 * a                   # (and not the bound of the stacked fan-in)


def test_which_path_runs_and_cpu_tensors_are_refused():
    import pytextgcn_amd as pkg
    from pytextgcn_amd.perlabel import GroupedRows, PerLabelMLP
    try:
        for p, training, fused_dropout, want in ((0.5, False, False, True), (0.0, True, False, True),
                                                 (0.5, True, False, False), (0.5, True, True, True),
                                                 (1.0, True, True, False)):
            pkg.enable_fused_dropout(fused_dropout)
            model = PerLabelMLP(10, [2, 3], [8], dropout=p).train(training)
            assert model.takes_fused_path() is want, (p, training, fused_dropout)
            was = pkg.enable_fused_mlp(False)
            assert model.takes_fused_path() is False
            pkg.enable_fused_mlp(was)
    finally:
        pkg.enable_fused_dropout(False)
    model = PerLabelMLP(10, [2, 3], [8]).eval()
    rows = GroupedRows(torch.tensor([0, 1, 1]), 2)
    x = torch.sparse_coo_tensor(torch.tensor([[0, 1, 2], [1, 5, 9]]), torch.ones(3), (3, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(rows.features(x), rows)
