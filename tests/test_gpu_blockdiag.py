"""GPU tests of the one-launch block-diagonal products (pytextgcn_amd/csrc/blockdiag.hip: `tgcn_blockdiag_xw`,
`tgcn_blockdiag_xw_grad`), of `perlabel.block_diag_xw` with a rate per member on both paths, and of `CrossValGCN` with
per-member dropout.

The kernels run through the C ABI on column slices of wider, poisoned buffers (offset 3 floats: nothing is 16-byte
aligned).  With small-integer operands and the rates {0, 0.5, 0.75} every product and every partial sum is an integer below
2^24, so fp32 is exact in any order and C, dX, colsum and dW must equal the float64 reference of tests/_blockdiag_ref.py
bit for bit.  On `randn` operands the bar is the project's, max|a - b| / max|b| <= 1e-5 (BASELINE.json).  The network is
held to `oracle.gcn_oracle.GCNOracle` in float64, member by member."""
import numpy as np
import pytest
import torch

import _blockdiag_ref as B
import _crossval_ref as R
import _dropout_hash as DH
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, dense, models, perlabel, synth
from pytextgcn_amd import plan as plan_mod
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits
from pytextgcn_amd.perlabel import BlockDiagLayout, block_diag_xw

pytestmark = pytest.mark.gpu
TOL = 1e-5
F32, I64 = torch.float32, torch.int64
OFF, EXTRA = 3, 5                                   # the operands start 3 floats into rows of width + 5


def _wide(dev, a, fill):
    """`a` [r, c] as a column slice of a poisoned [r + 1, c + EXTRA] buffer"""
    r, c = a.shape
    wide = torch.full((r + 1, c + EXTRA), fill, dtype=F32, device=dev)
    wide[:r, OFF:OFF + c] = torch.as_tensor(a).to(dev)
    return wide, wide[:r, OFF:OFF + c]


def _untouched(wide, r, c):
    w = wide.cpu()
    return bool((w[:r, :OFF] == B.FILL).all()) and bool((w[:r, OFF + c:] == B.FILL).all()) and bool((w[r:] == B.FILL).all())


def raw_products(dev, X, W, G, h, starts, widths, rates, seeds, mask_row0=0, outputs="all"):
    """The three products through ctypes.  `seeds`: K Python ints or None (the eval product).  Returns the results on the
    CPU (None: not asked for) after checking that nothing outside their extents was written."""
    lib = _lib.load()
    K, N, n_cols = len(widths), X.shape[0], W.shape[1]
    lay = BlockDiagLayout(starts, widths, h, n_cols, rates, dev)
    nan = float("nan")
    (xw, x), (ww, w), (gw, g) = _wide(dev, X, nan), _wide(dev, W, nan), _wide(dev, G, nan)
    cw, c = _wide(dev, np.full((N, n_cols), B.FILL, np.float32), B.FILL)
    dxw, dx = _wide(dev, np.full((N, K * h), B.FILL, np.float32), B.FILL)
    dww, dw = _wide(dev, np.full((h, n_cols), B.FILL, np.float32), B.FILL)
    cs = torch.full((K * h + 4,), B.FILL, dtype=F32, device=dev)
    sd = None if seeds is None else torch.tensor(seeds, dtype=I64, device=dev)
    sp = None if sd is None else sd.data_ptr()
    stream = plan_mod._stream_ptr(dev)
    st = lib.tgcn_blockdiag_xw(x.data_ptr(), xw.size(1), w.data_ptr(), ww.size(1), c.data_ptr(), cw.size(1), N,
                               lay.host.ctypes.data, lay.dev.data_ptr(), sp, mask_row0, stream)
    assert st == _lib.OK, lib.tgcn_last_error()
    want_x, want_w = outputs != "no-dx", outputs != "no-dw"
    need = lib.tgcn_blockdiag_xw_grad_workspace_bytes(lay.host.ctypes.data, N)
    ws = torch.full((need // 4 + 4,), B.FILL, dtype=F32, device=dev)
    st = lib.tgcn_blockdiag_xw_grad(x.data_ptr(), xw.size(1), w.data_ptr(), ww.size(1), g.data_ptr(), gw.size(1),
                                    dx.data_ptr() if want_x else None, dxw.size(1), cs.data_ptr() if want_x else None,
                                    dw.data_ptr() if want_w else None, dww.size(1), N, lay.host.ctypes.data,
                                    lay.dev.data_ptr(), sp, mask_row0, ws.data_ptr(), need, stream)
    assert st == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    assert _untouched(cw, N, n_cols) and _untouched(dxw, N, K * h) and _untouched(dww, h, n_cols)
    assert bool((cs[K * h:] == B.FILL).all()) and bool((ws[need // 4:] == B.FILL).all())
    if not want_x:
        assert bool((dxw == B.FILL).all()) and bool((cs == B.FILL).all())
    if not want_w:
        assert bool((dww == B.FILL).all())
    return dict(C=c.cpu(), dX=dx.cpu() if want_x else None, colsum=cs[:K * h].cpu() if want_x else None,
                dW=dw.cpu() if want_w else None)


def _pad_columns(starts, widths, n_cols):
    pad = np.ones(n_cols, dtype=bool)
    for s, c in zip(starts, widths):
        pad[s:s + c] = False
    return pad


def _run_exact(dev, c):
    K, N, h = len(c["widths"]), c["N"], c["h"]
    assert B.partial_sum_bound(c) < 2 ** 24
    starts, n_cols = B.layout(c["widths"], c["lead"], c["gap"])
    X, W, G = B.operands(N, h, K, n_cols, "int", c["salt"])
    seeds = None if c["eval"] else B.seeds_for(K, c["salt"])
    want = B.products(X, W, G, h, starts, c["widths"], c["rates"], seeds, c["mask_row0"])
    got = raw_products(dev, X, W, G, h, starts, c["widths"], c["rates"], seeds, c["mask_row0"], c["outputs"])
    pad = _pad_columns(starts, c["widths"], n_cols)
    for name, ref in zip(("C", "dX", "colsum", "dW"), want):
        if got[name] is None:
            continue
        assert np.abs(ref).max(initial=0.0) < 2 ** 24
        assert np.array_equal(got[name].numpy().astype(np.float64), ref), (name, {k: c[k] for k in ("N", "h", "widths")})
    assert not got["C"].numpy()[:, pad].any()
    if got["dW"] is not None:
        assert not got["dW"].numpy()[:, pad].any()
    if N == 0 and got["colsum"] is not None:
        assert not got["colsum"].numpy().any()


@pytest.mark.parametrize("widths", B.WIDTHS, ids=lambda w: "w" + "-".join(map(str, w[:4])) + ("x%d" % len(w) if len(w) > 4 else ""))
def test_exact_cases_equal_the_float64_reference_bit_for_bit(cuda, widths):
    for c in B.exact_cases(widths):
        _run_exact(cuda, c)


@pytest.mark.parametrize("c", B.MANY_MEMBERS, ids=["K64", "K128"])
def test_exact_cases_with_many_members(cuda, c):
    _run_exact(cuda, c)


@pytest.mark.parametrize("c", B.PAST_SLICE_CAP, ids=lambda c: f"K{len(c['widths'])}-n{max(c['widths'])}-h{c['h']}-N{c['N']}")
def test_exact_cases_past_the_slice_cap_of_dw(cuda, c):
    """one row more than dW's capped slice grid covers with a chunk per workgroup: slices of two chunks, the last one short"""
    K = len(c["widths"])
    assert B.dw_slices(c["N"], K)[1] == 2 * B.W_CHUNK and B.dw_slices(c["N"] - 1, K)[1] == B.W_CHUNK
    _run_exact(cuda, c)


def test_second_run_gives_the_same_bits(cuda):
    starts, n_cols = B.layout([64, 65, 1, 7])
    X, W, G = B.operands(1000, 100, 4, n_cols, "randn")
    seeds, rates = B.seeds_for(4), [0.0, 0.1, 0.4, 0.7]
    a = raw_products(cuda, X, W, G, 100, starts, [64, 65, 1, 7], rates, seeds)
    b = raw_products(cuda, X, W, G, 100, starts, [64, 65, 1, 7], rates, seeds)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_mask_read_back(cuda):
    """h = n_k = 33, W_k = I, X = 1: C is s_k keep_k itself; G = 1 shows the same decisions in dX (times the row sum of W_k =
    1) and dW[j, m] = sum_i a(i, j) G(i, m) = the column sums of s_k keep_k"""
    h, rates, N = 33, [0.0, 0.3, 0.5, 0.999], 300
    widths = [h] * 4
    starts, n_cols = B.layout(widths)
    seeds = B.seeds_for(4, 3)
    X = np.ones((N, 4 * h), np.float32)
    W = np.zeros((h, n_cols), np.float32)
    for s in starts:
        W[:, s:s + h] = np.eye(h, dtype=np.float32)
    G = np.ones((N, n_cols), np.float32)
    for row0 in B.MASK_ROW0:
        got = raw_products(cuda, X, W, G, h, starts, widths, rates, seeds, row0)
        rows = (np.arange(N, dtype=np.uint64) + np.uint64(row0))[:, None]
        cols = np.arange(h, dtype=np.uint64)[None, :]
        for k, (s, p) in enumerate(zip(starts, rates)):
            keep = DH.keep_mask(seeds[k], rows, cols, p) if p else np.ones((N, h), bool)
            scale = np.float32(1.0 / (1.0 - p))
            want = np.where(keep, scale, np.float32(0.0)).astype(np.float32)
            assert np.array_equal(got["C"].numpy()[:, s:s + h], want), (k, row0)
            assert np.array_equal(got["dX"].numpy()[:, k * h:(k + 1) * h], want), (k, row0)
            dw = got["dW"].numpy()[:, s:s + h]
            assert np.array_equal(dw != 0, np.repeat(keep.any(0)[:, None], h, 1))
            count = want.astype(np.float64).sum(0)               # s_k times the kept rows of column j
            if p in (0.0, 0.5):                                  # s_k count_j <= 600 is exact in fp32: every decision counts
                assert np.array_equal(dw.astype(np.float64), np.repeat(count[:, None], h, 1)), (k, row0)
            assert R.rel_err(torch.from_numpy(dw[:, 0].copy()), torch.from_numpy(count)) <= TOL
            if p:
                assert abs(keep.mean() - (1.0 - p)) < 0.02


RANDOM = [(5000, 100, [5] * 12), (1, 3, [3, 4]), (33, 31, [1]), (B.T + 1, 200, [64, 65, 1, 7]), (2 * B.T + 1, 32, [257, 2]),
          (1000, B.H_MAX, [40, 33]), (31, 33, [257, 2]), (B.T, 1, [64, 65, 1, 7])]


@pytest.mark.parametrize("N,h,widths", RANDOM, ids=lambda v: "x".join(map(str, v[:3])) if isinstance(v, list) else str(v))
def test_random_operands_against_float64(cuda, N, h, widths):
    K = len(widths)
    starts, n_cols = B.layout(widths)
    X, W, G = B.operands(N, h, K, n_cols, "randn")
    rates = [(0.0, 0.1, 0.4, 0.7)[k % 4] for k in range(K)]
    seeds = B.seeds_for(K, N)
    want = B.products(X, W, G, h, starts, widths, rates, seeds, 7)
    got = raw_products(cuda, X, W, G, h, starts, widths, rates, seeds, 7)
    errs = {name: R.rel_err(got[name], torch.from_numpy(ref)) for name, ref in zip(("C", "dX", "colsum", "dW"), want)}
    print(f"\nblockdiag randn N={N} h={h} widths={widths[:4]}: {errs}")
    assert all(e <= TOL for e in errs.values()), errs
    assert bool((got["dX"][torch.from_numpy(want[1] == 0)] == 0.0).all())          # the dropped elements: exactly zero


# ----------------------------------------------------------------------------------------------------------------------
# perlabel.block_diag_xw: the switch, and sequence rates on the K-launch path
# ----------------------------------------------------------------------------------------------------------------------
def _noted(dev, x, w, starts, widths, p, seeds, g):
    """(C, dX, dW, the column sums noted for dX) of one `block_diag_xw` call and its backward"""
    seen = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.view_as(t)

        @staticmethod
        def backward(ctx, grad):
            known = plan_mod._known_colsum(grad)
            seen["colsum"] = None if known is None else known.clone()
            return grad

    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    out = block_diag_xw(Probe.apply(xr), wr, starts, widths, p, seeds)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), xr.grad, wr.grad, seen["colsum"]


@pytest.mark.parametrize("widths,h", [([5] * 6, 40), ([64, 65, 1, 7], 8), ([257, 2], 200)], ids=["c5x6", "mixed", "wide"])
def test_switch_on_and_off_agree_bit_for_bit_on_exact_operands(cuda, widths, h):
    K, N = len(widths), 2 * B.T + 1
    starts, n_cols = B.layout(widths)
    X, W, G = (torch.from_numpy(a).to(cuda) for a in B.operands(N, h, K, n_cols, "int"))
    pad = torch.from_numpy(_pad_columns(starts, widths, n_cols)).to(cuda)
    W[:, pad] = 0.0
    seeds = torch.tensor(B.seeds_for(K, 4), dtype=I64, device=cuda)
    rates = [B.EXACT_RATES[(k + 1) % 3] for k in range(K)]
    assert perlabel._FUSED_BLOCK_DIAG is False
    for p, sd in ((rates, seeds), (0.5, seeds), (0.0, None)):
        off = _noted(cuda, X, W, starts, widths, p, sd, G)
        was = perlabel.enable_fused_block_diag()
        try:
            on = _noted(cuda, X, W, starts, widths, p, sd, G)
        finally:
            perlabel.enable_fused_block_diag(was)
        for name, a, b in zip(("C", "dX", "dW", "colsum"), off, on):
            assert a is not None and b is not None and torch.equal(a, b), (name, p)
    assert perlabel._FUSED_BLOCK_DIAG is False


def test_sequence_rates_on_the_k_launch_path_are_xw_dropout_per_member_bit_for_bit(cuda):
    widths, h, N = [5, 5, 5, 5, 3, 9], 40, 400
    K = len(widths)
    starts, n_cols = B.layout(widths)
    rates = [0.0, 0.4, 0.1, 0.0, 0.7, 0.4]
    gen = torch.Generator().manual_seed(17)
    H0 = torch.randn(N, K * h, generator=gen).to(cuda)
    W0 = torch.randn(h, n_cols, generator=gen).to(cuda)
    G = torch.randn(N, n_cols, generator=gen).to(cuda)
    seeds = torch.tensor([0x1234567890ABCDE, -77, (1 << 40) + 12345, 5, -(1 << 62), 99], dtype=I64, device=cuda)
    H, W = H0.clone().requires_grad_(), W0.clone().requires_grad_()
    out = block_diag_xw(H, W, starts, widths, rates, seeds)
    out.backward(G)
    for k, (s, c) in enumerate(zip(starts, widths)):
        Hk = H0[:, k * h:(k + 1) * h].contiguous().requires_grad_()
        Wk = W0[:, s:s + c].contiguous().requires_grad_()
        ok = dense.xw_dropout(Hk, Wk, rates[k], seeds[k:k + 1])
        ok.backward(torch.nn.functional.pad(G[:, s:s + c], (0, (-c) % 4))[:, :c])     # rows of 4 j floats, as a member GCN sees
        assert torch.equal(out[:, s:s + c], ok), k
        assert torch.equal(H.grad[:, k * h:(k + 1) * h], Hk.grad), k
        assert torch.equal(W.grad[:, s:s + c], Wk.grad), k
    with pytest.raises(ValueError, match="at least one rate"):
        block_diag_xw(H0, W0, starts, widths, [0.0] * K, seeds)
    with pytest.raises(ValueError):
        block_diag_xw(H0, W0, starts, widths, [0.5] * (K - 1), seeds)
    with pytest.raises(ValueError):
        block_diag_xw(H0, W0, starts, widths, [0.5] * (K - 1) + [1.0], seeds)


# ----------------------------------------------------------------------------------------------------------------------
# the network: the 400-node synth graph and the 6 members of tests/test_gpu_crossval.py's `_build`, restated
# ----------------------------------------------------------------------------------------------------------------------
N_NODES, N_CLASSES, N_FOLDS = 400, 5, 3
LR_AXIS = (0.05, 0.01)
LRS = [lr for lr in LR_AXIS for _ in range(N_FOLDS)]                 # member l * 3 + f: rate l, fold f
DROPOUT = [0.0, 0.0, 0.0, 0.5, 0.5, 0.7]
ADAM_EPS = 0.1


def _build(cuda, h):
    from oracle import gcn_oracle as O
    N, C, K = N_NODES, N_CLASSES, len(LRS)
    g = synth.word_doc_graph(N, 3000, seed=7, n_classes=C)
    doc_rows = np.arange(g.n_vocab, N)
    order = np.random.default_rng(11).permutation(doc_rows.size)
    folds = [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)]
    train_bits, val_bits = fold_bits(doc_rows, folds, N, n_repeats=len(LR_AXIS))
    target = g.y.clone().long()
    torch.manual_seed(3 + h)
    members = [pkg.GCN(N, C, n_hidden_gcn=h, dropout=0.0) for _ in range(K)]
    with torch.no_grad():
        for mem in members:
            for layer in mem.layers:
                layer.bias.uniform_(-0.5, 0.5)
    g64 = pkg.Data(x=g.x.double(), edge_index=g.edge_index, edge_attr=g.edge_attr.double())
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    truth = []
    for k, mem in enumerate(members):
        ref = O.GCNOracle(N, C, n_hidden_gcn=h, dropout=0.0)
        ref.load_state_dict(mem.state_dict())
        ref = ref.double().train()
        z = ref(g64)
        sel = R.selected(train_bits, k)
        lk = crit(z[sel], target[sel])
        lk.backward()
        grads = {n_: p.grad.clone() for n_, p in ref.named_parameters()}
        torch.optim.Adam(ref.parameters(), lr=LRS[k], eps=ADAM_EPS).step()
        truth.append(dict(logits=z.detach(), loss=lk.item(), grads=grads,
                          after={n_: p.detach().clone() for n_, p in ref.named_parameters()}))
    gd = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(cuda)
    return dict(gd=gd, target=target.to(cuda), train_bits=train_bits.to(cuda), val_bits=val_bits.to(cuda),
                bits_host=(train_bits, val_bits), members=members, truth=truth, h=h, N=N, K=K, C=C)


@pytest.fixture(scope="module", params=[8, 40], ids=["h8", "h40"])
def small(request, cuda):
    return _build(cuda, request.param)


def _net(s, cuda, dropout=DROPOUT):
    return CrossValGCN.from_members(s["members"], dropout=dropout).to(cuda).float()


def _member_slices(net, k):
    h, S, C = net.n_hidden, net.seg_stride, net.out_channels
    first, second = net.layers
    return {"layers.0.weight": (first.weight, (slice(None), slice(k * h, (k + 1) * h))),
            "layers.0.bias": (first.bias, (slice(k * h, (k + 1) * h),)),
            "layers.1.weight": (second.weight, (slice(None), slice(k * S, k * S + C))),
            "layers.1.bias": (second.bias, (slice(k * S, k * S + C),))}


class _switches:
    """fused dropout and the fused block-diagonal products, put back on exit"""

    def __init__(self, dropout=True, block_diag=True):
        self.want = (dropout, block_diag)

    def __enter__(self):
        self.was = (models._FUSED_DROPOUT, perlabel._FUSED_BLOCK_DIAG)
        pkg.enable_fused_dropout(self.want[0])
        perlabel.enable_fused_block_diag(self.want[1])

    def __exit__(self, *exc):
        pkg.enable_fused_dropout(self.was[0])
        perlabel.enable_fused_block_diag(self.was[1])


def test_rate_zero_members_match_the_oracle_and_the_others_do_not(cuda, small):
    net, gd, K, truth = _net(small, cuda).train(), small["gd"], small["K"], small["truth"]
    assert net.dropout == tuple(DROPOUT)
    with _switches():
        loss, loss_k = net.loss(gd, small["target"], small["train_bits"])
        loss.backward()
        MemberAdam(net, LRS, eps=ADAM_EPS).step()
        torch.cuda.synchronize()
    for k in range(K):
        want = truth[k]
        errs = {"loss": abs(float(loss_k[k]) - want["loss"]) / want["loss"]}
        for name, (p, idx) in _member_slices(net, k).items():
            errs["d " + name] = R.rel_err(p.grad[idx], want["grads"][name])
            errs[name] = R.rel_err(p.detach()[idx], want["after"][name])
        print(f"h={small['h']} member {k} (p={DROPOUT[k]}): {errs}")
        if DROPOUT[k] == 0.0:
            assert all(e <= TOL for e in errs.values()), (k, errs)
        else:       # its own rate: half or more of the hidden activation is dropped, which is an O(1) change of dW2 and dW1
            assert errs["d layers.1.weight"] > 100 * TOL and errs["d layers.0.weight"] > 100 * TOL, (k, errs)
    pad = torch.from_numpy(_pad_columns(net.seg_start, net.seg_width, net.n_cols))
    second = net.layers[1]
    assert bool((second.weight.grad.cpu()[:, pad] == 0.0).all()) and bool((second.weight.detach().cpu()[:, pad] == 0.0).all())


def test_block_diag_on_against_off_under_the_same_torch_seed(cuda, small):
    net, gd = _net(small, cuda).train(), small["gd"]
    with _switches(True, False):
        net.zero_grad(set_to_none=True)
        torch.cuda.manual_seed(1234)
        z_off = net(gd)
        z_off.backward(torch.ones_like(z_off) / z_off.numel())
        g_off = [p.grad.clone() for p in net.parameters()]
    with _switches(True, True):
        net.zero_grad(set_to_none=True)
        torch.cuda.manual_seed(1234)
        z_on = net(gd)
        z_on.backward(torch.ones_like(z_on) / z_on.numel())
        g_on = [p.grad.clone() for p in net.parameters()]
    torch.cuda.synchronize()
    assert R.rel_err(z_on, z_off) <= TOL
    for a, b in zip(g_on, g_off):
        assert R.rel_err(a, b) <= TOL
    S, C = net.seg_stride, net.out_channels
    assert R.rel_err(z_on[:, :C], small["truth"][0]["logits"]) <= TOL           # member 0 drops nothing
    assert R.rel_err(z_on[:, 5 * S:5 * S + C], small["truth"][5]["logits"]) > 100 * TOL


def test_eval_is_unaffected_by_the_rates(cuda, small):
    gd = small["gd"]
    plain = _net(small, cuda, dropout=0.0).eval()
    mixed = _net(small, cuda).eval()
    with torch.no_grad():
        want = plain(gd)
        with _switches(True, False):
            assert torch.equal(mixed(gd), want)                # today's path: the same bits
        with _switches(False, False):
            assert torch.equal(mixed(gd), want)
        with _switches(True, True):
            z = mixed(gd)
        assert R.rel_err(z, want) <= TOL
        S, C = mixed.seg_stride, mixed.out_channels
        for k in range(small["K"]):
            assert R.rel_err(z[:, k * S:k * S + C], small["truth"][k]["logits"]) <= TOL
        with _switches(True, True):
            val_k, pred = mixed.evaluate(gd, small["target"], small["val_bits"])
        assert pred.shape == (small["N"], small["K"]) and bool(torch.isfinite(val_k).all())


def test_torch_stream_dropout_takes_each_members_rate(cuda, small):
    """without fused dropout: F.dropout per column block; the rate-0 members are untouched, the others are not"""
    net, gd = _net(small, cuda).train(), small["gd"]
    S, C = net.seg_stride, net.out_channels
    with _switches(False, False), torch.no_grad():
        z = net(gd)
    for k in range(small["K"]):
        e = R.rel_err(z[:, k * S:k * S + C], small["truth"][k]["logits"])
        assert (e <= TOL) == (DROPOUT[k] == 0.0), (k, e)


def test_captured_step_with_mixed_rates(cuda):
    """loss + backward + MemberAdam(capturable=True).step() with both switches on, captured once after two eager warm-up
    steps and replayed three times.  Members are independent, so the rate-0 members hold the parameters of five eager steps
    bit for bit whatever the others draw; the others are finite and differ between two captured runs (fresh seeds per
    replay)."""
    s = _build(cuda, 8)
    gd, target, bits = s["gd"], s["target"], s["train_bits"]
    counts = R.counts_of(s["bits_host"][0], s["K"])
    was = conv._REUSE
    conv.enable_activation_reuse(False)                                # a replay must not depend on Python-side caches
    try:
        with _switches():
            nets = [_net(s, cuda).train() for _ in range(3)]
            opts = [MemberAdam(n_, LRS, amsgrad=True, capturable=True) for n_ in nets]

            def eager(net, opt):
                loss, _ = net.loss(gd, target, bits, counts=counts)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()

            for _ in range(5):
                eager(nets[0], opts[0])
            graphs = []
            for net, opt in zip(nets[1:], opts[1:]):
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        eager(net, opt)
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                opt.zero_grad(set_to_none=True)
                with torch.cuda.graph(graph):
                    loss, loss_k = net.loss(gd, target, bits, counts=counts)
                    loss.backward()
                    opt.step()
                for _ in range(3):
                    graph.replay()
                graphs.append(graph)
            torch.cuda.synchronize()
        for k in range(s["K"]):
            for name in _member_slices(nets[0], k):
                a, b, c = (_member_slices(n_, k)[name] for n_ in nets)
                a, b, c = (p.detach()[idx] for p, idx in (a, b, c))
                assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(c).all())
                if DROPOUT[k] == 0.0:
                    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (k, name)
                    assert torch.equal(a.contiguous().view(torch.int32), c.contiguous().view(torch.int32)), (k, name)
                elif name == "layers.1.weight":
                    assert not torch.equal(b, c), (k, name)
        assert int(opts[1].state[nets[1].layers[0].weight]["step"]) == 5
    finally:
        conv.enable_activation_reuse(was)
