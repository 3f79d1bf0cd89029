"""GPU tests of the per-label strategy: the grouped masked cross-entropy (libtgcn.so `tgcn_grouped_ce`,
pytextgcn_amd/csrc/perlabel.hip), `functional.grouped_masked_cross_entropy`, `PerLabelGCN` and
examples/perlabel_synthetic.py.

The kernel is held to the float64 restatement of tests/_perlabel_ref.py (which tests/test_perlabel_host.py holds to K
separate `CrossEntropyLoss('mean')` calls) at the project's bar, max|a - b| / max|b| <= 1e-5 (BASELINE.json; `TOL` of
tests/test_gpu_parity.py), with logits ~ 3 N(0, 1).  An fp32 evaluation of the same expressions on the CPU over every case of
`KERNEL_CASES` below sits at most 1.5e-7 (loss; n = 257, widths [257, 2], packed), 1.9e-7 (loss_k; n = 63, [64, 65, 1, 7],
packed), 3.2e-7 (dlogits; n = 70 000, [64, 65, 1, 7], packed) and 3.6e-7 (dbias; n = 63, [3, 4], packed) from float64 -- the
worst of each over all cases -- so the bar leaves more than ten-fold room at every shape used here and no operand is
rescaled.  `pred` is compared for equality: it is an arg-max over the same fp32
numbers.  The model is held to `oracle.gcn_oracle.GCNOracle` in float64, member by member."""
import os
import re
import subprocess
import sys

import pytest
import torch

import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, dense, functional, synth
from pytextgcn_amd import plan as plan_mod
from pytextgcn_amd.perlabel import PerLabelGCN, block_diag_xw, column_class_map, relabel

import _perlabel_ref as R
from _perlabel_ref import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = [[1], [3, 4], [64, 65, 1, 7], [257, 2]]
# aligned: starts at multiples of 4 with gaps (16-byte path); packed: back to back, n_cols = sum (4-byte path; [257, 2]: the
# wave-per-row kernel either way); packed4: back to back in 16-byte rows (the 16-byte path under unaligned starts)
LAYOUTS = ["aligned", "packed", "packed4"]
# n_cols per widths: 4 / 1 / 4 (4 lanes per row), 12 / 7 / 8 (4), 148 / 137 / 140 (64 lanes per row), 268 / 259 / 260 (wide)
KERNEL_CASES = [(n, w, lay) for n in (0, 1, 63, 65, 257, 5000) for w in WIDTHS for lay in LAYOUTS] + \
               [(70_000, [3, 4], "aligned"), (70_000, [64, 65, 1, 7], "packed")]      # 547 and 1024 workgroup partials


def case_of(n, widths, lay):
    return R.make_case(n, widths, lay == "aligned", seed=100 + n + 7 * len(widths) + len(lay), round_cols=lay == "packed4",
                       empty_group=n)


def raw_grouped_ce(dev, c, lay, want_grad=True, want_pred=True, use_route=True, use_map=True):
    """`tgcn_grouped_ce` on column slices of wider buffers (ld, ldd > n_cols): offset 4 and 8 spare columns keep 16-byte
    rows where the layout has them; the packed layout sits at offset 3 in rows of n_cols + 5 floats."""
    lib = _lib.load()
    n, C, K = c["logits"].size(0), c["n_cols"], len(c["widths"])
    off, extra = (3, 5) if lay == "packed" else (4, 8)
    wide = torch.full((n, C + extra), 55.0, device=dev)
    wide[:, off:off + C] = c["logits"].to(dev)
    logits = wide[:, off:off + C]
    dwide = torch.full((n, C + extra), 7.0, device=dev)
    dlogits = dwide[:, off:off + C]
    seg = functional.Segments.of(c["starts"], c["widths"], dev)
    counts = [int((c["mask"] & (c["group"] == k)).sum()) for k in range(K)]
    inv = torch.tensor([1.0 / v if v else 0.0 for v in counts], dtype=torch.float32, device=dev)
    t, m, g, rt, cm = (c[k].to(dev) for k in ("target", "mask", "group", "route", "class_map"))
    loss = torch.full((), -5.0, device=dev)
    loss_k = torch.full((K,), -5.0, device=dev)
    dbias = torch.full((C,), 7.0, device=dev)
    pred = torch.full((n,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(max(16, lib.tgcn_grouped_ce_workspace_bytes(n, C, K)), dtype=torch.uint8, device=dev)
    st = lib.tgcn_grouped_ce(
        logits.data_ptr(), C + extra, n, C, K, seg.host_start, seg.host_width, seg.dev_start.data_ptr(),
        seg.dev_width.data_ptr(), g.data_ptr(), rt.data_ptr() if use_route else None, t.data_ptr(), m.data_ptr(),
        inv.data_ptr(), cm.data_ptr() if use_map else None, loss.data_ptr(), loss_k.data_ptr(),
        dlogits.data_ptr() if want_grad else None, C + extra, dbias.data_ptr() if want_grad else None,
        pred.data_ptr() if want_pred else None, ws.data_ptr(), ws.numel(), plan_mod._stream_ptr(dev))
    _lib.check(st)
    torch.cuda.synchronize()
    return dict(loss=loss, loss_k=loss_k, dlogits=dlogits, dbias=dbias, pred=pred, dwide=dwide, off=off)


def _err(got, want):
    """max|got - want| / max|want|; against an all-zero (or empty) truth: max|got|, which must then be 0 to pass."""
    if want.numel() == 0 or float(want.abs().max()) == 0.0:
        return float(got.abs().max()) if got.numel() else 0.0
    return rel_err(got, want)


@pytest.mark.parametrize("n,widths,lay", KERNEL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_kernel_against_float64(cuda, n, widths, lay):
    c = case_of(n, widths, lay)
    C, K = c["n_cols"], len(widths)
    out = raw_grouped_ce(cuda, c, lay)
    loss, loss_k, d, db = R.grouped_ce(c["logits"], c["target"], c["mask"], c["group"], c["starts"], c["widths"])
    empty = torch.isnan(loss_k)
    got_k = out["loss_k"].cpu()
    assert torch.equal(torch.isnan(got_k), empty)                     # NaN exactly where the group has no selected row
    if K >= 2 and n >= 63:
        assert bool(empty[n % K]) and int(empty.sum()) == 1
    errs = {"loss": _err(out["loss"].reshape(1), loss.reshape(1)), "loss_k": _err(got_k[~empty], loss_k[~empty]),
            "dlogits": _err(out["dlogits"], d), "dbias": _err(out["dbias"], db)}
    print(f"grouped ce n={n} widths={widths} {lay}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    # exactly zero outside the row's segment, on unselected rows, on rows of group -1 and in pad columns
    inside = torch.zeros(n, C, dtype=torch.bool)
    for k, (s, w) in enumerate(zip(c["starts"], c["widths"])):
        inside[(c["mask"] & (c["group"] == k)).nonzero().flatten(), s:s + w] = True
    got_d = out["dlogits"].cpu()
    assert bool((got_d[~inside] == 0.0).all())
    pad = torch.ones(C, dtype=torch.bool)
    for s, w in zip(c["starts"], c["widths"]):
        pad[s:s + w] = False
    assert bool((out["dbias"].cpu()[pad] == 0.0).all())
    for k in torch.nonzero(empty).flatten().tolist():                 # a group nobody trains: no bias gradient either
        assert bool((out["dbias"].cpu()[c["starts"][k]:c["starts"][k] + widths[k]] == 0.0).all())
    if widths == [1]:                                                 # a parent with one child: loss 0, gradient 0
        assert float(out["loss"]) == 0.0 and float(got_d.abs().max() if n else 0.0) == 0.0
    # nothing outside the n_cols columns of the slice
    off = out["off"]
    assert bool((out["dwide"][:, :off] == 7.0).all()) and bool((out["dwide"][:, off + C:] == 7.0).all())
    # predictions: routed (route != group on most rows), first index on ties, mapped
    want = R.routed_pred(c["logits"], c["route"], c["starts"], c["widths"], c["class_map"])
    assert torch.equal(out["pred"].cpu(), want)
    if n >= 63:
        assert bool((want == -1).any()) and bool((c["route"] != c["group"]).any())
        s0 = c["starts"][int(c["route"][0])] if int(c["route"][0]) >= 0 else None
        assert s0 is None or int(out["pred"][0]) == int(c["class_map"][s0])       # the all-zero row: the segment's first class


@pytest.mark.parametrize("n,widths,lay", [(257, [3, 4], "aligned"), (65, [64, 65, 1, 7], "packed"), (63, [257, 2], "packed4")])
def test_kernel_optional_outputs_and_default_route(cuda, n, widths, lay):
    """Without `route` the prediction is taken in the training group; without `class_map` it is the column; the loss alone
    (no gradient, no prediction) is the same number bit for bit (fixed-order reductions)."""
    c = case_of(n, widths, lay)
    full = raw_grouped_ce(cuda, c, lay)
    plain = raw_grouped_ce(cuda, c, lay, want_grad=False, want_pred=True, use_route=False, use_map=False)
    assert torch.equal(plain["pred"].cpu(), R.routed_pred(c["logits"], c["group"], c["starts"], c["widths"]))
    bare = raw_grouped_ce(cuda, c, lay, want_grad=False, want_pred=False)
    for other in (plain, bare):
        assert torch.equal(other["loss"], full["loss"])
        assert torch.equal(other["loss_k"].view(torch.int32), full["loss_k"].view(torch.int32))
        assert bool((other["dwide"] == 7.0).all()) and bool((other["dbias"] == 7.0).all())       # untouched
    assert bool((bare["pred"] == -7).all())
    again = raw_grouped_ce(cuda, c, lay)                             # deterministic: the same bits run to run
    assert all(torch.equal(again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k],
                           full[k].view(torch.int32) if full[k].dtype == torch.float32 else full[k])
               for k in ("loss", "loss_k", "dlogits", "dbias", "pred"))


def test_invalid_arguments_are_refused(cuda):
    c = case_of(65, [3, 4], "aligned")
    lg, t, m, g = (c[k].to(cuda) for k in ("logits", "target", "mask", "group"))
    for starts, widths in (([0, 2], [3, 4]),            # overlapping
                           ([8, 0], [3, 4]),            # decreasing
                           ([0, 8], [3, 5]),            # past n_cols (12)
                           ([0, 8], [3, 0])):           # an empty segment
        with pytest.raises(ValueError, match="tgcn_grouped_ce"):
            functional.grouped_masked_cross_entropy(lg, t, m, g, starts, widths, counts=[1, 1])
    lib = _lib.load()
    seg = functional.Segments.of(c["starts"], c["widths"], cuda)
    inv = torch.ones(2, device=cuda)
    loss = torch.zeros((), device=cuda)
    ws = torch.empty(lib.tgcn_grouped_ce_workspace_bytes(65, 12, 2), dtype=torch.uint8, device=cuda)
    args = lambda ld, ws_bytes: (lg.data_ptr(), ld, 65, 12, 2, seg.host_start, seg.host_width, seg.dev_start.data_ptr(),
                                 seg.dev_width.data_ptr(), g.data_ptr(), None, t.data_ptr(), m.data_ptr(), inv.data_ptr(), None,
                                 loss.data_ptr(), None, None, 12, None, None, ws.data_ptr(), ws_bytes, plan_mod._stream_ptr(cuda))
    assert lib.tgcn_grouped_ce(*args(11, ws.numel())) == _lib.E_INVALID          # ld < n_cols
    assert lib.tgcn_grouped_ce(*args(12, 16)) == _lib.E_WORKSPACE
    assert lib.tgcn_grouped_ce(*args(12, ws.numel())) == _lib.OK
    # targets and groups of the selected rows are range-checked once per object and version
    bad = t.clone()
    row = int(torch.nonzero(m & (g == 0))[0])
    bad[row] = 3                                                      # group 0 has 3 classes
    with pytest.raises(IndexError, match="out of bounds"):
        functional.grouped_masked_cross_entropy(lg, bad, m, g, c["starts"], c["widths"])
    with pytest.raises(IndexError, match="group"):
        functional.grouped_masked_cross_entropy(lg, t, m, torch.full_like(g, 2), c["starts"], c["widths"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,widths,lay,scale", [(257, [3, 4], "packed", 2.5), (5000, [64, 65, 1, 7], "aligned", 2.5),
                                                (65, [257, 2], "aligned", 1.0)])
def test_functional_backward_scales_and_leaves_its_notes(cuda, n, widths, lay, scale):
    """`(loss * 2.5).backward()` through the autograd node: the gradient, the column sums found by the node that stands where
    the last propagate step stands (no second pass over dlogits), and the zero-row note."""
    c = case_of(n, widths, lay)
    lg0, t, m, g = (c[k].to(cuda) for k in ("logits", "target", "mask", "group"))
    seen = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, grad):
            seen["g"] = grad
            seen["known"] = plan_mod._known_colsum(grad)
            seen["colsum"] = plan_mod.colsum(grad)
            seen["keep"] = plan_mod.known_nonzero_rows(grad)
            return grad

    lg = lg0.clone().requires_grad_()
    loss, loss_k, pred = functional.grouped_masked_cross_entropy(Probe.apply(lg), t, m, g, c["starts"], c["widths"],
                                                                 return_pred=True)
    assert not loss_k.requires_grad and not pred.requires_grad
    (loss * scale if scale != 1.0 else loss).backward()
    want_loss, want_k, d, db = R.grouped_ce(c["logits"], c["target"], c["mask"], c["group"], c["starts"], c["widths"])
    ok = ~torch.isnan(want_k)
    assert abs(loss.item() - float(want_loss)) <= TOL * abs(float(want_loss))
    assert torch.equal(torch.isnan(loss_k.cpu()), ~ok) and rel_err(loss_k.cpu()[ok], want_k[ok]) <= TOL
    assert torch.equal(pred.cpu(), R.routed_pred(c["logits"], c["group"], c["starts"], c["widths"]))
    assert rel_err(lg.grad, d * scale) <= TOL
    assert bool((lg.grad.cpu()[d == 0] == 0.0).all())
    assert seen["known"] is not None and seen["colsum"].data_ptr() == seen["known"].data_ptr()        # no second pass
    assert seen["colsum"].shape == (c["n_cols"],) and rel_err(seen["colsum"], db * scale) <= TOL
    assert seen["keep"] is not None and torch.equal(seen["keep"].cpu(), c["mask"] & (c["group"] >= 0))
    with pytest.raises(RuntimeError, match="already run"):            # single use: the buffer was scaled in place
        lg2 = lg0.clone().requires_grad_()
        l2, _ = functional.grouped_masked_cross_entropy(lg2, t, m, g, c["starts"], c["widths"])
        l2.backward(retain_graph=True)
        l2.backward()
    # without autograd: the same loss bits, no gradient buffers
    with torch.no_grad():
        l3, k3 = functional.grouped_masked_cross_entropy(lg0, t, m, g, c["starts"], c["widths"])
    assert torch.equal(l3, loss.detach()) and torch.equal(k3.view(torch.int32), loss_k.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
COUNTS = [2, 5, 1]
TOP_OF = torch.tensor([0, 0, 1, 1, 1, 1, 1, 2])            # global class -> top-level label: 2, 5 and 1 classes


@pytest.fixture(scope="module")
def small(cuda):
    """A 400-node synth graph with a two-level label, K = 3 members of hidden width 8 with random biases, the concatenated
    network built from them, and the float64 oracle's logits, losses and gradients member by member (computed once)."""
    from oracle import gcn_oracle as O
    N, h = 400, 8
    g = synth.word_doc_graph(N, 3000, seed=7, n_classes=8)
    docs = torch.arange(N) >= g.n_vocab
    group, target, counts, cmap = relabel(g.y, TOP_OF[g.y], docs)
    assert counts == COUNTS and cmap == [[0, 1], [2, 3, 4, 5, 6], [7]]
    torch.manual_seed(3)
    members = [pkg.GCN(N, c, n_hidden_gcn=h, dropout=0.0) for c in COUNTS]
    with torch.no_grad():
        for mem in members:
            for layer in mem.layers:
                layer.bias.uniform_(-0.5, 0.5)
    g64 = pkg.Data(x=g.x.double(), edge_index=g.edge_index, edge_attr=g.edge_attr.double())
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    truth = []
    for k, mem in enumerate(members):
        ref = O.GCNOracle(N, COUNTS[k], n_hidden_gcn=h, dropout=0.0)
        ref.load_state_dict(mem.state_dict())
        ref = ref.double().train()
        z = ref(g64)
        sel = g.train_mask & (group == k)
        lk = crit(z[sel], target[sel])
        lk.backward()
        truth.append(dict(logits=z.detach(), loss=lk.item(), grads={n_: p.grad.clone() for n_, p in ref.named_parameters()}))
    net = PerLabelGCN.from_members(members).to(cuda).float()
    gd = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(cuda)
    return dict(g=g, gd=gd, group=group, target=target, cmap=cmap, members=members, truth=truth, net=net, h=h, N=N)


def test_eval_logits_of_every_segment_against_the_oracle_and_the_member(cuda, small):
    net, gd = small["net"].eval(), small["gd"]
    with torch.no_grad():
        z = net(gd)
        assert z.shape == (small["N"], net.n_cols)
        for k, (s, c) in enumerate(zip(net.seg_start, net.seg_width)):
            assert rel_err(z[:, s:s + c], small["truth"][k]["logits"]) <= TOL
            mine = small["members"][k].to(cuda).eval()(gd)
            assert rel_err(z[:, s:s + c], mine.double()) <= TOL
        # `rows`: the rows that are read hold the same numbers
        rows = gd.test_mask | gd.val_mask
        zr = net(gd, rows=rows)
        assert rel_err(zr[rows], z[rows].double()) <= 1e-6
        # routed prediction (eval_perlabel.py:71-78): by the true top label here; mapped to the global class
        route = small["group"].to(cuda)
        cm = column_class_map(small["cmap"], cuda)
        pred = net.predict(gd, route, cm)
        want = R.routed_pred(z, small["group"], net.seg_start, net.seg_width, cm)
        assert torch.equal(pred.cpu(), want) and bool((pred.cpu()[small["group"] < 0] == -1).all())
        assert bool((pred.cpu()[small["group"] == 2] == 7).all())                 # the one-class member


def test_one_training_step_against_k_oracle_models(cuda, small):
    net, gd, h = small["net"].train(), small["gd"], small["h"]
    net.zero_grad(set_to_none=True)
    target, group = small["target"].to(cuda), small["group"].to(cuda)
    loss, loss_k = net.loss(gd, target, gd.train_mask, group)
    loss.backward()
    torch.cuda.synchronize()
    truth = small["truth"]
    assert abs(float(loss) - sum(t["loss"] for t in truth)) <= TOL * sum(t["loss"] for t in truth)
    first, second = net.layers
    for k, (s, c) in enumerate(zip(net.seg_start, net.seg_width)):
        want = truth[k]
        assert abs(float(loss_k[k]) - want["loss"]) <= TOL * max(want["loss"], 1e-30), (k, float(loss_k[k]), want["loss"])
        got = {"layers.0.weight": first.weight.grad[:, k * h:(k + 1) * h], "layers.0.bias": first.bias.grad[k * h:(k + 1) * h],
               "layers.1.weight": second.weight.grad[:, s:s + c], "layers.1.bias": second.bias.grad[s:s + c]}
        for name, gr in got.items():
            e = rel_err(gr, want["grads"][name])
            print(f"member {k} {name}: {e:.2e}")
            assert e <= TOL, (k, name, e)
    assert truth[2]["loss"] == 0.0                                                # one class: nothing to learn
    # pad columns: exactly zero gradient for the weight and the bias (nothing off the diagonal is stored)
    pad = torch.ones(net.n_cols, dtype=torch.bool)
    for s, c in zip(net.seg_start, net.seg_width):
        pad[s:s + c] = False
    assert bool((second.weight.grad.cpu()[:, pad] == 0.0).all()) and bool((second.bias.grad.cpu()[pad] == 0.0).all())
    # and the package's fused Adam keeps them zero
    opt = pkg.optim.Adam(net.parameters(), lr=0.05)
    opt.step()
    assert bool((second.weight.detach().cpu()[:, pad] == 0.0).all()) and bool((second.bias.detach().cpu()[pad] == 0.0).all())
    net.load_state_dict(PerLabelGCN.from_members(small["members"]).state_dict())   # (the fixture is shared)


def test_fused_dropout_is_xw_dropout_per_group_bit_for_bit(cuda, small):
    net, h, N = small["net"], small["h"], small["N"]
    starts, widths, p = net.seg_start, net.seg_width, 0.4
    gen = torch.Generator().manual_seed(17)
    H0 = torch.randn(N, 3 * h, generator=gen).to(cuda)
    W0 = net.layers[1].weight.detach().clone()
    G = torch.randn(N, net.n_cols, generator=gen).to(cuda)
    seeds = torch.tensor([0x1234567890ABCDE, -77, (1 << 40) + 12345], dtype=torch.int64, device=cuda)
    H, W = H0.clone().requires_grad_(), W0.clone().requires_grad_()
    out = block_diag_xw(H, W, starts, widths, p, seeds)
    out.backward(G)
    for k, (s, c) in enumerate(zip(starts, widths)):
        Hk = H0[:, k * h:(k + 1) * h].contiguous().requires_grad_()
        Wk = W0[:, s:s + c].contiguous().requires_grad_()
        ok = dense.xw_dropout(Hk, Wk, p, seeds[k:k + 1])
        # the gradient as the propagate step hands it to a member GCN: rows of 4 j floats (the weight-gradient product picks
        # its kernel, hence its summation order, by the 16-byte alignment of its operands' rows)
        ok.backward(torch.nn.functional.pad(G[:, s:s + c], (0, (-c) % 4))[:, :c])
        assert torch.equal(out[:, s:s + c], ok), k
        assert torch.equal(H.grad[:, k * h:(k + 1) * h], Hk.grad), k
        assert torch.equal(W.grad[:, s:s + c], Wk.grad), k
    # the model takes that path under the switch (and only in training), and the switch is put back
    from pytextgcn_amd import models
    was = models._FUSED_DROPOUT
    try:
        pkg.enable_fused_dropout()
        net.dropout = p
        z1, z2 = net.train()(small["gd"]), net(small["gd"])
        assert bool(torch.isfinite(z1).all()) and not torch.equal(z1, z2)         # a fresh seed per forward
        with torch.no_grad():
            assert torch.equal(net.eval()(small["gd"]), net(small["gd"]))
    finally:
        pkg.enable_fused_dropout(was)
        net.dropout = 0.0
    assert models._FUSED_DROPOUT == was


def test_example_trains_every_group(cuda):
    """`examples/perlabel_synthetic.py --docs 600 --epochs 30` in a fresh child process: exit 0, every non-empty group's final
    training loss below its first, and the routed evaluation prints its two figures."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "perlabel_synthetic.py"), "--docs", "600", "--epochs",
                          "30"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0, (out[-1500:], res.stderr.decode()[-3000:])
    rows = re.findall(r"^group (\d+): \d+ classes, first loss\s+([-\d.naninf]+), final loss\s+([-\d.naninf]+)", out, flags=re.M)
    assert len(rows) >= 2, out[-1500:]
    for k, first, last in rows:
        if first != "nan":
            assert float(last) < float(first), (k, first, last)
    assert re.search(r"test accuracy: [\d.]+\s+test f1-macro: [\d.]+", out), out[-800:]
