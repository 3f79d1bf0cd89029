"""GPU tests of the cross-validation sweep cell: the member masked cross-entropy (libtgcn.so `tgcn_member_ce`) and Adam with
one learning rate per column block (`tgcn_adam_members`) of pytextgcn_amd/csrc/crossval.hip,
`functional.member_masked_cross_entropy`, `CrossValGCN` and `MemberAdam`.

The loss kernel is held to the float64 restatement of tests/_crossval_ref.py (which tests/test_crossval_host.py holds to K
separate `CrossEntropyLoss('mean')` calls) at the project's bar, max|a - b| / max|b| <= 1e-5 (BASELINE.json).  Its arithmetic
is k_masked_ce's, which tests/test_gpu_train_kernels.py measured at 1.2e-7 (loss), 1.9e-6 (gradient rows, each against its OWN
largest entry) and 7.9e-7 (bias gradient) over the same value rows: the bar leaves five-fold room and more.  On those value
rows every gradient row of every member is ALSO held to its own scale.  `pred`, the zeros, the NaN of an empty member and the
poison around the buffers are compared for equality.  Adam is compared bit for bit: the update is elementwise, so member
k's column block must be what `tgcn_adam_step` with lr[k] makes of a contiguous copy of it.  The network is held to
`oracle.gcn_oracle.GCNOracle` in float64, member by member."""
import ctypes

import numpy as np
import pytest
import torch

import _crossval_ref as R
import _train_cases as tc
import pytextgcn_amd as pkg
from pytextgcn_amd import _lib, conv, dense, functional, synth
from pytextgcn_amd import plan as plan_mod
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits
from pytextgcn_amd.perlabel import block_diag_xw

pytestmark = pytest.mark.gpu
TOL = 1e-5
F32, I64 = torch.float32, torch.int64
CLASSES = (1, 2, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300)
MEMBERS = (1, 3, 12, 64)
ROWS = (0, 1, 63, 65, 257, 5000)
OUTPUTS = tuple((lk, gr, pr) for lk in (True, False) for gr in ("none", "grad", "dbias") for pr in (True, False))


def strides_of(C):
    r4 = (C + 3) & ~3
    return (C, r4, r4 + 4)


def _err(got, want):
    """max|got - want| / max|want|; against an all-zero (or empty) truth: max|got|, which must then be 0 to pass."""
    if want.numel() == 0 or float(want.abs().max()) == 0.0:
        return float(got.abs().max()) if got.numel() else 0.0
    return R.rel_err(got, want)


def raw_member_ce(dev, c, lay, want_loss_k=True, grad="dbias", want_pred=True):
    """`tgcn_member_ce` through ctypes on column slices of wider, poisoned buffers: "v4" puts the slice at offset 4 in rows
    of n_cols + 8 floats (16-byte rows when the stride is a multiple of 4), "scalar" at offset 3 in rows of n_cols + 5."""
    lib = _lib.load()
    K, C, S = c["K"], c["C"], c["S"]
    n, W = c["logits"].size(0), K * S
    off, extra = (3, 5) if lay == "scalar" else (4, 8)
    wide = torch.full((n + 1, W + extra), float("nan"), device=dev)
    wide[:n, off:off + W] = c["logits"].to(dev)
    dwide = torch.full((n + 1, W + extra), R.FILL, device=dev)
    assert wide.data_ptr() % 16 == 0 and dwide.data_ptr() % 16 == 0
    logits, dlogits = wide[:, off:off + W], dwide[:, off:off + W]
    counts = R.counts_of(c["bits"], K)
    inv = torch.tensor([1.0 / v if v else 0.0 for v in counts], dtype=F32, device=dev)
    target = torch.zeros(max(n, 1), dtype=I64, device=dev)
    bits = torch.zeros(max(n, 1), dtype=I64, device=dev)
    target[:n], bits[:n] = c["target"].to(dev), c["bits"].to(dev)
    loss = torch.full((2,), -5.0, device=dev)
    loss_k = torch.full((K + 1,), -5.0, device=dev)
    dbias = torch.full((W + 4,), R.FILL, device=dev)
    pred = torch.full((n + 1, K), -7, dtype=torch.int32, device=dev)
    ws_bytes = lib.tgcn_member_ce_workspace_bytes(n, K, C)
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device=dev)
    st = lib.tgcn_member_ce(
        logits.data_ptr(), W + extra, n, K, C, S, target.data_ptr(), bits.data_ptr(), inv.data_ptr(), loss.data_ptr(),
        loss_k.data_ptr() if want_loss_k else None, dlogits.data_ptr() if grad != "none" else None, W + extra,
        dbias.data_ptr() if grad == "dbias" else None, pred.data_ptr() if want_pred else None, ws.data_ptr(), ws_bytes,
        plan_mod._stream_ptr(dev))
    assert st == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), loss_k=loss_k.cpu(), dwide=dwide.cpu(), dbias=dbias.cpu(), pred=pred.cpu(), off=off, W=W, n=n,
                v4=R.mce_v4(S, W + extra, W + extra, off, off, grad != "none"))


def check(c, out, ref, want_loss_k=True, grad="dbias", want_pred=True, rows_to_own_scale=False, worst=None):
    """everything one call could have written, against the float64 reference; returns the four figures"""
    K, C, S, n, W, off = c["K"], c["C"], c["S"], out["n"], out["W"], out["off"]
    loss, loss_k, d, db, pred = ref
    empty = torch.isnan(loss_k)
    errs = {"loss": _err(out["loss"][:1], loss.reshape(1))}
    assert float(out["loss"][1]) == -5.0
    if want_loss_k:
        got_k = out["loss_k"][:K]
        assert torch.equal(torch.isnan(got_k), empty), (got_k, loss_k)       # NaN exactly at the members nobody selects
        errs["loss_k"] = _err(got_k[~empty], loss_k[~empty])
        assert float(out["loss_k"][K]) == -5.0
    else:
        assert bool((out["loss_k"] == -5.0).all())
    dwide = out["dwide"]
    if grad == "none":
        assert bool((dwide == R.FILL).all())
    else:
        got_d = dwide[:n, off:off + W]
        errs["dlogits"] = _err(got_d, d)
        assert bool((got_d[d == 0] == 0.0).all())        # other segments, unselected rows, pad columns: exactly 0.0f
        sel = torch.stack([R.selected(c["bits"], k) for k in range(K)], 1) if n else torch.zeros(0, K, dtype=torch.bool)
        outside = torch.ones(n, K, S, dtype=torch.bool)
        outside[:, :, :C] = ~sel[:, :, None]
        assert bool((got_d.reshape(n, K, S)[outside] == 0.0).all())
        assert bool((dwide[:n, :off] == R.FILL).all()) and bool((dwide[:n, off + W:] == R.FILL).all())     # the poison
        assert bool((dwide[n:] == R.FILL).all())
        if rows_to_own_scale:                             # every (row, member) against its own largest entry
            errs["row"] = R.row_err(got_d.reshape(n * K, S), d.reshape(n * K, S))
    if grad == "dbias":
        errs["dbias"] = _err(out["dbias"][:W], db)
        pad = torch.ones(K, S, dtype=torch.bool)
        pad[:, :C] = False
        pad[empty] = True                                 # a member nobody trains: no bias gradient either
        assert bool((out["dbias"][:W][pad.flatten()] == 0.0).all())
        assert bool((out["dbias"][W:] == R.FILL).all())
    else:
        assert bool((out["dbias"] == R.FILL).all())
    if want_pred:
        assert torch.equal(out["pred"][:n], pred)         # every row, selected or not; first index on ties
        assert bool((out["pred"][n:] == -7).all())
    else:
        assert bool((out["pred"] == -7).all())
    if worst is not None:
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert all(v <= TOL for v in errs.values()), (c["K"], C, S, n, errs)
    return errs


def leaf_of(C, v4):
    return R.mce_leaf(C)[:2] + (v4,)


LEAVES = tuple((lpr, kpl, v4) for v4 in (True, False) for lpr, kpl in R.LEAF_C)
leaf_id = lambda leaf: f"lpr{leaf[0]}-kpl{leaf[1]}-{'v4' if leaf[2] else 'scalar'}"


@pytest.mark.parametrize("C", CLASSES)
def test_member_ce_every_class_count_and_stride(cuda, C):
    """K = 3, 257 rows; the three strides {C, C rounded up to 4, that + 4} in 16-byte rows (the 16-byte leaf where the stride
    is a multiple of 4 -- whatever C is) and at offset 3 in rows of n_cols + 5 floats (the 4-byte leaf)"""
    worst, leaves = {}, set()
    for S in strides_of(C):
        c, ref = R.make_case(257, 3, C, S), R.reference(257, 3, C, S)
        for lay in ("v4", "scalar"):
            out = raw_member_ce(cuda, c, lay)
            assert out["v4"] == (lay == "v4" and S % 4 == 0)
            leaves.add(leaf_of(C, out["v4"]))
            check(c, out, ref, worst=worst)
    assert leaves == {leaf_of(C, True), leaf_of(C, False)}
    print(f"\nmember ce C={C}: worst {worst}")


@pytest.mark.parametrize("K", MEMBERS)
def test_member_ce_member_and_row_counts(cuda, K):
    """K in {1, 3, 12, 64} x n in {0, 1, 63, 65, 257, 5000}; the class count and the stride change from case to case (wide
    members stay with few members: the float64 reference of 5000 x 64 x 300 would not be small)"""
    classes = {1: (300, 257, 256, 2, 1, 129), 3: (128, 129, 256, 257, 300, 65), 12: (32, 33, 64, 65, 5, 17),
               64: (1, 2, 17, 16, 33, 5)}[K]
    worst = {}
    for i, (n, C) in enumerate(zip(ROWS, classes)):
        S = strides_of(C)[(i + K) % 3]
        c, ref = R.make_case(n, K, C, S), R.reference(n, K, C, S)
        if K >= 2 and n >= 63:
            assert bool(torch.isnan(ref[1][c["empty"]])) and int(torch.isnan(ref[1]).sum()) == 1
        check(c, raw_member_ce(cuda, c, "v4" if i % 2 == 0 else "scalar"), ref, worst=worst)
    print(f"\nmember ce K={K}: worst {worst}")


@pytest.mark.parametrize("leaf", LEAVES, ids=leaf_id)
def test_member_ce_optional_outputs_of_every_leaf(cuda, leaf):
    """every combination of loss_k, dlogits (+ dbias) and pred on one case per leaf; the loss is the same number bit for bit
    whatever else is asked for (fixed-order reductions), and so is a second run"""
    C = R.LEAF_C[leaf[:2]]
    S = strides_of(C)[1] if leaf[2] else C
    lay = "v4" if leaf[2] else "scalar"
    c, ref = R.make_case(257, 3, C, S), R.reference(257, 3, C, S)
    full = raw_member_ce(cuda, c, lay)
    for lk, gr, pr in OUTPUTS:
        out = raw_member_ce(cuda, c, lay, lk, gr, pr)
        assert leaf_of(C, out["v4"]) == leaf
        check(c, out, ref, lk, gr, pr)
        assert torch.equal(out["loss"].view(torch.int32), full["loss"].view(torch.int32))
        for key, asked in (("loss_k", lk), ("dwide", gr != "none"), ("dbias", gr == "dbias"), ("pred", pr)):
            if asked:
                assert torch.equal(out[key].view(torch.int32), full[key].view(torch.int32)), key


@pytest.mark.parametrize("leaf", LEAVES, ids=leaf_id)
def test_member_ce_value_edges(cuda, leaf):
    """the value rows of tests/_train_cases.py -- logits at and scaled to +-80 / +-1e4, -inf columns, all-equal rows, one
    selected row, ties at the hand-over columns of both column maps -- with every gradient row held to its own scale"""
    C = R.LEAF_C[leaf[:2]]
    S = strides_of(C)[2] if leaf[2] else strides_of(C)[0]
    worst = {}
    for values in tc.EDGE_VALUES:
        c, ref = R.make_case(257, 3, C, S, values), R.reference(257, 3, C, S, values)
        out = raw_member_ce(cuda, c, "v4" if leaf[2] else "scalar")
        assert leaf_of(C, out["v4"]) == leaf
        check(c, out, ref, rows_to_own_scale=True, worst=worst)
    print(f"\nmember ce edges {leaf_id(leaf)}: worst {worst}")


@pytest.mark.parametrize("leaf", LEAVES, ids=leaf_id)
def test_member_ce_second_grid_stride(cuda, leaf):
    """one row more than the capped grid covers in one stride (64 members: 32 workgroups each), one-hot rows that name
    themselves so that a wrong row assignment is a wrong row"""
    K, C = 64, R.LEAF_C[leaf[:2]]
    S = strides_of(C)[1] if leaf[2] else C
    n = R.mce_rows_past_cap(K, C)
    assert n == 32 * 2 * 4 * (64 // leaf[0]) + 1
    c, ref = R.make_case(n, K, C, S, "onehot"), R.reference(n, K, C, S, "onehot")
    out = raw_member_ce(cuda, c, "v4" if leaf[2] else "scalar")
    assert leaf_of(C, out["v4"]) == leaf
    print(f"\nmember ce stride {leaf_id(leaf)} n={n}: {check(c, out, ref)}")


ONE_MEMBER = [(C, tc.N_SMALL) for v4 in (True, False) for C in tc.LEAF_WIDTH[v4]] + \
             [(C, tc.CE_BLOCKS * tc.ce_leaf(C, False)[3] + 37) for C in (16, 260)]


@pytest.mark.parametrize("C,n", ONE_MEMBER, ids=[f"C{C}-n{n}" for C, n in ONE_MEMBER])
def test_one_member_without_pad_is_the_flat_masked_ce_bit_for_bit(cuda, C, n):
    """K = 1, seg_stride == C, bits = mask: `tgcn_member_ce` against `tgcn_masked_ce_grad` on the same logits, targets and
    mask -- one width per leaf of both column maps at 257 rows, and C = 16 / C = 260 one ragged row group past the launch cap
    (mce_cap(1) == kCeBlocks: the same grid).  Both kernels are the one row body of csrc/masked_ce.h under two views, so
    the loss, the gradient and the arg-max are the same bits, and so is the bias gradient on the register path
    (C <= 256), where both sides reduce the workgroups' column sums in k_colsum_final's order.  Wider members: see below."""
    lib = _lib.load()
    assert R.mce_cap(1) == tc.CE_BLOCKS
    inp = tc.ce_inputs(C, n, "randn")
    logits = torch.from_numpy(inp["x"]).to(cuda)
    target = torch.from_numpy(inp["target"]).to(cuda)
    mask = torch.from_numpy(inp["mask"].astype(np.uint8)).to(cuda)
    assert logits.data_ptr() % 16 == 0
    stream = plan_mod._stream_ptr(cuda)
    new = lambda *shape, dtype=F32: torch.full(shape, R.FILL, dtype=dtype, device=cuda)
    # the flat kernel
    f_loss, f_d, f_db, f_pred = new(1), new(n, C), new(C), new(n, dtype=I64)
    ws_bytes = lib.tgcn_masked_ce_grad_workspace_bytes(n, C)
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device=cuda)
    assert lib.tgcn_masked_ce_grad(logits.data_ptr(), C, n, C, target.data_ptr(), mask.data_ptr(), ctypes.c_float(inp["inv_count"]),
                                   f_loss.data_ptr(), f_d.data_ptr(), C, f_db.data_ptr(), f_pred.data_ptr(), ws.data_ptr(),
                                   ws_bytes, stream) == _lib.OK, lib.tgcn_last_error()
    # one member, no pad
    m_loss, m_loss_k, m_d, m_db, m_pred = new(1), new(1), new(n, C), new(C), new(n, 1, dtype=torch.int32)
    inv = torch.tensor([inp["inv_count"]], dtype=F32, device=cuda)
    bits = mask.to(I64)                                                # uint64 words: bit 0 is the mask
    ws_bytes = lib.tgcn_member_ce_workspace_bytes(n, 1, C)
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device=cuda)
    assert lib.tgcn_member_ce(logits.data_ptr(), C, n, 1, C, C, target.data_ptr(), bits.data_ptr(), inv.data_ptr(),
                              m_loss.data_ptr(), m_loss_k.data_ptr(), m_d.data_ptr(), C, m_db.data_ptr(), m_pred.data_ptr(),
                              ws.data_ptr(), ws_bytes, stream) == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    words = lambda t: t.view(torch.int32)
    equal = {"loss": torch.equal(words(m_loss), words(f_loss)), "loss_k": torch.equal(words(m_loss_k), words(f_loss)),
             "dlogits": torch.equal(words(m_d), words(f_d)), "dbias": torch.equal(words(m_db), words(f_db)),
             "pred": torch.equal(m_pred[:, 0].to(I64), f_pred)}
    e_db = _err(m_db.cpu(), f_db.cpu())
    print(f"\none member C={C} n={n}: bit-equal {equal}; dbias max|a - b| / max|b| = {e_db:.2e}")
    assert bool(torch.isfinite(f_loss).all()) and float(f_d.abs().max()) > 0 and int(f_pred.max()) > 0
    assert equal["loss"] and equal["loss_k"] and equal["dlogits"] and equal["pred"], equal
    # Wider than 256 classes the bias gradient is a second pass over dlogits, and the two sides sum its rows in another
    # order (launch_colsum against k_member_colsum_wide): measured before the kernels shared their body, 2.8e-7 (C = 260),
    # 1.9e-7 (C = 257) and 2.4e-7 (C = 260 at 16 421 rows) apart, everything else bit-equal.  Held to the file's bar.
    assert equal["dbias"] if C <= 256 else e_db <= TOL, (equal, e_db)


def test_functional_backward_scales_and_leaves_its_notes(cuda):
    """`(loss * 2.5).backward()` through the autograd node: the gradient, the column sums found by the node that stands where
    the last propagate step stands (no second pass over dlogits), and the zero-row note with keep = bits != 0"""
    n, K, C, S, scale = 257, 6, 5, 8, 2.5
    c = R.make_case(n, K, C, S)
    want_loss, want_k, d, db, want_pred = R.reference(n, K, C, S)
    lg0, t, b = c["logits"].to(cuda), c["target"].to(cuda), c["bits"].to(cuda)
    seen = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, grad):
            seen["known"] = plan_mod._known_colsum(grad)
            seen["colsum"] = plan_mod.colsum(grad)
            seen["keep"] = plan_mod.known_nonzero_rows(grad)
            return grad

    lg = lg0.clone().requires_grad_()
    loss, loss_k, pred = functional.member_masked_cross_entropy(Probe.apply(lg), t, b, K, C, S, return_pred=True)
    assert not loss_k.requires_grad and not pred.requires_grad and pred.dtype == torch.int32 and pred.shape == (n, K)
    (loss * scale).backward()
    ok = ~torch.isnan(want_k)
    assert abs(loss.item() - float(want_loss)) <= TOL * abs(float(want_loss))
    assert torch.equal(torch.isnan(loss_k.cpu()), ~ok) and R.rel_err(loss_k.cpu()[ok], want_k[ok]) <= TOL
    assert torch.equal(pred.cpu(), want_pred)
    assert R.rel_err(lg.grad, d * scale) <= TOL and bool((lg.grad.cpu()[d == 0] == 0.0).all())
    assert seen["known"] is not None and seen["colsum"].data_ptr() == seen["known"].data_ptr()        # no second pass
    assert seen["colsum"].shape == (K * S,) and R.rel_err(seen["colsum"], db * scale) <= TOL
    assert seen["keep"] is not None and torch.equal(seen["keep"].cpu(), c["bits"] != 0)
    with pytest.raises(RuntimeError, match="already run"):            # single use: the buffer was scaled in place
        lg2 = lg0.clone().requires_grad_()
        l2, _ = functional.member_masked_cross_entropy(lg2, t, b, K, C, S)
        l2.backward(retain_graph=True)
        l2.backward()
    with torch.no_grad():                                             # without autograd: the same loss bits
        l3, k3 = functional.member_masked_cross_entropy(lg0, t, b, K, C, S)
    assert torch.equal(l3, loss.detach()) and torch.equal(k3.view(torch.int32), loss_k.view(torch.int32))
    bad = t.clone()
    bad[int(torch.nonzero(b != 0)[0])] = C                            # range-checked once per (bits, target) object
    with pytest.raises(IndexError, match="out of bounds"):
        functional.member_masked_cross_entropy(lg0, bad, b, K, C, S)
    with pytest.raises(ValueError, match="seg_stride"):
        functional.member_masked_cross_entropy(lg0, t, b, K, C, S + 4)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# Adam with one learning rate per member
# ----------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 4, 100, 128)
ADAM_ROWS = (1, 7, 1025)
AMS_WD = ((True, 0.0), (False, 0.01), (True, 0.01), (False, 0.0))
BETA1, BETA2, EPS, STEPS = 0.9, 0.999, 1e-8, 3


def _rates(K):
    return [(0.1, 0.05, 0.01, 0.001)[k % 4] * (1.0 + k // 4) for k in range(K)]


def _adam_state(n_rows, n_cols, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    f = lambda: torch.randn(n_rows, n_cols, generator=gen)
    p, m = f(), f()
    v = torch.rand(n_rows, n_cols, generator=gen) + 0.1
    vmax = v * (0.5 + torch.rand(n_rows, n_cols, generator=gen))
    grads = [f() * s for s in (1.0, 0.1, 3.0)[:STEPS]]
    return [t.to(dev) for t in (p, m, v, vmax)], [g.to(dev) for g in grads]


def _run_adam_members(lib, dev, n_rows, width, K, ams, wd, lrs, check_blocks=True):
    """three steps of the host form, of the capturable form and of K `tgcn_adam_step` calls on contiguous copies of the
    column blocks; everything compared bit for bit after every step"""
    n_cols = width * K
    state, grads = _adam_state(n_rows, n_cols, 1000 * width + 10 * K + n_rows, dev)
    host = [t.clone() for t in state]
    capt = [t.clone() for t in state]
    blocks = [[t[:, k * width:(k + 1) * width].clone() for t in state] for k in range(K)] if check_blocks else None
    lr_host = (ctypes.c_double * K)(*lrs)
    step_dev = torch.zeros((), dtype=I64, device=dev)
    scalars = torch.full((K + 2,), R.FILL, dtype=F32, device=dev)
    stream = plan_mod._stream_ptr(dev)
    ptrs = lambda ts: [t.data_ptr() for t in ts[:3]] + [ts[3].data_ptr() if ams else None]
    for step, g in enumerate(grads, 1):
        p, m, v, x = ptrs(host)
        assert lib.tgcn_adam_members(p, g.data_ptr(), m, v, x, n_rows, n_cols, width, K, lr_host, BETA1, BETA2, EPS, wd, step,
                                     stream) == _lib.OK, lib.tgcn_last_error()
        p, m, v, x = ptrs(capt)
        assert lib.tgcn_adam_members_capturable(p, g.data_ptr(), m, v, x, n_rows, n_cols, width, K, lr_host, BETA1, BETA2, EPS,
                                                wd, step_dev.data_ptr(), scalars.data_ptr(), stream) == _lib.OK
        if blocks is not None:
            for k, blk in enumerate(blocks):
                gk = g[:, k * width:(k + 1) * width].clone()              # (a 16-byte aligned copy: tgcn_adam_step asks for one)
                p, m, v, x = ptrs(blk)
                assert lib.tgcn_adam_step(p, gk.data_ptr(), m, v, x, gk.numel(), lrs[k], BETA1, BETA2, EPS, wd, step,
                                          stream) == _lib.OK
        torch.cuda.synchronize()
        assert int(step_dev) == step
        want = [tc.adam_scalars(step, lr, BETA1, BETA2) for lr in lrs]
        got = scalars.cpu().numpy()
        assert [got[k] for k in range(K)] == [w[0] for w in want] and got[K] == want[0][1] and got[K + 1] == R.FILL
        for i, name in enumerate(("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")):
            if i == 3 and not ams:
                assert torch.equal(host[3], state[3]) and torch.equal(capt[3], state[3])              # untouched
                continue
            assert torch.equal(host[i].view(torch.int32), capt[i].view(torch.int32)), (name, step)
            if blocks is not None:
                for k, blk in enumerate(blocks):
                    assert torch.equal(host[i][:, k * width:(k + 1) * width].view(torch.int32), blk[i].view(torch.int32)), \
                        (name, step, k)
    assert not torch.equal(host[0], state[0]) or n_rows * n_cols == 0
    return host, state, grads


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("K", MEMBERS)
def test_adam_members_is_adam_step_on_every_column_block_bit_for_bit(cuda, width, K):
    lib = _lib.load()
    for i, n_rows in enumerate(ADAM_ROWS):
        for ams, wd in AMS_WD[(i + K + width) % 2::2] if n_rows == 1025 else AMS_WD:
            _run_adam_members(lib, cuda, n_rows, width, K, ams, wd, _rates(K))


@pytest.mark.parametrize("width,K,ams,wd", [(128, 64, True, 0.01), (3, 3, False, 0.0)], ids=["16-byte", "4-byte"])
def test_adam_members_past_the_workgroup_cap(cuda, width, K, ams, wd):
    """more elements than 8192 workgroups cover in one stride, on both leaves"""
    lib = _lib.load()
    n_rows = R.ADAM_CAP // (width * K) + 2
    assert n_rows * width * K > R.ADAM_CAP and R.adam_members_v4(width, width * K) == (width == 128)
    _run_adam_members(lib, cuda, n_rows, width, K, ams, wd, _rates(K))


@pytest.mark.parametrize("width,K", [(4, 12), (3, 12), (100, 3)])
def test_adam_members_with_equal_rates_is_one_adam_step_on_the_whole_tensor(cuda, width, K):
    lib = _lib.load()
    for ams, wd in AMS_WD:
        host, state, grads = _run_adam_members(lib, cuda, 7, width, K, ams, wd, [0.02] * K, check_blocks=False)
        whole = [t.clone() for t in state]
        for step, g in enumerate(grads, 1):
            assert lib.tgcn_adam_step(whole[0].data_ptr(), g.data_ptr(), whole[1].data_ptr(), whole[2].data_ptr(),
                                      whole[3].data_ptr() if ams else None, g.numel(), 0.02, BETA1, BETA2, EPS, wd, step,
                                      plan_mod._stream_ptr(cuda)) == _lib.OK
        torch.cuda.synchronize()
        for a, b in zip(host, whole):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_adam_members_of_size_zero(cuda):
    """a no-op; the capturable form still advances the device step and leaves its scalars"""
    lib = _lib.load()
    lrs = _rates(3)
    lr_host = (ctypes.c_double * 3)(*lrs)
    step_dev = torch.zeros((), dtype=I64, device=cuda)
    scalars = torch.full((5,), R.FILL, device=cuda)
    stream = plan_mod._stream_ptr(cuda)
    for n_rows, n_cols, width in ((0, 12, 4), (5, 0, 0)):
        assert lib.tgcn_adam_members(None, None, None, None, None, n_rows, n_cols, width, 3, lr_host, BETA1, BETA2, EPS, 0.0, 1,
                                     stream) == _lib.OK
        assert lib.tgcn_adam_members_capturable(None, None, None, None, None, n_rows, n_cols, width, 3, lr_host, BETA1, BETA2,
                                                EPS, 0.0, step_dev.data_ptr(), scalars.data_ptr(), stream) == _lib.OK
    torch.cuda.synchronize()
    assert int(step_dev) == 2
    want = [tc.adam_scalars(2, lr, BETA1, BETA2) for lr in lrs]
    got = scalars.cpu().numpy()
    assert [got[k] for k in range(3)] == [w[0] for w in want] and got[3] == want[0][1] and got[4] == R.FILL


# ----------------------------------------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------------------------------------
N_NODES, N_CLASSES, N_FOLDS = 400, 5, 3
RATES = (0.05, 0.01)
LRS = [lr for lr in RATES for _ in range(N_FOLDS)]                   # member l * 3 + f: rate l, fold f
ADAM_EPS = 0.1


def _build(cuda, h):
    """A 400-node synth graph, 3 folds x 2 rates = 6 members of hidden width h with random biases, the one network built
    from them, and per member the float64 oracle's logits, loss, gradients and parameters after one
    `torch.optim.Adam(lr=LRS[k], eps=ADAM_EPS)` step (computed once)."""
    from oracle import gcn_oracle as O
    N, C, K = N_NODES, N_CLASSES, len(LRS)
    g = synth.word_doc_graph(N, 3000, seed=7, n_classes=C)
    doc_rows = np.arange(g.n_vocab, N)
    order = np.random.default_rng(11).permutation(doc_rows.size)
    folds = [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)]
    train_bits, val_bits = fold_bits(doc_rows, folds, N, n_repeats=len(RATES))
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
        before = {n_: p.detach().clone() for n_, p in ref.named_parameters()}
        grads = {n_: p.grad.clone() for n_, p in ref.named_parameters()}
        torch.optim.Adam(ref.parameters(), lr=LRS[k], eps=ADAM_EPS).step()
        truth.append(dict(logits=z.detach(), loss=lk.item(), grads=grads, before=before,
                          after={n_: p.detach().clone() for n_, p in ref.named_parameters()}))
    net = CrossValGCN.from_members(members).to(cuda).float()
    gd = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(cuda)
    return dict(g=g, gd=gd, target=target.to(cuda), train_bits=train_bits.to(cuda), val_bits=val_bits.to(cuda),
                bits_host=(train_bits, val_bits), members=members, truth=truth, net=net, h=h, N=N, K=K, C=C)


@pytest.fixture(scope="module", params=[8, 40], ids=["h8-subgroup-leaf", "h40-gather-leaf"])
def small(request, cuda):
    """layer 1 is 6 x 8 = 48 columns wide (the sub-group SpMM leaf) or 6 x 40 = 240 (the gather leaf)"""
    return _build(cuda, request.param)


def _member_slices(net, k):
    h, S, C = net.n_hidden, net.seg_stride, net.out_channels
    first, second = net.layers
    return {"layers.0.weight": (first.weight, (slice(None), slice(k * h, (k + 1) * h))),
            "layers.0.bias": (first.bias, (slice(k * h, (k + 1) * h),)),
            "layers.1.weight": (second.weight, (slice(None), slice(k * S, k * S + C))),
            "layers.1.bias": (second.bias, (slice(k * S, k * S + C),))}


def test_eval_logits_of_every_member_against_the_oracle_and_the_exported_gcn(cuda, small):
    net, gd, C, S = small["net"].eval(), small["gd"], small["C"], small["net"].seg_stride
    assert net.layers[0].weight.size(1) == small["K"] * small["h"] and S == 8
    with torch.no_grad():
        z = net(gd)
        assert z.shape == (small["N"], small["K"] * S)
        exported = net.export_members()
        for k in range(small["K"]):
            assert R.rel_err(z[:, k * S:k * S + C], small["truth"][k]["logits"]) <= TOL
            mine = exported[k].eval()(gd)
            assert R.rel_err(z[:, k * S:k * S + C], mine.double()) <= TOL
        # evaluate: every member's validation loss on its fold, its arg-max on every row
        val_k, pred = net.evaluate(gd, small["target"], small["val_bits"])
        assert not net.training and pred.shape == (small["N"], small["K"])
        want = R.member_ce(z, small["target"], small["val_bits"], small["K"], C, S)
        assert R.rel_err(val_k, want[1]) <= TOL and torch.equal(pred.cpu(), want[4])
        net.train()
        net.evaluate(gd, small["target"], small["val_bits"])
        assert net.training                                            # the mode is put back
        net.eval()


def test_one_training_step_with_distinct_rates_against_k_oracle_models(cuda, small):
    net, gd, K = small["net"].train(), small["gd"], small["K"]
    start = {n_: p.detach().clone() for n_, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    loss, loss_k = net.loss(gd, small["target"], small["train_bits"])
    loss.backward()
    torch.cuda.synchronize()
    truth = small["truth"]
    total = sum(t["loss"] for t in truth)
    assert abs(loss.item() - total) <= TOL * total
    for k in range(K):
        want = truth[k]
        assert abs(float(loss_k[k]) - want["loss"]) <= TOL * want["loss"], (k, float(loss_k[k]), want["loss"])
        for name, (p, idx) in _member_slices(net, k).items():
            e = R.rel_err(p.grad[idx], want["grads"][name])
            print(f"h={small['h']} member {k} {name} gradient: {e:.2e}")
            assert e <= TOL, (k, name, e)
    pad = torch.ones(net.n_cols, dtype=torch.bool)
    for k in range(K):
        pad[k * net.seg_stride:k * net.seg_stride + net.out_channels] = False
    second = net.layers[1]
    assert bool((second.weight.grad.cpu()[:, pad] == 0.0).all()) and bool((second.bias.grad.cpu()[pad] == 0.0).all())
    # one step of MemberAdam: member k moves as its own oracle model does under torch.optim.Adam(lr=LRS[k]).  The first step
    # is lr * g / (|g| + eps): at torch's eps = 1e-8 that is lr * sign(g), which carries no gradient error, however small,
    # over to the parameters where g is near 0.  With eps = 0.1, of the size of the largest gradient entries, a relative
    # error of the gradient arrives as about (1 + max|g| / eps) times that in the update.  The default eps is covered bit
    # for bit by the kernel tests above.
    opt = MemberAdam(net, LRS, eps=ADAM_EPS)
    opt.step()
    torch.cuda.synchronize()
    try:
        for k in range(K):
            want = truth[k]
            for name, (p, idx) in _member_slices(net, k).items():
                got = p.detach()[idx].cpu().double()
                assert R.rel_err(got, want["after"][name]) <= TOL, (k, name)
                # the update itself: to 1e-5 of its size, plus the rounding of the stored fp32 parameter
                upd, wupd = got - want["before"][name], want["after"][name] - want["before"][name]
                bound = TOL * float(wupd.abs().max()) + 2.0 ** -23 * float(want["after"][name].abs().max())
                assert float((upd - wupd).abs().max()) <= bound, (k, name, float((upd - wupd).abs().max()), bound)
        assert bool((second.weight.detach().cpu()[:, pad] == 0.0).all()) and bool((second.bias.detach().cpu()[pad] == 0.0).all())
    finally:
        with torch.no_grad():                                                     # (the fixture is shared)
            for n_, p in net.named_parameters():
                p.copy_(start[n_])
        net.zero_grad(set_to_none=True)


def test_notes_are_left_and_consumed(cuda, small, monkeypatch):
    """the backward propagate step takes the loss's column sums and zero rows; without the notes it sums and gathers
    everything itself and arrives at the same gradients"""
    net, gd = small["net"].train(), small["gd"]

    def grads():
        net.zero_grad(set_to_none=True)
        loss, _ = net.loss(gd, small["target"], small["train_bits"])
        loss.backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in net.parameters()]

    left = {"colsum": 0, "rows": 0}
    real_colsum, real_rows = functional.note_colsum, functional.note_zero_rows
    monkeypatch.setattr(functional, "note_colsum", lambda t, s: (left.__setitem__("colsum", left["colsum"] + 1), real_colsum(t, s))[1])
    monkeypatch.setattr(functional, "note_zero_rows", lambda t, k: (left.__setitem__("rows", left["rows"] + 1), real_rows(t, k))[1])
    with_notes = grads()
    assert left == {"colsum": 1, "rows": 1}
    monkeypatch.setattr(functional, "note_colsum", lambda t, s: None)
    monkeypatch.setattr(functional, "note_zero_rows", lambda t, k: None)
    without = grads()
    for a, b in zip(with_notes, without):
        assert R.rel_err(a, b.double()) <= 1e-6
    net.zero_grad(set_to_none=True)


def test_fused_dropout_is_xw_dropout_per_member_bit_for_bit(cuda, small):
    net, h, N, K = small["net"], small["h"], small["N"], small["K"]
    starts, widths, p = net.seg_start, net.seg_width, 0.4
    gen = torch.Generator().manual_seed(17)
    H0 = torch.randn(N, K * h, generator=gen).to(cuda)
    W0 = net.layers[1].weight.detach().clone()
    G = torch.randn(N, net.n_cols, generator=gen).to(cuda)
    seeds = torch.tensor([0x1234567890ABCDE, -77, (1 << 40) + 12345, 5, -(1 << 62), 99][:K], dtype=I64, device=cuda)
    H, W = H0.clone().requires_grad_(), W0.clone().requires_grad_()
    out = block_diag_xw(H, W, starts, widths, p, seeds)
    out.backward(G)
    for k, (s, c) in enumerate(zip(starts, widths)):
        Hk = H0[:, k * h:(k + 1) * h].contiguous().requires_grad_()
        Wk = W0[:, s:s + c].contiguous().requires_grad_()
        ok = dense.xw_dropout(Hk, Wk, p, seeds[k:k + 1])
        ok.backward(torch.nn.functional.pad(G[:, s:s + c], (0, (-c) % 4))[:, :c])     # rows of 4 j floats, as a member GCN sees
        assert torch.equal(out[:, s:s + c], ok), k
        assert torch.equal(H.grad[:, k * h:(k + 1) * h], Hk.grad), k
        assert torch.equal(W.grad[:, s:s + c], Wk.grad), k
    from pytextgcn_amd import models
    was = models._FUSED_DROPOUT
    try:
        pkg.enable_fused_dropout()
        net.dropout = p
        z1, z2 = net.train()(small["gd"]), net(small["gd"])
        assert bool(torch.isfinite(z1).all()) and not torch.equal(z1, z2)         # a fresh seed per member and forward
    finally:
        pkg.enable_fused_dropout(was)
        net.dropout = 0.0
    assert models._FUSED_DROPOUT == was


def test_captured_step_replays_to_the_eager_parameters_bit_for_bit(cuda):
    """loss + backward + MemberAdam(capturable=True).step() captured once after two eager warm-up steps and replayed three
    times: the parameters of five eager steps, bit for bit (dropout 0)"""
    s = _build(cuda, 8)
    gd, target, bits = s["gd"], s["target"], s["train_bits"]
    counts = R.counts_of(s["bits_host"][0], s["K"])
    was = conv._REUSE
    conv.enable_activation_reuse(False)                                # a replay must not depend on Python-side caches
    try:
        nets = [CrossValGCN.from_members(s["members"]).to(cuda).float().train() for _ in range(2)]
        opts = [MemberAdam(n_, LRS, amsgrad=True, capturable=True) for n_ in nets]

        def eager(net, opt):
            loss, _ = net.loss(gd, target, bits, counts=counts)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        for _ in range(5):
            eager(nets[0], opts[0])
        net, opt = nets[1], opts[1]
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
        torch.cuda.synchronize()
        for (name, a), b in zip(nets[0].named_parameters(), net.parameters()):
            assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), name
        assert int(opt.state[net.layers[0].weight]["step"]) == 5
        assert bool(torch.isfinite(loss)) and loss_k.shape == (s["K"],)
    finally:
        conv.enable_activation_reuse(was)
