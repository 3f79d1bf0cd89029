"""The kernels of csrc/train.hip at every dispatch leaf, launch cap and value edge, through the C ABI with raw pointers
(strides, alignment and workspaces are the test's own) against float64 references computed on the host.  The cases, the
inputs and the references are tests/_train_cases.py's; tests/test_train_cases.py keeps that list complete on the CPU.

  masked cross-entropy   k_masked_ce<LPR, V4, KPL> + k_ce_final: the 6 class-count ranges x {16-byte, scalar} column map,
                         each with loss / loss + gradient / loss + gradient + bias gradient, with and without the arg-max,
                         inside padded buffers whose padding, spare rows and workspace are poisoned; the value edges; the
                         grid-stride loop (2048 * rows_per_block + 1 rows) of every leaf; n = 0; invalid targets.
  Adam                   k_adam<AMSGRAD, false>: sizes without a float4 body, around one workgroup, around the launch cap of
                         8192 workgroups; amsgrad x weight decay x beta1 on both sides of adam_element's lerp branch; the
                         first moment against at::lerp's formula bit for bit; k_adam_scalars against the host's two floats.
  k_scale_unless_one     the identity at exactly 1.0f, the 4096-block cap, n = 0.

The gradient is held to `row_rel_err`: every row to its OWN largest entry.  Observed on an MI355X, largest over all cases
of all leaves, against the bound 1e-5: loss 1.2e-7, gradient row 1.9e-6 (5.5e-7 without the rows scaled to +-80), bias
gradient 7.9e-7 (bound 2e-5); Adam 6.6e-7 on the parameter, 3.5e-7 on the state; the capturable scalars bit-equal to the
host's on all 50 steps.  Each run prints its own figures and hands them to test_gpu_parity's `_report` (keys train_ce_* /
train_adam_*).

What the file found when it was written: k_masked_ce computed the gradient at the target as `p_t - 1.f` and the loss as
`(m + log(sum)) - x_t`.  The first rounds to a multiple of 2^-24 where the whole row is of that size (row errors up to 100 %
of the row's scale on confident rows; 5e-4 .. 1e-3 on plain randn * 3 rows at 262 145 rows), the second rounds the loss to
the spacing of fp32 at |m| (7.8e-5 on all-equal rows at +-1e4), and the streaming path's `expf(x - lse)` did the same to
the gradient (4.5e-4 at +-1e4).  The kernel now keeps the target's term out of the sum and subtracts the row maximum first."""
import ctypes

import numpy as np
import pytest
import torch

import _train_cases as tc
from pytextgcn_amd import _lib
from test_gpu_parity import TOL, _report, row_rel_err

pytestmark = pytest.mark.gpu
F32, I64 = torch.float32, torch.int64


def _buffer(cuda, rows, ld, off, fill, dtype=F32):
    """a [rows, ld] view that starts `off` elements into a 16-byte aligned allocation filled with `fill`, four spare
    elements behind it; returns (whole allocation, view)"""
    base = torch.full((rows * ld + off + 4,), fill, dtype=dtype, device=cuda)
    assert base.data_ptr() % 16 == 0
    return base, base[off:off + rows * ld].view(rows, ld)


def _run_ce(lib, cuda, c, inp):
    """one call of the entry point `c.out` names, inside poisoned buffers; everything the call could have written, on the
    host"""
    n, C = c.n, c.C
    ld, ldd = C + c.pad, C + c.pad2
    lg_all, lg = _buffer(cuda, n + 1, ld, c.off, float("nan"))        # NaN padding, and a NaN row behind the last one
    lg[:n, :C] = torch.tensor(inp["x"]).to(cuda)
    dl_all, dl = _buffer(cuda, n + 3, ldd, c.offd, tc.FILL)
    db = torch.full((C + 4,), tc.FILL, dtype=F32, device=cuda)
    pr = torch.full((n + 3,), 7, dtype=I64, device=cuda)
    loss = torch.full((2,), tc.FILL, dtype=F32, device=cuda)
    target = torch.zeros(max(n, 1), dtype=I64, device=cuda)               # (n = 0 still hands over real pointers)
    mask = torch.zeros(max(n, 1), dtype=torch.uint8, device=cuda)
    target[:n] = torch.tensor(inp["target"]).to(cuda)
    mask[:n] = torch.from_numpy(inp["mask"].astype(np.uint8)).to(cuda)
    ws_bytes = lib.tgcn_masked_ce_grad_workspace_bytes(n, C) if c.out == "dbias" else lib.tgcn_masked_ce_workspace_bytes()
    ws = torch.full((ws_bytes // 4 + 4,), float("nan"), dtype=F32, device=cuda)
    assert ws_bytes % 4 == 0 and (lg.data_ptr() % 16 == 0) == (c.off % 4 == 0) and (dl.data_ptr() % 16 == 0) == (c.offd % 4 == 0)
    inv = ctypes.c_float(inp["inv_count"])
    pred_ptr = pr.data_ptr() if c.pred else None
    if c.out == "dbias":
        rc = lib.tgcn_masked_ce_grad(lg.data_ptr(), ld, n, C, target.data_ptr(), mask.data_ptr(), inv, loss.data_ptr(),
                                     dl.data_ptr(), ldd, db.data_ptr(), pred_ptr, ws.data_ptr(), ws_bytes, None)
    else:
        rc = lib.tgcn_masked_ce_pred(lg.data_ptr(), ld, n, C, target.data_ptr(), mask.data_ptr(), inv, loss.data_ptr(),
                                     dl.data_ptr() if c.out == "grad" else None, ldd, pred_ptr, ws.data_ptr(), ws_bytes, None)
    assert rc == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    return {"loss": loss.cpu(), "dl_all": dl_all.cpu(), "dl": dl.cpu(), "db": db.cpu(), "pred": pr.cpu(),
            "ws_tail": ws[ws_bytes // 4:].cpu(), "lg_all": lg_all.cpu()}


def _row_err(got, ref):
    """row_rel_err over the rows whose own scale fp32 can hold (or that are exactly zero); the few rows below
    tc.TINY_ROW -- see there -- against that scale"""
    rowmax = ref.abs().max(1).values
    held = (rowmax >= tc.TINY_ROW) | (rowmax == 0)
    err = row_rel_err(got[held], ref[held]) if bool(held.any()) else 0.0
    if bool((~held).any()):
        err = max(err, float((got[~held].double() - ref[~held]).abs().max()) / tc.TINY_ROW)
    return err


def _check_ce(c, got, inp, ref, worst, loss_is_nan=False):
    n, C = c.n, c.C
    mask = torch.tensor(inp["mask"])
    assert float(got["loss"][1]) == tc.FILL and bool(torch.isnan(got["ws_tail"]).all())
    if loss_is_nan:
        assert bool(torch.isnan(got["loss"][0])) and np.isnan(ref["loss"]), tc.ce_case_id(c)
    else:
        e_loss = abs(float(got["loss"][0]) - ref["loss"]) / abs(ref["loss"]) if ref["loss"] != 0 else abs(float(got["loss"][0]))
        worst["loss"] = max(worst.get("loss", 0.0), e_loss)
        assert e_loss < TOL, (tc.ce_case_id(c), float(got["loss"][0]), ref["loss"])
    dl = got["dl"]
    if c.out == "loss":
        assert bool((got["dl_all"] == tc.FILL).all()), tc.ce_case_id(c)
    else:
        want = torch.tensor(ref["grad"])
        e_row = _row_err(dl[:n, :C][mask], want[mask])
        worst["row"] = max(worst.get("row", 0.0), e_row)
        assert e_row < TOL, (tc.ce_case_id(c), e_row)
        assert bool((dl[:n, :C][~mask] == 0).all()), tc.ce_case_id(c)               # masked-out rows: exactly zero
        assert bool((dl[:n, C:] == tc.FILL).all()) and bool((dl[n:] == tc.FILL).all()), tc.ce_case_id(c)
        # ... and everything of the allocation outside the view
        assert bool((got["dl_all"][:c.offd] == tc.FILL).all()) and bool((got["dl_all"][c.offd + (n + 3) * (C + c.pad2):] == tc.FILL).all())
    if c.out == "dbias":
        wdb = torch.tensor(ref["dbias"])
        e_db = float((got["db"][:C].double() - wdb).abs().max()) / max(float(wdb.abs().max()), 1e-30)
        worst["dbias"] = max(worst.get("dbias", 0.0), e_db)
        assert e_db < 2e-5, (tc.ce_case_id(c), e_db)
        assert bool((got["db"][C:] == tc.FILL).all())
    else:
        assert bool((got["db"] == tc.FILL).all())
    if c.pred:
        assert torch.equal(got["pred"][:n], torch.tensor(ref["pred"])), tc.ce_case_id(c)     # every row, masked or not
        assert bool((got["pred"][n:] == 7).all())
    else:
        assert bool((got["pred"] == 7).all())


def _sweep(cuda, cases, key):
    lib = _lib.load()
    worst = {}
    for c in cases:
        inp, ref = tc.ce_inputs(c.C, c.n, c.values), tc.ce_reference(c.C, c.n, c.values)
        _check_ce(c, _run_ce(lib, cuda, c, inp), inp, ref, worst)
    print(f"\n{key}: {len(cases)} cases, worst {worst}")
    _report(key, cases=len(cases), **worst)


_SMALL, _EDGE, _STRIDE = tc.by_leaf(tc.small_cases()), tc.by_leaf(tc.edge_cases()), tc.by_leaf(tc.stride_cases())


@pytest.mark.parametrize("leaf", tc.LEAVES, ids=tc.leaf_id)
def test_masked_ce_leaf_layouts_and_outputs(cuda, leaf):
    """every width, layout and output combination of one leaf at 257 rows (and 1 / 37 rows where the leaf has them)"""
    _sweep(cuda, _SMALL[leaf], "train_ce_small_" + tc.leaf_id(leaf))


@pytest.mark.parametrize("leaf", tc.LEAVES, ids=tc.leaf_id)
def test_masked_ce_value_edges(cuda, leaf):
    """rows at +-80 and +-1e4, rows scaled to +-80 and +-1e4, -inf in a third of the other columns, all-equal rows, one
    masked row, ties across the hand-over points of both column maps"""
    _sweep(cuda, _EDGE[leaf], "train_ce_edges_" + tc.leaf_id(leaf))


@pytest.mark.parametrize("leaf", tc.LEAVES, ids=tc.leaf_id)
def test_masked_ce_grid_stride_loop(cuda, leaf):
    """2048 * rows_per_block + 1 rows: a workgroup takes a second stride; random rows, and one-hot rows that name
    themselves so that a wrong row assignment is a wrong row"""
    _sweep(cuda, _STRIDE[leaf], "train_ce_stride_" + tc.leaf_id(leaf))


@pytest.mark.parametrize("C", [16, 300, 33])
def test_masked_ce_of_no_rows(cuda, C):
    """n_rows = 0: TGCN_OK, a loss of exactly 0 and a bias gradient of zeros; nothing else is written"""
    lib = _lib.load()
    empty = {"x": np.zeros((0, C), np.float32), "target": np.zeros(0, np.int64), "mask": np.zeros(0, bool), "inv_count": 1.0}
    for out in tc.OUTPUTS:
        got = _run_ce(lib, cuda, tc.CeCase(C, 0, 4, 4, 0, 0, out, True, "randn"), empty)
        assert float(got["loss"][0]) == 0.0 and float(got["loss"][1]) == tc.FILL
        assert bool((got["dl_all"] == tc.FILL).all()) and bool((got["pred"] == 7).all())
        if out == "dbias":
            assert bool((got["db"][:C] == 0).all()) and bool((got["db"][C:] == tc.FILL).all())
        else:
            assert bool((got["db"] == tc.FILL).all())


@pytest.mark.parametrize("C,lay", [(16, (4, 4, 0, 0)), (33, (1, 3, 0, 0)), (64, (0, 0, 1, 1)), (260, (0, 4, 0, 0)), (257, (1, 1, 0, 0))],
                         ids=["regs-v4", "regs-scalar", "regs-shifted", "stream-v4", "stream-scalar"])
@pytest.mark.parametrize("bad", [-1, "C"])
def test_masked_ce_invalid_target_poisons_the_loss_and_reads_nothing_outside_the_row(cuda, C, lay, bad):
    """a target of -1 or C on a masked-in row: the loss is NaN, every gradient row is still right (the bad row's is its
    softmax: no class to subtract), and nothing outside the row is touched.  The row behind the logits is the test's own
    and holds NaN: a read of it would show in the gradient."""
    lib = _lib.load()
    base = tc.ce_inputs(C, tc.N_SMALL, "randn")
    target = base["target"].copy()
    rows = np.flatnonzero(base["mask"])
    target[[rows[0], rows[-1], rows[len(rows) // 2]]] = C if bad == "C" else -1
    inp = dict(base, target=target)
    ref = tc.ce_reference_of(inp["x"], target, inp["mask"], inp["inv_count"])
    assert np.isnan(ref["loss"]) and np.isfinite(ref["grad"]).all()
    worst = {}
    for out in ("grad", "dbias"):
        c = tc.CeCase(C, tc.N_SMALL, *lay, out, True, "randn")
        got = _run_ce(lib, cuda, c, inp)
        _check_ce(c, got, inp, ref, worst, loss_is_nan=True)
        assert bool(torch.isnan(got["lg_all"][c.off + c.n * (C + c.pad):]).all())


# ---- Adam ------------------------------------------------------------------------------------------------------------
def _adam_device(cuda, arrays):
    """each array followed by four elements of 7.0 that no call may touch"""
    out = []
    for a in arrays:
        t = torch.full((a.size + 4,), tc.FILL, dtype=F32, device=cuda)
        t[:a.size] = torch.from_numpy(a).to(cuda)
        assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


def adam_rel_err(name, got, ref):
    """the measure every Adam result is held to (bound: TOL), against a float64 reference: the parameter ("p") relative to
    max(|p|, 1e-3), element by element; the state relative to max(|.|, 1) -- operands of size O(1) (|g| <= 15), where fp32's
    6e-8 per operation leaves a factor of ten"""
    floor = 1e-3 if name == "p" else 1.0
    return float(((got.double() - ref).abs() / ref.abs().clamp_min(floor)).max())


def _run_adam(lib, cuda, c, check_lerp=False):
    p, m, v, vmax, grads = tc.adam_inputs(c)
    want = tc.adam_reference(c, p, m, v, vmax, grads)
    dp, dm, dv, dx = _adam_device(cuda, (p, m, v, vmax))
    for step, g in enumerate(grads, 1):
        (dg,) = _adam_device(cuda, (g,))
        rc = lib.tgcn_adam_step(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), dx.data_ptr() if c.amsgrad else None,
                                c.n, tc.ADAM_LR, c.beta1, tc.ADAM_BETA2, tc.ADAM_EPS, c.wd, step, None)
        assert rc == _lib.OK, lib.tgcn_last_error()
        if check_lerp and step == 1:
            # the first moment, bit for bit: at::lerp's formula in fp32 without contraction, as adam_element states it --
            # `weight < 0.5 ? m + weight * (g - m) : g - (g - m) * (1 - weight)`, weight = float(1 - beta1)
            w1 = np.float32(1.0 - c.beta1)
            gr = g + np.float32(c.wd) * p if c.wd else g
            diff = gr - m
            lerp = m + w1 * diff if w1 < np.float32(0.5) else gr - diff * (np.float32(1.0) - w1)
            assert lerp.dtype == np.float32
            assert torch.equal(dm[:c.n].cpu().view(torch.int32), torch.from_numpy(lerp).view(torch.int32)), tc.adam_case_id(c)
    torch.cuda.synchronize()
    errs = {}
    for name, dev, ref, first in (("p", dp, want[0], p), ("m", dm, want[1], m), ("v", dv, want[2], v), ("vmax", dx, want[3], vmax)):
        got = dev.cpu()
        assert bool((got[c.n:] == tc.FILL).all()), (tc.adam_case_id(c), name)
        if name == "vmax" and not c.amsgrad:
            assert torch.equal(got[:c.n], torch.from_numpy(first))                  # not an operand without amsgrad
            continue
        e = adam_rel_err(name, got[:c.n], torch.from_numpy(ref))
        errs[name] = e
        assert e < TOL, (tc.adam_case_id(c), name, e)
    return errs


def test_adam_small_sizes_whole_grid(cuda):
    """n in 1, 2, 3, 5, 6, 7 (no float4 body, or a body and a tail), 1023, 1024, 1025 (one workgroup and one element more) x
    amsgrad x weight decay x beta1 in 0.9, 0.5, 0.3: three steps against float64, and the first moment of the first step
    against at::lerp's fp32 formula bit for bit -- beta1 = 0.5 sits on the branch (w1 = 0.5f is not < 0.5f)"""
    lib = _lib.load()
    worst = {}
    for c in tc.adam_small_cases():
        for k, e in _run_adam(lib, cuda, c, check_lerp=True).items():
            worst[k] = max(worst.get(k, 0.0), e)
    print(f"\ntrain_adam_small: {len(tc.adam_small_cases())} cases, worst {worst}")
    _report("train_adam_small", **worst)


@pytest.mark.parametrize("case", tc.adam_big_cases(), ids=tc.adam_case_id)
def test_adam_around_the_launch_cap_of_the_plain_leaf(cuda, case):
    """8192 workgroups x 1024 elements: at 8 388 604 no thread loops, at 8 388 612 one float4 is a second stride, at
    8 388 608 + 3 * 1024 + 1 three workgroups and a scalar tail are"""
    errs = _run_adam(_lib.load(), cuda, case, check_lerp=True)
    print(f"\ntrain_adam_{tc.adam_case_id(case)}: {errs}")
    _report("train_adam_" + tc.adam_case_id(case), **errs)


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("beta1,beta2", [(0.9, 0.999), (0.3, 0.5)])
def test_adam_capturable_scalars_are_the_host_paths(cuda, beta1, beta2):
    """k_adam_scalars derives lr / bc1 and 1 / sqrt(bc2) in double on the device: after each of 50 steps the step count is
    the host's and the two floats are the ones adam_impl computes on the host, and the parameters of the capturable form
    are bit for bit those of the host-step form."""
    lib = _lib.load()
    c = tc.AdamCase(1025, True, 0.01, beta1)
    p, m, v, vmax, _ = tc.adam_inputs(c)
    host, cap = _adam_device(cuda, (p, m, v, vmax)), _adam_device(cuda, (p, m, v, vmax))
    step_dev = torch.zeros(2, dtype=I64, device=cuda)
    step_dev[1] = 7
    scal = torch.full((4,), tc.FILL, dtype=F32, device=cuda)
    gen = np.random.default_rng(50)
    worst = 0
    for step in range(1, 51):
        (dg,) = _adam_device(cuda, (gen.standard_normal(c.n, dtype=np.float32),))
        hyper = (c.n, tc.ADAM_LR, beta1, beta2, tc.ADAM_EPS, c.wd)
        assert lib.tgcn_adam_step(*(t.data_ptr() for t in (host[0], dg, host[1], host[2], host[3])), *hyper, step, None) == _lib.OK
        assert lib.tgcn_adam_step_capturable(*(t.data_ptr() for t in (cap[0], dg, cap[1], cap[2], cap[3])), *hyper,
                                             step_dev.data_ptr(), scal.data_ptr(), None) == _lib.OK
        assert step_dev.tolist() == [step, 7]
        got = scal.cpu().numpy()
        want = tc.adam_scalars(step, tc.ADAM_LR, beta1, beta2)
        assert got[2] == tc.FILL and got[3] == tc.FILL
        u = max(_ulps(got[0], want[0]), _ulps(got[1], want[1]))
        worst = max(worst, u)
        # (one ulp would be what double pow on the device may differ by; they were bit-equal on the MI355X at both pairs of
        # betas on all 50 steps, so equality is what is asserted)
        assert u == 0, (step, got[:2], want)
        for a, b in zip(host, cap):                        # the same scalars: the same parameters and state, bit for bit
            assert torch.equal(a, b), step
    print(f"\ntrain_adam_capturable b1={beta1} b2={beta2}: largest distance {worst} ulp")
    _report(f"train_adam_capturable_b{beta1:g}_{beta2:g}", worst_ulp=worst)


# ---- k_scale_unless_one ----------------------------------------------------------------------------------------------
def test_scale_by_one_is_the_identity_on_every_bit_pattern(cuda):
    """a device scalar of exactly 1.0f: NaN payloads, -0.0, infinities and subnormals come back bit for bit"""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(1)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (tc.SCALE_CAP + 257,), generator=gen, dtype=torch.int64).to(torch.int32)
    bits[:6] = torch.tensor([0x7FC00001, -0x80000000, 0x7F800000, -0x00800000, 0x00000001, 0x7FA00000], dtype=torch.int64).to(torch.int32)
    x = bits.to(cuda)
    assert bool(torch.isnan(x.view(F32)).any())
    one = torch.ones(1, device=cuda)
    assert lib.tgcn_scale_by_device_scalar(x.data_ptr(), x.numel(), one.data_ptr(), None) == _lib.OK
    assert torch.equal(x.cpu(), bits)


@pytest.mark.parametrize("scale", tc.SCALES)
def test_scale_by_a_device_scalar_is_the_fp32_product_at_every_size(cuda, scale):
    """1, 255, 256, 257 elements, 1 048 576 (the 4096-block cap) and 1 048 577 + 256 (a second stride and a ragged end):
    x * s exactly as fp32 multiplies, the sign of zero included; nothing behind the n-th element is touched"""
    lib = _lib.load()
    s_dev = torch.full((1,), scale, device=cuda)
    for n in tc.SCALE_N:
        x = torch.randn(n + 4, generator=torch.Generator().manual_seed(n))
        x[::5] = -0.0
        x[n:] = tc.FILL
        d = x.to(cuda)
        assert lib.tgcn_scale_by_device_scalar(d.data_ptr(), n, s_dev.data_ptr(), None) == _lib.OK
        want = x.clone()
        want[:n] *= torch.tensor(scale, dtype=F32)
        assert torch.equal(d.cpu().view(torch.int32), want.view(torch.int32)), (scale, n)


def test_scale_of_no_elements(cuda):
    lib = _lib.load()
    one = torch.full((1,), 2.5, device=cuda)
    assert lib.tgcn_scale_by_device_scalar(None, 0, one.data_ptr(), None) == _lib.OK
    assert lib.tgcn_scale_by_device_scalar(None, 1, one.data_ptr(), None) == _lib.E_INVALID
