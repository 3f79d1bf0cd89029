"""`tgcn_grouped_ce` (csrc/perlabel.hip) at every dispatch leaf, segment layout, output combination, launch cap, group edge
and value edge, through the C ABI with raw pointers (strides, alignment and workspace are the test's own) against the
float64 reference of tests/_grouped_ce_cases.py; tests/test_grouped_ce_cases.py keeps that list complete on the CPU and shows
that an fp32 evaluation of the intended arithmetic meets every bar used here.

  k_grouped_ce<LPR, V4>   5 lane counts x {16-byte, scalar} column map, the scalar one forced by each of its five causes alone
  k_grouped_ce_wide       n_cols > 256, aligned or not
  each with               four segment layouts x loss / + gradient / + bias gradient x arg-max off / in the group / routed /
                          mapped; K = 128 and K = 16 width-1 segments; the value edges; 1024 * rows_per_block (+ 1) rows

Every logits column outside a row's own training and routing segment holds NaN (pad columns, the row behind the last one
and the workspace too), every output sits in a padded, shifted buffer filled with 7: the call with the poison gives bit for
bit what the call without it gives, writes exactly 0 outside the segments and nothing outside its views.

The gradient is held row by row: every selected row to its OWN largest entry (`TINY_ROW` for rows below fp32's reach),
bound `TOL` = 1e-5; `loss` and every finite `loss_k` relative to float64 at `TOL`; the bias gradient at 2e-5; `pred` for
equality.  Each run prints its worst figures and hands them to test_gpu_parity's `_report` (keys grouped_ce_*).

Observed on an MI355X, largest over all cases of all leaves: loss 6.8e-7, loss_k 3.0e-6 (segments scaled to +-80), gradient
row 3.8e-6 (the same; 6.3e-7 on the grid-stride cases), bias gradient 4.2e-7 (bound 2e-5).

What the file found when it was written: the kernels formed the gradient at the target as `e_t / sum - 1.f`, the loss term
as `(m + log(sum)) - x_t` and the wide gradient as `expf(x - lse)`, the three roundings the flat kernel had shed.  Against
that kernel 45 of the 49 items failed, in 433 of the 1 215 cases of the three sweeps -- every leaf, every family but the one selected row:
  gradient row   1.0 (the whole row) on one-hot rows, on confident rows of 3 N(0, 1) logits and of segments scaled to +-80 /
                 +-1e4, on rows at -1e4; 0.46 at +1e4; 2.4e-2 / 3.8e-2 at +-80; 2.2e-2 with target = arg-max; 2.9e-3 with -inf
                 columns; 5.0e-4 next to all-NaN rows; 2.1e-4 on all-equal rows; 9.1e-5 on ties; on plain 3 N(0, 1) rows at
                 257 rows between 2.1e-5 (16 columns) and 3.7e-3 (257 columns)
  loss_k         6.0e-4 at +1e4, 3.6e-4 at -1e4, 3.1e-4 on all-equal rows, 2.8e-4 on segments scaled to +-80
  loss           5.7e-5 on all-equal rows, 1.7e-5 at +-1e4
  bias gradient  4.5e-4 at -1e4, 1.9e-4 at +1e4, 2.1e-4 on all-equal rows
while the max-norm error of the same gradients stayed below 1e-6.  The kernels now keep the target's term out of the sum and
subtract the segment's maximum first, as `ce_rows` (csrc/masked_ce.h) does."""
import ctypes

import numpy as np
import pytest
import torch

import _grouped_ce_cases as gc
from pytextgcn_amd import _lib
from test_gpu_parity import TOL, _report

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64
DBIAS_TOL = 2e-5                                 # the flat sweep's bound (tests/test_gpu_train_kernels.py)


def _buffer(cuda, rows, ld, off, fill, dtype=F32):
    """a [rows, ld] view that starts `off` elements into a 16-byte aligned allocation filled with `fill`, four spare
    elements behind it; returns (whole allocation, view)"""
    base = torch.full((rows * ld + off + 4,), fill, dtype=dtype, device=cuda)
    assert base.data_ptr() % 16 == 0
    return base, base[off:off + rows * ld].view(rows, ld)


def _dev(cuda, a, dtype, least=1):
    """a device copy with at least one element (n = 0 still hands over real pointers)"""
    t = torch.zeros(max(len(a), least), dtype=dtype, device=cuda)
    t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t


def _run(lib, cuda, c, inp, x, ws_short=0):
    """one call inside poisoned buffers; (status, everything the call could have written, on the host)"""
    n, C = c.n, c.C
    K = len(inp["starts"])
    ld, ldd = C + c.pad, C + c.pad2
    lg_all, lg = _buffer(cuda, n + 1, ld, c.off, float("nan"))        # NaN padding, and a NaN row behind the last one
    lg[:n, :C] = torch.from_numpy(x).to(cuda)
    dl_all, dl = _buffer(cuda, n + 3, ldd, c.offd, gc.FILL)
    db = torch.full((C + 4,), gc.FILL, dtype=F32, device=cuda)
    pr = torch.full((n + 3,), 7, dtype=I64, device=cuda)
    loss = torch.full((2,), gc.FILL, dtype=F32, device=cuda)
    loss_k = torch.full((K + 2,), gc.FILL, dtype=F32, device=cuda)
    host_start = (ctypes.c_int32 * K)(*[int(v) for v in inp["starts"]])
    host_width = (ctypes.c_int32 * K)(*[int(v) for v in inp["widths"]])
    d_start, d_width = _dev(cuda, inp["starts"].astype(np.int32), I32), _dev(cuda, inp["widths"].astype(np.int32), I32)
    group, route = _dev(cuda, inp["group"], I32), _dev(cuda, inp["route"], I32)
    target, mask = _dev(cuda, inp["target"], I64), _dev(cuda, inp["mask"].astype(np.uint8), torch.uint8)
    inv, cmap = _dev(cuda, inp["inv_count"], F32), _dev(cuda, inp["class_map"], I64)
    ws_bytes = lib.tgcn_grouped_ce_workspace_bytes(n, C, K)
    ws = torch.full((ws_bytes // 4 + 4,), float("nan"), dtype=F32, device=cuda)
    assert ws_bytes % 4 == 0 and (lg.data_ptr() % 16 == 0) == (c.off % 4 == 0) and (dl.data_ptr() % 16 == 0) == (c.offd % 4 == 0)
    rc = lib.tgcn_grouped_ce(lg.data_ptr(), ld, n, C, K, host_start, host_width, d_start.data_ptr(),
                             d_width.data_ptr(), group.data_ptr(), route.data_ptr() if c.route else None, target.data_ptr(),
                             mask.data_ptr(), inv.data_ptr(), cmap.data_ptr() if c.cmap else None, loss.data_ptr(),
                             loss_k.data_ptr(), dl.data_ptr() if c.out != "loss" else None, ldd,
                             db.data_ptr() if c.out == "dbias" else None, pr.data_ptr() if c.pred else None, ws.data_ptr(),
                             ws_bytes - ws_short, None)
    torch.cuda.synchronize()
    return rc, {"loss": loss.cpu(), "loss_k": loss_k.cpu(), "dl_all": dl_all.cpu(), "dl": dl.cpu(), "db": db.cpu(),
                "pred": pr.cpu(), "ws_tail": ws[ws_bytes // 4:].cpu(), "lg_all": lg_all.cpu()}


def _same_bits(a, b):
    return all(torch.equal(a[k].view(I32) if a[k].dtype == F32 else a[k], b[k].view(I32) if b[k].dtype == F32 else b[k])
               for k in ("loss", "loss_k", "dl_all", "db", "pred", "ws_tail"))


def _check(c, got, inp, ref, worst, nan_groups=()):
    """`nan_groups`: the groups whose loss_k (and with them `loss`) a selected row with an invalid target turns into NaN"""
    n, C, K = c.n, c.C, len(inp["starts"])
    cid = gc.case_id(c)
    assert float(got["loss"][1]) == gc.FILL and bool((got["loss_k"][K:] == gc.FILL).all()) and bool(torch.isnan(got["ws_tail"]).all()), cid
    mine = {"loss": float(got["loss"][0]), "loss_k": got["loss_k"][:K].numpy().astype(np.float64)}
    if c.out != "loss":
        mine["grad"] = got["dl"][:n, :C].numpy()
    if c.out == "dbias":
        mine["dbias"] = got["db"][:C].numpy().astype(np.float64)
    want = dict(ref)
    if len(nan_groups):
        assert np.isnan(mine["loss"]) and np.isnan(mine["loss_k"][list(nan_groups)]).all(), cid
        keep = np.ones(K, dtype=bool)
        keep[list(nan_groups)] = False
        want["loss_k"] = np.where(keep, ref["loss_k"], np.nan)
        mine["loss"] = want["loss"] = 0.0
    errs = gc.errors(mine, want, inp)
    for k, v in errs.items():
        worst[k] = max(worst.get(k, 0.0), v)
    bounds = {"loss": TOL, "loss_k": TOL, "row": TOL, "dbias": DBIAS_TOL}
    over = {k: v for k, v in errs.items() if not v < bounds[k]}                 # (asserted by the caller, after the rest)
    if c.out == "loss":
        assert bool((got["dl_all"] == gc.FILL).all()), cid
    else:
        # exactly zero on the rows that are not selected and outside the training segment of those that are
        dl = got["dl"]
        sel = gc.selected_rows(inp)
        inside = gc.own_columns(inp, False, False) & sel[:, None]
        assert bool((dl[:n, :C][torch.from_numpy(~inside)] == 0).all()), cid
        assert bool((dl[:n, C:] == gc.FILL).all()) and bool((dl[n:] == gc.FILL).all()), cid
        assert bool((got["dl_all"][:c.offd] == gc.FILL).all()) and bool((got["dl_all"][c.offd + (n + 3) * (C + c.pad2):] == gc.FILL).all())
    if c.out == "dbias":
        assert bool((got["db"][:C][torch.from_numpy(~gc.trained_columns(inp))] == 0).all()), cid      # pad columns, idle groups
        assert bool((got["db"][C:] == gc.FILL).all()), cid
    else:
        assert bool((got["db"] == gc.FILL).all()), cid
    if c.pred:
        assert torch.equal(got["pred"][:n], torch.from_numpy(ref["pred"][c.route, c.cmap])), cid    # every row, selected or not
        assert bool((got["pred"][n:] == 7).all()), cid
    else:
        assert bool((got["pred"] == 7).all()), cid
    return over


def _sweep(cuda, cases, key):
    lib = _lib.load()
    worst, missed = {}, []
    for c in cases:
        inp, ref = gc.gce_inputs(c.C, c.n, c.seg, c.values), gc.gce_reference(c.C, c.n, c.seg, c.values)
        rc, got = _run(lib, cuda, c, inp, gc.poisoned(inp, c.pred, c.route))
        assert rc == _lib.OK, lib.tgcn_last_error()
        over = _check(c, got, inp, ref, worst)
        if over:
            missed.append((gc.case_id(c), over))
        if c.n <= gc.N_GROUP_EDGE:
            # no output changes with what the columns outside the row's own segments hold
            rc, plain = _run(lib, cuda, c, inp, inp["x"])
            assert rc == _lib.OK and _same_bits(got, plain), gc.case_id(c)
    print(f"\n{key}: {len(cases)} cases, worst {worst}")
    for m in missed:
        print("  over the bound:", *m)
    _report(key, cases=len(cases), **worst)
    assert not missed, (len(missed), missed[:4])               # every case was run and printed before this


_SMALL, _EDGE, _STRIDE = gc.by_leaf(gc.small_cases()), gc.by_leaf(gc.edge_cases()), gc.by_leaf(gc.stride_cases())


@pytest.mark.parametrize("leaf", gc.LEAVES, ids=gc.leaf_id)
def test_grouped_ce_leaf_layouts_and_outputs(cuda, leaf):
    """every width, buffer layout, segment layout and output combination of one leaf at 257 rows (1 / 37 rows and the K = 16
    / K = 128 segment lists where the leaf has them)"""
    _sweep(cuda, _SMALL[leaf], "grouped_ce_small_" + gc.leaf_id(leaf))


@pytest.mark.parametrize("leaf", gc.LEAVES, ids=gc.leaf_id)
def test_grouped_ce_value_edges(cuda, leaf):
    """rows at +-80 and +-1e4, segments scaled to +-80 and +-1e4, -inf in a third of the other columns, all-equal rows, one
    selected row, ties across the hand-over columns of both column maps and at a segment's ends, one-hot rows, rows whose
    target is their arg-max, all-NaN rows"""
    _sweep(cuda, _EDGE[leaf], "grouped_ce_edges_" + gc.leaf_id(leaf))


@pytest.mark.parametrize("leaf", gc.LEAVES, ids=gc.leaf_id)
def test_grouped_ce_grid_stride_loop(cuda, leaf):
    """1024 * rows_per_block + 1 rows: a workgroup takes a second stride; random rows, and one-hot rows that name
    themselves so that a wrong row assignment is a wrong row; and exactly 1024 * rows_per_block rows"""
    _sweep(cuda, _STRIDE[leaf], "grouped_ce_stride_" + gc.leaf_id(leaf))


@pytest.mark.parametrize("C", [16, 300, 33])
def test_grouped_ce_of_no_rows(cuda, C):
    """n_rows = 0: TGCN_OK, a loss of exactly 0, NaN for every group (a mean over nothing), a bias gradient of zeros;
    nothing else is written"""
    lib = _lib.load()
    for out in gc.OUTPUTS:
        c = gc.GceCase(C, 0, "packed", 4, 4, 0, 0, out, True, True, True, "randn")
        inp = gc.gce_inputs(c.C, 0, c.seg, c.values)
        K = len(inp["starts"])
        rc, got = _run(lib, cuda, c, inp, inp["x"])
        assert rc == _lib.OK, lib.tgcn_last_error()
        assert float(got["loss"][0]) == 0.0 and float(got["loss"][1]) == gc.FILL
        assert bool(torch.isnan(got["loss_k"][:K]).all()) and bool((got["loss_k"][K:] == gc.FILL).all())
        assert bool((got["dl_all"] == gc.FILL).all()) and bool((got["pred"] == 7).all()) and bool(torch.isnan(got["ws_tail"]).all())
        if out == "dbias":
            assert bool((got["db"][:C] == 0).all()) and bool((got["db"][C:] == gc.FILL).all())
        else:
            assert bool((got["db"] == gc.FILL).all())


def test_grouped_ce_refuses_more_than_128_groups_and_a_short_workspace(cuda):
    """K = 129 is E_INVALID (kGceMaxGroups = 128 is what the LDS slots hold), K = 128 is served; a workspace one byte short
    of the advertised size is E_WORKSPACE; neither call writes anything"""
    lib = _lib.load()
    c = gc.GceCase(300, 37, "ones_spread", 0, 0, 0, 0, "dbias", True, True, True, "randn")
    inp = dict(gc.gce_inputs(c.C, c.n, c.seg, c.values))
    assert len(inp["starts"]) == gc.GCE_MAX_GROUPS
    rc, _ = _run(lib, cuda, c, inp, inp["x"])
    assert rc == _lib.OK
    rc, got = _run(lib, cuda, c, inp, inp["x"], ws_short=1)
    assert rc == _lib.E_WORKSPACE
    more = dict(inp, starts=np.append(inp["starts"], 257), widths=np.append(inp["widths"], 1), inv_count=np.append(inp["inv_count"], np.float32(0)))
    rc, got2 = _run(lib, cuda, c, more, inp["x"])
    assert rc == _lib.E_INVALID and "129" in lib.tgcn_last_error().decode()
    for g in (got, got2):
        assert bool((g["loss"] == gc.FILL).all()) and bool((g["loss_k"] == gc.FILL).all()) and bool((g["dl_all"] == gc.FILL).all())
        assert bool((g["db"] == gc.FILL).all()) and bool((g["pred"] == 7).all()) and bool(torch.isnan(g["ws_tail"]).all())


@pytest.mark.parametrize("C,lay", [(16, (4, 4, 0, 0)), (33, (1, 3, 0, 0)), (64, (0, 0, 1, 1)), (128, (4, 4, 0, 0)), (260, (0, 4, 0, 0)),
                                   (257, (1, 1, 0, 0))], ids=["lpr4-v4", "lpr16-scalar", "lpr16-shifted", "lpr32-v4", "wide-aligned", "wide-odd"])
@pytest.mark.parametrize("bad", [-1, "width"])
def test_grouped_ce_invalid_target_poisons_its_group_alone(cuda, C, lay, bad):
    """a target of -1 or of the segment's width on a selected row: that group's loss_k and the loss are NaN, every other
    group's loss_k stays within the bar, every gradient row is still right (the bad row's is its softmax: no class to
    subtract) and nothing outside the row's segment is read -- the columns around it hold NaN"""
    lib = _lib.load()
    base = gc.gce_inputs(C, gc.N_SMALL, "packed", "randn")
    K = len(base["starts"])
    target = base["target"].copy()
    rows = np.flatnonzero(gc.selected_rows(base))
    hit = rows[[0, len(rows) // 2]]
    for r in hit:
        target[r] = base["widths"][base["group"][r]] if bad == "width" else -1
    groups = sorted({int(base["group"][r]) for r in hit})
    assert 1 <= len(groups) < int((base["inv_count"] != 0).sum())
    inp = dict(base, target=target)
    ref = gc.grouped_ce_of(inp["x"], target, inp["mask"], inp["group"], inp["starts"], inp["widths"], inp["inv_count"])
    assert np.isnan(ref["loss"]) and np.isnan(ref["loss_k"][groups]).all() and np.isfinite(ref["grad"]).all()
    ref["loss_k"] = gc.gce_reference(C, gc.N_SMALL, "packed", "randn")["loss_k"]      # (of the groups that stay finite)
    ref["pred"] = gc.gce_reference(C, gc.N_SMALL, "packed", "randn")["pred"]
    worst = {}
    for out in ("grad", "dbias"):
        c = gc.GceCase(C, gc.N_SMALL, "packed", *lay, out, True, True, True, "randn")
        rc, got = _run(lib, cuda, c, inp, gc.poisoned(inp, True, True))
        assert rc == _lib.OK, lib.tgcn_last_error()
        assert not _check(c, got, inp, ref, worst, nan_groups=groups), worst
        assert bool(torch.isnan(got["lg_all"][c.off + c.n * (C + c.pad):]).all())
