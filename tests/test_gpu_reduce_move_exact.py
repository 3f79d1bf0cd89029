"""`tgcn_colsum` and `tgcn_act_grad` (csrc/colsum.hip) and `tgcn_rows_gather`, `tgcn_rows_scatter`,
`tgcn_rows_reduce_ranked` (csrc/rows.hip) at every dispatch leaf, bit for bit, through the C ABI with raw pointers.  The
cases, the operands and the int64 references are tests/_reduce_move_cases.py's; tests/test_reduce_move_cases.py keeps the
lists complete on the CPU.

Operands are integers in [-7, 7] with 7 * n_rows < 2^24: every partial sum is an integer fp32 holds, so the result is exact
whatever the order -- a row dropped, added twice or handed to the wrong column is a wrong bit.  Every output is a view in a
guarded pool (tests/_arena.py) filled with 7 -- padding columns, the rows around it and everything misalignment skips must
still hold 7 afterwards --, the workspace has exactly the advertised size, starts as NaN and has a guard behind it.

  colsum / act_grad   {16, 32, 64 lanes float4, scalar} x F on both sides of 64 | 68, 128 | 132, 256 | 260, 65 / 129 / 516 (more
                      than one column tile) x strides and bases that force the scalar leaf one cause at a time x row counts
                      around one pass and around the unrolled loop's stride; 1 .. 2048 partial rows for k_colsum_final's
                      eight-deep unroll and its tail; 2048 * 256 + 1 rows.  act_grad with and without the sums, A holding
                      0, -0.0 and NaN (gate closed), G holding NaN exactly there: +0.0 comes out, the sums do not see it.
  rows                {gather, scatter, ranked reduction} x {float4, scalar}, source and destination strided and shifted
                      apart; 32 768 and 32 769 rows (the grid cap: a wave takes a second row); duplicate and descending
                      indices, a permutation, out-of-range indices that must leave the sentinel; W = 1, 2, 8 ranks, a row
                      step of 3, skipped table entries, recv == NULL; one fp32 family against the documented order."""
import numpy as np
import pytest
import torch

import _reduce_move_cases as rm
from _arena import _Arena
from pytextgcn_amd import _lib

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64


class _Pools:
    """the pools the arenas of this module carve their views from (kept across cases)"""
    pool = None

    def __init__(self, dev):
        self.dev = dev


@pytest.fixture(scope="module")
def pools(cuda):
    return _Pools(cuda)


def _place(cuda, a, ld, off, fill=float("nan")):
    """an input matrix with rows of `ld` floats, `off` floats into a 16-byte aligned allocation, NaN in its padding; returns
    (allocation, address)"""
    n, F = a.shape
    base = torch.full((max(n, 1) * ld + off + 4,), fill, dtype=F32, device=cuda)
    assert base.data_ptr() % 16 == 0
    if n:
        base[off:off + n * ld].view(n, ld)[:, :F] = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return base, base.data_ptr() + 4 * off


def _bits(t):
    return t.contiguous().view(I32)


def _same(got, want):
    """bit equality of a device fp32 view with a host float32 array"""
    return torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32))))


def _workspace(cuda, n_bytes):
    """exactly `n_bytes` of NaN inside a larger NaN allocation: (allocation, address, the part behind the workspace)"""
    assert n_bytes % 4 == 0
    ws = torch.full((n_bytes // 4 + 64,), float("nan"), dtype=F32, device=cuda)
    return ws, ws.data_ptr(), ws[n_bytes // 4:]


# ---- tgcn_colsum / tgcn_act_grad -------------------------------------------------------------------------------------
def _run_colsum(lib, pools, c):
    G, want = rm.col_operand(c)
    keep, g_ptr = _place(pools.dev, G, c.F + c.pad, c.off)
    arena = _Arena(pools, "pool", F32)
    out = arena.take(1, c.F, c.F, 1)                              # (the sums need no alignment)
    arena.fill(rm.FILL)
    need = lib.tgcn_colsum_workspace_bytes(c.n, c.F)
    assert need == 4 * rm.colsum_blocks(c.n) * c.F
    ws, ws_ptr, tail = _workspace(pools.dev, need)
    assert lib.tgcn_colsum(g_ptr, c.F + c.pad, c.n, c.F, arena.ptr(out), ws_ptr, need - 1, None) == _lib.E_WORKSPACE
    assert arena.untouched() and bool((arena.view(out) == rm.FILL).all())
    assert lib.tgcn_colsum(g_ptr, c.F + c.pad, c.n, c.F, arena.ptr(out), ws_ptr, need, None) == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    assert _same(arena.view(out)[0], want.astype(np.float32)), c
    assert arena.untouched() and bool(torch.isnan(tail).all()), c


def _run_act(lib, pools, c):
    A, G, want, sums = rm.act_operands(c)
    keep, a_ptr = _place(pools.dev, A, c.F + c.pada, c.offa)
    arena = _Arena(pools, "pool", F32)
    g = arena.take(c.n, c.F, c.F + c.padg, c.offg)
    out = arena.take(1, c.F, c.F, 1)
    arena.fill(rm.FILL)
    if c.n:
        arena.view(g).copy_(torch.from_numpy(G).to(pools.dev))
    need = lib.tgcn_act_grad_workspace_bytes(c.n, c.F)
    assert need == 4 * rm.colsum_blocks(c.n) * c.F
    ws, ws_ptr, tail = _workspace(pools.dev, need)
    args = (c.act, a_ptr, c.F + c.pada, arena.ptr(g), c.F + c.padg, c.n, c.F)
    if c.sums:
        assert lib.tgcn_act_grad(*args, arena.ptr(out), ws_ptr, need - 1, None) == _lib.E_WORKSPACE
        rc = lib.tgcn_act_grad(*args, arena.ptr(out), ws_ptr, need, None)
    else:
        rc = lib.tgcn_act_grad(*args, None, None, 0, None)       # (no sums: no workspace either)
    assert rc == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    assert _same(arena.view(g), want), c                          # +0.0 where the gate is closed, G's own bits elsewhere
    if c.sums:
        assert _same(arena.view(out)[0], sums.astype(np.float32)), c
    else:
        assert bool((arena.view(out) == rm.FILL).all()) and bool(torch.isnan(ws).all()), c
    assert arena.untouched() and bool(torch.isnan(tail).all()), c


_COL, _ACT = rm.by_col_leaf(rm.col_cases()), rm.by_col_leaf(rm.act_cases())


@pytest.mark.parametrize("leaf", rm.COLSUM_LEAVES, ids=rm.col_leaf_id)
def test_colsum_is_exact_on_every_leaf(cuda, pools, leaf):
    lib = _lib.load()
    for c in _COL[leaf]:
        _run_colsum(lib, pools, c)
    print(f"\ncolsum {rm.col_leaf_id(leaf)}: {len(_COL[leaf])} cases bit for bit")


@pytest.mark.parametrize("leaf", rm.COLSUM_LEAVES, ids=rm.col_leaf_id)
def test_act_grad_is_exact_on_every_leaf(cuda, pools, leaf):
    lib = _lib.load()
    for c in _ACT[leaf]:
        _run_act(lib, pools, c)
    print(f"\nact_grad {rm.col_leaf_id(leaf)}: {len(_ACT[leaf])} cases bit for bit")


# ---- tgcn_rows_* -----------------------------------------------------------------------------------------------------
def _run_move(lib, pools, c):
    x, idx, want, n_indexed = rm.move_operands(c)
    keep, x_ptr = _place(pools.dev, x, c.F + c.pads, c.offs)
    d_idx = torch.from_numpy(np.append(idx, 0)).to(pools.dev)      # (one element more: a real address at n = 0)
    arena = _Arena(pools, "pool", F32)
    dst = arena.take(want.shape[0], c.F, c.F + c.padd, c.offd)
    arena.fill(rm.FILL)
    if c.op == "gather":
        rc = lib.tgcn_rows_gather(x_ptr, c.F + c.pads, n_indexed, d_idx.data_ptr(), c.n, c.F, arena.ptr(dst), c.F + c.padd, None)
    else:
        rc = lib.tgcn_rows_scatter(x_ptr, c.F + c.pads, d_idx.data_ptr(), c.n, c.F, arena.ptr(dst), c.F + c.padd, n_indexed, None)
    assert rc == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    assert _same(arena.view(dst), want), c                        # skipped and unaddressed rows: the sentinel
    assert arena.untouched(), c


def _run_reduce(lib, pools, c, floats=False, null_recv=False):
    recv, inv, y, want, n_recv = rm.reduce_operands(c, floats)
    if null_recv:                                                 # no rank sent anything: every entry is skipped, y + 0 remains
        n_recv, want = 0, y.copy()
        rows = rm.ROW0 + np.arange(c.n) * c.step
        want[rows] = y[rows] + np.float32(0.0)
    keep, r_ptr = _place(pools.dev, recv, c.F + c.pads, c.offs)
    d_inv = torch.from_numpy(np.append(inv.reshape(-1), np.int32(0))).to(pools.dev)
    arena = _Arena(pools, "pool", F32)
    dst = arena.take(y.shape[0], c.F, c.F + c.padd, c.offd)
    arena.fill(rm.FILL)
    arena.view(dst).copy_(torch.from_numpy(y).to(pools.dev))
    rc = lib.tgcn_rows_reduce_ranked(None if null_recv else r_ptr, c.F + c.pads, n_recv, d_inv.data_ptr(), c.W, c.n, c.F, arena.ptr(dst),
                                     c.F + c.padd, y.shape[0], rm.ROW0, c.step, None)
    assert rc == _lib.OK, lib.tgcn_last_error()
    torch.cuda.synchronize()
    assert _same(arena.view(dst), want), (c, floats, null_recv)
    assert arena.untouched(), c


_ROWS = rm.by_row_leaf(rm.row_cases())


@pytest.mark.parametrize("leaf", rm.ROW_LEAVES, ids=rm.row_leaf_id)
def test_row_movement_is_exact_on_every_leaf(cuda, pools, leaf):
    lib = _lib.load()
    for c in _ROWS[leaf]:
        if c.op == "reduce":
            _run_reduce(lib, pools, c)
        else:
            _run_move(lib, pools, c)
    print(f"\nrows {rm.row_leaf_id(leaf)}: {len(_ROWS[leaf])} cases bit for bit")


@pytest.mark.parametrize("F,lay", [(260, (4, 0, 8, 0)), (7, (1, 1, 2, 3))], ids=["v4", "scalar"])
def test_ranked_reduction_adds_in_the_documented_order_and_without_a_receive_buffer(cuda, pools, F, lay):
    """fp32 operands: zero, plus the ranks in rank order, then one add into y -- evaluated in fp32 on the host, bit for bit;
    and recv == NULL with n_recv_rows = 0, where y + 0 remains (-0.0 becomes +0.0 in the rows the call names, nowhere else)"""
    lib = _lib.load()
    for W, step in ((1, 1), (2, 3), (8, 1)):
        c = rm.RowCase("reduce", F, 37, *lay, True, W, step)
        _run_reduce(lib, pools, c, floats=True)
        _run_reduce(lib, pools, c, null_recv=True)
        _run_reduce(lib, pools, c._replace(n=0), null_recv=True)
