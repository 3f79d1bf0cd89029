"""The case lists of the exact sweeps over csrc/colsum.hip and csrc/rows.hip (tests/_reduce_move_cases.py) on the CPU: every
leaf of each restated dispatch on both sides of every boundary, each cause of a scalar leaf on its own, one case above every
launch cap, and operands whose sums fp32 holds exactly -- so that thinning the lists later fails here, without a GPU."""
import numpy as np

import _reduce_move_cases as rm


def test_the_restated_launcher_choices():
    assert [rm.colsum_blocks(n) for n in (0, 1, 256, 257, 524_288, 524_289, 10 ** 7)] == [1, 1, 1, 2, 2048, 2048, 2048]
    assert [rm.colsum_leaf(F, True) for F in (4, 64, 68, 128, 132, 256, 260, 516)] == \
        [(4, 16, 1), (4, 16, 1), (4, 32, 1), (4, 32, 1), (4, 64, 1), (4, 64, 1), (4, 64, 2), (4, 64, 3)]
    assert [rm.colsum_leaf(F, False) for F in (1, 64, 65, 129, 516)] == [(1, 64, 1), (1, 64, 1), (1, 64, 2), (1, 64, 3), (1, 64, 9)]
    assert [rm.pass_rows(leaf) for leaf in rm.COLSUM_LEAVES] == [16, 8, 4, 4]
    assert [rm.final_unrolled(nb) for nb in rm.COL_BLOCKS] == [(False, True), (False, True), (False, True), (False, True),
                                                               (True, True), (True, False), (True, True), (True, False)]
    assert [rm.rows_grid(n) for n in (0, 1, 4, 5, 32_768, 32_769)] == [1, 1, 1, 2, 8192, 8192] and rm.ROWS_CAP == 32_768
    assert rm.rows_vec4(4, 4, 8, 0, 0) and not rm.rows_vec4(3, 4, 4, 0, 0) and not rm.rows_vec4(4, 5, 4, 0, 0)
    assert not rm.rows_vec4(4, 4, 5, 0, 0) and not rm.rows_vec4(4, 4, 4, 1, 0) and not rm.rows_vec4(4, 4, 4, 0, 1)


def _one_cause(cases, terms):
    """the sets of failed terms of the 16-byte test over the cases"""
    return {frozenset(name for name, bad in terms(c) if bad) for c in cases}


def test_every_colsum_and_act_grad_leaf_boundary_and_cap_is_in_the_lists():
    col, act = rm.col_cases(), rm.act_cases()
    assert len(set(col)) == len(col) and len(set(act)) == len(act)
    for cases, relu_only in ((col, False), (act, True)):
        groups = rm.by_col_leaf(cases)
        assert set(groups) == set(rm.COLSUM_LEAVES) and all(groups.values())
        Fs = {c.F for c in cases}
        assert Fs == {1, 3, 4, 64, 68, 128, 132, 256, 260, 65, 129, 516}
        for lo, hi in rm.COLSUM_EDGES:                          # both sides of every boundary, on the 16-byte leaves
            v4 = {c.F for c in cases if rm.col_leaf_of(c)[0] == 4}
            assert lo in v4 and hi in v4 and rm.colsum_leaf(lo, True) != rm.colsum_leaf(hi, True)
        scalar = groups[(1, 64)]
        assert {rm.colsum_leaf(c.F, False)[2] for c in scalar} >= {1, 2, 3, 9}               # column tiles of the scalar leaf
        assert {rm.colsum_leaf(c.F, True)[2] for c in groups[(4, 64)]} == {1, 2, 3}
        for leaf, mine in groups.items():
            ns = {c.n for c in mine}
            p = rm.pass_rows(leaf)
            assert ns >= {0, 1, p - 1, p, p + 1, 4 * p - 1, 4 * p, 4 * p + 1, 3 * p + 1, 8 * p + 1, 257}, leaf
            assert all(7 * c.n < 2 ** 24 for c in mine)
        # k_colsum_final's eight-deep unroll and its tail, and a workgroup with more than 256 rows
        for F in (4, 3):
            mine = [c for c in cases if c.F == F and (not relu_only or (c.act == rm.ACT_RELU and c.sums))]
            assert {rm.colsum_blocks(c.n) for c in mine} >= set(rm.COL_BLOCKS), F
            assert {rm.final_unrolled(rm.colsum_blocks(c.n)) for c in mine} == {(False, True), (True, True), (True, False)}
            over = [c for c in mine if c.n > rm.COLSUM_MAX_BLOCKS * rm.COLSUM_ROWS_PER_BLOCK]
            assert [c.n for c in over] == [524_289] and -(-over[0].n // rm.colsum_blocks(over[0].n)) == 257
        assert max(c.n * c.F for c in cases) <= 129 * 256 * 264
    # each cause of the scalar leaf on its own
    assert _one_cause([c for c in col if not rm.col_is_vec4(c)],
                      lambda c: (("F", c.F % 4), ("ld", (c.F + c.pad) % 4), ("base", c.off % 4))) >= \
        {frozenset(["F"]), frozenset(["ld"]), frozenset(["base"])}
    assert _one_cause([c for c in act if not rm.act_is_vec4(c)],
                      lambda c: (("F", c.F % 4), ("lda", (c.F + c.pada) % 4), ("ldg", (c.F + c.padg) % 4), ("a", c.offa % 4),
                                 ("g", c.offg % 4))) >= {frozenset([k]) for k in ("F", "lda", "ldg", "a", "g")}
    # act_grad: every leaf with and without the sums; the identity with and without them
    for leaf, mine in rm.by_col_leaf(act).items():
        assert {(c.act, c.sums) for c in mine} == {(a, s) for a in (rm.ACT_NONE, rm.ACT_RELU) for s in (True, False)}, leaf
    assert any(c.pada != c.padg for c in act if rm.act_is_vec4(c))


def test_the_colsum_operands():
    c = rm.ActCase(rm.ACT_RELU, 68, 257, 0, 0, 0, 0, True)
    A, G, want, sums = rm.act_operands(c)
    closed = ~(A > 0)
    assert np.isnan(G[closed]).all() and not np.isnan(G[~closed]).any() and np.isnan(A).any()
    assert (np.signbit(A) & (A == 0)).any() and ((A == 0) & ~np.signbit(A)).any()            # -0.0 and +0.0
    assert (want[closed] == 0).all() and not np.signbit(want[closed]).any() and np.array_equal(want[~closed], G[~closed])
    assert sums.dtype == np.int64 and np.abs(sums).max() > 0 and np.array_equal(sums, want.astype(np.int64).sum(0))
    A, G, want, sums = rm.act_operands(c._replace(act=rm.ACT_NONE))
    assert want is G and not np.isnan(G).any()
    G, sums = rm.col_operand(rm.ColCase(65, 33, 0, 0))
    assert G.min() == -7 and G.max() == 7 and np.array_equal(G, np.round(G)) and np.array_equal(sums, G.astype(np.float64).sum(0))


def test_every_row_movement_leaf_cause_and_cap_is_in_the_list():
    cases = rm.row_cases()
    assert len(set(cases)) == len(cases)
    groups = rm.by_row_leaf(cases)
    assert set(groups) == set(rm.ROW_LEAVES) and len(rm.ROW_LEAVES) == 6
    for (op, v4), mine in groups.items():
        assert {c.n for c in mine} == {0, 1, 5, 32_768, 32_769}, (op, v4)
        assert {c.F for c in mine if c.n > 5} == ({4} if v4 else {7})
        assert {c.F for c in mine} >= ({4, 252, 256, 260, 516} if v4 else {1, 3, 4, 252, 256, 260, 516})
        assert {c.skip for c in mine} == {False, True}
        assert max(c.n for c in mine) > rm.ROWS_CAP and rm.rows_grid(rm.ROWS_CAP + 1) == rm.ROWS_MAX_BLOCKS
        if v4:
            assert any(c.pads and c.padd and c.pads != c.padd for c in mine)
        else:
            causes = _one_cause(mine, lambda c: (("F", c.F % 4), ("lds", (c.F + c.pads) % 4), ("ldd", (c.F + c.padd) % 4),
                                                 ("src", c.offs % 4), ("dst", c.offd % 4)))
            assert causes >= {frozenset([k]) for k in ("F", "lds", "ldd", "src", "dst")}, (op, causes)
        if op == "reduce":
            assert {(c.W, c.step) for c in mine} >= {(1, 1), (2, 3), (8, 1)}


def test_the_row_movement_operands():
    c = rm.RowCase("gather", 4, 32_769, 4, 0, 4, 0, True, 0, 0)
    x, idx, want, n_x = rm.move_operands(c)
    inner = idx[(idx >= 0) & (idx < n_x)]
    assert n_x == c.n + rm.SPARE and len(inner) == c.n - 3 and (np.diff(inner) <= 0).all()        # descending
    assert idx[0] == -1 and idx[-1] == n_x and idx[c.n // 2] == 1 << 40
    assert (want[[0, -1, c.n // 2]] == rm.FILL).all() and np.array_equal(want[1], x[idx[1]])
    assert len(np.unique(idx)) < c.n                                          # duplicates
    x, idx, want, n_y = rm.move_operands(c._replace(op="scatter"))
    ok = (idx >= 0) & (idx < n_y)
    assert len(np.unique(idx[ok])) == ok.sum() == c.n - 3 and (want[np.setdiff1d(np.arange(n_y), idx[ok])] == rm.FILL).all()
    x, idx, want, _ = rm.move_operands(rm.RowCase("gather", 3, 5, 0, 0, 0, 0, False, 0, 0))
    assert (np.diff(idx) <= 0).all() and idx[0] == idx[1] and np.array_equal(want, x[idx])
    r = rm.RowCase("reduce", 4, 5, 0, 0, 0, 0, True, 8, 3)
    for floats in (False, True):
        recv, inv, y, want, n_recv = rm.reduce_operands(r, floats)
        assert inv.dtype == np.int32 and inv.shape == (8, 5) and (inv == -1).any() and (inv == n_recv).any() and (inv == n_recv + 5).any()
        assert (inv[:, 2] == -1).all() and want.dtype == np.float32
        rows = rm.ROW0 + np.arange(5) * 3
        untouched = np.setdiff1d(np.arange(len(y)), rows)
        assert np.array_equal(want[untouched].view(np.int32), y[untouched].view(np.int32))
        assert np.array_equal(want[rows[2]], y[rows[2]] + np.float32(0.0)) and not np.signbit(want[rows[2]][y[rows[2]] == 0]).any()
        assert (want[rows] != y[rows]).any()
    assert (np.signbit(y) & (y == 0)).any()
    recv, inv, y, want, n_recv = rm.reduce_operands(r._replace(n=0))
    assert n_recv == 0 and recv.shape == (0, 4) and np.array_equal(want, y)
