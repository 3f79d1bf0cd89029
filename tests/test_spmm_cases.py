"""CPU checks of the SpMM sweep's case table (tests/_spmm_cases.py): the restated dispatch against hand-written
expectations on both sides of every boundary, every leaf reached in every layout that applies to it, the exactness bound,
and the structure of the operators that the branches inside the leaves need."""
import numpy as np

import _spmm_cases as sc

SEGS, SHORT = sc.make_op("segs"), sc.make_op("short")
HOT40, HOT12 = sc.make_op("hot40", 4097), sc.make_op("hot12", 4100)
ALL = sc.int_cases()


def _case(op, form, F, lay="tight", bias=None, split=None, t=0):
    bias = form in ("plain", "relu", "split") if bias is None else bias
    return sc.Case(op, t, form, F, lay, bias, split, sc._ADAMS[0] if form == "adam" else None)


def test_leaf_of_on_both_sides_of_every_boundary():
    # the hot kernel's tile count: 32 k | 32 k + 4 for k = 1 .. 8, and the second grid row above 256
    for k in range(1, 9):
        assert f"hot<{k}>" in sc.leaf_of(_case(HOT40, "plain", 32 * k))
        assert f"hot<{min(k + 1, 8)}>" in sc.leaf_of(_case(HOT40, "plain", 32 * k + 4))
        assert sc.hot_nt(32 * k) == (k, 1)
    assert sc.hot_nt(256) == (8, 1) and sc.hot_nt(260) == (8, 2) and sc.hot_nt(512) == (8, 2) and sc.hot_nt(516) == (8, 3)
    # the sub-group kernel: G = 16 up to 64, G = 32 up to 128, the full-wave kernel above
    for form, tag in (("plain", ""), ("acc", ",acc"), ("relu", ",relu")):
        p = {"plain": "P3", "acc": "P1", "relu": "P3"}[form]
        assert sc.leaf_of(_case(SEGS, form, 64)) == {f"subb<16{tag}>", f"fix<4{tag}>"}
        assert sc.leaf_of(_case(SEGS, form, 68)) == {f"subb<32{tag}>", f"fix<4{tag}>"}
        assert sc.leaf_of(_case(SEGS, form, 128)) == {f"subb<32{tag}>", f"fix<4{tag}>"}
        assert sc.leaf_of(_case(SEGS, form, 132)) == {f"gather<4,{p}{tag}>", f"fix<4{tag}>"}
        assert sc.leaf_of(_case(SEGS, form, 256)) == sc.leaf_of(_case(SEGS, form, 260)) == {f"gather<4,{p}{tag}>", f"fix<4{tag}>"}
        # F % 4 and every alignment rule
        assert sc.leaf_of(_case(SEGS, form, 130)) == {f"gather<1,P0{tag}>", f"fix<1{tag}>"}
        for lay in ("odd_ldx", "odd_ldy", "x_off", "y_off") + (("bias_off",) if form != "acc" else ()):
            assert sc.leaf_of(_case(SEGS, form, 64, lay)) == {f"gather<1,P0{tag}>", f"fix<1{tag}>"}, (form, lay)
        assert sc.leaf_of(_case(SEGS, form, 64, "pad")) == {f"subb<16{tag}>", f"fix<4{tag}>"}
        assert sc.leaf_of(_case(SHORT, form, 64)) == {f"subb<16{tag}>"}                    # no long row: nothing to fix
    assert sc.tiles(_case(SEGS, "plain", 256)) == 1 and sc.tiles(_case(SEGS, "plain", 260)) == 2
    assert sc.tiles(_case(SEGS, "plain", 64, "odd_ldx")) == 1 and sc.tiles(_case(SEGS, "plain", 65)) == 2
    assert sc.tiles(_case(SEGS, "plain", 129)) == 3
    # a split operand takes the full-wave kernel at any width; its own alignment rules
    assert sc.leaf_of(_case(SEGS, "split", 64, split=450)) == {"gather<4,P3>", "fix<4>"}
    assert sc.leaf_of(_case(SEGS, "acc", 128, split=450)) == {"gather<4,P1,acc>", "fix<4,acc>"}
    assert sc.leaf_of(_case(SEGS, "split", 64, "x2_off", split=450)) == {"gather<1,P0>", "fix<1>"}
    assert sc.leaf_of(_case(SEGS, "split", 64, "odd_ldx2", split=450)) == {"gather<1,P0>", "fix<1>"}
    assert sc.leaf_of(_case(SEGS, "plain", 64, "bias_off", bias=False)) == {"subb<16>", "fix<4>"}    # no bias: no rule
    assert not sc.buf_ok(_case(SEGS, "split", 64, split=450)) and sc.buf_ok(_case(SEGS, "plain", 64))
    # the optimizer epilogue
    assert sc.leaf_of(_case(SEGS, "adam", 64)) == {"gather_adam<4>", "fix<4,adam>"}
    assert sc.leaf_of(_case(HOT40, "adam", 200)) == {"hot<7>", "gather_adam<4>", "fix<4,adam>"}
    # hot or not: the float4 kernels run next to the hot block, the scalar kernels on the complete partition
    assert sc.leaf_of(_case(HOT40, "relu", 64)) == {"hot<2>", "subb<16,relu>", "fix<4,relu>"}
    assert sc.leaf_of(_case(HOT40, "relu", 65)) == {"gather<1,P0,relu>", "fix<1,relu>"}
    assert sc.leaf_of(_case(HOT40, "plain", 64, t=1)) == {"subb<16>", "fix<4>"}            # 300 columns: no hot block
    cold = sc.make_op("hot40", 4097, knobs=(("TGCN_HOT_ROWS", "0"),))
    assert sc.leaf_of(_case(cold, "plain", 200)) == {"gather<4,P3>", "fix<4>"}


def test_restated_partition_of_the_operators():
    f = sc.facts(SHORT, 0)
    assert f.T == 128 and not f.long_rows and f.segments == 0 and f.n_hot == 0
    sizes = [e - b for b, e in f.blocks]
    assert max(sizes) == 128 and any(all(f.deg[r] == 0 for r in range(b, e)) and e - b == 128 for b, e in f.blocks)
    b0, e0 = f.blocks[0]
    assert b0 == 0 and e0 > 70 and all(f.deg[r] == 0 for r in range(70)) and all(f.deg[r] > 0 for r in range(70, e0))
    assert any(e - b > 66 and [f.deg[b + i] for i in (62, 63, 64, 65, 66)] == [0, 1, 1, 1, 0] for b, e in f.blocks)
    assert f.deg[-1] == 0 and set(range(1, 13)) <= set(f.deg.tolist())
    f = sc.facts(SEGS, 0)
    assert f.T == 64 and f.n_hot == 0 and f.exact_segments
    assert {65, 129, 900}.issubset({int(f.deg[r]) for r in f.long_rows}) and 64 in f.deg and 0 in f.long_rows
    assert len(f.deg) - 1 in f.long_rows
    assert set(sc.SEGS_COUNTS) <= set(f.seg_counts.values()), sorted(set(f.seg_counts.values()))
    assert f.segments == sum(f.seg_counts.values()) and f.segments_all == 0
    n_rows, n_cols, rows, cols, _ = sc.structure(SEGS)
    full = np.unique(cols[rows == 8])
    assert full.size == 900 and (rows == 8).sum() == 900
    assert len(sc.facts(SEGS, 1).long_rows) >= 3                                           # the hub columns
    # the three loops of k_spmm_fix: a wave enters the 8-way loop at s + 28 < count, the 4-way one at s + 12 < count
    eight = [c for c in f.seg_counts.values() if c > 28]
    assert any(c % 32 for c in eight) and any(12 < c <= 28 for c in f.seg_counts.values())
    f = sc.facts(HOT12, 0)
    assert f.n_hot == 12 == len(f.long_rows) and f.hot_cpw == 64 and f.hot_parts == 9 and f.segments == 12 * 9
    f = sc.facts(HOT40, 0)
    assert f.n_hot == 32 and len(f.long_rows) == 40 and f.hot_parts == 9
    assert f.segments == 32 * 9 + sum(c for r, c in f.seg_counts.items() if r not in f.hot_rows)
    assert f.segments_all == sum(f.seg_counts.values())
    assert min(f.deg[r] for r in f.hot_rows) >= max(f.deg[r] for r in f.long_rows if r not in f.hot_rows)
    assert sc.facts(sc.make_op("hot40", 4096), 0).hot_parts == 8 and sc.facts(sc.make_op("hot40", 4100), 0).hot_parts == 9
    assert sc.facts(sc.make_op("hot40", 4096, swap=True), 1).n_hot == 32
    assert sc.facts(sc.make_op("hot40", 4097, knobs=(("TGCN_HOT_ROWS", "0"),)), 0).n_hot == 0
    f = sc.facts(sc.make_op("hot_parts34"), 0)
    assert f.n_hot == 32 and f.hot_parts == 34 and f.hot_cpw == 64 and len(f.long_rows) == 34
    f = sc.facts(sc.make_op("hot_cpw72"), 0)
    assert f.n_hot == 32 and f.hot_cpw == 72 and f.hot_parts == 228
    # the hot rows hold duplicate columns, column 0 and the last column
    for op in (HOT12, HOT40):
        n_rows, n_cols, rows, cols, _ = sc.structure(op)
        for r in sc.facts(op, 0).hot_rows:
            c = cols[rows == r]
            assert (c == 0).sum() >= 4 and (c == n_cols - 1).sum() >= 4 and np.unique(c).size < c.size
    for op in {c.op for c in ALL}:
        n_rows, n_cols, rows, cols, vals = sc.structure(op)
        assert rows.size <= 100_000 and set(np.unique(vals).tolist()) <= {-3, -2, -1, 1, 2, 3}, sc.op_id(op)
        assert rows.min() >= 0 and rows.max() < n_rows and cols.min() >= 0 and cols.max() < n_cols


def test_every_leaf_in_every_layout_that_applies():
    by_leaf = {}
    for c in ALL:
        for leaf in sc.leaf_of(c):
            by_leaf.setdefault(leaf, []).append(c)
    assert set(by_leaf) == set(sc.LEAVES), set(sc.LEAVES) ^ set(by_leaf)
    for leaf in sc.LEAVES:
        lays = {c.layout for c in by_leaf[leaf]}
        assert {"tight", "pad"} <= lays, (leaf, lays)
    for leaf in sc.SCALAR_LEAVES:
        causes = {c.layout for c in by_leaf[leaf] if c.F % 4 == 0}
        want = {l for l in sc.SCALAR_CAUSES if not ("acc" in leaf and l == "bias_off")}
        if "relu" in leaf:
            want -= {"x2_off", "odd_ldx2"}                   # tgcn_spmm_act takes one operand
        assert causes == want, (leaf, causes ^ want)
        assert any(c.F % 4 for c in by_leaf[leaf]), leaf


def test_exact_bound_and_operand_size_of_every_case():
    for c in ALL:
        assert sc.exact_bound(c) < sc.EXACT_LIMIT, sc.case_id(c)
    for c in ALL + sc.float_cases():
        assert sc.operand_bytes(c) < sc.BYTES_CAP, (sc.case_id(c), sc.operand_bytes(c))
        assert c.form != "adam" or c.F % 4 == 0
        assert c.split is None or 0 <= c.split < sc.applied(c.op, c.t)[1]


def test_case_ids_are_unique_and_every_width_and_form_occurs():
    ids = [sc.case_id(c) for c in ALL + sc.float_cases()]
    assert len(set(ids)) == len(ids)
    for op in (SEGS, HOT40):
        for t in (0, 1):
            for form in ("plain", "relu"):
                got = {c.F for c in ALL if c.op == op and c.t == t and c.form == form and c.bias and c.layout == "tight"}
                assert set(sc.FLOAT4_WIDTHS + sc.SCALAR_WIDTHS) <= got, (sc.op_id(op), t, form)
    for op in (SHORT, SEGS, HOT12):
        for F in sc.PIVOTS:
            mine = [c for c in ALL if c.op == op and c.F == F]
            assert {c.form for c in mine} == set(sc.FORMS)
            assert {c.layout for c in mine} == set(sc.LAYOUTS)
            assert {(c.bias, c.form) for c in mine} >= {(True, "plain"), (False, "plain"), (True, "relu"), (False, "relu")}
            assert {c.split is None for c in mine if c.form == "acc"} == {True, False}
            n_in = sc.applied(op, 0)[1]
            assert {0, 1, n_in // 2, n_in - 1} <= {c.split for c in mine if c.form == "split"}
            adams = [c for c in mine if c.form == "adam"]
            assert {(a.adam.amsgrad, a.adam.wd > 0, a.adam.dev) for a in adams} >= {(True, False, False), (False, True, False),
                                                                                    (True, True, True), (False, False, True)}
            assert any(a.split is not None for a in adams) and any(sc.layout(a).ldp > F for a in adams)
    assert any(c.split == 700 and sc.facts(c.op, c.t).n_hot for c in ALL)
    assert {c.F for c in ALL if c.op.name == "hot_parts34"} <= set(range(65))
    assert {c.F for c in ALL if c.op.name == "hot_cpw72"} == {8, 32}
    knob_sets = {c.op.knobs for c in ALL if c.op.name == "segs"}
    assert len(knob_sets) == 3
    print(f"\n{len(ALL)} integer cases in {len(sc.grouped(ALL))} items, {len(sc.float_cases())} float cases")


def test_relu_and_acc_cases_can_tell_their_form():
    for c in sorted((c for c in ALL if c.form == "relu"), key=lambda c: (sc.op_id(c.op), c.t, c.F)):
        pre = sc.reference(c)["pre"]
        assert (pre < 0).mean() >= 0.1 and (pre > 0).mean() >= 0.1, (sc.case_id(c), (pre < 0).mean(), (pre > 0).mean())
    for c in ALL:
        if c.form == "acc":
            deg = sc.facts(c.op, c.t).deg
            assert (deg == 0).any() and (deg > 0).any(), sc.case_id(c)
