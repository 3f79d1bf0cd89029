"""CPU checks of tests/_extent_cases.py, the table behind tests/test_gpu_extents_families.py: every placed operand starts
rows in the windows it is named for and fits the pool, and every leading dimension that include/tgcn.h declares is either
placed by a case or exempted with a reason -- so a kernel added later with a leading dimension and no extents case fails
here, on any machine."""
import pytest

import _extent_cases as X


def test_tall_operands_start_rows_in_all_four_windows():
    for rows in (X.TALL_MIN_ROWS, X.TALL_ROWS):
        p = X.place("tall", rows, 100)
        assert p.ld == 1 << 24 and X.windows_hit(rows, p.ld) == X.WINDOWS
    assert X.TALL_ROWS == 273 and X.TALL_ROWS > 2 * 128 and X.TALL_ROWS % 4 and X.TALL_ROWS % 128
    with pytest.raises(AssertionError):
        X.place("tall", 256, 100)                      # no row at or past 2^32 elements
    # the row of each window's first start: 2^31 B, 2^32 B, 2^31 and 2^32 elements at ld = 2^24
    assert [r * X.TALL_LD for r in (32, 64, 128, 256)] == [1 << 29, 1 << 30, 1 << 31, 1 << 32]


@pytest.mark.parametrize("rows", [3, 4, 5, 6, 7, 12, 24, 56, 63])
def test_short_operands_put_their_last_row_at_or_past_2_to_the_32(rows):
    p = X.place("short", rows, 7)
    assert p.ld % 4 == 0 and (rows - 1) * p.ld >= 1 << 32
    assert (rows - 1) * (p.ld - 4) < 1 << 32           # the smallest such multiple of 4
    assert 4 * p.pool_elems <= X.POOL_LIMIT_BYTES
    for bad in (2, 64):
        with pytest.raises(AssertionError):
            X.place("short", bad, 7)                   # fewer than 3 rows are not placed; 64 and more are tall


def test_planes_pass_2_to_the_32_with_the_plane_offset_alone():
    op = X.operand("tgcn_jk_attention", "h")
    p = X.placement_of(op)
    assert p.hstep == p.rows * p.ld and (p.planes - 1) * p.hstep >= 1 << 32 and p.ld % 4 == 0
    assert 4 * p.pool_elems <= X.POOL_LIMIT_BYTES


def test_margin_keeps_every_wrapped_offset_inside_the_pool():
    assert X.MARGIN >= 1 << 31 and (4 * X.MARGIN) % 16 == 0
    for _, ops in X.ENTRIES.values():
        for op in ops:
            p = X.placement_of(op)
            last = (p.planes - 1) * p.hstep + (p.rows - 1) * p.ld + p.width - 1          # the view's last element
            assert X.MARGIN + last < p.pool_elems
            for el in (last, (p.rows - 1) * p.ld):
                wraps = [el - (1 << 32) if el & (1 << 31) else el & 0x7FFFFFFF,          # int32 element index
                         el & 0xFFFFFFFF,                                                # uint32 element index
                         (4 * el & 0xFFFFFFFF) // 4,                                     # uint32 byte offset
                         ((4 * el & 0xFFFFFFFF) - (1 << 32 if 4 * el & (1 << 31) else 0)) // 4]      # int32 byte offset
                assert all(0 <= X.MARGIN + w < p.pool_elems for w in wraps), (op, el, wraps)


def test_every_case_fits_the_pool_and_names_its_windows():
    assert len(X.CASES) == len(set(X.CASES))
    for c in X.CASES:
        op = X.operand(c.entry, c.operand)
        p = X.placement_of(op)                                                       # (asserts the windows of its kind)
        assert 4 * p.pool_elems <= 32 * X.GiB, (c, p)
        assert p.ld % 4 == 0 and p.ld >= op.width
        if op.kind == "tall":
            assert X.windows_hit(op.rows, p.ld) == X.WINDOWS, c
        assert op.io in ("in", "out", "inout") and op.dtype in ("f32", "i32")
        assert op.dtype == "f32" or op.io == "in"
    assert 26 * X.GiB < 4 * X.pool_elems() <= 32 * X.GiB
    # the dropout products run at p = 0 and p = 0.5
    for entry, (rates, _) in X.ENTRIES.items():
        fused_dropout = entry.startswith(("tgcn_blockdiag", "tgcn_embed", "tgcn_mlp"))
        assert rates == ((0.0, 0.5) if fused_dropout else (None,)), entry


def test_the_header_parse_sees_the_leading_dimensions():
    d = X.declared_leading_dimensions()
    assert d["tgcn_jk_attention"] == ["ldxs", "ldh", "hstep", "ldo", "lda"]
    assert d["tgcn_spmm"] == ["ldx", "ldy"] and d["tgcn_act_grad"] == ["lda", "ldg"]
    assert d["tgcn_embed_xw_members_grad"] == ["lde", "ldeh", "ldh", "ldw", "ldg", "ldde", "lddeh", "lddw"]
    assert "tgcn_adam_members" not in d and "tgcn_plan_create" not in d
    assert len(d) >= 50


def test_every_declared_leading_dimension_is_placed_or_exempt():
    declared = X.declared_leading_dimensions()
    assert X.uncovered() == [], f"no extents case and no exemption for {X.uncovered()}"
    for entry in list(X.ENTRIES) + list(X.EXEMPT):
        assert entry in declared, f"{entry} is not an entry point with a leading dimension in include/tgcn.h"
    assert not set(X.ENTRIES) & set(X.EXEMPT)
    assert all(len(reason) > 20 for reason in X.EXEMPT.values())
    # every parameter a case names exists in the declaration
    for entry, (_, ops) in X.ENTRIES.items():
        for op in ops:
            assert set(op.params) <= set(declared[entry]), (entry, op.name)


def test_a_deleted_case_is_named():
    entries = dict(X.ENTRIES)
    rates, ops = entries["tgcn_jk_cell"]
    entries["tgcn_jk_cell"] = (rates, [op for op in ops if op.name != "c_prev"])
    assert X.uncovered(entries) == [("tgcn_jk_cell", "ldcp")]
    del entries["tgcn_act_grad"]
    assert ("tgcn_act_grad", "lda") in X.uncovered(entries) and ("tgcn_act_grad", "ldg") in X.uncovered(entries)
    # an entry point added to the header later
    later = "int tgcn_new_product(const float *A, int64_t lda, float *C, int64_t ldc, int64_t N, tgcn_stream stream);"
    assert X.uncovered(declared=X.declared_leading_dimensions(later)) == [("tgcn_new_product", "lda"), ("tgcn_new_product", "ldc")]
