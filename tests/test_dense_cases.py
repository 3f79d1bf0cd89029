"""The case list of the exact dense sweep (tests/_dense_cases.py) on the CPU: the bound that makes "any correct kernel
returns these exact bits in any summation order" true holds for EVERY case, and the generated list contains every named
boundary, form and layout -- so that thinning the list later cannot silently drop an edge."""
import numpy as np

import _dense_cases as dc


def test_every_case_stays_below_two_to_the_24():
    cases = dc.all_cases()
    assert len(cases) > 10_000
    for c in cases:
        assert c.amax in (1, 2, 3) and dc.exact_bound(c) < dc.EXACT_LIMIT, c
        if c.p is not None:
            s = dc.scale_of(c.p)
            assert c.p in (0.0, 0.5, 0.75, 1.0) and s in (0.0, 1.0, 2.0, 4.0), c        # a power of two (or zero): exact
    lists = [dc.sweep_cases(f) for f in dc.FORMS] + [dc.big_cases(), dc.split_cases(), dc.foreign_record_cases(),
                                                     dc.edge_rate_cases() + dc.keyed_cases() + dc.zero_row_cases()]
    for one in lists:                                                                   # ids name their leaf uniquely
        assert len({dc.case_id(c) for c in one}) == len(one)
        groups = dc.grouped(one)                                                        # grouping loses and repeats nothing
        assert sorted(c for g in groups for c in g) == sorted(one)
        assert all(len({(c.family, c.form, c.k) for c in g}) == 1 for g in groups)


def test_every_named_boundary_form_and_layout_is_in_the_list():
    for family, forms in dc.FORMS.items():
        cases = dc.sweep_cases(family)
        seen = {(c.form, c.k, c.n) for c in cases}
        pairs = {(c.k, c.n) for c in cases}
        ks, ns = {k for k, _ in pairs}, {n for _, n in pairs}
        for lo, hi in dc.N_EDGES:
            assert lo in ns and hi in ns, (family, lo, hi)
            for k in dc.K_PIVOTS:                                  # both sides of the edge at the SAME reduction
                assert (k, lo) in pairs and (k, hi) in pairs, (family, k, lo, hi)
        for k in dc.K_MOD8:
            assert k in ks and k % 8 in {v % 8 for v in ks}
        assert {k % 8 for k in ks} == set(range(8))
        for lo, hi in dc.K_EDGES:
            for n in dc.N_PIVOTS:
                assert (lo, n) in pairs and (hi, n) in pairs, (family, lo, hi, n)
        for pair in dc.LDS_EDGE + dc.LDS_EDGE_COLSUM + dc.SPECIAL_PAIRS:
            assert pair in pairs, (family, pair)
        for k, n in pairs:
            for form in forms:
                if family == "nn" and form == "recorded" and k > 256:
                    assert (form, k, n) not in seen                # refused, pinned by REFUSED_RECORD_SHAPES
                    continue
                here = [c for c in cases if (c.form, c.k, c.n) == (form, k, n)]
                assert {c.layout for c in here} == set(dc.LAYOUTS), (family, form, k, n)
                for lay in dc.LAYOUTS:
                    rows = {c.N for c in here if c.layout == lay}
                    assert rows == set(dc.N_AXIS_ROWS), (family, form, k, n, lay)       # the WHOLE N axis at every leaf
    assert dc.N_AXIS_ROWS == (0, 1, 31, 32, 33, 127, 129, 1024, 1025)
    assert all(k > 256 for k, _ in dc.REFUSED_RECORD_SHAPES) and {k for k, _ in dc.RECORDED_AT_THE_EDGE} == {256}
    assert any(k == 257 for k, _ in dc.REFUSED_RECORD_SHAPES)
    big = dc.big_cases()
    assert {c.family for c in big} == set(dc.FORMS)
    assert any(c.family == "tn" and c.N > 512 * 1024 for c in big)
    # the persistent grid of nn / nt really loops: more rows than one pass of the largest grid (4 blocks x 256 CUs x 4
    # resident workgroups x 32 rows) -- the nt product that masks from the record against ITS grid (two workgroups per CU)
    assert dc.ROWS_OF_ONE_GRID_PASS == 131072 and dc.ROWS_OF_ONE_RECORD_GRID_PASS == 65536
    for c in big:
        if c.family == "tn":
            continue
        if c.N == dc.N_PERSISTENT_RECORD:
            assert (c.form, c.k, c.layout) == ("colsum_recorded", 64, "pad") and 192 < c.n <= 224
            assert c.N > dc.ROWS_OF_ONE_RECORD_GRID_PASS
        else:
            assert c.N > dc.ROWS_OF_ONE_GRID_PASS, c
    small = dc.edge_rate_cases() + dc.keyed_cases() + dc.zero_row_cases()
    for family, forms in dc.FORMS.items():
        for form in forms:
            mine = [c for c in small if (c.family, c.form) == (family, form)]
            assert any(c.N == 0 for c in mine)
            if dc.has_drop(form):
                assert {0.0, 1.0} <= {c.p for c in mine} and any(c.keys == dc.ROW_KEYS for c in mine), (family, form)
    foreign = dc.foreign_record_cases()
    assert {(c.family, c.form) for c in foreign} == {("tn", "recorded"), ("nt", "colsum_recorded")}
    for c in foreign:                       # the record differs from the hash, and the reference follows the record
        assert c.foreign and c.k <= 256 and c.layout in ("pad", "tight")
        own = dc.keep_of(*dc.mask_shape(c), c.p)
        assert (dc.reference(c)["keep"] != own).mean() > 0.3
    split = dc.split_cases()
    for family, pairs in dc.SPLIT_SHAPES.items():
        assert {(c.k, c.n) for c in split if c.family == family} == set(pairs)


def test_layouts_keep_the_header_contract_and_leave_the_free_arguments_free():
    for c in dc.all_cases():
        lay = dc.layout(c)
        (_, wa), (_, wb), (_, wc) = dc.shapes(c)
        assert lay.lda >= wa and lay.ldb >= wb and lay.ldc >= wc and lay.mask_stride >= dc.mask_words(dc.mask_shape(c)[1])
        if c.family != "tn":
            assert lay.lda % 4 == 0 and lay.off_a == 0
        if c.layout == "odd":
            assert lay.ldb % 4 and lay.ldc % 4 and lay.off_b % 4 and lay.off_c % 4 and lay.off_mask % 4
            assert c.family != "tn" or (lay.lda % 4 and lay.off_a % 4)
            assert lay.lda > wa                                         # NaNs right behind each row of A
        if c.layout == "shift":                                         # the base alignment alone is off
            assert lay.ldb % 4 == 0 and lay.ldc % 4 == 0 and lay.mask_stride % 4 == 0 and lay.lda % 4 == 0
            assert lay.off_b % 4 and lay.off_c % 4 and lay.off_mask % 4 and (c.family != "tn" or lay.off_a % 4)
        if c.layout == "pad":
            assert lay.off_a == lay.off_b == lay.off_c == lay.off_mask == 0
            assert lay.lda % 4 == 0 and lay.ldb % 4 == 0 and lay.ldc % 4 == 0 and lay.lda >= wa + 4 and lay.mask_stride % 4 == 0
        if c.layout == "tight":
            assert lay.ldb == wb and lay.ldc == wc and lay.lda == (wa if c.family == "tn" else (wa + 3) // 4 * 4)


def test_reference_operands_and_record_round_trip():
    rng = np.random.default_rng(5)
    for width in (1, 3, 4, 7, 8, 9, 63, 64, 65, 200, 256, 257):
        keep = rng.random((37, width)) < 0.5
        rec = dc.encode_record(keep)
        assert rec.shape == (37, dc.mask_words(width)) and (dc.decode_record(rec, width) == keep).all()
    assert dc.mask_words(200) == 8 and dc.mask_words(64) == 2 and dc.mask_words(65) == 4
    c0 = int(np.flatnonzero(dc.encode_record(np.eye(1, 200, 77, dtype=bool))[0])[0])    # the header's formula, spelled out
    assert c0 == ((77 // 4) & 1) * 4 + 77 // 64
    assert dc.encode_record(np.eye(1, 200, 77, dtype=bool))[0, c0] == 1 << (4 * ((77 // 8) % 8) + (77 & 3))
    for c in (dc.make_case("nn", "hashed", 33, 7, 33, "odd"), dc.make_case("nt", "colsum_hashed", 129, 64, 200, "pad"),
              dc.make_case("tn", "recorded", 127, 9, 5, "tight"), dc.make_case("nt", "colsum", 0, 8, 4, "tight")):
        r = dc.reference(c)
        a, b = r["a"].astype(np.float64), r["b"].astype(np.float64)
        assert np.abs(a).max(initial=0) <= c.amax and np.abs(b).max(initial=0) <= c.amax
        if a.size:
            assert a.any(0).all() and a.any(1).all()                   # no all-zero row or column
            if min(a.shape) >= 5:
                assert not np.array_equal(a[:5, :5], a[:5, :5].T)      # asymmetric
        assert b.any(0).all() and b.any(1).all()
        s = dc.scale_of(c.p)
        if c.family == "nn":                         # the reference again, element by element in int64
            want = (np.where(r["keep"], a, 0).astype(np.int64) @ b.astype(np.int64)) * int(s)
        elif c.family == "nt":
            want = a.astype(np.int64) @ b.astype(np.int64).T
            if c.p is not None:
                want = np.where(r["keep"], want, 0) * int(s)
        else:
            want = (np.where(r["keep"], a, 0).astype(np.int64).T @ b.astype(np.int64)) * int(s)
        assert np.array_equal(r["c"].astype(np.int64), want)
        if r["colsum"] is not None:
            assert np.array_equal(r["colsum"].astype(np.int64), want.sum(0))
    assert 0.3 < dc.reference(dc.make_case("nn", "hashed", 1025, 64, 33, "pad"))["keep"].mean() < 0.7
