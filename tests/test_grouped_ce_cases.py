"""The case list of the grouped cross-entropy sweep (tests/_grouped_ce_cases.py) on the CPU: every one of the eleven leaves
of `tgcn_grouped_ce` with every segment layout and output combination, both sides of every column-count boundary, each
cause of the scalar leaf on its own, one case above and one at the launch cap, the group edges -- so that thinning the list
later fails here, without a GPU.  And the bars themselves: the fp32 restatement of the arithmetic the kernel is meant to use
meets them on every case, so a kernel that misses one is wrong, not unlucky."""
import numpy as np
import torch

import _grouped_ce_cases as gc
import _perlabel_ref as R

TOL = 1e-5                                       # tests/test_gpu_parity.py's TOL, restated: that module loads the library
DBIAS_TOL = 2e-5                                 # the bias gradient's bound in tests/test_gpu_train_kernels.py


def test_the_restated_launcher_choices():
    assert [gc.gce_lanes(C) for C in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert [gc.gce_rows_per_block(C) for C in (16, 32, 64, 128, 256, 257, 300)] == [128, 64, 32, 16, 8, 8, 8]
    assert gc.gce_grid(16, 0) == 1 and gc.gce_grid(16, 128) == 1 and gc.gce_grid(16, 129) == 2
    assert gc.gce_grid(16, 131_072) == 1024 and gc.gce_grid(16, 131_073) == 1024 and gc.gce_grid(300, 8_193) == 1024
    assert gc.gce_v4(64, 64, 68, 0, 0, True) and not gc.gce_v4(64, 65, 64, 0, 0, True) and not gc.gce_v4(64, 64, 67, 0, 0, True)
    assert gc.gce_v4(64, 64, 67, 0, 1, False) and not gc.gce_v4(64, 64, 64, 1, 0, False) and not gc.gce_v4(63, 64, 64, 0, 0, False)
    assert not gc.gce_v4(64, 64, 64, 0, 1, True) and not gc.gce_v4(260, 260, 260, 0, 0, True)
    assert len(gc.LEAVES) == 11 and len(set(gc.LEAVES)) == 11
    for lo, hi in gc.GCE_EDGES:
        assert (gc.gce_lanes(lo), lo <= 256) != (gc.gce_lanes(hi), hi <= 256)


def test_the_segment_layouts():
    for C in sorted({c.C for c in gc.all_cases()}):
        for seg in gc.SEG_LAYOUTS:
            starts, widths = gc.segments(C, seg)
            assert len(starts) <= gc.GCE_MAX_GROUPS
        s, w = (np.asarray(v) for v in gc.segments(C, "packed"))
        assert s[0] == 0 and (s[1:] == (s + w)[:-1]).all() and s[-1] + w[-1] == C           # back to back, no pad column
        if C >= 16:
            assert (s % 4 != 0).any() and ((s % 4) + w > 4).any()                          # off a lane's float4, and across one
            assert 1 in w
        s, w = (np.asarray(v) for v in gc.segments(C, "gaps"))
        if C >= 16:
            assert (s % 4 == 0).all() and (s[1:] > (s + w)[:-1]).any()
        s, w = gc.segments(C, "one")
        assert 1 in w and sum(w) == C
        assert gc.segments(C, "full") == ((0,), (C,))
    assert max(gc.segments(300, "packed")[1]) == 70 and max(gc.segments(257, "packed")[1]) == 70     # more than one pass of 64 lanes
    assert gc.segments(128, "ones") == (tuple(range(128)), (1,) * 128) and len(gc.segments(16, "ones")[0]) == 16
    assert len(gc.segments(300, "ones_spread")[0]) == 128 and len(gc.segments(300, "alt13")[0]) == 128


def test_every_leaf_layout_output_boundary_and_launch_cap_is_in_the_list():
    cases = gc.all_cases()
    assert len({gc.case_id(c) for c in cases}) == len(cases)
    groups = gc.by_leaf(cases)
    assert set(groups) == set(gc.LEAVES)
    assert sorted(c for g in groups.values() for c in g) == sorted(cases)
    for leaf, mine in groups.items():
        lpr, v4 = leaf
        regs = lpr != gc.WIDE
        small = [c for c in mine if c.n == gc.N_SMALL]
        for c in mine:
            assert (c.C <= 256) == regs and (not regs or gc.gce_lanes(c.C) == lpr) and gc.case_is_v4(c) == v4
        # the four segment layouts, each with every output combination
        for seg in gc.SEG_LAYOUTS:
            assert {(c.out, c.pred, c.route, c.cmap) for c in small if c.seg == seg and c.values == "randn"} == \
                {(o,) + combo for o in gc.OUTPUTS for combo in gc.PRED_COMBOS}, (leaf, seg)
        # a gradient with ldd > n_cols and with ldd == n_cols on every leaf
        assert any(c.out != "loss" and c.pad2 > 0 for c in mine) and any(c.out != "loss" and c.pad2 == 0 for c in mine), leaf
        if v4:
            assert {(c.pad, c.pad2) for c in mine} >= {(0, 0), (4, 4), (0, 4), (4, 0)}, leaf
        elif regs:
            # each cause of the scalar leaf on its own; the two of the gradient only when there is one
            causes = {gc.scalar_causes(c.C, c.C + c.pad, c.C + c.pad2, c.off, c.offd, c.out != "loss") for c in mine}
            for cause in ("n_cols", "ld", "base", "ldd", "dbase"):
                assert frozenset([cause]) in causes, (leaf, cause)
            assert all(causes), leaf
            for c in mine:
                if c.out == "loss":
                    assert gc.scalar_causes(c.C, c.C + c.pad, c.C + c.pad2, c.off, c.offd, False), c
        else:
            assert any(c.C % 4 == 0 and c.pad == c.pad2 == c.off == c.offd == 0 for c in mine)     # wide whatever the layout
            assert any(c.C % 4 for c in mine) and any(c.off % 4 for c in mine)
        # the launch cap: one case above 1024 * rows_per_block rows, one exactly at it, one with several workgroups below it
        rpb = gc.gce_rows_per_block(mine[0].C)
        assert all(gc.gce_rows_per_block(c.C) == rpb for c in mine)
        cap = gc.GCE_BLOCKS * rpb
        assert any(c.n == cap + 1 and c.out == "dbias" and c.values == "randn" for c in mine), leaf
        assert any(c.n == cap + 1 and c.out == "grad" and c.values == "onehot" for c in mine), leaf
        assert any(c.n == cap for c in mine) and max(c.n for c in mine) == cap + 1, leaf
        assert any(c.n < cap and gc.gce_grid(c.C, c.n) > 1 for c in mine), leaf
        # every value edge, at one small n
        assert {c.values for c in small} == set(gc.VALUES), leaf
    assert max(c.n for c in cases) == 131_073 and max(c.n for c in groups[(gc.WIDE, False)]) == 8_193
    assert max(c.n * (c.C + c.pad) for c in cases) <= 131_073 * 20
    widths = {c.C for c in cases}
    for lo, hi in gc.GCE_EDGES:                                                     # both sides of every boundary
        assert lo in widths and hi in widths, (lo, hi)
        assert lo in {c.C for c in cases if gc.case_is_v4(c)} and lo in {c.C for c in cases if not gc.case_is_v4(c)}
    for leaf, mine in groups.items():                                               # ... seen from every leaf
        cs = {c.C for c in mine}
        lows = {(4, True): 4, (4, False): 1, (8, True): 20, (16, True): 36, (32, True): 68, (64, True): 132}
        lo = lows.get(leaf, {8: 17, 16: 33, 32: 65, 64: 129, gc.WIDE: 257}.get(leaf[0]))
        hi = {4: 16, 8: 32, 16: 64, 32: 128, 64: 256}.get(leaf[0])
        assert lo in cs and (hi is None or hi in cs), leaf
    # the group edges: K = 128 width-1 segments at 128 columns on both lpr-32 leaves and on the wide one, K = 16 at 16
    for C, seg, leaves in ((128, "ones", {(32, True), (32, False)}), (16, "ones", {(4, True), (4, False)}),
                           (300, "ones_spread", {(gc.WIDE, False)}), (300, "alt13", {(gc.WIDE, False)})):
        assert {gc.leaf_of(c) for c in cases if c.C == C and c.seg == seg} == leaves
        assert {c.out for c in cases if c.C == C and c.seg == seg} == set(gc.OUTPUTS)
    assert len(gc.segments(128, "ones")[0]) == gc.GCE_MAX_GROUPS


def test_the_inputs_hold_what_the_cases_are_named_for():
    for c in gc.edge_cases() + tuple(c for c in gc.small_cases() if c.n == gc.N_SMALL and c.seg in gc.SEG_LAYOUTS)[::15]:
        i, ref = gc.gce_inputs(c.C, c.n, c.seg, c.values), gc.gce_reference(c.C, c.n, c.seg, c.values)
        x, mask, g, t = i["x"], i["mask"], i["group"], i["target"]
        K = len(i["starts"])
        sel = gc.selected_rows(i)
        assert x.shape == (c.n, c.C) and sel.any()
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all() and np.isfinite(ref["dbias"]).all(), c
        fin = ~np.isnan(ref["loss_k"])
        assert np.array_equal(fin, i["inv_count"] != 0)
        if c.values not in ("onehot", "onemask"):
            # selected rows of the groups K, -1 and -5; a group with rows but none selected; routes out of range
            assert {K, -1, -5} <= set(g[mask].tolist()), c
            assert {K, -1, -5} <= set(i["route"].tolist()) and (i["route"] != g).any(), c
            if K >= 2:
                assert (g == K // 2).any() and not fin[K // 2] and not mask[g == K // 2].any()
        assert (ref["grad"][~sel] == 0).all() and (ref["dbias"][~gc.trained_columns(i)] == 0).all()
        rowmax = np.abs(ref["grad"][sel]).max(1)
        tiny = (rowmax > 0) & (rowmax < gc.TINY_ROW)
        if c.values in ("x80", "x1e4"):
            assert tiny.mean() < 0.25, c
        else:
            assert not tiny.any(), c
        own = gc.own_columns(i, True, True)
        assert not own.all() or c.seg == "full" or c.C <= 2
        if c.values == "nanrow":
            assert np.isnan(x[1::4]).all() and not np.isnan(x[0::4]).any() and not mask[1::4].any()
            for key, p in ref["pred"].items():
                ids = (i["route"] if key[0] else g)[1::4]
                ok = (ids >= 0) & (ids < K)
                first = i["starts"][np.where(ok, ids, 0)]
                assert (p[1::4][ok] == (i["class_map"][first] if key[1] else first)[ok]).all() and (p[1::4][~ok] == -1).all()
        elif c.values != "neginf":
            assert np.isfinite(x).all()
        if c.values == "neginf":
            v = (g >= 0) & (g < K)
            assert np.isfinite(x[np.flatnonzero(v), (i["starts"][g[v]] + t[v])]).all() and 0.2 < np.isinf(x).mean() < 0.45
        if c.values == "onemask":
            assert sel.sum() == 1 and fin.sum() == 1 and i["inv_count"].max() == 1.0
        if c.values == "equal":
            assert (x == x[:, :1]).all() and len(np.unique(x[:, 0])) == 5
        if c.values == "argmax":
            k = int(g[sel][0])
            s, w = int(i["starts"][k]), int(i["widths"][k])
            r = np.flatnonzero(sel)[0]
            assert t[r] == x[r, s:s + w].argmax()
        if c.values == "onehot":
            assert mask.all() and (ref["pred"][True, False] == i["starts"][g] + (np.arange(c.n) // K) % i["widths"][g]).all()
            assert ref["loss_k"][i["widths"] > 1].min() > 1.0
        if c.values == "ties":
            seen = [0, 0, 0]
            for s, w in zip(i["starts"], i["widths"]):
                for cls, pair in enumerate(gc.tie_pairs(c.C, int(s), int(w))):
                    if pair is None:
                        continue
                    rows = np.arange(cls, c.n, 4)
                    seg = x[rows, s:s + w]
                    assert (seg[:, pair[0] - s] == seg.max(1)).all() and (seg[:, pair[1] - s] == seg.max(1)).all()
                    seen[cls] += 1
            assert all(seen), (c, seen)                  # first / last, a float4 hand-over and a lane-stride hand-over
    # the one-hot rows of the grid-stride cases name themselves
    c = gc.stride_cases()[1]
    i, ref = gc.gce_inputs(c.C, c.n, c.seg, c.values), gc.gce_reference(c.C, c.n, c.seg, c.values)
    K = len(i["starts"])
    assert c.values == "onehot" and (ref["pred"][False, False] == i["starts"][i["group"]] + (np.arange(c.n) // K) % i["widths"][i["group"]]).all()


def test_the_fp32_restatement_meets_the_bars_on_every_case():
    """the arithmetic of csrc/masked_ce.h, evaluated in numpy's float32 over the inputs of every case, against float64: the
    bars the GPU test holds the kernel to are reachable by the formulation alone"""
    worst = {}
    outs = {}
    for c in gc.all_cases():                         # (an input is held to the outputs that a case asks of it)
        outs.setdefault((c.C, c.n, c.seg, c.values), set()).add(c.out)
    keys = sorted(outs)
    for key in keys:
        i, ref = gc.gce_inputs(*key), gc.gce_reference(*key)
        got = gc.grouped_ce_of(i["x"], i["target"], i["mask"], i["group"], i["starts"], i["widths"], i["inv_count"], dtype=np.float32)
        assert got["grad"].dtype == np.float32 and got["loss_k"].dtype == np.float32
        got["dbias"] = gc.blocked_sum(got["grad"])
        if "dbias" not in outs[key]:
            del got["dbias"]
        if outs[key] == {"loss"}:
            del got["grad"]
        errs = gc.errors(got, ref, i)
        for k, v in errs.items():
            if v > worst.get(k, (0.0, None))[0]:
                worst[k] = (v, key)
        assert errs["loss"] < TOL and errs["loss_k"] < TOL and errs.get("row", 0) < TOL and errs.get("dbias", 0) < DBIAS_TOL, (key, errs)
    print(f"\nfp32 restatement over {len(keys)} inputs, worst: " + ", ".join(f"{k} {v[0]:.2e} at {v[1]}" for k, v in worst.items()))


def test_the_reference_against_separate_torch_losses():
    c = gc.GceCase(33, gc.N_SMALL, "packed", 0, 0, 0, 0, "dbias", True, True, True, "randn")
    i, ref = gc.gce_inputs(c.C, c.n, c.seg, c.values), gc.gce_reference(c.C, c.n, c.seg, c.values)
    K = len(i["starts"])
    t = lambda a: torch.from_numpy(np.array(a))
    starts, widths = [int(v) for v in i["starts"]], [int(v) for v in i["widths"]]
    target = np.where(gc.selected_rows(i), i["target"], 0)
    loss_k, grad = R.separate_ce(t(i["x"]), t(target), t(i["mask"]), t(i["group"]), starts, widths)
    fin = ~np.isnan(ref["loss_k"])
    assert np.array_equal(torch.isnan(loss_k).numpy(), ~fin) and K > 4
    # (inv_count is 1 / count rounded to fp32: the two differ by that rounding)
    assert (np.abs(loss_k.numpy()[fin] - ref["loss_k"][fin]) <= 1e-7 * np.abs(ref["loss_k"][fin])).all()
    assert np.abs(grad.numpy() - ref["grad"]).max() < 1e-7 * np.abs(ref["grad"]).max()
    want = R.routed_pred(t(i["x"]), t(i["route"]), starts, widths, t(i["class_map"]))
    assert np.array_equal(want.numpy(), ref["pred"][True, True])
