"""The case lists of the training-kernel sweep (tests/_train_cases.py) on the CPU: every leaf of the masked cross-entropy
with every output combination, both sides of every class-count boundary, one case above and one at or below every launch
cap, the Adam grid and the scale sizes -- so that thinning the lists later fails here, without a GPU.  And the inputs of
the value edges: the float64 reference is finite where it must be, so that no edge can be "passed" by NaN on both sides."""
import numpy as np

import _train_cases as tc


def test_the_restated_launcher_choices():
    assert [tc.ce_leaf(C, False) for C in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300)] == [
        (4, 4, True, 128), (4, 4, True, 128), (4, 8, True, 128), (4, 8, True, 128), (8, 8, True, 64), (8, 8, True, 64),
        (16, 8, True, 32), (16, 8, True, 32), (32, 8, True, 16), (32, 8, True, 16), (64, 4, False, 8), (64, 4, False, 8)]
    for lo, hi in tc.CE_EDGES:
        assert tc.ce_leaf(lo, False)[:2] != tc.ce_leaf(hi, False)[:2]
    assert tc.ce_v4(64, 64, 68, 0, 0, True) and not tc.ce_v4(64, 65, 64, 0, 0, True) and not tc.ce_v4(64, 64, 67, 0, 0, True)
    assert tc.ce_v4(64, 64, 67, 0, 1, False) and not tc.ce_v4(64, 64, 64, 1, 0, False) and not tc.ce_v4(63, 64, 64, 0, 0, False)
    assert not tc.ce_v4(64, 64, 64, 0, 1, True)
    assert tc.ce_grid(16, 0) == 1 and tc.ce_grid(16, 128) == 1 and tc.ce_grid(16, 129) == 2 and tc.ce_grid(300, 10 ** 6) == 2048
    assert tc.adam_leaf(1, True) == (False, 1) and tc.adam_leaf(1024, False) == (False, 2)
    assert tc.adam_leaf(tc.ADAM_CAP - 4, True) == (False, 8192) and tc.adam_leaf(1 << 24, True) == (True, 8192)
    assert tc.adam_leaf((1 << 24) - 1, True)[0] is False
    assert tc.ADAM_CAP == 8_388_608 and tc.SCALE_CAP == 1_048_576


def test_every_ce_leaf_output_boundary_and_launch_cap_is_in_the_list():
    cases = tc.all_ce_cases()
    assert len({tc.ce_case_id(c) for c in cases}) == len(cases)
    groups = tc.by_leaf(cases)
    assert set(groups) == set(tc.LEAVES) and len(tc.LEAVES) == 12
    assert sorted(c for g in groups.values() for c in g) == sorted(cases)          # grouping loses and repeats nothing
    for leaf, mine in groups.items():
        lpr, kpl, v4 = leaf
        for c in mine:
            assert tc.ce_leaf(c.C, v4)[:2] == (lpr, kpl) and tc.case_is_v4(c) == v4
        # the three outputs, each with and without the arg-max
        assert {(c.out, c.pred) for c in mine} == {(o, p) for o in tc.OUTPUTS for p in (False, True)}, leaf
        # a gradient with ldd > C on every leaf: "padding columns are never written" for both kinds of store
        assert any(c.out != "loss" and c.pad2 > 0 for c in mine), leaf
        assert any(c.out != "loss" and c.pad2 == 0 for c in mine), leaf
        if v4:
            assert {(c.pad, c.pad2) for c in mine} >= {(0, 0), (4, 4), (0, 4), (4, 0)}, leaf
        else:
            # forced by an odd leading dimension and by the base pointer alone, at widths that are multiples of 4 too
            assert any(c.C % 4 == 0 and c.pad % 2 and c.off == 0 for c in mine), leaf
            assert any(c.C % 4 == 0 and c.off % 4 and c.pad % 4 == 0 for c in mine), leaf
            assert any(c.C % 4 == 0 and c.offd % 4 and c.off == 0 and c.pad2 % 4 == 0 and c.out != "loss" for c in mine), leaf
            assert any(c.C % 4 for c in mine), leaf
        # the launch cap: one case above 2048 * rows_per_block rows, one at or below it
        rpb = tc.ce_leaf(mine[0].C, v4)[3]
        assert all(tc.ce_leaf(c.C, v4)[3] == rpb for c in mine)
        assert any(c.n > tc.CE_BLOCKS * rpb and c.out != "loss" and c.values == "randn" for c in mine), leaf
        assert any(c.n > tc.CE_BLOCKS * rpb and c.values == "onehot" for c in mine), leaf
        assert any(c.n == tc.CE_BLOCKS * rpb + 1 for c in mine) and any(c.n == tc.CE_BLOCKS * rpb for c in mine), leaf
        assert any(c.n <= tc.CE_BLOCKS * rpb and tc.ce_grid(c.C, c.n) > 1 for c in mine), leaf
        # every value edge, at one small n
        assert {c.values for c in mine if c.n == tc.N_SMALL} >= set(tc.EDGE_VALUES) | {"randn"}, leaf
    assert max(c.n * (c.C + c.pad) for c in cases) <= 262_145 * 36
    widths = {c.C for c in cases}
    for lo, hi in tc.CE_EDGES:                                                      # both sides of every boundary
        assert lo in widths and hi in widths, (lo, hi)
        assert lo in {c.C for c in cases if tc.case_is_v4(c)} and lo in {c.C for c in cases if not tc.case_is_v4(c)}
    assert {257, 258, 259} <= widths                                                # a little more than four passes of 64 lanes
    assert tc.EDGE_VALUES == ("at+80", "at-80", "at+1e4", "at-1e4", "x80", "x1e4", "neginf", "equal", "onemask", "ties")


def test_the_adam_grid_and_the_scale_sizes():
    cases = tc.all_adam_cases()
    assert len({tc.adam_case_id(c) for c in cases}) == len(cases)
    ns = {c.n for c in cases}
    assert ns >= {1, 2, 3, 5, 6, 7, 1023, 1024, 1025, 8_388_604, 8_388_612, 8_388_608 + 1024 * 3 + 1}
    for n in tc.ADAM_SMALL_N:                                                       # the whole grid at every small size
        assert {(c.amsgrad, c.wd, c.beta1) for c in cases if c.n == n} == {(a, w, b) for a in (True, False)
                                                                            for w in (0.0, 0.01) for b in (0.9, 0.5, 0.3)}
    big = tc.adam_big_cases()
    assert {(c.amsgrad, c.wd > 0) for c in big} == {(a, w) for a in (True, False) for w in (True, False)}
    assert {c.beta1 for c in big} == {0.9, 0.5, 0.3}
    # both sides of the launch cap, on the plain leaf; the second stride with a float4 body and with a scalar tail
    assert any(not tc.adam_second_stride(c.n) and tc.adam_leaf(c.n, c.amsgrad) == (False, 8192) for c in big)
    over = [c for c in big if tc.adam_second_stride(c.n)]
    assert over and all(tc.adam_leaf(c.n, c.amsgrad) == (False, 8192) for c in over)
    assert any((c.n - tc.ADAM_CAP) % 4 == 0 for c in over) and any((c.n - tc.ADAM_CAP) % 4 for c in over)
    assert any(c.n - tc.ADAM_CAP > 2 * tc.ADAM_PER_BLOCK for c in over)
    # both sides of 2^24: the streaming leaf keeps its own test
    assert all(c.n < tc.ADAM_NT for c in cases) and tc.adam_leaf(tc.ADAM_NT_TESTED_ELSEWHERE, True)[0]
    assert tc.adam_second_stride(tc.ADAM_NT_TESTED_ELSEWHERE)
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py")) as f:
        assert "n = (1 << 24) + 5" in f.read().split("def test_fused_adam_streaming_path_for_large_tensors")[1][:400]
    # beta1 on both sides of the lerp branch, and 0.5 ON it: w1 = float(1 - 0.5) = 0.5f is not below 0.5f
    assert [tc.lerp_branch(b) for b in (0.9, 0.5, 0.3)] == ["low", "high", "high"]
    assert {tc.lerp_branch(c.beta1) for c in cases} == {"low", "high"} and any(c.beta1 == 0.5 for c in cases)
    # sizes without a float4 body, sizes with a body and a tail
    assert {n for n in ns if n < 4} == {1, 2, 3} and {5, 6, 7} <= ns
    assert tc.SCALE_N == (1, 255, 256, 257, 1_048_576, 1_048_577 + 256) and tc.SCALES == (2.5, 0.0)
    assert any(n > tc.SCALE_CAP for n in tc.SCALE_N) and any(1 < n <= tc.SCALE_CAP for n in tc.SCALE_N)


def test_the_value_edges_have_a_finite_reference_and_the_ties_sit_where_the_column_maps_differ():
    for c in tc.edge_cases():
        i, ref = tc.ce_inputs(c.C, c.n, c.values), tc.ce_reference(c.C, c.n, c.values)
        x, mask, t = i["x"], i["mask"], i["target"]
        assert x.shape == (tc.N_SMALL, c.C) and mask.any() and not np.isnan(x).any()
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all() and np.isfinite(ref["dbias"]).all(), c
        assert np.isfinite(x[np.arange(c.n), t]).all()                             # -inf never at the target
        rowmax = np.abs(ref["grad"][mask]).max(1)
        tiny = (rowmax > 0) & (rowmax < tc.TINY_ROW)
        if c.values in ("x80", "x1e4"):
            assert np.abs(x).max(1).min() == np.abs(x).max() == float(c.values[1:])
            assert tiny.mean() < 0.25, c                                           # most rows are held to their own scale
        else:
            assert not tiny.any(), c
        if c.values.startswith("at"):
            assert abs(np.median(x) - float(c.values[2:])) < 1.0
        if c.values == "neginf":
            assert 0.2 < np.isinf(x).mean() < 0.4 or c.C < 8
        if c.values == "equal":
            assert (x == x[:, :1]).all() and len(np.unique(x[:, 0])) == 5
            assert (ref["pred"] == 0).all()
        if c.values == "onemask":
            assert mask.sum() == 1 and i["inv_count"] == 1.0
        if c.values == "ties":
            lpr, kpl, _, _ = tc.ce_leaf(c.C, False)
            pairs = tc.tie_pairs(c.C)
            assert set(pairs) == {(0, c.C - 1), (lpr - 1, lpr), (kpl - 1, kpl)}
            for a, b in pairs:
                rows = (x[:, a] == x.max(1)) & (x[:, b] == x.max(1)) & ((x == x.max(1, keepdims=True)).sum(1) == 2)
                assert rows.sum() > 10 and (ref["pred"][rows] == a).all()
    # the one-hot rows of the grid-stride cases: every row names itself in its arg-max, and the loss is well away from 0
    for c in tc.stride_cases()[1:6:3]:
        i, ref = tc.ce_inputs(c.C, c.n, c.values), tc.ce_reference(c.C, c.n, c.values)
        assert (ref["pred"] == np.arange(c.n) % c.C).all() and i["mask"].all() and ref["loss"] > 30.0
        assert (i["target"] == ref["pred"]).any() and (i["target"] != ref["pred"]).any()


def test_the_references_against_a_second_formulation():
    import torch
    c = tc.CeCase(20, 37, 0, 0, 0, 0, "dbias", True, "randn")
    i, ref = tc.ce_inputs(c.C, c.n, c.values), tc.ce_reference(c.C, c.n, c.values)
    x = torch.from_numpy(i["x"].copy()).double().requires_grad_()
    m, t = torch.from_numpy(i["mask"].copy()), torch.from_numpy(i["target"].copy())
    loss = torch.nn.functional.cross_entropy(x[m], t[m], reduction="sum") * i["inv_count"]
    loss.backward()
    assert abs(loss.item() - ref["loss"]) < 1e-12 * abs(ref["loss"])
    assert np.abs(x.grad.numpy() - ref["grad"]).max() < 1e-15
    assert (ref["pred"] == i["x"].argmax(1)).all()
    for b1 in tc.ADAM_BETA1:
        a = tc.AdamCase(1025, True, 0.01, b1)
        p, mm, v, vmax, grads = tc.adam_inputs(a)
        assert (v >= 0).all() and (vmax >= 0).all() and (vmax > v).any() and (vmax < v).any()
        want = tc.adam_reference(a, p, mm, v, vmax, grads)
        tp = torch.from_numpy(p.copy()).double().requires_grad_()
        opt = torch.optim.Adam([tp], lr=tc.ADAM_LR, betas=(b1, tc.ADAM_BETA2), eps=tc.ADAM_EPS, weight_decay=a.wd, amsgrad=True)
        tp.grad = torch.zeros_like(tp)
        opt.step()                                     # creates the state; overwritten below, the step count rewound
        st = opt.state[tp]
        with torch.no_grad():
            tp.copy_(torch.from_numpy(p.copy()).double())
            st["exp_avg"].copy_(torch.from_numpy(mm.copy()).double())
            st["exp_avg_sq"].copy_(torch.from_numpy(v.copy()).double())
            st["max_exp_avg_sq"].copy_(torch.from_numpy(vmax.copy()).double())
            st["step"] = torch.zeros_like(st["step"]) if torch.is_tensor(st["step"]) else 0
        for g in grads:
            tp.grad = torch.from_numpy(g.copy()).double()
            opt.step()
        assert np.abs(tp.detach().numpy() - want[0]).max() < 1e-13
        assert np.abs(st["max_exp_avg_sq"].numpy() - want[3]).max() < 1e-13
    s1, s2 = tc.adam_scalars(1)
    assert s1 == np.float32(1e-3 / (1.0 - 0.9)) and s2 == np.float32(1.0 / np.sqrt(1.0 - 0.999))
