#!/usr/bin/env python3
"""Interleaved timing of the whole grid of one graph of old/h_o_train.py's sweep (2 dropout values x 4 learning rates x
KFold(3) = 24 two-layer GCNs) in three forms, in one process:

    (a) fused       ONE 24-member `CrossValGCN` with a dropout rate per member and `enable_fused_block_diag()`: the three
                    layer-2 products are one launch each for all members (tgcn_blockdiag_xw, tgcn_blockdiag_xw_grad)
    (b) k-launch    the same network with the layer-2 products on the K-launch path (72 launches per step)
    (c) per-dropout TWO 12-member networks, one per dropout value, trained one after the other: what the package offered
                    before a rate per member -- the comparison with before is (a) against (c)

Settings: dropouts [0.5, 0.7] x rates [0.001, 0.005, 0.01, 0.05] x 3 folds, hidden width 100, 8 classes, fused dropout on
in every form.  Shapes: config c2 of bench.py (100 000 nodes / 2 M edges) and a `synth` word-document graph of real-corpus
size (60 000 nodes / 6 M edges).  The train step (forward, loss, backward, optimizer step, all 24 members) and the eval
forward with validation losses and predictions (all 24) are timed with HIP events after a warm-up round; several rounds with
the forms alternating, so that clock and temperature drift hits all alike.  Reported: the median and the spread (max - min)
of the repetitions, and the peak memory a call allocates on top of what is live before it.  Verdict by the project's rule: a
form is faster or slower than another only if the medians differ by more than the SUM of the two spreads.  Before timing,
the eval logits of form (a) are compared with those of forms (b) and (c).

    timeout 900 python tools/ab_crossval_grid.py [--shapes c2 corpus] [--rounds 5] [--reps 5] [--log profiles/r16_ab_crossval_grid.log]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import perlabel, synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits, grid_members  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
DOS, LRS, N_FOLDS, N_CLASSES = [0.5, 0.7], [0.001, 0.005, 0.01, 0.05], 3, 8

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r16_ab_crossval_grid.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
h, C = args.hidden, N_CLASSES
member_lrs, member_dos = grid_members(LRS, DOS, N_FOLDS)
K, K1 = len(member_lrs), len(LRS) * N_FOLDS
log = open(args.log, "w")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def verdict(a, b):
    """(median, spread) of two forms -> what may be said about a against b"""
    if abs(a[0] - b[0]) <= a[1] + b[1]:
        return "no difference (the medians differ by less than the sum of the spreads)"
    return f"{'faster' if a[0] < b[0] else 'slower'} ({b[0] / a[0]:.2f} x)"


pkg.enable_fused_dropout()
say(f"ab_crossval_grid: {torch.cuda.get_device_name(0)}; K={K} ({len(DOS)} dropouts x {len(LRS)} rates x {N_FOLDS} folds) "
    f"hidden={h} classes={C} fused dropout on; 1 warm-up round, then {args.rounds} rounds x {args.reps} timed repetitions, "
    "forms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    g = synth.word_doc_graph(N, E, seed=44, n_classes=C)
    doc_rows = np.arange(g.n_vocab, N)
    order = np.random.default_rng(44).permutation(doc_rows.size)
    folds = [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)]
    train_bits, val_bits = fold_bits(doc_rows, folds, N, n_repeats=len(DOS) * len(LRS))
    train_half, val_half = fold_bits(doc_rows, folds, N, n_repeats=len(LRS))
    g = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(dev)
    train_bits, val_bits, train_half, val_half = (t.to(dev) for t in (train_bits, val_bits, train_half, val_half))
    target = g.y.long()
    torch.manual_seed(0)
    members = [pkg.GCN(N, C, n_hidden_gcn=h, dropout=p).to(dev).float() for p in member_dos]
    nets = {"fused": CrossValGCN.from_members(members), "k-launch": CrossValGCN.from_members(members)}
    assert nets["fused"].dropout == tuple(member_dos)
    halves = [CrossValGCN.from_members(members[d * K1:(d + 1) * K1]) for d in range(len(DOS))]
    assert [n_.dropout for n_ in halves] == DOS
    opts = {name: MemberAdam(n_, member_lrs) for name, n_ in nets.items()}
    opt_halves = [MemberAdam(n_, member_lrs[:K1]) for n_ in halves]
    S = nets["fused"].seg_stride

    def with_switch(on, fn):
        was = perlabel.enable_fused_block_diag(on)
        try:
            return fn()
        finally:
            perlabel.enable_fused_block_diag(was)

    with torch.no_grad():                                   # the same function, before anything is timed
        z = with_switch(True, lambda: nets["fused"].eval()(g))
        zb = with_switch(False, lambda: nets["k-launch"].eval()(g))
        zc = torch.cat([with_switch(False, lambda n_=n_: n_.eval()(g)) for n_ in halves], 1)
        err_b = float((z - zb).abs().max() / zb.abs().max())
        err_c = float((z - zc).abs().max() / zc.abs().max())
        del z, zb, zc
    say(f"{shape}: N={N} edges={E}; eval logits of (a) against (b): max|a - b| / max|b| = {err_b:.2e}, against (c): {err_c:.2e}")

    def train_net(name):
        net, opt = nets[name], opts[name]
        net.train()
        loss, _ = net.loss(g, target, train_bits)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    def train_halves():
        for net, opt in zip(halves, opt_halves):
            net.train()
            loss, _ = net.loss(g, target, train_half)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    forms = {"(a) fused": (True, lambda: train_net("fused"), lambda: nets["fused"].evaluate(g, target, val_bits)),
             "(b) k-launch": (False, lambda: train_net("k-launch"), lambda: nets["k-launch"].evaluate(g, target, val_bits)),
             "(c) per-dropout": (False, train_halves, lambda: [n_.evaluate(g, target, val_half) for n_ in halves])}
    cases = [(name, form, on, fns[i]) for i, name in enumerate(("train step", "eval + pred"))
             for form, (on, *fns) in forms.items()]
    times = {(name, form): [] for name, form, _, _ in cases}
    peak = {}
    for rnd in range(args.rounds + 1):                      # round 0 = warm-up (plans, layouts, restricted operators, allocator)
        for name, form, on, fn in cases:
            was = perlabel.enable_fused_block_diag(on)
            fn()
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            perlabel.enable_fused_block_diag(was)
            if rnd:
                times[(name, form)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
                peak[(name, form)] = max(peak.get((name, form), 0), torch.cuda.max_memory_allocated() - before)
    res = {}
    for (name, form), ts in times.items():
        ts = sorted(ts)
        res[(name, form)] = (ts[len(ts) // 2], ts[-1] - ts[0])
        say(f"  {name:12s} {form:16s} median {res[(name, form)][0]:9.3f} ms   min {ts[0]:9.3f}   max {ts[-1]:9.3f}   spread "
            f"(max - min) {ts[-1] - ts[0]:8.3f} ms   peak extra memory {peak[(name, form)] / 2 ** 20:9.1f} MiB")
    for name in ("train step", "eval + pred"):
        for other in ("(b) k-launch", "(c) per-dropout"):
            say(f"  {shape} {name}: (a) fused against {other}: {verdict(res[(name, '(a) fused')], res[(name, other)])}")
    del nets, halves, members, opts, opt_halves, g
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
