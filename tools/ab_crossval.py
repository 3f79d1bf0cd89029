#!/usr/bin/env python3
"""Interleaved timing of one cell of old/h_o_train.py's sweep (4 learning rates x KFold(3) = 12 two-layer GCNs on one graph)
in three forms, in one process:

    one network   `CrossValGCN` + `member_masked_cross_entropy` (tgcn_member_ce) + `MemberAdam` (tgcn_adam_members)
    sequential    12 `GCN`s one after the other, each on the fused `masked_cross_entropy` and the fused `optim.Adam` --
                  what the sweep runs, on this package
    composed      the one network with its loss composed from 12 `masked_cross_entropy` calls on column slices of its logits
                  (what the network costs WITHOUT the member kernel; Adam is `MemberAdam` here too)

Settings: K = 12, hidden width 100, dropout 0.5 (torch's), 8 classes.  Shapes: config c2 of bench.py (100 000 nodes / 2 M
edges) and a `synth` word-document graph of real-corpus size (60 000 nodes / 6 M edges).  The train step (forward, loss,
backward, optimizer step, all 12 members) and the eval forward with validation losses and predictions (all 12) are timed
with HIP events after a warm-up round; several rounds with the forms alternating, so that clock and temperature drift hits
all alike.  Reported: the median and the spread (max - min) of the repetitions, and the peak memory a call allocates on top
of what is live before it.  Verdict by the project's rule: a form is faster or slower than another only if the medians differ
by more than the SUM of the two spreads.  Before timing, the eval logits of the network are compared with its members'.

    timeout 900 python tools/ab_crossval.py [--shapes c2 corpus] [--rounds 5] [--reps 5] [--log profiles/r15_ab_crossval.log]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import synth  # noqa: E402
from pytextgcn_amd.crossval import CrossValGCN, MemberAdam, fold_bits  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
LRS, N_FOLDS, N_CLASSES = [0.001, 0.005, 0.01, 0.05], 3, 8

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r15_ab_crossval.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
K, h, C = len(LRS) * N_FOLDS, args.hidden, N_CLASSES
member_lrs = [lr for lr in LRS for _ in range(N_FOLDS)]
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


say(f"ab_crossval: {torch.cuda.get_device_name(0)}; K={K} ({len(LRS)} rates x {N_FOLDS} folds) hidden={h} classes={C} "
    f"dropout={args.dropout}; 1 warm-up round, then {args.rounds} rounds x {args.reps} timed repetitions, forms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    g = synth.word_doc_graph(N, E, seed=44, n_classes=C)
    doc_rows = np.arange(g.n_vocab, N)
    order = np.random.default_rng(44).permutation(doc_rows.size)
    train_bits, val_bits = fold_bits(doc_rows, [np.sort(order[f::N_FOLDS]) for f in range(N_FOLDS)], N, n_repeats=len(LRS))
    g = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(dev)
    train_bits, val_bits, target = train_bits.to(dev), val_bits.to(dev), g.y.long()
    train_masks = [((train_bits >> k) & 1).bool() for k in range(K)]
    val_masks = [((val_bits >> k) & 1).bool() for k in range(K)]
    torch.manual_seed(0)
    members = [pkg.GCN(N, C, n_hidden_gcn=h, dropout=args.dropout).to(dev).float() for _ in range(K)]
    net = CrossValGCN.from_members(members)
    net2 = CrossValGCN.from_members(members)
    S = net.seg_stride
    opt_net, opt_net2 = MemberAdam(net, member_lrs), MemberAdam(net2, member_lrs)
    opt_members = [pkg.optim.Adam(m.parameters(), lr=lr) for m, lr in zip(members, member_lrs)]

    with torch.no_grad():                                   # the same function, before anything is timed
        z = net.eval()(g)
        worst = 0.0
        for k, m in enumerate(members):
            zk = m.eval()(g)
            worst = max(worst, float((z[:, k * S:k * S + C] - zk).abs().max() / zk.abs().max()))
        del z, zk
    say(f"{shape}: N={N} edges={E}; eval logits, the network against its members: max|a - b| / max|b| = {worst:.2e}")

    def train_one():
        net.train()
        loss, _ = net.loss(g, target, train_bits)
        opt_net.zero_grad(set_to_none=True)
        loss.backward()
        opt_net.step()

    def train_sequential():
        for m, opt, mask in zip(members, opt_members, train_masks):
            m.train()
            loss = masked_cross_entropy(m(g), target, mask)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    def train_composed():
        net2.train()
        z_ = net2(g)
        loss = sum(masked_cross_entropy(z_[:, k * S:k * S + C], target, train_masks[k]) for k in range(K))
        opt_net2.zero_grad(set_to_none=True)
        loss.backward()
        opt_net2.step()

    def eval_one():
        return net.evaluate(g, target, val_bits)

    def eval_sequential():
        with torch.no_grad():
            return [masked_cross_entropy(m.eval()(g), target, mask, return_pred=True) for m, mask in zip(members, val_masks)]

    def eval_composed():
        net2.eval()
        with torch.no_grad():
            z_ = net2(g)
            return [masked_cross_entropy(z_[:, k * S:k * S + C], target, val_masks[k], return_pred=True) for k in range(K)]

    cases = [("train step", "one network", train_one), ("train step", "sequential", train_sequential),
             ("train step", "composed", train_composed), ("eval + pred", "one network", eval_one),
             ("eval + pred", "sequential", eval_sequential), ("eval + pred", "composed", eval_composed)]
    times = {(name, form): [] for name, form, _ in cases}
    peak = {}
    for rnd in range(args.rounds + 1):                      # round 0 = warm-up (plans, restricted operators, allocator)
        for name, form, fn in cases:
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
            if rnd:
                times[(name, form)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
                peak[(name, form)] = max(peak.get((name, form), 0), torch.cuda.max_memory_allocated() - before)
    res = {}
    for (name, form), ts in times.items():
        ts = sorted(ts)
        res[(name, form)] = (ts[len(ts) // 2], ts[-1] - ts[0])
        say(f"  {name:12s} {form:12s} median {res[(name, form)][0]:9.3f} ms   min {ts[0]:9.3f}   max {ts[-1]:9.3f}   spread "
            f"(max - min) {ts[-1] - ts[0]:8.3f} ms   peak extra memory {peak[(name, form)] / 2 ** 20:9.1f} MiB")
    for name in ("train step", "eval + pred"):
        for other in ("sequential", "composed"):
            say(f"  {shape} {name}: one network against {other}: {verdict(res[(name, 'one network')], res[(name, other)])}")
    del net, net2, members, opt_net, opt_net2, opt_members, g
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
