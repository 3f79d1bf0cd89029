#!/usr/bin/env python3
"""Interleaved timing of the per-label strategy as ONE concatenated network (`PerLabelGCN` + the grouped cross-entropy)
against K sequential `GCN`s (what perlabel_amazon.py:90-155 runs, one model after the other), in one process, both on the
package's fused loss and fused Adam and torch's dropout.  Settings: K = 6 classifiers, hidden width 100, class counts
summing to 64 (Amazon's 64 Cat2 classes under 6 Cat1 labels).  Shapes: config c2 of bench.py (100 000 nodes / 2 M edges) and
a `synth` word-document graph of real-corpus size (60 000 nodes / 6 M edges).  The train step (forward, loss, backward,
optimizer step, for all K classifiers) and the eval forward (all K) are timed with HIP events after a warm-up round; several
rounds with the two forms alternating, so that clock and temperature drift hits both alike; reported are the median and the
spread (max - min) / median of the repetitions.  Before timing, the grouped network is built from the K members and its eval
logits are compared with theirs segment by segment (faster and different is not faster).

    timeout 900 python tools/ab_perlabel.py [--shapes c2 corpus] [--rounds 5] [--reps 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import synth  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402
from pytextgcn_amd.perlabel import PerLabelGCN, relabel  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
COUNTS = [10, 11, 11, 10, 11, 11]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
K, h = len(COUNTS), args.hidden
top_of = torch.repeat_interleave(torch.arange(K), torch.tensor(COUNTS))


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, ts[0], ts[-1], (ts[-1] - ts[0]) / med


print(f"ab_perlabel: {torch.cuda.get_device_name(0)}; K={K} hidden={h} class counts {COUNTS} dropout={args.dropout}; 1 warm-up "
      f"round, then {args.rounds} rounds x {args.reps} timed repetitions, forms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    g = synth.word_doc_graph(N, E, seed=44, n_classes=sum(COUNTS))
    is_doc = torch.arange(N) >= g.n_vocab
    group, target, counts, _ = relabel(g.y, top_of[g.y], is_doc)
    assert counts == COUNTS
    g = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(dev)
    group, target = group.to(dev), target.to(dev)
    torch.manual_seed(0)
    members = [pkg.GCN(N, c, n_hidden_gcn=h, dropout=args.dropout).to(dev).float() for c in COUNTS]
    net = PerLabelGCN.from_members(members)
    masks = [g.train_mask & (group == k) for k in range(K)]
    opt_net = pkg.optim.Adam(net.parameters(), lr=0.01)
    opt_members = [pkg.optim.Adam(m.parameters(), lr=0.01) for m in members]

    with torch.no_grad():                                   # the same function, before anything is timed
        z = net.eval()(g)
        worst = 0.0
        for k, (m, s, c) in enumerate(zip(members, net.seg_start, net.seg_width)):
            zk = m.eval()(g)
            worst = max(worst, float((z[:, s:s + c] - zk).abs().max() / zk.abs().max()))
    print(f"{shape}: N={N} edges={E}; eval logits, grouped against the members: max|a - b| / max|b| = {worst:.2e}")

    def train_grouped():
        net.train()
        loss, _ = net.loss(g, target, g.train_mask, group)
        opt_net.zero_grad(set_to_none=True)
        loss.backward()
        opt_net.step()

    def train_sequential():
        for m, opt, mask in zip(members, opt_members, masks):
            m.train()
            loss = masked_cross_entropy(m(g), target, mask)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    def eval_grouped():
        net.eval()
        with torch.no_grad():
            net(g)

    def eval_sequential():
        with torch.no_grad():
            for m in members:
                m.eval()(g)

    cases = [("train step", "grouped", train_grouped), ("train step", "sequential", train_sequential),
             ("eval forward", "grouped", eval_grouped), ("eval forward", "sequential", eval_sequential)]
    times = {(name, form): [] for name, form, _ in cases}
    for rnd in range(args.rounds + 1):                      # round 0 = warm-up (plans, restricted operators, allocator)
        for name, form, fn in cases:
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if rnd:
                times[(name, form)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
    med = {}
    for (name, form), ts in times.items():
        m_, lo, hi, spread = stats(ts)
        med[(name, form)] = m_
        print(f"  {name:12s} {form:10s}  median {m_:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   spread (max - min) / median "
              f"{100 * spread:5.1f} %")
    for name in ("train step", "eval forward"):
        a, b = med[(name, "grouped")], med[(name, "sequential")]
        print(f"  {shape} {name}: grouped / sequential = {a / b:.3f}  ({b / a:.2f} x)")
    del net, members, opt_net, opt_members, g
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
