#!/usr/bin/env python3
"""Interleaved timing of the level-2 `GCN` of the per-level strategy (perlevel_amazon.py:122-150) on its two feature forms, in
one process, both on the package's fused loss and fused Adam:

    A  sparse      g.x is the sparse [I_N | H] tensor: `conv.features_times` composes w[:N] + sparse_times(H, w[N:])
    B  features    g.x is `HierarchyFeatures` (class ids): the kernels of pytextgcn_amd/csrc/hier.hip

Settings: hidden width 100, dropout 0.5, Fh = 6 top labels, 64 classes.  Shapes: config c2 of bench.py (100 000 nodes / 2 M
edges) and a `synth` word-document graph of real-corpus size (60 000 nodes / 6 M edges).  The train step (forward, loss,
backward, optimizer step) and the eval forward are timed with HIP events after a warm-up round; several rounds with the two
arms alternating, so that clock and temperature drift hits both alike; reported are the median and the spread (max - min) /
median of the repetitions, and the extra peak memory of one train step.  Before timing, the two arms' eval logits on the
same weights are compared (faster and different is not faster).  No ratio is fixed in advance: the composition on the
same commit is the yardstick.

    timeout 900 python tools/ab_perlevel.py [--shapes c2 corpus] [--rounds 5] [--reps 5]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import perlevel, synth  # noqa: E402
from pytextgcn_amd.functional import masked_cross_entropy  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--hidden", type=int, default=100)
ap.add_argument("--dropout", type=float, default=0.5)
ap.add_argument("--top", type=int, default=6)
ap.add_argument("--classes", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
h, Fh, C = args.hidden, args.top, args.classes


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, ts[0], ts[-1], (ts[-1] - ts[0]) / med


print(f"ab_perlevel: {torch.cuda.get_device_name(0)}; hidden={h} dropout={args.dropout} Fh={Fh} classes={C}; 1 warm-up round, "
      f"then {args.rounds} rounds x {args.reps} timed repetitions, arms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    g = synth.word_doc_graph(N, E, seed=44, n_classes=C)
    y_top = g.y[g.n_vocab:] * Fh // C                       # the top label of a document: its class's block
    g = pkg.Data(**{k: getattr(g, k) for k in g.keys}).to(dev)
    feats = perlevel.one_hot_hierarchy(g, y_top, n_classes=Fh)
    graphs = {"features": perlevel.with_hierarchy(g, feats), "sparse": perlevel.with_hierarchy(g, feats.to_sparse())}
    torch.manual_seed(0)
    models = {"features": pkg.GCN(N + Fh, C, n_hidden_gcn=h, dropout=args.dropout).to(dev).float()}
    models["sparse"] = pkg.GCN(N + Fh, C, n_hidden_gcn=h, dropout=args.dropout).to(dev).float()
    models["sparse"].load_state_dict(models["features"].state_dict())
    opts = {k: pkg.optim.Adam(m.parameters(), lr=0.01) for k, m in models.items()}

    with torch.no_grad():                                   # the same function, before anything is timed
        za, zb = (models[k].eval()(graphs[k]) for k in ("sparse", "features"))
        print(f"{shape}: N={N} edges={E} documents={N - g.n_vocab}; eval logits, features against sparse: max|a - b| / max|b| = "
              f"{float((zb - za).abs().max() / za.abs().max()):.2e}")

    def train(k):
        def fn():
            models[k].train()
            loss = masked_cross_entropy(models[k](graphs[k]), g.y, g.train_mask)
            opts[k].zero_grad(set_to_none=True)
            loss.backward()
            opts[k].step()
        return fn

    def evaluate(k):
        def fn():
            models[k].eval()
            with torch.no_grad():
                models[k](graphs[k])
        return fn

    cases = [("train step", "sparse", train("sparse")), ("train step", "features", train("features")),
             ("eval forward", "sparse", evaluate("sparse")), ("eval forward", "features", evaluate("features"))]
    times = {(name, arm): [] for name, arm, _ in cases}
    for rnd in range(args.rounds + 1):                      # round 0 = warm-up (plans, feature plans, allocator)
        for name, arm, fn in cases:
            fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for i in range(args.reps):
                fn()
                ev[i + 1].record()
            torch.cuda.synchronize()
            if rnd:
                times[(name, arm)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
    med = {}
    for (name, arm), ts in times.items():
        m_, lo, hi, spread = stats(ts)
        med[(name, arm)] = m_
        print(f"  {name:12s} {arm:9s}  median {m_:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   spread (max - min) / median "
              f"{100 * spread:5.1f} %")
    for name in ("train step", "eval forward"):
        a, b = med[(name, "features")], med[(name, "sparse")]
        print(f"  {shape} {name}: features / sparse = {a / b:.3f}  ({b / a:.2f} x)")
    for arm in ("sparse", "features"):                      # extra peak memory of one (warm) train step
        opts[arm].zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        train(arm)()
        torch.cuda.synchronize()
        print(f"  {shape} train step {arm:9s} extra peak memory {(torch.cuda.max_memory_allocated() - base) / 2**20:8.1f} MiB "
              f"(W1 is {(N + Fh) * h * 4 / 2**20:.1f} MiB)")
    del models, opts, graphs, feats, g
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
