#!/usr/bin/env python3
"""Interleaved timing of JumpingKnowledge("lstm")'s fused forward kernel against the composed forward (the chunked pieces
of the backward run forward only, `jk.enable_fused_jk(False)`), at c2's node count and (C, L) = (64, 2) and (200, 2): the
eval forward, the train step (forward with ReLU epilogue + backward; the backward is the same chunked recomputation for both)
and the peak memory above the operands (`torch.cuda.max_memory_allocated`), with HIP events, a warm-up round and the median
of the repetitions (several rounds, variants alternating, so that clock and temperature drift hits both alike).

    python tools/ab_jkn.py [--config c2] [--rounds 6] [--reps 5] [--chunk-rows 8192]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytextgcn_amd import jk  # noqa: E402

CONFIGS = {"c1": 5_000, "c2": 100_000}      # nodes (BASELINE.json)

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=sorted(CONFIGS), default="c2")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--chunk-rows", type=int, default=jk.DEFAULT_CHUNK_ROWS)
args = ap.parse_args()

dev = torch.device("cuda:0")
N = CONFIGS[args.config]
print(f"ab_jkn: {torch.cuda.get_device_name(0)}; config {args.config}: N={N}; chunk_rows={args.chunk_rows}; "
      f"{args.rounds} rounds x {args.reps} repetitions, interleaved")


def stats(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return med, ts[0], ts[-1], (ts[-1] - ts[0]) / med


for C, L in ((64, 2), (200, 2)):
    torch.manual_seed(0)
    agg = jk.JumpingKnowledge("lstm", channels=C, num_layers=L, chunk_rows=args.chunk_rows).to(dev).float()
    xs = [torch.randn(N, C, device=dev).requires_grad_() for _ in range(L)]
    G = torch.randn(N, C, device=dev)

    def eval_forward():
        with torch.no_grad():
            agg.aggregate(xs, relu=True)

    def train_step():
        for x in xs:
            x.grad = None
        agg.zero_grad(set_to_none=True)
        agg.aggregate(xs, relu=True).backward(G)

    cases = [(name, fn, fused) for name, fn in (("eval forward", eval_forward), ("train step", train_step))
             for fused in (True, False)]
    times = {(name, fused): [] for name, _, fused in cases}
    for rnd in range(args.rounds + 1):                       # round 0 = warm-up
        for name, fn, fused in cases:
            was = jk.enable_fused_jk(fused)
            try:
                fn()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
                ev[0].record()
                for i in range(args.reps):
                    fn()
                    ev[i + 1].record()
                torch.cuda.synchronize()
            finally:
                jk.enable_fused_jk(was)
            if rnd:
                times[(name, fused)] += [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
    peak = {}
    for fused in (True, False):
        was = jk.enable_fused_jk(fused)
        try:
            for x in xs:
                x.grad = None
            agg.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            train_step()
            torch.cuda.synchronize()
            peak[fused] = torch.cuda.max_memory_allocated() - base
        finally:
            jk.enable_fused_jk(was)
    H = agg.lstm.hidden_size
    print(f" C={C} L={L} H={H}:")
    med = {}
    for (name, fused), ts in times.items():
        m, lo, hi, spread = stats(ts)
        med[(name, fused)] = m
        print(f"  {name:13s} {'fused   ' if fused else 'composed'}  median {m:8.3f} ms   min {lo:8.3f}   max {hi:8.3f}   "
              f"spread (max - min) / median {100 * spread:5.1f} %")
    for name in ("eval forward", "train step"):
        f, c = med[(name, True)], med[(name, False)]
        print(f"  {name}: fused / composed = {f / c:.3f}  ({c / f:.2f} x)")
    flop = 2.0 * N * 2 * (L * C + (L - 1) * H) * 4 * H
    print(f"  fused forward: {flop / med[('eval forward', True)] / 1e9:.1f} TFLOP/s of gate products ({flop / 1e9:.1f} GFLOP)")
    for fused in (True, False):
        share = 1.0 - med[("eval forward", fused)] / med[("train step", fused)]
        print(f"  {'fused   ' if fused else 'composed'}: the backward is about {100 * share:.0f} % of the train step; peak memory of a "
              f"train step above the operands {peak[fused] / 2**20:8.1f} MiB (operands: {L} x N x C x 4 B = "
              f"{L * N * C * 4 / 2**20:.1f} MiB; stored gates of a library LSTM would be N L 2 4H 4 B = "
              f"{N * L * 8 * H * 4 / 2**20:.1f} MiB)")
    del xs, G, agg
