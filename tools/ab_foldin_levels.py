#!/usr/bin/env python3
"""Interleaved timing of classifying a batch of NEW documents through the per-level hierarchy (two or three trained
two-layer GCNs on one graph), four ways, in one process:

    (a)  fused      `FoldInLevels.logits`: one launch of tgcn_foldin_levels on the frozen tables, batch handed over as a scipy
                    CSR on the host (what `Text2GraphTransformer.transform` returns: host checks and the copy are inside)
    (a') the same on device-resident CSR tensors
    (b)  composed   the same definition after `enable_fused_foldin(False)`: ONE plan of the [B, V] matrix per batch, one SpMM
                    at the combined table's width, torch's softmax, `dense.xw` for H_d Wh and u W2
    (c)  today      what a user does without it: per level `extended_graph` (from the second level on with the softmax of
                    the level above as the new rows' H) + a new plan + the model's eval forward on all N + B nodes

Shapes: h = 100 with C = (6, 64) and C = (9, 70, 128), on config c2 of bench.py (100 000 nodes / 2 M edges) and the `synth`
word-document graph of real-corpus size (60 000 nodes / 6 M edges), each generated with 8 192 extra documents that are then
held out; batches of 1, 256, 4 096 and 65 536 rows cut from them.  The old documents carry `predicted_hierarchy` in every
arm.  HIP events around each call; one warm-up round, then `--rounds` rounds with the arms alternating.  Reported per arm:
median and spread (max - min).  Verdict by the project's rule: faster or slower only if the medians differ by more than the
SUM of the two spreads.  Before timing, the arms' last-level logits are compared.

    timeout 900 python tools/ab_foldin_levels.py [--shapes c2 corpus] [--rounds 5] [--log profiles/r20_ab_foldin_levels.log]
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytextgcn_amd as pkg  # noqa: E402
from pytextgcn_amd import synth  # noqa: E402
from pytextgcn_amd.inductive import FoldInLevels, enable_fused_foldin, extended_graph, levels_lds_bytes  # noqa: E402
from pytextgcn_amd.perlevel import predicted_hierarchy, with_hierarchy  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
CLASSES = {"6-64": (6, 64), "9-70-128": (9, 70, 128)}
N_HOLD, HIDDEN = 8192, 100
BATCHES = [1, 256, 4096, 65536]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--classes", nargs="+", default=sorted(CLASSES), choices=sorted(CLASSES))
ap.add_argument("--batches", nargs="+", type=int, default=BATCHES)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r20_ab_foldin_levels.log"))
args = ap.parse_args()
dev = torch.device("cuda:0")
log = open(args.log, "w")
warnings.filterwarnings("ignore")


def say(line=""):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def verdict(a, b):
    """(median, spread) of two arms -> what may be said about a against b"""
    if abs(a[0] - b[0]) <= a[1] + b[1]:
        return "no difference (the medians differ by less than the sum of the spreads)"
    return f"{'faster' if a[0] < b[0] else 'SLOWER'} ({b[0] / a[0]:.2f} x)"


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


say(f"ab_foldin_levels: {torch.cuda.get_device_name(0)}; h={HIDDEN}; {N_HOLD} documents held out of each graph; HIP events; "
    f"1 warm-up round, then {args.rounds} rounds, arms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    scale = (N + N_HOLD) / N
    full = synth.word_doc_graph(N + N_HOLD, int(E * scale) // 2 * 2, seed=44, device=dev, n_classes=64,
                                vocab_frac=0.1 * N / (N + N_HOLD))
    g, held, _ = synth.hold_out_documents(full, N_HOLD)
    del full
    V, Ng = int(g.n_vocab), g.x.size(0)
    say(f"{shape}: training graph N={Ng} V={V} edges={g.edge_index.size(1)}; held-out rows hold "
        f"{held.nnz / N_HOLD:.1f} words on average")
    for name in args.classes:
        Cs = CLASSES[name]
        torch.manual_seed(0)
        models, graphs = [], [g]
        for l, C in enumerate(Cs):
            models.append(pkg.GCN(Ng + (Cs[l - 1] if l else 0), C, n_hidden_gcn=HIDDEN).to(dev).float().eval())
            if l + 1 < len(Cs):
                graphs.append(with_hierarchy(g, predicted_hierarchy(models[l], graphs[l])))
        fold = FoldInLevels(models, graphs)
        say(f" {shape} C={Cs}: {levels_lds_bytes([HIDDEN] * len(Cs), Cs)} bytes of LDS per workgroup, "
            f"{4 * fold._tab.stride(0)} B of table per word")
        for B in args.batches:
            rows = np.arange(B) % N_HOLD
            batch = held[rows].tocsr()
            dev_csr = tuple(torch.from_numpy(a).to(dev) for a in (batch.indptr.astype(np.int64), batch.indices.astype(np.int32),
                                                                  batch.data.astype(np.float32)))

            def arm_fused(inp=batch):
                return fold.logits(inp)

            def arm_fused_dev():
                return fold.logits(dev_csr)

            def arm_composed():
                was = enable_fused_foldin(False)
                try:
                    return fold.logits(batch)
                finally:
                    enable_fused_foldin(was)

            def arm_today():
                pkg.clear_plan_cache()
                with torch.no_grad():
                    z = models[0](extended_graph(g, batch))
                    for m, gl in zip(models[1:], graphs[1:]):
                        z = m(extended_graph(gl, batch, hierarchy=torch.softmax(z[Ng:].float(), dim=1)))
                return z[Ng:]

            za, zb, zc = arm_fused()[-1], arm_composed()[-1], arm_today()
            ref = float(zc.abs().max())
            say(f"  {shape} C={Cs} B={B}: nnz={batch.nnz}; last level, max-norm relative difference fused / composed "
                f"{float((za - zb).abs().max()) / ref:.1e}, fused / today's forward {float((za - zc).abs().max()) / ref:.1e}")
            del za, zb, zc
            pkg.clear_plan_cache()
            arms = {"(a) fused": arm_fused, "(a') fused, device CSR": arm_fused_dev, "(b) composed": arm_composed,
                    "(c) today": arm_today}
            times = {k: [] for k in arms}
            for rnd in range(args.rounds + 1):              # round 0 = warm-up
                for k, fn in arms.items():
                    ms = timed(fn)
                    if rnd:
                        times[k].append(ms)
            res = {}
            for k, ts in times.items():
                ts = sorted(ts)
                res[k] = (ts[len(ts) // 2], ts[-1] - ts[0])
                say(f"    {k:24s} median {res[k][0]:10.3f} ms   spread (max - min) {res[k][1]:9.3f} ms   "
                    f"{B / res[k][0] * 1e3:12.0f} docs/s")
            say(f"    {shape} C={Cs} B={B}: (a) fused against (b) composed: {verdict(res['(a) fused'], res['(b) composed'])}")
            say(f"    {shape} C={Cs} B={B}: (a) fused against (c) today: {verdict(res['(a) fused'], res['(c) today'])}")
        del fold, models, graphs
    del g, held
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
