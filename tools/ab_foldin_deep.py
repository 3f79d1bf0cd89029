#!/usr/bin/env python3
"""Interleaved timing of classifying a batch of NEW documents with a trained JumpingKnowledgeNetwork(n_gcn=2) and a trained
GCN(n_gcn=3), three ways, in one process (the mould of tools/ab_foldin.py):

    (a) fused      `FoldInDeep.logits`: one launch of tgcn_foldin_layers on the frozen tables (JKN: then the JK-LSTM
                   aggregation and `lin` on the B rows)
    (b) composed   the same definition after `enable_fused_foldin(False)`: tgcn_gcn_norm on the bipartite edges, a plan of
                   the [B, V] matrix per batch, one SpMM per layer, one dense product per layer from the second on
    (c) full       what a user does without fold-in: `extended_graph` + a new plan + the model's eval forward on all
                   N + B nodes (the plan cache is cleared per call: the edge list is new every time)

Every arm is handed the batch as a scipy CSR on the host (what `Text2GraphTransformer.transform` returns), so host checks
and the copy to the device are inside every figure; (a) is timed a second time on device-resident CSR tensors.  For the JKN
the device-CSR arm is also split: the fold-in launch alone (`FoldInDeep.activations`) and the JK + `lin` remainder (the
difference of the medians).  Shapes: config c2 of bench.py (100 000 nodes / 2 M edges) and a `synth` word-document graph of
real-corpus size (60 000 nodes / 6 M edges), each generated with 8 192 extra documents that are then held out of the
graph; batches of 1, 256, 4 096 and 65 536 rows cut from them (the held-out rows repeat in the largest batch).  Hidden
width 100, 64 classes.

HIP events around each call; one warm-up round, then `--rounds` rounds with the arms alternating.  Reported per arm: the
median and the spread (max - min) of the rounds and documents per second.  Verdict by the project's rule: faster or slower
only if the medians differ by more than the SUM of the two spreads.  Before timing, the three results are compared.

    timeout 900 python tools/ab_foldin_deep.py [--shapes c2 corpus] [--rounds 5] [--log profiles/r24_ab_foldin_deep.log]
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
from pytextgcn_amd.inductive import FoldInDeep, enable_fused_foldin, extended_graph  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
N_HOLD, N_CLASSES, HIDDEN = 8192, 64, 100
BATCHES = [1, 256, 4096, 65536]
MODELS = {
    "JKN(h=100, n_gcn=2)": lambda N: pkg.JumpingKnowledgeNetwork(N, N_CLASSES, n_gcn=2, n_hidden_gcn=HIDDEN),
    "GCN(h=100, n_gcn=3)": lambda N: pkg.GCN(N, N_CLASSES, n_gcn=3, n_hidden_gcn=HIDDEN),
}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--batches", nargs="+", type=int, default=BATCHES)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r24_ab_foldin_deep.log"))
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
    """ms between two HIP events around fn"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


say(f"ab_foldin_deep: {torch.cuda.get_device_name(0)}; classes={N_CLASSES}, hidden={HIDDEN}; {N_HOLD} documents held out of each "
    f"graph; HIP events; 1 warm-up round, then {args.rounds} rounds, arms interleaved")
for shape in args.shapes:
    N, E = SHAPES[shape]
    scale = (N + N_HOLD) / N
    full = synth.word_doc_graph(N + N_HOLD, int(E * scale) // 2 * 2, seed=44, device=dev, n_classes=N_CLASSES,
                                vocab_frac=0.1 * N / (N + N_HOLD))
    g, held, _ = synth.hold_out_documents(full, N_HOLD)
    del full
    V = int(g.n_vocab)
    say(f"{shape}: training graph N={g.x.size(0)} V={V} edges={g.edge_index.size(1)}; held-out rows hold "
        f"{held.nnz / N_HOLD:.1f} words on average")
    for name, make in MODELS.items():
        torch.manual_seed(0)
        model = make(g.x.size(0)).to(dev).float().eval()
        fold = FoldInDeep(model, g)
        jkn = fold.jkn
        for B in args.batches:
            rows = np.arange(B) % N_HOLD
            batch = held[rows].tocsr()
            dev_csr = tuple(torch.from_numpy(a).to(dev) for a in (batch.indptr.astype(np.int64), batch.indices.astype(np.int32),
                                                                  batch.data.astype(np.float32)))

            def arm_fused(inp=batch):
                return fold.logits(inp)

            def arm_fused_dev():
                return fold.logits(dev_csr)

            def arm_chain_dev():
                return fold.activations(dev_csr)

            def arm_composed():
                was = enable_fused_foldin(False)
                try:
                    return fold.logits(batch)
                finally:
                    enable_fused_foldin(was)

            def arm_full():
                pkg.clear_plan_cache()
                ge = extended_graph(g, batch)
                with torch.no_grad():
                    return model(ge)[g.x.size(0):]

            za, zb, zc = arm_fused(), arm_composed(), arm_full()
            ref = float(zc.abs().max())
            say(f"  {shape} {name} B={B}: nnz={batch.nnz}; max-norm relative difference fused / composed "
                f"{float((za - zb).abs().max()) / ref:.1e}, fused / full forward {float((za - zc).abs().max()) / ref:.1e}")
            del za, zb, zc
            pkg.clear_plan_cache()
            arms = {"(a) fused": arm_fused, "(a') fused, device CSR": arm_fused_dev, "(b) composed": arm_composed,
                    "(c) full forward": arm_full}
            if jkn:
                arms["(a'') fold-in launch alone, device CSR"] = arm_chain_dev
            times = {k: [] for k in arms}
            for rnd in range(args.rounds + 1):              # round 0 = warm-up
                for arm, fn in arms.items():
                    ms = timed(fn)
                    if rnd:
                        times[arm].append(ms)
            res = {}
            for arm, ts in times.items():
                ts = sorted(ts)
                res[arm] = (ts[len(ts) // 2], ts[-1] - ts[0])
                say(f"    {arm:40s} median {res[arm][0]:10.3f} ms   spread (max - min) {res[arm][1]:9.3f} ms   "
                    f"{B / res[arm][0] * 1e3:12.0f} docs/s")
            if jkn:
                whole, chain = res["(a') fused, device CSR"], res["(a'') fold-in launch alone, device CSR"]
                say(f"    {shape} {name} B={B}: JKN split on device CSR: fold-in launch {chain[0]:.3f} ms, JK + lin remainder "
                    f"{whole[0] - chain[0]:.3f} ms (difference of the medians; spreads {chain[1]:.3f} / {whole[1]:.3f} ms)")
            say(f"    {shape} {name} B={B}: (a) fused against (b) composed: {verdict(res['(a) fused'], res['(b) composed'])}")
            say(f"    {shape} {name} B={B}: (a) fused against (c) full forward: {verdict(res['(a) fused'], res['(c) full forward'])}")
        del fold, model
    del g, held
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
