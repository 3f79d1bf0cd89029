#!/usr/bin/env python3
"""Interleaved timing of classifying a batch of NEW documents through the per-label strategy (a top two-layer GCN and the K
per-label two-layer GCNs of a `PerLabelGCN` on one graph), five ways, in one process:

    (a)  fused      `FoldInPerLabel.predict_levels`: one launch of tgcn_foldin_routed on the frozen tables, batch handed over
                    as a scipy CSR on the host (what `Text2GraphTransformer.transform` returns: checks and copy are inside)
    (a') the same with `route=` given (the top model is not evaluated; the route is device-resident)
    (b)  composed   the same definition after `enable_fused_foldin(False)`: ONE plan of the [B, V] matrix per batch, one SpMM
                    over the whole combined table, `dense.xw` for the top model and per member present in the batch
    (b') sorted     the obvious alternative without a new kernel: tgcn_foldin_two_layer on the top tables, the routes to the
                    host, a stable sort of the rows by route, then K launches of tgcn_foldin_two_layer on the members' tables
    (c)  today      what a user does without any of it: `extended_graph` + a new plan + the top model's eval forward on all
                    N + B nodes + `PerLabelGCN.predict` on them

Shapes: h = 100, K = 6 members with 10 + 11 + 11 + 10 + 11 + 11 = 64 classes, on config c2 of bench.py (100 000 nodes / 2 M
edges) and the `synth` word-document graph of real-corpus size (60 000 nodes / 6 M edges), each generated with 8 192 extra
documents that are then held out; batches of 1, 256, 4 096 and 65 536 rows cut from them.  HIP events around each call; one
warm-up round, then `--rounds` rounds with the arms alternating.  Reported per arm: median and spread (max - min).  Verdict
by the project's rule: faster or slower only if the medians differ by more than the SUM of the two spreads.  Before timing,
the arms' predictions are compared.

    timeout 900 python tools/ab_foldin_perlabel.py [--shapes c2 corpus] [--rounds 7] [--log profiles/r23_ab_foldin_perlabel.log]
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
from pytextgcn_amd import _lib, synth  # noqa: E402
from pytextgcn_amd.inductive import FoldIn, FoldInPerLabel, enable_fused_foldin, extended_graph, routed_lds_bytes  # noqa: E402
from pytextgcn_amd.plan import _stream_ptr  # noqa: E402

SHAPES = {"c2": (100_000, 2_000_000), "corpus": (60_000, 6_000_000)}
CLASSES = (10, 11, 11, 10, 11, 11)
N_HOLD, HIDDEN = 8192, 100
BATCHES = [1, 256, 4096, 65536]

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["c2", "corpus"], choices=sorted(SHAPES))
ap.add_argument("--batches", nargs="+", type=int, default=BATCHES)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r23_ab_foldin_perlabel.log"))
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


def r4(v):
    return (v + 3) & ~3


def sorted_launches(fold, flat_top, batch):
    """(b'): the flat kernel on the top tables, then per member on the rows that route to it."""
    lib = _lib.load()
    route = flat_top.predict(batch)
    order = torch.argsort(route, stable=True)
    counts = torch.bincount(route, minlength=fold.K).cpu().numpy()
    rows = batch[order.cpu().numpy()].tocsr()
    rowptr = torch.from_numpy(rows.indptr.astype(np.int64)).to(dev)
    col = torch.from_numpy(rows.indices.astype(np.int32)).to(dev)
    val = torch.from_numpy(rows.data.astype(np.float32)).to(dev)
    if col.numel() == 0:
        col, val = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    B = rows.shape[0]
    pred = torch.empty(B, dtype=torch.int32, device=dev)
    logits = torch.empty(B, r4(max(fold.C)), dtype=torch.float32, device=dev)
    at, tab = 0, fold._tab
    for k, n in enumerate(counts.tolist()):
        if n == 0:
            continue
        s, C = fold.seg_start[k], fold.C[k]
        _lib.check(lib.tgcn_foldin_two_layer(
            n, rowptr.data_ptr() + 8 * at, col.data_ptr(), val.data_ptr(), fold.n_vocab, fold.dis.data_ptr(),
            _lib.DEGREE_SUMS[fold.degree_sum], tab.data_ptr() + 4 * fold.t1_col[k + 1], tab.stride(0), fold.h, None,
            fold.b1[k].data_ptr(), _lib.ACT_NONE, tab.data_ptr() + 4 * fold.p_col[k + 1], tab.stride(0), C,
            fold.W2.data_ptr() + 4 * s, fold.W2.stride(0), fold.b2.data_ptr() + 4 * s, logits.data_ptr() + 4 * at * logits.stride(0),
            logits.stride(0), pred.data_ptr() + 4 * at, None, 0, _stream_ptr(dev)))
        at += n
    out = torch.empty(B, dtype=torch.int64, device=dev)
    seg = torch.tensor(fold.seg_start, device=dev)[route[order]]
    out[order] = fold.class_map[seg + pred.long()] if fold.class_map is not None else pred.long()
    return torch.stack([route, out], dim=1)


say(f"ab_foldin_perlabel: {torch.cuda.get_device_name(0)}; h={HIDDEN}; K={len(CLASSES)} members with {CLASSES} classes; "
    f"{N_HOLD} documents held out of each graph; HIP events; 1 warm-up round, then {args.rounds} rounds, arms interleaved")
K = len(CLASSES)
class_map = [[100 * k + j for j in range(C)] for k, C in enumerate(CLASSES)]
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
    torch.manual_seed(0)
    top = pkg.GCN(Ng, K, n_hidden_gcn=HIDDEN).to(dev).float().eval()
    net = pkg.PerLabelGCN(Ng, CLASSES, n_hidden_gcn=HIDDEN).to(dev).float().eval()
    fold = FoldInPerLabel(top, net, g, class_map)
    flat_top = FoldIn(top, g)
    cm_dev = pkg.perlabel.column_class_map(class_map, dev)
    say(f" {shape}: {routed_lds_bytes([HIDDEN] * (K + 1), [K] + list(CLASSES))} bytes of LDS per workgroup, "
        f"{4 * fold._tab.stride(0)} B of table per word, of which a document reads {4 * (2 * r4(HIDDEN) + r4(K) + r4(max(CLASSES)))}")
    for B in args.batches:
        rows = np.arange(B) % N_HOLD
        batch = held[rows].tocsr()
        route_dev = fold.predict_levels(batch)[:, 0].to(torch.int32).contiguous()

        def arm_fused():
            return fold.predict_levels(batch)

        def arm_fused_route():
            return fold.predict(batch, route=route_dev)

        def arm_composed():
            was = enable_fused_foldin(False)
            try:
                return fold.predict_levels(batch)
            finally:
                enable_fused_foldin(was)

        def arm_sorted():
            return sorted_launches(fold, flat_top, batch)

        def arm_today():
            pkg.clear_plan_cache()
            with torch.no_grad():
                ge = extended_graph(g, batch)
                route = torch.full((Ng + B,), -1, dtype=torch.int32, device=dev)
                route[Ng:] = top(ge)[Ng:].argmax(dim=1).to(torch.int32)
                return torch.stack([route[Ng:].long(), net.predict(ge, route, cm_dev)[Ng:]], dim=1)

        pa, pr, pb, ps, pc = arm_fused(), arm_fused_route(), arm_composed(), arm_sorted(), arm_today()
        say(f"  {shape} B={B}: nnz={batch.nnz}; predictions that differ from (a): (a') {int((pr != pa[:, 1]).sum())}, "
            f"(b) {int((pb != pa).any(dim=1).sum())}, (b') {int((ps != pa).any(dim=1).sum())}, (c) {int((pc != pa).any(dim=1).sum())} "
            f"of {B} (untrained models: near-ties of the logits may fall either way in another summation order)")
        del pa, pr, pb, ps, pc
        pkg.clear_plan_cache()
        arms = {"(a) fused": arm_fused, "(a') fused, route given": arm_fused_route, "(b) composed": arm_composed,
                "(b') sorted, K launches": arm_sorted, "(c) today": arm_today}
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
            say(f"    {k:26s} median {res[k][0]:10.3f} ms   spread (max - min) {res[k][1]:9.3f} ms   "
                f"{B / res[k][0] * 1e3:12.0f} docs/s")
        for other in ("(b) composed", "(b') sorted, K launches", "(c) today"):
            say(f"    {shape} B={B}: (a) fused against {other}: {verdict(res['(a) fused'], res[other])}")
    del fold, flat_top, top, net, g, held
    pkg.clear_plan_cache()
    torch.cuda.empty_cache()
log.close()
