#!/usr/bin/env python3
"""Interleaved A/B of the ReLU fused into the SpMM epilogue at the c4 shapes (2 M nodes, 50 M edges, hidden 200, 64 classes).

  python tools/ab_activation.py            both parts below, each a child process under its own time limit; stops at the
                                           first one that fails
  python tools/ab_activation.py spmm       (a) tgcn_spmm against tgcn_spmm_act(RELU) at F = 200 -- the bytes are equal, so
                                           the times should be -- with the same launch against ITSELF beside it (the
                                           run-to-run spread a difference has to exceed), and the backward gate pass
                                           (tgcn_act_grad with the column sums) on its own: ms and GB/s of the 3 N F 4 bytes
                                           it has to move
  python tools/ab_activation.py epoch      (b) FlatLoop.epoch(): the linear network, the activation fused
                                           (GCN(apply_activation=True)), and the composition a user could write before
                                           (torch.relu on the first layer's output, torch dropout, torch autograd)

Every variant is warmed up, the variants alternate in an order that rotates from round to round, and medians and the
min-max spread of the rounds are printed."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, E, H, C = 2_000_000, 50_000_000, 200, 64
if os.environ.get("AB_SHAPE"):               # AB_SHAPE=100000,2000000,200,64: another configuration (c2)
    N, E, H, C = (int(v) for v in os.environ["AB_SHAPE"].split(","))
ROUNDS = int(os.environ.get("AB_ROUNDS", "7"))


def report(title, times):
    print(title)
    base = None
    for name, ts in times.items():
        ts = ts[1:]                          # the first round is warm-up
        med = statistics.median(ts)
        base = med if base is None else base
        print(f"  {name:34s} median {med:8.3f} ms   min {min(ts):8.3f}   max {max(ts):8.3f}   "
              f"({100.0 * (med / base - 1.0):+.2f} % against the first row)")


def rotate(cases, rnd):
    names = list(cases)
    k = rnd % len(names)
    return names[k:] + names[:k]


def part_spmm():
    import torch
    from pytextgcn_amd import _lib, plan as plan_mod, synth
    dev = torch.device("cuda:0")
    g = synth.word_doc_graph(N, E, seed=44, n_classes=C, device=dev)
    plan = plan_mod.plan_for(g.edge_index, g.edge_attr, N)
    x, b = torch.randn(N, H, device=dev), torch.randn(H, device=dev)
    out = torch.empty(N, H, device=dev)
    a = torch.relu(torch.randn(N, H, device=dev))
    grad = torch.randn(N, H, device=dev)
    cases = {
        "tgcn_spmm": lambda: plan.spmm(x, b, out=out),
        "tgcn_spmm (the same, again)": lambda: plan.spmm(x, b, out=out),
        "tgcn_spmm_act(RELU)": lambda: plan.spmm(x, b, out=out, activation=_lib.ACT_RELU),
        "tgcn_act_grad + column sums": lambda: plan_mod.relu_grad_(a, grad, want_colsum=True),
        "tgcn_colsum alone": lambda: plan_mod.colsum(grad),
    }
    assert torch.equal(plan.spmm(x, b, activation=_lib.ACT_RELU), torch.relu(plan.spmm(x, b)))
    times = {k: [] for k in cases}
    reps = 10
    for rnd in range(ROUNDS + 1):
        for name in rotate(cases, rnd):
            fn = cases[name]
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    report(f"(a) one launch, N={N} E={E} F={H}; HIP events around {reps} launches, {ROUNDS} rounds, rotating order", times)
    gate = statistics.median(times["tgcn_act_grad + column sums"][1:])
    nbytes = 3 * N * H * 4
    print(f"  backward gate pass: {nbytes / 1e9:.2f} GB (read A, read and write G) in {gate:.3f} ms = "
          f"{nbytes / gate / 1e6:.0f} GB/s")


def part_epoch():
    import torch
    import pytextgcn_amd as pkg
    from pytextgcn_amd import synth
    from pytextgcn_amd.train import FlatLoop
    dev = torch.device("cuda:0")
    g = synth.word_doc_graph(N, E, seed=44, n_classes=C, device=dev)

    class UnfusedRelu(pkg.GCN):
        """What a user had to write: torch.relu on the first layer's output, torch's dropout and autograd."""

        def forward(self, g, rows=None):
            l1, l2 = self.layers
            x = torch.relu(l1(g.x, g.edge_index, g.edge_attr))
            x = torch.nn.functional.dropout(x, p=self.dropout, training=self.training)
            return l2(x, g.edge_index, g.edge_attr, rows=rows) if rows is not None else l2(x, g.edge_index, g.edge_attr)

    def loop_of(cls, **kw):
        torch.manual_seed(0)
        return FlatLoop(cls(N, C, n_hidden_gcn=H, dropout=0.5, **kw).to(dev), g, lr=0.02)
    loops = {
        "linear (the default network)": loop_of(pkg.GCN),
        "activation on, fused": loop_of(pkg.GCN, apply_activation=True),
        "activation on, unfused composition": loop_of(UnfusedRelu),
    }
    times = {k: [] for k in loops}
    reps = 5
    for rnd in range(ROUNDS + 1):
        for name in rotate(loops, rnd):
            loop = loops[name]
            loop.epoch()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                loop.epoch()                 # ends in a stream synchronisation
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    report(f"(b) FlatLoop.epoch(), N={N} E={E} hidden={H} classes={C} dropout=0.5; host clock around {reps} epochs, "
           f"{ROUNDS} rounds, rotating order", times)
    for loop in loops.values():
        loop.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        {"spmm": part_spmm, "epoch": part_epoch}[sys.argv[1]]()
        sys.exit(0)
    for part, limit in (("spmm", 240), ("epoch", 300)):
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), part]).returncode
        if rc != 0:
            print(f"part {part} ended with status {rc}: nothing more is started")
            sys.exit(rc)
