"""The first GCNConv's x @ W on [I_N | H] features (`tgcn_hier_xw*`) as plain tensor expressions, for the tests: the truth
the kernels are held to, and the sparse tensor the composition takes.  Test infrastructure; nothing under pytextgcn_amd/
imports this.

    C  = W[:N] + H @ W[N:]                      H [N, Fh]: the rows `Hd` from node h_row0 on, zeros above
    dW = [G ; H^T @ G]                          one matrix of W's shape"""
import math

import torch


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def one_hot(cls, Fh, dtype=torch.float32):
    """[rows, Fh]: the one-hot rows of the class ids; an id outside [0, Fh) leaves its row empty."""
    H = torch.zeros(cls.numel(), Fh, dtype=dtype)
    ok = (cls >= 0) & (cls < Fh)
    H[ok.nonzero().flatten(), cls[ok].long()] = 1.0
    return H


def operands(N, F, Fh, h_row0, form, seed):
    """W [N + Fh, F] glorot (as GCNConv initialises it), G standard normal, and the hierarchy rows: int32 class ids
    ("onehot": the training features, perlevel_amazon.py:112) or softmax rows ("dense": the test features, :110).  CPU."""
    gen = torch.Generator().manual_seed(seed)
    a = math.sqrt(6.0 / (N + Fh + F))
    W = (torch.rand(N + Fh, F, generator=gen) * 2 - 1) * a
    G = torch.randn(N, F, generator=gen)
    rows = N - h_row0
    if form == "onehot":
        held = torch.randint(0, Fh, (rows,), generator=gen).to(torch.int32)
    else:
        held = torch.softmax(2.0 * torch.randn(rows, Fh, generator=gen), dim=1)
    return W, G, held


def dense_rows(held, Fh, dtype=torch.float32):
    return one_hot(held, Fh, dtype) if not held.dtype.is_floating_point else held.to(dtype)


def truth(W, G, held, h_row0, dtype=torch.float64):
    """(C, dW) in `dtype` (float32: the same expressions in the kernels' precision, summed sequentially by torch's CPU)."""
    Fh = W.size(0) - G.size(0)
    N = G.size(0)
    W, G = W.detach().cpu().to(dtype), G.detach().cpu().to(dtype)
    Hd = dense_rows(held.detach().cpu(), Fh, dtype)
    C = W[:N].clone()
    C[h_row0:] += Hd @ W[N:]
    dW = torch.cat([G, Hd.t() @ G[h_row0:]], 0)
    return C, dW


def sparse_features(N, h_row0, held, Fh):
    """The coalesced sparse COO [I_N | H] tensor as text2graph.py:226-246 builds it (CPU)."""
    Hd = dense_rows(held.detach().cpu(), Fh)
    nz = torch.nonzero(Hd)
    ar = torch.arange(N)
    idx = torch.cat([torch.stack([ar, ar]), torch.stack([nz[:, 0] + h_row0, nz[:, 1] + N])], 1)
    val = torch.cat([torch.ones(N), Hd[nz[:, 0], nz[:, 1]]])
    return torch.sparse_coo_tensor(idx, val, (N, N + Fh), dtype=torch.float32).coalesce()
