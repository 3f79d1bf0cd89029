"""The reference's EGCN (textgcn/lib/models.py:28-52) restated for the tests from torch's `nn.Linear`, `torch.selu`,
dropout and the CPU oracle's GCNConv -- and, for the kernel tests, the fused front end as plain tensor expressions in
any dtype.  Test infrastructure; nothing under pytextgcn_amd/ imports this."""
import numpy as np
import torch
from torch import nn

from oracle.gcn_oracle import GCNConvOracle

import _dropout_hash as H


class EGCNRef(nn.Module):
    def __init__(self, in_channels, out_channels, embedding_dim=2000, n_gcn=2, n_hidden_gcn=64, activation=nn.ReLU,
                 dropout=0.5):
        super().__init__()
        self.activation = activation()            # constructed, never applied (models.py:32,49)
        self.dropout = dropout
        self.layers = nn.ModuleList([nn.Linear(in_channels, embedding_dim), GCNConvOracle(embedding_dim, n_hidden_gcn)])
        for _ in range(n_gcn - 2):
            self.layers.append(GCNConvOracle(n_hidden_gcn, n_hidden_gcn))
        self.layers.append(GCNConvOracle(n_hidden_gcn, out_channels))

    def forward(self, g):
        x = g.x
        lin = self.layers[0]
        # nn.Linear on the (possibly sparse) features: x @ weight^T + bias
        x = (torch.sparse.mm(x, lin.weight.t()) if x.is_sparse else x @ lin.weight.t()) + lin.bias
        x = torch.selu(x)
        x = nn.functional.dropout(x, p=self.dropout, training=self.training)
        for layer in self.layers[1:]:
            x = layer(x, g.edge_index, g.edge_attr)
            # the reference's guard `i < len(self.layers) - 1` runs over enumerate(self.layers[1:]): always true
            x = nn.functional.dropout(x, p=self.dropout, training=self.training)
        return x


def keep_matrix(seed: int, N: int, K: int, p: float, row0: int = 0) -> torch.Tensor:
    """[N, K] bool: the kernels' keep decision for node i (mask row i + row0) and column k."""
    rows = (np.arange(N, dtype=np.uint64) + np.uint64(row0))[:, None]
    cols = np.arange(K, dtype=np.uint64)[None, :]
    return torch.from_numpy(np.asarray(H.keep_mask(seed, rows, cols, p)).reshape(N, K))


def activation(E, b, keep=None, p=0.0):
    """a [N, K] = s * keep * selu(E^T + b) in the dtype of E (float64 for the truth)."""
    a = torch.selu(E.t() + b)
    if keep is not None:
        a = a * keep.to(a.dtype) / (1.0 - p)
    return a


def fused_truth(E, b, W, G=None, keep=None, p=0.0):
    """float64 C = a @ W and, given G = dC, (dE, db, dW) by autograd through the expressions above."""
    E, b, W = (t.detach().cpu().double().requires_grad_() for t in (E, b, W))
    C = activation(E, b, keep, p) @ W
    if G is None:
        return C.detach()
    dE, db, dW = torch.autograd.grad(C, (E, b, W), G.detach().cpu().double())
    return C.detach(), dE, db, dW


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
