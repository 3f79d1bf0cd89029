"""The reference's MLP (textgcn/lib/models.py:83-102) restated for the tests from torch's `nn.Linear`, `nn.SELU` and
`nn.Dropout` -- and, for the kernel tests, the two entry points of pytextgcn_amd/csrc/mlp.hip as plain tensor expressions
in any dtype (float64 for the truth), with the dropout mask given as a boolean keep matrix built from
tests/_dropout_hash.py.  Test infrastructure; nothing under pytextgcn_amd/ imports this."""
import numpy as np
import torch
from torch import nn

import _dropout_hash as H


class MLPRef(nn.Module):
    def __init__(self, in_channels, out_channels, hidden, dropout=0.5):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        assert hidden
        sizes = [in_channels] + list(hidden) + [out_channels]
        self.layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(sizes, sizes[1:])])
        self.act = nn.SELU()

    def forward(self, x):
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            # nn.Linear on the (possibly sparse) features: x @ weight^T + bias
            x = (torch.sparse.mm(x, layer.weight.t()) if x.is_sparse else x @ layer.weight.t()) + layer.bias
            if i < last:
                x = self.dropout(self.act(x))
        return x


def keep_matrix(seed: int, N: int, k: int, p: float, row0: int = 0) -> torch.Tensor:
    """[N, k] bool: the kernels' keep decision for row i (mask row i + row0) and column j."""
    rows = (np.arange(N, dtype=np.uint64) + np.uint64(row0))[:, None]
    cols = np.arange(k, dtype=np.uint64)[None, :]
    return torch.from_numpy(np.asarray(H.keep_mask(seed, rows, cols, p)).reshape(N, k))


def activation(Z, b, keep=None, p=0.0):
    """a [N, k] = s * keep * selu(Z + b) in the dtype of Z."""
    a = torch.selu(Z + b)
    if keep is not None:
        a = a * keep.to(a.dtype) / (1.0 - p)
    return a


def act_linear(Z, b, W, c=None, keep=None, p=0.0):
    """C = a @ W^T (+ c) in the dtype of the operands."""
    C = activation(Z, b, keep, p) @ W.t()
    return C if c is None else C + c


def fused_truth(Z, b, W, c=None, G=None, keep=None, p=0.0, dtype=torch.float64):
    """C and, given G = dC, (dZ, db, dW, dc) by autograd through the expressions above, evaluated in `dtype`."""
    Z, b, W = (t.detach().cpu().to(dtype).requires_grad_() for t in (Z, b, W))
    c = None if c is None else c.detach().cpu().to(dtype).requires_grad_()
    C = act_linear(Z, b, W, c, keep, p)
    if G is None:
        return C.detach()
    if C.numel() == 0:
        return C.detach(), torch.zeros_like(Z), torch.zeros_like(b), torch.zeros_like(W), None if c is None else torch.zeros_like(c)
    grads = torch.autograd.grad(C, (Z, b, W) + (() if c is None else (c,)), G.detach().cpu().to(dtype))
    return (C.detach(),) + tuple(grads) + ((None,) if c is None else ())


def mlp_truth(params, x, keeps=None, p=0.0, dtype=torch.float64):
    """The whole network from the expressions above: `params` = [(W_0, b_0), ...] as leaf tensors of `dtype`, x a dense
    [N, in] tensor of `dtype`; keeps[i] the keep matrix after layer i (None: no dropout)."""
    W0, b0 = params[0]
    z = x @ W0.t()
    for i in range(1, len(params)):
        W, c = params[i]
        z = act_linear(z, params[i - 1][1], W, c if i == len(params) - 1 else None,
                       None if keeps is None else keeps[i - 1], p)
    return z


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
