"""The fused EGCN front end on [I_N | H] features (`tgcn_embed_xw_h*`) as plain tensor expressions in float64, for the
tests: the truth that the kernels are held to.  Test infrastructure; nothing under pytextgcn_amd/ imports this.

    z(i, k) = (E[k, i] + b[k]) + sum_f H[i, f] Eh[k, f]      (the nodes below h_row0 have no H term)
    a(i, k) = s * keep(i, k) * selu(z(i, k))
    C = a @ W,  and (dWeight, db, dW) by autograd, dWeight in the [K, N + Fh] layout of the one parameter [E | Eh]."""
import torch

from _egcn_ref import keep_matrix, rel_err  # noqa: F401 -- the mask of tests/_dropout_hash.py and BASELINE's measure


def full_h(Hd, h_row0, N):
    """[N, Fh]: the dense rows `Hd` from node `h_row0` on, zeros above."""
    H = torch.zeros(N, Hd.size(1), dtype=Hd.dtype)
    H[h_row0:] = Hd
    return H


def activation(weight, b, Hd, h_row0, keep=None, p=0.0):
    """a [N, K] in the dtype of `weight` [K, N + Fh]."""
    Fh = Hd.size(1)
    N = weight.size(1) - Fh
    z = weight[:, :N].t() + b
    if h_row0 < N:
        z = z + full_h(Hd.to(weight.dtype), h_row0, N) @ weight[:, N:].t()
    a = torch.selu(z)
    if keep is not None:
        a = a * keep.to(a.dtype) / (1.0 - p)
    return a


def truth(weight, b, Hd, h_row0, W, G=None, keep=None, p=0.0, dtype=torch.float64):
    """C and, given G = dC, (dWeight, db, dW); `dtype` float32 evaluates the same expressions in the kernels' precision."""
    weight, b, W = (t.detach().cpu().to(dtype).requires_grad_() for t in (weight, b, W))
    C = activation(weight, b, Hd.detach().cpu().to(dtype), h_row0, keep, p) @ W
    if G is None:
        return C.detach()
    dWeight, db, dW = torch.autograd.grad(C, (weight, b, W), G.detach().cpu().to(dtype))
    return C.detach(), dWeight, db, dW
