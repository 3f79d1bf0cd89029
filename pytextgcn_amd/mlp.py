"""The middle of the reference's MLP as one product per layer (libtgcn.so `tgcn_mlp_act_linear*`, pytextgcn_amd/csrc/mlp.hip):
`dropout(selu(Z + b)) @ W.t() + c` of textgcn/lib/models.py:95-100 without the activated N x k matrix.  Z [N, k] is the
previous Linear's product WITHOUT its bias b, W [n, k] the next `nn.Linear`'s weight in torch's (out, in) layout, c its
bias.  The kernels form s * keep * selu(Z[i, j] + b[j]) in registers on the way into the matrix cores, in the forward
product and again (same mask, regenerated from an 8-byte seed) in the weight gradient.  The backward holds dZ -- the
gradient that the previous layer needs -- and nothing else of that size."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .dense import _check_seed, new_seed
from .plan import _stream_ptr, alloc_padded, colsum


def _require(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor] = None) -> None:
    """libtgcn.so only: anything else is an error, never a silent fallback."""
    for name, t in (("Z", Z), ("b", b), ("W", W), ("c", c)):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"pytextgcn_amd: the fused MLP product needs `{name}` on an AMD GPU (it lives on "
                               f"{t.device}); there is no CPU fallback")
        if t.dtype != torch.float32:
            raise TypeError(f"pytextgcn_amd: the fused MLP product takes float32 operands, `{name}` is {t.dtype} "
                            "(the reference casts the model with .float(), MLP_flat.py)")
    if Z.dim() != 2 or W.dim() != 2 or b.dim() != 1 or Z.size(1) != b.size(0) or Z.size(1) != W.size(1) \
            or Z.size(1) == 0 or W.size(0) == 0 or (c is not None and (c.dim() != 1 or c.size(0) != W.size(0))):
        raise ValueError(f"act_linear: Z {tuple(Z.shape)} (N, k), b {tuple(b.shape)}, W {tuple(W.shape)} (n, k)"
                         + (f" and c {tuple(c.shape)}" if c is not None else "") + " do not fit")


def _unit_cols(t: Tensor) -> Tensor:
    return t if (t.stride(1) == 1 and t.stride(0) >= t.size(1)) else t.contiguous()


def _seed_ptr(seed: Optional[Tensor], dev):
    if seed is None:
        return None
    _check_seed(seed, dev)
    return seed.data_ptr()


def act_linear_forward(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor] = None, p: float = 0.0,
                       seed: Optional[Tensor] = None, out: Optional[Tensor] = None, mask_row0: int = 0) -> Tensor:
    """C [N, n] = dropout(selu(Z + b), p) @ W.t() (+ c); `seed` None (or p = 0): no mask.  No autograd."""
    lib = _lib.load()
    Z, W, b = _unit_cols(Z), _unit_cols(W), b.contiguous()
    N, k = Z.shape
    n = W.size(0)
    C = alloc_padded(N, n, Z.device) if out is None else out
    _lib.check(lib.tgcn_mlp_act_linear(Z.data_ptr(), max(Z.stride(0), k), b.data_ptr(), W.data_ptr(), max(W.stride(0), k),
                                       c.contiguous().data_ptr() if c is not None else None, C.data_ptr(),
                                       max(C.stride(0), n), N, k, n, float(p), _seed_ptr(seed, Z.device), int(mask_row0),
                                       _stream_ptr(Z.device)))
    return C


def act_linear_backward(Z: Tensor, b: Tensor, W: Tensor, G: Tensor, p: float = 0.0, seed: Optional[Tensor] = None,
                        want_z: bool = True, want_w: bool = True, mask_row0: int = 0):
    """(dZ, db, dW) of `act_linear_forward` for G = dC; a pair that is not wanted comes back as None."""
    if not (want_z or want_w):
        return None, None, None
    lib = _lib.load()
    Z, W, b, G = _unit_cols(Z), _unit_cols(W), b.contiguous(), _unit_cols(G)
    N, k = Z.shape
    n = W.size(0)
    dZ = alloc_padded(N, k, Z.device) if want_z else None
    db = torch.empty(k, dtype=torch.float32, device=Z.device) if want_z else None
    dW = torch.empty(n, k, dtype=torch.float32, device=Z.device) if want_w else None
    ws = torch.empty(max(lib.tgcn_mlp_act_linear_grad_workspace_bytes(N, k, n), 16), dtype=torch.uint8, device=Z.device)
    _lib.check(lib.tgcn_mlp_act_linear_grad(Z.data_ptr(), max(Z.stride(0), k), b.data_ptr(), W.data_ptr(),
                                            max(W.stride(0), k), G.data_ptr(), max(G.stride(0), n),
                                            dZ.data_ptr() if want_z else None, max(dZ.stride(0), k) if want_z else k,
                                            db.data_ptr() if want_z else None, dW.data_ptr() if want_w else None, k, N, k,
                                            n, float(p), _seed_ptr(seed, Z.device), int(mask_row0), ws.data_ptr(),
                                            ws.numel(), _stream_ptr(Z.device)))
    return dZ, db, dW


class _ActLinear(torch.autograd.Function):
    """Saves Z, b, W and the seed; the activation is recomputed where it is needed."""

    @staticmethod
    def forward(ctx, Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], p: float, seed: Optional[Tensor]):
        ctx.p = p
        ctx.has_seed = seed is not None
        ctx.save_for_backward(Z, b, W, *([seed] if seed is not None else []))
        return act_linear_forward(Z.detach(), b.detach(), W.detach(), None if c is None else c.detach(), p, seed)

    @staticmethod
    def backward(ctx, G: Tensor):
        Z, b, W = ctx.saved_tensors[:3]
        seed = ctx.saved_tensors[3] if ctx.has_seed else None
        need = ctx.needs_input_grad
        dZ, db, dW = act_linear_backward(Z, b, W, G, ctx.p, seed, want_z=need[0] or need[1], want_w=need[2])
        dc = colsum(G) if need[3] else None
        return (dZ if need[0] else None), (db if need[1] else None), dW, dc, None, None


def act_linear(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor] = None, p: float = 0.0,
               seed: Optional[Tensor] = None) -> Tensor:
    """dropout(selu(Z + b), p) @ W.t() (+ c) with gradients for Z [N, k], b [k], W [n, k] and c [n].  p > 0 is
    training-mode inverted dropout whose mask is a stateless hash of (seed, row, column) -- the library's random stream,
    not torch's; `seed` None draws one from torch's generator on the device (`dense.new_seed`)."""
    _require(Z, b, W, c)
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"act_linear: dropout rate {p} outside [0, 1)")
    if p == 0.0:
        seed = None
    elif seed is None:
        seed = new_seed(Z.device)
    return _ActLinear.apply(Z, b, W, c, p, seed)
