"""The front end of EGCN on one-hot features as one product (libtgcn.so `tgcn_embed_xw*`, pytextgcn_amd/csrc/embed.hip):
`dropout(selu(Linear(I))) @ W` of textgcn/lib/models.py:43-47 without the N x embedding_dim activation.  With x = I the
Linear's output is `E.t() + b` for its weight E [K, N]; the kernels form s * keep * selu(E[k, i] + b[k]) in registers on
the way into the matrix cores, in the forward product and again (same mask, regenerated from an 8-byte seed) in the
weight gradient.  The backward holds dE -- one N x K matrix, the gradient of the parameter -- and nothing else of that size.

With [I_N | H] features (`h`, `h_row0`: the dense rows of the hierarchy block from `conv.dense_hierarchy_block`) the
Linear's weight is [K, N + Fh] and the pre-activation gains sum_f H[i, f] weight[k, N + f] on the rows i >= h_row0
(`tgcn_embed_xw_h*`); the weight's gradient is still ONE tensor of the weight's shape."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .dense import _check_seed, new_seed
from .plan import _stream_ptr, alloc_padded


def _require(E: Tensor, b: Tensor, W: Tensor) -> None:
    """libtgcn.so only: anything else is an error, never a silent fallback."""
    for name, t in (("E", E), ("b", b), ("W", W)):
        if not t.is_cuda:
            raise RuntimeError(f"pytextgcn_amd: the fused embedding product needs `{name}` on an AMD GPU (it lives on "
                               f"{t.device}); there is no CPU fallback")
        if t.dtype != torch.float32:
            raise TypeError(f"pytextgcn_amd: the fused embedding product takes float32 operands, `{name}` is {t.dtype} "
                            "(the reference casts the model with .float(), flat_amazon.py:85)")
    if E.dim() != 2 or W.dim() != 2 or b.dim() != 1 or E.size(0) != b.size(0) or E.size(0) != W.size(0) \
            or E.size(0) == 0 or W.size(1) == 0:
        raise ValueError(f"embed_xw: E {tuple(E.shape)} (embedding_dim, N), b {tuple(b.shape)} and W {tuple(W.shape)} "
                         "(embedding_dim, n) do not fit")


def _unit_cols(t: Tensor) -> Tensor:
    return t if (t.stride(1) == 1 and t.stride(0) >= t.size(1)) else t.contiguous()


def max_hierarchy_features() -> int:
    """The widest hierarchy block H that the fused product takes (`tgcn_embed_xw_h_max_features`)."""
    return int(_lib.load().tgcn_embed_xw_h_max_features())


def _require_h(E: Tensor, h: Tensor, h_row0: int) -> int:
    """Checks `h` [N - h_row0, Fh] against the weight E [K, N + Fh]; returns N."""
    if not h.is_cuda or h.device != E.device:
        raise RuntimeError(f"pytextgcn_amd: the fused embedding product needs `h` on the weight's AMD GPU (it lives on "
                           f"{h.device}); there is no CPU fallback")
    if h.dtype != torch.float32:
        raise TypeError(f"pytextgcn_amd: the fused embedding product takes float32 operands, `h` is {h.dtype}")
    if h.dim() != 2 or not 1 <= h.size(1) <= max_hierarchy_features():
        raise ValueError(f"embed_xw: h {tuple(h.shape)} must be [rows, Fh] with 1 <= Fh <= {max_hierarchy_features()}")
    N = E.size(1) - h.size(1)
    if N < 0 or not 0 <= h_row0 <= N or h.size(0) != N - h_row0:
        raise ValueError(f"embed_xw: h {tuple(h.shape)} with h_row0={h_row0} does not fit the weight {tuple(E.shape)} "
                         "(embedding_dim, N + Fh): it holds the rows h_row0 .. N - 1")
    return N


def embed_xw_forward(E: Tensor, b: Tensor, W: Tensor, p: float = 0.0, seed: Optional[Tensor] = None,
                     out: Optional[Tensor] = None, h: Optional[Tensor] = None, h_row0: int = 0) -> Tensor:
    """C [N, n] = dropout(selu(E.t() + b), p) @ W; `seed` None (or p = 0): no mask.  No autograd.  With `h` [N - h_row0,
    Fh], E is the whole [K, N + Fh] weight and the rows from h_row0 on gain h @ E[:, N:].t() before the SELU."""
    lib = _lib.load()
    E, W, b = _unit_cols(E), _unit_cols(W), b.contiguous()
    K, N = E.shape
    n = W.size(1)
    if seed is not None:
        _check_seed(seed, E.device)
    if h is not None:
        N = _require_h(E, h, h_row0)
        h = _unit_cols(h)
        Fh = h.size(1)
        c = alloc_padded(N, n, E.device) if out is None else out
        lde = max(E.stride(0), N + Fh)
        _lib.check(lib.tgcn_embed_xw_h(E.data_ptr(), lde, b.data_ptr(), E.data_ptr() + 4 * N, lde, h.data_ptr(),
                                       max(h.stride(0), Fh), h_row0, Fh, W.data_ptr(), W.stride(0), c.data_ptr(),
                                       max(c.stride(0), n), N, K, n, float(p), seed.data_ptr() if seed is not None else None,
                                       0, _stream_ptr(E.device)))
        return c
    c = alloc_padded(N, n, E.device) if out is None else out
    _lib.check(lib.tgcn_embed_xw(E.data_ptr(), max(E.stride(0), N), b.data_ptr(), W.data_ptr(), W.stride(0), c.data_ptr(),
                                 max(c.stride(0), n), N, K, n, float(p), seed.data_ptr() if seed is not None else None, 0,
                                 _stream_ptr(E.device)))
    return c


def embed_xw_backward(E: Tensor, b: Tensor, W: Tensor, G: Tensor, p: float = 0.0, seed: Optional[Tensor] = None,
                      want_e: bool = True, want_w: bool = True, h: Optional[Tensor] = None, h_row0: int = 0):
    """(dE, db, dW) of `embed_xw_forward` for G = dC; a pair that is not wanted comes back as None.  With `h`, dE is the
    gradient of the whole [K, N + Fh] weight: the kernels write its two column ranges in place."""
    lib = _lib.load()
    E, W, b, G = _unit_cols(E), _unit_cols(W), b.contiguous(), _unit_cols(G)
    K, N = E.shape
    n = W.size(1)
    if h is not None:
        N = _require_h(E, h, h_row0)
        if not (want_e or want_w):
            return None, None, None
        h = _unit_cols(h)
        Fh = h.size(1)
        dE = torch.empty(K, N + Fh, dtype=torch.float32, device=E.device) if want_e else None
        db = torch.empty(K, dtype=torch.float32, device=E.device) if want_e else None
        dW = torch.empty(K, n, dtype=torch.float32, device=E.device) if want_w else None
        ws = torch.empty(max(lib.tgcn_embed_xw_h_grad_workspace_bytes(N, K, n, Fh), 16), dtype=torch.uint8, device=E.device)
        if seed is not None:
            _check_seed(seed, E.device)
        lde = max(E.stride(0), N + Fh)
        _lib.check(lib.tgcn_embed_xw_h_grad(E.data_ptr(), lde, b.data_ptr(), E.data_ptr() + 4 * N, lde, h.data_ptr(),
                                            max(h.stride(0), Fh), h_row0, Fh, W.data_ptr(), W.stride(0), G.data_ptr(),
                                            max(G.stride(0), n), dE.data_ptr() if want_e else None, N + Fh,
                                            db.data_ptr() if want_e else None, dE.data_ptr() + 4 * N if want_e else None,
                                            N + Fh, dW.data_ptr() if want_w else None, n, N, K, n, float(p),
                                            seed.data_ptr() if seed is not None else None, 0, ws.data_ptr(), ws.numel(),
                                            _stream_ptr(E.device)))
        return dE, db, dW
    dE = torch.empty(K, N, dtype=torch.float32, device=E.device) if want_e else None
    db = torch.empty(K, dtype=torch.float32, device=E.device) if want_e else None
    dW = torch.empty(K, n, dtype=torch.float32, device=E.device) if want_w else None
    if not (want_e or want_w):
        return None, None, None
    ws_bytes = lib.tgcn_embed_xw_grad_workspace_bytes(N, K, n) if want_w else 0
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=E.device)
    if seed is not None:
        _check_seed(seed, E.device)
    _lib.check(lib.tgcn_embed_xw_grad(E.data_ptr(), max(E.stride(0), N), b.data_ptr(), W.data_ptr(), W.stride(0),
                                      G.data_ptr(), max(G.stride(0), n), dE.data_ptr() if want_e else None, N,
                                      db.data_ptr() if want_e else None, dW.data_ptr() if want_w else None, n, N, K, n,
                                      float(p), seed.data_ptr() if seed is not None else None, 0, ws.data_ptr(), ws.numel(),
                                      _stream_ptr(E.device)))
    return dE, db, dW


class _EmbedXW(torch.autograd.Function):
    """Saves the three parameters, the seed and (with [I | H] features) the dense rows of H; the activation is recomputed
    where it is needed."""

    @staticmethod
    def forward(ctx, E: Tensor, b: Tensor, W: Tensor, p: float, seed: Optional[Tensor], h: Optional[Tensor], h_row0: int):
        ctx.p = p
        ctx.has_seed = seed is not None
        ctx.has_h = h is not None
        ctx.h_row0 = h_row0
        ctx.save_for_backward(E, b, W, *([seed] if seed is not None else []), *([h] if h is not None else []))
        return embed_xw_forward(E.detach(), b.detach(), W.detach(), p, seed, h=h, h_row0=h_row0)

    @staticmethod
    def backward(ctx, G: Tensor):
        E, b, W = ctx.saved_tensors[:3]
        seed = ctx.saved_tensors[3] if ctx.has_seed else None
        h = ctx.saved_tensors[-1] if ctx.has_h else None
        need = ctx.needs_input_grad
        dE, db, dW = embed_xw_backward(E, b, W, G, ctx.p, seed, want_e=need[0] or need[1], want_w=need[2], h=h,
                                       h_row0=ctx.h_row0)
        return (dE if need[0] else None), (db if need[1] else None), dW, None, None, None, None


def embed_xw(E: Tensor, b: Tensor, W: Tensor, p: float = 0.0, seed: Optional[Tensor] = None, h: Optional[Tensor] = None,
             h_row0: int = 0) -> Tensor:
    """dropout(selu(E.t() + b), p) @ W with gradients for E [K, N], b [K] and W [K, n].  p > 0 is training-mode inverted
    dropout whose mask is a stateless hash of (seed, node, column) -- the library's random stream, not torch's; `seed`
    None draws one from torch's generator on the device (`dense.new_seed`).

    `h` [N - h_row0, Fh] (float32, no gradient): [I_N | H] features.  E is then the whole [K, N + Fh] weight of the Linear,
    the nodes from `h_row0` on gain `h @ E[:, N:].t()` before the SELU, and E's gradient is one tensor of E's shape."""
    _require(E, b, W)
    if h is not None:
        _require_h(E, h, int(h_row0))
        h = h.detach()
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"embed_xw: dropout rate {p} outside [0, 1)")
    if p == 0.0:
        seed = None
    elif seed is None:
        seed = new_seed(E.device)
    return _EmbedXW.apply(E, b, W, p, seed, h, int(h_row0))


# ---------------------------------------------------------------------------------------------------------------------
# M members in one call (libtgcn.so `tgcn_embed_xw_members*`): the EGCN members of a sweep cell, `crossval.CrossValEGCN`.
# ---------------------------------------------------------------------------------------------------------------------
MAX_MEMBERS = 64


def _member_rates(p, M: int):
    rates = [float(p)] * M if isinstance(p, (int, float)) else [float(v) for v in p]
    if len(rates) != M:
        raise ValueError(f"embed_xw_members: {len(rates)} rates for {M} members")
    if not all(0.0 <= v < 1.0 for v in rates):
        raise ValueError(f"embed_xw_members: every member's rate must be in [0, 1), got {rates}")
    return tuple(rates)


def _members_call(E: Tensor, b: Tensor, W: Tensor, M: int, h: Optional[Tensor], h_row0: int):
    """(E, b, W, h, N, D, n, Fh, head): the operands as the kernels take them and the arguments the two calls share."""
    E, W, b = _unit_cols(E), _unit_cols(W), b.contiguous()
    D, n = E.size(0) // M, W.size(1)
    if h is not None:
        N = _require_h(E, h, h_row0)
        h = _unit_cols(h)
        Fh = h.size(1)
        lde = max(E.stride(0), N + Fh)
        hier = (E.data_ptr() + 4 * N, lde, h.data_ptr(), max(h.stride(0), Fh), h_row0, Fh)
    else:
        N, Fh = E.size(1), 0
        lde = max(E.stride(0), N)
        hier = (None, 0, None, 0, 0, 0)
    head = (E.data_ptr(), lde, b.data_ptr(), *hier, W.data_ptr(), W.stride(0))
    return E, b, W, h, N, D, n, Fh, head


def _rates_array(rates):
    return (ctypes.c_double * len(rates))(*rates)


def embed_xw_members_forward(E: Tensor, b: Tensor, W: Tensor, n_members: int, p=0.0, seeds: Optional[Tensor] = None,
                             out: Optional[Tensor] = None, h: Optional[Tensor] = None, h_row0: int = 0) -> Tensor:
    """C [N, M n]: member m's columns are `embed_xw_forward` of the rows [m D, (m + 1) D) of E, b and W with `p[m]` and
    `seeds[m]` (`seeds` None: no mask).  One launch per 256 columns of n, whatever M is.  No autograd."""
    lib = _lib.load()
    M = int(n_members)
    rates = _member_rates(p, M)
    E, b, W, h, N, D, n, Fh, head = _members_call(E, b, W, M, h, h_row0)
    c = alloc_padded(N, M * n, E.device) if out is None else out
    _lib.check(lib.tgcn_embed_xw_members(*head, c.data_ptr(), max(c.stride(0), M * n), N, D, n, M, _rates_array(rates),
                                         seeds.data_ptr() if seeds is not None else None, 0, _stream_ptr(E.device)))
    return c


def embed_xw_members_backward(E: Tensor, b: Tensor, W: Tensor, G: Tensor, n_members: int, p=0.0,
                              seeds: Optional[Tensor] = None, want_e: bool = True, want_w: bool = True,
                              h: Optional[Tensor] = None, h_row0: int = 0):
    """(dE, db, dW) of `embed_xw_members_forward` for G = dC [N, M n], stacked as E, b and W are; a pair that is not wanted
    comes back as None.  With `h`, dE is the gradient of the whole [M D, N + Fh] weight."""
    if not (want_e or want_w):
        return None, None, None
    lib = _lib.load()
    M = int(n_members)
    rates = _member_rates(p, M)
    E, b, W, h, N, D, n, Fh, head = _members_call(E, b, W, M, h, h_row0)
    G = _unit_cols(G)
    dev = E.device
    dE = torch.empty(M * D, N + Fh, dtype=torch.float32, device=dev) if want_e else None
    db = torch.empty(M * D, dtype=torch.float32, device=dev) if want_e else None
    dW = torch.empty(M * D, n, dtype=torch.float32, device=dev) if want_w else None
    ws = torch.empty(max(lib.tgcn_embed_xw_members_grad_workspace_bytes(N, D, n, Fh, M), 16), dtype=torch.uint8, device=dev)
    _lib.check(lib.tgcn_embed_xw_members_grad(
        *head, G.data_ptr(), max(G.stride(0), M * n), dE.data_ptr() if want_e else None, N + Fh,
        db.data_ptr() if want_e else None, dE.data_ptr() + 4 * N if want_e and Fh else None, N + Fh,
        dW.data_ptr() if want_w else None, n, N, D, n, M, _rates_array(rates),
        seeds.data_ptr() if seeds is not None else None, 0, ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return dE, db, dW


class _EmbedXWMembers(torch.autograd.Function):
    """`_EmbedXW` for M members: saves the stacked parameters, the seeds and the dense rows of H; the activation is
    recomputed where it is needed."""

    @staticmethod
    def forward(ctx, E: Tensor, b: Tensor, W: Tensor, M: int, rates, seeds: Optional[Tensor], h: Optional[Tensor],
                h_row0: int):
        ctx.M, ctx.rates, ctx.h_row0 = M, rates, h_row0
        ctx.has_seeds, ctx.has_h = seeds is not None, h is not None
        ctx.save_for_backward(E, b, W, *([seeds] if seeds is not None else []), *([h] if h is not None else []))
        return embed_xw_members_forward(E.detach(), b.detach(), W.detach(), M, rates, seeds, h=h, h_row0=h_row0)

    @staticmethod
    def backward(ctx, G: Tensor):
        E, b, W = ctx.saved_tensors[:3]
        seeds = ctx.saved_tensors[3] if ctx.has_seeds else None
        h = ctx.saved_tensors[-1] if ctx.has_h else None
        need = ctx.needs_input_grad
        dE, db, dW = embed_xw_members_backward(E, b, W, G, ctx.M, ctx.rates, seeds, want_e=need[0] or need[1],
                                               want_w=need[2], h=h, h_row0=ctx.h_row0)
        return (dE if need[0] else None), (db if need[1] else None), dW, None, None, None, None, None


def embed_xw_members(E: Tensor, b: Tensor, W: Tensor, n_members: int, p=0.0, seeds: Optional[Tensor] = None,
                     h: Optional[Tensor] = None, h_row0: int = 0) -> Tensor:
    """`embed_xw` for M = `n_members` networks of equal widths in one call, with gradients: E [M D, N] (with `h`:
    [M D, N + Fh]), b [M D] and W [M D, n] are stacked by rows, the result is [N, M n] and member m owns its columns
    [m n, (m + 1) n).  `p` is one rate or M rates in [0, 1) -- a member at rate 0 keeps everything -- and `seeds` an int64
    [M] device tensor, one seed of the library's random stream per member; None with some rate > 0 draws M fresh ones from
    torch's generator.  Member m's block of the result and of every gradient is bit for bit what `embed_xw` gives on the
    member's rows with `p[m]` and `seeds[m:m + 1]`."""
    _require(E, b, W)
    M = int(n_members)
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"embed_xw_members takes 1..{MAX_MEMBERS} members, got {n_members}")
    if E.size(0) % M:
        raise ValueError(f"embed_xw_members: the {E.size(0)} rows of E are not {M} equal blocks")
    if h is not None:
        _require_h(E, h, int(h_row0))
        h = h.detach()
    rates = _member_rates(p, M)
    if max(rates) == 0.0:
        seeds = None
    elif seeds is None:
        seeds = torch.empty(M, dtype=torch.int64, device=E.device).random_()
    elif seeds.dtype != torch.int64 or seeds.shape != (M,) or seeds.device != E.device or not seeds.is_contiguous():
        raise TypeError("embed_xw_members: seeds must be a contiguous int64 [M] tensor on the operands' device")
    return _EmbedXWMembers.apply(E, b, W, M, rates, seeds, h, int(h_row0))
