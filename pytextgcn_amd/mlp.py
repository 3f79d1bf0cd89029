"""The middle of the reference's MLP as one product per layer (libtgcn.so `tgcn_mlp_act_linear*`, pytextgcn_amd/csrc/mlp.hip):
`dropout(selu(Z + b)) @ W.t() + c` of textgcn/lib/models.py:95-100 without the activated N x k matrix.  Z [N, k] is the
previous Linear's product WITHOUT its bias b, W [n, k] the next `nn.Linear`'s weight in torch's (out, in) layout, c its
bias.  The kernels form s * keep * selu(Z[i, j] + b[j]) in registers on the way into the matrix cores, in the forward
product and again (same mask, regenerated from an 8-byte seed) in the weight gradient.  The backward holds dZ -- the
gradient that the previous layer needs -- and nothing else of that size."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .dense import _check_seed, new_seed
from .plan import _stream_ptr, alloc_padded, colsum


def _require_on_gpu(what: str, Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], note: str = "") -> None:
    """libtgcn.so only: anything else is an error, never a silent fallback."""
    for name, t in (("Z", Z), ("b", b), ("W", W), ("c", c)):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"pytextgcn_amd: the {what} MLP product needs `{name}` on an AMD GPU (it lives on "
                               f"{t.device}); there is no CPU fallback")
        if t.dtype != torch.float32:
            raise TypeError(f"pytextgcn_amd: the {what} MLP product takes float32 operands, `{name}` is {t.dtype}{note}")


def _require(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor] = None) -> None:
    _require_on_gpu("fused", Z, b, W, c, " (the reference casts the model with .float(), MLP_flat.py)")
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


# ---------------------------------------------------------------------------------------------------------------------
# The product with an optional bias that depends on the ROW (libtgcn.so `tgcn_mlp_act_linear_cls*`): the one-hot class
# columns that MLP_level.py appends to its features, as rows of a table T [Fh, k] picked by ids cls [N, S] (S = 1 or 2).
# The pre-activation is ((Z + T[cls[:, 0]]) + T[cls[:, 1]]) + b; an id outside [0, Fh) selects nothing.  One forward, one
# backward and one autograd Function serve both forms: `term` is None or (cls, T), as the library's one nullable ClassTerm.
# ---------------------------------------------------------------------------------------------------------------------
MAX_CLASS_SLOTS = 2


def max_class_rows() -> int:
    """The cap on the rows of T (`tgcn_hier_max_features`, 128)."""
    return int(_lib.load().tgcn_hier_max_features())


def _require_cls(Z: Tensor, cls: Tensor, T: Tensor) -> None:
    if not cls.is_cuda or not T.is_cuda:
        raise RuntimeError("pytextgcn_amd: the fused MLP product needs `cls` and `T` on an AMD GPU; there is no CPU fallback")
    if cls.dtype != torch.int32 or T.dtype != torch.float32:
        raise TypeError(f"act_linear_cls: `cls` must be int32 and `T` float32 (got {cls.dtype}, {T.dtype})")
    if cls.dim() != 2 or T.dim() != 2 or cls.size(0) != Z.size(0) or T.size(1) != Z.size(1) \
            or not 1 <= cls.size(1) <= MAX_CLASS_SLOTS or not 1 <= T.size(0) <= max_class_rows():
        raise ValueError(f"act_linear_cls: cls {tuple(cls.shape)} (N, S in 1..{MAX_CLASS_SLOTS}) and T {tuple(T.shape)} "
                         f"(Fh in 1..{max_class_rows()}, k) do not fit Z {tuple(Z.shape)} (N, k)")


def _class_args(Z: Tensor, term):
    """(cls, T) checked against Z, with unit column strides, and the six arguments that describe them; `term` None: none."""
    if term is None:
        return None, ()
    _require_cls(Z, *term)
    cls, T = _unit_cols(term[0]), _unit_cols(term[1])
    S, (Fh, k) = cls.size(1), T.shape
    return (cls, T), (cls.data_ptr(), max(cls.stride(0), S), S, T.data_ptr(), max(T.stride(0), k), Fh)


def _forward(Z: Tensor, b: Tensor, W: Tensor, term, c: Optional[Tensor], p: float, seed: Optional[Tensor],
             out: Optional[Tensor], mask_row0: int) -> Tensor:
    lib = _lib.load()
    term, term_args = _class_args(Z, term)         # (`term` keeps the unit-stride copies alive over the call)
    Z, W, b = _unit_cols(Z), _unit_cols(W), b.contiguous()
    N, k = Z.shape
    n = W.size(0)
    C = alloc_padded(N, n, Z.device) if out is None else out
    fn = lib.tgcn_mlp_act_linear if term is None else lib.tgcn_mlp_act_linear_cls
    _lib.check(fn(Z.data_ptr(), max(Z.stride(0), k), *term_args, b.data_ptr(), W.data_ptr(), max(W.stride(0), k),
                  c.contiguous().data_ptr() if c is not None else None, C.data_ptr(), max(C.stride(0), n), N, k, n, float(p),
                  _seed_ptr(seed, Z.device), int(mask_row0), _stream_ptr(Z.device)))
    return C


def _backward(Z: Tensor, b: Tensor, W: Tensor, term, G: Tensor, p: float, seed: Optional[Tensor], want_z: bool, want_w: bool,
              want_t: bool, mask_row0: int):
    """(dZ, db, dW, dT); dT comes with dZ: `want_t` implies `want_z`."""
    want_z = want_z or want_t
    if not (want_z or want_w):
        return None, None, None, None
    lib = _lib.load()
    term, term_args = _class_args(Z, term)
    Z, W, b, G = _unit_cols(Z), _unit_cols(W), b.contiguous(), _unit_cols(G)
    N, k = Z.shape
    n = W.size(0)
    dev = Z.device
    dZ = alloc_padded(N, k, dev) if want_z else None
    db = torch.empty(k, dtype=torch.float32, device=dev) if want_z else None
    dT = torch.empty(term[1].size(0), k, dtype=torch.float32, device=dev) if want_t else None
    dW = torch.empty(n, k, dtype=torch.float32, device=dev) if want_w else None
    if term is None:
        fn, t_args, ws_bytes = lib.tgcn_mlp_act_linear_grad, (), lib.tgcn_mlp_act_linear_grad_workspace_bytes(N, k, n)
    else:
        fn, t_args = lib.tgcn_mlp_act_linear_cls_grad, (dT.data_ptr() if want_t else None, k)
        ws_bytes = lib.tgcn_mlp_act_linear_cls_grad_workspace_bytes(N, k, n, term[1].size(0))
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    _lib.check(fn(Z.data_ptr(), max(Z.stride(0), k), *term_args, b.data_ptr(), W.data_ptr(), max(W.stride(0), k), G.data_ptr(),
                  max(G.stride(0), n), dZ.data_ptr() if want_z else None, max(dZ.stride(0), k) if want_z else k,
                  db.data_ptr() if want_z else None, *t_args, dW.data_ptr() if want_w else None, k, N, k, n, float(p),
                  _seed_ptr(seed, dev), int(mask_row0), ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return dZ, db, dW, dT


class _ActLinear(torch.autograd.Function):
    """Saves Z, b, W, the class term (when there is one) and the seed; the activation is recomputed where it is needed."""

    @staticmethod
    def forward(ctx, Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], cls: Optional[Tensor], T: Optional[Tensor],
                p: float, seed: Optional[Tensor]):
        ctx.p = p
        ctx.has_term, ctx.has_seed = cls is not None, seed is not None
        ctx.save_for_backward(Z, b, W, *([cls, T] if ctx.has_term else []), *([seed] if ctx.has_seed else []))
        term = (cls, T.detach()) if ctx.has_term else None
        return _forward(Z.detach(), b.detach(), W.detach(), term, None if c is None else c.detach(), p, seed, None, 0)

    @staticmethod
    def backward(ctx, G: Tensor):
        saved = list(ctx.saved_tensors)
        seed = saved.pop() if ctx.has_seed else None
        Z, b, W = saved[:3]
        term = tuple(saved[3:5]) if ctx.has_term else None
        need = ctx.needs_input_grad
        dZ, db, dW, dT = _backward(Z, b, W, term, G, ctx.p, seed, need[0] or need[1], need[2], need[5], 0)
        dc = colsum(G) if need[3] else None
        return (dZ if need[0] else None), (db if need[1] else None), dW, dc, None, dT, None, None


def _apply(name: str, Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], term, p: float, seed: Optional[Tensor]) -> Tensor:
    _require(Z, b, W, c)
    if term is not None:
        _require_cls(Z, *term)
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}: dropout rate {p} outside [0, 1)")
    if p == 0.0:
        seed = None
    elif seed is None:
        seed = new_seed(Z.device)
    return _ActLinear.apply(Z, b, W, c, *(term or (None, None)), p, seed)


def act_linear_forward(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor] = None, p: float = 0.0,
                       seed: Optional[Tensor] = None, out: Optional[Tensor] = None, mask_row0: int = 0) -> Tensor:
    """C [N, n] = dropout(selu(Z + b), p) @ W.t() (+ c); `seed` None (or p = 0): no mask.  No autograd."""
    return _forward(Z, b, W, None, c, p, seed, out, mask_row0)


def act_linear_backward(Z: Tensor, b: Tensor, W: Tensor, G: Tensor, p: float = 0.0, seed: Optional[Tensor] = None,
                        want_z: bool = True, want_w: bool = True, mask_row0: int = 0):
    """(dZ, db, dW) of `act_linear_forward` for G = dC; a pair that is not wanted comes back as None."""
    return _backward(Z, b, W, None, G, p, seed, want_z, want_w, False, mask_row0)[:3]


def act_linear(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor] = None, p: float = 0.0,
               seed: Optional[Tensor] = None) -> Tensor:
    """dropout(selu(Z + b), p) @ W.t() (+ c) with gradients for Z [N, k], b [k], W [n, k] and c [n].  p > 0 is
    training-mode inverted dropout whose mask is a stateless hash of (seed, row, column) -- the library's random stream,
    not torch's; `seed` None draws one from torch's generator on the device (`dense.new_seed`)."""
    return _apply("act_linear", Z, b, W, c, None, p, seed)


def act_linear_cls_forward(Z: Tensor, b: Tensor, W: Tensor, cls: Tensor, T: Tensor, c: Optional[Tensor] = None,
                           p: float = 0.0, seed: Optional[Tensor] = None, out: Optional[Tensor] = None,
                           mask_row0: int = 0) -> Tensor:
    """C [N, n] = dropout(selu(Z + T[cls[:, 0]] (+ T[cls[:, 1]]) + b), p) @ W.t() (+ c).  No autograd."""
    return _forward(Z, b, W, (cls, T), c, p, seed, out, mask_row0)


def act_linear_cls_backward(Z: Tensor, b: Tensor, W: Tensor, cls: Tensor, T: Tensor, G: Tensor, p: float = 0.0,
                            seed: Optional[Tensor] = None, want_z: bool = True, want_w: bool = True, want_t: bool = True,
                            mask_row0: int = 0):
    """(dZ, db, dW, dT) of `act_linear_cls_forward` for G = dC; what is not wanted comes back as None.  dT [Fh, k] is the
    sum of dZ's rows per id (zero for a row of T that no id selects) and comes with dZ: `want_t` implies `want_z`."""
    return _backward(Z, b, W, (cls, T), G, p, seed, want_z, want_w, want_t, mask_row0)


def act_linear_cls(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], cls: Tensor, T: Tensor, p: float = 0.0,
                   seed: Optional[Tensor] = None) -> Tensor:
    """`act_linear` on the pre-activation `Z + T[cls[:, 0]] (+ T[cls[:, 1]]) + b`, with gradients for Z [N, k], b [k],
    W [n, k], c [n] and T [Fh, k].  `cls` is int32 [N, 1] or [N, 2]; an id outside [0, Fh) selects nothing.  Dropout as in
    `act_linear`."""
    return _apply("act_linear_cls", Z, b, W, c, (cls, T), p, seed)


# ---------------------------------------------------------------------------------------------------------------------
# The same product with a weight per GROUP of rows (libtgcn.so `tgcn_mlp_grouped_*`, pytextgcn_amd/csrc/mlp_grouped.hip):
# the K per-label MLPs of MLP_label.py as one network (pytextgcn_amd.perlabel.PerLabelMLP).
# ---------------------------------------------------------------------------------------------------------------------
class GroupedLayout:
    """What the grouped products read besides their operands: the rows [row_ptr[g], row_ptr[g + 1]) of group g use rows
    [w_row0[g], w_row0[g] + n[g]) of the stacked weight W [w_rows, k], entries [b_off[g], b_off[g] + k) of the stacked bias
    b [b_len] and columns [col0[g], col0[g] + n[g]) of the result C [N, c_cols].  Built and validated on the HOST by
    `tgcn_mlp_grouped_layout` (a ValueError names what does not fit; no GPU is touched); `host` is the blob as a uint8
    array, `dev` its copy on `device` (None: host only, for inspection), uploaded once."""

    HEADER = ("magic", "bytes", "K", "N", "k", "w_rows", "c_cols", "b_len", "n_max", "n_tiles", "n_slices",
              "chunks_per_slice")
    GROUP = np.dtype([("row0", "<i8"), ("rows", "<i8"), ("w_row0", "<i4"), ("n", "<i4"), ("col0", "<i4"), ("b_off", "<i4"),
                      ("tile0", "<i4"), ("n_tiles", "<i4"), ("slice0", "<i4"), ("n_slices", "<i4")])
    TILE = np.dtype([("row0", "<i8"), ("group", "<i4"), ("count", "<i4")])
    SLICE = np.dtype([("row0", "<i8"), ("row_end", "<i8"), ("group", "<i4"), ("pad", "<i4")])

    def __init__(self, row_ptr: Sequence[int], w_row0: Sequence[int], n: Sequence[int], col0: Sequence[int],
                 b_off: Sequence[int], N: int, k: int, w_rows: int, c_cols: int, b_len: int, device=None):
        lib = _lib.load()
        K = len(row_ptr) - 1
        rp = np.ascontiguousarray(np.asarray(row_ptr, dtype=np.int64))
        args = [np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (w_row0, n, col0, b_off)]
        if any(a.shape != (K,) for a in args):
            raise ValueError(f"GroupedLayout: w_row0, n, col0 and b_off need one entry per group (K = {K})")
        size = lib.tgcn_mlp_grouped_layout_bytes(K, rp.ctypes.data) if 1 <= K else 0
        self.host = np.zeros(max(size, 8), dtype=np.uint8)
        _lib.check(lib.tgcn_mlp_grouped_layout(K, rp.ctypes.data, *[a.ctypes.data for a in args], int(N), int(k), int(w_rows),
                                               int(c_cols), int(b_len), self.host.ctypes.data, size))
        self.header = dict(zip(self.HEADER, np.frombuffer(self.host, dtype="<i8", count=len(self.HEADER)).tolist()))
        self.K, self.N, self.k, self.w_rows, self.c_cols = K, int(N), int(k), int(w_rows), int(c_cols)
        self.n_routed = int(rp[K])
        # every element of C [N, c_cols] is written: the result needs no zero fill
        self.covers = self.n_routed == int(N) and all(int(c) == 0 for c in args[2]) and all(int(m) == c_cols for m in args[1])
        self.dev = None if device is None else torch.from_numpy(self.host).to(device)

    def tables(self):
        """(groups, tiles, slices) of the blob as numpy record arrays (views of `host`)."""
        h, at = self.header, 8 * len(self.HEADER)
        groups = np.frombuffer(self.host, dtype=self.GROUP, count=h["K"], offset=at)
        at += self.GROUP.itemsize * h["K"]
        tiles = np.frombuffer(self.host, dtype=self.TILE, count=h["n_tiles"], offset=at)
        at += self.TILE.itemsize * h["n_tiles"]
        return groups, tiles, np.frombuffer(self.host, dtype=self.SLICE, count=h["n_slices"], offset=at)


def _require_grouped(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], layout: GroupedLayout) -> None:
    _require_on_gpu("grouped", Z, b, W, c)
    if not isinstance(layout, GroupedLayout) or layout.dev is None or layout.dev.device != Z.device:
        raise ValueError("grouped_act_linear: `layout` must be a GroupedLayout uploaded to the operands' device")
    if Z.dim() != 2 or W.dim() != 2 or b.dim() != 1 or Z.shape != (layout.N, layout.k) or W.shape != (layout.w_rows, layout.k) \
            or b.size(0) != layout.header["b_len"] or (c is not None and c.shape != (layout.c_cols,)):
        raise ValueError(f"grouped_act_linear: Z {tuple(Z.shape)}, b {tuple(b.shape)}, W {tuple(W.shape)}"
                         + (f", c {tuple(c.shape)}" if c is not None else "") + f" do not fit the layout (N {layout.N}, "
                         f"k {layout.k}, W rows {layout.w_rows}, b entries {layout.header['b_len']}, C columns {layout.c_cols})")


def grouped_act_linear_forward(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], layout: GroupedLayout, p: float = 0.0,
                               seed: Optional[Tensor] = None, out: Optional[Tensor] = None, mask_row0: int = 0) -> Tensor:
    """C [N, c_cols]: row i of group g holds `dropout(selu(Z[i] + b_g), p) @ W_g.t() (+ c_g)` in its group's columns;
    everything else of `out` keeps what it held (default: a new result, zero where nothing is written).  No autograd."""
    lib = _lib.load()
    _require_grouped(Z, b, W, c, layout)
    Z, W, b = _unit_cols(Z), _unit_cols(W), b.contiguous()
    N, k = Z.shape
    new = torch.empty if layout.covers else torch.zeros
    C = new(N, layout.c_cols, dtype=torch.float32, device=Z.device) if out is None else out
    if C.dim() != 2 or C.size(0) != N or C.size(1) != layout.c_cols or (N and C.stride(1) != 1) or not C.is_cuda \
            or C.dtype != torch.float32:
        raise ValueError(f"grouped_act_linear: `out` must be a float32 [N, {layout.c_cols}] tensor with unit column stride")
    _lib.check(lib.tgcn_mlp_grouped_act_linear(Z.data_ptr(), max(Z.stride(0), k), b.data_ptr(), W.data_ptr(),
                                               max(W.stride(0), k), c.contiguous().data_ptr() if c is not None else None,
                                               C.data_ptr(), max(C.stride(0), layout.c_cols), N, k,
                                               layout.host.ctypes.data, layout.dev.data_ptr(), float(p),
                                               _seed_ptr(seed, Z.device), int(mask_row0), _stream_ptr(Z.device)))
    return C


def grouped_act_linear_backward(Z: Tensor, b: Tensor, W: Tensor, G: Tensor, layout: GroupedLayout, p: float = 0.0,
                                seed: Optional[Tensor] = None, want_z: bool = True, want_w: bool = True,
                                want_c: bool = False, mask_row0: int = 0, out=None):
    """(dZ, db, dW, dc) of `grouped_act_linear_forward` for G = dC [N, c_cols] (only the rows' own segments are read);
    what is not wanted comes back as None.  dZ [N, k] is zero on rows without a group, db and dW have the stacked layouts
    of b and W (rows of W that belong to no group: zero), dc [c_cols] is the gradient of c.  `out`: (dZ, db, dW, dc)
    buffers to write into instead (elements outside the groups' ranges keep what they hold)."""
    if not (want_z or want_w or want_c):
        return None, None, None, None
    lib = _lib.load()
    _require_grouped(Z, b, W, None, layout)
    if not G.is_cuda or G.dtype != torch.float32 or G.dim() != 2 or G.shape != (Z.size(0), layout.c_cols):
        raise ValueError(f"grouped_act_linear: G must be a float32 [N, {layout.c_cols}] tensor on the GPU")
    Z, W, b, G = _unit_cols(Z), _unit_cols(W), b.contiguous(), _unit_cols(G)
    N, k = Z.shape
    dev = Z.device
    if out is not None:
        dZ, db, dW, dc = out
    else:
        new = torch.empty if layout.n_routed == N else torch.zeros
        dZ = new(N, k, dtype=torch.float32, device=dev) if want_z else None
        db = torch.empty(b.size(0), dtype=torch.float32, device=dev) if want_z else None
        dW = torch.zeros(W.size(0), k, dtype=torch.float32, device=dev) if want_w else None
        dc = torch.zeros(layout.c_cols, dtype=torch.float32, device=dev) if want_c else None
    ws = torch.empty(max(lib.tgcn_mlp_grouped_act_linear_grad_workspace_bytes(layout.host.ctypes.data), 16),
                     dtype=torch.uint8, device=dev)
    _lib.check(lib.tgcn_mlp_grouped_act_linear_grad(
        Z.data_ptr(), max(Z.stride(0), k), b.data_ptr(), W.data_ptr(), max(W.stride(0), k), G.data_ptr(),
        max(G.stride(0), layout.c_cols), dZ.data_ptr() if want_z else None, max(dZ.stride(0), k) if want_z else k,
        db.data_ptr() if want_z else None, dW.data_ptr() if want_w else None, max(dW.stride(0), k) if want_w else k,
        dc.data_ptr() if want_c else None, N, k, layout.host.ctypes.data, layout.dev.data_ptr(), float(p),
        _seed_ptr(seed, dev), int(mask_row0), ws.data_ptr(), ws.numel(), _stream_ptr(dev)))
    return dZ, db, dW, dc


class _GroupedActLinear(torch.autograd.Function):
    """Saves Z, b, W and the seed, like `_ActLinear`."""

    @staticmethod
    def forward(ctx, Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], layout: GroupedLayout, p: float,
                seed: Optional[Tensor]):
        ctx.p, ctx.layout = p, layout
        ctx.has_seed = seed is not None
        ctx.save_for_backward(Z, b, W, *([seed] if seed is not None else []))
        return grouped_act_linear_forward(Z.detach(), b.detach(), W.detach(), None if c is None else c.detach(), layout, p,
                                          seed)

    @staticmethod
    def backward(ctx, G: Tensor):
        Z, b, W = ctx.saved_tensors[:3]
        seed = ctx.saved_tensors[3] if ctx.has_seed else None
        need = ctx.needs_input_grad
        dZ, db, dW, dc = grouped_act_linear_backward(Z, b, W, G, ctx.layout, ctx.p, seed, want_z=need[0] or need[1],
                                                     want_w=need[2], want_c=need[3])
        return (dZ if need[0] else None), (db if need[1] else None), dW, dc, None, None, None


def grouped_act_linear(Z: Tensor, b: Tensor, W: Tensor, c: Optional[Tensor], layout: GroupedLayout, p: float = 0.0,
                       seed: Optional[Tensor] = None) -> Tensor:
    """`act_linear` with the weight, the biases and the result columns of the row's group (`GroupedLayout`), with gradients
    for Z [N, k], b, W and c in their stacked layouts.  The mask row of row i is i, its index in grouped order, so group
    g's slice equals `act_linear` on `Z[row_ptr[g]:row_ptr[g + 1]]` under the same seed with `mask_row0 = row_ptr[g]`."""
    _require_grouped(Z, b, W, c, layout)
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"grouped_act_linear: dropout rate {p} outside [0, 1)")
    if p == 0.0:
        seed = None
    elif seed is None:
        seed = new_seed(Z.device)
    return _GroupedActLinear.apply(Z, b, W, c, layout, p, seed)
