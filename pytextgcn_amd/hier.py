"""The hierarchy features [I_N | H] of the per-level scripts (perlevel_amazon.py:122,156; text2graph.py:226-246) as an
operand of their own (libtgcn.so `tgcn_hier_xw*`, pytextgcn_amd/csrc/hier.hip).

The scripts train the level-2 `GCN` on the one-hot of the documents' top label and test it on the softmax of the level-1
logits.  Either way H is zero on the word rows and has one short dense row per document, and with Wh = W1[N:]

    X @ W1 = W1[:N] + H @ Wh.

`HierarchyFeatures` holds H the way it arises -- the class ids, or the dense rows on the device -- and stands in for the
sparse tensor as `g.x`; `xw` is the first layer's product on it: a row gather of Wh (one-hot) or a small dense product
(softmax) added to W1's rows in the pass that copies them, and in the backward ONE buffer of W1's shape whose first N
rows are the incoming gradient and whose last Fh rows are its per-class column sums (one-hot) or Hd^T @ G (dense, the
existing `tgcn_gemm_tn`).  H gets no gradient.  There is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib, dense
from .plan import _stream_ptr, alloc_padded


def max_features() -> int:
    """The widest hierarchy block the kernels take (`tgcn_hier_max_features`)."""
    return int(_lib.load().tgcn_hier_max_features())


class HierarchyFeatures:
    """The matrix [I_N | H], H [N, Fh] zero on the rows below `h_row0` (the word rows; `h_row0 = g.n_vocab`).  Exactly one
    of the two forms is given:

        classes   integer [N - h_row0]: H is the one-hot of these ids over `n_classes` columns (an id outside
                  [0, n_classes) leaves its row empty).  `n_classes` None: the largest id + 1.
        dense     float32 [N - h_row0, Fh]: the rows of H from h_row0 on.

    It exposes what the models ask of `g.x` (`shape`, `size`, `is_sparse`, `is_cuda`, `device`, `to`) and `to_sparse()`,
    the sparse COO tensor that `Text2GraphTransformer.node_feats(H)` builds, for every path that wants that."""

    is_sparse = False

    def __init__(self, n_nodes: int, h_row0: int, classes=None, dense=None, n_classes: Optional[int] = None):
        if (classes is None) == (dense is None):
            raise ValueError("HierarchyFeatures: give exactly one of `classes` and `dense`")
        n_nodes, h_row0 = int(n_nodes), int(h_row0)
        if not 0 <= h_row0 <= n_nodes:
            raise ValueError(f"HierarchyFeatures: h_row0 must be in [0, n_nodes] (h_row0={h_row0}, n_nodes={n_nodes})")
        self.n_nodes, self.h_row0 = n_nodes, h_row0
        self.classes = self.dense = None
        if classes is not None:
            classes = torch.as_tensor(classes)
            if classes.dim() != 1 or classes.dtype.is_floating_point or classes.dtype == torch.bool:
                raise TypeError("HierarchyFeatures: `classes` must be a 1-D integer tensor")
            if n_classes is None:
                n_classes = int(classes.max()) + 1 if classes.numel() else 1
            if int(n_classes) < 1:
                raise ValueError(f"HierarchyFeatures: n_classes must be >= 1 ({n_classes})")
            self.classes = classes.detach().to(torch.int32).contiguous()
            self.n_features = int(n_classes)
            rows = classes.numel()
        else:
            dense = torch.as_tensor(dense)
            if dense.dim() != 2 or dense.dtype != torch.float32 or dense.size(1) < 1:
                raise TypeError("HierarchyFeatures: `dense` must be a float32 [N - h_row0, Fh] tensor with Fh >= 1")
            self.dense = dense.detach()
            if self.dense.stride(1) != 1:
                self.dense = self.dense.contiguous()
            self.n_features = int(dense.size(1))
            rows = dense.size(0)
        if rows != n_nodes - h_row0:
            raise ValueError(f"HierarchyFeatures: {rows} rows given, the nodes h_row0 .. N - 1 are {n_nodes - h_row0}")
        self._sparse = None
        self._block = None

    n_classes = property(lambda self: self.n_features)

    @property
    def _held(self) -> Tensor:
        return self.classes if self.classes is not None else self.dense

    @property
    def shape(self) -> torch.Size:
        return torch.Size([self.n_nodes, self.n_nodes + self.n_features])

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self) -> int:
        return 2

    @property
    def device(self) -> torch.device:
        return self._held.device

    @property
    def is_cuda(self) -> bool:
        return self._held.is_cuda

    @property
    def dtype(self) -> torch.dtype:
        return torch.float32

    def to(self, device, *args, **kwargs) -> "HierarchyFeatures":
        """The same features on `device` (itself when they already live there)."""
        held = self._held.to(device, *args, **kwargs)
        if held is self._held:
            return self
        if self.classes is not None:
            return HierarchyFeatures(self.n_nodes, self.h_row0, classes=held, n_classes=self.n_features)
        return HierarchyFeatures(self.n_nodes, self.h_row0, dense=held)

    def dense_block(self) -> Tensor:
        """The float32 rows [N - h_row0, Fh] of H from h_row0 on (class ids are densified once and kept)."""
        if self.dense is not None:
            return self.dense
        if self._block is None:
            ids = self.classes.long()
            ok = (ids >= 0) & (ids < self.n_features)
            block = torch.zeros(ids.numel(), self.n_features, dtype=torch.float32, device=ids.device)
            block[ok.nonzero().flatten(), ids[ok]] = 1.0
            self._block = block
        return self._block

    def to_sparse(self) -> Tensor:
        """The coalesced sparse COO [N, N + Fh] tensor `Text2GraphTransformer.node_feats(H)` returns, on this device; built
        once and kept, so the caches keyed by it (its split, its SpMM plan) are built once too."""
        if self._sparse is None:
            n, dev = self.n_nodes, self.device
            ar = torch.arange(n, device=dev)
            if self.classes is not None:
                ids = self.classes.long()
                r = ((ids >= 0) & (ids < self.n_features)).nonzero().flatten()
                c, v = ids[r], torch.ones(r.numel(), dtype=torch.float32, device=dev)
            else:
                nz = torch.nonzero(self.dense)
                r, c = nz[:, 0], nz[:, 1]
                v = self.dense[r, c]
            idx = torch.cat([torch.stack([ar, ar]), torch.stack([r + self.h_row0, c + n])], 1)
            val = torch.cat([torch.ones(n, dtype=torch.float32, device=dev), v])
            self._sparse = torch.sparse_coo_tensor(idx, val, size=(n, n + self.n_features), dtype=torch.float32).coalesce()
        return self._sparse

    def __repr__(self) -> str:
        form = "classes" if self.classes is not None else "dense"
        return f"HierarchyFeatures(n_nodes={self.n_nodes}, h_row0={self.h_row0}, {form}, Fh={self.n_features}, {self.device})"


def takes(feats: HierarchyFeatures, w: Tensor) -> bool:
    """Whether `xw(feats, w)` runs on the kernels: `w` is a row-major float32 matrix with N + Fh rows and H is no wider
    than `max_features()`.  Anything else (a transposed `nn.Linear` weight, a wider H) is the composition's."""
    return (w.dim() == 2 and w.size(0) == feats.size(1) and w.size(1) >= 1 and w.stride(1) == 1 and w.stride(0) >= w.size(1)
            and w.dtype == torch.float32 and feats.n_features <= max_features())


def _form(feats: HierarchyFeatures):
    if feats.classes is not None:
        return _lib.HIER_ONEHOT, feats.classes.data_ptr(), None, feats.n_features
    d = feats.dense
    return _lib.HIER_DENSE, None, d.data_ptr(), max(d.stride(0), feats.n_features)


def xw_forward(feats: HierarchyFeatures, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """C [N, F] = [I_N | H] @ w.  No autograd.  `out`: a float32 [N, F] buffer of the caller's with unit column stride."""
    N, F = feats.n_nodes, w.size(1)
    c = alloc_padded(N, F, w.device) if out is None else dense._check_out("hier.xw", out, N, F, w, False)
    form, cls, hd, ldh = _form(feats)
    _lib.check(_lib.load().tgcn_hier_xw(w.data_ptr(), w.stride(0), form, cls, hd, ldh, feats.h_row0, feats.n_features,
                                        c.data_ptr(), max(c.stride(0), F), N, F, _stream_ptr(w.device)))
    return c


def xw_backward(feats: HierarchyFeatures, g: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """dW [N + Fh, F] of `xw_forward` for g = dC: ONE buffer, its first N rows g and its last Fh rows H^T @ g."""
    lib = _lib.load()
    if g.stride(1) != 1 or (g.size(0) > 1 and g.stride(0) < g.size(1)):
        g = g.contiguous()
    N, Fh, h0, F = feats.n_nodes, feats.n_features, feats.h_row0, g.size(1)
    dw = torch.empty(N + Fh, F, dtype=torch.float32, device=g.device) if out is None \
        else dense._check_out("hier.xw_backward", out, N + Fh, F, g, False)
    form, cls, _, _ = _form(feats)
    ws = torch.empty(max(lib.tgcn_hier_xw_grad_workspace_bytes(N, F, Fh, h0, form), 16), dtype=torch.uint8, device=g.device)
    _lib.check(lib.tgcn_hier_xw_grad(g.data_ptr(), max(g.stride(0), F), form, cls, h0, Fh, dw.data_ptr(),
                                     max(dw.stride(0), F), N, F, ws.data_ptr(), ws.numel(), _stream_ptr(g.device)))
    if form == _lib.HIER_DENSE:
        if N > h0:
            dense.gemm_tn(feats.dense, g[h0:], out=dw[N:])      # Hd^T @ G[h_row0:], into the same buffer
        else:
            dw[N:].zero_()
    return dw


class _HierXW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats: HierarchyFeatures, w: Tensor):
        ctx.feats = feats
        return xw_forward(feats, w.detach())

    @staticmethod
    def backward(ctx, g: Tensor):
        return None, xw_backward(ctx.feats, g)


def xw(feats: HierarchyFeatures, w: Tensor) -> Tensor:
    """[I_N | H] @ w with the gradient of `w` [N + Fh, F] (row-major; `takes(feats, w)`).  The result is the leading part
    of a buffer with whole float4 rows, so the propagate step pads nothing."""
    if not isinstance(feats, HierarchyFeatures):
        raise TypeError("hier.xw: `feats` must be a HierarchyFeatures")
    if not w.is_cuda or feats.device != w.device:
        raise RuntimeError(f"pytextgcn_amd: the hierarchy product needs the features and `w` on one AMD GPU (they live on "
                           f"{feats.device} and {w.device}); there is no CPU fallback")
    if w.dtype != torch.float32:
        raise TypeError(f"pytextgcn_amd: the hierarchy product takes a float32 weight, `w` is {w.dtype} "
                        "(the reference casts the model with .float(), flat_amazon.py:85)")
    if not takes(feats, w):
        raise ValueError(f"hier.xw: w {tuple(w.shape)} (strides {tuple(w.stride())}) must be row-major with "
                         f"{feats.size(1)} rows, and Fh = {feats.n_features} at most {max_features()}")
    return _HierXW.apply(feats, w)
