"""JumpingKnowledge (PyG 1.6.3 `torch_geometric.nn.JumpingKnowledge`), the aggregation step of the reference's
JumpingKnowledgeNetwork (textgcn/lib/models.py:64,75), on libtgcn.so (`tgcn_jk_*`, pytextgcn_amd/csrc/jk.hip).

Mode "lstm" is a bidirectional LSTM over the L per-layer activations of every node, a Linear on its outputs, a softmax over
the layers and a weighted sum of the activations.  Composed from library calls that stacks the activations into [N, L, C],
stores LSTM outputs [N, L, 2 H] and keeps N L 2 4H gate values for the backward.  Here

  * the forward is ONE kernel (`tgcn_jk_lstm_forward`): a wave carries 32 nodes through both directions and all L steps on
    the fp32 matrix cores and writes `out` [N, C] and `alpha` [N, L]; no gate, cell or hidden value reaches memory;
  * the backward recomputes them in chunks of `chunk_rows` rows from the L inputs (which the graph holds anyway) and
    `alpha`: the library's tall-skinny products around three pointwise kernels, a workspace proportional to `chunk_rows`
    and not to N, every sum in a fixed order (no atomics: two runs give the same bits);
  * the same chunked pieces run forward only are the composed path, `enable_fused_jk(False)`: the A/B baseline and the
    second implementation the tests hold the fused kernel against.

The gradient of `att.bias` is returned as exact zeros: the softmax over the layers is invariant to a shift common to all of
them, so the true gradient is identically zero (torch's autograd returns rounding noise there)."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch
from torch import Tensor, nn

from . import _lib, dense
from .plan import _stream_ptr, alloc_padded, colsum

MAX_LAYERS = 8                     # TGCN_JK_MAX_LAYERS of include/tgcn.h
DEFAULT_CHUNK_ROWS = 8192          # rows of one backward chunk: 2 L x 8192 x 6 H floats of workspace (75 MB at H = 200, L = 2)

# On by default: mode "lstm" forward as the one fused kernel.  Off: the composed path (module docstring).
_FUSED_JK = True


def enable_fused_jk(on: bool = True) -> bool:
    """Returns the previous setting."""
    global _FUSED_JK
    was, _FUSED_JK = _FUSED_JK, bool(on)
    return was


def _require(tensors: Sequence[Tensor], what: str) -> None:
    """libtgcn.so only: anything else is an error, never a silent fallback."""
    for t in tensors:
        if t.dtype != torch.float32:
            raise TypeError(f"pytextgcn_amd: JumpingKnowledge takes float32 operands, one of {what} is {t.dtype} "
                            "(the reference casts the model with .float(), flat_amazon.py:85)")
        if not t.is_cuda:
            raise RuntimeError(f"pytextgcn_amd: JumpingKnowledge needs {what} on an AMD GPU (one lives on {t.device}); "
                               "there is no CPU fallback")


def _unit_cols(t: Tensor) -> Tensor:
    return t if (t.stride(1) == 1 and (t.size(0) <= 1 or t.stride(0) >= t.size(1))) else t.contiguous()


def _ld(t: Tensor) -> int:
    return max(t.stride(0), t.size(1))


def _pointers(tensors: Sequence[Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _lds(tensors: Sequence[Tensor]):
    return (ctypes.c_int64 * len(tensors))(*[_ld(t) for t in tensors])


def _round_up4(v: int) -> int:
    return (v + 3) & ~3


def _aligned_rows(t: Tensor) -> Tensor:
    """`t` [r, C] as the A operand of tgcn_gemm_nn / _nt: a 16-byte aligned base and a row stride that is a multiple of 4
    (a copy of the chunk when the caller's tensor is neither)."""
    if t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= t.size(1) and t.data_ptr() % 16 == 0:
        return t
    buf = torch.empty(t.size(0), _round_up4(t.size(1)), dtype=t.dtype, device=t.device)[:, :t.size(1)]
    buf.copy_(t)
    return buf


def fused_forward_takes(H: int) -> bool:
    """Whether the fused kernel takes hidden width H (it keeps the cell state in registers: H <= 256)."""
    return bool(_lib.load().tgcn_jk_lstm_forward_supported(int(H)))


class _Workspace:
    """Everything the pieces store for one chunk of at most R rows.  `keep`: the gates and cells of every step stay (the
    backward reads them); without it one gate buffer serves all steps."""

    def __init__(self, R: int, L: int, C: int, H: int, dev, keep: bool):
        e = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)      # noqa: E731
        H4 = _round_up4(H)
        self.R, self.H4, self.keep = R, H4, keep
        self.gates = e(2, L if keep else 1, R, 4 * H)
        self.c = e(2, L, R, H4)
        self.h = e(2, L, R, H4)
        self.pre_h = e(R, 4 * H)
        if keep:
            self.dgates = e(L, R, 8 * H)          # [d gates fwd | d gates bwd] of step t: one product gives d x_t
            self.dc = e(R, H4)
            self.dh = e(R, H4)
            self.dscore = e(R, L)
            self.T = e(R, _round_up4(C))


def _mm(fn, a: Tensor, b: Tensor, out: Tensor, k: int, n: int) -> None:
    """out [r, n] = a [r, k] (x) b through tgcn_gemm_nn / tgcn_gemm_nt; `a` has 16-byte rows."""
    _lib.check(fn(a.data_ptr(), _ld(a), b.data_ptr(), b.stride(0), out.data_ptr(), _ld(out), a.size(0), k, n,
                  _stream_ptr(a.device)))


def _run_cells(lib, ws: _Workspace, xa: List[Tensor], params: List[Tensor], r: int, C: int, H: int) -> None:
    """Both directions of the LSTM over the chunk `xa` (L tensors [r, C] with 16-byte rows) into the workspace."""
    L, H4, stream = len(xa), ws.H4, _stream_ptr(xa[0].device)
    for d in (0, 1):
        wih, whh, bih, bhh = params[4 * d:4 * d + 4]
        prev = None
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            g = ws.gates[d, t if ws.keep else 0, :r]
            _mm(lib.tgcn_gemm_nt, xa[t], wih, g, C, 4 * H)
            if prev is not None:
                _mm(lib.tgcn_gemm_nt, ws.h[d, prev, :r, :H], whh, ws.pre_h[:r], H, 4 * H)
            _lib.check(lib.tgcn_jk_cell(g.data_ptr(), 4 * H, ws.pre_h.data_ptr() if prev is not None else None, 4 * H,
                                        bih.data_ptr(), bhh.data_ptr(),
                                        ws.c[d, prev].data_ptr() if prev is not None else None, H4, g.data_ptr(), 4 * H,
                                        ws.c[d, t].data_ptr(), H4, ws.h[d, t].data_ptr(), H4, r, H, stream))
            prev = t


def _chunks(N: int, chunk_rows: Optional[int]):
    step = N if chunk_rows is None else int(chunk_rows)
    return [(r0, min(step, N - r0)) for r0 in range(0, N, step)]


def lstm_forward(xs: Sequence[Tensor], params: Sequence[Tensor], att_w: Tensor, att_b: Tensor, relu: bool = False,
                 fused: bool = True, chunk_rows: Optional[int] = DEFAULT_CHUNK_ROWS):
    """(out [N, C], alpha [N, L]) of mode "lstm" for the L inputs `xs`; `params` are the LSTM's eight tensors (forward
    direction, then reverse; weight_ih, weight_hh, bias_ih, bias_hh), `att_w` [2 H], `att_b` [1].  No autograd."""
    lib = _lib.load()
    xs = [_unit_cols(x) for x in xs]
    L, (N, C), dev = len(xs), xs[0].shape, xs[0].device
    H = params[1].size(1)
    out = alloc_padded(N, C, dev)
    alpha = torch.empty(N, L, dtype=torch.float32, device=dev)
    if N == 0:
        return out, alpha
    stream = _stream_ptr(dev)
    if fused:
        _lib.check(lib.tgcn_jk_lstm_forward(_pointers(xs), _lds(xs), L, N, C, H, _pointers(params), C, H, att_w.data_ptr(),
                                            att_b.data_ptr(), out.data_ptr(), _ld(out), alpha.data_ptr(), L, int(relu),
                                            stream))
        return out, alpha
    pieces = _chunks(N, chunk_rows)
    ws = _Workspace(pieces[0][1], L, C, H, dev, keep=False)
    for r0, r in pieces:
        xc = [x[r0:r0 + r] for x in xs]
        _run_cells(lib, ws, [_aligned_rows(x) for x in xc], params, r, C, H)
        _lib.check(lib.tgcn_jk_attention(_pointers(xc), _lds(xc), L, r, C, H, ws.h[0].data_ptr(), ws.h[1].data_ptr(), ws.H4,
                                         ws.R * ws.H4, att_w.data_ptr(), att_b.data_ptr(), out[r0:].data_ptr(), _ld(out),
                                         alpha[r0:].data_ptr(), L, int(relu), stream))
    return out, alpha


def lstm_backward(xs: Sequence[Tensor], params: Sequence[Tensor], att_w: Tensor, alpha: Tensor, G: Tensor,
                  out: Optional[Tensor] = None, chunk_rows: Optional[int] = DEFAULT_CHUNK_ROWS):
    """Gradients of `lstm_forward` for G = d out: (dxs [L x [N, C]], dparams [8], d att_w [2 H]).  `out`: the forward's
    result when it ran with `relu` (its sign is the mask), else None.  Recomputes the LSTM in chunks of `chunk_rows` rows;
    the chunks' contributions to the parameter gradients are added in the order of the rows."""
    lib = _lib.load()
    xs = [_unit_cols(x) for x in xs]
    G = _unit_cols(G)
    L, (N, C), dev = len(xs), xs[0].shape, xs[0].device
    H = params[1].size(1)
    stream = _stream_ptr(dev)
    dxs = [torch.empty(N, C, dtype=torch.float32, device=dev) for _ in range(L)]
    dparams = [torch.zeros_like(p) for p in params]
    d_aw = torch.zeros(2 * H, dtype=torch.float32, device=dev)
    if N == 0:
        return dxs, dparams, d_aw
    w_cat = torch.cat([params[0], params[4]], 0)             # [8 H, C]: d x_t's LSTM part is one product per step
    pieces = _chunks(N, chunk_rows)
    ws = _Workspace(pieces[0][1], L, C, H, dev, keep=True)
    H4 = ws.H4
    for r0, r in pieces:
        xc = [x[r0:r0 + r] for x in xs]
        xa = [_aligned_rows(x) for x in xc]
        Gc, alpha_c = G[r0:r0 + r], alpha[r0:r0 + r]
        out_ptr, ldo = (out[r0:].data_ptr(), _ld(out)) if out is not None else (None, 0)
        _run_cells(lib, ws, xa, params, r, C, H)
        _lib.check(lib.tgcn_jk_attention_grad(_pointers(xc), _lds(xc), L, r, C, Gc.data_ptr(), _ld(Gc), out_ptr, ldo,
                                              alpha_c.data_ptr(), L, ws.dscore.data_ptr(), L, stream))
        for d in (0, 1):
            whh = params[4 * d + 1]
            back = list(range(L - 1, -1, -1) if d == 0 else range(L))       # the direction's steps, last one first
            for idx, t in enumerate(back):
                prev = back[idx + 1] if idx + 1 < L else None                # the step before t in the direction's time
                dg = ws.dgates[t, :r, 4 * H * d:4 * H * (d + 1)]
                _lib.check(lib.tgcn_jk_cell_grad(
                    ws.gates[d, t].data_ptr(), 4 * H, ws.c[d, t].data_ptr(), H4,
                    ws.c[d, prev].data_ptr() if prev is not None else None, H4, ws.dh.data_ptr() if idx > 0 else None, H4,
                    ws.dscore[:, t:].data_ptr(), L, att_w[d * H:].data_ptr(), ws.dc.data_ptr(), H4, int(idx == 0),
                    dg.data_ptr(), 8 * H, r, H, stream))
                if prev is not None:
                    _mm(lib.tgcn_gemm_nn, dg, whh, ws.dh[:r], 4 * H, H)    # d h_prev = d gates_t @ W_hh
                    dparams[4 * d + 1] += dense.gemm_tn(dg, ws.h[d, prev, :r, :H])
                dparams[4 * d] += dense.gemm_tn(dg, xa[t])
                db = colsum(dg)
                dparams[4 * d + 2] += db
                dparams[4 * d + 3] += db
                d_aw[d * H:(d + 1) * H] += dense.gemm_tn(ws.h[d, t, :r, :H], ws.dscore[:r, t:t + 1]).view(H)
        for t in range(L):
            _mm(lib.tgcn_gemm_nn, ws.dgates[t, :r], w_cat, ws.T[:r], 8 * H, C)
            _lib.check(lib.tgcn_jk_input_grad(dxs[t][r0:].data_ptr(), C, ws.T.data_ptr(), ws.T.stride(0), Gc.data_ptr(),
                                              _ld(Gc), out_ptr, ldo, alpha_c[:, t:].data_ptr(), L, r, C, stream))
    return dxs, dparams, d_aw


class _JKLstm(torch.autograd.Function):
    """Saves the L inputs, alpha, the parameters and -- for the sign of the relu epilogue -- the result itself."""

    @staticmethod
    def forward(ctx, cfg, att_w: Tensor, att_b: Tensor, *rest: Tensor):
        relu, fused, chunk_rows = cfg
        params, xs = rest[:8], rest[8:]
        out, alpha = lstm_forward([x.detach() for x in xs], [p.detach().contiguous() for p in params],
                                  att_w.detach().reshape(-1), att_b.detach(), relu, fused, chunk_rows)
        ctx.cfg = cfg
        ctx.save_for_backward(att_w, alpha, *rest, *([out] if relu else []))
        return out

    @staticmethod
    def backward(ctx, G: Tensor):
        relu, _, chunk_rows = ctx.cfg
        saved = ctx.saved_tensors
        att_w, alpha = saved[0], saved[1]
        out = saved[-1] if relu else None
        rest = saved[2:-1] if relu else saved[2:]
        params, xs = [p.contiguous() for p in rest[:8]], rest[8:]
        dxs, dparams, d_aw = lstm_backward(xs, params, att_w.reshape(-1), alpha, G, out, chunk_rows)
        d_ab = torch.zeros(1, dtype=torch.float32, device=G.device)          # identically zero (module docstring)
        return (None, d_aw.view_as(att_w), d_ab, *dparams, *dxs)


class JumpingKnowledge(nn.Module):
    """PyG 1.6.3's `JumpingKnowledge(mode, channels=None, num_layers=None)`: "cat", "max" or "lstm" over a list of L
    tensors [N, C].  Mode "lstm" holds `self.lstm = nn.LSTM(channels, (num_layers * channels) // 2, bidirectional=True,
    batch_first=True)` and `self.att = nn.Linear(2 * ((num_layers * channels) // 2), 1)` as PARAMETER HOLDERS -- the
    state_dict keys, shapes, gate order and initialisation are PyG's, a checkpoint of the reference loads with strict=True --
    and never calls their `forward`: the arithmetic runs on `tgcn_jk_*` (see the module docstring).

    `chunk_rows` (an extension, last keyword): rows per chunk of the backward and of the composed path; None = one chunk.
    The gradient of `att.bias` is exact zeros (the softmax is shift invariant; torch returns rounding noise).  At most
    `MAX_LAYERS` = 8 inputs; CPU tensors or operands that are not float32 raise -- there is no CPU fallback.  Hidden widths
    beyond 256 (the fused kernel keeps the cell state in registers) always take the composed path."""

    def __init__(self, mode, channels=None, num_layers=None, chunk_rows: Optional[int] = DEFAULT_CHUNK_ROWS):
        super().__init__()
        self.mode = mode.lower()
        assert self.mode in ["cat", "max", "lstm"]
        if chunk_rows is not None and int(chunk_rows) < 1:
            raise ValueError(f"chunk_rows must be >= 1 or None, got {chunk_rows}")
        self.chunk_rows = None if chunk_rows is None else int(chunk_rows)
        if self.mode == "lstm":
            assert channels is not None, "channels cannot be None for lstm"
            assert num_layers is not None, "num_layers cannot be None for lstm"
            if num_layers > MAX_LAYERS:
                raise ValueError(f"JumpingKnowledge: num_layers={num_layers}; libtgcn.so takes at most {MAX_LAYERS} "
                                 "(TGCN_JK_MAX_LAYERS)")
            self.lstm = nn.LSTM(channels, (num_layers * channels) // 2, bidirectional=True, batch_first=True)
            self.att = nn.Linear(2 * ((num_layers * channels) // 2), 1)
        self.reset_parameters()

    def reset_parameters(self):
        if hasattr(self, "lstm"):
            self.lstm.reset_parameters()
        if hasattr(self, "att"):
            self.att.reset_parameters()

    def _lstm_parameters(self) -> List[Tensor]:
        m = self.lstm
        return [m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0,
                m.weight_ih_l0_reverse, m.weight_hh_l0_reverse, m.bias_ih_l0_reverse, m.bias_hh_l0_reverse]

    def takes_fused_path(self) -> bool:
        """Whether mode "lstm" runs the fused forward kernel (the switch is on and the kernel takes the hidden width)."""
        return self.mode == "lstm" and _FUSED_JK and fused_forward_takes(self.lstm.hidden_size)

    def aggregate(self, xs, relu: bool = False) -> Tensor:
        """`forward(xs)` with an optional ReLU on the result (mode "lstm": in the kernel's epilogue)."""
        assert isinstance(xs, (list, tuple))
        if self.mode != "lstm":
            out = torch.cat(xs, dim=-1) if self.mode == "cat" else torch.stack(xs, dim=-1).max(dim=-1)[0]
            return torch.relu(out) if relu else out
        xs = list(xs)
        if not 1 <= len(xs) <= MAX_LAYERS:
            raise ValueError(f"JumpingKnowledge: {len(xs)} inputs; libtgcn.so takes 1 .. {MAX_LAYERS} (TGCN_JK_MAX_LAYERS)")
        params = self._lstm_parameters()
        _require(xs, "its inputs")
        _require(params + [self.att.weight, self.att.bias], "its parameters")
        C = self.lstm.input_size
        if any(x.dim() != 2 or x.shape != xs[0].shape or x.size(1) != C for x in xs):
            raise ValueError(f"JumpingKnowledge: the inputs must all be [N, {C}], got {[tuple(x.shape) for x in xs]}")
        cfg = (bool(relu), self.takes_fused_path(), self.chunk_rows)
        return _JKLstm.apply(cfg, self.att.weight, self.att.bias, *params, *xs)

    def forward(self, xs):
        return self.aggregate(xs)

    def __repr__(self):
        return "{}({})".format(self.__class__.__name__, self.mode)
