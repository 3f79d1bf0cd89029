"""The grouped masked cross-entropy of pytextgcn_amd/csrc/perlabel.hip restated as plain tensor expressions in any dtype
(float64 for the truth), the K separate `CrossEntropyLoss('mean')` calls of perlabel_amazon.py:130-137 it must equal, the
routed prediction of eval_perlabel.py:71-78, and the operands the kernel tests share.  Test infrastructure; nothing under
pytextgcn_amd/ imports this."""
import numpy as np
import torch


def selections(mask, group, K):
    """[sel_k] = the rows `mask & (group == k)` for k in 0..K-1."""
    return [mask & (group == k) for k in range(K)]


def grouped_ce(logits, target, mask, group, starts, widths, dtype=torch.float64):
    """(loss, loss_k [K], dlogits [n, n_cols], dbias [n_cols]) in `dtype`, in closed form:
         loss_k  = mean over sel_k of  lse(x[r, seg_k]) - x[r, start_k + target[r]]      (NaN for an empty selection)
         loss    = sum of the loss_k of the non-empty groups
         dlogits = (softmax(x[r, seg_k]) - one-hot) / |sel_k| inside the segment of a selected row, 0 everywhere else."""
    x = logits.detach().cpu().to(dtype)
    target, mask, group = target.cpu(), mask.cpu(), group.cpu().long()
    n, C = x.shape
    K = len(starts)
    d = torch.zeros(n, C, dtype=dtype)
    loss_k = torch.full((K,), float("nan"), dtype=dtype)
    loss = torch.zeros((), dtype=dtype)
    for k, sel in enumerate(selections(mask, group, K)):
        rows = torch.nonzero(sel).flatten()
        if rows.numel() == 0:
            continue
        s, w = starts[k], widths[k]
        seg = x[rows, s:s + w]
        m = seg.max(dim=1, keepdim=True).values
        e = torch.exp(seg - m)
        tot = e.sum(dim=1, keepdim=True)
        lse = (m + torch.log(tot)).flatten()
        t = target[rows]
        loss_k[k] = (lse - seg[torch.arange(rows.numel()), t]).sum() / rows.numel()
        loss = loss + loss_k[k]
        g = e / tot
        g[torch.arange(rows.numel()), t] -= 1.0
        d[rows, s:s + w] = g / rows.numel()
    return loss, loss_k, d, d.sum(0)


def separate_ce(logits, target, mask, group, starts, widths):
    """What the reference computes: one `CrossEntropyLoss('mean')(logits[sel_k][:, seg_k], target[sel_k])` per group, each
    with its own backward.  Returns (loss_k [K] float64 with NaN where sel_k is empty, the sum of the K gradients w.r.t. the
    full logits)."""
    x = logits.detach().cpu().double().requires_grad_()
    K = len(starts)
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    loss_k = torch.full((K,), float("nan"), dtype=torch.float64)
    grad = torch.zeros_like(x)
    for k, sel in enumerate(selections(mask.cpu(), group.cpu().long(), K)):
        if not bool(sel.any()):
            continue
        lk = crit(x[sel][:, starts[k]:starts[k] + widths[k]], target.cpu()[sel])
        grad += torch.autograd.grad(lk, x)[0]
        loss_k[k] = lk.detach()
    return loss_k, grad


def routed_pred(logits, route, starts, widths, class_map=None):
    """int64 [n]: start_q + argmax(x[r, seg_q]) with q = route[r] (numpy's argmax: the first index on ties), through
    `class_map` when given, -1 where q is -1."""
    x = logits.detach().cpu().numpy()
    route = route.cpu().numpy()
    out = np.full(x.shape[0], -1, dtype=np.int64)
    for k, (s, w) in enumerate(zip(starts, widths)):
        rows = np.nonzero(route == k)[0]
        if rows.size:
            out[rows] = s + np.argmax(x[rows, s:s + w], axis=1)
    if class_map is not None:
        cm = class_map.cpu().numpy()
        out = np.where(out >= 0, cm[np.maximum(out, 0)], -1)
    return torch.from_numpy(out)


def layout(widths, aligned, round_cols=False):
    """(starts, n_cols): `aligned` -- every start a multiple of 4 with a gap of four more pad columns in front of every odd
    segment; otherwise the segments back to back from column 0 (starts at any residue, no pad column at all).
    `round_cols` (without `aligned`): the same back-to-back starts in a row of 4 j columns (pad columns at the tail only):
    16-byte rows under unaligned starts."""
    starts, at = [], 0
    for k, w in enumerate(widths):
        if aligned:
            at = ((at + 3) & ~3) + (4 if k % 2 else 0)
        starts.append(at)
        at += w
    return starts, ((at + 3) & ~3) if (aligned or round_cols) else at


def make_case(n, widths, aligned, seed, scale=3.0, round_cols=False, empty_group=-1):
    """Operands on the CPU.  logits ~ scale * N(0, 1) over ALL n_cols columns (pad columns hold numbers too: the kernel must
    not read them into anything); groups uniform in {-1, 0..K-1}; with K >= 2 group `empty_group` has rows but none selected;
    row 0 is all zero, every 5th row is constant inside each segment's first half (ties), a few hold two equal maxima;
    `route` is drawn independently of `group`; `class_map` is a non-trivial injection."""
    gen = torch.Generator().manual_seed(seed)
    K = len(widths)
    starts, n_cols = layout(widths, aligned, round_cols)
    x = torch.randn(n, n_cols, generator=gen) * scale
    if n:
        x[0] = 0.0
        for s, w in zip(starts, widths):
            x[4::5, s:s + (w + 1) // 2] = x[4::5, s:s + 1]
            if w >= 3:
                x[2::7, s + w - 1] = x[2::7, s + 1] = x[2::7, s:s + w].max(dim=1).values + 1.0
    group = torch.randint(-1, K, (n,), generator=gen).to(torch.int32)
    route = torch.randint(-1, K, (n,), generator=gen).to(torch.int32)
    mask = torch.rand(n, generator=gen) < 0.6
    if K >= 2:
        mask &= group != empty_group % K
    w_of = torch.tensor(widths)[group.long().clamp(min=0)]
    target = (torch.rand(n, generator=gen) * w_of).long().clamp(max=w_of - 1) if n else torch.zeros(0, dtype=torch.int64)
    target[group < 0] = -1                                   # `g.y[:] = -1` elsewhere (perlabel_amazon.py:108)
    class_map = 1000 + 3 * torch.arange(n_cols - 1, -1, -1, dtype=torch.int64)
    return dict(logits=x, target=target, mask=mask, group=group, route=route, class_map=class_map, starts=starts,
                widths=list(widths), n_cols=n_cols)


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
