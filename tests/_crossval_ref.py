"""The member masked cross-entropy of pytextgcn_amd/csrc/crossval.hip restated in float64, the K separate
`CrossEntropyLoss('mean')` calls of the sweeps under old/ (h_o_train.py: one per learning rate and fold) it must equal, a
pure-Python restatement of what the two launchers choose, and the operands the kernel tests share.  CPU only.  Test
infrastructure; nothing under pytextgcn_amd/ imports this.

The restated choices are written from `tgcn_member_ce` and `adam_members_impl` (csrc/crossval.hip) with what they share with
the flat kernels: `ce_dispatch` / `ce_grid` / `ce_v4` (csrc/masked_ce.h) and `adam_launch` (csrc/adam.h).  They exist so that
the tests can say "every leaf, one case past each launch cap" about their case lists -- no test asks them what the right
answer is."""
import zlib
from functools import lru_cache

import numpy as np
import torch

import _train_cases as tc

FILL = 7.0                                      # what every output buffer holds before a call

# ---- tgcn_member_ce: the launcher's choice ---------------------------------------------------------------------------
MCE_BLOCKS, MCE_MIN_BLOCKS = 2048, 32           # crossval.hip: `kMceBlocks = 2048`, `kMceMinBlocks = 32`


def mce_cap(K):
    """`mce_cap` (crossval.hip), tgcn_member_ce's cap for ce_grid: `std::max(kMceMinBlocks, kMceBlocks / K)` workgroups per member"""
    return max(MCE_MIN_BLOCKS, MCE_BLOCKS // K)


def mce_leaf(C):
    """(LPR, KPL, rows_per_block) by class count: `ce_dispatch` / `ce_grid` of csrc/masked_ce.h, the one table tgcn_member_ce
    and masked_ce_impl both call"""
    lpr, kpl, _, rpb = tc.ce_leaf(C, False)
    return lpr, kpl, rpb


def mce_v4(S, ld, ldd, off, offd, has_grad):
    """`ce_v4(S, logits, ld, dlogits, ldd)` (csrc/masked_ce.h, called by tgcn_member_ce with width = S): `width % 4 == 0 &&
    ld % 4 == 0 && logits % 16 == 0 && (!dlogits || (ldd % 4 == 0 && dlogits % 16 == 0))` for buffers that start `off` /
    `offd` floats into a 16-byte aligned allocation -- whatever C is"""
    return S % 4 == 0 and ld % 4 == 0 and off % 4 == 0 and (not has_grad or (ldd % 4 == 0 and offd % 4 == 0))


def mce_rows_past_cap(K, C):
    """the smallest row count at which a workgroup of the launch takes a second stride of rows"""
    return mce_cap(K) * mce_leaf(C)[2] + 1


LEAF_C = {(4, 4): 5, (4, 8): 17, (8, 8): 33, (16, 8): 65, (32, 8): 129, (64, 4): 257}     # one class count per leaf

# ---- tgcn_adam_members: the launcher's choice ------------------------------------------------------------------------
ADAM_CAP = tc.ADAM_CAP                          # adam_launch (csrc/adam.h), for adam_members_impl as for adam_impl


def adam_members_v4(width, n_cols):
    return width % 4 == 0 and n_cols % 4 == 0


# ---- the float64 reference -------------------------------------------------------------------------------------------
def selected(bits, k):
    """bool [n]: bit k of the int64 `bits`"""
    return ((bits >> k) & 1).bool()


def member_ce(logits, target, bits, K, C, S, dtype=torch.float64):
    """(loss, loss_k [K], dlogits [n, K S], dbias [K S], pred int32 [n, K]) in `dtype`:
         loss_k  = mean over the rows bit k selects of  lse(x[r, seg_k]) - x[r, k S + target[r]]   (NaN when none is)
         loss    = the sum of the loss_k of the non-empty members, in index order
         dlogits = (softmax(x[r, seg_k]) - one-hot) / |sel_k| inside segment k of a selected row -- the entry at the target as
                   -(sum of the OTHER terms) / sum, which does not cancel -- and 0 everywhere else
         pred    = the first-index arg-max of every segment of every row."""
    x = logits.detach().cpu().to(dtype)
    target, bits = target.cpu(), bits.cpu()
    n = x.size(0)
    d = torch.zeros(n, K * S, dtype=dtype)
    loss_k = torch.full((K,), float("nan"), dtype=dtype)
    loss = torch.zeros((), dtype=dtype)
    pred = np.zeros((n, K), dtype=np.int32)
    for k in range(K):
        seg_all = x[:, k * S:k * S + C]
        if n:
            pred[:, k] = np.argmax(seg_all.numpy(), axis=1)
        rows = torch.nonzero(selected(bits, k)).flatten()
        m_ = rows.numel()
        if m_ == 0:
            continue
        seg = seg_all[rows]
        t = target[rows]
        r = torch.arange(m_)
        m = seg.max(dim=1, keepdim=True).values
        e = torch.exp(seg - m)
        et = e[r, t].clone()
        e_others = e.clone()
        e_others[r, t] = 0.0
        others = e_others.sum(1)
        tot = others + et
        loss_k[k] = (torch.log(tot) - (seg[r, t] - m.flatten())).sum() / m_
        loss = loss + loss_k[k]
        g = e / tot[:, None]
        g[r, t] = -(others / tot)
        d[rows, k * S:k * S + C] = g / m_
    return loss, loss_k, d, d.sum(0), torch.from_numpy(pred)


def separate_ce(logits, target, bits, K, C, S):
    """What the sweeps compute: one `CrossEntropyLoss('mean')(logits[sel_k][:, seg_k], target[sel_k])` per member, each with
    its own backward.  Returns (loss_k [K] float64, NaN where sel_k is empty; the sum of the K gradients w.r.t. the logits)."""
    x = logits.detach().cpu().double().requires_grad_()
    crit = torch.nn.CrossEntropyLoss(reduction="mean")
    loss_k = torch.full((K,), float("nan"), dtype=torch.float64)
    grad = torch.zeros_like(x)
    for k in range(K):
        sel = selected(bits.cpu(), k)
        if not bool(sel.any()):
            continue
        lk = crit(x[sel][:, k * S:k * S + C], target.cpu()[sel])
        grad += torch.autograd.grad(lk, x)[0]
        loss_k[k] = lk.detach()
    return loss_k, grad


# ---- operands --------------------------------------------------------------------------------------------------------
def _seed(*v):
    return zlib.crc32(repr(v).encode())


def _bit(k):
    return (1 << k) - (1 << 64) if k == 63 else 1 << k


def make_bits(n, K, gen, empty):
    """int64 [n]: two thirds of the rows 0 (word nodes); the others cycle through all K bits, one bit, a random subset, and
    a subset with every bit at or above K set as well (ignored).  No row selects member `empty` (-1: none left out)."""
    every = sum(_bit(k) for k in range(K) if k != empty)
    high = sum(_bit(k) for k in range(K, 64))
    out = np.zeros(n, dtype=np.int64)
    docs = np.nonzero(gen.random(n) < 1.0 / 3.0)[0] if n > 2 else np.arange(n)
    for i, r in enumerate(docs):
        kind = i % 4
        if kind == 0:
            b = every
        elif kind == 1:
            b = _bit(int(gen.integers(0, K)))
        else:
            b = sum(_bit(k) for k in range(K) if gen.random() < 0.5)
            if kind == 3:
                b |= high
        if empty >= 0:
            b &= ~_bit(empty)
        out[r] = b                       # (bit 63 is the sign: every sum above stays inside int64)
    return torch.from_numpy(out)


@lru_cache(maxsize=4)
def make_case(n, K, C, S, values="randn"):
    """Operands on the CPU, shared by the cases of one (n, K, C, S, values) and left unchanged.  Segment k of the logits holds
    `_train_cases.ce_inputs(C, n, values)["x"]` with its rows rotated by k, so that every member meets every value row at
    another row; the pad columns hold 1e30 (a pad that leaks into a maximum or a sum is seen at once).  The target is
    `ce_inputs`' and is shared by the members; where the rotation puts a -inf of the "neginf" rows on a target column, that
    entry becomes 0.5 (a target of probability zero has an infinite loss).  With K >= 2 member n % K has no selected row."""
    gen = np.random.default_rng(_seed("mce", n, K, C, S, values))
    base = tc.ce_inputs(C, n, values)
    x = np.full((n, K * S), 1e30, dtype=np.float32)
    target = base["target"].copy()
    for k in range(K):
        seg = np.roll(base["x"], k, axis=0) if n else base["x"]
        if values == "neginf" and n:
            seg = seg.copy()
            r = np.arange(n)
            fix = np.isneginf(seg[r, target])
            seg[r[fix], target[fix]] = np.float32(0.5)
        x[:, k * S:k * S + C] = seg
    empty = n % K if K >= 2 else -1
    bits = make_bits(n, K, gen, empty)
    if values == "onemask" and n:
        bits = torch.zeros(n, dtype=torch.int64)
        bits[n // 2] = _bit(0)
    if values == "randn" and bool((bits == 0).any()):
        x[int(torch.nonzero(bits == 0)[0]), :C] = -np.inf              # a row of -inf nobody trains on: arg-max 0
    return dict(logits=torch.from_numpy(x), target=torch.from_numpy(np.ascontiguousarray(target)), bits=bits, K=K, C=C, S=S,
                empty=empty)


@lru_cache(maxsize=4)
def reference(n, K, C, S, values="randn"):
    c = make_case(n, K, C, S, values)
    return member_ce(c["logits"], c["target"], c["bits"], K, C, S)


def counts_of(bits, K):
    return [int(selected(bits, k).sum()) for k in range(K)]


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if b.numel() == 0:
        return 0.0 if a.numel() == 0 else float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def row_err(got, ref):
    """every gradient row held to its OWN largest entry (all-zero rows must be zero); the rows below
    `_train_cases.TINY_ROW` -- see there -- against that scale"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if ref.numel() == 0:
        return 0.0
    num, den = (got - ref).abs().max(1).values, ref.abs().max(1).values
    zero, tiny = den == 0, (den > 0) & (den < tc.TINY_ROW)
    held = ~zero & ~tiny
    err = float(num[zero].max()) / tc.TINY_ROW if bool(zero.any()) else 0.0      # (0 unless a zero row is not zero)
    if bool(held.any()):
        err = max(err, float((num[held] / den[held]).max()))
    if bool(tiny.any()):
        err = max(err, float(num[tiny].max()) / tc.TINY_ROW)
    return err
