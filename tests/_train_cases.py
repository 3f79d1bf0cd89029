"""Cases of the sweep over the training-step kernels of csrc/train.hip (tests/test_gpu_train_kernels.py): the masked
cross-entropy (k_masked_ce + k_ce_final; row body and leaf table in csrc/masked_ce.h), Adam (k_adam + k_adam_scalars; sweep
and launcher in csrc/adam.h) and k_scale_unless_one.  The case lists, a
pure-Python restatement of what the launchers choose, the inputs and the float64 references.  CPU only: numpy; nothing here
imports torch.cuda or the library.  Test infrastructure; tests/test_train_cases.py keeps the lists honest.

The restated choices are written from `masked_ce_impl` (csrc/train.hip) with `ce_dispatch` / `ce_grid` / `ce_v4`
(csrc/masked_ce.h) and from `adam_launch` (csrc/adam.h); the lines are cited where they are restated.  They
exist so that the host test can say "every leaf, both sides of every boundary, one case above each launch cap" about the
LIST -- the GPU test never asks them what the right answer is."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

FILL = 7.0                                      # what every output buffer holds before a call
N_SMALL = 257                                   # rows of the small cases: five row groups of the widest leaf, one ragged

# ---- masked cross-entropy: the launcher's choice ---------------------------------------------------------------------
CE_BLOCKS = 2048                                # train.hip: `constexpr int kCeBlocks = 2048` (masked_ce_impl's cap for ce_grid)
CE_EDGES = ((16, 17), (32, 33), (64, 65), (128, 129), (256, 257))
CE_RANGES = ((1, 16), (17, 32), (33, 64), (65, 128), (129, 256), (257, None))


def ce_leaf(C, v4):
    """(LPR, KPL, in_regs, rows_per_block) of `ce_dispatch` / `ce_grid` (csrc/masked_ce.h) for C classes.

    `if (C <= 16) leaf(4, 4); else if (C <= 32) leaf(4, 8); else if (C <= 64) leaf(8, 8); else if (C <= 128) leaf(16, 8);
    else if (C <= 256) leaf(32, 8); else leaf(64, 4);` (the arguments as std::integral_constant).  ce_grid's
    `rows_per_block = 2 * 4 * (64 / lpr)` is UN = 2 row groups x 4 waves x (64 / LPR) rows; `in_regs = C <= KPL * LPR` is
    ce_rows' own test.  `v4` (`leaf`'s `if (v4)`) picks the column map, not the tuple; it is an argument so that a leaf is
    (C range, v4)."""
    assert C >= 1 and (not v4 or C % 4 == 0)
    if C <= 16:
        lpr, kpl = 4, 4
    elif C <= 32:
        lpr, kpl = 4, 8
    elif C <= 64:
        lpr, kpl = 8, 8
    elif C <= 128:
        lpr, kpl = 16, 8
    elif C <= 256:
        lpr, kpl = 32, 8
    else:
        lpr, kpl = 64, 4
    return lpr, kpl, C <= lpr * kpl, 2 * 4 * (64 // lpr)


def ce_v4(C, ld, ldd, off, offd, has_grad):
    """`ce_v4(C, logits, ld, dlogits, ldd)` (csrc/masked_ce.h, called by masked_ce_impl with width = C): `width % 4 == 0 &&
    ld % 4 == 0 && logits % 16 == 0 && (!dlogits || (ldd % 4 == 0 && dlogits % 16 == 0))`, for buffers whose base is 16-byte
    aligned and that start `off` / `offd` floats into it."""
    return C % 4 == 0 and ld % 4 == 0 and off % 4 == 0 and (not has_grad or (ldd % 4 == 0 and offd % 4 == 0))


def ce_grid(C, n):
    """ce_grid(n_rows, lpr, kCeBlocks): `min(cap, max(1, (n_rows + rows_per_block - 1) / rows_per_block))`"""
    rpb = ce_leaf(C, False)[3]
    return min(CE_BLOCKS, max(1, -(-n // rpb)))


# ---- masked cross-entropy: the cases ---------------------------------------------------------------------------------
OUTPUTS = ("loss", "grad", "dbias")             # tgcn_masked_ce_pred without / with dlogits; tgcn_masked_ce_grad
CeCase = namedtuple("CeCase", "C n pad pad2 off offd out pred values")
CeCase.__doc__ = """C classes, n rows; logits are [n, C + pad] starting `off` floats into a 16-byte aligned buffer, dlogits
[n + 3, C + pad2] starting `offd` floats in; `out` (OUTPUTS), `pred` (arg-max wanted), `values` (VALUES)."""

# widths per class-count range: for the 16-byte leaf multiples of 4, the upper edge of the range among them; for the
# scalar leaf the lower edge, an odd width, and the multiples of 4 that only a layout can force onto it
V4_WIDTHS = ((4, 16), (20, 32), (36, 64), (68, 128), (132, 256), (260, 300))
SCALAR_WIDTHS = ((3, 7, 16), (17, 32), (33, 64), (65, 128), (129, 219, 256), (257, 258, 259, 260))
# (pad, pad2, off, offd)
V4_LAYOUTS = ((0, 0, 0, 0), (4, 4, 0, 0), (0, 4, 0, 0), (4, 0, 0, 0))
ODD_LAYOUTS = ((1, 3, 0, 0), (0, 0, 1, 1), (4, 4, 1, 0), (0, 4, 0, 1), (3, 4, 0, 0), (4, 1, 0, 0))   # for C % 4 == 0
ANY_LAYOUTS = ((0, 0, 0, 0), (1, 3, 0, 0), (5, 0, 0, 0))                                             # for C % 4 != 0

VALUES = ("randn", "at+80", "at-80", "at+1e4", "at-1e4", "x80", "x1e4", "neginf", "equal", "onemask", "ties", "onehot")
EDGE_VALUES = VALUES[1:11]
# one width per leaf for the value edges and the grid-stride cases: the full width of the 16-byte leaf, the lower edge
# of the scalar one (C > LPR and C > KPL everywhere, so that all three tie placements exist)
LEAF_WIDTH = {True: (16, 32, 64, 128, 256, 260), False: (7, 17, 33, 65, 129, 257)}


def case_is_v4(c):
    return ce_v4(c.C, c.C + c.pad, c.C + c.pad2, c.off, c.offd, c.out != "loss")


def leaf_of(c):
    """(LPR, KPL, v4): the kernel instantiation the case runs"""
    lpr, kpl, _, _ = ce_leaf(c.C, False)
    return lpr, kpl, case_is_v4(c)


LEAVES = tuple((lpr, kpl, v4) for v4 in (True, False) for lpr, kpl in ((4, 4), (4, 8), (8, 8), (16, 8), (32, 8), (64, 4)))


def leaf_id(leaf):
    return f"lpr{leaf[0]}-kpl{leaf[1]}-{'v4' if leaf[2] else 'scalar'}"


def ce_case_id(c):
    return f"C{c.C}-n{c.n}-pad{c.pad}.{c.pad2}-off{c.off}.{c.offd}-{c.out}{'-pred' if c.pred else ''}-{c.values}"


@lru_cache(maxsize=None)
def small_cases():
    """every width of every leaf x every layout that keeps it on the leaf x the three outputs x with / without pred"""
    out = []
    for widths in V4_WIDTHS:
        for C in widths:
            for lay in V4_LAYOUTS:
                out += [CeCase(C, N_SMALL, *lay, o, p, "randn") for o in OUTPUTS for p in (False, True)]
    for widths in SCALAR_WIDTHS:
        for C in widths:
            for lay in (ODD_LAYOUTS if C % 4 == 0 else ANY_LAYOUTS):
                for o in OUTPUTS:
                    c = CeCase(C, N_SMALL, *lay, o, False, "randn")
                    if not case_is_v4(c):                      # (a shifted dlogits does not move the loss-alone call)
                        out += [c, c._replace(pred=True)]
    out += [CeCase(C, n, 0, 0, 0, 0, "dbias", True, "randn") for C in (2, 16, 64, 300) for n in (1, 37)]
    return tuple(out)


def _leaf_case(leaf, n, values, out="dbias", pred=True):
    lpr, kpl, v4 = leaf
    C = LEAF_WIDTH[v4][[l[:2] for l in LEAVES[:6]].index((lpr, kpl))]
    lay = (4, 4, 0, 0) if v4 else ((1, 3, 0, 0) if C % 4 else (0, 0, 1, 1))
    return CeCase(C, n, *lay, out, pred, values)


@lru_cache(maxsize=None)
def edge_cases():
    """the value edges, at N_SMALL rows per leaf"""
    return tuple(_leaf_case(leaf, N_SMALL, v) for leaf in LEAVES for v in EDGE_VALUES)


@lru_cache(maxsize=None)
def stride_cases():
    """per leaf the smallest n at which a workgroup takes a second stride of rows, 2048 * rows_per_block + 1, with random
    values and with the one-hot rows; and the largest n at which none does"""
    out = []
    for leaf in LEAVES:
        rpb = 2 * 4 * (64 // leaf[0])
        out += [_leaf_case(leaf, CE_BLOCKS * rpb + 1, "randn"), _leaf_case(leaf, CE_BLOCKS * rpb + 1, "onehot", out="grad"),
                _leaf_case(leaf, CE_BLOCKS * rpb, "onehot", out="loss")]
    return tuple(out)


def all_ce_cases():
    return small_cases() + edge_cases() + stride_cases()


def by_leaf(cases):
    """{leaf: [cases]} -- one GPU test function per leaf"""
    out = {leaf: [] for leaf in LEAVES}
    for c in cases:
        out[leaf_of(c)].append(c)
    return out


# ---- masked cross-entropy: inputs and reference ----------------------------------------------------------------------
def _seed(*v):
    return zlib.crc32(repr(v).encode())


def tie_pairs(C):
    """the column pairs that hold a row's tied maximum: the ends of the row, and the two places where the column maps of
    the two leaves hand over from one lane to the next -- (LPR-1, LPR) for the strided map, (KPL-1, KPL) for the
    consecutive one"""
    lpr, kpl, _, _ = ce_leaf(C, False)
    return tuple(p for p in ((0, C - 1), (lpr - 1, lpr), (kpl - 1, kpl)) if p[1] < C and p[0] != p[1])


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@lru_cache(maxsize=6)
def ce_inputs(C, n, values):
    """{"x": float32 [n, C], "target": int64 [n], "mask": bool [n], "inv_count": float}; shared by the cases of one
    (C, n, values) and read-only"""
    gen = np.random.default_rng(_seed(C, n, values))
    target = gen.integers(0, C, size=n).astype(np.int64)
    mask = gen.random(n) < 0.5
    if n:
        mask[gen.integers(0, n)] = True
    if values == "onehot":
        r = np.arange(n)
        x = np.zeros((n, C), dtype=np.float32)
        x[r, r % C] = 40.0
        target, mask = (r // 3) % C, np.ones(n, dtype=bool)
    else:
        x = gen.standard_normal((n, C), dtype=np.float32) * np.float32(3.0)
    r = np.arange(n)
    if values.startswith("at"):                   # rows AT +-L: what the subtraction of the row maximum is for
        x = x + np.float32(float(values[2:]))
    elif values in ("x80", "x1e4"):               # rows SCALED to +-L: one-hot softmax, exp underflows next to the maximum
        x = x / np.abs(x).max(1, keepdims=True) * np.float32(float(values[1:]))
    elif values == "neginf":
        drop = gen.random((n, C)) < 1.0 / 3.0
        drop[r, target] = False
        x = np.where(drop, np.float32(-np.inf), x)
    elif values == "equal":
        x = np.repeat(np.asarray([0.0, 5.0, -80.0, 1e4, -1e4], dtype=np.float32)[r % 5][:, None], C, axis=1)
    elif values == "onemask":
        mask = np.zeros(n, dtype=bool)
        mask[n // 2] = True
    elif values == "ties":
        pairs = tie_pairs(C)
        x = np.minimum(x, np.float32(4.0))
        for i, (a, b) in enumerate(pairs):
            rows = r[r % (len(pairs) + 1) == i]   # (the remaining rows keep their own maximum, several times over)
            x[rows, a] = x[rows, b] = np.float32(6.0)
        x[r % (len(pairs) + 1) == len(pairs)] = np.round(x[r % (len(pairs) + 1) == len(pairs)])
    x = np.ascontiguousarray(x, dtype=np.float32)
    inv = float(np.float32(1.0 / max(int(mask.sum()), 1)))
    return _frozen(x=x, target=np.ascontiguousarray(target, dtype=np.int64), mask=mask, inv_count=inv)


def ce_reference_of(x, target, mask, inv_count):
    """float64: loss = inv_count * sum over masked rows of logsumexp(x_r) - x_r[t_r]; its gradient (softmax - one-hot) *
    inv_count on the masked rows and 0 elsewhere, the entry at the target as -(sum of the OTHER terms) / sum so that it does
    not cancel; the column sums; the first-index arg-max of every row.  Rows with a target outside [0, C) contribute NaN to
    the loss and softmax * inv_count to the gradient (no class to subtract)."""
    x = np.asarray(x, dtype=np.float64)
    n, C = x.shape
    r = np.arange(n)
    ok = (target >= 0) & (target < C)
    tc = np.where(ok, target, 0)
    m = x.max(1, keepdims=True) if n else np.zeros((0, 1))
    with np.errstate(invalid="ignore"):
        d = x - m
    e = np.exp(d)
    et = np.where(ok, e[r, tc], 0.0)
    e_others = e.copy()
    e_others[r[ok], tc[ok]] = 0.0
    others = e_others.sum(1)
    s = others + et
    rows = np.where(ok, np.log(s) - d[r, tc], np.nan)
    loss = float(rows[mask].sum() * inv_count)
    grad = e / s[:, None]
    grad[r[ok], tc[ok]] = -(others / s)[ok]
    grad *= inv_count
    grad[~mask] = 0.0
    return _frozen(loss=loss, grad=grad, dbias=grad.sum(0), pred=x.argmax(1).astype(np.int64) if n else np.zeros(0, np.int64))


@lru_cache(maxsize=6)
def ce_reference(C, n, values):
    i = ce_inputs(C, n, values)
    return ce_reference_of(i["x"], i["target"], i["mask"], i["inv_count"])


# A gradient row whose largest entry is below this is held to THIS scale instead of its own.  fp32 has no normal number
# below 2^-126 and expf may flush what lies below to zero: an error of 2^-126 is TOL times 2^-109.4, so a row of scale
# 2^-100 can still be held to TOL with 9 bits to spare, and a smaller one cannot be held to its own scale by any fp32
# kernel.  (Only rows SCALED to +-80 / +-1e4 get there: softmax entries of exp(-100) and less.)
TINY_ROW = 2.0 ** -100


# ---- Adam ------------------------------------------------------------------------------------------------------------
ADAM_BLOCKS = 8192                              # adam_launch (csrc/adam.h): `a.grid = min(8192, (n / 4 + 255) / 256 + 1)`
ADAM_PER_BLOCK = 1024                           # 256 threads x 4 elements
ADAM_CAP = ADAM_BLOCKS * ADAM_PER_BLOCK         # 8 388 608: above it a thread takes a second stride
ADAM_NT = 1 << 24                               # adam_launch: `const bool nt = n >= (int64_t(1) << 24)`
AdamCase = namedtuple("AdamCase", "n amsgrad wd beta1")
ADAM_SMALL_N = (1, 2, 3, 5, 6, 7, 1023, 1024, 1025)
ADAM_BETA1 = (0.9, 0.5, 0.3)
ADAM_STEPS = 3
ADAM_LR, ADAM_BETA2, ADAM_EPS = 1e-3, 0.999, 1e-8


def adam_leaf(n, amsgrad):
    """(nt, grid) of `adam_launch` (csrc/adam.h), which `adam_impl` (csrc/train.hip) calls: `a.grid = min(8192, (n / 4 + 255) /
    256 + 1)` workgroups of 256 threads, four elements per thread and stride; `nt = n >= 1 << 24` streams the state past the
    caches.  `amsgrad` (max_exp_avg_sq != NULL) picks the other template argument and changes neither."""
    return n >= ADAM_NT, min(ADAM_BLOCKS, (n // 4 + 255) // 256 + 1)


def adam_second_stride(n, amsgrad=True):
    """does a thread of the launch run its loop a second time?"""
    return n > adam_leaf(n, amsgrad)[1] * ADAM_PER_BLOCK


def lerp_branch(beta1):
    """which branch of adam_element's `m = w1 < 0.5f ? m + w1 * diff : gr - diff * (1.f - w1)` a beta1 takes, with
    `w1 = static_cast<float>(1.0 - beta1)` as adam_launch derives it.  beta1 = 0.5 gives w1 = 0.5f exactly: NOT below 0.5f, the
    second branch."""
    return "low" if np.float32(1.0 - beta1) < np.float32(0.5) else "high"


@lru_cache(maxsize=None)
def adam_small_cases():
    return tuple(AdamCase(n, a, wd, b1) for n in ADAM_SMALL_N for a in (True, False) for wd in (0.0, 0.01) for b1 in ADAM_BETA1)


@lru_cache(maxsize=None)
def adam_big_cases():
    """around the launch cap of the plain leaf -- the combinations are not crossed at this size: every n, both amsgrad
    settings, both weight decays and all three beta1 appear once or twice"""
    return (AdamCase(ADAM_CAP - 4, True, 0.0, 0.9),               # the last n without a second stride
            AdamCase(ADAM_CAP + 4, True, 0.01, 0.3),              # one float4 in the second stride
            AdamCase(ADAM_CAP + 4, False, 0.0, 0.5),
            AdamCase(ADAM_CAP + 1024 * 3 + 1, False, 0.01, 0.9))  # three workgroups of the second stride and a scalar tail


def all_adam_cases():
    return adam_small_cases() + adam_big_cases()


# the n of tests/test_gpu_parity.py::test_fused_adam_streaming_path_for_large_tensors, which keeps the streaming leaf
ADAM_NT_TESTED_ELSEWHERE = (1 << 24) + 5


def adam_case_id(c):
    return f"n{c.n}-{'ams' if c.amsgrad else 'plain'}-wd{c.wd:g}-b{c.beta1:g}"


def adam_inputs(c):
    """p, m ~ N(0, 1); v, vmax >= 0 with vmax on either side of v; three gradients of differing scale (float32)"""
    gen = np.random.default_rng(_seed("adam", *c))
    f = lambda: gen.standard_normal(c.n, dtype=np.float32)
    p, m = f(), f()
    v = gen.random(c.n, dtype=np.float32) + np.float32(0.1)
    vmax = v * (np.float32(0.5) + gen.random(c.n, dtype=np.float32))
    grads = [f() * np.float32(s) for s in (1.0, 0.1, 3.0)[:ADAM_STEPS]]
    return p, m, v, vmax, grads


def adam_scalars(step, lr=ADAM_LR, beta1=0.9, beta2=ADAM_BETA2):
    """the two step-dependent floats as adam_launch derives them on the host: `bc = 1.0 - std::pow(beta, double(step))`,
    `float(lr / bc1)`, `float(1.0 / std::sqrt(bc2))` -- all in double, rounded once"""
    bc1, bc2 = 1.0 - beta1 ** float(step), 1.0 - beta2 ** float(step)
    return np.float32(lr / bc1), np.float32(1.0 / np.sqrt(bc2))


def adam_reference(c, p, m, v, vmax, grads, lr=ADAM_LR, beta2=ADAM_BETA2, eps=ADAM_EPS):
    """torch/optim/adam.py `_single_tensor_adam` in float64, steps 1 .. len(grads); returns (p, m, v, vmax)"""
    p, m, v, vmax = (a.astype(np.float64) for a in (p, m, v, vmax))
    for step, g in enumerate(grads, 1):
        g = g.astype(np.float64)
        if c.wd:
            g = g + c.wd * p
        m += (g - m) * (1.0 - c.beta1)                            # exp_avg.lerp_(grad, 1 - beta1)
        v = beta2 * v + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - c.beta1 ** step, 1.0 - beta2 ** step
        if c.amsgrad:
            vmax = np.maximum(vmax, v)
            denom = np.sqrt(vmax) / np.sqrt(bc2) + eps
        else:
            denom = np.sqrt(v) / np.sqrt(bc2) + eps
        p = p - (lr / bc1) * (m / denom)
    return p, m, v, vmax


# ---- k_scale_unless_one ----------------------------------------------------------------------------------------------
SCALE_BLOCKS = 4096                             # tgcn_scale_by_device_scalar: `grid = min(4096, (n + 255) / 256)`
SCALE_CAP = SCALE_BLOCKS * 256                  # 1 048 576: above it a thread takes a second stride
SCALE_N = (1, 255, 256, 257, SCALE_CAP, SCALE_CAP + 1 + 256)
SCALES = (2.5, 0.0)
