"""The per-level fold-in definition (include/tgcn.h `tgcn_foldin_levels`) restated in numpy, on top of
tests/_foldin_ref.py.  Test infrastructure; nothing under pytextgcn_amd/ imports this.

The document scalars are _foldin_ref's (fp32, bit for bit).  The sums over j, c and k are evaluated in `sum_dtype`.  A level
is a dict: T1 [V, h], P [V, C], W2 [h, C], Wh [C_prev, h] (None at level 1), b1, b2, act, link ("softmax" / "one_hot"; level
1: ignored)."""
import numpy as np

import _foldin_ref as R

F32 = np.float32
SOFTMAX, ONE_HOT = "softmax", "one_hot"
LINK_ID = {SOFTMAX: 0, ONE_HOT: 1}


def scalars(rowptr, col, val, dis, mode, n_vocab):
    """(a, a_dd, keep): _foldin_ref.doc_scalars with an entry whose column lies outside [0, n_vocab) left out of the sums
    over j (keep False, a = 0) -- it still counts in deg_d."""
    col = np.asarray(col, dtype=np.int64)
    keep = (col >= 0) & (col < n_vocab)
    a, a_dd, _ = R.doc_scalars(rowptr, np.where(keep, col, 0), val, dis, mode)
    return np.where(keep, a, F32(0)).astype(F32), a_dd, keep


def softmax_rows(z, dt):
    """The link in `dt`; in float32 it is the header's own order: m, e_c = exp(z_c - m), t_i = e_i (+ e_{i+64}), the butterfly
    over 64 slots, a division."""
    z = np.asarray(z).astype(dt)
    B, C = z.shape
    if B == 0:
        return z.copy()
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m).astype(dt)
    t = np.zeros((B, 64), dtype=dt)
    t[:, :min(C, 64)] = e[:, :64]
    if C > 64:
        t[:, :C - 64] = (t[:, :C - 64] + e[:, 64:]).astype(dt)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        t = (t + t[:, lanes ^ off]).astype(dt)
    return (e / t[:, :1]).astype(dt)


def one_hot_rows(z):
    z = np.asarray(z)
    p = np.zeros(z.shape, dtype=F32)
    if z.shape[0]:
        p[np.arange(z.shape[0]), R.first_argmax(z)] = 1.0
    return p


def foldin_levels(rowptr, col, val, dis, mode, levels, sum_dtype=np.float64, links_given=None, want_abs=False):
    """Per level a dict: z [B, C], u [B, h], p [B, C_prev] (the link row used; None at level 1), pred; with `want_abs` also
    U, Zp (sums of absolute values, as _foldin_ref.foldin) and Cp.  `links_given[l]` (fp32 [B, C_prev]) replaces the link of
    level l + 1's input: the evaluation then takes THOSE rows as p.  The link and the arg-max are taken from the logits
    rounded to fp32, which is what a kernel stores."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    V = levels[0]["T1"].shape[0]
    a, a_dd, keep = scalars(rowptr, col, val, dis, mode, V)
    col = np.where(keep, np.asarray(col, dtype=np.int64), 0)
    dt = sum_dtype
    B = len(rowptr) - 1
    add = a_dd.astype(dt)[:, None]
    out, z_up = [], None
    for li, lv in enumerate(levels):
        T1, P, W2, b1, b2 = (np.asarray(lv[k]).astype(dt) for k in ("T1", "P", "W2", "b1", "b2"))
        h, C = T1.shape[1], P.shape[1]
        su, sz = np.zeros((B, h), dtype=dt), np.zeros((B, C), dtype=dt)
        U, Zp = np.zeros((B, h)), np.zeros((B, C))
        for d in range(B):
            tu, tz = np.zeros(h, dtype=dt), np.zeros(C, dtype=dt)
            for j in range(rowptr[d], rowptr[d + 1]):      # CSR order, from zero
                if keep[j]:
                    tu = tu + a[j].astype(dt) * T1[col[j]]
                    tz = tz + a[j].astype(dt) * P[col[j]]
            su[d], sz[d] = tu, tz
            if want_abs:
                sl = slice(rowptr[d], rowptr[d + 1])
                aa = np.abs(a[sl].astype(np.float64))
                U[d] = aa @ np.abs(T1[col[sl]].astype(np.float64))
                Zp[d] = aa @ np.abs(P[col[sl]].astype(np.float64))
        p = None
        if li:
            Wh = np.asarray(lv["Wh"]).astype(dt)
            if links_given is not None and links_given[li - 1] is not None:
                p = np.asarray(links_given[li - 1], dtype=F32)
            elif lv["link"] == ONE_HOT:
                p = one_hot_rows(z_up)
            else:
                p = softmax_rows(z_up, F32 if dt == F32 else np.float64)
            if lv["link"] == ONE_HOT:
                s = Wh[R.first_argmax(p)] if B else np.zeros((0, h), dtype=dt)     # the row itself
                sabs = np.abs(s.astype(np.float64))
            else:
                s = np.zeros((B, h), dtype=dt)
                for c in range(Wh.shape[0]):               # c in order from zero
                    s = s + p[:, c:c + 1].astype(dt) * Wh[c][None, :]
                sabs = np.abs(p.astype(np.float64)) @ np.abs(Wh.astype(np.float64))
            su = su + add * s
            U = U + np.abs(a_dd.astype(np.float64))[:, None] * sabs
        u = su + b1[None, :]
        if lv["act"] == R.ACT_RELU:
            u = np.where(u < 0, dt(0), u)
        y = np.zeros((B, C), dtype=dt)
        for k in range(h):                                  # k in order
            y = y + u[:, k:k + 1] * W2[k][None, :]
        z = (sz + add * y) + b2[None, :]
        z_up = z.astype(F32)
        res = {"z": z, "u": u, "p": p, "pred": R.first_argmax(z_up), "a_dd": a_dd}
        if want_abs:
            res.update(U=U + np.abs(b1.astype(np.float64))[None, :], Zp=Zp, Cp=(levels[li - 1]["P"].shape[1] if li else 0))
        out.append(res)
    return out


def float_bounds(rowptr, res, lv):
    """(bu, bz) of one level, as _foldin_ref.float_bounds, for an evaluation that takes the SAME fp32 link rows p: s^l costs
    C_prev FMAs and enters through one more (a_dd s + sum), so a term of u carries at most n + C_prev + 2 roundings:
        |du_k| <= gamma_{n + C_prev + 2} U_k,   U = sum_j |a_j||T1[w_j]| + a_dd sum_c |p_c||Wh[c]| + |b1|
    and z is _foldin_ref's bound on the computed u: gamma_{n+h+3} (Zp + a_dd (|u| + du)|W2| + |b2|) + a_dd (du |W2|)."""
    n = np.diff(np.asarray(rowptr)).astype(np.float64)
    h = lv["T1"].shape[1]
    bu = R.gamma(n + res["Cp"] + 2)[:, None] * res["U"]
    aw = np.abs(np.asarray(lv["W2"], dtype=np.float64))
    add = np.abs(np.asarray(res["a_dd"], dtype=np.float64))[:, None]
    bz = R.gamma(n + h + 3)[:, None] * (res["Zp"] + add * ((np.abs(res["u"]) + bu) @ aw)
                                        + np.abs(np.asarray(lv["b2"], dtype=np.float64))[None, :]) + add * (bu @ aw)
    return bu, bz


def lds_bytes(hs, Cs, docs_per_workgroup=16):
    """tgcn_foldin_levels_lds_bytes restated: W2 (tight, rounded up to 4), Wh rows padded to 4, the biases once, and per wave
    a slice with every level's u and z."""
    r4 = lambda v: (v + 3) & ~3                            # noqa: E731
    w = sum(r4(h * C) for h, C in zip(hs, Cs)) + sum(Cs[l - 1] * r4(hs[l]) for l in range(1, len(hs)))
    per = sum(r4(h) + r4(C) for h, C in zip(hs, Cs))
    return 4 * (w + (1 + docs_per_workgroup) * per)
