"""The layer-chain fold-in definition (include/tgcn.h `tgcn_foldin_layers`) restated in numpy, on top of
tests/_foldin_ref.py.  Test infrastructure; nothing under pytextgcn_amd/ imports this.

The document scalars are _foldin_ref's (fp32, bit for bit; an entry whose column lies outside [0, n_vocab) is left out of
the sums over j and still counts in deg_d, as _foldin_levels_ref.scalars has it).  The sums over j and k are evaluated in
`sum_dtype`.  A layer is a dict: T [V, w_l], W [w_{l-1}, w_l] (None at layer 1), b [w_l], act."""
import numpy as np

import _foldin_levels_ref as LR
import _foldin_ref as R

F32 = np.float32


def foldin_layers(rowptr, col, val, dis, mode, layers, s1=None, sum_dtype=np.float64, want_abs=False):
    """Per layer a dict: x [B, w_l] in `sum_dtype` (after the activation) and a_dd; with `want_abs` also
    A = sum_j |a_j||T^l[w_j]| + a_dd |s1| (layer 1) or a_dd (|x^{l-1}| |W_l|) (l >= 2) + |b_l|: the sum of the absolute values
    of every term of the pre-activation, which the exactness condition and the forward-error bound are built from."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    V = layers[0]["T"].shape[0]
    a, a_dd, keep = LR.scalars(rowptr, col, val, dis, mode, V)
    col = np.where(keep, np.asarray(col, dtype=np.int64), 0)
    dt = sum_dtype
    B = len(rowptr) - 1
    add = a_dd.astype(dt)[:, None]
    add64 = np.abs(a_dd.astype(np.float64))[:, None]
    out, x = [], None
    for li, ly in enumerate(layers):
        T, b = np.asarray(ly["T"]).astype(dt), np.asarray(ly["b"]).astype(dt)
        w = T.shape[1]
        s, S = np.zeros((B, w), dtype=dt), np.zeros((B, w))
        for d in range(B):
            t = np.zeros(w, dtype=dt)
            for j in range(rowptr[d], rowptr[d + 1]):      # CSR order, from zero
                if keep[j]:
                    t = t + a[j].astype(dt) * T[col[j]]
            s[d] = t
            if want_abs:
                sl = slice(rowptr[d], rowptr[d + 1])
                S[d] = np.abs(a[sl].astype(np.float64)) @ np.abs(T[col[sl]].astype(np.float64))
        if li == 0:
            s1v = np.zeros(w, dtype=dt) if s1 is None else np.asarray(s1).astype(dt)
            s = s + add * s1v[None, :]
            S = S + add64 * np.abs(s1v.astype(np.float64))[None, :]
        else:
            W = np.asarray(ly["W"]).astype(dt)
            y = np.zeros((B, w), dtype=dt)
            for k in range(W.shape[0]):                    # k in order
                y = y + x[:, k:k + 1] * W[k][None, :]
            s = s + add * y                                # fmaf(a_dd, y, sum)
            S = S + add64 * (np.abs(x.astype(np.float64)) @ np.abs(W.astype(np.float64)))
        x = s + b[None, :]
        if ly["act"] == R.ACT_RELU:
            x = np.where(x < 0, dt(0), x)
        res = {"x": x, "a_dd": a_dd}
        if want_abs:
            res["A"] = S + np.abs(b.astype(np.float64))[None, :]
        out.append(res)
    return out


def float_bounds(rowptr, res, layers):
    """Per-element forward-error bounds [B, w_l], one per layer, of any fp32 evaluation of the definition in its order against
    the float64 evaluation `res` (foldin_layers(..., np.float64, want_abs=True)) from the same fp32 scalars.  Derived, not
    measured -- _foldin_ref.float_bounds extended layer by layer:
      x^1  takes n FMAs, one FMA for a_dd s1 and one add for b_1:   |dx^1| <= gamma_{n+2} A^1          (its `bu`);
      x^l  takes n FMAs for the gathered sum, w_{l-1} FMAs for x^{l-1} W_l, one FMA for a_dd y + sum and one add for b_l: layer
           l adds w_{l-1} + 2 roundings to the n of the sum, at most n + w_{l-1} + 2 on any term (gamma_{n + w_{l-1} + 3}, as
           its `bz` has it) -- on the COMPUTED x^{l-1}, whose own error passes through a_dd |W_l|:
           |dx^l| <= gamma_{n + w_{l-1} + 3} (A^l + a_dd (dx^{l-1} |W_l|)) + a_dd (dx^{l-1} |W_l|).
    The ReLU is 1-Lipschitz, so the bound of the pre-activation holds after it; A^l is taken on the float64 |x^{l-1}|."""
    n = np.diff(np.asarray(rowptr)).astype(np.float64)
    bounds, prev = [], None
    for li, (r, ly) in enumerate(zip(res, layers)):
        if li == 0:
            b = R.gamma(n + 2)[:, None] * r["A"]
        else:
            aw = np.abs(np.asarray(ly["W"], dtype=np.float64))
            add = np.abs(np.asarray(r["a_dd"], dtype=np.float64))[:, None]
            through = add * (prev @ aw)
            b = R.gamma(n + aw.shape[0] + 3)[:, None] * (r["A"] + through) + through
        bounds.append(b)
        prev = b
    return bounds


def lds_bytes(widths, docs_per_workgroup=16):
    """tgcn_foldin_layers_lds_bytes restated: W_2 .. W_L (tight, rounded up to 4), the biases once, and per wave a slice with
    every layer's row."""
    r4 = lambda v: (v + 3) & ~3                            # noqa: E731
    w = sum(r4(widths[l - 1] * widths[l]) for l in range(1, len(widths)))
    per = sum(r4(v) for v in widths)
    return 4 * (w + per + docs_per_workgroup * per)
