"""The routed (per-label) fold-in definition (include/tgcn.h `tgcn_foldin_routed`) restated in numpy, on top of
tests/_foldin_ref.py and tests/_foldin_levels_ref.py.  Test infrastructure; nothing under pytextgcn_amd/ imports this.

A network is a dict: T1 [V, h], P [V, C], W2 [h, C], b1, b2, act.  `nets[0]` is the top network (None: there is none, the
route is given), `nets[1 + k]` member k.  A routed document is the two-layer definition (one level of `foldin_levels`, which
skips the columns outside [0, V) as the kernels do) on the top tables, then on member `route`'s tables."""
import numpy as np

import _foldin_levels_ref as LR
import _foldin_ref as R

F32 = np.float32


def sub_csr(rowptr, col, val, docs):
    """The CSR rows `docs`, in that order."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    lens = np.diff(rowptr)[docs]
    sel = np.concatenate([np.arange(rowptr[d], rowptr[d + 1]) for d in docs] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(col)[sel], np.asarray(val)[sel]


def two_layer(rowptr, col, val, dis, mode, net, sum_dtype=np.float64, want_abs=False):
    """One network on every row: dict z, u, pred, a_dd (and U, Zp, Cp with `want_abs`)."""
    lv = dict(net, Wh=None, link=None)
    return LR.foldin_levels(rowptr, col, val, dis, mode, [lv], sum_dtype, want_abs=want_abs)[0]


def foldin_routed(rowptr, col, val, dis, mode, nets, route_in=None, sum_dtype=np.float64, want_bounds=False):
    """dict: top (the top network's `two_layer`, None with `route_in`), route int32 [B], z [B, Cmax] (-inf behind C_k and in
    the rows of a route outside [0, K)), u [B, h] (zeros there), pred int64 [B] (local; -1 there).  With `want_bounds` also
    bu, bz (and top_bu, top_bz): _foldin_levels_ref.float_bounds per element, 0 where nothing is computed, and U / Zp-based
    `absz` [B, Cmax], the sum of absolute values behind every logit (for the exact family's unit count)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    B, K = len(rowptr) - 1, len(nets) - 1
    h, cmax = nets[1]["T1"].shape[1], max(n["P"].shape[1] for n in nets[1:])
    out = {"top": None}
    if route_in is None:
        top = two_layer(rowptr, col, val, dis, mode, nets[0], sum_dtype, want_bounds)
        out["top"] = top
        route = top["pred"].astype(np.int32)                       # the first arg-max of the logits rounded to fp32
        if want_bounds:
            out["top_bu"], out["top_bz"] = LR.float_bounds(rowptr, top, nets[0])
    else:
        route = np.asarray(route_in, dtype=np.int32)
    z = np.full((B, cmax), -np.inf, dtype=sum_dtype)
    u = np.zeros((B, h), dtype=sum_dtype)
    pred = np.full(B, -1, dtype=np.int64)
    bu, bz, absz, absu = np.zeros((B, h)), np.zeros((B, cmax)), np.zeros((B, cmax)), np.zeros((B, h))
    for k in np.unique(route):
        if not 0 <= k < K:
            continue
        docs = np.nonzero(route == k)[0]
        net = nets[1 + k]
        C = net["P"].shape[1]
        rp, cj, vj = sub_csr(rowptr, col, val, docs)
        r = two_layer(rp, cj, vj, dis, mode, net, sum_dtype, want_bounds)
        z[docs, :C], u[docs], pred[docs] = r["z"], r["u"], r["pred"]
        if want_bounds:
            b_u, b_z = LR.float_bounds(rp, r, net)
            bu[docs], bz[docs, :C] = b_u, b_z
            add = np.abs(r["a_dd"].astype(np.float64))[:, None]
            absu[docs] = r["U"]
            absz[docs, :C] = r["Zp"] + add * (np.abs(r["u"]) @ np.abs(net["W2"].astype(np.float64))) + \
                np.abs(net["b2"].astype(np.float64))[None, :]
    out.update(route=route, z=z, u=u, pred=pred)
    if want_bounds:
        out.update(bu=bu, bz=bz, absz=absz, absu=absu)
    return out


def global_pred(pred, route, class_map, Cs):
    """`pred` through perlabel.column_class_map's layout: class_map[seg_k + local], -1 stays."""
    seg = np.concatenate([[0], np.cumsum([(c + 3) & ~3 for c in Cs])])
    out = np.full(pred.shape, -1, dtype=np.int64)
    ok = pred >= 0
    out[ok] = np.asarray(class_map)[seg[route[ok]] + pred[ok]]
    return out


def lds_bytes(hs, Cs, docs_per_workgroup=16):
    """tgcn_foldin_routed_lds_bytes restated: per network that takes part (hs[0] == 0: no top network) W2 (tight, rounded up
    to 4) and b2 (rounded up to 4), and per wave one slice of the widest u and the widest z."""
    r4 = lambda v: (v + 3) & ~3                            # noqa: E731
    nets = [(h, C) for m, (h, C) in enumerate(zip(hs, Cs)) if m or h]
    w = sum(r4(h * C) + r4(C) for h, C in nets)
    return 4 * (w + docs_per_workgroup * (max(r4(h) for h, _ in nets) + max(r4(C) for _, C in nets)))
