"""The fold-in definition (include/tgcn.h `tgcn_foldin_two_layer`) restated in numpy, and the frozen tables
of the CPU oracles.  Test infrastructure; nothing under pytextgcn_amd/ imports this.

The scalars of a document -- deg_d, dis_d, a_j, a_dd -- are specified bit for bit and are computed here in fp32 by the
definition's own rules.  The sums over j and k are evaluated in `sum_dtype`: float64 for the truth the float family's bound is
taken against (and for the exact family, whose dyadic operands make float64 exact), float32 for a plain fp32 restatement
(multiply, then add, in the definition's order)."""
import numpy as np
import torch

F32 = np.float32
REFERENCE, ACCURATE = "reference", "accurate"
ACT_NONE, ACT_RELU = 0, 1


def doc_dis(t, mode):
    """dis_d (fp32) of a document with the weights `t` (fp32, CSR order)."""
    t = np.asarray(t, dtype=F32)
    if mode == REFERENCE:
        s = F32(0.0)
        for v in t:                                    # ONE fp32 accumulator, j in order
            s = F32(s + v)
        deg = F32(s + F32(1.0))                        # the loop's 1.0 last
    else:
        part = np.zeros(64, dtype=np.float64)
        for j in range(0, t.size, 64):                 # lane j % 64 sums its entries in order
            chunk = t[j:j + 64].astype(np.float64)
            part[:chunk.size] = part[:chunk.size] + chunk
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):               # the butterfly
            part = part + part[lanes ^ off]
        deg = F32(part[0] + 1.0)                       # rounded to fp32 once
    with np.errstate(divide="ignore"):
        d = F32(1.0) / np.sqrt(deg, dtype=F32)
    return F32(0.0) if np.isinf(d) else F32(d)


def doc_scalars(rowptr, col, val, dis, mode):
    """(a [nnz] fp32, a_dd [B] fp32, dis_d [B] fp32) by the definition's associations."""
    B = len(rowptr) - 1
    val, dis = np.asarray(val, dtype=F32), np.asarray(dis, dtype=F32)
    dis_d = np.array([doc_dis(val[rowptr[d]:rowptr[d + 1]], mode) for d in range(B)], dtype=F32).reshape(B)
    row = np.repeat(np.arange(B), np.diff(rowptr))
    dw = dis[col]
    if mode == REFERENCE:
        a = (dw * val).astype(F32) * dis_d[row]
    else:
        a = val * (dw * dis_d[row]).astype(F32)
    a_dd = (dis_d * F32(1.0)).astype(F32) * dis_d
    return a.astype(F32), a_dd.astype(F32), dis_d


def foldin(rowptr, col, val, dis, mode, T1, s1, b1, act, P, W2, b2, sum_dtype=np.float64, want_abs=False):
    """(z [B, C], u [B, h]) in `sum_dtype`.  With `want_abs` also (U, Zp): the sums of absolute values
    U = sum_j |a_j||T1[w_j]| + |a_dd s1| + |b1| and Zp = sum_j |a_j||P[w_j]| that the forward-error bound is built from."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    a, a_dd, _ = doc_scalars(rowptr, col, val, dis, mode)
    dt = sum_dtype
    B, h, C = len(rowptr) - 1, T1.shape[1], P.shape[1]
    T1, P, W2, b1, b2 = (np.asarray(m).astype(dt) for m in (T1, P, W2, b1, b2))
    s1 = np.zeros(h, dtype=dt) if s1 is None else np.asarray(s1).astype(dt)
    u, zp = np.zeros((B, h), dtype=dt), np.zeros((B, C), dtype=dt)
    U, Zp = np.zeros((B, h)), np.zeros((B, C))
    for d in range(B):
        su, sz = np.zeros(h, dtype=dt), np.zeros(C, dtype=dt)
        for j in range(rowptr[d], rowptr[d + 1]):      # CSR order, from zero
            su = su + a[j].astype(dt) * T1[col[j]]
            sz = sz + a[j].astype(dt) * P[col[j]]
        u[d], zp[d] = su, sz
        if want_abs:
            sl = slice(rowptr[d], rowptr[d + 1])
            aa = np.abs(a[sl].astype(np.float64))
            U[d] = aa @ np.abs(T1[col[sl]].astype(np.float64))
            Zp[d] = aa @ np.abs(P[col[sl]].astype(np.float64))
    add = a_dd.astype(dt)[:, None]
    u = (u + add * s1[None, :]) + b1[None, :]
    if act == ACT_RELU:
        u = np.where(u < 0, dt(0), u)
    y = np.zeros((B, C), dtype=dt)
    for k in range(h):                                  # k in order
        y = y + u[:, k:k + 1] * W2[k][None, :]
    z = (zp + add * y) + b2[None, :]
    if want_abs:
        U = U + np.abs(a_dd.astype(np.float64))[:, None] * np.abs(s1.astype(np.float64))[None, :] + np.abs(b1.astype(np.float64))
        return z, u, U, Zp
    return z, u


def first_argmax(z):
    """tgcn_masked_ce_pred's rule: the first index that holds the row maximum (0 for a row without one)."""
    z = np.asarray(z)
    if z.shape[0] == 0:
        return np.zeros(0, dtype=np.int32)
    return np.argmax(z, axis=1).astype(np.int32)       # numpy returns the first occurrence


def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-24: the bound of k fp32 roundings in a row."""
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def float_bounds(rowptr, a_dd, h, u64, U, Zp, W2, b2):
    """Per-element forward-error bounds (bu [B, h], bz [B, C]) of any fp32 evaluation of the definition in its order, against
    the float64 evaluation from the same fp32 scalars.  Derived, not measured:
      u_k  takes n FMAs, one FMA for a_dd s1 and one add for b1:  |du_k| <= gamma_{n+2} U_k;  the ReLU is 1-Lipschitz;
      z_c  takes n FMAs for the P sum, h FMAs for u W2, one FMA for a_dd (u W2) + (P sum) and one add for b2 -- at most
           n + h + 2 roundings on any term -- on the COMPUTED u, whose own error passes through a_dd |W2|:
           |dz_c| <= gamma_{n+h+3} (Zp_c + a_dd (|u| + du) |W2|_c + |b2_c|) + a_dd (du |W2|)_c."""
    n = np.diff(np.asarray(rowptr)).astype(np.float64)
    bu = gamma(n + 2)[:, None] * U
    aw = np.abs(np.asarray(W2, dtype=np.float64))
    add = np.abs(np.asarray(a_dd, dtype=np.float64))[:, None]
    bz = gamma(n + h + 3)[:, None] * (Zp + add * ((np.abs(u64) + bu) @ aw) + np.abs(np.asarray(b2, dtype=np.float64))[None, :]) \
        + add * (bu @ aw)
    return bu, bz


# ---- the frozen tables of the CPU oracles ----------------------------------------------------------------------------
def word_dis(g, mode=REFERENCE):
    """deg^-1/2 of the word nodes of the training graph `g` as oracle/gcn_oracle.py's gcn_norm sums it (the reference mode:
    index_add_ on the CPU adds in edge order, the loops sit at the tail)."""
    from oracle import gcn_oracle as O
    assert mode == REFERENCE
    N = g.x.size(0)
    ei, w = O.add_remaining_self_loops(g.edge_index, g.edge_attr, 1.0, N)
    deg = torch.zeros(N, dtype=torch.float32).index_add_(0, ei[1], w)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float("inf"), 0)
    return dis[:int(g.n_vocab)].numpy()


def gcn_forward(model, g, relu):
    """(logits, H1) of a two-layer `GCNOracle`, with the ReLU between the layers that the reference comments out
    (textgcn/lib/models.py:22) when `relu`; eval mode, so no dropout."""
    first, second = model.layers
    h1 = first(g.x, g.edge_index, g.edge_attr)
    if relu:
        h1 = torch.relu(h1)
    return second(h1, g.edge_index, g.edge_attr), h1


def rel_err(a, b):
    """BASELINE.json's measure: max|a - b| / max|b|."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0
