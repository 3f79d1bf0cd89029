"""The kernels on operands past the byte sizes where their addressing changes: 2^31 bytes (a byte offset turns negative
as a signed int), 0xFFFF0000 bytes (the largest operand the narrow SpMM kernel `k_spmm_subb` addresses through a buffer
descriptor with 32-bit offsets; beyond it the launcher takes the full-wave `k_spmm_gather`), 4 GiB and 2^31 elements.

Large extents come from few rows: an operand is a strided view `buf.view(n, ld)[:, :F]` of one big buffer whose gaps
are NaN, so a read of a wrong row, or past a row's end, shows up as a non-finite result while the float64 truth on the
host stays a few thousand rows.  Every case asserts that its extent lies in the window it is named for."""
import numpy as np
import pytest
import torch

from _dropout_hash import keep_mask
from pytextgcn_amd import _lib, dense
from pytextgcn_amd.plan import GraphPlan, colsum
from test_gpu_parity import TOL, rel_err, row_rel_err

pytestmark = pytest.mark.gpu

GiB = 1 << 30
SUBB_LIMIT = 0xFFFF0000          # launch_vec (csrc/spmm.hip): largest operand extent of the buffer-addressed kernel


def _extent(n, F, ld):
    """bytes from the first element of row 0 to the end of row n - 1 (what the SpMM launcher compares with its limit)"""
    return ((n - 1) * ld + F) * 4


def _ld_below(n, F, target):
    """the largest row stride (a multiple of 4 floats) whose extent is <= target bytes"""
    return (target // 4 - F) // (n - 1) // 4 * 4


def _need(nbytes, cuda):
    free = torch.cuda.mem_get_info(cuda)[0]
    if free < nbytes + GiB:
        pytest.skip(f"needs {nbytes / 1e9:.1f} GB of free device memory, {free / 1e9:.1f} GB free")


def _release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _nan_buffer(nfloats, cuda):
    _need(4 * nfloats, cuda)
    return torch.full((nfloats,), float("nan"), device=cuda)


def _csr_product64(plan, x64, transpose=False):
    """float64 product of the plan's own exported CSR with a float64 host operand"""
    rp, col, val = (t.cpu() for t in plan.export_csr(transpose))
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1), (rp[1:] - rp[:-1]).long())
    y = torch.zeros(rp.numel() - 1, x64.size(1), dtype=torch.float64)
    y.index_add_(0, rows, val.double().unsqueeze(1) * x64[col.long()])
    return y, (rp[1:] == rp[:-1])


def _check_rows(got, ref, case):
    """finite where the truth is finite (a wrong-row read hits the NaN gaps), +-inf where it is, and 1e-5 in the max
    norm and row by row on the finite rows"""
    got = got.detach().cpu().double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), case
    assert torch.equal(got[~fin], ref[~fin]), case
    ok = fin.all(1)
    e, er = rel_err(got[ok], ref[ok]), row_rel_err(got[ok], ref[ok])
    assert e < TOL and er < TOL, (case, e, er)


# ------------------------------------------------------------------------------------------------
# A. narrow SpMM on one operand buffer around 2^31 bytes, the buffer-path limit and 6 GiB
# ------------------------------------------------------------------------------------------------
_N = 4100                       # >= 4096 operand rows: the dense hot block can be chosen
_HUBS = range(1, 9)
_EMPTY_FWD = range(2000, 2050)  # rows of M without entries
_EMPTY_T = range(3000, 3050)    # columns of M without entries: rows of M^T without entries


def _narrow_operator(cuda):
    """An explicit asymmetric N x N operator: eight hub rows and hub columns of ~1000-3700 entries (far beyond the
    384-entry work item: split into segments, or the dense hot block), a sparse random background, entries in the
    last operand row and column, node 0 with its diagonal entry only (nobody else gathers operand row 0), and rows /
    columns without entries."""
    gen = torch.Generator().manual_seed(2024)
    n = _N
    rows, cols = [], []
    for h in _HUBS:
        others = torch.nonzero(torch.rand(n, generator=gen) < 0.9 / (1 + 0.35 * (h - 1))).flatten()
        others = others[others != h]
        rows += [torch.full_like(others, h), others]
        cols += [others, torch.full_like(others, h)]
    bg = torch.randint(0, n, (2, 4 * n), generator=gen)
    last = torch.tensor([[5, n - 1, 1, n - 1, n - 1], [n - 1, 7, n - 1, 1, n - 1]])
    r, c = torch.cat(rows + [bg[0], last[0]]), torch.cat(cols + [bg[1], last[1]])
    keep = (r != 0) & (c != 0) & ~torch.isin(r, torch.tensor(list(_EMPTY_FWD))) & \
        ~torch.isin(c, torch.tensor(list(_EMPTY_T)))
    r, c = torch.cat([r[keep], torch.zeros(1, dtype=torch.long)]), torch.cat([c[keep], torch.zeros(1, dtype=torch.long)])
    v = torch.rand(r.numel(), generator=gen) + 0.05
    return r.to(cuda), c.to(cuda), v.to(cuda)


@pytest.fixture(scope="module")
def narrow_plans(cuda):
    r, c, v = _narrow_operator(cuda)
    import os
    old = os.environ.pop("TGCN_HOT_ROWS", None)
    try:
        hot = GraphPlan.from_coo(r, c, v, _N, _N, with_transpose=True)
        os.environ["TGCN_HOT_ROWS"] = "0"
        plain = GraphPlan.from_coo(r, c, v, _N, _N, with_transpose=True)
    finally:
        os.environ.pop("TGCN_HOT_ROWS", None)
        if old is not None:
            os.environ["TGCN_HOT_ROWS"] = old
    assert hot.query(_lib.Q_HOT_ROWS) > 0 and hot.query(_lib.Q_HOT_ROWS_T) > 0      # the default picks the hot block
    assert plain.query(_lib.Q_HOT_ROWS) == 0 and plain.query(_lib.Q_HOT_ROWS_T) == 0
    for t in (False, True):
        rp = plain.export_csr(t)[0].long()
        assert int((rp[1:] - rp[:-1]).max()) > 2000                               # long rows: segments
    yield hot, plain
    hot.close()
    plain.close()
    _release()


def _window(name, n, F):
    """(row stride, extent) of the named window, the extent asserted to lie in it"""
    if name == "below_2g":
        ld = _ld_below(n, F, (1 << 31) - 1)
        ext = _extent(n, F, ld)
        assert (1 << 31) - 4 * ld < ext < (1 << 31)
    elif name == "above_2g":                     # the LAST row starts past 2^31 (a negative signed offset)
        ld = -(-(1 << 31) // (4 * (n - 1)) // 4) * 4
        ld = ld + 4 if (n - 1) * ld * 4 < (1 << 31) else ld
        ext = _extent(n, F, ld)
        assert (n - 1) * ld * 4 >= (1 << 31) and (1 << 31) < ext <= (1 << 31) + 4 * ld
    elif name == "at_limit":
        ld = _ld_below(n, F, SUBB_LIMIT)
        ext = _extent(n, F, ld)
        assert SUBB_LIMIT - 4 * ld < ext <= SUBB_LIMIT
    elif name == "above_limit":
        ld = _ld_below(n, F, SUBB_LIMIT) + 4
        ext = _extent(n, F, ld)
        assert SUBB_LIMIT < ext <= SUBB_LIMIT + 4 * ld
    else:
        assert name == "6g"
        ld = _ld_below(n, F, 6 * GiB)
        ext = _extent(n, F, ld)
        assert 6 * GiB - 4 * ld < ext <= 6 * GiB and ext > (1 << 32) + GiB
    return ld, ext


@pytest.mark.parametrize("window", ["below_2g", "above_2g", "at_limit", "above_limit", "6g"])
def test_narrow_spmm_on_one_operand_buffer_around_the_offset_limits(cuda, narrow_plans, window):
    """F = 64 (16 lanes per row) and 128 (32 lanes): forward and transposed block, plain and accumulate forms, with the
    dense hot block (the default here) and without it (long rows as segments); operand row 0 holds inf in the plan
    without the hot block (nobody but row 0 itself gathers it: a padding offset that wraps would turn 0 * inf into nan
    elsewhere).  Against float64 products of the plans' own CSR."""
    hot, plain = narrow_plans
    n = _N
    ld_max = max(_window(window, n, F)[0] for F in (64, 128))
    buf = _nan_buffer(n * ld_max, cuda)
    gen = torch.Generator().manual_seed(len(window))
    for F in (64, 128):
        ld, ext = _window(window, n, F)
        buf.fill_(float("nan"))
        x = buf[:n * ld].view(n, ld)[:, :F]
        assert x.stride() == (ld, 1) and x.data_ptr() % 16 == 0
        x_host = torch.randn(n, F, generator=gen)
        x.copy_(x_host)
        y0 = torch.randn(n, F, generator=gen)
        for plan, poison in ((hot, False), (plain, True)):
            xh = x_host.clone()
            if poison:
                xh[0, :60] = float("inf")
                x[0, :60] = float("inf")
            x64 = xh.double()
            for transpose in (False, True):
                case = (window, F, ext, "hot" if plan is hot else "plain", "T" if transpose else "fwd")
                ref, empty = _csr_product64(plan, x64, transpose)
                designated = list(_EMPTY_T if transpose else _EMPTY_FWD)
                assert bool(empty[designated].all()) and int(empty.sum()) < 100
                _check_rows(plan.spmm(x, transpose=transpose), ref, case)
                # accumulate: sums added on the rows that hold entries, the others not touched (bit for bit)
                out = y0.to(cuda)
                plan.spmm(x, transpose=transpose, out=out, accumulate=True)
                out = out.cpu()
                assert torch.equal(out[empty], y0[empty]), case
                _check_rows(out[~empty], (y0.double() + ref)[~empty], case + ("acc",))
            if poison:
                x[0].copy_(x_host[0])
        del x
    del buf
    _release()


# ------------------------------------------------------------------------------------------------
# B. the real tall shape: the c5 graph (8 M nodes) with 72 and 128 columns
# ------------------------------------------------------------------------------------------------
def _chunks(n, step=1 << 20):
    return ((i, min(n, i + step)) for i in range(0, n, step))


def _dot64(a, b):
    return sum(float((a[i:j].double() * b[i:j].double()).sum()) for i, j in _chunks(a.size(0)))


@pytest.fixture(scope="module")
def c5plan(cuda, c5case):
    """the c5 operator (accurate degree sums: symmetric, one stored copy), shared by the three operand forms"""
    g = c5case.g
    plan = GraphPlan(g.edge_index, g.edge_attr, c5case.N, degree_sum="accurate")
    assert plan.symmetric
    yield plan
    plan.close()
    _release()


@pytest.mark.parametrize("F,ld", [(72, 72), (128, 128), (128, 136)])
def test_c5_narrow_operand_past_2g_at_and_past_the_limit(cuda, c5case, c5plan, F, ld):
    """F = 72 contiguous: 2.3 GB, the buffer path past 2^31; F = 128 contiguous: 4.10 GB, just under the limit; F = 128
    at row stride 136: past 4 GiB, the full-wave fallback.  Sampled rows (the heaviest, and rows that gather operand rows
    past the 2^31- and 4 GiB-offset points) against float64, the whole result against the split-operand product (the
    full-wave kernel) and the adjoint identity <Mx, z> = <x, M^T z>."""
    N, plan = c5case.N, c5plan
    ext = _extent(N, F, ld)
    if F == 72:
        assert (1 << 31) < ext <= SUBB_LIMIT
    elif ld == F:
        assert SUBB_LIMIT - 256 * (1 << 20) < ext <= SUBB_LIMIT
    else:
        assert ext > (1 << 32)
    _need(4 * N * ld * 3 + 4 * GiB, cuda)
    gen = torch.Generator(device=cuda).manual_seed(F + ld)
    buf = torch.full((N * ld,), float("nan"), device=cuda)
    x = buf.view(N, ld)[:, :F]
    x.normal_(generator=gen)
    y = plan.spmm(x)
    assert all(bool(torch.isfinite(y[i:j]).all()) for i, j in _chunks(N))
    # sampled rows against float64
    rp, col, val = plan.export_csr()
    deg = rp[1:] - rp[:-1]
    r2g = -(-(1 << 31) // (4 * ld))                 # first operand row at a byte offset >= 2^31
    r4g = -(-(1 << 32) // (4 * ld))
    pick = [deg.long().topk(6).indices, torch.arange(N - 3, N, device=cuda),
            torch.randint(0, N, (100,), device=cuda, generator=gen),
            torch.randint(r2g, N, (60,), device=cuda, generator=gen)]
    if r4g < N:
        pick.append(torch.randint(r4g, N, (60,), device=cuda, generator=gen))
    rows = torch.unique(torch.cat(pick))
    # every picked row past the offset points gathers its own (self-loop) operand row there
    assert int((rows >= r2g).sum()) >= 60 and (r4g >= N or int((rows >= r4g).sum()) >= 60)
    ref = torch.zeros(rows.numel(), F, dtype=torch.float64, device=cuda)
    bounds = torch.stack([rp[rows], rp[rows + 1]], 1).tolist()
    for k, (lo, hi) in enumerate(bounds):               # one float64 vector-matrix product per row (heavy rows in chunks)
        for i, j in _chunks(hi - lo):
            ref[k] += val[lo + i:lo + j].double() @ x[col[lo + i:lo + j].long()].double()
    got = y[rows]
    assert rel_err(got, ref) < TOL and row_rel_err(got, ref) < TOL, (F, ld)
    del rp, col, val, deg, ref
    # the whole result against the full-wave kernel (a split operand never takes the buffer-addressed one)
    s = N // 3
    y2 = plan.spmm(x[:s], x2=x[s:])
    e = max(float((y[i:j] - y2[i:j]).abs().max()) for i, j in _chunks(N)) / max(
        float(y2[i:j].abs().max()) for i, j in _chunks(N))
    assert e < 1e-6, (F, ld, e)
    del y2
    # adjoint identity
    z = torch.randn(N, F, device=cuda, generator=gen)
    lhs = _dot64(y, z)
    del y
    mz = plan.spmm(z, transpose=True)
    rhs = _dot64(x, mz)
    assert abs(lhs - rhs) < 1e-6 * max(abs(lhs), abs(rhs)) + 1e-2, (lhs, rhs)
    del x, buf, z, mz
    _release()


# ------------------------------------------------------------------------------------------------
# C. the fused W1 update on a parameter past 4 GiB
# ------------------------------------------------------------------------------------------------
def test_fused_w1_update_on_a_parameter_past_4g(cuda):
    """`tgcn_spmm_adam` (amsgrad) on a contiguous 4.3 M x 256 parameter (4.4 GB; state 3 x 4.4 GB more): M^T g of a
    sparse random operator with a long row at the very end, the update of ~200 sampled rows (the last ones included)
    against a float64 Adam step of the float64 (M^T g) rows."""
    P, R, F = 4_300_000, 4096, 256
    assert P * F * 4 > (1 << 32)
    _need(4 * P * F * 4 + 2 * GiB, cuda)
    gen = torch.Generator(device=cuda).manual_seed(7)
    # M is R x P: every column holds one entry, 1.5 M columns a second one, the last column 3000 more
    col = torch.cat([torch.arange(P, device=cuda), torch.randint(0, P, (1_500_000,), device=cuda, generator=gen),
                     torch.full((3000,), P - 1, device=cuda)])
    row = torch.randint(0, R, (col.numel(),), device=cuda, generator=gen)
    val = torch.rand(col.numel(), device=cuda, generator=gen) + 0.05
    plan = GraphPlan.from_coo(row, col, val, R, P, with_transpose=True)
    del row, col, val
    g = torch.randn(R, F, device=cuda, generator=gen)
    param = torch.randn(P, F, device=cuda, generator=gen)
    m = torch.randn(P, F, device=cuda, generator=gen).mul_(0.1)
    v = torch.rand(P, F, device=cuda, generator=gen).mul_(0.01).add_(0.005)
    vmax = v.clone()
    vmax[::2].add_(0.004)                   # every other row: the running maximum stays above the new v
    rows = torch.unique(torch.cat([torch.randint(0, P, (190,), device=cuda, generator=gen),
                                   torch.arange(P - 10, P, device=cuda)]))
    before = [t[rows].double().cpu() for t in (param, m, v, vmax)]
    lr, b1, b2, eps, step = 0.05, 0.9, 0.999, 1e-8, 3
    plan.spmm_adam(g, param, m, v, vmax, lr, b1, b2, eps, 0.0, step)
    after = [t[rows].double().cpu() for t in (param, m, v, vmax)]
    # float64 (M^T g) rows from the plan's own transposed CSR
    rp, cc, vv = (t.cpu() for t in plan.export_csr(transpose=True))
    assert rp.numel() == P + 1 and int(rp[P] - rp[P - 1]) > 3000
    gh = g.double().cpu()
    grad = torch.stack([(vv[rp[r]:rp[r + 1]].double().unsqueeze(1) * gh[cc[rp[r]:rp[r + 1]].long()]).sum(0)
                        for r in rows.tolist()])
    p0, m0, v0, x0 = before
    m1 = b1 * m0 + (1 - b1) * grad
    v1 = b2 * v0 + (1 - b2) * grad * grad
    x1 = torch.maximum(x0, v1)
    p1 = p0 - lr / (1 - b1 ** step) * m1 / (x1.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    for name, got, want in zip(("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"), after, (p1, m1, v1, x1)):
        assert rel_err(got, want) < TOL and row_rel_err(got, want) < TOL, name
    assert rel_err(after[0] - p0, p1 - p0) < 1e-3                  # the step itself, not only the parameter
    plan.close()
    del plan, g, param, m, v, vmax
    _release()


# ------------------------------------------------------------------------------------------------
# D. dense products past 2^31 elements and 4 GiB
# ------------------------------------------------------------------------------------------------
def test_dense_products_past_2g_elements(cuda, request):
    """gemm_nn / gemm_tn at the GCN shapes (k = 200, n = 64), gemm_nt at k = 64, n = 200 (the pipelined kernel), plain
    and with column sums, and a chunked k = 300: every tall operand and the nn result are strided views whose last row
    sits past 2^31 elements of one NaN-gapped buffer.  The dropout forms (hashed, and from the record gemm_nn leaves)
    agree bit for bit with each other and with the masked float64 products."""
    before = dense.enable_split_gemms(False)
    request.addfinalizer(lambda: dense.enable_split_gemms(before))
    N = 3000
    ld = -(-(1 << 31) // (N - 1) // 4) * 4 + 4
    assert (N - 1) * ld > (1 << 31) and (N - 1) * ld * 4 > (1 << 33)
    buf = _nan_buffer(N * ld, cuda)
    rows = buf.view(N, ld)
    xv, cv, gv, x3v = rows[:, :200], rows[:, 256:320], rows[:, 384:448], rows[:, 512:812]
    gen = torch.Generator().manual_seed(31)
    x, g, x3 = torch.randn(N, 200, generator=gen), torch.randn(N, 64, generator=gen), torch.randn(N, 300, generator=gen)
    w, w3 = torch.randn(200, 64, generator=gen), torch.randn(300, 64, generator=gen)
    xv.copy_(x); gv.copy_(g); x3v.copy_(x3)
    wd, w3d = w.to(cuda), w3.to(cuda)
    x64, g64, w64 = x.double(), g.double(), w.double()
    assert cv.stride(0) == ld and cv.data_ptr() % 16 == 0
    # plain products
    dense.gemm_nn(xv, wd, out=cv)
    assert rel_err(cv, x64 @ w64) < TOL
    assert rel_err(dense.gemm_tn(xv, gv), x64.t() @ g64) < TOL
    ref_nt = g64 @ w64.t()
    assert rel_err(dense.gemm_nt(gv, wd), ref_nt) < TOL
    got = dense.gemm_nt(gv, wd, note_colsums=True)
    assert rel_err(got, ref_nt) < TOL and rel_err(colsum(got), ref_nt.sum(0)) < 2e-5
    dense.gemm_nn(x3v, w3d, out=cv)                                       # k = 300: two k chunks accumulate into C
    assert rel_err(cv, x3.double() @ w3.double()) < TOL
    assert rel_err(dense.gemm_tn(x3v, gv), x3.double().t() @ g64) < TOL
    # dropout: the documented hash of (seed, row, column)
    p = 0.5
    seed = torch.tensor([0x5DEECE66D12345], dtype=torch.int64, device=cuda)
    keep = torch.from_numpy(keep_mask(int(seed.item()), np.arange(N, dtype=np.uint64)[:, None],
                                      np.arange(200, dtype=np.uint64)[None, :], p))
    xd = x64 * keep / (1 - p)
    ref_nt_d = ref_nt * keep / (1 - p)
    fwd = dense.gemm_nn(xv, wd, p, seed, out=cv).cpu()
    assert rel_err(fwd, xd @ w64) < TOL
    dw = dense.gemm_tn(xv, gv, p, seed)
    assert rel_err(dw, xd.t() @ g64) < TOL
    dx = dense.gemm_nt(gv, wd, p, seed)
    assert rel_err(dx, ref_nt_d) < TOL and torch.equal((dx != 0).cpu(), keep)
    dxs = dense.gemm_nt(gv, wd, p, seed, note_colsums=True)
    assert torch.equal(dxs, dx) and rel_err(colsum(dxs), ref_nt_d.sum(0)) < 2e-5
    s_hash = colsum(dxs).clone()
    fwd_r, mask = dense.gemm_nn(xv, wd, p, seed, record_mask=True, out=cv)
    assert mask is not None and torch.equal(fwd_r.cpu(), fwd)
    assert torch.equal(dense.gemm_tn(xv, gv, p, seed, mask), dw)
    dx_r = dense.gemm_nt(gv, wd, p, seed, note_colsums=True, mask=mask)
    assert torch.equal(dx_r, dx) and rel_err(colsum(dx_r), s_hash) < 1e-5
    # nothing outside the views was written: the gaps of the first and the last row are still NaN
    for r in (0, N - 1):
        assert bool(rows[r, 200:256].isnan().all() and rows[r, 320:384].isnan().all() and rows[r, 812:1024].isnan().all())
    del xv, cv, gv, x3v, rows, buf
    _release()


# ------------------------------------------------------------------------------------------------
# E. row keys of the dropout hash at and past 2^32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [(0, 0, (1 << 32) - 1031 - 1), (0, 0, (1 << 32) - 1031 + 1), (500, (1 << 32) - 250, 3 * (1 << 32) + 77),
                                  (0, 0, (1 << 40) + 12345), (700, 1 << 33, 1 << 62)])
def test_dropout_row_keys_past_2_32_are_the_documented_hash(cuda, keys):
    """tgcn_set_dropout_row_keys places row i at mask row i + key: with keys just below / across 2^32 and far above it
    the mask is the numpy restatement evaluated at those 64-bit rows (the row's high word enters the hash)."""
    N, w, p = 1031, 200, 0.3
    split, k0, k1 = keys
    seed = dense.new_seed(cuda)
    sd = int(seed.item())
    keep_gpu = (dense.gemm_nt(torch.ones(N, 1, device=cuda), torch.ones(w, 1, device=cuda), p, seed,
                              keys=keys) != 0).cpu().numpy()
    i = np.arange(N, dtype=np.uint64)
    mrow = np.where(i < split, i + np.uint64(k0), i + np.uint64(k1))[:, None]
    assert int(mrow.max()) >= (1 << 32) or int(mrow.max()) == (1 << 32) - 2
    want = keep_mask(sd, mrow, np.arange(w, dtype=np.uint64)[None, :], p)
    assert (keep_gpu == want).all(), keys
    # the high word matters: the same rows with it dropped draw another mask
    if int(mrow.max()) >= (1 << 32):
        low = keep_mask(sd, mrow & np.uint64(0xFFFFFFFF), np.arange(w, dtype=np.uint64)[None, :], p)
        assert (low != want).any()


# ------------------------------------------------------------------------------------------------
# F. side kernels with the last row past 4 GiB
# ------------------------------------------------------------------------------------------------
def test_side_kernels_on_rows_past_4g(cuda):
    """colsum, the masked cross-entropy (loss, gradient, predictions) and the row movement of the exchange
    (tgcn_rows_gather / _scatter / _reduce_ranked) on strided views whose last row starts past 4 GiB."""
    from pytextgcn_amd.functional import masked_cross_entropy
    from pytextgcn_amd.sharded import HipEngine
    n = 3000
    ld = -(-(1 << 32) // (4 * (n - 1)) // 4) * 4 + 4
    assert (n - 1) * ld * 4 > (1 << 32)
    buf = _nan_buffer(n * ld, cuda)
    rows = buf.view(n, ld)
    gen = torch.Generator().manual_seed(3)
    for F in (64, 200, 7):
        a = torch.randn(n, F, generator=gen)
        av = rows[:, :F]
        av.copy_(a)
        assert rel_err(colsum(av), a.double().sum(0)) < TOL, F
    # cross-entropy on strided logits
    C = 64
    logits = torch.randn(n, C, generator=gen) * 3
    y = torch.randint(0, C, (n,), generator=gen)
    mask = torch.rand(n, generator=gen) < 0.6
    mask[n - 1] = True
    lv = rows[:, 16:16 + C]
    lv.copy_(logits)
    lg = lv.detach().requires_grad_()
    assert lg.stride(0) == ld
    loss, pred = masked_cross_entropy(lg, y.to(cuda), mask.to(cuda), return_pred=True)
    loss.backward()
    lr = logits.double().requires_grad_()
    want = torch.nn.functional.cross_entropy(lr[mask], y[mask])
    want.backward()
    assert abs(loss.item() - want.item()) < TOL * abs(want.item())
    assert rel_err(lg.grad, lr.grad) < TOL and row_rel_err(lg.grad, lr.grad) < TOL
    assert torch.equal(pred.cpu(), logits.argmax(1))
    # row movement: gather from, scatter into and reduce into strided matrices
    eng = HipEngine()
    for F in (200, 64, 7):
        buf.fill_(float("nan"))
        x = torch.randn(n, F, generator=gen)
        xv = rows[:, :F]
        xv.copy_(x)
        idx = torch.cat([torch.randperm(n, generator=gen)[:1500], torch.tensor([n - 1])]).unique()
        assert torch.equal(eng.rows_gather(xv, idx.to(cuda)).cpu(), x[idx]), F
        yv = rows[:, 256:256 + F]
        yv.zero_()
        src = torch.randn(idx.numel(), F, generator=gen)
        eng.rows_scatter_(yv, idx.to(cuda), src.to(cuda))
        ref = torch.zeros(n, F).index_copy_(0, idx, src)
        assert torch.equal(yv.cpu(), ref), F
        W, m, K, k0 = 3, 1000, 3, 2                 # target rows k0, k0 + K, ... : the last is n - 1
        assert k0 + K * (m - 1) == n - 1
        inv = torch.full((W, m), -1, dtype=torch.int32)
        cnt = 0
        for q in range(W):
            pos = (torch.rand(m, generator=gen) < 0.7).nonzero().flatten()
            pos = torch.cat([pos, torch.tensor([m - 1])]).unique()
            inv[q, pos] = torch.arange(cnt, cnt + pos.numel(), dtype=torch.int32)
            cnt += pos.numel()
        recv = torch.randn(cnt, F, generator=gen)
        want_y = ref.clone()
        acc = torch.zeros(m, F)
        for q in range(W):
            sel = inv[q] >= 0
            acc[sel] += recv[inv[q][sel].long()]
        want_y[k0:k0 + K * m:K] += acc
        eng.reduce_ranked_(yv, recv.to(cuda), inv.to(cuda), W, m, k0, K)
        assert torch.equal(yv.cpu(), want_y), F
    del rows, buf
    _release()
