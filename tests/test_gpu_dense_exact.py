"""Exact sweep of the dense kernels (csrc/dense.hip) through the C ABI: every named boundary of the nn / nt / tn dispatch
(tests/_dense_cases.py), in every product form, with leading dimensions and base alignments of the test's choice.

Operands are small integers, so the fp32 result of ANY correct kernel is the float64 reference bit for bit (the bound
that makes this true is asserted per case on the CPU, tests/test_dense_cases.py): there is no tolerance anywhere in this
module.  The dropout masks come from the documented hash (tests/_dropout_hash.py), never from a kernel.

Every operand is a strided view into a pool of NaN, every result (C, column sums, the mask record) a view into a pool of
a sentinel no result can equal.  After a call: status, exact result (values and, with -0.0 normalised, bit patterns),
every sentinel outside the view still in place (gap columns of each row, the rows before and behind: a store from a
ragged last block or a column tile wider than n lands there), and a finite result (no NaN from an operand gap)."""
import numpy as np
import pytest
import torch

import _dense_cases as dc
from _arena import _Arena
from pytextgcn_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 0.15625               # finite, exact in fp32 and not an integer: no result of the sweep can equal it
BITS_SENTINEL = 0x5A5A5A5A


class _Pools:
    def __init__(self, dev):
        self.dev = dev
        self.nan = self.out = self.bits = None
        self.seed = torch.tensor([dc.SEED - (1 << 64)], dtype=torch.int64, device=dev)
        self.ws = None

    def workspace(self, nbytes):
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=self.dev)
        return self.ws

    def release(self):
        self.nan = self.out = self.bits = self.ws = None
        dc._reference.cache_clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def pools(cuda):
    p = _Pools(cuda)
    yield p
    p.release()


@pytest.fixture
def lib(cuda, request):
    lib = _lib.load()
    before = lib.tgcn_set_gemm_split(0)                   # the fp32 kernels are the subject (and the ones that record)
    request.addfinalizer(lambda: lib.tgcn_set_gemm_split(before))
    return lib


def _exact(got, want_np, what, case):
    want = torch.from_numpy(np.ascontiguousarray(want_np)).to(got.device)
    assert got.shape == want.shape, (what, case)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values (an operand gap reached the result) {case}"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, c = (int(v) for v in bad[0])
        pytest.fail(f"{what} differs at {bad.shape[0]} of {got.numel()} elements, first [{r}, {c}]: "
                    f"{float(got[r, c])} != {float(want[r, c])}  {case}")
    assert torch.equal((got + 0.0).contiguous().view(torch.int32), (want + 0.0).view(torch.int32)), (what, case)


def run_case(lib, pools, c, record=None, expect=_lib.OK):
    """One call of the case's entry point on guarded, strided buffers and all the checks of the module docstring.
    record = (int32 tensor, first element, stride): a consumer reads THAT record instead of one encoded here.
    expect: a status other than TGCN_OK -- the call must return it and leave every result buffer as it was."""
    ref, lay = dc.reference(c), dc.layout(c)
    (ra, wa), (rb, wb), (rc, wc) = dc.shapes(c)
    drop, colsum, recorded = dc.has_drop(c.form), dc.has_colsum(c.form), "recorded" in c.form
    mrows, mwidth = dc.mask_shape(c)
    words = dc.mask_words(mwidth)
    writes_record = recorded and c.family == "nn"

    ins = _Arena(pools, "nan", torch.float32)
    ia, ib = ins.take(ra, wa, lay.lda, lay.off_a), ins.take(rb, wb, lay.ldb, lay.off_b)
    ins.fill(float("nan"))
    ins.view(ia).copy_(torch.from_numpy(ref["a"]))
    ins.view(ib).copy_(torch.from_numpy(ref["b"]))

    outs = _Arena(pools, "out", torch.float32)
    ic = outs.take(rc, wc, lay.ldc, lay.off_c)
    ics = outs.take(1, c.n, c.n, lay.off_c) if colsum else None
    outs.fill(SENTINEL)

    bits, mptr, mstride = None, None, lay.mask_stride
    if record is not None:
        mptr, mstride = record[0].data_ptr() + 4 * record[1], record[2]
    elif recorded:
        bits = _Arena(pools, "bits", torch.int32)
        im = bits.take(mrows, words, lay.mask_stride, lay.off_mask)
        bits.fill(BITS_SENTINEL)
        if not writes_record:          # the consumers read a record encoded HERE from the documented hash
            bits.view(im).copy_(torch.from_numpy(dc.encode_record(ref["keep"]).view(np.int32)))
        mptr = bits.ptr(im)

    A, B, C = ins.ptr(ia), ins.ptr(ib), outs.ptr(ic)
    seed = pools.seed.data_ptr()
    p = c.p if drop else 0.0
    if c.keys:
        assert lib.tgcn_set_dropout_row_keys(*c.keys) == _lib.OK
    try:
        if c.family == "nn":
            if not drop:
                st = lib.tgcn_gemm_nn(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, None)
            elif not recorded:
                st = lib.tgcn_gemm_nn_dropout(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed, None)
            else:
                assert expect != _lib.OK or int(lib.tgcn_dropout_mask_words(c.k, c.n)) == words
                st = lib.tgcn_gemm_nn_dropout_mask(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed, mptr, mstride,
                                                   None)
        elif c.family == "nt":
            if colsum:
                nb = int(lib.tgcn_gemm_nt_colsum_workspace_bytes(c.n))
                ws = pools.workspace(nb).data_ptr()
                if recorded:
                    st = lib.tgcn_gemm_nt_colsum_mask(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed, mptr, mstride,
                                                      outs.ptr(ics), ws, nb, None)
                else:
                    st = lib.tgcn_gemm_nt_colsum(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed if drop else None,
                                                 outs.ptr(ics), ws, nb, None)
            elif drop:
                st = lib.tgcn_gemm_nt_dropout(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed, None)
            else:
                st = lib.tgcn_gemm_nt(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, None)
        else:
            nb = int(lib.tgcn_gemm_tn_workspace_bytes(c.N, c.k, c.n))
            ws = pools.workspace(nb).data_ptr()
            if not drop:
                st = lib.tgcn_gemm_tn(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, ws, nb, None)
            elif not recorded:
                st = lib.tgcn_gemm_tn_dropout(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed, ws, nb, None)
            else:
                st = lib.tgcn_gemm_tn_dropout_mask(A, lay.lda, B, lay.ldb, C, lay.ldc, c.N, c.k, c.n, p, seed, mptr, mstride, ws,
                                                   nb, None)
    finally:
        if c.keys:
            lib.tgcn_set_dropout_row_keys(0, 0, 0)
    torch.cuda.synchronize()
    if expect != _lib.OK:
        assert st == expect, (st, expect, c)
        assert bool((outs.pool[:outs.used] == SENTINEL).all()), f"a refused call wrote to a result {c}"
        assert bits is None or bool((bits.pool[:bits.used] == BITS_SENTINEL).all()), f"a refused call wrote to the record {c}"
        return ins, outs, bits
    assert st == _lib.OK, (st, lib.tgcn_last_error().decode(), c)
    _exact(outs.view(ic), ref["c"], "C", c)
    if colsum:
        _exact(outs.view(ics), ref["colsum"][None, :], "column sums", c)
    assert outs.untouched(), f"a store outside the result view (gap columns / rows before or behind) {c}"
    if bits is not None:
        if writes_record:              # every bit of every existing column; words beyond the record keep their sentinel
            rec = bits.view(im).contiguous().cpu().numpy().view(np.uint32)
            got = dc.decode_record(rec, mwidth)
            assert (got == ref["keep"]).all(), f"record differs from the hash at {int((got != ref['keep']).sum())} bits {c}"
        else:
            assert torch.equal(bits.view(im).contiguous().cpu(), torch.from_numpy(dc.encode_record(ref["keep"]).view(np.int32))), c
        assert bits.untouched(), f"a word outside the mask record was written {c}"
    return ins, outs, bits


def _ids(cases):
    return [dc.case_id(c) for c in cases]


def _group_ids(groups):
    return [f"{g[0].family}-{g[0].form}-k{g[0].k}" for g in groups]


def run_group(lib, pools, cases, one=run_case):
    """Every case of a group, each on its own buffers; a case that fails does not hide the ones behind it: the failure
    names each failing leaf by its case id (family, form, N, k, n, layout).  A group -- the cases of one family, form and
    k -- is the pytest item, so that the sweep's items stay in proportion to the rest of the suite."""
    failures = []
    for c in cases:
        try:
            one(lib, pools, c)
        except (AssertionError, pytest.fail.Exception) as e:
            failures.append(f"{dc.case_id(c)}: {str(e)[:400]}")
    if failures:
        pytest.fail(f"{len(failures)} of {len(cases)} cases fail:\n" + "\n".join(failures), pytrace=False)


# ------------------------------------------------------------------------------------------------
# the sweep: one parametrised test per product family over the generated cases, grouped by (form, k)
# ------------------------------------------------------------------------------------------------
_NN, _NT, _TN = (dc.sweep_cases(f) for f in ("nn", "nt", "tn"))
_NN_G, _NT_G, _TN_G = (dc.grouped(cs) for cs in (_NN, _NT, _TN))


@pytest.mark.parametrize("cases", _NN_G, ids=_group_ids(_NN_G))
def test_nn_exact(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("cases", _NT_G, ids=_group_ids(_NT_G))
def test_nt_exact(lib, pools, cases):
    run_group(lib, pools, cases)


@pytest.mark.parametrize("cases", _TN_G, ids=_group_ids(_TN_G))
def test_tn_exact(lib, pools, cases):
    run_group(lib, pools, cases)


_TN_UNSTAGED = dc.grouped([c for c in _TN if c.layout in ("tight", "pad")])    # (odd and shift run unstaged anyway)


@pytest.mark.parametrize("cases", _TN_UNSTAGED, ids=_group_ids(_TN_UNSTAGED))
def test_tn_exact_with_the_staged_kernels_switched_off(lib, pools, monkeypatch, cases):
    """TGCN_TN_STAGED_OFF is read at call time: the unstaged kernels see the shapes that normally go through LDS stages"""
    monkeypatch.setenv("TGCN_TN_STAGED_OFF", "1")
    run_group(lib, pools, cases)


_SMALL = dc.grouped(dc.edge_rate_cases() + dc.keyed_cases() + dc.zero_row_cases(), by_k=False)


@pytest.mark.parametrize("cases", _SMALL, ids=[f"{g[0].family}-{g[0].form}" for g in _SMALL])
def test_rates_zero_and_one_row_keys_and_zero_rows(lib, pools, cases):
    """p = 0 is the identity and p = 1 zeros; row keys move the mask rows; N = 0 succeeds, stores nothing for nn / nt (the
    sentinel check), leaves zero column sums and a zero tn matrix (the reference of zero rows)."""
    run_group(lib, pools, cases)


_BIG = dc.big_cases()


@pytest.mark.parametrize("case", _BIG, ids=_ids(_BIG))
def test_rows_beyond_one_pass_of_the_persistent_grid(lib, pools, case):
    """nn / nt at an N whose 32-row blocks exceed four per workgroup of any grid (the persistent loop runs), tn past
    512 * 1024 rows (the partial tiles stop growing): entries narrowed so that the bound still holds."""
    try:
        run_case(lib, pools, case)
    finally:
        pools.release()


# ------------------------------------------------------------------------------------------------
# the record of the forward product feeds the two gradient products
# ------------------------------------------------------------------------------------------------
_CHAIN = dc.grouped([c for c in _NN if c.form == "recorded" and c.layout == "pad" and c.N in (33, 1025)])


@pytest.mark.parametrize("cases", _CHAIN, ids=_group_ids(_CHAIN))
def test_record_of_the_forward_product_feeds_both_gradient_products(lib, pools, cases):
    """tgcn_gemm_nn_dropout_mask's record (checked against the hash inside run_case), handed as it is to
    tgcn_gemm_tn_dropout_mask (same masked operand) and to tgcn_gemm_nt_colsum_mask (mask over its result): the exact
    results of the hashed forms."""
    run_group(lib, pools, cases, one=_chain)


def _chain(lib, pools, case):
    _, _, bits = run_case(lib, pools, case)
    _, _, stride, start = bits.views[0]
    record = bits.pool[:bits.used].clone()                  # keep the kernel's record, sentinels included
    N, h, C = case.N, case.k, case.n
    for family, k, n in (("tn", h, C), ("nt", C, h)):
        g = dc.make_case(family, "recorded" if family == "tn" else "colsum_recorded", N, k, n, "pad", p=case.p)
        run_case(lib, pools, g, record=(record, start, stride))
    assert torch.equal(record, bits.pool[:bits.used]), "a consumer wrote to the record"


_FOREIGN = dc.foreign_record_cases()


@pytest.mark.parametrize("case", _FOREIGN, ids=_ids(_FOREIGN))
def test_consumers_follow_the_record_not_the_hash(lib, pools, case):
    """The record handed over holds the keep mask of ANOTHER seed, at shapes whose kernel takes the record: the result is
    the record's (a kernel that hashed again would return the seed's mask and pass every case whose record equals it)."""
    run_case(lib, pools, case)


def test_record_is_refused_past_one_k_chunk_and_kept_at_256(lib, pools):
    """tgcn_dropout_mask_words is 0 for k > 256 and the _mask entry point then refuses without touching a buffer; k = 256
    still records its 8 words per row."""
    for k, n in dc.REFUSED_RECORD_SHAPES:
        assert int(lib.tgcn_dropout_mask_words(k, n)) == 0
        for lay in dc.LAYOUTS:
            run_case(lib, pools, dc.make_case("nn", "recorded", 33, k, n, lay), expect=_lib.E_INVALID)
    for k, n in dc.RECORDED_AT_THE_EDGE:
        assert int(lib.tgcn_dropout_mask_words(k, n)) == 8 == dc.mask_words(k)
        for lay in dc.LAYOUTS:
            run_case(lib, pools, dc.make_case("nn", "recorded", 129, k, n, lay))


# ------------------------------------------------------------------------------------------------
# the split-bf16 mode on the shapes it claims and on their neighbours
# ------------------------------------------------------------------------------------------------
_SPLIT = dc.grouped(dc.split_cases())


@pytest.mark.parametrize("cases", _SPLIT, ids=_group_ids(_SPLIT))
def test_split_bf16_mode_is_exact_on_small_integers(lib, pools, request, cases):
    """Integers up to 3 (and their doubles and quadruples under the dropout scale) are bf16 values: the low terms of the
    three-way split are zero and the mode must return the same exact bits -- on the shapes it claims (nn k = 200,
    33 <= n <= 64; nt k = 64, 193 <= n <= 224; tn k = 200, 33 <= n <= 64 contiguous) and on the neighbours it leaves to the
    fp32 kernels (n = 32 / 65, 192 / 225, strided tn)."""
    lib.tgcn_set_gemm_split(1)
    request.addfinalizer(lambda: lib.tgcn_set_gemm_split(0))
    assert int(lib.tgcn_dropout_mask_words(cases[0].k, cases[0].n)) == 0          # nothing records in this mode
    run_group(lib, pools, cases)


# ------------------------------------------------------------------------------------------------
# argument checks at the edges of the sweep: refused before any launch, nothing written
# ------------------------------------------------------------------------------------------------
def test_bad_leading_dimensions_alignment_and_workspace_are_refused(lib, pools):
    N, k, n = 33, 12, 20
    ins = _Arena(pools, "nan", torch.float32)
    ia, ib, ig = ins.take(N, k, 16, 0), ins.take(max(k, n), max(k, n), 24, 0), ins.take(N, n, 24, 0)
    ins.fill(1.0)
    outs = _Arena(pools, "out", torch.float32)
    ic = outs.take(max(N, k), n, 24, 0)
    ics = outs.take(1, n, n, 0)
    outs.fill(SENTINEL)
    A, B, G, C = ins.ptr(ia), ins.ptr(ib), ins.ptr(ig), outs.ptr(ic)
    seed = pools.seed.data_ptr()
    nbc = int(lib.tgcn_gemm_nt_colsum_workspace_bytes(n))
    nbt = int(lib.tgcn_gemm_tn_workspace_bytes(N, k, n))
    ws = pools.workspace(max(nbc, nbt)).data_ptr()
    INV, WSP = _lib.E_INVALID, _lib.E_WORKSPACE
    # (lda, A, ldb, ldc) variations for nn and nt; ldb must reach n for nn and k for nt
    for fam, wb in (("nn", n), ("nt", k)):
        plain = getattr(lib, f"tgcn_gemm_{fam}")
        dropf = getattr(lib, f"tgcn_gemm_{fam}_dropout")
        for lda, a, ldb, ldc in ((k - 4, A, 24, 24), (16, A, wb - 1, 24), (16, A, 24, n - 1), (k + 1, A, 24, 24), (14, A, 24, 24),
                                 (16, A + 4, 24, 24), (16, A + 8, 24, 24)):
            assert plain(a, lda, B, ldb, C, ldc, N, k, n, None) == INV, (fam, lda, ldb, ldc)
            assert dropf(a, lda, B, ldb, C, ldc, N, k, n, 0.5, seed, None) == INV, (fam, lda, ldb, ldc)
        assert plain(A, 16, B, 24, C, 24, N, 0, n, None) == INV and plain(A, 16, B, 24, C, 24, -1, k, n, None) == INV
        assert dropf(A, 16, B, 24, C, 24, N, k, n, 1.5, seed, None) == INV
        assert dropf(A, 16, B, 24, C, 24, N, k, n, 0.5, None, None) == INV
    assert lib.tgcn_gemm_nt_colsum(A, k - 4, B, 24, C, 24, N, k, n, 0.0, None, outs.ptr(ics), ws, nbc, None) == INV
    assert lib.tgcn_gemm_nt_colsum(A, 16, B, 24, C, 24, N, k, n, 0.0, None, outs.ptr(ics), ws, nbc - 1, None) == WSP
    # tn: any lda / ldg / ldc that reaches the width; a workspace one byte short
    for lda, ldg, ldc in ((k - 1, 24, 24), (16, n - 1, 24), (16, 24, n - 1)):
        assert lib.tgcn_gemm_tn(A, lda, G, ldg, C, ldc, N, k, n, ws, nbt, None) == INV
        assert lib.tgcn_gemm_tn_dropout(A, lda, G, ldg, C, ldc, N, k, n, 0.5, seed, ws, nbt, None) == INV
    assert lib.tgcn_gemm_tn(A, 16, G, 24, C, 24, N, k, n, ws, nbt - 1, None) == WSP
    assert lib.tgcn_gemm_tn_dropout(A, 16, G, 24, C, 24, N, k, n, 0.5, seed, ws, nbt - 1, None) == WSP
    assert lib.tgcn_gemm_tn(A, 16, G, 24, C, 24, N, k, n, None, nbt, None) == WSP
    # a record too narrow for its operand
    bits = _Arena(pools, "bits", torch.int32)
    im = bits.take(N, 8, 8, 0)
    bits.fill(BITS_SENTINEL)
    M = bits.ptr(im)
    assert lib.tgcn_gemm_nn_dropout_mask(A, 16, B, 24, C, 24, N, k, n, 0.5, seed, M, dc.mask_words(k) - 1, None) == INV
    assert lib.tgcn_gemm_tn_dropout_mask(A, 16, G, 24, C, 24, N, k, n, 0.5, seed, M, dc.mask_words(k) - 1, ws, nbt, None) == INV
    assert lib.tgcn_gemm_nt_colsum_mask(A, 16, B, 24, C, 24, N, k, n, 0.5, seed, M, dc.mask_words(n) - 1, outs.ptr(ics), ws, nbc,
                                        None) == INV
    torch.cuda.synchronize()
    assert bool((outs.pool[:outs.used] == SENTINEL).all()) and bool((bits.pool[:bits.used] == BITS_SENTINEL).all())


def test_nt_of_217_to_224_columns_takes_any_legal_row_stride(lib, pools):
    """The unrolled nt kernel of 216 < k <= 224 reads a row's last piece up to round_up(k, 4): the header's contract (lda a
    multiple of 4) makes every legal lda reach that far, so lda == k exists only for k = 220 and 224 -- exact there, at
    lda == round_up(k, 4) for the others (the pad columns hold NaN), and an lda == k that is not a multiple of 4 is
    refused."""
    for k in (217, 219, 220, 221, 224):
        for n in (96, 128):
            for form in ("plain", "colsum_hashed"):
                c = dc.make_case("nt", form, 129, k, n, "tight")
                assert dc.layout(c).lda == (k + 3) // 4 * 4
                run_case(lib, pools, c)
        if k % 4:
            a = torch.ones(4 * k + 8, device=pools.dev)
            b = torch.ones(96 * k, device=pools.dev)
            out = torch.full((4 * 96,), SENTINEL, device=pools.dev)
            assert lib.tgcn_gemm_nt(a.data_ptr(), k, b.data_ptr(), k, out.data_ptr(), 96, 4, k, 96, None) == _lib.E_INVALID
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all())
