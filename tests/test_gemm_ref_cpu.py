"""The library-GEMM host layer (csrc/gemm_lt.hip), the part that needs no GPU: the float64 restatement (tests/gemm_ref.py)
against torch.matmul in float64 -- a wrong restatement cannot hide a wrong GEMM --, the size-bucket rule, and the host-side
refusals of csl_gemm_f32 and csl_sum_slabs_f32, which return before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_ref as R

E_INVALID = -1                    # CSL_E_INVALID (cslicer_hip.h)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def _torch_product(transa, transb, a2, b2, bias, relu):
    a, b = torch.from_numpy(a2).double(), torch.from_numpy(b2).double()
    c = torch.matmul(a.t() if transa else a, b.t() if transb else b)
    if bias is not None:
        c = c + torch.from_numpy(bias).double()
    return (c.relu() if relu else c).numpy()


@pytest.mark.parametrize("transa", [0, 1])
@pytest.mark.parametrize("transb", [0, 1])
@pytest.mark.parametrize("bias,relu", [(False, False), (True, False), (False, True), (True, True)])
def test_restatement_is_torch_matmul_on_column_blocks(transa, transb, bias, relu):
    """every operand a block of a wider buffer, C too: the product lands in its block, the rest of C keeps its values"""
    rng = np.random.default_rng(10 * transa + transb)
    m, n, k = 13, 7, 5
    ar, ac = (k, m) if transa else (m, k)
    br, bc = (n, k) if transb else (k, n)
    abuf, bbuf = rng.standard_normal((ar + 1, ac + 3)).astype(np.float32), rng.standard_normal((br + 2, bc + 4)).astype(np.float32)
    cbuf = rng.standard_normal((m + 1, n + 5)).astype(np.float32)
    bv = rng.standard_normal(n + 2).astype(np.float32) if bias else None
    a_off, b_off, c_off = 2, (bc + 4) + 1, 3          # A from column 2, B from row 1 column 1, C from column 3
    got = R.gemm(transa, transb, m, n, k, abuf.reshape(-1)[a_off:], ac + 3, 0, bbuf.reshape(-1)[b_off:], bc + 4, 0,
                 cbuf.reshape(-1)[c_off:], n + 5, 0, 1, bv, relu)
    want = cbuf.astype(np.float64)
    want[:m, 3:3 + n] = _torch_product(transa, transb, abuf[:ar, 2:2 + ac], bbuf[1:1 + br, 1:1 + bc],
                                       None if bv is None else bv[:n], relu)
    want = want.reshape(-1)[c_off:]
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-13, atol=1e-13)
    bd = R.bound(transa, transb, m, n, k, abuf.reshape(-1)[a_off:], ac + 3, 0, bbuf.reshape(-1)[b_off:], bc + 4, 0,
                 cbuf.reshape(-1)[c_off:], n + 5, 0, 1, bv, relu)
    own = R.owned(m, n, n + 5, 0, 1, bd.shape[0])
    assert int(own.sum()) == m * n and bool((bd[~own] == 0).all()) and bool((bd[own] > 0).all())
    assert np.array_equal(got[~own], want[~own])          # what the product does not own is carried over bit for bit
    full = np.zeros((m + 1, n + 5))
    full[:m, 3:3 + n] = R.gamma(k + 1) * (_torch_product(transa, transb, np.abs(abuf[:ar, 2:2 + ac]),
                                                         np.abs(bbuf[1:1 + br, 1:1 + bc]),
                                                         None if bv is None else np.abs(bv[:n]), False))
    assert np.allclose(bd, full.reshape(-1)[c_off:], rtol=1e-14, atol=0)


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("n_out", [1, 33])
def test_restatement_on_the_interleaved_heads_of_the_attention_input_layer(H, n_out):
    """the three strided-batched forms of cslicer/aggr.py (projection, weight gradient, operand gradient): a head is a
    column block of every row, so the batch stride is SMALLER than the leading dimension"""
    rng = np.random.default_rng(H + n_out)
    D, F = 8, 12
    Cw = H * D
    agg = rng.standard_normal((n_out, H * F)).astype(np.float32)
    weight = rng.standard_normal((Cw, F)).astype(np.float32)
    gg = rng.standard_normal((n_out, Cw)).astype(np.float32)
    a64, w64, g64 = (torch.from_numpy(x).double() for x in (agg, weight, gg))
    a3, w3, g3 = a64.view(n_out, H, F), w64.view(H, D, F), g64.view(n_out, H, D)
    out = R.gemm(0, 1, n_out, D, F, agg, H * F, F, weight, F, D * F, np.full(n_out * Cw, 7.5), Cw, D, H)
    assert np.allclose(out.reshape(n_out, H, D), torch.einsum("rhf,hdf->rhd", a3, w3).numpy(), rtol=1e-13, atol=1e-13)
    gw = R.gemm(1, 0, D, F, n_out, gg, Cw, D, agg, H * F, F, np.full(Cw * F, 7.5), F, D * F, H)
    assert np.allclose(gw.reshape(H, D, F), torch.einsum("rhd,rhf->hdf", g3, a3).numpy(), rtol=1e-13, atol=1e-13)
    dagg = R.gemm(0, 0, n_out, F, D, gg, Cw, D, weight, F, D * F, np.full(n_out * H * F, 7.5), H * F, F, H)
    assert np.allclose(dagg.reshape(n_out, H, F), torch.einsum("rhd,hdf->rhf", g3, w3).numpy(), rtol=1e-13, atol=1e-13)


def test_restatement_on_row_slabs_and_a_gap_between_the_results():
    """the slabbed weight gradient (batch = slabs of rows) and a batched C whose matrices lie further apart than m * ldc:
    the gap keeps what it held"""
    rng = np.random.default_rng(3)
    ns, rs, out_f, in_f = 3, 5, 4, 8
    gy, x = rng.standard_normal((ns * rs, out_f)).astype(np.float32), rng.standard_normal((ns * rs, in_f)).astype(np.float32)
    wn = out_f * in_f
    slabs = R.gemm(1, 0, out_f, in_f, rs, gy, out_f, rs * out_f, x, in_f, rs * in_f, np.full((ns + 1) * wn, 7.5), in_f, wn, ns)
    assert bool((slabs[ns * wn:] == 7.5).all())
    total = R.sum_slabs(slabs, wn, ns)
    want = (torch.from_numpy(gy).double().t() @ torch.from_numpy(x).double()).numpy().reshape(-1)
    assert np.allclose(total, want, rtol=1e-13, atol=1e-13)
    assert bool((R.sum_slabs_bound(slabs, wn, 1) == 0).all()) and bool((R.sum_slabs_bound(slabs, wn, ns) > 0).all())
    m, n, k, ldc, sc = 3, 2, 4, 5, 3 * 5 + 7
    a, b = rng.standard_normal((2, m, k)).astype(np.float32), rng.standard_normal((2, k, n)).astype(np.float32)
    c = R.gemm(0, 0, m, n, k, a, k, m * k, b, n, k * n, np.full(2 * sc, 7.5), ldc, sc, 2).reshape(2, sc)
    for i in range(2):
        blk = c[i, :m * ldc].reshape(m, ldc)
        assert np.allclose(blk[:, :n], (torch.from_numpy(a[i]).double() @ torch.from_numpy(b[i]).double()).numpy(), rtol=1e-13,
                           atol=1e-13)
        assert bool((blk[:, n:] == 7.5).all()) and bool((c[i, m * ldc:] == 7.5).all())
    z = R.gemm(0, 0, m, n, 0, None, 0, 0, None, 0, 0, np.full(2 * sc, 7.5), ldc, sc, 2)     # an empty reduction: zeros
    own = R.owned(m, n, ldc, sc, 2, 2 * sc)
    assert bool((z[own] == 0).all()) and bool((z[~own] == 7.5).all()) and int(own.sum()) == 2 * m * n
    with pytest.raises(ValueError):                    # a matrix that does not lie inside its buffer is an error, not a wrap
        R.gemm(0, 0, m, n, k, a[0], k, 0, b[0], n, 0, np.zeros(m * ldc - (ldc - n) - 1), ldc, 0, 1)


def test_gamma_is_the_textbook_constant():
    assert R.U == 2.0 ** -24 and R.gamma(0) == 0.0
    assert R.gamma(1) == R.U / (1 - R.U) and abs(R.gamma(201) / (201 * R.U) - 1) < 2e-5


# ---- the size buckets --------------------------------------------------------------------------------------------------

def test_bucket_rule():
    assert [R.bucket(0, m, 200) for m in (1, 1023, 1024, 4095, 4096, 20001)] == [1, 1, 2, 2, 0, 0]
    assert [R.bucket(1, 256, k) for k in (1, 1023, 1024, 4096, 10007)] == [1, 1, 0, 0, 0]
    assert R.bucket(0, 1023, 5000) == 1 and R.bucket(1, 5000, 1023) == 1          # only the long dimension counts


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from cslicer import _abi
    return _abi.load()


def test_the_gemm_prototypes_are_bound_from_the_header(lib):
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert list(lib.csl_gemm_f32.argtypes) == [i32, i32, i64, i64, i64, vp, i64, i64, vp, i64, i64, vp, i64, i64, i32, vp, i32, vp]
    assert list(lib.csl_sum_slabs_f32.argtypes) == [vp, i64, i32, vp, vp]
    assert list(lib.csl_gemm_save_plans.argtypes) == [C.c_char_p] and list(lib.csl_gemm_load_plans.argtypes) == [C.c_char_p]
    assert lib.csl_gemm_last_error.restype is C.c_char_p


def test_gemm_refuses_before_any_hip_call(lib):
    """no GPU here: every one of these returns CSL_E_INVALID from the host-side checks; the addresses are host addresses
    that are never dereferenced"""
    buf = np.zeros(64, dtype=np.float32)
    x, nul = C.c_void_p(buf.ctypes.data), C.c_void_p(0)
    ok = dict(ta=0, tb=0, m=4, n=5, k=6, A=x, lda=6, sa=0, B=x, ldb=5, sb=0, C=x, ldc=5, sc=0, batch=1, bias=nul, relu=0,
              stream=nul)

    def call(**kw):
        return lib.csl_gemm_f32(*dict(ok, **kw).values())
    for bad in (dict(m=-1), dict(n=-1), dict(k=-1), dict(batch=0), dict(batch=-3), dict(C=nul), dict(A=nul), dict(B=nul),
                dict(k=0, bias=x), dict(k=0, relu=1), dict(k=0, bias=x, relu=1), dict(k=0, C=nul)):
        assert call(**bad) == E_INVALID, bad
    # a leading dimension one below its minimum: lda >= k (m when transa), ldb >= n (k when transb), ldc >= n
    for ta in (0, 1):
        for tb in (0, 1):
            lda, ldb = (4 if ta else 6), (6 if tb else 5)
            for bad in (dict(lda=lda - 1, ldb=ldb), dict(lda=lda, ldb=ldb - 1), dict(lda=lda, ldb=ldb, ldc=4)):
                assert call(ta=ta, tb=tb, **bad) == E_INVALID, (ta, tb, bad)
    # nothing to compute: 0, whatever else is passed
    assert call(m=0) == 0 and call(n=0) == 0 and call(m=0, n=0, A=nul, B=nul, C=nul) == 0
    assert call(m=0, k=0, bias=x) == 0 and call(n=0, lda=1, ldb=1, ldc=0) == 0
    assert call(m=-1, n=0) == E_INVALID and call(m=0, batch=0) == E_INVALID       # (the signs are looked at first)


def test_sum_slabs_refuses_before_any_hip_call(lib):
    buf = np.zeros(64 + 8, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16              # a 16-byte aligned host address: never dereferenced
    x, nul = C.c_void_p(base), C.c_void_p(0)
    ok = dict(slabs=x, n=8, n_slabs=2, out=C.c_void_p(base + 64), stream=nul)

    def call(**kw):
        return lib.csl_sum_slabs_f32(*dict(ok, **kw).values())
    for bad in (dict(n=-4), dict(n_slabs=0), dict(n_slabs=-1), dict(n=6), dict(n=7), dict(n=9), dict(slabs=nul), dict(out=nul),
                dict(slabs=C.c_void_p(base + 4)), dict(slabs=C.c_void_p(base + 8)), dict(out=C.c_void_p(base + 64 + 12))):
        assert call(**bad) == E_INVALID, bad
    assert call(n=0) == 0 and call(n=0, slabs=nul, out=nul) == 0   # nothing to sum
    assert call(n=0, n_slabs=0) == E_INVALID
