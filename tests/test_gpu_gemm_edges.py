"""The library-GEMM host layer (csl_gemm_f32, its plan cache, shape classes and recorded plans) and csl_sum_slabs_f32
(csrc/gemm_lt.hip) through the C ABI, on device tensors as they are, against the float64 restatement in tests/gemm_ref.py.

What this file can get wrong is host logic, so that is what is varied:
  * the row-major-to-column-major swap, the four transposes, the four epilogues, the bias along OUR columns;
  * leading dimensions and batch strides: every operand a block of a wider buffer, heads interleaved in a row (batch
    stride < leading dimension), results further apart than m * ldc;
  * the shape CLASS: a shape is timed once, every other row count of its size bucket takes that algorithm untimed --
    both sides of every bucket edge, 1, odd sizes;
  * a cached plan called again with other bias / A / B / C pointers;  k == 0;  another stream;
  * recorded plans: saved, loaded into a fresh process, used; the shipped file's classes at both ends of their buckets.

Two kinds of data.  Small integers (A, B in [-3, 3], bias in [-4, 4]): every partial sum is an integer below 2^24, so the
fp32 result is exact in any order and the whole C buffer -- padding, gaps and guard rows included, prefilled with a
sentinel -- is compared with torch.equal.  Standard normals: every element within gemm_ref.bound(), the derived worst case
of an fp32 dot product (threshold 1, not a measured tolerance); elements the GEMM does not own have bound 0.

Worst observed error / bound per test (MI355X, hipBLASLt version 100000; a finding, not a threshold -- the threshold is 1):
    test_every_row_count_of_a_class                         0.037   (NT 256x200 0.032, NT 47x512 0.011, NN 0.037 / 0.011)
    test_every_reduction_length_of_a_weight_gradient_class  0.50    (k = 1: one product, bound 2 u, rounding u)
    test_slabbed_weight_gradient_and_its_sum                0.23    (8 slabs 0.23, 32 slabs 0.043)
    test_interleaved_heads                                  0.47    (n_out = 1; 0.24 at 33, 0.34 at 1025)
    test_batched_results_with_a_gap_between_them            0.37
    test_sum_slabs                                          1.00    (0.9998 at two slabs: one add, bound u; 0.052 at 33)
    test_without_tuning_the_first_supported_candidate_is_taken  0.047
No size of any class was refused by the library or came out wrong: every later size of every bucket took the class's
algorithm untimed, and the recorded-plan child timed none of the shipped file's 23 classes at either end of its bucket
(the shipped header's version is the library's).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -123.25                    # what every C buffer holds before a call: not an integer, not a result
E_STATE = -4                      # CSL_E_STATE (cslicer_hip.h)
EPILOGUES = [(False, False), (True, False), (False, True), (True, True)]          # (bias, relu)
LOG = "[csl_gemm]"                # a timing line of CSLICER_GEMM_LOG=1: one per plan whose algorithm was chosen afresh


@pytest.fixture(scope="module")
def lib():
    from cslicer import aggr
    return aggr._lib()


@pytest.fixture
def ratio(request):
    """records the worst error / bound of the test's normal-data comparisons and prints it"""
    worst = [0.0]
    yield worst
    print("\n[ratio] %s worst error / bound = %.4f" % (request.node.name, worst[0]))


def _stream():
    from cslicer import aggr
    return aggr._stream()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def _data(rng, size, exact, lim=3):
    if exact:
        return rng.integers(-lim, lim + 1, size=size).astype(np.float32)
    return rng.standard_normal(size).astype(np.float32)


def _err(lib):
    return lib.csl_gemm_last_error().decode()


def _compare(got, ref, bnd, exact, what, ratio=None):
    """the whole flat buffer: exact -> torch.equal; else |got - ref| <= bnd element by element (bnd = 0: same value)"""
    got = torch.from_numpy(np.asarray(got, dtype=np.float64))
    ref = torch.from_numpy(np.asarray(ref, dtype=np.float64))
    if exact:
        if not torch.equal(got, ref):
            bad = torch.nonzero(got != ref).reshape(-1)
            raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r"
                                 % (what, bad.numel(), ref.numel(), int(bad[0]), float(got[bad[0]]), float(ref[bad[0]])))
        return
    bnd = torch.from_numpy(np.asarray(bnd, dtype=np.float64))
    err = (got - ref).abs()
    over = torch.nonzero(~(err <= bnd)).reshape(-1)            # (a NaN is over)
    own = bnd > 0
    r = float((err[own] / bnd[own]).max()) if bool(own.any()) else 0.0
    if ratio is not None:
        ratio[0] = max(ratio[0], r)
    assert over.numel() == 0, ("%s: %d elements over the bound (worst error / bound %.3g), first at %d: got %r, want %r, "
                               "bound %.3g" % (what, over.numel(), r, int(over[0]), float(got[over[0]]),
                                               float(ref[over[0]]), float(bnd[over[0]])))


def _check(lib, ta, tb, m, n, k, A, a_off, lda, sa, B, b_off, ldb, sb, c_size, c_off, ldc, sc, batch, bias, relu, exact, what,
           ratio=None, calls=1, dev=None):
    """csl_gemm_f32 on flat host arrays A, B (the operands start a_off / b_off elements in), bias; C a fresh buffer of c_size
    sentinels, written from c_off.  `calls` calls (the first makes the plan, the others take it from the cache), each into a
    fresh C, each compared over the WHOLE buffer.  Returns the last C (device)."""
    Ad, Bd, bd = dev if dev is not None else (_dev(A), _dev(B), _dev(bias))
    c0 = np.full(c_size, SENT, dtype=np.float32)
    args = (ta, tb, m, n, k, None if A is None else A[a_off:], lda, sa, None if B is None else B[b_off:], ldb, sb, c0[c_off:],
            ldc, sc, batch, bias, relu)
    ref = np.concatenate([c0[:c_off].astype(np.float64), R.gemm(*args)])
    bnd = None if exact else np.concatenate([np.zeros(c_off), R.bound(*args)])
    Cd = None
    for call in range(calls):
        Cd = torch.full((c_size,), SENT, dtype=torch.float32, device="cuda")
        rc = lib.csl_gemm_f32(ta, tb, m, n, k, _ptr(Ad, a_off), lda, sa, _ptr(Bd, b_off), ldb, sb, _ptr(Cd, c_off), ldc, sc, batch,
                              _ptr(bd), int(relu), _stream())
        assert rc == 0, "%s (call %d): %d %s" % (what, call, rc, _err(lib))
        _compare(Cd.cpu().numpy(), ref, bnd, exact, "%s (call %d)" % (what, call), ratio)
    return Cd


def _timing_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith(LOG)]


# ---- 1. operand layout: transposes x epilogues x shapes, tight and as blocks of wider buffers, exact -------------------------

@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_operand_layout_exact(lib, ta, tb):
    """m != n and the bias is asymmetric (bias[j] = j-dependent integers), so a bias applied along the rows, a swapped
    operand or a swapped transpose flag cannot come out right.  The wide form puts A, B, C and the bias inside larger
    buffers (two leading columns, a leading row of B, spare rows and columns behind): everything around the m x n block
    of C keeps the sentinel.  Two calls each: the one that makes the plan and the cached one."""
    rng = np.random.default_rng(100 + 2 * ta + tb)
    for (m, n, k) in [(1, 1, 1), (33, 7, 5), (257, 47, 100), (65, 200, 36)]:
        ar, ac = (k, m) if ta else (m, k)
        br, bc = (n, k) if tb else (k, n)
        for wide in (False, True):
            if wide:
                lda, a_off, a_rows = ac + 3, 2, ar + 1
                ldb, b_rows = bc + 8, br + 7
                b_off = ldb + 2
                ldc, c_off, c_rows = n + 5, 2, m + 1
                nb = n + 8
            else:
                lda, a_off, a_rows, ldb, b_off, b_rows, ldc, c_off, c_rows, nb = ac, 0, ar, bc, 0, br, n, 0, m, n
            A, B = _data(rng, a_rows * lda, True), _data(rng, b_rows * ldb, True)
            bias_v = (rng.integers(-4, 5, size=nb) + (np.arange(nb) % 3 == 0)).clip(-4, 4).astype(np.float32)
            for has_bias, relu in EPILOGUES:
                _check(lib, ta, tb, m, n, k, A, a_off, lda, 0, B, b_off, ldb, 0, c_rows * ldc, c_off, ldc, 0, 1,
                       bias_v if has_bias else None, relu, True,
                       "%s%s %dx%dx%d wide=%d bias=%d relu=%d" % ("NT"[ta], "NT"[tb], m, n, k, wide, has_bias, relu), calls=2)


# ---- 2. every row count of a class ---------------------------------------------------------------------------------------------

M_BUCKETS = [[1000, 1, 7, 33, 255, 1023], [2048, 1024, 1025, 3001, 4095], [8192, 4096, 4097, 20001]]
K_BUCKETS = [[1000, 1, 3, 1023], [2048, 1024, 1025, 10007]]


def _class_sweep(lib, capfd, monkeypatch, ratio, ta, tb, buckets, shape_of, has_bias, relu, seed):
    """buckets: lists of the long dimension's sizes, the first of each on a class nobody has used (it must log ONE timing
    line), the others on the class it made (at least one of them must log none: the reuse branch of make_plan_impl).  At
    every size: integers, exact (this call makes the plan), then normals within the bound (the cached plan)."""
    monkeypatch.setenv("CSLICER_GEMM_LOG", "1")
    monkeypatch.delenv("CSLICER_GEMM_TUNE", raising=False)
    rng = np.random.default_rng(seed)
    retimed = []
    for sizes in buckets:
        codes = set()
        reused = 0
        for i, size in enumerate(sizes):
            m, n, k, lda, ldb, ldc = shape_of(size)
            codes.add(R.bucket(ta, m, k))
            ar = k if ta else m
            br = n if tb else k
            what = "%s%s m=%d n=%d k=%d" % ("NT"[ta], "NT"[tb], m, n, k)
            bias_i = _data(rng, n, True, 4) if has_bias else None
            capfd.readouterr()
            _check(lib, ta, tb, m, n, k, _data(rng, ar * lda, True), 0, lda, 0, _data(rng, br * ldb, True), 0, ldb, 0,
                   (m + 1) * ldc, 0, ldc, 0, 1, bias_i, relu, True, what + " integers")
            lines = _timing_lines(capfd)
            if i == 0:
                assert len(lines) == 1, "%s: the first size of a fresh class logs one timing line, got %r" % (what, lines)
            else:
                assert len(lines) <= 1, (what, lines)
                reused += not lines
                retimed += [what] * len(lines)
            _check(lib, ta, tb, m, n, k, _data(rng, ar * lda, False), 0, lda, 0, _data(rng, br * ldb, False), 0, ldb, 0,
                   (m + 1) * ldc, 0, ldc, 0, 1, _data(rng, n, False) if has_bias else None, relu, False, what + " normals", ratio)
            assert not _timing_lines(capfd), what + ": a cached plan was timed again"
        assert len(codes) == 1, "the sizes %r are meant to be one bucket" % (sizes,)
        assert reused >= 1, ("no size of %r after the first took the class's algorithm untimed: the reuse path was not "
                             "reached (the library refused the algorithm at every other size)" % (sizes,))
    print("\n[reuse] sizes the library refused the class's algorithm for (timed afresh): %r" % (retimed,))


@pytest.mark.parametrize("n,k", [(256, 200), (47, 512)])
@pytest.mark.parametrize("form", ["NT_bias_relu", "NN_plain"])
def test_every_row_count_of_a_class(lib, capfd, monkeypatch, ratio, form, n, k):
    """the forward (NT, bias + ReLU) and the input gradient (NN) at the real widths; the classes are fresh because no other
    caller pads these leading dimensions by 4 (a class keeps lda, ldb, ldc)"""
    tb = 1 if form.startswith("NT") else 0
    epi = tb == 1

    def shape_of(m):
        return m, n, k, k + 4, (k + 4 if tb else n + 4), n + 4
    _class_sweep(lib, capfd, monkeypatch, ratio, 0, tb, M_BUCKETS, shape_of, epi, epi, 7 * n + tb)


def test_every_reduction_length_of_a_weight_gradient_class(lib, capfd, monkeypatch, ratio):
    """TN: the long dimension is k, two buckets"""
    def shape_of(k):
        return 40, 72, k, 44, 76, 76
    _class_sweep(lib, capfd, monkeypatch, ratio, 1, 0, K_BUCKETS, shape_of, False, False, 11)


# ---- 3. a cached plan follows its arguments --------------------------------------------------------------------------------------

def test_cached_plan_follows_its_arguments(lib):
    """one key, three calls, each with its own bias, A, B and C tensors (all kept alive, so a stale pointer reads valid
    memory and shows as a wrong value); then the same shape under the four epilogues in turn, twice: a plan made for
    one epilogue must not serve another"""
    rng = np.random.default_rng(3)
    m, n, k = 65, 40, 72
    keep = []
    for call in range(3):
        A, B, bias = _data(rng, m * k, True), _data(rng, n * k, True), _data(rng, n, True, 4)
        dev = (_dev(A), _dev(B), _dev(bias))
        keep.append((dev, _check(lib, 0, 1, m, n, k, A, 0, k, 0, B, 0, k, 0, m * n + 8, 0, n, 0, 1, bias, True, True,
                                 "call %d of one key" % call, dev=dev)))
    for rnd in range(2):
        for has_bias, relu in EPILOGUES:
            A, B, bias = _data(rng, m * k, True), _data(rng, n * k, True), _data(rng, n, True, 4)
            dev = (_dev(A), _dev(B), _dev(bias) if has_bias else None)
            keep.append((dev, _check(lib, 0, 1, m, n, k, A, 0, k, 0, B, 0, k, 0, m * n + 8, 0, n, 0, 1, bias if has_bias else None,
                                     relu, True, "round %d bias=%d relu=%d" % (rnd, has_bias, relu), dev=dev)))


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rs", [1023, 1024, 1025])
@pytest.mark.parametrize("n_slabs", [8, 32])
def test_slabbed_weight_gradient_and_its_sum(lib, ratio, n_slabs, rs):
    """gW = gy^T cat as the native step issues it (csrc/sage_step.hip, weight_grad): n_slabs row slabs as one batched TN
    GEMM, then csl_sum_slabs_f32 into the row behind the slabs (cslicer.aggr.weight_grad_slabs).  Held to the float64
    product of the WHOLE matrices."""
    out_f, in2 = 40, 72
    wn, rows = out_f * in2, n_slabs * rs
    for exact in (True, False):
        rng = np.random.default_rng(n_slabs * rs + exact)
        gy, cat = _data(rng, rows * out_f, exact), _data(rng, rows * in2, exact)
        size = (n_slabs + 1) * wn + 4
        what = "%d slabs of %d rows, %s" % (n_slabs, rs, "integers" if exact else "normals")
        Cd = _check(lib, 1, 0, out_f, in2, rs, gy, 0, out_f, rs * out_f, cat, 0, in2, rs * in2, size, 0, in2, wn, n_slabs,
                    None, False, exact, what, ratio)
        slabs = Cd.cpu().numpy()[:n_slabs * wn].copy()
        assert lib.csl_sum_slabs_f32(_ptr(Cd), wn, n_slabs, _ptr(Cd, n_slabs * wn), _stream()) == 0
        got = Cd.cpu().numpy()
        assert np.array_equal(got[:n_slabs * wn], slabs) and bool((got[(n_slabs + 1) * wn:] == SENT).all()), what
        total = got[n_slabs * wn:(n_slabs + 1) * wn]
        whole = (gy.reshape(rows, out_f).astype(np.float64).T @ cat.reshape(rows, in2).astype(np.float64)).reshape(-1)
        _compare(total, R.sum_slabs(slabs, wn, n_slabs), R.sum_slabs_bound(slabs, wn, n_slabs), exact, what + ": the sum", ratio)
        if exact:
            _compare(total, whole, None, True, what + ": the whole product")
        else:
            args = (1, 0, out_f, in2, rs, gy, out_f, rs * out_f, cat, in2, rs * in2, np.zeros(n_slabs * wn), in2, wn, n_slabs)
            _compare(total, whole, R.slabbed_bound(R.gemm(*args), R.bound(*args), wn, n_slabs), False,
                     what + ": the whole product", ratio)


@pytest.mark.parametrize("n_out", [1, 33, 1025])
@pytest.mark.parametrize("H", [2, 4])
def test_interleaved_heads(lib, ratio, H, n_out):
    """the attention input layer's three strided-batched products (cslicer.aggr.GatInputLayer): a head is a column block
    of every row, so stride_a = F under lda = H F and stride_c = D under ldc = H D"""
    D, F = 8, 12
    Cw = H * D
    for exact in (True, False):
        rng = np.random.default_rng(100 * H + n_out + exact)
        agg, weight, gg = _data(rng, n_out * H * F, exact), _data(rng, Cw * F, exact), _data(rng, n_out * Cw, exact)
        what = "H=%d n_out=%d %s " % (H, n_out, "integers" if exact else "normals")
        _check(lib, 0, 1, n_out, D, F, agg, 0, H * F, F, weight, 0, F, D * F, n_out * Cw + 8, 0, Cw, D, H, None, False, exact,
               what + "projection", ratio, calls=2)
        _check(lib, 1, 0, D, F, n_out, gg, 0, Cw, D, agg, 0, H * F, F, Cw * F + 8, 0, F, D * F, H, None, False, exact,
               what + "weight gradient", ratio, calls=2)
        _check(lib, 0, 0, n_out, F, D, gg, 0, Cw, D, weight, 0, F, D * F, n_out * H * F + 8, 0, H * F, F, H, None, False, exact,
               what + "operand gradient", ratio, calls=2)


def test_batched_results_with_a_gap_between_them(lib, ratio):
    """stride_c > m * ldc, ldc > n, and operands further apart than their own size: the gaps keep the sentinel"""
    m, n, k, batch = 33, 7, 5, 3
    ldc, lda, ldb = n + 5, k + 1, n + 2
    sa, sb, sc = m * lda + 3, k * ldb + 1, m * ldc + 11
    for exact in (True, False):
        rng = np.random.default_rng(40 + exact)
        for has_bias, relu in ((False, False), (True, True)):
            _check(lib, 0, 0, m, n, k, _data(rng, batch * sa, exact), 0, lda, sa, _data(rng, batch * sb, exact), 0, ldb, sb,
                   batch * sc + ldc, 2, ldc, sc, batch, _data(rng, n, exact, 4) if has_bias else None, relu, exact,
                   "gap, bias=%d %s" % (has_bias, "integers" if exact else "normals"), ratio, calls=2)


# ---- 5. k == 0 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3])
def test_empty_reduction_zeroes_its_blocks_only(lib, batch):
    """what a rank with an empty share of the minibatch calls: the owned m x n blocks become zero, the columns between
    them, the gap between the batches and the rows behind keep the sentinel"""
    m, n, ldc, c_off = 33, 7, 12, 2
    sc = (m + 1) * ldc + 3
    for ta, tb in ((0, 0), (1, 0), (0, 1)):
        Cd = _check(lib, ta, tb, m, n, 0, None, 0, 1, 0, None, 0, 1, 0, batch * sc + ldc, c_off, ldc, sc, batch, None, False, True,
                    "k = 0, batch %d" % batch)
        got = Cd.cpu().numpy()
        assert int((got == 0).sum()) == batch * m * n and int((got == SENT).sum()) == got.shape[0] - batch * m * n


# ---- 6. csl_sum_slabs_f32 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_slabs", [1, 2, 3, 4, 5, 7, 8, 9, 32, 33])
def test_sum_slabs(lib, ratio, n_slabs):
    """the loop takes four slabs at a time and then the rest; a block covers 256 float4: one float4, a block less one, a
    block, a block and one, several blocks.  The float behind out[n - 1] keeps its bits."""
    for n4 in (1, 255, 256, 257, 1000):
        n = 4 * n4
        for exact in (True, False):
            rng = np.random.default_rng(1000 * n_slabs + n4 + exact)
            slabs = _data(rng, n_slabs * n, exact, 100)
            sd = _dev(slabs)
            out = torch.full((n + 4,), SENT, dtype=torch.float32, device="cuda")
            assert lib.csl_sum_slabs_f32(_ptr(sd), n, n_slabs, _ptr(out), _stream()) == 0
            want = np.concatenate([R.sum_slabs(slabs, n, n_slabs), np.full(4, SENT)])
            bnd = np.concatenate([R.sum_slabs_bound(slabs, n, n_slabs), np.zeros(4)])
            _compare(out.cpu().numpy(), want, bnd, exact, "%d slabs of %d floats" % (n_slabs, n), ratio)
            assert torch.equal(sd.cpu(), torch.from_numpy(slabs))


# ---- 7. CSLICER_GEMM_TUNE=0 -------------------------------------------------------------------------------------------------------

def test_without_tuning_the_first_supported_candidate_is_taken(lib, capfd, monkeypatch, ratio):
    """the variable is read when a plan is made: on a fresh class nothing is timed (the log line says `0 timed`), and the
    values are right at two row counts of the class"""
    monkeypatch.setenv("CSLICER_GEMM_TUNE", "0")
    monkeypatch.setenv("CSLICER_GEMM_LOG", "1")
    rng = np.random.default_rng(7)
    n, k, lda = 40, 72, 72 + 16                      # (a leading dimension no other caller of these widths uses)
    for i, m in enumerate((500, 777)):
        capfd.readouterr()
        for exact in (True, False):
            _check(lib, 0, 1, m, n, k, _data(rng, m * lda, exact), 0, lda, 0, _data(rng, n * k, exact), 0, k, 0, m * n + 8, 0, n, 0,
                   1, _data(rng, n, exact, 4), True, exact, "untuned m=%d" % m, ratio)
        lines = _timing_lines(capfd)
        assert len(lines) == (1 if i == 0 else len(lines)) and len(lines) <= 1, lines
        assert all("(0 timed)" in l for l in lines), lines


# ---- 8. one stream -----------------------------------------------------------------------------------------------------------------

def test_a_call_from_another_stream_is_refused_and_writes_nothing(lib):
    rng = np.random.default_rng(8)
    m, n, k = 33, 7, 5
    A, B = _data(rng, m * k, True), _data(rng, k * n, True)
    dev = (_dev(A), _dev(B), None)
    _check(lib, 0, 0, m, n, k, A, 0, k, 0, B, 0, n, 0, m * n, 0, n, 0, 1, None, False, True, "the bound stream", dev=dev)
    other = torch.cuda.Stream()
    Cd = torch.full((m * n,), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        assert _stream().value, "the side stream is the null stream"
        rc = lib.csl_gemm_f32(0, 0, m, n, k, _ptr(dev[0]), k, 0, _ptr(dev[1]), n, 0, _ptr(Cd), n, 0, 1, C.c_void_p(0), 0, _stream())
    assert rc == E_STATE and "stream" in _err(lib), (rc, _err(lib))
    torch.cuda.synchronize()
    assert bool((Cd == SENT).all())
    _check(lib, 0, 0, m, n, k, A, 0, k, 0, B, 0, n, 0, m * n, 0, n, 0, 1, None, False, True, "the bound stream again", dev=dev)


# ---- 9. recorded plans: save, load into a fresh process, use ------------------------------------------------------------------------

PLAN_N, PLAN_K = 24, 56           # the forward family of the round trip: NT, bias, [m, 56] x [24, 56]^T, tight
PLAN_TN = (24, 56)                # the weight-gradient family: TN, [k, 24]^T x [k, 56]
OTHER_N, OTHER_K = 28, 52         # a class the saved file does not hold


def _plan_call(lib, rng, ta, m, n, k, what, has_bias):
    ar = k if ta else m
    lda = m if ta else k
    tb = 0 if ta else 1
    _check(lib, ta, tb, m, n, k, _data(rng, ar * lda, True), 0, lda, 0, _data(rng, (k if ta else n) * (n if ta else k), True), 0,
           n if ta else k, 0, m * n + 8, 0, n, 0, 1, _data(rng, n, True, 4) if has_bias else None, False, True, what)


def _fields(path):
    lines = open(path).read().splitlines()
    return lines[0], [l.split() for l in lines[1:]]


def test_recorded_plans_round_trip(lib, capfd, monkeypatch, tmp_path):
    """Parent: two fresh families tuned on both sides of every bucket edge (a size whose bucket is new logs a timing line:
    that is the bucket rule seen from outside), saved; the file names each class once, with gemm_ref.bucket()'s code where
    the long dimension was.  Child (a fresh process: empty plan tables): loads the file, runs the same classes at other
    sizes untimed, a class the file lacks timed, the file under another version timed again; then the shipped file's
    classes at both ends of their buckets.  All on integers, exact."""
    monkeypatch.setenv("CSLICER_GEMM_LOG", "1")
    monkeypatch.delenv("CSLICER_GEMM_TUNE", raising=False)
    rng = np.random.default_rng(9)
    seen = set()
    for ta, sizes in ((0, (1023, 1024, 4095, 4096)), (1, (1023, 1024))):
        for size in sizes:
            m, n, k = (PLAN_TN[0], PLAN_TN[1], size) if ta else (size, PLAN_N, PLAN_K)
            capfd.readouterr()
            _plan_call(lib, rng, ta, m, n, k, "tuning %d" % size, not ta)
            lines = _timing_lines(capfd)
            code = (ta, R.bucket(ta, m, k))
            if code not in seen:
                assert len(lines) == 1, "size %d opens bucket %d of its family: one timing line, got %r" % (size, code[1], lines)
            seen.add(code)
    path = str(tmp_path / "plans.txt")
    assert lib.csl_gemm_save_plans(path.encode()) == 0
    header, rows = _fields(path)
    assert header.startswith("# csl_gemm_f32 plans: hipblaslt ") and int(header.split()[-1]) >= 0
    assert rows and all(len(r) == 14 for r in rows) and len(set(tuple(r[:13]) for r in rows)) == len(rows)
    fwd = sorted(int(r[2]) for r in rows if r[:2] == ["0", "1"] and r[3:9] == [str(PLAN_N), str(PLAN_K), str(PLAN_K), str(PLAN_K),
                                                                              str(PLAN_N), "1"])
    wg = sorted(int(r[4]) for r in rows if r[:4] == ["1", "0", str(PLAN_TN[0]), str(PLAN_TN[1])] and r[5:9] ==
                [str(PLAN_TN[0]), str(PLAN_TN[1]), str(PLAN_TN[1]), "1"])
    assert fwd == sorted({R.bucket(0, m, PLAN_K) for m in (1023, 1024, 4095, 4096)}) == [0, 1, 2], fwd
    assert wg == sorted({R.bucket(1, 24, k) for k in (1023, 1024)}) == [0, 1], wg
    env = dict(os.environ, CSLICER_GEMM_PLANS=path, CSLICER_GEMM_LOG="1")
    env.pop("CSLICER_GEMM_TUNE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path, str(len(rows))], env=env, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    report = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert report["loaded"] == len(rows) and report["shipped_classes"] == 23 and report["ok"]


class _Fd2:
    """what the process writes to file descriptor 2 inside the block (the library's fprintf included)"""

    def __enter__(self):
        import tempfile
        sys.stderr.flush()
        self.saved, self.f = os.dup(2), tempfile.TemporaryFile()
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.lines = [l for l in self.f.read().decode(errors="replace").splitlines() if l.startswith(LOG)]
        self.f.close()


def _child(path, n_lines):
    from cslicer import aggr
    lib = aggr._lib()
    rng = np.random.default_rng(19)
    report = {"ok": False}
    report["loaded"] = int(lib.csl_gemm_load_plans(path.encode()))
    assert report["loaded"] == n_lines, report
    # the recorded classes, at other sizes of their buckets: no timing line (forward buckets 1 and 2, weight gradient 1)
    with _Fd2() as fd:
        for m in (7, 1000, 3001):
            _plan_call(lib, rng, 0, m, PLAN_N, PLAN_K, "recorded forward m=%d" % m, True)
        _plan_call(lib, rng, 1, PLAN_TN[0], PLAN_TN[1], 333, "recorded weight gradient k=333", False)
    assert fd.lines == [], "recorded classes were timed: %r" % fd.lines
    # a class the file does not hold: one line
    with _Fd2() as fd:
        _plan_call(lib, rng, 0, 500, OTHER_N, OTHER_K, "a class the file lacks", True)
    assert len(fd.lines) == 1, fd.lines
    # the same file under another version: its entries are ignored.  The two recorded classes this process has not used
    # yet (forward bucket 0, weight gradient bucket 0) are timed, and right.
    header, rows = _fields(path)
    other = path + ".other_version"
    with open(other, "w") as f:
        f.write(" ".join(header.split()[:-1] + [str(int(header.split()[-1]) + 1)]) + "\n")
        f.write("\n".join(" ".join(r) for r in rows) + "\n")
    assert int(lib.csl_gemm_load_plans(other.encode())) == n_lines
    with _Fd2() as fd:
        _plan_call(lib, rng, 0, 5000, PLAN_N, PLAN_K, "another version, forward m=5000", True)
        _plan_call(lib, rng, 1, PLAN_TN[0], PLAN_TN[1], 2000, "another version, weight gradient k=2000", False)
    assert len(fd.lines) == 2, "a file of another library version must be ignored: %r" % fd.lines
    # the shipped file: every class at a size just inside each end of its bucket
    version = int(header.split()[-1])                     # (csl_gemm_save_plans wrote the loaded library's version)
    s_header, s_rows = _fields(aggr.GEMM_PLANS)
    report["shipped_classes"] = len(s_rows)
    report["library_version"], report["shipped_version"] = version, int(s_header.split()[-1])
    report["shipped_version_is_the_library's"] = report["shipped_version"] == version
    assert int(lib.csl_gemm_load_plans(aggr.GEMM_PLANS.encode())) == len(s_rows)
    timed = 0
    for r in s_rows:
        ta, tb, m, n, k, lda, ldb, ldc, batch, sa, sb, sc, epi, _ = (int(x) for x in r)
        code = k if ta else m
        ends = {(0, 1): (1, 1023), (0, 2): (1024, 4095), (0, 0): (4096, 5001), (1, 1): (1, 1023), (1, 0): (1024, 1537)}[(ta, code)]
        if batch > 1:
            ends = (ends[0], min(ends[1], 1025))          # (32 slabs: the rows stay near 32 k)
        for size in ends:
            if ta:
                k = size
                sa, sb = k * lda, k * ldb
            else:
                m = size
            assert R.bucket(ta, m, k) == code
            ar, br = (k if ta else m), (n if tb else k)
            has_bias, relu = epi in (4, 6), epi in (2, 6)          # HIPBLASLT_EPILOGUE_RELU = 2, _BIAS = 4, _RELU_BIAS = 6
            assert epi in (1, 2, 4, 6), epi
            with _Fd2() as fd:
                _check(lib, ta, tb, m, n, k, _data(rng, batch * ar * lda, True), 0, lda, sa if batch > 1 else 0,
                       _data(rng, batch * br * ldb, True), 0, ldb, sb if batch > 1 else 0, max(batch * sc, m * ldc) + 8, 0, ldc, sc,
                       batch, _data(rng, n, True, 4) if has_bias else None, relu, True, "shipped class %s at %d" % (" ".join(r), size))
            timed += len(fd.lines)
    report["shipped_sizes_timed"] = timed
    report["ok"] = True
    print(json.dumps(report))


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "child":
    for p in (ROOT, os.path.join(ROOT, "occ-gnn_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    _child(sys.argv[2], int(sys.argv[3]))
