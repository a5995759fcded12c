"""CPU-side checks of the 16-bit feature table: the L0 round trip of a float16 / bfloat16 features.bin, the C ABI of
include/cslicer_feat16.h (symbols, argument checks that return before any HIP call) and the trainer's argument
handling that needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cslicer import _abi, aggr, l0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _features(n, f, seed=0):
    """float32 rows whose 16-bit roundings hit ties, both signs of zero, subnormals and the top of the float16 range"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, f)) * 10.0 ** rng.integers(-8, 4, size=(n, f))).astype(np.float32)
    x[0, :6] = [-0.0, 65504.0, 6e-8, -6.1e-5, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -11]   # (the last two: bfloat16 / float16 ties)
    return x


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_l0_round_trip(tmp_path, dtype):
    indptr, indices = l0.synth_graph(300, 5.0, seed=1)
    n, f = 300, 12
    x = _features(n, f)
    d = str(tmp_path / dtype)
    meta = l0.write_l0(d, indptr, indices, features=x, labels=np.arange(n) % 3, num_classes=3, feature_dtype=dtype)
    assert meta["feature_dtype"] == dtype
    assert "feature_dtype=%s\n" % dtype in open(os.path.join(d, "meta.txt")).read()
    a, b, m = l0.read_l0(d, mmap=False)
    np.testing.assert_array_equal(a, indptr)
    assert m["feature_dtype"] == dtype and l0.read_meta(d)["feature_dtype"] == dtype
    assert m["feature_dim"] == f and m["num_classes"] == 3
    size = os.path.getsize(os.path.join(d, "features.bin"))
    assert size == n * f * (4 if dtype == "float32" else 2)
    want = torch.as_tensor(x).to(TORCH_DTYPES[dtype])
    rows, stored = l0.read_features(d, m, mmap=False)
    assert stored == dtype and rows.shape == (n, f)
    if dtype == "bfloat16":
        got = torch.from_numpy(rows.view(np.int16).copy()).view(torch.bfloat16)
    else:
        got = torch.from_numpy(rows.copy())
    assert got.dtype == want.dtype
    # bit-identical, zero signs included
    bits = torch.int32 if dtype == "float32" else torch.int16
    assert torch.equal(got.view(bits), want.view(bits))
    # the checksum rule, unchanged: the sum of the stored values
    assert m["csum_features"] == int(want.to(torch.float64).sum().item())
    # the memory map the command line uses has the stored element type
    mm, _ = l0.read_features(d)
    assert mm.dtype.itemsize == (4 if dtype == "float32" else 2) and mm.shape == (n, f)


def test_l0_without_the_key_is_float32(tmp_path):
    indptr, indices = l0.synth_graph(50, 4.0, seed=2)
    x = _features(50, 8)
    d = str(tmp_path / "plain")
    l0.write_l0(d, indptr, indices, features=x)           # exactly the call the parent commit accepted
    assert "feature_dtype" not in open(os.path.join(d, "meta.txt")).read()
    assert l0.read_meta(d)["feature_dtype"] == "float32" and l0.read_l0(d)[2]["feature_dtype"] == "float32"
    rows, stored = l0.read_features(d, mmap=False)
    assert stored == "float32" and rows.dtype == np.float32
    np.testing.assert_array_equal(rows.view(np.uint32), x.view(np.uint32))
    with pytest.raises(ValueError):
        l0.write_l0(str(tmp_path / "bad"), indptr, indices, features=x, feature_dtype="int8")


def test_bfloat16_words_round_to_nearest_even():
    x = _features(2000, 16, seed=3)
    want = torch.as_tensor(x).to(torch.bfloat16)
    got = l0.to_bfloat16_words(x)
    assert np.array_equal(got, want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(l0.bfloat16_words_to_float32(got).view(np.uint32), want.float().numpy().view(np.uint32))


def header_functions():
    src = open(os.path.join(ROOT, "include", "cslicer_feat16.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src)))


def test_feat16_symbols_exported():
    L = _abi.load()
    names = header_functions()
    assert len(names) == 6
    assert names == sorted(aggr.FEAT16_SYMBOLS)
    for n in names:
        assert hasattr(L, n), "libcslicer_hip.so does not export %s" % n
    # the other headers' lists are what they were: none of the new names leaked into them
    assert not set(names) & (set(aggr.SYMBOLS) | set(_abi.SYMBOLS))


def test_feat16_host_side_argument_checks():
    """Every 16-bit entry point refuses, before any HIP call (there is no GPU here): an unknown kind, a null table, a row
    stride that is not a multiple of 4 elements, a base that is not 8-byte aligned, and what its fp32 twin refuses."""
    L = aggr._lib()
    null, st = C.c_void_p(0), C.c_void_p(0)
    tab, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)      # never dereferenced: every call below is refused
    F16, BF16 = 1, 2
    assert aggr.FEAT_KINDS == {torch.float16: F16, torch.bfloat16: BF16}

    def mfma(x, kind, ldx, H=100, out=256, n=10, W=tab):
        return L.csl_sage_fwd_mfma_x16(null, null, null, null, x, kind, ldx, W, 200, null, n, n, H, out, 0, 1, null, 0,
                                       tab, 256, tab, st)

    def cat(x, kind, ldx, H=100, n=10):
        return L.csl_sage_cat_x16(null, null, null, null, null, null, x, kind, ldx, null, 0, n, n, tab, 2 * H, H, 0, st)

    def spmm(x, kind, ldx, H=100, n=10):
        return L.csl_spmm_sum_map_x16(null, null, null, n, x, kind, ldx, null, tab, H, H, 0, st)

    def gather(x, kind, ldx, H=100, n=10):
        return L.csl_gather_rows_x16(x, kind, ldx, null, n, tab, H, H, st)

    dims = (C.c_int32 * 4)(100, 256, 256, 47)

    def step(x, kind, ldx):
        return L.csl_sage_fwd_bwd_x16(3, dims, null, null, null, x, kind, ldx, null, null, null, 1.0, 0, 1, null, null,
                                      null, 0, st)

    def rank_step(x, kind, ldx):
        return L.csl_sage_rank_fwd_bwd_x16(3, dims, null, null, null, x, kind, ldx, null, null, null, null, 1.0, 0, 1,
                                           aggr.EXCHANGE_FN(0), aggr.EXCHANGE_WAIT_FN(0), null, null, null, null, 0, st)

    for fn in (mfma, cat, spmm, gather, step, rank_step):
        for kind in (F16, BF16):
            assert fn(null, kind, 100) == -1, fn.__name__      # a null table
            assert fn(tab, kind, 102) == -1, fn.__name__       # a row stride that is not a multiple of 4 elements
            assert fn(odd, kind, 100) == -1, fn.__name__       # a base that is not 8-byte aligned
        for kind in (0, 3, -1):
            assert fn(tab, kind, 100) == -1, fn.__name__       # an unknown kind (0 is float32: the fp32 entry points)
    # the shape limits of the fp32 twins, with a table that passes: null index lists, widths, rows narrower than H
    for kind in (F16, BF16):
        assert mfma(tab, kind, 100) == -1                      # (null row pointers)
        assert mfma(tab, kind, 100, H=102) == -1 and mfma(tab, kind, 100, out=257) == -1 and mfma(tab, kind, 96) == -1
        assert mfma(tab, kind, 300, H=300) == -1               # more LDS than a workgroup has
        assert mfma(tab, kind, 100, W=null) == -1
        assert cat(tab, kind, 100) == -1 and cat(tab, kind, 100, H=6) == -1 and cat(tab, kind, 96) == -1
        assert spmm(tab, kind, 100) == -1 and spmm(tab, kind, 100, n=-1) == -1 and spmm(tab, kind, 96) == -1
        assert gather(tab, kind, 100) == -1 and gather(tab, kind, 100, n=-1) == -1 and gather(tab, kind, 96) == -1
        assert step(tab, kind, 100) == -1 and rank_step(tab, kind, 100) == -1     # (null slices)
        # nothing to do is not an error, as for the twins
        assert mfma(tab, kind, 100, n=0) == 0 and cat(tab, kind, 100, n=0) == 0
        assert spmm(tab, kind, 100, n=0) == 0 and gather(tab, kind, 100, n=0) == 0

    # ---- parity: each _f32 entry point and its _x16 twin (both kinds) get the same arguments and give the same stated
    # code.  Every case is refused or has nothing to do, so no HIP call is reached.  Defaults: the aligned dummy table,
    # H = 100, out = 256, n = n_pad = 10, the natural leading dimensions, null index lists.
    def mfma2(kind, indptr=null, self_ids=null, x=tab, ldx=None, W=tab, ldw=None, n=10, n_pad=10, H=100, out=256,
              cat=null, ldc=None, y=tab, ldy=None, wpack=tab):
        ldx, ldw = H if ldx is None else ldx, 2 * H if ldw is None else ldw
        ldc, ldy = 2 * H if ldc is None else ldc, out if ldy is None else ldy
        table = (x, ldx) if kind is None else (x, kind, ldx)
        fn = L.csl_sage_fwd_mfma_f32 if kind is None else L.csl_sage_fwd_mfma_x16
        return fn(indptr, indptr, self_ids, null, *table, W, ldw, null, n, n_pad, H, out, 0, 1, cat, ldc, y, ldy, wpack, st)

    def cat2(kind, indptr=null, self_ids=null, owned=null, deg=null, x=tab, ldx=None, agg=null, lda=None, n=10, n_pad=10,
             cat=tab, ldc=None, H=100):
        ldx, lda, ldc = H if ldx is None else ldx, H if lda is None else lda, 2 * H if ldc is None else ldc
        table = (x, ldx) if kind is None else (x, kind, ldx)
        fn = L.csl_sage_cat_f32 if kind is None else L.csl_sage_cat_x16
        return fn(indptr, indptr, self_ids, owned, deg, null, *table, agg, lda, n, n_pad, cat, ldc, H, 0, st)

    def spmm2(kind, indptr=null, rows=null, n=10, x=tab, ldx=None, out=tab, ldo=None, H=100, compact=0):
        ldx, ldo = H if ldx is None else ldx, H if ldo is None else ldo
        table = (x, ldx) if kind is None else (x, kind, ldx)
        fn = L.csl_spmm_sum_map_f32 if kind is None else L.csl_spmm_sum_map_x16
        return fn(indptr, indptr, rows, n, *table, null, out, ldo, H, compact, st)

    def gather2(kind, x=tab, lds=None, idx=null, n=10, dst=tab, ldd=None, H=100):
        lds, ldd = H if lds is None else lds, H if ldd is None else ldd
        table = (x, lds) if kind is None else (x, kind, lds)
        fn = L.csl_gather_rows_f32 if kind is None else L.csl_gather_rows_x16
        return fn(*table, idx, n, dst, ldd, H, st)

    merged = dict(self_ids=tab, owned=tab, deg=tab, agg=tab)      # sage_cat's merged-sums form: no indptr
    without = lambda d, *keys: {k: v for k, v in d.items() if k not in keys}
    matrix = {
        mfma2: ([dict(n=0, n_pad=0)],
                [dict(), dict(indptr=tab), dict(self_ids=tab), dict(H=102), dict(out=257), dict(out=0), dict(ldx=96),
                 dict(H=300), dict(W=null), dict(W=odd), dict(ldw=196), dict(ldw=202), dict(n_pad=8), dict(n=-1),
                 dict(y=null), dict(ldy=252), dict(wpack=null), dict(wpack=odd), dict(cat=tab, ldc=196), dict(cat=odd),
                 dict(indptr=tab, self_ids=tab, cat=tab, ldc=202)]),
        cat2: ([dict(n=0, n_pad=0)],
               [dict(), dict(H=6), dict(H=2), dict(ldx=96), dict(n_pad=8), dict(n=-1), dict(cat=null), dict(cat=odd),
                dict(ldc=196), dict(ldc=202), without(merged, "owned"), without(merged, "deg"), without(merged, "agg"),
                without(merged, "owned", "deg", "agg"), dict(merged, lda=96), dict(merged, lda=102), dict(merged, agg=odd),
                dict(indptr=tab)]),
        spmm2: ([dict(n=0)],
                [dict(), dict(n=-1), dict(ldx=96), dict(out=null), dict(ldo=96), dict(indptr=tab, compact=1), dict(H=0)]),
        gather2: ([dict(n=0)], [dict(), dict(n=-1), dict(lds=96), dict(dst=null), dict(ldd=96), dict(H=0)]),
    }
    assert [len(ok) + len(bad) for ok, bad in matrix.values()] == [22, 19, 8, 7]
    for fn, (ok, bad) in matrix.items():
        for want, cases in ((0, ok), (-1, bad)):
            for kw in cases:
                got = [fn(kind, **kw) for kind in (None, F16, BF16)]
                assert got == [want] * 3, (fn.__name__, kw, got)
    # the one difference that is meant: with nothing to do, a 16-bit table is still checked (here rows narrower than H), a
    # float32 table is not looked at
    for fn, kw in ((mfma2, dict(n=0, n_pad=0, ldx=96)), (cat2, dict(n=0, n_pad=0, ldx=96)), (spmm2, dict(n=0, ldx=96)),
                   (gather2, dict(n=0, lds=96))):
        assert [fn(kind, **kw) for kind in (None, F16, BF16)] == [0, -1, -1], fn.__name__


def test_trainer_refuses_an_unknown_feature_dtype():
    """raised before anything touches a device"""
    from cslicer import train
    indptr, indices = l0.synth_graph(40, 3.0, seed=0)
    x = np.zeros((40, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="feature_dtype"):
        train.Trainer(indptr, indices, x, np.zeros(40, dtype=np.int64), 3, feature_dtype="int8")
    assert sorted(aggr.FEATURE_DTYPES) == ["bfloat16", "float16", "float32"]
    assert train._parser().parse_args(["--feature-dtype", "bfloat16"]).feature_dtype == "bfloat16"
    assert train._parser().parse_args([]).feature_dtype is None
