"""Training on a 16-bit feature table (float16 / bfloat16 rows resident in HBM, include/cslicer_feat16.h) on the GPU box.

Both upcasts to float32 are exact, and everything after the load is the fp32 code, so NOTHING here has a tolerance:
every 16-bit kernel must give bitwise what its fp32 twin gives on the table upcast to float32, and a model trained on a
16-bit table must be bitwise the model trained on that table upcast to float32 -- losses, parameters, evaluation.
"Bitwise" is taken literally: tensors are compared as int32 words (torch.equal on the bit patterns), which also tells
-0.0 from +0.0.

Table contents: random values plus, in both formats, negative zero, the largest finite value and subnormals (no NaN, no
Inf).  In the kernel cases all of them are read.  In the trainer cases the largest finite value sits in the row of a node
that is never sampled (node 0: no edges, not among the training nodes): bfloat16's 3.39e38 survives one fp32 sum but not
the layers behind it, and a loss of Inf or NaN would compare nothing.
"""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
EC, EMAX, BM = 6, 16, 32          # csrc/sage_mfma.hip


@pytest.fixture(scope="module")
def lib():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr._lib()


def _same(a, b):
    """bitwise: the float32 words themselves"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _specials(dt):
    fi = torch.finfo(dt)
    # -0, largest finite, smallest and largest subnormal (both signs), smallest normal
    return torch.tensor([-0.0, fi.max, -fi.max, fi.smallest_normal * 2.0 ** -(10 if dt == torch.float16 else 7),
                         -fi.smallest_normal * (1 - 2.0 ** -(10 if dt == torch.float16 else 7)), fi.smallest_normal, fi.tiny],
                        dtype=torch.float64).to(dt)


def _table(rng, rows, H, dt, extremes=True):
    """[rows, H] of dtype dt on the host: normal values, a tenth of them scaled down into the subnormal range, negative
    zeros, and (extremes) the format's special values in row 1 (the largest finite value once per sign, in columns of
    their own: one fp32 sum of a column holds it)"""
    x = torch.from_numpy(rng.standard_normal((rows, H)).astype(np.float32))
    tiny = torch.from_numpy(rng.random((rows, H)) < 0.1)
    x = torch.where(tiny, x * float(torch.finfo(dt).smallest_normal) * 0.37, x)
    x = torch.where(torch.from_numpy(rng.random((rows, H)) < 0.03), torch.full_like(x, -0.0), x)
    t = x.to(dt)
    if extremes and rows > 1:
        sp = _specials(dt)
        t[1, :sp.numel()] = sp[:min(H, sp.numel())]
    assert bool(torch.isfinite(t.float()).all())
    sub = (t.float().abs() > 0) & (t.float().abs() < float(torch.finfo(dt).smallest_normal))
    assert bool(sub.any()) and bool((t.view(torch.int16) == -32768).any())      # subnormals and -0.0 are in
    return t


def _graph(rng, deg, n_src, no_self_every=5):
    deg = np.asarray(deg, dtype=np.int64)
    n = deg.shape[0]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    # (never source 1, the row of special values: a case places it itself, at most once per destination row, so that
    # no neighbour sum holds the largest finite value twice and overflows -- every sum compared here is finite)
    indices = rng.integers(0, n_src - 1, size=int(indptr[-1])).astype(np.int64)
    indices[indices >= 1] += 1
    self_ids = rng.integers(0, n_src, size=n).astype(np.int64)
    if no_self_every:
        self_ids[::no_self_every] = -1
    return indptr, indices, self_ids


def _rowmap(rng, table_rows, n_src):
    """n_src distinct table rows, source 1 -> table row 1 (the row of special values)"""
    m = rng.permutation(table_rows)[:n_src]
    j = np.flatnonzero(m == 1)
    if j.size:
        m[j[0]] = m[1]
    m[1] = 1
    return m


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).int().cuda() if a is not None else None


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _weights(rng, H, out):
    return (torch.from_numpy((rng.standard_normal((out, 2 * H)) / np.sqrt(2 * H)).astype(np.float32)).cuda(),
            torch.from_numpy(rng.standard_normal(out).astype(np.float32)).cuda())


# ---- the fused forward against csl_sage_fwd_mfma_f32 on the upcast table ---------------------------------------------

def _fused_pair(g, t16, W, b, n_pad, relu_in, rowmap, what):
    from cslicer import aggr
    indptr, indices, self_ids = g
    n = indptr.shape[0] - 1
    d = dict(self_ids=_i32(self_ids), indptr=_i32(indptr),
             indices=_i32(indices) if indices.shape[0] else torch.zeros(1, dtype=torch.int32, device="cuda"),
             weight=W, bias=b, n=n, n_pad=n_pad, rowmap=_i32(rowmap), relu_in=relu_in, relu_out=True)
    x16 = t16.cuda()
    x32 = x16.float()
    assert x16.element_size() == 2
    y16, c16 = aggr.sage_fwd_mfma(x16, want_cat=True, **d)
    y32, c32 = aggr.sage_fwd_mfma(x32, want_cat=True, **d)
    y16n = aggr.sage_fwd_mfma(x16, want_cat=False, **d)
    torch.cuda.synchronize()
    assert _same(c16, c32), what + ": cat"
    assert bool(torch.isfinite(c16).all()), what + ": the sums hold the extremes (row 1 at most once per row)"
    assert _same(y16, y32), what + ": y"
    assert _same(y16n, y16), what + ": y without the operand output"
    return c16


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H", [100, 132, 256])
@pytest.mark.parametrize("longest", [0, 1, 6, 7, 12, 13, 16, 17, 40])
def test_fused_forward_row_lengths_on_both_sides_of_every_producer_switch(lib, dtype, H, longest):
    """a workgroup owns ONE tile here (3 tiles, hundreds of CUs); longest row 0 .. 40 takes every producer path at
    H = 100 (one, two, three edge passes, generic), H = 132 and 256 are generic whatever the rows are; n_pad - n of 0, 1, 31;
    with and without a row map, relu_in on and off"""
    dt = DTYPES[dtype]
    rng = np.random.default_rng(1000 * H + longest)
    n, n_src, out = 77, 60, 40
    for extra in (0, 1, 31):
        for mapped in (False, True):
            deg = rng.integers(0, longest + 1, size=n)
            deg[[2, 40, 76]] = longest
            deg[[3, 41]] = max(longest - 1, 0)
            g = _graph(rng, deg, n_src)
            g[2][2], g[2][40], g[2][41] = -1, 7, 1       # a longest row without a self row; row 1 (the extremes) as a self row
            if g[1].shape[0]:
                g[1][0] = 1                              # ... and as a neighbour
            rowmap = _rowmap(rng, 150, n_src) if mapped else None
            t16 = _table(rng, 150 if mapped else n_src, H, dt)
            W, b = _weights(rng, H, out)
            for relu_in in (False, True):
                _fused_pair(g, t16, W, b, n + extra, relu_in, rowmap,
                            "%s H %d longest %d pad %d map %d relu_in %d" % (dtype, H, longest, extra, mapped, relu_in))


def _path_degrees(rng, n, path):
    lo, hi = {1: (4, EC), 2: (EC + 1, 2 * EC), 3: (2 * EC + 1, EMAX), 0: (EMAX + 1, 23)}[path]
    deg = rng.integers(0, 4, size=n)
    pick = rng.random(n) < 0.1
    deg[pick] = rng.integers(lo, hi + 1, size=int(pick.sum()))
    deg[[5, n - 1]] = hi
    return deg


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H,path,relu_in,mapped", [(100, 1, False, True), (100, 2, True, False), (100, 3, False, False),
                                                   (100, 0, True, True), (132, 1, False, True), (256, 0, True, False)])
def test_fused_forward_workgroups_that_own_three_tiles(lib, dtype, H, path, relu_in, mapped):
    """n_pad so large that workgroups own 3 tiles and some 2 (a partial last round): the staged-address buffers and the
    two register sets of raw 16-bit quads rotate over tiles, the last tile is cut by n and by n_pad"""
    dt = DTYPES[dtype]
    cus = _cus()
    rng = np.random.default_rng(path * 100 + H)
    n_tiles = 2 * cus + max(3, cus // 3)
    n = n_tiles * BM - 13
    n_pad = n + 11
    n_src, out = 5000, 40
    g = _graph(rng, _path_degrees(rng, n, path), n_src, no_self_every=7)
    g[1][3], g[2][8] = 1, 1
    rowmap = _rowmap(rng, 9000, n_src) if mapped else None
    t16 = _table(rng, 9000 if mapped else n_src, H, dt)
    W, b = _weights(rng, H, out)
    assert -(-n_pad // BM) == n_tiles and 2 * cus < n_tiles < 3 * cus
    _fused_pair(g, t16, W, b, n_pad, relu_in, rowmap, "%s S 3 path %d H %d" % (dtype, path, H))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_fused_forward_table_as_a_column_block(lib, dtype):
    """the table as a column block of a wider 16-bit buffer: ldx > H (a multiple of 4 elements), base 8-byte aligned but
    not 16"""
    from cslicer import aggr
    dt = DTYPES[dtype]
    rng = np.random.default_rng(5)
    n, n_src, H, out = 300, 120, 100, 47
    g = _graph(rng, rng.integers(0, 15, size=n), n_src)
    wide = _table(rng, n_src, H + 12, dt).cuda()
    x16 = wide[:, 4:4 + H]
    assert x16.data_ptr() % 16 == 8 and x16.stride(0) == H + 12
    W, b = _weights(rng, H, out)
    d = dict(self_ids=_i32(g[2]), indptr=_i32(g[0]), indices=_i32(g[1]), weight=W, bias=b, n=n, n_pad=311, relu_out=True)
    y16, c16 = aggr.sage_fwd_mfma(x16, want_cat=True, **d)
    y32, c32 = aggr.sage_fwd_mfma(x16.float().contiguous(), want_cat=True, **d)
    torch.cuda.synchronize()
    assert _same(y16, y32) and _same(c16, c32)
    # ... and refusals on the device: a base 2 or 4 bytes off, a stride that is not a multiple of 4 elements
    wpack = torch.empty((lib.csl_sage_fwd_mfma_scratch(H, out),), device="cuda")
    y = torch.empty((311, out), device="cuda")

    def rc(x):
        return lib.csl_sage_fwd_mfma_x16(C.c_void_p(d["indptr"].data_ptr()), C.c_void_p(d["indices"].data_ptr()),
                                         C.c_void_p(d["self_ids"].data_ptr()), C.c_void_p(0), C.c_void_p(x.data_ptr()),
                                         aggr.FEAT_KINDS[dt], x.stride(0), C.c_void_p(W.data_ptr()), W.stride(0),
                                         C.c_void_p(b.data_ptr()), n, 311, H, out, 0, 1, C.c_void_p(0), 0,
                                         C.c_void_p(y.data_ptr()), out, C.c_void_p(wpack.data_ptr()), aggr._stream())
    assert rc(wide[:, 2:2 + H]) == -1 and rc(wide[:, 1:1 + H]) == -1
    assert rc(_table(rng, n_src, H + 2, dt).cuda()[:, :H]) == -1
    assert rc(x16) == 0
    torch.cuda.synchronize()


# ---- the two-kernel form, the rank path's sums, the upcasting gather ---------------------------------------------------

@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H", [4, 100, 132, 256, 300])
def test_sage_cat_against_its_fp32_twin(lib, dtype, H):
    from cslicer import aggr
    dt = DTYPES[dtype]
    rng = np.random.default_rng(H)
    n, n_src = 333, 200
    g = _graph(rng, rng.integers(0, 24, size=n), n_src)
    g[1][0], g[2][1] = 1, 1
    for mapped in (False, True):
        rowmap = _rowmap(rng, 500, n_src) if mapped else None
        x16 = _table(rng, 500 if mapped else n_src, H, dt).cuda()
        for relu_in in (False, True):
            for n_pad in (n, n + 1, n + 31):
                a = dict(self_ids=_i32(g[2]), n=n, n_pad=n_pad, indptr=_i32(g[0]), indices=_i32(g[1]), rowmap=_i32(rowmap),
                         relu_in=relu_in)
                c16, c32 = aggr.sage_cat(x16, **a), aggr.sage_cat(x16.float(), **a)
                torch.cuda.synchronize()
                assert _same(c16, c32), (dtype, H, mapped, relu_in, n_pad)
    # the several-parts form: self rows from the 16-bit table through the map, the merged sums (fp32) by owned row
    owned = _i32(rng.permutation(n)[:150])
    deg = _i32(rng.integers(0, 9, size=150))
    agg = torch.from_numpy(rng.standard_normal((n, H)).astype(np.float32)).cuda()
    a = dict(self_ids=_i32(g[2][:150]), n=150, n_pad=160, owned=owned, deg=deg, agg=agg, rowmap=_i32(rowmap))
    c16, c32 = aggr.sage_cat(x16, **a), aggr.sage_cat(x16.float(), **a)
    torch.cuda.synchronize()
    assert _same(c16, c32)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H", [4, 100, 102, 132, 256])
def test_spmm_sum_map_against_its_fp32_twin(lib, dtype, H):
    """(H = 102: a width that is not whole quads -- the table's rows still are, stride 104)"""
    from cslicer import aggr
    dt = DTYPES[dtype]
    rng = np.random.default_rng(H + 1)
    n, n_src = 400, 250
    g = _graph(rng, rng.integers(0, 30, size=n), n_src)
    g[1][0] = 1
    ld = (H + 3) // 4 * 4
    rows = _i32(np.sort(rng.permutation(n)[:170]))
    for mapped in (False, True):
        rowmap = _rowmap(rng, 600, n_src) if mapped else None
        x16 = _table(rng, 600 if mapped else n_src, ld, dt).cuda()[:, :H]
        x32 = x16.float()          # (contiguous [rows, H]: the twin's own layout)
        for compact in (False, True):
            a = dict(rows=rows, rowmap=_i32(rowmap), compact=compact, n_out=n)
            o16 = aggr.spmm_sum_map(_i32(g[0]), _i32(g[1]), x16, **a)
            o32 = aggr.spmm_sum_map(_i32(g[0]), _i32(g[1]), x32, **a)
            torch.cuda.synchronize()
            assert _same(o16, o32), (dtype, H, mapped, compact)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H", [4, 100, 102, 256])
def test_upcasting_gather_writes_its_block_and_nothing_else(lib, dtype, H):
    from cslicer import aggr
    dt = DTYPES[dtype]
    rng = np.random.default_rng(H + 2)
    n_src, n = 300, 411
    ld = (H + 3) // 4 * 4
    x16 = _table(rng, n_src, ld, dt).cuda()[:, :H]
    idx = rng.integers(0, n_src, size=n)
    idx[::9] = -1                                  # (a zero row)
    idx[1] = 1
    want = x16.float()[torch.from_numpy(np.maximum(idx, 0)).cuda()]
    want[torch.from_numpy(idx < 0).cuda()] = 0.0
    got = aggr.gather_rows(x16, _i32(idx))
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and _same(got, want)
    # straight into a wider, row-padded destination: sentinels all round
    S = 9.75
    for off in (0, 4, 3):                          # (a 16-byte aligned block, and one that is not: element-wise stores)
        wide = torch.full((n + 40, H + 12), S, device="cuda")
        aggr.gather_rows(x16, _i32(idx), out=wide[:n, off:off + H])
        torch.cuda.synchronize()
        assert _same(wide[:n, off:off + H], want)
        assert bool((wide[:, :off] == S).all()) and bool((wide[:, off + H:] == S).all()) and bool((wide[n:] == S).all())


# ---- trainers ----------------------------------------------------------------------------------------------------------

def _task(dt, n=12000, F=100, classes=7, seed=3):
    """a small synthetic graph; node 0 is isolated and holds the format's largest finite value (see the module docstring)"""
    from cslicer import l0
    indptr, indices = l0.synth_graph(n, 12.0, seed=seed)
    keep = indices != 0
    keep[indptr[0]:indptr[1]] = False
    rows = np.repeat(np.arange(n), np.diff(indptr))[keep]
    indices = indices[keep]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    assert indptr[1] == 0 and not (indices == 0).any()
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.random((n, F), dtype=np.float32))
    t = torch.where(torch.from_numpy(rng.random((n, F)) < 0.05), t * float(torch.finfo(dt).smallest_normal) * 0.4, t)
    t = torch.where(torch.from_numpy(rng.random((n, F)) < 0.02), torch.full_like(t, -0.0), t)
    labels = np.argmax(t[:, :classes].numpy(), axis=1).astype(np.int64)
    t16 = t.to(dt)
    t16[0, :3] = torch.tensor([torch.finfo(dt).max, -torch.finfo(dt).max, -0.0], dtype=torch.float64).to(dt)
    sub = (t16.float().abs() > 0) & (t16.float().abs() < float(torch.finfo(dt).smallest_normal))
    assert bool(sub.any()) and bool((t16.view(torch.int16) == -32768).any()) and bool(torch.isfinite(t16.float()).all())
    perm = rng.permutation(np.arange(1, n))
    return indptr, indices, t16, labels, perm, classes


def _train_pair(make, dtype, steps, evaluate=False, parameters=True):
    """make(features, **kw) -> trainer: the trainer on the 16-bit table, then on the table upcast to float32, same seeds;
    returns both trainers after asserting that the losses and (parameters) every parameter are bitwise the same"""
    dt = DTYPES[dtype]
    indptr, indices, t16, labels, perm, classes = _task(dt)
    out = []
    for sixteen in (True, False):
        feats = t16 if sixteen else t16.float().numpy()
        tr = make(indptr, indices, feats, labels, classes, **({"feature_dtype": dtype} if sixteen else {}))
        if sixteen:
            assert tr.feat.dtype == dt and tr.feat.element_size() == 2
            assert tr.feat.numel() * tr.feat.element_size() == t16.shape[0] * t16.shape[1] * 2      # N F 2 bytes
            assert torch.equal(tr.feat.cpu().view(torch.int16), t16.view(torch.int16))
        else:
            assert tr.feat.dtype == torch.float32
        tr.set_nodes(perm)
        losses = tr.run(steps)
        params = [p.detach().clone() for p in tr.model.parameters()]
        ev = tr.evaluate(perm[:1500]) if evaluate else None
        out.append((losses, params, ev, tr))
    (l16, p16, e16, tr16), (l32, p32, e32, tr32) = out
    assert len(l16) == steps and all(np.isfinite(l16))
    assert np.array_equal(np.asarray(l16, dtype=np.float32).view(np.uint32), np.asarray(l32, dtype=np.float32).view(np.uint32)), \
        (l16, l32)
    assert len(p16) == len(p32) and (not parameters or all(_same(a, b) for a, b in zip(p16, p32)))
    if evaluate:
        assert e16 == e32 and e16["n"] == 1500, (e16, e32)
    return tr16, tr32


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("hidden,fused", [(256, True), (260, False)])
def test_native_step_on_a_16_bit_table(dtype, hidden, fused):
    """fanout 15/10/5, features 100; hidden 256: the fused deepest layer; hidden 260: a width the fused kernel refuses
    (out > 256), so the two-kernel form (csl_sage_cat_x16 + GEMM) runs.  Evaluation (full-neighbour inference, which works
    on a float32 copy of the table) returns the same dict."""
    from cslicer.train import Trainer

    def make(indptr, indices, feats, labels, classes, **kw):
        return Trainer(indptr, indices, feats, labels, classes, fanouts=(15, 10, 5), batch=256, streams=4, hidden=hidden,
                       lr=1e-2, seed=5, **kw)
    tr16, tr32 = _train_pair(make, dtype, 8, evaluate=True)
    for tr in (tr16, tr32):
        assert tr.native is not None and tr.fused_deepest_layer() == fused
    # step_work counts the gathered table rows at the table's element size: 2 bytes fewer per element than float32
    w16, w32 = tr16.step_work(8), tr32.step_work(8)
    u = tr16.units[0]
    assert u == tr32.units[0] and u["edges"] > 0
    group = "fused_forward" if fused else "aggregation"
    assert w32[group]["bytes"] - w16[group]["bytes"] == (u["rows"] + u["edges"]) / 8 * 100 * 2
    assert w32["aggregation_bytes"] - w16["aggregation_bytes"] == (u["rows"] + u["edges"]) / 8 * 100 * 2
    assert w16["gemm_flops"] == w32["gemm_flops"]
    for tr in (tr16, tr32):
        tr.close()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("model", ["sage", "gat"])
def test_a_width_that_is_no_multiple_of_4(dtype, model, monkeypatch):
    """features 50: the float32 trainer takes such a width through the gathered matrix (no native step), and so does a
    16-bit table -- stored with its rows padded to 52 elements, tr.feat the [N, 50] view, read by the upcasting gather
    (training) and by inference's float32 working copy (evaluation)"""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", True)
    dt = DTYPES[dtype]
    indptr, indices, t16, labels, perm, classes = _task(dt, n=4000)
    t16 = t16[:, :50].contiguous()
    kw = dict(fanouts=(2, 2, 2), batch=128, streams=2, hidden=32, heads=4, model=model, lr=1e-2, seed=5)
    res = []
    for sixteen in (True, False):
        tr = Trainer(indptr, indices, t16 if sixteen else t16.float().numpy(), labels, classes,
                     **({"feature_dtype": dtype} if sixteen else {}), **kw)
        if sixteen:
            assert tr.feat.dtype == dt and tr.feat.shape == (4000, 50) and tr.feat.stride(0) == 52
            assert torch.equal(tr.feat.cpu().contiguous().view(torch.int16), t16.view(torch.int16))
        assert tr.native is None
        tr.set_nodes(perm)
        ev = tr.evaluate(perm[:500])                      # (the weights as seeded: the same in both trainers)
        losses = tr.run(3)
        res.append((losses, ev))
        tr.close()
    (l16, e16), (l32, e32) = res
    assert all(np.isfinite(l16)) and all(np.isfinite(l32))
    # the first step's loss is the forward alone, all of it behind the table, and is compared bitwise; the later steps
    # (the gathered-matrix path's backward, which never sees the table) only have to stay finite
    assert np.float32(l16[0]).view(np.uint32) == np.float32(l32[0]).view(np.uint32), (l16, l32)
    assert e16 == e32 and e16["n"] == 500


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_data_parallel_world_of_one_on_a_16_bit_table(dtype):
    from cslicer.train import DataParallelTrainer

    def make(indptr, indices, feats, labels, classes, **kw):
        return DataParallelTrainer(indptr, indices, feats, labels, classes, 0, 1, None, batch=256, fanouts=(15, 10, 5),
                                   streams=4, hidden=256, lr=1e-2, seed=5, **kw)
    for tr in _train_pair(make, dtype, 8):
        assert tr.native is not None
        tr.close()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_autograd_step_on_a_16_bit_table(dtype, monkeypatch):
    """CSLICER_PY_STEP=1: the same kernels issued through autograd nodes; the deepest layer's csl_sage_cat reads the table"""
    from cslicer.train import Trainer
    monkeypatch.setenv("CSLICER_PY_STEP", "1")

    def make(indptr, indices, feats, labels, classes, **kw):
        return Trainer(indptr, indices, feats, labels, classes, fanouts=(15, 10, 5), batch=256, streams=4, hidden=256,
                       lr=1e-2, seed=5, **kw)
    for tr in _train_pair(make, dtype, 8):
        assert tr.native is None
        tr.close()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_attention_model_on_a_16_bit_table(dtype, monkeypatch):
    """a 16-bit table takes the project-then-aggregate input path (its rows arrive through the upcasting gather, straight
    into the row-padded buffer): the float32 trainer it is compared with has the input-layer shortcut switched off.

    Fanout 2/2/2, because that is where the float32 attention step ITSELF is bitwise reproducible: its backward adds the
    logit gradient of a destination's edges to g_er[r, h] with float atomics, one addend per sampled edge from whichever
    wave gets there first (csl_gat_bwd_t_fused_f32; tests/test_gpu_infer.py measures the resulting run-to-run spread of
    float32 twins).  0 + a + b is the same float in either order (IEEE addition is commutative, the first addend lands on
    a zero), three addends are not -- at fanout 10 two float32 trainers on the SAME table drift apart in the last bits
    after a few steps, and a bitwise comparison would test the atomics' arrival order, not the table.  Everything else in
    the step has a fixed order (by-source lists are sorted, the weight gradient sums its slabs in order).  The deepest
    slice still has more than ROW_PAD rows (256 seeds x up to 15), so the gather writes into a padded buffer."""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", True)
    rows = []

    def make(indptr, indices, feats, labels, classes, **kw):
        return Trainer(indptr, indices, feats, labels, classes, fanouts=(2, 2, 2), batch=256, streams=4, hidden=32,
                       heads=4, model="gat", lr=1e-2, seed=5, **kw)
    for tr in _train_pair(make, dtype, 4):
        assert not tr.gat_input
        rows.append(tr.units[0]["src"] // tr.steps_done)
        tr.close()
    assert rows[0] == rows[1] and rows[0] > splitgnn.ROW_PAD        # (mean rows of the deepest slice per step)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_attention_model_forward_at_fanout_ten(dtype, monkeypatch):
    """the wider fanout of the other trainer cases: the forward has no atomics, so the first step's loss (computed before
    any gradient exists) is bitwise that of the float32 trainer; later steps carry the float32 step's own atomics (see
    test_attention_model_on_a_16_bit_table) and are not compared"""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", True)

    def make(indptr, indices, feats, labels, classes, **kw):
        return Trainer(indptr, indices, feats, labels, classes, fanouts=(10, 10, 10), batch=256, streams=4, hidden=32,
                       heads=4, model="gat", lr=1e-2, seed=5, **kw)
    for tr in _train_pair(make, dtype, 1, parameters=False):
        assert not tr.gat_input
        tr.close()


def test_attention_model_turns_the_input_layer_off_for_a_16_bit_table(monkeypatch):
    """without the switch: float32 keeps the aggregate-then-project input layer, a 16-bit table does not take it"""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", False)
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", False)
    indptr, indices, t16, labels, perm, classes = _task(torch.bfloat16, n=3000)
    kw = dict(fanouts=(10, 10, 10), batch=128, streams=2, hidden=32, heads=4, model="gat")
    a = Trainer(indptr, indices, t16.float().numpy(), labels, classes, **kw)
    b = Trainer(indptr, indices, t16, labels, classes, feature_dtype="bfloat16", **kw)
    assert a.gat_input and not b.gat_input
    b.set_nodes(perm)
    assert all(np.isfinite(b.run(2)))
    a.close()
    b.close()


def test_argument_handling():
    from cslicer.train import Trainer
    indptr, indices, t16, labels, perm, classes = _task(torch.float16, n=2000)
    x = t16.float().numpy() * np.float32(1.001)          # float32 values that are NOT bfloat16 values
    with pytest.raises(ValueError):
        Trainer(indptr, indices, x, labels, classes, fanouts=(5, 5), batch=64, streams=2, hidden=16, feature_dtype="int8")
    tr = Trainer(indptr, indices, x, labels, classes, fanouts=(5, 5), batch=64, streams=2, hidden=16,
                 feature_dtype="bfloat16")
    want = torch.from_numpy(x).to(torch.bfloat16)        # round to nearest even
    assert tr.feat.dtype == torch.bfloat16 and torch.equal(tr.feat.cpu().view(torch.int16), want.view(torch.int16))
    assert not torch.equal(want.float(), torch.from_numpy(x))
    tr.close()
    # a float16 host array, stored as it is; and stored as float32 when nothing is asked for
    h = t16.numpy()
    assert h.dtype == np.float16
    tr = Trainer(indptr, indices, h, labels, classes, fanouts=(5, 5), batch=64, streams=2, hidden=16, feature_dtype="float16")
    assert tr.feat.dtype == torch.float16 and torch.equal(tr.feat.cpu().view(torch.int16), t16.view(torch.int16))
    tr.close()
    tr = Trainer(indptr, indices, h, labels, classes, fanouts=(5, 5), batch=64, streams=2, hidden=16)
    assert tr.feat.dtype == torch.float32 and torch.equal(tr.feat.cpu(), t16.float())
    tr.close()


# ---- the rank path: one process per part over gloo, as tests/test_gpu_train.py launches its ranks -----------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, q, dtype):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "occ-gnn_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cslicer.train import Trainer
        from test_gpu_feat16 import DTYPES, _same, _task
        dt = DTYPES[dtype]
        indptr, indices, t16, labels, perm, classes = _task(dt)
        res = []
        for sixteen in (True, False):
            feats = t16 if sixteen else t16.float().numpy()
            tr = Trainer(indptr, indices, feats, labels, classes, rank=rank, world=world, fanouts=(15, 10, 5), batch=256,
                         streams=4, hidden=256, lr=1e-2, seed=5, dist=dist, rank_path=True,
                         **({"feature_dtype": dtype} if sixteen else {}))
            assert tr.native_rank is not None
            assert tr.feat.dtype == (dt if sixteen else torch.float32) and tr.feat.shape[0] == tr.n_own
            tr.set_nodes(perm)
            losses = tr.run(8)
            res.append((losses, [p.detach().clone() for p in tr.model.parameters()]))
            tr.close()
        (l16, p16), (l32, p32) = res
        same_l = np.array_equal(np.asarray(l16, dtype=np.float32).view(np.uint32),
                                np.asarray(l32, dtype=np.float32).view(np.uint32))
        same_p = all(_same(a, b) for a, b in zip(p16, p32))
        dist.barrier()
        q.put((rank, bool(same_l), bool(same_p), l16, l32))
        dist.destroy_process_group()
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex), None, None, None))
        raise


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("world", [2, 1])
def test_native_rank_step_on_a_16_bit_table(dtype, world):
    """the native rank step on a world of two (boundary rows: csl_spmm_sum_map_x16 + the merged-sums csl_sage_cat_x16) and
    on a world of one with rank_path=True (no boundary rows: the fused kernel), each rank a fresh child process with a
    time limit of its own; in every rank the 16-bit run and the float32 run on the upcast rows agree bitwise"""
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q, dtype)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():         # (its own time limit: a rank that hangs is ended, not waited for)
                p.kill()
                p.join()
    for r_ in res:
        assert not isinstance(r_[1], str), r_[1]
    for p in procs:
        assert p.exitcode == 0
    for rank, same_l, same_p, l16, l32 in res:
        assert same_l, (rank, l16, l32)
        assert same_p, rank
        assert len(l16) == 8 and all(np.isfinite(l16))
