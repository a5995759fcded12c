"""Full-neighbour inference reading a 16-bit feature table in place (include/cslicer_infer16.h) on the GPU box.

Both upcasts to float32 are exact and everything behind the load is the float32 code, so nothing here has a tolerance:
every comparison is BITWISE (the float32 words as int32) against the float32 twin / the same call on `table.float()`; the
float32 side is pinned against float64 by tests/test_gpu_infer.py and tests/test_gpu_infer_parts.py.

Table contents as in tests/test_gpu_feat16.py::_task: subnormals of the format and -0.0 sprinkled in, and the format's
largest finite values on an isolated node only (node / source 0: its own row is read as a self row, no sum holds it).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEG = 512
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
KIND = {"float16": 1, "bfloat16": 2}
S = 9.75                 # sentinel around every output
MB = 1 << 20


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _table(rng, rows, H, dt):
    """[rows, H] of dtype dt on the host: values in [0, 1), 5 % of them scaled into the format's subnormal range, 2 %
    negative zeros; row 0 starts with the largest finite value of either sign"""
    t = torch.from_numpy(rng.random((rows, H), dtype=np.float32))
    t = torch.where(torch.from_numpy(rng.random((rows, H)) < 0.05), t * float(torch.finfo(dt).smallest_normal) * 0.4, t)
    t = torch.where(torch.from_numpy(rng.random((rows, H)) < 0.02), torch.full_like(t, -0.0), t)
    t16 = t.to(dt)
    t16[0, :3] = torch.tensor([torch.finfo(dt).max, -torch.finfo(dt).max, -0.0], dtype=torch.float64).to(dt)
    if rows * H >= 400:
        sub = (t16.float().abs() > 0) & (t16.float().abs() < float(torch.finfo(dt).smallest_normal))
        assert bool(sub.any()) and bool((t16.view(torch.int16) == -32768).any())
    assert bool(torch.isfinite(t16.float()).all())
    return t16


def _block(t16, ld):
    """the table on the device with row stride ld: itself (ld == H), or columns 4 .. 4 + H of a wider 16-bit buffer (an
    8-byte aligned base that is not 16-byte aligned)"""
    H = t16.shape[1]
    if ld == H:
        return t16.cuda()
    wide = torch.full((t16.shape[0], ld), 3.0, dtype=t16.dtype)
    wide[:, 4:4 + H] = t16
    x = wide.cuda()[:, 4:4 + H]
    assert x.stride(0) == ld and x.data_ptr() % 16 == 8
    return x


def _p(t, off=0):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


# ------------------------------------------------------------------ kernel twins

# one item, exactly SEG, hubs of 2 and 3 parts; a few short rows between them
# (a hub in either half: called in two chunks, the second starts at part 2)
LENS = [0, 1, 513, 7, 8, 9, 63, 64, 65, 512, 1300, 3, 0, 5]
N_SRC = 300


def _csr(lens, seed):
    """rows of `lens` entries over sources 1 .. N_SRC - 1 (never 0, the row of the largest finite values)"""
    rng = np.random.default_rng(seed)
    ip = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    return ip, rng.integers(1, N_SRC, int(ip[-1])).astype(np.int32)


def _cuts(w, n, two):
    """the plan of n rows as one call or as two (pos0 / part0 != 0 in the second)"""
    out = []
    for s0, s1 in (((0, n // 2), (n // 2, n)) if two else ((0, n),)):
        h0, h1 = (int(x) for x in np.searchsorted(w["hub_pos"], [s0, s1]))
        out.append((s0, s1, int(w["item_first"][s0]), int(w["item_first"][s1]), h0, h1, int(w["part_first"][s0]),
                    int(w["part_first"][s1] - w["part_first"][s0])))
    return out


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("W", [4, 100, 256, 260])
def test_infer_sage_x16_against_its_float32_twin(dtype, W):
    """csl_infer_sage_x16 (aggregate-first: [x[v] | mean x[u]]) over rows of every length class, as one call and as two,
    the table contiguous and as a column block; out and partial inside sentinels"""
    from cslicer import aggr, infer
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    L = infer._lib()
    n = len(LENS)
    ip, ix = _csr(LENS, W)
    w = infer.build_plan(ip)
    assert w["hubs"].shape[0] == 2 and w["n_parts"] == 5
    items, hubs = torch.from_numpy(w["items"]).to(dev), torch.from_numpy(w["hubs"]).to(dev)
    dip, dix = torch.from_numpy(ip.astype(np.int32)).to(dev), torch.from_numpy(ix).to(dev)
    t16 = _table(np.random.default_rng(W + 1), N_SRC, W, dt)
    x32 = t16.float().to(dev)
    st = aggr._stream()
    ldo = 2 * W + 8

    def run(x, ldx, two):
        out = torch.full((n + 2, ldo), S, device=dev)
        parts = []
        for s0, s1, i0, i1, h0, h1, p0, npart in _cuts(w, n, two):
            part = torch.full((npart + 2, W), S, device=dev)
            args = (_p(dip), _p(dix), _p(items, 4 * i0), i1 - i0, _p(hubs, 4 * h0), h1 - h0, s0, p0, _p(x))
            rest = (ldx, W, 0, None, 0, _p(part, W), _p(out, (1 + s0) * ldo + 4), ldo, st)
            rc = (L.csl_infer_sage_f32(*args, *rest) if x.dtype == torch.float32
                  else L.csl_infer_sage_x16(*args, KIND[dtype], *rest))
            assert rc == 0
            parts.append(part)
        torch.cuda.synchronize()
        for part in parts:
            assert bool((part[0] == S).all()) and bool((part[-1] == S).all())
        assert bool((out[0] == S).all()) and bool((out[-1] == S).all())
        assert bool((out[:, :4] == S).all()) and bool((out[:, 4 + 2 * W:] == S).all())
        return out[1:-1, 4:4 + 2 * W], torch.cat([p[1:-1] for p in parts])

    want, want_p = run(x32, W, False)
    assert bool(torch.isfinite(want).all())
    assert _same(want[0, :3], t16[0, :3].float().to(dev))            # the largest finite values, as a self row
    for ld in (W, W + 12):
        x16 = _block(t16, ld)
        for two in (False, True):
            got, got_p = run(x16, ld, two)
            assert _same(got, want), (dtype, W, ld, two)
            assert _same(got_p, want_p), (dtype, W, ld, two)
    got2, _ = run(x32, W, True)
    assert _same(got2, want)
    # proj != 0: refused (the projected operand is float32)
    x16 = _block(t16, W)
    out = torch.empty((n, ldo), device=dev)
    assert L.csl_infer_sage_x16(_p(dip), _p(dix), _p(items), 1, None, 0, 0, 0, _p(x16), KIND[dtype], W, W, 1, None, 0, None,
                                _p(out), ldo, st) == -1


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("W", [4, 100, 256, 260])
@pytest.mark.parametrize("pack", [1, 2, 4])
def test_infer_sage_part_x16_against_its_float32_twin(dtype, W, pack):
    """csl_infer_sage_part_x16 over a sub-CSR (the `pack` values of tests/test_gpu_infer_parts.py), as one call and as
    two"""
    from cslicer import aggr, infer
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    L = infer._lib()
    n = len(LENS)
    ip, ix = _csr(LENS, W + pack)
    w = infer.build_plan(ip)
    items, hubs = torch.from_numpy(w["items"]).to(dev), torch.from_numpy(w["hubs"]).to(dev)
    dip, dix = torch.from_numpy(ip.astype(np.int32)).to(dev), torch.from_numpy(ix).to(dev)
    t16 = _table(np.random.default_rng(W + 2), N_SRC, W, dt)
    x32 = t16.float().to(dev)
    st = aggr._stream()

    def run(y, ldy, two):
        send = torch.full((n + 2, W), S, device=dev)
        parts = []
        for s0, s1, i0, i1, h0, h1, p0, npart in _cuts(w, n, two):
            part = torch.full((npart + 2, W), S, device=dev)
            args = (_p(dip), _p(dix), _p(items, 4 * i0), i1 - i0, _p(hubs, 4 * h0), h1 - h0, s0, p0, _p(y))
            rest = (ldy, W, pack, _p(part, W), _p(send, (1 + s0) * W), st)
            rc = (L.csl_infer_sage_part_f32(*args, *rest) if y.dtype == torch.float32
                  else L.csl_infer_sage_part_x16(*args, KIND[dtype], *rest))
            assert rc == 0
            parts.append(part)
        torch.cuda.synchronize()
        for part in parts:
            assert bool((part[0] == S).all()) and bool((part[-1] == S).all())
        assert bool((send[0] == S).all()) and bool((send[-1] == S).all())
        return send[1:-1], torch.cat([p[1:-1] for p in parts])

    want, want_p = run(x32, W, False)
    assert bool(torch.isfinite(want).all()) and not bool((want[1] == S).any())
    for ld in (W, W + 12):
        y16 = _block(t16, ld)
        for two in (False, True):
            got, got_p = run(y16, ld, two)
            assert _same(got, want), (dtype, W, pack, ld, two)
            assert _same(got_p, want_p), (dtype, W, pack, ld, two)


def _merge_lists(n, P, seed):
    """destinations with 0, 1, 2 and P partials over a receive buffer of distinct rows, in rank order (the list shapes
    of tests/test_gpu_infer_parts.py::test_sage_merge_kernel)"""
    rng = np.random.default_rng(seed)
    ml = np.full((n, P), -1, dtype=np.int32)
    r = 0
    for i in range(n):
        k = [0, 1, min(2, P), P][i % 4]
        for q in sorted(rng.choice(P, k, replace=False)):
            ml[i, q] = r
            r += 1
    return ml, r


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("W", [4, 100, 256, 260])
def test_infer_sage_merge_x16_against_its_float32_twin(dtype, W):
    from cslicer import aggr, infer
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    L = infer._lib()
    P, n, n_own = 3, 101, 60
    ml, R = _merge_lists(n, P, W)
    rng = np.random.default_rng(W)
    recv = torch.from_numpy(rng.random((R, W), dtype=np.float32) * 2 - 1).to(dev)
    dst = np.stack([rng.integers(0, n_own, n), rng.integers(0, 30, n)], 1).astype(np.int32)
    dst[:, 1][(ml >= 0).sum(1) == 0] = 0
    dst[5, 0] = 0                                                 # the row of the largest finite values as a self row
    t16 = _table(rng, n_own, W, dt)
    x32 = t16.float().to(dev)
    dd, mld = torch.from_numpy(dst).to(dev), torch.from_numpy(ml).to(dev)
    ldo = 2 * W + 8
    st = aggr._stream()

    def run(x, ldx):
        out = torch.full((n + 2, ldo), S, device=dev)
        args = (_p(dd), _p(mld), n, P, _p(recv), _p(x))
        rest = (ldx, W, 0, None, 0, _p(out, ldo + 4), ldo, st)
        rc = (L.csl_infer_sage_merge_f32(*args, *rest) if x.dtype == torch.float32
              else L.csl_infer_sage_merge_x16(*args, KIND[dtype], *rest))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((out[0] == S).all()) and bool((out[-1] == S).all())
        assert bool((out[:, :4] == S).all()) and bool((out[:, 4 + 2 * W:] == S).all())
        return out[1:-1, 4:4 + 2 * W]

    want = run(x32, W)
    assert bool(torch.isfinite(want).all()) and _same(want[5, :3], t16[0, :3].float().to(dev))
    for ld in (W, W + 12):
        assert _same(run(_block(t16, ld), ld), want), (dtype, W, ld)
    assert L.csl_infer_sage_merge_x16(_p(dd), _p(mld), n, P, _p(recv), _p(_block(t16, W)), KIND[dtype], W, W, 1, None, 0,
                                      _p(torch.empty((n, ldo), device=dev)), ldo, st) == -1


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H", [4, 100, 260])
@pytest.mark.parametrize("n", [0, 1, 1000])
def test_upcast_rows_writes_its_block_and_nothing_else(dtype, H, n):
    """source and destination as column blocks of wider buffers, a destination row stride beyond H, rows r0 .. r0 + n of
    the source (a chunk of a table)"""
    from cslicer import aggr, infer
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    L = infer._lib()
    r0 = 3
    t16 = _table(np.random.default_rng(H + n), n + 5, H, dt)
    for ld in (H, H + 12):
        src = _block(t16, ld)
        wide = torch.full((n + 2, H + 16), S, device=dev)
        rc = L.csl_upcast_rows_x16(_p(src, r0 * ld), KIND[dtype], ld, n, _p(wide, H + 16 + 4), H + 16, H, aggr._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert _same(wide[1:1 + n, 4:4 + H], t16[r0:r0 + n].float().to(dev)), (dtype, H, n, ld)
        assert bool((wide[:, :4] == S).all()) and bool((wide[:, 4 + H:] == S).all())
        assert bool((wide[0] == S).all()) and bool((wide[1 + n:] == S).all())


# ------------------------------------------------------------------ whole calls

def _hub_graph(n=3000, seed=0):
    """rows of 0 and 1 entries, a hub of 3,000 neighbours, rows around SEG, self loops and duplicates; the rest 0 .. 16.
    Node 0 is isolated: no entries of its own, in nobody's row."""
    rng = np.random.default_rng(seed)
    degs = rng.integers(0, 17, n)
    degs[:5] = [0, 1, min(3000, 3 * n), SEG, SEG + 1]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(degs, out=indptr[1:])
    indices = rng.integers(1, n, int(indptr[-1]))
    rows = np.repeat(np.arange(n), degs)
    sl = rng.random(indices.shape[0]) < 0.03
    indices[sl] = rows[sl]
    assert not (indices == 0).any()
    return indptr, indices


MODELS = {
    # name: (constructor arguments after F, nodes of the graph, class of the first layer)
    "sage_agg": (("sage", 128, 7, 2), 3000),        # 100 -> 128: aggregate first (the _x16 kernels)
    "sage_proj": (("sage", 32, 7, 3), 3000),        # 100 -> 32: project first (chunk upcast + GEMM)
    "gat": (("gat", 8, 7, 2, 4), 3000),             # 4 heads x 8
    "gat_wide": (("gat", 260, 7, 2, 1), 400),       # 1 head x 260: Dp > 256, el / er by GEMMs on the table too
}


def _model(name, F, dev, seed=4):
    from cslicer import splitgnn
    a = MODELS[name][0]
    torch.manual_seed(seed)
    if a[0] == "sage":
        return splitgnn.DistSAGEModel(F, a[1], a[2], n_layers=a[3]).to(dev)
    return splitgnn.DistGATModel(F, a[1], a[2], heads=a[4], n_layers=a[3]).to(dev)


def _problem(name, dt, F=100):
    n = MODELS[name][1]
    indptr, indices = _hub_graph(n)
    rng = np.random.default_rng(3)
    t16 = _table(rng, n, F, dt)
    labels = np.argmax(t16[:, :7].float().numpy(), axis=1).astype(np.int64)
    nodes = np.concatenate([rng.permutation(n)[:700], [0, 1, 2, 3, 4]])
    return indptr, indices, t16, labels, nodes


def _spy(monkeypatch):
    """records how full_inference got its 16-bit table: (in place?, dtype and shape of the table the layers read)"""
    from cslicer import infer
    seen = []
    real = infer._table16

    def table16(features, rows, view, dtype, dev):
        h = real(features, rows, view, dtype, dev)
        seen.append((view is not None, h.dtype, tuple(h.shape)))
        return h
    monkeypatch.setattr(infer, "_table16", table16)
    return seen


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(MODELS))
def test_whole_calls_are_bitwise_the_float32_calls(dtype, name, monkeypatch):
    """full_inference and evaluate on the 16-bit device table (read in place) against the same calls on table.float(),
    chunk_rows 256 (many chunks, the hub in one of them) and the default; a host float16 array and a misaligned device
    view take the 16-bit copy and give the same bits"""
    from cslicer import infer
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    indptr, indices, t16, labels, nodes = _problem(name, dt)
    model = _model(name, 100, dev)
    d16 = t16.to(dev)
    d32 = d16.float()
    seen = _spy(monkeypatch)
    for cr in (256, infer.CHUNK_ROWS):
        want = infer.full_inference(model, indptr, indices, d32, nodes=nodes, chunk_rows=cr)
        assert not seen and bool(torch.isfinite(want).all())
        got = infer.full_inference(model, indptr, indices, d16, nodes=nodes, chunk_rows=cr)
        assert seen.pop() == (True, dt, tuple(d16.shape))
        assert _same(got, want), (name, dtype, cr)
        e32 = infer.evaluate(model, indptr, indices, d32, nodes, labels, chunk_rows=cr)
        e16 = infer.evaluate(model, indptr, indices, d16, nodes, labels, chunk_rows=cr)
        assert e16 == e32 and e16["n"] == nodes.shape[0] and np.isfinite(e16["loss"]), (e16, e32)
        seen.clear()
    want = infer.full_inference(model, indptr, indices, d32, chunk_rows=1000)          # every node
    assert _same(infer.full_inference(model, indptr, indices, d16, chunk_rows=1000), want)
    seen.clear()
    # a deliberately misaligned device view (its base 2 bytes off an 8-byte boundary) and a host array: a 16-bit copy
    flat = torch.empty((t16.numel() + 1,), dtype=dt, device=dev)
    off = flat[1:].view(t16.shape)
    off.copy_(d16)
    assert off.data_ptr() % 8 == 2
    inputs = [off, t16] + ([t16.numpy()] if dt == torch.float16 else [])
    for feats in inputs:
        got = infer.full_inference(model, indptr, indices, feats, chunk_rows=1000)
        assert seen.pop() == (False, dt, tuple(t16.shape))
        assert _same(got, want)
    infer.release(indptr, indices)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("model", ["sage", "gat"])
def test_trainer_with_a_width_that_is_no_multiple_of_4_evaluates_in_place(dtype, model, monkeypatch):
    """F = 50 through Trainer(feature_dtype=...): rows stored padded to 52, tr.feat the [N, 50] view; evaluate / predict
    read that storage in place (the trainer vouches for the zero padding) and equal the float32 trainer's.  The same view
    handed to full_inference WITHOUT that word is copied (nothing is guessed from a view)."""
    from cslicer import infer, splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", True)
    dt = DTYPES[dtype]
    indptr, indices = _hub_graph(3000)
    rng = np.random.default_rng(8)
    t16 = _table(rng, 3000, 50, dt)
    labels = np.argmax(t16[:, :7].float().numpy(), axis=1).astype(np.int64)
    nodes = np.concatenate([rng.permutation(3000)[:500], [0, 1, 2, 3, 4]])
    kw = dict(fanouts=(2, 2), batch=128, streams=2, hidden=32, heads=4, model=model, lr=1e-2, seed=5)
    seen = _spy(monkeypatch)
    res = []
    for sixteen in (True, False):
        tr = Trainer(indptr, indices, t16 if sixteen else t16.float().numpy(), labels, 7,
                     **({"feature_dtype": dtype} if sixteen else {}), **kw)
        ev, lg = tr.evaluate(nodes), tr.predict(nodes, chunk_rows=300)
        if sixteen:
            assert tr.feat.dtype == dt and tr.feat.shape == (3000, 50) and tr.feat.stride(0) == 52
            assert seen == [(True, dt, (3000, 52))] * 2
            del seen[:]
            again = infer.full_inference(tr.model, indptr, indices, tr.feat, nodes=nodes, chunk_rows=300)
            assert seen.pop() == (False, dt, (3000, 52)) and _same(again, lg)
        else:
            assert not seen
        res.append((ev, lg))
        tr.close()
    assert res[0][0] == res[1][0] and res[0][0]["n"] == 505, (res[0][0], res[1][0])
    assert _same(res[0][1], res[1][1])


# ------------------------------------------------------------------ no float32 copy

N_BIG, F_BIG, CHUNK_BIG = 20000, 256, 2048
BIG = {
    # widths such that no activation table reaches N F 4 bytes: the aggregate-first layer (out >= in = 256) is the
    # model's only one and is computed for 2,000 nodes
    "sage_agg": ("sage", None, 256, 1),
    "sage_proj": ("sage", 32, 7, 3),
    "gat": ("gat", 8, 7, 2, 4),
    "gat_wide": ("gat", 260, 7, 2, 1),       # (its z table is N x 260 floats -- on both sides of the comparison)
}


def _big_graph(n=N_BIG, seed=1):
    rng = np.random.default_rng(seed)
    degs = rng.integers(0, 9, n)
    degs[2] = 700
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(degs, out=indptr[1:])
    return indptr, rng.integers(1, n, int(indptr[-1]))


def _big_model(name, dev):
    from cslicer import splitgnn
    a = BIG[name]
    torch.manual_seed(2)
    if a[0] == "sage":
        return splitgnn.DistSAGEModel(F_BIG, a[1], a[2], n_layers=a[3]).to(dev)
    return splitgnn.DistGATModel(F_BIG, a[1], a[2], heads=a[4], n_layers=a[3]).to(dev)


def _peak_increase(fn, dev):
    """how far torch's allocated bytes rise above their level before the call (garbage that only the collector frees,
    such as an earlier case's traceback with its frames' tensors, is freed first: freed during the call it would hide
    the rise)"""
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    inc = torch.cuda.max_memory_allocated(dev) - base
    del out
    return inc


def _needed(fn):
    """the "needs %d bytes" figure of the MemoryError raised when 1 KiB is free and torch has no cached blocks"""
    real, reserved = torch.cuda.mem_get_info, torch.cuda.memory_reserved
    torch.cuda.mem_get_info = lambda dev=None: (1024, real(dev)[1])
    torch.cuda.memory_reserved = lambda dev=None: torch.cuda.memory_allocated(dev)
    msg = None
    try:
        fn()
    except MemoryError as ex:
        msg = str(ex)                                        # (only the text is kept: no traceback, no frames)
    finally:
        torch.cuda.mem_get_info, torch.cuda.memory_reserved = real, reserved
    assert msg is not None, "no MemoryError"
    return int(re.search(r"needs (\d+) bytes", msg).group(1))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(BIG))
def test_no_float32_copy_of_a_16_bit_table(dtype, name):
    """N = 20,000, F = 256 (a float32 copy: 20.5 MB), chunk_rows 2048, the graph cached by a first call.  The peak of
    torch's allocations over the call on the 16-bit table in place is at most that of the call on the float32 table in
    place (which copies nothing) plus one upcast buffer (2048 x 256 x 4 = 2 MB) plus 1 MB for the allocator's rounding;
    the bytes the memory check asks for likewise exceed the float32 in-place figure by at most the upcast buffer.
    (Before the table was read in place the rise on a 16-bit table was 42.0 MB for every model here, against 5.9 - 7.8 MB
    on the float32 table: the float32 working copy and the temporary of its conversion.)"""
    from cslicer import infer
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    indptr, indices = _big_graph()
    rng = np.random.default_rng(5)
    d16 = _table(rng, N_BIG, F_BIG, dt).to(dev)
    d32 = d16.float()
    model = _big_model(name, dev)
    nodes = rng.permutation(N_BIG)[:2000]
    up = CHUNK_BIG * F_BIG * 4
    assert N_BIG * F_BIG * 4 > 20e6 and up == 2 * MB

    def call(t):
        return infer.full_inference(model, indptr, indices, t, nodes=nodes, chunk_rows=CHUNK_BIG)
    want = call(d32)                                       # (the graph is on the device now, the GEMM plans are made)
    inc32 = _peak_increase(lambda: call(d32), dev)
    inc16 = _peak_increase(lambda: call(d16), dev)
    need32, need16 = _needed(lambda: call(d32)), _needed(lambda: call(d16))
    print("%s %s: peak increase float32 in place %d, 16-bit in place %d; needs %d and %d bytes"
          % (name, dtype, inc32, inc16, need32, need16))
    assert _same(call(d16), want)
    assert inc16 <= inc32 + up + MB, (inc16, inc32)
    assert need16 <= need32 + up, (need16, need32)
    infer.release(indptr, indices)


# ------------------------------------------------------------------ ranks (gloo, fresh child processes sharing the GPU)

def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, scenario, kw):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "occ-gnn_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_gpu_infer16 import _SCENARIOS
        res = _SCENARIOS[scenario](rank, world, dist, **kw)
        dist.barrier()
        q.put((rank, res))
        dist.destroy_process_group()
    except BaseException as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: %s: %s" % (type(ex).__name__, ex)))
        raise


def _spawn(world, scenario, timeout=150, **kw):
    import torch.multiprocessing as mp
    assert world <= 3
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, scenario, kw)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=timeout) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return [res[r] for r in range(world)]


def _own_rows(t16, world, rank, dev):
    return t16[torch.arange(rank, t16.shape[0], world)].contiguous().to(dev)      # owner v % P, ascending


def _sc_ranks(rank, world, dist, dtype):
    """each rank's full_inference_parts on its 16-bit rows against the call on the same rows upcast: both GraphSAGE
    forms and the attention model, chunk_rows 257 and the default; a world of one against full_inference"""
    from cslicer import infer, splitgnn
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    comm = splitgnn.DistComm(device=dev)
    out = []
    for name in ("sage_agg", "sage_proj", "gat"):
        indptr, indices, t16, labels, nodes = _problem(name, dt)
        model = _model(name, 100, dev)
        o16 = _own_rows(t16, world, rank, dev)
        o32 = o16.float()
        lab = torch.from_numpy(labels)[torch.arange(rank, labels.shape[0], world)].to(dev)
        for cr in (257, infer.CHUNK_ROWS):
            a = infer.full_inference_parts(model, indptr, indices, o16, comm, nodes=nodes, chunk_rows=cr)
            b = infer.full_inference_parts(model, indptr, indices, o32, comm, nodes=nodes, chunk_rows=cr)
            assert a.shape[0] == int(infer.owns(t16.shape[0], world, rank, nodes).sum())
            assert _same(a, b), (name, cr)
            if world == 1:
                assert _same(a, infer.full_inference(model, indptr, indices, o16, nodes=nodes, chunk_rows=cr)), (name, cr)
        ea = infer.evaluate_parts(model, indptr, indices, o16, comm, nodes, lab, chunk_rows=500)
        eb = infer.evaluate_parts(model, indptr, indices, o32, comm, nodes, lab, chunk_rows=500)
        assert ea == eb and ea["n"] == nodes.shape[0], (ea, eb)
        out.append(ea)
        infer.release(indptr, indices)
    return out


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("world", [1, 2, 3])
def test_ranks_on_16_bit_rows_are_bitwise_the_ranks_on_upcast_rows(dtype, world):
    res = _spawn(world, "ranks", dtype=dtype)
    for r in res:
        assert not isinstance(r, str), r
    assert all(r == res[0] for r in res)                         # the same dicts on every rank


def _sc_memory(rank, world, dist, dtype):
    """a rank short of memory makes every rank raise MemoryError before the first exchange (a rank that went on would
    wait in it for ever); then, with the graph's plans on the device, the rank path's share of the no-copy check"""
    from cslicer import infer, splitgnn
    dt, dev = DTYPES[dtype], torch.device("cuda", 0)
    comm = splitgnn.DistComm(device=dev)
    indptr, indices = _big_graph()
    rng = np.random.default_rng(5)
    o16 = _own_rows(_table(rng, N_BIG, F_BIG, dt), world, rank, dev)
    o32 = o16.float()
    n_own = o16.shape[0]
    nodes = rng.permutation(N_BIG)[:2000]
    up = CHUNK_BIG * F_BIG * 4
    out = []
    for name in ("sage_agg", "sage_proj", "gat"):
        model = _big_model(name, dev)

        def call(t):
            return infer.full_inference_parts(model, indptr, indices, t, comm, nodes=nodes, chunk_rows=CHUNK_BIG)
        real, reserved = torch.cuda.mem_get_info, torch.cuda.memory_reserved
        if rank == 1:                                        # 1 KiB free, no cached blocks
            torch.cuda.mem_get_info = lambda dev=None: (1024, real(dev)[1])
            torch.cuda.memory_reserved = lambda dev=None: torch.cuda.memory_allocated(dev)
        needs = []
        for t in (o32, o16):
            try:
                call(t)
                needs.append(None)
            except MemoryError as ex:
                needs.append(int(re.search(r"needs (\d+) bytes", str(ex)).group(1)))
        torch.cuda.mem_get_info, torch.cuda.memory_reserved = real, reserved
        assert None not in needs, "no MemoryError on rank %d" % rank
        want = call(o32)                                     # afterwards the ranks are in step again
        inc32 = _peak_increase(lambda: call(o32), dev)
        inc16 = _peak_increase(lambda: call(o16), dev)
        assert _same(call(o16), want)
        out.append({"model": name, "n_own": n_own, "inc32": inc32, "inc16": inc16, "need32": needs[0], "need16": needs[1],
                    "ok_peak": inc16 <= inc32 + up + MB, "ok_need": needs[1] <= needs[0] + up})
    return out


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_ranks_agree_on_memory_and_make_no_float32_copy(dtype):
    """(the figures of the MemoryError are those of the short rank, rank 1, on every rank)"""
    res = _spawn(2, "memory", dtype=dtype)
    for r in res:
        assert not isinstance(r, str), r
    for r in res:
        for m in r:
            print(dtype, m)
            assert m["n_own"] == N_BIG // 2 and m["n_own"] * F_BIG * 4 > 10e6
            assert m["ok_peak"], m
            assert m["ok_need"], m
    assert [m["need16"] for m in res[0]] == [m["need16"] for m in res[1]]


_SCENARIOS = {"ranks": _sc_ranks, "memory": _sc_memory}
