"""The attention model's input layer (aggregate-then-project, csrc/gat_input.hip) on a float16 / bfloat16 feature table
read IN PLACE (include/cslicer_gat_in16.h): both edge passes load 8 bytes per lane and upcast in registers, exactly, so
everything must be BITWISE what the float32 layer computes on the table upcast to float32 -- compared as int32 words --
through aggr.GatInputLayer (MFMA and CSLICER_GAT_IN_LIBGEMM paths), through the C ABI, and through the trainers with
gat_input=True.  One float64 anchor per element type keeps the pair from being wrong together.

Table contents: normal values, negative zeros, subnormals and the format's smallest normal in rows the edges and self
ids reach; the format's largest finite value only in a row nothing reaches (a bfloat16 maximum of 3.4e38 in a sampled row
makes the logits infinite, and the comparison would be about NaNs)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gat_ref
from test_gpu_feat16 import DTYPES, _same, _task, _train_pair
from test_gpu_gat_edges import _attn_grads_close, _rows_close

pytestmark = pytest.mark.gpu

INSTANCES = [(1, 32), (2, 16), (2, 17), (4, 16), (4, 17), (8, 12), (8, 13)]     # (H, max_deg): every <H, ME> the host picks
SLOPE = 0.2


@pytest.fixture(scope="module")
def aggr():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr


def _me(H, max_deg):
    """the edges per row of the kernel instance with_gatin_instance picks"""
    return 32 if H == 1 or max_deg > (12 if H == 8 else 16) else (12 if H == 8 else 16)


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32, device="cuda")


def _table(rng, n_rows, F, dt, spare):
    """[n_rows, F] of dt on the device.  A tenth of the entries are subnormals of dt, 3 % negative zeros, every fifth row
    starts with -0, the smallest and the largest subnormal, the smallest normal; row `spare` (which no edge and no self id
    reaches) holds the largest finite value of both signs."""
    fi = torch.finfo(dt)
    x = torch.from_numpy(rng.standard_normal((n_rows, F)).astype(np.float32))
    x = torch.where(torch.from_numpy(rng.random((n_rows, F)) < 0.1), x * float(fi.smallest_normal) * 0.37, x)
    x = torch.where(torch.from_numpy(rng.random((n_rows, F)) < 0.03), torch.full_like(x, -0.0), x)
    t = x.to(dt)
    frac = 2.0 ** -(10 if dt == torch.float16 else 7)
    sp = torch.tensor([-0.0, fi.smallest_normal * frac, -fi.smallest_normal * (1 - frac), fi.smallest_normal],
                      dtype=torch.float64).to(dt)
    t[::5, :min(F, 4)] = sp[:min(F, 4)]
    t[spare, :2] = torch.tensor([fi.max, -fi.max], dtype=torch.float64).to(dt)[:2]
    f = t.float()
    assert bool(torch.isfinite(f).all()) and bool(((f.abs() > 0) & (f.abs() < float(fi.smallest_normal))).any())
    assert bool((t.view(torch.int16) == -32768).any())
    return t.cuda()


def _case(H, max_deg, F, n_out, dt, seed, mapped, extra=()):
    """A CSR of n_out destinations (the recipe of test_gpu_gat_edges._graph): degrees in [0, max_deg]; the first rows have
    0, 1 and exactly ME edges (ME: the instance's capacity), so has the last one, every seventh row has max_deg; every 13th
    row has ONE source on all its edges; every sixth destination has no self row.  mapped: the sources reach the table
    through a permutation, else source s is table row s.  extra: degrees of the last rows."""
    rng = np.random.default_rng(seed)
    me = _me(H, max_deg)
    n_src = 2 * n_out + 50
    deg = rng.integers(0, max_deg + 1, size=n_out)
    deg[2::7] = max_deg
    deg[:3] = [me, 1, 0][:n_out]           # (n_out = 1: the one row is full)
    deg[-1] = me
    if len(extra):
        deg[-len(extra):] = extra
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = rng.integers(0, n_src, size=int(indptr[-1]))
    for r in range(4, n_out, 13):
        indices[indptr[r]:indptr[r + 1]] = indices[indptr[r]] if deg[r] else 0
    self_ids = rng.integers(0, n_src, size=n_out)
    self_ids[1::6] = -1
    n_table = n_src + 1 if not mapped else n_src + 98
    spare = n_table - 1                                               # the row of the largest finite values
    rows = _i32(rng.permutation(n_table - 1)[:n_src]) if mapped else None
    table = _table(rng, n_table, F, dt, spare)
    return table, rows, _i32(indptr), _i32(indices), _i32(self_ids), deg


def _params(H, D, F, seed):
    torch.manual_seed(seed)
    weight = torch.randn(H * D, F, device="cuda") / F ** 0.5
    al, ar = torch.randn(H, D, device="cuda") / D ** 0.5, torch.randn(H, D, device="cuda") / D ** 0.5
    return weight, al, ar, 0.1 * torch.randn(H * D, device="cuda")


def _layer(aggr, table, rows, params, indptr, indices, self_ids, n_out, max_deg, w, elu=True):
    leaves = [p.detach().clone().requires_grad_() for p in params]
    out = aggr.GatInputLayer.apply(table, rows, *leaves, indptr, indices, self_ids, n_out, int(indices.numel()), max_deg,
                                   SLOPE, elu, 0, False)
    out.backward(w)
    torch.cuda.synchronize()
    return [out.detach()] + [p.grad for p in leaves]


NAMES = ("out", "grad weight", "grad attn_l", "grad attn_r", "grad bias")


def _assert_layers_same(aggr, table16, table32, rows, params, g, n_out, max_deg, w, what, skip=None, elu=True):
    a = _layer(aggr, table16, rows, params, *g, n_out, max_deg, w, elu)
    b = _layer(aggr, table32, rows, params, *g, n_out, max_deg, w, elu)
    for name, x, y in zip(NAMES, a, b):
        if skip is not None and name == "out":
            assert torch.equal(torch.isnan(x), torch.isnan(y)), what
            x, y = x[~skip], y[~skip]
        assert _same(x, y), "%s: %s differs from the float32 layer's" % (what, name)
    return a, b


def _abi_pair(aggr, kind, table16, table32, rows, g, H, F, n_out, max_deg, seed):
    """csl_gat_in_fwd_x16 / _bwd_x16 against csl_gat_in_fwd_f32 / _bwd_f32: (agg, alpha), (g_vl, g_vr) of both"""
    L = aggr._lib()
    indptr, indices, self_ids = g
    n_edges = int(indices.numel())
    torch.manual_seed(seed)
    vl, vr = torch.randn(H, F, device="cuda") / F ** 0.5, torch.randn(H, F, device="cuda") / F ** 0.5
    dagg = torch.randn(n_out, H * F, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)      # noqa: E731
    st = aggr._stream()
    res = []
    for table, k in ((table16, kind), (table32, None)):
        agg = torch.full((n_out, H * F), 7.0, device="cuda")
        alpha = torch.full((max(n_edges, 1), H), 7.0, device="cuda")
        head = (p(indptr), p(indices), p(self_ids), p(rows), p(table)) + (() if k is None else (k,))
        fwd = L.csl_gat_in_fwd_f32 if k is None else L.csl_gat_in_fwd_x16
        assert fwd(*head, table.stride(0), F, p(vl), p(vr), H, SLOPE, n_out, n_edges, max_deg, p(agg), p(alpha), st) == 0
        gv = torch.full((2, H, F), 7.0, device="cuda")
        buf = torch.empty((max(int(L.csl_gat_in_bwd_scratch(n_out, H, F)), 4),), device="cuda")
        bwd = L.csl_gat_in_bwd_f32 if k is None else L.csl_gat_in_bwd_x16
        assert bwd(*head, table.stride(0), F, p(alpha), p(dagg), H * F, F, H, SLOPE, n_out, n_edges, max_deg, p(gv[0]),
                   p(gv[1]), p(buf), st) == 0
        torch.cuda.synchronize()
        res.append((agg, alpha, gv))
    return res


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("F", [4, 100, 128])            # one lane on, 25 of 32, all
@pytest.mark.parametrize("H,max_deg", INSTANCES)
def test_every_instance_is_bitwise_the_float32_layer(aggr, dtype, H, max_deg, F, monkeypatch):
    """n_out of 1, 8 and 700, through a permutation row map and without one; the layer on both of its paths and the two
    edge passes through the C ABI"""
    dt, D = DTYPES[dtype], 16
    assert aggr.gat_input_ok(H, F, max_deg, D) and aggr._lib().csl_gat_in_proj_ok(H, F, D)
    params = _params(H, D, F, H + F)
    for n_out, mapped in ((1, True), (8, False), (700, True), (700, False)):
        seed = 1000 * H + 10 * max_deg + F + n_out
        table, rows, *g, deg = _case(H, max_deg, F, n_out, dt, seed, mapped)
        assert deg.max() == _me(H, max_deg) and (n_out < 3 or (deg[1] == 1 and deg[2] == 0))
        table32 = table.float()
        w = torch.randn(n_out, H * D, device="cuda")
        what = "n_out %d, %s" % (n_out, "row map" if mapped else "no row map")
        for libgemm in (False, True):
            if libgemm:
                monkeypatch.setenv("CSLICER_GAT_IN_LIBGEMM", "1")
            else:
                monkeypatch.delenv("CSLICER_GAT_IN_LIBGEMM", raising=False)
            a, _ = _assert_layers_same(aggr, table, table32, rows, params, g, n_out, max_deg, w,
                                       what + (", libgemm" if libgemm else ", mfma"))
            assert all(bool(torch.isfinite(t).all()) for t in a)
        (agg16, alpha16, gv16), (agg32, alpha32, gv32) = _abi_pair(aggr, aggr.FEAT_KINDS[dt], table, table32, rows, g, H, F,
                                                                   n_out, max_deg, seed)
        assert _same(agg16, agg32) and _same(alpha16, alpha32), what + ": csl_gat_in_fwd_x16"
        assert _same(gv16, gv32), what + ": csl_gat_in_bwd_x16"
        assert bool(torch.isfinite(agg16).all()) and bool(torch.isfinite(gv16).all())
        assert not bool((agg16 == 7.0).all()) and not bool((gv16 == 7.0).any())      # (written, not the fill)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_rows_past_one_grid_stride(aggr, dtype):
    """6,145 rows: the forward's 768 workgroups x 8 rows walk a second pass, the backward's workgroups take 8 rows each"""
    dt, H, max_deg, F, D, n_out = DTYPES[dtype], 8, 12, 100, 16, 6145
    table, rows, *g, _ = _case(H, max_deg, F, n_out, dt, 77, True)
    table32 = table.float()
    w = torch.randn(n_out, H * D, device="cuda")
    _assert_layers_same(aggr, table, table32, rows, _params(H, D, F, 3), g, n_out, max_deg, w, "6145 rows")
    (agg16, alpha16, gv16), (agg32, alpha32, gv32) = _abi_pair(aggr, aggr.FEAT_KINDS[dt], table, table32, rows, g, H, F, n_out,
                                                               max_deg, 5)
    assert _same(agg16, agg32) and _same(alpha16, alpha32) and _same(gv16, gv32)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H,max_deg", [(8, 12), (2, 17)])
def test_table_as_a_column_block(aggr, dtype, H, max_deg, monkeypatch):
    """table = wide[:, 4:4 + F] of a wider 16-bit matrix: ldx > F and a base that is 8-byte but not 16-byte aligned (what
    the float32 kernel could not take); NaN sentinel columns on both sides, which a lane that read outside its block
    would carry into the result.  Compared with the float32 layer on a contiguous upcast copy."""
    dt, F, D, n_out = DTYPES[dtype], 100, 16, 700
    monkeypatch.delenv("CSLICER_GAT_IN_LIBGEMM", raising=False)
    table, rows, *g, _ = _case(H, max_deg, F, n_out, dt, 11 + H, True)
    wide = torch.full((table.shape[0], F + 12), float("nan"), dtype=dt, device="cuda")
    wide[:, 4:4 + F] = table
    block = wide[:, 4:4 + F]
    assert block.stride(0) == F + 12 and block.data_ptr() % 16 == 8
    table32 = table.float().contiguous()
    w = torch.randn(n_out, H * D, device="cuda")
    a, _ = _assert_layers_same(aggr, block, table32, rows, _params(H, D, F, 9), g, n_out, max_deg, w, "column block")
    assert all(bool(torch.isfinite(t).all()) for t in a)
    (agg16, alpha16, gv16), (agg32, alpha32, gv32) = _abi_pair(aggr, aggr.FEAT_KINDS[dt], block, table32, rows, g, H, F, n_out,
                                                               max_deg, 13)
    assert _same(agg16, agg32) and _same(alpha16, alpha32) and _same(gv16, gv32)
    assert bool(torch.isnan(wide[:, :4].float()).all()) and bool(torch.isnan(wide[:, 4 + F:].float()).all())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("H,max_deg", [(8, 12), (2, 16), (1, 32)])
def test_an_over_long_row_is_nan_as_in_the_float32_twin(aggr, dtype, H, max_deg, monkeypatch):
    """a row of ME + 1 edges under max_deg = ME: the same NaN rows and NaN attention gradients as the float32 layer,
    every other row bitwise equal"""
    dt, F, D, n_out = DTYPES[dtype], 20, 16, 500
    monkeypatch.delenv("CSLICER_GAT_IN_LIBGEMM", raising=False)
    table, rows, *g, deg = _case(H, max_deg, F, n_out, dt, 31 + H, True, extra=[max_deg + 1] * 2)
    over = torch.as_tensor(deg > max_deg, device="cuda")
    assert int(over.sum()) == 2
    w = torch.randn(n_out, H * D, device="cuda")
    # (no ELU: its derivative at a NaN output would carry the NaN into the bias gradient, which the edges do not feed)
    a, b = _assert_layers_same(aggr, table, table.float(), rows, _params(H, D, F, 4), g, n_out, max_deg, w, "over-long row",
                               skip=over, elu=False)
    for res in (a, b):
        assert bool(torch.isnan(res[0][over]).all()) and not bool(torch.isnan(res[0][~over]).any())
        assert all(bool(torch.isnan(t).all()) for t in res[1:4]) and bool(torch.isfinite(res[4]).all())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_float64_anchor(aggr, dtype, monkeypatch):
    """(H, max_deg) = (8, 12), F = 100, D = 32, 700 rows against tests/gat_ref.py on table.double(): outputs within 1e-5 of
    the row's largest entry, gradients within 1e-4 of the tensor's largest entry"""
    dt, H, max_deg, F, D, n_out = DTYPES[dtype], 8, 12, 100, 32, 700
    monkeypatch.delenv("CSLICER_GAT_IN_LIBGEMM", raising=False)
    table, rows, *g, _ = _case(H, max_deg, F, n_out, dt, 21, True)
    params = _params(H, D, F, 6)
    w = torch.randn(n_out, H * D, device="cuda")
    got = _layer(aggr, table, rows, params, *g, n_out, max_deg, w)
    p64 = [p.detach().double().requires_grad_() for p in params]
    ref = gat_ref.input_layer(table.double(), rows, *p64, *g, SLOPE, True)
    ref.backward(w.double())
    _rows_close(got[0], ref.detach(), 1e-5, "out")
    _attn_grads_close(("weight", "attn_l", "attn_r", "bias"), got[1:], [p.grad for p in p64], 1e-4, False)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("libgemm", [True, False], ids=["libgemm", "mfma"])
def test_no_float32_copy_of_the_table(aggr, dtype, libgemm, monkeypatch):
    """A table of 200,000 x 128 (51 MB in 16 bits), a layer of 256 destinations, H = 8, D = 32: over forward + backward the
    peak of torch's allocations rises by less than N F 2 bytes -- a float32 copy of the table alone is N F 4.

    What the layer allocates itself is summed from its shapes below, and the rise may not exceed that sum by more than
    2 MiB: torch's allocator may hand out a cached block up to 1 MiB larger than asked for without splitting it, and
    1 MiB covers its 512-byte rounding of some twenty tensors and the [H, D, F]-sized temporaries of the library path's
    chain rule.  On the library-GEMM path that sum is 3.3 MB and the rise is held against N F 2 as it stands.  The MFMA
    path's backward takes csl_gat_in_proj_bwd_scratch(H, F, D) floats for the weight gradient's partial sums -- 67 MB at
    this shape whatever the table is -- so there the rise BEYOND that scratch is held against N F 2."""
    dt, N, F, H, D, n_out, max_deg = DTYPES[dtype], 200_000, 128, 8, 32, 256, 10
    if libgemm:
        monkeypatch.setenv("CSLICER_GAT_IN_LIBGEMM", "1")
    else:
        monkeypatch.delenv("CSLICER_GAT_IN_LIBGEMM", raising=False)
    L = aggr._lib()
    rng = np.random.default_rng(2)
    table = (torch.randn(N, F, device="cuda") * 0.5).to(dt)
    deg = np.full(n_out, max_deg)
    indptr, indices = _i32(np.concatenate([[0], np.cumsum(deg)])), _i32(rng.integers(0, 3000, size=int(deg.sum())))
    self_ids, rows = _i32(rng.integers(0, 3000, size=n_out)), _i32(rng.permutation(N)[:3000])
    params = [p.requires_grad_() for p in _params(H, D, F, 8)]
    w = torch.randn(n_out, H * D, device="cuda")
    n_edges, Cw, f4 = int(indices.numel()), H * D, 4
    FP = F if libgemm else int(L.csl_gat_in_proj_fpad(F))
    own = f4 * (n_out * H * F + n_edges * H + n_out * Cw)                       # agg, alpha, out: kept for the backward
    own += f4 * (n_out * Cw + Cw + n_out * H * FP + 2 * H * D * F + 2 * H * F + 2 * H * D)   # gg, g_bias, dagg, gW (twice), g_v, g_a
    own += f4 * 3 * H * F                                                       # v_l, v_r (library path) / the forward's scratch
    scratch = 0
    if libgemm:
        own += f4 * max(int(L.csl_elu_bwd_colsum_scratch(n_out, Cw)), int(L.csl_gat_in_bwd_scratch(n_out, H, F)), 4)
        assert own + (2 << 20) < N * F * 2
    else:
        scratch = f4 * int(L.csl_gat_in_proj_bwd_scratch(H, F, D))
        own += f4 * int(L.csl_gat_in_layer_bwd_scratch(n_out, H, F, D))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = aggr.GatInputLayer.apply(table, rows, *params, indptr, indices, self_ids, n_out, n_edges, max_deg, SLOPE, True, 0,
                                   False)
    out.backward(w)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("rise %d bytes, own buffers %d, of them scratch %d, N F 2 = %d" % (rise, own, scratch, N * F * 2))
    assert rise <= own + (2 << 20)
    assert rise - scratch < N * F * 2
    assert all(bool(torch.isfinite(p.grad).all()) for p in params)


# ---- trainers --------------------------------------------------------------------------------------------------------

def _gat(cls, fanouts, *lead):
    def make(indptr, indices, feats, labels, classes, **kw):
        # the 16-bit trainer asks for the input layer; the float32 trainer's default (auto) has it on
        on = {"gat_input": True} if "feature_dtype" in kw else {}
        return cls(indptr, indices, feats, labels, classes, *lead, fanouts=fanouts, batch=256, streams=4, hidden=32, heads=4,
                   model="gat", lr=1e-2, seed=5, **on, **kw)
    return make


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_trainer_with_the_input_layer_on_a_16_bit_table(dtype, monkeypatch):
    """fanout 2/2/2 (where the float32 attention step itself is bitwise reproducible: see
    test_gpu_feat16.test_attention_model_on_a_16_bit_table): four steps' losses, every parameter and evaluate() on 1,500
    nodes are those of the float32 trainer on the upcast table"""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", False)
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", False)
    tr16, tr32 = _train_pair(_gat(Trainer, (2, 2, 2)), dtype, 4, evaluate=True)
    assert tr16.gat_input and tr32.gat_input
    assert tr16.feat.dtype == DTYPES[dtype] and tr16.eng.flags == tr32.eng.flags      # (no by-source slice of the deepest layer)
    tr16.close()
    tr32.close()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_trainer_forward_at_fanout_ten(dtype, monkeypatch):
    """the first step's loss alone: the upper layers' float atomics make later steps of two float32 trainers differ"""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", False)
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", False)
    for tr in _train_pair(_gat(Trainer, (10, 10, 10)), dtype, 1, parameters=False):
        assert tr.gat_input
        tr.close()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_data_parallel_world_of_one(dtype, monkeypatch):
    from cslicer import splitgnn
    from cslicer.train import DataParallelTrainer
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", False)
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", False)
    for tr in _train_pair(_gat(DataParallelTrainer, (2, 2, 2), 0, 1, None), dtype, 4):
        assert tr.gat_input
        tr.close()


def test_gat_input_false_is_the_switch(monkeypatch):
    """gat_input=False on a float32 table: the losses of a trainer built under splitgnn._NO_GAT_INPUT, bitwise"""
    from cslicer import splitgnn
    from cslicer.train import Trainer
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", False)
    indptr, indices, t16, labels, perm, classes = _task(torch.float16)
    kw = dict(fanouts=(2, 2, 2), batch=256, streams=4, hidden=32, heads=4, model="gat", lr=1e-2, seed=5)
    losses = []
    for switch in (False, True):
        monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", switch)
        tr = Trainer(indptr, indices, t16.float().numpy(), labels, classes, **({} if switch else {"gat_input": False}), **kw)
        assert not tr.gat_input
        assert tr.eng.flags & 8                                   # FLAG_TRANSPOSE_ALL: the deepest layer projects its sources
        tr.set_nodes(perm)
        losses.append(np.asarray(tr.run(4), dtype=np.float32))
        tr.close()
    assert np.isfinite(losses[0]).all() and np.array_equal(losses[0].view(np.uint32), losses[1].view(np.uint32)), losses
