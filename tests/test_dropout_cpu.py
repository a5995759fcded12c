"""Dropout between the GraphSAGE layers, the part that needs no GPU: the numpy restatement (tests/dropout_ref.py) against
the specification's known answers, the header against what the binder bound, the host-side refusals of the C entry points,
cslicer.train.step_plan with dropout, the constructor's three ValueErrors and the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dropout_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the mask ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = dropout_ref.philox4x32_10(ctr, key)
    assert " ".join("%08x" % int(w) for w in got) == want


def test_counter_layout_pin():
    """ids 1000..1063, H = 256, p = 0.5, seed 12345, layer 1, step 7: 8,202 of 16,384 kept, 109..146 per row"""
    keep = dropout_ref.keep_mask(np.arange(1000, 1064), 256, 0.5, 12345, 1, 7)
    assert keep.shape == (64, 256) and int(keep.sum()) == 8202
    assert int(keep.sum(1).min()) == 109 and int(keep.sum(1).max()) == 146


def test_mask_depends_on_every_part_of_the_counter():
    ids = np.arange(50)
    base = dropout_ref.keep_mask(ids, 64, 0.5, 3, 0, 0)
    assert np.array_equal(base, dropout_ref.keep_mask(ids, 64, 0.5, 3, 0, 1 << 32))          # t mod 2^32
    for other in (dropout_ref.keep_mask(ids, 64, 0.5, 4, 0, 0), dropout_ref.keep_mask(ids, 64, 0.5, 3 + (1 << 32), 0, 0),
                  dropout_ref.keep_mask(ids, 64, 0.5, 3, 1, 0), dropout_ref.keep_mask(ids, 64, 0.5, 3, 0, 1),
                  dropout_ref.keep_mask(ids + 1, 64, 0.5, 3, 0, 0)):
        assert 0.4 < float((other != base).mean()) < 0.6
    # keyed by the node id, not by the row position
    perm = np.random.default_rng(0).permutation(50)
    assert np.array_equal(dropout_ref.keep_mask(ids[perm], 64, 0.5, 3, 0, 0), base[perm])
    # the kept share follows p; the threshold and the scale are the specification's
    assert abs(float(dropout_ref.keep_mask(np.arange(400), 256, 0.1, 1, 0, 0).mean()) - 0.9) < 0.01
    assert dropout_ref.threshold(0.5) == 1 << 31 and dropout_ref.scale(0.5) == np.float32(2)
    assert dropout_ref.threshold(0.1) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32))


def test_threshold_and_scale_at_the_two_ends_of_p():
    """p = 2^-33: threshold 0 and s == 1.0f, nothing is dropped and nothing scaled; p = 1 - 2^-24 (the largest float32
    below 1): threshold 2^32 - 256 and s == 2^24.  tests/test_gpu_dropout_edges.py runs the kernel and the step there."""
    lo, hi = 2.0 ** -33, 1.0 - 2.0 ** -24
    assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi and 0.0 < lo and hi < 1.0
    assert dropout_ref.threshold(lo) == 0 and dropout_ref.scale(lo) == np.float32(1.0)
    assert dropout_ref.scale(lo).view(np.uint32) == np.float32(1.0).view(np.uint32)
    assert dropout_ref.threshold(hi) == (1 << 32) - 256 and dropout_ref.scale(hi) == np.float32(2.0 ** 24)
    assert bool(dropout_ref.keep_mask(np.arange(300), 64, lo, 12345, 1, 7).all())
    # one element in 2^24 is kept: none of these 19,200, and what the map gives is +0.0 whatever the input held
    assert not dropout_ref.keep_mask(np.arange(300), 64, hi, 12345, 1, 7).any()
    x = np.array([[1.5, -0.0, np.inf, np.nan]], dtype=np.float32)
    assert dropout_ref.apply(x, [3], hi, 12345, 1, 7).view(np.uint32).tolist() == [[0, 0, 0, 0]]
    assert np.array_equal(dropout_ref.apply(x, [3], lo, 12345, 1, 7).view(np.uint32)[0, :3], x.view(np.uint32)[0, :3])
    # and the wrapper's scale is the reference's
    from cslicer import aggr
    for p in (lo, 0.1, 0.3, 0.9, hi):
        assert np.float32(aggr.dropout_scale(p)) == dropout_ref.scale(p)


def test_reference_backward_is_autograd_of_the_masked_model():
    """the hand-written float64 backward of dropout_ref.model_on_layers against torch float64 autograd of the same
    forward, on a small random two- and three-layer model: a wrong restatement cannot hide a wrong kernel"""
    import sage_ref
    rng = np.random.default_rng(5)
    for L in (2, 3):
        sizes = [40, 25, 12, 6][:L + 1]
        layers, dims = [], [8] + [12] * (L - 1) + [5]
        for k in range(L):
            n_src, n = sizes[k], sizes[k + 1]
            deg = rng.integers(0, 5, size=n)
            indptr = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(deg, out=indptr[1:])
            layers.append({"indptr": indptr, "indices": rng.integers(0, n_src, size=int(indptr[-1])),
                           "self_ids": rng.permutation(n_src)[:n], "n_src": n_src,
                           "out_nodes": rng.permutation(10 ** 6)[:n]})
        ws = [rng.standard_normal((dims[k + 1], 2 * dims[k])) * 0.3 for k in range(L)]
        bs = [rng.standard_normal(dims[k + 1]) * 0.3 for k in range(L)]
        x0, labels = rng.standard_normal((sizes[0], dims[0])), rng.integers(0, 5, size=sizes[L])
        loss, grads = dropout_ref.model_on_layers(layers, x0, labels, ws, bs, 0.25, 0.5, 9, 2)
        wt = [torch.tensor(w, requires_grad=True) for w in ws]
        bt = [torch.tensor(b, requires_grad=True) for b in bs]
        h = torch.tensor(x0)
        for k, ly in enumerate(layers):
            sid, idx = torch.as_tensor(ly["self_ids"]), torch.as_tensor(ly["indices"])
            rows = sage_ref.csr_rows(ly["indptr"])
            n = sid.numel()
            agg = torch.zeros((n, h.shape[1]), dtype=torch.float64).index_add(0, rows, h[idx])
            deg = torch.bincount(rows, minlength=n).double().clamp(min=1)
            h = torch.cat([h[sid], agg / deg[:, None]], 1) @ wt[k].t() + bt[k]
            if k + 1 < L:
                keep = torch.from_numpy(dropout_ref.keep_mask(ly["out_nodes"], h.shape[1], 0.5, 9, k, 2))
                h = torch.relu(h) * keep * 2.0
        want = torch.nn.functional.cross_entropy(h, torch.as_tensor(labels), reduction="sum") * 0.25
        want.backward()
        assert abs(loss - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        for k in range(L):
            assert torch.allclose(grads[2 * k], wt[k].grad, rtol=1e-10, atol=1e-13)
            assert torch.allclose(grads[2 * k + 1], bt[k].grad, rtol=1e-10, atol=1e-13)
        assert float(sum(g.abs().sum() for g in grads)) > 0


# ---- the C ABI -----------------------------------------------------------------------------------------------------------

def test_header_names_are_what_the_binder_bound():
    from cslicer import _abi, aggr
    L = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_dropout.h")).read(), flags=re.S)
    names = re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src)
    assert names == ["csl_dropout_f32", "csl_scale_segments_f32", "csl_sage_fwd_bwd_dropout"]
    assert "cslicer_dropout.h" in _abi.HEADERS and _abi.BOUND["cslicer_dropout.h"] == names == aggr.DROPOUT_SYMBOLS
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    assert list(L.csl_dropout_f32.argtypes) == [vp, i64, vp, i64, vp, i64, i32, f32, i64, i32, i64, vp]
    assert list(L.csl_scale_segments_f32.argtypes) == [i32, vp, vp, vp, vp]
    assert list(L.csl_sage_fwd_bwd_dropout.argtypes) == [i32, vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, f32, i64, i32, vp, vp,
                                                         vp, i64, vp, f32, i64, i64, vp]
    for n in names:
        assert getattr(L, n).restype is C.c_int


def test_the_kernel_entry_points_refuse_before_any_hip_call():
    """no GPU here: every one of these returns CSL_E_INVALID (-1) from the host-side checks"""
    from cslicer import _abi
    L = _abi.load()
    buf = np.zeros(64 + 8, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16              # a 16-byte aligned host address: never dereferenced
    x, nul, st = C.c_void_p(base), C.c_void_p(0), C.c_void_p(0)
    ok = dict(x=x, ldx=8, y=x, ldy=8, ids=nul, n=4, H=8, p=0.5, seed=1, layer=0, step=0, stream=st)

    def call(**kw):
        return L.csl_dropout_f32(*dict(ok, **kw).values())
    for bad in (dict(p=0.0), dict(p=1.0), dict(p=-0.25), dict(p=1.5), dict(p=float("nan")), dict(x=nul), dict(y=nul),
                dict(n=-1), dict(x=C.c_void_p(base + 4)), dict(y=C.c_void_p(base + 8)), dict(H=6), dict(H=0), dict(ldx=6),
                dict(ldx=10), dict(ldy=4)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0 and call(n=0, x=nul, y=nul) == 0         # no rows: nothing to launch
    seg, cnt, fac = (C.c_void_p * 9)(), (C.c_int64 * 9)(), (C.c_float * 9)()
    assert L.csl_scale_segments_f32(9, seg, cnt, fac, st) == -1    # more than 2 * CSL_MAX_LAYERS
    assert L.csl_scale_segments_f32(-1, seg, cnt, fac, st) == -1
    assert L.csl_scale_segments_f32(2, nul, cnt, fac, st) == -1
    cnt[0] = 5
    assert L.csl_scale_segments_f32(1, seg, cnt, fac, st) == -1    # a null segment with elements
    cnt[0] = -1
    assert L.csl_scale_segments_f32(1, seg, cnt, fac, st) == -1
    cnt[0] = 0
    assert L.csl_scale_segments_f32(1, seg, cnt, fac, st) == 0 and L.csl_scale_segments_f32(0, nul, nul, nul, st) == 0
    # the step: p outside (0, 1) and missing out-node ids, before its layout is even looked at
    dims = (C.c_int32 * 3)(8, 8, 4)
    from cslicer import aggr
    sl = (aggr.SageSlice * 2)()
    sl[0].n_out = 3
    ids = (C.c_void_p * 1)()
    step = lambda p, out_ids: L.csl_sage_fwd_bwd_dropout(2, dims, sl, nul, nul, nul, 0, 8, nul, nul, nul, 1.0, 0, 1, nul, nul,  # noqa: E731
                                                         nul, 0, out_ids, p, 1, 0, st)
    assert step(0.0, ids) == -1 and step(1.0, ids) == -1 and step(0.5, nul) == -1 and step(0.5, ids) == -1
    assert b"dropout" in L.csl_sage_last_error()


# ---- step_plan -------------------------------------------------------------------------------------------------------------

def _rows():
    import test_step_plan_cpu as T
    return T


def test_step_plan_with_dropout():
    """dropout = 0: every tabulated plan is today's.  dropout > 0: the rank path's native_rank becomes the autograd rank
    step -- the plan CSLICER_PY_STEP gives that configuration, engine flags included -- and every other row is unchanged."""
    from cslicer.train import Switches, step_plan
    T = _rows()
    moved = 0
    for row, change, flags, path, gat_input, input_form in T.ROWS:
        cfg = dict(T.BASE, **change)
        sw = Switches(**{k: cfg.pop(k) for k in Switches._fields})
        today = step_plan(sw=sw, **cfg)
        assert tuple(today) == (flags, path, gat_input, input_form), row
        assert step_plan(sw=sw, dropout=0.0, **cfg) == today, row
        got = step_plan(sw=sw, dropout=0.5, **cfg)
        if path == "native_rank":
            moved += 1
            assert got == step_plan(sw=sw._replace(py_step=True), **cfg), row
            assert got.path == "parts" and got.input_form == "rows" and not got.gat_input, row
            assert got.engine_flags == flags & ~T.T, row      # the autograd rank step does not read the slices by source
        else:
            assert got == today, row
    assert moved == 5
    assert step_plan(**dict({k: v for k, v in T.BASE.items() if k not in Switches._fields}, dropout=0.5)).path == "native"


# ---- the constructor and the command line --------------------------------------------------------------------------------

def _tiny():
    indptr = np.arange(9, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, 8, size=16).astype(np.int64)
    return indptr, indices, np.zeros((8, 8), dtype=np.float32), np.zeros(8, dtype=np.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(dropout=1.0), r"dropout must be in \[0, 1\)"), (dict(dropout=-0.1), r"dropout must be in \[0, 1\)"),
    (dict(dropout=0.5, model="gat"), "attention model"), (dict(dropout=0.5, hidden=30), "multiple of 4"),
])
def test_constructor_refuses_before_any_device_call(kw, match, monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats, labels = _tiny()
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, **kw)


def test_command_line_dropout_reaches_the_constructor(monkeypatch):
    from cslicer import l0, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train, "Trainer", fake)
    monkeypatch.setattr(l0, "synth_graph", lambda n, d, seed=0: _tiny()[:2])
    for argv, want in ((["--dropout", "0.5"], 0.5), ([], 0.0)):
        seen.clear()
        with pytest.raises(Stop):
            train.main(["--graph", "synthetic", "--num-layers", "2", "--fan-out", "2,2"] + argv)
        assert seen["dropout"] == want
    assert "--dropout: `Trainer(dropout=...)`" in train.main.__doc__
    ignored = train.main.__doc__.split("Accepted and ignored")[1].split("--eval-split")[0]
    assert "--dropout" not in ignored
