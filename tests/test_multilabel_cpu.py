"""Multi-label classification without a GPU (include/cslicer_multilabel.h): the float64 restatement of
tests/bce_ref.py against torch's own binary_cross_entropy_with_logits, the packed label format, the C ABI as bound and its
refusals, step_plan with `multilabel`, the constructor's refusals, the L0 directory in both label formats, the synthetic
multi-labels and the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bce_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = [1, 31, 32, 33, 64, 65]


# ---- the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3, 33])
def test_restatement_is_torchs_bce_with_logits_in_float64(Cn):
    rng = np.random.default_rng(Cn)
    n = 9
    z = rng.standard_normal((n, Cn)) * 3
    z[0, :] = 80.0
    z[1, :] = -80.0
    z[2, :] = 0.0
    z[3, 0], z[4, 0] = 80.0, -80.0
    y = rng.random((n, Cn)) < 0.5
    y[0, 0], y[1, 0], y[3, 0], y[4, 0] = False, True, True, False
    scale = 1.0 / 7
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    want = scale * torch.nn.functional.binary_cross_entropy_with_logits(zt, torch.tensor(y, dtype=torch.float64),
                                                                        reduction="sum")
    want.backward()
    want = want.detach()
    loss, rows, grad, col = bce_ref.sigmoid_bce(z, y, scale, n_pad=n + 3)
    assert abs(loss - float(want)) <= 1e-13 * abs(float(want))
    assert torch.allclose(grad[:n], zt.grad, rtol=1e-13, atol=1e-300) and bool((grad[n:] == 0).all())
    assert torch.allclose(col, zt.grad.sum(0), rtol=1e-12, atol=1e-18)
    assert torch.allclose(rows.sum(), want, rtol=1e-13)
    # zeros: log 2 per element; +-80 against the label: 80 + log1p(exp(-80)); with it: log1p(exp(-80))
    l, sig = bce_ref.elements(z, y)
    assert torch.allclose(l[2], torch.full((Cn,), np.log(2.0), dtype=torch.float64), rtol=1e-15)
    assert abs(float(l[0, 0]) - 80.0) < 1e-12 and abs(float(l[1, 0]) - 80.0) < 1e-12
    assert 0 < float(l[3, 0]) < 1e-34 and 0 < float(l[4, 0]) < 1e-34
    assert float(sig[2, 0]) == 0.5 and bool(torch.isfinite(l).all())
    lp, cp = bce_ref.block_partials(rows, grad, n + 3)
    assert lp.shape == (3,) and cp.shape == (3, Cn) and torch.allclose(lp.sum(), rows.sum(), rtol=1e-14)
    pred, (tp, fp, fn), lrow = bce_ref.eval_head(z, y)
    assert not pred[2].any() and pred[0].all() and torch.allclose(lrow * scale, rows, rtol=1e-14)
    assert tp + fn == int(y.sum()) and tp + fp == int(pred.sum())
    assert bce_ref.micro_f1(0, 0, 0) == 0.0 and bce_ref.micro_f1(3, 1, 1) == 0.75


# ---- the label format ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", CS)
def test_pack_unpack_round_trip(Cn):
    from cslicer import aggr
    rng = np.random.default_rng(Cn)
    y = rng.random((37, Cn)) < 0.4
    y[0], y[1] = True, False
    w = aggr.pack_labels(y)
    W = (Cn + 31) // 32
    assert w.dtype == np.int32 and w.shape == (37, W) and aggr.label_words(Cn) == W
    assert np.array_equal(w.view(np.uint32), bce_ref.pack(y))                    # class c = bit c % 32 of word c / 32
    assert np.array_equal(aggr.unpack_labels(w, Cn), y) and np.array_equal(bce_ref.unpack(w, Cn), y)
    for other in (y.astype(np.int64), y.astype(np.uint8), torch.from_numpy(y), torch.from_numpy(y.astype(np.int32))):
        assert np.array_equal(aggr.pack_labels(other), w)
    # bits at and above C of the last word: zero as packed, and never looked at when unpacked
    if Cn % 32:
        assert not (w.view(np.uint32)[:, -1] >> np.uint32(Cn % 32)).any()
        g = w.copy()
        g.view(np.uint32)[:, -1] |= np.uint32((0xFFFFFFFF << (Cn % 32)) & 0xFFFFFFFF)
        assert np.array_equal(aggr.unpack_labels(g, Cn), y)
    assert np.array_equal(aggr.unpack_labels(torch.from_numpy(w), Cn), y)
    assert aggr.pack_labels(y[:0]).shape == (0, W)


def test_pack_refuses_anything_but_zero_and_one():
    from cslicer import aggr
    y = np.zeros((4, 5), dtype=np.int64)
    for bad in (2, -1):
        z = y.copy()
        z[2, 3] = bad
        with pytest.raises(ValueError, match="0 or 1"):
            aggr.pack_labels(z)
    with pytest.raises(ValueError):
        aggr.pack_labels(np.zeros((4, 5), dtype=np.float32))
    with pytest.raises(ValueError):
        aggr.pack_labels(np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError):
        aggr.unpack_labels(np.zeros((4, 2), dtype=np.int32), 5)            # y.shape[1] must equal C: one word here
    with pytest.raises(ValueError):
        aggr.unpack_labels(np.zeros((4, 1), dtype=np.int64), 5)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

NAMES = ["csl_sigmoid_bce_scratch", "csl_sigmoid_bce_f32", "csl_sigmoid_bce_partial_f32", "csl_infer_eval_multilabel_f32",
         "csl_sage_fwd_bwd_multilabel"]


def test_header_names_are_what_the_binder_bound():
    from cslicer import _abi, aggr
    L = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_multilabel.h")).read(), flags=re.S)
    assert re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src) == NAMES
    assert "cslicer_multilabel.h" in _abi.HEADERS and _abi.BOUND["cslicer_multilabel.h"] == NAMES == aggr.MULTILABEL_SYMBOLS
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    assert list(L.csl_sigmoid_bce_scratch.argtypes) == [i64] and L.csl_sigmoid_bce_scratch.restype is i64
    assert list(L.csl_sigmoid_bce_f32.argtypes) == [vp, i64, i64, i32, vp, vp, vp, i64, f32, vp, vp, i64, vp, vp]
    assert list(L.csl_sigmoid_bce_partial_f32.argtypes) == [vp, i64, i64, i64, i32, vp, vp, vp, i64, f32, vp, i64, vp, vp, vp]
    assert list(L.csl_infer_eval_multilabel_f32.argtypes) == [vp, i64, i64, i32, vp, i64, vp, vp, vp, vp, vp]
    # csl_sage_fwd_bwd_dropout's list with `labels` -> (label_words, ldw)
    drop = list(L.csl_sage_fwd_bwd_dropout.argtypes)
    assert list(L.csl_sage_fwd_bwd_multilabel.argtypes) == drop[:10] + [vp, i64] + drop[11:]
    for n in NAMES[1:]:
        assert getattr(L, n).restype is C.c_int
    assert [L.csl_sigmoid_bce_scratch(n) for n in (0, 1, 4, 5, 889)] == [0, 1, 1, 2, 223]


def test_entry_points_refuse_before_any_hip_call():
    """no GPU here: every one of these returns CSL_E_INVALID (-1) from the host-side checks"""
    from cslicer import _abi, aggr
    L = _abi.load()
    buf = np.zeros(64, dtype=np.float32)
    x, nul, st = C.c_void_p(buf.ctypes.data), C.c_void_p(0), C.c_void_p(0)       # a host address: never dereferenced
    ok = dict(logits=x, ldl=8, n=4, n_pad=6, C=8, ids=x, rowmap=nul, words=x, ldw=1, scale=1.0, grad=x, ldgr=8, lpart=x,
              cpart=x, stream=st)

    def partial(**kw):
        return L.csl_sigmoid_bce_partial_f32(*dict(ok, **kw).values())
    for bad in (dict(C=4097, ldl=5000, ldgr=5000, ldw=200, cpart=nul), dict(C=257, ldl=300, ldgr=300, ldw=9), dict(C=0),
                dict(n=-1), dict(n_pad=3), dict(logits=nul), dict(ids=nul), dict(words=nul), dict(grad=nul), dict(lpart=nul),
                dict(ldl=7), dict(ldgr=7), dict(ldw=0), dict(C=33, ldl=40, ldgr=40, ldw=1)):
        assert partial(**bad) == -1, bad
    assert partial(n=0, n_pad=0, logits=nul, ids=nul, words=nul, grad=nul, lpart=nul, cpart=nul) == 0   # nothing to launch
    okw = dict(logits=x, ldl=8, n=4, C=8, ids=x, rowmap=nul, words=x, ldw=1, scale=1.0, loss=x, grad=x, ldgr=8, scratch=x,
               stream=st)

    def whole(**kw):
        return L.csl_sigmoid_bce_f32(*dict(okw, **kw).values())
    for bad in (dict(C=4097, ldl=5000, ldgr=5000, ldw=200), dict(C=0), dict(n=-1), dict(logits=nul), dict(ids=nul),
                dict(words=nul), dict(grad=nul), dict(scratch=nul), dict(loss=nul), dict(loss=nul, n=0), dict(ldl=7),
                dict(ldgr=7), dict(ldw=0)):
        assert whole(**bad) == -1, bad
    oke = dict(logits=x, ld=8, n=4, C=8, words=x, ldw=1, pred=x, lrow=x, lsum=x, counts=x, stream=st)

    def head(**kw):
        return L.csl_infer_eval_multilabel_f32(*dict(oke, **kw).values())
    for bad in (dict(C=4097, ld=5000, ldw=200), dict(C=0), dict(n=-1), dict(ld=7), dict(ldw=0), dict(logits=nul),
                dict(words=nul), dict(pred=nul), dict(lrow=nul), dict(lsum=nul), dict(counts=nul), dict(n=0, counts=nul)):
        assert head(**bad) == -1, bad
    # the step: the label words, their stride, the class count, and p / out_ids that do not go together
    dims = (C.c_int32 * 3)(8, 8, 40)
    sl = (aggr.SageSlice * 2)()
    sl[0].n_out = 3
    ids = (C.c_void_p * 1)()

    def step(words=x, ldw=2, p=0.0, out_ids=nul, dims=dims):
        return L.csl_sage_fwd_bwd_multilabel(2, dims, sl, nul, nul, nul, 0, 8, nul, nul, words, ldw, 1.0, 0, 1, nul, nul, nul, 0,
                                             out_ids, p, 1, 0, st)
    assert step(words=nul) == -1 and b"multilabel" in L.csl_sage_last_error()
    assert step(ldw=1) == -1 and step(p=1.0, out_ids=ids) == -1 and step(p=0.5) == -1 and step(p=0.5, out_ids=ids) == -1
    assert step(p=0.0, out_ids=ids) == -1 and step(dims=(C.c_int32 * 3)(8, 8, 4097), ldw=200) == -1
    assert step() == -1 and b"multilabel" not in L.csl_sage_last_error()     # accepted here, refused by the step (null weights)


# ---- step_plan -------------------------------------------------------------------------------------------------------------

def test_step_plan_with_multilabel():
    """multilabel=False: every tabulated plan is the call's without the keyword.  True: the rank path's native_rank becomes
    the autograd rank step -- the plan CSLICER_PY_STEP gives that configuration, engine flags included -- and no other
    row moves (what dropout > 0 does)."""
    import test_step_plan_cpu as T
    from cslicer.train import Switches, step_plan
    moved = 0
    for row, change, flags, path, gat_input, input_form in T.ROWS:
        cfg = dict(T.BASE, **change)
        sw = Switches(**{k: cfg.pop(k) for k in Switches._fields})
        today = step_plan(sw=sw, **cfg)
        assert tuple(today) == (flags, path, gat_input, input_form), row
        assert step_plan(sw=sw, multilabel=False, **cfg) == today, row
        got = step_plan(sw=sw, multilabel=True, **cfg)
        if path == "native_rank":
            moved += 1
            assert got == step_plan(sw=sw._replace(py_step=True), **cfg) == step_plan(sw=sw, dropout=0.5, **cfg), row
            assert got.path == "parts" and got.input_form == "rows" and not got.gat_input, row
            assert got.engine_flags == flags & ~T.T, row
            assert step_plan(sw=sw, multilabel=True, dropout=0.5, **cfg) == got, row
        else:
            assert got == today, row
    assert moved == 5
    base = {k: v for k, v in T.BASE.items() if k not in Switches._fields}
    assert step_plan(**dict(base, multilabel=True)).path == "native"


# ---- the constructor -------------------------------------------------------------------------------------------------------

def _tiny():
    indptr = np.arange(9, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, 8, size=16).astype(np.int64)
    return indptr, indices, np.zeros((8, 8), dtype=np.float32)


def _two():
    y = np.zeros((8, 3), dtype=np.int64)
    y[1, 2] = 2
    return y


@pytest.mark.parametrize("labels,match", [
    (np.zeros(8, dtype=np.int64), "matrix"), (np.zeros((8, 3, 1), dtype=np.int64), "matrix"),
    (np.zeros((8, 4), dtype=np.int64), "n_classes = 3"), (np.zeros((7, 3), dtype=np.int64), "num_nodes = 8"),
    (_two(), "0 or 1"), (-_two(), "0 or 1"), (np.zeros((8, 3), dtype=np.float32), "0 or 1"),
])
def test_constructor_refuses_before_any_device_call(labels, match, monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats = _tiny()
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, multilabel=True)


def test_data_parallel_trainer_passes_the_keyword_through(monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats = _tiny()
    with pytest.raises(ValueError, match="matrix"):
        train.DataParallelTrainer(indptr, indices, feats, np.zeros(8, dtype=np.int64), 3, 0, 1, None, batch=4, fanouts=(2, 2),
                                  streams=1, multilabel=True)


# ---- L0 --------------------------------------------------------------------------------------------------------------------

def _l0_graph(n=11):
    indptr = np.arange(n + 1, dtype=np.int64) * 2
    indices = np.random.default_rng(1).integers(0, n, size=2 * n).astype(np.int64)
    return indptr, indices


@pytest.mark.parametrize("Cn", [5, 32, 70])
def test_l0_multilabel_round_trip_and_checksum(Cn, tmp_path):
    from cslicer import l0
    n = 11
    indptr, indices = _l0_graph(n)
    y = np.random.default_rng(Cn).random((n, Cn)) < 0.5
    y[3] = True                                                       # (words with the top bit set: read as unsigned)
    d = str(tmp_path / "m")
    meta = l0.write_l0(d, indptr, indices, labels=y, num_classes=Cn)
    W = (Cn + 31) // 32
    raw = np.fromfile(os.path.join(d, "labels.bin"), dtype="<u4")
    assert raw.shape == (n * W,) and np.array_equal(raw.reshape(n, W), bce_ref.pack(y))
    assert meta["multilabel"] == 1 and meta["csum_labels"] == int(raw.astype(np.int64).sum())
    text = open(os.path.join(d, "meta.txt")).read()
    assert text.endswith("multilabel=1\n") and ("csum_labels=%d\n" % meta["csum_labels"]) in text
    _, _, m = l0.read_l0(d, mmap=False)                               # (checks the label checksum too)
    assert m["multilabel"] == 1 and m["num_classes"] == Cn
    for mm in (True, False):
        words = l0.read_labels(d, mmap=mm)
        assert words.shape == (n, W) and np.array_equal(l0.unpack_labels(np.asarray(words), Cn), y)
    # one flipped bit is caught, in either reading mode
    raw[W * 5] ^= np.uint32(1)
    raw.tofile(os.path.join(d, "labels.bin"))
    for mm in (True, False):
        with pytest.raises(ValueError, match="labels checksum"):
            l0.read_l0(d, mmap=mm)
    l0.read_l0(d, check=False)
    with pytest.raises(ValueError, match="num_classes"):
        l0.write_l0(str(tmp_path / "x"), indptr, indices, labels=y, num_classes=Cn + 1)
    with pytest.raises(ValueError, match="0 or 1"):
        l0.write_l0(str(tmp_path / "x"), indptr, indices, labels=y.astype(np.int64) * 2, num_classes=Cn)


def test_l0_single_label_directory_is_byte_for_byte_the_documented_format(tmp_path):
    """meta.txt and labels.bin of a single-label directory, computed here from the format l0.py's header documents: no
    new key, int32 labels"""
    from cslicer import l0
    n = 11
    indptr, indices = _l0_graph(n)
    labels = (np.arange(n) * 7) % 5
    feats = (np.arange(n * 3, dtype=np.float32).reshape(n, 3) / 4)
    d = str(tmp_path / "s")
    l0.write_l0(d, indptr, indices, features=feats, labels=labels, num_classes=5)
    assert open(os.path.join(d, "labels.bin"), "rb").read() == labels.astype("<i4").tobytes()
    want = "".join("%s=%d\n" % kv for kv in (
        ("num_nodes", n), ("num_edges", 2 * n), ("feature_dim", 3), ("csum_features", int(feats.sum(dtype=np.float64))),
        ("csum_labels", int(labels.sum())), ("csum_offsets", int(indptr.sum())), ("csum_edges", int(indices.sum())),
        ("num_classes", 5)))
    assert open(os.path.join(d, "meta.txt")).read() == want
    _, _, m = l0.read_l0(d)
    assert "multilabel" not in m and np.array_equal(l0.read_labels(d), labels)
    # the label checksum is checked in this form too
    bad = labels.astype("<i4")
    bad[2] += 1
    bad.tofile(os.path.join(d, "labels.bin"))
    with pytest.raises(ValueError, match="labels checksum"):
        l0.read_l0(d)


# ---- synthetic data and the command line ----------------------------------------------------------------------------------

def test_synthetic_multilabels_are_a_function_of_the_nodes_own_features():
    from cslicer import train
    n, F, Cn = 500, 12, 40
    y = train.synthetic_multilabels(n, Cn, seed=3, feat_dim=F)
    assert y.shape == (n, Cn) and y.dtype == np.bool_ and 0.35 < y.mean() < 0.65
    rows = np.array([7, 499, 0, 7])
    assert np.array_equal(train.synthetic_multilabels(n, Cn, seed=3, rows=rows, feat_dim=F), y[rows])
    assert not np.array_equal(train.synthetic_multilabels(n, Cn, seed=4, feat_dim=F), y)
    x = train.synthetic_node_data(n, F, 2, seed=3)[0]
    c = 17
    assert np.array_equal(y[:, c], x[:, c % F] + x[:, (3 * c + 1) % F] - x[:, (5 * c + 2) % F] > np.float32(0.5))


def test_command_line_multilabel(monkeypatch, tmp_path):
    from cslicer import l0, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(indptr, indices, feats, labels, n_classes, **kw):
        seen.update(kw, labels=labels(np.arange(4)), n_classes=n_classes)
        raise Stop()
    monkeypatch.setattr(train, "Trainer", fake)
    tiny = _tiny()
    monkeypatch.setattr(l0, "synth_graph", lambda n, d, seed=0: tiny[:2])
    base = ["--graph", "synthetic", "--num-layers", "2", "--fan-out", "2,2"]
    with pytest.raises(Stop):
        train.main(base)
    assert "multilabel" not in seen and seen["labels"].shape == (4,)
    seen.clear()
    with pytest.raises(Stop):
        train.main(base + ["--multilabel"])
    assert seen["multilabel"] is True and seen["labels"].shape == (4, 40) and seen["labels"].dtype == np.bool_
    assert np.array_equal(seen["labels"], train.synthetic_multilabels(200_000, 40, seed=0, rows=np.arange(4), feat_dim=128))
    # an L0 directory: the flag and the directory's format must agree; a multi-label one hands over its unpacked rows
    indptr, indices = _l0_graph(11)
    y = np.random.default_rng(2).random((11, 37)) < 0.5
    single, multi = str(tmp_path / "s"), str(tmp_path / "m")
    l0.write_l0(single, indptr, indices, labels=np.arange(11) % 3, num_classes=3)
    l0.write_l0(multi, indptr, indices, labels=y, num_classes=37)
    with pytest.raises(SystemExit, match="multilabel=1"):
        train.main(["--graph", single, "--multilabel"])
    with pytest.raises(SystemExit, match="--multilabel"):
        train.main(["--graph", multi])
    seen.clear()
    with pytest.raises(Stop):
        train.main(["--graph", multi, "--multilabel", "--num-layers", "2", "--fan-out", "2,2"])
    assert seen["multilabel"] is True and seen["n_classes"] == 37 and np.array_equal(seen["labels"], y[:4])
    assert "--multilabel (extra): `Trainer(multilabel=True)`" in train.main.__doc__
