"""Class weights and label smoothing of the single-label loss, the part that needs no GPU: the float64 restatement
(tests/loss_ref.py) against torch, train.balanced_class_weight, the constructor's refusals before any device call, the
command line, cslicer.train.step_plan (unchanged), the header against what the binder bound and the host-side refusals of
the C entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import loss_ref
import tail_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional


# ---- the restatement ---------------------------------------------------------------------------------------------------

def _case(C_, n=9, seed=0):
    rng = np.random.default_rng(1000 * C_ + seed)
    z = (rng.standard_normal((n, C_)) * 3).astype(np.float32)
    node = rng.permutation(50)[:n].astype(np.int32)
    labels = rng.integers(0, C_, size=50).astype(np.int64)
    w = (rng.random(C_) * 4).astype(np.float32)
    return z, node, labels, w


@pytest.mark.parametrize("C_", [1, 2, 47, 257])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_weighted_ce_is_torchs(C_, weighted, eps):
    z, node, labels, w = _case(C_)
    w = w if weighted else None
    n, scale = z.shape[0], 1.0 / 7
    loss_rows, g, colsum, Q, terms = loss_ref.weighted_ce(z, C_, n, n + 3, C_, node, None, labels, w, eps, scale)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    y = torch.as_tensor(labels[node])
    e32, s32 = float(np.float32(eps)), float(np.float32(scale))
    want = s32 * F.cross_entropy(zt, y, weight=None if w is None else torch.tensor(w, dtype=torch.float64),
                                 label_smoothing=e32, reduction="sum")
    want.backward()
    got = float(loss_rows.sum())
    assert abs(got - float(want.detach())) <= 1e-12 * max(abs(float(want.detach())), 1.0)
    assert g.shape == (n + 3, C_) and float(g[n:].abs().max()) == 0.0
    assert float((g[:n] - zt.grad).abs().max()) <= 1e-12 * max(float(zt.grad.abs().max()), 1.0)
    assert torch.allclose(colsum, g.sum(0))
    # Q = sum_c q_c; every term of the loss is >= 0, so the |terms| add up to the unscaled loss
    q = loss_ref.target(y, C_, w, eps)
    assert torch.allclose(Q, q.sum(1), rtol=1e-14, atol=0) and float((terms * s32 - loss_rows).abs().max()) <= 1e-15


def test_defaults_are_the_plain_loss_entry_for_entry():
    for C_ in (1, 3, 47):
        z, node, labels, _ = _case(C_, seed=1)
        n = z.shape[0]
        rowmap = np.random.default_rng(2).permutation(50).astype(np.int32)
        wide = np.zeros((n, C_ + 5), dtype=np.float32)
        wide[:, :C_] = z
        a = loss_ref.weighted_ce(wide, C_ + 5, n, n + 2, C_, node, rowmap, labels, None, 0.0, 0.25)
        b = tail_ref.softmax_ce(wide, C_ + 5, n, n + 2, C_, node, rowmap, labels, 0.25)
        for x, y in zip(a[:3], b):
            assert torch.allclose(x, y, rtol=1e-14, atol=1e-16)
        assert torch.equal(a[3], torch.ones(n, dtype=torch.float64))


def test_a_bad_label_is_nan_in_its_row_only():
    z, node, labels, w = _case(5)
    n = z.shape[0]
    labels = labels.copy()
    labels[node[2]], labels[node[6]] = -1, 5
    buf = torch.full((n * 8,), 7.0, dtype=torch.float64)
    loss_rows, g, colsum, _, _ = loss_ref.weighted_ce(z, 5, n, n, 5, node, None, labels, w, 0.1, 1.0, grad=buf, ldgr=8)
    bad = np.zeros(n, dtype=bool)
    bad[[2, 6]] = True
    assert torch.isnan(loss_rows[bad]).all() and torch.isfinite(loss_rows[~bad]).all()
    assert torch.isnan(g[bad]).all() and torch.isfinite(g[~bad]).all() and torch.isnan(colsum).all()
    v = buf.reshape(n, 8)
    assert torch.equal(v[:, 5:], torch.full((n, 3), 7.0, dtype=torch.float64)) and torch.isnan(v[bad, :5]).all()


def test_a_masked_class_has_neither_loss_nor_gradient():
    z, node, labels, w = _case(6)
    w = w.copy()
    w[labels[node[0]]] = 0.0
    loss_rows, g, _, Q, _ = loss_ref.weighted_ce(z, 6, 9, 9, 6, node, None, labels, w, 0.0, 1.0)
    hit = torch.as_tensor(labels[node] == labels[node[0]])
    assert float(loss_rows[hit].abs().max()) == 0.0 and float(g[hit].abs().max()) == 0.0 and float(Q[hit].abs().max()) == 0.0


def test_model_backward_is_autograd_of_the_same_model():
    """loss_ref.model_on_layers (hand-written backward, with and without dropout masks) against torch float64 autograd
    with torch's own weighted, smoothed cross-entropy"""
    import dropout_ref
    import sage_ref
    rng = np.random.default_rng(11)
    for L, drop in ((1, None), (2, None), (3, (0.5, 9, 2))):
        sizes = [40, 25, 12, 6][:L + 1]
        layers, dims = [], [8] + [12] * (L - 1) + [5]
        for k in range(L):
            n_src, n = sizes[k], sizes[k + 1]
            indptr = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(rng.integers(0, 5, size=n), out=indptr[1:])
            layers.append({"indptr": indptr, "indices": rng.integers(0, n_src, size=int(indptr[-1])),
                           "self_ids": rng.permutation(n_src)[:n], "n_src": n_src, "out_nodes": rng.permutation(10 ** 6)[:n]})
        ws = [rng.standard_normal((dims[k + 1], 2 * dims[k])) * 0.3 for k in range(L)]
        bs = [rng.standard_normal(dims[k + 1]) * 0.3 for k in range(L)]
        x0, labels = rng.standard_normal((sizes[0], dims[0])), rng.integers(0, 5, size=sizes[L])
        w = rng.random(5).astype(np.float32)
        loss, grads = loss_ref.model_on_layers(layers, x0, labels, ws, bs, 0.25, w, 0.125, drop)
        wt = [torch.tensor(x, requires_grad=True) for x in ws]
        bt = [torch.tensor(b, requires_grad=True) for b in bs]
        h = torch.tensor(x0)
        for k, ly in enumerate(layers):
            sid, idx = torch.as_tensor(ly["self_ids"]), torch.as_tensor(ly["indices"])
            rows = sage_ref.csr_rows(ly["indptr"])
            agg = torch.zeros((sid.numel(), h.shape[1]), dtype=torch.float64).index_add(0, rows, h[idx])
            deg = torch.bincount(rows, minlength=sid.numel()).double().clamp(min=1)
            h = torch.cat([h[sid], agg / deg[:, None]], 1) @ wt[k].t() + bt[k]
            if k + 1 < L:
                h = torch.relu(h)
                if drop:
                    h = h * torch.from_numpy(dropout_ref.keep_mask(ly["out_nodes"], h.shape[1], drop[0], drop[1], k, drop[2])) * 2.0
        want = 0.25 * F.cross_entropy(h, torch.as_tensor(labels), weight=torch.tensor(w, dtype=torch.float64),
                                      label_smoothing=0.125, reduction="sum")
        want.backward()
        assert abs(loss - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        for k in range(L):
            assert torch.allclose(grads[2 * k], wt[k].grad, rtol=1e-10, atol=1e-13)
            assert torch.allclose(grads[2 * k + 1], bt[k].grad, rtol=1e-10, atol=1e-13)


def test_balanced_class_weight():
    from cslicer import train
    labels = np.array([0, 0, 0, 2, 2, 4, 0, 2, 0, 0])       # 6 of class 0, 3 of class 2, 1 of class 4; 1 and 3 absent
    w = train.balanced_class_weight(labels, 5)
    assert w.dtype == np.float32 and w.shape == (5,)
    assert np.array_equal(w, np.array([10 / 30.0, 0.0, 10 / 15.0, 0.0, 10 / 5.0], dtype=np.float64).astype(np.float32))
    assert np.array_equal(train.balanced_class_weight(np.zeros(0, dtype=np.int64), 3), np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError):
        train.balanced_class_weight([0, 5], 5)


# ---- the constructor and the command line --------------------------------------------------------------------------------

def _tiny():
    indptr = np.arange(9, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, 8, size=16).astype(np.int64)
    return indptr, indices, np.zeros((8, 8), dtype=np.float32), np.zeros(8, dtype=np.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(label_smoothing=1.0), r"label_smoothing must be in \[0, 1\)"),
    (dict(label_smoothing=-0.1), r"label_smoothing must be in \[0, 1\)"),
    (dict(label_smoothing=float("nan")), r"label_smoothing must be in \[0, 1\)"),
    (dict(class_weight=[1.0, 2.0]), "n_classes = 3"), (dict(class_weight=[[1.0, 2.0, 3.0]]), "n_classes = 3"),
    (dict(class_weight=[1.0, -2.0, 1.0]), "finite numbers >= 0"), (dict(class_weight=[1.0, float("nan"), 1.0]), "finite numbers >= 0"),
    (dict(class_weight=[1.0, float("inf"), 1.0]), "finite numbers >= 0"), (dict(class_weight=[0.0, 0.0, 0.0]), "at least one > 0"),
    (dict(label_smoothing=0.1, multilabel=True), "sigmoid-BCE loss has no weights yet"),
    (dict(class_weight=[1.0, 1.0, 1.0], multilabel=True), "sigmoid-BCE loss has no weights yet"),
])
def test_constructor_refuses_before_any_device_call(kw, match, monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats, labels = _tiny()
    if kw.get("multilabel"):
        labels = np.zeros((8, 3), dtype=np.int64)
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, **kw)


def _main_kw(monkeypatch, argv):
    from cslicer import l0, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train, "Trainer", fake)
    monkeypatch.setattr(l0, "synth_graph", lambda n, d, seed=0: _tiny()[:2])
    with pytest.raises(Stop):
        train.main(["--graph", "synthetic", "--num-layers", "2", "--fan-out", "2,2"] + argv)
    return seen


def test_command_line(monkeypatch, tmp_path):
    from cslicer import train
    seen = _main_kw(monkeypatch, [])
    assert "label_smoothing" not in seen and "class_weight" not in seen
    seen = _main_kw(monkeypatch, ["--label-smoothing", "0.1"])
    assert seen["label_smoothing"] == 0.1 and "class_weight" not in seen
    # `balanced`: over the labels of the training nodes -- every node of the tiny graph, or the 80 % of the holdout split
    lab = lambda ids: train.synthetic_node_data(200_000, 1, 40, seed=0, rows=ids)[1]      # noqa: E731 (what main() trains on)
    seen = _main_kw(monkeypatch, ["--class-weight", "balanced"])
    assert "label_smoothing" not in seen
    assert np.array_equal(seen["class_weight"], train.balanced_class_weight(lab(np.arange(8)), 40))
    assert seen["class_weight"].shape == (40,) and (seen["class_weight"] > 0).sum() == len(set(lab(np.arange(8)).tolist()))
    seen = _main_kw(monkeypatch, ["--class-weight", "balanced", "--eval-split", "holdout"])
    held = np.sort(np.random.default_rng(0).permutation(8)[:6])
    assert np.array_equal(seen["class_weight"], train.balanced_class_weight(lab(held), 40))
    path = tmp_path / "w.txt"
    path.write_text("\n".join("%g" % (0.5 + c) for c in range(40)) + "\n")
    seen = _main_kw(monkeypatch, ["--class-weight", str(path), "--label-smoothing", "0.25"])
    assert np.array_equal(seen["class_weight"], 0.5 + np.arange(40)) and seen["label_smoothing"] == 0.25
    for argv in (["--label-smoothing", "0.1"], ["--class-weight", "balanced"]):
        with pytest.raises(SystemExit) as ex:
            train.main(["--graph", "synthetic", "--multilabel"] + argv)
        assert "--label-smoothing" in str(ex.value) and "--class-weight" in str(ex.value)
    assert "--label-smoothing EPS" in train.main.__doc__ and "--class-weight balanced|FILE" in train.main.__doc__


def test_step_plan_does_not_see_the_options():
    """every tabulated row is today's, and step_plan has no parameter of the loss options: they cannot choose the path"""
    import inspect

    import test_step_plan_cpu as T
    from cslicer.train import Switches, step_plan
    for row, change, flags, path, gat_input, input_form in T.ROWS:
        cfg = dict(T.BASE, **change)
        sw = Switches(**{k: cfg.pop(k) for k in Switches._fields})
        assert tuple(step_plan(sw=sw, **cfg)) == (flags, path, gat_input, input_form), row
    assert list(inspect.signature(step_plan).parameters) == [
        "kind", "world", "rank_path", "n_layers", "F", "hidden", "n_classes", "heads", "fanout", "table_f32", "gat_input",
        "replace", "sw", "width_known", "dropout", "multilabel"]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------

NAMES = ["csl_softmax_ce_w_f32", "csl_softmax_ce_w_partial_f32", "csl_sage_fwd_bwd_ce", "csl_sage_rank_fwd_bwd_ce"]


def test_header_names_are_what_the_binder_bound():
    from cslicer import _abi, aggr
    L = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_loss.h")).read(), flags=re.S)
    assert re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src) == NAMES
    assert "cslicer_loss.h" in _abi.HEADERS and _abi.BOUND["cslicer_loss.h"] == NAMES == aggr.LOSS_SYMBOLS
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    assert list(L.csl_softmax_ce_w_f32.argtypes) == [vp, i64, i64, i32, vp, vp, vp, vp, f32, f32, vp, vp, i64, vp, vp]
    assert list(L.csl_softmax_ce_w_partial_f32.argtypes) == [vp, i64, i64, i64, i32, vp, vp, vp, vp, f32, f32, vp, i64, vp, vp, vp]
    assert list(L.csl_sage_fwd_bwd_ce.argtypes) == [i32, vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, f32, f32, i64, i32, vp, vp,
                                                    vp, i64, vp, f32, i64, i64, vp]
    assert list(L.csl_sage_rank_fwd_bwd_ce.argtypes) == [i32, vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, f32, f32, i64, i32,
                                                         _abi.EXCHANGE_FN, _abi.EXCHANGE_WAIT_FN, vp, vp, vp, vp, i64, vp]
    for n in NAMES:
        assert getattr(L, n).restype is C.c_int


def test_the_entry_points_refuse_before_any_hip_call():
    """no GPU here: every one of these returns CSL_E_INVALID (-1) from the host-side checks"""
    from cslicer import _abi, aggr
    L = _abi.load()
    buf = np.zeros(64, dtype=np.float32)
    x, nul, st = C.c_void_p(buf.ctypes.data), C.c_void_p(0), C.c_void_p(0)      # a host address: never dereferenced
    one = dict(logits=x, ldl=8, n=4, C=8, ids=x, rowmap=nul, labels=x, cw=nul, eps=0.1, scale=1.0, loss=x, grad=x, ldgr=8,
               scratch=x, stream=st)
    part = dict(logits=x, ldl=8, n=4, n_pad=4, C=8, ids=x, rowmap=nul, labels=x, cw=nul, eps=0.1, scale=1.0, grad=x, ldgr=8,
                loss_partial=x, col_partial=nul, stream=st)
    common = (dict(eps=1.0), dict(eps=-0.1), dict(eps=1.5), dict(eps=float("nan")), dict(n=-1), dict(C=0), dict(C=4097),
              dict(logits=nul), dict(ids=nul), dict(labels=nul), dict(grad=nul), dict(ldl=7), dict(ldgr=7))
    for bad in common + (dict(loss=nul), dict(scratch=nul)):
        assert L.csl_softmax_ce_w_f32(*dict(one, **bad).values()) == -1, bad
    for bad in common + (dict(n_pad=3), dict(loss_partial=nul), dict(C=257, ldl=300, ldgr=300, col_partial=x)):
        assert L.csl_softmax_ce_w_partial_f32(*dict(part, **bad).values()) == -1, bad
    assert L.csl_softmax_ce_w_partial_f32(*dict(part, n=0, n_pad=0, logits=nul, grad=nul, loss_partial=nul).values()) == 0
    # the steps: the loss options are checked before the layout is looked at, and the sentence names the argument
    dims = (C.c_int32 * 3)(8, 8, 4)
    sl, rsl = (aggr.SageSlice * 2)(), (aggr.SageRankSlice * 2)()
    step = lambda eps, labels=x, p=0.0, out_ids=nul: L.csl_sage_fwd_bwd_ce(                     # noqa: E731
        2, dims, sl, nul, nul, nul, 0, 8, nul, nul, labels, nul, eps, 1.0, 0, 1, nul, nul, nul, 0, out_ids, p, 1, 0, st)
    rank = lambda eps, labels=x: L.csl_sage_rank_fwd_bwd_ce(                                    # noqa: E731
        2, dims, rsl, nul, nul, nul, 0, 8, nul, nul, nul, labels, nul, eps, 1.0, 0, 1, _abi.EXCHANGE_FN(0),
        _abi.EXCHANGE_WAIT_FN(0), nul, nul, nul, nul, 0, st)
    for f in (step, rank):
        for eps in (1.0, -0.5, float("nan")):
            assert f(eps) == -1 and b"label_smoothing" in L.csl_sage_last_error()
        assert f(0.1, nul) == -1 and b"labels" in L.csl_sage_last_error()
        assert f(0.1) == -1 and b"bad argument" in L.csl_sage_last_error()       # (null weights: sage_step's own check)
    assert step(0.1, p=0.5) == -1 and b"dropout" in L.csl_sage_last_error()       # p without out-node ids
    assert step(0.1, p=1.0, out_ids=x) == -1 and b"dropout" in L.csl_sage_last_error()
    dims[2] = 5000
    assert step(0.1) == -1 and b"classes" in L.csl_sage_last_error()
