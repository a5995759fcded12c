"""Correct and Smooth without a GPU: the float64 restatement of tests/smooth_ref.py against the dense
formulation, the rules of the correct step, the bound header and the host-side refusals of csl_prop_f32, both command
lines and the trainer's refusals, and the planted-partition conditions that tests/test_gpu_smooth.py relies on."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import smooth_ref as R


def _messy_graph(n, seed):
    """a raw CSR with isolated nodes, duplicate edges and self loops; not symmetric"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, n)
    lens[rng.integers(0, n, n // 8)] = 0                     # isolated rows
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    ix = rng.integers(0, n, int(ip[-1]))
    rows = np.repeat(np.arange(n), lens)
    ix[::7] = rows[::7]                                      # self loops
    ix[1::5] = ix[0:-1:5][:ix[1::5].shape[0]]                # duplicates (where the neighbour sits in the same row)
    return ip, ix


def _dense_prop(ip, ix, x0, alpha, T, lo, hi, fix=None):
    n = ip.shape[0] - 1
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(ip)), ix), 1.0)
    dv = R.dinv32(ip).astype(np.float64)
    S = dv[:, None] * A * dv[None, :]
    x = x0.astype(np.float64).copy()
    for _ in range(T):
        x = alpha * (S @ x) + ((1.0 - alpha) * x0 if alpha != 1.0 else 0.0)
        x = np.clip(x, lo, hi)
        if fix is not None:
            x[fix[0]] = fix[1]
    return x


@pytest.mark.parametrize("n,seed", [(1, 0), (37, 1), (200, 2)])
def test_prop_is_the_dense_iteration(n, seed):
    raw_ip, raw_ix = _messy_graph(n, seed)
    ip, ix = R.neighbour_csr(raw_ip, raw_ix)
    rows = np.repeat(np.arange(n), np.diff(ip))
    assert not (ix == rows).any() and (n == 1 or (np.diff(ip) == 0).any())
    if n == 200:
        assert ip[-1] < raw_ip[-1] and any(np.unique(ix[ip[v]:ip[v + 1]]).shape[0] < ip[v + 1] - ip[v] for v in range(n))
    dv = R.dinv32(ip)
    assert dv.dtype == np.float32 and (dv[np.diff(ip) == 0] == 0).all()
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((n, 5))
    fix = (np.arange(0, n, 3), rng.standard_normal((np.arange(0, n, 3).shape[0], 5)))
    for alpha, lo, hi, fx in ((0.8, -1.0, 1.0, None), (0.5, 0.0, 1.0, None), (1.0, -np.inf, np.inf, fix), (0.8, -np.inf, np.inf, fix),
                              (1.0, -0.25, 0.25, None)):
        got = R.prop(ip, ix, x0, alpha, 6, lo, hi, fix=fx)
        want = _dense_prop(ip, ix, x0, alpha, 6, lo, hi, fx)
        assert np.abs(got - want).max() <= 1e-12, (alpha, lo, hi)
        if fx is not None:
            assert np.array_equal(got[fx[0]], fx[1])         # the fixed-scale reset: the rows are what they were set to
    assert np.array_equal(R.prop(ip, ix, x0, 0.8, 0, 0.0, 1.0), x0)          # steps == 0
    got, B = R.prop(ip, ix, x0, 0.8, 3, -1.0, 1.0, bounds=True)
    assert len(B) == 4 and all(b.shape == x0.shape and (b > 0).all() for b in B[1:])


def test_the_autoscale_rule_has_three_branches():
    e = np.array([[0.0, 0.0], [1e-5, -1e-5], [0.25, -0.25]])
    s, raw = R.autoscale_factors(0.1, e)
    assert np.isinf(raw[0]) and raw[1] == pytest.approx(5000.0) and raw[2] == pytest.approx(0.2)
    assert s.tolist() == [1.0, 1.0, pytest.approx(0.2)]
    assert R.autoscale_factors(0.0, e[:1])[0].tolist() == [1.0]             # 0 / 0: not finite either
    # through the whole step: node 3 is isolated and unlabelled, its error row stays zero, its factor is 1, its row P
    ip, ix = np.array([0, 1, 3, 4, 4]), np.array([1, 0, 2, 1])
    logits = np.array([[2.0, 0.0], [0.0, 1.0], [0.5, 0.0], [0.0, 3.0]])
    r = R.correct_and_smooth(logits, ip, ix, [0], [1], T1=4, T2=0, autoscale=True)
    assert np.isinf(r["raw_scale"][3]) and np.allclose(r["out"][3], R.softmax(logits)[3])
    assert r["out"][0].tolist() == [0.0, 1.0]                                 # T2 == 0: the training row is its label
    assert not np.allclose(r["out"][1], R.softmax(logits)[1])                 # the neighbour was corrected


def test_fixed_scale_and_zero_steps():
    ip, ix = np.array([0, 1, 3, 4, 4]), np.array([1, 0, 2, 1])
    logits = np.array([[2.0, 0.0], [0.0, 1.0], [0.5, 0.0], [0.0, 3.0]])
    P = R.softmax(logits)
    r = R.correct_and_smooth(logits, ip, ix, [0, 2], [1, 0], T1=0, T2=0, autoscale=False, scale=2.0)
    want = P.copy()
    want[[0, 2]] = [[0.0, 1.0], [1.0, 0.0]]                 # T1 == 0: E = E0, zero off the training rows; then the labels
    assert np.allclose(r["out"], want) and r["raw_scale"] is None
    # one fixed-scale step by hand: E1 = S E0 with the training rows put back, P' = P + 2 E1
    dv = R.dinv32(ip).astype(np.float64)
    E0 = np.zeros_like(P)
    E0[0], E0[2] = [0.0, 1.0] - P[0], [1.0, 0.0] - P[2]
    E1 = np.zeros_like(P)
    E1[1] = dv[1] * (dv[0] * E0[0] + dv[2] * E0[2])
    E1[0], E1[2] = E0[0], E0[2]
    r = R.correct_and_smooth(logits, ip, ix, [0, 2], [1, 0], T1=1, a1=1.0, T2=0, autoscale=False, scale=2.0)
    assert np.allclose(r["out"][[1, 3]], (P + 2.0 * E1)[[1, 3]])
    lp = R.label_propagation(ip, ix, 2, [0, 2], [1, 0], alpha=1.0, T=1)
    assert np.allclose(lp[1], dv[1] * np.array([dv[2], dv[0]])) and not lp[3].any()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def test_the_header_is_bound_and_the_module_imports():
    from cslicer import _abi, smooth
    L = _abi.load()
    assert "cslicer_smooth.h" in _abi.HEADERS and _abi.BOUND["cslicer_smooth.h"] == ["csl_prop_f32"] == smooth.SYMBOLS
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert list(L.csl_prop_f32.argtypes) == [vp, vp, vp, i64, vp, i64, i64, i64, vp, i64, i32, vp, f32, vp, i64, f32, f32, f32,
                                             vp, vp, i64, vp, i64, vp]
    assert L.csl_prop_f32.restype is C.c_int
    for name in ("dinv_of", "propagate", "correct_and_smooth", "label_propagation", "need_bytes"):
        assert callable(getattr(smooth, name))
    w = 48
    assert smooth.need_bytes(1000, 47) == 4 * (4 * 1000 * w + 2000) and smooth.need_bytes(10, 4, 3, 2, False) == 4 * (200 + 20 + 8 + 36)


def test_csl_prop_refuses_before_any_hip_call():
    """no GPU here: every one of these answers CSL_E_INVALID (-1) from the host-side checks and touches no buffer"""
    from cslicer import _abi
    L = _abi.load()
    buf = np.full(512 + 8, -7777.0, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16          # 16-byte aligned host addresses: never dereferenced
    x, x2, x3, odd, nul = C.c_void_p(base), C.c_void_p(base + 256), C.c_void_p(base + 512), C.c_void_p(base + 4), C.c_void_p(0)
    nan, inf = float("nan"), float("inf")
    ok = dict(indptr=x, indices=x, items=x, n_items=1, hubs=x, n_hubs=1, pos0=0, part0=0, xs=x, ldx=8, W=8, dinv=x, alpha=0.8,
              base=x2, ldb=8, beta=0.2, lo=-1.0, hi=1.0, partial=x2, out=x2, ldo=8, out_s=x3, ldos=8, st=nul)

    def prop(**kw):
        return L.csl_prop_f32(*dict(ok, **kw).values())
    bad = [dict(W=0), dict(W=-4), dict(W=6), dict(ldx=4), dict(ldx=10), dict(ldb=4), dict(ldb=9), dict(ldo=6), dict(ldo=4),
           dict(ldos=4), dict(ldos=11), dict(xs=odd), dict(base=odd), dict(out=odd), dict(out_s=odd), dict(partial=odd),
           dict(items=odd), dict(hubs=odd), dict(dinv=nul), dict(xs=nul), dict(out=nul, out_s=nul), dict(out_s=x), dict(out=x),
           dict(lo=1.0, hi=-1.0), dict(lo=nan), dict(hi=nan), dict(alpha=nan), dict(alpha=inf), dict(beta=nan), dict(beta=-inf),
           dict(n_items=-1), dict(n_hubs=-1), dict(pos0=-1), dict(part0=-1), dict(indptr=nul), dict(indices=nul), dict(items=nul),
           dict(hubs=nul), dict(partial=nul)]
    for kw in bad:
        assert prop(**kw) == -1, kw
    # nothing to do: CSL_OK without a launch, whatever the pointers; a bad shape is still refused
    none = dict(n_items=0, n_hubs=0)
    assert prop(**none) == 0
    assert prop(indptr=nul, indices=nul, items=nul, hubs=nul, xs=nul, dinv=nul, base=nul, partial=nul, out=nul, out_s=nul, **none) == 0
    assert prop(W=6, **none) == -1 and prop(lo=nan, **none) == -1 and prop(ldx=4, **none) == -1
    assert (buf == -7777.0).all()


# ---- the Python interface ------------------------------------------------------------------------------------------------

def _no_device(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)


def test_python_refusals_come_before_any_device_work(monkeypatch):
    from cslicer import smooth
    _no_device(monkeypatch)
    ip, ix = np.array([0, 1, 2, 3]), np.array([1, 2, 0])
    logits = np.zeros((3, 4), dtype=np.float32)

    def cs(train=(0, 1), labels=(1, 3), **kw):
        return smooth.correct_and_smooth(logits, ip, ix, np.array(train), np.array(labels), **kw)
    for kw, match in ((dict(train=(0, 0)), "duplicate training nodes"), (dict(labels=(1, 4)), r"label outside \[0, 4\)"),
                      (dict(labels=(-1, 0)), "label outside"), (dict(train=(0, 3)), "training node outside"),
                      (dict(labels=(1,)), "2 training nodes, 1 labels"), (dict(correction_alpha=0.0), "alpha must be in"),
                      (dict(smoothing_alpha=1.5), "alpha must be in"), (dict(correction_alpha=float("nan")), "alpha must be in"),
                      (dict(num_correction_layers=-1), "must be >= 0"), (dict(num_smoothing_layers=-2), "must be >= 0"),
                      (dict(autoscale=False, scale=float("inf")), "scale must be finite")):
        with pytest.raises(ValueError, match=match):
            cs(**kw)
    for kw, match in ((dict(train_nodes=[1, 1], train_labels=[0, 0]), "duplicate"), (dict(train_nodes=[1], train_labels=[2]), "label"),
                      (dict(train_nodes=[1], train_labels=[0], alpha=0.0), "alpha"),
                      (dict(train_nodes=[1], train_labels=[0], num_layers=-1), ">= 0")):
        with pytest.raises(ValueError, match=match):
            smooth.label_propagation(ip, ix, 2, **kw)
    with pytest.raises(ValueError, match="alpha"):
        smooth.propagate(None, None, 1.01, 3, 0.0, 1.0)


def test_trainer_refuses_multilabel_and_the_rank_path(monkeypatch):
    from cslicer import train
    _no_device(monkeypatch)
    t = object.__new__(train.Trainer)
    t.predict = lambda *a, **kw: pytest.fail("device work before the refusal")
    t.multilabel, t.rank_path, t.N, t.n_own = True, False, 8, 8
    with pytest.raises(ValueError, match="multi-label"):
        t.correct_and_smooth([0], [1])
    t.multilabel, t.rank_path = False, True
    with pytest.raises(ValueError, match="rank path"):
        t.correct_and_smooth([0], [1])
    t.rank_path, t.n_own = False, 4
    with pytest.raises(ValueError, match="single process"):
        t.correct_and_smooth([0], [1])
    t.n_own = 8
    with pytest.raises(ValueError, match=r"nodes outside \[0, 8\)"):
        t.correct_and_smooth([8], [1])
    assert "correct_and_smooth" in train.Trainer.correct_and_smooth.__doc__


# ---- the command lines -------------------------------------------------------------------------------------------------------

def test_train_command_line(monkeypatch):
    from cslicer import l0, smooth, train

    def boom(*a, **kw):
        raise AssertionError("the graph was loaded before the refusal")
    _no_device(monkeypatch)
    monkeypatch.setattr(l0, "synth_graph", boom)
    monkeypatch.setattr(l0, "read_l0", boom)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = train._parser().parse_args([])
    assert a.correct_smooth is False and a.cs_layers is None and a.cs_alpha is None and a.cs_scale is None
    assert smooth.options_of(a) is None
    a = train._parser().parse_args(["--correct-smooth", "--cs-layers", "20,30", "--cs-alpha", "0.9,0.7", "--cs-scale", "1.5"])
    assert smooth.options_of(a) == {"num_correction_layers": 20, "num_smoothing_layers": 30, "correction_alpha": 0.9,
                                    "smoothing_alpha": 0.7, "autoscale": False, "scale": 1.5}
    assert smooth.options_of(train._parser().parse_args(["--correct-smooth", "--cs-scale", "auto"])) == {}
    with pytest.raises(SystemExit, match="needs --eval-split"):
        train.main(["--correct-smooth"])
    with pytest.raises(SystemExit, match="multi-label"):
        train.main(["--correct-smooth", "--eval-split", "holdout", "--multilabel"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single process"):
        train.main(["--correct-smooth", "--eval-split", "holdout"])
    monkeypatch.delenv("WORLD_SIZE")
    for argv, match in ((["--cs-layers", "5,5"], "--cs-layers belongs to --correct-smooth"),
                        (["--cs-scale", "2"], "--cs-scale belongs to --correct-smooth"),
                        (["--correct-smooth", "--cs-layers", "5"], "--cs-layers T1,T2"),
                        (["--correct-smooth", "--cs-alpha", "0.5,1.5"], "alpha must be in"),
                        (["--correct-smooth", "--cs-layers=-1,5"], "must be >= 0"),
                        (["--correct-smooth", "--cs-scale", "big"], "--cs-scale auto")):
        with pytest.raises(SystemExit, match=match):
            train.main(["--eval-split", "holdout"] + argv)
    assert "--correct-smooth [--cs-layers T1,T2] [--cs-alpha A1,A2] [--cs-scale auto|NUMBER] (extra)" in train.main.__doc__
    assert "Eval Acc C&S %.4f (plain %.4f) | %d nodes in %.2f s" in train.main.__doc__


def test_train_prints_the_line_after_eval_acc(monkeypatch, capsys):
    """the epoch loop alone, on a stand-in trainer: the new line follows every `Eval Acc` line and only with the option"""
    from cslicer import train
    calls = []

    class Stub(object):
        N, n_batches = 10, 1

        def set_nodes(self, nodes):
            pass

        def run(self, steps):
            return [1.0, 0.5]

        def evaluate(self, nodes):
            return {"accuracy": 0.5, "loss": 1.0, "n": len(nodes)}

        def correct_and_smooth(self, eval_nodes, train_nodes, **kw):
            calls.append((list(eval_nodes), list(train_nodes), kw))
            return {"accuracy": 0.75, "base_accuracy": 0.5, "n": len(eval_nodes)}
    tn, en = np.arange(6), np.arange(6, 10)
    a = train._parser().parse_args(["--num-epochs", "2", "--eval-every", "1", "--eval-split", "holdout"])
    train._train_epochs(a, Stub(), 0, tn, en, 0)
    plain = capsys.readouterr().out
    assert plain.count("Eval Acc 0.5000") == 2 and "C&S" not in plain and not calls
    a = train._parser().parse_args(["--num-epochs", "2", "--eval-every", "1", "--eval-split", "holdout", "--correct-smooth",
                                    "--cs-layers", "3,4"])
    train._train_epochs(a, Stub(), 0, tn, en, 0)
    lines = [ln for ln in capsys.readouterr().out.split("\n") if ln.startswith("Eval Acc")]
    assert len(lines) == 4 and [ln.startswith("Eval Acc C&S 0.7500 (plain 0.5000) | 4 nodes in ") for ln in lines] == [False, True] * 2
    assert calls == [(list(en), list(tn), {"num_correction_layers": 3, "num_smoothing_layers": 4})] * 2
    train._train_epochs(a, Stub(), 0, tn, en, 1)                       # another rank prints nothing
    assert "Eval Acc" not in capsys.readouterr().out


def test_predict_command_line(tmp_path, monkeypatch):
    from cslicer import checkpoint, l0, predict, splitgnn
    indptr, indices = l0.synth_graph(50, 4.0, seed=1)
    rng = np.random.default_rng(0)
    torch.manual_seed(3)
    single, multi = str(tmp_path / "m.ckpt"), str(tmp_path / "ml.ckpt")
    checkpoint.write(single, splitgnn.DistSAGEModel(16, 16, 5))
    checkpoint.write(multi, splitgnn.DistSAGEModel(16, 16, 5), multilabel=True)
    feats, labels = rng.random((50, 16), dtype=np.float32), rng.integers(0, 5, 50).astype(np.int32)
    bare, split, nolab = (str(tmp_path / d) for d in ("bare", "split", "nolab"))
    l0.write_l0(bare, indptr, indices, features=feats, labels=labels, num_classes=5)
    l0.write_l0(split, indptr, indices, features=feats, labels=labels, num_classes=5, train_idx=np.arange(30), val_idx=np.arange(30, 50))
    l0.write_l0(nolab, indptr, indices, features=feats, num_classes=5, train_idx=np.arange(30), val_idx=np.arange(30, 50))
    if os.path.exists(os.path.join(nolab, "labels.bin")):
        os.remove(os.path.join(nolab, "labels.bin"))
    _no_device(monkeypatch)
    for name in ("read_l0", "read_features"):
        monkeypatch.setattr(l0, name, lambda *a, **kw: pytest.fail("the graph was read before the refusal"))
    out = str(tmp_path / "p.npy")
    a = predict._parser().parse_args(["--model", single, "--graph", bare, "--out", out])
    assert a.correct_smooth is False and a.train_nodes is None and a.cs_layers is None
    assert "not logits" in predict._parser().format_help().replace("\n", " ")
    go = ["--model", single, "--out", out]
    with pytest.raises(SystemExit, match="--correct-smooth needs .*train_idx.bin"):
        predict.main(go + ["--graph", bare, "--correct-smooth"])
    with pytest.raises(SystemExit, match="--correct-smooth needs .*labels.bin"):
        predict.main(go + ["--graph", nolab, "--correct-smooth"])
    with pytest.raises(SystemExit, match="multi-label model"):
        predict.main(["--model", multi, "--out", out, "--graph", split, "--correct-smooth"])
    with pytest.raises(SystemExit, match="--train-nodes belongs to --correct-smooth"):
        predict.main(go + ["--graph", split, "--train-nodes", os.path.join(split, "train_idx.bin")])
    with pytest.raises(SystemExit, match="--cs-alpha belongs to --correct-smooth"):
        predict.main(go + ["--graph", split, "--cs-alpha", "0.5,0.5"])
    with pytest.raises(SystemExit, match="node ids outside"):
        np.array([0, 50], dtype=np.int64).tofile(str(tmp_path / "far.bin"))
        predict.main(go + ["--graph", split, "--correct-smooth", "--train-nodes", str(tmp_path / "far.bin")])
    assert not os.path.exists(out)
    # with everything there the refusals are passed: the next thing main() does is read the graph
    with pytest.raises(pytest.fail.Exception, match="the graph was read"):
        predict.main(go + ["--graph", split, "--correct-smooth", "--cs-scale", "2"])


# ---- the planted partition: what the GPU comparison relies on, on the reference alone -------------------------------------------

def test_planted_partition_on_the_reference():
    d = R.planted()
    assert d["n"] == 3000 and d["C"] == 7 and d["train"].shape[0] == 1500
    raw = (d["indptr"], d["indices"])
    ip, ix = R.neighbour_csr(*raw)
    assert ip[-1] < raw[0][-1]                                # self loops were in the raw graph
    # symmetric: every (u, v) as often as (v, u)
    rows = np.repeat(np.arange(d["n"]), np.diff(ip))
    assert np.array_equal(np.sort(rows * d["n"] + ix), np.sort(ix * d["n"] + rows))
    same = (d["cls"][rows] == d["cls"][ix]).mean() * ip[-1] / d["n"]
    assert 5.5 < same < 7.5 and 8.0 < ip[-1] / d["n"] < 10.0
    test, cls = d["test"], d["cls"]
    plain = float((d["logits"].argmax(1) == cls)[test].mean())
    assert 0.35 < plain < 0.55
    for auto, a1 in ((True, 0.8), (False, 0.8), (False, 1.0)):
        r = R.correct_and_smooth(d["logits"], ip, ix, d["train"], cls[d["train"]], 20, a1, 20, 0.8, auto, 1.0)
        acc = float((r["out"].argmax(1) == cls)[test].mean())
        small = float((R.margins(r["out"]) < 1e-4).mean())
        print("autoscale %s a1 %.1f: accuracy %.3f (plain %.3f), margins below 1e-4: %.4f" % (auto, a1, acc, plain, small))
        assert acc >= plain + 0.3
        assert small <= 0.01
        if auto:
            rs = r["raw_scale"]
            assert not ((rs >= 900.0) & (rs <= 1100.0)).any()
    lp = R.label_propagation(ip, ix, 7, d["train"], cls[d["train"]], 0.8, 20)
    assert float((lp.argmax(1) == cls)[test].mean()) >= plain + 0.3
