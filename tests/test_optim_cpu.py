"""Weight decay, gradient-norm clipping, the non-finite guard and the learning-rate schedule, the part that needs no GPU
(DESIGN 4.9): tests/optim_ref.py against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW / Adam in float64 (a wrong
restatement must not be able to hide a wrong kernel), cslicer.train.lr_schedule's values, the constructors' refusals, the
command line, and the refusals of csl_adamw_f32 that return before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import optim_ref as R

F64 = torch.float64
U = 2.0 ** -24
f = lambda x: float(np.float32(x))      # noqa: E731


# ---- the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("decoupled", [True, False])
def test_restatement_is_torch_clip_then_adamw_or_adam(decoupled):
    """20 steps on three tensors with their own decays (parameter groups; one of them 0), max_norm 2: the gradients' scale
    changes from step to step, so most steps clip and some (norm below 2, step 7 by construction) do not.  torch runs in
    float64 on the float32-rounded scalars, so the only differences left are the two roundings abi_rounding stands for."""
    rng = np.random.default_rng(4)
    lr, b1, b2, eps, max_norm = 3e-3, 0.9, 0.999, 1e-8, 2.0
    sizes, wds = [(5, 7), (11,), (3, 2)], [0.05, 0.0, 0.3]
    p0 = [rng.standard_normal(s) for s in sizes]
    tp = [torch.from_numpy(a.copy()).requires_grad_() for a in p0]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": [q], "weight_decay": f(w)} for q, w in zip(tp, wds)], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps))
    mine = [torch.from_numpy(a.copy()) for a in p0]
    ms, vs = [torch.zeros(s, dtype=F64) for s in sizes], [torch.zeros(s, dtype=F64) for s in sizes]
    clipped = unclipped = 0
    for step in range(1, 21):
        scale = 1e-2 if step == 7 else 10.0 ** rng.integers(-1, 3)
        gs = [torch.from_numpy(rng.standard_normal(s) * scale) for s in sizes]
        for q, g in zip(tp, gs):
            q.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(tp, f(max_norm))
        opt.step()
        n = R.grad_norm(gs)
        assert abs(n - float(total)) <= 1e-13 * n and not R.skipped(n, max_norm)
        c = R.clip_coef(n, max_norm, abi_rounding=False)
        c32 = R.clip_coef(n, max_norm)
        assert c32 == f(c) and (c == 1.0) == (n + 1e-6 <= f(max_norm))
        clipped, unclipped = clipped + (c < 1.0), unclipped + (c == 1.0)
        for j in range(3):
            st = R.adamw_step(mine[j], gs[j], ms[j], vs[j], c, wds[j], decoupled, lr, b1, b2, eps, step, abi_rounding=False)
            torch.testing.assert_close(st.p, tp[j].detach(), rtol=1e-12, atol=1e-12)
            assert st.g2_roundings == (c != 1.0) + 2 * (wds[j] > 0 and not decoupled)
            assert bool((st.g2_abs >= st.g2.abs()).all()) and bool((st.m_abs >= st.m.abs()).all())
            assert bool((st.v_abs >= st.v * (1 - 1e-15)).all())
            # the float32-rounded c and factor: the same step up to those two roundings
            r = R.adamw_step(mine[j], gs[j], ms[j], vs[j], c32, wds[j], decoupled, lr, b1, b2, eps, step)
            assert bool(((r.g2 - st.g2).abs() <= U * st.g2_abs).all())
            assert bool(((r.p_in - st.p_in).abs() <= U * st.p_in.abs()).all())
            mine[j], ms[j], vs[j] = st.p, st.m, st.v
            state = opt.state[tp[j]]
            torch.testing.assert_close(st.m, state["exp_avg"], rtol=1e-12, atol=1e-12)
            torch.testing.assert_close(st.v, state["exp_avg_sq"], rtol=1e-12, atol=0)
    assert clipped >= 10 and unclipped >= 1


def test_restatement_corners():
    g = [np.array([3.0, 4.0], dtype=np.float32), np.zeros(0, dtype=np.float32), np.array([12.0], dtype=np.float32)]
    assert R.grad_norm(g) == 13.0
    assert R.clip_coef(13.0, None) == 1.0 and R.clip_coef(13.0, 0.0) == 1.0 and R.clip_coef(13.0, float("inf")) == 1.0
    assert R.clip_coef(0.0, 1.0) == 1.0 and R.clip_coef(13.0, 1.0) == f(1.0 / (13.0 + 1e-6))
    assert R.grad_norm([np.array([1e20, 1e20], dtype=np.float32)]) == pytest.approx(math.sqrt(2) * 1e20, rel=1e-7)
    assert R.grad_norm([np.array([1e-30], dtype=np.float32)]) == pytest.approx(1e-30, rel=1e-7)
    bad = R.grad_norm([np.array([1.0, float("nan")], dtype=np.float32)])
    assert R.skipped(bad, 1.0) and R.skipped(float("inf"), float("inf")) and not R.skipped(bad, None)
    assert not R.skipped(3.0, 1.0)
    assert R.decay_factor(1e-2, 0.1) == f(1.0 - f(1e-2) * f(0.1))
    # no clipping, no decay: tail_ref.adam_step itself
    import tail_ref as T
    rng = np.random.default_rng(0)
    p, gr, m, v = rng.standard_normal((4, 9))
    v = v ** 2
    st = R.adamw_step(p, gr, m, v, 1.0, 0.0, True, 1e-3, 0.9, 0.999, 1e-8, 5)
    want = T.adam_step(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 5)
    assert torch.equal(st.p, want[0]) and torch.equal(st.m, want[1]) and torch.equal(st.v, want[2])
    assert st.g2_roundings == 0 and torch.equal(st.m_abs, want[4]) and torch.equal(st.v_abs, want[5])


# ---- the schedule --------------------------------------------------------------------------------------------------------

def test_lr_schedule_values():
    from cslicer import train
    s = train.lr_schedule("cosine", 0.01, warmup=10, total=110, min_lr=0.001)
    assert s(0) == pytest.approx(0.001) and s(9) == pytest.approx(0.01)          # first and last warm-up step
    assert s(10) == pytest.approx(0.01)                                          # the cosine starts at the base rate
    assert s(60) == pytest.approx(0.0055)                                        # its midpoint: (base + min) / 2
    assert s(109) == pytest.approx(0.001 + 0.009 * 0.5 * (1 + math.cos(math.pi * 99 / 100)))
    assert s(110) == 0.001 and s(111) == 0.001 and s(10 ** 9) == 0.001           # its end, and beyond total
    assert all(s(t + 1) < s(t) for t in range(10, 109))
    z = train.lr_schedule("cosine", 0.5, warmup=0, total=4)
    assert [z(t) for t in range(6)] == pytest.approx([0.5, 0.5 * 0.5 * (1 + math.cos(math.pi / 4)), 0.25,
                                                      0.5 * 0.5 * (1 + math.cos(3 * math.pi / 4)), 0.0, 0.0])
    k = train.lr_schedule("constant", 0.02, warmup=4)
    assert [k(t) for t in range(6)] == pytest.approx([0.005, 0.01, 0.015, 0.02, 0.02, 0.02]) and k(10 ** 6) == 0.02
    assert train.lr_schedule("constant", 0.02)(0) == 0.02
    for bad in (dict(kind="linear", base_lr=0.1), dict(kind="cosine", base_lr=0.1, warmup=5, total=5),
                dict(kind="constant", base_lr=0.1, warmup=-1), dict(kind="cosine", base_lr=0.1, total=9, min_lr=0.2),
                dict(kind="constant", base_lr=0.0)):
        with pytest.raises(ValueError):
            train.lr_schedule(**bad)


# ---- the constructors and the command line -----------------------------------------------------------------------------

def _tiny():
    indptr = np.arange(9, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, 8, size=16).astype(np.int64)
    return indptr, indices, np.zeros((8, 8), dtype=np.float32), np.zeros(8, dtype=np.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(weight_decay=-1e-3), "weight_decay must be >= 0"), (dict(weight_decay=float("nan")), "weight_decay must be >= 0"),
    (dict(max_grad_norm=0.0), "max_grad_norm must be None or > 0"), (dict(max_grad_norm=-1.0), "max_grad_norm must be"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm must be"), (dict(lr_schedule=0.01), "lr_schedule must be None or a callable"),
])
def test_trainer_refuses_before_any_device_call(kw, match, monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats, labels = _tiny()
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(weight_decay=[0.1]), "one per parameter tensor"), (dict(weight_decay=[0.1, 0.1, 0.1]), "one per parameter tensor"),
    (dict(weight_decay=-0.1), "weight_decay must be >= 0"), (dict(weight_decay=[0.0, float("nan")]), "weight_decay must be"),
    (dict(max_grad_norm=0), "max_grad_norm must be"), (dict(max_grad_norm=-2.0), "max_grad_norm must be"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm must be"),
])
def test_adam_refuses_before_it_looks_at_the_tensors(kw, match):
    """the new arguments are checked first: host tensors (a TypeError) are never reached"""
    from cslicer import aggr
    params = [torch.zeros(3), torch.zeros(2, 2)]
    with pytest.raises(ValueError, match=match):
        aggr.Adam(params, **kw)
    with pytest.raises(TypeError):                      # legal values: the next check is the old one
        aggr.Adam(params, weight_decay=[0.0, 0.1], max_grad_norm=float("inf"))


def test_command_line_reaches_the_constructor(monkeypatch):
    from cslicer import l0, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train, "Trainer", fake)
    monkeypatch.setattr(l0, "synth_graph", lambda n, d, seed=0: _tiny()[:2])
    new = ("weight_decay", "decoupled_weight_decay", "decay_bias", "max_grad_norm", "lr_schedule")
    base = ["--graph", "synthetic", "--num-layers", "2", "--fan-out", "2,2", "--batch-size", "2", "--num-epochs", "3"]

    def run(argv):
        seen.clear()
        with pytest.raises(Stop):
            train.main(base + argv)
        return {k: seen[k] for k in new if k in seen}
    assert run([]) == {}                                             # no option, no new keyword
    assert run(["--dropout", "0.5"]) == {}
    assert run(["--weight-decay", "5e-4"]) == {"weight_decay": 5e-4}
    assert run(["--weight-decay", "0.1", "--adam-l2", "--decay-bias"]) == {
        "weight_decay": 0.1, "decoupled_weight_decay": False, "decay_bias": True}
    assert run(["--clip-grad-norm", "inf"]) == {"max_grad_norm": float("inf")}
    assert run(["--clip-grad-norm", "1.5"]) == {"max_grad_norm": 1.5}
    # 8 nodes in minibatches of 2: 4 steps per epoch, 3 epochs: total = 12
    got = run(["--lr", "0.02", "--lr-warmup", "2", "--lr-schedule", "cosine", "--lr-min", "0.002"])
    sched = got.pop("lr_schedule")
    assert got == {} and [sched(t) for t in (0, 1, 2, 7, 12, 50)] == pytest.approx([0.01, 0.02, 0.02, 0.011, 0.002, 0.002])
    sched = run(["--lr", "0.02", "--lr-schedule", "cosine", "--max-steps", "2"])["lr_schedule"]      # total = 3 x 2
    assert [sched(t) for t in (0, 3, 6)] == pytest.approx([0.02, 0.01, 0.0])
    sched = run(["--lr", "0.02", "--lr-warmup", "4"])["lr_schedule"]                                # constant after it
    assert [sched(t) for t in (0, 3, 4, 100)] == pytest.approx([0.005, 0.02, 0.02, 0.02])
    for opt in ("--weight-decay", "--adam-l2", "--decay-bias", "--clip-grad-norm", "--lr-warmup", "--lr-schedule", "--lr-min"):
        assert opt in train.main.__doc__, opt


# ---- the C entry point's refusals ----------------------------------------------------------------------------------------

def test_entry_point_refuses_before_any_hip_call():
    """every refusal of include/cslicer_optim.h returns CSL_E_INVALID before a HIP call (there is no GPU here); the
    tensor pointers are made-up addresses nothing may follow"""
    from cslicer import _abi, aggr
    L = _abi.load()
    assert _abi.BOUND["cslicer_optim.h"] == ["csl_adamw_scratch", "csl_adamw_f32"] == aggr.OPTIM_SYMBOLS
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert list(L.csl_adamw_f32.argtypes) == [i32, vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, f32, f32, i64, vp, vp, vp, vp]
    assert L.csl_adamw_f32.restype is C.c_int and L.csl_adamw_scratch.restype is i64
    E = -1

    def scratch(numel):
        return L.csl_adamw_scratch(len(numel), (i64 * max(len(numel), 1))(*numel))
    assert [scratch(n) for n in ([], [0], [0, 0], [1], [1024], [1025], [1, 1], [255 * 1024], [256 * 1024],
                                 [256 * 1024 + 1], [1 << 40])] == [0, 0, 0, 8, 8, 16, 16, 2040, 2048, 2048, 2048]
    assert scratch([4, -1]) == E and L.csl_adamw_scratch(25, (i64 * 25)(*[1] * 25)) == E
    assert L.csl_adamw_scratch(-1, None) == E and L.csl_adamw_scratch(2, None) == E and scratch([1 << 43]) == E

    def call(count=2, numel=(4, 4), wd=(0.0, 0.0), max_norm=0.0, step=1, null=None, null_tensor=None, scr=4096, dec=1):
        n = max(count, 1)
        arrs = [(vp * n)(*[4096 * (k + 1) + 64 * t for t in range(n)]) for k in range(4)]
        if null_tensor is not None:
            arrs[null_tensor[0]][null_tensor[1]] = None
        args = [arrs[0], arrs[1], arrs[2], arrs[3], (i64 * n)(*(list(numel) + [0] * n)[:n])]
        if null is not None:
            args[null] = None
        w = None if wd is None else (C.c_float * n)(*(list(wd) + [0.0] * n)[:n])
        return L.csl_adamw_f32(count, *args, w, dec, max_norm, 1e-3, 0.9, 0.999, 1e-8, step, None, None, vp(scr), vp(0))
    assert call(count=25, numel=[4] * 25, wd=[0.0] * 25) == E and call(count=-1) == E       # count outside 0..24
    assert call(step=0) == E and call(step=-3) == E                                         # steps count from 1
    assert call(numel=(4, -1)) == E                                                         # a negative size
    for k in range(5):
        assert call(null=k) == E                                                            # a null array
    for k in range(4):
        assert call(null_tensor=(k, 1)) == E                                                # a null tensor, not empty
    assert call(wd=(0.0, -1e-3)) == E and call(wd=(float("nan"), 0.0)) == E                 # decay negative or NaN
    assert call(wd=(0.0, -1e-3), dec=0) == E
    assert call(max_norm=float("nan")) == E
    assert call(max_norm=1.0, scr=0) == E and call(max_norm=float("inf"), scr=0) == E       # clipping without its scratch
    assert call(max_norm=1.0, scr=4100) == E                                                # ... or one that is not 8-byte aligned
    # nothing to do: CSL_OK without a launch -- no tensors, only empty ones (null pointers allowed, with or without clipping)
    assert call(count=0) == 0 and call(count=0, null=0) == 0
    assert call(numel=(0, 0)) == 0 and call(numel=(0, 0), null_tensor=(0, 1), max_norm=1.0, scr=0, wd=None) == 0
