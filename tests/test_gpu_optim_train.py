"""The optimizer's new arguments through the trainer: Trainer(weight_decay=, decoupled_weight_decay=,
decay_bias=, max_grad_norm=, lr_schedule=) on the native GraphSAGE step (one flat gradient buffer), on the attention
model's autograd step (separate p.grad tensors) and on a world-of-one rank path (the all-reduced flat buffer, gloo, a
fresh child process).

The gradients are the trainer's own, read back after each step, so only the optimizer is under test: every step is
replayed by tests/optim_ref.py in float64 from the trainer's previous parameters and moments, within the one-step bounds
derived in tests/test_gpu_optim_edges.py's docstring.  A model's gradients are not range-controlled as that file's are, so
each bound carries the absolute floor of the format as well: a float32 result below 2^-126 is rounded to a multiple of
2^-149 (an error of up to 2^-150 whatever its size), counted once per rounding.
"""
import os
import socket

import numpy as np
import pytest
import torch

import optim_ref as R
import tail_ref as T

pytestmark = pytest.mark.gpu

U, TINY = 2.0 ** -24, 2.0 ** -149
N_NODES, F, HIDDEN, CLASSES, FAN, BATCH, STEPS = 3000, 16, 16, 5, (3, 3), 64, 4
LR, WD, MAX_NORM = 1e-2, 0.05, 1e-2
B1, B2, EPS = 0.9, 0.999, 1e-8


def _task():
    from cslicer import l0
    indptr, indices = l0.synth_graph(N_NODES, 8.0, seed=0)
    rng = np.random.default_rng(7)
    return (indptr, indices, rng.standard_normal((N_NODES, F)).astype(np.float32),
            rng.integers(0, CLASSES, size=N_NODES).astype(np.int64), rng.permutation(N_NODES))


def _trainer(model="sage", **kw):
    from cslicer.train import Trainer
    indptr, indices, feats, labels, perm = _task()
    if model == "gat":
        kw = dict(kw, heads=2)
    t = Trainer(indptr, indices, feats, labels, CLASSES, fanouts=FAN, batch=BATCH, streams=2, hidden=HIDDEN, lr=LR, seed=3,
                model=model, **kw)
    t.set_nodes(perm)
    return t


def _bits(t):
    """parameters and both moments, as int32 words"""
    out = [p.detach().cpu().view(torch.int32).clone() for p in t.opt.params]
    for m, v in t.opt.state:
        out += [m.cpu().view(torch.int32).clone(), v.cpu().view(torch.int32).clone()]
    return out


def _step_grads(t):
    """the gradients the step just done handed to the optimizer, one float64 host tensor per parameter"""
    flat = t.native.grads if t.native is not None else (t.native_rank.grads if t.native_rank is not None else None)
    out, o = [], 0
    for p in t.opt.params:
        if flat is not None:
            out.append(flat[o:o + p.numel()].detach().cpu().double())
            o += p.numel()
        else:
            out.append(p.grad.detach().reshape(-1).cpu().double())
    return out


def test_infinite_max_norm_and_no_decay_train_the_defaults_native_step():
    a, b = _trainer(), _trainer(max_grad_norm=float("inf"), weight_decay=0.0)
    assert a.native is not None and b.native is not None and a.opt.grad_norm is None and b.opt.grad_norm is not None
    la, lb = a.run(STEPS), b.run(STEPS)
    assert la == lb and len(la) == STEPS
    for x, y in zip(_bits(a), _bits(b)):
        assert torch.equal(x, y)
    assert a.opt.t == b.opt.t == STEPS and int(b.opt.skipped) == 0 and int(a.opt.skipped) == 0
    n = float(b.opt.grad_norm)
    n64 = R.grad_norm(_step_grads(b))
    assert 0 < n < 100 and abs(n - n64) <= (U + 1e-12) * n64
    # the report: three lines without clipping, as they always were; two more with it
    assert a.report().count("\n") == 2 and b.report().startswith(a.report().split("\n")[0][:18])
    assert b.report().split("\n")[3:] == ["last gradient norm: %.6g" % n, "skipped steps (non-finite gradient): 0"]
    a.close()
    b.close()


def test_infinite_max_norm_and_no_decay_train_the_defaults_autograd_step():
    """the attention model: separate p.grad tensors.  Its backward may add in any order, so instead of a second trainer the
    default optimizer (csl_adam_f32) shadows this one on copies, fed the very gradients of each step"""
    from cslicer import aggr
    t = _trainer("gat", max_grad_norm=float("inf"), weight_decay=0.0)
    assert t.native is None and t.plan.path == "parts" and not t.opt._plain
    shadow = aggr.Adam([p.detach().clone() for p in t.opt.params], lr=LR)
    assert shadow._plain
    for step in range(STEPS):
        t.run(1, first_batch=step)
        for q, p in zip(shadow.params, t.opt.params):
            q.grad = p.grad.detach().clone()
        shadow.step()
        torch.cuda.synchronize()
        for q, p, (qm, qv), (pm, pv) in zip(shadow.params, t.opt.params, shadow.state, t.opt.state):
            for x, y in ((q, p), (qm, pm), (qv, pv)):
                assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32)), step
    assert t.opt.t == STEPS and int(t.opt.skipped) == 0 and float(t.opt.grad_norm) > 0
    t.close()


def replay(t, decoupled, steps=STEPS):
    """`steps` single steps of a trainer built with weight_decay=WD, decay_bias=False, max_grad_norm=MAX_NORM, each replayed
    in float64; returns the clip coefficients"""
    cs = []
    wds = [WD if p.dim() >= 2 else 0.0 for p in t.opt.params]
    assert t.opt.weight_decay == wds and 0.0 in wds and WD in wds and t.opt.decoupled == decoupled
    for step in range(1, steps + 1):
        before = [(p.detach().cpu().clone(), m.cpu().clone(), v.cpu().clone()) for p, (m, v) in zip(t.opt.params, t.opt.state)]
        t.run(1, first_batch=step - 1)
        assert t.opt.t == step and t.steps_done == step
        grads = _step_grads(t)
        n64 = R.grad_norm(grads)
        N = sum(g.numel() for g in grads)
        assert abs(float(t.opt.grad_norm) - n64) <= (U + (N + 2) * 2.0 ** -53) * n64
        c = R.clip_coef(n64, MAX_NORM)
        cs.append(c)
        for j, (p, (m, v)) in enumerate(zip(t.opt.params, t.opt.state)):
            p0, m0, v0 = (x.reshape(-1) for x in before[j])
            st = R.adamw_step(p0, grads[j], m0, v0, c, wds[j], decoupled, LR, B1, B2, EPS, step)
            kg = st.g2_roundings
            p1, m1, v1 = p.detach().reshape(-1).cpu(), m.reshape(-1).cpu(), v.reshape(-1).cpu()
            what = "step %d, tensor %d %r" % (step, j, tuple(p.shape))

            def within(got, want, bound, name):
                err = (got.double() - want).abs()
                ratio = float((err / bound).max())
                print("error / bound: %s %s %.6g" % (what, name, ratio))
                assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, name, ratio)
            within(m1, st.m, (4 + kg) * (U * st.m_abs + TINY), "m")
            within(v1, st.v, (4 + 2 * kg) * (U * st.v_abs + TINY), "v")
            upd_k = T.adam_update(m1, v1, LR, B1, B2, EPS, step)                  # from the kernel's own moments
            pk = st.p_in - upd_k
            extra = U * st.p_in.abs() if (wds[j] > 0 and decoupled) else 0.0
            within(p1, pk, 2 * U * pk.abs() + 16 * U * upd_k.abs() + extra + 19 * TINY, "p")
            assert not torch.equal(p1, p0)
    assert int(t.opt.skipped) == 0
    return cs


@pytest.mark.parametrize("model,decoupled", [("sage", True), ("sage", False), ("gat", False), ("gat", True)])
def test_every_step_replays_in_float64(model, decoupled):
    t = _trainer(model, weight_decay=WD, decoupled_weight_decay=decoupled, decay_bias=False, max_grad_norm=MAX_NORM)
    assert (t.native is not None) == (model == "sage")
    cs = replay(t, decoupled)
    assert len(cs) == STEPS and all(c < 1.0 for c in cs), cs           # every step clipped
    t.close()


def test_decay_bias_decays_every_tensor():
    t = _trainer(weight_decay=WD, decay_bias=True)
    assert t.opt.weight_decay == [WD] * len(t.opt.params) and t.opt.grad_norm is None and not t.opt._plain
    t.close()


# ---- the rank path: one part, one fresh child process over gloo ---------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "occ-gnn_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        import test_gpu_optim_train as M
        t = M._trainer(weight_decay=M.WD, decoupled_weight_decay=False, max_grad_norm=M.MAX_NORM, dist=dist, rank_path=True)
        assert t.native_rank is not None and t.plan.path == "native_rank"
        cs = M.replay(t, False)
        t.close()
        q.put(("ok", cs))
        dist.destroy_process_group()
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put(("error: " + repr(ex), None))
        raise


def test_every_step_replays_on_a_world_of_one_rank_path():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_rank_main, args=(_free_port(), q))
    proc.start()
    try:
        res = q.get(timeout=240)
    finally:
        proc.join(timeout=60)
        if proc.is_alive():          # (its own time limit: a rank that hangs is ended, not waited for)
            proc.kill()
            proc.join()
    assert res[0] == "ok", res[0]
    assert proc.exitcode == 0
    assert len(res[1]) == STEPS and all(c < 1.0 for c in res[1]), res[1]


# ---- the schedule ------------------------------------------------------------------------------------------------------

def test_lr_schedule_sets_the_rate_before_every_step():
    from cslicer import train
    sched = train.lr_schedule("cosine", LR, warmup=2, total=10, min_lr=1e-4)
    seen = []

    def spy(t):
        seen.append(t)
        return sched(t)
    t = _trainer(lr_schedule=spy, max_grad_norm=float("inf"))
    assert t.opt.lr == LR                                   # not touched before the first step
    t.run(3)
    assert seen == [0, 1, 2] and t.opt.lr == sched(2) and sched(2) == LR and sched(0) == LR / 2
    assert t.steps_done == 3 and t.opt.t == 3 and int(t.opt.skipped) == 0
    t.run(2, first_batch=3)
    assert seen == [0, 1, 2, 3, 4] and t.opt.lr == sched(4) < LR
    t.close()
    # None never touches opt.lr
    t = _trainer()
    t.opt.lr = 0.5 * LR
    t.run(2)
    assert t.opt.lr == 0.5 * LR and t.lr_schedule is None
    t.close()
