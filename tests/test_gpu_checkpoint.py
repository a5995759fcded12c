"""Checkpoints on the GPU: Trainer.save_checkpoint / load_checkpoint / skip, infer.load_model, and the
command lines (cslicer.train --save / --resume, cslicer.predict).

Two promises are tested.  LOAD EQUALS SAVE: every parameter, both moments, opt.t, opt.skipped and steps_done come back
bitwise, and predict() / evaluate() of the loaded trainer are the saver's -- both models, a 16-bit table, multi-label.
A RESUMED RUN IS THE UNINTERRUPTED RUN: load, replay the slicer with skip(), continue -- losses, parameters and moments
bitwise those of the run that was never interrupted, on the native GraphSAGE step, and for the attention model at the
fanouts (2, 2, 2) at which its backward adds at most two numbers per destination.  The three trainers of such a test live
in ONE process and share its GEMM plans (csl_gemm_f32 picks an algorithm per shape class and process): what is pinned is
that state, replay and counters come back exactly; a restarted process that picks other algorithms continues up to
float32 summation order.

Shapes: 3000 nodes, batch 64, two engine streams: 47 minibatches per epoch, an odd number, so every epoch ends in a short
round -- the round and slot logic of skip() can only go wrong there and where the epoch wraps.
"""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_NODES, F, HIDDEN, CLASSES, FAN, BATCH = 3000, 16, 16, 5, (3, 3), 64
GAT_FAN = (2, 2, 2)
LR, WD, MAX_NORM = 1e-2, 0.05, 1e-2
PER_EPOCH = (N_NODES + BATCH - 1) // BATCH
_TASK = []


def _task():
    """(indptr, indices, features, labels, node order of epoch 0, node order of epoch 1): made once, never changed"""
    if not _TASK:
        from cslicer import l0
        indptr, indices = l0.synth_graph(N_NODES, 8.0, seed=0)
        rng = np.random.default_rng(7)
        _TASK.append((indptr, indices, rng.standard_normal((N_NODES, F)).astype(np.float32),
                      rng.integers(0, CLASSES, size=N_NODES).astype(np.int64), rng.permutation(N_NODES),
                      rng.permutation(N_NODES)))
    return _TASK[0]


def _trainer(model="sage", seed=3, **kw):
    from cslicer.train import Trainer
    indptr, indices, feats, labels, p0, _ = _task()
    if model == "gat":
        kw = dict({"heads": 2, "fanouts": GAT_FAN}, **kw)
    if kw.get("multilabel"):
        labels = (feats[:, :CLASSES] > 0)                  # [N, CLASSES] of 0 / 1: a half-space of the node's own row
    kw.setdefault("fanouts", FAN)
    kw.setdefault("hidden", HIDDEN)
    t = Trainer(indptr, indices, feats, labels, CLASSES, batch=BATCH, streams=2, lr=LR, seed=seed, model=model, **kw)
    t.set_nodes(p0)
    return t


def _bits(t):
    """parameters and both moments, as int32 words on the host"""
    out = [p.detach().cpu().view(torch.int32).clone() for p in t.opt.params]
    for m, v in t.opt.state:
        out += [m.cpu().view(torch.int32).clone(), v.cpu().view(torch.int32).clone()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _schedule():
    from cslicer import train
    return train.lr_schedule("cosine", LR, warmup=5, total=PER_EPOCH + 20, min_lr=1e-4)


CASES = {"sage": ("sage", {}), "sage-bfloat16": ("sage", {"feature_dtype": "bfloat16"}),
         "sage-multilabel": ("sage", {"multilabel": True}), "gat": ("gat", {})}


@pytest.mark.parametrize("case", list(CASES))
def test_load_equals_save(case, tmp_path):
    model, kw = CASES[case]
    kw = dict(kw, weight_decay=WD, max_grad_norm=MAX_NORM)
    path = str(tmp_path / "t.ckpt")
    nodes = _task()[4][:500]
    a = _trainer(model, **kw)
    a.run(4)
    a.save_checkpoint(path, extra={"epoch": 0, "tag": case})
    assert sorted(os.listdir(str(tmp_path))) == ["t.ckpt"]
    want_bits, want_pred, want_eval = _bits(a), a.predict(nodes).cpu(), a.evaluate(nodes)
    fields = a.checkpoint_fields()
    a.close()
    b = _trainer(model, seed=4, **kw)
    assert not _same(_bits(b)[:len(b.opt.params)], want_bits[:len(b.opt.params)])       # other weights before the load
    ptrs = [p.data_ptr() for p in b.opt.params] + [x.data_ptr() for mv in b.opt.state for x in mv]
    was, extra = b.load_checkpoint(path)
    assert extra == {"epoch": 0, "tag": case} and was == fields and was["steps_done"] == 4
    assert was["seed"] == 3 and was["fanouts"] == list(GAT_FAN if model == "gat" else FAN) and was["world"] == 1
    assert ptrs == [p.data_ptr() for p in b.opt.params] + [x.data_ptr() for mv in b.opt.state for x in mv]   # filled in place
    assert _same(_bits(b), want_bits)
    assert b.opt.t == 4 and b.steps_done == 4 and int(b.opt.skipped) == 0
    assert b.opt.lr == LR
    assert torch.equal(b.predict(nodes).cpu(), want_pred)
    assert b.evaluate(nodes) == want_eval
    b.close()


def test_skipped_count_and_weights_only_load(tmp_path):
    """opt.skipped travels; optimizer=False takes the weights and nothing else; another architecture is refused by name"""
    path = str(tmp_path / "t.ckpt")
    a = _trainer(max_grad_norm=MAX_NORM)
    a.run(3)
    a.opt.skipped.fill_(2)
    a.save_checkpoint(path)
    want = _bits(a)
    a.close()
    b = _trainer(seed=4, max_grad_norm=MAX_NORM)
    b.load_checkpoint(path)
    assert int(b.opt.skipped) == 2 and b.opt.t == 3
    b.close()
    c = _trainer(seed=4)
    n = len(c.opt.params)
    assert c.load_checkpoint(path, optimizer=False)[1] == {}
    got = _bits(c)
    assert _same(got[:n], want[:n]) and c.opt.t == 0 and c.steps_done == 0 and int(c.opt.skipped) == 0
    assert all(int(x.abs().max()) == 0 for x in got[n:])                       # the moments: still zero
    c.close()
    d = _trainer(seed=4, hidden=32)
    before = _bits(d)
    with pytest.raises(ValueError, match="model has hidden = 16, the trainer has 32"):
        d.load_checkpoint(path)
    assert _same(_bits(d), before)
    d.close()


def _resume_case(model, tmp_path, **kw):
    """A: the uninterrupted run; B: the same up to the save; C: a fresh trainer that loads, skips and continues"""
    _, _, _, _, p0, p1 = _task()
    path = str(tmp_path / "epoch.ckpt")
    a = _trainer(model, lr_schedule=_schedule(), **kw)
    la0 = a.run(PER_EPOCH)
    a.set_nodes(p1)
    la1 = a.run(9)
    bits_a = _bits(a)
    assert a.steps_done == PER_EPOCH + 9 == a.opt.t
    a.close()
    b = _trainer(model, lr_schedule=_schedule(), **kw)
    assert b.run(PER_EPOCH) == la0
    b.save_checkpoint(path, extra={"epoch": 1})
    b.close()
    # (its own initial weights; the dropout masks are keyed by dropout_seed, which a resumed command line repeats)
    c = _trainer(model, seed=4, dropout_seed=3, lr_schedule=_schedule(), **kw)
    c.load_checkpoint(path)
    assert c.skip(PER_EPOCH) == (PER_EPOCH + 1) // 2 and c.steps_done == PER_EPOCH
    c.set_nodes(p1)
    lc1 = c.run(9)
    print("uninterrupted:", la1, "\nresumed:      ", lc1)
    assert lc1 == la1
    assert _same(_bits(c), bits_a)
    assert c.steps_done == PER_EPOCH + 9 == c.opt.t
    c.close()
    return path, la1


def test_resumed_run_is_the_uninterrupted_run(tmp_path):
    kw = dict(dropout=0.5, weight_decay=WD, max_grad_norm=MAX_NORM)
    path, la1 = _resume_case("sage", tmp_path, **kw)
    _, _, _, _, p0, p1 = _task()
    # controls: the same continuation WITHOUT the replay, and without the optimizer state, is another run
    c = _trainer(seed=4, dropout_seed=3, lr_schedule=_schedule(), **kw)
    assert c.native is not None
    c.load_checkpoint(path)
    c.set_nodes(p1)
    assert c.run(9) != la1
    c.close()
    c = _trainer(seed=4, dropout_seed=3, lr_schedule=_schedule(), **kw)
    c.load_checkpoint(path, optimizer=False)
    c.skip(PER_EPOCH)
    c.set_nodes(p1)
    lc = c.run(9)
    assert lc[1:] != la1[1:] and all(x != y for x, y in zip(lc[1:], la1[1:]))
    c.close()
    # once mid-epoch: rounds (0, 2) (2, 2) (4, 1), then (5, 2) (7, 2) (9, 2)
    mid = str(tmp_path / "mid.ckpt")
    a = _trainer(lr_schedule=_schedule(), **kw)
    a.run(5)
    a.save_checkpoint(mid)
    la = a.run(6, first_batch=5)
    bits_a = _bits(a)
    a.close()
    c = _trainer(seed=4, dropout_seed=3, lr_schedule=_schedule(), **kw)
    c.load_checkpoint(mid)
    assert c.skip(5) == 3
    assert c.run(6, first_batch=5) == la
    assert _same(_bits(c), bits_a)
    # a round announced by run(then=...) must be trained, not skipped
    c.run(2, first_batch=11, then=(13, 2))
    with pytest.raises(RuntimeError, match="then"):
        c.skip(2, first_batch=13)
    c.run(2, first_batch=13)
    c.close()


def test_gat_resumes_at_bit_stable_fanouts(tmp_path):
    _resume_case("gat", tmp_path, feat_dropout=0.5, weight_decay=WD, max_grad_norm=MAX_NORM)


@pytest.mark.parametrize("model", ["sage", "gat"])
def test_inference_without_a_trainer(model, tmp_path):
    from cslicer import infer, splitgnn
    indptr, indices, feats, _, p0, _ = _task()
    path = str(tmp_path / "m.ckpt")
    nodes = p0[:700]
    t = _trainer(model)
    t.run(4)
    t.save_checkpoint(path)
    want = t.predict(nodes).cpu()
    t.close()
    m = infer.load_model(path)
    assert type(m) is (splitgnn.DistGATModel if model == "gat" else splitgnn.DistSAGEModel)
    assert all(p.is_cuda for p in m.parameters())
    got = infer.full_inference(m, indptr, indices, feats, nodes=nodes)
    assert got.shape == (700, CLASSES) and torch.equal(got.cpu(), want)
    infer.release(indptr, indices)


def _eval_line(out):
    lines = [ln for ln in out.split("\n") if ln.startswith("Eval Acc")]
    assert lines, out
    return lines[-1].split(" nodes in")[0]


def test_cli_save_resume_predict(capsys, tmp_path):
    from cslicer import checkpoint, l0, predict, train
    n = 4000
    indptr, indices = l0.synth_graph(n, 9.0, seed=4)
    feats = np.random.default_rng(0).random((n, 12), dtype=np.float32)
    labels = np.argmax(feats[:, :3], axis=1).astype(np.int32)
    d = str(tmp_path / "l0")
    l0.write_l0(d, indptr, indices, features=feats, labels=labels, num_classes=3)
    f1, f2, f3 = (str(tmp_path / name) for name in ("two.ckpt", "resumed.ckpt", "three.ckpt"))
    # 3200 training nodes in minibatches of 300: 11 per epoch, rounds of 8 and 3.  Dropout and a warm-up: the step count
    # matters.  (No cosine schedule: it spans --num-epochs, which the first command line below gives as 2, not 3.)
    args = ["--graph", d, "--eval-split", "holdout", "--fan-out", "4,6", "--num-layers", "2", "--num-hidden", "16",
            "--batch-size", "300", "--dropout", "0.5", "--lr-warmup", "3", "--weight-decay", "0.01"]
    train.main(args + ["--num-epochs", "2", "--save", f1])
    out = capsys.readouterr().out
    assert "epoch 0: 11 minibatches" in out and "epoch 1: 11 minibatches" in out and "resumed" not in out
    ck = checkpoint.read(f1)
    assert ck["extra"] == {"epoch": 2} and ck["trainer"]["steps_done"] == 22 and ck["trainer"]["fanouts"] == [6, 4]
    train.main(args + ["--num-epochs", "3", "--resume", f1, "--save", f2])
    resumed = capsys.readouterr().out
    assert "resumed from %s: epoch 2, 22 steps" % f1 in resumed and "will not be" not in resumed
    assert "epoch 2: 11 minibatches" in resumed and "epoch 0:" not in resumed and "epoch 1:" not in resumed
    train.main(args + ["--num-epochs", "3", "--save", f3])
    whole = capsys.readouterr().out
    assert "epoch 2: 11 minibatches" in whole and "epoch 0:" in whole
    print(_eval_line(resumed), "|", _eval_line(whole))
    assert _eval_line(resumed) == _eval_line(whole)
    epoch2 = [[ln for ln in o.split("\n") if ln.startswith("epoch 2:")][0].split(", loss ")[1] for o in (resumed, whole)]
    assert epoch2[0] == epoch2[1]
    a, b = checkpoint.read(f2), checkpoint.read(f3)
    assert a["extra"] == b["extra"] == {"epoch": 3} and a["trainer"] == b["trainer"]
    for k in a["state"]:
        assert torch.equal(a["state"][k].view(torch.int32), b["state"][k].view(torch.int32)), k
    for name in ("m", "v"):
        assert _same([x.view(torch.int32) for x in a["optimizer"][name]], [x.view(torch.int32) for x in b["optimizer"][name]])
    # a changed setting is reported, not refused
    train.main(args + ["--batch-size", "200", "--num-epochs", "2", "--resume", f1])      # (the later --batch-size holds)
    odd = capsys.readouterr().out
    assert "resume: batch was 300, is 200: the continuation will not be the uninterrupted run's" in odd
    # ... and a file that already holds --num-epochs epochs says so instead of replaying them for nothing
    assert "resume: the file holds 2 epochs and --num-epochs is 2: nothing is left to train" in odd and "epoch 0:" not in odd
    # the saved model applied without a trainer: the accuracy the run printed
    perm = np.random.default_rng(0).permutation(n)
    hold = np.sort(perm[int(n * 0.8):])
    nodes_file, preds = str(tmp_path / "hold.npy"), str(tmp_path / "preds.npy")
    np.save(nodes_file, hold)
    predict.main(["--model", f2, "--graph", d, "--out", preds, "--nodes", nodes_file])
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and line.startswith("predict: 800 nodes, sage model (3 classes)")
    got = np.load(preds)
    assert got.dtype == np.int64 and got.shape == (800,)
    assert "Eval Acc %.4f " % float((got == labels[hold]).mean()) in _eval_line(resumed) + " "
    predict.main(["--model", f2, "--graph", d, "--out", preds, "--nodes", nodes_file, "--logits"])
    capsys.readouterr()
    logits = np.load(preds)
    assert logits.dtype == np.float32 and logits.shape == (800, 3) and np.array_equal(np.argmax(logits, axis=1), got)


def test_optimizer_state_refusals_name_the_tensor_and_change_nothing(tmp_path):
    """aggr.Adam.load_state_dict: another tensor count, shape or type is a ValueError naming the tensor, raised before
    anything is filled -- and Trainer.load_checkpoint asks before it fills the model"""
    from cslicer import checkpoint
    t = _trainer(max_grad_norm=MAX_NORM)
    t.run(3)
    good = t.opt.state_dict()
    before = _bits(t)
    n = len(t.opt.params)
    assert n >= 2 and good["m"][0].shape != good["m"][1].shape

    def bad(**kw):
        return dict(good, **kw)
    cases = [(bad(m=good["m"][:-1]), r"%d / %d moment tensors for %d parameters" % (n - 1, n, n)),
             (bad(v=good["v"] + [good["v"][0]]), r"%d / %d moment tensors" % (n, n + 1)),
             (bad(m=[good["m"][1]] + good["m"][1:]), r"m\[0\] is torch.float32 .*parameter 0 needs torch.float32"),
             (bad(v=good["v"][:1] + [good["v"][1].double()] + good["v"][2:]), r"v\[1\] is torch.float64"),
             (bad(v=good["v"][:-1] + [3.0]), r"v\[%d\] is float" % (n - 1))]
    for d, msg in cases:
        with pytest.raises(ValueError, match=msg):
            t.opt.load_state_dict(dict(d, t=99, skipped=7))
        assert _same(_bits(t), before) and t.opt.t == 3 and int(t.opt.skipped) == 0
    # through the trainer: a file whose optimizer block does not fit leaves weights, moments and counters alone
    path = str(tmp_path / "odd.ckpt")
    checkpoint.write(path, t.model, optimizer=bad(m=good["m"][:-1]), trainer=t.checkpoint_fields())
    t.close()
    b = _trainer(seed=4, max_grad_norm=MAX_NORM)
    before = _bits(b)
    with pytest.raises(ValueError, match="moment tensors"):
        b.load_checkpoint(path)
    assert _same(_bits(b), before) and b.opt.t == 0 and b.steps_done == 0
    b.load_checkpoint(path, optimizer=False)                 # the weights alone are fine
    b.close()


def test_data_parallel_replica_saves_skips_and_resumes(tmp_path):
    """DataParallelTrainer (one replica, no process group): its own _submit / loss divisors under skip(), its own writer
    rule, and the JOB's batch and replica count in the file"""
    from cslicer.train import DataParallelTrainer
    indptr, indices, feats, labels, p0, _ = _task()

    def dp(seed):
        t = DataParallelTrainer(indptr, indices, feats, labels, CLASSES, 0, 1, None, batch=BATCH, fanouts=FAN, streams=2,
                                hidden=HIDDEN, lr=LR, seed=seed, dropout=0.5, dropout_seed=3)
        t.set_nodes(p0)
        return t
    path = str(tmp_path / "dp.ckpt")
    a = dp(3)
    assert a.native is not None and a._checkpoint_peers() == (True, None)
    a.run(5)
    a.save_checkpoint(path)
    la = a.run(6, first_batch=5)
    bits_a = _bits(a)
    a.close()
    c = dp(4)
    was, _ = c.load_checkpoint(path)
    assert was["batch"] == BATCH and was["world"] == 1 and was == dict(c.checkpoint_fields(), seed=3)
    assert c.skip(5) == 3 and c.steps_done == 5
    assert c.run(6, first_batch=5) == la and _same(_bits(c), bits_a)
    c.close()


def _reorder_bound(model, feats, indptr, indices, nodes):
    """(float64 logits, bound) for `nodes`: how far two float32 evaluations of a GraphSAGE model's full-neighbour logits
    may lie apart when they differ only in the ORDER of their sums.  An output of a layer is
        sum_j W[o, j] h[v, j] + sum_j W[o, in + j] (1 / d_v) sum_u h[u, j] + b[o],
    a sum of products whichever way a kernel groups it (aggregate then project, or project then aggregate).  A term passes
    through at most K_v = 2 in + d_v + 4 roundings (the additions of the sums it is part of, its product, the division or a
    reciprocal and a product, the bias), so
    any evaluation lies within gamma_K sum |terms| of the exact value, gamma_K = K u / (1 - K u), u = 2^-24 (Higham,
    Accuracy and Stability, 3.1), and two evaluations within twice that.  A difference E of a layer's inputs reaches its
    outputs as at most [E | mean E] |W|^T (ReLU does not enlarge it) and enters the magnitudes of the next layer's terms."""
    import gat_ref
    import infer_ref
    ip, ix = infer_ref.neighbour_csr(indptr, indices)
    r = gat_ref.csr_rows(ip)
    deg = (ip[1:] - ip[:-1]).double()
    u = 2.0 ** -24

    def mean(x):
        return torch.zeros_like(x).index_add(0, r, x[ix]) / deg.clamp_min(1)[:, None]
    h = torch.as_tensor(feats).double()
    E = torch.zeros_like(h)
    for k, conv in enumerate(model.convs):
        W, b = conv.fc.weight.detach().cpu().double(), conv.fc.bias.detach().cpu().double()
        K = (W.shape[1] + deg + 4)[:, None]
        gamma = K * u / (1 - K * u)
        mag = torch.cat([h.abs() + E, mean(h.abs() + E)], 1) @ W.abs().t() + b.abs()
        E = torch.cat([E, mean(E)], 1) @ W.abs().t() + 2 * gamma * mag
        h = torch.cat([h, mean(h)], 1) @ W.t() + b
        if k + 1 < len(model.convs):
            h = torch.relu(h)
    nodes = torch.as_tensor(np.asarray(nodes, dtype=np.int64))
    return h[nodes], E[nodes]


# ---- the rank path: one part, one fresh child process over gloo ---------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(port, path, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "occ-gnn_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        import test_gpu_checkpoint as M
        t = M._trainer(weight_decay=M.WD, max_grad_norm=M.MAX_NORM, dist=dist, rank_path=True)
        assert t.native_rank is not None and t.plan.path == "native_rank"
        t.run(4)
        t.save_checkpoint(path, extra={"epoch": 0})
        nodes = M._task()[4][:500]
        assert bool(t.owns(nodes).all())
        logits, bits = t.predict(nodes).cpu(), M._bits(t)
        torch.save({"logits": logits, "bits": bits}, path + ".child")
        t.close()
        # the file in a single-GPU trainer of THIS process (the same GEMM plans: see the test's docstring)
        s = M._trainer(seed=4, weight_decay=M.WD, max_grad_norm=M.MAX_NORM)
        assert s.native is not None and not s.rank_path
        s.load_checkpoint(path)
        assert M._same(M._bits(s), bits) and torch.equal(s.predict(nodes).cpu(), logits)
        s.close()
        q.put("ok")
        dist.destroy_process_group()
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put("error: " + repr(ex))
        raise


def test_rank_path_checkpoint_loads_on_one_gpu(tmp_path):
    """A world-of-one rank-path trainer (a fresh child process, gloo) saves; a single-GPU trainer loads the file and
    predicts the rank path's logits, bit for bit.  That comparison is made INSIDE the child: the projections of inference
    are library GEMMs whose algorithm csl_gemm_f32 chooses per process, by timing the candidates on a shape class's first
    use (csrc/gemm_lt.hip), so two processes with different histories may sum in different orders.  This process, whose
    plans earlier tests of a suite run have made, loads the file too: every parameter and moment is bitwise the child's,
    and its logits equal the child's within _reorder_bound, the distance two float32 evaluations of the same sums may have
    (run alone: bitwise equal; behind other test files that had planned the same GEMM classes: max |difference| 7.15e-07
    at logits up to 5.47)."""
    import torch.multiprocessing as mp
    path = str(tmp_path / "rank.ckpt")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_rank_main, args=(_free_port(), path, q))
    proc.start()
    try:
        res = q.get(timeout=240)
    finally:
        proc.join(timeout=60)
        if proc.is_alive():          # (its own time limit: a rank that hangs is ended, not waited for)
            proc.kill()
            proc.join()
    assert res == "ok", res
    assert proc.exitcode == 0
    t = _trainer(seed=4, weight_decay=WD, max_grad_norm=MAX_NORM)
    assert t.native is not None and not t.rank_path
    was, extra = t.load_checkpoint(path)
    assert extra == {"epoch": 0} and was["steps_done"] == 4 and t.opt.t == 4 and t.steps_done == 4
    child = torch.load(path + ".child", weights_only=True)
    assert _same(_bits(t), child["bits"])
    nodes = _task()[4][:500]
    got = t.predict(nodes).cpu()
    indptr, indices, feats = _task()[:3]
    ref, bound = _reorder_bound(t.model, feats, indptr, indices, nodes)
    diff = (got.double() - child["logits"].double()).abs()
    print("logits, this process against the child: max |difference| %.3g, largest |logit| %.3g, bitwise equal: %s; "
          "difference / bound: max %.3g (bound: %.3g .. %.3g)"
          % (float(diff.max()), float(child["logits"].abs().max()), torch.equal(got, child["logits"]),
             float((diff / bound).max()), float(bound.min()), float(bound.max())))
    assert got.shape == child["logits"].shape and bool(torch.isfinite(got).all())
    assert bool((diff <= bound).all())
    # and each of the two is an evaluation of those sums: within half the bound of the float64 logits
    for name, x in (("this process", got), ("the child", child["logits"])):
        assert bool(((x.double() - ref).abs() <= bound / 2).all()), name
    t.close()
