"""Full-neighbour inference (cslicer.infer, csrc/infer.hip) on the GPU: every layer form against float64
(tests/infer_ref.py), equivalence with the trainer's own sampled forward where sampling takes every neighbour,
reproducibility, the evaluation head against torch, training left undisturbed by evaluation, accuracy of a trained
model, 64-bit row offsets, and the CLI's --eval-split."""
import numpy as np
import pytest
import torch

import infer_ref

pytestmark = pytest.mark.gpu

SEG = 512
HUB = 200_000


def _graph(n=5000, seed=0):
    """rows of 0 and 1 edges, of exactly SEG and SEG + 1, a hub of HUB edges, self loops, duplicate edges and rows whose
    only entries are self loops; the rest 0..20 random neighbours"""
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        if v == 0:
            r = []
        elif v == 1:
            r = [7]
        elif v == 2:
            r = list(rng.integers(0, n, SEG))
        elif v == 3:
            r = list(rng.integers(0, n, SEG + 1))
        elif v == 4:
            r = list(rng.integers(0, n, HUB))
        elif v == 5:
            r = [5, 5]                                    # only self loops
        elif v == 6:
            r = [9, 9, 6, 11, 9]                          # duplicates and a self loop
        elif v == 7:
            r = list(rng.integers(0, n, SEG)) + [7]       # SEG neighbours once its self loop is dropped
        else:
            r = list(rng.integers(0, n, int(rng.integers(0, 21))))
            if v % 17 == 0:
                r.append(v)
        rows.append(np.asarray(r, dtype=np.int64))
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    return indptr, np.concatenate(rows)


@pytest.fixture(scope="module")
def graph():
    return _graph()


def _close(got, want, tol, hub_rows=(), hub_tol=1e-4):
    """|got - want| <= tol * max|want[row]| per row (hub_rows: hub_tol)"""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape
    scale = want.abs().amax(1).clamp_min(1e-30)
    err = (got - want).abs().amax(1) / scale
    t = torch.full_like(err, tol)
    for r in hub_rows:
        t[r] = hub_tol
    bad = torch.nonzero(err > t).reshape(-1)
    assert bad.numel() == 0, "rows %s: relative errors %s" % (bad[:10].tolist(), err[bad[:10]].tolist())


def _models(F, dev):
    from cslicer import splitgnn
    torch.manual_seed(1)
    return {
        # 10 -> 256 aggregate first (a feature width not divisible by 4), 256 -> 7 project first (odd class count)
        "sage_a": (splitgnn.DistSAGEModel(10, 256, 7, n_layers=2).to(dev), 10),
        # 64 -> 4 project first, 4 -> 5 aggregate first
        "sage_b": (splitgnn.DistSAGEModel(64, 4, 5, n_layers=2).to(dev), 64),
        # heads 4 x 6 (a head width the kernels pad), last layer 7 classes (8 columns per head)
        "gat_a": (splitgnn.DistGATModel(10, 6, 7, heads=4, n_layers=2).to(dev), 10),
        # 8 x 32 = 256 wide hidden layer
        "gat_b": (splitgnn.DistGATModel(64, 32, 5, heads=8, n_layers=2).to(dev), 64),
    }


@pytest.mark.parametrize("name", ["sage_a", "sage_b", "gat_a", "gat_b"])
def test_layer_forms_against_float64(graph, name):
    """The hub row (4, HUB neighbours) sums 2 * 10^5 float32 rows in a different order than float64: 1e-4 there."""
    from cslicer import infer
    indptr, indices = graph
    dev = torch.device("cuda", 0)
    model, F = _models(10, dev)[name]
    n = indptr.shape[0] - 1
    feats = torch.rand((n, F), generator=torch.Generator().manual_seed(2)) * 2 - 1
    nodes = np.concatenate([np.arange(12), np.random.default_rng(3).choice(n, 300, replace=False)])
    got = infer.full_inference(model, indptr, indices, feats.numpy(), nodes=nodes, chunk_rows=777)
    want = infer_ref.model(model, feats, indptr, indices, nodes=nodes)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == want.shape
    _close(got, want, 1e-5, hub_rows=[4])
    # every node as the last layer's rows too
    allg = infer.full_inference(model, indptr, indices, feats.numpy(), chunk_rows=1500)
    _close(allg, infer_ref.model(model, feats, indptr, indices), 1e-5, hub_rows=[4])


def test_wide_attention_hidden_layer():
    """a hidden layer of 8 heads x 520 = 4,160 columns (more than a last layer may have): column tiles of one wave"""
    from cslicer import infer, splitgnn
    indptr, indices = _small_graph(n=1500, max_deg=8)
    dev = torch.device("cuda", 0)
    torch.manual_seed(12)
    model = splitgnn.DistGATModel(12, 520, 5, heads=8, n_layers=2).to(dev)
    feats = torch.rand((1500, 12), generator=torch.Generator().manual_seed(13))
    nodes = np.arange(0, 1500, 7)
    got = infer.full_inference(model, indptr, indices, feats.numpy(), nodes=nodes, chunk_rows=500)
    _close(got, infer_ref.model(model, feats, indptr, indices, nodes=nodes), 1e-5)


def test_reproducible_and_chunk_independent(graph):
    from cslicer import infer
    indptr, indices = graph
    dev = torch.device("cuda", 0)
    n = indptr.shape[0] - 1
    feats = torch.rand((n, 64), generator=torch.Generator().manual_seed(4)).to(dev)
    for name in ("sage_b", "gat_b"):
        model, _ = _models(64, dev)[name]
        a = infer.full_inference(model, indptr, indices, feats, chunk_rows=777)
        b = infer.full_inference(model, indptr, indices, feats, chunk_rows=777)
        assert torch.equal(a, b), name                    # bitwise, hub rows included
        c = infer.full_inference(model, indptr, indices, feats, chunk_rows=4096)
        _close(c, a, 1e-5)


def test_eval_head_against_torch():
    from cslicer import infer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    logits = torch.randn((3001, 13), generator=g)
    logits[::7, 3] = logits[::7, 9] = logits[::7].amax(1) + 1.0      # exact ties: the lower index wins
    logits[5] = 0.25                                                   # all equal
    labels = torch.randint(0, 13, (3001,), generator=g)
    labels[::3] = logits[::3].argmax(1)
    pred, correct, loss = infer.eval_head(logits.to(dev), labels.to(dev))
    assert torch.equal(pred.cpu(), torch.argmax(logits, 1))
    assert pred[5].item() == 0
    assert correct == int((torch.argmax(logits, 1) == labels).sum())
    want = torch.nn.functional.cross_entropy(logits.double(), labels, reduction="sum").item()
    assert abs(loss - want) <= 1e-5 * abs(want)
    pred, correct, loss = infer.eval_head(torch.empty((0, 13), device=dev), torch.empty((0,), dtype=torch.int64, device=dev))
    assert pred.numel() == 0 and correct == 0 and loss == 0.0


def _small_graph(n=3000, seed=6, max_deg=4):
    """max degree below every fanout of the tests (5): sampling takes every neighbour; with self loops and duplicates"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, max_deg + 1, n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n, int(indptr[-1]))
    rows = np.repeat(np.arange(n), deg)
    sl = rng.random(indices.shape[0]) < 0.05
    indices[sl] = rows[sl]                                             # self loops
    first = indptr[:-1][deg >= 2]
    indices[first + 1] = indices[first]                                # a duplicate edge in every row of 2+
    return indptr, indices


@pytest.mark.parametrize("kind", ["sage", "gat"])
def test_equals_sampled_forward(kind):
    """Where the slicer takes every neighbour, full inference is the trained model's own forward.  GAT: 1e-4 (the
    trainer's input layer aggregates and then projects, full inference projects first)."""
    from cslicer import aggr, infer, splitgnn
    from cslicer.train import Trainer
    indptr, indices = _small_graph()
    n = indptr.shape[0] - 1
    rng = np.random.default_rng(7)
    feats = rng.random((n, 24), dtype=np.float32)
    labels = rng.integers(0, 5, n)
    t = Trainer(indptr, indices, feats, labels, 5, fanouts=(5, 5), batch=512, streams=1, hidden=16, model=kind,
                heads=4)
    t.set_nodes(rng.permutation(n))
    t.run(3)                                                           # weights that are not the initial ones
    seeds = rng.choice(n, 400, replace=False)
    with torch.no_grad():
        t.eng.submit_seeds([seeds], slot=0)
        meta = t.eng.meta(0, 0)
        slices = splitgnn.slices_of(t.eng, 0, 0, parts=[0], device=t.dev, meta=meta)
        top, deep = slices[0][0], slices[t.L - 1][0]
        if kind == "sage":
            logits = t.model.forward_local(slices, t.feat)
        else:
            x = (aggr.FeatureRows(t.feat, deep.in_nodes) if getattr(t, "gat_input", False)
                 else aggr.gather_rows(t.feat, deep.in_nodes))
            logits = t.model.forward_parts(slices, {0: x})[0]
        order = top.out_nodes.long().cpu().numpy()
    full = infer.full_inference(t.model, indptr, indices, t.feat, nodes=order)
    assert sorted(order.tolist()) == sorted(seeds.tolist())
    tol = 1e-5 if kind == "sage" else 1e-4
    scale = logits.abs().max().item()
    assert (full - logits).abs().max().item() <= tol * scale, (full - logits).abs().max().item() / scale
    t.close()


def _task(n=6000, F0=24, classes=5, seed=3):
    from cslicer import l0
    indptr, indices = l0.synth_graph(n, 14.0, seed=seed)
    rng = np.random.default_rng(seed)
    feats = rng.random((n, F0), dtype=np.float32)
    labels = np.argmax(feats[:, :classes], axis=1).astype(np.int64)   # learnable from the self features
    return indptr, indices, feats, labels, rng.permutation(n)


def _training_state(t):
    """everything a training step reads or advances, copied: parameters, Adam moments and step count, the loss ring,
    the engine's totals, torch's CPU and device RNG states"""
    torch.cuda.synchronize()
    ring = getattr(t, "_loss_ring", None)
    return {
        "params": [p.detach().clone() for p in t.model.parameters()],
        "adam": [(m.clone(), v.clone()) for m, v in t.opt.state],
        "adam_t": t.opt.t,
        "ring": None if ring is None else (ring.clone(), t._ring_at),
        "totals": t.eng.totals(),
        "rng": (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()),
        "steps": t.steps_done,
    }


def _same_state(a, b):
    assert a["adam_t"] == b["adam_t"] and a["totals"] == b["totals"] and a["steps"] == b["steps"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a["adam"], b["adam"]))
    assert (a["ring"] is None) == (b["ring"] is None)
    if a["ring"] is not None:
        assert torch.equal(a["ring"][0], b["ring"][0]) and a["ring"][1] == b["ring"][1]
    assert torch.equal(a["rng"][0], b["rng"][0]) and torch.equal(a["rng"][1], b["rng"][1])


@pytest.mark.parametrize("kind", ["sage", "sage_py", "gat"])
def test_evaluation_does_not_disturb_training(kind, monkeypatch):
    """evaluate() / predict() between two run(10) calls leave every piece of training state bitwise as it was
    (parameters, Adam moments and step count, loss ring, engine totals, RNG states).  A twin that does not evaluate then
    samples exactly the same work (units, totals).  Its losses agree within the run-to-run spread of twins that never
    evaluate (the steps' float atomics), measured over three such twins, with a floor of 1e-4 of the mean loss."""
    from cslicer.train import Trainer
    if kind == "sage_py":
        monkeypatch.setenv("CSLICER_PY_STEP", "1")
    indptr, indices, feats, labels, perm = _task()
    model = "gat" if kind == "gat" else "sage"

    def twin(evaluate):
        t = Trainer(indptr, indices, feats, labels, 5, fanouts=(10, 5), batch=256, streams=4, hidden=32, lr=1e-2,
                    model=model, heads=4)
        t.set_nodes(perm[:4800])
        a = t.run(10)
        if evaluate:
            before = _training_state(t)
            ev = t.evaluate(perm[4800:])
            assert ev["n"] == 1200 and 0.0 <= ev["accuracy"] <= 1.0 and np.isfinite(ev["loss"])
            assert t.predict().shape == (6000, 5)
            _same_state(before, _training_state(t))
        b = t.run(10)
        out = (np.array(a + b), [dict(u) for u in t.units], t.eng.totals())
        t.close()
        return out

    plain = [twin(False) for _ in range(3)]
    evald = twin(True)
    for p in plain:
        assert evald[1] == p[1] and evald[2] == p[2]
    spread = max(float(np.max(np.abs(x[0] - y[0]))) for i, x in enumerate(plain) for y in plain[i + 1:])
    tol = max(4 * spread, 1e-4 * float(np.mean(np.abs(plain[0][0]))))
    diff = max(float(np.max(np.abs(evald[0] - p[0]))) for p in plain)
    assert diff <= tol, (diff, spread, tol)


def _homophilous(indptr, labels, deg=10, seed=11):
    """the same nodes with every row replaced by `deg` neighbours of the node's own class: the attention model has no
    self term (its softmax runs over the neighbours only), so its task must be visible in the neighbours"""
    rng = np.random.default_rng(seed)
    n = labels.shape[0]
    indices = np.empty(n * deg, dtype=np.int64)
    for c in np.unique(labels):
        m = np.flatnonzero(labels == c)
        pick = m[rng.integers(0, m.shape[0], (m.shape[0], deg))]
        indices[(m[:, None] * deg + np.arange(deg)[None, :]).reshape(-1)] = pick.reshape(-1)
    return np.arange(0, n * deg + 1, deg, dtype=np.int64), indices


@pytest.mark.parametrize("kind", ["sage", "gat"])
def test_trained_model_is_accurate(kind):
    """test_gpu_train._task (labels = argmax of a node's first five features); for the attention model the same
    features and labels over a graph whose neighbours share the node's class."""
    from cslicer.train import Trainer
    indptr, indices, feats, labels, perm = _task()
    if kind == "gat":
        indptr, indices = _homophilous(indptr, labels)
    t = Trainer(indptr, indices, feats, labels, 5, fanouts=(10, 5), batch=256, streams=4, hidden=32, lr=1e-2,
                model=kind, heads=4)
    held = perm[4800:]
    before = t.evaluate(held)
    t.set_nodes(perm[:4800])
    t.run(60)
    after = t.evaluate(held)
    assert after["accuracy"] > 0.5 and after["accuracy"] > before["accuracy"] + 0.2, (before, after)
    assert after["loss"] < before["loss"]
    logits = t.predict(held)
    assert logits.shape == (1200, 5)
    acc = (logits.argmax(1).cpu().numpy() == labels[held]).mean()
    assert abs(acc - after["accuracy"]) < 1e-9
    t.close()


def test_data_parallel_trainer_evaluates():
    """a DataParallelTrainer replica (every feature row, the native GraphSAGE step) evaluates and predicts like the model
    it holds"""
    from cslicer import infer
    from cslicer.train import DataParallelTrainer
    indptr, indices, feats, labels, perm = _task()
    t = DataParallelTrainer(indptr, indices, feats, labels, 5, dp_rank=0, dp_world=1, dist=None, batch=256,
                            fanouts=(10, 5), streams=4, hidden=32, lr=1e-2)
    assert t.native is not None
    held = perm[4800:]
    t.set_nodes(perm[:4800])
    t.run(60)
    ev = t.evaluate(held)
    assert ev["n"] == 1200 and ev["accuracy"] > 0.5
    logits = t.predict(held)
    want = infer.full_inference(t.model, indptr, indices, feats, nodes=held)
    assert torch.equal(logits, want)
    assert abs((logits.argmax(1).cpu().numpy() == labels[held]).mean() - ev["accuracy"]) < 1e-9
    t.close()


def test_rank_path_refuses_evaluation():
    from cslicer.train import Trainer
    t = Trainer.__new__(Trainer)
    t.rank_path = True
    with pytest.raises(NotImplementedError, match="rank path"):
        t.evaluate(np.arange(3))


def test_64bit_offsets():
    """A first-layer input of 9 M x 256 floats (> 2^31) generated on the device; rows near the end against float64."""
    from cslicer import infer, splitgnn
    dev = torch.device("cuda", 0)
    n, F = 9_000_000, 256
    rng = np.random.default_rng(8)
    indptr = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    indices = rng.integers(0, n, 2 * n)
    indices[-4:] = [n - 1, n - 2, 17, n - 3]
    feats = torch.empty((n, F), dtype=torch.float32, device=dev)
    feats.uniform_(-1, 1, generator=torch.Generator(device=dev).manual_seed(9))
    torch.manual_seed(10)
    model = splitgnn.DistSAGEModel(F, 256, 5, n_layers=2).to(dev)     # 256 -> 256 aggregate first over the big table
    nodes = np.array([n - 1, n - 2, n - 5, 3], dtype=np.int64)
    got = infer.full_inference(model, indptr, indices, feats, nodes=nodes)
    ip, ix = infer_ref.neighbour_csr(indptr, indices)
    need = np.unique(np.concatenate([nodes] + [ix[ip[v]:ip[v + 1]].numpy() for v in nodes]))
    hop2 = np.unique(np.concatenate([need] + [ix[ip[v]:ip[v + 1]].numpy() for v in need]))
    f = {int(v): feats[int(v)].double().cpu() for v in hop2}
    c0, c1 = model.convs
    W0, b0 = c0.fc.weight.double().cpu(), c0.fc.bias.double().cpu()
    W1, b1 = c1.fc.weight.double().cpu(), c1.fc.bias.double().cpu()

    def mean(v, table):
        nb = ix[ip[v]:ip[v + 1]].tolist()
        return torch.stack([table[u] for u in nb]).mean(0) if nb else torch.zeros(F, dtype=torch.float64)

    h1 = {int(v): torch.relu(torch.cat([f[int(v)], mean(int(v), f)]) @ W0.t() + b0) for v in need}
    want = torch.stack([torch.cat([h1[int(v)], mean(int(v), h1)]) @ W1.t() + b1 for v in nodes])
    del feats
    _close(got, want, 1e-5)


def _write_dir(path, n=3000, splits=None):
    from cslicer import l0
    indptr, indices, feats, labels, perm = _task(n=n)
    kw = {} if splits is None else {"train_idx": splits[0], "val_idx": splits[1]}
    l0.write_l0(str(path), indptr, indices, features=feats, labels=labels, num_classes=5, **kw)
    return perm


def test_cli_eval_split(tmp_path, capsys, monkeypatch):
    from cslicer import train
    _write_dir(tmp_path / "h")
    args = ["--num-epochs", "2", "--fan-out", "5,5", "--num-layers", "2", "--batch-size", "256", "--max-steps", "3",
            "--num-hidden", "32", "--eval-every", "1"]
    train.main(["--graph", str(tmp_path / "h"), "--eval-split", "holdout"] + args)
    out = capsys.readouterr().out
    assert out.count("Eval Acc") == 2, out
    # file: training only ever sees train_idx
    tr_idx = np.arange(0, 3000, 3)
    va_idx = np.setdiff1d(np.arange(3000), tr_idx)
    _write_dir(tmp_path / "f", splits=(tr_idx, va_idx))
    seen = []
    orig = train.Trainer.set_nodes
    monkeypatch.setattr(train.Trainer, "set_nodes", lambda self, nodes: (seen.append(np.array(nodes)), orig(self, nodes)))
    train.main(["--graph", str(tmp_path / "f"), "--eval-split", "file"] + args)
    out = capsys.readouterr().out
    assert out.count("Eval Acc") == 2
    assert len(seen) == 2 and all(sorted(s.tolist()) == tr_idx.tolist() for s in seen)
    assert ("%d nodes" % va_idx.shape[0]) in out
