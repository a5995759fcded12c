"""Layer normalisation between the GraphSAGE layers on the GPU, from the native step to the trainer (DESIGN 4.13;
include/cslicer_layernorm.h, csrc/sage_step.hip; the kernels alone: tests/test_gpu_norm_edges.py):

* csl_sage_fwd_bwd_norm against the float64 model of tests/norm_ref.py on the same slices, L = 2, 3, 4, with the fused
  deepest layer and without, with dropout at p = 0.5 under the same masks, class weights and label smoothing, the
  multi-label loss, a bfloat16 table, rows that make the sequencer pad (a layer shorter than row_pad among them); L = 1 is
  bitwise the plain step;
* trainers: norm=None is the trainer without the argument, equal seeds give equal runs, the native step against
  CSLICER_PY_STEP=1 and against the `parts` path;
* the rank path over gloo, two ranks and one, against the single-process float64 model: the step and predict();
* evaluate / predict of a normalised model against float64, whole-graph; save -> load -> predict.

Tolerances: loss 1e-5 relative, every parameter gradient within 1e-4 of its largest entry, logits 1e-5;
everything said to be "the same run" bit for bit.
"""
import os
import socket

import numpy as np
import pytest
import torch

import norm_ref

pytestmark = pytest.mark.gpu

N_NODES, F0, HIDDEN, CLASSES, BATCH = 2000, 12, 24, 5, 64
ROW_PAD, N_SLABS = 64, 4
P, SEED, STEP = 0.5, (5 << 32) | 4242, 3
EPS = 1e-5
FANS = {2: (3, 3), 3: (3, 3, 2), 4: (2, 2, 2, 2)}


def _graph(n=N_NODES, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 13, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(d, out=indptr[1:])
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)


def _node_data(n=N_NODES, F=F0, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, F)).astype(np.float32), rng.integers(0, CLASSES, size=n).astype(np.int64),
            rng.permutation(n))


def _model(L, F=F0, norm="layer", classes=CLASSES):
    from cslicer import splitgnn
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(F, HIDDEN, classes, n_layers=L, norm=norm, norm_eps=EPS).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
        for m in getattr(model, "norms", ()):        # (away from ones and zeros, a zero and negative entries among them)
            m.gamma.normal_(1.0, 0.5)
            m.gamma[3] = 0.0
            m.gamma[5] = -0.7
            m.beta.normal_(0, 0.3)
    return model


def _parts(model):
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    return ws, bs, [m.gamma for m in model.norms], [m.beta for m in model.norms]


def _native(model, fan, seeds, feats, labels, drop=None, loss=None):
    """(loss, flat gradients) of one native step on a fresh engine's first sample"""
    from cslicer import _abi, aggr, splitgnn
    L = len(fan)
    indptr, indices = _graph()
    eng = _abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=max(BATCH, len(seeds)), mode=_abi.MODE_GRAPH,
                      flags=_abi.FLAG_TRANSPOSE)
    try:
        eng.submit_seeds([seeds])
        slices = splitgnn.slices_of(eng)
        order = [slices[L - 1 - k][0] for k in range(L)]
        step = aggr.SageStep(model, ROW_PAD, N_SLABS)
        out = torch.zeros(1, device="cuda")
        for _ in range(2):     # (the second call runs on the recorded GEMM plans and the reused workspace)
            # (the multi-label loss is the mean over seeds x classes)
            step(order, feats, labels, 1.0 / (len(seeds) * (CLASSES_ML if labels.dim() == 2 else 1)), out, drop,
                 **({} if loss is None else {"loss": loss}))
        torch.cuda.synchronize()
        return float(out[0]), step.grads.clone()
    finally:
        eng.close()


CLASSES_ML = 37     # multi-label targets: two packed words per row


def _assert_close(got_loss, got_grads, want_loss, want, L, what=""):
    print("%sloss %.9g (float64 %.9g)" % (what, got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    names = [n for k in range(L) for n in ("W_%d" % k, "b_%d" % k)] + [n for k in range(L - 1) for n in ("gamma_%d" % k, "beta_%d" % k)]
    assert len(want) == len(names)
    at = 0
    for name, g in zip(names, want):
        seg = got_grads[at:at + g.numel()].reshape(g.shape)
        at += g.numel()
        err, ref = float((seg - g).abs().max()), float(g.abs().max())
        print("%sgradient of %s: max error %.3g, largest entry %.3g" % (what, name, err, ref))
        assert ref > 0 and err <= 1e-4 * ref, "gradient of %s: max error %.3g against a largest entry of %.3g" % (name, err, ref)
    assert at == got_grads.numel()


def _traversal(fan, seeds):
    from oracle import oracle as orc
    indptr, indices = _graph()
    return orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)


@pytest.mark.parametrize("fused", [True, False], ids=["fused-deepest-layer", "no-mfma-fwd"])
@pytest.mark.parametrize("L", [2, 3, 4])
def test_native_step_matches_float64(L, fused, monkeypatch):
    from cslicer import aggr
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    assert aggr._lib().csl_sage_fwd_mfma_scratch(F0, HIDDEN) > 0       # these widths are the fused layer's
    fan = FANS[L]
    feats, labels, perm = _node_data()
    seeds = perm[:BATCH]
    model = _model(L)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    got_loss, got = _native(model, fan, seeds, x, lab)
    want_loss, want = norm_ref.model_on_traversal(_traversal(fan, seeds), feats, labels, *_parts(model), EPS, N_NODES)
    _assert_close(got_loss, got.double().cpu(), want_loss, want, L)
    # and it IS the norm: the plain model with the same layers is another loss
    plain = _model(L, norm=None)
    plain.load_state_dict({k: v for k, v in model.state_dict().items() if k.startswith("convs.")})
    plain_loss, _ = _native(plain, fan, seeds, x, lab)
    assert abs(plain_loss - got_loss) > 1e-3 * abs(plain_loss)


@pytest.mark.parametrize("L", [3, 4])
def test_native_step_with_dropout_matches_float64_with_the_same_masks(L):
    """(four layers: more second stages and more rescaled segments than one launch of either takes)"""
    from cslicer import aggr
    fan = FANS[L]
    feats, labels, perm = _node_data()
    seeds = perm[:BATCH]
    model = _model(L)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    got_loss, got = _native(model, fan, seeds, x, lab, aggr.DropSpec(P, SEED, STEP))
    want_loss, want = norm_ref.model_on_traversal(_traversal(fan, seeds), feats, labels, *_parts(model), EPS, N_NODES,
                                                  drop=(P, SEED, STEP))
    _assert_close(got_loss, got.double().cpu(), want_loss, want, L)


def test_native_step_with_class_weights_and_label_smoothing():
    from cslicer import aggr
    L, fan = 3, FANS[3]
    feats, labels, perm = _node_data()
    seeds = perm[:BATCH]
    model = _model(L)
    w = np.linspace(0.5, 2.0, CLASSES).astype(np.float32)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    got_loss, got = _native(model, fan, seeds, x, lab, aggr.DropSpec(P, SEED, STEP),
                            aggr.LossSpec(torch.from_numpy(w).cuda(), 0.1))
    want_loss, want = norm_ref.model_on_traversal(_traversal(fan, seeds), feats, labels, *_parts(model), EPS, N_NODES,
                                                  drop=(P, SEED, STEP), w=w, smoothing=float(np.float32(0.1)))
    _assert_close(got_loss, got.double().cpu(), want_loss, want, L)


def test_native_step_with_the_multilabel_loss():
    from cslicer import aggr
    L, fan = 3, FANS[3]
    feats, _, perm = _node_data()
    seeds = perm[:BATCH]
    y = np.random.default_rng(2).random((N_NODES, CLASSES_ML)) < 0.3
    model = _model(L, classes=CLASSES_ML)
    x, words = torch.from_numpy(feats).cuda(), torch.from_numpy(aggr.pack_labels(y)).cuda()
    got_loss, got = _native(model, fan, seeds, x, words)
    want_loss, want = norm_ref.model_on_traversal(_traversal(fan, seeds), feats, y, *_parts(model), EPS, N_NODES, multilabel=True)
    _assert_close(got_loss, got.double().cpu(), want_loss, want, L)


def test_bfloat16_table_is_its_float32_upcast():
    feats, labels, perm = _node_data()
    t16 = torch.from_numpy(feats).to(torch.bfloat16).cuda()
    lab = torch.from_numpy(labels).cuda()
    model = _model(3)
    a = _native(model, FANS[3], perm[:BATCH], t16, lab)
    b = _native(model, FANS[3], perm[:BATCH], t16.float(), lab)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


@pytest.mark.parametrize("n_seeds", [40, 64, 65], ids=["top-layer-shorter-than-row-pad", "a-multiple", "one-more"])
def test_rows_the_sequencer_pads(n_seeds):
    """row_pad = 64: 40 seeds are a layer shorter than it (padded to 64), 65 one row into the next multiple; the layers
    below are whatever the sample gives"""
    L, fan = 3, FANS[3]
    feats, labels, perm = _node_data()
    seeds = perm[:n_seeds]
    model = _model(L)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    got_loss, got = _native(model, fan, seeds, x, lab)
    want_loss, want = norm_ref.model_on_traversal(_traversal(fan, seeds), feats, labels, *_parts(model), EPS, N_NODES)
    _assert_close(got_loss, got.double().cpu(), want_loss, want, L)


def test_one_layer_is_bitwise_the_plain_step():
    feats, labels, perm = _node_data()
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    normed, plain = _model(1), _model(1, norm=None)
    plain.load_state_dict(normed.state_dict())
    from cslicer import aggr
    assert aggr.SageStep(normed, ROW_PAD, N_SLABS).norm is not None          # (csl_sage_fwd_bwd_norm is what runs)
    a = _native(normed, (4,), perm[:BATCH], x, lab)
    b = _native(plain, (4,), perm[:BATCH], x, lab)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


def test_native_step_refuses_bad_norm_arguments():
    """through the C ABI: eps <= 0, a missing gamma -- CSL_E_INVALID before anything is launched"""
    from cslicer import _abi, aggr
    feats, labels, perm = _node_data()
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    model = _model(2)
    model.norm_eps = 0.0
    with pytest.raises(_abi.CslError, match="norm: eps > 0"):
        _native(model, FANS[2], perm[:BATCH], x, lab)
    with pytest.raises(TypeError):
        aggr.SageRankStep(_model(2), ROW_PAD, N_SLABS, None)


# ---- trainers --------------------------------------------------------------------------------------------------------------

T_F, T_FAN = 16, (3, 3)


def _trainer(**kw):
    from cslicer.train import Trainer
    indptr, indices = _graph()
    feats, labels, perm = _node_data(F=T_F)
    t = Trainer(indptr, indices, feats, labels, CLASSES, fanouts=T_FAN, batch=BATCH, streams=2, hidden=HIDDEN, lr=1e-2,
                seed=3, **kw)
    t.set_nodes(perm)
    return t


def _params(t):
    return torch.cat([p.detach().reshape(-1) for p in t.model.parameters()]).cpu()


def _run4(**kw):
    t = _trainer(**kw)
    try:
        losses = t.run(4)
        return losses, _params(t), t.plan
    finally:
        t.close()


@pytest.fixture(scope="module")
def runs():
    return {"a": _run4(norm="layer", dropout=0.5), "b": _run4(norm="layer", dropout=0.5), "off": _run4(norm=None, dropout=0.5),
            "none": _run4(dropout=0.5)}


def test_equal_seeds_train_bit_for_bit(runs):
    assert runs["a"][2].path == "native"
    assert runs["a"][0] == runs["b"][0] and torch.equal(runs["a"][1], runs["b"][1])
    assert all(np.isfinite(runs["a"][0]))
    assert all(x != y for x, y in zip(runs["a"][0], runs["none"][0]))         # and the norm is not a no-op


def test_norm_none_is_the_trainer_without_the_argument(runs):
    assert runs["off"][0] == runs["none"][0] and torch.equal(runs["off"][1], runs["none"][1])
    assert runs["off"][2] == runs["none"][2]


def test_gamma_and_beta_are_parameters_behind_the_layers_and_never_decayed():
    t = _trainer(norm="layer", weight_decay=0.1, decay_bias=True)
    try:
        names = [n for n, _ in t.model.named_parameters()]
        assert names == ["convs.0.fc.weight", "convs.0.fc.bias", "convs.1.fc.weight", "convs.1.fc.bias", "norms.0.gamma",
                         "norms.0.beta"]
        assert [float(w) for w in t.opt.state_dict()["weight_decay"]] == [pytest.approx(0.1)] * 4 + [0.0, 0.0]
        assert t.native.grads.numel() == sum(p.numel() for p in t.model.parameters())
        assert t.checkpoint_fields()["norm"] == "layer"
    finally:
        t.close()


def _first_step(env, monkeypatch, **kw):
    """(loss, [gradient per parameter, float64]) of a trainer's first step under the environment / module switches `env`"""
    from cslicer import splitgnn
    for k, v in env.items():
        if k == "_NO_LOCAL_FUSE":
            monkeypatch.setattr(splitgnn, k, v)
        else:
            monkeypatch.setenv(k, v)
    t = _trainer(norm="layer", dropout=0.5, **kw)
    try:
        path = t.plan.path
        loss = float(t.run(1)[0])
        if t.native is not None:
            g, at, grads = t.native.grads.double().cpu(), 0, []
            for p in t.model.parameters():
                grads.append(g[at:at + p.numel()].reshape(p.shape))
                at += p.numel()
        else:
            grads = [p.grad.double().cpu() for p in t.model.parameters()]
        return path, loss, grads
    finally:
        t.close()


def test_native_step_against_the_autograd_steps_at_the_first_step(monkeypatch):
    """same minibatch, same weights, same masks: csl_sage_fwd_bwd_norm, CSLICER_PY_STEP=1 (splitgnn._SageModelLocal with the
    norm in place) and the `parts` path (a node per layer and aggr.LayerNormRelu), at the dropout test's agreement bound"""
    path_n, loss_n, g_n = _first_step({}, monkeypatch)
    assert path_n == "native"
    path_p, loss_p, g_p = _first_step({"CSLICER_PY_STEP": "1"}, monkeypatch)
    assert path_p == "local"
    path_q, loss_q, g_q = _first_step({"_NO_LOCAL_FUSE": True}, monkeypatch)
    assert path_q == "parts"
    for loss, grads in ((loss_p, g_p), (loss_q, g_q)):
        flat = torch.cat([g.reshape(-1) for g in g_n])
        # (the order of parameters() is the native step's layout: W_0, b_0, W_1, b_1, gamma_0, beta_0)
        _assert_close(loss_n, flat, loss, grads, 2)


# ---- the rank path, inference, checkpoints -------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _partition(world):
    return np.random.default_rng(11).integers(0, world, size=N_NODES).astype(np.int32)


EVAL_NODES = np.arange(0, N_NODES, 3)


def _rank_main(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "occ-gnn_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_gpu_norm as T
        from cslicer.train import Trainer
        indptr, indices = T._graph()
        feats, labels, perm = T._node_data(F=T.T_F)
        t = Trainer(indptr, indices, feats, labels, T.CLASSES, rank=rank, world=world, fanouts=T.T_FAN, batch=T.BATCH,
                    streams=1, hidden=T.HIDDEN, lr=1e-2, seed=3, dist=dist, rank_path=True,
                    workload=T._partition(world) if world > 1 else None, dropout=T.P, dropout_seed=T.SEED, norm="layer")
        assert t.plan.path == "parts" and t.native_rank is None and t.rank_path
        with torch.no_grad():
            for m in t.model.norms:       # (replicated: the same seed on every rank)
                torch.manual_seed(17)
                m.gamma.normal_(1.0, 0.5)
                m.beta.normal_(0, 0.3)
        weights = [p.detach().cpu().numpy().copy() for p in t.model.parameters()]
        t.set_nodes(perm)
        reduced = []
        t.on_reduced_grads = lambda flat: reduced.append(flat.detach().cpu().clone())
        loss = torch.tensor(t.run(1), dtype=torch.float64)
        dist.all_reduce(loss)           # the minibatch's loss = the sum of the ranks' shares
        # split inference of the stepped model: this rank's rows of EVAL_NODES, and the collective evaluation
        logits, mask, ev = t.predict(T.EVAL_NODES).cpu().numpy(), t.owns(T.EVAL_NODES), t.evaluate(T.EVAL_NODES)
        state = {k: v.detach().cpu() for k, v in t.model.state_dict().items()}
        t.close()
        dist.barrier()
        q.put((rank, float(loss[0]), reduced[0].numpy(), weights, logits, mask, ev, state))
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex)) + (None,) * 6)
        raise
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 1], ids=["two-ranks", "one-rank-on-the-rank-path"])
def test_ranks_sum_to_the_float64_model_and_infer_like_it(world):
    import torch.multiprocessing as mp
    from cslicer import splitgnn
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=150) for _ in range(world)], key=lambda x: x[0])
        for r_ in res:
            assert not isinstance(r_[1], str), r_[1]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for r_ in res:      # (all-reduced values, replicated weights: the same on every rank)
        assert r_[1] == res[0][1] and np.array_equal(r_[2], res[0][2])
        assert all(np.array_equal(a, b) for a, b in zip(r_[3], res[0][3]))
        assert r_[6] == res[0][6]
    feats, labels, perm = _node_data(F=T_F)
    w = res[0][3]
    want_loss, want = norm_ref.model_on_traversal(_traversal(T_FAN, perm[:BATCH]), feats, labels, w[0:4:2], w[1:4:2], w[4::2],
                                                  w[5::2], EPS, N_NODES, drop=(P, SEED, 0))       # the first step: counter 0
    _assert_close(res[0][1], torch.from_numpy(res[0][2]).double(), want_loss, want, 2, "world %d: " % world)
    # inference of the stepped model, split over the ranks, against float64
    model = splitgnn.DistSAGEModel(T_F, HIDDEN, CLASSES, n_layers=2, norm="layer", norm_eps=EPS)
    model.load_state_dict(res[0][7])
    indptr, indices = _graph()
    ref = norm_ref.infer_model(model, feats, indptr, indices, EVAL_NODES).numpy()
    cover = np.sum([r_[5] for r_ in res], axis=0)
    assert (cover == 1).all()
    for r_ in res:
        assert r_[4].shape == (int(r_[5].sum()), CLASSES)
        assert float(np.abs(r_[4] - ref[r_[5]]).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    want_ce = float(torch.nn.functional.cross_entropy(torch.from_numpy(ref), torch.from_numpy(labels[EVAL_NODES])))
    assert res[0][6]["n"] == len(EVAL_NODES) and abs(res[0][6]["loss"] - want_ce) <= 1e-5 * want_ce


@pytest.mark.parametrize("hidden,L", [(24, 3), (8, 2)], ids=["aggregate-first", "project-first"])
def test_whole_graph_inference_against_float64_and_a_checkpoint_round_trip(hidden, L, tmp_path):
    """hidden 24 >= 12 features: the aggregate-first form (a GEMM per chunk, then the norm); hidden 8 < 12: project-first
    (the norm behind the merge kernel); chunks of 257 rows and one chunk; a bfloat16 table bitwise its upcast; then
    save -> load -> predict"""
    from cslicer import checkpoint, infer, splitgnn
    indptr, indices = _graph()
    feats, labels, _ = _node_data()
    torch.manual_seed(hidden)
    model = splitgnn.DistSAGEModel(F0, hidden, CLASSES, n_layers=L, norm="layer", norm_eps=EPS).cuda()
    with torch.no_grad():
        for m in model.norms:
            m.gamma.normal_(1.0, 0.5)
            m.beta.normal_(0, 0.3)
    x = torch.from_numpy(feats).cuda()
    ref = norm_ref.infer_model(model, feats, indptr, indices, EVAL_NODES).numpy()
    try:
        a = infer.full_inference(model, indptr, indices, x, nodes=EVAL_NODES)
        b = infer.full_inference(model, indptr, indices, x, nodes=EVAL_NODES, chunk_rows=257)
        for got in (a, b):
            assert float(np.abs(got.cpu().numpy() - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))
        ev = infer.evaluate(model, indptr, indices, x, EVAL_NODES, labels)
        want_ce = float(torch.nn.functional.cross_entropy(torch.from_numpy(ref), torch.from_numpy(labels[EVAL_NODES])))
        assert ev["n"] == len(EVAL_NODES) and abs(ev["loss"] - want_ce) <= 1e-5 * want_ce
        t16 = x.to(torch.bfloat16)
        assert torch.equal(infer.full_inference(model, indptr, indices, t16, nodes=EVAL_NODES),
                           infer.full_inference(model, indptr, indices, t16.float(), nodes=EVAL_NODES))
        # the plain model with the same layers is another function
        plain = splitgnn.DistSAGEModel(F0, hidden, CLASSES, n_layers=L).cuda()
        plain.load_state_dict({k: v for k, v in model.state_dict().items() if k.startswith("convs.")})
        assert not torch.allclose(infer.full_inference(plain, indptr, indices, x, nodes=EVAL_NODES), a, atol=1e-3)
        path = str(tmp_path / "normed.pt")
        checkpoint.write(path, model)
        ck = checkpoint.read(path)
        assert ck["model"]["norm"] == "layer" and ck["model"]["norm_eps"] == pytest.approx(EPS)
        loaded = infer.load_model(path)
        assert loaded.norm == "layer" and [n for n, _ in loaded.named_parameters()] == [n for n, _ in model.named_parameters()]
        assert torch.equal(infer.full_inference(loaded, indptr, indices, x, nodes=EVAL_NODES), a)
        with pytest.raises(ValueError, match="norm"):
            checkpoint.check_model(ck["model"], checkpoint.model_block(plain))
    finally:
        infer.release(indptr, indices)


def test_trainer_checkpoint_round_trip_predicts_the_same(tmp_path):
    t = _trainer(norm="layer")
    u = _trainer(norm="layer")
    v = _trainer()
    try:
        t.run(2)
        path = str(tmp_path / "run.pt")
        t.save_checkpoint(path)
        u.load_checkpoint(path)
        assert u.steps_done == 2 and torch.equal(_params(t), _params(u))
        nodes = np.arange(0, N_NODES, 7)
        assert torch.equal(t.predict(nodes), u.predict(nodes)) and t.evaluate(nodes) == u.evaluate(nodes)
        with pytest.raises(ValueError, match="norm"):
            v.load_checkpoint(path)
    finally:
        for x in (t, u, v):
            x.close()
