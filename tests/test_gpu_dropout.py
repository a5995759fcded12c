"""Dropout between the GraphSAGE layers on the GPU (include/cslicer_dropout.h, csrc/dropout.hip):

* csl_dropout_f32 against the numpy mask of tests/dropout_ref.py, bit for bit, at the shapes where its launch changes
  (a row on 1, 32 and 64 lanes; less than, exactly and more than a workgroup of rows), strided and in place;
* aggr.Dropout's backward = the same map on the gradient;
* the native step (csl_sage_fwd_bwd_dropout) at p = 0.5 against the float64 model with the same masks;
* trainers: determinism, the seed, dropout = 0, native against the autograd step, evaluation untouched;
* the rank path (autograd rank step over gloo): the ranks' sum against the single-process float64 model -- a node's mask
  is keyed by its id, so it is the same whatever part computes the row.

Tolerances: loss 1e-5 relative, every parameter gradient within 1e-4 of its largest entry; the mask itself
and everything said to be "the same run" bit for bit.
"""
import os
import socket

import numpy as np
import pytest
import torch

import dropout_ref

pytestmark = pytest.mark.gpu

SENTINEL = -77.25


# ---- the kernel ----------------------------------------------------------------------------------------------------------

def _ids(n, rng):
    """distinct non-negative int32 node ids in no order, the largest one 2^31 - 1"""
    ids = rng.permutation(1 << 20)[:n].astype(np.int64) * 2047 + 5
    ids[rng.integers(0, n)] = (1 << 31) - 1
    return ids


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("H", [4, 100, 256])
def test_kernel_is_the_numpy_mask_bit_for_bit(H, n):
    from cslicer import aggr
    rng = np.random.default_rng(H * 10007 + n)
    ids_np = _ids(n, rng)
    ids = torch.from_numpy(ids_np.astype(np.int32)).cuda()
    x_np = rng.standard_normal((n, H)).astype(np.float32)
    x_np[rng.random((n, H)) < 0.1] = 0.0
    x = torch.from_numpy(x_np).cuda()
    # (p, seed, layer, step, keyed by ids): a seed with a high word, a step >= 2^32, two layers, two steps
    cases = [(0.1, 12345, 0, 0, True), (0.5, (0x9abcdef1 << 32) | 77, 1, 7, True), (0.9, 3, 0, (1 << 32) + 5, True),
             (0.5, (0x9abcdef1 << 32) | 77, 0, 7, True), (0.5, (0x9abcdef1 << 32) | 77, 1, 8, True), (0.5, 9, 2, 1, False)]
    outs = {}
    for p, seed, layer, step, keyed in cases:
        want = dropout_ref.apply(x_np, ids_np if keyed else np.arange(n), p, seed, layer, step)
        got = aggr.dropout(x, ids if keyed else None, p, seed, layer, step)
        assert got.data_ptr() != x.data_ptr() and torch.equal(x.cpu(), torch.from_numpy(x_np))      # out of place
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (p, seed, layer, step, keyed)
        outs[(p, seed, layer, step)] = want
    a = outs[(0.5, (0x9abcdef1 << 32) | 77, 1, 7)]
    if n * H >= 64:     # (another layer, another step: another mask)
        assert not np.array_equal(a, outs[(0.5, (0x9abcdef1 << 32) | 77, 0, 7)])
        assert not np.array_equal(a, outs[(0.5, (0x9abcdef1 << 32) | 77, 1, 8)])
    # leading dimensions beyond H, sentinels all around the block; out of place into a strided block, then in place
    p, seed, layer, step = 0.5, (0x9abcdef1 << 32) | 77, 1, 7
    ld = H + 8
    src = torch.full((n + 2, ld), SENTINEL, device="cuda")
    dst = torch.full((n + 2, ld), SENTINEL, device="cuda")
    src[1:n + 1, 4:4 + H] = x
    keep_out = torch.ones((n + 2, ld), dtype=torch.bool)
    keep_out[1:n + 1, 4:4 + H] = False
    got = aggr.dropout(src[1:n + 1, 4:4 + H], ids, p, seed, layer, step, out=dst[1:n + 1, 4:4 + H])
    assert got.data_ptr() == dst[1:n + 1, 4:4 + H].data_ptr()
    assert np.array_equal(dst[1:n + 1, 4:4 + H].cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert bool((dst.cpu()[keep_out] == SENTINEL).all()) and torch.equal(src[1:n + 1, 4:4 + H].cpu(), x.cpu())
    aggr.dropout(src[1:n + 1, 4:4 + H], ids, p, seed, layer, step, out=src[1:n + 1, 4:4 + H])
    assert np.array_equal(src[1:n + 1, 4:4 + H].cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert bool((src.cpu()[keep_out] == SENTINEL).all())
    # in place on a contiguous matrix
    y = x.clone()
    aggr.dropout(y, ids, p, seed, layer, step, out=y)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), a.view(np.uint32))


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from cslicer import _abi, aggr
    x = torch.zeros((8, 8), device="cuda")
    ids = torch.arange(8, dtype=torch.int32, device="cuda")
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(_abi.CslError):
            aggr.dropout(x, ids, bad, 1, 0, 0)
    with pytest.raises(_abi.CslError):
        aggr.dropout(torch.zeros((8, 6), device="cuda"), ids, 0.5, 1, 0, 0)
    with pytest.raises(ValueError):
        aggr.dropout(x, ids[:5], 0.5, 1, 0, 0)
    with pytest.raises(TypeError):
        aggr.dropout(x.double(), ids, 0.5, 1, 0, 0)
    assert aggr.dropout(x[:0], ids[:0], 0.5, 1, 0, 0).shape == (0, 8)


def test_autograd_node_backward_is_the_map_of_the_gradient():
    from cslicer import aggr
    rng = np.random.default_rng(1)
    n, H = 130, 36
    ids_np = _ids(n, rng)
    ids = torch.from_numpy(ids_np.astype(np.int32)).cuda()
    x_np, g_np = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((n, H)).astype(np.float32)
    x = torch.from_numpy(x_np).cuda().requires_grad_()
    y = aggr.Dropout.apply(x, ids, 0.5, 11, 1, 3)
    # no mask is saved, the backward recomputes it: the node keeps the int32 ids alone
    assert [(t.dtype, tuple(t.shape)) for t in y.grad_fn.saved_tensors] == [(torch.int32, (n,))]
    y.backward(torch.from_numpy(g_np).cuda())
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint32),
                          dropout_ref.apply(x_np, ids_np, 0.5, 11, 1, 3).view(np.uint32))
    assert np.array_equal(x.grad.cpu().numpy().view(np.uint32),
                          dropout_ref.apply(g_np, ids_np, 0.5, 11, 1, 3).view(np.uint32))


# ---- the native step -------------------------------------------------------------------------------------------------------

N_NODES, F0, HIDDEN, CLASSES, BATCH = 2000, 12, 24, 5, 64
ROW_PAD, N_SLABS = 64, 4
P, SEED, STEP = 0.5, (5 << 32) | 4242, 3


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


def _model(L, F=F0):
    from cslicer import splitgnn
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(F, HIDDEN, CLASSES, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    return model


def _native(model, fan, seeds, feats, labels, drop):
    """(loss, flat gradients) of one native step on a fresh engine's first sample"""
    from cslicer import _abi, aggr, splitgnn
    L = len(fan)
    indptr, indices = _graph()
    eng = _abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=BATCH, mode=_abi.MODE_GRAPH,
                      flags=_abi.FLAG_TRANSPOSE)
    try:
        eng.submit_seeds([seeds])
        slices = splitgnn.slices_of(eng)
        order = [slices[L - 1 - k][0] for k in range(L)]
        step = aggr.SageStep(model, ROW_PAD, N_SLABS)
        loss = torch.zeros(1, device="cuda")
        for _ in range(2):     # (the second call runs on the recorded GEMM plans and the reused workspace)
            step(order, feats, labels, 1.0 / len(seeds), loss, drop)
        torch.cuda.synchronize()
        return float(loss[0]), step.grads.clone()
    finally:
        eng.close()


def _assert_close(got_loss, got_grads, want_loss, want, what=""):
    print("%sloss %.9g (float64 %.9g)" % (what, got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    at = 0
    for k, g in enumerate(want):
        seg = got_grads[at:at + g.numel()].reshape(g.shape)
        at += g.numel()
        err, ref = float((seg - g).abs().max()), float(g.abs().max())
        print("%sgradient %d: max error %.3g, largest entry %.3g" % (what, k, err, ref))
        assert ref > 0 and err <= 1e-4 * ref, "gradient %d (%s of layer %d): max error %.3g against a largest entry of %.3g" % (
            k, "weight" if k % 2 == 0 else "bias", k // 2, err, ref)
    assert at == got_grads.numel()


@pytest.mark.parametrize("fused", [True, False], ids=["fused-deepest-layer", "no-mfma-fwd"])
@pytest.mark.parametrize("fan", [(3, 3), (3, 3, 2)], ids=["L2", "L3"])
def test_native_step_matches_float64_with_the_same_masks(fan, fused, monkeypatch):
    from cslicer import aggr
    from oracle import oracle as orc
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    assert (aggr._lib().csl_sage_fwd_mfma_scratch(F0, HIDDEN) > 0)       # these widths are the fused layer's
    L = len(fan)
    feats, labels, perm = _node_data()
    seeds = perm[:BATCH]
    model = _model(L)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    got_loss, got = _native(model, fan, seeds, x, lab, aggr.DropSpec(P, SEED, STEP))
    indptr, indices = _graph()
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    want_loss, want = dropout_ref.model_on_traversal(trav, feats, labels, ws, bs, N_NODES, P, SEED, STEP)
    _assert_close(got_loss, got.double().cpu(), want_loss, want)
    # and it IS dropout: the same step without it is another loss
    plain_loss, _ = _native(model, fan, seeds, x, lab, None)
    assert abs(plain_loss - got_loss) > 1e-3 * abs(plain_loss)


def test_one_layer_has_nothing_to_drop():
    from cslicer import aggr
    feats, labels, perm = _node_data()
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    model = _model(1)
    a = _native(model, (4,), perm[:BATCH], x, lab, aggr.DropSpec(P, SEED, STEP))
    b = _native(model, (4,), perm[:BATCH], x, lab, None)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


def test_bfloat16_table_is_its_float32_upcast_with_the_same_masks():
    from cslicer import aggr
    feats, labels, perm = _node_data()
    t16 = torch.from_numpy(feats).to(torch.bfloat16).cuda()
    lab = torch.from_numpy(labels).cuda()
    model = _model(3)
    drop = aggr.DropSpec(P, SEED, STEP)
    a = _native(model, (3, 3, 2), perm[:BATCH], t16, lab, drop)
    b = _native(model, (3, 3, 2), perm[:BATCH], t16.float(), lab, drop)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


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
    """four steps of: two trainers with dropout 0.5 and equal seeds, one with another dropout_seed, one with dropout=0.0,
    one built without the argument"""
    return {"a": _run4(dropout=0.5), "b": _run4(dropout=0.5), "c": _run4(dropout=0.5, dropout_seed=99),
            "zero": _run4(dropout=0.0), "none": _run4()}


def test_equal_seeds_train_bit_for_bit(runs):
    assert runs["a"][2].path == "native"
    assert runs["a"][0] == runs["b"][0] and torch.equal(runs["a"][1], runs["b"][1])
    assert all(np.isfinite(runs["a"][0]))


def test_another_dropout_seed_is_another_run(runs):
    assert all(x != y for x, y in zip(runs["a"][0], runs["c"][0]))
    assert all(x != y for x, y in zip(runs["a"][0], runs["none"][0]))         # and dropout is not a no-op


def test_dropout_zero_is_the_trainer_without_the_argument(runs):
    assert runs["zero"][0] == runs["none"][0] and torch.equal(runs["zero"][1], runs["none"][1])
    assert runs["zero"][2] == runs["none"][2]


def test_native_step_against_the_autograd_step_at_the_first_step(monkeypatch):
    """same minibatch, same weights, same masks: the native step (csl_sage_fwd_bwd_dropout) and CSLICER_PY_STEP=1
    (splitgnn._SageModelLocal with its in-place drop, torch's GEMMs)"""
    t = _trainer(dropout=0.5)
    try:
        assert t.native is not None
        loss_n = t.run(1)[0]
        grads_n = t.native.grads.double().cpu()
    finally:
        t.close()
    monkeypatch.setenv("CSLICER_PY_STEP", "1")
    t = _trainer(dropout=0.5)
    try:
        assert t.native is None and t.plan.path == "local"
        loss_p = t.run(1)[0]
        want = []
        for conv in t.model.convs:
            want += [conv.fc.weight.grad.double().cpu(), conv.fc.bias.grad.double().cpu()]
    finally:
        t.close()
    _assert_close(loss_n, grads_n, loss_p, want)


def test_evaluation_never_drops():
    """evaluate on a trainer with dropout = 0.5 == evaluate on a dropout = 0 trainer holding the same parameters"""
    t = _trainer(dropout=0.5)
    u = _trainer()
    try:
        t.run(2)
        u.model.load_state_dict(t.model.state_dict())
        nodes = np.arange(0, N_NODES, 3)
        a, b = t.evaluate(nodes), u.evaluate(nodes)
        assert a == b and a["n"] == len(nodes) and np.isfinite(a["loss"])
        assert torch.equal(t.predict(nodes), u.predict(nodes))
    finally:
        t.close()
        u.close()


# ---- the rank path ---------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _partition(world):
    return np.random.default_rng(11).integers(0, world, size=N_NODES).astype(np.int32)


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
        import test_gpu_dropout as T
        from cslicer.train import Trainer
        indptr, indices = T._graph()
        feats, labels, perm = T._node_data(F=T.T_F)
        t = Trainer(indptr, indices, feats, labels, T.CLASSES, rank=rank, world=world, fanouts=T.T_FAN, batch=T.BATCH,
                    streams=1, hidden=T.HIDDEN, lr=1e-2, seed=3, dist=dist, rank_path=True,
                    workload=T._partition(world) if world > 1 else None, dropout=T.P, dropout_seed=T.SEED)
        assert t.plan.path == "parts" and t.native_rank is None and t.rank_path
        weights = [p.detach().cpu().numpy().copy() for p in t.model.parameters()]
        t.set_nodes(perm)
        reduced = []
        t.on_reduced_grads = lambda flat: reduced.append(flat.detach().cpu().clone())
        loss = torch.tensor(t.run(1), dtype=torch.float64)
        dist.all_reduce(loss)           # the minibatch's loss = the sum of the ranks' shares
        t.close()
        dist.barrier()
        q.put((rank, float(loss[0]), reduced[0].numpy(), weights))
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex), None, None))
        raise
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 1], ids=["two-ranks", "one-rank-on-the-rank-path"])
def test_ranks_sum_to_the_float64_model_with_the_same_masks(world):
    import torch.multiprocessing as mp
    from oracle import oracle as orc
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
    for rank, loss, grads, weights in res:      # (all-reduced values, replicated weights: the same on every rank)
        assert loss == res[0][1] and np.array_equal(grads, res[0][2])
        assert all(np.array_equal(a, b) for a, b in zip(weights, res[0][3]))
    indptr, indices = _graph()
    feats, labels, perm = _node_data(F=T_F)
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=T_FAN).sample(perm[:BATCH])
    ws, bs = res[0][3][0::2], res[0][3][1::2]
    # the trainer's first step: counter 0
    want_loss, want = dropout_ref.model_on_traversal(trav, feats, labels, ws, bs, N_NODES, P, SEED, 0)
    _assert_close(res[0][1], torch.from_numpy(res[0][2]).double(), want_loss, want, "world %d: " % world)
