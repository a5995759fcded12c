"""One rank of the split-parallel GraphSAGE step (csl_sage_rank_fwd_bwd_f32, csrc/sage_step.hip) pinned from outside:

* its collectives are UNIFORM: every rank enters the same exchanges in the same order whatever its own slice holds (a
  rank whose deepest slice has no boundary rows, or that owns nothing in the minibatch, used to skip the forward
  exchange of layer 0 while its peers entered it) -- checked in one process with a recording stand-in for the
  communicator, no process group, nothing that could hang;
* its numbers: the ranks' summed loss and gradients against tests/sage_ref.py (float64) on the ORACLE's traversal of the
  same seeds, ranks over gloo on one GPU (worlds of 2, 3 and 4, sequential and side-stream exchanges, backward by
  destination and by source, partitions that leave a rank without boundary rows and without any row);
* the branches it shares with the single-GPU step (row padding, weight-gradient slabs, hub lists by source, one to four
  layers, the deepest layer fused and not), which the widths above do not reach: a world of one over the table of
  tests/test_gpu_sage_step.py, against the same float64 model.

Tolerances (north_star, as tests/test_gpu_step_bench_widths.py): loss 1e-5 relative, every parameter gradient within 1e-4
of its largest entry.
"""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FAN = (4, 3)
F0, HIDDEN, CLASSES = 8, 16, 5
ROW_PAD, N_SLABS = 64, 4


def two_component_graph(n_a=240, n_b=120, deg=6, seed=5):
    """Component A = nodes [0, n_a) shared by parts 0 and 1, component B = [n_a, n_a + n_b) owned by part 2 alone; no edge
    between them.  Returns (indptr, indices, table)."""
    rng = np.random.default_rng(seed)
    n = n_a + n_b
    indptr = np.arange(n + 1, dtype=np.int64) * deg
    indices = np.empty(n * deg, dtype=np.int64)
    indices[:n_a * deg] = rng.integers(0, n_a, size=n_a * deg)
    indices[n_a * deg:] = rng.integers(n_a, n, size=n_b * deg)
    table = np.where(np.arange(n) < n_a, rng.integers(0, 2, size=n), 2).astype(np.int32)
    return indptr, indices, table


def two_component_minibatches(n_a=240, n_b=120):
    """(seeds from both components, seeds from A only)"""
    rng = np.random.default_rng(1)
    both = np.concatenate([rng.permutation(n_a)[:24], n_a + rng.permutation(n_b)[:8]])
    return both, rng.permutation(n_a)[:32]


def random_graph(n=3000, mean_deg=8, seed=2):
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 2 * mean_deg + 1, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)


def node_data(n, seed=4):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, F0)).astype(np.float32), rng.integers(0, CLASSES, size=n).astype(np.int64)


def case(name, world):
    """(indptr, indices, table, seeds) of a named case: every rank process and the parent build the same one"""
    if name.startswith("two-component"):
        indptr, indices, table = two_component_graph()
        assert world == 3
        both, a_only = two_component_minibatches()
        return indptr, indices, table, both if name.endswith("both") else a_only
    indptr, indices = random_graph()
    n = indptr.shape[0] - 1
    table = np.random.default_rng(11).integers(0, world, size=n).astype(np.int32)
    return indptr, indices, table, np.random.default_rng(3).permutation(n)[:96]


def make_model(L=2):
    from cslicer import splitgnn
    torch.manual_seed(0)
    model = splitgnn.DistSAGEModel(F0, HIDDEN, CLASSES, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    return model


def rank_inputs(indptr, indices, table, seeds, world, rank, by_source):
    """(engine, the rank's slices in MODEL order) of one minibatch: only this part is sliced (part_mask)"""
    from cslicer import _abi, splitgnn
    eng = _abi.Engine(indptr, indices, n_parts=world, fanouts=FAN, max_batch=128, n_streams=1, mode=_abi.MODE_GRAPH,
                      flags=_abi.FLAG_TRANSPOSE if by_source else 0, workload=table, part_mask=1 << rank)
    eng.submit_seeds([seeds])
    sl = splitgnn.slices_of(eng, parts=[rank])
    L = len(FAN)
    return eng, [sl[L - 1 - k][rank] for k in range(L)]


def run_step(step, slices, feats, labels, n_seeds):
    """one native call; returns the loss tensor (this rank's share)"""
    top, deep = slices[-1], slices[0]
    seeds = top.out_nodes[top.owned_out_nodes.long()] if top.n_owned else torch.zeros(0, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    step(slices, feats, deep.in_nodes, seeds, None, labels, 1.0 / n_seeds, loss)
    torch.cuda.synchronize()
    return loss


# ---- E: the call sequence, one process, a recording stand-in for the communicator -----------------------------------

class _RecordingComm(object):
    """what aggr.SageRankStep needs of a communicator: world, exchange_into, side_stream.  Records every exchange and
    hands back zeros for the received rows."""

    def __init__(self, world):
        self.world, self.calls, self.now, self._side = world, [], None, None

    def side_stream(self):
        if self._side is None:
            self._side = torch.cuda.Stream()
        return self._side

    def exchange_into(self, out, send_cat, send_counts, recv_counts):
        assert send_cat.shape[0] == sum(send_counts) and out.shape[0] == sum(recv_counts)
        self.calls.append(self.now + (tuple(send_counts), tuple(recv_counts)))
        out.zero_()
        return out


def _recording_step(aggr, model, comm, overlap):
    class Step(aggr.SageRankStep):
        def _exchange(self, user, layer, backward, src, dst, width, stream):
            self.comm.now = (int(layer), int(backward))
            return aggr.SageRankStep._exchange(self, user, layer, backward, src, dst, width, stream)
    return Step(model, ROW_PAD, N_SLABS, comm, overlap=overlap)


@pytest.mark.parametrize("overlap", [False, True], ids=["sequential", "side-stream"])
def test_every_rank_enters_the_same_exchanges_whatever_its_slice_holds(overlap):
    """Parts 0 and 1 share component A, part 2 owns all of component B.  Minibatch 1 (seeds from both): part 2's slices
    have no boundary rows ("local"); minibatch 2 (seeds from A): part 2 owns nothing.  All three parts must record the
    same sequence -- forward layers 0 .. L-1, then backward L-1 .. 1 -- because each exchange is an all_to_all_single
    that every rank of the group has to enter."""
    from cslicer import _abi, aggr
    _abi.load()
    indptr, indices, table = two_component_graph()
    feats_np, labels_np = node_data(indptr.shape[0] - 1)
    feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
    model = make_model()
    L = len(FAN)
    want_seq = [(k, 0) for k in range(L)] + [(k, 1) for k in range(L - 1, 0, -1)]
    for mb, seeds in enumerate(two_component_minibatches()):
        for g in range(3):
            eng, slices = rank_inputs(indptr, indices, table, seeds, 3, g, by_source=True)
            try:
                deep = slices[0]
                n_from, n_to = sum(deep.from_counts), sum(deep.to_counts)
                local = n_from == 0 and n_to == 0 and deep.n_owned == deep.n_out
                # the premise of the test, from the slices themselves
                if g == 2 and mb == 0:
                    assert local and deep.n_out > 0, "part 2 must be local in the minibatch with seeds of both components"
                    for s in slices:
                        # what the fused shortcut of the deepest layer relies on: the owned rows ARE the out rows, the
                        # true degree IS the CSR row length
                        assert torch.equal(s.owned_out_nodes.cpu(), torch.arange(s.n_out, dtype=torch.int32))
                        assert torch.equal(s.owned_degree.cpu(), s.indptr.cpu().diff().int())
                elif g == 2:
                    assert all(s.n_out == 0 and s.n_in == 0 for s in slices), "part 2 must be empty in the A-only minibatch"
                else:
                    assert not local and deep.n_out > 0 and n_from > 0 and n_to > 0, (g, mb)
                comm = _RecordingComm(3)
                step = _recording_step(aggr, model, comm, overlap)
                run_step(step, slices, feats, labels, len(seeds))
                got = [c[:2] for c in comm.calls]
                missing = [("layer %d %s" % (k, "backward" if b else "forward")) for k, b in want_seq if (k, b) not in got]
                assert got == want_seq, "rank %d, minibatch %d: exchanges %r, expected %r; missing: %s" % (
                    g, mb, got, want_seq, ", ".join(missing) or "none")
                for k, b, send, recv in comm.calls:
                    s = slices[k]
                    assert (send, recv) == ((tuple(s.to_counts), tuple(s.from_counts)) if b else
                                            (tuple(s.from_counts), tuple(s.to_counts)))
                assert bool(torch.isfinite(step.grads).all())
            finally:
                eng.close()


def test_a_world_of_one_starts_no_exchange():
    """with no peer the callback returns at once: the single-rank rate does not pay for empty collectives"""
    from cslicer import _abi, aggr
    _abi.load()
    indptr, indices = random_graph()
    n = indptr.shape[0] - 1
    feats_np, labels_np = node_data(n)
    feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
    seeds = np.random.default_rng(3).permutation(n)[:96]
    model = make_model()
    res = []
    for overlap in (False, True):
        eng, slices = rank_inputs(indptr, indices, None, seeds, 1, 0, by_source=True)
        comm = _RecordingComm(1)
        step = aggr.SageRankStep(model, ROW_PAD, N_SLABS, comm, overlap=overlap)
        loss = run_step(step, slices, feats, labels, len(seeds))
        assert comm.calls == []
        res.append((float(loss), step.grads.clone()))
        eng.close()
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    _check_against_float64(indptr, indices, seeds, feats_np, labels_np, model, res[0][0], res[0][1].double().cpu(), n)


# ---- D: the ranks' sum against float64 on the oracle's traversal -----------------------------------------------------

def _check_against_float64(indptr, indices, seeds, feats, labels, model, got_loss, got_grads, n, frontiers=None, fan=FAN):
    import sage_ref
    from oracle import oracle as orc
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
    if frontiers is not None:
        # the same sample: the ranks' owned rows add up to the oracle's frontier at every layer
        for l, rows in enumerate(frontiers):
            assert np.array_equal(np.sort(rows), np.sort(np.asarray(trav["frontier"][l]))), "frontier of hop %d" % l
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    want_loss, want = sage_ref.model_on_traversal(trav, feats, labels, ws, bs, n)
    print("loss %.9g (float64 %.9g)" % (got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    at = 0
    for k, g in enumerate(want):
        seg = got_grads[at:at + g.numel()].reshape(g.shape)
        at += g.numel()
        err, ref = float((seg - g).abs().max()), float(g.abs().max())
        print("gradient %d: max error %.3g, largest entry %.3g" % (k, err, ref))
        assert err <= 1e-4 * ref, "gradient %d (%s of layer %d): max error %.3g against a largest entry of %.3g" % (
            k, "weight" if k % 2 == 0 else "bias", k // 2, err, ref)
    assert at == got_grads.numel()


def _world_of_one_cases():
    """the single-GPU step's table (at most 256 classes: a rank has no separate column-sum pass), the slice by source
    present; and one row without it: the atomic fallback"""
    from test_gpu_sage_step import CASES
    return [c + (True,) for c in CASES if c[2] <= 256] + [(3, (5, 4, 3), 5, 64, 4, "random", True, False)]


@pytest.mark.parametrize("L,fan,classes,row_pad,n_slabs,graph,fused,by_source", _world_of_one_cases())
def test_a_world_of_one_matches_float64_on_the_oracle_traversal(L, fan, classes, row_pad, n_slabs, graph, fused, by_source,
                                                                monkeypatch):
    """The rank step where it runs the code it shares with the single-GPU step: no padding, padding to row_pad and to
    256, slabs that do and do not divide the rows, L = 1 .. 4, hub lists by source, the deepest layer fused and not."""
    from cslicer import _abi, aggr, splitgnn
    from test_gpu_sage_step import _graph
    _abi.load()
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    n, f0, hidden, B = 20000, 12, 24, 200
    indptr, indices = _graph(graph, n)
    rng = np.random.default_rng(7)
    feats_np = rng.standard_normal((n, f0)).astype(np.float32)
    labels_np = rng.integers(0, classes, size=n).astype(np.int64)
    seeds = rng.permutation(n)[:B]
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(f0, hidden, classes, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    eng = _abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=B, n_streams=1, mode=_abi.MODE_GRAPH,
                      flags=_abi.FLAG_TRANSPOSE if by_source else 0, part_mask=1)
    try:
        eng.submit_seeds([seeds])
        sl = splitgnn.slices_of(eng, parts=[0])
        slices = [sl[L - 1 - k][0] for k in range(L)]
        assert slices[-1].n_owned == B
        if graph == "hub" and L > 1:
            assert max(s.t_max_len for s in slices[1:]) > _abi.T_SORTED_MAX
        comm = _RecordingComm(1)
        step = aggr.SageRankStep(model, row_pad, n_slabs, comm)
        feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
        for _ in range(2):   # (the second call runs on the recorded GEMM plans and the reused workspace)
            loss = run_step(step, slices, feats, labels, B)
        assert comm.calls == []
        got_loss, got = float(loss), step.grads.double().cpu()
    finally:
        eng.close()
    _check_against_float64(indptr, indices, seeds, feats_np, labels_np, model, got_loss, got, n, fan=fan)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, q, name, overlap, by_source):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "occ-gnn_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cslicer import _abi, aggr, splitgnn
        import test_gpu_sage_rank as T
        _abi.load()
        indptr, indices, table, seeds = T.case(name, world)
        feats_np, labels_np = T.node_data(indptr.shape[0] - 1)
        feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
        model = T.make_model()
        eng, slices = T.rank_inputs(indptr, indices, table, seeds, world, rank, by_source)
        step = aggr.SageRankStep(model, T.ROW_PAD, T.N_SLABS, splitgnn.DistComm(device=torch.device("cuda", 0)),
                                 overlap=overlap)
        loss = T.run_step(step, slices, feats, labels, len(seeds))     # one step, no optimizer
        grads, loss = step.grads.cpu(), loss.cpu()
        dist.all_reduce(grads)
        dist.all_reduce(loss)
        L = len(T.FAN)
        owned = [slices[L - 1 - l].out_nodes[slices[L - 1 - l].owned_out_nodes.long()].cpu().numpy() for l in range(L)]
        eng.close()
        dist.barrier()
        q.put((rank, float(loss), grads.numpy(), owned))
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex), None, None))
        raise
    dist.destroy_process_group()


@pytest.mark.parametrize("world,name,overlap,by_source", [
    (2, "random", False, True), (2, "random", True, False),
    (3, "two-component-both", False, True), (3, "two-component-both", True, False),
    (3, "two-component-a-only", True, True), (3, "two-component-a-only", False, False),
    (4, "random", True, True), (4, "random", False, False)])
def test_ranks_sum_to_the_float64_model_on_the_oracle_traversal(world, name, overlap, by_source):
    import torch.multiprocessing as mp
    from cslicer import _abi
    _abi.load()
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q, name, overlap, by_source)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        # one tiny step per rank: the time is the interpreter start, the imports and the engine, a minute at the most
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
    indptr, indices, table, seeds = case(name, world)
    n = indptr.shape[0] - 1
    feats_np, labels_np = node_data(n)
    L = len(FAN)
    frontiers = [np.concatenate([r_[3][l] for r_ in res]) for l in range(L)]
    for rank, loss, grads, _ in res:           # (an all-reduced value: the same on every rank)
        assert loss == res[0][1] and np.array_equal(grads, res[0][2])
    _check_against_float64(indptr, indices, seeds, feats_np, labels_np, make_model(), res[0][1],
                           torch.from_numpy(res[0][2]).double(), n, frontiers)
