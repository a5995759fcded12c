"""Split-parallel full-neighbour inference (cslicer.infer.full_inference_parts, csrc/infer_parts.hip) on the GPU: each
kernel against float64, a world of one against the single-process path (bitwise), two and three gloo ranks sharing the
GPU against float64 and the single-process path, agreement of the ranks on errors, evaluation leaving training
undisturbed, and the CLI's --eval-split with one process per part."""
import os
import socket

import numpy as np
import pytest
import torch

import infer_ref

pytestmark = pytest.mark.gpu

SEG = 512


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)) if want.size else 0.0


# ------------------------------------------------------------------ kernels, one process

def _sub_csr(lens, n_src, seed):
    rng = np.random.default_rng(seed)
    ip = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    return ip, rng.integers(0, n_src, int(ip[-1])).astype(np.int32)


LENS = [0, 1, SEG - 1, SEG, SEG + 1, 3 * SEG + 7, 5, 2, 9, 17, 40, 3, 0, 6]


def _run_part(kind, lens, W, pack, seed, H=1, D=4, slope=0.2, shift=0.0):
    """the partial kernel over a sub-CSR of rows `lens`, split into two calls (chunks), against float64"""
    from cslicer import aggr, infer
    dev = torch.device("cuda", 0)
    L = infer._lib()
    n_src = 300
    ip, ix = _sub_csr(lens, n_src, seed)
    w = infer.build_plan(ip)
    g = torch.Generator().manual_seed(seed)
    items, hubs = torch.from_numpy(w["items"]).to(dev), torch.from_numpy(w["hubs"]).to(dev)
    dip, dix = torch.from_numpy(ip.astype(np.int32)).to(dev), torch.from_numpy(ix).to(dev)
    n = len(lens)
    cut = n // 2
    chunks = []
    for s0, s1 in ((0, cut), (cut, n)):
        h0, h1 = (int(x) for x in np.searchsorted(w["hub_pos"], [s0, s1]))
        chunks.append((s0, s1, int(w["item_first"][s0]), int(w["item_first"][s1]), h0, h1, int(w["part_first"][s0]),
                       int(w["part_first"][s1] - w["part_first"][s0])))
    st = aggr._stream()
    if kind == "sage":
        ldy = W + 8
        y = (torch.rand((n_src, ldy), generator=g) * 2 - 1)
        yd = y.to(dev)
        send = torch.full((n, W), float("nan"), device=dev)
        for s0, s1, i0, i1, h0, h1, p0, npart in chunks:
            part = torch.empty((max(npart, 1), W), device=dev)
            rc = L.csl_infer_sage_part_f32(infer._ptr(dip), infer._ptr(dix), infer._ptr(items, 4 * i0), i1 - i0,
                                           infer._ptr(hubs, 4 * h0), h1 - h0, s0, p0, infer._ptr(yd, 4), ldy, W, pack,
                                           infer._ptr(part), infer._ptr(send, s0 * W), st)
            assert rc == 0
        torch.cuda.synchronize()
        yy = y.double()[:, 4:4 + W]
        want = torch.stack([yy[torch.from_numpy(ix[ip[i]:ip[i + 1]]).long()].sum(0) if lens[i] else
                            torch.zeros(W, dtype=torch.float64) for i in range(n)])
        got = send.cpu().double()
        live = [i for i in range(n) if lens[i]]             # rows without edges are not in a sub-CSR: untouched
        return _rel(got[live], want[live])
    C_ = H * D
    pld = int(L.csl_infer_gat_partial_ld(H, D))
    z = torch.rand((n_src, C_), generator=g) * 2 - 1
    el = torch.rand((n_src, H), generator=g) * 4 - 2 + shift
    er = torch.rand((n, H), generator=g) * 4 - 2 + shift
    zd, eld, erd = z.to(dev), el.to(dev), er.to(dev)
    send = torch.zeros((n, pld), device=dev)
    for s0, s1, i0, i1, h0, h1, p0, npart in chunks:
        part = torch.empty((max(npart, 1), pld), device=dev)
        rc = L.csl_infer_gat_part_f32(infer._ptr(dip), infer._ptr(dix), infer._ptr(items, 4 * i0), i1 - i0,
                                      infer._ptr(hubs, 4 * h0), h1 - h0, s0, p0, infer._ptr(zd), infer._ptr(eld),
                                      infer._ptr(erd, s0 * H), H, D, float(slope), pack, infer._ptr(part),
                                      infer._ptr(send, s0 * pld), st)
        assert rc == 0
    torch.cuda.synchronize()
    got = send.cpu().double()
    err = 0.0
    for i in range(n):
        if not lens[i]:
            continue
        src = torch.from_numpy(ix[ip[i]:ip[i + 1]]).long()
        sc = torch.nn.functional.leaky_relu(el[src] + er[i], slope).double()     # the kernel's float32 scores
        m_k = got[i, C_:C_ + H]                      # compare at the kernel's own stabiliser
        p = torch.exp(sc - m_k)
        s = p.sum(0)
        nn_ = (p[:, :, None] * z.double()[src].view(-1, H, D)).sum(0).reshape(-1)
        assert torch.equal(m_k, sc.max(0).values.float().double())
        err = max(err, _rel(got[i, C_ + H:C_ + 2 * H], s), _rel(got[i, :C_], nn_))
    return err


@pytest.mark.parametrize("W", [4, 24, 48, 100, 256])
@pytest.mark.parametrize("pack", [1, 2, 4])
def test_sage_part_kernel(W, pack):
    assert _run_part("sage", LENS, W, pack, seed=W + pack) <= 1e-5


@pytest.mark.parametrize("H,D", [(1, 4), (4, 8), (2, 32), (4, 32), (8, 32), (3, 100)])
@pytest.mark.parametrize("slope,shift", [(0.0, 0.0), (0.2, 120.0), (1.0, -120.0)])
def test_gat_part_kernel(H, D, slope, shift):
    for pack in (1, 4):
        assert _run_part("gat", LENS, None, pack, seed=H * D, H=H, D=D, slope=slope, shift=shift) <= 1e-5


def _merge_lists(n, P, seed):
    """destinations with 0, 1, 2 and P partials over a receive buffer of distinct rows, in rank order"""
    rng = np.random.default_rng(seed)
    ml = np.full((n, P), -1, dtype=np.int32)
    r = 0
    for i in range(n):
        k = [0, 1, min(2, P), P][i % 4]
        for q in sorted(rng.choice(P, k, replace=False)):
            ml[i, q] = r
            r += 1
    return ml, r


@pytest.mark.parametrize("W,proj", [(4, 0), (24, 0), (48, 1), (100, 0), (256, 1)])
def test_sage_merge_kernel(W, proj):
    from cslicer import aggr, infer
    dev = torch.device("cuda", 0)
    P, n, n_own = 3, 101, 60
    ml, R = _merge_lists(n, P, W)
    g = torch.Generator().manual_seed(W)
    recv = torch.rand((R, W), generator=g) * 2 - 1
    ldx = 2 * W if proj else W
    x = torch.rand((n_own, ldx), generator=g) * 2 - 1
    bias = torch.rand((W,), generator=g) - 0.5
    rng = np.random.default_rng(W)
    dst = np.stack([rng.integers(0, n_own, n), rng.integers(0, 30, n)], 1).astype(np.int32)
    dst[:, 1][(ml >= 0).sum(1) == 0] = 0
    ldo = W if proj else 2 * W
    out = torch.full((n, ldo), float("nan"), device=dev)
    # (every device buffer held until the kernel has run)
    dd, mld, rd_, xd, bd = (torch.from_numpy(dst).to(dev), torch.from_numpy(ml).to(dev), recv.to(dev), x.to(dev),
                            bias.to(dev))
    rc = infer._lib().csl_infer_sage_merge_f32(infer._ptr(dd), infer._ptr(mld), n, P, infer._ptr(rd_), infer._ptr(xd), ldx,
                                               W, proj, infer._ptr(bd) if proj else None, proj, infer._ptr(out), ldo,
                                               aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    rd = recv.double()
    acc = torch.stack([sum((rd[j] for j in ml[i] if j >= 0), torch.zeros(W, dtype=torch.float64)) for i in range(n)])
    mean = acc / torch.from_numpy(np.maximum(dst[:, 1], 1)).double()[:, None]
    self_ = x.double()[torch.from_numpy(dst[:, 0]).long(), :W]
    want = torch.relu(self_ + mean + bias.double()) if proj else torch.cat([self_, mean], 1)
    assert _rel(out.cpu(), want) <= 1e-5


@pytest.mark.parametrize("H,D,last,n_cls", [(1, 4, 0, 0), (4, 8, 1, 7), (2, 32, 0, 0), (4, 32, 1, 20), (8, 32, 0, 0),
                                            (8, 32, 1, 32)])
def test_gat_merge_kernel(H, D, last, n_cls):
    from cslicer import aggr, infer
    dev = torch.device("cuda", 0)
    L = infer._lib()
    P, n = 4, 97
    ml, R = _merge_lists(n, P, H * D)
    C_ = H * D
    pld = int(L.csl_infer_gat_partial_ld(H, D))
    g = torch.Generator().manual_seed(H + D)
    recv = torch.zeros((R, pld))
    recv[:, :C_] = torch.rand((R, C_), generator=g) * 2 - 1
    recv[:, C_:C_ + H] = torch.round((torch.rand((R, H), generator=g) * 240 - 120) * 8) / 8   # stabilisers +-120
    recv[:, C_ + H:C_ + 2 * H] = torch.rand((R, H), generator=g) * 3 + 0.5
    bias = torch.rand((C_,), generator=g) - 0.5
    width = n_cls if last else C_
    out = torch.full((n, width), float("nan"), device=dev)
    mld, rd_, bd = torch.from_numpy(ml).to(dev), recv.to(dev), bias.to(dev)     # held until the kernel has run
    rc = L.csl_infer_gat_merge_f32(infer._ptr(mld), n, P, infer._ptr(rd_), H, D, infer._ptr(bd), last, n_cls,
                                   infer._ptr(out), width, aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    rd = recv.double()
    want = []
    for i in range(n):
        rows = [j for j in ml[i] if j >= 0]
        if rows:
            m = torch.stack([rd[j, C_:C_ + H] for j in rows]).max(0).values
            s = sum(rd[j, C_ + H:C_ + 2 * H] * torch.exp(rd[j, C_:C_ + H] - m) for j in rows)
            nn_ = sum(rd[j, :C_].view(H, D) * torch.exp(rd[j, C_:C_ + H] - m)[:, None] for j in rows)
            y = nn_ / s[:, None] + bias.double().view(H, D)
        else:
            y = bias.double().view(H, D).clone()
        want.append(y.mean(0)[:n_cls] if last else torch.nn.functional.elu(y).reshape(-1))
    assert _rel(out.cpu(), torch.stack(want)) <= 1e-5


# ------------------------------------------------------------------ ranks (gloo, processes sharing the GPU)

def _hub_graph(n=3000, seed=0):
    """rows of 0 and 1 entries, a hub of 3,000 neighbours, rows around SEG, self loops and duplicates; the rest 0..16"""
    rng = np.random.default_rng(seed)
    degs = rng.integers(0, 17, n)
    degs[:5] = [0, 1, 3000, SEG, SEG + 1]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(degs, out=indptr[1:])
    indices = rng.integers(0, n, int(indptr[-1]))
    rows = np.repeat(np.arange(n), degs)
    sl = rng.random(indices.shape[0]) < 0.03
    indices[sl] = rows[sl]
    return indptr, indices


def _task(n=3000):
    indptr, indices = _hub_graph(n)
    rng = np.random.default_rng(3)
    feats = rng.random((n, 24), dtype=np.float32)
    labels = np.argmax(feats[:, :5], axis=1).astype(np.int64)
    return indptr, indices, feats, labels, rng.permutation(n)


def _table(n, world, kind):
    rng = np.random.default_rng(9)
    if kind == "mod":
        return None
    if kind == "tiny":                                   # three ranks, one with a tiny part
        return rng.choice(3, size=n, p=[0.55, 0.445, 0.005]).astype(np.int32)
    t = rng.integers(0, world - 1, n).astype(np.int32)   # "empty": the last rank owns nothing
    return t


def _worker(rank, world, port, q, scenario, kw):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "occ-gnn_amd"))
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_gpu_infer_parts import _SCENARIOS
        res = _SCENARIOS[scenario](rank, world, dist, **kw)
        dist.barrier()
        q.put((rank, res))
        dist.destroy_process_group()
    except BaseException as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: %s: %s" % (type(ex).__name__, ex)))
        raise


def _spawn(world, scenario, timeout=150, **kw):
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, scenario, kw)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=timeout) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    return [res[r] for r in range(world)]


def _trainer(rank, world, dist, kind, table, steps=3, rank_path=None):
    from cslicer.train import Trainer
    indptr, indices, feats, labels, perm = _task()
    wl = _table(indptr.shape[0] - 1, world, table)
    t = Trainer(indptr, indices, feats, labels, 5, rank=rank, world=world, fanouts=(10, 5), batch=256, streams=2,
                hidden=16, lr=1e-2, dist=dist, model="gat" if kind == "gat" else "sage", heads=2, workload=wl,
                feat_dim=feats.shape[1], rank_path=rank_path)
    t.set_nodes(perm)
    if steps:
        t.run(steps)
    return t, (indptr, indices, feats, labels, perm)


def _sc_world_of_one(rank, world, dist, kind):
    """rank_path=True with one part: bitwise the single-process path (GraphSAGE both forms, GAT, a hub row)"""
    from cslicer import infer, splitgnn
    indptr, indices, feats, labels, perm = _task()
    dev = torch.device("cuda", 0)
    torch.manual_seed(4)
    model = {"sage_agg": lambda: splitgnn.DistSAGEModel(24, 32, 5, n_layers=2),
             "sage_proj": lambda: splitgnn.DistSAGEModel(24, 12, 5, n_layers=3),
             "gat": lambda: splitgnn.DistGATModel(24, 8, 5, heads=4, n_layers=2)}[kind]().to(dev)
    comm = splitgnn.DistComm(device=dev)
    nodes = perm[:700]
    f = torch.from_numpy(feats).to(dev)
    for cr in (257, 1 << 16):
        a = infer.full_inference_parts(model, indptr, indices, f, comm, nodes=nodes, chunk_rows=cr)
        b = infer.full_inference(model, indptr, indices, f, nodes=nodes, chunk_rows=cr)
        assert torch.equal(a, b), (kind, cr, (a - b).abs().max().item())
    a = infer.full_inference_parts(model, indptr, indices, f, comm, chunk_rows=1000)
    assert torch.equal(a, infer.full_inference(model, indptr, indices, f, chunk_rows=1000))
    ea = infer.evaluate_parts(model, indptr, indices, f, comm, nodes, torch.from_numpy(labels).to(dev), chunk_rows=500)
    eb = infer.evaluate(model, indptr, indices, f, nodes, labels, chunk_rows=500)
    assert ea == eb, (ea, eb)
    # the Trainer with rank_path=True and one part
    t, _ = _trainer(rank, world, dist, "gat" if kind == "gat" else "sage", "mod", steps=2, rank_path=True)
    assert torch.equal(t.predict(nodes, chunk_rows=300), infer.full_inference(t.model, indptr, indices, t.feat,
                                                                              nodes=nodes, chunk_rows=300))
    assert t.evaluate(nodes) == infer.evaluate(t.model, indptr, indices, t.feat, nodes, labels)
    t.close()
    return "ok"


@pytest.mark.parametrize("kind", ["sage_agg", "sage_proj", "gat"])
def test_world_of_one_is_the_single_process_path(kind):
    assert _spawn(1, "world_of_one", kind=kind) == ["ok"]


def _sc_ranks(rank, world, dist, kind, table):
    """trained a few steps on the rank path; each rank's logits against float64 and single-process inference"""
    from cslicer import infer
    # (a rank that owns nothing does not train: the trainer's step is not what is tested here; its weights are the
    # replicated initial ones)
    t, (indptr, indices, feats, labels, perm) = _trainer(rank, world, dist, kind, table, steps=0 if table == "empty" else 3)
    nodes = np.concatenate([perm[:600], [0, 1, 2, 3, 4]])       # the hub and the rows around SEG among them
    a = t.predict(nodes)
    b = t.predict(nodes)
    assert torch.equal(a, b)                                    # bitwise reproducible
    c = t.predict(nodes, chunk_rows=257)
    mask = t.owns(nodes)
    assert a.shape == (int(mask.sum()), 5)
    want = infer_ref.model(t.model, torch.from_numpy(feats), indptr, indices, nodes=nodes[mask]).numpy()
    single = infer.full_inference(t.model, indptr, indices, feats, nodes=nodes[mask]) if mask.any() else None
    errs = [_rel(a.cpu(), want), _rel(c.cpu(), a.cpu()), _rel(a.cpu(), single.cpu()) if single is not None else 0.0]
    ev = t.evaluate(nodes)
    ref = infer.evaluate(t.model, indptr, indices, feats, nodes, labels)
    full = infer.full_inference(t.model, indptr, indices, feats, nodes=nodes).cpu()
    top2 = torch.topk(full, 2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-5).sum())
    t.close()
    return {"errs": errs, "mask": mask, "ev": ev, "ref": ref, "near": near, "own": t.n_own}


@pytest.mark.parametrize("world,kind,table", [(2, "sage", "mod"), (2, "gat", "mod"), (3, "sage", "tiny"),
                                              (3, "gat", "empty")],
                         ids=["two-ranks-sage", "two-ranks-gat", "three-ranks-tiny-part", "three-ranks-one-empty-gat"])
def test_ranks_match_float64_and_single_process(world, kind, table):
    res = _spawn(world, "ranks", kind=kind, table=table)
    for r in res:
        assert not isinstance(r, str), r
        assert r["errs"][0] <= 1e-5 and r["errs"][1] <= 1e-5 and r["errs"][2] <= 1e-5, r["errs"]
    # the ranks' rows cover the nodes exactly once
    cover = np.sum([r["mask"] for r in res], axis=0)
    assert (cover == 1).all()
    if table == "empty":
        assert res[-1]["own"] == 0
    evs = [r["ev"] for r in res]
    assert all(e == evs[0] for e in evs)                        # the same dict on every rank
    ref = res[0]["ref"]
    assert evs[0]["n"] == ref["n"]
    assert abs(evs[0]["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    if res[0]["near"] == 0:
        assert evs[0]["accuracy"] == ref["accuracy"]
    else:
        assert abs(evs[0]["accuracy"] - ref["accuracy"]) * ref["n"] <= res[0]["near"]


def _sc_errors(rank, world, dist):
    """a rank short of memory makes every rank raise MemoryError; different nodes make every rank raise ValueError"""
    from cslicer import infer
    t, (indptr, indices, feats, labels, perm) = _trainer(rank, world, dist, "sage", "mod", steps=1)
    out = []
    real, reserved = torch.cuda.mem_get_info, torch.cuda.memory_reserved
    if rank == 1:                                        # 1 KiB free, no cached blocks
        torch.cuda.mem_get_info = lambda dev=None: (1024, real(dev)[1])
        torch.cuda.memory_reserved = lambda dev=None: torch.cuda.memory_allocated(dev)
    try:
        t.predict(perm[:100])
        out.append("no error")
    except MemoryError:
        out.append("MemoryError")
    finally:
        torch.cuda.mem_get_info, torch.cuda.memory_reserved = real, reserved
    try:
        t.evaluate(perm[:100] if rank == 0 else perm[1:101])
        out.append("no error")
    except ValueError:
        out.append("ValueError")
    # afterwards the ranks are in step again
    out.append(t.evaluate(perm[:100])["n"])
    t.close()
    return out


def test_ranks_agree_on_errors():
    assert _spawn(2, "errors") == [["MemoryError", "ValueError", 100]] * 2


def _state(t):
    torch.cuda.synchronize()
    return {"params": [p.detach().clone() for p in t.model.parameters()],
            "adam": [(m.clone(), v.clone()) for m, v in t.opt.state], "adam_t": t.opt.t,
            "ring": None if getattr(t, "_loss_ring", None) is None else (t._loss_ring.clone(), t._ring_at),
            "totals": t.eng.totals(), "rng": (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())}


def _same(a, b):
    assert a["adam_t"] == b["adam_t"] and a["totals"] == b["totals"]
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a["adam"], b["adam"]))
    assert (a["ring"] is None) == (b["ring"] is None)
    if a["ring"] is not None:
        assert torch.equal(a["ring"][0], b["ring"][0]) and a["ring"][1] == b["ring"][1]
    assert torch.equal(a["rng"][0], b["rng"][0]) and torch.equal(a["rng"][1], b["rng"][1])


def _sc_undisturbed(rank, world, dist, kind):
    """evaluate() between two run() calls changes nothing a step reads: state bitwise, the next losses those of a twin"""
    losses = []
    for evaluate in (False, True):
        t, (indptr, indices, feats, labels, perm) = _trainer(rank, world, dist, kind, "mod", steps=4)
        if evaluate:
            before = _state(t)
            t.evaluate(perm[2400:])
            t.predict(perm[:50])
            _same(before, _state(t))
        losses.append(t.run(4))
        t.close()
    return losses


@pytest.mark.parametrize("kind", ["sage", "gat"])
def test_rank_path_evaluation_does_not_disturb_training(kind):
    for r in _spawn(2, "undisturbed", kind=kind):
        assert not isinstance(r, str), r
        np.testing.assert_allclose(r[1], r[0], rtol=1e-6)


def _sc_cli(rank, world, dist, path):
    import contextlib
    import io
    from cslicer import train
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", CSLICER_DIST_BACKEND="gloo")
    buf = io.StringIO()
    real_init = dist.init_process_group
    dist.init_process_group = lambda *a, **k: None           # the group is already up
    real_destroy = dist.destroy_process_group
    dist.destroy_process_group = lambda *a, **k: None
    try:
        with contextlib.redirect_stdout(buf):
            train.main(["--graph", path, "--eval-split", "holdout", "--eval-every", "1", "--num-epochs", "2",
                        "--fan-out", "5,5", "--num-layers", "2", "--batch-size", "256", "--max-steps", "3",
                        "--num-hidden", "32"])
    finally:
        dist.init_process_group, dist.destroy_process_group = real_init, real_destroy
    return buf.getvalue()


def test_cli_eval_split_with_two_ranks(tmp_path):
    from cslicer import l0
    indptr, indices, feats, labels, perm = _task()
    l0.write_l0(str(tmp_path / "h"), indptr, indices, features=feats, labels=labels, num_classes=5)
    out = _spawn(2, "cli", path=str(tmp_path / "h"))
    assert not out[0].startswith("error"), out[0]
    assert not out[1].startswith("error"), out[1]
    assert out[0].count("Eval Acc") == 2, out[0]
    assert "Eval Acc" not in out[1]


_SCENARIOS = {"world_of_one": _sc_world_of_one, "ranks": _sc_ranks, "errors": _sc_errors,
              "undisturbed": _sc_undisturbed, "cli": _sc_cli}
