"""Correct and Smooth on the GPU: csl_prop_f32 through the C ABI against tests/smooth_ref.py at every
dispatch edge, cslicer.smooth.propagate along a trajectory, correct_and_smooth / label_propagation end to end, and the
trainer's and the command line's paths.

One step.  Every element of `out` and `out_s` is compared with the float64 step on the same float32 inputs; the error
over the DERIVED bound of smooth_ref.step (d + 2 roundings counted in the kernel on the gathered term, one more for alpha
itself becoming a float32: gamma(d + 3), the constant the design states) must be at most 1.  W takes both sides of every groups_for step and one column tile beyond 64 float4s;
the rows take degree 0, 1, 2, 63, 64, 65, the lengths either side of a wave's G * U edges per step, 511, 512 (one item),
513, 600 (hubs of 2 parts) and 1025 (3 parts); the plan is over the rows in shuffled order (row != position), cut whole,
into chunks of 7 (a hub first in a chunk, one last, pos0 and part0 non-zero) and of 1, which must give the same bits.

Trajectory.  For a symmetric graph ||S||_2 <= 1 and clamp and reset are 1-Lipschitz, so
    ||X_T^gpu - X_T^ref||_F <= alpha^T ||B_-1||_F + sum_{t < T} alpha^(T - 1 - t) ||B_t||_F
with B_t the one-step bound on the float64 iterate plus the rounding of the pre-scaled operand handed on (smooth_ref.prop),
B_-1 the rounding of the first operand, all inflated by 1.001 for the second-order terms.

Largest error over bound seen on an MI355X: one step 0.44 (W = 256), trajectory 0.002; largest element difference end
to end 4.0e-7 (each test prints its own figures)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import smooth_ref as R

pytestmark = pytest.mark.gpu

S = -7777.0
WIDTHS = [4, 8, 12, 16, 20, 32, 36, 48, 64, 68, 128, 132, 256, 260]
U = 8
# (alpha, beta, base?, lo, hi, out?, out_s?): both outputs and no clamp; `out` alone, no base, a clamp that bites (its ends are
# float32 numbers: the bound has no term for rounding them); `out_s` alone
CONFIGS = {"both": (0.8, 0.2, True, -np.inf, np.inf, True, True), "out": (0.5, 0.0, False, -2.0 ** -9, 2.0 ** -8, True, False),
           "out_s": (1.0, -0.5, True, -np.inf, np.inf, False, True)}


def _groups_for(c4):
    lg = 4
    while lg < 64 and lg < c4:
        lg <<= 1
    return 64 // lg


@functools.lru_cache(maxsize=None)
def _graph(W):
    """rows of every length the kernel switches on, hubs at positions 3 (first of no chunk), 7 (first of a chunk of 7) and
    13 (last of one), rows in shuffled order"""
    from cslicer import infer
    step = _groups_for(W // 4) * U
    lens = sorted({0, 1, 2, 63, 64, 65, 511, 512, max(step - 1, 0), step, step + 1, 3, 9, 17, 100, 0, 5})
    order = lens[:3] + [513] + lens[3:6] + [600] + lens[6:11] + [1025] + lens[11:] + [0, 7]
    assert order[3] == 513 and order[7] == 600 and order[13] == 1025
    n = len(order)
    rng = np.random.default_rng(W)
    rows = rng.permutation(n).astype(np.int64)                 # position k holds graph row rows[k]
    glens = np.zeros(n, dtype=np.int64)
    glens[rows] = order
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(glens, out=ip[1:])
    ix = rng.integers(0, n, int(ip[-1])).astype(np.int32)
    plan = infer.build_plan(ip, rows)
    assert plan["hubs"][:, 3].tolist() == [2, 2, 3] and plan["hub_pos"].tolist() == [3, 7, 13]
    assert np.count_nonzero(plan["items"][:, 0] != plan["items"][:, 1]) > n // 2
    ch = infer.plan_chunks(plan, 7)
    assert ch[1].k0 == 7 and ch[1].part0 == 2 and ch[1].h1 - ch[1].h0 == 2 and ch[1].k1 == 14     # hub first and last
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("ip", ip.astype(np.int32)), ("ix", ix), ("items", plan["items"]),
                                                      ("hubs", plan["hubs"]))}
    return {"ip": ip, "ix": ix, "rows": rows, "n": n, "plan": plan, "dev": dev, "dinv": R.dinv32(ip)}


def _inputs(W, n, nan_row=None):
    rng = np.random.default_rng(100 + W)
    ldx, ldb = W + 4, W + 8
    xs = np.full((n, ldx), S, dtype=np.float32)
    xs[:, :W] = rng.standard_normal((n, W)).astype(np.float32) * 0.01
    if nan_row is not None:
        xs[nan_row, :W] = np.nan
    base = np.full((n, ldb), S, dtype=np.float32)
    base[:, :W] = rng.standard_normal((n, W)).astype(np.float32) * 0.1
    return xs, ldx, base, ldb


def _run(g, W, cfg, chunk_rows, xs, ldx, base, ldb):
    """the plan of g through csl_prop_f32 in chunks of chunk_rows; (out, out_s) as host arrays with their sentinels"""
    from cslicer import infer, smooth
    alpha, beta, use_base, lo, hi, want_out, want_s = cfg
    L = smooth._abi.load()
    n, d = g["n"], g["dev"]
    ldo, ldos = W + 4, W + 12
    dxs, dbase, ddinv = torch.from_numpy(xs).cuda(), torch.from_numpy(base).cuda(), torch.from_numpy(g["dinv"]).cuda()
    out = torch.full((n, ldo), S, dtype=torch.float32, device="cuda")
    out_s = torch.full((n, ldos), S, dtype=torch.float32, device="cuda")
    nul = C.c_void_p(0)
    for c in infer.plan_chunks(g["plan"], chunk_rows):
        part = torch.full((max(c.n_parts, 1) + 2, W), S, dtype=torch.float32, device="cuda")
        rc = L.csl_prop_f32(*infer._list_args(d["ip"], d["ix"], d["items"], d["hubs"], c, c.k0), infer._ptr(dxs), ldx, W,
                            infer._ptr(ddinv), alpha, infer._ptr(dbase, c.k0 * ldb) if use_base else nul, ldb, beta,
                            float(lo), float(hi), infer._ptr(part, W) if c.n_parts else nul,
                            infer._ptr(out, c.k0 * ldo) if want_out else nul, ldo,
                            infer._ptr(out_s, c.k0 * ldos) if want_s else nul, ldos, nul)
        assert rc == 0
        part = part.cpu().numpy()
        assert (part[0] == S).all() and (part[1 + c.n_parts:] == S).all()          # the partial rows of this call only
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_s.cpu().numpy()


def _reference(g, W, cfg, xs, ldx, base, ldb):
    alpha, beta, use_base, lo, hi, _, _ = cfg
    return R.step(g["ip"], g["ix"], g["rows"], xs.reshape(-1), ldx, W, g["dinv"], alpha, base.reshape(-1) if use_base else None,
                  ldb, beta, lo, hi)


@pytest.mark.parametrize("W", WIDTHS)
def test_one_step_within_the_derived_bound_at_every_edge(W):
    g = _graph(W)
    xs, ldx, base, ldb = _inputs(W, g["n"])
    worst = 0.0
    for name, cfg in CONFIGS.items():
        y, ys, by, bs = _reference(g, W, cfg, xs, ldx, base, ldb)
        if name == "out":
            assert (y == cfg[3]).any() and (y == cfg[4]).any() and ((y > cfg[3]) & (y < cfg[4])).any()      # the clamp bites
        whole = _run(g, W, cfg, g["n"], xs, ldx, base, ldb)
        again = _run(g, W, cfg, g["n"], xs, ldx, base, ldb)
        for ways in (7, 1):
            cut = _run(g, W, cfg, ways, xs, ldx, base, ldb)
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(whole, cut)), (name, ways)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(whole, again)), name
        for got, want, bound, on in ((whole[0], y, by, cfg[5]), (whole[1], ys, bs, cfg[6])):
            assert (got[:, W:] == S).all(), name                        # columns [W, ld) untouched
            if not on:
                assert (got == S).all(), name                           # a null output: nothing written anywhere
                continue
            assert np.isfinite(got[:, :W]).all()
            ratio = float((np.abs(got[:, :W].astype(np.float64) - want) / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, ratio)
    print("W = %d: largest error over the derived bound %.3f" % (W, worst))


@pytest.mark.parametrize("W", [4, 48, 260])
def test_a_nan_row_shows_in_exactly_the_rows_that_gather_it(W):
    g = _graph(W)
    nan_row = int(g["ix"][g["ip"][g["rows"][13]]])              # a source of the 3-part hub
    xs, ldx, base, ldb = _inputs(W, g["n"], nan_row)
    out, out_s = _run(g, W, (0.8, 0.2, True, -0.05, 0.1, True, True), 7, xs, ldx, base, ldb)
    gathers = np.array([nan_row in g["ix"][g["ip"][r]:g["ip"][r + 1]] for r in g["rows"]])
    assert gathers.any() and not gathers.all()
    for got in (out, out_s):
        assert np.isnan(got[gathers, :W]).all() and np.isfinite(got[~gathers, :W]).all()


def test_one_node_without_edges():
    from cslicer import infer, smooth
    L = smooth._abi.load()
    plan = infer.build_plan(np.zeros(2, dtype=np.int64))
    assert plan["items"].tolist() == [[0, 0, 0, -1]]
    ip, ix = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    items = torch.from_numpy(plan["items"]).cuda()
    xs = torch.full((1, 4), 3.0, device="cuda")
    base = torch.tensor([[0.5, -2.0, 8.0, 0.0]], device="cuda")
    dinv = torch.zeros(1, device="cuda")
    out, out_s = torch.full((1, 4), S, device="cuda"), torch.full((1, 4), S, device="cuda")
    nul = C.c_void_p(0)
    rc = L.csl_prop_f32(infer._ptr(ip), infer._ptr(ix), infer._ptr(items), 1, nul, 0, 0, 0, infer._ptr(xs), 4, 4, infer._ptr(dinv), 0.8,
                        infer._ptr(base), 4, 0.5, -0.5, 1.0, nul, infer._ptr(out), 4, infer._ptr(out_s), 4, nul)
    assert rc == 0
    assert out.cpu().tolist() == [[0.25, -0.5, 1.0, 0.0]] and not out_s.cpu().numpy().any()


# ---- propagate along a trajectory ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _symmetric_graph():
    """the planted graph of 1200 nodes with a star of 700 spokes on node 0 (a hub of 2 parts) and two isolated nodes"""
    d = R.planted(n=1200, C=5)
    ip, ix = R.neighbour_csr(d["indptr"], d["indices"])
    n = 1202
    rows = np.repeat(np.arange(1200), np.diff(ip))
    spokes = np.arange(1, 701)
    src = np.concatenate([rows, np.zeros(700, dtype=np.int64), spokes])
    dst = np.concatenate([ix, spokes, np.zeros(700, dtype=np.int64)])
    o = np.argsort(src, kind="stable")
    nip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=nip[1:])
    nix = dst[o]
    assert nip[1] - nip[0] > 512 and nip[-1] == nip[-3]
    assert np.array_equal(np.sort(src * n + dst), np.sort(dst * n + src))          # symmetric
    return nip, nix


@pytest.mark.parametrize("alpha", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("fixed", [False, True])
def test_propagate_stays_within_the_trajectory_bound(alpha, fixed):
    from cslicer import infer, smooth
    ip, ix = _symmetric_graph()
    N, W, T = ip.shape[0] - 1, 8, 20
    g = infer.InferGraph(ip, ix, torch.device("cuda", torch.cuda.current_device())).upload()
    assert g.all_rows.plan["hubs"].shape[0] == 1
    rng = np.random.default_rng(5)
    x0 = np.zeros((N, W), dtype=np.float32)
    x0[:, :5] = rng.standard_normal((N, 5)).astype(np.float32)
    rows = np.sort(rng.permutation(N)[:300])
    vals = np.zeros((300, W), dtype=np.float32)
    vals[:, :5] = rng.standard_normal((300, 5)).astype(np.float32)
    fix_ref = (rows, vals.astype(np.float64)) if fixed else None
    fix_dev = (torch.from_numpy(rows).cuda(), torch.from_numpy(vals).cuda()) if fixed else None
    want, B = R.prop(ip, ix, x0, alpha, T, -1.0, 1.0, fix=fix_ref, bounds=True)
    dx0 = torch.from_numpy(x0).cuda()
    got = smooth.propagate(g, dx0, alpha, T, -1.0, 1.0, fix=fix_dev, chunk_rows=500)
    assert torch.equal(dx0.cpu(), torch.from_numpy(x0))                            # x0 is read, never written
    assert torch.equal(got, smooth.propagate(g, dx0, alpha, T, -1.0, 1.0, fix=fix_dev, chunk_rows=N))       # any chunking, same bits
    got = got.cpu().numpy().astype(np.float64)
    assert not got[:, 5:].any()                                                    # the padding columns stay zero
    if fixed:
        assert np.array_equal(got[rows], vals.astype(np.float64))
    bound = 1.001 * (alpha ** T * np.linalg.norm(B[0]) + sum(alpha ** (T - 1 - t) * np.linalg.norm(B[t + 1]) for t in range(T)))
    ratio = np.linalg.norm(got - want) / bound
    print("alpha %.1f fixed %s: ||X_T gpu - ref||_F / bound = %.3f" % (alpha, fixed, ratio))
    assert ratio <= 1.0
    zero = smooth.propagate(g, dx0, alpha, 0, -1.0, 1.0)
    assert torch.equal(zero, dx0) and zero.data_ptr() != dx0.data_ptr()            # steps == 0: a copy


# ---- end to end ------------------------------------------------------------------------------------------------------------

SEEDS = {2: 2}       # the seed of the planted inputs per class count: the first at which the REFERENCE meets the conditions below


@functools.lru_cache(maxsize=None)
def _planted_case(n_classes):
    d = R.planted(C=n_classes, seed=SEEDS.get(n_classes, 0))
    d["csr"] = R.neighbour_csr(d["indptr"], d["indices"])
    return d


def _same_classes(got, want64, d, what):
    """classes equal wherever the float64 margin is at least 1e-4; accuracy on the unlabelled half within the excluded share"""
    sure = R.margins(want64) >= 1e-4
    excluded = 1.0 - float(sure.mean())
    assert excluded <= 0.01, what                                                # (on the reference alone)
    pg, pw = got.argmax(1), want64.argmax(1)
    assert np.array_equal(pg[sure], pw[sure]), what
    test, cls = d["test"], d["cls"]
    acc_g, acc_w = float((pg == cls)[test].mean()), float((pw == cls)[test].mean())
    print("%s: accuracy %.4f (float64 %.4f), excluded share %.4f, largest difference %.3g"
          % (what, acc_g, acc_w, excluded, float(np.abs(got - want64).max())))
    assert abs(acc_g - acc_w) <= excluded + 1e-12, what


@pytest.mark.parametrize("n_classes", [1, 2, 3, 7, 47])
def test_correct_and_smooth_and_label_propagation_end_to_end(n_classes):
    from cslicer import infer, smooth
    d = _planted_case(n_classes)
    ip, ix = d["csr"]
    train, lab = d["train"], d["cls"][d["train"]]
    kw = dict(num_correction_layers=20, correction_alpha=0.8, num_smoothing_layers=20, smoothing_alpha=0.8)
    ref = R.correct_and_smooth(d["logits"], ip, ix, train, lab, 20, 0.8, 20, 0.8, True, 1.0)
    rs = ref["raw_scale"]
    assert not ((rs >= 900.0) & (rs <= 1100.0)).any()                              # no factor near the rule's threshold
    logits = torch.from_numpy(d["logits"]).cuda()
    got = smooth.correct_and_smooth(logits, d["indptr"], d["indices"], train, lab, **kw)
    assert got.shape == (d["n"], n_classes) and got.dtype == torch.float32 and got.is_contiguous()
    _same_classes(got.cpu().numpy().astype(np.float64), ref["out"], d, "C = %d autoscale" % n_classes)
    some = d["test"][::-1][:500].copy()
    sub = smooth.correct_and_smooth(d["logits"], d["indptr"], d["indices"], train, lab, nodes=some, chunk_rows=1000, **kw)
    assert torch.equal(sub, got[torch.from_numpy(some).cuda()])                    # host logits, a node list, other chunks
    if n_classes == 7:
        for a1 in (0.8, 1.0):
            ref = R.correct_and_smooth(d["logits"], ip, ix, train, lab, 20, a1, 20, 0.8, False, 1.0)
            fx = smooth.correct_and_smooth(logits, d["indptr"], d["indices"], train, lab, autoscale=False, scale=1.0,
                                           **dict(kw, correction_alpha=a1))
            _same_classes(fx.cpu().numpy().astype(np.float64), ref["out"], d, "C = 7 fixed scale, a1 = %.1f" % a1)
    lp = smooth.label_propagation(d["indptr"], d["indices"], n_classes, train, lab, alpha=0.8, num_layers=20)
    _same_classes(lp.cpu().numpy().astype(np.float64), R.label_propagation(ip, ix, n_classes, train, lab, 0.8, 20), d,
                  "C = %d label propagation" % n_classes)
    infer.release(d["indptr"], d["indices"])


# ---- the trainer and the command line --------------------------------------------------------------------------------------

def _task():
    from cslicer import l0
    n = 3000
    indptr, indices = l0.synth_graph(n, 8.0, seed=0)
    rng = np.random.default_rng(7)
    feats = rng.standard_normal((n, 12)).astype(np.float32)
    labels = np.argmax(feats[:, :3], axis=1).astype(np.int64)
    perm = rng.permutation(n)
    return indptr, indices, feats, labels, np.sort(perm[:2400]), np.sort(perm[2400:])


def test_trainer_and_predict_command_line(tmp_path, capsys):
    from cslicer import infer, l0, predict, smooth
    from cslicer.train import Trainer
    indptr, indices, feats, labels, train, hold = _task()
    t = Trainer(indptr, indices, feats, labels, 3, batch=64, streams=2, lr=1e-2, seed=3, fanouts=(3, 3), hidden=16)
    t.set_nodes(train)
    t.run(6)
    before = [p.detach().clone() for p in t.model.parameters()]
    steps = t.steps_done
    kw = dict(num_correction_layers=5, num_smoothing_layers=7, correction_alpha=0.7)
    res = t.correct_and_smooth(hold, train, **kw)
    ev = t.evaluate(hold)
    assert res["n"] == 600 and res["base_accuracy"] == ev["accuracy"]
    logits = t.predict()
    scores = smooth.correct_and_smooth(logits, indptr, indices, train, labels[train], nodes=hold, **kw)
    assert res["accuracy"] == float((scores.argmax(1).cpu().numpy() == labels[hold]).mean())
    assert t.steps_done == steps and all(torch.equal(a, b) for a, b in zip(before, t.model.parameters()))
    print("trainer: accuracy %.4f after Correct and Smooth, %.4f before" % (res["accuracy"], res["base_accuracy"]))
    # the command line on a written directory: the .npy is the Python interface's result
    d, ckpt, out = str(tmp_path / "l0"), str(tmp_path / "m.ckpt"), str(tmp_path / "p.npy")
    l0.write_l0(d, indptr, indices, features=feats, labels=labels.astype(np.int32), num_classes=3, train_idx=train, val_idx=hold)
    t.save_checkpoint(ckpt)
    t.close()
    nodes_file = str(tmp_path / "hold.npy")
    np.save(nodes_file, hold)
    argv = ["--model", ckpt, "--graph", d, "--out", out, "--nodes", nodes_file, "--correct-smooth", "--cs-layers", "5,7",
            "--cs-alpha", "0.7,0.8"]
    predict.main(argv + ["--logits"])
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (600, 3) and np.array_equal(got, scores.cpu().numpy())
    predict.main(argv)
    assert np.array_equal(np.load(out), got.argmax(1)) and np.load(out).dtype == np.int64
    predict.main(argv + ["--logits", "--cs-scale", "0.5"])
    fixed = smooth.correct_and_smooth(logits, indptr, indices, train, labels[train], nodes=hold, autoscale=False, scale=0.5, **kw)
    assert np.array_equal(np.load(out), fixed.cpu().numpy()) and not np.array_equal(np.load(out), got)
    assert capsys.readouterr().out.count("predict: 600 nodes") == 3
    infer.release(indptr, indices)
