"""Layer normalisation between the GraphSAGE layers without a GPU: tests/norm_ref.py pinned to
torch.nn.functional.layer_norm + relu under float64 autograd, the C ABI's binding and host-side refusals,
cslicer.train.step_plan_norm, the constructor's ValueErrors, the command line, and checkpoints of a normalised model on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_ref

NAMES = ["csl_layernorm_relu_fwd_f32", "csl_layernorm_bwd_scratch", "csl_layernorm_bwd_f32", "csl_sage_fwd_bwd_norm_workspace",
         "csl_sage_fwd_bwd_norm"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,H,eps", [(1, 4, 1e-5), (7, 12, 1e-5), (33, 256, 1e-3), (5, 1028, 1e-5)])
def test_restatement_is_torch_layer_norm_relu_under_float64_autograd(n, H, eps):
    rng = np.random.default_rng(n * 31 + H)
    z, g, b, up = rng.standard_normal((n, H)), rng.standard_normal(H), rng.standard_normal(H), rng.standard_normal((n, H))
    z[0] = 3.0 if n > 1 else z[0]                 # a constant row: variance 0
    g[1] = 0.0
    y, xhat, rstd = norm_ref.forward(z, g, b, eps)
    zt, gt, bt = (torch.tensor(a, requires_grad=True) for a in (z, g, b))
    yt = torch.relu(torch.nn.functional.layer_norm(zt, (H,), gt, bt, float(np.float32(eps))))
    yt.backward(torch.tensor(up))
    assert float(np.abs(y - yt.detach().numpy()).max()) <= 1e-12
    pre = norm_ref.forward(z, g, b, eps, relu=False)[0]
    assert np.array_equal(np.maximum(pre, 0), y) and (pre < 0).any()
    dn = up * (y > 0)                               # the caller's ReLU mask
    dz, dgamma, colsum = norm_ref.backward(dn, xhat, rstd, g)
    scale = lambda t: max(1.0, float(t.abs().max()))      # noqa: E731
    assert float(np.abs(dz - zt.grad.numpy()).max()) <= 1e-10 * scale(zt.grad)
    assert float(np.abs(dgamma - gt.grad.numpy()).max()) <= 1e-10 * scale(gt.grad)
    assert float(np.abs(dn.sum(0) - bt.grad.numpy()).max()) <= 1e-10 * scale(bt.grad)
    assert float(np.abs(colsum - dz.sum(0)).max()) == 0.0
    if n > 1:                                       # zero variance: xhat = 0, y = relu(beta)
        assert float(np.abs(xhat[0]).max()) == 0.0 and np.array_equal(y[0], np.maximum(b, 0))
        assert rstd[0] == pytest.approx(1.0 / np.sqrt(float(np.float32(eps))))


def test_the_variance_is_the_biased_one_and_every_backward_term_counts():
    """the three value-only mistakes DESIGN 4.13 lists are visible to the restatement's pin"""
    rng = np.random.default_rng(1)
    z, g, b, dn = rng.standard_normal((6, 8)), rng.standard_normal(8), rng.standard_normal(8), rng.standard_normal((6, 8))
    y, xhat, rstd = norm_ref.forward(z, g, b, 1e-5)
    unbiased = 1.0 / np.sqrt(z.var(1, ddof=1) + 1e-5)
    assert float(np.abs(unbiased / rstd - 1).max()) > 0.05
    dz, dgamma, _ = norm_ref.backward(dn, xhat, rstd, g)
    a = g[None, :] * dn
    dropped = rstd[:, None] * (a - a.mean(1, keepdims=True))
    assert float(np.abs(dropped - dz).max()) > 1e-2 and float(np.abs(dn.sum(0) - dgamma).max()) > 1e-2


def test_rounding_bounds_cover_a_float32_evaluation_on_the_cpu():
    """the same operation sequence in numpy float32 (sequential sums: inside the d-deep tree's worst case for these widths
    is not claimed -- the kernels' own check is tests/test_gpu_norm_edges.py); here the bounds must at least hold for
    torch's float32 layer_norm on ill-conditioned rows, and be tight enough to mean something on well-conditioned ones"""
    rng = np.random.default_rng(2)
    H = 64
    z = np.concatenate([rng.standard_normal((8, H)), 1e4 + rng.standard_normal((8, H)), np.full((2, H), 0.1)]).astype(np.float32)
    g, b = rng.standard_normal(H).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    y64 = norm_ref.forward(z, g, b, 1e-5)[0]
    e_y, e_x, e_r = norm_ref.forward_bounds(z, g, b, 1e-5)
    assert float(e_y[:8].max()) < 1e-5 and float(e_x[:8].max()) < 1e-5          # standard-normal rows: within DESIGN 4.2's
    assert float(e_x[8:16].max()) > 1e-3                                         # an offset of 1e4 costs what it costs
    y32 = torch.relu(torch.nn.functional.layer_norm(torch.from_numpy(z), (H,), torch.from_numpy(g), torch.from_numpy(b), 1e-5))
    assert bool((np.abs(y32.numpy() - y64)[:8] <= e_y[:8]).all())
    assert norm_ref.sum_depth(4) == 3 and norm_ref.sum_depth(256) == 9 and norm_ref.sum_depth(1024) == 12
    assert norm_ref.sum_depth(1028) == 13 and [norm_ref.lanes_lg(4 * q) for q in (1, 2, 3, 4, 5, 64, 65)] == [0, 1, 2, 2, 3, 6, 6]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def test_the_header_is_bound_like_the_others():
    from cslicer import _abi, aggr
    L = _abi.load()
    assert "cslicer_layernorm.h" in _abi.HEADERS and _abi.BOUND["cslicer_layernorm.h"] == NAMES == aggr.LAYERNORM_SYMBOLS
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert list(L.csl_layernorm_relu_fwd_f32.argtypes) == [vp, i64, vp, vp, f32, i64, i32, vp, i64, vp, i64, vp, i32, vp]
    assert list(L.csl_layernorm_bwd_f32.argtypes) == [vp, i64, vp, i64, vp, vp, i64, i64, i32, vp, vp, vp]
    assert list(L.csl_layernorm_bwd_scratch.argtypes) == [i64, i32] and L.csl_layernorm_bwd_scratch.restype is i64
    assert list(L.csl_sage_fwd_bwd_norm.argtypes) == [i32, vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, f32, f32, i64, i32, vp, vp,
                                                      vp, i64, vp, f32, i64, i64, vp, i64, vp, vp, f32, vp]
    assert L.csl_sage_fwd_bwd_norm_workspace.restype is i64


def test_the_entry_points_refuse_before_any_hip_call():
    """no GPU here: every one of these returns CSL_E_INVALID (-1) from the host-side checks"""
    from cslicer import _abi, aggr
    L = _abi.load()
    buf = np.zeros(256 + 8, dtype=np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16              # a 16-byte aligned host address: never dereferenced
    x, odd, nul = C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(0)
    ok = dict(z=x, ldz=8, g=x, b=x, eps=1e-5, n=4, H=8, y=x, ldy=8, xh=x, ldh=8, rs=x, relu=1, st=nul)

    def fwd(**kw):
        return L.csl_layernorm_relu_fwd_f32(*dict(ok, **kw).values())
    for bad in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(n=-1), dict(H=6), dict(H=0), dict(ldz=4), dict(ldz=10),
                dict(ldy=6), dict(ldh=4), dict(xh=nul), dict(rs=nul), dict(z=nul), dict(y=nul), dict(g=nul), dict(b=nul),
                dict(z=odd), dict(y=odd), dict(xh=odd), dict(g=odd), dict(b=odd)):
        assert fwd(**bad) == -1, bad
    assert fwd(n=0) == 0 and fwd(n=0, z=nul, y=nul, g=nul, b=nul, xh=nul, rs=nul) == 0       # no rows: nothing to launch
    okb = dict(dn=x, ldd=8, xh=x, ldh=8, rs=x, g=x, n=4, n_pad=4, H=8, gp=x, bp=x, st=nul)

    def bwd(**kw):
        return L.csl_layernorm_bwd_f32(*dict(okb, **kw).values())
    for bad in (dict(n=-1), dict(n_pad=3), dict(H=6), dict(ldd=4), dict(ldh=9), dict(gp=nul), dict(bp=nul), dict(gp=odd),
                dict(dn=nul), dict(xh=nul), dict(rs=nul), dict(g=nul), dict(dn=odd), dict(xh=odd), dict(g=odd)):
        assert bwd(**bad) == -1, bad
    assert bwd(n=0, n_pad=0, dn=nul, xh=nul, rs=nul, g=nul, gp=nul, bp=nul) == 0
    # the scratch: ceil(n_pad / rows of a block) blocks of H floats; a block has 32 rows, or one pass of the workgroup
    # (256 >> lg rows) where that is more, 128 for a row wider than the registers hold; doubled beyond 2048 blocks
    S = L.csl_layernorm_bwd_scratch
    assert S(-1, 8) == -1 and S(8, 6) == -1 and S(8, 0) == -1 and S(0, 8) == 0
    assert S(128, 8) == 8 and S(129, 8) == 16 and S(256, 4) == 4 and S(257, 4) == 8 and S(129, 1028) == 2 * 1028
    assert S(32, 256) == 256 and S(33, 256) == 512 and S(32, 36) == 36 and S(33, 36) == 72 and S(128, 1028) == 1028
    assert S(2048 * 128, 8) == 2048 * 8 and S(2048 * 128 + 1, 8) == 1025 * 8 and S(10 ** 6, 1028) == 7813 * 1028
    # the step: eps, gamma / beta and the dropout arguments, before its layout is even looked at
    dims = (C.c_int32 * 3)(8, 8, 4)
    sl = (aggr.SageSlice * 2)()
    sl[0].n_out = 3
    ptrs, none = (C.c_void_p * 1)(base), (C.c_void_p * 1)()

    def step(eps=1e-5, gammas=ptrs, betas=ptrs, p=0.0, out_ids=nul, labels=x, smoothing=0.0, words=nul, ldw=0):
        return L.csl_sage_fwd_bwd_norm(2, dims, sl, nul, nul, nul, 0, 8, nul, nul, labels, nul, smoothing, 1.0, 0, 1, nul, nul, nul, 0,
                                       out_ids, p, 1, 0, words, ldw, gammas, betas, eps, nul)
    for bad in (dict(eps=0.0), dict(gammas=nul), dict(betas=none), dict(gammas=(C.c_void_p * 1)(base + 4))):
        assert step(**bad) == -1 and b"norm: eps > 0" in L.csl_sage_last_error(), bad
    assert step(p=0.5) == -1 and b"norm step" in L.csl_sage_last_error()
    assert step(words=x, ldw=0) == -1 and b"norm step" in L.csl_sage_last_error()
    assert step(labels=nul) == -1 and b"labels" in L.csl_sage_last_error()
    assert step(smoothing=1.0) == -1 and b"label_smoothing" in L.csl_sage_last_error()
    assert step() == -1 and b"bad argument" in L.csl_sage_last_error()      # (past the norm's checks: the null weights)
    # the workspace of the normalised step: the plain one plus xhat, rstd and the two first stages per normalised layer
    for k in range(2):
        sl[k].n_out, sl[k].n_in = (40, 100) if k == 0 else (10, 40)
    plain, normed = L.csl_sage_fwd_bwd_workspace(2, dims, sl, 0, 1), L.csl_sage_fwd_bwd_norm_workspace(2, dims, sl, 0, 1)
    assert plain > 0 and normed == plain + 40 * 8 + 40 + 2 * 8


# ---- step_plan -----------------------------------------------------------------------------------------------------------

def test_step_plan_with_norm():
    """norm=None: every tabulated plan is today's.  norm="layer": the rank path's native_rank becomes the autograd rank step
    -- exactly the rows that dropout moves, to the same plans -- and every other row is unchanged.  (step_plan's own
    signature is pinned by tests/test_loss_ref_cpu.py; the norm is step_plan_norm's keyword, the plan the trainer asks for.)"""
    import test_step_plan_cpu as T
    from cslicer.train import Switches, step_plan, step_plan_norm
    moved = 0
    for row, change, flags, path, gat_input, input_form in T.ROWS:
        cfg = dict(T.BASE, **change)
        sw = Switches(**{k: cfg.pop(k) for k in Switches._fields})
        today = step_plan(sw=sw, **cfg)
        assert tuple(today) == (flags, path, gat_input, input_form), row
        assert step_plan_norm(sw=sw, **cfg) == step_plan_norm(None, sw=sw, **cfg) == step_plan_norm(norm=None, sw=sw, **cfg) == today, row
        got = step_plan_norm("layer", sw=sw, **cfg)
        assert got == step_plan(sw=sw, dropout=0.5, **cfg) == step_plan_norm("layer", sw=sw, dropout=0.5, **cfg), row
        if path == "native_rank":
            moved += 1
            assert got == step_plan(sw=sw._replace(py_step=True), **cfg), row
            assert got.path == "parts" and got.input_form == "rows" and not got.gat_input, row
            assert got.engine_flags == flags & ~T.T, row
        else:
            assert got == today, row
    assert moved == 5
    base = {k: v for k, v in T.BASE.items() if k not in Switches._fields}
    assert step_plan_norm("layer", **base).path == "native" and step_plan_norm("layer", **dict(base, dropout=0.5)).path == "native"


# ---- the constructor, the model and the command line ---------------------------------------------------------------------------

def _tiny():
    indptr = np.arange(9, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, 8, size=16).astype(np.int64)
    return indptr, indices, np.zeros((8, 8), dtype=np.float32), np.zeros(8, dtype=np.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(norm="layer", model="gat"), "attention model"), (dict(norm="layer", hidden=30), "multiple of 4"),
    (dict(norm="batch"), "norm must be None or 'layer'"), (dict(norm=True), "norm must be None or 'layer'"),
    (dict(norm="layer", norm_eps=0.0), "norm_eps must be > 0"), (dict(norm="layer", norm_eps=-1e-5), "norm_eps must be > 0"),
    (dict(norm_eps=float("nan")), "norm_eps must be > 0"),
])
def test_constructor_refuses_before_any_device_call(kw, match, monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats, labels = _tiny()
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, **kw)


def test_model_registers_gamma_and_beta_behind_the_layers():
    from cslicer import splitgnn
    plain = splitgnn.DistSAGEModel(8, 16, 3, n_layers=3)
    torch.manual_seed(0)
    a = splitgnn.DistSAGEModel(8, 16, 3, n_layers=3, norm=None)
    torch.manual_seed(0)
    m = splitgnn.DistSAGEModel(8, 16, 3, n_layers=3, norm="layer", norm_eps=1e-4)
    names = [n for n, _ in m.named_parameters()]
    assert names[:6] == [n for n, _ in plain.named_parameters()] == [n for n, _ in a.named_parameters()]
    assert names[6:] == ["norms.0.gamma", "norms.0.beta", "norms.1.gamma", "norms.1.beta"]
    assert not hasattr(plain, "norms") and list(plain.state_dict()) == list(a.state_dict())
    for k in range(2):
        assert torch.equal(m.norms[k].gamma, torch.ones(16)) and torch.equal(m.norms[k].beta, torch.zeros(16))
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), m.parameters()))       # the layers' own initial weights
    assert m.norm == "layer" and m.norm_eps == 1e-4 and plain.norm is None
    assert len(splitgnn.DistSAGEModel(8, 16, 3, n_layers=1, norm="layer").norms) == 0
    for bad in (dict(norm="batch"), dict(norm="layer", norm_eps=0), dict(norm="layer", hidden=10)):
        with pytest.raises(ValueError):
            splitgnn.DistSAGEModel(8, bad.pop("hidden", 16), 3, n_layers=2, **bad)


def test_command_line_norm_reaches_the_constructor(monkeypatch):
    from cslicer import l0, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train, "Trainer", fake)
    monkeypatch.setattr(l0, "synth_graph", lambda n, d, seed=0: _tiny()[:2])
    for argv, want in ((["--norm", "layer"], {"norm": "layer"}), (["--norm", "layer", "--norm-eps", "1e-6"],
                                                                   {"norm": "layer", "norm_eps": 1e-6}), ([], {})):
        seen.clear()
        with pytest.raises(Stop):
            train.main(["--graph", "synthetic", "--num-layers", "2", "--fan-out", "2,2"] + argv)
        assert {k: v for k, v in seen.items() if k.startswith("norm")} == want
    with pytest.raises(SystemExit):
        train._parser().parse_args(["--norm", "batch"])
    assert "--norm layer" in train.main.__doc__


# ---- checkpoints ---------------------------------------------------------------------------------------------------------

TODAY = {"kind", "in_feats", "hidden", "n_classes", "heads", "n_layers", "multilabel"}


def test_checkpoint_round_trip_of_a_normalised_model_on_the_cpu(tmp_path):
    from cslicer import checkpoint, splitgnn
    torch.manual_seed(1)
    m = splitgnn.DistSAGEModel(8, 16, 3, n_layers=3, norm="layer", norm_eps=1e-4)
    with torch.no_grad():
        for x in m.norms:
            x.gamma.normal_()
            x.beta.normal_()
    path = str(tmp_path / "m.pt")
    checkpoint.write(path, m, trainer={"steps_done": 0, "norm": "layer"})
    ck = checkpoint.read(path)
    assert set(ck["model"]) == TODAY | {"norm", "norm_eps"} and ck["model"]["norm"] == "layer" and ck["model"]["norm_eps"] == 1e-4
    assert ck["trainer"]["norm"] == "layer"
    back = checkpoint.model_from(ck)
    assert back.norm == "layer" and back.norm_eps == 1e-4
    assert list(back.state_dict()) == list(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), m.state_dict().values()))
    checkpoint.check_model(ck["model"], checkpoint.model_block(m))
    plain = splitgnn.DistSAGEModel(8, 16, 3, n_layers=3)
    with pytest.raises(ValueError, match="norm = 'layer'.*has None"):
        checkpoint.check_model(ck["model"], checkpoint.model_block(plain))
    with pytest.raises(ValueError, match="norm_eps"):
        checkpoint.check_model(ck["model"], checkpoint.model_block(splitgnn.DistSAGEModel(8, 16, 3, norm="layer")))


def test_a_norm_free_file_has_the_keys_it_always_had(tmp_path):
    from cslicer import checkpoint, splitgnn
    plain = splitgnn.DistSAGEModel(8, 16, 3, n_layers=2)
    path = str(tmp_path / "p.pt")
    checkpoint.write(path, plain)
    ck = checkpoint.read(path)
    assert set(ck["model"]) == TODAY and set(ck) == {"format", "version", "model", "state", "optimizer", "trainer", "extra"}
    assert list(ck["state"]) == ["convs.0.fc.weight", "convs.0.fc.bias", "convs.1.fc.weight", "convs.1.fc.bias"]
    back = checkpoint.model_from(ck)
    assert back.norm is None and not hasattr(back, "norms")
    checkpoint.check_model(ck["model"], checkpoint.model_block(plain))
    with pytest.raises(ValueError, match="norm = None"):
        checkpoint.check_model(ck["model"], checkpoint.model_block(splitgnn.DistSAGEModel(8, 16, 3, n_layers=2, norm="layer")))
    gat = splitgnn.DistGATModel(8, 4, 3, heads=2, n_layers=2)
    checkpoint.write(path, gat)
    assert set(checkpoint.read(path)["model"]) == TODAY
