"""tests/tail_ref.py against torch float64 autograd (cross_entropy, elu, (z.view(n, H, D) * a).sum(-1),
gat_ref.finish) and torch.optim.Adam in float64: a wrong restatement must not be able to hide a wrong kernel.  No GPU.
Differences stay at float64 rounding."""
import numpy as np
import pytest
import torch

import gat_ref
import sage_ref
import tail_ref as T

TOL = dict(rtol=1e-12, atol=1e-13)
F64 = torch.float64


@pytest.mark.parametrize("C", [1, 2, 3, 47, 65])
@pytest.mark.parametrize("shift", [0.0, 80.0, -80.0])
@pytest.mark.parametrize("use_map", [False, True])
def test_loss_rows_gradient_and_column_sums(C, shift, use_map):
    rng = np.random.default_rng(C)
    n, n_pad, ldl, ldgr, scale = 13, 16, C + 3, C + 5, 1.0 / 29
    buf = rng.standard_normal((n_pad + 1, ldl)) * 3 + shift
    n_nodes, n_lab = 40, 55
    ids = rng.permutation(n_nodes)[:n]
    rowmap = rng.permutation(n_lab)[:n_nodes] if use_map else None
    labels = rng.integers(0, C, size=n_lab)
    SENT = -777.0
    gbuf = torch.full((n_pad + 2, ldgr), SENT, dtype=F64)
    rows, g, cs = T.softmax_ce(buf.astype(np.float32), ldl, n, n_pad, C, ids, rowmap, labels, scale, gbuf, ldgr)
    s32 = float(np.float32(scale))
    z = torch.from_numpy(buf.astype(np.float32)[:n, :C].astype(np.float64)).requires_grad_()
    lab = torch.from_numpy(labels[rowmap[ids]] if use_map else labels[ids])
    want = torch.nn.functional.cross_entropy(z, lab, reduction="none") * s32
    want.sum().backward()
    torch.testing.assert_close(rows, want.detach(), **TOL)
    torch.testing.assert_close(g[:n], z.grad, **TOL)
    assert bool((g[n:] == 0).all()) and g.shape == (n_pad, C)
    torch.testing.assert_close(cs, z.grad.sum(0), **TOL)
    # the sum of the rows is sage_ref's loss
    assert abs(float(rows.sum()) - sage_ref.softmax_ce(z.detach(), lab, s32)[0]) <= 1e-12 * max(1.0, float(rows.sum()))
    # the wider buffer: rows [0, n_pad) x columns [0, C) written, everything else as it was
    assert torch.equal(gbuf[:n_pad, :C], g)
    assert bool((gbuf[:n_pad, C:] == SENT).all()) and bool((gbuf[n_pad:] == SENT).all())


def test_loss_bad_labels_and_infinite_logits():
    rng = np.random.default_rng(5)
    n, C = 8, 5
    z = (rng.standard_normal((n, C)) * 3).astype(np.float32)
    z[2, [0, 3]] = -np.inf                       # not the label: finite loss, zero gradient there
    z[3, 1] = -np.inf                            # the label: loss +inf
    z[4, :] = 7.5                                # all equal: log C
    labels = np.array([0, 4, 1, 1, 2, -1, C, 3])
    rows, g, cs = T.softmax_ce(z, C, n, n, C, np.arange(n), None, labels, 1.0)
    good = [0, 1, 2, 4, 7]
    zt = torch.from_numpy(z.astype(np.float64))
    want = torch.nn.functional.cross_entropy(zt[good], torch.from_numpy(labels[good]), reduction="none")
    torch.testing.assert_close(rows[good], want, **TOL)
    assert bool(torch.isfinite(rows[2])) and bool((g[2, [0, 3]] == 0).all())
    assert float(rows[3]) == float("inf")
    assert abs(float(rows[4]) - np.log(C)) <= 1e-15 * 8
    assert bool(torch.isnan(rows[[5, 6]]).all()) and bool(torch.isnan(g[[5, 6]]).all())
    assert bool(torch.isfinite(g[good]).all())
    assert bool(torch.isnan(rows.sum())) and bool(torch.isnan(cs).all())


@pytest.mark.parametrize("lr", [1e-3, 3e-3, 1.0])
def test_adam_step_is_torch_adam_with_float32_rounded_betas(lr):
    """20 steps of tail_ref.adam_step = torch.optim.Adam in float64 GIVEN the float32-rounded lr, betas and eps; with
    the double betas torch is a different function (the docstring's 6e-5), which the last assertion shows"""
    rng = np.random.default_rng(1)
    b1, b2, eps = 0.9, 0.999, 1e-8
    f = lambda x: float(np.float32(x))
    p0 = rng.standard_normal(97)
    p = torch.from_numpy(p0.copy()).requires_grad_()
    q = torch.from_numpy(p0.copy()).requires_grad_()
    opt = torch.optim.Adam([p], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps))
    opt_d = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    mine, m, v = torch.from_numpy(p0.copy()), torch.zeros(97, dtype=F64), torch.zeros(97, dtype=F64)
    for step in range(1, 21):
        g = torch.from_numpy(rng.standard_normal(97) * 10.0 ** rng.integers(-3, 4))
        p.grad, q.grad = g.clone(), g.clone()
        opt.step()
        opt_d.step()
        mine, m, v, upd, m_abs, v_abs = T.adam_step(mine, g, m, v, lr, b1, b2, eps, step)
        torch.testing.assert_close(mine, p.detach(), rtol=1e-12, atol=1e-12)
        assert bool((m_abs >= m.abs()).all()) and torch.equal(v_abs, v)
    st = opt.state[p]
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=1e-12)      # (torch: a lerp, the same number)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=0)
    rel = ((v - opt_d.state[q]["exp_avg_sq"]).abs() / v).max()
    assert 1e-9 < float(rel) < 1e-4                 # double betas: another function, far beyond float64 rounding


@pytest.mark.parametrize("H,D", [(1, 4), (3, 8), (2, 68), (1, 252)])
def test_logits_forward_and_backward(H, D):
    rng = np.random.default_rng(H * 1000 + D)
    n = 7
    z = torch.from_numpy(rng.standard_normal((n, H * D))).requires_grad_()
    al = torch.from_numpy(rng.standard_normal((H, D))).requires_grad_()
    ar = torch.from_numpy(rng.standard_normal((H, D))).requires_grad_()
    g_el, g_er = torch.from_numpy(rng.standard_normal((n, H))), torch.from_numpy(rng.standard_normal((n, H)))
    before = torch.from_numpy(rng.standard_normal((n, H * D)))
    el, er = (z.view(n, H, D) * al).sum(-1), (z.view(n, H, D) * ar).sum(-1)
    ((el * g_el).sum() + (er * g_er).sum()).backward()
    got_el, got_er = T.logits_fwd(z, al, ar, H, D)
    torch.testing.assert_close(got_el, el.detach(), **TOL)
    torch.testing.assert_close(got_er, er.detach(), **TOL)
    g_z, g_al, g_ar = T.logits_bwd(z, al, ar, g_el, g_er, H, D)
    torch.testing.assert_close(g_z, z.grad, **TOL)
    torch.testing.assert_close(g_al, al.grad, **TOL)
    torch.testing.assert_close(g_ar, ar.grad, **TOL)
    acc, g_al2, _ = T.logits_bwd(z, al, ar, g_el, g_er, H, D, g_z_before=before)
    torch.testing.assert_close(acc, before + z.grad, **TOL)
    assert torch.equal(g_al2, g_al)


@pytest.mark.parametrize("use_elu", [False, True])
@pytest.mark.parametrize("H,D", [(1, 4), (3, 8), (2, 68)])
def test_finish_forward_and_backward(H, D, use_elu):
    rng = np.random.default_rng(H + D)
    n = 9
    nn = torch.from_numpy(rng.standard_normal((n, H * D)) * 3).requires_grad_()
    s = torch.from_numpy(rng.uniform(0.5, 9.0, size=(n, H))).requires_grad_()
    bias = torch.from_numpy(rng.standard_normal(H * D)).requires_grad_()
    g = torch.from_numpy(rng.standard_normal((n, H * D)))
    out = gat_ref.finish(nn, s, bias, H, D, use_elu)
    (out * g).sum().backward()
    got = T.finish_fwd(nn, s, bias, H, D, use_elu)
    torch.testing.assert_close(got, out.detach(), **TOL)
    g_n, g_s, g_b, p = T.finish_bwd(g, got, nn, s, H, D, use_elu)
    torch.testing.assert_close(g_n, nn.grad, **TOL)
    torch.testing.assert_close(g_s, s.grad, **TOL)
    torch.testing.assert_close(g_b, bias.grad, **TOL)


def test_finish_floor_and_elu_corners():
    H, D = 2, 4
    bias = torch.tensor([0.5, -0.25, 0.0, 2.0, -200.0, -105.0, 1.0, -1.0], dtype=F64)
    # a head sum of 0 with n = 0: act(bias); a head sum below the floor divides by the floor
    n0, s0 = torch.zeros((1, H * D), dtype=F64), torch.zeros((1, H), dtype=F64)
    out = T.finish_fwd(n0, s0, bias, H, D, True)
    torch.testing.assert_close(out[0], torch.nn.functional.elu(bias), **TOL)
    assert float(out[0, 2]) == 0.0
    g = torch.ones((1, H * D), dtype=F64)
    g_n, g_s, g_b, p = T.finish_bwd(g, out.float(), n0, s0, H, D, True)   # (the float32 out: -1 exactly below -104)
    assert bool(torch.isfinite(g_s).all()) and bool((g_s == 0).all())
    assert p[0, :4].tolist() == [1.0, float(out.float()[0, 1]) + 1.0, 1.0, 1.0]      # out == 0 exactly: slope 1
    assert float(out.float()[0, 4]) == -1.0 and float(p[0, 4]) == 0.0 and float(p[0, 5]) == 0.0
    torch.testing.assert_close(g_n, p / T.S_FLOOR, **TOL)
    small = torch.full((1, H), 1e-35, dtype=F64)
    n1 = torch.full((1, H * D), 3e-31, dtype=F64)
    out1 = T.finish_fwd(n1, small, bias, H, D, False)
    torch.testing.assert_close(out1[0], 3e-31 / T.S_FLOOR + bias, **TOL)
    # at and above the floor it is gat_ref.finish
    s2 = torch.tensor([[T.S_FLOOR, 4.0]], dtype=F64)
    torch.testing.assert_close(T.finish_fwd(n1, s2, bias, H, D, True), gat_ref.finish(n1, s2, bias, H, D, True), **TOL)


@pytest.mark.parametrize("use_elu", [False, True])
def test_bias_elu_and_its_backward(use_elu):
    rng = np.random.default_rng(11)
    n, C = 6, 12
    y = torch.from_numpy(rng.standard_normal((n, C)) * 4).requires_grad_()
    bias = torch.from_numpy(rng.standard_normal(C)).requires_grad_()
    g = torch.from_numpy(rng.standard_normal((n, C)))
    want = torch.nn.functional.elu(y + bias) if use_elu else y + bias
    (want * g).sum().backward()
    got = T.bias_elu(y, bias, use_elu)
    torch.testing.assert_close(got, want.detach(), **TOL)
    out, cs = T.elu_bwd_colsum(g, got, use_elu)
    torch.testing.assert_close(out, y.grad, **TOL)
    torch.testing.assert_close(cs, bias.grad, **TOL)
    # the corners of the slope read off the output
    sl = T.elu_slope_from_output(torch.tensor([0.0, -1.0, 3.0, -0.25], dtype=F64))
    assert sl.tolist() == [1.0, 0.0, 1.0, 0.75]
