"""The two layer-normalisation kernels (include/cslicer_layernorm.h, csrc/layernorm.hip) through the C ABI
against the float64 restatement of tests/norm_ref.py, at every width where their launch changes -- H / 4 on both sides of
every lane-group switch (1 | 2 | 3-4 | 5-8 | 9-16 | 17-32 | 33-64 lanes' worth), of the one-quad / four-quad register
switch (64 | 65) and of the register / re-read switch (256 | 257: H = 1024 | 1028) -- and at 1, R-1, R, R+1, 3R+1 rows
(R = 256 >> lg, the rows of one pass of a workgroup).  Every case runs as a block inside sentinel-filled wider buffers, in
place and out of place, forward-only and storing, with 0, 1 and 31 pad rows behind the gradient.

Tolerances.  Standard-normal rows: DESIGN 4.2's -- 1e-5 on forward values, 1e-4 x the largest entry on gradients.
Ill-conditioned rows (constant rows, rows at an offset of 1e4 with unit spread, rows with one non-zero element, zero rows):
the bound counted in fp32 roundings from the kernels' operation sequence (norm_ref.forward_bounds / backward_bounds); the
largest observed error / bound ratio is printed and recorded in DESIGN 4.13.  Sentinels, pad rows and everything said to be
"the same call" bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_ref

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
EPS = 1e-5
HQS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 256, 257]
E_INVALID = -1


def _lib():
    from cslicer import aggr
    return aggr._lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _rows(H):
    R = 256 >> norm_ref.lanes_lg(H)
    return sorted({1, R - 1, R, R + 1, 3 * R + 1})


def _data(kind, n, H, rng):
    """float32 rows, gamma (zeros and negative entries among them), beta"""
    if kind == "normal":
        z = rng.standard_normal((n, H))
    else:
        z = np.zeros((n, H))
        for r in range(n):
            c = r % 5
            if c == 0:
                z[r] = rng.choice([0.1, -3.7, 1e4, 1e-3])            # a constant row: variance 0
            elif c == 1:
                z[r] = 1e4 + rng.standard_normal(H)                   # unit spread far from zero
            elif c == 2:
                z[r, rng.integers(0, H)] = rng.choice([1.0, -250.0, 1e-6])      # one non-zero element
            elif c == 3:
                z[r] = -1e4 + 1e-2 * rng.standard_normal(H)
            # c == 4: a row of zeros
    gamma = rng.standard_normal(H)
    gamma[rng.random(H) < 0.25] = 0.0
    gamma[0] = -1.5
    return z.astype(np.float32), gamma.astype(np.float32), rng.standard_normal(H).astype(np.float32)


def _block(n, H, pad_rows=0):
    """a sentinel-filled [n + pad_rows + 2, H + 8] buffer, the [n + pad_rows, H] block inside it, and the mask of what is
    outside the block"""
    buf = torch.full((n + pad_rows + 2, H + 8), SENTINEL, device="cuda")
    outside = torch.ones(buf.shape, dtype=torch.bool)
    outside[1:n + pad_rows + 1, 4:4 + H] = False
    return buf, buf[1:n + pad_rows + 1, 4:4 + H], outside


def _fwd(z, gamma, beta, y, xhat, rstd, relu=1, eps=EPS):
    n, H = z.shape
    rc = _lib().csl_layernorm_relu_fwd_f32(_ptr(z), z.stride(0), _ptr(gamma), _ptr(beta), eps, n, H, _ptr(y), y.stride(0),
                                           _ptr(xhat) if xhat is not None else None, xhat.stride(0) if xhat is not None else 0,
                                           _ptr(rstd) if rstd is not None else None, relu, None)
    assert rc == 0, rc


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _check(what, got, want, bound, worst):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / bound).max()) if err.size else 0.0
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert ratio <= 1.0, "%s: error / bound = %.3g (largest error %.3g)" % (what, ratio, float(err.max()))


@pytest.mark.parametrize("kind", ["normal", "ill-conditioned"])
@pytest.mark.parametrize("hq", HQS)
def test_forward_and_backward_at_the_dispatch_edges(hq, kind):
    H = 4 * hq
    worst = {}
    for n in _rows(H):
        rng = np.random.default_rng(hq * 1009 + n)
        z_np, g_np, b_np = _data(kind, n, H, rng)
        gamma, beta = torch.from_numpy(g_np).cuda(), torch.from_numpy(b_np).cuda()
        y64, xh64, rs64 = norm_ref.forward(z_np, g_np, b_np, EPS)
        e_y, e_x, e_r = norm_ref.forward_bounds(z_np, g_np, b_np, EPS)
        # ---- forward, storing, out of place, every matrix a block of a wider sentinel-filled one
        zbuf, z, z_out = _block(n, H)
        ybuf, y, y_out = _block(n, H)
        xbuf, xhat, x_out = _block(n, H)
        rbuf = torch.full((n + 2,), SENTINEL, device="cuda")
        z.copy_(torch.from_numpy(z_np))
        _fwd(z, gamma, beta, y, xhat, rbuf[1:n + 1])
        torch.cuda.synchronize()
        assert np.array_equal(_bits(z), z_np.view(np.uint32))
        for buf, outside in ((zbuf, z_out), (ybuf, y_out), (xbuf, x_out)):
            assert bool((buf.cpu()[outside] == SENTINEL).all())
        assert float(rbuf[0]) == SENTINEL and float(rbuf[n + 1]) == SENTINEL
        y32, x32, r32 = y.cpu().numpy(), xhat.cpu().numpy(), rbuf[1:n + 1].cpu().numpy()
        if kind == "normal":
            assert float(np.abs(y32 - y64).max()) <= 1e-5 and float(np.abs(x32 - xh64).max()) <= 1e-5
        _check("y", y32, y64, e_y, worst)
        _check("xhat", x32, xh64, e_x, worst)
        _check("rstd", r32, rs64, e_r, worst)
        const = np.ptp(z_np, axis=1) == 0
        if const.any():   # zero variance: xhat = 0 up to the mean's rounding, y = relu(beta) up to |gamma| times that
            assert float(np.abs(y32[const] - np.maximum(b_np, 0)[None, :]).max()) <= float(e_y[const].max())
        # ---- the same call forward-only and in place (on the strided block), storing and in place (contiguous),
        # forward-only and out of place, and without the ReLU: bit for bit the first call's
        _fwd(z, gamma, beta, z, None, None)
        assert np.array_equal(_bits(z), _bits(y)) and bool((zbuf.cpu()[z_out] == SENTINEL).all())
        zc = torch.from_numpy(z_np).cuda()
        xc, rc_ = torch.empty_like(zc), torch.empty((n,), device="cuda")
        _fwd(zc, gamma, beta, zc, xc, rc_)
        assert np.array_equal(_bits(zc), _bits(y)) and np.array_equal(_bits(xc), _bits(xhat))
        assert np.array_equal(_bits(rc_), _bits(rbuf[1:n + 1]))
        zc = torch.from_numpy(z_np).cuda()
        yc = torch.empty_like(zc)
        _fwd(zc, gamma, beta, yc, None, None)
        assert np.array_equal(_bits(yc), _bits(y)) and np.array_equal(_bits(zc), z_np.view(np.uint32))
        _fwd(zc, gamma, beta, yc, None, None, relu=0)
        assert torch.equal(torch.relu(yc), y) and (kind != "normal" or n * H < 64 or bool((yc < 0).any()))
        # ---- backward, in place on the gradient, with 0, 1 and 31 pad rows of zeros behind it
        dn_np = rng.standard_normal((n, H)).astype(np.float32)
        dn_np[y32 <= 0] = 0.0                                        # (the caller's ReLU mask)
        dz64, dg64, db64 = norm_ref.backward(dn_np, x32, r32, g_np)
        e_dz, e_g, e_b = norm_ref.backward_bounds(dn_np, x32, r32, g_np)
        xh_dev, rs_dev = xhat, rbuf[1:n + 1].contiguous()
        for pad in (0, 1, 31):
            n_pad = n + pad
            floats = int(_lib().csl_layernorm_bwd_scratch(n_pad, H))
            assert floats > 0 and floats % H == 0
            dbuf, dn, d_out = _block(n, H, pad)
            dn[:n].copy_(torch.from_numpy(dn_np))
            dn[n:].zero_()
            parts = torch.full((2, floats + 4), SENTINEL, device="cuda")
            rc = _lib().csl_layernorm_bwd_f32(_ptr(dn), dn.stride(0), _ptr(xh_dev), xh_dev.stride(0), _ptr(rs_dev), _ptr(gamma), n,
                                              n_pad, H, _ptr(parts[0]), _ptr(parts[1]), None)
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert bool((dbuf.cpu()[d_out] == SENTINEL).all()) and bool((parts[:, floats:] == SENTINEL).all())
            assert not bool((_bits(dn[n:]) != 0).any())                                  # the pad rows: the zeros they were
            assert np.array_equal(_bits(xh_dev), x32.view(np.uint32))
            dz32 = dn[:n].cpu().numpy()
            if kind == "normal":
                assert float(np.abs(dz32 - dz64).max()) <= 1e-4 * float(np.abs(dz64).max())
            _check("dz", dz32, dz64, e_dz, worst)
            p = parts[:, :floats].double().cpu().numpy().reshape(2, floats // H, H).sum(1)   # the second stage, in float64
            if kind == "normal":
                assert float(np.abs(p[0] - dg64).max()) <= 1e-4 * float(np.abs(dg64).max()) + 1e-30
                assert float(np.abs(p[1] - db64).max()) <= 1e-4 * float(np.abs(db64).max()) + 1e-30
            _check("dgamma", p[0], dg64, e_g, worst)
            _check("colsum", p[1], db64, e_b, worst)
    print("H = %d, %s rows: largest error / bound %s" % (H, kind, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_more_blocks_than_2048_doubles_the_rows_of_a_block():
    """the first stage keeps at most 2048 blocks: 262,145 rows of width 8 are 1,025 blocks of 256 rows, not 2,049 of 128"""
    H, n = 8, 2048 * 128 + 1
    floats = int(_lib().csl_layernorm_bwd_scratch(n, H))
    assert floats == 1025 * H and int(_lib().csl_layernorm_bwd_scratch(2048 * 128, H)) == 2048 * H
    rng = np.random.default_rng(5)
    z_np, g_np, b_np = _data("normal", n, H, rng)
    z, gamma, beta = torch.from_numpy(z_np).cuda(), torch.from_numpy(g_np).cuda(), torch.from_numpy(b_np).cuda()
    y, xhat, rstd = torch.empty_like(z), torch.empty_like(z), torch.empty((n,), device="cuda")
    _fwd(z, gamma, beta, y, xhat, rstd)
    y64, xh64, _ = norm_ref.forward(z_np, g_np, b_np, EPS)
    assert float(np.abs(y.cpu().numpy() - y64).max()) <= 1e-5 and float(np.abs(xhat.cpu().numpy() - xh64).max()) <= 1e-5
    dn_np = rng.standard_normal((n, H)).astype(np.float32)
    dn = torch.from_numpy(dn_np).cuda()
    parts = torch.full((2, floats + 4), SENTINEL, device="cuda")
    rc = _lib().csl_layernorm_bwd_f32(_ptr(dn), H, _ptr(xhat), H, _ptr(rstd), _ptr(gamma), n, n, H, _ptr(parts[0]), _ptr(parts[1]), None)
    assert rc == 0
    dz64, dg64, db64 = norm_ref.backward(dn_np, xhat.cpu().numpy(), rstd.cpu().numpy(), g_np)
    assert float(np.abs(dn.cpu().numpy() - dz64).max()) <= 1e-4 * float(np.abs(dz64).max())
    assert bool((parts[:, floats:] == SENTINEL).all())
    p = parts[:, :floats].double().cpu().numpy().reshape(2, floats // H, H).sum(1)
    e_dz, e_g, e_b = norm_ref.backward_bounds(dn_np, xhat.cpu().numpy(), rstd.cpu().numpy(), g_np)
    assert bool((np.abs(p[0] - dg64) <= e_g).all()) and bool((np.abs(p[1] - db64) <= e_b).all())


def test_no_rows_and_only_pad_rows():
    L = _lib()
    H = 16
    g = torch.ones(H, device="cuda")
    assert L.csl_layernorm_relu_fwd_f32(None, H, None, None, EPS, 0, H, None, H, None, 0, None, 1, None) == 0
    assert L.csl_layernorm_bwd_f32(None, H, None, H, None, None, 0, 0, H, None, None, None) == 0
    assert int(L.csl_layernorm_bwd_scratch(0, H)) == 0
    # only pad rows: every block of the scratch is written, with zeros; the rows stay untouched
    n_pad = 300
    floats = int(L.csl_layernorm_bwd_scratch(n_pad, H))
    dn = torch.full((n_pad, H), SENTINEL, device="cuda")
    parts = torch.full((2, floats), SENTINEL, device="cuda")
    assert L.csl_layernorm_bwd_f32(_ptr(dn), H, None, H, None, _ptr(g), 0, n_pad, H, _ptr(parts[0]), _ptr(parts[1]), None) == 0
    assert bool((parts == 0).all()) and bool((dn == SENTINEL).all())


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    n, H = 8, 16
    z = torch.zeros((n, H), device="cuda")
    y, xh, rs = torch.zeros_like(z), torch.zeros_like(z), torch.zeros(n, device="cuda")
    g, b = torch.ones(H + 4, device="cuda"), torch.zeros(H + 4, device="cuda")
    ok = dict(z=_ptr(z), ldz=H, g=_ptr(g), b=_ptr(b), eps=EPS, n=n, H=H, y=_ptr(y), ldy=H, xh=_ptr(xh), ldh=H, rs=_ptr(rs))

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.csl_layernorm_relu_fwd_f32(a["z"], a["ldz"], a["g"], a["b"], a["eps"], a["n"], a["H"], a["y"], a["ldy"], a["xh"],
                                            a["ldh"], a["rs"], 1, None)
    assert fwd() == 0
    off = lambda t: C.c_void_p(t.data_ptr() + 4)      # noqa: E731  (4-byte aligned only)
    for bad in (dict(H=14), dict(H=0), dict(ldz=H - 4), dict(ldy=H + 2), dict(ldh=H - 4), dict(eps=0.0), dict(eps=-1e-5),
                dict(eps=float("nan")), dict(n=-1), dict(xh=None), dict(rs=None), dict(z=None), dict(y=None), dict(g=None),
                dict(b=None), dict(z=off(z), n=n - 1), dict(y=off(y), n=n - 1), dict(xh=off(xh), n=n - 1), dict(g=off(g)),
                dict(b=off(b))):
        assert fwd(**bad) == E_INVALID, bad
    assert L.csl_layernorm_bwd_scratch(-1, H) == E_INVALID and L.csl_layernorm_bwd_scratch(8, 6) == E_INVALID
    parts = torch.zeros((2, int(L.csl_layernorm_bwd_scratch(n + 3, H)) + 4), device="cuda")
    okb = dict(dn=_ptr(z), ldd=H, xh=_ptr(xh), ldh=H, rs=_ptr(rs), g=_ptr(g), n=n, n_pad=n, H=H, gp=_ptr(parts[0]), bp=_ptr(parts[1]))

    def bwd(**kw):
        a = dict(okb, **kw)
        return L.csl_layernorm_bwd_f32(a["dn"], a["ldd"], a["xh"], a["ldh"], a["rs"], a["g"], a["n"], a["n_pad"], a["H"], a["gp"],
                                       a["bp"], None)
    assert bwd() == 0
    for bad in (dict(H=14), dict(n=-1), dict(n_pad=n - 1), dict(ldd=H - 4), dict(ldh=H + 1), dict(gp=None), dict(bp=None),
                dict(dn=None), dict(xh=None), dict(rs=None), dict(g=None), dict(dn=off(z), n=n - 1, n_pad=n - 1), dict(g=off(g)),
                dict(gp=off(parts[0]))):
        assert bwd(**bad) == E_INVALID, bad
    torch.cuda.synchronize()


def test_autograd_node_against_float64_autograd():
    """aggr.LayerNormRelu (both kernels, the mask pass and the second stage of the sums) against
    relu(F.layer_norm(z) * gamma + beta) under float64 autograd, with and without the ReLU"""
    from cslicer import aggr
    rng = np.random.default_rng(3)
    for n, H, relu in ((700, 36, True), (130, 256, True), (50, 1028, True), (65, 20, False)):
        z_np, g_np, b_np = _data("normal", n, H, rng)
        up_np = rng.standard_normal((n, H)).astype(np.float32)
        z, gamma, beta = (torch.from_numpy(a).cuda().requires_grad_() for a in (z_np, g_np, b_np))
        y = aggr.LayerNormRelu.apply(z, gamma, beta, EPS, relu)
        y.backward(torch.from_numpy(up_np).cuda())
        zd, gd, bd = (torch.from_numpy(a).double().requires_grad_() for a in (z_np, g_np, b_np))
        yd = torch.nn.functional.layer_norm(zd, (H,), gd, bd, float(np.float32(EPS)))
        yd = torch.relu(yd) if relu else yd
        yd.backward(torch.from_numpy(up_np).double())
        assert float((y.detach().cpu().double() - yd.detach()).abs().max()) <= 1e-5
        for got, want in ((z.grad, zd.grad), (gamma.grad, gd.grad), (beta.grad, bd.grad)):
            assert float((got.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
        assert torch.equal(z.detach().cpu(), torch.from_numpy(z_np))
