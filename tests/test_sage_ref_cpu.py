"""tests/sage_ref.py against torch float64 autograd, without a GPU: the hand-written backward formulas, the slice by
source and the whole model must agree with what autograd derives from the forward definitions alone.  (A wrong
restatement must not be able to hide a wrong kernel.)  Float64 on both sides: 1e-12."""
import numpy as np
import pytest
import torch

import sage_ref as R

TOL = dict(rtol=1e-12, atol=1e-12)


def _csr(rng, n, n_src, max_deg, no_self_every=3):
    deg = rng.integers(0, max_deg + 1, size=n)
    deg[: min(n, 2)] = (0, 1)[: min(n, 2)]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n_src, size=int(indptr[-1]))
    self_ids = rng.permutation(n_src)[:n] if n <= n_src else rng.integers(0, n_src, size=n)
    self_ids = self_ids.astype(np.int64)
    if no_self_every:
        self_ids[::no_self_every] = -1
    return indptr, indices, self_ids


def _autograd_operand(x, indptr, indices, self_ids, rowmap, relu_in):
    """the operand from the definition, with torch ops that autograd differentiates"""
    h = torch.relu(x) if relu_in else x
    sid, idx = torch.from_numpy(self_ids), torch.from_numpy(indices)
    if rowmap is not None:
        rm = torch.from_numpy(rowmap)
        sid_rows, idx = rm[sid.clamp_min(0)], rm[idx]
    else:
        sid_rows = sid.clamp_min(0)
    n = sid.numel()
    rows = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(indptr)))
    parts = []
    for r in range(n):                                       # row by row, nothing shared with sage_ref's index_add
        nb = h[idx[rows == r]]
        parts.append(torch.cat([h[sid_rows[r]] if sid[r] >= 0 else torch.zeros_like(h[0]),
                                nb.sum(0) / max(nb.shape[0], 1)]))
    return torch.stack(parts) if parts else torch.zeros((0, 2 * x.shape[1]), dtype=x.dtype)


@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("use_map", [False, True])
def test_operand_and_layer_output(relu_in, use_map):
    rng = np.random.default_rng(1 + relu_in + 2 * use_map)
    n, n_src, H, out, n_pad = 37, 23, 8, 5, 64
    indptr, indices, self_ids = _csr(rng, n, n_src, 6)
    rowmap = rng.permutation(50)[:n_src] if use_map else None
    x = torch.from_numpy(rng.standard_normal((50 if use_map else n_src, H)))
    W, b = rng.standard_normal((out, 2 * H)), rng.standard_normal(out)
    cat = R.operand(x, indptr, indices, self_ids, n_pad, rowmap=rowmap, relu_in=relu_in)
    want = _autograd_operand(x, indptr, indices, self_ids, rowmap, relu_in)
    torch.testing.assert_close(cat[:n], want, **TOL)
    assert cat.shape == (n_pad, 2 * H) and bool((cat[n:] == 0).all())
    assert bool((cat[:n][self_ids < 0, :H] == 0).all()) and bool((cat[0, H:] == 0).all())      # no self row; empty row
    for relu_out in (False, True):
        y = R.layer_out(cat, W, b, relu_out)
        yw = torch.nn.functional.linear(cat, torch.from_numpy(W), torch.from_numpy(b))
        torch.testing.assert_close(y, torch.relu(yw) if relu_out else yw, **TOL)
        torch.testing.assert_close(y[n:], (torch.from_numpy(b).clamp_min(0) if relu_out else torch.from_numpy(b))
                                   .expand(n_pad - n, -1), **TOL)


def test_operand_gradient_by_destination_and_by_source_equal_autograd():
    rng = np.random.default_rng(7)
    n, n_src, H = 41, 19, 4
    indptr, indices, self_ids = _csr(rng, n, n_src, 9)
    self_ids[5] = -1
    x = torch.from_numpy(rng.standard_normal((n_src, H))).requires_grad_()
    gcat = torch.from_numpy(rng.standard_normal((n, 2 * H)))
    (_autograd_operand(x, indptr, indices, self_ids, None, False) * gcat).sum().backward()
    gd = R.operand_grad_by_destination(gcat, indptr, indices, self_ids, n_src)
    torch.testing.assert_close(gd, x.grad, **TOL)
    tp, ti = R.by_source(indptr, indices, self_ids, n_src)
    assert tp[-1] == ti.shape[0] == indices.shape[0] + int((self_ids >= 0).sum())
    for u in range(n_src):      # every list: the self entries (if any) first, then destination rows in edge order
        lst = ti[tp[u]:tp[u + 1]]
        assert sorted(lst[lst >= 0].tolist()) == lst[lst >= 0].tolist() and (np.diff((lst >= 0).astype(int)) >= 0).all()
        assert all(self_ids[~t] == u for t in lst[lst < 0]) and all(u in indices[indptr[t]:indptr[t + 1]] for t in lst[lst >= 0])
    gs, ab = R.operand_grad_by_source(gcat, tp, ti, indptr)
    torch.testing.assert_close(gs, x.grad, **TOL)
    assert bool((ab >= gs.abs() - 1e-12).all())
    # the rank step's form: the mean half divided beforehand, no indptr
    g2 = gcat.clone()
    g2[:, H:] /= torch.from_numpy(np.diff(indptr)).double().clamp_min(1)[:, None]
    torch.testing.assert_close(R.operand_grad_by_source(g2, tp, ti, None)[0], x.grad, **TOL)
    # ReLU mask of the layer below + column sums
    y_below = torch.from_numpy(rng.standard_normal((n_src, H)))
    out, cs = R.masked_colsum(gd, y_below, 32)
    xb = y_below.clone().requires_grad_()
    (_autograd_operand(xb, indptr, indices, self_ids, None, True) * gcat).sum().backward()
    torch.testing.assert_close(out[:n_src], xb.grad, **TOL)
    assert bool((out[n_src:] == 0).all())
    torch.testing.assert_close(cs, xb.grad.sum(0), **TOL)
    out_u, _ = R.masked_colsum(gd, None, n_src)
    torch.testing.assert_close(out_u, gd, **TOL)


def test_spmm_gather_and_their_gradients():
    rng = np.random.default_rng(3)
    n, n_src, H = 17, 11, 3
    indptr, indices, _ = _csr(rng, n, n_src, 5)
    x = torch.from_numpy(rng.standard_normal((n_src, H))).requires_grad_()
    g = torch.from_numpy(rng.standard_normal((n, H)))
    want = torch.stack([x[torch.from_numpy(indices[indptr[r]:indptr[r + 1]])].sum(0) for r in range(n)])
    torch.testing.assert_close(R.spmm_sum(x.detach(), indptr, indices), want.detach(), **TOL)
    (want * g).sum().backward()
    torch.testing.assert_close(R.spmm_sum_bwd(g, indptr, indices, n_src), x.grad, **TOL)
    idx = np.array([3, -1, 0, 3, 10])
    got = R.gather_rows(x.detach(), idx)
    assert bool((got[1] == 0).all()) and torch.equal(got[[0, 2, 3, 4]], x.detach()[[3, 0, 3, 10]])


@pytest.mark.parametrize("C", [1, 2, 47])
@pytest.mark.parametrize("shift", [0.0, 80.0, -80.0])
def test_softmax_cross_entropy(C, shift):
    rng = np.random.default_rng(C)
    n, n_pad, scale = 13, 16, 1.0 / 29
    z = torch.from_numpy(rng.standard_normal((n_pad, C)) * 3 + shift).requires_grad_()
    lab = rng.integers(0, C, size=n)
    loss, grad, cs = R.softmax_ce(z.detach(), lab, scale, n_pad)
    want = torch.nn.functional.cross_entropy(z[:n], torch.from_numpy(lab), reduction="sum") * scale
    want.backward()
    assert abs(loss - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    torch.testing.assert_close(grad, z.grad, **TOL)
    assert bool((grad[n:] == 0).all())
    torch.testing.assert_close(cs, z.grad.sum(0), **TOL)


@pytest.mark.parametrize("L", [1, 2, 4])
def test_whole_model_by_hand_equals_autograd(L):
    rng = np.random.default_rng(10 + L)
    dims = [8] + [12] * (L - 1) + [5]
    sizes = [60 // (k + 1) for k in range(L + 1)]           # sources of layer 0 ... rows of the last layer
    layers = []
    for k in range(L):
        indptr, indices, self_ids = _csr(rng, sizes[k + 1], sizes[k], 5, no_self_every=4)
        layers.append({"indptr": indptr, "indices": indices, "self_ids": self_ids, "n_src": sizes[k]})
    x0 = rng.standard_normal((sizes[0], dims[0]))
    labels = rng.integers(0, dims[-1], size=sizes[L])
    ws = [rng.standard_normal((dims[k + 1], 2 * dims[k])) / 3 for k in range(L)]
    bs = [rng.standard_normal(dims[k + 1]) for k in range(L)]
    loss, grads = R.model_on_layers(layers, x0, labels, ws, bs, 1.0 / 7)
    loss_a, grads_a = R.model_autograd(layers, x0, labels, ws, bs, 1.0 / 7)
    assert abs(loss - loss_a) <= 1e-12 * abs(loss_a)
    assert len(grads) == len(grads_a) == 2 * L
    for g, ga in zip(grads, grads_a):
        assert float(ga.abs().max()) > 0
        torch.testing.assert_close(g, ga, **TOL)


def test_traversal_layers_on_the_oracle():
    """the oracle's traversal as layer CSRs: sizes chain, every row's self id names itself, no self loop survives"""
    from oracle import oracle as orc
    rng = np.random.default_rng(0)
    n = 300
    deg = rng.integers(0, 9, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)
    o = orc.Oracle(indptr, indices, n_parts=1, fanouts=(3, 4))
    trav = o.sample(rng.permutation(n)[:16])
    layers = R.traversal_layers(trav, n)
    assert len(layers) == 2 and layers[0]["n_src"] == len(trav["frontier"][2])
    assert layers[1]["n_src"] == len(layers[0]["indptr"]) - 1 == len(trav["frontier"][1])
    for ly in layers:
        rows = np.repeat(np.arange(len(ly["indptr"]) - 1), np.diff(ly["indptr"]))
        assert np.array_equal(ly["src_nodes"][ly["self_ids"]], ly["out_nodes"])
        assert (ly["indices"] != ly["self_ids"][rows]).all()
    feats, labels = rng.standard_normal((n, 4)), rng.integers(0, 3, size=n)
    ws = [rng.standard_normal((6, 8)), rng.standard_normal((3, 12))]
    bs = [rng.standard_normal(6), rng.standard_normal(3)]
    a = R.model_on_traversal(trav, feats, labels, ws, bs, n)
    b = R.model_on_traversal(trav, feats, labels, ws, bs, n, autograd=True)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0])
    for g, ga in zip(a[1], b[1]):
        torch.testing.assert_close(g, ga, **TOL)
