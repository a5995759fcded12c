"""Layer normalisation between the GraphSAGE layers (include/cslicer_layernorm.h) restated in float64 numpy:
the forward and the hand-written backward of one block of rows, the rounding bounds of their float32 evaluation counted
from the kernels' operation sequence, and the float64 model of tests/sage_ref.py with the norm on every layer but the last.
No project kernel, no GPU.  tests/test_norm_cpu.py pins forward / backward to torch.nn.functional.layer_norm + relu under
float64 autograd.

    mean = sum(z) / H,  var = sum((z - mean)^2) / H  (biased),  rstd = 1 / sqrt(var + eps),  xhat = (z - mean) * rstd
    n = gamma * xhat + beta,  y = relu(n)
    a = gamma * dn:  dz = rstd * (a - mean_row(a) - xhat * mean_row(a * xhat)),  dgamma = sum_rows dn * xhat
"""
import numpy as np
import torch

import bce_ref
import dropout_ref
import loss_ref
import sage_ref

U = 2.0 ** -24      # the unit roundoff of float32


def _f64(a):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)


def forward(z, gamma, beta, eps, relu=True):
    """(y, xhat, rstd) in float64; eps as the float32 that is passed"""
    z, gamma, beta = _f64(z), _f64(gamma), _f64(beta)
    eps = float(np.float32(eps))
    mean = z.mean(1, keepdims=True)
    c = z - mean
    rstd = 1.0 / np.sqrt((c * c).mean(1, keepdims=True) + eps)
    xhat = c * rstd
    n = gamma[None, :] * xhat + beta[None, :]
    return (np.maximum(n, 0.0) if relu else n), xhat, rstd[:, 0]


def backward(dn, xhat, rstd, gamma):
    """(dz, dgamma, column sums of dz) in float64 from the gradient dn w.r.t. the normalised row (ReLU mask applied)"""
    dn, xhat, rstd, gamma = _f64(dn), _f64(xhat), _f64(rstd), _f64(gamma)
    a = gamma[None, :] * dn
    dz = rstd[:, None] * (a - a.mean(1, keepdims=True) - xhat * (a * xhat).mean(1, keepdims=True))
    return dz, (dn * xhat).sum(0), dz.sum(0)


# ---- rounding bounds of the kernels' float32 evaluation (first order in U, times 1.01 for the higher orders).
# A row of H = 4 hq values is summed as: (x + y) + (z + w) inside a quad (2 additions deep), the lane's quads one after
# another (nq = ceil(hq / lanes)), then lg butterfly steps across the 2^lg lanes: an element passes through
# d = 2 + nq + lg additions, so |fl(sum) - sum| <= d U sum|terms|; the division by H adds one rounding.

def lanes_lg(H):
    hq, lg = H // 4, 0
    while lg < 6 and (1 << lg) < hq:
        lg += 1
    return lg


def sum_depth(H):
    lg = lanes_lg(H)
    return 2 + -(-(H // 4) // (1 << lg)) + lg


def forward_bounds(z, gamma, beta, eps, relu=True):
    """(bound on |y_kernel - y|, bound on |xhat_kernel - xhat|, bound on |rstd_kernel - rstd|) for float32 inputs z, gamma,
    beta, against forward() on the same values:
        mean:  delta = (d + 1) U max|z|                  (sum of H terms d deep, one division)
        c_i = fl(z_i - mean):  |c_i^ - c_i| <= delta + U (|c_i| + delta)
        v = sum c^2 / H:  the shift by the mean's error adds at most delta^2 (sum c_i = 0), the squares, the d-deep sum
            and the division (d + 2) U relative, the errors of the c_i 2 U relative:  rho_v = (d + 5) U + delta^2 / (var + eps)
        rstd = 1 / sqrt(v + eps): one addition, one square root and one division of at most 2 U each:  rho_r = rho_v / 2 + 5 U
        xhat_i = c_i^ * rstd^ (one rounding):  |.| <= rstd (delta + U (|c_i| + delta)) + |xhat_i| (rho_r + U)
        y_i = fma(gamma_i, xhat_i^, beta_i) (one rounding; the ReLU is 1-Lipschitz):  |gamma_i| err(xhat_i) + U |n_i|"""
    z64, g64, b64 = _f64(z), _f64(gamma), _f64(beta)
    H = z64.shape[1]
    d = sum_depth(H)
    n, xhat, rstd = forward(z64, g64, b64, eps, relu=False)
    c = z64 - z64.mean(1, keepdims=True)
    delta = (d + 1) * U * np.abs(z64).max(1, keepdims=True)
    rho_v = (d + 5) * U + delta ** 2 * rstd[:, None] ** 2
    rho_r = rho_v / 2 + 5 * U
    e_x = rstd[:, None] * (delta + U * (np.abs(c) + delta)) + np.abs(xhat) * (rho_r + U)
    e_y = np.abs(g64)[None, :] * e_x + U * np.abs(n)
    return 1.01 * e_y + 1e-37, 1.01 * e_x + 1e-37, 1.01 * rstd * rho_r[:, 0]


def backward_bounds(dn, xhat, rstd, gamma):
    """(bound on |dz_kernel - dz| [n, H], on the dgamma column sums [H], on the dz column sums [H]) for float32 inputs,
    against backward() on the same values.  a_i = fl(gamma_i dn_i): U |a_i|; m1 = fl(sum a / H): (d + 2) U mean|a|;
    m2 = fl(sum a xhat / H): (d + 3) U mean|a xhat|; then a subtraction, a product, a subtraction and the product by rstd:
        |dz_i^ - dz_i| <= (d + 8) U rstd (|a_i| + mean|a| + |xhat_i| mean|a xhat|)
    A column sum over n rows in ANY order is within (n - 1) U of the sum of its |terms|, its terms' own errors on top."""
    dn, xhat, rstd, gamma = _f64(dn), _f64(xhat), _f64(rstd), _f64(gamma)
    n, H = dn.shape
    d = sum_depth(H)
    a = np.abs(gamma[None, :] * dn)
    ax = a * np.abs(xhat)
    e_dz = (d + 8) * U * rstd[:, None] * (a + a.mean(1, keepdims=True) + np.abs(xhat) * ax.mean(1, keepdims=True))
    dz = backward(dn, xhat, rstd, gamma)[0]
    e_g = (n + 1) * U * np.abs(dn * xhat).sum(0)
    e_b = e_dz.sum(0) + n * U * (np.abs(dz) + e_dz).sum(0)
    return 1.01 * e_dz + 1e-37, 1.01 * e_g + 1e-37, 1.01 * e_b + 1e-37


# ---- the model

def model_on_layers(layers, x0, target, weights, biases, gammas, betas, eps, loss_scale, w=None, smoothing=0.0, drop=None,
                    multilabel=False):
    """sage_ref.model_on_layers with h_k = dropout(relu(layer_norm(cat_k W_k^T + b_k) * gamma_k + beta_k)) for k < L-1.
    target: int labels of the last layer's rows, or (multilabel) bool [rows, C]; w / smoothing: loss_ref's class weights
    and label smoothing; drop: None or (p, seed, step) as dropout_ref has it.  Returns the loss and
    [gW_0, gb_0, ..., gW_{L-1}, gb_{L-1}, ggamma_0, gbeta_0, ggamma_1, gbeta_1, ...] in float64, backward by hand."""
    F64 = sage_ref.F64
    L = len(layers)
    t = lambda a: sage_ref._t(a.detach().cpu() if torch.is_tensor(a) else a, F64)     # noqa: E731
    ws, bs, gs, be = [t(a) for a in weights], [t(a) for a in biases], [t(a) for a in gammas], [t(a) for a in betas]
    s = float(dropout_ref.scale(drop[0])) if drop else 1.0
    h = t(x0)
    cats, hs, xh, rs = [], [], [], []
    for k, ly in enumerate(layers):
        cat = sage_ref.operand(h, ly["indptr"], ly["indices"], ly["self_ids"])
        h = sage_ref.layer_out(cat, ws[k], bs[k], relu_out=False)
        if k + 1 < L:
            y, xhat, rstd = forward(h.numpy(), gs[k].numpy(), be[k].numpy(), eps)
            h = torch.from_numpy(y)
            xh.append(xhat)
            rs.append(rstd)
            if drop:
                keep = dropout_ref.keep_mask(ly["out_nodes"], h.shape[1], drop[0], drop[1], k, drop[2])
                h = h * torch.from_numpy(keep).to(F64) * s
        cats.append(cat)
        hs.append(h)
    if multilabel:
        loss, _, gy, _ = bce_ref.sigmoid_bce(h, target, loss_scale)
    else:
        loss_rows, gy, _, _ = loss_ref.rows_ce(h, target, w, smoothing, float(loss_scale))
        loss = float(loss_rows.sum())
    gb = gy.sum(0)
    grads, ngrads = [None] * (2 * L), [None] * (2 * (L - 1))
    for k in range(L - 1, -1, -1):
        grads[2 * k], grads[2 * k + 1] = gy.t() @ cats[k], gb
        if k == 0:
            break
        ly = layers[k]
        gx = sage_ref.operand_grad_by_destination(gy @ ws[k], ly["indptr"], ly["indices"], ly["self_ids"], ly["n_src"])
        dn = (gx * (hs[k - 1] > 0) * s).numpy()
        dz, dgamma, colsum = backward(dn, xh[k - 1], rs[k - 1], gs[k - 1].numpy())
        ngrads[2 * (k - 1)], ngrads[2 * (k - 1) + 1] = torch.from_numpy(dgamma), torch.from_numpy(dn.sum(0))
        gy, gb = torch.from_numpy(dz), torch.from_numpy(colsum)
    return loss, grads + ngrads


def model_on_traversal(trav, feats, target, weights, biases, gammas, betas, eps, n_nodes, **kw):
    """loss and gradients on the sequential sampler's traversal (sage_ref.traversal_layers); the loss is the mean over the
    seeds (multilabel: over seeds x classes)"""
    layers = sage_ref.traversal_layers(trav, n_nodes)
    seeds = np.asarray(trav["frontier"][0], dtype=np.int64)
    x0 = np.asarray(feats)[layers[0]["src_nodes"]]
    target = np.asarray(target)
    den = seeds.shape[0] * (target.shape[1] if kw.get("multilabel") else 1)
    return model_on_layers(layers, x0, target[seeds], weights, biases, gammas, betas, eps, 1.0 / den, **kw)


def logits_on_layers(layers, x0, weights, biases, gammas, betas, eps):
    """the forward alone (no dropout): the last layer's rows in float64"""
    F64 = sage_ref.F64
    t = lambda a: sage_ref._t(a.detach().cpu() if torch.is_tensor(a) else a, F64)     # noqa: E731
    h = t(x0)
    L = len(layers)
    for k, ly in enumerate(layers):
        cat = sage_ref.operand(h, ly["indptr"], ly["indices"], ly["self_ids"])
        h = sage_ref.layer_out(cat, t(weights[k]), t(biases[k]), relu_out=False)
        if k + 1 < L:
            h = torch.from_numpy(forward(h.numpy(), _f64(gammas[k]), _f64(betas[k]), eps)[0])
    return h


def infer_model(m, features, indptr, indices, nodes=None):
    """float64 logits of a (normalised) DistSAGEModel by full-neighbour inference: infer_ref.model with the norm on every
    layer but the last"""
    import infer_ref
    ip, ix = infer_ref.neighbour_csr(indptr, indices)
    h = torch.as_tensor(features).double().cpu()
    L = len(m.convs)
    normed = getattr(m, "norm", None) is not None
    for k, conv in enumerate(m.convs):
        last = k + 1 == L
        w, b = conv.fc.weight.detach().cpu(), conv.fc.bias.detach().cpu()
        h = infer_ref.sage_layer(h, w, b, ip, ix, not last and not normed, nodes if last else None)
        if normed and not last:
            h = torch.from_numpy(forward(h.numpy(), m.norms[k].gamma, m.norms[k].beta, m.norm_eps)[0])
    return h
