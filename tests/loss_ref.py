"""The class-weighted, label-smoothed softmax cross-entropy (include/cslicer_loss.h) restated in float64 with
plain torch ops, and the GraphSAGE model of tests/sage_ref.py with that loss (optionally with the dropout masks of
tests/dropout_ref.py).  No project kernel, no GPU.  The backward is written out by hand (that is what the kernels
implement); tests/test_loss_ref_cpu.py checks it against torch float64 autograd.

    q_c = w_c ((1 - eps) [c == y] + eps / C),   Q = sum_c q_c,   d_c = (max - z_c) + log sum exp(z - max)
    loss_row = scale sum_c q_c d_c,             grad_c = scale (softmax(z)_c Q - q_c)
"""
import numpy as np
import torch

import dropout_ref
import sage_ref
from tail_ref import _f32, _t

F64 = torch.float64


def target(lab, C, w, eps):
    """q [n, C] in float64 for labels in [0, C) (w None: all ones; eps as the float32 that is passed)"""
    lab = _t(lab, torch.int64)
    eps = _f32(eps)
    q = torch.full((lab.numel(), C), eps / C, dtype=F64)
    q[torch.arange(lab.numel()), lab] += 1.0 - eps
    return q if w is None else q * _t(w, F64)[None, :]


def rows_ce(z, lab, w, eps, scale, n_pad=None):
    """(loss_rows [n], grad [n_pad, C], Q [n], terms_abs [n]) of the logits z [>= n, C] against labels in [0, C); scale
    as given (float64).  terms_abs: sum_c |q_c d_c|, the unscaled loss itself (every term is >= 0)."""
    lab = _t(lab, torch.int64)
    n = lab.numel()
    z = _t(z, F64)[:n]
    C = z.shape[1]
    n_pad = n if n_pad is None else n_pad
    q = target(lab, C, w, eps)
    m = z.max(1, keepdim=True).values if n else z.new_zeros((0, 1))
    e = torch.exp(z - m)
    s = e.sum(1, keepdim=True)
    d = (m - z) + torch.log(s)
    Q = q.sum(1)
    terms = (q * d).sum(1)
    grad = torch.zeros((n_pad, C), dtype=F64)
    grad[:n] = scale * (e / s * Q[:, None] - q)
    return scale * terms, grad, Q, terms


def weighted_ce(logits, ldl, n, n_pad, C, ids, rowmap, labels, w, eps, scale, grad=None, ldgr=None):
    """csl_softmax_ce_w_partial_f32 on flat buffers, as tail_ref.softmax_ce restates the plain loss: row r < n of the
    logits is logits[r * ldl : r * ldl + C], its label labels[rowmap[ids[r]]] (rowmap None: labels[ids[r]]); scale and eps
    as the float32 that are passed; w: [C] or None.  Rows [n, n_pad) of the gradient are zero.
    A label outside [0, C): that row's loss is NaN and its gradient row is NaN (so are the sums they enter).
    grad / ldgr: an optional flat float64 buffer the gradient rows are also written into, row r at r * ldgr.
    Returns (loss_rows [n], grad [n_pad, C], colsum [C], Q [n], terms_abs [n]); the loss of the call is loss_rows.sum()."""
    flat = _t(logits, F64).reshape(-1)
    scale = _f32(scale)
    idx = _t(ids, torch.int64)[:n]
    if rowmap is not None:
        idx = _t(rowmap, torch.int64)[idx]
    lab = _t(labels, torch.int64)[idx]
    rows = torch.arange(n)
    z = flat[(rows[:, None] * ldl + torch.arange(C)[None, :]).reshape(-1)].reshape(n, C)
    bad = (lab < 0) | (lab >= C)
    safe = torch.where(bad, torch.zeros_like(lab), lab)
    loss_rows, g, Q, terms = rows_ce(z, safe, w, eps, scale, n_pad)
    loss_rows[bad] = float("nan")
    g[:n][bad] = float("nan")
    if grad is not None:
        cells = (torch.arange(n_pad)[:, None] * ldgr + torch.arange(C)[None, :]).reshape(-1)
        grad.reshape(-1)[cells] = g.reshape(-1)
    return loss_rows, g, g.sum(0), Q, terms


def model_on_layers(layers, x0, labels, weights, biases, loss_scale, w=None, eps=0.0, drop=None):
    """sage_ref.model_on_layers with the weighted, smoothed loss: loss and [gW_0, gb_0, gW_1, ...] in float64.
    drop: None or (p, seed, step): dropout on the output of every layer but the last, rows keyed by the layer's out_nodes
    (dropout_ref.keep_mask), as dropout_ref.model_on_layers has it."""
    L = len(layers)
    ws = [sage_ref._t(x.detach().cpu() if torch.is_tensor(x) else x, F64) for x in weights]
    bs = [sage_ref._t(b.detach().cpu() if torch.is_tensor(b) else b, F64) for b in biases]
    s = float(dropout_ref.scale(drop[0])) if drop else 1.0
    h = sage_ref._t(x0, F64)
    cats, hs = [], []
    for k, ly in enumerate(layers):
        cat = sage_ref.operand(h, ly["indptr"], ly["indices"], ly["self_ids"])
        h = sage_ref.layer_out(cat, ws[k], bs[k], relu_out=k + 1 < L)
        if drop and k + 1 < L:
            keep = dropout_ref.keep_mask(ly["out_nodes"], h.shape[1], drop[0], drop[1], k, drop[2])
            h = h * torch.from_numpy(keep).to(F64) * s
        cats.append(cat)
        hs.append(h)
    loss_rows, gy, _, _ = rows_ce(h, labels, w, eps, float(loss_scale))
    gb = gy.sum(0)
    grads = [None] * (2 * L)
    for k in range(L - 1, -1, -1):
        grads[2 * k], grads[2 * k + 1] = gy.t() @ cats[k], gb
        if k == 0:
            break
        ly = layers[k]
        gx = sage_ref.operand_grad_by_destination(gy @ ws[k], ly["indptr"], ly["indices"], ly["self_ids"], ly["n_src"])
        gy = gx * (hs[k - 1] > 0) * s
        gb = gy.sum(0)
    return float(loss_rows.sum()), grads


def model_on_traversal(trav, feats, labels, weights, biases, n_nodes, w=None, eps=0.0, drop=None):
    """loss (the weighted, smoothed sum over the seeds / their count) and parameter gradients on the sequential sampler's
    traversal (sage_ref.traversal_layers)"""
    layers = sage_ref.traversal_layers(trav, n_nodes)
    seeds = np.asarray(trav["frontier"][0], dtype=np.int64)
    x0 = np.asarray(feats)[layers[0]["src_nodes"]]
    return model_on_layers(layers, x0, np.asarray(labels)[seeds], weights, biases, 1.0 / seeds.shape[0], w, eps, drop)
