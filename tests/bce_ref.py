"""The multi-label loss and evaluation head (include/cslicer_multilabel.h) restated in float64 numpy / torch:
packed labels, the element-wise loss and gradient, the kernel's block partials and column sums, micro-F1 counts, and the
float64 forward / backward of the model of tests/sage_ref.py with that loss (dropout of tests/dropout_ref.py optional).  No
project kernel, no GPU.

    e = exp(-|z|);  l = max(z, 0) - (y ? z : 0) + log1p(e);  sigma = z >= 0 ? 1 / (1 + e) : e / (1 + e)
    grad = scale (sigma - y);  loss of a row = scale sum_c l;  class c = bit c % 32 of word c / 32
"""
import numpy as np
import torch

import dropout_ref
import sage_ref

F64 = torch.float64


def pack(y):
    """bool / 0-1 [n, C] -> uint32 [n, ceil(C / 32)], bit by bit (the slow, obvious way)"""
    y = np.asarray(y).astype(bool)
    n, C = y.shape
    w = np.zeros((n, (C + 31) // 32), dtype=np.uint64)
    for c in range(C):
        w[:, c // 32] |= y[:, c].astype(np.uint64) << np.uint64(c % 32)
    return w.astype(np.uint32)


def unpack(words, C):
    w = np.asarray(words).view(np.uint32) if np.asarray(words).dtype == np.int32 else np.asarray(words, dtype=np.uint32)
    c = np.arange(C)
    return ((w[:, c // 32] >> (c % 32).astype(np.uint32)) & 1).astype(bool)


def elements(z, y):
    """(l, sigma) element by element in float64, the overflow-free form"""
    z = sage_ref._t(z, F64)
    y = torch.as_tensor(np.asarray(y).astype(np.float64))
    e = torch.exp(-z.abs())
    l = z.clamp_min(0) - y * z + torch.log1p(e)
    sig = torch.where(z >= 0, 1 / (1 + e), e / (1 + e))
    return l, sig


def sigmoid_bce(logits, y, scale, n_pad=None):
    """(loss, loss of every row [n] (scaled), grad [n_pad, C], colsum [C]) for the rows of y; rows of the gradient
    beyond them are padding: zero"""
    y = np.asarray(y).astype(bool)
    n = y.shape[0]
    z = sage_ref._t(logits, F64)[:n]
    n_pad = n if n_pad is None else n_pad
    l, sig = elements(z, y)
    rows = scale * l.sum(1)
    grad = torch.zeros((n_pad, z.shape[1]), dtype=F64)
    grad[:n] = scale * (sig - torch.as_tensor(y.astype(np.float64)))
    return float(rows.sum()), rows, grad, grad.sum(0)


def block_partials(rows, grad, n_pad):
    """(loss_partial [blocks], col_partial [blocks, C]) of blocks of four rows, blocks = ceil(n_pad / 4)"""
    blocks = (n_pad + 3) // 4
    r = torch.zeros(blocks * 4, dtype=F64)
    r[:rows.numel()] = rows
    g = torch.zeros((blocks * 4, grad.shape[1]), dtype=F64)
    g[:grad.shape[0]] = grad
    return r.view(blocks, 4).sum(1), g.view(blocks, 4, -1).sum(1)


def eval_head(logits, y):
    """(pred bool [n, C], (tp, fp, fn), loss_row [n] float64 unscaled): a class is predicted where its logit is > 0"""
    z = np.asarray(logits)
    y = np.asarray(y).astype(bool)
    pred = z > 0
    l, _ = elements(z.astype(np.float64), y)
    return pred, (int((pred & y).sum()), int((pred & ~y).sum()), int((~pred & y).sum())), l.sum(1)


def micro_f1(tp, fp, fn):
    return 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0


def model_on_layers(layers, x0, y, weights, biases, loss_scale, drop=None):
    """dropout_ref.model_on_layers with the sigmoid-BCE loss on the last layer's rows (y: bool [rows, C]); drop: None or
    (p, seed, step).  Loss and [gW_0, gb_0, gW_1, ...] in float64, backward written out by hand."""
    L = len(layers)
    ws = [sage_ref._t(w.detach().cpu() if torch.is_tensor(w) else w, F64) for w in weights]
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
    loss, _, gy, gb = sigmoid_bce(h, y, loss_scale)
    grads = [None] * (2 * L)
    for k in range(L - 1, -1, -1):
        grads[2 * k], grads[2 * k + 1] = gy.t() @ cats[k], gb
        if k == 0:
            break
        ly = layers[k]
        gx = sage_ref.operand_grad_by_destination(gy @ ws[k], ly["indptr"], ly["indices"], ly["self_ids"], ly["n_src"])
        gy = gx * (hs[k - 1] > 0) * s
        gb = gy.sum(0)
    return loss, grads


def model_on_traversal(trav, feats, y, weights, biases, n_nodes, drop=None):
    """loss (mean over seeds x classes) and parameter gradients on the sequential sampler's traversal; y: bool [N, C]"""
    layers = sage_ref.traversal_layers(trav, n_nodes)
    seeds = np.asarray(trav["frontier"][0], dtype=np.int64)
    x0 = np.asarray(feats)[layers[0]["src_nodes"]]
    y = np.asarray(y)
    return model_on_layers(layers, x0, y[seeds], weights, biases, 1.0 / (seeds.shape[0] * y.shape[1]), drop)
