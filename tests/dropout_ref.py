"""Dropout between the GraphSAGE layers (include/cslicer_dropout.h) restated in numpy: Philox4x32-10, the
keep mask of a block of rows, and the float64 forward / backward of the model of tests/sage_ref.py with that mask on every
hidden layer's output.  No project kernel, no GPU.

    (w0..w3) = philox4x32_10(ctr = (c >> 2, v, k, t mod 2^32), key = (seed mod 2^32, (seed >> 32) mod 2^32))
    keep(v, c) = w[c & 3] >= T,  T = floor(float32(p) * 2^32);   y = keep ? x * s : 0,  s = float32(1 / (1 - float32(p)))
"""
import numpy as np
import torch

import sage_ref

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) that broadcast against each other; key: two ints.  Returns four uint64 arrays
    holding the 32-bit result words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(U32) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & U32, int(key[1]) & U32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]           # (32 x 32 bits: no overflow of the 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(U32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(U32)]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c


def threshold(p):
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def scale(p):
    """s as a float32"""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_mask(ids, H, p, seed, layer, step):
    """bool [len(ids), H]: the elements kept, rows keyed by the node ids `ids` (non-negative, below 2^32)"""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((H + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((q[None, :], ids[:, None], int(layer) & U32, step & U32), (seed & U32, seed >> 32))
    words = np.stack(w, axis=-1).reshape(ids.shape[0], -1)[:, :H]       # column c = word c & 3 of quad c >> 2
    return words >= np.uint64(threshold(p))


def apply(x, ids, p, seed, layer, step):
    """the map on a float32 matrix, in float32 (one multiplication, one rounding): what the kernel must give bit for bit"""
    x = np.asarray(x, dtype=np.float32)
    keep = keep_mask(ids, x.shape[1], p, seed, layer, step)
    return np.where(keep, x * scale(p), np.float32(0)).astype(np.float32)


def model_on_layers(layers, x0, labels, weights, biases, loss_scale, p, seed, step):
    """sage_ref.model_on_layers with dropout on the output of every layer but the last (after its ReLU), rows keyed by the
    layer's out_nodes: loss and [gW_0, gb_0, gW_1, ...] in float64, backward written out by hand.
        h_k = relu(cat_k W_k^T + b_k) * keep_k * s         dh_k / dy_k = (y_k > 0) * keep_k * s = (h_k > 0) * s"""
    F64 = sage_ref.F64
    L = len(layers)
    ws = [sage_ref._t(w.detach().cpu() if torch.is_tensor(w) else w, F64) for w in weights]
    bs = [sage_ref._t(b.detach().cpu() if torch.is_tensor(b) else b, F64) for b in biases]
    s = float(scale(p))
    h = sage_ref._t(x0, F64)
    cats, hs = [], []
    for k, ly in enumerate(layers):
        cat = sage_ref.operand(h, ly["indptr"], ly["indices"], ly["self_ids"])
        h = sage_ref.layer_out(cat, ws[k], bs[k], relu_out=k + 1 < L)
        if k + 1 < L:
            keep = keep_mask(ly["out_nodes"], h.shape[1], p, seed, k, step)
            h = h * torch.from_numpy(keep).to(F64) * s
        cats.append(cat)
        hs.append(h)
    loss, gy, gb = sage_ref.softmax_ce(h, labels, loss_scale)
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


def model_on_traversal(trav, feats, labels, weights, biases, n_nodes, p, seed, step):
    """loss (mean over the seeds) and parameter gradients on the sequential sampler's traversal (sage_ref.traversal_layers)"""
    layers = sage_ref.traversal_layers(trav, n_nodes)
    seeds = np.asarray(trav["frontier"][0], dtype=np.int64)
    x0 = np.asarray(feats)[layers[0]["src_nodes"]]
    return model_on_layers(layers, x0, np.asarray(labels)[seeds], weights, biases, 1.0 / seeds.shape[0], p, seed, step)
