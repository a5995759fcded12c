"""The GraphSAGE definitions restated in float64 with plain numpy / torch index ops, over an arbitrary CSR: what the SAGE
kernels (include/cslicer_aggr.h: csl_sage_fwd_mfma_f32, csl_sage_cat_*, csl_spmm_sum_*, csl_softmax_ce_*, the native
steps) are pinned against.  No project kernel, no GPU.  The backward formulas are written out by hand (that is what the
kernels implement); tests/test_sage_ref_cpu.py checks them against torch float64 autograd, so that a wrong restatement
cannot hide a wrong kernel.

    cat[r, 0:H)  = act(x[map(self_ids[r])])                        (a zero row for self_ids[r] = -1)
    cat[r, H:2H) = sum_{e in row r} act(x[map(indices[e])]) / max(deg_r, 1)
    y[r]         = act_out(cat[r] W^T + b)                         rows [n, n_pad): cat = 0, y = act_out(b)
    loss         = -scale sum_r log softmax(y[r])[label_r]
"""
import numpy as np
import torch

F64 = torch.float64


def _t(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dtype) if dtype is not None else t


def csr_rows(indptr):
    """the destination row of every edge of the CSR"""
    ip = _t(indptr, torch.int64)
    deg = ip[1:] - ip[:-1]
    return torch.repeat_interleave(torch.arange(deg.numel()), deg)


def spmm_sum(x, indptr, indices, rowmap=None):
    """out[r] = sum over the edges of CSR row r of x[map(indices[e])]"""
    x = _t(x, F64)
    src = _t(indices, torch.int64)
    if rowmap is not None:
        src = _t(rowmap, torch.int64)[src]
    n = len(indptr) - 1
    return torch.zeros((n, x.shape[1]), dtype=F64).index_add_(0, csr_rows(indptr), x[src])


def spmm_sum_bwd(g, indptr, indices, n_src):
    """gradient of spmm_sum w.r.t. x (no row map): gx[indices[e]] += g[row of e]"""
    g = _t(g, F64)
    return torch.zeros((n_src, g.shape[1]), dtype=F64).index_add_(0, _t(indices, torch.int64), g[csr_rows(indptr)])


def gather_rows(src, idx):
    """dst[k] = src[idx[k]], a zero row for idx[k] = -1"""
    src, idx = _t(src, F64), _t(idx, torch.int64)
    return torch.where((idx >= 0)[:, None], src[idx.clamp_min(0)], torch.zeros((1, src.shape[1]), dtype=F64))


def operand(x, indptr, indices, self_ids, n_pad=None, rowmap=None, relu_in=False, deg=None):
    """[self | mean] operand [n_pad, 2H].  deg: the divisors (default the CSR row lengths), floored at 1."""
    x = _t(x, F64)
    if relu_in:
        x = x.clamp_min(0)
    n, H = len(indptr) - 1, x.shape[1]
    n_pad = n if n_pad is None else n_pad
    sid = _t(self_ids, torch.int64)
    rows = sid.clamp_min(0)
    if rowmap is not None:
        rows = _t(rowmap, torch.int64)[rows]
    d = _t(np.diff(np.asarray(indptr)) if deg is None else deg, F64).clamp_min(1)
    cat = torch.zeros((n_pad, 2 * H), dtype=F64)
    cat[:n, :H] = torch.where((sid >= 0)[:, None], x[rows], torch.zeros((1, H), dtype=F64))
    cat[:n, H:] = spmm_sum(x, indptr, indices, rowmap) / d[:, None]
    return cat


def layer_out(cat, weight, bias=None, relu_out=False):
    """act(cat W^T + b) for every row of cat (padding rows included: act(b))"""
    y = _t(cat, F64) @ _t(weight, F64).t()
    if bias is not None:
        y = y + _t(bias, F64)
    return y.clamp_min(0) if relu_out else y


def operand_grad_by_destination(gcat, indptr, indices, self_ids, n_src, deg=None):
    """gx [n_src, H] from gcat [>= n, 2H], walking the destination rows: gx[self_ids[r]] += gcat[r, :H],
    gx[indices[e]] += gcat[r, H:] / max(deg_r, 1)"""
    n = len(indptr) - 1
    g = _t(gcat, F64)[:n]
    H = g.shape[1] // 2
    sid = _t(self_ids, torch.int64)
    d = _t(np.diff(np.asarray(indptr)) if deg is None else deg, F64).clamp_min(1)
    gx = torch.zeros((n_src, H), dtype=F64)
    has = sid >= 0
    gx.index_add_(0, sid[has], g[has, :H])
    gx.index_add_(0, _t(indices, torch.int64), (g[:, H:] / d[:, None])[csr_rows(indptr)])
    return gx


def by_source(indptr, indices, self_ids, n_src):
    """The slice by source (cslicer_hip.h CSL_T_INDPTR / CSL_T_INDICES) of a CSR with self ids, in numpy: per source u
    the destination rows that read it -- ~r (negative) where u is r's self row, r for every edge of r that names u --
    self entry first, then the edges in edge order.  Returns int64 (t_indptr [n_src + 1], t_indices)."""
    indptr, indices, self_ids = (np.asarray(a, dtype=np.int64) for a in (indptr, indices, self_ids))
    n = indptr.shape[0] - 1
    has = self_ids >= 0
    src = np.concatenate([self_ids[has], indices])
    ent = np.concatenate([~np.arange(n, dtype=np.int64)[has], np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))])
    order = np.argsort(src, kind="stable")
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n_src), out=t_indptr[1:])
    return t_indptr, ent[order]


def operand_grad_by_source(gcat, t_indptr, t_indices, indptr=None):
    """The same gradient as a gather over the slice by source; indptr None: the mean half of gcat is already divided.
    Returns (gx [n_src, H], abs [n_src, H]): abs is the sum of the |terms| of every entry (what a rounding bound of an
    fp32 summation in any order is made of)."""
    g = _t(gcat, F64)
    H = g.shape[1] // 2
    t = _t(t_indices, torch.int64)
    isself = t < 0
    r = torch.where(isself, ~t, t)
    if indptr is not None:
        d = _t(np.diff(np.asarray(indptr)), F64).clamp_min(1)
        mean = g[r, H:] / d[r][:, None]
    else:
        mean = g[r, H:]
    term = torch.where(isself[:, None], g[r, :H], mean)
    n_src = len(t_indptr) - 1
    u = csr_rows(t_indptr)
    gx = torch.zeros((n_src, H), dtype=F64).index_add_(0, u, term)
    ab = torch.zeros((n_src, H), dtype=F64).index_add_(0, u, term.abs())
    return gx, ab


def masked_colsum(g, y_below, n_pad):
    """(out [n_pad, H], colsum [H]): g masked by y_below > 0 (None: unmasked), zero padding rows, column sums: the ReLU
    backward of the layer below + its bias gradient"""
    g = _t(g, F64)
    n = g.shape[0]
    out = torch.zeros((n_pad, g.shape[1]), dtype=F64)
    out[:n] = g if y_below is None else g * (_t(y_below, F64)[:n] > 0)
    return out, out.sum(0)


def softmax_ce(logits, labels, scale, n_pad=None):
    """(loss, grad [n_pad, C], colsum [C]) of -scale sum_r log softmax(logits[r])[labels[r]] over the rows of `labels`;
    rows of logits beyond them are padding: zero gradient"""
    lab = _t(labels, torch.int64)
    n = lab.numel()
    z = _t(logits, F64)[:n]
    n_pad = n if n_pad is None else n_pad
    m = z.max(1, keepdim=True).values if n else z
    e = torch.exp(z - m)
    s = e.sum(1, keepdim=True)
    logp = z - m - torch.log(s)
    loss = -scale * logp[torch.arange(n), lab].sum()
    grad = torch.zeros((n_pad, z.shape[1]), dtype=F64)
    grad[:n] = e / s
    grad[torch.arange(n), lab] -= 1.0
    grad *= scale
    return float(loss), grad, grad.sum(0)


def traversal_layers(trav, n_nodes):
    """The oracle's traversal as one CSR per MODEL layer (deepest hop first): a list of dicts with indptr, indices,
    self_ids (all into the layer's source list, which is the frontier below) and n_src.  A sampled self loop is not a
    neighbour; every destination is its own self row."""
    L = len(trav["nbr_counts"])
    layers = []
    src_nodes = np.asarray(trav["frontier"][L], dtype=np.int64)
    for k in range(L):
        l = L - 1 - k
        fr = np.asarray(trav["frontier"][l], dtype=np.int64)
        counts = np.asarray(trav["nbr_counts"][l], dtype=np.int64)
        flat = np.asarray(trav["nbr_flat"][l], dtype=np.int64)
        lut = np.full(n_nodes, -1, dtype=np.int64)
        lut[src_nodes] = np.arange(src_nodes.shape[0])
        starts = np.zeros(fr.shape[0] + 1, dtype=np.int64)
        np.cumsum(counts, out=starts[1:])
        assert np.array_equal(flat[starts[:-1]], fr)                       # every list starts with the node itself
        keep = np.ones(flat.shape[0], dtype=bool)
        keep[starts[:-1]] = False
        row = np.repeat(np.arange(fr.shape[0]), counts)
        keep &= flat != fr[row]                                            # (a sampled self loop is not a neighbour)
        row, nb = row[keep], flat[keep]
        assert (lut[nb] >= 0).all() and (lut[fr] >= 0).all()
        indptr = np.zeros(fr.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(row, minlength=fr.shape[0]), out=indptr[1:])
        layers.append({"indptr": indptr, "indices": lut[nb], "self_ids": lut[fr], "n_src": src_nodes.shape[0],
                       "src_nodes": src_nodes, "out_nodes": fr})
        src_nodes = fr
    return layers


def model_on_layers(layers, x0, labels, weights, biases, scale):
    """Loss and parameter gradients [gW_0, gb_0, gW_1, ...] (float64, by the formulas above, no autograd) of the L-layer
    model (ReLU between the layers) on a list of layer CSRs (traversal_layers), x0 = the deepest layer's source rows,
    labels = those of the last layer's rows."""
    L = len(layers)
    ws, bs = [_t(w.detach().cpu() if torch.is_tensor(w) else w, F64) for w in weights], \
             [_t(b.detach().cpu() if torch.is_tensor(b) else b, F64) for b in biases]
    h = _t(x0, F64)
    cats, ys = [], []
    for k, ly in enumerate(layers):
        cat = operand(h, ly["indptr"], ly["indices"], ly["self_ids"], relu_in=k > 0)
        h = layer_out(cat, ws[k], bs[k])          # kept PRE-activation: the next layer applies the ReLU on the way in
        cats.append(cat)
        ys.append(h)
    loss, gy, gb = softmax_ce(h, labels, scale)
    grads = [None] * (2 * L)
    for k in range(L - 1, -1, -1):
        grads[2 * k], grads[2 * k + 1] = gy.t() @ cats[k], gb
        if k == 0:
            break
        gcat = gy @ ws[k]
        ly = layers[k]
        gx = operand_grad_by_destination(gcat, ly["indptr"], ly["indices"], ly["self_ids"], ly["n_src"])
        gy, gb = masked_colsum(gx, ys[k - 1], gx.shape[0])
    return loss, grads


def model_on_traversal(trav, feats, labels, weights, biases, n_nodes, autograd=False):
    """loss (mean over the seeds) and parameter gradients of the model on the oracle's traversal; autograd: through
    model_autograd below instead of the hand-written backward"""
    layers = traversal_layers(trav, n_nodes)
    seeds = np.asarray(trav["frontier"][0], dtype=np.int64)
    x0 = np.asarray(feats)[layers[0]["src_nodes"]]
    f = model_autograd if autograd else model_on_layers
    return f(layers, x0, np.asarray(labels)[seeds], weights, biases, 1.0 / seeds.shape[0])


def model_autograd(layers, x0, labels, weights, biases, scale):
    """The same model through torch float64 autograd (torch's own cross_entropy and relu): the independent statement the
    hand-written formulas above are checked against, and what test_gpu_step_bench_widths.py has always used."""
    ws = [_t(w.detach().cpu() if torch.is_tensor(w) else w, F64).clone().requires_grad_() for w in weights]
    bs = [_t(b.detach().cpu() if torch.is_tensor(b) else b, F64).clone().requires_grad_() for b in biases]
    h = _t(x0, F64)
    for k, ly in enumerate(layers):
        sid, idx = _t(ly["self_ids"], torch.int64), _t(ly["indices"], torch.int64)
        rows = csr_rows(ly["indptr"])
        n = sid.numel()
        agg = torch.zeros((n, h.shape[1]), dtype=F64).index_add(0, rows, h[idx])
        deg = torch.bincount(rows, minlength=n).double().clamp(min=1)
        cat = torch.cat([h[sid.clamp_min(0)] * (sid >= 0).double().unsqueeze(1), agg / deg.unsqueeze(1)], 1)
        h = cat @ ws[k].t() + bs[k]
        if k + 1 < len(layers):
            h = torch.relu(h)
    loss = torch.nn.functional.cross_entropy(h, _t(labels, torch.int64), reduction="sum") * scale
    loss.backward()
    grads = []
    for w, b in zip(ws, bs):
        grads += [w.grad, b.grad]
    return float(loss.detach()), grads
