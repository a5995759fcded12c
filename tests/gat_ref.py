"""The attention (GAT) definitions restated in float64 with torch index ops, over an arbitrary CSR: what the GAT kernels
(include/cslicer_aggr.h: csl_gat_fwd_f32 / csl_gat_bwd_f32, csl_gat_in_*) are pinned against.  Gradients come from
autograd on these functions.  (The whole sampled model on the oracle's traversal: test_gpu_gat._dense_gat_vectorised.)

    score[e, h] = LeakyReLU_slope(el[src_e, h] + er[r, h])          for the edges e of destination row r
    m = max_e score,  s = sum_e exp(score - m),  n[h, :] = sum_e exp(score - m) z[src_e, h, :]
    out[r] = act(n / s + bias)                                        (a row without edges: act(bias))
"""
import torch


def csr_rows(indptr):
    """the destination row of every edge of the CSR"""
    deg = (indptr[1:] - indptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(deg.numel(), device=indptr.device), deg)


def partial_state(el, er, z, indptr, indices, H, D, slope, m=None):
    """(m, s, n) of the rows: el [n_src, H], er [n_rows, H], z [n_src, H*D].  m: the stabiliser to use (e.g. the
    kernel's own, so that s and n are comparable entry by entry); by default the row maximum (-1e30 for an empty row, the
    kernel's convention).  m is not differentiated, as in the kernels."""
    n_rows = indptr.numel() - 1
    rows, src = csr_rows(indptr), indices.long()
    score = torch.nn.functional.leaky_relu(el[src] + er[rows], slope)                       # [E, H]
    if m is None:
        m = torch.full((n_rows, H), -1e30, dtype=z.dtype, device=z.device).scatter_reduce(
            0, rows[:, None].expand(-1, H), score.detach(), "amax", include_self=True)
    m = m.detach().to(z.dtype)
    p = torch.exp(score - m[rows])
    s = torch.zeros((n_rows, H), dtype=z.dtype, device=z.device).index_add(0, rows, p)
    n = torch.zeros((n_rows, H, D), dtype=z.dtype, device=z.device).index_add(0, rows, p[:, :, None] * z[src].view(-1, H, D))
    return m, s, n.reshape(n_rows, H * D)


def finish(n, s, bias, H, D, elu):
    """act(n / s + bias) per head (n = s = 0 for a row without edges: the bias)"""
    out = (n.view(-1, H, D) / s.clamp_min(1e-300)[:, :, None]).reshape(-1, H * D) + bias
    return torch.nn.functional.elu(out) if elu else out


def _self_rows(v, self_ids):
    """v[self_ids[r]] per destination row, a zero row where self_ids[r] = -1"""
    sid = self_ids.long()
    return torch.where((sid >= 0)[:, None], v[sid.clamp_min(0)], torch.zeros_like(v[:1]))


def layer(x, weight, attn_l, attn_r, bias, indptr, indices, self_ids, slope, elu):
    """A whole DistGATConv layer (aggr.GatLayerLocal) project-then-aggregate: z = x W^T, el = <z, a_l>, er = <z, a_r>
    per head, a destination's er from its self row (0 without one)."""
    H, D = attn_l.shape
    z = x @ weight.t()
    zv = z.view(-1, H, D)
    el, er = (zv * attn_l).sum(-1), (zv * attn_r).sum(-1)
    _, s, n = partial_state(el, _self_rows(er, self_ids), z, indptr, indices, H, D, slope)
    return finish(n, s, bias, H, D, elu)


def input_layer(table, rows, weight, attn_l, attn_r, bias, indptr, indices, self_ids, slope, elu):
    """aggr.GatInputLayer's aggregate-then-project form on the feature table read through `rows` (source i is
    table[rows[i]]): v_l[h] = W_h^T a_l[h], el[u] = <x[u], v_l>, er[r] = <x[self(r)], v_r> (0 without a self row),
    agg[r, h] = sum_e alpha[e, h] x[src_e], out[r, h] = act(W_h agg[r, h] + bias)."""
    H, D = attn_l.shape
    x = table[rows.long()] if rows is not None else table
    F = x.shape[1]
    Wv = weight.view(H, D, F)
    vl, vr = torch.einsum("hdf,hd->hf", Wv, attn_l), torch.einsum("hdf,hd->hf", Wv, attn_r)
    el, er = x @ vl.t(), _self_rows(x @ vr.t(), self_ids)                                   # [n_src, H], [n_rows, H]
    xh = x[:, None, :].expand(-1, H, -1).reshape(-1, H * F)                                 # the raw row once per head
    _, s, agg = partial_state(el, er, xh, indptr, indices, H, F, slope)
    agg = agg.view(-1, H, F) / s.clamp_min(1e-300)[:, :, None]
    out = torch.einsum("rhf,hdf->rhd", agg, Wv).reshape(-1, H * D) + bias
    return torch.nn.functional.elu(out) if elu else out
