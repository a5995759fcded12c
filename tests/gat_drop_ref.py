"""Dropout for the attention model (include/cslicer_gat_dropout.h) restated in float64 on top of gat_ref.py
and dropout_ref.py: the attention mask, the partial softmax state with a dropped numerator, a whole layer with both
dropouts, and the unsplit model on the oracle's traversal.  Gradients come from autograd on these functions.  No project
kernel, no GPU.

    kappa[e, h] = keep ? s_a : 0,  keep = w[h & 3] >= T of
        philox4x32_10(ctr = (u_e, v_e, 0x80000000 | (h >> 2) << 8 | k, t mod 2^32), key = the seed's halves)
    with u_e / v_e the NODE ids of the edge's source / destination
    n[h, :] = sum_e kappa p_e z[src_e, h, :],  s = sum_e p_e,  m as without dropout
    y = keep_f ? act(n / s + bias) * s_f : 0      (dropout_ref.keep_mask over all H * D columns, keyed by the out node)
"""
import numpy as np
import torch

import dropout_ref
import gat_ref

ATTN_BIT = 0x80000000


def attn_counter(u, v, h, layer, step):
    """the four counter words of edge (u -> v), head h (arrays broadcast), and the index of the head's result word"""
    h = np.asarray(h, dtype=np.uint64)
    w2 = np.uint64(ATTN_BIT) | ((h >> np.uint64(2)) << np.uint64(8)) | np.uint64(int(layer))
    return (u, v, w2, (int(step) & 0xFFFFFFFFFFFFFFFF) & dropout_ref.U32), h & np.uint64(3)


def attn_keep_edges(u, v, H, p, seed, layer, step):
    """bool [E, H]: the (edge, head) pairs kept, edges given by the node ids of their ends"""
    u = np.asarray(u, dtype=np.int64).astype(np.uint64)[:, None]
    v = np.asarray(v, dtype=np.int64).astype(np.uint64)[:, None]
    ctr, word = attn_counter(u, v, np.arange(H)[None, :], layer, step)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = np.stack(dropout_ref.philox4x32_10(ctr, (seed & dropout_ref.U32, seed >> 32)), axis=-1)     # [E, H, 4]
    pick = np.take_along_axis(w, np.broadcast_to(word, w.shape[:2])[..., None].astype(np.int64), axis=-1)[..., 0]
    return pick >= np.uint64(dropout_ref.threshold(p))


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def attn_keep(src_ids, dst_ids, indptr, indices, H, p, seed, layer, step):
    """bool [E, H] over the edges of the CSR in order: src_ids[i] / dst_ids[r] are the node ids of source row i /
    destination row r"""
    indptr, indices = _np(indptr).astype(np.int64), _np(indices).astype(np.int64)
    rows = np.repeat(np.arange(indptr.shape[0] - 1), np.diff(indptr))
    return attn_keep_edges(_np(src_ids)[indices], _np(dst_ids)[rows], H, p, seed, layer, step)


def partial_state_drop(el, er, z, indptr, indices, H, D, slope, keep, p, m=None):
    """gat_ref.partial_state with the numerator dropped: keep bool [E, H] (attn_keep), p the probability"""
    n_rows = indptr.numel() - 1
    rows, src = gat_ref.csr_rows(indptr), indices.long()
    score = torch.nn.functional.leaky_relu(el[src] + er[rows], slope)                       # [E, H]
    if m is None:
        m = torch.full((n_rows, H), -1e30, dtype=z.dtype, device=z.device).scatter_reduce(
            0, rows[:, None].expand(-1, H), score.detach(), "amax", include_self=True)
    m = m.detach().to(z.dtype)
    pe = torch.exp(score - m[rows])
    kappa = torch.as_tensor(_np(keep), device=z.device).to(z.dtype) * float(dropout_ref.scale(p))
    s = torch.zeros((n_rows, H), dtype=z.dtype, device=z.device).index_add(0, rows, pe)
    n = torch.zeros((n_rows, H, D), dtype=z.dtype, device=z.device).index_add(
        0, rows, (kappa * pe)[:, :, None] * z[src].view(-1, H, D))
    return m, s, n.reshape(n_rows, H * D)


def feat_drop(out, ids, p, seed, layer, step):
    """the feature mask on a layer's output rows (node ids `ids`), in out's dtype"""
    keep = dropout_ref.keep_mask(_np(ids), out.shape[1], p, seed, layer, step)
    return out * torch.as_tensor(keep, device=out.device).to(out.dtype) * float(dropout_ref.scale(p))


def layer_drop(x, weight, attn_l, attn_r, bias, indptr, indices, self_ids, slope, elu, src_ids, dst_ids, p_f, p_a, seed,
               layer, step):
    """gat_ref.layer with attention dropout p_a on its coefficients and feature dropout p_f on its output (after the
    activation).  Both 0: gat_ref.layer's own operations, nothing else."""
    H, D = attn_l.shape
    z = x @ weight.t()
    zv = z.view(-1, H, D)
    el, er = (zv * attn_l).sum(-1), gat_ref._self_rows((zv * attn_r).sum(-1), self_ids)
    if p_a > 0:
        keep = attn_keep(src_ids, dst_ids, indptr, indices, H, p_a, seed, layer, step)
        _, s, n = partial_state_drop(el, er, z, indptr, indices, H, D, slope, keep, p_a)
    else:
        _, s, n = gat_ref.partial_state(el, er, z, indptr, indices, H, D, slope)
    out = gat_ref.finish(n, s, bias, H, D, elu)
    return feat_drop(out, dst_ids, p_f, seed, layer, step) if p_f > 0 else out


def model_on_traversal(model, trav, feats, p_f, p_a, seed, step):
    """The unsplit model (a DistGATModel, any dtype / device) on the oracle's traversal with both dropouts: rows are node
    ids, so the masks' keys are the indices themselves.  Returns [num_nodes, n_classes]; rows of the seeds are meaningful.
    (test_gpu_gat._dense_gat_vectorised with the two masks.)"""
    L = len(trav["nbr_counts"])
    dev = feats.device
    h = feats
    for k, conv in enumerate(model.convs):
        lv = L - 1 - k
        fr = torch.as_tensor(np.asarray(trav["frontier"][lv]), device=dev).long()
        counts = torch.as_tensor(np.asarray(trav["nbr_counts"][lv]), device=dev).long()
        flat = torch.as_tensor(np.asarray(trav["nbr_flat"][lv]), device=dev).long()
        owner = torch.repeat_interleave(fr, counts)
        live = flat != owner                                        # drops the leading self entry and sampled self loops
        dst, src = owner[live], flat[live]
        z = h @ conv.fc.weight.t()
        zv = z.view(-1, conv.H, conv.D)
        el, er = (zv * conv.attn_l).sum(-1), (zv * conv.attn_r).sum(-1)
        score = torch.nn.functional.leaky_relu(el[src] + er[dst], conv.slope)            # [E, H]
        n_all = h.shape[0]
        m = torch.full((n_all, conv.H), -1e30, device=dev, dtype=h.dtype).scatter_reduce(
            0, dst[:, None].expand(-1, conv.H), score.detach(), "amax", include_self=True)
        pe = torch.exp(score - m[dst])
        ssum = torch.zeros((n_all, conv.H), device=dev, dtype=h.dtype).index_add(0, dst, pe)
        if p_a > 0:
            keep = attn_keep_edges(_np(src), _np(dst), conv.H, p_a, seed, k, step)
            pe = pe * torch.as_tensor(keep, device=dev).to(h.dtype) * float(dropout_ref.scale(p_a))
        num = torch.zeros((n_all, conv.H, conv.D), device=dev, dtype=h.dtype).index_add(0, dst, pe[:, :, None] * zv[src])
        out = (num / ssum.clamp_min(1e-300 if h.dtype == torch.float64 else 1e-30)[:, :, None]).reshape(n_all, -1) + conv.bias
        new = torch.zeros_like(out).index_copy(0, fr, out[fr])
        if k + 1 < len(model.convs):
            h = torch.nn.functional.elu(new)
            if p_f > 0:
                h = feat_drop(h, np.arange(n_all), p_f, seed, k, step)
        else:
            h = new.view(-1, model.heads, conv.D).mean(1)[:, :model.n_classes]
    return h
