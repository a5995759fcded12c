"""Full-neighbour inference restated in float64 with torch index ops over an arbitrary CSR: what cslicer.infer and
csrc/infer.hip are pinned against.  Neighbours of v: the entries u != v of CSR row v, with multiplicity.

    SAGE layer  y[v] = act([h[v] | mean_u h[u]] . W^T + b)      (mean over no neighbours: a zero row)
    GAT layer   gat_ref.partial_state over the neighbour CSR, er[v] from v's own row, then gat_ref.finish
"""
import numpy as np
import torch

import gat_ref


def neighbour_csr(indptr, indices):
    """(indptr, indices) int64 torch tensors of the CSR with self loops removed"""
    indptr = torch.as_tensor(np.asarray(indptr, dtype=np.int64))
    indices = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    rows = gat_ref.csr_rows(indptr)
    keep = indices != rows
    cnt = torch.bincount(rows[keep], minlength=indptr.numel() - 1)
    ip = torch.zeros(indptr.numel(), dtype=torch.int64)
    ip[1:] = torch.cumsum(cnt, 0)
    return ip, indices[keep]


def sage_layer(h, weight, bias, indptr, indices, relu, rows=None):
    """one DistSageConv over the neighbour CSR (indptr, indices), for `rows` (None: all)"""
    h = h.double()
    n = indptr.numel() - 1
    r = gat_ref.csr_rows(indptr)
    s = torch.zeros((n, h.shape[1]), dtype=torch.float64).index_add(0, r, h[indices])
    deg = (indptr[1:] - indptr[:-1]).clamp_min(1).double()
    cat = torch.cat([h, s / deg[:, None]], 1)
    if rows is not None:
        cat = cat[torch.as_tensor(rows)]
    y = cat @ weight.double().t() + bias.double()
    return torch.relu(y) if relu else y


def gat_layer(h, conv, indptr, indices, last, n_cls=None, rows=None):
    """one DistGATConv over the neighbour CSR, hidden (ELU, heads concatenated) or last (head mean, class slice)"""
    H, D = conv.H, conv.D
    z = h.double() @ conv.fc.weight.double().t()
    zv = z.view(-1, H, D)
    el = (zv * conv.attn_l.double()).sum(-1)
    er = (zv * conv.attn_r.double()).sum(-1)
    _, s, nn_ = gat_ref.partial_state(el, er, z, indptr, indices, H, D, conv.slope)
    out = gat_ref.finish(nn_, s, conv.bias.double(), H, D, elu=not last)
    if rows is not None:
        out = out[torch.as_tensor(rows)]
    if last:
        out = out.view(-1, H, D).mean(1)[:, :n_cls]
    return out


def model(m, features, indptr, indices, nodes=None):
    """float64 logits of a DistSAGEModel / DistGATModel (CPU copies of the parameters are used)"""
    ip, ix = neighbour_csr(indptr, indices)
    h = torch.as_tensor(features).double().cpu()
    L = len(m.convs)
    for k, conv in enumerate(m.convs):
        last = k + 1 == L
        rows = nodes if last else None
        if hasattr(conv, "fc") and not hasattr(conv, "H"):
            h = sage_layer(h, conv.fc.weight.detach().cpu(), conv.fc.bias.detach().cpu(), ip, ix, not last, rows)
        else:
            c = _cpu_conv(conv)
            h = gat_layer(h, c, ip, ix, last, getattr(m, "n_classes", None), rows)
    return h


class _cpu_conv(object):
    def __init__(self, conv):
        self.H, self.D, self.slope = conv.H, conv.D, conv.slope
        self.fc = type("fc", (), {"weight": conv.fc.weight.detach().cpu()})
        self.attn_l, self.attn_r, self.bias = (conv.attn_l.detach().cpu(), conv.attn_r.detach().cpu(),
                                               conv.bias.detach().cpu())
