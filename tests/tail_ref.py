"""The row-wise kernels that close a training step, restated in float64 with plain torch ops: the loss
(csl_softmax_ce_f32 / csl_softmax_ce_partial_f32), one Adam step (csl_adam_f32), the attention logits
(csl_gat_logits_fwd_f32 / _bwd_f32 / _bwd_acc_f32), the attention epilogue (csl_gat_finish_fwd_f32 / _bwd_f32) and the
bias + ELU pair (csl_bias_elu_f32 / csl_elu_bwd_colsum_f32) of include/cslicer_aggr.h.  No project kernel, no GPU.  The
backward formulas are written out by hand (that is what the kernels implement); tests/test_tail_ref_cpu.py checks them
against torch float64 autograd.  tests/sage_ref.softmax_ce and tests/gat_ref.finish are reused where they already say it.

Every function takes the float32 (or float64) arrays a kernel is given and evaluates the kernel's FORMULA on exactly those
values in float64.  The products and sums here are linear in each operand, so the sum of the |terms| of an entry (what
a rounding bound of an fp32 evaluation is made of) is the same function of the operands' absolute values.
"""
import numpy as np
import torch

import gat_ref
import sage_ref

F64 = torch.float64
S_FLOOR = float(np.float32(1e-30))     # the floor of a head's sum in the epilogue, as the float the kernels compare with


def _t(a, dtype=None):
    t = a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dtype) if dtype is not None else t


def _f32(x):
    """a Python float as the float32 the C ABI passes"""
    return float(np.float32(x))


# ---- the loss ---------------------------------------------------------------------------------------------------------

def softmax_ce(logits, ldl, n, n_pad, C, ids, rowmap, labels, scale, grad=None, ldgr=None):
    """csl_softmax_ce_partial_f32 on flat buffers: row r < n of the logits is logits[r * ldl : r * ldl + C], its label
    labels[rowmap[ids[r]]] (rowmap None: labels[ids[r]]); scale as the float32 that is passed.

        loss_rows[r] = scale * ((max - z[label]) + log sum exp(z - max))          [n]
        grad[r, :]   = scale * (softmax(z) - onehot(label)),  rows [n, n_pad) zero  [n_pad, C]
        colsum[c]    = sum_r grad[r, c]                                            [C]

    A label outside [0, C): that row's loss is NaN and its gradient row is NaN (so are the sums they enter).
    grad / ldgr: an optional flat float64 buffer the gradient rows are also written into, row r at r * ldgr, everything
    else left as it was (what the kernel may touch of a wider buffer).
    Returns (loss_rows, grad, colsum); the loss of the call is loss_rows.sum() (csl_softmax_ce_f32: with n_pad = n)."""
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
    _, g, _ = sage_ref.softmax_ce(z, safe, scale, n_pad)
    m = z.max(1).values if n else z.new_zeros(0)
    loss_rows = scale * ((m - z[rows, safe]) + torch.log(torch.exp(z - m[:, None]).sum(1)))
    loss_rows[bad] = float("nan")
    g[:n][bad] = float("nan")
    if grad is not None:
        cells = (torch.arange(n_pad)[:, None] * ldgr + torch.arange(C)[None, :]).reshape(-1)
        grad.reshape(-1)[cells] = g.reshape(-1)
    return loss_rows, g, g.sum(0)


# ---- Adam -------------------------------------------------------------------------------------------------------------

def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    """One step of csl_adam_f32 on one tensor: the kernel's formula

        m' = b1 m + (1 - b1) g;   v' = b2 v + (1 - b2) g^2;
        p' = p - (lr / (1 - b1^t)) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

    in float64 ON THE ABI'S OWN float32 ARGUMENTS: lr, beta1, beta2 and eps are rounded to float32 first, as the call
    passes them, and every later operation (1 - b, the powers, the bias corrections, which the entry point itself
    computes in double) is float64.  This matters: 0.999 as a float32 is 0.99900001287..., and half a float32 step of
    a beta2 near it puts 1 - beta2 up to 6e-5 (relatively) off the double value (1.3e-5 for 0.999 itself), so a float64
    trajectory with DOUBLE betas is a different function, not a more accurate one.
    Returns (p', m', v', update, m_abs, v_abs): update = p - p', m_abs / v_abs the sums of the |terms| of the moments
    (what a rounding bound of their fp32 evaluation is made of)."""
    p, g, m, v = (_t(a, F64) for a in (p, g, m, v))
    lr, b1, b2, eps = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    upd = adam_update(m1, v1, lr, b1, b2, eps, step)
    return p - upd, m1, v1, upd, (b1 * m).abs() + ((1.0 - b1) * g).abs(), b2 * v + (1.0 - b2) * g * g


def adam_update(m1, v1, lr, beta1, beta2, eps, step):
    """the parameter's decrement from given new moments (float32 ABI arguments, as adam_step)"""
    lr, b1, b2, eps = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return (lr / bc1) * _t(m1, F64) / (torch.sqrt(_t(v1, F64)) / np.sqrt(bc2) + eps)


# ---- attention logits -------------------------------------------------------------------------------------------------

def logits_fwd(z, attn_l, attn_r, H, D):
    """el[r, h] = <z[r, h, :], attn_l[h, :]>, er likewise: ([n, H], [n, H])"""
    zv = _t(z, F64).reshape(-1, H, D)
    return (zv * _t(attn_l, F64).reshape(H, D)).sum(-1), (zv * _t(attn_r, F64).reshape(H, D)).sum(-1)


def logits_bwd(z, attn_l, attn_r, g_el, g_er, H, D, g_z_before=None):
    """g_z[r, h, :] = g_el[r, h] a_l[h, :] + g_er[r, h] a_r[h, :] (+ g_z_before: csl_gat_logits_bwd_acc_f32 with
    accumulate), g_attn_l[h, :] = sum_r g_el[r, h] z[r, h, :], g_attn_r likewise: ([n, H*D], [H, D], [H, D])"""
    zv = _t(z, F64).reshape(-1, H, D)
    al, ar = _t(attn_l, F64).reshape(H, D), _t(attn_r, F64).reshape(H, D)
    ge, gr = _t(g_el, F64).reshape(-1, H, 1), _t(g_er, F64).reshape(-1, H, 1)
    g_z = (ge * al + gr * ar).reshape(-1, H * D)
    if g_z_before is not None:
        g_z = g_z + _t(g_z_before, F64).reshape(-1, H * D)
    return g_z, (ge * zv).sum(0), (gr * zv).sum(0)


# ---- attention epilogue -----------------------------------------------------------------------------------------------

def elu(x):
    return torch.where(x > 0, x, torch.expm1(x))


def elu_slope_from_output(out):
    """ELU' read off the activation's OUTPUT, as the kernels do: out > 0 ? 1 : out + 1 (exactly 1 at out == 0, exactly
    0 at out == -1, where a very negative input ends up)"""
    out = _t(out, F64)
    return torch.where(out > 0, torch.ones_like(out), out + 1.0)


def finish_fwd(n, s, bias, H, D, use_elu):
    """out[r, h, :] = act(n[r, h, :] / max(s[r, h], 1e-30f) + bias[h, :]): gat_ref.finish with the kernel's floor (a
    head sum of 0, or below the floor, divides by the floor)"""
    s = _t(s, F64).reshape(-1, H).clamp_min(S_FLOOR)
    return gat_ref.finish(_t(n, F64).reshape(-1, H * D), s, _t(bias, F64).reshape(-1), H, D, bool(use_elu))


def finish_bwd(g, out, n, s, H, D, use_elu):
    """p = g .* act'(out);  g_n = p / s;  g_s[r, h] = -sum_d g_n n / s;  g_bias = column sums of p (s floored as in
    finish_fwd; g: the [rows, H*D] gradient of out, already cut out of any wider buffer).
    Returns (g_n [rows, H*D], g_s [rows, H], g_bias [H*D], p)"""
    p = _t(g, F64).reshape(-1, H * D)
    if use_elu:
        p = p * elu_slope_from_output(out).reshape(-1, H * D)
    sv = _t(s, F64).reshape(-1, H, 1).clamp_min(S_FLOOR)
    g_n = p.reshape(-1, H, D) / sv
    g_s = -(g_n * _t(n, F64).reshape(-1, H, D)).sum(-1) / sv[:, :, 0]
    return g_n.reshape(-1, H * D), g_s, p.sum(0), p


# ---- bias + ELU -------------------------------------------------------------------------------------------------------

def bias_elu(y, bias, use_elu):
    """act(y + bias) row by row (y: [n, C], already cut out of any wider buffer)"""
    x = _t(y, F64) + _t(bias, F64)
    return elu(x) if use_elu else x


def elu_bwd_colsum(g, y, use_elu):
    """out = g .* act'(y) from the activation's output y, and the column sums of out: ([n, C], [C])"""
    out = _t(g, F64)
    if use_elu:
        out = out * elu_slope_from_output(y)
    return out, out.sum(0)
