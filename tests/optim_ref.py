"""One step of csl_adamw_f32 (include/cslicer_optim.h) restated in float64 with plain torch ops: the gradient's global norm,
the clip coefficient, the non-finite guard and the update of one tensor.  No project kernel, no GPU.
tests/test_optim_cpu.py checks it against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW / Adam in float64.

As tail_ref.adam_step, everything is evaluated in float64 ON THE ABI'S OWN float32 ARGUMENTS (lr, betas, eps, the decays
and max_norm are rounded to float32 first), and with abi_rounding=True (default) the two numbers the entry point rounds
once more are rounded here too: the clip coefficient c (float64 -> float32 on the device) and the decoupled factor
1 - lr wd (float64 -> float32 on the host).  abi_rounding=False keeps both in float64: the formula torch evaluates.
"""
import collections

import numpy as np
import torch

import tail_ref as T

F64 = torch.float64
Step = collections.namedtuple("Step", "p m v p_in g2 g2_abs g2_roundings upd m_abs v_abs")


def grad_norm(grads):
    """sqrt(sum g^2) over every tensor, float64 (a Python float; nan / inf where a gradient is)"""
    total = 0.0
    for g in grads:
        total += float((T._t(g, F64) ** 2).sum())
    return float(np.sqrt(total))


def clip_coef(n, max_norm, abi_rounding=True):
    """c = min(1, max_norm / (n + 1e-6)) (torch.nn.utils.clip_grad_norm_); max_norm None or <= 0: no clipping, 1"""
    if max_norm is None or not max_norm > 0:
        return 1.0
    c = min(1.0, T._f32(max_norm) / (n + 1e-6))
    return T._f32(c) if abi_rounding else c


def skipped(n, max_norm):
    """the guard: with clipping on, a norm that is not finite skips the step"""
    return max_norm is not None and max_norm > 0 and not np.isfinite(n)


def decay_factor(lr, weight_decay, abi_rounding=True):
    d = 1.0 - T._f32(lr) * T._f32(weight_decay)
    return T._f32(d) if abi_rounding else d


def adamw_step(p, g, m, v, c, weight_decay, decoupled, lr, beta1, beta2, eps, step, abi_rounding=True):
    """One step on one tensor, c from clip_coef (1.0: no clipping):

        g1 = g c;   wd > 0, coupled:    g2 = g1 + wd p,  p_in = p
                    wd > 0, decoupled:  g2 = g1,         p_in = p (1 - lr wd)
                    wd == 0:            g2 = g1,         p_in = p
        (p', m', v') = tail_ref.adam_step(p_in, g2, m, v)

    Returns Step: p, m, v (the new ones), p_in, g2, g2_abs = |g c| + |wd p| (the sum of the |terms| of g2),
    g2_roundings (the fp32 roundings g2 goes through: 1 for g c when c != 1, 2 more for the coupled product and sum),
    upd = p_in - p', and the moments' sums of |terms| WITH g2_abs in the place of |g2|:
    m_abs = |b1 m| + (1 - b1) g2_abs, v_abs = b2 v + (1 - b2) g2_abs^2."""
    p, g, m, v = (T._t(a, F64) for a in (p, g, m, v))
    wd = T._f32(weight_decay)
    b1, b2 = T._f32(beta1), T._f32(beta2)
    g2 = g * c
    g2_abs = g2.abs()
    k = 0 if c == 1.0 else 1
    p_in = p
    if wd > 0 and decoupled:
        p_in = p * decay_factor(lr, wd, abi_rounding)
    elif wd > 0:
        g2 = g2 + wd * p
        g2_abs = g2_abs + (wd * p).abs()
        k += 2
    p1, m1, v1, upd, _, _ = T.adam_step(p_in, g2, m, v, lr, beta1, beta2, eps, step)
    return Step(p1, m1, v1, p_in, g2, g2_abs, k, upd, (b1 * m).abs() + (1.0 - b1) * g2_abs,
                b2 * v + (1.0 - b2) * g2_abs * g2_abs)
