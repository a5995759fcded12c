"""Dropout for the attention model on the GPU (include/cslicer_gat_dropout.h, csrc/aggregate.hip):

* the attention mask of csl_gat_drop_fwd_f32 against tests/gat_drop_ref.py, bit for bit (z = 1, el = er = 0: the numerator
  counts the kept edges);
* the four dropped twins against float64 at every dispatch edge of their parents: rows of 0, 1, 16 and 17 edges, head
  groups of 1, 5, 8 and 16 lanes (one chunk of columns and two), 1, 4 and 5 rows, the by-source forms with padding rows
  and self entries, the fused by-source form against the unfused one;
* the dropped epilogue pair = its parent and csl_dropout_f32, bit for bit, forward and backward;
* every dropped entry point at p = 2^-33 (no edge dropped, a scale of 1.0f) = its parent, bit for bit: the two are one
  kernel template and one host path;
* spec None / both probabilities 0: today's nodes and model, no new call;
* DistGATModel.forward_parts with both dropouts on one part and on two, against the float64 model with the same masks;
* trainers: determinism, the seed, 0 / 0, evaluation, the plan;
* the rank form over gloo (node by node), the ranks' sum against the single-process float64 model.

Tolerances: per-layer outputs within 1e-5 of the row's largest entry, gradients within 1e-4 of the tensor's
largest entry; a whole model: loss 1e-5 relative, every parameter gradient within 1e-4 of its largest entry; the mask and
everything said to be "the same run" bit for bit.  (The entry points' refusals run without a GPU: test_gat_drop_cpu.py.)
"""
import copy
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

import gat_drop_ref
import gat_ref

pytestmark = pytest.mark.gpu


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32, device="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _rows_close(got, want, tol, what):
    """|got - want| <= tol * (the row's largest |want|) row by row (rows of zeros: exact)"""
    assert got.shape == want.shape, what
    g64 = got.double()
    assert bool(torch.isfinite(g64).all()), what + ": not finite"
    err, scale = (g64 - want).abs().amax(1), want.abs().amax(1)
    print("%s: largest row error %.3g (row scale %.3g)" % (what, float(err.detach().max()), float(scale.detach().max())))
    bad = err > tol * scale
    assert not bool(bad.any()), "%s: rows %s, error %s, row scale %s" % (
        what, torch.nonzero(bad)[:5, 0].tolist(), err[bad][:5].tolist(), scale[bad][:5].tolist())


def _grad_close(got, want, tol, what, scale=None):
    """max |got - want| <= tol * max |want| over the tensor (or tol * scale)"""
    g64 = got.double()
    assert bool(torch.isfinite(g64).all()), what + ": not finite"
    err, scale = float((g64 - want).abs().max()), float(want.abs().max()) if scale is None else scale
    print("%s: max error %.3g, tensor scale %.3g" % (what, err, scale))
    assert err <= tol * scale, "%s: max error %g, tensor scale %g" % (what, err, scale)


def _ids(n, rng, top):
    """distinct non-negative int32 node ids in no order, the largest one `top`"""
    ids = rng.permutation(1 << 20)[:n].astype(np.int64) * 2047 + 5
    ids[rng.integers(0, n)] = top
    return ids


# ---- the mask, bit for bit --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 3, 8])
def test_attention_mask_is_the_reference_bit_for_bit(H):
    """z = 1, el = er = 0, D = 4: every p_e is 1, so s is the degree and n[r, h, :] / s_a the number of kept edges of
    (r, h).  p = 0.5 and 0.75: s_a = 2 and 4, the products exact.  Rows of 0, 1, 2, 3, 16 and 17 edges (both branches of the
    forward), ids up to 2^31 - 1, a seed with a high word, a step >= 2^32, layers 0 and 2."""
    from cslicer import aggr
    L = aggr._lib()
    rng = np.random.default_rng(100 + H)
    n_rows, n_src, D = 203, 150, 4
    deg = np.resize(np.array([0, 1, 2, 3, 1, 2, 16, 17]), n_rows)
    indptr_np = np.concatenate([[0], np.cumsum(deg)])
    indices_np = rng.integers(0, n_src, size=int(deg.sum()))
    src_np, dst_np = _ids(n_src, rng, (1 << 31) - 1), _ids(n_rows, rng, (1 << 31) - 2)
    indptr, indices, src_ids, dst_ids = _i32(indptr_np), _i32(indices_np), _i32(src_np), _i32(dst_np)
    z = torch.ones(n_src, H * D, device="cuda")
    el, er = torch.zeros(n_src, H, device="cuda"), torch.zeros(n_rows, H, device="cuda")
    rows = np.repeat(np.arange(n_rows), deg)
    masks = {}
    for p, seed, layer, step in ((0.5, (0x9abcdef1 << 32) | 77, 0, 7), (0.5, (0x9abcdef1 << 32) | 77, 2, 7),
                                 (0.75, 12345, 2, (1 << 32) + 5), (0.5, (0x9abcdef1 << 32) | 77, 0, 8), (0.5, 78, 0, 7)):
        keep = gat_drop_ref.attn_keep(src_np, dst_np, indptr_np, indices_np, H, p, seed, layer, step)        # [E, H]
        count = np.zeros((n_rows, H), dtype=np.int64)
        np.add.at(count, rows, keep.astype(np.int64))
        # the reference itself: at least one (row, head) with every edge dropped, one with >= 2 edges all kept
        assert ((count == 0) & (deg[:, None] >= 1)).any() and ((count == deg[:, None]) & (deg[:, None] >= 2)).any()
        assert 0 < keep.sum() < keep.size
        m = torch.full((n_rows, H), 5.0, device="cuda")
        s = torch.full((n_rows, H), -1.0, device="cuda")
        n = torch.full((n_rows, H * D), -1.0, device="cuda")
        rc = L.csl_gat_drop_fwd_f32(_p(indptr), _p(indices), n_rows, _p(el), _p(er), _p(z), H, D, 0.2, _p(m), _p(s), _p(n),
                                    _p(src_ids), _p(dst_ids), p, aggr._i64(seed), layer, aggr._i64(step), aggr._stream())
        assert rc == 0
        torch.cuda.synchronize()
        s_a = 1.0 / (1.0 - p)
        assert np.array_equal(s.cpu().numpy(), np.broadcast_to(deg[:, None], (n_rows, H)).astype(np.float32))
        got = n.cpu().numpy().reshape(n_rows, H, D)
        assert np.array_equal(got, np.broadcast_to((count * s_a).astype(np.float32)[:, :, None], got.shape)), (p, seed, layer, step)
        assert np.array_equal(m.cpu().numpy()[deg > 0], np.zeros((int((deg > 0).sum()), H), dtype=np.float32))
        masks[(p, seed, layer, step)] = keep
    a = masks[(0.5, (0x9abcdef1 << 32) | 77, 0, 7)]
    for other in ((0.5, (0x9abcdef1 << 32) | 77, 2, 7), (0.5, (0x9abcdef1 << 32) | 77, 0, 8), (0.5, 78, 0, 7)):
        assert not np.array_equal(a, masks[other])       # another layer, step, seed: another mask


# ---- values at every dispatch edge ------------------------------------------------------------------------------------------

DEGREES = (17, 16, 1, 0, 16)      # 1 row: the general loop; 4 rows: every branch in one workgroup; 5: a second workgroup
SHAPES = [(1, 4), (3, 20), (8, 32), (8, 64)]      # head groups of 1, 5 and 8 lanes in one chunk of columns; 16 lanes, two chunks
N_SRC, P_A, SEED, LAYER, STEP = 21, 0.5, (7 << 32) | 99, 2, (1 << 32) + 3


def _case(H, D, n_rows, seed):
    rng = np.random.default_rng(seed)
    deg = np.resize(np.array(DEGREES), n_rows)
    indptr_np = np.concatenate([[0], np.cumsum(deg)])
    indices_np = rng.integers(0, N_SRC, size=int(deg.sum()))
    src_np, dst_np = _ids(N_SRC, rng, (1 << 31) - 1), _ids(n_rows, rng, (1 << 31) - 2)
    self_np = rng.permutation(N_SRC)[:n_rows]           # (a source is the self row of one destination at most)
    if n_rows > 1:
        self_np[1] = -1
    return indptr_np, indices_np, src_np, dst_np, self_np


@pytest.mark.parametrize("n_rows", [1, 4, 5])
@pytest.mark.parametrize("H,D", SHAPES)
def test_dropped_aggregation_against_float64(H, D, n_rows):
    """csl_gat_drop_fwd_f32 / csl_gat_drop_bwd_f32 (aggr.GatAggregate with attention dropout): (m, s, n) and the gradients
    of el, er, z; s and n at the kernel's own stabiliser m"""
    from cslicer import aggr
    indptr_np, indices_np, src_np, dst_np, _ = _case(H, D, n_rows, H * D + n_rows)
    indptr, indices = _i32(indptr_np), _i32(indices_np)
    attn = (_i32(src_np), _i32(dst_np), P_A, SEED, LAYER, STEP)
    keep = gat_drop_ref.attn_keep(src_np, dst_np, indptr_np, indices_np, H, P_A, SEED, LAYER, STEP)
    torch.manual_seed(H + D)
    el0, er0 = torch.randn(N_SRC, H, device="cuda"), torch.randn(n_rows, H, device="cuda")
    z0 = torch.randn(N_SRC, H * D, device="cuda")
    gs, gn = torch.randn(n_rows, H, device="cuda"), torch.randn(n_rows, H * D, device="cuda")
    el, er, z = (t.clone().requires_grad_() for t in (el0, er0, z0))
    m, s, n = aggr.GatAggregate.apply(el, er, z, indptr, indices, n_rows, H, D, 0.2, attn)
    ((s * gs).sum() + (n * gn).sum()).backward()
    torch.cuda.synchronize()
    l64 = [t.double().requires_grad_() for t in (el0, er0, z0)]
    m_ref, _, _ = gat_ref.partial_state(*l64, indptr, indices, H, D, 0.2)
    _, s_ref, n_ref = gat_drop_ref.partial_state_drop(*l64, indptr, indices, H, D, 0.2, keep, P_A, m=m.double())
    ((s_ref * gs.double()).sum() + (n_ref * gn.double()).sum()).backward()
    torch.testing.assert_close(m.double(), m_ref, rtol=1e-6, atol=0)
    _rows_close(s, s_ref.detach(), 1e-5, "s")
    _rows_close(n, n_ref.detach(), 1e-5, "n")
    for name, g, t in zip(("el", "er", "z"), (el.grad, er.grad, z.grad), l64):
        _grad_close(g, t.grad, 1e-4, "grad " + name)
    # it IS dropout: the undropped numerator is another one, the denominator the same
    _, s_plain, n_plain = aggr.GatAggregate.apply(el0, er0, z0, indptr, indices, n_rows, H, D, 0.2)
    assert torch.equal(s_plain, s) and not torch.equal(n_plain, n)


def _by_source(indptr_np, indices_np, self_np, n_src):
    """the slice by source as the engine emits it: per source u the destination rows of its edges (ascending), and a -1
    entry for a destination whose self row u is (attention skips it)"""
    rows = np.repeat(np.arange(indptr_np.size - 1), np.diff(indptr_np))
    own = np.flatnonzero(self_np >= 0)
    key_src = np.concatenate([indices_np, self_np[own]])
    key_dst = np.concatenate([rows, np.full(own.size, -1)])
    order = np.lexsort((key_dst, key_src))
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(key_src, minlength=n_src), out=t_indptr[1:])
    return _i32(t_indptr), _i32(key_dst[order]), int(np.diff(t_indptr).max())


def _er_blind(x, weight, al, ar, indptr, indices, self_ids):
    """whether leaky' is constant over every (row, head) of the float64 layer: a row's softmax then does not see er (a
    constant of the row), attn_r's exact gradient is 0 and what a float32 kernel returns is the rounding of its cancelling
    per-edge terms, which have the size of attn_l's (test_gpu_gat_edges._attn_grads_close: measured against that scale)"""
    H, D = al.shape
    zv = (x @ weight.t()).view(-1, H, D)
    el, er = (zv * al).sum(-1), gat_ref._self_rows((zv * ar).sum(-1), self_ids)
    rows = gat_ref.csr_rows(indptr)
    pos = ((el[indices.long()] + er[rows]) > 0).double()
    n_rows = indptr.numel() - 1
    cnt = torch.zeros((n_rows, H), dtype=torch.float64, device=x.device).index_add(0, rows, pos)
    deg = (indptr[1:] - indptr[:-1]).double()[:, None]
    return bool(((cnt == 0) | (cnt == deg)).all())


@pytest.mark.parametrize("n_rows", [1, 4, 5])
@pytest.mark.parametrize("H,D", SHAPES)
def test_dropped_layer_in_its_three_backward_forms_against_float64(H, D, n_rows, monkeypatch):
    """aggr.GatLayerLocal with attention dropout: the forward twin, then the backward by source with the logits folded in
    (csl_gat_drop_bwd_t_fused_f32), by source (csl_gat_drop_bwd_t_f32 + csl_gat_logits_bwd_acc_f32) and by destination
    with atomics (csl_gat_drop_bwd_f32), each against float64 and the fused form against the unfused one.  21 source rows
    under a row padding of 8: the GEMM operand has 24 rows (n_pad > n_src); the lists by source carry the self entries."""
    from cslicer import aggr
    indptr_np, indices_np, src_np, dst_np, self_np = _case(H, D, n_rows, 7 * H + D + n_rows)
    indptr, indices, self_ids = _i32(indptr_np), _i32(indices_np), _i32(self_np)
    tptr, trow, t_max = _by_source(indptr_np, indices_np, self_np, N_SRC)
    assert bool((trow < 0).any()) and t_max <= 64
    attn = (_i32(src_np), _i32(dst_np), P_A, SEED, LAYER, STEP)
    F_in = 12
    torch.manual_seed(n_rows + H)
    x0 = torch.randn(N_SRC, F_in, device="cuda")
    weight0 = torch.randn(H * D, F_in, device="cuda") / F_in ** 0.5
    al0, ar0 = torch.randn(H, D, device="cuda") / D ** 0.5, torch.randn(H, D, device="cuda") / D ** 0.5
    bias0 = 0.1 * torch.randn(H * D, device="cuda")
    w = torch.randn(n_rows, H * D, device="cuda")
    calls = []
    real = aggr._gat_call
    monkeypatch.setattr(aggr, "_gat_call", lambda stem, a, *args: (calls.append((stem, a is not None)), real(stem, a, *args))[1])
    for elu in (True, False):
        l64 = [t.double().requires_grad_() for t in (x0, weight0, al0, ar0, bias0)]
        ref = gat_drop_ref.layer_drop(*l64, indptr, indices, self_ids, 0.2, elu, src_np, dst_np, 0.0, P_A, SEED, LAYER, STEP)
        (ref * w.double()).sum().backward()
        with torch.no_grad():
            blind = _er_blind(*l64[:4], indptr, indices, self_ids)
        r_scale = lambda name: float(l64[2].grad.abs().max()) if name == "attn_r" and blind else None      # noqa: E731
        got = {}
        for mode in ("fused", "nofold", "atomic"):
            if mode == "nofold":
                monkeypatch.setenv("CSLICER_GAT_NO_FOLD", "1")
            else:
                monkeypatch.delenv("CSLICER_GAT_NO_FOLD", raising=False)
            by_source = mode != "atomic"
            leaves = [t.clone().requires_grad_() for t in (x0, weight0, al0, ar0, bias0)]
            del calls[:]
            out = aggr.GatLayerLocal.apply(*leaves, indptr, indices, self_ids, n_rows, 0.2, elu, 8,
                                           lambda gz, xp: gz.t() @ xp, tptr if by_source else None,
                                           trow if by_source else None, t_max, None, False, attn)
            (out * w).sum().backward()
            torch.cuda.synchronize()
            assert calls == [("fwd", True), ({"fused": "bwd_t_fused", "nofold": "bwd_t", "atomic": "bwd"}[mode], True)]
            what = "%s, elu %s" % (mode, elu)
            _rows_close(out.detach(), ref.detach(), 1e-5, "out, " + what)
            for name, g, t in zip(("x", "weight", "attn_l", "attn_r", "bias"), [t.grad for t in leaves], l64):
                _grad_close(g, t.grad, 1e-4, "grad %s, %s" % (name, what), r_scale(name))
            got[mode] = [t.grad for t in leaves]
        for name, a, b, t in zip(("x", "weight", "attn_l", "attn_r", "bias"), got["fused"], got["nofold"], l64):
            _grad_close(a, b.double(), 1e-4, "grad %s, fused against unfused, elu %s" % (name, elu),
                        r_scale(name) or float(t.grad.abs().max()))


@pytest.mark.parametrize("H,D,n", [(1, 4, 1), (3, 20, 5), (8, 32, 130), (8, 64, 67)])
def test_dropped_epilogue_is_the_parent_and_the_dropout_kernel_bit_for_bit(H, D, n):
    """csl_gat_finish_drop_fwd_f32 = csl_gat_finish_fwd_f32 then csl_dropout_f32 (both outputs; y the first rows of a larger
    buffer whose other rows stay as they were), csl_gat_finish_drop_bwd_f32 = csl_dropout_f32 on the gradient (strided
    rows) then csl_gat_finish_bwd_f32: g_n, g_s and the bias gradient, with and without the ELU, a row with s = 0 among them"""
    from cslicer import aggr
    L = aggr._lib()
    Cw = H * D
    rng = np.random.default_rng(H * D + n)
    ids = _i32(_ids(n, rng, (1 << 31) - 1))
    torch.manual_seed(n)
    nsum, ssum = torch.randn(n, Cw, device="cuda"), torch.rand(n, H, device="cuda") + 0.1
    ssum[0], nsum[0] = 0.0, 0.0                  # a row without edges
    bias = torch.randn(Cw, device="cuda")
    g = torch.randn(n, Cw + 4, device="cuda")[:, :Cw]
    p_f, seed, layer, step = 0.6, (3 << 32) | 17, 1, (1 << 32) + 2
    tail = (_p(ids), p_f, aggr._i64(seed), layer, aggr._i64(step), aggr._stream())
    for elu in (1, 0):
        out_p = torch.empty(n, Cw, device="cuda")
        assert L.csl_gat_finish_fwd_f32(_p(nsum), _p(ssum), _p(bias), n, H, D, elu, _p(out_p), aggr._stream()) == 0
        y_p = aggr.dropout(out_p, ids, p_f, seed, layer, step)
        out_d, ybuf = torch.empty(n, Cw, device="cuda"), torch.full((n + 3, Cw), -77.25, device="cuda")
        assert L.csl_gat_finish_drop_fwd_f32(_p(nsum), _p(ssum), _p(bias), n, H, D, elu, _p(out_d), _p(ybuf), *tail) == 0
        torch.cuda.synchronize()
        assert torch.equal(out_d, out_p) and torch.equal(ybuf[:n], y_p) and bool((ybuf[n:] == -77.25).all())
        assert bool((y_p == 0).any()) and bool((y_p != 0).any())
        words = max(int(L.csl_gat_finish_bwd_scratch(n, H, D)), 4)
        res = []
        for dropped in (False, True):
            g_n, g_s = torch.empty(n, Cw, device="cuda"), torch.empty(n, H, device="cuda")
            g_bias, scratch = torch.empty(Cw, device="cuda"), torch.empty(words, device="cuda")
            if dropped:
                rc = L.csl_gat_finish_drop_bwd_f32(_p(g), g.stride(0), _p(out_p), _p(nsum), _p(ssum), n, H, D, elu, _p(g_n),
                                                   _p(g_s), _p(g_bias), _p(scratch), *tail)
            else:
                gd = aggr.dropout(g, ids, p_f, seed, layer, step)
                rc = L.csl_gat_finish_bwd_f32(_p(gd), gd.stride(0), _p(out_p), _p(nsum), _p(ssum), n, H, D, elu, _p(g_n),
                                              _p(g_s), _p(g_bias), _p(scratch), aggr._stream())
            assert rc == 0
            torch.cuda.synchronize()
            res.append((g_n, g_s, g_bias))
        for a, b in zip(*res):
            assert torch.equal(a, b)


# ---- the dropped instantiation is its parent ---------------------------------------------------------------------------------
# p = 2^-33: floor(p 2^32) = 0, so no word is below the threshold and every edge / element is kept, and
# (float)(1 / (1 - p)) == 1.0f, so kappa = 1.0f and the mask multiplies by 1.0f.  The dropped entry point then computes what
# its parent computes, operation for operation, and must return the same bits.  Wherever float atomics add (g_z and g_el
# by destination, g_er by source) no address takes more than two addends onto its zero: either order gives the same sum.

P_KEEP = 2.0 ** -33
ONE_SHAPES = [(1, 4), (3, 20), (8, 64)]     # a head per lane; head groups of 5 lanes; 16 lanes and two chunks of columns


def test_p_keep_keeps_everything_at_scale_one():
    import dropout_ref
    assert np.float32(P_KEEP) == P_KEEP and int(np.floor(np.float64(np.float32(P_KEEP)) * 2.0 ** 32)) == 0
    assert np.float32(1.0 / (1.0 - np.float64(np.float32(P_KEEP)))) == np.float32(1.0)
    assert dropout_ref.threshold(P_KEEP) == 0 and np.float32(dropout_ref.scale(P_KEEP)) == np.float32(1.0)


def _keep_tail(aggr, *ids):
    return tuple(_p(i) for i in ids) + (P_KEEP, aggr._i64((9 << 32) | 5), 1, aggr._i64((1 << 32) + 2), aggr._stream())


@pytest.mark.parametrize("H,D", ONE_SHAPES)
def test_dropped_aggregation_that_keeps_every_edge_is_the_parent_bit_for_bit(H, D):
    """csl_gat_drop_fwd_f32 = csl_gat_fwd_f32 (m, s, n) and csl_gat_drop_bwd_f32 = csl_gat_bwd_f32 (g_el, g_er, g_z): 5 rows
    of 17, 16, 1, 0 and 16 edges (the 16-edge branch, the chunked loop, a second workgroup), node ids up to 2^31 - 1, every
    source in at most two of the 50 edges"""
    from cslicer import aggr
    L = aggr._lib()
    rng = np.random.default_rng(H * D)
    n_rows, n_src, Cw = 5, 27, H * D
    deg = np.array(DEGREES)
    indptr_np = np.concatenate([[0], np.cumsum(deg)])
    indices_np = rng.permutation(np.arange(int(deg.sum())) // 2)
    assert np.bincount(indices_np).max() == 2 and indices_np.max() < n_src
    indptr, indices = _i32(indptr_np), _i32(indices_np)
    src_ids, dst_ids = _i32(_ids(n_src, rng, (1 << 31) - 1)), _i32(_ids(n_rows, rng, (1 << 31) - 2))
    tail = _keep_tail(aggr, src_ids, dst_ids)
    torch.manual_seed(H + D)
    el, er, z = torch.randn(n_src, H, device="cuda"), torch.randn(n_rows, H, device="cuda"), torch.randn(n_src, Cw, device="cuda")
    gs, gn = torch.randn(n_rows, H, device="cuda"), torch.randn(n_rows, Cw, device="cuda")
    head = (_p(indptr), _p(indices), n_rows, _p(el), _p(er), _p(z), H, D, 0.2)
    fwd, bwd = [], []
    for dropped in (False, True):
        m, s_, n = (torch.full(shape, -7.5, device="cuda") for shape in ((n_rows, H), (n_rows, H), (n_rows, Cw)))
        if dropped:
            rc = L.csl_gat_drop_fwd_f32(*head, _p(m), _p(s_), _p(n), *tail)
        else:
            rc = L.csl_gat_fwd_f32(*head, _p(m), _p(s_), _p(n), aggr._stream())
        assert rc == 0
        g_el, g_z = torch.zeros(n_src, H, device="cuda"), torch.zeros(n_src, Cw, device="cuda")
        g_er = torch.full((n_rows, H), -7.5, device="cuda")
        if dropped:
            rc = L.csl_gat_drop_bwd_f32(*head, _p(m), _p(gs), _p(gn), _p(g_el), _p(g_er), _p(g_z), *tail)
        else:
            rc = L.csl_gat_bwd_f32(*head, _p(m), _p(gs), _p(gn), _p(g_el), _p(g_er), _p(g_z), aggr._stream())
        assert rc == 0
        torch.cuda.synchronize()
        fwd.append((m, s_, n))
        bwd.append((g_el, g_er, g_z))
    for name, a, b in zip(("m", "s", "n", "g_el", "g_er", "g_z"), fwd[0] + bwd[0], fwd[1] + bwd[1]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name
    assert float(fwd[0][1][3].abs().max()) == 0 and float(fwd[0][1][0].min()) > 0       # the empty row, a full one
    assert float(bwd[0][2].abs().max()) > 0 and float(bwd[0][0].abs().max()) > 0


@pytest.mark.parametrize("H,D", ONE_SHAPES)
def test_dropped_backward_by_source_that_keeps_every_edge_is_the_parent_bit_for_bit(H, D):
    """csl_gat_drop_bwd_t_f32 = csl_gat_bwd_t_f32 (g_z, g_el, g_er) and csl_gat_drop_bwd_t_fused_f32 =
    csl_gat_bwd_t_fused_f32 (g_z, g_er, g_attn_l, g_attn_r): 5 source rows under n_pad = 8, lists of 17, 1, 0, 17 and 1
    entries, self entries (-1) inside a list, at its end and alone, every destination in at most two edges"""
    from cslicer import aggr
    L = aggr._lib()
    rng = np.random.default_rng(H + D)
    n_src, n_pad, n_dst, Cw = 5, 8, 20, H * D
    lists = [list(range(16)) + [-1], [3], [], list(range(4, 12)) + [-1] + list(range(12, 20)), [-1]]
    assert [len(x) for x in lists] == [17, 1, 0, 17, 1]
    trow_np = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])
    assert np.bincount(trow_np[trow_np >= 0], minlength=n_dst).max() == 2
    tptr, trow = _i32(np.concatenate([[0], np.cumsum([len(x) for x in lists])])), _i32(trow_np)
    self_np = np.full(n_dst, -1)
    self_np[[0, 5, 7]] = [0, 3, 4]               # (a source is the self row of one destination at most)
    self_ids = _i32(self_np)
    src_ids, dst_ids = _i32(_ids(n_src, rng, (1 << 31) - 1)), _i32(_ids(n_dst, rng, (1 << 31) - 2))
    tail = _keep_tail(aggr, src_ids, dst_ids)
    torch.manual_seed(H * D + 1)
    el, er, z = torch.randn(n_src, H, device="cuda"), torch.randn(n_dst, H, device="cuda"), torch.randn(n_src, Cw, device="cuda")
    m = torch.full((n_dst, H), 4.0, device="cuda") + torch.rand(n_dst, H, device="cuda")
    gs, gn = torch.randn(n_dst, H, device="cuda"), torch.randn(n_dst, Cw, device="cuda")
    al, ar = torch.randn(Cw, device="cuda"), torch.randn(Cw, device="cuda")
    head = (_p(tptr), _p(trow), n_src, n_pad, _p(el), _p(er), _p(z), H, D, 0.2, _p(m), _p(gs), _p(gn))
    words = max(int(L.csl_gat_bwd_t_fused_scratch(n_pad, n_dst, H, D)), 4)
    plain, fused = [], []
    for dropped in (False, True):
        g_el, g_er = torch.full((n_src, H), -7.5, device="cuda"), torch.zeros(n_dst, H, device="cuda")
        g_z = torch.full((n_pad, Cw), -7.5, device="cuda")
        if dropped:
            rc = L.csl_gat_drop_bwd_t_f32(*head, _p(g_el), _p(g_er), _p(g_z), *tail)
        else:
            rc = L.csl_gat_bwd_t_f32(*head, _p(g_el), _p(g_er), _p(g_z), aggr._stream())
        assert rc == 0
        plain.append((g_z, g_el, g_er))
        g_er2, g_z2 = torch.full((n_dst, H), -7.5, device="cuda"), torch.full((n_pad, Cw), -7.5, device="cuda")
        g_al, g_ar = torch.full((Cw,), -7.5, device="cuda"), torch.full((Cw,), -7.5, device="cuda")
        scratch = torch.empty(words, device="cuda")
        args = head + (_p(al), _p(ar), _p(self_ids), n_dst, _p(g_er2), _p(g_z2), _p(g_al), _p(g_ar), _p(scratch))
        rc = L.csl_gat_drop_bwd_t_fused_f32(*args, *tail) if dropped else L.csl_gat_bwd_t_fused_f32(*args, aggr._stream())
        assert rc == 0
        torch.cuda.synchronize()
        fused.append((g_z2, g_er2, g_al, g_ar))
    for name, a, b in zip(("g_z", "g_el", "g_er", "fused g_z", "fused g_er", "g_attn_l", "g_attn_r"),
                          plain[0] + fused[0], plain[1] + fused[1]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), name
    g_z, g_el, g_er = plain[0]
    assert float(g_z[n_src:].abs().max()) == 0 and float(g_z[2].abs().max()) == 0 and float(g_z[0].abs().max()) > 0
    assert float(g_er.abs().max()) > 0 and float(fused[0][3].abs().max()) > 0


@pytest.mark.parametrize("n", [1, 5, 130])
@pytest.mark.parametrize("H,D", ONE_SHAPES)
def test_dropped_epilogue_that_keeps_every_element_is_the_parent_bit_for_bit(H, D, n):
    """csl_gat_finish_drop_fwd_f32: out AND y = csl_gat_finish_fwd_f32's out; csl_gat_finish_drop_bwd_f32: g_n, g_s and the
    bias gradient = csl_gat_finish_bwd_f32's; with the ELU and without"""
    from cslicer import aggr
    L = aggr._lib()
    Cw = H * D
    ids = _i32(_ids(n, np.random.default_rng(Cw + n), (1 << 31) - 1))
    tail = _keep_tail(aggr, ids)
    torch.manual_seed(n + H)
    nsum, ssum = torch.randn(n, Cw, device="cuda"), torch.rand(n, H, device="cuda") + 0.1
    bias, g = torch.randn(Cw, device="cuda"), torch.randn(n, Cw, device="cuda")
    words = max(int(L.csl_gat_finish_bwd_scratch(n, H, D)), 4)
    for elu in (1, 0):
        out_p, out_d, y = (torch.full((n, Cw), -7.5, device="cuda") for _ in range(3))
        assert L.csl_gat_finish_fwd_f32(_p(nsum), _p(ssum), _p(bias), n, H, D, elu, _p(out_p), aggr._stream()) == 0
        assert L.csl_gat_finish_drop_fwd_f32(_p(nsum), _p(ssum), _p(bias), n, H, D, elu, _p(out_d), _p(y), *tail) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out_p).all()) and torch.equal(out_d, out_p) and torch.equal(y, out_p)
        res = []
        for dropped in (False, True):
            g_n, g_s = torch.full((n, Cw), -7.5, device="cuda"), torch.full((n, H), -7.5, device="cuda")
            g_bias, scratch = torch.full((Cw,), -7.5, device="cuda"), torch.empty(words, device="cuda")
            args = (_p(g), g.stride(0), _p(out_p), _p(nsum), _p(ssum), n, H, D, elu, _p(g_n), _p(g_s), _p(g_bias), _p(scratch))
            rc = L.csl_gat_finish_drop_bwd_f32(*args, *tail) if dropped else L.csl_gat_finish_bwd_f32(*args, aggr._stream())
            assert rc == 0
            torch.cuda.synchronize()
            res.append((g_n, g_s, g_bias))
        for name, a, b in zip(("g_n", "g_s", "g_bias"), *res):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (name, elu)


# ---- identities -------------------------------------------------------------------------------------------------------------

N_NODES, F0, HIDDEN, HEADS, CLASSES, BATCH = 2000, 12, 8, 4, 5, 64
BIT_FAN = (2, 2, 2)     # a destination takes at most two atomic addends: the attention step is reproducible to the bit
P_F = 0.5


def _graph(n=N_NODES, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 13, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(d, out=indptr[1:])
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)


def _node_data(n=N_NODES, F=F0, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, F)).astype(np.float32), rng.integers(0, CLASSES, size=n).astype(np.int64),
            rng.permutation(n))


def _model(L, F=F0):
    from cslicer import splitgnn
    torch.manual_seed(L)
    model = splitgnn.DistGATModel(F, HIDDEN, CLASSES, heads=HEADS, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.bias.normal_(0, 0.3)
    return model


def _forward_backward(model, fan, seeds, feats, labels, n_parts, drop_kw, table=False):
    """(loss, [parameter gradients]) of the model on a fresh engine's first sample, all parts in this process"""
    from cslicer import _abi, aggr, splitgnn
    L = len(fan)
    indptr, indices = _graph()
    flags = (_abi.FLAG_TRANSPOSE | (0 if table else _abi.FLAG_TRANSPOSE_ALL)) if n_parts == 1 else 0
    eng = _abi.Engine(indptr, indices, n_parts=n_parts, fanouts=fan, max_batch=BATCH, mode=_abi.MODE_GRAPH, flags=flags)
    try:
        eng.submit_seeds([seeds])
        slices = splitgnn.slices_of(eng)
        model.zero_grad()
        x = {}
        for g in range(n_parts):
            rows = slices[L - 1][g].in_nodes
            x[g] = aggr.FeatureRows(feats, rows) if table else feats[rows.long()]
        out = model.forward_parts(slices, x, **drop_kw)
        seeds_t = torch.from_numpy(seeds).cuda()
        loss = 0
        for g in range(n_parts):
            top = slices[0][g]
            own = top.out_nodes[top.owned_out_nodes.long()].long()
            loss = loss + torch.nn.functional.cross_entropy(out[g], labels[own], reduction="sum") / len(seeds)
        loss.backward()
        torch.cuda.synchronize()
        assert sum(out[g].shape[0] for g in range(n_parts)) == len(seeds_t)
        return float(loss.detach()), [p.grad.clone() for p in model.parameters()]
    finally:
        eng.close()


def test_no_spec_and_zero_probabilities_are_todays_model(monkeypatch):
    """drop=None and GatDropSpec(0, 0, ...) against the call without the keyword: the same calls (no dropped twin, no
    dropout kernel), the same bits of the loss and of every gradient, on the feature table (the input layer) and on
    gathered rows.  Fanout 2/2/2, where the attention step is reproducible to the bit: its backward adds the destinations'
    logit gradients with float atomics, and at most two addends onto a zero come out the same in either order
    (test_gpu_feat16.test_attention_model_on_a_16_bit_table)."""
    from cslicer import aggr
    feats_np, labels_np, perm = _node_data()
    feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
    model = _model(3)
    calls = []
    real_call, real_drop = aggr._gat_call, aggr.dropout
    monkeypatch.setattr(aggr, "_gat_call", lambda stem, a, *args: (calls.append((stem, a is not None)), real_call(stem, a, *args))[1])
    monkeypatch.setattr(aggr, "dropout", lambda *a, **kw: (calls.append(("dropout", True)), real_drop(*a, **kw))[1])
    for table in (False, True):
        res = []
        for kw in ({}, {"drop": None}, {"drop": aggr.GatDropSpec(0.0, 0.0, 5, 3)}):
            del calls[:]
            res.append(_forward_backward(model, BIT_FAN, perm[:BATCH], feats, labels, 1, kw, table) + (list(calls),))
            assert calls and not any(dropped for _, dropped in calls)
        for r in res[1:]:
            assert r[0] == res[0][0] and r[2] == res[0][2]
            assert all(torch.equal(a, b) for a, b in zip(r[1], res[0][1])), "gradients, table %s" % table
    # the node: attn=None is the call without the argument
    rng = np.random.default_rng(1)
    indptr_np, indices_np, _, _, _ = _case(3, 20, 5, 1)
    indptr, indices = _i32(indptr_np), _i32(indices_np)
    el, er, z = torch.randn(N_SRC, 3, device="cuda"), torch.randn(5, 3, device="cuda"), torch.randn(N_SRC, 60, device="cuda")
    a = aggr.GatAggregate.apply(el, er, z, indptr, indices, 5, 3, 20, 0.2)
    b = aggr.GatAggregate.apply(el, er, z, indptr, indices, 5, 3, 20, 0.2, None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the model --------------------------------------------------------------------------------------------------------------

def _float64_model(model, fan, seeds, feats_np, labels_np, p_f, p_a, seed, step, n_parts=1):
    from oracle import oracle as orc
    indptr, indices = _graph()
    trav = orc.Oracle(indptr, indices, n_parts=n_parts, fanouts=fan).sample(seeds)
    m64 = copy.deepcopy(model).double().cpu()
    m64.zero_grad()
    out = gat_drop_ref.model_on_traversal(m64, trav, torch.from_numpy(feats_np).double(), p_f, p_a, seed, step)
    seeds_t = torch.from_numpy(seeds)
    loss = torch.nn.functional.cross_entropy(out[seeds_t], torch.from_numpy(labels_np)[seeds_t], reduction="sum") / len(seeds)
    loss.backward()
    return float(loss.detach()), [(n, p.grad) for n, p in m64.named_parameters()]


def _assert_model_close(got_loss, got_grads, want_loss, want, what=""):
    print("%sloss %.9g (float64 %.9g)" % (what, got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    for g, (name, r) in zip(got_grads, want):
        _grad_close(g.cpu(), r, 1e-4, "%sgrad %s" % (what, name))
        assert float(r.abs().max()) > 0


MODEL_SEED, MODEL_STEP = (5 << 32) | 4242, 3


@pytest.mark.parametrize("fan", [(3, 3), (3, 3, 2)], ids=["L2", "L3"])
def test_model_on_one_part_matches_float64_with_the_same_masks(fan):
    """DistGATModel.forward_parts, the fused single-part layers, both probabilities 0.5: loss and every gradient"""
    from cslicer import aggr
    feats_np, labels_np, perm = _node_data()
    feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
    model = _model(len(fan))
    seeds = perm[:BATCH]
    drop = aggr.GatDropSpec(P_F, P_A, MODEL_SEED, MODEL_STEP)
    got = _forward_backward(model, fan, seeds, feats, labels, 1, {"drop": drop})
    want = _float64_model(model, fan, seeds, feats_np, labels_np, P_F, P_A, MODEL_SEED, MODEL_STEP)
    _assert_model_close(*got, *want)
    # and it IS dropout: the same model without it, with one of the two, at another step: other losses
    others = [_forward_backward(model, fan, seeds, feats, labels, 1, kw)[0] for kw in (
        {}, {"drop": drop._replace(p_f=0.0)}, {"drop": drop._replace(p_a=0.0)}, {"drop": drop._replace(step=MODEL_STEP + 1)})]
    assert all(abs(o - got[0]) > 1e-4 * abs(got[0]) for o in others) and len(set(others)) == 4
    # each of the two alone against float64 too (feature dropout alone keeps the input layer on the feature table)
    for kw, table in ((dict(p_a=0.0), True), (dict(p_f=0.0), False)):
        d = drop._replace(**kw)
        got = _forward_backward(model, fan, seeds, feats, labels, 1, {"drop": d}, table)
        want = _float64_model(model, fan, seeds, feats_np, labels_np, d.p_f, d.p_a, MODEL_SEED, MODEL_STEP)
        _assert_model_close(*got, *want, what="%r: " % (kw,))


def test_two_parts_in_one_process_match_the_same_float64_model():
    """the masks are keyed by node ids: two parts (partial softmax states merged across them) give the one-part numbers"""
    from cslicer import aggr
    fan = (3, 3, 2)
    feats_np, labels_np, perm = _node_data()
    feats, labels = torch.from_numpy(feats_np).cuda(), torch.from_numpy(labels_np).cuda()
    model = _model(3)
    seeds = perm[:BATCH]
    drop = aggr.GatDropSpec(P_F, P_A, MODEL_SEED, MODEL_STEP)
    got = _forward_backward(model, fan, seeds, feats, labels, 2, {"drop": drop})
    want = _float64_model(model, fan, seeds, feats_np, labels_np, P_F, P_A, MODEL_SEED, MODEL_STEP, n_parts=2)
    _assert_model_close(*got, *want)


# ---- trainers ---------------------------------------------------------------------------------------------------------------

T_F, T_FAN = 16, (3, 3)      # (T_FAN: the rank test's)


def _trainer(**kw):
    from cslicer.train import Trainer
    indptr, indices = _graph()
    feats, labels, perm = _node_data(F=T_F)
    # (fanout 2/2/2: two trainers of one configuration agree to the bit, see BIT_FAN)
    t = Trainer(indptr, indices, feats, labels, CLASSES, fanouts=BIT_FAN, batch=BATCH, streams=2, hidden=HIDDEN, heads=HEADS,
                lr=1e-2, seed=3, model="gat", **kw)
    t.set_nodes(perm)
    return t


def _params(t):
    return torch.cat([p.detach().reshape(-1) for p in t.model.parameters()]).cpu()


def _run4(**kw):
    t = _trainer(**kw)
    try:
        losses = [float(x) for x in t.run(4)]
        return losses, _params(t), t.plan
    finally:
        t.close()


@pytest.fixture(scope="module")
def runs():
    both = dict(feat_dropout=0.5, attn_dropout=0.5)
    return {"a": _run4(**both), "b": _run4(**both), "c": _run4(dropout_seed=99, **both), "feat": _run4(feat_dropout=0.5),
            "feat_b": _run4(feat_dropout=0.5),
            "zero": _run4(feat_dropout=0.0, attn_dropout=0.0), "none": _run4()}


def _same_run(a, b):
    """two runs that must be ONE run: every loss, every parameter and the plan, bit for bit"""
    assert a[0] == b[0], (a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert a[2] == b[2]


def test_equal_seeds_train_bit_for_bit(runs):
    _same_run(runs["a"], runs["b"])
    _same_run(runs["feat"], runs["feat_b"])      # (feature dropout alone: the input layer stays, the drop follows it)
    assert all(np.isfinite(runs["a"][0]))


def test_another_dropout_seed_is_another_run(runs):
    other = lambda u, v: all(x != y for x, y in zip(u, v))      # noqa: E731
    assert other(runs["a"][0], runs["c"][0])
    assert other(runs["a"][0], runs["none"][0])         # and dropout is not a no-op
    assert other(runs["a"][0], runs["feat"][0]) and other(runs["feat"][0], runs["none"][0])


def test_zero_probabilities_are_the_trainer_without_the_arguments(runs):
    _same_run(runs["zero"], runs["none"])
    t = _trainer(feat_dropout=0.0, attn_dropout=0.0)
    try:
        assert t._gat_drop() == {}          # the model is called without the keyword: no dropout code at all
    finally:
        t.close()


def test_attention_dropout_turns_the_input_layer_off(runs):
    assert runs["none"][2].gat_input and runs["none"][2].input_form == "table"
    assert not runs["a"][2].gat_input and runs["a"][2].input_form == "padded"
    assert runs["feat"][2] == runs["none"][2]                                  # feature dropout alone: the plan is unchanged


def test_evaluation_never_drops():
    t = _trainer(feat_dropout=0.5, attn_dropout=0.5)
    u = _trainer()
    try:
        t.run(2)
        u.model.load_state_dict(t.model.state_dict())
        nodes = np.arange(0, N_NODES, 3)
        a, b = t.evaluate(nodes), u.evaluate(nodes)
        assert a == b and a["n"] == len(nodes) and np.isfinite(a["loss"])
        assert torch.equal(t.predict(nodes), u.predict(nodes))
    finally:
        t.close()
        u.close()


# ---- the rank form ----------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _partition(world):
    return np.random.default_rng(11).integers(0, world, size=N_NODES).astype(np.int32)


def _rank_main(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "occ-gnn_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_gpu_gat_dropout as T
        from cslicer import aggr
        from cslicer.train import Trainer
        indptr, indices = T._graph()
        feats, labels, perm = T._node_data(F=T.T_F)
        t = Trainer(indptr, indices, feats, labels, T.CLASSES, rank=rank, world=world, fanouts=T.T_FAN, batch=T.BATCH,
                    streams=1, hidden=T.HIDDEN, heads=T.HEADS, lr=1e-2, seed=3, dist=dist, rank_path=True, model="gat",
                    workload=T._partition(world), feat_dropout=T.P_F, attn_dropout=T.P_A, dropout_seed=T.MODEL_SEED)
        assert t.plan.path == "parts" and t.rank_path and not t.plan.gat_input
        fused = []
        real = aggr.GatLayerRank.apply
        aggr.GatLayerRank.apply = lambda *a: (fused.append(1), real(*a))[1]
        weights = {n: p.detach().cpu().numpy().copy() for n, p in t.model.named_parameters()}
        t.set_nodes(perm)
        reduced = []
        t.on_reduced_grads = lambda flat: reduced.append(flat.detach().cpu().clone())
        loss = torch.tensor([float(x) for x in t.run(1)], dtype=torch.float64)
        dist.all_reduce(loss)           # the minibatch's loss = the sum of the ranks' shares
        t.close()
        dist.barrier()
        q.put((rank, float(loss[0]), reduced[0].numpy(), weights, len(fused)))
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex), None, None, None))
        raise
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_float64_model_with_the_same_masks():
    """one process per part over gloo, both on this GPU: with dropout the layers run node by node (the fused rank node is
    never called), and the all-reduced loss and gradient of the first step (counter 0) are the single-process float64
    model's"""
    import torch.multiprocessing as mp
    from cslicer import splitgnn
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=150) for _ in range(world)], key=lambda x: x[0])
        for r_ in res:
            assert not isinstance(r_[1], str), r_[1]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    for rank, loss, grads, weights, fused in res:      # (all-reduced values, replicated weights: the same on every rank)
        assert loss == res[0][1] and np.array_equal(grads, res[0][2]) and fused == 0
        assert all(np.array_equal(weights[k], res[0][3][k]) for k in weights)
    feats_np, labels_np, perm = _node_data(F=T_F)
    model = splitgnn.DistGATModel(T_F, HIDDEN, CLASSES, heads=HEADS, n_layers=len(T_FAN))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in res[0][3].items()})
    want_loss, want = _float64_model(model, T_FAN, perm[:BATCH], feats_np, labels_np, P_F, P_A, MODEL_SEED, 0)
    flat, at, got = torch.from_numpy(res[0][2]), 0, []
    for p in model.parameters():
        got.append(flat[at:at + p.numel()].reshape(p.shape))
        at += p.numel()
    assert at == flat.numel()
    _assert_model_close(res[0][1], got, want_loss, want)
