"""Multi-label classification on the GPU (include/cslicer_multilabel.h, csrc/multilabel.hip) against the float64
restatement of tests/bce_ref.py:

* k_sigmoid_bce through the C ABI (csl_sigmoid_bce_partial_f32 / csl_sigmoid_bce_f32), in the manner of
  tests/test_gpu_tail_edges.py: sentinel-filled oversize buffers, ldl = C + 3, ldgr = C + 5, ldw = W + 1, ids with and
  without rowmap, with and without col_partial, at the edges of the kernel (a wave walks a row in strides of 64 columns,
  a label word holds 32, the column sums stop at 256, a block is four rows): C in 1 .. 4096, n around one block and
  around 223 blocks, rows at 0, +80 and -80, all-zero logits, all-ones and all-zeros label rows, garbage in the unused
  bits, Inf and NaN;
* csl_infer_eval_multilabel_f32: predictions and tp / fp / fn exactly, the loss within the rows' bounds;
* the native step (csl_sage_fwd_bwd_multilabel) against the float64 model on the oracle's traversal, with and without
  dropout, a bfloat16 table bitwise equal to its upcast;
* trainers: native against CSLICER_PY_STEP=1, determinism, the attention model's loss, evaluate against the head on
  predict()'s logits, learning on train.synthetic_multilabels;
* two ranks over gloo on one GPU (the `parts` path) against the single-process float64 model, and their evaluation.

Tolerances (u = 2^-24; derived, none tuned to the kernel; a ratio above 1 is a failure):
  * gradient rows of the loss: 1e-4 of the tensor's largest entry (the project's rule for gradients);
  * a row's loss: 1e-5 max(loss, 0.05) + k u sum_c |l_c|, k counted beside _row_bound below;
  * block column sums: the any-order rule, k u sum |terms| over the four rows' fp32 gradient entries, k = 4;
  * the step and the trainers: loss 1e-5 relative, every parameter gradient within 1e-4 of its largest entry.

Largest error / bound seen on an MI355X, per group (the tests print them: pytest -s):
    gradient rows 0.00092    loss rows 0.0152    loss sum 0.0113    block column sums 0.435
    evaluation head: loss rows 0.0135, loss sum 0.0070    the attention model's logit gradient 0.0014
The step and the trainers: loss within 1.4e-7 relative, gradients within 2.4e-7 of their largest entry.
"""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

import bce_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -777.0
F64 = torch.float64
WORST = {}
CLASSES = [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4096]
LOSS_SCALE = 1.0 / 256      # a power of two: loss_partial / scale is exact, a row's loss is seen as the kernel formed it
FILL = 110.0                # a filler row's logits: +110 under a set bit, -110 under a clear one.  expf(-110) is 0 in fp32
                            # (below half the smallest denormal), so its loss and gradient row are exactly 0; in float64
                            # the row's loss is C * 1.7e-48


@pytest.fixture(scope="module")
def mods():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr, aggr._lib()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + t.element_size() * off) if t is not None else C.c_void_p(0)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def _buf(numel, tail=8):
    return torch.full((numel + tail,), SENT, device="cuda")


def _within(group, got, want, bound, what):
    """|got - want| <= bound entry by entry; notes and prints the group's largest error / bound"""
    got = got.detach().cpu().to(F64).reshape(-1)
    want, bound = want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == want.shape == bound.shape, what
    assert bool(torch.isfinite(got).all()), "%s: not finite at %s" % (what, torch.nonzero(~torch.isfinite(got))[:5, 0].tolist())
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("error / bound: %-16s %.6g   (%s; largest of the group so far %.6g)" % (group, worst, what, WORST[group]))
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError("%s: entry %d is %.9g, float64 %.9g: error %.3g = %.3g x its bound %.3g; %d of %d entries miss"
                             % (what, i, float(got[i]), float(want[i]), float(err[i]), worst, float(bound[i]),
                                int((ratio > 1).sum()), ratio.numel()))


def _row_bound(l, Cn):
    """1e-5 max(loss, 0.05) + k u sum_c |l_c| on the UNSCALED loss of every row of l [rows, C] (float64 elements).
    k = 7 + ceil(C / 64) + 6, from the kernel's own order of operations:
      * an element is l_c = t + log1pf(expf(-|z|)) with t one of z, 0, -z (exact) and t >= 0, so log1p(e) <= l_c.  expf
        is within 1 ulp = 2 u of e, which moves log1p(e) by at most 2 u e <= 4 u log1p(e) (e <= 2 log1p(e) on [0, 1]);
        log1pf is within 1 ulp = 2 u of its value; the addition rounds once, u l_c: 7 u l_c per element;
      * a lane adds its ceil(C / 64) elements serially, then six xor-shuffle steps add the 64 lanes: every term goes through
        at most ceil(C / 64) + 6 roundings of partial sums that are no larger than the row's sum (all terms are >= 0).
    The scale is a power of two here: the product is exact."""
    k = 7 + (Cn + 63) // 64 + 6
    loss = l.sum(1)
    return 1e-5 * loss.clamp_min(0.05) + k * U * l.abs().sum(1)


def _case(Cn, n, shift, use_map, seed, garbage="random"):
    """Blocks of four consecutive rows.  In block b row 4 b + b % 4 is MEASURED (N(0, 3) + shift; random labels) and the
    others are fillers (an exactly zero loss and gradient row), so loss_partial[b] is that row's loss times the scale;
    every tenth block is fillers only.  The first measured rows are special: all-zero logits, an all-ones and an
    all-zeros label row.  garbage: what the bits at and above C of the last word and the pad word of a label row hold."""
    rng = np.random.default_rng(seed)
    n_pad = n + 7
    W = (Cn + 31) // 32
    ldl, ldgr, ldw = Cn + 3, Cn + 5, W + 1
    n_nodes, n_lab = n + 50, n + 90
    ids = rng.permutation(n_nodes)[:n]
    rowmap = rng.permutation(n_lab)[:n_nodes] if use_map else None
    lab_rows = rowmap[ids] if use_map else ids
    y_all = rng.random((n_lab if use_map else n_nodes, Cn)) < 0.4
    r = np.arange(n)
    measured = (r % 4) == ((r // 4) % 4)
    measured[(r // 4) % 10 == 9] = False
    if n < 8:
        measured[:] = True                         # (a single block or two: every row is looked at through the gradient)
    m_rows = np.nonzero(measured)[0]
    z = (rng.standard_normal((n, Cn)) * 3 + shift).astype(np.float32)
    if m_rows.size > 0:
        z[m_rows[0]] = 0.0                                         # all-zero logits: C log 2
    if m_rows.size > 1:
        y_all[lab_rows[m_rows[1]]] = True
    if m_rows.size > 2:
        y_all[lab_rows[m_rows[2]]] = False
    y = y_all[lab_rows]
    fill = ~measured
    z[fill] = np.where(y[fill], np.float32(FILL), np.float32(-FILL))
    zbuf = rng.standard_normal((n_pad + 1, ldl)).astype(np.float32)
    zbuf[:n, :Cn] = z
    words = np.zeros((y_all.shape[0], ldw), dtype=np.uint32)
    words[:, :W] = bce_ref.pack(y_all)
    spare = np.uint32((0xFFFFFFFF << (Cn % 32)) & 0xFFFFFFFF) if Cn % 32 else np.uint32(0)
    if garbage == "random":
        junk = rng.integers(0, 1 << 32, size=words.shape, dtype=np.uint64).astype(np.uint32)
    else:
        junk = np.full(words.shape, 0xFFFFFFFF if garbage == "ones" else 0, dtype=np.uint32)
    words[:, W - 1] |= junk[:, W - 1] & spare
    words[:, W] = junk[:, W]
    return dict(C=Cn, n=n, n_pad=n_pad, W=W, ldl=ldl, ldgr=ldgr, ldw=ldw, ids=ids, rowmap=rowmap, y=y, z=z, zbuf=zbuf,
                words=words.view(np.int32), measured=measured)


def _args(cs):
    return (_dev(cs["zbuf"]), _dev(cs["ids"], torch.int32),
            _dev(cs["rowmap"], torch.int32) if cs["rowmap"] is not None else None, _dev(cs["words"], torch.int32))


def _run_partial(mods, cs, with_cols):
    aggr, L = mods
    Cn, n, n_pad = cs["C"], cs["n"], cs["n_pad"]
    blocks = (n_pad + 3) // 4
    zd, ids, rm, wd = _args(cs)
    grad = torch.full((n_pad + 2, cs["ldgr"]), SENT, device="cuda")
    lpart = _buf(blocks)
    cpart = _buf(blocks * Cn) if with_cols else None
    rc = L.csl_sigmoid_bce_partial_f32(_ptr(zd), cs["ldl"], n, n_pad, Cn, _ptr(ids), _ptr(rm), _ptr(wd), cs["ldw"], LOSS_SCALE,
                                       _ptr(grad), cs["ldgr"], _ptr(lpart), _ptr(cpart), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    # rows past n_pad and columns past C of the wider gradient buffer, the floats behind the partials
    assert bool((grad[n_pad:] == SENT).all()) and bool((grad[:, Cn:] == SENT).all())
    assert bool((lpart[blocks:] == SENT).all()) and (cpart is None or bool((cpart[blocks * Cn:] == SENT).all()))
    return grad[:n_pad, :Cn], lpart[:blocks], (cpart[:blocks * Cn].view(blocks, Cn) if with_cols else None)


def _run_whole(mods, cs):
    aggr, L = mods
    Cn, n = cs["C"], cs["n"]
    zd, ids, rm, wd = _args(cs)
    grad = torch.full((n + 2, cs["ldgr"]), SENT, device="cuda")
    ns = int(L.csl_sigmoid_bce_scratch(n))
    assert ns == (n + 3) // 4
    scratch, loss = _buf(ns), _buf(1)
    rc = L.csl_sigmoid_bce_f32(_ptr(zd), cs["ldl"], n, Cn, _ptr(ids), _ptr(rm), _ptr(wd), cs["ldw"], LOSS_SCALE, _ptr(loss),
                               _ptr(grad), cs["ldgr"], _ptr(scratch), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((grad[n:] == SENT).all()) and bool((grad[:, Cn:] == SENT).all())
    assert bool((scratch[ns:] == SENT).all()) and bool((loss[1:] == SENT).all())
    return grad[:n, :Cn], loss[0]


def _check_case(mods, cs, what):
    Cn, n, n_pad = cs["C"], cs["n"], cs["n_pad"]
    blocks = (n_pad + 3) // 4
    _, rows, gwant, _ = bce_ref.sigmoid_bce(cs["z"], cs["y"], LOSS_SCALE, n_pad=n_pad)
    l, _ = bce_ref.elements(cs["z"], cs["y"])
    rb = _row_bound(l, Cn) * LOSS_SCALE
    m0 = np.nonzero(cs["measured"])[0][0]
    assert abs(float(rows[m0]) / LOSS_SCALE - Cn * np.log(2.0)) <= 1e-12 * Cn        # the all-zero row: C log 2
    want_lp, _ = bce_ref.block_partials(rows, gwant, n_pad)
    bound_lp, _ = bce_ref.block_partials(rb, gwant, n_pad)
    # (where a block holds more than one measured row -- n < 8 -- its four losses are added in fp32: four terms, 4 u)
    bound_lp = bound_lp + 4 * U * bce_ref.block_partials(rows.abs(), gwant, n_pad)[0] * (1 if n < 8 else 0)
    gmax = float(gwant.abs().max())
    outs = []
    for with_cols in ([True, False] if Cn <= 256 else [False]):
        grad, lpart, cpart = _run_partial(mods, cs, with_cols)
        outs.append((grad.clone(), lpart.clone()))
        assert bool((grad[n:] == 0).all())                                     # the padding rows of the GEMM operand
        assert bool((grad[:n][torch.from_numpy(~cs["measured"]).cuda()] == 0).all())      # fillers: exactly zero
        _within("gradient rows", grad, gwant, torch.full_like(gwant, 1e-4 * gmax), what)
        # (a block's partial = its one measured row's loss: the fillers add exact zeros, in float64 C * 1.7e-48)
        _within("loss rows", lpart, want_lp, bound_lp, what)
        if with_cols:
            g4 = torch.zeros((blocks * 4, Cn), dtype=F64)
            g4[:n_pad] = grad.cpu().to(F64)
            g4 = g4.view(blocks, 4, Cn)
            # the kernel's (a + b) + (c + d) of its own fp32 entries: four terms in any order, k = 4
            _within("block column sums", cpart, g4.sum(1), 4 * U * g4.abs().sum(1), what)
    if len(outs) == 2:       # the column sums change neither the gradient nor the loss
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    grad, loss = _run_whole(mods, cs)
    assert torch.equal(grad, outs[0][0][:n])
    # the blocks' partials summed in an order of the reduction's choosing: (blocks + 4) u sum |rows| on top of the rows' bounds
    tot = rows.sum().reshape(1)
    _within("loss sum", loss.reshape(1), tot, (rb.sum() + (blocks + 4) * U * rows.abs().sum()).reshape(1), what)
    return outs[0]


@pytest.mark.parametrize("Cn", CLASSES)
def test_kernel_against_float64_at_its_edges(mods, Cn):
    k = 0
    for n in [1, 3, 4, 5, 889, 890, 891, 892]:
        for shift in (0.0, 80.0, -80.0):
            cs = _case(Cn, n, shift, use_map=k % 2 == 0, seed=Cn * 1009 + k)
            _check_case(mods, cs, "C %d, n %d, shift %+g, %s" % (Cn, n, shift, "rowmap" if k % 2 == 0 else "ids"))
            k += 1


@pytest.mark.parametrize("Cn", [1, 31, 33, 64, 257])
def test_unused_label_bits_change_nothing(mods, Cn):
    """the last word's bits at and above C (and the pad word of ldw = W + 1) as ones and as zeros: bitwise the same"""
    aggr, L = mods
    res = []
    for garbage in ("ones", "zeros"):
        cs = _case(Cn, 45, 0.0, True, seed=Cn, garbage=garbage)
        grad, lpart, cpart = _run_partial(mods, cs, Cn <= 256)
        y = cs["y"]
        yw = _dev(cs["words"][cs["rowmap"][cs["ids"]]], torch.int32)
        zd = _dev(cs["z"])
        pred = torch.zeros((45, cs["W"]), dtype=torch.int32, device="cuda")
        lrow, lsum, cnt = torch.zeros(45, device="cuda"), torch.zeros(1, dtype=F64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
        assert L.csl_infer_eval_multilabel_f32(_ptr(zd), Cn, 45, Cn, _ptr(yw), cs["ldw"], _ptr(pred), _ptr(lrow), _ptr(lsum),
                                               _ptr(cnt), aggr._stream()) == 0
        torch.cuda.synchronize()
        res.append([t.cpu() for t in (grad, lpart, pred, lrow, lsum, cnt)] + ([cpart.cpu()] if cpart is not None else []))
        assert cnt.tolist() == list(bce_ref.eval_head(cs["z"], y)[1])
    if Cn % 32:
        a, b = (_case(Cn, 45, 0.0, True, seed=Cn, garbage=g)["words"] for g in ("ones", "zeros"))
        assert not np.array_equal(a[:, -2], b[:, -2])          # the two inputs do differ in the last word
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_a_non_finite_logit_is_its_rows_nan_alone(mods):
    Cn, n = 70, 21
    cs = _case(Cn, n, 0.0, False, seed=5)
    cs["measured"][:] = True
    clean = _run_partial(mods, cs, True)
    bad = dict(cs, zbuf=cs["zbuf"].copy())
    bad["zbuf"][6, 3], bad["zbuf"][13, 69] = np.inf, np.nan
    grad, lpart, cpart = _run_partial(mods, bad, True)
    rows = torch.ones(cs["n_pad"], dtype=torch.bool)
    rows[6] = rows[13] = False
    blk = torch.ones(lpart.numel(), dtype=torch.bool)
    blk[6 // 4] = blk[13 // 4] = False
    assert bool(torch.isnan(grad[6]).all()) and bool(torch.isnan(grad[13]).all())
    assert bool(torch.isnan(lpart[~blk]).all()) and bool(torch.isnan(cpart[~blk]).all())
    assert torch.equal(grad[rows], clean[0][rows]) and torch.equal(lpart[blk], clean[1][blk])
    assert torch.equal(cpart[blk], clean[2][blk])
    g2, loss = _run_whole(mods, bad)
    assert bool(torch.isnan(loss)) and torch.equal(g2[rows[:n]], clean[0][:n][rows[:n]]) and bool(torch.isnan(g2[6]).all())


def test_entry_points_refuse_bad_arguments(mods):
    aggr, L = mods
    x = torch.zeros(64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    nul, st = C.c_void_p(0), aggr._stream()
    f = L.csl_sigmoid_bce_partial_f32
    assert f(_ptr(x), 5000, 1, 1, 4097, _ptr(i), nul, _ptr(i), 200, 1.0, _ptr(x), 5000, _ptr(x), nul, st) == -1
    assert f(_ptr(x), 300, 1, 1, 257, _ptr(i), nul, _ptr(i), 9, 1.0, _ptr(x), 300, _ptr(x), _ptr(x), st) == -1
    for bad in range(4):
        a = [_ptr(x), 8, 2, 2, 8, _ptr(i), nul, _ptr(i), 1, 1.0, _ptr(x), 8, _ptr(x), nul, st]
        a[(0, 5, 7, 10)[bad]] = nul
        assert f(*a) == -1
    assert L.csl_sigmoid_bce_f32(_ptr(x), 8, 2, 8, _ptr(i), nul, _ptr(i), 1, 1.0, nul, _ptr(x), 8, _ptr(x), st) == -1
    assert L.csl_infer_eval_multilabel_f32(_ptr(x), 8, 2, 8, _ptr(i), 1, _ptr(i), _ptr(x), nul, _ptr(i), st) == -1
    torch.cuda.synchronize()
    assert bool((x == 0).all())


# ---- the evaluation head ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", CLASSES)
def test_eval_head_counts_exactly(mods, Cn):
    from cslicer import infer
    aggr, L = mods
    W = (Cn + 31) // 32
    for n in (0, 1, 5, 1000):
        rng = np.random.default_rng(Cn * 31 + n)
        z = (rng.standard_normal((n, Cn)) * 3).astype(np.float32)
        z[rng.random((n, Cn)) < 0.1] = 0.0                       # a logit of exactly 0 predicts negative
        z[rng.random((n, Cn)) < 0.02] = -0.0
        y = rng.random((n, Cn)) < 0.4
        ld, ldw = Cn + 3, W + 1
        zb = torch.full((n + 1, ld), SENT, device="cuda")
        zb[:n, :Cn] = _dev(z)
        words = np.zeros((n + 1, ldw), dtype=np.uint32)
        words[:n, :W] = bce_ref.pack(y)
        words[:, W] = 0xFFFFFFFF
        if Cn % 32:
            words[:, W - 1] |= np.uint32((0xFFFFFFFF << (Cn % 32)) & 0xFFFFFFFF)
        wd = _dev(words.view(np.int32), torch.int32)
        pred = torch.full(((n + 1) * W,), -7, dtype=torch.int32, device="cuda")
        lrow, lsum = _buf(n), torch.full((2,), SENT, dtype=F64, device="cuda")
        cnt = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        rc = L.csl_infer_eval_multilabel_f32(_ptr(zb), ld, n, Cn, _ptr(wd), ldw, _ptr(pred), _ptr(lrow), _ptr(lsum), _ptr(cnt),
                                             aggr._stream())
        assert rc == 0
        torch.cuda.synchronize()
        want_pred, counts, want_rows = bce_ref.eval_head(z, y)
        assert np.array_equal(pred[:n * W].cpu().numpy().view(np.uint32).reshape(n, W), bce_ref.pack(want_pred))
        assert bool((pred[n * W:] == -7).all()) and bool((lrow[n:] == SENT).all())
        assert cnt.tolist() == list(counts) + [-7] and float(lsum[1]) == SENT
        l, _ = bce_ref.elements(z, y)
        rb = _row_bound(l, Cn)
        what = "C %d, n %d" % (Cn, n)
        _within("eval loss rows", lrow[:n], want_rows, rb, what)
        # float64 additions of the fp32 rows: the rows' own bounds (and 1e-15 of the sum)
        _within("eval loss sum", lsum[:1], want_rows.sum().reshape(1), (rb.sum() + 1e-15 * want_rows.sum()).reshape(1), what)
        # the wrapper: the same numbers
        p2, c2, s2 = infer.eval_head_multilabel(zb[:n, :Cn], wd[:n, :W])
        assert torch.equal(p2.reshape(-1), pred[:n * W]) and c2 == counts and s2 == float(lsum[0])


# ---- the native step ---------------------------------------------------------------------------------------------------------

N_NODES, F0, BATCH = 300, 12, 37
ROW_PAD, N_SLABS = 64, 4
P, SEED, STEP = 0.5, (5 << 32) | 4242, 3


def _graph(n=N_NODES, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 9, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(d, out=indptr[1:])
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)


def _node_data(Cn, n=N_NODES, F=F0, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, F)).astype(np.float32), rng.random((n, Cn)) < 0.3, rng.permutation(n)


def _model(L, hidden, Cn, F=F0):
    from cslicer import splitgnn
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(F, hidden, Cn, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    return model


def _native(model, fan, seeds, feats, words, Cn, drop):
    """(loss, flat gradients) of one native step on a fresh engine's first sample"""
    from cslicer import _abi, aggr, splitgnn
    L = len(fan)
    indptr, indices = _graph()
    eng = _abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=BATCH, mode=_abi.MODE_GRAPH,
                      flags=_abi.FLAG_TRANSPOSE)
    try:
        eng.submit_seeds([seeds])
        slices = splitgnn.slices_of(eng)
        order = [slices[L - 1 - k][0] for k in range(L)]
        step = aggr.SageStep(model, ROW_PAD, N_SLABS)
        loss = torch.zeros(1, device="cuda")
        for _ in range(2):     # (the second call runs on the recorded GEMM plans and the reused workspace)
            step(order, feats, words, 1.0 / (len(seeds) * Cn), loss, drop)
        torch.cuda.synchronize()
        return float(loss[0]), step.grads.clone()
    finally:
        eng.close()


def _assert_close(got_loss, got_grads, want_loss, want, what=""):
    print("%sloss %.9g (float64 %.9g)" % (what, got_loss, want_loss))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    at = 0
    for k, g in enumerate(want):
        seg = got_grads[at:at + g.numel()].reshape(g.shape)
        at += g.numel()
        err, ref = float((seg - g).abs().max()), float(g.abs().max())
        print("%sgradient %d: max error %.3g, largest entry %.3g" % (what, k, err, ref))
        assert ref > 0 and err <= 1e-4 * ref, "gradient %d (%s of layer %d): max error %.3g against a largest entry of %.3g" % (
            k, "weight" if k % 2 == 0 else "bias", k // 2, err, ref)
    assert at == got_grads.numel()


STEP_CASES = [((3,), 8, 5), ((3,), 8, 260)] + [((3, 2), 8, Cn) for Cn in (5, 40, 121, 260)] + \
             [((3, 2, 2), 16, Cn) for Cn in (5, 40, 121, 260)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused-deepest-layer", "no-mfma-fwd"])
@pytest.mark.parametrize("fan,hidden,Cn", STEP_CASES, ids=["L%d-h%d-C%d" % (len(f), h, c) for f, h, c in STEP_CASES])
def test_native_step_matches_float64(fan, hidden, Cn, fused, monkeypatch):
    from cslicer import aggr
    from oracle import oracle as orc
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    L = len(fan)
    feats, y, perm = _node_data(Cn)
    seeds = perm[:BATCH]
    model = _model(L, hidden, Cn)
    x, words = torch.from_numpy(feats).cuda(), torch.from_numpy(aggr.pack_labels(y)).cuda()
    got_loss, got = _native(model, fan, seeds, x, words, Cn, None)
    indptr, indices = _graph()
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    want_loss, want = bce_ref.model_on_traversal(trav, feats, y, ws, bs, N_NODES)
    _assert_close(got_loss, got.double().cpu(), want_loss, want)


@pytest.mark.parametrize("fan,hidden,Cn", [((3, 2), 8, 260), ((3, 2, 2), 16, 40)], ids=["L2-C260", "L3-C40"])
def test_native_step_with_dropout_matches_float64_with_the_same_masks(fan, hidden, Cn):
    from cslicer import aggr
    from oracle import oracle as orc
    feats, y, perm = _node_data(Cn)
    seeds = perm[:BATCH]
    model = _model(len(fan), hidden, Cn)
    x, words = torch.from_numpy(feats).cuda(), torch.from_numpy(aggr.pack_labels(y)).cuda()
    got_loss, got = _native(model, fan, seeds, x, words, Cn, aggr.DropSpec(P, SEED, STEP))
    indptr, indices = _graph()
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    want_loss, want = bce_ref.model_on_traversal(trav, feats, y, ws, bs, N_NODES, drop=(P, SEED, STEP))
    _assert_close(got_loss, got.double().cpu(), want_loss, want)
    plain_loss, _ = _native(model, fan, seeds, x, words, Cn, None)
    assert abs(plain_loss - got_loss) > 1e-4 * abs(plain_loss)                 # and it IS dropout


def test_bfloat16_table_is_its_float32_upcast():
    from cslicer import aggr
    Cn = 121
    feats, y, perm = _node_data(Cn)
    t16 = torch.from_numpy(feats).to(torch.bfloat16).cuda()
    words = torch.from_numpy(aggr.pack_labels(y)).cuda()
    model = _model(3, 16, Cn)
    for drop in (None, aggr.DropSpec(P, SEED, STEP)):
        a = _native(model, (3, 2, 2), perm[:BATCH], t16, words, Cn, drop)
        b = _native(model, (3, 2, 2), perm[:BATCH], t16.float(), words, Cn, drop)
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


def test_step_refuses_labels_that_are_not_packed_words():
    from cslicer import aggr
    feats, y, perm = _node_data(40)
    model = _model(2, 8, 40)
    x = torch.from_numpy(feats).cuda()
    with pytest.raises(TypeError, match="packed words"):
        _native(model, (3, 2), perm[:BATCH], x, torch.from_numpy(y.astype(np.int64)).cuda(), 40, None)


# ---- trainers --------------------------------------------------------------------------------------------------------------

T_F, T_FAN, T_C, T_HIDDEN = 16, (3, 2), 40, 16


def _trainer(**kw):
    from cslicer.train import Trainer
    indptr, indices = _graph()
    feats, y, perm = _node_data(T_C, F=T_F)
    kw.setdefault("hidden", T_HIDDEN)
    t = Trainer(indptr, indices, feats, y, T_C, fanouts=T_FAN, batch=BATCH, streams=2, lr=1e-2, seed=3, multilabel=True, **kw)
    t.set_nodes(perm)
    return t


def _params(t):
    return torch.cat([p.detach().reshape(-1) for p in t.model.parameters()]).cpu()


def test_trainer_holds_the_packed_labels():
    t = _trainer()
    try:
        _, y, _ = _node_data(T_C, F=T_F)
        assert t.multilabel and t.plan.path == "native" and t.labels.dtype == torch.int32 and t.labels.shape == (N_NODES, 2)
        assert np.array_equal(t.labels.cpu().numpy().view(np.uint32), bce_ref.pack(y))
    finally:
        t.close()


def test_equal_seeds_train_bit_for_bit():
    runs = []
    for kw in (dict(), dict(), dict(dropout=0.5, replace=False, feature_dtype="bfloat16"),
               dict(dropout=0.5, replace=False, feature_dtype="bfloat16")):
        t = _trainer(**kw)
        try:
            assert t.plan.path == "native"
            runs.append((t.run(4), _params(t)))
        finally:
            t.close()
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and all(np.isfinite(runs[0][0]))
    assert runs[2][0] == runs[3][0] and torch.equal(runs[2][1], runs[3][1]) and all(np.isfinite(runs[2][0]))
    assert runs[0][0] != runs[2][0]
    assert 0.3 < runs[0][0][0] < 2.0          # a mean over elements: about log 2 at the start, not 40 times that


@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_native_step_against_the_autograd_step_at_the_first_step(dropout, monkeypatch):
    """same minibatch, same weights (same masks): csl_sage_fwd_bwd_multilabel and CSLICER_PY_STEP=1 (the fused autograd
    layers, torch's GEMMs, aggr.SigmoidBCE)"""
    t = _trainer(dropout=dropout)
    try:
        assert t.native is not None
        loss_n = t.run(1)[0]
        grads_n = t.native.grads.double().cpu()
    finally:
        t.close()
    monkeypatch.setenv("CSLICER_PY_STEP", "1")
    t = _trainer(dropout=dropout)
    try:
        assert t.native is None and t.plan.path == "local"
        loss_p = t.run(1)[0]
        want = []
        for conv in t.model.convs:
            want += [conv.fc.weight.grad.double().cpu(), conv.fc.bias.grad.double().cpu()]
    finally:
        t.close()
    _assert_close(loss_n, grads_n, loss_p, want)


def test_attention_model_trains_through_sigmoid_bce(monkeypatch):
    """GAT on the `parts` path: the loss and the logit gradient of aggr.SigmoidBCE against float64 on the same logits"""
    from cslicer import aggr
    seen = {}
    real = aggr.SigmoidBCE.apply

    def spy(logits, ids, words, scale, rowmap=None):
        logits.register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))
        seen.update(logits=logits.detach().clone(), ids=ids.clone(), scale=scale, strides=logits.stride())
        return real(logits, ids, words, scale, rowmap)
    monkeypatch.setattr(aggr.SigmoidBCE, "apply", spy)
    t = _trainer(model="gat", heads=2, hidden=8)
    try:
        assert t.plan.path == "parts"
        loss = t.run(1)[0]
        _, y, _ = _node_data(T_C, F=T_F)
        ids = seen["ids"].cpu().numpy()
        assert seen["logits"].shape == (BATCH, T_C) and seen["scale"] == 1.0 / (BATCH * T_C)
        want, _, gwant, _ = bce_ref.sigmoid_bce(seen["logits"].cpu().numpy(), y[ids], seen["scale"])
        print("GAT loss %.9g (float64 %.9g)" % (loss, want))
        assert abs(loss - want) <= 1e-5 * abs(want)
        _within("GAT logit gradient", seen["grad"], gwant, torch.full_like(gwant, 1e-4 * float(gwant.abs().max())), "GAT")
        assert np.isfinite(t.run(2)).all()
    finally:
        t.close()


def test_evaluate_is_the_head_on_predicts_logits():
    from cslicer import infer
    t = _trainer()
    try:
        t.run(3)
        nodes = np.arange(1, N_NODES, 3)
        ev = t.evaluate(nodes)
        lg = t.predict(nodes)
        _, y, _ = _node_data(T_C, F=T_F)
        _, (tp, fp, fn), loss = infer.eval_head_multilabel(lg, t.labels[torch.from_numpy(nodes).cuda()])
        assert (ev["tp"], ev["fp"], ev["fn"], ev["n"]) == (tp, fp, fn, len(nodes))
        assert ev["loss"] == loss / (len(nodes) * T_C) and ev["micro_f1"] == bce_ref.micro_f1(tp, fp, fn)
        assert set(ev) == {"micro_f1", "loss", "n", "tp", "fp", "fn"}
        # and the counts are numpy's on the same logits
        assert (tp, fp, fn) == bce_ref.eval_head(lg.cpu().numpy(), y[nodes])[1]
        assert infer.evaluate(t.model, t.eng.indptr, t.eng.indices, t.feat, nodes, t.labels, multilabel=True) == ev
    finally:
        t.close()


def test_a_seeded_run_learns_the_synthetic_multilabels():
    from cslicer import train
    n, F, Cn = 2000, 16, 10
    indptr, indices = _graph(n, seed=2)
    feats = train.synthetic_node_data(n, F, 2, seed=1)[0]
    y = train.synthetic_multilabels(n, Cn, seed=1, feat_dim=F)
    perm = np.random.default_rng(0).permutation(n)
    held, tr_nodes = perm[:400], perm[400:]
    t = train.Trainer(indptr, indices, feats, y, Cn, fanouts=(3, 2), batch=64, streams=2, hidden=32, lr=1e-2, seed=1,
                      multilabel=True)
    try:
        assert t.plan.path == "native"
        before = t.evaluate(held)
        t.set_nodes(tr_nodes)
        losses = t.run(150)
        after = t.evaluate(held)
    finally:
        t.close()
    first, last = float(np.mean(losses[:6])), float(np.mean(losses[-6:]))
    print("loss %.4f -> %.4f, held-out micro-F1 %.4f -> %.4f" % (first, last, before["micro_f1"], after["micro_f1"]))
    assert last < first and after["micro_f1"] > before["micro_f1"] and after["loss"] < before["loss"]


# ---- two ranks over gloo on one GPU ---------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _partition(world):
    return np.random.default_rng(11).integers(0, world, size=N_NODES).astype(np.int32)


EVAL_NODES = np.arange(2, N_NODES, 2)


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
        import test_gpu_multilabel as T
        from cslicer.train import Trainer
        indptr, indices = T._graph()
        feats, y, perm = T._node_data(T.T_C, F=T.T_F)
        t = Trainer(indptr, indices, feats, y, T.T_C, rank=rank, world=world, fanouts=T.T_FAN, batch=T.BATCH, streams=1,
                    hidden=T.T_HIDDEN, lr=1e-2, seed=3, dist=dist, rank_path=True, workload=T._partition(world),
                    multilabel=True)
        assert t.plan.path == "parts" and t.native_rank is None and t.rank_path
        weights = [p.detach().cpu().numpy().copy() for p in t.model.parameters()]
        t.set_nodes(perm)
        reduced = []
        t.on_reduced_grads = lambda flat: reduced.append(flat.detach().cpu().clone())
        loss = torch.tensor(t.run(1), dtype=torch.float64)
        dist.all_reduce(loss)           # the minibatch's loss = the sum of the ranks' shares
        ev = t.evaluate(T.EVAL_NODES)
        lg = t.predict(T.EVAL_NODES).cpu().numpy()
        mine = T.EVAL_NODES[t.owns(T.EVAL_NODES)]
        counts = bce_ref.eval_head(lg, y[mine])[1] + (len(mine),)
        t.close()
        dist.barrier()
        q.put((rank, float(loss[0]), reduced[0].numpy(), weights, ev, counts))
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex), None, None, None, None))
        raise
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_float64_model_and_evaluate_together():
    import torch.multiprocessing as mp
    from oracle import oracle as orc
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
    for rank, loss, grads, weights, ev, counts in res:      # (all-reduced values, replicated weights: the same on every rank)
        assert loss == res[0][1] and np.array_equal(grads, res[0][2]) and ev == res[0][4]
        assert all(np.array_equal(a, b) for a, b in zip(weights, res[0][3]))
    indptr, indices = _graph()
    feats, y, perm = _node_data(T_C, F=T_F)
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=T_FAN).sample(perm[:BATCH])
    ws, bs = res[0][3][0::2], res[0][3][1::2]
    want_loss, want = bce_ref.model_on_traversal(trav, feats, y, ws, bs, N_NODES)
    _assert_close(res[0][1], torch.from_numpy(res[0][2]).double(), want_loss, want, "world 2: ")
    # evaluation: the ranks' own counts, from their own logits, add up to the collective's
    ev = res[0][4]
    tot = np.sum([r_[5] for r_ in res], axis=0)
    assert (ev["tp"], ev["fp"], ev["fn"], ev["n"]) == tuple(int(v) for v in tot) and ev["n"] == len(EVAL_NODES)
    assert ev["micro_f1"] == bce_ref.micro_f1(ev["tp"], ev["fp"], ev["fn"]) and np.isfinite(ev["loss"]) and ev["loss"] > 0
