"""Class weights and label smoothing of the single-label loss on the GPU (include/cslicer_loss.h, csrc/loss.hip),
everything against the float64 restatement of tests/loss_ref.py:

* k_softmax_ce_w through csl_softmax_ce_w_partial_f32 / csl_softmax_ce_w_f32 at its edges: C on both sides of the lane
  stride (64) and of the column-sum tile (256), up to 4096; 0 to 9 rows (less than, exactly and more than a block of four,
  more than one block); n_pad = n, the next multiple of 4 above n and n + 7; with and without a row map, column sums, weights
  (none, uniform in [0, 100], the label class of row 0 at weight 0), eps 0 / 0.1 / 0.9, rows at +-80, a row of equal logits;
  labels -1 and C; the host-side refusals.  Every output buffer is larger than what may be written and filled with a
  sentinel that must survive.
* the native step (csl_sage_fwd_bwd_ce) against the float64 model on the oracle's traversal;
* trainers on every path, evaluation untouched, a seeded run that learns;
* the rank path (csl_sage_rank_fwd_bwd_ce) over gloo: two ranks and a world of one, with and without overlap.

Bounds (u = 2^-24; derived, none tuned to the kernel; a ratio above 1 is a failure).  Loss and gradient are linear in the
target q, so they are the project's rules for the plain loss (tests/test_gpu_tail_edges.py) scaled by the weights:
  * a row's unscaled loss: Q (1e-5 max(loss / Q, 0.05) + C u) + (ceil(C / 64) + 8) u sum_c q_c d_c: the plain row rule times
    Q = sum_c q_c (1 for the plain loss), plus the any-order fp32 sum of the C non-negative terms q_c d_c (ceil(C / 64) per
    lane, 6 for the xor tree, 2 for the product and d_c's own sum); Q == 0 (a masked class): exactly 0;
  * a row's loss is seen alone through a call on that row only (one row per block; the lanes' work on a row does not depend
    on where the row sits); a block's partial: the fp32 sum of its four rows as the kernel formed them, 4 u sum |rows|;
  * gradient rows: 1e-4 of the tensor's largest entry; block column sums: 4 u sum |stored entries|;
  * the one-call form's summed loss: the rows' bounds added up, plus blocks u sum.
  * the steps and trainers: loss 1e-5 relative, every parameter gradient within 1e-4 of its largest entry.
Largest error / bound seen on an MI355X, per group (printed: pytest -s): loss rows 0.068, block losses 0.42, summed loss
0.050, gradient rows 0.0091, block column sums 0.44.

Finding.  The kernel first formed Q as (1 - eps) w_y + (eps / C) sum_c w_c.  With one class the softmax is 1 and the
gradient p Q - q is 0 in float64, a bound of 0; that Q and q = w_0 ((1 - eps) + eps) round differently, and the C = 1 case
with weights and eps = 0.1 saw -1.49e-8 in 9 of 9 rows.  Q is now the fp32 sum of the q_c the gradient subtracts: exactly 0.
"""
import ctypes as C
import itertools
import math
import os
import socket

import numpy as np
import pytest
import torch

import loss_ref

pytestmark = pytest.mark.gpu

E_INVALID = -1
U = 2.0 ** -24
SENT = -777.0
F64 = torch.float64
WORST = {}
LOSS_SCALE = 1.0 / 256      # a power of two: loss_partial / scale is exact, a row's loss is seen as the kernel formed it


@pytest.fixture(scope="module")
def mods():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr, aggr._lib()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + t.element_size() * off) if t is not None and t.numel() else C.c_void_p(0)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dtype).cuda().contiguous()


def _buf(numel, tail=8):
    return torch.full((numel + tail,), SENT, device="cuda")


def _within(group, got, want, bound, what):
    """|got - want| <= bound entry by entry (bound 0: equal); notes the group's largest error / bound"""
    got = got.detach().cpu().to(F64).reshape(-1)
    want, bound = want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == want.shape == bound.shape, what
    assert bool(torch.isfinite(got).all()), "%s: not finite at %s" % (what, torch.nonzero(~torch.isfinite(got))[:5, 0].tolist())
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[group] = max(WORST.get(group, 0.0), worst)
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError("%s: entry %d is %.9g, float64 %.9g: error %.3g = %.3g x its bound %.3g; %d of %d entries miss"
                             % (what, i, float(got[i]), float(want[i]), float(err[i]), worst, float(bound[i]),
                                int((ratio > 1).sum()), ratio.numel()))
    return worst


def _row_bound(loss, Q, terms, Cn):
    """on the UNSCALED loss of a row: Q (1e-5 max(loss / Q, 0.05) + C u) + (ceil(C / 64) + 8) u sum_c q_c d_c"""
    per = torch.where(Q > 0, loss / Q.clamp_min(1e-300), torch.zeros_like(loss))
    return Q * (1e-5 * per.clamp_min(0.05) + Cn * U) + (math.ceil(Cn / 64) + 8) * U * terms


# ---- the kernel through the C ABI --------------------------------------------------------------------------------------------

CLASSES = [1, 2, 3, 47, 63, 64, 65, 256, 257, 1000, 4096]
ROWS = [0, 1, 3, 4, 5, 9]
WEIGHTS = ["none", "uniform", "zero"]
EPS = [0.0, 0.1, 0.9]
SHIFTS = [0.0, 80.0, -80.0]
PADS = ["n", "next4", "n+7"]


def _combos(Cn):
    """(n, weights, eps) in full; the n_pad form, the offset, the row map and the column sums drawn per combination from a
    seeded generator (every value of each is drawn for every C: asserted)"""
    rng = np.random.default_rng(77 + Cn)
    out = []
    for k, (n, wk, eps) in enumerate(itertools.product(ROWS, WEIGHTS, EPS)):
        out.append(dict(n=n, wk=wk, eps=eps, pad=PADS[int(rng.integers(3))], shift=SHIFTS[int(rng.integers(3))],
                        use_map=bool(rng.integers(2)), cols=bool(rng.integers(2)) and Cn <= 256, seed=1000 * Cn + k))
    for key, vals in (("pad", PADS), ("shift", SHIFTS), ("use_map", [False, True])):
        assert {c[key] for c in out} == set(vals)
        for wk in WEIGHTS:       # ... and beside every kind of weights
            assert {c[key] for c in out if c["wk"] == wk and c["n"] > 0} == set(vals)
    assert Cn > 256 or {c["cols"] for c in out} == {False, True}
    return out


def _case(Cn, n, wk, eps, pad, shift, use_map, seed, **_):
    rng = np.random.default_rng(seed)
    n_pad = {"n": n, "next4": (n // 4 + 1) * 4, "n+7": n + 7}[pad]
    ldl, ldgr = Cn + 3, Cn + 5
    n_nodes, n_lab = n + 20, n + 30
    ids = rng.permutation(n_nodes)[:n]
    rowmap = rng.permutation(n_lab)[:n_nodes] if use_map else None
    lab_rows = rowmap[ids] if use_map else ids
    labels = rng.integers(0, Cn, size=n_lab if use_map else n_nodes)
    zbuf = rng.standard_normal((n_pad + 1, ldl)).astype(np.float32)      # (the pad columns and rows: anything finite)
    zbuf[:n, :Cn] = (rng.standard_normal((n, Cn)) + shift).astype(np.float32)
    if n >= 3:
        zbuf[1, :Cn] = np.float32(shift + 0.5)                           # a row of equal logits
    w = None
    if wk != "none":
        w = (rng.random(Cn) * 100).astype(np.float32)
        if wk == "zero" and n:
            w[labels[lab_rows[0]]] = 0.0                                 # row 0's label class is masked
    return dict(C=Cn, n=n, n_pad=n_pad, ldl=ldl, ldgr=ldgr, ids=ids, rowmap=rowmap, labels=labels, zbuf=zbuf, w=w, eps=eps,
                lab_rows=lab_rows)


def _device(cs, labels=None):
    return dict(z=_dev(cs["zbuf"]), ids=_dev(cs["ids"], torch.int32),
                rm=_dev(cs["rowmap"], torch.int32) if cs["rowmap"] is not None else None,
                lab=_dev(cs["labels"] if labels is None else labels, torch.int64),
                w=_dev(cs["w"]) if cs["w"] is not None else None)


def _run_partial(mods, cs, d, with_cols, row=None):
    """the partial entry point on the whole case, or on row `row` alone (n = n_pad = 1)"""
    aggr, L = mods
    Cn = cs["C"]
    n, n_pad, first = (cs["n"], cs["n_pad"], 0) if row is None else (1, 1, row)
    blocks = (n_pad + 3) // 4
    grad = torch.full((n_pad + 2, cs["ldgr"]), SENT, device="cuda")
    lpart = _buf(blocks)
    cpart = _buf(blocks * Cn) if with_cols else None
    rc = L.csl_softmax_ce_w_partial_f32(_ptr(d["z"], first * cs["ldl"]), cs["ldl"], n, n_pad, Cn, _ptr(d["ids"], first),
                                        _ptr(d["rm"]), _ptr(d["lab"]), _ptr(d["w"]), cs["eps"], LOSS_SCALE, _ptr(grad),
                                        cs["ldgr"], _ptr(lpart), _ptr(cpart), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    # rows past n_pad and columns past C of the wider gradient buffer, the floats behind the partials
    assert bool((grad[n_pad:] == SENT).all()) and bool((grad[:, Cn:] == SENT).all())
    assert bool((lpart[blocks:] == SENT).all()) and (cpart is None or bool((cpart[blocks * Cn:] == SENT).all()))
    return grad[:n_pad, :Cn], lpart[:blocks], (cpart[:blocks * Cn].view(blocks, Cn) if with_cols else None)


def _run_whole(mods, cs, d):
    aggr, L = mods
    Cn, n = cs["C"], cs["n"]
    grad = torch.full((n + 2, cs["ldgr"]), SENT, device="cuda")
    ns = int(L.csl_softmax_ce_scratch(n))
    scratch, loss = _buf(ns), _buf(1)
    rc = L.csl_softmax_ce_w_f32(_ptr(d["z"]), cs["ldl"], n, Cn, _ptr(d["ids"]), _ptr(d["rm"]), _ptr(d["lab"]), _ptr(d["w"]),
                                cs["eps"], LOSS_SCALE, _ptr(loss), _ptr(grad), cs["ldgr"], _ptr(scratch), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((grad[n:] == SENT).all()) and bool((grad[:, Cn:] == SENT).all())
    assert bool((scratch[ns:] == SENT).all()) and bool((loss[1:] == SENT).all())
    return grad[:n, :Cn], loss[0]


def _reference(cs, labels=None):
    return loss_ref.weighted_ce(cs["zbuf"], cs["ldl"], cs["n"], cs["n_pad"], cs["C"], cs["ids"], cs["rowmap"],
                                cs["labels"] if labels is None else labels, cs["w"], cs["eps"], LOSS_SCALE)


def _check(mods, cs, with_cols, what):
    Cn, n, n_pad = cs["C"], cs["n"], cs["n_pad"]
    blocks = (n_pad + 3) // 4
    d = _device(cs)
    want_rows, want_g, want_cs, Q, terms = _reference(cs)
    grad, lpart, cpart = _run_partial(mods, cs, d, with_cols)
    g = grad.cpu().double()               # (n_pad == 0: nothing may be launched, and every comparison below is over nothing)
    gmax = float(want_g.abs().max()) if want_g.numel() else 0.0
    # each row's loss, unscaled (the scale is a power of two), from a call on that row alone; its gradient row is the same
    own = torch.zeros(4 * blocks, dtype=F64)
    for r in range(n):
        g1, lp1, _ = _run_partial(mods, cs, d, False, row=r)
        own[r] = float(lp1[0])
        assert torch.equal(g1[0].cpu(), grad[r].cpu()), "%s: row %d alone has another gradient row" % (what, r)
    _within("loss rows", own[:n] / LOSS_SCALE, want_rows / LOSS_SCALE, _row_bound(want_rows / LOSS_SCALE, Q, terms, Cn),
            "loss rows " + what)
    if cs["w"] is not None and cs["eps"] == 0.0 and n and float(cs["w"][cs["labels"][cs["lab_rows"][0]]]) == 0.0:
        assert float(own[0]) == 0.0 and bool((g[0] == 0).all()), "%s: a masked class has a loss or a gradient" % what
    # a block's partial: its four rows' losses added in fp32
    _within("loss blocks", lpart, own.view(blocks, 4).sum(1), 4 * U * own.view(blocks, 4).abs().sum(1), "block losses " + what)
    # gradient rows: 1e-4 of the tensor's largest entry; padding rows zero
    _within("gradient", g, want_g, torch.full_like(want_g, 1e-4 * gmax), "gradient rows " + what)
    assert bool((grad[n:] == 0).all())
    if with_cols:
        # a block's column sums are 4 stored gradient entries added in fp32: any order, 4 terms
        gp = torch.zeros((4 * blocks, Cn), dtype=F64)
        gp[:n_pad] = g
        gp = gp.view(blocks, 4, Cn)
        _within("loss colsum", cpart, gp.sum(1), 4 * U * gp.abs().sum(1), "block column sums " + what)
        tot = cpart.cpu().double().sum(0)
        assert float((tot - want_cs).abs().max()) <= 1e-4 * float(want_cs.abs().max())
    # the one-call form: the same gradient rows; the summed loss: the rows' bounds added up plus blocks u sum
    grad1, loss1 = _run_whole(mods, cs, d)
    assert torch.equal(grad1.cpu(), grad[:n].cpu())
    want_sum = float(want_rows.sum())
    bound = float((_row_bound(want_rows / LOSS_SCALE, Q, terms, Cn) * LOSS_SCALE).sum()) + ((n + 3) // 4) * U * abs(want_sum)
    _within("loss sum", loss1.reshape(1), torch.tensor([want_sum], dtype=F64), torch.tensor([bound], dtype=F64),
            "summed loss " + what)


@pytest.mark.parametrize("Cn", CLASSES)
def test_kernel_against_float64_at_its_edges(mods, Cn):
    for cb in _combos(Cn):
        cs = _case(Cn, **cb)
        _check(mods, cs, cb["cols"], "C=%d n=%d n_pad=%d %s eps=%g shift=%g map=%d cols=%d" % (
            Cn, cs["n"], cs["n_pad"], cb["wk"], cb["eps"], cb["shift"], cb["use_map"], cb["cols"]))
    print("C = %d, largest error / bound so far: %s" % (Cn, ", ".join("%s %.6g" % kv for kv in sorted(WORST.items()))))


@pytest.mark.parametrize("Cn,shift,wk,eps", [(1, 0.0, "uniform", 0.1), (3, 80.0, "none", 0.1), (64, 0.0, "uniform", 0.0),
                                             (256, -80.0, "uniform", 0.9), (300, 0.0, "none", 0.0)])
def test_bad_labels_are_their_rows_nan_alone(mods, Cn, shift, wk, eps):
    """labels -1 and C: NaN for the row's loss, its block's partial and column sums and the total, NaN for its gradient row;
    every other row within its bounds"""
    cs = _case(Cn, 9, wk, eps, "n+7", shift, Cn % 2 == 1, 500 + Cn)
    n, n_pad = cs["n"], cs["n_pad"]
    with_cols = Cn <= 256
    labels = cs["labels"].copy()
    labels[cs["lab_rows"][2]], labels[cs["lab_rows"][4]] = -1, Cn           # blocks 0 and 1; block 2 (row 8) is clean
    bad = np.zeros(n_pad, dtype=bool)
    bad[[2, 4]] = True
    d = _device(cs, labels)
    want_rows, want_g, _, Q, terms = _reference(cs, labels)
    assert np.array_equal(torch.isnan(want_rows).numpy(), bad[:n]) and np.array_equal(torch.isnan(want_g).all(1).numpy(), bad)
    grad, lpart, cpart = _run_partial(mods, cs, d, with_cols)
    g = grad.cpu().double()
    assert bool(torch.isnan(g[bad]).all()) and bool(torch.isnan(lpart.cpu()[:2]).all()) and bool(torch.isfinite(lpart.cpu()[2:]).all())
    ok = torch.from_numpy(~bad)
    _within("gradient", g[ok], want_g[ok], torch.full_like(want_g[ok], 1e-4 * float(want_g[ok].abs().max())),
            "bad labels, the other rows C=%d" % Cn)
    for r in range(n):
        _, lp1, _ = _run_partial(mods, cs, d, False, row=r)
        if bad[r]:
            assert bool(torch.isnan(lp1[0]))
        else:
            _within("loss rows", lp1[:1] / LOSS_SCALE, want_rows[r:r + 1] / LOSS_SCALE,
                    _row_bound(want_rows[r:r + 1] / LOSS_SCALE, Q[r:r + 1], terms[r:r + 1], Cn), "bad labels, row %d C=%d" % (r, Cn))
    if with_cols:
        cp = cpart.cpu()
        assert bool(torch.isnan(cp[:2]).all()) and bool(torch.isfinite(cp[2:]).all())
    grad1, loss1 = _run_whole(mods, cs, d)
    assert bool(torch.isnan(loss1)) and torch.equal(torch.isnan(grad1.cpu()).all(1), torch.from_numpy(bad[:n]))


def test_entry_points_refuse_and_leave_the_buffers_alone(mods):
    aggr, L = mods
    cs = _case(8, 5, "uniform", 0.1, "n+7", 0.0, True, 3)
    d = _device(cs)
    grad, lpart, cpart, loss, scratch = _buf(12 * 13), _buf(3), _buf(3 * 300), _buf(1), _buf(2)
    st = aggr._stream()
    part = dict(z=_ptr(d["z"]), ldl=11, n=5, n_pad=12, C=8, ids=_ptr(d["ids"]), rm=_ptr(d["rm"]), lab=_ptr(d["lab"]),
                w=_ptr(d["w"]), eps=0.1, scale=1.0, grad=_ptr(grad), ldgr=13, lpart=_ptr(lpart), cpart=_ptr(cpart), st=st)
    one = dict(z=_ptr(d["z"]), ldl=11, n=5, C=8, ids=_ptr(d["ids"]), rm=_ptr(d["rm"]), lab=_ptr(d["lab"]), w=_ptr(d["w"]),
               eps=0.1, scale=1.0, loss=_ptr(loss), grad=_ptr(grad), ldgr=13, scratch=_ptr(scratch), st=st)
    nul = C.c_void_p(0)
    common = (dict(eps=1.0), dict(eps=-0.1), dict(eps=float("nan")), dict(eps=float("inf")), dict(n=-1), dict(C=0),
              dict(C=4097), dict(ldl=7), dict(ldgr=7), dict(z=nul), dict(ids=nul), dict(lab=nul), dict(grad=nul))
    for bad in common + (dict(n_pad=4), dict(lpart=nul), dict(C=257, ldl=300, ldgr=300)):
        assert L.csl_softmax_ce_w_partial_f32(*dict(part, **bad).values()) == E_INVALID, bad
    for bad in common + (dict(loss=nul), dict(scratch=nul)):
        assert L.csl_softmax_ce_w_f32(*dict(one, **bad).values()) == E_INVALID, bad
    torch.cuda.synchronize()
    for b in (grad, lpart, cpart, loss, scratch):
        assert bool((b == SENT).all())
    # and the wrapper: class_weight of another length or type is a TypeError before the call
    z = torch.zeros((4, 8), device="cuda")
    ids, lab = torch.arange(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    for w in (torch.ones(7, device="cuda"), torch.ones(8, device="cuda", dtype=torch.float64), torch.ones(8)):
        with pytest.raises(TypeError):
            aggr.SoftmaxCE.apply(z, ids, lab, 1.0, None, w, 0.0)
    from cslicer import _abi
    with pytest.raises(_abi.CslError):
        aggr.SoftmaxCE.apply(z, ids, lab, 1.0, None, None, 1.0)


def test_autograd_node_defaults_are_the_plain_call(mods):
    """SoftmaxCE with both options at their defaults is bitwise the five-argument call; with options its backward hands the
    kernel's gradient on"""
    aggr, _ = mods
    rng = np.random.default_rng(4)
    z_np = rng.standard_normal((37, 47)).astype(np.float32)
    ids = torch.from_numpy(rng.permutation(60)[:37].astype(np.int32)).cuda()
    lab_np = rng.integers(0, 47, size=60)
    lab = torch.from_numpy(lab_np).cuda()
    outs = []
    for tail in ((), (None, None, 0.0)):
        z = torch.from_numpy(z_np).cuda().requires_grad_()
        loss = aggr.SoftmaxCE.apply(z, ids, lab, 0.125, *tail)
        loss.backward()
        outs.append((loss.detach().cpu(), z.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    w_np = (rng.random(47) * 3).astype(np.float32)
    z = torch.from_numpy(z_np).cuda().requires_grad_()
    loss = aggr.SoftmaxCE.apply(z, ids, lab, 0.125, None, torch.from_numpy(w_np).cuda(), 0.1)
    (2.0 * loss).backward()
    rows, g, _, _, _ = loss_ref.weighted_ce(z_np, 47, 37, 37, 47, ids.cpu().numpy(), None, lab_np, w_np, 0.1, 0.125)
    assert abs(float(loss) - float(rows.sum())) <= 1e-5 * float(rows.sum()) and float(loss) != float(outs[0][0])
    _within("gradient", z.grad, 2.0 * g, torch.full_like(g, 2e-4 * float(g.abs().max())), "autograd node")


# ---- the native step -------------------------------------------------------------------------------------------------------

N_NODES, F0, HIDDEN, BATCH = 2000, 12, 24, 64
ROW_PAD, N_SLABS = 64, 4
P, SEED, STEP = 0.5, (5 << 32) | 4242, 3
EPS_ON = 0.1


def _graph(n=N_NODES, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 13, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(d, out=indptr[1:])
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)


def _node_data(Cn, n=N_NODES, F=F0, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, F)).astype(np.float32), rng.integers(0, Cn, size=n).astype(np.int64), rng.permutation(n))


def _class_weight(Cn):
    return (0.2 + 2.8 * np.random.default_rng(100 + Cn).random(Cn)).astype(np.float32)


def _model(L, Cn, F=F0):
    from cslicer import splitgnn
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(F, HIDDEN, Cn, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    return model


def _native(model, fan, seeds, feats, labels, drop, loss_spec):
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
            step(order, feats, labels, 1.0 / len(seeds), loss, drop, loss=loss_spec)
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


def _step_against_float64(fan, Cn, use_w, eps, drop=None):
    from cslicer import aggr
    from oracle import oracle as orc
    L = len(fan)
    feats, labels, perm = _node_data(Cn)
    seeds = perm[:BATCH]
    model = _model(L, Cn)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    w = _class_weight(Cn) if use_w else None
    spec = aggr.LossSpec(torch.from_numpy(w).cuda() if use_w else None, eps)
    got_loss, got = _native(model, fan, seeds, x, lab, aggr.DropSpec(*drop) if drop else None, spec)
    indptr, indices = _graph()
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    want_loss, want = loss_ref.model_on_traversal(trav, feats, labels, ws, bs, N_NODES, w, eps, drop)
    _assert_close(got_loss, got.double().cpu(), want_loss, want)
    # and the options are live: the plain step (with the same masks) is another loss
    plain_loss, _ = _native(model, fan, seeds, x, lab, aggr.DropSpec(*drop) if drop else None, None)
    assert abs(plain_loss - got_loss) > 1e-4 * abs(plain_loss)


@pytest.mark.parametrize("fused", [True, False], ids=["fused-deepest-layer", "no-mfma-fwd"])
@pytest.mark.parametrize("Cn", [47, 300], ids=["C47-top-cols", "C300-column-sum-pass"])
@pytest.mark.parametrize("fan", [(4,), (3, 3), (3, 3, 2)], ids=["L1", "L2", "L3"])
def test_native_step_matches_float64(fan, Cn, fused, monkeypatch):
    from cslicer import aggr
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    assert aggr._lib().csl_sage_fwd_mfma_scratch(F0, HIDDEN) > 0        # these widths are the fused layer's
    _step_against_float64(fan, Cn, True, EPS_ON)


@pytest.mark.parametrize("use_w,eps", [(True, 0.0), (False, EPS_ON)], ids=["weights-alone", "smoothing-alone"])
def test_native_step_with_one_option_alone(use_w, eps):
    _step_against_float64((3, 3), 47, use_w, eps)


@pytest.mark.parametrize("fan,Cn", [((3, 3, 2), 47), ((3, 3), 300)], ids=["L3-C47", "L2-C300"])
def test_native_step_with_dropout_under_the_same_masks(fan, Cn):
    _step_against_float64(fan, Cn, True, EPS_ON, drop=(P, SEED, STEP))


def test_bfloat16_table_is_its_float32_upcast():
    from cslicer import aggr
    feats, labels, perm = _node_data(47)
    t16 = torch.from_numpy(feats).to(torch.bfloat16).cuda()
    lab = torch.from_numpy(labels).cuda()
    model = _model(3, 47)
    spec = aggr.LossSpec(torch.from_numpy(_class_weight(47)).cuda(), EPS_ON)
    a = _native(model, (3, 3, 2), perm[:BATCH], t16, lab, None, spec)
    b = _native(model, (3, 3, 2), perm[:BATCH], t16.float(), lab, None, spec)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


def test_steps_refuse_a_loss_spec_with_packed_labels():
    from cslicer import aggr
    model = _model(2, 47)
    step = aggr.SageStep(model, ROW_PAD, N_SLABS)
    words = torch.zeros((N_NODES, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError, match="single-label"):
        step([], torch.zeros((N_NODES, F0), device="cuda"), words, 1.0, torch.zeros(1, device="cuda"),
             loss=aggr.LossSpec(None, 0.1))
    rank = aggr.SageRankStep(model, ROW_PAD, N_SLABS, None)
    with pytest.raises(TypeError, match="single-label"):
        rank([], torch.zeros((N_NODES, F0), device="cuda"), None, None, None, words, 1.0, torch.zeros(1, device="cuda"),
             loss=aggr.LossSpec(None, 0.1))


# ---- trainers (the tiny graph of the dropout tests) --------------------------------------------------------------------------

T_F, T_FAN, T_C = 16, (3, 3), 5
T_W = [0.5, 2.0, 1.0, 0.0, 3.5]


def _trainer(**kw):
    from cslicer.train import Trainer
    indptr, indices = _graph()
    feats, labels, perm = _node_data(T_C, F=T_F)
    kw.setdefault("hidden", HIDDEN)
    t = Trainer(indptr, indices, feats, labels, T_C, fanouts=T_FAN, batch=BATCH, streams=2, lr=1e-2, seed=3, **kw)
    t.set_nodes(perm)
    return t


def _params(t):
    return torch.cat([p.detach().reshape(-1) for p in t.model.parameters()]).cpu()


def _float64_first_step(weights, w, eps, fan=T_FAN):
    from oracle import oracle as orc
    indptr, indices = _graph()
    feats, labels, perm = _node_data(T_C, F=T_F)
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(perm[:BATCH])
    return loss_ref.model_on_traversal(trav, feats, labels, weights[0::2], weights[1::2], N_NODES,
                                       None if w is None else np.asarray(w, dtype=np.float32), eps)


def test_default_options_are_the_trainer_without_them():
    runs = []
    for kw in (dict(), dict(class_weight=None, label_smoothing=0.0), dict(class_weight=T_W, label_smoothing=EPS_ON)):
        t = _trainer(**kw)
        try:
            assert t.plan.path == "native" and (t.loss_spec is None) == (len(runs) < 2)
            runs.append((t.run(4), _params(t), t.plan))
        finally:
            t.close()
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] == runs[2][2]
    assert all(np.isfinite(runs[2][0])) and all(a != b for a, b in zip(runs[0][0], runs[2][0]))


def test_native_step_against_the_autograd_step_at_the_first_step(monkeypatch):
    kw = dict(class_weight=T_W, label_smoothing=EPS_ON)
    t = _trainer(**kw)
    try:
        assert t.native is not None and t.loss_spec is not None
        loss_n = t.run(1)[0]
        grads_n = t.native.grads.double().cpu()
    finally:
        t.close()
    monkeypatch.setenv("CSLICER_PY_STEP", "1")
    t = _trainer(**kw)
    try:
        assert t.native is None and t.plan.path == "local"
        loss_p = t.run(1)[0]
        want = []
        for conv in t.model.convs:
            want += [conv.fc.weight.grad.double().cpu(), conv.fc.bias.grad.double().cpu()]
    finally:
        t.close()
    _assert_close(loss_n, grads_n, loss_p, want)


@pytest.mark.parametrize("path", ["local", "parts"])
def test_autograd_paths_against_float64_at_the_first_step(path, monkeypatch):
    from cslicer import splitgnn
    if path == "local":
        monkeypatch.setenv("CSLICER_PY_STEP", "1")
    else:
        monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", True)
    t = _trainer(class_weight=T_W, label_smoothing=EPS_ON)
    try:
        assert t.plan.path == path
        weights = [p.detach().cpu().numpy().copy() for p in t.model.parameters()]
        loss = t.run(1)[0]
        got = torch.cat([p.grad.double().reshape(-1) for p in t.model.parameters()]).cpu()
    finally:
        t.close()
    want_loss, want = _float64_first_step(weights, T_W, EPS_ON)
    _assert_close(loss, got, want_loss, want, path + ": ")


def test_attention_model_hands_the_options_to_torchs_loss(monkeypatch):
    """GAT on the `parts` path: torch's cross_entropy with the same arguments, against float64 on its own logits"""
    seen = {}
    real = torch.nn.functional.cross_entropy

    def spy(logits, y, **kw):
        logits.register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))
        seen.update(logits=logits.detach().clone(), y=y.clone(), kw=kw)
        return real(logits, y, **kw)
    monkeypatch.setattr(torch.nn.functional, "cross_entropy", spy)
    t = _trainer(model="gat", heads=2, hidden=8, class_weight=T_W, label_smoothing=EPS_ON)
    try:
        assert t.plan.path == "parts"
        loss = t.run(1)[0]
    finally:
        t.close()
    assert seen["kw"]["reduction"] == "sum" and seen["kw"]["label_smoothing"] == EPS_ON
    assert torch.equal(seen["kw"]["weight"].cpu(), torch.tensor(T_W))
    assert seen["logits"].shape == (BATCH, T_C)
    rows, g, _, _ = loss_ref.rows_ce(seen["logits"].cpu().numpy(), seen["y"].cpu().numpy(), np.asarray(T_W, dtype=np.float32),
                                     EPS_ON, 1.0 / BATCH)
    want = float(rows.sum())
    print("GAT loss %.9g (float64 %.9g)" % (loss, want))
    assert abs(loss - want) <= 1e-5 * abs(want)
    _within("GAT logit gradient", seen["grad"], g, torch.full_like(g, 1e-4 * float(g.abs().max())), "GAT")


def test_evaluation_is_the_plain_one():
    t = _trainer(class_weight=T_W, label_smoothing=EPS_ON)
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


def test_a_seeded_run_with_balanced_weights_and_smoothing_learns():
    from cslicer import train
    n, F, Cn = 2000, 16, 5
    indptr, indices = _graph(n, seed=2)
    feats = train.synthetic_node_data(n, F, 2, seed=1)[0]
    # a long-tailed target a model can learn: the largest of five offset columns of the node's own feature row
    y = np.argmax(feats[:, :Cn] + np.array([0.3, 0.15, 0.0, 0.0, -0.1], dtype=np.float32), axis=1).astype(np.int64)
    perm = np.random.default_rng(0).permutation(n)
    w = train.balanced_class_weight(y[perm], Cn)
    assert w.max() > 2 * w.min() > 0
    t = train.Trainer(indptr, indices, feats, y, Cn, fanouts=(3, 2), batch=64, streams=2, hidden=32, lr=1e-2, seed=1,
                      class_weight=w, label_smoothing=0.1)
    try:
        assert t.plan.path == "native"
        t.set_nodes(perm)
        losses = t.run(150)
    finally:
        t.close()
    first, last = float(np.mean(losses[:6])), float(np.mean(losses[-6:]))
    print("loss %.4f -> %.4f" % (first, last))
    assert np.isfinite(losses).all() and last < first


# ---- the rank path: csl_sage_rank_fwd_bwd_ce over gloo on one GPU --------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _partition(world):
    return np.random.default_rng(11).integers(0, world, size=N_NODES).astype(np.int32)


def _rank_main(rank, world, port, overlap, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "occ-gnn_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_gpu_loss as T
        from cslicer.train import Trainer
        indptr, indices = T._graph()
        feats, labels, perm = T._node_data(T.T_C, F=T.T_F)
        t = Trainer(indptr, indices, feats, labels, T.T_C, rank=rank, world=world, fanouts=T.T_FAN, batch=T.BATCH,
                    streams=1, hidden=T.HIDDEN, lr=1e-2, seed=3, dist=dist, rank_path=True, overlap=overlap,
                    workload=T._partition(world) if world > 1 else None, class_weight=T.T_W, label_smoothing=T.EPS_ON)
        assert t.plan.path == "native_rank" and t.native_rank is not None and t.native is None and t.loss_spec is not None
        weights = [p.detach().cpu().numpy().copy() for p in t.model.parameters()]
        t.set_nodes(perm)
        loss = torch.tensor(t.run(1), dtype=torch.float64)
        grads = t.native_rank.grads.detach().cpu().numpy().copy()      # all-reduced in place by the step
        dist.all_reduce(loss)           # the minibatch's loss = the sum of the ranks' shares
        t.close()
        dist.barrier()
        q.put((rank, float(loss[0]), grads, weights))
    except Exception as ex:      # the parent must hear about it instead of waiting for the queue
        q.put((rank, "error: " + repr(ex), None, None))
        raise
    dist.destroy_process_group()


RANK_RUNS = {}


def _rank_run(world, overlap):
    if (world, overlap) in RANK_RUNS:
        return RANK_RUNS[(world, overlap)]
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, overlap, q)) for r in range(world)]
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
    for rank, loss, grads, weights in res:      # (all-reduced values, replicated weights: the same on every rank)
        assert loss == res[0][1] and np.array_equal(grads, res[0][2])
        assert all(np.array_equal(a, b) for a, b in zip(weights, res[0][3]))
    RANK_RUNS[(world, overlap)] = res[0][1:]
    return RANK_RUNS[(world, overlap)]


@pytest.mark.parametrize("world,overlap", [(2, False), (1, False), (2, True)],
                         ids=["two-ranks", "one-rank-on-the-rank-path", "two-ranks-overlap"])
def test_ranks_sum_to_the_float64_model(world, overlap):
    loss, grads, weights = _rank_run(world, overlap)
    want_loss, want = _float64_first_step(weights, T_W, EPS_ON)
    _assert_close(loss, torch.from_numpy(grads).double(), want_loss, want, "world %d%s: " % (world, ", overlap" if overlap else ""))
    if overlap:
        # the schedule changes, the numbers do not (up to the order of the boundary rows' atomic adds)
        loss0, grads0, _ = _rank_run(world, False)
        assert abs(loss - loss0) <= 1e-6 * abs(loss0)
        assert float(np.abs(grads - grads0).max()) <= 1e-5 * float(np.abs(grads0).max())
