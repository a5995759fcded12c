"""The row-wise kernels that close every training step, called through the C ABI against the float64 restatement in
tests/tail_ref.py: the loss (csl_softmax_ce_partial_f32 / csl_softmax_ce_f32), Adam (csl_adam_f32), the attention
logits (csl_gat_logits_fwd_f32 / _bwd_acc_f32), the attention epilogue (csl_gat_finish_fwd_f32 / _bwd_f32) and
csl_bias_elu_f32 / csl_elu_bwd_colsum_f32.

What decides how a kernel runs, and what is therefore varied here:
  * k_softmax_ce: one wave per row, 4 rows per block, lanes stride the C classes (C around 64 and 256, up to 4096);
    SM_CMAX = 256 classes for the column sums; the row's offset (logits of about +-80);
  * k_adam: 1,024 elements per block, up to 24 tensors back to back in one launch, empty tensors among them;
  * the attention row kernels: gsz = D / 4 lanes per head, lpc = (64 / gsz) * gsz live lanes per wave, so a row is walked in
    chunks of 4 * lpc columns: a partial chunk, exactly one chunk and one head past it for gsz = 1, 2, 3, 5, 8, 17 (lpc =
    51), 48, 63 and 64; gat_finish_rows(n) rows per block (4 up to 4,096 rows, then steps of 4, rb_rows(n) beyond 131,072
    rows, which doubles beyond 262,144), the second stage over zero blocks (n = 0), the accumulate flag;
  * k_elu_bwd_colsum: BLK / (C / 4) rows of a block at once (C = 252: 4 rows on 252 of 256 threads).

Every output buffer is larger than what the kernel may write and filled with a sentinel that must survive: rows past n
or n_pad, columns past C under a wider leading dimension, the floats behind a scratch buffer of exactly the size the
_scratch function reports.

Tolerances (u = 2^-24; every one derived, none tuned to a kernel; a ratio above 1 is a failure):
  * an entry that goes through k fp32 roundings: k u (sum of the |terms| of that entry), k counted beside the assertion;
    where it is tighter, the project's rule, 1e-5 of the row's largest float64 entry (test_gpu_gat_edges._rows_close);
  * a sum of k terms in any order: k u (sum of the |terms|), the rule of tests/test_gpu_sage_aggr.py, which counts one
    more for every further rounding a term or the sum goes through -- they are counted beside the assertion too;
  * a row's loss: 1e-5 max(loss, 0.05) + C u (the project's 1e-5; logf of a sum rounded to fp32 cannot be relatively
    accurate for a vanishing loss, hence the floor; C u is the any-order bound on the sum of the exponentials);
  * gradient rows of the loss: 1e-4 of the tensor's largest entry (the project's rule for gradients);
  * Adam: |m' - m64| <= 4 u (|b1 m| + |(1-b1) g|), |v' - v64| <= 4 u (b2 v + (1-b2) g^2),
    |p' - p64| <= 2 u |p64| + 16 u |update| with p64 evaluated in float64 from the kernel's own stored m', v' (so that a
    cancellation in the moments stays out of the parameter's bound): the update goes through seven roundings (lr / bc1,
    1 / sqrt(bc2), sqrtf, its product, + eps, step_size * m', the quotient), doubled for a division and a square root
    that need not be correctly rounded.

Finding.  k_softmax_ce formed scale * (logf(s) + m - z[label]), which rounds at the size of the logits.  On the build
before this file 4 of the 33 per-row loss cases fail, C = 2 and C = 3 at +80 and at -80: 46, 62, 27 and 30 of their 200
measured rows miss the bound, the worst by 6.17 times (a row loss of 0.0241 off by 3.8e-6); at 47 classes and more the
same error stays inside the bound's C u.  It now forms (m - z[label]) + logf(s), as k_infer_eval_rows does: no case
fails, worst row 0.147 of its bound.  A label outside [0, C) was used as an index into the row, and the gradient row
silently became scale * softmax (the 5 bad-label cases fail there): the row's loss and gradient row are now NaN.

Largest error / bound seen on an MI355X, per group (the tests print them to six digits: pytest -s):
    loss rows 0.147 (C = 3, +80)    loss sum 0.0061 (C = 257, -80)    gradient rows 0.0028 (C = 4096)
    block column sums 0.12    Adam m 0.45, v 0.49, p 0.50    finish 0.91 (g_n, D = 256)
    logits 0.998271 (g_attn_r at n = 1: one product, one rounding)
    ELU kernels 0.9999997 (y + bias without the ELU: one rounding; 2.0435944 + 1.9564068 lands just above 4)
The last two bounds ARE the rounding limit of a single fp32 operation (half a unit in the last place is at most u of the
result, and the result is no larger than the sum of the |terms|), so ratios just under 1 are what a correct kernel gives;
1 itself cannot be reached (it would need an exact sum that is a power of two, which has no rounding error).  The error
and these bounds are evaluated in float64 from fp32 values -- a difference of two fp32 numbers, a sum of two magnitudes, a
power of two -- which float64 holds exactly unless the operands lie more than 2^29 apart, so `ratio > 1` does not hang
on float64 rounding there; for the longer bounds the float64 evaluation is off by 1e-16 of the bound at most.

Scratch checks, not in the tree.  The `gl + o < gsz` guard of k_gat_logits_fwd's tree dropped: the 24 cases of D = 12 (H =
21, 22), D = 20 and D = 68 fail (el off by O(1)); D = 12 with one head, D = 192 and D = 252 pass, and so do the powers of
two: where a chunk holds a single head the lanes past it hold zeros, so the guard only matters where heads share a chunk.
gat_finish_rows replaced by a constant 4: everything passes, rightly: the choice only sets speed, and the scratch size
follows it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tail_ref as T

pytestmark = pytest.mark.gpu

E_INVALID = -1
U = 2.0 ** -24
SENT = -777.0
F64 = torch.float64
WORST = {}


@pytest.fixture(scope="module")
def mods():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr, aggr._lib()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off) if t is not None else C.c_void_p(0)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dtype).cuda().contiguous()


def _buf(numel, tail=8):
    """`numel` floats to be written, followed by `tail` more; all sentinels"""
    return torch.full((numel + tail,), SENT, device="cuda")


def _tail_ok(b, numel):
    return bool((b[numel:] == SENT).all())


def _within(group, got, want, bound, what):
    """|got - want| <= bound entry by entry (bound 0: equal); notes and prints the group's largest error / bound"""
    got = got.detach().cpu().to(F64).reshape(-1)
    want, bound = want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == want.shape == bound.shape, what
    assert bool(torch.isfinite(got).all()), "%s: not finite at %s" % (what, torch.nonzero(~torch.isfinite(got))[:5, 0].tolist())
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("error / bound: %-14s %.6g   (%s; largest of the group so far %.6g)" % (group, worst, what, WORST[group]))
    if worst > 1.0:
        i = int(ratio.argmax())
        raise AssertionError("%s: entry %d is %.9g, float64 %.9g: error %.3g = %.3g x its bound %.3g; %d of %d entries miss"
                             % (what, i, float(got[i]), float(want[i]), float(err[i]), worst, float(bound[i]),
                                int((ratio > 1).sum()), ratio.numel()))
    return worst


def _entry_bound(k, terms, want, H_cols):
    """k u terms, or where tighter 1e-5 of the row's largest float64 entry"""
    row = want.abs().reshape(-1, H_cols).amax(1, keepdim=True).expand(-1, H_cols)
    return torch.minimum(k * U * terms.reshape(-1, H_cols), 1e-5 * row)


# ---------------------------------------------------------------------------------------------------------------------
# the loss

LOSS_SCALE = 1.0 / 256          # a power of two: loss_partial / scale is exact, the row's loss is seen as the kernel formed it
FILL = 60.0                     # a filler row's label logit over its others: exp(-60) vanishes beside 1 in both precisions


def _loss_case(Cn, shift, rem, use_map, seed, blocks=222):
    """A block of the kernel is 4 consecutive rows.  Row 4b is MEASURED (N(0, 3) + shift, a random label); rows 4b + 1
    .. 4b + 3 are fillers (label logit 60 above the others: s == 1 and m == z[label], a loss of exactly 0 in fp32 and in
    float64), so loss_partial[b] is row 4b's loss times the scale.  Every tenth block is fillers only.  n % 4 == rem.
    Logits and gradient are column blocks [0, C) of buffers C + 3 and C + 5 wide."""
    rng = np.random.default_rng(seed)
    n = 4 * (blocks - 1) + (rem if rem else 4)
    n_pad = n + 7
    ldl, ldgr = Cn + 3, Cn + 5
    n_nodes, n_lab = n + 50, n + 90
    ids = rng.permutation(n_nodes)[:n]
    rowmap = rng.permutation(n_lab)[:n_nodes] if use_map else None
    lab_rows = rowmap[ids] if use_map else ids
    labels = rng.integers(0, Cn, size=n_lab if use_map else n_nodes)
    zbuf = rng.standard_normal((n_pad + 1, ldl)).astype(np.float32)             # (the pad columns and rows: anything finite)
    z = (rng.standard_normal((n, Cn)) * 3 + shift).astype(np.float32)
    measured = np.zeros(n, dtype=bool)
    measured[0::4] = True
    measured[36::40] = False                                                  # every tenth block: fillers only
    fill = np.nonzero(~measured)[0]
    z[fill] = np.float32(shift)
    z[fill, labels[lab_rows[fill]]] = np.float32(shift + FILL)
    zbuf[:n, :Cn] = z
    return dict(C=Cn, n=n, n_pad=n_pad, ldl=ldl, ldgr=ldgr, ids=ids, rowmap=rowmap, labels=labels, zbuf=zbuf,
                measured=measured, lab_rows=lab_rows)


def _run_partial(mods, cs, labels=None, with_cols=True):
    aggr, L = mods
    Cn, n, n_pad = cs["C"], cs["n"], cs["n_pad"]
    blocks = (n_pad + 3) // 4
    zd = _dev(cs["zbuf"])
    grad = torch.full((n_pad + 2, cs["ldgr"]), SENT, device="cuda")
    lpart = _buf(blocks)
    cpart = _buf(blocks * Cn) if with_cols else None
    lab = _dev(cs["labels"] if labels is None else labels, torch.int64)
    ids, rm = _dev(cs["ids"], torch.int32), (_dev(cs["rowmap"], torch.int32) if cs["rowmap"] is not None else None)
    rc = L.csl_softmax_ce_partial_f32(_ptr(zd), cs["ldl"], n, n_pad, Cn, _ptr(ids), _ptr(rm), _ptr(lab), LOSS_SCALE,
                                      _ptr(grad), cs["ldgr"], _ptr(lpart), _ptr(cpart), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    # rows past n_pad and columns past C of the wider gradient buffer, the floats behind the partials
    assert bool((grad[n_pad:] == SENT).all()) and bool((grad[:, Cn:] == SENT).all())
    assert _tail_ok(lpart, blocks) and (cpart is None or _tail_ok(cpart, blocks * Cn))
    return grad[:n_pad, :Cn], lpart[:blocks], (cpart[:blocks * Cn].view(blocks, Cn) if with_cols else None)


def _run_whole(mods, cs, labels=None):
    aggr, L = mods
    Cn, n = cs["C"], cs["n"]
    zd = _dev(cs["zbuf"])
    grad = torch.full((n + 2, cs["ldgr"]), SENT, device="cuda")
    ns = int(L.csl_softmax_ce_scratch(n))
    scratch, loss = _buf(ns), _buf(1)
    lab = _dev(cs["labels"] if labels is None else labels, torch.int64)
    ids, rm = _dev(cs["ids"], torch.int32), (_dev(cs["rowmap"], torch.int32) if cs["rowmap"] is not None else None)
    rc = L.csl_softmax_ce_f32(_ptr(zd), cs["ldl"], n, Cn, _ptr(ids), _ptr(rm), _ptr(lab), LOSS_SCALE, _ptr(loss),
                              _ptr(grad), cs["ldgr"], _ptr(scratch), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((grad[n:] == SENT).all()) and bool((grad[:, Cn:] == SENT).all())
    assert _tail_ok(scratch, ns) and _tail_ok(loss, 1)
    return grad[:n, :Cn], loss[0]


def _row_loss_bound(want_rows, Cn):
    """1e-5 max(loss, 0.05) + C u, on the unscaled loss of a row"""
    return 1e-5 * want_rows.clamp_min(0.05) + Cn * U


LOSS_C = [1, 2, 3, 47, 63, 64, 65, 255, 256, 257, 4096]
LOSS_SHIFT = [0.0, 80.0, -80.0]


@pytest.mark.parametrize("shift", LOSS_SHIFT)
@pytest.mark.parametrize("Cn", LOSS_C)
def test_loss_row_by_row(mods, Cn, shift):
    k = LOSS_C.index(Cn) * 3 + LOSS_SHIFT.index(shift)
    cs = _loss_case(Cn, shift, rem=k % 4, use_map=k % 2 == 1, seed=1000 + k)
    n, n_pad, meas = cs["n"], cs["n_pad"], cs["measured"]
    with_cols = Cn <= 256                                      # (SM_CMAX: wider rows have no column sums)
    want_rows, want_g, want_cs = T.softmax_ce(cs["zbuf"], cs["ldl"], n, n_pad, Cn, cs["ids"], cs["rowmap"], cs["labels"],
                                              LOSS_SCALE)
    assert bool((want_rows[torch.from_numpy(~meas)] == 0).all())                 # the fillers: exactly 0 in float64
    grad, lpart, cpart = _run_partial(mods, cs, with_cols=with_cols)
    lp = lpart.cpu().double()
    nb = (n + 3) // 4
    meas_b = torch.from_numpy(meas[0::4])
    assert bool((lp[:nb][~meas_b] == 0).all()) and bool((lp[nb:] == 0).all())    # ... and in the kernel; padding blocks
    # a measured row's loss, unscaled (the scale is a power of two), against float64
    want_m = want_rows[0::4][meas_b] / LOSS_SCALE
    _within("loss rows", lp[:nb][meas_b] / LOSS_SCALE, want_m, _row_loss_bound(want_m, Cn),
            "loss rows C=%d shift=%g" % (Cn, shift))
    # gradient rows: 1e-4 of the tensor's largest entry; padding rows zero
    g = grad.cpu().double()
    _within("gradient", g, want_g, torch.full_like(want_g, 1e-4 * float(want_g.abs().max())),
            "gradient rows C=%d shift=%g" % (Cn, shift))
    assert bool((grad[n:] == 0).all())
    if with_cols:
        # a block's column sums are 4 stored gradient entries added in fp32: any order, 4 terms: 4 u sum |entries|
        blocks = (n_pad + 3) // 4
        gp = torch.zeros((4 * blocks, Cn), dtype=F64)
        gp[:n_pad] = g
        gp = gp.view(blocks, 4, Cn)
        _within("loss colsum", cpart, gp.sum(1), 4 * U * gp.abs().sum(1), "block column sums C=%d shift=%g" % (Cn, shift))
        # and their total is the bias gradient: 1e-4 of its largest entry
        tot = cpart.cpu().double().sum(0)
        assert float((tot - want_cs).abs().max()) <= 1e-4 * float(want_cs.abs().max())
    # the one-call form: the same gradient rows, and the summed loss: the rows' bounds added up, plus an fp32 sum of the
    # blocks in any order (blocks u sum |partials|)
    grad1, loss1 = _run_whole(mods, cs)
    assert torch.equal(grad1, grad[:n])
    want_sum = float(want_rows.sum())
    bound = float((_row_loss_bound(want_m, Cn) * LOSS_SCALE).sum()) + nb * U * want_sum
    _within("loss sum", loss1.reshape(1), torch.tensor([want_sum], dtype=F64), torch.tensor([bound], dtype=F64),
            "summed loss C=%d shift=%g" % (Cn, shift))


def test_loss_special_rows(mods):
    """-inf beside the label (finite loss, gradient exactly 0 there), -inf AT the label (loss +inf, as float64 gives),
    all logits equal (log C)"""
    Cn = 7
    cs = _loss_case(Cn, 0.0, rem=3, use_map=True, seed=77, blocks=12)
    z, lab_of = cs["zbuf"], cs["labels"][cs["lab_rows"]]
    z[0, :Cn] = -np.inf
    z[0, lab_of[0]] = 1.5                                          # only the label is finite: loss 0
    z[4, (lab_of[4] + 1) % Cn] = -np.inf
    z[4, (lab_of[4] + 3) % Cn] = -np.inf
    z[8, lab_of[8]] = -np.inf                                      # the label itself
    z[12, :Cn] = -3.25                                             # all equal
    z[16, :Cn] = 80.0
    n, n_pad = cs["n"], cs["n_pad"]
    want_rows, want_g, _ = T.softmax_ce(z, cs["ldl"], n, n_pad, Cn, cs["ids"], cs["rowmap"], cs["labels"], LOSS_SCALE)
    grad, lpart, _ = _run_partial(mods, cs)
    lp = lpart.cpu().double() / LOSS_SCALE
    want = want_rows[0::4] / LOSS_SCALE
    assert float(want[2]) == float("inf") and float(lp[2]) == float("inf")
    fin = torch.isfinite(want)
    assert int(fin.sum()) == want.numel() - 1
    _within("loss rows", lp[:want.numel()][fin], want[fin], _row_loss_bound(want[fin], Cn), "special rows")
    assert float(lp[0]) == 0.0 and abs(float(want[3]) - np.log(Cn)) < 1e-12
    g = grad.cpu().double()
    assert bool((g[0, np.arange(Cn) != lab_of[0]] == 0).all())
    assert float(g[4, (lab_of[4] + 1) % Cn]) == 0.0 and float(g[4, (lab_of[4] + 3) % Cn]) == 0.0
    _within("gradient", g, want_g, torch.full_like(want_g, 1e-4 * float(want_g.abs().max())), "special rows, gradient")
    _, loss1 = _run_whole(mods, cs)
    assert float(loss1) == float("inf")


@pytest.mark.parametrize("Cn,shift", [(1, 0.0), (3, 80.0), (64, 0.0), (255, -80.0), (300, 0.0)])
def test_loss_bad_labels(mods, Cn, shift):
    """A label of -1 or of C (interior rows only: the logits are a column block of a wider buffer, so the element the
    parent's kernel read for them is the test's own): NaN for the row's loss, its block's partial and the total, NaN for
    its gradient row; every other row, partial and block column sum bitwise what a run without the bad labels gives."""
    cs = _loss_case(Cn, shift, rem=2, use_map=Cn % 2 == 1, seed=500 + Cn, blocks=40)
    n, n_pad = cs["n"], cs["n_pad"]
    with_cols = Cn <= 256
    bad_rows = {8: -1, 20: Cn, 41: Cn, 62: -1, 100: Cn}           # measured rows (8, 20, 100) and fillers (41, 62)
    labels = cs["labels"].copy()
    for r, v in bad_rows.items():
        labels[cs["lab_rows"][r]] = v
    hit = np.isin(cs["lab_rows"], cs["lab_rows"][list(bad_rows)])  # (a label row may serve one row only: ids are a permutation)
    assert int(hit.sum()) == len(bad_rows)
    grad0, lp0, cp0 = _run_partial(mods, cs, with_cols=with_cols)
    grad, lp, cp = _run_partial(mods, cs, labels=labels, with_cols=with_cols)
    rows_bad = torch.from_numpy(np.concatenate([hit, np.zeros(n_pad - n, dtype=bool)]))
    blocks_bad = torch.zeros(lp.numel(), dtype=torch.bool)
    blocks_bad[[r // 4 for r in bad_rows]] = True
    assert bool(torch.isnan(grad.cpu()[rows_bad]).all()), "gradient rows of the bad labels are not NaN"
    assert bool(torch.isnan(lp.cpu()[blocks_bad]).all()), "loss partials of the bad labels' blocks are not NaN"
    assert torch.equal(grad.cpu()[~rows_bad], grad0.cpu()[~rows_bad])
    assert torch.equal(lp.cpu()[~blocks_bad], lp0.cpu()[~blocks_bad])
    if with_cols:
        assert bool(torch.isnan(cp.cpu()[blocks_bad]).all())
        assert torch.equal(cp.cpu()[~blocks_bad], cp0.cpu()[~blocks_bad])
    # the float64 statement says the same
    want_rows, want_g, want_cs = T.softmax_ce(cs["zbuf"], cs["ldl"], n, n_pad, Cn, cs["ids"], cs["rowmap"], labels, LOSS_SCALE)
    assert torch.equal(torch.isnan(want_rows), rows_bad[:n]) and torch.equal(torch.isnan(want_g).all(1), rows_bad)
    grad1, loss1 = _run_whole(mods, cs, labels=labels)
    assert bool(torch.isnan(loss1)) and bool(torch.isnan(grad1.cpu()[rows_bad[:n]]).all())
    assert torch.equal(grad1.cpu()[~rows_bad[:n]], grad0.cpu()[:n][~rows_bad[:n]])


# ---------------------------------------------------------------------------------------------------------------------
# Adam

ADAM_NUMEL = [0, 1, 3, 0, 1023, 1024, 1025, 2049, 4097, 0, 0, 1, 1025, 3, 4097, 1023, 0, 2049, 1024, 1, 3, 1025, 1023, 0]
ADAM_ZERO_GRAD = 5              # this tensor (1,024 elements) has zero gradients on zero moments in every case
B1, B2, EPS = 0.9, 0.999, 1e-8


def _adam_state(rng, numel, step):
    """gradient magnitudes 1e-12 .. 1e12 (every seventh gradient 0), parameters 1e-6 .. 1e3, moments of the gradients'
    size (zero at step 1)"""
    mag = 10.0 ** rng.uniform(-12, 12, size=numel)
    g = mag * rng.uniform(0.5, 1.0, size=numel) * rng.choice([-1.0, 1.0], size=numel)
    g[::7] = 0.0
    p = 10.0 ** rng.uniform(-6, 3, size=numel) * rng.choice([-1.0, 1.0], size=numel)
    if step == 1:
        m, v = np.zeros(numel), np.zeros(numel)
    else:
        m = mag * rng.standard_normal(numel) * 0.5
        v = (mag * rng.uniform(0.3, 1.5, size=numel)) ** 2
    return [a.astype(np.float32) for a in (p, g, m, v)]


def _adam_call(mods, count, bufs, numel, lr, step, null_empty=True):
    aggr, L = mods
    arr = lambda k: (C.c_void_p * count)(*[(0 if (numel[t] == 0 and null_empty and t % 2 == 0) else bufs[t][k].data_ptr())
                                           for t in range(count)])
    return L.csl_adam_f32(count, arr(0), arr(1), arr(2), arr(3), (C.c_int64 * count)(*numel), lr, B1, B2, EPS, step,
                          aggr._stream())


@pytest.mark.parametrize("lr", [1e-3, 3e-3, 1.0])
@pytest.mark.parametrize("step", [1, 2, 10, 1000, 10 ** 6, 10 ** 9])
def test_adam_one_step(mods, step, lr):
    rng = np.random.default_rng(step % 9973 + int(lr * 1000))
    host = [_adam_state(rng, k, step) for k in ADAM_NUMEL]
    for a in host[ADAM_ZERO_GRAD][1:]:
        a[:] = 0.0
    bufs = []
    for t, k in enumerate(ADAM_NUMEL):
        four = []
        for a in host[t]:
            b = _buf(k)                                            # sentinels past every tensor's end
            b[:k] = torch.from_numpy(a).cuda()
            four.append(b)
        bufs.append(four)
    assert _adam_call(mods, 24, bufs, ADAM_NUMEL, lr, step) == 0
    torch.cuda.synchronize()
    for t, k in enumerate(ADAM_NUMEL):
        p0, g0, m0, v0 = host[t]
        what = "tensor %d (%d elements) step %d lr %g" % (t, k, step, lr)
        for b in bufs[t]:
            assert _tail_ok(b, k), what
        assert torch.equal(bufs[t][1][:k].cpu(), torch.from_numpy(g0))            # the gradient is read only
        if k == 0:
            continue
        p1, m1, v1 = (bufs[t][j][:k].cpu() for j in (0, 2, 3))
        p64, m64, v64, upd, m_abs, v_abs = T.adam_step(p0, g0, m0, v0, lr, B1, B2, EPS, step)
        _within("adam m", m1, m64, 4 * U * m_abs, what + ": m")       # two products and a sum; bound as the issue states it
        _within("adam v", v1, v64, 4 * U * v_abs, what + ": v")       # three products and a sum
        upd_k = T.adam_update(m1, v1, lr, B1, B2, EPS, step)                      # from the kernel's own moments
        pk = torch.from_numpy(p0).double() - upd_k
        _within("adam p", p1, pk, 2 * U * pk.abs() + 16 * U * upd_k.abs(), what + ": p")
        if t == ADAM_ZERO_GRAD:                                                   # zero gradients on zero moments
            assert torch.equal(p1, torch.from_numpy(p0)) and not bool(m1.any()) and not bool(v1.any())


def test_adam_refusals(mods):
    numel = [4] * 25
    bufs = [[torch.zeros(4, device="cuda") for _ in range(4)] for _ in range(25)]
    before = [[b.clone() for b in four] for four in bufs]
    assert _adam_call(mods, 25, bufs, numel, 1e-3, 1) == E_INVALID           # more than 24 tensors
    assert _adam_call(mods, 24, bufs, numel[:24], 1e-3, 0) == E_INVALID      # steps count from 1
    assert _adam_call(mods, 3, bufs, [4, -1, 4], 1e-3, 1) == E_INVALID       # a negative size
    torch.cuda.synchronize()
    for four, ref in zip(bufs, before):
        for b, r in zip(four, ref):
            assert torch.equal(b, r)


def test_adam_flat_gradients_equal_separate_ones(mods):
    """aggr.Adam.step(flat_grads=...): the gradients back to back in one buffer, the second tensor 12 bytes off a 16-byte
    boundary, must give bitwise what step() gives on the same gradients"""
    aggr, L = mods
    torch.manual_seed(3)
    sizes = [(3,), (41, 25), (64,)]
    pa = [torch.randn(s, device="cuda") for s in sizes]
    pb = [p.clone() for p in pa]
    oa, ob = aggr.Adam(pa, lr=3e-3), aggr.Adam(pb, lr=3e-3)
    for _ in range(3):
        flat = torch.randn(sum(p.numel() for p in pa), device="cuda")
        assert (flat.data_ptr() + 4 * pa[0].numel()) % 16 == 12
        o = 0
        for p in pb:
            p.grad = flat[o:o + p.numel()].clone().view_as(p)
            o += p.numel()
        oa.step(flat_grads=flat)
        ob.step()
    torch.cuda.synchronize()
    for a, b, sa, sb in zip(pa, pb, oa.state, ob.state):
        assert torch.equal(a, b) and torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
        assert bool(sa[1].any())


# ---------------------------------------------------------------------------------------------------------------------
# the attention row kernels

# (D, H): a partial chunk, exactly one chunk and one head past it for every lane-group class
WIDTHS = [(4, 1), (4, 64), (4, 65), (8, 3), (12, 1), (12, 21), (12, 22), (20, 12), (20, 13), (32, 8), (68, 2), (68, 3),
          (68, 4), (68, 7), (192, 1), (192, 2), (252, 1), (252, 2), (256, 1), (256, 3)]


def _logits_bwd(mods, z, al, ar, g_el, g_er, n, H, D, prefill, accumulate):
    """csl_gat_logits_bwd_acc_f32 on a g_z prefilled with `prefill` (a tensor, or a float), a scratch buffer of exactly
    the reported size; returns (g_z, g_attn_l, g_attn_r), sentinels checked"""
    aggr, L = mods
    Cw = H * D
    gz = _buf(n * Cw)
    if torch.is_tensor(prefill):
        gz[:n * Cw] = prefill.reshape(-1)
    else:
        gz[:n * Cw] = prefill
    before = gz.clone()
    ns = int(L.csl_gat_logits_bwd_scratch(n, H, D))
    scratch, gal, gar = _buf(ns), _buf(Cw), _buf(Cw)
    rc = L.csl_gat_logits_bwd_acc_f32(_ptr(z), _ptr(al), _ptr(ar), _ptr(g_el), _ptr(g_er), n, H, D, _ptr(gz), accumulate,
                                      _ptr(gal), _ptr(gar), _ptr(scratch), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _tail_ok(gz, n * Cw) and _tail_ok(scratch, ns) and _tail_ok(gal, Cw) and _tail_ok(gar, Cw)
    if n == 0:
        assert torch.equal(gz, before)
    return gz[:n * Cw].view(n, Cw), gal[:Cw], gar[:Cw]


def _check_logits(mods, rng, n, H, D, what):
    aggr, L = mods
    Cw = H * D
    z = rng.standard_normal((n, Cw)).astype(np.float32)
    al, ar = (rng.standard_normal((H, D)) / D ** 0.5).astype(np.float32), (rng.standard_normal((H, D)) / D ** 0.5).astype(np.float32)
    g_el, g_er = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((n, H)).astype(np.float32)
    zd, ald, ard, geld, gerd = (_dev(a) for a in (z, al, ar, g_el, g_er))
    ab = lambda a: np.abs(a)
    if n > 0:
        el, er = _buf(n * H), _buf(n * H)
        assert L.csl_gat_logits_fwd_f32(_ptr(zd), _ptr(ald), _ptr(ard), n, H, D, _ptr(el), _ptr(er), aggr._stream()) == 0
        torch.cuda.synchronize()
        assert _tail_ok(el, n * H) and _tail_ok(er, n * H)
        want_l, want_r = T.logits_fwd(z, al, ar, H, D)
        abs_l, abs_r = T.logits_fwd(ab(z), ab(al), ab(ar), H, D)
        # a head's logit: D products added in any order: D u sum |terms|
        _within("logits", el[:n * H], want_l, D * U * abs_l, what + ": el")
        _within("logits", er[:n * H], want_r, D * U * abs_r, what + ": er")
    want_gz, want_gl, want_gr = T.logits_bwd(z, al, ar, g_el, g_er, H, D)
    abs_gz, abs_gl, abs_gr = T.logits_bwd(ab(z), ab(al), ab(ar), ab(g_el), ab(g_er), H, D)
    # accumulate = 0 writes: whatever g_z held (NaN) must vanish
    gz0, gl0, gr0 = _logits_bwd(mods, zd, ald, ard, geld, gerd, n, H, D, float("nan"), 0)
    if n > 0:
        # an entry of g_z: two products and a sum, k = 3
        _within("logits", gz0, want_gz, _entry_bound(3, abs_gz, want_gz, Cw), what + ": g_z")
    # the attention vectors' gradients: n products added in any order: n u sum |terms| (n = 0: zeros)
    _within("logits", gl0, want_gl, n * U * abs_gl, what + ": g_attn_l")
    _within("logits", gr0, want_gr, n * U * abs_gr, what + ": g_attn_r")
    # accumulate = 1: the prefill plus what accumulate = 0 writes, one fp32 addition; the sums are the same sums
    pre = torch.from_numpy(rng.standard_normal((n, Cw)).astype(np.float32)).cuda()
    gz1, gl1, gr1 = _logits_bwd(mods, zd, ald, ard, geld, gerd, n, H, D, pre, 1)
    assert torch.equal(gz1, pre + gz0), what + ": accumulate"
    assert torch.equal(gl1, gl0) and torch.equal(gr1, gr0)
    if n > 0:
        want_acc, _, _ = T.logits_bwd(z, al, ar, g_el, g_er, H, D, g_z_before=pre.cpu())
        _within("logits", gz1, want_acc, _entry_bound(4, abs_gz + pre.cpu().double().abs(), want_acc, Cw), what + ": g_z accumulated")


def _finish_inputs(rng, n, H, D):
    """(n, s, bias, g) of the epilogue: rows r % 16 == 3 have a head sum of 0 with n = 0 (a row without edges), rows
    r % 16 == 11 a head sum of 1e-35, below the floor of 1e-30, with n of that size; bias[0] = 0 (an output of exactly 0
    on the empty rows), bias[1] = -120 (an input below -104: expm1f gives -1 exactly), bias[2] = -0.5"""
    Cw = H * D
    s = rng.uniform(0.5, 9.0, size=(n, H)).astype(np.float32)
    nn = (rng.standard_normal((n, Cw)) * 3).astype(np.float32)
    rows = np.arange(n)
    s[rows % 16 == 3] = 0.0
    nn[rows % 16 == 3] = 0.0
    s[rows % 16 == 11] = 1e-35
    nn[rows % 16 == 11] = (rng.standard_normal((int((rows % 16 == 11).sum()), Cw)) * 1e-30).astype(np.float32)
    bias = rng.standard_normal(Cw).astype(np.float32)
    bias[:3] = (0.0, -120.0, -0.5)
    return nn, s, bias


def _check_finish(mods, rng, n, H, D, use_elu, what):
    aggr, L = mods
    Cw, ldg = H * D, H * D + 4
    nn, s, bias = _finish_inputs(rng, n, H, D)
    nd, sd, bd = _dev(nn), _dev(s), _dev(bias)
    out = _buf(n * Cw)
    assert L.csl_gat_finish_fwd_f32(_ptr(nd), _ptr(sd), _ptr(bd), n, H, D, use_elu, _ptr(out), aggr._stream()) == 0
    torch.cuda.synchronize()
    assert _tail_ok(out, n * Cw)
    o32 = out[:n * Cw].view(n, Cw).cpu()
    if n > 0:
        want = T.finish_fwd(nn, s, bias, H, D, use_elu)
        sf = torch.from_numpy(s).double().clamp_min(T.S_FLOOR).repeat_interleave(D, 1)
        terms = torch.from_numpy(nn).double().abs() / sf + torch.from_numpy(bias).double().abs()
        # the reciprocal, its product, the sum, and expm1f to 1 ulp = 2 u of a result no larger than its argument: k = 5
        # (ELU is 1-Lipschitz, so the argument's error passes at most unchanged); k = 3 without the ELU
        _within("finish", o32, want, _entry_bound(5 if use_elu else 3, terms, want, Cw), what + ": out")
        empty = torch.from_numpy(np.arange(n) % 16 == 3)
        if bool(empty.any()):                                   # a row without edges: act(bias); 0 and -1 exactly
            assert bool((o32[empty][:, 0] == 0).all())
            assert bool((o32[empty][:, 1] == (-1.0 if use_elu else -120.0)).all())
    # backward, from the kernel's own output (with exact zeros and, under ELU, exact -1s), g with a leading dimension
    g = rng.standard_normal((n, Cw)).astype(np.float32)
    gb = torch.full((n, ldg), SENT, device="cuda")
    gb[:, :Cw] = torch.from_numpy(g).cuda()
    ns = int(L.csl_gat_finish_bwd_scratch(n, H, D))
    g_n, g_s, g_b, scratch = _buf(n * Cw), _buf(n * H), _buf(Cw), _buf(ns)
    rc = L.csl_gat_finish_bwd_f32(_ptr(gb), ldg, _ptr(out), _ptr(nd), _ptr(sd), n, H, D, use_elu, _ptr(g_n), _ptr(g_s),
                                  _ptr(g_b), _ptr(scratch), aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _tail_ok(g_n, n * Cw) and _tail_ok(g_s, n * H) and _tail_ok(g_b, Cw) and _tail_ok(scratch, ns)
    want_gn, want_gs, want_gb, p = T.finish_bwd(g, o32, nn, s, H, D, use_elu)
    if n > 0:
        # g_n: out + 1, its product with g, the reciprocal, its product: k = 4, all relative to the entry itself
        _within("finish", g_n[:n * Cw], want_gn, 4 * U * want_gn.abs(), what + ": g_n")
        # g_s: D terms in any order (D u), every term through the 4 roundings of g_n, the sum through the reciprocal
        # once more and its product: D + 6
        sf = torch.from_numpy(s).double().clamp_min(T.S_FLOOR)
        abs_gs = (want_gn.abs() * torch.from_numpy(nn).double().abs()).view(n, H, D).sum(-1) / sf
        _within("finish", g_s[:n * H], want_gs, (D + 6) * U * abs_gs, what + ": g_s")
        assert bool(torch.isfinite(g_s[:n * H]).all())
        if use_elu:                                            # the slope is 1 at out == 0 and 0 at out == -1, exactly
            gn32, zero, minus1 = g_n[:n * Cw].view(n, Cw).cpu(), o32 == 0, o32 == -1
            assert bool((gn32[minus1] == 0).all()) and bool(minus1[:, 1].all())
            inv = (1.0 / torch.from_numpy(s).clamp_min(1e-30)).repeat_interleave(D, 1)
            assert torch.equal(gn32[zero], (torch.from_numpy(g) * inv)[zero])
    # the bias gradient: n terms in any order, each through out + 1 and its product: n + 2 (n = 0: zeros)
    _within("finish", g_b[:Cw], want_gb, (n + 2) * U * p.abs().sum(0), what + ": g_bias")


@pytest.mark.parametrize("n", [1, 5, 333])
@pytest.mark.parametrize("D,H", WIDTHS)
def test_attention_rows_at_every_lane_group(mods, D, H, n):
    rng = np.random.default_rng(D * 1000 + H * 10 + n)
    what = "D=%d H=%d n=%d" % (D, H, n)
    _check_logits(mods, rng, n, H, D, what)
    for use_elu in (1, 0):
        _check_finish(mods, rng, n, H, D, use_elu, what + " elu=%d" % use_elu)


@pytest.mark.parametrize("n", [0, 4096, 4097, 131072, 131073, 262144, 262145])
@pytest.mark.parametrize("D", [4, 8])
def test_attention_rows_per_block_edges(mods, D, n):
    """gat_finish_rows(n): 4 rows per block up to 4,096 rows, 8 from 4,097, 128 at 131,072, rb_rows(n) = 128 from
    131,073, 256 from 262,145; n = 0: the second stages run over zero blocks, the gradients are zeros, nothing else is
    touched (the scratch buffers have exactly the reported size, here none)"""
    rng = np.random.default_rng(n + D)
    what = "D=%d H=1 n=%d" % (D, n)
    _check_logits(mods, rng, n, 1, D, what)
    _check_finish(mods, rng, n, 1, D, 1, what)


# ---------------------------------------------------------------------------------------------------------------------
# bias + ELU and its backward

def _elu_rows(Cw):
    """row counts around the BLK / (C / 4) rows a block of k_elu_bwd_colsum takes at once, and beyond one block of 8 rows"""
    at_once = 256 // (Cw // 4)
    return sorted({1, 7, 9, at_once - 1, at_once, at_once + 1, 2 * at_once + 1, 1029})


@pytest.mark.parametrize("use_elu", [1, 0])
@pytest.mark.parametrize("Cw", [4, 12, 60, 252, 256])
def test_bias_elu_and_its_backward(mods, Cw, use_elu):
    aggr, L = mods
    rng = np.random.default_rng(Cw + use_elu)
    for n in _elu_rows(Cw):
        what = "C=%d n=%d elu=%d" % (Cw, n, use_elu)
        ldy, ldg, ldo = Cw + 4, Cw + 8, Cw + 12
        y = (rng.standard_normal((n, Cw)) * 3).astype(np.float32)
        bias = rng.standard_normal(Cw).astype(np.float32)
        y[0, :3] = (0.0, -110.0, 0.25)
        bias[:3] = (0.0, -10.0, -0.25)                              # row 0: an input of 0, one below -104, one that cancels to 0
        yb = torch.full((n + 1, ldy), SENT, device="cuda")
        yb[:n, :Cw] = torch.from_numpy(y).cuda()
        assert L.csl_bias_elu_f32(_ptr(yb), ldy, _ptr(_dev(bias)), n, Cw, use_elu, aggr._stream()) == 0
        torch.cuda.synchronize()
        assert bool((yb[n:] == SENT).all()) and bool((yb[:, Cw:] == SENT).all())
        want = T.bias_elu(y, bias, use_elu)
        terms = torch.from_numpy(y).double().abs() + torch.from_numpy(bias).double().abs()
        # the sum, and expm1f to 1 ulp = 2 u: k = 3 (k = 1 without the ELU)
        y32 = yb[:n, :Cw].cpu()
        _within("elu kernels", y32, want, _entry_bound(3 if use_elu else 1, terms, want, Cw), what + ": bias_elu")
        assert float(y32[0, 0]) == 0.0 and float(y32[0, 2]) == 0.0 and float(y32[0, 1]) == (-1.0 if use_elu else -120.0)
        # backward from that output
        g = rng.standard_normal((n, Cw)).astype(np.float32)
        gb = torch.full((n, ldg), SENT, device="cuda")
        gb[:, :Cw] = torch.from_numpy(g).cuda()
        ob = torch.full((n + 1, ldo), SENT, device="cuda")
        ns = int(L.csl_elu_bwd_colsum_scratch(n, Cw))
        cs, scratch = _buf(Cw), _buf(ns)
        rc = L.csl_elu_bwd_colsum_f32(_ptr(gb), ldg, _ptr(yb), ldy, n, Cw, use_elu, _ptr(ob), ldo, _ptr(cs), _ptr(scratch),
                                      aggr._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((ob[n:] == SENT).all()) and bool((ob[:, Cw:] == SENT).all()) and _tail_ok(cs, Cw) and _tail_ok(scratch, ns)
        want_o, want_cs = T.elu_bwd_colsum(g, y32, use_elu)
        # y + 1 and its product with g: k = 2, relative to the entry itself (the mask of an exact 0 or -1 is exact)
        o32 = ob[:n, :Cw].cpu()
        _within("elu kernels", o32, want_o, 2 * U * want_o.abs(), what + ": elu_bwd")
        assert float(o32[0, 0]) == float(g[0, 0]) and float(o32[0, 1]) == (0.0 if use_elu else float(g[0, 1]))
        # the column sums: n terms in any order, each through those two roundings: n + 2
        _within("elu kernels", cs[:Cw], want_cs, (n + 2) * U * want_o.abs().sum(0), what + ": column sums")


def test_elu_backward_of_no_rows_zeroes_the_column_sums(mods):
    aggr, L = mods
    for Cw in (4, 252, 256):
        cs = _buf(Cw)
        assert L.csl_elu_bwd_colsum_f32(None, Cw, None, Cw, 0, Cw, 1, None, Cw, _ptr(cs), None, aggr._stream()) == 0
        assert L.csl_bias_elu_f32(None, Cw, None, 0, Cw, 1, aggr._stream()) == 0
        torch.cuda.synchronize()
        assert not bool(cs[:Cw].any()) and _tail_ok(cs, Cw)
    # rows wider than 256 columns are refused
    b = torch.zeros((4 * 272,), device="cuda")
    assert L.csl_elu_bwd_colsum_f32(_ptr(b), 260, _ptr(b), 260, 4, 260, 1, _ptr(b), 260, _ptr(b), _ptr(b), aggr._stream()) == E_INVALID
    torch.cuda.synchronize()
    assert not bool(b.any())


# ---------------------------------------------------------------------------------------------------------------------
# refusals: the return code only (every one of these is refused before any launch: a launch with D > 256 would have no live
# lane, lpc = 0, and a column loop that never ends)

@pytest.mark.parametrize("H,D,off", [(1, 0, 0), (1, 2, 0), (1, 6, 0), (1, 260, 0), (0, 8, 0), (2, 8, 1)])
def test_attention_row_kernels_refuse(mods, H, D, off):
    """D in {0, 2, 6, 260}, H = 0, and (off = 1) a pointer 4 bytes off 16-byte alignment"""
    aggr, L = mods
    n = 3
    big = torch.zeros((8192,), device="cuda")
    st = aggr._stream()
    a, m = _ptr(big), _ptr(big, off)               # an aligned pointer and the one under test
    ldg = max(16, H * D)                           # (itself acceptable: the width or the pointer is what is refused)
    assert L.csl_gat_logits_fwd_f32(m, a, a, n, H, D, a, a, st) == E_INVALID
    assert L.csl_gat_logits_bwd_acc_f32(m, a, a, a, a, n, H, D, a, 0, a, a, a, st) == E_INVALID
    assert L.csl_gat_logits_bwd_f32(m, a, a, a, a, n, H, D, a, a, a, a, st) == E_INVALID
    assert L.csl_gat_finish_fwd_f32(m, a, a, n, H, D, 1, a, st) == E_INVALID
    assert L.csl_gat_finish_bwd_f32(a, ldg, a, m, a, n, H, D, 1, a, a, a, a, st) == E_INVALID
    if off:                                        # each aligned operand in turn
        assert L.csl_gat_logits_fwd_f32(a, m, a, n, H, D, a, a, st) == E_INVALID
        assert L.csl_gat_logits_fwd_f32(a, a, m, n, H, D, a, a, st) == E_INVALID
        assert L.csl_gat_logits_bwd_acc_f32(a, a, a, a, a, n, H, D, m, 0, a, a, a, st) == E_INVALID
        assert L.csl_gat_logits_bwd_acc_f32(a, a, a, a, a, n, H, D, a, 0, a, a, m, st) == E_INVALID
        assert L.csl_gat_finish_fwd_f32(a, a, m, n, H, D, 1, a, st) == E_INVALID
        assert L.csl_gat_finish_fwd_f32(a, a, a, n, H, D, 1, m, st) == E_INVALID
        assert L.csl_gat_finish_bwd_f32(m, ldg, a, a, a, n, H, D, 1, a, a, a, a, st) == E_INVALID
        assert L.csl_gat_finish_bwd_f32(a, ldg, m, a, a, n, H, D, 1, a, a, a, a, st) == E_INVALID
        assert L.csl_gat_finish_bwd_f32(a, ldg, a, a, a, n, H, D, 1, m, a, a, a, st) == E_INVALID
        assert L.csl_gat_finish_bwd_f32(a, ldg, a, a, a, n, H, D, 1, a, a, a, m, st) == E_INVALID
        assert L.csl_bias_elu_f32(m, 16, a, n, 16, 1, st) == E_INVALID
        assert L.csl_bias_elu_f32(a, 16, m, n, 16, 1, st) == E_INVALID
        assert L.csl_elu_bwd_colsum_f32(m, 16, a, 16, n, 16, 1, a, 16, a, a, st) == E_INVALID
        assert L.csl_elu_bwd_colsum_f32(a, 16, m, 16, n, 16, 1, a, 16, a, a, st) == E_INVALID
        assert L.csl_elu_bwd_colsum_f32(a, 16, a, 16, n, 16, 1, m, 16, a, a, st) == E_INVALID
        assert L.csl_elu_bwd_colsum_f32(a, 16, a, 16, n, 16, 1, a, 16, a, m, st) == E_INVALID
    torch.cuda.synchronize()
    assert not bool(big.any())
