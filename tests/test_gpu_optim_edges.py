"""csl_adamw_f32 (include/cslicer_optim.h: weight decay, global-norm clipping, the non-finite guard) through the C ABI against
the float64 restatement in tests/optim_ref.py, and bitwise against csl_adam_f32 where the two must be one.

What decides how the kernels run, and what is therefore varied here:
  * k_adamw: k_adam's layout, ADAM_CHUNK = 1,024 elements per block, up to 24 tensors back to back, empty ones among them
    (the sizes are test_gpu_tail_edges.ADAM_NUMEL, copied); the per-tensor decay (0 or not), its two forms, clipping or not;
  * k_grad_sqsum: min(chunks, NORM_BLOCKS = 256) blocks, block b takes chunks b, b + 256, ...; one float64 partial per
    block, which every update block sums again: 1, 2, 255, 256, 257 and 513 chunks.

Tolerances (u = 2^-24; derived, none fitted; a ratio above 1 is a failure).  The update is test_gpu_tail_edges' Adam
bound with the roundings in front of it added.  g2 = g c (+ wd p, coupled) goes through k_g fp32 roundings: 1 for g c when
c != 1, 2 more for the product wd p and the sum (0 for the decoupled form and for wd = 0); with g2_abs = |g c| + |wd p|,
|g2' - g2| <= k_g u g2_abs.  Then
  * m' = b1 m + (1 - b1) g2: the 4 u of the Adam test on the terms' magnitudes, plus (1 - b1) times the error of g2:
        |m' - m64| <= (4 + k_g) u (|b1 m| + (1 - b1) g2_abs);
  * v' = b2 v + (1 - b2) g2^2: g2'^2 - g2^2 = (g2' - g2)(g2' + g2) <= 2 k_g u g2_abs^2:
        |v' - v64| <= (4 + 2 k_g) u (b2 v + (1 - b2) g2_abs^2);
  * p' = p_in - update with the update evaluated in float64 from the kernel's own stored m', v' (as the Adam test does, so
    that a cancellation in the moments stays out of this bound): 2 u |p64| + 16 u |update|; decoupled with wd > 0, p_in =
    p d is one more product, d being the float32 the entry point itself rounds 1 - lr wd to: + u |p d|.
  A fused multiply-add in place of a product and a sum drops a rounding and stays inside these.  They are relative
  bounds and hold while nothing underflows: where a step clips, gradients are 1e-3 .. 1e3 and c >= 1e-6, so that
  (1 - b2) g2^2 >= 1e-21; parameters are 1e-6 .. 1e3 and decays >= 5e-4.  The expected c is formed from the float64 norm;
  the device's own float64 sum differs from it by N 2^-53 relatively, 1e-9 of the spacing of float32, so the two round to
  the same float32 c.
  * the norm: the float64 sum of N squares in any order and the square root, (N + 2) 2^-53, and the rounding of the
    result to float32, u:  |grad_norm - n64| <= (u + (N + 2) 2^-53) n64.

Largest error / bound seen on an MI355X, per group (the tests print them to six digits: pytest -s):
    adamw m 0.434    adamw v 0.651    adamw p 0.649    the norm 0.849 (1e20 gradients; 0.805 at 1e-30, 0 for all-zero ones)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
import tail_ref as T

pytestmark = pytest.mark.gpu

E_INVALID = -1
U = 2.0 ** -24
SENT = -777.0
F64 = torch.float64
WORST = {}
ADAM_CHUNK, NORM_BLOCKS = 1024, 256             # csrc/adam_dev.h, csrc/optim.hip
# tests/test_gpu_tail_edges.ADAM_NUMEL (a copy)
ADAM_NUMEL = [0, 1, 3, 0, 1023, 1024, 1025, 2049, 4097, 0, 0, 1, 1025, 3, 4097, 1023, 0, 2049, 1024, 1, 3, 1025, 1023, 0]
FIRST, LAST = 1, 22                             # the first and the last tensor that are not empty
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 3e-3
DECAY = (0.0, 0.1, 5e-4, 0.0, 0.01)             # tensor t decays by DECAY[t % 5]: the sizes above meet 0 and positive ones


@pytest.fixture(scope="module")
def mods():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr, aggr._lib()


def _within(group, got, want, bound, what):
    """|got - want| <= bound entry by entry; notes and prints the group's largest error / bound"""
    got = got.detach().cpu().to(F64).reshape(-1)
    want, bound = want.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == want.shape == bound.shape, what
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
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


def _state(rng, numel, step, lo, hi):
    """gradient magnitudes 10^lo .. 10^hi (every seventh gradient 0), parameters 1e-6 .. 1e3, moments of the gradients'
    size (zero at step 1): test_gpu_tail_edges._adam_state with the gradients' range a parameter"""
    mag = 10.0 ** rng.uniform(lo, hi, size=numel)
    g = mag * rng.uniform(0.5, 1.0, size=numel) * rng.choice([-1.0, 1.0], size=numel)
    g[::7] = 0.0
    p = 10.0 ** rng.uniform(-6, 3, size=numel) * rng.choice([-1.0, 1.0], size=numel)
    if step == 1:
        m, v = np.zeros(numel), np.zeros(numel)
    else:
        m = mag * rng.standard_normal(numel) * 0.5
        v = (mag * rng.uniform(0.3, 1.5, size=numel)) ** 2
    return [a.astype(np.float32) for a in (p, g, m, v)]


class Call(object):
    """device copies of the tensors (sentinels behind each), a scratch buffer of exactly the reported size with sentinels
    behind it, the norm and the counter between sentinels; run() is one csl_adamw_f32 call"""

    def __init__(self, mods, host, numel):
        self.aggr, self.L = mods
        self.numel, self.count = list(numel), len(numel)
        self.bufs = []
        for four, k in zip(host, numel):
            row = []
            for a in four:
                b = torch.full((k + 8,), SENT, device="cuda")
                b[:k] = torch.from_numpy(a).cuda()
                row.append(b)
            self.bufs.append(row)
        self.n64 = (C.c_int64 * self.count)(*numel)
        self.scratch_bytes = int(self.L.csl_adamw_scratch(self.count, self.n64))
        chunks = sum((k + ADAM_CHUNK - 1) // ADAM_CHUNK for k in numel)
        assert self.scratch_bytes == 8 * min(chunks, NORM_BLOCKS)
        self.scratch = torch.full((self.scratch_bytes // 8 + 4,), SENT, dtype=F64, device="cuda")
        self.gn = torch.full((3,), SENT, device="cuda")
        self.sk = torch.full((3,), 7, dtype=torch.int32, device="cuda")

    def run(self, wd, decoupled, max_norm, step, lr=LR):
        arr = lambda k: (C.c_void_p * self.count)(*[(0 if (self.numel[t] == 0 and t % 2 == 0) else self.bufs[t][k].data_ptr())
                                                   for t in range(self.count)])       # noqa: E731
        w = None if wd is None else (C.c_float * self.count)(*wd)
        rc = self.L.csl_adamw_f32(self.count, arr(0), arr(1), arr(2), arr(3), self.n64, w, int(decoupled), max_norm, lr, B1,
                                  B2, EPS, step, C.c_void_p(self.gn.data_ptr() + 4), C.c_void_p(self.sk.data_ptr() + 4),
                                  C.c_void_p(self.scratch.data_ptr()), self.aggr._stream())
        torch.cuda.synchronize()
        return rc

    def tensors(self, t):
        """(p, m, v) of tensor t on the host"""
        return [self.bufs[t][j][:self.numel[t]].cpu() for j in (0, 2, 3)]

    def norm(self):
        return float(self.gn[1])

    def skipped(self):
        return int(self.sk[1]) - 7

    def untouched_around(self, host):
        """sentinels behind every tensor, the scratch, the norm and the counter; the gradients read only"""
        for t, k in enumerate(self.numel):
            for b in self.bufs[t]:
                assert bool((b[k:] == SENT).all()), t
            assert torch.equal(self.bufs[t][1][:k].cpu().view(torch.int32), torch.from_numpy(host[t][1]).view(torch.int32)), t
        assert bool((self.scratch[self.scratch_bytes // 8:] == SENT).all())
        assert float(self.gn[0]) == SENT and float(self.gn[2]) == SENT and int(self.sk[0]) == 7 and int(self.sk[2]) == 7


def _norm_bound(n64, N):
    return (U + (N + 2) * 2.0 ** -53) * n64


def _check_step(call, host, wd, decoupled, max_norm, step, what, lr=LR):
    """every tensor of `call` after one step against optim_ref, within the module docstring's bounds"""
    n64 = R.grad_norm([four[1] for four in host])
    c = R.clip_coef(n64, max_norm)
    if max_norm > 0:
        N = sum(call.numel)
        assert abs(call.norm() - n64) <= _norm_bound(n64, N), (what, call.norm(), n64)
    else:
        assert call.norm() == SENT                        # no clipping: the norm is not touched
    assert call.skipped() == 0
    call.untouched_around(host)
    for t, k in enumerate(call.numel):
        if k == 0:
            continue
        p0, g0, m0, v0 = host[t]
        w = 0.0 if wd is None else wd[t]
        st = R.adamw_step(p0, g0, m0, v0, c, w, decoupled, lr, B1, B2, EPS, step)
        kg = st.g2_roundings
        assert kg == (c != 1.0) + 2 * (w > 0 and not decoupled)
        p1, m1, v1 = call.tensors(t)
        tag = "%s: tensor %d (%d elements, decay %g)" % (what, t, k, w)
        _within("adamw m", m1, st.m, (4 + kg) * U * st.m_abs, tag + ": m")
        _within("adamw v", v1, st.v, (4 + 2 * kg) * U * st.v_abs, tag + ": v")
        upd_k = T.adam_update(m1, v1, lr, B1, B2, EPS, step)                 # from the kernel's own moments
        pk = st.p_in - upd_k
        extra = U * st.p_in.abs() if (w > 0 and decoupled) else torch.zeros_like(pk)
        _within("adamw p", p1, pk, 2 * U * pk.abs() + 16 * U * upd_k.abs() + extra, tag + ": p")
    return n64, c


def _hosts(seed, numel, step, lo=-3, hi=3):
    rng = np.random.default_rng(seed)
    return [_state(rng, k, step, lo, hi) for k in numel]


def _next_f32_at_or_above(x):
    f = np.float32(x)
    return float(f if float(f) >= x else np.nextafter(f, np.float32(np.inf)))


CLIPS = ["far above", "just above", "at", "below", "inf", "off"]


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("decoupled", [True, False])
def test_one_step_over_24_tensors(mods, decoupled, step, clip):
    host = _hosts(step + 17 * CLIPS.index(clip) + decoupled, ADAM_NUMEL, step)
    n64 = R.grad_norm([four[1] for four in host])
    max_norm = {"far above": n64 * 1e-6, "just above": n64 * (1 - 1e-5), "at": _next_f32_at_or_above(n64 + 1e-6),
                "below": n64 * 1.5, "inf": float("inf"), "off": 0.0}[clip]
    max_norm = float(np.float32(max_norm))
    wd = [DECAY[t % 5] for t in range(24)]
    assert any(w > 0 and k > 1024 for w, k in zip(wd, ADAM_NUMEL)) and any(w == 0 and k > 1024 for w, k in zip(wd, ADAM_NUMEL))
    call = Call(mods, host, ADAM_NUMEL)
    assert call.run(wd, decoupled, max_norm, step) == 0
    _, c = _check_step(call, host, wd, decoupled, max_norm, step, "%s, step %d, %s" % (clip, step, "AdamW" if decoupled else "L2"))
    assert (c < 1e-5) == (clip == "far above") and (1 - 1e-4 < c < 1.0) == (clip == "just above")
    assert (c == 1.0) == (clip in ("at", "below", "inf", "off"))


@pytest.mark.parametrize("how", ["off", "inf", "below", "zero decay array, L2", "at"])
def test_bitwise_csl_adam_f32_without_clipping_and_decay(mods, how):
    """c == 1 and every decay 0: the parameters and moments are bitwise csl_adam_f32's on the same inputs (gradients of
    1e-12 .. 1e12 as in that kernel's own test; steps 1 and 1000)"""
    aggr, L = mods
    for step in (1, 1000):
        host = _hosts(5 + step, ADAM_NUMEL, step, -12, 12)
        n64 = R.grad_norm([four[1] for four in host])
        a, b = Call(mods, host, ADAM_NUMEL), Call(mods, host, ADAM_NUMEL)
        arr = lambda k: (C.c_void_p * 24)(*[a.bufs[t][k].data_ptr() for t in range(24)])      # noqa: E731
        assert L.csl_adam_f32(24, arr(0), arr(1), arr(2), arr(3), a.n64, LR, B1, B2, EPS, step, aggr._stream()) == 0
        max_norm = {"off": 0.0, "inf": float("inf"), "below": float(np.float32(n64 * 2)), "zero decay array, L2": -1.0,
                    "at": _next_f32_at_or_above(n64 + 1e-6)}[how]
        wd = None if how in ("off", "inf") else [0.0] * 24
        assert b.run(wd, how != "zero decay array, L2", max_norm, step) == 0
        moved = 0
        for t, k in enumerate(ADAM_NUMEL):
            for x, y in zip(a.tensors(t), b.tensors(t)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (how, step, t)
            moved += int((a.tensors(t)[0] != torch.from_numpy(host[t][0])).sum())
        assert moved > 1000 and b.skipped() == 0
        b.untouched_around(host)


@pytest.mark.parametrize("mag,max_norm", [(1e20, 1.0), (1e20, float("inf")), (1e-30, 1.0), (0.0, 1.0), (0.0, float("inf"))])
def test_the_norm_where_a_float32_square_overflows_or_vanishes(mods, mag, max_norm):
    numel = [1025, 0, 3, 4097]
    rng = np.random.default_rng(2)
    host = _hosts(3, numel, 1)
    for four, k in zip(host, numel):
        four[1][:] = (mag * rng.uniform(0.5, 1.0, size=k) * rng.choice([-1.0, 1.0], size=k)).astype(np.float32)
    call = Call(mods, host, numel)
    assert call.run(None, True, max_norm, 1) == 0
    n64 = R.grad_norm([four[1] for four in host])
    assert np.isfinite(n64) and (n64 > 0) == (mag > 0)
    assert abs(call.norm() - n64) <= _norm_bound(n64, sum(numel)), (call.norm(), n64)
    print("norm %.9g, float64 %.9g: error / bound %.6g" % (call.norm(), n64,
                                                           abs(call.norm() - n64) / max(_norm_bound(n64, sum(numel)), 1e-300)))
    assert call.skipped() == 0
    call.untouched_around(host)
    for t, k in enumerate(numel):
        p1, m1, v1 = call.tensors(t)
        assert bool(torch.isfinite(p1).all()) and bool(torch.isfinite(m1).all()) and bool(torch.isfinite(v1).all())
        if mag == 0.0:        # zero gradients on zero moments: c = 1, the step runs and changes nothing
            assert torch.equal(p1, torch.from_numpy(host[t][0])) and not bool(m1.any()) and not bool(v1.any())
        elif max_norm == 1.0 and mag == 1e20 and k:
            # clipped from 1e22 to 1: the first moment is (1 - b1) g c, of the size 0.1 / sqrt(N)
            c = R.clip_coef(n64, max_norm)
            _within("adamw m", m1, (1.0 - T._f32(B1)) * torch.from_numpy(host[t][1]).double() * c,
                    5 * U * (1.0 - T._f32(B1)) * torch.from_numpy(host[t][1]).double().abs() * c, "1e20, tensor %d: m" % t)
        elif k:
            assert bool(m1.any())


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("max_norm", [1.0, float("inf")])
def test_a_gradient_that_is_not_finite_skips_the_step(mods, bad, max_norm):
    """one NaN in the last element of the last tensor that has elements / one +Inf in the first element of the first:
    every tensor keeps its bits and the counter goes up by one; the finite step that follows updates as a step on fresh
    copies does, and counts nothing"""
    step = 1000
    host = _hosts(11, ADAM_NUMEL, step)
    wd = [DECAY[t % 5] for t in range(24)]
    good = host[LAST][1][-1], host[FIRST][1][0]
    if bad == "nan":
        host[LAST][1][-1] = np.nan
    else:
        host[FIRST][1][0] = np.inf
    call = Call(mods, host, ADAM_NUMEL)
    for again in (1, 2):
        assert call.run(wd, True, max_norm, step) == 0
        assert call.skipped() == again
        assert np.isnan(call.norm()) if bad == "nan" else call.norm() == float("inf")
        call.untouched_around(host)
        for t, k in enumerate(ADAM_NUMEL):
            for got, j in zip(call.tensors(t), (0, 2, 3)):
                assert torch.equal(got.view(torch.int32), torch.from_numpy(host[t][j]).view(torch.int32)), (bad, t, j)
    # the gradient repaired: the step runs
    host[LAST][1][-1], host[FIRST][1][0] = good
    for t in (FIRST, LAST):
        call.bufs[t][1][:ADAM_NUMEL[t]] = torch.from_numpy(host[t][1]).cuda()
    assert call.run(wd, True, max_norm, step + 1) == 0
    fresh = Call(mods, host, ADAM_NUMEL)
    assert fresh.run(wd, True, max_norm, step + 1) == 0
    assert call.skipped() == 2 and fresh.skipped() == 0 and call.norm() == fresh.norm() and np.isfinite(call.norm())
    for t in range(24):
        for x, y in zip(call.tensors(t), fresh.tensors(t)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), t
    assert not torch.equal(call.tensors(LAST)[0], torch.from_numpy(host[LAST][0]))
    # without clipping there is no guard: the same NaN reaches its own element (and only that one), as in csl_adam_f32
    if bad == "nan":
        host[LAST][1][-1] = np.nan
        plain = Call(mods, host, ADAM_NUMEL)
        assert plain.run(None, True, 0.0, step) == 0
        p1 = plain.tensors(LAST)[0]
        assert bool(torch.isnan(p1[-1])) and bool(torch.isfinite(p1[:-1]).all()) and plain.skipped() == 0


def test_two_calls_give_the_same_bits(mods):
    host = _hosts(23, ADAM_NUMEL, 1000)
    n64 = R.grad_norm([four[1] for four in host])
    wd = [DECAY[t % 5] for t in range(24)]
    a, b = Call(mods, host, ADAM_NUMEL), Call(mods, host, ADAM_NUMEL)
    for call in (a, b):
        assert call.run(wd, False, float(np.float32(n64 / 3)), 1000) == 0
    assert np.float32(a.norm()).view(np.uint32) == np.float32(b.norm()).view(np.uint32)
    assert torch.equal(a.scratch.view(torch.int64), b.scratch.view(torch.int64))          # the partials themselves
    for t in range(24):
        for x, y in zip(a.tensors(t), b.tensors(t)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), t


def test_flat_gradients_equal_separate_ones_with_clipping_and_decay(mods):
    """aggr.Adam.step(flat_grads=...) with the second tensor 12 bytes off a 16-byte boundary against step() on separate
    gradient tensors: bitwise the same parameters, moments and norm, for both forms of the decay"""
    aggr, L = mods
    sizes = [(3,), (41, 25), (64,), (1100,)]
    for decoupled in (True, False):
        torch.manual_seed(3)
        pa = [torch.randn(s, device="cuda") for s in sizes]
        pb = [p.clone() for p in pa]
        kw = dict(lr=3e-3, weight_decay=[0.0, 0.05, 0.0, 0.01], decoupled=decoupled, max_grad_norm=5.0)
        oa, ob = aggr.Adam(pa, **kw), aggr.Adam(pb, **kw)
        assert oa.grad_norm.shape == (1,) and oa.skipped.dtype == torch.int32 and oa._scratch.numel() == 6      # chunks: 1 + 2 + 1 + 2
        for _ in range(3):
            flat = torch.randn(sum(p.numel() for p in pa), device="cuda")
            assert (flat.data_ptr() + 4 * pa[0].numel()) % 16 == 12
            o = 0
            for p in pb:
                p.grad = flat[o:o + p.numel()].clone().view_as(p)
                o += p.numel()
            oa.step(flat_grads=flat)
            ob.step()
            n64 = float(flat.double().norm())
            assert n64 > 5.0 and abs(float(oa.grad_norm) - n64) <= _norm_bound(n64, flat.numel())
            assert torch.equal(oa.grad_norm, ob.grad_norm)
        torch.cuda.synchronize()
        for a, b, sa, sb in zip(pa, pb, oa.state, ob.state):
            assert torch.equal(a, b) and torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
            assert bool(sa[1].any())
        assert int(oa.skipped) == 0 and oa.t == 3


# chunks of the first stage: one block; two; NORM_BLOCKS - 1, NORM_BLOCKS, NORM_BLOCKS + 1 (block 0 takes a second chunk);
# 2 NORM_BLOCKS + 1 (a third).  One tensor, and the same elements over several tensors with an empty one between.
@pytest.mark.parametrize("chunks", [1, 2, NORM_BLOCKS - 1, NORM_BLOCKS, NORM_BLOCKS + 1, 2 * NORM_BLOCKS + 1])
@pytest.mark.parametrize("split", [False, True])
def test_reduction_edges(mods, chunks, split):
    total = (chunks - 1) * ADAM_CHUNK + 1                 # the last chunk holds ONE element
    if split and chunks > 1:
        # a tensor ends inside a chunk: chunks are per tensor, so the parts are sized to keep the count
        numel = [ADAM_CHUNK, 0, total - ADAM_CHUNK]
    elif split:
        numel = [0, 1, 0]
    else:
        numel = [total]
    host = _hosts(chunks, numel, 1)
    last = max(t for t, k in enumerate(numel) if k)
    host[last][1][-1] = np.float32(1e4)                   # the lone element of the last chunk: 1e8 of a sum of squares of
    #                                                       at most 5e5 x 1e6, so a norm that drops it misses the bound
    call = Call(mods, host, numel)
    assert call.scratch_bytes == 8 * min(chunks, NORM_BLOCKS)
    n64 = R.grad_norm([four[1] for four in host])
    max_norm = float(np.float32(n64 / 10))
    assert call.run(None, True, max_norm, 1) == 0
    _check_step(call, host, None, True, max_norm, 1, "%d chunks%s" % (chunks, ", split" if split else ""))


@pytest.mark.parametrize("numel", [[1025], [0] * 13 + [2049] + [0] * 10])
def test_count_edges(mods, numel):
    host = _hosts(len(numel), numel, 1000)
    n64 = R.grad_norm([four[1] for four in host])
    wd = [0.02] * len(numel)
    for decoupled in (True, False):
        call = Call(mods, host, numel)
        max_norm = float(np.float32(n64 / 2))
        assert call.run(wd, decoupled, max_norm, 1000) == 0
        _check_step(call, host, wd, decoupled, max_norm, 1000, "count %d" % len(numel))


def test_refusals_leave_everything_alone(mods):
    host = _hosts(1, [4, 4, 4], 1)
    call = Call(mods, host, [4, 4, 4])
    assert call.run([0.0, -1.0, 0.0], True, 1.0, 1) == E_INVALID
    assert call.run([0.0, float("nan"), 0.0], False, 1.0, 1) == E_INVALID
    assert call.run(None, True, float("nan"), 1) == E_INVALID
    assert call.run(None, True, 1.0, 0) == E_INVALID
    call.untouched_around(host)
    assert call.norm() == SENT and call.skipped() == 0 and bool((call.scratch == SENT).all())
    for t in range(3):
        for got, j in zip(call.tensors(t), (0, 2, 3)):
            assert torch.equal(got, torch.from_numpy(host[t][j]))
