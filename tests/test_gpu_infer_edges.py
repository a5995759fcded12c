"""The full-neighbour inference kernels of csrc/infer.hip (csl_infer_sage_f32, csl_infer_gat_f32, csl_infer_eval_f32 and
the row ends of csrc/infer_dev.h they share) against float64, called through the C ABI at every dispatch edge.

Which parameter reaches which kernel instance.  Both kernels take G = groups_for(width / 4) groups of 64 / G lanes: a
group holds a column tile of 64 / G float4s and a wave reads G * U = 8 G edges per step.

    G    width (W or H * D)   GraphSAGE W    attention (H, D): C                 edges / step   column tile
    16   4 .. 16              4, 16          (1, 4): 4      (4, 4): 16           128            16 floats
    8    20 .. 32             20, 32         (1, 20): 20    (8, 4): 32           64             32
    4    36 .. 64             36, 64         (3, 12): 36    (2, 32): 64          32             64
    2    68 .. 128            68, 128        (1, 68): 68    (4, 32): 128         16             128
    1    132 ..               132, 256,      (3, 44): 132   (8, 32): 256         8              256
                              260, 516       (5, 52): 260   (4, 132): 528

so k_infer_sage<G> and k_infer_gat<G> are launched for every G, on both sides of every switch.  260 walks a full and a
partial column tile, 516 and 528 a first, an INTERIOR full and a partial last one; in (3, 12), (3, 44), (5, 52) and
(4, 132) heads straddle groups' lanes or column tiles and H is no power of two.  The last attention layer (last = 1:
row staged in LDS, head mean) runs at G = 8 (4, 8), 4 (8, 8), 2 (2, 64), 1 (2, 68), (8, 32) and, at exactly
GAT_LAST_MAX_C = 4096 columns (64 KiB of LDS a block), (8, 512) with n_cls = D and n_cls = 500; n_cls 65, 500 and 512
make the head-mean loop stride, 7, 1 and 65 give output rows that are not 16-byte aligned (ldo = n_cls).

Row lengths (LENS) meet both sides of every step size above (8, 16, 32, 64, 128), of the 64-edge index batch and of an
item's CSL_INFER_SEG = 512 edges.  Lengths 513 and 1024 are hubs of 2 parts, 1025 of 3, 3584 of 7, 4096 of 8, 4097 of 9
and 8193 of 17: the hub pass of k_infer_sage_hubs adds partials in groups of U = 8 with a remainder loop, so 7 is
remainder only, 8 one full group, 9 and 17 groups with a remainder of one; k_infer_gat_hubs merges the same part counts
with lse_merge.  The part counts are asserted from build_plan's result: another CSL_INFER_SEG fails here loudly.

The plan is over the rows in shuffled order (item.row != item.pos: er and the self row are indexed by graph row, out by
position), a few graph rows are in no plan, and every call is made whole, in two (the second chunk starts with a hub:
pos0 and part0 non-zero) and in three, bitwise equal.  out and partial sit inside sentinels.

Tolerances.  Outputs: every row within 1e-5 of that row's largest float64 reference entry (the rule of
tests/test_gpu_infer.py::_close, without the 1e-4 it grants its 200,000-edge hub: a sequential float32 sum of these
inputs, a worse order than the kernels' tree, stays below 4e-6 of the row's largest entry up to 8,193 edges, and the
running-maximum softmax recurrence at scores of about 120 below 6e-6).  The attention reference takes the score as the
kernel forms it, leaky(float32(el[u] + er[v])), so no logit rounding is magnified by exp and the 3e-5 that
tests/test_gpu_gat_edges.py derives for that cause is not needed.  Evaluation head: pred and correct exact, loss_row
within 1e-5 relative of float64 logsumexp - logit[label], loss_sum within 1e-6 relative of the float64 sum of the
kernel's own loss_row (the kernel adds in double).  That bound on loss_row is why k_infer_eval_rows forms the loss as
(max - logit[label]) + log(sum): with max + log(sum) first the sum rounds at the size of the logits, and the rows shifted
by 80 missed it at C = 2 (up to 3.5e-6 absolute, 2.6e-5 of the row's loss).

Largest errors seen on an MI355X, as fractions of the row's largest entry: GraphSAGE 1.7e-6, attention hidden 2.7e-6,
attention last 4.1e-7; loss_row 3.4e-7 relative."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEG = 512
S = -7777.0          # sentinel around out and partial
N_SRC = 700          # rows of the source tables (graph nodes)
TOL = 1e-5

# rows in the plan, by graph order (short rows between the edges of the step sizes)
LENS = [0, 1, 7, 8, 9, 3, 15, 16, 17, 5, 31, 32, 33, 2, 63, 64, 65, 11, 127, 128, 129, 6, 511, 512, 513, 4, 1024, 1025,
        0, 3584, 13, 4096, 4097, 40, 8193, 1, 20, 3]
HUB_PARTS = {513: 2, 1024: 2, 1025: 3, 3584: 7, 4096: 8, 4097: 9, 8193: 17}
EXTRA = {0: 5, 10: 600, 25: 0, 30: 9}      # graph row -> length of the rows that are in no plan
ONE_SOURCE, REPEATS = 33, (129, 4097)      # a row whose sources are all one source; rows that repeat one many times


def _rows_close(got, want, tol, what):
    """every entry finite and |got - want| <= tol * (the row's largest |want|), row by row; returns the largest ratio"""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, what
    assert bool(torch.isfinite(got).all()), "%s: not finite at %s" % (what, torch.nonzero(~torch.isfinite(got))[:5].tolist())
    err = (got - want).abs().amax(1) / want.abs().amax(1).clamp_min(1e-30)
    worst = float(err.max())
    print("%s: largest row error %.3g of the row's largest entry (tolerance %g)" % (what, worst, tol))
    bad = torch.nonzero(err > tol).reshape(-1)
    assert bad.numel() == 0, "%s: positions %s: relative errors %s" % (what, bad[:10].tolist(), err[bad[:10]].tolist())
    return worst


@functools.lru_cache(maxsize=None)
def _host_graph(max_len):
    """The graph (rows of LENS up to max_len edges, the EXTRA rows between them) and the plan over its planned rows in
    shuffled order, with the positions at which the calls are cut"""
    from cslicer import infer
    rng = np.random.default_rng(20 + max_len)
    planned = [n for n in LENS if n <= max_len]
    glens, in_plan = [], []
    it = iter(planned)
    for r in range(len(planned) + len(EXTRA)):
        glens.append(EXTRA[r] if r in EXTRA else next(it))
        in_plan.append(r not in EXTRA)
    ip = np.zeros(len(glens) + 1, dtype=np.int64)
    np.cumsum(glens, out=ip[1:])
    ix = rng.integers(0, N_SRC, int(ip[-1])).astype(np.int32)
    for r, n in enumerate(glens):
        if in_plan[r] and n == ONE_SOURCE:
            ix[ip[r]:ip[r + 1]] = ix[ip[r]]
        if in_plan[r] and n in REPEATS:
            ix[ip[r]:ip[r + 1]:2] = ix[ip[r]]
    rows = rng.permutation(np.flatnonzero(in_plan)).astype(np.int64)
    n = rows.shape[0]
    w = infer.build_plan(ip, rows)
    # row != pos almost everywhere
    assert np.count_nonzero(w["items"][:, 0] != w["items"][:, 1]) >= w["items"].shape[0] - 2
    # the hub shapes, from the plan itself
    want_parts = [HUB_PARTS[x] for x in planned if x > SEG]
    assert sorted(w["hubs"][:, 3].tolist()) == sorted(want_parts)
    assert [HUB_PARTS[glens[r]] for r in w["hubs"][:, 0]] == w["hubs"][:, 3].tolist()
    assert w["n_parts"] == sum(want_parts) and w["n"] == n
    assert w["items"].shape[0] == n - len(want_parts) + sum(want_parts)
    if max_len >= max(LENS):
        assert sorted(want_parts) == [2, 2, 3, 7, 8, 9, 17] and w["n_parts"] == 48
    hp = w["hub_pos"]
    cuts = {1: [], 2: [int(hp[len(hp) // 2])], 3: [int(hp[1]), int(hp[-1])]}
    for c in cuts[2] + cuts[3]:
        assert c > 0 and w["part_first"][c] > 0 and c in hp       # pos0 != 0, part0 != 0, a hub first
    return {"ip": ip, "ix": ix, "rows": rows, "n": n, "w": w, "cuts": cuts, "n_graph": len(glens),
            "edge_row": torch.from_numpy(np.repeat(np.arange(len(glens)), glens))}


@functools.lru_cache(maxsize=None)
def _graph(max_len):
    """_host_graph with the device copies of its CSR and work list"""
    g = dict(_host_graph(max_len))
    for name, a in (("dip", g["ip"].astype(np.int32)), ("dix", g["ix"]), ("items", g["w"]["items"]),
                    ("hubs", g["w"]["hubs"])):
        g[name] = torch.from_numpy(a).cuda()
    return g


def _chunks(g, ways):
    """the plan cut into `ways` calls: (s0, s1, i0, i1, h0, h1, part0, n_parts) each"""
    w = g["w"]
    b = [0] + g["cuts"][ways] + [g["n"]]
    out = []
    for s0, s1 in zip(b[:-1], b[1:]):
        h0, h1 = (int(x) for x in np.searchsorted(w["hub_pos"], [s0, s1]))
        p0 = int(w["part_first"][s0])
        out.append((s0, s1, int(w["item_first"][s0]), int(w["item_first"][s1]), h0, h1, p0, int(w["part_first"][s1]) - p0))
    return out


class _Guarded(object):
    """n rows of `width` floats at row stride ld, `left` guard columns before them, a guard row before and after: all
    of it the sentinel until a kernel writes"""

    def __init__(self, n, width, ld, left):
        assert left + width <= ld
        self.n, self.width, self.ld, self.left = n, width, ld, left
        self.buf = torch.full(((n + 2) * ld,), S, device="cuda")

    def at(self, row):
        from cslicer import infer
        return infer._ptr(self.buf, (1 + row) * self.ld + self.left)

    def inner(self):
        return self.buf.view(self.n + 2, self.ld)[1:-1, self.left:self.left + self.width]

    def result(self, what):
        """the rows written, after checking that every sentinel survived and no written entry is one"""
        guard = self.buf.clone().view(self.n + 2, self.ld)
        guard[1:-1, self.left:self.left + self.width] = S
        assert bool((guard == S).all()), what + ": a sentinel was overwritten"
        got = self.inner().clone()
        assert not bool((got == S).any()), what + ": an entry was not written"
        return got


def _list_args(g, c):
    from cslicer import infer
    s0, s1, i0, i1, h0, h1, p0, npart = c
    return (infer._ptr(g["dip"]), infer._ptr(g["dix"]), infer._ptr(g["items"], 4 * i0), i1 - i0,
            infer._ptr(g["hubs"], 4 * h0) if h1 > h0 else None, h1 - h0, s0, p0)


def _three_ways(run, what):
    """run(ways) -> (out, partial rows) as one call, two and three: bitwise equal; returns the one-call result"""
    out, part = run(1)
    for ways in (2, 3):
        out_w, part_w = run(ways)
        assert torch.equal(out_w, out), "%s: %d calls differ from one" % (what, ways)
        assert torch.equal(part_w, part), "%s: the partials of %d calls differ from one" % (what, ways)
    return out


def _column_block(t, wide):
    """t on the device: contiguous, or as a 16-byte aligned column block of a wider buffer (row stride + 8)"""
    if not wide:
        return t.cuda()
    buf = torch.full((t.shape[0], t.shape[1] + 8), 3.0)
    buf[:, 4:4 + t.shape[1]] = t
    x = buf.cuda()[:, 4:4 + t.shape[1]]
    assert x.stride(0) == t.shape[1] + 8 and x.data_ptr() % 16 == 0
    return x


# ---------------------------------------------------------------------------------------------------------------------
# GraphSAGE

SAGE_W = [4, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 516]
# (W, proj, bias, relu, x as a column block): both forms at every width, ldx above its minimum in half of the cases
SAGE_CASES = ([(W, 0, False, False, i % 2 == 0) for i, W in enumerate(SAGE_W)]
              + [(W, 1, True, True, i % 2 == 1) for i, W in enumerate(SAGE_W)]
              + [(36, 1, False, True, False), (132, 1, True, False, True)])


@pytest.mark.parametrize("W,proj,bias,relu,wide", SAGE_CASES)
def test_sage_against_float64(W, proj, bias, relu, wide):
    from cslicer import aggr, infer
    L, st = infer._lib(), aggr._stream()
    g = _graph(max(LENS))
    n, rows = g["n"], g["rows"]
    gen = torch.Generator().manual_seed(W * 4 + proj * 2 + bias)
    xw = 2 * W if proj else W
    x = torch.rand((N_SRC, xw), generator=gen) * 2 - 1
    b = torch.rand((W,), generator=gen) - 0.5 if bias else None
    xd = _column_block(x, wide)
    bd = b.cuda() if bias else None
    out_w = W if proj else 2 * W
    what = "sage W=%d proj=%d bias=%d relu=%d" % (W, proj, bias, relu)

    def run(ways):
        out = _Guarded(n, out_w, out_w + 8, 4)
        parts = []
        for c in _chunks(g, ways):
            part = torch.full((c[7] + 2, W), S, device="cuda")
            rc = L.csl_infer_sage_f32(*_list_args(g, c), infer._ptr(xd), xd.stride(0), W, proj, infer._ptr(bd), int(relu),
                                      infer._ptr(part, W), out.at(c[0]), out.ld, st)
            assert rc == 0, what
            parts.append(part)
        torch.cuda.synchronize()
        for part in parts:
            assert bool((part[0] == S).all()) and bool((part[-1] == S).all()), what + ": partial guard rows"
        return out.result(what), torch.cat([p[1:-1] for p in parts])

    got = _three_ways(run, what).cpu()
    x64 = x.double()
    noff = W if proj else 0
    acc = torch.zeros((g["n_graph"], W), dtype=torch.float64)
    acc.index_add_(0, g["edge_row"], x64[torch.from_numpy(g["ix"]).long(), noff:noff + W])
    deg = torch.from_numpy(np.diff(g["ip"])[rows]).double()
    mean = acc[rows] / deg.clamp_min(1.0)[:, None]
    assert bool((mean[deg == 0] == 0).all())
    self_ = x64[rows, :W]
    if proj:
        want = self_ + mean + (b.double() if bias else 0.0)
        want = torch.relu(want) if relu else want
    else:
        want = torch.cat([self_, mean], 1)
        assert torch.equal(got[:, :W], x[rows, :W]), what + ": the self half is a copy"
    _rows_close(got, want, TOL, what)


# ---------------------------------------------------------------------------------------------------------------------
# attention

def _gat_inputs(g, H, D, shift, bias, seed, bias_lo=-0.5):
    """z in [-1, 1), el / er in [-2, 2) + shift (er by graph row), bias in [bias_lo, bias_lo + 1) or None"""
    gen = torch.Generator().manual_seed(seed)
    z = torch.rand((N_SRC, H * D), generator=gen) * 2 - 1
    el = torch.rand((N_SRC, H), generator=gen) * 4 - 2 + shift
    er = torch.rand((g["n_graph"], H), generator=gen) * 4 - 2 + shift        # by graph row
    b = torch.rand((H * D,), generator=gen) + bias_lo if bias else None
    return z, el, er, b


def _gat_ref(g, z, el, er, b, H, D, slope, last, n_cls):
    """float64 from the kernel's float32 scores leaky(float32(el[u] + er[v])): softmax over the row's edges with
    multiplicity, n / s + bias, then ELU (hidden) or the head mean sliced to n_cls (last)"""
    z64 = z.double()
    b64 = b.double().view(H, D) if b is not None else torch.zeros((H, D), dtype=torch.float64)
    want = []
    for row in g["rows"]:
        src = torch.from_numpy(g["ix"][g["ip"][row]:g["ip"][row + 1]]).long()
        if src.numel():
            sc = torch.nn.functional.leaky_relu(el[src] + er[row], slope).double()
            p = torch.exp(sc - sc.max(0).values)
            y = torch.einsum("eh,ehd->hd", p, z64[src].view(-1, H, D)) / p.sum(0)[:, None] + b64
        else:
            y = b64.clone()
        want.append(y.mean(0)[:n_cls] if last else torch.nn.functional.elu(y).reshape(-1))
    return torch.stack(want)


def _run_gat(g, z, el, er, b, H, D, slope, last, n_cls, ldo, left, what):
    from cslicer import aggr, infer
    L, st = infer._lib(), aggr._stream()
    pld = int(L.csl_infer_gat_partial_ld(H, D))
    assert pld >= H * D + 2 * H and pld % 4 == 0
    zd, eld, erd = z.cuda(), el.cuda(), er.cuda()
    bd = b.cuda() if b is not None else None
    width = n_cls if last else H * D

    def run(ways):
        out = _Guarded(g["n"], width, ldo, left)
        parts = []
        for c in _chunks(g, ways):
            part = torch.full((c[7] + 2, pld), S, device="cuda")
            rc = L.csl_infer_gat_f32(*_list_args(g, c), infer._ptr(zd), infer._ptr(eld), infer._ptr(erd), H, D,
                                     float(slope), infer._ptr(bd), int(last), n_cls if last else 0, infer._ptr(part, pld),
                                     out.at(c[0]), ldo, st)
            assert rc == 0, what
            parts.append(part)
        torch.cuda.synchronize()
        for part in parts:
            assert bool((part[0] == S).all()) and bool((part[-1] == S).all()), what + ": partial guard rows"
            assert not bool((part[1:-1, :H * D + 2 * H] == S).any()), what + ": a partial state was not written"
        return out.result(what), torch.cat([p[1:-1] for p in parts])

    return _three_ways(run, what)


GAT_HIDDEN = [(1, 4), (4, 4), (1, 20), (8, 4), (3, 12), (2, 32), (1, 68), (4, 32), (3, 44), (8, 32), (5, 52), (4, 132)]
# 0 and 0.2 with scores of both signs; about +120 an unshifted exp overflows (above 88), about -120 (slope 1 keeps the
# score negative) it underflows (below -103)
SLOPE_SHIFT = [(0.0, 0.0), (0.2, 0.0), (0.2, 120.0), (1.0, -120.0)]


@pytest.mark.parametrize("slope,shift", SLOPE_SHIFT)
@pytest.mark.parametrize("H,D,bias", [(H, D, True) for H, D in GAT_HIDDEN] + [(3, 12, False)])
def test_gat_hidden_against_float64(H, D, bias, slope, shift):
    g = _graph(max(LENS))
    C = H * D
    what = "gat hidden H=%d D=%d bias=%d slope=%g shift=%g" % (H, D, bias, slope, shift)
    z, el, er, b = _gat_inputs(g, H, D, shift, bias, 100 * C + int(shift))
    got = _run_gat(g, z, el, er, b, H, D, slope, 0, 0, C + 8, 4, what)
    _rows_close(got, _gat_ref(g, z, el, er, b, H, D, slope, False, 0), TOL, what)


# (H, D, n_cls, guard columns (left, right) around the n_cls outputs, score shift): ldo = n_cls unless guarded
GAT_LAST = [(4, 8, 7, (0, 0), 0.0), (8, 8, 1, (0, 0), 120.0), (2, 64, 64, (0, 0), 0.0), (2, 68, 65, (0, 0), -120.0),
            (8, 32, 32, (3, 2), 120.0), (8, 512, 512, (0, 0), 0.0), (8, 512, 500, (0, 0), 120.0)]


@pytest.mark.parametrize("H,D,n_cls,guard,shift", GAT_LAST)
def test_gat_last_against_float64(H, D, n_cls, guard, shift):
    from cslicer import infer
    C = H * D
    assert C <= infer.GAT_LAST_MAX_C
    # at 4,096 columns the rows of up to 1,025 edges: hubs of 2, 2 and 3 parts among them
    g = _graph(1025 if C == infer.GAT_LAST_MAX_C else max(LENS))
    assert g["w"]["hubs"].shape[0] >= 3 and g["n"] >= 30
    slope = 1.0 if shift < 0 else 0.2
    what = "gat last H=%d D=%d n_cls=%d shift=%g" % (H, D, n_cls, shift)
    # bias in [1, 2): every head's term n / s + bias (n / s is a mean of z, inside (-1, 1)) is positive, so the head mean
    # does not cancel and the row's largest entry is the size of the data.  It has to be: at n_cls = 1 that entry is the
    # row's only one, and with a bias in [-0.5, 0.5) the 4,097-edge row came out as 0.0125 from head terms of up to
    # 0.83; the kernel's error there, 2.1e-7 (2.5e-7 of the largest term, two float32 roundings), read as 1.67e-5.
    z, el, er, b = _gat_inputs(g, H, D, shift, True, 7 * C + n_cls, bias_lo=1.0)
    got = _run_gat(g, z, el, er, b, H, D, slope, 1, n_cls, n_cls + sum(guard), guard[0], what)
    _rows_close(got, _gat_ref(g, z, el, er, b, H, D, slope, True, n_cls), TOL, what)


# ---------------------------------------------------------------------------------------------------------------------
# evaluation head

def _eval_rows(rng, n, C):
    """logits [n, C] in [-1, 1) and labels; by k: exact ties of the maximum in different lanes (column % 64), in
    different strides of one lane (columns 64 apart), an all-equal row, -inf everywhere but at the label, the row
    shifted by +80 and by -80"""
    x = rng.uniform(-1.0, 1.0, (n, C)).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.int64)
    for k in range(n):
        kind = (k + n) % 8
        if kind == 2 and C > 64:                                 # one lane, two or three of its strides
            j = int(rng.integers(0, C - 64))
            x[k, j::64] = 2.0
        elif kind in (1, 2) and C >= 2:                          # different lanes (the higher column may be the lower lane's)
            j1 = int(rng.integers(0, C - 1))
            j2 = int(rng.integers(j1 + 1, C))
            if (j2 - j1) % 64 == 0:
                j2 = j1 + 1
            x[k, [j1, j2]] = 2.0
        elif kind == 3:
            x[k] = 0.25
        elif kind == 4:
            keep = x[k, y[k]]
            x[k] = -np.inf
            x[k, y[k]] = keep
        elif kind == 5:
            x[k] += np.float32(80.0)
        elif kind == 6:
            x[k] -= np.float32(80.0)
    return x, y


def _call_eval(lg, n, C, labels):
    from cslicer import aggr, infer
    pred = torch.full((n + 2,), -5, dtype=torch.int64, device="cuda")
    loss_row = torch.full((n + 2,), S, device="cuda")
    loss_sum = torch.full((3,), S, dtype=torch.float64, device="cuda")
    correct = torch.full((3,), -5, dtype=torch.int64, device="cuda")
    yd = torch.from_numpy(labels).cuda()
    rc = infer._lib().csl_infer_eval_f32(infer._ptr(lg), lg.stride(0), n, C, infer._ptr(yd), infer._ptr(pred, 1),
                                         infer._ptr(loss_row, 1), infer._ptr(loss_sum, 1), infer._ptr(correct, 1),
                                         aggr._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert pred[0] == -5 and pred[-1] == -5 and loss_row[0] == S and loss_row[-1] == S
    assert loss_sum[0] == S and loss_sum[2] == S and correct[0] == -5 and correct[2] == -5
    return pred[1:-1].cpu().numpy(), loss_row[1:-1].cpu().numpy(), float(loss_sum[1]), int(correct[1])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3001])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 128, 200])
def test_eval_head_against_float64(C, n):
    x, y = _eval_rows(np.random.default_rng(1000 * C + n), n, C)
    x64 = x.astype(np.float64)
    m = x64.max(1)
    want = m + np.log(np.exp(x64 - m[:, None]).sum(1)) - x64[np.arange(n), y]
    assert np.isfinite(want).all()
    want_pred = np.argmax(x, axis=1)
    for ld in (C, C + 3):
        if ld == C:
            lg = torch.from_numpy(x).cuda()
        else:                                                    # a column block; its neighbours would win every argmax
            buf = torch.full((n, ld), 1e30)
            buf[:, 2:2 + C] = torch.from_numpy(x)
            lg = buf.cuda()[:, 2:2 + C]
        assert lg.stride(0) == ld
        pred, loss_row, loss_sum, correct = _call_eval(lg, n, C, y)
        assert np.array_equal(pred, want_pred)
        assert correct == int(np.count_nonzero(want_pred == y))
        err = np.abs(loss_row.astype(np.float64) - want)
        print("eval C=%d n=%d ld=%d: largest loss_row error %.3g relative (tolerance 1e-5)"
              % (C, n, ld, float((err / np.maximum(np.abs(want), 1e-300)).max())))
        assert (err <= 1e-5 * np.abs(want)).all(), (np.flatnonzero(err > 1e-5 * np.abs(want))[:5],
                                                    err[err > 1e-5 * np.abs(want)][:5])
        total = float(loss_row.astype(np.float64).sum())
        assert abs(loss_sum - total) <= 1e-6 * abs(total)
        # a label outside [0, C): that row's loss and the sum are NaN, pred and the other rows' losses stay
        for bad in (-1, C):
            y2 = y.copy()
            y2[n // 2] = bad
            pred2, loss_row2, loss_sum2, correct2 = _call_eval(lg, n, C, y2)
            assert np.isnan(loss_row2[n // 2]) and np.isnan(loss_sum2)
            assert np.array_equal(pred2, want_pred)
            assert correct2 == int(np.count_nonzero(want_pred == y2))
            others = np.arange(n) != n // 2
            assert np.array_equal(loss_row2[others].view(np.int32), loss_row[others].view(np.int32))
