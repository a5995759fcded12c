"""Dropout between the GraphSAGE layers (include/cslicer_dropout.h, csrc/dropout.hip, the `drop` branch of sage_step in
csrc/sage_step.hip) at its dispatch edges and beyond p = 0.5 -- next to tests/test_gpu_dropout.py, which pins
p = 0.5 at small shapes.  The kernels are called through the C ABI, so that leading dimensions and pointer offsets are
the test's own.

What decides how the code runs, and what is therefore varied here:
  * k_dropout: a row is walked by 2^lg lanes, lg = ceil(log2(H / 4)) <= 6, 256 >> lg rows per workgroup, the lanes stride
    the quads beyond 64: H / 4 on both sides of every power of two up to 64 and 2, 3, 4 trips of the stride loop, one row,
    one row less than, exactly and one more than a workgroup's rows, three workgroups and a row; x and y as blocks of wider
    sentinel-filled buffers, in place; ids and row indices; p whose threshold is 0 and 2^32 - 256; -0.0, Inf, NaN under
    the mask (a dropped element is +0.0 whatever it held);
  * k_scale_segments: blocks of 1,024 elements, the block-to-segment lookup first_block[], zero-length segments skipped
    on the host, up to 8 segments of up to 128 blocks at odd offsets of one flat buffer, a factor of its own per segment;
  * sage_step with `drop`: a scale s that is no power of two (p = 0.1, 0.3, 0.7, 0.9), the deferred factors s^(L-1-j) up to
    s^3 (L = 4 = CSL_MAX_LAYERS), no row padding, a layer shorter than row_pad, slabs that do not divide the rows, hub
    lists by source, more than 256 classes, the bench's widths (weight-gradient segments of 131,072 and 51,200 floats:
    the scaling launch spans 180 blocks), and the same through csl_sage_fwd_bwd_ce and csl_sage_fwd_bwd_multilabel.

Tolerances.  The two kernels: bit for bit (each is ONE fp32 multiplication per element, the numpy reference restates it;
a NaN matches any NaN).  The step: loss within 1e-5 relative, every parameter gradient within 1e-4 of the
float64 tensor's largest entry, against the float64 model with the same masks on the oracle's traversal -- never against
another HIP path.  p = 2^-33 (threshold 0, s == 1.0f) against the plain step and a 16-bit table against its upcast: bit for
bit.

Largest error / bound seen on an MI355X, per group (every test prints its own: pytest -s); nothing comes near the rule,
p = 0.9 at four layers (gradients up to 5.1, a factor of 999.99945 on the deepest layer's) included:
    sequencer matrix 0.0068 (the loss of L = 3, 300 classes, p = 0.7; L = 4 at p = 0.9: 0.0044, at p = 0.3: 0.0041)
    bench widths 0.0077 (gW_0)    cross-entropy options 0.0074 (loss)    multi-label 0.012 (loss)
    native against autograd trainer step at dropout = 0.3: 0.0024
No defect was found in dropout.hip, sage_step.hip or aggr.py.

Scratch checks, not in the tree (each a build with one line changed, every access still in bounds):
  * k_scale_segments looks its segment up with `blockIdx.x > first_block[j + 1]`: the 8 scale cases of more than one
    non-empty segment fail, the single-segment and the empty ones pass (rightly); every float64 step test fails too
    (the step's launch has 2 to 6 segments);
  * k_dropout's stride loop stops after one trip: all 20 cases of H = 260, 512, 516, 1024 fail, the 60 narrower pass;
  * drop4 multiplies by a 0 / s mask instead of selecting 0.f: all 80 kernel cases fail (a dropped negative is -0.0, a
    dropped Inf or NaN a NaN);
  * the factors s^(L-2-j) in place of s^(L-1-j): all 8 matrix rows, the bench widths, the two other entry points and the
    trainer comparison fail; p = 2^-33 and the 16-bit twins pass (rightly: all factors are 1, both sides are alike);
  * the factor carried as a float product instead of a double product cast once: NOT observable.  For p = 0.3, 0.5, 0.7
    and 0.9 both give the same float32 s^2 and s^3; for p = 0.1 the cubes differ in the last bit, 6e-8 relative, far
    inside any bound against float64, and the step's unscaled gradient cannot be read through the C ABI.  What is pinned
    is that k_scale_segments applies exactly the factor it is handed (test_the_factors_are_distinct_and_formed_in_double).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dropout_ref

pytestmark = pytest.mark.gpu

SENT = -77.25
P_LO = 2.0 ** -33            # threshold 0, s == 1.0f: nothing is dropped, nothing is scaled
P_HI = 1.0 - 2.0 ** -24      # the largest float32 below 1: threshold 2^32 - 256, s == 2^24


@pytest.fixture(scope="module")
def lib():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr._lib()


def _same(got, want, what=""):
    """bit for bit as uint32 views, except that a NaN matches any NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert bool(np.isnan(got[nan]).all()), what + ": a NaN was expected"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not bad.any(), "%s: %d of %d floats differ, the first at %s" % (what, int(bad.sum()), bad.size,
                                                                         tuple(np.argwhere(bad)[0]))


# ---- A. csl_dropout_f32 against dropout_ref.apply ---------------------------------------------------------------------------

WIDTHS = [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024]
ROWS = ["1", "R-1", "R", "R+1", "3R+1"]
SEED_A = (0x9abcdef1 << 32) | 77
# (p, layer, step, keyed by ids); every step >= 2^32
COMBOS = [(0.1, 0, (1 << 32) + 5, True), (0.3, 3, (1 << 32) + 5, False), (0.5, 3, (1 << 32) + 5, True),
          (0.5, 0, (1 << 32) + 5, True), (0.9, 0, (7 << 32) + 1, True), (P_LO, 3, (1 << 32) + 5, True),
          (P_HI, 0, (1 << 32) + 5, False)]


def _lg(H):
    lg = 0
    while lg < 6 and (1 << lg) < H // 4:
        lg += 1
    return lg


def _rows(H, which):
    R = 256 >> _lg(H)
    return {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "3R+1": 3 * R + 1}[which]


def _ids(n, rng):
    """distinct non-negative int32 node ids in no order, one of them 2^31 - 1"""
    ids = rng.permutation(1 << 20)[:n].astype(np.int64) * 2047 + 5
    ids[rng.integers(0, n)] = (1 << 31) - 1
    return ids


def _data(n, H, rng):
    """normals with exact zeros, -0.0, Inf, -Inf and NaN scattered in (about one element in six, the five in turn)"""
    x = rng.standard_normal(n * H).astype(np.float32)
    at = np.flatnonzero(rng.random(n * H) < 0.17)
    x[at] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(at.shape[0]) % 5]
    return x.reshape(n, H)


def _drop_call(lib, src, ldx, dst, ldy, ids, n, H, p, layer, step, seed=SEED_A):
    """csl_dropout_f32 on the block that starts at row 1, column 4 of src [n + 2, ldx] and of dst [n + 2, ldy]"""
    from cslicer import aggr
    x, y = src.data_ptr() + 4 * (ldx + 4), dst.data_ptr() + 4 * (ldy + 4)
    assert src.is_contiguous() and dst.is_contiguous() and src.shape == (n + 2, ldx) and dst.shape == (n + 2, ldy)
    rc = lib.csl_dropout_f32(C.c_void_p(x), ldx, C.c_void_p(y), ldy, C.c_void_p(ids.data_ptr() if ids is not None else 0),
                             n, H, p, aggr._i64(seed), layer, aggr._i64(step), aggr._stream())
    assert rc == 0, (rc, n, H, p)


@pytest.mark.parametrize("which", ROWS)
@pytest.mark.parametrize("H", WIDTHS)
def test_dropout_kernel_is_the_numpy_mask_at_every_lane_count_and_row_edge(lib, H, which):
    n = _rows(H, which)
    assert n * H < 300_000
    rng = np.random.default_rng(H * 10007 + n)
    ldx, ldy = H + 4, H + 8
    ids_np = _ids(n, rng)
    ids = torch.from_numpy(ids_np.astype(np.int32)).cuda()
    x_np = _data(n, H, rng)
    src0 = np.full((n + 2, ldx), SENT, dtype=np.float32)
    src0[1:n + 1, 4:4 + H] = x_np
    blocks = {}
    for p, layer, step, keyed in COMBOS:
        what = "H %d n %d p %.9g layer %d step %d %s" % (H, n, p, layer, step, "ids" if keyed else "rows")
        key = ids_np if keyed else np.arange(n)
        with np.errstate(all="ignore"):
            want = dropout_ref.apply(x_np, key, p, SEED_A, layer, step)
        keep = dropout_ref.keep_mask(key, H, p, SEED_A, layer, step)
        # out of place into a block of another leading dimension: x and every float around both blocks unchanged
        src = torch.from_numpy(src0).cuda()
        dst = torch.full((n + 2, ldy), SENT, device="cuda")
        _drop_call(lib, src, ldx, dst, ldy, ids if keyed else None, n, H, p, layer, step)
        want_dst = np.full((n + 2, ldy), SENT, dtype=np.float32)
        want_dst[1:n + 1, 4:4 + H] = want
        got_dst = dst.cpu().numpy()
        _same(got_dst, want_dst, what + ", out of place")
        _same(src.cpu().numpy(), src0, what + ", out of place: x")
        # in place (y == x)
        _drop_call(lib, src, ldx, src, ldx, ids if keyed else None, n, H, p, layer, step)
        want_src = src0.copy()
        want_src[1:n + 1, 4:4 + H] = want
        _same(src.cpu().numpy(), want_src, what + ", in place")
        # what the header promises, said without the reference's arithmetic: y = keep ? x * s : 0
        got = got_dst[1:n + 1, 4:4 + H]
        assert bool((got.view(np.uint32)[~keep] == 0).all()), what + ": a dropped element is +0.0 whatever it held"
        inf = np.isinf(x_np) & keep
        assert np.array_equal(got[inf], x_np[inf]) and bool(np.isnan(got[np.isnan(x_np) & keep]).all()), what
        blocks[(p, layer)] = (got, keep)
    # p = 2^-33: the input itself, -0.0 included
    got, keep = blocks[(P_LO, 3)]
    assert bool(keep.all())
    _same(got, x_np, "p = 2^-33")
    assert np.array_equal(np.signbit(got), np.signbit(x_np))
    # p = 1 - 2^-24: a kept element is x * 2^24 (one element in 2^24 is kept: none in most cases)
    got, keep = blocks[(P_HI, 0)]
    with np.errstate(all="ignore"):
        _same(got[keep], x_np[keep] * np.float32(2.0 ** 24), "p = 1 - 2^-24")
    # the counter words: step mod 2^32, and the neighbouring steps and the other layer are other masks
    a = blocks[(0.5, 3)][0]
    outs = []
    for layer, step in ((3, 5), (3, (1 << 32) + 4), (3, (1 << 32) + 6)):
        src = torch.from_numpy(src0).cuda()
        _drop_call(lib, src, ldx, src, ldx, ids, n, H, 0.5, layer, step)
        outs.append(src.cpu().numpy()[1:n + 1, 4:4 + H])
    _same(outs[0], a, "step 2^32 + 5 is step 5")
    if n * H >= 64:
        for other in (outs[1], outs[2], blocks[(0.5, 0)][0]):
            assert not np.array_equal(np.nan_to_num(other), np.nan_to_num(a))
    if n * H >= 256:    # (the data of this case does put Inf / NaN on both sides of the mask)
        keep = blocks[(0.5, 3)][1]
        bad = ~np.isfinite(x_np)
        assert bool((bad & keep).any()) and bool((bad & ~keep).any())


# ---- B. csl_scale_segments_f32 against one numpy float32 multiplication -----------------------------------------------------

def _step_factor(p, k):
    """s^k as sage_step forms it: s1 = (double)(float)(1 / (1 - (double)p)), a double product, ONE cast to float"""
    s1 = float(np.float32(1.0 / (1.0 - float(np.float32(p)))))
    f = 1.0
    for _ in range(k):
        f *= s1
    return np.float32(f)


FACTORS = [_step_factor(0.3, 1), _step_factor(0.9, 3), np.float32(-1.75), _step_factor(0.3, 3), np.float32(1.0),
           _step_factor(0.9, 2), _step_factor(0.3, 2), _step_factor(0.9, 1), _step_factor(0.1, 3)]
BIG = 131072                 # a 256 x 512 weight gradient: 128 blocks
SCALE_CASES = [
    ("one-of-128-blocks", [BIG]),
    ("one-element", [1]),
    ("eight-non-empty", [1, 255, 256, 257, 1023, 1024, 1025, 2048]),
    ("zero-first-adjacent-in-the-middle-last", [0, 3 * 1024 + 5, 0, 0, BIG, 1, 0]),
    ("chunk-boundary-then-one-element", [1024, 1]),
    ("two-chunks-then-one-then-a-partial", [2048, 1, 1023, 1025]),
    ("eight-with-two-of-128-blocks", [3 * 1024 + 5, BIG, 257, 0, 1024, 1, BIG, 255]),
    ("three", [1025, 1024, 1023]),
    ("five-with-a-zero", [256, 0, 257, 2048, 1]),
    ("six-single-elements", [1, 1, 1, 1, 1, 1]),
    ("only-zeros", [0, 0, 0]),
    ("none", []),
]


def test_the_factors_are_distinct_and_formed_in_double():
    """a factor of its own per segment, so that a wrong segment lookup shows.  For p = 0.3 and 0.9 a product carried in
    float32 happens to round to the same s^2 and s^3 as the double product cast once; for p = 0.1 the cubes differ in the
    last bit (1.3717422 against 1.3717424): the pool holds the double one"""
    assert len(set(float(f) for f in FACTORS)) == len(FACTORS) > 8
    for p in (0.1, 0.3, 0.9):
        assert _step_factor(p, 1) == dropout_ref.scale(p)
    s = dropout_ref.scale(0.1)
    assert np.float32(np.float32(s * s) * s) != _step_factor(0.1, 3)


@pytest.mark.parametrize("case", range(len(SCALE_CASES)), ids=[c[0] for c in SCALE_CASES])
def test_scale_segments_is_one_float32_product_per_element(lib, case):
    from cslicer import aggr
    lengths = SCALE_CASES[case][1]
    rng = np.random.default_rng(len(lengths) * 1000003 + sum(lengths))
    k = len(lengths)
    offs, at = [], 1
    for ln in lengths:          # odd offsets, gaps of sentinels between the segments and after the last
        at += 1 - at % 2
        offs.append(at)
        at += ln + int(rng.integers(1, 8))
    total = at + 9
    buf0 = np.full(total, SENT, dtype=np.float32)
    fac = [FACTORS[(j + case) % len(FACTORS)] for j in range(k)]       # a factor of its own per segment
    for o, ln in zip(offs, lengths):       # magnitudes in [0.5, 2): every product (twice over) stays normal
        buf0[o:o + ln] = ((0.5 + 1.5 * rng.random(ln)) * rng.choice([-1.0, 1.0], size=ln)).astype(np.float32)
    buf = torch.from_numpy(buf0).cuda()
    base = buf.data_ptr()
    # (a segment without elements may come with or without a pointer)
    seg = (C.c_void_p * max(k, 1))(*[base + 4 * o if ln or j % 2 else None for j, (o, ln) in enumerate(zip(offs, lengths))])
    cnt = (C.c_int64 * max(k, 1))(*lengths)
    fa = (C.c_float * max(k, 1))(*[float(f) for f in fac])
    want = buf0.copy()
    for call in (1, 2):         # the second call applies the factors again: nothing is kept between calls
        if k:
            rc = lib.csl_scale_segments_f32(k, seg, cnt, fa, aggr._stream())
        else:
            rc = lib.csl_scale_segments_f32(0, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), aggr._stream())
        assert rc == 0
        for o, ln, f in zip(offs, lengths, fac):
            want[o:o + ln] = want[o:o + ln] * f
        assert bool(np.isfinite(want).all()) and (not sum(lengths) or float(np.abs(want).min()) > 1e-30)
        _same(buf.cpu().numpy(), want, "call %d, lengths %s" % (call, lengths))
    assert not sum(lengths) or not np.array_equal(want, buf0)


# ---- C. the dropped native step against float64 on the oracle's traversal ---------------------------------------------------

N, F0, HIDDEN, BATCH = 20000, 12, 24, 200          # tests/test_gpu_sage_step.py
SEED, STEP = (5 << 32) | 4242, (1 << 32) + 3
EPS = 0.1


@functools.lru_cache(maxsize=None)
def _graph(kind):
    import test_gpu_sage_step as S
    return S._graph(kind, N)


@functools.lru_cache(maxsize=None)
def _feats(F):
    return np.random.default_rng(7 + F).standard_normal((N, F)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _labels(classes):
    return np.random.default_rng(70 + classes).integers(0, classes, size=N).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _multi_labels(classes):
    return np.random.default_rng(700 + classes).random((N, classes)) < 0.3


@functools.lru_cache(maxsize=None)
def _seeds(B):
    return np.random.default_rng(11).permutation(N)[:B]


@functools.lru_cache(maxsize=None)
def _traversal(kind, fan, B):
    from oracle import oracle as orc
    indptr, indices = _graph(kind)
    return orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(_seeds(B))


def _model(L, classes, F=F0, hidden=HIDDEN):
    from cslicer import splitgnn
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(F, hidden, classes, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    return model


def _params(model):
    return [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]


def _native(model, kind, fan, B, row_pad, n_slabs, labels, scale, runs):
    """[(loss, flat gradients)] of the native step for every run = (feature table, DropSpec or None, LossSpec or None), all
    on ONE engine's first sample (a fresh SageStep each, two calls: the second runs on the recorded GEMM plans and the
    reused workspace).  The sample is the oracle's: every frontier's size is checked."""
    from cslicer import _abi, aggr, splitgnn
    L = len(fan)
    indptr, indices = _graph(kind)
    trav = _traversal(kind, fan, B)
    eng = _abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=B, mode=_abi.MODE_GRAPH, flags=_abi.FLAG_TRANSPOSE)
    try:
        eng.submit_seeds([_seeds(B)])
        slices = splitgnn.slices_of(eng)
        order = [slices[L - 1 - k][0] for k in range(L)]
        if kind == "hub":
            assert max(s.t_max_len for s in order[1:]) > _abi.T_SORTED_MAX
        assert int(slices[0][0].n_out) == B
        for l in range(L):
            assert int(slices[l][0].n_out) == len(trav["frontier"][l]) and int(slices[l][0].n_in) == len(trav["frontier"][l + 1])
        outs = []
        for feat, drop, spec in runs:
            step = aggr.SageStep(model, row_pad, n_slabs)
            loss = torch.zeros(1, device="cuda")
            for _ in range(2):
                step(order, feat, labels, scale, loss, drop, loss=spec)
            torch.cuda.synchronize()
            outs.append((float(loss[0]), step.grads.clone()))
        return outs
    finally:
        eng.close()


def _assert_close(group, got_loss, got_grads, want_loss, want):
    """the rule of DESIGN 4.2; prints every error over its bound and the largest of them"""
    got_grads = got_grads.double().cpu()
    worst = abs(got_loss - want_loss) / (1e-5 * abs(want_loss))
    print("[%s] loss %.9g (float64 %.9g): error / bound %.3g" % (group, got_loss, want_loss, worst))
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    at = 0
    for k, g in enumerate(want):
        seg = got_grads[at:at + g.numel()].reshape(g.shape)
        at += g.numel()
        err, ref = float((seg - g).abs().max()), float(g.abs().max())
        assert ref > 0
        print("[%s] gradient %d: max error %.3g, largest entry %.3g: error / bound %.3g" % (group, k, err, ref, err / (1e-4 * ref)))
        worst = max(worst, err / (1e-4 * ref))
        assert err <= 1e-4 * ref, "gradient %d (%s of layer %d): max error %.3g against a largest entry of %.3g" % (
            k, "weight" if k % 2 == 0 else "bias", k // 2, err, ref)
    assert at == got_grads.numel()
    print("[%s] largest error / bound %.3g" % (group, worst))


# (L, fan, classes, row_pad, n_slabs, graph, fused deepest layer, p)
MATRIX = [
    (4, (4, 3, 3, 2), 9, 64, 2, "random", True, 0.3),       # CSL_MAX_LAYERS: s, s^2, s^3
    (4, (4, 3, 3, 2), 9, 64, 2, "random", False, 0.9),      # ... of 10.000001f
    (2, (6, 4), 7, 0, 4, "random", True, 0.9),              # no row padding
    (2, (6, 4), 7, 64, 3, "random", False, 0.3),            # 3 slabs do not divide every layer's rows
    (2, (6, 4), 7, 512, 8, "random", True, 0.1),            # the top layer is shorter than row_pad
    (2, (8, 6), 300, 0, 1, "hub", False, 0.1),              # hub lists by source, more than 256 classes, one slab
    (2, (8, 6), 7, 64, 4, "hub", True, 0.3),
    (3, (6, 4, 3), 300, 64, 4, "random", True, 0.7),
]


@pytest.mark.parametrize("L,fan,classes,row_pad,n_slabs,graph,fused,p", MATRIX)
def test_dropped_step_matches_float64_with_the_same_masks(L, fan, classes, row_pad, n_slabs, graph, fused, p, monkeypatch):
    from cslicer import aggr
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    assert aggr._lib().csl_sage_fwd_mfma_scratch(F0, HIDDEN) > 0        # these widths are the fused layer's
    feats, labels = _feats(F0), _labels(classes)
    model = _model(L, classes)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    (got_loss, got), (plain_loss, _) = _native(model, graph, fan, BATCH, row_pad, n_slabs, lab, 1.0 / BATCH,
                                               [(x, aggr.DropSpec(p, SEED, STEP), None), (x, None, None)])
    want_loss, want = dropout_ref.model_on_traversal(_traversal(graph, fan, BATCH), feats, labels, *_params(model), N, p,
                                                     SEED, STEP)
    _assert_close("sequencer", got_loss, got, want_loss, want)
    # and it IS dropout: the step without it is another loss
    assert abs(plain_loss - want_loss) > 1e-4 * abs(plain_loss)


BENCH = dict(F=100, hidden=256, classes=47, fan=(3, 3, 2), B=64)


def _bench_case():
    from cslicer import splitgnn
    b = BENCH
    model = _model(3, b["classes"], b["F"], b["hidden"])
    x = torch.from_numpy(_feats(b["F"])).cuda()
    lab = torch.from_numpy(_labels(b["classes"])).cuda()
    assert model.convs[1].fc.weight.numel() == 131072 and model.convs[0].fc.weight.numel() == 51200
    return model, x, lab, ("random", b["fan"], b["B"], splitgnn.ROW_PAD, splitgnn.SPLIT_K, lab, 1.0 / b["B"])


def test_dropped_step_at_the_bench_widths():
    """features 100, hidden 256, 47 classes, the trainer's ROW_PAD and SPLIT_K: the scaling launch covers weight-gradient
    segments of 131,072 and 51,200 floats"""
    from cslicer import aggr
    b = BENCH
    model, x, lab, args = _bench_case()
    (got_loss, got), (plain_loss, _) = _native(model, *args, [(x, aggr.DropSpec(0.3, SEED, STEP), None), (x, None, None)])
    want_loss, want = dropout_ref.model_on_traversal(_traversal("random", b["fan"], b["B"]), _feats(b["F"]),
                                                     _labels(b["classes"]), *_params(model), N, 0.3, SEED, STEP)
    _assert_close("bench widths", got_loss, got, want_loss, want)
    assert abs(plain_loss - want_loss) > 1e-4 * abs(plain_loss)


L4 = (4, (4, 3, 3, 2), 9, 64, 2)         # the first row of MATRIX


def test_ce_step_with_weights_and_smoothing_at_four_layers():
    import loss_ref
    from cslicer import aggr
    L, fan, classes, row_pad, n_slabs = L4
    feats, labels = _feats(F0), _labels(classes)
    model = _model(L, classes)
    x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
    w = (0.2 + 2.8 * np.random.default_rng(100 + classes).random(classes)).astype(np.float32)
    spec = aggr.LossSpec(torch.from_numpy(w).cuda(), EPS)
    drop = aggr.DropSpec(0.3, SEED, STEP)
    (got_loss, got), (unweighted, _) = _native(model, "random", fan, BATCH, row_pad, n_slabs, lab, 1.0 / BATCH,
                                               [(x, drop, spec), (x, drop, None)])
    want_loss, want = loss_ref.model_on_traversal(_traversal("random", fan, BATCH), feats, labels, *_params(model), N, w, EPS,
                                                  (0.3, SEED, STEP))
    _assert_close("cross-entropy options", got_loss, got, want_loss, want)
    assert abs(unweighted - want_loss) > 1e-4 * abs(unweighted)        # (the options are live)


def test_multilabel_step_at_four_layers():
    import bce_ref
    from cslicer import aggr
    L, fan, classes, row_pad, n_slabs = L4
    feats, y = _feats(F0), _multi_labels(classes)
    model = _model(L, classes)
    x, words = torch.from_numpy(feats).cuda(), torch.from_numpy(aggr.pack_labels(y)).cuda()
    (got_loss, got), (plain_loss, _) = _native(model, "random", fan, BATCH, row_pad, n_slabs, words, 1.0 / (BATCH * classes),
                                               [(x, aggr.DropSpec(0.3, SEED, STEP), None), (x, None, None)])
    want_loss, want = bce_ref.model_on_traversal(_traversal("random", fan, BATCH), feats, y, *_params(model), N,
                                                 drop=(0.3, SEED, STEP))
    _assert_close("multi-label", got_loss, got, want_loss, want)
    assert abs(plain_loss - want_loss) > 1e-4 * abs(plain_loss)


@pytest.mark.parametrize("case", ["four-layers", "bench-widths"])
def test_threshold_zero_and_unit_scale_is_the_plain_step_bit_for_bit(case):
    """p = 2^-33: every element is kept and s, s^2, s^3 are 1.0f -- dropout adds nothing but the mask and the factors"""
    from cslicer import aggr
    assert dropout_ref.threshold(P_LO) == 0 and dropout_ref.scale(P_LO) == np.float32(1)
    if case == "bench-widths":
        model, x, lab, args = _bench_case()
    else:
        L, fan, classes, row_pad, n_slabs = L4
        model = _model(L, classes)
        x, lab = torch.from_numpy(_feats(F0)).cuda(), torch.from_numpy(_labels(classes)).cuda()
        args = ("random", fan, BATCH, row_pad, n_slabs, lab, 1.0 / BATCH)
    a, b = _native(model, *args, [(x, aggr.DropSpec(P_LO, SEED, STEP), None), (x, None, None)])
    assert a[0] == b[0] and np.isfinite(a[0]) and a[0] > 0
    assert torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_16_bit_table_is_its_float32_upcast_at_four_layers(dtype):
    from cslicer import aggr
    L, fan, classes, row_pad, n_slabs = L4
    model = _model(L, classes)
    t16 = torch.from_numpy(_feats(F0)).to(dtype).cuda()
    lab = torch.from_numpy(_labels(classes)).cuda()
    drop = aggr.DropSpec(0.3, SEED, STEP)
    a, b = _native(model, "random", fan, BATCH, row_pad, n_slabs, lab, 1.0 / BATCH, [(t16, drop, None), (t16.float(), drop, None)])
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and bool(a[1].abs().sum() > 0)


# ---- D. the trainer ---------------------------------------------------------------------------------------------------------

def test_native_step_against_the_autograd_step_at_dropout_0_3(monkeypatch):
    """tests/test_gpu_dropout.py's comparison (same minibatch, same weights, same masks: csl_sage_fwd_bwd_dropout against
    CSLICER_PY_STEP=1, splitgnn._SageModelLocal with torch's GEMMs) at a scale that is no power of two"""
    import test_gpu_dropout as D
    t = D._trainer(dropout=0.3)
    try:
        assert t.native is not None
        loss_n = t.run(1)[0]
        grads_n = t.native.grads.clone()
    finally:
        t.close()
    monkeypatch.setenv("CSLICER_PY_STEP", "1")
    t = D._trainer(dropout=0.3)
    try:
        assert t.native is None and t.plan.path == "local"
        loss_p = t.run(1)[0]
        want = []
        for conv in t.model.convs:
            want += [conv.fc.weight.grad.double().cpu(), conv.fc.bias.grad.double().cpu()]
    finally:
        t.close()
    _assert_close("trainer", loss_n, grads_n, loss_p, want)
