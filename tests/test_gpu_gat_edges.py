"""The attention kernels against float64 (tests/gat_ref.py) at their dispatch edges and on data that stresses their
numerics: every instance of the input layer's edge kernels (csl_gat_in_fwd_f32 / _bwd_f32: H x the ME edges a row may
have), rows of 0, 1 and exactly ME edges, the grid-stride walk past 6,144 rows, destinations without a self row, the
fp32-MFMA projection and the library GEMMs; the partial aggregation (csl_gat_fwd_f32 / csl_gat_bwd_f32) on both sides of
its 16-edge fast path and its 256-column chunks; the layer's three backward forms (by source with the logits folded in,
by source, atomic); scores of about +-120 (no max subtraction: inf / NaN), rows whose sources are all equal, slopes 0,
0.01, 0.2 and 1 with scores of both signs.

Tolerances: outputs within 1e-5 of the row's largest entry, gradients within 1e-4 of the tensor's largest entry, except
where a test says why not."""
import numpy as np
import pytest
import torch

import gat_ref

pytestmark = pytest.mark.gpu

SLOPES = (0.0, 0.01, 0.2, 1.0)
BIG = 120.0     # largest |score|: exp overflows fp32 above 88, underflows below -103


@pytest.fixture(scope="module")
def mods():
    from cslicer import _abi, aggr, splitgnn
    _abi.load()
    return _abi, aggr, splitgnn


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32, device="cuda")


def _graph(rng, n_rows, n_src, max_deg, extra=()):
    """A CSR of n_rows destinations over n_src sources with degrees in [0, max_deg]: the first rows have 0, 1 and
    max_deg edges, so does the last one (max_deg) and every seventh row; every 13th row has ONE source on all its edges
    (alpha = 1 / deg exactly); every sixth destination has no self row (self id -1).  extra: degrees of the last rows
    (dispatch edges beyond max_deg)."""
    deg = rng.integers(0, max_deg + 1, size=n_rows)
    deg[2::7] = max_deg
    deg[:3] = [0, 1, max_deg][:n_rows]
    deg[-1] = max_deg
    if len(extra):
        deg[-len(extra):] = extra
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n_src, size=int(indptr[-1]))
    for r in range(4, n_rows, 13):
        indices[indptr[r]:indptr[r + 1]] = indices[indptr[r]] if deg[r] else 0
    self_ids = rng.integers(0, n_src, size=n_rows)
    self_ids[1::6] = -1
    return _i32(indptr), _i32(indices), _i32(self_ids), deg


def _rows_close(got, want, tol, what):
    """|got - want| <= tol * (the row's largest |want|) row by row (rows of zeros: exact)"""
    assert got.shape == want.shape, what
    want = want.to(got.dtype) if want.dtype != torch.float64 else want
    g64 = got.double()
    assert bool(torch.isfinite(g64).all()), what + ": not finite at %s" % (torch.nonzero(~torch.isfinite(g64))[:5].tolist(),)
    err = (g64 - want).abs().amax(1)
    scale = want.abs().amax(1)
    bad = err > tol * scale
    assert not bool(bad.any()), "%s: rows %s, error %s, row scale %s" % (
        what, torch.nonzero(bad)[:5, 0].tolist(), err[bad][:5].tolist(), scale[bad][:5].tolist())


def _grad_close(got, want, tol, what, scale=None):
    """max |got - want| <= tol * max |want| over the tensor (or tol * scale)"""
    g64 = got.double()
    assert bool(torch.isfinite(g64).all()), what + ": not finite"
    err, scale = float((g64 - want).abs().max()), float(want.abs().max()) if scale is None else scale
    assert err <= tol * scale, "%s: max error %g, tensor scale %g" % (what, err, scale)


def _shift_scores(x, weight, al, ar, shift):
    """scores about `shift` + N(0, 2) without changing how the softmax spreads over a row's edges: feature 0 of every
    row becomes 1 and column 0 of W_h becomes shift (a_l + a_r) / |a_l + a_r|^2, so that el + er gains `shift` (a row
    without a self row gains the el part alone).  In place."""
    H, D = al.shape
    with torch.no_grad():
        t = al + ar
        x[:, 0] = 1.0
        weight[:, 0] = (shift * t / (t * t).sum(1, keepdim=True)).reshape(-1)


def _attn_grads_close(names, grads, ref_grads, tol, er_blind, what=""):
    """every gradient against float64.  er_blind: leaky' is constant over every row (slope 1, or all scores shifted to one
    side of 0), so a row's softmax does not see er (a constant of the row) and the gradient of attn_r is zero up to the
    rounding of its cancelling terms: it is measured against the scale of attn_l's"""
    ref = dict(zip(names, ref_grads))
    for name, g, r in zip(names, grads, ref_grads):
        scale = float(ref["attn_l"].abs().max()) if name == "attn_r" and er_blind else None
        _grad_close(g, r, tol, "grad %s%s" % (name, what), scale)


def _big(slope):
    """+120 (exp of an unshifted score overflows above 88), -120 at slope 1 (it underflows below -103)"""
    return -BIG if slope == 1.0 else BIG


# ---------------------------------------------------------------------------------------------------------------------
# the input layer (aggr.GatInputLayer) directly against float64

def _run_input_layer(aggr, table, rows, params, indptr, indices, self_ids, n_out, max_deg, slope, elu, w):
    weight, al, ar, bias = (p.detach().clone().requires_grad_() for p in params)
    out = aggr.GatInputLayer.apply(table, rows, weight, al, ar, bias, indptr, indices, self_ids, n_out,
                                   int(indices.numel()), max_deg, slope, elu, 0, False)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), [weight.grad, al.grad, ar.grad, bias.grad]


def _ref_input_layer(table, rows, params, indptr, indices, self_ids, slope, elu, w):
    p64 = [p.detach().double().requires_grad_() for p in params]
    out = gat_ref.input_layer(table.double(), rows, *p64, indptr, indices, self_ids, slope, elu)
    (out * w.double()).sum().backward()
    return out.detach(), [p.grad for p in p64]


def _input_case(aggr, H, D, F, n_out, max_deg, seed, shift=0.0, extra=()):
    rng = np.random.default_rng(seed)
    n_src = 2 * n_out + 50
    indptr, indices, self_ids, deg = _graph(rng, n_out, n_src, max_deg, extra)
    n_table = n_src + 97
    rows = _i32(rng.permutation(n_table)[:n_src])                     # source i is table row rows[i]
    torch.manual_seed(seed)
    table = torch.randn(n_table, F, device="cuda")
    weight = torch.randn(H * D, F, device="cuda") / F ** 0.5
    al, ar = torch.randn(H, D, device="cuda") / D ** 0.5, torch.randn(H, D, device="cuda") / D ** 0.5   # scores ~ N(0, 2)
    bias = 0.1 * torch.randn(H * D, device="cuda")
    if shift:
        _shift_scores(table, weight, al, ar, shift)
    w = torch.randn(n_out, H * D, device="cuda")
    return table, rows, (weight, al, ar, bias), indptr, indices, self_ids, deg, w


# (H, max_deg): every instance the host can pick -- ME = 32 for one head, 16 / 32 for two and four (switch at 16 / 17),
# 12 / 32 for eight (switch at 12 / 13) -- with rows of exactly ME edges where max_deg = ME; F across the MFMA
# projection's k-tile switches (64 / 68, 112 / 116) and the float4 lane limits (4, 128); n_out across the 768 x 8 = 6,144
# rows of one grid-stride pass
IN_CASES = [  # H, max_deg, F, n_out, D, elu, slope
    (1, 32, 4, 1, 64, True, 0.2),
    (1, 32, 116, 6145, 16, False, 0.01),
    (2, 16, 20, 8, 32, True, 0.2),
    (2, 17, 68, 6143, 64, False, 0.2),
    (2, 32, 128, 20011, 16, True, 0.0),
    (4, 16, 64, 20011, 32, True, 1.0),
    (4, 17, 112, 8, 64, False, 0.2),
    (4, 32, 4, 6145, 16, True, 0.2),
    (8, 12, 128, 6145, 32, True, 0.2),
    (8, 13, 116, 20011, 16, False, 0.2),
    (8, 32, 68, 6143, 32, True, 0.01),
]


@pytest.mark.parametrize("libgemm", [False, True], ids=["mfma", "libgemm"])
@pytest.mark.parametrize("H,max_deg,F,n_out,D,elu,slope", IN_CASES)
def test_input_layer_instances_against_float64(mods, H, max_deg, F, n_out, D, elu, slope, libgemm, monkeypatch):
    _, aggr, _ = mods
    if libgemm:
        monkeypatch.setenv("CSLICER_GAT_IN_LIBGEMM", "1")
    assert aggr.gat_input_ok(H, F, max_deg, D) and aggr._lib().csl_gat_in_proj_ok(H, F, D)
    table, rows, params, indptr, indices, self_ids, _, w = _input_case(aggr, H, D, F, n_out, max_deg, H * 1000 + F + n_out)
    out, grads = _run_input_layer(aggr, table, rows, params, indptr, indices, self_ids, n_out, max_deg, slope, elu, w)
    ref, ref_grads = _ref_input_layer(table, rows, params, indptr, indices, self_ids, slope, elu, w)
    _rows_close(out, ref, 1e-5, "out")
    _attn_grads_close(("weight", "attn_l", "attn_r", "bias"), grads, ref_grads, 1e-4, slope == 1.0)


@pytest.mark.parametrize("big", [False, True], ids=["scores-N(0,2)", "scores-120"])
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,max_deg", [(8, 12), (1, 32)])
def test_input_layer_numerics_against_float64(mods, H, max_deg, slope, big):
    """slopes with scores of both signs (leaky' and the sign bit the forward keeps in alpha for the backward), scores about
    +-120 (without the max subtraction exp overflows or underflows), rows whose sources are all one row (alpha = 1 / deg)"""
    _, aggr, _ = mods
    F, D, n_out = 36, 16, 700
    table, rows, params, indptr, indices, self_ids, _, w = _input_case(aggr, H, D, F, n_out, max_deg, 7 + H,
                                                                       shift=_big(slope) if big else 0.0)
    for elu in (False, True):
        out, grads = _run_input_layer(aggr, table, rows, params, indptr, indices, self_ids, n_out, max_deg, slope, elu, w)
        ref, ref_grads = _ref_input_layer(table, rows, params, indptr, indices, self_ids, slope, elu, w)
        # at |score| ~ 120 the fp32 logit (a dot product of F terms, one of them ~120) is off by a few 1e-6 in ABSOLUTE
        # terms, and exp turns that into the same RELATIVE error of every attention weight: 3e-5 there.  Gradients: the
        # shift is a column of W of ~60 (_shift_scores), and its partner in the chain rule, g_v[h, 0] = the sum over a
        # row's edges of d score, cancels to ~0 wherever leaky' is constant over the row: the fp32 rounding of the O(1)
        # terms, times 60, reaches 1e-4 of attn_l's gradient -- 1e-3 there
        _rows_close(out, ref, 3e-5 if big else 1e-5, "out (elu %s)" % elu)
        _attn_grads_close(("weight", "attn_l", "attn_r", "bias"), grads, ref_grads, 1e-3 if big else 1e-4,
                          big or slope == 1.0, " (elu %s)" % elu)


@pytest.mark.parametrize("H,max_deg", [(8, 12), (2, 16), (1, 32)])
def test_input_layer_rows_longer_than_max_deg_are_nan(mods, H, max_deg):
    """max_deg picks the kernel instance and the host does not read indptr: a row of ME + 1 edges under a max_deg of ME
    must come out NaN (with the attention gradients it feeds), never as a softmax over a subset of its edges.  Every other
    row is exact."""
    _, aggr, _ = mods
    F, D, n_out = 20, 16, 500
    long_rows = [max_deg + 1] * 3
    table, rows, params, indptr, indices, self_ids, deg, w = _input_case(aggr, H, D, F, n_out, max_deg, 31 + H,
                                                                         extra=long_rows)
    deg[250] = max_deg + 1                                               # one in the middle of the walk too
    indptr = _i32(np.concatenate([[0], np.cumsum(deg)]))
    indices = _i32(np.random.default_rng(5).integers(0, rows.numel(), size=int(deg.sum())))
    over = torch.as_tensor(deg > max_deg, device="cuda")
    assert int(over.sum()) == 4
    out, grads = _run_input_layer(aggr, table, rows, params, indptr, indices, self_ids, n_out, max_deg, 0.2, False, w)
    assert bool(torch.isnan(out[over]).all()) and not bool(torch.isnan(out[~over]).any())
    ref, ref_grads = _ref_input_layer(table, rows, params, indptr, indices, self_ids, 0.2, False, w)
    _rows_close(out[~over], ref[~over], 1e-5, "out of the rows within max_deg")
    for name, g in zip(("weight", "attn_l", "attn_r"), grads[:3]):
        assert bool(torch.isnan(g).all()), "grad " + name + " is not poisoned"
    _grad_close(grads[3], ref_grads[3], 1e-4, "grad bias")     # (the bias gradient does not pass the edges)


# ---------------------------------------------------------------------------------------------------------------------
# the partial aggregation (aggr.GatAggregate: csl_gat_fwd_f32 / csl_gat_bwd_f32, the atomic backward)

AGG_DEGREES = (0, 1, 15, 16, 17, 40)   # the fast path holds up to 16 edges


@pytest.mark.parametrize("big", [False, True], ids=["scores-N(0,2)", "scores-120"])
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,D", [(4, 16), (8, 48), (2, 256)])
def test_partial_aggregate_against_float64(mods, H, D, slope, big):
    """(m, s, n) and the gradients of el, er, z.  H x D = 64 fits one 256-column chunk of a wave (fast path up to 16
    edges, generic path above); 8 x 48 = 384 and 2 x 256 = 512 take two chunks (generic path only).  s and n are
    compared at the kernel's own stabiliser m (m itself against the float64 row maximum)."""
    _, aggr, _ = mods
    rng = np.random.default_rng(H * D)
    n_rows, n_src = 240, 300
    deg = np.resize(np.asarray(AGG_DEGREES), n_rows)
    indptr_np = np.concatenate([[0], np.cumsum(deg)])
    indices_np = rng.integers(0, n_src, size=int(deg.sum()))
    for r in range(5, n_rows, 11):                                   # every source of the row the same
        indices_np[indptr_np[r]:indptr_np[r + 1]] = indices_np[indptr_np[r]] if deg[r] else 0
    indptr, indices = _i32(indptr_np), _i32(indices_np)
    torch.manual_seed(H + D)
    el0, er0 = torch.randn(n_src, H, device="cuda"), torch.randn(n_rows, H, device="cuda")
    if big:
        er0 = er0 + _big(slope)
    z0 = torch.randn(n_src, H * D, device="cuda")
    gs, gn = torch.randn(n_rows, H, device="cuda"), torch.randn(n_rows, H * D, device="cuda")
    el, er, z = (t.clone().requires_grad_() for t in (el0, er0, z0))
    m, s, n = aggr.GatAggregate.apply(el, er, z, indptr, indices, n_rows, H, D, slope)
    ((s * gs).sum() + (n * gn).sum()).backward()
    l64 = [t.double().requires_grad_() for t in (el0, er0, z0)]
    m_ref, _, _ = gat_ref.partial_state(*l64, indptr, indices, H, D, slope)
    _, s_ref, n_ref = gat_ref.partial_state(*l64, indptr, indices, H, D, slope, m=m.double())
    ((s_ref * gs.double()).sum() + (n_ref * gn.double()).sum()).backward()
    torch.testing.assert_close(m.double(), m_ref, rtol=1e-6, atol=0)
    # (s and n at |score| ~ 120: the fp32 sum el + er carries half an ulp of 120, 3.8e-6, into every exp: 2e-5)
    tol = 2e-5 if big else 1e-5
    _rows_close(s, s_ref, tol, "s")
    _rows_close(n, n_ref, tol, "n")
    for name, g, t in zip(("el", "er", "z"), (el.grad, er.grad, z.grad), l64):
        _grad_close(g, t.grad, 1e-4, "grad " + name)


# ---------------------------------------------------------------------------------------------------------------------
# the whole layer (aggr.GatLayerLocal) and its three backward forms

def _by_source(indptr, indices, self_ids, n_src):
    """the slice by source as the engine emits it: per source u the destination rows of its edges (ascending), and a
    -1 entry for a destination whose self row u is (attention skips it)"""
    rows = gat_ref.csr_rows(indptr).cpu().numpy()
    src = indices.long().cpu().numpy()
    sid = self_ids.long().cpu().numpy()
    own = np.flatnonzero(sid >= 0)
    key_src = np.concatenate([src, sid[own]])
    key_dst = np.concatenate([rows, np.full(own.size, -1)])
    order = np.lexsort((key_dst, key_src))
    t_indptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(key_src, minlength=n_src), out=t_indptr[1:])
    return _i32(t_indptr), _i32(key_dst[order]), int(np.diff(t_indptr).max())


def _layer_case(rng, n_out, n_in, degrees, hub=0):
    deg = np.resize(np.asarray(degrees), n_out)
    indptr_np = np.concatenate([[0], np.cumsum(deg)])
    indices_np = rng.integers(0, n_in, size=int(deg.sum()))
    for r in range(5, n_out, 11):
        indices_np[indptr_np[r]:indptr_np[r + 1]] = indices_np[indptr_np[r]] if deg[r] else 0
    if hub:
        indices_np[indptr_np[1:-1][deg[1:] > 0][:hub]] = 3          # source 3 in `hub` rows: a hub's list
    self_ids = rng.permutation(n_in)[:n_out]        # (a source is the self row of one destination at most)
    self_ids[1::6] = -1
    return _i32(indptr_np), _i32(indices_np), _i32(self_ids)


LAYER_CASES = [  # mode, H, D, n_out, n_in, F_in
    ("fused", 4, 16, 240, 500, 24),          # H x D in one chunk
    ("fused", 2, 256, 240, 500, 20),         # two chunks
    ("nofold", 8, 48, 240, 500, 20),
    ("nofold", 4, 16, 240, 500, 24),
    ("atomic", 4, 16, 240, 500, 24),
    ("atomic", 2, 256, 240, 500, 20),
    ("hub", 4, 16, 600, 700, 24),            # a list longer than T_SORTED_MAX: the atomic form
    ("fused", 2, 16, 3000, 40000, 12),       # > 32,768 source rows: 32 rows per workgroup of k_gat_bwd_t2
    ("nofold", 2, 16, 3000, 40000, 12),
]


@pytest.mark.parametrize("big", [False, True], ids=["scores-N(0,2)", "scores-120"])
@pytest.mark.parametrize("mode,H,D,n_out,n_in,F_in", LAYER_CASES)
def test_local_layer_against_float64(mods, mode, H, D, n_out, n_in, F_in, big, monkeypatch):
    """output and every gradient (input, weight, attention, bias) of GatLayerLocal over rows of 0, 1, 15, 16, 17 and 40
    edges; each slope in turn, ELU on and off"""
    abi, aggr, _ = mods
    rng = np.random.default_rng(n_in + D)
    indptr, indices, self_ids = _layer_case(rng, n_out, n_in, AGG_DEGREES, hub=300 if mode == "hub" else 0)
    tptr, trow, t_max = _by_source(indptr, indices, self_ids, n_in)
    assert (t_max > abi.T_SORTED_MAX) == (mode == "hub")
    if mode == "nofold":
        monkeypatch.setenv("CSLICER_GAT_NO_FOLD", "1")
    by_source = mode != "atomic"
    torch.manual_seed(n_out + H)
    x0 = torch.randn(n_in, F_in, device="cuda")
    weight0 = torch.randn(H * D, F_in, device="cuda") / F_in ** 0.5
    al0, ar0 = torch.randn(H, D, device="cuda") / D ** 0.5, torch.randn(H, D, device="cuda") / D ** 0.5   # scores ~ N(0, 2)
    bias0 = 0.1 * torch.randn(H * D, device="cuda")
    w = torch.randn(n_out, H * D, device="cuda")
    for k, slope in enumerate(SLOPES):
        elu = k % 2 == 1
        if big:
            _shift_scores(x0, weight0, al0, ar0, _big(slope))
        leaves = [t.clone().requires_grad_() for t in (x0, weight0, al0, ar0, bias0)]
        x, weight, al, ar, bias = leaves
        out = aggr.GatLayerLocal.apply(x, weight, al, ar, bias, indptr, indices, self_ids, n_out, slope, elu, 0,
                                       lambda gz, xp: gz.t() @ xp, tptr if by_source else None,
                                       trow if by_source else None, t_max)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        l64 = [t.double().requires_grad_() for t in (x0, weight0, al0, ar0, bias0)]
        ref = gat_ref.layer(*l64, indptr, indices, self_ids, slope, elu)
        (ref * w.double()).sum().backward()
        what = "slope %g, elu %s" % (slope, elu)
        # (at |score| ~ 120: 3e-5 for the reasons given in test_input_layer_numerics_against_float64; gradients 5e-3: the
        # same cancelling sums as there, which the atomic form adds in a varying order -- the hub's attn_l gradient has
        # come out 1.3e-3 off)
        _rows_close(out.detach(), ref.detach(), 3e-5 if big else 1e-5, "out, " + what)
        _attn_grads_close(("x", "weight", "attn_l", "attn_r", "bias"), [t.grad for t in leaves], [t.grad for t in l64],
                          5e-3 if big else 1e-4, big or slope == 1.0, ", " + what)


# ---------------------------------------------------------------------------------------------------------------------
# wider than the input layer's backward covers: the model falls back to the gathered input

def test_model_with_eight_heads_of_64_on_the_feature_table(mods):
    """DistGATModel(100, 64, C, heads=8) on aggr.FeatureRows: H x D = 512 > 256, which the input layer's backward
    epilogue (csl_elu_bwd_colsum_f32) refuses.  The layer must not be chosen (it ran forward, then raised in backward);
    one step's loss and gradients match the model on the gathered input and the float64 definition."""
    abi, aggr, sg = mods
    from cslicer import l0
    from oracle import oracle as orc
    from test_gpu_gat import _dense_gat_vectorised
    import copy
    torch.manual_seed(3)
    n, F0, hidden, classes, B, heads, fan = 20_000, 100, 64, 7, 128, 8, (10, 10)
    assert not aggr.gat_input_ok(heads, F0, fan[-1], hidden)
    indptr, indices = l0.synth_graph(n, 12.0, seed=3)
    seeds = np.random.default_rng(5).permutation(n)[:B]
    feats = torch.randn(n, F0, device="cuda")
    labels = torch.from_numpy(np.random.default_rng(6).integers(0, classes, size=n)).cuda()
    model = sg.DistGATModel(F0, hidden, classes, heads=heads, n_layers=2).cuda()
    with torch.no_grad():
        for conv in model.convs:
            conv.bias.normal_(0, 0.1)
    seeds_t = torch.from_numpy(seeds).cuda()
    res = []
    for table in (True, False):
        eng = abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=B, mode=abi.MODE_GRAPH,
                         flags=abi.FLAG_TRANSPOSE | (0 if table else abi.FLAG_TRANSPOSE_ALL))
        eng.submit_seeds([seeds])
        slices = sg.slices_of(eng)
        deep = slices[1][0]
        model.zero_grad()
        x = aggr.FeatureRows(feats, deep.in_nodes) if table else feats[deep.in_nodes.long()]
        out = model.forward_parts(slices, {0: x})[0]
        loss = torch.nn.functional.cross_entropy(out, labels[seeds_t], reduction="sum") / B
        loss.backward()
        torch.cuda.synchronize()
        res.append((float(loss), out.detach().clone(), [p.grad.clone() for p in model.parameters()]))
        eng.close()
    model64 = copy.deepcopy(model).double()
    model64.zero_grad()
    trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
    ref = _dense_gat_vectorised(model64, trav, feats.double())[seeds_t]
    loss64 = torch.nn.functional.cross_entropy(ref, labels[seeds_t], reduction="sum") / B
    loss64.backward()
    for loss, out, grads in res:
        assert abs(loss - float(loss64)) <= 1e-5 * abs(float(loss64))
        _rows_close(out, ref.detach(), 1e-5, "logits")
        for (name, p_), g in zip(model64.named_parameters(), grads):
            _grad_close(g, p_.grad, 1e-4, "grad " + name)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-5 * float(res[1][1].abs().max()))
