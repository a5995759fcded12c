"""Dropout for the attention model (include/cslicer_gat_dropout.h) without a GPU: the attention mask's counter
layout pinned to dropout_ref.philox4x32_10 (itself held to Random123's known answers in test_dropout_cpu.py), the float64
restatement tests/gat_drop_ref.py against an explicit dense masked softmax, the trainer's refusals, step_plan's new
keywords and the command line."""
import numpy as np
import pytest
import torch

import dropout_ref
import gat_drop_ref
import gat_ref

F64 = torch.float64


# ---- the counter layout -----------------------------------------------------------------------------------------------------

def _word(u, v, h, layer, step, seed):
    """the head's result word, written out from the header's text with plain ints"""
    ctr = (u, v, 0x80000000 | ((h >> 2) << 8) | layer, step % (1 << 32))
    w = dropout_ref.philox4x32_10(ctr, (seed % (1 << 32), (seed >> 32) % (1 << 32)))
    return int(w[h & 3])


def test_attention_counter_layout():
    """ctr = (u, v, 0x80000000 | (h >> 2) << 8 | k, t mod 2^32), word h & 3, key = the seed's halves: attn_keep_edges
    against the words computed one by one, over ids up to 2^31 - 1, heads past the first quad, a seed with a high word
    and a step beyond 2^32"""
    u = np.array([0, 1, 7, 2**31 - 1, 12345, 7])
    v = np.array([0, 7, 1, 2**31 - 2, 54321, 1])
    for H, p, seed, layer, step in ((1, 0.5, 1, 0, 0), (3, 0.25, 0x123456789ABCDEF, 2, 5), (8, 0.6, 2**63 + 11, 3, 2**32 + 9),
                                    (9, 0.9, 77, 1, 2**40)):
        keep = gat_drop_ref.attn_keep_edges(u, v, H, p, seed, layer, step)
        assert keep.shape == (u.size, H) and keep.dtype == np.bool_
        T = dropout_ref.threshold(p)
        for e in range(u.size):
            for h in range(H):
                assert bool(keep[e, h]) == (_word(int(u[e]), int(v[e]), h, layer, step, seed) >= T), (H, e, h)
    # the direction matters, the step is taken mod 2^32, the layer and the seed's high word are part of the key
    a = gat_drop_ref.attn_keep_edges(u, v, 8, 0.5, 5, 1, 3)
    assert not np.array_equal(a, gat_drop_ref.attn_keep_edges(v, u, 8, 0.5, 5, 1, 3))
    assert np.array_equal(a, gat_drop_ref.attn_keep_edges(u, v, 8, 0.5, 5, 1, 3 + 2**32))
    assert not np.array_equal(a, gat_drop_ref.attn_keep_edges(u, v, 8, 0.5, 5, 2, 3))
    assert not np.array_equal(a, gat_drop_ref.attn_keep_edges(u, v, 8, 0.5, 5 + 2**32, 1, 3))
    assert np.array_equal(a[2], a[5])          # two copies of one edge (u, v): one draw


def _small_csr():
    rng = np.random.default_rng(11)
    deg = np.array([0, 1, 16, 17, 3, 5, 2, 9])
    indptr = np.concatenate([[0], np.cumsum(deg)])
    indices = rng.integers(0, 40, size=int(deg.sum()))
    src_ids = rng.permutation(100000)[:40] + 2**30
    dst_ids = rng.permutation(100000)[:8] + 5
    return indptr, indices, src_ids, dst_ids


KEPT_PAIRS = 176    # of 53 edges x 8 heads = 424 at p = 0.6: 41.5 % (expected 40 %)


def test_recorded_count_of_kept_pairs():
    """one end-to-end number: _small_csr's 53 edges, 8 heads, p = 0.6, seed 0x5EED00000007, layer 1, step 3"""
    indptr, indices, src_ids, dst_ids = _small_csr()
    keep = gat_drop_ref.attn_keep(src_ids, dst_ids, indptr, indices, 8, 0.6, 0x5EED00000007, 1, 3)
    assert keep.shape == (53, 8)
    assert int(keep.sum()) == KEPT_PAIRS


def test_counter_spaces_are_disjoint():
    """the feature mask's third counter word is the layer number, below CSL_MAX_LAYERS; the attention mask's has bit 31 set
    and carries the layer in its low 8 bits, the head quad above them: no (layer, head) collides with a layer, and distinct
    (layer, head quad) pairs give distinct words"""
    from cslicer import _abi
    assert _abi.MAX_LAYERS <= 256
    feature_words = set(range(_abi.MAX_LAYERS))
    seen = {}
    for k in range(_abi.MAX_LAYERS):
        for h in (0, 3, 4, 7, 8, 255, 256, 2**16):
            ctr, word = gat_drop_ref.attn_counter(1, 2, h, k, 0)
            w2 = int(ctr[2])
            assert w2 not in feature_words and w2 >> 31 == 1 and w2 < 2**32
            assert seen.setdefault(w2, (k, h >> 2)) == (k, h >> 2)
            assert int(word) == h & 3


# ---- the float64 restatement -------------------------------------------------------------------------------------------------

def _layer_inputs(H, D, seed=3):
    indptr, indices, src_ids, dst_ids = _small_csr()
    g = torch.Generator().manual_seed(seed)
    n_src, n_out, Fin = 40, indptr.size - 1, 6
    x = torch.randn(n_src, Fin, dtype=F64, generator=g)
    weight = torch.randn(H * D, Fin, dtype=F64, generator=g) / Fin ** 0.5
    al, ar = torch.randn(H, D, dtype=F64, generator=g) / D ** 0.5, torch.randn(H, D, dtype=F64, generator=g) / D ** 0.5
    bias = 0.1 * torch.randn(H * D, dtype=F64, generator=g)
    self_ids = torch.tensor([3, -1, 5, 7, 9, -1, 11, 13])
    return (x, weight, al, ar, bias), torch.as_tensor(indptr), torch.as_tensor(indices), self_ids, src_ids, dst_ids, n_out


def test_layer_drop_without_dropout_is_the_layer():
    params, indptr, indices, self_ids, src_ids, dst_ids, _ = _layer_inputs(3, 4)
    for elu in (False, True):
        a = gat_drop_ref.layer_drop(*params, indptr, indices, self_ids, 0.2, elu, src_ids, dst_ids, 0.0, 0.0, 1, 0, 0)
        assert torch.equal(a, gat_ref.layer(*params, indptr, indices, self_ids, 0.2, elu))


def _dense_layer(params, indptr, indices, self_ids, src_ids, dst_ids, slope, elu, p_f, p_a, seed, layer, step):
    """the same layer through a dense [n_out, n_src, H] masked softmax: alpha = cnt exp(score) / sum cnt exp(score) with
    cnt the edge multiplicities, then kappa (one value per (u, v, h): copies of an edge share it) on alpha"""
    x, weight, al, ar, bias = params
    H, D = al.shape
    n_src, n_out = x.shape[0], indptr.numel() - 1
    z = (x @ weight.t()).view(n_src, H, D)
    el, er_all = (z * al).sum(-1), (z * ar).sum(-1)
    er = torch.where((self_ids >= 0)[:, None], er_all[self_ids.clamp_min(0)], torch.zeros(1, H, dtype=F64))
    cnt = torch.zeros(n_out, n_src, dtype=F64)
    rows = gat_ref.csr_rows(indptr)
    cnt.index_put_((rows, indices.long()), torch.ones(indices.numel(), dtype=F64), accumulate=True)
    score = torch.nn.functional.leaky_relu(el[None, :, :] + er[:, None, :], slope)              # [n_out, n_src, H]
    w = cnt[:, :, None] * torch.exp(score - score.detach().amax(1, keepdim=True))
    alpha = w / w.sum(1, keepdim=True).clamp_min(1e-300)
    if p_a > 0:
        uu, vv = np.meshgrid(np.asarray(src_ids), np.asarray(dst_ids))                         # [n_out, n_src]
        keep = gat_drop_ref.attn_keep_edges(uu.reshape(-1), vv.reshape(-1), H, p_a, seed, layer, step)
        alpha = alpha * torch.as_tensor(keep.reshape(n_out, n_src, H)).to(F64) * float(dropout_ref.scale(p_a))
    out = torch.einsum("ruh,uhd->rhd", alpha, z).reshape(n_out, H * D) + bias
    if elu:
        out = torch.nn.functional.elu(out)
    if p_f > 0:
        keep = dropout_ref.keep_mask(dst_ids, H * D, p_f, seed, layer, step)
        out = out * torch.as_tensor(keep).to(F64) * float(dropout_ref.scale(p_f))
    return out


@pytest.mark.parametrize("H,D", [(1, 4), (3, 8), (8, 4)])
@pytest.mark.parametrize("p_f,p_a", [(0.0, 0.5), (0.5, 0.0), (0.6, 0.6)])
def test_layer_drop_against_a_dense_masked_softmax(H, D, p_f, p_a):
    """output and every gradient, ELU on (the feature mask follows it) and off; the CSR has rows of 0, 1, 16 and 17 edges
    and repeated edges (53 draws out of 40 sources)"""
    params, indptr, indices, self_ids, src_ids, dst_ids, n_out = _layer_inputs(H, D)
    w = torch.randn(n_out, H * D, dtype=F64, generator=torch.Generator().manual_seed(9))
    for elu in (True, False):
        res = []
        for fn in ("ref", "dense"):
            leaves = [t.clone().requires_grad_() for t in params]
            if fn == "ref":
                out = gat_drop_ref.layer_drop(*leaves, indptr, indices, self_ids, 0.2, elu, src_ids, dst_ids, p_f, p_a,
                                              0xABCD00001234, 2, 7)
            else:
                out = _dense_layer(leaves, indptr, indices, self_ids, src_ids, dst_ids, 0.2, elu, p_f, p_a, 0xABCD00001234, 2, 7)
            (out * w).sum().backward()
            res.append([out.detach()] + [t.grad for t in leaves])
        for a, b in zip(*res):
            torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-12)
    if p_a > 0:   # a row whose edges are all dropped for a head yields act(bias) there: row 1 has one edge
        keep = gat_drop_ref.attn_keep(src_ids, dst_ids, indptr, indices, H, p_a, 0xABCD00001234, 2, 7)
        out = gat_drop_ref.layer_drop(*params, indptr, indices, self_ids, 0.2, False, src_ids, dst_ids, 0.0, p_a,
                                      0xABCD00001234, 2, 7)
        for h in range(H):
            if not keep[0, h]:       # (edge 0 is row 1's only edge)
                assert torch.equal(out[1, h * D:(h + 1) * D], params[4][h * D:(h + 1) * D])


# ---- step_plan ----------------------------------------------------------------------------------------------------------------

def test_step_plan_with_the_new_keywords():
    """step_plan_gat_drop (step_plan's own parameter list is pinned by test_loss_ref_cpu.py, so the two keywords live on a
    function beside it): at their defaults every tabulated plan is today's; attn_dropout > 0 turns the input layer off under gat_input=None
    (the plan that gat_input=False gives) and nowhere else; feat_dropout alone changes no row"""
    import test_step_plan_cpu as T
    from cslicer.train import Switches, step_plan
    from cslicer.train import step_plan_gat_drop as plan_drop
    moved = 0
    for row, change, flags, path, gat_input, input_form in T.ROWS:
        cfg = dict(T.BASE, **change)
        sw = Switches(**{k: cfg.pop(k) for k in Switches._fields})
        today = step_plan(sw=sw, **cfg)
        assert tuple(today) == (flags, path, gat_input, input_form), row
        assert plan_drop(sw=sw, feat_dropout=0.0, attn_dropout=0.0, **cfg) == today and plan_drop(sw=sw, **cfg) == today, row
        if cfg["kind"] != "gat":
            continue
        assert plan_drop(sw=sw, feat_dropout=0.6, **cfg) == today, row
        got = plan_drop(sw=sw, feat_dropout=0.6, attn_dropout=0.6, **cfg)
        if gat_input and cfg["gat_input"] is None:
            moved += 1
            assert not got.gat_input and got == step_plan(sw=sw, **dict(cfg, gat_input=False)), row
        else:
            assert got == today, row
    assert moved == 2       # rows 15 and 2515


# ---- the constructor and the command line ----------------------------------------------------------------------------------

def _tiny():
    indptr = np.arange(9, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, 8, size=16).astype(np.int64)
    return indptr, indices, np.zeros((8, 8), dtype=np.float32), np.zeros(8, dtype=np.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(model="gat", feat_dropout=1.0), r"feat_dropout must be in \[0, 1\)"),
    (dict(model="gat", feat_dropout=-0.1), r"feat_dropout must be in \[0, 1\)"),
    (dict(model="gat", attn_dropout=1.5), r"attn_dropout must be in \[0, 1\)"),
    (dict(model="gat", attn_dropout=float("nan")), r"attn_dropout must be in \[0, 1\)"),
    (dict(model="sage", feat_dropout=0.5), "model='gat'"),
    (dict(model="sage", attn_dropout=0.5), "model='gat'"),
    (dict(model="gat", attn_dropout=0.5, gat_input=True), "gat_input=True"),
    (dict(model="gat", dropout=0.5, feat_dropout=0.5), "attention model"),       # (`dropout` stays GraphSAGE's)
])
def test_constructor_refuses_before_any_device_call(kw, match, monkeypatch):
    from cslicer import train
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    indptr, indices, feats, labels = _tiny()
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, hidden=8, heads=2, **kw)


def test_constructor_accepts_the_arguments(monkeypatch):
    """valid values pass the argument checks (the first device call is where this test stops)"""
    from cslicer import train

    class Stop(Exception):
        pass

    def stop(*a):
        raise Stop()
    monkeypatch.setattr(torch.cuda, "set_device", stop)
    indptr, indices, feats, labels = _tiny()
    for kw in (dict(feat_dropout=0.6), dict(attn_dropout=0.6), dict(feat_dropout=0.0, attn_dropout=0.0),
               dict(attn_dropout=0.5, gat_input=False)):
        with pytest.raises(Stop):
            train.Trainer(indptr, indices, feats, labels, 3, fanouts=(2, 2), batch=4, streams=1, hidden=8, heads=2,
                          model="gat", **kw)


def test_command_line_reaches_the_constructor(monkeypatch):
    from cslicer import l0, train
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(train, "Trainer", fake)
    monkeypatch.setattr(l0, "synth_graph", lambda n, d, seed=0: _tiny()[:2])
    base = ["--graph", "synthetic", "--model-name", "gat", "--num-layers", "2", "--fan-out", "2,2"]
    for argv, want in ((["--feat-dropout", "0.6", "--attn-dropout", "0.25"], (0.6, 0.25)), (["--attn-dropout", "0.5"], (None, 0.5)),
                       ([], (None, None))):
        seen.clear()
        with pytest.raises(Stop):
            train.main(base + argv)
        assert (seen.get("feat_dropout"), seen.get("attn_dropout")) == want
        assert seen["model"] == "gat"
    doc = train.main.__doc__
    assert "--feat-dropout P, --attn-dropout P (extra)" in doc and "--feat-dropout 0.6 --attn-dropout 0.6" in doc
    ignored = doc.split("Accepted and ignored")[1].split("--eval-split")[0]
    assert "--feat-dropout" not in ignored and "--attn-dropout" not in ignored


def test_the_header_is_bound():
    """every entry point of cslicer_gat_dropout.h is bound from the header's text, and refuses p outside (0, 1), a layer
    outside [0, 256) and missing ids before any HIP call (no device here)"""
    import ctypes as C
    from cslicer import _abi
    L = _abi.load()
    names = _abi.BOUND["cslicer_gat_dropout.h"]
    assert names == ["csl_gat_drop_fwd_f32", "csl_gat_drop_bwd_f32", "csl_gat_drop_bwd_t_f32", "csl_gat_drop_bwd_t_fused_f32",
                     "csl_gat_finish_drop_fwd_f32", "csl_gat_finish_drop_bwd_f32"]
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) // 16 * 16
    x, nul = C.c_void_p(base), C.c_void_p(0)
    ok = dict(indptr=x, indices=x, n_rows=1, el=x, er=x, z=x, H=1, D=4, slope=0.2, m=x, s=x, n=x, src_ids=x, dst_ids=x, p=0.5,
              seed=1, layer=0, step=0, stream=nul)

    def fwd(**kw):
        return L.csl_gat_drop_fwd_f32(*dict(ok, **kw).values())
    for bad in (dict(p=0.0), dict(p=1.0), dict(p=-0.5), dict(p=float("nan")), dict(layer=-1), dict(layer=256), dict(src_ids=nul),
                dict(dst_ids=nul), dict(D=6), dict(D=260), dict(H=0), dict(n_rows=-1), dict(indptr=nul), dict(n=nul),
                dict(z=C.c_void_p(base + 4))):
        assert fwd(**bad) == -1, bad
    assert fwd(n_rows=0, src_ids=nul, dst_ids=nul, indptr=nul) == 0       # no rows: nothing to launch
    okb = dict(indptr=x, indices=x, n_rows=1, el=x, er=x, z=x, H=1, D=4, slope=0.2, m=x, gs=x, gn=x, gel=x, ger=x, gz=x,
               src_ids=x, dst_ids=x, p=0.5, seed=1, layer=0, step=0, stream=nul)
    for bad in (dict(p=0.0), dict(p=1.0), dict(layer=256), dict(src_ids=nul), dict(dst_ids=nul), dict(gz=C.c_void_p(base + 8))):
        assert L.csl_gat_drop_bwd_f32(*dict(okb, **bad).values()) == -1, bad
    okt = dict(tptr=x, trow=x, n_src=1, n_pad=1, el=x, er=x, z=x, H=1, D=4, slope=0.2, m=x, gs=x, gn=x, gel=x, ger=x, gz=x,
               src_ids=x, dst_ids=x, p=0.5, seed=1, layer=0, step=0, stream=nul)
    for bad in (dict(p=0.0), dict(p=1.0), dict(layer=-1), dict(src_ids=nul), dict(dst_ids=nul), dict(n_pad=0), dict(gz=nul)):
        assert L.csl_gat_drop_bwd_t_f32(*dict(okt, **bad).values()) == -1, bad
    okf = dict(tptr=x, trow=x, n_src=1, n_pad=1, el=x, er=x, z=x, H=1, D=4, slope=0.2, m=x, gs=x, gn=x, al=x, ar=x, sid=x,
               n_out=1, ger=x, gz=x, gal=x, gar=x, scratch=x, src_ids=x, dst_ids=x, p=0.5, seed=1, layer=0, step=0, stream=nul)
    for bad in (dict(p=0.0), dict(p=1.0), dict(layer=256), dict(src_ids=nul), dict(dst_ids=nul), dict(gal=nul), dict(scratch=nul),
                dict(ar=nul), dict(sid=nul)):
        assert L.csl_gat_drop_bwd_t_fused_f32(*dict(okf, **bad).values()) == -1, bad
    oke = dict(n_in=x, s_in=x, bias=x, n=1, H=1, D=4, elu=1, out=x, y=x, ids=x, p=0.5, seed=1, layer=0, step=0, stream=nul)
    for bad in (dict(p=0.0), dict(p=1.0), dict(p=float("nan")), dict(ids=nul), dict(y=nul), dict(out=nul), dict(D=6), dict(n=-1),
                dict(y=C.c_void_p(base + 4))):
        assert L.csl_gat_finish_drop_fwd_f32(*dict(oke, **bad).values()) == -1, bad
    assert L.csl_gat_finish_drop_fwd_f32(*dict(oke, n=0, ids=nul, y=nul).values()) == 0
    okg = dict(g=x, ldg=4, out=x, n_in=x, s_in=x, n=1, H=1, D=4, elu=1, g_n=x, g_s=x, g_bias=x, scratch=x, ids=x, p=0.5, seed=1,
               layer=0, step=0, stream=nul)
    for bad in (dict(p=0.0), dict(p=1.0), dict(ids=nul), dict(ldg=3), dict(ldg=6), dict(g_bias=nul), dict(out=nul), dict(g=nul)):
        assert L.csl_gat_finish_drop_bwd_f32(*dict(okg, **bad).values()) == -1, bad
