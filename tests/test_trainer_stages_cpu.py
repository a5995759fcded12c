"""The stages Trainer.__init__ is a sequence of, each called directly with no device: the argument checkers (an accepting
call and every refusal, matched on its message), the refusals that now come before any device call (an unknown model, a
bad workload), the host-row loading, and l0.feature_rows, which cslicer.train and cslicer.predict both load features.bin
through.  8 nodes, feature width 6 (no multiple of 4), 3 classes."""
import numpy as np
import pytest
import torch

from cslicer import _abi, aggr, l0, train

N, F, C = 8, 6, 3


def _refuses(fn, cases):
    for args, match in cases:
        with pytest.raises(ValueError, match=match):
            fn(*args)


def test_check_labels():
    y = np.arange(N * C).reshape(N, C) % 2
    assert train._check_labels(y, True, N, C) is True and train._check_labels(y.astype(bool), 1, N, C) is True
    assert train._check_labels(np.zeros(N, dtype=np.int64), False, N, C) is False
    assert train._check_labels(lambda own: None, True, N, C) is True         # (a callable's rows: checked when loaded)
    _refuses(train._check_labels, [
        ((np.zeros(N, dtype=np.int64), True, N, C), r"labels must be a matrix \[num_nodes, n_classes\] of 0 / 1, not shape \(8,\)"),
        ((y[:, :2], True, N, C), r"labels must be \[num_nodes = 8, n_classes = 3\], not \(8, 2\)"),
        ((y + 1, True, N, C), r"every label must be 0 or 1 \(bool or integer\)"),
        ((y.astype(np.float32), True, N, C), "every label must be 0 or 1"),
    ])


def test_check_dropouts():
    assert train._check_dropouts("sage", 8, 0.5, 0, 0.0, None) == (0.5, 0.0, 0.0)
    got = train._check_dropouts("gat", 6, 0, 0.6, 0.25, None)
    assert got == (0.0, 0.6, 0.25) and all(type(v) is float for v in got)
    assert train._check_dropouts("gat", 8, 0.0, 0.0, 0.5, False) == (0.0, 0.0, 0.5)
    _refuses(train._check_dropouts, [
        (("sage", 8, 1.0, 0.0, 0.0, None), r"dropout must be in \[0, 1\), not 1.0"),
        (("sage", 8, float("nan"), 0.0, 0.0, None), r"dropout must be in \[0, 1\), not nan"),
        (("gat", 8, 0.5, 0.0, 0.0, None), r"dropout > 0: the attention model has no dropout \(model='sage' only\)"),
        (("sage", 6, 0.5, 0.0, 0.0, None), r"dropout > 0: hidden must be a multiple of 4 .*, not 6"),
        (("gat", 8, 0.0, 1.0, 0.0, None), r"feat_dropout must be in \[0, 1\), not 1.0"),
        (("gat", 8, 0.0, 0.0, -0.1, None), r"attn_dropout must be in \[0, 1\), not -0.1"),
        (("sage", 8, 0.0, 0.5, 0.0, None), "feat_dropout > 0: GraphSAGE has `dropout`; feat_dropout / attn_dropout belong to model='gat'"),
        (("sage", 8, 0.0, 0.0, 0.5, None), "attn_dropout > 0: GraphSAGE has `dropout`"),
        (("gat", 8, 0.0, 0.0, 0.5, True), r"attn_dropout > 0 with gat_input=True: .* \(gat_input=None turns it off\)"),
        (("gat", 8, 0.5, 0.5, 0.0, None), "attention model has no dropout"),            # (the earlier check wins)
    ])


def test_check_optimizer():
    assert train._check_optimizer(0, None, None) == (0.0, None)
    assert train._check_optimizer(5e-4, "inf", lambda t: 0.1) == (5e-4, float("inf"))
    _refuses(train._check_optimizer, [
        ((-1e-3, None, None), "weight_decay must be >= 0, not -0.001"),
        ((float("nan"), None, None), "weight_decay must be >= 0, not nan"),
        ((0.0, 0.0, None), r"max_grad_norm must be None or > 0 \(float\('inf'\): .*\), not 0.0"),
        ((0.0, float("nan"), None), "max_grad_norm must be None or > 0"),
        ((0.0, None, 0.01), "lr_schedule must be None or a callable steps_done -> lr, not 0.01"),
    ])


def test_check_loss():
    assert train._check_loss(0, None, C, False) == (0.0, None) and train._check_loss(0.0, None, C, True) == (0.0, None)
    eps, w = train._check_loss(0.1, [1, 0, 2.5], C, False)
    assert eps == 0.1 and w.dtype == np.float64 and w.tolist() == [1.0, 0.0, 2.5]
    _refuses(train._check_loss, [
        ((1.0, None, C, False), r"label_smoothing must be in \[0, 1\), not 1.0"),
        ((float("nan"), None, C, False), r"label_smoothing must be in \[0, 1\), not nan"),
        ((0.0, [1.0, 2.0], C, False), "class_weight must be a sequence of n_classes = 3 numbers"),
        ((0.0, [[1.0, 2.0, 3.0]], C, False), "class_weight must be a sequence of n_classes = 3 numbers"),
        ((0.0, [1.0, -1.0, 1.0], C, False), "class_weight: finite numbers >= 0 with at least one > 0 expected"),
        ((0.0, [0.0, 0.0, 0.0], C, False), "class_weight: finite numbers >= 0 with at least one > 0"),
        ((0.0, [1.0, float("inf"), 1.0], C, False), "class_weight: finite numbers"),
        ((0.1, None, C, True), "multilabel=True: class_weight / label_smoothing belong to the single-label loss"),
        ((0.0, [1.0, 1.0, 1.0], C, True), "the sigmoid-BCE loss has no weights yet"),
    ])


def test_check_sampling():
    lim = _abi.noreplace_max_fanout()
    assert train._check_sampling(None, True, (lim + 1, 2), 16) is None
    assert train._check_sampling(None, False, (lim, 2), 16) is None
    w = train._check_sampling(np.ones(16, dtype=np.float32), True, (2, 2), 16)
    assert w.dtype == np.float64 and w.shape == (16,)
    _refuses(train._check_sampling, [
        ((np.ones(16), False, (2, 2), 16), r"edge_weight with replace=False: weighted sampling draws with replacement"),
        ((np.ones(16), False, (lim + 1,), 16), "edge_weight with replace=False"),          # (before the fanouts)
        ((np.ones(15), True, (2, 2), 16), r"edge weights have shape \(15,\), the graph has 16 edges"),
        ((-np.ones(16), True, (2, 2), 16), "edge weights must be finite and >= 0"),
        ((None, False, (2, lim + 1), 16), r"replace=False: fanouts \(2, %d\) exceed the limit of %d neighbours per row" % (lim + 1, lim)),
    ])


def test_check_table():
    for name, dt in (("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        assert train._check_table(name, None) is dt
    assert train._check_table("float16", True) is torch.float16 and train._check_table("float32", False) is torch.float32
    _refuses(train._check_table, [
        (("float64", None), "feature_dtype must be one of float32, float16, bfloat16, not 'float64'"),
        (("float32", 1), "gat_input must be None, True or False, not 1"),
        (("int8", "on"), "feature_dtype must be one of"),                                  # (the earlier check wins)
    ])


def test_check_gat_input_on():
    sw = train.Switches()
    ok = ("gat", 1, False, 2, 8, 8, C, 2, 2, sw)            # gat_input_obstacle's arguments: a shape the layer covers
    assert train.gat_input_obstacle(*ok) is None
    assert train._check_gat_input_on(True, *ok) is None
    bad = ("gat", 1, False, 2, F, 8, C, 2, 2, sw)           # F = 6: no multiple of 4
    for gat_input in (None, False):                         # only gat_input=True asks
        assert train._check_gat_input_on(gat_input, *bad) is None
    _refuses(train._check_gat_input_on, [
        ((True,) + bad, r"gat_input=True: aggr.gat_input_ok\(heads=2, F=6, fanout=2, D=8\) is false"),
        ((True, "sage") + ok[1:], "gat_input=True: model is 'sage', the input layer belongs to model='gat'"),
        ((True, "foo") + ok[1:], "gat_input=True: model is 'foo'"),
        ((True, "gat", 2) + ok[2:], "gat_input=True: more than one part or rank_path"),
        ((True,) + ok[:4] + (None,) + ok[5:], r"gat_input=True: the feature width is unknown \(pass feat_dim with callable features\)"),
        ((True,) + ok[:-1] + (train.Switches(no_gat_input=True),), "gat_input=True: CSLICER_GAT_NO_INPUT_LAYER is set"),
    ])


def test_check_workload_and_model():
    assert train._check_workload(None, N, 2) is None
    w = train._check_workload([0, 1] * 4, N, 2)
    assert w.dtype == np.int32 and w.flags.c_contiguous and w.tolist() == [0, 1] * 4
    msg = r"workload must be int32 \[num_nodes\] with values in \[0, world\)"
    _refuses(train._check_workload, [(([0, 1] * 3, N, 2), msg), (([0, 2] * 4, N, 2), msg), (([0, -1] * 4, N, 2), msg),
                                     ((np.zeros((N, 1)), N, 1), msg)])
    assert train._check_model("sage") is None and train._check_model("gat") is None
    _refuses(train._check_model, [(("foo",), "model must be 'sage' or 'gat'"), ((None,), "model must be 'sage' or 'gat'")])


def _tiny():
    indptr = np.arange(N + 1, dtype=np.int64) * 2
    indices = np.random.default_rng(0).integers(0, N, size=2 * N).astype(np.int64)
    return indptr, indices, np.zeros((N, 8), dtype=np.float32), np.zeros(N, dtype=np.int64)


@pytest.mark.parametrize("kw,match", [
    (dict(model="foo"), "model must be 'sage' or 'gat'"),
    (dict(model="foo", gat_input=True), "gat_input=True: model is 'foo'"),                  # (today's winner stays)
    (dict(workload=np.zeros(N - 1, dtype=np.int32)), r"workload must be int32 \[num_nodes\]"),
    (dict(workload=np.ones(N, dtype=np.int32)), r"values in \[0, world\)"),
    (dict(workload=np.ones(N, dtype=np.int32), model="foo"), "workload must be"),           # (as before: the workload first)
])
def test_constructor_refuses_before_any_device_call(kw, match, monkeypatch):
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("a device call before the arguments were checked"))
    monkeypatch.setattr(_abi, "Engine", lambda *a, **k: pytest.fail("an engine before the arguments were checked"))
    indptr, indices, feats, labels = _tiny()
    with pytest.raises(ValueError, match=match):
        train.Trainer(indptr, indices, feats, labels, C, fanouts=(2, 2), batch=4, streams=1, hidden=8, heads=2, **kw)


def test_own_nodes():
    assert train._own_nodes(None, 1, 3, N).tolist() == [1, 4, 7] and train._own_nodes(None, 0, 1, N).tolist() == list(range(N))
    own = train._own_nodes(np.array([1, 0, 1, 1, 0, 0, 1, 2], dtype=np.int32), 1, 3, N)
    assert own.dtype == np.int64 and own.tolist() == [0, 2, 3, 6]
    assert train._own_nodes(np.zeros(N, dtype=np.int32), 1, 2, N).shape == (0,)


def _rows():
    rng = np.random.default_rng(3)
    return rng.standard_normal((N, F)).astype(np.float32), rng.integers(0, C, size=N).astype(np.int64)


def test_host_rows_callables_and_arrays_agree():
    x, y = _rows()
    own = np.array([1, 4, 7], dtype=np.int64)
    for fdt in (torch.float32, torch.float16, torch.bfloat16):
        fa, la = train._host_rows(x, y, own, 3, fdt, False, C)
        fc, lc = train._host_rows(lambda ids: x[ids], lambda ids: y[ids], own, 3, fdt, False, C)
        assert fa.dtype == fdt and fa.is_contiguous() and fa.shape == (3, F) and torch.equal(fa, fc)
        assert torch.equal(fa, torch.from_numpy(x[own]).to(fdt))              # round to nearest even, on the host
        assert la.dtype == np.int64 and la.tolist() == lc.tolist() == y[own].tolist()
    # one part takes the arrays whole
    fa, la = train._host_rows(x, y, np.arange(N, dtype=np.int64), 1, torch.float32, False, C)
    assert torch.equal(fa, torch.from_numpy(x)) and la.tolist() == y.tolist()
    # a tensor of one of the three types passes as it is
    fb, _ = train._host_rows(lambda ids: torch.from_numpy(x[ids]).to(torch.bfloat16), y, own, 3, torch.bfloat16, False, C)
    assert torch.equal(fb, torch.from_numpy(x[own]).to(torch.bfloat16))


def test_host_rows_element_types(monkeypatch):
    x, y = _rows()
    own = np.arange(N, dtype=np.int64)
    h = x.astype(np.float16)
    f16, _ = train._host_rows(h, y, own, 1, torch.float16, False, C)
    assert f16.dtype == torch.float16 and torch.equal(f16.view(torch.int16), torch.from_numpy(h).view(torch.int16))
    f32, _ = train._host_rows(h, y, own, 1, torch.float32, False, C)
    assert torch.equal(f32, torch.from_numpy(h).to(torch.float32))
    # what becomes a tensor: float16 rows as they come (no float32 copy of them, whatever the stored type), integers and
    # float64 through float32
    seen, orig = [], torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: (seen.append(a.dtype), orig(a))[1])
    train._host_rows(h, y, own, 1, torch.bfloat16, False, C)
    train._host_rows(np.arange(N * F).reshape(N, F), y, own, 1, torch.float32, False, C)
    train._host_rows(x.astype(np.float64), y, own, 1, torch.float16, False, C)
    monkeypatch.undo()
    assert seen == [np.float16, np.float32, np.float32]
    fi, _ = train._host_rows(np.arange(N * F).reshape(N, F), y, own, 1, torch.float16, False, C)
    assert torch.equal(fi, torch.arange(N * F, dtype=torch.float32).reshape(N, F).to(torch.float16))
    for bad in (x[:, 0], torch.zeros((N, F), dtype=torch.float64), torch.zeros((N, F), dtype=torch.int32)):
        with pytest.raises(ValueError, match="features: a float32, float16 or bfloat16 matrix expected"):
            train._host_rows(lambda ids, bad=bad: bad, y, own, 1, torch.float32, False, C)


def test_host_rows_multilabel_and_coverage():
    x, _ = _rows()
    own = np.array([0, 2, 3, 6], dtype=np.int64)
    ym = np.random.default_rng(5).integers(0, 2, size=(N, C))
    _, packed = train._host_rows(x, ym, own, 2, torch.float32, True, C)
    assert packed.dtype == np.int32 and packed.shape == (4, 1) and np.array_equal(packed, aggr.pack_labels(ym[own]))
    assert np.array_equal(l0.unpack_labels(packed, C), ym[own].astype(bool))
    _, again = train._host_rows(x, lambda ids: ym[ids].astype(bool), own, 2, torch.float32, True, C)
    assert np.array_equal(again, packed)
    with pytest.raises(ValueError, match=r"multilabel=True: the rank's label rows must be \[4, 3\], not \(3, 3\)"):
        train._host_rows(x, lambda ids: ym[ids[1:]], own, 2, torch.float32, True, C)
    with pytest.raises(ValueError):
        train._host_rows(x, lambda ids: ym[ids] + 1, own, 2, torch.float32, True, C)     # (aggr.pack_labels: 0 / 1 only)
    y = np.zeros(N, dtype=np.int64)
    with pytest.raises(ValueError, match="features / labels do not cover the rank's 4 nodes"):
        train._host_rows(lambda ids: x[ids[:-1]], y, own, 2, torch.float32, False, C)
    with pytest.raises(ValueError, match="features / labels do not cover the rank's 4 nodes"):
        train._host_rows(x, lambda ids: y[:3], own, 2, torch.float32, False, C)
    with pytest.raises(ValueError, match="do not cover the rank's 8 nodes"):
        train._host_rows(x[:5], y, np.arange(N, dtype=np.int64), 1, torch.float32, False, C)


def test_upload_table_on_the_host():
    """the padded form of a 16-bit table whose width is no multiple of 4, on the one device a CPU test has"""
    x, _ = _rows()
    cpu = torch.device("cpu")
    t32 = torch.from_numpy(x)
    feat, padded = train._upload_table(t32, cpu)
    assert padded is False and torch.equal(feat, t32)
    t16 = t32.to(torch.float16)
    feat, padded = train._upload_table(t16, cpu)
    assert padded is True and feat.shape == (N, F) and feat.stride() == (8, 1) and torch.equal(feat, t16)
    whole = torch.as_strided(feat, (N, 8), (8, 1))
    assert torch.equal(whole[:, F:], torch.zeros((N, 2), dtype=torch.float16))
    feat, padded = train._upload_table(t16[:, :4].contiguous(), cpu)
    assert padded is False and feat.is_contiguous()


def test_feature_rows_round_trip(tmp_path):
    """float32, float16 and bfloat16 words of 4 x 6 rows: what l0.feature_rows returns holds the stored bits"""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((4, F)).astype(np.float32)
    f32 = l0.feature_rows(x, "float32")
    assert isinstance(f32, np.ndarray) and f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), x.view(np.uint32))
    h = x.astype(np.float16)
    f16 = l0.feature_rows(h, "float16")
    assert isinstance(f16, np.ndarray) and f16.dtype == np.float16 and np.array_equal(f16.view(np.uint16), h.view(np.uint16))
    words = l0.to_bfloat16_words(x)
    bf = l0.feature_rows(words, "bfloat16")
    assert torch.is_tensor(bf) and bf.dtype == torch.bfloat16 and bf.shape == (4, F)
    assert np.array_equal(bf.view(torch.int16).numpy().view(np.uint16), words)
    assert torch.equal(bf, torch.from_numpy(x).to(torch.bfloat16))
    assert np.array_equal(bf.to(torch.float32).numpy(), l0.bfloat16_words_to_float32(words))
    # through a memory map, selected rows (what the trainer's callable does) and a copy of the whole map (predict's)
    path = str(tmp_path / "features.bin")
    words.tofile(path)
    fmap = np.memmap(path, dtype=np.uint16, mode="r", shape=(4, F))
    own = np.array([3, 1])
    assert torch.equal(l0.feature_rows(fmap[own], "bfloat16"), bf[[3, 1]])
    assert torch.equal(torch.as_tensor(l0.feature_rows(np.array(fmap), "bfloat16")), bf)
    assert type(l0.feature_rows(fmap[own], "float16")) is np.ndarray
