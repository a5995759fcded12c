"""The checkpoint file (cslicer.checkpoint) and the command lines' refusals, without a GPU: the round trip of
both models, the refusals of read(), the atomic write, and the early exits of train.main / predict.main."""
import os

import numpy as np
import pytest
import torch

from cslicer import checkpoint, infer, l0, predict, splitgnn, train


def _models():
    torch.manual_seed(11)
    return {"sage": splitgnn.DistSAGEModel(16, 16, 5), "gat": splitgnn.DistGATModel(16, 8, 5, heads=2)}


BLOCKS = {"sage": {"kind": "sage", "in_feats": 16, "hidden": 16, "n_classes": 5, "heads": 0, "n_layers": 3, "multilabel": False},
          "gat": {"kind": "gat", "in_feats": 16, "hidden": 8, "n_classes": 5, "heads": 2, "n_layers": 3, "multilabel": False}}


def _opt_state(model, t=7):
    """what aggr.Adam.state_dict() returns, made on the host (the optimizer itself needs device parameters)"""
    g = torch.Generator().manual_seed(5)
    ps = list(model.parameters())
    return {"t": t, "lr": 1e-2, "betas": [0.9, 0.999], "eps": 1e-8, "weight_decay": [0.05 if p.dim() >= 2 else 0.0 for p in ps],
            "decoupled": True, "max_grad_norm": float("inf"), "m": [torch.randn(p.shape, generator=g) for p in ps],
            "v": [torch.rand(p.shape, generator=g) for p in ps], "skipped": 2}


@pytest.mark.parametrize("kind", ["sage", "gat"])
def test_round_trip_and_load_model(kind, tmp_path):
    model = _models()[kind]
    opt = _opt_state(model)
    fields = {"steps_done": 7, "seed": 3, "dropout_seed": 3, "rng_seed": 5489, "fanouts": (3, 3, 3), "batch": 64, "streams": 2,
              "replace": True, "world": 4, "feature_dtype": "bfloat16", "dropout": 0.5, "feat_dropout": 0.0,
              "attn_dropout": 0.0, "edge_weighted": False}
    path = str(tmp_path / "m.ckpt")
    checkpoint.write(path, model, optimizer=opt, trainer=fields, extra={"epoch": 2, "note": "x", "nested": {"a": [1, 2.5, None]}})
    assert not os.path.exists(path + ".tmp")
    ck = checkpoint.read(path)
    assert ck["format"] == "cslicer-checkpoint" and ck["version"] == 1
    assert ck["model"] == BLOCKS[kind] == checkpoint.model_block(model)
    assert ck["extra"] == {"epoch": 2, "note": "x", "nested": {"a": [1, 2.5, None]}}
    assert ck["trainer"] == dict(fields, fanouts=[3, 3, 3])          # (tuples are stored as lists)
    want = model.state_dict()
    assert list(ck["state"]) == list(want)
    for k, v in want.items():
        assert ck["state"][k].device.type == "cpu" and torch.equal(ck["state"][k].view(torch.int32), v.view(torch.int32)), k
    o = ck["optimizer"]
    assert {k: o[k] for k in o if k not in ("m", "v")} == {k: opt[k] for k in opt if k not in ("m", "v")}
    assert o["max_grad_norm"] == float("inf")
    for name in ("m", "v"):
        assert len(o[name]) == len(opt[name]) and all(torch.equal(x, y) for x, y in zip(o[name], opt[name]))
    # inference without a trainer: the right class, equal tensors, fresh storage
    got = infer.load_model(path, "cpu")
    assert type(got) is type(model) and got is not model
    assert checkpoint.model_block(got) == BLOCKS[kind]
    for (ka, pa), (kb, pb) in zip(got.state_dict().items(), want.items()):
        assert ka == kb and torch.equal(pa, pb) and pa.data_ptr() != pb.data_ptr()
    # a bare model: no optimizer, no trainer block
    checkpoint.write(path, model, multilabel=True)
    ck = checkpoint.read(path)
    assert ck["optimizer"] is None and ck["trainer"] is None and ck["extra"] == {} and ck["model"]["multilabel"] is True


def test_one_layer_models_round_trip(tmp_path):
    """`hidden` is no part of a one-layer architecture: recorded as 0, and the model is rebuilt all the same"""
    for model in (splitgnn.DistSAGEModel(8, 32, 3, n_layers=1), splitgnn.DistGATModel(8, 4, 3, heads=2, n_layers=1)):
        path = str(tmp_path / "one.ckpt")
        checkpoint.write(path, model)
        assert checkpoint.read(path)["model"]["hidden"] == 0
        got = infer.load_model(path, "cpu")
        assert all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), model.state_dict().values()))


class _Custom(object):
    def __init__(self):
        self.x = 1


def test_read_refuses(tmp_path):
    path = str(tmp_path / "f")
    torch.save([1, 2], path)
    with pytest.raises(ValueError, match="not a cslicer checkpoint"):
        checkpoint.read(path)
    torch.save({"format": "something-else", "version": 1}, path)
    with pytest.raises(ValueError, match="not a cslicer checkpoint"):
        checkpoint.read(path)
    model = _models()["sage"]
    checkpoint.write(path, model)
    good = torch.load(path, weights_only=True)
    torch.save(dict(good, version=99), path)
    with pytest.raises(ValueError, match="version 99"):
        checkpoint.read(path)
    torch.save({k: v for k, v in good.items() if k != "state"}, path)
    with pytest.raises(ValueError, match="'state'"):
        checkpoint.read(path)
    # a pickled class: torch.load(weights_only=True) must reject the file, whatever else it holds
    torch.save(dict(good, extra={"thing": _Custom()}), path)
    with pytest.raises(ValueError, match="weights_only"):
        checkpoint.read(path)
    with open(path, "wb") as f:
        f.write(b"not a torch file at all")
    with pytest.raises(ValueError, match="weights_only"):
        checkpoint.read(path)
    with pytest.raises(OSError):
        checkpoint.read(str(tmp_path / "missing"))
    # write() itself never stores what read() would refuse
    for extra in ({"thing": _Custom()}, {"f": len}, {1: 2}, [1]):
        with pytest.raises(ValueError, match="extra"):
            checkpoint.write(path, model, extra=extra)


def test_architecture_mismatch_names_the_field(tmp_path):
    path = str(tmp_path / "m.ckpt")
    checkpoint.write(path, _models()["sage"])
    ck = checkpoint.read(path)
    for other, field in ((splitgnn.DistSAGEModel(16, 32, 5), "hidden"), (splitgnn.DistSAGEModel(12, 16, 5), "in_feats"),
                         (splitgnn.DistSAGEModel(16, 16, 6), "n_classes"), (splitgnn.DistSAGEModel(16, 16, 5, n_layers=2), "n_layers"),
                         (_models()["gat"], "kind")):
        with pytest.raises(ValueError, match=r"model has %s = " % field):
            checkpoint.check_model(ck["model"], checkpoint.model_block(other))
    with pytest.raises(ValueError, match="multilabel = False"):
        checkpoint.check_model(ck["model"], checkpoint.model_block(_models()["sage"], multilabel=True))
    checkpoint.check_model(ck["model"], checkpoint.model_block(_models()["sage"]))
    checkpoint.write(path, _models()["gat"])
    with pytest.raises(ValueError, match="model has heads = 2"):
        checkpoint.check_model(checkpoint.read(path)["model"], checkpoint.model_block(splitgnn.DistGATModel(16, 8, 5, heads=4)))


def test_a_failed_write_leaves_the_old_file(tmp_path, monkeypatch):
    path = str(tmp_path / "m.ckpt")
    models = _models()
    checkpoint.write(path, models["sage"], extra={"epoch": 1})
    with open(path, "rb") as f:
        before = f.read()

    def half_way(obj, f, *a, **kw):
        f.write(b"half a file")
        raise IOError("disk full")
    monkeypatch.setattr(torch, "save", half_way)
    with pytest.raises(IOError, match="disk full"):
        checkpoint.write(path, models["gat"], extra={"epoch": 2})
    monkeypatch.undo()
    with open(path, "rb") as f:
        assert f.read() == before
    assert sorted(os.listdir(str(tmp_path))) == ["m.ckpt"]
    assert checkpoint.read(path)["extra"] == {"epoch": 1}
    # and a first write that fails leaves nothing at all
    monkeypatch.setattr(torch, "save", half_way)
    with pytest.raises(IOError):
        checkpoint.write(str(tmp_path / "new.ckpt"), models["gat"])
    monkeypatch.undo()
    assert sorted(os.listdir(str(tmp_path))) == ["m.ckpt"]


def _no_device(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(l0, "read_l0", boom)
    monkeypatch.setattr(l0, "synth_graph", boom)
    monkeypatch.setattr(l0, "read_features", boom)


def test_train_cli_refuses_before_the_graph_is_loaded(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(SystemExit, match="--resume /nonexistent: no such file"):
        train.main(["--resume", "/nonexistent"])
    path = str(tmp_path / "f")
    torch.save([1, 2], path)
    with pytest.raises(SystemExit, match="not a cslicer checkpoint"):
        train.main(["--resume", path])
    checkpoint.write(path, _models()["sage"])                 # a checkpoint, but not one --save wrote: no epoch
    with pytest.raises(SystemExit, match="not written by --save"):
        train.main(["--resume", path])
    with pytest.raises(SystemExit, match="--save"):
        train.main(["--save", str(tmp_path / "no" / "such" / "dir" / "f")])
    with pytest.raises(SystemExit, match="--save-every"):
        train.main(["--save", path, "--save-every", "0"])
    a = train._parser().parse_args([])
    assert a.save is None and a.resume is None and a.save_every == 1
    for word in ("--save FILE [--save-every N] (extra)", "--resume FILE (extra)"):
        assert word in train.main.__doc__
    for name in ("save_checkpoint", "load_checkpoint", "skip"):
        assert name in train.Trainer.__init__.__doc__ and callable(getattr(train.Trainer, name))


def test_predict_cli_refuses_mismatched_meta(tmp_path, monkeypatch):
    indptr, indices = l0.synth_graph(50, 4.0, seed=1)
    rng = np.random.default_rng(0)
    ckpt = str(tmp_path / "m.ckpt")
    checkpoint.write(ckpt, _models()["sage"])                 # 16 features, 5 classes
    dirs = {}
    for name, (F, C) in {"width": (12, 5), "classes": (16, 4)}.items():
        dirs[name] = str(tmp_path / name)
        l0.write_l0(dirs[name], indptr, indices, features=rng.random((50, F), dtype=np.float32),
                    labels=rng.integers(0, C, 50).astype(np.int32), num_classes=C)
    _no_device(monkeypatch)
    out = str(tmp_path / "p.npy")
    with pytest.raises(SystemExit, match="feature_dim = 12, the model .* was trained with 16"):
        predict.main(["--model", ckpt, "--graph", dirs["width"], "--out", out])
    with pytest.raises(SystemExit, match="num_classes = 4, the model .* was trained with 5"):
        predict.main(["--model", ckpt, "--graph", dirs["classes"], "--out", out])
    with pytest.raises(SystemExit, match="no such file"):
        predict.main(["--model", str(tmp_path / "missing"), "--graph", dirs["width"], "--out", out])
    assert not os.path.exists(out)                            # a refused predict writes nothing
    torch.save([1, 2], out)
    with pytest.raises(SystemExit, match="not a cslicer checkpoint"):
        predict.main(["--model", out, "--graph", dirs["width"], "--out", out])
    with pytest.raises(SystemExit, match="not an L0 directory"):
        predict.main(["--model", ckpt, "--graph", str(tmp_path), "--out", out])
