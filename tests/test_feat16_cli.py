"""`python -m cslicer.train` on an L0 directory whose features.bin is float16: the table is memory-mapped in its stored
type, kept in HBM as float16, trained from in place and evaluated."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _l0_dir(tmp_path, feature_dtype):
    from cslicer import l0
    n = 4000
    indptr, indices = l0.synth_graph(n, 9.0, seed=4)
    rng = np.random.default_rng(0)
    feats = rng.random((n, 12), dtype=np.float32)
    labels = np.argmax(feats[:, :3], axis=1).astype(np.int32)
    d = str(tmp_path / feature_dtype)
    l0.write_l0(d, indptr, indices, features=feats, labels=labels, num_classes=3, feature_dtype=feature_dtype)
    return d, n


def _spy_on_trainers(monkeypatch):
    """every Trainer the command line builds, so that the test can look at the table it trained from"""
    from cslicer import train
    made = []
    real = train.Trainer

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(train, "Trainer", Spy)
    return made


def test_train_cli_trains_from_a_float16_l0_directory(capsys, tmp_path, monkeypatch):
    from cslicer import l0, train
    d, n = _l0_dir(tmp_path, "float16")
    assert l0.read_meta(d)["feature_dtype"] == "float16"
    made = _spy_on_trainers(monkeypatch)
    train.main(["--graph", d, "--eval-split", "holdout", "--fan-out", "4,6", "--num-layers", "2", "--num-hidden", "16",
                "--batch-size", "300", "--num-epochs", "1", "--max-steps", "4"])
    out = capsys.readouterr().out
    assert "Eval Acc" in out and "epoch 0: 4 minibatches" in out and "avg forward time" in out
    assert "feature table: float16, %d bytes" % (n * 12 * 2) in out
    (tr,) = made
    # the table the steps read is the directory's own 16-bit rows, bit for bit: nothing was widened on the way
    assert tr.feat.dtype == torch.float16 and tr.feat.element_size() == 2 and tr.feat.shape == (n, 12)
    stored, _ = l0.read_features(d, mmap=False)
    assert torch.equal(tr.feat.cpu().view(torch.int16), torch.from_numpy(stored.view(np.int16)))
    assert tr.native is not None and tr.steps_done == 4


@pytest.mark.parametrize("stored,asked", [("float32", "bfloat16"), ("bfloat16", None), ("float16", "float32")])
def test_train_cli_converts_on_load_when_asked_for_another_type(capsys, tmp_path, monkeypatch, stored, asked):
    from cslicer import l0, train
    d, n = _l0_dir(tmp_path, stored)
    made = _spy_on_trainers(monkeypatch)
    train.main(["--graph", d, "--eval-split", "holdout", "--fan-out", "4,6", "--num-layers", "2", "--num-hidden", "16",
                "--batch-size", "300", "--num-epochs", "1", "--max-steps", "2"] +
               (["--feature-dtype", asked] if asked else []))
    assert "Eval Acc" in capsys.readouterr().out
    (tr,) = made
    want_dt = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[asked or stored]
    rows, _ = l0.read_features(d, mmap=False)
    if stored == "bfloat16":
        rows = torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16)
    else:
        rows = torch.from_numpy(rows)
    assert tr.feat.dtype == want_dt
    bits = torch.int32 if want_dt == torch.float32 else torch.int16
    assert torch.equal(tr.feat.cpu().view(bits), rows.to(want_dt).view(bits))
