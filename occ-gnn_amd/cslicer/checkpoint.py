"""A trained model on disk: ONE file, written by torch.save and read back with
torch.load(weights_only=True, map_location="cpu").

The file is a dict of tensors, numbers, strings, bools, None, lists and dicts -- no pickled class, no callable (a trainer's
lr_schedule is not stored) -- so reading one never runs code of the file's:

    format      "cslicer-checkpoint"
    version     1
    model       kind ("sage" / "gat"), in_feats, hidden, n_classes, heads, n_layers, multilabel: what build_model needs;
                a normalised GraphSAGE model adds norm ("layer") and norm_eps, any other has neither key
    state       model.state_dict(), on the CPU
    optimizer   aggr.Adam.state_dict(): t, lr, betas, eps, weight_decay (per tensor), decoupled, max_grad_norm, the two
                moments per parameter (m, v: lists in parameter order), skipped; None for a file written from a bare model
    trainer     what the run was built with and where it stands (Trainer.checkpoint_fields): steps_done, seed, dropout_seed,
                rng_seed, fanouts, batch, streams, replace, world, feature_dtype, dropout, feat_dropout, attn_dropout,
                edge_weighted, and norm where the model is normalised; None for a bare model
    extra       the caller's own plain values (the command line stores {"epoch": epochs done})

Nothing in it depends on the number of ranks: the weights are replicated on every path, so a file written by rank 0 of 4
loads into a single-GPU trainer and the other way round.  The sampler's position is NOT in the file: a resumed run replays
the slicer instead (Trainer.skip).

write() is atomic: the bytes go to path + ".tmp" in the same directory, are flushed to the disk and renamed over `path`;
a write that fails leaves an earlier file as it was and no .tmp behind.
"""
import os

import torch

from . import splitgnn

FORMAT, VERSION = "cslicer-checkpoint", 1
# the `model` block, in the order a mismatch is reported
MODEL_FIELDS = ("kind", "in_feats", "hidden", "n_classes", "heads", "n_layers", "multilabel")
NORM_FIELDS = ("norm", "norm_eps")      # a normalised model's; absent from every other block
_PLAIN = (type(None), bool, int, float, str)


def model_block(model, multilabel=False):
    """the `model` block of a DistSAGEModel / DistGATModel, from its layers' shapes.  What the architecture does not
    depend on is recorded as 0: `heads` of a GraphSAGE model, `hidden` of a one-layer model."""
    L = len(model.convs)
    first = model.convs[0]
    if isinstance(model, splitgnn.DistSAGEModel):
        block = {"kind": "sage", "in_feats": first.fc.in_features // 2, "hidden": first.fc.out_features if L > 1 else 0,
                 "n_classes": model.convs[-1].fc.out_features, "heads": 0, "n_layers": L, "multilabel": bool(multilabel)}
        if model.norm is not None:       # (a model without norm keeps exactly the keys it has always had)
            block.update(norm=model.norm, norm_eps=float(model.norm_eps))
        return block
    if isinstance(model, splitgnn.DistGATModel):
        return {"kind": "gat", "in_feats": first.fc.in_features, "hidden": first.D if L > 1 else 0,
                "n_classes": int(model.n_classes), "heads": int(model.heads), "n_layers": L, "multilabel": bool(multilabel)}
    raise TypeError("a DistSAGEModel or a DistGATModel expected, not %s" % type(model).__name__)


def build_model(block):
    """a fresh model (CPU, its own initial weights) of the architecture a `model` block records"""
    if block["kind"] == "sage":
        # (a one-layer model records hidden = 0: nothing is normalised there, whatever `norm` says)
        return splitgnn.DistSAGEModel(block["in_feats"], block["hidden"], block["n_classes"], n_layers=block["n_layers"],
                                      norm=block.get("norm"), norm_eps=block.get("norm_eps", 1e-5))
    if block["kind"] == "gat":
        return splitgnn.DistGATModel(block["in_feats"], block["hidden"], block["n_classes"], heads=block["heads"],
                                     n_layers=block["n_layers"])
    raise ValueError("checkpoint: model kind %r is neither 'sage' nor 'gat'" % (block["kind"],))


def check_model(block, own, what="the trainer"):
    """ValueError naming the first field of MODEL_FIELDS -- then norm, norm_eps (absent: None) -- in which the file's `model`
    block differs from `own`"""
    for k in MODEL_FIELDS + NORM_FIELDS:
        if block.get(k) != own.get(k):
            raise ValueError("checkpoint: the file's model has %s = %r, %s has %r" % (k, block.get(k), what, own.get(k)))


def _check_plain(v, where):
    """ValueError unless v is made of plain values, lists, dicts with string keys and tensors only"""
    if isinstance(v, _PLAIN) or torch.is_tensor(v):
        return
    if isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _check_plain(x, "%s[%d]" % (where, i))
    elif isinstance(v, dict):
        for k, x in v.items():
            if not isinstance(k, str):
                raise ValueError("checkpoint: %s has the key %r, strings expected" % (where, k))
            _check_plain(x, "%s[%r]" % (where, k))
    else:
        raise ValueError("checkpoint: %s is a %s; numbers, strings, bools, None, tensors, lists and dicts expected"
                         % (where, type(v).__name__))


def _listed(v):
    """tuples as lists, all the way down (what the file holds)"""
    if isinstance(v, (list, tuple)):
        return [_listed(x) for x in v]
    if isinstance(v, dict):
        return {k: _listed(x) for k, x in v.items()}
    return v


def write(path, model, optimizer=None, trainer=None, extra=None, multilabel=False):
    """Write the checkpoint of `model` to `path`, atomically (module docstring).  optimizer: an aggr.Adam, or its
    state_dict(), or None; trainer: the dict of the `trainer` block, or None; extra: a dict of plain values."""
    extra = {} if extra is None else extra
    if not isinstance(extra, dict):
        raise ValueError("checkpoint: extra must be a dict of plain values, not a %s" % type(extra).__name__)
    _check_plain(extra, "extra")
    if trainer is not None:
        _check_plain(trainer, "trainer")
    if optimizer is not None and not isinstance(optimizer, dict):
        optimizer = optimizer.state_dict()
    obj = {"format": FORMAT, "version": VERSION, "model": model_block(model, multilabel),
           "state": {k: v.detach().cpu() for k, v in model.state_dict().items()},
           "optimizer": _listed(optimizer), "trainer": _listed(trainer), "extra": _listed(extra)}
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def read(path):
    """The dict write() stored.  ValueError with the reason for a file torch.load(weights_only=True) rejects (a pickled
    class among them), one that is no checkpoint (no or another `format`), an unknown `version`, or a missing block; a
    file that is not there is the OSError of opening it."""
    path = os.fspath(path)
    try:
        obj = torch.load(path, weights_only=True, map_location="cpu")
    except OSError:
        raise
    except Exception as ex:
        raise ValueError("checkpoint: %s cannot be read with weights_only=True: %s" % (path, str(ex).split("\n")[0]))
    if not isinstance(obj, dict) or obj.get("format") != FORMAT:
        raise ValueError("checkpoint: %s is not a cslicer checkpoint (no format = %r)" % (path, FORMAT))
    if obj.get("version") != VERSION:
        raise ValueError("checkpoint: %s has version %r, this code reads version %d" % (path, obj.get("version"), VERSION))
    for k in ("model", "state", "optimizer", "trainer", "extra"):
        if k not in obj:
            raise ValueError("checkpoint: %s has no %r block" % (path, k))
    if not isinstance(obj["model"], dict) or any(k not in obj["model"] for k in MODEL_FIELDS):
        raise ValueError("checkpoint: the model block of %s lacks one of %s" % (path, ", ".join(MODEL_FIELDS)))
    return obj


def model_from(ck, device="cpu"):
    """the model a read() checkpoint holds, on `device`, weights loaded"""
    model = build_model(ck["model"])
    try:
        model.load_state_dict(ck["state"])
    except RuntimeError as ex:
        raise ValueError("checkpoint: the stored tensors are not those of the recorded model: %s" % str(ex).split("\n")[0])
    return model.to(device)
