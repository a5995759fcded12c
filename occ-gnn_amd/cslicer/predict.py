"""Apply a saved model to a graph: full-neighbour inference (cslicer.infer) of a checkpoint file, without a trainer.

    python -m cslicer.predict --model run.ckpt --graph <L0 dir> --out preds.npy [--nodes FILE] [--logits] [--feature-dtype T]
                              [--correct-smooth [--train-nodes FILE] [--cs-layers T1,T2] [--cs-alpha A1,A2] [--cs-scale auto|NUMBER]]
"""
import os
import time

import numpy as np
import torch

from . import aggr, checkpoint, l0, smooth


def _parser():
    import argparse
    ap = argparse.ArgumentParser("full-neighbour inference of a saved model on MI355X")
    ap.add_argument("--model", type=str, required=True, metavar="FILE", help="a checkpoint written by cslicer.train --save")
    ap.add_argument("--graph", type=str, required=True, help="an L0 directory (cslicer.l0) with features.bin")
    ap.add_argument("--out", type=str, required=True, metavar="FILE", help="the .npy file to write")
    ap.add_argument("--nodes", type=str, default=None, metavar="FILE",
                    help="the nodes to predict, in this order: a .npy array or a raw int64 binary (as train_idx.bin); "
                         "default: every node")
    ap.add_argument("--logits", action="store_true",
                    help="write the float32 logits [n, n_classes] instead of classes (with --correct-smooth: the smoothed class "
                         "scores in [0, 1], which are not logits)")
    ap.add_argument("--feature-dtype", choices=tuple(aggr.FEATURE_DTYPES), default=None,
                    help="element type of the feature table on the device (default: what the directory's meta.txt says)")
    ap.add_argument("--correct-smooth", action="store_true",
                    help="Correct and Smooth (cslicer.smooth) over the predictions of every node, with the directory's labels.bin "
                         "on the training nodes; classes or --logits are then written from the smoothed scores")
    ap.add_argument("--train-nodes", type=str, default=None, metavar="FILE",
                    help="--correct-smooth: the labelled nodes, a file as --nodes takes (default: the directory's train_idx.bin)")
    smooth.add_options(ap)
    return ap


def read_nodes(path, num_nodes, option="--nodes"):
    """int64 node ids of --nodes FILE (or of `option`'s); SystemExit for ids outside the graph"""
    ids = np.load(path) if path.endswith(".npy") else np.fromfile(path, dtype=np.int64)
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= num_nodes):
        raise SystemExit("%s %s: node ids outside [0, %d)" % (option, path, num_nodes))
    return ids


def _smooth_inputs(a, mb, num_nodes):
    """--correct-smooth: (training nodes, their labels, correct_and_smooth's keywords), None without it.  SystemExit for
    a multi-label model and for a directory without the labels or the training nodes."""
    kw = smooth.options_of(a)
    if kw is None:
        if a.train_nodes is not None:
            raise SystemExit("--train-nodes belongs to --correct-smooth")
        return None
    if mb["multilabel"]:
        raise SystemExit("--correct-smooth: %s holds a multi-label model, which has no one-hot labels to propagate" % a.model)
    path = a.train_nodes or os.path.join(a.graph, "train_idx.bin")
    labels = os.path.join(a.graph, "labels.bin")
    for need in (path, labels):
        if not os.path.isfile(need):
            raise SystemExit("--correct-smooth needs %s" % need)
    train = read_nodes(path, num_nodes, "--train-nodes")
    lab = np.memmap(labels, dtype=np.int32, mode="r", shape=(num_nodes,))
    return train, np.asarray(lab[train]).astype(np.int64), kw


def main(argv=None):
    """Write the predictions of the model in --model for the nodes of --graph to --out (numpy .npy), one row per node of
    --nodes (default: all, ascending): int64 classes [n] (the argmax, ties to the lowest class), for a multi-label model
    int8 rows [n, n_classes] of 0 / 1 (logit > 0), with --logits the float32 logits [n, n_classes].  The model is applied
    with EVERY neighbour (cslicer.infer.full_inference), as `Trainer.evaluate` applies it.  A directory whose feature_dim /
    num_classes are not the model's is refused before its features are read.  --feature-dtype: the table's element type on
    the device (default: as stored); a model trained on a 16-bit table predicts bitwise what its trainer did on the same
    type.  --correct-smooth: the model is applied to EVERY node and its predictions go through
    cslicer.smooth.correct_and_smooth with the labels (labels.bin) of --train-nodes (default: train_idx.bin); the rows of
    --nodes are then taken from the smoothed scores: their argmax, or with --logits the scores themselves (float32 in
    [0, 1], not logits).  Prints one summary line."""
    a = _parser().parse_args(argv)
    if not os.path.isfile(a.model):
        raise SystemExit("--model %s: no such file" % a.model)
    try:
        ck = checkpoint.read(a.model)
    except ValueError as ex:
        raise SystemExit("--model %s: %s" % (a.model, ex))
    mb = ck["model"]
    if not os.path.isfile(os.path.join(a.graph, "meta.txt")):
        raise SystemExit("--graph %s: not an L0 directory (no meta.txt)" % a.graph)
    meta = l0.read_meta(a.graph)
    for key, have in (("feature_dim", mb["in_feats"]), ("num_classes", mb["n_classes"])):
        if meta.get(key) != have:       # (before the features are loaded)
            raise SystemExit("--graph %s has %s = %r, the model in %s was trained with %d"
                             % (a.graph, key, meta.get(key), a.model, have))
    cs = _smooth_inputs(a, mb, meta["num_nodes"])        # (refused before the graph is read)
    from . import infer
    t0 = time.time()
    indptr, indices, meta = l0.read_l0(a.graph, mmap=False)
    n = meta["num_nodes"]
    nodes = None if a.nodes is None else read_nodes(a.nodes, n)
    rows, stored = l0.read_features(a.graph, meta)
    feats = torch.as_tensor(l0.feature_rows(np.array(rows), stored))        # (np.array: a copy, the map is read-only)
    # converted on the HOST, round to nearest even, as the trainer stores its table
    feats = feats.to(aggr.FEATURE_DTYPES[a.feature_dtype or stored]).contiguous()
    dev = torch.device("cuda", torch.cuda.current_device())
    model = checkpoint.model_from(ck, dev)
    logits = infer.full_inference(model, indptr, indices, feats, nodes=nodes if cs is None else None)
    if cs is not None:
        try:
            logits = smooth.correct_and_smooth(logits, indptr, indices, cs[0], cs[1], nodes=nodes, **cs[2])
        except ValueError as ex:
            raise SystemExit("--correct-smooth: %s" % ex)
    if a.logits:
        out = logits.cpu().numpy()
    elif mb["multilabel"]:
        out = (logits > 0).to(torch.int8).cpu().numpy()
    else:
        out = torch.argmax(logits, dim=1).cpu().numpy().astype(np.int64)
    infer.release(indptr, indices)
    with open(a.out, "wb") as f:        # (np.save would append .npy to another name)
        np.save(f, out)
    print("predict: %d nodes, %s model (%d classes%s), %s %r -> %s in %.2f s"
          % (out.shape[0], mb["kind"], mb["n_classes"], ", multi-label" if mb["multilabel"] else "", out.dtype,
             tuple(out.shape), a.out, time.time() - t0))


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
