"""End-to-end split-parallel GraphSAGE training step on the slices: the counterpart of the
reference's python/train.py:19-106 (Adam, cross-entropy, 3-layer DistSAGEModel), one process per
GPU over torch.distributed (RCCL) instead of one process driving 4 GPUs with
torch.nn.parallel.replicate/gather.

Per rank g (= part g): an engine in CSL_MODE_GRAPH slices S minibatches per round (every rank
slices the same minibatches, deterministically; nothing about topology is communicated), the rank
keeps the features and labels of the nodes it owns, runs DistSAGEModel.forward_rank on its slice,
cross-entropy on the seeds it owns, backward (boundary gradients travel the reverse all-to-all),
all-reduce of the replicated weights' gradients, Adam.

The print keys of train.py:101-103 are kept (`avg forward time`, `batch slice time`,
`cache refresh time`; there is no feature cache here: features are resident in HBM, so the last
one is reported as 0).
"""
import collections
import math
import os
import time

import numpy as np
import torch

from . import _abi, _roctx, aggr, l0, shard, splitgnn


# The A/B switches a trainer is built under.  They are read when the constructor runs (read_switches), never at import:
# the tests set them per trainer.
Switches = collections.namedtuple("Switches", "no_transpose py_step no_local_fuse no_gat_input",
                                  defaults=(False, False, False, False))

# How a trainer trains a minibatch and what it asks of its engine (step_plan):
#   engine_flags  the _abi.FLAG_* of the engine
#   path          "native" (aggr.SageStep), "native_rank" (aggr.SageRankStep), "local" (autograd, model.forward_local on
#                 the single part) or "parts" (autograd, model.forward_parts / forward_rank on a gathered input)
#   gat_input     whether the attention model's deepest layer is aggr.GatInputLayer
#   input_form    the "parts" path's input matrix: "table" (aggr.FeatureRows: the table read in place), "padded"
#                 (aggr.padded_rows and a gather into it) or "rows" (aggr.gather_rows); None on the other paths
StepPlan = collections.namedtuple("StepPlan", "engine_flags path gat_input input_form")


def read_switches():
    return Switches(no_transpose=bool(os.environ.get("CSLICER_NO_TRANSPOSE")), py_step=bool(os.environ.get("CSLICER_PY_STEP")),
                    no_local_fuse=bool(splitgnn._NO_LOCAL_FUSE), no_gat_input=bool(splitgnn._NO_GAT_INPUT))


def gat_input_obstacle(kind, world, rank_path, n_layers, F, hidden, n_classes, heads, fanout, sw):
    """Why the attention model's deepest layer cannot run aggregate-then-project on the raw feature rows
    (aggr.GatInputLayer), or None where it can.  F: the feature width as known BEFORE the rank's rows are loaded (None:
    callable features without feat_dim); fanout: the deepest layer's.  The one statement of the layer's prerequisites:
    the constructor's gat_input=True refusal raises the text, step_plan turns the layer on where there is none."""
    D = hidden if n_layers > 1 else (n_classes + 3) // 4 * 4
    if kind != "gat":
        return "model is %r, the input layer belongs to model='gat'" % (kind,)
    if world > 1 or rank_path:
        return "more than one part or rank_path: the rank path's attention layer has no aggregate-then-project form"
    if F is None:
        return "the feature width is unknown (pass feat_dim with callable features)"
    if not aggr.gat_input_ok(heads, F, fanout, D):
        return ("aggr.gat_input_ok(heads=%d, F=%d, fanout=%d, D=%d) is false: heads in (1, 2, 4, 8), F %% 4 == 0, "
                "4 <= F <= 128, heads * D <= %d, fanout <= %d" % (heads, F, fanout, D, aggr.GAT_IN_MAX_WIDTH,
                                                                  aggr.gat_in_max_degree()))
    if sw.no_transpose:
        return "CSLICER_NO_TRANSPOSE is set: the upper layers' slices by source are off"
    if sw.no_local_fuse:
        return "CSLICER_NO_LOCAL_FUSE is set: the fused single-part layers are off"
    if sw.no_gat_input:
        return "CSLICER_GAT_NO_INPUT_LAYER is set: the input layer is switched off"
    return None


def step_plan(kind, world, rank_path, n_layers, F, hidden, n_classes, heads, fanout, table_f32, gat_input, replace,
              sw=Switches(), width_known=True, dropout=0.0, multilabel=False):
    """The StepPlan of a configuration, from plain values only (no device, no engine): every rule is written here once.
    ONE function, called when the rank's host rows are in hand -- F is the loaded table's width (feat_dim where given),
    which the path depends on -- so the constructor creates its engine after the host-side loading.
    rank_path: as resolved (None -> world > 1); fanout: the deepest layer's; table_f32: whether the feature table is
    float32; gat_input: the constructor's None / True / False; width_known: whether F was known before the rows were
    loaded (feat_dim, or the shape of a feature matrix; False: callable features without feat_dim); dropout: the
    trainer's probability -- above 0 the rank path runs its autograd step (the native rank sequencer has no dropout), with
    the engine flags that step has always asked for; every other row is what it is at 0.  multilabel: the trainer's --
    the native rank sequencer has no sigmoid-BCE loss either, so with True its row moves the same way and no other does.
    (The attention model's dropout: step_plan_gat_drop below; layer normalisation: step_plan_norm.)"""
    sage, gat = kind == "sage", kind == "gat"
    single = not rank_path and world == 1      # one part in one process, no collective
    want = table_f32 if gat_input is None else gat_input     # (None: a 16-bit table keeps the numbers its runs have had)
    gat_in = bool(want) and gat_input_obstacle(kind, world, rank_path, n_layers, F if width_known else None, hidden,
                                               n_classes, heads, fanout, sw) is None
    # GraphSAGE's backward gathers its input gradients over the upper layers' slices by source (CSLICER_NO_TRANSPOSE:
    # atomic scatter instead)
    by_source = sage and n_layers > 1 and not sw.no_transpose
    # the single part with every layer as one fused node, the deepest reading the resident table through in_nodes
    local = single and sage and F % 4 == 0 and not sw.no_local_fuse
    native_rank = rank_path and sage and F % 4 == 0 and hidden % 4 == 0 and n_classes <= 256 and not sw.py_step
    if native_rank and (dropout > 0 or multilabel):
        # the native rank sequencer has no dropout and no multi-label loss: the rank's autograd step, planned as
        # CSLICER_PY_STEP plans it
        return step_plan(kind, world, rank_path, n_layers, F, hidden, n_classes, heads, fanout, table_f32, gat_input,
                         replace, sw._replace(py_step=True), width_known)

    flags = 0
    if by_source and (single or (rank_path and not sw.py_step)):
        # Neither the widths nor n_classes are looked at: a rank-path model with more than 256 classes, whose autograd
        # step never reads them, still gets the slices by source.  Kept as it is (behaviour, not a rule of this table).
        flags = _abi.FLAG_TRANSPOSE
    elif gat and single and not sw.no_transpose:
        # GAT aggregates PROJECTED features: every layer's sources take a gradient -- the deepest layer's too, unless it
        # is the input layer (no source gradient at all)
        flags = _abi.FLAG_TRANSPOSE | (0 if gat_in else _abi.FLAG_TRANSPOSE_ALL)
    if not replace:
        flags |= _abi.FLAG_NO_REPLACE

    if native_rank:
        path = "native_rank"
    elif local and by_source and hidden % 4 == 0 and not sw.py_step:
        path = "native"
    elif local:
        path = "local"
    else:
        path = "parts"

    form = None
    if path == "parts":
        # "padded": straight into the row-padded buffer the fused GAT layer multiplies (no second copy of 0.3 GB)
        form = "table" if gat_in else "padded" if gat and single and not sw.no_local_fuse else "rows"
    return StepPlan(flags, path, gat_in, form)


def step_plan_gat_drop(feat_dropout=0.0, attn_dropout=0.0, *, kind, gat_input, **cfg):
    """step_plan(kind=kind, gat_input=gat_input, **cfg) under the attention model's two dropout probabilities;
    at 0, their defaults, it IS step_plan.  attn_dropout > 0 turns the input layer off where gat_input is None
    (aggr.GatInputLayer has no attention dropout; gat_input=True with it is the constructor's refusal): the plan is
    gat_input=False's, engine flags and input form included.  Either above 0 moves a rank run of the attention model from the
    fused rank node to its node-by-node form; that is the model's doing (DistGATModel.forward_rank with a drop spec) -- the
    plan's fields, flags 0, path "parts", input form "rows", are the same for both forms.  feat_dropout alone changes no plan.
    (A function of its own: step_plan's parameter list is pinned.)"""
    if kind == "gat" and attn_dropout > 0 and gat_input is None:
        gat_input = False
    return step_plan(kind=kind, gat_input=gat_input, **cfg)


# ---- the stages of Trainer.__init__.  The _check_* functions are its argument checks, one per group of arguments, in the
# order the constructor calls them (of two bad arguments the earlier group's error is raised): pure -- numpy and
# _abi.noreplace_max_fanout() only, no device, no engine -- and each returns its arguments normalised.

def step_plan_norm(norm=None, **cfg):
    """step_plan_gat_drop(**cfg) under the trainer's `norm` (None / "layer"); with None it IS that plan.  The
    native rank sequencer has no layer normalisation, as it has no dropout: with norm="layer" the row that `dropout` moves
    (`native_rank` -> the rank's autograd step, planned as CSLICER_PY_STEP plans it, engine flags included) moves the same
    way, and no other row does."""
    plan = step_plan_gat_drop(**cfg)
    if norm is None or plan.path != "native_rank":
        return plan
    return step_plan_gat_drop(**dict(cfg, sw=cfg.get("sw", Switches())._replace(py_step=True)))


def _check_labels(labels, multilabel, num_nodes, n_classes):
    """multilabel as a bool; with it, a host `labels` (a callable's rows are checked when they are loaded) must be a
    [num_nodes, n_classes] matrix of 0 / 1"""
    multilabel = bool(multilabel)
    if multilabel and not callable(labels):
        shape = np.shape(labels)
        if len(shape) != 2:
            raise ValueError("multilabel=True: labels must be a matrix [num_nodes, n_classes] of 0 / 1, not shape %r"
                             % (shape,))
        if shape != (num_nodes, n_classes):
            raise ValueError("multilabel=True: labels must be [num_nodes = %d, n_classes = %d], not %r"
                             % (num_nodes, n_classes, shape))
        la = np.asarray(labels)
        if la.dtype != np.bool_ and (la.dtype.kind not in "iu" or (la.size and not np.isin(la, (0, 1)).all())):
            raise ValueError("multilabel=True: every label must be 0 or 1 (bool or integer)")
    return multilabel


def _check_dropouts(model, hidden, dropout, feat_dropout, attn_dropout, gat_input):
    """(dropout, feat_dropout, attn_dropout) as floats in [0, 1): the first GraphSAGE's, the other two the attention model's"""
    dropout = float(dropout)
    if not 0.0 <= dropout < 1.0:
        raise ValueError("dropout must be in [0, 1), not %r" % (dropout,))
    if dropout > 0 and model == "gat":
        raise ValueError("dropout > 0: the attention model has no dropout (model='sage' only)")
    if dropout > 0 and hidden % 4 != 0:
        raise ValueError("dropout > 0: hidden must be a multiple of 4 (the kernel moves float4 columns), not %d" % hidden)
    feat_dropout, attn_dropout = float(feat_dropout), float(attn_dropout)
    for name, v in (("feat_dropout", feat_dropout), ("attn_dropout", attn_dropout)):
        if not 0.0 <= v < 1.0:      # (a NaN compares false)
            raise ValueError("%s must be in [0, 1), not %r" % (name, v))
        if v > 0 and model == "sage":
            raise ValueError("%s > 0: GraphSAGE has `dropout`; feat_dropout / attn_dropout belong to model='gat'" % name)
    if attn_dropout > 0 and gat_input is True:
        raise ValueError("attn_dropout > 0 with gat_input=True: the aggregate-then-project input layer has no attention "
                         "dropout (gat_input=None turns it off)")
    return dropout, feat_dropout, attn_dropout


def _check_norm(model, hidden, n_layers, norm, norm_eps):
    """(norm, norm_eps): None or "layer", and eps as a float > 0"""
    if norm not in (None, "layer"):
        raise ValueError("norm must be None or 'layer', not %r" % (norm,))
    norm_eps = float(norm_eps)
    if not norm_eps > 0:
        raise ValueError("norm_eps must be > 0, not %r" % (norm_eps,))
    if norm is not None and model == "gat":
        raise ValueError("norm: the attention model has no normalisation layer (model='sage' only)")
    if norm is not None and hidden % 4 != 0:
        raise ValueError("norm: hidden must be a multiple of 4 (the kernels move float4 columns), not %d" % hidden)
    return norm, norm_eps


def _check_optimizer(weight_decay, max_grad_norm, lr_schedule):
    """(weight_decay, max_grad_norm) as floats (the latter or None); lr_schedule must be None or a callable"""
    weight_decay = float(weight_decay)
    if not weight_decay >= 0.0:      # (a NaN compares false)
        raise ValueError("weight_decay must be >= 0, not %r" % (weight_decay,))
    if max_grad_norm is not None:
        max_grad_norm = float(max_grad_norm)
        if not max_grad_norm > 0.0:
            raise ValueError("max_grad_norm must be None or > 0 (float('inf'): the norm and the non-finite guard "
                             "without clipping), not %r" % (max_grad_norm,))
    if lr_schedule is not None and not callable(lr_schedule):
        raise ValueError("lr_schedule must be None or a callable steps_done -> lr, not %r" % (lr_schedule,))
    return weight_decay, max_grad_norm


def _check_loss(label_smoothing, class_weight, n_classes, multilabel):
    """(label_smoothing as a float, class_weight as float64 [n_classes] or None): the single-label loss's options"""
    label_smoothing = float(label_smoothing)
    if not 0.0 <= label_smoothing < 1.0:     # (a NaN compares false)
        raise ValueError("label_smoothing must be in [0, 1), not %r" % (label_smoothing,))
    if class_weight is not None:
        class_weight = np.asarray(class_weight, dtype=np.float64).reshape(-1) if np.ndim(class_weight) == 1 else None
        if class_weight is None or class_weight.shape[0] != n_classes:
            raise ValueError("class_weight must be a sequence of n_classes = %d numbers" % n_classes)
        if not np.isfinite(class_weight).all() or (class_weight < 0).any() or not (class_weight > 0).any():
            raise ValueError("class_weight: finite numbers >= 0 with at least one > 0 expected")
    if multilabel and (class_weight is not None or label_smoothing != 0.0):
        raise ValueError("multilabel=True: class_weight / label_smoothing belong to the single-label loss; the "
                         "sigmoid-BCE loss has no weights yet")
    return label_smoothing, class_weight


def _check_sampling(edge_weight, replace, fanouts, num_edges):
    """edge_weight as float64 [num_edges] (l0.check_edge_weights) or None; replace=False goes with neither edge weights nor
    a fanout above _abi.noreplace_max_fanout()"""
    if edge_weight is not None:
        if not replace:
            raise ValueError("edge_weight with replace=False: weighted sampling draws with replacement (weighted sampling "
                             "without replacement is not built)")
        edge_weight = l0.check_edge_weights(edge_weight, num_edges)
    if not replace and max(fanouts) > _abi.noreplace_max_fanout():
        raise ValueError("replace=False: fanouts %r exceed the limit of %d neighbours per row"
                         % (tuple(fanouts), _abi.noreplace_max_fanout()))
    return edge_weight


def _check_table(feature_dtype, gat_input):
    """the torch dtype of the feature table named `feature_dtype`; gat_input must be one of None, True, False"""
    if feature_dtype not in aggr.FEATURE_DTYPES:
        raise ValueError("feature_dtype must be one of %s, not %r" % (", ".join(aggr.FEATURE_DTYPES), feature_dtype))
    if not any(gat_input is v for v in (None, True, False)):
        raise ValueError("gat_input must be None, True or False, not %r" % (gat_input,))
    return aggr.FEATURE_DTYPES[feature_dtype]


def _check_gat_input_on(gat_input, *obstacle_args):
    """gat_input=True where gat_input_obstacle(*obstacle_args) names a reason why the input layer cannot run"""
    why = gat_input_obstacle(*obstacle_args) if gat_input is True else None
    if why is not None:
        raise ValueError("gat_input=True: " + why)


def _check_workload(workload, num_nodes, world):
    """the owner table as contiguous int32 [num_nodes] with values in [0, world), or None (v % world)"""
    if workload is not None:
        workload = np.ascontiguousarray(workload, dtype=np.int32)
        if workload.shape != (num_nodes,) or workload.min() < 0 or workload.max() >= world:
            raise ValueError("workload must be int32 [num_nodes] with values in [0, world)")
    return workload


def _check_model(model):
    """the last of the argument checks: every refusal above that names the model has been raised by now"""
    if model not in ("sage", "gat"):
        raise ValueError("model must be 'sage' or 'gat'")


def _own_nodes(workload, rank, world, num_nodes):
    """int64 ids of the nodes rank `rank` owns, ascending: the local row of a node is its position among them"""
    if workload is None:
        return np.arange(rank, num_nodes, world, dtype=np.int64)       # owner v % P holds v at local row v // P
    return np.flatnonzero(workload == rank).astype(np.int64)          # ascending: local row = rank among owned


def _host_rows(features, labels, own, world, fdt, multilabel, n_classes):
    """(f_own, l_own) on the host: the feature rows of the nodes `own` as a contiguous tensor of the stored type `fdt`, and
    their labels as int64 [n_own] or, multi-label, packed int32 words (aggr.pack_labels).  features / labels: callables of
    `own`, or arrays over all nodes (one part takes them whole)."""
    take = (lambda a: a(own)) if callable(features) else (lambda a: a[own] if world > 1 else a)
    f_own = take(features)
    if not torch.is_tensor(f_own):
        f_own = np.asarray(f_own)
        # (host arrays: float32 or float16 as they come, anything else through float32 as before)
        f_own = torch.from_numpy(np.ascontiguousarray(
            f_own, dtype=None if f_own.dtype in (np.float32, np.float16) else np.float32))
    if f_own.dtype not in (torch.float32, torch.float16, torch.bfloat16) or f_own.dim() != 2:
        raise ValueError("features: a float32, float16 or bfloat16 matrix expected")
    # converted on the HOST (round to nearest even), so that the device only ever holds the table in its stored type
    f_own = f_own.to(fdt).contiguous()
    n_own = own.shape[0]
    l_own = labels(own) if callable(labels) else (labels[own] if world > 1 else labels)
    if multilabel:
        if np.shape(l_own) != (n_own, n_classes):
            raise ValueError("multilabel=True: the rank's label rows must be [%d, %d], not %r"
                             % (n_own, n_classes, np.shape(l_own)))
        l_own = aggr.pack_labels(l_own)          # (ValueError for anything but 0 / 1)
    else:
        l_own = np.ascontiguousarray(l_own, dtype=np.int64)
    if f_own.shape[0] != n_own or l_own.shape[0] != n_own:
        raise ValueError("features / labels do not cover the rank's %d nodes" % n_own)
    return f_own, l_own


def _upload_table(f_own, dev):
    """(the resident table [n_own, F] on `dev`, whether it is a view of rows stored zero-padded).  The readers of a 16-bit
    table load whole quads of a row (8 bytes): a width that is no multiple of 4 is stored with its rows padded to one
    (zeros), which is also what lets inference read it in place."""
    n_own, F = f_own.shape
    if f_own.dtype == torch.float32 or F % 4 == 0:
        return f_own.to(dev), False
    wide = torch.zeros((n_own, (F + 3) // 4 * 4), dtype=f_own.dtype)
    wide[:, :F] = f_own
    return wide.to(dev)[:, :F], True


class Trainer(object):
    # result slots of the engine: round r lives in slot r % SLOTS.  Three, so that the slot the NEXT round is sliced
    # into was last read two rounds ago: waiting for that round's end event never drains the training stream (with
    # two slots the wait was for the steps just enqueued, an idle gap on the GPU once per round).
    SLOTS = 3

    def __init__(self, indptr, indices, features, labels, n_classes, rank=0, world=1, fanouts=(15, 10, 5),
                 batch=1024, streams=8, hidden=256, lr=1e-3, device=0, dist=None, seed=0, overlap=False,
                 model="sage", heads=8, rank_path=None, workload=None, feat_dim=None, rng_seed=5489,
                 feature_dtype="float32", gat_input=None, replace=True, dropout=0.0, dropout_seed=None,
                 multilabel=False, weight_decay=0.0, decoupled_weight_decay=True, decay_bias=False, max_grad_norm=None,
                 lr_schedule=None, class_weight=None, label_smoothing=0.0, feat_dropout=0.0, attn_dropout=0.0,
                 edge_weight=None, norm=None, norm_eps=1e-5):
        """Part `rank` of `world`.  Ownership = the engine's workload table (`workload` int32 [N], the METIS map of
        python/utils/sampler.py:64-134 / partition_map_opt.bin; None = v % world like pyfrontend.cpp:57): the rank
        keeps the feature and label rows of the nodes it owns, in ascending node order.

        features / labels: either host arrays over ALL nodes (float32 [N, F], int64 [N]; the rank copies its own
        rows) or callables `f(own_ids) -> rows` so that a rank never holds more than its share (papers100M:
        57 GB of features over 8 ranks); with a callable `features`, pass `feat_dim`.

        feature_dtype: "float32" (default), "float16" or "bfloat16": the element type of the resident feature table
        `self.feat`.  The rows (float32 or float16 numpy arrays, torch tensors of any of the three types) are stored as
        torch.as_tensor(rows).to(dtype), round to nearest even; a 16-bit table is half the HBM, no float32 copy of it
        is ever made on the device, and the deepest layer's forward -- and the first layer of evaluate() / predict() --
        reads it in place and upcasts in registers (exact), so the model is bitwise the one trained on the stored table
        upcast to float32.  A 16-bit table whose width
        is no multiple of 4 is stored with zero-padded rows; `self.feat` is then the [n_own, F] view of it.

        gat_input: whether the attention model's deepest layer runs aggregate-then-project on the raw feature rows
        (aggr.GatInputLayer, which reads a table of any of the three types in place).  None (default): on for a float32
        table where the layer covers the shape (aggr.gat_input_ok), off for a 16-bit table, whose runs keep the numbers
        they had (the two forms of the layer agree up to fp32 rounding only).  False: off.  True: on, for any table
        type; a ValueError names the reason where the layer cannot run (another model, more than one part or the rank
        path, a shape outside gat_input_ok, one of the A/B switches that take its prerequisites away).  `self.gat_input`
        is the outcome.

        replace: True (default): a row with at least `fanout` edges is sampled with replacement, the reference slicer's
        draw (slicer.cpp:10-21).  False: such a row yields `fanout` distinct edges (_abi.FLAG_NO_REPLACE: the same
        mt19937 words, mapped by Floyd's subset algorithm), the default of dgl.sampling.sample_neighbors that the
        reference's Python trainers sample with; every fanout must then be <= _abi.noreplace_max_fanout().

        dropout: probability in [0, 1) of dropping each element of every hidden layer's output (after its ReLU; the
        feature table and the last layer are not dropped: models/factory.py:41), kept elements scaled by 1 / (1 - p).
        GraphSAGE only.  The mask is a pure function of (dropout_seed, step, layer, node id, column) -- Philox4x32-10,
        include/cslicer_dropout.h -- with the step counted by `self.steps_done`, so that a node's mask never repeats
        across epochs and is the same on one GPU and on any number of ranks; dropout_seed=None takes `seed`.  0 (default)
        runs no dropout code at all; evaluate() / predict() never drop (inverted scaling makes inference the identity).

        norm: None (default) or "layer": layer normalisation of every GraphSAGE layer's result but the last, before its ReLU
        and dropout (SAGEConv's `norm`; torch.nn.LayerNorm over the hidden width, biased variance, norm_eps inside the root;
        DESIGN 4.13, include/cslicer_layernorm.h).  gamma_k (ones) and beta_k (zeros) are parameters behind the layers' own;
        they are clipped and all-reduced like every other and never weight-decayed, not even with decay_bias=True.  A
        function of one node's row only: the same numbers on one GPU and on any number of ranks, and evaluate() / predict()
        normalise with the same kernel.  GraphSAGE only, hidden % 4 == 0.  None runs none of that code.

        multilabel: False (default): one class per node, `labels` int [N], softmax cross-entropy.  True: a node carries a
        SET of classes (PPI, ogbn-proteins, Yelp, Amazon): `labels` is a host array [N, n_classes] of 0 / 1 (bool or
        integer), or a callable returning the rank's [n_own, n_classes] rows; they are packed on the host
        (aggr.pack_labels: 32 classes per int32 word) and `self.labels` is the int32 [n_own, ceil(n_classes / 32)] device
        tensor.  The loss is the mean binary cross-entropy with logits over the minibatch's seeds x classes
        (torch.nn.BCEWithLogitsLoss()): one fused HIP pass, inside the native step (csl_sage_fwd_bwd_multilabel) or as
        aggr.SigmoidBCE on the autograd paths, both models; on the rank path the autograd step runs (the native rank
        sequencer has no multi-label loss).  evaluate() then reports micro-F1.  Dropout, a 16-bit table and
        replace=False combine with it unchanged.

        weight_decay (default 0: none): the optimizer's weight decay (aggr.Adam, csl_adamw_f32).
        decoupled_weight_decay=True: AdamW's p <- p (1 - lr wd); False: the L2 term wd p added to the gradient
        (torch.optim.Adam(weight_decay=)).  decay_bias=False: only parameters with ndim >= 2 decay (the layers' weight
        matrices, the attention model's attn_l / attn_r), bias vectors do not; True: every parameter.
        max_grad_norm (default None: off): a number > 0 clips the gradient's global 2-norm to it
        (torch.nn.utils.clip_grad_norm_) and SKIPS, on the device, a step whose gradient holds a NaN or an Inf: weights and
        moments are left as they were.  float("inf"): the norm and the guard, never a clip.  On the rank path and in the
        data-parallel trainer the norm is that of the all-reduced gradient: the same on every rank, the weights stay
        replicated.  `self.opt.grad_norm` / `self.opt.skipped` (device tensors) hold the last norm and the skipped count.
        lr_schedule (default None: `lr` throughout): a callable steps_done -> learning rate, evaluated before every step
        and stored into `self.opt.lr` (lr_schedule() below builds warm-up + constant / cosine ones).

        class_weight (default None), label_smoothing (default 0.0): the options of the single-label loss (DESIGN 4.10,
        include/cslicer_loss.h).  class_weight: a sequence of n_classes finite numbers >= 0, at least one > 0 (0 with
        label_smoothing == 0 masks a class: no loss, no gradient; balanced_class_weight() below builds the usual
        n / (n_classes count_c)); label_smoothing in [0, 1).  The training loss of a minibatch is then
        F.cross_entropy(logits, y, weight=class_weight, label_smoothing=label_smoothing, reduction="sum") / seeds: the SUM
        over the seeds divided by their count, NOT torch's weighted "mean" (which divides by the sum of w[y]), so that the
        loss of a minibatch split over ranks is still the sum of the ranks' shares.  Every path computes it: the native steps
        (csl_sage_fwd_bwd_ce, csl_sage_rank_fwd_bwd_ce), aggr.SoftmaxCE on the autograd paths, torch's own loss for the
        attention model.  The options do not choose the path (step_plan does not see them).  With both at their defaults
        `self.loss_spec` is None and no new code runs.  evaluate()["loss"] stays the plain mean cross-entropy whatever
        the options.  multilabel=True refuses both: the sigmoid-BCE loss has no weights yet.

        feat_dropout, attn_dropout (default 0.0 both): the attention model's dropout (include/
        cslicer_gat_dropout.h), two independent probabilities in [0, 1), model="gat" only.  feat_dropout drops each element of
        every hidden layer's output after its ELU (the input of every layer but the deepest; the feature table is never
        dropped); attn_dropout drops each normalised attention coefficient alpha_h(u -> v) of every layer, inside the fused
        aggregation kernels (the softmax's numerator only).  Both masks are Philox4x32-10 of (dropout_seed, steps_done,
        layer, ...): the feature mask keyed by (node id, column) as `dropout`'s, the attention mask by (source node id,
        destination node id, head) -- so two sampled copies of one edge share a draw, and a run is the same on one GPU and
        on any number of parts.  attn_dropout > 0 takes the deepest layer off aggr.GatInputLayer (gat_input=None: off;
        gat_input=True: a ValueError); either above 0 runs a rank's layers node by node (the fused rank node has neither).
        At 0 / 0 no dropout code runs; evaluate() / predict() never drop.

        edge_weight (default None: every edge of a row alike): a host float array [num_edges] in the CSR's edge order, finite
        and >= 0 -- the `prob` argument of dgl.sampling.sample_neighbors.  A row with at least `fanout` edges then draws its
        `fanout` neighbours, with replacement, with probability proportional to the weights: the weights are
        quantised once on the host (l0.edge_cdf) and given to the engine (_abi.Engine.set_edge_cdf), which maps the same
        mt19937 words through the table.  A zero-weight edge of such a row is never drawn; a row with FEWER than `fanout`
        edges keeps all of them, zero-weight ones included: weights bias the draw, they do not filter the graph.  A row whose
        weights are all zero is drawn uniformly.  replace=False refuses it (weighted sampling without replacement is not
        built).  Everything behind the sampler is unchanged: the mean over the sampled neighbours stays a plain mean, and
        evaluate() / predict() stay full-neighbour and unweighted.  Every rank holds the whole table, as it holds the whole
        CSR.  None runs no new code.

        Persistence: save_checkpoint(path) writes the model, the optimizer state and `steps_done` to one file;
        load_checkpoint(path) fills them back in place, bitwise; skip(n_steps, first_batch) issues the engine submissions of
        run(n_steps, first_batch) without training, which is how a resumed run brings the sampler back to where the saved run
        stood (the engine's state is not in the file).  A trainer that calls none of the three runs no new code.

        `self.plan` is the StepPlan of the configuration (step_plan above): which step the trainer runs, decided here
        once; `self.native` / `self.native_rank` are the native stepper of that path, None on every other path."""
        # -- 1. the arguments (before any device call: a request that cannot be served is an error, never a quiet fall-back)
        N = indptr.shape[0] - 1
        self.n_classes = int(n_classes)
        self.multilabel = _check_labels(labels, multilabel, N, n_classes)
        dropout, feat_dropout, attn_dropout = _check_dropouts(model, hidden, dropout, feat_dropout, attn_dropout, gat_input)
        self.norm, self.norm_eps = _check_norm(model, hidden, len(fanouts), norm, norm_eps)
        weight_decay, max_grad_norm = _check_optimizer(weight_decay, max_grad_norm, lr_schedule)
        label_smoothing, class_weight = _check_loss(label_smoothing, class_weight, self.n_classes, self.multilabel)
        edge_weight = _check_sampling(edge_weight, replace, fanouts, np.shape(indices)[0])
        fdt = _check_table(feature_dtype, gat_input)
        # rank_path=True forces the one-process-per-part code (collectives included) even for a single part:
        # a way to run the RCCL calls on a one-GPU box
        self.rank_path = (world > 1) if rank_path is None else bool(rank_path)
        sw = read_switches()
        F_early = None
        if model == "gat":   # (the attention model's input width, known before the rows are loaded)
            F_early = features.shape[1] if feat_dim is None and not callable(features) else feat_dim
        _check_gat_input_on(gat_input, model, world, self.rank_path, len(fanouts), F_early, hidden, n_classes, heads,
                            fanouts[-1], sw)
        workload = _check_workload(workload, N, world)
        _check_model(model)
        self.dropout, self.dropout_seed = dropout, int(seed if dropout_seed is None else dropout_seed)
        self.feat_dropout, self.attn_dropout, self.lr_schedule = feat_dropout, attn_dropout, lr_schedule
        self.rank, self.world, self.dist = rank, world, dist
        # (kept for the record a checkpoint holds: checkpoint_fields)
        self.seed, self.rng_seed, self.feature_dtype = int(seed), int(rng_seed), feature_dtype
        self.fanouts = tuple(int(f) for f in fanouts)
        self.P = world
        self.N, self.B, self.S, self.L = N, batch, streams, len(fanouts)
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        # -- 2. the rank's nodes (ascending) and their rows, on the host; the owner table (None: v % P) is what rank-path
        # evaluation needs
        own = _own_nodes(workload, rank, world, N)
        self.own, self.owner, self.n_own = own, workload, own.shape[0]
        f_own, l_own = _host_rows(features, labels, own, world, fdt, self.multilabel, n_classes)
        F = f_own.shape[1] if feat_dim is None else feat_dim
        # -- 3. how this configuration trains, 4. the engine it needs.  One process per part: only this rank's slices are
        # materialised (the sampling itself is replicated)
        self.plan = step_plan_norm(self.norm, feat_dropout=feat_dropout, attn_dropout=attn_dropout, kind=model, world=world,
                                   rank_path=self.rank_path, n_layers=self.L, F=F, hidden=hidden, n_classes=n_classes,
                                   heads=heads, fanout=fanouts[-1], table_f32=fdt == torch.float32, gat_input=gat_input,
                                   replace=replace, sw=sw, width_known=F_early is not None, dropout=dropout,
                                   multilabel=self.multilabel)
        self.gat_input, self.replace = self.plan.gat_input, bool(replace)
        self.edge_weighted = edge_weight is not None
        cdf = l0.edge_cdf(indptr, edge_weight) if self.edge_weighted else None
        del edge_weight
        self.eng = _abi.Engine(indptr, indices, n_parts=self.P, fanouts=fanouts, max_batch=batch,
                               n_streams=streams, n_slots=self.SLOTS, device=device, mode=_abi.MODE_GRAPH,
                               workload=workload, part_mask=(1 << rank) if self.rank_path else 0,
                               flags=self.plan.engine_flags, rng_seed=rng_seed)
        if cdf is not None:
            self.eng.set_edge_cdf(cdf)
            del cdf
        # -- 5. the resident table and the model
        self.feat, self._feat_padded = _upload_table(f_own, self.dev)
        self.labels = torch.from_numpy(l_own).to(self.dev)
        del f_own, l_own
        # the single-label loss's options (None: the plain cross-entropy, the calls as they have always been)
        self.loss_spec = None
        if class_weight is not None or label_smoothing != 0.0:
            self.loss_spec = aggr.LossSpec(None if class_weight is None else
                                           torch.from_numpy(class_weight.astype(np.float32)).to(self.dev), label_smoothing)
        # global node id -> local row of the owner (-1 elsewhere); a single part holds every node at its own id
        self.local_row = None
        if self.P > 1:
            lr_ = np.full(N, -1, dtype=np.int32)
            lr_[own] = np.arange(self.n_own, dtype=np.int32)
            self.local_row = torch.from_numpy(lr_).to(self.dev)
        torch.manual_seed(seed)      # identical replicated weights on every rank
        self.kind = model
        if model == "sage":
            norm_kw = {} if self.norm is None else {"norm": self.norm, "norm_eps": self.norm_eps}
            self.model = splitgnn.DistSAGEModel(F, hidden, n_classes, n_layers=self.L, **norm_kw).to(self.dev)
        else:
            self.model = splitgnn.DistGATModel(F, hidden, n_classes, heads=heads, n_layers=self.L).to(self.dev)
        # -- 6. torch.optim.Adam's update in one HIP launch per step (the library's for-each form is eight small
        # launches, ~0.1 ms of GPU time per step; its fused form one of 42 us for these six small tensors)
        params = list(self.model.parameters())
        # (a normalised model's gamma and beta are never decayed, not even with decay_bias)
        undecayed = {id(p) for m in getattr(self.model, "norms", ()) for p in m.parameters()}
        self.opt = aggr.Adam(params, lr=lr, decoupled=bool(decoupled_weight_decay), max_grad_norm=max_grad_norm,
                             weight_decay=[weight_decay if (decay_bias or p.dim() >= 2) and id(p) not in undecayed else 0.0
                                           for p in params])
        # data-parallel replicas: called with the flat gradient, sums it over the ranks' shares of the minibatch
        self.grad_sync = None
        # rank path, autograd step: called with the flat gradient right after its all-reduce (what the optimizer applies)
        self.on_reduced_grads = None
        self.comm = splitgnn.DistComm(device=self.dev) if self.rank_path else None
        self.overlap = overlap
        # -- 7. the native stepper the plan names.  "native": the fused single-GPU GraphSAGE step as one native call per
        # minibatch.  "native_rank": the same idea with one process per part -- everything between two boundary exchanges
        # is issued by one native call, the exchanges come back as callbacks into self.comm, on its side stream with
        # overlap=True.  (CSLICER_PY_STEP=1: the same kernels issued from Python through autograd nodes, A/B switch and
        # what the tests compare the native steps with)
        self.native = self.native_rank = None
        if self.plan.path == "native":
            self.native = aggr.SageStep(self.model, splitgnn.ROW_PAD, splitgnn.SPLIT_K)
        elif self.plan.path == "native_rank":
            self.native_rank = aggr.SageRankStep(self.model, splitgnn.ROW_PAD, splitgnn.SPLIT_K, self.comm,
                                                 overlap=overlap)
        self._path_step = getattr(self, "_step_" + self.plan.path)
        # -- 8. the native steps write each loss into the next element of a ring (run() sizes it for its steps)
        self._loss_ring, self._ring_at = None, 0
        if self.native is not None or self.native_rank is not None:
            self._loss_ring = torch.zeros((4096,), dtype=torch.float32, device=self.dev)
        self.t_forward = self.t_slice = 0.0
        self.steps_done = 0
        self._round_base, self._slot_done, self._ahead = 0, [None] * self.SLOTS, None
        # units of the steps done (measurement only): per model layer k the output rows, source rows and edges
        self.units = [{"rows": 0, "src": 0, "edges": 0} for _ in range(self.L)]

    def set_nodes(self, nodes):
        self.eng.set_nodes(nodes)
        self.n_batches = (len(nodes) + self.B - 1) // self.B

    def _step(self, stream, slot):
        # ROCTX ranges = the reference's nvtx annotations (python/train.py:68, dist_sageconv.py:52-65)
        t0 = time.perf_counter()
        _roctx.push("slice")
        meta = self.eng.meta(stream, slot)
        slices = splitgnn.slices_of(self.eng, stream, slot, parts=[self.rank], device=self.dev, meta=meta)
        _roctx.pop()
        self.t_slice += time.perf_counter() - t0
        layers = [slices[self.L - 1 - k][self.rank] for k in range(self.L)]    # the rank's slices in MODEL order
        for u, sl in zip(self.units, layers):
            u["rows"] += sl.n_owned
            u["src"] += sl.n_in
            u["edges"] += sl.n_edges
        if self.lr_schedule is not None:
            self.opt.lr = float(self.lr_schedule(self.steps_done))
        loss = self._path_step(slices, layers, int(meta.n_seeds), stream, slot)    # (_step_<plan.path>)
        self.steps_done += 1
        return loss

    def _drop(self):
        """the DropSpec of the step about to run (its counter: the steps done so far), None without dropout"""
        return aggr.DropSpec(self.dropout, self.dropout_seed, self.steps_done) if self.dropout > 0 else None

    def _gat_drop(self):
        """the attention model's keyword for the step about to run: its GatDropSpec (counter: the steps done so far), or
        nothing without feat_dropout / attn_dropout, so that the call is the one it has been"""
        if not (self.feat_dropout > 0 or self.attn_dropout > 0):
            return {}
        return {"drop": aggr.GatDropSpec(self.feat_dropout, self.attn_dropout, self.dropout_seed, self.steps_done)}

    def _scale(self, den):
        """what the summed loss is multiplied by: 1 / seeds, and for the multi-label loss 1 / (seeds * classes), the
        mean over elements"""
        return 1.0 / (den * self.n_classes) if self.multilabel else 1.0 / den

    def _loss_kw(self):
        """the native steppers' `loss` keyword: absent without loss options, so that their call is the one it has been"""
        return {} if self.loss_spec is None else {"loss": self.loss_spec}

    def _loss_tail(self):
        """what follows `scale` in aggr.SoftmaxCE.apply with loss options (rowmap, class_weight, label_smoothing): nothing
        without them"""
        return () if self.loss_spec is None else (None, self.loss_spec.class_weight, self.loss_spec.label_smoothing)

    def _next_loss(self):
        """the loss ring's next element (run() sized the ring for its steps)"""
        loss = self._loss_ring[self._ring_at:self._ring_at + 1]
        self._ring_at += 1
        return loss

    def _input_rows(self, deep):
        """rows of self.feat that hold the deepest slice's input nodes (row v // P of the owner v % P, or the table's)"""
        return deep.in_nodes if self.local_row is None else self.local_row[deep.in_nodes.long()]

    def _step_native(self, slices, layers, n_seeds, stream, slot):
        # forward, loss, backward: one native call; the optimizer: a second one on the flat gradient buffer
        _roctx.push("step_native")
        loss = self._next_loss()
        self.native(layers, self.feat, self.labels, self._scale(self._loss_den(stream, slot, n_seeds)), loss, self._drop(),
                    **self._loss_kw())
        if self.grad_sync is not None:
            self.grad_sync(self.native.grads)             # (data-parallel: sum over the ranks' shares of the minibatch)
        self.opt.step(flat_grads=self.native.grads)
        _roctx.pop()
        return loss

    def _step_native_rank(self, slices, layers, n_seeds, stream, slot):
        _roctx.push("step_native_rank")
        loss = self._next_loss()
        top = layers[-1]
        seeds = top.out_nodes[top.owned_out_nodes.long()]              # the seeds this rank owns, frontier order
        self.native_rank(layers, self.feat, self._input_rows(layers[0]), seeds, self.local_row, self.labels,
                         1.0 / max(n_seeds, 1), loss, **self._loss_kw())
        self.dist.all_reduce(self.native_rank.grads)                   # replicated weights: sum of the ranks' shares
        self.opt.step(flat_grads=self.native_rank.grads)
        _roctx.pop()
        return loss

    def _step_local(self, slices, layers, n_seeds, stream, slot):
        # one GPU holding every node: the deepest layer reads the resident feature table through the slice's
        # in_nodes (no gathered input matrix), every layer is one fused node, the loss is one HIP pass
        t1 = time.perf_counter()
        _roctx.push("forward")
        logits = self.model.forward_local(slices, self.feat, drop=self._drop())
        loss_fn = aggr.SigmoidBCE if self.multilabel else aggr.SoftmaxCE
        loss = loss_fn.apply(logits, layers[-1].out_nodes, self.labels, self._scale(max(n_seeds, 1)), *self._loss_tail())
        _roctx.pop()
        self.t_forward += time.perf_counter() - t1
        return self._backward_and_update(loss)

    def _step_parts(self, slices, layers, n_seeds, stream, slot):
        # gather of owned input features, int32 indices, float4 row kernel
        _roctx.push("gather")
        rows = self._input_rows(layers[0])
        if self.plan.input_form == "table":
            x = aggr.FeatureRows(self.feat, rows)       # the deepest layer reads the table through in_nodes
        elif self.plan.input_form == "padded":
            x = aggr.padded_rows(rows.numel(), self.feat.shape[1], splitgnn.ROW_PAD, self.dev)
            aggr.gather_rows(self.feat, rows, out=x.t[:x.n])
        else:
            x = aggr.gather_rows(self.feat, rows)
        _roctx.pop()
        t1 = time.perf_counter()
        _roctx.push("forward")
        # (`dropout` is GraphSAGE's -- the constructor refuses the attention model with dropout > 0 -- and feat_dropout /
        # attn_dropout the attention model's)
        kw = {"drop": self._drop()} if self.kind == "sage" else self._gat_drop()
        if not self.rank_path:
            logits = self.model.forward_parts(slices, {0: x}, **kw)[0]
        elif self.kind == "gat":
            logits = self.model.forward_rank(slices, x, self.rank, self.comm, **kw)
        else:
            logits = self.model.forward_rank(slices, x, self.rank, self.comm, overlap=self.overlap, **kw)
        top = layers[-1]
        seeds = top.out_nodes[top.owned_out_nodes.long()]  # the seeds this rank owns, frontier order
        # mean over the WHOLE minibatch: sum of local losses / global seed count
        if self.multilabel:
            den = max(n_seeds, 1) if self.rank_path else self._loss_den(stream, slot, n_seeds)   # (data-parallel: global)
            loss = aggr.SigmoidBCE.apply(logits, seeds, self.labels, self._scale(den), self.local_row)
        elif self.kind == "sage" and logits.shape[0] > 0:
            loss = aggr.SoftmaxCE.apply(logits, seeds, self.labels, 1.0 / max(n_seeds, 1), self.local_row,
                                        *self._loss_tail()[1:])
        else:
            seeds = seeds.long()
            y = self.labels[seeds if self.P == 1 else self.local_row[seeds].long()]
            den = max(n_seeds, 1) if self.rank_path else self._loss_den(stream, slot, n_seeds)   # (data-parallel: global)
            kw = {} if self.loss_spec is None else {"weight": self.loss_spec.class_weight,
                                                    "label_smoothing": self.loss_spec.label_smoothing}
            loss = torch.nn.functional.cross_entropy(logits, y, reduction="sum", **kw) / den
        _roctx.pop()
        self.t_forward += time.perf_counter() - t1
        return self._backward_and_update(loss)

    def _flat_grads(self):
        """the parameters' gradients back to back (a rank whose share of the minibatch produced no gradient for a
        parameter still takes part: zeros)"""
        return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                          for p in self.model.parameters()])

    def _backward_and_update(self, loss):
        """the autograd paths' second half: backward, the gradients' reduction where there is one, the optimizer"""
        _roctx.push("backward")
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        _roctx.pop()
        # rank path: replicated weights, sum of the per-rank gradients.  Data-parallel replicas on the autograd path (GAT):
        # one all-reduce of the flat gradient, as the native step's
        reduce = self.dist.all_reduce if self.rank_path else self.grad_sync
        flat = None
        if reduce is not None:
            _roctx.push("grad_allreduce")
            flat = self._flat_grads()
            reduce(flat)
            if self.rank_path and self.on_reduced_grads is not None:
                self.on_reduced_grads(flat)
            _roctx.pop()
        _roctx.push("optimizer")
        self.opt.step(flat_grads=flat)                    # (the reduced buffer is used in place)
        _roctx.pop()
        return loss.detach()

    def run(self, n_steps, first_batch=0, then=None):
        """n_steps minibatches starting at minibatch `first_batch` of the node order (wrapping around the epoch),
        up to S per engine round; the next round is sliced while this one trains.  A round never crosses the end
        of the epoch: the last round of an epoch holds the remaining n_batches % S minibatches, the last of them
        possibly short -- every minibatch of the epoch is trained exactly once.

        then = (first_batch, n_steps) of the run() call that will follow: its first round is sliced while this call's
        last round trains, so the follow-up call starts without waiting for the slicer (the caller MUST make that call
        next: the round is already submitted and has advanced the streams' mt19937 positions)."""
        losses = []
        plan = shard.round_plan(self.n_batches, self.S, first_batch, n_steps)
        if not plan:
            return losses

        if self._loss_ring is not None:
            if self._loss_ring.numel() < n_steps:
                self._loss_ring = torch.zeros((n_steps,), dtype=torch.float32, device=self.dev)
            self._ring_at = 0
        ahead, self._ahead = self._ahead, None
        if ahead is not None and ahead != plan[0]:
            raise RuntimeError("run(then=...) announced the round %r, this call starts with %r" % (ahead, plan[0]))
        nxt = shard.round_plan(self.n_batches, self.S, then[0], then[1])[:1] if then else []
        # rounds keep rotating through the result slots from call to call (shard.round_walk)
        for what, entry, slot in shard.round_walk(plan, nxt, self._round_base, ahead, self.SLOTS):
            if what == "submit":
                self._submit_when_free(entry, slot)
                continue
            for s in range(entry[1]):
                losses.append(self._step(s, slot))
            ev = torch.cuda.Event()                       # behind the last step that reads the slot
            ev.record()
            self._slot_done[slot] = ev
        self._ahead = nxt[0] if nxt else None
        self._round_base = (self._round_base + len(plan)) % self.SLOTS
        torch.cuda.synchronize()
        return [float(x) for x in losses]

    def skip(self, n_steps, first_batch=0):
        """The engine submissions of run(n_steps, first_batch), and nothing else: the same rounds (shard.round_plan) into the
        same result slots, every stream's meta read (so an engine error or the frontier-overflow recovery surfaces as it
        does in a step), no minibatch trained, `steps_done` left alone.  What a resumed run calls for the minibatches the
        interrupted run had trained: a sequence of set_nodes / run calls with some run()s replaced by skip()s
        leaves the engine's mt19937 positions and the slot rotation where the original sequence does.  The next round is
        sliced while this one is waited for, as in run().  Returns the number of rounds submitted."""
        if self._ahead is not None:
            raise RuntimeError("skip(): run(then=...) has already submitted the round %r; the announced run() must follow"
                               % (self._ahead,))
        plan = shard.round_plan(self.n_batches, self.S, first_batch, n_steps)
        for what, entry, slot in shard.round_walk(plan, [], self._round_base, None, self.SLOTS):
            if what == "submit":
                self._submit_when_free(entry, slot)
                continue
            for s in range(entry[1]):
                self.eng.meta(s, slot)                    # waits for the round; raises what _step would
        self._round_base = (self._round_base + len(plan)) % self.SLOTS
        return len(plan)

    def _submit_when_free(self, entry, slot):
        """the round `entry` = (first minibatch, count) into result slot `slot`, once the last step that read the slot (a
        run()'s, recorded in _slot_done) has finished"""
        ev = self._slot_done[slot]
        if ev is not None:
            ev.synchronize()
            self._slot_done[slot] = None
        self._submit(entry[0], entry[1], slot)

    def _submit(self, first, n, slot):
        """minibatches [first, first + n) of the node order into result slot `slot`"""
        self.eng.submit_round(first, self.B, n, slot=slot)

    def _loss_den(self, stream, slot, n_seeds):
        """what the summed loss of this rank's seeds is divided by: the minibatch's seed count"""
        return max(n_seeds, 1)

    def reset_units(self):
        for u in self.units:
            u["rows"] = u["src"] = u["edges"] = 0

    def fused_deepest_layer(self):
        """whether the native step runs the deepest layer as the one fused gather -> fp32-MFMA kernel"""
        if self.plan.path != "native" or os.environ.get("CSLICER_NO_MFMA_FWD"):
            return False
        fout, fin2 = self.model.convs[0].fc.weight.shape
        return aggr._lib().csl_sage_fwd_mfma_scratch(fin2 // 2, fout) > 0

    def step_work(self, steps):
        """Algorithmic work of one training step on this rank (fp32), by the groups csl_sage_step_timing measures, from
        the slices actually trained (units per model layer k: m output rows, src source rows, e edges):
          gemm          flops of the library GEMMs: forward (k >= 1, or every layer when the deepest is not fused),
                        weight gradient (every layer), input gradient (k >= 1), 2 m 2in out each
          fused_forward the deepest layer as one kernel: 2 m 2in out flops; HBM bytes: (m + e) in 4 of gathered
                        feature-table rows (in 2 on a 16-bit table: the table's element size, here and in the two-kernel
                        form below) + m out 4 of result + m 2in 4 of operand kept for the weight gradient
          aggregation   HBM bytes of the gather kernels, every row counted ONCE (the per-edge re-reads of a layer's
                        sources are served by L2: the whole source matrix is a few tens of MB):
                        forward k >= 1: src in 4 read + m 2in 4 written; backward k >= 1 (by source): m 2in 4 read
                        + src in 4 (ReLU mask) read + src in 4 written
        The returned dict also has the totals `gemm_flops` (fused forward included) and `aggregation_bytes`."""
        fused = self.fused_deepest_layer()
        w = {"gemm": {"flops": 0.0}, "fused_forward": {"flops": 0.0, "bytes": 0.0}, "aggregation": {"bytes": 0.0}}
        esz = self.feat.element_size()
        for k, (u, conv) in enumerate(zip(self.units, self.model.convs)):
            if not hasattr(conv, "fc"):
                return None
            fout, fin2 = conv.fc.weight.shape
            fin = fin2 // 2
            m, src, e = u["rows"] / steps, u["src"] / steps, u["edges"] / steps
            g = 2.0 * m * fin2 * fout
            w["gemm"]["flops"] += g                                            # weight gradient
            if k > 0:
                w["gemm"]["flops"] += 2 * g                                    # forward + input gradient
                w["aggregation"]["bytes"] += (src * fin + m * fin2) * 4 + (m * fin2 + 2 * src * fin) * 4
            elif fused:
                w["fused_forward"]["flops"] += g
                w["fused_forward"]["bytes"] += (m + e) * fin * esz + m * fout * 4 + m * fin2 * 4
            else:
                w["gemm"]["flops"] += g
                w["aggregation"]["bytes"] += (m + e) * fin * esz + m * fin2 * 4
        w["gemm_flops"] = w["gemm"]["flops"] + w["fused_forward"]["flops"]
        w["aggregation_bytes"] = w["aggregation"]["bytes"] + w["fused_forward"]["bytes"]
        return w

    def report(self):
        n = max(self.steps_done, 1)
        # keys of python/train.py:101-103 (parsed by experiments/exp6/occ.py:21-23)
        out = ("avg forward time: %.6f sec\nbatch slice time: %.6f sec\ncache refresh time: %.6f sec"
               % (self.t_forward / n, self.t_slice / n, 0.0))
        if self.opt.grad_norm is not None:     # (clipping on: two more lines; reading the two elements waits for the stream)
            out += "\nlast gradient norm: %.6g\nskipped steps (non-finite gradient): %d" % (
                float(self.opt.grad_norm), int(self.opt.skipped))
        return out

    # -- evaluation: full-neighbour, layer-wise inference of the model as trained (cslicer.infer)
    def _infer_args(self):
        if self.rank_path and getattr(self, "comm", None) is None:
            raise NotImplementedError(
                "evaluation on the rank path runs collectively over the trainer's process group (one process per "
                "part, each with its own rows); this rank path trainer has none")
        return self.model, self.eng.indptr, self.eng.indices, self.feat

    def _infer_kw(self, nodes, chunk_rows):
        from . import infer
        return {"nodes": nodes, "chunk_rows": chunk_rows or infer.CHUNK_ROWS, "_zero_padded": self._feat_padded}

    def predict(self, nodes=None, chunk_rows=None):
        """float32 logits of the current weights by full-neighbour inference, enqueued on the training stream after every
        step already enqueued.  It neither submits to the engine nor draws random numbers nor touches the optimizer
        state.  Single process / data-parallel replica: [len(nodes) (or N), n_classes] (cslicer.infer.full_inference).
        Rank path: collective, every rank calls it with the same nodes; the logits of the rank's own nodes among `nodes`
        in `nodes` order, the rows owns(nodes) marks (cslicer.infer.full_inference_parts)."""
        from . import infer
        args, kw = self._infer_args(), self._infer_kw(nodes, chunk_rows)
        if self.rank_path:
            return infer.full_inference_parts(*args, self.comm, owner=self.owner, **kw)
        return infer.full_inference(*args, **kw)

    def owns(self, nodes):
        """bool mask over `nodes`: the nodes this rank owns, i.e. the rows predict(nodes) returns on the rank path"""
        from . import infer
        return infer.owns(self.N, self.P, self.rank, nodes, self.owner)

    def evaluate(self, nodes, chunk_rows=None):
        """{"accuracy", "loss", "n"} of the current weights on `nodes` (argmax accuracy, mean cross-entropy against the
        trainer's labels -- the PLAIN one: class_weight / label_smoothing shape the training loss only) by full-neighbour
        inference; see predict().  Rank path: collective, the same dict on every
        rank (cslicer.infer.evaluate_parts).  A multi-label trainer: {"micro_f1", "loss", "n", "tp", "fp", "fn"}
        (micro-F1 of logits > 0, mean binary cross-entropy per element)."""
        from . import infer
        args, kw = self._infer_args(), self._infer_kw(nodes, chunk_rows)
        if self.multilabel:
            kw["multilabel"] = True
        if self.rank_path:
            del kw["nodes"]
            return infer.evaluate_parts(*args, self.comm, nodes, self.labels, owner=self.owner, **kw)
        return infer.evaluate(*args, labels=self.labels, **kw)

    def correct_and_smooth(self, eval_nodes, train_nodes, **options):
        """{"accuracy", "base_accuracy", "n"} on `eval_nodes`: the argmax accuracy of the current weights' predictions
        after Correct and Smooth (cslicer.smooth.correct_and_smooth, DESIGN 4.14: the residuals of `train_nodes` against
        the trainer's labels spread over the graph, the corrected scores smoothed) and, as base_accuracy, before it.  The
        logits are predict()'s over all nodes; like it, this neither submits to the engine nor draws random numbers nor
        touches the optimizer state.  options: correct_and_smooth's keywords (num_correction_layers, correction_alpha,
        num_smoothing_layers, smoothing_alpha, autoscale, scale, chunk_rows).  ValueError, before any device work, for a
        multi-label trainer and on the rank path (propagation over split ranks is not built: DESIGN 8)."""
        if self.multilabel:
            raise ValueError("correct_and_smooth: a multi-label trainer has no one-hot labels to propagate (DESIGN 8)")
        if self.rank_path or self.n_own != self.N:
            raise ValueError("correct_and_smooth runs in a single process that holds every node's row; propagation on the "
                             "rank path is not built (DESIGN 8)")
        from . import infer, smooth
        ev, trn = infer._node_ids(eval_nodes), infer._node_ids(train_nodes)
        for ids in (ev, trn):
            if ids.size and (ids.min() < 0 or ids.max() >= self.N):
                raise ValueError("correct_and_smooth: nodes outside [0, %d)" % self.N)
        logits = self.predict()
        dev_ev, dev_trn = torch.from_numpy(ev).to(self.dev), torch.from_numpy(trn).to(self.dev)
        want = self.labels[dev_ev]
        scores = smooth.correct_and_smooth(logits, self.eng.indptr, self.eng.indices, trn, self.labels[dev_trn], nodes=ev,
                                           **options)
        n = int(ev.shape[0])
        plain, smoothed = infer.eval_head(logits[dev_ev], want)[1], infer.eval_head(scores, want)[1]
        return {"accuracy": smoothed / max(n, 1), "base_accuracy": plain / max(n, 1), "n": n}

    # -- persistence: one file (cslicer.checkpoint)
    def checkpoint_fields(self):
        """the `trainer` block of a checkpoint: where the run stands and what it was built with (plain values only)"""
        return {"steps_done": int(self.steps_done), "seed": self.seed, "dropout_seed": self.dropout_seed,
                "rng_seed": self.rng_seed, "fanouts": list(self.fanouts), "batch": int(self.B), "streams": int(self.S),
                "replace": self.replace, "world": int(self.world), "feature_dtype": self.feature_dtype,
                "dropout": self.dropout, "feat_dropout": self.feat_dropout, "attn_dropout": self.attn_dropout,
                "edge_weighted": self.edge_weighted, **({} if self.norm is None else {"norm": self.norm})}

    def _checkpoint_peers(self):
        """(whether this process writes the file, the torch.distributed module to meet the others at, or None)"""
        return self.rank == 0, (self.dist if self.world > 1 else None)

    def save_checkpoint(self, path, extra=None):
        """Write the model, the optimizer state and the run's position to `path` (cslicer.checkpoint.write: one file,
        atomically) after every step enqueued so far has finished.  extra: a dict of plain values kept in the file.  With
        more than one rank, rank 0 writes -- the weights are replicated -- and every rank returns after a barrier."""
        from . import checkpoint
        torch.cuda.synchronize()
        writer, dist = self._checkpoint_peers()
        try:
            if writer:
                checkpoint.write(path, self.model, optimizer=self.opt, trainer=self.checkpoint_fields(), extra=extra,
                                 multilabel=self.multilabel)
        finally:
            if dist is not None:
                dist.barrier()

    def load_checkpoint(self, path, optimizer=True):
        """Load the file save_checkpoint wrote; every rank reads it.  Its `model` block must be this trainer's architecture
        (ValueError naming the first differing field).  The parameters are filled in place (model.load_state_dict: the native
        steps and the optimizer alias their storage).  optimizer=True: the moments, opt.t, opt.skipped and `steps_done` --
        which keys the dropout masks and the learning-rate schedule -- are restored too, every one bitwise; the
        hyperparameters stay this trainer's.  optimizer=False: the weights only (fine-tuning, inference).  The sampler is
        not in the file: call set_nodes / skip for what the saved run had trained.
        Returns the file's (`trainer`, `extra`) dicts."""
        from . import checkpoint
        ck = checkpoint.read(path)
        checkpoint.check_model(ck["model"], checkpoint.model_block(self.model, self.multilabel))
        if optimizer and (ck["optimizer"] is None or ck["trainer"] is None):
            raise ValueError("checkpoint: %s holds a bare model, no optimizer state (load it with optimizer=False)" % path)
        if self._ahead is not None:
            raise RuntimeError("load_checkpoint(): run(then=...) has a round pending; the announced run() must follow")
        if optimizer:
            self.opt.check_state_dict(ck["optimizer"])       # (a refused load changes nothing)
        torch.cuda.synchronize()
        try:
            self.model.load_state_dict(ck["state"])
        except RuntimeError as ex:
            raise ValueError("checkpoint: the stored tensors are not this model's: %s" % str(ex).split("\n")[0])
        if optimizer:
            self.opt.load_state_dict(ck["optimizer"])
            self.steps_done = int(ck["trainer"]["steps_done"])
        torch.cuda.synchronize()
        return ck["trainer"], ck["extra"]

    def close(self):
        from . import infer
        infer.release(self.eng.indptr, self.eng.indices)   # the graph evaluation kept on the device, if any
        self.eng.close()


class DataParallelTrainer(Trainer):
    """The same model trained DATA-parallel: every GPU holds the whole graph and feature table (288 GB of HBM per
    MI355X: ogbn-products is 1.5 GB, papers100M 64 GB), samples and trains its 1/W share of every minibatch with the
    single-GPU native step (GraphSAGE; the attention model: the single-GPU autograd step with its fused layers), and one
    all-reduce (RCCL) sums the 0.7 MB of gradients.  Not the reference's design -- its
    trainer is split-parallel (python/train.py, `Trainer` above with world > 1) -- but what the same slicer + step give
    when a GPU is large enough to hold everything: no per-layer boundary exchange, the only collective is the gradient
    all-reduce.  A minibatch of B seeds is dealt in contiguous chunks of ceil(B / W); the loss is the sum over a
    rank's seeds / B, so the reduced gradient is the whole minibatch's (each chunk samples its own neighbourhoods)."""

    def __init__(self, indptr, indices, features, labels, n_classes, dp_rank, dp_world, dist, batch=1024, **kw):
        self.dp_rank, self.dp_world, self.dp_dist, self.global_B = int(dp_rank), int(dp_world), dist, int(batch)
        self.chunk = (self.global_B + self.dp_world - 1) // self.dp_world
        # every rank samples its OWN chunk of a minibatch: the ranks' mt19937 streams must differ, or rank r and rank r'
        # consume the same draws for their chunks and the sampling noise of the reduced gradient does not average out as
        # 1 / W (the split-parallel trainer is the opposite case: every rank must slice the SAME minibatch, same seed)
        kw.setdefault("rng_seed", 5489 + 7919 * self.dp_rank)
        super().__init__(indptr, indices, features, labels, n_classes, rank=0, world=1, batch=self.chunk, dist=None,
                         rank_path=False, **kw)
        if self.plan.path != "native" and self.kind != "gat":
            raise ValueError("the data-parallel trainer runs the native GraphSAGE step (feature and hidden widths "
                             "multiples of 4, at least two layers) or the single-GPU GAT step")
        if self.dp_world > 1:
            self.grad_sync = lambda flat: self.dp_dist.all_reduce(flat)
        self._den = {}

    def set_nodes(self, nodes):
        self.nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        self.n_batches = (len(self.nodes) + self.global_B - 1) // self.global_B

    def _submit(self, first, n, slot):
        mine = []
        for j in range(n):
            a, b, total = shard.dp_chunk(first + j, self.global_B, len(self.nodes), self.dp_rank, self.dp_world)
            mine.append(self.nodes[a:b])
            self._den[(j, slot)] = max(total, 1)
        self.eng.submit_seeds(mine, slot=slot)

    def _loss_den(self, stream, slot, n_seeds):
        return self._den[(stream, slot)]

    def _checkpoint_peers(self):
        # replicas: the first one writes (its rng_seed is the one recorded: DESIGN 8)
        return self.dp_rank == 0, (self.dp_dist if self.dp_world > 1 else None)

    def checkpoint_fields(self):
        # the job's values, not one replica's: the whole minibatch and the number of replicas
        return dict(super().checkpoint_fields(), batch=self.global_B, world=self.dp_world)


def balanced_class_weight(labels, n_classes):
    """float32 [n_classes]: n / (n_classes * count_c), the "balanced" class weights (sklearn's compute_class_weight) of the
    int labels given, computed in float64; a class no node carries gets 0.  For Trainer(class_weight=...)."""
    labels = np.asarray(labels).reshape(-1)
    if labels.size and (labels.min() < 0 or labels.max() >= n_classes):
        raise ValueError("labels must be in [0, n_classes = %d)" % n_classes)
    count = np.bincount(labels.astype(np.int64), minlength=n_classes).astype(np.float64)
    w = np.zeros(n_classes, dtype=np.float64)
    w[count > 0] = labels.size / (n_classes * count[count > 0])
    return w.astype(np.float32)


def lr_schedule(kind, base_lr, warmup=0, total=0, min_lr=0.0):
    """A learning-rate schedule for Trainer(lr_schedule=...): the callable t -> lr, t the steps done so far.
        t < warmup:  base_lr (t + 1) / warmup                       (linear warm-up; its last step runs at base_lr)
        then `constant`: base_lr;
             `cosine`:   min_lr + (base_lr - min_lr) (1 + cos(pi (t - warmup) / (total - warmup))) / 2 for t < total, half
                         a cosine from base_lr at the end of the warm-up down to min_lr at t = total, min_lr from there on."""
    if kind not in ("constant", "cosine"):
        raise ValueError("lr schedule kind must be 'constant' or 'cosine', not %r" % (kind,))
    base_lr, min_lr, warmup, total = float(base_lr), float(min_lr), int(warmup), int(total)
    if warmup < 0 or not base_lr > 0.0 or not 0.0 <= min_lr <= base_lr:
        raise ValueError("lr schedule: warmup >= 0 and 0 <= min_lr <= base_lr, base_lr > 0 expected")
    if kind == "cosine" and total <= warmup:
        raise ValueError("cosine lr schedule: total (%d) must exceed warmup (%d)" % (total, warmup))

    def at(t):
        if t < warmup:
            return base_lr * (t + 1) / warmup
        if kind == "constant":
            return base_lr
        if t >= total:
            return min_lr
        return min_lr + (base_lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (t - warmup) / (total - warmup)))
    return at


TUNED_GEMMS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_gfx950.csv")


def use_tuned_gemms(path=TUNED_GEMMS):
    """Let torch pick the library GEMM kernels recorded in `path` (PyTorch TunableOp results for the trainer's
    shapes on gfx950, written by profiles/tune_gemms.sh) instead of hipBLASLt's default heuristic: the deepest
    layer's forward GEMM runs in 81 us instead of 100, its weight gradient in 73 instead of 83.  Recorded
    selections only, no tuning at run time; shapes that are not in the file keep the default.  Process-wide."""
    if not os.path.exists(path) or not hasattr(torch.cuda, "tunable"):
        return False
    torch.cuda.tunable.enable(True)
    torch.cuda.tunable.tuning_enable(False)
    if hasattr(torch.cuda.tunable, "write_file_on_exit"):
        torch.cuda.tunable.write_file_on_exit(False)      # the recorded file is an input, never rewritten
    torch.cuda.tunable.set_filename(path)
    return True


def _mix64(x):
    """splitmix64 finaliser on uint64 arrays: a counter-based generator, so any subset of rows can be produced
    without the rows before it."""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def synthetic_node_data(num_nodes, feat_dim, n_classes, seed=0, rows=None):
    """features f32 U[0,1) and random labels (datasets are not available offline).  Every value is
    a hash of (seed, node id, column), so `rows` (node ids) yields exactly the rows of the full matrix: each
    rank generates only the nodes it owns."""
    ids = np.arange(num_nodes, dtype=np.uint64) if rows is None else np.asarray(rows).astype(np.uint64)
    base = np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    feats = np.empty((ids.shape[0], feat_dim), dtype=np.float32)
    step = max(1, (1 << 24) // max(feat_dim, 1))
    cols = np.arange(feat_dim, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        for lo in range(0, ids.shape[0], step):
            h = _mix64((ids[lo:lo + step, None] * np.uint64(feat_dim) + cols + base) * np.uint64(0x9E3779B97F4A7C15))
            feats[lo:lo + step] = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / (1 << 24))
        labels = (_mix64((ids + base) * np.uint64(0xD6E8FEB86659FD93)) % np.uint64(n_classes)).astype(np.int64)
    return feats, labels


def synthetic_multilabels(num_nodes, n_classes, seed=0, rows=None, feat_dim=128):
    """bool [len(rows) (or num_nodes), n_classes]: multi-label targets for synthetic_node_data's features of width
    `feat_dim` under the same seed.  Class c of node v is x[v, a] + x[v, b] - x[v, d] > 0.5 for three columns (a, b, d)
    fixed by c: a half-space of the node's OWN feature row (so a model can learn it), true for half of the nodes.  The
    features are hashes of (seed, node id, column), hence so are these: `rows` yields exactly the rows of the full
    matrix, and a rank generates only the nodes it owns."""
    x = synthetic_node_data(num_nodes, feat_dim, 1, seed=seed, rows=rows)[0]
    c = np.arange(n_classes)
    a, b, d = c % feat_dim, (3 * c + 1) % feat_dim, (5 * c + 2) % feat_dim
    return (x[:, a] + x[:, b] - x[:, d]) > np.float32(0.5)


def _parser():
    import argparse
    ap = argparse.ArgumentParser("split-parallel training on MI355X")
    ap.add_argument("--graph", type=str, default="synthetic")
    ap.add_argument("--log-every", type=int, default=20)
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--debug", type=bool, default=False)
    ap.add_argument("--cache-per", type=float)
    ap.add_argument("--model-name", default="gcn", help="gcn|gat")
    ap.add_argument("--num-epochs", type=int, default=2)
    ap.add_argument("--num-hidden", type=int, default=256)
    ap.add_argument("--num-layers", type=int, default=3)
    ap.add_argument("--num-heads", type=int, default=8)
    ap.add_argument("--fan-out", type=str, default="10,10,25")
    ap.add_argument("--batch-size", type=int, default=1032)
    ap.add_argument("--dropout", type=float, default=0)
    ap.add_argument("--feat-dropout", type=float, default=None,
                    help="(extra) --model-name gat: dropout on every hidden attention layer's output "
                         "(`Trainer(feat_dropout=...)`)")
    ap.add_argument("--attn-dropout", type=float, default=None,
                    help="(extra) --model-name gat: dropout on the normalised attention coefficients "
                         "(`Trainer(attn_dropout=...)`); --gat-input auto then turns the input layer off")
    ap.add_argument("--norm", choices=("layer",), default=None,
                    help="(extra) layer normalisation of every GraphSAGE layer's result but the last, before its ReLU "
                         "(`Trainer(norm='layer')`)")
    ap.add_argument("--norm-eps", type=float, default=None, metavar="E", help="(extra) --norm: eps inside the root (default 1e-5)")
    ap.add_argument("--max-steps", type=int, default=0, help="(extra) stop an epoch after this many minibatches")
    ap.add_argument("--partition", choices=("mod", "file"), default="mod",
                    help="(extra) node ownership: `mod` = v %% world (pyfrontend.cpp:57), `file` = the L0 directory's "
                         "partition_map_opt.bin (the METIS map of python/utils/sampler.py:64-134; its values must be "
                         "< the number of ranks)")
    ap.add_argument("--eval-split", choices=("none", "file", "holdout"), default="none",
                    help="(extra) node split for evaluation: none, the L0 directory's train_idx.bin / val_idx.bin, or a "
                         "seeded 80/20 holdout")
    ap.add_argument("--feature-dtype", choices=tuple(aggr.FEATURE_DTYPES), default=None,
                    help="(extra) element type of the feature table resident in HBM (default: float32, or what an L0 "
                         "directory's meta.txt says); a 16-bit table is half the memory and trains bitwise the model of "
                         "the same table upcast to float32")
    ap.add_argument("--gat-input", choices=("auto", "on", "off"), default="auto",
                    help="(extra) --model-name gat: the deepest layer as aggregate-then-project on the raw feature rows "
                         "(`Trainer(gat_input=...)`).  auto: on for a float32 table, off for a 16-bit one; on: for any "
                         "table type, an error where the layer cannot run; off: never")
    ap.add_argument("--no-replace", action="store_true",
                    help="(extra) sample rows with at least fan-out edges WITHOUT replacement (`Trainer(replace=False)`), "
                         "as dgl.sampling.sample_neighbors does by default; every fan-out must be <= 64")
    ap.add_argument("--edge-weight", type=str, default=None, metavar="FILE|l0|inv-degree",
                    help="(extra) edge-weighted neighbour sampling (`Trainer(edge_weight=...)`): FILE = a float32 binary of "
                         "num_edges numbers in CSR order, l0 = the L0 directory's edge_weight.bin, inv-degree = "
                         "1 / max(deg(source), 1) computed from the graph; not with --no-replace")
    ap.add_argument("--multilabel", action="store_true",
                    help="(extra) multi-label classification (`Trainer(multilabel=True)`): sigmoid + binary cross-entropy "
                         "over n_classes targets per node, evaluation by micro-F1; an L0 directory must say multilabel=1")
    ap.add_argument("--weight-decay", type=float, default=None,
                    help="(extra) the optimizer's weight decay (`Trainer(weight_decay=...)`), decoupled (AdamW) unless "
                         "--adam-l2; weight matrices only unless --decay-bias")
    ap.add_argument("--adam-l2", action="store_true",
                    help="(extra) --weight-decay as an L2 term of the gradient, torch.optim.Adam(weight_decay=)'s form "
                         "(`Trainer(decoupled_weight_decay=False)`)")
    ap.add_argument("--decay-bias", action="store_true", help="(extra) decay the bias vectors too (`Trainer(decay_bias=True)`)")
    ap.add_argument("--clip-grad-norm", type=float, default=None,
                    help="(extra) clip the gradient's global 2-norm to this value and skip a step whose gradient is not "
                         "finite (`Trainer(max_grad_norm=...)`); inf: the norm and the guard only")
    ap.add_argument("--lr-warmup", type=int, default=None, help="(extra) linear learning-rate warm-up over this many steps")
    ap.add_argument("--lr-schedule", choices=("constant", "cosine"), default=None,
                    help="(extra) after the warm-up: --lr throughout, or half a cosine down to --lr-min at the last step "
                         "of the last epoch (`train.lr_schedule`)")
    ap.add_argument("--lr-min", type=float, default=None, help="(extra) where the cosine schedule ends (default 0)")
    ap.add_argument("--label-smoothing", type=float, default=None, metavar="EPS",
                    help="(extra) label smoothing of the softmax cross-entropy, in [0, 1) (`Trainer(label_smoothing=EPS)`)")
    ap.add_argument("--class-weight", type=str, default=None, metavar="balanced|FILE",
                    help="(extra) per-class weights of the softmax cross-entropy (`Trainer(class_weight=...)`): `balanced` = "
                         "n / (n_classes * count_c) over the training nodes' labels, or a text file of n_classes numbers, "
                         "one per line")
    ap.add_argument("--save", type=str, default=None, metavar="FILE",
                    help="(extra) write a checkpoint (`Trainer.save_checkpoint`: model, optimizer state, position) to FILE "
                         "after every --save-every-th epoch and after the last one")
    ap.add_argument("--save-every", type=int, default=1, metavar="N", help="(extra) --save after every N-th epoch (default 1)")
    ap.add_argument("--resume", type=str, default=None, metavar="FILE",
                    help="(extra) continue the run that wrote FILE with --save: same command line, same --num-epochs; the "
                         "epochs it had finished are replayed through the slicer only (`Trainer.skip`), not trained")
    ap.add_argument("--correct-smooth", action="store_true",
                    help="(extra) after every evaluation, Correct and Smooth (`Trainer.correct_and_smooth`): label propagation "
                         "of the training nodes' residuals and labels over the graph; needs --eval-split, one process")
    from . import smooth
    smooth.add_options(ap)
    return ap


def _optimizer_kw(a, steps_per_epoch):
    """the Trainer keywords of the optimizer options, each only where its option was given"""
    kw = {}
    if a.weight_decay is not None:
        kw["weight_decay"] = a.weight_decay
    if a.adam_l2:
        kw["decoupled_weight_decay"] = False
    if a.decay_bias:
        kw["decay_bias"] = True
    if a.clip_grad_norm is not None:
        kw["max_grad_norm"] = a.clip_grad_norm
    if a.lr_warmup is not None or a.lr_schedule is not None or a.lr_min is not None:
        kw["lr_schedule"] = lr_schedule(a.lr_schedule or "constant", a.lr, warmup=a.lr_warmup or 0,
                                        total=a.num_epochs * steps_per_epoch, min_lr=a.lr_min or 0.0)
    return kw


def _loss_kw(a, labels, train_nodes, n, n_classes):
    """the Trainer keywords of --label-smoothing / --class-weight, each only where its option was given.  `balanced`
    counts the labels of the training nodes of the WHOLE job (labels(ids) serves any id on any rank): every rank gets the
    same vector."""
    kw = {}
    if a.label_smoothing is not None:
        kw["label_smoothing"] = a.label_smoothing
    if a.class_weight == "balanced":
        ids = np.arange(n, dtype=np.int64) if train_nodes is None else np.asarray(train_nodes, dtype=np.int64)
        kw["class_weight"] = balanced_class_weight(labels(ids), n_classes)
    elif a.class_weight is not None:
        kw["class_weight"] = np.loadtxt(a.class_weight, dtype=np.float64, ndmin=1)
    return kw


def _split(a, n):
    """(train nodes, evaluation nodes) of --eval-split; (None, None) for `none`"""
    from . import l0
    if a.eval_split == "none":
        return None, None
    if a.eval_split == "file":
        if a.graph == "synthetic" or a.graph in l0.PRESETS:
            raise SystemExit("--eval-split file needs an L0 directory")
        sp = l0.read_splits(a.graph)
        if sp is None:
            raise SystemExit("--eval-split file: %s has no train_idx.bin / val_idx.bin" % a.graph)
        return sp
    perm = np.random.default_rng(0).permutation(n)          # seeded, as the reference converter's 80/20 split
    cut = int(n * 0.8)
    return np.sort(perm[:cut]), np.sort(perm[cut:])


# ---- the stages of main(), in the order it calls them

def _refuse_early(a):
    """the refusals that need the command line only, before anything is loaded"""
    if a.multilabel and (a.label_smoothing is not None or a.class_weight is not None):
        raise SystemExit("--multilabel: --label-smoothing and --class-weight belong to the single-label loss (the sigmoid-BCE "
                         "loss has no weights yet)")
    if a.edge_weight is not None and a.no_replace:
        raise SystemExit("--edge-weight: weighted sampling draws with replacement and does not combine with --no-replace "
                         "(weighted sampling without replacement is not built)")
    if a.no_replace:
        lim = _abi.noreplace_max_fanout()
        if any(int(x) > lim for x in a.fan_out.split(",")):
            raise SystemExit("--no-replace: --fan-out %s exceeds the limit of %d neighbours per row" % (a.fan_out, lim))
    if a.save is not None and (a.save_every < 1 or not os.path.isdir(os.path.dirname(os.path.abspath(a.save)))):
        raise SystemExit("--save %s: --save-every must be >= 1 and the file's directory must exist" % a.save)
    from . import smooth
    if smooth.options_of(a) is not None:
        if a.eval_split == "none":
            raise SystemExit("--correct-smooth propagates the training nodes' labels to the evaluation nodes: it needs --eval-split")
        if a.multilabel:
            raise SystemExit("--correct-smooth: a multi-label run has no one-hot labels to propagate")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("--correct-smooth runs in a single process (propagation over split ranks is not built)")


def _resume_epochs(a):
    """the finished epochs that --resume's file records (0 without --resume): the file is checked before the graph is loaded"""
    if a.resume is None:
        return 0
    from . import checkpoint
    if not os.path.isfile(a.resume):
        raise SystemExit("--resume %s: no such file" % a.resume)
    try:
        epochs_done = checkpoint.read(a.resume)["extra"].get("epoch")
    except ValueError as ex:
        raise SystemExit("--resume %s: %s" % (a.resume, ex))
    if not isinstance(epochs_done, int) or isinstance(epochs_done, bool) or epochs_done < 0:
        raise SystemExit("--resume %s: the file records no finished epochs (it was not written by --save)" % a.resume)
    return epochs_done


def _process_group():
    """(rank, world, local rank, torch.distributed or None) of the torchrun environment; with more than one process the
    group is initialised here"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        dist.init_process_group(backend=os.environ.get("CSLICER_DIST_BACKEND", "nccl"))
    return rank, world, local, dist


# what --graph names: feats / labels are callables own ids -> rows, so that every rank generates or reads (memory-mapped)
# only the rows of the nodes it owns; fdim, fdtype: the table's width and the element type it is kept in; workload: the
# owner table of --partition file, else None
_Graph = collections.namedtuple("_Graph", "indptr indices feats labels n_classes fdim fdtype workload")


def _load_graph(a):
    """the _Graph of --graph: `synthetic` or a preset (generated), or an L0 directory (read)"""
    if a.graph == "synthetic" or a.graph in l0.PRESETS:
        n, d, fdim, n_classes = (200_000, 20.0, 128, 40) if a.graph == "synthetic" else l0.PRESETS[a.graph]
        indptr, indices = l0.synth_graph(n, d, seed=0)
        feats = lambda own: synthetic_node_data(n, fdim, n_classes, seed=0, rows=own)[0]    # noqa: E731
        labels = lambda own: synthetic_node_data(n, 1, n_classes, seed=0, rows=own)[1]      # noqa: E731
        if a.multilabel:
            labels = lambda own: synthetic_multilabels(n, n_classes, seed=0, rows=own, feat_dim=fdim)   # noqa: E731
        if a.partition == "file":
            raise SystemExit("--partition file needs an L0 directory")
        return _Graph(indptr, indices, feats, labels, n_classes, fdim, a.feature_dtype or "float32", None)
    indptr, indices, meta = l0.read_l0(a.graph, mmap=False)
    n, n_classes = meta["num_nodes"], meta["num_classes"]
    fmap, stored = l0.read_features(a.graph, meta)          # (in the stored element type)
    if bool(meta.get("multilabel")) != bool(a.multilabel):
        raise SystemExit("--multilabel needs an L0 directory whose meta.txt says multilabel=1 (%s does not)" % a.graph
                         if a.multilabel else
                         "%s is a multi-label directory (multilabel=1 in its meta.txt): pass --multilabel" % a.graph)
    lmap = (l0.read_labels(a.graph, meta) if a.multilabel else
            np.memmap(os.path.join(a.graph, "labels.bin"), dtype=np.int32, mode="r", shape=(n,)))
    feats = lambda own: l0.feature_rows(fmap[own], stored)                                # noqa: E731
    labels = lambda own: np.asarray(lmap[own]).astype(np.int64)                          # noqa: E731
    if a.multilabel:
        labels = lambda own: l0.unpack_labels(np.asarray(lmap[own]), n_classes)              # noqa: E731
    workload = None
    if a.partition == "file":
        workload = np.fromfile(os.path.join(a.graph, "partition_map_opt.bin"), dtype=np.int32)
    return _Graph(indptr, indices, feats, labels, n_classes, meta["feature_dim"], a.feature_dtype or stored, workload)


def _edge_weight(a, indptr, indices):
    """the host edge weights --edge-weight names, None without it"""
    if a.edge_weight == "inv-degree":
        return l0.inv_degree_weights(indptr, indices)
    if a.edge_weight == "l0":
        if a.graph == "synthetic" or a.graph in l0.PRESETS:
            raise SystemExit("--edge-weight l0 needs an L0 directory")
        return l0.read_edge_weight(a.graph)
    if a.edge_weight is not None:
        if os.path.getsize(a.edge_weight) != 4 * indices.shape[0]:
            raise SystemExit("--edge-weight %s: %d bytes, the graph's %d edges need %d (float32 each)"
                             % (a.edge_weight, os.path.getsize(a.edge_weight), indices.shape[0], 4 * indices.shape[0]))
        return np.fromfile(a.edge_weight, dtype="<f4")
    return None


def _trainer_kw(a, g, train_nodes, steps_per_epoch, edge_weight):
    """every optional Trainer keyword of the command line, each only where its option was given: the place where a new
    option adds its line"""
    kw = {"multilabel": True} if a.multilabel else {}
    kw.update(_optimizer_kw(a, steps_per_epoch))
    if a.feat_dropout is not None:
        kw["feat_dropout"] = a.feat_dropout
    if a.attn_dropout is not None:
        kw["attn_dropout"] = a.attn_dropout
    if a.norm is not None:
        kw["norm"] = a.norm
    if a.norm_eps is not None:
        kw["norm_eps"] = a.norm_eps
    kw.update(_loss_kw(a, g.labels, train_nodes, g.indptr.shape[0] - 1, g.n_classes))
    if edge_weight is not None:
        kw["edge_weight"] = edge_weight
    return kw


def _start_epoch(a, tr, train_nodes, epoch):
    """the epoch's node order (a pure function of its number) into the trainer; returns its minibatches"""
    if train_nodes is None:
        tr.set_nodes(np.random.default_rng(epoch).permutation(tr.N))
    else:
        tr.set_nodes(train_nodes[np.random.default_rng(epoch).permutation(train_nodes.shape[0])])
    return tr.n_batches if a.max_steps <= 0 else min(a.max_steps, tr.n_batches)


def _resume(a, tr, epochs_done, train_nodes, rank):
    """--resume: the file into the trainer, the sampler back to its position -- the finished epochs through the slicer,
    nothing trained -- and rank 0's report"""
    try:
        was, _ = tr.load_checkpoint(a.resume)
    except ValueError as ex:
        raise SystemExit("--resume %s: %s" % (a.resume, ex))
    left = epochs_done < a.num_epochs        # (nothing to continue: nothing to replay)
    replayed = 0
    for e in range(epochs_done if left else 0):
        steps = _start_epoch(a, tr, train_nodes, e)
        tr.skip(steps)
        replayed += steps
    if rank != 0:
        return
    print("resumed from %s: epoch %d, %d steps" % (a.resume, epochs_done, tr.steps_done))
    now = tr.checkpoint_fields()
    odd = ["%s was %r, is %r" % (k, was[k], now[k]) for k in sorted(now)
           if k not in ("steps_done", "world") and k in was and was[k] != now[k]]
    if left and replayed != tr.steps_done:
        odd.append("the file holds %d steps, %d epochs of this command line are %d" % (tr.steps_done, epochs_done, replayed))
    for line in odd:
        print("resume: %s: the continuation will not be the uninterrupted run's" % line)
    if not left:
        print("resume: the file holds %d epochs and --num-epochs is %d: nothing is left to train"
              % (epochs_done, a.num_epochs))


def _train_epochs(a, tr, first_epoch, train_nodes, eval_nodes, rank):
    """epochs first_epoch .. --num-epochs - 1: train, --save and evaluate where they are due"""
    for epoch in range(first_epoch, a.num_epochs):
        steps = _start_epoch(a, tr, train_nodes, epoch)
        t0 = time.time()
        losses = tr.run(steps)
        if rank == 0:
            print("epoch %d: %d minibatches in %.2f s, loss %.4f -> %.4f" % (epoch, steps, time.time() - t0, losses[0], losses[-1]))
        if a.save is not None and ((epoch + 1) % a.save_every == 0 or epoch + 1 == a.num_epochs):
            tr.save_checkpoint(a.save, extra={"epoch": epoch + 1})
        if eval_nodes is not None and ((epoch + 1) % max(a.eval_every, 1) == 0 or epoch + 1 == a.num_epochs):
            t0 = time.time()
            ev = tr.evaluate(eval_nodes)
            if rank == 0:
                # the key of the reference's trainers (pa_cache_multi_gpu.py:252)
                if a.multilabel:
                    print("Eval F1 %.4f | loss %.4f | %d nodes in %.2f s" % (ev["micro_f1"], ev["loss"], ev["n"], time.time() - t0))
                else:
                    print("Eval Acc %.4f | loss %.4f | %d nodes in %.2f s" % (ev["accuracy"], ev["loss"], ev["n"], time.time() - t0))
            if a.correct_smooth:
                from . import smooth
                t0 = time.time()
                cs = tr.correct_and_smooth(eval_nodes, train_nodes, **smooth.options_of(a))
                if rank == 0:
                    print("Eval Acc C&S %.4f (plain %.4f) | %d nodes in %.2f s" % (cs["accuracy"], cs["base_accuracy"], cs["n"], time.time() - t0))


def main(argv=None):
    """Command line with the argument names of the reference's python/train.py:109-131 (same spelling, same
    defaults where they apply); one process per GPU under torchrun, or a single process.

        python -m cslicer.train --graph synthetic --model-name gcn --fan-out 5,10,15 --batch-size 1024
        python -m torch.distributed.run --nproc-per-node 4 --master-addr 127.0.0.1 -m cslicer.train --graph <L0 dir>

    --fan-out follows the reference (DGL) convention, input side first (python/train.py:128,
    batch_slice_multi_gpu.py:202): the LAST number is the hop from the seeds.  --graph: an L0 directory
    (cslicer.l0), a preset name (arxiv-like, products-like, papers-like) or `synthetic`.
    --dropout: `Trainer(dropout=...)`, between the GraphSAGE layers as models/factory.py:41 applies it (the default, 0,
    runs none; the attention model refuses a value above 0).
    --norm layer [--norm-eps E] (extra): `Trainer(norm="layer", norm_eps=E)`: layer normalisation of every GraphSAGE layer's
    result but the last, before its ReLU and dropout; without it no norm code runs; the attention model refuses it.
    --feat-dropout P, --attn-dropout P (extra): `Trainer(feat_dropout=P)`, `Trainer(attn_dropout=P)`, --model-name gat only:
    dropout on every hidden attention layer's output (after its ELU) and on the normalised attention coefficients (DESIGN
    4.11); both keyed by the run's seed and the step.  --attn-dropout above 0 takes the deepest layer off the
    aggregate-then-project input layer (--gat-input auto: off; --gat-input on: an error).
    Accepted and ignored (no counterpart here): --cache-per (features are resident in HBM), --num-workers,
    --debug, --log-every.
    --eval-split (extra): `none` (default) trains on every node and never evaluates; `file` trains on the L0 directory's
    train_idx.bin and evaluates val_idx.bin; `holdout` trains on a seeded 80 % of the nodes and evaluates the other
    20 %.  With a split the model is evaluated by full-neighbour inference every --eval-every epochs and after the last
    one; with one process per part every rank takes part (each holds only its own rows) and rank 0 prints `Eval Acc`.
    --feature-dtype (extra): float32, float16 or bfloat16, the element type of the feature table kept in HBM
    (`Trainer(feature_dtype=...)`).  Default: float32, or with an L0 directory what its meta.txt records
    (feature_dtype=, cslicer.l0.write_l0); features.bin is memory-mapped in its stored type and, where the two differ,
    the rank's rows are converted on load.
    --gat-input (extra): auto (default), on or off, `Trainer(gat_input=...)`: whether the attention model's deepest layer
    aggregates the raw feature rows before it projects.  auto keeps a 16-bit table on the project-then-aggregate path.
    --no-replace (extra): `Trainer(replace=False)`: a row with at least fan-out edges yields that many DISTINCT edges
    (the default of dgl.sampling.sample_neighbors) instead of independent draws.  Every --fan-out number must then be
    <= 64 (_abi.noreplace_max_fanout()).
    --edge-weight FILE|l0|inv-degree (extra): `Trainer(edge_weight=...)`: a row with at least fan-out edges draws its
    neighbours with probability proportional to the edge weights (with replacement).  FILE = a float32 binary of
    num_edges numbers in the CSR's edge order, `l0` = the --graph directory's edge_weight.bin (cslicer.l0.write_edge_weight),
    `inv-degree` = w(v <- u) = 1 / max(deg(u), 1) computed from the graph, which gives `synthetic` and the presets a
    weighted run without a file.  Weights bias the draw, they do not filter the graph: a shorter row keeps all its edges,
    zero-weight ones included.  Evaluation stays full-neighbour and unweighted.  Not with --no-replace.
    --weight-decay W [--adam-l2] [--decay-bias] (extra): `Trainer(weight_decay=W)`: AdamW's decoupled decay of the weight
    matrices; --adam-l2: as an L2 term of the gradient instead; --decay-bias: the bias vectors too.
    --clip-grad-norm M (extra): `Trainer(max_grad_norm=M)`: the gradient's global norm is clipped to M, and a step whose
    gradient holds a NaN or an Inf is skipped on the device; the report then ends with the last norm and the skipped count.
    --lr-warmup K, --lr-schedule {constant,cosine}, --lr-min (extra): `Trainer(lr_schedule=train.lr_schedule(...))` with
    --lr as the base rate and total = --num-epochs x the minibatches of an epoch (--max-steps where it is smaller).
    --multilabel (extra): `Trainer(multilabel=True)`: a node carries a set of classes; the loss is the mean binary
    cross-entropy with logits and rank 0 prints `Eval F1` (micro-F1) where it prints `Eval Acc`.  `synthetic` and the
    presets train on synthetic_multilabels; an L0 directory must hold packed multi-label words (multilabel=1 in its
    meta.txt, cslicer.l0.write_l0 with a 2-D `labels`).
    --label-smoothing EPS (extra): `Trainer(label_smoothing=EPS)`, EPS in [0, 1).
    --class-weight balanced|FILE (extra): `Trainer(class_weight=...)`: `balanced` = n / (n_classes * count_c) over the labels
    of the training nodes (train.balanced_class_weight; a class without a node gets 0), FILE = n_classes numbers, one per
    line.  The training loss is the weighted, smoothed sum over a minibatch's seeds divided by their count; `Eval Acc`'s
    loss stays the plain mean cross-entropy.  Neither combines with --multilabel (the sigmoid-BCE loss has no weights yet).
    --save FILE [--save-every N] (extra): `Trainer.save_checkpoint(FILE, extra={"epoch": epochs done})` after every N-th
    epoch (default 1) and after the last one: the model, the optimizer state and the run's position in one file, written
    atomically by rank 0 (cslicer.checkpoint).  `python -m cslicer.predict --model FILE` applies the model.
    --resume FILE (extra): continue the run that wrote FILE.  The file is checked before the graph is loaded.  The weights,
    the moments and the step count come from the file; the sampler is brought back by replaying the finished epochs through
    the slicer without training them (`Trainer.skip`; an epoch's node order is a function of its number), and the epoch
    loop continues where the file ends.  Give the command line of the original run, --num-epochs included (it still means
    the whole run, and it is what --lr-schedule spans): the continuation is then the uninterrupted run's: bit for bit on the
    native GraphSAGE step where the new process's library GEMMs run the algorithms the old one's ran (csl_gemm_f32 picks one per
    shape class, from the recorded plans or else by timing: DESIGN 4.12), otherwise equal up to float32 summation order.  Rank 0 prints `resumed from FILE: epoch E, S steps`, and one line for every recorded setting
    (fan-outs, batch size, --no-replace, ...) the command line changes: such a run continues, but as another run.  A file that already
    holds --num-epochs epochs is reported (`nothing is left to train`) and not replayed.
    --correct-smooth [--cs-layers T1,T2] [--cs-alpha A1,A2] [--cs-scale auto|NUMBER] (extra): after every `Eval Acc` line rank 0
    prints `Eval Acc C&S %.4f (plain %.4f) | %d nodes in %.2f s`: `Trainer.correct_and_smooth` on the evaluation nodes, with the
    training nodes' labels (defaults 50,50 / 0.8,0.8 / auto).  Needs --eval-split; not with --multilabel, one process.

        python -m cslicer.train --graph products-like --num-epochs 20 --eval-split holdout --save run.ckpt
        python -m cslicer.train --graph products-like --num-epochs 20 --eval-split holdout --save run.ckpt --resume run.ckpt
        python -m cslicer.train --graph products-like --class-weight balanced --label-smoothing 0.1 --eval-split holdout --max-steps 50
        python -m cslicer.train --graph products-like --multilabel --eval-split holdout --max-steps 50
        python -m cslicer.train --graph products-like --edge-weight inv-degree --eval-split holdout --max-steps 50
        python -m cslicer.train --graph products-like --dropout 0.5 --weight-decay 5e-4 --clip-grad-norm 1 --lr-warmup 100 --lr-schedule cosine
        python -m cslicer.train --graph products-like --norm layer --dropout 0.5 --lr-warmup 100 --lr-schedule cosine
        python -m cslicer.train --graph <L0 dir> --feature-dtype bfloat16 --eval-split holdout
        python -m cslicer.train --graph products-like --eval-split holdout --correct-smooth --cs-layers 50,50 --cs-alpha 0.8,0.8
        python -m cslicer.train --graph products-like --model-name gat --feature-dtype bfloat16 --gat-input on
        python -m cslicer.train --graph products-like --model-name gat --feat-dropout 0.6 --attn-dropout 0.6 --eval-split holdout"""
    a = _parser().parse_args(argv)
    _refuse_early(a)
    epochs_done = _resume_epochs(a)
    rank, world, local, dist = _process_group()
    g = _load_graph(a)
    edge_weight = _edge_weight(a, g.indptr, g.indices)
    n = g.indptr.shape[0] - 1
    train_nodes, eval_nodes = _split(a, n)
    fan = tuple(int(x) for x in a.fan_out.split(","))[::-1]          # engine order: layer 0 = hop from the seeds
    if len(fan) != a.num_layers:
        fan = fan[:a.num_layers] if len(fan) > a.num_layers else fan
    n_train = n if train_nodes is None else train_nodes.shape[0]
    per_epoch = (n_train + a.batch_size - 1) // a.batch_size           # (Trainer.set_nodes' n_batches)
    per_epoch = per_epoch if a.max_steps <= 0 else min(a.max_steps, per_epoch)
    kind = "gat" if a.model_name == "gat" else "sage"
    hidden = a.num_hidden // a.num_heads if kind == "gat" else a.num_hidden
    tr = Trainer(g.indptr, g.indices, g.feats, g.labels, g.n_classes, rank=rank, world=world, fanouts=fan,
                 batch=a.batch_size, streams=8, hidden=max(4, hidden // 4 * 4), lr=a.lr, device=local, dist=dist, model=kind,
                 heads=a.num_heads, workload=g.workload, feat_dim=g.fdim, feature_dtype=g.fdtype,
                 gat_input={"auto": None, "on": True, "off": False}[a.gat_input], replace=not a.no_replace,
                 dropout=a.dropout, **_trainer_kw(a, g, train_nodes, per_epoch, edge_weight))
    del edge_weight
    if rank == 0 and g.fdtype != "float32":
        print("feature table: %s, %d bytes on this rank" % (g.fdtype, tr.feat.numel() * tr.feat.element_size()))
    if a.resume is not None:
        _resume(a, tr, epochs_done, train_nodes, rank)
    _train_epochs(a, tr, epochs_done, train_nodes, eval_nodes, rank)
    if rank == 0:
        print(tr.report())
    tr.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
