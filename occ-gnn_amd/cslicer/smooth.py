"""Correct and Smooth: full-graph label propagation over a model's predictions (include/cslicer_smooth.h).

After `full_inference` the user holds the logits of every node, the labels of the training nodes and the neighbour CSR on
the device.  Correct and Smooth (Huang et al. 2020, "Combining label propagation and simple models out-performs graph
neural networks"; PyG's CorrectAndSmooth, DGL's correct_and_smooth example) combines them without retraining: the
residual errors of the training nodes are spread over the graph and added to the predictions (correct), then the
corrected predictions, with the training rows set to their labels, are smoothed.

    S = D^-1/2 A D^-1/2      A: the neighbour CSR of cslicer.infer (self loops removed, duplicates counted),
                             deg[v] the length of row v, dinv[v] = deg[v] > 0 ? 1 / sqrt(deg[v]) : 0, on BOTH sides
    prop(X0, alpha, T, lo, hi, fix):  X = X0;  T times:  X = clamp(alpha S X + (1 - alpha) X0, lo, hi), X[rows] = values

For a symmetric graph S is the symmetric normalised adjacency.  For a directed one it is this definition as it stands:
row v gathers the sources of CSR row v and both factors come from row lengths (in-degrees of the stored direction).

The hot path is csl_prop_f32 (csrc/smooth.hip): one gather pass per iteration over the work list of cslicer.infer (hub
rows cut into CSL_INFER_SEG-edge items).  The iterate travels pre-scaled, xs = dinv (.) X, so that the gather is a plain
row sum and the row end writes the next iteration's operand; X itself is written by the last iteration only.  Softmax,
the one-hot scatter, the row norms and the final add are torch calls: each happens once.

All matrices are float32 on the device, [N, round4(C)], the padding columns zero (a clamp range that contains 0 keeps them
zero).  Single process only.  The defaults (50 iterations, alpha 0.8, autoscale) are those of the published examples,
untuned: no real dataset has been run through this code.
"""
import math

import numpy as np
import torch

from . import _abi, aggr, infer

SYMBOLS = _abi.BOUND["cslicer_smooth.h"]
_r4, _ptr, _chk = infer._r4, infer._ptr, infer._chk


def dinv_of(graph):
    """float32 [N] device tensor of an infer.InferGraph: 1 / sqrt(deg) (0 for a row without neighbours), computed on the
    host in float64 and rounded once; kept on the graph, so it goes when the graph is released"""
    d = getattr(graph, "dinv", None)
    if d is None:
        deg = np.diff(graph.host_indptr).astype(np.float64)
        d = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0).astype(np.float32)
        d = graph.dinv = torch.from_numpy(d).to(graph.device)
    return d


def _check_prop(alpha, steps, what):
    alpha, steps = float(alpha), int(steps)
    if not (0.0 < alpha <= 1.0):
        raise ValueError("%s: alpha must be in (0, 1], not %r" % (what, alpha))
    if steps < 0:
        raise ValueError("%s: the number of iterations must be >= 0, not %d" % (what, steps))
    return alpha, steps


def propagate(graph, x0, alpha, steps, lo, hi, fix=None, chunk_rows=infer.CHUNK_ROWS):
    """prop(x0, alpha, steps, lo, hi, fix) of the module docstring on an uploaded infer.InferGraph.  x0: float32 device
    [N, W], W % 4 == 0, unit column stride, a row stride that is a multiple of 4; it is read, never written.  fix:
    (rows int64 device [m], values float32 device [m, W]) set after every step.  Returns a new [N, W] matrix (steps == 0:
    a copy of x0).  Two pre-scaled buffers ping-pong; the last step writes X into the spare one, so three matrices
    are live here beside x0's owner: x0 (the base term; not read when alpha == 1) and the two buffers.  A fixed row
    costs one index_copy_ per step, into whichever matrix the step wrote."""
    alpha, steps = _check_prop(alpha, steps, "propagate")
    N, W = x0.shape
    if N != graph.N or W % 4 or x0.dtype != torch.float32 or x0.stride(1) != 1 or x0.stride(0) % 4:
        raise ValueError("propagate: x0 must be float32 [%d, W], W %% 4 == 0, with rows 16-byte aligned" % graph.N)
    if steps == 0 or N == 0:
        return x0.clone()
    dinv = dinv_of(graph)
    plan = graph.all_rows
    chunks = plan.chunks(int(chunk_rows))
    part = infer._partial(max(c.n_parts for c in chunks), W, x0.device)
    cur = x0 * dinv[:, None]
    nxt = torch.empty_like(cur)
    if fix is not None:
        rows, values = fix
        values_s = values * dinv[rows][:, None]
    beta = 1.0 - alpha
    base = x0 if alpha != 1.0 else None
    L, st, nul = _abi.load(), aggr._stream(), _ptr(None)
    for t in range(steps):
        last = t + 1 == steps
        for c in chunks:
            dst = _ptr(nxt, c.k0 * nxt.stride(0))
            _chk(L.csl_prop_f32(*infer._list_args(graph.indptr, graph.indices, plan.items, plan.hubs, c, c.k0), _ptr(cur),
                                cur.stride(0), W, _ptr(dinv), alpha, nul if base is None else _ptr(base, c.k0 * base.stride(0)),
                                0 if base is None else base.stride(0), beta, float(lo), float(hi),
                                _ptr(part) if c.n_parts else nul, dst if last else nul, nxt.stride(0),
                                nul if last else dst, nxt.stride(0), st), "csl_prop_f32")
        if fix is not None:
            nxt.index_copy_(0, rows, values if last else values_s)
        cur, nxt = nxt, cur
    return cur


def need_bytes(N, C, n_train=0, max_parts=0, logits_on_device=True):
    """the device bytes correct_and_smooth allocates at its peak (the graph and its work list not included).  Live at
    the peak, inside the correct step's propagation: P (the softmax), E0 (the base term) and the two pre-scaled buffers
    -- four [N, round4(C)] float32 matrices; a fifth while logits that came from the host sit beside P.  The smooth step
    holds three (P' made in place of P, with the training rows set, and the two buffers).  Beside them dinv and the row
    scale [N], the hub partials, and the training rows' ids, one-hot and residual rows."""
    w = _r4(C)
    return 4 * ((4 if logits_on_device else 5) * N * w + 2 * N + max_parts * w + n_train * (2 * w + 4))


def _train_rows(train_nodes, train_labels, N, C, what):
    nodes = infer._node_ids(train_nodes)
    labels = infer._node_ids(train_labels)
    if nodes.shape != labels.shape:
        raise ValueError("%s: %d training nodes, %d labels" % (what, nodes.shape[0], labels.shape[0]))
    if nodes.size and (nodes.min() < 0 or nodes.max() >= N):
        raise ValueError("%s: a training node outside [0, %d)" % (what, N))
    if np.unique(nodes).shape[0] != nodes.shape[0]:
        raise ValueError("%s: duplicate training nodes" % what)
    if labels.size and (labels.min() < 0 or labels.max() >= C):
        raise ValueError("%s: a label outside [0, %d)" % (what, C))
    return nodes, labels


def _prepared(indptr, indices, dev, N, C, n_train, chunk_rows, logits_on_device, what):
    """the uploaded InferGraph of (indptr, indices), after the memory check"""
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    g = infer.graph_of(indptr, indices, dev)
    if g.N != N:
        raise ValueError("%s: the graph has %d nodes, not %d" % (what, g.N, N))
    max_parts = max([c.n_parts for c in g.all_rows.chunks(chunk_rows)] + [0])
    infer._check_memory(need_bytes(N, C, n_train, max_parts, logits_on_device) + (0 if g.uploaded() else g.device_bytes()),
                        dev)
    return g.upload(), chunk_rows


def _onehot(labels, w, dev):
    y = torch.zeros((labels.shape[0], w), dtype=torch.float32, device=dev)
    if labels.shape[0]:
        y.scatter_(1, torch.from_numpy(labels).to(dev)[:, None], 1.0)
    return y


def _rows_of(x, nodes, N, C, dev):
    """the [n, C] rows of `nodes` (None: all) without the padding columns"""
    if nodes is None:
        return x[:, :C]
    nodes = infer._node_ids(nodes)
    if nodes.size and (nodes.min() < 0 or nodes.max() >= N):
        raise ValueError("nodes outside [0, %d)" % N)
    return x[torch.from_numpy(nodes).to(dev)][:, :C]


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def correct_and_smooth(logits, indptr, indices, train_nodes, train_labels, num_correction_layers=50, correction_alpha=0.8,
                       num_smoothing_layers=50, smoothing_alpha=0.8, autoscale=True, scale=1.0, nodes=None,
                       chunk_rows=infer.CHUNK_ROWS):
    """The smoothed class scores float32 [len(nodes) (or N), C] of Correct and Smooth over the graph (indptr, indices):
    logits [N, C] of every node (a device tensor, or anything torch.as_tensor takes), train_nodes [m] with their labels
    train_labels [m].  With P = softmax(logits) by rows and Y the one-hot rows of the labels:

        correct, autoscale (default):  E0 = 0, E0[train] = Y - P[train];  E = prop(E0, a1, T1, -1, 1);
                                       sigma = sum |E0[train]| / m;  s_v = sigma / ||E_v||_1, where that is not finite
                                       or exceeds 1000: 1;  P' = P + s (.) E
        correct, autoscale=False:      E = prop(E0, a1, T1, -inf, +inf, fix=(train, E0[train]));  P' = P + scale E
        smooth:                        G = P', G[train] = Y;  the result is prop(G, a2, T2, 0, 1)

    (T1, a1) = (num_correction_layers, correction_alpha), (T2, a2) the smoothing pair.  The predicted class is the row's
    argmax.  The graph is the one full_inference caches (infer.graph_of), so a call after it uploads nothing.
    ValueError, before any device work: duplicate training nodes, a label outside [0, C), an alpha outside (0, 1], a
    negative iteration count.  MemoryError as full_inference's, from need_bytes.  Runs on torch's current stream."""
    what = "correct_and_smooth"
    a1, T1 = _check_prop(correction_alpha, num_correction_layers, what)
    a2, T2 = _check_prop(smoothing_alpha, num_smoothing_layers, what)
    scale = float(scale)
    if not autoscale and not math.isfinite(scale):
        raise ValueError("%s: scale must be finite" % what)
    on_dev = torch.is_tensor(logits) and logits.is_cuda
    if not torch.is_tensor(logits):
        logits = torch.as_tensor(np.asarray(logits, dtype=np.float32))
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError("%s: logits must be [N, C]" % what)
    N, C = logits.shape
    train, labels = _train_rows(train_nodes, train_labels, N, C, what)
    dev = logits.device if on_dev else _device()
    with torch.no_grad():
        g, chunk_rows = _prepared(indptr, indices, dev, N, C, train.shape[0], chunk_rows, on_dev, what)
        w = _r4(C)
        p = torch.zeros((N, w), dtype=torch.float32, device=dev)
        p[:, :C] = torch.softmax(logits.to(dev, torch.float32), dim=1)
        rows = torch.from_numpy(train).to(dev)
        y = _onehot(labels, w, dev)
        e0 = torch.zeros_like(p)
        r0 = y - p[rows]
        e0.index_copy_(0, rows, r0)
        if autoscale:
            e = propagate(g, e0, a1, T1, -1.0, 1.0, chunk_rows=chunk_rows)
            sigma = r0.abs().sum() / max(train.shape[0], 1)
            s = sigma / torch.linalg.vector_norm(e, ord=1, dim=1, keepdim=True)
            s[~torch.isfinite(s) | (s > 1000.0)] = 1.0
            p.addcmul_(e, s)
        else:
            e = propagate(g, e0, a1, T1, -math.inf, math.inf, fix=(rows, r0), chunk_rows=chunk_rows)
            p.add_(e, alpha=scale)
        del e, e0
        p.index_copy_(0, rows, y)
        out = propagate(g, p, a2, T2, 0.0, 1.0, chunk_rows=chunk_rows)
        return _rows_of(out, nodes, N, C, dev).contiguous()


def label_propagation(indptr, indices, n_classes, train_nodes, train_labels, alpha=0.8, num_layers=50, nodes=None,
                      chunk_rows=infer.CHUNK_ROWS):
    """prop(Y scattered into zeros, alpha, num_layers, 0, 1): the baseline that uses no model at all.  float32
    [len(nodes) (or N), n_classes] on the current device; refusals as correct_and_smooth's."""
    what = "label_propagation"
    alpha, steps = _check_prop(alpha, num_layers, what)
    C = int(n_classes)
    if C < 1:
        raise ValueError("%s: n_classes must be positive" % what)
    N = int(np.asarray(indptr).shape[0]) - 1
    train, labels = _train_rows(train_nodes, train_labels, N, C, what)
    dev = _device()
    with torch.no_grad():
        g, chunk_rows = _prepared(indptr, indices, dev, N, C, train.shape[0], chunk_rows, True, what)
        y0 = torch.zeros((N, _r4(C)), dtype=torch.float32, device=dev)
        y0.index_copy_(0, torch.from_numpy(train).to(dev), _onehot(labels, _r4(C), dev))
        return _rows_of(propagate(g, y0, alpha, steps, 0.0, 1.0, chunk_rows=chunk_rows), nodes, N, C, dev).contiguous()


# ------------------------------------------------------------------ the command lines' three options

def add_options(ap):
    """--cs-layers, --cs-alpha and --cs-scale of cslicer.train and cslicer.predict (beside their own --correct-smooth)"""
    ap.add_argument("--cs-layers", type=str, default=None, metavar="T1,T2",
                    help="(extra) --correct-smooth: iterations of the correct and of the smooth step (default 50,50)")
    ap.add_argument("--cs-alpha", type=str, default=None, metavar="A1,A2",
                    help="(extra) --correct-smooth: alpha of the correct and of the smooth step, each in (0, 1] (default 0.8,0.8)")
    ap.add_argument("--cs-scale", type=str, default=None, metavar="auto|NUMBER",
                    help="(extra) --correct-smooth: auto (default) scales every node's correction to the training residual's "
                         "size; NUMBER adds NUMBER times the propagated residual, the training rows held fixed")


def options_of(a):
    """the correct_and_smooth keywords of a parsed command line; SystemExit for an option without --correct-smooth or a
    malformed one"""
    given = [o for o in ("cs_layers", "cs_alpha", "cs_scale") if getattr(a, o) is not None]
    if not a.correct_smooth:
        if given:
            raise SystemExit("--%s belongs to --correct-smooth" % given[0].replace("_", "-"))
        return None
    kw = {}
    try:
        if a.cs_layers is not None:
            kw["num_correction_layers"], kw["num_smoothing_layers"] = (int(x) for x in a.cs_layers.split(","))
        if a.cs_alpha is not None:
            kw["correction_alpha"], kw["smoothing_alpha"] = (float(x) for x in a.cs_alpha.split(","))
        if a.cs_scale is not None and a.cs_scale != "auto":
            kw["autoscale"], kw["scale"] = False, float(a.cs_scale)
        for k in ("correction", "smoothing"):
            _check_prop(kw.get(k + "_alpha", 0.8), kw.get("num_%s_layers" % k, 50), "--correct-smooth")
    except ValueError as ex:
        raise SystemExit("--cs-layers T1,T2 / --cs-alpha A1,A2 / --cs-scale auto|NUMBER: %s" % ex)
    return kw
