"""L0 on-disk dataset format of the reference (reader/writer) + synthetic graphs.

Format (reference writer python/utils/convert_dgl_dataset.py:99-127, reference
reader cslicer/dataset.cpp:18-113):

    <dir>/meta.txt            key=value lines: num_nodes, num_edges, feature_dim,
                              csum_features, csum_labels, csum_offsets,
                              csum_edges, num_classes; optionally
                              feature_dtype=float32|float16|bfloat16 (no key:
                              float32, what the reference writes and reads)
    <dir>/indptr.bin          int64[N+1]
    <dir>/indices.bin         int64[E]
    <dir>/features.bin        float32[N*feature_dim]   (unused by the slicer);
                              float16 / bfloat16 (raw 16-bit words) when
                              meta.txt says so
    <dir>/labels.bin          int32[N]                 (unused by the slicer);
                              multi-label (meta.txt: multilabel=1): the
                              packed words int32[N, ceil(num_classes / 32)],
                              class c = bit c % 32 of word c / 32
    <dir>/partition_map_opt.bin int32[N]               (loaded, ignored: the
                              reference uses v % 4, cslicer/pyfrontend.cpp:57)
    <dir>/train_idx.bin       int64[...]  optional training / evaluation node
    <dir>/val_idx.bin         int64[...]  split, with csum_train / csum_test
                              in meta.txt (convert_dgl_dataset.py:107-112)
    <dir>/edge_weight.bin     float32[E]  optional (not the reference's): edge
                              weights in CSR order, for weighted sampling
                              (write_edge_weight / read_edge_weight)

The reference reader skips a final line that has no trailing newline
(dataset.cpp:75), so the writer always terminates every line with '\n'.

OGB datasets are not available offline; `synth_graph` generates graphs of the
same shape: pareto(alpha=1.5) degrees scaled to the requested
mean, uniform random neighbours, rows sorted, no self loops.
"""
import os

import numpy as np

PRESETS = {
    # name: (num_nodes, mean_degree, feature_dim, num_classes)
    "arxiv-like": (169_343, 6.9, 128, 40),
    "products-like": (2_449_029, 50.5, 100, 47),
    "papers-like": (111_059_956, 14.5, 128, 172),
}


def synth_degrees(num_nodes, mean_deg, rng, alpha=1.5, d0=1, cap=None):
    """deg = min(floor(pareto(alpha) * s + d0), cap), s tuned so mean(deg) ~= mean_deg."""
    if cap is None:
        cap = int(min(num_nodes - 1, 20_000))
    x = rng.pareto(alpha, num_nodes)
    lo, hi = 0.0, float(max(mean_deg, 1.0)) * 64.0

    def degs(s):
        return np.minimum(np.floor(x * s + d0), cap).astype(np.int64)

    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if degs(mid).mean() < mean_deg:
            lo = mid
        else:
            hi = mid
    return degs(0.5 * (lo + hi))


def synth_graph(num_nodes, mean_deg, seed=0, alpha=1.5, degrees=None, sort_rows=True):
    """Return (indptr int64[N+1], indices int64[E]) of a synthetic CSR graph."""
    rng = np.random.default_rng(seed)
    if degrees is None:
        deg = synth_degrees(num_nodes, mean_deg, rng, alpha=alpha)
    else:
        deg = np.asarray(degrees, dtype=np.int64)
        assert deg.shape == (num_nodes,)
    indptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    num_edges = int(indptr[-1])
    rows = np.repeat(np.arange(num_nodes, dtype=np.int64), deg)
    cols = rng.integers(0, num_nodes, size=num_edges, dtype=np.int64)
    # no self loops (convert_dgl_dataset.py:45 removes them)
    if num_nodes > 1:
        hit = cols == rows
        cols[hit] = (cols[hit] + 1) % num_nodes
    if sort_rows and num_edges:
        # rows sorted (convert_dgl_dataset.py:47); rows are already grouped, so
        # sorting row*N+col keeps the grouping and orders within a row.
        key = rows * np.int64(num_nodes) + cols
        key.sort()
        cols = key - rows * np.int64(num_nodes)
    return indptr, cols


def synth_graph_big(num_nodes, mean_deg, seed=0, alpha=1.5, chunk=4_000_000):
    """synth_graph for graphs with 10^9 edges (papers-like): same degree law and uniform neighbours, rows NOT
    sorted, built node-chunk by node-chunk so that only the result itself (indptr + indices) is ever held;
    the degree scale is tuned on the first two million draws instead of all of them."""
    rng = np.random.default_rng(seed)
    cap = int(min(num_nodes - 1, 20_000))
    x = rng.pareto(alpha, num_nodes)
    sub = x[:2_000_000]
    lo, hi = 0.0, float(max(mean_deg, 1.0)) * 64.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if np.minimum(np.floor(sub * mid + 1), cap).mean() < mean_deg:
            lo = mid
        else:
            hi = mid
    deg = np.minimum(np.floor(x * (0.5 * (lo + hi)) + 1), cap).astype(np.int64)
    del x
    indptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    cols = np.empty(int(indptr[-1]), dtype=np.int64)
    for a in range(0, num_nodes, chunk):
        b = min(num_nodes, a + chunk)
        e0, e1 = int(indptr[a]), int(indptr[b])
        c = rng.integers(0, num_nodes, size=e1 - e0, dtype=np.int64)
        rows = np.repeat(np.arange(a, b, dtype=np.int64), deg[a:b])
        hit = c == rows                                    # no self loops (convert_dgl_dataset.py:45)
        c[hit] = (c[hit] + 1) % num_nodes
        cols[e0:e1] = c
    return indptr, cols


def synth_preset(name, seed=0):
    n, d, _, _ = PRESETS[name]
    return synth_graph(n, d, seed=seed)


FEATURE_DTYPES = ("float32", "float16", "bfloat16")


def to_bfloat16_words(x):
    """float32 array -> its bfloat16 values as raw uint16 words, round to nearest even (what
    torch.as_tensor(x).to(torch.bfloat16) stores); a NaN stays a (quiet) NaN."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    if nan.any():
        r[nan] = ((b[nan] >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16)
    return r


def bfloat16_words_to_float32(w):
    """raw bfloat16 words (uint16) -> float32, exact"""
    return (np.asarray(w).astype(np.uint32) << np.uint32(16)).view(np.float32)


def feature_file_dtype(feature_dtype):
    """numpy dtype of features.bin's elements: bfloat16 has none, its words are read as uint16"""
    if feature_dtype not in FEATURE_DTYPES:
        raise ValueError("feature_dtype must be one of %s, not %r" % (", ".join(FEATURE_DTYPES), feature_dtype))
    return {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[feature_dtype]


def read_features(path, meta=None, mmap=True):
    """(rows, feature_dtype) of an L0 directory: features.bin as [N, feature_dim] in its stored element type -- float32,
    float16, or for bfloat16 the raw uint16 words (bfloat16_words_to_float32, or a torch view as torch.bfloat16)."""
    meta = read_meta(path) if meta is None else meta
    dt = feature_file_dtype(meta["feature_dtype"])
    shape = (meta["num_nodes"], meta["feature_dim"])
    f = os.path.join(path, "features.bin")
    if mmap:
        return np.memmap(f, dtype=dt, mode="r", shape=shape), meta["feature_dtype"]
    return np.fromfile(f, dtype=dt, count=shape[0] * shape[1]).reshape(shape), meta["feature_dtype"]


def feature_rows(rows, feature_dtype):
    """Rows of features.bin in their stored element type (read_features' map, a selection or a copy of it) as what
    Trainer(features=...) takes: a numpy array, or for bfloat16 -- numpy has none -- the same words as a torch.bfloat16
    tensor.  No copy is made beyond np.asarray's."""
    rows = np.asarray(rows)
    if feature_dtype != "bfloat16":
        return rows
    import torch
    return torch.from_numpy(rows.view(np.int16)).view(torch.bfloat16)


def label_words(num_classes):
    """W = ceil(C / 32): the 32-bit words of a node's packed multi-label row"""
    return (int(num_classes) + 31) // 32


def pack_labels(y):
    """[n, C] of 0 / 1 (bool or integer) -> int32 [n, ceil(C / 32)]: class c is bit c % 32 of word c / 32, the bits at and
    above C of the last word zero (include/cslicer_multilabel.h).  Any other value is a ValueError."""
    y = np.asarray(y)
    if y.ndim != 2 or y.shape[1] < 1:
        raise ValueError("pack_labels: a matrix [n, C] with C >= 1 expected, not shape %r" % (y.shape,))
    if y.dtype != np.bool_:
        if y.dtype.kind not in "iu":
            raise ValueError("pack_labels: bool or integer labels expected, not %s" % y.dtype)
        if y.size and not np.isin(y, (0, 1)).all():
            raise ValueError("pack_labels: every label must be 0 or 1")
    n, C = y.shape
    W = label_words(C)
    bits = np.zeros((n, W * 32), dtype=np.uint8)
    bits[:, :C] = y != 0
    # (bitorder little: column c lands in bit c % 8 of byte c / 8, i.e. bit c % 32 of the little-endian word c / 32)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4").astype(np.uint32).view(np.int32)


def unpack_labels(words, num_classes):
    """int32 (or uint32) [n, ceil(C / 32)] -> bool [n, C]; bits at and above C are not looked at"""
    w = np.ascontiguousarray(words)
    C = int(num_classes)
    if w.ndim != 2 or w.dtype.kind not in "iu" or w.dtype.itemsize != 4 or C < 1 or w.shape[1] != label_words(C):
        raise ValueError("unpack_labels: 32-bit words [n, %d] expected for %d classes" % (label_words(max(C, 1)), C))
    by = w.view(np.uint32).astype("<u4").view(np.uint8).reshape(w.shape[0], -1)
    return np.unpackbits(by, axis=1, bitorder="little")[:, :C].astype(np.bool_)


def write_l0(path, indptr, indices, features=None, labels=None, partition=None,
             feature_dim=None, num_classes=2, train_idx=None, val_idx=None, feature_dtype=None):
    """Write an L0 dataset directory readable by the reference's Dataset class.  train_idx / val_idx (both or
    neither): the node split, written as train_idx.bin / val_idx.bin (int64) with their sums csum_train / csum_test
    in meta.txt, as the reference's converter does (convert_dgl_dataset.py:107-112).

    feature_dtype ("float32", "float16" or "bfloat16"; None: float32 and no key, the reference's own format):
    features.bin is written in that element type -- float32 input rounded to nearest even, bfloat16 as its raw 16-bit
    words -- and meta.txt records feature_dtype=.  csum_features is the sum of the STORED values, as for float32."""
    if (train_idx is None) != (val_idx is None):
        raise ValueError("write_l0: pass both train_idx and val_idx, or neither")
    if feature_dtype is not None:
        feature_file_dtype(feature_dtype)      # (raises for an unknown name)
    os.makedirs(path, exist_ok=True)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    n = indptr.shape[0] - 1
    if features is None:
        feature_dim = 1 if feature_dim is None else feature_dim
        features = np.zeros((n, feature_dim), dtype=np.float32)
    features = np.ascontiguousarray(features, dtype=np.float32).reshape(n, -1)
    if labels is None:
        labels = np.zeros(n, dtype=np.int32)
    multilabel = np.ndim(labels) == 2
    if multilabel:
        if np.shape(labels) != (n, int(num_classes)):
            raise ValueError("write_l0: multi-label labels must be [%d, num_classes = %d], not %r"
                             % (n, int(num_classes), np.shape(labels)))
        labels = pack_labels(labels).astype("<i4")
        lsum = int(labels.view(np.uint32).sum(dtype=np.int64))
    else:
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        lsum = int(labels.sum(dtype=np.int64))
    if partition is None:
        partition = (np.arange(n) % 4).astype(np.int32)
    partition = np.ascontiguousarray(partition, dtype=np.int32)
    indptr.tofile(os.path.join(path, "indptr.bin"))
    indices.tofile(os.path.join(path, "indices.bin"))
    if feature_dtype == "float16":
        with np.errstate(over="ignore"):
            stored = features.astype(np.float16)              # (numpy rounds to nearest even, as torch does)
        if np.isinf(stored).any() and not np.isinf(features).any():
            raise ValueError("write_l0: features beyond float16's range (65504) would be stored as Inf; use bfloat16")
        fsum = stored.astype(np.float32).sum(dtype=np.float64)
    elif feature_dtype == "bfloat16":
        stored = to_bfloat16_words(features)
        fsum = bfloat16_words_to_float32(stored).sum(dtype=np.float64)
    else:
        stored, fsum = features, features.sum(dtype=np.float64)
    stored.tofile(os.path.join(path, "features.bin"))
    labels.tofile(os.path.join(path, "labels.bin"))
    partition.tofile(os.path.join(path, "partition_map_opt.bin"))
    meta = {
        "num_nodes": n,
        "num_edges": int(indices.shape[0]),
        "feature_dim": int(features.shape[1]),
        "csum_features": int(fsum),
        "csum_labels": lsum,
    }
    if train_idx is not None:
        train_idx = np.ascontiguousarray(train_idx, dtype=np.int64)
        val_idx = np.ascontiguousarray(val_idx, dtype=np.int64)
        for name, idx in (("train_idx", train_idx), ("val_idx", val_idx)):
            if idx.ndim != 1 or (idx.size and (idx.min() < 0 or idx.max() >= n)):
                raise ValueError("write_l0: %s must be node ids in [0, %d)" % (name, n))
        train_idx.tofile(os.path.join(path, "train_idx.bin"))
        val_idx.tofile(os.path.join(path, "val_idx.bin"))
        meta["csum_train"] = int(train_idx.sum(dtype=np.int64))
        meta["csum_test"] = int(val_idx.sum(dtype=np.int64))
    meta.update({
        "csum_offsets": int(indptr.sum(dtype=np.int64)),
        "csum_edges": int(indices.sum(dtype=np.int64)),
        "num_classes": int(num_classes),
    })
    with open(os.path.join(path, "meta.txt"), "w") as f:
        for k, v in meta.items():
            f.write("%s=%d\n" % (k, v))
        if feature_dtype is not None:
            f.write("feature_dtype=%s\n" % feature_dtype)
        if multilabel:
            f.write("multilabel=1\n")
    meta["feature_dtype"] = feature_dtype or "float32"
    if multilabel:
        meta["multilabel"] = 1
    return meta


def read_meta(path):
    meta = {}
    with open(os.path.join(path, "meta.txt")) as f:
        for line in f:
            if not line.endswith("\n"):
                break  # dataset.cpp:75: an unterminated last line is dropped
            line = line.strip()
            if not line:
                continue
            k, _, v = line.partition("=")
            meta[k] = v if k == "feature_dtype" else int(v)
    meta.setdefault("feature_dtype", "float32")     # (a directory without the key: the reference's float32)
    feature_file_dtype(meta["feature_dtype"])
    return meta


def read_labels(path, meta=None, mmap=True):
    """labels.bin of an L0 directory: int32 [N], or for a multi-label directory (meta.txt: multilabel=1) the packed words
    int32 [N, ceil(num_classes / 32)] (unpack_labels)."""
    meta = read_meta(path) if meta is None else meta
    n = meta["num_nodes"]
    shape = (n, label_words(meta["num_classes"])) if meta.get("multilabel") else (n,)
    f = os.path.join(path, "labels.bin")
    if mmap:
        return np.memmap(f, dtype="<i4", mode="r", shape=shape)
    return np.fromfile(f, dtype="<i4", count=int(np.prod(shape))).reshape(shape)


def labels_checksum(labels, multilabel):
    """csum_labels of meta.txt: the int64 sum of the labels, of a multi-label file's words read as unsigned"""
    a = np.asarray(labels)
    return int((a.view(np.uint32) if multilabel else a).sum(dtype=np.int64))


def read_l0(path, mmap=True, check=True):
    """Read the graph part of an L0 directory. Returns (indptr, indices, meta).  check: the checksums of indptr.bin,
    indices.bin and (where the file and its csum_labels are there) labels.bin, in either label format."""
    meta = read_meta(path)
    n, e = meta["num_nodes"], meta["num_edges"]
    if mmap:
        indptr = np.memmap(os.path.join(path, "indptr.bin"), dtype=np.int64, mode="r", shape=(n + 1,))
        indices = np.memmap(os.path.join(path, "indices.bin"), dtype=np.int64, mode="r", shape=(e,))
    else:
        indptr = np.fromfile(os.path.join(path, "indptr.bin"), dtype=np.int64, count=n + 1)
        indices = np.fromfile(os.path.join(path, "indices.bin"), dtype=np.int64, count=e)
    if check:
        # dataset.cpp:27,35 checksum asserts (compiled out in the reference's
        # setup.py build; enforced here, loudly)
        if int(np.sum(indptr, dtype=np.int64)) != meta["csum_offsets"]:
            raise ValueError("indptr checksum mismatch in %s" % path)
        if int(np.sum(indices, dtype=np.int64)) != meta["csum_edges"]:
            raise ValueError("indices checksum mismatch in %s" % path)
        lf = os.path.join(path, "labels.bin")
        if "csum_labels" in meta and os.path.exists(lf):
            multi = bool(meta.get("multilabel"))
            want = (n * label_words(meta["num_classes"]) if multi else n) * 4
            if os.path.getsize(lf) != want:
                raise ValueError("labels.bin of %s holds %d bytes, %d expected" % (path, os.path.getsize(lf), want))
            if labels_checksum(read_labels(path, meta), multi) != meta["csum_labels"]:
                raise ValueError("labels checksum mismatch in %s" % path)
    return indptr, indices, meta


def read_splits(path):
    """(train_idx, val_idx) int64 of an L0 directory, or None when it has no split files.  The sums are checked
    against meta.txt's csum_train / csum_test where it has them (a mismatch raises ValueError)."""
    tp, vp = os.path.join(path, "train_idx.bin"), os.path.join(path, "val_idx.bin")
    have = os.path.exists(tp), os.path.exists(vp)
    if not any(have):
        return None
    if not all(have):
        raise ValueError("%s has only one of train_idx.bin / val_idx.bin" % path)
    meta = read_meta(path)
    out = []
    for f, key in ((tp, "csum_train"), (vp, "csum_test")):
        if os.path.getsize(f) % 8:
            raise ValueError("%s is not an int64 array" % f)
        idx = np.fromfile(f, dtype=np.int64)
        if key in meta and int(idx.sum(dtype=np.int64)) != meta[key]:
            raise ValueError("%s checksum mismatch in %s" % (os.path.basename(f), path))
        if "num_nodes" in meta and idx.size and (idx.min() < 0 or idx.max() >= meta["num_nodes"]):
            raise ValueError("%s holds node ids outside [0, num_nodes)" % f)
        out.append(idx)
    return out[0], out[1]


def check_edge_weights(weights, num_edges):
    """float64 [num_edges] of a host edge-weight array; ValueError for another length, a negative or a non-finite weight"""
    w = np.asarray(weights)
    if w.ndim != 1 or w.shape[0] != int(num_edges):
        raise ValueError("edge weights have shape %r, the graph has %d edges" % (w.shape, int(num_edges)))
    if w.dtype.kind not in "fiub":
        raise ValueError("edge weights must be numbers, not %s" % w.dtype)
    w = w.astype(np.float64)
    if w.size and not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("edge weights must be finite and >= 0")
    return w


def edge_cdf(indptr, weights):
    """uint32 [E]: the table of csl_set_edge_cdf (include/cslicer_hip.h) for float edge weights in CSR order.  The only
    float-to-integer step of weighted sampling: with S_v the float64 sum of row v, q_i = floor(w_i / S_v * 2^31), raised to
    1 where w_i > 0 (so q_i == 0 iff w_i == 0), and the table holds every row's running sum of q (T_v <= 2^31 + deg).  A
    row whose weights are all zero gets zeros: the engine draws it uniformly.  Weights must be finite and >= 0 and a row
    may have at most 2^31 - 1 edges, else ValueError."""
    indptr = np.asarray(indptr, dtype=np.int64)
    w = check_edge_weights(weights, indptr[-1])
    deg = np.diff(indptr)
    if deg.size and int(deg.max()) > 2 ** 31 - 1:
        raise ValueError("edge_cdf: a row of %d edges (at most 2^31 - 1)" % int(deg.max()))
    if w.size == 0:
        return np.zeros(0, dtype=np.uint32)
    rows = np.repeat(np.arange(deg.shape[0], dtype=np.int64), deg)
    start = indptr[:-1][deg > 0]
    S = np.zeros(deg.shape[0], dtype=np.float64)
    S[deg > 0] = np.add.reduceat(w, start)
    Se = S[rows]
    q = np.zeros(w.shape[0], dtype=np.int64)
    pos = Se > 0
    q[pos] = np.floor(w[pos] / Se[pos] * 2.0 ** 31).astype(np.int64)
    q[pos & (w > 0) & (q == 0)] = 1
    q[w == 0] = 0
    c = np.cumsum(q)
    before = np.zeros(deg.shape[0], dtype=np.int64)       # sum of q over the rows before this one
    before[deg > 0] = c[start] - q[start]
    cum = c - before[rows]
    assert int(cum.max()) <= 2 ** 32 - 1
    return cum.astype(np.uint32)


def inv_degree_weights(indptr, indices):
    """float32 [E]: w(v <- u) = 1 / max(deg(u), 1) for every edge of row v with source u, deg the CSR's row lengths --
    an importance scheme that keeps hubs from flooding the deeper frontiers"""
    deg = np.diff(np.asarray(indptr, dtype=np.int64))
    return (1.0 / np.maximum(deg[np.asarray(indices, dtype=np.int64)], 1)).astype(np.float32)


def write_edge_weight(path, weights):
    """edge_weight.bin of an L0 directory: float32 [num_edges] in CSR order, beside the other files (meta.txt unchanged)"""
    w = check_edge_weights(weights, read_meta(path)["num_edges"])
    w.astype("<f4").tofile(os.path.join(path, "edge_weight.bin"))


def read_edge_weight(path):
    """float32 [num_edges] of an L0 directory's edge_weight.bin; ValueError if the file's length is not the graph's"""
    f = os.path.join(path, "edge_weight.bin")
    if not os.path.exists(f):
        raise ValueError("%s has no edge_weight.bin" % path)
    e = read_meta(path)["num_edges"]
    if os.path.getsize(f) != 4 * e:
        raise ValueError("%s holds %d bytes, %d expected (float32 per edge)" % (f, os.path.getsize(f), 4 * e))
    return np.fromfile(f, dtype="<f4", count=e)


def from_edge_list(num_nodes, src, dst, symmetric=False, rows="in"):
    """Edge list -> L0 CSR the way the reference converter prepares it
    (python/utils/convert_dgl_dataset.py:42-49): self loops removed (:45), rows sorted (:47),
    duplicate edges kept.  rows="in": row v lists the sources of edges u -> v (what a GNN samples
    from); rows="out": row u lists the destinations.  The reference takes DGL's `adj()`, whose
    orientation changed between DGL versions; for the symmetric OGB graphs it converts both are the
    same matrix.  symmetric=True adds the reverse of every edge first."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    if src.shape != dst.shape:
        raise ValueError("src and dst differ in length")
    if src.size and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= num_nodes):
        raise ValueError("edge endpoint outside [0, num_nodes)")
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    keep = src != dst                                   # convert_dgl_dataset.py:45
    src, dst = src[keep], dst[keep]
    if rows == "out":
        src, dst = dst, src
    elif rows != "in":
        raise ValueError("rows must be 'in' or 'out'")
    key = dst * np.int64(num_nodes) + src               # group by destination, sort sources in a row
    key.sort()
    rows, cols = key // np.int64(num_nodes), key % np.int64(num_nodes)
    indptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=num_nodes), out=indptr[1:])
    return indptr, cols


def _main(argv):
    """python -m cslicer.l0 convert <edges.npz|edges.npy> <out_dir> [--symmetric] [--num-nodes N]
                                 [--feature-dtype float32|float16|bfloat16]
    edges.npz: arrays `src`, `dst` (optionally `features`, `labels`, `partition`, `num_nodes`);
    edges.npy: int array of shape [2, E] or [E, 2]."""
    import argparse
    ap = argparse.ArgumentParser(prog="cslicer.l0")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("convert")
    c.add_argument("edges")
    c.add_argument("out_dir")
    c.add_argument("--symmetric", action="store_true")
    c.add_argument("--num-nodes", type=int, default=None)
    c.add_argument("--feature-dtype", choices=FEATURE_DTYPES, default=None,
                   help="element type of features.bin (recorded in meta.txt; default: float32, no key)")
    a = ap.parse_args(argv)
    feats = labels = part = None
    if a.edges.endswith(".npz"):
        z = np.load(a.edges)                              # allow_pickle stays False
        src, dst = z["src"], z["dst"]
        feats = z["features"] if "features" in z.files else None
        labels = z["labels"] if "labels" in z.files else None
        part = z["partition"] if "partition" in z.files else None
        n = a.num_nodes or (int(z["num_nodes"]) if "num_nodes" in z.files else None)
    else:
        e = np.load(a.edges)
        e = e if e.shape[0] == 2 else e.T
        src, dst, n = e[0], e[1], a.num_nodes
    if n is None:
        n = int(max(src.max(), dst.max())) + 1
    indptr, indices = from_edge_list(n, src, dst, symmetric=a.symmetric)
    classes = int(labels.max()) + 1 if labels is not None else 2
    meta = write_l0(a.out_dir, indptr, indices, features=feats, labels=labels, partition=part, num_classes=classes,
                    feature_dtype=a.feature_dtype)
    print("wrote %s: %s" % (a.out_dir, meta))


if __name__ == "__main__":
    import sys
    _main(sys.argv[1:])
