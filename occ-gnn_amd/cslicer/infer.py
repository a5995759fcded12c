"""Full-neighbour, layer-wise inference and evaluation of the trained models (include/cslicer_infer.h).

The trained model applied with EVERY neighbour instead of a sample, each layer computed for every node, layer by layer
(the standard `inference()` of DGL-style trainers; the reference evaluates this way, python/no_cache_multi_gpu.py:24-40).
It equals the sampled forward wherever sampling takes every neighbour (a row with fewer entries than the fanout,
slicer.cpp:9-13).  The neighbours of v are the entries u != v of CSR row v, with multiplicity: a self loop is dropped (as
the slicer's owned_degree does), a duplicate edge counts twice.

    GraphSAGE layer  y[v] = act([h[v] | mean_u h[u]] . W^T + b)            (zero mean without neighbours)
    GAT layer        softmax over v's neighbours only, er[v] from v's own row; a row without neighbours gets act(bias);
                     hidden layers concatenate heads + ELU, the last averages heads and drops the padded classes

The hot path is csrc/infer.hip: full-row gathers over a work list in which hub rows are cut into CSL_INFER_SEG-edge items
summed by separate waves.  The list is built here, on the host, with numpy: it is a handful of vectorised passes over
indptr, done once per graph (cached), and keeping it on the host lets a chunk of output rows find its slice of the list
without a device round trip.  Projections go through csl_gemm_f32 and csl_gat_logits_fwd_f32.  Everything runs on torch's
current stream, after whatever is already enqueued there.

Widths that are not multiples of 4 (the kernels move float4 columns) are padded: the feature table on upload, every
later table by zero weight rows / columns, so that padding columns hold exact zeros.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, aggr, splitgnn

# every symbol include/cslicer_infer.h declares (checked by tests/test_infer_cpu.py)
SYMBOLS = ["csl_infer_seg", "csl_infer_sage_f32", "csl_infer_gat_partial_ld", "csl_infer_gat_f32", "csl_infer_eval_f32"]
SEG = 512                 # CSL_INFER_SEG
CHUNK_ROWS = 1 << 16      # output rows per kernel call / GEMM (bounds the operand and partial scratch)
GAT_LAST_MAX_C = 4096     # heads x padded classes of an attention model's last layer (csl_infer_gat_f32, last != 0)
_ready = False


def _lib():
    global _ready
    L = _abi.load()
    if not _ready:
        vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
        L.csl_infer_seg.restype = i32
        L.csl_infer_sage_f32.argtypes = [vp, vp, vp, i64, vp, i64, i64, i64, vp, i64, i32, i32, vp, i32, vp, vp, i64, vp]
        L.csl_infer_gat_partial_ld.argtypes = [i32, i32]
        L.csl_infer_gat_partial_ld.restype = i64
        L.csl_infer_gat_f32.argtypes = [vp, vp, vp, i64, vp, i64, i64, i64, vp, vp, vp, i32, i32, f32, vp, i32, i32, vp, vp,
                                        i64, vp]
        L.csl_infer_eval_f32.argtypes = [vp, i64, i64, i32, vp, vp, vp, vp, vp, vp]
        if L.csl_infer_seg() != SEG:
            raise ImportError("libcslicer_hip.so: CSL_INFER_SEG differs from cslicer.infer.SEG")
        _ready = True
    return L


def _ptr(t, off=0):
    """device address of element `off` (flat, in elements) of t; NULL for None"""
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def _chk(rc, what):
    if rc < 0:
        raise _abi.CslError(rc, what + " failed")


def _r4(x):
    return (int(x) + 3) // 4 * 4


# ------------------------------------------------------------------ graph and work list (host)

def neighbour_csr(indptr, indices):
    """(indptr int64 [N + 1], indices int32 [E']) of the neighbour CSR: self loops removed, duplicates kept, row order
    kept.  int32 like the engine's device CSR."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.asarray(indices)
    n = indptr.shape[0] - 1
    if n >= 2 ** 31 - 1:
        raise ValueError("full_inference: at most 2^31 - 2 nodes (int32 CSR)")
    if indptr[0] != 0 or indptr[-1] != indices.shape[0] or (n and (np.diff(indptr) < 0).any()):
        raise ValueError("full_inference: indptr is not a CSR row pointer of the %d indices" % indices.shape[0])
    if indices.shape[0] and (indices.min() < 0 or indices.max() >= n):
        raise ValueError("full_inference: a neighbour index outside [0, %d)" % n)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    keep = indices != rows
    if keep.all():
        out = np.ascontiguousarray(indices, dtype=np.int32)
        ip = indptr.copy()
    else:
        out = np.ascontiguousarray(indices[keep], dtype=np.int32)
        ip = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[keep], minlength=n), out=ip[1:])
    if ip[-1] >= 2 ** 31:
        raise ValueError("full_inference: at most 2^31 - 1 edges (int32 CSR)")
    return ip, out


def build_plan(indptr, rows=None, seg=SEG):
    """Work list of the rows `rows` (graph row ids in output order; None: every row, in order) of the neighbour CSR
    `indptr` (int64).  Returns a dict of host arrays:
      items [n_items, 4] int32: {row, pos, e0, part}; a row of at most `seg` edges is one item (part -1), a longer one
            (hub) ceil(deg / seg) items of `seg` edges with consecutive part numbers
      hubs  [n_hubs, 4] int32: {row, pos, part_first, n_parts}
      item_first [n + 1] int64: the first item of every output position
      n_parts: partial rows of the whole list"""
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.arange(indptr.shape[0] - 1, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    n = rows.shape[0]
    deg = indptr[rows + 1] - indptr[rows]
    hub = deg > seg
    nseg = np.where(hub, (deg + seg - 1) // seg, 1)
    item_first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(nseg, out=item_first[1:])
    n_items = int(item_first[-1])
    pos = np.repeat(np.arange(n, dtype=np.int64), nseg)
    j = np.arange(n_items, dtype=np.int64) - item_first[pos]
    items = np.empty((n_items, 4), dtype=np.int32)
    items[:, 0] = rows[pos]
    items[:, 1] = pos
    items[:, 2] = indptr[rows[pos]] + j * seg
    hub_nseg = np.where(hub, nseg, 0)
    part_first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hub_nseg, out=part_first[1:])
    items[:, 3] = np.where(hub[pos], part_first[pos] + j, -1)
    hp = np.flatnonzero(hub)
    hubs = np.empty((hp.shape[0], 4), dtype=np.int32)
    hubs[:, 0], hubs[:, 1], hubs[:, 2], hubs[:, 3] = rows[hp], hp, part_first[hp], nseg[hp]
    return {"items": items, "hubs": hubs, "item_first": item_first, "part_first": part_first,
            "hub_pos": hp.astype(np.int64), "n": n, "n_parts": int(part_first[-1])}


def plan_chunks(plan, chunk_rows):
    """[(k0, k1, i0, i1, h0, h1, part0, n_parts)] per chunk of `chunk_rows` output positions"""
    out = []
    n = plan["n"]
    for k0 in range(0, n, chunk_rows):
        k1 = min(n, k0 + chunk_rows)
        h0, h1 = (int(x) for x in np.searchsorted(plan["hub_pos"], [k0, k1]))
        p0, p1 = int(plan["part_first"][k0]), int(plan["part_first"][k1])
        out.append((k0, k1, int(plan["item_first"][k0]), int(plan["item_first"][k1]), h0, h1, p0, p1 - p0))
    return out


class _DevPlan(object):
    """a work list built on the host; its device copy is made by upload()"""

    def __init__(self, plan, device):
        self.plan, self.device = plan, device
        self.items = self.hubs = None
        self._chunks = {}

    def nbytes(self):
        return self.plan["items"].nbytes + self.plan["hubs"].nbytes

    def upload(self):
        if self.items is None and self.plan["items"].shape[0]:
            self.items = torch.from_numpy(self.plan["items"]).to(self.device)
        if self.hubs is None and self.plan["hubs"].shape[0]:
            self.hubs = torch.from_numpy(self.plan["hubs"]).to(self.device)
        return self

    def chunks(self, chunk_rows):
        if chunk_rows not in self._chunks:
            self._chunks[chunk_rows] = plan_chunks(self.plan, chunk_rows)
        return self._chunks[chunk_rows]


class InferGraph(object):
    """A graph prepared for inference: the int32 neighbour CSR and the work list of all its rows, built on the host;
    upload() makes the device copies (device_bytes() of them), which stay until the graph is released."""

    def __init__(self, indptr, indices, device):
        ip, ix = neighbour_csr(indptr, indices)
        self.N = ip.shape[0] - 1
        self.n_edges = int(ix.shape[0])
        self.device = device
        self.host_indptr, self._host_indices = ip, ix
        self.indptr = self.indices = None
        self.all_rows = _DevPlan(build_plan(ip), device)

    def uploaded(self):
        return self.indptr is not None

    def device_bytes(self):
        return 4 * (self.N + 1) + 4 * max(self.n_edges, 1) + self.all_rows.nbytes()

    def upload(self):
        if self.indptr is None:
            ix = self._host_indices
            self.indptr = torch.from_numpy(self.host_indptr.astype(np.int32)).to(self.device)
            self.indices = torch.from_numpy(ix if ix.shape[0] else np.zeros(1, dtype=np.int32)).to(self.device)
            self._host_indices = None
        self.all_rows.upload()
        return self

    def plan(self, nodes=None):
        return self.all_rows if nodes is None else _DevPlan(build_plan(self.host_indptr, nodes), self.device)


_GRAPHS = []   # [(indptr, indices, device, InferGraph)]: the arrays are held, so that their ids stay theirs


def graph_of(indptr, indices, device):
    """the InferGraph of (indptr, indices) on `device`, prepared once and cached (the two most recent graphs; release()
    drops one).  Nothing is put on the device here."""
    for ip, ix, dev, g in _GRAPHS:
        if ip is indptr and ix is indices and dev == device:
            return g
    g = InferGraph(indptr, indices, device)
    _GRAPHS.insert(0, (indptr, indices, device, g))
    del _GRAPHS[2:]
    return g


def release(indptr=None, indices=None):
    """drop the cached graph of (indptr, indices) (all cached graphs when both are None), with its device memory"""
    _GRAPHS[:] = [e for e in _GRAPHS if not ((indptr is None or e[0] is indptr) and (indices is None or e[1] is indices))]


# ------------------------------------------------------------------ device steps

def _gemm_into(out, a, w, bias=None, relu=False):
    """out[m, n] (row stride out.stride(0)) = a[m, k] . w[n, k]^T (+ bias) (ReLU): csl_gemm_f32 on torch's stream"""
    m, k = a.shape
    n = w.shape[0]
    if m == 0:
        return
    L = aggr._lib()
    rc = L.csl_gemm_f32(0, 1, m, n, k, _ptr(a), a.stride(0), 0, _ptr(w), w.stride(0), 0, _ptr(out), out.stride(0), 0, 1,
                        _ptr(bias), int(relu), aggr._stream())
    if rc < 0:
        raise _abi.CslError(rc, "csl_gemm_f32: " + L.csl_gemm_last_error().decode())


def _project_rows(h, w, out, chunk_rows, bias=None):
    """out[r] = h[r] . w^T (+ bias) for every row, chunk by chunk (shapes that repeat; no GEMM over 10^7 rows)"""
    for r0 in range(0, h.shape[0], chunk_rows):
        r1 = min(h.shape[0], r0 + chunk_rows)
        _gemm_into(out[r0:r1], h[r0:r1], w, bias)


def _partial(n_rows, width, device):
    return torch.empty((max(n_rows, 1), width), dtype=torch.float32, device=device)


def sage_rows(g, dplan, x, ldx, W, proj, bias, relu, out, chunk_rows, scratch=None):
    """csl_infer_sage_f32 over every chunk of the plan; out row k of the plan is out[k] (proj) -- for the aggregate-first
    form `out` is a callable (k0, k1) -> the chunk's operand buffer, and `scratch` is called after each chunk"""
    L = _lib()
    st = aggr._stream()
    for (k0, k1, i0, i1, h0, h1, p0, npart) in dplan.chunks(chunk_rows):
        part = _partial(npart, W, x.device) if npart else None
        dst = out(k0, k1) if callable(out) else out[k0:k1]
        _chk(L.csl_infer_sage_f32(_ptr(g.indptr), _ptr(g.indices), _ptr(dplan.items, 4 * i0), i1 - i0,
                                  _ptr(dplan.hubs, 4 * h0) if h1 > h0 else C.c_void_p(0), h1 - h0, k0, p0, _ptr(x), ldx, W,
                                  int(proj), _ptr(bias), int(relu), _ptr(part), _ptr(dst), dst.stride(0), st),
             "csl_infer_sage_f32")
        if scratch is not None:
            scratch(k0, k1, dst)


def gat_rows(g, dplan, z, el, er, H, D, slope, bias, last, n_cls, out, chunk_rows):
    L = _lib()
    st = aggr._stream()
    pld = int(L.csl_infer_gat_partial_ld(H, D))
    for (k0, k1, i0, i1, h0, h1, p0, npart) in dplan.chunks(chunk_rows):
        part = _partial(npart, pld, z.device) if npart else None
        dst = out[k0:k1]
        _chk(L.csl_infer_gat_f32(_ptr(g.indptr), _ptr(g.indices), _ptr(dplan.items, 4 * i0), i1 - i0,
                                 _ptr(dplan.hubs, 4 * h0) if h1 > h0 else C.c_void_p(0), h1 - h0, k0, p0, _ptr(z), _ptr(el),
                                 _ptr(er), H, D, float(slope), _ptr(bias), int(last), int(n_cls), _ptr(part), _ptr(dst),
                                 dst.stride(0), st),
             "csl_infer_gat_f32")


def _sage_layer(g, dplan, h, conv, relu, chunk_rows):
    """One DistSageConv over the rows of `dplan`; h: [N, hp] table (hp % 4 == 0, padding columns zero).  Aggregate
    first when out >= in, project first otherwise.  Returns the [rows, round4(out)] table (padding columns zero)."""
    dev = h.device
    W, b = conv.fc.weight.detach().float(), conv.fc.bias.detach().float()
    out_w, in_w = W.shape[0], W.shape[1] // 2
    hp, op = h.shape[1], _r4(out_w)
    n_rows = dplan.plan["n"]
    if out_w >= in_w:
        # (a) [h[v] | mean h[u]] chunk by chunk, then the Linear with its bias / ReLU epilogue into the output table
        wc = torch.zeros((out_w, 2 * hp), dtype=torch.float32, device=dev)
        wc[:, :in_w], wc[:, hp:hp + in_w] = W[:, :in_w], W[:, in_w:]
        y = torch.zeros((n_rows, op), dtype=torch.float32, device=dev)
        cat = torch.empty((min(chunk_rows, max(n_rows, 1)), 2 * hp), dtype=torch.float32, device=dev)
        sage_rows(g, dplan, h, hp, hp, False, None, False, lambda k0, k1: cat[:k1 - k0], chunk_rows,
                  scratch=lambda k0, k1, c: _gemm_into(y[k0:k1, :out_w], c, wc, b, relu))
        return y
    # (b) P = h . [W_self; W_neigh]^T once for every node, then act(P[v, :out] + mean P[u, out:] + b) in one pass
    wp = torch.zeros((2 * op, hp), dtype=torch.float32, device=dev)
    wp[:out_w, :in_w], wp[op:op + out_w, :in_w] = W[:, :in_w], W[:, in_w:]
    bp = torch.zeros((op,), dtype=torch.float32, device=dev)
    bp[:out_w] = b
    P = torch.empty((g.N, 2 * op), dtype=torch.float32, device=dev)
    _project_rows(h, wp, P, chunk_rows)
    y = torch.empty((n_rows, op), dtype=torch.float32, device=dev)
    sage_rows(g, dplan, P, 2 * op, op, True, bp, relu, y, chunk_rows)
    return y


def _gat_layer(g, dplan, h, in_map, conv, last, n_cls, chunk_rows):
    """One DistGATConv over the rows of `dplan`; h: [N, hp] table whose logical column c sits at in_map[c].  Returns
    (table, its column map): hidden layers [N, H * round4(D)], the last [rows, n_cls]."""
    dev = h.device
    H, D = conv.H, conv.D
    Dp = _r4(D)
    hp = h.shape[1]
    Wt = conv.fc.weight.detach().float().view(H, D, -1)
    wz = torch.zeros((H, Dp, hp), dtype=torch.float32, device=dev)
    wz[:, :D, in_map] = Wt
    wz = wz.view(H * Dp, hp)
    al = torch.zeros((H, Dp), dtype=torch.float32, device=dev)
    ar = torch.zeros((H, Dp), dtype=torch.float32, device=dev)
    bz = torch.zeros((H, Dp), dtype=torch.float32, device=dev)
    al[:, :D], ar[:, :D], bz[:, :D] = conv.attn_l.detach(), conv.attn_r.detach(), conv.bias.detach().view(H, D)
    Cz = H * Dp
    z = torch.empty((g.N, Cz), dtype=torch.float32, device=dev)
    el = torch.empty((g.N, H), dtype=torch.float32, device=dev)
    er = torch.empty((g.N, H), dtype=torch.float32, device=dev)
    AL = aggr._lib()
    if Dp > 256:
        # csl_gat_logits_fwd_f32 holds a head in one wave (D <= 256): wider heads take el = h . (W_h^T a_l[h]) and er
        # likewise, two [N, H] GEMMs on the layer's input (the same logits, summed in another order)
        wv = wz.view(H, Dp, hp)
        vl, vr = torch.einsum("hdf,hd->hf", wv, al).contiguous(), torch.einsum("hdf,hd->hf", wv, ar).contiguous()
    for r0 in range(0, g.N, chunk_rows):
        r1 = min(g.N, r0 + chunk_rows)
        _gemm_into(z[r0:r1], h[r0:r1], wz)
        if Dp > 256:
            _gemm_into(el[r0:r1], h[r0:r1], vl)
            _gemm_into(er[r0:r1], h[r0:r1], vr)
        else:
            _chk(AL.csl_gat_logits_fwd_f32(_ptr(z[r0]), _ptr(al), _ptr(ar), r1 - r0, H, Dp, _ptr(el[r0]), _ptr(er[r0]),
                                           aggr._stream()), "csl_gat_logits_fwd_f32")
    n_rows = dplan.plan["n"]
    if last:
        out = torch.empty((n_rows, n_cls), dtype=torch.float32, device=dev)
        gat_rows(g, dplan, z, el, er, H, Dp, conv.slope, bz, True, n_cls, out, chunk_rows)
        return out, None
    out = torch.empty((n_rows, Cz), dtype=torch.float32, device=dev)
    gat_rows(g, dplan, z, el, er, H, Dp, conv.slope, bz, False, 0, out, chunk_rows)
    cmap = (torch.arange(H, device=dev)[:, None] * Dp + torch.arange(D, device=dev)[None, :]).reshape(-1)
    return out, cmap


# ------------------------------------------------------------------ public interface

def _need_bytes(model, N, n_out, F, chunk_rows, max_parts):
    """the device bytes full_inference allocates at its peak (float32 tables; the graph and plan not included)"""
    f = 4
    need, width = 0, _r4(F)
    if isinstance(model, splitgnn.DistSAGEModel):
        for k, conv in enumerate(model.convs):
            out_w, in_w = conv.fc.weight.shape[0], conv.fc.weight.shape[1] // 2
            rows = n_out if k + 1 == len(model.convs) else N
            op = _r4(out_w)
            t = N * width + rows * op
            if out_w >= in_w:
                t += min(chunk_rows, rows) * 2 * width + max_parts * width
            else:
                t += N * 2 * op + max_parts * op
            need, width = max(need, t), op
    else:
        for k, conv in enumerate(model.convs):
            last = k + 1 == len(model.convs)
            C_ = conv.H * _r4(conv.D)
            t = N * width + N * C_ + 2 * N * conv.H + (n_out * model.n_classes if last else N * C_)
            t += max_parts * (C_ + 2 * conv.H + 4)
            need, width = max(need, t), C_
    return need * f


def _check_memory(need, device):
    free, _ = torch.cuda.mem_get_info(device)
    free += torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)   # torch's cached blocks
    if need > free:
        raise MemoryError("full_inference needs %d bytes of device memory, %d are free" % (need, free))


def full_inference(model, indptr, indices, features, nodes=None, chunk_rows=CHUNK_ROWS):
    """float32 logits [len(nodes) (or N), n_classes] on the device of `features` of a DistSAGEModel or DistGATModel
    applied with every neighbour (module docstring).  Hidden layers are computed for all N nodes, the last one only for
    `nodes` (int array of node ids; None: all).  features: float32 [N, F] (a device tensor is used in place when F % 4 == 0;
    anything else is uploaded / padded).  Runs under torch.no_grad() and changes no parameter.  Every width is supported
    except an attention model whose last layer has more than GAT_LAST_MAX_C = 4096 heads x padded-class columns
    (ValueError).  Before allocating, the device bytes it needs (tables, scratch and, on first use of a graph, the
    graph's CSR and work list) are checked against the free memory: MemoryError with both counts."""
    if not isinstance(model, (splitgnn.DistSAGEModel, splitgnn.DistGATModel)):
        raise TypeError("full_inference takes a DistSAGEModel or a DistGATModel")
    if isinstance(model, splitgnn.DistGATModel) and model.convs[-1].H * _r4(model.convs[-1].D) > GAT_LAST_MAX_C:
        raise ValueError("full_inference: the attention model's last layer has heads x classes (padded to 4) = %d > %d "
                         "columns; its head mean stages a row in LDS" % (model.convs[-1].H * _r4(model.convs[-1].D),
                                                                       GAT_LAST_MAX_C))
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    dev = features.device if torch.is_tensor(features) and features.is_cuda else torch.device(
        "cuda", torch.cuda.current_device())
    with torch.no_grad():
        g = graph_of(indptr, indices, dev)
        N = g.N
        F = features.shape[1]
        if features.shape[0] != N:
            raise ValueError("features must have one row per node (%d), got %d" % (N, features.shape[0]))
        if nodes is not None:
            nodes = np.asarray(nodes.cpu() if torch.is_tensor(nodes) else nodes).astype(np.int64).reshape(-1)
            if nodes.size and (nodes.min() < 0 or nodes.max() >= N):
                raise ValueError("nodes outside [0, %d)" % N)
        dlast = g.plan(nodes)
        n_out = dlast.plan["n"]
        max_parts = max([c[7] for c in g.all_rows.chunks(chunk_rows)] + [c[7] for c in dlast.chunks(chunk_rows)] + [0])
        need = _need_bytes(model, N, n_out, F, chunk_rows, max_parts)
        need += (0 if g.uploaded() else g.device_bytes()) + (dlast.nbytes() if nodes is not None else 0)
        upload = not (torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32
                      and F % 4 == 0 and features.stride(1) == 1 and features.stride(0) == F)
        _check_memory(need + (N * _r4(F) * 4 if upload else 0), dev)
        g.upload()
        dlast.upload()
        if upload:
            h = torch.zeros((N, _r4(F)), dtype=torch.float32, device=dev)
            h[:, :F] = torch.as_tensor(features).to(dev, torch.float32)
        else:
            h = features
        in_map = torch.arange(F, device=dev)
        L = len(model.convs)
        for k, conv in enumerate(model.convs):
            last = k + 1 == L
            dplan = dlast if last else g.all_rows
            if isinstance(model, splitgnn.DistSAGEModel):
                h = _sage_layer(g, dplan, h, conv, not last, chunk_rows)
            else:
                h, in_map = _gat_layer(g, dplan, h, in_map, conv, last, model.n_classes, chunk_rows)
        if isinstance(model, splitgnn.DistSAGEModel):
            n_cls = model.convs[-1].fc.weight.shape[0]
            if h.shape[1] != n_cls:
                h = h[:, :n_cls].contiguous()
        return h


def eval_head(logits, labels):
    """(pred int64 [n], correct count, summed cross-entropy) of logits [n, C] against labels [n] (int64, device), in one
    pass over the logits (csl_infer_eval_f32; ties of the argmax go to the lowest class, as torch.argmax)."""
    logits = logits if logits.stride(1) == 1 else logits.contiguous()
    labels = labels.to(logits.device, torch.int64).contiguous()
    n, C_ = logits.shape
    pred = torch.empty((max(n, 1),), dtype=torch.int64, device=logits.device)
    loss_row = torch.empty((max(n, 1),), dtype=torch.float32, device=logits.device)
    loss_sum = torch.empty((1,), dtype=torch.float64, device=logits.device)
    correct = torch.empty((1,), dtype=torch.int64, device=logits.device)
    _chk(_lib().csl_infer_eval_f32(_ptr(logits), logits.stride(0), n, C_, _ptr(labels), _ptr(pred), _ptr(loss_row),
                                   _ptr(loss_sum), _ptr(correct), aggr._stream()), "csl_infer_eval_f32")
    return pred[:n], int(correct.item()), float(loss_sum.item())


def evaluate(model, indptr, indices, features, nodes, labels, chunk_rows=CHUNK_ROWS):
    """{"accuracy", "loss", "n"} of the model on `nodes` by full-neighbour inference: argmax accuracy and mean
    cross-entropy.  labels: int [N], the label of every node of the graph (those of `nodes` are used)."""
    nodes = np.asarray(nodes.cpu() if torch.is_tensor(nodes) else nodes).astype(np.int64).reshape(-1)
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.shape[0] != features.shape[0]:
        raise ValueError("labels must hold one label per node of the graph ([%d])" % features.shape[0])
    logits = full_inference(model, indptr, indices, features, nodes=nodes, chunk_rows=chunk_rows)
    lab = lab[torch.from_numpy(nodes).to(lab.device)]
    _, correct, loss = eval_head(logits, lab.to(logits.device))
    n = int(nodes.shape[0])
    return {"accuracy": correct / max(n, 1), "loss": loss / max(n, 1), "n": n}
