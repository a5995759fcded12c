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

A float16 / bfloat16 feature table (include/cslicer_infer16.h) is read IN PLACE by the first layer, the only one that
reads it: the GraphSAGE aggregate-first kernels load its rows and upcast them in registers (the _x16 twins), and where
the library GEMM reads the table (GraphSAGE project-first, the attention model's projections) each chunk of rows is
upcast into one reusable float32 buffer first.  Both upcasts are exact and everything behind them is the float32 code, so
the logits are bitwise those of the same call on the table upcast to float32 -- without ever holding that copy.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _abi, aggr, splitgnn

# every entry point include/cslicer_infer.h and include/cslicer_infer_parts.h declare (bound from the headers' text when
# the library is loaded: _abi.bind_header)
_abi.load()
SYMBOLS, PARTS_SYMBOLS = _abi.BOUND["cslicer_infer.h"], _abi.BOUND["cslicer_infer_parts.h"]
FEAT16_SYMBOLS = _abi.BOUND["cslicer_infer16.h"]    # the readers of a 16-bit feature table
SEG = 512                 # CSL_INFER_SEG
CHUNK_ROWS = 1 << 16      # output rows per kernel call / GEMM (bounds the operand and partial scratch)
GAT_LAST_MAX_C = 4096     # heads x padded classes of an attention model's last layer (csl_infer_gat_f32, last != 0)
_lib = _abi.load      # (every prototype is bound there; the tests and profiles/ reach the library by this name)
if _lib().csl_infer_seg() != SEG:
    raise ImportError("libcslicer_hip.so: CSL_INFER_SEG differs from cslicer.infer.SEG")


def _ptr(t, off=0):
    """device address of element `off` (flat, in elements) of t; NULL for None"""
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def _chk(rc, what):
    if rc < 0:
        raise _abi.CslError(rc, what + " failed")


def _r4(x):
    return (int(x) + 3) // 4 * 4


def _kind(t):
    """None for a float32 table, the element kind (CSL_FEAT_F16 / CSL_FEAT_BF16) of a 16-bit one"""
    return None if t.dtype == torch.float32 else aggr.FEAT_KINDS[t.dtype]


def _node_ids(nodes):
    """a list of node ids (array, list or tensor) as a contiguous int64 [n] host array"""
    return np.ascontiguousarray(np.asarray(nodes.cpu() if torch.is_tensor(nodes) else nodes).astype(np.int64).reshape(-1))


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


# a chunk of output positions [k0, k1): its items [i0, i1), hubs [h0, h1) and partial rows part0 .. part0 + n_parts
Chunk = collections.namedtuple("Chunk", "k0 k1 i0 i1 h0 h1 part0 n_parts")
# the same over the sub-rows [s0, s1) a rank sends, with its own destinations [o0, o1) and receive rows [r0, r1)
PartsChunk = collections.namedtuple("PartsChunk", "s0 s1 i0 i1 h0 h1 part0 n_parts o0 o1 r0 r1")


def plan_chunks(plan, chunk_rows):
    """[Chunk] per chunk of `chunk_rows` output positions"""
    out = []
    n = plan["n"]
    for k0 in range(0, n, chunk_rows):
        k1 = min(n, k0 + chunk_rows)
        h0, h1 = (int(x) for x in np.searchsorted(plan["hub_pos"], [k0, k1]))
        p0, p1 = int(plan["part_first"][k0]), int(plan["part_first"][k1])
        out.append(Chunk(k0, k1, int(plan["item_first"][k0]), int(plan["item_first"][k1]), h0, h1, p0, p1 - p0))
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
    """drop the cached graph of (indptr, indices) (all cached graphs when both are None), with its device memory, and
    the rank plans of full_inference_parts over it"""
    def keep(e):
        return not ((indptr is None or e[0] is indptr) and (indices is None or e[1] is indices))
    _GRAPHS[:] = [e for e in _GRAPHS if keep(e)]
    _RANKS[:] = [e for e in _RANKS if keep(e)]


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


class _RowChunks(object):
    """The rows [r0, r1) of a layer's input table as a float32 GEMM operand, r1 - r0 <= chunk_rows: a float32 table's
    rows in place; a 16-bit table's upcast (csl_upcast_rows_x16) into ONE reusable buffer [min(chunk_rows, rows), width]
    -- the float32 path's chunk boundaries, shapes and row stride, so the GEMM computes the same bits."""

    def __init__(self, h, chunk_rows):
        self.h, self.kind, self.buf = h, _kind(h), None
        if self.kind is not None:
            self.buf = torch.empty((min(chunk_rows, max(h.shape[0], 1)), h.shape[1]), dtype=torch.float32, device=h.device)

    def __call__(self, r0, r1):
        h = self.h
        if self.kind is None:
            return h[r0:r1]
        _chk(_lib().csl_upcast_rows_x16(_ptr(h, r0 * h.stride(0)), self.kind, h.stride(0), r1 - r0, _ptr(self.buf),
                                        self.buf.stride(0), h.shape[1], aggr._stream()), "csl_upcast_rows_x16")
        return self.buf[:r1 - r0]


def _project_rows(h, w, out, chunk_rows, bias=None):
    """out[r] = h[r] . w^T (+ bias) for every row, chunk by chunk (shapes that repeat; no GEMM over 10^7 rows)"""
    rows = _RowChunks(h, chunk_rows)
    for r0 in range(0, h.shape[0], chunk_rows):
        r1 = min(h.shape[0], r0 + chunk_rows)
        _gemm_into(out[r0:r1], rows(r0, r1), w, bias)


def _partial(n_rows, width, device):
    return torch.empty((max(n_rows, 1), width), dtype=torch.float32, device=device)


def _list_args(indptr, indices, items, hubs, c, pos0):
    """the leading arguments of every kernel that walks a work list: the CSR, chunk c's slice of items and hubs, the
    chunk's first position and first partial row"""
    return (_ptr(indptr), _ptr(indices), _ptr(items, 4 * c.i0), c.i1 - c.i0,
            _ptr(hubs, 4 * c.h0) if c.h1 > c.h0 else C.c_void_p(0), c.h1 - c.h0, pos0, c.part0)


def sage_rows(g, dplan, x, ldx, W, proj, bias, relu, out, chunk_rows, scratch=None):
    """csl_infer_sage_f32 over every chunk of the plan; out row k of the plan is out[k] (proj) -- for the aggregate-first
    form `out` is a callable (k0, k1) -> the chunk's operand buffer, and `scratch` is called after each chunk.  x may be
    a 16-bit feature table (aggregate-first only): csl_infer_sage_x16 reads it in place."""
    twins, kind = aggr._twins("infer_sage"), _kind(x)
    st = aggr._stream()
    for c in dplan.chunks(chunk_rows):
        part = _partial(c.n_parts, W, x.device) if c.n_parts else None
        dst = out(c.k0, c.k1) if callable(out) else out[c.k0:c.k1]
        aggr._table_call(twins, kind, _list_args(g.indptr, g.indices, dplan.items, dplan.hubs, c, c.k0) + (_ptr(x),),
                         (ldx, W, int(proj), _ptr(bias), int(relu), _ptr(part), _ptr(dst), dst.stride(0), st), _chk)
        if scratch is not None:
            scratch(c.k0, c.k1, dst)


def gat_rows(g, dplan, z, el, er, H, D, slope, bias, last, n_cls, out, chunk_rows):
    L = _lib()
    st = aggr._stream()
    pld = int(L.csl_infer_gat_partial_ld(H, D))
    for c in dplan.chunks(chunk_rows):
        part = _partial(c.n_parts, pld, z.device) if c.n_parts else None
        dst = out[c.k0:c.k1]
        _chk(L.csl_infer_gat_f32(*_list_args(g.indptr, g.indices, dplan.items, dplan.hubs, c, c.k0), _ptr(z), _ptr(el),
                                 _ptr(er), H, D, float(slope), _ptr(bias), int(last), int(n_cls), _ptr(part), _ptr(dst),
                                 dst.stride(0), st),
             "csl_infer_gat_f32")


def _sage_operands(conv, hp, dev):
    """(agg_first, weight, bias) of a DistSageConv on an [*, hp] input table (hp % 4 == 0).  Aggregate first (out >= in):
    the Linear's weight [out, 2 hp] over the operand [h[v] | mean h[u]], its halves at columns 0 and hp, and its bias.
    Project first: [W_self; W_neigh] as [2 op, hp] (op = round4(out)), the halves at rows 0 and op, and the bias padded
    to op.  Every padding entry is zero."""
    W, b = conv.fc.weight.detach().float(), conv.fc.bias.detach().float()
    out_w, in_w = W.shape[0], W.shape[1] // 2
    if out_w >= in_w:
        wc = torch.zeros((out_w, 2 * hp), dtype=torch.float32, device=dev)
        wc[:, :in_w], wc[:, hp:hp + in_w] = W[:, :in_w], W[:, in_w:]
        return True, wc, b
    op = _r4(out_w)
    wp = torch.zeros((2 * op, hp), dtype=torch.float32, device=dev)
    wp[:out_w, :in_w], wp[op:op + out_w, :in_w] = W[:, :in_w], W[:, in_w:]
    bp = torch.zeros((op,), dtype=torch.float32, device=dev)
    bp[:out_w] = b
    return False, wp, bp


def _layer_norm(model, k):
    """(gamma, beta, eps) of a normalised GraphSAGE model's layer k, None for every other layer and model"""
    if getattr(model, "norm", None) is None or k + 1 >= len(model.convs):
        return None
    m = model.norms[k]
    return m.gamma.detach(), m.beta.detach(), model.norm_eps


def _norm_rows(y, norm):
    """a finished chunk of a normalised layer's rows: relu(gamma * layer_norm(y) + beta) in place, forward-only
    (csl_layernorm_relu_fwd_f32 without xhat / rstd).  The layer's own kernels ran with their ReLU off."""
    if norm is not None and y.shape[0]:
        aggr.layernorm_relu(y, norm[0], norm[1], norm[2], relu=True, out=y, store=False)


def _sage_layer(g, dplan, h, conv, relu, chunk_rows, norm=None):
    """One DistSageConv over the rows of `dplan`; h: [N, hp] table (hp % 4 == 0, padding columns zero; float32, or the
    first layer's feature table in its stored 16-bit type, row stride h.stride(0)).  Aggregate first when out >= in,
    project first otherwise.  norm: _layer_norm's tuple: the layer's kernels run without their ReLU and every finished
    chunk of rows is normalised in place (a normalised width is a multiple of 4: no padding columns).
    Returns the [rows, round4(out)] float32 table (padding columns zero)."""
    dev = h.device
    agg_first, w, b = _sage_operands(conv, h.shape[1], dev)
    out_w = conv.fc.weight.shape[0]
    hp, op = h.shape[1], _r4(out_w)
    n_rows = dplan.plan["n"]
    relu = relu and norm is None
    if agg_first:
        # (a) [h[v] | mean h[u]] chunk by chunk, then the Linear with its bias / ReLU epilogue into the output table
        y = torch.zeros((n_rows, op), dtype=torch.float32, device=dev)
        cat = torch.empty((min(chunk_rows, max(n_rows, 1)), 2 * hp), dtype=torch.float32, device=dev)

        def finish(k0, k1, c):
            _gemm_into(y[k0:k1, :out_w], c, w, b, relu)
            _norm_rows(y[k0:k1], norm)
        sage_rows(g, dplan, h, h.stride(0), hp, False, None, False, lambda k0, k1: cat[:k1 - k0], chunk_rows, scratch=finish)
        return y
    # (b) P = h . [W_self; W_neigh]^T once for every node, then act(P[v, :out] + mean P[u, out:] + b) in one pass
    P = torch.empty((g.N, 2 * op), dtype=torch.float32, device=dev)
    _project_rows(h, w, P, chunk_rows)
    y = torch.empty((n_rows, op), dtype=torch.float32, device=dev)
    sage_rows(g, dplan, P, 2 * op, op, True, b, relu, y, chunk_rows,
              scratch=None if norm is None else (lambda k0, k1, dst: _norm_rows(dst, norm)))
    return y


_GatOps = collections.namedtuple("_GatOps", "H D Dp wz al ar bz vl vr cmap")


def _gat_operands(conv, in_map, hp, dev):
    """The operands of a DistGATConv on an [*, hp] input table whose logical column c sits at in_map[c], every head
    padded to Dp = round4(D) columns with zeros: wz [H Dp, hp], al / ar / bz [H, Dp], cmap (where the layer's logical
    output column sits in its [*, H Dp] table), and for Dp > 256 vl / vr [H, hp] (else None)."""
    H, D = conv.H, conv.D
    Dp = _r4(D)
    Wt = conv.fc.weight.detach().float().view(H, D, -1)
    wz = torch.zeros((H, Dp, hp), dtype=torch.float32, device=dev)
    wz[:, :D, in_map] = Wt
    wz = wz.view(H * Dp, hp)
    al = torch.zeros((H, Dp), dtype=torch.float32, device=dev)
    ar = torch.zeros((H, Dp), dtype=torch.float32, device=dev)
    bz = torch.zeros((H, Dp), dtype=torch.float32, device=dev)
    al[:, :D], ar[:, :D], bz[:, :D] = conv.attn_l.detach(), conv.attn_r.detach(), conv.bias.detach().view(H, D)
    vl = vr = None
    if Dp > 256:
        # csl_gat_logits_fwd_f32 holds a head in one wave (D <= 256): wider heads take el = h . (W_h^T a_l[h]) and er
        # likewise, two [N, H] GEMMs on the layer's input (the same logits, summed in another order)
        wv = wz.view(H, Dp, hp)
        vl, vr = torch.einsum("hdf,hd->hf", wv, al).contiguous(), torch.einsum("hdf,hd->hf", wv, ar).contiguous()
    cmap = (torch.arange(H, device=dev)[:, None] * Dp + torch.arange(D, device=dev)[None, :]).reshape(-1)
    return _GatOps(H, D, Dp, wz, al, ar, bz, vl, vr, cmap)


def _gat_project(h, ops, n_rows, chunk_rows):
    """(z [n_rows, H Dp], el, er [max(n_rows, 1), H]) of the rows of h, chunk by chunk.  (The upcast buffer of a 16-bit
    table goes back on return: before the caller allocates the layer's outputs or exchange buffers.)"""
    dev, H, Dp = h.device, ops.H, ops.Dp
    z = torch.empty((n_rows, H * Dp), dtype=torch.float32, device=dev)
    el = torch.empty((max(n_rows, 1), H), dtype=torch.float32, device=dev)
    er = torch.empty((max(n_rows, 1), H), dtype=torch.float32, device=dev)
    AL, st = aggr._lib(), aggr._stream()
    rows = _RowChunks(h, chunk_rows)
    for r0 in range(0, n_rows, chunk_rows):
        r1 = min(n_rows, r0 + chunk_rows)
        hc = rows(r0, r1)
        _gemm_into(z[r0:r1], hc, ops.wz)
        if ops.vl is not None:
            _gemm_into(el[r0:r1], hc, ops.vl)
            _gemm_into(er[r0:r1], hc, ops.vr)
        else:
            _chk(AL.csl_gat_logits_fwd_f32(_ptr(z[r0]), _ptr(ops.al), _ptr(ops.ar), r1 - r0, H, Dp, _ptr(el[r0]),
                                           _ptr(er[r0]), st), "csl_gat_logits_fwd_f32")
    return z, el, er


def _gat_layer(g, dplan, h, in_map, conv, last, n_cls, chunk_rows):
    """One DistGATConv over the rows of `dplan`; h: [N, hp] table whose logical column c sits at in_map[c] (float32, or
    the first layer's feature table in its stored 16-bit type: its rows reach the GEMMs through _RowChunks).  Returns
    (table, its column map): hidden layers [N, H * round4(D)], the last [rows, n_cls]."""
    ops = _gat_operands(conv, in_map, h.shape[1], h.device)
    z, el, er = _gat_project(h, ops, g.N, chunk_rows)
    out = torch.empty((dplan.plan["n"], n_cls if last else ops.H * ops.Dp), dtype=torch.float32, device=h.device)
    gat_rows(g, dplan, z, el, er, ops.H, ops.Dp, conv.slope, ops.bz, last, n_cls if last else 0, out, chunk_rows)
    return out, (None if last else ops.cmap)


# ------------------------------------------------------------------ public interface

def _feat16_dtype(features):
    """torch.float16 / torch.bfloat16 if `features` holds 16-bit elements (a tensor of either type, a float16 host
    array), else None: everything else takes the float32 path"""
    if torch.is_tensor(features):
        return features.dtype if features.dtype in aggr.FEAT_KINDS else None
    return torch.float16 if getattr(features, "dtype", None) == np.float16 else None


def _feat16_in_place(t, zero_padded):
    """The [rows, round4(F)] view of the 16-bit device table t [rows, F] that the first layer can read in place, or None
    (a copy is needed): unit column stride, a row stride that is a multiple of 4 and at least round4(F), an 8-byte aligned
    base, and either F % 4 == 0 or the caller's word (zero_padded) that the columns F .. round4(F) of every row are
    stored and hold zeros.  An empty table is never read in place (the kernels refuse a null table)."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dim() != 2 or t.shape[0] == 0:
        return None
    F, w = t.shape[1], _r4(t.shape[1])
    if t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < w or t.data_ptr() % 8:
        return None
    if w == F:
        return t
    if not zero_padded or (t.storage_offset() + (t.shape[0] - 1) * t.stride(0) + w) * 2 > t.untyped_storage().nbytes():
        return None
    return t.as_strided((t.shape[0], w), (t.stride(0), 1))


def _table16(features, rows, view, dtype, dev):
    """the first layer's table of a 16-bit input: the in-place view, else a zero-padded 16-bit device copy
    [rows, round4(F)] (2 bytes per element, never a float32 copy); without rows an empty float32 table"""
    if view is not None:
        return view
    F = features.shape[1]
    if rows == 0:
        return torch.zeros((0, _r4(F)), dtype=torch.float32, device=dev)
    h = torch.zeros((rows, _r4(F)), dtype=dtype, device=dev)
    h[:, :F].copy_(torch.as_tensor(features))
    return h


def _first_table(features, rows, zero_padded, dev):
    """How the first layer's input table [rows, round4(F)] comes about, decided before anything is allocated:
    (make, feat_size, feat_copy, upload_bytes).  make() returns the table -- to be called once the memory check has
    passed; feat_size: bytes per element of the feature table, feat_copy: whether a 16-bit device copy is made
    (_need_bytes counts it), upload_bytes: those of the padded float32 device copy of a float32 input that cannot be
    used in place (a device tensor with F % 4 == 0 and dense rows can)."""
    F = features.shape[1]
    dt16 = _feat16_dtype(features)
    if dt16 is not None:
        view = _feat16_in_place(features, zero_padded)
        return (lambda: _table16(features, rows, view, dt16, dev)), 2, view is None, 0
    if (torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32 and F % 4 == 0
            and features.stride(1) == 1 and features.stride(0) == F):
        return (lambda: features), 4, False, 0

    def upload():
        h = torch.zeros((rows, _r4(F)), dtype=torch.float32, device=dev)
        if rows:
            h[:, :F] = torch.as_tensor(features).to(dev, torch.float32)
        return h
    return upload, 4, False, rows * _r4(F) * 4


def _input_bytes(k, rows, width, chunk_rows, gemm_form, feat_size, feat_copy):
    """the bytes layer k's input table contributes: rows width 4 for a float32 table (every layer after the first, and
    a float32 feature table); for a 16-bit feature table (k == 0, feat_size == 2) rows width 2 only if a device copy of
    it is made (feat_copy), plus, where the library GEMM reads it (gemm_form), the one upcast buffer
    min(chunk_rows, rows) width 4"""
    if k > 0 or feat_size == 4:
        return rows * width * 4
    return (rows * width * 2 if feat_copy else 0) + (min(chunk_rows, rows) * width * 4 if gemm_form else 0)


def _need_bytes(model, N, n_out, F, chunk_rows, max_parts, feat_size=4, feat_copy=False):
    """the device bytes full_inference allocates at its peak (the graph and plan not included): per layer its input
    table (_input_bytes), its float32 output table and its scratch; feat_size: bytes per element of the feature table"""
    need, width = 0, _r4(F)
    if isinstance(model, splitgnn.DistSAGEModel):
        for k, conv in enumerate(model.convs):
            out_w, in_w = conv.fc.weight.shape[0], conv.fc.weight.shape[1] // 2
            rows = n_out if k + 1 == len(model.convs) else N
            op = _r4(out_w)
            t = rows * op
            if out_w >= in_w:
                t += min(chunk_rows, rows) * 2 * width + max_parts * width
            else:
                t += N * 2 * op + max_parts * op
            t = 4 * t + _input_bytes(k, N, width, chunk_rows, out_w < in_w, feat_size, feat_copy)
            need, width = max(need, t), op
    else:
        for k, conv in enumerate(model.convs):
            last = k + 1 == len(model.convs)
            C_ = conv.H * _r4(conv.D)
            t = N * C_ + 2 * N * conv.H + (n_out * model.n_classes if last else N * C_)
            t += max_parts * (C_ + 2 * conv.H + 4)
            t = 4 * t + _input_bytes(k, N, width, chunk_rows, True, feat_size, feat_copy)
            need, width = max(need, t), C_
    return need


def _free_bytes(device):
    free, _ = torch.cuda.mem_get_info(device)
    return free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)   # torch's cached blocks


def _check_memory(need, device):
    free = _free_bytes(device)
    if need > free:
        raise MemoryError("full_inference needs %d bytes of device memory, %d are free" % (need, free))


def _check_model(model, who):
    """what `who` (full_inference / full_inference_parts) refuses about its model before anything else"""
    if not isinstance(model, (splitgnn.DistSAGEModel, splitgnn.DistGATModel)):
        raise TypeError(who + " takes a DistSAGEModel or a DistGATModel")
    if isinstance(model, splitgnn.DistGATModel) and model.convs[-1].H * _r4(model.convs[-1].D) > GAT_LAST_MAX_C:
        raise ValueError("%s: the attention model's last layer has heads x classes (padded to 4) = %d > %d columns%s"
                         % (who, model.convs[-1].H * _r4(model.convs[-1].D), GAT_LAST_MAX_C,
                            "; its head mean stages a row in LDS" if who == "full_inference" else ""))


def load_model(path, device=None):
    """The model of a checkpoint file (cslicer.checkpoint, Trainer.save_checkpoint) on `device` (default: the current
    GPU): a DistSAGEModel / DistGATModel built from the file's `model` block with the stored weights, ready for
    full_inference / evaluate / full_inference_parts -- no Trainer, no engine.  ValueError for a file that is no
    checkpoint."""
    from . import checkpoint
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return checkpoint.model_from(checkpoint.read(path), device)


def _class_columns(model, h):
    """the last table without a GraphSAGE model's padding columns (the attention model's last layer writes none)"""
    if isinstance(model, splitgnn.DistSAGEModel):
        n_cls = model.convs[-1].fc.weight.shape[0]
        if h.shape[1] != n_cls:
            h = h[:, :n_cls].contiguous()
    return h


def full_inference(model, indptr, indices, features, nodes=None, chunk_rows=CHUNK_ROWS, _zero_padded=False):
    """float32 logits [len(nodes) (or N), n_classes] on the device of `features` of a DistSAGEModel or DistGATModel
    applied with every neighbour (module docstring).  Hidden layers are computed for all N nodes, the last one only for
    `nodes` (int array of node ids; None: all).  features: float32 [N, F] (a device tensor is used in place when F % 4 == 0;
    anything else is uploaded / padded), or float16 / bfloat16 [N, F]: a device tensor with unit column stride, a row
    stride that is a multiple of 4 and at least round4(F), an 8-byte aligned base and F % 4 == 0 is read in place by the
    first layer (module docstring); any other 16-bit input (a host array, another width, another alignment) becomes a
    zero-padded 16-bit device copy [N, round4(F)], never a float32 one.  The logits are bitwise those of the call on
    the table upcast to float32.  (_zero_padded: the caller's word that the rows of a device table with F % 4 != 0 are
    stored padded to round4(F) with zeros -- the trainer's own storage -- so that it too is read in place.)
    Runs under torch.no_grad() and changes no parameter.  Every width is supported
    except an attention model whose last layer has more than GAT_LAST_MAX_C = 4096 heads x padded-class columns
    (ValueError).  Before allocating, the device bytes it needs (tables, scratch and, on first use of a graph, the
    graph's CSR and work list) are checked against the free memory: MemoryError with both counts."""
    _check_model(model, "full_inference")
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
            nodes = _node_ids(nodes)
            if nodes.size and (nodes.min() < 0 or nodes.max() >= N):
                raise ValueError("nodes outside [0, %d)" % N)
        dlast = g.plan(nodes)
        n_out = dlast.plan["n"]
        max_parts = max([c.n_parts for c in g.all_rows.chunks(chunk_rows) + dlast.chunks(chunk_rows)] + [0])
        first_table, feat_size, feat_copy, upload_bytes = _first_table(features, N, _zero_padded, dev)
        need = _need_bytes(model, N, n_out, F, chunk_rows, max_parts, feat_size, feat_copy)
        need += (0 if g.uploaded() else g.device_bytes()) + (dlast.nbytes() if nodes is not None else 0)
        _check_memory(need + upload_bytes, dev)
        g.upload()
        dlast.upload()
        h = first_table()
        in_map = torch.arange(F, device=dev)
        L = len(model.convs)
        for k, conv in enumerate(model.convs):
            last = k + 1 == L
            dplan = dlast if last else g.all_rows
            if isinstance(model, splitgnn.DistSAGEModel):
                h = _sage_layer(g, dplan, h, conv, not last, chunk_rows, _layer_norm(model, k))
            else:
                h, in_map = _gat_layer(g, dplan, h, in_map, conv, last, model.n_classes, chunk_rows)
        return _class_columns(model, h)


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


def eval_head_multilabel(logits, label_words):
    """(pred_words int32 [n, W], (tp, fp, fn), summed binary cross-entropy) of logits [n, C] against the packed labels
    [n, W = ceil(C / 32)] of the same rows (int32, aggr.pack_labels), in one pass over the logits
    (csl_infer_eval_multilabel_f32): class c is predicted where logits[:, c] > 0; the loss is summed over rows and
    classes (float64, fixed order)."""
    logits = logits if logits.stride(1) == 1 else logits.contiguous()
    n, C_ = logits.shape
    W = aggr.label_words(C_)
    words = torch.as_tensor(label_words).to(logits.device)
    if words.dtype != torch.int32 or words.dim() != 2 or words.shape != (n, W):
        raise ValueError("label_words must be int32 [%d, %d] packed words (aggr.pack_labels)" % (n, W))
    words = words if words.stride(1) == 1 else words.contiguous()
    pred = torch.empty((max(n, 1), W), dtype=torch.int32, device=logits.device)
    loss_row = torch.empty((max(n, 1),), dtype=torch.float32, device=logits.device)
    loss_sum = torch.empty((1,), dtype=torch.float64, device=logits.device)
    counts = torch.empty((3,), dtype=torch.int64, device=logits.device)
    _chk(_lib().csl_infer_eval_multilabel_f32(_ptr(logits), logits.stride(0), n, C_, _ptr(words), max(words.stride(0), W),
                                              _ptr(pred), _ptr(loss_row), _ptr(loss_sum), _ptr(counts), aggr._stream()),
         "csl_infer_eval_multilabel_f32")
    tp, fp, fn = (int(v) for v in counts.tolist())
    return pred[:n], (tp, fp, fn), float(loss_sum.item())


def multilabel_scores(tp, fp, fn, loss_sum, n, n_classes):
    """the dict evaluate(multilabel=True) returns: micro-F1 = 2 tp / (2 tp + fp + fn) (0.0 over an empty denominator),
    the loss as the mean per element"""
    den = 2 * tp + fp + fn
    return {"micro_f1": (2 * tp / den) if den else 0.0, "loss": loss_sum / max(n * n_classes, 1), "n": n,
            "tp": tp, "fp": fp, "fn": fn}


def evaluate(model, indptr, indices, features, nodes, labels, chunk_rows=CHUNK_ROWS, _zero_padded=False, multilabel=False):
    """{"accuracy", "loss", "n"} of the model on `nodes` by full-neighbour inference: argmax accuracy and mean
    cross-entropy.  labels: int [N], the label of every node of the graph (those of `nodes` are used).
    multilabel=True: labels are the packed words int32 [N, ceil(C / 32)] (aggr.pack_labels) and the result is
    {"micro_f1", "loss", "n", "tp", "fp", "fn"} (multilabel_scores)."""
    nodes = _node_ids(nodes)
    lab = torch.as_tensor(labels)
    if multilabel:
        if lab.dim() != 2 or lab.shape[0] != features.shape[0] or lab.dtype != torch.int32:
            raise ValueError("multilabel=True: labels must be the packed int32 words of every node of the graph ([%d, W])"
                             % features.shape[0])
        logits = full_inference(model, indptr, indices, features, nodes=nodes, chunk_rows=chunk_rows,
                                _zero_padded=_zero_padded)
        lab = lab[torch.from_numpy(nodes).to(lab.device)]
        _, (tp, fp, fn), loss = eval_head_multilabel(logits, lab)
        return multilabel_scores(tp, fp, fn, loss, int(nodes.shape[0]), int(logits.shape[1]))
    if lab.dim() != 1 or lab.shape[0] != features.shape[0]:
        raise ValueError("labels must hold one label per node of the graph ([%d])" % features.shape[0])
    logits = full_inference(model, indptr, indices, features, nodes=nodes, chunk_rows=chunk_rows,
                            _zero_padded=_zero_padded)
    lab = lab[torch.from_numpy(nodes).to(lab.device)]
    _, correct, loss = eval_head(logits, lab.to(logits.device))
    n = int(nodes.shape[0])
    return {"accuracy": correct / max(n, 1), "loss": loss / max(n, 1), "n": n}


# ------------------------------------------------------------------ split over ranks (include/cslicer_infer_parts.h)
#
# One process per part, each holding only the rows of the nodes it owns (the trainer's rank path).  A layer is cut as
# the training step cuts it: rank q sums, for every destination v, the neighbours of v that q owns (GraphSAGE: the raw
# sum of Y rows; GAT: the online-softmax state, with er[v] sent by v's owner), the partials go to the owner of v through
# one all_to_all_single, and the owner merges them in rank order and finishes the row.  Destinations are cut into global
# chunks of `chunk_rows` positions, derived from replicated data only, so every rank issues the same collectives, empty
# ones included.  With one part every step is the single-process one and the result is bitwise the same.

def owner_table(N, P, owner=None):
    """int32 [N] owner of every node: `owner` checked, or v % P"""
    if owner is None:
        return (np.arange(N, dtype=np.int64) % P).astype(np.int32)
    owner = np.ascontiguousarray(owner, dtype=np.int32)
    if owner.shape != (N,) or (N and (owner.min() < 0 or owner.max() >= P)):
        raise ValueError("owner must be int32 [%d] with values in [0, %d)" % (N, P))
    return owner


class RankGraph(object):
    """The host data of one rank of P over one graph and owner table, built once (vectorised numpy, O(E)):
      lrow  int32 [N]: the row of every node in its owner's tables (its rank among the owner's nodes, ascending)
      deg   int64 [N]: full neighbour degree
      vsub_ip / vsub_ix: the rank's local-source CSR in node order: for every v, the neighbours of v this rank owns, in
            CSR order, as local rows (int64 [N + 1], int32 [E_r])
      pres  bool [n_own, P]: whether rank q owns a neighbour of the rank's own node (local row order)
    Peak host bytes: neighbour_csr's 13 E (int64 row ids, keep mask, int32 copy), then 13 E here (int32 owner per edge,
    the rank's edge mask, an int32 running count), plus about 40 N of node arrays."""

    def __init__(self, indptr, indices, owner, P, rank):
        ip, ix = neighbour_csr(indptr, indices)
        N = ip.shape[0] - 1
        self.N, self.P, self.rank, self.owner = N, int(P), int(rank), owner
        self.deg = np.diff(ip)
        self.lrow = np.empty(N, dtype=np.int32)
        for p in range(self.P):
            idx = np.flatnonzero(owner == p)
            self.lrow[idx] = np.arange(idx.shape[0], dtype=np.int32)
            if p == self.rank:
                self.own = idx
        self.n_own = int(self.own.shape[0])
        eo = owner[ix]                                       # owner of every edge's source
        mine = eo == self.rank
        cs = np.zeros(ix.shape[0] + 1, dtype=np.int32)       # (< 2^31 edges: neighbour_csr)
        np.cumsum(mine, dtype=np.int32, out=cs[1:])
        self.vsub_ip = np.zeros(N + 1, dtype=np.int64)
        np.cumsum(cs[ip[1:]].astype(np.int64) - cs[ip[:-1]], out=self.vsub_ip[1:])
        del cs
        self.vsub_ix = self.lrow[ix[mine]]
        del mine
        own_edges = np.repeat(owner == self.rank, self.deg)
        self.pres = np.zeros((self.n_own, self.P), dtype=bool)
        self.pres[np.repeat(np.arange(self.n_own, dtype=np.int64), self.deg[self.own]), eo[own_edges]] = True
        self._plans = {}

    def plan(self, chunk_rows, nodes=None):
        """the PartsPlan of the destinations `nodes` (None: every node, cached per chunk_rows)"""
        if nodes is not None:
            return PartsPlan(self, nodes, chunk_rows)
        if chunk_rows not in self._plans:
            self._plans[chunk_rows] = PartsPlan(self, None, chunk_rows)
        return self._plans[chunk_rows]


class PartsPlan(object):
    """The exchange plan of one rank for a destination list (positions k, node D[k]) cut into chunks of chunk_rows
    positions.  Send side: the sub-CSR whose rows are the destinations with a neighbour this rank owns, ordered by
    (chunk, owner, position), its work list (build_plan: the CSL_INFER_SEG rule) and sub_counts [chunks, P] (rows sent to
    each owner per chunk).  Receive side: the rank's own destinations in position order, dst int32 [m, 2] {self row,
    degree}, merge lists ml int32 [m, P] (row of rank q's partial in the chunk's receive buffer, -1: none) and
    own_counts [chunks, P] (rows received from each rank per chunk).  er_src: for the attention model's first
    exchange, the self row of the destination of every receive-buffer row (that exchange sends er[v] back along the
    partials' path).  Rank q's sub_counts[c, p] equals rank p's own_counts[c, q]."""

    def __init__(self, rg, nodes, chunk_rows):
        P, rank = rg.P, rg.rank
        D = np.arange(rg.N, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
        n = D.shape[0]
        self.n, self.chunk_rows, self.P = n, int(chunk_rows), P
        nch = (n + chunk_rows - 1) // chunk_rows
        self.n_chunks = nch
        ck = np.arange(n, dtype=np.int64) // chunk_rows
        od_owner = rg.owner[D]
        # send side
        cnt = (rg.vsub_ip[D + 1] - rg.vsub_ip[D])
        sel = np.flatnonzero(cnt > 0)
        key = ck[sel] * P + od_owner[sel]
        order = sel[np.argsort(key, kind="stable")]
        self.sub_counts = np.bincount(key, minlength=nch * P).reshape(nch, P).astype(np.int64)
        self.sub_first = np.zeros(nch + 1, dtype=np.int64)
        np.cumsum(self.sub_counts.sum(1), out=self.sub_first[1:])
        scnt = cnt[order]
        sub_ip = np.zeros(order.shape[0] + 1, dtype=np.int64)
        np.cumsum(scnt, out=sub_ip[1:])
        self.sub_nodes = D[order]
        idx = np.repeat(rg.vsub_ip[self.sub_nodes] - sub_ip[:-1], scnt) + np.arange(sub_ip[-1], dtype=np.int64)
        self.sub_ip, self.sub_ix = sub_ip, rg.vsub_ix[idx]
        del idx
        self.work = build_plan(sub_ip)
        # receive side
        opos = np.flatnonzero(od_owner == rank)
        self.opos = opos
        od = D[opos]
        m = opos.shape[0]
        self.m = m
        self_row = rg.lrow[od]
        self.dst = np.empty((m, 2), dtype=np.int32)
        self.dst[:, 0], self.dst[:, 1] = self_row, rg.deg[od]
        self.own_first = np.searchsorted(opos, np.arange(nch + 1, dtype=np.int64) * chunk_rows).astype(np.int64)
        pr = rg.pres[self_row]
        cum = np.zeros((m + 1, P), dtype=np.int64)
        np.cumsum(pr, axis=0, out=cum[1:])
        self.own_counts = cum[self.own_first[1:]] - cum[self.own_first[:-1]]
        seg = np.zeros((nch, P), dtype=np.int64)
        np.cumsum(self.own_counts[:, :-1], axis=1, out=seg[:, 1:])
        ci = ck[opos]
        row = seg[ci] + cum[1:] - cum[self.own_first[ci]] - 1
        self.ml = np.where(pr, row, -1).astype(np.int32)
        self.recv_first = np.zeros(nch + 1, dtype=np.int64)
        np.cumsum(self.own_counts.sum(1), out=self.recv_first[1:])
        ii, qq = np.nonzero(pr)
        self.er_src = np.empty(int(self.recv_first[-1]), dtype=np.int64)
        self.er_src[self.recv_first[ci[ii]] + row[ii, qq]] = self_row[ii]
        self.dev = None

    def chunks(self):
        """[PartsChunk] per chunk: its sub-rows, items, hubs and parts, own destinations and receive rows"""
        w = self.work
        out = []
        for c in range(self.n_chunks):
            s0, s1 = int(self.sub_first[c]), int(self.sub_first[c + 1])
            h0, h1 = (int(x) for x in np.searchsorted(w["hub_pos"], [s0, s1]))
            p0, p1 = int(w["part_first"][s0]), int(w["part_first"][s1])
            out.append(PartsChunk(s0, s1, int(w["item_first"][s0]), int(w["item_first"][s1]), h0, h1, p0, p1 - p0,
                                  int(self.own_first[c]), int(self.own_first[c + 1]), int(self.recv_first[c]),
                                  int(self.recv_first[c + 1])))
        return out

    def device_bytes(self, gat):
        b = 4 * (self.sub_ip.shape[0] + self.sub_ix.shape[0]) + self.work["items"].nbytes + self.work["hubs"].nbytes
        return b + self.dst.nbytes + self.ml.nbytes + (self.er_src.nbytes if gat else 0) + 64

    def upload(self, device, gat):
        if self.dev is None:
            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros(4, dtype=a.dtype)).to(device)
            self.dev = {"ip": up(self.sub_ip.astype(np.int32)), "ix": up(self.sub_ix), "items": up(self.work["items"]),
                        "hubs": up(self.work["hubs"]), "dst": up(self.dst), "ml": up(self.ml)}
        if gat and "er_src" not in self.dev:
            self.dev["er_src"] = torch.from_numpy(self.er_src).to(device)
        return self.dev

    def pack(self, width):
        """sub-CSR rows per wave of the partial kernels: one.  Two or four rows per wave were measured slower at every
        width and part count of profiles/infer_parts_bench_products.txt (a slot's narrower column tiles walk the row's
        edges once per tile)."""
        return 1


_RANKS = []   # [(indptr, indices, key, RankGraph)]: the rank plans of the two most recent (graph, owner, P, rank)


def rank_graph(indptr, indices, owner, P, rank):
    """the RankGraph of (indptr, indices) for `rank` of P with the int32 owner table `owner`, built once and cached beside
    the graph (release() drops it)"""
    import hashlib
    key = (int(P), int(rank), hashlib.blake2b(owner.tobytes(), digest_size=16).hexdigest())
    for ip, ix, k, rg in _RANKS:
        if ip is indptr and ix is indices and k == key:
            return rg
    rg = RankGraph(indptr, indices, owner, P, rank)
    _RANKS.insert(0, (indptr, indices, key, rg))
    del _RANKS[2:]
    return rg


def _gather(comm, vals):
    """all-gather of a few int64 per rank: [[...] of rank 0, ...]"""
    dist = comm.dist
    dev = torch.device("cpu") if dist.get_backend(comm.group) == "gloo" else comm.device
    t = torch.tensor(vals, dtype=torch.int64, device=dev)
    out = [torch.empty_like(t) for _ in range(comm.world)]
    dist.all_gather(out, t, group=comm.group)
    return [o.cpu().tolist() for o in out]


def _exchange(comm, recv, R, send, S, send_counts, recv_counts):
    """one all_to_all_single of send[:S] (rows grouped by destination rank) into recv[:R]"""
    comm.exchange_into(recv[:R], send[:S], [int(c) for c in send_counts], [int(c) for c in recv_counts])


def _buffer_rows(pp):
    """(send rows, receive rows, partial rows) of the largest chunk of a plan, each at least 1: a layer's buffers"""
    ch = [PartsChunk(*c) for c in pp.chunks()]
    return (max([c.s1 - c.s0 for c in ch] + [1]), max([c.r1 - c.r0 for c in ch] + [1]),
            max([c.n_parts for c in ch] + [1]))


def _sage_layer_parts(pp, dp, h, conv, relu, comm, norm=None):
    """One DistSageConv over the rank's destinations of `pp`; h: [n_own, hp] own rows (float32, or the first layer's
    feature rows in their stored 16-bit type: the aggregate-first kernels read them in place, the projection through
    _RowChunks).  norm: as _sage_layer's, over the rank's own rows (the norm is row-wise: any partition gives the same
    numbers).  Returns [m, round4(out)]."""
    L, st, dev, kind = _lib(), aggr._stream(), h.device, _kind(h)
    relu = relu and norm is None
    part_twins, merge_twins = aggr._twins("infer_sage_part"), aggr._twins("infer_sage_merge")
    agg_first, w, b = _sage_operands(conv, h.shape[1], dev)
    out_w = conv.fc.weight.shape[0]
    hp, op = h.shape[1], _r4(out_w)
    if agg_first:
        y = torch.zeros((pp.m, op), dtype=torch.float32, device=dev)
        cat = torch.empty((min(pp.chunk_rows, max(pp.m, 1)), 2 * hp), dtype=torch.float32, device=dev)
        Y, ldy, Wy = h, h.stride(0), hp
    else:
        Y = torch.empty((h.shape[0], 2 * op), dtype=torch.float32, device=dev)
        _project_rows(h, w, Y, pp.chunk_rows)
        ldy, Wy = 2 * op, op
        y = torch.empty((pp.m, op), dtype=torch.float32, device=dev)
    pack = pp.pack(Wy)
    S_max, R_max, parts = _buffer_rows(pp)
    send = torch.empty((S_max, Wy), dtype=torch.float32, device=dev)
    recv = torch.empty((R_max, Wy), dtype=torch.float32, device=dev)
    part = _partial(parts, Wy, dev)
    for i, c in enumerate(pp.chunks()):
        # (Y is the layer's input table itself in the aggregate-first form, else the float32 projection)
        aggr._table_call(part_twins, kind if agg_first else None,
                         _list_args(dp["ip"], dp["ix"], dp["items"], dp["hubs"], c, c.s0)
                         + (_ptr(Y, 0 if agg_first else op),), (ldy, Wy, pack, _ptr(part), _ptr(send), st), _chk)
        _exchange(comm, recv, c.r1 - c.r0, send, c.s1 - c.s0, pp.sub_counts[i], pp.own_counts[i])
        merge = (_ptr(dp["dst"], 2 * c.o0), _ptr(dp["ml"], pp.P * c.o0), c.o1 - c.o0, pp.P, _ptr(recv))
        if agg_first:
            aggr._table_call(merge_twins, kind, merge + (_ptr(h),),
                             (h.stride(0), hp, 0, None, 0, _ptr(cat), 2 * hp, st), _chk)
            _gemm_into(y[c.o0:c.o1, :out_w], cat[:c.o1 - c.o0], w, b, relu)
        else:
            _chk(L.csl_infer_sage_merge_f32(*merge, _ptr(Y), 2 * op, op, 1, _ptr(b), int(relu), _ptr(y, c.o0 * op), op, st),
                 "csl_infer_sage_merge_f32")
        _norm_rows(y[c.o0:c.o1], norm)
    return y


def _gat_layer_parts(pp, dp, h, in_map, conv, last, n_cls, comm):
    """One DistGATConv over the rank's destinations of `pp`; h: [n_own, hp] own rows whose logical column c sits at
    in_map[c] (float32, or the first layer's feature rows in their stored 16-bit type).  Returns (table, column map) as
    _gat_layer."""
    L, st, dev = _lib(), aggr._stream(), h.device
    ops = _gat_operands(conv, in_map, h.shape[1], dev)
    H, Dp = ops.H, ops.Dp
    z, el, er = _gat_project(h, ops, h.shape[0], pp.chunk_rows)
    pld = int(L.csl_infer_gat_partial_ld(H, Dp))
    pack = pp.pack(H * Dp)
    S_max, R_max, parts = _buffer_rows(pp)
    send = torch.empty((S_max, pld), dtype=torch.float32, device=dev)
    recv = torch.empty((R_max, pld), dtype=torch.float32, device=dev)
    er_in = torch.empty((S_max, H), dtype=torch.float32, device=dev)
    part = _partial(parts, pld, dev)
    out = torch.empty((pp.m, n_cls if last else H * Dp), dtype=torch.float32, device=dev)
    for i, c in enumerate(pp.chunks()):
        # er of the owned destinations out to the ranks holding their neighbours (the partials' path, reversed)
        er_out = er.index_select(0, dp["er_src"][c.r0:c.r1]) if c.r1 > c.r0 else er[:0]
        _exchange(comm, er_in, c.s1 - c.s0, er_out, c.r1 - c.r0, pp.own_counts[i], pp.sub_counts[i])
        _chk(L.csl_infer_gat_part_f32(*_list_args(dp["ip"], dp["ix"], dp["items"], dp["hubs"], c, c.s0), _ptr(z),
                                      _ptr(el), _ptr(er_in), H, Dp, float(conv.slope), pack, _ptr(part), _ptr(send), st),
             "csl_infer_gat_part_f32")
        _exchange(comm, recv, c.r1 - c.r0, send, c.s1 - c.s0, pp.sub_counts[i], pp.own_counts[i])
        dst = out[c.o0:c.o1]
        _chk(L.csl_infer_gat_merge_f32(_ptr(dp["ml"], pp.P * c.o0), c.o1 - c.o0, pp.P, _ptr(recv), H, Dp, _ptr(ops.bz),
                                       int(last), int(n_cls), _ptr(dst), dst.stride(0), st), "csl_infer_gat_merge_f32")
    return out, (None if last else ops.cmap)


def _need_bytes_parts(model, n_own, F, plans, feat_size=4, feat_copy=False):
    """the device bytes full_inference_parts allocates at its peak (tables and per-chunk buffers; the plans' device
    copies not included): as _need_bytes, over the rank's n_own rows"""
    hid, lastp = plans
    need, width = 0, _r4(F)
    for k, conv in enumerate(model.convs):
        pp = lastp if k + 1 == len(model.convs) else hid
        S, R, parts = _buffer_rows(pp)
        if isinstance(model, splitgnn.DistSAGEModel):
            out_w, in_w = conv.fc.weight.shape[0], conv.fc.weight.shape[1] // 2
            op = _r4(out_w)
            t = pp.m * op
            if out_w >= in_w:
                t += min(pp.chunk_rows, max(pp.m, 1)) * 2 * width + (S + R + parts) * width
            else:
                t += n_own * 2 * op + (S + R + parts) * op
            gemm_form, out_width = out_w < in_w, op
        else:
            C_ = conv.H * _r4(conv.D)
            pld = C_ + 2 * conv.H + 4
            t = n_own * C_ + 2 * n_own * conv.H + pp.m * C_ + (S + R + parts) * pld + S * conv.H
            gemm_form, out_width = True, C_
        t = 4 * t + _input_bytes(k, n_own, width, pp.chunk_rows, gemm_form, feat_size, feat_copy)
        need, width = max(need, t), out_width
    return need


def _nodes_key(nodes):
    import hashlib
    if nodes is None:
        return -1, 0
    h = int.from_bytes(hashlib.blake2b(nodes.tobytes(), digest_size=8).digest(), "little", signed=True)
    return int(nodes.shape[0]), h


def full_inference_parts(model, indptr, indices, features_own, comm, owner=None, nodes=None, chunk_rows=CHUNK_ROWS,
                         _check=None, _zero_padded=False):
    """full_inference on one rank of a split-parallel run: float32 logits [own positions of `nodes`, n_classes] of the
    nodes of `nodes` this rank owns, in `nodes` order (None: every node; see owns()).  Collective over comm (a
    splitgnn.DistComm): every rank calls it with the same model, graph, owner table and nodes.

    features_own: float32, float16 or bfloat16 [n_own, F], the rows of the rank's own nodes in ascending node order (a
    16-bit device table is read in place or copied in its own type as full_inference says; _zero_padded likewise).  owner: int32 [N] owner
    rank of every node (None: v % P).  Hidden layers are computed for the rank's own nodes, the last one for its own
    nodes among `nodes`.  Every rank receives at most P partial rows per own destination and chunk; no rank ever holds
    another rank's feature or hidden rows.  `nodes` is compared across ranks (length and a 64-bit hash: ValueError on
    every rank if they differ), and the device-memory check is agreed on: if one rank would raise MemoryError, every rank
    does, before the first exchange.  With one part the result is bitwise that of full_inference."""
    _check_model(model, "full_inference_parts")
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    P, rank = comm.world, comm.rank
    N = np.asarray(indptr).shape[0] - 1
    dev = features_own.device if torch.is_tensor(features_own) and features_own.is_cuda else comm.device
    if nodes is not None:
        nodes = _node_ids(nodes)
    # arguments that could differ between ranks are agreed on before anything else, so that no rank is left waiting
    err = None
    try:
        owner = owner_table(N, P, owner)
        n_own = int(np.count_nonzero(owner == rank))
        if features_own.shape[0] != n_own:
            raise ValueError("features_own must hold the rank's %d own rows, got %d" % (n_own, features_own.shape[0]))
        if _check is not None:
            _check(n_own)
    except ValueError as ex:
        err = ex
    ln, hs = _nodes_key(nodes)
    got = _gather(comm, [ln, hs, int(err is not None)])
    if any(g[2] for g in got):
        raise err if err is not None else ValueError("full_inference_parts: invalid arguments on another rank")
    if any(g[:2] != got[0][:2] for g in got):
        raise ValueError("full_inference_parts: the ranks were given different nodes (lengths %s)"
                         % [g[0] for g in got])
    if nodes is not None and nodes.size and (nodes.min() < 0 or nodes.max() >= N):
        raise ValueError("nodes outside [0, %d)" % N)
    gat = isinstance(model, splitgnn.DistGATModel)
    with torch.no_grad():
        rg = rank_graph(indptr, indices, owner, P, rank)
        hid = rg.plan(chunk_rows)
        lastp = hid if nodes is None else rg.plan(chunk_rows, nodes)
        F = features_own.shape[1]
        first_table, feat_size, feat_copy, upload_bytes = _first_table(features_own, n_own, _zero_padded, dev)
        need = _need_bytes_parts(model, n_own, F, (hid, lastp), feat_size, feat_copy) + upload_bytes
        need += (0 if hid.dev is not None else hid.device_bytes(gat)) + (lastp.device_bytes(gat) if lastp is not hid else 0)
        short = [g for g in _gather(comm, [int(need), int(_free_bytes(dev))]) if g[0] > g[1]]
        if short:
            raise MemoryError("full_inference_parts needs %d bytes of device memory on a rank where %d are free"
                              % (short[0][0], short[0][1]))
        dh, dl = hid.upload(dev, gat), lastp.upload(dev, gat)
        h = first_table()
        in_map = torch.arange(F, device=dev)
        Lc = len(model.convs)
        for k, conv in enumerate(model.convs):
            last = k + 1 == Lc
            pp, dp = (lastp, dl) if last else (hid, dh)
            if gat:
                h, in_map = _gat_layer_parts(pp, dp, h, in_map, conv, last, model.n_classes, comm)
            else:
                h = _sage_layer_parts(pp, dp, h, conv, not last, comm, _layer_norm(model, k))
        return _class_columns(model, h)


def owns(N, P, rank, nodes, owner=None):
    """bool [len(nodes)]: which of `nodes` rank `rank` owns (the rows full_inference_parts returns on that rank)"""
    nodes = _node_ids(nodes)
    own = (nodes % P) if owner is None else np.asarray(owner)[nodes]
    return own == rank


def evaluate_parts(model, indptr, indices, features_own, comm, nodes, labels_own, owner=None, chunk_rows=CHUNK_ROWS,
                   _zero_padded=False, multilabel=False):
    """evaluate() on one rank of a split-parallel run (collective, see full_inference_parts): {"accuracy", "loss", "n"}
    of the model on `nodes`, the same dict on every rank.  labels_own: int [n_own], the labels of the rank's own nodes in
    ascending node order.  Each rank scores its own nodes among `nodes`; the per-rank (correct, float64 loss sum, n) are
    all-gathered and added in rank order, so the result is reproducible bit for bit.
    multilabel=True: labels_own are the packed words int32 [n_own, ceil(C / 32)]; the per-rank (tp, fp, fn, float64 loss
    sum, n) are gathered and added the same way, the result is multilabel_scores'."""
    nodes = _node_ids(nodes)
    lab = torch.as_tensor(labels_own)

    def check(n_own):
        if multilabel:
            if lab.dim() != 2 or lab.shape[0] != n_own or lab.dtype != torch.int32:
                raise ValueError("multilabel=True: labels_own must be the packed int32 words of the rank's own nodes "
                                 "([%d, W])" % n_own)
        elif lab.dim() != 1 or lab.shape[0] != n_own:
            raise ValueError("labels_own must hold one label per own node of the rank ([%d])" % n_own)
    logits = full_inference_parts(model, indptr, indices, features_own, comm, owner=owner, nodes=nodes,
                                  chunk_rows=chunk_rows, _check=check, _zero_padded=_zero_padded)
    N = np.asarray(indptr).shape[0] - 1
    rg = rank_graph(indptr, indices, owner_table(N, comm.world, owner), comm.world, comm.rank)
    mine = nodes[rg.owner[nodes] == comm.rank] if nodes.size else nodes
    rows = torch.from_numpy(rg.lrow[mine].astype(np.int64)).to(lab.device)
    if multilabel:
        _, (tp, fp, fn), loss = eval_head_multilabel(logits, lab[rows])
        got = _gather(comm, [tp, fp, fn, int(np.float64(loss).view(np.int64)), int(mine.shape[0])])
        t = [0, 0, 0, 0.0, 0]
        for a, b, c, l, n in got:
            t = [t[0] + a, t[1] + b, t[2] + c, t[3] + float(np.int64(l).view(np.float64)), t[4] + n]
        return multilabel_scores(t[0], t[1], t[2], t[3], t[4], int(logits.shape[1]))
    _, correct, loss = eval_head(logits, lab[rows].to(logits.device))
    got = _gather(comm, [correct, int(np.float64(loss).view(np.int64)), int(mine.shape[0])])
    tc, tl, tn = 0, 0.0, 0
    for c, l, n in got:
        tc, tl, tn = tc + c, tl + float(np.int64(l).view(np.float64)), tn + n
    return {"accuracy": tc / max(tn, 1), "loss": tl / max(tn, 1), "n": tn}
