"""Inputs that land on the slicer kernels' dispatch edges (csrc/cslicer_hip.hip, k_sample_body.inc) -- TEST
INFRASTRUCTURE, plain numpy: no GPU, no engine.

On a random graph it is an accident where a frontier, a bucket queue or a by-source list falls relative to a kernel's
internal switch.  Here the three id hashes and the geometry the kernels derive from a layer are restated, and graphs
are built whose layer 0 is known WITHOUT the rng: a frontier row with deg < fanout is taken whole and draws nothing,
and layer 0's frontier is the seed list itself.  So a case can ask for "bucket 0 of 4 receives exactly 4097 queue
entries, all distinct, 4096 of them in pass class 0" and get it.

CASES is the one table both test files read: tests/test_slicer_edges_cpu.py measures, on the CPU oracle's output, the
quantity every case is named for and asserts it equals the case's target exactly; tests/test_gpu_slicer_edges.py runs
the engine against the oracle on the same inputs, bit for bit.  Nothing on the GPU side is asked which path it took.
"""
import functools
from collections import deque

import numpy as np

# ---- the kernels' constants ------------------------------------------------------------------------------------------
TN = 256             # frontier nodes per tile (k_sample, k_emit, k_graph: one tile per block)
QMEAN = 2048         # candidates per dedup bucket: nb = max(1, ceil(C / QMEAN))
HCAP = 4096          # slots of k_bucket's LDS table
REG_ENTRIES = 2048   # RC * BT: queue entries k_bucket keeps in registers; the tail is read again from the queue
BPB = 4              # buckets one k_bucket block resolves
SCT = 4096           # candidates one k_scatter block stages
SCATTER_SCAN = 256   # k_scatter scans ceil(nb / 256) buckets per thread
TT = 2048            # in nodes per tile of k_tsum / k_tptr, 8 per thread
TT_STRIDE = 256      # k_tptr sums the tiles before its own with a stride of 256: loops twice beyond 256 tiles
EP = 8               # candidate steps a k_emit thread preloads
TPB = 4              # tiles per k_sample block once a layer's capacity exceeds TPB_ABOVE tiles
TPB_ABOVE = 128
DS_T = 256           # k_dupseeds walks the seeds in chunks of this many
DEGREE_TILES, COUNT_TILES, SELFIN_TILES = 4, 16, 4    # tiles a block of k_degree / k_count / k_selfin owns
INSERTION_MAX = 24   # k_tsort: insertion sort up to here, heap sort up to T_SORTED_MAX, longer lists left alone
T_SORTED_MAX = 128   # (== cslicer._abi.T_SORTED_MAX == CSL_T_SORTED_MAX: the GPU test checks that)
ERR_BUCKET_FULL = 16

_M32 = np.uint64(0xFFFFFFFF)


def _u64(v):
    return np.asarray(v).astype(np.uint64)


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def _umulhi(a, b):
    return (a * np.uint64(b)) >> np.uint64(32)


# ---- the three id hashes ---------------------------------------------------------------------------------------------
def bucket_of(v, nb):
    """dedup bucket of a node id: umulhi(v * 0x9E3779B1, nb)"""
    return _umulhi(_mul32(_u64(v), 0x9E3779B1), nb).astype(np.int64)


def pass_of(v, npass):
    """which pass of an oversized bucket resolves an id"""
    x = _mul32(_u64(v), 0x27D4EB2F)
    x ^= x >> np.uint64(13)
    return _umulhi(_mul32(x, 0x165667B1), npass).astype(np.int64)


def slot_of(v):
    """first slot an id probes in the 4096-slot table"""
    x = _mul32(_u64(v), 0x85EBCA6B)
    x ^= x >> np.uint64(15)
    x = _mul32(x, 0xC2B2AE35)
    return (x >> np.uint64(32 - 12)).astype(np.int64)


# ---- geometry of a layer ---------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-int(a) // int(b))


def geometry(F, fanout):
    """what the kernels derive from a frontier of F nodes: W, C, nb, tiles, blocks per kernel, steps per tile"""
    W = fanout + 1
    C = F * W
    tiles = ceil_div(F, TN)
    return {"W": W, "C": C, "nb": max(1, ceil_div(C, QMEAN)), "tiles": tiles,
            "degree_blocks": max(1, ceil_div(tiles, DEGREE_TILES)), "count_blocks": max(1, ceil_div(tiles, COUNT_TILES)),
            "selfin_blocks": ceil_div(tiles, SELFIN_TILES), "scatter_blocks": ceil_div(C, SCT),
            "bucket_blocks": ceil_div(max(1, ceil_div(C, QMEAN)), BPB),
            "steps": [ceil_div(min(TN, F - t * TN) * W, TN) for t in range(tiles)]}


def npass_of(cnt):
    """passes k_bucket makes over a bucket of cnt queue entries"""
    return ceil_div(cnt, HCAP // 2) if cnt > HCAP else 1


def bucket_path(cnt):
    return "registers" if cnt <= REG_ENTRIES else "tail" if cnt <= HCAP else "passes"


def tsort_path(length):
    return "insertion" if length <= INSERTION_MAX else "heap" if length <= T_SORTED_MAX else "unsorted"


def sample_tpb(max_batch):
    return TPB if ceil_div(max_batch, TN) > TPB_ABOVE else 1


# ---- what the oracle's output says about a layer ---------------------------------------------------------------------
def queue_ids(sample, layer=0):
    """ids of a layer's bucket queue entries, from the oracle's pre-dedup stream: every entry of nbr_flat (the self
    entry of a row is its first one) except a sampled self loop, which is a hole and never reaches a bucket"""
    flat, counts = np.asarray(sample["nbr_flat"][layer]), np.asarray(sample["nbr_counts"][layer])
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    own = np.repeat(flat[starts], counts)
    keep = flat != own
    keep[starts] = True
    return flat[keep]


def bucket_census(ids, nb):
    """(entries, distinct ids, distinct ids per pass class) per bucket, of a layer's queue ids"""
    b = bucket_of(ids, nb)
    entries = np.bincount(b, minlength=nb).tolist()
    distinct, classes = [], []
    for k in range(nb):
        u = np.unique(ids[b == k])
        distinct.append(len(u))
        npass = npass_of(entries[k])
        classes.append(np.bincount(pass_of(u, npass), minlength=npass).tolist() if len(u) else [0] * npass)
    return entries, distinct, classes


def by_source_lengths(bp):
    """entries per in node of a graph-mode slice's list by source: its edges, plus the self entry of a frontier node"""
    n_in = len(bp["in_nodes"])
    return np.bincount(np.asarray(bp["indices"], dtype=np.int64), minlength=n_in) + \
        np.bincount(np.asarray(bp["self_ids_in"], dtype=np.int64), minlength=n_in)


def parts_with_an_edge(sample, owner, layer=0):
    """[F] bit mask per frontier node: the parts that own at least one of its sampled neighbours (k_emit's `hb`)"""
    flat, counts = np.asarray(sample["nbr_flat"][layer]), np.asarray(sample["nbr_counts"][layer])
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    row = np.repeat(np.arange(len(counts)), counts)
    own = np.repeat(flat[starts], counts)
    edge = flat != own
    hb = np.zeros(len(counts), dtype=np.int64)
    np.bitwise_or.at(hb, row[edge], 1 << owner(flat[edge]))
    return hb


# ---- builders --------------------------------------------------------------------------------------------------------
def assemble(N, seeds, rows):
    """CSR of a graph of N nodes in which only the (distinct) seeds have a row"""
    seeds = np.asarray(seeds, dtype=np.int64)
    assert len(np.unique(seeds)) == len(seeds) and len(rows) == len(seeds)
    deg = np.zeros(N, dtype=np.int64)
    deg[seeds] = [len(r) for r in rows]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.zeros(int(indptr[-1]), dtype=np.int64)
    for s, r in zip(seeds.tolist(), rows):
        indices[indptr[s]:indptr[s] + len(r)] = r
    return indptr, indices


def random_graph(N, max_deg, seed, min_deg=0):
    """degrees uniform in [min_deg, max_deg], neighbours v + (distinct positive offsets): no self loop, no multi-edge"""
    rng = np.random.default_rng(seed)
    assert N > 16 * max_deg
    deg = rng.integers(min_deg, max_deg + 1, size=N)
    off = np.cumsum(rng.integers(1, 16, size=(N, max_deg)), axis=1)
    nbr = (np.arange(N, dtype=np.int64)[:, None] + off) % N
    indices = nbr[np.arange(max_deg)[None, :] < deg[:, None]]
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), indices.astype(np.int64)


def _deal(seeds, entries, lens):
    """rows for the seeds, lens[i] entries each, taken from `entries` in order; an entry equal to the row's own id or
    already in the row waits for the next row (no self loop, no multi-edge)"""
    q = deque(int(x) for x in entries)
    rows = []
    for sid, need in zip((int(s) for s in seeds), lens):
        row, seen, skipped = [], {sid}, []
        while len(row) < need:
            if not q:
                raise ValueError("entries left over that fit no row")
            x = q.popleft()
            if x in seen:
                skipped.append(x)
            else:
                row.append(x)
                seen.add(x)
        q.extendleft(reversed(skipped))
        rows.append(row)
    if q:
        raise ValueError("%d entries not placed" % len(q))
    return rows


def _spread(E, F, cap):
    base, extra = divmod(E, F)
    lens = [base + 1] * extra + [base] * (F - extra)
    assert max(lens) <= cap, "rows of %d entries, the fanout leaves room for %d" % (max(lens), cap)
    return lens


@functools.lru_cache(maxsize=None)
def _ids_by_bucket(N, nb):
    ids = np.arange(N, dtype=np.int64)
    b = bucket_of(ids, nb)
    order = np.argsort(b, kind="stable")
    bounds = np.searchsorted(b[order], np.arange(nb + 1))
    return [ids[order[bounds[k]:bounds[k + 1]]] for k in range(nb)]


def bucket_graph(F, fanout, buckets, N=1 << 20, full_rows=False, seed=0):
    """(indptr, indices, seeds): F distinct seeds whose layer-0 bucket queues are exactly the asked layout.

    buckets[k] = {"seeds": seeds whose id hashes to bucket k, "entries": queue entries of bucket k (self entries of
    those seeds + edge entries), "distinct": distinct ids among them, "classes": optionally the distinct ids per pass
    class (sum == distinct, one figure per pass)}.  len(buckets) must be the nb the kernels derive from (F, fanout).
    Rows have deg < fanout and are taken whole; full_rows: every row has deg == fanout instead (the rows of a
    CSL_FLAG_NO_REPLACE engine, which picks `fanout` DISTINCT positions: the whole row again, in drawn order)."""
    nb = geometry(F, fanout)["nb"]
    assert len(buckets) == nb, "F=%d fanout=%d gives %d buckets" % (F, fanout, nb)
    assert sum(b["seeds"] for b in buckets) == F
    rng = np.random.default_rng(seed)
    seed_ids, seqs = [], []
    for k, spec in enumerate(buckets):
        s, cnt, dis = spec["seeds"], spec["entries"], spec["distinct"]
        assert s <= dis <= cnt, spec
        pool = rng.permutation(_ids_by_bucket(N, nb)[k])
        if spec.get("classes") is not None:
            npass = npass_of(cnt)
            assert len(spec["classes"]) == npass and sum(spec["classes"]) == dis, spec
            pc = pass_of(pool, npass)
            chosen = np.concatenate([pool[pc == c][:m] for c, m in enumerate(spec["classes"])])
            assert len(chosen) == dis, "bucket %d: not enough ids of a pass class" % k
            chosen = rng.permutation(chosen)
        else:
            chosen = pool[:dis]
            assert len(chosen) == dis
        new = chosen[s:]
        e = cnt - s
        assert e >= len(new), spec          # every id that is no seed needs an edge entry
        seed_ids.append(chosen[:s])
        # each new id once, then round and round the bucket's ids
        seqs.append(np.concatenate([new, chosen[np.arange(e - len(new)) % max(dis, 1)]]) if dis else new)
    seeds = rng.permutation(np.concatenate(seed_ids))
    entries = np.concatenate(seqs)
    if full_rows:
        assert len(entries) == F * fanout, (len(entries), F * fanout)
        lens = [fanout] * F
    else:
        lens = _spread(len(entries), F, fanout - 1)
    indptr, indices = assemble(N, seeds, _deal(seeds, entries, lens))
    return indptr, indices, seeds


def slice_graph(P, fanout, seeds_per_part, n_in, N=1 << 16, seed=0):
    """(indptr, indices, seeds) with v % P owners: part g owns seeds_per_part[g] seeds, and its graph-mode slice gets
    exactly n_in[g] in nodes (the self entries of its seeds + n_in[g] - seeds_per_part[g] neighbours nobody else has)"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(N)
    seeds, new = [], []
    for g in range(P):
        mine = ids[ids % P == g]
        assert n_in[g] >= seeds_per_part[g] and len(mine) >= n_in[g]
        seeds.append(mine[:seeds_per_part[g]])
        new.append(mine[seeds_per_part[g]:n_in[g]])
    seeds = rng.permutation(np.concatenate(seeds))
    entries = rng.permutation(np.concatenate(new))
    indptr, indices = assemble(N, seeds, _deal(seeds, entries, _spread(len(entries), len(seeds), fanout - 1)))
    return indptr, indices, seeds


def wide_slice_graph(F, deg, N=1 << 20):
    """(indptr, indices, seeds): seeds 0..F-1, row i = the deg ids F + i*deg .. nobody else has: with one part the slice
    has F * (deg + 1) in nodes"""
    assert F * (deg + 1) <= N
    d = np.zeros(N, dtype=np.int64)
    d[:F] = deg
    return (np.concatenate([[0], np.cumsum(d)]).astype(np.int64), F + np.arange(F * deg, dtype=np.int64),
            np.arange(F, dtype=np.int64))


def tlist_graph(lengths, F=160, P=2, N=1 << 14, seed=0):
    """(indptr, indices, seeds, named): slice 0 (v % P owners) holds, for every L of `lengths`, a source that is NOT a
    frontier node and one that IS, both with a by-source list of exactly L entries (the frontier node's includes its
    self entry ~r, which sorts first), and one source that row 3 holds twice and row 5 once (equal keys).
    named = {"plain": {L: id}, "frontier": {L: id}, "twice": id}"""
    rng = np.random.default_rng(seed)
    n = len(lengths)
    assert max(lengths) < F - n
    ids = rng.permutation(N)
    mine = ids[ids % P == 0]
    plain, front, twice = mine[:n], mine[n:2 * n], int(mine[2 * n])
    others = np.setdiff1d(ids, mine[:2 * n + 1], assume_unique=True)
    seeds = np.concatenate([rng.permutation(others)[:F - n], front])        # the frontier sources come last
    rows = []
    for i in range(F):
        row = [int(plain[k]) for k, L in enumerate(lengths) if i < L] + \
              [int(front[k]) for k, L in enumerate(lengths) if i < L - 1]
        if i == 3:
            row += [twice, twice]
        if i == 5:
            row += [twice]
        rows.append(row)
    indptr, indices = assemble(N, seeds, rows)
    named = {"plain": {L: int(plain[k]) for k, L in enumerate(lengths)},
             "frontier": {L: int(front[k]) for k, L in enumerate(lengths)}, "twice": twice}
    return indptr, indices, seeds, named


def one_part_graph(F, P, part, deg, N=1 << 14, seed=0):
    """(indptr, indices, seeds): every seed and every neighbour has id % P == part, every seed has `deg` neighbours: all
    F frontier nodes have an edge from `part` and are owned by it"""
    rng = np.random.default_rng(seed)
    mine = rng.permutation(np.arange(part, N, P))
    seeds, pool = mine[:F], mine[F:]
    rows = [pool[(i * deg + np.arange(deg)) % len(pool)].tolist() for i in range(F)]
    indptr, indices = assemble(N, seeds, rows)
    return indptr, indices, seeds


def workload_table(kind, N, P):
    """owner tables of the cases: None = v % P"""
    if kind == "mod":
        return None
    if kind == "table":
        return np.random.default_rng(11).integers(0, P, size=N).astype(np.int32)
    if isinstance(kind, tuple) and kind[0] == "all":
        return np.full(N, kind[1], dtype=np.int32)
    raise ValueError(kind)


# ---- the case table --------------------------------------------------------------------------------------------------
# A case: name, family, build() -> {"indptr", "indices", "streams": [seeds per stream], ...}, P, fanouts, owners (the
# workload kinds it runs with), modes, max_batch (None: the longest stream), target: what the CPU test must measure.
CASES = {}


def _case(name, family, build, P, fanouts, target, owners=("mod",), modes=("strict", "graph"), max_batch=None, **kw):
    assert name not in CASES
    CASES[name] = dict(name=name, family=family, build=build, P=P, fanouts=tuple(fanouts), target=target,
                       owners=tuple(owners), modes=tuple(modes), max_batch=max_batch, **kw)


@functools.lru_cache(maxsize=8)
def materialise(name):
    g = CASES[name]["build"]()
    if isinstance(g, tuple):
        g = {"indptr": g[0], "indices": g[1], "streams": [g[2]]}
    return g


def cases_of(*families):
    return [c for c in CASES.values() if c["family"] in families]


# -- k_bucket's three paths: bucket 0 of 4 (512 seeds, fanout 15) receives exactly `cnt` entries
def _split(total, n):
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def _bucket_case(cnt, all_distinct):
    npass = npass_of(cnt)
    if all_distinct:
        dis = cnt
        # multi-pass: one pass class fills the table to the last slot, the last class is empty
        classes = ([HCAP] + _split(dis - HCAP, npass - 2) + [0]) if npass > 1 else None
    else:
        dis = 160
        classes = _split(dis, npass) if npass > 1 else None
    b0 = {"seeds": 128, "entries": cnt, "distinct": dis, "classes": classes}
    rest = [{"seeds": 128, "entries": 300, "distinct": 200} for _ in range(3)]
    target = {"entries": [cnt, 300, 300, 300], "distinct": [dis, 200, 200, 200], "path": bucket_path(cnt),
              "npass": npass, "largest_class": max(classes) if classes else dis}
    _case("bucket-%d-%s" % (cnt, "distinct" if all_distinct else "few"), "bucket",
          lambda: bucket_graph(512, 15, [b0] + rest), 4, (15,), target, owners=("mod", "table"))


BUCKET_COUNTS = (2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145)
for _cnt in BUCKET_COUNTS:
    for _all in (False, True):
        _bucket_case(_cnt, _all)


# -- buckets per block (BPB = 4): nb = 1, 4, 5, 8, and [4097, 0, 2049, 0, 1]
def _blocks_case(name, F, layout):
    _case("blocks-" + name, "blocks", lambda: bucket_graph(F, 15, layout), 4, (15,),
          {"nb": len(layout), "entries": [b["entries"] for b in layout], "distinct": [b["distinct"] for b in layout],
           "bucket_blocks": ceil_div(len(layout), BPB)})


_blocks_case("nb1", 128, [{"seeds": 128, "entries": 1500, "distinct": 700}])
_blocks_case("nb4", 512, [{"seeds": 128, "entries": e, "distinct": d}
                          for e, d in ((1000, 600), (900, 500), (1100, 700), (800, 400))])
_blocks_case("nb5", 640, [{"seeds": 128, "entries": e, "distinct": d}
                          for e, d in ((1000, 600), (900, 500), (1100, 700), (800, 400), (1200, 800))])
_blocks_case("nb8", 1024, [{"seeds": 128, "entries": 900 + 10 * k, "distinct": 500 + k} for k in range(8)])
_blocks_case("nb5-gaps", 640, [{"seeds": 400, "entries": 4097, "distinct": 1000, "classes": [400, 300, 300]},
                               {"seeds": 0, "entries": 0, "distinct": 0},
                               {"seeds": 239, "entries": 2049, "distinct": 2049},
                               {"seeds": 0, "entries": 0, "distinct": 0},
                               {"seeds": 1, "entries": 1, "distinct": 1}])

# -- overflow: 4200 entries in bucket 0, all distinct, 4100 of them in pass class 0 of 3: four ids too many for the table
_case("overflow", "overflow",
      lambda: bucket_graph(512, 15, [{"seeds": 128, "entries": 4200, "distinct": 4200, "classes": [4100, 100, 0]}] +
                           [{"seeds": 128, "entries": 300, "distinct": 200} for _ in range(3)]),
      4, (15,), {"entries": [4200, 300, 300, 300], "npass": 3, "largest_class": 4100}, modes=("strict",))


# -- frontier sizes: where k_degree / k_count / k_selfin / k_emit gain a tile or a block; three streams per round
FRONTIER_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)


def _frontier_build(sizes):
    def build():
        indptr, indices = random_graph(1 << 15, 7, seed=5)
        perm = np.random.default_rng(6).permutation(1 << 15)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        return {"indptr": indptr, "indices": indices, "streams": [perm[offs[i]:offs[i + 1]] for i in range(len(sizes))]}
    return build


for _sizes in ((1, 256, 1025), (255, 1024, 4097), (257, 1023, 4096), (4095, 1, 257)):
    _case("frontier-%d-%d-%d" % _sizes, "frontier", _frontier_build(_sizes), 4, (5, 4),
          {"F": list(_sizes), "tiles": [ceil_div(f, TN) for f in _sizes]})

# -- steps per tile of k_emit (EP = 8 preloaded, double-buffered by parity): W = 8, 9, 16, 17, 32 on a full tile + 1 node
for _f in (7, 8, 15, 16, 31):
    _case("steps-fanout%d" % _f, "steps",
          (lambda f: lambda: {"indptr": None, "streams": [np.random.default_rng(f).permutation(1 << 13)[:257]],
                              "graph": (1 << 13, f + 2, 7)})(_f),
          3, (_f,), {"steps": [_f + 1, 1], "chunks": [ceil_div(_f + 1, EP), 1]})

# -- k_emit's byte counters at 255: all 256 nodes of a tile have an edge from one part and are owned by it
for _name, _P, _part, _own in (("P1", 1, 0, "mod"), ("P4-part3", 4, 3, "mod"), ("P8-part7", 8, 7, ("all", 7))):
    for _f in (4, 255):
        _case("bytes-%s-fanout%d" % (_name, _f), "bytes",
              (lambda P, part, own: lambda: one_part_graph(257, 1 if own != "mod" else P, 0 if own != "mod" else part,
                                                           3))(_P, _part, _own),
              _P, (_f,), {"part": _part, "with_edge_in_tile0": 256, "owned_in_tile0": 256,
                          "flag_bytes_tile0": 256 * (_f + 1)}, owners=(_own,))

# -- k_scatter: C at 4080, 4096, 4112 (one block, exactly one, two); more than 524288 candidates (nb > 256)
for _F in (255, 256, 257):
    _case("scatter-C%d" % (_F * 16), "scatter",
          (lambda F: lambda: {"indptr": None, "streams": [np.random.default_rng(F).permutation(1 << 13)[:F]],
                              "graph": (1 << 13, 17, 8)})(_F),
          4, (15,), {"C": _F * 16, "scatter_blocks": ceil_div(_F * 16, SCT)})
_case("scatter-nb257", "large",
      lambda: {"indptr": None, "streams": [np.random.default_rng(9).permutation(1 << 17)[:32800]],
               "graph": (1 << 17, 17, 9)},
      4, (15,), {"C": 524800, "nb": 257, "buckets_per_thread": 2, "tpb": 4})

# -- k_sample with TPB = 4 (capacity above 128 tiles): a frontier that ends inside a block of four tiles
_case("tpb4", "tpb",
      lambda: {"indptr": None, "graph": (1 << 14, 12, 10),
               "streams": [np.random.default_rng(3).permutation(1 << 14)[:1025],
                           np.random.default_rng(4).permutation(1 << 14)[:2049]]},
      4, (10, 3), {"tpb": 4, "tiles": [5, 9], "tiles_in_last_block": [1, 1]}, max_batch=33000)

# -- slices by source: n_in of slice 0 on the edges of k_tsum / k_tptr's tiles of 2048; part 1 has no in node at all
SLICE_N_IN = (2047, 2048, 2049, 4096, 4097, 1000)
for _n in SLICE_N_IN:
    _case("slice-n_in%d" % _n, "slice", (lambda n: lambda: slice_graph(3, 15, [300, 0, 100], [n, 0, 137]))(_n),
          3, (15, 3), {"n_in": [_n, 0, 137], "ttiles": ceil_div(_n, TT)}, modes=("graph",))
_case("slice-323-tiles", "large", lambda: wide_slice_graph(33000, 19), 1, (20,),
      {"n_in": [660000], "ttiles": 323, "tptr_strides": 2}, modes=("graph",))

# -- by-source list lengths on k_tsort's three boundaries
TLIST_LENGTHS = (1, 2, 23, 24, 25, 26, 127, 128, 129)


def _tlist_build():
    indptr, indices, seeds, named = tlist_graph(TLIST_LENGTHS)
    return {"indptr": indptr, "indices": indices, "streams": [seeds], "named": named}


_case("tlist", "tlist", _tlist_build, 2, (20, 2),
      {"lengths": list(TLIST_LENGTHS), "twice": 3, "t_max_len": 129,
       "paths": [tsort_path(L) for L in TLIST_LENGTHS]}, modes=("graph",))


# -- k_dupseeds across its chunk boundary (chunks of 256 seeds, carried scans)
def _dup_build(runs):
    def build():
        indptr, indices = random_graph(1 << 12, 24, seed=12, min_deg=2)
        rng = np.random.default_rng(13)
        perm = rng.permutation(1 << 12)
        dup = perm[:600].copy()
        for lo, hi in runs:
            dup[lo:hi + 1] = dup[lo]
        return {"indptr": indptr, "indices": indices, "streams": [dup], "plain": perm[600:1200]}
    return build


_case("dup-runs-254-256-511-513", "dup", _dup_build(((254, 256), (511, 513))), 4, (6, 3),
      {"repeats": [[254, 255, 256], [511, 512, 513]]}, owners=("mod", "table"), modes=("strict",))
_case("dup-pair-255-256", "dup", _dup_build(((255, 256),)), 3, (6, 3),
      {"repeats": [[255, 256]]}, owners=("mod",), modes=("strict",))


# -- CSL_FLAG_NO_REPLACE feeds the same queues: rows of deg == fanout are picked whole, in drawn order
def _norep_case(cnt, F, layout):
    _case("norep-%d" % cnt, "norep", lambda: bucket_graph(F, 15, layout, full_rows=True), 4, (15,),
          {"entries": [b["entries"] for b in layout], "path": bucket_path(cnt), "draws": F * 15}, modes=("graph",))


_norep_case(2049, 256, [{"seeds": 128, "entries": 2049, "distinct": 1500},
                        {"seeds": 128, "entries": 2047, "distinct": 1400}])
_norep_case(4097, 512, [{"seeds": 128, "entries": 4097, "distinct": 3000, "classes": [1000, 1000, 1000]}] +
            [{"seeds": 128, "entries": 1365, "distinct": 900} for _ in range(3)])


def graph_of(g):
    """(indptr, indices) of a materialised case: its own, or the random graph it names as (N, max_deg, seed)"""
    if g.get("indptr") is not None:
        return g["indptr"], g["indices"]
    return _random_graph_cached(*g["graph"])


@functools.lru_cache(maxsize=4)
def _random_graph_cached(N, max_deg, seed):
    return random_graph(N, max_deg, seed)


# ---- what a case is named for, measured on the oracle's output -------------------------------------------------------
def measure(case, g, samples, graphs=None):
    """The quantities of case["target"], from the ORACLE's output for the case's streams: samples[s] a strict-mode (or
    restatement) dict with nbr_flat / nbr_counts / frontier, graphs[s] a graph-mode dict.  Compared with == against the
    target: a case that drifts off its edge fails on the CPU before anything runs on a GPU."""
    fam, P, fanout = case["family"], case["P"], case["fanouts"][0]
    s0 = samples[0]
    F = len(s0["frontier"][0])
    geo = geometry(F, fanout)
    if fam in ("bucket", "blocks", "overflow", "norep"):
        entries, distinct, classes = bucket_census(queue_ids(s0), geo["nb"])
        out = {"entries": entries, "distinct": distinct, "nb": geo["nb"], "bucket_blocks": geo["bucket_blocks"],
               "path": bucket_path(entries[0]), "npass": npass_of(entries[0]), "largest_class": max(classes[0]),
               "draws": int(s0["draws"][0])}
    elif fam == "frontier":
        out = {"F": [len(s["frontier"][0]) for s in samples],
               "tiles": [geometry(len(s["frontier"][0]), fanout)["tiles"] for s in samples]}
    elif fam == "steps":
        out = {"steps": geo["steps"], "chunks": [ceil_div(x, EP) for x in geo["steps"]]}
    elif fam == "bytes":
        wl = workload_table(case["owners"][0], len(graph_of(g)[0]) - 1, P)
        owner = (lambda v: wl[v].astype(np.int64)) if wl is not None else (lambda v: np.asarray(v) % P)
        hb = parts_with_an_edge(s0, owner)
        part = case["target"]["part"]
        out = {"part": part, "with_edge_in_tile0": int(((hb[:TN] >> part) & 1).sum()),
               "owned_in_tile0": int((owner(np.asarray(s0["frontier"][0][:TN])) == part).sum()),
               "flag_bytes_tile0": min(F, TN) * geo["W"]}
    elif fam == "scatter":
        out = {"C": geo["C"], "scatter_blocks": geo["scatter_blocks"]}
    elif fam == "tpb":
        tiles = [geometry(len(s["frontier"][0]), fanout)["tiles"] for s in samples]
        out = {"tpb": sample_tpb(case["max_batch"]), "tiles": tiles, "tiles_in_last_block": [t % TPB or TPB for t in tiles]}
    elif fam == "slice":
        n_in = [len(bp["in_nodes"]) for bp in graphs[0]["layers"][0]]
        out = {"n_in": n_in, "ttiles": ceil_div(n_in[0], TT)}
    elif fam == "large" and case["modes"] == ("graph",):
        n_in = [len(bp["in_nodes"]) for bp in graphs[0]["layers"][0]]
        out = {"n_in": n_in, "ttiles": ceil_div(n_in[0], TT), "tptr_strides": ceil_div(ceil_div(n_in[0], TT), TT_STRIDE)}
    elif fam == "large":
        out = {"C": geo["C"], "nb": geo["nb"], "buckets_per_thread": ceil_div(geo["nb"], SCATTER_SCAN),
               "tpb": sample_tpb(F)}
    elif fam == "tlist":
        bp = graphs[0]["layers"][0][0]
        lens = by_source_lengths(bp)
        rank = {int(v): i for i, v in enumerate(bp["in_nodes"])}
        named, frontier = g["named"], set(int(v) for v in s0["frontier"][0])
        assert all(v in frontier for v in named["frontier"].values())
        assert not any(v in frontier for v in named["plain"].values()) and named["twice"] not in frontier
        got = [int(lens[rank[named["plain"][L]]]) for L in case["target"]["lengths"]]
        assert got == [int(lens[rank[named["frontier"][L]]]) for L in case["target"]["lengths"]]
        out = {"lengths": got, "twice": int(lens[rank[named["twice"]]]),
               "t_max_len": max(int(by_source_lengths(b).max()) for b in graphs[0]["layers"][0] if len(b["in_nodes"])),
               "paths": [tsort_path(L) for L in got]}
    elif fam == "dup":
        fr = np.asarray(s0["frontier"][0])
        ids, cnt = np.unique(fr, return_counts=True)
        out = {"repeats": sorted(np.flatnonzero(fr == v).tolist() for v in ids[cnt > 1])}
    else:
        raise ValueError(fam)
    return {k: out[k] for k in case["target"]}
