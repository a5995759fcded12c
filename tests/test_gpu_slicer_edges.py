"""The slicer kernels (csrc/cslicer_hip.hip, k_sample_body.inc) against the oracle at every dispatch edge, bit for bit.

The inputs come from tests/slicer_edges.py: crafted graphs whose layer 0 lands where it is aimed -- a bucket of exactly
2049 queue entries, a slice of exactly 2048 in nodes, a by-source list of 25 entries.  tests/test_slicer_edges_cpu.py
proves on the CPU oracle that every case sits on its edge; nothing here asks the GPU which path it took.  Every case
runs two rounds on one engine (the second, with the seeds reversed, sees the scratch the first left behind); strict mode
keeps the raw candidate stream (FLAG_KEEP_CANDIDATES), graph mode also builds the slices by source of every layer.
Everything is exact: there are no tolerances."""
import ctypes

import numpy as np
import pytest

import slicer_edges as se
from golden_util import assert_same_sample
from test_gpu_graph_mode import assert_same_graph, check_graph_invariants, check_transposed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from cslicer import _abi
    _abi.load()
    assert _abi.T_SORTED_MAX == se.T_SORTED_MAX
    return _abi


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def variants(*families):
    """(case name, mode, owners) of every case of the families"""
    return [pytest.param(c["name"], m, o, id="%s-%s-%s" % (c["name"], m, o if isinstance(o, str) else "all%d" % o[1]))
            for c in se.cases_of(*families) for m in c["modes"] for o in c["owners"]]


def make_engine(abi, case, g, mode, owners, extra_flags=0, part_mask=0):
    indptr, indices = se.graph_of(g)
    wl = se.workload_table(owners, len(indptr) - 1, case["P"])
    B = case["max_batch"] or max(len(s) for s in g["streams"])
    flags = (abi.FLAG_KEEP_CANDIDATES if mode == "strict" else abi.FLAG_TRANSPOSE | abi.FLAG_TRANSPOSE_ALL) | extra_flags
    e = abi.Engine(indptr, indices, n_parts=case["P"], fanouts=case["fanouts"], max_batch=B,
                   n_streams=len(g["streams"]), workload=wl, part_mask=part_mask,
                   mode=abi.MODE_STRICT if mode == "strict" else abi.MODE_GRAPH, flags=flags)
    return e, wl


def compare(e, oracle, seeds, mode, indptr, indices, P, wl, stream, tag):
    if mode == "strict":
        want, got = oracle.sample(seeds), e.sample_dict(stream)        # (sample_dict raises on any device error bit)
        assert_same_sample(got, want, what=tag)
    else:
        want, got = oracle.sample_graph(seeds), e.graph_dict(stream)
        assert_same_graph(got, want, what=tag)
        check_graph_invariants(got, indptr, indices, P, workload=wl)
        check_transposed(got, deepest_too=True)
    assert got["draws_total"] == want["draws_total"], tag
    assert got["sampled_edges"] == want["sampled_edges"], tag
    return got, want


def run_case(abi, orc, name, mode, owners):
    case, g = se.CASES[name], se.materialise(name)
    indptr, indices = se.graph_of(g)
    e, wl = make_engine(abi, case, g, mode, owners)
    oracles = [orc.Oracle(indptr, indices, n_parts=case["P"], fanouts=case["fanouts"], workload=wl) for _ in g["streams"]]
    out = []
    try:
        for r in range(2):
            batches = [s if r == 0 else s[::-1].copy() for s in g["streams"]]
            e.submit_seeds(batches)
            for s, seeds in enumerate(batches):
                out.append(compare(e, oracles[s], seeds, mode, indptr, indices, case["P"], wl, s,
                                   "%s %s round %d stream %d" % (name, mode, r, s))[0])
    finally:
        e.close()
    return out


@pytest.mark.parametrize("name,mode,owners", variants("bucket"))
def test_k_bucket_paths(abi, orc, name, mode, owners):
    """bucket 0 of 4 receives exactly 2047 ... 6145 queue entries: registers only up to 2048, the tail re-read from the
    queue up to 4096, passes over pass_of beyond; few distinct ids, or as many as entries (4096 of them fill the table,
    or one pass's table, to the last slot); v % P owners and a workload table (k_bucket<true>)"""
    run_case(abi, orc, name, mode, owners)


@pytest.mark.parametrize("name,mode,owners", variants("blocks"))
def test_buckets_per_block(abi, orc, name, mode, owners):
    """nb = 1, 4, 5, 8 and [4097, 0, 2049, 0, 1]: a block resolves four buckets and prefetches the next one's entries --
    over an empty bucket, a large one behind a small one, a second block with a single bucket"""
    run_case(abi, orc, name, mode, owners)


def test_a_pass_that_overflows_the_table_is_flagged(abi, orc):
    """4100 distinct ids of one bucket AND one pass class against 4096 slots: CSL_ERR_BUCKET_FULL and no other bit --
    ht_insert gives up after HCAP probes, nothing is mis-sliced silently -- and the engine then slices an ordinary
    minibatch exactly"""
    case, g = se.CASES["overflow"], se.materialise("overflow")
    indptr, indices = se.graph_of(g)
    seeds = g["streams"][0]
    e, wl = make_engine(abi, case, g, "strict", "mod")
    try:
        e.submit_seeds([seeds])
        with pytest.raises(abi.CslError) as ei:
            e.meta(0)
        assert ei.value.code == abi.E_DEVICE
        m = abi.SampleMeta()         # (csl_get_meta fills the meta, error word included, before it reports the error)
        assert abi.load().csl_get_meta(e._h, 0, 0, ctypes.byref(m)) == abi.E_DEVICE
        assert int(m.error) == se.ERR_BUCKET_FULL == [b for b, n in abi.ERR_BITS.items() if n == "BUCKET_FULL"][0]
        rest = np.setdiff1d(np.arange(4000), seeds)[:100]                # (nodes without a row)
        for r, plain in enumerate((np.concatenate([seeds[:250], rest]), seeds[250:])):
            e.submit_seeds([plain])
            o = orc.Oracle(indptr, indices, n_parts=4, fanouts=case["fanouts"])
            compare(e, o, plain, "strict", indptr, indices, 4, wl, 0, "after the overflow, batch %d" % r)
    finally:
        e.close()


@pytest.mark.parametrize("name,mode,owners", variants("frontier"))
def test_frontier_sizes(abi, orc, name, mode, owners):
    """F in {1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097}, three streams of different F per round: where
    k_degree, k_count, k_selfin and k_emit gain a tile or a block and the ticket count of a stream changes"""
    run_case(abi, orc, name, mode, owners)


@pytest.mark.parametrize("name,mode,owners", variants("steps"))
def test_steps_per_tile(abi, orc, name, mode, owners):
    """W = 8, 9, 16, 17, 32 steps on a full tile (and one node in a second tile), P = 3: k_emit preloads 8 steps and
    double-buffers by step parity across chunks"""
    run_case(abi, orc, name, mode, owners)


@pytest.mark.parametrize("name,mode,owners", variants("bytes"))
def test_byte_counters_at_255(abi, orc, name, mode, owners):
    """all 256 nodes of a tile have an edge from one part and are owned by it: k_emit's node-level ranks, byte counters,
    reach exactly 255 -- in the second counter word for part 7 of 8 -- and at fanout 255 k_count reduces unpacked"""
    run_case(abi, orc, name, mode, owners)


@pytest.mark.parametrize("name,mode,owners", variants("scatter", "tpb"))
def test_scatter_blocks_and_sample_tiles_per_block(abi, orc, name, mode, owners):
    """C = 4080, 4096, 4112 candidates against k_scatter's 4096 per block; k_sample with four tiles per block
    (capacity above 128 tiles) and frontiers that end one tile into a block"""
    run_case(abi, orc, name, mode, owners)


@pytest.mark.parametrize("name,mode,owners", variants("large"))
def test_large_layers(abi, orc, name, mode, owners):
    """more than 524288 candidates (nb > 256: k_scatter scans two buckets per thread); a slice of 660000 in nodes
    (323 tiles of k_tptr, whose strided tile-base sum loops twice beyond 256)"""
    run_case(abi, orc, name, mode, owners)


@pytest.mark.parametrize("name,mode,owners", variants("slice"))
def test_slice_sizes_by_source(abi, orc, name, mode, owners):
    """n_in of slice 0 at 2047, 2048, 2049, 4096, 4097 and 1000 (k_tsum / k_tptr: tiles of 2048, eight per thread, one
    thread closes the row pointers), next to a part without any in node"""
    got = run_case(abi, orc, name, mode, owners)
    assert [len(bp["in_nodes"]) for bp in got[0]["layers"][0]] == se.CASES[name]["target"]["n_in"]
    assert len(got[0]["layers"][0][1]["t_indptr"]) == 1


def test_by_source_list_lengths(abi, orc):
    """lists of 1, 2, 23, 24, 25, 26, 127, 128, 129 entries in one slice, for sources that are and are not frontier
    nodes, and one source a row holds twice: k_tsort's insertion sort, heap sort and hands-off ranges.  Up to
    T_SORTED_MAX the order is pinned (~r of the self entry first, then the rows ascending), 129 as a multiset
    (check_transposed); t_max_len is exact"""
    case, g = se.CASES["tlist"], se.materialise("tlist")
    for r, d in enumerate(run_case(abi, orc, "tlist", "graph", "mod")):
        bp = d["layers"][0][0]
        rank = {int(v): i for i, v in enumerate(bp["in_nodes"])}
        ptr, idx = bp["t_indptr"], bp["t_indices"]
        for kind in ("plain", "frontier"):
            for L, v in g["named"][kind].items():
                lst = idx[ptr[rank[v]]:ptr[rank[v] + 1]]
                assert len(lst) == L, (kind, L)
                # the self entry ~r of a frontier node is the list's one negative entry
                assert int((lst < 0).sum()) == (kind == "frontier"), (kind, L, lst)
                if L <= abi.T_SORTED_MAX:          # pinned order: ~r first, then the rows ascending
                    assert (np.diff(lst) >= 0).all(), (kind, L, lst)
                # (a longer list is in unspecified order: check_transposed compared it as a multiset)
        tw = idx[ptr[rank[g["named"]["twice"]]]:ptr[rank[g["named"]["twice"]] + 1]]
        assert len(tw) == 3 and len(np.unique(tw)) == 2 and (np.diff(tw) >= 0).all(), tw
        assert bp["t_max_len"] == case["target"]["t_max_len"]


@pytest.mark.parametrize("name,mode,owners", variants("dup"))
def test_k_dupseeds_across_its_chunk_boundary(abi, orc, name, mode, owners):
    """runs of three equal seed ids at indices 254-256 and 511-513, and an id at 255 and 256: the `previous push carried
    the same id` rule across k_dupseeds' chunks of 256; a distinct-seed minibatch before and after on the same stream"""
    case, g = se.CASES[name], se.materialise(name)
    indptr, indices = se.graph_of(g)
    dup, plain = g["streams"][0], g["plain"]
    e, wl = make_engine(abi, case, {**g, "streams": [dup, dup]}, "strict", owners)
    oracles = [orc.Oracle(indptr, indices, n_parts=case["P"], fanouts=case["fanouts"], workload=wl) for _ in range(2)]
    try:
        for r, batches in enumerate(([plain, dup], [dup, plain], [dup[::-1].copy(), dup], [plain, plain])):
            e.submit_seeds(batches)
            for s in range(2):
                compare(e, oracles[s], batches[s], "strict", indptr, indices, case["P"], wl, s,
                        "%s round %d stream %d" % (name, r, s))
    finally:
        e.close()


@pytest.mark.parametrize("name,part", [("bucket-4097-few", 2), ("tlist", 0)])
def test_part_mask_on_the_edges(abi, name, part):
    """a mask of one part on two of the cases above: the lists of that part, every size and offset in the meta, the
    frontiers and the draw counts equal the unmasked engine's"""
    case, g = se.CASES[name], se.materialise(name)
    full, _ = make_engine(abi, case, g, "graph", "mod")
    e, _ = make_engine(abi, case, g, "graph", "mod", part_mask=1 << part)
    try:
        for eng in (full, e):
            eng.submit_seeds(g["streams"])
        m0, m1 = full.meta(0), e.meta(0)
        # sizes, offsets, rng positions: all of the meta -- but for t_max_len of the parts left out, a figure about
        # the CONTENTS of a list by source that is not built: it stays 0
        want = type(m0).from_buffer_copy(bytes(m0))
        for l in range(len(case["fanouts"])):
            for p in range(case["P"]):
                if p != part:
                    assert m1.layer[l].t_max_len[p] == 0
                    want.layer[l].t_max_len[p] = 0
            assert m1.layer[l].t_max_len[part] == m0.layer[l].t_max_len[part]
        assert bytes(want) == bytes(m1)
        for l in range(len(case["fanouts"])):
            np.testing.assert_array_equal(full.copy_frontier(l + 1, 0), e.copy_frontier(l + 1, 0))
            lists = [[eng.copy_list(l, k, part, 0, meta=m) for k in range(abi.NUM_LISTS)] for eng, m in ((full, m0), (e, m1))]
            ptr = lists[0][abi.T_INDPTR]
            for k in range(abi.NUM_LISTS):
                a, b = lists[0][k].copy(), lists[1][k].copy()
                if k == abi.T_INDICES:
                    # a list by source longer than T_SORTED_MAX is in unspecified order in either engine: as a multiset
                    for u in np.flatnonzero(np.diff(ptr) > abi.T_SORTED_MAX):
                        a[ptr[u]:ptr[u + 1]].sort()
                        b[ptr[u]:ptr[u + 1]].sort()
                np.testing.assert_array_equal(a, b, err_msg="%s layer %d kind %d" % (name, l, k))
    finally:
        full.close()
        e.close()


@pytest.mark.parametrize("name", [c["name"] for c in se.cases_of("norep")])
def test_no_replace_feeds_the_same_queues(abi, name):
    """CSL_FLAG_NO_REPLACE (k_sample_norep) with every row at deg == fanout: all rows draw, the picks are the whole row
    in drawn order, and bucket 0 receives 2049 / 4097 entries -- asserted on the restatement's own output"""
    from noreplace_ref import GraphRef
    case, g = se.CASES[name], se.materialise(name)
    indptr, indices = se.graph_of(g)
    e, _ = make_engine(abi, case, g, "graph", "mod", extra_flags=abi.FLAG_NO_REPLACE | abi.FLAG_KEEP_CANDIDATES)
    ref = GraphRef(indptr, indices, case["P"], case["fanouts"], replace=False)
    try:
        for r in range(2):
            seeds = g["streams"][0] if r == 0 else g["streams"][0][::-1].copy()
            e.submit_seeds([seeds])
            want = ref.sample_graph(seeds)
            assert se.measure(case, g, [want]) == case["target"]
            m, got = e.meta(0), e.graph_dict(0)
            assert_same_graph(got, want, what="%s round %d" % (name, r))
            assert [int(m.layer[0].draws), got["draws_total"], got["sampled_edges"]] == \
                [want["draws"][0], want["draws_total"], want["sampled_edges"]]
            flat, counts = e.copy_candidates(0, 0, 0, m)
            np.testing.assert_array_equal(flat, want["nbr_flat"][0])
            np.testing.assert_array_equal(counts, want["nbr_counts"][0])
            check_transposed(got, deepest_too=True)
    finally:
        e.close()
