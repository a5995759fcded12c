"""The inputs of tests/test_gpu_slicer_edges.py are what they claim: for every case of tests/slicer_edges.py the
quantity the case is named for -- queue entries and distinct ids per bucket, passes and the largest pass class, in nodes
per slice, by-source list lengths, steps per tile, ... -- is computed from the CPU ORACLE's output for the case's seeds
and must equal the case's target exactly.  No GPU, no engine: a case cannot drift off its edge without this file
failing first."""
import numpy as np
import pytest

import slicer_edges as se
from noreplace_ref import GraphRef


def oracle_samples(case, g):
    """(strict dicts, graph dicts) per stream, from the C oracle -- from the no-replace restatement for that family"""
    from oracle import oracle as orc
    indptr, indices = se.graph_of(g)
    wl = se.workload_table(case["owners"][0], len(indptr) - 1, case["P"])
    samples, graphs = [], []
    for seeds in g["streams"]:
        if case["family"] == "norep":
            d = GraphRef(indptr, indices, case["P"], case["fanouts"], workload=wl, replace=False).sample_graph(seeds)
            samples.append(d)
            graphs.append(d)
            continue
        samples.append(orc.Oracle(indptr, indices, n_parts=case["P"], fanouts=case["fanouts"], workload=wl).sample(seeds))
        graphs.append(orc.Oracle(indptr, indices, n_parts=case["P"], fanouts=case["fanouts"], workload=wl)
                      .sample_graph(seeds) if "graph" in case["modes"] else None)
    return samples, graphs


@pytest.mark.parametrize("name", list(se.CASES))
def test_the_oracle_puts_the_case_on_its_edge(name):
    case = se.CASES[name]
    g = se.materialise(name)
    samples, graphs = oracle_samples(case, g)
    got = se.measure(case, g, samples, graphs)
    print(name, got)
    assert got == case["target"]
    if case["family"] in ("bucket", "blocks", "overflow", "slice", "tlist", "bytes") or name == "slice-323-tiles":
        assert samples[0]["draws"][0] == 0, "layer 0 of a crafted graph draws nothing: its candidates are known exactly"


def test_the_case_table_names_every_edge():
    """the exact figures of the kernels' switches appear as targets, not as ranges"""
    t = {n: c["target"] for n, c in se.CASES.items()}
    assert sorted({x["entries"][0] for n, x in t.items() if n.startswith("bucket-")}) == \
        [2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145]
    assert [se.bucket_path(c) for c in (2048, 2049, 4096, 4097)] == ["registers", "tail", "tail", "passes"]
    assert t["bucket-4096-distinct"]["distinct"][0] == se.HCAP                  # the table filled to the last slot
    assert t["bucket-4097-distinct"]["largest_class"] == se.HCAP and t["bucket-6145-distinct"]["npass"] == 4
    assert t["blocks-nb5-gaps"]["entries"] == [4097, 0, 2049, 0, 1]
    assert sorted(c["target"]["nb"] for c in se.cases_of("blocks")) == [1, 4, 5, 5, 8]
    assert t["overflow"]["largest_class"] > se.HCAP
    assert sorted({f for c in se.cases_of("frontier") for f in c["target"]["F"]}) == list(se.FRONTIER_SIZES)
    assert [c["target"]["steps"][0] for c in se.cases_of("steps")] == [8, 9, 16, 17, 32]
    assert [c["target"]["C"] for c in se.cases_of("scatter")] == [4080, 4096, 4112]
    assert t["scatter-nb257"]["C"] > 524288 and t["scatter-nb257"]["nb"] > se.SCATTER_SCAN
    assert [c["target"]["n_in"][0] for c in se.cases_of("slice")] == [2047, 2048, 2049, 4096, 4097, 1000]
    assert all(c["target"]["n_in"][1] == 0 for c in se.cases_of("slice"))       # a part with no in node
    assert t["slice-323-tiles"]["ttiles"] > se.TT_STRIDE
    assert t["tlist"]["lengths"] == [1, 2, 23, 24, 25, 26, 127, 128, 129]
    assert t["tlist"]["paths"] == ["insertion"] * 4 + ["heap"] * 4 + ["unsorted"]
    assert any(c["target"]["flag_bytes_tile0"] == 65536 and c["P"] > 4 for c in se.cases_of("bytes"))
    assert t["tpb4"]["tpb"] == se.TPB and se.sample_tpb(32768) == 1


def test_hashes_against_known_values():
    """the restated hashes, on values worked out by hand from the formulas in csrc/cslicer_hip.hip"""
    v = 12345
    h = (v * 0x9E3779B1) & 0xFFFFFFFF
    assert int(se.bucket_of(v, 7)) == (h * 7) >> 32
    x = (v * 0x27D4EB2F) & 0xFFFFFFFF
    x ^= x >> 13
    assert int(se.pass_of(v, 3)) == ((((x * 0x165667B1) & 0xFFFFFFFF) * 3) >> 32)
    y = (v * 0x85EBCA6B) & 0xFFFFFFFF
    y ^= y >> 15
    y = (y * 0xC2B2AE35) & 0xFFFFFFFF
    assert int(se.slot_of(v)) == y >> 20
    ids = np.arange(1 << 16)
    assert se.bucket_of(ids, 5).max() == 4 and se.slot_of(ids).max() < se.HCAP and se.pass_of(ids, 4).max() == 3
    # the ids test_gpu_stress.py aims at bucket 0 of any bucket count: v * inverse has a hashed value < 2^24
    inv = pow(0x9E3779B1, -1, 1 << 32)
    t = (np.arange(1000, dtype=np.uint64) * np.uint64(inv)) & np.uint64(0xFFFFFFFF)
    assert (se.bucket_of(t, 256) == 0).all()


def test_constants_shared_with_the_binding():
    """T_SORTED_MAX decides which lists the tlist case calls sorted: it must be the binding's (no library is loaded)"""
    from cslicer import _abi
    assert se.T_SORTED_MAX == _abi.T_SORTED_MAX
    assert _abi.ERR_BITS[se.ERR_BUCKET_FULL] == "BUCKET_FULL"


def test_geometry():
    g = se.geometry(512, 15)
    assert (g["W"], g["C"], g["nb"], g["tiles"]) == (16, 8192, 4, 2)
    assert se.geometry(1, 3)["nb"] == 1 and se.geometry(129, 15)["nb"] == 2
    assert [se.npass_of(c) for c in (4096, 4097, 6144, 6145)] == [1, 3, 3, 4]
    assert se.geometry(1025, 5)["degree_blocks"] == 2 and se.geometry(4097, 5)["count_blocks"] == 2
    assert se.geometry(257, 7)["steps"] == [8, 1]
