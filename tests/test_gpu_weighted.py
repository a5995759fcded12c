"""Edge-weighted neighbour sampling on the GPU (csl_set_edge_cdf): the engine against the sequential restatement
(tests/weighted_ref.py), bit for bit -- graph lists, frontiers, draw counts and the raw candidate stream -- at the
kernel's dispatch edges and over the shapes a table can take, then the property the feature exists for, the refusals,
the recovery replay and the trainer surface."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library, as in every trainer test: one HIP runtime per process, torch's)

from golden_util import load_case
from noreplace_ref import GKEYS, crafted_graph
from weighted_ref import WeightedGraphRef

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from cslicer import _abi
    _abi.load()
    return _abi


def engine_sample(abi, e, stream, slot=0):
    """graph_dict plus what the restatement also records: per-layer draws and the raw neighbour_sample stream"""
    m = e.meta(stream, slot)       # (first: the call that recovers from a frontier overflow)
    d = e.graph_dict(stream, slot)
    d["draws"] = [int(m.layer[l].draws) for l in range(e.n_layers)]
    if e.flags & abi.FLAG_KEEP_CANDIDATES:
        d["nbr_flat"], d["nbr_counts"] = [], []
        for l in range(e.n_layers):
            flat, counts = e.copy_candidates(l, stream, slot, m)
            d["nbr_flat"].append(flat)
            d["nbr_counts"].append(counts)
    return d


def assert_same(got, want, what="", stream=True):
    assert len(got["layers"]) == len(want["layers"])
    for l, (gl, wl) in enumerate(zip(got["layers"], want["layers"])):
        assert len(gl) == len(wl)
        for p, (gb, wb) in enumerate(zip(gl, wl)):
            tag = "%s layer %d part %d " % (what, l, p)
            for k in GKEYS:
                np.testing.assert_array_equal(gb[k], wb[k], err_msg=tag + k)
            for j in range(len(wl)):
                np.testing.assert_array_equal(gb["from_ids"][j], wb["from_ids"][j], err_msg=tag + "from_ids[%d]" % j)
                np.testing.assert_array_equal(gb["to_ids"][j], wb["to_ids"][j], err_msg=tag + "to_ids[%d]" % j)
    assert len(got["frontier"]) == len(want["frontier"])
    for l, (a, b) in enumerate(zip(got["frontier"], want["frontier"])):
        np.testing.assert_array_equal(a, b, err_msg="%s frontier[%d]" % (what, l))
    assert got["draws"] == want["draws"], what
    assert got["draws_total"] == want["draws_total"], what
    assert got["sampled_edges"] == want["sampled_edges"], what
    if stream:
        for l in range(len(want["layers"])):
            np.testing.assert_array_equal(got["nbr_counts"][l], want["nbr_counts"][l], err_msg="%s nbr_counts[%d]" % (what, l))
            np.testing.assert_array_equal(got["nbr_flat"][l], want["nbr_flat"][l], err_msg="%s nbr_flat[%d]" % (what, l))


def check_transposed(d):
    """t_indptr / t_indices of every layer but the deepest: the slice CSR + self lists by source (cslicer_hip.h,
    CSL_T_INDPTR): per in node ~r of its self entry, then the out rows of its edges ascending"""
    L = len(d["layers"])
    for l, parts in enumerate(d["layers"]):
        for g, bp in enumerate(parts):
            tag = "layer %d part %d " % (l, g)
            if l == L - 1:
                assert len(bp["t_indptr"]) == 0 and len(bp["t_indices"]) == 0, tag
                continue
            n_in = len(bp["in_nodes"])
            if len(bp["out_nodes"]) == 0 and n_in == 0 and len(bp["t_indptr"]) == 0:
                continue
            rows = np.repeat(np.arange(len(bp["out_nodes"]), dtype=np.int64), np.diff(bp["indptr"]))
            u = np.concatenate([bp["indices"].astype(np.int64), bp["self_ids_in"].astype(np.int64)])
            val = np.concatenate([rows, ~bp["self_ids_out"].astype(np.int64)])
            order = np.lexsort((val, u))
            want_ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n_in))])
            np.testing.assert_array_equal(bp["t_indptr"], want_ptr, err_msg=tag + "t_indptr")
            got_idx, lens = bp["t_indices"].copy(), np.diff(want_ptr)
            for k in np.flatnonzero(lens > 128):       # (longer than CSL_T_SORTED_MAX: unspecified order)
                got_idx[want_ptr[k]:want_ptr[k + 1]] = np.sort(got_idx[want_ptr[k]:want_ptr[k + 1]])
            np.testing.assert_array_equal(got_idx, val[order], err_msg=tag + "t_indices")
            assert bp["t_max_len"] == (int(lens.max()) if len(lens) else 0), tag


def int_cum(indptr, q):
    """the table of integer weights q (per row their running sum), uint32"""
    q = np.asarray(q, dtype=np.int64)
    c = np.cumsum(q)
    deg = np.diff(indptr)
    before = np.repeat(np.concatenate([[0], c])[indptr[:-1]], deg)
    out = c - before
    assert out.size == 0 or out.max() <= 2 ** 32 - 1
    return out.astype(np.uint32)


def seeded_weights(indptr, seed=9):
    """integer weights in [0, 9]: zeros and ties in most rows"""
    return int_cum(indptr, np.random.default_rng(seed).integers(0, 10, int(indptr[-1])))


def run_rounds(abi, indptr, indices, cum, P, fan, B, S, rounds=2, extra_flags=0, perm_seed=3, first=None):
    """`rounds` consecutive rounds of S minibatches, batch k of a round on stream k, against one restatement per stream"""
    n = indptr.shape[0] - 1
    perm = np.random.default_rng(perm_seed).permutation(n)
    if first is not None:        # a node the first minibatch must hold
        perm = np.concatenate([[first], perm[perm != first]])
    flags = abi.FLAG_KEEP_CANDIDATES | extra_flags
    e = abi.Engine(indptr, indices, n_parts=P, fanouts=fan, max_batch=B, n_streams=S, mode=abi.MODE_GRAPH, flags=flags)
    bytes0 = e.device_bytes()
    e.set_edge_cdf(cum)
    assert e.device_bytes() == bytes0 + 4 * max(len(cum), 1)
    e.set_nodes(perm)
    refs = [WeightedGraphRef(indptr, indices, P, fan, cum=cum) for _ in range(S)]
    out = []
    for r in range(rounds):
        e.submit_round(r * S, B, S)
        for s in range(S):
            seeds = perm[(r * S + s) * B:(r * S + s + 1) * B]
            assert len(seeds)
            got = engine_sample(abi, e, s)
            assert_same(got, refs[s].sample_graph(seeds), what="round %d stream %d" % (r, s))
            out.append(got)
    e.close()
    return out


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("case", ["toy40", "powerlaw2k", "selfloops_multiedges", "dense_small"])
def test_engine_equals_the_restatement(abi, case, P):
    indptr, indices, _ = load_case(case)
    n = indptr.shape[0] - 1
    S = 2
    B = max(1, min(64, n // (2 * S)))
    run_rounds(abi, indptr, indices, seeded_weights(indptr), P, (10, 5, 3), B, S)


@pytest.mark.parametrize("fan", [(1,), (5, 5), (200,)], ids=str)
def test_dispatch_edges(abi, fan):
    """rows of degree f-1, f, f+1, 2f and one of 5000; 300 seeds with the long row first: a 13-probe search shares a wave
    with 1- to 4-probe ones, in a frontier of more than one tile that is no multiple of it"""
    indptr, indices = crafted_graph(fan[0], n=320)
    assert set(np.diff(indptr).tolist()) == {fan[0] - 1, fan[0], fan[0] + 1, 2 * fan[0], 5000}
    cum = seeded_weights(indptr)
    out = run_rounds(abi, indptr, indices, cum, 4, fan, 300, 1, rounds=1, first=7)
    assert len(out[0]["frontier"][0]) == 300 and out[0]["frontier"][0][0] == 7
    # (and on two streams, each with its own generator, two rounds)
    run_rounds(abi, indptr, indices, cum, 1, fan, 80, 2, rounds=2, perm_seed=5, first=7)


def shape_graph(n=300, seed=2):
    """every row has 6..40 edges (>= the fanout 6 used below), uniform sources, a few self loops and parallel edges"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(6, 41, n)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return indptr, rng.integers(0, n, int(indptr[-1])).astype(np.int64)


def shape_tables(indptr):
    E, deg = int(indptr[-1]), np.diff(indptr)
    first = np.zeros(E, dtype=np.int64)
    first[indptr[:-1]] = 1
    last = np.zeros(E, dtype=np.int64)
    last[indptr[1:] - 1] = 1
    pos = np.arange(E) - np.repeat(indptr[:-1], deg)          # position inside the row
    d = np.repeat(deg, deg)
    holes = np.random.default_rng(4).integers(1, 6, E)
    holes[(pos == 0) | (pos == d - 1) | (pos == d // 2) | (pos == d // 2 + 1)] = 0
    huge = np.zeros(E, dtype=np.int64)                        # T = 2^32 - 1: the product's top word decides
    huge[indptr[:-1] + 1] = 2 ** 31
    huge[indptr[1:] - 2] += 2 ** 31 - 1
    return {
        "first edge": int_cum(indptr, first * 1000),
        "last edge": int_cum(indptr, last * 1000),
        "zeros first, middle, last": int_cum(indptr, holes),
        "T = 1": int_cum(indptr, (pos == d // 3).astype(np.int64)),
        "T = 2^32 - 1": int_cum(indptr, huge),
        "all ones": int_cum(indptr, np.ones(E, dtype=np.int64)),
    }


@pytest.mark.parametrize("name", ["first edge", "last edge", "zeros first, middle, last", "T = 1", "T = 2^32 - 1",
                                  "all ones"])
def test_table_shapes(abi, name):
    indptr, indices = shape_graph()
    cum = shape_tables(indptr)[name]
    if name == "T = 2^32 - 1":
        assert (cum[indptr[1:] - 1] == 2 ** 32 - 1).all()
    out = run_rounds(abi, indptr, indices, cum, 2, (6, 6), 100, 1, rounds=2)
    if name in ("first edge", "last edge"):
        at = indptr[:-1] if name == "first edge" else indptr[1:] - 1
        for d in out:          # every row's candidates are its one weighted edge, six times
            fr, flat = d["frontier"][0], d["nbr_flat"][0].reshape(-1, 7)
            np.testing.assert_array_equal(flat[:, 1:], np.repeat(indices[at[fr]][:, None], 6, axis=1))


def test_all_zero_rows_draw_as_an_unweighted_engine(abi):
    indptr, indices = shape_graph()
    zero = np.zeros(int(indptr[-1]), dtype=np.uint32)
    got = run_rounds(abi, indptr, indices, zero, 2, (6, 6), 100, 1, rounds=2)
    perm = np.random.default_rng(3).permutation(300)
    e = abi.Engine(indptr, indices, n_parts=2, fanouts=(6, 6), max_batch=100, n_streams=1, mode=abi.MODE_GRAPH,
                   flags=abi.FLAG_KEEP_CANDIDATES)
    e.set_nodes(perm)
    for r in range(2):
        e.submit_round(r, 100, 1)
        assert_same(got[r], engine_sample(abi, e, 0), what="round %d" % r)
    e.close()


def test_rowinfo64_table(abi, monkeypatch):
    indptr, indices, _ = load_case("powerlaw2k")
    n = indptr.shape[0] - 1
    kw = dict(n_parts=4, fanouts=(10, 5, 3), max_batch=64, n_streams=2, mode=abi.MODE_GRAPH)
    e = abi.Engine(indptr, indices, **kw)
    small = e.device_bytes()
    e.close()
    monkeypatch.setenv("CSLICER_ROWINFO64", "1")          # (read when the engine is created: the 8-byte row table)
    e = abi.Engine(indptr, indices, **kw)
    assert e.device_bytes() - small == 8 * n - 4 * (n + 1)
    e.close()
    run_rounds(abi, indptr, indices, seeded_weights(indptr), 4, (10, 5, 3), 64, 2)


def test_slices_by_source_follow_the_weighted_picks(abi):
    indptr, indices, _ = load_case("powerlaw2k")
    for d in run_rounds(abi, indptr, indices, seeded_weights(indptr), 4, (10, 5, 3), 64, 2, extra_flags=abi.FLAG_TRANSPOSE):
        check_transposed(d)


def ring_lattice(n=2000, k=5):
    v = np.arange(n)[:, None]
    nb = np.concatenate([(v + d) % n for d in range(1, k + 1)] + [(v - d) % n for d in range(1, k + 1)], axis=1)
    return np.arange(0, n * 2 * k + 1, 2 * k, dtype=np.int64), nb.reshape(-1).astype(np.int64)


def test_zero_weight_edges_are_never_sampled(abi):
    """weight 0 on the five forward neighbours of every node, 1 on the five backward ones: every edge source of every
    slice is a backward neighbour of its row's node; the same seeds without a table do sample forward ones"""
    n, k = 2000, 5
    indptr, indices = ring_lattice(n, k)
    cum = int_cum(indptr, np.tile(np.concatenate([np.zeros(k, dtype=np.int64), np.ones(k, dtype=np.int64)]), n))
    seeds = np.random.default_rng(0).permutation(n)[:256]
    forward = {}
    for weighted in (True, False):
        e = abi.Engine(indptr, indices, n_parts=2, fanouts=(6, 6), max_batch=256, mode=abi.MODE_GRAPH)
        if weighted:
            e.set_edge_cdf(cum)
        e.submit_seeds([seeds])
        d = e.graph_dict(0)
        e.close()
        forward[weighted] = edges = 0
        for parts in d["layers"]:
            for bp in parts:
                src = bp["in_nodes"][bp["indices"]]
                row = np.repeat(bp["out_nodes"], np.diff(bp["indptr"]))
                back = (row - src) % n          # 1..k for a backward neighbour, n-k..n-1 for a forward one
                edges += len(src)
                forward[weighted] += int((back > k).sum())
                assert ((back >= 1) & ((back <= k) | (back >= n - k))).all()
        assert edges > 256 * 6
    assert forward[True] == 0
    assert forward[False] > 0       # (the same seeds without a table: the check above can fail)


def test_refusals(abi):
    indptr, indices = shape_graph()
    E = int(indptr[-1])
    ones = int_cum(indptr, np.ones(E, dtype=np.int64))
    kw = dict(n_parts=2, fanouts=(6, 6), max_batch=100, n_streams=1)
    e = abi.Engine(indptr, indices, mode=abi.MODE_STRICT, **kw)
    with pytest.raises(abi.CslError, match="needs CSL_MODE_GRAPH without CSL_FLAG_NO_REPLACE") as ei:
        e.set_edge_cdf(ones)
    assert ei.value.code == -1 and e.edge_cdf is None
    e.close()
    e = abi.Engine(indptr, indices, mode=abi.MODE_GRAPH, flags=abi.FLAG_NO_REPLACE, **kw)
    with pytest.raises(abi.CslError, match="needs CSL_MODE_GRAPH without CSL_FLAG_NO_REPLACE") as ei:
        e.set_edge_cdf(ones)
    assert ei.value.code == -1
    e.close()
    with pytest.raises(ValueError, match="edges"):
        abi.Engine(indptr, indices, mode=abi.MODE_GRAPH, **kw).set_edge_cdf(ones[:-1])
    # one decreasing row
    bad = ones.copy()
    v = int(np.argmax(np.diff(indptr)))
    bad[indptr[v] + 3] = 0
    perm = np.random.default_rng(3).permutation(300)
    e = abi.Engine(indptr, indices, mode=abi.MODE_GRAPH, flags=abi.FLAG_KEEP_CANDIDATES, **kw)
    plain = abi.Engine(indptr, indices, mode=abi.MODE_GRAPH, flags=abi.FLAG_KEEP_CANDIDATES, **kw)
    bytes0 = e.device_bytes()
    with pytest.raises(abi.CslError, match="decreases inside a row") as ei:
        e.set_edge_cdf(bad)
    assert ei.value.code == -1 and e.edge_cdf is None and e.device_bytes() == bytes0
    for x in (e, plain):
        x.set_nodes(perm)
        x.submit_round(0, 100, 1)
    assert_same(engine_sample(abi, e, 0), engine_sample(abi, plain, 0), what="after a refused table")
    with pytest.raises(abi.CslError, match="before the first round") as ei:      # after a submitted round
        e.set_edge_cdf(ones)
    assert ei.value.code == -4
    e.close()
    plain.close()
    # a decrease far into a long row (the check strides a row 64 edges at a time), then the mended table is taken
    indptr, indices = crafted_graph(5, n=320)
    good = seeded_weights(indptr)
    bad = good.copy()
    assert indptr[8] - indptr[7] == 5000 and good[indptr[7] + 2999] > 0
    bad[indptr[7] + 3000] = good[indptr[7] + 2999] - 1
    e = abi.Engine(indptr, indices, mode=abi.MODE_GRAPH, **kw)
    with pytest.raises(abi.CslError, match="decreases inside a row"):
        e.set_edge_cdf(bad)
    e.set_edge_cdf(good)
    assert e.edge_cdf is good or np.array_equal(e.edge_cdf, good)
    e.close()


def test_recovered_engine_replays_with_the_table(abi):
    from cslicer import l0
    n, B, fan = 20000, 64, (10, 10, 10)
    indptr, indices = l0.synth_graph(n, 20.0, seed=4)
    cum = l0.edge_cdf(indptr, l0.inv_degree_weights(indptr, indices))
    perm = np.random.default_rng(0).permutation(n)
    kw = dict(n_parts=4, fanouts=fan, max_batch=B, n_streams=2, n_slots=2, mode=abi.MODE_GRAPH)
    room = abi.Engine(indptr, indices, **kw)
    small = abi.Engine(indptr, indices, frontier_cap=[B, 2000, 2000, 2000], **kw)
    plain = abi.Engine(indptr, indices, **kw)
    for e in (room, small):
        e.set_edge_cdf(cum)
    for e in (room, small, plain):
        e.set_nodes(perm)
    differs = False
    for r in range(3):
        for e in (room, small, plain):
            e.submit_round(2 * r, B, 2, slot=r % 2)
        for s in range(2):
            want = engine_sample(abi, room, s, r % 2)
            assert_same(engine_sample(abi, small, s, r % 2), want, what="round %d stream %d" % (r, s), stream=False)
            other = plain.graph_dict(s, r % 2)
            differs |= not np.array_equal(other["frontier"][1], want["frontier"][1])
    assert small.recovered == 1 and room.recovered == 0
    assert small.edge_cdf is not None
    assert differs            # the replay kept the table: without it the samples are other samples
    for e in (room, small, plain):
        e.close()


def _task(n=4000, F0=24, classes=5, seed=3):
    from cslicer import l0
    indptr, indices = l0.synth_graph(n, 14.0, seed=seed)
    rng = np.random.default_rng(seed)
    feats = rng.random((n, F0), dtype=np.float32)
    labels = np.argmax(feats[:, :classes], axis=1).astype(np.int64)
    return indptr, indices, feats, labels, rng.permutation(n)


@pytest.mark.parametrize("kind", ["sage", "gat"])
def test_trainer_with_edge_weights(abi, kind):
    from cslicer import l0
    from cslicer.train import Trainer
    indptr, indices, feats, labels, perm = _task()
    w = l0.inv_degree_weights(indptr, indices)
    kw = dict(fanouts=(10, 5), batch=256, streams=2, hidden=32 if kind == "sage" else 16, lr=1e-2, model=kind, heads=4)
    t = Trainer(indptr, indices, feats, labels, 5, edge_weight=w, **kw)
    assert t.edge_weighted and t.replace is True
    np.testing.assert_array_equal(t.eng.edge_cdf, l0.edge_cdf(indptr, w))
    if kind == "sage":
        assert t.native is not None
    t.set_nodes(perm)
    losses = t.run(8)
    assert len(losses) == 8 and all(np.isfinite(losses))
    ev = t.evaluate(perm[:500])
    assert ev["n"] == 500 and np.isfinite(ev["loss"]) and 0.0 <= ev["accuracy"] <= 1.0
    flags_w, path_w = t.eng.flags, t.plan.path
    t.close()
    t = Trainer(indptr, indices, feats, labels, 5, **kw)          # edge_weight=None: the engine the trainer has always made
    assert not t.edge_weighted and t.eng.edge_cdf is None
    want = abi.FLAG_TRANSPOSE if (kind == "sage" or t.gat_input) else abi.FLAG_TRANSPOSE | abi.FLAG_TRANSPOSE_ALL
    assert t.eng.flags == want == flags_w and t.plan.path == path_w
    t.close()


@pytest.mark.parametrize("how", ["inv-degree", "l0"])
def test_train_cli_edge_weight(abi, how, capsys, tmp_path, monkeypatch):
    from cslicer import l0, train
    n = 4000
    indptr, indices = l0.synth_graph(n, 9.0, seed=4)
    feats = np.random.default_rng(0).random((n, 12), dtype=np.float32)
    labels = np.argmax(feats[:, :3], axis=1).astype(np.int32)
    d = str(tmp_path / "l0")
    l0.write_l0(d, indptr, indices, features=feats, labels=labels, num_classes=3)
    w = l0.inv_degree_weights(indptr, indices)
    if how == "l0":
        w = np.random.default_rng(1).random(indices.shape[0]).astype(np.float32)
        l0.write_edge_weight(d, w)
    made, real = [], train.Trainer

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(train, "Trainer", Spy)
    train.main(["--graph", d, "--eval-split", "holdout", "--fan-out", "4,6", "--num-layers", "2", "--num-hidden", "16",
                "--batch-size", "300", "--num-epochs", "1", "--max-steps", "4", "--edge-weight", how])
    out = capsys.readouterr().out
    assert "Eval Acc" in out and "epoch 0: 4 minibatches" in out
    (tr,) = made
    assert tr.edge_weighted and tr.steps_done == 4
    np.testing.assert_array_equal(tr.eng.edge_cdf, l0.edge_cdf(indptr, w))
