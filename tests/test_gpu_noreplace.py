"""CSL_FLAG_NO_REPLACE on the GPU: the engine against the sequential restatement (tests/noreplace_ref.py, pinned to the
C oracle by tests/test_noreplace_cpu.py), bit for bit -- graph lists, frontiers, draw counts and the raw candidate
stream -- then the properties the flag exists for, the recovery replay and the trainer surface."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library, as in every trainer test: one HIP runtime per process, torch's)

from golden_util import load_case
from noreplace_ref import GKEYS, GraphRef, crafted_graph

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


def run_rounds(abi, indptr, indices, P, fan, B, S, rounds=2, extra_flags=0, perm_seed=3, first=None):
    """`rounds` consecutive rounds of S minibatches, batch k of a round on stream k, against one GraphRef per stream"""
    n = indptr.shape[0] - 1
    perm = np.random.default_rng(perm_seed).permutation(n)
    if first is not None:        # a node the first minibatch must hold
        perm = np.concatenate([[first], perm[perm != first]])
    flags = abi.FLAG_NO_REPLACE | abi.FLAG_KEEP_CANDIDATES | extra_flags
    e = abi.Engine(indptr, indices, n_parts=P, fanouts=fan, max_batch=B, n_streams=S, mode=abi.MODE_GRAPH, flags=flags)
    e.set_nodes(perm)
    refs = [GraphRef(indptr, indices, P, fan, replace=False) for _ in range(S)]
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
    run_rounds(abi, indptr, indices, P, (10, 5, 3), B, S)


def test_slices_by_source_follow_the_distinct_picks(abi):
    indptr, indices, _ = load_case("powerlaw2k")
    for d in run_rounds(abi, indptr, indices, 4, (10, 5, 3), 64, 2, extra_flags=abi.FLAG_TRANSPOSE):
        check_transposed(d)


@pytest.mark.parametrize("fan", [(1,), (5, 5), (64,)], ids=str)
def test_dispatch_edges(abi, fan):
    """rows of degree f-1, f, f+1, 2f and one of 5000; 300 seeds: a frontier of more than one tile, not a multiple of it"""
    indptr, indices = crafted_graph(fan[0], n=320)
    assert set(np.diff(indptr).tolist()) == {fan[0] - 1, fan[0], fan[0] + 1, 2 * fan[0], 5000}
    out = run_rounds(abi, indptr, indices, 4, fan, 300, 1, rounds=1, first=7)
    assert len(out[0]["frontier"][0]) == 300 and out[0]["frontier"][0][0] == 7
    # (and on two streams, each with its own generator, two rounds)
    run_rounds(abi, indptr, indices, 1, fan, 80, 2, rounds=2, perm_seed=5, first=7)


def ring_lattice(n=2000, k=5):
    v = np.arange(n)[:, None]
    nb = np.concatenate([(v + d) % n for d in range(1, k + 1)] + [(v - d) % n for d in range(1, k + 1)], axis=1)
    return np.arange(0, n * 2 * k + 1, 2 * k, dtype=np.int64), nb.reshape(-1).astype(np.int64)


def test_rows_have_distinct_sources(abi):
    indptr, indices = ring_lattice()
    seeds = np.random.default_rng(0).permutation(2000)[:256]
    repeated = {}
    for flags in (abi.FLAG_NO_REPLACE, 0):
        e = abi.Engine(indptr, indices, n_parts=2, fanouts=(6, 6), max_batch=256, mode=abi.MODE_GRAPH, flags=flags)
        e.submit_seeds([seeds])
        d = e.graph_dict(0)
        e.close()
        repeated[flags] = rows = 0
        for parts in d["layers"]:
            for bp in parts:
                src = bp["in_nodes"][bp["indices"]]
                for a, b in zip(bp["indptr"][:-1], bp["indptr"][1:]):
                    rows += 1
                    repeated[flags] += len(set(src[a:b].tolist())) != b - a
        assert rows > 256
        # every owned row has min(deg, fanout) = 6 edges over the two slices
        assert all((bp["owned_degree"] == 6).all() for parts in d["layers"] for bp in parts)
    assert repeated[abi.FLAG_NO_REPLACE] == 0
    assert repeated[0] > 0       # (the same seeds with replacement: the check above can fail)


def test_recovered_engine_replays_with_the_flag(abi):
    from cslicer import l0
    n, B, fan = 20000, 64, (10, 10, 10)
    indptr, indices = l0.synth_graph(n, 20.0, seed=4)
    perm = np.random.default_rng(0).permutation(n)
    kw = dict(n_parts=4, fanouts=fan, max_batch=B, n_streams=2, n_slots=2, mode=abi.MODE_GRAPH,
              flags=abi.FLAG_NO_REPLACE)
    room = abi.Engine(indptr, indices, **kw)
    small = abi.Engine(indptr, indices, frontier_cap=[B, 2000, 2000, 2000], **kw)
    plain = abi.Engine(indptr, indices, **dict(kw, flags=0))
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
    assert small.flags & abi.FLAG_NO_REPLACE
    assert differs            # the replay kept the flag: without it the samples are other samples
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
def test_trainer_without_replacement(abi, kind):
    from cslicer.train import Trainer
    indptr, indices, feats, labels, perm = _task()
    kw = dict(fanouts=(10, 5), batch=256, streams=2, hidden=32 if kind == "sage" else 16, lr=1e-2, model=kind, heads=4)
    t = Trainer(indptr, indices, feats, labels, 5, replace=False, **kw)
    assert t.replace is False and t.eng.flags & abi.FLAG_NO_REPLACE
    if kind == "sage":
        assert t.native is not None
    t.set_nodes(perm)
    losses = t.run(8)
    assert len(losses) == 8 and all(np.isfinite(losses))
    ev = t.evaluate(perm[:500])
    assert ev["n"] == 500 and np.isfinite(ev["loss"]) and 0.0 <= ev["accuracy"] <= 1.0
    flags_nr = t.eng.flags
    t.close()
    t = Trainer(indptr, indices, feats, labels, 5, **kw)          # replace=True: the flags the trainer has always set
    assert t.replace is True and t.eng.flags == flags_nr & ~abi.FLAG_NO_REPLACE
    want = abi.FLAG_TRANSPOSE if (kind == "sage" or t.gat_input) else abi.FLAG_TRANSPOSE | abi.FLAG_TRANSPOSE_ALL
    assert t.eng.flags == want
    t.close()


def test_train_cli_no_replace(abi, capsys, tmp_path, monkeypatch):
    from cslicer import l0, train
    n = 4000
    indptr, indices = l0.synth_graph(n, 9.0, seed=4)
    feats = np.random.default_rng(0).random((n, 12), dtype=np.float32)
    labels = np.argmax(feats[:, :3], axis=1).astype(np.int32)
    d = str(tmp_path / "l0")
    l0.write_l0(d, indptr, indices, features=feats, labels=labels, num_classes=3)
    made, real = [], train.Trainer

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(train, "Trainer", Spy)
    train.main(["--graph", d, "--eval-split", "holdout", "--fan-out", "4,6", "--num-layers", "2", "--num-hidden", "16",
                "--batch-size", "300", "--num-epochs", "1", "--max-steps", "4", "--no-replace"])
    out = capsys.readouterr().out
    assert "Eval Acc" in out and "epoch 0: 4 minibatches" in out
    (tr,) = made
    assert tr.replace is False and tr.eng.flags & abi.FLAG_NO_REPLACE and tr.steps_done == 4
