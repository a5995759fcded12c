"""CSL_FLAG_NO_REPLACE without a GPU: the Python restatement of graph mode (tests/noreplace_ref.py) is pinned to the C
oracle with replacement, Floyd's map is checked for its properties and its uniformity, and the host refuses what the
flag does not cover before any HIP call."""
import itertools
import math

import numpy as np
import pytest

from golden_util import UNIQUE_SEED_CASES, load_case
from noreplace_ref import GKEYS, GraphRef, MT19937Words, crafted_graph, floyd_picks


def assert_same_graph(got, want, what=""):
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


def test_mt19937_words():
    g = MT19937Words(5489)
    assert [g.next() for _ in range(3)] == [3499211612, 581869302, 3890346734]
    for _ in range(9996):
        g.next()
    assert g.next() == 4123659995          # the 10000th output of std::mt19937() (C++ standard, [rand.predef])


@pytest.mark.parametrize("case", UNIQUE_SEED_CASES)
def test_restatement_equals_the_oracle_with_replacement(case):
    from oracle import oracle as orc
    indptr, indices, batches = load_case(case)
    fan = (10, 10, 10)
    o = orc.Oracle(indptr, indices, n_parts=4, fanouts=fan)
    r = GraphRef(indptr, indices, 4, fan, replace=True)
    for b, rec in enumerate(batches):          # consecutive minibatches: the generator position is handed over
        want = o.sample_graph(rec["seeds"])
        got = r.sample_graph(rec["seeds"])
        what = "%s batch %d" % (case, b)
        assert_same_graph(got, want, what)
        assert got["draws_total"] == want["draws_total"], what
        assert got["sampled_edges"] == want["sampled_edges"], what
        for l in range(3):
            assert got["draws"][l] == int(orc.lib().orc_layer_draws(o._h, l)), what
            np.testing.assert_array_equal(got["nbr_counts"][l], o._get(l, 0, orc.NBR_COUNTS), err_msg=what)
            np.testing.assert_array_equal(got["nbr_flat"][l], o._get(l, 0, orc.NBR_FLAT), err_msg=what)
            # ... and the reference's own record of the same minibatch
            np.testing.assert_array_equal(got["nbr_flat"][l], rec["nbr_flat"][l], err_msg=what)
            assert got["draws"][l] == rec["draws"][l], what


def test_floyd_properties():
    f = 5
    indptr, indices = crafted_graph(f)
    perm = np.random.default_rng(2).permutation(300)
    seeds = np.array([7] + [v for v in perm if v != 7][:63])        # (the 5000-edge row among them)
    a = GraphRef(indptr, indices, 4, (f, f), replace=True)
    b = GraphRef(indptr, indices, 4, (f, f), replace=False)
    da, db = a.sample_graph(seeds), b.sample_graph(seeds)
    deg = np.diff(indptr)
    seen_degs = set()
    for l in range(2):
        fr = db["frontier"][l]
        assert len(b.picks[l]) == int((deg[fr] >= f).sum())
        for i, d, picks in b.picks[l]:
            assert d == deg[fr[i]] and d >= f
            assert len(picks) == f and len(set(picks)) == f and all(0 <= p < d for p in picks)
            if d == f:
                assert sorted(picks) == list(range(f))       # a permutation of all its edges
            seen_degs.add(int(d))
    assert {f, f + 1, 2 * f, 5000} <= seen_degs
    # layer 0: same frontier, hence the same consumers, the same draws and the same short rows
    np.testing.assert_array_equal(da["frontier"][0], db["frontier"][0])
    assert da["draws"][0] == db["draws"][0] == f * int((deg[seeds] >= f).sum())
    np.testing.assert_array_equal(da["nbr_counts"][0], db["nbr_counts"][0])
    oa = np.concatenate([[0], np.cumsum(da["nbr_counts"][0])])
    for i, v in enumerate(seeds):
        if deg[v] < f:
            np.testing.assert_array_equal(da["nbr_flat"][0][oa[i]:oa[i + 1]], db["nbr_flat"][0][oa[i]:oa[i + 1]])
            np.testing.assert_array_equal(db["nbr_flat"][0][oa[i] + 1:oa[i + 1]], indices[indptr[v]:indptr[v + 1]])
    assert not np.array_equal(da["nbr_flat"][0], db["nbr_flat"][0])
    # every call consumes fanout words per consumer, whatever the map
    assert db["draws_total"] == sum(db["draws"])


@pytest.mark.parametrize("deg,f", [(5, 3), (7, 2)])
def test_floyd_is_uniform_over_subsets(deg, f):
    """100 000 rows consuming words 0.. of mt19937(5489): every f-subset of the positions within 4.5 standard deviations
    of n * p (the input is fixed, so this is a condition, not a measurement: the worst cells are 2.7 and 2.8 sd off)."""
    n = 100_000
    g = MT19937Words(5489)
    count = {c: 0 for c in itertools.combinations(range(deg), f)}
    for _ in range(n):
        count[tuple(sorted(floyd_picks([g.next() for _ in range(f)], deg)))] += 1
    assert len(count) == math.comb(deg, f) and sum(count.values()) == n
    p = 1.0 / len(count)
    sd = math.sqrt(n * p * (1 - p))
    worst = max(abs(c - n * p) for c in count.values()) / sd
    print("deg %d fanout %d: %d subsets, worst deviation %.2f sd" % (deg, f, len(count), worst))
    assert worst < 4.5


def test_host_refuses_what_the_flag_does_not_cover():
    from cslicer import _abi
    indptr = np.array([0, 1, 2], dtype=np.int64)
    indices = np.array([1, 0], dtype=np.int64)
    assert _abi.FLAG_NO_REPLACE == 16
    assert _abi.load().csl_noreplace_max_fanout() == 64 and _abi.noreplace_max_fanout() == 64
    with pytest.raises(_abi.CslError, match="CSL_FLAG_NO_REPLACE needs CSL_MODE_GRAPH") as ei:
        _abi.Engine(indptr, indices, mode=_abi.MODE_STRICT, flags=_abi.FLAG_NO_REPLACE)
    assert ei.value.code == -1
    with pytest.raises(_abi.CslError, match=r"fanout\[1\]=65.*at most 64") as ei:
        _abi.Engine(indptr, indices, fanouts=(64, 65), mode=_abi.MODE_GRAPH, flags=_abi.FLAG_NO_REPLACE)
    assert ei.value.code == -1


def test_cli_and_trainer_surface():
    import inspect
    from cslicer import train
    assert train._parser().parse_args(["--no-replace"]).no_replace is True
    assert train._parser().parse_args([]).no_replace is False
    assert inspect.signature(train.Trainer.__init__).parameters["replace"].default is True
    assert "--no-replace (extra)" in train.main.__doc__
    with pytest.raises(SystemExit, match="64"):
        train.main(["--no-replace", "--fan-out", "10,65"])
    with pytest.raises(ValueError, match="64"):      # (before any device call)
        train.Trainer(np.array([0, 1, 2]), np.array([1, 0]), None, None, 2, fanouts=(65,), replace=False)
