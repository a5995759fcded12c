"""Edge-weighted sampling without a GPU: the restatement (tests/weighted_ref.py) falls through to the pinned one without
a table, l0.edge_cdf keeps the properties its formula promises, the map from words to edge positions follows the
weights, and the trainer and the command line refuse what the option does not cover before any device call."""
import math

import numpy as np
import pytest

from golden_util import load_case
from noreplace_ref import GraphRef, MT19937Words
from weighted_ref import WeightedGraphRef, weighted_pick

ROWS = [[0, 1, 2, 3, 0, 4, 6], [1e-12, 1, 1, 1], [5] * 11, [0, 0, 7, 0], [1, 1e6, 1]]


def same(a, b):
    """two structures of lists / dicts / arrays, equal leaf for leaf"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("case", ["toy40", "powerlaw2k"])
def test_no_table_is_the_pinned_restatement(case):
    indptr, indices, batches = load_case(case)
    fan = (10, 5, 3)
    a = GraphRef(indptr, indices, 4, fan, replace=True)
    b = WeightedGraphRef(indptr, indices, 4, fan, cum=None)
    for rec in batches[:3]:
        assert same(b.sample_graph(rec["seeds"]), a.sample_graph(rec["seeds"]))
    assert a.draws_total == b.draws_total > 0


def check_cdf(indptr, w):
    from cslicer import l0
    cum = l0.edge_cdf(indptr, w)
    assert cum.dtype == np.uint32 and cum.shape == (len(w),)
    for v in range(len(indptr) - 1):
        a, b = int(indptr[v]), int(indptr[v + 1])
        if a == b:
            continue
        c = cum[a:b].astype(np.int64)
        q = np.diff(np.concatenate([[0], c]))
        wr = np.asarray(w[a:b], dtype=np.float64)
        deg, T, S = b - a, int(c[-1]), wr.sum()
        assert (q >= 0).all()                                     # non-decreasing inside the row
        np.testing.assert_array_equal(q == 0, wr == 0)
        assert T <= 2 ** 32 - 1
        if S == 0:
            assert T == 0
            continue
        assert T <= 2 ** 31 + deg
        assert np.abs(q / T - wr / S).max() <= (deg + 1) / (2 ** 31 - deg)
    return cum


def test_edge_cdf_properties():
    from cslicer import l0
    rng = np.random.default_rng(11)
    deg = np.concatenate([rng.integers(0, 40, 200), [0, 1, 3000, 0]])
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    w = rng.random(int(indptr[-1])) * 10.0 ** rng.integers(-6, 6, int(indptr[-1]))
    w[rng.random(w.shape[0]) < 0.3] = 0.0
    w[indptr[5]:indptr[6]] = 0.0                                  # an all-zero row
    check_cdf(indptr, w)
    check_cdf(indptr, w.astype(np.float32))
    rows_ptr = np.concatenate([[0], np.cumsum([len(r) for r in ROWS])]).astype(np.int64)
    cum = check_cdf(rows_ptr, np.concatenate(ROWS))
    assert cum[rows_ptr[2]:rows_ptr[3]].tolist() == [(2 ** 31 // 11) * (i + 1) for i in range(11)]
    assert l0.edge_cdf(np.array([0, 0, 0]), np.zeros(0)).shape == (0,)
    good = np.ones(int(indptr[-1]))
    for bad in (-1.0, float("nan"), float("inf")):
        x = good.copy()
        x[7] = bad
        with pytest.raises(ValueError):
            l0.edge_cdf(indptr, x)
    with pytest.raises(ValueError):
        l0.edge_cdf(indptr, good[:-1])


def test_inv_degree_and_the_weight_file(tmp_path):
    from cslicer import l0
    indptr, indices = l0.synth_graph(300, 6.0, seed=1)
    w = l0.inv_degree_weights(indptr, indices)
    deg = np.diff(indptr)
    assert w.dtype == np.float32 and w.shape == indices.shape
    np.testing.assert_allclose(w, 1.0 / np.maximum(deg[indices], 1), rtol=1e-7)
    d = str(tmp_path / "g")
    meta = l0.write_l0(d, indptr, indices)
    before = open(d + "/meta.txt").read()
    with pytest.raises(ValueError):
        l0.read_edge_weight(d)
    l0.write_edge_weight(d, w)
    assert open(d + "/meta.txt").read() == before and l0.read_meta(d)["num_edges"] == meta["num_edges"]
    got = l0.read_edge_weight(d)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, w)
    with pytest.raises(ValueError):
        l0.write_edge_weight(d, w[:-1])


def test_the_map_follows_the_weights():
    """the first 700 000 words of mt19937(5489) on each single row: no zero-weight cell is ever hit, and every cell is
    within 4 standard deviations of n q_i / T (fixed input: a condition, not a measurement)"""
    from cslicer import l0
    n = 700_000
    g = MT19937Words(5489)
    words = [g.next() for _ in range(n)]
    for row in ROWS:
        cum = [int(c) for c in l0.edge_cdf(np.array([0, len(row)]), np.array(row, dtype=np.float64))]
        q = np.diff([0] + cum)
        T = cum[-1]
        count = np.bincount([weighted_pick(w, cum) for w in words], minlength=len(row))
        assert count.sum() == n and len(count) == len(row)
        assert (count[q == 0] == 0).all()
        p = q[q > 0] / T
        dev = np.abs(count[q > 0] - n * p) / np.sqrt(np.maximum(n * p * (1 - p), 1e-300))
        hit = p < 1
        worst = float(dev[hit].max()) if hit.any() else 0.0
        print("row %r: worst cell %.2f sd" % (row, worst))
        assert worst < 4.0
        assert (count[q > 0][~hit] == n).all()
    # T == 0: the parent's draw
    assert [weighted_pick(w, [0, 0, 0]) for w in words[:50]] == [w % 3 for w in words[:50]]


def test_trainer_refuses_before_any_device_call():
    from cslicer import train
    indptr, indices = np.array([0, 1, 2]), np.array([1, 0])
    with pytest.raises(ValueError, match="replace=False"):
        train.Trainer(indptr, indices, None, None, 2, fanouts=(2,), replace=False, edge_weight=np.ones(2))
    with pytest.raises(ValueError, match="2 edges"):
        train.Trainer(indptr, indices, None, None, 2, fanouts=(2,), edge_weight=np.ones(3))
    with pytest.raises(ValueError, match=">= 0"):
        train.Trainer(indptr, indices, None, None, 2, fanouts=(2,), edge_weight=np.array([1.0, -1.0]))
    with pytest.raises(ValueError, match="finite"):
        train.Trainer(indptr, indices, None, None, 2, fanouts=(2,), edge_weight=np.array([1.0, float("nan")]))


def test_cli_surface():
    import inspect
    from cslicer import _abi, train
    assert train._parser().parse_args(["--edge-weight", "inv-degree"]).edge_weight == "inv-degree"
    assert train._parser().parse_args([]).edge_weight is None
    assert inspect.signature(train.Trainer.__init__).parameters["edge_weight"].default is None
    assert "--edge-weight FILE|l0|inv-degree (extra)" in train.main.__doc__
    assert "--edge-weight inv-degree" in train.main.__doc__.split("--class-weight balanced --label-smoothing")[1]
    with pytest.raises(SystemExit, match="--no-replace"):
        train.main(["--edge-weight", "inv-degree", "--no-replace"])
    assert "csl_set_edge_cdf" in _abi.SYMBOLS and hasattr(_abi.Engine, "set_edge_cdf")
