"""The single-GPU native training step (csl_sage_fwd_bwd_f32, csrc/sage_step.hip) at SMALL widths, against tests/sage_ref.py
(float64) on the oracle's traversal -- next to tests/test_gpu_step_bench_widths.py, which pins the bench's widths only.

Varied here, because the sequencer branches on it: the row padding (pad_rows: none; up to a multiple of row_pad; up to
a multiple of 256 for a layer shorter than row_pad), weight-gradient slabs that do and do not divide the padded rows, a
layer whose slice by source has hub lists, more than 256 classes (the loss pass then leaves no bias column sums: a
separate pass), one, two and four layers, the deepest layer fused and not.

Tolerances (north_star): loss 1e-5 relative, every parameter gradient within 1e-4 of its largest entry.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _graph(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "hub":                        # every row points at three hubs: their lists by source are B x fanout long
        deg = 10
        nb = rng.integers(0, n, size=(n, deg))
        nb[:, :3] = np.array([5, 9, 17])
        nb[[5, 9, 17]] = rng.integers(100, n, size=(3, deg))
        return np.arange(n + 1, dtype=np.int64) * deg, np.sort(nb, axis=1).reshape(-1).astype(np.int64)
    d = rng.integers(0, 17, size=n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(d, out=indptr[1:])
    return indptr, rng.integers(0, n, size=int(indptr[-1])).astype(np.int64)


# (L, fan, classes, row_pad, n_slabs, graph, fused); tests/test_gpu_sage_rank.py runs the rows of at most 256 classes too
CASES = [
    (2, (6, 4), 7, 0, 4, "random", True),          # no padding at all
    (2, (6, 4), 7, 64, 4, "random", True),         # rows up to a multiple of 64; 4 slabs divide them
    (2, (6, 4), 7, 64, 3, "random", False),        # ... 3 slabs do not divide every layer's rows
    (2, (6, 4), 7, 512, 8, "random", True),        # the top layer (200 rows) is shorter than row_pad: multiples of 256
    (3, (5, 4, 3), 5, 512, 32, "random", False),
    (1, (8,), 7, 64, 4, "random", True),           # one layer: the fused forward, the loss, one weight gradient
    (1, (8,), 300, 64, 4, "random", False),
    (4, (4, 3, 3, 2), 9, 64, 2, "random", True),   # CSL_MAX_LAYERS
    (2, (8, 6), 7, 64, 4, "hub", True),            # hub lists by source in the upper layer
    (3, (6, 4, 3), 300, 64, 4, "random", True),    # more than 256 classes
    (2, (8, 6), 300, 0, 1, "hub", False),
]


@pytest.mark.parametrize("L,fan,classes,row_pad,n_slabs,graph,fused", CASES)
def test_native_step_at_small_widths_matches_float64_on_the_oracle_traversal(L, fan, classes, row_pad, n_slabs, graph,
                                                                               fused, monkeypatch):
    import sage_ref
    from cslicer import _abi, aggr, splitgnn
    from oracle import oracle as orc
    _abi.load()
    if not fused:
        monkeypatch.setenv("CSLICER_NO_MFMA_FWD", "1")
    n, F0, hidden, B = 20000, 12, 24, 200
    indptr, indices = _graph(graph, n)
    rng = np.random.default_rng(7)
    feats = rng.standard_normal((n, F0)).astype(np.float32)
    labels = rng.integers(0, classes, size=n).astype(np.int64)
    seeds = rng.permutation(n)[:B]
    torch.manual_seed(L)
    model = splitgnn.DistSAGEModel(F0, hidden, classes, n_layers=L).cuda()
    with torch.no_grad():
        for c in model.convs:
            c.fc.bias.normal_(0, 0.3)
    ws, bs = [c.fc.weight for c in model.convs], [c.fc.bias for c in model.convs]
    eng = _abi.Engine(indptr, indices, n_parts=1, fanouts=fan, max_batch=B, mode=_abi.MODE_GRAPH, flags=_abi.FLAG_TRANSPOSE)
    try:
        eng.submit_seeds([seeds])
        slices = splitgnn.slices_of(eng)
        order = [slices[L - 1 - k][0] for k in range(L)]
        if graph == "hub" and L > 1:
            assert max(s.t_max_len for s in order[1:]) > _abi.T_SORTED_MAX
        step = aggr.SageStep(model, row_pad, n_slabs)
        got_loss = torch.zeros(1, device="cuda")
        x, lab = torch.from_numpy(feats).cuda(), torch.from_numpy(labels).cuda()
        for _ in range(2):   # (the second call runs on the recorded GEMM plans and the reused workspace)
            step(order, x, lab, 1.0 / B, got_loss)
        torch.cuda.synchronize()
        got = step.grads.double().cpu()
        trav = orc.Oracle(indptr, indices, n_parts=1, fanouts=fan).sample(seeds)
        assert int(slices[0][0].n_out) == B
        for l in range(L):   # the same sample: sizes of every frontier
            assert int(slices[l][0].n_out) == len(trav["frontier"][l]) and int(slices[l][0].n_in) == len(trav["frontier"][l + 1])
        want_loss, want = sage_ref.model_on_traversal(trav, feats, labels, ws, bs, n)
    finally:
        eng.close()
    print("loss %.9g (float64 %.9g)" % (float(got_loss[0]), want_loss))
    assert abs(float(got_loss[0]) - want_loss) <= 1e-5 * abs(want_loss), (float(got_loss[0]), want_loss)
    at = 0
    for k, g in enumerate(want):
        seg = got[at:at + g.numel()].reshape(g.shape)
        at += g.numel()
        err, ref = float((seg - g).abs().max()), float(g.abs().max())
        print("gradient %d: max error %.3g, largest entry %.3g" % (k, err, ref))
        assert err <= 1e-4 * ref, "gradient %d (%s of layer %d): max error %.3g against a largest entry of %.3g" % (
            k, "weight" if k % 2 == 0 else "bias", k // 2, err, ref)
    assert at == got.numel()
