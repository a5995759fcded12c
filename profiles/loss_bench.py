"""What class weights and label smoothing cost the native GraphSAGE step on bench.py's products-like workload
(cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5; features 100, hidden 256, fanout 15/10/5, batch
1024, one GPU), and how k_softmax_ce_w stands beside k_softmax_ce and against the bytes it moves.

    python profiles/loss_bench.py [--reps 5] [--steps 64] [--out FILE]

* csl_softmax_ce_w_partial_f32 (weights and eps = 0.1 on, with the column sums) and, beside it, csl_softmax_ce_partial_f32
  per launch by device events, 20 back-to-back launches per event pair, at [1024 x 47] (the step's top layer), [1024 x 256]
  and [65,536 x 47], against the bytes each moves (logits read, gradient written, the label, the node id, the partials; the
  weights once): GB/s and elements/s, and which bound applies;
* the native step's rate with the options off and on: two trainers in ONE process (and a third, options off again, as a
  control for the position in the rotation), alternating, `--steps` steps per timed run (wall clock around Trainer.run
  ending in a device synchronise, every run slicing one round ahead as bench.py's end-to-end leg does), median (min, max).
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "occ-gnn_amd"))

from cslicer import aggr, l0  # noqa: E402
from cslicer.train import Trainer, balanced_class_weight, synthetic_node_data, use_tuned_gemms  # noqa: E402

CALLS = 20
HBM_GBS = 8000.0      # MI355X peak HBM bandwidth (GB/s)


def kernels(lines, reps):
    L = aggr._lib()
    lines += ["", "the loss pass with its column sums, %d launches per event pair, median (min, max) of %d:" % (CALLS, reps)]
    for m, Cn in ((1024, 47), (1024, 256), (65536, 47)):
        z = torch.randn((m, Cn), device="cuda") * 3
        ids = torch.arange(m, dtype=torch.int32, device="cuda")
        lab = torch.randint(0, Cn, (m,), dtype=torch.int64, device="cuda")
        w = torch.rand(Cn, device="cuda") * 3 + 0.1
        grad = torch.empty((m, Cn), device="cuda")
        blocks = (m + 3) // 4
        lpart, cpart = torch.empty(blocks, device="cuda"), torch.empty((blocks, Cn), device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
        calls = {
            "k_softmax_ce_w": lambda: L.csl_softmax_ce_w_partial_f32(p(z), Cn, m, m, Cn, p(ids), None, p(lab), p(w), 0.1, 1.0 / m,
                                                                     p(grad), Cn, p(lpart), p(cpart), aggr._stream()),
            "k_softmax_ce": lambda: L.csl_softmax_ce_partial_f32(p(z), Cn, m, m, Cn, p(ids), None, p(lab), 1.0 / m, p(grad), Cn,
                                                                 p(lpart), p(cpart), aggr._stream()),
        }
        for name, call in calls.items():
            for _ in range(3):
                assert call() == 0
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _c in range(CALLS):
                    call()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3 / CALLS)
            byt = 2.0 * m * Cn * 4 + m * 4 + m * 8 + blocks * (Cn + 1) * 4 + (Cn * 4 if name == "k_softmax_ce_w" else 0)
            med = np.median(ts)
            floor = byt / (HBM_GBS * 1e9)
            lines.append("  %-15s [%6d x %3d] (%6.2f MB moved): %7.1f us (%.1f, %.1f) = %5.0f GB/s, %5.1f G elements/s; "
                         "the HBM floor is %.2f us: %s"
                         % (name, m, Cn, byt / 1e6, med * 1e6, min(ts) * 1e6, max(ts) * 1e6, byt / med / 1e9, m * Cn / med / 1e9,
                            floor * 1e6, "launch- and latency-bound" if med > 10 * floor else "%.0f %% of the HBM bound" % (100 * floor / med)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, F, Cn = l0.PRESETS["products-like"]
    hidden, fan, B, S = 256, (15, 10, 5), 1024, 8
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    use_tuned_gemms()
    feats = lambda own: synthetic_node_data(n, F, Cn, seed=0, rows=own)[0]    # noqa: E731
    labels = lambda own: synthetic_node_data(n, 1, Cn, seed=0, rows=own)[1]   # noqa: E731
    perm = np.random.default_rng(1).permutation(n).astype(np.int64)
    lines = ["products-like: N %d, E %d, features %d, hidden %d, %d classes, fanout 15/10/5, batch %d, %d streams (graph %.1f s)"
             % (n, indices.shape[0], F, hidden, Cn, B, S, time.time() - t0)]
    kernels(lines, a.reps)
    on = dict(class_weight=balanced_class_weight(labels(np.arange(n)), Cn), label_smoothing=0.1)
    # (the third trainer is the first one again: what the position in the rotation alone does to a rate)
    kinds = ("options off", "weights + eps 0.1", "options off again")
    trs = [Trainer(indptr, indices, feats, labels, Cn, fanouts=fan, batch=B, streams=S, hidden=hidden, feat_dim=F, **kw)
           for kw in ({}, on, {})]
    at = []
    for tr in trs:
        assert tr.plan.path == "native"
        tr.set_nodes(perm)
        tr.run(48, then=(48, a.steps))
        at.append(48)
    assert trs[0].loss_spec is None and trs[1].loss_spec is not None
    rates = [[] for _ in kinds]
    for _ in range(a.reps):
        for k, tr in enumerate(trs):
            nxt = (at[k] + a.steps) % tr.n_batches
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.run(a.steps, first_batch=at[k], then=(nxt, a.steps))
            torch.cuda.synchronize()
            rates[k].append(a.steps / (time.perf_counter() - t))
            at[k] = nxt
    lines += ["", "native step, %d steps per run, median (min, max) of %d runs, the trainers alternating:" % (a.steps, a.reps)]
    for kind, r in zip(kinds, rates):
        lines.append("  %-18s  %8.0f minibatches/s (%.0f, %.0f)" % (kind, np.median(r), min(r), max(r)))
    lines.append("  ratio of the medians (on / off): %.3f; (off again / off): %.3f"
                 % (np.median(rates[1]) / np.median(rates[0]), np.median(rates[2]) / np.median(rates[0])))
    for tr in trs:
        tr.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
