"""What dropout between the layers costs the native GraphSAGE step on bench.py's products-like workload
(cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5; features 100, hidden 256, fanout 15/10/5, batch
1024, one GPU), and what bounds the drop kernel.

    python profiles/dropout_bench.py [--reps 5] [--steps 64] [--out FILE]

* the native step's rate at dropout 0 and 0.5: two trainers in ONE process, alternating, `--steps` steps per timed run
  (wall clock around Trainer.run, every run slicing one round ahead as bench.py's end-to-end leg does), median (min, max);
* csl_dropout_f32 per launch by device events, in place, on matrices of the two hidden layers' sizes at this shape and
  on one far larger than the caches, against the bytes it moves (2 * rows * width * 4: one read, one write): the
  GB/s of each, 20 back-to-back launches per event pair.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "occ-gnn_amd"))

from cslicer import aggr, l0  # noqa: E402
from cslicer.train import Trainer, synthetic_node_data, use_tuned_gemms  # noqa: E402

CALLS = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, F, C = l0.PRESETS["products-like"]
    hidden, fan, B, S = 256, (15, 10, 5), 1024, 8
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    use_tuned_gemms()
    feats = lambda own: synthetic_node_data(n, F, C, seed=0, rows=own)[0]    # noqa: E731
    labels = lambda own: synthetic_node_data(n, 1, C, seed=0, rows=own)[1]   # noqa: E731
    perm = np.random.default_rng(1).permutation(n).astype(np.int64)
    lines = ["products-like: N %d, E %d, features %d, hidden %d, fanout 15/10/5, batch %d, %d streams (graph %.1f s)"
             % (n, indices.shape[0], F, hidden, B, S, time.time() - t0)]
    ps = (0.0, 0.5)
    trs = [Trainer(indptr, indices, feats, labels, C, fanouts=fan, batch=B, streams=S, hidden=hidden, feat_dim=F, dropout=p)
           for p in ps]
    at = []
    for tr in trs:
        assert tr.plan.path == "native"
        tr.set_nodes(perm)
        tr.run(48, then=(48, a.steps))
        at.append(48)
    rates = [[] for _ in ps]
    for _ in range(a.reps):
        for k, tr in enumerate(trs):
            nxt = (at[k] + a.steps) % tr.n_batches
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.run(a.steps, first_batch=at[k], then=(nxt, a.steps))
            torch.cuda.synchronize()
            rates[k].append(a.steps / (time.perf_counter() - t))
            at[k] = nxt
    rows = [[u["rows"] / max(tr.steps_done, 1) for u in tr.units] for tr in trs]
    lines += ["", "native step, %d steps per run, median (min, max) of %d runs, the two trainers alternating:" % (a.steps, a.reps)]
    for p, r in zip(ps, rates):
        lines.append("  dropout %.1f  %8.0f minibatches/s (%.0f, %.0f)" % (p, np.median(r), min(r), max(r)))
    lines.append("  ratio of the medians (0.5 / 0): %.3f" % (np.median(rates[1]) / np.median(rates[0])))
    lines.append("  output rows per step of the model's layers (deepest first): %s" % " ".join("%.0f" % x for x in rows[1]))
    for tr in trs:
        tr.close()
    # ---- the kernel alone
    lines += ["", "csl_dropout_f32 in place, width %d, p 0.5, %d launches per event pair, median (min, max) of %d:"
              % (hidden, CALLS, a.reps)]
    sizes = [int(rows[1][0]), int(rows[1][1]), 1 << 20]
    for m in sizes:
        x = torch.rand((m, hidden), device="cuda")
        ids = torch.randperm(n, device="cuda")[:m].int() if m <= n else None
        aggr.dropout(x, ids, 0.5, 1, 0, 0, out=x)
        torch.cuda.synchronize()
        ts = []
        for r in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for c in range(CALLS):
                aggr.dropout(x, ids, 0.5, 1, 0, r * CALLS + c, out=x)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3 / CALLS)
        byt = 2.0 * m * hidden * 4
        lines.append("  %8d rows (%7.1f MB moved): %7.1f us (%.1f, %.1f) = %6.0f GB/s"
                     % (m, byt / 1e6, np.median(ts) * 1e6, min(ts) * 1e6, max(ts) * 1e6, byt / np.median(ts) / 1e9))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
