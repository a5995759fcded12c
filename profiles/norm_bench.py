"""What layer normalisation between the layers costs the native GraphSAGE step on bench.py's products-like workload
(cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5; features 100, hidden 256, fanout 15/10/5, batch
1024, one GPU), and what bounds the two norm kernels.

    python profiles/norm_bench.py [--reps 5] [--steps 64] [--out FILE]

* the native step's rate without and with norm="layer": two trainers in ONE process, alternating, `--steps` steps per timed
  run (wall clock around Trainer.run, every run slicing one round ahead as bench.py's end-to-end leg does), median (min, max);
* csl_layernorm_relu_fwd_f32 (storing, in place) and csl_layernorm_bwd_f32 per launch by device events, on matrices of the
  two hidden layers' sizes at this shape and on one far larger than the caches, against the bytes each moves -- forward: the
  row read, y and xhat written, 3 * rows * width * 4 (+ rstd); backward: dn and xhat read, dz written, 3 * rows * width * 4
  (+ rstd and the block partials) -- the GB/s of each, 20 back-to-back launches per event pair.
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


def _timed(fn, reps):
    """seconds per call: median, min, max over `reps` event pairs of CALLS back-to-back calls"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _c in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / CALLS)
    return np.median(ts), min(ts), max(ts)


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
    norms = (None, "layer")
    trs = [Trainer(indptr, indices, feats, labels, C, fanouts=fan, batch=B, streams=S, hidden=hidden, feat_dim=F, norm=nm)
           for nm in norms]
    at = []
    for tr in trs:
        assert tr.plan.path == "native"
        tr.set_nodes(perm)
        tr.run(48, then=(48, a.steps))
        at.append(48)
    rates = [[] for _ in norms]
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
    for nm, r in zip(norms, rates):
        lines.append("  norm %-6s %8.0f minibatches/s (%.0f, %.0f)" % (nm, np.median(r), min(r), max(r)))
    lines.append("  ratio of the medians (layer / None): %.3f" % (np.median(rates[1]) / np.median(rates[0])))
    lines.append("  output rows per step of the model's layers (deepest first): %s" % " ".join("%.0f" % x for x in rows[1]))
    for tr in trs:
        tr.close()
    # ---- the kernels alone
    L = aggr._lib()
    gamma, beta = torch.rand(hidden, device="cuda") + 0.5, torch.rand(hidden, device="cuda")
    lines += ["", "width %d, %d launches per event pair, median (min, max) of %d:" % (hidden, CALLS, a.reps)]
    for m in (int(rows[1][0]), int(rows[1][1]), 1 << 20):
        z = torch.randn((m, hidden), device="cuda")
        y = torch.empty_like(z)
        _, xhat, rstd = aggr.layernorm_relu(z, gamma, beta, 1e-5, out=y)
        floats = int(L.csl_layernorm_bwd_scratch(m, hidden))
        parts = torch.empty((2, floats), device="cuda")
        dn = torch.randn((m, hidden), device="cuda")
        p = lambda t: aggr.C.c_void_p(t.data_ptr())      # noqa: E731

        def fwd():
            aggr._chk(L.csl_layernorm_relu_fwd_f32(p(z), hidden, p(gamma), p(beta), 1e-5, m, hidden, p(y), hidden, p(xhat), hidden,
                                                   p(rstd), 1, aggr._stream()), "csl_layernorm_relu_fwd_f32")

        def bwd():     # (in place again and again: the values decay, the bytes do not change)
            aggr._chk(L.csl_layernorm_bwd_f32(p(dn), hidden, p(xhat), hidden, p(rstd), p(gamma), m, m, hidden, p(parts[0]),
                                              p(parts[1]), aggr._stream()), "csl_layernorm_bwd_f32")
        for name, fn, byt in (("forward ", fwd, 3.0 * m * hidden * 4 + 4.0 * m),
                              ("backward", bwd, 3.0 * m * hidden * 4 + 4.0 * m + 8.0 * floats)):
            med, lo, hi = _timed(fn, a.reps)
            lines.append("  %s %8d rows (%7.1f MB moved): %7.1f us (%.1f, %.1f) = %6.0f GB/s"
                         % (name, m, byt / 1e6, med * 1e6, lo * 1e6, hi * 1e6, byt / med / 1e9))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
