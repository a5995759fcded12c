"""Correct and Smooth on the products-shaped preset (cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5,
47 classes: W = 48), in one process:

  * one csl_prop_f32 pass over all rows, as an inner iteration runs it (base term read, the pre-scaled operand written);
  * the existing csl_infer_sage_f32 project-first pass at the same W on the same graph -- the same gather shape, the
    yardstick -- the two alternating, three runs each of --passes passes between two device events, median (min, max);
  * the new pass's algorithmic bytes over its time: E W 4 (neighbour rows) + N W 4 (base) + N W 4 (written);
  * the wall time of a whole default correct_and_smooth (50 + 50 iterations, autoscale; a tenth of the nodes labelled).

    python profiles/smooth_bench.py [--passes 20] [--out profiles/smooth_bench_products.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "occ-gnn_amd"))

from cslicer import infer, l0, smooth  # noqa: E402


def run_ms(fn, passes):
    """milliseconds per pass of `passes` back-to-back passes between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(passes):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / passes


def stats(ts):
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, d, _, C = l0.PRESETS["products-like"]
    W = infer._r4(C)
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    g = infer.graph_of(indptr, indices, dev).upload()
    N, E = g.N, g.n_edges
    lines = ["products-like: N %d, E %d (self loops removed), hub rows (> %d edges) %d, C = %d, W = %d, graph + plan %.1f s"
             % (N, E, infer.SEG, g.all_rows.plan["hubs"].shape[0], C, W, time.time() - t0)]
    chunk = infer.CHUNK_ROWS
    torch.manual_seed(0)
    x0 = torch.rand((N, W), device=dev)
    x0[:, C:] = 0

    # one inner iteration as smooth.propagate issues it: alpha 0.8, base read, only the pre-scaled operand written
    dinv = smooth.dinv_of(g)
    cur, nxt = x0 * dinv[:, None], torch.empty_like(x0)
    plan = g.all_rows
    chunks = plan.chunks(chunk)
    part = infer._partial(max(c.n_parts for c in chunks), W, dev)
    L, st, nul = smooth._abi.load(), smooth.aggr._stream(), infer._ptr(None)

    def prop_pass():
        for c in chunks:
            infer._chk(L.csl_prop_f32(*infer._list_args(g.indptr, g.indices, plan.items, plan.hubs, c, c.k0), infer._ptr(cur), W, W,
                                      infer._ptr(dinv), 0.8, infer._ptr(x0, c.k0 * W), W, 0.2, 0.0, 1.0,
                                      infer._ptr(part) if c.n_parts else nul, nul, W, infer._ptr(nxt, c.k0 * W), W, st),
                       "csl_prop_f32")
    P = torch.rand((N, 2 * W), device=dev)
    y = torch.empty((N, W), device=dev)
    bias = torch.zeros((W,), device=dev)

    def sage_pass():
        infer.sage_rows(g, plan, P, 2 * W, W, True, bias, True, y, chunk)
    for fn in (prop_pass, sage_pass):                      # warm-up: code objects, caches
        run_ms(fn, 3)
    tp, ts = [], []
    for _ in range(3):                                      # alternating, so that drift and neighbours hit both alike
        tp.append(run_ms(prop_pass, a.passes))
        ts.append(run_ms(sage_pass, a.passes))
    byt = (E * W + 2 * N * W) * 4
    mp, ms = stats(tp), stats(ts)
    lines.append("csl_prop_f32, one pass over all rows (base read, out_s written): %.3f ms (min %.3f, max %.3f of 3 runs of %d passes)"
                 % (mp + (a.passes,)))
    lines.append("csl_infer_sage_f32 project first, W = %d, same graph:            %.3f ms (min %.3f, max %.3f of 3 runs of %d passes)"
                 % ((W,) + ms + (a.passes,)))
    lines.append("csl_prop_f32: %.2f GB algorithmic (E W 4 + N W 4 base + N W 4 written), %.2f TB/s; the sibling moves the same bytes: "
                 "%.2f TB/s" % (byt / 1e9, byt / mp[0] / 1e9, byt / ms[0] / 1e9))
    lines.append("new pass / sibling: %.3f of its time (medians); the sibling's own min-max spread is %.1f %% of its median"
                 % (mp[0] / ms[0], 100 * (ms[2] - ms[1]) / ms[0]))
    del P, y, cur, nxt
    # the whole default call: random logits, a tenth of the nodes labelled
    logits = torch.randn((N, C), device=dev)
    rng = np.random.default_rng(0)
    train = np.sort(rng.permutation(N)[:N // 10])
    labels = rng.integers(0, C, train.shape[0])

    def whole():
        t = time.time()
        out = smooth.correct_and_smooth(logits, indptr, indices, train, labels)
        torch.cuda.synchronize()
        del out
        return (time.time() - t) * 1e3
    whole()
    tw = stats([whole() for _ in range(3)])
    lines.append("whole default correct_and_smooth (50 + 50 iterations, autoscale, %d labelled nodes): %.1f ms wall (min %.1f, max %.1f "
                 "of 3), %.2f ms per iteration" % ((train.shape[0],) + tw + (tw[0] / 100,)))
    res = {"N": N, "E": E, "W": W, "prop_ms": mp, "sage_ms": ms, "bytes": byt, "whole_ms": tw, "passes": a.passes}
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
