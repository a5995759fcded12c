"""The feature table in float32, float16 and bfloat16 on the products-shaped preset at the bench shape
(cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5; features 100, hidden 256, fanout 15/10/5, batch
1024): device bytes of the table, the deepest layer's forward as the one fused kernel (csl_sage_fwd_mfma_f32 / _x16)
and as the two-kernel form (csl_sage_cat_f32 / _x16 + GEMM) on ONE minibatch's deepest slice, and the native training
step.  Device events, after a warm-up, median (min, max) of repeated runs; a kernel figure is 10 back-to-back calls / 10.

    python profiles/feat16_bench.py [--reps 7] [--steps 64] [--out FILE]

The same values in all three tables: uniform [0, 1) rounded to bfloat16 first and float16 second (so every entry is
exact in all three formats and the three trainers see the same numbers; their losses are printed and must agree).
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

from cslicer import aggr, l0, splitgnn  # noqa: E402
from cslicer.train import Trainer  # noqa: E402

DTYPES = ("float32", "float16", "bfloat16")
CALLS = 10


def timed(fn, reps, per=1):
    fn()                                                    # warm-up (GEMM plans, caches)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / per)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=64, help="native steps per timed run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, F, C = l0.PRESETS["products-like"]
    hidden, fan, B = 256, (15, 10, 5), 1024              # (engine order, as bench.py passes it: layer 0 = the seeds' hop)
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    rng = np.random.default_rng(0)
    base = torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(torch.bfloat16).to(torch.float16).float()
    assert torch.equal(base.to(torch.bfloat16).float(), base) and torch.equal(base.to(torch.float16).float(), base)
    labels = rng.integers(0, C, size=n).astype(np.int64)
    perm = rng.permutation(n)
    lines = ["products-like: N %d, E %d, features %d, hidden %d, fanout 15/10/5, batch %d (graph + table %.1f s)"
             % (n, indices.shape[0], F, hidden, B, time.time() - t0)]
    res = {}
    for dt in DTYPES:
        tr = Trainer(indptr, indices, base, labels, C, fanouts=fan, batch=B, streams=64, hidden=hidden, lr=1e-3,
                     seed=0, feature_dtype=dt)
        assert tr.native is not None and tr.fused_deepest_layer()
        tr.set_nodes(perm)
        table_bytes = tr.feat.numel() * tr.feat.element_size()
        assert table_bytes == n * F * (4 if dt == "float32" else 2)
        # ---- one minibatch's deepest slice, the two forms of its forward
        tr.eng.submit_round(0, B, 1, slot=0)
        deep = splitgnn.slices_of(tr.eng, 0, 0, parts=[0], device=tr.dev)[len(fan) - 1][0]
        m, mp = deep.n_out, splitgnn._pad_rows(deep.n_out)
        conv = tr.model.convs[0]
        W, b = conv.fc.weight.detach(), conv.fc.bias.detach()

        def fused():
            for _ in range(CALLS):
                aggr.sage_fwd_mfma(tr.feat, deep.self_ids_in, deep.indptr, deep.indices, W, b, m, mp,
                                   rowmap=deep.in_nodes, relu_out=True, want_cat=True)

        def two_kernels():
            for _ in range(CALLS):
                cat = aggr.sage_cat(tr.feat, deep.self_ids_in, m, mp, indptr=deep.indptr, indices=deep.indices,
                                    rowmap=deep.in_nodes)
                aggr.gemm(cat, W, transb=True, bias=b, relu=True)

        def cat_only():
            for _ in range(CALLS):
                aggr.sage_cat(tr.feat, deep.self_ids_in, m, mp, indptr=deep.indptr, indices=deep.indices,
                              rowmap=deep.in_nodes)

        with torch.no_grad():
            tf = timed(fused, a.reps, CALLS)
            t2 = timed(two_kernels, a.reps, CALLS)
            tc = timed(cat_only, a.reps, CALLS)
        edges = int(deep.indices.numel())
        row_bytes = (m + edges) * F * (4 if dt == "float32" else 2)     # gathered feature-table rows, every use counted
        # ---- the native step
        tr.run(a.steps)                                                   # warm-up: plans, allocator, slicer ahead
        at = [a.steps]
        losses = []

        def steps():
            losses.append(tr.run(a.steps, first_batch=at[0] % tr.n_batches))
            at[0] += a.steps

        ts = timed(steps, a.reps, a.steps)
        res[dt] = {"table_bytes": table_bytes, "rows": m, "edges": edges, "gathered_row_bytes": row_bytes,
                   "fused_us": [x * 1e6 for x in tf], "two_kernel_us": [x * 1e6 for x in t2],
                   "sage_cat_us": [x * 1e6 for x in tc], "step_ms": [x * 1e3 for x in ts],
                   "first_losses": losses[0][:4]}
        lines.append("%-8s table %.3f GB on the device | deepest layer, %d rows, %d edges, %.0f MB of gathered rows: fused "
                     "%.1f us (min %.1f, max %.1f), two-kernel form %.1f us (min %.1f, max %.1f; its csl_sage_cat alone %.1f) "
                     "| native step %.4f ms (min %.4f, max %.4f of %d x %d steps)"
                     % (dt, table_bytes / 1e9, m, edges, row_bytes / 1e6, tf[0] * 1e6, tf[1] * 1e6, tf[2] * 1e6, t2[0] * 1e6,
                        t2[1] * 1e6, t2[2] * 1e6, tc[0] * 1e6, ts[0] * 1e3, ts[1] * 1e3, ts[2] * 1e3, a.reps, a.steps))
        tr.close()
        del tr
        torch.cuda.empty_cache()
    same = all(res[dt]["first_losses"] == res["float32"]["first_losses"] for dt in DTYPES)
    lines.append("the three trainers' losses agree bitwise: %s" % same)
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
