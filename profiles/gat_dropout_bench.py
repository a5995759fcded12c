"""What dropout costs the attention model's training step on bench.py's products-like workload at BASELINE config 5's
shape (cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5; features 100, 3 layers, 8 heads x 32, fanout
10/10/10, batch 1024, one GPU), and where the cost of attention dropout comes from.

    python profiles/gat_dropout_bench.py [--reps 5] [--steps 64] [--out FILE]

* the step's rate with no dropout, feat_dropout 0.6, attn_dropout 0.6 and both, plus no dropout with gat_input off (what
  attn_dropout loses by taking the deepest layer off aggr.GatInputLayer): five trainers in ONE process, alternating,
  `--steps` steps per timed run (wall clock around Trainer.run, every run slicing one round ahead as bench.py's end-to-end
  leg does), median (min, max);
* csl_gat_drop_fwd_f32 against csl_gat_fwd_f32 per launch by device events at the three layers' shapes of this workload
  (rows and sources per step as the trainers counted them, fanout edges per row, random sources): what the Philox calls
  cost the forward aggregation, 20 back-to-back launches per event pair on the same inputs -- the two smaller shapes
  therefore run out of cache and their ratios are indicative only.
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
from cslicer.train import Trainer, synthetic_node_data, use_tuned_gemms  # noqa: E402

CALLS = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, F, Cn = l0.PRESETS["products-like"]
    heads, hidden, fan, B, S = 8, 32, (10, 10, 10), 1024, 8
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    use_tuned_gemms()
    feats = lambda own: synthetic_node_data(n, F, Cn, seed=0, rows=own)[0]    # noqa: E731
    labels = lambda own: synthetic_node_data(n, 1, Cn, seed=0, rows=own)[1]   # noqa: E731
    perm = np.random.default_rng(1).permutation(n).astype(np.int64)
    lines = ["products-like: N %d, E %d, features %d, GAT %d heads x %d, fanout 10/10/10, batch %d, %d streams (graph %.1f s)"
             % (n, indices.shape[0], F, heads, hidden, B, S, time.time() - t0)]
    cfgs = [("no dropout", {}), ("feat_dropout 0.6", dict(feat_dropout=0.6)), ("attn_dropout 0.6", dict(attn_dropout=0.6)),
            ("both 0.6", dict(feat_dropout=0.6, attn_dropout=0.6)), ("no dropout, gat_input off", dict(gat_input=False))]
    trs = [Trainer(indptr, indices, feats, labels, Cn, fanouts=fan, batch=B, streams=S, hidden=hidden, heads=heads, feat_dim=F,
                   model="gat", **kw) for _, kw in cfgs]
    at = []
    for tr in trs:
        tr.set_nodes(perm)
        tr.run(32, then=(32, a.steps))
        at.append(32)
    rates = [[] for _ in cfgs]
    for _ in range(a.reps):
        for k, tr in enumerate(trs):
            nxt = (at[k] + a.steps) % tr.n_batches
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.run(a.steps, first_batch=at[k], then=(nxt, a.steps))
            torch.cuda.synchronize()
            rates[k].append(a.steps / (time.perf_counter() - t))
            at[k] = nxt
    units = [{k: v / max(trs[0].steps_done, 1) for k, v in u.items()} for u in trs[0].units]
    lines += ["", "training step, %d steps per run, median (min, max) of %d runs, the %d trainers alternating:"
              % (a.steps, a.reps, len(cfgs))]
    base = np.median(rates[0])
    for (name, _), tr, r in zip(cfgs, trs, rates):
        lines.append("  %-26s %7.1f minibatches/s (%.1f, %.1f)  %.3f of no dropout  [gat_input %s]"
                     % (name, np.median(r), min(r), max(r), np.median(r) / base, "on" if tr.gat_input else "off"))
    lines.append("  per step, the model's layers (deepest first): output rows %s, source rows %s, edges %s" % tuple(
        " ".join("%.0f" % u[k] for u in units) for k in ("rows", "src", "edges")))
    for tr in trs:
        tr.close()
    # ---- the forward aggregation alone, with and without the mask
    L = aggr._lib()
    C_ = heads * hidden
    lines += ["", "csl_gat_fwd_f32 / csl_gat_drop_fwd_f32 (p_a 0.6), %d x %d columns, 10 edges per row, %d launches per event pair, "
              "median (min, max) of %d:" % (heads, hidden, CALLS, a.reps)]
    for u in units:
        rows, src = int(u["rows"]), int(u["src"])
        g = torch.Generator(device="cuda").manual_seed(rows)
        indptr_t = (torch.arange(rows + 1, device="cuda") * 10).int()
        indices_t = torch.randint(0, src, (rows * 10,), device="cuda", generator=g).int()
        el, er = torch.randn(src, heads, device="cuda"), torch.randn(rows, heads, device="cuda")
        z = torch.randn(src, C_, device="cuda")
        src_ids = torch.randperm(n, device="cuda")[:src].int()
        dst_ids = src_ids[:rows].clone()
        m, s = torch.empty(rows, heads, device="cuda"), torch.empty(rows, heads, device="cuda")
        out = torch.empty(rows, C_, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())    # noqa: E731
        head = (p(indptr_t), p(indices_t), rows, p(el), p(er), p(z), heads, hidden, 0.2, p(m), p(s), p(out))

        def plain(step):
            assert L.csl_gat_fwd_f32(*head, aggr._stream()) == 0

        def dropped(step):
            assert L.csl_gat_drop_fwd_f32(*head, p(src_ids), p(dst_ids), 0.6, 1, 1, step, aggr._stream()) == 0
        res = {}
        for name, fn in (("plain", plain), ("dropped", dropped)):
            fn(0)
            torch.cuda.synchronize()
            ts = []
            for r in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for c in range(CALLS):
                    fn(r * CALLS + c)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / CALLS)
            res[name] = ts
        lines.append("  %7d rows, %7d sources: plain %7.1f us (%.1f, %.1f), dropped %7.1f us (%.1f, %.1f), ratio %.2f"
                     % (rows, src, np.median(res["plain"]), min(res["plain"]), max(res["plain"]), np.median(res["dropped"]),
                        min(res["dropped"]), max(res["dropped"]), np.median(res["dropped"]) / np.median(res["plain"])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
