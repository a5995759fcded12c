"""Full-neighbour inference of both models on the products-shaped preset (cslicer.l0.PRESETS["products-like"]:
2.45 M nodes, mean degree 50.5, pareto degrees): per layer the time of its full-row aggregation kernels (device events,
after a warm-up, median and spread of repeated runs), the algorithmic bytes they gather and write, and the fraction of
8 TB/s that is; then the whole inference call.

    python profiles/infer_bench.py [--reps 7] [--out FILE]

Algorithmic bytes of a layer's aggregation (every row counted once per use, fp32, padded widths):
  SAGE aggregate first (w = input width):  E w 4 (neighbour rows) + N w 4 (own row) + N 2w 4 (operand written)
  SAGE project first   (w = output width): E w 4 (neighbour half of P) + N w 4 (own half) + N w 4 (output written)
  GAT                  (C = H D):          E (C + H) 4 (z and el rows) + N (C + H) 4 (er, output written)
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

from cslicer import infer, l0, splitgnn  # noqa: E402

PEAK = 8e12


def timed(fn, reps):
    fn()                                                    # warm-up (GEMM plans, caches)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, d, F, C = l0.PRESETS["products-like"]
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    g = infer.graph_of(indptr, indices, dev).upload()
    E = g.n_edges
    lines = ["products-like: N %d, E %d (self loops removed), max degree %d, hub rows (> %d edges) %d, graph + plan %.1f s"
             % (g.N, E, int(np.diff(g.host_indptr).max()), infer.SEG, g.all_rows.plan["hubs"].shape[0], time.time() - t0)]
    feats = torch.rand((n, F), device=dev)
    res = {"graph": {"N": g.N, "E": E}, "models": {}}
    torch.manual_seed(0)
    models = {"sage": splitgnn.DistSAGEModel(F, 256, C, n_layers=3).to(dev),
              "gat": splitgnn.DistGATModel(F, 32, C, heads=8, n_layers=3).to(dev)}
    chunk = infer.CHUNK_ROWS
    for name, model in models.items():
        layers = []
        with torch.no_grad():
            h = feats
            in_map = torch.arange(F, device=dev)
            for k, conv in enumerate(model.convs):
                last = k + 1 == len(model.convs)
                if name == "sage":
                    W = conv.fc.weight
                    out_w, in_w = W.shape[0], W.shape[1] // 2
                    hp, op = h.shape[1], infer._r4(out_w)
                    if out_w >= in_w:
                        cat = torch.empty((chunk, 2 * hp), device=dev)
                        fn = lambda h=h, hp=hp, cat=cat: infer.sage_rows(   # noqa: E731
                            g, g.all_rows, h, hp, hp, False, None, False, lambda k0, k1: cat[:k1 - k0], chunk)
                        form, w = "aggregate first", hp
                        byt = (E * w + g.N * w + g.N * 2 * w) * 4
                    else:
                        P = torch.empty((g.N, 2 * op), device=dev).uniform_()
                        y = torch.empty((g.N, op), device=dev)
                        bp = torch.zeros((op,), device=dev)
                        fn = lambda P=P, y=y, op=op, bp=bp: infer.sage_rows(  # noqa: E731
                            g, g.all_rows, P, 2 * op, op, True, bp, True, y, chunk)
                        form, w = "project first", op
                        byt = (E * w + g.N * w + g.N * w) * 4
                    tk = timed(fn, a.reps)
                    h_next = infer._sage_layer(g, g.all_rows, h, conv, not last, chunk)
                    desc = "%d -> %d %s" % (in_w, out_w, form)
                else:
                    H, Dp = conv.H, infer._r4(conv.D)
                    z = torch.empty((g.N, H * Dp), device=dev).uniform_()
                    el = torch.empty((g.N, H), device=dev).uniform_()
                    er = torch.empty((g.N, H), device=dev).uniform_()
                    bz = torch.zeros((H * Dp,), device=dev)
                    out = torch.empty((g.N, C) if last else (g.N, H * Dp), device=dev)
                    fn = lambda z=z, el=el, er=er, bz=bz, out=out, H=H, Dp=Dp, last=last: infer.gat_rows(  # noqa: E731
                        g, g.all_rows, z, el, er, H, Dp, 0.2, bz, last, C if last else 0, out, chunk)
                    tk = timed(fn, a.reps)
                    del z, el, er, out
                    byt = (E * (H * Dp + H) + g.N * (H * Dp + H)) * 4
                    h_next, in_map = infer._gat_layer(g, g.all_rows, h, in_map, conv, last, C, chunk)
                    desc = "%d heads x %d %s" % (H, Dp, "head mean" if last else "ELU")
                h = h_next
                layers.append({"layer": k, "what": desc, "kernel_s": tk[0], "min_s": tk[1], "max_s": tk[2], "bytes": byt,
                               "TBps": byt / tk[0] / 1e12, "peak_frac": byt / tk[0] / PEAK})
                lines.append("%-5s layer %d %-28s aggregation %.3f ms (min %.3f, max %.3f of %d), %.2f GB, %.2f TB/s = "
                             "%.0f %% of 8 TB/s" % (name, k, desc, tk[0] * 1e3, tk[1] * 1e3, tk[2] * 1e3, a.reps, byt / 1e9,
                                                    byt / tk[0] / 1e12, 100 * byt / tk[0] / PEAK))
            del h
        tw = timed(lambda model=model: infer.full_inference(model, indptr, indices, feats), max(3, a.reps // 2))
        lines.append("%-5s whole full_inference (all nodes): %.1f ms (min %.1f, max %.1f)" % (name, tw[0] * 1e3, tw[1] * 1e3,
                                                                                            tw[2] * 1e3))
        res["models"][name] = {"layers": layers, "total_s": tw[0], "total_min_s": tw[1], "total_max_s": tw[2]}
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
