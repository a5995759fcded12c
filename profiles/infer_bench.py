"""Full-neighbour inference of both models on the products-shaped preset (cslicer.l0.PRESETS["products-like"]:
2.45 M nodes, mean degree 50.5, pareto degrees): per layer the time of its full-row aggregation kernels (device events,
after a warm-up, median and spread of repeated runs), the algorithmic bytes they gather and write, and the fraction of
8 TB/s that is; then the whole inference call.

    python profiles/infer_bench.py [--reps 7] [--out FILE] [--feature-dtype float32,float16,bfloat16]

--feature-dtype: the element types of the feature table, one pass each in the same run (default float32 alone).  Only a
model's first layer reads the table, so a 16-bit pass times that layer -- GraphSAGE's aggregate-first kernels on the table
in place (csl_infer_sage_x16), the attention model's first projection (per-chunk upcast + GEMM against the float32 GEMM
in place) and the upcast kernel alone over the whole table -- then the whole call, and the rise of torch's allocated
bytes over it.

Algorithmic bytes of a layer's aggregation (every row counted once per use, padded widths; e = 4, or 2 where the rows
gathered are those of a 16-bit feature table):
  SAGE aggregate first (w = input width):  E w e (neighbour rows) + N w e (own row) + N 2w 4 (operand written)
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


def peak_rise(fn):
    """bytes by which torch's allocations rise over one call"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--feature-dtype", default="float32",
                    help="comma-separated element types of the feature table (float32, float16, bfloat16), one pass each")
    a = ap.parse_args()
    dtypes = a.feature_dtype.split(",")
    for d in dtypes:
        if d not in l0.FEATURE_DTYPES:
            ap.error("--feature-dtype: %r is not one of %s" % (d, ", ".join(l0.FEATURE_DTYPES)))
    dev = torch.device("cuda", 0)
    n, d, F, C = l0.PRESETS["products-like"]
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    g = infer.graph_of(indptr, indices, dev).upload()
    E = g.n_edges
    lines = ["products-like: N %d, E %d (self loops removed), max degree %d, hub rows (> %d edges) %d, graph + plan %.1f s"
             % (g.N, E, int(np.diff(g.host_indptr).max()), infer.SEG, g.all_rows.plan["hubs"].shape[0], time.time() - t0)]
    feats32 = torch.rand((n, F), device=dev)
    res = {"graph": {"N": g.N, "E": E}, "models": {}}
    torch.manual_seed(0)
    models = {"sage": splitgnn.DistSAGEModel(F, 256, C, n_layers=3).to(dev),
              "gat": splitgnn.DistGATModel(F, 32, C, heads=8, n_layers=3).to(dev)}
    chunk = infer.CHUNK_ROWS
    feats = feats32
    for name, model in (models.items() if "float32" in dtypes else ()):
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
        if len(dtypes) > 1:
            first_layer_f32(name, model, feats, g, indptr, indices, chunk, a.reps, lines, res)
    for fd in dtypes:                                       # (after the float32 pass: its figures are the comparison)
        if fd != "float32":
            first_layer_16(fd, feats32.to(getattr(torch, fd)), g, models, indptr, indices, chunk, a.reps, lines, res)
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(res) + "\n")


def first_projection(model, h, g, chunk):
    """the attention model's first projection z = h W^T over every row, as _gat_layer runs it: chunk by chunk, a 16-bit
    table's rows upcast into one buffer first (the preset's widths are multiples of 4: the weight needs no padding)"""
    wz = model.convs[0].fc.weight.detach()
    z = torch.empty((g.N, wz.shape[0]), device=h.device)
    return lambda: infer._project_rows(h, wz, z, chunk)


def first_layer_f32(name, model, feats, g, indptr, indices, chunk, reps, lines, res):
    """what first_layer_16 times, on the float32 table in place: the figures a 16-bit pass is compared with"""
    rec = res["models"][name]
    if name == "gat":
        tp = timed(first_projection(model, feats, g, chunk), reps)
        lines.append("gat   float32  layer 0 projection z = h W^T (GEMM on the table in place) %.3f ms (min %.3f, max %.3f of %d)"
                     % (tp[0] * 1e3, tp[1] * 1e3, tp[2] * 1e3, reps))
        rec["projection_s"] = tp
    rise = peak_rise(lambda: infer.full_inference(model, indptr, indices, feats))
    lines.append("%-5s float32  whole full_inference: torch's allocated bytes rise by %.1f MB (table %.1f MB, in place)"
                 % (name, rise / 1e6, feats.numel() * 4 / 1e6))
    rec["peak_rise_bytes"] = rise


def first_layer_16(fd, feats, g, models, indptr, indices, chunk, reps, lines, res):
    """one pass over a 16-bit table: the first layer's readers, the whole calls"""
    dev = feats.device
    E, F = g.n_edges, feats.shape[1]
    out = res.setdefault(fd, {})
    cat = torch.empty((chunk, 2 * F), device=dev)
    tk = timed(lambda: infer.sage_rows(g, g.all_rows, feats, feats.stride(0), F, False, None, False,
                                       lambda k0, k1: cat[:k1 - k0], chunk), reps)
    byt = (E * F + g.N * F) * 2 + g.N * 2 * F * 4
    lines.append("sage  %-8s layer 0 %d -> 256 aggregate first, table in place  aggregation %.3f ms (min %.3f, max %.3f of %d), "
                 "%.2f GB, %.2f TB/s = %.0f %% of 8 TB/s" % (fd, F, tk[0] * 1e3, tk[1] * 1e3, tk[2] * 1e3, reps, byt / 1e9,
                                                            byt / tk[0] / 1e12, 100 * byt / tk[0] / PEAK))
    out["sage_layer0"] = {"kernel_s": tk[0], "min_s": tk[1], "max_s": tk[2], "bytes": byt}
    del cat
    tp = timed(first_projection(models["gat"], feats, g, chunk), reps)
    lines.append("gat   %-8s layer 0 projection z = h W^T (per-chunk upcast + GEMM)         %.3f ms (min %.3f, max %.3f of %d)"
                 % (fd, tp[0] * 1e3, tp[1] * 1e3, tp[2] * 1e3, reps))
    rows = infer._RowChunks(feats, chunk)

    def upcast():
        for r0 in range(0, g.N, chunk):
            rows(r0, min(g.N, r0 + chunk))
    tu = timed(upcast, reps)
    ub = g.N * F * 6
    lines.append("      %-8s csl_upcast_rows_x16 over the whole table, chunk by chunk       %.3f ms (min %.3f, max %.3f of %d), "
                 "%.2f GB, %.2f TB/s" % (fd, tu[0] * 1e3, tu[1] * 1e3, tu[2] * 1e3, reps, ub / 1e9, ub / tu[0] / 1e12))
    out["gat_projection_s"], out["upcast_s"] = tp, tu
    del rows
    for name, model in models.items():
        tw = timed(lambda model=model: infer.full_inference(model, indptr, indices, feats), max(3, reps // 2))
        rise = peak_rise(lambda model=model: infer.full_inference(model, indptr, indices, feats))
        lines.append("%-5s %-8s whole full_inference (all nodes): %.1f ms (min %.1f, max %.1f); torch's allocated bytes rise "
                     "by %.1f MB (table %.1f MB, in place)" % (name, fd, tw[0] * 1e3, tw[1] * 1e3, tw[2] * 1e3, rise / 1e6,
                                                              feats.numel() * 2 / 1e6))
        out[name] = {"total_s": tw[0], "total_min_s": tw[1], "total_max_s": tw[2], "peak_rise_bytes": rise}


if __name__ == "__main__":
    main()
