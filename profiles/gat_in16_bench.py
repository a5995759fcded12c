"""The attention model's input layer on a float32, float16 and bfloat16 feature table, on the products-shaped preset
(cslicer.l0.PRESETS["products-like"]: 2.45 M nodes, mean degree 50.5, features 100) with BASELINE config 5's model
(3 layers, 8 heads x 32, fanout 10/10/10, batch 1024).  Per table type, float32 first:

    k_gatin_fwd and k_gatin_bwd alone (csl_gat_in_fwd_* / csl_gat_in_bwd_*; the backward's call includes the second
        stage of its two-stage sums) on ONE minibatch's deepest slice, 10 back-to-back calls / 10;
    the whole layer, forward + backward (aggr.GatInputLayer: one native call per direction);
    the trainer's step with gat_input on and off.  The off leg on a 16-bit table is the project-then-aggregate path such
        a table had before the layer could read it (upcasting gather, projection of every source row): the baseline.

Device events, after a warm-up, median (min, max) of repeated runs.

    python profiles/gat_in16_bench.py [--reps 7] [--steps 32] [--out FILE]

The same values in all three tables: uniform [0, 1) rounded to bfloat16 first and float16 second, so every entry is
exact in all three formats.  The first step's loss of the three `on` trainers is printed and must agree bitwise (later
steps carry the upper layers' float atomics, whose order varies from run to run).
"""
import argparse
import ctypes as C
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


def mmm(t, scale):
    return "%.1f (min %.1f, max %.1f)" % (t[0] * scale, t[1] * scale, t[2] * scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=32, help="training steps per timed run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, F, classes = l0.PRESETS["products-like"]
    heads, hid, fan, B, slope = 8, 32, (10, 10, 10), 1024, 0.2
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    rng = np.random.default_rng(0)
    base = torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(torch.bfloat16).to(torch.float16).float()
    assert torch.equal(base.to(torch.bfloat16).float(), base) and torch.equal(base.to(torch.float16).float(), base)
    labels = rng.integers(0, classes, size=n).astype(np.int64)
    perm = rng.permutation(n)
    lines = ["products-like: N %d, E %d, features %d, %d heads x %d, fanout 10/10/10, batch %d (graph + table %.1f s)"
             % (n, indices.shape[0], F, heads, hid, B, time.time() - t0)]
    L = aggr._lib()
    res = {}
    for dt in DTYPES:
        r = res[dt] = {}
        for on in (True, False):
            tr = Trainer(indptr, indices, base, labels, classes, fanouts=fan, batch=B, streams=32, hidden=hid, heads=heads,
                         model="gat", lr=1e-3, seed=0, feature_dtype=dt, gat_input=on)
            assert bool(tr.gat_input) == on and tr.feat.element_size() == (4 if dt == "float32" else 2)
            tr.set_nodes(perm)
            if on:
                # ---- one minibatch's deepest slice: the two edge kernels alone, then the whole layer
                tr.eng.submit_round(0, B, 1, slot=0)
                deep = splitgnn.slices_of(tr.eng, 0, 0, parts=[0], device=tr.dev)[len(fan) - 1][0]
                n_out, n_edges, n_src = deep.n_out, deep.n_edges, int(deep.in_nodes.numel())
                conv = tr.model.convs[0]
                H, D = conv.attn_l.shape
                kind = aggr._table(tr.feat)
                Wv = conv.fc.weight.detach().view(H, D, F)
                vl = torch.einsum("hdf,hd->hf", Wv, conv.attn_l.detach()).contiguous()
                vr = torch.einsum("hdf,hd->hf", Wv, conv.attn_r.detach()).contiguous()
                agg = torch.empty((n_out, H * F), device=tr.dev)
                alpha = torch.empty((max(n_edges, 1), H), device=tr.dev)
                dagg = torch.randn((n_out, H * F), device=tr.dev)
                gv = torch.empty((2, H, F), device=tr.dev)
                buf = torch.empty((max(int(L.csl_gat_in_bwd_scratch(n_out, H, F)), 4),), device=tr.dev)
                p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
                head = (p(deep.indptr), p(deep.indices), p(deep.self_ids_in), p(deep.in_nodes), p(tr.feat))
                twins_f, twins_b = aggr._twins("gat_in_fwd"), aggr._twins("gat_in_bwd")

                def k_fwd():
                    for _ in range(CALLS):
                        aggr._table_call(twins_f, kind, head, (tr.feat.stride(0), F, p(vl), p(vr), H, slope, n_out, n_edges,
                                                               deep.fanout, p(agg), p(alpha), aggr._stream()))

                def k_bwd():
                    for _ in range(CALLS):
                        aggr._table_call(twins_b, kind, head, (tr.feat.stride(0), F, p(alpha), p(dagg), H * F, F, H, slope,
                                                               n_out, n_edges, deep.fanout, p(gv[0]), p(gv[1]), p(buf),
                                                               aggr._stream()))

                params = [t.detach().clone().requires_grad_() for t in (conv.fc.weight, conv.attn_l, conv.attn_r, conv.bias)]
                g_out = torch.randn((n_out, H * D), device=tr.dev)

                def layer():
                    out = aggr.GatInputLayer.apply(tr.feat, deep.in_nodes, *params, deep.indptr, deep.indices,
                                                   deep.self_ids_in, n_out, n_edges, deep.fanout, slope, True, 0, False)
                    out.backward(g_out)

                tf, tb, tl = timed(k_fwd, a.reps, CALLS), timed(k_bwd, a.reps, CALLS), timed(layer, a.reps)
                row_bytes = (n_out + n_edges) * F * tr.feat.element_size()       # table rows a pass reads, every use counted
                r.update({"rows": n_out, "edges": n_edges, "sources": n_src, "row_bytes_per_pass": row_bytes,
                          "k_gatin_fwd_us": [x * 1e6 for x in tf], "k_gatin_bwd_us": [x * 1e6 for x in tb],
                          "layer_fwd_bwd_us": [x * 1e6 for x in tl]})
                lines.append("%-8s deepest layer, %d rows, %d edges, %d sources, %.0f MB of table rows per pass: k_gatin_fwd %s us, "
                             "k_gatin_bwd %s us, layer forward + backward %s us"
                             % (dt, n_out, n_edges, n_src, row_bytes / 1e6, mmm(tf, 1e6), mmm(tb, 1e6), mmm(tl, 1e6)))
            # ---- the training step
            first = tr.run(a.steps)                                           # warm-up: plans, allocator, slicer ahead
            at = [a.steps]

            def steps():
                tr.run(a.steps, first_batch=at[0] % tr.n_batches)
                at[0] += a.steps

            ts = timed(steps, a.reps, a.steps)
            leg = "on" if on else "off"
            r["step_%s_ms" % leg], r["first_loss_%s" % leg] = [x * 1e3 for x in ts], float(first[0])
            lines.append("%-8s trainer step, gat_input %-3s (%s): %.4f ms (min %.4f, max %.4f of %d x %d steps) = %.0f minibatches/s"
                         % (dt, leg, "aggregate-then-project" if on else "project-then-aggregate", ts[0] * 1e3, ts[1] * 1e3,
                            ts[2] * 1e3, a.reps, a.steps, 1.0 / ts[0]))
            tr.close()
            del tr
            torch.cuda.empty_cache()
    same = all(np.float32(res[dt]["first_loss_on"]).view(np.uint32) == np.float32(res["float32"]["first_loss_on"]).view(np.uint32)
               for dt in DTYPES)
    lines.append("first-step loss of the three `on` trainers agrees bitwise: %s" % same)
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
