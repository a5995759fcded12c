"""Split-parallel full-neighbour inference (cslicer.infer.full_inference_parts) on the products-shaped preset
(cslicer.l0.PRESETS["products-like"]), one process emulating rank 0 of P in {2, 4, 8} with ownership v % P.  Per layer
of the two models of profiles/infer_bench.py: the part and merge kernel times over every chunk (device events, after a
warm-up, median of repeated runs), their algorithmic bytes and TB/s, and the rank's exchange bytes (computed from its
plan: rows sent to the other ranks; nothing here measures an inter-GPU link, so exchange time is not measured).  The
merge kernels read a received buffer of the plan's size filled on the device, in place of the exchange.  Then the whole
call: a gloo world-of-one rank-path evaluate (its exchanges staged through host memory) next to the single-process
evaluate.

    python profiles/infer_parts_bench.py [--reps 7] [--out FILE]

Algorithmic bytes (fp32, padded widths; E_r local edges, S sub-CSR rows, R received rows, m own destinations):
  SAGE part   (w = gathered width):  E_r w 4 (source rows) + S w 4 (partial sums written)
  SAGE merge  aggregate first:       R w 4 + m w 4 (self row) + m 2w 4 (operand written)
              project first:         R w 4 + m w 4 (self half of P) + m w 4 (output written)
  GAT part    (C = H D, L = its state row, C + 2H padded to 4):  E_r (C + H) 4 (z, el) + S H 4 (er) + S L 4 (states)
  GAT merge:  R L 4 + m C 4 (hidden output; the last layer m n_cls 4)
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

from cslicer import aggr, infer, l0, splitgnn  # noqa: E402

PEAK = 8e12


def timed(fn, reps):
    fn()
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


def sage_part(pp, dp, Y, ldy, w, pack, send, part):
    L, st = infer._lib(), aggr._stream()
    for (s0, s1, i0, i1, h0, h1, p0, npart, o0, o1, r0, r1) in pp.chunks():
        infer._chk(L.csl_infer_sage_part_f32(infer._ptr(dp["ip"]), infer._ptr(dp["ix"]), infer._ptr(dp["items"], 4 * i0),
                                             i1 - i0, infer._ptr(dp["hubs"], 4 * h0), h1 - h0, s0, p0, infer._ptr(Y), ldy,
                                             w, pack, infer._ptr(part), infer._ptr(send), st), "sage_part")


def sage_merge(pp, dp, recv, x, ldx, w, proj, bias, out, ldo):
    L, st = infer._lib(), aggr._stream()
    for (s0, s1, i0, i1, h0, h1, p0, npart, o0, o1, r0, r1) in pp.chunks():
        o = out if not proj else out[o0:]
        infer._chk(L.csl_infer_sage_merge_f32(infer._ptr(dp["dst"], 2 * o0), infer._ptr(dp["ml"], pp.P * o0), o1 - o0,
                                              pp.P, infer._ptr(recv), infer._ptr(x), ldx, w, proj, infer._ptr(bias), proj,
                                              infer._ptr(o), ldo, st), "sage_merge")


def gat_part(pp, dp, z, el, er_in, H, Dp, pack, send, part):
    L, st = infer._lib(), aggr._stream()
    for (s0, s1, i0, i1, h0, h1, p0, npart, o0, o1, r0, r1) in pp.chunks():
        infer._chk(L.csl_infer_gat_part_f32(infer._ptr(dp["ip"]), infer._ptr(dp["ix"]), infer._ptr(dp["items"], 4 * i0),
                                            i1 - i0, infer._ptr(dp["hubs"], 4 * h0), h1 - h0, s0, p0, infer._ptr(z),
                                            infer._ptr(el), infer._ptr(er_in), H, Dp, 0.2, pack, infer._ptr(part),
                                            infer._ptr(send), st), "gat_part")


def gat_merge(pp, dp, recv, H, Dp, bias, last, n_cls, out):
    L, st = infer._lib(), aggr._stream()
    for (s0, s1, i0, i1, h0, h1, p0, npart, o0, o1, r0, r1) in pp.chunks():
        infer._chk(L.csl_infer_gat_merge_f32(infer._ptr(dp["ml"], pp.P * o0), o1 - o0, pp.P, infer._ptr(recv), H, Dp,
                                             infer._ptr(bias), int(last), n_cls, infer._ptr(out, o0 * out.shape[1]),
                                             out.shape[1], st), "gat_merge")


def rank_zero(indptr, indices, P, dev, F, C, reps, lines, res):
    t0 = time.time()
    owner = infer.owner_table(indptr.shape[0] - 1, P)
    rg = infer.RankGraph(indptr, indices, owner, P, 0)
    pp = rg.plan(infer.CHUNK_ROWS)
    dp = pp.upload(dev, True)
    Er, S, m, R = int(pp.sub_ix.shape[0]), int(pp.sub_ip.shape[0] - 1), pp.m, int(pp.recv_first[-1])
    S_max = max(c[1] - c[0] for c in pp.chunks())
    R_max = max(c[11] - c[10] for c in pp.chunks())
    parts = max([c[7] for c in pp.chunks()] + [1])
    out_rows = S - int(pp.sub_counts[:, 0].sum())          # sub-CSR rows that go to another rank
    lines.append("P %d, rank 0: n_own %d, local edges %d (%.1f per sub-CSR row), sub-CSR rows %d (%d to other ranks), "
                 "received rows %d, hub items %d, plan %.1f s" % (P, rg.n_own, Er, Er / max(S, 1), S, out_rows, R,
                                                                  pp.work["hubs"].shape[0], time.time() - t0))
    layers = []
    n_own = rg.n_own

    def row(model, k, what, kern, t, byt, extra=None):
        d = {"P": P, "model": model, "layer": k, "what": what, "kernel": kern, "s": t[0], "min_s": t[1], "max_s": t[2],
             "bytes": byt, "TBps": byt / t[0] / 1e12}
        if extra:
            d.update(extra)
        layers.append(d)
        lines.append("  %-4s layer %d %-26s %-14s %8.3f ms (min %.3f, max %.3f of %d) %7.2f GB %5.2f TB/s" % (
            model, k, what, kern, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, reps, byt / 1e9, byt / t[0] / 1e12))

    # GraphSAGE 100 -> 256 -> 256 -> 47: gathered widths 100, 256 (aggregate first), 48 (project first)
    for k, (w, proj, desc) in enumerate([(100, 0, "100 -> 256 aggregate first"), (256, 0, "256 -> 256 aggregate first"),
                                         (48, 1, "256 -> 47 project first")]):
        ldy = 2 * w if proj else w
        Y = torch.empty((n_own, ldy), device=dev).uniform_(-1, 1)
        send = torch.empty((S_max, w), device=dev)
        part = torch.empty((parts, w), device=dev)
        pack = pp.pack(w)
        for pk in (1, 2, 4):
            t = timed(lambda pk=pk: sage_part(pp, dp, Y[:, w:] if proj else Y, ldy, w, pk, send, part), reps)
            row("sage", k, desc, "part pack %d%s" % (pk, " *" if pk == pack else ""), t, (Er + S) * w * 4)
        recv = torch.empty((R_max, w), device=dev).uniform_(-1, 1)
        bias = torch.zeros((w,), device=dev)
        out = torch.empty((min(infer.CHUNK_ROWS, max(m, 1)), 2 * w), device=dev) if not proj else \
            torch.empty((m, w), device=dev)
        t = timed(lambda: sage_merge(pp, dp, recv, Y, ldy, w, proj, bias, out, w if proj else 2 * w), reps)
        row("sage", k, desc, "merge", t, (R + m + (1 if proj else 2) * m) * w * 4,
            {"exchange_bytes": out_rows * w * 4})
        lines.append("  sage layer %d exchange: %d rows x %d floats = %.3f GB sent to the other ranks (not measured)"
                     % (k, out_rows, w, out_rows * w * 4 / 1e9))
        del Y, send, part, recv, out
    # GAT 8 heads x 32 (ELU) twice, then 8 heads x 48 head mean
    H = 8
    for k, (Dp, last) in enumerate([(32, False), (32, False), (48, True)]):
        Cz = H * Dp
        pld = int(infer._lib().csl_infer_gat_partial_ld(H, Dp))
        z = torch.empty((n_own, Cz), device=dev).uniform_()
        el = torch.empty((n_own, H), device=dev).uniform_()
        er_in = torch.empty((S_max, H), device=dev).uniform_()
        send = torch.empty((S_max, pld), device=dev)
        part = torch.empty((parts, pld), device=dev)
        pack = pp.pack(Cz)
        desc = "8 heads x %d %s" % (Dp, "head mean" if last else "ELU")
        t = timed(lambda: gat_part(pp, dp, z, el, er_in, H, Dp, pack, send, part), reps)
        row("gat", k, desc, "part pack %d" % pack, t, (Er * (Cz + H) + S * H + S * pld) * 4)
        del z, el, send, part
        recv = torch.empty((R_max, pld), device=dev).uniform_()
        recv.view(-1, pld)[:, Cz + H:Cz + 2 * H] += 0.5                    # s > 0
        bias = torch.zeros((Cz,), device=dev)
        out = torch.empty((m, C if last else Cz), device=dev)
        t = timed(lambda: gat_merge(pp, dp, recv, H, Dp, bias, last, C if last else 0, out), reps)
        row("gat", k, desc, "merge", t, (R * pld + m * (C if last else Cz)) * 4,
            {"exchange_bytes": out_rows * (pld + H) * 4})
        lines.append("  gat  layer %d exchange: %d rows x (%d + %d) floats = %.3f GB sent to the other ranks (er out, "
                     "states back; not measured)" % (k, out_rows, pld, H, out_rows * (pld + H) * 4 / 1e9))
        del recv, out
    res["ranks"].append({"P": P, "n_own": n_own, "local_edges": Er, "sub_rows": S, "sent_rows": out_rows,
                         "recv_rows": R, "layers": layers})
    infer.release()


def whole_calls(indptr, indices, dev, F, C, lines, res):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("gloo", rank=0, world_size=1)
    comm = splitgnn.DistComm(device=dev)
    n = indptr.shape[0] - 1
    feats = torch.rand((n, F), device=dev)
    labels = torch.randint(0, C, (n,), device=dev)
    nodes = np.sort(np.random.default_rng(0).permutation(n)[:n // 5])
    torch.manual_seed(0)
    models = {"sage": splitgnn.DistSAGEModel(F, 256, C, n_layers=3).to(dev),
              "gat": splitgnn.DistGATModel(F, 32, C, heads=8, n_layers=3).to(dev)}
    for name, model in models.items():
        ts = {}
        for how in ("single", "rank"):
            def call():
                if how == "single":
                    return infer.evaluate(model, indptr, indices, feats, nodes, labels)
                return infer.evaluate_parts(model, indptr, indices, feats, comm, nodes, labels)
            call()
            w = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev = call()
                torch.cuda.synchronize()
                w.append(time.perf_counter() - t0)
            ts[how] = (float(np.median(w)), ev)
        same = ts["single"][1] == ts["rank"][1]
        lines.append("%-4s evaluate of %d nodes: single process %.1f ms, gloo world-of-one rank path %.1f ms (exchanges "
                     "staged through host memory), results %s" % (name, nodes.shape[0], ts["single"][0] * 1e3,
                                                                  ts["rank"][0] * 1e3, "identical" if same else "DIFFER"))
        res["whole"][name] = {"single_s": ts["single"][0], "rank_world_of_one_s": ts["rank"][0], "identical": same}
    infer.release()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default="2,4,8")
    ap.add_argument("--no-whole", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, d, F, C = l0.PRESETS["products-like"]
    t0 = time.time()
    indptr, indices = l0.synth_graph(n, d, seed=0)
    lines = ["products-like: N %d, %d CSR entries, graph %.1f s; kernel times: device events, median of %d after a warm-up"
             % (n, indices.shape[0], time.time() - t0, a.reps)]
    res = {"ranks": [], "whole": {}}
    for P in (int(x) for x in a.parts.split(",")):
        rank_zero(indptr, indices, P, dev, F, C, a.reps, lines, res)
    if not a.no_whole:
        whole_calls(indptr, indices, dev, F, C, lines, res)
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
