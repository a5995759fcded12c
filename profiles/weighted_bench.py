"""What edge-weighted sampling (csl_set_edge_cdf) costs the slicer on bench.py's default workload, in graph mode: the
products-shaped synthetic graph (2.45 M nodes, mean degree 50.5, graph seed 0), fanout 15/10/5, batch 1024, 4 parts,
S = 128 minibatches per round, 3 result slots.  Three samplers in one process, on the same node order: the default
(uniform, `k_sample`), and `k_sample_weighted` with two tables --

  * inv-degree: w(v <- u) = 1 / max(deg(u), 1), quantised by l0.edge_cdf: the scheme that keeps hubs out of the deeper
    frontiers, so the frontiers are other frontiers;
  * all-ones: the integer table cum[off + i] = i + 1, the uniform distribution through the search: the same frontiers in
    distribution as the default, so the difference per launch is the search's own cost.

    python profiles/weighted_bench.py [--rounds 20] [--reps 3] [--out FILE]

Two figures per sampler, as profiles/noreplace_bench.py takes them:
  * minibatches/s of the whole slicer: `--rounds` rounds back to back after a warm-up, wall clock around submit..sync,
    median (min, max) of `--reps` runs, the samplers alternating;
  * k_sample microseconds per launch, per layer, by device events (csl_timing_enable; the weighted kernel is timed in
    k_sample's slot) on an engine with CSL_FLAG_SERIAL_ROUNDS.  The engine's timers add up a kernel's launches over the
    layers, so layer l is the difference between an engine of l + 1 layers and one of l layers (fanout prefixes 15,
    15/10, 15/10/5: the same seeds, generator and table give every prefix the same frontiers layer for layer).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "occ-gnn_amd"))

from cslicer import _abi, l0, shard  # noqa: E402

N, DEG, FAN, B, P, S, SLOTS = 2_449_029, 50.5, (15, 10, 5), 1024, 4, 128, 3


def engine(indptr, indices, perm, fan, cum, flags=0):
    e = _abi.Engine(indptr, indices, n_parts=P, fanouts=fan, max_batch=B, n_streams=S, n_slots=SLOTS,
                    mode=_abi.MODE_GRAPH, flags=flags)
    if cum is not None:
        e.set_edge_cdf(cum)
    e.set_nodes(perm)
    return e


def run(e, n_rounds_epoch, first, count):
    for k in range(first, first + count):
        lo, nb = shard.batches_of_round(shard.round_of(k, 0, 1, n_rounds_epoch), S)
        e.submit_round(lo, B, nb, slot=k % SLOTS)
    e.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _abi.load()
    t0 = time.time()
    indptr, indices = l0.synth_graph(N, DEG, seed=0)
    t1 = time.time()
    deg = np.diff(indptr)
    ones = (np.arange(indices.shape[0], dtype=np.int64) - np.repeat(indptr[:-1], deg) + 1).astype(np.uint32)
    inv = l0.edge_cdf(indptr, l0.inv_degree_weights(indptr, indices))
    perm = np.random.default_rng(1).permutation(N).astype(np.int64)
    n_rounds_epoch, _ = shard.rounds_per_epoch(N, B, S)
    lines = ["products-like synthetic: N %d, E %d, fanout %s, batch %d, %d parts, S %d, graph mode (graph %.1f s, tables %.1f s)"
             % (N, indices.shape[0], "/".join(map(str, FAN)), B, P, S, t1 - t0, time.time() - t1)]
    kinds = (("uniform (k_sample)", None), ("weighted, inv-degree", inv), ("weighted, all-ones", ones))
    # ---- whole slicer, minibatches/s
    engs = [engine(indptr, indices, perm, FAN, cum) for _, cum in kinds]
    for e in engs:
        run(e, n_rounds_epoch, 0, a.warmup)
    rates = [[] for _ in kinds]
    at = a.warmup
    for _ in range(a.reps):
        for k, e in enumerate(engs):
            t = time.perf_counter()
            run(e, n_rounds_epoch, at, a.rounds)
            rates[k].append(a.rounds * S / (time.perf_counter() - t))
        at += a.rounds
    sizes = []
    for e in engs:
        m = e.meta(0, (at - 1) % SLOTS)
        sizes.append([int(m.layer[l].frontier) for l in range(len(FAN))] + [int(m.layer[len(FAN) - 1].next_frontier)])
        e.close()
    lines.append("")
    lines.append("slicer, %d rounds of %d minibatches, median (min, max) of %d runs:" % (a.rounds, S, a.reps))
    for (name, _), r in zip(kinds, rates):
        lines.append("  %-24s %9.0f minibatches/s (%.0f, %.0f)   ratio to uniform %.3f"
                     % (name, np.median(r), min(r), max(r), np.median(r) / np.median(rates[0])))
    lines.append("  frontiers of one minibatch (seeds, layer 1, layer 2, input nodes):")
    for (name, _), sz in zip(kinds, sizes):
        lines.append("    %-24s %s" % (name, " ".join(map(str, sz))))
    # ---- k_sample per launch and layer
    per = []
    for _, cum in kinds:
        tot = [0.0]
        for L in range(1, len(FAN) + 1):
            e = engine(indptr, indices, perm, FAN[:L], cum, _abi.FLAG_SERIAL_ROUNDS)
            run(e, n_rounds_epoch, 0, a.warmup)
            e.timing_enable(True)
            run(e, n_rounds_epoch, a.warmup, a.rounds)
            ms, n = e.timing_read()["k_sample"]
            e.timing_enable(False)
            e.close()
            assert n == a.rounds * L
            tot.append(ms * 1e3 / a.rounds)
        per.append([tot[l + 1] - tot[l] for l in range(len(FAN))])
    lines.append("")
    lines.append("k_sample / k_sample_weighted, microseconds per launch (one launch = one layer of %d minibatches), %d rounds, "
                 "serial rounds:" % (S, a.rounds))
    lines.append("  %-8s %10s %12s %8s %12s %8s" % ("layer", "uniform", "inv-degree", "ratio", "all-ones", "ratio"))
    rows = [("%d (f=%d)" % (l, FAN[l]), [p[l] for p in per]) for l in range(len(FAN))] + [("sum", [sum(p) for p in per])]
    for name, (u, i, o) in rows:
        lines.append("  %-8s %10.1f %12.1f %8.2f %12.1f %8.2f" % (name, u, i, i / u, o, o / u))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
