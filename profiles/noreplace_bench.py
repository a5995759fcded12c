"""What CSL_FLAG_NO_REPLACE costs the slicer on bench.py's default workload, in graph mode: the products-shaped synthetic
graph (2.45 M nodes, mean degree 50.5, graph seed 0), fanout 15/10/5, batch 1024, 4 parts, S = 128 minibatches per
round, 3 result slots.  Both samplers in one process, on the same node order.

    python profiles/noreplace_bench.py [--rounds 20] [--reps 3] [--out FILE]

Two figures per sampler:
  * minibatches/s of the whole slicer: `--rounds` rounds back to back after a warm-up, wall clock around submit..sync,
    median (min, max) of `--reps` runs, the two samplers alternating;
  * k_sample microseconds per launch, per layer, by device events (csl_timing_enable) on an engine with
    CSL_FLAG_SERIAL_ROUNDS, so that a neighbouring round does not stretch a kernel.  The engine's timers add up a
    kernel's launches over the layers, so layer l is the difference between an engine of l + 1 layers and one of l
    layers (fanout prefixes 15, 15/10, 15/10/5: the same seeds and the same generator give every prefix the same
    frontiers layer for layer).
Without replacement the deeper frontiers are not the same ones -- distinct picks reach more distinct nodes -- so the
frontier sizes are printed beside the times: a difference per launch is the map's cost plus that of the larger frontier.
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


def engine(indptr, indices, perm, fan, flags):
    e = _abi.Engine(indptr, indices, n_parts=P, fanouts=fan, max_batch=B, n_streams=S, n_slots=SLOTS,
                    mode=_abi.MODE_GRAPH, flags=flags)
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
    perm = np.random.default_rng(1).permutation(N).astype(np.int64)
    n_rounds_epoch, _ = shard.rounds_per_epoch(N, B, S)
    lines = ["products-like synthetic: N %d, E %d, fanout %s, batch %d, %d parts, S %d, graph mode (graph %.1f s)"
             % (N, indices.shape[0], "/".join(map(str, FAN)), B, P, S, time.time() - t0)]
    kinds = (("with replacement", 0), ("without (CSL_FLAG_NO_REPLACE)", _abi.FLAG_NO_REPLACE))
    # ---- whole slicer, minibatches/s
    engs = [engine(indptr, indices, perm, FAN, fl) for _, fl in kinds]
    for e in engs:
        run(e, n_rounds_epoch, 0, a.warmup)
    rates = [[], []]
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
        lines.append("  %-32s %9.0f minibatches/s (%.0f, %.0f)" % (name, np.median(r), min(r), max(r)))
    lines.append("  ratio of the medians (without / with): %.3f" % (np.median(rates[1]) / np.median(rates[0])))
    lines.append("  frontiers of one minibatch (seeds, layer 1, layer 2, input nodes): %s | %s"
                 % (" ".join(map(str, sizes[0])), " ".join(map(str, sizes[1]))))
    # ---- k_sample per launch and layer
    per = []
    for _, fl in kinds:
        tot = [0.0]
        for L in range(1, len(FAN) + 1):
            e = engine(indptr, indices, perm, FAN[:L], fl | _abi.FLAG_SERIAL_ROUNDS)
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
    lines.append("k_sample, microseconds per launch (one launch = one layer of %d minibatches), %d rounds, serial rounds:"
                 % (S, a.rounds))
    lines.append("  %-8s %18s %18s %8s" % ("layer", "with replacement", "without", "ratio"))
    for l in range(len(FAN)):
        lines.append("  %-8s %18.1f %18.1f %8.2f" % ("%d (f=%d)" % (l, FAN[l]), per[0][l], per[1][l], per[1][l] / per[0][l]))
    lines.append("  %-8s %18.1f %18.1f %8.2f" % ("sum", sum(per[0]), sum(per[1]), sum(per[1]) / sum(per[0])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
