"""Trainer.evaluate on a 16-bit feature table of the products-shaped preset (cslicer.l0.PRESETS["products-like"]), whole
call, wall clock: one process = one tree, so that two checkouts of the repository can be run alternately on one box.

    python profiles/eval16_ab.py [--pkg PATH/occ-gnn_amd] [--feature-dtype bfloat16] [--model sage] [--reps 7] [--tag NAME]

--pkg: the package directory of the tree to time (default: this tree's), with its library built.  Prints one line: the
median, min and max of `reps` evaluate() calls after a warm-up one (each ended by the device synchronisation its result
needs), and the rise of torch's allocated bytes over one call (the table itself is allocated before).
"""
import argparse
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "occ-gnn_amd"))
ap.add_argument("--feature-dtype", default="bfloat16")
ap.add_argument("--model", default="sage")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--nodes", type=int, default=200000)
ap.add_argument("--tag", default=None)
a = ap.parse_args()
sys.path.insert(0, a.pkg)

import torch  # noqa: E402

from cslicer import l0  # noqa: E402
from cslicer.train import Trainer  # noqa: E402


def main():
    n, d, F, C = l0.PRESETS["products-like"]
    indptr, indices = l0.synth_graph(n, d, seed=0)
    rng = np.random.default_rng(0)
    feats = torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(getattr(torch, a.feature_dtype))
    labels = rng.integers(0, C, n)
    tr = Trainer(indptr, indices, feats, labels, C, fanouts=(15, 10, 5), batch=1024, streams=8, hidden=256, model=a.model,
                 heads=8, feature_dtype=a.feature_dtype)
    del feats
    nodes = rng.permutation(n)[:a.nodes]
    ev = tr.evaluate(nodes)                                  # warm-up: the graph's device copy, the GEMM plans
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ev = tr.evaluate(nodes)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tr.evaluate(nodes)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("%s: %s %s table (%.1f MB), evaluate on %d nodes: %.2f ms (min %.2f, max %.2f of %d); torch's allocated bytes rise "
          "by %.1f MB; loss %.6f"
          % (a.tag or a.pkg, a.model, a.feature_dtype, tr.feat.numel() * tr.feat.element_size() / 1e6, a.nodes,
             float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3, a.reps, rise / 1e6, ev["loss"]), flush=True)
    tr.close()


if __name__ == "__main__":
    main()
