"""What weight decay and gradient-norm clipping cost the optimizer step (aggr.Adam.step on one flat gradient buffer), at
the parameter shapes of bench.py's end-to-end models: GraphSAGE (3 layers, features 100, hidden 256, 47 classes) and the
attention model (3 layers, 8 heads of 32).

    python profiles/optim_bench.py [--reps 7] [--steps 200] [--out FILE]

Four optimizers over copies of the same parameters, alternating, `--steps` back-to-back step() calls between two device
events per timed run (the time per step is then the larger of the kernels' time and the host's enqueue time of one or two
launches: what a training step pays), median (min, max) of `--reps` runs:
  default      csl_adam_f32, one launch (the parent commit's optimizer, the code the default trainer still runs)
  decay        csl_adamw_f32, weight matrices decayed, no clipping: one launch (k_adamw)
  clip         csl_adamw_f32, max_grad_norm = 1: two launches (k_grad_sqsum, k_adamw)
  clip+decay   both: two launches
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "occ-gnn_amd"))

from cslicer import aggr, splitgnn  # noqa: E402

MODES = (("default", {}, 1), ("decay", dict(weight_decay=5e-4), 1), ("clip", dict(max_grad_norm=1.0), 2),
         ("clip+decay", dict(weight_decay=5e-4, max_grad_norm=1.0), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    models = (("GraphSAGE 100-256-256-47", lambda: splitgnn.DistSAGEModel(100, 256, 47, n_layers=3)),
              ("GAT 100-8x32-8x32-47", lambda: splitgnn.DistGATModel(100, 32, 47, heads=8, n_layers=3)))
    for name, make in models:
        torch.manual_seed(0)
        base = [p.detach().cuda().contiguous() for p in make().parameters()]
        total = sum(p.numel() for p in base)
        flat = torch.randn(total, device="cuda") * 1e-2
        opts = []
        for _, kw, _ in MODES:
            params = [p.clone() for p in base]
            if "weight_decay" in kw:
                kw = dict(kw, weight_decay=[kw["weight_decay"] if p.dim() >= 2 else 0.0 for p in params])
            opts.append(aggr.Adam(params, lr=1e-3, **kw))
        for o in opts:                               # warm-up: code objects loaded, every shape seen
            for _ in range(20):
                o.step(flat_grads=flat)
        torch.cuda.synchronize()
        ts = [[] for _ in MODES]
        for _ in range(a.reps):
            for k, o in enumerate(opts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _s in range(a.steps):
                    o.step(flat_grads=flat)
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
        lines += ["%s: %d tensors, %d parameters (%d chunks of 1,024); %d steps per run, us per step, median (min, max) of %d runs"
                  % (name, len(base), total, sum((p.numel() + 1023) // 1024 for p in base), a.steps, a.reps)]
        ref = np.median(ts[0])
        for (mode, _, launches), t in zip(MODES, ts):
            lines.append("  %-11s %d launch%s  %7.2f us (%.2f, %.2f)  %+6.2f us on the default"
                         % (mode, launches, " " if launches == 1 else "es", np.median(t), min(t), max(t), np.median(t) - ref))
        assert all(int(o.skipped) == 0 for o in opts)
        lines.append("")
    text = "\n".join(lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
