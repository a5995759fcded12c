"""Sequential restatement of edge-weighted neighbour sampling (csl_set_edge_cdf, include/cslicer_hip.h): noreplace_ref's
GraphRef with the map from a row's draws to its edge positions replaced by the table lookup.  TEST INFRASTRUCTURE:
tests/test_weighted_cpu.py pins cum=None to GraphRef(replace=True), which tests/test_noreplace_cpu.py pins to the C
oracle; the GPU tests then trust the weighted form."""
from bisect import bisect_right

import numpy as np

from noreplace_ref import GraphRef


def weighted_pick(word, row_cum):
    """edge position of one 32-bit word in a row whose running integer weights are `row_cum` (a list of ints):
    x = (word * T) >> 32, the smallest i with row_cum[i] > x; a row with T == 0 takes word % deg"""
    T = row_cum[-1]
    if T == 0:
        return int(word) % len(row_cum)
    return bisect_right(row_cum, (int(word) * T) >> 32)


class WeightedGraphRef(GraphRef):
    """GraphRef drawing with replacement through a per-edge table `cum` (uint32 [E], per row the running sum of the
    integer weights); cum=None: the parent's draw."""

    def __init__(self, indptr, indices, n_parts, fanouts, cum=None, workload=None, seed=5489):
        super().__init__(indptr, indices, n_parts, fanouts, workload=workload, seed=seed, replace=True)
        self.cum = None if cum is None else np.asarray(cum, dtype=np.uint32)
        if self.cum is not None:
            assert self.cum.shape == self.indices.shape

    def neighbour_sample(self, nd1, fanout, picks_out=None):
        if self.cum is None:
            return super().neighbour_sample(nd1, fanout, picks_out)
        off, deg = int(self.indptr[nd1]), int(self.indptr[nd1 + 1] - self.indptr[nd1])
        if deg < fanout:          # (all its edges in order, zero-weight ones included)
            return [nd1] + [int(x) for x in self.indices[off:off + deg]]
        words = [self.rng.next() for _ in range(fanout)]
        self.draws_total += fanout
        row = [int(c) for c in self.cum[off:off + deg]]
        picks = [weighted_pick(w, row) for w in words]
        if picks_out is not None:
            picks_out.append((deg, picks))
        return [nd1] + [int(self.indices[off + p]) for p in picks]
