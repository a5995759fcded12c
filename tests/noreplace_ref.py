"""Sequential restatement, in plain Python, of the graph-mode specification (oracle/cslicer_oracle.c:
orc_neighbour_sample, the frontier rule of orc_slice_layer, orc_graph_layer) with one switch the C oracle does not
have: replace=False maps a row's draws to edge positions by Floyd's subset algorithm (CSL_FLAG_NO_REPLACE,
include/cslicer_hip.h).  TEST INFRASTRUCTURE: tests/test_noreplace_cpu.py pins replace=True to the C oracle list for
list; the GPU tests then trust replace=False."""
import numpy as np

GKEYS = ["in_nodes", "out_nodes", "indptr", "indices", "owned_out_nodes", "self_ids_in", "self_ids_out",
         "owned_degree"]


class MT19937Words:
    """std::mt19937(seed)'s 32-bit outputs, one after the other (numpy's legacy seeding is init_genrand)."""

    def __init__(self, seed=5489):
        self._bg = np.random.MT19937()
        self._bg._legacy_seeding(int(seed))
        self._buf = np.zeros(0, dtype=np.uint64)
        self._at = 0

    def next(self):
        if self._at == self._buf.shape[0]:
            self._buf, self._at = self._bg.random_raw(4096), 0
        self._at += 1
        return int(self._buf[self._at - 1])


def floyd_picks(words, deg):
    """f = len(words) distinct edge positions of a row of `deg` >= f edges: for j = 0..f-1, J = deg - f + j,
    t = r_j % (J + 1), pick_j = J if t was picked before, else t."""
    f = len(words)
    picks = []
    for j, r in enumerate(words):
        J = deg - f + j
        t = int(r) % (J + 1)
        picks.append(J if t in picks else t)
    return picks


def crafted_graph(f, n=300, big=5000, seed=1):
    """rows of degree f-1, f, f+1, 2f in turn (distinct neighbours per row, no self loops) and one row of `big`
    edges (node 7, parallel edges among them)"""
    rng = np.random.default_rng(seed)
    rows = []
    for v in range(n):
        d = big if v == 7 else (f - 1, f, f + 1, 2 * f)[v % 4]
        if d <= n - 1:
            nb = rng.permutation(n - 1)[:d]
        else:
            nb = rng.integers(0, n - 1, d)
        rows.append(nb + (nb >= v))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int64)


def _a(x):
    return np.asarray(x, dtype=np.int64)


class GraphRef:
    """One worker (its own mt19937 position, kept from call to call) slicing in graph mode."""

    def __init__(self, indptr, indices, n_parts, fanouts, workload=None, seed=5489, replace=True):
        self.indptr, self.indices = _a(indptr), _a(indices)
        self.P, self.fanouts = int(n_parts), tuple(int(f) for f in fanouts)
        self.workload = None if workload is None else _a(workload)
        self.replace = bool(replace)
        self.rng = MT19937Words(seed)
        self.draws_total = 0
        self.picks = []    # last sample: per layer [(frontier index, deg, [edge positions])] of the rng consumers

    def owner(self, v):
        return int(self.workload[v]) if self.workload is not None else int(v) % self.P

    def neighbour_sample(self, nd1, fanout, picks_out=None):
        off, deg = int(self.indptr[nd1]), int(self.indptr[nd1 + 1] - self.indptr[nd1])
        if deg < fanout:
            return [nd1] + [int(x) for x in self.indices[off:off + deg]]
        words = [self.rng.next() for _ in range(fanout)]
        self.draws_total += fanout
        picks = [w % deg for w in words] if self.replace else floyd_picks(words, deg)
        if picks_out is not None:
            picks_out.append((deg, picks))
        return [nd1] + [int(self.indices[off + p]) for p in picks]

    def graph_layer(self, frontier, nbrs):
        P = self.P
        parts = []
        for g in range(P):
            rank, in_nodes = {}, []
            for nd1, nb in zip(frontier, nbrs):
                for j, nd2 in enumerate(nb):
                    take = (self.owner(nd1) == g) if j == 0 else (nd2 != nd1 and self.owner(nd2) == g)
                    if take and nd2 not in rank:
                        rank[nd2] = len(in_nodes)
                        in_nodes.append(nd2)
            b = {k: [] for k in GKEYS}
            b["in_nodes"], b["indptr"] = in_nodes, [0]
            for nd1, nb in zip(frontier, nbrs):
                own = self.owner(nd1) == g
                e0 = len(b["indices"])
                b["indices"] += [rank[nd2] for nd2 in nb[1:] if nd2 != nd1 and self.owner(nd2) == g]
                if own or len(b["indices"]) > e0:
                    b["out_nodes"].append(nd1)
                    b["indptr"].append(len(b["indices"]))
                    if own:
                        r = len(b["out_nodes"]) - 1
                        b["owned_out_nodes"].append(r)
                        b["self_ids_out"].append(r)
                        b["self_ids_in"].append(rank[nd1])
                        b["owned_degree"].append(sum(1 for nd2 in nb[1:] if nd2 != nd1))
            b["from_ids"] = [[] for _ in range(P)]
            b["to_ids"] = [[] for _ in range(P)]
            b["gpu_id"] = g
            parts.append(b)
        for p in range(P):
            row = {nd: r for r, nd in enumerate(parts[p]["out_nodes"])}
            for g in range(P):
                if g == p:
                    continue
                for r, nd1 in enumerate(parts[g]["out_nodes"]):
                    if self.owner(nd1) == p:
                        parts[g]["from_ids"][p].append(r)
                        parts[p]["to_ids"][g].append(row[nd1])
        for b in parts:
            for k in GKEYS:
                b[k] = _a(b[k])
            b["from_ids"] = [_a(x) for x in b["from_ids"]]
            b["to_ids"] = [_a(x) for x in b["to_ids"]]
        return parts

    def sample_graph(self, seeds):
        out = {"layers": [], "frontier": [], "nbr_counts": [], "nbr_flat": [], "draws": [], "sampled_edges": 0}
        self.picks = []
        frontier = [int(s) for s in np.asarray(seeds).reshape(-1)]
        for fanout in self.fanouts:
            d0, lp = self.draws_total, []
            nbrs, seen, nxt = [], set(), []
            for i, nd1 in enumerate(frontier):
                got = []
                nb = self.neighbour_sample(nd1, fanout, got)
                lp += [(i, deg, picks) for deg, picks in got]
                nbrs.append(nb)
                for nd2 in nb:                      # slicer.cpp:45-49: first occurrences, the node itself included
                    if nd2 not in seen:
                        seen.add(nd2)
                        nxt.append(nd2)
            self.picks.append(lp)
            out["frontier"].append(_a(frontier))
            out["nbr_counts"].append(_a([len(nb) for nb in nbrs]))
            out["nbr_flat"].append(_a([x for nb in nbrs for x in nb]))
            out["draws"].append(self.draws_total - d0)
            out["sampled_edges"] += sum(len(nb) - 1 for nb in nbrs)
            out["layers"].append(self.graph_layer(frontier, nbrs))
            frontier = nxt
        out["frontier"].append(_a(frontier))
        out["draws_total"] = self.draws_total
        return out
