"""CPU-side checks of split-parallel full-neighbour inference (cslicer.infer.full_inference_parts): the C ABI of
include/cslicer_infer_parts.h (symbols, argument checks that return before anything reaches a GPU), the per-rank
exchange plan's invariants, and a float64 restatement of the whole split computation, driven by the plans of every
rank, against tests/infer_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import infer_ref
from cslicer import infer, splitgnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = infer.SEG


def test_header_matches_binding_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_infer_parts.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src)))
    assert len(names) == 4
    assert names == sorted(infer.PARTS_SYMBOLS)
    L = infer._lib()
    for n in names:
        assert hasattr(L, n)
    # the single-process header keeps its five entry points
    src1 = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_infer.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src1))) == sorted(infer.SYMBOLS)


def test_bad_arguments_are_refused_without_a_gpu():
    L = infer._lib()
    null, st = C.c_void_p(0), C.c_void_p(0)
    fake = C.c_void_p(1 << 20)        # never dereferenced: every call below fails its checks first
    odd = C.c_void_p((1 << 20) + 4)   # not 16-byte aligned
    sp = L.csl_infer_sage_part_f32
    # W not a multiple of 4, W < 4, ldy < W, pack < 1, negative counts, missing plan / hub scratch, misaligned rows
    assert sp(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 10, 1, null, fake, st) == -1
    assert sp(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 0, 1, null, fake, st) == -1
    assert sp(fake, fake, fake, 10, null, 0, 0, 0, fake, 96, 100, 1, null, fake, st) == -1
    assert sp(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 100, 0, null, fake, st) == -1
    assert sp(fake, fake, fake, -1, null, 0, 0, 0, fake, 100, 100, 1, null, fake, st) == -1
    assert sp(fake, fake, null, 10, null, 0, 0, 0, fake, 100, 100, 1, null, fake, st) == -1
    assert sp(fake, fake, fake, 10, fake, 3, 0, 0, fake, 100, 100, 1, null, fake, st) == -1
    assert sp(fake, fake, fake, 10, null, 0, 0, 0, odd, 100, 100, 1, null, fake, st) == -1
    assert sp(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 100, 1, null, null, st) == -1
    assert sp(null, null, null, 0, null, 0, 0, 0, null, 100, 100, 1, null, null, st) == 0    # nothing to do
    sm = L.csl_infer_sage_merge_f32
    # P < 1, ldo too small for the operand, missing lists / received rows / records, misaligned output, n < 0
    assert sm(fake, fake, 10, 0, fake, fake, 100, 100, 0, null, 0, fake, 200, st) == -1
    assert sm(fake, fake, 10, 2, fake, fake, 100, 100, 0, null, 0, fake, 100, st) == -1
    assert sm(fake, null, 10, 2, fake, fake, 100, 100, 0, null, 0, fake, 200, st) == -1
    assert sm(fake, fake, 10, 2, null, fake, 100, 100, 0, null, 0, fake, 200, st) == -1
    assert sm(null, fake, 10, 2, fake, fake, 100, 100, 0, null, 0, fake, 200, st) == -1
    assert sm(fake, fake, 10, 2, fake, fake, 100, 100, 1, null, 0, odd, 100, st) == -1
    assert sm(fake, fake, -1, 2, fake, fake, 100, 100, 1, null, 0, fake, 100, st) == -1
    assert sm(null, null, 0, 2, null, null, 100, 100, 1, null, 0, null, 100, st) == 0
    gp = L.csl_infer_gat_part_f32
    # D % 4, H < 1, missing er rows, pack < 1
    assert gp(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 8, 6, 0.2, 1, null, fake, st) == -1
    assert gp(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 0, 8, 0.2, 1, null, fake, st) == -1
    assert gp(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, null, 8, 8, 0.2, 1, null, fake, st) == -1
    assert gp(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 8, 8, 0.2, 0, null, fake, st) == -1
    gm = L.csl_infer_gat_merge_f32
    # a last layer over 4,096 columns, n_cls > D, a hidden ldo too small, P < 1
    assert gm(fake, 10, 2, fake, 8, 1024, null, 1, 5, fake, 5, st) == -1
    assert gm(fake, 10, 2, fake, 8, 48, null, 1, 49, fake, 49, st) == -1
    assert gm(fake, 10, 2, fake, 8, 32, null, 0, 0, fake, 128, st) == -1
    assert gm(fake, 10, 0, fake, 8, 32, null, 0, 0, fake, 256, st) == -1
    assert gm(null, 0, 2, null, 8, 32, null, 0, 0, null, 256, st) == 0


def _csr(degs, seed=0):
    rng = np.random.default_rng(seed)
    degs = np.asarray(degs, dtype=np.int64)
    indptr = np.zeros(len(degs) + 1, dtype=np.int64)
    np.cumsum(degs, out=indptr[1:])
    indices = rng.integers(0, len(degs), size=int(indptr[-1]))
    rows = np.repeat(np.arange(len(degs)), degs)
    sl = rng.random(indices.shape[0]) < 0.05
    indices[sl] = rows[sl]                                   # self loops (not neighbours)
    return indptr, indices


def _graph(n=400, seed=1):
    """rows of 0, 1, SEG - 1, SEG, SEG + 1 and 3 SEG + 7 entries, the rest 0..12"""
    rng = np.random.default_rng(seed)
    degs = rng.integers(0, 13, n)
    degs[:6] = [0, 1, S - 1, S, S + 1, 3 * S + 7]
    return _csr(degs, seed)


def _tables(n, P, seed=2):
    rng = np.random.default_rng(seed)
    empty = rng.integers(0, P, n).astype(np.int32)
    empty[empty == P - 1] = 0                                # the last part owns nothing
    return {"mod": None, "random": rng.integers(0, P, n).astype(np.int32), "empty": empty,
            "all": np.zeros(n, dtype=np.int32)}


@pytest.mark.parametrize("P,table", [(P, t) for P in (1, 2, 3, 5) for t in ("mod", "random", "empty", "all")])
def test_plan_invariants(P, table):
    indptr, indices = _graph()
    n = indptr.shape[0] - 1
    owner = infer.owner_table(n, P, _tables(n, P)[table])
    ip, ix = infer.neighbour_csr(indptr, indices)
    rng = np.random.default_rng(3)
    for nodes in (None, rng.choice(n, 150, replace=True)):
        for chunk_rows in (64, 1000):
            rgs = [infer.RankGraph(indptr, indices, owner, P, r) for r in range(P)]
            plans = [rg.plan(chunk_rows, nodes) for rg in rgs]
            D = np.arange(n) if nodes is None else nodes
            # the chunk sequence: the same on every rank, from replicated data only
            assert len({p.n_chunks for p in plans}) == 1 and plans[0].n_chunks == (len(D) + chunk_rows - 1) // chunk_rows
            # every neighbour edge of every destination is in exactly one rank's sub-CSR: that of its source's owner
            want = {}
            for k, v in enumerate(D):
                for u in ix[ip[v]:ip[v + 1]]:
                    want.setdefault((k, int(owner[u])), []).append(int(u))
            got = {}
            for r, (rg, pp) in enumerate(zip(rgs, plans)):
                # sub-rows: the destinations with a neighbour r owns, in (chunk, owner, position) order
                kk = [k for k in range(len(D)) if any(owner[u] == r for u in ix[ip[D[k]]:ip[D[k] + 1]])]
                kk.sort(key=lambda k: (k // chunk_rows, int(owner[D[k]]), k))
                assert [int(D[k]) for k in kk] == [int(v) for v in pp.sub_nodes]
                for i, k in enumerate(kk):
                    got[(k, r)] = rg.own[pp.sub_ix[pp.sub_ip[i]:pp.sub_ip[i + 1]]].tolist()
                for c in range(pp.n_chunks):
                    sub = [k for k in kk if k // chunk_rows == c]
                    assert pp.sub_first[c + 1] - pp.sub_first[c] == len(sub)
                    assert pp.sub_counts[c].tolist() == [sum(1 for k in sub if owner[D[k]] == p) for p in range(P)]
                # hubs are cut as in build_plan
                ref = infer.build_plan(pp.sub_ip)
                for key in ("items", "hubs", "item_first", "part_first"):
                    assert np.array_equal(pp.work[key], ref[key])
            assert got == want
            # sender counts equal receiver counts per chunk and peer
            for q in range(P):
                for p in range(P):
                    assert np.array_equal(plans[q].sub_counts[:, p], plans[p].own_counts[:, q])
            # merge lists: own destinations in position order, one row per rank holding a neighbour, in rank order,
            # together every row of the chunk's receive buffer once
            for r, pp in enumerate(plans):
                own_k = np.flatnonzero(owner[D] == r)
                assert np.array_equal(pp.opos, own_k)
                for c in range(pp.n_chunks):
                    o0, o1 = pp.own_first[c], pp.own_first[c + 1]
                    ml = pp.ml[o0:o1]
                    live = ml[ml >= 0]
                    assert sorted(live.tolist()) == list(range(pp.recv_first[c + 1] - pp.recv_first[c]))
                    for i in range(o1 - o0):
                        k = own_k[o0 + i]
                        has = [q for q in range(P) if ml[i, q] >= 0]
                        assert has == sorted({int(owner[u]) for u in ix[ip[D[k]]:ip[D[k] + 1]]})
                        seg = np.r_[0, np.cumsum(pp.own_counts[c])]
                        assert all(seg[q] <= ml[i, q] < seg[q + 1] for q in has)      # rank q's segment
                    assert np.array_equal(pp.dst[o0:o1, 1], np.diff(ip)[D[own_k[o0:o1]]])
                    assert np.array_equal(pp.dst[o0:o1, 0], rgs[r].lrow[D[own_k[o0:o1]]])


def _route(sub_first, sub_counts, c, rows_of, width):
    """the chunk's all_to_all in Python: rows_of[q] holds rank q's send rows of chunk c (grouped by receiver, counts
    sub_counts[q][c]) -> the rows each rank receives (segments by sender, in rank order)"""
    P = len(rows_of)
    out = []
    for r in range(P):
        segs = []
        for q in range(P):
            off = int(sub_counts[q][c, :r].sum())
            segs.append(rows_of[q][off:off + sub_counts[q][c, r]])
        out.append(np.concatenate(segs, 0) if segs else np.zeros((0, width)))
    return out


def _simulate(model, indptr, indices, feats, owner, P, nodes, chunk_rows):
    """float64 restatement of full_inference_parts on all P ranks, driven by their plans: per rank, partial sums / states
    over its sub-CSR, routed by the plan's counts, merged along its merge lists.  Returns the logits of every rank."""
    rgs = [infer.RankGraph(indptr, indices, owner, P, r) for r in range(P)]
    h = [np.asarray(feats, dtype=np.float64)[rg.own] for rg in rgs]
    sage = isinstance(model, splitgnn.DistSAGEModel)
    L = len(model.convs)
    for k, conv in enumerate(model.convs):
        last = k + 1 == L
        plans = [rg.plan(chunk_rows, nodes if last else None) for rg in rgs]
        subc = [pp.sub_counts for pp in plans]
        ownc = [pp.own_counts for pp in plans]
        outs = [[] for _ in range(P)]
        if sage:
            W = conv.fc.weight.detach().double().numpy()
            b = conv.fc.bias.detach().double().numpy()
            fin = W.shape[1] // 2
        else:
            H, Dh = conv.H, conv.D
            z = [x @ conv.fc.weight.detach().double().numpy().T for x in h]
            el = [(zz.reshape(-1, H, Dh) * conv.attn_l.detach().double().numpy()).sum(-1) for zz in z]
            er = [(zz.reshape(-1, H, Dh) * conv.attn_r.detach().double().numpy()).sum(-1) for zz in z]
            bias = conv.bias.detach().double().numpy().reshape(H, Dh)
        for c in range(plans[0].n_chunks):
            if sage:
                part = []
                for q, pp in enumerate(plans):
                    rows = range(pp.sub_first[c], pp.sub_first[c + 1])
                    part.append(np.stack([h[q][pp.sub_ix[pp.sub_ip[i]:pp.sub_ip[i + 1]]].sum(0) for i in rows])
                                if len(rows) else np.zeros((0, fin)))
                recv = _route(None, subc, c, part, fin)
                for r, pp in enumerate(plans):
                    for i in range(pp.own_first[c], pp.own_first[c + 1]):
                        acc = np.zeros(fin)
                        for j in pp.ml[i]:
                            if j >= 0:
                                acc = acc + recv[r][j]
                        self_row, deg = pp.dst[i]
                        y = np.concatenate([h[r][self_row], acc / max(deg, 1)]) @ W.T + b
                        outs[r].append(y if last else np.maximum(y, 0))
            else:
                # er of every owned destination out to the ranks holding its neighbours, then the states back
                er_out = [er[r][pp.er_src[pp.recv_first[c]:pp.recv_first[c + 1]]] for r, pp in enumerate(plans)]
                er_in = _route(None, ownc, c, er_out, H)
                part = []
                for q, pp in enumerate(plans):
                    s0 = pp.sub_first[c]
                    st = []
                    for i in range(s0, pp.sub_first[c + 1]):
                        src = pp.sub_ix[pp.sub_ip[i]:pp.sub_ip[i + 1]]
                        sc = el[q][src] + er_in[q][i - s0]
                        sc = np.where(sc > 0, sc, sc * conv.slope)
                        m = sc.max(0)
                        p_ = np.exp(sc - m)
                        n_ = (p_[:, :, None] * z[q][src].reshape(-1, H, Dh)).sum(0)
                        st.append(np.concatenate([n_.reshape(-1), m, p_.sum(0)]))
                    part.append(np.stack(st) if st else np.zeros((0, H * Dh + 2 * H)))
                recv = _route(None, subc, c, part, H * Dh + 2 * H)
                for r, pp in enumerate(plans):
                    for i in range(pp.own_first[c], pp.own_first[c + 1]):
                        m, s, n_ = np.full(H, -1e300), np.zeros(H), np.zeros((H, Dh))
                        for j in pp.ml[i]:
                            if j >= 0:
                                row = recv[r][j]
                                m2, s2, n2 = row[H * Dh:H * Dh + H], row[H * Dh + H:], row[:H * Dh].reshape(H, Dh)
                                M = np.maximum(m, m2)
                                a, b2 = np.exp(m - M), np.exp(m2 - M)
                                s, n_, m = s * a + s2 * b2, n_ * a[:, None] + n2 * b2[:, None], M
                        y = n_ / np.where(s > 0, s, 1)[:, None] + bias
                        outs[r].append(y.mean(0)[:model.n_classes] if last else
                                       np.where(y > 0, y, np.expm1(np.minimum(y, 0))).reshape(-1))
        width = conv.fc.weight.shape[0] if sage else (model.n_classes if last else conv.H * conv.D)
        h = [np.stack(o) if o else np.zeros((0, width)) for o in outs]
    return h


@pytest.mark.parametrize("kind", ["sage_agg", "sage_proj", "gat"])
@pytest.mark.parametrize("P,table", [(1, "mod"), (2, "mod"), (3, "random"), (3, "empty"), (5, "all")])
def test_float64_restatement_matches_reference(kind, P, table):
    indptr, indices = _csr(np.random.default_rng(4).integers(0, 9, 150), seed=4)
    n = indptr.shape[0] - 1
    owner = infer.owner_table(n, P, _tables(n, P)[table])
    torch.manual_seed(5)
    if kind == "sage_agg":
        model, F = splitgnn.DistSAGEModel(6, 12, 5, n_layers=2), 6          # 6 -> 12 aggregate first
    elif kind == "sage_proj":
        model, F = splitgnn.DistSAGEModel(12, 4, 3, n_layers=2), 12         # 12 -> 4 project first
    else:
        model, F = splitgnn.DistGATModel(6, 4, 5, heads=3, n_layers=2), 6
    feats = np.random.default_rng(6).random((n, F))
    nodes = np.random.default_rng(7).choice(n, 60, replace=False)
    got = _simulate(model, indptr, indices, feats, owner, P, nodes, chunk_rows=37)
    want = infer_ref.model(model, torch.as_tensor(feats), indptr, indices, nodes=nodes).numpy()
    for r in range(P):
        mine = owner[nodes] == r
        assert got[r].shape[0] == int(mine.sum())
        if mine.any():
            np.testing.assert_allclose(got[r], want[mine], rtol=0, atol=1e-12 * max(np.abs(want).max(), 1))


def test_owns_and_owner_table():
    assert infer.owns(10, 3, 1, [0, 1, 4, 9, 7]).tolist() == [False, True, True, False, True]
    t = np.array([2, 0, 1, 1], dtype=np.int32)
    assert infer.owns(4, 3, 1, [3, 0, 2], owner=t).tolist() == [True, False, True]
    assert infer.owner_table(5, 2).tolist() == [0, 1, 0, 1, 0]
    with pytest.raises(ValueError):
        infer.owner_table(4, 2, np.array([0, 1, 2, 0]))
    with pytest.raises(ValueError):
        infer.owner_table(4, 2, np.array([0, 1, 0]))


def test_release_drops_rank_plans():
    indptr, indices = _csr([3, 0, 2, 5, 1])
    owner = infer.owner_table(5, 2)
    rg = infer.rank_graph(indptr, indices, owner, 2, 1)
    assert infer.rank_graph(indptr, indices, owner, 2, 1) is rg
    assert infer.rank_graph(indptr, indices, owner, 2, 0) is not rg
    infer.release(indptr, indices)
    assert not infer._RANKS
