"""CPU-side checks of full-neighbour inference: the C ABI of include/cslicer_infer.h (symbols, argument checks that
return before anything reaches a GPU), the host-built work list, the L0 split files and the CLI option."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cslicer import _abi, infer, l0, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_binding_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_infer.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src)))
    assert len(names) == 5
    assert names == sorted(infer.SYMBOLS)
    L = infer._lib()
    for n in names:
        assert hasattr(L, n)
    assert L.csl_infer_seg() == infer.SEG
    assert L.csl_infer_gat_partial_ld(8, 32) == 256 + 16 and L.csl_infer_gat_partial_ld(3, 4) == 12 + 8


def test_bad_arguments_are_refused_without_a_gpu():
    L = infer._lib()
    null, st = C.c_void_p(0), C.c_void_p(0)
    fake = C.c_void_p(1 << 20)        # never dereferenced: every call below fails its checks first
    # W not a multiple of 4, W < 4, ldx / ldo too small, negative counts, missing plan
    assert L.csl_infer_sage_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 10, 0, null, 0, null, fake, 20, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 0, 0, null, 0, null, fake, 200, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 100, 0, null, 0, null, fake, 100, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, 100, 100, 1, null, 0, null, fake, 100, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, fake, -1, null, 0, 0, 0, fake, 100, 100, 0, null, 0, null, fake, 200, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, null, 10, null, 0, 0, 0, fake, 100, 100, 0, null, 0, null, fake, 200, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, fake, 10, fake, 3, 0, 0, fake, 100, 100, 0, null, 0, null, fake, 200, st) == -1
    assert L.csl_infer_sage_f32(fake, fake, fake, 10, null, 0, 0, 0, null, 100, 100, 0, null, 0, null, fake, 200, st) == -1
    # nothing to do: accepted without a launch
    assert L.csl_infer_sage_f32(null, null, null, 0, null, 0, 0, 0, null, 100, 100, 0, null, 0, null, null, 200, st) == 0
    # hub rows only, everything there but indptr: these hub passes read a row's degree from it (the one check the rank
    # path's csl_infer_*_part_f32 do not make)
    assert L.csl_infer_sage_f32(null, null, null, 0, fake, 3, 0, 0, fake, 100, 100, 0, null, 0, fake, fake, 200, st) == -1
    assert L.csl_infer_gat_f32(null, null, null, 0, fake, 3, 0, 0, fake, fake, fake, 8, 32, 0.2, null, 0, 0, fake, fake,
                               256, st) == -1
    # GAT: D % 4, H * D > 4096, n_cls > D, ldo of a hidden layer too small
    assert L.csl_infer_gat_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 8, 6, 0.2, null, 0, 0, null, fake,
                               48, st) == -1
    assert L.csl_infer_gat_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 8, 1024, 0.2, null, 1, 5, null,
                               fake, 5, st) == -1         # a last layer's head mean: H * D <= 4096
    assert L.csl_infer_gat_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 8, 48, 0.2, null, 1, 49, null,
                               fake, 49, st) == -1
    assert L.csl_infer_gat_f32(fake, fake, fake, 10, null, 0, 0, 0, fake, fake, fake, 8, 32, 0.2, null, 0, 0, null,
                               fake, 128, st) == -1
    assert L.csl_infer_gat_f32(fake, fake, fake, 10, null, 0, 0, 0, null, fake, fake, 8, 32, 0.2, null, 0, 0, null,
                               fake, 256, st) == -1
    # evaluation head: C < 1, ld < C, missing outputs
    assert L.csl_infer_eval_f32(fake, 10, 5, 0, fake, fake, fake, fake, fake, st) == -1
    assert L.csl_infer_eval_f32(fake, 4, 5, 10, fake, fake, fake, fake, fake, st) == -1
    assert L.csl_infer_eval_f32(fake, 10, 5, 10, fake, fake, fake, null, fake, st) == -1
    assert L.csl_infer_eval_f32(null, 10, 5, 10, fake, fake, fake, fake, fake, st) == -1


def _csr(degs, seed=0):
    rng = np.random.default_rng(seed)
    degs = np.asarray(degs, dtype=np.int64)
    indptr = np.zeros(len(degs) + 1, dtype=np.int64)
    np.cumsum(degs, out=indptr[1:])
    return indptr, rng.integers(0, len(degs), size=int(indptr[-1]))


def test_neighbour_csr_drops_self_loops_keeps_duplicates():
    indptr = np.array([0, 3, 3, 5, 6], dtype=np.int64)
    indices = np.array([0, 2, 2, 2, 1, 3], dtype=np.int64)     # row 0: self + duplicate, row 3: only a self loop
    ip, ix = infer.neighbour_csr(indptr, indices)
    assert ip.tolist() == [0, 2, 2, 3, 3] and ix.tolist() == [2, 2, 1] and ix.dtype == np.int32


def test_plan_segment_layout():
    S = infer.SEG
    degs = [0, 1, S, S + 1, 3 * S, 5, 2 * S + 7]
    indptr, _ = _csr(degs)
    p = infer.build_plan(indptr)
    items, hubs = p["items"], p["hubs"]
    # whole rows: one item, part -1; hubs: ceil(deg / SEG) items with consecutive parts, in row order
    assert [int(x) for x in p["item_first"]] == [0, 1, 2, 3, 5, 8, 9, 12]
    assert items[:, 0].tolist() == [0, 1, 2, 3, 3, 4, 4, 4, 5, 6, 6, 6]
    assert items[:, 1].tolist() == items[:, 0].tolist()
    assert items[:, 3].tolist() == [-1, -1, -1, 0, 1, 2, 3, 4, -1, 5, 6, 7]
    starts = [int(indptr[r]) + S * j for r, j in [(3, 0), (3, 1), (4, 0), (4, 1), (4, 2), (6, 0), (6, 1), (6, 2)]]
    assert items[items[:, 3] >= 0, 2].tolist() == starts
    assert hubs.tolist() == [[3, 3, 0, 2], [4, 4, 2, 3], [6, 6, 5, 3]]
    # every edge of every row is covered exactly once
    cover = np.zeros(int(indptr[-1]), dtype=np.int64)
    for row, _, e0, part in items:
        e1 = int(indptr[row + 1]) if part < 0 else min(e0 + S, int(indptr[row + 1]))
        cover[e0:e1] += 1
    assert (cover == 1).all()
    # a subset in its own order: positions follow the list
    q = infer.build_plan(indptr, rows=[6, 0, 3])
    assert q["items"][:, 1].tolist() == [0, 0, 0, 1, 2, 2] and q["hubs"][:, :2].tolist() == [[6, 0], [3, 2]]
    # chunks: the parts of a chunk are contiguous and counted from the chunk's first one
    ch = infer.plan_chunks(p, 3)
    assert [c[:2] for c in ch] == [(0, 3), (3, 6), (6, 7)]
    assert [(c[6], c[7]) for c in ch] == [(0, 0), (0, 5), (5, 3)]
    assert [(c[4], c[5]) for c in ch] == [(0, 0), (0, 2), (2, 3)]
    # a chunk is a record that still compares and unpacks as the tuple it was
    assert ch[0] == (0, 3, 0, 3, 0, 0, 0, 0) and ch[1] == (3, 6, 3, 9, 0, 2, 0, 5)
    assert ch[0].n_parts == 0 and ch[1].n_parts == 5 and (ch[1].k0, ch[1].i1, ch[1].h1, ch[1].part0) == (3, 9, 2, 0)


def test_parts_plan_chunks_are_records():
    S = infer.SEG
    indptr, indices = _csr([3, 2 * S + 5, 1, 0, 4, 2, S + 1], seed=3)
    N, P = 7, 2
    rg = infer.RankGraph(indptr, indices, infer.owner_table(N, P), P, 0)
    pp = rg.plan(3)
    ch, w = pp.chunks(), pp.work
    assert len(ch) == pp.n_chunks == 3
    for c, rec in enumerate(ch):
        s0, s1 = int(pp.sub_first[c]), int(pp.sub_first[c + 1])
        h0, h1 = (int(x) for x in np.searchsorted(w["hub_pos"], [s0, s1]))
        p0, p1 = int(w["part_first"][s0]), int(w["part_first"][s1])
        assert rec == (s0, s1, int(w["item_first"][s0]), int(w["item_first"][s1]), h0, h1, p0, p1 - p0,
                       int(pp.own_first[c]), int(pp.own_first[c + 1]), int(pp.recv_first[c]), int(pp.recv_first[c + 1]))
        assert (rec.r0, rec.r1) == (int(pp.recv_first[c]), int(pp.recv_first[c + 1])) and rec.n_parts == p1 - p0
        assert (rec.s0, rec.o1) == (s0, int(pp.own_first[c + 1])) and len(tuple(rec)) == 12
    assert sum(r.n_parts for r in ch) == w["n_parts"] > 0          # (the hub rows were cut)


def test_sage_operands_place_both_halves_and_pad_with_zeros():
    import torch
    from cslicer import splitgnn
    cpu = torch.device("cpu")
    conv = splitgnn.DistSageConv(5, 7)                              # out >= in: aggregate first, table width 8
    W, b = conv.fc.weight.detach(), conv.fc.bias.detach()
    agg_first, w, bias = infer._sage_operands(conv, 8, cpu)
    want = torch.zeros((7, 16))
    want[:, 0:5], want[:, 8:13] = W[:, :5], W[:, 5:]
    assert agg_first is True and torch.equal(w, want) and torch.equal(bias, b)
    conv = splitgnn.DistSageConv(7, 3)                              # out < in: project first, op = 4
    W, b = conv.fc.weight.detach(), conv.fc.bias.detach()
    agg_first, w, bias = infer._sage_operands(conv, 8, cpu)
    want = torch.zeros((8, 8))
    want[0:3, :7], want[4:7, :7] = W[:, :7], W[:, 7:]
    assert agg_first is False and torch.equal(w, want)
    assert bias.shape == (4,) and torch.equal(bias[:3], b) and bias[3] == 0


def test_gat_operands_follow_the_column_map_and_pad_with_zeros():
    import torch
    from cslicer import splitgnn
    H, D, Dp, hp = 2, 3, 4, 8
    conv = splitgnn.DistGATConv(6, D, H)
    with torch.no_grad():
        conv.bias.copy_(torch.arange(1, H * D + 1, dtype=torch.float32))
    in_map = torch.tensor([0, 1, 2, 4, 5, 6])
    ops = infer._gat_operands(conv, in_map, hp, torch.device("cpu"))
    W = conv.fc.weight.detach()
    want = torch.zeros((H * Dp, hp))
    for h in range(H):
        for d in range(D):
            for c in range(6):
                want[h * Dp + d, int(in_map[c])] = W[h * D + d, c]
    assert torch.equal(ops.wz, want) and (ops.H, ops.D, ops.Dp) == (H, D, Dp)
    for got, src in ((ops.al, conv.attn_l), (ops.ar, conv.attn_r), (ops.bz, conv.bias.view(H, D))):
        assert got.shape == (H, Dp) and torch.equal(got[:, :D], src.detach()) and (got[:, D:] == 0).all()
    assert ops.cmap.tolist() == [0, 1, 2, 4, 5, 6] and ops.vl is None and ops.vr is None


def test_splits_round_trip(tmp_path):
    indptr, indices = _csr([2, 1, 3, 0, 2])
    d = str(tmp_path / "g")
    assert l0.write_l0(d, indptr, indices)["num_nodes"] == 5
    assert l0.read_splits(d) is None
    ip, ix, meta = l0.read_l0(d)
    assert "csum_train" not in meta
    tr, va = np.array([0, 2, 4]), np.array([1, 3])
    meta = l0.write_l0(str(tmp_path / "s"), indptr, indices, train_idx=tr, val_idx=va)
    assert meta["csum_train"] == 6 and meta["csum_test"] == 4
    got = l0.read_splits(str(tmp_path / "s"))
    assert got[0].dtype == np.int64 and got[0].tolist() == [0, 2, 4] and got[1].tolist() == [1, 3]
    ip2, ix2, _ = l0.read_l0(str(tmp_path / "s"))
    assert (ip2 == ip).all() and (ix2 == ix).all()
    with pytest.raises(ValueError):
        l0.write_l0(str(tmp_path / "x"), indptr, indices, train_idx=tr)


def test_splits_checksum_mismatch_raises(tmp_path):
    indptr, indices = _csr([2, 1, 3, 0, 2])
    d = str(tmp_path / "s")
    l0.write_l0(d, indptr, indices, train_idx=np.array([0, 2, 4]), val_idx=np.array([1, 3]))
    np.array([0, 2, 3], dtype=np.int64).tofile(os.path.join(d, "train_idx.bin"))
    with pytest.raises(ValueError, match="checksum"):
        l0.read_splits(d)


def test_cli_accepts_eval_split():
    ap = train._parser()
    assert ap.parse_args([]).eval_split == "none"
    for v in ("none", "file", "holdout"):
        assert ap.parse_args(["--eval-split", v, "--eval-every", "1"]).eval_split == v
    with pytest.raises(SystemExit):
        ap.parse_args(["--eval-split", "bogus"])
    a = ap.parse_args(["--eval-split", "holdout"])
    tr, va = train._split(a, 1000)
    assert len(tr) == 800 and len(va) == 200 and len(np.intersect1d(tr, va)) == 0
    assert (train._split(a, 1000)[1] == va).all()               # seeded
    assert train._split(ap.parse_args([]), 1000) == (None, None)


def test_graph_cache_is_host_side_until_used_and_released():
    import torch
    indptr, indices = _csr([3, 0, 2, 5, 1])
    dev = torch.device("cuda", 0)
    g = infer.graph_of(indptr, indices, dev)
    assert infer.graph_of(indptr, indices, dev) is g and not g.uploaded()      # prepared on the host only
    assert g.device_bytes() == 4 * 6 + 4 * g.n_edges + g.all_rows.nbytes()
    infer.release(indptr, indices)
    assert infer.graph_of(indptr, indices, dev) is not g
    infer.release()
    assert not infer._GRAPHS


def test_width_limit_of_the_attention_last_layer():
    from cslicer import splitgnn
    m = splitgnn.DistGATModel(8, 4, 600, heads=8, n_layers=2)       # 8 x 600 columns in the last layer
    indptr, indices = _csr([1, 1])
    with pytest.raises(ValueError, match="last layer"):
        infer.full_inference(m, indptr, indices, np.zeros((2, 8), dtype=np.float32))


def test_evaluate_takes_labels_of_every_node():
    from cslicer import splitgnn
    m = splitgnn.DistSAGEModel(4, 4, 3, n_layers=1)
    indptr, indices = _csr([1, 1, 1])
    with pytest.raises(ValueError, match="one label per node"):
        infer.evaluate(m, indptr, indices, np.zeros((3, 4), dtype=np.float32), [0, 1], np.zeros(2, dtype=np.int64))
