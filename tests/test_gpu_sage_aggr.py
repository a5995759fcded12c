"""The GraphSAGE kernels of csrc/aggregate.hip at their dispatch edges, against the float64 restatement in
tests/sage_ref.py (tests/test_gpu_aggr.py compares them with fp32 torch and with each other, at one shape each).

What decides a kernel's instance, and what is therefore varied here:
  * group_for(H): 1 .. 64 lanes per row (powers of two over ceil(H / 4) column quads);
  * vec_ok: float4 accesses only when H % 4 == 0, the leading dimensions are multiples of 4 and the operands are
    16-byte aligned -- the scalar fallback is reached here at the SAME H through a view offset by one float and through a
    leading dimension of H + 1, not only through odd H;
  * tb_rows / rb_rows: rows per block double beyond 2,048 blocks (n_pad > 32,768 by source, > 262,144 for the ReLU pass);
  * CSL_T_SORTED_MAX = 128 entries (longer lists by source are hub lists), cut into segments of 512 entries;
  * SM_CMAX = 256 classes, RM_L = 16 lanes x 4 columns per block of csl_reduce_multi_f32.

Tolerances: forward values rtol = atol = 1e-5, gradients within 1e-4 of the tensor's largest entry (north_star).  Where
a sum is too long for that (hub lists, column sums over 10^5 rows) the bound is derived from the float64 reference: an
fp32 sum of k terms in any order is within k * 2^-24 * (sum of the |terms|) of the exact one (each of the at most k - 1
additions an entry goes through rounds a partial sum no larger than the sum of the |terms| by at most 2^-24 of it; one more
for the product with 1 / deg) -- written beside the assertion.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sage_ref as R

pytestmark = pytest.mark.gpu

E_INVALID = -1
EPS = 2.0 ** -24
T_SORTED_MAX, HUB_SEG = 128, 512
FWD = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module")
def mods():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr, aggr._lib()


def _grad_close(got, want, what=""):
    """a gradient: within 1e-4 of the tensor's largest entry"""
    want = want if torch.is_tensor(want) else torch.from_numpy(want)
    err, ref = float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())
    assert err <= 1e-4 * ref, "%s: max error %.3g against a largest entry of %.3g" % (what, err, ref)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).int().cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


SENT = -777.0


def _lay(a, kind):
    """the float32 matrix `a` on the device as (view, backing): 'dense' (aligned, contiguous), 'offset' (the same rows one
    float into an aligned buffer) or 'ld+1' (a leading dimension of H + 1)"""
    a = torch.as_tensor(a, dtype=torch.float32)
    n, H = a.shape
    if kind == "dense":
        back = a.cuda().contiguous()
        return back, back
    if kind == "offset":
        back = torch.full((n * H + 8,), SENT, device="cuda")
        v = back[1:1 + n * H].view(n, H)
    else:
        back = torch.full((n, H + 1), SENT, device="cuda")
        v = back[:, :H]
    v.copy_(a.cuda())
    return v, back


def _untouched(v, back, kind):
    if kind == "offset":
        return bool((back[:1] == SENT).all()) and bool((back[1 + v.numel():] == SENT).all())
    if kind == "ld+1":
        return bool((back[:, -1] == SENT).all())
    return True


LAYOUTS = ("dense", "offset", "ld+1")
ALL_H = [1, 3, 4, 5, 8, 12, 16, 17, 32, 33, 64, 100, 128, 129, 252, 256, 260, 300]


def _csr(rng, n, n_src, max_deg):
    deg = rng.integers(0, max_deg + 1, size=n)
    deg[:3] = (0, 1, max_deg)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    return indptr, rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int64)


# ---- the row kernels: every group size, the vector path and the scalar fallback at the same H -----------------------

@pytest.mark.parametrize("H", ALL_H)
def test_spmm_sum_in_all_its_forms(mods, H):
    aggr, L = mods
    rng = np.random.default_rng(H)
    n, n_src, table = 203, 91, 160                    # (203 rows leave the last block partial for every group size)
    indptr, indices = _csr(rng, n, n_src, 9)
    x = rng.standard_normal((table, H)).astype(np.float32)
    rowmap = rng.permutation(table)[:n_src]
    rows = np.sort(rng.permutation(n)[:57])
    ip, ix, rws, rm = _i32(indptr), _i32(indices), _i32(rows), _i32(rowmap)
    want = R.spmm_sum(x[:n_src], indptr, indices)
    want_map = R.spmm_sum(x, indptr, indices, rowmap=rowmap)
    st = aggr._stream
    res = {}
    for kind in LAYOUTS:
        xv, _ = _lay(x, kind)
        got = {}
        for form in ("plain", "subset", "compact", "map", "map-compact"):
            m = rows.shape[0] if form in ("compact", "map-compact") else n
            ov, ob = _lay(np.full((m, H), SENT, dtype=np.float32), kind)
            if form == "plain":
                rc = L.csl_spmm_sum_f32(_ptr(ip), _ptr(ix), None, n, _ptr(xv), xv.stride(0), _ptr(ov), ov.stride(0), H, st())
            elif form == "subset":
                rc = L.csl_spmm_sum_f32(_ptr(ip), _ptr(ix), _ptr(rws), rows.shape[0], _ptr(xv), xv.stride(0), _ptr(ov),
                                        ov.stride(0), H, st())
            elif form == "compact":
                rc = L.csl_spmm_sum_compact_f32(_ptr(ip), _ptr(ix), _ptr(rws), rows.shape[0], _ptr(xv), xv.stride(0),
                                                _ptr(ov), ov.stride(0), H, st())
            else:
                comp = form == "map-compact"
                rc = L.csl_spmm_sum_map_f32(_ptr(ip), _ptr(ix), _ptr(rws) if comp else None, rows.shape[0] if comp else n,
                                            _ptr(xv), xv.stride(0), _ptr(rm), _ptr(ov), ov.stride(0), H, int(comp), st())
            assert rc == 0, (form, kind)
            torch.cuda.synchronize()
            assert _untouched(ov, ob, kind), (form, kind)
            o = ov.cpu().double()
            if form == "plain":
                torch.testing.assert_close(o, want, **FWD)
            elif form == "subset":
                torch.testing.assert_close(o[rows], want[rows], **FWD)
                rest = np.setdiff1d(np.arange(n), rows)
                assert bool((o[rest] == SENT).all())           # the rows not listed are not touched
            elif form == "compact":
                torch.testing.assert_close(o, want[rows], **FWD)
            elif form == "map":
                torch.testing.assert_close(o, want_map, **FWD)
            else:
                torch.testing.assert_close(o, want_map[rows], **FWD)
            got[form] = ov.clone() if form != "subset" else ov[torch.from_numpy(rows).cuda()].clone()
        res[kind] = got
    for form in res["dense"]:          # the sum is in edge order on both paths: bit for bit the same
        assert torch.equal(res["dense"][form], res["offset"][form]) and torch.equal(res["dense"][form], res["ld+1"][form]), form


@pytest.mark.parametrize("H", ALL_H)
def test_spmm_sum_backward(mods, H):
    aggr, L = mods
    rng = np.random.default_rng(50 + H)
    n, n_src = 203, 91
    indptr, indices = _csr(rng, n, n_src, 9)
    rows = np.sort(rng.permutation(n)[:57])
    g = rng.standard_normal((n, H)).astype(np.float32)
    ip, ix, rws = _i32(indptr), _i32(indices), _i32(rows)
    want = R.spmm_sum_bwd(g, indptr, indices, n_src)
    sub_ip = np.zeros(n + 1, dtype=np.int64)          # the CSR with only the listed rows' edges
    deg = np.diff(indptr)
    keep = np.zeros(n, dtype=bool)
    keep[rows] = True
    np.cumsum(np.where(keep, deg, 0), out=sub_ip[1:])
    sub_ix = indices[np.repeat(keep, deg)]
    want_rows = R.spmm_sum_bwd(g, sub_ip, sub_ix, n_src)
    for kind in LAYOUTS:
        gv, _ = _lay(g, kind)
        gc, _ = _lay(g[rows], kind)
        for form in ("all", "subset", "compact"):
            ov, ob = _lay(np.zeros((n_src, H), dtype=np.float32), kind)
            if form == "all":
                rc = L.csl_spmm_sum_bwd_f32(_ptr(ip), _ptr(ix), None, n, _ptr(gv), gv.stride(0), 0, _ptr(ov), ov.stride(0),
                                            H, aggr._stream())
            else:
                src = gc if form == "compact" else gv
                rc = L.csl_spmm_sum_bwd_f32(_ptr(ip), _ptr(ix), _ptr(rws), rows.shape[0], _ptr(src), src.stride(0),
                                            int(form == "compact"), _ptr(ov), ov.stride(0), H, aggr._stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert _untouched(ov, ob, kind)
            _grad_close(ov, want if form == "all" else want_rows, "%s %s" % (form, kind))


@pytest.mark.parametrize("H", ALL_H)
def test_gather_scatter_and_divide_rows(mods, H):
    aggr, L = mods
    rng = np.random.default_rng(90 + H)
    n_src, n = 131, 203
    src = rng.standard_normal((n_src, H)).astype(np.float32)
    idx = rng.integers(0, n_src, size=n)
    idx[[0, 77, n - 1]] = -1
    uniq = rng.permutation(n_src)[:101]
    uniq_m = uniq.copy()
    uniq_m[[4, 100]] = -1
    add = rng.standard_normal((n, H)).astype(np.float32)
    deg = rng.integers(0, 7, size=n_src)
    st = aggr._stream
    res = {}
    for kind in LAYOUTS:
        sv, _ = _lay(src, kind)
        # gather (index -1: a zero row)
        ov, ob = _lay(np.full((n, H), SENT, dtype=np.float32), kind)
        assert L.csl_gather_rows_f32(_ptr(sv), sv.stride(0), _ptr(_i32(idx)), n, _ptr(ov), ov.stride(0), H, st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ov.cpu().double(), R.gather_rows(src, idx)) and _untouched(ov, ob, kind)
        # scatter-add over unique rows (index -1: skipped)
        dv, db = _lay(src, kind)
        av, _ = _lay(add[:101], kind)
        assert L.csl_scatter_add_rows_f32(_ptr(dv), dv.stride(0), _ptr(_i32(uniq_m)), 101, _ptr(av), av.stride(0), H, st()) == 0
        want = torch.from_numpy(src).double()
        ok = uniq_m >= 0
        want[torch.from_numpy(uniq_m[ok])] += torch.from_numpy(add[:101][ok]).double()
        torch.cuda.synchronize()
        torch.testing.assert_close(dv.cpu().double(), want, **FWD)
        assert _untouched(dv, db, kind)
        res[kind] = dv.clone()
        # scatter-add where the rows repeat (atomics)
        dv, db = _lay(src, kind)
        av, _ = _lay(add, kind)
        assert L.csl_scatter_add_rows_atomic_f32(_ptr(dv), dv.stride(0), _ptr(_i32(idx)), n, _ptr(av), av.stride(0), H,
                                                 st()) == 0
        want = torch.from_numpy(src).double()
        ok = idx >= 0
        want.index_add_(0, torch.from_numpy(idx[ok]), torch.from_numpy(add[ok]).double())
        torch.cuda.synchronize()
        torch.testing.assert_close(dv.cpu().double(), want, **FWD)
        assert _untouched(dv, db, kind)
        # divide by max(deg, 1)
        dv, db = _lay(src, kind)
        assert L.csl_div_rows_f32(_ptr(dv), dv.stride(0), _ptr(_i32(deg)), n_src, H, st()) == 0
        torch.cuda.synchronize()
        torch.testing.assert_close(dv.cpu().double(), torch.from_numpy(src).double() /
                                   torch.from_numpy(np.maximum(deg, 1)).double()[:, None], **FWD)
        assert _untouched(dv, db, kind)
        res[kind + " div"] = dv.clone()
        # set rows (csl_scatter_rows_f32: float4 only, refuses everything else before a launch)
        dv, db = _lay(src, kind)
        av, _ = _lay(add[:101], kind)
        rc = L.csl_scatter_rows_f32(_ptr(dv), dv.stride(0), _ptr(_i32(uniq)), 101, _ptr(av), av.stride(0), H, st())
        torch.cuda.synchronize()
        if H % 4 == 0 and kind == "dense":
            want = torch.from_numpy(src).clone()
            want[torch.from_numpy(uniq)] = torch.from_numpy(add[:101])
            assert rc == 0 and torch.equal(dv.cpu(), want)
        else:
            assert rc == E_INVALID and torch.equal(dv.cpu(), torch.from_numpy(src))
    assert torch.equal(res["dense"], res["offset"]) and torch.equal(res["dense"], res["ld+1"])
    assert torch.equal(res["dense div"], res["offset div"]) and torch.equal(res["dense div"], res["ld+1 div"])


def test_refusals_of_the_row_kernels(mods):
    aggr, L = mods
    H, n = 8, 4
    a = torch.zeros((n, H), device="cuda")
    b = torch.zeros((n, H), device="cuda")
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    ip = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    st = aggr._stream
    assert L.csl_gather_rows_f32(None, H, _ptr(idx), n, _ptr(b), H, H, st()) == E_INVALID          # no source
    assert L.csl_gather_rows_f32(_ptr(a), H - 1, _ptr(idx), n, _ptr(b), H, H, st()) == E_INVALID   # lds < H
    assert L.csl_gather_rows_f32(_ptr(a), H, _ptr(idx), n, _ptr(b), H - 1, H, st()) == E_INVALID   # ldd < H
    assert L.csl_gather_rows_f32(_ptr(a), H, _ptr(idx), n, _ptr(b), H, H, st()) == 0
    assert L.csl_spmm_sum_bwd_f32(_ptr(ip), _ptr(idx), None, n, _ptr(a), H - 1, 0, _ptr(b), H, H, st()) == E_INVALID   # ldg
    assert L.csl_spmm_sum_bwd_f32(_ptr(ip), _ptr(idx), None, n, _ptr(a), H, 0, _ptr(b), H - 1, H, st()) == E_INVALID   # ldx
    assert L.csl_spmm_sum_bwd_f32(_ptr(ip), _ptr(idx), None, n, _ptr(a), H, 0, _ptr(b), H, H, st()) == 0
    torch.cuda.synchronize()


# ---- the operand kernels --------------------------------------------------------------------------------------------

CAT_H = [4, 8, 12, 16, 20, 32, 36, 60, 64, 68, 124, 128, 132, 252, 256, 260]      # both sides of every group size


@pytest.mark.parametrize("H", CAT_H)
def test_sage_cat_both_forms_and_their_gradients(mods, H):
    aggr, L = mods
    rng = np.random.default_rng(300 + H)
    n, n_src, n_pad, n_agg = 203, 150, 256, 240
    indptr, indices = _csr(rng, n, n_src, 7)
    self_ids = rng.permutation(n_src)[:n_src].tolist() + rng.integers(0, n_src, size=n - n_src).tolist()
    self_ids = np.asarray(self_ids, dtype=np.int64)
    self_ids[::6] = -1
    x = rng.standard_normal((n_src, H)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    ip, ix, sid = _i32(indptr), _i32(indices), _i32(self_ids)
    for relu_in in (False, True):
        cat = aggr.sage_cat(xd, sid, n, n_pad, indptr=ip, indices=ix, relu_in=relu_in)
        want = R.operand(x, indptr, indices, self_ids, n_pad, relu_in=relu_in)
        torch.testing.assert_close(cat.cpu().double(), want, **FWD)
        assert bool((cat[n:] == 0).all())
    # merged-sums form: agg[owned[r]] / max(deg[r], 1), the degree given (a rank's true degree, not a CSR's row length)
    owned = rng.permutation(n_agg)[:n]
    deg = rng.integers(0, 9, size=n)
    agg = rng.standard_normal((n_agg, H)).astype(np.float32)
    cat = aggr.sage_cat(xd, sid, n, n_pad, owned=_i32(owned), deg=_i32(deg), agg=torch.from_numpy(agg).cuda())
    want = torch.zeros((n_pad, 2 * H), dtype=torch.float64)
    want[:n, :H] = R.gather_rows(x, self_ids)
    want[:n, H:] = torch.from_numpy(agg[owned]).double() / torch.from_numpy(np.maximum(deg, 1)).double()[:, None]
    torch.testing.assert_close(cat.cpu().double(), want, **FWD)
    assert bool((cat[n:] == 0).all())
    # gradients: CSR form (atomics) ...
    gcat = rng.standard_normal((n_pad, 2 * H)).astype(np.float32)
    gd = torch.from_numpy(gcat).cuda()
    gx = aggr.sage_cat_bwd(ip, ix, sid, gd, n, n_src)
    _grad_close(gx, R.operand_grad_by_destination(gcat, indptr, indices, self_ids, n_src), "sage_cat_bwd")
    # ... and merged-sums form (self ids unique where present): three lines of numpy
    uniq = rng.permutation(n_src + 60)[:n].astype(np.int64)
    uniq[::5] = -1
    gx2, gagg = aggr.sage_cat_rows_bwd(_i32(uniq), _i32(owned), _i32(deg), gd, n, n_src + 60, n_agg)
    wx, wa = np.zeros((n_src + 60, H)), np.zeros((n_agg, H))
    wx[uniq[uniq >= 0]] = gcat[:n][uniq >= 0, :H]
    wa[owned] = gcat[:n, H:].astype(np.float64) / np.maximum(deg, 1)[:, None]
    assert torch.equal(gx2.cpu().double(), torch.from_numpy(wx))
    torch.testing.assert_close(gagg.cpu().double(), torch.from_numpy(wa), rtol=1e-6, atol=0)
    # the rank step's re-ordering into out rows (three lines of numpy): rows nobody owns keep what was there
    g2 = torch.full((n_agg, 2 * H), SENT, device="cuda")
    assert L.csl_sage_rank_g2_f32(_ptr(_i32(owned)), _ptr(_i32(deg)), n, _ptr(gd), 2 * H, _ptr(g2), 2 * H, H,
                                  aggr._stream()) == 0
    w2 = np.full((n_agg, 2 * H), SENT, dtype=np.float64)
    w2[owned, :H] = gcat[:n, :H]
    w2[owned, H:] = gcat[:n, H:].astype(np.float64) / np.maximum(deg, 1)[:, None]
    torch.cuda.synchronize()
    torch.testing.assert_close(g2.cpu().double(), torch.from_numpy(w2), rtol=1e-6, atol=0)


# ---- the gradient by source -----------------------------------------------------------------------------------------

def _by_source_case(rng, n_dst, n_src, max_deg, H, hubs=()):
    """a destination CSR over n_src sources (hubs: [(source, list length)]: exactly that many rows name the source, which
    is nobody's self row), its slice by source and a random operand gradient"""
    deg = rng.integers(0, max_deg + 1, size=n_dst)
    indptr = np.zeros(n_dst + 1, dtype=np.int64)
    hub_ids = [h for h, _ in hubs]
    extra = np.zeros(n_dst, dtype=np.int64)
    for _, ln in hubs:
        extra[:ln] += 1
    np.cumsum(deg + extra, out=indptr[1:])
    pool = np.setdiff1d(np.arange(n_src), hub_ids + [n_src - 1, n_src - 2])     # (two sources nobody names)
    indices = np.empty(int(indptr[-1]), dtype=np.int64)
    for r in range(n_dst):
        # half of the edges name one of the first 300 sources: lists of a few dozen entries next to short and empty ones
        pick = np.where(rng.random(deg[r]) < 0.5, rng.integers(0, min(300, pool.shape[0]), size=deg[r]),
                        rng.integers(0, pool.shape[0], size=deg[r]))
        indices[indptr[r]:indptr[r + 1]] = [h for h, ln in hubs if r < ln] + pool[pick].tolist()
    self_ids = rng.choice(pool, size=n_dst, replace=n_dst > pool.shape[0])
    self_ids[::7] = -1
    self_ids[1] = n_src - 2                                                       # a source that is ONLY a self row
    gcat = rng.standard_normal((n_dst, 2 * H)).astype(np.float32)
    tp, ti = R.by_source(indptr, indices, self_ids, n_src)
    return indptr, indices, self_ids, gcat, tp, ti


def _check_by_source(aggr, case, n_src, n_pad, H, masked, hub, rng):
    indptr, indices, self_ids, gcat, tp, ti = case
    y = rng.standard_normal((n_pad, H)).astype(np.float32) if masked else None
    args = (_i32(tp), _i32(ti), _i32(indptr), torch.from_numpy(gcat).cuda(), torch.from_numpy(y).cuda() if masked else None,
            n_src, n_pad)
    out, cs = aggr.sage_cat_bwd_t(*args, hub=hub)
    out, cs = out.clone(), cs.clone()
    gx, ab = R.operand_grad_by_source(gcat, tp, ti, indptr)
    want, wcs = R.masked_colsum(gx, y, n_pad)
    o = out.cpu().double()
    assert bool((out[n_src:] == 0).all())
    assert bool((o[n_src - 1] == 0).all())                                       # a source nobody points at
    if masked:
        assert bool((o[:n_src][torch.from_numpy(y[:n_src]) <= 0] == 0).all())
    k = int(np.diff(tp).max())
    if k <= T_SORTED_MAX:
        _grad_close(out, want, "by source")
    # Every entry is an fp32 sum of its list's k terms in some order; a term is gcat * (1 / deg): the reciprocal and the
    # product round once each (2 * 2^-24 |term|), each of the k - 1 additions rounds a partial sum of at most sum |terms|:
    # |error| <= (k + 1) 2^-24 sum |terms| to first order, (k + 2) with room for the second -- the derived bound, which
    # holds for hub lists too
    lens = torch.from_numpy(np.diff(tp)).double()[:, None]
    bound = (lens + 2) * EPS * ab
    assert bool(((o[:n_src] - want[:n_src]).abs() <= bound + 1e-30).all()), float(((o[:n_src] - want[:n_src]).abs() - bound).max())
    # the existing hub test's measure: relative to the row's largest |term| sum
    rel = (o[:n_src] - want[:n_src]).abs() / ab.max(dim=1, keepdim=True).values.clamp(min=1.0)
    assert float(rel.max()) <= 1e-5
    # column sums: within 1e-4 of the largest entry, as tests/test_gpu_aggr.py has it
    assert float((cs.cpu().double() - wcs).abs().max()) <= 1e-4 * float(wcs.abs().max())
    out2, cs2 = aggr.sage_cat_bwd_t(*args, hub=hub)
    if not hub or k <= T_SORTED_MAX:
        assert torch.equal(out2, out) and torch.equal(cs2, cs)                   # deterministic: no atomics
    return out


@pytest.mark.parametrize("H,n_pad", [(H, p) for H in (4, 60, 64, 68, 128, 132, 256) for p in (32768, 32800)] +
                         [(64, 65536), (64, 65568), (132, 65536), (132, 65568)])
def test_sage_cat_bwd_by_source_on_both_sides_of_a_block_resize(mods, H, n_pad):
    """tb_rows: 16 rows per block up to n_pad = 32,768 (2,048 blocks), 32 up to 65,536, then 64"""
    aggr, L = mods
    rng = np.random.default_rng(H + n_pad)
    n_src = n_pad - 9
    case = _by_source_case(rng, 6000, n_src, 8, H)
    for masked in (False, True):
        _check_by_source(aggr, case, n_src, n_pad, H, masked, False, rng)


@pytest.mark.parametrize("longest", [T_SORTED_MAX, T_SORTED_MAX + 1, HUB_SEG, HUB_SEG + 1, 1700])
@pytest.mark.parametrize("H", [64, 100, 256])
def test_hub_lists_against_float64(mods, longest, H):
    """Synthetic slices by source whose longest list is exactly the threshold, one more, one segment, one more, several
    segments: one hub between short lists (source 40) and two hubs side by side (sources 5 and 6, the second shorter)"""
    aggr, L = mods
    rng = np.random.default_rng(longest + H)
    n_src, n_dst, n_pad = 300, 2000, 320
    hubs = [(5, longest), (6, max(longest - 37, 1)), (40, longest)]
    case = _by_source_case(rng, n_dst, n_src, 3, H, hubs=hubs)
    tp = case[4]
    assert int(np.diff(tp).max()) == longest and tp[6] - tp[5] == longest and tp[41] - tp[40] == longest
    outs = [_check_by_source(aggr, case, n_src, n_pad, H, masked, True, rng) for masked in (False, True)]
    if longest <= T_SORTED_MAX:      # no list beyond the threshold: the hub entry point is the plain kernel
        plain, _ = aggr.sage_cat_bwd_t(_i32(tp), _i32(case[5]), _i32(case[0]), torch.from_numpy(case[3]).cuda(), None, n_src,
                                       n_pad)
        assert torch.equal(plain, outs[0])


# ---- ReLU mask + column sums, the loss, the second stage ------------------------------------------------------------

@pytest.mark.parametrize("n_pad", [262144 - 128, 262144, 262144 + 128])
@pytest.mark.parametrize("H,masked", [(8, True), (36, False)])
def test_relu_bwd_colsum_across_a_block_resize(mods, n_pad, H, masked):
    """rb_rows: 128 rows per block up to n_pad = 262,144 (2,048 blocks), then 256"""
    aggr, L = mods
    rng = np.random.default_rng(n_pad + H)
    n = n_pad - 77
    g = rng.standard_normal((n, H)).astype(np.float32)
    y = rng.standard_normal((n_pad, H)).astype(np.float32) if masked else None
    out, cs = aggr.relu_bwd_colsum(torch.from_numpy(g).cuda(), torch.from_numpy(y).cuda() if masked else None, n, n_pad)
    want, wcs = R.masked_colsum(g, y, n_pad)
    assert torch.equal(out.cpu().double(), want)                                 # a copy under a mask: exact
    _grad_close(cs, wcs, "column sums")                                          # the bias gradient: 1e-4 of its largest entry
    # and, entry by entry, what an fp32 sum of n terms in any order allows: n 2^-24 sum |terms| (module docstring)
    assert bool(((cs.cpu().double() - wcs).abs() <= n * EPS * want.abs().sum(0)).all())


@pytest.mark.parametrize("C", [1, 2, 47, 255, 256])
@pytest.mark.parametrize("shift", [0.0, 80.0, -80.0])
def test_softmax_cross_entropy_both_entry_points(mods, C, shift):
    aggr, L = mods
    rng = np.random.default_rng(C)
    n, n_pad, scale = 203, 256, 1.0 / 203
    z = (rng.standard_normal((n_pad, C)) * 3 + shift).astype(np.float32)
    labels_all = rng.integers(0, C, size=500)
    ids = rng.permutation(500)[:n]
    want_loss, want_g, want_cs = R.softmax_ce(z, labels_all[ids], scale, n_pad)
    zd, idd, lab = torch.from_numpy(z).cuda(), _i32(ids), torch.from_numpy(labels_all).cuda()
    # one call
    loss = torch.zeros(1, device="cuda")
    grad = torch.full((n_pad, C), SENT, device="cuda")
    scratch = torch.zeros((int(L.csl_softmax_ce_scratch(n)) + 1,), device="cuda")
    assert L.csl_softmax_ce_f32(_ptr(zd), C, n, C, _ptr(idd), None, _ptr(lab), scale, _ptr(loss), _ptr(grad), C,
                                _ptr(scratch), aggr._stream()) == 0
    torch.cuda.synchronize()
    assert abs(float(loss) - want_loss) <= 1e-5 * max(abs(want_loss), 1e-30)
    _grad_close(grad[:n], want_g[:n], "softmax_ce grad")
    assert bool((grad[n:] == SENT).all())
    # the open two-stage form: padded rows zeroed, per-block loss and column sums
    blocks = (n_pad + 3) // 4
    grad = torch.full((n_pad, C), SENT, device="cuda")
    lpart = torch.full((blocks,), SENT, device="cuda")
    cpart = torch.full((blocks, C), SENT, device="cuda")
    assert L.csl_softmax_ce_partial_f32(_ptr(zd), C, n, n_pad, C, _ptr(idd), None, _ptr(lab), scale, _ptr(grad), C,
                                        _ptr(lpart), _ptr(cpart), aggr._stream()) == 0
    torch.cuda.synchronize()
    assert abs(float(lpart.double().sum()) - want_loss) <= 1e-5 * max(abs(want_loss), 1e-30)
    _grad_close(grad, want_g, "softmax_ce_partial grad")
    assert bool((grad[n:] == 0).all())
    _grad_close(cpart.double().sum(0), want_cs, "bias column sums")


def test_softmax_partial_refuses_column_sums_beyond_256_classes(mods):
    aggr, L = mods
    z = torch.zeros((4, 300), device="cuda")
    one = torch.zeros((4 * 300,), device="cuda")
    lp = torch.zeros((4,), device="cuda")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    lab = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert L.csl_softmax_ce_partial_f32(_ptr(z), 300, 4, 4, 300, _ptr(ids), None, _ptr(lab), 1.0, _ptr(one), 300, _ptr(lp),
                                        _ptr(one), aggr._stream()) == E_INVALID
    assert L.csl_softmax_ce_partial_f32(_ptr(z), 300, 4, 4, 300, _ptr(ids), None, _ptr(lab), 1.0, _ptr(one), 300, _ptr(lp),
                                        None, aggr._stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("nblk", [0, 1, 2, 2049])
def test_reduce_multi_twelve_jobs(mods, nblk):
    """12 jobs in one launch, vector (H % 4 == 0, aligned) and scalar (odd H, or a source one float off alignment) mixed,
    H at and around 4 * RM_L = 64 columns per block"""
    aggr, L = mods
    rng = np.random.default_rng(nblk)
    Hs = [1, 63, 64, 65, 4096, 64, 4096, 1, 63, 64, 65, 68]
    off = [0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0]                 # jobs 5, 6: H % 4 == 0 but a misaligned source: scalar
    nb = [nblk if j != 9 else 0 for j in range(12)]            # job 9 always has no partial rows: zeros
    src_np = [rng.standard_normal((nb[j], Hs[j])).astype(np.float32) for j in range(12)]
    bufs, srcs, dsts = [], [], []
    for j in range(12):
        b = torch.zeros((nb[j] * Hs[j] + 8,), device="cuda")
        v = b[off[j]:off[j] + nb[j] * Hs[j]]
        v.copy_(torch.from_numpy(src_np[j]).reshape(-1).cuda())
        bufs.append(b)
        srcs.append(v)
        dsts.append(torch.full((Hs[j] + 4,), SENT, device="cuda"))
    a_src = (C.c_void_p * 12)(*[v.data_ptr() for v in srcs])
    a_dst = (C.c_void_p * 12)(*[d.data_ptr() for d in dsts])
    a_n = (C.c_int64 * 12)(*nb)
    a_h = (C.c_int32 * 12)(*Hs)
    assert L.csl_reduce_multi_f32(12, a_src, a_n, a_h, a_dst, aggr._stream()) == 0
    torch.cuda.synchronize()
    for j in range(12):
        want = torch.from_numpy(src_np[j]).double().sum(0)
        ab = torch.from_numpy(src_np[j]).double().abs().sum(0)
        got = dsts[j][:Hs[j]].cpu().double()
        # a sum of nblk fp32 terms in any order: nblk 2^-24 sum |terms| (module docstring); exact for 0 and 1 rows, one fp32 addition for 2
        assert bool(((got - want).abs() <= nb[j] * EPS * ab).all()), (j, float((got - want).abs().max()))
        if nb[j] <= 1:
            assert torch.equal(got, want)
        elif nb[j] == 2:             # one fp32 addition
            assert torch.equal(dsts[j][:Hs[j]].cpu(), torch.from_numpy(src_np[j][0] + src_np[j][1]))
        assert bool((dsts[j][Hs[j]:] == SENT).all()), j
    assert L.csl_reduce_multi_f32(13, a_src, a_n, a_h, a_dst, aggr._stream()) == E_INVALID
