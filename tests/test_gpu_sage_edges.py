"""The fused GraphSAGE forward (csl_sage_fwd_mfma_f32, csrc/sage_mfma.hip) at its dispatch edges, against the float64
restatement in tests/sage_ref.py.

What decides the kernel's path, and what is therefore varied here:
  * the longest row among a WORKGROUP's tiles: <= EC = 6 edges one pass, <= 12 two, <= EMAX = 16 three, longer (or H > 128)
    the generic producer, which reads the edges beyond the 16 staged ones straight from the index arrays;
  * the number of tiles S a workgroup owns (tiles b, b + G, ...; G = min(tiles, CUs)): the three staged-address buffers
    rotate over them ((t+4)%3, (t+5)%3, (t+6)%3), so S = 2, 3, 4 with a partial last round take every residue;
  * KQ = H / 4 k-groups of W: 25 and 24 (registers + LDS), 16 (registers), > 16 (registers + streamed), < 16 (streamed);
    the parity of the 32-column tiles of `out` (a consumer wave owns two);
  * leading dimensions, the row map, 64-bit row addresses.

Tolerance: y and cat within rtol = atol = 1e-5 of float64 (north_star: aggregation outputs within 1e-5 fp32); bit-exact on
small integers with degrees in {0, 1, 2, 4}.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sage_ref as R

pytestmark = pytest.mark.gpu

EC, EMAX, BM = 6, 16, 32          # csrc/sage_mfma.hip
WIDEST = 276                      # the widest H whose two operand tiles + staged rows fit a CU's 160 KB of LDS (lds_for)
E_INVALID = -1                    # CSL_E_INVALID (cslicer_hip.h)
TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module")
def lib():
    from cslicer import _abi, aggr
    _abi.load()
    return aggr._lib()


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _graph(rng, deg, n_src, no_self_every=5):
    deg = np.asarray(deg, dtype=np.int64)
    n = deg.shape[0]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    indices = rng.integers(0, n_src, size=int(indptr[-1])).astype(np.int64)
    self_ids = rng.integers(0, n_src, size=n).astype(np.int64)
    if no_self_every:
        self_ids[::no_self_every] = -1
    return indptr, indices, self_ids


def _weights(rng, H, out, integers=False):
    if integers:
        W = rng.integers(-2, 3, size=(out, 2 * H)).astype(np.float32)
        W[np.arange(out), np.arange(out) % (2 * H)] += 5.0      # asymmetric
        return W, rng.integers(-4, 5, size=out).astype(np.float32)
    return ((rng.standard_normal((out, 2 * H)) / np.sqrt(2 * H)).astype(np.float32),
            rng.standard_normal(out).astype(np.float32))


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).int().cuda() if a is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _call(lib, indptr, indices, self_ids, rowmap, x, W, b, n, n_pad, H, out, relu_in, relu_out, cat, y, wpack=None):
    """csl_sage_fwd_mfma_f32 on device tensors as they are (views included): returns the code"""
    from cslicer import aggr
    if wpack is None:
        nw = lib.csl_sage_fwd_mfma_scratch(H, out)
        assert nw > 0, (H, out)
        wpack = torch.empty((nw,), dtype=torch.float32, device="cuda")
    return lib.csl_sage_fwd_mfma_f32(_ptr(indptr), _ptr(indices), _ptr(self_ids), _ptr(rowmap), _ptr(x),
                                     x.stride(0) if x is not None else 0, _ptr(W), W.stride(0), _ptr(b), n, n_pad, H, out,
                                     int(relu_in), int(relu_out), _ptr(cat), cat.stride(0) if cat is not None else 0,
                                     _ptr(y), y.stride(0), _ptr(wpack), aggr._stream())


def _check(lib, g, x, W, b, n_pad, relu_in=False, relu_out=True, rowmap=None, exact=False, x_ref=None, what=""):
    """run with and without the operand output, compare with float64; returns (y, cat) on the device"""
    indptr, indices, self_ids = g
    n, H, out = indptr.shape[0] - 1, x.shape[1], W.shape[0]
    d = [_i32(indptr), _i32(indices) if indices.shape[0] else None, _i32(self_ids), _i32(rowmap)]
    xd = x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    Wd, bd = torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda()
    y = torch.full((n_pad, out), 7.5, device="cuda")
    cat = torch.full((n_pad, 2 * H), 7.5, device="cuda")
    assert _call(lib, *d, xd, Wd, bd, n, n_pad, H, out, relu_in, relu_out, cat, y) == 0
    y2 = torch.full((n_pad, out), 7.5, device="cuda")
    assert _call(lib, *d, xd, Wd, bd, n, n_pad, H, out, relu_in, relu_out, None, y2) == 0
    torch.cuda.synchronize()
    if x_ref is None:
        cr = R.operand(x, indptr, indices, self_ids, n_pad, rowmap=rowmap, relu_in=relu_in)
    else:       # (a table too large to restate: x_ref holds the rows the map names, in source order)
        cr = R.operand(x_ref, indptr, indices, self_ids, n_pad, relu_in=relu_in)
    yr = R.layer_out(cr, W, b, relu_out)
    if exact:
        assert torch.equal(cat.cpu().double(), cr), what
        assert torch.equal(y.cpu().double(), yr), what
    else:
        torch.testing.assert_close(cat.cpu().double(), cr, msg=lambda m: what + " cat: " + m, **TOL)
        torch.testing.assert_close(y.cpu().double(), yr, msg=lambda m: what + " y: " + m, **TOL)
    assert bool((cat[n:] == 0).all()), what
    assert torch.equal(y2, y), what + ": want_cat=False differs in y"
    return y, cat


# ---- row lengths: both sides of every producer switch, of EMAX and of 3 EC ------------------------------------------

@pytest.mark.parametrize("longest", [0, 1, 6, 7, 12, 13, 16, 17, 18, 19, 40])
@pytest.mark.parametrize("H", [100, 132])
def test_row_lengths_on_both_sides_of_every_producer_switch(lib, longest, H):
    rng = np.random.default_rng(1000 * H + longest)
    n, n_src, out = 77, 60, 40                      # n is not a multiple of 32
    for extra in (0, 1, 31, 70):                    # n_pad - n: none, one row, a tile less one, more than a tile
        deg = rng.integers(0, longest + 1, size=n)
        deg[[2, 40, 76]] = longest                  # the switch value itself, in the first, a middle and the last row
        deg[[3, 41]] = max(longest - 1, 0)
        g = _graph(rng, deg, n_src)
        g[2][2] = -1                                # a longest row without a self row, and one with
        g[2][40] = 7
        x = rng.standard_normal((n_src, H)).astype(np.float32)
        W, b = _weights(rng, H, out)
        _check(lib, g, x, W, b, n + extra, relu_in=bool(extra & 1), what="longest %d pad %d" % (longest, extra))


# ---- S >= 2: a workgroup owns several tiles, the staged-address buffers rotate --------------------------------------

def _path_degrees(rng, n, path):
    """row lengths that put (nearly) every workgroup on the named producer path: short rows, and in one row of ten a
    length from the path's own range"""
    lo, hi = {1: (4, EC), 2: (EC + 1, 2 * EC), 3: (2 * EC + 1, EMAX), 0: (EMAX + 1, 23)}[path]
    deg = rng.integers(0, 4, size=n)
    pick = rng.random(n) < 0.1
    deg[pick] = rng.integers(lo, hi + 1, size=int(pick.sum()))
    deg[[5, n - 1]] = hi
    return deg


_MULTI = ([(S, path, 100, relu, mapped) for S in (2, 3, 4) for path in (1, 2, 3, 0) for relu in (False, True)
           for mapped in ((S + path + relu) % 2 == 0,)] +
          [(S, path, H, (S + path) % 2 == 1, H == 104) for S in (2, 3, 4) for path in (1, 2, 3, 0) for H in (104, 128)] +
          [(S, path, H, (S + path // 2) % 2 == 0, H == 256) for S in (2, 3, 4) for path in (1, 0) for H in (132, 256)])


@pytest.mark.parametrize("S,path,H,relu_in,mapped", _MULTI)
def test_workgroups_that_own_several_tiles(lib, S, path, H, relu_in, mapped):
    """n_pad so large that workgroups own S tiles and some S - 1 (a partial last round): S = 2, 3, 4 put a workgroup's
    last tile on each of the three staged-address buffers.  path: the producer (1, 2, 3 edge passes, 0 generic; H > 128 is
    generic whatever the rows are, with short and with long rows)."""
    cus = _cus()
    rng = np.random.default_rng(S * 1000 + path * 100 + H)
    n_tiles = (S - 1) * cus + max(3, cus // 3)
    n = n_tiles * BM - 13
    n_pad = n + 11                                   # the last tile is cut by n and by n_pad
    n_src, out = 5000, 40
    g = _graph(rng, _path_degrees(rng, n, path), n_src, no_self_every=7)
    rowmap = rng.permutation(9000)[:n_src] if mapped else None
    x = rng.standard_normal((9000 if mapped else n_src, H)).astype(np.float32)
    W, b = _weights(rng, H, out)
    assert -(-n_pad // BM) == n_tiles and n_tiles > (S - 1) * cus and n_tiles < S * cus
    _check(lib, g, x, W, b, n_pad, relu_in=relu_in, relu_out=not relu_in, rowmap=rowmap,
           what="S %d path %d H %d" % (S, path, H))


# ---- mixed paths in one launch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("long_row", [7, 13, 17, 40])
@pytest.mark.parametrize("where", ["first tile", "last tile", "second tile of a workgroup"])
def test_one_long_row_changes_only_its_workgroups_path(lib, long_row, where):
    """every row short (one pass) except ONE: only the workgroup that owns its tile takes another producer, and all of
    that workgroup's tiles, and everybody else's, must still be right"""
    cus = _cus()
    rng = np.random.default_rng(long_row)
    n_tiles = 2 * cus + 7
    n = n_tiles * BM - 5
    tile = {"first tile": 0, "last tile": n_tiles - 1, "second tile of a workgroup": cus + 3}[where]
    deg = rng.integers(0, EC, size=n)
    deg[tile * BM + 9] = long_row
    n_src = 3000
    g = _graph(rng, deg, n_src, no_self_every=6)
    rowmap = rng.permutation(4000)[:n_src]
    x = rng.standard_normal((4000, 100)).astype(np.float32)
    W, b = _weights(rng, 100, 47)
    _check(lib, g, x, W, b, n + 5, rowmap=rowmap, what="%d edges in the %s" % (long_row, where))


# ---- consumer splits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [4, 60, 64, 68, 96, 100, 128, 132, 256, WIDEST])
@pytest.mark.parametrize("out", [1, 31, 32, 33, 64, 65, 255, 256])
def test_every_split_of_w_and_every_column_tile_parity(lib, H, out):
    """KQ = H/4 in {1, 15 | 16 | 17, 32, 33, 64, 69 | 24 | 25} x 1 .. 8 column tiles (odd counts leave half a wave's pair
    empty): exact on small integers (degrees 0, 1, 2, 4), 1e-5 on random data with rows up to 9 edges"""
    rng = np.random.default_rng(100 * H + out)
    n, n_src, n_pad = 205, 90, 224
    g = _graph(rng, rng.choice([0, 1, 2, 4], size=n), n_src)
    x = rng.integers(-3, 4, size=(n_src, H)).astype(np.float32)
    W, b = _weights(rng, H, out, integers=True)
    _check(lib, g, x, W, b, n_pad, relu_out=False, exact=True, what="integers")
    g = _graph(rng, rng.integers(0, 10, size=n), n_src)
    x = rng.standard_normal((n_src, H)).astype(np.float32)
    W, b = _weights(rng, H, out)
    _check(lib, g, x, W, b, n_pad, relu_in=True, what="random")


def test_widest_accepted_width_is_what_the_kernel_accepts(lib):
    assert lib.csl_sage_fwd_mfma_scratch(WIDEST, 256) > 0 and lib.csl_sage_fwd_mfma_scratch(WIDEST + 4, 1) == E_INVALID


# ---- strides ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,longest", [(100, 5), (100, 14), (132, 5), (128, 30)])
def test_column_blocks_of_wider_buffers(lib, H, longest):
    """x, cat and y as column blocks of wider 16-byte-aligned buffers (ldx > H, ldc > 2 H, ldy > out): same numbers, and
    not one float outside the blocks or below row n_pad is touched"""
    rng = np.random.default_rng(H + longest)
    n, n_src, out, n_pad = 300, 120, 47, 311           # (the last tile holds rows beyond n_pad)
    g = _graph(rng, rng.integers(0, longest + 1, size=n), n_src)
    x = rng.standard_normal((n_src, H)).astype(np.float32)
    W, b = _weights(rng, H, out)
    xw = torch.full((n_src, H + 12), 3.25, device="cuda")
    xw[:, 4:4 + H] = torch.from_numpy(x).cuda()
    Ww = torch.full((out, 2 * H + 8), -2.5, device="cuda")
    Ww[:, :2 * H] = torch.from_numpy(W).cuda()
    S = 9.75
    catw = torch.full((n_pad + 40, 2 * H + 8), S, device="cuda")
    yw = torch.full((n_pad + 40, out + 9), S, device="cuda")
    d = [_i32(g[0]), _i32(g[1]), _i32(g[2]), None]
    for want_cat in (True, False):
        yw.fill_(S)
        rc = _call(lib, *d, xw[:, 4:4 + H], Ww[:, :2 * H], torch.from_numpy(b).cuda(), n, n_pad, H, out, False, True,
                   catw[:n_pad, 4:4 + 2 * H] if want_cat else None, yw[:n_pad, 3:3 + out])
        assert rc == 0
        torch.cuda.synchronize()
        cr = R.operand(x, *g, n_pad)
        yr = R.layer_out(cr, W, b, True)
        torch.testing.assert_close(yw[:n_pad, 3:3 + out].cpu().double(), yr, **TOL)
        assert bool((yw[:, :3] == S).all()) and bool((yw[:, 3 + out:] == S).all()) and bool((yw[n_pad:] == S).all())
    torch.testing.assert_close(catw[:n_pad, 4:4 + 2 * H].cpu().double(), cr, **TOL)
    assert bool((catw[:, :4] == S).all()) and bool((catw[:, 4 + 2 * H:] == S).all()) and bool((catw[n_pad:] == S).all())


# ---- a feature table beyond 4 GB -------------------------------------------------------------------------------------

@pytest.mark.parametrize("longest", [5, 20])
def test_feature_rows_on_both_sides_of_the_4_gb_line(lib, longest):
    """the staged entries are 64-bit addresses: a row map into a table of more than 2^32 bytes, sources on both sides of
    the line (the table is allocated, not filled: only the rows the case reads are written)"""
    H, out, n, n_src = 128, 33, 2500, 3000
    line = (1 << 32) // (4 * H)                      # the first row that starts at or beyond 2^32 bytes
    rows = line + (1 << 19)
    rng = np.random.default_rng(longest)
    rowmap = np.concatenate([rng.choice(line - 2, size=n_src // 2 - 2, replace=False),
                             [line - 2, line - 1, line, line + 1],
                             line + 2 + rng.choice(rows - line - 2, size=n_src // 2 - 2, replace=False)])
    rowmap = rowmap[rng.permutation(n_src)].astype(np.int64)
    table = torch.empty((rows, H), dtype=torch.float32, device="cuda")
    assert table.numel() * 4 > (1 << 32)
    x_ref = rng.standard_normal((n_src, H)).astype(np.float32)
    table[torch.from_numpy(rowmap).cuda()] = torch.from_numpy(x_ref).cuda()
    g = _graph(rng, rng.integers(0, longest + 1, size=n), n_src)
    W, b = _weights(rng, H, out)
    _check(lib, g, table, W, b, 2528, rowmap=rowmap, x_ref=x_ref, what="4 GB table")
    del table
    torch.cuda.empty_cache()


# ---- no rows at all --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("relu_out", [False, True])
def test_a_tile_of_padding_only(lib, relu_out):
    H, out = 100, 47
    rng = np.random.default_rng(0)
    W, b = _weights(rng, H, out)
    y = torch.full((32, out), 7.5, device="cuda")
    cat = torch.full((32, 2 * H), 7.5, device="cuda")
    rc = _call(lib, None, None, None, None, None, torch.from_numpy(W).cuda(), torch.from_numpy(b).cuda(), 0, 32, H, out,
               False, relu_out, cat, y)
    assert rc == 0
    torch.cuda.synchronize()
    want = torch.from_numpy(b).clamp_min(0) if relu_out else torch.from_numpy(b)
    assert bool((cat == 0).all()) and torch.equal(y.cpu(), want.expand(32, -1))


# ---- refusals: the return code only, nothing is launched -------------------------------------------------------------

def test_refusals(lib):
    n, n_src, H, out = 8, 8, 8, 4
    ip = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    ix = torch.zeros(n, dtype=torch.int32, device="cuda")
    sid = torch.zeros(n, dtype=torch.int32, device="cuda")
    wpack = torch.zeros((1 << 20,), device="cuda")          # room for any width below: the refusal is not about the scratch
    big = torch.zeros((1 << 16,), device="cuda")

    def run(H=H, out=out, x_off=0, w_off=0, cat_off=0, ldc=None, ldx=None, want_cat=True):
        x = big[x_off:x_off + n_src * H].view(n_src, H)
        W = big[w_off:w_off + out * 2 * H].view(out, 2 * H)
        cat = big[cat_off:cat_off + n * 2 * H].view(n, 2 * H) if want_cat else None
        y = torch.zeros((n, out), device="cuda")
        return _call(lib, ip, ix, sid, None, x, W, None, n, n, H, out, False, False, cat, y, wpack=wpack)

    assert lib.csl_sage_fwd_mfma_scratch(WIDEST + 4, 64) == E_INVALID and run(H=WIDEST + 4) == E_INVALID
    assert lib.csl_sage_fwd_mfma_scratch(8, 257) == E_INVALID and run(out=257) == E_INVALID
    assert run(w_off=1) == E_INVALID          # W four bytes off a 16-byte boundary
    assert run(x_off=1) == E_INVALID
    assert run(cat_off=1) == E_INVALID
    assert run(H=6) == E_INVALID
    assert run() == 0                         # (the same call with nothing wrong)
    torch.cuda.synchronize()
