"""Full-neighbour inference over a 16-bit feature table (include/cslicer_infer16.h), the part that needs no GPU: the
header is bound, the library exports its four entry points, each refuses bad arguments before any HIP call, and the
memory accounting of cslicer.infer counts what is allocated for each of the three element types."""
import ctypes as C

import pytest
import torch

F16, BF16 = 1, 2            # CSL_FEAT_F16, CSL_FEAT_BF16
INVALID = -1                # CSL_E_INVALID
NAMES = ["csl_infer_sage_x16", "csl_infer_sage_part_x16", "csl_infer_sage_merge_x16", "csl_upcast_rows_x16"]


def _r4(x):
    return (x + 3) // 4 * 4


def test_the_header_is_bound_and_exported():
    from cslicer import _abi, infer
    L = _abi.load()
    assert "cslicer_infer16.h" in _abi.HEADERS
    assert infer.FEAT16_SYMBOLS == NAMES == _abi.BOUND["cslicer_infer16.h"]
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    for n in NAMES:
        assert hasattr(L, n) and getattr(L, n).restype is C.c_int
    # `kind` directly after the table pointer, strides in elements after it
    assert L.csl_upcast_rows_x16.argtypes == [vp, i32, i64, i64, vp, i64, i32, vp]
    f32 = L.csl_infer_sage_f32.argtypes
    assert L.csl_infer_sage_x16.argtypes == f32[:9] + [i32] + f32[9:]
    f32 = L.csl_infer_sage_part_f32.argtypes
    assert L.csl_infer_sage_part_x16.argtypes == f32[:9] + [i32] + f32[9:]
    f32 = L.csl_infer_sage_merge_f32.argtypes
    assert L.csl_infer_sage_merge_x16.argtypes == f32[:6] + [i32] + f32[6:]
    # nothing was added to the headers whose entry points tests/test_abi.py counts
    assert not set(NAMES) & set(infer.SYMBOLS + infer.PARTS_SYMBOLS)


# pointers that are never dereferenced: every call below must return before any HIP call
P = 0x10000          # 16-byte aligned
NULL = None


def _sage(L, x=P, kind=F16, ldx=8, W=8, proj=0, out=P, ldo=16, n_items=4):
    return L.csl_infer_sage_x16(P, P, P, n_items, NULL, 0, 0, 0, x, kind, ldx, W, proj, NULL, 0, NULL, out, ldo, NULL)


def _part(L, y=P, kind=BF16, ldy=8, W=8, pack=1, n_items=4):
    return L.csl_infer_sage_part_x16(P, P, P, n_items, NULL, 0, 0, 0, y, kind, ldy, W, pack, NULL, P, NULL)


def _merge(L, x=P, kind=F16, ldx=8, W=8, proj=0, ldo=16, n=4):
    return L.csl_infer_sage_merge_x16(P, P, n, 3, P, x, kind, ldx, W, proj, NULL, 0, P, ldo, NULL)


def _upcast(L, src=P, kind=BF16, lds=8, n=4, dst=P, ldd=8, H=8):
    return L.csl_upcast_rows_x16(src, kind, lds, n, dst, ldd, H, NULL)


@pytest.mark.parametrize("call", [_sage, _part, _merge, _upcast], ids=lambda f: f.__name__)
def test_bad_tables_are_refused_without_a_device(call):
    from cslicer import _abi
    L = _abi.load()
    table = {"_sage": "x", "_part": "y", "_merge": "x", "_upcast": "src"}[call.__name__]
    stride = {"_sage": "ldx", "_part": "ldy", "_merge": "ldx", "_upcast": "lds"}[call.__name__]
    count = "n" if call in (_merge, _upcast) else "n_items"
    for n in (4, 0):                                            # (a bad table is refused even when there is nothing to do)
        assert call(L, kind=0, **{count: n}) == INVALID
        assert call(L, kind=3, **{count: n}) == INVALID
        assert call(L, **{table: NULL, count: n}) == INVALID
        assert call(L, **{stride: 10, count: n}) == INVALID      # >= W, but no multiple of 4
        for off in (2, 4, 6, 12):
            assert call(L, **{table: P + off, count: n}) == INVALID, off   # a base that is not 8-byte aligned


def test_what_the_float32_twins_refuse_is_refused():
    from cslicer import _abi
    L = _abi.load()
    assert _sage(L, proj=1, ldx=16) == INVALID and _sage(L, proj=1, ldx=16, n_items=0) == INVALID
    assert _merge(L, proj=1) == INVALID and _merge(L, proj=1, n=0) == INVALID
    assert _sage(L, W=6) == INVALID and _sage(L, ldx=4) == INVALID and _sage(L, ldo=12) == INVALID
    assert _sage(L, out=NULL) == INVALID and _sage(L, out=P + 8) == INVALID
    assert _sage(L, n_items=-1) == INVALID
    assert _part(L, W=6) == INVALID and _part(L, ldy=4) == INVALID and _part(L, pack=0) == INVALID
    assert _merge(L, W=2) == INVALID and _merge(L, ldx=4) == INVALID and _merge(L, ldo=8) == INVALID
    assert _upcast(L, H=6) == INVALID and _upcast(L, H=0) == INVALID and _upcast(L, lds=4) == INVALID
    assert _upcast(L, ldd=4) == INVALID and _upcast(L, ldd=10) == INVALID and _upcast(L, n=-1) == INVALID
    assert _upcast(L, dst=NULL) == INVALID and _upcast(L, dst=P + 8) == INVALID
    # nothing to do, table in order (8-byte aligned is enough): CSL_OK without a launch
    assert _upcast(L, src=P + 8, n=0) == 0
    assert _sage(L, x=P + 8, n_items=0) == 0 and _part(L, y=P + 8, n_items=0) == 0 and _merge(L, x=P + 8, n=0) == 0


# ---- memory accounting --------------------------------------------------------------------------------------------------

def _models():
    from cslicer import splitgnn
    return {"sage_agg": splitgnn.DistSAGEModel(100, 128, 7, n_layers=3),     # 100 -> 128 aggregate first
            "sage_proj": splitgnn.DistSAGEModel(100, 32, 7, n_layers=3),     # 100 -> 32 project first
            "sage_odd": splitgnn.DistSAGEModel(50, 32, 7, n_layers=2),       # width 50: tables of 52 columns
            "gat": splitgnn.DistGATModel(100, 8, 7, heads=4, n_layers=2)}


def _layers(model, N, n_out, F, chunk, parts):
    """per layer (floats of everything but the input table, input width, whether the library GEMM reads the input),
    written out from the allocations of _sage_layer / _gat_layer"""
    from cslicer import splitgnn
    out, w = [], _r4(F)
    L = len(model.convs)
    for k, conv in enumerate(model.convs):
        rows = n_out if k + 1 == L else N
        if isinstance(model, splitgnn.DistSAGEModel):
            out_w, in_w = conv.fc.weight.shape[0], conv.fc.weight.shape[1] // 2
            op = _r4(out_w)
            if out_w >= in_w:
                out.append((rows * op + min(chunk, rows) * 2 * w + parts * w, w, False))
            else:
                out.append((rows * op + N * 2 * op + parts * op, w, True))
            w = op
        else:
            Cz = conv.H * _r4(conv.D)
            res = n_out * model.n_classes if k + 1 == L else N * Cz
            out.append((N * Cz + 2 * N * conv.H + res + parts * (Cz + 2 * conv.H + 4), w, True))
            w = Cz
    return out


@pytest.mark.parametrize("name", ["sage_agg", "sage_proj", "sage_odd", "gat"])
@pytest.mark.parametrize("chunk", [256, 1 << 16])
def test_need_bytes_counts_what_is_allocated(name, chunk):
    from cslicer import infer
    model = _models()[name]
    N, n_out, parts = 5000, 700, 6
    F = model.convs[0].fc.weight.shape[1] // (2 if name.startswith("sage") else 1)
    lay = _layers(model, N, n_out, F, chunk, parts)
    up = min(chunk, N) * _r4(F) * 4
    f32 = max(4 * rest + N * w * 4 for rest, w, _ in lay)
    want = {}
    for copy in (False, True):
        first = 4 * lay[0][0] + (N * lay[0][1] * 2 if copy else 0) + (up if lay[0][2] else 0)
        want[copy] = max([first] + [4 * rest + N * w * 4 for rest, w, _ in lay[1:]])
    assert infer._need_bytes(model, N, n_out, F, chunk, parts) == f32                       # float32: as it was
    assert infer._need_bytes(model, N, n_out, F, chunk, parts, 4, True) == f32
    assert infer._need_bytes(model, N, n_out, F, chunk, parts, 2, False) == want[False]
    assert infer._need_bytes(model, N, n_out, F, chunk, parts, 2, True) == want[True]
    # in place: never more than the float32 in-place figure plus the upcast buffer, and the float32 working copy
    # (N round4(F) 4 bytes on top of the float32 figure, as an uploaded float32 table costs) is gone
    assert want[False] <= f32 + up and want[True] <= f32 + up
    assert want[True] < f32 + N * _r4(F) * 4


class _Plan(object):
    """what _need_bytes_parts reads of a PartsPlan"""

    def __init__(self, m, chunk_rows, chunks):
        self.m, self.chunk_rows, self._chunks = m, chunk_rows, chunks

    def chunks(self):
        return self._chunks


@pytest.mark.parametrize("name", ["sage_agg", "sage_proj", "gat"])
def test_need_bytes_parts_counts_what_is_allocated(name):
    from cslicer import infer, splitgnn
    model = _models()[name]
    n_own, chunk, F = 3000, 512, 100
    #        s0  s1   i0 i1 h0 h1 p0 parts o0  o1   r0 r1
    hid = _Plan(3000, chunk, [(0, 400, 0, 0, 0, 0, 0, 5, 0, 512, 0, 900), (400, 700, 0, 0, 0, 0, 5, 2, 512, 3000, 900, 1300)])
    last = _Plan(250, chunk, [(0, 120, 0, 0, 0, 0, 0, 0, 0, 250, 0, 300)])
    w, lay = _r4(F), []
    L = len(model.convs)
    for k, conv in enumerate(model.convs):
        pp = last if k + 1 == L else hid
        S = max(c[1] - c[0] for c in pp.chunks())
        R = max(c[11] - c[10] for c in pp.chunks())
        parts = max([c[7] for c in pp.chunks()] + [1])
        if isinstance(model, splitgnn.DistSAGEModel):
            out_w, in_w = conv.fc.weight.shape[0], conv.fc.weight.shape[1] // 2
            op = _r4(out_w)
            if out_w >= in_w:
                lay.append((pp.m * op + min(chunk, pp.m) * 2 * w + (S + R + parts) * w, w, False))
            else:
                lay.append((pp.m * op + n_own * 2 * op + (S + R + parts) * op, w, True))
            w = op
        else:
            Cz = conv.H * _r4(conv.D)
            pld = Cz + 2 * conv.H + 4
            lay.append((n_own * Cz + 2 * n_own * conv.H + pp.m * Cz + (S + R + parts) * pld + S * conv.H, w, True))
            w = Cz
    up = min(chunk, n_own) * _r4(F) * 4
    f32 = max(4 * rest + n_own * w_ * 4 for rest, w_, _ in lay)
    assert infer._need_bytes_parts(model, n_own, F, (hid, last)) == f32
    for copy in (False, True):
        first = 4 * lay[0][0] + (n_own * lay[0][1] * 2 if copy else 0) + (up if lay[0][2] else 0)
        want = max([first] + [4 * rest + n_own * w_ * 4 for rest, w_, _ in lay[1:]])
        assert infer._need_bytes_parts(model, n_own, F, (hid, last), 2, copy) == want
        assert want <= f32 + up


def test_which_inputs_count_as_16_bit():
    import numpy as np
    from cslicer import infer
    assert infer._feat16_dtype(torch.zeros((2, 4), dtype=torch.float16)) == torch.float16
    assert infer._feat16_dtype(torch.zeros((2, 4), dtype=torch.bfloat16)) == torch.bfloat16
    assert infer._feat16_dtype(np.zeros((2, 4), dtype=np.float16)) == torch.float16
    for other in (torch.zeros((2, 4)), np.zeros((2, 4), dtype=np.float32), np.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.float64)):
        assert infer._feat16_dtype(other) is None
    # a host table is never "in place"
    assert infer._feat16_in_place(torch.zeros((2, 4), dtype=torch.float16), True) is None
