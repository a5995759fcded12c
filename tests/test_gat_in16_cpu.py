"""CPU-side checks of the attention input layer over a 16-bit feature table: the C ABI of include/cslicer_gat_in16.h
(symbols, argument checks that return before any HIP call, parity with the float32 entry points on refused and
nothing-to-do arguments) and the trainer's gat_input argument, which is checked before anything touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cslicer import _abi, aggr, infer, l0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["csl_gat_in_fwd_x16", "csl_gat_in_bwd_x16", "csl_gat_in_layer_fwd_x16", "csl_gat_in_layer_bwd_x16"]
F16, BF16 = 1, 2
null, st = C.c_void_p(0), C.c_void_p(0)
tab, odd = C.c_void_p(0x1000), C.c_void_p(0x1004)      # never dereferenced: every call below is refused or has nothing to do


def test_the_header_declares_the_four_twins():
    L = _abi.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cslicer_gat_in16.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(csl_[a-z_0-9]+)\s*\(", src)))
    assert names == sorted(NAMES)
    assert "cslicer_gat_in16.h" in _abi.HEADERS
    assert aggr.GAT_IN16_SYMBOLS == NAMES == _abi.BOUND["cslicer_gat_in16.h"]
    for n in NAMES:
        assert hasattr(L, n), "libcslicer_hip.so does not export %s" % n
        twin = getattr(L, n.replace("_x16", "_f32"))
        # the twin's prototype with `kind` (int32) directly after the table pointer, the fifth argument
        assert list(getattr(L, n).argtypes) == list(twin.argtypes[:5]) + [C.c_int32] + list(twin.argtypes[5:]), n
        assert getattr(L, n).restype is twin.restype
    others = (set(aggr.SYMBOLS) | set(aggr.FEAT16_SYMBOLS) | set(_abi.SYMBOLS) | set(infer.SYMBOLS) | set(infer.PARTS_SYMBOLS)
              | set(infer.FEAT16_SYMBOLS))
    assert not set(NAMES) & others
    # the neighbouring headers kept their counts: the comment that points here is not a declaration
    assert len(aggr.FEAT16_SYMBOLS) == 6 and len(aggr.SYMBOLS) == 66


# ---- the four pairs, every argument with a default that passes the checks (dummy aligned pointers, H = 8, F = 100,
# D = 32, ten rows of at most ten edges).  kind None: the float32 entry point.

def _call(stem, kind, x, ldx, rest):
    L = aggr._lib()
    fn = getattr(L, "csl_%s_%s" % (stem, "f32" if kind is None else "x16"))
    table = (x, ldx) if kind is None else (x, kind, ldx)
    return fn(tab, tab, tab, null, *table, *rest)


def fwd(kind, x=tab, ldx=None, F=100, vl=tab, vr=tab, H=8, n_out=10, n_edges=10, max_deg=10, agg=tab, alpha=tab):
    return _call("gat_in_fwd", kind, x, F if ldx is None else ldx, (F, vl, vr, H, 0.2, n_out, n_edges, max_deg, agg, alpha, st))


def bwd(kind, x=tab, ldx=None, F=100, alpha=tab, dagg=tab, ld_r=None, ld_h=None, H=8, n_out=10, n_edges=10, max_deg=10,
        g_vl=tab, g_vr=tab, scratch=tab):
    ld_h = F if ld_h is None else ld_h
    return _call("gat_in_bwd", kind, x, F if ldx is None else ldx,
                 (F, alpha, dagg, H * ld_h if ld_r is None else ld_r, ld_h, H, 0.2, n_out, n_edges, max_deg, g_vl, g_vr, scratch, st))


def layer_fwd(kind, x=tab, ldx=None, F=100, W=tab, attn=tab, H=8, D=32, n_out=10, n_edges=10, max_deg=10, agg=tab, alpha=tab,
              out=tab, scratch=tab):
    return _call("gat_in_layer_fwd", kind, x, F if ldx is None else ldx,
                 (F, W, attn, attn, tab, H, D, 0.2, 1, n_out, n_edges, max_deg, agg, alpha, out, H * D, scratch, st))


def layer_bwd(kind, x=tab, ldx=None, F=100, W=tab, attn=tab, H=8, D=32, n_out=10, n_edges=10, max_deg=10, agg=tab, alpha=tab,
              dagg=tab, gW=tab, g_vl=tab, scratch=tab):
    return _call("gat_in_layer_bwd", kind, x, F if ldx is None else ldx,
                 (F, W, attn, attn, H, D, 0.2, 1, n_out, n_edges, max_deg, agg, alpha, tab, H * D, tab, H * D, tab, dagg, gW,
                  g_vl, tab, tab, scratch, st))


TWINS = (fwd, bwd, layer_fwd, layer_bwd)


def test_each_twin_refuses_a_bad_table():
    """before any HIP call and whatever the row count: a null table, a stride that is not a multiple of 4 elements, a base
    that is not 8-byte aligned, rows narrower than F, an unknown kind (0 is float32: the _f32 entry points)"""
    for fn in TWINS:
        for n_out in (10, 0):
            for kind in (F16, BF16):
                assert fn(kind, x=null, n_out=n_out) == -1, fn.__name__
                assert fn(kind, ldx=102, n_out=n_out) == -1, fn.__name__
                assert fn(kind, x=odd, n_out=n_out) == -1, fn.__name__
                assert fn(kind, ldx=96, n_out=n_out) == -1, fn.__name__
            for kind in (0, 3, -1):
                assert fn(kind, n_out=n_out) == -1, fn.__name__


def test_parity_with_the_float32_entry_points():
    """Each _f32 entry point and its twin (both kinds) get the same arguments and give the same code.  Every case is
    refused from the arguments alone, or has nothing to do and returns before a HIP call: nothing is launched."""
    edge = [dict(H=3), dict(F=102), dict(F=132), dict(F=0), dict(max_deg=33), dict(max_deg=-1), dict(n_out=-1),
            dict(n_edges=-1), dict(ldx=102)]
    bad = {
        fwd: edge + [dict(vl=null), dict(vr=null), dict(vl=odd), dict(agg=null), dict(agg=odd), dict(alpha=null)],
        bwd: edge + [dict(g_vl=null), dict(g_vr=null), dict(g_vl=odd), dict(scratch=null), dict(scratch=odd), dict(dagg=null),
                     dict(dagg=odd), dict(alpha=null), dict(ld_r=802), dict(ld_h=102),
                     dict(n_out=0, g_vl=null), dict(n_out=0, ld_r=802)],
        # the layer calls: what bd_ok refuses (heads, widths, D), their own null arguments, then the edge pass's list
        layer_fwd: edge + [dict(D=12), dict(D=0), dict(D=128), dict(H=16), dict(F=2), dict(W=null), dict(attn=null),
                           dict(scratch=null), dict(scratch=odd), dict(agg=null), dict(agg=odd), dict(alpha=null)],
        layer_bwd: edge + [dict(D=12), dict(D=0), dict(D=128), dict(H=16), dict(F=2), dict(W=null), dict(attn=null),
                           dict(scratch=null), dict(scratch=odd), dict(gW=null), dict(g_vl=null), dict(dagg=null),
                           dict(dagg=odd), dict(alpha=null), dict(n_out=0, scratch=null), dict(n_out=0, D=12)],
    }
    # nothing to do: the forward returns before it looks at anything but the shape.  (The backward zeroes g_vl / g_vr
    # then -- a HIP call on these dummy pointers -- so its nothing-to-do cases are the refused ones above.)
    ok = {fwd: [dict(n_out=0), dict(n_out=0, n_edges=0), dict(n_out=0, vl=null, agg=null, alpha=null)], bwd: [],
          layer_fwd: [], layer_bwd: []}
    assert [len(bad[f]) + len(ok[f]) for f in TWINS] == [18, 21, 21, 25]
    for fn in TWINS:
        for want, cases in ((0, ok[fn]), (-1, bad[fn])):
            for kw in cases:
                got = [fn(kind, **kw) for kind in (None, F16, BF16)]
                assert got == [want] * 3, (fn.__name__, kw, got)
    # The one difference that is meant: with nothing to do a 16-bit table is still checked, a float32 table is not
    # looked at -- its pointer, that is: null or misaligned.  The float32 forward does check the STRIDE whatever the row
    # count (ldx % 4, ldx >= F sit in its first check, and its return codes are unchanged), so rows narrower than F are
    # refused by all three.
    for kw in (dict(n_out=0, x=null), dict(n_out=0, x=odd)):
        assert [fwd(kind, **kw) for kind in (None, F16, BF16)] == [0, -1, -1], kw
    assert [fwd(kind, n_out=0, ldx=96) for kind in (None, F16, BF16)] == [-1, -1, -1]
    # a base that is 8-byte but not 16-byte aligned is a 16-bit table's right
    assert [fwd(kind, n_out=0, x=C.c_void_p(0x1008)) for kind in (F16, BF16)] == [0, 0]


def _trainer(**kw):
    from cslicer import train
    indptr, indices = l0.synth_graph(40, 3.0, seed=0)
    x = np.zeros((40, 8), dtype=np.float32)
    return train.Trainer(indptr, indices, x, np.zeros(40, dtype=np.int64), 3, fanouts=(2, 2), hidden=16, **kw)


def test_trainer_checks_gat_input_before_any_device_call():
    with pytest.raises(ValueError, match="gat_input"):
        _trainer(model="gat", heads=4, gat_input="yes")
    with pytest.raises(ValueError, match="gat_input"):
        _trainer(model="gat", heads=4, gat_input=1)
    with pytest.raises(ValueError, match="gat_input=True.*model"):
        _trainer(model="sage", gat_input=True)
    with pytest.raises(ValueError, match="gat_input=True.*gat_input_ok"):
        _trainer(model="gat", heads=3, gat_input=True)
    with pytest.raises(ValueError, match="gat_input=True.*gat_input_ok"):
        _trainer(model="gat", heads=4, gat_input=True, feat_dim=6)            # F % 4
    with pytest.raises(ValueError, match="gat_input=True.*more than one part"):
        _trainer(model="gat", heads=4, gat_input=True, world=2)
    with pytest.raises(ValueError, match="gat_input=True.*rank_path"):
        _trainer(model="gat", heads=4, gat_input=True, rank_path=True)
    for dtype in ("float16", "bfloat16"):                                     # (the same answers for a 16-bit table)
        with pytest.raises(ValueError, match="gat_input=True.*gat_input_ok"):
            _trainer(model="gat", heads=3, gat_input=True, feature_dtype=dtype)


def test_trainer_refuses_gat_input_under_the_switches(monkeypatch):
    from cslicer import splitgnn
    monkeypatch.setenv("CSLICER_NO_TRANSPOSE", "1")
    with pytest.raises(ValueError, match="gat_input=True.*CSLICER_NO_TRANSPOSE"):
        _trainer(model="gat", heads=4, gat_input=True)
    monkeypatch.delenv("CSLICER_NO_TRANSPOSE")
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", True)
    with pytest.raises(ValueError, match="gat_input=True.*CSLICER_NO_LOCAL_FUSE"):
        _trainer(model="gat", heads=4, gat_input=True)


def test_command_line():
    from cslicer import train
    assert train._parser().parse_args(["--gat-input", "on"]).gat_input == "on"
    assert train._parser().parse_args(["--gat-input", "off"]).gat_input == "off"
    assert train._parser().parse_args([]).gat_input == "auto"
    with pytest.raises(SystemExit):
        train._parser().parse_args(["--gat-input", "yes"])
