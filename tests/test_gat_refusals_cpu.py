"""The attention aggregation's entry points and their dropped twins (include/cslicer_aggr.h, cslicer_gat_dropout.h) share one
host path per pair (csrc/aggregate.hip); this pins what each member of each pair answers to a bad argument
tuple, without a GPU: ONE table of tuples driven through both members of the six pairs, the expected codes written out.

Only tuples that return before any HIP call are here (no device on this machine), which leaves out for the plain member
* whatever only the dropped member refuses (p, layer, the ids, H > 2^24 with rows to do): the plain call would launch;
* csl_gat_bwd_t_fused_f32 with first-stage rows and a bad second-stage argument: it is refused (CSL_E_INVALID), but the
  library this table was first run against launched its first stage before it looked;
* csl_gat_finish_bwd_f32 with n = 0 (its second stage is launched whatever n is).
`None` in the table marks such a member.  The three places where the two members answer differently (DESIGN 4.11,
"Refusals"): (a) no rows and a bad shape, (b) H > 2^24, (c) the order inside the fused by-source form."""
import ctypes as C

import pytest

OK, INVALID = 0, -1

_buf = (C.c_float * 64)()
_base = (C.addressof(_buf) + 15) // 16 * 16
X, NUL = C.c_void_p(_base), C.c_void_p(0)
OFF4, OFF8 = C.c_void_p(_base + 4), C.c_void_p(_base + 8)       # float-aligned, not 16-byte-aligned
BIG_H = (1 << 24) + 1

ATTN = dict(src_ids=X, dst_ids=X, p=0.5, seed=1, layer=0, step=0)
FEAT = dict(ids=X, p=0.5, seed=1, layer=0, step=0)

# pair -> (plain entry point, dropped entry point, the plain member's arguments in order (all valid), the dropped tail)
PAIRS = {
    "fwd": ("csl_gat_fwd_f32", "csl_gat_drop_fwd_f32",
            dict(indptr=X, indices=X, n_rows=1, el=X, er=X, z=X, H=1, D=4, slope=0.2, m=X, s=X, n=X), ATTN),
    "bwd": ("csl_gat_bwd_f32", "csl_gat_drop_bwd_f32",
            dict(indptr=X, indices=X, n_rows=1, el=X, er=X, z=X, H=1, D=4, slope=0.2, m=X, gs=X, gn=X, gel=X, ger=X, gz=X), ATTN),
    "bwd_t": ("csl_gat_bwd_t_f32", "csl_gat_drop_bwd_t_f32",
              dict(tptr=X, trow=X, n_src=1, n_pad=1, el=X, er=X, z=X, H=1, D=4, slope=0.2, m=X, gs=X, gn=X, gel=X, ger=X, gz=X),
              ATTN),
    "bwd_t_fused": ("csl_gat_bwd_t_fused_f32", "csl_gat_drop_bwd_t_fused_f32",
                    dict(tptr=X, trow=X, n_src=1, n_pad=1, el=X, er=X, z=X, H=1, D=4, slope=0.2, m=X, gs=X, gn=X, al=X, ar=X,
                         sid=X, n_out=1, ger=X, gz=X, gal=X, gar=X, scratch=X), ATTN),
    "finish_fwd": ("csl_gat_finish_fwd_f32", "csl_gat_finish_drop_fwd_f32",
                   dict(n_in=X, s_in=X, bias=X, n=1, H=1, D=4, elu=1, out=X), dict(y=X, **FEAT)),
    "finish_bwd": ("csl_gat_finish_bwd_f32", "csl_gat_finish_drop_bwd_f32",
                   dict(g=X, ldg=4, out=X, n_in=X, s_in=X, n=1, H=1, D=4, elu=1, g_n=X, g_s=X, g_bias=X, scratch=X), FEAT),
}


def _nul(*names):
    return {k: NUL for k in names}


NO_ROWS = dict(n_rows=0, **_nul("indptr", "indices", "el", "er", "z"))
NO_SRC = dict(n_src=0, n_pad=0, **_nul("tptr", "trow", "el", "er", "z", "m", "gs", "gn", "gel", "ger", "gz"))
ATTN_BAD = [dict(p=0.0), dict(p=1.0), dict(p=-0.5), dict(p=float("nan")), dict(layer=-1), dict(layer=256), dict(src_ids=NUL),
            dict(dst_ids=NUL), dict(H=BIG_H)]
FEAT_BAD = [dict(p=0.0), dict(p=1.0), dict(p=float("nan")), dict(ids=NUL), dict(H=BIG_H)]

# (pair, what differs from the valid tuple, the plain member's code, the dropped member's code)
TABLE = (
    # ---- csl_gat_fwd_f32 / csl_gat_drop_fwd_f32
    [("fwd", dict(NO_ROWS, **_nul("m", "s", "n")), OK, OK),
     ("fwd", dict(NO_ROWS, src_ids=NUL, dst_ids=NUL), None, OK),
     ("fwd", dict(NO_ROWS, D=6), OK, INVALID),                      # (a): the plain one answers before it sees the shape
     ("fwd", dict(NO_ROWS, H=0), OK, INVALID),
     ("fwd", dict(NO_ROWS, D=260), OK, INVALID),
     ("fwd", dict(NO_ROWS, H=BIG_H), OK, INVALID),                  # (b)
     ("fwd", dict(NO_ROWS, H=1 << 24), OK, OK),
     ("fwd", dict(NO_ROWS, p=0.0), None, INVALID),
     ("fwd", dict(n_rows=-1), INVALID, INVALID)]
    + [("fwd", bad, INVALID, INVALID) for bad in (
        dict(D=6), dict(D=0), dict(D=260), dict(H=0), dict(H=-3), dict(indptr=NUL), dict(er=NUL), dict(m=NUL), dict(s=NUL),
        dict(n=NUL), dict(z=OFF4), dict(n=OFF8))]
    + [("fwd", bad, None, INVALID) for bad in ATTN_BAD]
    # ---- csl_gat_bwd_f32 / csl_gat_drop_bwd_f32
    + [("bwd", dict(NO_ROWS, **_nul("m", "gs", "gn", "gel", "ger", "gz")), OK, OK),
       ("bwd", dict(NO_ROWS, src_ids=NUL, dst_ids=NUL), None, OK),
       ("bwd", dict(NO_ROWS, D=6), OK, INVALID),                    # (a)
       ("bwd", dict(NO_ROWS, H=0), OK, INVALID),
       ("bwd", dict(NO_ROWS, H=BIG_H), OK, INVALID),                # (b)
       ("bwd", dict(NO_ROWS, layer=256), None, INVALID),
       ("bwd", dict(n_rows=-1), INVALID, INVALID)]
    + [("bwd", bad, INVALID, INVALID) for bad in (
        dict(D=6), dict(D=260), dict(H=0), dict(indptr=NUL), dict(er=NUL), dict(m=NUL), dict(gs=NUL), dict(gn=NUL),
        dict(ger=NUL), dict(z=OFF4), dict(gn=OFF8), dict(gz=OFF8))]
    + [("bwd", bad, None, INVALID) for bad in ATTN_BAD]
    # ---- csl_gat_bwd_t_f32 / csl_gat_drop_bwd_t_f32: both look at the shape before n_pad == 0
    + [("bwd_t", NO_SRC, OK, OK),
       ("bwd_t", dict(NO_SRC, src_ids=NUL, dst_ids=NUL), None, OK),
       ("bwd_t", dict(NO_SRC, D=6), INVALID, INVALID),
       ("bwd_t", dict(NO_SRC, H=0), INVALID, INVALID),
       ("bwd_t", dict(NO_SRC, H=BIG_H), OK, INVALID),               # (b)
       ("bwd_t", dict(NO_SRC, H=1 << 24), OK, OK),
       ("bwd_t", dict(NO_SRC, p=1.0), None, INVALID)]
    + [("bwd_t", bad, INVALID, INVALID) for bad in (
        dict(n_src=-1), dict(n_pad=0), dict(n_src=2), dict(D=6), dict(D=260), dict(H=0), dict(gz=NUL), dict(gz=OFF4),
        dict(tptr=NUL), dict(el=NUL), dict(z=NUL), dict(gel=NUL), dict(z=OFF8), dict(er=NUL), dict(m=NUL), dict(gs=NUL),
        dict(gn=NUL), dict(ger=NUL), dict(gn=OFF4))]
    + [("bwd_t", bad, None, INVALID) for bad in ATTN_BAD]
    # ---- csl_gat_bwd_t_fused_f32 / csl_gat_drop_bwd_t_fused_f32
    + [("bwd_t_fused", bad, INVALID, INVALID) for bad in (
        dict(n_src=-1), dict(n_pad=0), dict(n_out=-1), dict(D=6), dict(D=260), dict(H=0), dict(gal=NUL), dict(gar=NUL),
        dict(n_src=0, n_pad=0, n_out=0, gal=NUL), dict(n_src=0, n_pad=0, n_out=0, D=6),
        dict(gz=NUL), dict(gz=OFF4), dict(scratch=NUL), dict(scratch=OFF8), dict(al=NUL), dict(al=OFF4),
        dict(tptr=NUL), dict(el=NUL), dict(z=NUL), dict(z=OFF4), dict(er=NUL), dict(m=NUL), dict(gs=NUL), dict(gn=NUL),
        dict(gn=OFF8), dict(ger=NUL),
        # the second stage alone (no first-stage rows: nothing is launched ahead of the check in either library)
        dict(n_src=0, n_pad=0, ar=NUL), dict(n_src=0, n_pad=0, ar=OFF4), dict(n_src=0, n_pad=0, sid=NUL))]
    # (c): with first-stage rows the dropped one refuses the second stage's arguments before any HIP call
    + [("bwd_t_fused", bad, None, INVALID) for bad in (
        dict(ar=NUL), dict(ar=OFF8), dict(sid=NUL), dict(n_src=0, n_pad=0, scratch=NUL), dict(n_src=0, n_pad=0, gz=NUL),
        dict(n_src=0, n_pad=0, z=NUL), dict(n_src=0, n_pad=0, ger=NUL))]
    + [("bwd_t_fused", bad, None, INVALID) for bad in ATTN_BAD]
    # ---- csl_gat_finish_fwd_f32 / csl_gat_finish_drop_fwd_f32: both look at the shape before n == 0
    + [("finish_fwd", dict(n=0, **_nul("n_in", "s_in", "bias", "out")), OK, OK),
       ("finish_fwd", dict(n=0, **_nul("n_in", "s_in", "bias", "out", "y", "ids")), None, OK),
       ("finish_fwd", dict(n=0, D=6), INVALID, INVALID),
       ("finish_fwd", dict(n=0, H=BIG_H), OK, INVALID),             # (b)
       ("finish_fwd", dict(n=0, H=1 << 24), OK, OK),
       ("finish_fwd", dict(n=0, p=0.0), None, INVALID)]
    + [("finish_fwd", bad, INVALID, INVALID) for bad in (
        dict(n=-1), dict(D=6), dict(D=260), dict(H=0), dict(n_in=NUL), dict(s_in=NUL), dict(bias=NUL), dict(out=NUL),
        dict(n_in=OFF4), dict(bias=OFF8), dict(out=OFF4))]
    + [("finish_fwd", bad, None, INVALID) for bad in FEAT_BAD + [dict(y=NUL), dict(y=OFF4)]]
    # ---- csl_gat_finish_bwd_f32 / csl_gat_finish_drop_bwd_f32
    + [("finish_bwd", bad, INVALID, INVALID) for bad in (
        dict(n=-1), dict(D=6), dict(D=260), dict(H=0), dict(g_bias=NUL), dict(n=0, g_bias=NUL), dict(n=0, D=6),
        dict(g=NUL), dict(ldg=3), dict(ldg=6), dict(n_in=NUL), dict(s_in=NUL), dict(g_n=NUL), dict(g_s=NUL), dict(scratch=NUL),
        dict(out=NUL), dict(g=OFF4), dict(n_in=OFF8), dict(g_n=OFF4), dict(scratch=OFF4), dict(out=OFF8),
        dict(elu=0, out=OFF8))]
    + [("finish_bwd", bad, None, INVALID) for bad in FEAT_BAD + [dict(n=0, p=0.0)]]
)


@pytest.fixture(scope="module")
def lib():
    from cslicer import _abi
    return _abi.load()


def test_the_table_covers_every_pair_and_every_difference():
    """the table itself: all six pairs, both members of each, the three differences, and no valid tuple (it would launch)"""
    assert {row[0] for row in TABLE} == set(PAIRS)
    for pair in PAIRS:
        rows = [r for r in TABLE if r[0] == pair]
        assert any(r[2] is not None for r in rows) and any(r[3] is not None for r in rows), pair
    differ = {r[0] for r in TABLE if r[2] is not None and r[3] is not None and r[2] != r[3]}
    assert differ == {"fwd", "bwd", "bwd_t", "finish_fwd"}      # (a) and (b); (c) is the `None` rows of bwd_t_fused
    for pair, change, plain, dropped in TABLE:
        assert change and (plain in (None, OK, INVALID)) and (dropped in (OK, INVALID)), (pair, change)
        keys = set(PAIRS[pair][2]) | set(PAIRS[pair][3])
        assert set(change) <= keys, (pair, change)
        if plain is not None:       # a tuple that only changes the dropped member's tail is the valid tuple to the plain one
            assert set(change) & set(PAIRS[pair][2]), (pair, change)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_both_members_answer_the_table(lib, pair):
    plain_name, dropped_name, args, tail = PAIRS[pair]
    plain_fn, dropped_fn = getattr(lib, plain_name), getattr(lib, dropped_name)
    n = 0
    for p_, change, plain, dropped in TABLE:
        if p_ != pair:
            continue
        both = dict(args, **tail)
        both.update(change)
        if plain is not None:
            assert plain_fn(*[both[k] for k in args], NUL) == plain, (plain_name, change)
        if dropped is not None:
            assert dropped_fn(*both.values(), NUL) == dropped, (dropped_name, change)
        n += 1
    assert n >= 10
