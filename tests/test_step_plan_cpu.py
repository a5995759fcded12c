"""cslicer.train.step_plan: which of its four ways a trainer trains a minibatch, the engine flags that way needs,
whether the attention model's deepest layer is the input layer and the form of the autograd paths' input matrix -- as a
table of configurations with the expected values written out, no device, no engine.  (aggr.gat_input_ok
asks the built library for its degree limit.)"""
import pytest

from cslicer import _abi
from cslicer.train import Switches, step_plan

T, A, NR = _abi.FLAG_TRANSPOSE, _abi.FLAG_TRANSPOSE_ALL, _abi.FLAG_NO_REPLACE

# sage on one GPU, two layers, widths that are multiples of 4, a float32 table, every switch off
BASE = dict(kind="sage", world=1, rank_path=False, n_layers=2, F=24, hidden=32, n_classes=5, heads=4, fanout=5,
            table_f32=True, gat_input=None, replace=True, width_known=True,
            no_transpose=False, py_step=False, no_local_fuse=False, no_gat_input=False)
RANKS = dict(world=2, rank_path=True)
GAT = dict(kind="gat")

# (row of the issue's table, what it changes, engine flags, path, gat_input, input_form)
ROWS = [
    (1, {}, T, "native", False, None),
    (2, dict(py_step=True), T, "local", False, None),
    (3, dict(no_transpose=True), 0, "local", False, None),
    (4, dict(n_layers=1), 0, "local", False, None),
    (5, dict(hidden=30), T, "local", False, None),
    (6, dict(F=22), T, "parts", False, "rows"),
    (7, dict(no_local_fuse=True), T, "parts", False, "rows"),
    (8, RANKS, T, "native_rank", False, None),
    (9, dict(RANKS, n_layers=1), 0, "native_rank", False, None),
    (10, dict(RANKS, n_classes=300), T, "parts", False, "rows"),    # (the slices by source are asked for, not read)
    (11, dict(RANKS, py_step=True), 0, "parts", False, "rows"),
    (12, dict(RANKS, no_transpose=True), 0, "native_rank", False, None),
    (13, dict(world=1, rank_path=True), T, "native_rank", False, None),
    (14, dict(world=2, rank_path=False), 0, "parts", False, "rows"),
    (15, GAT, T, "parts", True, "table"),
    (16, dict(GAT, table_f32=False), T | A, "parts", False, "padded"),
    (17, dict(GAT, table_f32=False, gat_input=True), T, "parts", True, "table"),
    (18, dict(GAT, gat_input=False), T | A, "parts", False, "padded"),
    (19, dict(GAT, no_transpose=True), 0, "parts", False, "padded"),
    (20, dict(GAT, no_local_fuse=True), T | A, "parts", False, "rows"),
    (21, dict(GAT, no_gat_input=True), T | A, "parts", False, "padded"),
    (22, dict(GAT, heads=3), T | A, "parts", False, "padded"),
    (23, dict(GAT, width_known=False), T | A, "parts", False, "padded"),
    (24, dict(GAT, **RANKS), 0, "parts", False, "rows"),
    # row 25: rows 1, 8 and 15 without replacement
    (251, dict(replace=False), T | NR, "native", False, None),
    (258, dict(RANKS, replace=False), T | NR, "native_rank", False, None),
    (2515, dict(GAT, replace=False), T | NR, "parts", True, "table"),
]


def test_switches_are_read_when_asked_for(monkeypatch):
    """not at import of cslicer.train: the tests set them per trainer"""
    from cslicer import splitgnn, train
    for name in ("CSLICER_NO_TRANSPOSE", "CSLICER_PY_STEP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", False)
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", False)
    assert train.read_switches() == Switches(False, False, False, False) == Switches()
    monkeypatch.setenv("CSLICER_PY_STEP", "1")
    monkeypatch.setattr(splitgnn, "_NO_GAT_INPUT", True)
    assert train.read_switches() == Switches(no_transpose=False, py_step=True, no_local_fuse=False, no_gat_input=True)
    monkeypatch.setenv("CSLICER_NO_TRANSPOSE", "1")
    monkeypatch.setattr(splitgnn, "_NO_LOCAL_FUSE", True)
    assert train.read_switches() == Switches(True, True, True, True)


def test_the_flag_values():
    assert (T, A, NR) == (4, 8, 16) and len({r[0] for r in ROWS}) == len(ROWS) == 27


@pytest.mark.parametrize("row,change,flags,path,gat_input,input_form", ROWS, ids=["row%d" % r[0] for r in ROWS])
def test_step_plan(row, change, flags, path, gat_input, input_form):
    cfg = dict(BASE, **change)
    sw = Switches(**{k: cfg.pop(k) for k in Switches._fields})
    plan = step_plan(sw=sw, **cfg)
    assert plan.gat_input is gat_input        # (a bool, always)
    assert tuple(plan) == (flags, path, gat_input, input_form)
    assert (plan.engine_flags, plan.path, plan.gat_input, plan.input_form) == tuple(plan)
