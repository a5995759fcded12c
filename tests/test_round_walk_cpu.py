"""shard.round_walk, the one round / slot / submit-ahead rotation behind Trainer.run and Trainer.skip, with no device: a
call is simulated as the trainer makes it (round_plan, the walk from the trainer's (_round_base, _ahead), the state moved
on as run / skip move it), and the stream of ("submit" | "use", round, slot) is checked over call sequences at every
(n_batches, S) of the grid -- whole rounds only, a short tail, a single round, more rounds than slots, an epoch wrap."""
import itertools

import pytest

from cslicer import shard

SLOTS = 3       # Trainer.SLOTS
GRID = list(itertools.product((1, 2, 5, 8, 9, 17), (1, 2, 3, 8)))


def _call(state, n_batches, S, n_steps, first=0, then=None):
    """the walk of run(n_steps, first, then) / skip(n_steps, first) from `state` = [base, ahead], and the state moved on"""
    plan = shard.round_plan(n_batches, S, first, n_steps)
    if not plan:                    # run() returns before it looks at _ahead; skip() submits nothing
        return []
    base, ahead = state
    assert ahead is None or ahead == plan[0]
    nxt = shard.round_plan(n_batches, S, then[0], then[1])[:1] if then else []
    state[:] = [(base + len(plan)) % SLOTS, nxt[0] if nxt else None]
    return list(shard.round_walk(plan, nxt, base, ahead, SLOTS))


def _sequences(nb):
    """call sequences as (n_steps, first_batch, then): run-like and skip-like calls (a skip is a call without `then` that
    no `then` announced), empty calls, a first_batch that wraps the epoch, a then= pair"""
    return [
        [(nb, 0, None)],
        [(5, 0, None), (3, 0, None), (4, 0, None)],
        [(3, 0, (3, 4)), (4, 3, None)],
        [(0, 0, None), (2, 0, None), (0, 5, None), (nb + 2, 1, None)],
        [(4, nb - 1, None), (2 * nb + 1, 3, None)],
        [(nb + 2, 0, None), (3, 2, (5, 2)), (2, 5, (0, 0)), (7, 0, None)],
    ]


@pytest.mark.parametrize("nb,S", GRID)
def test_rotation_over_call_sequences(nb, S):
    for seq in _sequences(nb):
        state, used, waiting = [0, None], 0, []        # waiting: rounds submitted and not yet used, oldest first
        for n_steps, first, then in seq:
            want = shard.round_plan(nb, S, first, n_steps)
            got = []
            for what, entry, slot in _call(state, nb, S, n_steps, first, then):
                if what == "submit":
                    # (c) the slot holds no round that is still to be used; (b) once: nothing is waiting twice
                    assert slot not in [s for _, s in waiting], (seq, entry, slot)
                    waiting.append((entry, slot))
                else:
                    # (b) submitted before it is used, rounds used in the order submitted; (a) global round r in slot r % 3
                    assert what == "use" and waiting and waiting.pop(0) == (entry, slot), (seq, entry, slot)
                    assert slot == used % SLOTS
                    used += 1
                    got.append(entry)
                assert len(waiting) <= 2
            assert got == want                          # the call used exactly its plan
            # between calls only an announced round waits, and it is the next call's first
            assert waiting == ([] if state[1] is None else [(state[1], used % SLOTS)])
        assert state == [used % SLOTS, None] and not waiting


@pytest.mark.parametrize("nb,S", GRID)
def test_a_skip_submits_what_the_run_would(nb, S):
    """(d) run and skip read the same walk, so a call sequence submits the same rounds into the same slots whichever of
    its calls train: stated against the loops run() and skip() each had before the walk (`_old_run`, `_old_skip`)"""
    for seq in _sequences(nb):
        for skipped in range(len(seq) + 1):
            state, old = [0, None], [0, None]
            for i, (n_steps, first, then) in enumerate(seq):
                new = [(e, s) for w, e, s in _call(state, nb, S, n_steps, first, then) if w == "submit"]
                announced = old[1] is not None
                if i == skipped and then is None and not announced:
                    assert new == _old_skip(old, nb, S, n_steps, first)
                else:
                    assert new == _old_run(old, nb, S, n_steps, first, then)
                assert state == old


def _old_run(state, nb, S, n_steps, first, then):
    plan, out = shard.round_plan(nb, S, first, n_steps), []
    if not plan:
        return out
    base, ahead = state
    state[1] = None
    if ahead is None:
        out.append((plan[0], base % SLOTS))
    nxt = shard.round_plan(nb, S, then[0], then[1])[:1] if then else []
    for r in range(len(plan)):
        if r + 1 < len(plan):
            out.append((plan[r + 1], (base + r + 1) % SLOTS))
        elif nxt:
            out.append((nxt[0], (base + r + 1) % SLOTS))
            state[1] = nxt[0]
    state[0] = (base + len(plan)) % SLOTS
    return out


def _old_skip(state, nb, S, n_steps, first):
    plan, base, out = shard.round_plan(nb, S, first, n_steps), state[0], []
    if plan:
        out.append((plan[0], base % SLOTS))
    for r in range(len(plan)):
        if r + 1 < len(plan):
            out.append((plan[r + 1], (base + r + 1) % SLOTS))
    state[0] = (base + len(plan)) % SLOTS
    return out


def test_literal_walks():
    """(e) three walks written out by hand"""
    # one round
    assert list(shard.round_walk([(0, 2)], [], 0, None, 3)) == [("submit", (0, 2), 0), ("use", (0, 2), 0)]
    # 5 minibatches, 2 streams: two whole rounds and a tail of one, from a rotation that stands at slot 2
    plan = shard.round_plan(5, 2, 0, 5)
    assert plan == [(0, 2), (2, 2), (4, 1)]
    assert list(shard.round_walk(plan, [], 2, None, 3)) == [
        ("submit", (0, 2), 2), ("submit", (2, 2), 0), ("use", (0, 2), 2), ("submit", (4, 1), 1), ("use", (2, 2), 0),
        ("use", (4, 1), 1)]
    # run(2, then=(2, 3)) and the announced run(3, first_batch=2): the announced round is submitted by the first call only
    state = [0, None]
    assert _call(state, 5, 2, 2, 0, then=(2, 3)) == [("submit", (0, 2), 0), ("submit", (2, 2), 1), ("use", (0, 2), 0)]
    assert state == [1, (2, 2)]
    assert _call(state, 5, 2, 3, 2) == [("submit", (4, 1), 2), ("use", (2, 2), 1), ("use", (4, 1), 2)]
    assert state == [0, None]
    # nothing to do: nothing yielded, with or without an announced follow-up
    assert list(shard.round_walk([], [(0, 1)], 1, None, 3)) == []
