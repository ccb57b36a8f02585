"""summation.run_groups, the batched callers' shared group loop, with a stub feed and a stub
preparer: the steps' order and slices, and what a step that raises leaves behind. No GPU."""

import pytest

from emri_frequencydomainwaveforms_amd.summation import run_groups


class _Future:
    def __init__(self):
        self.cancelled = 0

    def cancel(self):
        self.cancelled += 1


class _Feed:
    def __init__(self, n):
        self.futs = [_Future() for _ in range(n)]


class _Preparer:
    dropped = 0

    def drop_pending(self):
        self.dropped += 1


def test_every_group_in_order():
    prep, feed, used, seen = _Preparer(), _Feed(7), [], []

    def step(g0, g):
        seen.append((g0, g))
        return (g0 // 3) % 2          # two rotating groups

    run_groups(prep, feed, 7, 3, step, used)
    assert seen == [(0, slice(0, 3)), (3, slice(3, 6)), (6, slice(6, 9))]
    assert used == [0, 1, 0]
    assert prep.dropped == 1 and all(f.cancelled == 1 for f in feed.futs)


def test_a_failing_step():
    """The second of three groups raises: the exception propagates, the third group never runs,
    the first group's index is reported, every future is cancelled and the preparer forgets its
    pending walkers, once."""
    prep, feed, used, seen = _Preparer(), _Feed(6), [], []

    def step(g0, g):
        seen.append(g0)
        if g0 == 2:
            raise RuntimeError("injected step failure")
        return 5 + g0

    with pytest.raises(RuntimeError, match="injected"):
        run_groups(prep, feed, 6, 2, step, used)
    assert seen == [0, 2]
    assert used == [5]
    assert prep.dropped == 1
    assert all(f.cancelled == 1 for f in feed.futs)
