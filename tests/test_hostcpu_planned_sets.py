"""hostcpu.rank_cores on a core set that is not the process's own (a node laid out for
planning, as tests/test_hostcpu.py fakes one): the split must not depend on the cores the host
running the call happens to allow. On a host whose cgroup allows a superset of the faked set
(a 256-core box: cores 100-227 are a strict subset) the set used to be taken for a per-rank
binding and returned whole to every rank."""

import os

from emri_frequencydomainwaveforms_amd import hostcpu


def test_planned_set_splits_whatever_the_host_allows(monkeypatch):
    monkeypatch.delenv("EFD_HOST_SPLIT", raising=False)
    monkeypatch.setattr(hostcpu, "allowed_cores", lambda: set(range(8192)))
    own = set(os.sched_getaffinity(0))
    fake = set(range(5000, 5128))
    assert fake != own
    shares = [hostcpu.rank_cores(fake, r, 8) for r in range(8)]
    assert [len(s) for s in shares] == [16] * 8
    assert sorted(c for s in shares for c in s) == sorted(fake)
    # the process's own set, a strict subset of what the cgroup allows: bound per rank, whole
    assert hostcpu.rank_cores(own, 1, 2) == sorted(own)
    assert hostcpu.rank_cores(None, 1, 2) == sorted(own)
    # a planned set that the process's own set comes to equal once pinned is still planned
    monkeypatch.setattr(hostcpu, "_START_AFFINITY", frozenset(range(6000, 6256)))
    half = set(range(6000, 6128))
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: half)
    assert hostcpu.rank_cores(half, 1, 2) == list(range(6064, 6128))
    # and an explicit bound still decides for any set
    assert hostcpu.rank_cores(fake, 3, 8, allowed=set(range(4096, 8192))) == sorted(fake)
    assert hostcpu.rank_cores(fake, 3, 8, allowed=fake) == list(range(5048, 5064))
