"""likelihood.choose_branch: the order of Likelihood._run's ladder, pinned with stub template
models, and _run's dispatch on it for both output kinds. No GPU."""

from types import SimpleNamespace as Stub

import numpy as np
import pytest

from emri_frequencydomainwaveforms_amd import likelihood as lk

EVERYTHING = Stub(can_pipeline=True, can_fill_batch=True, can_fill=True)
FD_MODEL = Stub(can_pipeline=True, can_fill_batch=False, can_fill=True)
WINDOWED = Stub(can_pipeline=False, can_fill_batch=True, can_fill=True)   # the TD template's too
FILL_ONLY = Stub(can_fill=True)
BARE = (lambda *a, **k: None)

CASES = [
    # template model, vectorized, positional waveform arguments, branch
    (EVERYTHING, True, False, "vectorized"),      # vectorized wins over everything
    (EVERYTHING, True, True, "vectorized"),
    (BARE, True, False, "vectorized"),
    (EVERYTHING, False, False, "pipelined"),      # can_pipeline over can_fill_batch and can_fill
    (EVERYTHING, False, True, "pipelined"),
    (FD_MODEL, False, False, "pipelined"),
    (WINDOWED, False, False, "window_batch"),     # no can_pipeline: the batch, not the fill
    (WINDOWED, False, True, "fill"),              # positional arguments fall through to the fill
    (Stub(can_fill_batch=True), False, True, "call"),   # ... or past it where there is none
    (FILL_ONLY, False, False, "fill"),
    (FILL_ONLY, False, True, "fill"),
    (BARE, False, False, "call"),                 # a bare callable takes the last branch
    (BARE, False, True, "call"),
    (Stub(can_pipeline=False, can_fill_batch=False, can_fill=False), False, False, "call"),
]


@pytest.mark.parametrize("tm, vectorized, has_args, branch", CASES)
def test_choose_branch(tm, vectorized, has_args, branch):
    assert lk.choose_branch(tm, vectorized, has_args) == branch


def test_run_takes_the_chosen_branch_for_both_kinds():
    """get_ll and parts of one object dispatch on choose_branch alone: the same _branch_* method
    runs for LOGL and for PAIR, with a slot of 1 and of 3 doubles per walker."""
    torch = pytest.importorskip("torch")
    like = object.__new__(lk.Likelihood)        # no device: the branches are recorders
    like.torch, like.device = torch, torch.device("cpu")
    like.frequency_domain = True
    like.use_gpu = like.return_cupy = like.separate_d_h = False
    seen = []
    for name in ("vectorized", "pipelined", "window_batch", "fill", "call"):
        def branch(kind, tm, params, args, kwargs, out, name=name):
            out.zero_()
            seen.append((name, kind, tuple(out.shape)))
        setattr(like, "_branch_" + name, branch)
    walkers = np.zeros((3, 2))
    for tm, vectorized, has_args, want in CASES:
        like.template_model, like.vectorized = tm, vectorized
        args = (1.0,) if has_args else ()
        ll = like.get_ll(walkers, *args)
        assert like.branch_taken == want
        d_h, h_h = like.parts(walkers, *args)
        assert like.branch_taken == want
        assert seen[-2:] == [(want, lk.LOGL, (3,)), (want, lk.PAIR, (3, 3))]
        assert ll.shape == d_h.shape == h_h.shape == (3,) and d_h.dtype == np.complex128
        like.separate_d_h = True                 # get_ll with lisatools' flag: the pair
        like.get_ll(walkers, *args)
        like.separate_d_h = False
        assert seen[-1] == (want, lk.PAIR, (3, 3))
