"""The host twin efd_modesum_cpu against the numpy oracle on the grids of tests/grid_cases.py:
non-uniform spacing, bins exactly on knot frequencies and on their floating-point neighbours,
even-length symmetric grids, lane counts at a tile boundary, nf = 1, 2, 3, repeated values.

The twin takes its lane bounds with std::upper_bound / lower_bound, the oracle with per-bin
comparisons: two independent statements of the open/closed rule at knots. Per grid:
- max|S_twin - R| <= 1e-9 max|R| (the rule of tests/test_cpu_twin.py), identical support, and the
  twin's contribution count equal to fd_oracle.contributions;
- on symmetric grids the forced-unpaired twin equals the paired one to 1e-13 max|S|.

It also pins the input conditions tests/test_gpu_grid_edges.py relies on: the device's linear
index guess fails to settle at least half of the bounds on every non-uniform grid
(grid_cases.guess_unsettled; printed with -s) and none on the uniform grid, and every knot-exact
grid holds each knot frequency and both of its neighbours bit for bit.
"""

import numpy as np
import pytest

from emri_frequencydomainwaveforms_amd import cputwin
from oracle import fd_oracle
from tests import grid_cases as gc
from tests.helpers import source_inputs


@pytest.fixture(scope="module")
def sources():
    full = source_inputs(**gc.SRC)
    return {"full": full, "first": gc.first_harmonics(full), "nonmono": source_inputs(**gc.NONMONO)}


def _twin(d, freq, **kw):
    return cputwin.modesum(d["t"], np.ascontiguousarray(np.asarray(d["amp"]).T), d["phi_phi"],
                           d["phi_r"], d["f_phi"], d["f_r"], d["m"], d["n"], d["ylm_p"],
                           d["ylm_m"], freq, d["prefactor"], **kw)


def _oracle(d, freq, caustic="uniform"):
    return fd_oracle.fd_modesum(d["t"], np.asarray(d["amp"]), d["phi_phi"], d["phi_r"],
                                d["f_phi"], d["f_r"], d["m"], d["n"], d["ylm_p"], d["ylm_m"],
                                freq, d["prefactor"], caustic=caustic)


def _both_signs(d):
    F = gc.knot_values(d)
    return np.concatenate([-F[::-1], F])


@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_twin_vs_oracle_on_grid(sources, case):
    d = sources[case[0]]
    freq = gc.grid(d, case[1])
    assert np.all(np.diff(freq) >= 0.0)
    S = _twin(d, freq)
    C = cputwin.stats()[0]
    R = _oracle(d, freq)
    mx = np.abs(R).max()
    err = np.abs(S - R).max()
    print(f"{gc.case_id(case)}: nf = {len(freq)}, max|S - R| / max|R| = "
          f"{err / mx if mx > 0 else 0.0:.3e}, C = {C}")
    assert err <= 1e-9 * mx
    np.testing.assert_array_equal(S != 0, R != 0)
    assert C == fd_oracle.contributions(d["t"], d["f_phi"], d["f_r"], d["m"], d["n"], freq)
    if gc.is_symmetric(freq):
        U = _twin(d, freq, grid_symmetric=False)
        assert np.abs(U - S).max() <= 1e-13 * np.abs(S).max()


@pytest.mark.parametrize("case", gc.SPA_CASES, ids=gc.case_id)
def test_twin_vs_oracle_on_grid_spa(sources, case):
    d = sources[case[0]]
    freq = gc.grid(d, case[1])
    S = _twin(d, freq, caustic="spa")
    R = _oracle(d, freq, "spa")
    assert np.abs(S - R).max() <= 1e-9 * np.abs(R).max()
    np.testing.assert_array_equal(S != 0, R != 0)


@pytest.mark.parametrize("name", gc.NONUNIFORM)
def test_guess_fails_on_nonuniform_grids(sources, name):
    d = sources["full"]
    share = gc.guess_unsettled(gc.grid(d, name), _both_signs(d))
    print(f"{name}: guess_unsettled = {share:.3f}")
    assert share >= 0.5


def test_guess_settles_every_bound_on_the_uniform_grid(sources):
    d = sources["full"]
    share = gc.guess_unsettled(d["freq"], _both_signs(d))
    print(f"fd_grid: guess_unsettled = {share:.3f}")
    assert share == 0.0


@pytest.mark.parametrize("src", ["full", "nonmono"])
@pytest.mark.parametrize("name", gc.KNOT_EXACT)
def test_knot_exact_grids_hold_the_knots(sources, src, name):
    d = sources[src]
    freq = gc.grid(d, name)
    F = gc.knot_values(d)
    assert len(F) > 100
    signs = (1.0,) if name == "knot_one" else (1.0, -1.0)
    for s in signs:
        assert np.isin(s * F, freq).all()
        assert np.isin(np.nextafter(s * F, np.inf), freq).all()
        assert np.isin(np.nextafter(s * F, -np.inf), freq).all()
    assert gc.is_symmetric(freq) == (name != "knot_one")
    assert (len(freq) % 2 == 0) == (name == "knot_even") or name == "knot_one"
    assert (0.0 in freq) == (name == "knot_odd")


def test_small_grid_shapes(sources):
    d = sources["full"]
    for nf in gc.SMALL_NF:
        s, o = gc.small(d, nf, True), gc.small(d, nf, False)
        assert len(s) == nf and len(o) == nf
        assert gc.is_symmetric(s) and (0.0 in s) == bool(nf % 2)
        assert not gc.is_symmetric(o) and o.min() > 0.0
    dups = gc.grid(d, "dups")
    assert gc.is_symmetric(dups) and np.count_nonzero(np.diff(dups) == 0.0) >= 400
