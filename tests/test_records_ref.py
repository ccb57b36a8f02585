"""The record reference (tests/records_ref.py) checked on the CPU: the input conditions that
tests/test_gpu_records.py's bounds rest on, from scipy's splines of the same two sources (the
device's spline build is held to scipy at 1e-11 in tests/test_gpu_modesum.py).

- the reference's own fits (env_fit restated in float64) stay within 1.0 x both tolerances on
  513 points of every record they certify, so the device test's 1.05 x leaves the reference
  itself 5% of room and a fit that is wrong between the check points none;
- the records within 1% of a threshold ("undecided") are at most 1%;
- the phase check stays sharp: 2 spacing(|Phi(t_j)|) <= 0.25 ENV_TOL_T on at least 70% of the
  envelope records and <= ENV_TOL_T on all;
- the prediction (safe bit ignored) contains the envelope class, the longest series lengths and
  empty records, and the stretched source of the device test the short ones;
- mpmath and np.longdouble agree on the exact envelope to 1e-17 relative.
"""

import functools

import numpy as np
import pytest

from tests import records_ref as rr
from tests.helpers import source_inputs

C = rr.C
SOURCES = {"small": dict(M=3e5, e0=0.35, T=0.02, dt=20.0, eps=1e-2),
           "A": dict(M=3e5, e0=0.35, T=0.01, dt=20.0, eps=1e-3)}


@functools.lru_cache(maxsize=None)
def _records(name, stretch=1.0):
    d = source_inputs(**SOURCES[name])
    d["t"] = d["t"] * stretch
    gm, gn, cnt = rr.host_groups(d)
    klo, khi = rr.host_lane_ranges(d, gm, gn, d["freq"])
    R = rr.Records(rr.scipy_coefT(d), d["t"], gm, gn, klo, khi, d["freq"], False, members=cnt)
    return R, R.predict(np.ones(len(R.g), bool))


def test_constants_are_parsed_from_the_sources():
    assert C.ENV_TOL_A == 1e-11 and C.ENV_TOL_T == 1e-10 and C.ENV_MIN_Y == 153.0
    assert C.FAST_J == 4 and C.JSER_Y[C.FAST_J] == C.ENV_MIN_Y
    assert C.KRH[0] == 1.0 and C.KTHN[0] == 1.0 and C.KTH0 == -5.0 / 72.0
    assert abs(C.TWO_PI - 2 * np.pi) == 0.0 and abs(C.ENV_AMP_SCALE - 1.0) < 1e-10
    # the interpolation matrices reproduce polynomials of their degree: A = s^i on the nodes
    # gives the unit coefficient vectors; theta's cubic is exact for cubics
    for i in range(7):
        e = np.zeros(7)
        e[i] = 1.0
        assert np.abs(C.ENV_W7 @ rr.NODES ** i - e).max() < 1e-9
    for i in range(4):
        e = np.zeros(4)
        e[i] = 1.0
        assert np.abs(C.ENV_W3 @ rr.NODES ** i - e).max() < 1e-12


@pytest.mark.parametrize("name", sorted(SOURCES))
def test_reference_fits_hold_between_the_check_points(name):
    R, (env, undecided, J, ymin, ra, rt) = _records(name)
    L = R.lanes
    cert = env & L
    assert cert.sum() > 0.5 * L.sum()
    _, _, _, a, th = R.env_fit(cert, R.fdneg_mid)
    da, dth = rr.dense_fit_error(R, cert, R.fdneg_mid, a, th)
    print(f"{name}: {int(cert.sum())} certified of {int(L.sum())} with lanes, worst dense error "
          f"/ tolerance: A {da.max():.3f}, theta {dth.max():.3f}")
    assert da.max() <= 1.0 and dth.max() <= 1.0
    assert (undecided & L).sum() <= 0.01 * L.sum()
    sp = 2.0 * np.spacing(np.abs(R.phi64[cert, 3]))
    assert np.mean(sp <= 0.25 * C.ENV_TOL_T) >= 0.70 and sp.max() <= C.ENV_TOL_T


def test_prediction_contains_every_class():
    seen = set()
    for name, stretch in (("small", 1.0), ("A", 1.0), ("small", 2.0 ** 20)):
        R, (env, _, J, ymin, ra, rt) = _records(name, stretch)
        L = R.lanes
        # the series length the bound gives, whatever the record's final class
        seen.update(int(v) for v in np.unique(J[L]))
        for key, mask in (("env", env & L), ("empty", ~L),
                          ("rejected", L & ~env & np.isfinite(ra))):   # tried, fit refused
            if mask.any():
                seen.add(key)
    assert seen >= {"env", "empty", "rejected", 1, 2, 3, 4}, seen


def test_longdouble_envelope_matches_mpmath():
    R, _ = _records("A")
    rng = np.random.default_rng(20261020)
    rec = rng.choice(np.flatnonzero(R.lanes & (R.ymin_bound() >= 1.0)), 100, replace=False)
    w = (R.dt[rec] * rng.uniform(0.0, 1.0, len(rec)))
    A, th, y = rr.env_exact(R.fq64[rec].astype(rr.LD), R.gq64[rec].astype(rr.LD),
                            R.fdneg_mid[rec], w.astype(rr.LD))
    import mpmath as mp
    worst = 0.0
    for i, r in enumerate(rec):
        Am, thm, ym = rr.env_exact_mp(R.fq64[r], R.gq64[r], bool(R.fdneg_mid[r]), w[i])
        with mp.workdps(40):
            for got, ref in ((A[i], Am), (th[i], thm), (y[i], ym)):
                # longdouble -> mpmath exactly, through its two float64 halves
                hi = float(got)
                g = mp.mpf(hi) + mp.mpf(float(got - rr.LD(hi)))
                worst = max(worst, float(abs(g - ref) / abs(ref)))
    print(f"worst relative difference longdouble - mpmath: {worst:.2e}")
    assert worst <= 1e-17
