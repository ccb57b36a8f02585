"""Noise realisations without a device: the host twins (efd_noise_fd_cpu,
efd_noise_overlap_rows_cpu) and the generator's definition against the numpy reference of
noise_ref.py (Philox4x32-10 in uint64 arithmetic, Box-Muller in long double)."""

import ctypes

import numpy as np
import pytest

from emri_frequencydomainwaveforms_amd import _lib
from tests import noise_ref as nr

SEEDS = (2601996, 2 ** 63 + 5)
TOL = 4e-14   # |xi| <= 8.57, r within ~1.5 ulp, sin and cos within ~2 ulp plus the 7e-16
#               rounding of 2 pi u2: ~1e-14 absolute, times 4


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_known_answers(lib):
    """The three known answers, by the numpy helper and by the twins' integer stage: the four
    words are read through the test-only entry efd_noise_philox_cpu, which calls the
    philox4x32_10 of csrc/emrifd_noise.h that efd_noise_fd_cpu and the device kernels call."""
    for ctr, key, want in nr.KNOWN_ANSWERS:
        got = tuple(int(x) for x in nr.philox4x32_10(*ctr, *key))
        assert got == want, [hex(x) for x in got]
        c = (ctypes.c_uint32 * 4)(*ctr)
        k = (ctypes.c_uint32 * 2)(*key)
        w = (ctypes.c_uint32 * 4)()
        assert lib.efd_noise_philox_cpu(c, k, w) == 0
        assert tuple(w) == want, [hex(x) for x in w]
    assert lib.efd_noise_philox_cpu(None, None, None) == -1


def _twin_err(lib, seed, real, nbin, bin0=0):
    got = nr.noise_fd_cpu(lib, 2, nbin, seed, real, bin0)
    ref = 0.5 * nr.xi(seed, real, 2, nbin, bin0)
    return max(float(np.max(np.abs(got.real - ref.real))),
               float(np.max(np.abs(got.imag - ref.imag)))) * 2.0   # of xi itself


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("real", [0, 7])
def test_twin_against_reference(lib, seed, real):
    """Every component of xi within 4e-14 absolute of the long-double reference (measured worst
    on the host twin: 2.0e-15, DESIGN.md "Noise realisations")."""
    worst = 0.0
    for nbin in (1, 63, 64, 65, 4099):
        worst = max(worst, _twin_err(lib, seed, real, nbin))
    # the counter's 32-bit carry: bins 2^32 - 3 ... 2^32 + 4
    worst = max(worst, _twin_err(lib, seed, real, 8, bin0=2 ** 32 - 3))
    print("worst |xi - ref|:", worst)
    assert worst <= TOL


def test_carry_reaches_the_second_counter_word(lib):
    """Bin 2^32 is not bin 0: the high word of the bin index is in the counter."""
    a = nr.noise_fd_cpu(lib, 1, 1, SEEDS[0], 0, bin0=2 ** 32)
    b = nr.noise_fd_cpu(lib, 1, 1, SEEDS[0], 0, bin0=0)
    assert a[0, 0] != b[0, 0]


def test_slices_are_bitwise_the_whole(lib):
    whole = nr.noise_fd_cpu(lib, 2, 4099, SEEDS[0], 3)
    for bin0, n in ((0, 1000), (1000, 2000), (3000, 1099)):
        part = nr.noise_fd_cpu(lib, 2, n, SEEDS[0], 3, bin0=bin0)
        assert np.array_equal(part.view(np.float64), whole[:, bin0:bin0 + n].copy().view(np.float64))


def test_gain_and_accumulate(lib):
    nbin = 515
    rng = np.random.default_rng(5)
    gain = rng.uniform(0.5, 2.0, (2, nbin))
    gain[:, 0] = np.nan
    gain[1, 7:40] = 0.0
    dead = np.isnan(gain) | (gain == 0.0)
    ones = nr.noise_fd_cpu(lib, 2, nbin, SEEDS[0])
    assert np.array_equal(ones, nr.noise_fd_cpu(lib, 2, nbin, SEEDS[0], gain=np.ones((2, nbin))))
    got = nr.noise_fd_cpu(lib, 2, nbin, SEEDS[0], gain=gain)
    assert np.all(got[dead] == 0.0) and not np.isnan(got.view(np.float64)).any()
    np.testing.assert_array_equal(got[~dead], (gain * ones)[~dead])   # s = 0.5 g, then s xi
    base = rng.standard_normal((2, nbin)) + 1j * rng.standard_normal((2, nbin))
    acc = nr.noise_fd_cpu(lib, 2, nbin, SEEDS[0], gain=gain, out=base.copy(), accumulate=True)
    np.testing.assert_array_equal(acc[dead], base[dead])
    np.testing.assert_array_equal(acc[~dead], (base + got)[~dead])
    # nbin = 0 is a no-op that returns 0, whatever the pointers
    assert lib.efd_noise_fd_cpu(None, None, 2, 0, 0, 1, 0, 0, None) == 0


def statistics_z(x):
    """z-scores under the null of unit complex normals x[realisation][channel][bin]
    (realisations 0 and 1, channels 0 and 1). Over the components of realisation 0, both
    channels: the mean, the variance, the excess kurtosis (the raw fourth moment, variance 96 /
    n), sum xi_r xi_i and the lag-1 product of the real parts along the bins; the cross-channel
    product Re conj(xi(c = 0)) xi(c = 1) of realisation 0 and the cross-realisation product of
    channel 0."""
    z = x[0]
    comp = np.concatenate([z.real.ravel(), z.imag.ravel()])
    n = comp.size

    def cross(a, b):
        return float(np.sum((a.conj() * b).real) / np.sqrt(2.0 * a.size))
    return {
        "mean": float(comp.mean() * np.sqrt(n)),
        "variance": float((comp.var() - 1.0) / np.sqrt(2.0 / n)),
        "kurtosis": float((np.mean(comp ** 4) - 3.0) / np.sqrt(96.0 / n)),
        "re_im": float(np.sum(z.real * z.imag) / np.sqrt(z.size)),
        "lag1": float(np.sum(z.real[:, :-1] * z.real[:, 1:]) / np.sqrt(z[:, 1:].size)),
        "cross_channel": cross(x[0, 0], x[0, 1]),
        "cross_realisation": cross(x[0, 0], x[1, 0]),
    }


# the numpy reference's z-scores at seed 2601996, nbin 4099 (two decimals)
REFERENCE_Z = dict(mean=-0.08, variance=-1.52, kurtosis=-1.49, re_im=-0.21, lag1=0.08,
                   cross_channel=0.15, cross_realisation=0.08)


def test_statistics(lib):
    """Deterministic: seed 2601996, nbin 4099, channels 0 and 1, realisations 0 and 1. The
    numpy reference gives |z| <= 1.6 on every statistic (REFERENCE_Z); the gate is |z| <= 4, for
    the reference and for the twin."""
    nbin = 4099
    ref = np.stack([nr.xi(SEEDS[0], r, 2, nbin) for r in (0, 1)])
    got = 2.0 * np.stack([nr.noise_fd_cpu(lib, 2, nbin, SEEDS[0], r) for r in (0, 1)])
    zr = statistics_z(ref)
    print("reference", {k: round(v, 2) for k, v in zr.items()})
    assert {k: round(v, 2) + 0.0 for k, v in zr.items()} == REFERENCE_Z
    for name, x in (("reference", ref), ("twin", got)):
        for k, v in statistics_z(x).items():
            assert abs(v) <= 4.0, (name, k, v)


@pytest.mark.parametrize("nbin", [1, 65, 4099])
@pytest.mark.parametrize("nrow", [1, 6])
def test_overlaps_against_explicit_noise(lib, nrow, nbin):
    rows, gain = nr.overlap_case(17 * nrow + nbin, nrow, 2, nbin)
    for real0 in (0, 9):
        val, bound = nr.overlaps_explicit(rows, gain, SEEDS[0], real0, 33)
        for ndraw in (1, 5, 33):
            got = nr.noise_overlap_rows_cpu(lib, rows, gain, SEEDS[0], real0, ndraw)
            err = np.abs(got - val[:ndraw])
            assert np.all(err <= bound[None, :]), (real0, ndraw, float(np.max(err / bound)))


def test_overlap_limits(lib):
    rows, gain = nr.overlap_case(1, 1, 1, 4)
    out = np.zeros(4)
    p = nr._ptr
    assert lib.efd_noise_overlap_rows_cpu(p(rows), 17, p(gain), 1, 4, 1, 0, 1, p(out), None,
                                          None) == -1
    assert lib.efd_noise_overlap_rows_cpu(p(rows), 1, p(gain), 1, 4, 1, 2 ** 32 - 1, 2, p(out),
                                          None, None) == -1
    assert lib.efd_noise_overlap_rows_cpu(p(rows), 1, p(gain), 1, 4, 1, 0, 0, p(out), None,
                                          None) == 0
    # the device entry's argument checks are host-side too
    assert lib.efd_noise_overlap_rows(p(rows), 17, p(gain), 1, 4, 1, 0, 1, p(out), p(out),
                                      None) == -1
    assert b"nrow outside 1..16" in _lib.last_error(lib).encode()
    assert lib.efd_noise_fd(None, None, 2, 0, 0, 1, 0, 0, None) == 0
    assert lib.efd_noise_fd(None, None, 2, 5, 0, 1, 0, 0, None) == -1


def sample_covariance_check(over, rows, gain):
    """max over the entries of |C_sample - G| / standard error, G = sum gain^2 Re(conj a b), the
    standard error from the Wishart variance (G_ii G_jj + G_ij^2) / R."""
    R = over.shape[0]
    g2 = np.where(np.isnan(gain) | (gain == 0.0), 0.0, gain) ** 2
    G = np.einsum("ck,pck,qck->pq", g2, rows.real, rows.real) \
        + np.einsum("ck,pck,qck->pq", g2, rows.imag, rows.imag)
    C = np.cov(over, rowvar=False).reshape(G.shape)
    se = np.sqrt((np.outer(np.diag(G), np.diag(G)) + G ** 2) / R)
    return float(np.max(np.abs(C - G) / se))


COV_SEED = 2601996


def test_sample_covariance(lib):
    """4096 draws of 3 random rows at nbin = 257: every entry of the overlaps' sample covariance
    within 5 standard errors of the rows' Gram matrix."""
    rows, gain = nr.overlap_case(3, 3, 2, 257)
    over = nr.noise_overlap_rows_cpu(lib, rows, gain, COV_SEED, 0, 4096)
    z = sample_covariance_check(over, rows, gain)
    print("worst |C - G| / se:", z)
    assert z <= 5.0
