"""The cosine-sum windows' first-order form on the CPU (no GPU needed): which windows
fdutils recognises and from which grid length it takes them, and the formula and its error
bound in numpy (tests/cosine_window_ref.py) against the exact DFT form ifft(w fft(S))."""

import math

import numpy as np
import pytest
import scipy.signal.windows as sw

from emri_frequencydomainwaveforms_amd.fdutils import (COSINE_WINDOWS, CosineWindowConvolution,
                                                       HannConvolution, cosine_window)
from tests import cosine_window_ref as ref

NAMES = ("hann", "hamming", "blackman", "nuttall", "blackmanharris")


def test_coefficients_are_scipys():
    assert tuple(COSINE_WINDOWS) == NAMES and COSINE_WINDOWS == ref.WINDOWS
    n = 1001
    k = np.arange(n)
    for name, a in ref.WINDOWS.items():
        w = sum((-1) ** j * aj * np.cos(2 * np.pi * j * k / (n - 1)) for j, aj in enumerate(a))
        np.testing.assert_allclose(w, getattr(sw, name)(n), rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", NAMES)
def test_recognition(name):
    n = 1001
    got = cosine_window(getattr(sw, name)(n))
    assert got == (name, ref.WINDOWS[name])
    assert cosine_window(getattr(sw, name)(n, sym=False)) is None


def test_recognition_rejects_other_windows():
    n = 1001
    assert cosine_window(sw.hann(n, sym=False)) is None
    assert cosine_window(sw.tukey(n, 0.1)) is None
    assert cosine_window(sw.blackman(n) * 1.0000001) is None
    assert cosine_window(np.ones(n)) is None
    assert cosine_window(sw.blackman(n)[None, :]) is None
    assert cosine_window(sw.blackman(n).astype(np.complex128)) is None


@pytest.mark.parametrize("name", NAMES)
def test_applies_threshold(name):
    a = ref.WINDOWS[name]
    q = ref.q(a)
    n0 = math.isqrt(int(10.0 * q * 1e12))
    while 10.0 * q / float(n0) ** 2 > 1e-12:
        n0 += 1
    while 10.0 * q / float(n0 - 1) ** 2 <= 1e-12:
        n0 -= 1
    assert CosineWindowConvolution.applies(n0, a)
    assert not CosineWindowConvolution.applies(n0 - 1, a)
    assert CosineWindowConvolution.applies(12623261, a)
    expect = {"hann": 2236068, "blackman": 2863565, "nuttall": 3363548}
    if name in expect:
        assert n0 == expect[name]
    # and never below the stencil's own width, whatever the tolerance
    assert not CosineWindowConvolution.applies(2 * (len(a) - 1), a)


def test_applies_is_hanns_for_hann():
    for n in (2, 3, 1001, 2236067, 2236068, 12623261):
        assert CosineWindowConvolution.applies(n, ref.WINDOWS["hann"]) == HannConvolution.applies(n)
        assert CosineWindowConvolution.applies(n) == HannConvolution.applies(n)
    assert HannConvolution.applies(2236068) and not HannConvolution.applies(2236067)


def test_exact_correction_is_the_lag_kernel_convolution():
    S = ref.spectrum(1001, 3)
    C, Ck = ref.exact_correction(S), ref.lag_kernel_correction(S)
    assert np.abs(C - Ck).max() <= 1e-12 * np.abs(C).max()


@pytest.mark.parametrize("n", [10001, 100001])
@pytest.mark.parametrize("name", NAMES)
def test_first_order_form_within_bound(name, n):
    """The first-order form with exact complex128 C against ifft(w fft(S)) on a random-phase
    spectrum whose lower third is zero: within 10 q / n^2 of max|S| (measured 0.67-0.72 of it
    for hann and hamming, 0.32-0.39 for the three- and four-term windows)."""
    a = ref.WINDOWS[name]
    S = ref.spectrum(n, n)
    got = ref.first_order(S, a, ref.exact_correction(S))
    exact = ref.dft_form(S, getattr(sw, name)(n))
    err = np.abs(got - exact).max() / np.abs(S).max()
    print(f"{name} n={n}: error / bound = {err / ref.bound(a, n):.3f}")
    assert err <= ref.bound(a, n)
    # the bound is not slack by orders: the form is first order, not better
    assert err >= 0.1 * ref.bound(a, n)


def test_hann_is_the_documented_form():
    n = 1001
    S = ref.spectrum(n, 1)
    C = ref.exact_correction(S)
    hann = (0.5 * S - 0.25 * (np.roll(S, -1) + np.roll(S, 1))
            - 0.25 / (n - 1) * (np.roll(C, -1) - np.roll(C, 1)))
    assert np.abs(ref.first_order(S, ref.WINDOWS["hann"], C) - hann).max() <= 1e-15
