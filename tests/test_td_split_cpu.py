"""efd_td_split_cpu / efd_td_split_loglike_cpu against the numpy restatement of the reference's
TD-template route (tests/td_template_ref.py). Runs without a GPU.

Bounds. Split: 4 ulp of gain (|Z[k]| + |Z[n-k]|) per component (two adds and two multiplies),
against numpy's Hermitian split of the same Z. logL: 1e-12 of 2 sum(|d|^2 + |h w|^2) (the
inner-product tolerance of tests/test_fisher_cpu.py and tests/test_gpu_likelihood.py), against
the route from the time series: two transforms per row, fftshift, the drivers' mask.
"""

import numpy as np
import pytest

from tests import td_template_ref as tr

GAIN = 20.0


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", tr.CASES_N)
def test_split_matches_numpy(n, rows):
    h = tr.series(rows, n, seed=n + rows)
    Z = np.fft.fft(h, axis=-1)
    nb = (n + 1) // 2
    assert nb == int(tr.positive_mask(n).sum())
    buf = tr.strided(Z, n + 5)
    got = tr.split_cpu(buf, n, GAIN, out_pad=3)
    ref = tr.channels_from_Z(Z, GAIN)
    bound = 4.0 * tr.EPS * tr.pair_magnitude(Z, GAIN)[:, None, :]
    err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    print(f"n={n} rows={rows}: max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # and the route from the time series lands on the same bins
    two = tr.channels_from_series(h, GAIN)
    assert np.abs(got - two).max() <= 1e-12 * np.abs(two).max()


@pytest.mark.parametrize("n", tr.CASES_N)
def test_split_keep_writes_exact_zeros(n):
    h = tr.series(3, n, seed=100 + n)
    Z = np.fft.fft(h, axis=-1)
    nb = (n + 1) // 2
    keep = np.ones(nb, dtype=np.uint8)
    keep[::3] = 0
    full = tr.split_cpu(tr.strided(Z, n + 1), n, GAIN)
    got = tr.split_cpu(tr.strided(Z, n + 1), n, GAIN, keep=keep)
    assert np.all(got[:, :, keep == 0] == 0.0)
    assert np.array_equal(got[:, :, keep != 0], full[:, :, keep != 0])


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", tr.CASES_N)
def test_loglike_matches_numpy(n, rows):
    h = tr.series(rows, n, seed=7 * n + rows)
    Z = np.fft.fft(h, axis=-1)
    nb = (n + 1) // 2
    d, w = tr.data_and_weights(nb, seed=n)
    w[:, ::5] = 0.0   # a mask folded into the weight
    got = tr.split_loglike_cpu(tr.strided(Z, n + 9), n, GAIN, d, w)
    chans = tr.channels_from_series(h, GAIN)
    for r in range(rows):
        ref = tr.loglike(d, chans[r], w)
        tol = 1e-12 * tr.loglike_scale(d, chans[r], w)
        print(f"n={n} row {r}: |dlogL| / scale {abs(got[r] - ref) / tol * 1e-12:.3e}")
        assert abs(got[r] - ref) <= tol


@pytest.mark.parametrize("n", [8, 1025])
def test_loglike_nan_poisons_its_row_only(n):
    h = tr.series(3, n, seed=3)
    Z = np.fft.fft(h, axis=-1)
    d, w = tr.data_and_weights((n + 1) // 2, seed=4)
    for where in (0, n // 2, n - 1):
        Zn = Z.copy()
        Zn[1, where] = np.nan
        got = tr.split_loglike_cpu(tr.strided(Zn, n + 2), n, GAIN, d, w)
        assert np.isnan(got[1]) and np.isfinite(got[0]) and np.isfinite(got[2]), where


def test_argument_errors():
    from emri_frequencydomainwaveforms_amd import _lib
    lib = _lib.load()
    Z = np.zeros(8, dtype=np.complex128)
    out = np.zeros(8, dtype=np.complex128)
    p = tr._p
    assert lib.efd_td_split_cpu(None, 8, 8, 1, 1.0, None, p(out), 8, None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split_cpu(p(Z), 7, 8, 1, 1.0, None, p(out), 8, None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split_cpu(p(Z), 8, 8, 1, 1.0, None, p(out), 7, None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split_loglike_cpu(p(Z), 8, 8, 1, 1.0, None, p(out), p(out), None,
                                        None) == _lib.EFD_ERR_ARG
    # the device entry points validate before any launch (no GPU needed to see it)
    fake = 16
    assert lib.efd_td_split(None, 8, 8, 1, 1.0, None, fake, 8, None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split(fake, 7, 8, 1, 1.0, None, fake, 8, None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split(fake, 8, 8, 0, 1.0, None, fake, 8, None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split_loglike(fake, 8, 8, 1, 1.0, fake, fake, fake, None,
                                    None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_split_loglike(fake, 7, 8, 1, 1.0, fake, fake, fake, fake,
                                    None) == _lib.EFD_ERR_ARG
    assert lib.efd_td_modesum_windowed(None, fake, fake, 1 << 40, None) == _lib.EFD_ERR_ARG


def test_pe_setup_td_rejects_downsampling():
    from emri_frequencydomainwaveforms_amd import pe
    with pytest.raises(ValueError, match="Cannot run downsampling with time domain template"):
        pe.setup(template="td", downsample=100)
