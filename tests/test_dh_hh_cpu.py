"""<d|h> and <h|h> without a device: efd_dh_hh_rows_cpu against numpy, the two new entries'
host-side argument checks, and ProfiledLikelihood's host arithmetic (the closed-form amplitude
maximum and the distance marginalisation's quadrature against scipy's adaptive one)."""

import ctypes

import numpy as np
import pytest

from emri_frequencydomainwaveforms_amd import _lib
from emri_frequencydomainwaveforms_amd import likelihood as lk


def _ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _rows_cpu(h, d, w):
    """efd_dh_hh_rows_cpu on numpy arrays: h complex [nrow][nchan][nbin] -> float64 [nrow][3]."""
    lib = _lib.load()
    nrow, nchan, nbin = h.shape
    out = np.full((nrow, 3), np.nan)
    rc = lib.efd_dh_hh_rows_cpu(_ptr(h), nchan * nbin, nrow, _ptr(d), _ptr(w), nchan, nbin,
                                _ptr(out), None, None)
    assert rc == _lib.EFD_OK
    return out


def _make(seed, nrow, nchan, nbin):
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal((nrow, nchan, nbin))
         + 1j * rng.standard_normal((nrow, nchan, nbin))) * 1e-62
    d = (rng.standard_normal((nchan, nbin)) + 1j * rng.standard_normal((nchan, nbin))) * 1e-22
    w = rng.uniform(0.5, 2.0, (nchan, nbin)) * 1e40
    d[:, 0] = 0.0          # a zeroed first bin, as _prepare_reduction leaves it
    w[:, 0] = 0.0
    return np.ascontiguousarray(h), d, w


def _reference(h, d, w):
    """numpy float64: the three sums and the sum of the terms' magnitudes, per row."""
    hw = h * w[None]
    val = np.stack([4 * np.sum(d.real * hw.real + d.imag * hw.imag, axis=(1, 2)),
                    4 * np.sum(d.real * hw.imag - d.imag * hw.real, axis=(1, 2)),
                    4 * np.sum(hw.real ** 2 + hw.imag ** 2, axis=(1, 2))], axis=1)
    mag = np.stack([4 * np.sum(np.abs(d.real * hw.real) + np.abs(d.imag * hw.imag), axis=(1, 2)),
                    4 * np.sum(np.abs(d.real * hw.imag) + np.abs(d.imag * hw.real), axis=(1, 2)),
                    val[:, 2]], axis=1)
    return val, mag


@pytest.mark.parametrize("nchan", [1, 2])
@pytest.mark.parametrize("nbin", [1, 255, 256, 257, 4097])
@pytest.mark.parametrize("nrow", [1, 8, 64])
def test_rows_cpu_against_numpy(nchan, nbin, nrow):
    h, d, w = _make(100 * nchan + nbin + nrow, nrow, nchan, nbin)
    got = _rows_cpu(h, d, w)
    val, mag = _reference(h, d, w)
    err = np.abs(got - val)
    print("worst |err| / sum|terms|:", float(np.max(err / np.where(mag > 0, mag, 1.0))))
    # 1e-12 of the sum of the terms' magnitudes for another order
    assert np.all(err <= 1e-12 * mag)


@pytest.mark.parametrize("nchan", [1, 2])
def test_rows_cpu_self_product_is_exact(nchan):
    """d == h w bit for bit: Re <d|h> == <h|h> bitwise and Im <d|h> == 0.0."""
    h, _, w = _make(7, 8, nchan, 4097)
    for r in range(8):
        d = np.ascontiguousarray(h[r].real * w + 1j * (h[r].imag * w))
        got = _rows_cpu(h[r:r + 1], d, w)[0]
        assert got[0] == got[2] and got[2] > 0.0
        assert got[1] == 0.0


def test_rows_cpu_row_alone_equals_row_in_call():
    h, d, w = _make(11, 64, 2, 4097)
    whole = _rows_cpu(h, d, w)
    for r in (0, 17, 63):
        assert np.array_equal(_rows_cpu(np.ascontiguousarray(h[r:r + 1]), d, w)[0], whole[r])


def test_rows_argument_errors_are_host_side():
    """efd_dh_hh_rows and its twin reject bad arguments before any device work."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    buf = ctypes.create_string_buffer(256)
    for fn, err in ((lib.efd_dh_hh_rows, lib.efd_last_error),
                    (lib.efd_dh_hh_rows_cpu, lib.efd_cpu_last_error)):
        def call(h=fake, stride=200, nrow=2, d=fake, w=fake, nchan=2, nbin=100, out=fake):
            rc = fn(h, stride, nrow, d, w, nchan, nbin, out, fake, None)
            err(buf, 256)
            return rc
        assert call(nrow=0) == _lib.EFD_ERR_ARG and b"nrow outside" in buf.value
        assert call(nrow=65) == _lib.EFD_ERR_ARG
        assert call(nchan=3) == _lib.EFD_ERR_ARG and b"nchan must be 1 or 2" in buf.value
        assert call(h=None) == _lib.EFD_ERR_ARG and b"NULL" in buf.value
        assert call(d=None) == _lib.EFD_ERR_ARG
        assert call(w=None) == _lib.EFD_ERR_ARG
        assert call(out=None) == _lib.EFD_ERR_ARG
        assert call(nbin=0) == _lib.EFD_ERR_ARG and b"nbin" in buf.value
        assert call(stride=199) == _lib.EFD_ERR_ARG and b"row_stride" in buf.value


def test_sum_dh_hh_argument_errors_are_host_side():
    """efd_modesum_sum_dh_hh has the fused logL entry's checks, before any device work: NULL
    d/w/part/out, the count, an asymmetric grid, accumulate = 1, k0 outside [0, nf), and members
    that disagree on k0."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    a = _lib.ModesumArgs()
    for f in ("t", "phi_phi", "phi_r", "f_phi", "f_r", "amp", "m", "n", "ylm_p", "ylm_m", "freq"):
        setattr(a, f, fake)
    a.nt, a.K, a.caustic, a.scale_re, a.nf, a.k0 = 100, 30, 1, 1.0, 1001, 500
    a.grid_symmetric = 1
    b = _lib.ModesumArgs.from_buffer_copy(a)
    buf = ctypes.create_string_buffer(256)
    ws = (ctypes.c_void_p * 2)(16, 16)
    nb = (ctypes.c_size_t * 2)(1 << 40, 1 << 40)

    def call(x, y, d=fake, w=fake, part=fake, out=fake, count=2):
        pa = (ctypes.POINTER(_lib.ModesumArgs) * 2)(ctypes.pointer(x), ctypes.pointer(y))
        rc = lib.efd_modesum_sum_dh_hh(pa, ws, nb, count, d, w, part, 0, out, None)
        lib.efd_last_error(buf, 256)
        return rc, buf.value

    for kw in ({"d": None}, {"w": None}, {"part": None}, {"out": None}):
        assert call(a, b, **kw)[0] == _lib.EFD_ERR_ARG and b"NULL d, w, part or out" in buf.value
    assert call(a, b, count=0)[0] == _lib.EFD_ERR_ARG and b"count out of range" in buf.value
    assert call(a, b, count=_lib.EFD_BATCH_MAX + 1)[0] == _lib.EFD_ERR_ARG
    for field, bad, both in (("grid_symmetric", 0, True), ("accumulate", 1, True),
                             ("k0", 1001, True), ("k0", 499, False)):
        c = _lib.ModesumArgs.from_buffer_copy(b)
        setattr(c, field, bad)
        a2 = _lib.ModesumArgs.from_buffer_copy(a)
        if both:   # (members that disagree fail the batch's agreement check first)
            setattr(a2, field, bad)
        rc, msg = call(a2, c)
        assert rc == _lib.EFD_ERR_ARG and b"fused likelihood needs" in msg, (field, msg)


# ---- ProfiledLikelihood's host arithmetic --------------------------------------------------
class _NoLike:
    separate_d_h = False


def test_profile_none_is_the_identity():
    rng = np.random.default_rng(3)
    d_d, re, hh = 41.5, rng.standard_normal(9) * 30, rng.uniform(0, 50, 9)
    P = lk.ProfiledLikelihood(_NoLike(), "none")
    assert np.array_equal(P.combine(d_d, re + 0.25j, hh), -0.5 * (d_d - 2.0 * re + hh))


def test_profile_amplitude_is_the_maximum_over_u():
    d_d = 123.0
    re = np.array([30.0, 2.0, 0.0, -5.0, 0.0, 1e3])
    hh = np.array([50.0, 2.0, 4.0, 9.0, 0.0, 2.5e3])
    P = lk.ProfiledLikelihood(_NoLike(), "amplitude", dist_ref=2.0)
    got = P.combine(d_d, re.astype(np.complex128), hh)
    u = np.linspace(0.0, 4.0, 400001)              # A_hat <= 3.5 for these cases
    for i in range(len(re)):
        brute = np.max(-0.5 * d_d + u * re[i] - 0.5 * u * u * hh[i]) if hh[i] > 0 else -0.5 * d_d
        # the grid's spacing h misses the maximum by at most hh h^2 / 8
        assert 0.0 <= got[i] - brute <= hh[i] * (u[1] - u[0]) ** 2 / 8 + 1e-12 * abs(got[i])
    # no gain where Re <d|h> <= 0 (or there is no template), and A_hat, D_hat of the last call
    assert np.array_equal(got[[2, 3, 4]], np.full(3, -0.5 * d_d))
    assert np.array_equal(P.last["A_hat"], np.array([0.6, 1.0, 0.0, 0.0, 0.0, 0.4]))
    assert np.allclose(P.last["D_hat"][[0, 1, 5]], 2.0 / np.array([0.6, 1.0, 0.4]), rtol=1e-15)
    assert np.all(np.isinf(P.last["D_hat"][[2, 3, 4]]))
    assert np.all(got >= lk.profile_none(d_d, re, hh))


DIST_REF, DIST_RANGE, D_D = 2.4539054256, (1.0, 10.0), 7.0
U_LO, U_HI = DIST_REF / DIST_RANGE[1], DIST_REF / DIST_RANGE[0]
# the peak u* = Re <d|h> / <h|h>: inside the range, at either edge, outside on either side
# (and on the far side of 0). The largest |log| of these cases is 3.6e6 < 2^22, where a double's
# spacing is 4.7e-10: the 1e-9 asserted below can be represented.
PEAKS = (1.0, U_LO, U_HI, 0.5 * U_LO, 1.1 * U_HI, -1.0, 0.0)


def _quad_reference(re, hh, power):
    from scipy.integrate import quad
    lo, hi = DIST_RANGE
    norm = (hi ** (power + 1) - lo ** (power + 1)) / (power + 1)
    expo = lambda u: u * re - 0.5 * u * u * hh   # noqa: E731
    us, sg = (re / hh, hh ** -0.5) if hh > 0 else (0.0, 1.0)
    m = max(expo(U_LO), expo(U_HI), expo(min(max(us, U_LO), U_HI)))
    f = lambda u: (DIST_REF / u) ** power / norm * DIST_REF / u ** 2 * np.exp(expo(u) - m)  # noqa
    pts = [us + k * sg for k in (-40, -20, -10, -6, -4, -2, -1, 0, 1, 2, 4, 6, 10, 20, 40)]
    # (and a ladder in from each end: a peak outside leaves an exponential against the end)
    pts += [U_LO + (U_HI - U_LO) * 2.0 ** -j for j in range(1, 45)]
    pts += [U_HI - (U_HI - U_LO) * 2.0 ** -j for j in range(1, 45)]
    pts = np.unique(np.clip(pts + [U_LO, U_HI], U_LO, U_HI))
    tot = 0.0
    for a, b in zip(pts[:-1], pts[1:]):
        v, _ = quad(f, a, b, epsrel=1e-13, epsabs=0.0, limit=400)
        tot += v
    return np.log(tot) + m - 0.5 * D_D


@pytest.mark.filterwarnings("ignore::scipy.integrate.IntegrationWarning")
@pytest.mark.parametrize("hh", [0.0, 1.0, 2.5e3, 1e6])
def test_distance_marginalisation_against_quad(hh):
    """log int pi(D) exp(-1/2 d_d + u Re<d|h> - 1/2 u^2 <h|h>) dD against scipy's adaptive
    quadrature of the definition (epsrel 1e-13, break points at u* +- k sigma). Measured worst
    |error in log| over these cases with DISTANCE_NODES = 16: 5.8e-11 at h_h = 1e6 (where
    |log| reaches 3.6e6 and a double's spacing is 4.7e-10: the last digits of the two sums),
    1.8e-12 at h_h = 2.5e3, 2.2e-15 at h_h <= 1."""
    worst = 0.0
    for power in (2, 0):
        for us in PEAKS:
            re = us * hh if hh > 0 else us
            ref = _quad_reference(re, hh, power)
            got = lk.marginalize_distance(D_D, [re], [hh], DIST_REF, DIST_RANGE, power)[0]
            assert np.isfinite(got)
            worst = max(worst, abs(got - ref))
            print(f"hh={hh:g} u*={us:.4f} p={power} ref={ref!r} got={got!r} "
                  f"err={abs(got - ref):.2e}")
            assert abs(got - ref) <= 1e-9
    print("worst:", worst)


def test_distance_mode_needs_its_arguments_and_stays_finite():
    with pytest.raises(ValueError):
        lk.ProfiledLikelihood(_NoLike(), "distance")
    with pytest.raises(ValueError):
        lk.ProfiledLikelihood(_NoLike(), "phase")
    P = lk.ProfiledLikelihood(_NoLike(), "distance", dist_ref=DIST_REF, dist_range=DIST_RANGE)
    got = P.combine(D_D, np.zeros(3, dtype=np.complex128), np.zeros(3))
    # no template: the integrand is the normalised prior alone
    assert np.all(np.abs(got + 0.5 * D_D) <= 1e-14)
