"""GPU parity of the cosine-sum windows' path (fdutils.CosineWindowConvolution; efd_cosw_*):
the stencil against the exact size-N DFT form and against the numpy first-order reference
(tests/cosine_window_ref.py), the pair-form logL against the written templates, and the API
(pe.setup(window=...), get_fd_waveform_fromFD, Likelihood) at the smallest grid that takes it.
"""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import scipy.signal.windows as sw  # noqa: E402

from emri_frequencydomainwaveforms_amd import _lib, pe  # noqa: E402
from emri_frequencydomainwaveforms_amd.fdutils import (COSINE_WINDOWS,  # noqa: E402
                                                       CosineWindowConvolution,
                                                       HannConvolution, window_multiplier,
                                                       windowed_spectrum)
from emri_frequencydomainwaveforms_amd.reductions import Reducer  # noqa: E402
from emri_frequencydomainwaveforms_amd.summation import td_length  # noqa: E402
from tests import cosine_window_ref as ref  # noqa: E402

TEST_SH_SOURCE = dict(dt=10.0, eps=1e-2, M=3670041.7362535275, mu=292.0583167470244,
                      e0=0.5794130830706371)


def _ptr(t):
    return torch.view_as_real(t).data_ptr() if t.is_complex() else t.data_ptr()


def _coeffs(a):
    return (ctypes.c_double * len(a))(*a)


def _tol_pol(a, n):
    """The Hann tests' tol_pol (a batch's and a single row's complex64 correction round
    differently: |dC| ~ 2^-23 |C|, |C| <= max|S| ln n, Hann weight e / 4 on each of two
    neighbours) scaled by this stencil's weight 2 sum_j j a_j (Hann: 1)."""
    return 2.0 ** -23 * np.log(n) * ref.stencil_weight(a) / (n - 1) + 1e-14


@pytest.mark.parametrize("support", [(1 / 3, 1.0), (0.45, 0.55), (0.0, 1.0)])
@pytest.mark.parametrize("name", ["blackman", "nuttall", "hamming", "blackmanharris"])
def test_stencil_matches_dft_form(name, support):
    """CosineWindowConvolution's windowed spectrum against windowed_spectrum (FP64 rocFFT) on
    two rows (the second scaled by 1e-21) of a random-phase spectrum nonzero on a sub-range,
    the last one the whole grid (the stencil wraps at both ends): within 10 q / n^2 + 1e-13 of
    each row's max|S|; and efd_cosw_polarizations of one row against efd_polarizations of the
    two-row call's windowed spectrum within tol_pol (_tol_pol)."""
    n = 100001
    a = COSINE_WINDOWS[name]
    rng = np.random.default_rng(n + len(name))
    S = rng.normal(size=(2, n)) + 1j * rng.normal(size=(2, n))
    lo, hi = int(support[0] * n), int(support[1] * n)
    S[:, :lo] = 0.0
    S[:, hi:] = 0.0
    S[1] *= 1e-21
    St = torch.as_tensor(S, device="cuda")
    w = getattr(sw, name)(n)
    cwc = CosineWindowConvolution(n, St.device, a)
    got = cwc(St)
    exact = windowed_spectrum(St, window_multiplier(w))
    tol = ref.bound(a, n) + 1e-13
    for r in range(2):
        mx = float(St[r].abs().max())
        err = float((got[r] - exact[r]).abs().max())
        print(f"{name} {support} row {r}: err / (tol max|S|) = {err / (tol * mx):.3f}")
        assert err <= tol * mx
    lib = _lib.load()
    k0 = n // 2
    tol_pol = _tol_pol(a, n)
    for r in range(2):
        hp = torch.empty(n - k0, dtype=torch.complex128, device="cuda")
        hc = torch.empty_like(hp)
        hp_ref = torch.empty_like(hp)
        hc_ref = torch.empty_like(hp)
        one = CosineWindowConvolution(n, St.device, a)
        one.polarizations(St[r].contiguous(), hp, hc, k0, lib)
        Sw = got[r].contiguous()
        _lib.check(lib.efd_polarizations(_ptr(Sw), n, k0, _ptr(hp_ref), _ptr(hc_ref), None),
                   "efd_polarizations", lib)
        torch.cuda.synchronize()
        mx = float(St[r].abs().max())
        ep, ec = float((hp - hp_ref).abs().max()), float((hc - hc_ref).abs().max())
        print(f"  polarizations row {r}: err / (tol_pol max|S|) = "
              f"{max(ep, ec) / (tol_pol * mx):.3f}")
        assert ep <= tol_pol * mx and ec <= tol_pol * mx


@pytest.mark.parametrize("scale", [1.0, 1e-21])
def test_smallest_grid_against_numpy_reference(scale):
    """n = 101, k0 = 50, full support, nuttall (J = 3: bins 0-2 and 98-100 wrap): the kernel's
    h+/hx against the numpy first-order reference fed the kernel's own C (gathered from Y as
    HannConvolution.correction does), within 2e-15 of max|S| (at most 2J + 2 FP64 roundings of
    terms no larger than max|S|); and efd_cosw_polarizations with a = (1/2, 1/2) against
    efd_hann_polarizations on the same Y, within the same."""
    n, k0 = 101, 50
    a = COSINE_WINDOWS["nuttall"]
    rng = np.random.default_rng(101)
    S = (rng.normal(size=n) + 1j * rng.normal(size=n)) * scale
    St = torch.as_tensor(S, device="cuda")[None].contiguous()
    lib = _lib.load()
    cwc = CosineWindowConvolution(n, St.device, a)
    Y, info, m = cwc.transform(St, lib)
    first = int(info[0, 1])
    assert first == 0 and int(info[0, 2]) == n and m >= 2 * n
    sc = float(info[0, 0:1].view(torch.float64)[0])
    q = (np.arange(n) - first) % n + (m - n)
    C = Y[0].cpu().numpy()[q].astype(np.complex128) * sc
    mx = np.abs(S).max()

    def run(fn, *coef):
        hp = torch.empty(n - k0, dtype=torch.complex128, device="cuda")
        hc = torch.empty_like(hp)
        _lib.check(fn(_ptr(St[0]), _ptr(Y[0]), info[0].data_ptr(), m, n, k0, *coef, _ptr(hp),
                      _ptr(hc), None), "polarizations", lib)
        torch.cuda.synchronize()
        return hp.cpu().numpy(), hc.cpu().numpy()

    hp, hc = run(lib.efd_cosw_polarizations, _coeffs(a), len(a))
    hp_ref, hc_ref = ref.polarizations(ref.first_order(S, a, C), k0)
    err = max(np.abs(hp - hp_ref).max(), np.abs(hc - hc_ref).max())
    print(f"nuttall n=101 scale {scale}: err / max|S| = {err / mx:.3e}")
    assert err <= 2e-15 * mx
    # not Hann's stencil by accident: the two differ by far more than the tolerance
    hann = (0.5, 0.5)
    hp_h, hc_h = run(lib.efd_hann_polarizations)
    assert np.abs(hp - hp_h).max() > 1e-3 * mx
    hp_1, hc_1 = run(lib.efd_cosw_polarizations, _coeffs(hann), 2)
    err = max(np.abs(hp_1 - hp_h).max(), np.abs(hc_1 - hc_h).max())
    print(f"a = (1/2, 1/2) against efd_hann_polarizations: err / max|S| = {err / mx:.3e}")
    assert err <= 2e-15 * mx


def test_argument_errors():
    """nf < 2 (nterm - 1) + 1, nterm outside 2..4 and a NULL coefficient array return
    EFD_ERR_ARG before anything touches the device."""
    lib = _lib.load()
    fake = ctypes.c_void_p(16)
    a = _coeffs(COSINE_WINDOWS["nuttall"])
    buf = ctypes.create_string_buffer(256)
    assert lib.efd_cosw_polarizations(fake, fake, fake, 8, 5, 2, a, 4, fake, fake, None) == -1
    lib.efd_last_error(buf, 256)
    assert b"efd_cosw_polarizations" in buf.value
    assert lib.efd_cosw_loglike(fake, 5, fake, fake, 8, 1, 5, 2, a, 4, fake, fake, fake, fake,
                                None) == -1
    lib.efd_last_error(buf, 256)
    assert b"efd_cosw_loglike" in buf.value
    for nterm in (1, 5):
        assert lib.efd_cosw_polarizations(fake, fake, fake, 128, 101, 50, a, nterm, fake, fake,
                                          None) == -1
    assert lib.efd_cosw_polarizations(fake, fake, fake, 128, 101, 50, None, 4, fake, fake,
                                      None) == -1
    assert lib.efd_cosw_loglike(fake, 101, fake, fake, 128, 17, 101, 50, a, 4, fake, fake, fake,
                                fake, None) == -1


@pytest.mark.parametrize("name", ["blackman", "nuttall"])
def test_loglike_matches_templates(name):
    """efd_cosw_loglike (no template written) against efd_cosw_polarizations + efd_loglike on
    rows of two different supports and an all-zero row (its logL is the data-only term):
    1e-12 relative (reduction order). Then four rows in one call (two rows a workgroup) against
    the first three in another (one row a workgroup), on the same transformed rows: bitwise
    (a row's logL does not depend on the row grouping or on the other rows; the comparison
    holds Y fixed because a batched transform may round a row differently in another batch)."""
    lib = _lib.load()
    a = COSINE_WINDOWS[name]
    n = 200001
    k0 = n // 2
    nb = n - k0
    rng = np.random.default_rng(7)
    S = (rng.normal(size=(4, n)) + 1j * rng.normal(size=(4, n))) * 1e-20
    S[0, : n // 4] = S[0, 3 * n // 4:] = 0.0
    S[1, : 2 * n // 5] = S[1, 3 * n // 5:] = 0.0
    S[2] = 0.0
    S[3, : n // 3] = S[3, 2 * n // 3:] = 0.0
    St = torch.as_tensor(S, device="cuda")
    d = torch.as_tensor((rng.normal(size=(2, nb)) + 1j * rng.normal(size=(2, nb))) * 1e-20,
                        device="cuda")
    w = torch.as_tensor(rng.uniform(0.5, 2.0, size=(2, nb)), device="cuda")
    cwc = CosineWindowConvolution(n, St.device, a)
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    scr = torch.empty(4 * _lib.EFD_LOGLIKE_SCRATCH, dtype=torch.float64, device="cuda")
    S3 = St[:3].contiguous()
    cwc.loglike_batch(S3, d, w, k0, out, scr, lib)
    red = Reducer(St.device)
    want = []
    for r in range(3):
        h = torch.empty((2, nb), dtype=torch.complex128, device="cuda")
        cwc.polarizations(S3[r].contiguous(), h[0], h[1], k0, lib)
        want.append(float(red.loglike(h, d, w)[0]))
    got = out.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got[2], float(red.loglike(None, d, w)[0]), rtol=1e-12, atol=0.0)
    assert got[0] != got[1] != got[2]
    # 4 rows (RPT = 2) and 3 rows (RPT = 1) of one transformed batch
    Y, info, m = cwc.transform(St, lib)
    outs = []
    for rows in (4, 3):
        o = torch.full((rows,), np.nan, dtype=torch.float64, device="cuda")
        _lib.check(lib.efd_cosw_loglike(_ptr(St), n, _ptr(Y), info.data_ptr(), m, rows, n, k0,
                                        _coeffs(a), len(a), _ptr(d), w.data_ptr(), o.data_ptr(),
                                        scr.data_ptr(), None), "efd_cosw_loglike", lib)
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy())
    assert np.array_equal(outs[0][:3], outs[1])
    np.testing.assert_allclose(outs[0][:3], want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", ["nuttall", "blackman"])
def test_api_smallest_full_size_grid(name):
    """pe.setup(window=name) with test.sh's source at Tobs = 1.07 yr, the shortest observation
    (in hundredths of a year, dt = 10 s) whose grid takes the first-order form for nuttall:
    the template model takes the batched path and never the Hann-only local logL form; fill
    against the exact transform pair of the same spectrum; fill_batch against fill; the
    likelihood's half-step against the written templates + efd_loglike, repeatable bitwise;
    the injection's logL against itself (measured 0.0 for both windows: the data and the
    template of the truth go through one-row transforms of the same spectrum)."""
    a = COSINE_WINDOWS[name]
    nut = COSINE_WINDOWS["nuttall"]
    assert CosineWindowConvolution.applies(td_length(1.07, 10.0), nut)
    assert not CosineWindowConvolution.applies(td_length(1.06, 10.0), nut)
    s = pe.setup(window=name, nwalkers=8, ntemps=1, Tobs=1.07, **TEST_SH_SOURCE)
    n = s.info["N_f"]
    assert n == td_length(1.07, 10.0) == 3376723 and s.info["window"] == name
    assert CosineWindowConvolution.applies(n, a) and s.half_step == 4
    gen, like = s.gen, s.like
    assert gen.can_fill and gen.can_fill_batch and not gen.can_pipeline
    assert gen._hann is None and isinstance(gen._cosw, CosineWindowConvolution)
    assert gen._cosw.coeffs == a and gen.window_name == name
    assert gen.hann_local(like._d, like._w_templ) is None
    assert like._hann_local(gen, s.kwargs) is None
    batch = s.half_steps()[0]
    params14 = s.transform.both_transforms(batch)
    nch, nb = like._d.shape
    cw = s.few.waveform_generator.create_waveform
    k0 = n - nb
    # fill against the exact size-N transform pair of the same spectrum
    S = s.few._spectrum(*params14[0], **s.kwargs)
    mx = float(S.abs().max())
    one = torch.empty((2, nb), dtype=torch.complex128, device="cuda")
    gen.fill(one, *params14[0], **s.kwargs)
    exact = torch.empty_like(one)
    cw.polarizations(windowed_spectrum(S, window_multiplier(gen.window)), True,
                     out=(exact[0], exact[1]))
    tol = ref.bound(a, n) + 2.0 ** -23 * np.log(n) * ref.stencil_weight(a) / (n - 1) + 1e-13
    err = float((one - exact).abs().max())
    print(f"{name} N={n}: fill against the DFT form, err / (tol max|S|) = {err / (tol * mx):.3f}")
    assert err <= tol * mx
    del exact
    # fill_batch of two walkers against their fills
    bufs = torch.empty((len(batch), nch, nb), dtype=torch.complex128, device="cuda")
    gen.fill_batch([bufs[i] for i in range(2)], params14[:2], **s.kwargs)
    for i in range(2):
        gen.fill(one, *params14[i], **s.kwargs)
        mxi = float(s.few._spectrum(*params14[i], **s.kwargs).abs().max())
        assert float((bufs[i] - one).abs().max()) <= _tol_pol(a, n) * mxi
    # the likelihood's half-step: in-place reduction against the written templates
    ll = like(batch, **s.kwargs)
    assert np.array_equal(like(batch, **s.kwargs), ll) and np.all(ll < 0.0)
    gen.fill_batch([bufs[i] for i in range(len(batch))], params14, **s.kwargs)
    ll_w = np.array([float(like._red.loglike(bufs[i], like._d, like._w_templ)[0])
                     for i in range(len(batch))])
    np.testing.assert_allclose(ll, ll_w, rtol=1e-12, atol=0.0)
    ll_truth = float(like(s.truth6[None, :], **s.kwargs)[0])
    print(f"{name}: logL(truth) = {ll_truth!r}, min |logL| = {np.abs(ll).min()!r}")
    assert abs(ll_truth) <= 1e-10 * np.abs(ll).min()
    assert k0 == gen._suffix_k0 and isinstance(gen._conv, HannConvolution)
