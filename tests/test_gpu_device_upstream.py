"""The batched callers with the amplitudes and the mode selection on the device
(upstream="device": generate_batch, spectrum_batch, pe.setup / Likelihood.device_upstream)
against the default host route. STAND-IN PHYSICS, NOT FEW.

The device amplitudes agree with the host's to 1e-14 max|A| (tests/test_gpu_modes_device.py),
not bitwise, so the templates are compared under the mode sum's own response to that agreement,
measured here from the host route alone: every host amplitude is multiplied by 1 + 1e-14 r, r
uniform in [-1, 1] from a fixed seed, and the allowed difference is twice the change that makes
(INTEGRATION.md section 3's factor for conditioning-limited bins).
"""

import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import pe  # noqa: E402
from emri_frequencydomainwaveforms_amd.amplitude import SyntheticTeukolskyAmplitude  # noqa: E402
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)
M, MU, E0, T, DT = 1e6, 10.0, 0.35, 0.1, 10.0    # S1: about 3.2e5 bins
PERTURB = 1e-14


@contextlib.contextmanager
def perturbed_host_amplitudes(seed=20260115):
    """The host upstream's amplitudes times 1 + PERTURB r, r in [-1, 1] (the same r for every
    call of a shape: the prefetch pool's threads take the calls in any order)."""
    orig = SyntheticTeukolskyAmplitude.select

    def select(self, p, e, ylms, eps, lib=None):
        keep, teuk = orig(self, p, e, ylms, eps, lib=lib)
        r = np.random.default_rng(seed).uniform(-1.0, 1.0, teuk.shape)
        return keep, np.ascontiguousarray(teuk * (1.0 + PERTURB * r))

    SyntheticTeukolskyAmplitude.select = select
    try:
        yield
    finally:
        SyntheticTeukolskyAmplitude.select = orig


@pytest.fixture(scope="module")
def scan():
    p0 = get_p_at_t(EMRIInspiral(), 0.99 * T, [M, MU, 0.0, E0, 1.0])
    base = np.array([M, MU, 0.0, p0, E0, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4])
    rows = np.repeat(base[None, :], 3, axis=0)
    rows[:, 0] *= [1.0, 1.0 + 2e-4, 1.0 - 3e-4]        # distinct M
    rows[:, 4] += [0.0, 2e-3, -1e-3]                    # distinct e0
    rows[:, 11] = [0.2, 1.7, 4.0]                       # distinct Phi_phi0
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW,
                               use_gpu=True, return_list=True)
    return gen, rows


@pytest.mark.parametrize("eps", [1e-2, 1e-5])
def test_templates_match_host_route(scan, eps):
    gen, rows = scan
    kw = dict(T=T, dt=DT, eps=eps)
    wg = gen.waveform_generator
    npos = gen.positive_bins(T=T, dt=DT)
    nf = int(wg.create_waveform._grid(T, DT, None)[0].numel())
    assert 3.0e5 < nf < 3.4e5

    def run(**extra):
        out = torch.full((3, 2, npos), complex(np.nan, np.nan), dtype=torch.complex128,
                         device="cuda")
        S = torch.full((3, nf), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        gen.generate_batch(rows, out, **kw, **extra)
        gen.spectrum_batch(rows, S, **kw, **extra)
        torch.cuda.synchronize()
        return out.cpu().numpy(), S.cpu().numpy()

    h_host, S_host = run()
    with perturbed_host_amplitudes():
        h_pert, S_pert = run()
    h_dev, S_dev = run(upstream="device")
    # the kept modes are the host route's
    calls, _ = gen.device_calls(rows, T, eps)
    assert len(wg.last_modes_batch) == 3
    for c, got in zip(calls, wg.last_modes_batch):
        wg._upstream(*c, None, True)
        for a, b in zip(got, wg.last_modes):
            np.testing.assert_array_equal(a, b)
    for b in range(3):
        for name, host, pert, dev in (("generate_batch", h_host, h_pert, h_dev),
                                      ("spectrum_batch", S_host, S_pert, S_dev)):
            tol = 2.0 * np.abs(pert[b] - host[b]).max()
            err = np.abs(dev[b] - host[b]).max()
            mx = np.abs(host[b]).max()
            print(f"eps={eps:g} row {b} {name}: |device - host| = {err / mx:.3g} max|S|, "
                  f"allowed 2 x perturbed response = {tol / mx:.3g} max|S|")
            assert np.isfinite(dev[b]).all() and tol > 0.0
            assert err <= tol, (name, b, err / mx, tol / mx)


def test_likelihood_matches_host_route():
    """pe.setup(upstream="device") against the default setup on the start walkers and on the
    truth: |dlogL| <= 2 (4 |r| delta + 2 delta^2), |r| = sqrt(-logL_host / 2), delta = the norm
    of the perturbed host route's weighted template change; at the truth the host logL is
    exactly 0 and the bound is 4 delta^2."""
    sh = pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4)
    sd = pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, upstream="device")
    assert sd.like.device_upstream is True and sh.like.device_upstream is False
    assert type(sh.like).device_upstream is False
    np.testing.assert_array_equal(sh.start, sd.start)
    pts = np.concatenate([sh.start, sh.truth6[None, :]])
    ll_host = sh.like(pts, **sh.kwargs)
    ll_dev = sd.like(pts, **sd.kwargs)
    np.testing.assert_array_equal(ll_host, sh.like(pts, **sh.kwargs))
    assert ll_host[-1] == 0.0 and np.all(ll_host[:-1] < 0.0)
    p14 = sh.transform.both_transforms(pts)
    n = len(pts)
    nb = int(sh.like._d.shape[1])

    def templates():
        out = torch.empty((n, 2, nb), dtype=torch.complex128, device="cuda")
        sh.few.generate_batch(p14, out, **sh.kwargs)
        torch.cuda.synchronize()
        return out

    h0 = templates()
    with perturbed_host_amplitudes():
        h1 = templates()
    w = sh.like._w_templ
    delta = torch.sqrt((((h1 - h0) * w[None]).abs() ** 2).sum(dim=(1, 2))).cpu().numpy()
    rnorm = np.sqrt(-ll_host / 2.0)
    bound = 2.0 * (4.0 * rnorm * delta + 2.0 * delta ** 2)
    diff = np.abs(ll_dev - ll_host)
    for i in range(n):
        print(f"walker {i}: logL host {ll_host[i]:.17g} device {ll_dev[i]:.17g} "
              f"|diff| {diff[i]:.3g} bound {bound[i]:.3g} (delta {delta[i]:.3g})")
    assert np.all(delta > 0.0) and bound[-1] == 4.0 * delta[-1] ** 2
    assert np.all(np.isfinite(ll_dev))
    assert np.all(diff <= bound), (diff, bound)


def test_upstream_argument_errors(scan):
    gen, rows = scan
    npos = gen.positive_bins(T=T, dt=DT)
    out = torch.empty((3, 2, npos), dtype=torch.complex128, device="cuda")
    kw = dict(T=T, dt=DT, eps=1e-2)
    with pytest.raises(ValueError):
        gen.generate_batch(rows, out, upstream="bogus", **kw)
    with pytest.raises(ValueError):
        gen.generate_batch(rows, out, upstream="device", mode_selection=[(2, 2, 0)], **kw)
    nf = int(gen.waveform_generator.create_waveform._grid(T, DT, None)[0].numel())
    S = torch.empty((3, nf), dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError):
        gen.spectrum_batch(rows, S, upstream="bogus", **kw)
    with pytest.raises(ValueError):
        gen.spectrum_batch(rows, S, upstream="device", mode_selection=[(2, 2, 0)], **kw)
    with pytest.raises(ValueError):
        pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, upstream="bogus")
