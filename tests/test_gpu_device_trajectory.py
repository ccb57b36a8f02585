"""The batched callers with the trajectories on the device as well (upstream="device",
trajectory="device": generate_batch, spectrum_batch, pe.setup / Likelihood.device_trajectory).
STAND-IN PHYSICS, NOT FEW.

(a) The plumbing is exact: the device knots, downloaded and handed to the existing
    device_inputs_batch(..., futures=...) route as completed futures, give bitwise the templates
    of trajectory="device".
(b) Against the host route: two valid integrations place their knots differently, so the
    templates are compared under the reference's own response to that, measured from the default
    route alone: the allowed difference per row is twice |template(native trajectory) -
    template(EMRIInspiral(backend="python") trajectory)|.
(c) The likelihood under the same Cauchy-Schwarz form as test_gpu_device_upstream.py's, with
    delta from (b)'s yardstick.
(d) Argument errors.

Measured on an MI355X, |device trajectory - host| and the allowed 2 x |python backend - native|,
both over max|S|, rows 0, 1, 2 (generate_batch; spectrum_batch's figures are within 25 %):
  eps = 1e-2   4.4e-15 / 8.1e-4    5.1e-16 / 2.0e-7    8.7e-11 / 4.2e-6
  eps = 1e-5   4.3e-15 / 6.4e-2    5.0e-16 / 1.3e-4    7.9e-4 / 1.6e-1
(rows 0 and 1 follow the host's steps bit for bit and differ by the device amplitudes alone; on
row 2 one power call rounds differently and the conditioning-limited bin of
test_gpu_device_upstream.py responds). logL differences 4.3e-19 ... 1.8e-12 under bounds
1.8e-6 ... 2.0e-5; 3.9e-20 under 5.0e-8 at the truth. With butterfly sums, an earlier form, the
device placed its knots as a third valid integration and row 1 missed (3.2e-5 against 2.0e-7).
"""

from concurrent.futures import Future

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import pe  # noqa: E402
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)
M, MU, E0, T, DT = 1e6, 10.0, 0.35, 0.1, 10.0    # test_gpu_device_upstream.py's shape: 3.2e5 bins


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
    gen_py = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW,
                                  use_gpu=True, return_list=True,
                                  inspiral_kwargs=dict(backend="python"))
    assert gen.waveform_generator.inspiral_generator.backend == "native"
    assert gen_py.waveform_generator.inspiral_generator.backend == "python"
    return gen, gen_py, rows


def _run(gen, rows, eps, **extra):
    npos = gen.positive_bins(T=T, dt=DT)
    nf = int(gen.waveform_generator.create_waveform._grid(T, DT, None)[0].numel())
    assert 3.0e5 < nf < 3.4e5
    out = torch.full((len(rows), 2, npos), complex(np.nan, np.nan), dtype=torch.complex128,
                     device="cuda")
    S = torch.full((len(rows), nf), complex(np.nan, np.nan), dtype=torch.complex128,
                   device="cuda")
    gen.generate_batch(rows, out, T=T, dt=DT, eps=eps, **extra)
    gen.spectrum_batch(rows, S, T=T, dt=DT, eps=eps, **extra)
    torch.cuda.synchronize()
    return out.cpu().numpy(), S.cpu().numpy()


@pytest.mark.parametrize("eps", [1e-2, 1e-5])
def test_templates_plumbing_exact_and_match_host_route(scan, eps):
    gen, gen_py, rows = scan
    wg = gen.waveform_generator
    h_dev, S_dev = _run(gen, rows, eps, upstream="device", trajectory="device")
    assert np.isfinite(h_dev).all() and np.isfinite(S_dev).all()

    # (a) the same knots through the existing route: completed futures in place of the pool's
    calls, _ = gen.device_calls(rows, T, eps)
    views = wg.device_trajectories(calls)
    torch.cuda.synchronize()
    knots = {c: tuple(v.cpu().numpy() for v in vs) for c, vs in zip(calls, views)}
    assert all(len(k) == 7 and len(k[0]) >= 2 for k in knots.values())

    def completed(cs):
        futs = []
        for c in cs:
            f = Future()
            f.set_result(knots[tuple(c)])
            futs.append(f)
        return futs

    wg.trajectories_async = completed          # (an instance attribute over the method)
    try:
        h_fut, S_fut = _run(gen, rows, eps, upstream="device")
    finally:
        del wg.trajectories_async
    np.testing.assert_array_equal(h_dev, h_fut)
    np.testing.assert_array_equal(S_dev, S_fut)

    # (b) against the default route, under its own response to another valid knot placement
    h_host, S_host = _run(gen, rows, eps)
    h_py, S_py = _run(gen_py, rows, eps)
    missed = []
    for b in range(len(rows)):
        for name, host, py, dev in (("generate_batch", h_host, h_py, h_dev),
                                    ("spectrum_batch", S_host, S_py, S_dev)):
            tol = 2.0 * np.abs(py[b] - host[b]).max()
            err = np.abs(dev[b] - host[b]).max()
            mx = np.abs(host[b]).max()
            print(f"eps={eps:g} row {b} {name}: |device trajectory - host| = {err / mx:.3g} "
                  f"max|S|, allowed 2 x |python backend - native| = {tol / mx:.3g} max|S|")
            assert tol > 0.0
            if not err <= tol:
                missed.append((name, b, err / mx, tol / mx))
    assert not missed, missed


def test_likelihood_matches_host_route():
    """pe.setup(upstream="device", trajectory="device") against the default setup on the start
    walkers and on the truth: |dlogL| <= 2 (4 |r| delta + 2 delta^2), |r| = sqrt(-logL_host / 2),
    delta = the norm of the default route's weighted template change between the native and the
    python backend's trajectories; at the truth the host logL is exactly 0 and the bound is
    4 delta^2."""
    sh = pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4)
    sd = pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, upstream="device", trajectory="device")
    assert sd.like.device_upstream is True and sd.like.device_trajectory is True
    assert sh.like.device_trajectory is False and type(sh.like).device_trajectory is False
    np.testing.assert_array_equal(sh.start, sd.start)
    pts = np.concatenate([sh.start, sh.truth6[None, :]])
    ll_host = sh.like(pts, **sh.kwargs)
    ll_dev = sd.like(pts, **sd.kwargs)
    np.testing.assert_array_equal(ll_dev, sd.like(pts, **sd.kwargs))
    assert ll_host[-1] == 0.0 and np.all(ll_host[:-1] < 0.0)
    p14 = sh.transform.both_transforms(pts)
    n = len(pts)
    nb = int(sh.like._d.shape[1])
    few_py = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=pe.SUM_KW,
                                  use_gpu=True, return_list=True,
                                  inspiral_kwargs=dict(backend="python"))

    def templates(few):
        out = torch.empty((n, 2, nb), dtype=torch.complex128, device="cuda")
        few.generate_batch(p14, out, **sh.kwargs)
        torch.cuda.synchronize()
        return out

    h0, h1 = templates(sh.few), templates(few_py)
    w = sh.like._w_templ
    delta = torch.sqrt((((h1 - h0) * w[None]).abs() ** 2).sum(dim=(1, 2))).cpu().numpy()
    rnorm = np.sqrt(-ll_host / 2.0)
    bound = 2.0 * (4.0 * rnorm * delta + 2.0 * delta ** 2)
    diff = np.abs(ll_dev - ll_host)
    for i in range(n):
        print(f"walker {i}: logL host {ll_host[i]:.17g} device trajectory {ll_dev[i]:.17g} "
              f"|diff| {diff[i]:.3g} bound {bound[i]:.3g} (delta {delta[i]:.3g})")
    assert np.all(delta > 0.0) and bound[-1] == 4.0 * delta[-1] ** 2
    assert np.all(np.isfinite(ll_dev))
    assert np.all(diff <= bound), (diff, bound)


def test_trajectory_argument_errors(scan):
    gen, _, rows = scan
    npos = gen.positive_bins(T=T, dt=DT)
    out = torch.empty((3, 2, npos), dtype=torch.complex128, device="cuda")
    nf = int(gen.waveform_generator.create_waveform._grid(T, DT, None)[0].numel())
    S = torch.empty((3, nf), dtype=torch.complex128, device="cuda")
    kw = dict(T=T, dt=DT, eps=1e-2)
    for call, buf in ((gen.generate_batch, out), (gen.spectrum_batch, S)):
        with pytest.raises(ValueError):
            call(rows, buf, trajectory="device", **kw)                   # needs upstream="device"
        with pytest.raises(ValueError):
            call(rows, buf, upstream="host", trajectory="device", **kw)
        with pytest.raises(ValueError):
            call(rows, buf, upstream="device", trajectory="bogus", **kw)
        with pytest.raises(ValueError):
            call(rows, buf, trajectory="bogus", **kw)
    with pytest.raises(ValueError):
        pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, trajectory="device")
    with pytest.raises(ValueError):
        pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, upstream="device", trajectory="bogus")
