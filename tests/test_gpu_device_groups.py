"""The device upstream (upstream="device", trajectory="device") over several groups: the rotating
groups' reuse, lane ranges with lanes_host, switching routes on one object, and a host-side
failure in a later group. STAND-IN PHYSICS, NOT FEW.

A row's launches do not depend on which group it falls in, so everything here is bitwise: several
groups against one group, a repeated call against its first. Public API only.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import pe  # noqa: E402
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)
M, MU, E0, T, DT, EPS = 1e6, 10.0, 0.35, 0.1, 10.0, 1e-2   # about 3.2e5 bins
KW = dict(T=T, dt=DT, eps=EPS)
ROUTES = [dict(upstream="device"), dict(upstream="device", trajectory="device")]
ROUTE_IDS = ["host_trajectory", "device_trajectory"]


@pytest.fixture(scope="module")
def scan():
    p0 = get_p_at_t(EMRIInspiral(), 0.99 * T, [M, MU, 0.0, E0, 1.0])
    base = np.array([M, MU, 0.0, p0, E0, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4])
    rows = np.repeat(base[None, :], 5, axis=0)
    rows[:, 0] *= [1.0, 1.0 + 2e-4, 1.0 - 3e-4, 1.0 + 1e-4, 1.0 - 1e-4]   # distinct M
    rows[:, 4] += [0.0, 2e-3, -1e-3, 1e-3, -2e-3]                         # distinct e0
    rows[:, 11] = [0.2, 1.7, 4.0, 2.9, 5.5]                               # distinct Phi_phi0
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW,
                               use_gpu=True, return_list=True)
    return gen, rows


def _nan(shape):
    return torch.full(shape, complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")


def _generate(gen, rows, **extra):
    out = _nan((len(rows), 2, gen.positive_bins(T=T, dt=DT)))
    gen.generate_batch(rows, out, **KW, **extra)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _both(gen, rows, **extra):
    """generate_batch, then spectrum_batch with lane ranges and check=False: (h, S, lanes,
    lanes_host as read right after lanes_ready(), generate_batch's last_modes_batch)."""
    wg = gen.waveform_generator
    B = len(rows)
    nf = int(wg.create_waveform._grid(T, DT, None)[0].numel())
    assert 3.0e5 < nf < 3.4e5
    h = _generate(gen, rows, **extra)
    modes = wg.last_modes_batch
    S = _nan((B, nf))
    lanes = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    lanes_host = torch.full((B, 2), -1, dtype=torch.int32).pin_memory()
    gen.spectrum_batch(rows, S, lanes=lanes, lanes_host=lanes_host, check=False, **KW, **extra)
    gen.lanes_ready()
    lh = lanes_host.numpy().copy()
    gen.check_batch()
    torch.cuda.synchronize()
    return h, S.cpu().numpy(), lanes.cpu().numpy(), lh, modes


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_generator_groups_and_slot_reuse(scan, monkeypatch, route):
    """5 rows in groups of 2 (the third group reuses the first's resources) against one group."""
    gen, rows = scan
    monkeypatch.setattr(GenerateEMRIWaveform, "BATCH_GROUP", 16)
    h1, S1, l1, lh1, m1 = _both(gen, rows, **route)
    monkeypatch.setattr(GenerateEMRIWaveform, "BATCH_GROUP", 2)
    h3, S3, l3, lh3, m3 = _both(gen, rows, **route)
    assert np.isfinite(h1).all() and np.isfinite(S1).all() and (l1 >= 0).all()
    assert (l1[:, 0] < l1[:, 1]).all()
    np.testing.assert_array_equal(h3, h1)
    np.testing.assert_array_equal(S3, S1)
    np.testing.assert_array_equal(l3, l1)
    np.testing.assert_array_equal(lh1, l1)
    np.testing.assert_array_equal(lh3, l3)
    # last_modes_batch: the last group's rows (all five; then row 4 alone)
    assert len(m1) == 5 and len(m3) == 1
    for a, b in zip(m3[0], m1[4]):
        np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def setups():
    made = {}

    def get(**route):
        key = tuple(sorted(route.items()))
        if key not in made:
            made[key] = pe.setup(Tobs=T, dt=DT, eps=EPS, nwalkers=4, **route)
        return made[key]

    return get


def _points(s):
    """17 points: the start walkers tiled with small distinct offsets, the truth last."""
    pts = np.tile(s.start, (4, 1))
    k = np.arange(len(pts), dtype=np.float64)
    pts[:, 3] += 1e-6 * k          # e0
    pts[:, 4] += 1e-3 * k          # Phi_phi0
    pts = np.concatenate([pts, s.truth6[None, :]])
    assert len(pts) == 17 and len(np.unique(pts, axis=0)) == 17
    return pts


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_likelihood_groups(setups, route):
    """17 walkers are two balanced groups of 9 and 8: bitwise those groups' own calls."""
    s = setups(**route)
    assert s.like.device_upstream is True
    assert s.like.device_trajectory is (route.get("trajectory") == "device")
    pts = _points(s)
    ll = s.like(pts, **s.kwargs)
    a, b = s.like(pts[:9], **s.kwargs), s.like(pts[9:], **s.kwargs)
    assert ll.shape == (17,) and np.all(np.isfinite(ll))
    np.testing.assert_array_equal(ll, np.concatenate([a, b]))
    np.testing.assert_array_equal(s.like(pts, **s.kwargs), ll)
    assert ll[-1] == b[-1]
    assert np.all(ll[:-1] < ll[-1])            # the truth is the best of them


def test_route_switching_generator(scan):
    gen, rows = scan
    host = _generate(gen, rows)
    dev = _generate(gen, rows, upstream="device")
    np.testing.assert_array_equal(_generate(gen, rows), host)
    np.testing.assert_array_equal(_generate(gen, rows, upstream="device"), dev)
    np.testing.assert_array_equal(_generate(gen, rows), host)
    assert np.isfinite(host).all() and np.isfinite(dev).all()


def test_route_switching_likelihood(setups):
    """A host and a device Likelihood around one template, interleaved; then one Likelihood
    switched between the routes."""
    from emri_frequencydomainwaveforms_amd.fdutils import get_sensitivity
    from emri_frequencydomainwaveforms_amd.likelihood import Likelihood
    sh = setups()
    assert sh.like.device_upstream is False
    ld = Likelihood(sh.gen, 2, parameter_transforms={"emri": sh.transform}, vectorized=False,
                    transpose_params=False, subset=24, f_arr=sh.f_like, use_gpu=True)
    ld.device_upstream = True
    ld.inject_signal(data_stream=sh.gen(*sh.truth14, **sh.kwargs),
                     noise_fn=[get_sensitivity, get_sensitivity], noise_kwargs=[{}, {}])
    pts = _points(sh)
    host = sh.like(pts, **sh.kwargs)
    dev = ld(pts, **sh.kwargs)
    assert np.all(np.isfinite(host)) and np.all(np.isfinite(dev)) and host[-1] == 0.0
    for _ in range(2):
        np.testing.assert_array_equal(sh.like(pts, **sh.kwargs), host)
        np.testing.assert_array_equal(ld(pts, **sh.kwargs), dev)
    try:
        sh.like.device_upstream = True
        np.testing.assert_array_equal(sh.like(pts, **sh.kwargs), dev)
    finally:
        del sh.like.device_upstream
    np.testing.assert_array_equal(sh.like(pts, **sh.kwargs), host)


def test_host_failure_in_a_later_group(scan, monkeypatch):
    """Row 3's host trajectory refuses its source (p0 inside the separatrix): the call raises
    from the second group, the device is left idle and sound, and the generator still works."""
    gen, rows = scan
    monkeypatch.setattr(GenerateEMRIWaveform, "BATCH_GROUP", 2)
    good = _generate(gen, rows, upstream="device")
    assert np.isfinite(good).all()
    bad = rows.copy()
    bad[3, 3] = 5.0
    out = _nan((5, 2, gen.positive_bins(T=T, dt=DT)))
    with pytest.raises(ValueError, match="separatrix"):
        gen.generate_batch(bad, out, upstream="device", **KW)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_generate(gen, rows, upstream="device"), good)
