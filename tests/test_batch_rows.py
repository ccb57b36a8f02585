"""GenerateEMRIWaveform.device_calls, the one unpacking of a 14-parameter row for the batched
callers, against the spellings it replaced (submit_batch's, prefetch's, time_series_batch's and
its own), and the prefetch tables' key against prepare()'s. No GPU."""

import numpy as np
import pytest

from emri_frequencydomainwaveforms_amd.constants import Gpc, MRSUN_SI
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform, _prefetch_key

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)


@pytest.mark.parametrize("frame", ["detector", "source"])
def test_device_calls_matches_the_old_spellings(frame):
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW, use_gpu=True,
                               return_list=True, frame=frame)
    rng = np.random.default_rng(20261020)
    rows = rng.uniform(0.1, 3.0, (7, 14)) * ([1e6, 10.0] + [1.0] * 12)
    T, eps = 0.7, 3e-4
    calls, scales = gen.device_calls(rows, T, eps)
    assert len(calls) == len(scales) == 7
    for prm, call, scale in zip(rows.tolist(), calls, scales):
        M, mu, a, p0, e0, x0, dist, qS, phiS, qK, phiK, Phi_phi0, Phi_theta0, Phi_r0 = prm
        theta, phi, rot = gen._angles(qS, phiS, qK, phiK)
        assert call == (M, mu, p0, e0, theta, phi, dist, Phi_phi0, Phi_r0, T, eps)
        assert all(type(v) is float for v in call)
        assert type(scale) is complex
        assert scale == complex(rot * (mu * MRSUN_SI / (dist * Gpc)))      # submit_batch's
        assert scale == complex(rot) * (mu * MRSUN_SI / (dist * Gpc))      # time_series_batch's
        if frame == "source":
            assert scale.imag == 0.0
    # one row, unshaped
    one, _ = gen.device_calls(rows[0], T, eps)
    assert one == calls[:1]


def test_prefetch_key_is_prepares_key():
    c = (np.float64(1e6), 10, 9.5, 0.35, 0.4, -1.5, 1.0, 0.2, 0.3, 2.0, 1e-2)
    M, mu, p0, e0, theta, phi, dist, Phi_phi0, Phi_r0, T, eps = c
    for minus_m in (True, False):
        old = (float(M), float(mu), float(p0), float(e0), float(theta), float(phi), float(dist),
               float(Phi_phi0), float(Phi_r0), float(T), float(eps), bool(minus_m))
        assert _prefetch_key(c, minus_m) == old
        assert all(type(v) is float for v in _prefetch_key(c, minus_m)[:11])
    assert _prefetch_key(c) == tuple(float(v) for v in c[:11]) + (True,)
    assert _prefetch_key(c + ("extra",)) == _prefetch_key(c)
