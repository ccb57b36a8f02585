"""ModeByModeStudy.fixed_inspiral(params, device=True): every drawn source's p0 root solve at
once on the device (trajectory.get_p_at_t_batch) against the default, one host solve after the
other. p0 agrees to 1e-13 p0, the tolerance tests/test_native_upstream.py holds native against
scipy to; a source the search refuses keeps its p0, as today. STAND-IN PHYSICS, NOT FEW."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import mode_by_mode  # noqa: E402

DT, T, EPS = 20.0, 0.02, 1e-2     # tests/test_gpu_mode_by_mode.py's grid


def test_fixed_inspiral_device_matches_host():
    study = mode_by_mode.setup(T, DT, EPS)
    rng = np.random.default_rng(7)
    params = np.tile(np.array([3e5, 10.0, 0.0, 12.0, 0.3, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0,
                               0.4]), (5, 1))
    params[:, 0] *= 1.0 + 0.05 * rng.uniform(-1, 1, size=5)       # M
    params[:, 1] *= 1.0 + 0.05 * rng.uniform(-1, 1, size=5)       # mu
    params[:, 4] += 0.05 * rng.uniform(-1, 1, size=5)             # e0
    # row 2: so light a secondary that the plunge from the separatrix buffer takes longer than
    # 0.99 T: the search is refused
    params[2, 1] = 1e-9
    params[2, 3] = 11.5
    before = params.copy()
    host = study.fixed_inspiral(params)
    dev = study.fixed_inspiral(params, device=True)
    np.testing.assert_array_equal(params, before)
    assert host.shape == dev.shape == (5, 14)
    cols = [c for c in range(14) if c != 3]
    np.testing.assert_array_equal(dev[:, cols], params[:, cols])
    np.testing.assert_array_equal(host[:, cols], params[:, cols])
    assert host[2, 3] == 11.5 and dev[2, 3] == 11.5                # refused: p0 kept
    for i in (0, 1, 3, 4):
        rel = abs(dev[i, 3] - host[i, 3]) / host[i, 3]
        print(f"source {i}: p0 device {dev[i, 3]:.17g} host {host[i, 3]:.17g} rel {rel:.3g}")
        assert host[i, 3] != 12.0 and rel <= 1e-13
    # Tobs given explicitly, as the default
    np.testing.assert_array_equal(study.fixed_inspiral(params, T, device=True), dev)
