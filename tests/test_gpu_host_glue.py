"""The batched host glue's shared pieces on the device: the host route over rotating groups
(generate_batch, spectrum_batch with lane ranges) and the pinned stage regrowing under reuse in
its three users. STAND-IN PHYSICS, NOT FEW.

A row's launches do not depend on the group it falls in, nor a source's on the staging buffer its
inputs went through, so everything here is bitwise. Public API only.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd.summation import (BatchPreparer, DeviceInputs,  # noqa: E402
                                                         ModeSumEngine, PinnedStage,
                                                         WaveformPipeline, sum_batch)
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402
from tests.helpers import source_inputs  # noqa: E402

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)
M, MU, E0, T, DT, EPS = 1e6, 10.0, 0.35, 0.01, 10.0, 1e-2   # about 3.2e4 bins
KW = dict(T=T, dt=DT, eps=EPS)


def _nan(shape):
    return torch.full(shape, complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")


def _both(gen, rows):
    """generate_batch, then spectrum_batch with lane ranges and check=False: (h, S, lanes,
    lanes_host as read right after lanes_ready())."""
    B = len(rows)
    nf = int(gen.waveform_generator.create_waveform._grid(T, DT, None)[0].numel())
    assert 3.0e4 < nf < 3.4e4
    h = _nan((B, 2, gen.positive_bins(T=T, dt=DT)))
    gen.generate_batch(rows, h, **KW)
    S = _nan((B, nf))
    lanes = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    lanes_host = torch.full((B, 2), -1, dtype=torch.int32).pin_memory()
    gen.spectrum_batch(rows, S, lanes=lanes, lanes_host=lanes_host, check=False, **KW)
    gen.lanes_ready()
    lh = lanes_host.numpy().copy()
    gen.check_batch()
    torch.cuda.synchronize()
    return h.cpu().numpy(), S.cpu().numpy(), lanes.cpu().numpy(), lh


def test_host_route_over_rotating_groups():
    """5 rows in groups of 2 over the preparer's two groups (the third flush reuses the first's
    workspaces, staging and events) against one group of 5, and against a second call."""
    p0 = get_p_at_t(EMRIInspiral(), 0.99 * T, [M, MU, 0.0, E0, 1.0])
    base = np.array([M, MU, 0.0, p0, E0, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4])
    rows = np.repeat(base[None, :], 5, axis=0)
    rows[:, 0] *= [1.0, 1.0 + 2e-4, 1.0 - 3e-4, 1.0 + 1e-4, 1.0 - 1e-4]   # distinct M
    rows[:, 4] += [0.0, 2e-3, -1e-3, 1e-3, -2e-3]                         # distinct e0
    rows[:, 11] = [0.2, 1.7, 4.0, 2.9, 5.5]                               # distinct Phi_phi0
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW,
                               use_gpu=True, return_list=True)
    assert gen.BATCH_GROUP >= 5
    h1, S1, l1, lh1 = _both(gen, rows)
    gen.BATCH_GROUP = 2
    h3, S3, l3, lh3 = _both(gen, rows)
    again = _both(gen, rows)
    assert np.isfinite(h1).all() and np.isfinite(S1).all()
    assert (l1 >= 0).all() and (l1[:, 0] < l1[:, 1]).all()
    assert len({a.tobytes() for a in S1}) == 5          # five different rows
    np.testing.assert_array_equal(lh1, l1)
    for got in ((h3, S3, l3, lh3), again):
        for a, b in zip(got, (h1, S1, l1, l1)):
            np.testing.assert_array_equal(a, b)


KEYS = ("t", "phi_phi", "phi_r", "f_phi", "f_r", "m", "n", "ylm_p", "ylm_m")


def _host(d):
    h = {k: d[k] for k in KEYS}
    h["amp"] = np.ascontiguousarray(d["amp"].T)     # [nt][K]
    return h


def _inputs(d, stage):
    h = _host(d)
    return DeviceInputs.from_host(h["t"], h["amp"], h["phi_phi"], h["phi_r"], h["f_phi"],
                                  h["f_r"], h["m"], h["n"], h["ylm_p"], h["ylm_m"], staging=stage)


@pytest.fixture(scope="module")
def ragged():
    """test_gpu_batch_prepare.py's six ragged sources, smallest inputs first, their grid on the
    device and each one's spectrum from objects of its own (stage, inputs, engine)."""
    srcs = [source_inputs(M=M_, e0=e0, T=0.02, dt=20.0, eps=eps)
            for M_, e0, eps in ((3e5, 0.35, 1e-2), (5e5, 0.2, 1e-3), (2e5, 0.5, 1e-2),
                                (4e5, 0.1, 1e-5), (3e5, 0.6, 1e-2), (6e5, 0.3, 1e-4))]
    srcs.sort(key=lambda d: d["amp"].size)
    sizes = [d["amp"].size for d in srcs]
    assert sizes == sorted(set(sizes)) and 16 * sizes[-1] > 1 << 20   # growth past the first MiB
    freq = torch.as_tensor(srcs[0]["freq"], device="cuda")
    ref = [ModeSumEngine().run(_inputs(d, PinnedStage()), freq, grid_symmetric=True,
                               scale=d["prefactor"]) for d in srcs]
    return srcs, freq, ref


def _outs(srcs, freq):
    return [_nan((int(freq.numel()),)) for _ in srcs]


def test_stage_growth_from_host(ragged):
    """DeviceInputs.from_host through one caller-owned stage, nothing awaited in between."""
    srcs, freq, ref = ragged
    stage, eng, outs = PinnedStage(), ModeSumEngine(), _outs(srcs, freq)
    for d, o in zip(srcs, outs):
        eng.run(_inputs(d, stage), freq, out=o, grid_symmetric=True, scale=d["prefactor"],
                check=False)
    assert eng.status()
    assert all(torch.equal(o, r) for o, r in zip(outs, ref))


def test_stage_growth_pipeline_slot(ragged):
    srcs, freq, ref = ragged
    P, outs = WaveformPipeline(num_slots=1), _outs(srcs, freq)
    for d, o in zip(srcs, outs):
        P.submit(_host(d), freq, True, d["prefactor"], out=torch.view_as_real(o))
    P.wait()
    torch.cuda.synchronize()
    assert all(torch.equal(o, r) for o, r in zip(outs, ref))


def test_stage_growth_batch_preparer(ragged):
    """One group of one walker: every flush reuses the group's stage right behind its last copy;
    the sums run on the group's own stream, which orders the workspace's reuse."""
    srcs, freq, ref = ragged
    B, outs = BatchPreparer(group=1, depth=1), _outs(srcs, freq)
    B.order_after_current()
    for d, o in zip(srcs, outs):
        B.submit(_host(d), freq, True, d["prefactor"], prepare_only=True)
        gi, jobs = B.flush()
        sum_batch([(jobs[0][0], dict(jobs[0][1], out=torch.view_as_real(o)))],
                  stream=B.stream(gi).cuda_stream)
    B.wait()
    torch.cuda.synchronize()
    assert all(torch.equal(o, r) for o, r in zip(outs, ref))
