"""mode_by_mode.setup / study.run on the device against the per-call route of the reference's
driver (check_mode_by_mode.py:246-326) written out here: get_fd_waveform_fromFD and
get_fd_waveform_fromTD __call__ per window and source, then diagnostic.inner_product in the
driver's sequence (SNR :292, mismatch :299, logl :313-317). Shape: the TD route tests' source
(tests/test_gpu_td_likelihood.py: N = 31,559, dt = 20 s, eps = 1e-2), 3 sources, the driver's
four windowings.

Bounds, with delta = ||a - a'|| + ||b - b'|| the measured (noise-weighted) distance between the
two routes' FD templates a and TD templates b, printed below:
  SNR       1e-9 relative, the project's TD parity bound;
  loglike   sqrt(dd') delta + delta^2 / 2 (Cauchy-Schwarz on -1/2 ||a - b||^2) plus 1e-12 of
            2 (aa + bb), the inner-product tolerance;
  mismatch  that bound divided by SNR^2, plus 1e-12.
A source the upstream refuses, in the middle of the batch, comes back NaN and listed in failed,
its neighbours bitwise unchanged; group sizes 2 and 3 give bitwise the same numbers (at this
grid length the windowed FD templates take the exact transform pair)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import diagnostic, mode_by_mode  # noqa: E402
from emri_frequencydomainwaveforms_amd.fdutils import (  # noqa: E402
    get_fd_waveform_fromFD, get_fd_waveform_fromTD, get_sensitivity)
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402

M, MU, E0, DT, T, EPS = 3e5, 10.0, 0.3, 20.0, 0.02, 1e-2
KEYS = ("SNR", "mismatch", "loglike", "snr_td", "overlap")


def _sources():
    p0 = get_p_at_t(EMRIInspiral(), 0.99 * T, [M, MU, 0.0, E0, 1.0])
    truth = np.array([M, MU, 0.0, p0, E0, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4])
    rng = np.random.default_rng(1)
    s = np.tile(truth, (3, 1))
    s[:, 0] *= 1.0 + 1e-4 * rng.normal(size=3)        # M
    s[:, 4] += 1e-4 * rng.normal(size=3)              # e0
    s[:, 11] += 0.1 * rng.normal(size=3)              # Phi_phi0
    s[:, 13] += 0.1 * rng.normal(size=3)              # Phi_r0
    return s


def _templates(study, count):
    """The study's own templates of its last (single) group: a as stored, b split from the kept
    transform; [count][W][2][nb] each."""
    W = len(study.windows)
    a = study._buf["a"][:count * W].clone()
    b = torch.empty_like(a)
    study._tdm._split(study._buf["Z"][:count * W], b)
    torch.cuda.synchronize()
    return a.view(count, W, 2, -1), b.view(count, W, 2, -1)


@pytest.fixture(scope="module")
def case():
    study = mode_by_mode.setup(T, DT, EPS)
    assert study.windows == ("none", "blackman", "hann", "nuttall")
    assert study.N % 2 == 1 and 30000 < study.N < 33000
    params = _sources()
    res = study.run(params)
    a, b = _templates(study, 3)
    return dict(study=study, params=params, res=res, a=a, b=b)


def _norm(x, w):
    return float(torch.sqrt(4.0 * (w * x.abs() ** 2).sum()))


def _check_against_per_call_route(study, params, res, a, b):
    import scipy.signal.windows as sw
    B, W = len(params), len(study.windows)
    assert len(res["failed"]) == 0
    for k in KEYS:
        assert res[k].shape == (B, W) and np.all(np.isfinite(res[k])), k
    pos = study.frequency >= 0.0
    f_pos = study.frequency[pos]
    ipk = dict(PSD=get_sensitivity(f_pos), f_arr=f_pos)
    kw = dict(T=study.Tobs, dt=study.dt, eps=study.eps)
    few = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                               sum_kwargs=dict(pad_output=True, output_type="fd", odd_len=True),
                               use_gpu=True, return_list=True)
    td = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                              sum_kwargs=dict(pad_output=True, odd_len=True), use_gpu=True,
                              return_list=True)
    for j, name in enumerate(study.windows):
        win = None if name == "none" else getattr(sw, name)(study.N)
        fd_t = get_fd_waveform_fromFD(few, pos, study.dt, window=win)
        td_t = get_fd_waveform_fromTD(td, pos, study.dt, window=win)
        for i, p in enumerate(params):
            sig_fd, sig_td = fd_t(*p, **kw), td_t(*p, **kw)
            snr = np.sqrt(float(diagnostic.inner_product(sig_fd, sig_fd, **ipk)))
            bb = float(diagnostic.inner_product(sig_td, sig_td, **ipk))
            mism = abs(1 - diagnostic.inner_product(sig_fd, sig_td, normalize=True, **ipk))
            inner = [sig_fd[0] - sig_td[0], sig_fd[1] - sig_td[1]]
            dd = sum(diagnostic.inner_product(el, el, normalize=False, **ipk) for el in inner)
            logl = -0.5 * dd
            delta = (_norm(torch.stack(sig_fd) - a[i, j], study.w)
                     + _norm(torch.stack(sig_td) - b[i, j], study.w))
            b_ll = np.sqrt(dd) * delta + 0.5 * delta ** 2 + 1e-12 * 2.0 * (snr ** 2 + bb)
            b_mm = b_ll / snr ** 2 + 1e-12
            print(f"{name} source {i}: SNR {snr:.6e} rel err {abs(res['SNR'][i, j] / snr - 1):.2e}"
                  f"; delta / SNR {delta / snr:.2e}; logl {logl:.6e} err "
                  f"{abs(res['loglike'][i, j] - logl):.2e} bound {b_ll:.2e}; mismatch {mism:.6e} "
                  f"err {abs(res['mismatch'][i, j] - mism):.2e} bound {b_mm:.2e}")
            assert abs(res["SNR"][i, j] - snr) <= 1e-9 * snr
            assert abs(res["loglike"][i, j] - logl) <= b_ll
            assert abs(res["mismatch"][i, j] - mism) <= b_mm
            assert abs(res["snr_td"][i, j] - np.sqrt(bb)) <= 1e-9 * np.sqrt(bb)
            assert abs(abs(1 - res["overlap"][i, j].real) - res["mismatch"][i, j]) == 0.0


def test_run_matches_the_per_call_route(case):
    res = case["res"]
    _check_against_per_call_route(case["study"], case["params"], res, case["a"], case["b"])
    # the windows change the numbers, and the sources differ
    assert len(set(res["SNR"][0])) == 4 and len(set(res["SNR"][:, 0])) == 3


def test_invalid_source_is_nan_and_listed(case):
    study, params, res = case["study"], case["params"], case["res"]
    bad = np.insert(params, 1, params[1], axis=0)
    bad[1, 3] = 5.0                      # p0 inside the separatrix: the upstream refuses it
    out = study.run(bad)
    assert list(out["failed"]) == [1]
    for k in KEYS:
        assert np.all(np.isnan(out[k][1])), k
        assert np.array_equal(out[k][[0, 2, 3]], res[k]), k
    again = study.run(params)            # and the study still runs
    for k in KEYS:
        assert np.array_equal(again[k], res[k]), k


def test_group_size_does_not_change_the_numbers(case):
    params, res = case["params"], case["res"]
    for group in (2, 3):
        study = mode_by_mode.setup(T, DT, EPS, group=group)
        out = study.run(params)
        assert len(out["failed"]) == 0
        for k in KEYS:
            assert np.array_equal(out[k], res[k]), (group, k)


def test_drop_static_and_window_choice(case):
    params, res = case["params"], case["res"]
    study = mode_by_mode.setup(T, DT, EPS, windows=("hann", "none"), drop_static=True)
    out = study.run(params[:1])
    assert out["SNR"].shape == (1, 2) and np.all(np.isfinite(out["mismatch"]))
    # no (l, 0, 0) harmonic reaches either sum
    for gen in (study.fd, study.td):
        theta, phi, _ = gen._angles(*params[0, 7:11])
        d = gen.waveform_generator.prepare(params[0, 0], params[0, 1], params[0, 3], params[0, 4],
                                           theta, phi, params[0, 6], params[0, 11],
                                           params[0, 13], T, EPS)
        assert len(d["m"]) > 0 and not np.any((d["m"] == 0) & (d["n"] == 0))
        assert d["teuk"].shape[1] == len(d["m"]) and len(d["ylms"]) == 2 * len(d["m"])
    toy = dict(m=np.array([0, 1, 0, 2]), n=np.array([0, 0, 1, 0]), t=np.zeros(3),
               teuk=np.arange(12.0).reshape(3, 4), ylms=np.arange(8.0), _src=b"", _shape=b"")
    kept = mode_by_mode._without_static(toy)
    assert list(kept["m"]) == [1, 0, 2] and list(kept["n"]) == [0, 1, 0]
    assert np.array_equal(kept["teuk"], toy["teuk"][:, 1:]) and "_src" not in kept
    assert list(kept["ylms"]) == [1.0, 2.0, 3.0, 5.0, 6.0, 7.0]
    print("drop_static: SNR", out["SNR"][0], "mismatch", out["mismatch"][0], "with the static "
          "harmonics:", res["SNR"][0, [2, 0]], res["mismatch"][0, [2, 0]])
    fixed = study.fixed_inspiral(params, T)
    assert np.allclose(fixed[:, 3], [get_p_at_t(EMRIInspiral(), 0.99 * T,
                                                [p[0], p[1], 0.0, p[4], 1.0]) for p in params],
                       rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        mode_by_mode.setup(T, DT, EPS, windows=("not_a_window",))


def test_first_order_windows_on_a_long_grid():
    """N = 2,953,125 = 3^3 5^6 7 (0.936 yr at 10 s; a length whose transform plans are quick to
    make): blackman is past its first-order length (N >= 2,863,565) and takes the shared
    correction transform and efd_cosw_polarizations, where the grids above take the exact
    transform pair. One source and that one window, the same bounds."""
    from emri_frequencydomainwaveforms_amd.constants import YRSID_SI
    Tl = (2953125 - 0.5) * 10.0 / YRSID_SI
    study = mode_by_mode.setup(Tl, 10.0, EPS, windows=("blackman",))
    assert study.N == 2953125 and study._coef[0] is not None and study._exact == []
    p0 = get_p_at_t(EMRIInspiral(), 0.99 * Tl, [1e6, 10.0, 0.0, 0.35, 1.0])
    params = np.array([[1e6, 10.0, 0.0, p0, 0.35, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4]])
    res = study.run(params)
    a, b = _templates(study, 1)
    _check_against_per_call_route(study, params, res, a, b)
