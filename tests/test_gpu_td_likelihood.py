"""The batched TD-template route on the device: efd_td_modesum_windowed, efd_td_split,
efd_td_split_loglike, get_fd_waveform_fromTD.fill_batch / loglike_batch, Likelihood.get_ll over a
get_fd_waveform_fromTD, and pe.setup(template="td").

Bounds.
  kernels   device against the CPU twins: the split within 4 ulp of gain (|Z[k]| + |Z[n-k]|) per
            component, the logL within 1e-12 of 2 sum(|d|^2 + |h w|^2) (tests/test_td_split_cpu.py);
            two runs of the logL are bitwise equal.
  routes    fill_batch against each walker's own __call__ (the reference's route: two transforms,
            fftshift, mask): 1e-9 max|ref| per channel, the project's TD parity bound (RTOL of
            tests/test_gpu_td.py). Both are FP64 transforms of the same series; the measured
            distance is printed.
  logL      |dlogL| <= 2 (2 ||r|| ||delta|| + ||delta||^2) + 1e-12 * 2 (||d||^2 + ||h w||^2) with
            r = d - h_exact w and delta = (h_batch - h_exact) w measured from __call__ and
            fill_batch: Cauchy-Schwarz on the measured distance (tests/test_gpu_pe_configs.py).
"""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib, pe  # noqa: E402
from emri_frequencydomainwaveforms_amd.fdutils import (  # noqa: E402
    get_fd_waveform_fromTD, get_sensitivity)
from emri_frequencydomainwaveforms_amd.likelihood import Likelihood  # noqa: E402
from emri_frequencydomainwaveforms_amd.summation import (  # noqa: E402
    DeviceInputs, TDEngine, td_length)
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402
from tests import td_template_ref as tr  # noqa: E402
from tests.helpers import source_inputs  # noqa: E402

GAIN = 20.0
RTOL = 1e-9


# ---- kernels against the CPU twins ---------------------------------------------------------
def _dev(x):
    return torch.as_tensor(x, device="cuda")


def _split_gpu(buf, n, gain, keep=None):
    lib = _lib.load()
    rows, stride = buf.shape
    nb = (n + 1) // 2
    Z = _dev(buf)
    out = torch.full((rows, 2 * nb + 3), 7.0 + 7.0j, dtype=torch.complex128, device="cuda")
    k8 = None if keep is None else _dev(np.ascontiguousarray(keep, dtype=np.uint8))
    _lib.check(lib.efd_td_split(torch.view_as_real(Z).data_ptr(), stride, n, rows, gain,
                                None if k8 is None else k8.data_ptr(),
                                torch.view_as_real(out).data_ptr(), 2 * nb + 3, None),
               "efd_td_split", lib)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[:, 2 * nb:] == 7.0 + 7.0j)
    return out[:, :2 * nb].reshape(rows, 2, nb)


def _split_loglike_gpu(buf, n, gain, d, w):
    lib = _lib.load()
    rows, stride = buf.shape
    Z, dd, ww = _dev(buf), _dev(np.ascontiguousarray(d)), _dev(np.ascontiguousarray(w))
    out = torch.zeros(rows, dtype=torch.float64, device="cuda")
    scr = torch.empty(rows * _lib.EFD_TD_SPLIT_SCRATCH, dtype=torch.float64, device="cuda")
    _lib.check(lib.efd_td_split_loglike(torch.view_as_real(Z).data_ptr(), stride, n, rows, gain,
                                        torch.view_as_real(dd).data_ptr(), ww.data_ptr(),
                                        out.data_ptr(), scr.data_ptr(), None),
               "efd_td_split_loglike", lib)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", tr.CASES_N)
def test_split_kernel_matches_twin(n, rows):
    Z = np.fft.fft(tr.series(rows, n, seed=n + rows), axis=-1)
    nb = (n + 1) // 2
    buf = tr.strided(Z, n + 5)
    bound = 4.0 * tr.EPS * tr.pair_magnitude(Z, GAIN)[:, None, :]
    keep = np.ones(nb, dtype=np.uint8)
    keep[::3] = 0
    for kp in (None, keep):
        got = _split_gpu(buf, n, GAIN, keep=kp)
        ref = tr.split_cpu(buf, n, GAIN, keep=kp)
        err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
        assert np.all(err <= bound)
        if kp is not None:
            assert np.all(got[:, :, kp == 0] == 0.0)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", tr.CASES_N)
def test_split_loglike_kernel_matches_twin(n, rows):
    h = tr.series(rows, n, seed=7 * n + rows)
    Z = np.fft.fft(h, axis=-1)
    d, w = tr.data_and_weights((n + 1) // 2, seed=n)
    w[:, ::5] = 0.0
    buf = tr.strided(Z, n + 9)
    got = _split_loglike_gpu(buf, n, GAIN, d, w)
    again = _split_loglike_gpu(buf, n, GAIN, d, w)
    assert np.array_equal(got, again)                      # bitwise reproducible
    ref = tr.split_loglike_cpu(buf, n, GAIN, d, w)
    chans = tr.channels_from_series(h, GAIN)
    for r in range(rows):
        scale = tr.loglike_scale(d, chans[r], w)
        print(f"n={n} row {r}: |gpu - twin| / scale {abs(got[r] - ref[r]) / scale:.3e}")
        assert abs(got[r] - ref[r]) <= 1e-12 * scale
        assert abs(got[r] - tr.loglike(d, chans[r], w)) <= 1e-12 * scale


def test_split_loglike_multiblock_and_nan():
    """A length that takes several workgroups per row (the twins' cases take one or a few), and
    a NaN anywhere in a row, the even length's Nyquist bin included, makes that row NaN."""
    for n in (300001, 40000):
        h = tr.series(3, n, seed=n)
        Z = np.fft.fft(h, axis=-1)
        d, w = tr.data_and_weights((n + 1) // 2, seed=5)
        buf = tr.strided(Z, n + 1)
        got = _split_loglike_gpu(buf, n, GAIN, d, w)
        ref = tr.split_loglike_cpu(buf, n, GAIN, d, w)
        chans = tr.channels_from_series(h, GAIN)
        for r in range(3):
            assert abs(got[r] - ref[r]) <= 1e-12 * tr.loglike_scale(d, chans[r], w)
        for where in (0, n // 2, n - 1):
            Zn = Z.copy()
            Zn[1, where] = np.nan
            bad = _split_loglike_gpu(tr.strided(Zn, n + 1), n, GAIN, d, w)
            assert np.isnan(bad[1]) and bad[0] == got[0] and bad[2] == got[2], (n, where)


# ---- the windowed TD sum ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def multimode():
    return source_inputs(M=3e5, mu=10.0, e0=0.35, T=0.02, dt=20.0, eps=1e-2)


def _inp(d):
    return DeviceInputs.from_host(d["t"], np.asarray(d["amp"]).T, d["phi_phi"], d["phi_r"],
                                  d["f_phi"], d["f_r"], d["m"], d["n"], d["ylm_p"], d["ylm_m"])


def test_windowed_entry_with_null_window_is_the_plain_sum(multimode):
    d = multimode
    ns = len(d["freq"]) + 777
    inp, eng = _inp(d), TDEngine()
    sc = d["prefactor"]
    a = torch.empty(ns, dtype=torch.complex128, device="cuda")
    b = torch.full_like(a, 3.0)
    eng.launch(inp, d["dt"], ns, out=torch.view_as_real(a), scale=sc)
    ws = eng._workspace(inp.nt, inp.K, a.device)
    args = _lib.TdArgs(
        t=inp.t.data_ptr(), phi_phi=inp.phi_phi.data_ptr(), phi_r=inp.phi_r.data_ptr(),
        f_phi=inp.f_phi.data_ptr(), f_r=inp.f_r.data_ptr(), nt=inp.nt, amp=inp.amp.data_ptr(),
        m=inp.m.data_ptr(), n=inp.n.data_ptr(), ylm_p=inp.ylm_p.data_ptr(),
        ylm_m=inp.ylm_m.data_ptr(), K=inp.K, dt=float(d["dt"]), nsamples=ns,
        scale_re=float(np.real(sc)), scale_im=float(np.imag(sc)), accumulate=0,
        out=torch.view_as_real(b).data_ptr(), hp=None, hc=None, prof_begin=None, prof_end=None)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(eng.lib.efd_td_modesum_windowed(ctypes.byref(args), None, ws.data_ptr(),
                                               ws.numel(), st), "efd_td_modesum_windowed",
               eng.lib)
    assert eng.status()
    assert torch.equal(a, b) and bool((a != 0).any())


def test_windowed_sum_multiplies_every_output(multimode):
    from scipy.signal.windows import hann
    d = multimode
    ns = len(d["freq"]) + 777   # a ragged last block
    inp, eng = _inp(d), TDEngine()
    sc = 0.7 - 0.4j
    win = torch.as_tensor(hann(ns), device="cuda")

    def run(window, accumulate=False, into=None):
        h, hp, hc = into or (torch.empty(ns, dtype=torch.complex128, device="cuda"),
                             torch.empty(ns, dtype=torch.float64, device="cuda"),
                             torch.empty(ns, dtype=torch.float64, device="cuda"))
        eng.launch(inp, d["dt"], ns, out=torch.view_as_real(h), hp=hp, hc=hc, scale=sc,
                   window=window, accumulate=accumulate)
        assert eng.status()
        return h, hp, hc
    h, hp, hc = run(None)
    hw, hpw, hcw = run(win)
    # multiplications only: nothing can contract
    assert torch.equal(torch.view_as_real(hw), torch.view_as_real(h) * win[:, None])
    assert torch.equal(hpw, hp * win) and torch.equal(hcw, hc * win)
    assert bool((hw != 0).any())
    first = hw.clone(), hpw.clone(), hcw.clone()
    hw2, hpw2, hcw2 = run(win, accumulate=True, into=(hw, hpw, hcw))
    assert torch.equal(hw2, 2 * first[0]) and torch.equal(hpw2, 2 * first[1])
    assert torch.equal(hcw2, 2 * first[2])
    with pytest.raises(ValueError):
        eng.launch(inp, d["dt"], ns, out=torch.view_as_real(h), scale=sc, window=win[:-1])


# ---- routes: fill_batch against __call__ --------------------------------------------------------
M, MU, E0, DT = 3e5, 10.0, 0.3, 20.0


def _source(T):
    p0 = get_p_at_t(EMRIInspiral(), 0.99 * T, [M, MU, 0.0, E0, 1.0])
    return np.array([M, MU, 0.0, p0, E0, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4])


def _walkers(truth, count, seed=1):
    rng = np.random.default_rng(seed)
    w = np.tile(truth, (count, 1))
    w[:, 0] *= 1.0 + 1e-4 * rng.normal(size=count)       # M
    w[:, 4] += 1e-4 * rng.normal(size=count)             # e0
    w[:, 11] += 0.1 * rng.normal(size=count)             # Phi_phi0
    w[:, 13] += 0.1 * rng.normal(size=count)             # Phi_r0
    return w


@pytest.fixture(scope="module", params=["odd", "even"])
def grid(request):
    """The test_td_generator_api source (N = 31,559, odd), and an even-length generator."""
    odd = request.param == "odd"
    T = 0.02 if odd else 0.02001
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                               sum_kwargs=dict(pad_output=True, odd_len=odd), use_gpu=True,
                               return_list=True)
    n = td_length(T, DT, odd)
    assert n % 2 == (1 if odd else 0) and 30000 < n < 33000
    freq = np.fft.fftshift(np.fft.fftfreq(n, DT))
    mask = torch.as_tensor(freq >= 0.0, device="cuda")
    truth = _source(T)
    return dict(gen=gen, n=n, mask=mask, freq=freq[freq >= 0.0], truth=truth,
                walkers=_walkers(truth, 3), kw=dict(T=T, dt=DT, eps=1e-2))


def _window(name, n):
    import scipy.signal.windows as sw
    return {"none": None, "hann": sw.hann(n), "tukey": sw.tukey(n, 0.1)}[name]


@pytest.mark.parametrize("window", ["none", "hann", "tukey"])
def test_fill_batch_matches_call(grid, window):
    g = grid
    nb = (g["n"] + 1) // 2
    tm = get_fd_waveform_fromTD(g["gen"], g["mask"], DT, window=_window(window, g["n"]))
    assert tm.batched and tm.can_fill and tm.can_fill_batch and tm.num_bins == nb
    outs = torch.empty((3, 2, nb), dtype=torch.complex128, device="cuda")
    tm.fill_batch(outs, g["walkers"], **g["kw"])
    one = torch.empty((2, nb), dtype=torch.complex128, device="cuda")
    tm.fill(one, *g["walkers"][1], **g["kw"])
    assert tm.info["transform"] in ("hipfft", "torch.fft")
    worst = 0.0
    for i, p in enumerate(g["walkers"]):
        ref = torch.stack(tm(*p, **g["kw"]))
        assert bool((ref != 0).any())
        for c in range(2):
            scale = float(ref[c].abs().max())
            err = float((outs[i, c] - ref[c]).abs().max()) / scale
            worst = max(worst, err)
            assert err <= RTOL, (i, c, err)
            if i == 1:
                assert float((one[c] - ref[c]).abs().max()) <= RTOL * scale
    print(f"n={g['n']} window={window} transform={tm.info['transform']}: "
          f"max |fill_batch - __call__| / max|ref| = {worst:.3e}")
    # distinct walkers gave distinct templates
    assert float((outs[0] - outs[1]).abs().max()) > 1e-3 * float(outs[0].abs().max())


def test_fill_batch_non_zero_mask_and_list_outputs(grid):
    g = grid
    nb = (g["n"] + 1) // 2
    nz = (torch.arange(nb, device="cuda") % 7) != 0
    tm = get_fd_waveform_fromTD(g["gen"], g["mask"], DT, non_zero_mask=nz)
    full = get_fd_waveform_fromTD(g["gen"], g["mask"], DT)
    outs = [torch.empty((2, nb), dtype=torch.complex128, device="cuda") for _ in range(3)]
    tm.WINDOW_GROUP = 2   # one full group and one ragged group
    tm.fill_batch(outs, g["walkers"], **g["kw"])
    ref = torch.empty((3, 2, nb), dtype=torch.complex128, device="cuda")
    full.fill_batch(ref, g["walkers"], **g["kw"])
    for i in range(3):
        assert bool((outs[i][:, ~nz] == 0).all())
        assert float((outs[i][:, nz] - ref[i][:, nz]).abs().max()) <= \
            RTOL * float(ref[i].abs().max())
        call = torch.stack(tm(*g["walkers"][i], **g["kw"]))
        assert bool((call[:, ~nz] == 0).all())
        assert float((outs[i] - call).abs().max()) <= RTOL * float(call.abs().max())


def test_other_cases_keep_the_old_route(grid, monkeypatch):
    g = grid
    tm = get_fd_waveform_fromTD(g["gen"], g["mask"], DT)
    tm.batched = False
    assert not tm.can_fill and not tm.can_fill_batch
    shifted = torch.roll(g["mask"], 1)
    assert not get_fd_waveform_fromTD(g["gen"], shifted, DT).can_fill
    assert not get_fd_waveform_fromTD(lambda *a, **k: None, g["mask"], DT).can_fill_batch
    fd = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                              sum_kwargs=dict(pad_output=True, output_type="fd", odd_len=True),
                              use_gpu=True, return_list=True)
    assert not get_fd_waveform_fromTD(fd, g["mask"], DT).can_fill
    monkeypatch.setenv("EFD_TD_BATCH", "0")
    assert not get_fd_waveform_fromTD(g["gen"], g["mask"], DT).can_fill_batch


# ---- Likelihood -----------------------------------------------------------------------------
def _norm(x):
    return float(torch.sqrt((x.abs() ** 2).sum()))


@pytest.mark.parametrize("window", ["none", "tukey"])
def test_likelihood_batched_against_per_walker(grid, window):
    g = grid
    nb = (g["n"] + 1) // 2
    tm = get_fd_waveform_fromTD(g["gen"], g["mask"], DT, window=_window(window, g["n"]))
    tm.WINDOW_GROUP = 3   # 6 walkers below: one full group and ... a ragged one of 5 + truth
    like = Likelihood(tm, 2, f_arr=g["freq"], use_gpu=True)
    like.inject_signal(params=g["truth"].copy(), waveform_kwargs=g["kw"],
                       noise_fn=get_sensitivity)
    walkers = np.vstack([_walkers(g["truth"], 5, seed=3)[:4], g["truth"][None, :]])
    assert len(walkers) == 5                               # groups of 3 and 2
    ll_b = like.get_ll(walkers, **g["kw"])
    assert tm.info.get("transform") in ("hipfft", "torch.fft")
    ll_b2 = like.get_ll(walkers, **g["kw"])
    assert np.array_equal(ll_b, ll_b2)
    tm.batched = False
    ll_e = like.get_ll(walkers, **g["kw"])
    tm.batched = True
    hb = torch.empty((5, 2, nb), dtype=torch.complex128, device="cuda")
    tm.fill_batch(hb, walkers, **g["kw"])
    d, w = like._d, like._w
    nd2 = _norm(d) ** 2
    assert np.all(np.isfinite(ll_b)) and np.all(np.isfinite(ll_e))
    for i, p in enumerate(walkers):
        he = torch.stack(tm(*p, **g["kw"]))
        r, delta = _norm(d - he * w), _norm((hb[i] - he) * w)
        bound = 2.0 * (2.0 * r * delta + delta ** 2) + 1e-12 * 2.0 * (nd2 + _norm(he * w) ** 2)
        print(f"n={g['n']} window={window} walker {i}: logL {ll_e[i]:.6e} |dlogL| "
              f"{abs(ll_b[i] - ll_e[i]):.3e} bound {bound:.3e} ||delta||/||hw|| "
              f"{delta / _norm(he * w):.3e}")
        assert abs(ll_b[i] - ll_e[i]) <= bound, (i, ll_b[i], ll_e[i], bound)
    # the injection's own parameters: r = 0 on the per-walker route
    assert ll_e[4] == 0.0
    assert ll_e[0] < -1e-6 * nd2                           # the other walkers are off the truth


def test_invalid_walker_is_an_error_or_nan(grid):
    g = grid
    tm = get_fd_waveform_fromTD(g["gen"], g["mask"], DT)
    like = Likelihood(tm, 2, f_arr=g["freq"], use_gpu=True)
    like.inject_signal(params=g["truth"].copy(), waveform_kwargs=g["kw"],
                       noise_fn=get_sensitivity)
    bad = _walkers(g["truth"], 3, seed=4)
    bad[1, 3] = 5.0            # p0 inside the separatrix: the upstream refuses it
    with pytest.raises(_lib.EFDError):
        like.get_ll(bad, **g["kw"])
    torch.cuda.synchronize()
    nan = _walkers(g["truth"], 3, seed=4)
    nan[1, 6] = np.nan         # a NaN distance: every sample of the walker's series is NaN
    ll = like.get_ll(nan, **g["kw"])
    assert np.isnan(ll[1]) and np.isfinite(ll[0]) and np.isfinite(ll[2])
    ok = like.get_ll(_walkers(g["truth"], 3, seed=4), **g["kw"])
    assert ok[0] == ll[0] and ok[2] == ll[2] and np.isfinite(ok[1])


def test_dt_only_likelihood_still_raises(grid):
    g = grid
    like = Likelihood(get_fd_waveform_fromTD(g["gen"], g["mask"], DT), 2, dt=DT, use_gpu=True)
    with pytest.raises(NotImplementedError):
        like.get_ll(g["walkers"], **g["kw"])


# ---- pe.setup(template="td") ------------------------------------------------------------------
SETUP = dict(Tobs=0.02, dt=20.0, M=3e5, nwalkers=4, freeze_gc=False)


def test_pe_setup_td_half_step():
    s = pe.setup(template="td", **SETUP)
    assert isinstance(s.gen, get_fd_waveform_fromTD) and s.gen.can_fill_batch
    assert s.info["template"] == "td" and s.info["injectFD"] is False
    assert s.few.waveform_generator.output_type == "td" and s.half_step == 2
    ll = s.like(s.half_steps()[0], **s.kwargs)
    assert ll.shape == (2,) and np.all(np.isfinite(ll)) and np.all(ll <= 0.0)
    at_truth = s.like(s.truth6[None, :], **s.kwargs)[0]
    assert np.isfinite(at_truth) and abs(at_truth) <= 1e-12 * 2.0 * float(
        (s.like._d.abs() ** 2).sum())


def test_pe_setup_td_template_fd_injection_and_windows():
    from scipy.signal.windows import tukey
    s = pe.setup(template="td", injectFD=True, **SETUP)
    assert s.info["injectFD"] is True
    at_truth = s.like(s.truth6[None, :], **s.kwargs)[0]
    assert np.isfinite(at_truth) and at_truth < 0.0       # the FD and TD models differ
    n = s.info["N_f"]
    sw = pe.setup(template="td", window=tukey(n, 0.1), **SETUP)
    assert sw.info["window"] == "array" and sw.gen.can_fill_batch
    assert np.all(np.isfinite(sw.like(sw.half_steps()[0], **sw.kwargs)))
    assert pe.setup(template="td", window="hann", **SETUP).info["window"] == "hann"
    with pytest.raises(ValueError):
        pe.setup(template="td", window=np.ones(n - 1), **SETUP)
    with pytest.raises(ValueError):
        pe.setup(template="fd", window=np.ones(n), **SETUP)


def test_pe_setup_fd_unchanged_by_the_new_arguments():
    a = pe.setup(**SETUP)
    b = pe.setup(template="fd", injectFD=None, **SETUP)
    assert np.array_equal(a.start, b.start)
    la = a.like(a.half_steps()[0], **a.kwargs)
    lb = b.like(b.half_steps()[0], **b.kwargs)
    assert np.array_equal(la, lb) and np.all(np.isfinite(la))
    assert torch.equal(a.like._d, b.like._d)
    # the driver's other cross-model run: an FD template on TD data
    c = pe.setup(template="fd", injectFD=False, **SETUP)
    at_truth = c.like(c.truth6[None, :], **c.kwargs)[0]
    assert np.isfinite(at_truth) and at_truth < 0.0
