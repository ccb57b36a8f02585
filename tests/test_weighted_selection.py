"""Noise-weighted mode selection without a GPU: the PSD table's host evaluation
(efd_psd_eval_cpu) against scipy's PPoly, the numpy ModeSelector(sensitivity_fn) against a plain
restatement, and efd_host_modes_weighted against numpy. STAND-IN PHYSICS, NOT FEW.

The native kept set is compared element for element only under the preconditions of
tests/test_gpu_modes_device.py taken on the weighted powers (sum margin >= 1e-11, cut gap >=
1e-9), and a third from scipy alone: the weight of a mode moves by <= 1e-12 relative when its
frequency moves by 4 u, and kappa = M / |S| <= 4, so the native cubic (two roundings per Horner
step) and scipy's agree to ~1e-14: well inside the gap.
"""

import ctypes
import threading

import numpy as np
import pytest
from scipy.interpolate import CubicSpline, PPoly

from emri_frequencydomainwaveforms_amd import _lib, amplitude, fdutils
from emri_frequencydomainwaveforms_amd.amplitude import ModeSelector, RomanAmplitude
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t
from emri_frequencydomainwaveforms_amd.ylm import GetYlms
from tests import weighted_selection_ref as ws

U = ws.U


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# -- the PSD table ----------------------------------------------------------------------------
def test_psd_eval_cpu_matches_ppoly(lib):
    tab = ws.lisa()
    f = ws.psd_points(tab)
    ref = PPoly(tab.c, tab.x, extrapolate=True)(f)
    got = ws.eval_cpu(lib, tab, f)
    bound, M = ws.psd_bound(tab, f)
    err = np.abs(got - ref)
    print(f"efd_psd_eval_cpu: {len(f)} points, max |d| / (u M) = {(err / (U * M)).max():.3g} "
          f"(<= 32), kappa = M/|S| up to {(M / np.abs(ref)).max():.3g}")
    assert np.all(err <= bound)
    np.testing.assert_array_equal(ref, tab(f))     # (the CubicSpline is that PPoly)
    # NaN in, NaN out; the neighbours untouched
    g = ws.eval_cpu(lib, tab, np.array([1e-3, np.nan, 2e-3]))
    assert np.isnan(g[1]) and g[0] == got_at(lib, tab, 1e-3) and np.isfinite(g[2])
    # lower-order tables are cubics with zero leading coefficients: exact
    np.testing.assert_array_equal(ws.eval_cpu(lib, ws.wall(), np.array([1e-3, 4e-3, 0.5, 7.0])),
                                  [1.0, 2.0 ** 120, 2.0 ** 120, 2.0 ** 120])
    np.testing.assert_array_equal(ws.eval_cpu(lib, ws.gentle(), np.array([0.0, 0.5])),
                                  [1.0, 16.0])


def got_at(lib, tab, f):
    return ws.eval_cpu(lib, tab, np.array([f]))[0]


def test_psd_eval_cpu_rejects_bad_arguments(lib):
    st, hold = ws.psd_struct(ws.lisa())
    f = np.array([1e-3])
    out = np.zeros(1)
    call = lambda t, fp=f.ctypes.data, op=out.ctypes.data, nf=1: lib.efd_psd_eval_cpu(  # noqa: E731
        t, fp, nf, op, None)
    assert call(ctypes.byref(st)) == 0
    assert call(None) == _lib.EFD_ERR_ARG
    assert call(ctypes.byref(st), fp=None) == _lib.EFD_ERR_ARG
    assert call(ctypes.byref(st), op=None) == _lib.EFD_ERR_ARG
    assert call(ctypes.byref(st), nf=0) == 0
    for n in (1, 0, 4097):
        bad = _lib.PsdTable(st.x, st.c, n)
        assert call(ctypes.byref(bad)) == _lib.EFD_ERR_ARG, n
    assert call(ctypes.byref(_lib.PsdTable(None, st.c, st.n))) == _lib.EFD_ERR_ARG
    assert call(ctypes.byref(_lib.PsdTable(st.x, None, st.n))) == _lib.EFD_ERR_ARG
    x = hold[0].copy()
    x[5] = x[4]                                    # not strictly ascending
    assert call(ctypes.byref(_lib.PsdTable(x.ctypes.data, st.c, st.n))) == _lib.EFD_ERR_ARG
    x[5] = np.nan
    assert call(ctypes.byref(_lib.PsdTable(x.ctypes.data, st.c, st.n))) == _lib.EFD_ERR_ARG
    # 4096 breakpoints are accepted
    xb = np.linspace(0.0, 1.0, 4096)
    cb = np.ones((4, 4095))
    assert call(ctypes.byref(_lib.PsdTable(xb.ctypes.data, cb.ctypes.data, 4096))) == 0


def test_psd_table_helper():
    t = amplitude.psd_table(fdutils.get_sensitivity)
    sp = fdutils._spline()
    np.testing.assert_array_equal(t.x, sp.x)
    np.testing.assert_array_equal(t.c, sp.c)
    assert t.host.n == len(sp.x) == 600
    cs = CubicSpline([0.0, 1.0, 3.0], [1.0, 2.0, 0.5])
    t = amplitude.psd_table(cs)
    np.testing.assert_array_equal(t.c, cs.c)
    t = amplitude.psd_table(ws.wall())
    assert t.c.shape == (4, 2) and not t.c[:3].any()
    assert amplitude.psd_table(lambda f: 1.0 + f) is None
    assert amplitude.psd_table(PPoly(np.ones((1, 1)), np.array([1.0, 0.0]))) is None   # descending
    assert amplitude.psd_table(PPoly(np.ones((5, 1)), np.array([0.0, 1.0]))) is None   # quartic


# -- numpy's definition against the restatement --------------------------------------------------
def run_numpy(case, fn, eps=None):
    teuk, ylms, m0mask, inds, eps0, fr = case
    return ModeSelector(m0mask, sensitivity_fn=fn)(teuk, ylms, inds,
                                                   eps=eps0 if eps is None else eps,
                                                   mode_freqs=fr)


def run_restated(case, fn):
    teuk, ylms, m0mask, inds, eps, (f_phi, f_r) = case
    W = ws.weights(fn, ws.mode_freq(inds[1], inds[2], f_phi, f_r))
    power, fold = ws.weighted_powers(teuk, ylms, m0mask, W)
    return ws.restated(power, fold, eps), power


@pytest.fixture(scope="module")
def cases():
    return ws.generic_cases()


def test_five_m0_modes(cases):
    c = cases["five_m0_modes"]
    ref, power = run_restated(c, ws.lisa())
    margin, _ = ws.assert_order_independent(power, c[4], "five_m0_modes")
    assert margin >= 1e-3                          # (1.3e-3 when the case was chosen)
    got = run_numpy(c, ws.lisa())
    np.testing.assert_array_equal(got, ref)
    unweighted = ModeSelector(c[2])(c[0], c[1], None, eps=c[4])
    assert len(got) == 3 and len(unweighted) == 4
    # get_sensitivity itself is the same function of f
    np.testing.assert_array_equal(run_numpy(c, fdutils.get_sensitivity), ref)


def test_one_mode(cases):
    c = cases["one_mode"]
    ref, _ = run_restated(c, ws.lisa())
    np.testing.assert_array_equal(run_numpy(c, ws.lisa()), ref)
    np.testing.assert_array_equal(ref, [0])


def test_forty_modes_three_tables(cases):
    c = cases["forty"]
    teuk, ylms, m0mask, inds, eps, (f_phi, f_r) = c
    F = ws.mode_freq(inds[1], inds[2], f_phi, f_r)
    unweighted = ModeSelector(m0mask)(teuk, ylms, None, eps=eps)
    # the wall: weights 1 below 4e-3 Hz, 2^-120 above
    ref, power = run_restated(c, ws.wall())
    ws.assert_order_independent(power, eps, "wall")
    got = run_numpy(c, ws.wall())
    np.testing.assert_array_equal(got, ref)
    never_below = np.nonzero((F >= 4e-3).all(axis=0))[0]
    assert len(never_below) == 6
    assert (F[:, got] < 4e-3).any(axis=0).all()
    assert set(never_below) & set(unweighted) and not set(never_below) & set(got)
    # flat S = 0.25: exact scaling, the unweighted set
    ref, power = run_restated(c, ws.flat())
    ws.assert_order_independent(power, eps, "flat")
    np.testing.assert_array_equal(run_numpy(c, ws.flat()), ref)
    np.testing.assert_array_equal(ref, unweighted)
    # S = -1 from 5e-3 Hz: weight 0 there, as for a callable that returns NaN there
    ref, power = run_restated(c, ws.negative())
    ws.assert_order_independent(power, eps, "negative")
    got = run_numpy(c, ws.negative())
    np.testing.assert_array_equal(got, ref)
    always_there = np.nonzero((F >= 5e-3).all(axis=0))[0]
    assert len(always_there) == 2 and not set(always_there) & set(got)
    nan_there = lambda f: np.where(f >= 5e-3, np.nan, 1.0)   # noqa: E731
    np.testing.assert_array_equal(run_numpy(c, nan_there), got)
    inf_there = lambda f: np.where(f >= 5e-3, np.inf, 1.0)   # noqa: E731
    np.testing.assert_array_equal(run_numpy(c, inf_there), got)


def test_frequency_arguments(cases):
    teuk, ylms, m0mask, inds, eps, _ = cases["forty"]
    from emri_frequencydomainwaveforms_amd.constants import MTSUN_SI
    from emri_frequencydomainwaveforms_amd.frequencies import get_fundamental_frequencies
    M, a, x = 1e6, 0.0, 1.0
    p, e = np.array([9.5, 9.0, 8.5]), np.array([0.3, 0.28, 0.26])
    op, _, orr = get_fundamental_frequencies(a, p, e, x)
    fr = (op / (2 * np.pi * M * MTSUN_SI), orr / (2 * np.pi * M * MTSUN_SI))
    sel = ModeSelector(m0mask, sensitivity_fn=ws.lisa())
    a1 = sel(teuk, ylms, inds, eps=eps, mode_freqs=fr)
    a2 = sel(teuk, ylms, inds, fund_freq_args=(M, a, p, e, x), eps=eps)
    a3 = sel(teuk, ylms, inds, (M, a, p, e, x), eps)             # FEW's positional order
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(a1, a3)
    assert len(a1) > 0
    with pytest.raises(ValueError):
        sel(teuk, ylms, inds, eps=eps)
    with pytest.raises(ValueError):
        sel(teuk, ylms, None, eps=eps, mode_freqs=fr)
    # without a sensitivity_fn the new arguments change nothing
    plain = ModeSelector(m0mask)
    np.testing.assert_array_equal(plain(teuk, ylms, None, eps=eps),
                                  plain(teuk, ylms, inds, eps=eps, mode_freqs=fr))


def test_all_negative_table_keeps_nothing(cases):
    c = cases["forty"]
    got = run_numpy(c, ws.all_negative())
    assert got.size == 0 and run_restated(c, ws.all_negative())[0].size == 0
    wg = bare_generator(ws.all_negative())
    with pytest.raises(ValueError, match="kept no mode"):
        wg.prepare(1e6, 10.0, 9.5, 0.3, 1.0, -np.pi / 2, 1.0, T=0.05, eps=1e-2)


# -- the host C++ against numpy --------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    traj = EMRIInspiral()
    amp = RomanAmplitude()
    src = {}
    for name, (M, mu, e0, T) in (("S1", ws.S1), ("S2", ws.S2)):
        p0 = get_p_at_t(traj, 0.99 * T, [M, mu, 0.0, e0, 1.0])
        t, p, e, _, _, f_phi, f_r = traj.with_frequencies(M, mu, 0.0, p0, e0, 1.0, T=T)
        A = amp(p, e)
        src[name] = (p, e, f_phi, f_r, A)
    ylms = GetYlms(assume_positive_m=True)(amp.l_arr, amp.m_arr, 1.0, -np.pi / 2)
    return amp, src, ylms


def weight_precondition(tab, F):
    """From scipy alone: the relative change of S under a 4 u relative change of F, and kappa."""
    S = tab(F)
    d = max((np.abs(tab(F * (1 + s * 4 * U)) - S) / np.abs(S)).max() for s in (1.0, -1.0))
    kappa = (ws.psd_bound(tab, F)[1] / np.abs(S)).max()
    return d, kappa


@pytest.mark.parametrize("eps", [1e-2, 1e-5])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_host_modes_weighted_matches_numpy(lib, model, name, eps):
    amp, src, ylms = model
    p, e, f_phi, f_r, A = src[name]
    tab = ws.lisa()
    inds = (amp.l_arr, amp.m_arr, amp.n_arr)
    F = ws.mode_freq(amp.m_arr, amp.n_arr, f_phi, f_r)
    d, kappa = weight_precondition(tab, F)
    print(f"{name}: weight response to 4 u in F {d:.3g} (<= 1e-12), kappa {kappa:.3g} (<= 4)")
    assert d <= 1e-12 and kappa <= 4.0
    power, _ = ws.weighted_powers(A, ylms, amp.m0mask, ws.weights(tab, F))
    ws.assert_order_independent(power, eps, f"{name} eps={eps:g}")
    ref = ModeSelector(amp.m0mask, sensitivity_fn=fdutils.get_sensitivity)(
        A, ylms, inds, eps=eps, mode_freqs=(f_phi, f_r))
    unweighted = ModeSelector(amp.m0mask)(A, ylms, None, eps=eps)
    print(f"{name} eps={eps:g}: K unweighted {len(unweighted)} -> weighted {len(ref)}")
    assert set(ref) != set(unweighted)
    psd = amplitude.psd_table(fdutils.get_sensitivity)
    res = []
    try:
        for nth in (1, 4):
            lib.efd_host_set_threads(nth)
            keep, teuk = amp.select(p, e, ylms, eps, lib=lib, f_phi=f_phi, f_r=f_r, psd=psd)
            res.append((keep, teuk))
    finally:
        lib.efd_host_set_threads(_lib.host_threads())
    for keep, teuk in res:
        np.testing.assert_array_equal(keep, ref)
        assert np.abs(teuk - A[:, ref]).max() <= 1e-14 * np.abs(A[:, ref]).max()
        np.testing.assert_array_equal(teuk, res[0][1])
    # the numpy fall-back of select (no library) evaluates the same table
    kn, _ = amp.select(p, e, ylms, eps, f_phi=f_phi, f_r=f_r, psd=psd)
    np.testing.assert_array_equal(kn, ref)
    with pytest.raises(ValueError):
        amp.select(p, e, ylms, eps, lib=lib, psd=psd)


def test_host_modes_weighted_rejects_bad_arguments(lib, model):
    amp, src, ylms = model
    p, e, f_phi, f_r, _ = src["S1"]
    K, nt = amp.num_teuk_modes, len(p)
    psd = amplitude.psd_table(fdutils.get_sensitivity)
    yp = np.ascontiguousarray(ylms[:K])
    ym = np.ascontiguousarray(ylms[K:])
    keep = np.empty(K, dtype=np.int32)
    nkeep = ctypes.c_int32(-1)

    def call(fp, fr, tab):
        return lib.efd_host_modes_weighted(
            p.ctypes.data, e.ctypes.data, nt, amp.l_arr.ctypes.data, amp.m_arr.ctypes.data,
            amp.n_arr.ctypes.data, amp._phase0.ctypes.data, amp._jitter.ctypes.data, K,
            yp.ctypes.data, ym.ctypes.data, 1e-2, fp, fr, tab, keep.ctypes.data,
            ctypes.byref(nkeep), None, 0)

    assert call(f_phi.ctypes.data, f_r.ctypes.data, ctypes.byref(psd.host)) == 0
    assert nkeep.value > 0
    assert call(None, f_r.ctypes.data, ctypes.byref(psd.host)) == _lib.EFD_ERR_ARG
    assert call(f_phi.ctypes.data, None, ctypes.byref(psd.host)) == _lib.EFD_ERR_ARG
    assert call(f_phi.ctypes.data, f_r.ctypes.data, None) == _lib.EFD_ERR_ARG
    bad = _lib.PsdTable(psd.host.x, psd.host.c, 1)
    assert call(f_phi.ctypes.data, f_r.ctypes.data, ctypes.byref(bad)) == _lib.EFD_ERR_ARG
    # an all-negative table: every knot keeps nothing, nkeep = 0 and the call succeeds
    neg = amplitude.psd_table(ws.all_negative())
    assert call(f_phi.ctypes.data, f_r.ctypes.data, ctypes.byref(neg.host)) == 0
    assert nkeep.value == 0


# -- the generator ---------------------------------------------------------------------------------
def bare_generator(fn, backend="auto"):
    """The FD generator's host half only (no GPU needed), with a weighted selector."""
    from emri_frequencydomainwaveforms_amd.waveform import FastSchwarzschildEccentricFlux
    wg = FastSchwarzschildEccentricFlux.__new__(FastSchwarzschildEccentricFlux)
    wg.inspiral_generator = EMRIInspiral(backend=backend)
    wg.amplitude_generator = RomanAmplitude()
    wg.ylm_gen = GetYlms(assume_positive_m=True)
    wg.mode_selector = ModeSelector(wg.amplitude_generator.m0mask, sensitivity_fn=fn)
    wg.output_type, wg.last_modes = "fd", None
    wg._ylm_cache, wg._prefetched, wg._lock = {}, {}, threading.Lock()
    wg._prefetched_bytes, wg._inflight = 0, {}
    return wg


def test_upstream_routes_agree():
    """prepare() with the table (efd_host_modes_weighted), with a plain callable of the same
    function (numpy's selector on the native trajectory) and on the python backend keep the same
    modes, and not the unweighted ones; an explicit mode list ignores the sensitivity."""
    call = (1e6, 10.0, 9.425031792736052, 0.35, 1.0, -np.pi / 2, 2.45, 1.0, 2.0, 0.1, 1e-2)
    table = bare_generator(fdutils.get_sensitivity).prepare(*call)
    plain = bare_generator(lambda f: fdutils.get_sensitivity(f)).prepare(*call)
    pyb = bare_generator(fdutils.get_sensitivity, backend="python").prepare(*call)
    unweighted = bare_generator(None).prepare(*call)
    for d in (plain, pyb):
        np.testing.assert_array_equal(d["m"], table["m"])
        np.testing.assert_array_equal(d["n"], table["n"])
    np.testing.assert_array_equal(plain["teuk"].shape, table["teuk"].shape)
    assert np.abs(plain["teuk"] - table["teuk"]).max() <= 1e-14 * np.abs(table["teuk"]).max()
    assert table["teuk"].shape[1] != unweighted["teuk"].shape[1]
    modes = [(2, 2, 0), (3, 2, 1)]
    a = bare_generator(fdutils.get_sensitivity).prepare(*call, mode_selection=modes)
    b = bare_generator(None).prepare(*call, mode_selection=modes)
    np.testing.assert_array_equal(a["teuk"], b["teuk"])


def test_generator_takes_mode_selector_kwargs():
    from emri_frequencydomainwaveforms_amd.waveform import (FastSchwarzschildEccentricFlux,
                                                            GenerateEMRIWaveform)
    kw = dict(mode_selector_kwargs=dict(sensitivity_fn=fdutils.get_sensitivity))
    for sum_kwargs in (dict(output_type="fd"), dict(output_type="td")):
        g = FastSchwarzschildEccentricFlux(sum_kwargs=sum_kwargs, **kw)
        assert g.mode_selector.sensitivity_fn is fdutils.get_sensitivity
        assert g.mode_selector.psd_table.host.n == 600 and g.mode_selector.use_gpu is False
    g = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=dict(output_type="fd"),
                             **kw)
    assert g.waveform_generator.mode_selector.sensitivity_fn is fdutils.get_sensitivity
    g = FastSchwarzschildEccentricFlux(sum_kwargs=dict(output_type="fd"))
    assert g.mode_selector.sensitivity_fn is None and g.mode_selector.psd_table is None
