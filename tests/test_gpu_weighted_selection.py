"""Noise-weighted mode selection on the device (efd_psd_eval, efd_modes_select_batch_weighted)
against scipy, the numpy ModeSelector(sensitivity_fn) and the host C++ (efd_host_modes_weighted),
and the batched callers with a weighted generator, upstream="device" against "host". STAND-IN
PHYSICS, NOT FEW.

The kept set is compared element for element under the preconditions of
tests/test_weighted_selection.py; the templates under the host route's own response to a 1e-14
amplitude perturbation (the method of tests/test_gpu_device_upstream.py).
"""

import contextlib
import ctypes

import numpy as np
import pytest
from scipy.interpolate import PPoly

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib, amplitude, fdutils, pe  # noqa: E402
from emri_frequencydomainwaveforms_amd.amplitude import (ModeSelector,  # noqa: E402
                                                         RomanAmplitude,
                                                         SyntheticTeukolskyAmplitude)
from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t  # noqa: E402
from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform  # noqa: E402
from emri_frequencydomainwaveforms_amd.ylm import GetYlms  # noqa: E402
from tests import weighted_selection_ref as ws  # noqa: E402
from tests.test_gpu_device_upstream import DT, E0, MU, PERTURB, SUM_KW, M, T  # noqa: E402
from tests.test_gpu_modes_device import CUT_GAP, views_numpy  # noqa: E402

SENS = dict(mode_selector_kwargs=dict(sensitivity_fn=fdutils.get_sensitivity))


@pytest.fixture(scope="module")
def model():
    """The amplitude model, the native trajectories (with their knot frequencies) of S1 and S2,
    numpy's amplitudes on them and the LISA table (computed once, read-only)."""
    traj = EMRIInspiral()
    amp = RomanAmplitude()
    src = {}
    for name, (M_, mu, e0, T_) in (("S1", ws.S1), ("S2", ws.S2)):
        p0 = get_p_at_t(traj, 0.99 * T_, [M_, mu, 0.0, e0, 1.0])
        t, p, e, _, _, f_phi, f_r = traj.with_frequencies(M_, mu, 0.0, p0, e0, 1.0, T=T_)
        A = amp(p, e)
        for a in (p, e, f_phi, f_r, A):
            a.setflags(write=False)
        src[name] = (p, e, f_phi, f_r, A)
    yg = GetYlms(assume_positive_m=True)
    ylms = {k: yg(amp.l_arr, amp.m_arr, th, ph)
            for k, (th, ph) in (("a", (1.0, -np.pi / 2)), ("b", (np.pi / 3, np.pi / 3)))}
    return amp, src, ylms, amplitude.psd_table(fdutils.get_sensitivity)


@pytest.mark.parametrize("nf", [1, 63, 64, 65, 1025])
def test_psd_eval_matches_ppoly(nf):
    tab = ws.lisa()
    lib = _lib.load()
    pts = ws.psd_points(tab)
    f = np.random.default_rng(nf).permutation(pts)[:nf].copy()
    if nf > 1:
        f[:5] = [0.0, 1e-6, 2.0, tab.x[0], tab.x[-1]]
        f[5] = np.nan
    ref = PPoly(tab.c, tab.x, extrapolate=True)(f)
    psd = amplitude.psd_table(tab)
    dev = torch.device("cuda")
    fd = torch.from_numpy(f).to(dev)
    guard = 8
    out = torch.full((nf + guard,), -7.0, dtype=torch.float64, device=dev)
    dpsd = psd.device(dev)
    _lib.check(lib.efd_psd_eval(ctypes.byref(dpsd), fd.data_ptr(), nf, out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream), "efd_psd_eval", lib)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[nf:] == -7.0).all()
    got = got[:nf]
    bound, Mf = ws.psd_bound(tab, f)
    fin = ~np.isnan(f)
    err = np.abs(got - ref)[fin]
    print(f"efd_psd_eval nf={nf}: max |d| / (u M) = {(err / (ws.U * Mf[fin])).max():.3g} (<= 32)")
    assert np.all(err <= bound[fin])
    assert np.isnan(got[~fin]).all()
    # the host twin rounds the same operations: the same bits
    np.testing.assert_array_equal(got, ws.eval_cpu(lib, tab, f))


def test_psd_eval_rejects_bad_arguments():
    lib = _lib.load()
    dev = torch.device("cuda")
    d = amplitude.psd_table(ws.lisa()).device(dev)
    f = torch.zeros(4, dtype=torch.float64, device=dev)
    assert lib.efd_psd_eval(None, f.data_ptr(), 4, f.data_ptr(), None) == _lib.EFD_ERR_ARG
    assert lib.efd_psd_eval(ctypes.byref(d), None, 4, f.data_ptr(), None) == _lib.EFD_ERR_ARG
    for n in (1, 4097):
        bad = _lib.PsdTable(d.x, d.c, n)
        assert lib.efd_psd_eval(ctypes.byref(bad), f.data_ptr(), 4, f.data_ptr(),
                                None) == _lib.EFD_ERR_ARG
    assert "efd_psd_eval" in _lib.last_error(lib)
    assert lib.efd_psd_eval(ctypes.byref(d), None, 0, None, None) == 0


def weighted_reference(amp, src, y, name, eps, psd):
    """(numpy's kept set, the weighted branch powers and fold map) of one source."""
    p, e, f_phi, f_r, A = src[name]
    F = ws.mode_freq(amp.m_arr, amp.n_arr, f_phi, f_r)
    power, fold = ws.weighted_powers(A, y, amp.m0mask, ws.weights(ws.lisa(), F))
    ref = ModeSelector(amp.m0mask, sensitivity_fn=fdutils.get_sensitivity)(
        A, y, (amp.l_arr, amp.m_arr, amp.n_arr), eps=eps, mode_freqs=(f_phi, f_r))
    return ref, power, fold


@pytest.mark.parametrize("eps", [1e-2, 1e-5])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_exact_set_and_amplitudes(model, name, eps):
    amp, src, ylms, psd = model
    p, e, f_phi, f_r, A = src[name]
    y = ylms["a"]
    ref, power, _ = weighted_reference(amp, src, y, name, eps, psd)
    ws.assert_order_independent(power, eps, f"{name} eps={eps:g}")
    khost, _ = amp.select(p, e, y, eps, lib=_lib.load(), f_phi=f_phi, f_r=f_r, psd=psd)
    np.testing.assert_array_equal(khost, ref)
    (keep, K, v), = amp.select_batch_device([p], [e], [y], eps, f_phi_list=[f_phi],
                                            f_r_list=[f_r], psd=psd)
    got = views_numpy(v)
    assert K == len(ref)
    np.testing.assert_array_equal(got["keep"], ref)
    np.testing.assert_array_equal(v["keep_host"], ref)
    unweighted = ModeSelector(amp.m0mask)(A, y, None, eps=eps)
    assert set(ref) != set(unweighted)
    Aref = A[:, ref]
    err = np.abs(got["amp"] - Aref).max() / np.abs(Aref).max()
    print(f"{name} eps={eps:g}: K = {K} (unweighted {len(unweighted)}), nt = {len(p)}, "
          f"amplitude error {err:.3g} max|A|")
    assert err <= 1e-14
    np.testing.assert_array_equal(got["m"], amp.m_arr[ref])
    np.testing.assert_array_equal(got["n"], amp.n_arr[ref])
    nm = amp.num_teuk_modes
    np.testing.assert_array_equal(got["ylm_p"], y[:nm][ref])
    np.testing.assert_array_equal(got["ylm_m"], y[nm:][ref])


GENERIC = [("five_m0_modes", "lisa"), ("one_mode", "lisa"), ("forty", "wall"), ("forty", "flat"),
           ("forty", "negative"), ("full_sort_8192", "gentle")]


@pytest.fixture(scope="module")
def cases():
    return ws.generic_cases()


@pytest.mark.parametrize("case,table", GENERIC)
def test_generic_route(cases, case, table):
    """ModeSelector(sensitivity_fn, use_gpu=True): the amplitudes are given, device tensors in,
    a device int32 tensor out, equal to the numpy ModeSelector with the same function."""
    teuk, ylms, m0mask, inds, eps, (f_phi, f_r) = cases[case]
    fn = getattr(ws, table)()
    W = ws.weights(fn, ws.mode_freq(inds[1], inds[2], f_phi, f_r))
    power, _ = ws.weighted_powers(teuk, ylms, m0mask, W)
    ws.assert_order_independent(power, eps, f"{case}/{table}")
    if case == "full_sort_8192":
        # every one of the 8,192 branches is a candidate: above the floor eps total / np
        assert (power.min(axis=1) > eps * power.sum(axis=1) / power.shape[1]).all()
    ref = ModeSelector(m0mask, sensitivity_fn=fn)(teuk, ylms, inds, eps=eps,
                                                 mode_freqs=(f_phi, f_r))
    dev = torch.device("cuda")
    sel = ModeSelector(m0mask, sensitivity_fn=fn, use_gpu=True)
    keep = sel(torch.from_numpy(teuk).to(dev), torch.from_numpy(ylms).to(dev), inds, eps=eps,
               mode_freqs=(torch.from_numpy(f_phi).to(dev), torch.from_numpy(f_r).to(dev)))
    assert keep.is_cuda and keep.dtype == torch.int32
    np.testing.assert_array_equal(keep.cpu().numpy(), ref)
    if table == "flat":
        np.testing.assert_array_equal(ref, ModeSelector(m0mask)(teuk, ylms, None, eps=eps))
    if table == "negative":   # nothing kept: an empty tensor, no error at this layer
        none = ModeSelector(m0mask, sensitivity_fn=ws.all_negative(), use_gpu=True)(
            torch.from_numpy(teuk).to(dev), torch.from_numpy(ylms).to(dev), inds, eps=eps,
            mode_freqs=(f_phi, f_r))
        assert none.numel() == 0


def test_no_table_is_an_error_on_the_device(cases):
    teuk, ylms, m0mask, inds, eps, fr = cases["forty"]
    dev = torch.device("cuda")
    sel = ModeSelector(m0mask, sensitivity_fn=lambda f: 1.0 + f, use_gpu=True)
    with pytest.raises(ValueError, match="CubicSpline"):
        sel(torch.from_numpy(teuk).to(dev), torch.from_numpy(ylms).to(dev), inds, eps=eps,
            mode_freqs=fr)
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW, use_gpu=True,
                               return_list=True,
                               mode_selector_kwargs=dict(sensitivity_fn=lambda f: 1.0 + f))
    rows = np.array([[M, MU, 0.0, 9.5, E0, 1.0, 1.0, 0.5, 0.3, 0.8, 1.1, 0.2, 0.0, 0.4]])
    out = torch.empty((1, 2, gen.positive_bins(T=0.01, dt=DT)), dtype=torch.complex128,
                      device=dev)
    with pytest.raises(ValueError, match="CubicSpline"):
        gen.generate_batch(rows, out, T=0.01, dt=DT, eps=1e-2, upstream="device")


def test_flat_table_is_the_unweighted_call_bitwise(model):
    """S = 0.25 scales every power by 4 exactly, so the sort, the sums and the cut are the
    unweighted ones: keep, amp, m, n and ylm are bitwise the unweighted call's."""
    amp, src, ylms, _ = model
    flat = amplitude.psd_table(ws.flat())
    for name, eps in (("S1", 1e-2), ("S2", 1e-5)):
        p, e, f_phi, f_r, _ = src[name]
        a = views_numpy(amp.select_batch_device([p], [e], [ylms["a"]], eps)[0][2])
        b = views_numpy(amp.select_batch_device([p], [e], [ylms["a"]], eps, f_phi_list=[f_phi],
                                                f_r_list=[f_r], psd=flat)[0][2])
        assert a["keep"].size > 0
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_batch_bitwise(model):
    """16 walkers (S1 and S2 mixed; two viewing angles; every third walker unweighted through
    NULL frequencies) in one call: bitwise the outputs of 16 calls with count = 1, and of a
    second run. The unweighted walkers keep efd_modes_select_batch's set."""
    amp, src, ylms, psd = model
    names = ["S1", "S2", "S2", "S1"] * 4
    ps = [src[k][0] for k in names]
    es = [src[k][1] for k in names]
    fp = [None if i % 3 == 0 else src[k][2] for i, k in enumerate(names)]
    fr = [None if i % 3 == 0 else src[k][3] for i, k in enumerate(names)]
    ys = [ylms["a" if i % 3 else "b"] for i in range(16)]
    eps = [1e-2 if i % 2 else 1e-3 for i in range(16)]
    runs = [[views_numpy(v) for _, _, v in
             amp.select_batch_device(ps, es, ys, eps, f_phi_list=fp, f_r_list=fr, psd=psd)]
            for _ in range(2)]
    single = [views_numpy(amp.select_batch_device([p], [e], [y], ep, f_phi_list=[a], f_r_list=[b],
                                                  psd=psd)[0][2])
              for p, e, y, ep, a, b in zip(ps, es, ys, eps, fp, fr)]
    plain = [views_numpy(v) for _, _, v in amp.select_batch_device(ps, es, ys, eps)]
    differ = 0
    for i, (a, b, c, d) in enumerate(zip(runs[0], runs[1], single, plain)):
        assert a["keep"].size > 0
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
            np.testing.assert_array_equal(a[k], c[k], err_msg=k)
        if i % 3 == 0:
            np.testing.assert_array_equal(a["keep"], d["keep"])
        else:
            differ += not np.array_equal(a["keep"], d["keep"])
    assert differ >= 5


def test_near_tie(model):
    """S1 seen from theta = phi = pi/3 at eps = 1e-5, weighted: the cut falls on two powers that
    agree to ~3e-15. The device set must hold every surely kept mode and nothing but those and
    the tied ones (the bracket of tests/test_gpu_modes_device.py: test_near_tie)."""
    amp, src, ylms, psd = model
    p, e, f_phi, f_r, A = src["S1"]
    y, eps = ylms["b"], 1e-5
    _, power, fold = weighted_reference(amp, src, y, "S1", eps, psd)
    sure, tied = set(), set()
    for i in range(len(power)):
        order = np.argsort(power[i])[::-1]
        ps = power[i][order]
        cs = np.cumsum(ps)
        before = np.concatenate([[0.0], cs[:-1]])
        kept = before < cs[-1] * (1.0 - eps)
        kept[0] = True
        c = int(kept.sum())
        pc = ps[c - 1]                       # the cut element: the last kept power
        near = np.abs(power[i] - pc) <= CUT_GAP * pc
        is_tied = c < len(ps) and ps[c] >= pc * (1.0 - CUT_GAP)
        sure |= set(fold[power[i] > pc * (1.0 + CUT_GAP)].tolist())
        if is_tied:
            tied |= set(fold[near].tolist())
        else:
            sure |= set(fold[order[:c]].tolist())
    loose = tied - sure
    print(f"near tie: {len(sure)} sure modes, {len(loose)} tied and not sure: {sorted(loose)}")
    assert tied, "the fixture has no tied cut"
    assert len(loose) <= 2
    (keep, K, v), = amp.select_batch_device([p], [e], [y], eps, f_phi_list=[f_phi],
                                            f_r_list=[f_r], psd=psd)
    got = set(keep.cpu().numpy().tolist())
    assert sure <= got <= (sure | tied), (sorted(sure - got), sorted(got - sure - tied))


# -- the batched callers ---------------------------------------------------------------------------
@contextlib.contextmanager
def perturbed_host_amplitudes(seed=20260115):
    """tests/test_gpu_device_upstream.py's patch, accepting select's new keywords."""
    orig = SyntheticTeukolskyAmplitude.select

    def select(self, p, e, ylms, eps, lib=None, **kw):
        keep, teuk = orig(self, p, e, ylms, eps, lib=lib, **kw)
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
    kw = dict(sum_kwargs=SUM_KW, use_gpu=True, return_list=True)
    gen = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", **kw, **SENS)
    plain = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", **kw)
    return gen, plain, rows


@pytest.mark.parametrize("eps", [1e-2, 1e-5])
def test_templates_match_host_route(scan, eps):
    gen, plain, rows = scan
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
    # the kept modes are the host route's, and not the unweighted generator's
    calls, _ = gen.device_calls(rows, T, eps)
    assert len(wg.last_modes_batch) == 3
    pw = plain.waveform_generator
    for c, got in zip(calls, wg.last_modes_batch):
        wg._upstream(*c, None, True)
        for a, b in zip(got, wg.last_modes):
            np.testing.assert_array_equal(a, b)
        pw._upstream(*c, None, True)
        assert set(zip(*(x.tolist() for x in got))) != set(zip(*(x.tolist() for x in
                                                                 pw.last_modes)))
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
    """pe.setup(mode_selector_kwargs=...), upstream="device" against "host", with the logL bound
    of tests/test_gpu_device_upstream.py: |dlogL| <= 2 (4 |r| delta + 2 delta^2)."""
    sh = pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, **SENS)
    sd = pe.setup(Tobs=T, dt=DT, eps=1e-2, nwalkers=4, upstream="device", **SENS)
    for s in (sh, sd):
        sel = s.few.waveform_generator.mode_selector
        assert sel.sensitivity_fn is fdutils.get_sensitivity and sel.psd_table is not None
    np.testing.assert_array_equal(sh.start, sd.start)
    pts = np.concatenate([sh.start, sh.truth6[None, :]])
    ll_host = sh.like(pts, **sh.kwargs)
    ll_dev = sd.like(pts, **sd.kwargs)
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
