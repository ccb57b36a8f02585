"""<d|h> and <h|h> from the fused mode sum (efd_modesum_sum_dh_hh), from written templates
(efd_dh_hh_rows) and through Likelihood.parts / ProfiledLikelihood / pe.setup(marginalize=...).

The kernel-level shapes are test_gpu_batch_prepare.py's: six ragged sources (T = 0.02 yr,
dt = 20 s, eps 1e-2 .. 1e-5: both list modes), the dt = 2 s grid where most tiles hold no
record, the no-segment grid and the split-plan shape. Tolerances: 1e-12 of the sum of the
terms' magnitudes where two summation orders meet, bitwise where the
order is the same."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib  # noqa: E402
from emri_frequencydomainwaveforms_amd.reductions import Reducer  # noqa: E402
from emri_frequencydomainwaveforms_amd.summation import (BatchPreparer, fd_grid,  # noqa: E402
                                                         sum_batch, sum_batch_dh_hh)
from tests.helpers import source_inputs  # noqa: E402

NAN = float("nan")
KEYS = ("t", "phi_phi", "phi_r", "f_phi", "f_r", "m", "n", "ylm_p", "ylm_m")


def _host(d):
    h = {k: d[k] for k in KEYS}
    h["amp"] = np.ascontiguousarray(d["amp"].T)     # [nt][K]
    return h


@pytest.fixture(scope="module")
def sources():
    out = []
    for M, e0, eps in ((3e5, 0.35, 1e-2), (5e5, 0.2, 1e-3), (2e5, 0.5, 1e-2), (4e5, 0.1, 1e-5),
                       (3e5, 0.6, 1e-2), (6e5, 0.3, 1e-4)):
        out.append(source_inputs(M=M, e0=e0, T=0.02, dt=20.0, eps=eps))
    return out


def _data(nb, seed, dscale=1e-22, wscale=1e40):
    rng = np.random.default_rng(seed)
    d = torch.as_tensor(rng.standard_normal((2, nb)) + 1j * rng.standard_normal((2, nb)),
                        device="cuda") * dscale
    w = torch.as_tensor(rng.uniform(0.5, 2.0, (2, nb)) * wscale, device="cuda")
    w[:, 0] = 0.0   # a zeroed bin, as Likelihood's start_ind
    return d, w


def _flush(srcs, freq, k0, group=None, depth=1):
    B = BatchPreparer(group=group or len(srcs), depth=depth)
    for s in srcs:
        B.submit(_host(s), freq, True, s["prefactor"], k0=k0, prepare_only=True)
    gi, jobs = B.flush()
    torch.cuda.current_stream().wait_stream(B.stream(gi))
    return B, gi, jobs


def _templates(jobs, nb):
    """The jobs' h+ / hx written by the same preparation: complex128 [n][2][nb]."""
    h = torch.zeros((len(jobs), 2, nb), dtype=torch.complex128, device="cuda")
    sum_batch([(eng, dict(kw, hp=torch.view_as_real(h[i, 0]), hc=torch.view_as_real(h[i, 1])))
               for i, (eng, kw) in enumerate(jobs)])
    return h


def _dh(B, gi, d, w, n, dense):
    """sum_dh_hh with the partials buffer filled with NaN first: nothing may leak from it."""
    out = torch.full((n, 3), NAN, dtype=torch.float64, device="cuda")
    G = B.groups[gi]
    if G.dh_part is not None:
        G.dh_part.fill_(NAN)
    B.sum_dh_hh(gi, d, w, out, torch.cuda.current_stream().cuda_stream, dense=dense)
    return out


def _numpy_sums(h, d, w):
    """float64 numpy: (values [n][3], sums of the terms' magnitudes [n][3], A = 4 sum |d||hw|)."""
    hw = (h * w[None]).cpu().numpy()
    dn = d.cpu().numpy()[None]
    ax = (1, 2)
    val = np.stack([4 * np.sum(dn.real * hw.real + dn.imag * hw.imag, axis=ax),
                    4 * np.sum(dn.real * hw.imag - dn.imag * hw.real, axis=ax),
                    4 * np.sum(hw.real ** 2 + hw.imag ** 2, axis=ax)], axis=1)
    mag = np.stack([4 * np.sum(np.abs(dn.real * hw.real) + np.abs(dn.imag * hw.imag), axis=ax),
                    4 * np.sum(np.abs(dn.real * hw.imag) + np.abs(dn.imag * hw.real), axis=ax),
                    val[:, 2]], axis=1)
    A = 4 * np.sum(np.abs(dn) * np.abs(hw), axis=ax)
    return val, mag, A


@pytest.fixture(scope="module")
def prepared(sources):
    """One flush of the six sources on their own grid, with the written templates and random
    data: shared, read-only."""
    freq_h = sources[0]["freq"]
    freq = torch.as_tensor(freq_h, device="cuda")
    nf, k0 = int(freq.numel()), int(np.searchsorted(freq_h, 0.0))
    d, w = _data(nf - k0, 3)
    B, gi, jobs = _flush(sources, freq, k0)
    # a first call sizes the group's partials buffer, which _dh then poisons before each call
    B.sum_dh_hh(gi, d, w, torch.empty((len(jobs), 3), dtype=torch.float64, device="cuda"),
                torch.cuda.current_stream().cuda_stream)
    h = _templates(jobs, nf - k0)
    torch.cuda.synchronize()
    B.wait()
    return dict(B=B, gi=gi, jobs=jobs, h=h, d=d, w=w, freq=freq, nf=nf, k0=k0)


@pytest.mark.parametrize("dt", [20.0, 2.0])
def test_against_numpy_on_written_templates(sources, prepared, dt):
    if dt == 20.0:
        P = prepared
        B, gi, jobs, h, d, w = (P[k] for k in ("B", "gi", "jobs", "h", "d", "w"))
    else:   # Nyquist ten times above the highest harmonic: most tiles hold no record
        freq_h = fd_grid(0.02, dt)
        freq = torch.as_tensor(freq_h, device="cuda")
        nf, k0 = int(freq.numel()), int(np.searchsorted(freq_h, 0.0))
        d, w = _data(nf - k0, 11)
        B, gi, jobs = _flush(sources, freq, k0)
        h = _templates(jobs, nf - k0)
        _dh(B, gi, d, w, len(jobs), False)
    dense = _dh(B, gi, d, w, len(jobs), True).cpu().numpy()
    sparse = _dh(B, gi, d, w, len(jobs), False).cpu().numpy()
    B.wait()
    val, mag, _ = _numpy_sums(h, d, w)
    assert np.all(np.isfinite(dense)) and np.all(np.isfinite(sparse))
    for got in (dense, sparse):
        print("worst |err| / sum|terms|:", np.max(np.abs(got - val) / mag))
        assert np.all(np.abs(got - val) <= 1e-12 * mag)
    assert np.all(val[:, 2] > 0)


def test_bitwise_routes_batches_and_repeats(sources, prepared):
    P = prepared
    B, gi, jobs, h, d, w = (P[k] for k in ("B", "gi", "jobs", "h", "d", "w"))
    n = len(jobs)
    dense = _dh(B, gi, d, w, n, True)
    runs = [_dh(B, gi, d, w, n, False) for _ in range(3)]
    assert all(torch.equal(r, dense) for r in runs)         # sparse == dense, repeats agree
    assert torch.all(torch.isfinite(dense))
    # a walker alone equals the same walker in the batch of six (both list modes)
    for i in (1, 3):
        one = torch.full((1, 3), NAN, dtype=torch.float64, device="cuda")
        part = torch.full((3 * int(B.lib.efd_loglike_tile_count(P["nf"])),), NAN,
                          dtype=torch.float64, device="cuda")
        for dn in (False, True):
            sum_batch_dh_hh([jobs[i]], d, w, one, dense=dn, part=part)
            assert torch.equal(one[0], dense[i])
    # the written templates through efd_dh_hh_rows: another order
    rows = Reducer().dh_hh_rows(h, d, w).cpu().numpy()
    _, mag, _ = _numpy_sums(h, d, w)
    assert np.all(np.abs(rows - dense.cpu().numpy()) <= 1e-12 * mag)
    # ... whose rows do not depend on the call's other rows, and repeat bitwise
    assert torch.equal(Reducer().dh_hh_rows(h[2], d, w)[0], torch.as_tensor(rows[2], device="cuda"))
    B.wait()


def test_seventeen_walkers_equal_smaller_groups(sources, prepared):
    """BatchPreparer.sum_dh_hh's chunks of EFD_BATCH_MAX: 17 walkers in one flush against
    groups of 9 and 8."""
    assert _lib.EFD_BATCH_MAX == 16
    P = prepared
    freq, k0, d, w = P["freq"], P["k0"], P["d"], P["w"]
    walkers = [sources[i % len(sources)] for i in range(17)]

    def run(B, parts):
        out = torch.full((17, 3), NAN, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        g0 = 0
        for cnt in parts:
            for s in walkers[g0:g0 + cnt]:
                B.submit(_host(s), freq, True, s["prefactor"], k0=k0, prepare_only=True)
            gi, jobs = B.flush()
            B.sum_dh_hh(gi, d, w, out[g0:g0 + cnt], B.stream(gi).cuda_stream)
            g0 += cnt
        B.wait()
        return out

    got = run(BatchPreparer(group=17, depth=1), (17,))
    ref = run(BatchPreparer(group=9, depth=2), (9, 8))
    assert torch.all(torch.isfinite(ref)) and torch.equal(got, ref)
    assert torch.equal(got[:6], _dh(P["B"], P["gi"], d, w, 6, False))


@pytest.mark.parametrize("split_min", ["", "-1"])
def test_split_tiles(split_min, monkeypatch):
    """test_fused_loglike_split_tiles' shape: the sparse launch runs the split plan (the last
    arriver's epilogue from spart), the dense one whole tiles."""
    if split_min:
        monkeypatch.setenv("EFD_SPLIT_MIN_COST", split_min)
    srcs = [source_inputs(M=M, e0=e0, T=0.5, dt=10.0, eps=3e-2)
            for M, e0 in ((1e6, 0.35), (8e5, 0.3), (1.2e6, 0.4), (9e5, 0.25))]
    fmax = max(float(np.abs(s["m"] * s["f_phi"][:, None] + s["n"] * s["f_r"][:, None]).max())
               for s in srcs)
    p = np.linspace(0.0, 1.01 * fmax, 4001)
    freq = torch.as_tensor(np.concatenate([-p[::-1][:-1], p]), device="cuda")
    nf = int(freq.numel())
    k0 = nf // 2
    d, w = _data(nf - k0, 3, 1e-21, 1e20)
    B, gi, jobs = _flush(srcs, freq, k0)
    _dh(B, gi, d, w, 4, False)
    dense = _dh(B, gi, d, w, 4, True)
    got = [_dh(B, gi, d, w, 4, False) for _ in range(3)]
    torch.cuda.synchronize()
    B.wait()
    plans = [eng.split_plan() for eng, _ in jobs]
    assert any(ns > 0 for _, ns in plans), plans
    assert torch.all(torch.isfinite(dense)) and torch.all(dense[:, 2] > 0)
    assert all(torch.equal(g, dense) for g in got)


def test_exact_identities(sources, prepared):
    P = prepared
    B, gi, jobs, h, w = (P[k] for k in ("B", "gi", "jobs", "h", "w"))
    for i in (0, 3):
        # d = (written template) w, each component's product rounded
        d = torch.view_as_complex((torch.view_as_real(h[i]) * w[..., None]).contiguous())
        for dense in (True, False):
            got = _dh(B, gi, d, w, len(jobs), dense)[i].cpu().numpy()
            assert got[0] == got[2] and got[2] > 0.0 and got[1] == 0.0
        r = Reducer().dh_hh_rows(h[i], d, w)[0].cpu().numpy()
        assert r[0] == r[2] and r[1] == 0.0
    got = _dh(B, gi, torch.zeros_like(P["d"]), w, len(jobs), False).cpu().numpy()
    assert np.all(got[:, :2] == 0.0) and np.all(got[:, 2] > 0)
    B.wait()


def test_no_segment_grid_is_exactly_zero(sources):
    fmax = max(float(np.abs(s["m"] * s["f_phi"][:, None] + s["n"] * s["f_r"][:, None]).max())
               for s in sources[:3])
    p = np.linspace(2.0 * fmax, 3.0 * fmax, 2001)
    freq = torch.as_tensor(np.concatenate([-p[::-1], [0.0], p]), device="cuda")
    nf = int(freq.numel())
    k0 = nf // 2
    d, w = _data(nf - k0, 5, 1.0, 1.0)
    B, gi, jobs = _flush(sources[:3], freq, k0)
    _dh(B, gi, d, w, 3, False)
    for dense in (True, False):
        got = _dh(B, gi, d, w, 3, dense).cpu().numpy()
        assert np.array_equal(got, np.zeros((3, 3)))
    B.wait()


def test_consistent_with_the_fused_loglike(sources, prepared):
    P = prepared
    B, gi, jobs, h, d, w = (P[k] for k in ("B", "gi", "jobs", "h", "d", "w"))
    n = len(jobs)
    ll = torch.empty(n, dtype=torch.float64, device="cuda")
    B.sum_loglike(gi, d, w, ll, torch.cuda.current_stream().cuda_stream)
    got = _dh(B, gi, d, w, n, False).cpu().numpy()
    ll = ll.cpu().numpy()
    B.wait()
    d_d = float(Reducer().inner(d, d).real.item())
    _, _, A = _numpy_sums(h, d, w)
    miss = np.abs(ll + 0.5 * (d_d - 2.0 * got[:, 0] + got[:, 2]))
    bound = 1e-12 * 0.5 * (d_d + 2.0 * A + got[:, 2])
    print("identity miss / bound:", miss / bound)
    assert np.all(miss <= bound)


def test_failing_walker_gets_three_nan(sources):
    """test_fused_loglike_marks_failing_walker_nan's mechanism: |m| > 255 on walker 2 sets the
    workspace's sticky flag; its three outputs are NaN, the others' are values, and the flag
    stays for efd_modesum_status_batch."""
    freq = torch.as_tensor(sources[0]["freq"], device="cuda")
    nf = int(freq.numel())
    B = BatchPreparer(group=3, depth=1)
    for i in range(3):
        hst = _host(sources[i])
        if i == 2:
            hst["m"] = hst["m"].copy()
            hst["m"][0] = 300
        B.submit(hst, freq, True, sources[i]["prefactor"], prepare_only=True)
    gi, jobs = B.flush()
    cur = torch.cuda.current_stream()
    cur.wait_stream(B.stream(gi))
    d = torch.ones((2, nf), dtype=torch.complex128, device="cuda")
    w = torch.ones((2, nf), dtype=torch.float64, device="cuda")
    for dense in (True, False):
        out = torch.full((3, 3), 1.0, dtype=torch.float64, device="cuda")
        B.sum_dh_hh(gi, d, w, out, cur.cuda_stream, dense=dense)
        got = out.cpu().numpy()
        assert np.all(np.isnan(got[2])) and np.all(np.isfinite(got[:2])) and np.all(got[:2, 2] > 0)
    lib = _lib.load()
    flags = (ctypes.c_int32 * 3)()
    lib.efd_modesum_status_batch(B.workspace_ptrs(gi), 3, flags, cur.cuda_stream)
    assert list(flags) == [0, 0, 2]


# ---- Likelihood.parts, one test per branch ---------------------------------------------------
def _check_parts(like, gen, walkers, kw, branch, templates=None):
    """parts against the identity with get_ll of the same object, and against
    diagnostic.inner_product(..., complex=True) on gen(*params); returns (d_h, h_h).
    branch: the branch both calls must report (Likelihood.branch_taken), so that neither output
    kind is quietly sent down another route.
    templates: the walkers' templates [n][2][nb] where gen(*params) is not what the branch
    evaluates (the device trajectory)."""
    from emri_frequencydomainwaveforms_amd import diagnostic as dg
    ll = like.get_ll(walkers, **kw)
    took = like.branch_taken
    d_h, h_h = like.parts(walkers, **kw)
    print("branch of get_ll, of parts:", took, like.branch_taken)
    assert took == like.branch_taken == branch
    assert d_h.dtype == np.complex128 and h_h.dtype == np.float64
    assert d_h.shape == h_h.shape == (len(walkers),)
    d_d = like.d_d
    s0 = like.start_ind
    f = like.freqs[s0:]
    psd = np.asarray(like.psd[0], dtype=np.float64)[s0:]
    # the unweighted data, from the weighted one (its dropped bin left out)
    with np.errstate(invalid="ignore", divide="ignore"):
        data = [(like._d[c] / like._w[c])[s0:] for c in range(2)]
    for i, p in enumerate(walkers):
        if templates is not None:
            h = templates[i]
        else:
            h = torch.stack([torch.as_tensor(c, device="cuda") for c in gen(*p, **kw)])
            h = h.to(torch.complex128)
        _, mag, A = _numpy_sums(h[None], like._d, like._w_templ)
        miss = abs(ll[i] + 0.5 * (d_d - 2.0 * d_h[i].real + h_h[i]))
        bound = 1e-12 * 0.5 * (d_d + 2.0 * A[0] + h_h[i])
        ip = dg.inner_product(data, [h[0, s0:], h[1, s0:]], f_arr=f, PSD=psd, complex=True)
        hh = dg.inner_product([h[0, s0:], h[1, s0:]], [h[0, s0:], h[1, s0:]], f_arr=f, PSD=psd)
        print(f"walker {i}: identity {miss / bound:.3f} of its bound; against inner_product "
              f"{abs(d_h[i].real - ip.real) / mag[0, 0]:.2e} "
              f"{abs(d_h[i].imag - ip.imag) / mag[0, 1]:.2e} "
              f"{abs(h_h[i] - hh) / mag[0, 2]:.2e} of sum|terms|")
        assert miss <= bound
        assert abs(d_h[i].real - ip.real) <= 1e-12 * mag[0, 0]
        assert abs(d_h[i].imag - ip.imag) <= 1e-12 * mag[0, 1]
        assert abs(h_h[i] - hh) <= 1e-12 * mag[0, 2]
    return d_h, h_h


SMALL = dict(Tobs=0.05, dt=20.0, eps=1e-2, M=3e5, e0=0.3, nwalkers=4)


@pytest.fixture(scope="module")
def small():
    from emri_frequencydomainwaveforms_amd import pe
    return pe.setup(**SMALL)


def _walkers(s):
    return np.vstack([s.truth14[None, :], s.transform.both_transforms(s.start)])


def test_parts_fused_host_upstream(small):
    s = small
    d_h, h_h = _check_parts(s.like, s.gen, _walkers(s), s.kwargs, "fused")
    # the data is the model's own output: the truth's numbers coincide
    assert d_h[0].real == h_h[0] and d_h[0].imag == 0.0
    # separate_d_h=True returns the pair through get_ll, and __call__ with subset through it
    s.like.separate_d_h, keep = True, s.like.subset
    try:
        a, b = s.like.get_ll(_walkers(s), **s.kwargs)
        assert np.array_equal(a, d_h) and np.array_equal(b, h_h)
        s.like.subset = 3
        start = np.vstack([s.truth6[None, :], s.start])
        a, b = s.like(start, **s.kwargs)
        assert a.shape == b.shape == (5,) and np.array_equal(a, d_h) and np.array_equal(b, h_h)
    finally:
        s.like.separate_d_h, s.like.subset = False, keep
    # device tensors on request
    s.like.return_cupy = True
    try:
        a, b = s.like.parts(_walkers(s), **s.kwargs)
        assert a.is_cuda and a.dtype == torch.complex128 and b.dtype == torch.float64
        assert np.array_equal(a.cpu().numpy(), d_h) and np.array_equal(b.cpu().numpy(), h_h)
    finally:
        s.like.return_cupy = False


def test_truth_d_d_equals_h_h_bitwise(small):
    """The truth's Re <d|h>, <h|h> and d_d, the data being the model's own output, on the fused
    route. Measured on the MI355X: see DESIGN.md's section on the pair."""
    s = small
    d_h, h_h = s.like.parts(s.truth14[None, :], **s.kwargs)
    print("Re d_h, h_h, d_d:", repr(d_h[0].real), repr(h_h[0]), repr(s.like.d_d))
    assert d_h[0].real == h_h[0] == s.like.d_d


@pytest.mark.parametrize("route", [dict(upstream="device"),
                                   dict(upstream="device", trajectory="device")])
def test_parts_device_routes(small, route):
    """With the device trajectory the templates compared are generate_batch's on that route:
    gen(*params) integrates the trajectory on the host, and its templates differ from this
    route's by test_gpu_device_trajectory.py's delta (measured here against gen(*params): 8.7e-12
    of sum|terms| in Im <d|h> on the last start walker, 3.5e-14 and 1.2e-13 in the other two;
    the other walkers and the device upstream with the host trajectory <= 9e-17)."""
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(**SMALL, **route)
    W, templates = _walkers(s), None
    if "trajectory" in route:
        templates = torch.empty((len(W), 2, int(s.like._d.shape[1])), dtype=torch.complex128,
                                device="cuda")
        s.few.generate_batch(W, templates, **s.kwargs, **route)
        torch.cuda.synchronize()
    d_h, h_h = _check_parts(s.like, s.gen, W, s.kwargs, "fused", templates)
    assert np.all(h_h > 0)


def test_parts_pipelined_asymmetric_grid(small):
    from emri_frequencydomainwaveforms_amd.fdutils import get_fd_waveform_fromFD, get_sensitivity
    from emri_frequencydomainwaveforms_amd.likelihood import Likelihood
    s = small
    fmax = float(s.f_like[np.abs(s.like._d[0].cpu().numpy()) > 0].max()) * 1.01
    f_arr = np.hstack((-np.linspace(fmax, 0.0, 400)[:-1], np.linspace(0.0, fmax, 601)))
    kw = dict(s.kwargs, f_arr=f_arr)
    s.few(*s.truth14, **kw)
    assert not s.few.waveform_generator.create_waveform._sym
    gen = get_fd_waveform_fromFD(s.few, f_arr >= 0, SMALL["dt"])
    assert gen.can_pipeline
    like = Likelihood(gen, 2, f_arr=f_arr[f_arr >= 0], use_gpu=True)
    like.inject_signal(data_stream=gen(*s.truth14, **kw), noise_fn=[get_sensitivity] * 2,
                       noise_kwargs=[{}, {}])
    _check_parts(like, gen, _walkers(s), kw, "per_slot")
    # the plain fill branch, a plain callable and a vectorized one on the same grid
    class FillOnly:
        can_fill = True

        def fill(self, out, *a, **k):
            return gen.fill(out, *a, **k)

        def __call__(self, *a, **k):
            return gen(*a, **k)

    for tm, vec, branch in ((FillOnly(), False, "fill"),
                            (lambda *a, **k: gen(*a, **k), False, "call"),
                            (lambda *rows, **k: [gen(*r, **k) for r in rows], True, "vectorized")):
        lk2 = Likelihood(tm, 2, f_arr=f_arr[f_arr >= 0], use_gpu=True, vectorized=vec)
        lk2.inject_signal(data_stream=gen(*s.truth14, **kw), noise_fn=[get_sensitivity] * 2,
                          noise_kwargs=[{}, {}])
        _check_parts(lk2, gen, _walkers(s)[:3], kw, branch)


def test_parts_td_template():
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(template="td", Tobs=0.02, dt=20.0, M=3e5, nwalkers=4)
    _check_parts(s.like, s.gen, _walkers(s), s.kwargs, "window_batch")


def test_parts_short_windowed_grid():
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(Tobs=0.02, dt=10.0, M=1e5, window_flag=True, nwalkers=4)
    # (a grid too short for HannConvolution keeps the exact transform pair: no batch, the fill)
    assert not s.gen.can_fill_batch
    _check_parts(s.like, s.gen, _walkers(s), s.kwargs, "fill")


def test_parts_batched_window_path():
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(Tobs=0.75, dt=10.0, eps=1e-2, nwalkers=4, ntemps=1, window_flag=True)
    assert s.gen.can_fill_batch
    _check_parts(s.like, s.gen, _walkers(s)[:3], s.kwargs, "window_batch")


@pytest.mark.parametrize("mode", ["amplitude", "distance"])
def test_setup_marginalize(small, mode):
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(marginalize=mode, dist_range=(0.5, 8.0), **SMALL)
    assert small.marg is None and s.marg.mode == mode
    start = np.vstack([s.truth6[None, :], s.start])
    got = s.marg(start, **s.kwargs)
    ll = s.like(start, **s.kwargs)
    assert got.shape == ll.shape and got.dtype == np.float64 and np.all(np.isfinite(got))
    if mode == "amplitude":
        assert np.all(got >= ll)
        # the truth sits at its own amplitude and distance
        assert abs(s.marg.last["A_hat"][0] - 1.0) <= 1e-12
        assert abs(s.marg.last["D_hat"][0] - s.truth14[6]) <= 1e-11
    rho, mf = s.marg.snr(start, **s.kwargs)
    assert rho[0] > 0 and abs(mf[0] - rho[0]) <= 1e-12 * rho[0]
    assert np.all(mf <= np.sqrt(s.like.d_d) * (1.0 + 1e-12))      # Cauchy-Schwarz
