"""Noise realisations on the device: efd_noise_fd and efd_noise_overlap_rows against their host
twins and the numpy reference (tests/noise_ref.py), and the noisy Likelihood: inject_signal(
add_noise=True), get_ll and parts on every branch, pe.noise_scatter.

Tolerances: a draw's components within 4e-14 absolute of the reference (|xi| <= 8.57, ~1.5 ulp
in r, ~2 ulp in sin and cos and the rounding of the angle: ~1e-14, times 4); overlaps within
1e-12 sum |gain rows| 8.57 where two summation orders meet; logL within 1e-10 |logL| of float64
numpy on the branch's own written templates."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib, noise  # noqa: E402
from emri_frequencydomainwaveforms_amd.reductions import Reducer  # noqa: E402
from tests import noise_ref as nr  # noqa: E402

SEEDS = (2601996, 2 ** 63 + 5)
TOL = 4e-14
SEED = 2601996
SMALL = dict(Tobs=0.02, dt=20.0, M=3e5, nwalkers=4, freeze_gc=False)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _dev(x):
    return torch.as_tensor(x, device="cuda")


# ---- the kernels -------------------------------------------------------------------------------
def test_device_against_twin_and_reference(lib):
    """test_noise_ref.py's shapes, the counter's carry included; gain-0 and NaN bins exactly 0.
    Measured on the MI355X: 2.1e-15 against the twin, 8.9e-16 against the reference."""
    worst_twin = worst_ref = 0.0
    for seed in SEEDS:
        for real in (0, 7):
            for nbin, bin0 in ((1, 0), (63, 0), (64, 0), (65, 0), (4099, 0), (8, 2 ** 32 - 3)):
                got = noise.standard_noise(2, nbin, seed, real, bin0).cpu().numpy()
                twin = nr.noise_fd_cpu(lib, 2, nbin, seed, real, bin0)
                ref = 0.5 * nr.xi(seed, real, 2, nbin, bin0)
                for other, name in ((twin, "twin"), (ref, "ref")):
                    e = 2.0 * max(float(np.max(np.abs(got.real - other.real))),
                                  float(np.max(np.abs(got.imag - other.imag))))
                    if name == "twin":
                        worst_twin = max(worst_twin, e)
                    else:
                        worst_ref = max(worst_ref, e)
    print("worst |xi_device - xi_twin|:", worst_twin, " |xi_device - xi_ref|:", worst_ref)
    assert worst_twin <= TOL and worst_ref <= TOL
    rng = np.random.default_rng(5)
    gain = rng.uniform(0.5, 2.0, (2, 515))
    gain[:, 0] = np.nan
    gain[1, 7:40] = 0.0
    dead = np.isnan(gain) | (gain == 0.0)
    got = noise.standard_noise(2, 515, SEED, gain=gain).cpu().numpy()
    twin = nr.noise_fd_cpu(lib, 2, 515, SEED, gain=gain)
    assert np.all(got[dead] == 0.0) and not np.isnan(got.view(np.float64)).any()
    assert np.max(np.abs(got - twin)) <= TOL
    base = rng.standard_normal((2, 515)) + 1j * rng.standard_normal((2, 515))
    acc = noise.standard_noise(2, 515, SEED, gain=gain, out=_dev(base.copy()),
                               accumulate=True).cpu().numpy()
    np.testing.assert_array_equal(acc[dead], base[dead])
    np.testing.assert_array_equal(acc[~dead], (base + got)[~dead])
    assert noise.standard_noise(2, 0, SEED).shape == (2, 0)


def test_device_slices_are_bitwise_the_whole():
    whole = noise.standard_noise(2, 4099, SEED, 3)
    for bin0, n in ((0, 1000), (1000, 2000), (3000, 1099)):
        part = noise.standard_noise(2, n, SEED, 3, bin0=bin0)
        assert torch.equal(torch.view_as_real(part),
                           torch.view_as_real(whole[:, bin0:bin0 + n].contiguous()))
    # a launch with more bins than one pass of the grid covers (2048 workgroups x 256) agrees
    # with its slices too
    n = 2048 * 256 + 777
    big = noise.standard_noise(1, n, SEED, 1)
    tail = noise.standard_noise(1, 1000, SEED, 1, bin0=n - 1000)
    assert torch.equal(torch.view_as_real(big[:, n - 1000:].contiguous()), torch.view_as_real(tail))


@pytest.mark.parametrize("nbin", [1, 65, 4099])
@pytest.mark.parametrize("nrow", [1, 6])
def test_device_overlaps_against_twin(lib, nrow, nbin):
    rows, gain = nr.overlap_case(17 * nrow + nbin, nrow, 2, nbin)
    red = Reducer()
    bound = 1e-12 * np.sum(np.abs(np.where(np.isnan(gain), 0.0, gain)[None] * rows),
                           axis=(1, 2)) * nr.XI_MAX
    for real0 in (0, 9):
        twin = nr.noise_overlap_rows_cpu(lib, rows, gain, SEED, real0, 33)
        for ndraw in (1, 5, 33):
            got = red.noise_overlap_rows(_dev(rows), _dev(gain), SEED, ndraw, real0=real0)
            err = np.abs(got.cpu().numpy() - twin[:ndraw])
            assert np.all(err <= bound[None, :]), (real0, ndraw, float(np.max(err / bound)))


def test_device_overlaps_do_not_depend_on_the_split():
    """ndraw = 33 as 20 + 13 is bitwise one call; a row alone is bitwise the row among 16 (two
    row launches); more draws than a launch holds (256) chunk inside the call."""
    rows, gain = nr.overlap_case(3, 16, 2, 4099)
    r, g = _dev(rows), _dev(gain)
    red = Reducer()
    one = red.noise_overlap_rows(r, g, SEED, 33, real0=4)
    two = torch.cat([red.noise_overlap_rows(r, g, SEED, 20, real0=4),
                     red.noise_overlap_rows(r, g, SEED, 13, real0=24)])
    assert torch.equal(one, two) and bool(torch.isfinite(one).all())
    for p in (0, 7, 8, 15):
        alone = red.noise_overlap_rows(r[p:p + 1].contiguous(), g, SEED, 33, real0=4)
        assert torch.equal(alone[:, 0], one[:, p])
    many = red.noise_overlap_rows(r[:3].contiguous(), g, SEED, 300, real0=0)
    late = red.noise_overlap_rows(r[:3].contiguous(), g, SEED, 50, real0=250)
    assert torch.equal(many[250:], late)
    with pytest.raises(ValueError):
        red.noise_overlap_rows(torch.cat([r, r[:1]]), g, SEED, 1)


def test_generate_noise_fd_matches_the_recipe():
    """lisatools' helper: sqrt(S) 0.5 / sqrt(df) xi of the given channel."""
    from emri_frequencydomainwaveforms_amd.fdutils import get_sensitivity
    f = np.linspace(1e-4, 1e-2, 300)
    df = float(f[1] - f[0])
    got = noise.generate_noise_fd(f, df, seed=SEED, realization=2, channel=1,
                                  sensitivity_fn=get_sensitivity).cpu().numpy()
    want = np.sqrt(get_sensitivity(f) / df) * 0.5 * nr.xi(SEED, 2, 2, 300)[1]
    assert np.max(np.abs(got - want) / np.sqrt(get_sensitivity(f) / df)) <= TOL


# ---- the likelihood ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setups():
    """The TD tests' small setup, noiseless and noisy (shared, read-only)."""
    from emri_frequencydomainwaveforms_amd import pe
    return pe.setup(**SMALL), pe.setup(**SMALL, add_noise=True, noise_seed=SEED)


def _walkers(s):
    return np.vstack([s.truth14[None, :], s.transform.both_transforms(s.start)])


def _numpy_ll(like, h):
    """float64 numpy -1/2 * 4 sum |d - h w|^2 per template of h [n][2][nb] (device)."""
    r = like._d.cpu().numpy()[None] - h.cpu().numpy() * like._w_templ.cpu().numpy()[None]
    return -2.0 * np.sum(r.real ** 2 + r.imag ** 2, axis=(1, 2))


def _written_templates(s, W, route=None):
    """The walkers' templates as the setup's branch writes them: [n][2][nb] on the device."""
    nb = int(s.like._d.shape[1])
    out = torch.empty((len(W), 2, nb), dtype=torch.complex128, device="cuda")
    if route:
        s.few.generate_batch(W, out, **s.kwargs, **route)
    elif getattr(s.gen, "can_fill_batch", False):
        s.gen.fill_batch(out, W, **s.kwargs)
    else:
        for i, p in enumerate(W):
            out[i] = torch.stack([torch.as_tensor(c, device="cuda") for c in s.gen(*p, **s.kwargs)])
    torch.cuda.synchronize()
    return out


def _check_branch(s, route=None):
    """get_ll of the truth and the four start walkers within 1e-10 |logL| of numpy on the written
    templates; parts' identity to the same tolerance; the amplitude-profiled logL >= logL."""
    from emri_frequencydomainwaveforms_amd.likelihood import ProfiledLikelihood
    like = s.like
    assert like.noise_has_been_added and like.noise_seed == SEED and like._inj_call is None
    W = _walkers(s)
    want = _numpy_ll(like, _written_templates(s, W, route))
    ll = like.get_ll(W, **s.kwargs)
    print("logL:", ll, " |ll - numpy| / |ll|:", np.abs(ll - want) / np.abs(want))
    assert np.all(np.isfinite(ll)) and np.all(ll < 0.0)
    assert np.all(np.abs(ll - want) <= 1e-10 * np.abs(want))
    d_h, h_h = like.parts(W, **s.kwargs)
    ident = -0.5 * (like.d_d - 2.0 * d_h.real + h_h)
    print("|identity - ll| / |ll|:", np.abs(ident - ll) / np.abs(ll))
    assert np.all(np.abs(ident - ll) <= 1e-10 * np.abs(ll))
    start = np.vstack([s.truth6[None, :], s.start])
    prof = ProfiledLikelihood(like, "amplitude")(start, **s.kwargs)
    assert np.all(prof >= like(start, **s.kwargs))
    return ll


def test_noisy_data_is_the_noiseless_plus_half_xi(setups):
    clean, noisy = setups
    a, b = clean.like, noisy.like
    assert not a.noise_has_been_added and clean.info["noise_seed"] is None
    assert b.noise_has_been_added and noisy.info["noise_seed"] == SEED == b.noise_seed
    nb = int(b._d.shape[1])
    diff = (b._d - a._d).cpu().numpy()
    live = (b._w_templ != 0.0).cpu().numpy()
    ref = 0.5 * nr.xi(SEED, 0, 2, nb)
    assert live.sum() > nb      # (this grid's table PSD is finite at f = 0: no bin is dropped)
    assert np.all(diff[~live] == 0.0)
    e = np.abs(diff - ref)[live]
    print("max |d| :", float(a._d.abs().max()), " worst |(d_noisy - d) - xi / 2|:", e.max())
    assert max(np.abs((diff - ref).real[live]).max(), np.abs((diff - ref).imag[live]).max()) <= TOL
    assert torch.equal(a._w, b._w) and torch.equal(a._w_templ, b._w_templ)
    # kept as the reference computes it (pi sum diff_freqs S per channel), not added to logL
    want = sum(np.pi * np.sum(np.diff(clean.f_like, prepend=2 * clean.f_like[0] - clean.f_like[1])
                              * np.asarray(p)) for p in b.psd)
    assert np.isnan(want) or abs(b.noise_likelihood_factor - want) <= 1e-12 * abs(want)
    # the properties regenerate the strain noise from the seed: n sqrt(df / S) = xi / 2
    n = b.noise_to_add
    back = (n * b._w).cpu().numpy()
    assert np.all(back[~live] == 0.0) and np.max(np.abs(back - ref)[live]) <= TOL
    base = torch.as_tensor(np.asarray(b.base_injections), device="cuda")
    assert torch.equal(b.noise_added_base_injections, base + n)
    with pytest.raises(AttributeError):
        a.noise_to_add


def test_noisy_truth_and_seeds(setups):
    from emri_frequencydomainwaveforms_amd.fdutils import get_sensitivity
    from emri_frequencydomainwaveforms_amd.likelihood import Likelihood
    clean, s = setups
    like = s.like
    nb = int(like._d.shape[1])
    live = (like._w_templ != 0.0).cpu().numpy()
    x = nr.xi(SEED, 0, 2, nb)
    want = -0.5 * float(np.sum((x.real ** 2 + x.imag ** 2)[live]))
    ll = float(like.get_ll(s.truth14[None, :], **s.kwargs)[0])
    print("logL(truth):", ll, " -1/2 sum |xi|^2:", want, " rel:", abs(ll - want) / abs(want))
    assert ll < 0.0 and abs(ll - want) <= 1e-12 * abs(want)

    def again(seed, **kw):
        lk = Likelihood(s.gen, 2, f_arr=s.f_like, use_gpu=True)
        lk.inject_signal(data_stream=s.gen(*s.truth14, **s.kwargs),
                         noise_fn=[get_sensitivity, get_sensitivity], noise_kwargs=[{}, {}],
                         add_noise=True, noise_seed=seed, **kw)
        return lk
    same, other = again(SEED), again(SEED + 1)
    assert torch.equal(torch.view_as_real(same._d), torch.view_as_real(like._d))
    assert not torch.equal(other._d, like._d)
    # a second injection into a noisy likelihood adds the signal again and no second noise
    same.inject_signal(data_stream=s.gen(*s.truth14, **s.kwargs),
                       noise_fn=[get_sensitivity, get_sensitivity], noise_kwargs=[{}, {}],
                       add_noise=True, noise_seed=SEED + 7)
    assert same.noise_seed == SEED
    twice = (same._d - 2.0 * clean.like._d).cpu().numpy()
    assert np.max(np.abs(twice - 0.5 * x)[live]) <= 4.0 * TOL
    # no seed: one from the OS, stored
    drawn = again(None)
    assert isinstance(drawn.noise_seed, int) and 0 <= drawn.noise_seed < 2 ** 63


def test_dt_only_likelihood_takes_noise():
    """A dt grid takes the noise too (its get_ll stays outside the FD path)."""
    from emri_frequencydomainwaveforms_amd.fdutils import get_sensitivity
    from emri_frequencydomainwaveforms_amd.likelihood import Likelihood
    n, dt = 1000, 10.0
    tm = lambda *a, **k: [np.zeros(n), np.zeros(n)]   # noqa: E731
    lk = Likelihood(tm, 2, dt=dt, use_gpu=True)
    lk.inject_signal(data_stream=[np.zeros(n), np.zeros(n)], noise_fn=[get_sensitivity] * 2,
                     noise_kwargs=[{}, {}], add_noise=True, noise_seed=SEED)
    nb = n // 2 + 1
    live = (torch.isfinite(lk._w) & (lk._w != 0.0)).cpu().numpy()
    d = lk._d.cpu().numpy()
    assert d.shape == (2, nb) and live.sum() >= 2 * (nb - 1)
    assert np.max(np.abs(d - 0.5 * nr.xi(SEED, 0, 2, nb))[live]) <= TOL
    with pytest.raises(NotImplementedError):
        lk.get_ll(np.zeros((1, 1)))


def test_branch_fused_and_per_walker(setups):
    _, s = setups
    fused = _check_branch(s)
    s.like.fused_likelihood = False
    try:
        plain = _check_branch(s)
    finally:
        s.like.fused_likelihood = True
    assert np.all(np.abs(fused - plain) <= 1e-10 * np.abs(fused))


@pytest.mark.parametrize("extra", [dict(upstream="device"), dict(window="hann"),
                                   dict(window="blackman"), dict(template="td")],
                         ids=["device-upstream", "hann", "blackman", "td"])
def test_branch(extra):
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(**SMALL, add_noise=True, noise_seed=SEED, **extra)
    _check_branch(s, route=extra if "upstream" in extra else None)


# ---- the scatter the Fisher matrix predicts ----------------------------------------------------
def test_noise_scatter(setups):
    from emri_frequencydomainwaveforms_amd import pe
    s, _ = setups
    R = 2048
    steps = np.where(s.truth6 != 0.0, 1e-6 * np.abs(s.truth6), 1e-6)
    dtheta, scov, agreement, info = pe.noise_scatter(s, steps, num_draws=R, seed=SEED)
    F, cov, over = info["fisher"], info["cov"], info["overlaps"]
    assert dtheta.shape == (R, 6) and scov.shape == (6, 6) and over.shape == (R, 6)
    # the overlaps' sample covariance estimates F, each entry with the Wishart standard error
    se = np.sqrt((np.outer(np.diag(F), np.diag(F)) + F ** 2) / R)
    z = np.abs(np.cov(over, rowvar=False) - F) / se
    print("worst |C_overlaps - F| / se:", z.max())
    assert z.max() <= 5.0
    # and the shifts' the covariance, with the same formula on cov
    sec = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / R)
    zc = np.abs(scov - cov) / sec
    sd = np.sqrt(np.diag(cov))
    print("worst |C_shifts - cov| / se:", zc.max(), " reported agreement:", agreement)
    assert zc.max() <= 5.0
    assert agreement == float(np.max(np.abs(scov - cov) / np.outer(sd, sd)))
    # draw 0 from explicit noise in numpy
    dh = info["derivs"].cpu().numpy()
    gain = np.sqrt(4.0 * info["weights"].cpu().numpy())
    x = nr.xi(SEED, 0, 2, dh.shape[2])
    o0 = np.sum(gain[None] * (x.real[None] * dh.real + x.imag[None] * dh.imag), axis=(1, 2))
    want = cov @ o0
    print("draw 0: |dtheta - cov @ overlaps| / |.|:", np.abs(dtheta[0] - want) / np.abs(want))
    assert np.all(np.abs(dtheta[0] - want) <= 1e-9 * np.abs(want))
