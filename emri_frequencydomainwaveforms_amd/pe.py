"""emri_pe.py-shaped likelihood setup (BASELINE.json configs 4 and 5) on the MI355X path.

Mirrors run_emri_pe's preamble (emri_pe.py:125-450) with this package's drop-ins:
  source and fixed angles                     emri_pe.py:590-635 (p0 re-solved for 0.99 Tobs)
  sampled 6-vector, fill_dict, transforms     :161-206 (TransformContainer, transform_mass_ratio)
  FD injection [h+, hx] over f >= 0           :203, 238-241, 276 (get_fd_waveform_fromFD)
  downsampled grid to 1.01 x the last non-zero bin, len/downsample points   :322-364
  Likelihood(..., subset=24) + inject_signal with LISA_Alloc_Sh noise         :381-417
  walker start multivariate_normal(truth, cov(covariance.npy) / (2.4 ndim))   :437-444
The covariance is shipped as data (data/walker_cov.npy, from tools/make_walker_cov.py). The
start uses numpy's Generator seeded with the reference's SEED = 2601996 (emri_pe.py:65), so the
walkers are reproducible, not the reference's own draws. One Eryn red-blue half-step evaluates
ntemps * nwalkers / 2 walkers in one Likelihood call (red_blue.py:149-156, ensemble.py:1283-1318).
"""

import os
from dataclasses import dataclass, field

import numpy as np

from .transforms import TransformContainer, transform_mass_ratio

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)
SEED = 2601996
FILL_INDS = np.array([2, 5, 6, 7, 8, 9, 10, 12])
_COV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "walker_cov.npy")


@dataclass
class PESetup:
    few: object              # the template's GenerateEMRIWaveform(..., return_list=True)
    gen: object              # get_fd_waveform_fromFD (or, template="td", _fromTD) template
    like: object             # Likelihood with the "emri" TransformContainer
    transform: object
    truth14: np.ndarray      # injection parameters (14, FEW order)
    truth6: np.ndarray       # sampled coordinates of the injection
    start: np.ndarray        # [ntemps * nwalkers, 6] walker start
    kwargs: dict             # waveform kwargs of every likelihood call (T, dt, eps[, f_arr])
    f_like: np.ndarray       # the likelihood's frequencies (f >= 0 of the template grid)
    half_step: int           # walkers per Likelihood call (ntemps * nwalkers / 2)
    info: dict = field(default_factory=dict)
    marg: object = None      # setup(marginalize=...): likelihood.ProfiledLikelihood around `like`

    def half_steps(self):
        """The start's walker batches, one per red-blue half-step."""
        B = self.half_step
        return [self.start[i:i + B] for i in range(0, len(self.start), B)]


def setup(Tobs=2.0, dt=10.0, eps=1e-2, M=1e6, mu=10.0, e0=0.35, downsample=None, nwalkers=16,
          ntemps=1, seed=SEED, caustic="uniform", subset=24, window_flag=False, freeze_gc=True,
          window=None, start_cov=None, template="fd", injectFD=None, upstream="host",
          mode_selector_kwargs=None, trajectory="host", marginalize=None,
          dist_range=(0.1, 10.0), add_noise=False, noise_seed=None):
    """template: "fd" (get_fd_waveform_fromFD around the FD generator) or "td" (the DFT of the TD
    generator's waveform, get_fd_waveform_fromTD: emri_pe.py -template td, :250-305); "td" does
    not go with downsample (:325-326). For "td", window may also be a 1-D array of the grid's
    length (the window is applied in the time domain, so any window will do).
    injectFD: None injects the template's own model; True / False force the FD / TD model for
    the data (the driver's -injectFD: its cross-model runs, :308-311).
    start_cov: a 6 x 6 covariance of the sampled coordinates for the walker start (e.g.
    fisher_covariance's, which belongs to this source), used in place of the shipped
    walker_cov.npy (the reference's chain covariance of its own source) before the same
    / (2.4 ndim) scaling; None keeps the shipped matrix.
    window_flag: the templates and the injection convolved with a Hann window of the grid's
    length (emri_pe.py:259-263, -window_flag 1 in test.sh: scipy.signal.windows.hann(N), N the
    TD/FD length, odd_len); not with downsampling (emri_pe.py:330-331).
    window: the same with another of scipy's symmetric cosine-sum windows, by name ("hann",
    "hamming", "blackman", "nuttall", "blackmanharris": fdutils.COSINE_WINDOWS, the windows
    check_mode_by_mode.py:269-272 uses and imports); window_flag=True alone means "hann".
    freeze_gc: collect, then move every object alive after the setup (torch's and scipy's
    modules, the likelihood, its grids) out of the cyclic collector's reach (gc.freeze), as a
    sampler process would once its setup is done: a full collection otherwise walks ~200 k
    objects, 35 ms (130 ms with a dropped setup's garbage), inside whichever likelihood call
    happens to trigger it (tools/api_trace.py, tools/gc_cycles.py).
    upstream: "host" (default) or "device": the likelihood's walkers take their amplitudes and
    mode selection on the device (Likelihood.device_upstream; only the trajectories stay on the
    host), where the template can pipeline on a symmetric grid. The injection is the same.
    trajectory: "host" (default) or "device" (with upstream="device" only): the walkers'
    trajectories are integrated on the device as well, all of a likelihood call's in one launch
    (Likelihood.device_trajectory; efd_traj_batch). The injection is the same.
    mode_selector_kwargs: passed to both generators, e.g. dict(sensitivity_fn=get_sensitivity)
    for the noise-weighted mode selection (amplitude.ModeSelector).
    marginalize: None, "amplitude" or "distance": PESetup.marg is then a
    likelihood.ProfiledLikelihood around `like` (the logL maximised over the template's overall
    amplitude, or marginalised over the distance on dist_range = (lo, hi) Gpc with a D^2 prior),
    a log-likelihood function of the same sampled coordinates in which the fixed distance of the
    templates is only the reference. `like` and the rest of the setup do not change.
    add_noise, noise_seed: Likelihood.inject_signal's: one stationary noise realisation added to
    the weighted data on the device, reproducible from info["noise_seed"] (None without noise;
    noise_seed=None draws a seed from the OS)."""
    if marginalize not in (None, "amplitude", "distance"):
        raise ValueError("marginalize: None, 'amplitude' or 'distance'")
    if template not in ("fd", "td"):
        raise ValueError("template: 'fd' or 'td'")
    from .waveform import GenerateEMRIWaveform, _check_trajectory, _check_upstream
    _check_upstream(upstream, {})
    if upstream == "device" and template != "fd":
        raise ValueError("upstream='device' is the FD template's")
    _check_trajectory(trajectory, upstream)
    if template == "td" and downsample:
        raise ValueError("Cannot run downsampling with time domain template")   # emri_pe.py:326
    from .fdutils import get_fd_waveform_fromFD, get_fd_waveform_fromTD, get_sensitivity
    from .likelihood import Likelihood
    from .trajectory import EMRIInspiral, get_p_at_t
    if start_cov is not None and np.shape(start_cov) != (6, 6):
        raise ValueError(f"start_cov must be 6 x 6, got {np.shape(start_cov)}")

    a, x0, Phi_theta0 = 0.1, 1.0, 0.0           # a, x0 ignored for Schwarzschild (:598, :602)
    qK = phiK = qS = phiS = np.pi / 3
    dist = 2.4539054256
    Phi_phi0 = Phi_r0 = np.pi / 3
    p0 = float(get_p_at_t(EMRIInspiral(), Tobs * 0.99, [M, mu, 0.0, e0, 1.0]))
    truth14 = np.array([M, mu, a, p0, e0, x0, dist, qS, phiS, qK, phiK, Phi_phi0, Phi_theta0,
                        Phi_r0], dtype=np.float64)
    fill = {"ndim_full": 14, "fill_values": np.array([0.0, x0, dist, qS, phiS, qK, phiK,
                                                      Phi_theta0]),
            "fill_inds": FILL_INDS.copy()}
    tc = TransformContainer({(0, 1): transform_mass_ratio}, fill)
    truth6 = np.delete(truth14.copy(), FILL_INDS)
    truth6[1] = np.log(truth6[1] / truth6[0])
    truth6[0] = np.log(truth6[0])
    injection = tc.both_transforms(truth6[None, :])[0]

    few = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW,
                               use_gpu=True, return_list=True, caustic=caustic,
                               mode_selector_kwargs=mode_selector_kwargs)
    kw = dict(T=Tobs, dt=dt, eps=eps)
    sig = few(*injection, mask_positive=True, **kw)
    frequency = few.waveform_generator.create_waveform.frequency
    frequency = frequency.cpu().numpy() if hasattr(frequency, "detach") else np.asarray(frequency)
    pos = frequency >= 0.0
    info = {"p0": p0, "N_f": int(len(frequency))}
    like_subset = subset
    window_name = window if window is not None else ("hann" if window_flag else None)
    window = None
    if template == "td" and window_name is not None and not isinstance(window_name, str):
        window = np.asarray(window_name, dtype=np.float64)
        if window.ndim != 1 or len(window) != len(frequency):
            raise ValueError(f"window: a name or a 1-D array of {len(frequency)} samples")
        info["window"] = "array"
    elif window_name is not None:
        from .fdutils import COSINE_WINDOWS
        if not isinstance(window_name, str) or window_name not in COSINE_WINDOWS:
            raise ValueError(f"window: one of {sorted(COSINE_WINDOWS)}")
        if downsample:
            raise ValueError("Cannot run downsampling with windowing")   # emri_pe.py:331
        import scipy.signal.windows as windows
        window = getattr(windows, window_name)(len(frequency))
        info["window"] = window_name
    if downsample:
        fixed = frequency[pos]
        nz = np.abs(sig[0].cpu().numpy()) > 1e-50                    # emri_pe.py:245
        num = int(nz.sum() / downsample)
        p_freq = np.linspace(0.0, fixed[nz].max() * 1.01, num=num)
        newfreq = np.hstack((-p_freq[::-1][:-1], p_freq))
        kw["f_arr"] = newfreq
        pos = newfreq >= 0.0
        f_like = newfreq[pos]
        like_subset = None                                           # like_ds (:366-374)
        info.update(downsample=downsample, N_f_downsampled=int(len(newfreq)))
    else:
        f_like = frequency[pos]
    inject_fd = template == "fd" if injectFD is None else bool(injectFD)
    gen = gen_fd = None
    if template == "fd" or inject_fd:
        gen = gen_fd = get_fd_waveform_fromFD(few, pos, dt, window=window)
    if template == "td" or not inject_fd:
        # the TD generator (td_gen_list, emri_pe.py:95-110) and its DFT template (:262, :266)
        td = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                                  sum_kwargs=dict(pad_output=True, odd_len=True), use_gpu=True,
                                  return_list=True, mode_selector_kwargs=mode_selector_kwargs)
        gen_td = get_fd_waveform_fromTD(td, pos, dt, window=window)
        if template == "td":
            gen, few = gen_td, td
    info.update(template=template, injectFD=bool(inject_fd))
    like = Likelihood(gen, 2, parameter_transforms={"emri": tc}, vectorized=False,
                      transpose_params=False, subset=like_subset, f_arr=f_like, use_gpu=True)
    if upstream == "device":
        like.device_upstream = True
        like.device_trajectory = trajectory == "device"
    info["upstream"] = upstream
    info["trajectory"] = trajectory
    data = (gen_fd if inject_fd else gen_td)(*injection, **kw)
    like.inject_signal(data_stream=data, noise_fn=[get_sensitivity, get_sensitivity],
                       noise_kwargs=[{}, {}], add_noise=add_noise, noise_seed=noise_seed)
    info["noise_seed"] = like.noise_seed if like.noise_has_been_added else None
    if start_cov is None:
        cov = np.load(_COV, allow_pickle=False) / (2.4 * 6)
    else:
        cov = np.asarray(start_cov, dtype=np.float64) / (2.4 * 6)
    rng = np.random.default_rng(seed)
    start = rng.multivariate_normal(truth6, cov, size=nwalkers * ntemps)
    if freeze_gc:
        import gc
        gc.collect()
        gc.freeze()
    marg = None
    if marginalize is not None:
        from .likelihood import ProfiledLikelihood
        marg = ProfiledLikelihood(like, marginalize, dist_ref=dist, dist_range=dist_range)
    return PESetup(few=few, gen=gen, like=like, transform=tc, truth14=injection,
                   truth6=truth6, start=start, kwargs=kw, f_like=f_like,
                   half_step=max(1, nwalkers * ntemps // 2), info=info, marg=marg)


class _SampledToWaveform:
    """fisher()'s parameter_transforms for a PESetup: a sampled 6-vector to FEW's 14."""

    def __init__(self, tc):
        self.tc = tc

    def transform_base_parameters(self, params):
        return self.tc.both_transforms(np.asarray(params, dtype=np.float64)[None, :])[0]


def fisher_covariance(s, eps, accuracy=True, waveform_model=None, return_derivs=False):
    """Fisher matrix and covariance of a PESetup's source in its six sampled coordinates at
    s.truth6, on the likelihood's grid and noise (s.f_like, the drivers' LISA_Alloc_Sh table):
    (F, cov, info). eps: the six steps (or one float). The stencil points go through
    s.transform.both_transforms to the generator's 14 parameters; waveform_model defaults to
    s.gen, whose rows come from one batched call (diagnostic.fisher_rows).
    info["stencil_agreement"] = max |F5 - F3| / sqrt(F5_ii F5_jj) with F3 the three-point matrix
    from the +-eps rows already in the five-point buffer (a second Gram call, no new
    waveforms): the step-size sanity number (accuracy=True only). info["derivs"] holds the
    derivatives (device, [6][2][nbin]) with return_derivs."""
    from . import diagnostic as dg
    torch = dg.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    model = s.gen if waveform_model is None else waveform_model
    steps, points, npoint = dg._fisher_points(s.truth6, eps, None, _SampledToWaveform(s.transform),
                                              accuracy)
    rows, _ = dg.fisher_rows(model, points, s.kwargs, extra_rows=6 if return_derivs else 0)
    rows = rows.to(torch.complex128)
    nchan, nbin = int(rows.shape[1]), int(rows.shape[2])
    # the likelihood's own grid and per-channel PSD; the bins it drops (f = 0, where its noise
    # factor is NaN) carry no weight here either
    with np.errstate(divide="ignore", invalid="ignore"):
        w = torch.stack([dg.fisher_weights(nbin, f_arr=s.like.freqs,
                                           PSD=np.asarray(p, dtype=np.float64))
                         for p in s.like.psd])
    w = torch.where(s.like._w > 0.0, w, torch.zeros_like(w)).contiguous()
    red = dg._reducer(dev)
    dh = (torch.empty((6, nchan, nbin), dtype=torch.complex128, device=dev)
          if return_derivs else None)
    gram = red.fisher_gram(rows, dg.stencil_coefficients(steps, accuracy), w, npoint, dh=dh)
    info = {"steps": steps, "npoint": npoint, "weights": w}
    if accuracy:
        c3 = np.zeros((6, 4))
        c3[:, 1:3] = dg.stencil_coefficients(steps, False)
        both = torch.stack([gram, red.fisher_gram(rows, c3, w, 4)]).cpu().numpy()
        F, F3 = both[0], both[1]
        d = np.sqrt(np.diag(F))
        info["fisher_three_point"] = F3
        info["stencil_agreement"] = float(np.max(np.abs(F - F3) / np.outer(d, d)))
    else:
        F = gram.cpu().numpy()
    if return_derivs:
        info["derivs"] = dh
    return F, dg.covariance(fish=F), info


def vallisneri_check(s, eps, num_samples=100, seed=None, accuracy=True, waveform_model=None):
    """Vallisneri's test of fisher_covariance's matrix for a PESetup's source (lisatools
    vallisneri_criterion_cdf, diagnostic.py:686-757, in the six sampled coordinates and with
    fisher_covariance's weights: the likelihood's grid and PSD, no weight on the bins it drops):
    (r_at_90, ratios, mismatches, info). num_samples directions on the 1-sigma ellipsoid, each
    moved point through s.transform to the generator's 14 parameters (polar angles wrapped as the
    reference does, :597-604), all waveforms from one batched call (diagnostic.fisher_rows) and
    one efd_overlap_rows pass against the waveform at s.truth6. ratios = |log r| per sample,
    r_at_90 their CDF's 90th percentile, mismatches = (1 - overlap) / 2. seed: seeds NumPy's
    global stream for the draws and puts its state back afterwards; None draws from the stream as
    it stands. info: "fisher", "cov", "offsets" (the drawn parameter offsets [n][6]), "points",
    "overlaps", "stencil_agreement" (accuracy=True), "h_true" and "weights" (device).
    eps: fisher_covariance's steps, named as in lisatools."""
    from . import diagnostic as dg
    model = s.gen if waveform_model is None else waveform_model
    F, cov, finfo = fisher_covariance(s, eps, accuracy=accuracy, waveform_model=model)
    tr = _SampledToWaveform(s.transform)
    state = np.random.get_state() if seed is not None else None
    if seed is not None:
        np.random.seed(seed)
    try:
        deltas = dg._ellipsoid_offsets(num_samples, F, np.linalg.eig(F))
    finally:
        if state is not None:
            np.random.set_state(state)
    points = [dg._perturbed_point(s.truth6, dl, range(6), tr) for dl in deltas]
    res, info = dg.sample_overlaps(model, tr.transform_base_parameters(s.truth6), points,
                                   s.kwargs, weights=finfo["weights"])
    mism, ratio, over = dg._criterion(res, deltas, F)
    ratios = np.abs(np.log(ratio))
    quantiles, counts = np.unique(ratios, return_counts=True)
    r_at_90 = float(np.interp(0.9, np.cumsum(counts).astype(np.double) / ratios.size, quantiles))
    info.update(fisher=F, cov=cov, offsets=deltas, points=np.asarray(points), overlaps=over)
    if "stencil_agreement" in finfo:
        info["stencil_agreement"] = finfo["stencil_agreement"]
    return r_at_90, ratios, mism, info


def systematic_bias(s, eps, approx_kwargs=None, approx_model=None, accuracy=True):
    """Cutler-Vallisneri bias of an approximate template for a PESetup's source (lisatools
    cutler_vallisneri_bias, diagnostic.py:760-840, in the six sampled coordinates with
    fisher_covariance's weights): (syst_vec, bias, info), syst_vec[k] = <dh_k | h_true -
    h_approx> from one efd_overlap_rows pass over fisher_covariance's derivatives (the difference
    is formed inside the kernel), bias = cov @ syst_vec, info["bias_sigma"] = bias / sqrt(diag
    cov); info also holds "fisher", "cov" and "stencil_agreement" (accuracy=True).
    The approximate template at the true parameters: approx_model (any callable on the same grid,
    e.g. the generator of a template="td" setup; default s.gen) called with s.kwargs overridden
    by approx_kwargs (e.g. a coarser mode threshold, or another setting that keeps f_arr).
    eps is fisher_covariance's step argument, named as in lisatools; the waveform keyword of the
    same name (the mode-selection threshold) is reachable only through
    approx_kwargs={"eps": ...}."""
    from . import diagnostic as dg
    torch = dg.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    F, cov, finfo = fisher_covariance(s, eps, accuracy=accuracy, return_derivs=True)
    p14 = _SampledToWaveform(s.transform).transform_base_parameters(s.truth6)
    t, _ = dg.fisher_rows(s.gen, [p14], s.kwargs)
    u, _ = dg.fisher_rows(s.gen if approx_model is None else approx_model, [p14],
                          {**s.kwargs, **(approx_kwargs or {})})
    dh = finfo["derivs"]
    if tuple(u.shape) != tuple(t.shape):
        raise ValueError(f"systematic_bias: the approximate template has shape "
                         f"{tuple(u.shape[1:])}, the true one {tuple(t.shape[1:])}")
    out, _ = dg._reducer(dev).overlap_rows(dh, t[0].to(torch.complex128).contiguous(),
                                           u[0].to(torch.complex128).contiguous(),
                                           finfo["weights"])
    syst_vec = out[:, 0].cpu().numpy()
    bias = cov @ syst_vec
    info = {"fisher": F, "cov": cov, "bias_sigma": bias / np.sqrt(np.diag(cov)),
            "weights": finfo["weights"]}
    if "stencil_agreement" in finfo:
        info["stencil_agreement"] = finfo["stencil_agreement"]
    return syst_vec, bias, info


def noise_scatter(s, eps, num_draws=1024, seed=SEED, accuracy=True, real0=0):
    """The scatter the Fisher covariance predicts, from explicit noise draws: for num_draws
    realisations n_r of the likelihood's noise (the generator of Likelihood.inject_signal's
    add_noise, keyed on seed; realisations real0 ...) the linearised maximum-likelihood shifts
    dtheta_r = cov <n_r | dh> in the six sampled coordinates. fisher_covariance's derivatives and
    weights w = df / S go through diagnostic.noise_overlaps with gain = sqrt(4 w) (the Fisher
    matrix is 4 sum w Re(conj dh_i dh_j)): one pass per draw block that regenerates the noise in
    registers, no noise buffer.
    Returns (dtheta [num_draws][6], sample_cov [6][6], agreement, info) with agreement =
    max_ij |sample_cov - cov|_ij / sqrt(cov_ii cov_jj); info holds "fisher", "cov", "overlaps"
    ([num_draws][6], host), "derivs" and "weights" (device) and, with accuracy,
    "stencil_agreement". The sample covariance of <n_r | dh> itself estimates the Fisher
    matrix, each entry with the Wishart standard error sqrt((F_ii F_jj + F_ij^2) / num_draws)."""
    from . import diagnostic as dg
    F, cov, finfo = fisher_covariance(s, eps, accuracy=accuracy, return_derivs=True)
    gain = (4.0 * finfo["weights"]).sqrt().contiguous()
    over = dg.noise_overlaps(finfo["derivs"], gain, seed, num_draws, real0=real0).cpu().numpy()
    dtheta = over @ cov.T
    sample_cov = np.cov(dtheta, rowvar=False) if num_draws > 1 else np.full((6, 6), np.nan)
    sd = np.sqrt(np.diag(cov))
    info = {"fisher": F, "cov": cov, "overlaps": over, "derivs": finfo["derivs"],
            "weights": finfo["weights"]}
    if "stencil_agreement" in finfo:
        info["stencil_agreement"] = finfo["stencil_agreement"]
    return dtheta, sample_cov, float(np.max(np.abs(sample_cov - cov) / np.outer(sd, sd))), info


class MemoizedUpstream:
    """Memoise a generator's host upstream (trajectory, amplitudes, Ylm, mode selection: the
    stand-ins of trajectory.py / amplitude.py) per parameter set, so repeated likelihood calls on
    the same walkers time the device path alone ("inputs resident"). Installed on the instance;
    `remove()` restores it. Arrays in kwargs (f_arr) are keyed by identity."""

    def __init__(self, wg):
        import time
        self._time = time.perf_counter
        self.wg = wg
        self.orig = wg.prepare
        self.memo = {}
        self.host_s = 0.0
        wg.prepare = self
        if hasattr(wg, "prefetch"):
            wg.prefetch = lambda calls, wait=True, concurrency=None: 0   # the memo holds it

    def __call__(self, *args, **kwargs):
        # submit_batch calls positionally with plain floats (and None / bool flags): the args
        # tuple is the key, as prepare()'s own prefetch lookup keys on them
        key = args if not kwargs else (
            tuple(float(a) if isinstance(a, (float, int, np.floating)) else a for a in args),
            tuple(sorted((k, ("id", id(v)) if hasattr(v, "shape") else v)
                         for k, v in kwargs.items())))
        hit = self.memo.get(key)
        if hit is None:
            t0 = self._time()
            hit = self.memo[key] = self.orig(*args, **kwargs)
            self.host_s += self._time() - t0
        return hit

    def remove(self):
        for name in ("prepare", "prefetch"):
            if name in self.wg.__dict__:
                delattr(self.wg, name)   # back to the class's methods
