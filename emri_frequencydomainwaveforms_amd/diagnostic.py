"""lisatools-compatible inner products on the device (LISAanalysistools/lisatools/diagnostic.py).

    inner_product(sig1, sig2, dt=None, df=None, f_arr=None, PSD="lisasens", PSD_args=(),
                  PSD_kwargs={}, normalize=False, use_gpu=False, complex=False)   :14-157
    snr(sig1, *args, data=None, use_gpu=False, **kwargs)                         :160-171
    pair_statistics(sig1_rows, sig2_rows, dt=None, df=None, f_arr=None, PSD="lisasens",
                    PSD_args=(), PSD_kwargs={})     many pairs' SNR, overlap, mismatch and logL of
                    the difference from one pass (efd_pair_stats; check_mode_by_mode.py:292-326)

Same arguments, rules and errors as the reference:
  - signals are one channel or a list of channels (equal counts, else ValueError);
  - dt: time-domain signals, rfft * dt with the DC bin dropped (:57-73);
  - df: frequencies (arange(N) + 1) * df (:79-80); f_arr: the given grid (:82-83);
  - PSD: an array (the drivers' usage, emri_pe.py:281-292), or a string naming a sensitivity
    function: "cornish_lisa_psd" (the notebooks' mismatch weighting, sensitivity.py) or
    "LISA_Alloc_Sh" / "lisa_alloc" (the drivers' table, FDutils.py:4-5); other lisatools curves
    raise NotImplementedError;
    PSD=None raises TypeError exactly like the reference (len() of a float at :97);
  - right-sum rule: x = diff(f) with the first spacing repeated (:97-100); out = 4 sum
    Re(conj(a) b) / PSD * x, or the complex sum with complex=True (:103-110);
  - normalize: True -> / sqrt(<a,a><b,b>); "sig1"/"sig2" -> / <s,s> (:112-154).
Further down: fisher / covariance / dh_dlambda / get_eigens (:189-451, 647-683) over
efd_fisher_gram, and mismatch_criterion / vallisneri_criterion_cdf / cutler_vallisneri_bias /
scale_snr (:489-644, 686-757, 760-840, 843-855) over efd_overlap_rows; see their section comments.
The reduction runs in libemrifd.so (efd_inner_product); the weights x/PSD are formed once per
call on the device. Inputs may be numpy arrays or torch tensors; the result is a Python float
(complex with complex=True), like the reference's numpy scalar.
"""

import numpy as np

from .summation import require_gpu

_REDUCERS = {}


def _reducer(device):
    from .reductions import Reducer
    key = str(device)
    if key not in _REDUCERS:
        _REDUCERS[key] = Reducer(device)
    return _REDUCERS[key]


def noise_overlaps(rows, gain, seed, num_draws, real0=0):
    """<n_r | rows_p> for num_draws noise draws r = real0 ... and every row p, as a float64
    [num_draws][nrow] device tensor (Reducer.noise_overlap_rows, efd_noise_overlap_rows): sum_c
    sum_k gain[c][k] Re(conj xi_r(c, k) rows[p][c][k]) with the noise regenerated in registers,
    never written. rows: complex128 [nrow][nchan][nbin] on the device (at most
    EFD_NOISE_MAX_ROWS rows, e.g. fisher's derivatives); gain: float64 [nchan][nbin], sqrt(4 df /
    S) = sqrt(4 fisher_weights) for the likelihood's noise, or None (= 1). The covariance of the
    result over the draws is then the rows' Fisher matrix 4 sum (df / S) Re(conj a b)."""
    torch = require_gpu()
    rows = rows.to(torch.complex128).contiguous()
    if gain is not None:
        gain = torch.as_tensor(gain, dtype=torch.float64, device=rows.device).contiguous()
    return _reducer(rows.device).noise_overlap_rows(rows, gain, seed, num_draws, real0=real0)


def _as_channels(sig, torch, device):
    if not isinstance(sig, list):
        sig = [sig]
    return [torch.as_tensor(s, device=device) for s in sig]


def _psd_array(PSD, freqs, PSD_args, PSD_kwargs, torch, device):
    if isinstance(PSD, str):
        fh = freqs.detach().cpu().numpy() if hasattr(freqs, "detach") else np.asarray(freqs)
        if PSD in ("LISA_Alloc_Sh", "lisa_alloc"):
            from .fdutils import get_sensitivity
            vals = get_sensitivity(fh, *PSD_args, **PSD_kwargs)
        else:   # lisatools' named curves (diagnostic.py:81-82): sensitivity.get_sensitivity
            from .sensitivity import get_sensitivity
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                vals = get_sensitivity(fh, PSD, *PSD_args, **PSD_kwargs)
        return torch.as_tensor(vals, device=device, dtype=torch.float64)
    if PSD is None:
        # the reference evaluates len(1.0) here (diagnostic.py:97) and fails the same way
        raise TypeError("object of type 'float' has no len()")
    if isinstance(PSD, (np.ndarray,)) or hasattr(PSD, "detach"):
        return torch.as_tensor(PSD, device=device, dtype=torch.float64)
    raise ValueError("PSD must be a string giving the sens_fn or a predetermimed array or None "
                     "if noise weighting is included in a signal.")


def _power_weight(freqs, nbin, PSD, PSD_args, PSD_kwargs, torch, dev):
    """x / PSD over one channel's nbin bins, x = diff(f) with the first spacing repeated
    (diagnostic.py:93-98): the weight of inner_product and pair_statistics."""
    psd = _psd_array(PSD, freqs, PSD_args, PSD_kwargs, torch, dev)
    x = torch.empty(nbin, dtype=torch.float64, device=dev)
    x[1:] = torch.diff(freqs)
    x[0] = x[1]
    return x / psd


def inner_product(sig1, sig2, dt=None, df=None, f_arr=None, PSD="lisasens", PSD_args=(),
                  PSD_kwargs={}, normalize=False, use_gpu=False, complex=False):
    torch = require_gpu()
    if df is None and dt is None and f_arr is None:
        raise ValueError("Must provide either df, dt or f_arr keyword arguments.")
    dev = torch.device("cuda", torch.cuda.current_device())
    s1 = _as_channels(sig1, torch, dev)
    s2 = _as_channels(sig2, torch, dev)
    if len(s1) != len(s2):
        raise ValueError("Signal 1 has {} channels. Signal 2 has {} channels. Must be "
                         "equal.".format(len(s1), len(s2)))
    if dt is not None:
        n = max(len(s1[0]), len(s2[0]))
        s1 = [torch.nn.functional.pad(s, (0, n - len(s))) for s in s1]
        s2 = [torch.nn.functional.pad(s, (0, n - len(s))) for s in s2]
        freqs = torch.fft.rfftfreq(n, dt, dtype=torch.float64, device=dev)[1:]
        f1 = [torch.fft.rfft(s.to(torch.float64))[1:] * dt for s in s1]
        f2 = [torch.fft.rfft(s.to(torch.float64))[1:] * dt for s in s2]
    else:
        f1 = [s.to(torch.complex128) for s in s1]
        f2 = [s.to(torch.complex128) for s in s2]
        if df is not None:
            freqs = (torch.arange(len(f1[0]), dtype=torch.float64, device=dev) + 1) * df
        else:
            freqs = torch.as_tensor(f_arr, dtype=torch.float64, device=dev)
    nbin = len(f1[0])
    w = _power_weight(freqs, nbin, PSD, PSD_args, PSD_kwargs, torch, dev)
    w = w.expand(len(f1), nbin).contiguous()
    a = torch.stack(f1).contiguous()
    b = torch.stack(f2).contiguous()
    val = _reducer(dev).inner(a, b, w).item()
    out = val if complex else val.real

    norm = 1.0
    kw = dict(dt=dt, df=df, f_arr=f_arr, PSD=PSD, PSD_args=PSD_args, PSD_kwargs=PSD_kwargs)
    if normalize is True:
        n1 = inner_product(sig1, sig1, use_gpu=use_gpu, normalize=False, **kw)
        n2 = inner_product(sig2, sig2, use_gpu=use_gpu, normalize=False, **kw)
        norm = np.sqrt(n1 * n2)
    elif isinstance(normalize, str):
        if normalize == "sig1":
            ref = sig1
        elif normalize == "sig2":
            ref = sig2
        else:
            raise ValueError("If normalizing with respect to sig1 or sig2, normalize kwarg must "
                             "either be 'sig1' or 'sig2'.")
        norm = inner_product(ref, ref, normalize=False, **kw)
    elif normalize is not False:
        raise ValueError("Normalize must be True, False, 'sig1', or 'sig2'.")
    return out / norm


class PairStatistics:
    """What the mode-by-mode driver derives for each (template 1, template 2) pair
    (check_mode_by_mode.py:292-326), as numpy arrays over the R pairs, from efd_pair_stats'
    numbers raw [R][nchan][5] = (aa, bb, abr, abi, dd):
      aa, bb, dd [R][nchan] and ab complex [R][nchan]: <1|1>, <2|2>, <1-2|1-2> and <1|2> per
        channel; aa_sum, bb_sum, dd_sum [R] and ab_sum complex [R]: summed over the channels;
      snr1 = sqrt(aa_sum), snr2 = sqrt(bb_sum)                              (:292)
      overlap = Re ab_sum / sqrt(aa_sum bb_sum), mismatch = |1 - overlap|   (:299-301)
      loglike = -1/2 dd_sum                                                 (:315-317)
    dd is the difference's own sum (formed per element), not aa + bb - 2 Re ab."""

    def __init__(self, raw):
        raw = np.asarray(raw, dtype=np.float64)
        self.raw = raw
        self.aa, self.bb, self.dd = raw[..., 0], raw[..., 1], raw[..., 4]
        self.ab = raw[..., 2] + 1j * raw[..., 3]
        self.aa_sum, self.bb_sum = self.aa.sum(axis=-1), self.bb.sum(axis=-1)
        self.ab_sum, self.dd_sum = self.ab.sum(axis=-1), self.dd.sum(axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.snr1, self.snr2 = np.sqrt(self.aa_sum), np.sqrt(self.bb_sum)
            self.overlap = self.ab_sum.real / np.sqrt(self.aa_sum * self.bb_sum)
        self.mismatch = np.abs(1.0 - self.overlap)
        self.loglike = -0.5 * self.dd_sum


def _as_rows(sig, torch, dev):
    """Rows of channels as one tensor [R][nchan][n]: a tensor as it is, a list of channel lists
    (or of single channels) stacked."""
    def row(r):
        if isinstance(r, (list, tuple)):
            return torch.stack(_as_channels(list(r), torch, dev))
        t = torch.as_tensor(r, device=dev)
        return t[None, :] if t.dim() == 1 else t

    if isinstance(sig, (list, tuple)):
        return torch.stack([row(r) for r in sig])
    t = torch.as_tensor(sig, device=dev)
    return t[:, None, :] if t.dim() == 2 else t


def pair_statistics(sig1_rows, sig2_rows, dt=None, df=None, f_arr=None, PSD="lisasens",
                    PSD_args=(), PSD_kwargs={}):
    """SNRs, normalised overlap, mismatch and the log-likelihood of the difference of R
    (signal 1, signal 2) pairs in one pass over each (efd_pair_stats): what the mode-by-mode
    driver takes from six to eight inner_product calls per pair (check_mode_by_mode.py:292-326).
    The rows are lists of channel lists, or tensors [R][nchan][nbin] (one or two channels); the
    frequency and PSD rules and errors are inner_product's, with one weight for all rows. Rows go
    in blocks of EFD_PAIR_MAX_ROWS and one host transfer brings everything back. Returns a
    PairStatistics."""
    torch = require_gpu()
    if df is None and dt is None and f_arr is None:
        raise ValueError("Must provide either df, dt or f_arr keyword arguments.")
    dev = torch.device("cuda", torch.cuda.current_device())
    a = _as_rows(sig1_rows, torch, dev)
    b = _as_rows(sig2_rows, torch, dev)
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0]:
        raise ValueError("pair_statistics: expected the same number of rows [R][nchan][n] on "
                         "both sides, got {} and {}".format(tuple(a.shape), tuple(b.shape)))
    if a.shape[1] != b.shape[1]:
        raise ValueError("Signal 1 has {} channels. Signal 2 has {} channels. Must be "
                         "equal.".format(a.shape[1], b.shape[1]))
    if dt is not None:
        n = max(a.shape[-1], b.shape[-1])
        a = torch.nn.functional.pad(a, (0, n - a.shape[-1]))
        b = torch.nn.functional.pad(b, (0, n - b.shape[-1]))
        freqs = torch.fft.rfftfreq(n, dt, dtype=torch.float64, device=dev)[1:]
        a = torch.fft.rfft(a.to(torch.float64))[..., 1:] * dt
        b = torch.fft.rfft(b.to(torch.float64))[..., 1:] * dt
    elif df is not None:
        freqs = (torch.arange(a.shape[-1], dtype=torch.float64, device=dev) + 1) * df
    else:
        freqs = torch.as_tensor(f_arr, dtype=torch.float64, device=dev)
    a = a.to(torch.complex128).contiguous()
    b = b.to(torch.complex128).contiguous()
    if a.shape != b.shape:
        raise ValueError("pair_statistics: the two sides' rows differ in length")
    w = _power_weight(freqs, int(a.shape[-1]), PSD, PSD_args, PSD_kwargs, torch, dev).contiguous()
    raw = _reducer(dev).pair_stats(a, b, w)
    return PairStatistics(raw.cpu().numpy())


def snr(sig1, *args, data=None, use_gpu=False, **kwargs):
    sig2 = sig1 if data is None else data
    return np.sqrt(inner_product(sig1, sig2, *args, use_gpu=use_gpu, **kwargs))


# ---------------------------------------------------------------------------------------------
# Fisher matrix and covariance (diagnostic.py:189-451, 647-683)
# ---------------------------------------------------------------------------------------------
# The reference forms dh_i per parameter from a central stencil (dh_dlambda, :263-267 / :294) and
# then fish[i][j] = inner_product([dh_i.real, dh_i.imag], [dh_j.real, dh_j.imag]) (:373-381),
# which for frequency-domain rows is 4 Re sum conj(dh_i) dh_j x / PSD over every leading
# dimension. Here the stencil points' waveforms sit in one device buffer [P npoint][nelem] and one
# efd_fisher_gram call forms the derivatives per element and all P (P + 1) / 2 products from
# them (reductions.Reducer.fisher_gram); one host transfer brings the matrix back.
# Kept from the reference: zip(deriv_inds, eps) pairs eps[k] with deriv_inds[k] BY POSITION
# (:354), a float eps is broadcast with np.full_like(params, eps) (:350-351). Widened on purpose:
# a model may return a list of channels (what get_fd_waveform_fromFD returns; the reference's
# dh_dlambda fails on a list's unary minus), which is stacked into [nchan][nbin].

# stencil offsets in units of eps and their weights times eps (dh_dlambda :263-267, :294)
_STENCILS = {True: ((2.0, 1.0, -1.0, -2.0), (-1.0 / 12, 8.0 / 12, -8.0 / 12, 1.0 / 12)),
             False: ((1.0, -1.0), (0.5, -0.5))}


def h_var_p_eps(waveform_model, params, step, i, parameter_transforms=None, waveform_kwargs={}):
    """The waveform with parameter i moved by `step` (diagnostic.py:189-204)."""
    params_p_eps = params.copy()
    params_p_eps[i] += step
    if parameter_transforms:
        params_p_eps = parameter_transforms.transform_base_parameters(params_p_eps)
    return waveform_model(*params_p_eps, **waveform_kwargs)


def _stack_channels(h, torch, dev):
    """A model's output as one tensor: an array as it is, a list of channels stacked."""
    if isinstance(h, (list, tuple)):
        return torch.stack([torch.as_tensor(c, device=dev) for c in h])
    return torch.as_tensor(h, device=dev)


def dh_dlambda(waveform_model, params, eps, i, parameter_transforms=None, waveform_kwargs={},
               accuracy=True):
    """Central-difference derivative of the waveform along parameter i (diagnostic.py:207-297):
    five-point (-h(+2e) + h(-2e) + 8 (h(+e) - h(-e))) / (12 e), or three-point
    (h(+e) - h(-e)) / (2 e) with accuracy=False, in the reference's association. A device
    tensor; fisher() does not go through here (its stencil runs inside efd_fisher_gram)."""
    torch = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = dict(waveform_kwargs=waveform_kwargs, parameter_transforms=parameter_transforms)

    def at(step):
        return _stack_channels(h_var_p_eps(waveform_model, params, step, i, **kw), torch, dev)

    if accuracy:
        up2, up1, dn2, dn1 = at(2 * eps), at(eps), at(-2 * eps), at(-eps)
        n = min(len(up2), len(up1), len(dn2), len(dn1))
        return (-up2[:n] + dn2[:n] + 8 * (up1[:n] - dn1[:n])) / (12 * eps)
    up1, dn1 = at(eps), at(-eps)
    n = min(len(up1), len(dn1))
    return (up1[:n] - dn1[:n]) / (2 * eps)


def _fisher_points(params, eps, deriv_inds, parameter_transforms, accuracy):
    """(steps [P], stencil parameter vectors [P npoint][...], npoint): row i npoint + s is the
    parameter vector at offset s of deriv_inds[i]'s stencil, transformed as h_var_p_eps does."""
    params = np.asarray(params, dtype=np.float64)
    if deriv_inds is None:
        deriv_inds = np.arange(len(params))
    if isinstance(eps, float):
        eps = np.full_like(params, eps)
    offsets = _STENCILS[bool(accuracy)][0]
    steps, points = [], []
    for i, eps_i in zip(deriv_inds, eps):   # positional pairing, as the reference's zip
        steps.append(float(eps_i))
        for o in offsets:
            p = params.copy()
            p[i] += o * eps_i
            if parameter_transforms:
                p = parameter_transforms.transform_base_parameters(p)
            points.append(np.asarray(p, dtype=np.float64))
    if not steps:
        raise ValueError("fisher: no parameters to differentiate")
    return np.asarray(steps), points, len(offsets)


def stencil_coefficients(steps, accuracy=True):
    """efd_fisher_gram's coef [P][npoint] for central differences with the given steps."""
    wts = np.asarray(_STENCILS[bool(accuracy)][1])
    return wts[None, :] / np.asarray(steps, dtype=np.float64)[:, None]


def _batched_model(waveform_model, points, waveform_kwargs):
    """The get_fd_waveform_fromFD whose stencil rows can come from one batched call, or None."""
    from .fdutils import get_fd_waveform_fromFD
    from .waveform import GenerateEMRIWaveform
    m = waveform_model
    if type(m) is not get_fd_waveform_fromFD or m._suffix_k0 is None:
        return None
    gen = m.waveform_generator
    if (not isinstance(gen, GenerateEMRIWaveform) or not gen.use_gpu
            or getattr(gen.waveform_generator, "output_type", None) != "fd"):
        return None
    if any(len(p) != 14 for p in points) or set(waveform_kwargs) - {"T", "dt", "eps", "f_arr"}:
        return None
    if m.window is not None and not m.can_fill_batch:
        return None
    return m


def _need_memory(nbytes, torch, dev, what):
    free = torch.cuda.mem_get_info(dev)[0]
    free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if nbytes > free:
        raise ValueError(f"fisher: {what} needs {nbytes} bytes of device memory, {free} are "
                         "free; use a coarser grid (f_arr) or fewer parameters (deriv_inds)")


def fisher_rows(waveform_model, points, waveform_kwargs={}, extra_rows=0):
    """The waveforms at the stencil points in one device buffer complex128 [len(points)][nchan]
    [nbin] (a 1-D model output counts as one channel; the second return value tells).
    Batched: a get_fd_waveform_fromFD over a GenerateEMRIWaveform FD generator fills all rows
    through generate_batch (unwindowed) or fill_batch (windowed), non_zero_mask applied as its
    __call__ does. Generic: any other callable, once per point, its array or list of channels
    stacked. extra_rows: complex rows of the same size the caller will allocate next (the
    derivatives), counted in the memory check."""
    torch = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(points)
    m = _batched_model(waveform_model, points, waveform_kwargs)
    if m is not None:
        gen = m.waveform_generator
        if m.window is None:
            kw = {k: waveform_kwargs[k] for k in ("T", "dt", "f_arr") if k in waveform_kwargs}
            if gen.positive_bins(**kw) != m.num_bins:
                raise ValueError("positive_frequency_mask does not match the generator's grid")
        _need_memory(16 * (B + extra_rows) * 2 * m.num_bins, torch, dev,
                     f"{B} stencil rows of 2 x {m.num_bins} bins")
        buf = torch.empty((B, 2, m.num_bins), dtype=torch.complex128, device=dev)
        P14 = np.asarray(points, dtype=np.float64)
        if m.window is None:
            gen.generate_batch(P14, buf, **waveform_kwargs)
        else:
            G = m.WINDOW_GROUP
            for g0 in range(0, B, G):
                m.fill_batch([buf[r] for r in range(g0, min(B, g0 + G))], P14[g0:g0 + G],
                             **waveform_kwargs)
        if m.non_zero_mask is not None:
            buf[:, :, ~m.non_zero_mask] = 0.0
        return buf, False
    buf, flat = None, False
    for r, p in enumerate(points):
        h = _stack_channels(waveform_model(*p, **waveform_kwargs), torch, dev)
        if buf is None:
            flat = h.dim() == 1
            shape = (1, h.shape[0]) if flat else tuple(h.shape)
            _need_memory(16 * (B + extra_rows) * int(h.numel()), torch, dev,
                         f"{B} stencil rows of {int(h.numel())} elements")
            dtype = torch.complex128 if h.is_complex() else torch.float64
            buf = torch.empty((B,) + shape, dtype=dtype, device=dev)
        if h.numel() != buf[r].numel():
            raise ValueError("fisher: the model's output changes shape between stencil points")
        buf[r].copy_(h.reshape(buf[r].shape))
    return buf, flat


def fisher_weights(nbin, n_td=None, dt=None, df=None, f_arr=None, PSD="lisasens", PSD_args=(),
                   PSD_kwargs={}, **other):
    """inner_product's weight x / PSD [nbin] on the device: the right-sum spacing x = diff(f)
    with the first spacing repeated (diagnostic.py:95-100), over rfftfreq(n_td, dt)[1:] (dt),
    (arange(nbin) + 1) df (df) or f_arr. normalize / complex are not Fisher options."""
    torch = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    if other.get("normalize", False) or other.get("complex", False):
        raise ValueError("fisher: inner_product_kwargs normalize / complex are not supported")
    if df is None and dt is None and f_arr is None:
        raise ValueError("Must provide either df, dt or f_arr keyword arguments.")
    if dt is not None:
        freqs = torch.fft.rfftfreq(n_td, dt, dtype=torch.float64, device=dev)[1:]
    elif df is not None:
        freqs = (torch.arange(nbin, dtype=torch.float64, device=dev) + 1) * df
    else:
        freqs = torch.as_tensor(f_arr, dtype=torch.float64, device=dev)
    psd = _psd_array(PSD, freqs, PSD_args, PSD_kwargs, torch, dev)
    x = torch.empty(nbin, dtype=torch.float64, device=dev)
    x[1:] = torch.diff(freqs)
    x[0] = x[1]
    return x / psd


def _kernel_rows(rows, inner_product_kwargs, torch):
    """(rows as the reduction kernels take them, complex128 [B][nchan][nbin]; n_td): with the dt
    form the rows are time-domain, their real and imaginary parts are the reference's channels,
    each rfft * dt with the DC bin dropped (diagnostic.py:57-73), and n_td is their length;
    otherwise the rows as they are and n_td = None."""
    dt_ = inner_product_kwargs.get("dt")
    if dt_ is None:
        return rows.to(torch.complex128), None
    parts = [rows.real, rows.imag] if rows.is_complex() else [rows]
    fd = torch.cat([torch.fft.rfft(p.to(torch.float64), dim=-1)[..., 1:] * dt_
                    for p in parts], dim=1).contiguous()
    return fd, rows.shape[-1]


def fisher(waveform_model, params, eps, use_gpu=False, deriv_inds=None,
           parameter_transforms=None, waveform_kwargs={}, inner_product_kwargs={},
           return_derivs=False, accuracy=True):
    """Fisher matrix of the parameters deriv_inds (all by default) as a numpy [P][P] array
    (diagnostic.py:300-386), and with return_derivs the derivatives as a device tensor
    [P][nchan][nbin] ([P][nbin] for a model that returns one 1-D array). See the section
    comment above for what is kept from the reference and what is widened."""
    torch = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    steps, points, npoint = _fisher_points(params, eps, deriv_inds, parameter_transforms,
                                           accuracy)
    P = len(steps)
    rows, flat = fisher_rows(waveform_model, points, waveform_kwargs,
                             extra_rows=P if return_derivs else 0)
    coef = stencil_coefficients(steps, accuracy)
    td = None
    if inner_product_kwargs.get("dt") is not None:
        td = rows
    rows, n_td = _kernel_rows(rows, inner_product_kwargs, torch)
    nchan, nbin = int(rows.shape[1]), int(rows.shape[2])
    w = fisher_weights(nbin, n_td=n_td, **inner_product_kwargs)
    w = w.expand(nchan, nbin).contiguous()
    dh = None
    if return_derivs and td is None:
        dh = torch.empty((P, nchan, nbin), dtype=torch.complex128, device=dev)
    gram = _reducer(dev).fisher_gram(rows, coef, w, npoint, dh=dh)
    fish = gram.cpu().numpy()
    if not return_derivs:
        return fish
    if td is not None:   # the reference returns the time-domain derivatives
        c = torch.as_tensor(coef, device=dev).to(td.dtype)
        dh = (td.reshape((P, npoint) + tuple(td.shape[1:])) * c[:, :, None, None]).sum(1)
    return fish, (dh[:, 0] if flat else dh)


def _mpmath(wanted, message):
    """mpmath set to 500 digits when `wanted` and importable, else None (the reference prints
    `message` and goes on in float64)."""
    if not wanted:
        return None
    try:
        import mpmath
    except ModuleNotFoundError:
        print(message)
        return None
    mpmath.mp.dps = 500
    return mpmath


def get_eigens(arr, high_precision=False):
    """Eigenvalues and right eigenvectors (evects[:, k] with evals[k]) of a Fisher or covariance
    matrix (diagnostic.py:647-683): numpy's eig, or mpmath's at 500 digits when asked for and
    importable."""
    mp = _mpmath(high_precision, "mpmath is not installed - using low-precision eigen "
                                 "decomposition.")
    if mp is None:
        return np.linalg.eig(arr)
    evals, _, right = mp.eig(mp.matrix(arr.tolist()), left=True, right=True)
    return np.array(evals, dtype=np.float64), np.array(right.tolist(), dtype=np.float64)


def covariance(*fisher_args, fish=None, diagonalize=False, return_fisher=False, precision=False,
               **fisher_kwargs):
    """Pseudo-inverse of the Fisher matrix (diagnostic.py:389-451): computed by fisher() unless
    `fish` is given; precision=True inverts through mpmath's SVD at 500 digits when mpmath is
    importable; diagonalize rotates into the eigenbasis (get_eigens). Returns cov, or the list
    [cov, fish (with return_fisher), dh (when fisher_kwargs names return_derivs)]."""
    if fish is None:
        fish = fisher(*fisher_args, **fisher_kwargs)
    # as the reference: the keyword's presence, not its value, says that fisher returned a pair
    with_derivs = "return_derivs" in fisher_kwargs
    if with_derivs:
        fish, dh = fish
    mp = _mpmath(precision, "mpmath module not installed. Defaulting to low precision...")
    if mp is None:
        cov = np.linalg.pinv(fish)
    else:
        U, sing, V = mp.svd_r(mp.matrix(fish.tolist()))
        pinv = V.T * mp.diag([1 / x for x in sing]) * U.T
        cov = np.array(pinv.tolist(), dtype=np.float64)
    if diagonalize:
        _, vecs = get_eigens(cov, high_precision=mp is not None)
        cov = vecs.T @ cov @ vecs
    out = [cov] + ([fish] if return_fisher else []) + ([dh] if with_derivs else [])
    return cov if len(out) == 1 else out


# ---------------------------------------------------------------------------------------------
# Vallisneri's mismatch criterion, its CDF, the Cutler-Vallisneri bias, scale_snr
# (diagnostic.py:489-644, 686-757, 760-840, 843-855)
# ---------------------------------------------------------------------------------------------
# The reference draws one direction on the Fisher ellipsoid per mismatch_criterion call, makes the
# perturbed waveform and takes three inner products of it with h_true (:622-638); the CDF loops
# over num_samples such calls (:731-741). Here all directions are drawn first (one
# np.random.normal(0, 1, d) per sample, in order: NumPy's global stream is consumed exactly as by
# the reference's loop, so a seeded run has the same directions), the perturbed waveforms sit in
# one device buffer (fisher_rows: one batched call where the model allows it), h_true is computed
# once, and one efd_overlap_rows pass (reductions.Reducer.overlap_rows) gives every sample's
# <h_k|h_true>, <h_k|h_k> and <h_true|h_true>; one host transfer brings them back. The bias
# vector <dh_k | h_true - h_approx> (:812-823) is the same pass over fisher's derivatives, the
# difference formed per element inside the kernel and never stored.
# Kept from the reference: the signatures and keywords, the polar-angle wrap on indices 7 and 9 of
# the TRANSFORMED vector with + pi on the azimuth beside it (:597-604; a transformed vector shorter
# than 11 fails with IndexError, as there), abs(log ratio), np.unique / cumsum / np.interp(0.9).
# Widened on purpose: a model may return a list of channels; parameter_transforms=None means
# identity (the reference fails on None); vallisneri_criterion_cdf takes eigens= too (the
# reference always recomputes them) and hands fisher's arguments given by keyword on to fisher;
# the rows held at once are bounded by the device memory that
# is free (_need_memory), larger sample counts go in blocks.


def _transformed(params, parameter_transforms):
    p = np.array(params, dtype=np.float64)
    if parameter_transforms:
        p = parameter_transforms.transform_base_parameters(p)
    return np.asarray(p, dtype=np.float64)


def _ellipsoid_offsets(num_samples, fish, eigens):
    """vec_delta [num_samples][d] of mismatch_criterion (:579-587): x uniform on the unit sphere,
    delta = sum_l x_l v[:, l] / sqrt(w_l), in the reference's order of operations."""
    w, v = eigens
    d = fish.shape[0]
    us = [np.random.normal(0, 1, d) for _ in range(num_samples)]   # all draws first, in order
    out = np.zeros((num_samples, d))
    for k, u in enumerate(us):
        x = u / np.sum(u ** 2) ** (0.5)
        for l in range(d):
            out[k] += x[l] * v[:, l] / np.sqrt(w[l])
    return out


def _perturbed_point(params, delta, deriv_inds, parameter_transforms):
    """The transformed parameters moved by delta along deriv_inds, polar angles wrapped and
    reflected (:590-604)."""
    var = np.array(params, dtype=np.float64)
    for i, ind in enumerate(deriv_inds):
        var[ind] = var[ind] + delta[i]
    var = _transformed(var, parameter_transforms).copy()
    for val in (7, 9):
        var[val] = var[val] % (2 * np.pi)
        if var[val] > np.pi:
            var[val] = 2 * np.pi - var[val]
            var[val + 1] += np.pi
    return var


def _free_bytes(torch, dev):
    return (torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev)
            - torch.cuda.memory_allocated(dev))


def _vallisneri(num_samples, waveform_model, params, deriv_inds=None, inner_product_kwargs={},
                waveform_kwargs={}, parameter_transforms=None, fish=None, eps=None, eigens=None,
                return_fish=False, fisher_kwargs={}):
    """mismatch_criterion's work for num_samples directions: (mism [n], ratio [n], fish, info)
    with info the offsets, perturbed points and overlaps. The signature after num_samples is
    mismatch_criterion's, so that its callers' arguments bind; return_fish is the caller's."""
    params = np.asarray(params, dtype=np.float64)
    if deriv_inds is None:
        deriv_inds = np.arange(len(params))
    if fish is None:
        if eps is None:
            raise ValueError("No numerical derivative step-sizes (eps) supplied for Fisher "
                             "matrix generation.")
        if isinstance(eps, float):
            eps = np.full_like(params, eps)
        fish = fisher(waveform_model=waveform_model, params=params, eps=eps,
                      deriv_inds=deriv_inds, parameter_transforms=parameter_transforms,
                      waveform_kwargs=waveform_kwargs,
                      inner_product_kwargs=inner_product_kwargs, **fisher_kwargs)
    fish = np.asarray(fish.get() if hasattr(fish, "get") else fish)
    if eigens is None:
        eigens = np.linalg.eig(fish)
    deltas = _ellipsoid_offsets(num_samples, fish, eigens)
    points = [_perturbed_point(params, dl, deriv_inds, parameter_transforms) for dl in deltas]
    res, info = sample_overlaps(waveform_model, _transformed(params, parameter_transforms),
                                points, waveform_kwargs, inner_product_kwargs)
    mism, ratio, over = _criterion(res, deltas, fish)
    info.update(offsets=deltas, points=np.asarray(points), overlaps=over)
    return mism, ratio, fish, info


def sample_overlaps(waveform_model, true_point, points, waveform_kwargs={},
                    inner_product_kwargs={}, weights=None):
    """efd_overlap_rows' numbers (host float64 [3 n + 1]: <h_k|h_true>, its imaginary partner and
    <h_k|h_k> per point, then <h_true|h_true>) for the model at the n (transformed) points
    against the model at true_point, and {"h_true", "weights"} (device). The waveforms come from
    fisher_rows in blocks that fit the free device memory, h_true is computed once, every block
    is one reduction pass and one host transfer brings all numbers back. weights: the kernel's
    w as a device tensor [nchan][nbin], or None for inner_product's x / PSD from
    inner_product_kwargs (fisher_weights)."""
    torch = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    red = _reducer(dev)
    n = len(points)
    t, _ = fisher_rows(waveform_model, [true_point], waveform_kwargs)   # (its own memory check)
    row_bytes = 16 * int(t[0].numel())
    t, n_td = _kernel_rows(t, inner_product_kwargs, torch)
    nchan, nbin = int(t.shape[1]), int(t.shape[2])
    if weights is None:
        w = fisher_weights(nbin, n_td=n_td, **inner_product_kwargs)
        w = w.expand(nchan, nbin).contiguous()
    else:
        w = weights
    t = t[0].contiguous()
    # rows held at once: a time-domain block also holds its transform
    per_row = row_bytes * (1 if n_td is None else 3)
    block = int(min(n, max(1, _free_bytes(torch, dev) // (2 * per_row))))
    parts = []
    for b0 in range(0, n, block):
        rows, _ = fisher_rows(waveform_model, points[b0:b0 + block], waveform_kwargs)
        rows, _ = _kernel_rows(rows, inner_product_kwargs, torch)
        if tuple(rows.shape[1:]) != (nchan, nbin):
            raise ValueError("the model's output changes shape between points")
        flat = red.overlap_rows_flat(rows, t, None, w)
        parts.append(flat if b0 + block >= n else flat[:-1])
        del rows
    res = torch.cat(parts).cpu().numpy()   # the one host transfer
    return res, {"h_true": t, "weights": w}


def _criterion(res, deltas, fish):
    """(mism, ratio, over) per sample from sample_overlaps' numbers (:609-639)."""
    rr = res[-1]
    over = res[0:-1:3] / np.sqrt(res[2:-1:3] * rr)
    prod = np.einsum("kj,ji,ki->k", deltas, fish, deltas)
    ratio = over / (1 - 0.5 * prod / rr)
    return (1.0 - over) / 2.0, ratio, over


def mismatch_criterion(waveform_model, params, deriv_inds=None, inner_product_kwargs={},
                       waveform_kwargs={}, parameter_transforms=None, fish=None, eps=None,
                       eigens=None, return_fish=False, fisher_kwargs={}):
    """Vallisneri's criterion for one random direction on the Fisher matrix's 1-sigma ellipsoid
    (diagnostic.py:489-644): (mism, ratio[, fish]) with mism = (1 - over) / 2,
    ratio = over / (1 - delta^T F delta / (2 <h_true|h_true>)), over the normalised overlap of the
    perturbed waveform with h_true. fish is computed by fisher(eps=...) unless given; eigens is
    its (eigenvalues, right eigenvectors) pair, np.linalg.eig's by default. The one-sample case of
    vallisneri_criterion_cdf's code; see the section comment above."""
    mism, ratio, fish, _ = _vallisneri(
        1, waveform_model, params, deriv_inds=deriv_inds,
        inner_product_kwargs=inner_product_kwargs, waveform_kwargs=waveform_kwargs,
        parameter_transforms=parameter_transforms, fish=fish, eps=eps, eigens=eigens,
        fisher_kwargs=fisher_kwargs)
    if not return_fish:
        return mism[0], ratio[0]
    return mism[0], ratio[0], fish


def vallisneri_criterion_cdf(*mismatch_args, num_samples=100, return_cdf=True,
                             return_ratios=False, fish=None, precision=False, fisher_kwargs={},
                             **mismatch_kwargs):
    """The CDF of abs(log r) over num_samples directions and its 90th percentile
    (diagnostic.py:686-757): (r_at_90[, quantiles, cdf][, ratios]). mismatch_args / _kwargs are
    mismatch_criterion's; fish comes from fisher(*mismatch_args, **fisher_kwargs) unless given,
    its eigen-pairs from get_eigens(fish, high_precision=precision) unless eigens= is given. All
    samples' waveforms come from one batched call and one reduction pass."""
    if fish is None:
        # the reference's call, plus fisher's own arguments where they were given by keyword
        # (there they reach mismatch_criterion only, and fisher fails for want of eps)
        named = {k: mismatch_kwargs[k] for k in ("eps", "deriv_inds", "parameter_transforms",
                                                 "waveform_kwargs", "inner_product_kwargs")
                 if k in mismatch_kwargs}
        fish = fisher(*mismatch_args, **named, **fisher_kwargs)
    fish = np.asarray(fish.get() if hasattr(fish, "get") else fish)
    eigens = mismatch_kwargs.pop("eigens", None)
    if eigens is None:
        eigens = get_eigens(fish, high_precision=precision)
    mismatch_kwargs.pop("return_fish", None)
    _, ratio, _, _ = _vallisneri(num_samples, *mismatch_args, fish=fish, eigens=eigens,
                                 **mismatch_kwargs)
    ratios = np.abs(np.log(ratio))
    quantiles, counts = np.unique(ratios, return_counts=True)
    cdf = np.cumsum(counts).astype(np.double) / ratios.size
    r_at_90 = np.interp(0.9, cdf, quantiles)
    out = (r_at_90,)
    if return_cdf:
        out += (quantiles, cdf)
    if return_ratios:
        out += (ratios,)
    return out


def cutler_vallisneri_bias(waveform_model_true, waveform_model_approx, params, eps,
                           in_diagnostics=None, fish=None, deriv_inds=None, return_fisher=False,
                           return_derivs=False, return_cov=False, parameter_transforms=None,
                           waveform_true_kwargs={}, waveform_approx_kwargs={},
                           inner_product_kwargs={}):
    """Cutler-Vallisneri systematic bias of an approximate template (diagnostic.py:760-840):
    syst_vec[k] = <dh_k | h_true - h_approx>, bias = cov @ syst_vec; (syst_vec, bias), or the
    list [syst_vec, bias, fish, cov, dh] with the entries the return_* flags ask for. cov, fish
    and dh come from covariance(..., return_fisher=True, return_derivs=True) on the true model,
    or cov, h_true and dh from the in_diagnostics dict. One efd_overlap_rows pass over dh forms
    the difference per element; h_true - h_approx is never stored."""
    torch = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    params = np.asarray(params, dtype=np.float64)
    if deriv_inds is None:
        deriv_inds = np.arange(len(params))
    if isinstance(eps, float):
        eps = np.full_like(params, eps)
    params_true = _transformed(params, parameter_transforms)
    if in_diagnostics is None:
        h_true, _ = fisher_rows(waveform_model_true, [params_true], waveform_true_kwargs)
        cov, fish, dh = covariance(waveform_model_true, params, eps, return_fisher=True,
                                   return_derivs=True, deriv_inds=deriv_inds,
                                   parameter_transforms=parameter_transforms,
                                   waveform_kwargs=waveform_true_kwargs,
                                   inner_product_kwargs=inner_product_kwargs)
    else:
        cov = in_diagnostics["cov"]
        h_true = _stack_channels(in_diagnostics["h_true"], torch, dev)
        h_true = h_true.reshape((1, 1, -1) if h_true.dim() == 1 else (1,) + tuple(h_true.shape))
        dh = in_diagnostics["dh"]
    h_approx, _ = fisher_rows(waveform_model_approx, [params_true], waveform_approx_kwargs)
    rows = torch.as_tensor(dh, device=dev)
    if rows.dim() == 2:   # a one-channel model's derivatives [P][n]
        rows = rows[:, None, :]
    rows, n_td = _kernel_rows(rows, inner_product_kwargs, torch)
    t, _ = _kernel_rows(h_true, inner_product_kwargs, torch)
    u, _ = _kernel_rows(h_approx, inner_product_kwargs, torch)
    nchan, nbin = int(rows.shape[1]), int(rows.shape[2])
    if tuple(t.shape[1:]) != (nchan, nbin) or tuple(u.shape[1:]) != (nchan, nbin):
        raise ValueError("cutler_vallisneri_bias: h_true, h_approx and the derivatives differ "
                         "in shape")
    w = fisher_weights(nbin, n_td=n_td, **inner_product_kwargs).expand(nchan, nbin).contiguous()
    out, _ = _reducer(dev).overlap_rows(rows.contiguous(), t[0].contiguous(), u[0].contiguous(),
                                        w)
    syst_vec = out[:, 0].cpu().numpy()
    bias = np.dot(cov, syst_vec)
    if True not in [return_fisher, return_cov, return_derivs]:
        return syst_vec, bias
    returns = [syst_vec, bias]
    if return_fisher:
        returns.append(fish)
    if return_cov:
        returns.append(cov)
    if return_derivs:
        returns.append(dh)
    return returns


def scale_snr(target_snr, sig, *snr_args, return_orig_snr=False, **snr_kwargs):
    """The signal's channels scaled to the target SNR (diagnostic.py:843-855): a list of
    channels, or (list, original snr) with return_orig_snr. Host arithmetic on top of snr()."""
    snr_out = snr(sig, *snr_args, **snr_kwargs)
    factor = target_snr / snr_out
    if isinstance(sig, list) is False:
        sig = [sig]
    out = [sig_i * factor for sig_i in sig]
    if return_orig_snr:
        return (out, snr_out)
    return out
