"""lisatools-compatible inner products on the device (LISAanalysistools/lisatools/diagnostic.py).

    inner_product(sig1, sig2, dt=None, df=None, f_arr=None, PSD="lisasens", PSD_args=(),
                  PSD_kwargs={}, normalize=False, use_gpu=False, complex=False)   :14-157
    snr(sig1, *args, data=None, use_gpu=False, **kwargs)                         :160-171

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
    psd = _psd_array(PSD, freqs, PSD_args, PSD_kwargs, torch, dev)
    nbin = len(f1[0])
    x = torch.empty(nbin, dtype=torch.float64, device=dev)
    x[1:] = torch.diff(freqs)
    x[0] = x[1]
    w = (x / psd).expand(len(f1), nbin).contiguous()
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
        # time-domain rows: real and imaginary parts are the reference's channels, each
        # rfft * dt with the DC bin dropped (diagnostic.py:57-73); the kernel takes those
        n_td = rows.shape[-1]
        td = rows
        parts = [rows.real, rows.imag] if rows.is_complex() else [rows]
        dt_ = inner_product_kwargs["dt"]
        rows = torch.cat([torch.fft.rfft(p.to(torch.float64), dim=-1)[..., 1:] * dt_
                          for p in parts], dim=1).contiguous()
    else:
        n_td = None
        rows = rows.to(torch.complex128)
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
