"""Teukolsky-amplitude STAND-IN and mode selection (host side, upstream of the hot path).

The reference evaluates `RomanAmplitude` (ROMAN network, 3843 complex modes l<=10, 0<=m<=l,
|n|<=30) and keeps modes with `ModeSelector(eps)` (Tutorial_FD_construction_single_mode.ipynb:32,
:37, :125-127; `eps` kwarg emri_pe.py:659-663). The network weights are absent offline (SURVEY.md
section 2, row 1c), so `SyntheticTeukolskyAmplitude` returns seeded, smooth complex amplitudes
with the same mode list, ordering and call surface. Magnitudes fall off geometrically in l, l-m
and |n - n_peak(e)| (eccentric orbits spread power over n), and grow as p shrinks, tuned so that
eps = 1e-5 keeps ~3000 modes and eps = 1e-2 keeps ~10^2 at e ~ 0.35 like the reference's
BASELINE configs. NOT FEW physics: only the workload shape (modes, supports) is meaningful.

`ModeSelector` restates FEW's power-based selection [FEW-ext, from the FEW 1.x sources as
recalled in SURVEY.md]: per trajectory point, sort |A Y|^2 over the m>=0 and partner -m
branches, keep the modes needed to reach (1 - eps) of the power, fold -m picks onto +m, take
the union over time.

The same model and selection also run on the device for batched callers
(csrc/emrifd_modes_device.inc: efd_modes_select_batch): `device_select`,
`SyntheticTeukolskyAmplitude.select_batch_device` and `ModeSelector(m0mask, use_gpu=True)`.

Noise-weighted selection (FEW's `ModeSelector(sensitivity_fn=...)`, as recalled): both branch
powers of mode k at knot i are divided by the PSD at |m_k f_phi[i] + n_k f_r[i]| before the cut,
so eps is a fraction of noise-weighted power. numpy defines it (`ModeSelector.__call__`); the
native routes (efd_host_modes_weighted, efd_modes_select_batch_weighted) evaluate the PSD from a
piecewise-cubic table (`psd_table`, `PsdTable`).
"""

import ctypes

import numpy as np

LMAX = 10
NMAX = 30
_SEED = 2601996  # the reference's SEED (check_mode_by_mode.py:47, emri_pe.py:65)


def mode_list(lmax=LMAX, nmax=NMAX):
    l_arr, m_arr, n_arr = [], [], []
    for l in range(2, lmax + 1):
        for m in range(0, l + 1):
            for n in range(-nmax, nmax + 1):
                l_arr.append(l)
                m_arr.append(m)
                n_arr.append(n)
    return (np.asarray(l_arr, dtype=np.int32), np.asarray(m_arr, dtype=np.int32),
            np.asarray(n_arr, dtype=np.int32))


def _f64(x):
    """float64 view of a device tensor (complex128 as interleaved re, im)."""
    import torch
    return torch.view_as_real(x).reshape(-1) if x.is_complex() else x


class PsdTable:
    """A PSD as a piecewise cubic in scipy's PPoly layout (x [n] ascending, c [4][n - 1]) for
    the native selections: `host` is the efd_psd_table over this object's arrays, `device(dev)`
    the one over their copies on a device (uploaded once per table and device)."""

    def __init__(self, x, c):
        from . import _lib
        x = np.ascontiguousarray(x, dtype=np.float64)
        c = np.asarray(c, dtype=np.float64)
        if x.ndim != 1 or c.ndim != 2 or not 1 <= c.shape[0] <= 4 or c.shape[1] != len(x) - 1:
            raise ValueError("PsdTable: x [n] and c [k <= 4][n - 1] (scipy's PPoly layout)")
        if not 2 <= len(x) <= 4096 or not np.all(np.diff(x) > 0):
            raise ValueError("PsdTable: 2 <= n <= 4096 breakpoints, strictly ascending")
        # a lower order is a cubic with zero leading coefficients
        self.x = x
        self.c = np.ascontiguousarray(np.concatenate([np.zeros((4 - c.shape[0], c.shape[1])), c]))
        self.host = _lib.PsdTable(self.x.ctypes.data, self.c.ctypes.data, len(x))
        self._dev = {}

    def device(self, device):
        import torch

        from . import _lib
        key = (device.type, device.index)
        if key not in self._dev:
            t = [torch.from_numpy(a).to(device) for a in (self.x, self.c)]
            torch.cuda.current_stream(device).synchronize()
            self._dev[key] = (_lib.PsdTable(t[0].data_ptr(), t[1].data_ptr(), len(self.x)), t)
        return self._dev[key][0]

    def ppoly(self):
        from scipy.interpolate import PPoly
        return PPoly(self.c, self.x, extrapolate=True)


def psd_table(sensitivity_fn):
    """The PsdTable of a sensitivity function the native selections can evaluate:
    fdutils.get_sensitivity (its module spline) or any object with PPoly-shaped .x and .c
    (scipy's CubicSpline, PPoly); None for other callables."""
    from . import fdutils
    if sensitivity_fn is fdutils.get_sensitivity:
        sensitivity_fn = fdutils._spline()
    x, c = getattr(sensitivity_fn, "x", None), getattr(sensitivity_fn, "c", None)
    if x is None or c is None:
        return None
    try:
        return PsdTable(x, c)
    except (ValueError, TypeError):
        return None


NO_TABLE = ("the sensitivity_fn has no piecewise-cubic table the device can evaluate: pass "
            "fdutils.get_sensitivity, or a scipy.interpolate.CubicSpline / PPoly of the PSD "
            "(e.g. CubicSpline(f, sensitivity_fn(f)))")


def device_select(table, nmodes, walkers, device, stream=None, state=None, prof=None, psd=None):
    """efd_modes_select_batch for 1..EFD_BATCH_MAX walkers on `stream` (a torch stream; default
    the current one), then one efd_download of every walker's nkeep, status and keep and one
    stream synchronisation (the mode sum's K is a host argument).

    table: _lib.ModesTable over device arrays. walkers: dicts with p, e (float64 [nt] on the
    device), ylm_p, ylm_m (float64 views of complex [nmodes]), eps, include_minus_m, teuk
    (float64 view of complex [nt][nmodes], or None: the stand-in model) and want_amp. state: a
    dict the caller keeps per stream (the pinned download buffer lives there). prof: a pair of
    torch timing events recorded around efd_modes_select_batch's launches alone. psd: a PsdTable;
    then the call is efd_modes_select_batch_weighted, and the walkers that carry f_phi and f_r
    (float64 [nt] on the device, Hz) are selected on noise-weighted power.

    Returns one dict per walker: K, keep (device int32 [K]), keep_host (numpy int32 [K]), amp
    (float64 view of complex [nt][K], or None), m, n (int32 [K]), ylm_p, ylm_m (float64 [2 K]):
    views into the selection's output buffers, in the mode sum's input layout. An amplitude
    buffer that turns out too small is an error (the buffers here hold the worst case)."""
    import torch

    from . import _lib
    lib = _lib.load()
    n = len(walkers)
    if not 1 <= n <= _lib.EFD_BATCH_MAX:
        raise ValueError(f"device_select takes 1..{_lib.EFD_BATCH_MAX} walkers")
    strm = stream if stream is not None else torch.cuda.current_stream(device)
    state = state if state is not None else {}
    row = 2 + nmodes                      # int32 per walker: nkeep, status, keep[nmodes]
    nts = [int(w["p"].numel()) for w in walkers]
    wsb = [int(lib.efd_modes_workspace_bytes(nt, nmodes)) for nt in nts]
    if not all(wsb):
        raise _lib.EFDError("efd_modes_workspace_bytes rejected the shape")
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    # one block per group: [ints | m, n | ylm_p, ylm_m | workspaces | amplitudes]
    o_int = 0
    o_mn = al(4 * row * n)
    o_y = o_mn + al(8 * nmodes * n)
    o_ws = o_y + al(32 * nmodes * n)
    offs_ws, off = [], o_ws
    for b in wsb:
        offs_ws.append(off)
        off = al(off + b)
    offs_amp = []
    for w, nt in zip(walkers, nts):
        offs_amp.append(off)
        if w.get("want_amp", True):
            off = al(off + 16 * nt * nmodes)
    with torch.cuda.stream(strm):
        blk = torch.empty(off, dtype=torch.uint8, device=device)
    base = blk.data_ptr()
    ints = blk[o_int:o_int + 4 * row * n].view(torch.int32)
    ws = (_lib.ModesWalker * n)()
    for i, (w, nt) in enumerate(zip(walkers, nts)):
        a = ws[i]
        a.p, a.e, a.nt = w["p"].data_ptr(), w["e"].data_ptr(), nt
        a.ylm_p, a.ylm_m = w["ylm_p"].data_ptr(), w["ylm_m"].data_ptr()
        a.eps, a.include_minus_m = float(w["eps"]), 1 if w.get("include_minus_m", True) else 0
        a.teuk = w["teuk"].data_ptr() if w.get("teuk") is not None else None
        a.nkeep = base + o_int + 4 * row * i
        a.status = a.nkeep + 4
        a.keep = a.nkeep + 8
        a.m_out = base + o_mn + 8 * nmodes * i
        a.n_out = a.m_out + 4 * nmodes
        a.ylm_p_out = base + o_y + 32 * nmodes * i
        a.ylm_m_out = a.ylm_p_out + 16 * nmodes
        a.workspace, a.workspace_bytes = base + offs_ws[i], wsb[i]
        if w.get("want_amp", True):
            a.amp, a.amp_cap = base + offs_amp[i], nt * nmodes
    st = strm.cuda_stream
    if psd is not None:
        wts = (_lib.ModesWeight * n)()
        for i, w in enumerate(walkers):
            if w.get("f_phi") is not None:
                wts[i].f_phi, wts[i].f_r = w["f_phi"].data_ptr(), w["f_r"].data_ptr()
        dpsd = psd.device(device)
    if prof is not None:   # (begin, end) torch events around the three launches alone
        prof[0].record(strm)
    if psd is not None:
        _lib.check(lib.efd_modes_select_batch_weighted(ctypes.byref(table), ws, wts,
                                                       ctypes.byref(dpsd), n, st),
                   "efd_modes_select_batch_weighted", lib)
    else:
        _lib.check(lib.efd_modes_select_batch(ctypes.byref(table), ws, n, st),
                   "efd_modes_select_batch", lib)
    if prof is not None:
        prof[1].record(strm)
    hb = state.get("ints")
    if hb is None or hb.numel() < row * n:
        hb = state["ints"] = torch.empty(row * _lib.EFD_BATCH_MAX, dtype=torch.int32,
                                         pin_memory=True)
    _lib.check(lib.efd_download(hb.data_ptr(), ints.data_ptr(), 4 * row * n, st), "efd_download",
               lib)
    strm.synchronize()
    host = hb.numpy()[:row * n].reshape(n, row)
    out = []
    for i, (w, nt) in enumerate(zip(walkers, nts)):
        K, status = int(host[i, 0]), int(host[i, 1])
        if status & _lib.EFD_MODES_AMP_OVERFLOW:
            raise _lib.EFDError("efd_modes_select_batch: amplitude buffer too small")
        o = o_mn + 8 * nmodes * i
        oy = o_y + 32 * nmodes * i
        amp = None
        if w.get("want_amp", True):
            amp = blk[offs_amp[i]:offs_amp[i] + 16 * nt * K].view(torch.float64)
        out.append(dict(
            K=K, nt=nt, keep=ints[row * i + 2:row * i + 2 + K],
            keep_host=host[i, 2:2 + K].copy(), amp=amp,
            m=blk[o:o + 4 * K].view(torch.int32),
            n=blk[o + 4 * nmodes:o + 4 * nmodes + 4 * K].view(torch.int32),
            ylm_p=blk[oy:oy + 16 * K].view(torch.float64),
            ylm_m=blk[oy + 16 * nmodes:oy + 16 * nmodes + 16 * K].view(torch.float64)))
    return out


class SyntheticTeukolskyAmplitude:
    """Seeded smooth complex A_lmn(p, e) over FEW's 3843-mode list (stand-in for RomanAmplitude)."""

    def __init__(self, lmax=LMAX, nmax=NMAX, seed=_SEED, use_gpu=False, **kwargs):
        self.l_arr, self.m_arr, self.n_arr = mode_list(lmax, nmax)
        self.num_teuk_modes = len(self.l_arr)
        self.m0mask = self.m_arr != 0
        self.num_m_zero_up = self.num_teuk_modes
        self.num_m0 = int(np.sum(~self.m0mask))
        self.num_m_1_p = self.num_teuk_modes  # index offset of the -m partners in power arrays
        self.lmn_indices = {(int(l), int(m), int(n)): i
                            for i, (l, m, n) in enumerate(zip(self.l_arr, self.m_arr, self.n_arr))}
        lm = np.stack([self.l_arr, self.m_arr], axis=1)
        unique_lm, self.inverse_lm = np.unique(lm, axis=0, return_inverse=True)
        self.inverse_lm = self.inverse_lm.reshape(-1)
        self.unique_l, self.unique_m = unique_lm[:, 0], unique_lm[:, 1]
        rng = np.random.default_rng(seed)
        self._phase0 = rng.uniform(0.0, 2.0 * np.pi, self.num_teuk_modes)
        self._jitter = rng.uniform(-0.15, 0.15, self.num_teuk_modes)

    def _log10_mag(self, p, e):
        l = self.l_arr[None, :].astype(np.float64)
        m = self.m_arr[None, :].astype(np.float64)
        n = self.n_arr[None, :].astype(np.float64)
        p = np.asarray(p, dtype=np.float64)[:, None]
        e = np.asarray(e, dtype=np.float64)[:, None]
        n_peak = m * 1.4 * e
        width = 0.35 + 2.2 * e        # eccentric orbits spread power over many n
        decay = 0.42 * (l - 2.0) + 0.30 * (l - m) + 0.60 * np.abs(n - n_peak) / width
        # a steep core holding ~99% of the power over a slowly decaying tail: eps = 1e-2 keeps
        # ~10^2 modes, eps = 1e-5 reaches into the tail and keeps ~3000
        core = -1.0 - decay
        tail = -3.6 - 0.085 * decay
        return (np.log10(10.0 ** core + 10.0 ** tail)
                + 0.5 * (l + 2.0) * np.log10(10.0 / p) + self._jitter[None, :])

    def __call__(self, p, e, *args, specific_modes=None, **kwargs):
        p = np.atleast_1d(np.asarray(p, dtype=np.float64))
        e = np.atleast_1d(np.asarray(e, dtype=np.float64))
        mag = 10.0 ** self._log10_mag(p, e)
        # slow, smooth phase drift along the inspiral keeps Re/Im splines non-trivial
        drift = 0.2 * (self.l_arr[None, :] - self.m_arr[None, :] + 1) * (10.0 / p[:, None]) \
            + 0.1 * self.n_arr[None, :] * e[:, None]
        amps = mag * np.exp(1j * (self._phase0[None, :] + drift))
        if specific_modes is None:
            return amps
        out = {}
        for lmn in specific_modes:
            l, m, n = (int(v) for v in lmn)
            if m >= 0:
                out[(l, m, n)] = amps[:, self.lmn_indices[(l, m, n)]]
            else:  # FEW symmetry A_{l,-m,-n} = (-1)^l conj(A_{l,m,n})
                out[(l, m, n)] = (-1.0) ** l * np.conj(amps[:, self.lmn_indices[(l, -m, -n)]])
        return out


    def device_table(self, device):
        """(_lib.ModesTable, tensors) of this model's mode list on `device`: l, m, n, phase0 and
        jitter, uploaded once per generator and device."""
        import torch

        from . import _lib
        cache = self.__dict__.setdefault("_dev_tables", {})
        key = (device.type, device.index)
        if key not in cache:
            t = [torch.from_numpy(np.ascontiguousarray(a)).to(device)
                 for a in (self.l_arr, self.m_arr, self.n_arr, self._phase0, self._jitter)]
            torch.cuda.current_stream(device).synchronize()
            cache[key] = (_lib.ModesTable(*[x.data_ptr() for x in t], self.num_teuk_modes), t)
        return cache[key]

    def select_batch_device(self, p_list, e_list, ylms_list, eps, include_minus_m=True,
                            device=None, stream=None, state=None, want_amp=True, prof=None,
                            f_phi_list=None, f_r_list=None, psd=None):
        """ModeSelector(eps) and the kept modes' amplitudes of several walkers on the device
        (efd_modes_select_batch, the stand-in model evaluated in the kernels): select() without
        the host. p_list, e_list: each walker's knots (float64 [nt], device tensors or numpy);
        ylms_list: each walker's GetYlms output over the whole mode list (complex128 [2 K],
        device tensor or numpy; walkers may share one object); eps: one value or one per walker.

        Returns one (keep, K, views) per walker: keep the kept indices (device int32 [K]), views
        a dict of amp, m, n, ylm_p, ylm_m (and keep_host, nt), ready to be
        summation.DeviceInputs fields. prof: device_select's event pair.

        psd (a PsdTable) with f_phi_list, f_r_list (each walker's knot frequencies in Hz, as p;
        an entry None leaves that walker unweighted): the noise-weighted selection."""
        import torch
        dev = device or torch.device("cuda", torch.cuda.current_device())
        table, _ = self.device_table(dev)
        n = len(p_list)
        eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (n,))
        K = self.num_teuk_modes
        strm = stream if stream is not None else torch.cuda.current_stream(dev)

        def dev_t(x, dt):
            if isinstance(x, np.ndarray):
                with torch.cuda.stream(strm):
                    return torch.from_numpy(np.array(x, dtype=dt, order="C")).to(dev)
            return x

        ycache = {}
        walkers = []
        for i in range(n):
            y = ycache.get(id(ylms_list[i]))
            if y is None:
                y = ycache[id(ylms_list[i])] = _f64(dev_t(ylms_list[i], np.complex128))
            if y.numel() != 4 * K:
                raise ValueError("ylms must hold 2 K complex values (+m, then the partners)")
            walkers.append(dict(p=dev_t(p_list[i], np.float64), e=dev_t(e_list[i], np.float64),
                                ylm_p=y[:2 * K], ylm_m=y[2 * K:], eps=float(eps[i]),
                                include_minus_m=include_minus_m, teuk=None, want_amp=want_amp))
            if psd is not None and f_phi_list is not None and f_phi_list[i] is not None:
                walkers[-1].update(f_phi=dev_t(f_phi_list[i], np.float64),
                                   f_r=dev_t(f_r_list[i], np.float64))
        res = device_select(table, K, walkers, dev, strm, state, prof, psd=psd)
        return [(r["keep"], r["K"], r) for r in res]

    def select(self, p, e, ylms, eps, lib=None, f_phi=None, f_r=None, psd=None):
        """(keep, teuk): ModeSelector(eps) over this model's modes and the kept modes' complex
        amplitudes [N_t][K], in one native call (csrc/emrifd_host.cpp: efd_host_modes) when the
        library is available, else through __call__ + ModeSelector (numpy). ylms: the GetYlms
        output [Y_lm..., (-1)^l Y_l-m...] over the whole mode list.

        psd (a PsdTable) with f_phi, f_r (the knot frequencies in Hz): the noise-weighted
        selection (efd_host_modes_weighted); the kept set may then be empty."""
        weighted = psd is not None
        if weighted and (f_phi is None or f_r is None):
            raise ValueError("the noise-weighted selection needs f_phi and f_r")
        if lib is None or not hasattr(lib, "efd_host_modes_weighted" if weighted
                                      else "efd_host_modes"):
            A = self(p, e)
            if weighted:
                keep = ModeSelector(self.m0mask, sensitivity_fn=psd.ppoly())(
                    A, ylms, (self.l_arr, self.m_arr, self.n_arr), eps=eps,
                    mode_freqs=(f_phi, f_r))
            else:
                keep = ModeSelector(self.m0mask)(A, ylms, None, eps=eps)
            return keep, np.ascontiguousarray(A[:, keep])
        p = np.ascontiguousarray(p, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64)
        K = self.num_teuk_modes
        yp = np.ascontiguousarray(ylms[:K], dtype=np.complex128)
        ym = np.ascontiguousarray(ylms[K:], dtype=np.complex128)
        keep = np.empty(K, dtype=np.int32)
        nkeep = ctypes.c_int32(0)
        nt = len(p)
        cap = 2 * nt * K   # np.empty: untouched pages cost nothing
        if weighted:
            f_phi = np.ascontiguousarray(f_phi, dtype=np.float64)
            f_r = np.ascontiguousarray(f_r, dtype=np.float64)
            if f_phi.shape != (nt,) or f_r.shape != (nt,):
                raise ValueError("f_phi and f_r must hold one value per knot")
        for _ in range(2):
            teuk = np.empty(cap // 2, dtype=np.complex128)
            head = (p.ctypes.data, e.ctypes.data, nt, self.l_arr.ctypes.data,
                    self.m_arr.ctypes.data, self.n_arr.ctypes.data, self._phase0.ctypes.data,
                    self._jitter.ctypes.data, K, yp.ctypes.data, ym.ctypes.data, float(eps))
            tail = (keep.ctypes.data, ctypes.byref(nkeep), teuk.ctypes.data, cap)
            if weighted:
                rc = lib.efd_host_modes_weighted(*head, f_phi.ctypes.data, f_r.ctypes.data,
                                                 ctypes.byref(psd.host), *tail)
            else:
                rc = lib.efd_host_modes(*head, *tail)
            if rc == 0:
                k = nkeep.value
                return keep[:k].astype(np.int64), teuk[:nt * k].reshape(nt, k)
            if rc != -3:
                raise RuntimeError(f"efd_host_modes failed ({rc})")
            cap = 2 * nt * nkeep.value
        raise RuntimeError("efd_host_modes: amplitude buffer")


# FEW-compatible name used by the reference notebooks
RomanAmplitude = SyntheticTeukolskyAmplitude


class ModeSelector:
    """Keep the modes carrying (1 - eps) of the power (few.utils.modeselector.ModeSelector).

    sensitivity_fn: a PSD S(f) (array in, array out). The branch powers of mode k at knot i are
    then divided by S(|m_k f_phi[i] + n_k f_r[i]|) before the cut (weight 0 where S is not
    finite or not > 0), so eps is a fraction of noise-weighted power."""

    def __init__(self, m0mask, sensitivity_fn=None, use_gpu=False):
        self.m0mask = np.asarray(m0mask, dtype=bool)
        self.num_m_1_p = len(self.m0mask)
        self.use_gpu = bool(use_gpu)
        self.sensitivity_fn = sensitivity_fn
        # what the native routes evaluate (None: only numpy can call sensitivity_fn)
        self.psd_table = psd_table(sensitivity_fn) if sensitivity_fn is not None else None
        self._table = {}

    @staticmethod
    def _frequencies(fund_freq_args, mode_freqs):
        """(f_phi, f_r) in Hz at the knots, from mode_freqs or FEW's fund_freq_args."""
        if mode_freqs is not None:
            return mode_freqs
        if fund_freq_args is None:
            raise ValueError("the noise-weighted selection needs mode_freqs=(f_phi, f_r) or "
                             "fund_freq_args=(M, a, p, e, x)")
        from .constants import MTSUN_SI
        from .frequencies import get_fundamental_frequencies
        M, a, p, e, x = fund_freq_args
        om_phi, _, om_r = get_fundamental_frequencies(a, p, e, x)
        return om_phi / (2.0 * np.pi * M * MTSUN_SI), om_r / (2.0 * np.pi * M * MTSUN_SI)

    def _device_call(self, teuk_modes, ylms, eps, modeinds=None, freqs=None):
        """The selection on the device (efd_modes_select_batch with the amplitudes given):
        complex128 device tensors in, the kept indices out as a device int32 tensor. freqs:
        (f_phi, f_r) of the noise-weighted selection (device tensors or numpy)."""
        import torch

        from . import _lib
        dev = teuk_modes.device
        nt, K = teuk_modes.shape
        if K != len(self.m0mask) or ylms.numel() != 2 * K:
            raise ValueError("teuk_modes [N_t, K] and ylms [2 K] must match m0mask")
        key = (dev.type, dev.index)
        if freqs is not None:
            # the weights need the modes' own m and n
            mh = np.ascontiguousarray(modeinds[1], dtype=np.int32)
            nh = np.ascontiguousarray(modeinds[2], dtype=np.int32)
            if mh.shape != (K,) or nh.shape != (K,) or not np.array_equal(mh != 0, self.m0mask):
                raise ValueError("modeinds (l, m, n) must hold [K] arrays with m != 0 as m0mask")
            key = key + (mh.tobytes(), nh.tobytes())
        if key not in self._table:
            # the selection reads m != 0 only; l, n, phase0 and jitter belong to the stand-in
            # model, which a call with the amplitudes given never evaluates
            m = torch.from_numpy(self.m0mask.astype(np.int32) if freqs is None else mh).to(dev)
            zi = torch.zeros(K, dtype=torch.int32, device=dev)
            nn = zi if freqs is None else torch.from_numpy(nh).to(dev)
            zd = torch.zeros(K, dtype=torch.float64, device=dev)
            self._table[key] = (_lib.ModesTable(zi.data_ptr(), m.data_ptr(), nn.data_ptr(),
                                                zd.data_ptr(), zd.data_ptr(), K), (m, zi, zd, nn))
        table = self._table[key][0]
        y = _f64(ylms.to(torch.complex128).contiguous())
        pe = torch.ones(nt, dtype=torch.float64, device=dev)   # unused with teuk given
        w = dict(p=pe, e=pe, ylm_p=y[:2 * K], ylm_m=y[2 * K:], eps=float(eps),
                 teuk=_f64(teuk_modes.to(torch.complex128).contiguous()), want_amp=False)
        if freqs is not None:
            f = [torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x,
                                 dtype=torch.float64, device=dev).contiguous() for x in freqs]
            if f[0].shape != (nt,) or f[1].shape != (nt,):
                raise ValueError("f_phi and f_r must hold one value per knot")
            w.update(f_phi=f[0], f_r=f[1])
        return device_select(table, K, [w], dev, psd=self.psd_table if freqs is not None
                             else None)[0]["keep"].clone()

    def __call__(self, teuk_modes, ylms, modeinds, fund_freq_args=None, eps=1e-5,
                 mode_freqs=None):
        """teuk_modes [N_t, K]; ylms [K + K] (+m then partner); returns kept mode indices (with
        use_gpu: device tensors in, a device int32 tensor out).

        With a sensitivity_fn: modeinds = (l, m, n) arrays [K] are required, and the knot
        frequencies come from mode_freqs=(f_phi, f_r) (Hz, [N_t] each) or from FEW's
        fund_freq_args=(M, a, p, e, x). A knot whose weighted total is 0 or not finite keeps
        nothing, so the result can be empty."""
        weighted = self.sensitivity_fn is not None
        if weighted:
            if modeinds is None:
                raise ValueError("the noise-weighted selection needs modeinds=(l, m, n)")
            f_phi, f_r = self._frequencies(fund_freq_args, mode_freqs)
        if self.use_gpu:
            if weighted and self.psd_table is None:
                raise ValueError("ModeSelector(use_gpu=True): " + NO_TABLE)
            return self._device_call(teuk_modes, ylms, eps, modeinds,
                                     (f_phi, f_r) if weighted else None)
        K = teuk_modes.shape[1]
        ylm_p, ylm_m = ylms[:K], ylms[K:]
        # m = 0 modes have no separate partner branch (their +-n mirrors are separate modes)
        partner = np.conj(teuk_modes[:, self.m0mask]) * ylm_m[self.m0mask][None, :]
        power = np.abs(np.concatenate([teuk_modes * ylm_p[None, :], partner], axis=1)) ** 2
        if weighted:
            m = np.asarray(modeinds[1], dtype=np.float64)
            n = np.asarray(modeinds[2], dtype=np.float64)
            f_phi = np.asarray(f_phi, dtype=np.float64)
            f_r = np.asarray(f_r, dtype=np.float64)
            if m.shape != (K,) or n.shape != (K,) or f_phi.shape != power.shape[:1] \
                    or f_r.shape != power.shape[:1]:
                raise ValueError("modeinds [K] and mode_freqs [N_t] must match teuk_modes")
            F = np.abs(m[None, :] * f_phi[:, None] + n[None, :] * f_r[:, None])
            S = np.asarray(self.sensitivity_fn(F), dtype=np.float64)
            ok = np.isfinite(S) & (S > 0.0)
            W = np.where(ok, 1.0 / np.where(ok, S, 1.0), 0.0)
            # the partner's frequency is -F: one weight serves both branches of a mode
            power = power * np.concatenate([W, W[:, self.m0mask]], axis=1)
        partner_idx = np.nonzero(self.m0mask)[0]
        inds_sort = np.argsort(power, axis=1)[:, ::-1]
        power = np.take_along_axis(power, inds_sort, axis=1)
        cumsum = np.cumsum(power, axis=1)
        keep = np.ones(cumsum.shape, dtype=bool)
        keep[:, 1:] = cumsum[:, :-1] < cumsum[:, -1][:, None] * (1.0 - eps)
        if weighted:
            # nothing can be ranked at a knot whose total is 0 or not finite: it keeps nothing
            total = cumsum[:, -1]
            keep[~(np.isfinite(total) & (total > 0.0)), :] = False
        picked = inds_sort[keep]
        # fold partner picks back onto their +m mode (no m != 0 mode: no partner to fold)
        if partner_idx.size:
            picked = np.where(picked < K, picked, partner_idx[np.clip(picked - K, 0, None)])
        return np.unique(picked)
