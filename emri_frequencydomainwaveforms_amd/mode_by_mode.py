"""The reference's mode-by-mode FD-vs-TD study (check_mode_by_mode.py run_check, :168-330) as a
batched call on the device.

    study = setup(Tobs, dt, eps, windows=("none", "blackman", "hann", "nuttall"))
    params = study.fixed_inspiral(params, Tobs)        # the driver's get_p_at_t step, :200-213
    res = study.run(params)                            # params [B][14], FEW's order

For every drawn source and each windowing the driver builds the FD template (:230-246, windowed
at :269-270), the DFT of the windowed TD template (:263-264, :271-272), and from six to eight
inner_product calls their SNR (:292), normalised overlap and mismatch (:299-301) and the
log-likelihood of their difference (:313-317). run() returns the same numbers as numpy arrays
named after the driver's h5 datasets (:352-358): SNR [B][W] (of the FD template, as the
driver's), mismatch [B][W], loglike [B][W]; and snr_td [B][W], the complex normalised overlap
[B][W], and failed: the indices of the sources whose upstream or device status reported an error.
Those rows come back NaN, like the driver's failed_points (:328-330), and do not abort the batch.

Work goes per group of `group` sources, queued on the current stream with no host
synchronisation inside a group except the generators' status reads:
  FD side   the spectra S = h+ - i hx once (GenerateEMRIWaveform.spectrum_batch). Where the
            first-order cosine-sum form holds at this grid length
            (CosineWindowConvolution.applies), the correction transform runs once per group
            (HannConvolution.transform: it does not depend on the window), then one
            efd_cosw_polarizations per (source, cosine-sum window) and efd_polarizations for
            "none". Elsewhere (short grids, other windows) the exact pair ifft(w fft(S)) runs per
            source: one forward transform and the windows' inverse transforms.
  TD side   the TD sum once per source (time_series_batch, no window), efd_window_rows into one
            [G W][N] buffer, one batched transform (get_fd_waveform_fromTD's plans and memory
            rule: a group shrinks rather than run out of memory).
  numbers   one efd_td_split_pair_stats over the group's G W rows straight from the transform
            (gain = dt, no keep mask): the TD channels are never stored.
A row's numbers do not depend on its group or its neighbours where the exact pair runs; in the
first-order form the transform length follows the group's longest support, so they agree to
that form's rounding (<= 1e-12 of max|S|) across groupings.

The (l, 0, 0) harmonics (F = 0) exist only in the TD sum. The driver compares the templates as
they are, and so does this module; drop_static=True removes those harmonics from both sides
(the convention of tools/td_vs_fd.py).
"""

import numpy as np

from . import _lib
from .summation import require_gpu

WINDOWS = ("none", "blackman", "hann", "nuttall")


def _without_static(d):
    """prepare()'s dictionary without the (l, 0, 0) harmonics."""
    keep = ~((np.asarray(d["m"]) == 0) & (np.asarray(d["n"]) == 0))
    if keep.all():
        return d
    K = len(d["m"])
    out = {k: v for k, v in d.items() if k not in ("_src", "_shape")}
    out["teuk"] = np.ascontiguousarray(d["teuk"][:, keep])
    out["m"] = np.ascontiguousarray(d["m"][keep])
    out["n"] = np.ascontiguousarray(d["n"][keep])
    out["ylms"] = np.concatenate([d["ylms"][:K][keep], d["ylms"][K:][keep]])
    return out


def _drop_static(gen):
    inner = gen.waveform_generator
    prepare = inner.prepare

    def filtered(*args, **kwargs):
        return _without_static(prepare(*args, **kwargs))

    inner.prepare = filtered


class ModeByModeStudy:
    """setup()'s result: the generators, the grid, the weights and the windows of one
    (Tobs, dt, eps); run() and fixed_inspiral() are the driver's loop body."""

    def __init__(self, Tobs, dt, eps, windows, PSD, group, drop_static, emri_kwargs):
        torch = self.torch = require_gpu()
        import scipy.signal.windows as sw
        from .fdutils import (COSINE_WINDOWS, CosineWindowConvolution, HannConvolution,
                              get_fd_waveform_fromTD)
        from .reductions import Reducer
        from .waveform import GenerateEMRIWaveform
        self.Tobs, self.dt, self.eps = float(Tobs), float(dt), float(eps)
        self.windows = tuple(windows)
        if not self.windows or len(self.windows) > _lib.EFD_WINDOW_MAX_ROWS:
            raise ValueError(f"windows: 1 to {_lib.EFD_WINDOW_MAX_ROWS} names")
        self.group = max(1, int(group))
        self.drop_static = bool(drop_static)
        self.kwargs = dict(emri_kwargs, T=self.Tobs, dt=self.dt, eps=self.eps)
        dev = self.device = torch.device("cuda", torch.cuda.current_device())
        # the driver's generators (:69-99): few_gen_list and td_gen_list
        self.fd = GenerateEMRIWaveform(
            "FastSchwarzschildEccentricFlux",
            sum_kwargs=dict(pad_output=True, output_type="fd", odd_len=True), use_gpu=True,
            return_list=True)
        self.td = GenerateEMRIWaveform(
            "FastSchwarzschildEccentricFlux", sum_kwargs=dict(pad_output=True, odd_len=True),
            use_gpu=True, return_list=True)
        if self.drop_static:
            _drop_static(self.fd)
            _drop_static(self.td)
        N = self.N = self.td.td_samples(self.Tobs, self.dt)
        nf, npos = self.fd._batch_grid(self.Tobs, self.dt, None)
        nb = self.nb = (N + 1) // 2
        if nf != N or npos != nb:
            raise ValueError("the FD grid and the TD series differ in length")
        # frequency goes from -1/dt/2 up to 1/dt/2 (:249-251); its f >= 0 part
        self.frequency = np.fft.fftshift(np.fft.fftfreq(N, self.dt))
        pos = self.frequency >= 0.0
        self.f_pos = self.frequency[pos]
        self.k0 = int(np.argmax(pos))
        # inner_product's weight for PSD = PSD(f_pos), f_arr = f_pos (:284-286)
        psd = np.asarray(PSD(self.f_pos), dtype=np.float64)
        x = np.empty(nb)
        x[1:] = np.diff(self.f_pos)
        x[0] = x[1]
        self.psd = psd
        self.w = torch.as_tensor(x / psd, dtype=torch.float64, device=dev).contiguous()
        # scipy's windows of the TD length (:269-272), on the device; "none" is no window
        self._win, self._coef, self._exact = [], [], []
        for j, name in enumerate(self.windows):
            if name in ("none", None):
                self._win.append(None)
                self._coef.append(None)
                continue
            if not hasattr(sw, name):
                raise ValueError(f"windows: {name!r} is not in scipy.signal.windows")
            self._win.append(torch.as_tensor(getattr(sw, name)(N), dtype=torch.float64,
                                             device=dev).contiguous())
            a = COSINE_WINDOWS.get(name)
            if a is not None and CosineWindowConvolution.applies(N, a):
                import ctypes
                self._coef.append((ctypes.c_double * len(a))(*a))
            else:
                self._coef.append(None)
                self._exact.append(j)
        self._conv = HannConvolution(N, dev) if any(c is not None for c in self._coef) else None
        self._mult = (torch.stack([self._win[j] for j in self._exact])
                      if self._exact else None)
        self._tdm = get_fd_waveform_fromTD(self.td, pos, self.dt)
        self.red = Reducer(dev)
        self.lib = self.red.lib
        self._buf = {}
        # a measurement hook (tools/mode_by_mode_bench.py): None, or a function called with the
        # name of each part of a group once its work is queued (to record an event there)
        self.timing = None

    # ---- the driver's get_p_at_t step (:196-213) ----------------------------------------------
    def fixed_inspiral(self, params, Tobs=None, device=False):
        """params [B][14] with p0 replaced by the value whose inspiral plunges after 0.99 Tobs
        years (trajectory.get_p_at_t, the driver's tolerances); a source the root search
        refuses keeps its p0 and fails in run() as the driver's would. device=True: every
        source's root solve at once on the device (trajectory.get_p_at_t_batch, one wavefront
        per source) instead of one host solve after the other."""
        from .trajectory import EMRIInspiral, get_p_at_t, get_p_at_t_batch
        Tobs = self.Tobs if Tobs is None else float(Tobs)
        out = np.array(params, dtype=np.float64).reshape(-1, 14)
        traj = EMRIInspiral(func="SchwarzEccFlux")
        if device:
            p0, _ = get_p_at_t_batch(traj, Tobs * 0.99, out[:, [0, 1, 4]], xtol=2e-12,
                                     rtol=8.881784197001252e-16, device=self.device,
                                     state=self._buf.setdefault("p0_state", {}))
            ok = ~np.isnan(p0)
            out[ok, 3] = p0[ok]
            return out
        for row in out:
            try:
                row[3] = get_p_at_t(traj, Tobs * 0.99, [row[0], row[1], 0.0, row[4], 1.0],
                                    index_of_p=3, index_of_a=2, index_of_e=4, index_of_x=5,
                                    traj_kwargs={}, xtol=2e-12, rtol=8.881784197001252e-16,
                                    bounds=None)
            except ValueError:
                pass
        return out

    # ---- buffers -----------------------------------------------------------------------------
    def _buffer(self, name, shape, dtype, pinned=False):
        b = self._buf.get(name)
        if b is None or tuple(b.shape) != tuple(shape):
            self._buf[name] = None
            kw = dict(pin_memory=True) if pinned else dict(device=self.device)
            b = self._buf[name] = self.torch.empty(shape, dtype=dtype, **kw)
        return b

    def _group_size(self, B):
        """Sources per group: `group`, at most EFD_BATCH_MAX, fewer while the [G W][N] series
        buffer and its plan would not fit (get_fd_waveform_fromTD._rows_that_fit)."""
        W = len(self.windows)
        G = min(B, self.group, _lib.EFD_BATCH_MAX)
        return max(1, self._tdm._rows_that_fit(G * W) // W)

    # ---- one group ---------------------------------------------------------------------------
    def _fd_side(self, params, a):
        """The FD templates of the group's sources under every window into a [G W][2][nb]."""
        torch = self.torch
        G, W, N = len(params), len(self.windows), self.N
        S = self._buffer("S", (self._cap, N), torch.complex128)[:G]
        lanes = lh = None
        if self._conv is not None:
            lanes = self._buffer("lanes", (max(self._cap, 16), 2), torch.int32)[:G]
            lh = self._buffer("lanes_host", (max(self._cap, 16), 2), torch.int32, pinned=True)[:G]
        self.fd.spectrum_batch(params, S, lanes=lanes, check=False, lanes_host=lh, **self.kwargs)
        cw = self.fd.waveform_generator.create_waveform
        if cw.positive_start() != self.k0:
            raise ValueError("the FD generator's grid is not the study's")
        st = torch.cuda.current_stream(self.device).cuda_stream
        Y = info = m = None
        if self._conv is not None:   # the window-independent correction, once per group
            self.fd.lanes_ready()
            support = self._conv.lane_support(lh.numpy(), N)
            Y, info, m = self._conv.transform(S, self.lib, lanes, support)
        for i in range(G):
            Sw = None
            if self._exact:   # the exact pair: one forward transform, the windows' inverses
                Sw = torch.fft.ifft(torch.fft.fft(S[i])[None, :] * self._mult, dim=-1)
            for j in range(W):
                hp, hc = a[i * W + j, 0], a[i * W + j, 1]
                if self._win[j] is None:
                    cw.polarizations(S[i], True, out=(hp, hc))
                elif self._coef[j] is not None:
                    _lib.check(self.lib.efd_cosw_polarizations(
                        torch.view_as_real(S[i]).data_ptr(), torch.view_as_real(Y[i]).data_ptr(),
                        info[i].data_ptr(), m, N, self.k0, self._coef[j], len(self._coef[j]),
                        torch.view_as_real(hp).data_ptr(), torch.view_as_real(hc).data_ptr(), st),
                        "efd_cosw_polarizations", self.lib)
                else:
                    cw.polarizations(Sw[self._exact.index(j)], True, out=(hp, hc))

    def _td_side(self, params):
        """Z = fft(window * h) of every (source, window) of the group: [G W][N], natural order."""
        torch = self.torch
        G, W, N = len(params), len(self.windows), self.N
        h = self._buffer("h", (self._cap, N), torch.complex128)[:G]
        Z = self._buffer("Z", (self._cap * W, N), torch.complex128)[:G * W]
        self.td.time_series_batch(params, h, window=None, check=False, **self.kwargs)
        if self.timing is not None:
            self.timing("td_sum")
        for i in range(G):
            self.red.window_rows(h[i], self._win, Z[i * W:(i + 1) * W])
        return self._tdm._transform(Z)

    def _run_group(self, params, raw):
        """The group's numbers into raw ([G W][2][5], device); raises when a source's upstream or
        device status reports an error (after the stream is idle)."""
        torch = self.torch
        G, W = len(params), len(self.windows)
        a = self._buffer("a", (self._cap * W, 2, self.nb), torch.complex128)[:G * W]
        mark = self.timing or (lambda name: None)
        try:
            mark("start")
            self._fd_side(params, a)
            mark("fd_side")
            Z = self._td_side(params)
            mark("window_transform")
            self.red.td_split_pair_stats(Z, self.N, self.dt, a, self.w, out=raw)
            mark("reduction")
        except BaseException:
            torch.cuda.current_stream(self.device).synchronize()
            raise
        self.fd.check_batch()
        self.td.check_td_batch()

    # ---- the batch -----------------------------------------------------------------------------
    def run(self, params):
        """The study over params [B][14] (FEW's order): a dict of numpy arrays SNR, mismatch,
        loglike, snr_td [B][W], overlap complex [B][W], failed (indices), windows (names)."""
        torch = self.torch
        params = np.asarray(params, dtype=np.float64).reshape(-1, 14)
        B, W = len(params), len(self.windows)
        raw = torch.full((B * W, 2, 5), float("nan"), dtype=torch.float64, device=self.device)
        failed = []
        G = self._group_size(B) if B else 1
        self._cap = max(G, getattr(self, "_cap", 0))
        errors = (_lib.EFDError, ValueError, RuntimeError)
        for g0 in range(0, B, G):
            rows = params[g0:g0 + G]
            out = raw[g0 * W:(g0 + len(rows)) * W]
            try:
                self._run_group(rows, out)
                continue
            except errors:
                out.fill_(float("nan"))
            # a source of the group failed: one at a time, so that only it comes back NaN (a
            # row's numbers do not depend on its group)
            for i in range(len(rows)):
                one = raw[(g0 + i) * W:(g0 + i + 1) * W]
                try:
                    self._run_group(rows[i:i + 1], one)
                except errors:
                    one.fill_(float("nan"))
                    failed.append(g0 + i)
        from .diagnostic import PairStatistics
        s = PairStatistics(raw.cpu().numpy())       # the one host transfer
        with np.errstate(divide="ignore", invalid="ignore"):
            overlap = s.overlap + 1j * (s.ab_sum.imag / np.sqrt(s.aa_sum * s.bb_sum))
        shape = (B, W)
        return dict(SNR=s.snr1.reshape(shape), mismatch=s.mismatch.reshape(shape),
                    loglike=s.loglike.reshape(shape), snr_td=s.snr2.reshape(shape),
                    overlap=overlap.reshape(shape), failed=np.asarray(failed, dtype=np.int64),
                    windows=self.windows)


def setup(Tobs, dt, eps, windows=WINDOWS, PSD=None, group=8, drop_static=False, **emri_kwargs):
    """The driver's generators (check_mode_by_mode.py:69-99), the positive-frequency grid, the
    inner products' weights (PSD: a function of frequency, default fdutils.get_sensitivity, the
    driver's :284-286) and scipy's windows of the TD length on the device, for run().
    windows: "none" or names of scipy.signal.windows (the driver's: none, blackman, hann,
    nuttall); group: sources per device group; drop_static: leave the (l, 0, 0) harmonics out of
    both sides (module docstring); emri_kwargs: further waveform keyword arguments."""
    if PSD is None:
        from .fdutils import get_sensitivity as PSD
    return ModeByModeStudy(Tobs, dt, eps, windows, PSD, group, drop_static, emri_kwargs)
