"""lisatools-compatible Gaussian likelihood with the reduction on the device.

Mirror of LISAanalysistools/lisatools/sampling/likelihood.py `Likelihood` (:13-334) for the FD
templates the reference drivers use (emri_pe.py:381-414: two channels h+, hx over f >= 0,
noise_fn = FDutils.get_sensitivity, f_arr = frequency[frequency >= 0]):

  inject_signal (:80-234)  data d = inj * sqrt(diff(f)/PSD) and the noise factor
                           w = sqrt(diff(f)/PSD), diff(f)[0] = diff(f)[1]; repeated
                           injections add up; add_noise=True adds one noise realisation on
                           the device (the reference raises at :184 and leaves the recipe
                           below it; see inject_signal)
  get_ll (:236-293)        per walker: template h, ll = -1/2 * 4 * sum |d - h w|^2 over
                           channels and bins, skipping bin 0 when w[0][0] is NaN (:268)
  __call__ (:295-334)      parameter transform, transpose_params, `subset` batching

What changes is where the work happens. Data and noise factor live on the device. On
symmetric grids (FEW's own and the drivers' downsampled f_arr) the walkers' mode sums run a few
at a time in one launch with the likelihood fused into the sum's epilogue
(efd_modesum_sum_loglike): the templates are never written, each walker's logL lands in its slot
of a device result vector, and the batch costs one host synchronisation. Otherwise (or with
fused_likelihood = False) each walker's template is reduced by efd_loglike (HIP) straight from
the template buffer, and the 2 x N_pos residual d - h w is never materialised. When the template is this package's
get_fd_waveform_fromFD around a GenerateEMRIWaveform (the drivers' case), h+ and hx are written
by efd_polarizations directly into one reusable [2][N_pos] buffer (the stream orders reuse), and
non_zero_mask is folded into the template weight (w * mask) instead of zeroing h.
The reference's other template mode, get_fd_waveform_fromTD around the TD GenerateEMRIWaveform
(emri_pe.py -template td), takes the same batched branch: groups of WINDOW_GROUP walkers, each
walker's windowed series h+ - i hx written by efd_td_modesum_windowed into one row of a shared
buffer, one batched complex transform, and efd_td_split_loglike reducing both channels' logL
straight from it (any window; non_zero_mask folded into w as above).
Results are numpy float64 arrays ([B]), or device tensors with use_gpu=True, return_cupy=True.
Likelihood.parts returns the pair the logL is made of instead, <d|h> (complex) and <h|h> per
walker with logL = -1/2 (d_d - 2 Re <d|h> + <h|h>): on the fused branches from the mode sum's
epilogue (efd_modesum_sum_dh_hh, no template written), elsewhere from the templates that branch
writes (efd_dh_hh_rows). separate_d_h=True (lisatools' flag) makes get_ll return that pair, and
ProfiledLikelihood turns it into the amplitude-maximised or distance-marginalised logL.
Likelihoods over time-domain DATA (dt only, no df or f_arr) are not part of this path: get_ll
raises NotImplementedError.
"""

import ctypes
import os
import sys

import numpy as np

from . import _lib
from .summation import require_gpu


class Likelihood:
    def __init__(self, template_model, num_channels, dt=None, df=None, f_arr=None,
                 parameter_transforms=None, use_gpu=False, vectorized=False,
                 separate_d_h=False, return_cupy=False, fill_data_noise=False,
                 transpose_params=False, subset=None):
        self.subset = subset
        self.transpose_params = transpose_params
        self.template_model = template_model
        self.parameter_transforms = parameter_transforms
        self.fill_data_noise = fill_data_noise
        self.use_gpu = use_gpu
        self.vectorized = vectorized
        self.num_channels = num_channels
        self.separate_d_h = separate_d_h
        if dt is None and df is None and f_arr is None:
            raise ValueError("Must provide dt, df or f_arr.")
        self.dt, self.df, self.f_arr = dt, df, f_arr
        self.frequency_domain = df is not None or f_arr is not None
        self.return_cupy = return_cupy
        self.noise_has_been_added = False
        self.noise_seed = None   # the seed of inject_signal(add_noise=True)'s realisation
        self.torch = torch = require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device())
        from .reductions import Reducer
        self._red = Reducer(self.device)
        self._buf = None
        # walkers whose templates are in flight at once in get_ll (WaveformPipeline slots);
        # one HIP stream each (the box exposes 4 hardware queues per process)
        self.num_streams = 4
        # pipelined templates on symmetric grids: the walkers' mode sums run FUSED_GROUP at a
        # time in one launch with the likelihood in its epilogue (efd_modesum_sum_loglike), so
        # no template is written; False keeps one template buffer + efd_loglike per walker
        self.fused_likelihood = True
        self._fused = None
        self._tile_const = None
        self._d_d = None
        self._specific_likelihood_setup()

    def _specific_likelihood_setup(self):
        if isinstance(self.template_model, list):
            raise ValueError("For single likelihood, template model cannot be a list.")
        if hasattr(self.template_model, "get_ll"):
            self.get_ll = self.template_model.get_ll
            self.like_here = False
        else:
            self.fill_data_noise = False
            self.like_here = True

    # ---------------------------------------------------------------------------------------
    def inject_signal(self, data_stream=None, params=None, waveform_kwargs={}, noise_fn=None,
                      noise_kwargs={}, add_noise=False, noise_seed=None):
        """lisatools' inject_signal. add_noise=True adds one stationary noise realisation to
        the data, once: a later injection into a likelihood that already has noise adds no
        second one (as the reference's guard, :183). The reference's recipe (:185-199) is
        n = sqrt(S) (0.5 / sqrt(df)) xi per bin, which in the weighted space d = x sqrt(df / S)
        is 0.5 xi on every bin whatever the PSD: efd_noise_fd adds it to the weighted data on
        the device (realisation 0 of the counter-based generator of include/emrifd.h, keyed on
        noise_seed, channel and bin). It works on df, f_arr and dt grids (the reference sets
        can_add_noise = False for f_arr, where its add_noise was a silent no-op; on such a grid
        df is diff_freqs). Bins the likelihood drops (w NaN or 0: f = 0 where the PSD is not
        finite, and bins outside the template's non_zero_mask) get no noise. noise_seed=None
        draws a seed from the OS and stores it in self.noise_seed; with more than one
        torch.distributed rank that raises ValueError, since the replicas' data would differ.
        noise_likelihood_factor is computed as the reference computes it (:202-207) and kept as
        an attribute; it is NOT added to logL (the reference marks it "TODO: need to check
        this", and it is a constant)."""
        torch = self.torch
        # the injection's parameters when the data is exactly the template model's output for
        # them (a single injection, no noise): the windowed logL's per-bin data is then made by
        # the logL's own arithmetic (get_fd_waveform_fromFD.hann_local)
        first = not hasattr(self, "injection_channels")
        self._inj_call = None
        if params is not None:
            if self.parameter_transforms is not None:
                key = list(self.parameter_transforms.keys())[0]
                params = self.parameter_transforms[key].both_transforms(params)
            injection_channels = _to_numpy(self.template_model(*params, **waveform_kwargs))
            if first:
                self._inj_call = (np.asarray(params, dtype=np.float64).reshape(-1),
                                  dict(waveform_kwargs))
        elif data_stream is not None:
            if isinstance(data_stream, list) is False:
                raise ValueError("If data_stream is provided, it must be as a list.")
            made_by = getattr(self.template_model, "made_by", None)
            if first and made_by is not None:
                self._inj_call = made_by(data_stream)
            injection_channels = _to_numpy(data_stream)
        else:
            raise ValueError("Must provide data_stream or params kwargs to inject signal.")

        self.injection_length = len(injection_channels[0])
        for inj in injection_channels:
            if len(inj) != self.injection_length:
                raise ValueError("Length of all injection channels must match.")
        if len(injection_channels) != self.num_channels:
            raise ValueError("Number of channels from template_model does not match number of "
                             "channels declare by user.")

        if isinstance(noise_fn, list):
            if len(noise_fn) != 1 and len(noise_fn) != self.num_channels:
                raise ValueError("Number of noise functions does not match number of channels "
                                 "declared by user.")
            elif len(noise_fn) == 1:
                noise_fn = [noise_fn[0] for _ in range(self.num_channels)]
        else:
            noise_fn = [noise_fn for _ in range(self.num_channels)]
        if isinstance(noise_kwargs, list):
            if len(noise_kwargs) != 1 and len(noise_kwargs) != self.num_channels:
                raise ValueError("Number of noise kwargs does not match number of channels "
                                 "declared by user.")
            elif len(noise_kwargs) == 1:
                noise_kwargs = [noise_kwargs[0] for _ in range(self.num_channels)]
        else:
            noise_kwargs = [noise_kwargs for _ in range(self.num_channels)]

        if self.frequency_domain:
            if self.df is not None:
                freqs = np.arange(self.injection_length) * self.df
                can_add_noise = True
            else:
                freqs = _to_numpy(self.f_arr)
                can_add_noise = True   # (False in the reference; df is diff_freqs here)
        else:
            freqs = np.fft.rfftfreq(self.injection_length, self.dt)
            can_add_noise = True
        psd = [np.asarray(_to_numpy(fn(freqs, **kw)), dtype=np.float64)
               for fn, kw in zip(noise_fn, noise_kwargs)]
        if self.frequency_domain is False:
            injection_channels = [np.fft.rfft(inj) * self.dt for inj in injection_channels]

        diff_freqs = np.zeros_like(freqs)
        diff_freqs[1:] = np.diff(freqs)
        diff_freqs[0] = diff_freqs[1]
        self.base_injections = injection_channels
        new_noise = bool(add_noise and can_add_noise and self.noise_has_been_added is False)
        if new_noise:
            if noise_seed is None:
                dist = getattr(torch, "distributed", None)
                if (dist is not None and dist.is_available() and dist.is_initialized()
                        and dist.get_world_size() > 1):
                    raise ValueError("inject_signal(add_noise=True) needs noise_seed when "
                                     "torch.distributed has more than one rank: the replicas' "
                                     "noise would differ")
                from .noise import new_seed
                noise_seed = new_seed()
            noise_seed = int(noise_seed)
            if not 0 <= noise_seed < 2 ** 64:
                raise ValueError("noise_seed: an integer in 0..2^64 - 1")

        with np.errstate(invalid="ignore", divide="ignore"):
            nf = np.asarray([(diff_freqs / p) ** 0.5 for p in psd])
        weighted = np.asarray([np.asarray(inj) * w for inj, w in zip(injection_channels, nf)],
                              dtype=np.complex128)
        self.noise_factor = torch.as_tensor(nf, dtype=torch.float64, device=self.device)
        if hasattr(self, "injection_channels") is False:
            self.injection_channels = torch.as_tensor(weighted, device=self.device)
            self.freqs = torch.as_tensor(freqs, dtype=torch.float64, device=self.device)
        else:
            self.injection_channels = self.injection_channels + torch.as_tensor(
                weighted, device=self.device)
        self.data_length = int(self.injection_channels.shape[1])
        self.psd = psd
        if new_noise:
            # 0.5 xi on every bin that carries weight, added to the weighted data in place
            self.noise_seed = noise_seed
            self.injection_channels = self.injection_channels.contiguous()
            self._red.noise_fd(self.injection_channels, noise_seed, 0, 0, self._noise_live(),
                               accumulate=True)
            with np.errstate(invalid="ignore"):
                self.noise_likelihood_factor = np.sum(
                    [1.0 / 2.0 * (2 * np.pi) * np.sum(diff_freqs * p) for p in psd])
            self.noise_has_been_added = True
        if self.noise_has_been_added:
            self._inj_call = None   # the data is no longer the template of any parameters
        self._prepare_reduction()   # (after the noise: drops the tile constants, d_d, _hloc)

    def _noise_live(self):
        """float64 [nchan][nbin]: 1 on the bins that carry noise, 0 on the bins the likelihood
        drops (noise factor NaN or 0, column 0 when w[0][0] is NaN, and bins outside the
        template's non_zero_mask)."""
        torch = self.torch
        w = self.noise_factor
        live = torch.isfinite(w) & (w != 0.0)
        if bool(torch.isnan(w[0, 0]).item()):
            live[:, 0] = False
        tm = self.template_model
        mask = getattr(tm, "non_zero_mask", None)
        if mask is not None and getattr(tm, "can_fill", False):
            live &= mask.to(device=self.device, dtype=torch.bool)[None, :]
        return live.to(torch.float64).contiguous()

    @property
    def noise_to_add(self):
        """The strain noise of the injection, sqrt(S) (0.5 / sqrt(df)) xi per channel and bin
        (the reference's attribute, :186-195), as a complex128 [nchan][nbin] device tensor
        regenerated from noise_seed on demand; 0 on the bins that carry no noise."""
        if not self.noise_has_been_added:
            raise AttributeError("noise_to_add: no noise has been added")
        torch = self.torch
        live = self._noise_live()
        gain = torch.where(live > 0.0, 1.0 / self.noise_factor, torch.zeros_like(live))
        out = torch.empty(tuple(live.shape), dtype=torch.complex128, device=self.device)
        return self._red.noise_fd(out, self.noise_seed, 0, 0, gain.contiguous())

    @property
    def noise_added_base_injections(self):
        """base_injections (the last injection's unweighted channels) plus noise_to_add, as a
        device tensor (the reference's attribute, :210), made on demand."""
        base = self.torch.as_tensor(np.asarray(self.base_injections, dtype=np.complex128),
                                    device=self.device)
        return base + self.noise_to_add

    def _prepare_reduction(self):
        """Device copies used by efd_loglike: skip bin 0 by zeroing it when w[0][0] is NaN."""
        torch = self.torch
        d = self.injection_channels.contiguous().clone()
        w = self.noise_factor.contiguous().clone()
        self.start_ind = 1 if bool(torch.isnan(self.noise_factor[0, 0]).item()) else 0
        if self.start_ind:
            d[:, 0] = 0.0
            w[:, 0] = 0.0
        self._d, self._w = d, w
        self._w_templ = w
        self._tile_const = None   # (their tile constants are made again on the next call)
        self._d_d = None          # (<d|d> too)
        self._hloc = None         # the windowed logL's per-bin data (made on the next call)
        tm = self.template_model
        mask = getattr(tm, "non_zero_mask", None)
        if mask is not None and getattr(tm, "can_fill", False):
            self._w_templ = (w * mask.to(torch.float64)[None, :]).contiguous()

    # ---------------------------------------------------------------------------------------
    @property
    def d_d(self):
        """<d|d> = 4 sum |d|^2 of the weighted data (efd_inner_product), made once per
        injection."""
        if self._d_d is None:
            self._d_d = float(self._red.inner(self._d, self._d).real.item())
        return self._d_d

    def parts(self, params, *args, **kwargs):
        """(<d|h>, <h|h>) of every walker: complex128 [B] and float64 [B] (numpy, or device
        tensors with use_gpu=True, return_cupy=True), with logL = -1/2 (d_d - 2 Re <d|h> +
        <h|h>) (inner_product(d, h, complex=True)'s convention). The branches are get_ll's: the
        fused ones take both numbers from the mode sum's epilogue (BatchPreparer.sum_dh_hh),
        the others reduce the templates they write anyway (Reducer.dh_hh_rows; the windowed and
        TD templates through fill_batch, a group of WINDOW_GROUP walkers per reduction)."""
        torch = self.torch
        if self.frequency_domain is False:
            raise NotImplementedError("a dt-only (time-domain data) likelihood is not part of "
                                      "the FD path")
        num_likes = params.shape[0]
        out = torch.empty((num_likes, 3), dtype=torch.float64, device=self.device)
        nch, nb = self._d.shape
        tm = self.template_model
        host = None
        if self.vectorized:
            h_all = tm(*params, *args, **kwargs)
            for i in range(num_likes):
                self._red.dh_hh_rows(self._as_channels(h_all[i]), self._d, self._w,
                                     out=out[i:i + 1])
        elif (getattr(tm, "can_pipeline", False)
              and (host := self._get_ll_fused(tm, params, args, kwargs, out, dh=True))
              is not None):
            pass
        elif getattr(tm, "can_pipeline", False):
            P = self._pipeline_for(tm)
            P.order_after_current()
            _prefetch(tm, params, args, kwargs)
            for i, params_i in enumerate(params):
                j = P.next_slot()
                slot = tm.submit(P, self._pbufs[j], *params_i, *args, order=False, **kwargs)
                with torch.cuda.stream(P.stream(slot)):
                    self._preds[slot].dh_hh_rows(self._pbufs[slot], self._d, self._w_templ,
                                                 out=out[i:i + 1])
            P.wait()
        elif getattr(tm, "can_fill_batch", False) and not args:
            G = min(max(1, int(os.environ.get("EFD_WINDOW_GROUP", 0))
                        or int(getattr(tm, "WINDOW_GROUP", 8))), _lib.EFD_DH_MAX_ROWS)
            rows = getattr(self, "_dh_rows", None)
            if rows is None or tuple(rows.shape) != (G, nch, nb):
                rows = self._dh_rows = torch.empty((G, nch, nb), dtype=torch.complex128,
                                                   device=self.device)
            _prefetch(tm, params, args, kwargs, concurrency=G if G < num_likes else None)
            for g0 in range(0, num_likes, G):
                m = len(params[g0:g0 + G])
                tm.fill_batch(rows[:m], params[g0:g0 + m], **kwargs)
                self._red.dh_hh_rows(rows[:m], self._d, self._w_templ, out=out[g0:g0 + m])
        elif getattr(tm, "can_fill", False):
            if self._buf is None or tuple(self._buf.shape) != (nch, nb):
                self._buf = torch.empty((nch, nb), dtype=torch.complex128, device=self.device)
            _prefetch(tm, params, args, kwargs)
            for i, params_i in enumerate(params):
                tm.fill(self._buf, *params_i, *args, **kwargs)
                self._red.dh_hh_rows(self._buf, self._d, self._w_templ, out=out[i:i + 1])
        else:
            for i, params_i in enumerate(params):
                h = self._as_channels(tm(*params_i, *args, **kwargs))
                self._red.dh_hh_rows(h, self._d, self._w, out=out[i:i + 1])
        if self.use_gpu and self.return_cupy:
            return torch.complex(out[:, 0], out[:, 1]), out[:, 2].clone()
        if host is None:
            host = out.cpu().numpy()
        return host[:, 0] + 1j * host[:, 1], host[:, 2].copy()

    def get_ll(self, params, *args, **kwargs):
        torch = self.torch
        if self.separate_d_h:
            return self.parts(params, *args, **kwargs)
        if self.frequency_domain is False:
            raise NotImplementedError("a dt-only (time-domain data) likelihood is not part of "
                                      "the FD path")
        num_likes = params.shape[0]
        out = torch.empty(num_likes, dtype=torch.float64, device=self.device)
        nch, nb = self._d.shape
        tm = self.template_model
        if self.vectorized:
            h_all = tm(*params, *args, **kwargs)
            for i in range(num_likes):
                h = self._as_channels(h_all[i])
                self._red.loglike(h, self._d, self._w, out=out[i:i + 1])
        elif (getattr(tm, "can_pipeline", False)
              and (host := self._get_ll_fused(tm, params, args, kwargs, out)) is not None):
            if self.use_gpu and self.return_cupy:
                return out
            return host
        elif getattr(tm, "can_pipeline", False):
            # several walkers in flight: each pipeline slot has its own template buffer,
            # stream and reduction scratch; walker i's template and logL run on one slot's
            # stream, the batch costs one host synchronisation
            P = self._pipeline_for(tm)
            P.order_after_current()
            _prefetch(tm, params, args, kwargs)
            for i, params_i in enumerate(params):
                j = P.next_slot()
                slot = tm.submit(P, self._pbufs[j], *params_i, *args, order=False, **kwargs)
                with torch.cuda.stream(P.stream(slot)):
                    self._preds[slot].loglike(self._pbufs[slot], self._d, self._w_templ,
                                              out=out[i:i + 1])
            P.wait()
        elif getattr(tm, "can_fill_batch", False) and not args:
            # windowed templates (the drivers' Hann window, or another of scipy's cosine-sum
            # windows: fdutils.COSINE_WINDOWS): groups of WINDOW_GROUP walkers,
            # their spectra in one buffer and the window's transforms batched over them
            # and the windowed templates' logL reduced in place (efd_hann_loglike or
            # efd_cosw_loglike, at most EFD_HANN_ROWS_MAX rows a call). TD templates
            # (get_fd_waveform_fromTD) group the same way: one transform per walker and
            # efd_td_split_loglike. The batch takes keyword waveform arguments only;
            # extra positional ones go to the per-walker fill below, which forwards them
            G = min(max(1, int(os.environ.get("EFD_WINDOW_GROUP", 0))
                        or int(getattr(tm, "WINDOW_GROUP", 8))), _lib.EFD_HANN_ROWS_MAX)
            scr = getattr(self, "_wscratch", None)
            per_row = max(_lib.EFD_LOGLIKE_SCRATCH, _lib.EFD_HANN_LOCAL_PARTIALS,
                          _lib.EFD_TD_SPLIT_SCRATCH)
            if scr is None or scr.numel() < G * per_row:
                scr = self._wscratch = torch.empty(G * per_row, dtype=torch.float64,
                                                   device=self.device)
            local = self._hann_local(tm, kwargs)
            # the upstream G walkers at a time, in order: the first group's device work then
            # overlaps the later walkers' upstream
            _prefetch(tm, params, args, kwargs, concurrency=G if G < num_likes else None)
            for g0 in range(0, num_likes, G):
                rows = params[g0:g0 + G]
                tm.loglike_batch(out[g0:g0 + len(rows)], rows, self._d, self._w_templ, scr,
                                 *args, local=local, **kwargs)
        elif getattr(tm, "can_fill", False):
            if self._buf is None or tuple(self._buf.shape) != (nch, nb):
                self._buf = torch.empty((nch, nb), dtype=torch.complex128, device=self.device)
            _prefetch(tm, params, args, kwargs)
            for i, params_i in enumerate(params):
                tm.fill(self._buf, *params_i, *args, **kwargs)
                self._red.loglike(self._buf, self._d, self._w_templ, out=out[i:i + 1])
        else:
            for i, params_i in enumerate(params):
                h = self._as_channels(tm(*params_i, *args, **kwargs))
                self._red.loglike(h, self._d, self._w, out=out[i:i + 1])
        if self.use_gpu and self.return_cupy:
            return out
        return out.cpu().numpy()

    # the windowed logL in its per-bin form, reduced inside the transforms' last pass
    # (efd_hann_loglike_local; False: efd_hann_loglike's mirror-pair form after the transforms)
    HANN_LOCAL = True

    def _hann_local(self, tm, kwargs):
        """The template model's per-bin windowed-logL data for this likelihood's d, w (made once
        per injection), or None."""
        hloc = getattr(self, "_hloc", None)
        if hloc is None:
            make = getattr(tm, "hann_local", None) if self.HANN_LOCAL else None
            inj = getattr(self, "_inj_call", None)
            if make is None:
                hloc = False
            elif inj is not None:
                hloc = make(self._d, self._w_templ, inj=inj[0], **inj[1]) or False
            else:
                hloc = make(self._d, self._w_templ, **kwargs) or False
            self._hloc = hloc
        return hloc or None

    # walkers per fused group (EFD_FUSED_GROUP overrides it: an experiment switch): one
    # efd_modesum_prepare_batch and one efd_modesum_sum_loglike each; FUSED_DEPTH groups rotate so group i+1's preparation runs beside group i's sum.
    # Balanced groups of at most 16 (EFD_BATCH_MAX): config 5's 64-walker half-steps (host-bound,
    # 43-tile grids) ran 54-60 k logL/s in 4 groups against 40-51 k in 8 (5 interleaved rounds);
    # config 4's 8 walkers are one group either way (groups of 4 or 3: -5 to -10%)
    FUSED_GROUP = min(max(1, int(os.environ.get("EFD_FUSED_GROUP", "16"))), 64)
    FUSED_DEPTH = max(1, int(os.environ.get("EFD_FUSED_DEPTH", "2")))
    # a group's staging, upload, preparation and fused sum in one native call
    # (BatchPreparer.flush_loglike, efd_fused_group); False: the Python steps of round 5
    FUSED_NATIVE_GROUP = True

    # amplitudes and mode selection on the device (pe.setup(upstream="device")): the fused
    # path's groups are fed by the generator's device_inputs_batch; False keeps the host upstream
    device_upstream = False
    # with device_upstream: the walkers' trajectories on the device too, all of a call's in one
    # launch ahead of the first group (pe.setup(trajectory="device"); efd_traj_batch)
    device_trajectory = False

    def _get_ll_fused(self, tm, params, args, kwargs, out, dh=False):
        """The pipelined path with the likelihood fused into the mode sum: per group of
        FUSED_GROUP walkers, the template chain collects each walker's host inputs
        (BatchPreparer), one upload and one efd_modesum_prepare_batch prepare the group on its
        stream, and one efd_modesum_sum_loglike right behind them on the same stream writes the
        group's log-likelihoods into its slice of out (the templates never reach HBM; a
        cross-stream wait between preparation and sum cost ~12 us of idle device per group on
        config 4's chain, tools/chain_timeline.py). A group's next flush is behind its sum in
        stream order; the streams join once, before the copy out.

        With device_upstream only the feed of a group differs: the walkers' trajectories start
        on the prefetch pool at once (device_trajectory: all of them in one launch on the
        current stream instead); per balanced group of at most EFD_BATCH_MAX walkers the
        generator's device_inputs_batch (packed trajectory upload, efd_modes_select_batch, the
        read of the group's K) runs on the group's stream and BatchPreparer.flush_device
        prepares the group from what it left on the device, so a group's device chain runs
        beside the next group's trajectories and selection. The groups live in the host
        route's preparer: a Likelihood switched between the routes keeps its workspaces.

        Returns the log-likelihoods on the host (one synchronisation per batch), or None,
        before queueing anything, when the template's grid is not symmetric, or neither route
        applies (fused_likelihood off; the device route needs a GenerateEMRIWaveform, keyword
        waveform arguments and no explicit mode list, and otherwise leaves the walkers to the
        host route): the caller then takes the per-walker path. A walker whose preparation or
        sum raised a device-side error comes back NaN from the kernel
        (efd_modesum_sum_loglike), and only then are the groups' status flags read, which
        raises.

        dh (Likelihood.parts): out is [n][3] and every group's sum is BatchPreparer.sum_dh_hh
        behind the Python steps (flush / flush_device), which needs no tile constants; the
        host result is [n][3]."""
        torch = self.torch
        from .summation import BatchPreparer
        from .waveform import GenerateEMRIWaveform
        few = getattr(tm, "waveform_generator", None)
        device = (self.device_upstream and not args and isinstance(few, GenerateEMRIWaveform)
                  and kwargs.get("mode_selection") is None)
        if not (device or self.fused_likelihood) or not self._fused_grid_ok(tm, kwargs):
            return None
        if device:
            cw = few.waveform_generator.create_waveform
            freq, _ = cw._grid(kwargs.get("T", 1.0), kwargs.get("dt", 10.0), kwargs.get("f_arr"))
            k0 = cw.positive_start()
            if getattr(tm, "_suffix_k0", k0) != k0:
                raise ValueError("positive_frequency_mask does not match the generator's grid")
        else:
            _prefetch(tm, params, args, kwargs)
        n = len(params)
        per = 3 if dh else 1     # doubles per walker in out
        if n == 0:
            return np.empty((0, 3) if dh else 0, dtype=np.float64)
        ngroups = -(-n // (_lib.EFD_BATCH_MAX if device else self.FUSED_GROUP))
        G = -(-n // ngroups)                       # balanced groups of at most that many
        caustic = getattr(getattr(getattr(tm.waveform_generator, "waveform_generator", None),
                                  "create_waveform", None), "caustic", "uniform")
        F = self._fused
        if F is None or F["prep"].caustic != caustic or F["prep"].group < G:
            B = BatchPreparer(max(G, self.FUSED_GROUP), self.FUSED_DEPTH, caustic=caustic,
                              device=self.device)
            # the group streams' handles, for the orderings below (efd_stream_order: one event
            # record and one stream wait each, in C)
            F = self._fused = dict(prep=B, gst=[B.stream(gi).cuda_stream
                                                for gi in range(len(B.groups))])
        B, gst = F["prep"], F["gst"]
        lib = B.lib
        # the device route's trajectories: on the prefetch pool, or all of them in one launch on
        # the current stream, which the groups' streams are ordered after below
        futs, trajs = [], None
        if device:
            B.restart()
            calls, scales = few.device_calls(params, kwargs.get("T", 1.0),
                                             kwargs.get("eps", 1e-5))
            if self.device_trajectory:
                trajs = few.device_trajectories(calls, self.device, F.setdefault("traj", {}))
            else:
                futs = few.waveform_generator.trajectories_async(calls)
        # the group streams this batch's flushes take (B's rotation from its next group), after
        # the work queued so far on the current stream: one stream wait each
        key = ("ord", gst.index(B.next_flush()[0].cuda_stream), min(ngroups, len(gst)))
        arr = F.get(key)
        if arr is None:
            arr = F[key] = (ctypes.c_void_p * key[2])(
                *[gst[(key[1] + k) % len(gst)] for k in range(key[2])])
        _lib.check(lib.efd_stream_order(torch.cuda.current_stream(self.device).cuda_stream,
                                        arr, len(arr)), "efd_stream_order", lib)
        pin = F.get("pin")
        if pin is None or pin.numel() < per * n:
            pin = F["pin"] = torch.empty(max(per * n, 64), dtype=torch.float64, pin_memory=True)
        native = self.FUSED_NATIVE_GROUP and hasattr(lib, "efd_fused_group") and not dh
        used = []
        try:
            batch = getattr(tm, "submit_batch", None)
            for g0 in range(0, n, G):
                g = slice(g0, g0 + G)
                if device:
                    sst = B.next_flush()[0]
                    inps = few.waveform_generator.device_inputs_batch(
                        calls[g], include_minus_m=bool(kwargs.get("include_minus_m", True)),
                        device=self.device, stream=sst, state=B.next_select(),
                        futures=futs[g] if trajs is None else None,
                        trajs=trajs[g] if trajs is not None else None)
                    gi, jobs = B.flush_device(inps, freq, scales[g], k0)
                else:
                    if batch is not None:
                        batch(B, params[g], *args, **kwargs)
                    else:
                        for i in range(g0, min(n, g0 + G)):
                            tm.submit(B, None, *params[i], *args, order=False,
                                      prepare_only=True, **kwargs)
                    sst, freq, k0 = B.next_flush()
                    if native:
                        # the tile constants are made on the group's stream (once per grid),
                        # before the sum that reads them
                        tc = self._tile_constants(freq, k0, sst, B)
                        used.append(B.flush_loglike(self._d, self._w_templ, out, tile_const=tc,
                                                    out_off=g0))
                        continue
                    gi, jobs = B.flush()
                used.append(gi)
                if dh:
                    B.sum_dh_hh(gi, self._d, self._w_templ, out[g0:g0 + len(jobs)],
                                sst.cuda_stream)
                    continue
                tc = self._tile_constants(freq, k0, sst, B)
                B.sum_loglike(gi, self._d, self._w_templ, out[g0:g0 + len(jobs)],
                              sst.cuda_stream, tile_const=tc)
            # the other groups' streams join the last one, which copies out
            last = used[-1]
            for gj in sorted(set(used) - {last}):
                _lib.check(lib.efd_stream_order(gst[gj], (ctypes.c_void_p * 1)(gst[last]), 1),
                           "efd_stream_order", lib)
            _lib.check(lib.efd_download(pin.data_ptr(), out.data_ptr(), 8 * per * n, gst[last]),
                       "efd_download", lib)
        finally:
            for f in futs:
                f.cancel()
            B.drop_pending()
            # `out` belongs to the current stream: nothing may still write it when it is
            # returned, or freed after an exception
            if sys.exc_info()[0] is not None:
                # a failure inside a flush (staging, workspace growth, the selection, the
                # preparation) may leave a group's work queued before that group reached
                # `used`: wait for every group stream, not only the recorded ones
                for gi in range(len(gst)):
                    B.stream(gi).synchronize()
            elif used:
                B.stream(used[-1]).synchronize()
        host = pin[:per * n].numpy().copy()
        if dh:
            host = host.reshape(n, 3)
        if np.isnan(host).any():
            B.wait()   # device-side errors of the groups' workspaces (sticky across reuse)
        return host

    # tiles no harmonic reaches take a precomputed partial instead of re-reading d and w
    # (efd_loglike_tile_constants; bitwise the same logL)
    fused_tile_constants = True

    def _tile_constants(self, freq, k0, stream, prep):
        """The fused sum's per-tile constants for (d, w_templ) on this grid, made once on
        `stream`, a group's (ordered after the data's creation: it waits on the current
        stream). Every group stream of the BatchPreparer `prep` is then ordered after `stream`,
        so any group's later sum may read them."""
        if not self.fused_tile_constants:
            return None
        from .summation import loglike_tile_constants
        nf, k0 = int(freq.numel()), int(k0)
        key = (nf, k0, id(self._d), id(self._w_templ))
        tc = self._tile_const
        if tc is None or tc[0] != key:
            tc = self._tile_const = (key, loglike_tile_constants(
                self._d, self._w_templ, nf, k0, stream.cuda_stream))
            order = [g.stream.cuda_stream for g in prep.groups]
            _lib.check(prep.lib.efd_stream_order(
                stream.cuda_stream, (ctypes.c_void_p * len(order))(*order), len(order)),
                "efd_stream_order", prep.lib)
        return tc[1]

    def _fused_grid_ok(self, tm, kwargs):
        """Whether the template's grid for these kwargs is mirror-symmetric (the fused sum's
        requirement); set up once per grid, without queueing any device work."""
        cw = getattr(getattr(getattr(tm, "waveform_generator", None), "waveform_generator", None),
                     "create_waveform", None)
        if cw is None or not hasattr(cw, "_grid"):
            return False
        _, sym = cw._grid(kwargs.get("T", 1.0), kwargs.get("dt", 10.0), kwargs.get("f_arr"))
        return bool(sym)

    def _pipeline_for(self, tm):
        """The WaveformPipeline (self.num_streams slots) and per-slot buffers of get_ll."""
        torch = self.torch
        from .reductions import Reducer
        from .summation import WaveformPipeline
        nch, nb = self._d.shape
        caustic = getattr(getattr(getattr(tm.waveform_generator, "waveform_generator", None),
                                  "create_waveform", None), "caustic", "uniform")
        P = getattr(self, "_pipe", None)
        if P is None or P.caustic != caustic:
            P = self._pipe = WaveformPipeline(self.num_streams, caustic=caustic,
                                              device=self.device)
            self._pbufs = [None] * P.num_slots
            self._preds = [Reducer(self.device) for _ in range(P.num_slots)]
        for j in range(P.num_slots):
            if self._pbufs[j] is None or tuple(self._pbufs[j].shape) != (nch, nb):
                with torch.cuda.stream(P.stream(j)):
                    self._pbufs[j] = torch.empty((nch, nb), dtype=torch.complex128,
                                                 device=self.device)
        return P

    def _as_channels(self, chans):
        torch = self.torch
        if hasattr(chans, "detach") and chans.dim() == 2:
            h = chans
        else:
            h = torch.stack([torch.as_tensor(c, device=self.device) for c in chans])
        h = h.to(device=self.device, dtype=torch.complex128).contiguous()
        if tuple(h.shape) != tuple(self._d.shape):
            raise ValueError(f"template has shape {tuple(h.shape)}, data {tuple(self._d.shape)}")
        return h

    def __call__(self, params, *args, **kwargs):
        if not isinstance(params, np.ndarray):
            raise ValueError("params must be np.ndarray.")
        if self.parameter_transforms is not None:
            key = list(self.parameter_transforms.keys())[0]
            params = self.parameter_transforms[key].both_transforms(params)
        if self.transpose_params:
            params = params.T
            subset_axis = 1
        else:
            subset_axis = 0
        num_likes = params.shape[subset_axis]
        inds_likes = np.arange(num_likes)
        if self.subset is not None:
            if not isinstance(self.subset, int):
                raise ValueError("Subset must be int.")
            inds_subset = np.split(inds_likes, np.arange(self.subset, num_likes, self.subset))
        else:
            inds_subset = [inds_likes]
        out_ll = []
        for inds in inds_subset:
            args_in = (params[inds],) if subset_axis == 0 else (params[:, inds],)
            args_in += args
            if self.fill_data_noise:
                args_in += (self.injection_channels, self.noise_factor)
            out_ll.append(_to_numpy(self.get_ll(*args_in, **kwargs)))
        if self.separate_d_h:   # (<d|h>, <h|h>) per subset: each concatenated on its own
            return tuple(np.concatenate([o[k] for o in out_ll], axis=0) for k in range(2))
        return np.concatenate(out_ll, axis=0)


def _prefetch(tm, params, args, kwargs, concurrency=None):
    """The batch's host upstream on the pool. Without waiting when the template supports it
    (PREFETCH_ASYNC): each walker's template then waits for its own upstream only, so the first
    groups' device work runs while the pool computes the later walkers' (concurrency: at most
    that many walkers' upstream at once, in order)."""
    if not hasattr(tm, "prefetch"):
        return
    if getattr(tm, "PREFETCH_ASYNC", False) and os.environ.get("EFD_PREFETCH_ASYNC", "1") != "0":
        if concurrency:
            tm.prefetch(params, *args, wait=False, concurrency=concurrency, **kwargs)
        else:
            tm.prefetch(params, *args, wait=False, **kwargs)
    else:
        tm.prefetch(params, *args, **kwargs)


def _to_numpy(x):
    if isinstance(x, (list, tuple)):
        return [_to_numpy(v) for v in x]
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


# ---- what the (<d|h>, <h|h>) pair is for: host arithmetic on float64 arrays [B] ---------------
def profile_none(d_d, re_dh, h_h):
    """logL = -1/2 (d_d - 2 Re <d|h> + <h|h>)."""
    return -0.5 * (d_d - 2.0 * np.asarray(re_dh, dtype=np.float64)
                   + np.asarray(h_h, dtype=np.float64))


def profile_amplitude(d_d, re_dh, h_h):
    """The logL maximised over an overall amplitude A >= 0 of the template, in closed form:
    (-1/2 d_d + 1/2 max(Re <d|h>, 0)^2 / <h|h>, A_hat = max(Re <d|h>, 0) / <h|h>); a walker
    with <h|h> = 0 (no template) has A_hat = 0 and no gain."""
    re = np.maximum(np.asarray(re_dh, dtype=np.float64), 0.0)
    hh = np.asarray(h_h, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(hh > 0.0, re / hh, 0.0)
    return -0.5 * d_d + 0.5 * re * A, A


# k of the break points u* +- k sigma of the distance quadrature's panels
_PEAK_K = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 16.0, 24.0, 40.0)
_PANEL_MAX = 0.25    # the widest panel in log u
DISTANCE_NODES = 16  # Gauss-Legendre nodes per panel


def _distance_panels(re, hh, u_lo, u_hi):
    """The panels' break points in t = log u for one walker: the range's ends, the Gaussian
    factor's u* +- k sigma (u* = Re <d|h> / <h|h>, sigma = <h|h>^(-1/2)), a geometric ladder in
    from each end at that end's decay length 1 / |Re <d|h> - u <h|h>| (a peak far outside the
    range leaves an exponential against the nearer end), and a uniform split of what is still
    wider than _PANEL_MAX."""
    pts = [u_lo, u_hi]
    if hh > 0.0:
        us, sg = re / hh, hh ** -0.5
        for k in _PEAK_K:
            pts += [us - k * sg, us + k * sg]
        pts.append(us)
    for edge, sign in ((u_lo, 1.0), (u_hi, -1.0)):
        slope = abs(re - edge * hh)
        if slope > 0.0:
            step = 1.0 / slope
            while step < u_hi - u_lo:
                pts.append(edge + sign * step)
                step *= 2.0
    t = np.log(np.unique(np.clip(np.asarray(pts, dtype=np.float64), u_lo, u_hi)))
    out = [t[:1]]
    for a, b in zip(t[:-1], t[1:]):
        m = max(1, int(np.ceil((b - a) / _PANEL_MAX)))
        out.append(a + (b - a) * np.arange(1, m + 1) / m)
    return np.concatenate(out)


def marginalize_distance(d_d, re_dh, h_h, dist_ref, dist_range, prior_power=2,
                         nodes=DISTANCE_NODES):
    """log of the likelihood marginalised over the distance D of a template made at dist_ref,
      log int pi(D) exp(-1/2 d_d + u Re <d|h> - 1/2 u^2 <h|h>) dD,  u = dist_ref / D,
    with pi proportional to D^prior_power, normalised on dist_range = (lo, hi). Per walker a
    composite Gauss-Legendre rule in t = log u (dD = -D dt: the power-law prior and Jacobian are
    smooth there) over _distance_panels' panels, `nodes` nodes each, summed in log-sum-exp form:
    finite for <h|h> = 0 (the integrand is then the prior alone, log = -1/2 d_d) and for peaks
    of any height."""
    re = np.atleast_1d(np.asarray(re_dh, dtype=np.float64))
    hh = np.atleast_1d(np.asarray(h_h, dtype=np.float64))
    lo, hi = float(dist_range[0]), float(dist_range[1])
    if not (0.0 < lo < hi) or not dist_ref > 0.0:
        raise ValueError("marginalize_distance: 0 < lo < hi and dist_ref > 0")
    p = float(prior_power)
    # log of the prior's norm int_lo^hi D^p dD, with D in units of hi (no overflow)
    lognorm = (np.log(np.log(hi / lo)) if p == -1.0
               else np.log((1.0 - (lo / hi) ** (p + 1.0)) / (p + 1.0))) + (p + 1.0) * np.log(hi)
    u_lo, u_hi = dist_ref / hi, dist_ref / lo
    x, wq = np.polynomial.legendre.leggauss(int(nodes))
    out = np.empty(len(re), dtype=np.float64)
    for i in range(len(re)):
        t = _distance_panels(re[i], hh[i], u_lo, u_hi)
        a, b = t[:-1, None], t[1:, None]
        tt = 0.5 * (a + b) + 0.5 * (b - a) * x[None, :]
        ww = 0.5 * (b - a) * wq[None, :]
        u = np.exp(tt)
        # pi(D) dD = D^(p + 1) dt / norm, D = dist_ref / u
        L = np.log(ww) + (p + 1.0) * (np.log(dist_ref) - tt) + u * re[i] - 0.5 * u * u * hh[i]
        m = L.max()
        out[i] = m + np.log(np.exp(L - m).sum()) - lognorm
    return -0.5 * d_d + out


class ProfiledLikelihood:
    """A Likelihood's logL with the template's overall amplitude (the source's distance) taken
    out, from Likelihood.parts' pair: a callable (params, **kwargs) -> float64 [B] that a sampler
    takes as its log-likelihood. The parameters go through the likelihood's own __call__ (its
    transforms and subset batching).

    mode: "none", -1/2 (d_d - 2 Re <d|h> + <h|h>): the plain logL from the pair;
          "amplitude", profile_amplitude's closed form; `last` then holds A_hat and, with
            dist_ref, D_hat = dist_ref / A_hat of the last call;
          "distance", marginalize_distance over dist_range with the prior D^prior_power, the
            templates being made at distance dist_ref.
    snr(params, **kwargs) returns (sqrt <h|h>, Re <d|h> / sqrt <h|h>): the optimal and the
    matched-filter SNR of every walker."""

    MODES = ("none", "amplitude", "distance")

    def __init__(self, like, mode, dist_ref=None, dist_range=None, prior_power=2):
        if mode not in self.MODES:
            raise ValueError(f"mode: one of {self.MODES}")
        if mode == "distance" and (dist_ref is None or dist_range is None):
            raise ValueError("mode 'distance' needs dist_ref and dist_range")
        self.like, self.mode = like, mode
        self.dist_ref, self.dist_range, self.prior_power = dist_ref, dist_range, prior_power
        self.last = {}

    def parts(self, params, **kwargs):
        """(<d|h> complex128 [B], <h|h> float64 [B]) through the likelihood's __call__."""
        like = self.like
        keep = like.separate_d_h
        like.separate_d_h = True
        try:
            d_h, h_h = like(params, **kwargs)
        finally:
            like.separate_d_h = keep
        return d_h, h_h

    def combine(self, d_d, d_h, h_h):
        """The mode's logL from given numbers (host arithmetic only)."""
        re = np.real(d_h)
        if self.mode == "none":
            return profile_none(d_d, re, h_h)
        if self.mode == "amplitude":
            ll, A = profile_amplitude(d_d, re, h_h)
            self.last = {"A_hat": A}
            if self.dist_ref is not None:
                with np.errstate(divide="ignore"):
                    self.last["D_hat"] = np.where(A > 0.0, self.dist_ref / A, np.inf)
            return ll
        return marginalize_distance(d_d, re, h_h, self.dist_ref, self.dist_range,
                                    self.prior_power)

    def __call__(self, params, **kwargs):
        d_h, h_h = self.parts(params, **kwargs)
        return self.combine(self.like.d_d, d_h, h_h)

    def snr(self, params, **kwargs):
        d_h, h_h = self.parts(params, **kwargs)
        rho = np.sqrt(h_h)
        with np.errstate(divide="ignore", invalid="ignore"):
            return rho, np.where(rho > 0.0, np.real(d_h) / rho, 0.0)
