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

What changes is where the work happens. Data and noise factor live on the device, and the
2 x N_pos residual d - h w is never materialised. Results are numpy float64 arrays ([B]), or
device tensors with use_gpu=True, return_cupy=True. Likelihood.parts returns the pair the logL
is made of instead, <d|h> (complex) and <h|h> per walker with logL = -1/2 (d_d - 2 Re <d|h> +
<h|h>); separate_d_h=True (lisatools' flag) makes get_ll return that pair, and
ProfiledLikelihood (profiled.py, re-exported here) turns it into the amplitude-maximised or
distance-marginalised logL. Likelihoods over time-domain DATA (dt only, no df or f_arr) are not
part of this path: get_ll raises NotImplementedError.

Routing. get_ll and parts hand Likelihood._run an output kind (LOGL or PAIR, below the class),
and _run takes the branch choose_branch names from the template model's flags:
  pipelined     get_fd_waveform_fromFD around a GenerateEMRIWaveform (the drivers' case). On
                symmetric grids (FEW's own and the drivers' downsampled f_arr) the walkers' mode
                sums run a group at a time in one launch with the reduction in the sum's
                epilogue (efd_modesum_sum_loglike, efd_modesum_sum_dh_hh): no template is
                written, and the batch costs one host synchronisation (_run_fused: _fused_route
                picks the feed, waveform._HostFeed or _DeviceFeed, which the batched generator
                shares; _fused_preparer holds the BatchPreparer; _fused_drive runs the groups
                through summation.run_groups, joins their streams and copies out). Otherwise, or
                with fused_likelihood = False, h+ and hx are written by efd_polarizations into
                one reusable [2][N_pos] buffer per pipeline slot and reduced from it
                (efd_loglike, efd_dh_hh_rows).
  window_batch  windowed templates, and get_fd_waveform_fromTD around the TD GenerateEMRIWaveform
                (emri_pe.py -template td): groups of WINDOW_GROUP walkers, their series in the
                rows of one buffer (TD: h+ - i hx by efd_td_modesum_windowed), one batched
                transform, and the logL reduced straight from it (efd_hann_loglike,
                efd_td_split_loglike), or the rows written (fill_batch) for efd_dh_hh_rows.
  fill, call, vectorized   one template at a time into a buffer, or as the model returns it.
Where the model fills a buffer, non_zero_mask is folded into the template weight (w * mask)
instead of zeroing h.
"""

import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np

from . import _lib
from .noise import check_seed, new_seed
from .profiled import (DISTANCE_NODES, ProfiledLikelihood, marginalize_distance,  # noqa: F401
                       profile_amplitude, profile_none)
from .reductions import Reducer
from .summation import (BatchPreparer, WaveformPipeline, loglike_tile_constants, require_gpu,
                        run_groups)
from .waveform import GenerateEMRIWaveform, _DeviceFeed, _HostFeed


def choose_branch(tm, vectorized, has_args):
    """The branch Likelihood._run takes, from the template model's flags alone (the output kind
    plays no part, no GPU state is touched). vectorized: the likelihood's flag; has_args: whether
    positional waveform arguments were passed (the windowed batch takes keyword ones only, the
    per-walker fill forwards them). "pipelined" is the fused groups or the per-slot pipeline."""
    if vectorized:
        return "vectorized"
    if getattr(tm, "can_pipeline", False):
        return "pipelined"
    if getattr(tm, "can_fill_batch", False) and not has_args:
        return "window_batch"
    if getattr(tm, "can_fill", False):
        return "fill"
    return "call"


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
        self._red = Reducer(self.device)
        self._buf = None
        self.branch_taken = None   # the branch of the last get_ll / parts (see _run)
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

        noise_fn = _per_channel(noise_fn, self.num_channels, "noise functions")
        noise_kwargs = _per_channel(noise_kwargs, self.num_channels, "noise kwargs")

        if self.df is not None:
            freqs = np.arange(self.injection_length) * self.df
        elif self.frequency_domain:
            # (the reference sets can_add_noise = False here; df is diff_freqs on this grid)
            freqs = _to_numpy(self.f_arr)
        else:
            freqs = np.fft.rfftfreq(self.injection_length, self.dt)
        psd = [np.asarray(_to_numpy(fn(freqs, **kw)), dtype=np.float64)
               for fn, kw in zip(noise_fn, noise_kwargs)]
        if self.frequency_domain is False:
            injection_channels = [np.fft.rfft(inj) * self.dt for inj in injection_channels]

        diff_freqs = np.zeros_like(freqs)
        diff_freqs[1:] = np.diff(freqs)
        diff_freqs[0] = diff_freqs[1]
        self.base_injections = injection_channels
        new_noise = bool(add_noise and self.noise_has_been_added is False)
        if new_noise:
            if noise_seed is None:
                dist = getattr(torch, "distributed", None)
                if (dist is not None and dist.is_available() and dist.is_initialized()
                        and dist.get_world_size() > 1):
                    raise ValueError("inject_signal(add_noise=True) needs noise_seed when "
                                     "torch.distributed has more than one rank: the replicas' "
                                     "noise would differ")
                noise_seed = new_seed()
            noise_seed = check_seed(noise_seed)

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
        mask = self._template_mask()
        if mask is not None:
            live &= mask.to(device=self.device, dtype=torch.bool)[None, :]
        return live.to(torch.float64).contiguous()

    def _template_mask(self):
        """The template model's non_zero_mask where it is folded into the template weight and
        its bins dropped from the likelihood (models that fill a buffer), or None."""
        tm = self.template_model
        mask = getattr(tm, "non_zero_mask", None)
        return mask if getattr(tm, "can_fill", False) else None

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
        mask = self._template_mask()
        if mask is not None:
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
        return self._run(PAIR, params, args, kwargs)

    def get_ll(self, params, *args, **kwargs):
        return self._run(PAIR if self.separate_d_h else LOGL, params, args, kwargs)

    def _run(self, kind, params, args, kwargs):
        """The branch ladder, walked once for either output kind: the _branch_* method that
        choose_branch names fills `out`, one slot per walker, and returns the host copy if it
        already has one (the fused groups' pinned download). branch_taken names the branch that
        ran ("pipelined" resolved to "fused" or "per_slot")."""
        if self.frequency_domain is False:
            raise NotImplementedError("a dt-only (time-domain data) likelihood is not part of "
                                      "the FD path")
        tm = self.template_model
        out = self.torch.empty((params.shape[0], *kind.tail), dtype=self.torch.float64,
                               device=self.device)
        self.branch_taken = name = choose_branch(tm, self.vectorized, bool(args))
        host = getattr(self, "_branch_" + name)(kind, tm, params, args, kwargs, out)
        if self.use_gpu and self.return_cupy:
            return kind.device(self, out)
        return kind.host(out.cpu().numpy() if host is None else host)

    def _branch_vectorized(self, kind, tm, params, args, kwargs, out):
        h_all = tm(*params, *args, **kwargs)
        for i in range(params.shape[0]):
            kind.reduce(self._red, self._as_channels(h_all[i]), self._d, self._w,
                        out=out[i:i + 1])

    def _branch_pipelined(self, kind, tm, params, args, kwargs, out):
        """The fused groups where they apply, else num_streams walkers in flight: a walker's
        template and reduction run on its slot's stream, with the slot's buffer and scratch;
        the batch costs one host synchronisation."""
        host = self._run_fused(kind, tm, params, args, kwargs, out)
        self.branch_taken = "per_slot" if host is None else "fused"
        if host is not None:
            return host
        P = self._pipeline_for(tm)
        P.order_after_current()
        _prefetch(tm, params, args, kwargs)
        for i, params_i in enumerate(params):
            j = P.next_slot()
            slot = tm.submit(P, self._pbufs[j], *params_i, *args, order=False, **kwargs)
            with self.torch.cuda.stream(P.stream(slot)):
                kind.reduce(self._preds[slot], self._pbufs[slot], self._d, self._w_templ,
                            out=out[i:i + 1])
        P.wait()

    def _branch_window_batch(self, kind, tm, params, args, kwargs, out):
        """Windowed (Hann, or another of fdutils.COSINE_WINDOWS) and TD templates: groups of G
        walkers, the transforms batched over a group; kind.window is what becomes of one."""
        n = params.shape[0]
        G = _window_group(tm, kind.window_cap)
        group = kind.window(self, tm, G, kwargs)
        # the upstream G walkers at a time, in order: the first group's device work then
        # overlaps the later walkers' upstream
        _prefetch(tm, params, args, kwargs, concurrency=G if G < n else None)
        for g0 in range(0, n, G):
            rows = params[g0:g0 + G]
            group(out[g0:g0 + len(rows)], rows)

    def _window_loglike(self, tm, G, kwargs):
        """LOGL's windowed action: the template model reduces the group's logL in place
        (efd_hann_loglike, efd_cosw_loglike or efd_td_split_loglike; EFD_HANN_ROWS_MAX rows)."""
        scr = getattr(self, "_wscratch", None)
        per_row = max(_lib.EFD_LOGLIKE_SCRATCH, _lib.EFD_HANN_LOCAL_PARTIALS,
                      _lib.EFD_TD_SPLIT_SCRATCH)
        if scr is None or scr.numel() < G * per_row:
            scr = self._wscratch = self.torch.empty(G * per_row, dtype=self.torch.float64,
                                                    device=self.device)
        local = self._hann_local(tm, kwargs)
        return lambda out_g, rows: tm.loglike_batch(out_g, rows, self._d, self._w_templ, scr,
                                                    local=local, **kwargs)

    def _window_rows(self, tm, G, kwargs):
        """PAIR's windowed action: the group's templates written as rows, then one
        efd_dh_hh_rows over them (EFD_DH_MAX_ROWS rows)."""
        shape = (G, *self._d.shape)
        buf = getattr(self, "_dh_rows", None)
        if buf is None or tuple(buf.shape) != shape:
            buf = self._dh_rows = self.torch.empty(shape, dtype=self.torch.complex128,
                                                   device=self.device)

        def group(out_g, rows):
            tm.fill_batch(buf[:len(rows)], rows, **kwargs)
            self._red.dh_hh_rows(buf[:len(rows)], self._d, self._w_templ, out=out_g)
        return group

    def _branch_fill(self, kind, tm, params, args, kwargs, out):
        shape = tuple(self._d.shape)
        if self._buf is None or tuple(self._buf.shape) != shape:
            self._buf = self.torch.empty(shape, dtype=self.torch.complex128, device=self.device)
        _prefetch(tm, params, args, kwargs)
        for i, params_i in enumerate(params):
            tm.fill(self._buf, *params_i, *args, **kwargs)
            kind.reduce(self._red, self._buf, self._d, self._w_templ, out=out[i:i + 1])

    def _branch_call(self, kind, tm, params, args, kwargs, out):
        for i, params_i in enumerate(params):
            h = self._as_channels(tm(*params_i, *args, **kwargs))
            kind.reduce(self._red, h, self._d, self._w, out=out[i:i + 1])

    # the windowed logL in its per-bin form, reduced inside the transforms' last pass
    # (efd_hann_loglike_local; False: efd_hann_loglike's mirror-pair form after the transforms)
    HANN_LOCAL = True

    def _hann_local(self, tm, kwargs):
        """The template model's per-bin windowed-logL data for this likelihood's d, w (made once
        per injection), or None."""
        if getattr(self, "_hloc", None) is None:
            make = getattr(tm, "hann_local", None) if self.HANN_LOCAL else None
            inj = getattr(self, "_inj_call", None)
            if make is not None and inj is not None:
                kwargs = dict(inj[1], inj=inj[0])
            self._hloc = make is not None and make(self._d, self._w_templ, **kwargs) or False
        return self._hloc or None

    # walkers per fused group (EFD_FUSED_GROUP overrides it: an experiment switch): one
    # efd_modesum_prepare_batch and one efd_modesum_sum_loglike each; FUSED_DEPTH groups rotate
    # so group i+1's preparation runs beside group i's sum.
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

    def _run_fused(self, kind, tm, params, args, kwargs, out):
        """The reduction fused into the mode sum: per balanced group of walkers, the feed puts
        the group's inputs on a group stream, one efd_modesum_prepare_batch prepares it there,
        and kind.fused_sum right behind it on the same stream writes the group's slice of out
        (no template reaches HBM; a cross-stream wait between preparation and sum cost ~12 us of
        idle device per group on config 4's chain, tools/chain_timeline.py). On the host route
        LOGL's group is one native call instead (flush_loglike, efd_fused_group). Both routes'
        groups live in one preparer: a Likelihood switched between them keeps its workspaces.
        Returns the result on the host, [n, *kind.tail] (one synchronisation per batch), or
        None, before queueing anything, when no route applies: the caller then takes the
        per-walker path."""
        route = self._fused_route(tm, args, kwargs)
        if route is None:
            return None
        n = len(params)
        if n == 0:
            return np.empty((0, *kind.tail), dtype=np.float64)
        ngroups = -(-n // (_lib.EFD_BATCH_MAX if route == "device" else self.FUSED_GROUP))
        G = -(-n // ngroups)                       # balanced groups of at most that many
        F = self._fused_preparer(tm, G)
        B = F.prep
        if route == "device":
            feed = _DeviceFeed(B, tm.waveform_generator, params, kwargs, self.device,
                               self.device_trajectory, F.traj, k0=getattr(tm, "_suffix_k0", None))
        else:
            feed = _HostFeed(B, params, getattr(tm, "submit_batch", None),
                             getattr(tm, "submit", None), args, kwargs,
                             prefetch=lambda p, *a, **k: _prefetch(tm, p, a, k))
        self._order_group_streams(F, ngroups)
        if (kind.native_group and route == "host" and self.FUSED_NATIVE_GROUP
                and hasattr(B.lib, "efd_fused_group")):
            def step(g0, g):
                # the tile constants are made on the group's stream (once per grid), before
                # the sum that reads them
                sst, freq, k0 = feed.collect(g)
                tc = self._tile_constants(freq, k0, sst, B)
                return B.flush_loglike(self._d, self._w_templ, out, tile_const=tc, out_off=g0)
        else:
            def step(g0, g):
                gi, m, sst, freq, k0 = feed.flush(g)
                kind.fused_sum(self, B, gi, out[g0:g0 + m], sst, freq, k0)
                return gi
        return self._fused_drive(F, feed, step, n, G, out, kind.width).reshape((n, *kind.tail))

    def _fused_route(self, tm, args, kwargs):
        """What feeds the fused groups: "device" (waveform._DeviceFeed) with device_upstream
        (it needs a GenerateEMRIWaveform, keyword waveform arguments and no explicit mode list,
        and otherwise leaves the walkers to the host route), "host" (waveform._HostFeed) with
        fused_likelihood, or None when neither applies or the template's grid is not symmetric.
        Queues nothing."""
        device = (self.device_upstream and not args
                  and isinstance(getattr(tm, "waveform_generator", None), GenerateEMRIWaveform)
                  and kwargs.get("mode_selection") is None)
        if not (device or self.fused_likelihood) or not self._fused_grid_ok(tm, kwargs):
            return None
        return "device" if device else "host"

    def _fused_preparer(self, tm, G):
        """self._fused: the groups' BatchPreparer (prep, made again when the caustic treatment
        changes or a group outgrows it) and what is cached beside it: the group streams'
        handles (gst; efd_stream_order takes them: one event record and one stream wait each,
        in C), arrays of them per ordering (order), the pinned result (pin) and the device
        trajectories' state (traj)."""
        caustic = _caustic(tm)
        F = self._fused
        if F is None or F.prep.caustic != caustic or F.prep.group < G:
            B = BatchPreparer(max(G, self.FUSED_GROUP), self.FUSED_DEPTH, caustic=caustic,
                              device=self.device)
            F = self._fused = SimpleNamespace(
                prep=B, gst=[B.stream(gi).cuda_stream for gi in range(len(B.groups))],
                order={}, pin=None, traj={})
        return F

    def _order_group_streams(self, F, ngroups):
        """The group streams this batch's flushes take (the preparer's rotation from its next
        group) wait for the work queued so far on the current stream: one stream wait each."""
        B, gst = F.prep, F.gst
        key = (gst.index(B.next_flush()[0].cuda_stream), min(ngroups, len(gst)))
        arr = F.order.get(key)
        if arr is None:
            arr = F.order[key] = (ctypes.c_void_p * key[1])(
                *[gst[(key[0] + k) % len(gst)] for k in range(key[1])])
        _lib.check(B.lib.efd_stream_order(
            self.torch.cuda.current_stream(self.device).cuda_stream, arr, len(arr)),
            "efd_stream_order", B.lib)

    def _fused_drive(self, F, feed, step, n, G, out, per):
        """step(g0, slice) for every group of G walkers (it returns the preparer's group), the
        join of the used group streams into the last one, which copies `out` (per doubles a
        walker) to the pinned buffer, and the wait for it. Returns the host copy; a failed
        walker comes back NaN from the kernel, and only then are the groups' flags read."""
        B, gst, lib = F.prep, F.gst, F.prep.lib
        pin = F.pin
        if pin is None or pin.numel() < per * n:
            pin = F.pin = self.torch.empty(max(per * n, 64), dtype=self.torch.float64,
                                           pin_memory=True)
        used = []
        try:
            run_groups(B, feed, n, G, step, used)
            # the other groups' streams join the last one, which copies out
            last = used[-1]
            for gj in sorted(set(used) - {last}):
                _lib.check(lib.efd_stream_order(gst[gj], (ctypes.c_void_p * 1)(gst[last]), 1),
                           "efd_stream_order", lib)
            _lib.check(lib.efd_download(pin.data_ptr(), out.data_ptr(), 8 * per * n, gst[last]),
                       "efd_download", lib)
        finally:
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
        if np.isnan(host).any():
            B.wait()   # device-side errors of the groups' workspaces (sticky across reuse)
        return host

    def _sum_loglike(self, B, gi, out_g, sst, freq, k0):
        """LOGL's sum behind a flushed group, on its stream (efd_modesum_sum_loglike)."""
        tc = self._tile_constants(freq, k0, sst, B)
        B.sum_loglike(gi, self._d, self._w_templ, out_g, sst.cuda_stream, tile_const=tc)

    def _sum_dh_hh(self, B, gi, out_g, sst, freq, k0):
        """PAIR's (efd_modesum_sum_dh_hh: no tile constants)."""
        B.sum_dh_hh(gi, self._d, self._w_templ, out_g, sst.cuda_stream)

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
        cw = _create_waveform(tm)
        if cw is None or not hasattr(cw, "_grid"):
            return False
        _, sym = cw._grid(kwargs.get("T", 1.0), kwargs.get("dt", 10.0), kwargs.get("f_arr"))
        return bool(sym)

    def _pipeline_for(self, tm):
        """The WaveformPipeline (self.num_streams slots) and per-slot buffers of get_ll."""
        torch = self.torch
        nch, nb = self._d.shape
        caustic = _caustic(tm)
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
        subset_axis = 1 if self.transpose_params else 0
        if subset_axis:
            params = params.T
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


# The output kinds of Likelihood._run. tail, width: a walker's slot in `out` ([n, *tail], width
# doubles); reduce(reducer, h, d, w, out=): one written template to its slot; window: the
# windowed branch's per-group action, at most window_cap rows a group; fused_sum: the sum behind
# a fused group's flush; native_group: whether the host route's one-call group may take it;
# device, host: the result as the caller gets it.
LOGL = SimpleNamespace(
    tail=(), width=1, reduce=Reducer.loglike,
    window=Likelihood._window_loglike, window_cap=_lib.EFD_HANN_ROWS_MAX,
    fused_sum=Likelihood._sum_loglike, native_group=True,
    device=lambda like, out: out, host=lambda host: host)
PAIR = SimpleNamespace(
    tail=(3,), width=3, reduce=Reducer.dh_hh_rows,
    window=Likelihood._window_rows, window_cap=_lib.EFD_DH_MAX_ROWS,
    fused_sum=Likelihood._sum_dh_hh, native_group=False,
    device=lambda like, out: (like.torch.complex(out[:, 0], out[:, 1]), out[:, 2].clone()),
    host=lambda host: (host[:, 0] + 1j * host[:, 1], host[:, 2].copy()))


def _create_waveform(tm):
    """tm.waveform_generator.waveform_generator.create_waveform (the mode sum's object), or None."""
    return getattr(getattr(getattr(tm, "waveform_generator", None), "waveform_generator", None),
                   "create_waveform", None)


def _caustic(tm):
    return getattr(_create_waveform(tm), "caustic", "uniform")


def _window_group(tm, cap):
    """Walkers per group of the windowed branch: EFD_WINDOW_GROUP, else the template model's
    WINDOW_GROUP (8), at most `cap` rows (the group's reduction's limit)."""
    return min(max(1, int(os.environ.get("EFD_WINDOW_GROUP", 0))
                   or int(getattr(tm, "WINDOW_GROUP", 8))), cap)


def _per_channel(x, nch, what):
    """inject_signal's noise_fn / noise_kwargs, one per channel: a list of nch, or a list of
    one or a single value repeated."""
    if not isinstance(x, list):
        return [x] * nch
    if len(x) not in (1, nch):
        raise ValueError(f"Number of {what} does not match number of channels declared by user.")
    return x * nch if len(x) == 1 else x


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
