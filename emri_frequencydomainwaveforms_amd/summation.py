"""FD interpolated mode sum on MI355X: host mirror of FEW's `FDInterpolatedModeSum`.

The reference reaches this through `GenerateEMRIWaveform(..., sum_kwargs=dict(pad_output=True,
output_type="fd", odd_len=True))` (check_mode_by_mode.py:69-83) and reads the grid back from
`.waveform_generator.create_waveform.frequency` (check_mode_by_mode.py:250, emri_pe.py:238).
Everything numerical runs in libemrifd.so (csrc/emrifd*.hip) through the C ABI of
include/emrifd.h; PyTorch only provides device memory and the stream.

Grid (FEW 1.x [FEW-ext], reproduces the published 6311631 positive bins at T = 4 yr,
figures/spectrum_downsampled.png): N = int(T * YRSID_SI / dt) + 1, made odd when odd_len,
frequency = fftshift(fftfreq(N, dt)); or the caller's `f_arr` (emri_pe.py:344-364).
"""

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .constants import MTSUN_SI, YRSID_SI
from .frequencies import get_fundamental_frequencies

CAUSTIC_MODES = {"spa": _lib.EFD_CAUSTIC_SPA, "uniform": _lib.EFD_CAUSTIC_UNIFORM}


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.EFDError("no ROCm GPU visible: the FD mode sum only runs on the HIP device path")
    return torch


def fd_grid(T, dt, odd_len=True):
    """FEW's default two-sided grid for an observation of T years sampled at dt seconds."""
    return np.fft.fftshift(np.fft.fftfreq(td_length(T, dt, odd_len), dt))


def is_symmetric(freq):
    f = np.asarray(freq)
    return bool(np.array_equal(f, -f[::-1]))


_F64, _I32, _C128 = np.dtype(np.float64), np.dtype(np.int32), np.dtype(np.complex128)
# the mode sum's ten host inputs, in the order the native staging and the packed uploads take them
HOST_KEYS = ("t", "phi_phi", "phi_r", "f_phi", "f_r", "amp", "m", "n", "ylm_p", "ylm_m")
_HOST_DTYPES = (_F64,) * 5 + (_C128, _I32, _I32, _C128, _C128)


def _host_arrays(host):
    """(arrays, (N_t, K)) of a host dict: HOST_KEYS' ten arrays, C-contiguous, in that order and
    in their device dtypes (amp [N_t][K], ylm_p, ylm_m complex128; m, n int32; the rest float64).
    Arrays that already are come back as they are, the others as converted copies."""
    arrays = [np.ascontiguousarray(host[k], dtype=dt) for k, dt in zip(HOST_KEYS, _HOST_DTYPES)]
    nt, K = arrays[5].shape
    if any(a.size != nt for a in arrays[:5]):
        raise ValueError("trajectory arrays and amplitudes must share N_t")
    if any(a.size != K for a in arrays[6:]):
        raise ValueError("m, n, ylm_p, ylm_m must have K entries")
    return arrays, (nt, K)


def _packed_offsets(arrays):
    """(offsets, total bytes >= 1) of the arrays packed in order, each 256-B aligned."""
    offs, off = [], 0
    for a in arrays:
        off = (off + 255) // 256 * 256
        offs.append(off)
        off += a.nbytes
    return offs, max(off, 1)


def _pack(hb, arrays, offs):
    """The arrays' bytes into the (pinned) uint8 numpy buffer hb at offs."""
    for a, o in zip(arrays, offs):
        hb[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)


def _packed_views(d, arrays, offs):
    """DeviceInputs' fields of the arrays packed in the device buffer d (complex as float64)."""
    torch = _torch()
    return {k: d[o:o + a.nbytes].view(torch.int32 if a.dtype == _I32 else torch.float64)
            for k, a, o in zip(HOST_KEYS, arrays, offs)}


@dataclass
class DeviceInputs:
    """Hot-path inputs resident in HBM (one waveform)."""
    t: object
    phi_phi: object
    phi_r: object
    f_phi: object
    f_r: object
    amp: object       # float64 view of complex [nt][K]
    m: object
    n: object
    ylm_p: object     # float64 view of complex [K]
    ylm_m: object
    nt: int
    K: int

    @classmethod
    def from_host(cls, t, amps, phi_phi, phi_r, f_phi, f_r, m, n, ylm_p, ylm_m, device=None,
                  stream=None, staging=None):
        """amps: complex [nt][K] (FEW teuk_modes layout).

        One host->device transfer: the arrays are packed (256-B aligned) into a reused pinned
        staging buffer and copied asynchronously on `stream` (default: the current stream) into
        one device buffer, whose typed slices are the fields (the ten separate pageable copies
        this replaces cost ~0.17 ms per waveform). Kernels launched on that stream see the data
        in order; the staging buffer is reused only after its previous copy has completed.
        `staging`: a PinnedStage owned by the caller (one per row or stream) instead of the
        per-device default, so waveforms on different streams do not wait on each other's copies.
        """
        torch = require_gpu()
        dev = device or torch.device("cuda", torch.cuda.current_device())
        arrays, (nt, K) = _host_arrays(dict(t=t, phi_phi=phi_phi, phi_r=phi_r, f_phi=f_phi,
                                            f_r=f_r, amp=amps, m=m, n=n, ylm_p=ylm_p,
                                            ylm_m=ylm_m))
        if nt < 2 or not np.all(np.diff(arrays[0]) > 0):
            raise ValueError("trajectory times must be strictly increasing with N_t >= 2")
        return cls(**_staged_upload(arrays, dev, stream, staging), nt=int(nt), K=int(K))


class PinnedStage:
    """A pinned host buffer that asynchronous host->device copies read, reused from copy to
    copy. The copies (efd_upload, efd_fused_group's) are invisible to torch's host allocator, so
    the reuse-after-DMA rule lives here and nowhere else: `reserve` waits for the last copy out
    of the buffer before the host may overwrite it or drop it for a larger one, and `sent`
    records that copy. buf (uint8 tensor), np (its numpy view), ptr and nbytes are None, None,
    0, 0 until the first reservation of at least a byte."""

    def __init__(self, stream=None):
        self.buf = self.np = self.done = None
        self.ptr = self.nbytes = 0
        if stream is not None:
            # a first record, on the still empty stream, creates the event's handle for callers
            # that re-record it natively (efd_fused_group)
            self.sent(stream)

    def reserve(self, nbytes=0):
        """At least nbytes of pinned buffer the host may write now (its numpy view): waits for
        the last copy recorded by `sent`, and only then replaces a buffer that is too small, by
        one of max(2 * nbytes, 1 MiB)."""
        if self.done is not None:
            self.done.synchronize()
        if self.nbytes < nbytes:
            self.buf = _torch().empty(max(2 * nbytes, 1 << 20), dtype=_torch().uint8,
                                      pin_memory=True)
            self.np = self.buf.numpy()
            self.ptr, self.nbytes = self.buf.data_ptr(), self.buf.numel()
        return self.np

    def sent(self, stream):
        """Record, on the torch stream, the copy out of the buffer just queued there."""
        if self.done is None:
            self.done = _torch().cuda.Event()
        self.done.record(stream)


_STAGING = {}


def _staged_upload(arrays, dev, stream=None, staging=None):
    """Copy _host_arrays' arrays into one device buffer through a pinned stage (see from_host;
    default: one per device); returns the fields' views."""
    torch = _torch()
    offs, total = _packed_offsets(arrays)
    if staging is None:
        staging = _STAGING.setdefault((dev.type, dev.index), PinnedStage())
    _pack(staging.reserve(total), arrays, offs)
    strm = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(strm):
        d = torch.empty(total, dtype=torch.uint8, device=dev)
        d.copy_(staging.buf[:total], non_blocking=True)
    staging.sent(strm)
    return _packed_views(d, arrays, offs)


_WS_BYTES = {}


def _ws_bytes(lib, nt, K, nf):
    """efd_modesum_workspace_bytes(N_t, K, N_f), kept in _WS_BYTES: walkers repeat shapes, and
    the lookup (which the hot callers make themselves first) is cheaper than the ctypes call."""
    nbytes = int(lib.efd_modesum_workspace_bytes(nt, K, nf))
    if nbytes == 0:
        raise _lib.EFDError("efd_modesum_workspace_bytes rejected the shape")
    if len(_WS_BYTES) > 65536:
        _WS_BYTES.clear()
    _WS_BYTES[(nt, K, nf)] = nbytes
    return nbytes


class ModeSumEngine:
    """Owns the workspace and launches efd_modesum on the current torch stream."""

    def __init__(self, caustic="uniform"):
        if caustic not in CAUSTIC_MODES:
            raise ValueError(f"caustic must be one of {sorted(CAUSTIC_MODES)}")
        self.caustic = caustic
        self.lib = _lib.load()
        self._ws = None
        self._ws_cap, self._ws_dev, self._ws_ptr = 0, None, 0
        self._last_args = None

    def _workspace(self, nt, K, nf, device, stream=None):
        """The workspace for (nt, K, nf), grown when too small. With `stream` (a torch stream)
        a new allocation is made on it, so the caching allocator ties the block to the stream
        that uses it (WaveformPipeline slots)."""
        nbytes = _WS_BYTES.get((nt, K, nf)) or _ws_bytes(self.lib, nt, K, nf)
        if self._ws is not None and self._ws_cap >= nbytes and self._ws_dev == device:
            return self._ws   # the walker-batch fast path: no torch calls
        torch = _torch()
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            old = self._ws if self._ws is not None and self._ws.device == device else None
            self._ws = None
            import contextlib
            ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
            with ctx:
                ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
                # the header's device-side error flags are sticky until efd_modesum_status
                # reads them: a grown workspace inherits its predecessor's header (stream
                # order), a first one starts clean (nothing from the memory's previous owner)
                if old is not None:
                    ws[:_lib.HEADER_BYTES].copy_(old[:_lib.HEADER_BYTES])
                else:
                    ws[:_lib.HEADER_BYTES].zero_()
            self._ws = ws
        self._ws_cap, self._ws_dev = self._ws.numel(), self._ws.device
        self._ws_ptr = self._ws.data_ptr()
        return self._ws

    def split_plan(self):
        """(items, split tiles) of the sparse fused likelihood's split plan in this workspace's
        header (k_segments_one; items = -1: no plan, the sum visits each union tile once).
        Synchronises the device; for tests and tools."""
        if self._ws is None:
            return (-1, 0)
        torch = _torch()
        torch.cuda.synchronize(self._ws.device)
        o = _lib.HEADER_SPLIT_PLAN
        v = self._ws[o:o + 8].cpu().numpy().view(np.int32)
        return int(v[0]), int(v[1])

    def launch(self, inp, freq, out, grid_symmetric, scale=1.0 + 0.0j, accumulate=False,
               stream=None, prof_events=(None, None), hp=None, hc=None, k0=0, phase="all"):
        """Asynchronous launch; returns the workspace (check with `status`).

        out: float64 view of the complex spectrum, or None when only the fused polarisations
        hp/hc (float64 views of complex [nf - k0], symmetric grids) are wanted. phase: "all"
        (efd_modesum), "prepare" or "sum" (efd_modesum_prepare / _sum, for overlapping one
        waveform's preparation with the previous one's sum on another stream).
        """
        torch = _torch()
        a, ws = self._args(inp, freq, out, grid_symmetric, scale, accumulate, prof_events, hp,
                           hc, k0)
        st = stream if stream is not None else torch.cuda.current_stream(freq.device).cuda_stream
        fn = {"all": "efd_modesum", "prepare": "efd_modesum_prepare",
              "sum": "efd_modesum_sum"}[phase]
        _lib.check(getattr(self.lib, fn)(a, ws.data_ptr(), ws.numel(), st), fn, self.lib)
        self._last_args = a
        return ws

    def _args(self, inp, freq, out, grid_symmetric, scale=1.0 + 0.0j, accumulate=False,
              prof_events=(None, None), hp=None, hc=None, k0=0):
        """(efd_modesum_args, workspace) of one launch."""
        nf = int(freq.numel())
        ws = self._workspace(inp.nt, inp.K, nf, freq.device)
        ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
        a = _lib.ModesumArgs(
            t=inp.t.data_ptr(), phi_phi=inp.phi_phi.data_ptr(), phi_r=inp.phi_r.data_ptr(),
            f_phi=inp.f_phi.data_ptr(), f_r=inp.f_r.data_ptr(), nt=inp.nt,
            amp=inp.amp.data_ptr(), m=inp.m.data_ptr(), n=inp.n.data_ptr(),
            ylm_p=inp.ylm_p.data_ptr(), ylm_m=inp.ylm_m.data_ptr(), K=inp.K,
            freq=freq.data_ptr(), nf=nf, grid_symmetric=1 if grid_symmetric else 0,
            scale_re=float(np.real(scale)), scale_im=float(np.imag(scale)),
            caustic=CAUSTIC_MODES[self.caustic], accumulate=1 if accumulate else 0,
            out=ptr(out), prof_begin=prof_events[0], prof_end=prof_events[1],
            hp=ptr(hp), hc=ptr(hc), k0=int(k0))
        return a, ws

    def status(self, stream=None):
        """Synchronise; True when the last launch reported no device-side error."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        return self.lib.efd_modesum_status(self._ws.data_ptr(), st) == _lib.EFD_OK

    def _header_counters(self, fn, ctypes_of, stream):
        """The workspace header's counters the C call `fn` reads after synchronising `stream`
        (None: the current one), one per ctypes type in ctypes_of, as Python ints."""
        st = stream if stream is not None else _torch().cuda.current_stream().cuda_stream
        vals = [t(0) for t in ctypes_of]
        _lib.check(getattr(self.lib, fn)(self._ws.data_ptr(), *map(ctypes.byref, vals), st),
                   fn, self.lib)
        return [int(v.value) for v in vals]

    def contributions(self, stream=None):
        return self._header_counters("efd_modesum_contributions", [ctypes.c_int64], stream)[0]

    def stats(self, stream=None):
        """(contributions C, SPA evaluations, (m, n) groups) of the last launch."""
        return tuple(self._header_counters(
            "efd_modesum_stats", [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32], stream))

    def env_evaluations(self, stream=None):
        """SPA evaluations of the last launch made on envelope records (k_items' per-record
        amplitude / K_1/3-phase polynomials)."""
        return self._header_counters("efd_modesum_env_evaluations", [ctypes.c_int64], stream)[0]

    def run(self, inp, freq, out=None, grid_symmetric=None, scale=1.0 + 0.0j, accumulate=False,
            check=True):
        """Launch on the current stream; with check=True synchronise and surface device errors."""
        torch = _torch()
        if grid_symmetric is None:
            grid_symmetric = is_symmetric(freq.detach().cpu().numpy())
        if out is None:
            out = torch.empty(int(freq.numel()), dtype=torch.complex128, device=freq.device)
        self.launch(inp, freq, torch.view_as_real(out), grid_symmetric, scale, accumulate)
        if check:
            if not self.status():
                raise _lib.EFDError(f"efd_modesum: {_lib.last_error(self.lib)}")
        return out


def _job_args(eng, kw, outputs=None, prof=None):
    """(argument struct, workspace) of one (engine, launch_kwargs) job of a batched sum. A
    BatchPreparer job carries its prepare call's struct (kw["_args"]): the fused sums, which
    write no template, take it as it is (outputs None); sum_batch passes the call's outputs (a
    dict with out / hp / hc / accumulate, the job's own kwargs) and gets a copy with those and
    the prof events set. A job without the struct, or sum_batch's with its `inp` (a
    WaveformPipeline slot's), is built from its kwargs by the engine."""
    a0 = kw.get("_args")
    if a0 is None or (outputs is not None and "inp" in kw):
        return eng._args(prof_events=prof or (None, None),
                         **{k: v for k, v in kw.items() if k != "_args"})
    if outputs is None:
        return a0, eng._ws
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    a = _lib.ModesumArgs.from_buffer_copy(a0)
    a.out, a.hp, a.hc = ptr(outputs.get("out")), ptr(outputs.get("hp")), ptr(outputs.get("hc"))
    a.accumulate = 1 if outputs.get("accumulate") else 0
    a.prof_begin, a.prof_end = prof or (None, None)
    return a, eng._ws


def _marshal(what, jobs, one, stream):
    """The batch calls' shared marshalling: (lib, args**, workspaces*, bytes*, count, stream
    handle, workspaces) of 1..EFD_BATCH_MAX (engine, launch_kwargs) jobs, each job's
    (argument struct, workspace) made by one(i, engine, kwargs); stream None: the current one
    on the grid's device."""
    jobs = list(jobs)
    n = len(jobs)
    if not 1 <= n <= _lib.EFD_BATCH_MAX:
        raise ValueError(f"{what} takes 1..{_lib.EFD_BATCH_MAX} waveforms")
    pairs = [one(i, eng, kw) for i, (eng, kw) in enumerate(jobs)]
    wss = [ws for _, ws in pairs]
    pa = (ctypes.POINTER(_lib.ModesumArgs) * n)(*[ctypes.pointer(a) for a, _ in pairs])
    pw = (ctypes.c_void_p * n)(*[ws.data_ptr() for ws in wss])
    pb = (ctypes.c_size_t * n)(*[ws.numel() for ws in wss])
    if stream is None:
        stream = _torch().cuda.current_stream(jobs[0][1]["freq"].device).cuda_stream
    return jobs[0][0].lib, pa, pw, pb, n, stream, wss


def sum_batch(jobs, stream=None, prof_events=(None, None)):
    """The mode sums of several prepared waveforms in one launch (efd_modesum_sum_batch).

    jobs: sequence of (engine, launch_kwargs) pairs; each engine was prepared with
    `launch(..., phase="prepare")` and launch_kwargs are the keyword arguments its
    `launch(..., phase="sum")` would take (inp, freq, out, grid_symmetric, and optionally scale,
    accumulate, hp, hc, k0). Every waveform's outputs are bitwise those of its own sum; the
    waveforms' tiles share one longest-first dispatch (one ramp, one tail, no launch gaps).
    prof_events bracket the launch. At most EFD_BATCH_MAX waveforms.
    """
    lib, pa, pw, pb, n, st, wss = _marshal(
        "sum_batch", jobs,
        lambda i, eng, kw: _job_args(eng, kw, kw, prof_events if i == 0 else None), stream)
    _lib.check(lib.efd_modesum_sum_batch(pa, pw, pb, n, st), "efd_modesum_sum_batch", lib)
    return wss


def prepare_batch(jobs, stream=None):
    """The preparations of several waveforms in one chain of launches
    (efd_modesum_prepare_batch). jobs: (engine, launch_kwargs) pairs as sum_batch takes them;
    each workspace ends bitwise as after the engine's own launch(..., phase="prepare"), so the
    jobs go on to sum_batch / sum_batch_loglike / launch(phase="sum") unchanged."""
    def one(i, eng, kw):
        a, ws = eng._args(**{k: v for k, v in kw.items() if k != "_args"})
        eng._last_args = a
        return a, ws

    lib, pa, pw, pb, n, st, wss = _marshal("prepare_batch", jobs, one, stream)
    _lib.check(lib.efd_modesum_prepare_batch(pa, pw, pb, n, st), "efd_modesum_prepare_batch",
               lib)
    return wss


def _check_ll_io(torch, d, w, out, nb, n):
    if (d.dtype != torch.complex128 or tuple(d.shape) != (2, nb) or not d.is_contiguous()
            or w.dtype != torch.float64 or tuple(w.shape) != (2, nb) or not w.is_contiguous()
            or out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous()):
        raise ValueError(f"sum_batch_loglike: d complex128 [2][{nb}], w float64 [2][{nb}] and "
                         f"out float64 [>= {n}], contiguous")


def loglike_tile_constants(d, w, nf, k0, stream=None, lib=None):
    """efd_loglike_tile_constants: the fused likelihood's partial of every tile on which a
    template is zero (float64 [efd_loglike_tile_count(nf)] on d's device). They depend on d, w
    and the grid only; sum_batch_loglike / BatchPreparer.sum_loglike take them as tile_const and
    then skip the d, w reads of the tiles no harmonic reaches, bitwise the same logL."""
    torch = _torch()
    lib = lib or _lib.load()
    nb = int(nf) - int(k0)
    _check_ll_io(torch, d, w, torch.empty(1, dtype=torch.float64), nb, 1)
    nt = int(lib.efd_loglike_tile_count(int(nf)))
    tc = torch.empty(nt, dtype=torch.float64, device=d.device)
    st = stream if stream is not None else torch.cuda.current_stream(d.device).cuda_stream
    _lib.check(lib.efd_loglike_tile_constants(torch.view_as_real(d).data_ptr(), w.data_ptr(),
                                              int(nf), int(k0), tc.data_ptr(), st),
               "efd_loglike_tile_constants", lib)
    return tc


def _tile_const_ptr(tile_const, nf, lib):
    if tile_const is None:
        return None
    if (tile_const.dtype != _torch().float64 or not tile_const.is_contiguous()
            or tile_const.numel() != int(lib.efd_loglike_tile_count(int(nf)))):
        raise ValueError("tile_const: loglike_tile_constants' output for this grid")
    return tile_const.data_ptr()


def sum_batch_loglike(jobs, d, w, out, stream=None, tile_const=None):
    """Mode sums of several prepared waveforms with the likelihood fused into the sum
    (efd_modesum_sum_loglike): out[i] = -1/2 * 4 * sum |d - h_i w|^2 over both channels, h_i
    the waveform's [h+, hx] over the f >= 0 bins, never written to HBM.

    jobs: as sum_batch, every one on a symmetric grid with the same k0 (the likelihood's
    f >= 0 start) and accumulate off. d: complex128 [2][nf - k0], w: float64 [2][nf - k0]
    (contiguous, on the device), out: float64 [len(jobs)] on the device (written in stream
    order, no host synchronisation). tile_const: loglike_tile_constants(d, w, nf, k0), or None.
    """
    torch = _torch()
    jobs = list(jobs)
    if jobs:   # (none: the marshaller's count check raises)
        kw0 = jobs[0][1]
        _check_ll_io(torch, d, w, out, int(kw0["freq"].numel()) - int(kw0.get("k0", 0)),
                     len(jobs))

    lib, pa, pw, pb, n, st, wss = _marshal("sum_batch_loglike", jobs,
                                           lambda i, eng, kw: _job_args(eng, kw), stream)
    tc = _tile_const_ptr(tile_const, jobs[0][1]["freq"].numel(), lib)
    _lib.check(lib.efd_modesum_sum_loglike_ex(pa, pw, pb, n, torch.view_as_real(d).data_ptr(),
                                              w.data_ptr(), tc, out.data_ptr(), st),
               "efd_modesum_sum_loglike_ex", lib)
    return wss


def _check_dh_out(torch, out, n):
    if out.dtype != torch.float64 or out.numel() < 3 * n or not out.is_contiguous():
        raise ValueError(f"sum_batch_dh_hh: out float64 [{n}][3], contiguous")


def sum_batch_dh_hh(jobs, d, w, out, stream=None, dense=False, part=None):
    """<d|h> and <h|h> of several prepared waveforms from the mode sum's epilogue
    (efd_modesum_sum_dh_hh): out[i] = (Re <d|h_i>, Im <d|h_i>, <h_i|h_i>), 4 sum conj(d) h w and
    4 sum |h w|^2 over both channels, h_i never written to HBM.

    jobs, d, w: as sum_batch_loglike; out: float64 [len(jobs)][3] on the device. dense: visit
    every tile (the sparse launch's A/B switch; bitwise the same numbers). part: float64
    [>= 3 len(jobs) efd_loglike_tile_count(nf)] for the tiles' partials (its contents do not
    matter), or None to allocate it. At most EFD_BATCH_MAX waveforms."""
    torch = _torch()
    jobs = list(jobs)
    if jobs:   # (none: the marshaller's count check raises)
        kw0 = jobs[0][1]
        _check_ll_io(torch, d, w, torch.empty(1, dtype=torch.float64),
                     int(kw0["freq"].numel()) - int(kw0.get("k0", 0)), 1)
        _check_dh_out(torch, out, len(jobs))

    lib, pa, pw, pb, n, st, wss = _marshal("sum_batch_dh_hh", jobs,
                                           lambda i, eng, kw: _job_args(eng, kw), stream)
    need = 3 * n * int(lib.efd_loglike_tile_count(int(jobs[0][1]["freq"].numel())))
    if part is None:
        part = torch.empty(need, dtype=torch.float64, device=d.device)
    elif part.dtype != torch.float64 or part.numel() < need or not part.is_contiguous():
        raise ValueError(f"sum_batch_dh_hh: part float64 [>= {need}], contiguous")
    _lib.check(lib.efd_modesum_sum_dh_hh(pa, pw, pb, n, torch.view_as_real(d).data_ptr(),
                                         w.data_ptr(), part.data_ptr(), 1 if dense else 0,
                                         out.data_ptr(), st),
               "efd_modesum_sum_dh_hh", lib)
    return wss


class _Slot:
    """One WaveformPipeline slot: its engine (workspace), stream and pinned stage; the device
    buffer the inputs are copied to with the (key, offsets, total) layout and the DeviceInputs
    views made for it; the sum job a prepare_only submit left; whether it was used; and S, the
    spectrum buffer submit_channels keeps here for grids that are not symmetric."""

    def __init__(self, caustic, device):
        self.engine = ModeSumEngine(caustic=caustic)
        self.stream = _torch().cuda.Stream(device)
        self.stage = PinnedStage()
        self.dbuf = self.layout = self.inp = self.job = self.S = None
        self.used = False


class WaveformPipeline:
    """Several FD waveforms in flight on one device.

    One waveform's device chain is mostly latency-bound preparation (grouping, spline
    recurrences, interval records, tile lists: a few workgroups each) and, for the small
    harmonic counts of parameter scans and MCMC walkers (eps = 1e-2: tens of harmonics), a short
    mode sum. Run one at a time they leave most of the GPU idle. The pipeline owns `num_slots`
    slots -- a ModeSumEngine workspace, a HIP stream and a pinned staging buffer each -- and
    `submit` puts waveform i's whole chain (input upload, efd_modesum, h+/hx) on slot
    i % num_slots's stream, so independent waveforms overlap. Nothing synchronises the host
    until `wait()` (which also surfaces device-side errors of every slot). A slot's workspace,
    device inputs and staging buffer are reused only in stream order (or after that slot's
    previous upload finished), so results match the one-at-a-time path bitwise.
    """

    def __init__(self, num_slots=4, caustic="uniform", device=None):
        torch = require_gpu()
        if num_slots < 1:
            raise ValueError("num_slots must be >= 1")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.slots = [_Slot(caustic, self.device) for _ in range(num_slots)]
        self._next = 0
        self.caustic = caustic

    @property
    def num_slots(self):
        return len(self.slots)

    def next_slot(self):
        """Index of the slot the next `submit` uses."""
        return self._next

    def stream(self, slot):
        return self.slots[slot].stream

    def submit(self, host, freq, grid_symmetric, scale=1.0 + 0.0j, out=None, hp=None, hc=None,
               k0=0, accumulate=False, order=True, prepare_only=False):
        """Queue one waveform; returns its slot index.

        host: dict of host arrays t, amp (complex [nt][K]), phi_phi, phi_r, f_phi, f_r, m, n,
        ylm_p, ylm_m. Outputs as ModeSumEngine.launch: out (float64 view of the complex
        spectrum) and/or hp, hc (float64 views of complex [nf - k0], symmetric grids: the
        polarisations written by the mode sum itself). Follow-up work on the outputs belongs on
        `stream(slot)` (or after `wait()`). order=False skips making the slot wait for the
        current stream (the caller did it once for the batch: `order_after_current`).
        prepare_only: upload and efd_modesum_prepare only; the slot keeps the sum's job
        (`job(slot)`, for sum_batch / sum_batch_loglike on another stream after the slot's).
        """
        torch = _torch()
        i = self._next
        self._next = (i + 1) % len(self.slots)
        sl = self.slots[i]
        st = sl.stream
        if order:
            # the caller produced freq / outputs on its own stream: order this slot after it
            st.wait_stream(torch.cuda.current_stream(self.device))
        inp = self._upload(sl, host)
        eng = sl.engine
        eng._workspace(inp.nt, inp.K, int(freq.numel()), freq.device, stream=st)
        eng.launch(inp, freq, out, grid_symmetric, scale, accumulate, stream=st.cuda_stream,
                   hp=hp, hc=hc, k0=k0, phase="prepare" if prepare_only else "all")
        # the prepare call's argument struct is the sum's too (same fields, no events)
        sl.job = (eng, dict(inp=inp, freq=freq, out=out, grid_symmetric=grid_symmetric,
                            scale=scale, accumulate=accumulate, hp=hp, hc=hc, k0=k0,
                            _args=eng._last_args)) if prepare_only else None
        sl.used = True
        return i

    def job(self, slot):
        """The sum job a prepare_only submit left on `slot` (engine, launch kwargs)."""
        return self.slots[slot].job

    def order_after_current(self):
        """Make every slot wait for the work queued so far on the current stream (once per
        batch, instead of `order=True` on each submit)."""
        torch = _torch()
        cur = torch.cuda.current_stream(self.device)
        for sl in self.slots:
            sl.stream.wait_stream(cur)

    def _upload(self, sl, host):
        """The waveform's inputs into the slot's device buffer: packed into the slot's pinned
        buffer, one asynchronous copy on the slot's stream (efd_upload). Buffers grow as needed
        and are reused in stream order; the field views are rebuilt only when (nt, K) change."""
        torch = _torch()
        arrays, key = _host_arrays(host)
        lay = sl.layout
        if lay is None or lay[0] != key:
            lay = (key,) + _packed_offsets(arrays)
        _, offs, total = lay
        _pack(sl.stage.reserve(total), arrays, offs)
        if sl.dbuf is None or sl.dbuf.numel() < total:
            with torch.cuda.stream(sl.stream):
                sl.dbuf = torch.empty(max(2 * total, 1 << 20), dtype=torch.uint8,
                                      device=self.device)
            sl.layout = None
        lib = sl.engine.lib
        _lib.check(lib.efd_upload(sl.dbuf.data_ptr(), sl.stage.ptr, total,
                                  sl.stream.cuda_stream), "efd_upload", lib)
        sl.stage.sent(sl.stream)
        if sl.layout is None or sl.layout[0] != key or sl.inp is None:
            sl.inp = DeviceInputs(**_packed_views(sl.dbuf, arrays, offs),
                                  nt=int(key[0]), K=int(key[1]))
            sl.layout = lay
        return sl.inp

    def join(self):
        """Make the current stream wait for every slot (device-side; no host sync)."""
        torch = _torch()
        cur = torch.cuda.current_stream(self.device)
        for sl in self.slots:
            if sl.used:
                cur.wait_stream(sl.stream)

    def wait(self):
        """Synchronise every slot and raise if any reported a device-side error."""
        for sl in self.slots:
            if sl.used and not sl.engine.status(sl.stream.cuda_stream):
                raise _lib.EFDError(f"efd_modesum: {_lib.last_error(sl.engine.lib)}")
        self.join()


class _Group:
    """One of a BatchPreparer's rotating walker groups: `size` engines (a workspace each), the
    stream its work runs on, its staging buffers and the argument arrays the native calls take."""

    def __init__(self, size, caustic, device):
        torch = _torch()
        self.engines = [ModeSumEngine(caustic=caustic) for _ in range(size)]
        self.stream = torch.cuda.Stream(device)
        # the pinned stage (its event exists from the start: efd_fused_group re-records it) and
        # the device buffer it is copied to (BatchPreparer._stage grows both)
        self.stage = PinnedStage(self.stream)
        self.dbuf = None
        self.busy = None      # release()'s event: the group's last sum has read its workspaces
        # the device upstream's selection state (device_inputs_batch's `state`: its pinned and
        # output buffers; the group's previous sum reads them on this stream)
        self.select = {}
        self.used = False
        self.n = 0            # walkers of the group's last flush
        # the walkers' argument structs, with the args** table, the workspace pointer and size
        # arrays of the batch calls, and the three arrays' addresses for efd_fused_group
        args_t, args_pp = _lib.ModesumArgs, ctypes.POINTER(ctypes.POINTER(_lib.ModesumArgs))
        self.args = (args_t * size)()
        self.args_ptr = ctypes.addressof(self.args)
        self.pa = ctypes.cast((ctypes.c_void_p * size)(
            *[self.args_ptr + i * ctypes.sizeof(args_t) for i in range(size)]), args_pp)
        self.pw = (ctypes.c_void_p * size)()
        self.pb = (ctypes.c_size_t * size)()
        self.pw_ptr, self.pb_ptr = ctypes.addressof(self.pw), ctypes.addressof(self.pb)
        self.arg_views = [self.args[i] for i in range(size)]   # stable per-walker views
        self.tmpl = None      # (key, template struct) of the last flush (BatchPreparer._take)
        self.ws_floor = None  # (device, smallest workspace, walkers) flush_loglike sized last
        self.dh_part = None   # sum_dh_hh's tile partials (grown on the group's stream)
        # (first, count, args**, workspaces*, bytes*) per launch of at most EFD_BATCH_MAX of
        # the group's first n walkers, for every n: pointers into the arrays above
        self.chunks = [None]
        pa0 = ctypes.cast(self.pa, ctypes.c_void_p).value
        step = _lib.EFD_BATCH_MAX
        for n in range(1, size + 1):
            self.chunks.append([
                (c0, min(step, n - c0), ctypes.cast(pa0 + 8 * c0, args_pp),
                 ctypes.cast(self.pw_ptr + 8 * c0, ctypes.POINTER(ctypes.c_void_p)),
                 ctypes.cast(self.pb_ptr + 8 * c0, ctypes.POINTER(ctypes.c_size_t)))
                for c0 in range(0, n, step)])


class BatchPreparer:
    """Walker batches prepared in one chain of launches (efd_modesum_prepare_batch).

    It stands in for a WaveformPipeline in the template chain's `submit(..., prepare_only=True)`
    (fdutils / waveform / FDInterpolatedModeSum.submit_channels): `submit` only collects the
    walker's host inputs. `flush()` then packs the collected walkers into one pinned buffer, makes
    one host->device copy and one efd_modesum_prepare_batch call on the next group's stream, and
    returns (group, jobs) for sum_batch_loglike / sum_batch. `depth` groups, each with `group`
    workspaces, rotate: a group is reused after the event its sum recorded (`release`), so
    group i+1's preparation runs beside group i's sum. Per walker the host pays the packing
    copies and one argument struct instead of ~10 launches (efd_modesum_prepare).
    `flush_device()` feeds the next group from inputs the device upstream left on the device
    instead; everything behind the feed is the same.
    """

    # walkers per flush: up to GROUP_MAX, staged and uploaded together; the preparation and sum
    # launches take them EFD_BATCH_MAX at a time (the kernels' argument limit)
    GROUP_MAX = 4 * _lib.EFD_BATCH_MAX

    def __init__(self, group=8, depth=2, caustic="uniform", device=None):
        torch = require_gpu()
        if not 1 <= group <= self.GROUP_MAX or depth < 1:
            raise ValueError(f"group must be in 1..{self.GROUP_MAX}, depth >= 1")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.caustic = caustic
        self.group = group
        self.groups = [_Group(group, caustic, self.device) for _ in range(depth)]
        self.lib = self.groups[0].engines[0].lib
        self._next = 0
        self._pending = []
        self._jobs = []          # the last flush()'s (engine, job) pairs (last_jobs)
        self._last = None        # (gi, n, freq, k0, sym) of the last flush_loglike (last_jobs)
        self._ll_checked = None  # the (d, w, bins) flush_loglike checked last

    # -- the WaveformPipeline surface the template chain uses ---------------------------------
    def next_slot(self):
        return len(self._pending)

    def submit(self, host, freq, grid_symmetric, scale=1.0 + 0.0j, out=None, hp=None, hc=None,
               k0=0, accumulate=False, order=True, prepare_only=False):
        if not prepare_only or out is not None or hp is not None or hc is not None:
            raise ValueError("BatchPreparer collects prepare_only submissions")
        if len(self._pending) >= self.group:
            raise ValueError(f"at most {self.group} walkers per flush")
        self._pending.append((host, freq, bool(grid_symmetric), complex(scale), int(k0),
                              bool(accumulate)))
        return len(self._pending) - 1

    def collect(self, host, freq, scale, k0):
        """submit(host, freq, True, scale, k0=k0, prepare_only=True) for callers that hold
        normalised arguments already (a complex scale, an int k0): a symmetric grid, accumulate
        off, no argument handling. A walker batch's loop binds it once."""
        if len(self._pending) >= self.group:
            raise ValueError(f"at most {self.group} walkers per flush")
        self._pending.append((host, freq, True, scale, k0, False))

    def order_after_current(self):
        torch = _torch()
        cur = torch.cuda.current_stream(self.device)
        for g in self.groups:
            g.stream.wait_stream(cur)

    def stream(self, gi):
        return self.groups[gi].stream

    def drop_pending(self):
        """Forget the walkers submitted since the last flush (a caller's error path)."""
        self._pending = []

    def next_flush(self):
        """(stream, freq, k0) of the next flush() / flush_loglike(): the stream of the group it
        rotates to and the pending walkers' grid (None, None while nothing is pending)."""
        p = self._pending
        freq, k0 = (p[0][1], p[0][4]) if p else (None, None)
        return self.groups[self._next].stream, freq, k0

    def restart(self):
        """The next flush takes the first group again. The device upstream starts every batch
        there, so a batch of one group keeps to one set of workspaces (reuse is ordered by the
        group's stream and `busy`, as for any rotation)."""
        self._next = 0

    def next_select(self):
        """The selection state of the group the next flush rotates to: device_inputs_batch's
        `state` for the walkers of the next flush_device(), run on next_flush()'s stream."""
        return self.groups[self._next].select

    def workspace_ptrs(self, gi):
        """Group gi's workspace pointer array (void*[group]; its last flush's walkers first)."""
        return self.groups[gi].pw

    # -- one batch -----------------------------------------------------------------------------
    def _rotate(self):
        """(group index, group) of the next flush: the groups rotate, and the group's stream
        waits for the sum that last read its workspaces."""
        gi = self._next
        self._next = (gi + 1) % len(self.groups)
        G = self.groups[gi]
        if G.busy is not None:
            G.stream.wait_event(G.busy)
        return gi, G

    def _take(self, what):
        """The pending walkers for the next group: (group index, group, walkers, template
        struct). The walkers are checked first (one grid; symmetry, k0 and accumulate agree);
        then the groups rotate and the group's stream waits for the sum that last read its
        workspaces, the host for the last copy out of its pinned stage (reserve)."""
        pend, self._pending = self._pending, []
        if not pend:
            raise ValueError(f"{what}: nothing submitted")
        _, freq, sym, _, k0, acc = pend[0]
        nf = int(freq.numel())
        for _, f, s, _, k, a in pend:
            if f is not freq and (int(f.numel()) != nf or f.data_ptr() != freq.data_ptr()):
                raise ValueError("flush: the walkers of a group share one frequency grid")
            if s != sym or k != k0 or a != acc:
                raise ValueError("flush: grid symmetry, k0 and accumulate must agree in a group")
        gi, G = self._rotate()
        G.stage.reserve()
        key = (freq.data_ptr(), nf, sym, acc, k0)
        if G.tmpl is None or G.tmpl[0] != key:
            G.tmpl = (key, _lib.ModesumArgs(
                freq=freq.data_ptr(), nf=nf, grid_symmetric=1 if sym else 0,
                caustic=CAUSTIC_MODES[self.caustic], accumulate=1 if acc else 0, k0=k0))
        return gi, G, pend, G.tmpl[1]

    @staticmethod
    def _sources(pend):
        """(src, shape, scale, keep) of efd_stage_batch for the pending walkers: the native
        upstream's packed addresses and shapes (host["_src"], host["_shape"]: bytes) joined in
        one call when every walker has them, or row by row with the other walkers' arrays
        converted (_host_arrays; kept alive in keep until the staging copy)."""
        n = len(pend)
        keep = []
        fast = [p[0].get("_src") for p in pend]
        scale = np.array([p[3] for p in pend], dtype=np.complex128).view(np.float64)
        if None not in fast:
            src = np.frombuffer(b"".join(fast), dtype=np.uint64)
            shape = np.frombuffer(b"".join([p[0]["_shape"] for p in pend]),
                                  dtype=np.int32).reshape(n, 2)
            return src, shape, scale, keep
        src = np.empty((n, 10), dtype=np.uint64)
        shape = np.empty((n, 2), dtype=np.int32)
        for i, p in enumerate(pend):
            if fast[i] is not None:
                src[i] = np.frombuffer(fast[i], dtype=np.uint64)
                shape[i] = np.frombuffer(p[0]["_shape"], dtype=np.int32)
            else:
                arrays, shape[i] = _host_arrays(p[0])
                keep.append(arrays)
                src[i] = [a.ctypes.data for a in arrays]
        return src, shape, scale, keep

    def _stage(self, G, call, failed):
        """The staging call call(pin, pin bytes, dbuf, dbuf bytes, &total) on G's buffers
        (efd_stage_batch, or efd_fused_group, which goes on to the launches); a buffer too
        small for `total` is grown (the pinned stage's reserve; the device one to
        max(2 * total, 1 MiB) on G's stream) and the call made once more. _take has waited for
        the last copy out of the stage. Returns total; failed(rc) is the error's text."""
        torch = _torch()
        total = ctypes.c_size_t(0)
        pin = G.stage
        for attempt in range(2):
            dbuf = G.dbuf
            rc = call(pin.ptr, pin.nbytes, dbuf.data_ptr() if dbuf is not None else 0,
                      dbuf.numel() if dbuf is not None else 0, ctypes.byref(total))
            need = total.value
            if rc == _lib.EFD_OK and dbuf is not None and dbuf.numel() >= need:
                return need
            if rc not in (_lib.EFD_OK, _lib.EFD_ERR_WORKSPACE) or attempt == 1:
                raise _lib.EFDError(failed(rc))
            pin.reserve(need)
            if dbuf is None or dbuf.numel() < need:
                with torch.cuda.stream(G.stream):
                    G.dbuf = torch.empty(max(2 * need, 1 << 20), dtype=torch.uint8,
                                         device=self.device)

    def _size_each(self, G, shape, freq, k0, sym):
        """flush()'s workspaces: every engine sized for its own walker's (N_t, K) (the
        generator's batches vary widely in K). Fills the group's pointer and size arrays and
        returns the walkers' jobs."""
        nf, dev, st = int(freq.numel()), freq.device, G.stream
        pw, pb, views, engines = G.pw, G.pb, G.arg_views, G.engines
        jobs = []
        for i, (nt_i, K_i) in enumerate(shape.tolist()):
            eng = engines[i]
            nbytes = _WS_BYTES.get((nt_i, K_i, nf))
            if nbytes is None or eng._ws is None or eng._ws_cap < nbytes or eng._ws_dev != dev:
                eng._workspace(nt_i, K_i, nf, dev, stream=st)   # sized, or grown, here
            pw[i] = eng._ws_ptr
            pb[i] = eng._ws_cap
            a_i = views[i]
            eng._last_args = a_i
            jobs.append((eng, {"freq": freq, "k0": k0, "grid_symmetric": sym, "_args": a_i}))
        return jobs

    def _size_group(self, G, shape, freq):
        """flush_loglike()'s workspaces: sized for the group's largest (N_t, K) (the layout
        grows with both), so once every engine holds that much the pointer and size arrays
        stand as they are and no per-walker step is needed."""
        nf, dev, n = int(freq.numel()), freq.device, len(shape)
        kb = (int(shape[:, 0].max()), int(shape[:, 1].max()), nf)
        nbmax = _WS_BYTES.get(kb) or _ws_bytes(self.lib, *kb)
        floor = G.ws_floor
        if floor is None or floor[0] != dev or floor[1] < nbmax or floor[2] < n:
            engines = G.engines
            for i in range(n):
                eng = engines[i]
                if eng._ws is None or eng._ws_cap < nbmax or eng._ws_dev != dev:
                    eng._workspace(kb[0], kb[1], nf, dev, stream=G.stream)   # sized, or grown
                G.pw[i] = eng._ws_ptr
                G.pb[i] = eng._ws_cap
                eng._last_args = G.arg_views[i]
            G.ws_floor = (dev, min(engines[i]._ws_cap for i in range(n)), n)

    def flush(self):
        """Upload and prepare the collected walkers; returns (group index, jobs). A job's
        argument struct lives in the group's reused array: use the jobs before the group's next
        flush (sum_batch / sum_batch_loglike copy what they need)."""
        gi, G, pend, tmpl = self._take("flush")
        _, freq, sym, _, k0, _ = pend[0]
        n, lib, st = len(pend), self.lib, G.stream
        src, shape, scale, keep = self._sources(pend)
        total = self._stage(
            G, lambda pin, pin_bytes, dbuf, dbuf_bytes, total: lib.efd_stage_batch(
                pin, pin_bytes, dbuf, n, src.ctypes.data, shape.ctypes.data, scale.ctypes.data,
                ctypes.byref(tmpl), G.args, total),
            lambda rc: f"efd_stage_batch failed ({rc})")
        del keep
        _lib.check(lib.efd_upload(G.dbuf.data_ptr(), G.stage.ptr, total, st.cuda_stream),
                   "efd_upload", lib)
        G.stage.sent(st)
        return gi, self._prepare(G, self._size_each(G, shape, freq, k0, sym))

    def flush_device(self, inputs, freq, scales, k0):
        """flush() for 1..group walkers whose inputs are on the device already: `inputs` are
        DeviceInputs made on next_flush()'s stream with next_select()'s state
        (device_inputs_batch), `scales` their complex scales; a symmetric grid, accumulate off.
        Nothing is staged or uploaded: the groups rotate as for flush(), every engine is sized
        for its own walker (a grown workspace on the group's stream) and the walkers' argument
        structs go into the group's array, so the jobs, sum_loglike, workspace_ptrs, last_jobs
        and wait() are flush()'s. Returns (group index, jobs)."""
        n = len(inputs)
        if not 1 <= n <= self.group or len(scales) != n or self._pending:
            raise ValueError(f"flush_device takes 1..{self.group} walkers, a scale each, and "
                             "none pending for flush()")
        gi, G = self._rotate()
        jobs = self._size_each(G, np.array([(inp.nt, inp.K) for inp in inputs]), freq, k0, True)
        for i, (inp, sc) in enumerate(zip(inputs, scales)):
            G.args[i] = G.engines[i]._args(inp, freq, None, True, sc, k0=k0)[0]
        return gi, self._prepare(G, jobs)

    def _prepare(self, G, jobs):
        """efd_modesum_prepare_batch over the group's first len(jobs) walkers on its stream;
        the jobs become the preparer's last."""
        n, lib, st = len(jobs), self.lib, G.stream.cuda_stream
        for c0, cnt, pa_c, pw_c, pb_c in G.chunks[n]:
            _lib.check(lib.efd_modesum_prepare_batch(pa_c, pw_c, pb_c, cnt, st),
                       "efd_modesum_prepare_batch", lib)
        G.used = True
        G.n = n
        self._jobs, self._last = jobs, None
        return jobs

    def flush_loglike(self, d, w, out, tile_const=None, out_off=0):
        """flush() and sum_loglike() of the collected walkers in one native call
        (efd_fused_group: staging, upload, the staged event, the preparation and the fused sum
        on the next group's stream); returns the group index. The fused likelihood's per-group
        host path (Likelihood._run_fused): the same launches on the same stream as flush()
        then sum_loglike(gi, ..., G's stream), bitwise the same logL, in one ctypes
        transition instead of five. d, w: checked once per pair of buffers. The logL go to
        out[out_off : out_off + n]."""
        torch = _torch()
        gi, G, pend, tmpl = self._take("flush_loglike")
        _, freq, sym, _, k0, _ = pend[0]
        n, lib, nf = len(pend), self.lib, int(freq.numel())
        dp, wp = d.data_ptr(), w.data_ptr()
        key = (dp, wp, nf - k0)
        if self._ll_checked != key:
            _check_ll_io(torch, d, w, out, nf - k0, n)
            self._ll_checked = key
        if out.dtype != torch.float64 or out.numel() < out_off + n or not out.is_contiguous():
            raise ValueError(f"flush_loglike: out float64 [>= {out_off + n}], contiguous")
        src, shape, scale, keep = self._sources(pend)
        self._size_group(G, shape, freq)
        tcp = tile_const.data_ptr() if tile_const is not None else None
        op = out.data_ptr() + 8 * out_off
        ev, sth = G.stage.done.cuda_event, G.stream.cuda_stream
        self._stage(
            G, lambda pin, pin_bytes, dbuf, dbuf_bytes, total: lib.efd_fused_group(
                pin, pin_bytes, dbuf, dbuf_bytes, n, src.ctypes.data, shape.ctypes.data,
                scale.ctypes.data, ctypes.byref(tmpl), G.args_ptr, G.pw_ptr, G.pb_ptr, dp, wp,
                tcp, op, ev, sth, total),
            lambda rc: f"efd_fused_group: {_lib.last_error(lib)} ({rc})")
        del keep
        G.used = True
        G.n = n
        self._last = (gi, n, freq, k0, sym)
        return gi

    @property
    def last_jobs(self):
        """(engine, job) of the last flush()'s or flush_loglike()'s walkers (made on demand)."""
        if self._last is None:
            return self._jobs
        gi, n, freq, k0, sym = self._last
        G = self.groups[gi]
        return [(G.engines[i], {"freq": freq, "k0": k0, "grid_symmetric": sym,
                                "_args": G.arg_views[i]}) for i in range(n)]

    def sum_loglike(self, gi, d, w, out, stream, tile_const=None):
        """efd_modesum_sum_loglike(_ex) over group gi's last flush (its argument and workspace
        arrays as they are, no per-walker rebuilding); d, w, out, tile_const as
        sum_batch_loglike."""
        torch = _torch()
        G = self.groups[gi]
        n = G.n
        nb = int(G.args[0].nf) - int(G.args[0].k0)
        _check_ll_io(torch, d, w, out, nb, n)
        dp, wp, op = torch.view_as_real(d).data_ptr(), w.data_ptr(), out.data_ptr()
        # (checked by the caller that made them for this grid: no per-call recount)
        tcp = tile_const.data_ptr() if tile_const is not None else None
        for c0, cnt, pa_c, pw_c, pb_c in G.chunks[n]:
            _lib.check(self.lib.efd_modesum_sum_loglike_ex(
                pa_c, pw_c, pb_c, cnt, dp, wp, tcp, op + 8 * c0, stream),
                "efd_modesum_sum_loglike_ex", self.lib)

    def sum_dh_hh(self, gi, d, w, out, stream, dense=False):
        """efd_modesum_sum_dh_hh over group gi's last flush, in launches of EFD_BATCH_MAX
        walkers like sum_loglike: out float64 [n][3] = (Re <d|h>, Im <d|h>, <h|h>) per walker;
        d, w as sum_batch_loglike. `stream` is the group's (its partials buffer, grown here
        when the grid or the group outgrows it, belongs to that stream)."""
        torch = _torch()
        G = self.groups[gi]
        n = G.n
        nf = int(G.args[0].nf)
        _check_ll_io(torch, d, w, torch.empty(1, dtype=torch.float64), nf - int(G.args[0].k0), 1)
        _check_dh_out(torch, out, n)
        per = 3 * int(self.lib.efd_loglike_tile_count(nf))
        if G.dh_part is None or G.dh_part.numel() < per * n:
            with torch.cuda.stream(G.stream):
                G.dh_part = torch.empty(per * max(n, len(G.engines)), dtype=torch.float64,
                                        device=self.device)
        dp, wp, op = torch.view_as_real(d).data_ptr(), w.data_ptr(), out.data_ptr()
        pp = G.dh_part.data_ptr()
        for c0, cnt, pa_c, pw_c, pb_c in G.chunks[n]:
            _lib.check(self.lib.efd_modesum_sum_dh_hh(pa_c, pw_c, pb_c, cnt, dp, wp,
                                                      pp + 8 * per * c0, 1 if dense else 0,
                                                      op + 24 * c0, stream),
                       "efd_modesum_sum_dh_hh", self.lib)

    def release(self, gi, event):
        """The group's workspaces and inputs are free again once `event` (recorded after the sum
        that reads them) has completed."""
        self.groups[gi].busy = event

    def wait(self):
        """Synchronise every group and raise if any workspace reported a device-side error."""
        for G in self.groups:
            wss = [eng._ws.data_ptr() for eng in G.engines if eng._ws is not None]
            if not G.used or not wss:
                continue
            for c0 in range(0, len(wss), _lib.EFD_BATCH_MAX):
                part = wss[c0:c0 + _lib.EFD_BATCH_MAX]
                pw = (ctypes.c_void_p * len(part))(*part)
                if self.lib.efd_modesum_status_batch(pw, len(part), None,
                                                     G.stream.cuda_stream) != _lib.EFD_OK:
                    raise _lib.EFDError(_lib.last_error(self.lib))


def run_groups(prep, feed, n, G, step, used):
    """The batched callers' group loop: step(g0, slice(g0, g0 + G)) for every group of G of n
    walkers, each step's return value (the preparer group it took) appended to the caller's
    list `used` once the step is through. However the loop ends, the feed's futures are
    cancelled and the preparer forgets what was collected for a group that never flushed; the
    caller joins or synchronises the group streams (its own policy) around this call."""
    try:
        for g0 in range(0, n, G):
            used.append(step(g0, slice(g0, g0 + G)))
    finally:
        for f in feed.futs:
            f.cancel()
        prep.drop_pending()


def td_length(T, dt, odd_len=True):
    """Samples of FEW's padded TD output: the length of the FD grid for the same (T, dt)."""
    N = int(T * YRSID_SI / dt) + 1
    if odd_len and N % 2 == 0:
        N += 1
    return N


class TDEngine:
    """Owns the workspace of efd_td_modesum (time-domain mode sum) and launches it."""

    def __init__(self):
        self.lib = _lib.load()
        if not hasattr(self.lib, "efd_td_modesum"):
            raise _lib.EFDError("libemrifd.so lacks efd_td_modesum: rebuild it")
        self._ws = None

    def _workspace(self, nt, K, device):
        torch = _torch()
        nbytes = int(self.lib.efd_td_workspace_bytes(nt, K))
        if nbytes == 0:
            raise _lib.EFDError("efd_td_workspace_bytes rejected the shape")
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def launch(self, inp, dt, nsamples, out=None, hp=None, hc=None, scale=1.0 + 0.0j,
               accumulate=False, stream=None, prof_events=(None, None), window=None):
        """Asynchronous launch. out: float64 view of complex [nsamples] (h = h+ - i hx);
        hp / hc: real float64 [nsamples]; any of them may be None (not all). window: float64
        [nsamples] on the device, multiplied into every stored sample
        (efd_td_modesum_windowed); None is efd_td_modesum."""
        torch = _torch()
        dev = inp.t.device
        ws = self._workspace(inp.nt, inp.K, dev)
        ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
        a = _lib.TdArgs(
            t=inp.t.data_ptr(), phi_phi=inp.phi_phi.data_ptr(), phi_r=inp.phi_r.data_ptr(),
            f_phi=inp.f_phi.data_ptr(), f_r=inp.f_r.data_ptr(), nt=inp.nt,
            amp=inp.amp.data_ptr(), m=inp.m.data_ptr(), n=inp.n.data_ptr(),
            ylm_p=inp.ylm_p.data_ptr(), ylm_m=inp.ylm_m.data_ptr(), K=inp.K,
            dt=float(dt), nsamples=int(nsamples), scale_re=float(np.real(scale)),
            scale_im=float(np.imag(scale)), accumulate=1 if accumulate else 0, out=ptr(out),
            hp=ptr(hp), hc=ptr(hc), prof_begin=prof_events[0], prof_end=prof_events[1])
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        if window is not None:
            if (window.dtype != torch.float64 or window.dim() != 1 or not window.is_contiguous()
                    or int(window.numel()) != int(nsamples) or window.device != dev):
                raise ValueError(f"window: contiguous float64 [{int(nsamples)}] on {dev}")
            _lib.check(self.lib.efd_td_modesum_windowed(a, window.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), st),
                       "efd_td_modesum_windowed", self.lib)
            return ws
        _lib.check(self.lib.efd_td_modesum(a, ws.data_ptr(), ws.numel(), st), "efd_td_modesum",
                   self.lib)
        return ws

    def status(self, stream=None):
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        return self.lib.efd_modesum_status(self._ws.data_ptr(), st) == _lib.EFD_OK

    def run(self, inp, dt, nsamples, scale=1.0 + 0.0j, check=True):
        """Complex h = h+ - i hx (torch complex128 [nsamples] on the GPU)."""
        torch = _torch()
        h = torch.empty(int(nsamples), dtype=torch.complex128, device=inp.t.device)
        self.launch(inp, dt, nsamples, out=torch.view_as_real(h), scale=scale)
        if check and not self.status():
            raise _lib.EFDError(f"efd_td_modesum: {_lib.last_error(self.lib)}")
        return h


class TDInterpolatedModeSum:
    """FEW-compatible TD summation module (`InterpolatedModeSum` [FEW-ext]): the comparison
    waveform of the reference (td_gen, check_mode_by_mode.py:85-99; Tutorial_FrequencyDomain_
    Waveforms.ipynb:61-66). Output length is the FD grid's for the same (T, dt, odd_len), so
    fftshift(fft(h+)) dt lines up with `FDInterpolatedModeSum.frequency` (notebook :187-188)."""

    def __init__(self, pad_output=True, odd_len=True, use_gpu=True, output_type="td", **kwargs):
        if output_type != "td":
            raise ValueError("TDInterpolatedModeSum implements output_type='td' only")
        self.pad_output = pad_output
        self.odd_len = odd_len
        self.use_gpu = use_gpu
        self.output_type = output_type
        self.engine = TDEngine()

    def waveform(self, t, teuk_modes, ylm_p, ylm_m, Phi_phi, Phi_r, m_arr, n_arr, M, p, e,
                 dt=10.0, T=1.0, scale=1.0 + 0.0j):
        """Complex h = h+ - i hx (torch complex128 on the GPU), distance-scaled by `scale`."""
        om_phi, _, om_r = get_fundamental_frequencies(0.0, p, e, 0.0)
        f_phi = om_phi / (2.0 * np.pi * M * MTSUN_SI)
        f_r = om_r / (2.0 * np.pi * M * MTSUN_SI)
        inp = DeviceInputs.from_host(t, teuk_modes, Phi_phi, Phi_r, f_phi, f_r, m_arr, n_arr,
                                     ylm_p, ylm_m)
        if self.pad_output:
            ns = td_length(T, dt, self.odd_len)
        else:
            ns = int(np.searchsorted(np.arange(int(t[-1] / dt) + 2) * dt, t[-1], side="right"))
        return self.engine.run(inp, dt, ns, scale=scale)

    @staticmethod
    def polarizations(h):
        """[h+, hx] real (FEW TD list output) from h = h+ - i hx."""
        return h.real.contiguous(), (-h.imag).contiguous()


class FDInterpolatedModeSum:
    """FEW-compatible FD summation module (`create_waveform` of the waveform class)."""

    def __init__(self, pad_output=True, output_type="fd", odd_len=True, use_gpu=True,
                 caustic="uniform", **kwargs):
        if output_type != "fd":
            raise ValueError("this module implements output_type='fd' only")
        self.pad_output = pad_output
        self.output_type = output_type
        self.odd_len = odd_len
        self.use_gpu = use_gpu
        self.engine = ModeSumEngine(caustic=caustic)
        self.frequency = None
        self._freq_dev = None
        self._freq_key = None
        self._k0 = 0
        self._fh = None
        self._f_obj = None
        self._f_tag = None

    @property
    def caustic(self):
        return self.engine.caustic

    def _grid(self, T, dt, f_arr):
        torch = require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        if f_arr is not None:
            # the drivers pass the same f_arr object on every call (emri_pe.py:344-364): a
            # device tensor seen last time is taken as is (no device->host copy, so the walker
            # loop of a pipelined Likelihood never synchronises); a host array is compared with
            # the cached copy before any validation
            # (unless it was modified in place since: its version counter or storage moved)
            if (f_arr is self._f_obj and hasattr(f_arr, "detach")
                    and self._f_tag == (f_arr._version, f_arr.data_ptr())):
                return self._freq_dev, self._sym
            if hasattr(f_arr, "detach"):
                fh = f_arr.detach().cpu().numpy().astype(np.float64)
            else:
                fh = np.asarray(f_arr, dtype=np.float64)
            if (self._freq_key is not None and self._freq_key[0] == "f"
                    and np.array_equal(fh, self._fh)):
                self._remember(f_arr)
                return self._freq_dev, self._sym
            if fh.ndim != 1 or len(fh) == 0 or np.any(np.diff(fh) <= 0):
                raise ValueError("f_arr must be a strictly increasing 1-D frequency array")
            key = ("f", fh.tobytes())
        else:
            key = ("T", float(T), float(dt), bool(self.odd_len))
            fh = None
        if key != self._freq_key:
            if fh is None:
                fh = fd_grid(T, dt, self.odd_len)
            self._freq_dev = torch.as_tensor(fh, device=dev)
            self._sym = is_symmetric(fh)
            self._k0 = int(np.searchsorted(fh, 0.0))   # first f >= 0 bin (sorted grid)
            self._freq_key = key
            self._fh = fh
            self.frequency = self._freq_dev if self.use_gpu else fh
        self._remember(f_arr)
        return self._freq_dev, self._sym

    def _remember(self, f_arr):
        self._f_obj = f_arr
        self._f_tag = (f_arr._version, f_arr.data_ptr()) if hasattr(f_arr, "detach") else None

    def submit_channels(self, pipeline, out, t, teuk_modes, ylm_p, ylm_m, Phi_phi, Phi_r, m_arr,
                        n_arr, M, p, e, dt=10.0, T=1.0, f_arr=None, scale=1.0 + 0.0j,
                        f_phi=None, f_r=None, order=True, prepare_only=False):
        """Queue [h+, hx] over f >= 0 into the rows of out (complex128 [2][nf - k0]) on a
        WaveformPipeline slot: no host synchronisation. Symmetric grids (FEW's own and the
        drivers' downsampled f_arr) get the polarisations from the mode sum itself; other grids
        go through the spectrum and efd_polarizations on the slot's stream. Returns the slot."""
        torch = require_gpu()
        if f_phi is None or f_r is None:
            om_phi, _, om_r = get_fundamental_frequencies(0.0, p, e, 0.0)
            f_phi = om_phi / (2.0 * np.pi * M * MTSUN_SI)
            f_r = om_r / (2.0 * np.pi * M * MTSUN_SI)
        host = dict(t=t, amp=teuk_modes, phi_phi=Phi_phi, phi_r=Phi_r, f_phi=f_phi, f_r=f_r,
                    m=m_arr, n=n_arr, ylm_p=ylm_p, ylm_m=ylm_m)
        freq, sym = self._grid(T, dt, f_arr)
        nf, k0 = int(freq.numel()), self._k0
        if prepare_only:
            # the sum (and the fused likelihood) come later from pipeline.job(slot)
            if not sym:
                raise ValueError("submit_channels(prepare_only=True) needs a symmetric grid")
            return pipeline.submit(host, freq, True, scale, k0=k0, order=order,
                                   prepare_only=True)
        if (out.dtype != torch.complex128 or tuple(out.shape) != (2, nf - k0)
                or not out.is_contiguous()):
            raise ValueError(f"submit_channels: out must be contiguous complex128 [2][{nf - k0}]")
        if sym:
            return pipeline.submit(host, freq, True, scale, hp=torch.view_as_real(out[0]),
                                   hc=torch.view_as_real(out[1]), k0=k0, order=order)
        slot = pipeline.next_slot()
        sl = pipeline.slots[slot]
        st = pipeline.stream(slot)
        with torch.cuda.stream(st):
            S = sl.S
            if S is None or S.numel() != nf:
                sl.S = S = torch.empty(nf, dtype=torch.complex128, device=freq.device)
        pipeline.submit(host, freq, False, scale, out=torch.view_as_real(S), order=order)
        lib = self.engine.lib
        _lib.check(lib.efd_polarizations(torch.view_as_real(S).data_ptr(), nf, k0,
                                         torch.view_as_real(out[0]).data_ptr(),
                                         torch.view_as_real(out[1]).data_ptr(), st.cuda_stream),
                   "efd_polarizations", lib)
        return slot

    def spectrum(self, t, teuk_modes, ylm_p, ylm_m, Phi_phi, Phi_r, m_arr, n_arr, M, p, e,
                 dt=10.0, T=1.0, f_arr=None, scale=1.0 + 0.0j, f_phi=None, f_r=None, out=None,
                 check=True):
        """S(f) = h+ - i hx on the grid (torch complex128 on the GPU; into out when given;
        check=False: no status synchronisation, see ModeSumEngine.run). f_phi, f_r: the orbital
        frequencies at the knots when the upstream already has them (the native trajectory),
        else FEW's get_fundamental_frequencies(p, e) (the same values submit_channels uses, so
        an injection and a walker on the same parameters give bitwise the same template)."""
        if f_phi is None or f_r is None:
            om_phi, _, om_r = get_fundamental_frequencies(0.0, p, e, 0.0)
            f_phi = om_phi / (2.0 * np.pi * M * MTSUN_SI)
            f_r = om_r / (2.0 * np.pi * M * MTSUN_SI)
        inp = DeviceInputs.from_host(t, teuk_modes, Phi_phi, Phi_r, f_phi, f_r, m_arr, n_arr,
                                     ylm_p, ylm_m)
        freq, sym = self._grid(T, dt, f_arr)
        return self.engine.run(inp, freq, out=out, grid_symmetric=sym, scale=scale, check=check)

    def positive_start(self):
        """Index of the first f >= 0 bin of the last grid (emri_pe.py:239 mask, sorted grid);
        kept on the host when the grid is set up, so asking costs no device synchronisation."""
        if self._freq_key is None:
            raise ValueError("no grid yet: call the generator first")
        return self._k0

    def polarizations(self, S, mask_positive=False, out=None):
        """[h+, hx] (FEW list output) from S; mask_positive keeps f >= 0.

        out: optional (hp, hc) complex128 device tensors of the output length to write into
        (e.g. the two rows of a [2][N] channel buffer).
        """
        torch = require_gpu()
        nf = int(S.numel())
        k0 = self.positive_start() if mask_positive else 0
        if out is None:
            hp = torch.empty(nf - k0, dtype=torch.complex128, device=S.device)
            hc = torch.empty_like(hp)
        else:
            hp, hc = out
            for o in (hp, hc):
                if (o.dtype != torch.complex128 or o.numel() != nf - k0
                        or not o.is_contiguous() or o.device != S.device):
                    raise ValueError("polarizations: out tensors must be contiguous complex128 "
                                     f"of length {nf - k0} on {S.device}")
        lib = self.engine.lib
        st = torch.cuda.current_stream(S.device).cuda_stream
        _lib.check(lib.efd_polarizations(torch.view_as_real(S).data_ptr(), nf, k0,
                                         torch.view_as_real(hp).data_ptr(),
                                         torch.view_as_real(hc).data_ptr(), st),
                   "efd_polarizations", lib)
        return hp, hc

    def __call__(self, t, teuk_modes, ylms, Phi_phi, Phi_r, m_arr, n_arr, M, p, e, *args,
                 dt=10.0, T=1.0, f_arr=None, mask_positive=False, scale=1.0 + 0.0j, **kwargs):
        K = len(m_arr)
        S = self.spectrum(t, teuk_modes, ylms[:K], ylms[K:], Phi_phi, Phi_r, m_arr, n_arr, M, p,
                          e, dt=dt, T=T, f_arr=f_arr, scale=scale)
        hp, hc = self.polarizations(S, mask_positive)
        torch = _torch()
        return torch.stack([hp, hc])
