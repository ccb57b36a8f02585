"""Noise realisations on the device (efd_noise_fd, csrc/emrifd_noise.hip).

The reference stubbed its noise (lisatools/sampling/likelihood.py:183-199 raises before the
recipe; lisatools/utils/utility.py:5-13 generate_noise_fd holds the same recipe): on a bin of
spacing df and PSD S,
    n = sqrt(S) * (0.5 / sqrt(df)) * xi,   xi = N(0, 1) + i N(0, 1).
Here xi comes from a counter-based generator keyed on (seed, realization, channel, bin)
(Philox4x32-10 and Box-Muller, include/emrifd.h "Noise realisations"), so a stored seed
reproduces a data set on any machine and on every rank without a broadcast, whatever the launch
geometry, and a slice of a grid (bin0) is bitwise the whole grid's.

  standard_noise     0.5 * gain * xi as a device tensor [nchan][nbin] (the likelihood's weighted
                     space has gain = 1: its noise is 0.5 xi on every bin, whatever the PSD)
  generate_noise_fd  lisatools' helper for one channel of strain noise
  new_seed           a 63-bit seed from the OS
  check_seed         the range a caller's seed must lie in
"""

import os

import numpy as np

from .summation import require_gpu

_REDUCERS = {}


def _reducer(device):
    from .reductions import Reducer
    key = str(device)
    if key not in _REDUCERS:
        _REDUCERS[key] = Reducer(device)
    return _REDUCERS[key]


def new_seed():
    """A seed from the OS's entropy (63 bits, so that it survives a signed 64-bit store)."""
    return int.from_bytes(os.urandom(8), "little") >> 1


def check_seed(seed, what="noise_seed"):
    """`seed` as an int the generator's 64-bit key holds, or ValueError."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what}: an integer in 0..2^64 - 1")
    return seed


def standard_noise(nchan, nbin, seed, realization=0, bin0=0, gain=None, out=None,
                   accumulate=False):
    """gain[c][i] * 0.5 * xi(c, bin0 + i) as a complex128 [nchan][nbin] device tensor (written
    into `out`, or added to it with accumulate). gain: float64 [nchan][nbin] (a device tensor or
    anything numpy converts) or None (= 1); a gain of 0 or NaN leaves its bin without noise."""
    torch = require_gpu()
    if out is None:
        if accumulate:
            raise ValueError("standard_noise: accumulate needs out")
        dev = torch.device("cuda", torch.cuda.current_device())
        out = torch.empty((int(nchan), int(nbin)), dtype=torch.complex128, device=dev)
    elif tuple(out.shape) != (int(nchan), int(nbin)):
        raise ValueError(f"out: expected shape {(int(nchan), int(nbin))}, got {tuple(out.shape)}")
    if gain is not None and not hasattr(gain, "detach"):
        gain = torch.as_tensor(np.ascontiguousarray(gain, dtype=np.float64), device=out.device)
    return _reducer(out.device).noise_fd(out, seed, realization, bin0, gain, accumulate)


def generate_noise_fd(freqs, df, seed=None, realization=0, channel=0, sensitivity_fn=None,
                      **sensitivity_kwargs):
    """lisatools.utils.utility.generate_noise_fd with the draw made on the device: strain noise
    sqrt(S(freqs)) * 0.5 / sqrt(df) * xi(channel, k) on the bins k = 0 .. len(freqs) - 1 as a
    complex128 device tensor. df: a float, or one spacing per bin. sensitivity_fn(freqs,
    **sensitivity_kwargs) gives the PSD; None is this package's sensitivity.get_sensitivity (pass
    sens_fn="cornish_lisa_psd", the curve built here), fdutils.get_sensitivity is the drivers'
    table. seed=None draws one from the OS (new_seed: not reproducible; pass a seed to keep it).
    Bins where the PSD or df is 0, negative or not finite get no noise."""
    torch = require_gpu()
    if sensitivity_fn is None:
        from .sensitivity import get_sensitivity as sensitivity_fn
    fh = freqs.detach().cpu().numpy() if hasattr(freqs, "detach") else np.asarray(freqs)
    psd = sensitivity_fn(fh, **sensitivity_kwargs)
    psd = psd.detach().cpu().numpy() if hasattr(psd, "detach") else np.asarray(psd)
    with np.errstate(invalid="ignore", divide="ignore"):
        amp = (np.asarray(psd, dtype=np.float64) / np.asarray(df, dtype=np.float64)) ** 0.5
    amp = np.where(np.isfinite(amp), amp, 0.0) * np.ones(len(fh))
    channel = int(channel)
    # the kernel's channels count from 0: the ones before `channel` have gain 0 (no draw)
    gain = np.zeros((channel + 1, len(fh)))
    gain[channel] = amp
    seed = new_seed() if seed is None else seed
    return standard_noise(channel + 1, len(fh), seed, realization, gain=gain)[channel]
