"""The noise draws' reference: Philox4x32-10 in numpy uint64 arithmetic and the Box-Muller step
in np.longdouble from the exact 53-bit integers (include/emrifd.h, "Noise realisations"). Shared by
test_noise_ref.py (the host twins) and test_gpu_noise.py (the device); a reference array is made
once per (seed, realisation, shape) and handed out read-only."""

import ctypes
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
XI_MAX = 8.57   # sqrt(-2 ln 2^-53)
# Salmon et al.'s known answers: (counter, key) -> words
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays (or scalars) holding 32-bit words; returns the four words."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK)
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def draw_bits(seed, realisation, channel, bins):
    """(a, b) of the draws at the 64-bit bin indices `bins`: u1 = (a + 1) 2^-53, u2 = b 2^-53."""
    k = np.asarray(bins, dtype=np.uint64)
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10(k & MASK, k >> np.uint64(32),
                                   np.full(k.shape, channel, dtype=np.uint64),
                                   np.full(k.shape, realisation, dtype=np.uint64),
                                   seed & 0xFFFFFFFF, seed >> 32)
    a = (w0 << np.uint64(21)) | (w1 >> np.uint64(11))
    b = (w2 << np.uint64(21)) | (w3 >> np.uint64(11))
    return a, b


def xi_longdouble(seed, realisation, channel, bins):
    """The unit complex normals as (re, im) np.longdouble arrays."""
    a, b = draw_bits(seed, realisation, channel, bins)
    L = np.longdouble
    two53 = L(2) ** 53
    u1 = (a.astype(L) + L(1)) / two53      # uint64 -> long double is exact (64-bit mantissa)
    u2 = b.astype(L) / two53
    r = np.sqrt(L(-2) * np.log(u1))
    ph = L(2) * np.arctan2(L(0), L(-1)) * u2    # 2 pi u2, pi in long double
    return r * np.cos(ph), r * np.sin(ph)


@functools.lru_cache(maxsize=None)
def xi(seed, realisation, nchan, nbin, bin0=0):
    """complex128 [nchan][nbin] of xi(c, bin0 + i), rounded from the long-double values;
    read-only (cached)."""
    bins = np.uint64(bin0) + np.arange(nbin, dtype=np.uint64)
    out = np.empty((nchan, nbin), dtype=np.complex128)
    for c in range(nchan):
        re, im = xi_longdouble(seed, realisation, c, bins)
        out[c] = re.astype(np.float64) + 1j * im.astype(np.float64)
    out.setflags(write=False)
    return out


# ---- the host twins on numpy arrays ---------------------------------------------------------
def _ptr(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def noise_fd_cpu(lib, nchan, nbin, seed, realisation=0, bin0=0, gain=None, out=None,
                 accumulate=False):
    if out is None:
        out = np.full((nchan, nbin), np.nan + 1j * np.nan, dtype=np.complex128)
    rc = lib.efd_noise_fd_cpu(_ptr(out), _ptr(gain), nchan, nbin, bin0, seed, realisation,
                              int(accumulate), None)
    assert rc == 0
    return out


def noise_overlap_rows_cpu(lib, rows, gain, seed, real0, ndraw):
    nrow, nchan, nbin = rows.shape
    out = np.full((ndraw, nrow), np.nan)
    rc = lib.efd_noise_overlap_rows_cpu(_ptr(rows), nrow, _ptr(gain), nchan, nbin, seed, real0,
                                        ndraw, _ptr(out), None, None)
    assert rc == 0
    return out


def overlap_case(seed, nrow, nchan, nbin):
    """Random rows and a random gain with zeros (and one NaN where there is room)."""
    rng = np.random.default_rng(seed)
    rows = np.ascontiguousarray(rng.standard_normal((nrow, nchan, nbin))
                                + 1j * rng.standard_normal((nrow, nchan, nbin)))
    gain = rng.uniform(0.5, 2.0, (nchan, nbin))
    gain[rng.uniform(size=gain.shape) < 0.2] = 0.0
    if nbin > 2:
        gain[-1, 1] = np.nan
    return rows, gain


def overlaps_explicit(rows, gain, seed, real0, ndraw):
    """(value, bound) of the overlaps from explicit noise buffers contracted in float64 numpy:
    value[r][p] = sum gain Re(conj xi_r rows_p), bound[p] = 1e-12 sum |gain rows_p| 8.57."""
    nrow, nchan, nbin = rows.shape
    g = np.where(np.isnan(gain) | (gain == 0.0), 0.0, gain)
    gr = g[None] * rows
    val = np.empty((ndraw, nrow))
    for j in range(ndraw):
        x = xi(seed, real0 + j, nchan, nbin)
        val[j] = np.sum(x.real[None] * gr.real + x.imag[None] * gr.imag, axis=(1, 2))
    return val, 1e-12 * np.sum(np.abs(gr), axis=(1, 2)) * XI_MAX
