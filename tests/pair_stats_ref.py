"""Shared pieces of the pair-statistics tests: seeded row pairs, efd_pair_stats' sums in plain
numpy, ctypes calls of the CPU twins on numpy arrays, and the tolerances.

Tolerances (twin or kernel against numpy): 1e-12 of the sum of absolute terms for aa, bb and dd
(their terms are non-negative for w >= 0, so that sum is the value itself) and 1e-12 of
sqrt(aa bb) for abr and abi: the project's inner-product tolerance; both sides form the same
float64 terms and only the order differs. Where b comes from a split of Z, numpy's b differs from
the twin's by rounding, and a Cauchy-Schwarz term from the measured distance
delta = sqrt(4 sum w |b_numpy - b_twin|^2) is added: sqrt(aa) delta on ab,
2 sqrt(bb) delta + delta^2 on bb, 2 sqrt(dd) delta + delta^2 on dd.
"""

import ctypes

import numpy as np

RTOL = 1e-12
NBINS = (1, 63, 257, 8194)
NROWS = (1, 9, 64)
GAIN = 20.0


def random_pairs(nbin, nrow, nchan, seed=0, pad=0):
    """a, b complex [nrow][nchan * nbin + pad] (the padding NaN) and w [nbin]."""
    rng = np.random.default_rng([seed, nbin, nrow, nchan])
    ne = nchan * nbin

    def rows():
        x = np.full((nrow, ne + pad), np.nan + 1j * np.nan)
        x[:, :ne] = rng.normal(size=(nrow, ne)) + 1j * rng.normal(size=(nrow, ne))
        return x

    return rows(), rows(), rng.uniform(0.5, 2.0, size=nbin)


def near_equal_pairs(nbin, nrow, seed=3):
    """b = a (1 + 1e-7 smooth): pairs at mismatch about 1e-15 whose dd is about 1e-14 aa."""
    rng = np.random.default_rng([seed, nbin, nrow])
    a = rng.normal(size=(nrow, 2 * nbin)) + 1j * rng.normal(size=(nrow, 2 * nbin))
    x = np.linspace(0.0, 1.0, 2 * nbin)
    smooth = np.cos(3.0 * x) + 1j * np.sin(5.0 * x)
    return a, a * (1.0 + 1e-7 * smooth), rng.uniform(0.5, 2.0, size=nbin)


def pair_numpy(a, b, w, nchan, nbin):
    """efd_pair_stats' outputs [nrow][nchan][5] as plain float64 numpy sums."""
    a = np.asarray(a)[:, :nchan * nbin].reshape(len(a), nchan, nbin)
    b = np.asarray(b)[:, :nchan * nbin].reshape(len(b), nchan, nbin)
    w = np.ones(nbin) if w is None else np.asarray(w)
    ab = 4.0 * np.sum(w * np.conj(a) * b, axis=-1)
    out = np.empty((len(a), nchan, 5))
    out[..., 0] = 4.0 * np.sum(w * np.abs(a) ** 2, axis=-1)
    out[..., 1] = 4.0 * np.sum(w * np.abs(b) ** 2, axis=-1)
    out[..., 2], out[..., 3] = ab.real, ab.imag
    out[..., 4] = 4.0 * np.sum(w * np.abs(a - b) ** 2, axis=-1)
    return out


def errors(got, ref, delta=None):
    """(err, allowed) [nrow][nchan][5] under the module's tolerances; delta [nrow][nchan]."""
    aa, bb, dd = ref[..., 0], ref[..., 1], ref[..., 4]
    tol = np.empty_like(ref)
    tol[..., 0], tol[..., 1], tol[..., 4] = RTOL * aa, RTOL * bb, RTOL * dd
    tol[..., 2] = tol[..., 3] = RTOL * np.sqrt(aa * bb)
    if delta is not None:
        tol[..., 1] += 2.0 * np.sqrt(bb) * delta + delta ** 2
        tol[..., 2] += np.sqrt(aa) * delta
        tol[..., 3] += np.sqrt(aa) * delta
        tol[..., 4] += 2.0 * np.sqrt(dd) * delta + delta ** 2
    return np.abs(got - ref), tol


def assert_close(got, ref, delta=None, what=""):
    err, tol = errors(got, ref, delta)
    scale = np.where(tol > 0.0, tol, 1.0)
    print(f"{what}: max err / allowed {np.max(err / scale):.3e}")
    assert np.all(err <= tol), what


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.ctypes.data)


def _lib():
    from emri_frequencydomainwaveforms_amd import _lib as L
    return L.load()


def pair_cpu(a, b, w, nchan, nbin, nrow=None, a_stride=None, b_stride=None):
    """efd_pair_stats_cpu on complex [nrow][stride] arrays -> (rc, [nrow][nchan][5])."""
    a = np.ascontiguousarray(a, dtype=np.complex128)
    b = np.ascontiguousarray(b, dtype=np.complex128)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    nrow = a.shape[0] if nrow is None else nrow
    out = np.full((max(nrow, 1), max(nchan, 1), 5), 7.0)
    rc = _lib().efd_pair_stats_cpu(_ptr(a), a.shape[1] if a_stride is None else a_stride, _ptr(b),
                                   b.shape[1] if b_stride is None else b_stride, nrow, nchan,
                                   nbin, _ptr(w), _ptr(out), None, None)
    return rc, out


def split_pair_cpu(Zbuf, n, gain, a, w, keep=None):
    """efd_td_split_pair_stats_cpu on Z [rows][stride] and a [rows][a_stride] -> [rows][2][5]."""
    Zbuf = np.ascontiguousarray(Zbuf, dtype=np.complex128)
    a = np.ascontiguousarray(a, dtype=np.complex128)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    k8 = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    rows = Zbuf.shape[0]
    out = np.full((rows, 2, 5), 7.0)
    rc = _lib().efd_td_split_pair_stats_cpu(_ptr(Zbuf), Zbuf.shape[1], n, rows, gain, _ptr(a),
                                            a.shape[1], _ptr(w), _ptr(k8), _ptr(out), None, None)
    assert rc == 0, rc
    return out


def split_case(n, rows, seed=0, a_pad=3):
    """Z = fft of seeded series in a padded buffer, a [rows][2 nb + a_pad] near the split's scale,
    w [nb] with zeros folded in."""
    from tests import td_template_ref as tr
    h = tr.series(rows, n, seed=11 * n + rows + seed)
    Z = np.fft.fft(h, axis=-1)
    nb = (n + 1) // 2
    rng = np.random.default_rng([seed, n, rows])
    a = np.full((rows, 2 * nb + a_pad), np.nan + 1j * np.nan)
    a[:, :2 * nb] = GAIN * np.sqrt(n) * (rng.normal(size=(rows, 2 * nb))
                                         + 1j * rng.normal(size=(rows, 2 * nb)))
    w = rng.uniform(0.1, 2.0, size=nb)
    w[2::5] = 0.0
    return Z, tr.strided(Z, n + 5), a, w


def split_delta(b_np, b_twin, w):
    """sqrt(4 sum w |b_numpy - b_twin|^2) per row and channel."""
    return np.sqrt(4.0 * np.sum(w * np.abs(b_np - b_twin) ** 2, axis=-1))


def windows_case(n, nwin=4, seed=5):
    rng = np.random.default_rng([seed, n])
    h = rng.normal(size=n) + 1j * rng.normal(size=n)
    win = [rng.uniform(0.0, 1.0, size=n) for _ in range(nwin)]
    win[1] = None                       # the unwindowed row
    if n > 1:
        win[0][0] = win[0][-1] = 0.0    # a window that ends in zeros, as hann does
    return h, win


def window_rows_numpy(h, win, stride):
    """[nwin][stride] with each part one real product; the padding keeps the fill value."""
    out = np.full((len(win), stride), 7.0 + 7.0j)
    for j, x in enumerate(win):
        if x is None:
            out[j, :len(h)] = h
        else:
            out[j, :len(h)].real = x * h.real
            out[j, :len(h)].imag = x * h.imag
    return out


def window_rows_cpu(h, win, stride):
    h = np.ascontiguousarray(h, dtype=np.complex128)
    ptrs = (ctypes.c_void_p * len(win))(*[None if x is None else x.ctypes.data for x in win])
    out = np.full((len(win), stride), 7.0 + 7.0j)
    rc = _lib().efd_window_rows_cpu(_ptr(h), len(h), ptrs, len(win), _ptr(out), stride, None)
    assert rc == 0, rc
    return out


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint64),
                          np.ascontiguousarray(y).view(np.uint64))
