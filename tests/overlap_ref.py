"""Shared pieces of the overlap tests: the fixture, the toy model and transform it was made from
(tests/golden/make_golden_overlap.py), ctypes calls of efd_overlap_rows_cpu on numpy arrays and
the same sums in plain numpy."""

import ctypes
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_golden.npz")

PARAMS = np.array([0.0, 0.0, 0.0, 0.3, 0.02])   # (x0, x1, x2, phi, qS), scaled coordinates
EPS = np.full(5, 1e-4)
SEED = 20081
NUM_SAMPLES = 40
APPROX_SCALE = 1.001


def golden():
    return np.load(GOLDEN)


def toy_inputs():
    f = np.linspace(1e-4, 1e-2, 4098)[1:]
    psd = 1e-40 * (1.0 + (2e-3 / f) ** 4 + (f / 5e-3) ** 2)   # the Fisher fixture's PSD
    return f, psd


class ToyTransform:
    """The five sampled coordinates to the model's 11-vector: slots 7..10 are (qS, phiS, qK,
    phiK), where mismatch_criterion wraps its polar angles (diagnostic.py:597-604)."""

    def transform_base_parameters(self, p):
        out = np.zeros(11)
        out[0] = np.log(1e-17) + p[0]
        out[1] = 3e-3 + 1e-5 * p[1]
        out[2] = 2e3 + 50.0 * p[2]
        out[3] = p[3]
        out[7] = p[4]
        out[8], out[9], out[10] = 1.0, 0.4, 2.0
        return out


def toy_model(f, scale=1.0):
    def model(lnA, f0, tau, phi, p4, p5, p6, qS, phiS, qK, phiK):
        env = scale * np.exp(lnA) * np.exp(-0.5 * ((f - f0) * tau) ** 2)
        ph = np.exp(1j * (2 * np.pi * (f - f0) * tau + phi))
        return np.array([env * ph * (1 + 0.5 * qS) * np.exp(0.2j * phiS),
                         0.5j * env * ph * (1 + 0.1 * f / f0) * (1 - 0.3 * qS)
                         * np.exp(-0.1j * phiS)])
    return model


def weights(f, psd, nchan):
    x = np.empty_like(f)
    x[1:] = np.diff(f)
    x[0] = x[1]
    return np.ascontiguousarray(np.tile(x / psd, nchan))


def perturbed_points(params, offsets, transform):
    """mismatch_criterion's perturbed, transformed and wrapped parameter vectors (:590-604) for
    the stored offsets, and which of them were reflected."""
    pts, refl = [], []
    for d in offsets:
        v = transform.transform_base_parameters(np.asarray(params) + d)
        hit = False
        for val in (7, 9):
            v[val] = v[val] % (2 * np.pi)
            if v[val] > np.pi:
                v[val] = 2 * np.pi - v[val]
                v[val + 1] += np.pi
                hit = True
        pts.append(v)
        refl.append(hit)
    return pts, np.array(refl)


def criterion(res, offsets, fish):
    """(over, mism, ratio) from efd_overlap_rows' numbers (diagnostic.py:609-639)."""
    rr = res[-1]
    over = res[0:-1:3] / np.sqrt(res[2:-1:3] * rr)
    prod = np.einsum("kj,ji,ki->k", offsets, fish, offsets)
    return over, (1.0 - over) / 2.0, over / (1 - 0.5 * prod / rr)


def overlap_numpy(rows, t, u, w):
    """efd_overlap_rows' outputs [3 nrow + 1] as plain float64 numpy sums."""
    rows = np.asarray(rows, dtype=np.complex128).reshape(len(rows), -1)
    r = np.asarray(t, dtype=np.complex128).reshape(-1)
    if u is not None:
        r = r - np.asarray(u, dtype=np.complex128).reshape(-1)
    w = np.ones(rows.shape[1]) if w is None else np.asarray(w).reshape(-1)
    x = 4.0 * np.einsum("ke,e,e->k", rows.conj(), r, w)
    nn = 4.0 * np.einsum("ke,e->k", np.abs(rows) ** 2, w)
    out = np.empty(3 * len(rows) + 1)
    out[0:-1:3], out[1:-1:3], out[2:-1:3] = x.real, x.imag, nn
    out[-1] = 4.0 * np.sum(w * np.abs(r) ** 2)
    return out


def random_case(nelem, nrow, seed=0, pad=0):
    rng = np.random.default_rng([seed, nelem, nrow])
    rows = rng.normal(size=(nrow, nelem + pad)) + 1j * rng.normal(size=(nrow, nelem + pad))
    t = rng.normal(size=nelem) + 1j * rng.normal(size=nelem)
    u = rng.normal(size=nelem) + 1j * rng.normal(size=nelem)
    w = rng.uniform(0.5, 2.0, size=nelem)
    return rows, t, u, w


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def overlap_cpu(rows, t, u, w, nelem=None, row_stride=None, nrow=None):
    """efd_overlap_rows_cpu on host arrays: rows complex128 [nrow][row_stride]; returns
    (rc, out [3 nrow + 1])."""
    from emri_frequencydomainwaveforms_amd import _lib
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.complex128)
    rows = rows.reshape(len(rows), -1)
    nrow = rows.shape[0] if nrow is None else nrow
    row_stride = rows.shape[1] if row_stride is None else row_stride
    nelem = rows.shape[1] if nelem is None else nelem
    t = np.ascontiguousarray(t, dtype=np.complex128)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.complex128)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    out = np.full(3 * max(nrow, 0) + 1, np.nan)
    rc = lib.efd_overlap_rows_cpu(_ptr(rows), row_stride, nrow, _ptr(t), _ptr(u), _ptr(w), nelem,
                                  _ptr(out), None, None)
    return rc, out


def cross_err(a, ref):
    """max over rows of |cross terms - ref| / sqrt(nn_k rr): the inner-product tolerance's
    normalisation."""
    s = np.sqrt(ref[2:-1:3] * ref[-1])
    s = np.where(s > 0.0, s, 1.0)
    return float(max(np.max(np.abs(a[0:-1:3] - ref[0:-1:3]) / s),
                     np.max(np.abs(a[1:-1:3] - ref[1:-1:3]) / s)))


def norm_err(a, ref):
    """max relative error of the norms nn_k and rr."""
    n = np.concatenate([ref[2:-1:3], ref[-1:]])
    m = np.concatenate([a[2:-1:3], a[-1:]])
    return float(np.max(np.abs(m - n) / np.where(n > 0.0, n, 1.0)))
