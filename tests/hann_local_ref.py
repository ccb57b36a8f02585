"""A plain float64 reference of the fused windowed logL (efd_hann_loglike_local) -- TEST
INFRASTRUCTURE ONLY. numpy alone: no call into the library and none of fdutils.HannConvolution's
arithmetic. It restates the definitions of include/emrifd.h and DESIGN.md (Round 6):

  lag kernel   K[0] = i pi (n-1)/n,  K[j] = (pi/n) cot(pi j/n) - i pi/n   (j != 0)
  correction   C[k] = sum_j K[(k-j) mod n] S[j]
  window       S_w[k] = S[k]/2 - (S[k+1] + S[k-1])/4 - (C[k+1] - C[k-1]) / (4 (n-1)),  indices mod n
  logL         h+ = (a + conj b)/2, hx = i (a - conj b)/2, a = S_w[k], b = S_w[n-1-k], k >= k0;
               logL = -2 sum |d - w h|^2  (oracle/likelihood_oracle.loglike's convention)
  emit         e[k] = wl[k] S_w[k], e[n] = e[kself]

The cotangent is taken at the lag reduced to (-n/2, n/2] (cot is odd and pi-periodic), so it
keeps its relative precision at the lags next to n; tables of n <= 8200 lags are computed in
longdouble and rounded once."""

import numpy as np

SMALL = 8200   # grids up to here: longdouble lag table, and the n x n product is affordable


def _cot_table(n):
    """c[u] = (pi/n) cot(pi u/n) for u = 0..n-1 (c[0] = 0), float64."""
    n = int(n)
    ft = np.longdouble if n <= SMALL else np.float64
    pn = 4 * np.arctan(ft(1)) / ft(n)               # pi / n in ft's own precision
    half = n // 2                                   # lags 1..half are their own reduced form
    u = np.arange(1, half + 1, dtype=np.int64).astype(ft)
    t = pn / np.tan(pn * u)
    c = np.zeros(n, dtype=ft)
    c[1:half + 1] = t
    # cot(pi (n-u)/n) = -cot(pi u/n): lags half+1..n-1 from 1..n-1-half
    c[half + 1:] = -t[:n - 1 - half][::-1]
    if n % 2 == 0:
        c[half] = 0.0                               # cot(pi/2)
    return c.astype(np.float64)


def lag_kernel(n):
    """K[0..n-1], complex128."""
    n = int(n)
    K = np.empty(n, dtype=np.complex128)
    K.real = _cot_table(n)
    K.imag = -np.pi / n
    K[0] = 1j * np.pi * (n - 1) / n
    return K


def correction_sum(S, K=None):
    """C by the direct sum over the nonzero bins of S, O(n nnz): every K[(k-j) mod n] over k is
    a slice of K laid out twice."""
    S = np.asarray(S, dtype=np.complex128)
    n = len(S)
    K = lag_kernel(n) if K is None else K
    K2 = np.concatenate((K, K))                     # K2[n + u] = K[u mod n] for u in [-n, n)
    C = np.zeros(n, dtype=np.complex128)
    for j in np.nonzero(S)[0]:
        C += S[j] * K2[n - j:2 * n - j]             # k - j for k = 0..n-1
    return C


def correction_matrix(S, K=None):
    """C by the n x n product with the circulant K[(k-j) mod n] (n <= SMALL). S: [n] or
    [rows][n]."""
    S = np.asarray(S, dtype=np.complex128)
    n = S.shape[-1]
    if n > SMALL:
        raise ValueError("correction_matrix: small grids only")
    K = lag_kernel(n) if K is None else K
    i = np.arange(n, dtype=np.int32)
    A = K[(i[:, None] - i[None, :]) % n]
    return (A @ S.T).T if S.ndim == 2 else A @ S


def correction_fft(S, K=None):
    """C by one zero-padded complex128 linear convolution of S with K at the lags -(n-1)..n-1
    (no wrap: exact up to the transforms' rounding)."""
    import scipy.fft as sf
    S = np.asarray(S, dtype=np.complex128)
    n = len(S)
    K = lag_kernel(n) if K is None else K
    Kext = np.concatenate((K[1:], K))               # lag u at u + n - 1
    L = sf.next_fast_len(3 * n - 2)
    full = sf.ifft(sf.fft(S, L) * sf.fft(Kext, L))
    return full[n - 1:2 * n - 1].copy()


def correction(S, form=None, K=None):
    """C = K (*) S. form: 'sum', 'matrix' or 'fft'; by default the sum for sparse rows, else the
    matrix on small grids and the transform on large ones."""
    S = np.asarray(S, dtype=np.complex128)
    if form is None:
        nnz = int(np.count_nonzero(S))
        form = "sum" if nnz <= 64 else ("matrix" if len(S) <= SMALL else "fft")
    return {"sum": correction_sum, "matrix": correction_matrix, "fft": correction_fft}[form](S, K)


def windowed(S, C=None):
    """S_w of S (first-order Hann form), indices mod n."""
    S = np.asarray(S, dtype=np.complex128)
    n = S.shape[-1]
    C = correction(S) if C is None else C
    return (0.5 * S - 0.25 * (np.roll(S, -1, -1) + np.roll(S, 1, -1))
            - (np.roll(C, -1, -1) - np.roll(C, 1, -1)) / (4.0 * (n - 1)))


def polarizations(Sw, k0):
    """[h+, hx] over the bins k >= k0 of the windowed spectrum."""
    n = len(Sw)
    k = np.arange(int(k0), n)
    a, b = Sw[k], np.conj(Sw[n - 1 - k])
    return np.stack([0.5 * (a + b), 0.5j * (a - b)])


def residual(Sw, d, w, k0):
    """d - w h, [2][n - k0] (d already weighted, as efd_loglike takes it)."""
    return d - w * polarizations(Sw, k0)


def loglike(Sw, d, w, k0):
    r = residual(Sw, d, w, k0)
    return -2.0 * float(np.sum(r.real ** 2 + r.imag ** 2))


def local_data_ref(Sw, wl, kself):
    """The emit definition: wl[k] S_w[k] and element n = element kself (0 without one)."""
    n = len(Sw)
    e = np.zeros(n + 1, dtype=np.complex128)
    e[:n] = wl * Sw
    if kself >= 0:
        e[n] = e[kself]
    return e


def local_weight(n, w1, k0):
    """wl over the grid: the weight of a kept bin k >= k0 at k and at its mirror n-1-k."""
    n, k0 = int(n), int(k0)
    wl = np.zeros(n)
    k = np.arange(k0, n)
    wl[n - 1 - k] = w1
    wl[k] = w1
    return wl
