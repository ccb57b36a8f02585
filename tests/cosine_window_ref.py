"""numpy reference of the cosine-sum windows' first-order form (fdutils.CosineWindowConvolution,
include/emrifd.h efd_cosw_*), shared by tests/test_cosine_window.py and
tests/test_gpu_cosine_window.py.

scipy's symmetric cosine-sum windows are w[n] = sum_j (-1)^j a_j cos(2 pi j n / (N - 1)). With
e = 1 / (N - 1) and S~ the DFT's trigonometric interpolant of S, ifft(w fft(S))[k] =
sum_j (-1)^j (a_j / 2) (S~(k + j (1 + e)) + S~(k - j (1 + e))), and to first order in e
  S_w[k] = a_0 S[k] + sum_{j>=1} (-1)^j (a_j / 2) [S[k+j] + S[k-j] + j e (C[k+j] - C[k-j])],
C = S~' at the integers (indices mod N). The dropped term scales with j^2 a_j per shift: scaled
from the Hann bound (5 / N^2 of max|S| at a_1 = 1/2) it is 10 q / N^2, q = sum_j a_j j^2.
"""

import numpy as np

WINDOWS = {
    "hann": (0.5, 0.5),
    "hamming": (0.54, 0.46),
    "blackman": (0.42, 0.5, 0.08),
    "nuttall": (0.3635819, 0.4891775, 0.1365995, 0.0106411),
    "blackmanharris": (0.35875, 0.48829, 0.14128, 0.01168),
}


def q(a):
    """sum_j a_j j^2."""
    return sum(aj * j * j for j, aj in enumerate(a))


def bound(a, n):
    """The first-order form's truncation bound, as a fraction of max|S|."""
    return 10.0 * q(a) / float(n) ** 2


def stencil_weight(a):
    """2 sum_j j a_j: the weight of the complex64 correction in the stencil relative to the
    Hann window's (1 = 2 * 1 * 1/2), the factor the Hann tests' tol_pol is scaled by."""
    return 2.0 * sum(j * aj for j, aj in enumerate(a))


def spectrum(n, seed=0, rows=None):
    """A random-phase spectrum of n bins whose lower third is zero: independent normal real and
    imaginary parts, as the Hann tests draw theirs (the measured error / bound figures quoted
    in the tests are for this spectrum, whose max|S| is ~4 times its rms)."""
    rng = np.random.default_rng(seed)
    shape = (n,) if rows is None else (rows, n)
    S = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    S[..., : n // 3] = 0.0
    return S


def exact_correction(S):
    """C[k] = S~'(k) in complex128: S~(u) = (1/N) sum_n fft(S)[n] exp(2 pi i n u / N), so
    C = ifft(2 pi i n / N * fft(S)) (the circular convolution of S with the lag kernel
    K[m] = -i pi / N + (pi / N) cot(pi m / N), K[0] = i pi (N - 1) / N)."""
    n = S.shape[-1]
    return np.fft.ifft(2j * np.pi * np.arange(n) / n * np.fft.fft(S, axis=-1), axis=-1)


def lag_kernel_correction(S):
    """The same C as the circular convolution with the lag kernel K (one row)."""
    n = len(S)
    m = np.arange(1, n)
    K = np.empty(n, dtype=np.complex128)
    K[0] = 1j * np.pi * (n - 1) / n
    K[1:] = -1j * np.pi / n + (np.pi / n) / np.tan(np.pi * m / n)
    return np.fft.ifft(np.fft.fft(K) * np.fft.fft(S))


def first_order(S, a, C):
    """The first-order windowed spectrum of S (last axis: bins) given the correction C."""
    n = S.shape[-1]
    e = 1.0 / (n - 1)
    out = a[0] * S
    for j in range(1, len(a)):
        b = (-1) ** j * 0.5 * a[j]
        out = out + b * (np.roll(S, -j, axis=-1) + np.roll(S, j, axis=-1)
                         + j * e * (np.roll(C, -j, axis=-1) - np.roll(C, j, axis=-1)))
    return out


def dft_form(S, w):
    """ifft(w fft(S)): the exact windowed spectrum."""
    return np.fft.ifft(w * np.fft.fft(S, axis=-1), axis=-1)


def polarizations(Sw, k0):
    """h+ = (S + conj(S_flip)) / 2, hx = i (S - conj(S_flip)) / 2 over bins [k0, n)."""
    M = np.conj(Sw[::-1])
    return (0.5 * (Sw + M))[k0:], (0.5j * (Sw - M))[k0:]
