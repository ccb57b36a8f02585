"""The float64 reference of the fused windowed logL (tests/hann_local_ref.py) held to closed
forms and to the project's own CPU statements, before the GPU tests rely on it. No GPU needed.

  - a delta at bin j gives C[k] = K[(k-j) mod n] exactly, in every form's sum;
  - the three evaluations of C = K (*) S (direct sum over the nonzero bins, n x n product,
    zero-padded complex128 transform) agree to 1e-13 of max|C|: n = 4097 and 4096 (dense rows,
    all three) and a sparse row at n = 1,000,001 (sum against transform);
  - windowed() is within 5/n^2 of max|S| of the exact form ifft(hann(n) fft(S)) at n = 4097 and
    100,001 (HannConvolution.TOL's bound, test_hann_convolution_matches_dft_form);
  - loglike() (the mirror-pair form on h+, hx) equals the per-bin sum over local_layout's dl, wl
    (tests/test_hann_local_layout.py) at 1e-12 relative, odd and even n."""

import numpy as np
import pytest

from tests import hann_local_ref as ref


@pytest.mark.parametrize("n", [11, 12, 4097, 4096])
def test_lag_kernel_definition(n):
    K = ref.lag_kernel(n)
    # the plain formula at the lags up to n/2 (next to j = n its argument loses relative
    # precision: those lags are held by the oddness below)
    j = np.arange(1, n // 2 + 1)
    want = (np.pi / n) / np.tan(np.pi * j / n)
    assert np.max(np.abs(K[j].real - want)) <= 4e-16 * np.max(np.abs(want))
    assert np.all(K[1:].imag == -np.pi / n)
    assert K[0] == 1j * np.pi * (n - 1) / n
    # cot is odd about n/2: Re K[n-j] = -Re K[j] exactly in the table
    assert np.array_equal(K[1:].real, -K[1:][::-1].real)


@pytest.mark.parametrize("n,j", [(4097, 0), (4097, 4096), (4096, 1), (1000001, 999999)])
def test_delta_gives_kernel(n, j):
    K = ref.lag_kernel(n)
    S = np.zeros(n, dtype=np.complex128)
    S[j] = 1.0
    want = K[(np.arange(n) - j) % n]
    assert np.array_equal(ref.correction_sum(S, K), want)
    if n <= ref.SMALL:
        assert np.array_equal(ref.correction_matrix(S, K), want)


@pytest.mark.parametrize("n", [4097, 4096])
def test_correction_forms_agree_small(n):
    rng = np.random.default_rng(n)
    K = ref.lag_kernel(n)
    S = rng.normal(size=n) + 1j * rng.normal(size=n)
    S[: n // 3] = 0.0
    Cs, Cm, Cf = (ref.correction(S, form, K) for form in ("sum", "matrix", "fft"))
    tol = 1e-13 * np.max(np.abs(Cm))
    assert np.max(np.abs(Cs - Cm)) <= tol and np.max(np.abs(Cf - Cm)) <= tol


def test_correction_forms_agree_sparse_large():
    n = 1000001
    rng = np.random.default_rng(3)
    K = ref.lag_kernel(n)
    S = np.zeros(n, dtype=np.complex128)
    at = np.array([0, 1, n // 3, n // 2, n // 2 + 1, n - 2, n - 1])
    S[at] = rng.normal(size=len(at)) + 1j * rng.normal(size=len(at))
    Cs, Cf = ref.correction_sum(S, K), ref.correction_fft(S, K)
    assert np.max(np.abs(Cs - Cf)) <= 1e-13 * np.max(np.abs(Cs))


@pytest.mark.parametrize("n", [4097, 100001])
def test_windowed_matches_dft_form(n):
    import scipy.fft as sf
    from scipy.signal.windows import hann
    rng = np.random.default_rng(n)
    S = rng.normal(size=n) + 1j * rng.normal(size=n)
    S[: n // 3] = 0.0
    exact = sf.ifft(hann(n) * sf.fft(S))
    got = ref.windowed(S, ref.correction(S, "matrix" if n <= ref.SMALL else "fft"))
    err = np.max(np.abs(got - exact)) / np.max(np.abs(S))
    print(f"n={n}: err {err:.3e} = {err * n * n / 5:.3f} of 5/n^2")
    assert err <= 5.0 / n ** 2


@pytest.mark.parametrize("n,k0", [(101, 50), (1001, 500), (100, 50), (4097, 2048), (4096, 2048)])
def test_loglike_equals_local_layout_sum(n, k0):
    torch = pytest.importorskip("torch")
    from emri_frequencydomainwaveforms_amd.fdutils import HannConvolution
    rng = np.random.default_rng(n)
    nb = n - k0
    Sw = rng.normal(size=n) + 1j * rng.normal(size=n)
    d = rng.normal(size=(2, nb)) + 1j * rng.normal(size=(2, nb))
    w1 = rng.uniform(0.5, 2.0, size=nb)
    w1[0] = 0.0
    w = np.stack([w1, w1])
    dl, wl, kself = HannConvolution.local_layout(n, torch.as_tensor(d), torch.as_tensor(w), k0)
    dl, wl = dl.numpy(), wl.numpy()
    local = 0.5 * float(np.sum(np.abs(dl[:n] - wl * Sw) ** 2))
    if kself >= 0:
        local += 0.5 * float(abs(dl[n] - wl[kself] * Sw[kself]) ** 2)
    got = ref.loglike(Sw, d, w, k0)
    assert abs(got - (-2.0 * local)) <= 1e-12 * abs(got)
    assert np.array_equal(wl, ref.local_weight(n, w1, k0))
    # the emit definition's layout: element n repeats the self-mirror bin
    e = ref.local_data_ref(Sw, wl, kself)
    assert np.array_equal(e[:n], wl * Sw) and e[n] == (e[kself] if kself >= 0 else 0.0)
