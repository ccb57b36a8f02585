"""efd_fisher_gram_cpu against lisatools' fisher on the toy model of tests/golden/fisher_golden.npz
(made by tests/golden/make_golden_fisher.py with the reference's own code). Runs without a GPU.

Tolerances, normalised by sqrt(F_ii F_jj): 1e-12 at the base steps (the inner-product tolerance of
tests/test_gpu_likelihood.py; forming the stencil per bin in float64 numpy is 7.5e-15 from the
reference), 1e-9 at steps 1e-3 times smaller (per bin: 1.2e-11; the Gram matrix of the raw stencil
spectra combined afterwards is >= 4.4e-2 off there, and 2e-8 at the base steps: that shortcut
fails both bounds)."""

import ctypes

import numpy as np
import pytest

from tests import fisher_ref as fr
from emri_frequencydomainwaveforms_amd import _lib


@pytest.fixture(scope="module")
def gold():
    g = fr.golden()
    return g, fr.toy_model(g["f"]), fr.weights(g["f"], g["psd"], 2)


@pytest.mark.parametrize("tag,scale,tol", [("base", 1.0, 1e-12), ("small", 1e-3, 1e-9)])
@pytest.mark.parametrize("accuracy", [True, False])
def test_matches_reference_fisher(gold, tag, scale, tol, accuracy):
    g, model, w = gold
    rows, coef = fr.stencil_rows(model, g["params"], g["eps"] * scale, range(4), accuracy)
    rc, F, _ = fr.gram_cpu(rows, coef, w)
    assert rc == 0
    ref = g[f"fisher{'5' if accuracy else '3'}_{tag}"]
    err = fr.rel(F, ref)
    print(f"{tag} accuracy={accuracy}: {err:.3e}")
    assert err <= tol
    assert np.array_equal(F, F.T)


def test_positional_eps_subset(gold):
    g, model, w = gold
    rows, coef = fr.stencil_rows(model, g["params"], g["sub_eps"], g["sub_inds"], True)
    rc, F, _ = fr.gram_cpu(rows, coef, w)
    assert rc == 0
    assert fr.rel(F, g["fisher5_sub"]) <= 1e-12


def test_derivative_row(gold):
    g, model, w = gold
    rows, coef = fr.stencil_rows(model, g["params"], g["eps"], range(4), True)
    rc, _, dh = fr.gram_cpu(rows, coef, w, want_dh=True)
    assert rc == 0
    ref = g["dh5_base_row2"].reshape(-1)
    assert np.abs(dh[2] - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("use_w", [True, False])
def test_single_point_is_the_inner_product(gold, use_w):
    g, model, w = gold
    lib = _lib.load()
    rng = np.random.default_rng(7)
    n = 2 * len(g["f"])
    rows = rng.normal(size=(3, n)) + 1j * rng.normal(size=(3, n))
    ww = w if use_w else None
    rc, G, _ = fr.gram_cpu(rows, np.ones((3, 1)), ww)
    assert rc == 0
    out = np.zeros(2)
    for i in range(3):
        for j in range(3):
            a, b = np.ascontiguousarray(rows[i]), np.ascontiguousarray(rows[j])
            assert lib.efd_inner_product_cpu(fr._ptr(a), fr._ptr(b), fr._ptr(ww), 2, n // 2,
                                             fr._ptr(out), None, None) == 0
            assert abs(G[i, j] - out[0]) <= 1e-13 * np.sqrt(G[i, i] * G[j, j])


def test_strided_rows_and_thread_count(gold):
    g, model, w = gold
    rng = np.random.default_rng(11)
    n = 8194
    wide = rng.normal(size=(10, n + 3)) + 1j * rng.normal(size=(10, n + 3))
    coef = rng.normal(size=(5, 2))
    ww = rng.uniform(size=n)
    rc, G, dh = fr.gram_cpu(wide, coef, ww, want_dh=True, nelem=n, row_stride=n + 3)
    assert rc == 0
    D = np.einsum("is,ise->ie", coef, wide[:, :n].reshape(5, 2, n))
    ref = 4.0 * np.real(np.einsum("ie,je,e->ij", D.conj(), D, ww))
    assert fr.rel(G, ref) <= 1e-12
    assert np.abs(dh - D).max() <= 1e-14 * np.abs(D).max()
    lib = _lib.load()
    prev = lib.efd_cpu_threads(1)
    try:
        rc, G1, _ = fr.gram_cpu(wide, coef, ww, nelem=n, row_stride=n + 3)
    finally:
        lib.efd_cpu_threads(prev)
    assert rc == 0 and np.array_equal(G1, G)


def test_argument_errors():
    lib = _lib.load()
    fake = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    buf = ctypes.create_string_buffer(256)

    def call(h=fake, stride=8, nparam=2, npoint=2, coef=fake, nelem=8, gram=fake):
        rc = lib.efd_fisher_gram_cpu(h, stride, nparam, npoint, coef, None, nelem, None, gram,
                                     None, None)
        lib.efd_cpu_last_error(buf, 256)
        return rc, buf.value

    for kw in (dict(nparam=0), dict(nparam=17), dict(npoint=3), dict(npoint=0), dict(h=None),
               dict(coef=None), dict(gram=None), dict(nelem=0), dict(nelem=-1),
               dict(stride=7)):
        rc, msg = call(**kw)
        assert rc == _lib.EFD_ERR_ARG and b"efd_fisher_gram_cpu" in msg, (kw, msg)
