"""efd_overlap_rows_cpu (the host twin of efd_overlap_rows) against numpy, its exact zeros and
argument errors, and the fixture's quantities (tests/golden/overlap_golden.npz, lisatools' own
mismatch_criterion / vallisneri_criterion_cdf / cutler_vallisneri_bias results) rebuilt from the
stored offsets with the toy model in numpy and the twin. Runs without a GPU.

Tolerance of twin against numpy: 1e-12 sqrt(nn_k rr) on the cross terms, the project's
inner-product tolerance (both sides form the same float64 terms; only the summation order
differs). Against the fixture: over / mism 1e-11 absolute, ratio / r_at_90 1e-11 relative,
syst_vec[k] 1e-11 sqrt(F_kk |dh|^2), bias 1e-9 sqrt(cov_kk); a plain numpy evaluation lies
3e-15, 6e-15, 1e-14, 1e-15 and 3e-17 from the reference (make_golden_overlap.py's print)."""

import ctypes

import numpy as np
import pytest

from tests import overlap_ref as orf

RTOL = 1e-12
random_case = orf.random_case


@pytest.mark.parametrize("with_u", [True, False])
@pytest.mark.parametrize("nrow", [1, 9, 64])
@pytest.mark.parametrize("nelem", [1, 63, 257, 8194])
def test_twin_matches_numpy(nelem, nrow, with_u):
    rows, t, u, w = random_case(nelem, nrow)
    u = u if with_u else None
    rc, out = orf.overlap_cpu(rows, t, u, w)
    ref = orf.overlap_numpy(rows, t, u, w)
    assert rc == 0
    assert orf.cross_err(out, ref) <= RTOL
    assert orf.norm_err(out, ref) <= RTOL


@pytest.mark.parametrize("nelem,nrow", [(257, 9), (8194, 5)])
def test_twin_variants(nelem, nrow):
    rows, t, u, w = random_case(nelem, nrow, seed=1, pad=3)
    tight = np.ascontiguousarray(rows[:, :nelem])
    rc, out = orf.overlap_cpu(rows, t, u, w, nelem=nelem, row_stride=nelem + 3)
    ref = orf.overlap_numpy(tight, t, u, w)
    assert rc == 0 and orf.cross_err(out, ref) <= RTOL and orf.norm_err(out, ref) <= RTOL
    assert np.array_equal(orf.overlap_cpu(tight, t, u, w)[1], out)   # the stride changes nothing
    rc, o1 = orf.overlap_cpu(tight, t, u, None)                      # w = NULL
    r1 = orf.overlap_numpy(tight, t, u, None)
    assert rc == 0 and orf.cross_err(o1, r1) <= RTOL and orf.norm_err(o1, r1) <= RTOL
    wz = w.copy()                                                     # masked bins
    wz[::3] = 0.0
    wz[nelem // 2:nelem // 2 + 70] = 0.0
    rc, o2 = orf.overlap_cpu(tight, t, u, wz)
    r2 = orf.overlap_numpy(tight, t, u, wz)
    assert rc == 0 and orf.cross_err(o2, r2) <= RTOL and orf.norm_err(o2, r2) <= RTOL
    # a row's numbers do not depend on the other rows
    rc, o3 = orf.overlap_cpu(tight[2:3], t, u, w)
    assert rc == 0 and np.array_equal(o3[:3], out[6:9]) and o3[3] == out[-1]


def test_twin_exact_zeros():
    nelem, nrow = 8194, 9
    rows, t, u, w = random_case(nelem, nrow, seed=2)
    rc, out = orf.overlap_cpu(rows, t, t.copy(), w)     # u == t bit for bit: r = 0
    assert rc == 0
    assert np.all(out[0:-1:3] == 0.0) and np.all(out[1:-1:3] == 0.0) and out[-1] == 0.0
    assert np.all(out[2:-1:3] > 0.0)
    # rows on the first half, r on the second: disjoint supports
    dis = rows.copy()
    dis[:, nelem // 2:] = 0.0
    t2, u2 = t.copy(), u.copy()
    t2[:nelem // 2] = u2[:nelem // 2] = 0.0
    for uu in (u2, None):
        rc, out = orf.overlap_cpu(dis, t2, uu, w)
        assert rc == 0
        assert np.all(out[0:-1:3] == 0.0) and np.all(out[1:-1:3] == 0.0)
        assert np.all(out[2:-1:3] > 0.0) and out[-1] > 0.0


def test_twin_argument_errors():
    from emri_frequencydomainwaveforms_amd import _lib
    lib = _lib.load()
    a = np.zeros(64, dtype=np.complex128)
    p = a.ctypes.data_as(ctypes.c_void_p)
    buf = ctypes.create_string_buffer(256)

    def call(h=p, stride=8, nrow=2, t=p, nelem=8, out=p):
        rc = lib.efd_overlap_rows_cpu(h, stride, nrow, t, None, None, nelem, out, None, None)
        lib.efd_cpu_last_error(buf, 256)
        return rc, buf.value

    assert call()[0] == 0
    for kw in (dict(nrow=0), dict(nrow=65), dict(h=None), dict(t=None), dict(out=None),
               dict(nelem=0), dict(nelem=-1), dict(stride=7)):
        rc, msg = call(**kw)
        assert rc == _lib.EFD_ERR_ARG and b"efd_overlap_rows_cpu" in msg, (kw, msg)


# ---- the fixture's quantities from the stored offsets, the toy model and the twin -----------
@pytest.fixture(scope="module")
def gold():
    g = orf.golden()
    f, psd = g["f"], g["psd"]
    T = orf.ToyTransform()
    model = orf.toy_model(f)
    pts, refl = orf.perturbed_points(g["params"], g["offsets"], T)
    h_true = model(*T.transform_base_parameters(g["params"]))
    return g, model, T, pts, refl, h_true, orf.weights(f, psd, 2)


def test_fixture_criterion_through_twin(gold):
    g, model, T, pts, refl, h_true, w = gold
    assert np.array_equal(refl, g["reflected"]) and refl.any() and not refl.all()
    rows = np.array([model(*q) for q in pts]).reshape(len(pts), -1)
    rc, res = orf.overlap_cpu(rows, h_true.reshape(-1), None, w)
    assert rc == 0
    over, mism, ratio = orf.criterion(res, g["offsets"], g["fisher"])
    assert np.abs(mism - g["mism"]).max() <= 1e-11
    assert np.abs(over - (1 - 2 * g["mism"])).max() <= 1e-11
    assert np.abs(ratio / g["ratio"] - 1).max() <= 1e-11
    ratios = np.abs(np.log(ratio))
    q, counts = np.unique(ratios, return_counts=True)
    r90 = np.interp(0.9, np.cumsum(counts).astype(np.double) / ratios.size, q)
    assert abs(r90 / g["r_at_90"] - 1) <= 1e-11


def test_fixture_bias_through_twin(gold):
    g, model, T, pts, refl, h_true, w = gold
    from tests import fisher_ref as fr
    p, eps = g["params"], g["eps"]
    both = lambda *x: model(*T.transform_base_parameters(np.array(x)))
    rows, coef = fr.stencil_rows(both, p, eps, range(5), True)
    rc, F, dh = fr.gram_cpu(rows, coef, w, want_dh=True)
    assert rc == 0 and fr.rel(F, g["fisher"]) <= 1e-12
    h_approx = orf.toy_model(g["f"], orf.APPROX_SCALE)(*T.transform_base_parameters(p))
    rc, res = orf.overlap_cpu(dh, h_true.reshape(-1), h_approx.reshape(-1), w)
    assert rc == 0
    syst = res[0:-1:3]
    assert np.all(np.abs(syst - g["syst_vec"]) <= 1e-11 * np.sqrt(np.diag(g["fisher"]) * res[-1]))
    bias = g["cov"] @ syst
    assert np.all(np.abs(bias - g["bias"]) <= 1e-9 * np.sqrt(np.diag(g["cov"])))
