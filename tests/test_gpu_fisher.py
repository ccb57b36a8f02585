"""efd_fisher_gram on the device: the C ABI against its CPU twin over the shapes at which the
kernel changes path (one element, around a wave, around the 256-element chunk, several workgroups;
1, 2, 3 and 4 tile rows of parameters; every stencil width), its reproducibility and subset
promises, and the Python surface (diagnostic.fisher / covariance, pe.fisher_covariance,
pe.setup(start_cov=...)) against lisatools' own results (tests/golden/fisher_golden.npz) and
against the likelihood kernel.

Tolerance of device against twin: 1e-12 sqrt(G_ii G_jj), the inner-product tolerance of
tests/test_gpu_likelihood.py (both sides form the same float64 terms; only the summation order
differs, ~sqrt(nelem) 1e-16 for the sizes here)."""

import ctypes

import numpy as np
import pytest

from tests import fisher_ref as fr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _dev(a):
    return None if a is None else torch.as_tensor(a, device="cuda")


def _p(t):
    if t is None:
        return None
    return ctypes.c_void_p((torch.view_as_real(t) if t.is_complex() else t).data_ptr())


def gram_gpu(rows, coef, w, want_dh=False, nelem=None, row_stride=None):
    """efd_fisher_gram through ctypes on device copies of host arrays (as fr.gram_cpu)."""
    from emri_frequencydomainwaveforms_amd import _lib
    lib = _lib.load()
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    P, npoint = coef.shape
    rows = np.ascontiguousarray(rows, dtype=np.complex128)
    row_stride = rows.shape[1] if row_stride is None else row_stride
    nelem = rows.shape[1] if nelem is None else nelem
    d_rows, d_w = _dev(rows), _dev(w)
    gram = torch.full((P, P), float("nan"), dtype=torch.float64, device="cuda")
    dh = torch.zeros((P, nelem), dtype=torch.complex128, device="cuda") if want_dh else None
    scr = torch.empty(_lib.EFD_FISHER_SCRATCH, dtype=torch.float64, device="cuda")
    rc = lib.efd_fisher_gram(_p(d_rows), row_stride, P, npoint, coef.ctypes.data, _p(d_w), nelem,
                             _p(dh), _p(gram), _p(scr), None)
    torch.cuda.synchronize()
    return rc, gram.cpu().numpy(), None if dh is None else dh.cpu().numpy()


def _random_case(nelem, nparam, npoint, seed=0, pad=0):
    rng = np.random.default_rng([seed, nelem, nparam, npoint])
    rows = rng.normal(size=(nparam * npoint, nelem + pad)) \
        + 1j * rng.normal(size=(nparam * npoint, nelem + pad))
    coef = rng.normal(size=(nparam, npoint))
    w = rng.uniform(0.5, 2.0, size=nelem)
    return rows, coef, w


@pytest.mark.parametrize("npoint", [1, 2, 4])
@pytest.mark.parametrize("nparam", [1, 2, 5, 16])
@pytest.mark.parametrize("nelem", [1, 63, 64, 65, 257, 8194])
def test_matches_cpu_twin(nelem, nparam, npoint):
    rows, coef, w = _random_case(nelem, nparam, npoint)
    rc, G, dh = gram_gpu(rows, coef, w, want_dh=True)
    rc2, Gc, dhc = fr.gram_cpu(rows, coef, w, want_dh=True)
    assert rc == 0 and rc2 == 0
    assert fr.rel(G, Gc) <= RTOL
    assert np.array_equal(G, G.T)
    assert np.array_equal(dh, dhc)   # the same stencil arithmetic per element on both sides
    rc, G0, _ = gram_gpu(rows, coef, w)             # dh = NULL: the same matrix
    assert rc == 0 and np.array_equal(G0, G)


@pytest.mark.parametrize("nelem,nparam,npoint", [(262401, 5, 2)])
def test_second_chunk_and_final_rounds(nelem, nparam, npoint):
    """262,401 = 1024 * 256 + 257 elements are 1026 chunks for 1024 workgroups: workgroups 0 and
    1 take a second chunk, the last chunk is partial, and the final pass adds 1024 partials, four
    rounds per thread."""
    test_matches_cpu_twin(nelem, nparam, npoint)


@pytest.mark.parametrize("nelem,nparam,npoint", [(257, 5, 2), (8194, 6, 4)])
def test_variants_match_cpu_twin(nelem, nparam, npoint):
    rows, coef, w = _random_case(nelem, nparam, npoint, seed=1, pad=3)
    # rows three elements apart from contiguous
    rc, G, dh = gram_gpu(rows, coef, w, want_dh=True, nelem=nelem, row_stride=nelem + 3)
    _, Gc, dhc = fr.gram_cpu(rows, coef, w, want_dh=True, nelem=nelem, row_stride=nelem + 3)
    assert rc == 0 and fr.rel(G, Gc) <= RTOL and np.array_equal(dh, dhc)
    tight = np.ascontiguousarray(rows[:, :nelem])
    assert np.array_equal(gram_gpu(tight, coef, w)[1], G)   # the stride changes nothing
    # w = NULL
    rc, G1, _ = gram_gpu(tight, coef, None)
    _, G1c, _ = fr.gram_cpu(tight, coef, None)
    assert rc == 0 and fr.rel(G1, G1c) <= RTOL
    # weights with zeros (masked bins)
    wz = w.copy()
    wz[::3] = 0.0
    wz[nelem // 2:nelem // 2 + 70] = 0.0
    rc, G2, _ = gram_gpu(tight, coef, wz)
    _, G2c, _ = fr.gram_cpu(tight, coef, wz)
    assert rc == 0 and fr.rel(G2, G2c) <= RTOL
    # rows with disjoint supports: parameter i lives on its own slice, so G is diagonal exactly
    dis = np.zeros_like(tight)
    edges = np.linspace(0, nelem, nparam + 1).astype(int)
    for i in range(nparam):
        dis[i * npoint:(i + 1) * npoint, edges[i]:edges[i + 1]] = \
            tight[i * npoint:(i + 1) * npoint, edges[i]:edges[i + 1]]
    rc, G3, _ = gram_gpu(dis, coef, w)
    _, G3c, _ = fr.gram_cpu(dis, coef, w)
    assert rc == 0
    assert np.array_equal(G3 - np.diag(np.diag(G3)), np.zeros_like(G3))
    assert np.all(np.abs(np.diag(G3) - np.diag(G3c)) <= RTOL * np.diag(G3c))


def test_bitwise_reproducible_and_subset_invariant():
    nelem, nparam, npoint = 8194, 5, 4
    rows, coef, w = _random_case(nelem, nparam, npoint, seed=2)
    rc, G, _ = gram_gpu(rows, coef, w)
    rc2, Gb, _ = gram_gpu(rows, coef, w)
    assert rc == 0 and rc2 == 0 and np.array_equal(G, Gb)
    blocks = [3, 1]
    sub = np.concatenate([rows[b * npoint:(b + 1) * npoint] for b in blocks])
    rc, Gs, _ = gram_gpu(sub, coef[blocks], w)
    assert rc == 0
    assert Gs[0, 0] == G[3, 3] and Gs[1, 1] == G[1, 1]
    assert Gs[0, 1] == G[3, 1] and Gs[1, 0] == G[3, 1]


def test_argument_errors_are_host_side():
    from emri_frequencydomainwaveforms_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    buf = ctypes.create_string_buffer(256)

    def call(h=fake, stride=8, nparam=2, npoint=2, coef=fake, nelem=8, gram=fake, scr=fake):
        rc = lib.efd_fisher_gram(h, stride, nparam, npoint, coef, None, nelem, None, gram, scr,
                                 None)
        lib.efd_last_error(buf, 256)
        return rc, buf.value

    for kw in (dict(nparam=0), dict(nparam=17), dict(npoint=3), dict(npoint=8), dict(h=None),
               dict(coef=None), dict(gram=None), dict(scr=None), dict(nelem=0),
               dict(stride=7)):
        rc, msg = call(**kw)
        assert rc == _lib.EFD_ERR_ARG and b"efd_fisher_gram" in msg, (kw, msg)


# ---- the lisatools surface on the fixture's toy model -------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = fr.golden()
    return g, fr.toy_model(g["f"])


@pytest.mark.parametrize("tag,scale,tol", [("base", 1.0, 1e-12), ("small", 1e-3, 1e-9)])
@pytest.mark.parametrize("accuracy", [True, False])
def test_diagnostic_fisher_matches_reference(gold, tag, scale, tol, accuracy):
    from emri_frequencydomainwaveforms_amd import diagnostic
    g, model = gold
    F = diagnostic.fisher(model, g["params"], g["eps"] * scale, accuracy=accuracy,
                          inner_product_kwargs=dict(f_arr=g["f"], PSD=g["psd"]))
    ref = g[f"fisher{'5' if accuracy else '3'}_{tag}"]
    assert isinstance(F, np.ndarray) and F.shape == (4, 4)
    assert fr.rel(F, ref) <= tol
    assert np.array_equal(F, F.T)


def test_diagnostic_fisher_derivs_list_model_and_positional_eps(gold):
    from emri_frequencydomainwaveforms_amd import diagnostic
    g, model = gold
    ipk = dict(f_arr=g["f"], PSD=g["psd"])
    F, dh = diagnostic.fisher(model, g["params"], g["eps"], inner_product_kwargs=ipk,
                              return_derivs=True)
    assert dh.is_cuda and tuple(dh.shape) == (4, 2, len(g["f"]))
    ref = g["dh5_base_row2"]
    assert np.abs(dh[2].cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    # a list of channels (what get_fd_waveform_fromFD returns) is stacked: the same matrix
    Fl = diagnostic.fisher(lambda *p: list(model(*p)), g["params"], g["eps"],
                           inner_product_kwargs=ipk)
    assert np.array_equal(Fl, F)
    # eps[k] goes with deriv_inds[k] by position, as the reference's zip
    Fs = diagnostic.fisher(model, g["params"], g["sub_eps"], deriv_inds=list(g["sub_inds"]),
                           inner_product_kwargs=ipk)
    assert fr.rel(Fs, g["fisher5_sub"]) <= 1e-12
    # the generic helper follows the reference's association too
    d2 = diagnostic.dh_dlambda(model, g["params"], g["eps"][2], 2)
    assert np.abs(d2.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


def test_covariance_of_supplied_fisher(gold):
    from emri_frequencydomainwaveforms_amd import diagnostic
    g, _ = gold
    C = diagnostic.covariance(fish=g["fisher5_base"])
    assert fr.rel(C, g["cov5_base"]) <= 1e-9
    C2, F2 = diagnostic.covariance(fish=g["fisher5_base"], return_fisher=True)
    assert np.array_equal(C2, C) and np.array_equal(F2, g["fisher5_base"])
    vals, vecs = diagnostic.get_eigens(C)
    # numpy's eig is backward stable: residuals are a few ulp of |C| (its condition is 4e11, so
    # nothing better holds element by element)
    assert np.abs(C @ vecs - vecs * vals).max() <= 1e-12 * np.linalg.norm(C, 2)


def _right_sum(f):
    x = np.empty_like(f)
    x[1:] = np.diff(f)
    x[0] = x[1]
    return x


def test_diagnostic_fisher_df_form_and_one_channel(gold):
    """A model returning one 1-D array with the df form of the frequencies,
    (arange(N) + 1) df (diagnostic.py:79-80): against the same sum in numpy."""
    from emri_frequencydomainwaveforms_amd import diagnostic
    g, model = gold
    n, df = 1500, 2e-6
    f = (np.arange(n) + 1) * df
    psd = g["psd"][:n]
    one = lambda *p: fr.toy_model(f)(*p)[1]
    eps = np.array([1e-3, 1e-3])   # for ln A and phi (by position)
    F, dh = diagnostic.fisher(one, g["params"], eps, deriv_inds=[0, 3], accuracy=False,
                              inner_product_kwargs=dict(df=df, PSD=psd), return_derivs=True)
    assert tuple(dh.shape) == (2, n)
    rows, coef = fr.stencil_rows(one, g["params"], eps, [0, 3], False)
    D = np.einsum("is,ise->ie", coef, rows.reshape(2, 2, n))
    ref = 4.0 * np.real(np.einsum("ie,je,e->ij", D.conj(), D, _right_sum(f) / psd))
    assert fr.rel(F, ref) <= 1e-12
    # (the stencil's terms are 500 |D| for ln A and each rounds at 1e-16: 1e-13 between two
    # associations of the same sum)
    assert np.abs(dh.cpu().numpy() - D).max() <= 1e-12 * np.abs(D).max()


def test_diagnostic_fisher_dt_form():
    """Time-domain rows (inner_product's dt form, diagnostic.py:57-73): each row's rfft * dt with
    the DC bin dropped feeds the kernel; the derivatives come back in the time domain.
    Tolerance: the transforms round at ~1e-15 of |h| and the differences keep >= 1e-3 of it
    (steps 1e-3 in the amplitude, 0.06 rad of phase at the end): 1e-12, asserted at 1e-10."""
    from emri_frequencydomainwaveforms_amd import diagnostic
    n, dt = 4096, 5.0
    t = np.arange(n) * dt
    model = lambda A, f0: A * np.sin(2 * np.pi * f0 * t) * np.exp(-0.5 * ((t - 1e4) / 4e3) ** 2)
    p, eps = np.array([1.0, 0.01]), np.array([1e-3, 1e-6])
    f = np.fft.rfftfreq(n, dt)[1:]
    psd = 1.0 + (1e-2 / f) ** 2
    F, dh = diagnostic.fisher(model, p, eps, inner_product_kwargs=dict(dt=dt, PSD=psd),
                              return_derivs=True)
    rows, coef = fr.stencil_rows(model, p, eps, [0, 1], True)
    D = np.einsum("is,ise->ie", coef, rows.real.reshape(2, 4, n))
    Df = np.fft.rfft(D, axis=-1)[:, 1:] * dt
    ref = 4.0 * np.real(np.einsum("ie,je,e->ij", Df.conj(), Df, _right_sum(f) / psd))
    assert fr.rel(F, ref) <= 1e-10
    assert tuple(dh.shape) == (2, n)
    assert np.abs(dh.cpu().numpy() - D).max() <= 1e-12 * np.abs(D).max()   # terms <= 1e3 |D|


def test_diagnostic_fisher_checks_device_memory(gold, monkeypatch):
    from emri_frequencydomainwaveforms_amd import diagnostic
    g, model = gold
    total = torch.cuda.mem_get_info()[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (0, total))
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda *a, **k: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda *a, **k: 0)
    need = 16 * (16 + 4) * 2 * len(g["f"])   # 16 stencil rows and 4 derivative rows
    with pytest.raises(ValueError, match=str(need)):
        diagnostic.fisher(model, g["params"], g["eps"], return_derivs=True,
                          inner_product_kwargs=dict(f_arr=g["f"], PSD=g["psd"]))


# ---- EMRI level -----------------------------------------------------------------------------
SETUP = dict(Tobs=0.05, dt=20.0, eps=1e-2, M=3e5, mu=10.0, e0=0.3, nwalkers=4, ntemps=1)


@pytest.fixture(scope="module")
def emri():
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(**SETUP)
    steps = np.where(s.truth6 != 0.0, 1e-6 * np.abs(s.truth6), 1e-6)
    F, cov, info = pe.fisher_covariance(s, steps, return_derivs=True)
    return s, steps, F, cov, info


def test_emri_batched_equals_generic_bitwise(emri):
    from emri_frequencydomainwaveforms_amd import pe
    s, steps, F, cov, info = emri
    Fg, covg, infog = pe.fisher_covariance(s, steps, return_derivs=True,
                                           waveform_model=lambda *a, **k: s.gen(*a, **k))
    assert np.array_equal(Fg, F)
    assert torch.equal(infog["derivs"], info["derivs"])


def test_emri_fisher_is_the_gram_of_its_derivatives(emri):
    s, steps, F, cov, info = emri
    D = info["derivs"].cpu().numpy().reshape(6, -1)
    f = np.asarray(s.f_like, dtype=np.float64)
    x = np.empty_like(f)
    x[1:] = np.diff(f)
    x[0] = x[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.array([x / np.asarray(p) for p in s.like.psd])
    # the bins the likelihood drops (f = 0, where its noise factor is NaN) carry no weight
    w = np.where(s.like._w.cpu().numpy() > 0.0, w, 0.0)
    ref = 4.0 * np.real(np.einsum("ie,je,e->ij", D.conj(), D, w.reshape(-1)))
    assert fr.rel(F, ref) <= 1e-12
    assert np.array_equal(F, F.T)
    d = np.sqrt(np.diag(F))
    assert np.linalg.eigvalsh(F / np.outer(d, d)).min() >= -1e-12
    assert np.isfinite(info["stencil_agreement"])
    assert cov.shape == (6, 6)


def test_emri_cross_kernel_identity_with_loglike(emri):
    """logL(h = h0; d = (h0 + sum_i delta_i D_i) wn, w = wn) = -1/2 delta^T F delta with
    delta_i = 1 / sqrt(F_ii) and wn = sqrt(x / PSD) (the likelihood's noise factor): the Gram
    kernel against efd_loglike. Both sides are float64; d - h w loses |h0| / |sum delta D|
    (the SNR over sqrt(delta^T F delta) / 2, < 1e3 here) times 1e-16: 1e-10 relative."""
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    s, steps, F, cov, info = emri
    delta = 1.0 / np.sqrt(np.diag(F))
    h0 = torch.stack(s.gen(*s.truth14, **s.kwargs)).contiguous()
    wn = s.like._w.contiguous()
    dd = (torch.as_tensor(delta, device=h0.device)[:, None, None] * info["derivs"]).sum(0)
    d = ((h0 + dd) * wn).contiguous()
    ll = Reducer(h0.device).loglike(h0, d, wn).item()
    want = -0.5 * delta @ F @ delta
    assert abs(ll - want) <= 1e-10 * abs(want)


def test_windowed_rows_batched_equals_generic():
    """A Hann-windowed model at the shortest grid that takes the batched window path
    (HannConvolution.applies: N >= 2,236,068): fisher_rows fills the stencil rows through
    fill_batch in groups of WINDOW_GROUP (5 parameters x 4 points: groups of 8, 8 and 4), the
    generic path through one __call__ per point. fill_batch promises its rows within 1e-12 of
    max|S| of the one-at-a-time fill (the batched transform's rounding; measured here: 0)."""
    from emri_frequencydomainwaveforms_amd import diagnostic as dg
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(Tobs=0.75, dt=10.0, eps=1e-2, nwalkers=4, ntemps=1, window_flag=True)
    assert s.gen.can_fill_batch
    steps6 = np.where(s.truth6 != 0.0, 1e-6 * np.abs(s.truth6), 1e-6)
    _, points, npoint = dg._fisher_points(s.truth6, steps6, [0, 1, 2, 3, 5],
                                          pe._SampledToWaveform(s.transform), True)
    assert dg._batched_model(s.gen, points, s.kwargs) is s.gen
    rb, _ = dg.fisher_rows(s.gen, points, s.kwargs)
    rg, _ = dg.fisher_rows(lambda *a, **k: s.gen(*a, **k), points, s.kwargs)
    assert tuple(rb.shape) == (20, 2, s.gen.num_bins) == tuple(rg.shape)
    err = float((rb - rg).abs().max()) / float(rg.abs().max())
    print(f"windowed rows, batched vs generic: {err:.3e} of max|h|")
    assert err <= 1e-12


def test_setup_start_cov(emri):
    from emri_frequencydomainwaveforms_amd import pe
    s, steps, F, cov, info = emri
    shipped = np.load(pe._COV, allow_pickle=False) / (2.4 * 6)
    want = np.random.default_rng(pe.SEED).multivariate_normal(s.truth6, shipped, size=4)
    assert np.array_equal(s.start, want)   # start_cov=None: the shipped matrix, as before
    C = np.diag((1e-3 * np.maximum(np.abs(s.truth6), 1.0)) ** 2)
    C[0, 1] = C[1, 0] = 0.3 * np.sqrt(C[0, 0] * C[1, 1])
    s2 = pe.setup(start_cov=C, **SETUP)
    want2 = np.random.default_rng(pe.SEED).multivariate_normal(s.truth6, C / (2.4 * 6), size=4)
    assert np.array_equal(s2.start, want2)
    with pytest.raises(ValueError):
        pe.setup(start_cov=np.eye(5), **SETUP)
