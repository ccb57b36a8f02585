"""efd_hann_loglike_local (the fused windowed logL, k_fc_cols_ll<R, C>) against a float64
evaluation of what it is defined to compute (tests/hann_local_ref.py, itself held to closed forms
in tests/test_hann_local_ref.py), on every four-step split: m = 2^21, 2^22, 2^23, 2^25 as R x 8192
(R = 256, 512, 1024, 4096) and 2^24 as 1024 x 16384. HannConvolution.local_data, local_emit and
loglike_local are driven as the likelihood drives them; `support=` chooses m (size_for), so any
split runs at any grid length.

Checks, every row of every case (no sampling of bins, no skips):

  emit    every one of the n + 1 emitted elements against wl[k] S_w[k] of the reference, within
            e_bin[k] = wl[k] (2 * 1e-5 max|C_ref| / (4 (n-1)) + 8 * 2^-53 max|S|):
          the complex64 correction's contract (1e-5 of max|C|, test_four_step_convolution) once
          for each of the two differenced neighbours, plus the float64 stencil's rounding. The
          wrapped element u = nf-1 (kfix), the mirror layout and e[n] == e[kself] are inside it.
  logL    against the reference's mirror-pair logL on h+, hx (not the dl / wl layout), for random
          data of the template's magnitude and for near-truth data d = w h_ref (1 + 1e-6 xi),
          both with a masked bin w[0] = 0:
            |logL - logL_ref| <= 4 ||r|| E + 2 E^2 + 64 * 2^-53 |logL_ref|,
          r the reference residual, E^2 = sum e_bin^2 over the grid (kself twice): a bound from
          the per-bin contract above, not from a measured distance.
  zero    the emitted data fed back at the same m gives logL == 0.0 exactly.

Cases: (a) grids of 4097 (odd, kself = 2048) and 4096 bins (even, no kself, nf divides m so
kfix = 0) on all five m, where nearly every element of the launch has u < 0: dense rows (whole
grid; [n/3, n) with |S[first]| the row's maximum, the largest kfix term), single bins at 0, n-1
and kself, bins 0 and n-1 only, all zero; scales 1 and 1e-21. (b) grids just under m/2 for each
m with sparse rows (<= 8 bins at 0, 1, first, kself, kself+-1, n-2, n-1; one support the whole
grid, one strictly inside; those two alone at the two largest n), and dense rows at n = 1,000,001 on m = 2^21 and, forced, 2^22.
(c) 1, 2, 3, 5 and 16 rows a call: each row within the bound and bitwise equal to the row alone.
(e) the defined NaN of an aliased support (len > m - nf) and of a row holding a NaN, the rows
beside them bitwise unchanged. (f) data emitted at m = 2^21 evaluated at m = 2^22: finite and
|logL| <= 2 (2 E)^2 (two float corrections differ by at most 2 e_bin a bin).

(g) S is read only inside the extent: values outside the scanned lane range change no bit.

Measured on an MI355X, worst err / bound over the cases of each m (every test prints its figures
before it asserts); the true float error sits a decade under the contract, nothing above 0.5:

    m       emit, per element   logL
    2^21    0.091               0.062
    2^22    0.102               0.062
    2^23    0.090               0.055
    2^24    0.104               0.055
    2^25    0.097               0.055

The tiny grids give the largest figures of both columns (emit 0.10 and logL 0.06 on
4097 bins); the sparse rows near m/2 reach 0.06-0.08 in emit and 1e-5..1e-3 in logL, the
dense rows 0.09-0.10 and 4e-4.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib  # noqa: E402
from emri_frequencydomainwaveforms_amd.fdutils import HannConvolution  # noqa: E402
from tests import hann_local_ref as ref  # noqa: E402

U = 2.0 ** -53
SPLITS = [1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25]


@functools.lru_cache(maxsize=2)
def _kernel(n):
    return ref.lag_kernel(n)


def _lag(n):
    # (the large grids' tables are 0.1-0.5 GB: used once, not kept)
    return _kernel(n) if n <= 2100000 else ref.lag_kernel(n)


def _crandn(rng, size):
    return rng.normal(size=size) + 1j * rng.normal(size=size)


class Grid:
    """One grid length n on one transform length m: the weights, the device objects and the
    checks of the module docstring."""

    def __init__(self, n, m, support, seed=0):
        self.n, self.m, self.support = n, m, support
        self.k0 = k0 = n // 2
        self.nb = nb = n - k0
        self.kself = k0 if n % 2 else -1
        self.rng = rng = np.random.default_rng(1000 + seed)
        w1 = rng.uniform(0.5, 2.0, size=nb)
        w1[0] = 0.0                                  # a masked bin (the likelihood's start_ind)
        self.w = np.stack([w1, w1])
        self.wl = ref.local_weight(n, w1, k0)
        self.lib = _lib.load()
        self.hcv = HannConvolution(n, torch.device("cuda", torch.cuda.current_device()))
        assert self.hcv.size_for(n, support) == m and self.hcv._four(m)
        assert self.lib.efd_hann_loglike_local_partials(m) <= _lib.EFD_HANN_LOCAL_PARTIALS
        self.w_t = torch.as_tensor(self.w, device="cuda")
        zero = torch.zeros((2, nb), dtype=torch.complex128, device="cuda")
        assert self.hcv.local_ok(zero, self.w_t, k0)
        _, self.wl_t, ks = self.hcv.local_data(zero, self.w_t, k0)
        assert ks == self.kself and np.array_equal(self.wl_t.cpu().numpy(), self.wl)
        self.scr = torch.empty(_lib.EFD_HANN_ROWS_MAX * _lib.EFD_HANN_LOCAL_PARTIALS,
                               dtype=torch.float64, device="cuda")
        self.worst = [0.0, 0.0]

    # -- the bound's pieces ---------------------------------------------------------------
    def e_bin(self, S, C):
        """e_bin over the n + 1 emitted elements, from the reference's C and S of one row."""
        n = self.n
        c = 2.0 * 1e-5 * float(np.max(np.abs(C))) / (4.0 * (n - 1)) + 8.0 * U * float(
            np.max(np.abs(S)))
        e = np.empty(n + 1)
        e[:n] = self.wl * c
        e[n] = e[self.kself] if self.kself >= 0 else 0.0
        return e

    # -- the device calls -----------------------------------------------------------------
    def rows(self, S):
        return torch.as_tensor(np.ascontiguousarray(S), device="cuda")

    def logl(self, St, d):
        """The rows' logL against d ([2][nb], numpy or tensor) through local_data."""
        d_t = torch.as_tensor(d, device="cuda")
        local = self.hcv.local_data(d_t, self.w_t, self.k0)
        return self.logl_local(St, local)

    def logl_local(self, St, local):
        out = torch.full((St.shape[0],), 7.0, dtype=torch.float64, device="cuda")
        assert self.hcv.loglike_local(St, local, out, self.scr, self.lib, support=self.support)
        return out.cpu().numpy()

    def emit(self, St_row):
        return self.hcv.local_emit(St_row, self.wl_t, self.kself, self.lib, support=self.support)

    # -- the checks -----------------------------------------------------------------------
    def check_emit(self, St_row, Sw, eb, tag):
        n, ks = self.n, self.kself
        e_t = self.emit(St_row)
        one = self.logl_local(St_row, (e_t, self.wl_t, ks))
        e = e_t.cpu().numpy()
        err = np.abs(e - ref.local_data_ref(Sw, self.wl, ks))
        pos = eb > 0
        ratio = float(np.max(err[pos] / eb[pos])) if pos.any() else 0.0
        worst = int(np.argmax(err - eb))
        print(f"{tag} emit: max err/e_bin {ratio:.3e}")
        self.worst[0] = max(self.worst[0], ratio)
        assert np.all(err <= eb), (tag, worst, err[worst], eb[worst])
        if ks >= 0:
            assert e[n] == e[ks]
        assert one[0] == 0.0, (tag, one)             # the emitted data fed back: exact zero
        return e_t

    def logl_bound(self, Sw, eb, d):
        r = ref.residual(Sw, d, self.w, self.k0)
        rn2 = float(np.sum(r.real ** 2 + r.imag ** 2))
        ll = -2.0 * rn2
        E2 = float(np.sum(eb ** 2))                  # element n: kself a second time
        return ll, 4.0 * np.sqrt(rn2 * E2) + 2.0 * E2 + 64.0 * U * abs(ll)

    def check_logl(self, got, Sw, eb, d, tag):
        ll, bound = self.logl_bound(Sw, eb, d)
        err = abs(got - ll)
        ratio = err / bound if bound > 0 else 0.0
        print(f"{tag} logL {got:.17g} ref {ll:.17g} err/bound {ratio:.3e}")
        self.worst[1] = max(self.worst[1], ratio)
        assert np.isfinite(got) and err <= bound, (tag, got, ll, err, bound)

    def data_sets(self, S, Sw):
        """(random data of the row's magnitude, near-truth data of the reference's own h)."""
        rng, nb = self.rng, self.nb
        mag = float(np.max(np.abs(S))) or 1.0
        xi = _crandn(rng, (2, nb))                   # (one draw serves both: they are never mixed)
        d_rand = xi * mag
        d_near = self.w * ref.polarizations(Sw, self.k0) * (1.0 + 1e-6 * xi)
        return (("rand", d_rand), ("near", d_near))

    def check_rows(self, S, Sw, Cs, tag, all_rows=False):
        """Every row's emit, feedback and logL (both data sets; the whole batch in the call,
        row r held to its own data, or with all_rows every row to every data set)."""
        St = self.rows(S)
        ebs = [self.e_bin(S[r], Cs[r]) for r in range(len(S))]
        for r in range(len(S)):
            self.check_emit(St[r:r + 1].contiguous(), Sw[r], ebs[r], f"{tag} row {r}")
            for name, d in self.data_sets(S[r], Sw[r]):
                got = self.logl(St, d)
                for q in (range(len(S)) if all_rows else [r]):
                    self.check_logl(got[q], Sw[q], ebs[q], d, f"{tag} row {q} data {name}{r}")
        print(f"{tag} m=2^{self.m.bit_length() - 1} WORST emit {self.worst[0]:.3e} "
              f"logL {self.worst[1]:.3e}")


def _reference(S, n, form=None):
    """(S_w, C) of each row of S."""
    K = _lag(n)
    Cs = [ref.correction(S[r], form, K) for r in range(len(S))]
    del K
    return np.stack([ref.windowed(S[r], Cs[r]) for r in range(len(S))]), Cs


# ---- (a) tiny grids on every split ------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _tiny(n):
    rng = np.random.default_rng(n)
    ks = n // 2
    S = np.zeros((7, n), dtype=np.complex128)
    S[0] = _crandn(rng, n)                                   # dense over the whole grid
    S[1, n // 3:] = _crandn(rng, n - n // 3)                 # dense on [n/3, n): wraps
    S[1, n // 3] *= 4.0 * np.max(np.abs(S[1])) / abs(S[1, n // 3])
    assert np.argmax(np.abs(S[1])) == n // 3
    S[2, 0] = 0.7 - 0.3j                                     # single bins
    S[3, n - 1] = -0.4 + 0.9j
    S[4, ks] = 0.6 + 0.5j                                    # kself on the odd grid
    S[5, 0], S[5, n - 1] = 0.8 + 0.1j, -0.2 - 0.9j           # bins 0 and n-1 only
    S[[1, 3, 5]] *= 1e-21
    K = _kernel(n)
    C = ref.correction_matrix(S, K)                          # the direct product
    Sw = np.stack([ref.windowed(S[r], C[r]) for r in range(7)])
    return S, Sw, list(C)


@pytest.mark.parametrize("m", SPLITS)
@pytest.mark.parametrize("n", [4097, 4096])
def test_tiny_grids(n, m):
    S, Sw, Cs = _tiny(n)
    g = Grid(n, m, m // 2, seed=n)
    assert (g.kself, g.k0) == ((2048, 2048) if n == 4097 else (-1, 2048))
    g.check_rows(S, Sw, Cs, f"tiny n={n}", all_rows=True)
    # the all-zero row: the data-only term, within the last summand (E = 0 in its bound)
    assert np.all(Sw[6] == 0)


# ---- (b) grids just under m / 2 -----------------------------------------------------------------
SCALES = np.array([1e-21, 1.0, 1e-21, 1e-21])


def _sparse_rows(n, count=4):
    """Sparse rows: the whole grid, strictly inside, touching bin 0, touching n-1."""
    rng = np.random.default_rng(n % 9973)
    ks, first = n // 2, n // 3
    sets = [[0, 1, first, ks - 1, ks, ks + 1, n - 2, n - 1],
            [first, first + 1, ks - 1, ks, ks + 1, n - 3, n - 2],
            [0, 1, first, ks],
            [first, ks + 1, n - 2, n - 1]]
    S = np.zeros((count, n), dtype=np.complex128)
    for r, at in enumerate(sets[:count]):
        S[r, at] = _crandn(rng, len(at)) * SCALES[r]
    return S


@functools.lru_cache(maxsize=1)
def _sparse_1m():
    n = 1000001
    S = _sparse_rows(n)
    Sw, Cs = _reference(S, n, "sum")
    return S, Sw, Cs


@pytest.mark.parametrize("n,m", [(1000001, 1 << 21), (2000001, 1 << 22), (4000001, 1 << 23),
                                 (8000001, 1 << 24), (16000001, 1 << 25)])
def test_sparse_rows_near_half(n, m):
    if n == 1000001:
        S, Sw, Cs = _sparse_1m()
    else:
        # two rows a call at the two largest n (memory, and ~6 s of reference a row at 16 M
        # bins): the whole-grid row and the one strictly inside
        S = _sparse_rows(n, 2 if n > 4000001 else 4)
        Sw, Cs = _reference(S, n, "sum")
    g = Grid(n, m, n, seed=m.bit_length())           # support: the whole grid (row 0's)
    g.check_rows(S, Sw, Cs, f"sparse n={n}")


@pytest.mark.parametrize("m,support", [(1 << 21, 1000001), (1 << 22, 1200000)])
def test_dense_rows(m, support):
    n = 1000001
    rng = np.random.default_rng(m.bit_length())
    S = np.zeros((2, n), dtype=np.complex128)
    lo, hi = int(0.45 * n), int(0.55 * n)
    S[0, lo:hi] = _crandn(rng, hi - lo) * 1e-21
    S[1] = _crandn(rng, n)
    Sw, Cs = _reference(S, n, "fft")
    Grid(n, m, support, seed=m.bit_length()).check_rows(S, Sw, Cs, "dense n=1000001")


# ---- (c) row mapping --------------------------------------------------------------------------
def test_row_mapping():
    n, m = 1000001, 1 << 21
    S4, Sw4, C4 = _sparse_1m()
    # rows of one magnitude (one data set for the call): the unit row times 2^-70, the all-zero
    # row fifth, and the next five a power of two down (exact in the reference)
    f4 = np.array([1.0, 2.0 ** -70, 1.0, 1.0])
    base = np.concatenate([S4 * f4[:, None], np.zeros((1, n), dtype=np.complex128)])
    base_w = np.concatenate([Sw4 * f4[:, None], np.zeros((1, n), dtype=np.complex128)])
    base_c = [float(np.max(np.abs(C4[r]))) * f4[r] for r in range(4)] + [0.0]
    S = np.stack([base[r % 5] * 2.0 ** -(r // 5) for r in range(16)])
    g = Grid(n, m, n, seed=77)
    d = _crandn(g.rng, (2, g.nb)) * 1e-21
    St = g.rows(S)
    alone = np.concatenate([g.logl(St[r:r + 1].contiguous(), d) for r in range(16)])
    for r in range(16):
        f = 2.0 ** -(r // 5)
        eb = g.e_bin(S[r], np.array([base_c[r % 5] * f]))
        g.check_logl(alone[r], base_w[r % 5] * f, eb, d, f"rows alone {r}")
    for count in (1, 2, 3, 5, 16):
        got = g.logl(St[:count].contiguous(), d)
        assert got.tobytes() == alone[:count].tobytes(), (count, got, alone[:count])
    print(f"rows m=2^21 WORST logL {g.worst[1]:.3e}")


# ---- (e) defined non-finite results -------------------------------------------------------------
def test_aliased_support_is_nan():
    n, m, support = 1100001, 1 << 21, 900000
    S = np.zeros((2, n), dtype=np.complex128)
    S[0, [0, 1, n // 2, n - 1]] = np.array([1 + 2j, -2 + 1j, 0.5j, 3.0]) * 1e-21   # len n > m - n
    S[1, [n // 10, n // 10 + 7, n // 10 + 900000 - 1]] = np.array([1 - 1j, 2j, -1.5]) * 1e-21
    g = Grid(n, m, support, seed=5)
    assert n > m - n >= 900000
    d = _crandn(g.rng, (2, g.nb)) * 1e-21
    St = g.rows(S)
    both = g.logl(St, d)
    fits = g.logl(St[1:2].contiguous(), d)
    assert np.isnan(both[0]) and np.isfinite(both[1])
    assert both[1:].tobytes() == fits.tobytes()
    Sw, Cs = _reference(S[1:2], n, "sum")
    g.check_logl(fits[0], Sw[0], g.e_bin(S[1], Cs[0]), d, "beside the aliased row")


def test_nan_row_beside_good_rows():
    n, m = 1000001, 1 << 21
    S4, Sw4, C4 = _sparse_1m()
    S = S4[[0, 2, 3]].copy()
    S[1, n // 3] = complex(np.nan, 1e-21)
    g = Grid(n, m, n, seed=6)
    d = _crandn(g.rng, (2, g.nb)) * 1e-21
    St = g.rows(S)
    got = g.logl(St, d)
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))
    for r, q in ((0, 0), (2, 3)):
        assert g.logl(St[r:r + 1].contiguous(), d).tobytes() == got[r:r + 1].tobytes()
        g.check_logl(got[r], Sw4[q], g.e_bin(S4[q], C4[q]), d, f"beside the NaN row {r}")


# ---- (f) emit at one transform length, evaluate at another ---------------------------------------
def test_emit_at_one_length_evaluate_at_another():
    """The injection's data emitted at m = 2^21 (its own support's length) against the same row
    evaluated at m = 2^22 (a walker batch with a longer support): finite, and within 2 (2 E)^2.
    Measured: logL = -9.0e-62 beside sum |dl|^2 = 1.3e-37 (7e-25 of it), 9.2e-7 of the bound
    9.9e-56: the zero is exact only at equal transform lengths."""
    n = 1000001
    rng = np.random.default_rng(21)
    S = np.zeros((1, n), dtype=np.complex128)
    lo, hi = int(0.45 * n), int(0.55 * n)
    S[0, lo:hi] = _crandn(rng, hi - lo) * 1e-21
    C = ref.correction_fft(S[0], _lag(n))
    g21 = Grid(n, 1 << 21, hi - lo, seed=8)
    g22 = Grid(n, 1 << 22, 1200000, seed=8)          # the same weights (same seed)
    assert np.array_equal(g21.wl, g22.wl)
    St = g21.rows(S)
    e_t = g21.emit(St)
    same = g21.logl_local(St, (e_t, g21.wl_t, g21.kself))[0]
    other = g22.logl_local(St, (e_t, g22.wl_t, g22.kself))[0]
    E2 = float(np.sum(g21.e_bin(S[0], C) ** 2))
    print(f"cross: logL at 2^21 {same!r}, at 2^22 {other!r}, bound {8.0 * E2:.3e}, "
          f"ratio {abs(other) / (8.0 * E2):.3e}, sum |dl|^2 {float((e_t.abs() ** 2).sum()):.3e}")
    assert same == 0.0
    assert np.isfinite(other) and abs(other) <= 2.0 * 4.0 * E2


# ---- (g) reads of S stay inside the extent -------------------------------------------------------
def test_bins_outside_the_lane_range_are_not_read():
    """The kernel reads S only inside the row's support (the stencil's three masks u, u+1, u-1
    < len). With a lane range the extent scan sees [k_lo, k_hi) alone, so values left in the
    buffer next to it on either side (k_lo - 1 and k_hi, where the stencil's neighbours of the
    first and the last bin look) must change no bit of the logL or of the emitted data, and the
    result is the reference's for the clean row."""
    n, m = 1000001, 1 << 21
    k_lo, k_hi = n // 3, n - n // 3
    S = np.zeros((1, n), dtype=np.complex128)
    S[0, [k_lo, k_lo + 1, n // 2, k_hi - 2, k_hi - 1]] = np.array(
        [1 - 2j, 0.5j, -1.5 + 1j, 2.0, -1 - 1j]) * 1e-21
    dirty = S.copy()
    dirty[0, k_lo - 1] = dirty[0, k_hi] = (3 + 4j) * 1e-21
    g = Grid(n, m, n, seed=9)
    lanes = torch.as_tensor(np.array([[k_lo, k_hi]], dtype=np.int32), device="cuda")
    d = _crandn(g.rng, (2, g.nb)) * 1e-21
    local = g.hcv.local_data(torch.as_tensor(d, device="cuda"), g.w_t, g.k0)
    got, emitted = [], []
    for rows in (S, dirty):
        St = g.rows(rows)
        out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        assert g.hcv.loglike_local(St, local, out, g.scr, g.lib, lanes=lanes, support=n)
        got.append(out.cpu().numpy())
        emitted.append(g.hcv.local_emit(St, g.wl_t, g.kself, g.lib, lanes=lanes, support=n))
    assert got[0].tobytes() == got[1].tobytes() and torch.equal(emitted[0], emitted[1])
    Sw, Cs = _reference(S, n, "sum")
    g.check_logl(got[1][0], Sw[0], g.e_bin(S[0], Cs[0]), d, "outside the lane range")
