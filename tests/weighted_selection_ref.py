"""Shared by tests/test_weighted_selection.py and tests/test_gpu_weighted_selection.py: a plain
restatement of the noise-weighted ModeSelector (sort every branch, cumulative sum), the PSD
tables and synthetic cases the issue names, and the preconditions under which the kept set does
not depend on the order of a sum. STAND-IN PHYSICS, NOT FEW."""

import ctypes

import numpy as np
from scipy.interpolate import PPoly

from emri_frequencydomainwaveforms_amd import _lib, fdutils
from tests.test_gpu_modes_device import CUT_GAP, SUM_MARGIN, branch_powers, synthetic

U = 2.0 ** -53
S1 = (1e6, 10.0, 0.35, 0.1)    # M, mu, e0, T [yr]
S2 = (5e6, 50.0, 0.1, 1.0)


def lisa():
    """The LISA_Alloc_Sh spline (fdutils.get_sensitivity's)."""
    return fdutils._spline()


def wall():
    """S = 1 below 4e-3 Hz, 2^120 above."""
    return PPoly(np.array([[1.0, 2.0 ** 120]]), np.array([0.0, 4e-3, 1.0]))


def flat():
    """S = 0.25: a power of two, so the weighting scales every power exactly."""
    return PPoly(np.array([[0.25]]), np.array([0.0, 1.0]))


def negative():
    """S = 1 below 5e-3 Hz, -1 from there on."""
    return PPoly(np.array([[1.0, -1.0]]), np.array([0.0, 5e-3, 1.0]))


def all_negative():
    return PPoly(np.array([[-1.0]]), np.array([0.0, 1.0]))


def gentle():
    """S = 1 + 30 f."""
    return PPoly(np.array([[30.0], [1.0]]), np.array([0.0, 1.0]))


def freqs(nt):
    f_phi = np.linspace(1e-3, 3e-3, nt)
    return f_phi, 0.6 * f_phi


def mode_freq(m, n, f_phi, f_r):
    """F[i, k] = |m_k f_phi[i] + n_k f_r[i]|."""
    m, n = np.asarray(m, dtype=np.float64), np.asarray(n, dtype=np.float64)
    return np.abs(m[None, :] * f_phi[:, None] + n[None, :] * f_r[:, None])


def weights(fn, F):
    S = np.asarray(fn(F), dtype=np.float64)
    ok = np.isfinite(S) & (S > 0.0)
    W = np.zeros_like(S)
    W[ok] = 1.0 / S[ok]
    return W


def weighted_powers(A, ylms, m0mask, W):
    """Branch powers [N_t][K + partners] times each mode's weight, and the fold map."""
    power, partner_idx = branch_powers(A, ylms, m0mask)
    K = A.shape[1]
    return power * np.concatenate([W, W[:, m0mask]], axis=1), \
        np.concatenate([np.arange(K), partner_idx])


def restated(power, fold, eps):
    """The selection on given branch powers, knot by knot: every branch sorted descending, a
    branch kept while the sum before it is < (1 - eps) total, the first always; a knot whose
    total is 0 or not finite keeps nothing; partner picks fold; union over the knots."""
    kept = set()
    for row in power:
        total = float(np.cumsum(np.sort(row)[::-1])[-1])
        if not (np.isfinite(total) and total > 0.0):
            continue
        order = sorted(range(len(row)), key=lambda q: -row[q])
        before = 0.0
        for c, q in enumerate(order):
            if c == 0 or before < total * (1.0 - eps):
                kept.add(int(fold[q]))
            before += row[q]
    return np.array(sorted(kept), dtype=np.int64)


def margins(power, eps):
    """tests/test_gpu_modes_device.py: cut_margins on given (weighted) powers; knots with a
    zero total keep nothing in any order and are skipped."""
    margin, gap = np.inf, np.inf
    for row in power:
        ps = np.sort(row)[::-1]
        cs = np.cumsum(ps)
        total = cs[-1]
        if not total > 0.0:
            continue
        thr = total * (1.0 - eps)
        before = np.concatenate([[0.0], cs[:-1]])
        kept = before < thr
        kept[0] = True
        c = int(kept.sum())
        assert kept[:c].all()
        if c > 1:
            margin = min(margin, (thr - before[c - 1]) / total)
        if c < len(ps):
            margin = min(margin, (before[c] - thr) / total)
            gap = min(gap, (ps[c - 1] - ps[c]) / ps[c - 1])
    return margin, gap


def assert_order_independent(power, eps, what=""):
    margin, gap = margins(power, eps)
    print(f"{what} precondition: sum margin {margin:.3g} (>= {SUM_MARGIN:g}), cut gap {gap:.3g} "
          f"(>= {CUT_GAP:g})")
    assert margin >= SUM_MARGIN and gap >= CUT_GAP, (margin, gap)
    return margin, gap


def generic_cases():
    """name -> (teuk, ylms, m0mask, (l, m, n), eps, (f_phi, f_r))."""
    cases = {}

    def add(name, seed, nt, K, m, n, eps, **kw):
        teuk, ylms = synthetic(seed, nt, K, **kw)
        m, n = np.asarray(m, dtype=np.int32), np.asarray(n, dtype=np.int32)
        cases[name] = (teuk, ylms, m != 0, (np.full(K, 2, dtype=np.int32), m, n), eps, freqs(nt))

    add("five_m0_modes", 11, 2, 5, np.zeros(5), np.arange(-2, 3), 1e-1)
    add("one_mode", 12, 3, 1, [1], [0], 1e-2)
    k = np.arange(40)
    add("forty", 15, 3, 40, k % 5, k // 5 - 4, 1e-2, decades=1.0)
    k = np.arange(4096)
    add("full_sort_8192", 13, 4, 4096, 1 + k % 10, (k // 10) % 61 - 30, 1e-6)
    return cases


def psd_struct(tab):
    """(efd_psd_table over host arrays, the arrays) of a PPoly-shaped object, padded to cubics."""
    x = np.ascontiguousarray(tab.x, dtype=np.float64)
    c = np.asarray(tab.c, dtype=np.float64)
    c = np.ascontiguousarray(np.concatenate([np.zeros((4 - c.shape[0], c.shape[1])), c]))
    return _lib.PsdTable(x.ctypes.data, c.ctypes.data, len(x)), (x, c)


def psd_points(tab):
    """Every knot, every midpoint, 0 and 1e-6 (below the table), 2.0 (above it) and 1,000
    log-uniform points."""
    x = np.asarray(tab.x)
    rng = np.random.default_rng(7)
    return np.concatenate([x, 0.5 * (x[1:] + x[:-1]), [0.0, 1e-6, 2.0],
                           10.0 ** rng.uniform(np.log10(x[0]), np.log10(x[-1]), 1000)])


def psd_bound(tab, f):
    """32 u M(f), M = |c0 s^3| + |c1 s^2| + |c2 s| + |c3| on f's piece: two Horner-like
    evaluations of about 10 u M each."""
    x, c = np.asarray(tab.x), np.asarray(tab.c)
    i = np.clip(np.searchsorted(x, f, side="right") - 1, 0, len(x) - 2)
    s = f - x[i]
    k = c.shape[0]
    M = sum(np.abs(c[j, i] * s ** (k - 1 - j)) for j in range(k))
    return 32.0 * U * M, M


def eval_cpu(lib, tab, f):
    st, hold = psd_struct(tab)
    f = np.ascontiguousarray(f, dtype=np.float64)
    out = np.full(f.shape, -7.0)
    rc = lib.efd_psd_eval_cpu(ctypes.byref(st), f.ctypes.data, f.size, out.ctypes.data, None)
    assert rc == 0, rc
    return out
