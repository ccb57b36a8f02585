"""efd_pair_stats_cpu / efd_td_split_pair_stats_cpu / efd_window_rows_cpu (the host twins of the
mode-by-mode study's reductions) against plain numpy, their exact zeros, row independence, NaN
confinement and argument errors. Runs without a GPU. Tolerances: tests/pair_stats_ref.py."""

import ctypes

import numpy as np
import pytest

from tests import pair_stats_ref as pr
from tests import td_template_ref as tr


@pytest.mark.parametrize("nchan", [1, 2])
@pytest.mark.parametrize("nrow", pr.NROWS)
@pytest.mark.parametrize("nbin", pr.NBINS)
def test_twin_matches_numpy(nbin, nrow, nchan):
    a, b, w = pr.random_pairs(nbin, nrow, nchan)
    rc, out = pr.pair_cpu(a, b, w, nchan, nbin)
    assert rc == 0
    pr.assert_close(out, pr.pair_numpy(a, b, w, nchan, nbin), what=f"nbin={nbin} nrow={nrow}")


@pytest.mark.parametrize("nchan", [1, 2])
@pytest.mark.parametrize("nbin,nrow", [(257, 9), (8194, 5)])
def test_twin_variants(nbin, nrow, nchan):
    a, b, w = pr.random_pairs(nbin, nrow, nchan, seed=1, pad=3)
    ne = nchan * nbin
    ta, tb = np.ascontiguousarray(a[:, :ne]), np.ascontiguousarray(b[:, :ne])
    rc, out = pr.pair_cpu(a, b, w, nchan, nbin)               # padded strides (NaN padding)
    assert rc == 0
    pr.assert_close(out, pr.pair_numpy(ta, tb, w, nchan, nbin), what="padded")
    assert pr.same_bits(pr.pair_cpu(ta, tb, w, nchan, nbin)[1], out)   # the stride changes nothing
    assert pr.same_bits(pr.pair_cpu(a, tb, w, nchan, nbin)[1], out)    # nor do unequal strides
    rc, o1 = pr.pair_cpu(ta, tb, None, nchan, nbin)            # w = NULL
    assert rc == 0
    pr.assert_close(o1, pr.pair_numpy(ta, tb, None, nchan, nbin), what="w NULL")
    wz = w.copy()                                              # masked bins
    wz[::3] = 0.0
    wz[nbin // 2:nbin // 2 + 70] = 0.0
    rc, o2 = pr.pair_cpu(ta, tb, wz, nchan, nbin)
    assert rc == 0
    pr.assert_close(o2, pr.pair_numpy(ta, tb, wz, nchan, nbin), what="w with zeros")


def test_near_equal_pair_keeps_dd():
    """b = a (1 + 1e-7 smooth): dd holds to 1e-12 relative; the same number taken as
    aa + bb - 2 abr (printed) has lost every digit."""
    nbin, nrow = 8194, 3
    a, b, w = pr.near_equal_pairs(nbin, nrow)
    rc, out = pr.pair_cpu(a, b, w, 2, nbin)
    ref = pr.pair_numpy(a, b, w, 2, nbin)
    assert rc == 0
    dd, dref = out[..., 4], ref[..., 4]
    alg = out[..., 0] + out[..., 1] - 2.0 * out[..., 2]
    print(f"dd rel err {np.max(np.abs(dd / dref - 1)):.3e}; "
          f"aa + bb - 2 abr rel err {np.max(np.abs(alg / dref - 1)):.3e}; dd / aa "
          f"{np.max(dref / ref[..., 0]):.3e}")
    assert np.all(dref > 0.0) and np.all(np.abs(dd - dref) <= 1e-12 * dref)
    pr.assert_close(out, ref, what="near-equal")


def test_exact_zeros_for_identical_pair():
    nbin, nrow = 8194, 9
    a, _, w = pr.random_pairs(nbin, nrow, 2, seed=2)
    rc, out = pr.pair_cpu(a, a.copy(), w, 2, nbin)
    assert rc == 0
    assert np.all(out[..., 3] == 0.0) and np.all(out[..., 4] == 0.0)
    assert np.all(out[..., 0] > 0.0)
    assert pr.same_bits(out[..., 0], out[..., 1]) and pr.same_bits(out[..., 0], out[..., 2])


@pytest.mark.parametrize("nchan", [1, 2])
def test_row_independence_bitwise(nchan):
    nbin = 8194
    a, b, w = pr.random_pairs(nbin, 9, nchan, seed=4, pad=1)
    rc, out = pr.pair_cpu(a, b, w, nchan, nbin)
    assert rc == 0
    for r in (0, 4, 8):
        rc, one = pr.pair_cpu(a[r:r + 1], b[r:r + 1], w, nchan, nbin)
        assert rc == 0 and pr.same_bits(one[0], out[r]), r


def test_nan_stays_in_its_row():
    nbin = 257
    a, b, w = pr.random_pairs(nbin, 3, 2, seed=6)
    ref = pr.pair_cpu(a, b, w, 2, nbin)[1]
    for side in (0, 1):
        for where in (0, nbin - 1, 2 * nbin - 1):
            x = [a.copy(), b.copy()]
            x[side][1, where] = np.nan
            out = pr.pair_cpu(x[0], x[1], w, 2, nbin)[1]
            assert np.isnan(out[1]).any() and np.isnan(out[1, where // nbin, 4])
            assert pr.same_bits(out[0], ref[0]) and pr.same_bits(out[2], ref[2])


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", tr.CASES_N)
def test_split_twin_matches_numpy(n, rows):
    Z, buf, a, w = pr.split_case(n, rows)
    nb = (n + 1) // 2
    got = pr.split_pair_cpu(buf, n, pr.GAIN, a, w)
    b_np = tr.channels_from_Z(Z, pr.GAIN)
    b_tw = tr.split_cpu(buf, n, pr.GAIN)
    delta = pr.split_delta(b_np, b_tw, w)
    ref = pr.pair_numpy(a, b_np.reshape(rows, -1), w, 2, nb)
    print(f"n={n} rows={rows}: |b_numpy - b_twin| / |b| "
          f"{np.max(delta / np.sqrt(ref[..., 1])):.3e} (largest distance {delta.max():.3e})")
    pr.assert_close(got, ref, delta, what=f"split n={n}")
    # and the fused form is the stored split through efd_pair_stats_cpu, bit for bit
    rc, two = pr.pair_cpu(a, b_tw.reshape(rows, -1), w, 2, nb)
    assert rc == 0 and pr.same_bits(two, got)


@pytest.mark.parametrize("n", [8, 1025])
def test_split_twin_keep_and_null_weight(n):
    Z, buf, a, w = pr.split_case(n, 3, seed=1)
    nb = (n + 1) // 2
    keep = np.ones(nb, dtype=np.uint8)
    keep[::3] = 0
    b_tw = tr.split_cpu(buf, n, pr.GAIN, keep=keep)
    assert np.all(b_tw[:, :, ::3] == 0.0)
    for ww in (w, None):
        got = pr.split_pair_cpu(buf, n, pr.GAIN, a, ww, keep=keep)
        rc, two = pr.pair_cpu(a, b_tw.reshape(3, -1), ww, 2, nb)
        assert rc == 0 and pr.same_bits(two, got)
    # a NaN under a dropped bin is never read
    bad = buf.copy()
    bad[1, 3] = np.nan
    assert pr.same_bits(pr.split_pair_cpu(bad, n, pr.GAIN, a, w, keep=keep),
                        pr.split_pair_cpu(buf, n, pr.GAIN, a, w, keep=keep))


@pytest.mark.parametrize("n", [8, 1025])
def test_split_twin_rows_and_nan(n):
    Z, buf, a, w = pr.split_case(n, 3, seed=2)
    ref = pr.split_pair_cpu(buf, n, pr.GAIN, a, w)
    one = pr.split_pair_cpu(buf[1:2], n, pr.GAIN, a[1:2], w)
    assert pr.same_bits(one[0], ref[1])
    for where in (0, n // 2, n - 1):   # even n: n // 2 is the Nyquist bin, in neither channel
        bad = buf.copy()
        bad[1, where] = np.nan
        out = pr.split_pair_cpu(bad, n, pr.GAIN, a, w)
        assert np.all(np.isnan(out[1, :, 4])) or where != n // 2
        assert np.isnan(out[1]).any(), where
        assert pr.same_bits(out[0], ref[0]) and pr.same_bits(out[2], ref[2])
        assert pr.same_bits(out[1, :, 0], ref[1, :, 0])   # aa does not depend on Z


def test_argument_errors():
    from emri_frequencydomainwaveforms_amd import _lib
    lib = _lib.load()
    x = np.zeros(64, dtype=np.complex128)
    p = ctypes.c_void_p(x.ctypes.data)
    buf = ctypes.create_string_buffer(256)
    wins = (ctypes.c_void_p * 2)(None, None)

    def pair(fn, a=p, sa=16, b=p, sb=16, nrow=2, nchan=2, nbin=8, out=p, scr=p):
        rc = fn(a, sa, b, sb, nrow, nchan, nbin, None, out, scr, None)
        (lib.efd_cpu_last_error if fn is lib.efd_pair_stats_cpu else lib.efd_last_error)(buf, 256)
        return rc, buf.value

    def split(fn, Z=p, stride=8, n=8, rows=2, a=p, sa=8, out=p, scr=p):
        rc = fn(Z, stride, n, rows, 1.0, a, sa, None, None, out, scr, None)
        (lib.efd_cpu_last_error if fn is lib.efd_td_split_pair_stats_cpu
         else lib.efd_last_error)(buf, 256)
        return rc, buf.value

    def window(fn, h=p, n=8, win=wins, nwin=2, out=p, stride=8):
        return fn(h, n, win, nwin, out, stride, None)

    assert pair(lib.efd_pair_stats_cpu)[0] == 0
    assert split(lib.efd_td_split_pair_stats_cpu)[0] == 0
    assert window(lib.efd_window_rows_cpu) == 0
    # the device entry points validate before any launch (fake pointers are never dereferenced)
    for fn, name in ((lib.efd_pair_stats_cpu, b"efd_pair_stats_cpu"),
                     (lib.efd_pair_stats, b"efd_pair_stats")):
        bad = [dict(a=None), dict(b=None), dict(out=None), dict(nrow=0), dict(nrow=65),
               dict(nbin=0), dict(nbin=-1), dict(sa=15), dict(sb=15), dict(nchan=0),
               dict(nchan=3)]
        if fn is lib.efd_pair_stats:
            bad.append(dict(scr=None))
        for kw in bad:
            rc, msg = pair(fn, **kw)
            assert rc == _lib.EFD_ERR_ARG and name in msg, (kw, msg)
    for fn, name in ((lib.efd_td_split_pair_stats_cpu, b"efd_td_split_pair_stats_cpu"),
                     (lib.efd_td_split_pair_stats, b"efd_td_split_pair_stats")):
        bad = [dict(Z=None), dict(a=None), dict(out=None), dict(rows=0), dict(rows=65),
               dict(n=0), dict(stride=7), dict(sa=7)]
        if fn is lib.efd_td_split_pair_stats:
            bad.append(dict(scr=None))
        for kw in bad:
            rc, msg = split(fn, **kw)
            assert rc == _lib.EFD_ERR_ARG and name in msg, (kw, msg)
    for fn in (lib.efd_window_rows_cpu, lib.efd_window_rows):
        for kw in (dict(h=None), dict(win=None), dict(out=None), dict(n=0), dict(nwin=0),
                   dict(nwin=17), dict(stride=7)):
            assert window(fn, **kw) == _lib.EFD_ERR_ARG, kw


@pytest.mark.parametrize("n", [1, 63, 257, 8194])
def test_window_rows_twin_bitwise(n):
    h, win = pr.windows_case(n)
    got = pr.window_rows_cpu(h, win, n + 3)
    ref = pr.window_rows_numpy(h, win, n + 3)
    assert pr.same_bits(got.view(np.float64), ref.view(np.float64))
    assert pr.same_bits(got[1, :n].view(np.float64), h.view(np.float64))   # NULL: a bitwise copy
