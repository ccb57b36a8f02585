"""efd_pair_stats / efd_td_split_pair_stats / efd_window_rows on the device, through
reductions.Reducer, against their CPU twins: the sizes of tests/test_pair_stats_cpu.py plus the
ones at which the partition changes (more than 8 chunks, the chunk cap), reproducibility, row
independence, the exact zeros and NaN confinement. Tolerances: tests/pair_stats_ref.py (device
against twin: the same float64 terms in another order; for the split form the two sides' b are
the same arithmetic, so no distance term is added)."""

import numpy as np
import pytest

from tests import pair_stats_ref as pr
from tests import td_template_ref as tr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def red():
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    return Reducer()


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def pair_gpu(red, a, b, w, nchan, nbin):
    """Reducer.pair_stats on device copies of [nrow][stride] host rows (strides kept)."""
    da, db = _dev(a), _dev(b)
    va = da[:, :nchan * nbin].unflatten(1, (nchan, nbin))
    vb = db[:, :nchan * nbin].unflatten(1, (nchan, nbin))
    out = red.pair_stats(va, vb, _dev(w))
    return out.cpu().numpy()


def split_pair_gpu(red, buf, n, a, w, keep=None):
    nb = (n + 1) // 2
    da = _dev(a)[:, :2 * nb].unflatten(1, (2, nb))
    out = red.td_split_pair_stats(_dev(buf), n, pr.GAIN, da, _dev(w), keep=_dev(keep))
    return out.cpu().numpy()


@pytest.mark.parametrize("nchan", [1, 2])
@pytest.mark.parametrize("nrow", pr.NROWS)
@pytest.mark.parametrize("nbin", pr.NBINS)
def test_matches_cpu_twin(red, nbin, nrow, nchan):
    a, b, w = pr.random_pairs(nbin, nrow, nchan, pad=3)
    got = pair_gpu(red, a, b, w, nchan, nbin)
    rc, ref = pr.pair_cpu(a, b, w, nchan, nbin)
    assert rc == 0
    pr.assert_close(got, ref, what=f"nbin={nbin} nrow={nrow} nchan={nchan}")


@pytest.mark.parametrize("nbin,nchan", [(300001, 2), (1048583, 1)])
def test_many_chunks_match_cpu_twin(red, nbin, nchan):
    """300,001 bins: 288 chunks (whole rounds of 8); 1,048,583: the cap of 1024 chunks."""
    a, b, w = pr.random_pairs(nbin, 2, nchan)
    got = pair_gpu(red, a, b, w, nchan, nbin)
    rc, ref = pr.pair_cpu(a, b, w, nchan, nbin)
    assert rc == 0
    pr.assert_close(got, ref, what=f"nbin={nbin}")
    assert pr.same_bits(pair_gpu(red, a[1:], b[1:], None, nchan, nbin)[0],
                        pair_gpu(red, a, b, None, nchan, nbin)[1])


def test_variants_and_reproducibility(red):
    nbin, nrow = 8194, 9
    a, b, w = pr.random_pairs(nbin, nrow, 2, seed=1, pad=3)
    got = pair_gpu(red, a, b, w, 2, nbin)
    assert pr.same_bits(pair_gpu(red, a, b, w, 2, nbin), got)          # two runs, bitwise
    ta, tb = a[:, :2 * nbin], b[:, :2 * nbin]
    assert pr.same_bits(pair_gpu(red, ta, tb, w, 2, nbin), got)        # the stride changes nothing
    for ww in (None, np.where(np.arange(nbin) % 3 == 0, 0.0, w)):      # w NULL, w with zeros
        rc, ref = pr.pair_cpu(a, b, ww, 2, nbin)
        assert rc == 0
        pr.assert_close(pair_gpu(red, a, b, ww, 2, nbin), ref, what="w variant")
    for r in (0, 4, 8):                                                # a row alone, bitwise
        assert pr.same_bits(pair_gpu(red, a[r:r + 1], b[r:r + 1], w, 2, nbin)[0], got[r]), r


def test_more_rows_than_a_call(red):
    """70 rows go in two calls; every row is bitwise what it is alone."""
    nbin = 257
    a, b, w = pr.random_pairs(nbin, 70, 2, seed=7)
    got = pair_gpu(red, a, b, w, 2, nbin)
    rc, ref = pr.pair_cpu(a[:64], b[:64], w, 2, nbin)
    assert rc == 0
    pr.assert_close(got[:64], ref, what="first 64 of 70")
    for r in (0, 63, 64, 69):
        assert pr.same_bits(pair_gpu(red, a[r:r + 1], b[r:r + 1], w, 2, nbin)[0], got[r]), r


def test_near_equal_and_exact_zeros(red):
    nbin = 8194
    a, b, w = pr.near_equal_pairs(nbin, 3)
    got = pair_gpu(red, a, b, w, 2, nbin)
    ref = pr.pair_numpy(a, b, w, 2, nbin)
    alg = got[..., 0] + got[..., 1] - 2.0 * got[..., 2]
    print(f"dd rel err {np.max(np.abs(got[..., 4] / ref[..., 4] - 1)):.3e}; aa + bb - 2 abr rel "
          f"err {np.max(np.abs(alg / ref[..., 4] - 1)):.3e}")
    assert np.all(np.abs(got[..., 4] - ref[..., 4]) <= 1e-12 * ref[..., 4])
    same = pair_gpu(red, a, a.copy(), w, 2, nbin)
    assert np.all(same[..., 3] == 0.0) and np.all(same[..., 4] == 0.0)
    assert np.all(same[..., 0] > 0.0)
    assert pr.same_bits(same[..., 0], same[..., 1]) and pr.same_bits(same[..., 0], same[..., 2])


def test_nan_stays_in_its_row(red):
    nbin = 8194
    a, b, w = pr.random_pairs(nbin, 3, 2, seed=6)
    ref = pair_gpu(red, a, b, w, 2, nbin)
    for side in (0, 1):
        for where in (0, nbin + 4000, 2 * nbin - 1):
            x = [a.copy(), b.copy()]
            x[side][1, where] = np.nan
            out = pair_gpu(red, x[0], x[1], w, 2, nbin)
            assert np.isnan(out[1, where // nbin, 4])
            assert pr.same_bits(out[0], ref[0]) and pr.same_bits(out[2], ref[2])


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", tr.CASES_N + (600001,))
def test_split_matches_cpu_twin(red, n, rows):
    Z, buf, a, w = pr.split_case(n, rows)
    got = split_pair_gpu(red, buf, n, a, w)
    pr.assert_close(got, pr.split_pair_cpu(buf, n, pr.GAIN, a, w), what=f"split n={n}")
    assert pr.same_bits(split_pair_gpu(red, buf, n, a, w), got)        # two runs, bitwise
    if rows == 3:                                                      # a row alone, bitwise
        assert pr.same_bits(split_pair_gpu(red, buf[1:2], n, a[1:2], w)[0], got[1])


@pytest.mark.parametrize("n", [8, 1025])
def test_split_keep_null_weight_and_nan(red, n):
    Z, buf, a, w = pr.split_case(n, 3, seed=1)
    nb = (n + 1) // 2
    keep = np.ones(nb, dtype=np.uint8)
    keep[::3] = 0
    for ww, kk in ((w, keep), (None, keep), (None, None)):
        pr.assert_close(split_pair_gpu(red, buf, n, a, ww, kk),
                        pr.split_pair_cpu(buf, n, pr.GAIN, a, ww, kk), what="keep / w NULL")
    # the fused form is the stored split through efd_pair_stats, bit for bit
    from emri_frequencydomainwaveforms_amd import _lib
    dz = _dev(buf)
    stored = torch.empty((3, 2, nb), dtype=torch.complex128, device="cuda")
    _lib.check(red.lib.efd_td_split(torch.view_as_real(dz).data_ptr(), buf.shape[1], n, 3,
                                    pr.GAIN, _dev(keep).data_ptr(),
                                    torch.view_as_real(stored).data_ptr(), 2 * nb, None),
               "efd_td_split")
    da = _dev(a)[:, :2 * nb].unflatten(1, (2, nb))
    assert pr.same_bits(red.pair_stats(da, stored, _dev(w)).cpu().numpy(),
                        split_pair_gpu(red, buf, n, a, w, keep))
    ref = split_pair_gpu(red, buf, n, a, w)
    for where in (0, n // 2, n - 1):   # even n: n // 2 is the Nyquist bin, in neither channel
        bad = buf.copy()
        bad[1, where] = np.nan
        out = split_pair_gpu(red, bad, n, a, w)
        assert np.isnan(out[1]).any(), where
        assert pr.same_bits(out[0], ref[0]) and pr.same_bits(out[2], ref[2])
        assert pr.same_bits(out[1, :, 0], ref[1, :, 0])


@pytest.mark.parametrize("n", [1, 63, 257, 8194])
def test_window_rows_bitwise(red, n):
    h, win = pr.windows_case(n)
    out = torch.full((len(win), n + 3), 7.0 + 7.0j, dtype=torch.complex128, device="cuda")
    red.window_rows(_dev(h), [_dev(x) for x in win], out)
    ref = pr.window_rows_cpu(h, win, n + 3)
    assert pr.same_bits(out.cpu().numpy().view(np.float64), ref.view(np.float64))


def test_python_argument_checks(red):
    a = torch.zeros((2, 2, 8), dtype=torch.complex128, device="cuda")
    w = torch.ones(8, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        red.pair_stats(a, a[:1], w)
    with pytest.raises(ValueError):
        red.pair_stats(a, a.to(torch.complex64), w)
    with pytest.raises(ValueError):
        red.pair_stats(a, a, w[:7])
    with pytest.raises(ValueError):
        red.pair_stats(a.cpu(), a, w)
    with pytest.raises(ValueError):
        red.pair_stats(a[:, :, ::2], a[:, :, ::2], w[:4])
    Z = torch.zeros((2, 16), dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError):
        red.td_split_pair_stats(Z, 16, 1.0, a[:, :, :7], w)
    with pytest.raises(ValueError):
        red.td_split_pair_stats(Z, 17, 1.0, a, w)
    assert red.td_split_pair_stats(Z, 16, 1.0, a, w).shape == (2, 2, 5)
