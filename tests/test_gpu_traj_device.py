"""The inspiral trajectories and the p0 solve on the device (efd_traj_batch,
efd_traj_p_at_t_batch: one wavefront per source) against the native host forms,
efd_host_trajectory and efd_host_p_at_t, which compile the same integrator and root solve
(csrc/emrifd_rk45.h) with their own powers, quadrature loop and knot store. STAND-IN PHYSICS,
NOT FEW.

The device integrates the same equations with the same integrator and aims at the host's own
steps: the quadrature is summed in the host's order and the three powers are correctly rounded,
which the host's std::pow is in 99.92 % of its calls. Where one call differs the two part by a
last bit from there on. It is held to the yardsticks tests/test_native_upstream.py holds native
to scipy by: knot count within 2, end time to 1e-10, a cubic spline through the device knots
reproducing the host knots' p, e to 1e-10 and the phases to 1e-9 of their maxima, the knot
frequencies to 1e-13 of get_fundamental_frequencies, p0 to 1e-13.

Measured on an MI355X (knots device / host, knots that coincide bit for bit, end time, spline p,
e, Phi_phi, Phi_r, knot frequencies against numpy's; p0 relative to the host's):
  source 0 (1e6, 10, 0.35, 2 yr)    95 / 95, 95, 0, 0 0 0 0, 8.9e-16; p0 3.8e-16
  source 1 (1e5, 1, 0.1, 1 yr)     137 / 137, 137, 0, 0 0 0 0, 1.0e-15; p0 2.6e-16
  source 2 (1e7, 100, 0.6, 1 yr)    26 / 26, 26, 0, 0 0 0 0, 8.9e-16; p0 0
  source 3 (3e5, 10, 0.3, 0.02 yr)  46 / 46, 33, 3.7e-15, 2.5e-16 1.9e-16 3.3e-15 6.3e-15, 1.0e-15; p0 0
  source 4 (p0 = 12, ends at T)     11 / 11, 11, 0, 0 0 0 0, 4.4e-16
An earlier form with butterfly sums placed its knots as a third valid integration does (2 knots
coinciding) and missed the phase yardstick on the 26-knot source (1.84e-9, 1.43e-9).
"""

import ctypes

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib  # noqa: E402
from emri_frequencydomainwaveforms_amd.constants import MTSUN_SI, YRSID_SI  # noqa: E402
from emri_frequencydomainwaveforms_amd.frequencies import get_fundamental_frequencies  # noqa: E402
from emri_frequencydomainwaveforms_amd.trajectory import (EMRIInspiral, device_trajectories,  # noqa: E402
                                                          get_p_at_t, get_p_at_t_batch)

# tests/test_native_upstream.py's SOURCES: (M, mu, e0, T)
SOURCES = [(1e6, 10.0, 0.35, 2.0), (1e5, 1.0, 0.1, 1.0), (1e7, 100.0, 0.6, 1.0),
           (3e5, 10.0, 0.3, 0.02)]
NO_PLUNGE = (1e6, 10.0, 12.0, 0.2, 0.5)      # (M, mu, p0, e0, T): ends at T
PHI = (0.3, 1.1)
RTOL = ATOL = 1e-12
L = 1000


@pytest.fixture(scope="module")
def ref():
    """Per source: the row (M, mu, p0, e0, Phi_phi0, Phi_r0, T) and the host's seven arrays;
    the host's p0 of the four plunging sources."""
    traj = EMRIInspiral(backend="native")
    p0s = [get_p_at_t(traj, 0.99 * T, [M, mu, 0.0, e0, 1.0]) for M, mu, e0, T in SOURCES]
    rows = [(M, mu, p0, e0, *PHI, T) for (M, mu, e0, T), p0 in zip(SOURCES, p0s)]
    M, mu, p0, e0, T = NO_PLUNGE
    rows.append((M, mu, p0, e0, *PHI, T))
    host = [traj.with_frequencies(r[0], r[1], 0.0, r[2], r[3], 1.0, Phi_phi0=r[4], Phi_r0=r[5],
                                  T=r[6]) for r in rows]
    return dict(traj=traj, p0=np.array(p0s), rows=np.array(rows), host=host)


@pytest.fixture(scope="module")
def dev(ref):
    """The five sources in one launch: (arrays per source as numpy, nt, status)."""
    knots, nt, status = device_trajectories(ref["rows"], RTOL, ATOL, L)
    k = knots.cpu().numpy()
    return [[k[i, j, :n].copy() for j in range(7)] for i, n in enumerate(nt)], nt, status


@pytest.mark.parametrize("i", range(5))
def test_trajectories_match_host(ref, dev, i):
    arrs, nt, status = dev
    assert status[i] == _lib.EFD_TRAJ_OK
    assert min(len(h[0]) for h in ref["host"][:4]) >= 20   # the plunging four
    row, a, b = ref["rows"][i], arrs[i], ref["host"][i]
    M = row[0]
    assert nt[i] == len(a[0])
    same = int(np.isin(a[0], b[0]).sum())
    tt = b[0][1:-1]
    errs = {}
    for j, name in ((1, "p"), (2, "e"), (3, "Phi_phi"), (4, "Phi_r")):
        s = CubicSpline(a[0], a[j])
        errs[name] = np.max(np.abs(s(tt) - b[j][1:-1])) / np.max(np.abs(b[j]))
    op, _, orr = get_fundamental_frequencies(0.0, a[1], a[2], 0.0)
    ef = max(np.max(np.abs(a[5] / (op / (2 * np.pi * M * MTSUN_SI)) - 1.0)),
             np.max(np.abs(a[6] / (orr / (2 * np.pi * M * MTSUN_SI)) - 1.0)))
    dt_end = abs(a[0][-1] - b[0][-1]) / b[0][-1]
    print(f"source {i}: knots device {len(a[0])} host {len(b[0])} ({same} coincide), "
          f"end time rel {dt_end:.3g}, spline p {errs['p']:.3g} e {errs['e']:.3g} "
          f"Phi_phi {errs['Phi_phi']:.3g} Phi_r {errs['Phi_r']:.3g}, freq rel {ef:.3g}")
    assert a[0][0] == 0.0 and np.all(np.diff(a[0]) > 0.0)
    assert a[1][0] == row[2] and a[2][0] == row[3] and a[3][0] == PHI[0] and a[4][0] == PHI[1]
    if i < 4:    # the four end on the separatrix event, the fifth at T
        assert abs(a[1][-1] - (6.0 + 2.0 * a[2][-1]) - 0.1) <= 1e-12
    else:
        assert a[0][-1] == pytest.approx(NO_PLUNGE[4] * YRSID_SI, rel=1e-15)
        assert a[1][-1] - (6.0 + 2.0 * a[2][-1]) > 0.1
    assert abs(len(a[0]) - len(b[0])) <= 2
    assert dt_end <= 1e-10
    assert ef <= 1e-13
    assert errs["p"] <= 1e-10 and errs["e"] <= 1e-10
    assert errs["Phi_phi"] <= 1e-9 and errs["Phi_r"] <= 1e-9


def test_device_batch_views_and_errors(ref, dev):
    """EMRIInspiral.device_batch: device views of the same knots; a refused source raises what
    the native host path raises."""
    traj = ref["traj"]
    views, nt = traj.device_batch([tuple(r) for r in ref["rows"]])
    assert list(nt) == list(dev[1])
    for v, a in zip(views, dev[0]):
        assert len(v) == 7 and all(x.is_cuda and x.dtype == torch.float64 for x in v)
        for x, y in zip(v, a):
            np.testing.assert_array_equal(x.cpu().numpy(), y)
    good = tuple(ref["rows"][3])
    with pytest.raises(ValueError, match="inside the separatrix buffer"):
        traj.device_batch([good, (1e6, 10.0, 6.75, 0.35, 0.0, 0.0, 1.0)])
    with pytest.raises(RuntimeError, match="trajectory integration failed"):
        traj.device_batch([good, (-1e6, 10.0, 12.0, 0.35, 0.0, 0.0, 1.0)])
    short = EMRIInspiral(backend="native", max_init_len=8)
    with pytest.raises(ValueError, match="longer than max_init_len"):
        short.device_batch([good])
    with pytest.raises(ValueError, match="longer than max_init_len"):
        short.with_frequencies(good[0], good[1], 0.0, good[2], good[3], 1.0, T=good[6])


def test_batch_of_17_is_bitwise_17_launches_of_one(ref):
    """One past EFD_BATCH_MAX, standing for any count."""
    assert _lib.EFD_BATCH_MAX == 16
    rows = np.array([ref["rows"][i % 5] for i in range(17)])
    rows[:, 4] += 0.37 * np.arange(17)                  # distinct Phi_phi0
    rows[:, 0] *= 1.0 + 1e-4 * (np.arange(17) // 5)     # and M from the second cycle on
    knots, nt, status = device_trajectories(rows, RTOL, ATOL, L)
    knots = knots.cpu().numpy()
    assert np.all(status == 0) and len(set(nt.tolist())) > 3
    for i in range(17):
        k1, n1, s1 = device_trajectories(rows[i:i + 1], RTOL, ATOL, L)
        assert s1[0] == 0 and n1[0] == nt[i]
        np.testing.assert_array_equal(k1.cpu().numpy()[0], knots[i])


def _raw_launch(rows9, max_len, sentinel, pad=64):
    """efd_traj_batch on a sentinel-filled knot buffer with `pad` doubles behind the last slab;
    nt and status start at -7."""
    lib = _lib.load()
    B = len(rows9)
    src = torch.from_numpy(np.ascontiguousarray(rows9, dtype=np.float64)).cuda()
    knots = torch.full((B * 7 * max_len + pad,), sentinel, dtype=torch.float64, device="cuda")
    ints = torch.full((2 * B,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.efd_traj_batch(src.data_ptr(), B, max_len, knots.data_ptr(), ints.data_ptr(),
                                  ints.data_ptr() + 4 * B, st), "efd_traj_batch", lib)
    torch.cuda.synchronize()
    k = knots.cpu().numpy()
    i = ints.cpu().numpy()
    return k[:B * 7 * max_len].reshape(B, 7, max_len), k[B * 7 * max_len:], i[:B], i[B:]


def test_status_words_without_faults(ref):
    """Five sources, max_len = 8, one launch: two that fit (a few knots each), one with p0 inside
    the separatrix buffer, one with a NaN mass, one with more than 8 knots. Each reports its own
    status; the good ones are bitwise their solo results; nothing outside a source's own 8 knots
    per array is written."""
    SENT = -777.25
    tol = [RTOL, ATOL]
    good_a = [1e6, 10.0, 12.0, 0.2, 0.3, 1.1, 1e-4, *tol]
    good_b = [3e5, 10.0, 10.0, 0.3, 0.0, 0.5, 3e-5, *tol]
    inside = [1e6, 10.0, 6.75, 0.35, 0.0, 0.0, 1.0, *tol]
    nan_m = [float("nan"), 10.0, 12.0, 0.2, 0.0, 0.0, 1.0, *tol]
    too_long = [*ref["rows"][0], *tol]
    rows = np.array([good_a, inside, nan_m, too_long, good_b])
    k, tail, nt, status = _raw_launch(rows, 8, SENT)
    assert status.tolist() == [_lib.EFD_TRAJ_OK, _lib.EFD_TRAJ_BAD_SOURCE,
                               _lib.EFD_TRAJ_BAD_SOURCE, _lib.EFD_TRAJ_TOO_LONG, _lib.EFD_TRAJ_OK]
    assert 2 <= nt[0] <= 8 and 2 <= nt[4] <= 8
    assert nt[1] == -7 and nt[2] == -7 and (nt[3] == -7 or nt[3] <= 8)
    assert np.all(tail == SENT)
    assert np.all(k[1] == SENT) and np.all(k[2] == SENT)
    for i in (0, 4):
        assert np.all(k[i, :, nt[i]:] == SENT) and np.all(k[i, :, :nt[i]] != SENT)
        k1, tail1, n1, s1 = _raw_launch(rows[i:i + 1], 8, SENT)
        assert s1[0] == 0 and n1[0] == nt[i] and np.all(tail1 == SENT)
        np.testing.assert_array_equal(k1[0], k[i])
    # the good sources' few knots are the host's trajectory too (the same yardstick: end time)
    traj = ref["traj"]
    for i in (0, 4):
        r = rows[i]
        h = traj.with_frequencies(r[0], r[1], 0.0, r[2], r[3], 1.0, Phi_phi0=r[4], Phi_r0=r[5],
                                  T=r[6])
        assert abs(len(h[0]) - nt[i]) <= 2
        assert abs(h[0][-1] - k[i, 0, nt[i] - 1]) <= 1e-10 * h[0][-1]
    # the other three's own status does not depend on the launch either
    for i, want in ((1, _lib.EFD_TRAJ_BAD_SOURCE), (2, _lib.EFD_TRAJ_BAD_SOURCE),
                    (3, _lib.EFD_TRAJ_TOO_LONG)):
        k1, tail1, n1, s1 = _raw_launch(rows[i:i + 1], 8, SENT)
        assert s1[0] == want and np.all(tail1 == SENT)
    # rtol, atol and T must be positive as well
    bad = np.array([good_a] * 3)
    bad[0, 6], bad[1, 7], bad[2, 8] = 0.0, -1e-12, 0.0
    _, _, n3, s3 = _raw_launch(bad, 8, SENT)
    assert s3.tolist() == [_lib.EFD_TRAJ_BAD_SOURCE] * 3 and n3.tolist() == [-7] * 3


def test_knot_count_boundary(ref):
    """The device's knot sink at the boundary (the host's: tests/test_native_upstream.py):
    max_len = nt succeeds with the knots of the roomy launch; max_len = nt - 1 is
    EFD_TRAJ_TOO_LONG and nothing behind the slab is written. NO_PLUNGE, one source a launch."""
    SENT = -777.25
    row = np.array([[*ref["rows"][4], RTOL, ATOL]])
    k, tail, nt, status = _raw_launch(row, L, SENT)
    n = int(nt[0])
    assert status[0] == _lib.EFD_TRAJ_OK and 2 < n < L and np.all(tail == SENT)
    assert np.all(k[0, :, :n] != SENT) and np.all(k[0, :, n:] == SENT)
    k1, tail1, nt1, status1 = _raw_launch(row, n, SENT)
    assert status1[0] == _lib.EFD_TRAJ_OK and nt1[0] == n and np.all(tail1 == SENT)
    np.testing.assert_array_equal(k1[0], k[0, :, :n])
    k2, tail2, nt2, status2 = _raw_launch(row, n - 1, SENT)
    assert status2[0] == _lib.EFD_TRAJ_TOO_LONG and nt2[0] == -7 and np.all(tail2 == SENT)
    # what it did write are the first n - 1 knots
    np.testing.assert_array_equal(k2[0], k[0, :, :n - 1])


def test_p_at_t_batch_matches_host(ref):
    traj = ref["traj"]
    rows = [(M, mu, e0) for M, mu, e0, T in SOURCES] + [(1e6, 10.0, 0.3)]
    t_out = [0.99 * T for *_, T in SOURCES] + [1e-4]     # the last: shorter than the plunge
    with pytest.raises(ValueError):                      # from the buffer; the host refuses it
        get_p_at_t(traj, t_out[-1], [1e6, 10.0, 0.0, 0.3, 1.0])
    p0, refused = get_p_at_t_batch(traj, t_out, rows)
    assert p0.shape == (5,) and refused.tolist() == [4] and np.isnan(p0[4])
    for i in range(4):
        rel = abs(p0[i] - ref["p0"][i]) / ref["p0"][i]
        print(f"source {i}: p0 device {p0[i]:.17g} host {ref['p0'][i]:.17g} rel {rel:.3g}")
        assert rel <= 1e-13
    # a scalar t_out, and each row alone gives the same bits
    for i in range(4):
        p1, r1 = get_p_at_t_batch(traj, t_out[i], [rows[i]])
        assert len(r1) == 0 and p1[0] == p0[i]
    # the raw call writes NaN and EFD_TRAJ_NO_BRACKET for the refused row
    lib = _lib.load()
    src = np.zeros((1, 9))
    src[0, [0, 1, 3, 6, 7, 8]] = [1e6, 10.0, 0.3, 1e-4, RTOL, ATOL]
    d = torch.from_numpy(src).cuda()
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    stw = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.efd_traj_p_at_t_batch(d.data_ptr(), 1, 2e-12, 8.881784197001252e-16,
                                         out.data_ptr(), stw.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream),
               "efd_traj_p_at_t_batch", lib)
    torch.cuda.synchronize()
    assert stw.item() == _lib.EFD_TRAJ_NO_BRACKET and np.isnan(out.item())
    assert ctypes.sizeof(_lib.TrajSource) == 72
