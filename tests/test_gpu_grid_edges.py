"""The HIP mode sum's lane-range code on the grids of tests/grid_cases.py: non-uniform spacing
(k_items' linear index guess fails, so grid_bound's galloping search, record_safe's fallback
grid load and the certification of the range ends produce what is checked here), bins exactly
on knot frequencies and on their floating-point neighbours (the open/closed rule of a record's
[F_j, F_{j+1}), strict at a run's first knot), even-length symmetric grids (no f = 0 bin), lane
counts at a tile boundary (768 lanes), nf = 1, 2, 3, and repeated grid values (ascending, not
strictly: accepted by the ABI, the twin and the oracle alike). The input conditions (the guess
really fails, the knots really are bins) are asserted in tests/test_cpu_twin_grids.py, where the
host twin is held to the oracle on the same grids.

What these grids found: k_items took its bounds from an FMA-contracted m f_phi + n f_r, an ulp off
numpy's value at some knots, so a bin sitting on a run's end knot (or next to it) gained or lost a
whole term (0.23 max|S| on the knot-exact grids, 16 contributions off; a turning-point knot
counted into one run). The bounds now use knotF_rn (emrifd_prepare.hip), numpy's rounding.

Every source has N_t = 45 knots (41 for "nonmono"); "full" (K = 75) builds its segment table with k_segment_slots /
_compact / k_seg_tiles, "first" (its first 8 harmonics) and "nonmono" (7 modes, F with turning
points) take k_prep_pcr_b's own grouping and k_segments_one.

Tolerances -- the project's existing rules, none new:
- GPU vs the numpy oracle: max|S - R| < 1e-9 max|R| (test_gpu_modesum.py / test_gpu_edges.py),
  identical support, the oracle's contribution count, every bin finite (the output starts as
  NaN, so an unwritten bin fails);
- GPU vs the host twin: 1e-10 max|S_twin| and equal (contributions, evaluations, groups)
  (test_gpu_twin.py's small-case rule; these short sources have no fold floor at that level).
  The evaluation count changes when any lane bound moves by one bin;
- paired vs forced-unpaired kernel on symmetric grids: 1e-13 max|S|
  (test_gpu_modesum.test_paired_equals_unpaired_on_symmetric_grid);
- fused h+/hx (prepare + sum) vs efd_modesum then efd_polarizations: bitwise
  (test_gpu_modesum.test_fused_polarizations_and_two_phase_api); vs the oracle's channels:
  1e-9 of the channels' maximum (each channel is half the sum of two bins of S, so S's rule
  carries over; max|h| <= max|S| makes this the tighter reading). check_modesum_args admits any
  0 <= k0 <= nf and the epilogue keeps the bins j >= k0 whatever nf's parity, so an even-length
  grid takes k0 = searchsorted(freq, 0) = nf / 2 like any other;
- lane range: exactly the smallest lane interval holding the oracle's support;
- fused likelihood with and without tile constants: bitwise; vs efd_loglike on the written
  h+/hx of the same walker: 1e-12 relative (fused path vs template-buffer path).
"""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from emri_frequencydomainwaveforms_amd import _lib, cputwin  # noqa: E402
from emri_frequencydomainwaveforms_amd.summation import DeviceInputs, ModeSumEngine  # noqa: E402
from oracle import fd_oracle  # noqa: E402
from tests import grid_cases as gc  # noqa: E402
from tests.helpers import channels, source_inputs  # noqa: E402


def _inp(d):
    return DeviceInputs.from_host(d["t"], np.asarray(d["amp"]).T, d["phi_phi"], d["phi_r"],
                                  d["f_phi"], d["f_r"], d["m"], d["n"], d["ylm_p"], d["ylm_m"])


class _Runs:
    """Each (source, grid, caustic) spectrum of the oracle, the twin and the GPU, computed once
    and shared by the tests (never modified)."""

    def __init__(self):
        full = source_inputs(**gc.SRC)
        self.src = {"full": full, "first": gc.first_harmonics(full),
                    "nonmono": source_inputs(**gc.NONMONO)}
        self._grid, self._oracle, self._twin, self._gpu = {}, {}, {}, {}

    def grid(self, case):
        if case not in self._grid:
            self._grid[case] = gc.grid(self.src[case[0]], case[1])
        return self._grid[case]

    def oracle(self, case, caustic="uniform"):
        key = (case, caustic)
        if key not in self._oracle:
            d = self.src[case[0]]
            freq = self.grid(case)
            R = fd_oracle.fd_modesum(d["t"], np.asarray(d["amp"]), d["phi_phi"], d["phi_r"],
                                     d["f_phi"], d["f_r"], d["m"], d["n"], d["ylm_p"],
                                     d["ylm_m"], freq, float(d["prefactor"]), caustic=caustic)
            C = fd_oracle.contributions(d["t"], d["f_phi"], d["f_r"], d["m"], d["n"], freq)
            self._oracle[key] = (R, C)
        return self._oracle[key]

    def twin(self, case, caustic="uniform"):
        key = (case, caustic)
        if key not in self._twin:
            d = self.src[case[0]]
            T = cputwin.modesum(d["t"], np.ascontiguousarray(np.asarray(d["amp"]).T),
                                d["phi_phi"], d["phi_r"], d["f_phi"], d["f_r"], d["m"], d["n"],
                                d["ylm_p"], d["ylm_m"], self.grid(case), d["prefactor"],
                                caustic=caustic)
            self._twin[key] = (T, cputwin.stats())
        return self._twin[key]

    def gpu(self, case, caustic="uniform", sym=None):
        """(S, stats, contributions); paired where the grid is symmetric unless sym says
        otherwise."""
        freq_h = self.grid(case)
        sym = gc.is_symmetric(freq_h) if sym is None else sym
        key = (case, caustic, sym)
        if key not in self._gpu:
            d = self.src[case[0]]
            freq = torch.as_tensor(freq_h, device="cuda")
            out = torch.full((len(freq_h),), np.nan, dtype=torch.complex128, device="cuda")
            eng = ModeSumEngine(caustic=caustic)
            S = eng.run(_inp(d), freq, out=out, grid_symmetric=sym, scale=float(d["prefactor"]))
            self._gpu[key] = (S.cpu().numpy(), eng.stats(), eng.contributions())
        return self._gpu[key]


@pytest.fixture(scope="module")
def runs():
    return _Runs()


def _vs_oracle(runs, case, caustic):
    S, _, C = runs.gpu(case, caustic)
    R, CR = runs.oracle(case, caustic)
    assert np.all(np.isfinite(S.view(np.float64)))
    mx = np.abs(R).max()
    err = np.abs(S - R).max()
    print(f"gpu-vs-oracle {gc.case_id(case)} {caustic}: nf = {len(R)}, "
          f"err = {err / mx if mx > 0 else 0.0:.3e}")
    if mx > 0:
        assert err < 1e-9 * mx, err / mx
    else:   # no bin inside any support: exact zeros
        assert not S.any()
    assert np.array_equal(S != 0, R != 0)
    assert C == CR


def _vs_twin(runs, case, caustic):
    S, st, _ = runs.gpu(case, caustic)
    T, tst = runs.twin(case, caustic)
    mx = np.abs(T).max()
    err = np.abs(S - T).max()
    print(f"gpu-vs-twin {gc.case_id(case)} {caustic}: nf = {len(T)}, "
          f"err = {err / mx if mx > 0 else 0.0:.3e}, stats = {st}")
    assert err <= 1e-10 * mx
    assert np.array_equal(S != 0, T != 0)
    assert st == tst


# Case 1 (every grid) and case 3 (both segment paths: the "full" and "first" sources)
@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_gpu_vs_oracle(runs, case):
    assert gc.is_symmetric(runs.grid(case)) == gc.symmetric_name(case[1])
    _vs_oracle(runs, case, "uniform")


# Case 2
@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_gpu_vs_twin(runs, case):
    _vs_twin(runs, case, "uniform")


@pytest.mark.parametrize("case", gc.SPA_CASES, ids=gc.case_id)
def test_spa_caustic_mode(runs, case):
    _vs_oracle(runs, case, "spa")
    _vs_twin(runs, case, "spa")


# Case 4
@pytest.mark.parametrize("case", gc.SYMMETRIC_CASES, ids=gc.case_id)
def test_paired_equals_unpaired(runs, case):
    Sp, stp, _ = runs.gpu(case, sym=True)
    Su, stu, _ = runs.gpu(case, sym=False)
    assert np.all(np.isfinite(Su.view(np.float64)))
    assert np.abs(Sp - Su).max() <= 1e-13 * np.abs(Sp).max()
    assert np.array_equal(Sp != 0, Su != 0)
    assert stp[0] == stu[0] and stp[2] == stu[2]   # contributions and groups; a paired lane
    #                                                evaluates a branch and its partner at once


# Case 5
@pytest.mark.parametrize("case", [("full", "geom"), ("full", "knot_even"), ("full", "sym_1536"),
                                  ("full", "sym_2"), ("full", "dups")], ids=gc.case_id)
def test_fused_polarizations(runs, case):
    d = runs.src[case[0]]
    freq_h = runs.grid(case)
    nf = len(freq_h)
    inp = _inp(d)
    freq = torch.as_tensor(freq_h, device="cuda")
    eng = ModeSumEngine()
    S = eng.run(inp, freq, grid_symmetric=True, scale=float(d["prefactor"]))
    st = torch.cuda.current_stream().cuda_stream
    kz = int(np.searchsorted(freq_h, 0.0))
    assert kz == nf // 2   # the f = 0 bin, or the first positive one of an even-length grid
    R, _ = runs.oracle(case)
    for k0 in (kz, 0):
        rp = torch.empty(nf - k0, dtype=torch.complex128, device="cuda")
        rc = torch.empty_like(rp)
        _lib.check(eng.lib.efd_polarizations(torch.view_as_real(S).data_ptr(), nf, k0,
                                             torch.view_as_real(rp).data_ptr(),
                                             torch.view_as_real(rc).data_ptr(),
                                             ctypes.c_void_p(st)), "pol")
        hp = torch.full_like(rp, np.nan)
        hc = torch.full_like(rp, np.nan)
        eng.launch(inp, freq, None, True, float(d["prefactor"]), phase="prepare")
        eng.launch(inp, freq, None, True, float(d["prefactor"]), phase="sum",
                   hp=torch.view_as_real(hp), hc=torch.view_as_real(hc), k0=k0)
        assert eng.status()
        assert torch.equal(hp, rp) and torch.equal(hc, rc)
        if k0 == kz:
            ref = channels(R, freq_h)
            assert ref.shape == (2, nf - k0)
            got = np.stack([hp.cpu().numpy(), hc.cpu().numpy()])
            mx = np.abs(ref).max()
            err = np.abs(got - ref).max()
            print(f"fused h+/hx vs oracle {gc.case_id(case)}: err = {err / mx:.3e}")
            assert mx > 0 and err <= 1e-9 * mx


# Case 6
@pytest.mark.parametrize("case", [("full", g) for g in ("geom", "two_density", "outlier", "dups",
                                                        "knot_odd", "knot_even", "sym_1536")]
                         + [("first", g) for g in ("geom", "outlier", "knot_even")]
                         + [("nonmono", "knot_even")], ids=gc.case_id)
def test_lane_range(runs, case):
    d = runs.src[case[0]]
    freq_h = runs.grid(case)
    n = len(freq_h)
    freq = torch.as_tensor(freq_h, device="cuda")
    eng = ModeSumEngine()
    ws = eng.launch(_inp(d), freq, None, True, float(d["prefactor"]), phase="prepare")
    lanes = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(eng.lib.efd_modesum_lane_ranges((ctypes.c_void_p * 1)(ws.data_ptr()), 1,
                                               lanes.data_ptr(), st), "lane_ranges", eng.lib)
    assert eng.status()
    lo, hi = (int(v) for v in lanes.cpu().numpy())
    S, _, _ = runs.gpu(case)
    k = np.nonzero(S)[0]
    assert len(k) and k.min() >= min(lo, n - hi) and k.max() < max(hi, n - lo)
    # the smallest lane interval holding the oracle's support (lane l = bin l and bin n-1-l)
    R, _ = runs.oracle(case)
    lane = np.minimum(np.nonzero(R)[0], n - 1 - np.nonzero(R)[0])
    assert (lo, hi) == (int(lane.min()), int(lane.max()) + 1)


# Case 7
def test_fused_loglike_on_geometric_grid(runs):
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    from emri_frequencydomainwaveforms_amd.summation import (BatchPreparer,
                                                             loglike_tile_constants, sum_batch)
    # the first three sources of test_gpu_batch_prepare.py's list, on the geometric grid
    srcs = [runs.src["full"]] + [source_inputs(M=M, e0=e0, T=0.02, dt=20.0, eps=eps)
                                 for M, e0, eps in ((5e5, 0.2, 1e-3), (2e5, 0.5, 1e-2))]
    freq_h = runs.grid(("full", "geom"))
    freq = torch.as_tensor(freq_h, device="cuda")
    nf = len(freq_h)
    k0 = int(np.searchsorted(freq_h, 0.0))
    nb = nf - k0
    rng = np.random.default_rng(11)
    d = torch.as_tensor(rng.standard_normal((2, nb)) + 1j * rng.standard_normal((2, nb)),
                        device="cuda") * 1e-22
    w = torch.as_tensor(rng.uniform(0.5, 2.0, (2, nb)) * 1e40, device="cuda")
    w[:, 0] = 0.0   # a zeroed bin, as Likelihood's start_ind
    tc = loglike_tile_constants(d, w, nf, k0)
    B = BatchPreparer(group=len(srcs), depth=1)
    for s in srcs:
        host = {k: s[k] for k in ("t", "phi_phi", "phi_r", "f_phi", "f_r", "m", "n", "ylm_p",
                                  "ylm_m")}
        host["amp"] = np.ascontiguousarray(np.asarray(s["amp"]).T)
        B.submit(host, freq, True, s["prefactor"], k0=k0, prepare_only=True)
    gi, jobs = B.flush()
    cur = torch.cuda.current_stream()
    cur.wait_stream(B.stream(gi))
    ref = torch.empty(len(srcs), dtype=torch.float64, device="cuda")
    got = torch.empty_like(ref)
    B.sum_loglike(gi, d, w, ref, cur.cuda_stream)
    B.sum_loglike(gi, d, w, got, cur.cuda_stream, tile_const=tc)
    # the same walkers' written h+/hx, reduced by efd_loglike
    hs = [torch.full((2, nb), np.nan, dtype=torch.complex128, device="cuda") for _ in srcs]
    sum_batch([(eng, dict(kw, hp=torch.view_as_real(h[0]), hc=torch.view_as_real(h[1])))
               for (eng, kw), h in zip(jobs, hs)], stream=cur.cuda_stream)
    red = Reducer()
    tmpl = torch.cat([red.loglike(h, d, w) for h in hs])
    torch.cuda.synchronize()
    B.wait()
    assert torch.all(torch.isfinite(ref)) and torch.all(ref < 0)
    assert torch.equal(got, ref)
    a, b = ref.cpu().numpy(), tmpl.cpu().numpy()
    print(f"fused logL vs efd_loglike on the written templates: {np.abs(a - b) / np.abs(b)}")
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b))
    assert all(bool(torch.all(torch.isfinite(torch.view_as_real(h)))) and float(h.abs().max()) > 0
               for h in hs)
