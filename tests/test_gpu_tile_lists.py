"""The tile's record list has two builds, and they must agree: k_tile_keys writes it in the
preparation phase (waveforms of at least LISTS_MIN_K = 1024 harmonics), modesum_tile builds it
in the sum (fewer harmonics, or a tile whose list k_tile_keys gave up on: more than KEYCAP
records or TK_HITS segments). Both write the same keys in the same order, so one waveform sent
through either gives the same spectrum to the last bit.

EFD_LISTS_MIN_K moves the threshold and is read once per process, so each setting runs in a
child process of its own:
- source A (1,049 harmonics in 280 (m, n) groups: more than one SEGWIN window of segments) with
  the default threshold (prebuilt lists) and with EFD_LISTS_MIN_K=1000000 (built in the sum);
- source B (75 harmonics) with the default (built in the sum) and with EFD_LISTS_MIN_K=1
  (prebuilt).
Grids: the source's own symmetric grid in both caustic modes, the same grid unpaired, and for A a
coarse symmetric grid of 799 bins: all of A's 34,617 records in one tile, more than KEYCAP, so
k_tile_keys answers tcnt = -1 and the sum builds that list over several passes in either child.

The children's spectra must be equal as raw float64 words, and the default one within RTOL of
the oracle (test_gpu_modesum.py's bound), so that two equal wrong answers do not pass. Which
build a child used is not visible from outside (tcnt is not exported): that rests on the
threshold logic of lists_min_k() / list_mode().
"""

import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import fd_oracle  # noqa: E402
from tests.helpers import source_inputs  # noqa: E402

RTOL = 1e-9
KEYCAP = 2048
INPUT_KEYS = ("t", "amp", "phi_phi", "phi_r", "f_phi", "f_r", "m", "n", "ylm_p", "ylm_m")

# (case, source, grid, caustic, grid_symmetric)
CASES = [("A-uniform", "A", "own", "uniform", True), ("A-spa", "A", "own", "spa", True),
         ("A-unpaired", "A", "own", "uniform", False),
         ("A-coarse", "A", "coarse", "uniform", True),
         ("B-uniform", "B", "own", "uniform", True), ("B-spa", "B", "own", "spa", True),
         ("B-unpaired", "B", "own", "uniform", False)]
CASE_IDS = [c[0] for c in CASES]

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
from emri_frequencydomainwaveforms_amd.summation import DeviceInputs, ModeSumEngine
z = np.load(sys.argv[2])
out = {}
for spec in sys.argv[4:]:
    case, src, grid, caustic, sym = spec.split(",")
    inp = DeviceInputs.from_host(*(z[f"{src}_{k}"] for k in ("t", "amp_t", "phi_phi", "phi_r",
                                                              "f_phi", "f_r", "m", "n", "ylm_p",
                                                              "ylm_m")))
    freq = torch.as_tensor(z[f"{src}_freq_{grid}"], device="cuda")
    eng = ModeSumEngine(caustic=caustic)
    S = eng.run(inp, freq, grid_symmetric=sym == "1", scale=float(z[f"{src}_prefactor"]))
    assert eng.status()
    out[case] = S.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def _run_child(root, inputs, out, cases, lists_min_k):
    env = dict(os.environ)
    env.pop("EFD_LISTS_MIN_K", None)
    if lists_min_k is not None:
        env["EFD_LISTS_MIN_K"] = str(lists_min_k)
    specs = [f"{c},{s},{g},{ca},{int(sym)}" for c, s, g, ca, sym in cases]
    r = subprocess.run([sys.executable, "-c", _CHILD, root, inputs, out, *specs],
                       capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def sources():
    A = source_inputs(M=3e5, mu=10.0, e0=0.35, T=0.01, dt=20.0, eps=1e-3)
    B = source_inputs(M=3e5, mu=10.0, e0=0.35, T=0.02, dt=20.0, eps=1e-2)
    p_freq = np.linspace(0.0, A["freq"].max(), 400)
    A["freq_coarse"] = np.hstack((-p_freq[::-1][:-1], p_freq))   # 799 bins: one tile
    return {"A": A, "B": B}


@pytest.fixture(scope="module")
def builds(sources, tmp_path_factory):
    """{"default" | "other": {case: spectrum}}: every case under the default threshold, and
    under the one that sends its source through the other build."""
    tmp = tmp_path_factory.mktemp("tile_lists")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = {}
    for s, d in sources.items():
        for k in INPUT_KEYS:
            z[f"{s}_{k}"] = np.asarray(d[k])
        z[f"{s}_amp_t"] = np.ascontiguousarray(np.asarray(d["amp"]).T)
        z[f"{s}_freq_own"] = d["freq"]
        z[f"{s}_prefactor"] = float(d["prefactor"])
    z["A_freq_coarse"] = sources["A"]["freq_coarse"]
    inputs = str(tmp / "inputs.npz")
    np.savez(inputs, **z)
    a_cases = [c for c in CASES if c[1] == "A"]
    b_cases = [c for c in CASES if c[1] == "B"]
    default = _run_child(root, inputs, str(tmp / "default.npz"), CASES, None)
    other = _run_child(root, inputs, str(tmp / "a_in_sum.npz"), a_cases, 1000000)
    other.update(_run_child(root, inputs, str(tmp / "b_prebuilt.npz"), b_cases, 1))
    return {"default": default, "other": other}


@pytest.fixture(scope="module")
def oracle(sources):
    """The oracle's spectrum per (source, grid, caustic): the unpaired case shares the paired's."""
    ref = {}

    def get(src, grid, caustic):
        if (src, grid, caustic) not in ref:
            d = sources[src]
            freq = d["freq"] if grid == "own" else d[f"freq_{grid}"]
            ref[src, grid, caustic] = fd_oracle.fd_modesum(
                d["t"], np.asarray(d["amp"]), d["phi_phi"], d["phi_r"], d["f_phi"], d["f_r"],
                d["m"], d["n"], d["ylm_p"], d["ylm_m"], freq, float(d["prefactor"]),
                caustic=caustic)
        return ref[src, grid, caustic]
    return get


def test_sources_reach_both_builds(sources):
    A, B = sources["A"], sources["B"]
    # A: prebuilt lists by default, and more than one SEGWIN = 256 window of segments (every
    # (m, n) group has at least one segment per sub-branch; the count itself is on the device)
    assert len(A["m"]) >= 1024
    assert len(set(zip(A["m"].tolist(), A["n"].tolist()))) > 128
    # the coarse grid's single tile holds more records than two KEYCAP passes
    assert len(A["freq_coarse"]) == 799
    assert len(A["m"]) * (len(A["t"]) - 1) > 2 * KEYCAP
    # B: built in the sum by default
    assert len(B["m"]) < 1024


@pytest.mark.parametrize("case", CASE_IDS)
def test_two_builds_agree_bitwise(builds, case):
    a, b = builds["default"][case], builds["other"][case]
    assert a.dtype == np.complex128 and a.shape == b.shape and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.float64), b.view(np.float64))


@pytest.mark.parametrize("case,src,grid,caustic,sym", CASES, ids=CASE_IDS)
def test_default_build_matches_oracle(builds, oracle, case, src, grid, caustic, sym):
    S, R = builds["default"][case], oracle(src, grid, caustic)
    err = np.abs(S - R).max() / np.abs(R).max()
    print(f"{case}: max|S - R| / max|R| = {err:.3e}")
    assert err < RTOL
