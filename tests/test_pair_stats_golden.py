"""diagnostic.pair_statistics against lisatools' own inner_product in the mode-by-mode driver's
sequence (tests/golden/pair_golden.npz: SNR, check_mode_by_mode.py:292; Mism, :299; logl,
:313-317; three seeded two-channel pairs over a non-uniform f_arr with an array PSD, at mismatch
about 0.3, about 1e-6 and identical). Without a GPU the CPU twin's numbers go through
PairStatistics (the arithmetic pair_statistics applies to the kernel's); a gpu-marked case runs
pair_statistics itself.

Tolerances: SNR and logl 1e-12 relative, mismatch 1e-12 absolute (the reference's 1 - x carries
no more); a plain numpy evaluation lies 0, 2e-16 and 0 from the reference
(make_golden_pair.py's print)."""

import os

import numpy as np
import pytest

from tests import overlap_ref as orf
from tests import pair_stats_ref as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def check(stats, g):
    print("SNR rel", np.abs(stats.snr1 / g["SNR"] - 1).max(), "Mism abs",
          np.abs(stats.mismatch - g["Mism"]).max(), "logl", stats.loglike, g["logl"])
    assert np.all(np.abs(stats.snr1 - g["SNR"]) <= 1e-12 * g["SNR"])
    assert np.all(np.abs(stats.mismatch - g["Mism"]) <= 1e-12)
    assert np.all(np.abs(stats.loglike - g["logl"]) <= 1e-12 * np.abs(g["logl"]))
    assert 0.2 < g["Mism"][0] < 0.4 and 5e-7 < g["Mism"][1] < 2e-6
    assert stats.mismatch[2] == 0.0 and stats.loglike[2] == 0.0       # the identical pair
    assert np.all(stats.ab_sum.imag[2] == 0.0) and stats.snr1[2] == stats.snr2[2]


def test_twin_arithmetic_matches_reference(gold):
    from emri_frequencydomainwaveforms_amd.diagnostic import PairStatistics
    nbin = gold["f"].size
    w = orf.weights(gold["f"], gold["psd"], 1)
    rc, raw = pr.pair_cpu(gold["sig1"].reshape(3, -1), gold["sig2"].reshape(3, -1), w, 2, nbin)
    assert rc == 0
    stats = PairStatistics(raw)
    check(stats, gold)
    # the same pair's log-likelihood from aa + bb - 2 ab, beside dd's: why dd is its own output
    alg = -0.5 * (stats.aa_sum + stats.bb_sum - 2.0 * stats.ab_sum.real)
    print("logl from aa + bb - 2 ab, rel err", np.abs(alg[:2] / gold["logl"][:2] - 1))


@pytest.mark.gpu
def test_pair_statistics_matches_reference(gold):
    pytest.importorskip("torch")
    from emri_frequencydomainwaveforms_amd.diagnostic import inner_product, pair_statistics
    kw = dict(f_arr=gold["f"], PSD=gold["psd"])
    stats = pair_statistics(gold["sig1"], gold["sig2"], **kw)
    check(stats, gold)
    lists = pair_statistics([[r[0], r[1]] for r in gold["sig1"]],
                            [[r[0], r[1]] for r in gold["sig2"]], **kw)
    assert pr.same_bits(lists.raw, stats.raw)
    # and against this package's inner_product, pair by pair (1e-12 of sqrt(aa bb))
    for r in range(3):
        s1, s2 = list(gold["sig1"][r]), list(gold["sig2"][r])
        ip = inner_product(s1, s2, complex=True, **kw)
        assert abs(ip - stats.ab_sum[r]) <= 1e-12 * stats.snr1[r] * stats.snr2[r]
    with pytest.raises(ValueError, match="Must provide either df, dt or f_arr"):
        pair_statistics(gold["sig1"], gold["sig2"], PSD=gold["psd"])
    with pytest.raises(ValueError, match="channels"):
        pair_statistics(gold["sig1"], gold["sig2"][:, :1], **kw)
    with pytest.raises(TypeError):
        pair_statistics(gold["sig1"], gold["sig2"], f_arr=gold["f"], PSD=None)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dt", "df"])
def test_pair_statistics_takes_inner_products_grids(mode):
    """dt (time-domain rows through rfft, the DC bin dropped) and df, with a named PSD: the same
    numbers as inner_product pair by pair, to the inner-product tolerance."""
    pytest.importorskip("torch")
    from emri_frequencydomainwaveforms_amd.diagnostic import inner_product, pair_statistics
    rng = np.random.default_rng(7)
    if mode == "dt":
        s1, s2 = rng.normal(size=(3, 2, 1024)), rng.normal(size=(3, 2, 1024))
        kw = dict(dt=10.0, PSD="cornish_lisa_psd")
    else:
        s1 = rng.normal(size=(3, 1, 500)) + 1j * rng.normal(size=(3, 1, 500))
        s2 = s1 + 0.1 * rng.normal(size=(3, 1, 500))
        kw = dict(df=1e-5, PSD="cornish_lisa_psd")
    stats = pair_statistics(s1, s2, **kw)
    for r in range(3):
        aa = inner_product(list(s1[r]), list(s1[r]), **kw)
        bb = inner_product(list(s2[r]), list(s2[r]), **kw)
        ab = inner_product(list(s1[r]), list(s2[r]), complex=True, **kw)
        dd = inner_product(list(s1[r] - s2[r]), list(s1[r] - s2[r]), **kw)
        assert abs(stats.aa_sum[r] - aa) <= 1e-12 * aa and abs(stats.bb_sum[r] - bb) <= 1e-12 * bb
        assert abs(stats.ab_sum[r] - ab) <= 1e-12 * np.sqrt(aa * bb)
        # the difference is formed before the transform there and after it here: 1e-12 of the
        # operands' norms
        assert abs(stats.dd_sum[r] - dd) <= 1e-12 * (aa + bb)
        assert abs(stats.loglike[r] + 0.5 * dd) <= 1e-12 * (aa + bb)
