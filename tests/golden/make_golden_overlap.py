"""Golden Vallisneri-criterion, CDF, Cutler-Vallisneri bias and scale_snr values, produced by the
reference's own code.

Run ONLY in the development container (imports Python modules from /root/reference):

    python tests/golden/make_golden_overlap.py

Imports, unchanged, from /root/reference/LISAanalysistools/lisatools/diagnostic.py: fisher
(:300-386), covariance (:389-451), mismatch_criterion (:489-644), vallisneri_criterion_cdf
(:686-757), cutler_vallisneri_bias (:760-840) and scale_snr (:843-855), and evaluates them on
the analytic toy model of tests/overlap_ref.py (scaled coordinates, so that the Fisher matrix is
well conditioned). Only inputs and outputs are written (tests/golden/overlap_golden.npz); no
reference text is stored.

Of its own it replays the seeded directions and stores the parameter offsets, asserts that at
least one sample takes the polar reflection and that the Fisher matrix's eigenvalues are
positive, and prints how far a plain float64 numpy evaluation of the same sums lies from the
reference, beside the tests' tolerances.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import overlap_ref as orf  # noqa: E402


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REF, "LISAanalysistools"))
    sys.path.insert(0, os.path.join(REF, "Eryn"))
    from lisatools.diagnostic import (covariance, cutler_vallisneri_bias, fisher,
                                      mismatch_criterion, scale_snr, snr,
                                      vallisneri_criterion_cdf)

    f, psd = orf.toy_inputs()
    model, approx = orf.toy_model(f), orf.toy_model(f, orf.APPROX_SCALE)
    T = orf.ToyTransform()
    p, eps = orf.PARAMS.copy(), orf.EPS.copy()
    ipk = dict(f_arr=f, PSD=psd)
    w = orf.weights(f, psd, 2)
    n = orf.NUM_SAMPLES

    F = fisher(model, p, eps, parameter_transforms=T, inner_product_kwargs=ipk)
    evals, evecs = np.linalg.eig(F)
    assert np.all(evals > 0.0), evals
    h_true = model(*T.transform_base_parameters(p))
    out = dict(f=f, psd=psd, params=p, eps=eps, seed=orf.SEED, fisher=F, evals=evals,
               evecs=evecs)
    print("snr", snr([h_true[0], h_true[1]], **ipk), "cond(F)", np.linalg.cond(F))

    # mismatch_criterion in a seeded loop
    np.random.seed(orf.SEED)
    pairs = np.array([mismatch_criterion(model, p, parameter_transforms=T, fish=F,
                                         eigens=(evals, evecs), inner_product_kwargs=ipk)
                      for _ in range(n)])
    out["mism"], out["ratio"] = pairs[:, 0], pairs[:, 1]
    assert np.all(np.isfinite(np.log(pairs[:, 1])))

    # the same directions, replayed
    np.random.seed(orf.SEED)
    offsets = np.zeros((n, 5))
    for k in range(n):
        u = np.random.normal(0, 1, 5)
        x = u / np.sum(u ** 2) ** (0.5)
        for l in range(5):
            offsets[k] += x[l] * evecs[:, l] / np.sqrt(evals[l])
    out["offsets"] = offsets
    pts, refl = orf.perturbed_points(p, offsets, T)
    out["reflected"] = refl
    assert refl.sum() >= 1
    print(f"{int(refl.sum())} of {n} samples reflected; |log ratio| from "
          f"{np.abs(np.log(pairs[:, 1])).min():.2e} to {np.abs(np.log(pairs[:, 1])).max():.2e}")

    # the CDF from the same seed
    np.random.seed(orf.SEED)
    r90, quant, cdf, ratios = vallisneri_criterion_cdf(
        model, p, num_samples=n, return_ratios=True, fish=F, parameter_transforms=T,
        inner_product_kwargs=ipk)
    out.update(r_at_90=r90, quantiles=quant, cdf=cdf, cdf_ratios=ratios)
    assert np.array_equal(ratios, np.abs(np.log(pairs[:, 1])))

    # Cutler-Vallisneri bias of the same model with scale = 1.001
    syst, bias, cov, dh = cutler_vallisneri_bias(
        model, approx, p, eps, parameter_transforms=T, inner_product_kwargs=ipk,
        return_cov=True, return_derivs=True)
    out.update(syst_vec=syst, bias=bias, cov=cov)
    assert np.array_equal(cov, covariance(fish=F))

    sc, snr0 = scale_snr(30.0, [h_true[0], h_true[1]], return_orig_snr=True, **ipk)
    out.update(scale_snr_orig=snr0, scale_snr_sample=np.array(sc)[:, ::64])

    # plain numpy on the same sums, beside the tests' tolerances
    rows = np.array([model(*q) for q in pts])
    over, mism, ratio = orf.criterion(orf.overlap_numpy(rows, h_true, None, w), offsets, F)
    d_mism = np.abs(mism - pairs[:, 0]).max()
    d_ratio = np.abs(ratio / pairs[:, 1] - 1).max()
    sv = orf.overlap_numpy(dh, h_true, approx(*T.transform_base_parameters(p)), w)
    dn = 4.0 * np.sum(w * np.abs(h_true - approx(*T.transform_base_parameters(p))).ravel() ** 2)
    d_syst = (np.abs(sv[0:-1:3] - syst) / np.sqrt(np.diag(F) * dn)).max()
    d_bias = (np.abs(cov @ sv[0:-1:3] - bias) / np.sqrt(np.diag(cov))).max()
    rn = float(np.interp(0.9, cdf, np.unique(np.abs(np.log(ratio)))))
    print(f"numpy vs reference: mism {d_mism:.2e} (bound 1e-11), ratio {d_ratio:.2e} rel "
          f"(1e-11), r_at_90 {abs(rn / r90 - 1):.2e} rel (1e-11), syst_vec {d_syst:.2e} of "
          f"sqrt(F_kk |dh|^2) (1e-11), bias {d_bias:.2e} of sqrt(cov_kk) (1e-9)")

    np.savez_compressed(os.path.join(HERE, "overlap_golden.npz"), **out)
    for k, v in out.items():
        v = np.asarray(v)
        print(k, v.shape, v.dtype, v.ravel()[:2])


if __name__ == "__main__":
    main()
