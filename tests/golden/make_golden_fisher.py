"""Golden Fisher matrices and covariance, produced by the reference's own code.

Run ONLY in the development container (imports Python modules from /root/reference):

    python tests/golden/make_golden_fisher.py

Imports, unchanged, from /root/reference/LISAanalysistools/lisatools/diagnostic.py: fisher
(:300-386, through dh_dlambda :207-297 and inner_product :14-157) and covariance (:389-451), and
evaluates them on an analytic toy model. Only inputs and outputs are written
(tests/golden/fisher_golden.npz); no reference text is stored.

It also prints, normalised by sqrt(F_ii F_jj), how far two ways of forming the same matrix in
float64 numpy are from the reference: the stencil per bin first (what efd_fisher_gram does) and
the Gram matrix of the raw stencil spectra combined afterwards (the shortcut it must not take).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

STENCILS = {True: ((2.0, 1.0, -1.0, -2.0), (-1.0 / 12, 8.0 / 12, -8.0 / 12, 1.0 / 12)),
            False: ((1.0, -1.0), (0.5, -0.5))}


def toy_inputs():
    f = np.linspace(1e-4, 1e-2, 4098)[1:]
    psd = 1e-40 * (1.0 + (2e-3 / f) ** 4 + (f / 5e-3) ** 2)
    p = np.array([np.log(1e-20), 3e-3, 2e3, 0.3])
    eps = np.array([1e-3, 1e-7, 1e-1, 1e-3])
    return f, psd, p, eps


def toy_model(f):
    def model(lnA, f0, tau, phi):
        env = np.exp(lnA) * np.exp(-0.5 * ((f - f0) * tau) ** 2)
        ph = np.exp(1j * (2 * np.pi * f * tau + phi))
        return np.array([env * ph, 0.5j * env * ph * (1 + 0.1 * f / f0)])
    return model


def stencil_rows(model, p, eps, inds, accuracy):
    """(rows [P npoint][2][nbin], coef [P][npoint]) for parameters inds with steps eps."""
    offs, wts = STENCILS[accuracy]
    rows, coef = [], []
    for i, e in zip(inds, eps):
        for o in offs:
            q = p.copy()
            q[i] += o * e
            rows.append(model(*q))
        coef.append(np.asarray(wts) / e)
    return np.array(rows), np.array(coef)


def weights(f, psd):
    x = np.empty_like(f)
    x[1:] = np.diff(f)
    x[0] = x[1]
    return x / psd


def rel(a, ref):
    d = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(a - ref) / np.outer(d, d)))


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REF, "LISAanalysistools"))
    sys.path.insert(0, os.path.join(REF, "Eryn"))
    from lisatools.diagnostic import covariance, fisher

    f, psd, p, eps = toy_inputs()
    model = toy_model(f)
    w = weights(f, psd)
    ipk = dict(f_arr=f, PSD=psd)
    out = dict(f=f, psd=psd, params=p, eps=eps)
    for scale, tag in ((1.0, "base"), (1e-3, "small")):
        for acc, name in ((True, "5"), (False, "3")):
            e = eps * scale
            F, dh = fisher(model, p, e, inner_product_kwargs=ipk, return_derivs=True,
                           accuracy=acc)
            out[f"fisher{name}_{tag}"] = F
            if scale == 1.0 and acc:
                out["dh5_base_row2"] = dh[2]
            rows, coef = stencil_rows(model, p, e, range(4), acc)
            P, npt = coef.shape
            R = rows.reshape(P, npt, -1)
            D = np.einsum("is,ise->ie", coef, R)
            per_bin = 4.0 * np.real(np.einsum("ie,je,e->ij", D.conj(), D, np.tile(w, 2)))
            Rf = R.reshape(P * npt, -1)
            G = 4.0 * np.real(np.einsum("ae,be,e->ab", Rf.conj(), Rf, np.tile(w, 2)))
            C = np.zeros((P, P * npt))
            for i in range(P):
                C[i, i * npt:(i + 1) * npt] = coef[i]
            raw = C @ G @ C.T
            print(f"{tag} steps, {name}-point: per-bin vs reference {rel(per_bin, F):.2e}, "
                  f"Gram of raw rows vs reference {rel(raw, F):.2e}")
    inds = [2, 0]
    e2 = np.array([3e-2, 2e-3])   # eps[k] goes with inds[k] by position
    out["sub_inds"] = np.array(inds)
    out["sub_eps"] = e2
    out["fisher5_sub"] = fisher(model, p, e2, deriv_inds=inds, inner_product_kwargs=ipk)
    out["cov5_base"] = covariance(fish=out["fisher5_base"])
    np.savez_compressed(os.path.join(HERE, "fisher_golden.npz"), **out)
    for k, v in out.items():
        v = np.asarray(v)
        print(k, v.shape, v.dtype, v.ravel()[:2])


if __name__ == "__main__":
    main()
