"""Golden SNR, mismatch and log-likelihood values of template pairs, produced by the reference's
own inner product in the mode-by-mode driver's sequence.

Run ONLY in the development container (imports Python modules from /root/reference):

    python tests/golden/make_golden_pair.py

Imports, unchanged, from /root/reference/LISAanalysistools/lisatools/diagnostic.py: inner_product
(:14-157), and runs the sequence of /root/reference/check_mode_by_mode.py on seeded two-channel
pairs over a non-uniform f_arr with an array PSD: SNR (:292), Mism (:299) and logl (:313-317).
Three pairs: mismatch about 0.3, about 1e-6, and an identical pair. Only inputs and outputs are
written (tests/golden/pair_golden.npz); no reference text is stored.

Of its own it prints how far a plain float64 numpy evaluation of the same sums lies from the
reference, beside the tests' tolerances (SNR and logl 1e-12 relative, mismatch 1e-12 absolute:
the reference's 1 - x carries no more).
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 31337
NBIN = 1201


def inputs():
    rng = np.random.default_rng(SEED)
    f = np.cumsum(rng.uniform(1.2e-6, 7.5e-6, size=NBIN)) + 1e-4      # a non-uniform grid
    psd = 1e-40 * (1.0 + (2e-3 / f) ** 4 + (f / 5e-3) ** 2)
    env = 1e-19 * np.exp(-0.5 * ((f - 3e-3) / 1.5e-3) ** 2)
    a = np.stack([env * np.exp(2j * np.pi * f * 900.0),
                  0.7j * env * np.exp(2j * np.pi * f * 900.0) * (1 + 40.0 * f)])
    noise = rng.normal(size=(2, NBIN)) + 1j * rng.normal(size=(2, NBIN))
    b_far = a * np.exp(0.6j) + 0.5 * env * noise                     # mismatch about 0.3
    b_near = a * (1.0 + 2.1e-3 * np.cos(2e3 * f) * np.exp(0.3j))     # mismatch about 1e-6
    sig1 = np.stack([a, a, a])
    sig2 = np.stack([b_far, b_near, a.copy()])
    return f, psd, sig1, sig2


def main():
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, os.path.join(REF, "LISAanalysistools"))
    sys.path.insert(0, os.path.join(REF, "Eryn"))
    from lisatools.diagnostic import inner_product

    f, psd, sig1, sig2 = inputs()
    kw = dict(PSD=psd, use_gpu=False, f_arr=f)
    snr, mism, logl = [], [], []
    for s1, s2 in zip(sig1, sig2):
        sig_fd, sig_td = [s1[0], s1[1]], [s2[0], s2[1]]
        snr.append(np.sqrt(float(inner_product(sig_fd, sig_fd, **kw))))                 # :292
        mism.append(np.abs(1 - inner_product(sig_fd, sig_td, normalize=True, **kw)))    # :299
        sig_inner = [sig_fd[0] - sig_td[0], sig_fd[1] - sig_td[1]]                      # :313
        logl.append(-0.5 * sum([inner_product(el, el, normalize=False, **kw)
                                for el in sig_inner]))                                  # :315
    out = dict(f=f, psd=psd, sig1=sig1, sig2=sig2, SNR=np.array(snr), Mism=np.array(mism),
               logl=np.array(logl))
    print("SNR", out["SNR"], "Mism", out["Mism"], "logl", out["logl"])
    assert 0.2 < out["Mism"][0] < 0.4 and 5e-7 < out["Mism"][1] < 2e-6 and out["Mism"][2] == 0.0

    # plain numpy on the same sums, beside the tests' tolerances
    x = np.empty_like(f)
    x[1:] = np.diff(f)
    x[0] = x[1]
    w = x / psd
    aa = 4.0 * np.sum(w * np.abs(sig1) ** 2, axis=(1, 2))
    bb = 4.0 * np.sum(w * np.abs(sig2) ** 2, axis=(1, 2))
    ab = 4.0 * np.sum(w * (np.conj(sig1) * sig2).real, axis=(1, 2))
    dd = 4.0 * np.sum(w * np.abs(sig1 - sig2) ** 2, axis=(1, 2))
    ok = out["logl"] != 0.0
    print(f"numpy vs reference: SNR {np.abs(np.sqrt(aa) / out['SNR'] - 1).max():.2e} rel (bound "
          f"1e-12), Mism {np.abs(np.abs(1 - ab / np.sqrt(aa * bb)) - out['Mism']).max():.2e} "
          f"(1e-12), logl {np.abs(-0.5 * dd[ok] / out['logl'][ok] - 1).max():.2e} rel (1e-12); "
          f"identical pair: logl {out['logl'][2]!r}")

    np.savez_compressed(os.path.join(HERE, "pair_golden.npz"), **out)
    for k, v in out.items():
        v = np.asarray(v)
        print(k, v.shape, v.dtype, v.ravel()[:2])


if __name__ == "__main__":
    main()
