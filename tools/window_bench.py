"""The cosine-sum windows' device path against the exact transform pair and against the Hann
path, at test.sh's shape (Tobs 4 yr, 12,623,261 bins, a half-step of 8 walkers) (GPU box).

    python tools/window_bench.py [--rounds R] [--reps K] [--window nuttall] [--out FILE.jsonl]
    python tools/window_bench.py --only cosw_loglike      (one section, for a counters pass)

The parent starts the measurement as a child process under its own time limit (--limit
seconds) and starts nothing else after it. The child makes the 8 walkers' spectra once (resident;
the mode sum is not timed), warms every section up once, then times R interleaved rounds of
  dft          windowed_spectrum (a size-N complex128 torch.fft pair) + polarizations per walker:
               what every window but Hann took before CosineWindowConvolution
  cosw_fill    CosineWindowConvolution.polarizations_batch (transforms + efd_cosw_polarizations)
  cosw_loglike CosineWindowConvolution.loglike_batch (transforms + efd_cosw_loglike)
  hann_fill    HannConvolution.polarizations_batch on the same spectra
  hann_loglike HannConvolution.loglike_batch (the pair form, efd_hann_loglike)
  extent_transform  the part the last four share (efd_hann_extent + efd_hann_convolve)
with device events (ms per call over K back-to-back calls; dft: one call per round). One JSON
line per round goes to --out, and a summary line (medians, the ratio of every paired round, the
new path's distance from the transform pair) to stdout.
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("dft", "cosw_fill", "cosw_loglike", "hann_fill", "hann_loglike", "extent_transform")


def child(args):
    import torch
    from emri_frequencydomainwaveforms_amd import _lib, pe
    from emri_frequencydomainwaveforms_amd.fdutils import (COSINE_WINDOWS, HannConvolution,
                                                           windowed_spectrum)
    s = pe.setup(Tobs=4.0, dt=10.0, eps=1e-2, M=3670041.7362535275, mu=292.0583167470244,
                 e0=0.5794130830706371, nwalkers=16, ntemps=1, window=args.window)
    gen, like = s.gen, s.like
    n = s.info["N_f"]
    lib = _lib.load()
    params14 = s.transform.both_transforms(s.half_steps()[0])
    B = len(params14)
    S, cw, single, lanes = gen._spectra(params14, **s.kwargs)
    support = gen._lane_support(S, lanes)
    gen._status(cw, single)
    S = S.clone()
    lanes = None if lanes is None else lanes.clone()
    k0 = gen._suffix_k0
    nb = n - k0
    cosw, hann = gen._cosw, HannConvolution(n, S.device)
    d, w = like._d, like._w_templ
    outs = torch.empty((B, 2, nb), dtype=torch.complex128, device=S.device)
    pairs = [(outs[i, 0], outs[i, 1]) for i in range(B)]
    ll = torch.empty(B, dtype=torch.float64, device=S.device)
    scr = torch.empty(B * _lib.EFD_LOGLIKE_SCRATCH, dtype=torch.float64, device=S.device)

    def dft():
        for i in range(B):
            cw.polarizations(windowed_spectrum(S[i], gen._mult), True, out=pairs[i])

    run = {
        "dft": dft,
        "cosw_fill": lambda: cosw.polarizations_batch(S, pairs, k0, lib, lanes, support),
        "cosw_loglike": lambda: cosw.loglike_batch(S, d, w, k0, ll, scr, lib, lanes, support),
        "hann_fill": lambda: hann.polarizations_batch(S, pairs, k0, lib, lanes, support),
        "hann_loglike": lambda: hann.loglike_batch(S, d, w, k0, ll, scr, lib, lanes, support),
        "extent_transform": lambda: cosw.transform(S, lib, lanes, support),
    }
    todo = [args.only] if args.only else list(SECTIONS)

    def timed(name, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            run[name]()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    # what the new path computes against the transform pair, at this shape
    check = {}
    if not args.only:
        run["dft"]()
        exact = outs.clone()
        run["cosw_fill"]()
        mx = S.abs().amax(dim=1)
        err = (outs - exact).abs().amax(dim=(1, 2)) / mx
        check = {"fill_vs_dft_max_err_over_maxS": float(err.max()),
                 "m": int(cosw.transform(S, lib, lanes, support)[2]), "support_bound": support}
        del exact
    for name in todo:      # warm-up: every section once
        run[name]()
    torch.cuda.synchronize()
    rows = []
    for r in range(args.rounds):
        row = {"round": r, "window": args.window, "N_f": n, "walkers": B}
        for name in todo:
            row[name + "_ms"] = timed(name, 1 if name == "dft" else args.reps)
        rows.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    summ = {"window": args.window, "coeffs": COSINE_WINDOWS[args.window], "N_f": n, "walkers": B,
            "rounds": args.rounds, "reps": args.reps, **check}
    for name in todo:
        summ[name + "_ms_median"] = float(np.median([r[name + "_ms"] for r in rows]))
    if not args.only:
        for name in ("cosw_fill", "cosw_loglike"):
            ratios = [r["dft_ms"] / r[name + "_ms"] for r in rows]
            summ["dft_over_" + name] = [round(x, 2) for x in ratios]
        summ["cosw_over_hann_loglike"] = [round(r["cosw_loglike_ms"] / r["hann_loglike_ms"], 3)
                                          for r in rows]
        summ["cosw_over_hann_fill"] = [round(r["cosw_fill_ms"] / r["hann_fill_ms"], 3)
                                       for r in rows]
    print(json.dumps(summ))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", default="nuttall")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=SECTIONS, default=None)
    ap.add_argument("--limit", type=int, default=300, help="the child's time limit [s]")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
