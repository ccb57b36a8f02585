"""The Fisher matrix's device path against what the package offered before it, at two shapes
(GPU box): config 2's full grid (pe.setup's defaults: Tobs 2 yr, 3,155,816 bins x 2 channels)
and config 5's (Tobs 4 yr, downsample=100). P = 6 sampled coordinates, five-point stencil.

    python tools/fisher_bench.py [--rounds R] [--reps K] [--shapes full,ds] [--out FILE.jsonl]

The parent starts the measurement as a child process under its own time limit (--limit seconds)
and starts nothing else after it. Per shape the child builds the setup, memoises the host
upstream (the timed sections are the device path, inputs resident), warms every section up
once, then times R interleaved rounds with device events:
  waveforms  the 24 stencil rows through GenerateEMRIWaveform.generate_batch
  gram       efd_fisher_gram on those rows (Reducer.fisher_gram: stencil, 21 products, mirror)
  pairwise   the same matrix from the same rows with the earlier pieces: the derivatives by torch
             ops, then diagnostic.inner_product for each of the 21 pairs (weights and PSD given
             as device tensors; each call expands the weights, launches twice and ends in .item())
One JSON line per round and shape goes to --out; the summary line per shape gives the medians,
gram's bytes read / time beside the 8 TB/s peak and the 6.29 TB/s measured copy rate, the
pairwise / gram ratio of every paired round, the two matrices' distance, and (full grid only,
not gated) -logL(truth6 + s v) / (s^2 / 2) for s = 1e-2 along the unit-Fisher-norm
eigen-directions v: 1 where the likelihood is the quadratic the covariance stands for. That
record is made twice, with the timed steps and with steps of 0.05 / sqrt(F_ii), each beside
pe.fisher_covariance's stencil_agreement.
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"full": dict(Tobs=2.0, dt=10.0, eps=1e-2, nwalkers=4, ntemps=1),
          "ds": dict(Tobs=4.0, dt=10.0, eps=1e-2, downsample=100, nwalkers=4, ntemps=1)}
PEAK_TBS, COPY_TBS = 8.0, 6.29


def measure(name, args):
    import torch
    from emri_frequencydomainwaveforms_amd import diagnostic as dg
    from emri_frequencydomainwaveforms_amd import pe
    s = pe.setup(**SHAPES[name])
    memo = pe.MemoizedUpstream(s.few.waveform_generator)
    dev = torch.device("cuda", torch.cuda.current_device())
    steps6 = np.where(s.truth6 != 0.0, 1e-6 * np.abs(s.truth6), 1e-6)
    steps, points, npoint = dg._fisher_points(s.truth6, steps6, None,
                                              pe._SampledToWaveform(s.transform), True)
    P14 = np.asarray(points)
    nb = s.gen.num_bins
    rows = torch.empty((len(points), 2, nb), dtype=torch.complex128, device=dev)
    coef = dg.stencil_coefficients(steps, True)
    coef_t = torch.as_tensor(coef, device=dev)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = torch.stack([dg.fisher_weights(nb, f_arr=s.like.freqs, PSD=np.asarray(p))
                         for p in s.like.psd])
    w = torch.where(s.like._w > 0.0, w, torch.zeros_like(w)).contiguous()
    red = dg._reducer(dev)
    f_dev = s.like.freqs
    psd_dev = torch.as_tensor(np.asarray(s.like.psd[0]), device=dev).clone()
    psd_dev[w[0] == 0.0] = float("inf")     # the bins the likelihood drops: zero weight
    out = {}

    def waveforms():
        s.few.generate_batch(P14, rows, **s.kwargs)

    def gram():
        out["gram"] = red.fisher_gram(rows, coef, w, npoint)

    def pairwise():
        D = (rows.view(6, npoint, 2, nb) * coef_t[:, :, None, None]).sum(1)
        F = np.zeros((6, 6))
        for i in range(6):
            for j in range(i, 6):
                F[i, j] = F[j, i] = dg.inner_product([D[i, 0], D[i, 1]], [D[j, 0], D[j, 1]],
                                                     f_arr=f_dev, PSD=psd_dev)
        out["pairwise"] = F

    run = {"waveforms": waveforms, "gram": gram, "pairwise": pairwise}

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for fn in run.values():   # warm-up (waveforms first: it fills the rows)
        fn()
    torch.cuda.synchronize()
    rounds = []
    for r in range(args.rounds):
        row = {"shape": name, "round": r, "nbin": nb, "rows": len(points)}
        for k, fn in run.items():
            row[k + "_ms"] = timed(fn, 1 if k == "pairwise" else args.reps)
        rounds.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    F = out["gram"].cpu().numpy()
    d = np.sqrt(np.diag(F))
    nbytes = rows.numel() * 16 + w.numel() * 8
    med = {k: float(np.median([r[k + "_ms"] for r in rounds])) for k in run}
    summ = {"shape": name, "setup": SHAPES[name], "nbin": nb, "rows": len(points),
            "rounds": args.rounds, "reps": args.reps,
            **{k + "_ms_median": v for k, v in med.items()},
            "gram_bytes_read": nbytes,
            "gram_TB_per_s": nbytes / (med["gram"] * 1e-3) / 1e12,
            "peak_TB_per_s": PEAK_TBS, "measured_copy_TB_per_s": COPY_TBS,
            "pairwise_over_gram": [round(r["pairwise_ms"] / r["gram_ms"], 2) for r in rounds],
            "gram_vs_pairwise_max_rel": float(np.max(np.abs(F - out["pairwise"])
                                                     / np.outer(d, d))),
            "fisher_diag": np.diag(F).tolist(),
            "host_upstream_memoised_s": memo.host_s}
    if name == "full":
        # the nonlinearity a user of the covariance should know about (recorded, not gated)
        # with the timed steps (1e-6 |truth6|, several sigma in the mass coordinates at this
        # length) and with steps of 0.05 / sqrt(F_ii) found by two refinements of them
        def nonlinearity(st):
            Fk, _, info = pe.fisher_covariance(s, st)
            lam, U = np.linalg.eigh(Fk)
            sc, ratios = 1e-2, []
            for k in range(6):
                if lam[k] <= 0.0:
                    ratios.append(None)
                    continue
                v = U[:, k] / np.sqrt(lam[k])
                p14 = s.transform.both_transforms((s.truth6 + sc * v)[None, :])
                ll = float(np.asarray(s.like.get_ll(p14, **s.kwargs))[0])
                ratios.append(-ll / (0.5 * sc * sc))
            return Fk, {"steps": np.asarray(st).tolist(), "fisher_diag": np.diag(Fk).tolist(),
                        "fisher_eigenvalues": lam.tolist(),
                        "stencil_agreement": info["stencil_agreement"],
                        "neg_logL_over_quadratic_s1e-2": ratios}
        Fa, rec_a = nonlinearity(steps6)
        Fb, _ = nonlinearity(0.05 / np.sqrt(np.diag(Fa)))
        _, rec_c = nonlinearity(0.05 / np.sqrt(np.diag(Fb)))
        summ["nonlinearity_steps_1e-6_truth"] = rec_a
        summ["nonlinearity_steps_0.05_sigma"] = rec_c
    memo.remove()
    print(json.dumps(summ), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps({"summary": summ}) + "\n")


def child(args):
    for name in args.shapes.split(","):
        measure(name, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="full,ds")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=400, help="the child's time limit [s]")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
