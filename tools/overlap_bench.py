"""efd_overlap_rows against what the package offered before it and against the Gram kernel, at
two shapes (GPU box): config 2's full grid (pe.setup's defaults: Tobs 2 yr, 3,155,816 bins x 2
channels) and config 5's (Tobs 4 yr, downsample=100), and one whole pe.vallisneri_check.

    python tools/overlap_bench.py [--rounds R] [--reps K] [--shapes full,ds] [--out FILE.jsonl]

The parent starts the measurement as a child process under its own time limit (--limit seconds)
and starts nothing else after it. Per shape the child builds the setup, memoises the host
upstream (the timed sections are the device path, inputs resident), fills 32 rows (the 24 rows of
the six-parameter five-point stencil and 8 of them again) through generate_batch, warms every
section up once, then times R interleaved rounds with device events:
  overlap32  Reducer.overlap_rows over the 32 rows against the waveform at the truth
  inner3     the same numbers the earlier way, normalize=True's work with the weights already on
             the device: three Reducer.inner calls per row (<h|t>, <h|h>, <t|t>), no host
             synchronisation between them
  inner2     the same with <t|t> taken once: two calls per row and one more
  overlap24  Reducer.overlap_rows over the 24 stencil rows
  gram24     efd_fisher_gram over the very same 24 rows (five-point stencil, 21 products)
One JSON line per round and shape goes to --out; the summary line per shape gives the medians,
every paired round's inner3 / overlap32, inner2 / overlap32 and overlap24 / gram24, the bytes
overlap_rows reads / time beside the 8 TB/s peak and the 6.29 TB/s measured copy rate, and the
distance of the two ways' numbers. Bars (full grid only; the small grid is launch-bound and only
reported): inner3 / overlap32 >= 3 and overlap24 / gram24 <= 1.3 in every round.
The last record (shape ds) is one pe.vallisneri_check with 100 samples: total wall time and its
split into waveforms (fisher_rows), reductions (the Gram and overlap passes) and the host's rest.
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"full": dict(Tobs=2.0, dt=10.0, eps=1e-2, nwalkers=4, ntemps=1),
          "ds": dict(Tobs=4.0, dt=10.0, eps=1e-2, downsample=100, nwalkers=4, ntemps=1)}
PEAK_TBS, COPY_TBS = 8.0, 6.29
RB = 8   # efd_overlap_rows' row block: t and w are read once per block


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
    P14 = np.asarray(points + points[:8])
    nb = s.gen.num_bins
    rows = torch.empty((32, 2, nb), dtype=torch.complex128, device=dev)
    s.few.generate_batch(P14, rows, **s.kwargs)
    t = torch.stack(s.gen(*s.truth14, **s.kwargs)).contiguous()
    coef = dg.stencil_coefficients(steps, True)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = torch.stack([dg.fisher_weights(nb, f_arr=s.like.freqs, PSD=np.asarray(p))
                         for p in s.like.psd])
    w = torch.where(s.like._w > 0.0, w, torch.zeros_like(w)).contiguous()
    red = dg._reducer(dev)
    out = {}

    def overlap32():
        out["overlap"] = red.overlap_rows_flat(rows, t, None, w)

    def inner3():
        out["inner3"] = [(red.inner(rows[k], t, w), red.inner(rows[k], rows[k], w),
                          red.inner(t, t, w)) for k in range(32)]

    def inner2():
        out["inner2"] = ([(red.inner(rows[k], t, w), red.inner(rows[k], rows[k], w))
                          for k in range(32)], red.inner(t, t, w))

    def overlap24():
        out["overlap24"] = red.overlap_rows_flat(rows[:24], t, None, w)

    def gram24():
        out["gram"] = red.fisher_gram(rows[:24], coef, w, npoint)

    run = {"overlap32": overlap32, "inner3": inner3, "inner2": inner2, "overlap24": overlap24,
           "gram24": gram24}

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for fn in run.values():
        fn()
    torch.cuda.synchronize()
    rounds = []
    for r in range(args.rounds):
        row = {"shape": name, "round": r, "nbin": nb}
        for k, fn in run.items():
            row[k + "_ms"] = timed(fn, args.reps)
        rounds.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    ov = out["overlap"].cpu().numpy()
    old = np.array([[a.real.item(), b.real.item(), c.real.item()] for a, b, c in out["inner3"]])
    dist = max(float(np.max(np.abs(ov[0:-1:3] - old[:, 0]) / np.sqrt(old[:, 1] * old[:, 2]))),
               float(np.max(np.abs(ov[2:-1:3] / old[:, 1] - 1))),
               float(abs(ov[-1] / old[0, 2] - 1)))

    def nbytes(nrow):
        return 2 * nb * (16 * nrow + (16 + 8) * ((nrow + RB - 1) // RB))

    med = {k: float(np.median([r[k + "_ms"] for r in rounds])) for k in run}
    i3 = [round(r["inner3_ms"] / r["overlap32_ms"], 2) for r in rounds]
    og = [round(r["overlap24_ms"] / r["gram24_ms"], 3) for r in rounds]
    summ = {"shape": name, "setup": SHAPES[name], "nbin": nb, "rounds": args.rounds,
            "reps": args.reps, **{k + "_ms_median": v for k, v in med.items()},
            "overlap32_bytes_read": nbytes(32),
            "overlap32_TB_per_s": nbytes(32) / (med["overlap32"] * 1e-3) / 1e12,
            "overlap24_TB_per_s": nbytes(24) / (med["overlap24"] * 1e-3) / 1e12,
            "gram24_TB_per_s": 2 * nb * (16 * 24 + 8) / (med["gram24"] * 1e-3) / 1e12,
            "peak_TB_per_s": PEAK_TBS, "measured_copy_TB_per_s": COPY_TBS,
            "inner3_over_overlap32": i3,
            "inner2_over_overlap32": [round(r["inner2_ms"] / r["overlap32_ms"], 2)
                                      for r in rounds],
            "overlap24_over_gram24": og,
            "overlap_vs_inner_max_rel": dist,
            "host_upstream_memoised_s": memo.host_s}
    if name == "full":
        summ["bar_inner3_over_overlap32_ge_3"] = bool(min(i3) >= 3.0)
        summ["bar_overlap24_over_gram24_le_1.3"] = bool(max(og) <= 1.3)
    memo.remove()
    del rows, out
    torch.cuda.empty_cache()
    print(json.dumps(summ), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps({"summary": summ}) + "\n")
    if name == "ds":
        whole_check(s, steps6, args)


def whole_check(s, steps6, args):
    """One pe.vallisneri_check with 100 samples at this setup, split by synchronised wall time."""
    import torch
    from emri_frequencydomainwaveforms_amd import diagnostic as dg
    from emri_frequencydomainwaveforms_amd import pe
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    spent = {"waveforms": 0.0, "reduction": 0.0}

    def clocked(fn, key):
        def inner(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            spent[key] += time.perf_counter() - t0
            return r
        return inner

    saved = dg.fisher_rows, Reducer.overlap_rows_flat, Reducer.fisher_gram
    # steps of 0.05 / sqrt(F_ii), found by two refinements of 1e-6 |truth6| (fisher_bench's)
    steps_in = steps6
    for _ in range(2):
        Fk, _, _ = pe.fisher_covariance(s, steps6)
        steps6 = 0.05 / np.sqrt(np.diag(Fk))
    pe.vallisneri_check(s, steps6, num_samples=8, seed=1)   # warm-up
    dg.fisher_rows = clocked(saved[0], "waveforms")
    Reducer.overlap_rows_flat = clocked(saved[1], "reduction")
    Reducer.fisher_gram = clocked(saved[2], "reduction")
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r90, ratios, mism, info = pe.vallisneri_check(s, steps6, num_samples=100, seed=1)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        dg.fisher_rows, Reducer.overlap_rows_flat, Reducer.fisher_gram = saved
    rec = {"vallisneri_check": {"setup": SHAPES["ds"], "num_samples": 100, "nbin": s.gen.num_bins,
                                "total_s": total, "waveforms_s": spent["waveforms"],
                                "reduction_s": spent["reduction"],
                                "host_s": total - spent["waveforms"] - spent["reduction"],
                                "steps": np.asarray(steps6).tolist(),
                                "steps_refined_from": np.asarray(steps_in).tolist(),
                                "r_at_90": r90, "max_mismatch": float(np.max(mism)),
                                "stencil_agreement": info.get("stencil_agreement")}}
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


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
