"""The TD-template likelihood's batched route against the per-walker route it replaces, at the
reference driver's shapes (GPU box).

    python tools/td_likelihood_bench.py [--rounds R] [--shapes t,t_hann,c4] [--out FILE.jsonl]

  t       emri_pe.py:7: Tobs 4 yr, dt 10 s, eps 1e-2, 16 walkers, -template td (N = 12.6 M)
  t_hann  the same with -window_flag 1 (scipy.signal.windows.hann(N))
  c4      config 4's source on its 2-yr grid (N = 6.3 M), -template td

Per shape one process builds pe.setup(template="td"), takes the first 8-walker half-step and times
interleaved paired rounds of Likelihood.get_ll (host clock; every call ends with its logL on the
host, so synchronised):
  old   gen.batched = False: per walker __call__ (TD sum, two complex transforms, fftshifts, the
        mask gather) and efd_loglike -- what the package did before the batched route
  new   groups of WINDOW_GROUP walkers: efd_td_modesum_windowed rows, one batched complex
        transform, efd_td_split_loglike
first with the host upstream included (the API rate), then with it memoised
(pe.MemoizedUpstream: the device rate). Both routes are warmed up at every shape first. Then the
split-logL kernel alone over the group's transform buffer, by device events: bytes moved / time
beside efd_fisher_gram's 5.7 TB/s and the 8 TB/s peak; `bytes_min` counts Z once per row and d, w
once in all (what HBM must deliver if the rows' workgroups share d and w in cache), `bytes_rows`
counts d and w once per row (what the kernel requests). One JSON line per round goes to --out,
then a summary per shape: medians, logL/s, old/new of every paired round, the largest
|logL_new - logL_old| relative to |logL_old|, and the transform the route used.

The parent starts each measurement as a child process under its own time limit (--limit seconds)
and starts nothing after one that failed.
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

PAPER = dict(M=3670041.7362535275, mu=292.0583167470244, e0=0.5794130830706371)
SHAPES = {"t": dict(Tobs=4.0, dt=10.0, eps=1e-2, nwalkers=16, ntemps=1, **PAPER),
          "t_hann": dict(Tobs=4.0, dt=10.0, eps=1e-2, nwalkers=16, ntemps=1, window="hann",
                         **PAPER),
          "c4": dict(Tobs=2.0, dt=10.0, eps=1e-2, nwalkers=16, ntemps=1)}
PEAK_TBS, GRAM_TBS = 8.0, 5.7


def measure(name, args):
    import torch
    from emri_frequencydomainwaveforms_amd import _lib, pe
    s = pe.setup(template="td", **SHAPES[name])
    gen, like = s.gen, s.like
    walkers = s.transform.both_transforms(s.half_steps()[0])
    B = len(walkers)
    n, nb = gen.num_samples, gen.num_bins

    def call(batched):
        gen.batched = batched
        t0 = time.perf_counter()
        ll = like.get_ll(walkers, **s.kwargs)
        return (time.perf_counter() - t0) * 1e3, ll

    def rounds(tag):
        for b in (False, True, False, True):     # warm-up: both routes, twice
            call(b)
        rows = []
        for r in range(args.rounds):
            old, ll_o = call(False)
            new, ll_n = call(True)
            row = {"shape": name, "mode": tag, "round": r, "walkers": B, "N": n,
                   "old_ms": old, "new_ms": new, "ratio": old / new,
                   "max_rel_dlogL": float(np.max(np.abs(ll_n - ll_o) / np.abs(ll_o)))}
            rows.append(row)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
        return rows

    api = rounds("api")
    memo = pe.MemoizedUpstream(s.few.waveform_generator)
    dev = rounds("device")
    memo.remove()
    gen.batched = True

    # the split-logL kernel alone, over the transform buffer the last group left
    lib = _lib.load()
    rows = min(B, int(gen.info.get("rows", B)))
    Z = gen._zbuf[:rows]
    out = torch.empty(rows, dtype=torch.float64, device=Z.device)
    scr = torch.empty(rows * _lib.EFD_TD_SPLIT_SCRATCH, dtype=torch.float64, device=Z.device)
    st = torch.cuda.current_stream(Z.device).cuda_stream

    def kernel():
        _lib.check(lib.efd_td_split_loglike(
            torch.view_as_real(Z).data_ptr(), int(Z.stride(0)), n, rows, float(gen.dt),
            torch.view_as_real(like._d).data_ptr(), like._w_templ.data_ptr(), out.data_ptr(),
            scr.data_ptr(), st), "efd_td_split_loglike", lib)
    for _ in range(3):
        kernel()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kt = []
    for _ in range(max(3, args.rounds)):
        torch.cuda.synchronize()
        a.record()
        for _ in range(10):
            kernel()
        b.record()
        torch.cuda.synchronize()
        kt.append(a.elapsed_time(b) / 10)
    k_ms = float(np.median(kt))
    bytes_min = rows * n * 16 + nb * 2 * (16 + 8)
    bytes_rows = rows * (n * 16 + nb * 2 * (16 + 8))

    def med(rs, k):
        return float(np.median([r[k] for r in rs]))
    summ = {"shape": name, "setup": {k: v for k, v in SHAPES[name].items()}, "N": n,
            "walkers": B, "rounds": args.rounds, "route": dict(gen.info),
            "window_group": int(gen.WINDOW_GROUP)}
    for tag, rs in (("api", api), ("device", dev)):
        summ[tag] = {"old_ms_per_half_step": med(rs, "old_ms"),
                     "new_ms_per_half_step": med(rs, "new_ms"),
                     "old_logL_per_s": B / med(rs, "old_ms") * 1e3,
                     "new_logL_per_s": B / med(rs, "new_ms") * 1e3,
                     "old_over_new_per_round": [round(r["ratio"], 3) for r in rs],
                     "new_faster_in_every_round": bool(all(r["ratio"] > 1.0 for r in rs)),
                     "max_rel_dlogL": max(r["max_rel_dlogL"] for r in rs)}
    summ["split_loglike_kernel"] = {
        "rows": rows, "ms": k_ms, "ms_min_max": [min(kt), max(kt)],
        "bytes_min": bytes_min, "bytes_rows": bytes_rows,
        "TB_per_s_min_bytes": bytes_min / (k_ms * 1e-3) / 1e12,
        "TB_per_s_requested": bytes_rows / (k_ms * 1e-3) / 1e12,
        "fisher_gram_TB_per_s": GRAM_TBS, "peak_TB_per_s": PEAK_TBS}
    summ["host_upstream_memoised_s"] = memo.host_s
    print(json.dumps(summ), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps({"summary": summ}) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="t,t_hann,c4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=280, help="each shape's time limit [s]")
    ap.add_argument("--child", default=None, help="(internal) measure this shape")
    args = ap.parse_args()
    if args.child:
        return measure(args.child, args)
    for name in args.shapes.split(","):
        if name not in SHAPES:
            sys.exit(f"unknown shape {name!r}: one of {sorted(SHAPES)}")
    for name in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--child", name, "--rounds", str(args.rounds)]
        if args.out:
            cmd += ["--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
