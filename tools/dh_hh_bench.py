"""Measurements of the <d|h>, <h|h> pair ("<d|h> and <h|h> from the fused sum").

  parts   Likelihood.parts against (a) the same object's plain fused logL (get_ll) and (b) what a
          user had to do before: per walker the template written (fill) and two inner products,
          at config 4's and config 5's shapes (tools/configs.py), host and device upstream,
          alternated rounds. All three return host values, so every call ends synchronised.
  rows    efd_dh_hh_rows over 16 written templates on config 2's grid (3,155,816 positive
          bins): time and achieved bandwidth, beside efd_td_split_pair_stats' recorded figure
          (profiles/mode_by_mode_bench.jsonl, c_new_ms).

One JSON line per round and a summary line per shape; --out appends them to a file
(profiles/dh_hh_bench.jsonl).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def parts_bench(name, setup_kw, rounds, reps, out):
    import torch
    from emri_frequencydomainwaveforms_amd import pe
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    for upstream in ("host", "device"):
        s = pe.setup(upstream=upstream, **setup_kw)
        like, kw = s.like, s.kwargs
        walkers = s.transform.both_transforms(s.half_steps()[0])
        walkers[0] = s.truth14
        red = Reducer(like.device)
        nch, nb = like._d.shape
        buf = torch.empty((nch, nb), dtype=torch.complex128, device=like.device)
        w2 = (like._w_templ * like._w_templ).contiguous()

        def plain():
            return like.get_ll(walkers, **kw)

        def parts():
            return like.parts(walkers, **kw)

        def user():
            # fill + two inner products per walker, each brought to the host as
            # diagnostic.inner_product does
            res = []
            for p in walkers:
                s.gen.fill(buf, *p, **kw)
                res.append((red.inner(like._d, buf, like._w_templ).item(),
                            red.inner(buf, buf, w2).item()))
            return res

        ll, (d_h, h_h), ref = plain(), parts(), user()
        miss = np.abs(ll + 0.5 * (like.d_d - 2.0 * d_h.real + h_h))
        agree = max(abs(a[0].real - b.real) / max(abs(b.real), 1e-300) for a, b in zip(ref, d_h))
        rows = []
        for r in range(rounds):
            row = {"bench": "parts", "shape": name, "upstream": upstream, "round": r,
                   "walkers": len(walkers), "N_pos": int(nb)}
            order = (("a", plain), ("p", parts), ("b", user))
            for key, fn in (order if r % 2 == 0 else order[::-1]):
                row[key + "_ms"] = _wall(fn, reps)
            rows.append(row)
            _emit(row, out)
        med = {k: float(np.median([x[k] for x in rows])) for k in ("a_ms", "p_ms", "b_ms")}
        spread = {k + "_min_max": [min(x[k] for x in rows), max(x[k] for x in rows)]
                  for k in ("a_ms", "p_ms", "b_ms")}
        _emit({"bench": "parts", "summary": name, "upstream": upstream, **med, **spread,
               "parts_over_plain": med["p_ms"] / med["a_ms"],
               "user_over_parts": med["b_ms"] / med["p_ms"],
               "identity_miss_max": float(miss.max()), "re_dh_rel_vs_user_max": float(agree)}, out)


def rows_bench(rounds, reps, out):
    import torch
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    nrow, nbin = 16, 3155816
    g = torch.Generator(device="cuda").manual_seed(1)
    h = torch.view_as_complex(torch.randn((nrow, 2, nbin, 2), dtype=torch.float64, device="cuda",
                                          generator=g))
    d = torch.view_as_complex(torch.randn((2, nbin, 2), dtype=torch.float64, device="cuda",
                                          generator=g))
    w = torch.rand((2, nbin), dtype=torch.float64, device="cuda", generator=g) + 0.5
    red = Reducer()
    res = torch.empty((nrow, 3), dtype=torch.float64, device="cuda")
    red.dh_hh_rows(h, d, w, out=res)
    nbytes = nrow * 2 * nbin * 16 + 2 * nbin * (16 + 8)   # the rows once, d and w once
    ms = []
    for r in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            red.dh_hh_rows(h, d, w, out=res)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
        _emit({"bench": "rows", "round": r, "rows": nrow, "nbin": nbin, "ms": ms[-1]}, out)
    med = float(np.median(ms))
    _emit({"bench": "rows", "summary": "config2 grid", "rows": nrow, "nbin": nbin, "ms_median": med,
           "ms_min_max": [min(ms), max(ms)], "bytes_read": nbytes,
           "TB_per_s": nbytes / (med * 1e-3) / 1e12}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="4,5,rows")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    which = set(args.only.split(","))
    if "4" in which:
        parts_bench("config4", dict(Tobs=2.0, eps=1e-2, nwalkers=16), args.rounds, args.reps,
                    args.out)
    if "5" in which:
        parts_bench("config5", dict(Tobs=4.0, eps=1e-2, downsample=100, nwalkers=128),
                    args.rounds, args.reps, args.out)
    if "rows" in which:
        rows_bench(args.rounds, args.reps, args.out)


if __name__ == "__main__":
    main()
