"""The device upstream (amplitudes and mode selection on the device, upstream="device") against
the host upstream of the same commit, at the batched callers' shapes (GPU box).

    python tools/upstream_bench.py [--rounds R] [--parts c4,c5,c3,sel] [--out FILE.jsonl]

  c4   config 4 through pe.setup: Tobs 2 yr, eps 1e-2, 16 walkers -> 8 per half-step, full grid
  c5   config 5 through pe.setup: Tobs 4 yr, downsample 100, 128 walkers -> 64 per half-step
  c3   config 3's scan: 10 x 10 grid M = logspace(5, 7), e0 = linspace(0.1, 0.6), mu = 1e-5 M,
       Tobs 1 yr, eps 1e-2 through generate_batch (the p0 root solves are made once, untimed)
  sel  efd_modes_select_batch alone, by device events, for one group of 16 walkers of config 4's
       start at eps = 1e-2 (config 4's shape) and eps = 1e-5 (config 2's); beside it
       efd_host_modes for the same walkers on the prefetch pool (one walker per thread)

c4, c5 and c3 are paired rounds on one box: each round times both routes, in an order that
rotates from round to round (host clock; every call ends with its results' stream joined and
synchronised). Both routes are warmed up first. One JSON line per round goes to --out (default
profiles/device_upstream_bench.jsonl), then a summary per part with the medians, the rates and
`device_faster_in_every_round`: the device route is the recommended one for a configuration only
where that is true.

The parent starts each part as a child process under its own time limit (--limit seconds) and
starts nothing after one that failed.
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

SUM_KW = dict(pad_output=True, output_type="fd", odd_len=True)
LIKE = {"c4": dict(Tobs=2.0, eps=1e-2, nwalkers=16),
        "c5": dict(Tobs=4.0, eps=1e-2, downsample=100, nwalkers=128)}
PARTS = ("c4", "c5", "c3", "sel")


def _emit(args, row):
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


def _paired(args, part, routes, unit, count):
    """Warm both routes up, then args.rounds paired rounds in rotated order; returns the rows."""
    names = list(routes)
    for _ in range(3):
        for k in names:
            routes[k]()
    rows = []
    for r in range(args.rounds):
        order = names[r % 2:] + names[:r % 2]
        ms = {}
        for k in order:
            t0 = time.perf_counter()
            routes[k]()
            ms[k] = (time.perf_counter() - t0) * 1e3
        row = {"part": part, "round": r, "order": order, "count": count,
               **{f"{k}_ms": ms[k] for k in names}, "host_over_device": ms["host"] / ms["device"]}
        rows.append(row)
        _emit(args, row)
    med = {k: float(np.median([r[f"{k}_ms"] for r in rows])) for k in names}
    summ = {"part": part, "rounds": args.rounds, "count": count,
            **{f"{k}_ms": med[k] for k in names},
            **{f"{k}_{unit}_per_s": count / med[k] * 1e3 for k in names},
            "host_over_device_per_round": [round(r["host_over_device"], 3) for r in rows],
            "device_faster_in_every_round": bool(all(r["host_over_device"] > 1.0 for r in rows))}
    return summ


def likelihood(part, args):
    from emri_frequencydomainwaveforms_amd import pe
    sh = pe.setup(**LIKE[part])
    sd = pe.setup(upstream="device", **LIKE[part])
    walkers = sh.transform.both_transforms(sh.half_steps()[0])
    ll = {}

    def run(s, k):
        def f():
            ll[k] = s.like.get_ll(walkers, **s.kwargs)
        return f

    summ = _paired(args, part, {"host": run(sh, "host"), "device": run(sd, "device")}, "logL",
                   len(walkers))
    summ["setup"] = LIKE[part]
    summ["N_pos"] = int(len(sh.f_like))
    summ["max_abs_dlogL"] = float(np.max(np.abs(ll["device"] - ll["host"])))
    summ["max_abs_logL"] = float(np.max(np.abs(ll["host"])))
    return summ


def scan(args):
    import torch
    from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t
    from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform, _pool
    T, dt, eps = 1.0, 10.0, 1e-2
    few = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux", sum_kwargs=SUM_KW, use_gpu=True,
                               return_list=True)
    traj = EMRIInspiral()
    pts = [(M, e0) for M in np.logspace(5, 7, 10) for e0 in np.linspace(0.1, 0.6, 10)]
    p0s = list(_pool().map(
        lambda me: float(get_p_at_t(traj, 0.99 * T, [me[0], 1e-5 * me[0], 0.0, me[1], 1.0])), pts))
    prm = np.array([[M, 1e-5 * M, 0.0, p0, e0, 1.0, 2.4539, 0.2, 0.2, 0.8, 0.8, 1.0, 0.0, 3.0]
                    for (M, e0), p0 in zip(pts, p0s)])
    out = torch.empty((len(pts), 2, few.positive_bins(T=T, dt=dt)), dtype=torch.complex128,
                      device="cuda")

    def run(upstream):
        def f():
            few.generate_batch(prm, out, T=T, dt=dt, eps=eps, upstream=upstream)
            torch.cuda.synchronize()
        return f

    summ = _paired(args, "c3", {"host": run("host"), "device": run("device")}, "waveforms",
                   len(pts))
    summ["note"] = "generate_batch over the 100 grid points; p0 root solves made once, untimed"
    return summ


def selection(args):
    import torch
    from emri_frequencydomainwaveforms_amd import _lib, pe
    from emri_frequencydomainwaveforms_amd.waveform import _pool
    s = pe.setup(**LIKE["c4"])
    few = s.few
    wg = few.waveform_generator
    amp = wg.amplitude_generator
    lib = _lib.load()
    rows = s.transform.both_transforms(s.start)[:16]
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"part": "sel", "walkers": len(rows)}
    for tag, eps, view in (("config4_eps1e-2", 1e-2, None),
                           ("config2_eps1e-5", 1e-5, (np.pi / 3, -np.pi / 2))):
        calls, _ = few.device_calls(rows, 2.0, eps)
        trajs = [f.result() for f in wg.trajectories_async(calls)]
        ps = [torch.from_numpy(t[1]).to(dev) for t in trajs]
        es = [torch.from_numpy(t[2]).to(dev) for t in trajs]
        # config 4's walkers see the source face-on (theta = pi: few branches carry power);
        # config 2's shape is bench.py's viewing angle, which keeps ~3,000 modes
        ys = [wg._ylms(*((c[4], c[5]) if view is None else view)) for c in calls]
        yd = {id(y): torch.from_numpy(np.ascontiguousarray(y)).to(dev) for y in ys}
        ydev = [yd[id(y)] for y in ys]
        state = {}
        res = amp.select_batch_device(ps, es, ydev, eps, state=state)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ka, kb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts, tk = [], []
        for _ in range(max(5, args.rounds)):
            torch.cuda.synchronize()
            a.record()
            amp.select_batch_device(ps, es, ydev, eps, state=state, prof=(ka, kb))
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
            tk.append(ka.elapsed_time(kb))
        # the same walkers' efd_host_modes on the prefetch pool, one OpenMP thread per walker
        def host(i):
            lib.efd_host_set_threads(1)
            return amp.select(trajs[i][1], trajs[i][2], ys[i], eps, lib=lib)
        list(_pool().map(host, range(len(rows))))
        th = []
        for _ in range(max(5, args.rounds)):
            t0 = time.perf_counter()
            list(_pool().map(host, range(len(rows))))
            th.append((time.perf_counter() - t0) * 1e3)
        out[tag] = {"nt_min_max": [min(len(t[0]) for t in trajs), max(len(t[0]) for t in trajs)],
                    "K_min_max": [min(r[1] for r in res), max(r[1] for r in res)],
                    "device_launches_ms": float(np.median(tk)),
                    "device_launches_ms_min_max": [min(tk), max(tk)],
                    "device_group_ms": float(np.median(ts)),
                    "device_group_ms_min_max": [min(ts), max(ts)],
                    "device_note": "device_launches: events around efd_modes_select_batch's "
                                   "three launches; device_group: around select_batch_device, "
                                   "which adds the download of nkeep/status/keep and the stream "
                                   "synchronisation",
                    "host_modes_pool_ms": float(np.median(th)),
                    "host_modes_pool_ms_min_max": [min(th), max(th)],
                    "pool_threads": _pool()._max_workers}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_upstream_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=280, help="each part's time limit [s]")
    ap.add_argument("--child", default=None, help="(internal) measure this part")
    args = ap.parse_args()
    if args.child:
        part = args.child
        summ = (likelihood(part, args) if part in LIKE else scan(args) if part == "c3"
                else selection(args))
        print(json.dumps(summ), flush=True)
        _emit(args, {"summary": summ})
        return
    parts = args.parts.split(",")
    for name in parts:
        if name not in PARTS:
            sys.exit(f"unknown part {name!r}: one of {PARTS}")
    for name in parts:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--child", name, "--rounds", str(args.rounds), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
