"""The noise-weighted mode selection (ModeSelector(sensitivity_fn=get_sensitivity)) against the
unweighted one of the same build (GPU box). Recorded, not gated.

    python tools/weighted_selection_bench.py [--rounds R] [--parts sel,mismatch,c4,c5]
                                             [--out FILE.jsonl] [--tag TEXT]

  sel       one 16-walker group through select_batch_device, device events around the three
            launches alone: weighted against unweighted in paired rounds of rotated order, at
            config 4's walkers (eps 1e-2) and config 2's viewing angle (eps 1e-5)
  mismatch  config 2's source at T = 0.1 yr, eps in {1e-2, 1e-3, 1e-5}: K of both selections and
            each selection's mismatch against the eps = 0 waveform under get_sensitivity
            (diagnostic.pair_statistics)
  c4, c5    tools/upstream_bench.py's config-4 and config-5 likelihood rates through
            pe.setup(upstream="device"), weighted beside unweighted, paired rounds

One JSON line per part goes to --out (default profiles/weighted_selection_bench.jsonl). The parent
starts each part as a child process under its own time limit (--limit seconds) and starts nothing
after one that failed. --tag labels the lines (e.g. a build variant chosen with EFD_LIB).
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
PARTS = ("sel", "mismatch", "c4", "c5")


def selection(args):
    import torch
    from emri_frequencydomainwaveforms_amd import amplitude, fdutils, pe
    s = pe.setup(**LIKE["c4"])
    few = s.few
    wg = few.waveform_generator
    amp = wg.amplitude_generator
    psd = amplitude.psd_table(fdutils.get_sensitivity)
    rows = s.transform.both_transforms(s.start)[:16]
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"part": "sel", "walkers": len(rows), "psd_knots": int(psd.host.n)}
    for tag, eps, view in (("config4_eps1e-2", 1e-2, None),
                           ("config2_eps1e-5", 1e-5, (np.pi / 3, -np.pi / 2))):
        calls, _ = few.device_calls(rows, 2.0, eps)
        trajs = [f.result() for f in wg.trajectories_async(calls)]
        ps, es, fp, fr = ([torch.from_numpy(t[j]).to(dev) for t in trajs] for j in (1, 2, 5, 6))
        ys = [wg._ylms(*((c[4], c[5]) if view is None else view)) for c in calls]
        yd = {id(y): torch.from_numpy(np.ascontiguousarray(y)).to(dev) for y in ys}
        ydev = [yd[id(y)] for y in ys]
        state = {}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run(weighted):
            kw = dict(f_phi_list=fp, f_r_list=fr, psd=psd) if weighted else {}
            res = amp.select_batch_device(ps, es, ydev, eps, state=state, prof=ev, **kw)
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]), res

        K = {}
        for _ in range(3):
            for wtd in (False, True):
                K[wtd] = [r[1] for r in run(wtd)[1]]
        rounds = []
        for r in range(max(5, args.rounds)):
            ms = {}
            for wtd in ((False, True) if r % 2 == 0 else (True, False)):
                ms[wtd] = run(wtd)[0]
            rounds.append({"unweighted_ms": ms[False], "weighted_ms": ms[True],
                           "ratio": ms[True] / ms[False]})
        out[tag] = {"nt_min_max": [min(len(t[0]) for t in trajs), max(len(t[0]) for t in trajs)],
                    "K_unweighted_min_max": [min(K[False]), max(K[False])],
                    "K_weighted_min_max": [min(K[True]), max(K[True])],
                    "unweighted_ms": float(np.median([r["unweighted_ms"] for r in rounds])),
                    "weighted_ms": float(np.median([r["weighted_ms"] for r in rounds])),
                    "median_ratio": float(np.median([r["ratio"] for r in rounds])),
                    "ratio_per_round": [round(r["ratio"], 4) for r in rounds]}
    return out


def mismatch(args):
    import torch
    from emri_frequencydomainwaveforms_amd import fdutils
    from emri_frequencydomainwaveforms_amd.diagnostic import pair_statistics
    from emri_frequencydomainwaveforms_amd.trajectory import EMRIInspiral, get_p_at_t
    from emri_frequencydomainwaveforms_amd.waveform import FastSchwarzschildEccentricFlux
    T, dt = 0.1, 10.0
    M, mu, e0, theta, phi = 1e6, 10.0, 0.35, np.pi / 3, -np.pi / 2   # config 2's source
    p0 = float(get_p_at_t(EMRIInspiral(), 0.99 * T, [M, mu, 0.0, e0, 1.0]))
    gens = {"unweighted": FastSchwarzschildEccentricFlux(sum_kwargs=SUM_KW, use_gpu=True),
            "weighted": FastSchwarzschildEccentricFlux(
                sum_kwargs=SUM_KW, use_gpu=True,
                mode_selector_kwargs=dict(sensitivity_fn=fdutils.get_sensitivity))}

    def wave(g, eps):
        h = g(M, mu, p0, e0, theta, phi, 1.0, T=T, dt=dt, eps=eps, mask_positive=True)
        return h[:, 1:].clone(), len(g.last_modes[0])   # (the f = 0 bin is dropped)

    full, K0 = wave(gens["unweighted"], 0.0)
    f = gens["unweighted"].create_waveform.frequency
    f = (f if hasattr(f, "detach") else torch.as_tensor(f)).to(full.device)
    f = f[f >= 0.0][1:]
    out = {"part": "mismatch", "T_yr": T, "dt": dt, "source": dict(M=M, mu=mu, e0=e0, p0=p0,
                                                                    theta=theta, phi=phi),
           "K_eps0": K0, "rows": []}
    for eps in (1e-2, 1e-3, 1e-5):
        row = {"eps": eps}
        for name, g in gens.items():
            h, K = wave(g, eps)
            st = pair_statistics(h[None], full[None], f_arr=f, PSD="LISA_Alloc_Sh")
            row[f"K_{name}"] = K
            row[f"mismatch_{name}"] = float(st.mismatch[0])
            row[f"snr_{name}"] = float(st.snr1[0])
        row["snr_eps0"] = float(st.snr2[0])
        out["rows"].append(row)
    return out


def likelihood(part, args):
    from emri_frequencydomainwaveforms_amd import fdutils, pe
    su = pe.setup(upstream="device", **LIKE[part])
    sw = pe.setup(upstream="device", **LIKE[part],
                  mode_selector_kwargs=dict(sensitivity_fn=fdutils.get_sensitivity))
    walkers = su.transform.both_transforms(su.half_steps()[0])
    routes = {"unweighted": lambda: su.like.get_ll(walkers, **su.kwargs),
              "weighted": lambda: sw.like.get_ll(walkers, **sw.kwargs)}
    names = list(routes)
    for _ in range(3):
        for k in names:
            routes[k]()
    rounds = []
    for r in range(args.rounds):
        ms = {}
        for k in names[r % 2:] + names[:r % 2]:
            t0 = time.perf_counter()
            routes[k]()
            ms[k] = (time.perf_counter() - t0) * 1e3
        rounds.append(ms)
    med = {k: float(np.median([r[k] for r in rounds])) for k in names}
    return {"part": part, "setup": LIKE[part], "upstream": "device", "count": len(walkers),
            "rounds": args.rounds, **{f"{k}_ms": med[k] for k in names},
            **{f"{k}_logL_per_s": len(walkers) / med[k] * 1e3 for k in names},
            "weighted_over_unweighted_per_round": [round(r["weighted"] / r["unweighted"], 4)
                                                   for r in rounds]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "weighted_selection_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=280, help="each part's time limit [s]")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--child", default=None, help="(internal) measure this part")
    args = ap.parse_args()
    if args.child:
        part = args.child
        summ = (likelihood(part, args) if part in LIKE else selection(args) if part == "sel"
                else mismatch(args))
        if args.tag:
            summ["tag"] = args.tag
        print(json.dumps(summ), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(summ) + "\n")
        return
    parts = args.parts.split(",")
    for name in parts:
        if name not in PARTS:
            sys.exit(f"unknown part {name!r}: one of {PARTS}")
    for name in parts:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--child", name, "--rounds", str(args.rounds), "--out", args.out]
        if args.tag:
            cmd += ["--tag", args.tag]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(rc)


if __name__ == "__main__":
    main()
