"""The batched mode-by-mode study against the per-call route it replaces, and its reduction
kernel against the kernels that replaces, at two shapes (GPU box): the driver's example
(check_mode_by_mode.py's header: Tobs 1 yr, dt 10 s, eps 1e-2) and config 2's grid (Tobs 2 yr).

    python tools/mode_by_mode_bench.py [--rounds R] [--sources S] [--shapes driver,config2]
                                       [--out profiles/mode_by_mode_bench.jsonl]

The parent starts the measurement as a child process under its own time limit (--limit seconds)
and starts nothing else after it. Per shape the child builds the study and the per-call route's
generators, memoises every generator's host upstream (the timed sections are the device path and
its host glue, inputs resident), warms both routes up once, then times R paired rounds, the
order rotated from round to round, with a host clock around work that ends in a device
synchronise:
  a  study.run over the S sources (mode_by_mode), split by device events into the FD side, the TD
     sums, window + transform, and the reduction;
  b  the per-call route on the same sources, the way of the code before the study:
     get_fd_waveform_fromFD / get_fd_waveform_fromTD __call__ per window and source, then
     diagnostic.inner_product in the driver's sequence (:292, :299, :313-317);
  c  efd_td_split_pair_stats alone over the group's S W rows against what it replaces on the same
     rows: efd_td_split, then per row the efd_inner_product calls of the driver's sequence (four
     over both channels, the difference a - b as a temporary, two more), weights resident, no
     host synchronisation. Time, and the bytes the new kernel reads (Z, a, w) over its time.
One JSON line per round and shape goes to --out, then a summary with the medians and every
round's ratios. Conditions: c's old / new > 1 and b / a >= 1 in every round.
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

SHAPES = {"driver": dict(Tobs=1.0, dt=10.0, eps=1e-2),
          "config2": dict(Tobs=2.0, dt=10.0, eps=1e-2)}
PEAK_TBS, COPY_TBS = 8.0, 6.29


def sources(study, count):
    """`count` sources around pe.setup's (M 1e6, mu 10, e0 0.35), each with the driver's fixed
    inspiral."""
    rng = np.random.default_rng(2601996)
    p = np.tile(np.array([1e6, 10.0, 0.0, 12.0, 0.35, 1.0, 2.4539054256, np.pi / 3, np.pi / 3,
                          np.pi / 3, np.pi / 3, np.pi / 3, 0.0, np.pi / 3]), (count, 1))
    p[:, 0] *= 1.0 + 0.05 * rng.uniform(-1, 1, size=count)
    p[:, 4] += 0.05 * rng.uniform(-1, 1, size=count)
    p[:, 11] = rng.uniform(0, 2 * np.pi, size=count)
    p[:, 13] = rng.uniform(0, 2 * np.pi, size=count)
    return study.fixed_inspiral(p)


def measure(name, args):
    import scipy.signal.windows as sw
    import torch
    from emri_frequencydomainwaveforms_amd import diagnostic, mode_by_mode, pe
    from emri_frequencydomainwaveforms_amd.fdutils import (get_fd_waveform_fromFD,
                                                           get_fd_waveform_fromTD, get_sensitivity)
    from emri_frequencydomainwaveforms_amd.waveform import GenerateEMRIWaveform
    shape = SHAPES[name]
    T, dt, eps = shape["Tobs"], shape["dt"], shape["eps"]
    study = mode_by_mode.setup(T, dt, eps, group=args.sources)
    params = sources(study, args.sources)
    W, N, nb = len(study.windows), study.N, study.nb
    few = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                               sum_kwargs=dict(pad_output=True, output_type="fd", odd_len=True),
                               use_gpu=True, return_list=True)
    td = GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
                              sum_kwargs=dict(pad_output=True, odd_len=True), use_gpu=True,
                              return_list=True)
    memos = [pe.MemoizedUpstream(g.waveform_generator) for g in (study.fd, study.td, few, td)]
    pos = study.frequency >= 0.0
    ipk = dict(PSD=get_sensitivity(study.f_pos), f_arr=study.f_pos)
    kw = dict(T=T, dt=dt, eps=eps)
    models = []
    for wname in study.windows:
        win = None if wname == "none" else getattr(sw, wname)(N)
        models.append((get_fd_waveform_fromFD(few, pos, dt, window=win),
                       get_fd_waveform_fromTD(td, pos, dt, window=win)))

    def per_call():
        out = np.empty((len(params), W, 3))
        for j, (fd_t, td_t) in enumerate(models):
            for i, p in enumerate(params):
                sig_fd, sig_td = fd_t(*p, **kw), td_t(*p, **kw)
                snr = np.sqrt(float(diagnostic.inner_product(sig_fd, sig_fd, **ipk)))
                mism = abs(1 - diagnostic.inner_product(sig_fd, sig_td, normalize=True, **ipk))
                inner = [sig_fd[0] - sig_td[0], sig_fd[1] - sig_td[1]]
                logl = -0.5 * sum(diagnostic.inner_product(el, el, normalize=False, **ipk)
                                  for el in inner)
                out[i, j] = snr, mism, logl
        return out

    marks = []

    def mark(label):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((label, ev))

    def batched():
        del marks[:]
        study.timing = mark
        try:
            return study.run(params)
        finally:
            study.timing = None

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def split():
        parts = {}
        for (_, e0), (label, e1) in zip(marks[:-1], marks[1:]):
            if label != "start":
                parts[label] = parts.get(label, 0.0) + e0.elapsed_time(e1)
        return parts

    _, res = wall(batched)
    _, ref = wall(per_call)
    assert len(res["failed"]) == 0
    dist = dict(SNR=float(np.max(np.abs(res["SNR"] / ref[..., 0] - 1))),
                mismatch=float(np.max(np.abs(res["mismatch"] - ref[..., 1]))),
                loglike=float(np.max(np.abs(res["loglike"] - ref[..., 2])
                                     / (res["SNR"] ** 2 + res["snr_td"] ** 2))))

    # c: the reduction alone on the group's rows (left in the study's buffers by the run above)
    R = len(params) * W
    Z, a, w = study._buf["Z"][:R], study._buf["a"][:R], study.w
    red = study.red
    w2 = w.expand(2, nb).contiguous()
    w1 = w[None, :].contiguous()
    b = torch.empty_like(a)

    def new():
        return red.td_split_pair_stats(Z, N, dt, a, w)

    def old():
        study._tdm._split(Z, b)
        out = []
        for r in range(R):
            ar, br = a[r], b[r]
            out += [red.inner(ar, ar, w2), red.inner(ar, br, w2), red.inner(ar, ar, w2),
                    red.inner(br, br, w2)]
            d = ar - br
            out += [red.inner(d[0:1], d[0:1], w1), red.inner(d[1:2], d[1:2], w1)]
        return out

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    new()
    old()
    nbytes = R * (16 * N + 32 * nb) + 8 * nb
    rounds = []
    for r in range(args.rounds):
        row = {"shape": name, "round": r, "N": N, "sources": len(params), "windows": W}
        for which in (("a", "b"), ("b", "a"))[r % 2]:
            if which == "a":
                row["a_study_ms"], _ = wall(batched)
                row["a_split_ms"] = split()
            else:
                row["b_per_call_ms"], _ = wall(per_call)
        for which in (("new", "old"), ("old", "new"))[r % 2]:
            row["c_" + which + "_ms"] = timed(new if which == "new" else old, args.reps)
        rounds.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    med = {k: float(np.median([r[k] for r in rounds]))
           for k in ("a_study_ms", "b_per_call_ms", "c_new_ms", "c_old_ms")}
    parts = {k: float(np.median([r["a_split_ms"].get(k, 0.0) for r in rounds]))
             for k in ("fd_side", "td_sum", "window_transform", "reduction")}
    ba = [round(r["b_per_call_ms"] / r["a_study_ms"], 3) for r in rounds]
    on = [round(r["c_old_ms"] / r["c_new_ms"], 3) for r in rounds]
    summ = {"shape": name, "setup": shape, "N": N, "sources": len(params), "windows": W,
            "rounds": args.rounds, "reps": args.reps,
            **{k + "_median": v for k, v in med.items()},
            "a_study_ms_per_source": med["a_study_ms"] / len(params),
            "a_split_ms_median": parts,
            "b_over_a": ba, "c_old_over_new": on,
            "c_new_bytes_read": nbytes,
            "c_new_GB_per_s": nbytes / (med["c_new_ms"] * 1e-3) / 1e9,
            "peak_TB_per_s": PEAK_TBS, "measured_copy_TB_per_s": COPY_TBS,
            "td_transform": study._tdm.info.get("transform"),
            "fd_windows_first_order": [wn for wn, c in zip(study.windows, study._coef)
                                       if c is not None],
            "a_vs_b_distance": dist,
            "host_upstream_memoised_s": sum(m.host_s for m in memos),
            "condition_c_old_over_new_gt_1": bool(min(on) > 1.0),
            "condition_b_over_a_ge_1": bool(min(ba) >= 1.0)}
    print(json.dumps(summ), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps({"summary": summ}) + "\n")
    for m in memos:
        m.remove()


def child(args):
    for name in args.shapes.split(","):
        measure(name, args)
        import torch
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--shapes", default="driver,config2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mode_by_mode_bench.jsonl"))
    ap.add_argument("--limit", type=int, default=500, help="the child's time limit [s]")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
