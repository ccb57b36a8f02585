"""Measurements of the noise realisations ("Noise realisations").

  gen       efd_noise_fd (0.5 gain xi, counter-based) at config 2's grid (2 x 3,155,816 bins) and
            at the windowed test.sh shape (2 x 6,311,631), against (1) torch.randn of the same
            size scaled by the gain on the device and (2) a numpy draw plus the upload.
  overlaps  efd_noise_overlap_rows for 6 rows x 1024 draws at config 2's grid (the noise
            regenerated in registers), against materialising each draw with efd_noise_fd and
            reducing it with efd_overlap_rows. Draws/s and the FP64 rate they imply at
            FLOPS_PER_DRAW_BIN operations per (bin, channel, draw).

Rounds rotate the arms' order (each arm leads once per cycle); one JSON line per round and a
summary line per shape. --out appends them to a file (profiles/noise_bench.jsonl).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 2601996
# Philox (40 32-bit multiplies, not counted), log, sqrt, sincospi and the two products: about
# 10^2 FP64 operations; plus 4 per row (two fmas)
FLOPS_PER_DRAW_BIN = 100


def _emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _device_ms(fn, reps):
    import torch
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _wall_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def _rounds(arms, rounds, base, out):
    """arms: (key, fn -> ms); round r starts with arm r mod len(arms)."""
    rows = []
    for r in range(rounds):
        row = dict(base, round=r)
        k = r % len(arms)
        for key, fn in arms[k:] + arms[:k]:
            row[key + "_ms"] = fn()
        rows.append(row)
        _emit(row, out)
    keys = [k + "_ms" for k, _ in arms]
    med = {k: float(np.median([x[k] for x in rows])) for k in keys}
    spread = {k + "_min_max": [min(x[k] for x in rows), max(x[k] for x in rows)] for k in keys}
    return med, spread


def gen_bench(name, nbin, rounds, reps, out):
    import torch
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    red = Reducer()
    dev = red.device
    gain = torch.rand((2, nbin), dtype=torch.float64, device=dev) + 0.5
    gain[:, 0] = 0.0
    buf = torch.empty((2, nbin), dtype=torch.complex128, device=dev)
    rbuf = torch.view_as_real(buf)
    rng = np.random.default_rng(SEED)
    gh = gain.cpu().numpy()

    def hip():
        red.noise_fd(buf, SEED, 0, 0, gain)

    def randn():
        torch.randn(rbuf.shape, dtype=torch.float64, device=dev, out=rbuf)
        rbuf.mul_((0.5 * gain)[..., None])

    def host():
        x = rng.standard_normal((2, nbin, 2))
        x *= (0.5 * gh)[..., None]
        buf.copy_(torch.view_as_complex(torch.from_numpy(x)))

    arms = [("hip", lambda: _device_ms(hip, reps)), ("randn", lambda: _device_ms(randn, reps)),
            ("numpy_upload", lambda: _wall_ms(host, 1))]
    med, spread = _rounds(arms, rounds, {"bench": "gen", "shape": name, "nbin": nbin}, out)
    nbytes = 2 * nbin * (16 + 8)   # the output written, the gain read
    _emit({"bench": "gen", "summary": name, "nbin": nbin, **med, **spread,
           "hip_TB_per_s": nbytes / (med["hip_ms"] * 1e-3) / 1e12,
           "randn_over_hip": med["randn_ms"] / med["hip_ms"],
           "numpy_upload_over_hip": med["numpy_upload_ms"] / med["hip_ms"]}, out)


def overlap_bench(rounds, out, nrow=6, ndraw=1024, nbin=3155816, explicit_draws=32):
    import torch
    from emri_frequencydomainwaveforms_amd.reductions import Reducer
    red = Reducer()
    dev = red.device
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.view_as_complex(torch.randn((nrow, 2, nbin, 2), dtype=torch.float64, device=dev,
                                             generator=g))
    gain = torch.rand((2, nbin), dtype=torch.float64, device=dev, generator=g) + 0.5
    gain[:, 0] = 0.0
    res = torch.empty((ndraw, nrow), dtype=torch.float64, device=dev)
    buf = torch.empty((2, nbin), dtype=torch.complex128, device=dev)

    def fused():
        red.noise_overlap_rows(rows, gain, SEED, ndraw, out=res)

    def explicit():
        # per draw: the buffer 2 gain (0.5 xi) = gain xi written, then 4 sum Re(conj rows n) / 4
        for r in range(explicit_draws):
            red.noise_fd(buf, SEED, r, 0, gain)
            red.overlap_rows_flat(rows, buf)

    fused()
    first = res[:explicit_draws, :].clone()
    chk = []
    for r in range(2):
        red.noise_fd(buf, SEED, r, 0, gain)
        chk.append(red.overlap_rows(rows, buf)[0][:, 0] * 0.5)
    agree = float((torch.stack(chk) - first[:2]).abs().max() / first[:2].abs().max())
    arms = [("fused", lambda: _device_ms(fused, 3)),
            ("explicit", lambda: _device_ms(explicit, 3) * (ndraw / explicit_draws))]
    base = {"bench": "overlaps", "nrow": nrow, "ndraw": ndraw, "nbin": nbin,
            "explicit_draws_timed": explicit_draws}
    med, spread = _rounds(arms, rounds, base, out)
    per = 2 * nbin * (FLOPS_PER_DRAW_BIN + 4 * nrow)
    _emit({**base, "summary": "config2 grid", **med, **spread,
           "draws_per_s": ndraw / (med["fused_ms"] * 1e-3),
           "fp64_TFLOPS_implied": ndraw * per / (med["fused_ms"] * 1e-3) / 1e12,
           "explicit_over_fused": med["explicit_ms"] / med["fused_ms"],
           "fused_vs_explicit_rel": agree}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="gen,overlaps")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=1000, help="launches per timed window of the "
                    "generation's device arms (0.06-0.25 ms each)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    which = set(args.only.split(","))
    if "gen" in which:
        gen_bench("config2", 3155816, args.rounds, args.reps, args.out)
        gen_bench("test_sh_windowed", 6311631, args.rounds, args.reps, args.out)
    if "overlaps" in which:
        overlap_bench(args.rounds, args.out)


if __name__ == "__main__":
    main()
