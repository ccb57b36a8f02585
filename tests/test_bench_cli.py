"""bench.py's rank-count guard (CPU): --gpus must equal the launcher's WORLD_SIZE, so a
multi-GPU figure can never come from one process timing one GPU (VERDICT r4 missing #3); the
--dump-outputs helpers (CPU) and one plain run with its result line and dump (GPU)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, world=None):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    if world is not None:
        env["WORLD_SIZE"] = str(world)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                          capture_output=True, text=True, timeout=120, env=env)


def test_gpus_without_launcher_fails():
    for mode in ([], ["--likelihood", "config4"], ["--scan", "config3"]):
        r = _run(["--gpus", "8", *mode])
        assert r.returncode == 2, r.stderr
        assert "WORLD_SIZE=1" in r.stderr and "torch.distributed.run" in r.stderr


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "2"], world=4)
    assert r.returncode == 2 and "--gpus 2 but WORLD_SIZE=4" in r.stderr


def test_world_size_helper():
    sys.path.insert(0, ROOT)
    import bench
    os.environ.pop("WORLD_SIZE", None)
    assert bench.world_size(1) == 1


def test_steps_must_be_positive():
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


def test_sample_bins_fixed_and_within_budget():
    sys.path.insert(0, ROOT)
    import bench
    n = 3155816                       # config 2's f >= 0 bins
    sel = bench.sample_bins(n, 16)    # h+ and hx of 8 waveforms
    assert np.array_equal(sel, bench.sample_bins(n, 16))
    assert np.all(np.diff(sel) > 0) and sel[0] >= 0 and sel[-1] < n
    assert 16 * 16 * len(sel) <= bench.DUMP_BYTES < 64e6
    assert np.array_equal(bench.sample_bins(1000, 16), np.arange(1000))


def test_dump_outputs_writes_float64(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    z = np.arange(6).reshape(3, 2).astype(np.float32) * (1 + 2j)
    bench.dump_outputs(str(tmp_path / "d"), [("z", z), ("k", np.arange(4))])
    got = np.load(tmp_path / "d" / "z.npy")
    assert got.dtype == np.float64 and got.shape == (3, 2, 2)
    assert np.array_equal(got[..., 0], z.real) and np.array_equal(got[..., 1], z.imag)
    k = np.load(tmp_path / "d" / "k.npy")
    assert k.dtype == np.float64 and np.array_equal(k, np.arange(4))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain run times exactly --steps steps, leaves the --full legs out and writes the last
    step's h+/hx (8 waveforms, sampled bins) as float64 files within the 64 MB budget."""
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "waveforms/s" and line["higher_is_better"] and line["dtype"] == "f64"
    assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    assert line["cpu_baseline"] is None and line["cpu_reference"] is None
    assert line["few_gen"] is None
    files = sorted(p.name for p in out.iterdir())
    assert files == sorted([f"{c}_{j}.npy" for c in ("hp", "hc") for j in range(8)]
                           + ["sample_bins.npy"])
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64e6
    sel = np.load(out / "sample_bins.npy")
    for name in files[:-1]:
        a = np.load(out / name)
        assert a.dtype == np.float64 and a.shape == (len(sel), 2)
        assert np.isfinite(a).all() and np.abs(a).max() > 0
