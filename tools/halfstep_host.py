"""Host time of one fused-likelihood half-step by phase (config 4 / 5, memoised upstream).

    python tools/halfstep_host.py config4|config5 [python]

("python": the groups' host steps in Python, Likelihood.FUSED_NATIVE_GROUP = False)

Runs bench.py's likelihood setup (pe.setup) and times the product code itself: the methods
Likelihood._run_fused's group steps call (the template's submit_batch, BatchPreparer.flush_loglike
or flush + sum_loglike, _tile_constants) and BatchPreparer's steps inside a flush (_take: the
checks and waits, _sources, _stage, the workspace sizing) are wrapped with perf_counter
accumulators. Prints microseconds per half-step; a flush's figure includes its steps'.
"""
import sys, time, json, collections
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
import torch
import bench
from emri_frequencydomainwaveforms_amd import pe, likelihood as L
from emri_frequencydomainwaveforms_amd.summation import BatchPreparer
cfg = bench.LIKE_CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "config5"]
if "python" in sys.argv[2:]:
    L.Likelihood.FUSED_NATIVE_GROUP = False
s = pe.setup(**cfg)
batches = s.half_steps()
memo = pe.MemoizedUpstream(s.few.waveform_generator)
acc = collections.defaultdict(float)
ft = collections.defaultdict(float)
pc = time.perf_counter


def timed(cls, name, into, key):
    """Replace cls.name by a wrapper that adds its wall time to into[key]."""
    f = getattr(cls, name)

    def wrap(*a, **k):
        t0 = pc()
        try:
            return f(*a, **k)
        finally:
            into[key] += pc() - t0
    setattr(cls, name, staticmethod(wrap) if isinstance(cls.__dict__.get(name), staticmethod)
            else wrap)


timed(type(s.like.template_model), "submit_batch", acc, "submit_batch")
for name, key in (("flush_loglike", "flush+sum (native)"), ("flush", "flush"),
                  ("sum_loglike", "sum_loglike")):
    timed(BatchPreparer, name, acc, key)
timed(L.Likelihood, "_tile_constants", acc, "tile_constants")
timed(L.Likelihood, "get_ll", acc, "get_ll_total")
for name, key in (("_take", "check+wait"), ("_sources", "src"), ("_stage", "stage"),
                  ("_size_each", "jobs"), ("_size_group", "workspaces")):
    timed(BatchPreparer, name, ft, key)
for i in range(5):
    s.like(batches[i % len(batches)], **s.kwargs)
torch.cuda.synchronize()
acc.clear()
ft.clear()
N = 40
t0 = pc()
for i in range(N):
    s.like(batches[i % len(batches)], **s.kwargs)
wall = pc() - t0
print(json.dumps({"cfg": sys.argv[1:], "walkers": s.half_step, "ms_per_half_step": wall / N * 1e3,
                  "us_per_half_step": {k: v / N * 1e6 for k, v in acc.items()},
                  "flush_us_per_half_step": {k: v / N * 1e6 for k, v in ft.items()}}, indent=1))
