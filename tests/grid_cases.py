"""Frequency grids that exercise the mode sum's lane-range code off the uniform FEW grid, shared
by tests/test_cpu_twin_grids.py and tests/test_gpu_grid_edges.py. Pure numpy.

The preparation (k_items, emrifd_prepare.hip; build of the interval records in emrifd_cpu.cpp)
turns each record's frequency interval into lane ranges on the caller's ascending grid. On the
device the four bounds come from a linear index guess floor((v - f0) (nf - 1) / span), three grid
values around it, and a galloping search only when those do not settle the bound; a record owns
[F_j, F_{j+1}), open at its run's first knot. The grids here make the guess useless
(non-uniform spacing), put bins exactly on the knot frequencies F = m f_phi + n f_r and on their
two floating-point neighbours, and take the shapes the uniform grids never have: even-length
symmetric grids (no f = 0 bin), lane counts at a tile boundary (768 lanes), nf = 1, 2, 3, and
repeated values.

Sources: SRC is the suite's usual small source (N_t = 45, K = 75: the segment table built by
k_segment_slots / _compact / k_seg_tiles); its first FIRST_K harmonics take the K <= 64 path
(k_prep_pcr_b's own grouping, k_segments_one). NONMONO is the source of
test_gpu_modesum.test_non_monotonic_and_negative_harmonics, whose F has turning points: the knot
at a turning point belongs to neither run.
"""

import numpy as np

SRC = dict(M=3e5, mu=10.0, e0=0.35, T=0.02, dt=20.0, eps=1e-2)
NONMONO_MODES = [(2, 1, -2), (3, 2, -4), (2, 0, -3), (2, 0, 2), (4, 1, -3), (3, 3, -5), (2, 2, 0)]
NONMONO = dict(M=3e5, mu=10.0, e0=0.5, T=0.02, dt=20.0, modes=NONMONO_MODES)
FIRST_K = 8

# grid sizes around one tile of lanes (TILE * BPL = 768): 1535 .. 1538 bins are 768 / 768 / 769 /
# 769 lanes of a symmetric grid, 767 .. 769 the lanes of a one-sided one
SMALL_NF = (1, 2, 3, 767, 768, 769, 1535, 1536, 1537, 1538)

NONUNIFORM = ("geom", "geom_one", "random", "two_density", "outlier", "dups")
KNOT_EXACT = ("knot_odd", "knot_even", "knot_one")


def first_harmonics(d, k=FIRST_K):
    """The source d restricted to its first k harmonics."""
    out = dict(d)
    out["amp"] = np.asarray(d["amp"])[:k]
    for key in ("m", "n", "ylm_p", "ylm_m"):
        out[key] = np.asarray(d[key])[:k]
    return out


def knot_values(d):
    """|m f_phi + n f_r| at every knot of every harmonic, nonzero entries, in numpy's own
    rounding (product, product, sum, each rounded once: the oracle's supports; the device's lane
    bounds must use the same doubles, knotF_rn in emrifd_prepare.hip)."""
    m = np.asarray(d["m"])
    n = np.asarray(d["n"])
    F = np.abs(m[None, :] * d["f_phi"][:, None] + n[None, :] * d["f_r"][:, None]).ravel()
    return np.unique(F[F != 0.0])


def mirrored(p, zero=True):
    """The symmetric grid of the positive half p: [-p reversed, 0, p], or without the 0 bin."""
    p = np.asarray(p, dtype=np.float64)
    mid = [0.0] if zero else []
    return np.concatenate([-p[::-1], mid, p])


def knot_exact(d, kind):
    """Bins exactly on every knot frequency, on both of its floating-point neighbours, and on a
    coarse linspace between them. kind: "odd" (symmetric with the 0 bin), "even" (symmetric
    without it) or "one" (the positive half alone)."""
    F = knot_values(d)
    fmax = d["freq"].max()
    v = np.unique(np.concatenate([F, np.nextafter(F, np.inf), np.nextafter(F, -np.inf),
                                  np.linspace(0.0, fmax, 400)[1:]]))
    v = v[v > 0.0]
    if kind == "odd":
        return mirrored(v)
    if kind == "even":
        return mirrored(v, zero=False)
    if kind == "one":
        return v
    raise ValueError(kind)


def nonuniform(d, name):
    """The non-uniform grids (NONUNIFORM) over the source's band."""
    fmax = d["freq"].max()
    geom = np.geomspace(1e-6, fmax, 1500)
    if name == "geom":
        return mirrored(geom)
    if name == "geom_one":
        return geom
    if name == "random":
        return np.sort(np.random.default_rng(5).uniform(-fmax, fmax, 3001))
    if name == "two_density":
        p = np.unique(np.concatenate([np.linspace(0.0, 0.1 * fmax, 50),
                                      np.linspace(0.1 * fmax, 0.12 * fmax, 2000),
                                      np.linspace(0.12 * fmax, fmax, 60)]))
        return mirrored(p[p > 0.0])
    if name == "outlier":
        return mirrored(np.concatenate([np.linspace(0.05 * fmax, 0.4 * fmax, 2000),
                                        [1e3 * fmax]]))
    if name == "dups":   # ascending, not strictly: every 7th value twice
        return mirrored(np.sort(np.concatenate([geom, geom[::7]])))
    raise ValueError(name)


def small(d, nf, symmetric):
    """nf uniformly spaced bins below 0.3 fmax: symmetric (the 0 bin iff nf is odd) or
    one-sided."""
    fmax = d["freq"].max()
    if symmetric:
        q = np.linspace(0.0, 0.3 * fmax, nf // 2 + 1)[1:]
        grid = mirrored(q, zero=bool(nf % 2))
    else:
        grid = np.linspace(0.01 * fmax, 0.3 * fmax, nf) if nf > 1 else np.array([0.1 * fmax])
    assert len(grid) == nf
    return grid


def grid(d, name):
    """The grid `name` for source d: a KNOT_EXACT or NONUNIFORM name, "sym_<nf>" or
    "one_<nf>"."""
    if name in KNOT_EXACT:
        return knot_exact(d, name[len("knot_"):])
    if name in NONUNIFORM:
        return nonuniform(d, name)
    kind, nf = name.split("_")
    return small(d, int(nf), {"sym": True, "one": False}[kind])


SMALL = tuple(f"{kind}_{nf}" for kind in ("sym", "one") for nf in SMALL_NF)
# (source, grid) pairs: every grid on the full source (K = 75); the knot-exact grids of the
# non-monotonic source; and, for the K <= 64 preparation path, the first FIRST_K harmonics
BOTH_PATHS = ("knot_odd", "knot_even", "geom", "outlier") + tuple(
    f"{kind}_{nf}" for kind in ("sym", "one") for nf in (1, 2, 3, 1536, 1537))
CASES = ([("full", g) for g in KNOT_EXACT + NONUNIFORM + SMALL]
         + [("nonmono", g) for g in KNOT_EXACT]
         + [("first", g) for g in BOTH_PATHS])
# the cases that also run with the plain stationary-phase caustic mode
SPA_CASES = (("full", "knot_odd"), ("full", "geom"), ("first", "knot_even"), ("first", "geom"))


def case_id(case):
    return "-".join(case)


def is_symmetric(freq):
    return bool(np.array_equal(freq, -freq[::-1]))


def symmetric_name(name):
    """Whether grid `name` is symmetric (known from its construction; the tests check it)."""
    return name in ("knot_odd", "knot_even", "geom", "two_density", "outlier", "dups") \
        or name.startswith("sym_")


SYMMETRIC_CASES = [c for c in CASES if symmetric_name(c[1])]


def guess_unsettled(freq, values):
    """numpy replica of k_items' bound shortcut: the share of (value, side) pairs, over the
    values inside the grid's span and both searchsorted sides, whose bound the three grid values
    around the linear guess g = floor((v - f0) (nf - 1) / span) do not settle, i.e. whose
    searchsorted index is not in {g, g + 1}."""
    freq = np.asarray(freq, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    nf = len(freq)
    f0, span = freq[0], freq[-1] - freq[0]
    v = v[(v >= f0) & (v <= freq[-1])]
    if v.size == 0:
        return 0.0
    gsc = (nf - 1) / span if span > 0.0 else 0.0
    g = np.clip(np.floor((v - f0) * gsc).astype(np.int64), 0, nf)
    bad = 0
    for side in ("left", "right"):
        k = np.searchsorted(freq, v, side)
        bad += int(np.count_nonzero((k != g) & (k != g + 1)))
    return bad / (2.0 * v.size)
