"""A plain reference of what the mode sum's interval records must satisfy.

The preparation (k_items, csrc/emrifd_prepare.hip) writes one `Item` per ((m, n) group, knot
interval). Besides coefficients a record carries three decisions the sum trusts without a per-bin
test: the safe bit (fdneg & 2), the K_{1/3} series length jser, and the envelope class (jser == 0:
A(w) as a degree-6 polynomial, theta(w) folded into the phase cubic, csrc/env_fit.inc). This module
evaluates the definitions those decisions rest on, from the trajectory spline coefficients `coefT`
([interval][coef][q], q: 0 Phi_phi, 1 Phi_r, 2 f_phi, 3 f_r, 4 f_phi', 5 f_r'; scipy PPoly order),
the call's inputs and the records' own lane ranges:

    F'(w)  = 3 F0 w^2 + 2 F1 w + F2,   Fc = m coefT[.][c][2] + n coefT[.][c][3]
    F''(w) = 3 G0 w^2 + 2 G1 w + G2,   Gc = m coefT[.][c][4] + n coefT[.][c][5]
    |y|    = 2 pi |F'|^3 / (3 F''^2)
    A      = rho(y) / sqrt|F'|,  rho = sum_j KRH_j u^j,  u = 1 / y^2
    theta  = -+ KTH0 / |y| sum_j KTHN_j u^j   (- for F' < 0)
    Phi    = m Phi_phi + n Phi_r (cubic in w)

in np.longdouble (mpmath for the cross-check of tests/test_records_ref.py), not in the device's
operation order. The constants are parsed out of the package's csrc at import, so the reference
follows the committed tables. Two float64 restatements predict the class only: the |y| lower bound
of build_item and env_fit's acceptance (7 Chebyshev nodes, 8 check points).
"""

import os
import re
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "emri_frequencydomainwaveforms_amd", "csrc")
_NUM = r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?"


def _values(txt, name):
    """The numbers of `name`'s initialiser in C source `txt` (scalar, array or matrix), as
    decimal strings."""
    mt = re.search(r"\b" + name + r"\b\s*(?:\[[^\]]*\]\s*)*=\s*([^;]+);", txt)
    if mt is None:
        raise KeyError(name)
    return re.findall(_NUM, mt.group(1))


def load_constants():
    def read(f):
        with open(os.path.join(CSRC, f)) as fh:
            return fh.read()
    env, spa = read("env_fit.inc"), read("spa_tables.inc")
    con, lay = read("emrifd_constants.h"), read("emrifd_layout.h")
    c = SimpleNamespace()
    c.text = {}   # the decimal strings (mpmath reads them at full precision)
    for name, txt in (("ENV_TOL_A", env), ("ENV_TOL_T", env), ("ENV_MIN_Y", env), ("KTH0", con),
                      ("FDD_SCALE", con), ("TWO_PI", con), ("ENV_AMP_SCALE", lay)):
        (v,) = _values(txt, name)
        c.text[name] = v
        setattr(c, name, float(v))
    c.ENV_DEG = int(_values(env, "ENV_DEG")[0])
    c.FAST_J = int(_values(con, "FAST_J")[0])
    for name, txt in (("JSER_Y", spa), ("KRH", spa), ("KTHN", spa)):
        c.text[name] = _values(spa, name)
        setattr(c, name, np.array([float(v) for v in c.text[name]]))
    c.ENV_W7 = np.array([float(v) for v in _values(env, "ENV_W7")]).reshape(7, 7)
    c.ENV_W3 = np.array([float(v) for v in _values(env, "ENV_W3")]).reshape(4, 7)
    assert c.ENV_DEG == 6 and len(c.JSER_Y) == 7 and len(c.KRH) == 4 and len(c.KTHN) == 4
    return c


C = load_constants()
NDENSE = 513   # uniform points of [0, dtj] per envelope record
# env_fit's nodes and check points on [0, 1]: the zeros and the extrema of T_7
NODES = 0.5 * (1.0 + np.cos((2 * np.arange(7) + 1) * np.pi / 14))
CHECKS = 0.5 * (1.0 - np.cos(np.arange(8) * np.pi / 7))


def _ld(text):
    return LD(text) if isinstance(text, str) else np.array([LD(v) for v in text])


def horner(coef, w):
    """sum_i coef[..., i] w^(n - 1 - i) (highest power first), coef's rows aligned with w."""
    v = coef[..., 0] + 0 * w
    for i in range(1, coef.shape[-1]):
        v = v * w + coef[..., i]
    return v


def env_exact(fq, gq, fdneg, w, one=LD):
    """(A, theta, |y|) of the definitions at w: fq, gq the F', F'' quadratics (highest power
    first, rows aligned with w), fdneg the record's sign bit; in the arithmetic of `one`."""
    if one is LD:
        krh, kthn = _ld(C.text["KRH"]), _ld(C.text["KTHN"])
        kth0, twopi, sqrt = _ld(C.text["KTH0"]), 2 * np.arccos(LD(-1)), np.sqrt
    else:
        krh, kthn, kth0, twopi, sqrt = C.KRH, C.KTHN, C.KTH0, 2 * np.pi, np.sqrt
    fp, fpp = horner(fq, w), horner(gq, w)
    afp = np.abs(fp)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = twopi * afp ** 3 / (3 * fpp * fpp)
        iy = 1 / y
        u = iy * iy
        rho = ((krh[3] * u + krh[2]) * u + krh[1]) * u + krh[0]
        thn = iy * (((kthn[3] * u + kthn[2]) * u + kthn[1]) * u + kthn[0])
        A = rho / sqrt(afp)
    return A, np.where(fdneg, -kth0, kth0) * thn, y


def env_exact_mp(fq, gq, fdneg, w, dps=40):
    """env_exact for one record in mpmath (fq, gq, w: float64)."""
    import mpmath as mp
    with mp.workdps(dps):
        fq, gq, w = [mp.mpf(float(v)) for v in fq], [mp.mpf(float(v)) for v in gq], mp.mpf(float(w))
        fp = (fq[0] * w + fq[1]) * w + fq[2]
        fpp = (gq[0] * w + gq[1]) * w + gq[2]
        y = 2 * mp.pi * abs(fp) ** 3 / (3 * fpp ** 2)
        u = 1 / y ** 2
        rho = sum(mp.mpf(c) * u ** j for j, c in enumerate(C.text["KRH"]))
        thn = sum(mp.mpf(c) * u ** j for j, c in enumerate(C.text["KTHN"])) / y
        th = (-1 if fdneg else 1) * mp.mpf(C.text["KTH0"]) * thn
        return rho / mp.sqrt(abs(fp)), th, y


def _ranges(lo, hi):
    """(row, index) of every index of the ranges [lo[r], hi[r])."""
    cnt = np.maximum(hi - lo, 0).astype(np.int64)
    row = np.repeat(np.arange(len(lo)), cnt)
    start = np.cumsum(cnt) - cnt
    idx = np.arange(cnt.sum()) - np.repeat(start, cnt) + np.repeat(lo.astype(np.int64), cnt)
    return row, idx


class Records:
    """Every (group, interval) record of one preparation, flattened [G * ni], with the reference
    quantities built from coefT. t, freq: the call's knot times and grid; gm, gn: the groups;
    klo, khi [G * ni][2]: the lane ranges; paired: the grid was declared symmetric; members [G]:
    harmonics per group."""

    def __init__(self, coefT, t, gm, gn, klo, khi, freq, paired, members=None):
        coefT = np.asarray(coefT, dtype=np.float64)
        self.t, self.freq, self.paired = np.asarray(t, np.float64), np.asarray(freq), bool(paired)
        ni, G = len(t) - 1, len(gm)
        self.ni, self.G = ni, G
        self.g = np.repeat(np.arange(G), ni)
        self.j = np.tile(np.arange(ni), G)
        self.m, self.n = np.asarray(gm)[self.g], np.asarray(gn)[self.g]
        self.klo, self.khi = np.asarray(klo).reshape(-1, 2), np.asarray(khi).reshape(-1, 2)
        self.nl = (self.khi - self.klo).sum(axis=1)
        self.lanes = self.nl > 0
        self.mult = np.where(self.m != 0, 2, 1) if paired else np.ones_like(self.m)
        self.evals = self.nl.astype(np.int64) * self.mult
        self.members = (np.ones(G, np.int64) if members is None else np.asarray(members))[self.g]
        self.tj = self.t[self.j]
        self.dt = self.t[self.j + 1] - self.t[self.j]
        ct = coefT[self.j]                       # [N][4][8]
        m64, n64 = self.m.astype(np.float64)[:, None], self.n.astype(np.float64)[:, None]
        mL, nL = m64.astype(LD), n64.astype(LD)
        ctL = ct.astype(LD)
        self.terms = {}
        # float64 as numpy rounds it (the restatements), longdouble for the reference
        self.phi64 = m64 * ct[:, :, 0] + n64 * ct[:, :, 1]
        self.phi = mL * ctL[:, :, 0] + nL * ctL[:, :, 1]                   # cubic, [N][4]
        k = np.array([3.0, 2.0, 1.0])
        self.F64 = m64 * ct[:, :3, 2] + n64 * ct[:, :3, 3]
        self.G64 = m64 * ct[:, :3, 4] + n64 * ct[:, :3, 5]
        self.fq64, self.gq64 = k * self.F64, k * self.G64                  # F', F'' quadratics
        self.fq = k.astype(LD) * (mL * ctL[:, :3, 2] + nL * ctL[:, :3, 3])
        self.gq = k.astype(LD) * (mL * ctL[:, :3, 4] + nL * ctL[:, :3, 5])
        # magnitude of the larger product of each combination (the scale of its rounding)
        self.tmax = {q: np.maximum(np.abs(m64 * ct[:, :, a]), np.abs(n64 * ct[:, :, b]))
                     for q, (a, b) in (("phi", (0, 1)), ("F", (2, 3)), ("G", (4, 5)))}
        self.tsum = {q: np.abs(m64 * ct[:, :, a]) + np.abs(n64 * ct[:, :, b])
                     for q, (a, b) in (("phi", (0, 1)), ("F", (2, 3)), ("G", (4, 5)))}
        # the record's sign as build_item takes it: F' at the midpoint
        h = 0.5 * self.dt
        self.fdneg_mid = ((self.fq64[:, 0] * h + self.fq64[:, 1]) * h + self.fq64[:, 2]) < 0.0

    # -- served bins ---------------------------------------------------------------------------
    def served(self, mask):
        """(record index, g) of every bin the records of `mask` serve: sub-branch s = 0 lanes k
        in [klo0, khi0) at g = -freq[k], s = 1 lanes in [klo1, khi1) at g = +freq[k]."""
        rec = np.flatnonzero(mask)
        r0, k0 = _ranges(self.klo[rec, 0], self.khi[rec, 0])
        r1, k1 = _ranges(self.klo[rec, 1], self.khi[rec, 1])
        return (np.concatenate([rec[r0], rec[r1]]),
                np.concatenate([-self.freq[k0], self.freq[k1]]))

    def dense(self, mask, npts=NDENSE):
        """(record index, w) of npts uniform points of [0, dtj] of the records of `mask`."""
        rec = np.flatnonzero(mask)
        s = np.linspace(0.0, 1.0, npts)
        return np.repeat(rec, npts), (self.dt[rec][:, None] * s[None, :]).ravel().astype(LD)

    # -- the definitions ----------------------------------------------------------------------
    def fprime(self, r, w):
        return horner(self.fq[r], w)

    def envelope(self, r, w, fdneg):
        """(A, theta, |y|) at (record r, w) with the records' sign bits fdneg [N]."""
        return env_exact(self.fq[r], self.gq[r], fdneg[r], w)

    def phase(self, r, w):
        return horner(self.phi[r], w)

    # -- float64 restatements that predict the class -------------------------------------------
    def ymin_bound(self):
        """build_item's lower bound of |y| over [0, dtj] (with its 10% margin): min |F'| and
        max |F''| from the quadratics' end points and vertices."""
        qv = lambda q, x: (q[:, 0] * x + q[:, 1]) * x + q[:, 2]  # noqa: E731
        f, g, dt = self.fq64, self.gq64, self.dt
        with np.errstate(divide="ignore", invalid="ignore"):
            fa, fb = f[:, 2], qv(f, dt)
            fdmin = np.minimum(np.abs(fa), np.abs(fb))
            fdmin = np.where(((fa > 0) != (fb > 0)) | (fa == 0) | (fb == 0), 0.0, fdmin)
            xv = np.where(f[:, 0] != 0, -f[:, 1] / (2.0 * f[:, 0]), -1.0)
            inside = (xv > 0) & (xv < dt)
            fv = qv(f, np.where(inside, xv, 0.0))
            fdmin = np.where(inside & ((fv > 0) != (fa > 0)), 0.0, fdmin)
            fdmin = np.where(inside, np.minimum(fdmin, np.abs(fv)), fdmin)
            gmax = np.maximum(np.abs(g[:, 2]), np.abs(qv(g, dt)))
            xg = np.where(g[:, 0] != 0, -g[:, 1] / (2.0 * g[:, 0]), -1.0)
            ing = (xg > 0) & (xg < dt)
            gmax = np.where(ing, np.maximum(gmax, np.abs(qv(g, np.where(ing, xg, 0.0)))), gmax)
            ymin = np.where(gmax > 0, C.TWO_PI * fdmin ** 3 / (3.0 * gmax * gmax) / 1.1, np.inf)
        return ymin

    def jser_of(self, ymin):
        """The series length build_item picks from its bound: the smallest J whose range holds."""
        J = np.full(len(ymin), C.FAST_J)
        for jj in range(C.FAST_J - 1, 0, -1):
            J = np.where(ymin >= C.JSER_Y[jj], jj, J)
        return J

    def env_fit(self, mask, fdneg):
        """env_fit's acceptance restated in float64 for the records of `mask`: interpolate A at
        the 7 Chebyshev nodes (ENV_W7) and theta's truncated series (ENV_W3), check at the 8
        extrema of T_7. Returns (record index, ea / (ENV_TOL_A amax), et / ENV_TOL_T, a [.][7],
        th [.][4]); a record is accepted when both ratios are <= 1 (and finite)."""
        rec = np.flatnonzero(mask)
        f, g, dt, neg = self.fq64[rec], self.gq64[rec], self.dt[rec], fdneg[rec]

        def exact(s):
            return env_exact(f, g, neg, dt * s, one=np.float64)[:2]
        fa, ft = zip(*[exact(s) for s in NODES])
        fa, ft = np.stack(fa, axis=1), np.stack(ft, axis=1)          # [R][7]
        pw = dt[:, None] ** -np.arange(7)[None, :]
        a = ((fa @ C.ENV_W7.T) * pw)[:, ::-1]                         # highest power first
        th = ((ft @ C.ENV_W3.T) * pw[:, :4])[:, ::-1]
        amax, ea, et = np.zeros(len(rec)), np.zeros(len(rec)), np.zeros(len(rec))
        with np.errstate(invalid="ignore"):
            for s in CHECKS:
                A, T = exact(s)
                w = dt * s
                amax = np.fmax(amax, np.abs(A))
                ea = np.maximum(ea, np.abs(horner(a, w) - A))
                et = np.maximum(et, np.abs(horner(th, w) - T))
            ra, rt = ea / (C.ENV_TOL_A * amax), et / C.ENV_TOL_T
        ra, rt = np.where(np.isfinite(ra), ra, np.inf), np.where(np.isfinite(rt), rt, np.inf)
        return rec, ra, rt, a, th

    def predict(self, safe, env_on=True):
        """The class the gates of build_item give each record: (envelope [N] bool, undecided [N]
        bool, jser [N], ymin [N], check ratios (amplitude, phase) [N], NaN where the fit was not
        tried). safe: the device's safe bits (or all True to ignore them). Undecided: a check
        ratio within 1% of 1, or ymin within 1% of ENV_MIN_Y."""
        N = len(self.g)
        ymin = self.ymin_bound()
        cand = np.asarray(safe, bool) & (self.evals > 0) & (ymin >= 0.99 * C.ENV_MIN_Y)
        ra, rt = np.full(N, np.nan), np.full(N, np.nan)
        if cand.any():
            rec, a, b, _, _ = self.env_fit(cand, self.fdneg_mid)
            ra[rec], rt[rec] = a, b
        with np.errstate(invalid="ignore"):
            accept = (ra <= 1.0) & (rt <= 1.0)
            near = cand & (((ra >= 0.99) & (ra <= 1.01) & (rt <= 1.01)) |
                           ((rt >= 0.99) & (rt <= 1.01) & (ra <= 1.01)))
        near_y = cand & (np.abs(ymin - C.ENV_MIN_Y) <= 0.01 * C.ENV_MIN_Y) & (ra <= 1.01) \
            & (rt <= 1.01)
        env = cand & accept & (ymin >= C.ENV_MIN_Y) & bool(env_on)
        undecided = (near | near_y) & bool(env_on)
        return env, undecided, self.jser_of(ymin), ymin, ra, rt


def dense_fit_error(R, mask, fdneg, a, th):
    """Worst error of the fits (a [.][7], th [.][4] of the records of `mask`, in flatnonzero
    order) against the exact envelope on NDENSE points per record, as ratios to the tolerances:
    (amplitude [R], phase [R])."""
    rec = np.flatnonzero(mask)
    r, w = R.dense(mask)
    pos = np.repeat(np.arange(len(rec)), NDENSE)
    A, T, _ = R.envelope(r, w, fdneg)
    ea = np.abs(horner(a.astype(LD)[pos], w) - A).reshape(len(rec), NDENSE)
    et = np.abs(horner(th.astype(LD)[pos], w) - T).reshape(len(rec), NDENSE)
    amax = np.abs(A).reshape(len(rec), NDENSE).max(axis=1)
    return (ea.max(axis=1) / (C.ENV_TOL_A * amax)).astype(np.float64), \
        (et.max(axis=1) / C.ENV_TOL_T).astype(np.float64)


def scipy_coefT(d):
    """coefT as scipy builds it from the inputs d (t, phi_phi, phi_r, f_phi, f_r): not-a-knot
    cubic splines of the four trajectory arrays, and of the knot values of f_phi', f_r' (the
    derivative of the frequency splines at the knots)."""
    from scipy.interpolate import CubicSpline
    t = np.asarray(d["t"], np.float64)
    cols = [CubicSpline(t, np.asarray(d[k], np.float64)) for k in
            ("phi_phi", "phi_r", "f_phi", "f_r")]
    cols += [CubicSpline(t, cols[q].derivative()(t)) for q in (2, 3)]
    out = np.zeros((len(t) - 1, 4, 8))
    for q, cs in enumerate(cols):
        out[:, :, q] = cs.c.T
    return out


def host_groups(d):
    """(gm, gn, members) of the call's harmonics: the sorted distinct (m, n) and their sizes."""
    mn = np.stack([np.asarray(d["m"]), np.asarray(d["n"])], axis=1)
    u, cnt = np.unique(mn, axis=0, return_counts=True)
    return u[:, 0].astype(np.int32), u[:, 1].astype(np.int32), cnt


def host_lane_ranges(d, gm, gn, freq):
    """Unpaired lane ranges of every (group, interval) from numpy's searchsorted on the knot
    frequencies F = m f_phi + n f_r: s = 1 serves f in [xlo, xhi), s = 0 (all groups) f in
    (-xhi, -xlo]; m = 0 groups have no s = 1 lanes. (The device's run ends are open and its flat
    intervals empty; those records differ by a bin, which the CPU conditions do not depend on.)"""
    F = gm[:, None] * np.asarray(d["f_phi"])[None, :] + gn[:, None] * np.asarray(d["f_r"])[None, :]
    xlo, xhi = np.minimum(F[:, :-1], F[:, 1:]).ravel(), np.maximum(F[:, :-1], F[:, 1:]).ravel()
    lo0, hi0 = np.searchsorted(freq, -xhi, "right"), np.searchsorted(freq, -xlo, "right")
    lo1, hi1 = np.searchsorted(freq, xlo, "left"), np.searchsorted(freq, xhi, "left")
    part = np.repeat(gm != 0, F.shape[1] - 1)
    hi1 = np.where(part, hi1, lo1)
    return np.stack([lo0, lo1], axis=1), np.stack([hi0, hi1], axis=1)
