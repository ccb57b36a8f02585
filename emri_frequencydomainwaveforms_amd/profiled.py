"""What Likelihood.parts' pair (<d|h>, <h|h>) is for: host arithmetic on float64 arrays [B], no
GPU. likelihood.py re-exports the public names."""

import numpy as np


def profile_none(d_d, re_dh, h_h):
    """logL = -1/2 (d_d - 2 Re <d|h> + <h|h>)."""
    return -0.5 * (d_d - 2.0 * np.asarray(re_dh, dtype=np.float64)
                   + np.asarray(h_h, dtype=np.float64))


def profile_amplitude(d_d, re_dh, h_h):
    """The logL maximised over an overall amplitude A >= 0 of the template, in closed form:
    (-1/2 d_d + 1/2 max(Re <d|h>, 0)^2 / <h|h>, A_hat = max(Re <d|h>, 0) / <h|h>); a walker
    with <h|h> = 0 (no template) has A_hat = 0 and no gain."""
    re = np.maximum(np.asarray(re_dh, dtype=np.float64), 0.0)
    hh = np.asarray(h_h, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(hh > 0.0, re / hh, 0.0)
    return -0.5 * d_d + 0.5 * re * A, A


# k of the break points u* +- k sigma of the distance quadrature's panels
_PEAK_K = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 16.0, 24.0, 40.0)
_PANEL_MAX = 0.25    # the widest panel in log u
DISTANCE_NODES = 16  # Gauss-Legendre nodes per panel


def _distance_panels(re, hh, u_lo, u_hi):
    """The panels' break points in t = log u for one walker: the range's ends, the Gaussian
    factor's u* +- k sigma (u* = Re <d|h> / <h|h>, sigma = <h|h>^(-1/2)), a geometric ladder in
    from each end at that end's decay length 1 / |Re <d|h> - u <h|h>| (a peak far outside the
    range leaves an exponential against the nearer end), and a uniform split of what is still
    wider than _PANEL_MAX."""
    pts = [u_lo, u_hi]
    if hh > 0.0:
        us, sg = re / hh, hh ** -0.5
        for k in _PEAK_K:
            pts += [us - k * sg, us + k * sg]
        pts.append(us)
    for edge, sign in ((u_lo, 1.0), (u_hi, -1.0)):
        slope = abs(re - edge * hh)
        if slope > 0.0:
            step = 1.0 / slope
            while step < u_hi - u_lo:
                pts.append(edge + sign * step)
                step *= 2.0
    t = np.log(np.unique(np.clip(np.asarray(pts, dtype=np.float64), u_lo, u_hi)))
    out = [t[:1]]
    for a, b in zip(t[:-1], t[1:]):
        m = max(1, int(np.ceil((b - a) / _PANEL_MAX)))
        out.append(a + (b - a) * np.arange(1, m + 1) / m)
    return np.concatenate(out)


def marginalize_distance(d_d, re_dh, h_h, dist_ref, dist_range, prior_power=2,
                         nodes=DISTANCE_NODES):
    """log of the likelihood marginalised over the distance D of a template made at dist_ref,
      log int pi(D) exp(-1/2 d_d + u Re <d|h> - 1/2 u^2 <h|h>) dD,  u = dist_ref / D,
    with pi proportional to D^prior_power, normalised on dist_range = (lo, hi). Per walker a
    composite Gauss-Legendre rule in t = log u (dD = -D dt: the power-law prior and Jacobian are
    smooth there) over _distance_panels' panels, `nodes` nodes each, summed in log-sum-exp form:
    finite for <h|h> = 0 (the integrand is then the prior alone, log = -1/2 d_d) and for peaks
    of any height."""
    re = np.atleast_1d(np.asarray(re_dh, dtype=np.float64))
    hh = np.atleast_1d(np.asarray(h_h, dtype=np.float64))
    lo, hi = float(dist_range[0]), float(dist_range[1])
    if not (0.0 < lo < hi) or not dist_ref > 0.0:
        raise ValueError("marginalize_distance: 0 < lo < hi and dist_ref > 0")
    p = float(prior_power)
    # log of the prior's norm int_lo^hi D^p dD, with D in units of hi (no overflow)
    lognorm = (np.log(np.log(hi / lo)) if p == -1.0
               else np.log((1.0 - (lo / hi) ** (p + 1.0)) / (p + 1.0))) + (p + 1.0) * np.log(hi)
    u_lo, u_hi = dist_ref / hi, dist_ref / lo
    x, wq = np.polynomial.legendre.leggauss(int(nodes))
    out = np.empty(len(re), dtype=np.float64)
    for i in range(len(re)):
        t = _distance_panels(re[i], hh[i], u_lo, u_hi)
        a, b = t[:-1, None], t[1:, None]
        tt = 0.5 * (a + b) + 0.5 * (b - a) * x[None, :]
        ww = 0.5 * (b - a) * wq[None, :]
        u = np.exp(tt)
        # pi(D) dD = D^(p + 1) dt / norm, D = dist_ref / u
        L = np.log(ww) + (p + 1.0) * (np.log(dist_ref) - tt) + u * re[i] - 0.5 * u * u * hh[i]
        m = L.max()
        out[i] = m + np.log(np.exp(L - m).sum()) - lognorm
    return -0.5 * d_d + out


class ProfiledLikelihood:
    """A Likelihood's logL with the template's overall amplitude (the source's distance) taken
    out, from Likelihood.parts' pair: a callable (params, **kwargs) -> float64 [B] that a sampler
    takes as its log-likelihood. The parameters go through the likelihood's own __call__ (its
    transforms and subset batching).

    mode: "none", -1/2 (d_d - 2 Re <d|h> + <h|h>): the plain logL from the pair;
          "amplitude", profile_amplitude's closed form; `last` then holds A_hat and, with
            dist_ref, D_hat = dist_ref / A_hat of the last call;
          "distance", marginalize_distance over dist_range with the prior D^prior_power, the
            templates being made at distance dist_ref.
    snr(params, **kwargs) returns (sqrt <h|h>, Re <d|h> / sqrt <h|h>): the optimal and the
    matched-filter SNR of every walker."""

    MODES = ("none", "amplitude", "distance")

    def __init__(self, like, mode, dist_ref=None, dist_range=None, prior_power=2):
        if mode not in self.MODES:
            raise ValueError(f"mode: one of {self.MODES}")
        if mode == "distance" and (dist_ref is None or dist_range is None):
            raise ValueError("mode 'distance' needs dist_ref and dist_range")
        self.like, self.mode = like, mode
        self.dist_ref, self.dist_range, self.prior_power = dist_ref, dist_range, prior_power
        self.last = {}

    def parts(self, params, **kwargs):
        """(<d|h> complex128 [B], <h|h> float64 [B]) through the likelihood's __call__."""
        like = self.like
        keep = like.separate_d_h
        like.separate_d_h = True
        try:
            d_h, h_h = like(params, **kwargs)
        finally:
            like.separate_d_h = keep
        return d_h, h_h

    def combine(self, d_d, d_h, h_h):
        """The mode's logL from given numbers (host arithmetic only)."""
        re = np.real(d_h)
        if self.mode == "none":
            return profile_none(d_d, re, h_h)
        if self.mode == "amplitude":
            ll, A = profile_amplitude(d_d, re, h_h)
            self.last = {"A_hat": A}
            if self.dist_ref is not None:
                with np.errstate(divide="ignore"):
                    self.last["D_hat"] = np.where(A > 0.0, self.dist_ref / A, np.inf)
            return ll
        return marginalize_distance(d_d, re, h_h, self.dist_ref, self.dist_range,
                                    self.prior_power)

    def __call__(self, params, **kwargs):
        d_h, h_h = self.parts(params, **kwargs)
        return self.combine(self.like.d_d, d_h, h_h)

    def snr(self, params, **kwargs):
        d_h, h_h = self.parts(params, **kwargs)
        rho = np.sqrt(h_h)
        with np.errstate(divide="ignore", invalid="ignore"):
            return rho, np.where(rho > 0.0, np.real(d_h) / rho, 0.0)
