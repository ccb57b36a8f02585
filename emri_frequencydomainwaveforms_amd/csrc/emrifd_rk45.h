// emrifd_rk45.h -- the inspiral integrator and the p0 root solve, written once for the host
// (emrifd_host.cpp: efd_host_trajectory, efd_host_p_at_t) and the device (emrifd_traj.hip:
// efd_traj_batch, efd_traj_p_at_t_batch, one wave64 per source).
//
// STAND-IN PHYSICS, NOT FEW (trajectory.py): Peters-Mathews fluxes in (p, e), the exact
// Schwarzschild Omega_phi, Omega_r by a 64-node trapezoid over the relativistic anomaly, scipy's
// RK45 (Dormand-Prince 5(4), its step control, dense output and terminal separatrix event) and
// Brent's root (scipy brentq's loop) for the event and for p0.
//
// The device aims at the host's own steps, not merely a valid integration: the first steps' error
// estimates are rounding noise, so one differing last bit there moves the early knots by 3-30 %.
// That is why this text exists once. Both units are built without contraction (-ffp-contract=off
// for the host, #pragma clang fp contract(off) ahead of the include in the .hip), and the
// -ffast-math unit emrifd_modes.cpp must not include this file.
//
// Included inside the unit's own namespace, after <cmath> and with fabs, sqrt, nextafter and
// signbit in scope, with
//   EFD_HD     the functions' qualifiers (inline; __device__ __forceinline__)
//   EFD_TABLE  the tableaus' (constexpr; __device__ constexpr)
// defined. What legitimately differs between the two comes in through one side type S:
//   s.pow_25_35(x, x25, x35)   x^2.5 and x^3.5       host: std::pow; device: correctly rounded
//   s.pow_m02(en)              en^(-1/5)             likewise
//   s.quad_sums(p, e, k, sdt, sdphi)   the sums of quad_node over the NCHI nodes c_i =
//                              cos(2 pi i / NCHI), added in index order: a loop on the host, one
//                              node per lane on the device
//   s.step(steps)              0, or the status that ends an integration at its steps-th step
//                              (accepted and rejected ones)
//   s.knot(i, tau, y, om)      takes knot i: the state y at tau and om = (Omega_phi, Omega_r) at
//                              y, or om == nullptr when they are not known yet. Returns 0, or the
//                              status that ends the integration when knot i has no room
//   S::STEP_FAILED, S::NO_BRACKET   the side's status words; 0 is success on both

constexpr double MTSUN_SI = 4.925491025543576e-06;
constexpr double YRSID_SI = 31558149.763545603;
constexpr double TWO_PI = 6.283185307179586476925286766559005768;
constexpr double DIST_TO_SEPARATRIX = 0.1;
constexpr int NCHI = 64;
constexpr int NY = 4;
constexpr int ROOT_MAXITER = 100;
constexpr double EPS4 = 4.0 * 2.220446049250313e-16;

// scipy RK45 tableau, error weights and dense-output matrix
EFD_TABLE double A[6][5] = {{0, 0, 0, 0, 0},
                            {1.0 / 5, 0, 0, 0, 0},
                            {3.0 / 40, 9.0 / 40, 0, 0, 0},
                            {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                            {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                            {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
EFD_TABLE double B[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
EFD_TABLE double E[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200,
                         -22.0 / 525, 1.0 / 40};
EFD_TABLE double P[7][4] = {
    {1.0, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0.0, 0.0, 0.0, 0.0},
    {0.0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0.0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0.0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
    {0.0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0.0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};

// std::min / std::max in their operand order (their NaN behaviour included)
EFD_HD double min_h(double a, double b) { return (b < a) ? b : a; }
EFD_HD double max_h(double a, double b) { return (a < b) ? b : a; }

EFD_HD double sep_event(const double* y) { return y[0] - (6.0 + 2.0 * y[1]) - DIST_TO_SEPARATRIX; }

// the p0 solve's default lower bracket end: just outside the separatrix buffer
EFD_HD double p0_bracket_lo(double e0) { return 6.0 + 2.0 * e0 + DIST_TO_SEPARATRIX + 1e-3; }

// One node of the trapezoid of Omega_phi, Omega_r (frequencies.py): c = cos(chi),
// k = (p - 2)^2 - 4 e^2
EFD_HD void quad_node(double p, double e, double k, double c, double& dt, double& dphi) {
    const double ec = e * c;
    const double den = p - 6.0 - 2.0 * ec;
    dphi = sqrt(p / den);
    const double q = 1.0 + ec;
    dt = p * p / ((p - 2.0 - 2.0 * ec) * q * q) * sqrt(k / den);
}

// Omega_phi, Omega_r of a Schwarzschild eccentric equatorial orbit
template <class S>
EFD_HD void fundamental(S& s, double p, double e, double& om_phi, double& om_r) {
    const double k = (p - 2.0) * (p - 2.0) - 4.0 * e * e;
    double sdt, sdphi;
    s.quad_sums(p, e, k, sdt, sdphi);
    const double t_r = sdt / NCHI * TWO_PI, phi_r = sdphi / NCHI * TWO_PI;
    om_phi = phi_r / t_r;
    om_r = TWO_PI / t_r;
}

// d/d tau of (p, e, Phi_phi, Phi_r), tau = t / M (trajectory.py _pn_rhs)
template <class S>
EFD_HD void rhs(S& s, const double* y, double q, double* f) {
    const double p = y[0], e = y[1], e2 = e * e;
    const double x = 1.0 - e2;
    const double a = p / x;
    double x25, x35;
    s.pow_25_35(x, x25, x35);
    const double da = -(64.0 / 5.0) * q / (a * a * a * x35) *
                      (1.0 + 73.0 / 24.0 * e2 + 37.0 / 96.0 * e2 * e2);
    const double de = -(304.0 / 15.0) * q * e / (a * a * a * a * x25) *
                      (1.0 + 121.0 / 304.0 * e2);
    f[0] = (1.0 - e2) * da - 2.0 * a * e * de;
    f[1] = de;
    fundamental(s, p, e, f[2], f[3]);
}

// One step of Brent's method (scipy brentq's loop body): from the bracket state with
// fcur = f(xcur) known, either converges (returns true; the root is xcur) or moves xcur to the
// next abscissa, whose f the caller supplies before the next call. brentq(f, xa, xb) is: xa where
// f(xa) == 0, else xb where f(xb) == 0, else brent_init and at most ROOT_MAXITER steps.
struct Brent {
    double xpre, xcur, xblk, fpre, fcur, fblk, spre, scur;
};
EFD_HD void brent_init(Brent& b, double xa, double fa, double xb, double fb) {
    b.xpre = xa; b.fpre = fa; b.xcur = xb; b.fcur = fb;
    b.xblk = 0.0; b.fblk = 0.0; b.spre = 0.0; b.scur = 0.0;
}
EFD_HD bool brent_step(Brent& b, double xtol, double rtol) {
    if (b.fpre != 0.0 && b.fcur != 0.0 && (signbit(b.fpre) != signbit(b.fcur))) {
        b.xblk = b.xpre;
        b.fblk = b.fpre;
        b.spre = b.scur = b.xcur - b.xpre;
    }
    if (fabs(b.fblk) < fabs(b.fcur)) {
        b.xpre = b.xcur; b.xcur = b.xblk; b.xblk = b.xpre;
        b.fpre = b.fcur; b.fcur = b.fblk; b.fblk = b.fpre;
    }
    const double delta = (xtol + rtol * fabs(b.xcur)) / 2.0;
    const double sbis = (b.xblk - b.xcur) / 2.0;
    if (b.fcur == 0.0 || fabs(sbis) < delta) return true;
    if (fabs(b.spre) > delta && fabs(b.fcur) < fabs(b.fpre)) {
        double stry;
        if (b.xpre == b.xblk) {
            stry = -b.fcur * (b.xcur - b.xpre) / (b.fcur - b.fpre);   // interpolate
        } else {                                                      // extrapolate
            const double dpre = (b.fpre - b.fcur) / (b.xpre - b.xcur);
            const double dblk = (b.fblk - b.fcur) / (b.xblk - b.xcur);
            stry = -b.fcur * (b.fblk * dblk - b.fpre * dpre) / (dblk * dpre * (b.fblk - b.fpre));
        }
        if (2.0 * fabs(stry) < min_h(fabs(b.spre), 3.0 * fabs(sbis) - delta)) {
            b.spre = b.scur;   // good short step
            b.scur = stry;
        } else {
            b.spre = sbis;     // bisect
            b.scur = sbis;
        }
    } else {
        b.spre = sbis;
        b.scur = sbis;
    }
    b.xpre = b.xcur;
    b.fpre = b.fcur;
    if (fabs(b.scur) > delta) b.xcur += b.scur;
    else b.xcur += (sbis > 0 ? delta : -delta);
    return false;
}

// the dense output of the step (t, y) -> t + h at tt: y + h Q (x, x^2, x^3, x^4), x = (tt - t)/h
EFD_HD void dense(const double (*Q)[4], const double* y, double t, double h, double tt,
                  double* out) {
    const double x = (tt - t) / h;
    const double pw[4] = {x, x * x, x * x * x, x * x * x * x};
    for (int k = 0; k < NY; ++k) {
        double acc = 0.0;
        for (int c = 0; c < 4; ++c) acc += Q[k][c] * pw[c];
        out[k] = h * acc + y[k];
    }
}

// The sparse inspiral: the accepted RK45 steps from (0, y0) to the separatrix event or tau_max,
// each handed to s.knot. Returns 0, with *nt the knot count and *tau_end the last knot's tau, or
// the side's status: S::STEP_FAILED, or what s.step() or s.knot() returned.
template <class S>
EFD_HD int integrate(S& s, double p0, double e0, double pp0, double pr0, double q, double tau_max,
                     double rtol, double atol, int* nt, double* tau_end) {
    double t = 0.0, y[NY] = {p0, e0, pp0, pr0}, f[NY];
    rhs(s, y, q, f);
    double h_abs = min_h(1e-3 * tau_max, 1e4);   // first_step (trajectory.py)
    int n = 0, steps = 0;
    if (const int st = s.knot(n, 0.0, y, f + 2)) return st;
    ++n;
    double g = sep_event(y);
    double K[7][NY];
    while (t < tau_max) {
        const double min_step = 10.0 * fabs(nextafter(t, INFINITY) - t);
        if (h_abs < min_step) h_abs = min_step;
        bool accepted = false, rejected = false;
        double t_new = t, y_new[NY], f_new[NY], h = 0.0;
        while (!accepted) {
            if (h_abs < min_step) return S::STEP_FAILED;
            if (const int st = s.step(++steps)) return st;
            h = h_abs;
            t_new = t + h;
            if (t_new - tau_max > 0) t_new = tau_max;
            h = t_new - t;
            h_abs = fabs(h);
            for (int k = 0; k < NY; ++k) K[0][k] = f[k];
#pragma unroll
            for (int i = 1; i < 6; ++i) {
                double ys[NY];
                for (int k = 0; k < NY; ++k) {
                    double dy = 0.0;
                    for (int r = 0; r < i; ++r) dy += K[r][k] * A[i][r];
                    ys[k] = y[k] + dy * h;
                }
                rhs(s, ys, q, K[i]);
            }
            for (int k = 0; k < NY; ++k) {
                double acc = 0.0;
                for (int r = 0; r < 6; ++r) acc += K[r][k] * B[r];
                y_new[k] = y[k] + h * acc;
            }
            rhs(s, y_new, q, f_new);
            for (int k = 0; k < NY; ++k) K[6][k] = f_new[k];
            double en = 0.0;
            for (int k = 0; k < NY; ++k) {
                double ek = 0.0;
                for (int r = 0; r < 7; ++r) ek += K[r][k] * E[r];
                ek *= h;
                const double sc = atol + max_h(fabs(y[k]), fabs(y_new[k])) * rtol;
                en += (ek / sc) * (ek / sc);
            }
            en = sqrt(en) / sqrt((double)NY);
            if (en < 1.0) {
                double factor = en == 0.0 ? 10.0 : min_h(10.0, 0.9 * s.pow_m02(en));
                if (rejected) factor = min_h(1.0, factor);
                h_abs *= factor;
                accepted = true;
            } else {
                h_abs *= max_h(0.2, 0.9 * s.pow_m02(en));
                rejected = true;
            }
        }
        const double g_new = sep_event(y_new);
        if (g >= 0.0 && g_new <= 0.0) {   // terminal event (direction -1): root of the dense output
            double Q[NY][4];
            for (int k = 0; k < NY; ++k)
                for (int c = 0; c < 4; ++c) {
                    double acc = 0.0;
                    for (int r = 0; r < 7; ++r) acc += K[r][k] * P[r][c];
                    Q[k][c] = acc;
                }
            double yy[NY];
            // brentq(f, t, t_new, EPS4, EPS4) of f(tt) = sep_event(dense(tt))
            dense(Q, y, t, h, t, yy);
            const double fa = sep_event(yy);
            dense(Q, y, t, h, t_new, yy);
            const double fb = sep_event(yy);
            double te;
            if (fa == 0.0) te = t;
            else if (fb == 0.0) te = t_new;
            else {
                Brent b;
                brent_init(b, t, fa, t_new, fb);
                for (int i = 0; i < ROOT_MAXITER; ++i) {
                    if (brent_step(b, EPS4, EPS4)) break;
                    dense(Q, y, t, h, b.xcur, yy);
                    b.fcur = sep_event(yy);
                }
                te = b.xcur;
            }
            double ye[NY];
            dense(Q, y, t, h, te, ye);
            if (const int st = s.knot(n, te, ye, nullptr)) return st;
            ++n;
            *nt = n;
            *tau_end = te;
            return 0;
        }
        g = g_new;
        t = t_new;
        for (int k = 0; k < NY; ++k) { y[k] = y_new[k]; f[k] = f_new[k]; }
        if (const int st = s.knot(n, t, y, f + 2)) return st;
        ++n;
    }
    *nt = n;
    *tau_end = t;
    return 0;
}

// get_p_at_t: Brent's root in p0 of t_plunge(p0) - t_out over [lo, hi], hi times 1.5 until it
// brackets the root or passes 500 (from 40: seven times at the most). tau_max bounds each
// integration, tscale = M MTSUN_SI, rt the root's relative tolerance. One integration per pass of
// the loop (a single call site); the bracket's end values are Brent's first two. The pass bound
// holds for every positive double hi (1.5^2048 overflows), so it ends no solve early. Returns 0
// and *root, or S::NO_BRACKET (f(lo) > 0: t_out shorter than the plunge from lo; or no bracket by
// 500), or the status of the integration that failed.
constexpr int P0_MAX_PASSES = 2 + 2048 + ROOT_MAXITER;
template <class S>
EFD_HD int p_at_t(S& s, double e0, double q, double tau_max, double rtol, double atol,
                  double tscale, double t_out, double lo, double hi, double xtol, double rt,
                  double* root) {
    double flo = 0.0, x = lo;
    int phase = 0, iters = 0, st = 0;
    Brent b;
    bool done = false;
    for (int pass = 0; pass < P0_MAX_PASSES && !done; ++pass) {
        int n;
        double tau_end;
        st = integrate(s, x, e0, 0.0, 0.0, q, tau_max, rtol, atol, &n, &tau_end);
        if (st != 0) break;
        const double fx = tau_end * tscale / YRSID_SI - t_out;
        if (phase == 0) {
            if (fx > 0) { st = S::NO_BRACKET; break; }
            flo = fx;
            phase = 1;
            x = hi;
            continue;
        }
        if (phase == 1) {
            if (fx < 0) {
                hi *= 1.5;
                if (hi > 500) { st = S::NO_BRACKET; break; }
                x = hi;
                continue;
            }
            if (flo == 0.0) { *root = lo; done = true; break; }
            if (fx == 0.0) { *root = hi; done = true; break; }
            brent_init(b, lo, flo, hi, fx);
            phase = 2;
        } else {
            b.fcur = fx;
        }
        if (iters++ >= ROOT_MAXITER || brent_step(b, xtol, rt)) {
            *root = b.xcur;
            done = true;
            break;
        }
        x = b.xcur;
    }
    if (st == 0 && !done) st = S::NO_BRACKET;   // (unreachable: the pass bound)
    return st;
}
