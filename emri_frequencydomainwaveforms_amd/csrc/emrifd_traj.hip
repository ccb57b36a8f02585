// emrifd_traj.hip -- the inspiral trajectory and the p0 root solve on the device, one wavefront
// per source (efd_traj_batch, efd_traj_p_at_t_batch; include/emrifd.h).
//
// STAND-IN PHYSICS, NOT FEW: this restates trajectory.py and csrc/emrifd_host.cpp, the same
// equations and the same integrator (scipy RK45's Dormand-Prince 5(4), its step control, dense
// output and terminal separatrix event; Brent's root for the event and for p0). The host forms,
// efd_host_trajectory and efd_host_p_at_t, are the reference.
//
// The right-hand side's cost is fundamental()'s 64-node trapezoid over the relativistic anomaly:
// lane i of the wave64 evaluates node i with the host's cosine table (traj_costab.inc, bit for
// bit), and every lane then adds the 64 nodes from LDS in the host's order. Everything else (the
// four state components, the six stages, the error norm, the controller, the event root) is
// wave-uniform: every lane carries the same values and takes the same branches, so no atomics
// are needed, and lane 0 stores the knots.
//
// The aim is the host's own steps, not merely a valid integration: the first steps' error
// estimates are rounding noise, so one differing last bit there moves the early knots by 3-30 %
// and the templates with them. The host unit is built with -ffp-contract=off; so is this one (the
// pragma below). Divisions and square roots are IEEE on both; the sums take the host's order; the
// three powers are formed correctly rounded (pow_25_35, pow_m02), which the host's std::pow is in
// 99.92 % of its calls. Where one of those calls differs the two integrations part by a last
// bit from there on.
//
// Every loop is bounded: accepted plus rejected steps of one integration by 4 EFD_TRAJ_MAX_LEN,
// the roots by 100 iterations, the bracket by 7 expansions. A source that hits a bound or fails
// the input checks writes its status word and its wave returns.
#include "emrifd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr double MTSUN_SI = 4.925491025543576e-06;
constexpr double YRSID_SI = 31558149.763545603;
constexpr double TWO_PI = 6.283185307179586476925286766559005768;
constexpr double DIST_TO_SEPARATRIX = 0.1;
constexpr int NCHI = 64;
constexpr int NY = 4;
constexpr int STEP_CAP = 4 * EFD_TRAJ_MAX_LEN;   // accepted + rejected steps of one integration
constexpr int ROOT_MAXITER = 100;
constexpr int BRACKET_MAX = 7;                   // 40 * 1.5^7 > 500

__constant__ double c_costab[NCHI] = {
#include "traj_costab.inc"
};

// scipy RK45 tableau, error weights and dense-output matrix (emrifd_host.cpp's)
__device__ constexpr double A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__device__ constexpr double B[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784,
                                    11.0 / 84};
__device__ constexpr double E[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920,
                                    17253.0 / 339200, -22.0 / 525, 1.0 / 40};
__device__ constexpr double P[7][4] = {
    {1.0, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
    {0.0, 0.0, 0.0, 0.0},
    {0.0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
    {0.0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
    {0.0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408,
     701980252875.0 / 199316789632},
    {0.0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
    {0.0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};

// The two sums of the quadrature over the wave64 in the host's order, ((x0 + x1) + x2) + ...:
// every lane stores its node to LDS; the lower half-wave then adds the 64 dt in lane order and
// the upper half-wave the 64 dphi (broadcast reads, one addition per node for the wave), and the
// two results are read from lanes 0 and 32 as wave-uniform values: the bits of emrifd_host.cpp's
// loop, in every lane. A butterfly costs a fraction of this, but its other summation order
// re-rolls the rounding noise that the first steps' error estimates consist of, and with it the
// early knots by 3-30 %: the device would be a third valid integration and its templates would
// differ from the host route's by up to 1e-1 of max|S|. The workgroup is this one
// wave, so the barriers are wave-wide; the control flow around every call is wave-uniform.
__device__ __forceinline__ void wave_sums_host_order(double dt, double dphi, double& sdt,
                                                     double& sdphi) {
    __shared__ double node[2][NCHI + 2];   // (+ 2: the columns start on different banks)
    const int lane = threadIdx.x & (NCHI - 1);
    __syncthreads();                       // the reads of the call before are done
    node[0][lane] = dt;
    node[1][lane] = dphi;
    __syncthreads();
    const double* col = node[lane >> 5];
    double a = 0.0;
#pragma unroll 16
    for (int i = 0; i < NCHI; ++i) a += col[i];
    const int lo = __double2loint(a), hi = __double2hiint(a);
    sdt = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
    sdphi = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
}

// Double-double helpers for the three powers below (explicit fma; the unit is built without
// contraction).
struct dd {
    double hi, lo;
};
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd fast_two_sum(double a, double b) {
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ dd dd_mul_d(dd a, double b) {
    dd p = two_prod(a.hi, b);
    p.lo = fma(a.lo, b, p.lo);
    return fast_two_sum(p.hi, p.lo);
}
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    p.lo += fma(a.hi, b.lo, a.lo * b.hi);
    return fast_two_sum(p.hi, p.lo);
}
// x^2.5 and x^3.5 correctly rounded (but for ties within 1e-30): x^2 sqrt(x), and that times x,
// in double-double. The host's std::pow is correctly rounded in 99.92 % of its calls (measured
// against these forms over 2e6 arguments), so the two agree bit for bit nearly always.
__device__ __forceinline__ void pow_25_35(double x, double& x25, double& x35) {
    const double s = sqrt(x);
    const dd sq = {s, fma(-s, s, x) / (2.0 * s)};
    const dd r25 = dd_mul(two_prod(x, x), sq);
    x25 = r25.hi;
    x35 = dd_mul_d(r25, x).hi;
}
// en^a, a = the double nearest -0.2 (-1/5 - 1.11e-17), correctly rounded likewise: one Newton
// step on y^-5 = en from the library's value in double-double, and the exponent's rounding
// as the factor 1 - 1.11e-17 ln(en).
__device__ __forceinline__ double pow_m02(double en) {
    const double y0 = pow(en, -1.0 / 5.0);
    const dd y2 = two_prod(y0, y0);
    const dd y4 = dd_mul(y2, y2);
    const dd y5 = dd_mul_d(y4, y0);
    const dd z = dd_mul_d(y5, en);
    const double r = (1.0 - z.hi) - z.lo;
    return y0 + y0 * (r / 5.0 - 1.1102230246251565e-17 * log(en));
}

// Omega_phi, Omega_r of a Schwarzschild eccentric equatorial orbit (emrifd_host.cpp
// fundamental()): this lane's node of the trapezoid, c = cos(2 pi lane / 64)
__device__ __forceinline__ void fundamental(double p, double e, double c, double& om_phi,
                                            double& om_r) {
    const double k = (p - 2.0) * (p - 2.0) - 4.0 * e * e;
    const double ec = e * c;
    const double den = p - 6.0 - 2.0 * ec;
    const double dphi = sqrt(p / den);
    const double q = 1.0 + ec;
    const double dt = p * p / ((p - 2.0 - 2.0 * ec) * q * q) * sqrt(k / den);
    double sdt, sdphi;
    wave_sums_host_order(dt, dphi, sdt, sdphi);
    const double t_r = sdt / NCHI * TWO_PI, phi_r = sdphi / NCHI * TWO_PI;
    om_phi = phi_r / t_r;
    om_r = TWO_PI / t_r;
}

// d/d tau of (p, e, Phi_phi, Phi_r), tau = t / M (trajectory.py _pn_rhs)
__device__ __forceinline__ void rhs(const double* y, double q, double c, double* f) {
    const double p = y[0], e = y[1], e2 = e * e;
    const double x = 1.0 - e2;
    const double a = p / x;
    double x25, x35;
    pow_25_35(x, x25, x35);
    const double da = -(64.0 / 5.0) * q / (a * a * a * x35) *
                      (1.0 + 73.0 / 24.0 * e2 + 37.0 / 96.0 * e2 * e2);
    const double de = -(304.0 / 15.0) * q * e / (a * a * a * a * x25) *
                      (1.0 + 121.0 / 304.0 * e2);
    f[0] = (1.0 - e2) * da - 2.0 * a * e * de;
    f[1] = de;
    fundamental(p, e, c, f[2], f[3]);
}

__device__ __forceinline__ double sep_event(const double* y) {
    return y[0] - (6.0 + 2.0 * y[1]) - DIST_TO_SEPARATRIX;
}

// std::min / std::max as the host writes them (their NaN behaviour included)
__device__ __forceinline__ double min_h(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double max_h(double a, double b) { return (a < b) ? b : a; }

// One step of Brent's method (scipy brentq's loop body, emrifd_host.cpp brentq): from the
// bracket state with fcur = f(xcur) known, either converges (returns true; the root is xcur) or
// moves xcur to the next abscissa, whose f the caller supplies before the next call.
struct Brent {
    double xpre, xcur, xblk, fpre, fcur, fblk, spre, scur;
};
__device__ __forceinline__ void brent_init(Brent& b, double xa, double fa, double xb, double fb) {
    b.xpre = xa; b.fpre = fa; b.xcur = xb; b.fcur = fb;
    b.xblk = 0.0; b.fblk = 0.0; b.spre = 0.0; b.scur = 0.0;
}
__device__ __forceinline__ bool brent_step(Brent& b, double xtol, double rtol) {
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
__device__ __forceinline__ void dense(const double (*Q)[4], const double* y, double t, double h,
                                      double tt, double* out) {
    const double x = (tt - t) / h;
    const double pw[4] = {x, x * x, x * x * x, x * x * x * x};
    for (int k = 0; k < NY; ++k) {
        double acc = 0.0;
        for (int c = 0; c < 4; ++c) acc += Q[k][c] * pw[c];
        out[k] = h * acc + y[k];
    }
}

// lane 0 stores knot i of the source's slab [7][max_len]; the caller has checked i < max_len
__device__ __forceinline__ void store_knot(double* slab, int max_len, int i, double t,
                                           const double* y, double f_phi, double f_r) {
    if ((threadIdx.x & (NCHI - 1)) == 0) {
        slab[i] = t;
        slab[(size_t)max_len + i] = y[0];
        slab[2 * (size_t)max_len + i] = y[1];
        slab[3 * (size_t)max_len + i] = y[2];
        slab[4 * (size_t)max_len + i] = y[3];
        slab[5 * (size_t)max_len + i] = f_phi;
        slab[6 * (size_t)max_len + i] = f_r;
    }
}

// The sparse inspiral (emrifd_host.cpp integrate()): the accepted RK45 steps from (0, y0) to the
// separatrix event or tau_max. STORE: knot i goes to slab as (tau tscale, y, Omega / fden) and a
// knot past max_len ends the integration with EFD_TRAJ_TOO_LONG (nothing past max_len knots is
// written). Returns the status; *nt the knot count and *tau_end the last knot's tau on success.
template <bool STORE>
__device__ int integrate(double p0, double e0, double pp0, double pr0, double q, double tau_max,
                         double rtol, double atol, double c, double* slab, int max_len,
                         double tscale, double fden, int* nt, double* tau_end) {
    double t = 0.0, y[NY] = {p0, e0, pp0, pr0}, f[NY];
    rhs(y, q, c, f);
    double h_abs = min_h(1e-3 * tau_max, 1e4);   // first_step (trajectory.py)
    int n = 0, steps = 0;
    if (STORE) store_knot(slab, max_len, n, 0.0, y, f[2] / fden, f[3] / fden);
    ++n;
    double g = sep_event(y);
    double K[7][NY];
    while (t < tau_max) {
        const double min_step = 10.0 * fabs(nextafter(t, INFINITY) - t);
        if (h_abs < min_step) h_abs = min_step;
        bool accepted = false, rejected = false;
        double t_new = t, y_new[NY], f_new[NY], h = 0.0;
        while (!accepted) {
            if (h_abs < min_step) return EFD_TRAJ_STEP_FAILED;
            if (++steps > STEP_CAP) return EFD_TRAJ_STEP_CAP;
            h = h_abs;
            t_new = t + h;
            if (t_new - tau_max > 0) t_new = tau_max;
            h = t_new - t;
            h_abs = fabs(h);
            for (int k = 0; k < NY; ++k) K[0][k] = f[k];
#pragma unroll
            for (int s = 1; s < 6; ++s) {
                double ys_[NY];
                for (int k = 0; k < NY; ++k) {
                    double dy = 0.0;
                    for (int r = 0; r < s; ++r) dy += K[r][k] * A[s][r];
                    ys_[k] = y[k] + dy * h;
                }
                rhs(ys_, q, c, K[s]);
            }
            for (int k = 0; k < NY; ++k) {
                double acc = 0.0;
                for (int r = 0; r < 6; ++r) acc += K[r][k] * B[r];
                y_new[k] = y[k] + h * acc;
            }
            rhs(y_new, q, c, f_new);
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
                double factor = en == 0.0 ? 10.0 : min_h(10.0, 0.9 * pow_m02(en));
                if (rejected) factor = min_h(1.0, factor);
                h_abs *= factor;
                accepted = true;
            } else {
                h_abs *= max_h(0.2, 0.9 * pow_m02(en));
                rejected = true;
            }
        }
        const double g_new = sep_event(y_new);
        if (g >= 0.0 && g_new <= 0.0) {   // terminal event (direction -1): root of the dense output
            double Q[NY][4];
            for (int k = 0; k < NY; ++k)
                for (int cc = 0; cc < 4; ++cc) {
                    double acc = 0.0;
                    for (int r = 0; r < 7; ++r) acc += K[r][k] * P[r][cc];
                    Q[k][cc] = acc;
                }
            const double eps4 = 4.0 * 2.220446049250313e-16;
            double yy[NY];
            // brentq(f, t, t_new): f(t) = g's dense-output value, f(t_new) likewise
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
                    if (brent_step(b, eps4, eps4)) break;
                    dense(Q, y, t, h, b.xcur, yy);
                    b.fcur = sep_event(yy);
                }
                te = b.xcur;
            }
            double ye[NY];
            dense(Q, y, t, h, te, ye);
            if (STORE) {
                if (n >= max_len) return EFD_TRAJ_TOO_LONG;
                double op, orr;
                fundamental(ye[0], ye[1], c, op, orr);
                store_knot(slab, max_len, n, te * tscale, ye, op / fden, orr / fden);
            }
            ++n;
            *nt = n;
            *tau_end = te;
            return EFD_TRAJ_OK;
        }
        g = g_new;
        t = t_new;
        for (int k = 0; k < NY; ++k) { y[k] = y_new[k]; f[k] = f_new[k]; }
        if (STORE) {
            if (n >= max_len) return EFD_TRAJ_TOO_LONG;
            store_knot(slab, max_len, n, t * tscale, y, f[2] / fden, f[3] / fden);
        }
        ++n;
    }
    *nt = n;
    *tau_end = t;
    return EFD_TRAJ_OK;
}

__device__ __forceinline__ bool finite_all(const efd_traj_source& s) {
    return isfinite(s.M) && isfinite(s.mu) && isfinite(s.p0) && isfinite(s.e0) &&
           isfinite(s.Phi_phi0) && isfinite(s.Phi_r0) && isfinite(s.T) && isfinite(s.rtol) &&
           isfinite(s.atol);
}

// one wave64 per source: blockIdx.x is the source
__global__ __launch_bounds__(NCHI) void k_traj_rk45(const efd_traj_source* __restrict__ src,
                                                    int count, int max_len,
                                                    double* __restrict__ knots,
                                                    int32_t* __restrict__ nt,
                                                    int32_t* __restrict__ status) {
    const int w = blockIdx.x;
    if (w >= count) return;
    const int lane = threadIdx.x & (NCHI - 1);
    const efd_traj_source s = src[w];
    int st = EFD_TRAJ_OK, n = 0;
    if (!finite_all(s) || !(s.M > 0) || !(s.mu > 0) || !(s.T > 0) || !(s.rtol > 0) ||
        !(s.atol > 0) || !(s.p0 - (6.0 + 2.0 * s.e0) > DIST_TO_SEPARATRIX)) {
        st = EFD_TRAJ_BAD_SOURCE;
    } else {
        const double tscale = s.M * MTSUN_SI;
        const double fden = TWO_PI * s.M * MTSUN_SI;   // (the host's divisor)
        double tau_end;
        st = integrate<true>(s.p0, s.e0, s.Phi_phi0, s.Phi_r0, s.mu / s.M,
                             s.T * YRSID_SI / tscale, s.rtol, s.atol, c_costab[lane],
                             knots + (size_t)w * 7 * (size_t)max_len, max_len, tscale, fden, &n,
                             &tau_end);
    }
    if (lane == 0) {
        status[w] = st;
        if (st == EFD_TRAJ_OK) nt[w] = n;
    }
}

// efd_host_p_at_t per source: the default bracket, the upper end times 1.5 until 500, Brent on
// t_plunge(p0) - t_out. One integration per pass of the loop (a single call site); the bracket's
// end values are reused as Brent's first two (the function is deterministic, so they are the
// bits the host recomputes).
__global__ __launch_bounds__(NCHI) void k_traj_p_at_t(const efd_traj_source* __restrict__ src,
                                                      int count, double xtol, double rtol_root,
                                                      double* __restrict__ p0_out,
                                                      int32_t* __restrict__ status) {
    const int w = blockIdx.x;
    if (w >= count) return;
    const int lane = threadIdx.x & (NCHI - 1);
    efd_traj_source s = src[w];
    s.p0 = 0.0;   // ignored
    int st = EFD_TRAJ_OK;
    double root = NAN;
    if (!finite_all(s) || !(s.M > 0) || !(s.mu > 0) || !(s.T > 0) || !(s.rtol > 0) ||
        !(s.atol > 0) || !isfinite(xtol) || !isfinite(rtol_root)) {
        st = EFD_TRAJ_BAD_SOURCE;
    } else {
        const double t_out = s.T;
        const double tscale = s.M * MTSUN_SI;
        const double tau_max = (2.0 * t_out + 1.0) * YRSID_SI / tscale;
        const double rt = max_h(rtol_root, 4 * 2.220446049250313e-16);
        const double c = c_costab[lane];
        const double lo = 6.0 + 2.0 * s.e0 + DIST_TO_SEPARATRIX + 1e-3;
        double hi = 40.0, flo = 0.0, x = lo;
        int phase = 0, expansions = 0, iters = 0;
        Brent b;
        bool done = false;
        // 1 + (1 + BRACKET_MAX) + ROOT_MAXITER integrations at the most
        for (int pass = 0; pass < 2 + BRACKET_MAX + ROOT_MAXITER && !done; ++pass) {
            int n;
            double tau_end;
            st = integrate<false>(x, s.e0, 0.0, 0.0, s.mu / s.M, tau_max, s.rtol, s.atol, c,
                                  nullptr, 0, tscale, 1.0, &n, &tau_end);
            if (st != EFD_TRAJ_OK) break;
            const double fx = tau_end * tscale / YRSID_SI - t_out;
            if (phase == 0) {
                if (fx > 0) { st = EFD_TRAJ_NO_BRACKET; break; }   // t_out shorter than the plunge
                flo = fx;                                           // from the buffer
                phase = 1;
                x = hi;
                continue;
            }
            if (phase == 1) {
                if (fx < 0) {
                    hi *= 1.5;
                    if (hi > 500 || ++expansions > BRACKET_MAX) { st = EFD_TRAJ_NO_BRACKET; break; }
                    x = hi;
                    continue;
                }
                if (flo == 0.0) { root = lo; done = true; break; }
                if (fx == 0.0) { root = hi; done = true; break; }
                brent_init(b, lo, flo, hi, fx);
                phase = 2;
            } else {
                b.fcur = fx;
            }
            if (iters++ >= ROOT_MAXITER || brent_step(b, xtol, rt)) {
                root = b.xcur;
                done = true;
                break;
            }
            x = b.xcur;
        }
        if (st == EFD_TRAJ_OK && !done) st = EFD_TRAJ_STEP_CAP;   // (unreachable: the pass bound)
    }
    if (lane == 0) {
        status[w] = st;
        p0_out[w] = st == EFD_TRAJ_OK ? root : NAN;
    }
}

}  // namespace

extern "C" {

int efd_traj_batch(const efd_traj_source* src, int32_t count, int32_t max_len, double* knots,
                   int32_t* nt, int32_t* status, void* stream) {
    if (!src || !knots || !nt || !status)
        return fail(EFD_ERR_ARG, "efd_traj_batch: NULL pointer");
    if (count < 1) return fail(EFD_ERR_ARG, "efd_traj_batch: count < 1");
    if (max_len < 2 || max_len > EFD_TRAJ_MAX_LEN)
        return fail(EFD_ERR_ARG, "efd_traj_batch: max_len outside 2..EFD_TRAJ_MAX_LEN");
    hipLaunchKernelGGL(k_traj_rk45, dim3((unsigned)count), dim3(NCHI), 0, (hipStream_t)stream, src,
                       (int)count, (int)max_len, knots, nt, status);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_traj_p_at_t_batch(const efd_traj_source* src, int32_t count, double xtol,
                          double rtol_root, double* p0, int32_t* status, void* stream) {
    if (!src || !p0 || !status) return fail(EFD_ERR_ARG, "efd_traj_p_at_t_batch: NULL pointer");
    if (count < 1) return fail(EFD_ERR_ARG, "efd_traj_p_at_t_batch: count < 1");
    hipLaunchKernelGGL(k_traj_p_at_t, dim3((unsigned)count), dim3(NCHI), 0, (hipStream_t)stream,
                       src, (int)count, xtol, rtol_root, p0, status);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

}  // extern "C"
