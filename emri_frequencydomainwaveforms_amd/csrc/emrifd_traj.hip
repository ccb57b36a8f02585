// emrifd_traj.hip -- the inspiral trajectory and the p0 root solve on the device, one wavefront
// per source (efd_traj_batch, efd_traj_p_at_t_batch; include/emrifd.h).
//
// STAND-IN PHYSICS, NOT FEW. The equations, the integrator and the root solve are
// csrc/emrifd_rk45.h, the text that emrifd_host.cpp's efd_host_trajectory and efd_host_p_at_t
// compile too; this unit holds what is the device's own: the quadrature's sums over the wave, the
// three powers, the knot store and the loop bounds (the side type Wave below), and the kernels.
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
// the roots by 100 iterations, the bracket by 7 expansions: from hi = 40 it is p_at_t's hi > 500
// test that ends it (40 * 1.5^7 > 500); the driver's own pass bound, P0_MAX_PASSES, is the wider
// one that the host's hi overrides need and is never reached here. A source that hits a bound or
// fails the input checks writes its status word and its wave returns.
#include "emrifd_common.h"

#pragma clang fp contract(off)

namespace {

#define EFD_HD __device__ __forceinline__
#define EFD_TABLE __device__ constexpr
#include "emrifd_rk45.h"
#undef EFD_TABLE
#undef EFD_HD

constexpr int STEP_CAP = 4 * EFD_TRAJ_MAX_LEN;   // accepted + rejected steps of one integration

__constant__ double c_costab[NCHI] = {
#include "traj_costab.inc"
};

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

// Double-double helpers for Wave's three powers (explicit fma; the unit is built without
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

// The device's side of emrifd_rk45.h: one wave64 integrates one source. Wave counts the knots
// (the p0 solve needs each integration's end only); WaveStore also stores them.
struct Wave {
    static constexpr int STEP_FAILED = EFD_TRAJ_STEP_FAILED, NO_BRACKET = EFD_TRAJ_NO_BRACKET;
    double c;   // this lane's node of the trapezoid, cos(2 pi lane / NCHI)

    // x^2.5 and x^3.5 correctly rounded (but for ties within 1e-30): x^2 sqrt(x), and that times
    // x, in double-double. The host's std::pow is correctly rounded in 99.92 % of its calls
    // (measured against these forms over 2e6 arguments), so the two agree bit for bit nearly
    // always.
    __device__ __forceinline__ static void pow_25_35(double x, double& x25, double& x35) {
        const double s = sqrt(x);
        const dd sq = {s, fma(-s, s, x) / (2.0 * s)};
        const dd r25 = dd_mul(two_prod(x, x), sq);
        x25 = r25.hi;
        x35 = dd_mul_d(r25, x).hi;
    }
    // en^a, a = the double nearest -0.2 (-1/5 - 1.11e-17), correctly rounded likewise: one Newton
    // step on y^-5 = en from the library's value in double-double, and the exponent's rounding
    // as the factor 1 - 1.11e-17 ln(en).
    __device__ __forceinline__ static double pow_m02(double en) {
        const double y0 = pow(en, -1.0 / 5.0);
        const dd y2 = two_prod(y0, y0);
        const dd y4 = dd_mul(y2, y2);
        const dd y5 = dd_mul_d(y4, y0);
        const dd z = dd_mul_d(y5, en);
        const double r = (1.0 - z.hi) - z.lo;
        return y0 + y0 * (r / 5.0 - 1.1102230246251565e-17 * log(en));
    }
    __device__ __forceinline__ void quad_sums(double p, double e, double k, double& sdt,
                                              double& sdphi) const {
        double dt, dphi;
        quad_node(p, e, k, c, dt, dphi);
        wave_sums_host_order(dt, dphi, sdt, sdphi);
    }
    __device__ __forceinline__ static int step(int steps) {
        return steps > STEP_CAP ? EFD_TRAJ_STEP_CAP : 0;
    }
    __device__ __forceinline__ static int knot(int, double, const double*, const double*) {
        return 0;
    }
};

// Knot i goes to the source's slab [7][max_len] as (tau tscale, y, Omega / fden), stored by lane
// 0; a knot past max_len ends the integration with EFD_TRAJ_TOO_LONG instead (nothing past
// max_len knots is written).
struct WaveStore : Wave {
    double* slab;
    int max_len;
    double tscale, fden;

    __device__ __forceinline__ int knot(int i, double tau, const double* y, const double* om) {
        // (max_len >= 2, checked ahead of the launch: knot 0 always has room)
        if (i > 0 && i >= max_len) return EFD_TRAJ_TOO_LONG;
        double o[2];
        if (om) { o[0] = om[0]; o[1] = om[1]; }
        else fundamental(*this, y[0], y[1], o[0], o[1]);
        if ((threadIdx.x & (NCHI - 1)) == 0) {
            slab[i] = tau * tscale;
            slab[(size_t)max_len + i] = y[0];
            slab[2 * (size_t)max_len + i] = y[1];
            slab[3 * (size_t)max_len + i] = y[2];
            slab[4 * (size_t)max_len + i] = y[3];
            slab[5 * (size_t)max_len + i] = o[0] / fden;
            slab[6 * (size_t)max_len + i] = o[1] / fden;
        }
        return 0;
    }
};

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
        WaveStore side{{c_costab[lane]}, knots + (size_t)w * 7 * (size_t)max_len, max_len,
                       tscale, fden};
        double tau_end;
        st = integrate(side, s.p0, s.e0, s.Phi_phi0, s.Phi_r0, s.mu / s.M,
                       s.T * YRSID_SI / tscale, s.rtol, s.atol, &n, &tau_end);
    }
    if (lane == 0) {
        status[w] = st;
        if (st == EFD_TRAJ_OK) nt[w] = n;
    }
}

// efd_host_p_at_t per source with the default bracket (emrifd_rk45.h: p_at_t)
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
        Wave side{c_costab[lane]};
        st = p_at_t(side, s.e0, s.mu / s.M, tau_max, s.rtol, s.atol, tscale, t_out,
                    p0_bracket_lo(s.e0), 40.0, xtol, max_h(rtol_root, EPS4), &root);
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
