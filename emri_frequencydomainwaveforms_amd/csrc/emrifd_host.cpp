// emrifd_host.cpp -- the host upstream of the hot path in C++ (linked into libemrifd.so):
// trajectory and p0 root solve for one source.
//
// STAND-IN PHYSICS, NOT FEW: FEW's SchwarzEccFlux trajectory and ROMAN amplitude network need
// data files absent offline. This is the C++ form of this
// package's Python stand-ins, same equations and the same integrator. The equations, the
// integrator and the root solve are csrc/emrifd_rk45.h, the text that emrifd_traj.hip compiles
// for the device too; this unit holds what is the host's own: std::pow, the quadrature's loop and
// the knot store (the side types Host and HostKnots below), and the C entry points. The PSD
// table's evaluation is csrc/emrifd_psd.h, shared with emrifd_modes_device.inc likewise.
//   trajectory.py  Peters-Mathews (quadrupole) fluxes in (p, e), exact Schwarzschild
//                  Omega_phi, Omega_r (frequencies.py: 64-node trapezoid over the relativistic
//                  anomaly) for the phases; scipy's RK45 (Dormand-Prince 5(4), its step-size
//                  control, dense output and terminal-event root) at rtol = atol = 1e-12,
//                  stopping 0.1 outside the separatrix p = 6 + 2e or at T
//                  (EMRIInspiral(func="SchwarzEccFlux"), check_mode_by_mode.py:34-35)
//   get_p_at_t     Brent's root of t_plunge(p0) = t_out (few.utils.utility.get_p_at_t,
//                  check_mode_by_mode.py:200-212)
// (the amplitude stand-in and mode selection are in emrifd_modes.cpp, built with vector math)
// so the drivers' upstream (30-50 ms per walker in numpy/scipy) costs ~1-3 ms per source and
// releases the GIL: the Python layer runs a batch of walkers on a thread pool.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/emrifd.h"
#define EFD_HD inline
#include "emrifd_psd.h"
#undef EFD_HD

namespace efdhost {

using std::fabs;
using std::nextafter;
using std::signbit;
using std::sqrt;

#define EFD_HD inline
#define EFD_TABLE constexpr
#include "emrifd_rk45.h"
#undef EFD_TABLE
#undef EFD_HD

struct CosTable {
    double c[NCHI];
    CosTable() {
        for (int i = 0; i < NCHI; ++i) c[i] = std::cos(TWO_PI * i / NCHI);
    }
};
const CosTable& costab() {
    static const CosTable t;
    return t;
}

// The host's side of emrifd_rk45.h. Host counts the knots (the p0 solve needs each integration's
// end only); HostKnots also keeps them.
struct Host {
    static constexpr int STEP_FAILED = EFD_ERR_ARG, NO_BRACKET = EFD_ERR_ARG;
    static void pow_25_35(double x, double& x25, double& x35) {
        x35 = std::pow(x, 3.5);
        x25 = std::pow(x, 2.5);
    }
    static double pow_m02(double en) { return std::pow(en, -1.0 / 5.0); }
    static void quad_sums(double p, double e, double k, double& sdt, double& sdphi) {
        const double* c = costab().c;
        sdt = sdphi = 0.0;
        for (int i = 0; i < NCHI; ++i) {
            double dt, dphi;
            quad_node(p, e, k, c[i], dt, dphi);
            sdt += dt;
            sdphi += dphi;
        }
    }
    static int step(int) { return 0; }   // no step cap
    static int knot(int i, double, const double*, const double*) {
        return i < (1 << 20) ? 0 : EFD_ERR_WORKSPACE;   // (the root solve's bound on a trajectory)
    }
};

// Knot i as (tau, y, Omega_phi, Omega_r), the frequencies only when freqs; knot max_len ends the
// integration with EFD_ERR_WORKSPACE (the caller's arrays are written after a success only).
struct HostKnots : Host {
    int max_len;
    bool freqs;
    std::vector<double> k;   // [n][7]

    int knot(int i, double tau, const double* y, const double* om) {
        if (i >= max_len) return EFD_ERR_WORKSPACE;
        double o[2] = {0.0, 0.0};
        if (om) { o[0] = om[0]; o[1] = om[1]; }
        else if (freqs) fundamental(*this, y[0], y[1], o[0], o[1]);
        k.insert(k.end(), {tau, y[0], y[1], y[2], y[3], o[0], o[1]});
        return 0;
    }
};

// -- the PSD table of the noise-weighted mode selection (emrifd_psd.h; this unit is built without
// -ffast-math and with -ffp-contract=off: the guards below hold and every operation rounds on
// its own)
int psd_check(const efd_psd_table* psd) {
    if (!psd || !psd->x || !psd->c || psd->n < 2 || psd->n > 4096) return EFD_ERR_ARG;
    for (int i = 1; i < psd->n; ++i)
        if (!(psd->x[i] > psd->x[i - 1])) return EFD_ERR_ARG;
    return EFD_OK;
}

void psd_weights(const efd_psd_table& psd, double f_phi, double f_r, const int32_t* m,
                 const int32_t* n, int nm, double* w) {
    for (int k = 0; k < nm; ++k)
        w[k] = efdpsd::psd_weight(psd.x, psd.c, psd.n, m[k], n[k], f_phi, f_r);
}

bool psd_total_ok(double total) { return std::isfinite(total) && total > 0.0; }

}  // namespace efdhost

extern "C" {

int efd_psd_eval_cpu(const efd_psd_table* psd, const double* f, int64_t nf, double* out,
                     void* /*stream*/) {
    if (efdhost::psd_check(psd) != EFD_OK || nf < 0 || (nf > 0 && (!f || !out)))
        return EFD_ERR_ARG;
    for (int64_t j = 0; j < nf; ++j) out[j] = efdpsd::psd_eval(psd->x, psd->c, psd->n, f[j]);
    return EFD_OK;
}

int efd_host_trajectory(double M, double mu, double p0, double e0, double Phi_phi0, double Phi_r0,
                        double T, double rtol, double atol, int32_t max_len, double* t, double* p,
                        double* e, double* phi_phi, double* phi_r, double* f_phi, double* f_r,
                        int32_t* nt) {
    using namespace efdhost;
    if (!t || !p || !e || !phi_phi || !phi_r || !nt || max_len < 2 || !(M > 0) || !(mu > 0))
        return EFD_ERR_ARG;
    if (p0 - (6.0 + 2.0 * e0) <= DIST_TO_SEPARATRIX) return EFD_ERR_ARG;
    const double tscale = M * MTSUN_SI;
    HostKnots side{{}, max_len, f_phi && f_r, {}};
    int n;
    double tau_end;
    if (const int st = integrate(side, p0, e0, Phi_phi0, Phi_r0, mu / M, T * YRSID_SI / tscale,
                                 rtol, atol, &n, &tau_end))
        return st;
    for (int i = 0; i < n; ++i) {
        const double* k = &side.k[7 * (size_t)i];
        t[i] = k[0] * tscale;
        p[i] = k[1];
        e[i] = k[2];
        phi_phi[i] = k[3];
        phi_r[i] = k[4];
        if (side.freqs) {
            f_phi[i] = k[5] / (TWO_PI * M * MTSUN_SI);
            f_r[i] = k[6] / (TWO_PI * M * MTSUN_SI);
        }
    }
    *nt = n;
    return EFD_OK;
}

int efd_host_p_at_t(double M, double mu, double e0, double t_out, double rtol, double atol,
                    double xtol, double rtol_root, double lo, double hi, double* p0) {
    using namespace efdhost;
    if (!p0 || !(M > 0) || !(mu > 0) || !(t_out > 0)) return EFD_ERR_ARG;
    const double tscale = M * MTSUN_SI;
    const double tau_max = (2.0 * t_out + 1.0) * YRSID_SI / tscale;
    if (!(lo > 0)) lo = p0_bracket_lo(e0);
    if (!(hi > 0)) hi = 40.0;
    Host side;
    double root;
    // (a failed integration, a too-long one included, is EFD_ERR_ARG here as well)
    if (p_at_t(side, e0, mu / M, tau_max, rtol, atol, tscale, t_out, lo, hi, xtol,
               max_h(rtol_root, EPS4), &root))
        return EFD_ERR_ARG;
    *p0 = root;
    return EFD_OK;
}

// Staging of a walker batch for efd_modesum_prepare_batch: the ten input arrays of each walker
// (src[10 i + f], f in t, phi_phi, phi_r, f_phi, f_r, amp, m, n, ylm_p, ylm_m; sizes from
// shape[2 i] = nt, shape[2 i + 1] = K) packed 256-B aligned into the pinned buffer, and each
// walker's argument struct (tmpl's grid, caustic and output fields; its own scale and the
// device pointers dev_base + offset, valid once pin has been copied to dev_base). The packing
// costs one memcpy per array instead of a Python slice assignment each.
int efd_stage_batch(void* pin, size_t pin_bytes, uint64_t dev_base, int32_t count,
                    const uint64_t* src, const int32_t* shape, const double* scale,
                    const efd_modesum_args* tmpl, efd_modesum_args* args, size_t* total) {
    if (!src || !shape || !scale || !tmpl || !args || !total || count < 1) return EFD_ERR_ARG;
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    // walker i's ten byte counts, in the order of src
    auto sizes = [shape](int i, size_t* bytes) {
        const size_t nt = (size_t)shape[2 * i], K = (size_t)shape[2 * i + 1];
        const size_t b[10] = {8 * nt, 8 * nt, 8 * nt, 8 * nt, 8 * nt, 16 * nt * K,
                              4 * K, 4 * K, 16 * K, 16 * K};
        std::copy(b, b + 10, bytes);
    };
    // one pass: each walker's offset, and whether every source pointer is there (reported
    // only once the buffer is known to fit, after *total is set)
    std::vector<size_t> woff((size_t)count + 1, 0);
    bool null_src = false;
    size_t bytes[10];
    for (int i = 0; i < count; ++i) {
        if (shape[2 * i] < 2 || shape[2 * i + 1] < 1) return EFD_ERR_ARG;
        sizes(i, bytes);
        size_t o = woff[i];
        for (int f = 0; f < 10; ++f) {
            o = al(o + bytes[f]);
            null_src |= !src[10 * (size_t)i + f];
        }
        woff[i + 1] = o;
    }
    const size_t off = woff[count];
    *total = off;
    if (!pin || off > pin_bytes) return EFD_ERR_WORKSPACE;
    if (null_src) return EFD_ERR_ARG;
    char* dst = (char*)pin;
    // the copies: walkers over OpenMP threads when the batch is large (config 5's groups of
    // 16: ~2-4 MB, one thread's memcpy bandwidth made the copy most of the group's flush)
    const int nth = off >= ((size_t)1 << 20) ? std::min(count, 8) : 1;
#pragma omp parallel for num_threads(nth) schedule(static) if (nth > 1)
    for (int i = 0; i < count; ++i) {
        size_t bytes[10];
        sizes(i, bytes);
        uint64_t dp[10];
        size_t o = woff[i];
        for (int f = 0; f < 10; ++f) {
            const void* sp = (const void*)(uintptr_t)src[10 * (size_t)i + f];
            std::memcpy(dst + o, sp, bytes[f]);
            dp[f] = dev_base + o;
            o = al(o + bytes[f]);
        }
        efd_modesum_args& a = args[i];
        a = *tmpl;
        a.t = (const double*)(uintptr_t)dp[0];
        a.phi_phi = (const double*)(uintptr_t)dp[1];
        a.phi_r = (const double*)(uintptr_t)dp[2];
        a.f_phi = (const double*)(uintptr_t)dp[3];
        a.f_r = (const double*)(uintptr_t)dp[4];
        a.amp = (const double*)(uintptr_t)dp[5];
        a.m = (const int32_t*)(uintptr_t)dp[6];
        a.n = (const int32_t*)(uintptr_t)dp[7];
        a.ylm_p = (const double*)(uintptr_t)dp[8];
        a.ylm_m = (const double*)(uintptr_t)dp[9];
        a.nt = shape[2 * i];
        a.K = shape[2 * i + 1];
        a.scale_re = scale[2 * i];
        a.scale_im = scale[2 * i + 1];
    }
    return EFD_OK;
}

}  // extern "C"
