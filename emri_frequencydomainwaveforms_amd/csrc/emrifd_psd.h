// emrifd_psd.h -- the PSD table (efd_psd_table) of the noise-weighted mode selection.
//
// The evaluation, written once for the host (emrifd_host.cpp) and the device
// (emrifd_modes_device.inc): the units that evaluate the table define EFD_HD (the functions'
// qualifiers: inline; __device__ inline) ahead of the include. Every product and sum rounds on
// its own: contraction is off inside both functions (the pragma for hipcc; the host unit is
// built with -ffp-contract=off), so the two give the same bits.
//
// The host's table checks and guards are defined in emrifd_host.cpp, which is built WITHOUT
// -ffast-math: emrifd_modes.cpp is built with it, and there isnan / isfinite and the S > 0 guard
// are not reliable, so it calls these (and does not define EFD_HD).
#include <cmath>
#include <cstdint>

#include "../../include/emrifd.h"

// (its own guard, not the declarations': a unit that saw this file first without EFD_HD still
// gets the functions from its include with EFD_HD)
#if defined(EFD_HD) && !defined(EMRIFD_PSD_EVAL_DEFINED)
#define EMRIFD_PSD_EVAL_DEFINED
namespace efdpsd {
// S(f) of a PPoly-layout table (include/emrifd.h): x the n breakpoints, c [4][n - 1]
EFD_HD double psd_eval(const double* x, const double* c, int n, double f) {
#pragma clang fp contract(off)
    int lo = 0, hi = n;   // -> #{j : x[j] <= f}; a NaN compares false everywhere and lands on
    while (lo < hi) {     // the last piece (n), as NaN
        const int mid = (lo + hi) >> 1;
        if (f < x[mid]) hi = mid; else lo = mid + 1;
    }
    int i = lo - 1;       // the piece: clamped to 0 .. n - 2
    if (i < 0) i = 0;
    if (i > n - 2) i = n - 2;
    const double s = f - x[i];
    const int st = n - 1;
    double r = c[i];
    r = r * s + c[st + i];
    r = r * s + c[2 * st + i];
    return r * s + c[3 * st + i];
}

// 1 / S(|m f_phi + n f_r|) where S is finite and > 0, else 0
EFD_HD double psd_weight(const double* x, const double* c, int n, int m, int nn, double f_phi,
                         double f_r) {
#pragma clang fp contract(off)
    const double F = std::fabs((double)m * f_phi + (double)nn * f_r);
    const double S = psd_eval(x, c, n, F);
    return (std::isfinite(S) && S > 0.0) ? 1.0 / S : 0.0;
}
}  // namespace efdpsd
#endif

#ifndef EMRIFD_PSD_H
#define EMRIFD_PSD_H
namespace efdhost {
// EFD_OK when psd is usable: pointers set, 2 <= n <= 4096, x strictly ascending (NaN fails)
int psd_check(const efd_psd_table* psd);
// w[k] = psd_weight of mode (m[k], n[k]) at the knot frequencies f_phi, f_r; k < nm
void psd_weights(const efd_psd_table& psd, double f_phi, double f_r, const int32_t* m,
                 const int32_t* n, int nm, double* w);
// a knot's weighted total can be ranked: finite and > 0
bool psd_total_ok(double total);
}  // namespace efdhost
#endif
