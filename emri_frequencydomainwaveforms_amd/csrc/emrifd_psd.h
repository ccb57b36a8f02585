// emrifd_psd.h -- the host PSD table (efd_psd_table) for the noise-weighted mode selection.
// Defined in emrifd_host.cpp, which is built WITHOUT -ffast-math: emrifd_modes.cpp is built with
// it, and there isnan / isfinite and the S > 0 guard are not reliable, so it calls these.
#pragma once
#include <cstdint>

#include "../../include/emrifd.h"

namespace efdhost {
// EFD_OK when psd is usable: pointers set, 2 <= n <= 4096, x strictly ascending (NaN fails)
int psd_check(const efd_psd_table* psd);
// S(f) of a checked table (include/emrifd.h: every operation rounded on its own)
double psd_eval(const efd_psd_table& psd, double f);
// w[k] = 1 / S(|m[k] f_phi + n[k] f_r|) where S is finite and > 0, else 0; k < nm
void psd_weights(const efd_psd_table& psd, double f_phi, double f_r, const int32_t* m,
                 const int32_t* n, int nm, double* w);
// a knot's weighted total can be ranked: finite and > 0
bool psd_total_ok(double total);
}  // namespace efdhost
