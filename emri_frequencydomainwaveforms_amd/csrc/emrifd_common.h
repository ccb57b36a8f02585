// emrifd_common.h -- what the library's HIP units share: emrifd.hip (mode sum),
// emrifd_prepare.hip (its preparation), emrifd_window.hip (window path) and emrifd_reduce.hip
// (channels and reductions). They share no device code; each is compiled on its own (no
// relocatable device code) and linked into libemrifd.so. The two units of the mode-sum chain
// share emrifd_layout.h on top of this. Names declared here have external linkage so that the units can reach them,
// and hidden visibility so that the library still exports only include/emrifd.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/emrifd.h"

#define EFD_INTERNAL __attribute__((visibility("hidden")))

namespace efdhip {
// sets the calling thread's last-error string (efd_last_error) and returns code; defined once,
// beside the string, in emrifd.hip
EFD_INTERNAL int fail(int code, const std::string& msg);
// k_final (emrifd_reduce.hip) with the likelihood's scale -2, one workgroup per row: out[r] from
// row r's np partials at part[r np ...]. The window path's likelihoods end in the same kernel,
// so they launch it through this instead of holding a copy; the caller checks hipGetLastError()
EFD_INTERNAL void launch_loglike_final(int rows, const double* part, int np, double* out,
                                       hipStream_t st);
}  // namespace efdhip
using efdhip::fail;

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(EFD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
