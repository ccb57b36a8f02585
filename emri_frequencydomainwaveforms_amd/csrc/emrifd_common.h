// emrifd_common.h -- what the library's HIP units share: emrifd.hip (mode sum),
// emrifd_prepare.hip (its preparation), emrifd_window.hip (window path) and emrifd_reduce.hip
// (channels and reductions). They share no device code but dh_term's few lines; each is compiled
// on its own (no relocatable device code) and linked into libemrifd.so. The two units of the
// mode-sum chain share emrifd_layout.h on top of this. Names declared here have external linkage
// so that the units can reach them, and hidden visibility so that the library still exports only
// include/emrifd.h.
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

// One bin of one channel of <d|h> and <h|h> (h already weighted) into s = (sum t_re, sum t_im,
// sum t_hh): the terms of include/emrifd.h's efd_modesum_sum_dh_hh, which the mode sum's epilogue
// and efd_dh_hh_rows both write through this. t_im is the difference of two rounded products, not
// an fma, and t_re and t_hh nest alike: with d == h bitwise, t_re == t_hh and t_im == 0 exactly.
__device__ __forceinline__ void dh_term(const double2 d, const double2 h, double* s) {
#pragma clang fp contract(off)
    s[0] += fma(d.x, h.x, d.y * h.y);
    s[1] += d.x * h.y - d.y * h.x;
    s[2] += fma(h.x, h.x, h.y * h.y);
}

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(EFD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
