// emrifd_cpu_internal.h -- what the host twins' two units share: emrifd_cpu.cpp (the mode sum's
// twin, which defines these beside the error string and the thread setting) and
// emrifd_reduce_cpu.cpp (the reductions' twins).
#pragma once

#include <string>

namespace efdcpu {
// sets the calling thread's last-error string (efd_cpu_last_error) and returns code
int fail(int code, const std::string& msg);
// the OpenMP threads of a twin's parallel region (efd_cpu_threads; 0: all)
int nthreads();
}  // namespace efdcpu
