// Stand-alone check of efd_overlap_rows_cpu for host sanitizers (no Python, no GPU):
//
//   g++ -O1 -g -std=c++17 -fopenmp -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I include tools/overlap_cpu_check.cpp \
//       emri_frequencydomainwaveforms_amd/csrc/emrifd_reduce_cpu.cpp \
//       emri_frequencydomainwaveforms_amd/csrc/emrifd_cpu.cpp -o overlap_cpu_check
//   ./overlap_cpu_check
//
// Runs the twin over the CPU test's shapes (nelem in {1, 63, 257, 8194} x nrow in {1, 9, 64}, u
// NULL and not, w NULL, a padded stride, weights with zeros) with every buffer allocated at its
// exact size, compares with a long-double sum, and checks the exact zeros and argument errors.

#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "emrifd.h"

static int failures = 0;

static void expect(bool ok, const char* what, long a = 0, long b = 0) {
    if (!ok) {
        std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
        ++failures;
    }
}

static void run(int64_t nelem, int nrow, bool with_u, bool with_w, int64_t pad, bool zeros) {
    std::mt19937_64 g(1234 + nelem * 131 + nrow);
    std::normal_distribution<double> N(0.0, 1.0);
    std::uniform_real_distribution<double> U(0.5, 2.0);
    const int64_t stride = nelem + pad;
    std::vector<double> h(2 * ((size_t)(nrow - 1) * stride + nelem)), t(2 * nelem), u(2 * nelem),
        w(nelem), out(3 * nrow + 1, NAN);
    for (auto& x : h) x = N(g);
    for (auto& x : t) x = N(g);
    for (auto& x : u) x = N(g);
    for (int64_t e = 0; e < nelem; ++e) w[e] = zeros && e % 3 == 0 ? 0.0 : U(g);
    const int rc = efd_overlap_rows_cpu(h.data(), stride, nrow, t.data(), with_u ? u.data() : nullptr,
                                        with_w ? w.data() : nullptr, nelem, out.data(), nullptr,
                                        nullptr);
    expect(rc == EFD_OK, "return code", nelem, nrow);
    long double rr = 0.0L;
    std::vector<long double> rre(nelem), rim(nelem);
    for (int64_t e = 0; e < nelem; ++e) {
        rre[e] = (long double)t[2 * e] - (with_u ? u[2 * e] : 0.0);
        rim[e] = (long double)t[2 * e + 1] - (with_u ? u[2 * e + 1] : 0.0);
        rr += (with_w ? w[e] : 1.0) * (rre[e] * rre[e] + rim[e] * rim[e]);
    }
    expect(std::fabs((double)(4 * rr) - out[3 * nrow]) <= 1e-12 * (double)(4 * rr), "rr", nelem, nrow);
    for (int k = 0; k < nrow; ++k) {
        long double re = 0.0L, im = 0.0L, nn = 0.0L;
        for (int64_t e = 0; e < nelem; ++e) {
            const long double hr = h[2 * (k * stride + e)], hi = h[2 * (k * stride + e) + 1];
            const long double ww = with_w ? w[e] : 1.0;
            re += ww * (hr * rre[e] + hi * rim[e]);
            im += ww * (hr * rim[e] - hi * rre[e]);
            nn += ww * (hr * hr + hi * hi);
        }
        const double s = std::sqrt((double)(4 * nn) * (double)(4 * rr));
        expect(std::fabs((double)(4 * re) - out[3 * k]) <= 1e-12 * s, "re", nelem, k);
        expect(std::fabs((double)(4 * im) - out[3 * k + 1]) <= 1e-12 * s, "im", nelem, k);
        expect(std::fabs((double)(4 * nn) - out[3 * k + 2]) <= 1e-12 * (double)(4 * nn), "nn", nelem, k);
    }
    if (with_u) {   // u == t bit for bit: exact zeros
        std::vector<double> z(3 * nrow + 1, NAN);
        efd_overlap_rows_cpu(h.data(), stride, nrow, t.data(), t.data(), with_w ? w.data() : nullptr,
                             nelem, z.data(), nullptr, nullptr);
        for (int k = 0; k < nrow; ++k)
            expect(z[3 * k] == 0.0 && z[3 * k + 1] == 0.0, "exact zero", nelem, k);
        expect(z[3 * nrow] == 0.0, "exact zero rr", nelem, nrow);
    }
}

int main() {
    const int64_t nelems[] = {1, 63, 257, 8194};
    const int nrows[] = {1, 9, 64};
    for (int64_t nelem : nelems)
        for (int nrow : nrows)
            for (int v = 0; v < 5; ++v)
                // v: 0 all given, 1 u NULL, 2 w NULL, 3 padded stride, 4 weights with zeros
                run(nelem, nrow, v != 1, v != 2, v == 3 ? 3 : 0, v == 4);
    for (int threads : {1, 3}) {   // the fixed partition: any thread count, the same bits
        efd_cpu_threads(threads);
        run(8194, 9, true, true, 0, false);
    }
    efd_cpu_threads(0);
    double x[16] = {0}, o[8];
    expect(efd_overlap_rows_cpu(x, 4, 0, x, nullptr, nullptr, 4, o, nullptr, nullptr) == EFD_ERR_ARG, "nrow 0");
    expect(efd_overlap_rows_cpu(x, 4, 65, x, nullptr, nullptr, 4, o, nullptr, nullptr) == EFD_ERR_ARG, "nrow 65");
    expect(efd_overlap_rows_cpu(nullptr, 4, 1, x, nullptr, nullptr, 4, o, nullptr, nullptr) == EFD_ERR_ARG, "h");
    expect(efd_overlap_rows_cpu(x, 4, 1, nullptr, nullptr, nullptr, 4, o, nullptr, nullptr) == EFD_ERR_ARG, "t");
    expect(efd_overlap_rows_cpu(x, 4, 1, x, nullptr, nullptr, 4, nullptr, nullptr, nullptr) == EFD_ERR_ARG, "out");
    expect(efd_overlap_rows_cpu(x, 4, 1, x, nullptr, nullptr, 0, o, nullptr, nullptr) == EFD_ERR_ARG, "nelem");
    expect(efd_overlap_rows_cpu(x, 3, 1, x, nullptr, nullptr, 4, o, nullptr, nullptr) == EFD_ERR_ARG, "stride");
    std::printf(failures ? "%d failures\n" : "overlap_cpu_check: all shapes pass (%d failures)\n",
                failures);
    return failures != 0;
}
