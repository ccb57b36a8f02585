// emrifd_reduce_cpu.cpp -- host twins of emrifd_reduce.hip's entry points (the channel split,
// the likelihood and inner product, the TD template's split, the Fisher Gram matrix, the overlap
// rows, the pair statistics, <d|h> and <h|h> of rows, the window rows) and of emrifd_noise.hip's
// (the noise draws and their overlaps with rows, on emrifd_noise.h): the same arithmetic in
// C++17 with OpenMP on host pointers, with the signatures of the HIP entry points (`stream` and
// scratch are accepted and unused). Built with contraction off: a product that feeds a sum
// rounds first unless it is a written fma. Shares emrifd_cpu_internal.h with the mode sum's twin
// (emrifd_cpu.cpp).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include <omp.h>

#include "../../include/emrifd.h"
#include "emrifd_cpu_internal.h"
#include "emrifd_noise.h"

namespace {

// The one reduction order of the twins that promise a result independent of the thread count
// (and, per row, of the call's other rows): fixed chunks of 4096 elements, one vector of nout
// partial sums per chunk -- body(e0, e1, acc) adds the elements [e0, e1) in ascending order to
// its zeroed acc[0 .. nout - 1] -- and the chunks' vectors added in chunk order into sum.
template <class Body>
void chunk_sums(int64_t nelem, int nout, double* sum, Body body) {
    const int64_t chunk = 4096;
    const int64_t nchunk = (nelem + chunk - 1) / chunk;
    std::vector<double> part((size_t)nchunk * nout, 0.0);
#pragma omp parallel for schedule(static) num_threads(efdcpu::nthreads())
    for (int64_t c = 0; c < nchunk; ++c)
        body(c * chunk, std::min(nelem, (c + 1) * chunk), part.data() + (size_t)c * nout);
    for (int o = 0; o < nout; ++o) {
        double s = 0.0;
        for (int64_t c = 0; c < nchunk; ++c) s += part[(size_t)c * nout + o];
        sum[o] = s;
    }
}

// efd_td_split's arithmetic
inline void td_split_pair(const double* z, int64_t n, int64_t k, double gain, double* hp,
                          double* hc) {
    const int64_t j = k == 0 ? 0 : n - k;
    const double ar = z[2 * k], ai = z[2 * k + 1], br = z[2 * j], bi = z[2 * j + 1];
    hp[0] = gain * (0.5 * (ar + br)); hp[1] = gain * (0.5 * (ai - bi));
    hc[0] = gain * (-0.5 * (ai + bi)); hc[1] = gain * (0.5 * (ar - br));
}

// efd_pair_stats' terms, the same nesting (include/emrifd.h): abi's term is the difference of
// two rounded products, so it is exactly 0 when b == a
inline void pair_term(double w, double ar, double ai, double br, double bi, double* s) {
    const double dr = ar - br, di = ai - bi;
    s[0] = std::fma(w, std::fma(ar, ar, ai * ai), s[0]);
    s[1] = std::fma(w, std::fma(br, br, bi * bi), s[1]);
    s[2] = std::fma(w, std::fma(ar, br, ai * bi), s[2]);
    s[3] = std::fma(w, ar * bi - ai * br, s[3]);
    s[4] = std::fma(w, std::fma(dr, dr, di * di), s[4]);
}

// Both pair statistics, a row at a time through chunk_sums: a row's numbers do not depend on
// other rows. zsplit: b is the split of row r of Z (efd_td_split's arithmetic and keep rule),
// nchan = 2.
void pair_stats_rows(const double* a, int64_t a_stride, const double* b, int64_t b_stride,
                     bool zsplit, int64_t n, double gain, const uint8_t* keep, int32_t nrow,
                     int32_t nchan, int64_t nbin, const double* w, double* out) {
    const int ns = 5 * nchan;
    for (int32_t r = 0; r < nrow; ++r) {
        const double* ar = a + 2 * (int64_t)r * a_stride;
        const double* br = b + 2 * (int64_t)r * b_stride;
        double* o = out + (int64_t)r * ns;
        chunk_sums(nbin, ns, o, [&](int64_t k0, int64_t k1, double* s) {
            for (int64_t k = k0; k < k1; ++k) {
                const double ww = w ? w[k] : 1.0;
                if (zsplit) {
                    double hp[2] = {0.0, 0.0}, hc[2] = {0.0, 0.0};
                    if (!keep || keep[k]) td_split_pair(br, n, k, gain, hp, hc);
                    pair_term(ww, ar[2 * k], ar[2 * k + 1], hp[0], hp[1], s);
                    pair_term(ww, ar[2 * (nbin + k)], ar[2 * (nbin + k) + 1], hc[0], hc[1], s + 5);
                } else {
                    for (int ch = 0; ch < nchan; ++ch) {
                        const int64_t e = 2 * (ch * nbin + k);
                        pair_term(ww, ar[e], ar[e + 1], br[e], br[e + 1], s + 5 * ch);
                    }
                }
            }
        });
        for (int i = 0; i < ns; ++i) o[i] = 4.0 * o[i];
        if (zsplit && (n & 1) == 0) {   // the Nyquist bin: in no channel, but a NaN there counts
            const double vr = br[n], vi = br[n + 1];
            if (vr != vr || vi != vi)
                for (int ch = 0; ch < 2; ++ch)
                    for (int i = 1; i < 5; ++i) o[5 * ch + i] = vr + vi;
        }
    }
}

}  // namespace

extern "C" {

int efd_polarizations_cpu(const double* S, int64_t nf, int64_t k0, double* hp, double* hc,
                          void* stream) {
    (void)stream;
    if (!S || !hp || !hc || nf <= 0 || k0 < 0 || k0 > nf)
        return efdcpu::fail(EFD_ERR_ARG, "efd_polarizations_cpu: bad arguments");
#pragma omp parallel for schedule(static) num_threads(efdcpu::nthreads())
    for (int64_t k = k0; k < nf; ++k) {
        const double ar = S[2 * k], ai = S[2 * k + 1];
        const double br = S[2 * (nf - 1 - k)], bi = S[2 * (nf - 1 - k) + 1];
        const int64_t i = k - k0;
        hp[2 * i] = 0.5 * (ar + br); hp[2 * i + 1] = 0.5 * (ai - bi);
        hc[2 * i] = -0.5 * (ai + bi); hc[2 * i + 1] = 0.5 * (ar - br);
    }
    return EFD_OK;
}

int efd_loglike_cpu(const double* h, const double* d, const double* w, int32_t nchan,
                    int64_t nbin, double* out, double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (!d || !w || !out || nchan <= 0 || nbin <= 0)
        return efdcpu::fail(EFD_ERR_ARG, "efd_loglike_cpu: bad arguments");
    const int64_t total = (int64_t)nchan * nbin;
    double acc = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : acc) num_threads(efdcpu::nthreads())
    for (int64_t i = 0; i < total; ++i) {
        double rr = d[2 * i], ri = d[2 * i + 1];
        if (h) {
            const double p = h[2 * i] * w[i], q = h[2 * i + 1] * w[i];
            rr -= p;
            ri -= q;
        }
        acc += rr * rr + ri * ri;
    }
    *out = -0.5 * 4.0 * acc;
    return EFD_OK;
}

int efd_inner_product_cpu(const double* a, const double* b, const double* w, int32_t nchan,
                          int64_t nbin, double* out, double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (!a || !b || !out || nchan <= 0 || nbin <= 0)
        return efdcpu::fail(EFD_ERR_ARG, "efd_inner_product_cpu: bad arguments");
    const int64_t total = (int64_t)nchan * nbin;
    double re = 0.0, im = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : re, im) num_threads(efdcpu::nthreads())
    for (int64_t i = 0; i < total; ++i) {
        const double ww = w ? w[i] : 1.0;
        re += ww * (a[2 * i] * b[2 * i] + a[2 * i + 1] * b[2 * i + 1]);
        im += ww * (a[2 * i] * b[2 * i + 1] - a[2 * i + 1] * b[2 * i]);
    }
    out[0] = 4.0 * re;
    out[1] = 4.0 * im;
    return EFD_OK;
}

// efd_fisher_gram's arithmetic: the stencil per element first (ascending s), then the symmetric
// term w (ar br + ai bi) of every pair i <= j; the partial triangles through chunk_sums.
int efd_fisher_gram_cpu(const double* h, int64_t row_stride, int32_t nparam, int32_t npoint,
                        const double* coef, const double* w, int64_t nelem, double* dh,
                        double* gram, double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (nparam < 1 || nparam > EFD_FISHER_MAX_PARAMS)
        return efdcpu::fail(EFD_ERR_ARG, "efd_fisher_gram_cpu: nparam outside 1..16");
    if (npoint != 1 && npoint != 2 && npoint != 4)
        return efdcpu::fail(EFD_ERR_ARG, "efd_fisher_gram_cpu: npoint must be 1, 2 or 4");
    if (!h || !coef || !gram)
        return efdcpu::fail(EFD_ERR_ARG, "efd_fisher_gram_cpu: NULL h, coef or gram");
    if (nelem <= 0) return efdcpu::fail(EFD_ERR_ARG, "efd_fisher_gram_cpu: nelem <= 0");
    if (row_stride < nelem)
        return efdcpu::fail(EFD_ERR_ARG, "efd_fisher_gram_cpu: row_stride < nelem");
    const int P = nparam;
    double tri[EFD_FISHER_MAX_PARAMS * (EFD_FISHER_MAX_PARAMS + 1) / 2];
    chunk_sums(nelem, P * (P + 1) / 2, tri, [&](int64_t e0, int64_t e1, double* acc) {
        double dr[EFD_FISHER_MAX_PARAMS], di[EFD_FISHER_MAX_PARAMS];
        for (int64_t e = e0; e < e1; ++e) {
            for (int i = 0; i < P; ++i) {
                const double* r = h + 2 * (row_stride * ((int64_t)i * npoint) + e);
                const double* cf = coef + (size_t)i * npoint;
                double xr = cf[0] * r[0], xi = cf[0] * r[1];
                for (int s = 1; s < npoint; ++s) {
                    xr = std::fma(cf[s], r[2 * row_stride * s], xr);
                    xi = std::fma(cf[s], r[2 * row_stride * s + 1], xi);
                }
                dr[i] = xr;
                di[i] = xi;
                if (dh) {
                    dh[2 * ((int64_t)i * nelem + e)] = xr;
                    dh[2 * ((int64_t)i * nelem + e) + 1] = xi;
                }
            }
            const double ww = w ? w[e] : 1.0;
            int p = 0;
            for (int i = 0; i < P; ++i)
                for (int j = i; j < P; ++j, ++p) {
                    const double q = di[i] * di[j];
                    acc[p] = std::fma(ww, std::fma(dr[i], dr[j], q), acc[p]);
                }
        }
    });
    int p = 0;
    for (int i = 0; i < P; ++i)
        for (int j = i; j < P; ++j, ++p) gram[i * P + j] = gram[j * P + i] = 4.0 * tri[p];
    return EFD_OK;
}

// efd_overlap_rows' arithmetic: r = t - u per element, then the three written fmas per row,
// through chunk_sums: a row's numbers do not depend on the other rows.
int efd_overlap_rows_cpu(const double* h, int64_t row_stride, int32_t nrow, const double* t,
                         const double* u, const double* w, int64_t nelem, double* out,
                         double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (nrow < 1 || nrow > EFD_OVERLAP_MAX_ROWS)
        return efdcpu::fail(EFD_ERR_ARG, "efd_overlap_rows_cpu: nrow outside 1..64");
    if (!h || !t || !out)
        return efdcpu::fail(EFD_ERR_ARG, "efd_overlap_rows_cpu: NULL h, t or out");
    if (nelem <= 0) return efdcpu::fail(EFD_ERR_ARG, "efd_overlap_rows_cpu: nelem <= 0");
    if (row_stride < nelem)
        return efdcpu::fail(EFD_ERR_ARG, "efd_overlap_rows_cpu: row_stride < nelem");
    const int nout = 3 * nrow + 1;
    chunk_sums(nelem, nout, out, [&](int64_t e0, int64_t e1, double* acc) {
        for (int64_t e = e0; e < e1; ++e) {
            double rr = t[2 * e], ri = t[2 * e + 1];
            if (u) {
                rr -= u[2 * e];
                ri -= u[2 * e + 1];
            }
            const double ww = w ? w[e] : 1.0;
            for (int k = 0; k < nrow; ++k) {
                const double* r = h + 2 * (row_stride * (int64_t)k + e);
                const double hr = r[0], hi = r[1];
                acc[3 * k] = std::fma(ww, std::fma(hr, rr, hi * ri), acc[3 * k]);
                acc[3 * k + 1] = std::fma(ww, std::fma(hr, ri, -(hi * rr)), acc[3 * k + 1]);
                acc[3 * k + 2] = std::fma(ww, std::fma(hr, hr, hi * hi), acc[3 * k + 2]);
            }
            acc[3 * nrow] = std::fma(ww, std::fma(rr, rr, ri * ri), acc[3 * nrow]);
        }
    });
    for (int o = 0; o < nout; ++o) out[o] = 4.0 * out[o];
    return EFD_OK;
}

int efd_td_split_cpu(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                     const uint8_t* keep, double* out, int64_t out_stride, void* stream) {
    (void)stream;
    const int64_t nb = (n + 1) / 2;
    if (!Z || !out) return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_cpu: NULL Z or out");
    if (n < 1 || rows < 1 || stride < n || out_stride < 2 * nb)
        return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_cpu: n, rows, stride or out_stride");
    for (int32_t r = 0; r < rows; ++r) {
        const double* z = Z + 2 * (int64_t)r * stride;
        double* o = out + 2 * (int64_t)r * out_stride;
#pragma omp parallel for schedule(static) num_threads(efdcpu::nthreads())
        for (int64_t k = 0; k < nb; ++k) {
            double hp[2] = {0.0, 0.0}, hc[2] = {0.0, 0.0};
            if (!keep || keep[k]) td_split_pair(z, n, k, gain, hp, hc);
            o[2 * k] = hp[0]; o[2 * k + 1] = hp[1];
            o[2 * (nb + k)] = hc[0]; o[2 * (nb + k) + 1] = hc[1];
        }
    }
    return EFD_OK;
}

// a row at a time through chunk_sums (no dependence on threads)
int efd_td_split_loglike_cpu(const double* Z, int64_t stride, int64_t n, int32_t rows,
                             double gain, const double* d, const double* w, double* out,
                             double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (!Z || !d || !w || !out)
        return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_loglike_cpu: NULL Z, d, w or out");
    if (n < 1 || rows < 1 || stride < n)
        return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_loglike_cpu: n, rows or stride");
    const int64_t nb = (n + 1) / 2;
    for (int32_t r = 0; r < rows; ++r) {
        const double* z = Z + 2 * (int64_t)r * stride;
        double s = 0.0;
        chunk_sums(nb, 1, &s, [&](int64_t k0, int64_t k1, double* acc) {
            for (int64_t k = k0; k < k1; ++k) {
                double hp[2], hc[2];
                td_split_pair(z, n, k, gain, hp, hc);
                const double w0 = w[k], w1 = w[nb + k];
                const double ar = d[2 * k] - hp[0] * w0, ai = d[2 * k + 1] - hp[1] * w0;
                const double br = d[2 * (nb + k)] - hc[0] * w1;
                const double bi = d[2 * (nb + k) + 1] - hc[1] * w1;
                *acc += ar * ar + ai * ai;
                *acc += br * br + bi * bi;
            }
        });
        if ((n & 1) == 0) {   // the Nyquist bin: in no channel, but a NaN there counts
            const double vr = z[n], vi = z[n + 1];
            if (vr != vr || vi != vi) s = vr + vi;
        }
        out[r] = -0.5 * 4.0 * s;
    }
    return EFD_OK;
}

int efd_pair_stats_cpu(const double* a, int64_t a_stride, const double* b, int64_t b_stride,
                       int32_t nrow, int32_t nchan, int64_t nbin, const double* w, double* out,
                       double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (nrow < 1 || nrow > EFD_PAIR_MAX_ROWS)
        return efdcpu::fail(EFD_ERR_ARG, "efd_pair_stats_cpu: nrow outside 1..64");
    if (nchan != 1 && nchan != 2)
        return efdcpu::fail(EFD_ERR_ARG, "efd_pair_stats_cpu: nchan must be 1 or 2");
    if (!a || !b || !out) return efdcpu::fail(EFD_ERR_ARG, "efd_pair_stats_cpu: NULL a, b or out");
    if (nbin <= 0) return efdcpu::fail(EFD_ERR_ARG, "efd_pair_stats_cpu: nbin <= 0");
    if (a_stride < nchan * nbin || b_stride < nchan * nbin)
        return efdcpu::fail(EFD_ERR_ARG, "efd_pair_stats_cpu: stride < nchan nbin");
    pair_stats_rows(a, a_stride, b, b_stride, false, 0, 1.0, nullptr, nrow, nchan, nbin, w, out);
    return EFD_OK;
}

int efd_td_split_pair_stats_cpu(const double* Z, int64_t stride, int64_t n, int32_t rows,
                                double gain, const double* a, int64_t a_stride, const double* w,
                                const uint8_t* keep, double* out, double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (!Z || !a || !out)
        return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_pair_stats_cpu: NULL Z, a or out");
    if (n < 1) return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_pair_stats_cpu: n < 1");
    if (rows < 1 || rows > EFD_PAIR_MAX_ROWS)
        return efdcpu::fail(EFD_ERR_ARG, "efd_td_split_pair_stats_cpu: rows outside 1..64");
    const int64_t nb = (n + 1) / 2;
    if (stride < n || a_stride < 2 * nb)
        return efdcpu::fail(EFD_ERR_ARG,
                            "efd_td_split_pair_stats_cpu: stride < n or a_stride < 2 nb");
    pair_stats_rows(a, a_stride, Z, stride, true, n, gain, keep, rows, 2, nb, w, out);
    return EFD_OK;
}

// efd_dh_hh_rows' arithmetic: h w with each component's product rounded, then the three written
// terms, a row at a time through chunk_sums (a row's numbers do not depend on the other rows)
int efd_dh_hh_rows_cpu(const double* h, int64_t row_stride, int32_t nrow, const double* d,
                       const double* w, int32_t nchan, int64_t nbin, double* out,
                       double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (nrow < 1 || nrow > EFD_DH_MAX_ROWS)
        return efdcpu::fail(EFD_ERR_ARG, "efd_dh_hh_rows_cpu: nrow outside 1..64");
    if (nchan != 1 && nchan != 2)
        return efdcpu::fail(EFD_ERR_ARG, "efd_dh_hh_rows_cpu: nchan must be 1 or 2");
    if (!h || !d || !w || !out)
        return efdcpu::fail(EFD_ERR_ARG, "efd_dh_hh_rows_cpu: NULL h, d, w or out");
    if (nbin <= 0) return efdcpu::fail(EFD_ERR_ARG, "efd_dh_hh_rows_cpu: nbin <= 0");
    if (row_stride < nchan * nbin)
        return efdcpu::fail(EFD_ERR_ARG, "efd_dh_hh_rows_cpu: row_stride < nchan nbin");
    for (int32_t r = 0; r < nrow; ++r) {
        const double* hr = h + 2 * (int64_t)r * row_stride;
        double* o = out + 3 * (int64_t)r;
        chunk_sums(nbin, 3, o, [&](int64_t k0, int64_t k1, double* s) {
            for (int64_t k = k0; k < k1; ++k)
                for (int ch = 0; ch < nchan; ++ch) {
                    const int64_t e = ch * nbin + k;
                    const double hx = hr[2 * e] * w[e], hy = hr[2 * e + 1] * w[e];
                    const double dx = d[2 * e], dy = d[2 * e + 1];
                    s[0] += std::fma(dx, hx, dy * hy);
                    s[1] += dx * hy - dy * hx;
                    s[2] += std::fma(hx, hx, hy * hy);
                }
        });
        for (int i = 0; i < 3; ++i) o[i] = 4.0 * o[i];
    }
    return EFD_OK;
}

int efd_window_rows_cpu(const double* h, int64_t n, const double* const* win, int32_t nwin,
                        double* out, int64_t out_stride, void* stream) {
    (void)stream;
    if (!h || !win || !out)
        return efdcpu::fail(EFD_ERR_ARG, "efd_window_rows_cpu: NULL h, win or out");
    if (n < 1 || nwin < 1 || nwin > EFD_WINDOW_MAX_ROWS || out_stride < n)
        return efdcpu::fail(EFD_ERR_ARG, "efd_window_rows_cpu: n, nwin or out_stride");
    for (int32_t j = 0; j < nwin; ++j) {
        const double* wj = win[j];
        double* o = out + 2 * (int64_t)j * out_stride;
#pragma omp parallel for schedule(static) num_threads(efdcpu::nthreads())
        for (int64_t k = 0; k < n; ++k) {
            const double x = wj ? wj[k] : 1.0;
            o[2 * k] = wj ? x * h[2 * k] : h[2 * k];
            o[2 * k + 1] = wj ? x * h[2 * k + 1] : h[2 * k + 1];
        }
    }
    return EFD_OK;
}

// efd_noise_fd's arithmetic: one draw per live bin (emrifd_noise.h), s = 0.5 gain, (s xi_r,
// s xi_i), added to out under accumulate
int efd_noise_fd_cpu(double* out, const double* gain, int32_t nchan, int64_t nbin, uint64_t bin0,
                     uint64_t seed, uint32_t realisation, int32_t accumulate, void* stream) {
    (void)stream;
    if (nbin == 0) return EFD_OK;
    if (!out) return efdcpu::fail(EFD_ERR_ARG, "efd_noise_fd_cpu: NULL out");
    if (nchan < 1 || nbin < 0)
        return efdcpu::fail(EFD_ERR_ARG, "efd_noise_fd_cpu: nchan < 1 or nbin < 0");
    for (int32_t c = 0; c < nchan; ++c) {
        double* o = out + 2 * (int64_t)c * nbin;
        const double* g = gain ? gain + (int64_t)c * nbin : nullptr;
#pragma omp parallel for schedule(static) num_threads(efdcpu::nthreads())
        for (int64_t i = 0; i < nbin; ++i) {
            const double gv = g ? g[i] : 1.0;
            if (!efdnoise::live_gain(gv)) {
                if (!accumulate) o[2 * i] = o[2 * i + 1] = 0.0;
                continue;
            }
            double xr, xi;
            efdnoise::draw_xi(seed, realisation, (uint32_t)c, bin0 + (uint64_t)i, xr, xi);
            const double s = 0.5 * gv;
            const double vr = s * xr, vi = s * xi;
            if (accumulate) {
                o[2 * i] += vr;
                o[2 * i + 1] += vi;
            } else {
                o[2 * i] = vr;
                o[2 * i + 1] = vi;
            }
        }
    }
    return EFD_OK;
}

// efd_noise_overlap_rows' arithmetic: the gain multiplied into the rows' bin once, then per draw
// fma(xi_r, g h_r, fma(xi_i, g h_i, acc)), channels inside bins, through chunk_sums: an entry
// does not depend on the other rows or draws. 64 draws at a time bound the partial sums' memory.
int efd_noise_overlap_rows_cpu(const double* rows, int32_t nrow, const double* gain,
                               int32_t nchan, int64_t nbin, uint64_t seed, uint32_t real0,
                               int64_t ndraw, double* out, double* scratch, void* stream) {
    (void)scratch; (void)stream;
    if (nrow < 1 || nrow > EFD_NOISE_MAX_ROWS)
        return efdcpu::fail(EFD_ERR_ARG, "efd_noise_overlap_rows_cpu: nrow outside 1..16");
    if (nchan < 1 || nbin < 1)
        return efdcpu::fail(EFD_ERR_ARG, "efd_noise_overlap_rows_cpu: nchan < 1 or nbin < 1");
    if (ndraw < 0 || (uint64_t)real0 + (uint64_t)ndraw > ((uint64_t)1 << 32))
        return efdcpu::fail(EFD_ERR_ARG,
                            "efd_noise_overlap_rows_cpu: real0 + ndraw outside 0..2^32");
    if (ndraw == 0) return EFD_OK;
    if (!rows || !out)
        return efdcpu::fail(EFD_ERR_ARG, "efd_noise_overlap_rows_cpu: NULL rows or out");
    const int64_t row_stride = (int64_t)nchan * nbin;
    for (int64_t d0 = 0; d0 < ndraw; d0 += 64) {
        const int nd = (int)std::min<int64_t>(64, ndraw - d0);
        chunk_sums(nbin, nd * nrow, out + d0 * nrow, [&](int64_t k0, int64_t k1, double* acc) {
            double hr[EFD_NOISE_MAX_ROWS], hi[EFD_NOISE_MAX_ROWS];
            for (int64_t k = k0; k < k1; ++k)
                for (int32_t c = 0; c < nchan; ++c) {
                    const int64_t e = (int64_t)c * nbin + k;
                    const double g = gain ? gain[e] : 1.0;
                    if (!efdnoise::live_gain(g)) continue;
                    for (int p = 0; p < nrow; ++p) {
                        hr[p] = g * rows[2 * (row_stride * p + e)];
                        hi[p] = g * rows[2 * (row_stride * p + e) + 1];
                    }
                    for (int j = 0; j < nd; ++j) {
                        double xr, xi;
                        efdnoise::draw_xi(seed, real0 + (uint32_t)(d0 + j), (uint32_t)c,
                                          (uint64_t)k, xr, xi);
                        double* a = acc + (int64_t)j * nrow;
                        for (int p = 0; p < nrow; ++p)
                            a[p] = std::fma(xr, hr[p], std::fma(xi, hi[p], a[p]));
                    }
                }
        });
    }
    return EFD_OK;
}

int efd_noise_philox_cpu(const uint32_t* counter, const uint32_t* key, uint32_t* words) {
    if (!counter || !key || !words)
        return efdcpu::fail(EFD_ERR_ARG, "efd_noise_philox_cpu: NULL argument");
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
    efdnoise::philox4x32_10(c, key[0], key[1]);
    for (int i = 0; i < 4; ++i) words[i] = c[i];
    return EFD_OK;
}

}  // extern "C"
