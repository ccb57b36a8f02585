// emrifd_reduce.hip -- the small kernels of libemrifd.so (MI355X, gfx950) that turn spectra into
// channels and numbers, and their C ABI (include/emrifd.h): the h+ / hx split
// (efd_polarizations), the log-likelihood and inner product (efd_loglike, efd_inner_product),
// the TD template's half-spectrum split and its fused likelihood (efd_td_split*), and the
// Fisher matrix's Gram kernel (efd_fisher_gram), and the overlaps of many rows with one fixed
// waveform (efd_overlap_rows), and the statistics of many row pairs of the mode-by-mode study
// (efd_pair_stats, efd_td_split_pair_stats, efd_window_rows), and <d|h> and <h|h> of written
// templates (efd_dh_hh_rows). Shares only emrifd_common.h with
// the mode sum (emrifd.hip) and the window path (emrifd_window.hip).

#include "emrifd_common.h"

namespace {

// h+ / hx split with FEW's array flip
__global__ void k_polarizations(const double2* __restrict__ S, int64_t nf, int64_t k0,
                                double2* __restrict__ hp, double2* __restrict__ hc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t k = k0 + i;
    if (k >= nf) return;
    const double2 a = S[k], b = S[nf - 1 - k];
    // h+ = (a + conj b)/2 ; hx = i (a - conj b)/2
    hp[i] = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
    hc[i] = make_double2(-0.5 * (a.y + b.y), 0.5 * (a.x - b.x));
}

// ---- the reductions' shared steps. Every reduction here promises bitwise reproducibility and
// that a row's numbers do not depend on the call's other rows; both rest on the orders written
// in this section and nowhere else. Every launch of this unit has RED_THREADS threads.
constexpr int RED_THREADS = 256;

// the workgroup's sum of each of v[0 .. N - 1] through LDS, all N behind one barrier sequence:
// the tree s = 128, 64, ..., 1. Every thread returns with the sums in v (thread 0 uses them).
template <int N>
__device__ __forceinline__ void block_sum(double* v) {
    __shared__ double red[N][RED_THREADS];
    const int tid = threadIdx.x;
#pragma unroll
    for (int n = 0; n < N; ++n) red[n][tid] = v[n];
    __syncthreads();
    for (int s = RED_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int n = 0; n < N; ++n) red[n][tid] += red[n][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = red[n][0];
}

// a wave's 64 lanes' sum by a butterfly: every lane ends with the same value
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The streaming reductions' workgroup epilogue: each of the thread's NS sums over its wave
// (wave_sum), the four waves' sums added as ((0 + 1) + 2) + 3, and sum i stored as this
// workgroup's partial of output o = out_of(i) at part[o gridDim.x + blockIdx.x] (o < 0: dropped).
template <int NS, class OutOf>
__device__ __forceinline__ void wg_store(const double (&v)[NS], double* __restrict__ part,
                                         OutOf out_of) {
    __shared__ double sm[4][NS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double x = wave_sum(v[i]);
        if (lane == 0) sm[wv][i] = x;
    }
    __syncthreads();
    if (tid < NS) {
        const double s = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
        const int64_t o = out_of(tid);
        if (o >= 0) part[o * gridDim.x + blockIdx.x] = s;
    }
}

// The one second pass: workgroup o adds output o's np partials part[o np ...] (thread t takes
// t, t + 256, ... in that order, then block_sum's tree) and writes out[o] = scale * sum.
__global__ __launch_bounds__(RED_THREADS) void k_final(const double* __restrict__ part, int np,
                                                       double scale, double* __restrict__ out) {
    part += (int64_t)blockIdx.x * np;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RED_THREADS) acc += part[i];
    block_sum<1>(&acc);
    if (threadIdx.x == 0) out[blockIdx.x] = scale * acc;
}

void launch_final(int nout, const double* part, int np, double scale, double* out,
                  hipStream_t st) {
    hipLaunchKernelGGL(k_final, dim3((unsigned)nout), dim3(RED_THREADS), 0, st, part, np, scale,
                       out);
}

// bins [k0, k1) of workgroup blockIdx.x of a row cut into chunks of `chunk` bins (row_chunks)
__device__ __forceinline__ void chunk_bounds(int64_t chunk, int64_t nb, int64_t& k0, int64_t& k1) {
    k0 = (int64_t)blockIdx.x * chunk;
    k1 = min(nb, k0 + chunk);
}

// f(std::integral_constant<int, V>{}) for the V of Vs that equals v (for none: nothing), so that
// a kernel's template arguments can follow run-time values
template <int... Vs, class F>
void for_value(int v, F f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// fused log-likelihood partials: one workgroup per chunk, then the second pass (k_final, -2)
__global__ void k_loglike_partial(const double2* __restrict__ h, const double2* __restrict__ d,
                                  const double* __restrict__ w, int64_t total,
                                  double* __restrict__ part) {
    // d - h*w rounded like the reference's numpy (product rounded, then difference): no FMA
    // contraction here, so a template equal to the injection gives exactly 0
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double2 dv = d[i];
        const double ww = w[i];
        double rr = dv.x, ri = dv.y;
        if (h) {
            const double2 hv = h[i];
            rr -= hv.x * ww;
            ri -= hv.y * ww;
        }
        acc = fma(rr, rr, fma(ri, ri, acc));
    }
    block_sum<1>(&acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ---- DFT of a TD template h = h+ - i hx into its two channels (efd_td_split*). Z = fft(w h)
// in natural order; the Hermitian split (k_polarizations' algebra, on the DFT's own pairing
// k <-> (n - k) mod n) gives both real series' transforms over the bins k < nb = ceil(n / 2),
// which are the drivers' positive-frequency bins (fftshift, then frequency >= 0):
//   H+ = (Z[k] + conj Z[n-k]) / 2,  Hx = i (Z[k] - conj Z[n-k]) / 2,  each times gain (= dt).
__device__ __forceinline__ void td_split_pair(const double2 a, const double2 b, double gain,
                                              double2& hp, double2& hc) {
#pragma clang fp contract(off)
    hp = make_double2(gain * (0.5 * (a.x + b.x)), gain * (0.5 * (a.y - b.y)));
    hc = make_double2(gain * (-0.5 * (a.y + b.y)), gain * (0.5 * (a.x - b.x)));
}

// The even-n rule of the split's reductions: the Nyquist bin Z[n / 2] belongs to neither
// channel's kept bins, but a NaN there still poisons the row, as one anywhere else does through
// the terms. True in the one thread of the row (thread 0 of chunk 0) that finds such a NaN, with
// the NaN its sums take in *poison.
__device__ __forceinline__ bool nyquist_nan(const double2* z, int64_t n, double* poison) {
    if (blockIdx.x != 0 || threadIdx.x != 0 || (n & 1) != 0) return false;
    const double2 v = z[n / 2];
    *poison = v.x + v.y;
    return v.x != v.x || v.y != v.y;
}

__global__ __launch_bounds__(256) void k_td_split(const double2* __restrict__ Z, int64_t stride,
                                                  int64_t n, int64_t nb, double gain,
                                                  const uint8_t* __restrict__ keep,
                                                  double2* __restrict__ out, int64_t out_stride) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nb) return;
    const double2* z = Z + (int64_t)blockIdx.y * stride;
    double2* o = out + (int64_t)blockIdx.y * out_stride;
    double2 hp = make_double2(0.0, 0.0), hc = hp;
    if (keep == nullptr || keep[k] != 0) td_split_pair(z[k], z[k == 0 ? 0 : n - k], gain, hp, hc);
    o[k] = hp;
    o[nb + k] = hc;
}

// logL partials of the split's channels against d ([2][nb]) and w ([2][nb]), the template kept
// in registers: workgroup (c, r) takes bins [c chunk, (c + 1) chunk) of row r, an ascending
// stream Z[k] and a descending one Z[n - k]; the row is the slow grid dimension, so the rows'
// workgroups of one chunk follow each other on one XCD and find d and w in its cache. Partials
// at part[r gridDim.x + c] (k_final's layout).
__global__ __launch_bounds__(256) void k_td_split_loglike(
    const double2* __restrict__ Z, int64_t stride, int64_t n, int64_t nb, int64_t chunk,
    double gain, const double2* __restrict__ d, const double* __restrict__ w,
    double* __restrict__ part) {
    // d - h w rounded as k_loglike_partial does (product, then difference)
#pragma clang fp contract(off)
    const double2* z = Z + (int64_t)blockIdx.y * stride;
    int64_t k0, k1;
    chunk_bounds(chunk, nb, k0, k1);
    double acc = 0.0, poison;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += 256) {
        double2 hp, hc;
        td_split_pair(z[k], z[k == 0 ? 0 : n - k], gain, hp, hc);
        const double2 d0 = d[k], d1 = d[nb + k];
        const double w0 = w[k], w1 = w[nb + k];
        const double ar = d0.x - hp.x * w0, ai = d0.y - hp.y * w0;
        const double br = d1.x - hc.x * w1, bi = d1.y - hc.y * w1;
        acc = fma(ar, ar, fma(ai, ai, acc));
        acc = fma(br, br, fma(bi, bi, acc));
    }
    if (nyquist_nan(z, n, &poison)) acc = poison;
    block_sum<1>(&acc);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// noise-weighted inner product partials: sum conj(a) b w (complex), one pair per workgroup; the
// real parts at part[blockIdx.x], the imaginary ones at part[gridDim.x + blockIdx.x] (k_final's
// layout for the two outputs re, im)
__global__ void k_inner_partial(const double2* __restrict__ a, const double2* __restrict__ b,
                                const double* __restrict__ w, int64_t total,
                                double* __restrict__ part) {
    double acc[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double2 av = a[i], bv = b[i];
        const double ww = w ? w[i] : 1.0;
        // conj(a) b = (ar br + ai bi) + i (ar bi - ai br)
        acc[0] = fma(ww, fma(av.x, bv.x, av.y * bv.y), acc[0]);
        acc[1] = fma(ww, fma(av.x, bv.y, -av.y * bv.x), acc[1]);
    }
    block_sum<2>(acc);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = acc[0];
        part[gridDim.x + blockIdx.x] = acc[1];
    }
}

// ---- weighted Gram matrix of stencil-combined rows (efd_fisher_gram) ----------------------
// One pass over h and w. A workgroup of 4 waves stages FG_CHUNK elements at a time: thread t
// forms D_i[e] = sum_s coef[i][s] h[i npoint + s][e] for its element (the stencil is applied per
// element, before any product: the Gram matrix of the raw rows combined afterwards loses the
// digits the differences cancel) and writes D_i and w to LDS, and D_i to dh. Then each wave
// takes 4 x 4 tiles (i, j) of the upper triangle's tile grid, its lanes run over the chunk's
// elements (lane l: l, l + 64, l + 128, l + 192; consecutive 16-byte LDS slots per read) and
// keep the tile's 16 sums in registers across the workgroup's chunks.
// What makes gram[i][j] a function of rows i, j, w and nelem alone (the subset promise):
//   - chunk c goes to workgroup c mod gridDim.x, and gridDim.x is a function of nelem;
//   - every pair sees the same element -> lane map, the same butterfly over the lanes and the
//     same final order over the workgroups, whichever wave and tile hold it;
//   - a term is fma(w, fma(ar, br, ai * bi), acc): symmetric in (a, b), so (j, i) of a
//     reordered call rounds as (i, j) does; contraction is off, the fmas are the written ones.
constexpr int FG_THREADS = 256;
constexpr int FG_CHUNK = 256;
constexpr int FG_MAXB = 1024;   // workgroups (4 per CU); EFD_FISHER_SCRATCH = FG_MAXB * 136

struct fg_coef {
    double c[EFD_FISHER_MAX_PARAMS * 4];
};

__host__ __device__ inline int fg_pair_index(int i, int j, int P) {   // i <= j, row-major upper
    return i * P - (i * (i - 1)) / 2 + (j - i);
}

// TP: tile rows = ceil(nparam / 4); the upper triangle has TP (TP + 1) / 2 tiles, wave v takes
// tiles v, v + 4, v + 8
template <int NPOINT, int TP>
__global__ __launch_bounds__(FG_THREADS) void k_fisher_partial(
    const double2* __restrict__ h, int64_t row_stride, int nparam, fg_coef cf,
    const double* __restrict__ w, int64_t nelem, double2* __restrict__ dh,
    double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int NTILE = TP * (TP + 1) / 2;
    constexpr int MAXT = (NTILE + 3) / 4;
    __shared__ double2 D[4 * TP * FG_CHUNK];
    __shared__ double wl[FG_CHUNK];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // rows nparam .. 4 TP - 1 pad the last tile row: zero, written once
    for (int r = nparam; r < 4 * TP; ++r) D[r * FG_CHUNK + tid] = make_double2(0.0, 0.0);
    int ti[MAXT], tj[MAXT];
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
        int t = wv + 4 * k, I = 0;
        while (I < TP - 1 && t >= TP - I) {   // tile row I holds TP - I tiles (J = I .. TP-1)
            t -= TP - I;
            ++I;
        }
        ti[k] = I;
        tj[k] = I + t;   // >= TP: this wave has no k-th tile
    }
    double acc[MAXT][16];
#pragma unroll
    for (int k = 0; k < MAXT; ++k)
#pragma unroll
        for (int p = 0; p < 16; ++p) acc[k][p] = 0.0;

    const int64_t nchunk = (nelem + FG_CHUNK - 1) / FG_CHUNK;
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t e = c * FG_CHUNK + tid;
        const bool live = e < nelem;
        wl[tid] = live ? (w ? w[e] : 1.0) : 0.0;
        for (int i = 0; i < nparam; ++i) {
            double dr = 0.0, di = 0.0;
            if (live) {
                const double2* r = h + row_stride * ((int64_t)i * NPOINT) + e;
                double2 v[NPOINT];
#pragma unroll
                for (int s = 0; s < NPOINT; ++s) v[s] = r[row_stride * s];
                const double c0 = cf.c[i * NPOINT];
                dr = c0 * v[0].x;
                di = c0 * v[0].y;
#pragma unroll
                for (int s = 1; s < NPOINT; ++s) {
                    const double cs = cf.c[i * NPOINT + s];
                    dr = fma(cs, v[s].x, dr);
                    di = fma(cs, v[s].y, di);
                }
                if (dh) dh[(int64_t)i * nelem + e] = make_double2(dr, di);
            }
            D[i * FG_CHUNK + tid] = make_double2(dr, di);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
            if (tj[k] >= TP) continue;
            const double2* A = D + 4 * ti[k] * FG_CHUNK;
            const double2* B = D + 4 * tj[k] * FG_CHUNK;
#pragma unroll
            for (int q = 0; q < FG_CHUNK / 64; ++q) {
                const int x = lane + 64 * q;
                const double ww = wl[x];
                double2 a[4], b[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a[r] = A[r * FG_CHUNK + x];
                    b[r] = B[r * FG_CHUNK + x];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc[k][4 * r + s] = fma(ww, fma(a[r].x, b[s].x, a[r].y * b[s].y),
                                                acc[k][4 * r + s]);
            }
        }
        __syncthreads();
    }
    // the 64 lanes' sums (wave_sum), lane 0 stores
    const int npair = nparam * (nparam + 1) / 2;
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
        if (tj[k] >= TP) continue;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const double v = wave_sum(acc[k][p]);
            const int gi = 4 * ti[k] + (p >> 2), gj = 4 * tj[k] + (p & 3);
            if (lane == 0 && gi <= gj && gj < nparam)
                part[(int64_t)blockIdx.x * npair + fg_pair_index(gi, gj, nparam)] = v;
        }
    }
}

// one workgroup per pair: the workgroups' partials in a fixed order, mirrored into both halves
__global__ void k_fisher_final(const double* __restrict__ part, int nb, int nparam,
                               double* __restrict__ gram) {
    const int npair = nparam * (nparam + 1) / 2;
    const int p = blockIdx.x;
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += RED_THREADS) acc += part[(int64_t)b * npair + p];
    block_sum<1>(&acc);
    if (threadIdx.x == 0) {
        int i = 0, q = p;
        while (q >= nparam - i) {
            q -= nparam - i;
            ++i;
        }
        const int j = i + q;
        const double g = 4.0 * acc;
        gram[i * nparam + j] = g;
        gram[j * nparam + i] = g;
    }
}

// ---- overlaps of many rows with one fixed waveform (efd_overlap_rows) ----------------------
// A streaming reduction with no cross-row products, so the rows are never staged in LDS.
// Workgroup (b, y) takes the 256-element chunks b, b + G, b + 2 G, ... (G = gridDim.x, a function
// of nelem alone) of the NR rows of row block y: a thread loads its element of t, u, w once,
// forms r = t - u, issues the 16-byte loads of its element of the block's NR rows together
// (8 rows x 256 threads x 16 B = 32 KiB in flight per workgroup) and keeps 3 NR sums in
// registers across the chunks. The epilogue is wg_store: a butterfly over the 64 lanes, the four
// waves' sums added as ((0 + 1) + 2) + 3, and one partial per (output, workgroup) at
// part[o G + b]; k_final adds each output's G partials in a fixed order and scales by 4.
// What makes out[3k .. 3k + 2] a function of row k, t, u, w and nelem alone (the subset
// promise): the element -> (workgroup, thread) map and both reduction orders depend on nelem
// only, and a row's terms never see another row, the row block's width or its position; the
// terms are the written fmas (contraction off), so every instantiation rounds alike.
constexpr int OV_THREADS = 256;
constexpr int OV_MAXB = 1024;   // workgroups per row block (4 per CU)
constexpr int OV_RB = 8;        // rows per full block
typedef double ov_d2 __attribute__((ext_vector_type(2)));

// row0: the first row of block y = 0 of this launch; the |r|^2 sum belongs to row 0's block.
// Row k's sums (re, im, nn) are acc[3 k .. 3 k + 2], the |r|^2 sum is acc[3 NR]
template <int NR>
__global__ __launch_bounds__(OV_THREADS) void k_overlap_partial(
    const double2* __restrict__ h, int64_t row_stride, int row0, int nrow,
    const double2* __restrict__ t, const double2* __restrict__ u, const double* __restrict__ w,
    int64_t nelem, double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int NS = 3 * NR + 1;
    const int tid = threadIdx.x;
    const int first = row0 + (int)blockIdx.y * NR;
    const double2* hb = h + row_stride * (int64_t)first;
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;

    const int64_t nchunk = (nelem + OV_THREADS - 1) / OV_THREADS;
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t e = c * OV_THREADS + tid;
        if (e >= nelem) continue;
        double2 v[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) {   // read once: streamed past the caches t, u, w stay in
            const ov_d2 x = __builtin_nontemporal_load((const ov_d2*)(hb + (row_stride * k + e)));
            v[k] = make_double2(x.x, x.y);
        }
        double2 r = t[e];
        if (u) {
            const double2 uv = u[e];
            r.x -= uv.x;
            r.y -= uv.y;
        }
        const double ww = w ? w[e] : 1.0;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            acc[3 * k] = fma(ww, fma(v[k].x, r.x, v[k].y * r.y), acc[3 * k]);
            acc[3 * k + 1] = fma(ww, fma(v[k].x, r.y, -(v[k].y * r.x)), acc[3 * k + 1]);
            acc[3 * k + 2] = fma(ww, fma(v[k].x, v[k].x, v[k].y * v[k].y), acc[3 * k + 2]);
        }
        if (first == 0) acc[3 * NR] = fma(ww, fma(r.x, r.x, r.y * r.y), acc[3 * NR]);
    }
    wg_store(acc, part, [=](int i) {
        return i < 3 * NR ? (int64_t)(3 * first + i) : first == 0 ? (int64_t)(3 * nrow) : -1;
    });
}

template <int NR>
void ov_launch(int nb, int blocks, hipStream_t st, const double2* h, int64_t row_stride, int row0,
               int nrow, const double2* t, const double2* u, const double* w, int64_t nelem,
               double* part) {
    hipLaunchKernelGGL((k_overlap_partial<NR>), dim3(nb, blocks), dim3(OV_THREADS), 0, st, h,
                       row_stride, row0, nrow, t, u, w, nelem, part);
}

// ---- statistics of many (a, b) row pairs (efd_pair_stats, efd_td_split_pair_stats) ----------
// A streaming reduction again: workgroup (c, r) takes bins [c chunk, (c + 1) chunk) of row pair
// r, both channels, so a thread loads w[k] (and keep[k]) once for its bin and keeps five sums per
// channel in registers. The row is the slow grid dimension: the workgroups of one chunk follow
// each other on one XCD (the chunk count is a multiple of 8 once there are that many) and find w
// and keep in its cache, while a and b (or Z) are read once and streamed past it. The epilogue
// is k_overlap_partial's (wg_store): a butterfly over the 64 lanes, the four waves' sums added
// as ((0 + 1) + 2) + 3, one partial per (output, workgroup) at part[o gridDim.x + c]; then
// k_final adds each output's partials in a fixed order and scales by 4.
// What makes a row's numbers a function of that row pair, w and the sizes alone: the bin ->
// (workgroup, thread) map and both reduction orders depend on nbin (n) only, a row's terms never
// see another row or its own position, and the terms are the written ones (contraction off).
constexpr int PS_THREADS = 256;
constexpr int PS_MAXB = 1024;   // chunks per row (4 workgroups per CU for a single row)

// one bin of one channel into its five sums. abi's term is the difference of two rounded
// products, not an fma: ar bi and ai br are then the same number when b == a, so it is exactly 0
__device__ __forceinline__ void ps_term(double w, const double2 a, const double2 b, double* s) {
#pragma clang fp contract(off)
    const double dr = a.x - b.x, di = a.y - b.y;
    s[0] = fma(w, fma(a.x, a.x, a.y * a.y), s[0]);
    s[1] = fma(w, fma(b.x, b.x, b.y * b.y), s[1]);
    s[2] = fma(w, fma(a.x, b.x, a.y * b.y), s[2]);
    s[3] = fma(w, a.x * b.y - a.y * b.x, s[3]);
    s[4] = fma(w, fma(dr, dr, di * di), s[4]);
}

__device__ __forceinline__ double2 ps_stream(const double2* p) {
    const ov_d2 x = __builtin_nontemporal_load((const ov_d2*)p);
    return make_double2(x.x, x.y);
}

// the workgroup's NS = 5 NCHAN sums (s[5 c + i]: sum i of channel c) as the partials of row
// blockIdx.y's outputs: part[((r NCHAN + c) 5 + i) gridDim.x + blockIdx.x]
template <int NS>
__device__ __forceinline__ void ps_store(const double (&s)[NS], double* __restrict__ part) {
    wg_store(s, part, [](int i) { return (int64_t)blockIdx.y * NS + i; });
}

template <int NCHAN>
__global__ __launch_bounds__(PS_THREADS) void k_pair_stats(
    const double2* __restrict__ a, int64_t a_stride, const double2* __restrict__ b,
    int64_t b_stride, const double* __restrict__ w, int64_t nbin, int64_t chunk,
    double* __restrict__ part) {
    const double2* ar = a + (int64_t)blockIdx.y * a_stride;
    const double2* br = b + (int64_t)blockIdx.y * b_stride;
    int64_t k0, k1;
    chunk_bounds(chunk, nbin, k0, k1);
    double s[5 * NCHAN];
#pragma unroll
    for (int i = 0; i < 5 * NCHAN; ++i) s[i] = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += PS_THREADS) {
        double2 av[NCHAN], bv[NCHAN];
#pragma unroll
        for (int c = 0; c < NCHAN; ++c) {
            av[c] = ps_stream(ar + (c * nbin + k));
            bv[c] = ps_stream(br + (c * nbin + k));
        }
        const double ww = w ? w[k] : 1.0;
#pragma unroll
        for (int c = 0; c < NCHAN; ++c) ps_term(ww, av[c], bv[c], s + 5 * c);
    }
    ps_store(s, part);
}

// the same with b = the split of row r of Z (k_td_split's arithmetic and keep rule), kept in
// registers: an ascending stream Z[k] and a descending one Z[n - k], as k_td_split_loglike
__global__ __launch_bounds__(PS_THREADS) void k_td_split_pair_stats(
    const double2* __restrict__ Z, int64_t stride, int64_t n, int64_t nb, int64_t chunk,
    double gain, const double2* __restrict__ a, int64_t a_stride, const double* __restrict__ w,
    const uint8_t* __restrict__ keep, double* __restrict__ part) {
    const double2* z = Z + (int64_t)blockIdx.y * stride;
    const double2* ar = a + (int64_t)blockIdx.y * a_stride;
    int64_t k0, k1;
    chunk_bounds(chunk, nb, k0, k1);
    double s[10], poison;
#pragma unroll
    for (int i = 0; i < 10; ++i) s[i] = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += PS_THREADS) {
        const double2 a0 = ps_stream(ar + k), a1 = ps_stream(ar + (nb + k));
        double2 hp = make_double2(0.0, 0.0), hc = hp;
        if (keep == nullptr || keep[k] != 0)
            td_split_pair(ps_stream(z + k), ps_stream(z + (k == 0 ? 0 : n - k)), gain, hp, hc);
        const double ww = w ? w[k] : 1.0;
        ps_term(ww, a0, hp, s);
        ps_term(ww, a1, hc, s + 5);
    }
    // a NaN in the Nyquist bin poisons every number of the row that depends on b
    if (nyquist_nan(z, n, &poison))
        for (int c = 0; c < 2; ++c)
            for (int i = 1; i < 5; ++i) s[5 * c + i] = poison;
    ps_store(s, part);
}

// <d|h> and <h|h> of written rows (efd_dh_hh_rows): k_pair_stats' shape with the mode sum
// epilogue's terms (dh_term on h w, each component's product rounded); w is per channel here.
// Workgroup (c, y) takes bins [c chunk, (c + 1) chunk) of the rows DH_RB y .. DH_RB y + DH_RB - 1:
// a thread loads its bin's d and w once for all of them (d and w are 1.5 times a row's bytes;
// one row per workgroup re-read them per row and ran at 0.55 ms for 16 rows of config 2's grid)
// and keeps three sums per row. A row's terms and their order are those of a call with that row
// alone: its numbers do not depend on the block it sits in.
constexpr int DH_RB = 8;

template <int NCHAN>
__global__ __launch_bounds__(PS_THREADS) void k_dh_hh_rows(
    const double2* __restrict__ h, int64_t row_stride, int nrow, const double2* __restrict__ d,
    const double* __restrict__ w, int64_t nbin, int64_t chunk, double* __restrict__ part) {
#pragma clang fp contract(off)
    const int row0 = (int)blockIdx.y * DH_RB;
    const int nr = min(DH_RB, nrow - row0);
    const double2* hb = h + (int64_t)row0 * row_stride;
    int64_t k0, k1;
    chunk_bounds(chunk, nbin, k0, k1);
    double s[3 * DH_RB];
#pragma unroll
    for (int i = 0; i < 3 * DH_RB; ++i) s[i] = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += PS_THREADS) {
        double2 dv[NCHAN];
        double ww[NCHAN];
#pragma unroll
        for (int c = 0; c < NCHAN; ++c) {
            dv[c] = d[c * nbin + k];
            ww[c] = w[c * nbin + k];
        }
#pragma unroll
        for (int r = 0; r < DH_RB; ++r) {
            if (r >= nr) break;   // (block-uniform)
            double2 hv[NCHAN];
#pragma unroll
            for (int c = 0; c < NCHAN; ++c) hv[c] = ps_stream(hb + (r * row_stride + c * nbin + k));
#pragma unroll
            for (int c = 0; c < NCHAN; ++c)
                dh_term(dv[c], make_double2(hv[c].x * ww[c], hv[c].y * ww[c]), s + 3 * r);
        }
    }
    wg_store(s, part, [=](int i) { return i < 3 * nr ? (int64_t)(3 * row0 + i) : (int64_t)-1; });
}

// out[j][k] = win[j][k] h[k]: every window of one series from one read of it
struct wr_ptrs {
    const double* p[EFD_WINDOW_MAX_ROWS];
};

__global__ __launch_bounds__(256) void k_window_rows(const double2* __restrict__ h, int64_t n,
                                                     wr_ptrs win, int nwin,
                                                     double2* __restrict__ out,
                                                     int64_t out_stride) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double2 v = h[k];
    for (int j = 0; j < nwin; ++j) {
        const double* wj = win.p[j];
        double2 o = v;
        if (wj) {
            const double x = wj[k];
            o = make_double2(x * v.x, x * v.y);
        }
        out[(int64_t)j * out_stride + k] = o;
    }
}

}  // namespace

void efdhip::launch_loglike_final(int rows, const double* part, int np, double* out,
                                  hipStream_t st) {
    launch_final(rows, part, np, -2.0, out, st);
}

// ========================================================================================
// C ABI
// ========================================================================================
extern "C" {

int efd_polarizations(const double* S, int64_t nf, int64_t k0, double* hp, double* hc,
                      void* stream) {
    if (!S || !hp || !hc || nf <= 0 || k0 < 0 || k0 > nf)
        return fail(EFD_ERR_ARG, "efd_polarizations: bad arguments");
    const int64_t cnt = nf - k0;
    if (cnt == 0) return EFD_OK;
    const int threads = 256;
    const int64_t blocks = (cnt + threads - 1) / threads;
    hipLaunchKernelGGL(k_polarizations, dim3((unsigned)blocks), dim3(threads), 0,
                       (hipStream_t)stream, (const double2*)S, nf, k0, (double2*)hp, (double2*)hc);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_loglike(const double* h, const double* d, const double* w, int32_t nchan, int64_t nbin,
                double* out, double* scratch, void* stream) {
    if (!d || !w || !out || !scratch || nchan <= 0 || nbin <= 0)
        return fail(EFD_ERR_ARG, "efd_loglike: bad arguments");
    const int64_t total = (int64_t)nchan * nbin;
    const int threads = 256;
    const int np = (int)std::min<int64_t>(EFD_LOGLIKE_SCRATCH, (total + threads - 1) / threads);
    hipStream_t st = (hipStream_t)stream;
    // fixed partition + fixed reduction tree: bitwise reproducible
    hipLaunchKernelGGL(k_loglike_partial, dim3(np), dim3(threads), 0, st, (const double2*)h,
                       (const double2*)d, w, total, scratch);
    HIP_TRY(hipGetLastError());
    launch_final(1, scratch, np, -2.0, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_inner_product(const double* a, const double* b, const double* w, int32_t nchan,
                      int64_t nbin, double* out, double* scratch, void* stream) {
    if (!a || !b || !out || !scratch || nchan <= 0 || nbin <= 0)
        return fail(EFD_ERR_ARG, "efd_inner_product: bad arguments");
    const int64_t total = (int64_t)nchan * nbin;
    const int threads = 256;
    const int np = (int)std::min<int64_t>(EFD_INNER_SCRATCH / 2, (total + threads - 1) / threads);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_inner_partial, dim3(np), dim3(threads), 0, st, (const double2*)a,
                       (const double2*)b, w, total, scratch);
    HIP_TRY(hipGetLastError());
    launch_final(2, scratch, np, 4.0, out, st);   // re, im
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

static_assert(EFD_FISHER_SCRATCH == FG_MAXB * (EFD_FISHER_MAX_PARAMS * (EFD_FISHER_MAX_PARAMS + 1) / 2),
              "EFD_FISHER_SCRATCH holds every workgroup's upper triangle");

int efd_fisher_gram(const double* h, int64_t row_stride, int32_t nparam, int32_t npoint,
                    const double* coef, const double* w, int64_t nelem, double* dh, double* gram,
                    double* scratch, void* stream) {
    if (nparam < 1 || nparam > EFD_FISHER_MAX_PARAMS)
        return fail(EFD_ERR_ARG, "efd_fisher_gram: nparam outside 1..16");
    if (npoint != 1 && npoint != 2 && npoint != 4)
        return fail(EFD_ERR_ARG, "efd_fisher_gram: npoint must be 1, 2 or 4");
    if (!h || !coef || !gram || !scratch)
        return fail(EFD_ERR_ARG, "efd_fisher_gram: NULL h, coef, gram or scratch");
    if (nelem <= 0) return fail(EFD_ERR_ARG, "efd_fisher_gram: nelem <= 0");
    if (row_stride < nelem) return fail(EFD_ERR_ARG, "efd_fisher_gram: row_stride < nelem");
    fg_coef cf;
    for (int i = 0; i < EFD_FISHER_MAX_PARAMS * 4; ++i)
        cf.c[i] = i < nparam * npoint ? coef[i] : 0.0;
    // the partition is a function of nelem alone
    const int nb = (int)std::min<int64_t>(FG_MAXB, (nelem + FG_CHUNK - 1) / FG_CHUNK);
    const int tp = (nparam + 3) / 4;
    hipStream_t st = (hipStream_t)stream;
    for_value<1, 2, 4>(npoint, [&](auto NP) {
        for_value<1, 2, 3, 4>(tp, [&](auto TP) {
            hipLaunchKernelGGL((k_fisher_partial<decltype(NP)::value, decltype(TP)::value>),
                               dim3(nb), dim3(FG_THREADS), 0, st, (const double2*)h, row_stride,
                               nparam, cf, w, nelem, (double2*)dh, scratch);
        });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fisher_final, dim3((unsigned)(nparam * (nparam + 1) / 2)), dim3(256), 0,
                       st, scratch, nb, nparam, gram);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

static_assert(EFD_OVERLAP_SCRATCH == OV_MAXB * (3 * EFD_OVERLAP_MAX_ROWS + 1),
              "EFD_OVERLAP_SCRATCH holds every workgroup's partial of every output");
static_assert(EFD_OVERLAP_MAX_ROWS % OV_RB == 0 && OV_RB == 8, "ov_launch's instantiations");
static_assert(OV_THREADS == RED_THREADS && PS_THREADS == RED_THREADS, "wg_store's four waves");

int efd_overlap_rows(const double* h, int64_t row_stride, int32_t nrow, const double* t,
                     const double* u, const double* w, int64_t nelem, double* out,
                     double* scratch, void* stream) {
    if (nrow < 1 || nrow > EFD_OVERLAP_MAX_ROWS)
        return fail(EFD_ERR_ARG, "efd_overlap_rows: nrow outside 1..64");
    if (!h || !t || !out || !scratch)
        return fail(EFD_ERR_ARG, "efd_overlap_rows: NULL h, t, out or scratch");
    if (nelem <= 0) return fail(EFD_ERR_ARG, "efd_overlap_rows: nelem <= 0");
    if (row_stride < nelem) return fail(EFD_ERR_ARG, "efd_overlap_rows: row_stride < nelem");
    // the partition is a function of nelem alone
    const int nb = (int)std::min<int64_t>(OV_MAXB, (nelem + OV_THREADS - 1) / OV_THREADS);
    const int full = nrow / OV_RB, rest = nrow % OV_RB;
    hipStream_t st = (hipStream_t)stream;
    const double2* h2 = (const double2*)h;
    const double2* t2 = (const double2*)t;
    const double2* u2 = (const double2*)u;
    if (full > 0) {
        ov_launch<OV_RB>(nb, full, st, h2, row_stride, 0, nrow, t2, u2, w, nelem, scratch);
        HIP_TRY(hipGetLastError());
    }
    const int r0 = full * OV_RB;   // the last, narrower block
    for_value<1, 2, 3, 4, 5, 6, 7>(rest, [&](auto NR) {
        ov_launch<decltype(NR)::value>(nb, 1, st, h2, row_stride, r0, nrow, t2, u2, w, nelem,
                                       scratch);
    });
    if (rest > 0) HIP_TRY(hipGetLastError());
    launch_final(3 * nrow + 1, scratch, nb, 4.0, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

static_assert(EFD_PAIR_SCRATCH == PS_MAXB * EFD_PAIR_MAX_ROWS * 2 * 5,
              "EFD_PAIR_SCRATCH holds every workgroup's partial of every output");
static_assert(EFD_TD_SPLIT_SCRATCH == PS_MAXB,
              "row_chunks' one cap is the most chunks a row of either reduction has");

// the chunks of a row of the TD split's likelihood (nbin = its nb) and of the pair statistics: a
// function of nbin alone (whole rounds of the 8 XCDs once there are that many), each a multiple
// of 256 bins and at least 1024 where nbin allows (four 16-byte loads per operand and thread)
static int row_chunks(int64_t nbin, int64_t* chunk) {
    int64_t np = std::min<int64_t>(PS_MAXB, (nbin + 1023) / 1024);
    if (np > 8) np -= np % 8;
    int64_t c = (nbin + np - 1) / np;
    c = (c + PS_THREADS - 1) / PS_THREADS * PS_THREADS;
    *chunk = c;
    return (int)((nbin + c - 1) / c);
}

int efd_td_split(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                 const uint8_t* keep, double* out, int64_t out_stride, void* stream) {
    if (!Z || !out) return fail(EFD_ERR_ARG, "efd_td_split: NULL Z or out");
    if (n < 1 || n > ((int64_t)1 << 40)) return fail(EFD_ERR_ARG, "efd_td_split: n out of range");
    if (rows < 1) return fail(EFD_ERR_ARG, "efd_td_split: rows < 1");
    const int64_t nb = (n + 1) / 2;
    if (stride < n) return fail(EFD_ERR_ARG, "efd_td_split: stride < n");
    if (out_stride < 2 * nb) return fail(EFD_ERR_ARG, "efd_td_split: out_stride < 2 nb");
    const int64_t blocks = (nb + 255) / 256;
    if (blocks > 0x7fffffffLL || rows > 65535)
        return fail(EFD_ERR_ARG, "efd_td_split: too many bins or rows");
    hipLaunchKernelGGL(k_td_split, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0,
                       (hipStream_t)stream, (const double2*)Z, stride, n, nb, gain, keep,
                       (double2*)out, out_stride);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_td_split_loglike(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                         const double* d, const double* w, double* out, double* scratch,
                         void* stream) {
    if (!Z || !d || !w || !out || !scratch)
        return fail(EFD_ERR_ARG, "efd_td_split_loglike: NULL Z, d, w, out or scratch");
    if (n < 1 || n > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_td_split_loglike: n out of range");
    if (rows < 1 || rows > 65535) return fail(EFD_ERR_ARG, "efd_td_split_loglike: rows out of range");
    if (stride < n) return fail(EFD_ERR_ARG, "efd_td_split_loglike: stride < n");
    const int64_t nb = (n + 1) / 2;
    int64_t chunk = 0;
    const int np = row_chunks(nb, &chunk);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_td_split_loglike, dim3((unsigned)np, (unsigned)rows), dim3(256), 0, st,
                       (const double2*)Z, stride, n, nb, chunk, gain, (const double2*)d, w, scratch);
    HIP_TRY(hipGetLastError());
    launch_final(rows, scratch, np, -2.0, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_pair_stats(const double* a, int64_t a_stride, const double* b, int64_t b_stride,
                   int32_t nrow, int32_t nchan, int64_t nbin, const double* w, double* out,
                   double* scratch, void* stream) {
    if (nrow < 1 || nrow > EFD_PAIR_MAX_ROWS)
        return fail(EFD_ERR_ARG, "efd_pair_stats: nrow outside 1..64");
    if (nchan != 1 && nchan != 2) return fail(EFD_ERR_ARG, "efd_pair_stats: nchan must be 1 or 2");
    if (!a || !b || !out || !scratch)
        return fail(EFD_ERR_ARG, "efd_pair_stats: NULL a, b, out or scratch");
    if (nbin <= 0 || nbin > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_pair_stats: nbin out of range");
    if (a_stride < nchan * nbin || b_stride < nchan * nbin)
        return fail(EFD_ERR_ARG, "efd_pair_stats: stride < nchan nbin");
    int64_t chunk = 0;
    const int np = row_chunks(nbin, &chunk);
    hipStream_t st = (hipStream_t)stream;
    for_value<1, 2>(nchan, [&](auto NC) {
        hipLaunchKernelGGL((k_pair_stats<decltype(NC)::value>), dim3((unsigned)np, (unsigned)nrow),
                           dim3(PS_THREADS), 0, st, (const double2*)a, a_stride, (const double2*)b,
                           b_stride, w, nbin, chunk, scratch);
    });
    HIP_TRY(hipGetLastError());
    launch_final(nrow * nchan * 5, scratch, np, 4.0, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

static_assert(EFD_DH_SCRATCH == PS_MAXB * EFD_DH_MAX_ROWS * 3,
              "EFD_DH_SCRATCH holds every workgroup's partial of every output");

int efd_dh_hh_rows(const double* h, int64_t row_stride, int32_t nrow, const double* d,
                   const double* w, int32_t nchan, int64_t nbin, double* out, double* scratch,
                   void* stream) {
    if (nrow < 1 || nrow > EFD_DH_MAX_ROWS)
        return fail(EFD_ERR_ARG, "efd_dh_hh_rows: nrow outside 1..64");
    if (nchan != 1 && nchan != 2) return fail(EFD_ERR_ARG, "efd_dh_hh_rows: nchan must be 1 or 2");
    if (!h || !d || !w || !out || !scratch)
        return fail(EFD_ERR_ARG, "efd_dh_hh_rows: NULL h, d, w, out or scratch");
    if (nbin <= 0 || nbin > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_dh_hh_rows: nbin out of range");
    if (row_stride < nchan * nbin)
        return fail(EFD_ERR_ARG, "efd_dh_hh_rows: row_stride < nchan nbin");
    int64_t chunk = 0;
    const int np = row_chunks(nbin, &chunk);
    hipStream_t st = (hipStream_t)stream;
    for_value<1, 2>(nchan, [&](auto NC) {
        hipLaunchKernelGGL((k_dh_hh_rows<decltype(NC)::value>),
                           dim3((unsigned)np, (unsigned)((nrow + DH_RB - 1) / DH_RB)),
                           dim3(PS_THREADS), 0, st, (const double2*)h, row_stride, (int)nrow,
                           (const double2*)d, w, nbin, chunk, scratch);
    });
    HIP_TRY(hipGetLastError());
    launch_final(nrow * 3, scratch, np, 4.0, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_td_split_pair_stats(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                            const double* a, int64_t a_stride, const double* w,
                            const uint8_t* keep, double* out, double* scratch, void* stream) {
    if (!Z || !a || !out || !scratch)
        return fail(EFD_ERR_ARG, "efd_td_split_pair_stats: NULL Z, a, out or scratch");
    if (n < 1 || n > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_td_split_pair_stats: n out of range");
    if (rows < 1 || rows > EFD_PAIR_MAX_ROWS)
        return fail(EFD_ERR_ARG, "efd_td_split_pair_stats: rows outside 1..64");
    if (stride < n) return fail(EFD_ERR_ARG, "efd_td_split_pair_stats: stride < n");
    const int64_t nb = (n + 1) / 2;
    if (a_stride < 2 * nb) return fail(EFD_ERR_ARG, "efd_td_split_pair_stats: a_stride < 2 nb");
    int64_t chunk = 0;
    const int np = row_chunks(nb, &chunk);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_td_split_pair_stats, dim3((unsigned)np, (unsigned)rows), dim3(PS_THREADS),
                       0, st, (const double2*)Z, stride, n, nb, chunk, gain, (const double2*)a,
                       a_stride, w, keep, scratch);
    HIP_TRY(hipGetLastError());
    launch_final(rows * 10, scratch, np, 4.0, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_window_rows(const double* h, int64_t n, const double* const* win, int32_t nwin,
                    double* out, int64_t out_stride, void* stream) {
    if (!h || !win || !out) return fail(EFD_ERR_ARG, "efd_window_rows: NULL h, win or out");
    if (n < 1 || n > ((int64_t)1 << 38))
        return fail(EFD_ERR_ARG, "efd_window_rows: n out of range");
    if (nwin < 1 || nwin > EFD_WINDOW_MAX_ROWS)
        return fail(EFD_ERR_ARG, "efd_window_rows: nwin outside 1..16");
    if (out_stride < n) return fail(EFD_ERR_ARG, "efd_window_rows: out_stride < n");
    wr_ptrs p;
    for (int j = 0; j < EFD_WINDOW_MAX_ROWS; ++j) p.p[j] = j < nwin ? win[j] : nullptr;
    hipLaunchKernelGGL(k_window_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const double2*)h, n, p, (int)nwin, (double2*)out,
                       out_stride);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

}  // extern "C"
