// emrifd_noise.hip -- noise realisations of libemrifd.so (MI355X, gfx950): the counter-based
// draws of emrifd_noise.h written to a buffer (efd_noise_fd) and contracted with a set of rows
// without ever being written (efd_noise_overlap_rows). A draw is a function of (seed,
// realisation, channel, bin) alone, so neither result depends on the launch geometry. Shares
// emrifd_common.h with the other units and emrifd_noise.h with the host twins.

#include "emrifd_common.h"
#include "emrifd_noise.h"

namespace {

constexpr int NZ_THREADS = 256;
constexpr int NZ_FD_MAXB = 2048;   // efd_noise_fd's workgroups per channel (8 per CU)

// out[c][i] (+)= gain[c][i] * 0.5 * xi(c, bin0 + i): one bin per lane and pass, one 16-byte
// store each; the channel is the slow grid dimension. A bin whose gain is 0 or NaN is written as
// 0 (left alone under accumulate) without a draw.
__global__ __launch_bounds__(NZ_THREADS) void k_noise_fd(
    double2* __restrict__ out, const double* __restrict__ gain, int64_t nbin, uint64_t bin0,
    uint64_t seed, uint32_t realisation, int accumulate) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.y;
    double2* o = out + (int64_t)c * nbin;
    const double* g = gain ? gain + (int64_t)c * nbin : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * NZ_THREADS + threadIdx.x; i < nbin;
         i += (int64_t)gridDim.x * NZ_THREADS) {
        const double gv = g ? g[i] : 1.0;
        if (!efdnoise::live_gain(gv)) {
            if (!accumulate) o[i] = make_double2(0.0, 0.0);
            continue;
        }
        double xr, xi;
        efdnoise::draw_xi(seed, realisation, c, bin0 + (uint64_t)i, xr, xi);
        const double s = 0.5 * gv;
        double2 v = make_double2(s * xr, s * xi);
        if (accumulate) {
            const double2 old = o[i];
            v.x += old.x;
            v.y += old.y;
        }
        o[i] = v;
    }
}

// ---- overlaps of many draws with a set of rows (efd_noise_overlap_rows) ---------------------
// Workgroup (y, b) takes the 256-bin chunks b, b + G, b + 2 G, ... (G = gridDim.y, a function of
// nbin alone) and the NZ_DB draws real0 + NZ_DB y ...: a thread loads its bin of the NR rows once
// per channel, multiplies the gain in, and then regenerates the bin's noise draw by draw in
// registers (about 10^2 integer and FP64 operations each) against 2 NR fmas per draw. It keeps
// NZ_DB NR sums across its chunks. The draw block is the fast grid dimension, so the workgroups
// that re-read the same chunks of the rows (ndraw / NZ_DB times in all, plain loads) follow each
// other; the kernel is bound by the draws' arithmetic either way (6 rows x 1024 draws on config
// 2's grid: 60.5 ms with the chunks or the draw blocks fastest). The
// epilogue is the reduction units' pattern: a butterfly over the 64 lanes, the four waves' sums
// added as ((0 + 1) + 2) + 3, one partial per (output, workgroup) at part[o G + b];
// k_noise_final adds each output's G partials in a fixed order.
// What makes out[r][p] a function of (seed, r, row p, gain, nchan, nbin) alone: the bin ->
// (workgroup, thread) map and both reduction orders depend on nbin only, a term never sees
// another row or draw, its slot in the draw block or the block's width, and the terms are the
// written fmas (contraction off), so every instantiation rounds alike.
constexpr int NZ_DB = 8;      // draws per workgroup
constexpr int NZ_RB = 8;      // rows per launch (EFD_NOISE_MAX_ROWS in two)
constexpr int NZ_MAXB = 256;  // chunk workgroups per draw block (one per CU)

__device__ __forceinline__ double nz_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// rows: the first of this launch's NR rows; row0 its index in the call; real0: the launch's
// first draw (the scratch's draw slot 0); nd: draws of this launch
template <int NR>
__global__ __launch_bounds__(NZ_THREADS) void k_noise_overlap_partial(
    const double2* __restrict__ rows, int64_t row_stride, int row0, int nrow,
    const double* __restrict__ gain, int nchan, int64_t nbin, uint64_t seed, uint32_t real0,
    int nd, double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int NS = NZ_DB * NR;
    __shared__ double sm[4][NS];
    const int tid = threadIdx.x;
    const int j0 = (int)blockIdx.x * NZ_DB;        // first draw slot of this workgroup
    const int nj = min(NZ_DB, nd - j0);            // (block-uniform)
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;

    const int64_t nchunk = (nbin + NZ_THREADS - 1) / NZ_THREADS;
    for (int64_t ch = blockIdx.y; ch < nchunk; ch += gridDim.y) {
        const int64_t k = ch * NZ_THREADS + tid;
        if (k >= nbin) continue;
        for (int c = 0; c < nchan; ++c) {
            const int64_t e = (int64_t)c * nbin + k;
            const double g = gain ? gain[e] : 1.0;
            if (!efdnoise::live_gain(g)) continue;
            double2 v[NR];
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const double2 x = rows[row_stride * p + e];
                v[p] = make_double2(g * x.x, g * x.y);
            }
#pragma unroll
            for (int j = 0; j < NZ_DB; ++j) {
                if (j >= nj) break;
                double xr, xi;
                efdnoise::draw_xi(seed, real0 + (uint32_t)(j0 + j), (uint32_t)c, (uint64_t)k, xr, xi);
#pragma unroll
                for (int p = 0; p < NR; ++p)
                    acc[j * NR + p] = fma(xr, v[p].x, fma(xi, v[p].y, acc[j * NR + p]));
            }
        }
    }
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double x = nz_wave_sum(acc[i]);
        if (lane == 0) sm[wv][i] = x;
    }
    __syncthreads();
    if (tid < NS) {
        const int j = tid / NR, p = tid % NR;
        if (j < nj) {
            const double s = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
            const int64_t o = (int64_t)(j0 + j) * nrow + row0 + p;
            part[o * gridDim.y + blockIdx.y] = s;
        }
    }
}

// workgroup o adds output o's np <= NZ_MAXB partials part[o np ...]: thread t holds partial t,
// then the tree s = 128, 64, ..., 1
__global__ __launch_bounds__(NZ_THREADS) void k_noise_final(const double* __restrict__ part,
                                                            int np, double* __restrict__ out) {
    __shared__ double red[NZ_THREADS];
    const int tid = threadIdx.x;
    red[tid] = tid < np ? part[(int64_t)blockIdx.x * np + tid] : 0.0;
    __syncthreads();
    for (int s = NZ_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0];
}

template <int NR>
void nz_launch(int nb, int nd, hipStream_t st, const double2* rows, int64_t row_stride, int row0,
               int nrow, const double* gain, int nchan, int64_t nbin, uint64_t seed,
               uint32_t real0, double* part) {
    hipLaunchKernelGGL((k_noise_overlap_partial<NR>), dim3((nd + NZ_DB - 1) / NZ_DB, nb),
                       dim3(NZ_THREADS), 0, st, rows + row_stride * row0, row_stride, row0, nrow,
                       gain, nchan, nbin, seed, real0, nd, part);
}

template <int... Vs, class F>
void nz_for_value(int v, F f) {
    (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

}  // namespace

extern "C" {

int efd_noise_fd(double* out, const double* gain, int32_t nchan, int64_t nbin, uint64_t bin0,
                 uint64_t seed, uint32_t realisation, int32_t accumulate, void* stream) {
    if (nbin == 0) return EFD_OK;
    if (!out) return fail(EFD_ERR_ARG, "efd_noise_fd: NULL out");
    if (nchan < 1 || nchan > 65535) return fail(EFD_ERR_ARG, "efd_noise_fd: nchan outside 1..65535");
    if (nbin < 0 || nbin > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_noise_fd: nbin out of range");
    const int nb = (int)std::min<int64_t>(NZ_FD_MAXB, (nbin + NZ_THREADS - 1) / NZ_THREADS);
    hipLaunchKernelGGL(k_noise_fd, dim3((unsigned)nb, (unsigned)nchan), dim3(NZ_THREADS), 0,
                       (hipStream_t)stream, (double2*)out, gain, nbin, bin0, seed, realisation,
                       accumulate != 0);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

static_assert(EFD_NOISE_MAX_ROWS == 2 * NZ_RB, "efd_noise_overlap_rows' two row launches");
static_assert(EFD_NOISE_DRAWS_PER_LAUNCH % NZ_DB == 0, "whole draw blocks per launch");
static_assert(EFD_NOISE_SCRATCH == NZ_MAXB * EFD_NOISE_DRAWS_PER_LAUNCH * EFD_NOISE_MAX_ROWS,
              "EFD_NOISE_SCRATCH holds every workgroup's partial of every output of a launch");

int efd_noise_overlap_rows(const double* rows, int32_t nrow, const double* gain, int32_t nchan,
                           int64_t nbin, uint64_t seed, uint32_t real0, int64_t ndraw, double* out,
                           double* scratch, void* stream) {
    if (nrow < 1 || nrow > EFD_NOISE_MAX_ROWS)
        return fail(EFD_ERR_ARG, "efd_noise_overlap_rows: nrow outside 1..16");
    if (nchan < 1 || nchan > 65535)
        return fail(EFD_ERR_ARG, "efd_noise_overlap_rows: nchan outside 1..65535");
    if (nbin < 1 || nbin > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_noise_overlap_rows: nbin out of range");
    if (ndraw < 0 || (uint64_t)real0 + (uint64_t)ndraw > ((uint64_t)1 << 32))
        return fail(EFD_ERR_ARG, "efd_noise_overlap_rows: real0 + ndraw outside 0..2^32");
    if (ndraw == 0) return EFD_OK;
    if (!rows || !out || !scratch)
        return fail(EFD_ERR_ARG, "efd_noise_overlap_rows: NULL rows, out or scratch");
    // the partition is a function of nbin alone
    const int nb = (int)std::min<int64_t>(NZ_MAXB, (nbin + NZ_THREADS - 1) / NZ_THREADS);
    const int64_t row_stride = (int64_t)nchan * nbin;
    hipStream_t st = (hipStream_t)stream;
    const double2* r2 = (const double2*)rows;
    for (int64_t d0 = 0; d0 < ndraw; d0 += EFD_NOISE_DRAWS_PER_LAUNCH) {
        const int nd = (int)std::min<int64_t>(EFD_NOISE_DRAWS_PER_LAUNCH, ndraw - d0);
        const uint32_t r0 = real0 + (uint32_t)d0;
        for (int p0 = 0; p0 < nrow; p0 += NZ_RB) {
            nz_for_value<1, 2, 3, 4, 5, 6, 7, 8>(std::min(NZ_RB, nrow - p0), [&](auto NR) {
                nz_launch<decltype(NR)::value>(nb, nd, st, r2, row_stride, p0, nrow, gain, nchan,
                                               nbin, seed, r0, scratch);
            });
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_noise_final, dim3((unsigned)(nd * nrow)), dim3(NZ_THREADS), 0, st,
                           scratch, nb, out + d0 * nrow);
        HIP_TRY(hipGetLastError());
    }
    return EFD_OK;
}

}  // extern "C"
