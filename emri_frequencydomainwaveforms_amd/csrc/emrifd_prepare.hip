// emrifd_prepare.hip -- the mode sum's preparation, K0-K5 of the pipeline mapped at the top of
// emrifd.hip: the (m, n) groups and their amplitudes (k_group*), the not-a-knot splines by
// Thomas chains or parallel cyclic reduction (k_prep*, k_spline_shared), the interval records
// (k_items) and the segment table (k_segment_*, k_seg_tiles, k_segments_one), with their host
// side: efd_modesum_prepare, efd_modesum_prepare_batch, efd_spline_build and the TD sum's
// preparation. It writes the workspace (emrifd_layout.h) that emrifd.hip's K6-K9 read, and uses
// nothing else of that unit's device code; the chain ends by launching K6 there. Every stage is
// one kernel that takes the batch descriptor by value and reads its waveform's inputs and
// workspace buffers through a PrepView; the TD sum's preparation is a batch of one through the
// first three of them.

#include "emrifd_layout.h"

namespace {

// rows of scratch / knot data fetched per block ahead of the serial spline recurrences
constexpr int SPLINE_PF = 8;   // 16: same, 32: slower (k_prep 110 -> 177 us)

// 1/x for the spline solves: the hardware reciprocal estimate and two Newton steps (5 dependent
// operations, within an ulp) instead of the IEEE division sequence (~10, with the scale and
// fixup steps) on the serial Thomas chains, whose latency sets the preparation's length; the
// coefficients stay within 1e-11 of scipy's (tests/test_gpu_modesum.py), their rounding level
__device__ __forceinline__ double spl_rcp(double x) {
#ifdef EFD_EXP_EXACT_RCP   // experiment: IEEE division (the host twin's), for the HIP = twin study
    return 1.0 / x;
#endif
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}

// ----------------------------------------------------------------------------------------
// Not-a-knot cubic spline solve (scipy.interpolate.CubicSpline semantics)
// ----------------------------------------------------------------------------------------
// Slopes s_i solve the tridiagonal system of scipy/_cubic.py (rows 0 and n-1 encode the
// not-a-knot end conditions); coefficients follow scipy's PPoly construction:
//   tt = (s_i + s_{i+1} - 2 slope_i)/dx_i; c0 = tt/dx_i; c1 = (slope_i - s_i)/dx_i - tt;
//   c2 = s_i; c3 = y_i.
// X(i), Y(i) load knot i; CP/DP are per-lane scratch accessors; OUT(i, c, v) stores.
template <class FX, class FY, class FCP, class FDP, class FOUT>
__device__ void spline_not_a_knot(int n, FX X, FY Y, FCP CP, FDP DP, FOUT OUT) {
    if (n < 2) return;
    if (n == 2) {
        const double dx = X(1) - X(0);
        const double slope = (Y(1) - Y(0)) / dx;
        OUT(0, 0, 0.0); OUT(0, 1, 0.0); OUT(0, 2, slope); OUT(0, 3, Y(0));
        return;
    }
    if (n == 3) {  // parabola through the three points (scipy special case)
        const double dx0 = X(1) - X(0), dx1 = X(2) - X(1);
        const double y0 = Y(0), y1 = Y(1), y2 = Y(2);
        const double sl0 = (y1 - y0) / dx0, sl1 = (y2 - y1) / dx1;
        const double s1 = (dx0 * sl1 + dx1 * sl0) / (dx0 + dx1);
        const double s0 = 2.0 * sl0 - s1, s2 = 2.0 * sl1 - s1;
        double tt = (s0 + s1 - 2.0 * sl0) / dx0;
        OUT(0, 0, tt / dx0); OUT(0, 1, (sl0 - s0) / dx0 - tt); OUT(0, 2, s0); OUT(0, 3, y0);
        tt = (s1 + s2 - 2.0 * sl1) / dx1;
        OUT(1, 0, tt / dx1); OUT(1, 1, (sl1 - s1) / dx1 - tt); OUT(1, 2, s1); OUT(1, 3, y1);
        return;
    }
    // forward sweep (Thomas); row 0
    double x0 = X(0), x1 = X(1), x2 = X(2);
    double y0 = Y(0), y1 = Y(1), y2 = Y(2);
    double dxm = x1 - x0, dxi = x2 - x1;          // dx_{i-1}, dx_i at i = 1
    double slm = (y1 - y0) / dxm, sli = (y2 - y1) / dxi;
    {
        const double d = x2 - x0;
        const double b0 = dxi, c0 = d;
        const double r0 = ((dxm + 2.0 * d) * dxi * slm + dxm * dxm * sli) / d;
        CP(0) = c0 / b0;
        DP(0) = r0 / b0;
    }
    double cpm = CP(0), dpm = DP(0);
    double xi = x2, yi = y2;
    for (int i = 1; i <= n - 2; ++i) {
        // row i: a = dx_i, b = 2(dx_{i-1} + dx_i), c = dx_{i-1}, r = 3(dx_i sl_{i-1} + dx_{i-1} sl_i)
        const double a = dxi, b = 2.0 * (dxm + dxi), c = dxm;
        const double r = 3.0 * (dxi * slm + dxm * sli);
        const double inv = spl_rcp(b - a * cpm);   // one reciprocal on the serial chain
        cpm = c * inv;
        dpm = (r - a * dpm) * inv;
        CP(i) = cpm;
        DP(i) = dpm;
        if (i + 2 <= n - 1) {
            const double xn = X(i + 2), yn = Y(i + 2);
            dxm = dxi; slm = sli;
            dxi = xn - xi; sli = (yn - yi) * spl_rcp(dxi);
            xi = xn; yi = yn;
        }
    }
    // last row (scipy: A[1,-1] = dx[-2], A[-1,-2] = x[-1] - x[-3]): a = x_{n-1} - x_{n-3},
    // b = dx_{n-3}; here dxm = dx_{n-3}, dxi = dx_{n-2}, slm = sl_{n-3}, sli = sl_{n-2}
    double s_next;
    {
        const double d = dxm + dxi;  // x_{n-1} - x_{n-3}
        const double a = X(n - 1) - X(n - 3);
        const double b = dxm;
        const double r = (dxi * dxi * slm + (2.0 * d + dxi) * dxm * sli) / d;
        const double mm = b - a * cpm;
        s_next = (r - a * dpm) / mm;
    }
    // back substitution, emitting interval coefficients from the right. CP/DP may live in
    // global memory: they are fetched PF rows at a time (independent loads, one wait per
    // block) so the serial chain does not pay a memory round trip per row.
    constexpr int PF = SPLINE_PF;
    double xr = X(n - 1), yr = Y(n - 1);
    for (int i0 = n - 2; i0 >= 0; i0 -= PF) {
        double cpb[PF], dpb[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int i = i0 - k;
            cpb[k] = i >= 0 ? CP(i) : 0.0;
            dpb[k] = i >= 0 ? DP(i) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int i = i0 - k;
            if (i < 0) break;
            const double xl = X(i), yl = Y(i);
            const double s_i = dpb[k] - cpb[k] * s_next;
            // one reciprocal for the interval's four quotients (an FP64 division is a ~10-op
            // sequence; x * (1/dx) differs from x / dx by at most an ulp)
            const double rdx = spl_rcp(xr - xl);
            const double sl = (yr - yl) * rdx;
            const double tt = (s_i + s_next - 2.0 * sl) * rdx;
            OUT(i, 0, tt * rdx);
            OUT(i, 1, (sl - s_i) * rdx - tt);
            OUT(i, 2, s_i);
            OUT(i, 3, yl);
            s_next = s_i;
            xr = xl; yr = yl;
        }
    }
}

// derivative of a cubic piece at w (scipy evaluates c2 + 2 c1 w + 3 c0 w^2 by power sum)
__device__ __forceinline__ double dcubic(const double* c, double w) {
    return (c[2] + (2.0 * c[1]) * w) + (3.0 * c[0]) * (w * w);
}

// ----------------------------------------------------------------------------------------
// The same not-a-knot system solved by one wave with parallel cyclic reduction.
// spline_not_a_knot's Thomas sweeps are serial chains of ~2n dependent steps per interpolant,
// with CP/DP round trips through global memory: k_prep took 60-75 us at N_t ~ 100 (the longest
// kernel of a walker's preparation, and the preparation is the latency of small waveforms).
// Here every knot row is a lane's: scipy's two boundary rows are eliminated into rows 1 and
// n-2 (row 0: dx_1 s_0 + (x_2 - x_0) s_1 = r_0, and a_1 = dx_1, so s_0 drops out of row 1
// exactly; the same at the other end), the remaining tridiagonal system in s_1 .. s_{n-2}
// (diagonally dominant: b = 2 (a + c) inside) is normalised to b = 1 and reduced in
// ceil(log2(n - 2)) PCR steps, each row combining its neighbours at distance h:
//   row_k - A_k row_{k-h} - C_k row_{k+h}, renormalised,
// after which every row reads s_k = R_k. The boundary slopes follow from rows 0 and n-1, and
// the interval coefficients are scipy's PPoly construction, in parallel. The slopes agree with
// the Thomas solve to rounding (both are stable on this matrix).
// L: LDS scratch of 7 n doubles; at exit L[0, n) = x, L[n, 2n) = y, L[4n, 5n) = the knot
// slopes s_i. Called by every lane of a one-wave (64-thread) workgroup, 4 <= n <= PCR_NMAX.
// ----------------------------------------------------------------------------------------
constexpr int PCR_RPL = 8;                 // rows per lane
constexpr int PCR_NMAX = 64 * PCR_RPL;     // knots; longer trajectories take the Thomas kernel
// Waveforms of PCR_MAX_K harmonics or more keep the Thomas kernel's amplitude role (one lane per
// interpolant, k_prep_b): their preparation runs beside the previous batch's mode sum, where
// its length is hidden and its CU time is not. One wave per interpolant is ~10x the Thomas
// kernel's wave-time, and with every role on PCR config 2 (3,020 harmonics: 3,139 waves of
// ~10 us, 2,508 of them amplitude splines) lost 1.2% of its rate (paired A/B, ratio 0.988) while
// the latency-bound walker batches gained 6.6% (config 4) and 8.7% (config 5). The trajectory
// and inverse splines (the phases) always take one path for a given N_t, so a harmonic subset
// and the full set share them (the linearity test's 1e-12 bound).
#ifndef PCR_MAX_K
#define PCR_MAX_K 1024
#endif
template <class FX, class FY, class FOUT>
__device__ void pcr_not_a_knot(int n, FX X, FY Y, FOUT OUT, double* L) {
    const int lane = threadIdx.x;
    double* xs = L;
    double* ys = L + n;
    double* dx = L + 2 * n;
    double* sl = L + 3 * n;
    double* A = L + 4 * n;
    double* C = L + 5 * n;
    double* R = L + 6 * n;
    for (int i = lane; i < n; i += 64) {
        xs[i] = X(i);
        ys[i] = Y(i);
    }
    __syncthreads();
    for (int i = lane; i < n - 1; i += 64) {
        const double d = xs[i + 1] - xs[i];
        dx[i] = d;
        sl[i] = (ys[i + 1] - ys[i]) / d;
    }
    __syncthreads();
    const int m = n - 2;   // unknowns s_1 .. s_{n-2}: interior row k holds s_{k+1}
    // scipy's boundary rows: row 0 = (dx_1, x_2 - x_0 | r0), row n-1 = (x_{n-1} - x_{n-3}, dx_{n-3} | rl)
    const double d0 = xs[2] - xs[0];
    const double r0 = ((dx[0] + 2.0 * d0) * dx[1] * sl[0] + dx[0] * dx[0] * sl[1]) / d0;
    const double dl = xs[n - 1] - xs[n - 3];
    const double rl = (dx[n - 2] * dx[n - 2] * sl[n - 3] +
                       (2.0 * dl + dx[n - 2]) * dx[n - 3] * sl[n - 2]) / dl;
    for (int k = lane; k < m; k += 64) {
        const int i = k + 1;
        double a = dx[i], b = 2.0 * (dx[i - 1] + dx[i]), c = dx[i - 1];
        double r = 3.0 * (dx[i] * sl[i - 1] + dx[i - 1] * sl[i]);
        if (i == 1) {       // a_1 = dx_1 = row 0's diagonal: a_1 s_0 = r0 - d0 s_1
            b -= d0;
            a = 0.0;
            r -= r0;
        }
        if (i == n - 2) {   // c_{n-2} = dx_{n-3} = row n-1's diagonal: c s_{n-1} = rl - dl s_{n-2}
            b -= dl;
            c = 0.0;
            r -= rl;
        }
        const double inv = spl_rcp(b);
        A[k] = a * inv;
        C[k] = c * inv;
        R[k] = r * inv;
    }
    __syncthreads();
    for (int h = 1; h < m; h <<= 1) {
        double na[PCR_RPL], nc[PCR_RPL], nr[PCR_RPL];
#pragma unroll
        for (int j = 0; j < PCR_RPL; ++j) {
            if (64 * j >= m) break;    // wave-uniform
            const int k = lane + 64 * j;
            if (k < m) {
                const double ak = A[k], ck = C[k], rk = R[k];
                double al = 0.0, cl = 0.0, rlf = 0.0, ar = 0.0, cr = 0.0, rr = 0.0;
                if (k >= h) { al = A[k - h]; cl = C[k - h]; rlf = R[k - h]; }
                if (k + h < m) { ar = A[k + h]; cr = C[k + h]; rr = R[k + h]; }
                const double inv = spl_rcp(fma(-ck, ar, fma(-ak, cl, 1.0)));
                na[j] = -(ak * al) * inv;
                nc[j] = -(ck * cr) * inv;
                nr[j] = fma(-ck, rr, fma(-ak, rlf, rk)) * inv;
            }
        }
        __syncthreads();   // every row's neighbours read before any row is overwritten
#pragma unroll
        for (int j = 0; j < PCR_RPL; ++j) {
            if (64 * j >= m) break;
            const int k = lane + 64 * j;
            if (k < m) { A[k] = na[j]; C[k] = nc[j]; R[k] = nr[j]; }
        }
        __syncthreads();
    }
    double* S = A;         // knot slopes s_i (A is spent)
    for (int k = lane; k < m; k += 64) S[k + 1] = R[k];
    __syncthreads();
    if (lane == 0) {
        S[0] = (r0 - d0 * S[1]) / dx[1];
        S[n - 1] = (rl - dl * S[n - 2]) / dx[n - 3];
    }
    __syncthreads();
    // scipy's PPoly coefficients per interval (spline_not_a_knot's back-substitution formulas)
    for (int i = lane; i < n - 1; i += 64) {
        const double si = S[i], sn = S[i + 1];
        const double rdx = spl_rcp(xs[i + 1] - xs[i]);
        const double s_l = (ys[i + 1] - ys[i]) * rdx;
        const double tt = (si + sn - 2.0 * s_l) * rdx;
        OUT(i, 0, tt * rdx);
        OUT(i, 1, (s_l - si) * rdx - tt);
        OUT(i, 2, si);
        OUT(i, 3, ys[i]);
    }
    __syncthreads();
}

// ----------------------------------------------------------------------------------------
// One waveform's preparation state as its workgroup sees it, built once from (B, blockIdx.z):
// the waveform's inputs and switches (PrepDesc: t .. f_r, amp, ylm_*, m, n, freq, the scale,
// nt, K, lists, pcr, env), the batch's grid scalars, and the workspace's buffers by name and
// type. A stage takes the view and names the buffers it touches. The three kernels the TD sum's
// preparation shares (k_group_b, k_group_amp_b, k_prep_b) pass td = B.td: in a TD workspace
// only the header, the spline and the group buffers exist (make_layout's td) and every other
// pointer of the view is null. The kernels of the FD chain alone leave td at its constant.
// ----------------------------------------------------------------------------------------
struct PrepView : PrepDesc {
    int64_t nf, nl, nl1, stbcap;
    int32_t paired, td;
    Header* header;
    double *coefA, *coefT, *kslope, *tscratch, *invcp, *invdp, *gamp;
    int32_t *runs, *nseg, *slotcnt, *slottiles, *segbase, *stb0, *stb1;
    int32_t *gm, *gn, *gstart, *gmem;
    unsigned long long* gkeys;
    Item* items;
    int4 *ranges, *seginfo, *slotinfo;
    int2 *seglh, *slotlh;
    double2* sctab;
    int4* sitem;     // the split plan: items, and one arrival counter per split tile
    int32_t* scnt;
    __device__ __forceinline__ explicit PrepView(const PrepBatch& B, bool td_ws = false)
        : PrepDesc(B.d[blockIdx.z]), nf(B.nf), nl(B.nl), nl1(B.nl1), paired(B.paired),
          td(td_ws) {
        const Layout L = make_layout(nt, K, nf, paired, td_ws);
        stbcap = L.stbcap;
        at(header, L.header); at(coefA, L.coefA); at(coefT, L.coefT); at(kslope, L.kslope);
        at(tscratch, L.tscratch); at(gm, L.gm); at(gn, L.gn); at(gstart, L.gstart);
        at(gmem, L.gmem); at(gkeys, L.gkeys); at(gamp, L.gamp);
        fd(invcp, L.invcp); fd(invdp, L.invdp); fd(runs, L.runs); fd(items, L.items);
        fd(ranges, L.ranges); fd(seglh, L.seglh); fd(seginfo, L.seginfo); fd(nseg, L.nseg);
        fd(slotlh, L.slotlh); fd(slotinfo, L.slotinfo); fd(slotcnt, L.slotcnt);
        fd(slottiles, L.slottiles); fd(segbase, L.segbase); fd(stb0, L.stb0); fd(stb1, L.stb1);
        fd(sctab, L.sctab); fd(sitem, L.sitem); fd(scnt, L.scnt);
    }
    // lane limit of sub-branch sb's segments (paired grids: the non-positive half, see K4)
    // (from copies: a choice between members themselves becomes a variable offset into the view,
    // which then lives in scratch memory)
    __device__ __forceinline__ int seg_lim(int sb) const {
        const int64_t all = nf, lim0 = nl, lim1 = nl1;
        return (int)(paired ? (sb ? lim1 : lim0) : all);
    }

private:
    template <class T>
    __device__ __forceinline__ void at(T*& p, size_t off) { p = ws_at<T>(ws, off); }
    template <class T>   // a buffer of the FD workspace alone
    __device__ __forceinline__ void fd(T*& p, size_t off) {
        p = td ? nullptr : ws_at<T>(ws, off);
    }
};

// ----------------------------------------------------------------------------------------
// K0: (m, n) groups: gm[g], gn[g]; members gmem[gstart[g] .. gstart[g+1]); G = hdr->groups.
// Groups ascend in (m, n), members in harmonic index h (the order every later kernel and the
// oracle's grouping use; a function of (m, n) alone, so everything downstream is deterministic). One 256-thread workgroup with a small LDS footprint: it
// runs while the previous waveform's mode sum holds the GPU, so it must fit where one k_modesum
// workgroup has left a CU (round 1's 1024-thread, 68 KB-LDS bitonic sort needed two to leave the
// same CU at once and waited up to the end of that sum's dispatch, delaying the whole
// preparation chain). Counting sort over the (m, n) box the harmonics span when it has at most
// GB_CAP cells (FEW's l <= 10, |n| <= 30: 21 x 61); otherwise a bitonic sort of (m, n, h) keys
// in the global scratch gkeys. Both give the same groups and member order.
constexpr int GB_CAP = 2048;
__device__ __forceinline__ void header_init(Header* hdr) {
    const bool init = hdr->magic == HDR_MAGIC;
    hdr->contributions = 0;
    hdr->evaluations = 0;
    hdr->env_evaluations = 0;
    hdr->groups = 0;
    hdr->lane_lo = INT32_MAX;   // empty until k_segment_compact's blocks widen it
    hdr->lane_hi = INT32_MIN;
    hdr->nitems = -1;           // no split plan unless k_segments_one makes one
    hdr->nsplit = 0;
    if (!init) {
        hdr->runs_overflow = 0;
        hdr->bad_mn = 0;
        hdr->bad_tile = 0;
        hdr->magic = HDR_MAGIC;
    }
}
__device__ __forceinline__ void group_minmax(int& v_lo, int& v_hi, int* red, int slot) {
    for (int o = 32; o > 0; o >>= 1) {
        v_lo = min(v_lo, __shfl_xor(v_lo, o));
        v_hi = max(v_hi, __shfl_xor(v_hi, o));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave * 4 + slot] = v_lo; red[16 + wave * 4 + slot] = v_hi; }
}
// (The sort's arrays arrive as __restrict__ parameters, filled from the view by k_group_b:
// read from the view itself, whose members cannot be __restrict__, the one workgroup ran 2%
// longer, 23.4 instead of 22.9 us.)
__device__ __forceinline__ void group_body(const PrepView& V, const int32_t* __restrict__ marr,
                                           const int32_t* __restrict__ narr,
                                           int32_t* __restrict__ gm, int32_t* __restrict__ gn,
                                           int32_t* __restrict__ gstart,
                                           int32_t* __restrict__ gmem,
                                           unsigned long long* __restrict__ gkeys) {
    const int K = V.K;
    Header* hdr = V.header;
    constexpr int NTH = 256, NW = NTH / 64;
    __shared__ int bcnt[GB_CAP], boff[GB_CAP];
    __shared__ int red[32];
    __shared__ int wsum[2 * NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the call's counters start at zero (this is the preparation's first kernel; every later
    // writer runs after it in stream order): no separate hipMemsetAsync per waveform. The error
    // flags stay set until efd_modesum_status clears them (sticky; see Header)
    if (tid == 0) header_init(hdr);
    __syncthreads();
    // k_modesum's (sin, cos)(k pi/256) table, computed once per waveform here and copied into
    // each tile's LDS by LDS-DMA (cheaper than 512 sincospi per tile at small harmonic counts);
    // the TD sum has no use for it and its workspace no room
    if (!V.td)
        for (int i = tid; i < 512; i += NTH) {
            double sv, cv;
            sincospi((double)i / 256.0, &sv, &cv);
            V.sctab[i] = make_double2(sv, cv);
        }
    auto mval = [&](int i) { return min(max(marr[i], -256), 255); };
    auto nval = [&](int i) { return min(max(narr[i], -1024), 1023); };
    int mlo = INT32_MAX, mhi = INT32_MIN, nlo = INT32_MAX, nhi = INT32_MIN;
    for (int i = tid; i < K; i += NTH) {
        const int m = marr[i], n = narr[i];
        if (m < -256 || m > 255 || n < -1024 || n > 1023) atomicOr(&hdr->bad_mn, 1);
        mlo = min(mlo, mval(i)); mhi = max(mhi, mval(i));
        nlo = min(nlo, nval(i)); nhi = max(nhi, nval(i));
    }
    group_minmax(mlo, mhi, red, 0);
    group_minmax(nlo, nhi, red, 1);
    __syncthreads();
    mlo = red[0]; mhi = red[16]; nlo = red[1]; nhi = red[17];
    for (int w = 1; w < NW; ++w) {
        mlo = min(mlo, red[w * 4]); mhi = max(mhi, red[16 + w * 4]);
        nlo = min(nlo, red[w * 4 + 1]); nhi = max(nhi, red[16 + w * 4 + 1]);
    }
    const int nbn = nhi - nlo + 1;
    const int64_t nb = (int64_t)(mhi - mlo + 1) * nbn;
    if (nb <= GB_CAP) {
        // ---- counting sort over the (m, n) cells: counts, then one pass over the cells (per
        // thread a block of consecutive cells) writes the groups and the cells' offsets
        const int NB = (int)nb;
        auto cell = [&](int i) { return (mval(i) - mlo) * nbn + (nval(i) - nlo); };
        for (int b = tid; b < NB; b += NTH) bcnt[b] = 0;
        __syncthreads();
        for (int i = tid; i < K; i += NTH) atomicAdd(&bcnt[cell(i)], 1);
        __syncthreads();
        const int per = (NB + NTH - 1) / NTH;
        const int b0 = min(NB, tid * per), b1 = min(NB, b0 + per);
        int cm = 0, gmine = 0;
        for (int b = b0; b < b1; ++b) { cm += bcnt[b]; gmine += bcnt[b] > 0; }
        int ci = cm, gi = gmine;   // inclusive wave scans, then across waves
        for (int o = 1; o < 64; o <<= 1) {
            const int vc = __shfl_up(ci, o, 64), vg = __shfl_up(gi, o, 64);
            if (lane >= o) { ci += vc; gi += vg; }
        }
        if (lane == 63) { wsum[wave] = ci; wsum[NW + wave] = gi; }
        __syncthreads();
        int off = ci - cm, g = gi - gmine, G = 0;
        for (int w = 0; w < NW; ++w) {
            if (w < wave) { off += wsum[w]; g += wsum[NW + w]; }
            G += wsum[NW + w];
        }
        for (int b = b0; b < b1; ++b) {
            const int c = bcnt[b];
            boff[b] = off;
            if (c > 0) {
                gm[g] = mlo + b / nbn;
                gn[g] = nlo + b % nbn;
                gstart[g] = off;
                ++g;
            }
            off += c;
        }
        __syncthreads();
        // members into their cells (any order), then each cell sorted by h (l values of one
        // (m, n): a handful of members)
        for (int i = tid; i < K; i += NTH) gmem[atomicAdd(&boff[cell(i)], 1)] = i;
        __syncthreads();
        for (int b = b0; b < b1; ++b) {
            const int c = bcnt[b];
            if (c < 2) continue;
            int32_t* mem = gmem + (boff[b] - c);
            for (int x = 1; x < c; ++x) {
                const int32_t v = mem[x];
                int y = x - 1;
                while (y >= 0 && mem[y] > v) { mem[y + 1] = mem[y]; --y; }
                mem[y + 1] = v;
            }
        }
        if (tid == 0) {
            gstart[G] = K;
            hdr->groups = G;
        }
        return;
    }
    // ---- general (m, n) ranges: bitonic sort of ((m, n) << 32 | h) keys in global scratch
    int P = 1;
    while (P < K) P <<= 1;
    for (int i = tid; i < P; i += NTH) {
        unsigned long long k = ~0ull;
        if (i < K) {
            const unsigned gk = ((unsigned)(mval(i) + 256) << 11) | (unsigned)(nval(i) + 1024);
            k = ((unsigned long long)gk << 32) | (unsigned)i;
        }
        gkeys[i] = k;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += NTH) {
                const int lo = 2 * t - (t & (stride - 1));   // index with bit `stride` clear
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = gkeys[lo], b = gkeys[hi];
                if ((a > b) == up) { gkeys[lo] = b; gkeys[hi] = a; }
            }
            __syncthreads();
        }
    }
    // group starts: position p starts a group if its (m, n) differs from p - 1; exclusive scan
    // of the start flags over per-thread blocks of consecutive positions
    const int per = (K + NTH - 1) / NTH;
    const int p0 = min(K, tid * per), p1 = min(K, p0 + per);
    int mine = 0;
    for (int p = p0; p < p1; ++p) mine += (p == 0 || (gkeys[p] >> 32) != (gkeys[p - 1] >> 32));
    int G;
    int g = block_excl_scan<NW>(mine, wsum, lane, wave, G);
    for (int p = p0; p < p1; ++p) {
        const unsigned long long k = gkeys[p];
        gmem[p] = (int32_t)(unsigned)(k & 0xffffffffu);
        if (p == 0 || (k >> 32) != (gkeys[p - 1] >> 32)) {
            const unsigned gk = (unsigned)(k >> 32);
            gm[g] = (int32_t)(gk >> 11) - 256;
            gn[g] = (int32_t)(gk & 2047u) - 1024;
            gstart[g] = p;
            ++g;
        }
    }
    if (tid == 0) {
        gstart[G] = K;
        hdr->groups = G;
    }
}
__global__ __launch_bounds__(256) void k_group_b(const PrepBatch B) {
    const PrepView V(B, B.td != 0);
    group_body(V, V.m, V.n, V.gm, V.gn, V.gstart, V.gmem, V.gkeys);
}

// K0b: group amplitudes at the knots, one thread per (knot i, group g):
//   Bp = sum_l y0_l A_l(t_i),  Bm = sum_l y1_l A_l(t_i),  y0 = -scale Y+,  y1 = conj(-scale Y-)
// (y1 = 0 for m = 0: no partner), summed in ascending h. gamp is [nt][4K]: (Bp re, Bp im,
// Bm re, Bm im) of group g at 4g. S = -h_nb(-f) * scale: the minus sign and scale live here.
// group_amp_at is the one evaluation: k_group_amp_b stores it for k_prep_b's Thomas roles, and
// k_prep_pcr_b's amplitude waves call it for their own component (no gamp pass, one launch
// fewer in the chain; the same operations in the same order, so the same values).
template <class MEM>
__device__ __forceinline__ double4 group_amp_sum(const PrepView& V, bool partner, int p0, int p1,
                                                 MEM mem, int i) {
    const double *amp = V.amp, *ylm_p = V.ylm_p, *ylm_m = V.ylm_m;
    const double sc_re = V.sc_re, sc_im = V.sc_im;
    const int K = V.K;
    double bpr = 0.0, bpi = 0.0, bmr = 0.0, bmi = 0.0;
    for (int p = p0; p < p1; ++p) {
        const int h = mem(p);
        const double ar = amp[((size_t)i * K + h) * 2], ai = amp[((size_t)i * K + h) * 2 + 1];
        const double vr = ylm_p[2 * h], vi = ylm_p[2 * h + 1];
        const double y0r = -(sc_re * vr - sc_im * vi), y0i = -(sc_re * vi + sc_im * vr);
        bpr += ar * y0r - ai * y0i;
        bpi += ar * y0i + ai * y0r;
        if (partner) {
            const double ur = ylm_m[2 * h], ui = ylm_m[2 * h + 1];
            const double y1r = -(sc_re * ur - sc_im * ui), y1i = (sc_re * ui + sc_im * ur);
            bmr += ar * y1r - ai * y1i;
            bmi += ar * y1i + ai * y1r;
        }
    }
    return make_double4(bpr, bpi, bmr, bmi);
}
__device__ __forceinline__ double4 group_amp_at(const PrepView& V, int i, int g) {
    return group_amp_sum(V, V.gm[g] != 0, V.gstart[g], V.gstart[g + 1],
                         [&](int p) { return V.gmem[p]; }, i);
}
// the grids of k_items and k_group_amp at K >= ITEMS_SPLIT_K: K / ITEMS_PER_THREAD_K threads per
// interval or knot, a thread taking every (K / ITEMS_PER_THREAD_K)-th of the G <= K (m, n) groups
// (config 2's 3,020 harmonics form 627 groups: K-sized grids were ~80% workgroups that exit at
// once, and each held a slot of the sum beside which the next batch is prepared; 1 -> 8:
// +2.2% waveforms/s, r06v, within noise on a slower box, r06w)
#ifndef ITEMS_PER_THREAD_K
#define ITEMS_PER_THREAD_K 8
#endif
constexpr int ITEMS_SPLIT_K = 1024;
__global__ __launch_bounds__(256) void k_group_amp_b(const PrepBatch B) {
    const PrepView V(B, B.td != 0);
    if (V.pcr & 2) return;   // k_prep_pcr_b evaluates this waveform's group amplitudes itself
    // (the grid covers K / ITEMS_PER_THREAD_K groups at large K: a thread may take several)
    const int i = blockIdx.y;
    const int G = V.header->groups;
    if (i >= V.nt) return;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
        const double4 v = group_amp_at(V, i, g);
        double* o = V.gamp + (size_t)i * 4 * V.K + 4 * g;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
}

// ----------------------------------------------------------------------------------------
// K1: trajectory splines (one wave; lanes 0..3 the knot data, then lanes 4..5 the slopes)
// coefT layout: [interval][coef c][q], q: 0 Phi_phi, 1 Phi_r, 2 f_phi, 3 f_r, 4 f_phi', 5 f_r'
// ----------------------------------------------------------------------------------------
__device__ void traj_splines(const PrepView& V) {
    const int nt = V.nt;
    double *coefT = V.coefT, *kslope = V.kslope;
    // the serial Thomas chains read their knots from LDS instead of global memory
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* xs = lds;                 // t
    double* ys = lds + nt;            // 6 interpolants: Phi_phi, Phi_r, f_phi, f_r, f_phi', f_r'
    for (int i = threadIdx.x; i < nt; i += blockDim.x) {
        xs[i] = V.t[i];
        ys[i] = V.phi_phi[i];
        ys[nt + i] = V.phi_r[i];
        ys[2 * nt + i] = V.f_phi[i];
        ys[3 * nt + i] = V.f_r[i];
    }
    __syncthreads();
    const int q = threadIdx.x;
    double* cp = V.tscratch + (size_t)q * nt;
    double* dp = V.tscratch + (size_t)(8 + q) * nt;
    auto X = [&](int i) { return xs[i]; };
    auto CP = [&](int i) -> double& { return cp[i]; };
    auto DP = [&](int i) -> double& { return dp[i]; };
    if (q < 4) {
        const double* y = ys + (size_t)q * nt;
        auto Y = [&](int i) { return y[i]; };
        auto OUT = [&](int i, int c, double v) { coefT[((size_t)i * 4 + c) * 8 + q] = v; };
        spline_not_a_knot(nt, X, Y, CP, DP, OUT);
    }
    __syncthreads();
    // knot values of f_phi'(t) and f_r'(t), evaluated like scipy's derivative PPoly at the knots
    for (int idx = threadIdx.x; idx < 2 * nt; idx += blockDim.x) {
        const int qq = 2 + idx / nt, i = idx % nt;
        double v;
        if (i < nt - 1) {
            v = coefT[((size_t)i * 4 + 2) * 8 + qq];
        } else {
            double c[4];
            for (int cc = 0; cc < 4; ++cc) c[cc] = coefT[((size_t)(nt - 2) * 4 + cc) * 8 + qq];
            v = dcubic(c, xs[nt - 1] - xs[nt - 2]);
        }
        ys[(size_t)(4 + idx / nt) * nt + i] = v;
        kslope[idx] = v;
    }
    __syncthreads();
    if (q >= 4 && q < 6) {
        const double* y = ys + (size_t)q * nt;
        auto Y = [&](int i) { return y[i]; };
        auto OUT = [&](int i, int c, double v) { coefT[((size_t)i * 4 + c) * 8 + q] = v; };
        spline_not_a_knot(nt, X, Y, CP, DP, OUT);
    }
}

// ----------------------------------------------------------------------------------------
// K2: shared-knot splines, one lane per interpolant q < count; knot values YF(i, q); coef is
// [n-1][4][stride] (stride >= count). For the mode sum the interpolants are the four real parts
// of the group amplitudes (Bp re, Bp im, Bm re, Bm im of group q/4), summed over the group's
// harmonics as they are read (FEW's teuk_modes[N_t][K] complex layout underneath).
// ----------------------------------------------------------------------------------------
template <class YF>
__device__ void spline_shared(const double* __restrict__ x, int n, YF yf, int count, int stride,
                              double* coef, int64_t scratch_stride, int block) {
    const int ninterp = stride;
    // The not-a-knot matrix depends only on the shared knots: one thread factors it into LDS
    // (cp_i, 1/m_i, a_i of the Thomas sweep), then every lane runs the two division-free
    // recurrences for its right-hand side. DP(i) lives in the c1 slot of interval i of the
    // output (read back, one row ahead, by the back substitution before that row is written).
    // grids are sized for the harmonic count K before the device knows the group count: blocks
    // past the interpolants leave before the shared factorisation (a serial chain of ~n steps)
    if (block * (int)blockDim.x >= count) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* xs = lds;
    double* cpl = lds + n;
    double* iml = lds + 2 * n;
    double* all = lds + 3 * n;
    double* ridx = lds + 4 * n;   // 1 / (x_{i+1} - x_i): every lane's quotients by dx_i
    for (int i = threadIdx.x; i < n; i += blockDim.x) xs[i] = x[i];
    __syncthreads();
    for (int i = threadIdx.x; i < n - 1; i += blockDim.x) ridx[i] = spl_rcp(xs[i + 1] - xs[i]);
    if (threadIdx.x == 0 && n >= 4) {
        double dxm = xs[1] - xs[0], dxi = xs[2] - xs[1];
        double d = xs[2] - xs[0];
        cpl[0] = d / dxi; iml[0] = 1.0 / dxi; all[0] = 0.0;
        for (int i = 1; i <= n - 2; ++i) {
            dxm = xs[i] - xs[i - 1];
            dxi = xs[i + 1] - xs[i];
            const double mm = 2.0 * (dxm + dxi) - dxi * cpl[i - 1];
            const double rm = spl_rcp(mm);
            cpl[i] = dxm * rm; iml[i] = rm; all[i] = dxi;
        }
        const double dl = xs[n - 1] - xs[n - 3];
        const double mm = (xs[n - 2] - xs[n - 3]) - dl * cpl[n - 2];
        iml[n - 1] = 1.0 / mm; all[n - 1] = dl; cpl[n - 1] = 0.0;
    }
    __syncthreads();
    const int q = block * blockDim.x + threadIdx.x;
    if (q >= count) return;
    auto Y = [&](int i) { return yf(i, q); };
    auto OUT = [&](int i, int c, double v) { coef[((size_t)i * 4 + c) * ninterp + q] = v; };
    if (n < 4) {
        double* cpbuf = coef;
        double* dpbuf = coef + ninterp;
        auto X = [&](int i) { return xs[i]; };
        auto CP = [&](int i) -> double& { return cpbuf[(size_t)i * scratch_stride + q]; };
        auto DP = [&](int i) -> double& { return dpbuf[(size_t)i * scratch_stride + q]; };
        spline_not_a_knot(n, X, Y, CP, DP, OUT);
        return;
    }
    double* dpbase = coef + ninterp;   // DP(i) at coef[(i*4+1)*ninterp + q]
    auto DPs = [&](int i) -> double& { return dpbase[(size_t)i * scratch_stride + q]; };
    // Global loads (y, and DP on the way back) are issued PF rows at a time, ahead of the
    // serial recurrence, so each block of rows waits for memory once.
    constexpr int PF = SPLINE_PF;
    // forward sweep: dp_i = (r_i - a_i dp_{i-1}) / m_i, r_i from sl_{i-1}, sl_i
    const double y0 = Y(0), y1 = Y(1);
    double yprev = Y(2);
    double dxm = xs[1] - xs[0], dxi = xs[2] - xs[1];
    double slm = (y1 - y0) * ridx[0], sli = (yprev - y1) * ridx[1];
    double dp;
    {
        const double d = xs[2] - xs[0];
        const double r0 = ((dxm + 2.0 * d) * dxi * slm + dxm * dxm * sli) / d;
        dp = r0 * iml[0];
        DPs(0) = dp;
    }
    for (int i0 = 1; i0 <= n - 2; i0 += PF) {
        double yb[PF];   // y_{i+2} for rows i0 .. i0+PF-1
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int j = i0 + k + 2;
            yb[k] = j <= n - 1 ? Y(j) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int i = i0 + k;
            if (i > n - 2) break;
            const double r = 3.0 * (dxi * slm + dxm * sli);
            dp = (r - all[i] * dp) * iml[i];
            DPs(i) = dp;
            if (i + 2 <= n - 1) {
                dxm = dxi; slm = sli;
                dxi = xs[i + 2] - xs[i + 1];
                sli = (yb[k] - yprev) * ridx[i + 1];
                yprev = yb[k];
            }
        }
    }
    double s_next;
    {
        const double d = dxm + dxi;
        const double r = (dxi * dxi * slm + (2.0 * d + dxi) * dxm * sli) / d;
        s_next = (r - all[n - 1] * dp) * iml[n - 1];
    }
    // back substitution
    double yr = Y(n - 1);
    for (int i0 = n - 2; i0 >= 0; i0 -= PF) {
        double dpb[PF], ylb[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int i = i0 - k;
            dpb[k] = i >= 0 ? DPs(i) : 0.0;
            ylb[k] = i >= 0 ? Y(i) : 0.0;
        }
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int i = i0 - k;
            if (i < 0) break;
            const double yl = ylb[k];
            const double s_i = dpb[k] - cpl[i] * s_next;
            const double rdx = ridx[i];
            const double sl = (yr - yl) * rdx;
            const double tt = (s_i + s_next - 2.0 * sl) * rdx;
            OUT(i, 0, tt * rdx);
            OUT(i, 1, (sl - s_i) * rdx - tt);
            OUT(i, 2, s_i);
            OUT(i, 3, yl);
            s_next = s_i;
            yr = yl;
        }
    }
}

// ----------------------------------------------------------------------------------------
// K3: inverse splines t(F) per monotonic run, one lane per (m, n) group h
// runs[h][r] = (ja, jb, sign, 0): forward intervals [ja, jb), F increasing (+1)/decreasing (-1)
// Item.gx / Item.ic are filled for the intervals of each run.
// ----------------------------------------------------------------------------------------
__device__ __forceinline__ double knotF(const double* f_phi, const double* f_r, int m, int n,
                                        int i) {
    // The abscissae of the inverse splines and the run signs. NOT numpy's rounding: the _rn
    // builtins are the plain operators in HIP's headers, so the compiler contracts this into one
    // rounded product and an FMA, an ulp off numpy's m * f_phi + n * f_r at some knots. That is
    // harmless for t(F) (and kept as it is: another rounding here moves every spectrum's last
    // digits), but not for a comparison with a grid value: k_items takes its bounds from knotF_rn.
    return __dadd_rn(__dmul_rn((double)m, f_phi[i]), __dmul_rn((double)n, f_r[i]));
}
// numpy's m * f_phi + n * f_r bit for bit (product, product, sum, each rounded once: no FMA
// contraction), as the oracle's supports and the host twin's knotF have it. The lane bounds
// compare it with the grid: a bin that equals a knot frequency belongs to [F_j, F_{j+1}) of one
// record, or to none at a run's open end, only if both sides hold the same double. With the
// contracted value a run's end knot could move an ulp past such a bin, which then gained or lost
// a whole term.
__device__ __forceinline__ double knotF_rn(const double* f_phi, const double* f_r, int m, int n,
                                           int i) {
#pragma clang fp contract(off)
    const double a = (double)m * f_phi[i];
    const double b = (double)n * f_r[i];
    return a + b;
}

__device__ void inverse_splines(const PrepView& V, int block) {
    const int nt = V.nt, K = V.K, G = V.header->groups;
    if (block * (int)blockDim.x >= G) return;   // grid sized for K >= G
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* ts = lds;              // t, f_phi, f_r staged in LDS for the serial chains
    double* fps = lds + nt;
    double* frs = lds + 2 * nt;
    for (int i = threadIdx.x; i < nt; i += blockDim.x) {
        ts[i] = V.t[i];
        fps[i] = V.f_phi[i];
        frs[i] = V.f_r[i];
    }
    __syncthreads();
    const int h = block * blockDim.x + threadIdx.x;   // (m, n) group
    if (h >= G) return;
    const int m = V.gm[h], n = V.gn[h];
    const int ni = nt - 1;
    Item* it = V.items + (size_t)h * ni;
    int32_t* rr = V.runs + (size_t)h * 4 * MAXRUNS;
    double *cpbuf = V.invcp, *dpbuf = V.invdp;
    for (int r = 0; r < MAXRUNS; ++r) { rr[4 * r] = 0; rr[4 * r + 1] = 0; rr[4 * r + 2] = 0; }
    int nrun = 0;
    int j = 0;
    double Fprev = knotF(fps, frs, m, n, 0);
    // scan the interval signs and emit maximal strictly monotonic runs
    int cur_sign = 0, ja = 0;
    for (j = 0; j <= ni; ++j) {
        int sg = 0;
        double Fn = 0.0;
        if (j < ni) {
            Fn = knotF(fps, frs, m, n, j + 1);
            sg = (Fn > Fprev) ? 1 : ((Fn < Fprev) ? -1 : 0);
        }
        if (sg != cur_sign || j == ni) {
            if (cur_sign != 0) {  // close run [ja, j)
                if (nrun < MAXRUNS) {
                    rr[4 * nrun] = ja; rr[4 * nrun + 1] = j; rr[4 * nrun + 2] = cur_sign;
                    ++nrun;
                } else {
                    atomicOr(&V.header->runs_overflow, 1);
                }
            }
            cur_sign = sg;
            ja = j;
        }
        Fprev = Fn;
    }
    // inverse spline per run: x = F ascending, y = t
    for (int r = 0; r < nrun; ++r) {
        const int a = rr[4 * r], b = rr[4 * r + 1], sg = rr[4 * r + 2];
        const int npts = b - a + 1;
        // ascending index q -> knot index
        auto KI = [&](int qq) { return sg > 0 ? a + qq : b - qq; };
        auto X = [&](int qq) { return knotF(fps, frs, m, n, KI(qq)); };
        auto Y = [&](int qq) { return ts[KI(qq)]; };
        auto CP = [&](int qq) -> double& { return cpbuf[(size_t)(a + qq) * K + h]; };
        auto DP = [&](int qq) -> double& { return dpbuf[(size_t)(a + qq) * K + h]; };
        // ascending interval qq covers knots KI(qq), KI(qq+1) -> forward interval
        auto OUT = [&](int qq, int c, double v) {
            const int jf = sg > 0 ? a + qq : b - 1 - qq;
            it[jf].ic[c] = v;
            if (c == 3) it[jf].gx = X(qq);
        };
        spline_not_a_knot(npts, X, Y, CP, DP, OUT);
    }
}

// K1-K3 fused into one launch: the three spline stages are independent, latency-bound serial
// chains on few workgroups, so running them side by side costs max() instead of sum().
// Block 0: trajectory splines; blocks [1, 1 + nb_amp): amplitude splines (64 interpolants per
// block); the rest: inverse splines (64 harmonics per block).
// The grid is sized for the batch's largest K: blocks past this waveform's roles leave at once.
// (The TD sum's preparation launches 1 + nb_amp blocks: it has no use for inverse splines.)
__global__ __launch_bounds__(64) void k_prep_b(const PrepBatch B) {
    const PrepView V(B, B.td != 0);
    const int b = blockIdx.x, K = V.K;
    const int nb_amp = (4 * K + 63) / 64, nb_inv = (K + 63) / 64;
    if (b >= 1 + nb_amp + nb_inv) return;
    // k_prep_pcr_b has the trajectory and inverse roles (and maybe this one)
    if ((V.pcr & 1) && (b == 0 || b >= 1 + nb_amp || (V.pcr & 2))) return;
    if (b == 0) {
        traj_splines(V);
    } else if (b < 1 + nb_amp) {
        const int G = V.header->groups;
        const double* gamp = V.gamp;
        auto yf = [&](int i, int q) { return gamp[(size_t)i * 4 * K + q]; };
        spline_shared(V.t, V.nt, yf, 4 * G, 4 * K, V.coefA, (int64_t)4 * 4 * K, b - 1);
    } else {
        inverse_splines(V, b - 1 - nb_amp);
    }
}

// The block's (m, n) group when k_prep_pcr_b groups the harmonics itself (PrepBatch::pcr_groups,
// k_group_b not launched): G, the group's (m, n) and its members in ascending h (LDS)
struct LocalGroups {
    bool on;
    int G, m, n, count;
    const int* mem;
};
// PrepBatch::pcr_groups (every waveform of the batch on the PCR roles with K <= 64): each block
// groups the K harmonics itself, one per lane: a harmonic's group is the rank of its (m, n) among
// the distinct pairs, its place in gmem the count of harmonics of smaller (m, n) plus the members
// of its own before it. The same groups, order and member lists as k_group_b's counting sort (the
// same clamping and bad_mn rule). Block 0 also writes them (gm, gn, gstart, gmem, G), initialises
// the header and fills the sin/cos table: k_group_b's work, without its launch.
constexpr int PCR_GROUPS_MAX_K = 64;
__device__ __forceinline__ LocalGroups pcr_local_groups(const PrepView& V, int* s_mem) {
    const int lane = threadIdx.x, K = V.K, b = blockIdx.x;
    int m = 0, n = 0, key = INT32_MAX;
    bool bad = false;
    if (lane < K) {
        const int mr = V.m[lane], nr = V.n[lane];
        bad = mr < -256 || mr > 255 || nr < -1024 || nr > 1023;
        m = min(max(mr, -256), 255);
        n = min(max(nr, -1024), 1023);
        key = ((m + 256) << 11) | (n + 1024);
    }
    int less = 0, eqb = 0;   // harmonics of smaller (m, n); of the same (m, n) before this one
    for (int j = 0; j < K; ++j) {
        const int kj = __shfl(key, j, 64);
        less += kj < key;
        eqb += (kj == key) & (j < lane);
    }
    const bool first = lane < K && eqb == 0;
    int rank = 0;   // distinct (m, n) below this one: the group index
    for (int j = 0; j < K; ++j) {
        const int kj = __shfl(key, j, 64);
        const int fj = __shfl(first ? 1 : 0, j, 64);
        rank += fj & (kj < key);
    }
    LocalGroups lg{};
    lg.on = true;
    lg.G = __popcll(__ballot(first));
    lg.mem = s_mem;
    if (b == 0) {
        Header* hdr = V.header;
        if (first) {
            V.gm[rank] = m;
            V.gn[rank] = n;
            V.gstart[rank] = less;
        }
        if (lane < K) V.gmem[less + eqb] = lane;
        const bool anybad = __ballot(bad) != 0ull;
        if (lane == 0) {
            header_init(hdr);
            V.gstart[lg.G] = K;
            hdr->groups = lg.G;
            if (anybad) hdr->bad_mn = 1;
        }
        for (int i = lane; i < 512; i += 64) {
            double sv, cv;
            sincospi((double)i / 256.0, &sv, &cv);
            V.sctab[i] = make_double2(sv, cv);
        }
    }
    const int g = b < 4 ? -1 : b < 4 + K ? b - 4 : (b - 4 - K) >> 2;
    if (g >= 0 && g < lg.G) {
        const unsigned long long sel = __ballot(first && rank == g);
        const int src = __ffsll((long long)sel) - 1;
        lg.m = __shfl(m, src, 64);
        lg.n = __shfl(n, src, 64);
        const int kg = __shfl(key, src, 64);
        const bool mine = lane < K && key == kg;
        if (mine) s_mem[eqb] = lane;
        lg.count = __popcll(__ballot(mine));
    }
    __syncthreads();
    return lg;
}

// K1-K3 with one wave per interpolant (parallel cyclic reduction): blocks [0, 4) the trajectory splines (Phi_phi,
// Phi_r, f_phi, f_r; the f_phi and f_r blocks go on to f_phi', f_r' from their own knot
// slopes), [4, 4 + K) the inverse splines of group h = b - 4 < G, [4 + K, 4 + 5K) the group
// amplitude splines (interpolant q = b - 4 - K < 4G; only when PrepDesc::pcr bit 1 is set, else
// the grid stops at 4 + K). Blocks past this waveform's G leave at once.
// The same coefficients as k_prep_b's (scipy's construction, to rounding); for 4 <= N_t <=
// PCR_NMAX (the host takes k_prep_b otherwise). Dynamic LDS: 9 N_t doubles.
__global__ __launch_bounds__(64) void k_prep_pcr_b(const PrepBatch B) {
    const PrepView V(B);
    const int nt = V.nt, K = V.K;
    if (!(V.pcr & 1) || (int)blockIdx.x >= 4 + ((V.pcr & 2) ? 5 : 1) * K) return;
    __shared__ int s_mem[PCR_GROUPS_MAX_K];
    LocalGroups lg{};
    if (B.pcr_groups && (blockIdx.x == 0 || blockIdx.x >= 4))   // (blocks 1-3: trajectory only)
        lg = pcr_local_groups(V, s_mem);
    const double *t = V.t, *phi_phi = V.phi_phi, *phi_r = V.phi_r, *f_phi = V.f_phi, *f_r = V.f_r;
    const int32_t *gm = V.gm, *gn = V.gn;
    double *coefT = V.coefT, *kslope = V.kslope, *coefA = V.coefA;
    double *invcp = V.invcp, *invdp = V.invdp;
    int32_t* runs = V.runs;
    Item* items = V.items;
    Header* hdr = V.header;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    auto X = [&](int i) { return t[i]; };
    if (b < 4) {
        // trajectory spline q; q = 2, 3 continue with the derivative splines 4, 5
        const double* y = b == 0 ? phi_phi : b == 1 ? phi_r : b == 2 ? f_phi : f_r;
        int q = b;
        auto Y = [&](int i) { return y[i]; };
        auto OUT = [&](int i, int c, double v) { coefT[((size_t)i * 4 + c) * 8 + q] = v; };
        pcr_not_a_knot(nt, X, Y, OUT, lds);
        if (b < 2) return;
        // knot values of the derivative, as k_prep takes them: c2 of each interval, and scipy's
        // derivative of the last piece at the last knot (the slopes stay in LDS at [4 nt, 5 nt))
        double* v = lds + 7 * nt;
        const double* xs = lds;
        const double* ys = lds + nt;
        const double* S = lds + 4 * nt;
        for (int i = lane; i < nt; i += 64) {
            double vi;
            if (i < nt - 1) {
                vi = S[i];
            } else {
                const double si = S[nt - 2], sn = S[nt - 1];
                const double rdx = spl_rcp(xs[nt - 1] - xs[nt - 2]);
                const double s_l = (ys[nt - 1] - ys[nt - 2]) * rdx;
                const double tt = (si + sn - 2.0 * s_l) * rdx;
                const double c[4] = {tt * rdx, (s_l - si) * rdx - tt, si, ys[nt - 2]};
                vi = dcubic(c, xs[nt - 1] - xs[nt - 2]);
            }
            v[i] = vi;
            kslope[(size_t)(b - 2) * nt + i] = vi;
        }
        __syncthreads();
        q = b + 2;
        auto YV = [&](int i) { return v[i]; };
        pcr_not_a_knot(nt, X, YV, OUT, lds);
        return;
    }
    const int G = lg.on ? lg.G : hdr->groups;
    if (b >= 4 + K) {
        const int q = b - 4 - K;
        if (q >= 4 * G) return;
        const size_t ninterp = (size_t)4 * K;
        // component q & 3 of group q >> 2 at knot i (group_amp_at; no gamp pass)
        auto Y = [&](int i) {
            const double4 v =
                lg.on ? group_amp_sum(V, lg.m != 0, 0, lg.count,
                                      [&](int p) { return lg.mem[p]; }, i)
                      : group_amp_at(V, i, q >> 2);
            const int c = q & 3;
            return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w;
        };
        auto OUT = [&](int i, int c, double v) { coefA[((size_t)i * 4 + c) * ninterp + q] = v; };
        pcr_not_a_knot(nt, X, Y, OUT, lds);
        return;
    }
    const int h = b - 4;   // (m, n) group
    if (h >= G) return;
    const int m = lg.on ? lg.m : gm[h], n = lg.on ? lg.n : gn[h];
    const int ni = nt - 1;
    Item* it = items + (size_t)h * ni;
    int32_t* rr = runs + (size_t)h * 4 * MAXRUNS;
    double* Fv = lds + 8 * nt;     // F at the knots (PCR uses [0, 7 npts))
    int* sgv = reinterpret_cast<int*>(lds + 7 * nt);   // sign of F_{j+1} - F_j
    for (int i = lane; i < nt; i += 64) Fv[i] = knotF(f_phi, f_r, m, n, i);
    __shared__ int rrs[4 * MAXRUNS];
    __shared__ int nrun_s;
    __syncthreads();
    for (int j = lane; j < ni; j += 64) {
        const double F0 = Fv[j], F1 = Fv[j + 1];
        sgv[j] = (F1 > F0) ? 1 : ((F1 < F0) ? -1 : 0);
    }
    __syncthreads();
    {
        // maximal strictly monotonic runs, as inverse_splines scans them: a run of sign s != 0
        // starts at j where sgv[j] = s differs from sgv[j - 1] (or j = 0) and ends at the next
        // index whose sign differs (or ni, sign 0); the k-th start and the k-th end are run k's.
        // The wave finds them 64 indices at a time with ballots (lane 0 walking every index
        // serially was a chain of ni dependent LDS reads).
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        int nst = 0, nen = 0;   // starts / ends in the earlier chunks
        for (int c = 0; c <= ni; c += 64) {
            const int j = c + lane;
            const int sj = j < ni ? sgv[j] : 0;
            const int sp = (j >= 1 && j <= ni) ? sgv[j - 1] : 0;
            const bool st = j < ni && sj != 0 && (j == 0 || sp != sj);
            const bool en = j >= 1 && j <= ni && sp != 0 && sj != sp;
            const unsigned long long bs = __ballot(st), be = __ballot(en);
            if (st) {
                const int r = nst + __popcll(bs & below);
                if (r < MAXRUNS) {
                    rr[4 * r] = rrs[4 * r] = j;
                    rr[4 * r + 2] = rrs[4 * r + 2] = sj;
                }
            }
            if (en) {
                const int r = nen + __popcll(be & below);
                if (r < MAXRUNS) rr[4 * r + 1] = rrs[4 * r + 1] = j;
            }
            nst += __popcll(bs);
            nen += __popcll(be);
        }
        const int nrun = min(nst, MAXRUNS);
        // the unused run slots zeroed (none of them written above)
        if (lane < 4 * MAXRUNS && (lane >> 2) >= nrun && (lane & 3) < 3) {
            rr[lane] = 0;
            rrs[lane] = 0;
        }
        if (lane == 0) {
            // the run-overflow marker (not the header itself: with pcr_groups its
            // initialisation runs in this same launch, block 0, unordered with this block),
            // raised into the header by k_items
            rr[3] = nst > MAXRUNS ? 1 : 0;
            nrun_s = nrun;
        }
    }
    __syncthreads();
    const int nrun = nrun_s;
    for (int r = 0; r < nrun; ++r) {
        const int a = rrs[4 * r], bb = rrs[4 * r + 1], sg = rrs[4 * r + 2];
        const int npts = bb - a + 1;
        auto KI = [&](int qq) { return sg > 0 ? a + qq : bb - qq; };
        auto XF = [&](int qq) { return Fv[KI(qq)]; };
        auto YT = [&](int qq) { return t[KI(qq)]; };
        auto OUT = [&](int qq, int c, double v) {
            const int jf = sg > 0 ? a + qq : bb - 1 - qq;
            it[jf].ic[c] = v;
            if (c == 3) it[jf].gx = XF(qq);
        };
        if (npts >= 4) {
            pcr_not_a_knot(npts, XF, YT, OUT, lds);
        } else {
            if (lane == 0) {   // 2 or 3 knots: the closed forms (no scratch)
                auto CP = [&](int qq) -> double& { return invcp[(size_t)(a + qq) * K + h]; };
                auto DP = [&](int qq) -> double& { return invdp[(size_t)(a + qq) * K + h]; };
                spline_not_a_knot(npts, XF, YT, CP, DP, OUT);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(64) void k_spline_shared(const double* __restrict__ x, int n,
                                                      const double* __restrict__ y, int ninterp,
                                                      double* coef, int64_t scratch_stride) {
    auto yf = [&](int i, int q) { return y[(size_t)i * ninterp + q]; };
    spline_shared(x, n, yf, ninterp, ninterp, coef, scratch_stride, blockIdx.x);
}

// ----------------------------------------------------------------------------------------
// K4: interval records. Lane ranges per sub-branch s over the "lane" index k of the output:
//   s = 0: g = -freq[k];  s = 1: g = +freq[k].
// The inverse interval (ascending) covers g in [x_lo, x_hi), open at the run's first knot
// (notebook supports are open: :569-570; scipy picks the interval x_r <= g < x_{r+1}).
// Paired (symmetric) grids restrict lanes to the non-positive half: s = 0 to [0, nl),
// s = 1 to [0, nl1) (nl1 excludes the f = 0 bin so it is counted once).
// ----------------------------------------------------------------------------------------
// First index with f[i] >= v (UPPER = false) or f[i] > v (UPPER = true) on the sorted grid.
// Starts from the linear-interpolation guess g (exact to +-1 bin on the uniform FEW grids) and
// gallops outward before bisecting, so a typical call reads 2-3 grid values instead of the
// ~23 dependent loads of a plain binary search over 6.3M bins.
template <bool UPPER>
__device__ int64_t grid_bound(const double* __restrict__ f, int64_t nf, double v, int64_t g) {
    auto pred = [&](int64_t i) { return UPPER ? (f[i] > v) : (f[i] >= v); };
    g = g < 0 ? 0 : (g > nf ? nf : g);
    int64_t lo, hi;   // answer in [lo, hi]
    if (g < nf && !pred(g)) {
        lo = g + 1;
        int64_t step = 1;
        while (true) {
            const int64_t p = lo + step - 1;
            if (p >= nf) { hi = nf; break; }
            if (pred(p)) { hi = p; break; }
            lo = p + 1;
            step <<= 1;
        }
    } else {
        hi = g;
        int64_t step = 1;
        while (true) {
            const int64_t p = hi - step;
            if (p < 0) { lo = 0; break; }
            if (pred(p)) { hi = p; step <<= 1; }
            else { lo = p + 1; break; }
        }
    }
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One interval record of group h; `evals` = its (branch x bin) evaluation count.
// Certified records: a record whose every lane is known to pass the fast path's per-lane validity
// tests -- t(g) inside the record's knot interval and F' of the record's sign, nonzero -- skips
// them (Item::fdneg bit 1, header bit 25): one 64-bit compare and one class test per bin, with
// their ballots and mask arithmetic. Certified here on the device, with the kernel's own
// arithmetic: t(g) is monotonic over the record's g range (its derivative keeps one sign at the
// range's ends and at the derivative's vertex), w = t(g) - t_j at the range's end bins (bitwise
// the values k_modesum computes there) lies inside [0, dtj) with a 1e-6 dtj margin for the
// interior bins' rounding, and F' keeps the record's sign over the whole interval with a margin
// of 1e-12 of its terms. Fold and edge records (overshooting t(g), turning points) keep the
// tests; a safe record's lanes would all have passed them, so the spectrum is bitwise the same.
// FAT(x) = freq[x] (build_item serves the range ends from the grid values it already holds)
template <class FAT>
__device__ bool record_safe(const Item& it, FAT fat, int64_t lo0, int64_t hi0, int64_t lo1,
                            int64_t hi1) {
    // the g range of the lanes: s = 0 lanes k in [lo0, hi0) at g = -freq[k], s = 1 at +freq[k]
    double ga = INFINITY, gb = -INFINITY;
    if (hi0 > lo0) {
        const double fa = fat(0, lo0), fb = fat(1, hi0 - 1);
        ga = fmin(ga, fmin(-fa, -fb));
        gb = fmax(gb, fmax(-fa, -fb));
    }
    if (hi1 > lo1) {
        const double fa = fat(2, lo1), fb = fat(3, hi1 - 1);
        ga = fmin(ga, fmin(fa, fb));
        gb = fmax(gb, fmax(fa, fb));
    }
    if (!(ga <= gb)) return false;   // no lanes (or NaN)
    // the fast path's w at both ends (its exact operations)
    auto wat = [&](double g) {
        const double u = g - it.gx;
        const double tt = fma(fma(fma(it.ic[0], u, it.ic[1]), u, it.ic[2]), u, it.ic[3]);
        return tt - it.tj;
    };
    const double wa = wat(ga), wb = wat(gb);
    const double mg = 1e-6 * it.dtj;
    if (!(fmin(wa, wb) >= mg && fmax(wa, wb) <= it.dtj - mg)) return false;
    // monotonic t(u): t'(u) = 3 c0 u^2 + 2 c1 u + c2 of one sign at both ends and at its vertex
    const double ua = ga - it.gx, ub = gb - it.gx;
    auto dt = [&](double u) { return fma(fma(3.0 * it.ic[0], u, 2.0 * it.ic[1]), u, it.ic[2]); };
    const double da = dt(ua), db = dt(ub);
    if (!((da > 0.0 && db > 0.0) || (da < 0.0 && db < 0.0))) return false;
    if (it.ic[0] != 0.0) {
        const double uv = -it.ic[1] / (3.0 * it.ic[0]);
        if (uv > ua && uv < ub) {
            const double dv = dt(uv);
            if (!((dv > 0.0) == (da > 0.0) && dv != 0.0)) return false;
        }
    }
    // F'(w) = (fd0 w + fd1) w + fd2 of the record's sign on [0, dtj], away from 0
    const double* f = it.fd;
    const double scale = fabs(f[0]) * it.dtj * it.dtj + fabs(f[1]) * it.dtj + fabs(f[2]);
    const double sg = (it.fdneg & 1) ? -1.0 : 1.0;
    auto fq = [&](double x) { return sg * fma(fma(f[0], x, f[1]), x, f[2]); };
    double fmn = fmin(fq(0.0), fq(it.dtj));
    if (f[0] != 0.0) {
        const double xv = -f[1] / (2.0 * f[0]);
        if (xv > 0.0 && xv < it.dtj) fmn = fmin(fmn, fq(xv));
    }
    return fmn > 1e-12 * scale && isfinite(scale);
}

// (build_item and items_body keep their __restrict__ pointer lists: read through the view,
// whose members cannot be __restrict__, k_items took 332 us instead of 202 us on the headline's
// batch, with 117 VGPRs instead of 125)
__device__ bool build_item(
    const double* __restrict__ t, const double* __restrict__ f_phi, const double* __restrict__ f_r,
    const int32_t* __restrict__ gm, const int32_t* __restrict__ gn, int ni, int K,
    const double* __restrict__ coefA, const double* __restrict__ coefT,
    const int32_t* __restrict__ runs, const double* __restrict__ freq, int64_t nf, int paired,
    int64_t nl, int64_t nl1, Item* __restrict__ items, int4* __restrict__ ranges, int h, int j,
    unsigned long long& evals, bool env) {
    Item& it = items[(size_t)h * ni + j];
    const int m = gm[h], n = gn[h];
    const int32_t* rr = runs + (size_t)h * 4 * MAXRUNS;
    int run = -1;
    for (int r = 0; r < MAXRUNS; ++r) {
        if (rr[4 * r + 2] != 0 && j >= rr[4 * r] && j < rr[4 * r + 1]) { run = r; break; }
    }
    const int partner = (m != 0) ? 1 : 0;
    evals = 0;
    it.fdneg = 0;
    if (run < 0) {  // flat interval (F_{j+1} == F_j): no support; place empty ranges at 0
        it.klo[0] = it.khi[0] = it.klo[1] = it.khi[1] = 0;
        ranges[(size_t)h * ni + j] = make_int4(0, 0, 0, 0);
        return false;
    }
    const int a = rr[4 * run], sg = rr[4 * run + 2];
    it.tj = t[j];
    it.dtj = t[j + 1] - t[j];
    const double dm = (double)m, dn = (double)n;
    for (int c = 0; c < 4; ++c) {
        const double* ca = coefA + ((size_t)j * 4 + c) * 4 * K + 4 * h;
        it.b[0][0][c] = ca[0];   // Bp re
        it.b[0][1][c] = ca[1];   // Bp im
        it.b[1][0][c] = ca[2];   // Bm re
        it.b[1][1][c] = ca[3];   // Bm im
        const double* ct = coefT + ((size_t)j * 4 + c) * 8;
        it.ph[c] = dm * ct[0] + dn * ct[1];
    }
    // F' = derivative of (m f_phi + n f_r) piece; F'' = derivative of (m f_phi' + n f_r') piece
    double gq[3], ymin_rec;   // F'' quadratic (unscaled) and the |y| bound, for the envelope
    {
        const double* ct = coefT + (size_t)j * 32;
        const double F0 = dm * ct[0 * 8 + 2] + dn * ct[0 * 8 + 3];
        const double F1 = dm * ct[1 * 8 + 2] + dn * ct[1 * 8 + 3];
        const double F2 = dm * ct[2 * 8 + 2] + dn * ct[2 * 8 + 3];
        it.fd[0] = 3.0 * F0; it.fd[1] = 2.0 * F1; it.fd[2] = F2;
        const double G0 = dm * ct[0 * 8 + 4] + dn * ct[0 * 8 + 5];
        const double G1 = dm * ct[1 * 8 + 4] + dn * ct[1 * 8 + 5];
        const double G2 = dm * ct[2 * 8 + 4] + dn * ct[2 * 8 + 5];
        // pre-scaled so the fast path's w = 3 F''^2 / (2 pi |F'|^3) is one square
        it.fdd[0] = FDD_SCALE * (3.0 * G0);
        it.fdd[1] = FDD_SCALE * (2.0 * G1);
        it.fdd[2] = FDD_SCALE * G2;
        // lower bound of |y| = 2 pi |F'|^3 / (3 F''^2) over w in [0, dtj]: min |F'| and max |F''|
        // of the two quadratics from their end points and vertices (F' changing sign -> 0)
        const double dt = it.dtj;
        auto qv = [](double a, double b, double c, double x) { return (a * x + b) * x + c; };
        const double fa = it.fd[2], fb = qv(it.fd[0], it.fd[1], it.fd[2], dt);
        it.fdneg = qv(it.fd[0], it.fd[1], it.fd[2], 0.5 * dt) < 0.0 ? 1 : 0;
        double fdmin = fmin(fabs(fa), fabs(fb));
        if ((fa > 0.0) != (fb > 0.0) || fa == 0.0 || fb == 0.0) fdmin = 0.0;
        if (it.fd[0] != 0.0) {
            const double xv = -it.fd[1] / (2.0 * it.fd[0]);
            if (xv > 0.0 && xv < dt) {
                const double fv = qv(it.fd[0], it.fd[1], it.fd[2], xv);
                if ((fv > 0.0) != (fa > 0.0)) fdmin = 0.0;
                fdmin = fmin(fdmin, fabs(fv));
            }
        }
        double gmax = fmax(fabs(G2), fabs(qv(3.0 * G0, 2.0 * G1, G2, dt)));
        if (G0 != 0.0) {
            const double xv = -(2.0 * G1) / (6.0 * G0);
            if (xv > 0.0 && xv < dt) gmax = fmax(gmax, fabs(qv(3.0 * G0, 2.0 * G1, G2, xv)));
        }
        // 10% margin for the rounding of both bounds and of the kernel's own evaluation
        const double ymin = gmax > 0.0 ? TWO_PI * fdmin * fdmin * fdmin / (3.0 * gmax * gmax) / 1.1
                                       : INFINITY;
        int J = FAST_J;
        for (int jj = 1; jj < FAST_J; ++jj)
            if (ymin >= JSER_Y[jj]) { J = jj; break; }
        it.jser = J;
        gq[0] = 3.0 * G0; gq[1] = 2.0 * G1; gq[2] = G2;
        ymin_rec = ymin;
    }
    // g-interval of this record: [x_lo, x_hi), lower end open at the run's first knot
    const double Fj = knotF_rn(f_phi, f_r, m, n, j), Fj1 = knotF_rn(f_phi, f_r, m, n, j + 1);
    const double xlo = sg > 0 ? Fj : Fj1;
    const double xhi = sg > 0 ? Fj1 : Fj;
    const bool strict_lo = sg > 0 ? (j == a) : (j + 1 == rr[4 * run + 1]);
    // linear-interpolation guess of the grid index of a frequency value
    const double f0 = freq[0], span = freq[nf - 1] - f0;
    const double gsc = span > 0.0 ? (double)(nf - 1) / span : 0.0;
    auto guess = [&](double v) { return (int64_t)floor((v - f0) * gsc); };
    // s = 0: g = -f  ->  f in (-xhi, -xlo]  (or (-xhi, -xlo) if strict)
    // s = 1: g = +f  ->  f in [xlo, xhi)  (or (xlo, xhi))
    // The four bounds' grid values around their guesses are loaded together (one round trip
    // instead of the ~2 dependent ones of each grid_bound in turn); a bound the three values do
    // not settle (a non-uniform grid) takes grid_bound. Same indices either way.
    const double bv[4] = {-xhi, -xlo, xlo, xhi};
    const bool bu[4] = {true, !strict_lo, strict_lo, false};   // UPPER: first f > v, else f >= v
    int64_t bg[4];
    double b3[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t g = guess(bv[q]);
        bg[q] = g < 0 ? 0 : (g > nf ? nf : g);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t g = bg[q];
        b3[q][0] = freq[g >= 1 ? g - 1 : 0];
        b3[q][1] = freq[g < nf ? g : nf - 1];
        b3[q][2] = freq[g + 1 < nf ? g + 1 : nf - 1];
    }
    int64_t bk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double v = bv[q];
        const int64_t g = bg[q];
        auto pred = [&](double x) { return bu[q] ? (x > v) : (x >= v); };
        int64_t k = -1;
        if (!(g >= 1 && pred(b3[q][0]))) {           // f[g - 1] fails: the answer is >= g
            if (g == nf) k = nf;
            else if (pred(b3[q][1])) k = g;
            else if (g + 1 == nf) k = nf;
            else if (pred(b3[q][2])) k = g + 1;
        }
        if (k < 0)
            k = bu[q] ? grid_bound<true>(freq, nf, v, g) : grid_bound<false>(freq, nf, v, g);
        bk[q] = k;
    }
    int64_t lo0 = bk[0], hi0 = bk[1], lo1 = bk[2], hi1 = bk[3];
    const int64_t lim0 = paired ? nl : nf;
    const int64_t lim1 = paired ? nl1 : (partner ? nf : 0);
    auto clampr = [](int64_t& lo, int64_t& hi, int64_t lim) {
        if (lo > lim) lo = lim;
        if (hi > lim) hi = lim;
        if (hi < lo) hi = lo;
    };
    clampr(lo0, hi0, lim0);
    clampr(lo1, hi1, lim1);
    it.klo[0] = (int32_t)lo0; it.khi[0] = (int32_t)hi0;
    it.klo[1] = (int32_t)lo1; it.khi[1] = (int32_t)hi1;
    ranges[(size_t)h * ni + j] = make_int4((int)lo0, (int)hi0, (int)lo1, (int)hi1);
    // freq[x] for a range end x: from bound q's three grid values when x is one of them (the
    // usual case: an end is its bound's answer or the index before), else loaded
    auto fat = [&](int q, int64_t x) {
        const int64_t g = bg[q];
        if (g >= 1 && x == g - 1) return b3[q][0];
        if (g < nf && x == g) return b3[q][1];
        if (g + 1 < nf && x == g + 1) return b3[q][2];
        return freq[x];
    };
    if (record_safe(it, fat, lo0, hi0, lo1, hi1)) it.fdneg |= 2;
    // branch x bin evaluations (on a paired grid one lane serves both the branch and its partner)
    const int mult = paired ? 1 + partner : 1;
    evals = (unsigned long long)((hi0 - lo0) + (hi1 - lo1)) * mult;
    // envelope record (env_fit.inc): a certified-safe record with |y| >= ENV_MIN_Y everywhere
    // whose A(w) and theta(w) polynomials pass the check; its F' / F'' / dtj slots then hold
    // A's coefficients, its phase cubic Phi - theta, and jser = 0 marks it for the sum
    if (env && (it.fdneg & 2) && ymin_rec >= ENV_MIN_Y && evals > 0) {
        EnvFit E;
        if (env_fit(it.fd, gq, it.dtj, (it.fdneg & 1) != 0, E)) {
            // A's coefficients times the cosine polynomial's constant (sincos_tab_amp's cos r =
            // COS_A - r^2/2 then costs one FMA on the scaled amplitude)
            double* e = env_of(&it);
            for (int c = 0; c <= ENV_DEG; ++c) e[c] = E.a[c] * ENV_AMP_SCALE;
            for (int c = 0; c < 4; ++c) it.ph[c] -= E.th[c];
            it.jser = 0;   // the sum's envelope class
            return true;
        }
    }
    return false;
}

// K4: one thread per (group g, knot interval j). Counts both the SPA evaluations the kernel
// makes (per group) and the reference formulation's contributions C (per (l, m, n) harmonic:
// the group's evaluations times its member count).
__device__ __forceinline__ void items_body(const double* __restrict__ t, const double* __restrict__ f_phi,
                        const double* __restrict__ f_r, const int32_t* __restrict__ gm,
                        const int32_t* __restrict__ gn, const int32_t* __restrict__ gstart,
                        int nt, int K, const double* __restrict__ coefA,
                        const double* __restrict__ coefT, const int32_t* __restrict__ runs,
                        const double* __restrict__ freq, int64_t nf, int paired, int64_t nl,
                        int64_t nl1, Item* __restrict__ items, int4* __restrict__ ranges,
                        Header* __restrict__ hdr, bool runs_mark, bool env) {
    const int ni = nt - 1;
    const int G = hdr->groups;
    // the grid is sized for K >= G groups (K / ITEMS_PER_THREAD_K threads per interval at large
    // K): whole blocks past the records leave at once; a thread takes the records gid, gid +
    // the grid's threads, ... (config 2: 627 groups over 377 threads an interval, one or two)
    const int64_t total = (int64_t)ni * G;
    if ((int64_t)blockIdx.x * blockDim.x >= total) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    __shared__ unsigned long long red[3][4];
    unsigned long long ev = 0, contrib = 0, eev = 0;
    for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid < total;
         gid += stride) {
        const int g = (int)(gid % G), j = (int)(gid / G);
        // the PCR inverse splines' run-overflow marker (rr[3]) into the header's sticky flag
        if (runs_mark && j == 0 && runs[(size_t)g * 4 * MAXRUNS + 3] != 0)
            atomicOr(&hdr->runs_overflow, 1);
        unsigned long long e1 = 0;
        const bool envr = build_item(t, f_phi, f_r, gm, gn, ni, K, coefA, coefT, runs, freq, nf,
                                     paired, nl, nl1, items, ranges, g, j, e1, env);
        ev += e1;
        contrib += e1 * (unsigned long long)(gstart[g + 1] - gstart[g]);
        eev += envr ? e1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        ev += __shfl_xor(ev, o);
        contrib += __shfl_xor(contrib, o);
        eev += __shfl_xor(eev, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = contrib;
        red[1][threadIdx.x >> 6] = ev;
        red[2][threadIdx.x >> 6] = eev;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long c = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        const unsigned long long e = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        const unsigned long long x = red[2][0] + red[2][1] + red[2][2] + red[2][3];
        if (c) atomicAdd((unsigned long long*)&hdr->contributions, c);
        if (e) atomicAdd((unsigned long long*)&hdr->evaluations, e);
        if (x) atomicAdd((unsigned long long*)&hdr->env_evaluations, x);
    }
}
__global__ __launch_bounds__(256) void k_items(const PrepBatch B) {
    const PrepView V(B);
    items_body(V.t, V.f_phi, V.f_r, V.gm, V.gn, V.gstart, V.nt, V.K, V.coefA, V.coefT, V.runs,
               V.freq, V.nf, V.paired, V.nl, V.nl1, V.items, V.ranges, V.header,
               (V.pcr & 1) != 0, V.env != 0);
}

// ----------------------------------------------------------------------------------------
// K5: segment table. A segment is (group, monotonic run, sub-branch s) with a non-empty lane
// range; its interval records are consecutive (h * ni + j, j in [ja, jb)) and, walked in lane
// order (j += dir), cover consecutive, disjoint lane ranges. K5a: one thread per (h, run, s)
// slot writes the slot's segment (or an empty marker) into a dense table plus a per-block count;
// K5b compacts the non-empty slots in slot order (block offsets from the counts), so the table
// is deterministic.
// seglh = (lo, hi) lane range; seginfo = (first record, count, dir, s).
// ----------------------------------------------------------------------------------------
// The segment of slot i = (group h, run r, sub-branch sb): its lane range lh and (first record,
// count, dir, s) info, or info.y == 0 when the slot holds none. G = the call's group count;
// ranges: V.ranges, or k_segments_one's copy of it in LDS.
__device__ __forceinline__ void slot_segment(const PrepView& V, int i,
                                             const int4* __restrict__ ranges, int G, int2& lh,
                                             int4& info) {
    const int h = i / (2 * MAXRUNS), r = (i >> 1) % MAXRUNS, sb = i & 1;
    const int ni = V.nt - 1;
    lh = make_int2(0, 0);
    info = make_int4(0, 0, 0, 0);
    const int32_t* rr = V.runs + (size_t)h * 4 * MAXRUNS + 4 * r;
    if (h < G && rr[2] != 0) {
        const int ja = rr[0], jb = rr[1], n = jb - ja;
        const int dir = (sb == 0) ? -rr[2] : rr[2];   // s = 0 walks g downward in lane order
        const int lim = V.seg_lim(sb);
        const int4* rg = ranges + (size_t)h * ni;
        // Records whose branch lies outside the lane range are empty and clamped to its
        // ends (lane 0 or lim); they sit at the two ends of the segment in lane order and
        // are trimmed, so the tiles holding lane 0 and lim do not collect all of them.
        int lo = 0, hi = n;                            // first p with khi > 0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int4 v = rg[dir > 0 ? ja + mid : jb - 1 - mid];
            if ((sb ? v.w : v.y) > 0) hi = mid; else lo = mid + 1;
        }
        const int pa = lo;
        hi = n;                                        // first p with klo >= lim
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int4 v = rg[dir > 0 ? ja + mid : jb - 1 - mid];
            if ((sb ? v.z : v.x) >= lim) hi = mid; else lo = mid + 1;
        }
        const int pb = lo;
        if (pb > pa) {
            const int4 rf = rg[dir > 0 ? ja + pa : jb - 1 - pa];
            const int4 rl = rg[dir > 0 ? ja + pb - 1 : jb - pb];
            const int klo = sb ? rf.z : rf.x, khi = sb ? rl.w : rl.y;
            if (khi > klo) {
                lh = make_int2(klo, khi);
                const int jfirst = dir > 0 ? ja + pa : jb - pb;   // lowest record index kept
                info = make_int4(h * ni + jfirst, pb - pa, dir, sb);
            }
        }
    }
}
// slot blocks of one waveform: (2 MAXRUNS K + 255) / 256; the grid has the batch's largest count
__device__ __forceinline__ int slot_blocks(int K) { return (2 * MAXRUNS * K + 255) / 256; }
__global__ __launch_bounds__(256) void k_segment_slots(const PrepBatch B) {
    const PrepView V(B);
    if ((int)blockIdx.x >= slot_blocks(V.K)) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ int wc[4], wt[4];
    int ntl = 0;   // tiles the slot's segment covers
    bool valid = false;
    if (i < V.K * MAXRUNS * 2) {
        int2 lh;
        int4 info;
        slot_segment(V, i, V.ranges, V.header->groups, lh, info);
        V.slotlh[i] = lh;
        V.slotinfo[i] = info;
        valid = info.y > 0;
        if (valid) ntl = (lh.y - 1) / TILE_LANES - lh.x / TILE_LANES + 1;
    }
    const unsigned long long bal = __ballot(valid);
    int tsum = ntl;
    for (int o = 32; o > 0; o >>= 1) tsum += __shfl_xor(tsum, o);
    if ((threadIdx.x & 63) == 0) {
        wc[threadIdx.x >> 6] = __popcll(bal);
        wt[threadIdx.x >> 6] = tsum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        V.slotcnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
        V.slottiles[blockIdx.x] = wt[0] + wt[1] + wt[2] + wt[3];
    }
}

// one workgroup per slot block: its output offset is the sum of the earlier blocks' counts
__global__ __launch_bounds__(256) void k_segment_compact(const PrepBatch B) {
    const PrepView V(B);
    const int nblk = slot_blocks(V.K), nslot = 2 * MAXRUNS * V.K;
    if ((int)blockIdx.x >= nblk) return;
    Header* hdr = V.header;
    __shared__ int wc[4];
    __shared__ int64_t wt[4];
    __shared__ int2 wr[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x;
    int before = 0;
    int64_t tbefore = 0;
    for (int b = tid; b < blk; b += 256) { before += V.slotcnt[b]; tbefore += V.slottiles[b]; }
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o);
        tbefore += __shfl_xor(tbefore, o);
    }
    if (lane == 0) { wc[wave] = before; wt[wave] = tbefore; }
    __syncthreads();
    const int base = wc[0] + wc[1] + wc[2] + wc[3];
    const int64_t tbase = wt[0] + wt[1] + wt[2] + wt[3];
    __syncthreads();
    const int i = blk * 256 + tid;
    int4 info = make_int4(0, 0, 0, 0);
    int2 lh = make_int2(0, 0);
    if (i < nslot) { info = V.slotinfo[i]; lh = V.slotlh[i]; }
    const bool valid = info.y > 0;
    const int ntl = valid ? (lh.y - 1) / TILE_LANES - lh.x / TILE_LANES + 1 : 0;
    // exclusive scan of the tile counts over the block's slots (slot order). Not block_excl_scan:
    // 64-bit wave totals, and the barrier is shared with the ballot counts
    int incl = ntl;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const unsigned long long bal = __ballot(valid);
    if (lane == 63) wt[wave] = incl;
    if (lane == 0) wc[wave] = __popcll(bal);
    __syncthreads();
    int pos = base;
    int64_t toff = tbase + incl - ntl;
    for (int w = 0; w < wave; ++w) { pos += wc[w]; toff += wt[w]; }
    pos += __popcll(bal & ((1ull << lane) - 1ull));
    if (valid) {
        V.seglh[pos] = lh;
        V.seginfo[pos] = info;
        V.segbase[pos] = (toff + ntl <= V.stbcap) ? (int32_t)(toff - lh.x / TILE_LANES)
                                                  : SEG_NO_STB;
    }
    if (blk == nblk - 1 && tid == 0) *V.nseg = base + wc[0] + wc[1] + wc[2] + wc[3];
    // the union of the block's segment lane ranges into the header: k_modesum's tiles outside
    // it skip the list build (one block-wide min / max, two global atomics per block)
    int lo = valid ? lh.x : INT32_MAX, hi = valid ? lh.y : INT32_MIN;
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) wr[wave] = make_int2(lo, hi);
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) { lo = min(lo, wr[w].x); hi = max(hi, wr[w].y); }
        if (lo < hi) {
            atomicMin(&hdr->lane_lo, lo);
            atomicMax(&hdr->lane_hi, hi);
        }
    }
}

// One workgroup per segment (grid-stride): for every record p of the segment in lane order
// (and the end marker p = n), the tiles t of [t0, t1] whose first record reaching them is p
// (p0(t) = first p with khi > t*TL) and whose first record past them is p (p1(t) = first p with
// klo >= (t+1)*TL). Lane ranges are monotone in p, so each tile gets exactly one of each: the
// same answers as k_modesum's bisection, from two loads instead of ~2 log2(n) dependent ones.
__device__ __forceinline__ int div_floor_nn(int64_t a) { return (int)(a / TILE_LANES); }   // a >= 0
// record p (0 <= p <= n: n is the end marker) of the segment (lh, info) with pair base sbase
__device__ __forceinline__ void seg_tiles_record(const int4* __restrict__ ranges, int2 lh,
                                                 int4 info, int32_t sbase, int p,
                                                 int32_t* __restrict__ stb0,
                                                 int32_t* __restrict__ stb1) {
    const int base = info.x, n = info.y, dir = info.z, sb = info.w;
    const int t0 = lh.x / TILE_LANES, t1 = (lh.y - 1) / TILE_LANES;
    auto rng = [&](int q) {   // (klo, khi) of record q in lane order
        const int4 rg = ranges[base + (dir > 0 ? q : n - 1 - q)];
        return sb ? make_int2(rg.z, rg.w) : make_int2(rg.x, rg.y);
    };
    const int2 cur = p < n ? rng(p) : make_int2(0, 0);
    const int2 prv = p > 0 ? rng(p - 1) : make_int2(0, 0);
    // p0: khi_{p-1} <= t TL < khi_p
    int a = p > 0 ? (int)((prv.y + TILE_LANES - 1) / TILE_LANES) : t0;
    int b = p < n ? (cur.y > 0 ? div_floor_nn(cur.y - 1) : -1) : t1;
    for (int t = max(a, t0); t <= min(b, t1); ++t) stb0[sbase + t] = p;
    // p1: klo_{p-1} < (t+1) TL <= klo_p
    a = p > 0 ? div_floor_nn(prv.x) : t0;
    b = p < n ? div_floor_nn(cur.x) - 1 : t1;
    for (int t = max(a, t0); t <= min(b, t1); ++t) stb1[sbase + t] = p;
}
__global__ __launch_bounds__(256) void k_seg_tiles(const PrepBatch B) {
    const PrepView V(B);
    const int nseg = *V.nseg;
    for (int sg = blockIdx.x; sg < nseg; sg += gridDim.x) {
        const int32_t sbase = V.segbase[sg];
        if (sbase == SEG_NO_STB) continue;
        const int2 lh = V.seglh[sg];
        const int4 info = V.seginfo[sg];
        for (int p = threadIdx.x; p <= info.y; p += blockDim.x)
            seg_tiles_record(V.ranges, lh, info, sbase, p, V.stb0, V.stb1);
    }
}

// K5 in one workgroup per waveform when its 2 MAXRUNS K slots fit one (K <= 64: the walker
// batches' sparse spectra): the slots' segments, their compaction in slot order (block scans in
// place of k_segment_compact's per-block offsets), the lane union, then the tile pairs of every
// (segment, record) (k_seg_tiles' work flattened over the workgroup: a record's segment found by
// bisection of the segments' record offsets in LDS). The same tables as the three kernels, in
// one launch instead of three.
constexpr int64_t SEG1_LDS_CAP = 40 * 1024;   // bytes of staged ranges (+ 33 KB static LDS)
__global__ __launch_bounds__(SEG1_NT) void k_segments_one(const PrepBatch B) {
    const PrepView V(B);
    constexpr int NW = SEG1_NT / 64;
    __shared__ int wsum[NW];
    __shared__ int2 wr[NW];
    __shared__ int2 s_lh[SEG1_NT];
    __shared__ int4 s_info[SEG1_NT];
    __shared__ int32_t s_base[SEG1_NT];
    __shared__ int32_t s_roff[SEG1_NT];
    Header* hdr = V.header;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nslot = 2 * MAXRUNS * V.K;   // <= SEG1_NT (host: every waveform has K <= SEG1_MAX_K)
    // the interval records' lane ranges staged in LDS when they fit (one coalesced pass): the
    // slots' bisections and the tile pairs then read LDS instead of chains of global loads
    extern __shared__ int4 s_rg[];
    const int ni = V.nt - 1;
    const int4* ranges = V.ranges;
    if ((int64_t)V.K * ni * (int64_t)sizeof(int4) <= (int64_t)B.seg_lds) {
        const int nrec = hdr->groups * ni;
        for (int i = tid; i < nrec; i += SEG1_NT) s_rg[i] = ranges[i];
        __syncthreads();
        ranges = s_rg;
    }
    int2 lh = make_int2(0, 0);
    int4 info = make_int4(0, 0, 0, 0);
    if (tid < nslot)
        slot_segment(V, tid, ranges, hdr->groups, lh, info);
    const bool valid = info.y > 0;
    const int ntl = valid ? (lh.y - 1) / TILE_LANES - lh.x / TILE_LANES + 1 : 0;
    // (a barrier after each block scan frees wsum for the next)
    int nseg, ntot;
    const int pos = block_excl_scan<NW>(valid ? 1 : 0, wsum, lane, wave, nseg);
    __syncthreads();
    const int toff = block_excl_scan<NW>(ntl, wsum, lane, wave, ntot);
    __syncthreads();
    int32_t sbase = SEG_NO_STB;
    if (valid) {
        sbase = ((int64_t)toff + ntl <= V.stbcap) ? (int32_t)(toff - lh.x / TILE_LANES)
                                                  : SEG_NO_STB;
        V.seglh[pos] = lh;
        V.seginfo[pos] = info;
        V.segbase[pos] = sbase;
        s_lh[pos] = lh;
        s_info[pos] = info;
        s_base[pos] = sbase;
    }
    int nrec_all;
    const int nrec = (valid && sbase != SEG_NO_STB) ? info.y + 1 : 0;
    const int roff = block_excl_scan<NW>(nrec, wsum, lane, wave, nrec_all);
    __syncthreads();
    if (valid) s_roff[pos] = roff;
    // the lane union (k_segment_compact's, one workgroup: no atomics)
    int lo = valid ? lh.x : INT32_MAX, hi = valid ? lh.y : INT32_MIN;
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) wr[wave] = make_int2(lo, hi);
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) { lo = min(lo, wr[w].x); hi = max(hi, wr[w].y); }
        if (lo < hi) {
            hdr->lane_lo = lo;
            hdr->lane_hi = hi;
        }
        *V.nseg = nseg;
    }
    // the sparse sum's split plan (paired grids, i.e. the fused likelihood): every union tile's
    // cost in wave-records, from the same (segment, record) pairs. Possible when the union fits
    // SPLIT_UNION_CAP tiles and every segment has its tile pairs (else nitems stays -1)
    __shared__ int s_cost[SPLIT_UNION_CAP];
    __syncthreads();   // wr[] (the union) is complete
    int ulo = INT32_MAX, uhi = INT32_MIN;
    for (int w = 0; w < NW; ++w) { ulo = min(ulo, wr[w].x); uhi = max(uhi, wr[w].y); }
    const int ut0 = ulo < uhi ? ulo / TILE_LANES : 0;
    const int nut = ulo < uhi ? (uhi - 1) / TILE_LANES - ut0 + 1 : 0;
    const bool plan = B.paired && nut > 0 && nut <= SPLIT_UNION_CAP &&
                      !__syncthreads_or(valid && sbase == SEG_NO_STB);
    if (plan)
        for (int i = tid; i < nut; i += SEG1_NT) s_cost[i] = 0;
    __syncthreads();
    for (int f = tid; f < nrec_all; f += SEG1_NT) {
        int a = 0, b = nseg - 1;   // the last segment q with s_roff[q] <= f
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (s_roff[mid] <= f) a = mid; else b = mid - 1;
        }
        const int p = f - s_roff[a];
        seg_tiles_record(ranges, s_lh[a], s_info[a], s_base[a], p, V.stb0, V.stb1);
        if (plan && p < s_info[a].y) {
            // record p's cost per tile it reaches: the 64 BPL-lane wave chunks it touches there
            // (modesum_tile evaluates a record on every wave whose bins it reaches)
            const int4 in = s_info[a];
            const int4 rg = ranges[in.x + (in.z > 0 ? p : in.y - 1 - p)];
            const int klo = in.w ? rg.z : rg.x, khi = in.w ? rg.w : rg.y;
            if (khi > klo) {
                constexpr int WL = 64 * BPL;
                for (int t = klo / TILE_LANES; t <= (khi - 1) / TILE_LANES; ++t) {
                    const int a0 = max(klo, t * TILE_LANES), b0 = min(khi, (t + 1) * TILE_LANES);
                    atomicAdd(&s_cost[t - ut0], (b0 - 1) / WL - a0 / WL + 1);
                }
            }
        }
    }
    if (!plan) return;
    __syncthreads();
    // each thread takes SPLIT_UNION_CAP / SEG1_NT consecutive union tiles
    constexpr int PER = SPLIT_UNION_CAP / SEG1_NT;
    int64_t csum = 0;
    for (int i = 0; i < PER; ++i) {
        const int u = tid * PER + i;
        csum += u < nut ? s_cost[u] : 0;
    }
    for (int o = 32; o > 0; o >>= 1) csum += __shfl_xor(csum, o);
    __shared__ int64_t s_csum[NW];
    if (lane == 0) s_csum[wave] = csum;
    __syncthreads();
    int64_t total = 0;
    for (int w = 0; w < NW; ++w) total += s_csum[w];
    // the fair share of one workgroup: the waveform's cost over SPLIT_SLOTS_PER_WF workgroups
    // (a walker group of 16 then fills the chip's ~1,024 resident slots); a tile above it (and
    // above B.split_min) is split into its BPL bins
    const int64_t share = max((int64_t)B.split_min, total / SPLIT_SLOTS_PER_WF);
    int nS[PER];
    int my_items = 0, my_split = 0;
    for (int i = 0; i < PER; ++i) {
        const int u = tid * PER + i;
        const int S = (u < nut && s_cost[u] > share) ? BPL : 1;
        nS[i] = u < nut ? S : 0;
        my_items += nS[i];
        my_split += S > 1 ? 1 : 0;
    }
    // no tile above the share (config 4's full grid: costs within 1.5x of the median): no plan,
    // and none of the scans below
    if (!__syncthreads_or(my_split > 0)) return;
    int n_items, n_split;
    const int io = block_excl_scan<NW>(my_items, wsum, lane, wave, n_items);
    __syncthreads();
    const int po = block_excl_scan<NW>(my_split, wsum, lane, wave, n_split);
    __syncthreads();
    if (n_split == 0 || n_items > SPLIT_ITEM_CAP || n_split > SPLIT_TILE_CAP)
        return;   // nothing to split, or past the plan's capacity: the plain tile loop
    int4* items = V.sitem;
    int32_t* cnt = V.scnt;
    int ii = io, sp = po;
    for (int i = 0; i < PER; ++i) {
        const int u = tid * PER + i, S = nS[i];
        for (int j = 0; j < S; ++j)
            items[ii + j] = make_int4(ut0 + u, (j << 16) | S, S > 1 ? sp : -1, S > 1 ? sp : -1);
        if (S > 1) {
            cnt[sp] = 0;
            ++sp;
        }
        ii += S;
    }
    if (tid == 0) {
        hdr->nitems = n_items;
        hdr->nsplit = n_split;
    }
}

}  // namespace

// the split plan's cost floor (k_segments_one): SPLIT_MIN_COST, or EFD_SPLIT_MIN_COST when set
// (read per preparation; -1 splits every tile of the union: the tests' bitwise check of the
// sub-bin form)
static int32_t split_min_cost() {
    const char* e = getenv("EFD_SPLIT_MIN_COST");
    if (!e || !*e) return SPLIT_MIN_COST;
    const long long x = atoll(e);
    return x >= -1 && x <= (1 << 30) ? (int32_t)x : SPLIT_MIN_COST;
}

// Envelope records (k_items, env_fit.inc) in the uniform caustic mode; EFD_ENV=0 (read once per
// process) builds none: the A/B and parity switch of DESIGN.md's round-6 study. prepare decides
// per waveform and the sum follows the records (Item::jser), so they always agree.
static bool env_records() {
    static const bool v = [] {
        const char* e = std::getenv("EFD_ENV");
        return !(e && e[0] == '0');
    }();
    return v;
}

// Waveform i of a batch, checked: its arguments, its workspace's size against its own layout L,
// and its descriptor d, with the switches (lists, pcr, env) that follow from its own (N_t, K).
// F names the caller in the error strings.
static int fill_desc(const std::string& F, const efd_modesum_args* const* a,
                     void* const* workspace, const size_t* workspace_bytes, int i, PrepDesc& d,
                     Layout& L) {
    const efd_modesum_args* ai = a[i];
    const int rc = efdhip::check_modesum_args(ai, workspace[i], 1);
    if (rc != EFD_OK) return rc;
    if (ai->nf != a[0]->nf || (ai->grid_symmetric != 0) != (a[0]->grid_symmetric != 0))
        return fail(EFD_ERR_ARG, F + ": nf and grid_symmetric must agree across the batch");
    L = make_layout(ai->nt, ai->K, ai->nf, ai->grid_symmetric ? 1 : 0);
    if (workspace_bytes[i] < L.total)
        return fail(EFD_ERR_WORKSPACE, F + ": workspace too small (see "
                                           "efd_modesum_workspace_bytes)");
    for (int j = 0; j < i; ++j)
        if (workspace[j] == workspace[i])
            return fail(EFD_ERR_ARG, F + ": one workspace per waveform");
    d.t = ai->t; d.phi_phi = ai->phi_phi; d.phi_r = ai->phi_r; d.f_phi = ai->f_phi;
    d.f_r = ai->f_r; d.amp = ai->amp; d.ylm_p = ai->ylm_p; d.ylm_m = ai->ylm_m;
    d.freq = ai->freq; d.m = ai->m; d.n = ai->n;
    d.ws = (char*)workspace[i];
    d.sc_re = ai->scale_re; d.sc_im = ai->scale_im;
    d.nt = ai->nt; d.K = ai->K;
    d.lists = efdhip::list_mode(ai->K, L.ntiles);
    d.env = (ai->caustic == EFD_CAUSTIC_UNIFORM && env_records()) ? 1 : 0;
#ifdef EFD_EXP_NO_PCR   // experiment: every waveform on the Thomas kernels (the twin's solve order)
    const bool pcr = false;
#else
    const bool pcr = ai->nt >= 4 && ai->nt <= PCR_NMAX;
#endif
    d.pcr = pcr ? (ai->K < PCR_MAX_K ? 3 : 1) : 0;
    return EFD_OK;
}

// The launch shape of a batch: the maxima its grids and dynamic LDS are sized for, and which
// kernels any of its waveforms needs
struct PrepShape {
    int ntmax = 0, Kmax = 0, ntmax_pcr = 0, pcr_blocks = 0;
    int64_t items_max = 0, seg_lds = 0;
    bool any_pcr = false, any_thomas = false, any_lists = false, any_order = false;
    void add(const PrepDesc& d) {
        any_lists |= d.lists != 0;
        any_order |= d.lists == 3;
        if (d.pcr) {
            any_pcr = true;
            ntmax_pcr = std::max(ntmax_pcr, d.nt);
            pcr_blocks = std::max(pcr_blocks, 4 + (d.pcr == 3 ? 5 : 1) * d.K);
        }
        if (d.pcr != 3) any_thomas = true;
        ntmax = std::max(ntmax, d.nt);
        Kmax = std::max(Kmax, d.K);
        // (G <= K groups; at large K each thread may take several records: config 2's 3,020
        // harmonics form 627 groups, so a K-sized grid was 79% workgroups that exit at once)
        const int64_t per = d.K >= ITEMS_SPLIT_K ? ITEMS_PER_THREAD_K : 1;
        items_max = std::max(items_max, ((int64_t)(d.nt - 1) * d.K + per - 1) / per);
        // k_segments_one: the largest ranges table that fits SEG1_LDS_CAP (K N_t int4s at most)
        const int64_t b = (int64_t)d.K * (d.nt - 1) * 16;
        if (b <= SEG1_LDS_CAP) seg_lds = std::max(seg_lds, b);
    }
};

// K0-K6 for the batch B of shape S on a grid of ntiles tiles
static int launch_chain(PrepBatch& B, const PrepShape& S, int64_t ntiles, hipStream_t st) {
    const unsigned nz = (unsigned)B.n;
    const int Kmax = S.Kmax;
    // K0: (m, n) groups (in k_prep_pcr_b's blocks when the batch allows) and, for the Thomas
    // kernel's amplitude role, their amplitudes at the knots (the PCR amplitude waves evaluate
    // their own)
    B.pcr_groups = (!S.any_thomas && Kmax <= PCR_GROUPS_MAX_K) ? 1 : 0;
    if (!B.pcr_groups) {
        hipLaunchKernelGGL(k_group_b, dim3(1, 1, nz), dim3(256), 0, st, B);
        HIP_TRY(hipGetLastError());
    }
    if (S.any_thomas) {
        const int gper = Kmax >= ITEMS_SPLIT_K ? ITEMS_PER_THREAD_K : 1;
        hipLaunchKernelGGL(k_group_amp_b, dim3((Kmax / gper + 255) / 256, S.ntmax, nz),
                           dim3(256), 0, st, B);
        HIP_TRY(hipGetLastError());
    }
    // K1-K3: trajectory splines, group amplitude splines, inverse splines (grids sized for
    // G = K, blocks past the device-side G return at once)
    if (S.any_pcr) {   // one wave per interpolant, parallel cyclic reduction
        hipLaunchKernelGGL(k_prep_pcr_b, dim3(S.pcr_blocks, 1, nz), dim3(64),
                           sizeof(double) * 9 * S.ntmax_pcr, st, B);
        HIP_TRY(hipGetLastError());
    }
    if (S.any_thomas) {
        const int nb = 1 + (4 * Kmax + 63) / 64 + (Kmax + 63) / 64;
        hipLaunchKernelGGL(k_prep_b, dim3(nb, 1, nz), dim3(64), sizeof(double) * 7 * S.ntmax,
                           st, B);
        HIP_TRY(hipGetLastError());
    }
    // K4: interval records
    hipLaunchKernelGGL(k_items, dim3((unsigned)((S.items_max + 255) / 256), 1, nz), dim3(256), 0,
                       st, B);
    HIP_TRY(hipGetLastError());
    // K5: segment table
    if (Kmax <= SEG1_MAX_K) {
        B.seg_lds = (int32_t)S.seg_lds;
        B.split_min = split_min_cost();
        hipLaunchKernelGGL(k_segments_one, dim3(1, 1, nz), dim3(SEG1_NT), (size_t)B.seg_lds, st,
                           B);
        HIP_TRY(hipGetLastError());
    } else {
        const int nslot = Kmax * MAXRUNS * 2;
        const int nblk = (nslot + 255) / 256;
        hipLaunchKernelGGL(k_segment_slots, dim3(nblk, 1, nz), dim3(256), 0, st, B);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_segment_compact, dim3(nblk, 1, nz), dim3(256), 0, st, B);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_seg_tiles, dim3((unsigned)std::min(nslot, 1024), 1, nz), dim3(256),
                           0, st, B);
        HIP_TRY(hipGetLastError());
    }
    // K6: the tiles' record lists (k_tile_keys, with the sum in emrifd.hip): moves the
    // latency-bound build out of the mode sum into the preparation phase, which overlaps the
    // previous waveform's sum in a two-stream pipeline
    return efdhip::launch_tile_lists(&B, ntiles, S.any_lists, S.any_order, st);
}

// Preparation (K0-K6) of `count` waveforms in one chain of launches; blockIdx.z = waveform.
// efd_modesum_prepare and efd_modesum's first phase are a batch of one.
int efdhip::prepare_batch(const char* fn, const efd_modesum_args* const* a,
                          void* const* workspace, const size_t* workspace_bytes, int32_t count,
                          void* stream) {
    const std::string F(fn);
    if (!a || !workspace || !workspace_bytes) return fail(EFD_ERR_ARG, F + ": NULL argument");
    if (count < 1 || count > EFD_BATCH_MAX)
        return fail(EFD_ERR_ARG, F + ": count out of range [1, EFD_BATCH_MAX]");
    PrepBatch B{};
    B.n = count;
    PrepShape S;
    int64_t ntiles = 0;
    for (int i = 0; i < count; ++i) {
        Layout L;
        const int rc = fill_desc(F, a, workspace, workspace_bytes, i, B.d[i], L);
        if (rc != EFD_OK) return rc;
        S.add(B.d[i]);
        if (i == 0) {   // the grid, which the batch shares
            B.paired = a[0]->grid_symmetric ? 1 : 0;
            B.nf = a[0]->nf;
            B.nl = L.nlanes;
            B.nl1 = B.paired ? ((B.nf % 2) ? L.nlanes - 1 : L.nlanes) : B.nf;
            ntiles = L.ntiles;
        }
    }
    return launch_chain(B, S, ntiles, (hipStream_t)stream);
}

// The TD sum's preparation: a batch of one on the TD workspace (B.td) through k_group_b,
// k_group_amp_b and k_prep_b with every role on Thomas (pcr = 0), on the grids of one waveform
int efdhip::td_prepare(const efd_td_args* a, void* workspace, hipStream_t st) {
    PrepBatch B{};
    B.n = 1;
    B.td = 1;
    PrepDesc& d = B.d[0];
    d.t = a->t; d.phi_phi = a->phi_phi; d.phi_r = a->phi_r; d.f_phi = a->f_phi; d.f_r = a->f_r;
    d.amp = a->amp; d.ylm_p = a->ylm_p; d.ylm_m = a->ylm_m; d.m = a->m; d.n = a->n;
    d.ws = (char*)workspace;
    d.sc_re = a->scale_re; d.sc_im = a->scale_im;
    d.nt = a->nt; d.K = a->K;
    const int nt = a->nt, K = a->K;

    HIP_TRY(hipMemsetAsync(d.ws + make_td_layout(nt, K).header, 0, sizeof(Header), st));
    hipLaunchKernelGGL(k_group_b, dim3(1), dim3(256), 0, st, B);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_group_amp_b, dim3((K + 255) / 256, nt), dim3(256), 0, st, B);
    HIP_TRY(hipGetLastError());
    // k_prep_b's first two roles only (trajectory splines, group amplitude splines): the grid
    // stops before the inverse-spline blocks, which the TD sum does not need
    const int nb_amp = (4 * K + 63) / 64;
    hipLaunchKernelGGL(k_prep_b, dim3(1 + nb_amp), dim3(64), sizeof(double) * 7 * nt, st, B);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

#include "emrifd_modes_device.inc"

extern "C" {

int efd_spline_build(const double* x, int n, const double* y, int ninterp, double* coef,
                     void* stream) {
    if (!x || !y || !coef || n < 2 || ninterp <= 0 || n > MAX_NT)
        return fail(EFD_ERR_ARG, "efd_spline_build: bad arguments");
    const int threads = 64;   // spline_shared assumes 64-thread blocks
    const int blocks = (ninterp + threads - 1) / threads;
    hipLaunchKernelGGL(k_spline_shared, dim3(blocks), dim3(threads), sizeof(double) * 5 * n,
                       (hipStream_t)stream, x, n, y, ninterp, coef, (int64_t)4 * ninterp);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_modesum_prepare(const efd_modesum_args* a, void* workspace, size_t workspace_bytes,
                        void* stream) {
    // (the checks and messages of efd_modesum, whose first phase this is)
    const int rc = efdhip::check_modesum_args(a, workspace, 1);
    if (rc != EFD_OK) return rc;
    if (workspace_bytes < make_layout(a->nt, a->K, a->nf, a->grid_symmetric ? 1 : 0).total)
        return fail(EFD_ERR_WORKSPACE, "efd_modesum: workspace too small (see efd_modesum_workspace_bytes)");
    return efdhip::prepare_batch("efd_modesum_prepare", &a, &workspace, &workspace_bytes, 1,
                                 stream);
}

int efd_modesum_prepare_batch(const efd_modesum_args* const* a, void* const* workspace,
                              const size_t* workspace_bytes, int32_t count, void* stream) {
    return efdhip::prepare_batch("efd_modesum_prepare_batch", a, workspace, workspace_bytes,
                                 count, stream);
}

}  // extern "C"
