// emrifd.hip -- MI355X (gfx950, CDNA4) FD EMRI mode-sum: kernels + C ABI (include/emrifd.h).
//
// Hot path (BASELINE.json:north_star): for every
// selected harmonic k = (l, m, n) of the sparse inspiral, the stationary-phase spectrum
//   S(f) = - scale * sum_k [ Y+_k z_k(g) at f = -g ,  Y-_k conj(z_k(g)) at f = +g ]
//   z_k(g) = A_k(t) Q(F', F'') exp(i (2 pi g t - Phi_k(t))),  t = t_k(g) (inverse spline)
// restated from the reference notebook FD_waveform (Tutorial_FD_construction_single_mode.ipynb
// :552-623): Phi_k = m Phi_phi + n Phi_r (:558), F_k = m f_phi + n f_r (:564), t(f) from the
// inverse spline CubicSpline(F, t) (:566), supports (:569-572), F' and F'' spline derivatives
// (:579-584), amplitude spline (:587-594), K_{1/3} factor (:599-613), phases (:615-616).
// The oracle (oracle/fd_oracle.py) states the same maths in numpy; tests pin them together.
//
// Pipeline (one stream per phase, no host sync, no allocation). Preparation
// (efd_modesum_prepare, latency-bound kernels on few CUs, overlapping the previous sum); K0-K5
// are emrifd_prepare.hip, K6-K9 this unit:
//   K0 k_group, k_group_amp  (m, n) groups of the harmonics; per knot, the group amplitudes
//                            Bp = sum_l y0_l A_l, Bm = sum_l y1_l A_l
//   K1-K3 k_prep          one launch, three independent roles by workgroup:
//                         - 1 wave: not-a-knot splines of Phi_phi, Phi_r, f_phi, f_r and of the
//                           knot derivatives f_phi'(t_i), f_r'(t_i) (for F'' as notebook :583)
//                         - 1 lane per group amplitude interpolant (4G lanes), sharing one LDS
//                           factorisation of the knot matrix
//                         - 1 lane per group: F knots, monotonic runs, inverse spline per run
//   K4 k_items            1 thread per (group, knot interval): gathers every cubic the SPA
//                         needs for that interval into one 288-B record + its bin (lane) ranges
//   K5 k_segment_slots    1 thread per (group, run, sub-branch): its segment of records,
//      k_segment_compact  trimmed of clamped empty records; then compacted in slot order;
//      k_seg_tiles        per (segment, tile it covers) the record sub-range reaching the tile
//   K6 k_tile_keys        per tile, its ordered record list (prebuilt keys); launched at the
//                         end of the preparation chain, but it writes the list format that only
//                         the sum reads, so it lives here
//   K7 k_tile_order       tiles by cost, most expensive first (the sum's dispatch order)
// Mode sum (efd_modesum_sum):
//   K8 k_modesum          OUTPUT-STATIONARY: one 4-wave workgroup per tile of 256*BPL bins;
//                         each lane owns BPL bins (and their mirrors -f when the grid is
//                         symmetric: the +m branch and its -m partner share t(g), the
//                         amplitude/phase splines and sin/cos, so one evaluation feeds two
//                         bins); the tile's record list comes by LDS-DMA from K6 (or is built
//                         in LDS from the segment table, fixed order -> bitwise reproducible),
//                         records stream through a double-buffered LDS stage, and the tile
//                         writes its bins (or h+/hx) once -- no atomics, no host sync.
// The SPA evaluation is FP64 VALU work (phases reach ~1e7 rad); MFMA is not applicable.
//
//   K9 k_td_modesum       the TD sum over k_group's groups and k_prep's splines
//
// Written once here: SumDesc (one prepared waveform as the sum sees it: sum_desc fills it, both
// sum kernels take it by value, one modesum_tile overload unpacks it); the pieces of the tile
// list that K6 and the sum's own build share (seg_hits_tile, hit_records, list_key,
// scatter_slot, and block_excl_scan of emrifd_layout.h), pinned together by
// tests/test_gpu_tile_lists.py; the chunk-record header (HDR_*, hdr_pack, hdr_lo ... hdr_j4); the
// experiment counters (-DEFD_EXP), every use one EFD_EXP_DO(...) line.
//
// This unit is the mode sum (FD and TD), the tile lists it reads, and their C ABI. The
// preparation (K0-K5, efd_modesum_prepare*, efd_spline_build) is emrifd_prepare.hip; the two
// share emrifd_layout.h (constants, record and workspace formats, the host functions that cross).
// The window path (efd_hann_*, efd_cosw_*) is emrifd_window.hip; the channel split and the
// reductions (efd_polarizations, efd_loglike, efd_inner_product, efd_td_split*, efd_fisher_gram)
// are emrifd_reduce.hip. All four share emrifd_common.h.

#include "emrifd_layout.h"

#define EFD_VERSION 100  // 0.1.0

// the thread's last error (efd_last_error), set by every unit through fail
static thread_local std::string g_err;

int efdhip::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {

constexpr int NWAVE = TILE / 64;    // waves per workgroup
constexpr int XCD_GROUP = 1024 / TILE;  // consecutive tiles per XCD in the dispatch order
constexpr int SEGWIN = TILE;        // segments examined per window (tile list build): 4 KB of LDS
                                    // instead of 16 at 4 x TILE, so 4 workgroups fit a CU
constexpr int PIECES = (int)sizeof(Item) / 16;  // 16-B pieces per record
constexpr int B_PIECE = (int)offsetof(Item, b) / 16;   // first piece of b (b[0]: 4, b[1]: 4)
constexpr int ROUNDS = 2;                        // 16-B pieces per thread per LDS stage
constexpr int NC = (ROUNDS * TILE) / PIECES;     // records per LDS stage

// ----------------------------------------------------------------------------------------
// The tile's record list: the pieces that its two builds (k_tile_keys in the preparation phase,
// modesum_tile's own in the sum) share, so that both write the same keys in the same order.
// With block_excl_scan (emrifd_layout.h) for the placement of the hits' keys.
// ----------------------------------------------------------------------------------------

// a segment with lane range lh = [lo, hi) reaches into the tile [tlo, thi)
__device__ __forceinline__ bool seg_hits_tile(int2 lh, int32_t tlo, int32_t thi) {
    return lh.y > tlo && lh.x < thi;
}

// Records [p0, p0 + count) (lane order) of segment sg that reach into the tile [tlo, thi): from
// the segment-tile boundaries of k_seg_tiles, or by two bisections over the records' lane ranges
struct HitRecords {
    int p0, count;
};
__device__ __forceinline__ HitRecords hit_records(
    int sg, int64_t tile, int32_t tlo, int32_t thi, const int32_t* __restrict__ segbase,
    const int32_t* __restrict__ stb0, const int32_t* __restrict__ stb1,
    const int4* __restrict__ seginfo, const int4* __restrict__ ranges) {
    const int32_t sbase = segbase[sg];
    if (sbase != SEG_NO_STB) {
        const int q0 = stb0[sbase + tile], q1 = stb1[sbase + tile];
        return {q0, max(q1 - q0, 0)};
    }
    const int4 info = seginfo[sg];
    const int base = info.x, n = info.y, dir = info.z, sb = info.w;
    int lo = 0, hi = n;            // first p (lane order) with khi > tlo
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int4 rg = ranges[base + (dir > 0 ? mid : n - 1 - mid)];
        if ((sb ? rg.w : rg.y) > tlo) hi = mid; else lo = mid + 1;
    }
    const int p0 = lo;
    hi = n;                        // first p with klo >= thi
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int4 rg = ranges[base + (dir > 0 ? mid : n - 1 - mid)];
        if ((sb ? rg.z : rg.x) >= thi) hi = mid; else lo = mid + 1;
    }
    return {p0, lo - p0};
}

// the key of record p (lane order) of the segment info = (first record, count, direction,
// sub-branch): record index << 1 | sub-branch
__device__ __forceinline__ uint32_t list_key(int4 info, int p) {
    const int j = info.z > 0 ? p : info.y - 1 - p;
    return ((uint32_t)(info.x + j) << 1) | (uint32_t)info.w;
}

// Where key x of a window's `take` keys goes: the bijection x -> x * P mod take (P prime,
// take % P != 0). A segment's records cover neighbouring lanes, i.e. mostly one wave, and
// unscattered a chunk of NC consecutive records would keep one wave busy while the others wait
// at its barrier
__device__ __forceinline__ int scatter_slot(int x, int take) {
    const int P = (take % 97) ? 97 : 101;
    return (int)(((unsigned)x * (unsigned)P) % (unsigned)take);
}

// ----------------------------------------------------------------------------------------
// SPA arithmetic
// ----------------------------------------------------------------------------------------

// sin/cos of a phase up to |x| ~ 1e9 rad: two-term FMA Cody-Waite reduction by pi/2 (the
// third term, q * 1.5e-33, is below half an ulp of r for |q| < 2^31) and fdlibm's kernel
// polynomials on [-pi/4, pi/4]. The quadrant is applied with a select (odd q swaps sin/cos)
// and sign-bit flips, all branch-free.
__device__ __forceinline__ double flip_sign_if(double v, int flip_bit_2) {
    // flip_bit_2 is 0 or 2: moves to bit 63
    return __longlong_as_double(__double_as_longlong(v) ^
                                ((unsigned long long)(unsigned)flip_bit_2 << 62));
}
__device__ __forceinline__ void sincos_big(double x, double& s, double& c) {
    constexpr double INV_PIO2 = 6.36619772367581382433e-01;
    constexpr double PIO2_1 = 1.57079632679489655800e+00;   // first 53 bits of pi/2
    constexpr double PIO2_2 = 6.12323399573676603587e-17;   // pi/2 - PIO2_1
    const double q = rint(x * INV_PIO2);
    double r = fma(-q, PIO2_1, x);
    r = fma(-q, PIO2_2, r);
    const int iq = (int)q;
    const double z = r * r;
    // fdlibm __kernel_sin / __kernel_cos coefficients
    const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10,
                       -2.50507602534068634195e-08), 2.75573137070700676789e-06),
                       -1.98412698298579493134e-04), 8.33333333332248946124e-03),
                       -1.66666666666666324348e-01);
    const double sr = fma(r * z, ps, r);
    const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11,
                       2.08757232129817482790e-09), -2.75573143513906633035e-07),
                       2.48015872894767294178e-05), -1.38888888888741095749e-03),
                       4.16666666666666019037e-02);
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double cr = w + (((1.0 - w) - hz) + z * z * pc);
    const bool odd = (iq & 1) != 0;
    s = flip_sign_if(odd ? cr : sr, iq & 2);
    c = flip_sign_if(odd ? sr : cr, (iq + 1) & 2);
}

// sin/cos for the fast path: reduce by pi/256 against a 512-entry table of
// (sin, cos)(k pi/256) held in LDS, then short Taylor polynomials on |r| <= pi/512 (sin to r^3:
// truncation r^5/120 < 7.4e-14, far below the ~1e-9 rad rounding of phases that reach 1e7 rad;
// cos to r^4: < 1e-16) and the angle-sum formula: ~13 FP64 operations
// instead of ~26 plus the quadrant logic of sincos_big. `shift` (an integer number of table
// steps) is added to the angle exactly, through the table index. Valid for |x| < 2^31 pi/256.
// The reduction is one FMA against the leading 53 bits of the step: the dropped q * STEP_2 is
// < 3.9e-17 |x|, below half an ulp of x itself (the rounding every phase already carries), and
// one FMA less on the longest dependency chain of an evaluation (k_modesum +1.2-1.6%, the
// spectrum moves by 8e-12 of max|S| at config 2).
constexpr int SCTAB = 512;
// The cosine on |r| <= pi/512 as COS_A - z/2 (z = r^2) with the constant chosen
// minimax (max error 2.95e-11 = half the dropped z^2/24 at r = pi/512; mpmath), one FMA instead
// of the r^4 Taylor form's two. 2.95e-11 of a term is far below the ~1e-9 rad rounding every
// term's phase already carries (phases reach 1e7 rad). The slope stays -0.5 (an inline
// constant: the free minimax slope, 7.4e-12, cost an SGPR pair and VGPR moves in the record
// loop). COS_A is the constant callers pass as c0 (J <= 2 records fold rho - 1 into it:
// fma(-v, v, COS_A) = COS_A rho to 2e-20).
// (COS_A, COS_B: emrifd_constants.h, shared with the host twin)
static_assert(COS_A == ENV_AMP_SCALE, "envelope amplitudes carry COS_A (k_items)");
__device__ __forceinline__ void sincos_tab(double x, int shift, const double2* __restrict__ tab,
                                           double& s, double& c, double extra = 0.0,
                                           bool use_extra = false, double extra_scale = 1.0,
                                           double c0 = COS_A) {
    constexpr double INV_STEP = 81.48733086305042;       // 256 / pi
    constexpr double STEP_1 = 0.01227184630308513;       // pi/256, leading part
    // q = nearest integer to x / step via the 1.5 * 2^52 shifter: its low word is q itself
    // (two's complement), so neither rint nor a float->int conversion is needed
    constexpr double SHIFTER = 6755399441055744.0;
    const double qs = fma(x, INV_STEP, SHIFTER);
    const double q = qs - SHIFTER;
    double r = fma(-q, STEP_1, x);
    // a small angle (|extra_scale * extra| < 1e-3) added after the reduction
    if (use_extra) r = fma(extra_scale, extra, r);
    const int qi = __double2loint(qs);
    // (sin, cos)((q + shift) pi/256), addressed in bytes: v_lshl_add + v_and
    const uint32_t off = ((uint32_t)qi * 16u + (uint32_t)shift * 16u) & (uint32_t)(16 * (SCTAB - 1));
    const double2 t = *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(tab) + off);
    const double z = r * r;
    const double sr = fma(r * z, -1.6666666666666666e-01, r);
    // c0: the cosine polynomial's constant term (1, or a factor 1 + O(1e-9) folded in by the
    // caller: rho (1 + d) E to within |d| |sr| < 3e-12, see spa_fast_m)
    const double cr = fma(z, COS_B, c0);
    s = fma(t.x, cr, t.y * sr);
    c = fma(t.y, cr, -t.x * sr);
}

// amp (sin, cos)(x + shift pi/256) for the envelope records, in the tangent form: with the
// table's (sin a, cos a), sin(a + r) = cos r (sin a + cos a tan r) and cos(a + r) =
// cos r (cos a - sin a tan r), so the amplitude multiplies cos r once instead of both outputs.
// tan r = r + r^3/3 (dropped 2 r^5/15 <= 1.1e-12 at |r| <= pi/512); cos r as sincos_tab's minimax
// COS_A - r^2/2, with COS_A already in the record's amplitude (k_items: amp = COS_A A) so that
// amp cos r = amp (1 + h), h = -r^2/2 (the product's -1/2 from the output modifier, IEEE mode
// off in k_modesum as for rsqrt_pos_sum; COS_A h against h: 6e-16 relative). 11 FP64 operations
// against sincos_tab's 11 plus the two products.
__device__ __forceinline__ void sincos_tab_amp(double x, int shift,
                                               const double2* __restrict__ tab, double amp,
                                               double& wr, double& wi) {
    constexpr double INV_STEP = 81.48733086305042;       // 256 / pi
    constexpr double STEP_1 = 0.01227184630308513;       // pi/256, leading part
    constexpr double SHIFTER = 6755399441055744.0;
    const double qs = fma(x, INV_STEP, SHIFTER);
    const double q = qs - SHIFTER;
    const double r = fma(-q, STEP_1, x);
    const int qi = __double2loint(qs);
    const uint32_t off = ((uint32_t)qi * 16u + (uint32_t)shift * 16u) & (uint32_t)(16 * (SCTAB - 1));
    const double2 t = *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(tab) + off);
    double h;
    asm("v_mul_f64 %0, -%1, %2 div:2" : "=v"(h) : "v"(r), "v"(r));
    const double tr = fma(r * h, -0.6666666666666666, r);
    const double ac = fma(amp, h, amp);
    wi = ac * fma(t.y, tr, t.x);
    wr = ac * fma(-t.x, tr, t.y);
}

// 1/sqrt(x) for finite x > 0 inside k_modesum: the hardware estimate plus one Newton
// (second-order) correction, relative error ~1e-15 (the OCML sequence's third-order step costs
// one more FP64 operation for the last bits; the SPA amplitude needs no more; callers mask
// x <= 0), with the halving on the FMA's output modifier: e/2 comes straight out of
// v_fma_f64 ... div:2, one FP64 operation fewer. The output modifiers apply only with IEEE mode
// off and FP64 denormals flushed (tools/rsq_omod_check.hip: otherwise the modifier is silently
// ignored), which modesum_tile sets in the MODE register; the compiler never emits them itself in
// IEEE mode, hence the inline asm. Only for k_modesum's mode.
__device__ __forceinline__ double rsqrt_pos_sum(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double h;
    asm("v_fma_f64 %0, -%1, %2, 1.0 div:2" : "=v"(h) : "v"(x * y), "v"(y));
    return fma(y, h, y);
}

// Q factor. The mirror-convention term of one branch is A Y Q e^{i(2 pi g t - Phi)} with
//   SPA:      Q_spa = e^{i sgn(F') 3 pi/4} / sqrt|F'|
//   uniform:  Q = i F'/|F''| K_{1/3}(z) e^{z} 2/sqrt(3),  z = -i y,  y = 2 pi F'^3 / (3 F''^2)
//             (notebook :599-608). Since i F'/|F''| sqrt(pi/(2z)) 2/sqrt(3) == Q_spa exactly,
//             Q = Q_spa * sum_k a_k (i w)^k,  w = 1/y, a_k the Hankel asymptotic coefficients
//             of K_{1/3}: a_k = a_{k-1} (4/9 - (2k-1)^2) / (8k).
// The kernel folds arg(Q_spa) into the phase and multiplies A by the series (R + i I).
// Series split: R = sum_j b_j u^j, I = w sum_j c_j u^j, u = w^2, b_j = (-1)^j a_{2j},
// c_j = (-1)^j a_{2j+1}. With 6 terms the truncation is < 1e-17 for |y| >= 555 (fast path);
// smaller |y| (hours before plunge, turning points) takes kfactor_slow.



// G(w) from the table of tools/gen_kfactor_table.py for w = 1/|y| in [2^KTAB_E_LO, 2^KTAB_E_HI)
// (y > 0; for y < 0 the caller negates I): interval (binade e, quarter k) from the bits of w,
// local variable x = 8 m - (9 + 2k) in [-1, 1) exact (m = mantissa in [1, 2)), then one Horner
// chain of KTAB_DEG FMAs each for Re and Im. Max error 1.1e-16 against mpmath. Outside the range
// the interval index is clamped (callers mask or never get there).
static_assert(KTAB_WMIN == 0x1p-8 && KTAB_WMAX == 0x1p10 &&   // (emrifd_constants.h)
              KTAB_E_LO == -8 && KTAB_E_HI == 10, "KTAB_WMIN/WMAX follow the table's range");
__device__ __forceinline__ void kfactor_tab(double ww, double& R, double& I) {
    const uint32_t hi = (uint32_t)__double2hiint(ww);
    const int k = (int)((hi >> 18) & 3u);
    const int idx = min(max(4 * ((int)(hi >> 20) - 1023 - KTAB_E_LO) + k, 0), KTAB_N - 1);
    const double m = __hiloint2double((int)((hi & 0x000FFFFFu) | 0x3FF00000u), __double2loint(ww));
    const double x = fma(8.0, m, -(double)(9 + 2 * k));
    const double2* c = KTAB[idx];
    // coefficients in groups of KTAB_GRP pairs: a compiler barrier between groups keeps the
    // loads from being hoisted all at once (the general path runs inside k_modesum's 128-VGPR
    // budget)
    constexpr int KTAB_GRP = 4;
    static_assert((KTAB_DEG + 1) % KTAB_GRP == 0, "whole coefficient groups");
    double r = 0.0, im = 0.0;
#pragma unroll
    for (int g = KTAB_DEG + 1 - KTAB_GRP; g >= 0; g -= KTAB_GRP) {
        double2 cc[KTAB_GRP];
#pragma unroll
        for (int j = 0; j < KTAB_GRP; ++j) cc[j] = c[g + j];
#pragma unroll
        for (int j = KTAB_GRP - 1; j >= 0; --j) {
            r = fma(r, x, cc[j].x);
            im = fma(im, x, cc[j].y);
        }
        asm volatile("" ::: "memory");
    }
    R = r;
    I = im;
}

template <int J>
__device__ __forceinline__ void kseries(double ww, double& R, double& I) {
    if (J == 1) {
        R = 1.0;
        I = ww * KC[0];
        return;
    }
    const double uu = ww * ww;
    double r = KB[J - 1], im = KC[J - 1];
#pragma unroll
    for (int j = J - 2; j >= 0; --j) {
        r = fma(r, uu, KB[j]);
        im = fma(im, uu, KC[j]);
    }
    R = r;
    I = ww * im;
}
__device__ __forceinline__ void kseries_fast(double ww, double& R, double& I) {
    kseries<FAST_J>(ww, R, I);
}

// Ascending-series coefficients of kfactor_slow, c+-_k = 1 / (k! Gamma(k + 1 +- 1/3)) (the
// recurrence c_k = c_(k-1) / (k (k +- 1/3)) evaluated once, in double), and the Horner degree
// for |y| < i + 1 (next term < 1e-19 of the leading one); |y| < 18.4 needs at most 41.

// (R + i I) for |y| < FAST_Y: the table (kfactor_tab) down to |y| = 2^-10, below that the
// ascending series K = pi/(2 sin(pi/3)) (I_{-1/3} - I_{1/3}) divided by Q_spa.
__device__ __noinline__ void kfactor_slow(double fd, double fdd, double& R, double& I) {
    const double y = TWO_PI * fd * fd * fd / (3.0 * fdd * fdd);
    const double ay = fabs(y);
    if (ay * KTAB_WMAX > 1.0) {   // |y| > 2^-10: asymptotic series above 256, else the table
        const double ww = 1.0 / ay;
        if (ww < KTAB_WMIN) kseries<FAST_J>(ww, R, I);
        else kfactor_tab(ww, R, I);
        if (y < 0.0) I = -I;
        return;
    }
    // ascending series for K_{1/3}(z), z = -i y; K~ = K e^{z}: sp, sm = sum_k c+-_k q^k,
    // q = -y^2/4, by Horner to the degree |y| needs (no divisions, no convergence test)
    const double sgn = y > 0 ? 1.0 : -1.0;
    const double q = -0.25 * y * y;
    const int deg = ASC_DEG[min(18, (int)ay)];
    double sp = ASC_P[deg], sm = ASC_M[deg];
    for (int k = deg - 1; k >= 0; --k) {
        sp = fma(sp, q, ASC_P[k]);
        sm = fma(sm, q, ASC_M[k]);
    }
    const double zp = cbrt(0.5 * ay);     // (|y|/2)^{1/3}
    const double zm = 1.0 / zp;
    constexpr double c6 = 0.86602540378443864676, s6 = 0.5;  // cos, sin(pi/6)
    const double ipr = zp * c6 * sp, ipi = -sgn * zp * s6 * sp;
    const double imr = zm * c6 * sm, imi = sgn * zm * s6 * sm;
    constexpr double pref = PI / (2.0 * 0.86602540378443864676);
    const double Kr = pref * (imr - ipr), Ki = pref * (imi - ipi);
    double sy, cy;
    sincos(y, &sy, &cy);
    const double kr = Kr * cy + Ki * sy;   // K e^{-i y}
    const double ki = Ki * cy - Kr * sy;
    // Q = i f K~, f = (2/sqrt3) F'/|F''|; (R + iI) = Q / Q_spa = Q conj(Q_spa) |F'|
    const double f = 1.15470053837925152902 * fd / fabs(fdd);
    const double qr = -f * ki, qi = f * kr;
    const double a = 1.0 / sqrt(fabs(fd));
    constexpr double c34 = -0.70710678118654752440;
    const double sr = a * c34, si = (fd > 0 ? a : -a) * 0.70710678118654752440;
    const double afd = fabs(fd);
    R = (qr * sr + qi * si) * afd;
    I = (qi * sr - qr * si) * afd;
}

// Generic (slow-path) evaluation of group h's forward splines at t when t(g) overshoots the
// record's interval: search the knot and gather the cubic pieces directly.
struct FwdEval {
    double b[4];   // Bp re, Bp im, Bm re, Bm im
    double ph, fd, fdd;
};
__device__ __noinline__ FwdEval forward_generic(double tt, const double* __restrict__ t, int nt,
                                                int jhint, int h, int K, int m, int n,
                                                const double* __restrict__ coefA,
                                                const double* __restrict__ coefT) {
    // scipy: interval i with t_i <= tt < t_{i+1}, clamped to [0, nt-2] (extrapolation). t(g)
    // overshoots the record's interval jhint by little, so walk from there (1-2 loads).
    int j = jhint;
    while (j > 0 && tt < t[j]) --j;
    while (j < nt - 2 && tt >= t[j + 1]) ++j;
    const double w = tt - t[j];
    auto cub = [&](double c0, double c1, double c2, double c3) {
        return fma(fma(fma(c0, w, c1), w, c2), w, c3);
    };
    const double* ca = coefA + (size_t)j * 4 * 4 * K + 4 * h;
    const double* ct = coefT + (size_t)j * 32;
    const double dm = (double)m, dn = (double)n;
    FwdEval e;
    for (int q = 0; q < 4; ++q) e.b[q] = cub(ca[q], ca[4 * K + q], ca[8 * K + q], ca[12 * K + q]);
    e.ph = cub(dm * ct[0] + dn * ct[1], dm * ct[8] + dn * ct[9], dm * ct[16] + dn * ct[17],
               dm * ct[24] + dn * ct[25]);
    const double F0 = dm * ct[2] + dn * ct[3], F1 = dm * ct[10] + dn * ct[11],
                 F2 = dm * ct[18] + dn * ct[19];
    e.fd = fma(fma(3.0 * F0, w, 2.0 * F1), w, F2);
    const double G0 = dm * ct[4] + dn * ct[5], G1 = dm * ct[12] + dn * ct[13],
                 G2 = dm * ct[20] + dn * ct[21];
    e.fdd = fma(fma(3.0 * G0, w, 2.0 * G1), w, G2);
    return e;
}

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// the thread index made opaque at a use site: values derived from it are recomputed there instead
// of being hoisted to the kernel's prologue as loop invariants (which, live across the record
// loop's cold call, were spilled to scratch by every wave)
__device__ __forceinline__ int opq(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

__device__ __forceinline__ double cubic(const double* __restrict__ c, double w) {
    return fma(fma(fma(c[0], w, c[1]), w, c[2]), w, c[3]);
}

// The fast path's K_{1/3} factor in polar form, G = rho e^{i theta}: log G of the Hankel series,
// re-expanded as rho = sum_j RH_j u^j and theta = w sum_j TH_j u^j (y > 0; theta is odd in y),
// u = w^2, TH = {-0.069444444444444444444, 0.035525977366255144033, -0.11095169967421124829,
// 0.85188445191064930488}. The first omitted terms fall below 1e-17 at the same |y| bounds as
// KB / KC (JSER_Y), so a record's series length J serves both forms. theta is added to the
// reduced sin/cos argument (|r| <= pi/512, where it costs no rounding) and rho scales the
// amplitude: two FP64 operations fewer per evaluation than rotating by (R + iI). theta comes out
// in units of its leading coefficient (thn = theta / TH_0), so the add of theta to the reduced
// angle is one FMA with TH_0 (with the sign of F' and the v rescaling: RecSign::kth).
//   - Records of series length 3 take the fourth terms too (below 1e-17 on their intervals, by the
//     choice of J), so J = 3 and J = 4 share one real branch (the compiler otherwise if-converts
//     the J >= 4 increments and merges the results with 4 v_cndmask per evaluation).
//   - theta is an angle added to phases that reach 1e7 rad and carry ~1e-9 rad of rounding, so
//     its series stops at terms below 1e-13 rad instead of the 1e-17 (relative) that picks J for
//     rho, an amplitude factor: for J <= 2 records (|y| >= 8.7e3, 82% of records) the KTHN1 term
//     is at most 0.0694 * 0.512 |w|^3 = 5.4e-14 rad and theta = TH_0 w; for J >= 3 the KTHN3
//     term is at most 4.2e-16 rad (|y| >= 153).
// Lane predicates as wave masks in scalar registers: every VALU instruction issues in 4 cycles
// per wave64, an FP64 FMA's cost, so the fast path's per-lane booleans (lane range: 2 integer
// compares per bin; the |y| test of a series-length-4 record; the any-lane test of the general
// path) are masks: the lane range from the record's bounds in SALU (lane_range_mask), each
// comparison's result taken by ballot (the compare itself writes the mask), the |y| test only in
// a wave-uniform branch for records that need it, and the masks combined in SALU.
// lanes l of the wave with lo <= l < hi (wave-uniform bounds, any range). Selects, not a clamp:
// min/max of a uniform value becomes v_med3 + v_readfirstlane (2 VALU), the selects stay SALU.
__device__ __forceinline__ uint64_t lanes_below(int32_t x) {
    const uint64_t m = x >= 64 ? ~0ull : ((1ull << (x & 63)) - 1ull);
    return x <= 0 ? 0ull : m;
}
__device__ __forceinline__ uint64_t lane_range_mask(int32_t lo, int32_t hi) {
    return lanes_below(hi) & ~lanes_below(lo);
}
// The sign of F' is the record's (Item::fdneg, wave-uniform), so the table shift and the angle's
// sign are scalar values: one v_cmp_class (F' of the record's sign, nonzero) replaces an |F'| > 0
// compare, a per-lane sign compare, a shift select and a copysign (lanes whose F' has the other
// sign, at turning points, take the general path). The class test is inline asm: the builtin's
// boolean is turned into a VGPR and compared back (2 VALU) before a ballot.
struct RecSign {
    int32_t fdcls;   // v_cmp_class mask: F' normal or subnormal of the record's sign
    int32_t shift;   // sign(F') 3 pi / 4 in table steps
    double kth;      // theta = kth * min(|thn|, 1): KTH0 with the sign of F'
    bool safe;       // every lane passes the interval and sign tests (record_safe)
};
// bits: Item::fdneg (bit 0: F' < 0, bit 1: safe record)
__device__ __forceinline__ RecSign rec_sign(uint32_t bits) {
    const bool fdneg = bits & 1u;
    RecSign r;
    r.safe = (bits & 2u) != 0;
    r.fdcls = fdneg ? 0x018 : 0x180;
    r.shift = fdneg ? -192 : 192;
    r.kth = fdneg ? -KTH0 / VS : KTH0 / VS;
    return r;
}
// lanes where v_cmp_class_f64(x, cls) holds, as a wave mask
__device__ __forceinline__ uint64_t class_mask(double x, int32_t cls) {
    uint64_t m;
    asm volatile("v_cmp_class_f64_e64 %0, %1, %2" : "=s"(m) : "v"(x), "s"(cls));
    return m;
}
// Masking the fast path's amplitude: k_modesum runs with FP64 denormals
// flushed (modesum_tile sets the MODE register; no value of the sum comes near 1e-308), so
// clearing the high word alone turns any amp -- inf and NaN included -- into a denormal that
// every later FP64 operation reads as +0: one v_cndmask_b32 instead of two for the 64-bit
// select, with bitwise the same W (+0 either way).
__device__ __forceinline__ double ftz_select(bool ok, double v) {
    return __hiloint2double(ok ? __double2hiint(v) : 0, __double2loint(v));
}
// k_modesum's packed chunk record header: one word per record, built by one lane per record
// once per chunk and read by v_readlane (a VALU instruction, as costly as an FMA) instead of an
// LDS round trip and 5 address / readfirstlane operations per record. Fields, low bits first:
// the sub-branch's lane range clamped to the tile, relative to its first lane (lo, hi: HDR_HB
// bits each), the sub-branch s (1 bit), the series length Item::jser (3 bits) and Item::fdneg
// (2 bits: F' < 0, certified safe)
constexpr int HDR_HB = TILE_LANES < 1024 ? 10 : 11;   // bits of a tile-relative bound
constexpr uint32_t HDR_HM = (1u << HDR_HB) - 1u;
constexpr int HDR_S = 2 * HDR_HB, HDR_J = 2 * HDR_HB + 1, HDR_FD = 2 * HDR_HB + 4;
static_assert(FAST_J < 8, "header: jser in 3 bits");
static_assert(TILE_LANES < 2048 && HDR_FD + 2 <= 32, "header: one 32-bit word");
__device__ __forceinline__ uint32_t hdr_pack(uint32_t lo, uint32_t hi, int s, int32_t jser,
                                             int32_t fdneg) {
    return lo | (hi << HDR_HB) | ((uint32_t)s << HDR_S) | ((uint32_t)jser << HDR_J) |
           ((uint32_t)fdneg << HDR_FD);
}
__device__ __forceinline__ int32_t hdr_lo(uint32_t ha) { return (int32_t)(ha & HDR_HM); }
__device__ __forceinline__ int32_t hdr_hi(uint32_t ha) {
    return (int32_t)((ha >> HDR_HB) & HDR_HM);
}
__device__ __forceinline__ int hdr_s(uint32_t ha) { return (int)((ha >> HDR_S) & 1u); }
__device__ __forceinline__ uint32_t hdr_jser(uint32_t ha) { return (ha >> HDR_J) & 7u; }
__device__ __forceinline__ uint32_t hdr_fdneg(uint32_t ha) { return (ha >> HDR_FD) & 3u; }
__device__ __forceinline__ uint32_t hdr_safe(uint32_t ha) { return (ha >> (HDR_FD + 1)) & 1u; }
// A wave-uniform test of the record header, re-derived in SALU at each use: the empty asm
// makes the header word "new" to the compiler, so the test is an s_and + s_cmp on the SGPR
// instead of a boolean kept alive across the bins' blocks, which the compiler turned into a
// VGPR and back (v_cndmask + v_cmp, 2 VALU) for every bin after the first.
__device__ __forceinline__ bool hdr_test(uint32_t ha, uint32_t mask) {
    asm volatile("" : "+s"(ha));
    return (ha & mask) != 0;
}
__device__ __forceinline__ bool hdr_j3(uint32_t ha) {   // the record's series length J >= 3
    asm volatile("" : "+s"(ha));
    return hdr_jser(ha) >= 3u;
}
__device__ __forceinline__ bool hdr_j4(uint32_t ha) {   // J >= 4
    asm volatile("" : "+s"(ha));
    return hdr_jser(ha) >= 4u;
}
// The common record class on its own straight-line body: certified safe, series length J <= 2
// and covering the wave's whole 64 BPL-lane chunk (every lane evaluates, every lane passes the
// interval and sign tests), so no lane mask, no amplitude select and no series branch:
// spa_fast_m's J <= 2 arithmetic, bitwise the same values (config 2: kernel 5.128 -> 4.978 ms
// per launch of 8, +3.2% waveforms/s, 3 paired rounds, profiles/r05d_ab_fastpath.jsonl)
__device__ __forceinline__ void spa_simple(const Item* __restrict__ it, double sfk, double stfk,
                                           const double2* __restrict__ sct, const RecSign& rs,
                                           double& wr, double& wi, double& w) {
    const double u = sfk - it->gx;
    const double tt = fma(fma(fma(it->ic[0], u, it->ic[1]), u, it->ic[2]), u, it->ic[3]);
    w = tt - it->tj;
    const double ph = fma(fma(fma(it->ph[0], w, it->ph[1]), w, it->ph[2]), w, it->ph[3]);
    const double fd = fma(fma(it->fd[0], w, it->fd[1]), w, it->fd[2]);
    const double amp = rsqrt_pos_sum(fabs(fd));
    const double psi0 = fma(stfk, tt, -ph);
    const double fdds = fma(fma(it->fdd[0], w, it->fdd[1]), w, it->fdd[2]);
    const double a3 = amp * amp * amp;
    const double t3 = fdds * a3;
    const double ww = t3 * t3;
    double sn, cs;
    sincos_tab(psi0, rs.shift, sct, sn, cs, ww, true, rs.kth, fma(-ww, ww, COS_A));
    wr = amp * cs;
    wi = amp * sn;
}
// The same for series length J = 3 (16% of config 2's records): spa_fast_m's J >= 3 branch with
// every lane active and in range (k_items gives J = 3 only when |y| >= 555 / 1.1 on the whole
// interval, far inside FAST_Y = 153), bitwise its values (+1.8% config 2, CI 1.006-1.023, 3
// paired rounds, profiles/r05g_ab_fast3.jsonl)
__device__ __forceinline__ void spa_simple3(const Item* __restrict__ it, double sfk, double stfk,
                                            const double2* __restrict__ sct, const RecSign& rs,
                                            double& wr, double& wi, double& w) {
    const double u = sfk - it->gx;
    const double tt = fma(fma(fma(it->ic[0], u, it->ic[1]), u, it->ic[2]), u, it->ic[3]);
    w = tt - it->tj;
    const double ph = fma(fma(fma(it->ph[0], w, it->ph[1]), w, it->ph[2]), w, it->ph[3]);
    const double fd = fma(fma(it->fd[0], w, it->fd[1]), w, it->fd[2]);
    const double amp = rsqrt_pos_sum(fabs(fd));
    const double psi0 = fma(stfk, tt, -ph);
    const double fdds = fma(fma(it->fdd[0], w, it->fdd[1]), w, it->fdd[2]);
    const double a3 = amp * amp * amp;
    const double t3 = fdds * a3;
    const double ww = t3 * t3;
    const double uu = ww * ww;
    const double r = fma(45.7, uu * uu, 1.0 - uu);
    const double thn = ww * fma(-14.733333333333333333, uu, 1.0);
    const double am = amp * r;
    double sn, cs;
    sincos_tab(psi0, rs.shift, sct, sn, cs, thn, true, rs.kth, COS_A);
    wr = am * cs;
    wi = am * sn;
}
// Envelope records (k_items, env_fit.inc; Item::jser = 0, always certified safe): the phase with
// theta already in the record's phase cubic and the amplitude A(w) = rho / sqrt|F'| from its
// degree-ENV_DEG polynomial, for the NB bins of the lane. 26 FP64 operations per bin instead of
// spa_simple's 36 (the sin/cos in sincos_tab_amp's tangent form): no F', F'' quadratics, no 1/sqrt|F'| Newton step, no 1/|y| and no angle or rho
// fold in the sin/cos.
// MASK: the record covers the wave's chunk only partly; lanes outside am[i] get A = +0 (flushed).
template <bool MASK, int NB>
__device__ __forceinline__ void env_record(const Item* __restrict__ it, const double* fk,
                                           const double* tfk, const double2* __restrict__ sct,
                                           const RecSign& rs, const uint64_t* am, double* wr,
                                           double* wi, double* w) {
    const double* e = env_of(it);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const double u = fk[i] - it->gx;
        const double tt = fma(fma(fma(it->ic[0], u, it->ic[1]), u, it->ic[2]), u, it->ic[3]);
        w[i] = tt - it->tj;
        const double ph = fma(fma(fma(it->ph[0], w[i], it->ph[1]), w[i], it->ph[2]), w[i], it->ph[3]);
        const double psi0 = fma(tfk[i], tt, -ph);
        double amp = e[0];
#pragma unroll
        for (int c = 1; c <= ENV_DEG; ++c) amp = fma(amp, w[i], e[c]);
        if (MASK) amp = ftz_select(__builtin_amdgcn_inverse_ballot_w64(am[i]), amp);
        sincos_tab_amp(psi0, rs.shift, sct, amp, wr[i], wi[i]);
    }
}
template <int CAUSTIC>
__device__ __forceinline__ void spa_fast_m(const Item* __restrict__ it, double sfk, double stfk,
                                           uint32_t ha, uint64_t actm,
                                           const double2* __restrict__ sct,
                                           const RecSign& rs, double& wr, double& wi, double& w,
                                           uint64_t& needm) {
    const double u = sfk - it->gx;
    const double tt = fma(fma(fma(it->ic[0], u, it->ic[1]), u, it->ic[2]), u, it->ic[3]);
    w = tt - it->tj;
    const double ph = fma(fma(fma(it->ph[0], w, it->ph[1]), w, it->ph[2]), w, it->ph[3]);
    const double fd = fma(fma(it->fd[0], w, it->fd[1]), w, it->fd[2]);
    const double afd = fabs(fd);
    uint64_t goodm = ~0ull;
    if (!hdr_test(ha, 2u << HDR_FD)) {   // wave-uniform: a record k_items could not certify tests every lane
        asm volatile("");
        goodm = __builtin_amdgcn_ballot_w64((unsigned long long)__double_as_longlong(w) <
                                            (unsigned long long)__double_as_longlong(it->dtj)) &
                class_mask(fd, rs.fdcls);
    }
    // F' = 0 gives amp = NaN here; every quantity it reaches is selected away below
    const double amp = rsqrt_pos_sum(afd);
    const double psi0 = fma(stfk, tt, -ph);
    double sn, cs;
    if (CAUSTIC == EFD_CAUSTIC_UNIFORM) {
        static_assert(FAST_J == 4, "early mask: the J >= 3 branch covers J = 3 and 4");
        // The amplitude is masked before it enters 1/|y|: masked lanes get amp = +0 (inf and
        // NaN included), so w = 0, theta = 0 and rho = 1 there and the angle stays finite with no
        // clamp; for J <= 3 records every in-interval lane is within the series' range, so
        // nothing else needs masking. J <= 2 (82% of records): rho - 1 = KRH_1 w^2 < 4.6e-10
        // goes into the cosine polynomial's constant term instead of a multiply of the
        // amplitude (rho E to within |rho - 1| |sr| < 3e-12, a rotation far below the phases'
        // 1e-9 rad rounding). J >= 3 (18%) tests |y| >= FAST_Y, clamps w for the lanes past it
        // and masks their amplitude again.
        const double ampm = ftz_select(__builtin_amdgcn_inverse_ballot_w64(actm & goodm), amp);
        const double fdds = fma(fma(it->fdd[0], w, it->fdd[1]), w, it->fdd[2]);
        const double a3 = ampm * ampm * ampm;
        const double t3 = fdds * a3;
        double ww = t3 * t3;   // 1/|y|
        double am, c0, thn;
        if (hdr_j3(ha)) {   // J >= 3: wave-uniform; a real branch (see KTH0's notes)
            asm volatile("");
            // the |y| >= FAST_Y test only matters for J = 4 (J = 3 lanes pass it by their
            // record's bound), but a nested J test's condition crossed the join as a per-lane
            // boolean (v_cndmask + v_cmp for every record)
            // |w| <= 1/153: rho's KRH_3 term (< 2.2e-14) and theta's KTHN_2 term (< 1.3e-12 rad)
            // are below the accuracy of the rest of the evaluation
            // ww = v = VS w: rho = 1 - v^2 + (KRH_2 / KRH_1^2) v^4, theta / (TH_0 / VS) =
            // v (1 + (KTHN_1 / |KRH_1|) v^2)
            // lanes past the series' range get w = +0 (high word cleared, flushed): finite
            // angle, masked amplitude below; one v_cndmask instead of fmin's max + min
            const uint64_t inrange = __builtin_amdgcn_ballot_w64(ww <= VS / FAST_Y);
            goodm &= inrange;
            ww = ftz_select(__builtin_amdgcn_inverse_ballot_w64(inrange), ww);
            const double uu = ww * ww;
            const double r = fma(45.7, uu * uu, 1.0 - uu);
            thn = ww * fma(-14.733333333333333333, uu, 1.0);
            am = ftz_select(__builtin_amdgcn_inverse_ballot_w64(actm & goodm), ampm * r);
            c0 = COS_A;
        } else {
            c0 = fma(-ww, ww, COS_A);   // (1 + KRH_1 w^2) COS_A = (1 - v^2) COS_A
            thn = ww;
            am = ampm;
        }
        sincos_tab(psi0, rs.shift, sct, sn, cs, thn, true, rs.kth, c0);
        wr = am * cs;
        wi = am * sn;
    } else {
        const bool ok = __builtin_amdgcn_inverse_ballot_w64(actm & goodm);
        const double am = ftz_select(ok, amp);
        sincos_tab(psi0, rs.shift, sct, sn, cs);
        wr = am * cs;
        wi = am * sn;
    }
    needm = actm & ~goodm;
}

#ifdef EFD_EXP
// record evals, cold-path evals, cold lanes, skips; cold lanes by cause: overshoot, 18.4 <= |y| <
// FAST_Y, |y| < 18.4
// Experiment build (-DEFD_EXP, tools/exp_variants.py): counters and per-tile clocks. Never in the
// product library (tests/test_abi.py checks that efd_exp_* is not exported).
constexpr int EXP_NCOUNT = 40;
__device__ unsigned long long g_exp_count[EXP_NCOUNT];  // [8..15]: |y| bands of kfactor_slow's J;
// [16, 17]: cold wave evaluations / lanes (one-body kernel); [18..23]: overshoot bands of
// max(-w, w - dtj) / dtj: < 1e-12, 1e-9, 1e-6, 1e-3, 1e-1, larger; [24, 25, 26]: chunk barrier
// balance: sum over chunks of the busiest wave's record evaluations, of all waves' evaluations,
// and the number of chunks; [27, 28]: segment table size, hits per tile summed (k_tile_keys);
// [29]: wave-records of certified-safe records; [32..35]: wave-records by series length J = 1..4,
// [36]: sub-branch flips; [37..39]: wave-records off the straight-line path by cause (partial
// coverage, J >= 3, not certified; a record may count in several)
__device__ unsigned int g_exp_tile[16384];       // record evaluations per tile (first 16384)
__device__ unsigned long long g_exp_tclk[16384];  // wall clock (s_memrealtime) per tile
// EFD_EXP_DO(statements): the statements in an experiment build, nothing in the product
#define EFD_EXP_DO(...) __VA_ARGS__
__device__ __forceinline__ void exp_add(int i, unsigned long long n = 1ull) {
    atomicAdd(&g_exp_count[i], n);
}
// spa_general: t(g) overshot the record's interval [4], by how much [18..23]
__device__ __forceinline__ void exp_overshoot(double wl, double dtj) {
    exp_add(4);
    const double ov = fmax(-wl, wl - dtj) / dtj;
    exp_add(ov < 1e-12 ? 18 : ov < 1e-9 ? 19 : ov < 1e-6 ? 20 : ov < 1e-3 ? 21
            : ov < 1e-1 ? 22 : 23);
}
// spa_general: |y| < FAST_Y [5, 6] and its band [8..15]
__device__ __forceinline__ void exp_small_y(double ww) {
    exp_add(fabs(ww) * 18.4 <= 1.0 ? 5 : 6);
    const double ay = 1.0 / fabs(ww);
    exp_add(ay >= 153.0 ? 8 : ay >= 75.0 ? 9 : ay >= 48.0 ? 10 : ay >= 29.4 ? 11
            : ay >= 23.1 ? 12 : ay >= 20.3 ? 13 : ay >= 18.4 ? 14 : 15);
}
// the last chunk's barrier balance [24..26] from the waves' evaluation counts wv[NWAVE]
__device__ __forceinline__ void exp_chunk_balance(const int* wv) {
    int mx = 0, sm = 0;
    for (int w = 0; w < NWAVE; ++w) { mx = max(mx, wv[w]); sm += wv[w]; }
    exp_add(24, (unsigned long long)mx);
    exp_add(25, (unsigned long long)sm);
    exp_add(26);
}
// a wave evaluates a record [0] of `tile`
__device__ __forceinline__ void exp_record(int64_t tile) {
    exp_add(0);
    if (tile < 16384) atomicAdd(&g_exp_tile[tile], 1u);
}
// the evaluated record's class from its header: [32..35], [29], [37..39] (partial: the record
// covers the wave's bins only partly)
__device__ __forceinline__ void exp_record_class(uint32_t ha, bool partial) {
    exp_add(31 + min((int)hdr_jser(ha), 4));
    if (hdr_safe(ha)) exp_add(29);
    if (partial) exp_add(37);
    if (hdr_jser(ha) >= 3u) exp_add(38);
    if (!hdr_safe(ha)) exp_add(39);
}
// the cold block runs for a wave [16] with this many lanes [17]
template <int NB>
__device__ __forceinline__ void exp_cold(const bool (&need)[NB], int lane) {
    unsigned long long nl = 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) nl += __popcll(__ballot(need[i]));
    if (lane == 0) {
        exp_add(16);
        exp_add(17, nl);
    }
}
__device__ __forceinline__ void exp_tile_clock(int64_t tile, unsigned long long t_start) {
    if (tile < 16384)
        g_exp_tclk[tile] = ((t_start & 0xffffffffull) << 32) |
                           ((wall_clock64() - t_start) & 0xffffffffull);
}
#else
#define EFD_EXP_DO(...)
#endif

// General (cold) path: scipy interval selection for t(g) and the full K_{1/3} evaluation.
// Returns W and both group amplitudes at t(g), the own bin's first (b[0], b[1]: the staged
// record's b[0]; from the spline coefficients, Bp for s = 0 and Bm for s = 1).
struct ColdEval {
    double wr, wi, b[4];
};
template <int CAUSTIC>
__device__ __noinline__ ColdEval spa_general(const Item* __restrict__ it, double g, int s, int h,
                                             int jrec,
                                             const double* __restrict__ t, int nt, int K,
                                             const int32_t* __restrict__ gm,
                                             const int32_t* __restrict__ gn,
                                             const double* __restrict__ coefA,
                                             const double* __restrict__ coefT) {
    const double u = g - it->gx;
    const double tt = fma(fma(fma(it->ic[0], u, it->ic[1]), u, it->ic[2]), u, it->ic[3]);
    double ph, fd, fdd;
    ColdEval c;
    const double wl = tt - it->tj;
    if (wl >= 0.0 && wl < it->dtj) {
        const double w = wl;
        for (int q = 0; q < 4; ++q) c.b[q] = cubic(it->b[q >> 1][q & 1], w);
        ph = fma(fma(fma(it->ph[0], w, it->ph[1]), w, it->ph[2]), w, it->ph[3]);
        fd = fma(fma(it->fd[0], w, it->fd[1]), w, it->fd[2]);
        fdd = INV_FDD_SCALE * fma(fma(it->fdd[0], w, it->fdd[1]), w, it->fdd[2]);
    } else {  // t(g) overshot the record's knot interval: evaluate like scipy
        EFD_EXP_DO(exp_overshoot(wl, it->dtj);)
        const FwdEval fe = forward_generic(tt, t, nt, jrec, h, K, gm[h], gn[h], coefA, coefT);
        for (int q = 0; q < 4; ++q) c.b[q] = fe.b[s ? q ^ 2 : q];
        ph = fe.ph; fd = fe.fd; fdd = fe.fdd;
    }
    const double amp = fd != 0.0 ? rsqrt(fabs(fd)) : 0.0;
    const double psi = fma(TWO_PI * g, tt, -ph) + (fd > 0.0 ? 0.75 * PI : -0.75 * PI);
    double R = 1.0, I = 0.0;
    if (CAUSTIC == EFD_CAUSTIC_UNIFORM && fd != 0.0 && fdd != 0.0) {
        const double a2 = amp * amp;
        const double a6 = a2 * a2 * a2;
        const double ww = (fd > 0.0 ? 1.0 : -1.0) * (3.0 / TWO_PI) * fdd * fdd * a6;
        if (fabs(ww) * FAST_Y <= 1.0) {
            kseries_fast(ww, R, I);
        } else {
            EFD_EXP_DO(exp_small_y(ww);)
            kfactor_slow(fd, fdd, R, I);
        }
    }
    double sn, cs;
    sincos_big(psi, sn, cs);
    c.wr = amp * (R * cs - I * sn);
    c.wi = amp * (R * sn + I * cs);
    return c;
}

// Accumulation of one evaluation into the lane's two bins. X is the own bin's group amplitude
// (b[S]), Z the mirror's (b[1-S]):
//   S = 0: own += X W,        mirror += conj(Z W)   (parent at f = -g, partner at the mirror)
//   S = 1: own += conj(X W),  mirror += Z W
template <int S, bool PAIRED>
__device__ __forceinline__ void accumulate(double wr, double wi, double xr, double xi, double zr,
                                           double zi, double& own_r, double& own_i,
                                           double& mir_r, double& mir_i) {
    own_r = fma(xr, wr, own_r);
    own_r = fma(-xi, wi, own_r);
    own_i = fma(S ? -xr : xr, wi, own_i);
    own_i = fma(S ? -xi : xi, wr, own_i);
    if (PAIRED) {
        mir_r = fma(zr, wr, mir_r);
        mir_r = fma(-zi, wi, mir_r);
        mir_i = fma(S ? zr : -zr, wi, mir_i);
        mir_i = fma(S ? zi : -zi, wr, mir_i);
    }
}

// One 16-B LDS-DMA piece per lane: global src (per lane) -> LDS dst (wave-uniform base + 16 B x
// lane). Issued through inline asm: the compiler's waitcnt pass treats the
// intrinsic's LDS write as possibly aliasing later ds_reads, so each wave waited for its prefetch
// of the next stage at the first record of every chunk (s_waitcnt vmcnt at the loop head). Hidden
// from that pass, the DMA is retired only by the explicit vmcnt(0) before each chunk barrier and
// at the end of the cold block (whose spill reloads would otherwise leave a vmcnt wait at the
// loop head): bitwise the same spectrum, ratio 1.005 (CI 1.002-1.015, 8 rounds). Round 1 measured
// the same idea as neutral (1.148 vs 1.14 ms) while the cold block's reloads still kept a vmcnt
// wait at the loop head. M0 (the DMA's LDS base) is set inside the asm: the k_modesum instances
// have no other M0 user (checked in their ISA), hence the local -Winline-asm silence.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void glds16(const uint4* src, uint4* dst) {
    const uint32_t base = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)(dst));
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                 :
                 : "v"(src), "s"(base)
                 : "memory", "m0");
}
#pragma clang diagnostic pop

// ----------------------------------------------------------------------------------------
// K8: the mode sum. One workgroup (4 waves) per tile of TILE * BPL frequency bins ("lanes");
// wave w owns the contiguous chunk [tile_base + w*64*BPL, +64*BPL) and lane l its bins
// chunk + 64 i + l (i < BPL). The tile's list of interval records is sorted in LDS (fixed
// summation order -> bitwise reproducible), then streamed through a double-buffered LDS stage:
// the whole workgroup streams the next NC records global -> LDS (global_load_lds, 16 B per lane)
// while the waves evaluate the current NC from LDS (broadcast reads; no dependent global latency
// in the loop).
// Each record feeds BPL independent, branch-free evaluations per lane (one per (m, n) group:
// every l of the group at once); lanes needing the general path get W = 0 there and add their
// term in a cold block. The sub-branch S of a record is wave-uniform: each S has its own copy of
// the evaluation (compile-time signs and LDS offsets).
// ----------------------------------------------------------------------------------------
// The tile's LDS, one object for every instantiation a kernel inlines (a kernel holding both the
// whole-tile and the sub-bin form of modesum_tile allocates it once, not twice)
struct TileLds {
    uint32_t keys[KEYCAP];
    Item stage[2][NC];
    int part[TILE];
    int hits[SEGWIN], hp0[SEGWIN], hcnt[SEGWIN], hoff[SEGWIN];
    int wcnt[(SEGWIN / TILE) * NWAVE];
    double2 sctab[SCTAB];   // (sin, cos)(k pi/128) for sincos_tab
    EFD_EXP_DO(int wimb[2][NWAVE];)   // records each wave evaluated in a chunk (barrier balance)
};
__device__ __forceinline__ TileLds& tile_lds() {
    __shared__ TileLds lds;
    return lds;
}

// The fused epilogue of a tile (the sum kernels' compile-time switch EPI): EPI_LL, the likelihood
// partial sum |d - h w|^2 at llpart[tile]; EPI_DH, the three partials of <d|h> and <h|h> (sum t_re,
// sum t_im, sum t_hh of dh_term) at llpart[s ntiles + tile], s = 0, 1, 2, where llpart is the
// waveform's [3][ntiles] slice of the caller's buffer (efd_modesum_sum_dh_hh)
constexpr int EPI_LL = 0, EPI_DH = 1;

template <bool PAIRED, int EPI>
__device__ __forceinline__ void tile_epilogue(
    double (&own_r)[BPL], double (&own_i)[BPL], double (&mir_r)[BPL], double (&mir_i)[BPL],
    int32_t w_lo, int lane, int wave, int tid, int64_t nlanes, int64_t nf, int64_t k0,
    int accumulate_out, double* __restrict__ out, double* __restrict__ hp,
    double* __restrict__ hc, const double* __restrict__ lld, const double* __restrict__ llw,
    double* __restrict__ llpart, int64_t tile, int64_t ntiles);

template <bool PAIRED, int CAUSTIC, int NB = BPL, int EPI = EPI_LL>
// 4 waves per SIMD (<= 128 VGPRs, 19 spilled, all outside the fast path's FMA chains): with
// 37.6 KB of LDS per workgroup 4 workgroups fit a CU, and the fourth wave hides more FP64
// latency than the spills cost (config 2: 1.00 ms against 1.09 ms at 3 waves / 147 VGPRs;
// 5 waves with a one-round stage: 1.07 ms)
#ifndef EFD_WAVES_PER_EU
#define EFD_WAVES_PER_EU 4
#endif
// 1: the tiles' record lists are built by k_tile_keys in the preparation phase and DMA'd in by
// the sum; tiles whose list needs more than one KEYCAP pass or has more than TK_HITS segments
// (tcnt = -1) build it in the sum as before. 0: always in the sum.
// sum dispatch order from k_tile_order: 0 = fixed (f = 0 outward), 1 = tiles longest first
__device__ __forceinline__ void modesum_tile(
    const Item* __restrict__ items, const int4* __restrict__ ranges,
    const int2* __restrict__ seglh, const int4* __restrict__ seginfo,
    const int32_t* __restrict__ nsegp, const double* __restrict__ freq, int64_t nf,
    int64_t nlanes, int64_t ntiles, int nt, int K, const int32_t* __restrict__ gm,
    const int32_t* __restrict__ gn, const double* __restrict__ t,
    const double* __restrict__ coefA, const double* __restrict__ coefT,
    const double2* __restrict__ sctab_g, const uint32_t* __restrict__ tkeys,
    const int32_t* __restrict__ tcnt, const int32_t* __restrict__ tperm,
    const int32_t* __restrict__ segbase, const int32_t* __restrict__ stb0,
    const int32_t* __restrict__ stb1, Header* __restrict__ hdr, int accumulate_out,
    double* __restrict__ out, double* __restrict__ hp, double* __restrict__ hc, int64_t k0,
    // fused likelihood (efd_modesum_sum_loglike; paired grids): d complex, w real [2][nf - k0];
    // the tile writes sum_c sum_j |d[c][j] - h_c[j] w[c][j]|^2 over its bins j >= k0 to
    // llpart[tile]. lld = NULL: not computed.
    const double* __restrict__ lld, const double* __restrict__ llw, double* __restrict__ llpart,
    // fused likelihood: the partial of a tile with no record (h = 0 on its bins), the same for
    // every walker (efd_loglike_tile_constants); NULL: such tiles compute it
    const double* __restrict__ llconst,
    int64_t b,     // b: this workgroup's place in the waveform's dispatch order
    bool direct = false,     // b is the tile itself (k_modesum_batch's sparse form)
    // NB < BPL: a split tile (k_segments_one's plan; sparse form), the sub-bin form. This
    // workgroup evaluates bins ioff .. ioff + NB - 1 of every lane (all of the tile's records, in
    // the whole tile's order, so each bin's sum is bitwise the whole tile's), stores them in the
    // tile's slot spart, and the last of the BPL / NB workgroups (arrival counter *scnt) loads
    // the slot and runs the epilogue
    int ioff = 0, double* __restrict__ spart = nullptr, int32_t* __restrict__ scnt = nullptr) {
    static_assert(NB == BPL || NB == 1, "sub-bin form: one bin per lane");
    TileLds& L_ = tile_lds();
    uint32_t* const keys = L_.keys;
    Item (*const stage)[NC] = L_.stage;
    int* const part = L_.part;
    int* const hits = L_.hits;
    int* const hp0 = L_.hp0;
    int* const hcnt = L_.hcnt;
    int* const hoff = L_.hoff;
    int* const wcnt = L_.wcnt;
    double2* const sctab = L_.sctab;
    EFD_EXP_DO(int (*const wimb)[NWAVE] = L_.wimb;)
    if (NB == BPL) ioff = 0;
    // Tile order. Blocks are dealt round-robin over the 8 XCDs; XCD x = b % 8 here gets groups
    // of XCD_GROUP consecutive tiles (neighbouring tiles share interval records, which then hit
    // in that XCD's L2) interleaved with the other XCDs' groups, so every XCD sees the same mix
    // of dense (low |f|) and empty (near Nyquist) tiles. The lane order runs from -Nyquist to
    // f = 0, so walking it backwards dispatches the dense band first and the cheap high-|f|
    // tiles last (short tail). The grid is padded to a multiple of 8 * XCD_GROUP.
    // With a cost order (tperm, k_tile_order) block b takes the b-th most expensive tile instead:
    // longest-first dispatch, so the launch does not end on expensive tiles started late;
    // consecutive blocks (similar cost) land on different XCDs.
    int64_t tile;
    if (direct) {
        tile = b;
    } else if (tperm != nullptr) {
        if (b >= ntiles) return;   // grid padding
        tile = tperm[b];
        if ((uint64_t)tile >= (uint64_t)ntiles) {
            // a corrupt or stale order entry: never index past the grid, and make
            // efd_modesum_status report it (the tile's bins would be left unwritten)
            if (threadIdx.x == 0) hdr->bad_tile = 1;
            return;
        }
    } else {
        // (the padded per-waveform grid, not gridDim: a batched launch holds several)
        const int64_t gq = 8 * XCD_GROUP, ngrid = (ntiles + gq - 1) / gq * gq;
        const int64_t r = b >> 3, grp = r / XCD_GROUP;
        const int64_t lin = (grp * 8 + (b & 7)) * XCD_GROUP + (r % XCD_GROUP);
        tile = ngrid - 1 - lin;
        if (tile >= ntiles) return;
    }
    EFD_EXP_DO(const unsigned long long t_start = wall_clock64();)
    // MODE.FP_DENORM[3:2] (FP64/FP16) = 0: flush denormal inputs and outputs (ftz_select). The
    // mode is per wave and set from the kernel descriptor at every wave launch.
    __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);   // hwreg(HW_REG_MODE, 6, 2)
    // MODE.IEEE = 0 (rsqrt_pos_sum's output modifier). Nothing here depends on IEEE mode's NaN
    // rules: the one min (fmin(|thn|, 1)) sees quiet NaNs at most and returns 1 in either mode.
    __builtin_amdgcn_s_setreg(1 | (9 << 6), 0);               // hwreg(HW_REG_MODE, 9, 1)
    // tid / lane are re-derived from tid0 through opq at the top of each loop and of the
    // epilogue, so nothing derived from them is live across the record loop's cold call (the
    // prologue's scratch stores of such values, 7 KB per wave, are gone)
    const int tid0 = threadIdx.x;
    int tid = tid0;
    int lane = tid & 63;
    const int ni = nt - 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform
    // Prebuilt record list: k_tile_keys, launched in the preparation phase, stored this tile's
    // keys when they fit in one KEYCAP pass (tcnt >= 0); they come in by LDS-DMA with the sin/cos
    // table and the build below is skipped. Same keys in the same order as the build below, so
    // the sum is bitwise the in-kernel build's.
    const int pre = tcnt != nullptr ? tcnt[tile] : -1;
    const int32_t tlo = (int32_t)(tile * TILE_LANES), thi = tlo + TILE_LANES;
    // a tile outside the union of the segments' lane ranges has no record: no list to build
    const int nseg = (pre < 0 && (hdr->lane_hi <= tlo || hdr->lane_lo >= thi))
                         ? 0 : *nsegp;
    // a tile that can have records (a prebuilt list, or segments to search): block-uniform. Tiles
    // without read neither their frequencies nor the sin/cos table
    const bool anyrec = pre > 0 || (pre < 0 && nseg > 0);
    bool seen = pre > 0;   // records evaluated (the fused likelihood's constant otherwise)
    // the (sin, cos) table: k_group's copy, global -> LDS by LDS-DMA (lane-linear pieces), with
    // a prebuilt list's keys
    static_assert(SCTAB % TILE == 0, "sin/cos table copy: whole rounds");
    if (anyrec) {
        if (pre > 0) {
            static_assert(KEYCAP % (4 * TILE) == 0, "key copy: whole rounds of 16-B pieces");
#pragma unroll
            for (int rd = 0; rd < KEYCAP / (4 * TILE); ++rd) {
                const int pc = rd * TILE + tid;                     // 16-B piece = 4 keys
                if (4 * pc < pre)
                    glds16(reinterpret_cast<const uint4*>(tkeys + (size_t)tile * KEYCAP) + pc,
                           reinterpret_cast<uint4*>(keys) + rd * TILE + wave * 64);
            }
        }
#pragma unroll
        for (int rd = 0; rd < SCTAB / TILE; ++rd)
            glds16(reinterpret_cast<const uint4*>(sctab_g) + rd * TILE + tid,
                   reinterpret_cast<uint4*>(sctab) + rd * TILE + wave * 64);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
        __syncthreads();
    }

    // ---- the tile's record list, built in LDS from the segment table (no global list, no
    // atomics). Segments are taken in windows of SEGWIN: (1) each thread tests SEGWIN/TILE
    // segments (strided, coalesced) for overlap with the tile, and a ballot compaction keeps the
    // hits in segment order; (2) one thread per hit bisects that segment's records for the
    // sub-range [p0, p0 + n) reaching into the tile; (3) a block scan places the keys. Keys go to
    // keys[] until KEYCAP, then the chunked evaluation below drains them. The summation order
    // (segment, then lane order) is fixed, so the result is bitwise reproducible.
    const int32_t w_lo = (int32_t)(tile * TILE_LANES + wave * 64 * BPL);
    // the bins this workgroup evaluates in the wave's chunk: [e_lo, e_hi), NB per lane
    const int32_t e_lo = w_lo + 64 * ioff;
    const int32_t e_hi = e_lo + 64 * NB;
    double fk[NB], tfk[NB];
    double own_r[NB], own_i[NB], mir_r[NB], mir_i[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int32_t k = e_lo + 64 * i + lane;
        fk[i] = (anyrec && k < nlanes) ? freq[k] : 0.0;
        tfk[i] = TWO_PI * fk[i];
        own_r[i] = own_i[i] = mir_r[i] = mir_i[i] = 0.0;
    }
    // Sub-branch sign state (wave-uniform): fk, tfk hold g = -+f, 2 pi g of the sub-branch s_cur
    // and own_i, mir_i hold sg * (the true sums), sg = -1 for s_cur = 1. A record of the other
    // sub-branch flips the 4 BPL registers in place (one v_xor each) instead of making signed
    // copies of fk, tfk, wi, wr for every record (16 VALU per record); negation commutes with
    // round-to-nearest, so the sums are bitwise those of the signed-copy form.
    int s_cur = 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) { fk[i] = -fk[i]; tfk[i] = -tfk[i]; }   // s = 0: g = -f

    // staging: a record is PIECES pieces of 16 B; NC records take at most ROUNDS pieces per thread.
    // The pieces go global -> LDS directly (gfx950 global_load_lds_dwordx4: no VGPR staging,
    // nothing held across the evaluation loop). The LDS destination of one wave-instruction is
    // a wave-uniform base + 16 B x lane, so piece p = round * TILE + 64 wave + lane of the chunk
    // lands at ((uint4*)stage[buf])[p], i.e. record p / PIECES, piece p % PIECES; its global
    // source is per lane.
    static_assert(PIECES * NC <= ROUNDS * TILE, "staging: at most ROUNDS 16-B pieces per thread");
#define EFD_GLDS(c, buf)                                                                      \
    do {                                                                                      \
        _Pragma("unroll") for (int rd_ = 0; rd_ < ROUNDS; ++rd_) {                            \
            const int p_ = rd_ * TILE + tid;                                                  \
            const int r_ = p_ / PIECES, q_ = p_ - r_ * PIECES;                                \
            if (r_ < NC && (c) * NC + r_ < cnt) {                                             \
                const uint32_t key_ = keys[(c) * NC + r_];                                    \
                /* sub-branch 1: b[0] and b[1] trade places in the stage, so the own bin's */ \
                /* amplitudes are always at b[0] (fixed LDS offsets in the hot loop) */       \
                const int qs_ = ((key_ & 1u) && q_ >= B_PIECE && q_ < B_PIECE + 8)            \
                                    ? ((q_ - B_PIECE + 4) & 7) + B_PIECE : q_;                \
                const uint4* src_ = reinterpret_cast<const uint4*>(items + (key_ >> 1)) + qs_; \
                uint4* dst_ = reinterpret_cast<uint4*>(&stage[(buf)][0]) + rd_ * TILE + wave * 64; \
                glds16(src_, dst_);                                                           \
            }                                                                                 \
        }                                                                                     \
    } while (0)

    int win = 0;        // next segment window
    int nhit = 0;       // overlapping segments of the current window
    int wtotal = 0;     // keys of the current window
    int wdone = 0;      // keys of the current window already written
    int nkeys = pre > 0 ? pre : 0;   // keys waiting in keys[]
    while (true) {
        // ---- fill keys[] (block-uniform control flow)
        while (pre < 0 && nkeys < KEYCAP) {
            tid = opq(tid0);
            lane = tid & 63;
            if (wdone == wtotal) {                 // need a new window of segments
                if (win >= nseg) break;
                // (1) overlap test + ordered compaction: every thread tests its SEGWIN/TILE
                // segments, one barrier publishes the per-(row, wave) counts
                constexpr int ROWS = SEGWIN / TILE;
                unsigned long long bal[ROWS];
#pragma unroll
                for (int row = 0; row < ROWS; ++row) {
                    const int sgi = win + row * TILE + tid;
                    bool hit = false;
                    if (sgi < nseg) hit = seg_hits_tile(seglh[sgi], tlo, thi);
                    bal[row] = __ballot(hit);
                    if (lane == 0) wcnt[row * NWAVE + wave] = __popcll(bal[row]);
                }
                __syncthreads();
                nhit = 0;
#pragma unroll
                for (int row = 0; row < ROWS; ++row) {
                    int before = nhit;
                    for (int w = 0; w < wave; ++w) before += wcnt[row * NWAVE + w];
                    if ((bal[row] >> lane) & 1ull) {
                        const unsigned long long below = bal[row] & ((1ull << lane) - 1ull);
                        hits[before + __popcll(below)] = win + row * TILE + tid;
                    }
#pragma unroll
                    for (int w = 0; w < NWAVE; ++w) nhit += wcnt[row * NWAVE + w];
                }
                __syncthreads();
                if (nhit == 0) {                   // nothing of this window reaches the tile
                    win += SEGWIN;
                    wtotal = wdone = 0;
                    continue;
                }
                win += SEGWIN;
                // (2) each hit segment's records reaching into the tile: [p0, p1) from the
                // segment-tile boundaries of k_seg_tiles, or by bisection
                for (int i = tid; i < nhit; i += TILE) {
                    const HitRecords hr = hit_records(hits[i], tile, tlo, thi, segbase, stb0,
                                                      stb1, seginfo, ranges);
                    hp0[i] = hr.p0;
                    hcnt[i] = hr.count;
                }
                __syncthreads();
                // (3) exclusive scan of the counts (serial per thread over a block of hits,
                // then the block scan of the threads' sums)
                const int hper = (nhit + TILE - 1) / TILE;
                const int h0 = min(nhit, tid * hper), h1 = min(nhit, h0 + hper);
                int mine = 0;
                for (int i = h0; i < h1; ++i) mine += hcnt[i];
                int run_off = block_excl_scan<NWAVE>(mine, part, lane, wave, wtotal);
                for (int i = h0; i < h1; ++i) { hoff[i] = run_off; run_off += hcnt[i]; }
                wdone = 0;
                __syncthreads();
                continue;
            }
            // write keys [wdone, wdone + take) of this window at keys[nkeys ...], scattered
            // (scatter_slot) over the take
            const int take = min(KEYCAP - nkeys, wtotal - wdone);
            for (int i = tid; i < nhit; i += TILE) {
                const int o = hoff[i], c = hcnt[i];
                const int lo = max(o, wdone), hi = min(o + c, wdone + take);
                if (lo >= hi) continue;
                const int4 info = seginfo[hits[i]];
                for (int g = lo; g < hi; ++g)
                    keys[nkeys + scatter_slot(g - wdone, take)] =
                        list_key(info, hp0[i] + (g - o));
            }
            nkeys += take;
            wdone += take;
            __syncthreads();
        }
        if (nkeys == 0) break;

        // ---- evaluate the nkeys records in chunks of NC through the double-buffered stage
        const int cnt = nkeys;
        const int nchunk = (cnt + NC - 1) / NC;
        seen = true;
        tid = opq(tid0);
        lane = tid & 63;
        EFD_GLDS(0, 0);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's LDS-DMA pieces landed
        __syncthreads();

        for (int c = 0; c < nchunk; ++c) {
            tid = opq(tid0);
            lane = tid & 63;
            // buffer (c+1)&1 was last read in chunk c-1, which every wave finished before the
            // barrier that closed it: chunk c+1's pieces stream in meanwhile
            if (c + 1 < nchunk) EFD_GLDS(c + 1, (c + 1) & 1);
            const int nin = (int)rfl((uint32_t)min(NC, cnt - c * NC));   // loop bound in an SGPR
            const Item* stg = stage[c & 1];
            // the chunk's record headers (hdr_pack), one lane per record, read from LDS once per
            // chunk; each record then takes one v_readlane
            uint32_t hdr = 0;
            if (lane < nin) {
                const uint32_t kl = keys[c * NC + lane];
                const int sl = (int)(kl & 1);
                const Item* il = stg + lane;
                const uint32_t lo = (uint32_t)min(max(il->klo[sl] - tlo, 0), TILE_LANES);
                const uint32_t hi = (uint32_t)min(max(il->khi[sl] - tlo, 0), TILE_LANES);
                hdr = hdr_pack(lo, hi, sl, il->jser, il->fdneg);
            }
            EFD_EXP_DO(int nev = 0; if (c > 0 && tid == 0) exp_chunk_balance(wimb[(c - 1) & 1]);)
            for (int ii = 0; ii < nin; ++ii) {
                const uint32_t ha = (uint32_t)__builtin_amdgcn_readlane((int)hdr, ii);
                const int s = hdr_s(ha);
                const int32_t klo = tlo + hdr_lo(ha);
                const int32_t khi = tlo + hdr_hi(ha);
                const Item* it = stg + ii;
                if (khi <= e_lo || klo >= e_hi) {              // misses this wave's bins
                    EFD_EXP_DO(if (lane == 0) exp_add(3);)
                    continue;
                }
                EFD_EXP_DO(++nev; if (lane == 0) exp_record(tile);)
                bool anyneed = false;
                bool need[NB];
                {
                    // one body: sub-branch sign (the register state above) and series length as
                    // wave-uniform values
                    EFD_EXP_DO(if (lane == 0 && s != s_cur) exp_add(36);)   // sub-branch flips
                    if (s != s_cur) {
#pragma unroll
                        for (int i = 0; i < NB; ++i) {
                            fk[i] = -fk[i];
                            tfk[i] = -tfk[i];
                            own_i[i] = -own_i[i];
                            mir_i[i] = -mir_i[i];
                        }
                        s_cur = s;
                    }
                    const int J = CAUSTIC == EFD_CAUSTIC_UNIFORM ? (int)hdr_jser(ha) : FAST_J;
                    // the stage holds b[s] at b[0] (EFD_GLDS swaps the halves for s = 1)
                    const double* xo = &it->b[0][0][0];
                    const double* xm = &it->b[1][0][0];
                    double wr[NB], wi[NB], w[NB];
                    uint64_t needm[NB], needany = 0;
                    const RecSign rs = rec_sign(hdr_fdneg(ha));
                    EFD_EXP_DO(if (lane == 0) exp_record_class(ha, e_lo < klo || khi < e_hi);)
                    // envelope records (series length field 0): the straight envelope body when
                    // the record covers the wave's whole chunk, else the same with a lane mask
                    if (CAUSTIC == EFD_CAUSTIC_UNIFORM && !hdr_test(ha, 7u << HDR_J)) {
                        if (!hdr_test((uint32_t)((e_lo - klo) | (khi - e_hi)) >> 31, 1u)) {
                            env_record<false, NB>(it, fk, tfk, sctab, rs, nullptr, wr, wi, w);
                        } else {
                            uint64_t am[NB];
#pragma unroll
                            for (int i = 0; i < NB; ++i) {
                                const int32_t base = e_lo + 64 * i;
                                am[i] = lane_range_mask(klo - base, khi - base);
                            }
                            env_record<true, NB>(it, fk, tfk, sctab, rs, am, wr, wi, w);
                        }
#pragma unroll
                        for (int i = 0; i < NB; ++i) need[i] = false;
                    } else
                    // certified safe, J <= 2 and covering the whole chunk: the straight-line
                    // evaluation (no lane masks, amplitude selects or series branch); the
                    // amplitude cubics and accumulation below are shared
                    if (CAUSTIC == EFD_CAUSTIC_UNIFORM &&
                        !hdr_test(((uint32_t)((e_lo - klo) | (khi - e_hi)) >> 31) |
                                  ((hdr_jser(ha) + 5u) >> 3) |
                                  (hdr_safe(ha) ^ 1u), 1u)) {
#pragma unroll
                        for (int i = 0; i < NB; ++i) {
                            spa_simple(it, fk[i], tfk[i], sctab, rs, wr[i], wi[i], w[i]);
                            need[i] = false;
                        }
                    } else
                    if (CAUSTIC == EFD_CAUSTIC_UNIFORM &&
                        !hdr_test(((uint32_t)((e_lo - klo) | (khi - e_hi)) >> 31) |
                                  (((hdr_jser(ha) ^ 3u) + 7u) >> 3) |
                                  (hdr_safe(ha) ^ 1u), 1u)) {
#pragma unroll
                        for (int i = 0; i < NB; ++i) {
                            spa_simple3(it, fk[i], tfk[i], sctab, rs, wr[i], wi[i], w[i]);
                            need[i] = false;
                        }
                    } else
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const int32_t base = e_lo + 64 * i;
                        const uint64_t am = lane_range_mask(klo - base, khi - base);
                        spa_fast_m<CAUSTIC>(it, fk[i], tfk[i], ha, am, sctab, rs,
                                            wr[i], wi[i], w[i], needm[i]);
                        need[i] = __builtin_amdgcn_inverse_ballot_w64(needm[i]);
                        needany |= needm[i];
                    }
                    anyneed = needany != 0;
                    // the own bins' amplitude cubics (b[0], 16 VGPRs) first, then the mirrors'
                    // (b[1], read after a compiler fence so they can reuse the registers)
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const double xr = cubic(xo, w[i]), xi = cubic(xo + 4, w[i]);
                        own_r[i] = fma(xr, wr[i], own_r[i]);
                        own_r[i] = fma(-xi, wi[i], own_r[i]);
                        own_i[i] = fma(xr, wi[i], own_i[i]);
                        own_i[i] = fma(xi, wr[i], own_i[i]);
                    }
                    if (PAIRED) {
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int i = 0; i < NB; ++i) {
                            const double zr = cubic(xm, w[i]), zi = cubic(xm + 4, w[i]);
                            mir_r[i] = fma(zr, wr[i], mir_r[i]);
                            mir_r[i] = fma(-zi, wi[i], mir_r[i]);
                            mir_i[i] = fma(-zr, wi[i], mir_i[i]);
                            mir_i[i] = fma(-zi, wr[i], mir_i[i]);
                        }
                    }
                    if (__builtin_expect(anyneed, 0)) {   // cold: general path, some lanes
                        EFD_EXP_DO(exp_cold(need, lane);)
                        const uint32_t key = rfl(keys[c * NC + ii]);
                        const int hg = (int)((key >> 1) / (uint32_t)ni);
                        const int jr = (int)((key >> 1) - (uint32_t)hg * (uint32_t)ni);
                        // the bins' g = -+f are reloaded from the grid around the calls (and
                        // fk, tfk after them), so they are not live across the calls: the
                        // caller-saved copies the kernel's prologue stored for every wave go
                        const int ln = opq(tid0) & 63;
#pragma unroll
                        for (int i = 0; i < NB; ++i) {
                            if (need[i]) {
                                const double f = freq[e_lo + 64 * i + ln];   // k < nlanes here
                                const ColdEval ce = spa_general<CAUSTIC>(
                                    it, s_cur ? f : -f, s, hg, jr, t, nt, K, gm, gn, coefA, coefT);
                                accumulate<0, PAIRED>(ce.wr, ce.wi, ce.b[0], ce.b[1], ce.b[2],
                                                      ce.b[3], own_r[i], own_i[i], mir_r[i],
                                                      mir_i[i]);
                            }
                        }
                        {
                            const int ln2 = opq(tid0) & 63;
#pragma unroll
                            for (int i = 0; i < NB; ++i) {
                                const int32_t k = e_lo + 64 * i + ln2;
                                const double f = k < nlanes ? freq[k] : 0.0;
                                fk[i] = s_cur ? f : -f;
                                tfk[i] = TWO_PI * fk[i];
                            }
                        }
                        // the cold block's reloads retired here, so the loop head needs no
                        // vmcnt wait (which would also wait for the hidden LDS-DMA)
                        __builtin_amdgcn_s_waitcnt(0x0f70);
                    }
                }
            }
            EFD_EXP_DO(if (lane == 0) wimb[c & 1][wave] = nev;)
            // retire this wave's LDS-DMA pieces, then the barrier publishes chunk c+1's stage
            __builtin_amdgcn_s_waitcnt(0x0f70);
            __syncthreads();
        }
        nkeys = 0;
        if (pre >= 0) break;   // a prebuilt list is the whole list
    }
#undef EFD_GLDS
    if constexpr (NB < BPL) {
        // the sub-bin form: this workgroup's bins (true signs) to the tile's slot, then the
        // arrival count (cdna_hip_programming.md's in-launch split-K reduction: plain stores ->
        // every wave's vmcnt(0) -> barrier -> lane 0 agent release -> vmcnt(0) -> relaxed agent
        // fetch_add; the last arriver: agent acquire -> vmcnt(0) -> barrier -> plain loads;
        // correct for any placement of the workgroups over XCDs and CUs). Each bin's sum is
        // complete here (all the tile's records, in its order): the slot is a handover, not a
        // reduction, so the spectrum is bitwise the whole tile's
        if (s_cur)
#pragma unroll
            for (int i = 0; i < NB; ++i) { own_i[i] = -own_i[i]; mir_i[i] = -mir_i[i]; }
        const int lt = opq(tid0);
        const int lw = lt >> 6, ll = lt & 63;
        double2* slot = reinterpret_cast<double2*>(spart);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int li = lw * 64 * BPL + 64 * (ioff + i) + ll;
            slot[2 * li] = make_double2(own_r[i], own_i[i]);
            slot[2 * li + 1] = make_double2(mir_r[i], mir_i[i]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (lt == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int arrived = __hip_atomic_fetch_add(scnt, 1, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
            const int last = arrived == BPL / NB - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                // re-armed for a later sum on the same preparation (k_segments_one zeroes it too)
                __hip_atomic_store(scnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            part[0] = last;   // "I am last", through an LDS array the tile already has
        }
        __syncthreads();
        if (!part[0]) return;
        const double2* s0 = reinterpret_cast<const double2*>(spart);
        double a_r[BPL], a_i[BPL], m_r[BPL], m_i[BPL];
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int li = lw * 64 * BPL + 64 * i + ll;
            const double2 a = s0[2 * li], m = s0[2 * li + 1];
            a_r[i] = a.x; a_i[i] = a.y; m_r[i] = m.x; m_i[i] = m.y;
        }
        tile_epilogue<PAIRED, EPI>(a_r, a_i, m_r, m_i, w_lo, ll, lw, lt, nlanes, nf, k0,
                                   accumulate_out, out, hp, hc, lld, llw, llpart, tile, ntiles);
    } else {
        if constexpr (EPI == EPI_DH) {
            if (PAIRED && !seen && out == nullptr && hp == nullptr) {
                // no record reached this tile: h = 0 on its bins, and every term of the three
                // sums is exactly 0 (w is finite), so the tile needs neither d nor w
                if (tid == 0) {
                    llpart[tile] = 0.0;
                    llpart[ntiles + tile] = 0.0;
                    llpart[2 * ntiles + tile] = 0.0;
                }
                return;
            }
        }
        if (PAIRED && llconst != nullptr && !seen && out == nullptr && hp == nullptr) {
            // no record reached this tile: h = 0 on its bins, whose likelihood partial is the
            // walker-independent one k_ll_tile_const computed with this epilogue's arithmetic
            if (tid == 0) llpart[tile] = llconst[tile];
            return;
        }
        if (s_cur)
#pragma unroll
            for (int i = 0; i < BPL; ++i) { own_i[i] = -own_i[i]; mir_i[i] = -mir_i[i]; }
        tid = opq(tid0);
        tile_epilogue<PAIRED, EPI>(own_r, own_i, mir_r, mir_i, w_lo, tid & 63, wave, tid, nlanes,
                                   nf, k0, accumulate_out, out, hp, hc, lld, llw, llpart, tile,
                                   ntiles);
    }
    EFD_EXP_DO(if (threadIdx.x == 0) exp_tile_clock(tile, t_start);)
}

// The tile's epilogue (whole tile, or the last arriver of a sub-bin split): the spectrum S,
// the symmetric grid's h+ / hx, and the fused likelihood's partial of the tile
template <bool PAIRED, int EPI>
__device__ __forceinline__ void tile_epilogue(
    double (&own_r)[BPL], double (&own_i)[BPL], double (&mir_r)[BPL], double (&mir_i)[BPL],
    int32_t w_lo, int lane, int wave, int tid, int64_t nlanes, int64_t nf, int64_t k0,
    int accumulate_out, double* __restrict__ out, double* __restrict__ hp,
    double* __restrict__ hc, const double* __restrict__ lld, const double* __restrict__ llw,
    double* __restrict__ llpart, int64_t tile, int64_t ntiles) {
    // S is written when out != NULL; on a symmetric grid h+ and hx of bins [k0, nf) are written
    // straight from the registers when hp != NULL (the lane holds S(k) and S(nf-1-k), the two
    // halves of efd_polarizations' flip), so the likelihood path never stores S
    double2* o = reinterpret_cast<double2*>(out);
    double2* php = reinterpret_cast<double2*>(hp);
    double2* phc = reinterpret_cast<double2*>(hc);
    double llacc = 0.0;   // fused likelihood: this lane's sum of |d - h w|^2
    double dh[3] = {0.0, 0.0, 0.0};   // EPI_DH: this lane's sums of t_re, t_im, t_hh
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int64_t k = w_lo + 64 * i + lane;
        if (k >= nlanes) continue;
        const int64_t km = PAIRED ? nf - 1 - k : k;
        double2 sk = make_double2(own_r[i], own_i[i]);
        double2 sm = make_double2(mir_r[i], mir_i[i]);
        if (PAIRED && km == k) {
            sk.x += sm.x;
            sk.y += sm.y;
            sm = sk;
        }
        if (o) {
            if (PAIRED && km != k) {
                double2 vm = sm;
                if (accumulate_out) { const double2 p = o[km]; vm.x += p.x; vm.y += p.y; }
                o[km] = vm;
            }
            double2 v = sk;
            if (accumulate_out) { const double2 p = o[k]; v.x += p.x; v.y += p.y; }
            o[k] = v;
        }
        if (PAIRED && (php || lld)) {
            // h+ = (a + conj b)/2, hx = i (a - conj b)/2 with a = S(j), b = S(nf-1-j)
            auto put = [&](int64_t j, double2 a, double2 b) {
                if (j < k0) return;
                double2 vp = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
                double2 vc = make_double2(-0.5 * (a.y + b.y), 0.5 * (a.x - b.x));
                if constexpr (EPI == EPI_DH) {
                    // h w with each component's product rounded (efd_loglike's rule), then the
                    // three written terms: no contraction
#pragma clang fp contract(off)
                    const int64_t q = j - k0, nb = nf - k0;
                    const double2 d0 = reinterpret_cast<const double2*>(lld)[q];
                    const double2 d1 = reinterpret_cast<const double2*>(lld)[nb + q];
                    const double w0 = llw[q], w1 = llw[nb + q];
                    dh_term(d0, make_double2(vp.x * w0, vp.y * w0), dh);
                    dh_term(d1, make_double2(vc.x * w1, vc.y * w1), dh);
                } else if (lld) {
                    // d - h w rounded like efd_loglike (product rounded, then difference: no
                    // contraction), so a template equal to the injection gives exactly 0
#pragma clang fp contract(off)
                    const int64_t q = j - k0, nb = nf - k0;
                    const double2 d0 = reinterpret_cast<const double2*>(lld)[q];
                    const double2 d1 = reinterpret_cast<const double2*>(lld)[nb + q];
                    const double w0 = llw[q], w1 = llw[nb + q];
                    const double r0 = d0.x - vp.x * w0, i0 = d0.y - vp.y * w0;
                    const double r1 = d1.x - vc.x * w1, i1 = d1.y - vc.y * w1;
                    llacc = fma(r0, r0, fma(i0, i0, llacc));
                    llacc = fma(r1, r1, fma(i1, i1, llacc));
                }
                if (!php) return;
                if (accumulate_out) {
                    const double2 pp = php[j - k0], pc = phc[j - k0];
                    vp.x += pp.x; vp.y += pp.y; vc.x += pc.x; vc.y += pc.y;
                }
                php[j - k0] = vp;
                phc[j - k0] = vc;
            };
            put(km, sm, sk);
            if (km != k) put(k, sk, sm);
        }
    }
    if constexpr (EPI == EPI_DH) {
        // the three partials in the likelihood partial's order (below)
        if (PAIRED && lld) {
            __shared__ double dhw4[3][NWAVE];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) dh[s] += __shfl_xor(dh[s], o, 64);
                if (lane == 0) dhw4[s][wave] = dh[s];
            }
            __syncthreads();
            if (tid < 3) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < NWAVE; ++w) t += dhw4[tid][w];
                llpart[tid * ntiles + tile] = t;
            }
        }
    } else if (PAIRED && lld) {
        // the tile's partial in a fixed order: a butterfly over each wave, then the waves in turn
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) llacc += __shfl_xor(llacc, o, 64);
        __shared__ double llw4[NWAVE];
        if (lane == 0) llw4[wave] = llacc;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) t += llw4[w];
            llpart[tile] = t;
        }
    }
}

// One prepared waveform as the sum sees it (sum_desc fills it): the workspace's buffers and the
// caller's arrays. k_modesum takes one by value, k_modesum_batch one per waveform (SumBatch).
struct SumDesc {
    const Item* items;
    const int4* ranges;
    const int2* seglh;
    const int4* seginfo;
    const int32_t* nseg;
    const double* freq;
    const int32_t* gm;
    const int32_t* gn;
    const double* t;
    const double* coefA;
    const double* coefT;
    const double2* sctab;
    const uint32_t* tkeys;
    const int32_t* tcnt;
    const int32_t* tperm;
    const int32_t* segbase;
    const int32_t* stb0;
    const int32_t* stb1;
    Header* hdr;
    double* out;
    double* hp;
    double* hc;
    double* llpart;
    int64_t k0;
    int32_t nt, K;
};
// The tile of waveform d: the one entry of the kernels into modesum_tile. The grid-wide values
// (nf, nlanes, ntiles, accumulate_out), the fused likelihood's data (lld, llw, llconst) and the
// tile's place (b, direct, ioff, spart, scnt) are the kernel's; the rest is unpacked here, into
// the restrict-qualified parameters the record loop's alias analysis works from. d comes by
// value: through a reference k_modesum_batch's sparse instances took up to 67 more SGPR spills
// and one a VGPR more; by value their registers, scratch and LDS are the explicit calls'.
template <bool PAIRED, int CAUSTIC, int NB = BPL, int EPI = EPI_LL>
__device__ __forceinline__ void modesum_tile(
    const SumDesc d, int64_t nf, int64_t nlanes, int64_t ntiles, int accumulate_out,
    const double* __restrict__ lld, const double* __restrict__ llw,
    const double* __restrict__ llconst, int64_t b, bool direct = false, int ioff = 0,
    double* __restrict__ spart = nullptr, int32_t* __restrict__ scnt = nullptr) {
    modesum_tile<PAIRED, CAUSTIC, NB, EPI>(
        d.items, d.ranges, d.seglh, d.seginfo, d.nseg, d.freq, nf, nlanes, ntiles, d.nt, d.K,
        d.gm, d.gn, d.t, d.coefA, d.coefT, d.sctab, d.tkeys, d.tcnt, d.tperm, d.segbase, d.stb0,
        d.stb1, d.hdr, accumulate_out, d.out, d.hp, d.hc, d.k0, lld, llw, d.llpart, llconst, b,
        direct, ioff, spart, scnt);
}

// K8: the mode sum (one workgroup per tile; prebuilt lists when tcnt is given)
template <bool PAIRED, int CAUSTIC, int BPL>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(EFD_WAVES_PER_EU, 8)))
void k_modesum(const SumDesc d, int64_t nf, int64_t nlanes, int64_t ntiles, int accumulate_out) {
    modesum_tile<PAIRED, CAUSTIC>(d, nf, nlanes, ntiles, accumulate_out, nullptr, nullptr,
                                  nullptr, (int64_t)blockIdx.x);
}

// K8 over a batch of prepared waveforms in one launch (efd_modesum_sum_batch): workgroup g takes
// waveform g mod n at place g / n of that waveform's dispatch order, so the waveforms' tiles
// interleave longest-first and one launch's ramp, tail and inter-launch gap are shared by n
// waveforms. Each waveform keeps its own workspace and outputs; its tiles run exactly the code of
// a single launch (bitwise the same spectrum). The per-waveform pointers travel in the kernel
// arguments (n <= EFD_BATCH_MAX), read with wave-uniform scalar loads. Config 2 (bench.py, 2
// rounds): 1,238 waveforms/s one sum per launch; 2 / 4 / 8 / 16 per launch 1,311 / 1,331 /
// 1,291 / 1,288 (k_modesum 0.781 -> 0.742 ms per waveform at 4; past 4 the concurrent
// waveforms' records outgrow the caches). Waveform-major order (each waveform's longest-first
// order in turn) measured 1,288 / 1,290 / 1,226 / 1,187.
struct SumBatch {
    SumDesc d[EFD_BATCH_MAX];
    int32_t n;
};
static_assert(sizeof(SumBatch) <= 3584, "batch descriptors must fit the kernel arguments");
// One waveform's logL from its tile partials p (with llconst: tiles outside the lane union take
// their constants): each thread's tiles i, i + 256, ... added in that order, then a tree; out =
// -1/2 * 4 * sum, or NaN when the workspace holds a device-side error flag (the flags stay set:
// efd_modesum_status_batch reports and clears them), so a caller that finds no NaN in the batch
// needs no status synchronisation. 256 threads. The same pass ends efd_modesum_sum_dh_hh's three
// sums: `sparse` says whether tiles outside the lane union take outside(i) (the constant; 0 for
// <d|h> and <h|h>) instead of p[i], and the sum is scaled by `scale`.
template <class Outside>
__device__ __forceinline__ void ll_final_reduce(const double* __restrict__ p,
                                                const Header* __restrict__ h, bool sparse,
                                                Outside outside, int64_t ntiles, double scale,
                                                double* __restrict__ out) {
    __shared__ double red[256];
    int64_t t0 = 0, t1 = ntiles - 1;
    if (sparse) {
        const int32_t lo = h->lane_lo, hi = h->lane_hi;
        t0 = lo < hi ? lo / TILE_LANES : ntiles;
        t1 = lo < hi ? (int64_t)(hi - 1) / TILE_LANES : -1;
    }
    auto val = [&](int64_t i) { return (i < t0 || i > t1) ? outside(i) : p[i]; };
    // four loads in flight at a time
    double acc = 0.0;
    int64_t i = threadIdx.x;
    for (; i + 3 * 256 < ntiles; i += 4 * 256) {
        const double v0 = val(i), v1 = val(i + 256), v2 = val(i + 512), v3 = val(i + 768);
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
    }
    for (; i < ntiles; i += 256) acc += val(i);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool bad = h->runs_overflow | h->bad_mn | h->bad_tile;
        *out = bad ? __longlong_as_double(0x7ff8000000000000LL) : scale * red[0];
    }
}
// SPARSE (the fused likelihood with tile constants, no written outputs): only the tiles inside the
// union of the waveform's segment lane ranges ([lane_lo, lane_hi) in its header, k_segment_compact)
// are visited, by nper workgroups per waveform striding over them; k_ll_final takes the constant
// of every tile outside. (Folding k_ll_final into the launch's last workgroup per waveform, with
// agent-scope partial stores and a completion count, made config 4's sum 6 us longer than the two
// kernels: the reduction then runs in the launch's tail.) A sparse spectrum (config 4: 15 harmonics cover 576 of 6,164 tiles) then
// launches a few hundred workgroups per walker instead of one per tile.
template <bool PAIRED, int CAUSTIC, int BPL, bool SPARSE, int EPI = EPI_LL>
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(EFD_WAVES_PER_EU, 8)))
void k_modesum_batch(const SumBatch batch, int64_t nf, int64_t nlanes, int64_t ntiles,
                     int accumulate_out, const double* __restrict__ lld,
                     const double* __restrict__ llw, const double* __restrict__ llconst,
                     int64_t nper) {
    const int n = batch.n;
    int w;
    int64_t pos;
    if (lld == nullptr) {
        w = (int)(blockIdx.x % (unsigned)n);
        pos = blockIdx.x / (unsigned)n;
    } else {
        // fused likelihood: the n waveforms of one dispatch place run back to back on one XCD
        // (workgroups are dealt round-robin over the 8 XCDs, x = g mod 8), so the tile's data
        // and weights (48 B per bin, the same for every walker) come from HBM once and from
        // that XCD's L2 for the other n - 1 walkers; place p*8 + x keeps each waveform's
        // place-to-XCD assignment that of a single launch
        const unsigned g = blockIdx.x, r = g >> 3;
        w = (int)(r % (unsigned)n);
        pos = (int64_t)(r / (unsigned)n) * 8 + (g & 7u);
    }
    const SumDesc& d = batch.d[w];
    if constexpr (SPARSE) {
        const int32_t nit = d.hdr->nitems;
        if (nit > 0) {
            // k_segments_one's split plan: items (tile, bin j, S, slot = counter); S = BPL: the
            // sub-bin form, one bin of every lane per workgroup
            const Layout L = make_layout(d.nt, d.K, nf, 1);
            char* W = reinterpret_cast<char*>(d.hdr);
            const int4* items = ws_at<const int4>(W, L.sitem);
            for (int64_t it = pos; it < nit; it += nper) {
                const int4 e = items[it];
                const int S = e.y & 0xffff, j = e.y >> 16;
                if (S > 1)
                    modesum_tile<PAIRED, CAUSTIC, 1, EPI>(
                        d, nf, nlanes, ntiles, accumulate_out, lld, llw, llconst, e.x, true, j,
                        ws_at<double>(W, L.spart) + (size_t)e.z * TILE_LANES * 4,
                        ws_at<int32_t>(W, L.scnt) + e.w);
                else
                    modesum_tile<PAIRED, CAUSTIC, BPL, EPI>(d, nf, nlanes, ntiles, accumulate_out,
                                                            lld, llw, llconst, e.x, true);
                __syncthreads();   // the next tile's LDS writes after every wave's last reads
            }
            return;
        }
        const int32_t lo = d.hdr->lane_lo, hi = d.hdr->lane_hi;
        if (lo < hi) {
            const int64_t t1 = min((int64_t)(hi - 1) / TILE_LANES, ntiles - 1);
            for (int64_t tile = lo / TILE_LANES + pos; tile <= t1; tile += nper) {
                modesum_tile<PAIRED, CAUSTIC, BPL, EPI>(d, nf, nlanes, ntiles, accumulate_out, lld,
                                                        llw, llconst, tile, true);
                __syncthreads();   // the next tile's LDS writes after every wave's last reads
            }
        }
        return;
    }
    modesum_tile<PAIRED, CAUSTIC, BPL, EPI>(d, nf, nlanes, ntiles, accumulate_out, lld, llw,
                                            llconst, pos);
}

// The fused likelihood's partial of a tile whose waveform has no record on it (every bin's
// h = 0): modesum_tile's epilogue with zero accumulators, the same operations in the same order,
// so a tile that takes it (llconst) gives bitwise what computing it would. Depends on the grid
// (nf, the paired tile layout), k0, d and w only: once per likelihood.
template <int BPL>
__global__ __launch_bounds__(TILE) void k_ll_tile_const(const double* __restrict__ lld,
                                                        const double* __restrict__ llw,
                                                        int64_t nf, int64_t nlanes, int64_t k0,
                                                        double* __restrict__ llconst) {
    const int64_t tile = blockIdx.x;
    // modesum_tile's FP modes, so the epilogue's arithmetic rounds the same
    __builtin_amdgcn_s_setreg(1 | (6 << 6) | (1 << 11), 0);
    __builtin_amdgcn_s_setreg(1 | (9 << 6), 0);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t w_lo = (int32_t)(tile * TILE_LANES + wave * 64 * BPL);
    double llacc = 0.0;
#pragma unroll
    for (int i = 0; i < BPL; ++i) {
        const int64_t k = w_lo + 64 * i + lane;
        if (k >= nlanes) continue;
        const int64_t km = nf - 1 - k;
        double2 sk = make_double2(0.0, 0.0);
        double2 sm = make_double2(0.0, 0.0);
        if (km == k) {
            sk.x += sm.x;
            sk.y += sm.y;
            sm = sk;
        }
        auto put = [&](int64_t j, double2 a, double2 b) {
            if (j < k0) return;
            double2 vp = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
            double2 vc = make_double2(-0.5 * (a.y + b.y), 0.5 * (a.x - b.x));
            {
#pragma clang fp contract(off)
                const int64_t q = j - k0, nb = nf - k0;
                const double2 d0 = reinterpret_cast<const double2*>(lld)[q];
                const double2 d1 = reinterpret_cast<const double2*>(lld)[nb + q];
                const double w0 = llw[q], w1 = llw[nb + q];
                const double r0 = d0.x - vp.x * w0, i0 = d0.y - vp.y * w0;
                const double r1 = d1.x - vc.x * w1, i1 = d1.y - vc.y * w1;
                llacc = fma(r0, r0, fma(i0, i0, llacc));
                llacc = fma(r1, r1, fma(i1, i1, llacc));
            }
        };
        put(km, sm, sk);
        if (km != k) put(k, sk, sm);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) llacc += __shfl_xor(llacc, o, 64);
    __shared__ double llw4[NWAVE];
    if (lane == 0) llw4[wave] = llacc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NWAVE; ++w) t += llw4[w];
        llconst[tile] = t;
    }
}

// Fused likelihood, second stage: waveform i's out[i] = -1/2 * 4 * (sum of its tiles' partials),
// one workgroup per waveform, fixed order (a strided pass per thread, then a tree)
struct LlBatch {
    const double* part[EFD_BATCH_MAX];
    const Header* hdr[EFD_BATCH_MAX];
    double* out;
    const double* llconst;   // sparse sum: the constants of the tiles outside each lane union
    int64_t ntiles;
    int32_t n;
};
// efd_modesum_status_batch: each workspace's error flags (bit 0 runs_overflow, 1 bad_mn,
// 2 bad_tile) into out[i], and the reported flags cleared (sticky until reported; see Header)
struct StatusBatch {
    Header* h[EFD_BATCH_MAX];
    int32_t n;
};
// efd_modesum_lane_ranges: each workspace's [lane_lo, lane_hi) (k_segment_compact's union of the
// segments' lane ranges) into out[2 i], out[2 i + 1]
__global__ __launch_bounds__(64) void k_lane_gather(const StatusBatch sb, int32_t* out) {
    const int i = threadIdx.x;
    if (i >= sb.n) return;
    out[2 * i] = sb.h[i]->lane_lo;
    out[2 * i + 1] = sb.h[i]->lane_hi;
}
__global__ __launch_bounds__(64) void k_status_gather(const StatusBatch sb, int32_t* out) {
    const int i = threadIdx.x;
    if (i >= sb.n) return;
    Header* h = sb.h[i];
    const int32_t f = (h->runs_overflow ? 1 : 0) | (h->bad_mn ? 2 : 0) | (h->bad_tile ? 4 : 0);
    out[i] = f;
    if (f) {
        h->runs_overflow = 0;
        h->bad_mn = 0;
        h->bad_tile = 0;
    }
}

__global__ __launch_bounds__(256) void k_ll_final(const LlBatch lb) {
    const double* llconst = lb.llconst;
    ll_final_reduce(lb.part[blockIdx.x], lb.hdr[blockIdx.x], llconst != nullptr,
                    [=](int64_t i) { return llconst[i]; }, lb.ntiles, -0.5 * 4.0,
                    lb.out + blockIdx.x);
}

// efd_modesum_sum_dh_hh, second stage: workgroup (i, s) turns sum s of waveform i, its ntiles
// partials at part[(3 i + s) ntiles ...], into out[3 i + s] = 4 * sum (NaN for all three of a
// waveform whose workspace holds an error flag). A sparse sum visited the lane union's tiles
// only, and the others' terms are exactly 0: they are never read.
struct DhBatch {
    const Header* hdr[EFD_BATCH_MAX];
    const double* part;
    double* out;
    int64_t ntiles;
    int32_t sparse;
};
__global__ __launch_bounds__(256) void k_dh_final(const DhBatch db) {
    const int64_t o = 3 * (int64_t)blockIdx.x + blockIdx.y;
    ll_final_reduce(db.part + o * db.ntiles, db.hdr[blockIdx.x], db.sparse != 0,
                    [](int64_t) { return 0.0; }, db.ntiles, 4.0, db.out + o);
}

// K6: the tiles' record lists, built in the preparation phase (k_modesum DMAs them in). The same
// keys in the same order as the sum's own build (segments in table order; each segment's records
// reaching the tile, [p0, p1) from the segment-tile boundaries or by bisection; the keys of each
// SEGWIN window of segment ids scattered by x -> P x mod n over that window), computed in one
// pass over the tile's hits instead of window by window: the segment table is read in batches
// of 8 windows per barrier, the hits' boundaries and counts in one round of loads, one block
// scan places them, and each thread then writes keys found by bisection over the hit offsets.
// The sum's build waits for every window's loads, scans and barriers in turn (~7.7 us per tile
// alone at config 2, 37 us for the launch); this kernel shares the GPU with the previous
// waveform's sum, so its resident time is what it costs. Tiles with more than TK_HITS hits or
// KEYCAP keys get tcnt = -1 and build in the sum.
constexpr int TK_HITS = TILE;
constexpr int TK_ROWS = 8;   // windows of the segment table per barrier
__device__ __forceinline__ void tile_keys_body(
    const int4* __restrict__ ranges, const int2* __restrict__ seglh,
    const int4* __restrict__ seginfo, const int32_t* __restrict__ nsegp,
    const int32_t* __restrict__ segbase, const int32_t* __restrict__ stb0,
    const int32_t* __restrict__ stb1, int64_t ntiles, uint32_t* __restrict__ tkeys,
    int32_t* __restrict__ tcnt) {
    static_assert(SEGWIN == TILE, "one segment per thread and window row");
    __shared__ int hits[TK_HITS], hp0[TK_HITS], hcnt[TK_HITS], hoff[TK_HITS], hws[TK_HITS],
        hwt[TK_HITS];
    __shared__ int4 hinfo[TK_HITS];
    __shared__ int wcnt[TK_ROWS * NWAVE];
    __shared__ int part[NWAVE];
    const int64_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t tlo = (int32_t)(tile * TILE_LANES), thi = tlo + TILE_LANES;
    const int nseg = *nsegp;
    // segment table size [27], hits per tile summed [28]
    EFD_EXP_DO(if (tile == 0 && tid == 0) exp_add(27, (unsigned long long)nseg);)
    // (1) the segments overlapping the tile, in table order
    int nhit = 0;
    for (int base = 0; base < nseg; base += TK_ROWS * TILE) {
        unsigned long long bal[TK_ROWS];
#pragma unroll
        for (int r = 0; r < TK_ROWS; ++r) {
            const int sgi = base + r * TILE + tid;
            bool hit = false;
            if (sgi < nseg) hit = seg_hits_tile(seglh[sgi], tlo, thi);
            bal[r] = __ballot(hit);
            if (lane == 0) wcnt[r * NWAVE + wave] = __popcll(bal[r]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TK_ROWS; ++r) {
            int before = nhit;
            for (int w = 0; w < wave; ++w) before += wcnt[r * NWAVE + w];
            if ((bal[r] >> lane) & 1ull) {
                const int pos = before + __popcll(bal[r] & ((1ull << lane) - 1ull));
                if (pos < TK_HITS) hits[pos] = base + r * TILE + tid;
            }
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) nhit += wcnt[r * NWAVE + w];
        }
        __syncthreads();
    }
    EFD_EXP_DO(if (tid == 0) exp_add(28, (unsigned long long)nhit);)
    if (nhit > TK_HITS) {
        if (tid == 0) tcnt[tile] = -1;
        return;
    }
    // (2) each hit's records reaching into the tile: [p0, p1)
    int c = 0;
    if (tid < nhit) {
        const int sg = hits[tid];
        const HitRecords hr = hit_records(sg, tile, tlo, thi, segbase, stb0, stb1, seginfo, ranges);
        c = hr.count;
        hp0[tid] = hr.p0;
        hcnt[tid] = c;
        hinfo[tid] = seginfo[sg];
    }
    // (3) exclusive scan of the counts
    int total;
    const int off = block_excl_scan<NWAVE>(c, part, lane, wave, total);
    if (total > KEYCAP) {
        if (tid == 0) tcnt[tile] = -1;
        return;
    }
    if (tid < nhit) hoff[tid] = off;
    __syncthreads();
    // (4) each hit's SEGWIN window: where its keys start and how many it holds (the scatter's
    // range). Hits are in table order, so a window's hits are consecutive: the window's start
    // is a max-scan of the offsets at window starts, its end a min-scan from the right of the
    // offsets past window ends
    {
        const int w = tid < nhit ? hits[tid] / SEGWIN : INT32_MAX;
        const bool first = tid < nhit && (tid == 0 || hits[tid - 1] / SEGWIN != w);
        const bool last = tid < nhit && (tid == nhit - 1 || hits[tid + 1] / SEGWIN != w);
        int st = first ? off : INT32_MIN;       // this hit's offset = hoff[tid]
        int en = last ? off + c : INT32_MAX;    // hoff[tid] + hcnt[tid]
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int vs = __shfl_up(st, o, 64), ve = __shfl_down(en, o, 64);
            if (lane >= o) st = max(st, vs);
            if (lane + o < 64) en = min(en, ve);
        }
        if (lane == 63) hws[wave] = st;   // wave carries (hws, hwt reused as scratch)
        if (lane == 0) hwt[wave] = en;
        __syncthreads();
        for (int v = 0; v < wave; ++v) st = max(st, hws[v]);
        for (int v = NWAVE - 1; v > wave; --v) en = min(en, hwt[v]);
        __syncthreads();
        if (tid < nhit) {
            hws[tid] = st;
            hwt[tid] = en - st;
        }
    }
    __syncthreads();
    // (5) the keys: position g of the list lies in hit i (bisection over the offsets)
    uint32_t* out = tkeys + (size_t)tile * KEYCAP;
    for (int g = tid; g < total; g += TILE) {
        int lo = 0, hi = nhit - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (hoff[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const int ws = hws[lo], take = hwt[lo];
        out[ws + scatter_slot(g - ws, take)] = list_key(hinfo[lo], hp0[lo] + (g - hoff[lo]));
    }
    if (tid == 0) tcnt[tile] = total;
}
__global__ __launch_bounds__(TILE) void k_tile_keys(const PrepBatch B) {
    PREP_WALKER(B);
    if (D.lists == 0) return;
    tile_keys_body(ws_at<int4>(W, L.ranges), ws_at<int2>(W, L.seglh), ws_at<int4>(W, L.seginfo),
                   ws_at<int32_t>(W, L.nseg), ws_at<int32_t>(W, L.segbase),
                   ws_at<int32_t>(W, L.stb0), ws_at<int32_t>(W, L.stb1), L.ntiles,
                   ws_at<uint32_t>(W, L.tkeys), ws_at<int32_t>(W, L.tcnt));
}

// K7: dispatch order for the sum, most expensive tiles first (longest-processing-time list
// scheduling). Cost = the tile's record count from k_tile_keys (tcnt; -1, a list over one
// KEYCAP pass, is the most expensive class), bucketed at quarter octaves: a counting sort in
// LDS by one workgroup. The order within a bucket follows LDS atomics and may vary from run to
// run; it changes only which block runs a tile, never a tile's arithmetic, so the spectrum is
// bitwise the same in every order.
constexpr int ORDER_BUCKETS = 64;
__device__ __forceinline__ int tile_cost_bucket(int32_t c) {
    if (c < 0) return ORDER_BUCKETS - 1;
    const float l = __log2f((float)c + 1.0f) * 4.0f;
    return min((int)l, ORDER_BUCKETS - 2);
}
// Wave-aggregated LDS atomic: the lanes of a wave holding the same bucket take one add by their
// lowest lane (a tile list's neighbours mostly share a bucket, so one add serves many lanes
// instead of a contended add per lane); returns the old value plus the lane's rank among them.
__device__ __forceinline__ int wave_bucket_add(int* hist, int bucket, bool valid) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    int res = 0;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int bl = __shfl(bucket, leader, 64);
        const unsigned long long same = __ballot(valid && bucket == bl) & todo;
        int base = 0;
        if (lane == leader) base = atomicAdd(&hist[bl], __popcll(same));
        base = __shfl(base, leader, 64);
        if ((same >> lane) & 1ull) res = base + __popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return res;
}
__device__ __forceinline__ void tile_order_body(const int32_t* __restrict__ tcnt,
                                                int64_t ntiles, int32_t* __restrict__ tperm) {
    __shared__ int hist[ORDER_BUCKETS];
    const int tid = threadIdx.x;
    if (tid < ORDER_BUCKETS) hist[tid] = 0;
    __syncthreads();
    // the first 16 x 1024 tiles' buckets stay in registers: one round of independent loads
    // instead of a dependent load-atomic chain per pass (the sort sits on the preparation
    // phase's critical path at small harmonic counts); every lane of a wave runs the same
    // number of passes (wave_bucket_add's ballots need the whole wave)
    constexpr int PER = 16;
    int bk[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int64_t i = tid + (int64_t)q * 1024;
        bk[q] = i < ntiles ? tile_cost_bucket(tcnt[i]) : -1;
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) wave_bucket_add(hist, bk[q], bk[q] >= 0);
    const int64_t npass = (ntiles + 1023) / 1024;
    for (int64_t p = PER; p < npass; ++p) {
        const int64_t i = tid + p * 1024;
        const int bkt = i < ntiles ? tile_cost_bucket(tcnt[i]) : 0;
        wave_bucket_add(hist, bkt, i < ntiles);
    }
    __syncthreads();
    if (tid == 0) {   // exclusive scan, most expensive bucket first
        int acc = 0;
        for (int q = ORDER_BUCKETS - 1; q >= 0; --q) { const int h = hist[q]; hist[q] = acc; acc += h; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int pos = wave_bucket_add(hist, bk[q], bk[q] >= 0);
        if (bk[q] >= 0) tperm[pos] = (int32_t)(tid + q * 1024);
    }
    for (int64_t p = PER; p < npass; ++p) {
        const int64_t i = tid + p * 1024;
        const int bkt = i < ntiles ? tile_cost_bucket(tcnt[i]) : 0;
        const int pos = wave_bucket_add(hist, bkt, i < ntiles);
        if (i < ntiles) tperm[pos] = (int32_t)i;
    }
}
__global__ __launch_bounds__(1024) void k_tile_order(const PrepBatch B) {
    PREP_WALKER(B);
    if (D.lists != 3) return;
    tile_order_body(ws_at<int32_t>(W, L.tcnt), L.ntiles, ws_at<int32_t>(W, L.tperm));
}

// ----------------------------------------------------------------------------------------
// K9: TD mode sum (FEW's InterpolatedModeSum [FEW-ext]; the reference's comparison path,
// check_mode_by_mode.py:85-99, 254-264). Sample-stationary: each
// thread owns TD_SPL samples t_i = i dt (strided by the block, so loads and stores coalesce).
// The (m, n) groups of k_group are walked in descending (m, n) order and, per m, summed by
// Horner's rule in z = e^{-i Phi_r}:
//   h(t) = - sum_m [ b_m P_m + conj(b_m Q_m) ],   b_m = e^{-i (m Phi_phi + n0 Phi_r)},
//   P_m = sum_n Bp_mn(t) z^(n - n0),  Q_m = sum_n Bm_mn(t) z^(n - n0),  n0 = min n of m,
// so a group costs its four amplitude cubics and two complex multiply-adds (20 FP64 FMAs); a
// sample pays one sin/cos for z and one per distinct m. Bp, Bm are k_group_amp's group
// amplitudes (they carry -scale Y+ and conj(-scale Y-): hence the leading minus, and the
// partner term conj(Bm e^{-i Phi}) = scale Y- conj(A) e^{+i Phi}). A gap in n multiplies by z
// once more per missing n. The knot interval is wave-uniform except in the few waves that
// straddle a knot; those read the amplitude coefficients per lane.
// ----------------------------------------------------------------------------------------
constexpr int TD_THREADS = 256;
constexpr int TD_SPL = 4;   // samples per thread

// scipy's interval choice: i with t_i <= x < t_{i+1}, clamped to [0, nt - 2]
__device__ __forceinline__ int knot_interval(const double* __restrict__ t, int nt, double x) {
    int lo = 0, hi = nt - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// WIN: the store epilogue multiplies each sample by window[s] (efd_td_modesum_windowed; the
// sum above it is the same code in both instantiations)
template <bool WIN>
__global__ __launch_bounds__(TD_THREADS) void k_td_modesum(
    const double* __restrict__ t, int nt, const double* __restrict__ coefT,
    const double* __restrict__ coefA, const int32_t* __restrict__ gm,
    const int32_t* __restrict__ gn, int K, const Header* __restrict__ hdr, double dt,
    int64_t ns, int accumulate_out, double* __restrict__ out, double* __restrict__ hp,
    double* __restrict__ hc, const double* __restrict__ window) {
    const int64_t s_base = (int64_t)blockIdx.x * (TD_THREADS * TD_SPL) + threadIdx.x;
    const double t_end = t[nt - 1];
    const int G = hdr->groups;
    double w[TD_SPL], pphi[TD_SPL], pr[TD_SPL], zr[TD_SPL], zi[TD_SPL];
    int jj[TD_SPL];
    bool valid[TD_SPL];
    bool any_valid = false;
#pragma unroll
    for (int i = 0; i < TD_SPL; ++i) {
        const int64_t s = s_base + (int64_t)i * TD_THREADS;
        const double ts = (double)s * dt;
        valid[i] = s < ns && ts <= t_end;
        any_valid |= valid[i];
        // samples past the end share the last interval, keeping the wave uniform there
        jj[i] = valid[i] ? knot_interval(t, nt, ts) : nt - 2;
        w[i] = valid[i] ? ts - t[jj[i]] : 0.0;
        const double* ct = coefT + (size_t)jj[i] * 32;
        pphi[i] = fma(fma(fma(ct[0], w[i], ct[8]), w[i], ct[16]), w[i], ct[24]);
        pr[i] = fma(fma(fma(ct[1], w[i], ct[9]), w[i], ct[17]), w[i], ct[25]);
        double sn, cs;
        sincos_big(pr[i], sn, cs);
        zr[i] = cs;
        zi[i] = -sn;
    }
    double Hr[TD_SPL], Hi[TD_SPL];
#pragma unroll
    for (int i = 0; i < TD_SPL; ++i) Hr[i] = Hi[i] = 0.0;

    if (__any(any_valid) && G > 0) {
        const int j0 = (int)rfl((uint32_t)jj[0]);
        bool same = true;
#pragma unroll
        for (int i = 0; i < TD_SPL; ++i) same &= jj[i] == j0;
        const size_t row = (size_t)4 * 4 * K;   // doubles per interval of coefA
        auto run = [&](auto UNI) {
            constexpr bool U = decltype(UNI)::value;
            double Pr[TD_SPL], Pi[TD_SPL], Qr[TD_SPL], Qi[TD_SPL];
#pragma unroll
            for (int i = 0; i < TD_SPL; ++i) Pr[i] = Pi[i] = Qr[i] = Qi[i] = 0.0;
            auto flush = [&](int m, int n0) {
#pragma unroll
                for (int i = 0; i < TD_SPL; ++i) {
                    double sn, cs;
                    sincos_big(fma((double)m, pphi[i], (double)n0 * pr[i]), sn, cs);
                    const double br = cs, bi = -sn;   // b = e^{-i (m Phi_phi + n0 Phi_r)}
                    // b P + conj(b Q)
                    Hr[i] += (br * Pr[i] - bi * Pi[i]) + (br * Qr[i] - bi * Qi[i]);
                    Hi[i] += (br * Pi[i] + bi * Pr[i]) - (br * Qi[i] + bi * Qr[i]);
                    Pr[i] = Pi[i] = Qr[i] = Qi[i] = 0.0;
                }
            };
            int cur_m = gm[G - 1], nprev = gn[G - 1];
            for (int g = G - 1; g >= 0; --g) {
                const int m = gm[g], n = gn[g];
                int d = nprev - n;
                if (m != cur_m) {
                    flush(cur_m, nprev);
                    cur_m = m;
                    d = 1;   // P = Q = 0: the Horner step below reduces to P = Bp
                }
                nprev = n;
                for (; d > 1; --d) {   // missing n between two groups of this m
#pragma unroll
                    for (int i = 0; i < TD_SPL; ++i) {
                        const double a = Pr[i], b = Qr[i];
                        Pr[i] = fma(a, zr[i], -Pi[i] * zi[i]);
                        Pi[i] = fma(a, zi[i], Pi[i] * zr[i]);
                        Qr[i] = fma(b, zr[i], -Qi[i] * zi[i]);
                        Qi[i] = fma(b, zi[i], Qi[i] * zr[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < TD_SPL; ++i) {
                    const double* ca = coefA + (size_t)(U ? j0 : jj[i]) * row + 4 * g;
                    const double wi = w[i];
                    const double bpr = fma(fma(fma(ca[0], wi, ca[4 * K]), wi, ca[8 * K]), wi, ca[12 * K]);
                    const double bpi = fma(fma(fma(ca[1], wi, ca[4 * K + 1]), wi, ca[8 * K + 1]), wi, ca[12 * K + 1]);
                    const double bmr = fma(fma(fma(ca[2], wi, ca[4 * K + 2]), wi, ca[8 * K + 2]), wi, ca[12 * K + 2]);
                    const double bmi = fma(fma(fma(ca[3], wi, ca[4 * K + 3]), wi, ca[8 * K + 3]), wi, ca[12 * K + 3]);
                    // P = P z + Bp, Q = Q z + Bm
                    const double a = Pr[i], b = Qr[i];
                    Pr[i] = fma(a, zr[i], fma(-Pi[i], zi[i], bpr));
                    Pi[i] = fma(a, zi[i], fma(Pi[i], zr[i], bpi));
                    Qr[i] = fma(b, zr[i], fma(-Qi[i], zi[i], bmr));
                    Qi[i] = fma(b, zi[i], fma(Qi[i], zr[i], bmi));
                }
            }
            flush(cur_m, nprev);
        };
        if (__all(same)) run(std::integral_constant<bool, true>{});
        else run(std::integral_constant<bool, false>{});
    }

    double2* o = reinterpret_cast<double2*>(out);
#pragma unroll
    for (int i = 0; i < TD_SPL; ++i) {
        const int64_t s = s_base + (int64_t)i * TD_THREADS;
        if (s >= ns) continue;
        // h = h+ - i hx = -H (zero past the trajectory's end: pad_output)
        double vr = valid[i] ? -Hr[i] : 0.0, vi = valid[i] ? -Hi[i] : 0.0;
        if constexpr (WIN) {
            const double wv = window[s];
            vr *= wv;
            vi *= wv;
        }
        if (o) {
            double2 v = make_double2(vr, vi);
            if (accumulate_out) { const double2 p = o[s]; v.x += p.x; v.y += p.y; }
            o[s] = v;
        }
        if (hp) hp[s] = accumulate_out ? hp[s] + vr : vr;
        if (hc) hc[s] = accumulate_out ? hc[s] - vi : -vi;
    }
}

}  // namespace

// ========================================================================================
// Host side
// ========================================================================================

// Workgroup slots k_modesum has resident at once on the current device (CUs x workgroups per
// CU from the occupancy query), cached per device. A grid with no more tiles than that starts
// every tile together, so there is no dispatch order to choose and k_tile_order is skipped (it
// would only lengthen the preparation: config 5's 43-tile downsampled grid lost 5.7% of its rate
// to it). The kernels' shapes do not depend on the caustic mode or pairing.
static int64_t resident_tile_slots() {
    constexpr int MAX_DEV = 64;
    static std::atomic<int64_t> cache[MAX_DEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return 1024;
    int64_t v = cache[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, reinterpret_cast<const void*>(&k_modesum<true, EFD_CAUSTIC_UNIFORM, BPL>),
            TILE, 0) != hipSuccess || cus <= 0 || per_cu <= 0)
        return 1024;   // MI355X: 256 CUs x 4 workgroups (LDS-bound)
    v = (int64_t)cus * per_cu;
    cache[dev].store(v, std::memory_order_relaxed);
    return v;
}

// Longest-first dispatch (k_tile_order) for one waveform: only when its tiles outnumber the
// resident slots and it has at least ORDER_MIN_K harmonics. With few harmonics the tiles' record
// lists are short and even, and the sort's ~9 us on the preparation chain cost more than the
// order saved: configs 1 and 3 (tens of harmonics, 3,082 tiles) ran 7% faster without it
// (2,147 / 2,122 vs 2,023 / 1,944 and 8,182 / 8,231 vs 7,777 / 7,410 waveforms/s, two rounds),
// while config 2 (3,020 harmonics) keeps +0.2% (paired A/B, ratio 1.002, CI 1.001-1.003).
// prepare and sum see the same arguments, so they agree on whether tperm exists.
constexpr int32_t ORDER_MIN_K = 1024;
// Prebuilt tile lists (k_tile_keys) from LISTS_MIN_K harmonics up; below, the sum builds
// them itself (short lists: one window pass per tile). With tens of harmonics (eps = 1e-2) the
// in-sum build is cheaper than k_tile_keys' pass over every tile in the batched likelihood:
// config 4's walker groups (bench.py --likelihood, 3 interleaved pairs) 11,253 -> 13,416 logL/s;
// configs 1 / 3 (tools/configs.py, 2 interleaved pairs) 2,938 vs 2,897 and 8,166 vs 7,996
// waveforms/s (neutral), config 5 40,729 vs 39,648 (neutral); config 2 (3,020 harmonics) keeps
// the prebuilt lists.
constexpr int32_t LISTS_MIN_K = 1024;
// (the environment variable EFD_LISTS_MIN_K, read once per process, overrides it:
// a tuning knob; prepare and sum read the same value, so they agree on whether lists exist)
static int32_t lists_min_k() {
    static const int32_t v = [] {
        const char* e = std::getenv("EFD_LISTS_MIN_K");
        return e ? (int32_t)std::atoi(e) : LISTS_MIN_K;
    }();
    return v;
}
static bool use_prebuilt(int32_t K) { return K >= lists_min_k(); }
static bool use_cost_order(int64_t ntiles, int32_t K) {
    return use_prebuilt(K) && K >= ORDER_MIN_K && ntiles > resident_tile_slots();
}
int32_t efdhip::list_mode(int32_t K, int64_t ntiles) {
    return use_prebuilt(K) ? (use_cost_order(ntiles, K) ? 3 : 1) : 0;
}

// argument checks of efd_modesum / _prepare / _sum (phase as in modesum_impl)
int efdhip::check_modesum_args(const efd_modesum_args* a, const void* workspace, int phase) {
    if (!a || !workspace) return fail(EFD_ERR_ARG, "efd_modesum: NULL argument");
    if (!a->t || !a->phi_phi || !a->phi_r || !a->f_phi || !a->f_r || !a->amp || !a->m ||
        !a->n || !a->ylm_p || !a->ylm_m || !a->freq)
        return fail(EFD_ERR_ARG, "efd_modesum: NULL array");
    const bool pol = a->hp != nullptr || a->hc != nullptr;
    if (pol && (!a->hp || !a->hc || !a->grid_symmetric || a->k0 < 0 || a->k0 > a->nf))
        return fail(EFD_ERR_ARG, "efd_modesum: hp/hc need both pointers, a symmetric grid and "
                                 "0 <= k0 <= nf");
    if ((phase & 2) && !a->out && !pol)
        return fail(EFD_ERR_ARG, "efd_modesum: no output (out or hp/hc)");
    if (a->nt < 2 || a->nt > MAX_NT) return fail(EFD_ERR_ARG, "efd_modesum: nt out of range");
    if (a->K <= 0 || a->K > MAX_K) return fail(EFD_ERR_ARG, "efd_modesum: K out of range [1, 8192]");
    if (a->nf <= 0 || a->nf >= (int64_t)INT32_MAX)
        return fail(EFD_ERR_ARG, "efd_modesum: nf out of range");
    if (a->caustic != EFD_CAUSTIC_SPA && a->caustic != EFD_CAUSTIC_UNIFORM)
        return fail(EFD_ERR_ARG, "efd_modesum: unknown caustic mode");
    return EFD_OK;
}

// K6 for the preparation chain of emrifd_prepare.hip (prep_batch: its PrepBatch)
int efdhip::launch_tile_lists(const void* prep_batch, int64_t ntiles, bool any_lists,
                              bool any_order, hipStream_t st) {
    const PrepBatch& B = *static_cast<const PrepBatch*>(prep_batch);
    const unsigned nz = (unsigned)B.n;
    if (any_lists) {
        hipLaunchKernelGGL(k_tile_keys, dim3((unsigned)ntiles, 1, nz), dim3(TILE), 0, st, B);
        HIP_TRY(hipGetLastError());
    }
    if (any_order) {
        hipLaunchKernelGGL(k_tile_order, dim3(1, 1, nz), dim3(1024), 0, st, B);
        HIP_TRY(hipGetLastError());
    }
    return EFD_OK;
}

// The sum's descriptor of one prepared waveform: the workspace's buffers (its Layout L) and the
// caller's arrays
static SumDesc sum_desc(const efd_modesum_args* a, void* workspace, const Layout& L) {
    char* ws = (char*)workspace;
    const int32_t lists = efdhip::list_mode(a->K, L.ntiles);
    SumDesc d{};
    d.items = (const Item*)(ws + L.items);
    d.ranges = (const int4*)(ws + L.ranges);
    d.seglh = (const int2*)(ws + L.seglh);
    d.seginfo = (const int4*)(ws + L.seginfo);
    d.nseg = (const int32_t*)(ws + L.nseg);
    d.freq = a->freq;
    d.gm = (const int32_t*)(ws + L.gm);
    d.gn = (const int32_t*)(ws + L.gn);
    d.t = a->t;
    d.coefA = (const double*)(ws + L.coefA);
    d.coefT = (const double*)(ws + L.coefT);
    d.sctab = (const double2*)(ws + L.sctab);
    d.tkeys = (const uint32_t*)(ws + L.tkeys);
    d.tcnt = lists ? (const int32_t*)(ws + L.tcnt) : nullptr;
    d.tperm = lists == 3 ? (const int32_t*)(ws + L.tperm) : nullptr;
    d.segbase = (const int32_t*)(ws + L.segbase);
    d.stb0 = (const int32_t*)(ws + L.stb0);
    d.stb1 = (const int32_t*)(ws + L.stb1);
    d.hdr = (Header*)(ws + L.header);
    d.out = a->out;
    d.hp = a->hp;
    d.hc = a->hc;
    d.llpart = (double*)(ws + L.llpart);
    d.k0 = a->k0;
    d.nt = a->nt;
    d.K = a->K;
    return d;
}

// f(PAIRED, CAUSTIC) with the sum kernels' two template arguments as integral constants, for
// the grid's symmetry and the caustic mode of a call
template <class F>
static void for_sum_variant(bool paired, int caustic, F f) {
    using Uniform = std::integral_constant<int, EFD_CAUSTIC_UNIFORM>;
    using Spa = std::integral_constant<int, EFD_CAUSTIC_SPA>;
    if (paired) {
        if (caustic == EFD_CAUSTIC_UNIFORM) f(std::true_type{}, Uniform{});
        else f(std::true_type{}, Spa{});
    } else {
        if (caustic == EFD_CAUSTIC_UNIFORM) f(std::false_type{}, Uniform{});
        else f(std::false_type{}, Spa{});
    }
}

// the workspace's header once `stream` has drained (the status and statistics calls)
static int read_header(const void* workspace, void* stream, Header& h) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(&h, workspace, sizeof(Header), hipMemcpyDeviceToHost));
    return EFD_OK;
}

// the headers of `count` workspaces as the gather kernels' argument; fn names the caller
static int fill_status_batch(const char* fn, void* const* workspace, int32_t count,
                             StatusBatch& sb) {
    sb.n = count;
    for (int i = 0; i < count; ++i) {
        if (!workspace[i]) return fail(EFD_ERR_ARG, std::string(fn) + ": NULL workspace");
        sb.h[i] = (Header*)workspace[i];
    }
    return EFD_OK;
}

// The device-side error flags (k_status_gather's bits: 1 runs_overflow, 2 bad_mn, 4 bad_tile),
// first one set, as the status calls' code and message; `who` starts the message.
static int status_error(int32_t flags, const std::string& who) {
    if (flags & 1) return fail(EFD_ERR_ARG, who + "a harmonic has more than 8 monotonic runs");
    if (flags & 2) return fail(EFD_ERR_ARG, who + "|m| > 255 or |n| > 1023");
    return fail(EFD_ERR_HIP, who + "a tile dispatch-order entry was out of range (prepare/sum "
                                   "workspace mismatch?); bins were left unwritten");
}

// ========================================================================================
// C ABI
// ========================================================================================
extern "C" {

int efd_version(void) { return EFD_VERSION; }

// The sources' hash this library was compiled from (_build.source_id(), passed by _build.py as
// -DEFD_BUILD_ID), kept as a tagged string so the build can check an existing binary without
// loading it: a shipped .so is reused only when its tag matches the sources at hand.
#ifndef EFD_BUILD_ID
#define EFD_BUILD_ID "unversioned"
#endif
__attribute__((used)) static const char efd_build_tag[] = "EFD_BUILD_ID=" EFD_BUILD_ID;
const char* efd_build_id(void) { return efd_build_tag + 13; }

#ifdef EFD_EXP
int efd_exp_counters(unsigned long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_exp_count), sizeof(unsigned long long) * EXP_NCOUNT));
    return EFD_OK;
}
int efd_exp_tiles(unsigned int* out, unsigned long long* clk) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_exp_tile), sizeof(unsigned int) * 16384));
    HIP_TRY(hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_exp_tclk), sizeof(unsigned long long) * 16384));
    return EFD_OK;
}
#endif

int efd_last_error(char* buf, int len) {
    if (!buf || len <= 0) return EFD_ERR_ARG;
    std::snprintf(buf, (size_t)len, "%s", g_err.c_str());
    return EFD_OK;
}

size_t efd_modesum_workspace_bytes(int32_t nt, int32_t K, int64_t nf) {
    if (nt < 2 || nt > MAX_NT || K <= 0 || K > MAX_K || nf <= 0) return 0;
    return make_layout(nt, K, nf, 0).total;  // unpaired has the most tiles
}

// phase: 1 = prepare (K0-K6), 2 = sum (K8), 3 = both
static int modesum_impl(const efd_modesum_args* a, void* workspace, size_t workspace_bytes,
                        void* stream, int phase) {
    {
        const int rc = efdhip::check_modesum_args(a, workspace, phase);
        if (rc != EFD_OK) return rc;
    }
    const int paired = a->grid_symmetric ? 1 : 0;
    const Layout L = make_layout(a->nt, a->K, a->nf, paired);
    if (workspace_bytes < L.total)
        return fail(EFD_ERR_WORKSPACE, "efd_modesum: workspace too small (see efd_modesum_workspace_bytes)");

    hipStream_t st = (hipStream_t)stream;
    if (phase & 1) {
        const int rc = efdhip::prepare_batch("efd_modesum_prepare", &a, &workspace,
                                             &workspace_bytes, 1, stream);
        if (rc != EFD_OK) return rc;
    }
    // K8: mode sum
    if (phase & 2) {
        const int64_t gq = 8 * XCD_GROUP;
        const dim3 grid((unsigned)((L.ntiles + gq - 1) / gq * gq)), block(TILE);
        const int acc = a->accumulate ? 1 : 0;
        const SumDesc d = sum_desc(a, workspace, L);
        if (a->prof_begin) HIP_TRY(hipEventRecord((hipEvent_t)a->prof_begin, st));
        for_sum_variant(paired != 0, a->caustic, [&](auto P, auto C) {
            hipLaunchKernelGGL((k_modesum<decltype(P)::value, decltype(C)::value, BPL>), grid,
                               block, 0, st, d, a->nf, L.nlanes, L.ntiles, acc);
        });
        HIP_TRY(hipGetLastError());
        if (a->prof_end) HIP_TRY(hipEventRecord((hipEvent_t)a->prof_end, st));
    }
    return EFD_OK;
}

int efd_modesum(const efd_modesum_args* a, void* workspace, size_t workspace_bytes, void* stream) {
    return modesum_impl(a, workspace, workspace_bytes, stream, 3);
}

int efd_modesum_sum(const efd_modesum_args* a, void* workspace, size_t workspace_bytes,
                    void* stream) {
    return modesum_impl(a, workspace, workspace_bytes, stream, 2);
}

// efd_modesum_sum_batch, and efd_modesum_sum_loglike when d != NULL (paired grids: the tiles
// write their likelihood partials, k_ll_final turns each waveform's into out[i])
constexpr int64_t SPARSE_WG = 4096;   // workgroups of a sparse launch, all waveforms
// (EFD_SPARSE_WG overrides it: an experiment switch for paired A/B runs, read once)
static int64_t sparse_wg() {
    static const int64_t v = [] {
        const char* e = getenv("EFD_SPARSE_WG");
        const long long x = e ? atoll(e) : 0;
        return x >= 64 && x <= (1 << 20) ? (int64_t)x : SPARSE_WG;
    }();
    return v;
}
int sum_batch_impl(const char* fn, const efd_modesum_args* const* a, void* const* workspace,
                   const size_t* workspace_bytes, int32_t count, const double* d, const double* w,
                   double* llout, void* stream, const double* llconst = nullptr,
                   double* dhpart = nullptr, int32_t dhflags = 0) {
    // dhpart: efd_modesum_sum_dh_hh (the EPI_DH instances; llout = its [count][3], no constants)
    const std::string F(fn);
    if (!a || !workspace || !workspace_bytes)
        return fail(EFD_ERR_ARG, F + ": NULL argument");
    if (count < 1 || count > EFD_BATCH_MAX)
        return fail(EFD_ERR_ARG, F + ": count out of range [1, EFD_BATCH_MAX]");
    SumBatch batch{};
    batch.n = count;
    Layout L0{};
    for (int i = 0; i < count; ++i) {
        const efd_modesum_args* ai = a[i];
        // (the fused likelihood needs no written output)
        const int rc = efdhip::check_modesum_args(ai, workspace[i], d ? 0 : 2);
        if (rc != EFD_OK) return rc;
        if (ai->nf != a[0]->nf || (ai->grid_symmetric != 0) != (a[0]->grid_symmetric != 0) ||
            ai->caustic != a[0]->caustic || (ai->accumulate != 0) != (a[0]->accumulate != 0))
            return fail(EFD_ERR_ARG, F + ": nf, grid_symmetric, caustic and accumulate must agree "
                                         "across the batch");
        if (d && (!ai->grid_symmetric || ai->accumulate || ai->k0 != a[0]->k0 || ai->k0 < 0 ||
                  ai->k0 >= ai->nf))
            return fail(EFD_ERR_ARG, F + ": the fused likelihood needs a symmetric grid, "
                                         "accumulate = 0 and one 0 <= k0 < nf for the batch");
        const int paired = ai->grid_symmetric ? 1 : 0;
        const Layout L = make_layout(ai->nt, ai->K, ai->nf, paired);
        if (workspace_bytes[i] < L.total)
            return fail(EFD_ERR_WORKSPACE, F + ": workspace too small (see "
                                               "efd_modesum_workspace_bytes)");
        if (i == 0) L0 = L;
        batch.d[i] = sum_desc(ai, workspace[i], L);
        if (dhpart) batch.d[i].llpart = dhpart + (size_t)i * 3 * L.ntiles;
    }
    hipStream_t st = (hipStream_t)stream;
    // the sparse form (k_modesum_batch): the fused likelihood with tile constants, nothing
    // written, and in-kernel lists (below 1,024 harmonics: the sparse spectra; denser ones keep
    // the longest-first order over every tile)
    // (<d|h> and <h|h> need no constants: a tile without a record adds exactly 0)
    bool sparse = d != nullptr && (dhpart ? !(dhflags & 1) : llconst != nullptr) &&
                  a[0]->grid_symmetric;
    for (int i = 0; i < count && sparse; ++i)
        sparse = !a[i]->out && !a[i]->hp && !a[i]->hc &&
                 efdhip::list_mode(a[i]->K, L0.ntiles) == 0;
    const int64_t gq = 8 * XCD_GROUP;
    int64_t nper = 0;
    if (sparse) {
        // workgroups per waveform: a multiple of 8 (one XCD place each), ~SPARSE_WG in all. With
        // a possible split plan (K <= SEG1_MAX_K: k_segments_one; its item count is on the
        // device) the whole share, so every item of a plan gets its own workgroup (those past
        // the items exit at once)
        const int64_t cap = std::max<int64_t>(64, (sparse_wg() / count + 7) / 8 * 8);
        bool planned = true;
        for (int i = 0; i < count; ++i) planned = planned && a[i]->K <= SEG1_MAX_K;
        nper = planned ? cap : std::min<int64_t>((L0.ntiles + 7) / 8 * 8, cap);
    }
    const int64_t nblk = sparse ? nper * count : (L0.ntiles + gq - 1) / gq * gq * count;
    if (nblk > (int64_t)UINT32_MAX) return fail(EFD_ERR_ARG, F + ": grid too large");
    const dim3 grid((unsigned)nblk), block(TILE);
    const int acc = a[0]->accumulate ? 1 : 0;
    if (a[0]->prof_begin) HIP_TRY(hipEventRecord((hipEvent_t)a[0]->prof_begin, st));
    for_sum_variant(a[0]->grid_symmetric != 0, a[0]->caustic, [&](auto P, auto C) {
        constexpr bool PAIRED = decltype(P)::value;
        constexpr int CAUSTIC = decltype(C)::value;
        if constexpr (PAIRED) {
            if (dhpart) {
                if (sparse)
                    hipLaunchKernelGGL((k_modesum_batch<true, CAUSTIC, BPL, true, EPI_DH>), grid,
                                       block, 0, st, batch, a[0]->nf, L0.nlanes, L0.ntiles, acc, d,
                                       w, nullptr, nper);
                else
                    hipLaunchKernelGGL((k_modesum_batch<true, CAUSTIC, BPL, false, EPI_DH>), grid,
                                       block, 0, st, batch, a[0]->nf, L0.nlanes, L0.ntiles, acc, d,
                                       w, nullptr, (int64_t)0);
                return;
            }
        }
        if (sparse)
            hipLaunchKernelGGL((k_modesum_batch<PAIRED, CAUSTIC, BPL, true>), grid, block, 0, st,
                               batch, a[0]->nf, L0.nlanes, L0.ntiles, acc, d, w, llconst, nper);
        else
            hipLaunchKernelGGL((k_modesum_batch<PAIRED, CAUSTIC, BPL, false>), grid, block, 0, st,
                               batch, a[0]->nf, L0.nlanes, L0.ntiles, acc, d, w,
                               d ? llconst : nullptr, (int64_t)0);
    });
    HIP_TRY(hipGetLastError());
    if (dhpart) {
        DhBatch db{};
        for (int i = 0; i < count; ++i) db.hdr[i] = (const Header*)workspace[i];
        db.part = dhpart;
        db.out = llout;
        db.ntiles = L0.ntiles;
        db.sparse = sparse ? 1 : 0;
        hipLaunchKernelGGL(k_dh_final, dim3((unsigned)count, 3), dim3(256), 0, st, db);
        HIP_TRY(hipGetLastError());
    } else if (d) {
        LlBatch lb{};
        lb.n = count;
        lb.ntiles = L0.ntiles;
        for (int i = 0; i < count; ++i) {
            lb.part[i] = batch.d[i].llpart;
            lb.hdr[i] = (const Header*)workspace[i];
        }
        lb.out = llout;
        lb.llconst = sparse ? llconst : nullptr;
        hipLaunchKernelGGL(k_ll_final, dim3((unsigned)count), dim3(256), 0, st, lb);
        HIP_TRY(hipGetLastError());
    }
    if (a[0]->prof_end) HIP_TRY(hipEventRecord((hipEvent_t)a[0]->prof_end, st));
    return EFD_OK;
}

int efd_modesum_sum_batch(const efd_modesum_args* const* a, void* const* workspace,
                          const size_t* workspace_bytes, int32_t count, void* stream) {
    return sum_batch_impl("efd_modesum_sum_batch", a, workspace, workspace_bytes, count, nullptr,
                          nullptr, nullptr, stream);
}

int efd_modesum_sum_loglike(const efd_modesum_args* const* a, void* const* workspace,
                            const size_t* workspace_bytes, int32_t count, const double* d,
                            const double* w, double* out, void* stream) {
    if (!d || !w || !out) return fail(EFD_ERR_ARG, "efd_modesum_sum_loglike: NULL d, w or out");
    return sum_batch_impl("efd_modesum_sum_loglike", a, workspace, workspace_bytes, count, d, w,
                          out, stream);
}

int efd_modesum_sum_dh_hh(const efd_modesum_args* const* a, void* const* workspace,
                          const size_t* workspace_bytes, int32_t count, const double* d,
                          const double* w, double* part, int32_t flags, double* out,
                          void* stream) {
    if (!d || !w || !part || !out)
        return fail(EFD_ERR_ARG, "efd_modesum_sum_dh_hh: NULL d, w, part or out");
    return sum_batch_impl("efd_modesum_sum_dh_hh", a, workspace, workspace_bytes, count, d, w, out,
                          stream, nullptr, part, flags);
}

int64_t efd_loglike_tile_count(int64_t nf) {
    if (nf < 1) return 0;
    return make_layout(2, 1, nf, 1).ntiles;
}

int efd_loglike_tile_constants(const double* d, const double* w, int64_t nf, int64_t k0,
                               double* tile_const, void* stream) {
    if (!d || !w || !tile_const)
        return fail(EFD_ERR_ARG, "efd_loglike_tile_constants: NULL d, w or tile_const");
    if (nf < 1 || k0 < 0 || k0 >= nf)
        return fail(EFD_ERR_ARG, "efd_loglike_tile_constants: need nf >= 1 and 0 <= k0 < nf");
    const Layout L = make_layout(2, 1, nf, 1);
    if (L.ntiles > (int64_t)UINT32_MAX) return fail(EFD_ERR_ARG, "efd_loglike_tile_constants: grid too large");
    hipLaunchKernelGGL(k_ll_tile_const<BPL>, dim3((unsigned)L.ntiles), dim3(TILE), 0,
                       (hipStream_t)stream, d, w, nf, L.nlanes, k0, tile_const);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_modesum_sum_loglike_ex(const efd_modesum_args* const* a, void* const* workspace,
                               const size_t* workspace_bytes, int32_t count, const double* d,
                               const double* w, const double* tile_const, double* out,
                               void* stream) {
    if (!d || !w || !out)
        return fail(EFD_ERR_ARG, "efd_modesum_sum_loglike_ex: NULL d, w or out");
    return sum_batch_impl("efd_modesum_sum_loglike_ex", a, workspace, workspace_bytes, count, d,
                          w, out, stream, tile_const);
}

// One walker group of the fused likelihood in one call (Likelihood.get_ll's per-group host
// path, likelihood.py:246-274 callers): efd_stage_batch into pin, the copy to dbuf, staged_event
// recorded after it (the pinned buffer's reuse waits on it), efd_modesum_prepare_batch and
// efd_modesum_sum_loglike_ex in launches of EFD_BATCH_MAX walkers, all on `stream`: the five
// ctypes transitions and the argument handling of the Python steps in one.
int efd_fused_group(void* pin, size_t pin_bytes, void* dbuf, size_t dbuf_bytes, int32_t count,
                    const uint64_t* src, const int32_t* shape, const double* scale,
                    const efd_modesum_args* tmpl, efd_modesum_args* args,
                    void* const* workspace, const size_t* workspace_bytes, const double* d,
                    const double* w, const double* tile_const, double* out, void* staged_event,
                    void* stream, size_t* total) {
    if (count < 1 || !args || !workspace || !workspace_bytes || !d || !w || !out || !total)
        return fail(EFD_ERR_ARG, "efd_fused_group: bad arguments");
    const int rs = efd_stage_batch(pin, pin_bytes, (uint64_t)(uintptr_t)dbuf, count, src, shape,
                                   scale, tmpl, args, total);
    if (rs == EFD_ERR_WORKSPACE || (rs == EFD_OK && (!dbuf || *total > dbuf_bytes)))
        return EFD_ERR_WORKSPACE;   // the caller grows pin / dbuf to *total and calls again
    if (rs != EFD_OK) return fail(rs, "efd_fused_group: staging failed (efd_stage_batch)");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(dbuf, pin, *total, hipMemcpyHostToDevice, st));
    if (staged_event) HIP_TRY(hipEventRecord((hipEvent_t)staged_event, st));
    const efd_modesum_args* ap[EFD_BATCH_MAX];
    for (int32_t c0 = 0; c0 < count; c0 += EFD_BATCH_MAX) {
        const int32_t cnt = std::min<int32_t>(EFD_BATCH_MAX, count - c0);
        for (int32_t i = 0; i < cnt; ++i) ap[i] = &args[c0 + i];
        const int rc = efd_modesum_prepare_batch(ap, workspace + c0, workspace_bytes + c0, cnt,
                                                 stream);
        if (rc != EFD_OK) return rc;
    }
    for (int32_t c0 = 0; c0 < count; c0 += EFD_BATCH_MAX) {
        const int32_t cnt = std::min<int32_t>(EFD_BATCH_MAX, count - c0);
        for (int32_t i = 0; i < cnt; ++i) ap[i] = &args[c0 + i];
        const int rc = efd_modesum_sum_loglike_ex(ap, workspace + c0, workspace_bytes + c0, cnt,
                                                  d, w, tile_const, out + c0, stream);
        if (rc != EFD_OK) return rc;
    }
    return EFD_OK;
}

int efd_modesum_status(const void* workspace, void* stream) {
    if (!workspace) return fail(EFD_ERR_ARG, "efd_modesum_status: NULL workspace");
    Header h{};
    const int rc = read_header(workspace, stream, h);
    if (rc != EFD_OK) return rc;
    const int32_t flags = (h.runs_overflow ? 1 : 0) | (h.bad_mn ? 2 : 0) | (h.bad_tile ? 4 : 0);
    if (!flags) return EFD_OK;
    // reported once: clear the sticky flags (the stream is idle, so nothing races this)
    char* w = (char*)const_cast<void*>(workspace);
    HIP_TRY(hipMemset(w + offsetof(Header, runs_overflow), 0, sizeof(int32_t)));
    HIP_TRY(hipMemset(w + offsetof(Header, bad_mn), 0, 2 * sizeof(int32_t)));
    return status_error(flags, "efd_modesum: ");
}

int efd_modesum_lane_ranges(void* const* workspace, int32_t count, int32_t* out, void* stream) {
    if (!workspace || !out || count < 1 || count > EFD_BATCH_MAX)
        return fail(EFD_ERR_ARG, "efd_modesum_lane_ranges: NULL argument or count out of range "
                                 "[1, EFD_BATCH_MAX]");
    StatusBatch sb{};
    const int rc = fill_status_batch("efd_modesum_lane_ranges", workspace, count, sb);
    if (rc != EFD_OK) return rc;
    hipLaunchKernelGGL(k_lane_gather, dim3(1), dim3(64), 0, (hipStream_t)stream, sb, out);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

int efd_modesum_status_batch(void* const* workspace, int32_t count, int32_t* flags,
                             void* stream) {
    if (!workspace || count < 1 || count > EFD_BATCH_MAX)
        return fail(EFD_ERR_ARG, "efd_modesum_status_batch: NULL workspaces or count out of "
                                 "range [1, EFD_BATCH_MAX]");
    StatusBatch sb{};
    const int rc = fill_status_batch("efd_modesum_status_batch", workspace, count, sb);
    if (rc != EFD_OK) return rc;
    // one gather kernel writing into mapped host memory, one synchronisation: the flags of a
    // walker batch cost what one efd_modesum_status costs
    static std::mutex mu;
    static int32_t* host = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!host) HIP_TRY(hipHostMalloc((void**)&host, sizeof(int32_t) * EFD_BATCH_MAX,
                                     hipHostMallocMapped));
    int32_t* dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&dev, host, 0));
    hipLaunchKernelGGL(k_status_gather, dim3(1), dim3(64), 0, (hipStream_t)stream, sb, dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    int first = -1;
    for (int i = 0; i < count; ++i) {
        const int32_t f = ((volatile int32_t*)host)[i];
        if (flags) flags[i] = f;
        if (f && first < 0) first = i;
    }
    if (first < 0) return EFD_OK;
    return status_error(host[first],
                        "efd_modesum (waveform " + std::to_string(first) + " of the batch): ");
}

int efd_modesum_contributions(const void* workspace, int64_t* contributions, void* stream) {
    if (!workspace || !contributions) return fail(EFD_ERR_ARG, "NULL argument");
    Header h{};
    const int rc = read_header(workspace, stream, h);
    if (rc != EFD_OK) return rc;
    *contributions = h.contributions;
    return EFD_OK;
}

int efd_modesum_stats(const void* workspace, int64_t* contributions, int64_t* evaluations,
                      int32_t* groups, void* stream) {
    if (!workspace) return fail(EFD_ERR_ARG, "NULL argument");
    Header h{};
    const int rc = read_header(workspace, stream, h);
    if (rc != EFD_OK) return rc;
    if (contributions) *contributions = h.contributions;
    if (evaluations) *evaluations = h.evaluations;
    if (groups) *groups = h.groups;
    return EFD_OK;
}

int efd_modesum_env_evaluations(const void* workspace, int64_t* env_evaluations, void* stream) {
    if (!workspace || !env_evaluations) return fail(EFD_ERR_ARG, "NULL argument");
    Header h{};
    const int rc = read_header(workspace, stream, h);
    if (rc != EFD_OK) return rc;
    *env_evaluations = h.env_evaluations;
    return EFD_OK;
}

size_t efd_td_workspace_bytes(int32_t nt, int32_t K) {
    if (nt < 2 || nt > MAX_NT || K <= 0 || K > MAX_K) return 0;
    return make_td_layout(nt, K).total;
}

static int td_modesum_run(const efd_td_args* a, const double* window, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (!a || !workspace) return fail(EFD_ERR_ARG, "efd_td_modesum: NULL argument");
    if (!a->t || !a->phi_phi || !a->phi_r || !a->f_phi || !a->f_r || !a->amp || !a->m ||
        !a->n || !a->ylm_p || !a->ylm_m)
        return fail(EFD_ERR_ARG, "efd_td_modesum: NULL array");
    if (!a->out && !a->hp && !a->hc)
        return fail(EFD_ERR_ARG, "efd_td_modesum: no output (out, hp or hc)");
    if (a->nt < 2 || a->nt > MAX_NT) return fail(EFD_ERR_ARG, "efd_td_modesum: nt out of range");
    if (a->K <= 0 || a->K > MAX_K)
        return fail(EFD_ERR_ARG, "efd_td_modesum: K out of range [1, 8192]");
    if (a->nsamples <= 0 || a->nsamples > ((int64_t)1 << 40))
        return fail(EFD_ERR_ARG, "efd_td_modesum: nsamples out of range");
    if (!(a->dt > 0.0)) return fail(EFD_ERR_ARG, "efd_td_modesum: dt must be > 0");
    const TdLayout L = make_td_layout(a->nt, a->K);
    if (workspace_bytes < L.total)
        return fail(EFD_ERR_WORKSPACE,
                    "efd_td_modesum: workspace too small (see efd_td_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const Header* hdr = (const Header*)(ws + L.header);
    const double* coefA = (const double*)(ws + L.coefA);
    const double* coefT = (const double*)(ws + L.coefT);
    const int32_t* gm = (const int32_t*)(ws + L.gm);
    const int32_t* gn = (const int32_t*)(ws + L.gn);
    const int nt = a->nt, K = a->K;
    {
        const int rc = efdhip::td_prepare(a, workspace, st);   // groups and splines
        if (rc != EFD_OK) return rc;
    }
    const int64_t per_block = (int64_t)TD_THREADS * TD_SPL;
    const int64_t nblk = (a->nsamples + per_block - 1) / per_block;
    if (nblk > 0x7fffffffLL) return fail(EFD_ERR_ARG, "efd_td_modesum: too many samples");
    if (a->prof_begin) HIP_TRY(hipEventRecord((hipEvent_t)a->prof_begin, st));
    if (window)
        hipLaunchKernelGGL(k_td_modesum<true>, dim3((unsigned)nblk), dim3(TD_THREADS), 0, st, a->t,
                           nt, coefT, coefA, gm, gn, K, hdr, a->dt, a->nsamples,
                           a->accumulate ? 1 : 0, a->out, a->hp, a->hc, window);
    else
        hipLaunchKernelGGL(k_td_modesum<false>, dim3((unsigned)nblk), dim3(TD_THREADS), 0, st,
                           a->t, nt, coefT, coefA, gm, gn, K, hdr, a->dt, a->nsamples,
                           a->accumulate ? 1 : 0, a->out, a->hp, a->hc, (const double*)nullptr);
    HIP_TRY(hipGetLastError());
    if (a->prof_end) HIP_TRY(hipEventRecord((hipEvent_t)a->prof_end, st));
    return EFD_OK;
}

int efd_td_modesum(const efd_td_args* a, void* workspace, size_t workspace_bytes, void* stream) {
    return td_modesum_run(a, nullptr, workspace, workspace_bytes, stream);
}

int efd_td_modesum_windowed(const efd_td_args* a, const double* window, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return td_modesum_run(a, window, workspace, workspace_bytes, stream);
}

int efd_upload(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return EFD_OK;
    if (!dst || !src) return fail(EFD_ERR_ARG, "efd_upload: NULL pointer");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return EFD_OK;
}

int efd_download(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return EFD_OK;
    if (!dst || !src) return fail(EFD_ERR_ARG, "efd_download: NULL pointer");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return EFD_OK;
}

int efd_stream_order(void* src, void* const* dst, int32_t count) {
    if (count < 0 || (count > 0 && !dst))
        return fail(EFD_ERR_ARG, "efd_stream_order: need count >= 0 and a stream array");
    if (count == 0) return EFD_OK;
    // one event per thread and device, re-recorded each call: a wait already enqueued keeps the
    // record it saw (stream-wait semantics), so reuse never loosens an earlier ordering
    // The event belongs to the source stream's device (not the caller's current device, which
    // may have changed since the streams were made): created and recorded with that device
    // current, the caller's device restored afterwards.
    constexpr int MAX_DEV = 64;
    thread_local hipEvent_t ev[MAX_DEV] = {};
    int cur = 0, dev = 0;
    HIP_TRY(hipGetDevice(&cur));
    dev = cur;
    if (src) HIP_TRY(hipStreamGetDevice((hipStream_t)src, &dev));
    if (dev < 0 || dev >= MAX_DEV) return fail(EFD_ERR_ARG, "efd_stream_order: device index");
    if (dev != cur) HIP_TRY(hipSetDevice(dev));
    hipError_t e = hipSuccess;
    if (!ev[dev]) e = hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev[dev], (hipStream_t)src);
    for (int32_t i = 0; e == hipSuccess && i < count; ++i)
        if (dst[i] != src) e = hipStreamWaitEvent((hipStream_t)dst[i], ev[dev], 0);
    if (dev != cur) HIP_TRY(hipSetDevice(cur));
    HIP_TRY(e);
    return EFD_OK;
}

}  // extern "C"
