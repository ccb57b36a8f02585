// emrifd_modes_device.inc -- amplitudes and ModeSelector(eps) on the device for batched callers
// (included by emrifd_prepare.hip; efd_modes_select_batch, efd_modes_select_batch_weighted,
// efd_modes_workspace_bytes, efd_psd_eval).
//
// The device form of emrifd_modes.cpp / amplitude.py: at every trajectory knot the branch powers
// |A_k|^2 |Y_k|^2 (every mode) and |A_k|^2 |Y_{l,-m}|^2 (modes with m != 0) are sorted
// descending, a branch is kept while the sum before it is < (1 - eps) total, partner picks fold
// onto their +m mode and the union over the knots is the kept set. Three launches for up to
// EFD_BATCH_MAX walkers:
//   k_modes_select   one workgroup per (knot, walker): powers in registers, total by a block
//                    reduction, candidates above the floor eps total / np compacted into LDS and
//                    sorted there (bitonic, ties by branch index), one block scan for the cut;
//                    the knot's kept modes go out as one row of byte flags
//   k_modes_compact  one workgroup per walker: OR of the rows -> keep (ascending), nkeep, status
//                    and the kept modes' m, n, ylm
//   k_modes_amp      (knot, walker) x lanes over K: the kept modes' complex amplitudes [nt][K]
// Fixed-order reductions and scans, no atomics: bitwise reproducible. With teuk == NULL the
// amplitudes are the STAND-IN model of emrifd_modes.cpp (not FEW physics), in plain FP64.
//
// Noise-weighted selection (k_modes_select<true>): both branch powers of mode k at knot i are
// multiplied by 1 / S(|m_k f_phi[i] + n_k f_r[i]|) where the PSD table's S is finite and > 0 and
// by 0 elsewhere; one interval search and one cubic per (knot, mode). The table's breakpoints are
// staged in s_key, which nothing else uses until the candidates are compacted (no LDS added);
// -DEFD_MODES_PSD_L2 searches them through L2 instead. A weighted knot whose total is 0 or not
// finite keeps nothing. k_modes_select<false> is the unweighted kernel, unchanged.

#include <type_traits>

// the PSD table's evaluation, the text the host compiles too
#define EFD_HD __device__ inline
#include "emrifd_psd.h"
#undef EFD_HD

namespace {

constexpr int MODES_MAX = 4096;           // modes; 2 MODES_MAX branch powers at most
constexpr int MODES_NT = 1024;             // threads of k_modes_select and k_modes_compact
constexpr int MODES_PER = MODES_MAX / MODES_NT;   // modes per thread
constexpr int MODES_WAVES = MODES_NT / 64;
constexpr int MODES_MAX_KNOTS = 1024;      // the mode sum's own limit on nt
constexpr double MODES_LN10 = 2.302585092994045684017991454684364208;

struct ModesDesc {   // one walker
    const double* p;
    const double* e;
    const double* ylm_p;
    const double* ylm_m;
    const double* teuk;
    double eps;
    int32_t* keep;
    int32_t* nkeep;
    int32_t* status;
    double* amp;
    int64_t amp_cap;
    int32_t* m_out;
    int32_t* n_out;
    double* ylm_p_out;
    double* ylm_m_out;
    uint8_t* flags;   // workspace: [nt][stride] bytes, one row per knot
    int32_t nt;
    int32_t include_minus_m;
};

struct ModesBatch {
    const int32_t* l;
    const int32_t* m;
    const int32_t* n;
    const double* phase0;
    const double* jitter;
    int32_t nmodes;
    int32_t stride;   // bytes of one flag row (nmodes rounded up to 4)
    ModesDesc d[EFD_BATCH_MAX];
};

// the weighted selection's extra kernel argument: the PSD table and each walker's knot
// frequencies (both NULL: that walker is selected unweighted)
struct ModesWeights {
    const double* x;   // [n]
    const double* c;   // [4][n - 1]
    int32_t n;
    efd_modes_weight w[EFD_BATCH_MAX];
};
struct ModesNoWeights {};

__host__ __device__ inline int modes_stride(int nmodes) { return (nmodes + 3) & ~3; }

// |A_lmn(p, e)| of the stand-in model (emrifd_modes.cpp: magnitudes)
__device__ inline double standin_mag(int l, int m, int n, double jit, double p, double e) {
    const double invw = 1.0 / (0.35 + 2.2 * e);
    const double pe = 1.4 * e;
    const double lp = log10(10.0 / p);
    const double c1 = 0.42 * (l - 2.0) + 0.30 * (double)(l - m);
    const double decay = c1 + 0.60 * fabs((double)n - (double)m * pe) * invw;
    const double x = 0.5 * (l + 2.0) * lp + jit;
    return exp(MODES_LN10 * (x - 1.0 - decay)) + exp(MODES_LN10 * (x - 3.6 - 0.085 * decay));
}

// |A_k|^2 at knot i
__device__ inline double modes_power(const ModesBatch& B, const ModesDesc& d, int i, int k,
                                     double p, double e) {
    if (d.teuk) {
        const double* a = d.teuk + 2 * ((size_t)i * B.nmodes + k);
        return a[0] * a[0] + a[1] * a[1];
    }
    const double mg = standin_mag(B.l[k], B.m[k], B.n[k], B.jitter[k], p, e);
    return mg * mg;
}

__device__ inline double abs2(const double* y, int k) {
    return y[2 * k] * y[2 * k] + y[2 * k + 1] * y[2 * k + 1];
}

// sum of v over the block in a fixed order (lanes by halving shuffles, then the waves' sums in
// wave order), the same value in every thread; red: MODES_WAVES doubles of LDS
__device__ inline double modes_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();   // red's previous readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < MODES_WAVES; ++w) s += red[w];
    return s;
}

// exclusive prefix of v over the block's threads, in thread order (fixed association), and the
// block's total; red: MODES_WAVES values of LDS
template <class T>
__device__ inline T modes_block_excl(T v, T* red, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < MODES_WAVES; ++w) {
        if (w == wave) base = tot;
        tot += red[w];
    }
    *total = tot;
    return base + (inc - v);
}

// branch a sorts before branch b: the larger power, ties by the smaller branch index
__device__ inline bool modes_before(double ka, uint16_t ia, double kb, uint16_t ib) {
    return ka > kb || (ka == kb && ia < ib);
}

template <bool WT>
__global__ __launch_bounds__(MODES_NT) void k_modes_select(
    const ModesBatch B, const typename std::conditional<WT, ModesWeights, ModesNoWeights>::type W) {
    const ModesDesc& d = B.d[blockIdx.z];
    const int i = blockIdx.x;
    if (i >= d.nt) return;
    const int nm = B.nmodes, tid = threadIdx.x;
    __shared__ double s_key[2 * MODES_MAX];
    __shared__ uint16_t s_idx[2 * MODES_MAX];
    __shared__ uint8_t s_flag[MODES_MAX];
    __shared__ double s_red[MODES_WAVES];
    __shared__ int s_redi[MODES_WAVES];

    // branch powers of this thread's modes k = tid + j MODES_NT: the +m branch (index k) and,
    // for m != 0, the partner (index MODES_MAX + k; the order of numpy's nm + rank numbering)
    const double p = d.p[i], e = d.e[i];
    // this walker's knot frequencies when it is weighted (block-uniform)
    bool weighted = false;
    double f_phi = 0.0, f_r = 0.0;
    const double* psd_x = nullptr;
    if constexpr (WT) {
        const efd_modes_weight& wt = W.w[blockIdx.z];
        weighted = wt.f_phi != nullptr;
        if (weighted) {
            f_phi = wt.f_phi[i];
            f_r = wt.f_r[i];
#ifdef EFD_MODES_PSD_L2
            psd_x = W.x;
#else
            for (int q = tid; q < W.n; q += MODES_NT) s_key[q] = W.x[q];
            psd_x = s_key;
            __syncthreads();   // (s_key is next written after modes_block_sum's barriers)
#endif
        }
    }
    double pw[2 * MODES_PER];
    double part = 0.0;
    int npart = 0;
#pragma unroll
    for (int j = 0; j < MODES_PER; ++j) {
        const int k = tid + j * MODES_NT;
        pw[2 * j] = pw[2 * j + 1] = -1.0;   // absent: below every floor
        if (k < nm) {
            const double a2 = modes_power(B, d, i, k, p, e);
            double wk = 1.0;   // one weight per (knot, mode) serves both branches
            if constexpr (WT)
                if (weighted)
                    wk = efdpsd::psd_weight(psd_x, W.c, W.n, B.m[k], B.n[k], f_phi, f_r);
            pw[2 * j] = a2 * abs2(d.ylm_p, k);
            if constexpr (WT) pw[2 * j] *= wk;
            part += pw[2 * j];
            if (B.m[k] != 0) {
                pw[2 * j + 1] = a2 * abs2(d.ylm_m, k);
                if constexpr (WT) pw[2 * j + 1] *= wk;
                part += pw[2 * j + 1];
                ++npart;
            }
        }
        s_flag[k] = 0;
    }
    const double total = modes_block_sum(part, s_red);
    int np_ = 0;
    modes_block_excl(npart, s_redi, &np_);
    np_ += nm;
    if constexpr (WT) {
        // weighted only: nothing can be ranked at a knot whose total is 0 or not finite, so it
        // keeps nothing (block-uniform: total is the same value in every thread)
        if (weighted && !(isfinite(total) && total > 0.0)) {
            for (int k = tid; k < B.stride; k += MODES_NT) d.flags[(size_t)i * B.stride + k] = 0;
            return;
        }
    }
    const double need = total * (1.0 - d.eps);
    // the c-th largest of the kept top-c exceeds eps total / np (the np - c + 1 powers from it
    // down sum to more than eps total): only powers above half that floor are candidates (the
    // half absorbs the rounding of total). No candidate at all (every power equal, or zero):
    // every branch is one.
    double floor_ = 0.5 * d.eps * total / (double)np_;
    int nc = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 2 * MODES_PER; ++q) cnt += pw[q] > floor_ ? 1 : 0;
        int at = modes_block_excl(cnt, s_redi, &nc);
        if (nc == 0) {
            floor_ = -0.5;
            continue;
        }
#pragma unroll
        for (int q = 0; q < 2 * MODES_PER; ++q)
            if (pw[q] > floor_) {
                s_key[at] = pw[q];
                s_idx[at] = (uint16_t)((q & 1) * MODES_MAX + tid + (q >> 1) * MODES_NT);
                ++at;
            }
        break;
    }
    if (nc == 0) {   // NaN powers only: nothing can be ranked, the knot keeps nothing
        for (int k = tid; k < B.stride; k += MODES_NT) d.flags[(size_t)i * B.stride + k] = 0;
        return;
    }
    int n2 = 2;
    while (n2 < nc) n2 <<= 1;   // <= 2 MODES_MAX
    for (int q = nc + tid; q < n2; q += MODES_NT) {
        s_key[q] = -1.0;
        s_idx[q] = 0xffffu;
    }
    __syncthreads();
    // bitonic sort, descending in (power, -index)
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += MODES_NT) {
                const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
                const int hi = lo | jj;
                const double ka = s_key[lo], kb = s_key[hi];
                const uint16_t ia = s_idx[lo], ib = s_idx[hi];
                const bool up = (lo & kk) == 0;   // this run descends
                if (modes_before(kb, ib, ka, ia) == up) {
                    s_key[lo] = kb; s_key[hi] = ka;
                    s_idx[lo] = ib; s_idx[hi] = ia;
                }
            }
            __syncthreads();
        }
    // the cut: position c is kept when c = 0 or the sum of the c powers before it is < need.
    // Each thread owns `chunk` consecutive positions; one block scan gives its offset.
    const int chunk = (nc + MODES_NT - 1) / MODES_NT;
    const int c0 = min(nc, tid * chunk), c1 = min(nc, c0 + chunk);
    double mine = 0.0;
    for (int c = c0; c < c1; ++c) mine += s_key[c];
    double all;
    double before = modes_block_excl(mine, s_red, &all);
    for (int c = c0; c < c1; ++c) {
        if (c == 0 || before < need) s_flag[s_idx[c] & (MODES_MAX - 1)] = 1;
        before += s_key[c];
    }
    __syncthreads();
    for (int k = tid; k < B.stride; k += MODES_NT)
        d.flags[(size_t)i * B.stride + k] = k < nm ? s_flag[k] : 0;
}

__global__ __launch_bounds__(MODES_NT) void k_modes_compact(const ModesBatch B) {
    const ModesDesc& d = B.d[blockIdx.x];
    const int nm = B.nmodes, tid = threadIdx.x;
    __shared__ int s_redi[MODES_WAVES];
    // this thread's modes 4 tid .. 4 tid + 3 (MODES_PER = 4: one 32-bit word of every flag row)
    static_assert(MODES_PER == 4, "k_modes_compact reads one word of flags per thread");
    uint32_t any = 0;
    if (4 * tid < B.stride)
        for (int i = 0; i < d.nt; ++i)
            any |= *(const uint32_t*)(d.flags + (size_t)i * B.stride + 4 * tid);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += (any >> (8 * j)) & 0xff ? 1 : 0;
    int K = 0;
    int at = modes_block_excl(cnt, s_redi, &K);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * tid + j;
        if (!((any >> (8 * j)) & 0xff) || k >= nm) continue;
        d.keep[at] = k;
        d.m_out[at] = B.m[k];
        d.n_out[at] = B.n[k];
        d.ylm_p_out[2 * at] = d.ylm_p[2 * k];
        d.ylm_p_out[2 * at + 1] = d.ylm_p[2 * k + 1];
        d.ylm_m_out[2 * at] = d.include_minus_m ? d.ylm_m[2 * k] : 0.0;
        d.ylm_m_out[2 * at + 1] = d.include_minus_m ? d.ylm_m[2 * k + 1] : 0.0;
        ++at;
    }
    if (tid == 0) {
        *d.nkeep = K;
        *d.status = (d.amp && (int64_t)K * d.nt > d.amp_cap) ? EFD_MODES_AMP_OVERFLOW : 0;
    }
}

__global__ __launch_bounds__(256) void k_modes_amp(const ModesBatch B) {
    const ModesDesc& d = B.d[blockIdx.z];
    const int i = blockIdx.y;
    if (i >= d.nt || !d.amp) return;
    const int K = *d.nkeep;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int64_t at = (int64_t)i * K + j;
    if (j >= K || at >= d.amp_cap) return;   // (capacity too small: status says so)
    const int k = d.keep[j];
    double re, im;
    if (d.teuk) {
        const double* a = d.teuk + 2 * ((size_t)i * B.nmodes + k);
        re = a[0];
        im = a[1];
    } else {
        const double p = d.p[i], e = d.e[i];
        const int l = B.l[k], m = B.m[k], n = B.n[k];
        const double mg = standin_mag(l, m, n, B.jitter[k], p, e);
        const double ph = B.phase0[k] + (0.2 * (double)(l - m + 1) * (10.0 / p)
                                         + 0.1 * (double)n * e);
        re = mg * cos(ph);
        im = mg * sin(ph);
    }
    d.amp[2 * at] = re;
    d.amp[2 * at + 1] = im;
}

}  // namespace

extern "C" {

size_t efd_modes_workspace_bytes(int32_t nt, int32_t nmodes) {
    if (nt < 1 || nt > MODES_MAX_KNOTS || nmodes < 1 || nmodes > MODES_MAX) return 0;
    return (size_t)nt * modes_stride(nmodes);
}

}  // extern "C"

namespace {

// efd_modes_select_batch (wt == NULL) and efd_modes_select_batch_weighted
int modes_select(const char* fname, const efd_modes_table* tab, const efd_modes_walker* w,
                 const efd_modes_weight* wt, const efd_psd_table* psd, int32_t count,
                 void* stream) {
    const std::string F(fname);
    if (!tab || !w) return fail(EFD_ERR_ARG, F + ": NULL argument");
    if (count < 1 || count > EFD_BATCH_MAX)
        return fail(EFD_ERR_ARG, F + ": count out of range [1, EFD_BATCH_MAX]");
    if (!tab->l || !tab->m || !tab->n || !tab->phase0 || !tab->jitter)
        return fail(EFD_ERR_ARG, F + ": NULL mode table");
    if (tab->nmodes < 1 || tab->nmodes > MODES_MAX)
        return fail(EFD_ERR_ARG, F + ": nmodes out of range [1, 4096]");
    ModesWeights W{};
    if (wt) {
        if (!psd || !psd->x || !psd->c) return fail(EFD_ERR_ARG, F + ": NULL PSD table");
        if (psd->n < 2 || psd->n > MODES_MAX)
            return fail(EFD_ERR_ARG, F + ": PSD table n out of range [2, 4096]");
        W.x = psd->x; W.c = psd->c; W.n = psd->n;
        for (int i = 0; i < count; ++i) {
            if ((wt[i].f_phi == nullptr) != (wt[i].f_r == nullptr))
                return fail(EFD_ERR_ARG, F + ": f_phi and f_r are both set or both NULL");
            W.w[i] = wt[i];
        }
    }
    ModesBatch B{};
    B.l = tab->l; B.m = tab->m; B.n = tab->n; B.phase0 = tab->phase0; B.jitter = tab->jitter;
    B.nmodes = tab->nmodes;
    B.stride = modes_stride(tab->nmodes);
    int ntmax = 0;
    bool any_amp = false;
    for (int i = 0; i < count; ++i) {
        const efd_modes_walker& wi = w[i];
        if (!wi.p || !wi.e || !wi.ylm_p || !wi.ylm_m || !wi.keep || !wi.nkeep || !wi.status ||
            !wi.m_out || !wi.n_out || !wi.ylm_p_out || !wi.ylm_m_out || !wi.workspace)
            return fail(EFD_ERR_ARG, F + ": NULL walker pointer");
        if ((uintptr_t)wi.workspace % 4)
            return fail(EFD_ERR_ARG, F + ": workspace must be 4-byte aligned");
        if (wi.nt < 1 || wi.nt > MODES_MAX_KNOTS)
            return fail(EFD_ERR_ARG, F + ": nt out of range [1, 1024]");
        if (!(wi.eps >= 0.0 && wi.eps <= 1.0))
            return fail(EFD_ERR_ARG, F + ": eps out of range [0, 1]");
        if (wi.amp_cap < 0 || (!wi.amp && wi.amp_cap != 0))
            return fail(EFD_ERR_ARG, F + ": amp_cap needs an amp buffer and must be >= 0");
        if (wi.workspace_bytes < efd_modes_workspace_bytes(wi.nt, tab->nmodes))
            return fail(EFD_ERR_WORKSPACE, F + ": workspace too small (see "
                                               "efd_modes_workspace_bytes)");
        for (int j = 0; j < i; ++j)
            if (w[j].workspace == wi.workspace || w[j].keep == wi.keep)
                return fail(EFD_ERR_ARG, F + ": one workspace and one output set per walker");
        ModesDesc& d = B.d[i];
        d.p = wi.p; d.e = wi.e; d.ylm_p = wi.ylm_p; d.ylm_m = wi.ylm_m; d.teuk = wi.teuk;
        d.eps = wi.eps;
        d.keep = wi.keep; d.nkeep = wi.nkeep; d.status = wi.status;
        d.amp = wi.amp; d.amp_cap = wi.amp_cap;
        d.m_out = wi.m_out; d.n_out = wi.n_out;
        d.ylm_p_out = wi.ylm_p_out; d.ylm_m_out = wi.ylm_m_out;
        d.flags = (uint8_t*)wi.workspace;
        d.nt = wi.nt;
        d.include_minus_m = wi.include_minus_m ? 1 : 0;
        ntmax = std::max(ntmax, (int)wi.nt);
        any_amp |= wi.amp != nullptr;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned nz = (unsigned)count;
    // (a weighted call runs the weighted instantiation for every walker, so a walker's outputs
    // never depend on its companions)
    if (wt)
        hipLaunchKernelGGL(k_modes_select<true>, dim3(ntmax, 1, nz), dim3(MODES_NT), 0, st, B, W);
    else
        hipLaunchKernelGGL(k_modes_select<false>, dim3(ntmax, 1, nz), dim3(MODES_NT), 0, st, B,
                           ModesNoWeights{});
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_modes_compact, dim3(nz), dim3(MODES_NT), 0, st, B);
    HIP_TRY(hipGetLastError());
    if (any_amp) {
        hipLaunchKernelGGL(k_modes_amp, dim3((B.nmodes + 255) / 256, ntmax, nz), dim3(256), 0, st,
                           B);
        HIP_TRY(hipGetLastError());
    }
    return EFD_OK;
}

__global__ __launch_bounds__(256) void k_psd_eval(const double* x, const double* c, int n,
                                                  const double* f, int64_t nf, double* out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < nf) out[j] = efdpsd::psd_eval(x, c, n, f[j]);
}

}  // namespace

extern "C" {

int efd_modes_select_batch(const efd_modes_table* tab, const efd_modes_walker* w, int32_t count,
                           void* stream) {
    return modes_select("efd_modes_select_batch", tab, w, nullptr, nullptr, count, stream);
}

int efd_modes_select_batch_weighted(const efd_modes_table* tab, const efd_modes_walker* w,
                                    const efd_modes_weight* wt, const efd_psd_table* psd,
                                    int32_t count, void* stream) {
    return modes_select("efd_modes_select_batch_weighted", tab, w, wt, psd, count, stream);
}

int efd_psd_eval(const efd_psd_table* psd, const double* f, int64_t nf, double* out,
                 void* stream) {
    const std::string F("efd_psd_eval");
    if (!psd || !psd->x || !psd->c || psd->n < 2 || psd->n > MODES_MAX || nf < 0 ||
        (nf > 0 && (!f || !out)))
        return fail(EFD_ERR_ARG, F + ": bad arguments (2 <= n <= 4096)");
    if (nf == 0) return EFD_OK;
    const int64_t nb = (nf + 255) / 256;
    if (nb > 0x7fffffff) return fail(EFD_ERR_ARG, F + ": nf out of range");
    hipLaunchKernelGGL(k_psd_eval, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, psd->x,
                       psd->c, psd->n, f, nf, out);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

}  // extern "C"
