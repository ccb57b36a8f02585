// emrifd_window.hip -- the windowed path of libemrifd.so (MI355X, gfx950): the Hann window's
// convolution (efd_hann_*: extent scan, staging, the four-step FFT kernels, the fused windowed
// log-likelihoods) and the cosine-sum windows' stencils (efd_cosw_*). Kernels first, then the
// host templates that pick a kernel instance, then the C ABI (include/emrifd.h). Shares only
// emrifd_common.h with the mode sum (emrifd.hip) and the reductions (emrifd_reduce.hip).

#include "emrifd_common.h"

namespace {

// ---- The Hann window's convolution (fdutils.HannConvolution; efd_hann_*). A row's correction
// C = K (*) S (circular, mod nf) is the linear convolution of the row's support [first, last) with
// the lag kernel, on m-point transforms (m >= nf + (last - first) - 1): the caller's Y[s] holds
// S[first + s] / scale for s < last - first, zero up to m (efd_hann_stage), and after its
// transforms (the kernel's spectrum includes 1/m) C[k] = scale Y[((k - first) mod nf) + m - nf].
// info[r] = {bits of scale = max(|Re|, |Im|), first nonzero bin, last nonzero bin + 1, 0}; a
// NaN anywhere in the row makes the scale NaN (the bit pattern orders above every finite
// value), so the row's outputs are NaN.
__global__ void k_hann_info_init(uint64_t* __restrict__ info, int32_t rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    info[4 * r + 0] = 0;
    info[4 * r + 1] = ~0ull;
    info[4 * r + 2] = 0;
    info[4 * r + 3] = 0;
}
// lanes (optional, int32 [rows][2]): each row's paired-grid lane range from its mode sum
// (efd_modesum_lane_ranges); bins outside {l, nf-1-l : lo <= l < hi} hold no term, so the scan
// covers [min(lo, nf-hi), max(hi, nf-lo)) only
__global__ __launch_bounds__(256) void k_hann_extent(const double2* __restrict__ S, int64_t stride,
                                                     int64_t nf, const int32_t* __restrict__ lanes,
                                                     uint64_t* __restrict__ info) {
    const double2* row = S + (int64_t)blockIdx.y * stride;
    int64_t k_lo = 0, k_hi = nf;
    if (lanes != nullptr) {
        const int64_t llo = lanes[2 * blockIdx.y], lhi = lanes[2 * blockIdx.y + 1];
        if (llo >= lhi) {
            k_hi = 0;   // no segment: an all-zero row
        } else {
            k_lo = max((int64_t)0, min(llo, nf - lhi));
            k_hi = min(nf, max(lhi, nf - llo));
        }
    }
    uint64_t mx = 0, lo = ~0ull, hi = 0;
#pragma unroll 8
    for (int64_t k = k_lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < k_hi;
         k += (int64_t)gridDim.x * blockDim.x) {
        const double2 v = row[k];
        const uint64_t bx = (uint64_t)__double_as_longlong(fabs(v.x));
        const uint64_t by = (uint64_t)__double_as_longlong(fabs(v.y));
        mx = max(mx, max(bx, by));
        if ((bx | by) != 0) {          // nonzero (or NaN)
            lo = min(lo, (uint64_t)k);
            hi = (uint64_t)k + 1;      // k grows along the thread's stride
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = max(mx, (uint64_t)__shfl_xor((unsigned long long)mx, o, 64));
        lo = min(lo, (uint64_t)__shfl_xor((unsigned long long)lo, o, 64));
        hi = max(hi, (uint64_t)__shfl_xor((unsigned long long)hi, o, 64));
    }
    // the block's 4 waves through LDS, then one thread's 3 atomics per block (a few hundred
    // per row: contention on the row's 3 words stays small)
    __shared__ uint64_t red[3][4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wv] = mx;
        red[1][wv] = lo;
        red[2][wv] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) {
            mx = max(mx, red[0][i]);
            lo = min(lo, red[1][i]);
            hi = max(hi, red[2][i]);
        }
        uint64_t* in = info + 4 * blockIdx.y;
        if (mx) atomicMax((unsigned long long*)&in[0], (unsigned long long)mx);
        if (hi) {
            atomicMin((unsigned long long*)&in[1], (unsigned long long)lo);
            atomicMax((unsigned long long*)&in[2], (unsigned long long)hi);
        }
    }
}
struct HannRow {
    int64_t first, len;
    double scale;   // 0 for an all-zero row (its Y is zero)
};
__device__ __forceinline__ HannRow hann_row(const uint64_t* __restrict__ info, int r) {
    HannRow h;
    const uint64_t lo = info[4 * r + 1], hi = info[4 * r + 2];
    h.first = hi ? (int64_t)lo : 0;
    h.len = hi ? (int64_t)(hi - lo) : 0;
    h.scale = __longlong_as_double((long long)info[4 * r + 0]);
    return h;
}
// complex64 values as 2-wide float vectors: the arithmetic below compiles to packed FP32
// instructions (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32, one issue slot per complex add or
// half a complex multiply), about half the VALU instructions of scalar float2 code
typedef float fcv __attribute__((ext_vector_type(2)));
// a row's scaled support, element s of the m-point transform's input: S[first + s] / scale for
// s < len, zero up to m
struct HannSupport {
    const double2* src;   // the row of S at its first nonzero bin
    int64_t len;
    double inv;           // 1 / scale (0 for an all-zero row; NaN scale: NaN row)
    bool bad;             // len > m (the host sized m from info: never, but never write past Y)
};
__device__ __forceinline__ HannSupport hann_support(const double2* __restrict__ S, int64_t stride,
                                                    const uint64_t* __restrict__ info, int r,
                                                    int64_t m) {
    const HannRow h = hann_row(info, r);
    return {S + (int64_t)r * stride + h.first, h.len, h.scale == 0.0 ? 0.0 : 1.0 / h.scale,
            h.len > m};
}
__device__ __forceinline__ fcv fc_load_scaled(const HannSupport x, int64_t s) {
    fcv v = {0.f, 0.f};
    if (x.bad) {
        v = (fcv){__int_as_float(0x7fc00000), 0.f};
    } else if (s < x.len) {
        const double2 d = x.src[s];
        v = (fcv){(float)(d.x * x.inv), (float)(d.y * x.inv)};
    }
    return v;
}
__global__ __launch_bounds__(256) void k_hann_stage(const double2* __restrict__ S, int64_t stride,
                                                    const uint64_t* __restrict__ info, int64_t m,
                                                    float2* __restrict__ Y) {
    const int r = blockIdx.y;
    fcv* y = reinterpret_cast<fcv*>(Y) + (int64_t)r * m;
    const HannSupport x = hann_support(S, stride, info, r, m);
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < m;
         s += (int64_t)gridDim.x * blockDim.x)
        y[s] = fc_load_scaled(x, s);
}
// ---- The Hann correction's convolution as one four-step FFT pipeline (efd_hann_convolve).
// Y = ifft_m(fft_m(y) * kf) for power-of-two m = R * C, C = 8192, R = m / C (256..4096), in
// complex64, with y the scaled support of each row (efd_hann_stage's values, computed on the
// fly). Index s = C r + c (row r, column c), frequency f = f_r + R f_c:
//   (A) columns: length-R FFT over r of every column c, times w_m^(c f_r)   -> [f_r][c]
//   (B) rows:    length-C FFT over c of every row f_r gives X[f_r + R f_c] at [f_r][f_c]; times
//                the lag kernel's spectrum in the same order (kfp[f_r C + f_c] = kf[f_r + R f_c],
//                1/m included); inverse length-C FFT                           -> [f_r][c]
//   (C) columns: times w_m^(-c f_r), inverse length-R FFT over f_r          -> [r][c] = Y[s]
// The spectrum is never put in natural order: the two transposes on each side of rocFFT's
// 2^24-point transform (five kernels per direction) and the separate stage and multiply passes
// are gone; three passes over Y remain. Stockham radix-8 passes (a radix-4 or -2 one last) in
// LDS, ~70 KB per workgroup so two share a CU (one's global loads overlap the other's
// transforms), twiddles from __sincosf (absolute error ~5e-7: the correction needs ~3 digits).
constexpr int FC_C = 8192;             // row length (LDS: 8192 x 8 B + 1/16 padding = 68 KB)
constexpr int FC_NT = 512;             // threads of a column or row workgroup
constexpr float FC_2PI = 6.283185307179586f;
constexpr float FC_SQRT_HALF = 0.70710678118654752f;

__device__ __forceinline__ fcv cmulf(fcv a, fcv b) {
    const fcv t = a.xx * b;
    return __builtin_elementwise_fma(a.yy, b.yx * (fcv){-1.0f, 1.0f}, t);
}
// x times -i (SIGN -1) or +i (SIGN +1)
template <int SIGN>
__device__ __forceinline__ fcv cmuli(fcv x) {
    return x.yx * (SIGN < 0 ? (fcv){1.0f, -1.0f} : (fcv){-1.0f, 1.0f});
}
// natural-order DFTs of 4 and 8 points in registers, exp(SIGN 2 pi i n k / N)
template <int SIGN>
__device__ __forceinline__ void fc_dft4(fcv& a0, fcv& a1, fcv& a2, fcv& a3) {
    const fcv t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3;
    const fcv t3 = cmuli<SIGN>(a1 - a3);
    a0 = t0 + t2;
    a1 = t1 + t3;
    a2 = t0 - t2;
    a3 = t1 - t3;
}
template <int SIGN>
__device__ __forceinline__ void fc_dft8(fcv* v) {
    fcv e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    fcv o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    fc_dft4<SIGN>(e0, e1, e2, e3);
    fc_dft4<SIGN>(o0, o1, o2, o3);
    // o_k times w8^k, w8 = (1 + SIGN i) / sqrt 2: w8 o = (o + SIGN i o) / sqrt 2,
    // w8^3 o = (-o + SIGN i o) / sqrt 2
    o1 = FC_SQRT_HALF * (o1 + cmuli<SIGN>(o1));
    o2 = cmuli<SIGN>(o2);
    o3 = FC_SQRT_HALF * (cmuli<SIGN>(o3) - o3);
    v[0] = e0 + o0;
    v[1] = e1 + o1;
    v[2] = e2 + o2;
    v[3] = e3 + o3;
    v[4] = e0 - o0;
    v[5] = e1 - o1;
    v[6] = e2 - o2;
    v[7] = e3 - o3;
}
// element e of line j in LDS: columns pass [e][j] rows padded to NCOL + 1, rows pass one line
// with a pad element every 16
template <int NCOL>
struct FcColIdx {
    // (2 columns: no pad, so m = 2^25's 4096-row blocks fit two workgroups per CU; 8 columns: no
    // pad either, the reads of 4 lines x 8 columns by 32 lanes then fill the 64 banks (the pad
    // of 9 made them 2-way, r05z5: 0.47 of the LDS cycles conflicts) and only the first
    // pass's stores, 2 lines x 8 columns per 16-lane group at 8 lines apart, are 2-way)
    static constexpr int STRIDE = (NCOL > 2 && NCOL != 8) ? NCOL + 1 : NCOL;
    __device__ __forceinline__ int operator()(int j, int e) const { return e * STRIDE + j; }
};
struct FcRowIdx {
    __device__ __forceinline__ int operator()(int, int e) const { return e + (e >> 4); }
};

// One Stockham pass of radix RAD over 2^LOGL lines of length L held in LDS (in place: every
// thread reads its butterflies into registers, barrier, writes). SIGN -1: forward.
template <int RAD, int SIGN, int NITEM, int LOGL, class Idx>
__device__ __forceinline__ void fc_pass(fcv* sm, int L, int lgNs, Idx idx) {
    fcv v[NITEM][RAD];
    const int Ns = 1 << lgNs;
    const int tid = threadIdx.x;
    const int bfly = L / RAD;
#pragma unroll
    for (int q = 0; q < NITEM; ++q) {
        const int item = tid + q * FC_NT;
        const int j = item & ((1 << LOGL) - 1), b = item >> LOGL;
        const int k = b & (Ns - 1);
#pragma unroll
        for (int r = 0; r < RAD; ++r) v[q][r] = sm[idx(j, b + r * bfly)];
        if (lgNs > 0) {
            float sn, cs;
            // 2 pi k / (Ns RAD): the power-of-two division as an exponent shift
            __sincosf((float)SIGN * FC_2PI * ldexpf((float)k, -(lgNs + (RAD == 8 ? 3 : RAD == 4 ? 2 : 1))),
                      &sn, &cs);
            const fcv w1 = {cs, sn};
            fcv w = w1;
#pragma unroll
            for (int r = 1; r < RAD; ++r) {
                v[q][r] = cmulf(v[q][r], w);
                if (r + 1 < RAD) w = cmulf(w, w1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NITEM; ++q) {
        const int item = tid + q * FC_NT;
        const int j = item & ((1 << LOGL) - 1), b = item >> LOGL;
        const int d = ((b >> lgNs) << lgNs) * RAD + (b & (Ns - 1));
        if (RAD == 8) {
            fc_dft8<SIGN>(v[q]);
        } else if (RAD == 4) {
            fc_dft4<SIGN>(v[q][0], v[q][1], v[q][2], v[q][3]);
        } else {
            const fcv a0 = v[q][0], a1 = v[q][1];
            v[q][0] = a0 + a1;
            v[q][1] = a0 - a1;
        }
#pragma unroll
        for (int r = 0; r < RAD; ++r) sm[idx(j, d + r * Ns)] = v[q][r];
    }
    __syncthreads();
}

// the whole length-L transform of 2^LOGL lines (natural order in, natural order out): radix-8
// passes, then one radix-4 or radix-2 pass for the rest
template <int SIGN, int L, int LOGL, class Idx>
__device__ __forceinline__ void fc_fft(fcv* sm, Idx idx) {
    constexpr int N8 = ((L / 8) << LOGL) / FC_NT;
    static_assert(((L / 8) << LOGL) % FC_NT == 0, "radix-8 butterflies: whole rounds per thread");
    int lg = 0;
#pragma unroll 1
    for (; (8 << lg) <= L; lg += 3) fc_pass<8, SIGN, N8, LOGL>(sm, L, lg, idx);
    if ((4 << lg) == L) fc_pass<4, SIGN, ((L / 4) << LOGL) / FC_NT, LOGL>(sm, L, lg, idx);
    else if ((2 << lg) == L) fc_pass<2, SIGN, ((L / 2) << LOGL) / FC_NT, LOGL>(sm, L, lg, idx);
}

template <int R>
struct FcCols {
    static constexpr int NCOL = R >= 4096 ? 2 : R >= 2048 ? 4 : R >= 1024 ? 8 : 16;
    static constexpr int LOGL = NCOL == 2 ? 1 : NCOL == 4 ? 2 : NCOL == 8 ? 3 : 4;
};
// XCD-aware column blocks: workgroups are dealt round-robin over the 8 XCDs (x = b mod 8), so
// XCD x takes the contiguous eighth [x G/8, (x+1) G/8) of the G column blocks in order; a
// block's rows are NCOL * 8 or 16 B wide, and the neighbouring blocks sharing their 128-B lines
// then hit the same L2. rows: the rows that share the grid's x with the column blocks, a column
// block's rows on consecutive workgroups of its XCD (1: the rows lie along y)
template <int G, class T>
__device__ __forceinline__ T fc_col_block(T rows) {
    static_assert(G % 8 == 0, "column blocks: a multiple of the 8 XCDs");
    return (T)(blockIdx.x & 7) * (G / 8) + (T)(blockIdx.x >> 3) / rows;
}
// the column twiddle w_M^(SIGN c e) of column c at row frequency e
template <int SIGN, int64_t M>
__device__ __forceinline__ fcv fc_col_twiddle(int c, int e) {
    const uint32_t p = (uint32_t)c * (uint32_t)e;   // < C R = M: no reduction
    float sn, cs;
    __sincosf((float)SIGN * FC_2PI * ((float)p * (1.0f / (float)M)), &sn, &cs);
    return (fcv){cs, sn};
}
// (C)'s first half for the NCOL columns from c0: load, conjugate twiddle, inverse FFT; the
// columns are left in sm in natural order
template <int R, int C>
__device__ __forceinline__ void fc_cols_inverse(fcv* sm, const fcv* y, int c0) {
    constexpr int NCOL = FcCols<R>::NCOL;
    static_assert(R * NCOL % FC_NT == 0, "whole rounds of elements per thread");
    const FcColIdx<NCOL> idx;
#pragma unroll
    for (int q = 0; q < R * NCOL / FC_NT; ++q) {
        const int i = threadIdx.x + q * FC_NT;
        const int e = i / NCOL, j = i % NCOL;   // e = f_r
        const int c = c0 + j;
        const fcv w = fc_col_twiddle<1, (int64_t)R * C>(c, e);
        sm[idx(j, e)] = cmulf(y[(int64_t)e * C + c], w);
    }
    __syncthreads();
    fc_fft<1, R, FcCols<R>::LOGL>(sm, idx);
}

// (A) and (C): NCOL columns per workgroup. FWD: load the scaled support of row blockIdx.y
// straight from S (efd_hann_stage's values), forward FFT, twiddle, store. Inverse: load,
// conjugate twiddle, inverse FFT, store in natural order.
// (<= 128 VGPRs: two 8-wave workgroups per CU, 4 waves per SIMD)
template <bool FWD, int R, int C = FC_C>
__global__ __launch_bounds__(FC_NT) __attribute__((amdgpu_waves_per_eu(4, 8)))
void k_fc_cols(const double2* __restrict__ S, int64_t stride, const uint64_t* __restrict__ info,
               float2* __restrict__ Yv) {
    constexpr int NCOL = FcCols<R>::NCOL, LOGL = FcCols<R>::LOGL;
    constexpr int64_t M = (int64_t)R * C;
    constexpr int NQ = R * NCOL / FC_NT;   // elements per thread
    static_assert(R * NCOL % FC_NT == 0, "whole rounds of elements per thread");
    __shared__ fcv sm[R * FcColIdx<NCOL>::STRIDE];
    const FcColIdx<NCOL> idx;
    const int row = blockIdx.y;
    const int c0 = fc_col_block<C / NCOL>(1u) * NCOL;
    fcv* y = reinterpret_cast<fcv*>(Yv) + (int64_t)row * M;
    if (FWD) {
        const HannSupport x = hann_support(S, stride, info, row, M);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = threadIdx.x + q * FC_NT;
            const int e = i / NCOL, j = i % NCOL;
            sm[idx(j, e)] = fc_load_scaled(x, (int64_t)e * C + c0 + j);
        }
        __syncthreads();
        fc_fft<-1, R, LOGL>(sm, idx);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = threadIdx.x + q * FC_NT;
            const int e = i / NCOL, j = i % NCOL;   // e = f_r
            const int c = c0 + j;
            const fcv w = fc_col_twiddle<-1, M>(c, e);
            y[(int64_t)e * C + c] = cmulf(sm[idx(j, e)], w);
        }
    } else {
        fc_cols_inverse<R, C>(sm, y, c0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = threadIdx.x + q * FC_NT;
            const int e = i / NCOL, j = i % NCOL;
            y[(int64_t)e * C + c0 + j] = sm[idx(j, e)];
        }
    }
}

// (B): one row f_r per workgroup: forward FFT, times the kernel's spectrum, inverse FFT, as
// three register stages per direction with two LDS exchanges between them (8192 = 32 x 16 x 16):
//   forward  (A) thread t = n2 (n = n2 + 256 n1): DFT-32 over n1, times w_8192^(n2 k1)
//            (B) task (k1, n2a) (n2 = n2a + 16 n2b): DFT-16 over n2b, times w_256^(n2a k2a)
//            (C) task (k1, k2a): DFT-16 over n2a -> X[k1 + 32 k2a + 512 k2b], natural index k
//   times the kernel's spectrum at k, then the transpose of the same steps: the inverse of (C) on
//   the same task's registers (no exchange), of (B), of (A) -> x[n2 + 256 n1], natural order.
// Four exchanges of 64 KB per row instead of the Stockham passes' ten (five radix-8/2 passes per
// direction, each a 64-KB LDS read and write) and the multiply's own pass; every exchange is
// bank-conflict free (exchange 1: rows of 257 elements, lanes along k1 at stride 514 words;
// exchange 2: [k2a][n2a][k1], lanes along k1). Twiddle powers from two __sincosf (w, w^8).
constexpr int FR_NT = 256;     // threads of the row workgroup (32 elements each)
constexpr int FR_S1 = 257;     // exchange 1: LDS row stride of [k1][n2] (elements)
// cos and sin of 2 pi j / 32
constexpr float FC_COS32[32] = {
    1.000000000e+00f, 9.807852804e-01f, 9.238795325e-01f, 8.314696123e-01f, 7.071067812e-01f,
    5.555702330e-01f, 3.826834324e-01f, 1.950903220e-01f, 0.0f, -1.950903220e-01f,
    -3.826834324e-01f, -5.555702330e-01f, -7.071067812e-01f, -8.314696123e-01f,
    -9.238795325e-01f, -9.807852804e-01f, -1.000000000e+00f, -9.807852804e-01f,
    -9.238795325e-01f, -8.314696123e-01f, -7.071067812e-01f, -5.555702330e-01f,
    -3.826834324e-01f, -1.950903220e-01f, 0.0f, 1.950903220e-01f, 3.826834324e-01f,
    5.555702330e-01f, 7.071067812e-01f, 8.314696123e-01f, 9.238795325e-01f, 9.807852804e-01f};
// w_N^j = exp(SIGN 2 pi i j / N) for N = 16, 32 (compile-time j: constant-folded)
template <int SIGN, int N>
__device__ __forceinline__ fcv fc_w(int j) {
    const int q = (j * (32 / N)) & 31;
    return (fcv){FC_COS32[q], (float)SIGN * FC_COS32[(q + 24) & 31]};
}
// natural-order DFT-16 (N1 = 4: 4 x 4) and DFT-32 (N1 = 8: 4 x 8) in registers,
// exp(SIGN 2 pi i n k / (4 N1))
template <int SIGN, int N1>
__device__ __forceinline__ void fc_dft4x(fcv* v) {
    static_assert(N1 == 4 || N1 == 8, "DFT-16 or DFT-32");
    fcv t[N1][4];
#pragma unroll
    for (int n1 = 0; n1 < N1; ++n1) {   // DFT-4 over n2 of x[n1 + N1 n2]
        fcv a0 = v[n1], a1 = v[n1 + N1], a2 = v[n1 + 2 * N1], a3 = v[n1 + 3 * N1];
        fc_dft4<SIGN>(a0, a1, a2, a3);
        t[n1][0] = a0; t[n1][1] = a1; t[n1][2] = a2; t[n1][3] = a3;
    }
#pragma unroll
    for (int n1 = 1; n1 < N1; ++n1)
#pragma unroll
        for (int k1 = 1; k1 < 4; ++k1) t[n1][k1] = cmulf(t[n1][k1], fc_w<SIGN, 4 * N1>(n1 * k1));
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {   // DFT-N1 over n1 -> X[k1 + 4 k2]
        fcv e[N1];
#pragma unroll
        for (int n1 = 0; n1 < N1; ++n1) e[n1] = t[n1][k1];
        if constexpr (N1 == 8) fc_dft8<SIGN>(e);
        else fc_dft4<SIGN>(e[0], e[1], e[2], e[3]);
#pragma unroll
        for (int k2 = 0; k2 < N1; ++k2) v[k1 + 4 * k2] = e[k2];
    }
}
template <int SIGN>
__device__ __forceinline__ void fc_dft16(fcv* v) { fc_dft4x<SIGN, 4>(v); }
template <int SIGN>
__device__ __forceinline__ void fc_dft32(fcv* v) { fc_dft4x<SIGN, 8>(v); }
// v[j] *= w^j, j = 0 .. N-1, w = exp(i theta): powers from w and w^8 (at most 3 + 7 products).
// FROM: v[j] *= w0 w^j, the constant factor w0 folded into the powers (8 products more instead
// of N); without it no product by 1 is formed
template <int N, bool FROM = false>
__device__ __forceinline__ void fc_twiddle_pow(fcv* v, float theta, fcv w0 = {1.0f, 0.0f}) {
    float s1, c1, s8, c8;
    __sincosf(theta, &s1, &c1);
    __sincosf(8.0f * theta, &s8, &c8);
    const fcv w1 = {c1, s1}, w8 = {c8, s8};
    fcv p[8];
    p[0] = w0;
    if constexpr (!FROM) p[1] = w1;
#pragma unroll
    for (int j = FROM ? 1 : 2; j < 8; ++j) p[j] = cmulf(p[j - 1], w1);
    fcv b = (fcv){1.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < N / 8; ++a) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (FROM || a + j > 0)
                v[8 * a + j] = cmulf(v[8 * a + j],
                                     a == 0 ? p[j] : (!FROM && j == 0) ? b : cmulf(b, p[j]));
        b = a == 0 ? w8 : cmulf(b, w8);
    }
}
// the workgroup's (row f_r, walker) pair as p = f_r rows + walker: XCD x = b mod 8 takes the
// contiguous eighth of the pairs in f_r-major order, so a kernel-spectrum row is read from HBM
// once per XCD and from its L2 for the group's other walkers (gridDim.x = R * rows, a multiple
// of 8). (The row kernels split p themselves: split in here, the compiler orders their address
// arithmetic differently, the only change that made to their instruction streams.)
__device__ __forceinline__ int64_t fc_row_pair() {
    const int64_t npair = (int64_t)gridDim.x;
    return (int64_t)(blockIdx.x & 7) * (npair >> 3) + (blockIdx.x >> 3);
}
__global__ __launch_bounds__(FR_NT)
void k_fc_rows(const float2* __restrict__ kfpv, int64_t m, int rows, float2* __restrict__ Yv) {
    static_assert(FC_C == 32 * 16 * 16 && FR_NT == 256, "row transform: 8192 = 32 x 16 x 16");
    __shared__ fcv sm[32 * FR_S1];   // exchange 1 [k1][n2] (stride 257); exchange 2 [k2a][n2a][k1]
    const fcv* kfp = reinterpret_cast<const fcv*>(kfpv);
    fcv* Y = reinterpret_cast<fcv*>(Yv);
    const int64_t p = fc_row_pair();   // = f_r rows + walker
    const int fr = (int)(p / rows), wk = (int)(p - (int64_t)fr * rows);
    fcv* y = Y + (int64_t)wk * m + (int64_t)fr * FC_C;
    const fcv* kr = kfp + (int64_t)fr * FC_C;
    const int t = threadIdx.x;
    constexpr float W8192 = FC_2PI / 8192.0f, W256 = FC_2PI / 256.0f;
    {   // forward (A): n2 = t
        fcv v[32];
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) v[n1] = y[t + 256 * n1];
        fc_dft32<-1>(v);
        fc_twiddle_pow<32>(v, -W8192 * (float)t);
#pragma unroll
        for (int k1 = 0; k1 < 32; ++k1) sm[k1 * FR_S1 + t] = v[k1];
    }
    __syncthreads();
    fcv u[2][16];
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // forward (B): task (k1, n2a)
        const int q = t + 256 * h, k1 = q & 31, n2a = q >> 5;
#pragma unroll
        for (int n2b = 0; n2b < 16; ++n2b) u[h][n2b] = sm[k1 * FR_S1 + n2a + 16 * n2b];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = t + 256 * h, k1 = q & 31, n2a = q >> 5;
        fc_dft16<-1>(u[h]);
        fc_twiddle_pow<16>(u[h], -W256 * (float)n2a);
#pragma unroll
        for (int k2a = 0; k2a < 16; ++k2a) sm[(k2a * 16 + n2a) * 32 + k1] = u[h][k2a];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // forward (C), the kernel's spectrum, inverse (C): (k1, k2a)
        const int q = t + 256 * h, k1 = q & 31, k2a = q >> 5;
#pragma unroll
        for (int n2a = 0; n2a < 16; ++n2a) u[h][n2a] = sm[(k2a * 16 + n2a) * 32 + k1];
        fc_dft16<-1>(u[h]);
#pragma unroll
        for (int k2b = 0; k2b < 16; ++k2b)
            u[h][k2b] = cmulf(u[h][k2b], kr[k1 + 32 * k2a + 512 * k2b]);
        fc_dft16<1>(u[h]);
        fc_twiddle_pow<16>(u[h], W256 * (float)k2a);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = t + 256 * h, k1 = q & 31, k2a = q >> 5;
#pragma unroll
        for (int n2a = 0; n2a < 16; ++n2a) sm[(k2a * 16 + n2a) * 32 + k1] = u[h][n2a];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // inverse (B): task (k1, n2a)
        const int q = t + 256 * h, k1 = q & 31, n2a = q >> 5;
#pragma unroll
        for (int k2a = 0; k2a < 16; ++k2a) u[h][k2a] = sm[(k2a * 16 + n2a) * 32 + k1];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = t + 256 * h, k1 = q & 31, n2a = q >> 5;
        fc_dft16<1>(u[h]);   // -> n2b
        // times w_8192^(-n2 k1), n2 = n2a + 16 n2b: w^(n2a k1) (w^(16 k1))^n2b
        float s0, c0;
        __sincosf(W8192 * (float)(n2a * k1), &s0, &c0);
        const fcv w0 = {c0, s0};
#pragma unroll
        for (int n2b = 0; n2b < 16; ++n2b) u[h][n2b] = cmulf(u[h][n2b], w0);
        fc_twiddle_pow<16>(u[h], W8192 * 16.0f * (float)k1);
#pragma unroll
        for (int n2b = 0; n2b < 16; ++n2b) sm[k1 * FR_S1 + n2a + 16 * n2b] = u[h][n2b];
    }
    __syncthreads();
    {   // inverse (A): n2 = t -> x[n2 + 256 n1]
        fcv v[32];
#pragma unroll
        for (int k1 = 0; k1 < 32; ++k1) v[k1] = sm[k1 * FR_S1 + t];
        fc_dft32<1>(v);
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) y[t + 256 * n1] = v[n1];
    }
}

// (B) for rows of C = 16384 (m = 2^24 as 1024 x 16384: wider column segments, 128 B of S and 64 B
// of Y per row of a column block), register-staged as k_fc_rows with 512 threads of 32 elements
// (16384 = 32 x 32 x 16; n = n2 + 512 n1, n2 = n2a + 16 n2b; k = k1 + 32 k2a + 1024 k2b): forward
// (A) thread n2: DFT-32 over n1, times w_16384^(n2 k1); (B) task (k1, n2a): DFT-32 over n2b,
// times w_512^(n2a k2a); (C) task (k1, k2a), two per thread: DFT-16 over n2a; the kernel's
// spectrum; the transposed steps back. (Round 5 also kept complex exchanges with 128 KB of LDS,
// one workgroup per CU: 650 against 575-579 us, r05z; deleted in round 6.)
constexpr int FC_C16 = 16384;
// Every exchange in two passes (real parts, then imaginary parts) through a float array: 69.6 KB of LDS and at most 128 VGPRs, so two workgroups share a CU and one's
// loads and stores overlap the other's transforms (one per CU leaves HBM idle while it
// computes). Exchange 1 [k1][n2] stride 513, exchange 2 [k2a][n2a][k1] unpadded: every b32
// access of a 32-lane bank group hits 32 distinct banks (ds_read_b32 / ds_write_b32 bank
// (a/4) mod 32; stride 514 read exchange 1 2-way, r05z5: 0.20 of the LDS cycles conflicts).
constexpr int FR16_T1 = 513, FR16_T2 = 512;
__global__ __launch_bounds__(FC_NT) __attribute__((amdgpu_waves_per_eu(4, 8)))
void k_fc_rows16k_h(const float2* __restrict__ kfpv, int64_t m, int rows, float2* __restrict__ Yv) {
    static_assert(FC_NT == 512 && FC_C16 == 32 * 32 * 16, "16384 = 32 x 32 x 16, 512 threads");
    __shared__ float sf[32 * (FR16_T1 > FR16_T2 ? FR16_T1 : FR16_T2)];
    const fcv* kfp = reinterpret_cast<const fcv*>(kfpv);
    fcv* Y = reinterpret_cast<fcv*>(Yv);
    const int64_t p = fc_row_pair();   // = f_r rows + walker
    const int fr = (int)(p / rows), wk = (int)(p - (int64_t)fr * rows);
    fcv* y = Y + (int64_t)wk * m + (int64_t)fr * FC_C16;
    const fcv* kr = kfp + (int64_t)fr * FC_C16;
    const int t = threadIdx.x;
    const int kb = t & 31, nb = t >> 5;
    constexpr float W16K = FC_2PI / 16384.0f, W512 = FC_2PI / 512.0f;
    fcv v[32], u[32], w[2][16];
#pragma unroll
    for (int n1 = 0; n1 < 32; ++n1) v[n1] = y[t + 512 * n1];
    fc_dft32<-1>(v);   // forward (A): n2 = t
    fc_twiddle_pow<32>(v, -W16K * (float)t);
#pragma unroll
    for (int c = 0; c < 2; ++c) {   // exchange 1 -> (B) task (k1 = kb, n2a = nb)
#pragma unroll
        for (int k1 = 0; k1 < 32; ++k1) sf[k1 * FR16_T1 + t] = c ? v[k1].y : v[k1].x;
        __syncthreads();
#pragma unroll
        for (int n2b = 0; n2b < 32; ++n2b) {
            const float x = sf[kb * FR16_T1 + nb + 16 * n2b];
            if (c) u[n2b].y = x; else u[n2b].x = x;
        }
        __syncthreads();
    }
    fc_dft32<-1>(u);
    fc_twiddle_pow<32>(u, -W512 * (float)nb);
#pragma unroll
    for (int c = 0; c < 2; ++c) {   // exchange 2 -> (C) tasks (k1, k2a)
#pragma unroll
        for (int k2a = 0; k2a < 32; ++k2a) sf[k2a * FR16_T2 + nb * 32 + kb] = c ? u[k2a].y : u[k2a].x;
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = t + 512 * h, k1 = q & 31, k2a = q >> 5;
#pragma unroll
            for (int n2a = 0; n2a < 16; ++n2a) {
                const float x = sf[k2a * FR16_T2 + n2a * 32 + k1];
                if (c) w[h][n2a].y = x; else w[h][n2a].x = x;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // forward (C), the kernel's spectrum, inverse (C)
        const int q = t + 512 * h, k1 = q & 31, k2a = q >> 5;
        fc_dft16<-1>(w[h]);
#pragma unroll
        for (int k2b = 0; k2b < 16; ++k2b)
            w[h][k2b] = cmulf(w[h][k2b], kr[k1 + 32 * k2a + 1024 * k2b]);
        fc_dft16<1>(w[h]);
        fc_twiddle_pow<16>(w[h], W512 * (float)k2a);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {   // exchange 2 back -> inverse (B)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = t + 512 * h, k1 = q & 31, k2a = q >> 5;
#pragma unroll
            for (int n2a = 0; n2a < 16; ++n2a)
                sf[k2a * FR16_T2 + n2a * 32 + k1] = c ? w[h][n2a].y : w[h][n2a].x;
        }
        __syncthreads();
#pragma unroll
        for (int k2a = 0; k2a < 32; ++k2a) {
            const float x = sf[k2a * FR16_T2 + nb * 32 + kb];
            if (c) u[k2a].y = x; else u[k2a].x = x;
        }
        __syncthreads();
    }
    fc_dft32<1>(u);   // -> n2b, times w_16384^(-n2 k1)
    {
        float s0, c0;
        __sincosf(W16K * (float)(nb * kb), &s0, &c0);
        const fcv w0 = {c0, s0};
        fc_twiddle_pow<32, true>(u, W16K * 16.0f * (float)kb, w0);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {   // exchange 1 back -> inverse (A): n2 = t
#pragma unroll
        for (int n2b = 0; n2b < 32; ++n2b) sf[kb * FR16_T1 + nb + 16 * n2b] = c ? u[n2b].y : u[n2b].x;
        __syncthreads();
#pragma unroll
        for (int k1 = 0; k1 < 32; ++k1) {
            const float x = sf[k1 * FR16_T1 + t];
            if (c) v[k1].y = x; else v[k1].x = x;
        }
        if (c == 0) __syncthreads();
    }
    fc_dft32<1>(v);
    // the store offsets from an opaque copy of t: else the compiler keeps the loads' 32
    // addresses live across the kernel (spilled to scratch)
    int to = t;
    __asm__ volatile("" : "+v"(to));
#pragma unroll
    for (int n1 = 0; n1 < 32; ++n1) y[to + 512 * n1] = v[n1];
}

// (A) for R = 1024 with rows of C = 16384 (m = 2^24 as 1024 x 16384), NCOL = 8 columns per
// workgroup, register-staged (1024 = 16 x 8 x 8; n = n2 + 64 n1, n2 = n2a + 8 n2b; k = k1 + 16 k2a
// + 128 k2b): task (j, n2): DFT-16 over n1, times w_1024^(n2 k1); (B) tasks (j, k1, n2a), two per
// thread: DFT-8 over n2b, times w_64^(n2a k2a); (C) tasks (j, k1, k2a), two per thread: DFT-8
// over n2a -> f_r = k. Exchange 1 [k1][n2][j], exchange 2 [k1][k2a][n2a (pad to 9)][j]: lanes
// along j then n2a / k2a, conflict-free. 252 against the Stockham kernel's 369 us (r05z3). The
// inverse columns stay on the Stockham kernel k_fc_cols<false, 1024, 16384>: the staged inverse
// measured 549 against 476 us (r05z3; deleted in round 6).
constexpr int FCD_R = 1024, FCD_NCOL = 8, FCD_S2 = 9;
__global__ __launch_bounds__(FC_NT) __attribute__((amdgpu_waves_per_eu(4, 8)))
void k_fc_cols1024(const double2* __restrict__ S, int64_t stride, const uint64_t* __restrict__ info,
                   float2* __restrict__ Yv) {
    static_assert(FC_NT == 512 && FCD_R * FCD_NCOL == 16 * FC_NT, "16 elements per thread");
    constexpr int C = FC_C16;
    constexpr int64_t M = (int64_t)FCD_R * C;
    // exchange 1: 16 x 64 x 8 = 8192; exchange 2: 16 x 8 x 9 x 8 = 9216 elements (73.7 KB)
    __shared__ fcv sm[16 * 8 * FCD_S2 * FCD_NCOL];
    const int row = blockIdx.y;
    const int c0 = fc_col_block<C / FCD_NCOL>(1u) * FCD_NCOL;
    fcv* y = reinterpret_cast<fcv*>(Yv) + (int64_t)row * M;
    const int t = threadIdx.x;
    const int j = t & 7;
    const int c = c0 + j;
    constexpr float W1024 = FC_2PI / 1024.0f, W64 = FC_2PI / 64.0f;
    auto e1 = [](int k1, int n2, int jj) { return (k1 * 64 + n2) * FCD_NCOL + jj; };
    auto e2 = [](int k1, int k2a, int n2a, int jj) {
        return ((k1 * 8 + k2a) * FCD_S2 + n2a) * FCD_NCOL + jj;
    };
    {
        const HannSupport x = hann_support(S, stride, info, row, M);
        {   // (A): task (j, n2)
            const int n2 = t >> 3;
            fcv v[16];
#pragma unroll
            for (int n1 = 0; n1 < 16; ++n1)
                v[n1] = fc_load_scaled(x, (int64_t)(n2 + 64 * n1) * C + c);
            fc_dft16<-1>(v);
            fc_twiddle_pow<16>(v, -W1024 * (float)n2);
#pragma unroll
            for (int k1 = 0; k1 < 16; ++k1) sm[e1(k1, n2, j)] = v[k1];
        }
        __syncthreads();
        fcv u[2][8];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {   // (B): tasks (j, n2a, k1)
            const int q = t + FC_NT * hh, n2a = (q >> 3) & 7, k1 = q >> 6;
#pragma unroll
            for (int n2b = 0; n2b < 8; ++n2b) u[hh][n2b] = sm[e1(k1, n2a + 8 * n2b, j)];
        }
        __syncthreads();
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int q = t + FC_NT * hh, n2a = (q >> 3) & 7, k1 = q >> 6;
            fc_dft8<-1>(u[hh]);
            fc_twiddle_pow<8>(u[hh], -W64 * (float)n2a);
#pragma unroll
            for (int k2a = 0; k2a < 8; ++k2a) sm[e2(k1, k2a, n2a, j)] = u[hh][k2a];
        }
        __syncthreads();
        int to = t;   // opaque: no store address kept live from (A)
        __asm__ volatile("" : "+v"(to));
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {   // (C): tasks (j, k2a, k1)
            const int q = to + FC_NT * hh, k2a = (q >> 3) & 7, k1 = q >> 6;
            fcv w[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) w[a] = sm[e2(k1, k2a, a, j)];
            fc_dft8<-1>(w);
#pragma unroll
            for (int k2b = 0; k2b < 8; ++k2b) {
                const int fr = k1 + 16 * k2a + 128 * k2b;
                y[(int64_t)fr * C + c] = cmulf(w[k2b], fc_col_twiddle<-1, M>(c, fr));
            }
        }
    }
}

// S_w at bin k: the 3-point stencil on S and the correction's difference (neighbours mod nf).
// S is zero outside the row's support [first, first + len) (cyclic; efd_hann_extent's bounds),
// so it is read only there: the support is ~40% of test.sh's grid, and the skipped reads were
// half of the reduction's HBM bytes (the correction C = Y is nonzero everywhere)
struct HannSrc {
    const double2* S;   // the row of S and of Y
    const float2* Y;
    int64_t nf;
    double c;           // the correction's weight e / 4 times the row's scale
    int64_t first, len, off;
};
__device__ __forceinline__ HannSrc hann_src(const double2* __restrict__ S, int64_t stride,
                                            const float2* __restrict__ Y,
                                            const uint64_t* __restrict__ info, int r, int64_t m,
                                            int64_t nf) {
    const HannRow h = hann_row(info, r);
    return {S + (int64_t)r * stride, Y + (int64_t)r * m, nf, h.scale / (4.0 * (double)(nf - 1)),
            h.first, h.len, m - nf};
}
__device__ __forceinline__ double2 hann_sw(const HannSrc x, int64_t k) {
    const int64_t nf = x.nf;
    const int64_t kp = k + 1 < nf ? k + 1 : 0, km = k > 0 ? k - 1 : nf - 1;
    int64_t qp = kp - x.first, qm = km - x.first, q0 = k - x.first;
    qp += qp < 0 ? nf : 0;
    qm += qm < 0 ? nf : 0;
    q0 += q0 < 0 ? nf : 0;
    const double2 z = make_double2(0.0, 0.0);
    const double2 s = q0 < x.len ? x.S[k] : z, sp = qp < x.len ? x.S[kp] : z,
                  sm = qm < x.len ? x.S[km] : z;
    const float2 cp = x.Y[qp + x.off], cm = x.Y[qm + x.off];
    return make_double2(0.5 * s.x - 0.25 * (sp.x + sm.x) - x.c * ((double)cp.x - (double)cm.x),
                        0.5 * s.y - 0.25 * (sp.y + sm.y) - x.c * ((double)cp.y - (double)cm.y));
}
// h+ = (a + conj b)/2, hx = i (a - conj b)/2 of the windowed spectrum at a bin (a) and at its
// mirror (b)
__device__ __forceinline__ void pol_split(double2 a, double2 b, double2& vp, double2& vc) {
    vp = make_double2(0.5 * (a.x + b.x), 0.5 * (a.y - b.y));
    vc = make_double2(-0.5 * (a.y + b.y), 0.5 * (a.x - b.x));
}
__device__ __forceinline__ void hann_pol(const HannSrc x, int64_t k, double2& vp, double2& vc) {
    pol_split(hann_sw(x, k), hann_sw(x, x.nf - 1 - k), vp, vc);
}
__global__ void k_hann_polarizations(const double2* __restrict__ S, const float2* __restrict__ Y,
                                     const uint64_t* __restrict__ info, int64_t m, int64_t nf,
                                     int64_t k0, double2* __restrict__ hp,
                                     double2* __restrict__ hc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t k = k0 + i;
    if (k >= nf) return;
    double2 vp, vc;
    hann_pol(hann_src(S, 0, Y, info, 0, m, nf), k, vp, vc);
    hp[i] = vp;
    hc[i] = vc;
}

// The pair-form logL kernels' shared pieces (k_hann_loglike_partial, k_cosw_loglike_partial).
// The workgroup's row group and bin chunk: RPT rows per workgroup (rows = RPT x the row groups),
// the row groups of a chunk on consecutive workgroups of one XCD (workgroup b runs on XCD b mod 8)
template <int RPT>
__device__ __forceinline__ void ll_row_group(int rows, int& r0, int& chunk) {
    const int ngr = rows / RPT;
    const int j = (int)(blockIdx.x >> 3);
    r0 = (j % ngr) * RPT;
    chunk = (int)(blockIdx.x & 7) + 8 * (j / ngr);
}
// efd_loglike's terms of one bin (d - h w, product rounded then difference) for both channels
__device__ __forceinline__ void ll_term(double2 d0, double2 d1, double w0, double w1, double2 vp,
                                        double2 vc, double& acc) {
#pragma clang fp contract(off)
    const double x0 = d0.x - vp.x * w0, y0 = d0.y - vp.y * w0;
    const double x1 = d1.x - vc.x * w1, y1 = d1.y - vc.y * w1;
    acc = fma(x0, x0, fma(y0, y0, acc));
    acc = fma(x1, x1, fma(y1, y1, acc));
}
// the workgroup's sum of each of its RPT accumulators: a butterfly over each wave, then the NW
// waves in turn (fixed order); thread q < RPT stores row r0 + q's (HALVE: the local form's 1/2)
// at part[(r0 + q) step + at] when the workgroup has a chunk (ok)
template <int RPT, int NW, bool HALVE>
__device__ __forceinline__ void ll_store(const double* acc, double* __restrict__ part, int r0,
                                         int step, int at, bool ok) {
    __shared__ double red[RPT][NW];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        double a = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = a;
    }
    __syncthreads();
    if (threadIdx.x < RPT && ok) {
        const int q = threadIdx.x;
        double t = red[q][0];
#pragma unroll
        for (int wv = 1; wv < NW; ++wv) t += red[q][wv];
        part[(int64_t)(r0 + q) * step + at] = HALVE ? 0.5 * t : t;
    }
}
// the windowed templates' log-likelihood partials of every row: efd_loglike's terms (d - h w,
// product rounded then difference) for both channels of every bin [k0, nf). One workgroup per
// (bin chunk, row): a thread holds one row's sum (70 VGPRs, 7 waves per SIMD: the loads of many
// waves in flight; the earlier form kept all rows' sums and loads in one thread, 233 VGPRs and
// 2 waves per SIMD, 0.53 of HBM). The rows of a chunk are consecutive workgroups of one XCD
// (workgroup b runs on XCD b mod 8), so d and w (48 B per bin, the same for every row) come from
// HBM once and from that XCD's L2 for the other rows. part[row * nchunk + chunk].
constexpr int HANN_ROWS_MAX = 16;
// RPT rows per workgroup (rows = RPT x the row groups; a thread reads its bin's d and w once
// for all of them: 48 B of the ~176 a bin-row loads from L1/L2). The rows of a chunk's row
// groups are consecutive workgroups of one XCD as with one row each; every row's partial sums
// the same bins in the same order, so the output is bitwise that of RPT = 1.
template <int RPT>
__global__ __launch_bounds__(256) void k_hann_loglike_partial(
    const double2* __restrict__ S, int64_t stride, const float2* __restrict__ Y,
    const uint64_t* __restrict__ info, int64_t m, int64_t nf, int64_t k0,
    const double2* __restrict__ d, const double* __restrict__ w, int rows, int nchunk,
    double* __restrict__ part) {
    int r0, chunk;
    ll_row_group<RPT>(rows, r0, chunk);
    HannSrc x[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) x[q] = hann_src(S, stride, Y, info, r0 + q, m, nf);
    const int64_t nb = nf - k0;
    double acc[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) acc[q] = 0.0;
    for (int64_t i = (int64_t)chunk * 256 + threadIdx.x; i < nb; i += (int64_t)nchunk * 256) {
        const double2 d0 = d[i], d1 = d[nb + i];
        const double w0 = w[i], w1 = w[nb + i];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            double2 vp, vc;
            hann_pol(x[q], k0 + i, vp, vc);
            ll_term(d0, d1, w0, w1, vp, vc, acc[q]);
        }
    }
    ll_store<RPT, 4, false>(acc, part, r0, nchunk, chunk, chunk < nchunk);
}

// ---- Cosine-sum windows (efd_cosw_*; fdutils.CosineWindowConvolution): scipy's symmetric
// w[n] = sum_j (-1)^j a_j cos(2 pi j n / (nf - 1)), j <= J <= 3 (hamming, blackman, nuttall,
// blackmanharris). The Hann expansion at the shifts +-j (1 + e), e = 1 / (nf - 1), with the same
// correction C (the transforms above, unchanged):
//   S_w[k] = a_0 S[k] + sum_j b_j (S[k+j] + S[k-j]) + sum_j b_j j e (C[k+j] - C[k-j]),
//   b_j = (-1)^j a_j / 2, indices mod nf.
// A bin's 2J+1 S and 2J Y neighbours overlap its neighbours' (26 loads a bin pair at J = 3
// against the Hann kernels' 10), so a workgroup stages its tile's bins and their mirrors, each
// with a halo of J, in LDS once (S zeroed outside the row's support as hann_sw reads it; Y at
// hann_sw's index) and every thread takes its neighbours from there.
struct CoswCoef {
    double a0;
    double b[3];   // (-1)^j a_j / 2 for j = 1..3 (0 past J)
    double g[3];   // b_j j / (nf - 1): times the row's scale, the weight of Y[k+j] - Y[k-j]
};
constexpr int COSW_TILE = 256;
template <int J>
struct CoswTile {
    // side 0: bins kb - J + e; side 1: the mirrors, bins nf - kb - COSW_TILE - J + e
    double2 s[2][COSW_TILE + 2 * J];
    float2 y[2][COSW_TILE + 2 * J];
};
// kb: the tile's first bin. A tile's last bins may lie past nf - 1 (and their mirrors below 0):
// such places hold 0 and no thread with a bin reads them. nf >= 2J + 1, so one wrap each way
// brings every neighbour of a bin in [0, nf) back into the grid.
// A thread fetches place threadIdx.x of both sides, and the first 2J lanes of waves 0 and 1 the
// halo place COSW_TILE + lane of side 0 and 1: straight-line loads into registers (cosw_fetch),
// all in flight together, then the LDS stores (cosw_put).
struct CoswRegs {
    double2 s[3];
    float2 y[3];
};
__device__ __forceinline__ void cosw_fetch_one(const double2* __restrict__ S,
                                               const float2* __restrict__ Y, int64_t nf,
                                               int64_t kk, int64_t first, int64_t len,
                                               int64_t off, double2& sv, float2& yv) {
    kk += kk < 0 ? nf : 0;
    kk -= kk >= nf ? nf : 0;
    sv = make_double2(0.0, 0.0);
    yv = make_float2(0.f, 0.f);
    if (kk >= 0 && kk < nf) {
        int64_t q = kk - first;
        q += q < 0 ? nf : 0;
        if (q < len) sv = S[kk];
        yv = Y[q + off];
    }
}
template <int J>
__device__ __forceinline__ void cosw_fetch(CoswRegs& r, const double2* __restrict__ S,
                                           const float2* __restrict__ Y, int64_t nf, int64_t kb,
                                           int64_t first, int64_t len, int64_t off) {
    const int64_t base0 = kb - J, base1 = nf - kb - COSW_TILE - J;
    const int x = threadIdx.x, hs = x >> 6, hl = x & 63;
    cosw_fetch_one(S, Y, nf, base0 + x, first, len, off, r.s[0], r.y[0]);
    cosw_fetch_one(S, Y, nf, base1 + x, first, len, off, r.s[1], r.y[1]);
    if (hs < 2 && hl < 2 * J)
        cosw_fetch_one(S, Y, nf, (hs == 0 ? base0 : base1) + COSW_TILE + hl, first, len, off,
                       r.s[2], r.y[2]);
}
template <int J>
__device__ __forceinline__ void cosw_put(CoswTile<J>& t, const CoswRegs& r) {
    const int x = threadIdx.x, hs = x >> 6, hl = x & 63;
    t.s[0][x] = r.s[0];
    t.y[0][x] = r.y[0];
    t.s[1][x] = r.s[1];
    t.y[1][x] = r.y[1];
    if (hs < 2 && hl < 2 * J) {
        t.s[hs][COSW_TILE + hl] = r.s[2];
        t.y[hs][COSW_TILE + hl] = r.y[2];
    }
}
// S_w of the bin staged at place c (g: CoswCoef.g times the row's scale)
template <int J>
__device__ __forceinline__ double2 cosw_sw(const double2* s, const float2* y, int c,
                                           const CoswCoef& cf, const double* g) {
#pragma clang fp contract(off)
    const double2 s0 = s[c];
    double2 v = make_double2(cf.a0 * s0.x, cf.a0 * s0.y);
#pragma unroll
    for (int j = 1; j <= J; ++j) {
        const double2 sp = s[c + j], sm = s[c - j];
        const float2 yp = y[c + j], ym = y[c - j];
        v.x = (v.x + cf.b[j - 1] * (sp.x + sm.x)) + g[j - 1] * ((double)yp.x - (double)ym.x);
        v.y = (v.y + cf.b[j - 1] * (sp.y + sm.y)) + g[j - 1] * ((double)yp.y - (double)ym.y);
    }
    return v;
}
// hann_pol's split for thread x of a staged tile: bin kb + x (a) and its mirror (b)
template <int J>
__device__ __forceinline__ void cosw_pol(const CoswTile<J>& t, int x, const CoswCoef& cf,
                                         const double* g, double2& vp, double2& vc) {
    pol_split(cosw_sw<J>(t.s[0], t.y[0], x + J, cf, g),
              cosw_sw<J>(t.s[1], t.y[1], COSW_TILE - 1 - x + J, cf, g), vp, vc);
}
template <int J>
__global__ __launch_bounds__(COSW_TILE) void k_cosw_polarizations(
    const double2* __restrict__ S, const float2* __restrict__ Y,
    const uint64_t* __restrict__ info, int64_t m, int64_t nf, int64_t k0, CoswCoef cf,
    double2* __restrict__ hp, double2* __restrict__ hc) {
    __shared__ CoswTile<J> t;
    const int64_t ib = (int64_t)blockIdx.x * COSW_TILE;
    const HannRow h = hann_row(info, 0);
    CoswRegs r;
    cosw_fetch<J>(r, S, Y, nf, k0 + ib, h.first, h.len, m - nf);
    cosw_put<J>(t, r);
    __syncthreads();
    const int64_t i = ib + threadIdx.x;
    if (k0 + i >= nf) return;
    double g[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] = cf.g[j] * h.scale;   // a NaN scale: a NaN row
    double2 vp, vc;
    cosw_pol<J>(t, threadIdx.x, cf, g, vp, vc);
    hp[i] = vp;
    hc[i] = vc;
}
// k_hann_loglike_partial with the general stencil: the same workgroup-to-XCD mapping, row
// groups, term order and reductions; a row's tile is staged by its workgroup alone and its
// partial sums the same bins in the same order whatever RPT and the other rows are.
template <int J, int RPT>
__global__ __launch_bounds__(COSW_TILE) void k_cosw_loglike_partial(
    const double2* __restrict__ S, int64_t stride, const float2* __restrict__ Y,
    const uint64_t* __restrict__ info, int64_t m, int64_t nf, int64_t k0, CoswCoef cf,
    const double2* __restrict__ d, const double* __restrict__ w, int rows, int nchunk,
    double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ CoswTile<J> t[RPT];
    int r0, chunk;
    ll_row_group<RPT>(rows, r0, chunk);
    double g[RPT][3];
    int64_t first[RPT], len[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
        const HannRow h = hann_row(info, r0 + q);
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) g[q][jj] = cf.g[jj] * h.scale;
        first[q] = h.first;
        len[q] = h.len;
    }
    const int64_t nb = nf - k0;
    double acc[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) acc[q] = 0.0;
    // (the tile loop is uniform over the workgroup: the barriers sit outside the bin's test)
    for (int64_t ib = (int64_t)chunk * COSW_TILE; ib < nb; ib += (int64_t)nchunk * COSW_TILE) {
        // the bin's d and w are asked for ahead of the staging, so that their latency runs
        // beside the tile's and not after the barrier
        const int64_t i = ib + threadIdx.x;
        double2 d0 = make_double2(0.0, 0.0), d1 = d0;
        double w0 = 0.0, w1 = 0.0;
        if (i < nb) {
            d0 = d[i];
            d1 = d[nb + i];
            w0 = w[i];
            w1 = w[nb + i];
        }
        CoswRegs r[RPT];
#pragma unroll
        for (int q = 0; q < RPT; ++q)
            cosw_fetch<J>(r[q], S + (int64_t)(r0 + q) * stride, Y + (int64_t)(r0 + q) * m, nf,
                          k0 + ib, first[q], len[q], m - nf);
#pragma unroll
        for (int q = 0; q < RPT; ++q) cosw_put<J>(t[q], r[q]);
        __syncthreads();
        if (i < nb) {
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                double2 vp, vc;
                cosw_pol<J>(t[q], threadIdx.x, cf, g[q], vp, vc);
                ll_term(d0, d1, w0, w1, vp, vc, acc[q]);
            }
        }
        __syncthreads();
    }
    ll_store<RPT, 4, false>(acc, part, r0, nchunk, chunk, chunk < nchunk);
}

// (C) with the windowed logL fused in (efd_hann_loglike_local). Per bin the two channels' terms
// of a bin k and of its mirror k' = nf-1-k combine into one term on each (with the same weight
// w on both channels, p = d0 - w h+, q = d1 - w hx: |p|^2 + |q|^2 = (|p - iq|^2 + |p + iq|^2)/2,
// p - iq = (d0 - i d1) - w S_w[k], p + iq = (d0 + i d1) - w conj(S_w[k'])), so the logL is
//   (1/2) sum_j |dl[j] - wl[j] S_w[j]|^2 over the whole grid
// with dl[k] = d0 - i d1 (k >= k0), dl[k'] = conj(d0 + i d1), wl = w at both (the caller's
// layout: fdutils.HannConvolution.local_data; the self-mirror bin kself takes its second term
// from dl[nf]). Every term is local to its bin, so the inverse column pass reduces them as it
// produces the correction: the correction array is neither written nor read back.
// The pipeline's kernel spectrum carries the difference factor 2i sin(2 pi f / m), so the
// transform yields Dc[s] = Y[s+1] - Y[s-1] directly (no neighbour column needed): valid for
// s in [m - nf, m - 1) when m >= nf + len, and at s = m - 1 (bin u = nf - 1, whose +1 neighbour
// wraps to u = 0) Y[m] = Y[0] differs from C(u = 0) = Y[m - nf] by y[0] (K[(-(m-nf)) mod nf] -
// K[0]) alone (kfix = K[0] - K[(-(m-nf)) mod nf], added back). emit (one row): write
// dl[j] = wl[j] S_w[j] (and dl[nf] = dl[kself]) instead, the data of an injection made by this
// same arithmetic (its logL against itself is then exactly 0).
// Workgroups: 1-D, b -> XCD b mod 8; XCD x takes column blocks [x G/8, (x+1) G/8) and on it the
// rows of one column block are consecutive, so dl / wl (24 B a bin, the same for every row) come
// from HBM once and from the XCD's L2 for the other rows. part[row * G + column block], halved.
// one element of the fused logL: bin offset u >= 0 from the row's first bin, its differenced
// correction dvf (the transform's output), its prefetched data dv and weight w
struct HannLl {
    const double2* Sr;   // the row of S
    int nfi, first, len;
    double cc, scale;    // e / 4 times the row's scale (NaN: aliased row); the scale
    double2 kfix;
    const double2* dl;
    int64_t kself, nf;
    double2* emit;
};
__device__ __forceinline__ void hann_ll_elem(const HannLl& x, int u, fcv dvf, double2 dv, double w,
                                             double& acc) {
#pragma clang fp contract(off)
    const double2 z = make_double2(0.0, 0.0);
    double dx = (double)dvf.x, dy = (double)dvf.y;
    if (u == x.nfi - 1 && x.len > 0) {   // the +1 neighbour wraps: Y[0] -> C(u = 0)
        const double inv = 1.0 / x.scale;
        const double2 s0 = x.Sr[x.first];
        const double yx = s0.x * inv, yy = s0.y * inv;
        dx += yx * x.kfix.x - yy * x.kfix.y;
        dy += yx * x.kfix.y + yy * x.kfix.x;
    }
    int k = u + x.first;
    k -= k >= x.nfi ? x.nfi : 0;
    const int kp = k + 1 < x.nfi ? k + 1 : 0, km = k > 0 ? k - 1 : x.nfi - 1;
    const int qp = u + 1 < x.nfi ? u + 1 : 0, qm = u > 0 ? u - 1 : x.nfi - 1;
    const double2 s = u < x.len ? x.Sr[k] : z, sp = qp < x.len ? x.Sr[kp] : z,
                  sn = qm < x.len ? x.Sr[km] : z;
    const double wx = 0.5 * s.x - 0.25 * (sp.x + sn.x) - x.cc * dx;
    const double wy = 0.5 * s.y - 0.25 * (sp.y + sn.y) - x.cc * dy;
    if (x.emit != nullptr) {
        const double2 o = make_double2(wx * w, wy * w);
        x.emit[k] = o;
        if (k == x.kself) x.emit[x.nf] = o;
        return;
    }
    const double rx = dv.x - wx * w, ry = dv.y - wy * w;
    acc = fma(rx, rx, fma(ry, ry, acc));
    if (k == x.kself) {
        const double2 d2 = x.dl[x.nf];
        const double tx = d2.x - wx * w, ty = d2.y - wy * w;
        acc = fma(tx, tx, fma(ty, ty, acc));
    }
}
// the row's context (hann_row) for hann_ll_elem
__device__ __forceinline__ HannLl hann_ll_ctx(const double2* S, int64_t stride,
                                              const uint64_t* info, int row, int64_t M,
                                              int64_t nf, const double2* dl, int64_t kself,
                                              double2 kfix, double2* emit) {
    const HannRow h = hann_row(info, row);
    HannLl x;
    x.Sr = S + (int64_t)row * stride;
    x.nfi = (int)nf;
    x.first = (int)h.first;
    x.len = (int)h.len;
    // a support longer than m - nf leaves Y[m - nf - 1] aliased: the row's logL is NaN
    x.cc = h.len > M - nf ? __longlong_as_double(0x7ff8000000000000ll)
                          : h.scale / (4.0 * (double)(nf - 1));
    x.scale = h.scale;
    x.kfix = kfix;
    x.dl = dl;
    x.kself = kself;
    x.nf = nf;
    x.emit = emit;
    return x;
}
// (the workgroup's partial is the pair form's ll_store over the 8 waves, halved: part[row G +
// cb]. Its sum starts from the first wave's where this kernel's own epilogue started from 0.0:
// the same bits, since a wave's sum of squares is never -0.0)
template <int R, int C>
__global__ __launch_bounds__(FC_NT) __attribute__((amdgpu_waves_per_eu(4, 8)))
void k_fc_cols_ll(const double2* __restrict__ S, int64_t stride, const uint64_t* __restrict__ info,
                  const float2* __restrict__ Yv, int64_t nf, const double2* __restrict__ dl,
                  const double* __restrict__ wl, int64_t kself, double2 kfix, int rows,
                  double* __restrict__ part, double2* __restrict__ emit) {
#pragma clang fp contract(off)
    constexpr int NCOL = FcCols<R>::NCOL;
    constexpr int64_t M = (int64_t)R * C;
    constexpr int NQ = R * NCOL / FC_NT;
    constexpr int G = C / NCOL;
    __shared__ fcv sm[R * FcColIdx<NCOL>::STRIDE];
    const FcColIdx<NCOL> idx;
    const int row = (int)(blockIdx.x >> 3) % rows, cb = fc_col_block<G>(rows);
    const int c0 = cb * NCOL;
    fc_cols_inverse<R, C>(sm, reinterpret_cast<const fcv*>(Yv) + (int64_t)row * M, c0);
    const HannLl x = hann_ll_ctx(S, stride, info, row, M, nf, dl, kself, kfix, emit);
    const int offi = (int)(M - nf);
    // the elements' data (dl, wl) requested QH at a time before any of them is used: QH loads
    // of each in flight per thread (the epilogue is latency-bound otherwise, one round trip per
    // few elements; all 16 at once spill past 128 VGPRs); indices fit 32 bits (nf < 2^31,
    // m <= 2^25)
    constexpr int QH = NQ >= 8 ? 8 : NQ;
    static_assert(NQ % QH == 0, "whole rounds of prefetched elements");
    double acc = 0.0;
#pragma unroll
    for (int q0 = 0; q0 < NQ; q0 += QH) {
        double2 dv[QH];
        double wv[QH];
#pragma unroll
        for (int t = 0; t < QH; ++t) {
            const int i = threadIdx.x + (q0 + t) * FC_NT;
            const int u = (i / NCOL) * C + c0 + i % NCOL - offi;
            int k = u + x.first;
            k -= k >= x.nfi ? x.nfi : 0;
            dv[t] = make_double2(0.0, 0.0);
            wv[t] = 0.0;
            if (u >= 0) {
                wv[t] = wl[k];
                if (emit == nullptr) dv[t] = dl[k];
            }
        }
#pragma unroll
        for (int t = 0; t < QH; ++t) {
            const int i = threadIdx.x + (q0 + t) * FC_NT;
            const int e = i / NCOL, j = i % NCOL;
            const int u = e * C + c0 + j - offi;   // the correction's bin offset from first
            if (u >= 0) hann_ll_elem(x, u, sm[idx(j, e)], dv[t], wv[t], acc);
        }
    }
    if (emit != nullptr) return;
    ll_store<1, FC_NT / 64, true>(&acc, part, row, G, cb, true);
}

}  // namespace

// ========================================================================================
// Host templates (kernel instances by transform split and stencil width), then the C ABI
// ========================================================================================

// the four-step pipeline for power-of-two m in [2^21, 2^25]: forward columns (staging folded
// in) and rows (the kernel spectrum kfp between the row transforms), then either the inverse
// columns (Y = the correction, efd_hann_convolve) or the inverse columns with the windowed logL
// reduced in place (ll != nullptr: efd_hann_loglike_local)
struct HannLocal {
    const double2* dl;
    const double* wl;
    int64_t kself;
    double2 kfix;
    double* part;
    double2* emit;
};
template <int RR, int CC>
static int hann_pipeline(const double* S, int64_t stride, int64_t nf, int32_t rows,
                         const uint64_t* info, const float* kfp, float* Y, const HannLocal* ll,
                         hipStream_t st) {
    constexpr int NC = FcCols<RR>::NCOL;
    constexpr int64_t M = (int64_t)RR * CC;
    float2* y = (float2*)Y;
    if constexpr (CC == FC_C16) {
        static_assert(RR == FCD_R && NC == FCD_NCOL, "1024 x 16384 split");
        hipLaunchKernelGGL(k_fc_cols1024, dim3(CC / NC, (unsigned)rows), dim3(FC_NT), 0, st,
                           (const double2*)S, stride, info, y);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_fc_rows16k_h, dim3(RR * (unsigned)rows), dim3(FC_NT), 0, st,
                           (const float2*)kfp, M, (int)rows, y);
    } else {
        hipLaunchKernelGGL((k_fc_cols<true, RR, CC>), dim3(CC / NC, (unsigned)rows), dim3(FC_NT),
                           0, st, (const double2*)S, stride, info, y);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_fc_rows, dim3(RR * (unsigned)rows), dim3(FR_NT), 0, st,
                           (const float2*)kfp, M, (int)rows, y);
    }
    HIP_TRY(hipGetLastError());
    if (ll == nullptr) {
        hipLaunchKernelGGL((k_fc_cols<false, RR, CC>), dim3(CC / NC, (unsigned)rows),
                           dim3(FC_NT), 0, st, (const double2*)nullptr, (int64_t)0,
                           (const uint64_t*)nullptr, y);
    } else {
        hipLaunchKernelGGL((k_fc_cols_ll<RR, CC>), dim3((CC / NC) * (unsigned)rows), dim3(FC_NT),
                           0, st, (const double2*)S, stride, info, (const float2*)y, nf, ll->dl,
                           ll->wl, ll->kself, ll->kfix, (int)rows, ll->part, ll->emit);
    }
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}
// The table of four-step splits m = R x C: f(FcSplit<R, C>) for the split of m, false when m has
// none. The row length C is 8192 but at m = 2^24, 1024 x 16384 (the column kernels read 128 B
// segments, r05z; the 2048 x 8192 split measured 1.08 against 0.73 ms of column passes and was
// deleted in round 6). The lag kernel's spectrum is laid out [f_r][f_c] for the same C.
template <int RR, int CC>
struct FcSplit {
    static constexpr int R = RR, C = CC, NCOL = FcCols<RR>::NCOL;
};
template <class F>
static bool fc_split(int64_t m, F f) {
    switch (m) {
        case (int64_t)256 * FC_C: f(FcSplit<256, FC_C>{}); return true;
        case (int64_t)512 * FC_C: f(FcSplit<512, FC_C>{}); return true;
        case (int64_t)1024 * FC_C: f(FcSplit<1024, FC_C>{}); return true;
        case (int64_t)1024 * FC_C16: f(FcSplit<1024, FC_C16>{}); return true;
        case (int64_t)4096 * FC_C: f(FcSplit<4096, FC_C>{}); return true;
        default: return false;
    }
}
static int hann_pipeline_m(const double* S, int64_t stride, int64_t nf, int32_t rows,
                           const uint64_t* info, int64_t m, const float* kfp, float* Y,
                           const HannLocal* ll, hipStream_t st) {
    int rc = EFD_OK;
    if (!fc_split(m, [&](auto s) {
            using T = decltype(s);
            rc = hann_pipeline<T::R, T::C>(S, stride, nf, rows, info, kfp, Y, ll, st);
        }))
        return fail(EFD_ERR_ARG, "efd_hann_convolve: no four-step split for this m");
    return rc;
}

// f(std::integral_constant<int, J>) for the stencil width J = nterm - 1 in 1..3 (cosw_coef has
// checked nterm)
template <class F>
static void cosw_width(int32_t nterm, F f) {
    switch (nterm - 1) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 3>{}); break;
    }
}
// the pair-form logL kernels' launch shape over nb bins, 256 a chunk. np chunks: a multiple of 8
// (one per XCD in turn), at most EFD_LOGLIKE_SCRATCH per row. rpt rows a workgroup: two when the
// rows pair up (d and w read once for both: 362 -> 318 us, r05zr), one for an odd row count.
struct PairShape {
    int np, rpt;
    unsigned blocks;
};
static PairShape pair_shape(int64_t nb, int32_t rows) {
    static_assert(EFD_LOGLIKE_SCRATCH % 8 == 0, "chunks: whole rounds of the 8 XCDs");
    static_assert(COSW_TILE == 256, "one chunk size for both stencils");
    const int np = (int)std::min<int64_t>(EFD_LOGLIKE_SCRATCH, ((nb + 255) / 256 + 7) / 8 * 8);
    const int rpt = (rows % 2 == 0) ? 2 : 1;
    return {np, rpt, (unsigned)(np * (rows / rpt))};
}

extern "C" {

static bool hann_rows_ok(const void* S, int64_t stride, int64_t nf, int32_t rows) {
    return S && nf >= 3 && rows >= 1 && rows <= 65535 && stride >= nf;
}
int efd_hann_extent(const double* S, int64_t stride, int64_t nf, int32_t rows,
                    const int32_t* lanes, uint64_t* info, void* stream) {
    if (!hann_rows_ok(S, stride, nf, rows) || !info)
        return fail(EFD_ERR_ARG, "efd_hann_extent: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hann_info_init, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, st, info,
                       rows);
    HIP_TRY(hipGetLastError());
    // (with lane ranges the rows' supports are a fraction of the grid: fewer workgroups; each
    // block's 3 atomics on its row's words serialise, so the grid stays small -- 512 blocks a
    // row took 94 against 44 us for 32, r05z8 -- and the loop is unrolled for loads in flight)
    const int64_t cap = lanes ? std::max(16, 512 / rows) : std::max(64, 1024 / rows);
    const int64_t blocks = std::min<int64_t>(cap, (nf + 255) / 256);
    hipLaunchKernelGGL(k_hann_extent, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0, st,
                       (const double2*)S, stride, nf, lanes, info);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}
int efd_hann_stage(const double* S, int64_t stride, int64_t nf, int32_t rows,
                   const uint64_t* info, int64_t m, float* Y, void* stream) {
    if (!hann_rows_ok(S, stride, nf, rows) || !info || !Y || m < nf)
        return fail(EFD_ERR_ARG, "efd_hann_stage: bad arguments");
    const int64_t blocks = std::min<int64_t>(4096, (m + 255) / 256);
    hipLaunchKernelGGL(k_hann_stage, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0,
                       (hipStream_t)stream, (const double2*)S, stride, info, m, (float2*)Y);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}
// the four-step split's row length C for a transform length m (fc_split; 8192 where m has none)
int efd_hann_four_step_cols(int64_t m) {
    int c = FC_C;
    fc_split(m, [&](auto s) { c = decltype(s)::C; });
    return c;
}
static bool hann_four_step_m(int64_t m, int64_t nf) {
    return m >= nf && m >= ((int64_t)1 << 21) && m <= ((int64_t)1 << 25) && (m & (m - 1)) == 0;
}
int efd_hann_convolve(const double* S, int64_t stride, int64_t nf, int32_t rows,
                      const uint64_t* info, int64_t m, const float* kfp, float* Y, void* stream) {
    if (!hann_rows_ok(S, stride, nf, rows) || !info || !kfp || !Y ||
        !hann_four_step_m(m, nf))
        return fail(EFD_ERR_ARG, "efd_hann_convolve: bad arguments (m: a power of two in "
                                 "[2^21, 2^25], >= nf)");
    return hann_pipeline_m(S, stride, nf, rows, info, m, kfp, Y, nullptr, (hipStream_t)stream);
}
int efd_hann_loglike_local_partials(int64_t m) {
    int np = 0;   // the split's column blocks
    fc_split(m, [&](auto s) { np = decltype(s)::C / decltype(s)::NCOL; });
    return np;
}
int efd_hann_loglike_local(const double* S, int64_t stride, int64_t nf, int32_t rows,
                           const uint64_t* info, int64_t m, const float* kfd, float* Y,
                           const double* dl, const double* wl, int64_t kself, double* out,
                           double* scratch, double* emit, void* stream) {
    const int np = hann_four_step_m(m, nf) ? efd_hann_loglike_local_partials(m) : 0;
    if (!hann_rows_ok(S, stride, nf, rows) || !info || !kfd || !Y ||
        !wl || np == 0 || kself < -1 || kself >= nf ||
        (emit ? rows != 1 : (!dl || !out || !scratch || rows > HANN_ROWS_MAX)))
        return fail(EFD_ERR_ARG, "efd_hann_loglike_local: bad arguments (m: a power of two in "
                                 "[2^21, 2^25], >= nf; rows <= 16, or 1 with emit)");
    // kfix = K[0] - K[(-(m - nf)) mod nf], K[j] = -i pi/nf + (pi/nf) cot(pi j/nf), K[0] = i pi
    // (nf - 1)/nf (fdutils.HannConvolution.kernel_spectrum's lag kernel)
    const double pn = M_PI / (double)nf;
    const int64_t jw = ((-(m - nf)) % nf + nf) % nf;
    double2 kfix = make_double2(0.0, pn * (double)(nf - 1));
    if (jw != 0) {
        kfix.x -= pn / std::tan(pn * (double)jw);
        kfix.y += pn;
    } else {
        kfix = make_double2(0.0, 0.0);
    }
    hipStream_t st = (hipStream_t)stream;
    const HannLocal ll{(const double2*)dl, wl, kself, kfix, scratch, (double2*)emit};
    const int rc = hann_pipeline_m(S, stride, nf, rows, info, m, kfd, Y, &ll, st);
    if (rc != EFD_OK || emit) return rc;
    efdhip::launch_loglike_final(rows, scratch, np, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}
int efd_hann_polarizations(const double* S, const float* Y, const uint64_t* info, int64_t m,
                           int64_t nf, int64_t k0, double* hp, double* hc, void* stream) {
    if (!S || !Y || !info || !hp || !hc || nf < 3 || m < nf || k0 < 0 || k0 > nf)
        return fail(EFD_ERR_ARG, "efd_hann_polarizations: bad arguments");
    const int64_t cnt = nf - k0;
    if (cnt == 0) return EFD_OK;
    const int threads = 256;
    const int64_t blocks = (cnt + threads - 1) / threads;
    hipLaunchKernelGGL(k_hann_polarizations, dim3((unsigned)blocks), dim3(threads), 0,
                       (hipStream_t)stream, (const double2*)S, (const float2*)Y, info, m, nf, k0,
                       (double2*)hp, (double2*)hc);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}
int efd_hann_loglike(const double* S, int64_t stride, const float* Y, const uint64_t* info,
                     int64_t m, int32_t rows, int64_t nf, int64_t k0, const double* d,
                     const double* w, double* out, double* scratch, void* stream) {
    if (!hann_rows_ok(S, stride, nf, rows) || !Y || !info || !d || !w ||
        !out || !scratch || m < nf || k0 < 0 || k0 >= nf || rows > HANN_ROWS_MAX)
        return fail(EFD_ERR_ARG, "efd_hann_loglike: bad arguments (rows <= 16)");
    const PairShape sh = pair_shape(nf - k0, rows);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sh.rpt == 2 ? k_hann_loglike_partial<2> : k_hann_loglike_partial<1>,
                       dim3(sh.blocks), dim3(256), 0, st, (const double2*)S, stride,
                       (const float2*)Y, info, m, nf, k0, (const double2*)d, w, (int)rows, sh.np,
                       scratch);
    HIP_TRY(hipGetLastError());
    efdhip::launch_loglike_final(rows, scratch, sh.np, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

// the stencil's weights from the window's coefficients a_0..a_J (host doubles)
static bool cosw_coef(const double* a, int32_t nterm, int64_t nf, CoswCoef& cf) {
    if (!a || nterm < 2 || nterm > 4 || nf < 2 * (int64_t)(nterm - 1) + 1) return false;
    cf.a0 = a[0];
    for (int j = 1; j <= 3; ++j) {
        cf.b[j - 1] = j < nterm ? ((j & 1) ? -0.5 : 0.5) * a[j] : 0.0;
        cf.g[j - 1] = cf.b[j - 1] * (double)j / (double)(nf - 1);
    }
    return true;
}
int efd_cosw_polarizations(const double* S, const float* Y, const uint64_t* info, int64_t m,
                           int64_t nf, int64_t k0, const double* a, int32_t nterm, double* hp,
                           double* hc, void* stream) {
    CoswCoef cf;
    if (!S || !Y || !info || !hp || !hc || !cosw_coef(a, nterm, nf, cf) || m < nf || k0 < 0 ||
        k0 > nf)
        return fail(EFD_ERR_ARG, "efd_cosw_polarizations: bad arguments (2 <= nterm <= 4, "
                                 "nf >= 2 (nterm - 1) + 1)");
    const int64_t cnt = nf - k0;
    if (cnt == 0) return EFD_OK;
    const int64_t blocks = (cnt + COSW_TILE - 1) / COSW_TILE;
    hipStream_t st = (hipStream_t)stream;
    cosw_width(nterm, [&](auto j) {
        hipLaunchKernelGGL(k_cosw_polarizations<decltype(j)::value>, dim3((unsigned)blocks),
                           dim3(COSW_TILE), 0, st, (const double2*)S, (const float2*)Y, info, m,
                           nf, k0, cf, (double2*)hp, (double2*)hc);
    });
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}
int efd_cosw_loglike(const double* S, int64_t stride, const float* Y, const uint64_t* info,
                     int64_t m, int32_t rows, int64_t nf, int64_t k0, const double* a,
                     int32_t nterm, const double* d, const double* w, double* out,
                     double* scratch, void* stream) {
    CoswCoef cf;
    if (!hann_rows_ok(S, stride, nf, rows) || !Y || !info || !d || !w ||
        !out || !scratch || !cosw_coef(a, nterm, nf, cf) || m < nf || k0 < 0 || k0 >= nf ||
        rows > HANN_ROWS_MAX)
        return fail(EFD_ERR_ARG, "efd_cosw_loglike: bad arguments (rows <= 16, 2 <= nterm <= 4, "
                                 "nf >= 2 (nterm - 1) + 1)");
    const PairShape sh = pair_shape(nf - k0, rows);
    hipStream_t st = (hipStream_t)stream;
    cosw_width(nterm, [&](auto j) {
        constexpr int J = decltype(j)::value;
        hipLaunchKernelGGL((sh.rpt == 2 ? k_cosw_loglike_partial<J, 2>
                                        : k_cosw_loglike_partial<J, 1>),
                           dim3(sh.blocks), dim3(COSW_TILE), 0, st, (const double2*)S, stride,
                           (const float2*)Y, info, m, nf, k0, cf, (const double2*)d, w, (int)rows,
                           sh.np, scratch);
    });
    HIP_TRY(hipGetLastError());
    efdhip::launch_loglike_final(rows, scratch, sh.np, out, st);
    HIP_TRY(hipGetLastError());
    return EFD_OK;
}

}  // extern "C"
