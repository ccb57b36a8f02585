/*
 * emrifd.h -- C ABI of the MI355X-native FD EMRI mode-sum library (libemrifd.so).
 *
 * Drop-in boundary for the hot path named in BASELINE.json:north_star. In the reference, the
 * FD summation is reached through FastEMRIWaveforms' Python call surface
 *   GenerateEMRIWaveform("FastSchwarzschildEccentricFlux",
 *                        sum_kwargs=dict(pad_output=True, output_type="fd", odd_len=True))
 * (check_mode_by_mode.py:69-83, emri_pe.py:86-105) whose native seam (FEW's Cython wrapper of
 * its FD kernels) is external and absent offline [FEW-ext]. The entry points below are what
 * that seam needs, per SURVEY.md section 8(b):
 *   - efd_spline_build   <- FEW CubicSplineInterpolant build over the sparse trajectory
 *                          (analogue: Tutorial_FD_construction_single_mode.ipynb:558, :594)
 *   - efd_modesum        <- FDInterpolatedModeSum.sum: spline -> SPA per harmonic -> sum over
 *                          harmonics into the two-sided spectrum (notebook :552-623,
 *                          summed over modes; called per waveform at check_mode_by_mode.py:226)
 *   - efd_polarizations  <- the h+/hx split of the 'fd' output (contract
 *                          check_mode_by_mode.py:247: S = h+ - i hx) and mask_positive
 *                          (emri_pe.py:241)
 *   - efd_loglike        <- Likelihood.get_ll's reduction -1/2 * 4 * sum |d - h w|^2
 *                          (LISAanalysistools/lisatools/sampling/likelihood.py:257-274)
 *   - efd_inner_product  <- lisatools inner_product / snr
 *                          (LISAanalysistools/lisatools/diagnostic.py:14-186)
 *
 * Conventions: all arrays are caller-owned DEVICE pointers (HIP, gfx950) unless stated;
 * complex numbers are interleaved (re, im) float64 pairs; every call is asynchronous on the
 * given hipStream_t (NULL = default stream) and never allocates device memory; return value 0
 * on success, negative on error (efd_last_error gives the message). Calls on different
 * streams/devices are independent (no global mutable state except the per-thread error string).
 */
#ifndef EMRIFD_H
#define EMRIFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EFD_OK 0
#define EFD_ERR_ARG (-1)        /* invalid argument (shape, NULL pointer, unsorted grid...)  */
#define EFD_ERR_HIP (-2)        /* HIP runtime error                                          */
#define EFD_ERR_WORKSPACE (-3)  /* workspace smaller than efd_modesum_workspace_bytes()     */

#define EFD_CAUSTIC_SPA 0       /* plain stationary phase: Q = e^{i sgn(F') 3pi/4} / sqrt|F'| */
#define EFD_CAUSTIC_UNIFORM 1   /* notebook K_{1/3} uniform form (notebook :599-613)          */

/* Library version (major*10000 + minor*100 + patch). */
int efd_version(void);

/* The source hash the library was built from (16 hex digits of the SHA-256 over its sources,
 * emri_frequencydomainwaveforms_amd/_build.py source_id), or "unversioned". Static storage. */
const char* efd_build_id(void);

/* Copies the last error message of the calling thread into buf (NUL-terminated). */
int efd_last_error(char* buf, int len);

/*
 * Batched not-a-knot cubic splines on shared knots x[n] (n >= 2, strictly increasing):
 * y is knot-major [n][ninterp]; coef is written as [n-1][4][ninterp] in scipy PPoly order
 * (c0 highest power): y(x) = ((c0 w + c1) w + c2) w + c3, w = x - x[i].
 * Matches scipy.interpolate.CubicSpline(x, y, bc_type='not-a-knot') including its n = 2
 * (line) and n = 3 (parabola) special cases. One lane per interpolant.
 */
int efd_spline_build(const double* x, int n, const double* y, int ninterp, double* coef,
                     void* stream);

/* Input of one FD mode sum (one waveform). */
typedef struct efd_modesum_args {
    /* sparse trajectory knots, length nt (device) */
    const double* t;          /* [nt] seconds, strictly increasing                           */
    const double* phi_phi;    /* [nt] azimuthal phase                                        */
    const double* phi_r;      /* [nt] radial phase                                           */
    const double* f_phi;      /* [nt] Omega_phi / (2 pi M MTSUN_SI) [Hz]                     */
    const double* f_r;        /* [nt] Omega_r / (2 pi M MTSUN_SI) [Hz]                       */
    int32_t nt;
    /* harmonics (device) */
    const double* amp;        /* complex [nt][K]: Teukolsky amplitude A_k(t_i) (FEW layout)  */
    const int32_t* m;         /* [K] 0 <= m <= 255; m > 0 adds the -m partner branch          */
    const int32_t* n;         /* [K] |n| <= 1023                                              */
    const double* ylm_p;      /* complex [K]: Y_lm                                            */
    const double* ylm_m;      /* complex [K]: (-1)^l Y_{l,-m} (ignored for m = 0)             */
    int32_t K;                /* 1 <= K <= 8192                                               */
    /* frequency grid (device), ascending */
    const double* freq;       /* [nf]                                                         */
    int64_t nf;
    int32_t grid_symmetric;   /* 1 iff freq[nf-1-k] == -freq[k] for all k (mirror pairing)    */
    /* scaling: S *= scale (complex), e.g. mu MRSUN_SI/(dist Gpc) * e^{-2 i psi_pol}           */
    double scale_re, scale_im;
    int32_t caustic;          /* EFD_CAUSTIC_*                                                */
    int32_t accumulate;       /* 1: outputs += new values, 0: outputs = new values            */
    double* out;              /* complex [nf] (device): FEW 'fd' spectrum S = h+ - i hx, or
                               * NULL when only hp/hc are wanted                               */
    /* optional hipEvent_t pair recorded on `stream` around the mode-sum kernel alone (K8), for
     * roofline timing; NULL = not recorded */
    void* prof_begin;
    void* prof_end;
    /* optional fused polarisations (symmetric grids only): complex [nf - k0] each, written as
     * efd_polarizations(S, nf, k0, hp, hc) would, from the registers that hold S (no S round
     * trip through HBM). NULL = not written. */
    double* hp;
    double* hc;
    int64_t k0;
} efd_modesum_args;

/* Bytes of device workspace efd_modesum needs for (nt, K, nf), valid for either grid kind;
 * 0 for an invalid shape (nt < 2 or nt > 1024, K <= 0, nf <= 0). Host-only query. */
size_t efd_modesum_workspace_bytes(int32_t nt, int32_t K, int64_t nf);

/*
 * Full FD mode sum: (m, n) grouping -> spline build (trajectory; group amplitudes
 * sum_l Y A_lmn) -> per-group t(f) inverse splines -> interval records ->
 * segment table -> SPA evaluation with output-stationary accumulation (each tile of frequency
 * bins builds its own record list in LDS). Asynchronous, allocation-free, no host sync, no
 * atomics on the spectrum; bitwise reproducible.
 */
int efd_modesum(const efd_modesum_args* a, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same call in two phases on possibly different streams (the caller orders them, e.g. with
 * an event): _prepare runs everything up to the tiles' record lists (grouping, splines,
 * inverse splines, interval records, segment table, per-tile key lists and the tiles'
 * longest-first dispatch order; latency-bound),
 * _sum the mode-sum kernel (reads
 * freq, writes out / hp / hc). With two workspaces, waveform i+1's prepare overlaps waveform
 * i's sum. efd_modesum == _prepare then _sum on one stream.
 */
int efd_modesum_prepare(const efd_modesum_args* a, void* workspace, size_t workspace_bytes,
                        void* stream);
int efd_modesum_sum(const efd_modesum_args* a, void* workspace, size_t workspace_bytes,
                    void* stream);

/*
 * _sum for `count` prepared waveforms in one kernel launch (1 <= count <= EFD_BATCH_MAX): the
 * waveforms' tiles interleave in one longest-first dispatch, so the launch's ramp, tail and the
 * gap between launches are shared (a batch of walkers in a likelihood, or of templates). a[i] and
 * workspace[i] are exactly what efd_modesum_sum would take for waveform i (each prepared by
 * efd_modesum_prepare on its own workspace); every a[i] must agree on nf, grid_symmetric, caustic
 * and accumulate. Each waveform's outputs are bitwise those of its own efd_modesum_sum. The
 * profiling events of a[0] bracket the launch; efd_modesum_status / _stats work per workspace.
 * Not part of the reference's interface: an extension for its batched callers.
 */
#define EFD_BATCH_MAX 16
int efd_modesum_sum_batch(const efd_modesum_args* const* a, void* const* workspace,
                          const size_t* workspace_bytes, int32_t count, void* stream);

/*
 * efd_modesum_prepare for `count` waveforms (1 <= count <= EFD_BATCH_MAX) in one chain of
 * launches: each preparation kernel runs once for the batch, its grid's z index picking the
 * waveform (one waveform's launches cost ~10 us of host time and as many dispatches; a
 * likelihood's walker batch pays them once). a[i], workspace[i] are what efd_modesum_prepare
 * would take for waveform i; every a[i] must agree on nf and grid_symmetric and each waveform
 * needs its own workspace. Each workspace ends up bitwise as after its own efd_modesum_prepare
 * (which is this call with count = 1). Not part of the reference's interface: an extension for
 * its batched callers (Likelihood over a walker batch, likelihood.py:246-274).
 */
int efd_modesum_prepare_batch(const efd_modesum_args* const* a, void* const* workspace,
                              const size_t* workspace_bytes, int32_t count, void* stream);

/*
 * efd_modesum_sum_batch with the Gaussian log-likelihood of each waveform fused into the mode
 * sum's epilogue (Likelihood.get_ll over a batch of walkers, likelihood.py:246-274):
 *   out[i] = -1/2 * 4 * sum_c sum_j | d[c][j] - h_c,i[j] * w[c][j] |^2,  c in {+, x},
 *   j over the bins [k0, nf) of the symmetric grid (c = + is h+, c = x is hx, as the fused
 *   polarisations would write them), d complex [2][nf - k0], w real [2][nf - k0]
 * (efd_loglike's terms and rounding), without writing the templates: the registers that hold
 * S(k), S(nf-1-k) feed the reduction, so h+/hx never go through HBM. Every a[i] needs
 * grid_symmetric = 1, accumulate = 0 and the same k0; hp/hc/out of a[i] are still written when
 * non-NULL. out: count device doubles. Per-tile partials live in each workspace; the final
 * reduction has a fixed order (bitwise reproducible; equal to efd_loglike on the written
 * templates to rounding). A waveform whose workspace holds a device-side error flag (see
 * efd_modesum_status) gets out[i] = NaN, and its flags stay set: a caller that finds no NaN
 * needs no status synchronisation, one that does calls efd_modesum_status_batch for the
 * message. An extension for batched likelihood callers.
 */
int efd_modesum_sum_loglike(const efd_modesum_args* const* a, void* const* workspace,
                            const size_t* workspace_bytes, int32_t count, const double* d,
                            const double* w, double* out, void* stream);

/*
 * The fused likelihood's per-tile constants: for each tile of the symmetric grid's paired layout
 * (efd_loglike_tile_count(nf) tiles), that tile's partial of efd_modesum_sum_loglike's sum when
 * the template is zero on all of its bins. They depend on (d, w, nf, k0) only, so a likelihood
 * computes them once; efd_modesum_sum_loglike_ex then gives a tile no harmonic reaches this value
 * instead of re-reading d and w there (at a high f_max most tiles of a sparse spectrum are empty).
 * The result is bitwise efd_modesum_sum_loglike's: the constants are that epilogue's arithmetic on
 * zero sums. tile_const: efd_loglike_tile_count(nf) device doubles. Extensions for batched
 * likelihood callers (likelihood.py:246-274).
 */
int64_t efd_loglike_tile_count(int64_t nf);
int efd_loglike_tile_constants(const double* d, const double* w, int64_t nf, int64_t k0,
                               double* tile_const, void* stream);

/* efd_modesum_sum_loglike with the constants of efd_loglike_tile_constants for the same d, w,
 * nf and k0 (tile_const NULL: efd_modesum_sum_loglike). */
int efd_modesum_sum_loglike_ex(const efd_modesum_args* const* a, void* const* workspace,
                               const size_t* workspace_bytes, int32_t count, const double* d,
                               const double* w, const double* tile_const, double* out,
                               void* stream);

/*
 * <d|h> and <h|h> of each waveform from the mode sum's epilogue, the templates again never
 * written (Likelihood.parts; lisatools' separate_d_h pair, inner_product(d, h, complex=True)'s
 * convention, diagnostic.py:103-110). With hw = h_c[j] * w[c][j] (each component's product
 * rounded, efd_loglike's rule) and dv = d[c][j], per bin and channel, as written (no contraction):
 *   t_re = fma(dv.x, hw.x, dv.y * hw.y)
 *   t_im = dv.x * hw.y - dv.y * hw.x      (two rounded products and their difference)
 *   t_hh = fma(hw.x, hw.x, hw.y * hw.y)
 *   out[3 i + 0] = Re <d|h> = 4 sum t_re,  out[3 i + 1] = Im <d|h> = 4 sum t_im,
 *   out[3 i + 2] = <h|h> = 4 sum t_hh,  so that logL = -1/2 (<d|d> - 2 Re <d|h> + <h|h>).
 * The three sums take their terms in the same order: a d equal to h w bit for bit gives
 * Re <d|h> == <h|h> bitwise and Im <d|h> == 0.0. a, workspace, d, w: efd_modesum_sum_loglike's,
 * with its argument checks; w must be finite (a zero weight drops a bin). part: caller-owned
 * device doubles [count][3][efd_loglike_tile_count(nf)] for the tiles' partials; every entry the
 * call reads it has written itself. A tile no harmonic reaches adds exactly 0, so the sparse
 * launch (only the tiles of each waveform's lane range; taken under efd_modesum_sum_loglike_ex's
 * rule, without needing constants) equals the dense one bitwise; flags bit 0 forces the dense
 * launch. Fixed reduction orders: bitwise reproducible, and a waveform's numbers do not depend
 * on the batch around it. A waveform whose workspace holds a device-side error flag gets three
 * NaN and keeps its flags (efd_modesum_status_batch). out: [count][3] device doubles.
 */
int efd_modesum_sum_dh_hh(const efd_modesum_args* const* a, void* const* workspace,
                          const size_t* workspace_bytes, int32_t count, const double* d,
                          const double* w, double* part, int32_t flags, double* out,
                          void* stream);

/* Synchronises `stream` and reports errors detected on the device by the calls on this
 * workspace since the previous efd_modesum_status (the flags are sticky across preparations, so
 * a workspace reused by several waveforms before its status is read loses none): a harmonic
 * with more than 8 monotonic frequency runs, or |m| > 255 or |n| > 1023 -> EFD_ERR_ARG; a tile
 * dispatch-order entry out of range in the sum (its bins left unwritten, e.g. a sum run on a
 * workspace another call prepared) -> EFD_ERR_HIP. Reported flags are cleared. */
int efd_modesum_status(const void* workspace, void* stream);

/* Each workspace's lane range [lane_lo, lane_hi) after its preparation: the union of its
 * harmonics' segment lane ranges (on symmetric grids lane l is bin l and its mirror nf-1-l; no
 * term reaches a bin outside), into out[2 i], out[2 i + 1] (device int32), stream-ordered. */
int efd_modesum_lane_ranges(void* const* workspace, int32_t count, int32_t* out, void* stream);

/*
 * efd_modesum_status for `count` workspaces (1 <= count <= EFD_BATCH_MAX) used on `stream`: one
 * gather launch and one synchronisation for a walker batch. flags (optional, int32[count])
 * receives each workspace's error bits (1: more than 8 monotonic runs, 2: |m| > 255 or
 * |n| > 1023, 4: tile dispatch-order entry out of range); the return value and efd_last_error
 * report the first failing waveform. Reported flags are cleared, as by efd_modesum_status.
 */
int efd_modesum_status_batch(void* const* workspace, int32_t count, int32_t* flags,
                             void* stream);

/* Contributions C (harmonic branch x bin pairs, the reference's per-(l, m, n) formulation) of
 * the last efd_modesum on this workspace (for the roofline); synchronises `stream`. */
int efd_modesum_contributions(const void* workspace, int64_t* contributions, void* stream);

/* Statistics of the last efd_modesum on this workspace; synchronises `stream`. contributions as
 * above; evaluations = SPA evaluations actually made (one per (m, n) group branch x bin: every
 * l of a group shares t(f), the phase and the K_{1/3} factor); groups = distinct (m, n).
 * NULL outputs are skipped. */
int efd_modesum_stats(const void* workspace, int64_t* contributions, int64_t* evaluations,
                      int32_t* groups, void* stream);

/* Of those evaluations, the ones made on envelope records (the records whose SPA amplitude and
 * K_{1/3} phase k_items carries as polynomials in t); synchronises `stream`.
 * An extension for the roofline accounting, not part of the reference's interface. */
int efd_modesum_env_evaluations(const void* workspace, int64_t* env_evaluations, void* stream);

/* Input of one time-domain mode sum (one waveform). */
typedef struct efd_td_args {
    /* sparse trajectory knots, length nt (device); as efd_modesum_args */
    const double* t;
    const double* phi_phi;
    const double* phi_r;
    const double* f_phi;
    const double* f_r;
    int32_t nt;
    /* harmonics (device); as efd_modesum_args */
    const double* amp;
    const int32_t* m;
    const int32_t* n;
    const double* ylm_p;
    const double* ylm_m;
    int32_t K;
    /* samples t_i = i dt, 0 <= i < nsamples; zero where t_i > t[nt-1] (FEW pad_output) */
    double dt;
    int64_t nsamples;
    double scale_re, scale_im;  /* h *= scale (complex)                                        */
    int32_t accumulate;         /* 1: outputs += new values, 0: outputs = new values           */
    double* out;                /* complex [nsamples] h = h+ - i hx, or NULL                    */
    double* hp;                 /* real [nsamples] h+, or NULL                                  */
    double* hc;                 /* real [nsamples] hx, or NULL                                  */
    void* prof_begin;           /* optional hipEvent_t pair around the TD kernel alone          */
    void* prof_end;
} efd_td_args;

/* Bytes of device workspace efd_td_modesum needs for (nt, K); 0 for an invalid shape. */
size_t efd_td_workspace_bytes(int32_t nt, int32_t K);

/*
 * Time-domain mode sum <- FEW InterpolatedModeSum, the TD generator the reference compares its
 * FD waveform against (td_gen: check_mode_by_mode.py:85-99, 254-264; Tutorial_FrequencyDomain_
 * Waveforms.ipynb:61-66, 184-188):
 *   h(t_i) = scale * sum_k [ Y+_k A_k(t_i) e^{-i Phi_k(t_i)} + (m_k > 0) Y-_k conj(A_k(t_i))
 *            e^{+i Phi_k(t_i)} ],  Phi_k = m Phi_phi + n Phi_r,
 * with not-a-knot cubic splines of A_k, Phi_phi, Phi_r over the knots. Its DFT,
 * fftshift(fft(h)) dt, is the FD spectrum efd_modesum returns. Asynchronous, allocation-free;
 * efd_modesum_status works on this workspace too.
 */
int efd_td_modesum(const efd_td_args* a, void* workspace, size_t workspace_bytes, void* stream);

/*
 * efd_td_modesum with a time-domain window: every stored sample (out, hp and hc alike) is
 * multiplied by window[s] (real doubles [nsamples], device) in the store epilogue; with
 * accumulate the outputs += window * new values. window = NULL is efd_td_modesum, bitwise (the
 * same kernel instantiation). The windowed series is what the reference transforms in
 * FDutils.get_fft_td_windowed (:49-64: fft(h * window)); any window takes this path.
 */
int efd_td_modesum_windowed(const efd_td_args* a, const double* window, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * The two channels of a TD template's transform <- get_fd_waveform_fromTD (FDutils.py:142-178:
 * fftshift(fft(h+ w)) dt and fftshift(fft(hx w)) dt over frequency >= 0). The TD sum writes
 * h = h+ - i hx as one complex series, so ONE complex transform Z = fft(w h) holds both:
 *   H+[k] = (Z[k] + conj Z[(n-k) mod n]) / 2,   Hx[k] = i (Z[k] - conj Z[(n-k) mod n]) / 2,
 * and the drivers' positive-frequency mask on the shifted grid is the natural-order bins
 * k = 0 .. nb - 1, nb = (n + 1) / 2 (even n: no Nyquist bin, it sits on the negative side; bin 0
 * pairs with itself). Row r of Z: complex [n] in natural DFT order at Z + 2 r stride doubles
 * (stride >= n). Asynchronous, allocation-free; EFD_ERR_ARG before any launch for NULL pointers
 * or size errors.
 *   efd_td_split: row r's block complex [2][nb] at out + 2 r out_stride doubles (out_stride >=
 *     2 nb): channel 0 = gain H+, channel 1 = gain Hx; bins with keep[k] == 0 (bytes [nb], or
 *     NULL: keep all) are written as exact zeros.
 *   efd_td_split_loglike: out[r] = -1/2 * 4 * sum_c sum_k | d[c][k] - h_r[c][k] w[c][k] |^2 with
 *     h_r what efd_td_split would write (never stored; the same arithmetic, and efd_loglike's
 *     rounding of d - h w); d complex [2][nb] and w real [2][nb], shared by the rows; scratch
 *     holds rows * EFD_TD_SPLIT_SCRATCH device doubles. The partition depends on n only and the
 *     final reduction has a fixed order: bitwise reproducible, no atomics. A NaN anywhere in a
 *     row of Z makes that row's out NaN.
 */
#define EFD_TD_SPLIT_SCRATCH 1024
int efd_td_split(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                 const uint8_t* keep, double* out, int64_t out_stride, void* stream);
int efd_td_split_loglike(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                         const double* d, const double* w, double* out, double* scratch,
                         void* stream);

/*
 * Asynchronous host -> device copy of `bytes` from `src` (pinned host memory) to `dst` on
 * `stream`: the input upload of a waveform on a pipeline slot's stream, issued through this
 * library's HIP runtime (no host synchronisation). Plumbing for the Python host layer.
 */
int efd_upload(void* dst, const void* src, size_t bytes, void* stream);

/* Host plumbing for batched callers: `bytes` from device memory into (pinned) host memory,
 * asynchronous on `stream` (hipMemcpyAsync). */
int efd_download(void* dst, const void* src, size_t bytes, void* stream);

/* Host plumbing: the `count` streams dst[i] wait for the work queued so far on stream `src`
 * (one event record, one stream wait each; nothing blocks the host). The library's event is
 * per thread and device and re-recorded by each call; waits already enqueued are unaffected. */
int efd_stream_order(void* src, void* const* dst, int32_t count);

/*
 * h+ = (S(f) + conj(S_flip))/2, hx = i (S(f) - conj(S_flip))/2 with S_flip the array reversed
 * (FEW list output). Writes bins [k0, nf) of each (k0 = first bin to keep, e.g. the f >= 0
 * bin for mask_positive) into hp, hc (complex [nf - k0]).
 */
int efd_polarizations(const double* S, int64_t nf, int64_t k0, double* hp, double* hc,
                      void* stream);

/*
 * The spectrum convolved with the reference's Hann window (FDutils.py:66-101 get_fd_windowed
 * with emri_pe.py:261's scipy hann(nf), sym=True) without size-nf DFTs: the windowed spectrum is
 *   S_w[k] = S[k]/2 - (S[k+1] + S[k-1])/4 - (C[k+1] - C[k-1]) / (4 (nf - 1)),   indices mod nf,
 * C = K (*) S the circular convolution with K[m] = -i pi/nf + (pi/nf) cot(pi m/nf),
 * K[0] = i pi (nf-1)/nf (the derivative of the DFT's trigonometric interpolant). C is the caller's
 * linear convolution of each row's support with K on m-point complex64 transforms
 * (fdutils.HannConvolution): rows of S (complex128 [nf], row r at S + 2 r stride doubles);
 * info[r] (4 x uint64 per row, device) = {bits of scale = max(|Re|, |Im|) over the row, first
 * nonzero bin, last nonzero bin + 1, 0} (first = ~0, last = 0 for an all-zero row; a NaN makes
 * the scale NaN); Y complex64 [rows][m], m >= nf + (last - first) - 1.
 *   efd_hann_extent: info from S. lanes (NULL, or device int32 [rows][2] from
 *                    efd_modesum_lane_ranges on the rows' workspaces, symmetric grids): only
 *                    the bins those lanes and their mirrors cover are read.
 *   efd_hann_stage:  Y[r][s] = S[r][first + s] / scale for s < last - first, 0 up to m. The
 *                    caller transforms Y in place: forward, times the lag kernel's spectrum
 *                    (z[t] = K[(t - (m - nf)) mod nf] / m), backward; then
 *                    C[k] = scale Y[r][((k - first) mod nf) + m - nf].
 *   efd_hann_polarizations: h+/hx (efd_polarizations' split) of one row's S_w over bins
 *                    [k0, nf) into hp, hc (complex [nf - k0]).
 *   efd_hann_loglike: efd_loglike of every row's windowed h+/hx against d, w ([2][nf - k0],
 *                    efd_loglike's layout and rounding), out[r] (device doubles [rows],
 *                    rows <= 16); scratch holds rows * EFD_LOGLIKE_SCRATCH doubles. No template
 *                    is written.
 * Replaces: no reference function (the reference convolves each channel with scipy/cupy at
 * FDutils.py:35-47, 95-96).
 */
int efd_hann_extent(const double* S, int64_t stride, int64_t nf, int32_t rows,
                    const int32_t* lanes, uint64_t* info, void* stream);
int efd_hann_stage(const double* S, int64_t stride, int64_t nf, int32_t rows,
                   const uint64_t* info, int64_t m, float* Y, void* stream);
/* efd_hann_stage + the caller's transform pair in one call, for power-of-two m in [2^21, 2^25]
 * (a four-step FFT: column FFTs of length R = m / C with the staging folded in, row FFTs of
 * C with the kernel multiply between forward and inverse, inverse column FFTs; the spectrum is
 * never reordered; C = efd_hann_four_step_cols(m)). kfp: the lag kernel's spectrum / m,
 * complex64 in the four-step order kfp[f_r C + f_c] = kf[f_r + R f_c]. Leaves Y as
 * efd_hann_stage + transforms do. */
int efd_hann_convolve(const double* S, int64_t stride, int64_t nf, int32_t rows,
                      const uint64_t* info, int64_t m, const float* kfp, float* Y, void* stream);
/* The four-step split's row length C that efd_hann_convolve uses for transform length m
 * (R = m / C; kfp's layout above with 8192 replaced by C): 16384 at m = 2^24, else 8192. */
int efd_hann_four_step_cols(int64_t m);
/* The windowed logL with the correction reduced inside efd_hann_convolve's inverse column pass
 * (no correction array written or read back): the reference's per-channel window convolution
 * (FDutils.py:95-96 under emri_pe.py:259-263) followed by Likelihood.get_ll's reduction
 * (likelihood.py:257-274), for a walker group. With the same weight w on both channels the two
 * channels' terms of a kept bin k and of its mirror k' = nf-1-k recombine into one term per bin:
 *   sum_k |d0 - w h+|^2 + |d1 - w hx|^2 = (1/2) sum_j |dl[j] - wl[j] S_w[j]|^2,
 * dl[k] = d0[k] - i d1[k], dl[k'] = conj(d0[k] + i d1[k]), wl = w at both (complex128 [nf + 1]
 * and float64 [nf]; the self-mirror bin kself, or -1, takes its second term from dl[nf]; other
 * bins hold 0). kfd: kfp times 2i sin(2 pi f / m) (the transforms then give the correction's
 * difference C[k+1] - C[k-1] directly); m >= nf + the rows' longest support (a longer support
 * makes the row's logL NaN). out[r] = -2 sum (efd_hann_loglike's value, up to rounding);
 * scratch: rows * efd_hann_loglike_local_partials(m) (<= 4096) doubles. emit (device complex128
 * [nf + 1], rows = 1; dl, out, scratch unused): writes wl[j] S_w[j] (and emit[nf] at kself)
 * instead, the dl of an injection made by this same arithmetic: the logL of the same spectrum
 * against it is exactly 0. */
int efd_hann_loglike_local(const double* S, int64_t stride, int64_t nf, int32_t rows,
                           const uint64_t* info, int64_t m, const float* kfd, float* Y,
                           const double* dl, const double* wl, int64_t kself, double* out,
                           double* scratch, double* emit, void* stream);
/* The partial sums per row efd_hann_loglike_local writes at transform length m (0: not a
 * four-step length). */
int efd_hann_loglike_local_partials(int64_t m);
int efd_hann_polarizations(const double* S, const float* Y, const uint64_t* info, int64_t m,
                           int64_t nf, int64_t k0, double* hp, double* hc, void* stream);
/*
 * The same for scipy's other symmetric cosine-sum windows (the reference's mode-by-mode driver
 * windows its FD templates with blackman, hann and nuttall, check_mode_by_mode.py:269-272, and
 * imports hamming and blackmanharris):
 *   w[n] = sum_{j=0..J} (-1)^j a_j cos(2 pi j n / (nf - 1)),   J = nterm - 1 in 1..3.
 * The Hann expansion at the shifts +-j (1 + e), e = 1 / (nf - 1), with the same C (and so the
 * same info, Y and m: efd_hann_extent, efd_hann_stage / efd_hann_convolve serve every window):
 *   S_w[k] = a_0 S[k] + sum_{j=1..J} (-1)^j (a_j / 2) [ S[k+j] + S[k-j]
 *                                                     + j e (C[k+j] - C[k-j]) ],  indices mod nf.
 * a = (1/2, 1/2) is the Hann form above. The dropped second-order term is within 10 q / nf^2 of
 * max|S|, q = sum_j a_j j^2 (Hann: 5 / nf^2). a: nterm host doubles a_0..a_J, 2 <= nterm <= 4;
 * nf >= 2 (nterm - 1) + 1 (every neighbour wraps at most once), else EFD_ERR_ARG.
 *   efd_cosw_polarizations: efd_hann_polarizations with this stencil (one row).
 *   efd_cosw_loglike: efd_hann_loglike with this stencil (rows <= 16, the same scratch, term
 *                    order and reductions; a row's value does not depend on the other rows of
 *                    the call).
 */
int efd_cosw_polarizations(const double* S, const float* Y, const uint64_t* info, int64_t m,
                           int64_t nf, int64_t k0, const double* a, int32_t nterm,
                           double* hp, double* hc, void* stream);
int efd_cosw_loglike(const double* S, int64_t stride, const float* Y, const uint64_t* info,
                     int64_t m, int32_t rows, int64_t nf, int64_t k0, const double* a,
                     int32_t nterm, const double* d, const double* w, double* out,
                     double* scratch, void* stream);

/*
 * Fused Gaussian log-likelihood over nchan channels of nbin bins each:
 *   out = -1/2 * 4 * sum_c sum_k | d[c][k] - h[c][k] * w[c][k] |^2
 * (likelihood.py:257-274 with noise factor w = sqrt(df/S) built at likelihood.py:213-220).
 * h, d complex [nchan][nbin]; w real [nchan][nbin]; out is one device double; scratch holds
 * EFD_LOGLIKE_SCRATCH device doubles. h = NULL gives the data-only term -2 sum |d|^2.
 * Bitwise reproducible (fixed partition and reduction order).
 */
#define EFD_LOGLIKE_SCRATCH 1024
int efd_loglike(const double* h, const double* d, const double* w, int32_t nchan, int64_t nbin,
                double* out, double* scratch, void* stream);
/* the windowed log-likelihood of rows of spectra (see efd_hann_extent above) */
int efd_hann_loglike(const double* S, int64_t stride, const float* Y, const uint64_t* info,
                     int64_t m, int32_t rows, int64_t nf, int64_t k0, const double* d,
                     const double* w, double* out, double* scratch, void* stream);

/*
 * Noise-weighted inner product over nchan channels of nbin bins each:
 *   out[0] + i out[1] = 4 * sum_c sum_k conj(a[c][k]) * b[c][k] * w[c][k]
 * (lisatools diagnostic.py:95-110: right-sum rule, w = diff(f) / PSD with the first spacing
 * repeated; inner_product takes out[0], or both parts with complex=True). a, b complex
 * [nchan][nbin]; w real [nchan][nbin] or NULL (w = 1); out is two device doubles; scratch
 * holds EFD_INNER_SCRATCH device doubles. Bitwise reproducible.
 */
#define EFD_INNER_SCRATCH 2048
int efd_inner_product(const double* a, const double* b, const double* w, int32_t nchan,
                      int64_t nbin, double* out, double* scratch, void* stream);

/*
 * Weighted Gram matrix of stencil-combined rows in one pass: the reduction of lisatools' fisher
 * (diagnostic.py:300-386: dh_dlambda's central differences :263-267, :294, then inner_product of
 * every pair of derivatives :373-381).
 *   D_i[e] = sum_s coef[i][s] * h[i npoint + s][e]      (ascending s, per element, in registers)
 *   gram[i][j] = 4 * sum_e w[e] * Re(conj(D_i[e]) D_j[e])
 * h: nparam * npoint complex rows of nelem elements (nelem = nchan * nbin flattened, as
 * efd_inner_product's operands), row r at h + 2 r row_stride doubles, row_stride >= nelem, h
 * 16-byte aligned; npoint in {1, 2, 4} (npoint = 1, coef = 1: the Gram matrix of the rows as
 * given); coef: HOST doubles [nparam][npoint]; w: real [nelem] or NULL (w = 1); gram: doubles
 * [nparam][nparam], full and exactly symmetric; dh: NULL, or complex [nparam][nelem]
 * (contiguous rows) receiving D_i from the registers that feed the products; scratch:
 * EFD_FISHER_SCRATCH device doubles. The stencil is applied before the products: the Gram
 * matrix of the raw rows combined afterwards is the same algebra and loses the digits the
 * differences cancel. Every element of h and w is read once. No atomics: a fixed partition that
 * depends on nelem only and a fixed-order final reduction, so results are bitwise reproducible,
 * and gram[i][j] is bitwise what the same two parameter blocks give in any other call over the
 * same w and nelem (a subset of the parameters, another order). EFD_ERR_ARG before any launch:
 * nparam outside 1..EFD_FISHER_MAX_PARAMS, npoint not 1, 2 or 4, NULL h, coef, gram or scratch,
 * nelem <= 0, row_stride < nelem.
 */
#define EFD_FISHER_MAX_PARAMS 16
#define EFD_FISHER_SCRATCH 139264
int efd_fisher_gram(const double* h, int64_t row_stride, int32_t nparam, int32_t npoint,
                    const double* coef, const double* w, int64_t nelem, double* dh, double* gram,
                    double* scratch, void* stream);

/*
 * Overlaps of many rows with one fixed waveform in one pass: the reduction of lisatools'
 * mismatch_criterion / vallisneri_criterion_cdf (diagnostic.py:489-757: every perturbed
 * waveform's normalised overlap with h_true, :622-638) and of cutler_vallisneri_bias
 * (:812-823: <dh_k | h_true - h_approx>, the difference formed on the fly).
 *   r[e]        = t[e] - u[e]                       (u == NULL: r = t)
 *   out[3k + 0] = 4 * sum_e w[e] Re(conj(h_k[e]) r[e])
 *   out[3k + 1] = 4 * sum_e w[e] Im(conj(h_k[e]) r[e])
 *   out[3k + 2] = 4 * sum_e w[e] |h_k[e]|^2          k = 0 .. nrow - 1
 *   out[3 nrow] = 4 * sum_e w[e] |r[e]|^2
 * h: nrow complex rows of nelem elements (efd_fisher_gram's conventions: row r at
 * h + 2 r row_stride doubles, row_stride >= nelem, 16-byte aligned; a slice of a wider buffer is
 * fine), 1 <= nrow <= EFD_OVERLAP_MAX_ROWS; t, u: contiguous complex [nelem]; w: real [nelem] or
 * NULL (w = 1); out: 3 nrow + 1 device doubles; scratch: EFD_OVERLAP_SCRATCH device doubles.
 * Every element of h is read once; t, u, w once per block of 8 rows. Terms, as written (no
 * contraction): fma(w, fma(hr, rr, hi ri), .), fma(w, fma(hr, ri, -(hi rr)), .),
 * fma(w, fma(hr, hr, hi hi), .). Promises:
 *   - no atomics, a fixed partition that depends on nelem only and fixed reduction orders:
 *     bitwise reproducible;
 *   - out[3k .. 3k + 2] is a function of row k, t, u, w and nelem alone: the same row gives the
 *     same bits alone, at another position, in another row block or beside other rows (so a
 *     caller may split more rows than EFD_OVERLAP_MAX_ROWS over several calls without changing
 *     any number);
 *   - the cross terms out[3k], out[3k + 1] are exactly 0 when u equals t bit for bit, and when
 *     row k's support is disjoint from r's.
 * EFD_ERR_ARG before any launch: nrow out of range, NULL h, t, out or scratch, nelem <= 0,
 * row_stride < nelem.
 */
#define EFD_OVERLAP_MAX_ROWS 64
#define EFD_OVERLAP_SCRATCH 197632
int efd_overlap_rows(const double* h, int64_t row_stride, int32_t nrow, const double* t,
                     const double* u, const double* w, int64_t nelem, double* out,
                     double* scratch, void* stream);

/*
 * Statistics of many (template a, template b) pairs in one pass over each operand: everything
 * the reference's mode-by-mode driver derives per (source, window) from six to eight
 * inner_product calls (check_mode_by_mode.py:292 SNR, :299-301 normalised overlap, :315-317 the
 * log-likelihood of the difference). For row pair r and channel c, out[(r nchan + c) 5 + i]:
 *   0: aa  = 4 sum_k w |a|^2
 *   1: bb  = 4 sum_k w |b|^2
 *   2: abr = 4 sum_k w Re(conj(a) b)
 *   3: abi = 4 sum_k w Im(conj(a) b)
 *   4: dd  = 4 sum_k w |a - b|^2        (a - b formed per element, then squared: a pair at
 *                                        mismatch 1e-6 does not get dd from aa + bb - 2 abr)
 * a_r, b_r: complex [nchan][nbin] at a + 2 r a_stride and b + 2 r b_stride doubles (strides >=
 * nchan nbin, rows 16-byte aligned; slices of wider buffers are fine), 1 <= nrow <=
 * EFD_PAIR_MAX_ROWS, nchan 1 or 2; w: real [nbin] shared by the channels and rows, or NULL
 * (w = 1): diff(f) / PSD with the first spacing repeated (lisatools diagnostic.py:93-98); out:
 * 5 nchan nrow device doubles; scratch: EFD_PAIR_SCRATCH device doubles. Every element of a and
 * b is read once; w once per row (from the XCD's cache after the first: the row is the slow
 * grid dimension). Terms, as written (no contraction), with dr = ar - br, di = ai - bi:
 *   fma(w, fma(ar, ar, ai ai), .), fma(w, fma(br, br, bi bi), .), fma(w, fma(ar, br, ai bi), .),
 *   fma(w, ar bi - ai br, .)   (two rounded products and their difference, no inner fma),
 *   fma(w, fma(dr, dr, di di), .).
 * efd_td_split_pair_stats: the same ten numbers per row (nchan = 2) with b_r never stored: b_r
 * is what efd_td_split writes for row r of Z (the same arithmetic, gain, and keep rule: a bin
 * with keep[k] == 0 has b = 0 and its Z is not read; a is taken as given), a_r complex [2][nb] at
 * a + 2 r a_stride doubles (a_stride >= 2 nb), w real [nb] or NULL, nb = (n + 1) / 2. Bin 0 pairs
 * with itself; for even n the Nyquist bin is in neither channel. Every element of Z and a is
 * read once.
 * Promises of both:
 *   - no atomics, a partition that depends on nbin (n) only and fixed reduction orders: bitwise
 *     reproducible;
 *   - a row's numbers are a function of that row pair, w (keep, gain) and the sizes alone: the
 *     same alone, at another position or beside other rows (so more than EFD_PAIR_MAX_ROWS
 *     pairs go in several calls without changing any number);
 *   - efd_pair_stats: dd and abi are exactly 0 and aa == bb == abr when b equals a bit for bit;
 *   - a NaN in a row makes only that row's outputs NaN. efd_td_split_pair_stats, even n: a NaN
 *     in the Nyquist bin of a row of Z makes that row's bb, abr, abi and dd NaN
 *     (efd_td_split_loglike's rule).
 * EFD_ERR_ARG before any launch: NULL a, b, Z, out or scratch, rows outside
 * 1..EFD_PAIR_MAX_ROWS, nbin <= 0, n < 1, a stride too small, nchan not 1 or 2.
 */
#define EFD_PAIR_MAX_ROWS 64
#define EFD_PAIR_SCRATCH 655360
int efd_pair_stats(const double* a, int64_t a_stride, const double* b, int64_t b_stride,
                   int32_t nrow, int32_t nchan, int64_t nbin, const double* w, double* out,
                   double* scratch, void* stream);
int efd_td_split_pair_stats(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                            const double* a, int64_t a_stride, const double* w,
                            const uint8_t* keep, double* out, double* scratch, void* stream);

/*
 * efd_modesum_sum_dh_hh's three numbers for templates that were written: row r, complex
 * [nchan][nbin] at h + 2 r row_stride doubles (row_stride >= nchan nbin), against one d complex
 * [nchan][nbin] and one w real [nchan][nbin]; out[3 r ..] = (Re <d|h>, Im <d|h>, <h|h>), the same
 * three terms per bin and channel. 1 <= nrow <= EFD_DH_MAX_ROWS, nchan 1 or 2; scratch:
 * EFD_DH_SCRATCH device doubles. Every element of h is read once; d and w once per row (from the
 * XCD's cache after the first). efd_pair_stats' promises: no atomics, a partition that depends on
 * nbin only, fixed orders (bitwise reproducible); a row's numbers are the same alone or beside
 * other rows; with d == h w bit for bit Re <d|h> == <h|h> and Im <d|h> == 0.0. EFD_ERR_ARG before
 * any launch: NULL h, d, w, out or scratch, nrow or nchan out of range, nbin <= 0, row_stride too
 * small.
 */
#define EFD_DH_MAX_ROWS 64
#define EFD_DH_SCRATCH 196608
int efd_dh_hh_rows(const double* h, int64_t row_stride, int32_t nrow, const double* d,
                   const double* w, int32_t nchan, int64_t nbin, double* out, double* scratch,
                   void* stream);

/*
 * Every windowing of one series from one read of it: out[j][k] = win[j][k] h[k] (real times
 * complex, each part one product), h complex [n], win: HOST array of nwin device pointers to
 * real windows [n], 1 <= nwin <= EFD_WINDOW_MAX_ROWS; a NULL entry copies the series bit for bit
 * (the unwindowed row); row j at out + 2 j out_stride doubles, out_stride >= n. One TD mode sum
 * then serves every window of a source (the driver windows and transforms the same series four
 * times, check_mode_by_mode.py:263-264, :271-272). EFD_ERR_ARG before any launch: NULL h, win
 * or out, n < 1, nwin out of range, out_stride < n.
 */
#define EFD_WINDOW_MAX_ROWS 16
int efd_window_rows(const double* h, int64_t n, const double* const* win, int32_t nwin,
                    double* out, int64_t out_stride, void* stream);

/*
 * CPU twins: the same algorithm on HOST pointers, C++17 + OpenMP
 * (csrc/emrifd_cpu.cpp: the mode sum's and the spline build's; csrc/emrifd_reduce_cpu.cpp: the
 * reductions', splits' and window rows'; both linked into libemrifd.so). Signatures are those of the HIP entry points;
 * `stream`, `workspace` and `scratch` are accepted for parity and ignored (pass NULL / 0). The
 * reference's CPU path is the numpy branch of the same FEW generator (check_mode_by_mode.py:50-60,
 * emri_pe.py:68-80); these twins are the CPU baseline bench.py times at 1 thread and all cores.
 * efd_modesum_cpu: the same grouping, splines, interval records and tile-wise output-stationary
 * sum with the uniform K_{1/3} fast path as efd_modesum, exact IEEE divisions / square roots;
 * synchronous. Errors (EFD_ERR_ARG) are reported by return code + efd_cpu_last_error.
 */
int efd_modesum_cpu(const efd_modesum_args* a, void* workspace, size_t workspace_bytes,
                    void* stream);
/* Counters of the calling thread's last efd_modesum_cpu (as efd_modesum_stats). */
int efd_modesum_cpu_stats(int64_t* contributions, int64_t* evaluations, int32_t* groups);
int efd_spline_build_cpu(const double* x, int n, const double* y, int ninterp, double* coef,
                         void* stream);
int efd_polarizations_cpu(const double* S, int64_t nf, int64_t k0, double* hp, double* hc,
                          void* stream);
int efd_loglike_cpu(const double* h, const double* d, const double* w, int32_t nchan,
                    int64_t nbin, double* out, double* scratch, void* stream);
int efd_inner_product_cpu(const double* a, const double* b, const double* w, int32_t nchan,
                          int64_t nbin, double* out, double* scratch, void* stream);
int efd_fisher_gram_cpu(const double* h, int64_t row_stride, int32_t nparam, int32_t npoint,
                        const double* coef, const double* w, int64_t nelem, double* dh,
                        double* gram, double* scratch, void* stream);
int efd_overlap_rows_cpu(const double* h, int64_t row_stride, int32_t nrow, const double* t,
                         const double* u, const double* w, int64_t nelem, double* out,
                         double* scratch, void* stream);
int efd_td_split_cpu(const double* Z, int64_t stride, int64_t n, int32_t rows, double gain,
                     const uint8_t* keep, double* out, int64_t out_stride, void* stream);
int efd_td_split_loglike_cpu(const double* Z, int64_t stride, int64_t n, int32_t rows,
                             double gain, const double* d, const double* w, double* out,
                             double* scratch, void* stream);
int efd_pair_stats_cpu(const double* a, int64_t a_stride, const double* b, int64_t b_stride,
                       int32_t nrow, int32_t nchan, int64_t nbin, const double* w, double* out,
                       double* scratch, void* stream);
int efd_td_split_pair_stats_cpu(const double* Z, int64_t stride, int64_t n, int32_t rows,
                                double gain, const double* a, int64_t a_stride, const double* w,
                                const uint8_t* keep, double* out, double* scratch, void* stream);
int efd_dh_hh_rows_cpu(const double* h, int64_t row_stride, int32_t nrow, const double* d,
                       const double* w, int32_t nchan, int64_t nbin, double* out,
                       double* scratch, void* stream);
int efd_window_rows_cpu(const double* h, int64_t n, const double* const* win, int32_t nwin,
                        double* out, int64_t out_stride, void* stream);
/* OpenMP threads of the twins (n <= 0: all available); returns the previous setting. */
int efd_cpu_threads(int n);
/* Last error message of the calling thread's CPU-twin call. */
int efd_cpu_last_error(char* buf, int len);

/*
 * Host upstream of the hot path (csrc/emrifd_host.cpp): STAND-IN PHYSICS, NOT FEW (FEW's flux
 * and amplitude data are absent offline). The C++ form of the package's Python stand-ins, with
 * the same equations and integrator (scipy RK45's Dormand-Prince 5(4), step control, dense
 * output and terminal separatrix event). Host pointers, synchronous, thread-safe.
 *
 * efd_host_trajectory <- EMRIInspiral(func="SchwarzEccFlux")(M, mu, 0, p0, e0, 1, T=T)
 *   (check_mode_by_mode.py:34-35): Peters-Mathews fluxes, exact Schwarzschild frequencies; knots
 *   t [s], p, e, Phi_phi, Phi_r and (optional, NULL to skip) f_phi, f_r = Omega / (2 pi M
 *   MTSUN_SI) [Hz], at most max_len (EFD_ERR_WORKSPACE beyond); *nt = knot count.
 * efd_host_p_at_t <- few.utils.utility.get_p_at_t (check_mode_by_mode.py:200-212): p0 whose
 *   inspiral plunges after t_out years (Brent; bracket [lo, hi], <= 0 for the defaults).
 * efd_host_modes <- RomanAmplitude + ModeSelector(eps) (notebook :125-127): the synthetic
 *   amplitude model over the given mode list (l, m, n, seeded phase0 and jitter), selection of
 *   the modes holding (1 - eps) of |A Y|^2 at every knot (+m and -m partner branches, union over
 *   knots) into keep[*nkeep]; with teuk != NULL also their complex amplitudes [nt][*nkeep]
 *   (EFD_ERR_WORKSPACE when 2 nt nkeep > teuk_cap doubles).
 */
int efd_host_trajectory(double M, double mu, double p0, double e0, double Phi_phi0, double Phi_r0,
                        double T, double rtol, double atol, int32_t max_len, double* t, double* p,
                        double* e, double* phi_phi, double* phi_r, double* f_phi, double* f_r,
                        int32_t* nt);
int efd_host_p_at_t(double M, double mu, double e0, double t_out, double rtol, double atol,
                    double xtol, double rtol_root, double lo, double hi, double* p0);
int efd_host_modes(const double* p, const double* e, int32_t nt, const int32_t* l,
                   const int32_t* m, const int32_t* n, const double* phase0, const double* jitter,
                   int32_t nmodes, const double* ylm_p, const double* ylm_m, double eps,
                   int32_t* keep, int32_t* nkeep, double* teuk, int64_t teuk_cap);
/* Threads the calling thread's later efd_host_modes calls spread their knots over (default 1;
 * the setting is per calling thread). Any count gives bitwise the same results. */
int efd_host_set_threads(int32_t n);

/*
 * Host staging of a walker batch for efd_modesum_prepare_batch (not part of the reference's
 * interface; the batched Likelihood's packing step, likelihood.py:246-274 callers): the ten
 * input arrays of walker i (src[10 i + f]: t, phi_phi, phi_r, f_phi, f_r, amp [nt][K] complex,
 * m, n, ylm_p, ylm_m; nt = shape[2 i], K = shape[2 i + 1]) are copied 256-B aligned into the
 * host buffer pin, and args[i] becomes *tmpl with walker i's nt, K, scale (scale[2 i] + i
 * scale[2 i + 1]) and device pointers dev_base + offset (valid after pin is copied to
 * dev_base). *total = bytes needed; EFD_ERR_WORKSPACE (nothing copied) when pin_bytes is less.
 */
int efd_stage_batch(void* pin, size_t pin_bytes, uint64_t dev_base, int32_t count,
                    const uint64_t* src, const int32_t* shape, const double* scale,
                    const efd_modesum_args* tmpl, efd_modesum_args* args, size_t* total);

/*
 * One walker group of the fused likelihood in one call: efd_stage_batch(pin, pin_bytes, dbuf,
 * count, src, shape, scale, tmpl, args, total), the host-to-device copy of pin to dbuf on
 * `stream`, staged_event (a hipEvent_t, or NULL) recorded after it, then
 * efd_modesum_prepare_batch and efd_modesum_sum_loglike_ex(args, workspace, workspace_bytes,
 * d, w, tile_const, out) in launches of EFD_BATCH_MAX walkers on `stream`. EFD_ERR_WORKSPACE
 * with *total set and nothing queued when pin or dbuf is shorter than *total. Not part of the
 * reference's interface: Likelihood.get_ll's per-group host steps (likelihood.py:246-274
 * callers) in one native call.
 */
int efd_fused_group(void* pin, size_t pin_bytes, void* dbuf, size_t dbuf_bytes, int32_t count,
                    const uint64_t* src, const int32_t* shape, const double* scale,
                    const efd_modesum_args* tmpl, efd_modesum_args* args,
                    void* const* workspace, const size_t* workspace_bytes, const double* d,
                    const double* w, const double* tile_const, double* out, void* staged_event,
                    void* stream, size_t* total);

/*
 * Amplitudes and ModeSelector(eps) on the device for batched callers (not part of the
 * reference's interface; csrc/emrifd_modes_device.inc). efd_host_modes' work for `count` walkers
 * (1 <= count <= EFD_BATCH_MAX) in three launches on `stream`: asynchronous, allocation-free, no
 * host synchronisation, no atomics; bitwise reproducible, and each walker's outputs are bitwise
 * those of its own call with count = 1.
 *
 * At every knot the branch powers |A_k|^2 |Y_k|^2 (every mode) and |A_k|^2 |Y_{l,-m}|^2 (modes
 * with m != 0) are sorted descending (ties: the +m branches before the partners, then by mode
 * index); a branch is kept while the sum of those before it is < (1 - eps) total, the largest
 * always; partner picks fold onto their +m mode; the kept set is the union over the knots.
 *
 * The mode table is shared by the walkers (device): 1 <= nmodes <= 4096.
 */
typedef struct efd_modes_table {
    const int32_t* l;         /* [nmodes]                                                     */
    const int32_t* m;         /* [nmodes] m != 0 adds the partner branch                      */
    const int32_t* n;         /* [nmodes]                                                     */
    const double* phase0;     /* [nmodes] the stand-in model's seeded phases                  */
    const double* jitter;     /* [nmodes] and log10-magnitude jitter                          */
    int32_t nmodes;
} efd_modes_table;

/* One walker of efd_modes_select_batch; every pointer is device memory. */
typedef struct efd_modes_walker {
    const double* p;          /* [nt] trajectory knots (1 <= nt <= 1024)                      */
    const double* e;          /* [nt]                                                         */
    int32_t nt;
    const double* ylm_p;      /* complex [nmodes]: Y_lm (walkers may share the pointer)       */
    const double* ylm_m;      /* complex [nmodes]: (-1)^l Y_{l,-m}                            */
    double eps;               /* 0 <= eps <= 1                                                */
    int32_t include_minus_m;  /* 0: ylm_m_out is written as zeros                             */
    const double* teuk;       /* optional complex [nt][nmodes]: the amplitudes to select on
                               * and to gather; NULL = the stand-in model of efd_host_modes,
                               * evaluated in the kernels (STAND-IN PHYSICS, NOT FEW)          */
    /* outputs, in the mode sum's input layout (efd_modesum_args: amp, m, n, ylm_p, ylm_m) */
    int32_t* keep;            /* [nmodes] capacity: kept mode indices, ascending              */
    int32_t* nkeep;           /* [1] K                                                        */
    int32_t* status;          /* [1] 0, or EFD_MODES_AMP_OVERFLOW                             */
    double* amp;              /* complex [nt][K], or NULL: no amplitudes wanted               */
    int64_t amp_cap;          /* complex elements amp holds; nt K > amp_cap sets
                               * EFD_MODES_AMP_OVERFLOW in status (nkeep is still written,
                               * nothing is stored past the capacity, amp's content is void)   */
    int32_t* m_out;           /* [nmodes] capacity: m of the kept modes                       */
    int32_t* n_out;           /* [nmodes] capacity                                            */
    double* ylm_p_out;        /* complex [nmodes] capacity                                    */
    double* ylm_m_out;        /* complex [nmodes] capacity                                    */
    void* workspace;          /* efd_modes_workspace_bytes(nt, nmodes), 4-byte aligned, the
                               * walker's own; needs no initialisation                         */
    size_t workspace_bytes;
} efd_modes_walker;

#define EFD_MODES_AMP_OVERFLOW 1

/* Bytes of workspace one walker of efd_modes_select_batch needs; 0 for an invalid shape
 * (nt < 1 or nt > 1024, nmodes < 1 or nmodes > 4096). Host-only query. */
size_t efd_modes_workspace_bytes(int32_t nt, int32_t nmodes);
int efd_modes_select_batch(const efd_modes_table* tab, const efd_modes_walker* w, int32_t count,
                           void* stream);

/*
 * Noise-weighted mode selection (not part of the reference's interface; FEW's ModeSelector with a
 * sensitivity_fn, as recalled): before the cut both branch powers of mode k at knot i are
 * multiplied by W[i][k] = 1 / S(F), F = |m_k f_phi[i] + n_k f_r[i]| (the partner's frequency is
 * -F: the same weight), where S(F) is finite and > 0, and by 0 elsewhere. eps is then a fraction
 * of the noise-weighted power. A knot whose weighted total is 0 or not finite keeps nothing (the
 * unweighted selection always keeps a knot's largest branch; here that would be a tie-break among
 * zeros), so the kept set can be empty.
 *
 * The PSD is a piecewise cubic in scipy's PPoly layout: x[n] strictly ascending breakpoints,
 * c[4][n - 1] row-major (c[j (n - 1) + i] the coefficient of s^(3 - j) on piece i),
 *   S(f) = ((c0 s + c1) s + c2) s + c3,  s = f - x[i],
 *   i = clamp(#{j : x[j] <= f} - 1, 0, n - 2)   (searchsorted(x, f, 'right') - 1),
 * so the end pieces extrapolate as PPoly(extrapolate=True) does, and NaN gives NaN. Every
 * product and sum is rounded on its own (no fused multiply-add): efd_psd_eval and
 * efd_psd_eval_cpu return the same bits.
 */
typedef struct efd_psd_table {
    const double* x;          /* [n] breakpoints, strictly ascending                          */
    const double* c;          /* [4][n - 1] coefficients, highest power first                 */
    int32_t n;                /* 2 <= n <= 4096                                               */
} efd_psd_table;

/* out[j] = S(f[j]), j < nf. efd_psd_eval: x, c, f and out are device memory, one launch on
 * `stream`, asynchronous (x's order is the caller's to guarantee). efd_psd_eval_cpu: host memory,
 * synchronous, `stream` ignored; x not strictly ascending is EFD_ERR_ARG. nf = 0 does nothing. */
int efd_psd_eval(const efd_psd_table* psd, const double* f, int64_t nf, double* out, void* stream);
int efd_psd_eval_cpu(const efd_psd_table* psd, const double* f, int64_t nf, double* out,
                     void* stream);

/* efd_host_modes with the noise weighting above: f_phi, f_r [nt] (Hz, efd_host_trajectory's) and
 * a host efd_psd_table. Any efd_host_set_threads count gives the same results; *nkeep may be 0. */
int efd_host_modes_weighted(const double* p, const double* e, int32_t nt, const int32_t* l,
                            const int32_t* m, const int32_t* n, const double* phase0,
                            const double* jitter, int32_t nmodes, const double* ylm_p,
                            const double* ylm_m, double eps, const double* f_phi,
                            const double* f_r, const efd_psd_table* psd, int32_t* keep,
                            int32_t* nkeep, double* teuk, int64_t teuk_cap);

/* One walker's knot frequencies for efd_modes_select_batch_weighted: [nt] each, device memory;
 * both NULL = this walker is selected unweighted (exactly as by efd_modes_select_batch). */
typedef struct efd_modes_weight {
    const double* f_phi;
    const double* f_r;
} efd_modes_weight;

/* efd_modes_select_batch with the noise weighting above formed inside the selection kernel (one
 * interval search and one cubic per (knot, mode), serving both branches): still three launches,
 * no allocation, no host synchronisation, no atomics, bitwise reproducible, each walker's outputs
 * bitwise those of its own count = 1 call. wt[count]; psd holds device pointers. wt = NULL (then
 * psd may be NULL), or every walker's frequencies NULL, is efd_modes_select_batch. With teuk
 * given, the table's m and n must be the modes' (the unweighted call reads m != 0 only). */
int efd_modes_select_batch_weighted(const efd_modes_table* tab, const efd_modes_walker* w,
                                    const efd_modes_weight* wt, const efd_psd_table* psd,
                                    int32_t count, void* stream);

/*
 * Inspiral trajectories and the p0 solve on the device for batched callers (not part of the
 * reference's interface; csrc/emrifd_traj.hip). STAND-IN PHYSICS, NOT FEW: efd_host_trajectory's
 * and efd_host_p_at_t's equations and integrator (scipy RK45's Dormand-Prince 5(4), step control,
 * dense output, terminal separatrix event, Brent's roots), one wavefront per source: lane i
 * evaluates node i of the 64-node frequency quadrature. Both calls are asynchronous on `stream`,
 * allocation-free, without host synchronisation or atomics; they accept any count >= 1, and
 * each source's outputs are bitwise those of its own count = 1 call. The host forms are the
 * reference, followed operation for operation (no fused multiply-add, the quadrature summed in
 * the host's order, correctly rounded powers): the knots are the host's bit for bit until one of
 * the host's pow calls is not correctly rounded (0.08 % of them), and within rounding after.
 *
 * efd_traj_batch: source i's knots into knots[i][7][max_len] (t [s], p, e, Phi_phi, Phi_r, f_phi,
 *   f_r [Hz], efd_host_trajectory's seven arrays), nt[i] knots, 2 <= max_len <=
 *   EFD_TRAJ_MAX_LEN. status[i] is written for every source; nt[i] only with EFD_TRAJ_OK. A source
 *   with another status stores nothing past its max_len knots and leaves the others untouched.
 * efd_traj_p_at_t_batch: p0[i] whose inspiral plunges after src[i].T = t_out years
 *   (efd_host_p_at_t with its default bracket; src[i].p0 is ignored), NaN unless status[i] is
 *   EFD_TRAJ_OK.
 * EFD_ERR_ARG before any launch: NULL pointers, count < 1, max_len out of range.
 *
 * Every device loop is bounded: an integration by 4 EFD_TRAJ_MAX_LEN accepted plus rejected steps,
 * a root by 100 iterations, the bracket by 7 expansions.
 */
typedef struct efd_traj_source {
    double M, mu, p0, e0, Phi_phi0, Phi_r0, T, rtol, atol;
} efd_traj_source;

#define EFD_TRAJ_MAX_LEN 1024
#define EFD_TRAJ_OK 0
#define EFD_TRAJ_BAD_SOURCE 1   /* not finite, M, mu, T, rtol or atol <= 0, p0 inside the buffer */
#define EFD_TRAJ_TOO_LONG 2     /* more than max_len knots                                       */
#define EFD_TRAJ_STEP_FAILED 3  /* step size below the representable minimum (the host's -2)     */
#define EFD_TRAJ_STEP_CAP 4     /* more than 4 EFD_TRAJ_MAX_LEN steps in one integration         */
#define EFD_TRAJ_NO_BRACKET 5   /* p0 solve: t_out shorter than the plunge from the buffer, or
                                 * no upper bracket end below 500                                */

int efd_traj_batch(const efd_traj_source* src /* device [count] */, int32_t count,
                   int32_t max_len, double* knots /* device [count][7][max_len] */,
                   int32_t* nt /* device [count] */, int32_t* status /* device [count] */,
                   void* stream);
int efd_traj_p_at_t_batch(const efd_traj_source* src /* p0 ignored, T = t_out in years */,
                          int32_t count, double xtol, double rtol_root,
                          double* p0 /* device [count] */, int32_t* status, void* stream);

/*
 * Noise realisations (not part of the reference's interface, which stubbed them:
 * lisatools/sampling/likelihood.py:183-199, utils/utility.py:5-13; csrc/emrifd_noise.hip and the
 * shared arithmetic csrc/emrifd_noise.h). One unit complex normal xi(c, k) per (seed,
 * realisation, channel c, bin k), a function of those four alone:
 *   Philox4x32-10 (Salmon et al. 2011) with counter (k & 0xffffffff, k >> 32, c, realisation)
 *   and key (seed & 0xffffffff, seed >> 32) gives the words w0..w3;
 *   a = (w0 << 21) | (w1 >> 11), b = (w2 << 21) | (w3 >> 11); u1 = (a + 1) 2^-53, u2 = b 2^-53;
 *   xi = sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2), so E |xi|^2 = 2.
 * lisatools' noise on a bin of spacing df and PSD S is sqrt(S) (0.5 / sqrt(df)) xi; in the
 * likelihood's weighted space (x sqrt(df / S)) that is 0.5 xi on every bin.
 *
 * efd_noise_fd: out[c][i] = gain[c][i] * 0.5 * xi(c, bin0 + i) for c < nchan, i < nbin (with
 *   accumulate != 0 added to out instead). out complex [nchan][nbin]; gain [nchan][nbin] or NULL
 *   (= 1). A gain of 0 or NaN gives exactly 0 (leaves out untouched under accumulate); the bin
 *   still counts, so slices of a grid (bin0) are bitwise the whole grid's. nbin = 0 does nothing
 *   and returns 0. One launch, asynchronous, no scratch.
 *
 * efd_noise_overlap_rows: out[r - real0][p] = sum_c sum_k gain[c][k] Re(conj xi_r(c, k)
 *   rows[p][c][k]) for the draws r in [real0, real0 + ndraw) and the rows p < nrow; the noise is
 *   regenerated in registers and never written. rows complex [nrow][nchan][nbin] contiguous; gain
 *   [nchan][nbin] or NULL (= 1), a gain of 0 or NaN contributes nothing; out [ndraw][nrow];
 *   scratch EFD_NOISE_SCRATCH doubles. With gain = sqrt(4 df / S) this is <n_r | rows_p> of the
 *   noise n_r = sqrt(S) (0.5 / sqrt(df)) xi_r, whose covariance over r is the rows' Fisher (Gram)
 *   matrix. Limits: 1 <= nrow <= EFD_NOISE_MAX_ROWS, 1 <= nbin <= 2^40, real0 + ndraw <= 2^32
 *   (EFD_ERR_ARG beyond); any ndraw: the call runs EFD_NOISE_DRAWS_PER_LAUNCH draws per launch.
 *   Fixed-partition two-pass reduction without atomics: an entry depends on (seed, r, row p,
 *   gain, nchan, nbin) only, not on the other rows, the other draws or how ndraw is split over
 *   calls. ndraw = 0 does nothing.
 *
 * The _cpu twins take host pointers (scratch and stream unused) and share the integer stage and
 * the order of the floating-point steps; efd_noise_philox_cpu returns the four words of one
 * Philox4x32-10 call (counter[4], key[2]) for known-answer tests.
 */
#define EFD_NOISE_MAX_ROWS 16
#define EFD_NOISE_DRAWS_PER_LAUNCH 256
#define EFD_NOISE_SCRATCH 1048576   /* 256 workgroups x 256 draws x 16 rows */

int efd_noise_fd(double* out, const double* gain, int32_t nchan, int64_t nbin, uint64_t bin0,
                 uint64_t seed, uint32_t realisation, int32_t accumulate, void* stream);
int efd_noise_overlap_rows(const double* rows, int32_t nrow, const double* gain, int32_t nchan,
                           int64_t nbin, uint64_t seed, uint32_t real0, int64_t ndraw, double* out,
                           double* scratch, void* stream);
int efd_noise_fd_cpu(double* out, const double* gain, int32_t nchan, int64_t nbin, uint64_t bin0,
                     uint64_t seed, uint32_t realisation, int32_t accumulate, void* stream);
int efd_noise_overlap_rows_cpu(const double* rows, int32_t nrow, const double* gain,
                               int32_t nchan, int64_t nbin, uint64_t seed, uint32_t real0,
                               int64_t ndraw, double* out, double* scratch, void* stream);
int efd_noise_philox_cpu(const uint32_t* counter, const uint32_t* key, uint32_t* words);

#ifdef __cplusplus
}
#endif

#endif /* EMRIFD_H */
