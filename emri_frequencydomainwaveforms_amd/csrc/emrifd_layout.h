// emrifd_layout.h -- what the two units of the mode-sum chain share: emrifd_prepare.hip (K0-K5)
// writes the workspace that emrifd.hip (K6-K9) reads. The constants, the record and header
// formats, the workspace layouts, the batch descriptor of the preparation kernels and the
// workgroup's exclusive scan (block_excl_scan), in an anonymous namespace: each unit compiles its
// own copy (no relocatable device code), and a table keeps a place only in the code object that
// reads it. Below them, the few host functions that cross between the two units.
#pragma once

#include "emrifd_common.h"

namespace {

#include "emrifd_constants.h"

constexpr int TILE_LANES = TILE * BPL;  // frequency bins (lanes) per tile
// k_segments_one: one 1024-thread workgroup per waveform when its 2 MAXRUNS K segment slots fit
constexpr int SEG1_NT = 1024;
constexpr int SEG1_MAX_K = SEG1_NT / (2 * MAXRUNS);
constexpr int KEYCAP = 2048;        // record keys per tile pass held in LDS
// Split tiles of the sparse fused likelihood (K <= SEG1_MAX_K: k_segments_one plans them). A
// tile whose estimated cost (wave-records: records x the 192-lane wave chunks each reaches)
// exceeds the waveform's fair share of the chip is evaluated by BPL workgroups, workgroup j
// taking bin j of every lane over the tile's whole record list (the sub-bin form of
// modesum_tile: each bin's sum in the whole tile's order, so the result is bitwise unsplit);
// the last of them (agent-scope release / acquire, counter per tile) runs the tile's epilogue
// from the bins they stored. A split across the record list instead (every S-th chunk, partial
// sums added by the last) reordered each bin's sum: the injection's logL became -6e-33, not 0.
// Items: the work units of the sparse launch, (tile, bin j, S, slot).
constexpr int SPLIT_ITEM_CAP = 8192;   // items per waveform (union tiles + extra splits)
constexpr int SPLIT_TILE_CAP = 128;    // split tiles per waveform (one slot and counter each)
constexpr int SPLIT_UNION_CAP = 4096;  // union tiles k_segments_one can cost (else no plan)
constexpr int SPLIT_MIN_COST = 48;     // wave-records: tiles below this are never split
constexpr int SPLIT_SLOTS_PER_WF = 64; // the fair share: a waveform's cost / this many workgroups

// Truncation after J terms is KB[J] w^(2J) < 1e-17 for |y| >= JSER_Y[J]; k_items picks the
// smallest J whose bound holds on the whole interval (a lower bound of |y| there).
#define EFD_TABLE __constant__
#include "spa_tables.inc"
// envelope records (k_items: A(w) polynomial, theta folded into the phase cubic); 1/sqrt from
// the hardware estimate and two Newton steps (~1 ulp; the fit's check needs 1e-11)
__device__ __forceinline__ double env_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    y = y * fma(-0.5 * x * y, y, 1.5);
    return y * fma(-0.5 * x * y, y, 1.5);
}
#define EFD_HD __device__
#include "env_fit.inc"
#undef EFD_HD

// ----------------------------------------------------------------------------------------
// Data layouts in HBM
// ----------------------------------------------------------------------------------------

// One record per ((m, n) group g, forward knot interval j): everything the SPA needs on the
// bins whose t(g) falls in [t_j, t_{j+1}). All harmonics (l, m, n) of one (m, n) share F, Phi,
// t(f), F', F'', sin/cos and the K_{1/3} factor; only A_lmn Y differs, and the not-a-knot spline
// is linear in its data, so the group carries the two combined amplitude splines
//   Bp(t) = sum_l y0_l A_l(t),  Bm(t) = sum_l y1_l A_l(t)   (y0 = -scale Y+, y1 = conj(-scale Y-))
// and one SPA evaluation serves every l. 288 B (18 pieces of 16 B), staged through LDS.
struct __attribute__((aligned(16))) Item {
    // Field order = the fast path's LDS reads: its first reads are 16-B pairs (ds_read_b128, 4
    // LDS cycles; a misaligned pair takes ds_read2_b64, 8): [gx, ic0] [ic1, ic2] [ic3, tj]
    // [ph0, ph1] [ph2, ph3] [fd0, fd1] [fd2, dtj]; dtj (uncertified records only) rides with fd2
    double gx;        // left end of the inverse-spline interval (ascending F)
    double ic[4];     // t(g) = ((ic0 u + ic1) u + ic2) u + ic3, u = g - gx
    double tj;        // forward interval [tj, tj + dtj)
    double ph[4];     // Phi_mn(t) = m Phi_phi + n Phi_r, w = t - tj (scipy PPoly order)
    double fd[3];     // F'(t)
    double dtj;
    double fdd[3];    // sqrt(3/(2 pi)) F''(t); F'' = derivative of the spline of F'(t_i) (:583)
    int32_t jser;     // K_{1/3} series terms the fast path needs on this interval (1..FAST_J)
    int32_t fdneg;    // F' < 0 at the interval's midpoint: the sign the fast path assumes for
                      // every lane (lanes of the other sign, at a turning point, take the general
                      // path). Also keeps b 16-B aligned, so its cubics come out of LDS by
                      // ds_read_b128 (8 ds_read2_b64 -> ds_read_b128 per record: k_modesum -3%)
    double b[2][2][4];  // b[0] = Bp (re, im cubics), b[1] = Bm: sub-branch s reads b[s] for its
                        // own bin and b[1-s] for the mirror
    int32_t klo[2], khi[2];  // lane ranges per sub-branch s (see k_items)
};
static_assert(sizeof(Item) == 288, "Item must be 288 B");
// Envelope records (k_items, env_fit.inc; Item::jser = 0): the fd, dtj, fdd slots hold the
// ENV_DEG + 1 coefficients of A(w) instead, highest power first, and ph holds Phi - theta. Only
// certified-safe records become envelope records, so nothing that reads fd / dtj / fdd (the
// masked body's tests, the general path) ever meets one.
static_assert(offsetof(Item, dtj) == offsetof(Item, fd) + 24 &&
              offsetof(Item, fdd) == offsetof(Item, fd) + 32 &&
              offsetof(Item, jser) == offsetof(Item, fd) + 8 * (ENV_DEG + 1),
              "envelope coefficients: fd, dtj, fdd contiguous");
// envelope records store A(w) times the sum's cosine constant (COS_A; static_assert in emrifd.hip)
constexpr double ENV_AMP_SCALE = 1.000000000029531;
__host__ __device__ __forceinline__ double* env_of(Item* it) {
    return reinterpret_cast<double*>(reinterpret_cast<char*>(it) + offsetof(Item, fd));
}
__host__ __device__ __forceinline__ const double* env_of(const Item* it) {
    return reinterpret_cast<const double*>(reinterpret_cast<const char*>(it) + offsetof(Item, fd));
}
static_assert(offsetof(Item, ph) % 16 == 0 && offsetof(Item, fd) % 16 == 0 &&
              offsetof(Item, fdd) % 16 == 0, "the fast path's coefficient pairs are 16-B aligned");
static_assert(offsetof(Item, b) % 16 == 0 && sizeof(Item::b) == 8 * 16, "b: 8 whole pieces");

// The error flags (runs_overflow, bad_mn, bad_tile) are sticky: k_group_b clears only the
// counters of a header it has initialised before (magic == HDR_MAGIC), so an error raised by any
// call on this workspace survives later preparations until efd_modesum_status reports and clears
// it (a pipeline slot reused by several walkers before its status is read loses none of them).
// A header without the magic (fresh device memory) is zeroed whole.
constexpr int64_t HDR_MAGIC = 0x45464448445233LL;   // "EFDHDR3"
struct Header {
    int64_t contributions;      // C of the last call: (l, m, n) branch x bin pairs (k_items)
    int64_t evaluations;        // SPA evaluations: (m, n) group branch x bin pairs
    int32_t runs_overflow;      // set by k_prep_b when a harmonic has > MAXRUNS monotonic runs
    int32_t groups;             // G: distinct (m, n) of the call (k_group_b)
    int32_t bad_mn;             // set by k_group_b when |m| > 255 or |n| > 1023
    int32_t bad_tile;           // set by k_modesum when a dispatch-order entry is out of range
    int64_t magic;              // HDR_MAGIC once k_group_b has initialised the header
    int32_t lane_lo, lane_hi;   // union [lo, hi) of the segments' lane ranges (k_segment_compact)
    int32_t nitems;             // sparse sum's work items (k_segments_one's split plan), -1: none
    int32_t nsplit;             // split tiles of the plan
    int64_t env_evaluations;    // evaluations on envelope records (k_items; 64 B)
};
static_assert(sizeof(Header) == 64, "Header must be 64 B");


struct Layout {
    size_t header, coefA, coefT, kslope, tscratch, invcp, invdp, runs, items, ranges, seglh,
        seginfo, nseg, slotlh, slotinfo, slotcnt, slottiles, segbase, stb0, stb1, gm, gn, gstart,
        gkeys,
        gmem, gamp, sctab, tkeys, tcnt, tperm, llpart, sitem, scnt, spart, total;
    int64_t stbcap;
    int64_t ntiles, nlanes;
};

__host__ __device__ inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// (also evaluated on the device by the batched preparation kernels: a few dozen scalar integer
// operations per workgroup, so the kernel arguments carry one workspace pointer per waveform)
// td: the TD sum's workspace instead, the FD layout's grouping and spline buffers only, in the
// same order (no records, no segment tables, no sin/cos table, no tile lists: those take no
// room there, and no stage of the TD preparation touches their offsets)
__host__ __device__ inline Layout make_layout(int32_t nt, int32_t K, int64_t nf, int paired,
                                              bool td = false) {
    Layout L{};
    const int64_t ni = nt - 1;
    L.nlanes = paired ? (nf + 1) / 2 : nf;
    L.ntiles = (L.nlanes + TILE_LANES - 1) / TILE_LANES;
    size_t off = 0;
    // all: a buffer of both workspaces; take: one of the FD workspace alone, no bytes under td
    // (the choice is made on the size, not on the offset: the offsets stay one chain of adds)
    auto all = [&](size_t bytes) { size_t o = off; off = align256(off + bytes); return o; };
    auto take = [&](size_t bytes) { return all(td ? 0 : bytes); };
    L.header = all(sizeof(Header));
    L.coefA = all(sizeof(double) * ni * 4 * 4 * K);   // [ni][4][4K]: Bp re/im, Bm re/im
    L.coefT = all(sizeof(double) * ni * 4 * 8);
    L.kslope = all(sizeof(double) * nt * 2);
    L.tscratch = all(sizeof(double) * nt * 16);
    L.invcp = take(sizeof(double) * nt * K);
    L.invdp = take(sizeof(double) * nt * K);
    L.runs = take(sizeof(int32_t) * 4 * MAXRUNS * K);
    L.items = take(sizeof(Item) * ni * K);
    L.ranges = take(sizeof(int4) * ni * K);
    L.seglh = take(sizeof(int2) * 2 * MAXRUNS * K);
    L.seginfo = take(sizeof(int4) * 2 * MAXRUNS * K);
    L.nseg = take(sizeof(int32_t));
    L.slotlh = take(sizeof(int2) * 2 * MAXRUNS * K);
    L.slotinfo = take(sizeof(int4) * 2 * MAXRUNS * K);
    L.slotcnt = take(sizeof(int32_t) * ((2 * MAXRUNS * K + 255) / 256));
    L.slottiles = take(sizeof(int32_t) * ((2 * MAXRUNS * K + 255) / 256));
    L.segbase = take(sizeof(int32_t) * 2 * MAXRUNS * K);
    // segment-tile boundaries (k_seg_tiles): one (p0, p1) pair per (segment, tile it covers);
    // segments past the capacity keep the bisection
    L.stbcap = 64 * L.ntiles + 4 * (int64_t)(2 * MAXRUNS * K);
    L.stb0 = take(sizeof(int32_t) * (size_t)L.stbcap);
    L.stb1 = take(sizeof(int32_t) * (size_t)L.stbcap);
    L.gm = all(sizeof(int32_t) * K);
    L.gn = all(sizeof(int32_t) * K);
    L.gstart = all(sizeof(int32_t) * (K + 1));
    L.gmem = all(sizeof(int32_t) * K);
    L.gkeys = all(sizeof(unsigned long long) * (size_t)MAX_K);   // k_group_b's general-case sort
    L.gamp = all(sizeof(double) * nt * 4 * K);
    L.sctab = take(sizeof(double) * 2 * 512);
    L.tkeys = take(sizeof(uint32_t) * (size_t)L.ntiles * KEYCAP);   // prebuilt tile lists
    L.tcnt = take(sizeof(int32_t) * (size_t)L.ntiles);
    L.tperm = take(sizeof(int32_t) * (size_t)L.ntiles);   // cost-ordered dispatch (k_tile_order)
    L.llpart = take(sizeof(double) * (size_t)L.ntiles);   // fused likelihood: per-tile partials
    // the sparse sum's split plan (k_segments_one, K <= SEG1_MAX_K only): items, one arrival
    // counter per split tile, the partial sums of the splits ([slot][lane][4] doubles)
    // (in both layouts: efd_modesum_workspace_bytes sizes by the unpaired one, which must stay
    // the larger)
    const bool plan = K <= SEG1_MAX_K;
    L.sitem = take(plan ? sizeof(int4) * SPLIT_ITEM_CAP : 0);
    L.scnt = take(plan ? sizeof(int32_t) * SPLIT_TILE_CAP : 0);
    L.spart = take(plan ? sizeof(double) * 4 * (size_t)SPLIT_TILE_CAP * TILE_LANES : 0);
    L.total = off;
    return L;
}

// Preparation of up to EFD_BATCH_MAX waveforms per launch (efd_modesum_prepare_batch; a single
// efd_modesum_prepare is a batch of one): blockIdx.z picks the waveform, the grids are sized for
// the batch's largest (nt, K), and each workgroup derives its waveform's workspace layout from
// (nt, K, nf, paired). Every waveform of a batch shares nf and the grid's symmetry.
struct PrepDesc {
    const double *t, *phi_phi, *phi_r, *f_phi, *f_r, *amp, *ylm_p, *ylm_m, *freq;
    const int32_t *m, *n;
    char* ws;
    double sc_re, sc_im;
    int32_t nt, K;
    int32_t lists;   // 1: prebuilt tile lists (k_tile_keys), 3: and cost-ordered dispatch
    int32_t pcr;     // bit 0: k_prep_pcr_b builds the trajectory and inverse splines, bit 1:
                     // and the amplitude splines (else k_prep_b's roles); set per waveform from
                     // its own (N_t, K), so a workspace never depends on its batch
    int32_t env;     // k_items makes envelope records (uniform caustic mode; EFD_ENV=0: none)
};
struct PrepBatch {
    PrepDesc d[EFD_BATCH_MAX];
    int64_t nf, nl, nl1;
    int32_t paired, n;
    int32_t pcr_groups;   // k_prep_pcr_b groups the harmonics itself (k_group_b not launched)
    int32_t seg_lds;      // k_segments_one's dynamic LDS bytes for the ranges table (0: none)
    int32_t split_min;    // k_segments_one: tiles costing at most this (wave-records) stay whole
    int32_t td;           // the TD sum's preparation: d[0].ws is a TD workspace (make_td_layout)
};
static_assert(sizeof(PrepBatch) <= 3072, "kernel arguments stay well inside 4 KB");

// the waveform of this workgroup: its descriptor and workspace layout
#define PREP_WALKER(B)                                                   \
    const PrepDesc& D = (B).d[blockIdx.z];                                \
    const Layout L = make_layout(D.nt, D.K, (B).nf, (B).paired);          \
    char* const W = D.ws
template <class T>
__device__ __forceinline__ T* ws_at(char* ws, size_t off) { return reinterpret_cast<T*>(ws + off); }

// Exclusive scan of one value per thread over a workgroup of NW waves, in thread order: a scan
// within each wave, the wave totals through wsum[NW] (LDS) and one barrier. Returns the sum of
// v over the threads before this one; total: over all of them. lane, wave: the caller's
// (threadIdx.x & 63, threadIdx.x >> 6). No barrier after the reads of wsum: a caller that
// writes wsum again adds its own.
template <int NW>
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int lane, int wave, int& total) {
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        before += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    return before + incl - v;
}

// Segment-tile boundaries: segment s covers tiles [t0, t1] (t0 = lo / TILE_LANES); its
// (p0, p1) pairs for those tiles sit at stb[toff(s) .. toff(s) + t1 - t0] in compacted segment
// order, and segbase[s] = toff(s) - t0 (so the pair of tile t is stb[segbase[s] + t]), or
// SEG_NO_STB when the pairs would pass the capacity (that segment keeps the bisection).
constexpr int32_t SEG_NO_STB = INT32_MIN;

// TD workspace: the FD layout's grouping and spline buffers only (no records, no tile lists)
using TdLayout = Layout;
inline TdLayout make_td_layout(int32_t nt, int32_t K) { return make_layout(nt, K, 0, 0, true); }

}  // namespace

// The host functions that cross between emrifd.hip and emrifd_prepare.hip (hidden, like fail).
// Their signatures name no type of the anonymous namespace above: such a function would have
// internal linkage itself.
namespace efdhip {
// argument checks of efd_modesum / _prepare / _sum and their batched forms (phase 1: prepare,
// 2: sum, needs an output; 0: the fused likelihood's sum, which writes none). In emrifd.hip.
EFD_INTERNAL int check_modesum_args(const efd_modesum_args* a, const void* workspace, int phase);
// PrepDesc::lists of a waveform of K harmonics on a grid of ntiles tiles: 0 the sum builds its
// tile lists itself, 1 prebuilt lists (k_tile_keys), 3 and the cost-ordered dispatch
// (k_tile_order). Preparation and sum ask the same question, so they agree. In emrifd.hip.
EFD_INTERNAL int32_t list_mode(int32_t K, int64_t ntiles);
// K6 at the end of the preparation chain (emrifd.hip): k_tile_keys over ntiles tiles when a
// waveform of the batch has lists, k_tile_order when one has lists == 3. prep_batch points at
// the chain's PrepBatch, whose type each unit compiles for itself.
EFD_INTERNAL int launch_tile_lists(const void* prep_batch, int64_t ntiles, bool any_lists,
                                   bool any_order, hipStream_t st);
// Preparation (K0-K6) of `count` waveforms in one chain of launches (emrifd_prepare.hip); fn
// names the caller in the error strings
EFD_INTERNAL int prepare_batch(const char* fn, const efd_modesum_args* const* a,
                               void* const* workspace, const size_t* workspace_bytes,
                               int32_t count, void* stream);
// The TD sum's preparation (emrifd_prepare.hip): header cleared, then a PrepBatch of one with
// td set through k_group_b, k_group_amp_b and k_prep_b's trajectory and amplitude roles, into
// the checked workspace (make_td_layout)
EFD_INTERNAL int td_prepare(const efd_td_args* a, void* workspace, hipStream_t st);
}  // namespace efdhip
