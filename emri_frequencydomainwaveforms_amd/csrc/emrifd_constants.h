// emrifd_constants.h -- the constants the device code (emrifd_layout.h, for emrifd.hip and
// emrifd_prepare.hip) and the host twin (emrifd_cpu.cpp) must agree on, defined once. Plain
// C++17, no HIP, no includes; like spa_tables.inc and env_fit.inc it is included inside the
// includer's own namespace (the units' anonymous one, the twin's efdcpu).
#pragma once

constexpr int TILE = 256;           // threads per workgroup in k_modesum (round 2: 512-thread
                                    // tiles of 8 waves ran 0.974x)
// bins (lanes) per thread in k_modesum. Round 4: 3 with the own/mirror amplitude cubics split
// fits the 128-VGPR budget without spills in the record loop: config 2 +2.1-2.4% over 2
// (paired A/B, 3 rounds on two boxes, profiles/r04_ab_bpl3.jsonl); 4 spilled (-4%)
#ifndef EFD_BPL
#define EFD_BPL 3   // (an experiment switch: -DEFD_BPL=4)
#endif
constexpr int BPL = EFD_BPL;
constexpr int MAXRUNS = 8;          // monotonic runs per harmonic
constexpr int MAX_NT = 1024;        // knots (FEW max_init_len is 1000); bounds LDS staging
constexpr int MAX_K = 8192;         // harmonics per call
constexpr double PI = 3.141592653589793238462643383279502884;
constexpr double TWO_PI = 6.283185307179586476925286766559005768;
// The records' F'' coefficients carry sqrt(3/(2 pi)) |KRH_1|^(1/4), so the fast path's square
// is v = sqrt|KRH_1| / |y| instead of 1/|y|: rho's leading correction 1 + KRH_1 / y^2 becomes
// 1 - v^2, one FMA (the K_{1/3} series constants of spa_tables.inc are rescaled to v)
constexpr double VS = 0.18633899812498247470;             // sqrt|KRH_1|
constexpr double FDD_SCALE = 0.29827892638794838654;      // sqrt(3/(2 pi)) |KRH_1|^(1/4)
constexpr double INV_FDD_SCALE = 3.3525667136785156343;

// Fast-path series length: FAST_J terms of each of R and I/w, exact (truncation < 1e-17) for
// |y| >= FAST_Y (J = 3 -> 555, 4 -> 153, 5 -> 75, 6 -> 48); lanes below FAST_Y take the general
// path, whose K_{1/3} factor comes from the piecewise-polynomial table of kfactor_table.inc.
constexpr int FAST_J = 4;
constexpr double FAST_Y = 153.0;
// the K_{1/3} factor's polar phase, leading coefficient TH_0 (see KTHN at its use in spa_fast_m)
constexpr double KTH0 = -0.069444444444444444444;   // TH_0
// The sum's cosine on |r| <= pi/512 is COS_A + COS_B r^2 (sincos_tab in emrifd.hip, where the
// choice is explained); the general path's K_{1/3} table covers w in [KTAB_WMIN, KTAB_WMAX]
constexpr double COS_A = 1.000000000029531;
constexpr double COS_B = -0.5;
constexpr double KTAB_WMIN = 0x1p-8, KTAB_WMAX = 0x1p10;
