// emrifd_noise.h -- the arithmetic of the noise draws, shared by the HIP unit (emrifd_noise.hip)
// and its host twins (emrifd_reduce_cpu.cpp), so that the integer stage cannot drift between
// them: Philox4x32-10 (Salmon et al. 2011), two 53-bit uniforms from its four words, and the
// Box-Muller step to one unit complex normal xi. Plain C++: no intrinsics beyond the device's
// 32-bit high multiply, no inline assembly.
//
// One draw is a function of (seed, realisation, channel, bin) alone:
//   counter = (bin & 0xffffffff, bin >> 32, channel, realisation), key = (seed & 0xffffffff,
//   seed >> 32); words w0..w3 = Philox4x32-10(counter, key);
//   a = (w0 << 21) | (w1 >> 11), b = (w2 << 21) | (w3 >> 11)        (53 bits each)
//   u1 = (a + 1) 2^-53 in (0, 1],  u2 = b 2^-53 in [0, 1)
//   xi = sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2).
// The device takes sin and cos of pi (2 u2) with 2 u2 exact (sincospi); the host those of the
// float64 product 2 pi u2. Both are within the bound the tests hold the draws to (4e-14
// absolute of a long-double evaluation from the exact integers).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define EFD_NOISE_FN __host__ __device__ __forceinline__
#else
#define EFD_NOISE_FN inline
#endif

namespace efdnoise {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

EFD_NOISE_FN uint32_t mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Philox4x32-10: c (counter) is replaced by the four output words; the key is bumped after
// every round
EFD_NOISE_FN void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
        const uint32_t hi1 = mulhi32(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
}

// the draw's two 53-bit integers: u1 = (a + 1) 2^-53, u2 = b 2^-53
EFD_NOISE_FN void draw_bits(uint64_t seed, uint32_t realisation, uint32_t channel, uint64_t bin,
                            uint64_t& a, uint64_t& b) {
    uint32_t c[4] = {(uint32_t)(bin & 0xffffffffu), (uint32_t)(bin >> 32), channel, realisation};
    philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
    a = ((uint64_t)c[0] << 21) | (uint64_t)(c[1] >> 11);
    b = ((uint64_t)c[2] << 21) | (uint64_t)(c[3] >> 11);
}

// the unit complex normal of (seed, realisation, channel, bin): E|xi|^2 = 2
EFD_NOISE_FN void draw_xi(uint64_t seed, uint32_t realisation, uint32_t channel, uint64_t bin,
                          double& re, double& im) {
    uint64_t a, b;
    draw_bits(seed, realisation, channel, bin, a, b);
    const double two53 = 1.0 / 9007199254740992.0;
    const double u1 = (double)(a + 1) * two53;   // (a + 1 <= 2^53: exact)
    const double u2 = (double)b * two53;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * u2, &s, &c);
#else
    const double ph = 6.283185307179586476925286766559 * u2;
    s = sin(ph);
    c = cos(ph);
#endif
    re = r * c;
    im = r * s;
}

// a gain that carries noise: neither 0 nor NaN (the bin the likelihood drops at f = 0 and the
// bins outside a template's mask have one of the two)
EFD_NOISE_FN bool live_gain(double g) { return g == g && g != 0.0; }

}  // namespace efdnoise
