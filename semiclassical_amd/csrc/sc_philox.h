// Counter-based standard-normal deviates of the device samplers (sc_sample.hip, sc_thermal.hip): Philox4x32-10 (Salmon et al.,
// SC'11: ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) and Box-Muller, defined ONCE.
//     key     = (seed lo, seed hi)
//     counter = (trajectory index lo, trajectory index hi, pair index | subsequence[32..55] << 8, subsequence[0..31])
// One call gives 128 bits = two 53-bit uniforms = one Box-Muller pair.  Pair index < 256, subsequence < 2^56.
#pragma once
#include "sc_common.h"

namespace {

struct PhiloxKey { uint32_t k0, k1; };

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, PhiloxKey key,
                                              uint32_t (&out)[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t k0 = key.k0, k1 = key.k1;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 53 random bits -> uniform in (0, 1]  (never 0: the logarithm of Box-Muller stays finite)
__device__ __forceinline__ double uniform_open0(uint32_t hi, uint32_t lo) {
    const uint64_t bits = (((uint64_t)hi << 32) | lo) >> 11;            // 53 bits
    return ((double)bits + 1.0) * (1.0 / 9007199254740992.0);
}

// the Box-Muller pair (a, b) of pair index `pair` of the trajectory with global index g; sub_hi = (subsequence >> 32) << 8,
// sub_lo = the low word of the subsequence
__device__ __forceinline__ void philox_normal_pair(uint64_t g, uint32_t pair, uint32_t sub_hi, uint32_t sub_lo, PhiloxKey key,
                                                   double &a, double &b) {
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), pair | sub_hi, sub_lo, key, r);
    const double u1 = uniform_open0(r[0], r[1]), u2 = uniform_open0(r[2], r[3]);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    a = rad * cs; b = rad * sn;
}

}  // namespace
