// The planner's random numbers, shared by cem_update_kernel (csrc/cem.hip) and cem_update_ex_kernel (csrc/mpc.hip): Philox4x32-10 and the
// Box-Muller transform on exact uniforms, as include/pivp_hip.h defines them for pivp_cem_update.  One definition, so that the two ops draw the
// same normal for the same (candidate, row, iteration, seed), bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace pivp {

struct Philox4 { unsigned x[4]; };
// Philox4x32-10 (Salmon et al. 2011, Random123): ten rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// Box-Muller on u1 = ((xa >> 8) + 0.5) 2^-24, u2 = ((xb >> 8) + 0.5) 2^-24.  n + 0.5 needs 25 significant bits once n >= 2^23, so the upper half of
// the range goes through the complement m = 2^24 - 1 - n (m + 0.5 is exact there): ln u1 = log1p(-(m + 0.5) 2^-24) and, the angle being periodic,
// 2 pi u2 = -2 pi (m + 0.5) 2^-24.  Every argument that reaches logf / log1pf / sincospif is therefore the exact value of the definition.
__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& z0, float& z1) {
    const unsigned na = xa >> 8, nb = xb >> 8;
    float l;
    if (na < (1u << 23)) l = logf(((float)na + 0.5f) * 5.9604644775390625e-08f);
    else l = log1pf(-(((float)(0xFFFFFFu - na) + 0.5f) * 5.9604644775390625e-08f));
    const float r = sqrtf(-2.0f * l);
    const float a = nb < (1u << 23) ? ((float)nb + 0.5f) * 1.1920928955078125e-07f : -(((float)(0xFFFFFFu - nb) + 0.5f) * 1.1920928955078125e-07f);
    float sn, cs;
    sincospif(a, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}

}  // namespace pivp
