// dc_sampler.hip.h -- the exact scoreline sampler and the wave helpers shared by the simulation
// kernels (dc_season, dc_tournament, dc_ppc).
// Randomness: threefry-2x32-20 (nd::tf_block) under the caller's key; a block (c0, c1) gives two words
// (o0, o1) and the uniforms u = (o + 0.5) 2^-32 (unit_open).  The counter space, in ONE place:
//     c0 = simulation / replication j
//     c1 = f                          fixture f (season and group fixtures; ppc: the fixture id)
//     c1 = 0x80000000 | slot          TIEBREAK_COUNTER: o0 is the slot's table tie-break word
//     c1 = 0x40000000 | k << 5 | t    dct::KNOCKOUT_COUNTER: knockout match k (over all rounds), attempt t < 32
//   under the extra-time rule (dc_knockout.hip.h) the same blocks, with t meaning:
//     t = 0                           the only leg, or leg 1
//     t = 1                           leg 2
//     t = 2                           extra time
//     t = 3                           the shoot-out (o0 only)
//   simulate_season's play-offs (dc_playoff.hip.h) use the same four blocks, k numbered over the bracket's matches.
//     c0 = 0, c1 = 0x20000000         dclive::RESAMPLE_COUNTER (dc_live.hip.h): o0 is the call's ONE systematic-
//                                     resampling offset; fixtures stay below 2^20, bit 31 marks the tie-break and
//                                     bit 30 the knockout, so bit 29 alone collides with none of them
// The scoreline is drawn EXACTLY from  max(tau, 0) Pois(x; lh) Pois(y; la) / Z  (no max_goals
// truncation) by two inverse-CDF walks, all float64:
//     t00 = max(1 - lh la rho, 0), t01 = max(1 + lh rho, 0), t10 = max(1 + la rho, 0), t11 = max(1 - rho, 0)
//     q0 = exp(-la), q1 = q0 la;  c0 = 1 + (t00-1) q0 + (t01-1) q1,  c1 = 1 + (t10-1) q0 + (t11-1) q1,  c_k = 1 (k >= 2)
//     p0 = exp(-lh), p1 = p0 lh;  Z = 1 + p0 (c0-1) + p1 (c1-1)      (= sum_x p_x c_x: c_x = sum_y tau(x,y) Pois(y))
//     home x: p_k = p_{k-1} lh / k, the first k with  u1 Z < sum_{i<=k} p_i c_i           (capped at 255)
//     away y: p'_0 = q0, p'_y = p'_{y-1} la / y, the first y with  u2 c_x < sum_{i<=y} p'_i tau(x,i)  (capped at 255)
// so x is drawn from its marginal p_x c_x / Z and y from its conditional tau(x,y) Pois(y) / c_x.  With
// nothing clipped Z = c0 = c1 = 1: the home marginal is exactly Poisson and tau only reshapes y | x <= 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcr {

constexpr uint32_t TIEBREAK_COUNTER = 0x80000000u;

// One scoreline from the two uniforms (contraction off: same rounding as the numpy restatements,
// tests/season_ref.py, operation for operation).
__device__ inline void sample_scoreline(double lh, double la, double rho, double u1, double u2, int* xo, int* yo) {
#pragma clang fp contract(off)
    const double t00 = fmax(1.0 - lh * la * rho, 0.0);
    const double t01 = fmax(1.0 + lh * rho, 0.0);
    const double t10 = fmax(1.0 + la * rho, 0.0);
    const double t11 = fmax(1.0 - rho, 0.0);
    const double q0 = exp(-la), q1 = q0 * la;
    const double c0 = 1.0 + (t00 - 1.0) * q0 + (t01 - 1.0) * q1;
    const double c1 = 1.0 + (t10 - 1.0) * q0 + (t11 - 1.0) * q1;
    const double p0 = exp(-lh), p1 = p0 * lh;
    const double Z = 1.0 + p0 * (c0 - 1.0) + p1 * (c1 - 1.0);
    // home goals: marginal p_x c_x / Z
    const double th = u1 * Z;
    double p = p0, acc = p0 * c0;
    int x = 0;
    while (!(th < acc) && x < 255) {
        ++x;
        p = p * lh / (double)x;
        acc = acc + (x == 1 ? p * c1 : p);
    }
    // away goals given x: tau(x, y) Pois(y; la) / c_x
    const double ta = u2 * (x == 0 ? c0 : x == 1 ? c1 : 1.0);
    const double tau0 = x == 0 ? t00 : x == 1 ? t10 : 1.0;
    const double tau1 = x == 0 ? t01 : x == 1 ? t11 : 1.0;
    p = q0;
    acc = q0 * tau0;
    int y = 0;
    while (!(ta < acc) && y < 255) {
        ++y;
        p = p * la / (double)y;
        acc = acc + (y == 1 ? p * tau1 : p);
    }
    *xo = x;
    *yo = y;
}

__device__ __forceinline__ double unit_open(uint32_t o) { return ((double)o + 0.5) * 0x1p-32; }
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int k) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
    return ((unsigned long long)hi << 32) | lo;
}
// the wave's own LDS rows are written and read by different lanes of the same wave: LDS operations
// of a wave complete in order, this keeps the compiler from moving them across each other
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace dcr
