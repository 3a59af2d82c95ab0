// dc_season.hip.h -- the rest of a season, simulated jointly over the posterior (simulate_season,
// bpl/base.py; SURVEY.md §8 row f-2: league-table questions are the predict path's main use).
//
// Simulation j uses posterior draw s = j mod S and plays EVERY remaining fixture from that one draw
// (a team strong in the draw is strong in all its matches), then ranks the table.  Fixture f =
// (h, a) of simulation j:
//     lh = exp((attack[s,h] - defence[s,a]) + ha),  ha = home_advantage[s] or home_advantage[s,h]
//     la = exp(attack[s,a] - defence[s,h]),  rho = corr_coef[s]
//     (o0, o1) = threefry-2x32-20 block (j, f) under the caller's key,  u = (o + 0.5) 2^-32
// The scoreline is drawn EXACTLY from  max(tau, 0) Pois(x; lh) Pois(y; la) / Z  (no max_goals
// truncation) by two inverse-CDF walks, all float64:
//     t00 = max(1 - lh la rho, 0), t01 = max(1 + lh rho, 0), t10 = max(1 + la rho, 0), t11 = max(1 - rho, 0)
//     q0 = exp(-la), q1 = q0 la;  c0 = 1 + (t00-1) q0 + (t01-1) q1,  c1 = 1 + (t10-1) q0 + (t11-1) q1,  c_k = 1 (k >= 2)
//     p0 = exp(-lh), p1 = p0 lh;  Z = 1 + p0 (c0-1) + p1 (c1-1)      (= sum_x p_x c_x: c_x = sum_y tau(x,y) Pois(y))
//     home x: p_k = p_{k-1} lh / k, the first k with  u1 Z < sum_{i<=k} p_i c_i           (capped at 255)
//     away y: p'_0 = q0, p'_y = p'_{y-1} la / y, the first y with  u2 c_x < sum_{i<=y} p'_i tau(x,i)  (capped at 255)
// so x is drawn from its marginal p_x c_x / Z and y from its conditional tau(x,y) Pois(y) / c_x.  With
// nothing clipped Z = c0 = c1 = 1: the home marginal is exactly Poisson and tau only reshapes y | x <= 1.
// The table (points, GF, GA on top of the current table) is ordered by points, goal difference, goals
// for (all descending), then o0 of block (j, 0x80000000 | slot) descending, then slot ascending; a
// slot's position is the number of slots ahead of it.  tests/season_ref.py restates all of this in
// numpy, operation for operation (contraction is off below: the only device/host difference left is
// exp's last bit).
//
// Layout: ONE WAVE PER SIMULATION, SEASON_WAVES per workgroup, grid-stride over the simulations.
//   sampling  lane = fixture (f = lane, lane + 64, ...): rates from the float64 tables (L2-resident),
//             one threefry block, the two walks; points / GF / GA into the wave's private LDS table
//             with integer LDS atomics (two lanes may share a slot).
//   ranking   lane = slot (n <= 64): two packed keys per slot, (points, GD) and (GF, o0); a lane
//             counts the slots ahead of it over wave-uniform readlanes -- no sort.
//   counts    a per-workgroup u32 LDS histogram [slot][position] and u64 LDS sums of points and GD,
//             flushed ONCE per workgroup with global u64 integer atomics.  Integer atomics only: the
//             results are bit-identical whatever the schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nuts_dev.hip.h"   // nd::tf_block

namespace dcs {

constexpr int SEASON_WAVES = 4;
constexpr int SEASON_BLOCKS_PER_CU = 4;
constexpr int SEASON_MAX_TEAMS = 64;
constexpr uint32_t TIEBREAK_COUNTER = 0x80000000u;

struct SeasonArgs {
    int S, T, n, nf;                 // draws, model teams, table slots, fixtures
    long long n_sims;
    uint32_t key_hi, key_lo;
    int win, draw, loss;
    const double* attack;            // [S,T]
    const double* defence;           // [S,T]
    const double* home_adv;          // [S] (ha_stride = 0) or [S,T] (ha_stride = T)
    int ha_stride;
    const double* corr;              // [S]
    const uint32_t* fix;             // [nf]: home | away << 16 (model indices)
    const uint16_t* fix_slot;        // [nf]: home slot | away slot << 8
    const int32_t* init;             // [3, n]: points, GF, GA of the current table
    unsigned long long* counts;      // [n, n] position counts (zeroed by the caller)
    unsigned long long* sums;        // [2, n] points, GD sums (two's complement, zeroed by the caller)
    int32_t* sim_points;             // [n_sims, n] or null
    uint8_t* sim_position;           // [n_sims, n] or null
    uint8_t* home_goals;             // [n_sims, nf] or null
    uint8_t* away_goals;             // [n_sims, nf] or null
};

// One scoreline from the two uniforms (see the header comment; contraction off: same rounding as
// the numpy restatement, operation for operation).
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

template <bool VENUE>
__global__ __launch_bounds__(64 * SEASON_WAVES) void dc_season(SeasonArgs A) {
    static_assert(!VENUE, "the venue-aware rate form (dc_predict.hip.h VENUE = 1) is not wired into the season kernel");
    __shared__ uint32_t hist[SEASON_MAX_TEAMS * SEASON_MAX_TEAMS];
    __shared__ unsigned long long bsum[2][SEASON_MAX_TEAMS];
    __shared__ int32_t tab[SEASON_WAVES][3][SEASON_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = A.n, nf = A.nf;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x < 2 * SEASON_MAX_TEAMS) (&bsum[0][0])[threadIdx.x] = 0ull;
    __syncthreads();

    int32_t* tp = tab[wave][0];
    int32_t* tf = tab[wave][1];
    int32_t* ta = tab[wave][2];
    const bool slot_lane = lane < n;
    const int32_t p_init = slot_lane ? A.init[lane] : 0;
    const int32_t f_init = slot_lane ? A.init[n + lane] : 0;
    const int32_t a_init = slot_lane ? A.init[2 * n + lane] : 0;
    long long psum = 0, gdsum = 0;   // this lane's slot over the wave's simulations

    const long long waves = (long long)gridDim.x * SEASON_WAVES;
    for (long long j = (long long)blockIdx.x * SEASON_WAVES + wave; j < A.n_sims; j += waves) {
        const int s = (int)(j % A.S);
        if (slot_lane) {
            tp[lane] = p_init;
            tf[lane] = f_init;
            ta[lane] = a_init;
        }
        wave_lds_order();
        const double* att = A.attack + (size_t)s * A.T;
        const double* dfn = A.defence + (size_t)s * A.T;
        const double* hadv = A.ha_stride ? A.home_adv + (size_t)s * A.T : A.home_adv + s;
        const double rho = A.corr[s];
        for (int f = lane; f < nf; f += 64) {
            const uint32_t hw = A.fix[f];
            const int h = (int)(hw & 0xFFFFu), a = (int)(hw >> 16);
            const uint32_t sl = A.fix_slot[f];
            const int hs = (int)(sl & 0xFFu), as = (int)(sl >> 8);
            double eh = att[h] - dfn[a];
            eh = eh + (A.ha_stride ? hadv[h] : hadv[0]);
            const double lh = exp(eh), la = exp(att[a] - dfn[h]);
            uint32_t o0, o1;
            nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, (uint32_t)f, &o0, &o1);
            int x, y;
            sample_scoreline(lh, la, rho, unit_open(o0), unit_open(o1), &x, &y);
            const int ph = x > y ? A.win : x == y ? A.draw : A.loss;
            const int pa = y > x ? A.win : x == y ? A.draw : A.loss;
            atomicAdd(&tp[hs], ph);
            atomicAdd(&tp[as], pa);
            atomicAdd(&tf[hs], x);
            atomicAdd(&tf[as], y);
            atomicAdd(&ta[hs], y);
            atomicAdd(&ta[as], x);
            if (A.home_goals) {
                A.home_goals[(size_t)j * nf + f] = (uint8_t)x;
                A.away_goals[(size_t)j * nf + f] = (uint8_t)y;
            }
        }
        wave_lds_order();
        const int32_t pts = slot_lane ? tp[lane] : 0;
        const int32_t gf = slot_lane ? tf[lane] : 0;
        const int32_t ga = slot_lane ? ta[lane] : 0;
        wave_lds_order();   // (the next simulation's reset comes after these reads)
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        // (points, GD + 2^31) and (GF, tie-break word): the host bounds keep every field in 32 bits
        const unsigned long long k1 = ((unsigned long long)(uint32_t)pts << 32) | (uint32_t)((gf - ga) ^ (int32_t)0x80000000);
        const unsigned long long k2 = ((unsigned long long)(uint32_t)gf << 32) | r0;
        int ahead = 0;
        for (int k = 0; k < n; ++k) {
            const unsigned long long o1k = readlane_u64(k1, k), o2k = readlane_u64(k2, k);
            ahead += (o1k > k1 || (o1k == k1 && (o2k > k2 || (o2k == k2 && k < lane)))) ? 1 : 0;
        }
        if (slot_lane) {
            atomicAdd(&hist[lane * n + ahead], 1u);
            psum += pts;
            gdsum += gf - ga;
            if (A.sim_points) A.sim_points[(size_t)j * n + lane] = pts;
            if (A.sim_position) A.sim_position[(size_t)j * n + lane] = (uint8_t)ahead;
        }
    }
    if (slot_lane) {
        atomicAdd(&bsum[0][lane], (unsigned long long)psum);
        atomicAdd(&bsum[1][lane], (unsigned long long)gdsum);
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&A.counts[i], (unsigned long long)v);
    }
    if (threadIdx.x < 2 * n) {
        const int which = threadIdx.x / n, slot = threadIdx.x % n;
        const unsigned long long v = bsum[which][slot];
        if (v) atomicAdd(&A.sums[which * n + slot], v);
    }
}

}  // namespace dcs
