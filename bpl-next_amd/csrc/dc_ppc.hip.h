// dc_ppc.hip.h -- posterior predictive replications of observed fixtures, simulated and reduced in one
// pass (posterior_predictive_check, bpl/ppc.py).  The [R, m] scorelines are never stored unless asked for.
//
// Replication r uses posterior draw s = r mod S for EVERY fixture.  Query fixture i (model indices h, a,
// fixture id f = fid[i], or i without ids) of replication r draws its scoreline with the exact sampler,
// dcr::sample_scoreline (dc_sampler.hip.h), on the threefry block (r, f) under the caller's key (no
// max_goals truncation, goals capped at 255).  The log-rates are those of dc_posterior.hip.h: the plain
// form (VENUE = 0, dc_season's) or the venue BRANCH form (VENUE = 1, dc_tournament's, with
// on = 1 - neutral_venue).  tests/ppc_ref.py restates this in numpy, operation for operation.
//
// Per replication row the kernel writes
//   score [(G+1)^2] u32   scoreline counts, row min(x, G), column min(y, G)
//   outcome [3] u32       home wins, draws, away wins (uncapped scorelines)
//   sums [5] i64          sum x, sum y, sum x^2, sum y^2, sum x y
//   team [k, 4] u32       per team slot: goals for, goals against, wins, draws
//   home / away goals [m] u8 (optional)
//
// Layout: ONE WORKGROUP PER REPLICATION (grid = R), PPC_WAVES waves, lane = fixture (i = tid, tid + 256, ...).
//   The row's team table and scoreline bins live in LDS and take integer LDS atomics: a slot's (GF, GA)
//   and (W, D) pairs are one u64 add each (a u32 half cannot carry: 255 x PPC_MAX_FIXTURES < 2^32).
//   Outcome counts and the five goal sums stay in each lane's registers, are reduced across the wave by
//   xor butterflies and added to LDS once per wave.  After a barrier the workgroup stores the row with
//   plain stores: every row has exactly one writer and every sum is an integer, so the outputs are
//   bit-identical from run to run.  One wave per replication (dc_season's layout) would need a private
//   team table per wave: four of them at 16 B per slot fill 64 KB at 1024 teams and leave no room for the
//   bins.  Sharing the row across four waves keeps LDS at ~17 KB (1024 slots) and spreads a long
//   fixture list (40 000 fixtures) over 256 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_posterior.hip.h"   // dcq::Posterior, log_rates_plain, log_rates_venue_branch
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dcppc {

constexpr int PPC_WAVES = 4;
constexpr int PPC_MAX_TEAMS = 1024;           // include/bplhip.h BPLHIP_PPC_MAX_TEAMS
constexpr int PPC_MAX_GOALS = 15;             // include/bplhip.h BPLHIP_PPC_MAX_GOALS: bins <= 256
constexpr int PPC_MAX_BINS = (PPC_MAX_GOALS + 1) * (PPC_MAX_GOALS + 1);

struct PpcArgs {
    int m, k, G;                     // query fixtures, team slots, max_goals
    uint32_t key_hi, key_lo;
    dcq::Posterior<double> P;        // row-major, plain (VENUE = 0) or venue (VENUE = 1)
    const uint32_t* fix;             // [m]: home | away << 16 (model indices)
    const uint32_t* slot;            // [m]: home slot | away slot << 16
    const uint32_t* fid;             // [m] fixture ids (RNG counter) or null: i
    const uint8_t* neutral;          // VENUE = 1: [m]
    const uint32_t* conf_idx;        // VENUE = 1 with confederations: [m] home | away << 16
    uint32_t* score;                 // [R, (G+1)^2]
    uint32_t* outcome;               // [R, 3]
    long long* sums;                 // [R, 5]
    uint32_t* team;                  // [R, k, 4]
    uint8_t* home_goals;             // [R, m] or null
    uint8_t* away_goals;
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool VENUE>
__global__ __launch_bounds__(64 * PPC_WAVES) void dc_ppc(PpcArgs A) {
#pragma clang fp contract(off)
    __shared__ unsigned long long tab[PPC_MAX_TEAMS * 2];   // per slot: GF | GA << 32, W | D << 32
    __shared__ uint32_t bins[PPC_MAX_BINS];
    __shared__ unsigned long long red[7];                  // home wins, draws, the five goal sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = A.k, m = A.m, G = A.G, nb = (G + 1) * (G + 1);
    for (int i = tid; i < 2 * k; i += blockDim.x) tab[i] = 0ull;
    for (int i = tid; i < nb; i += blockDim.x) bins[i] = 0u;
    if (tid < 7) red[tid] = 0ull;
    __syncthreads();

    const uint32_t r = blockIdx.x;
    const int s = (int)(r % (uint32_t)A.P.S);
    const double rho = A.P.corr[s];
    unsigned long long hw = 0, dr = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int i = tid; i < m; i += blockDim.x) {
        const uint32_t hw_ = A.fix[i];
        const int h = (int)(hw_ & 0xFFFFu), a = (int)(hw_ >> 16);
        double eh, ea;
        if constexpr (VENUE) {
            dcq::log_rates_venue_branch(A.P, s, h, a, !A.neutral[i], &eh, &ea);
            if (A.P.C) {
                const uint32_t ci = A.conf_idx[i];
                dcq::add_confederations(A.P, s, (int)(ci & 0xFFFFu), (int)(ci >> 16), &eh, &ea);
            }
        } else {
            dcq::log_rates_plain(A.P, s, h, a, &eh, &ea);
        }
        const double lh = exp(eh), la = exp(ea);
        uint32_t o0, o1;
        nd::tf_block(A.key_hi, A.key_lo, r, A.fid ? A.fid[i] : (uint32_t)i, &o0, &o1);
        int x, y;
        dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
        const uint32_t sl = A.slot[i];
        const int hs = (int)(sl & 0xFFFFu), as = (int)(sl >> 16);
        const unsigned long long ux = (unsigned)x, uy = (unsigned)y;
        atomicAdd(&tab[2 * hs], ux | (uy << 32));
        atomicAdd(&tab[2 * as], uy | (ux << 32));
        const unsigned long long home_res = x > y ? 1ull : x == y ? (1ull << 32) : 0ull;
        const unsigned long long away_res = y > x ? 1ull : x == y ? (1ull << 32) : 0ull;
        if (home_res) atomicAdd(&tab[2 * hs + 1], home_res);
        if (away_res) atomicAdd(&tab[2 * as + 1], away_res);
        atomicAdd(&bins[min(x, G) * (G + 1) + min(y, G)], 1u);
        hw += x > y;
        dr += x == y;
        sx += ux;
        sy += uy;
        sxx += ux * ux;
        syy += uy * uy;
        sxy += ux * uy;
        if (A.home_goals) {
            A.home_goals[(size_t)r * m + i] = (uint8_t)x;
            A.away_goals[(size_t)r * m + i] = (uint8_t)y;
        }
    }
    const unsigned long long v[7] = {wave_sum_u64(hw), wave_sum_u64(dr), wave_sum_u64(sx), wave_sum_u64(sy),
                                     wave_sum_u64(sxx), wave_sum_u64(syy), wave_sum_u64(sxy)};
    if (lane == 0)
        for (int j = 0; j < 7; ++j) atomicAdd(&red[j], v[j]);
    __syncthreads();

    // the row, one writer: the team table as [k, 4] u32 (the u64 pairs are little-endian u32 pairs)
    const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tab);
    uint32_t* team = A.team + (size_t)r * k * 4;
    for (int i = tid; i < 4 * k; i += blockDim.x) team[i] = t32[i];
    uint32_t* score = A.score + (size_t)r * nb;
    for (int i = tid; i < nb; i += blockDim.x) score[i] = bins[i];
    if (tid < 3) {
        const uint32_t hwins = (uint32_t)red[0], draws = (uint32_t)red[1];
        A.outcome[(size_t)r * 3 + tid] = tid == 0 ? hwins : tid == 1 ? draws : (uint32_t)m - hwins - draws;
    }
    if (tid >= 64 && tid < 69) A.sums[(size_t)r * 5 + (tid - 64)] = (long long)red[2 + (tid - 64)];
}

}  // namespace dcppc
