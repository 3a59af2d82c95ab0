// dc_season.hip.h -- the rest of a season, simulated jointly over the posterior (simulate_season,
// bpl/base.py; SURVEY.md §8 row f-2: league-table questions are the predict path's main use).
//
// Simulation j uses posterior draw s = j mod S and plays EVERY remaining fixture from that one draw
// (a team strong in the draw is strong in all its matches), then ranks the table.  Fixture f =
// (h, a) takes the plain log-rates (written out below, own argument layout: with dcq::Posterior the kernel
// measured 2-3 % slower), rho = corr_coef[s] and the threefry block (j, f) for dcr::sample_scoreline's exact draw.
// (Tried and not kept: a record and a fixture step shared with dc_leverage_sim -- with a common base record all four
// league instantiations compiled differently, and the step alone reordered instructions in dc_leverage_sim<true>.)
// The table (points, GF, GA on top of the current table) is booked through dc_table.hip.h and ranked below.
// tests/season_ref.py restates all of this in numpy, operation for operation (contraction is off in
// the rates and the sampler: the only device/host difference left is exp's last bit).
//
// Layout: ONE WAVE PER SIMULATION, SEASON_WAVES per workgroup, grid-stride over the simulations.
//   sampling  lane = fixture (f = lane, lane + 64, ...): rates from the float64 tables (L2-resident),
//             one threefry block, the two walks; points / GF / GA into the wave's private LDS table.
//   ranking   lane = slot (n <= 64): a lane counts the slots ahead of it -- no sort.
//   counts    a per-workgroup u32 LDS histogram [slot][position] and u64 LDS sums of points and GD,
//             flushed ONCE per workgroup with global u64 integer atomics.  Integer atomics only: the
//             results are bit-identical whatever the schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dcs {

constexpr int SEASON_WAVES = 4;
constexpr int SEASON_BLOCKS_PER_CU = 4;
constexpr int SEASON_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;

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

// H2H: the table is ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  (The venue-aware rate forms of
// dc_posterior.hip.h are not wired into the season kernel.)
template <bool H2H>
__global__ __launch_bounds__(64 * SEASON_WAVES) void dc_season(SeasonArgs A, dch::PairArgs H) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist[SEASON_MAX_TEAMS * SEASON_MAX_TEAMS];
    __shared__ unsigned long long bsum[2][SEASON_MAX_TEAMS];
    __shared__ int32_t tab[SEASON_WAVES][3][SEASON_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : SEASON_WAVES;
    const int n = A.n, nf = A.nf;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x < 2 * SEASON_MAX_TEAMS) (&bsum[0][0])[threadIdx.x] = 0ull;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;   // (not formed in the overall order: even unused it changed the compiled code)
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    long long psum = 0, gdsum = 0;   // this lane's slot over the wave's simulations

    const long long waves = (long long)gridDim.x * nw;
    for (long long j = (long long)blockIdx.x * nw + wave; j < A.n_sims; j += waves) {
        const int s = (int)(j % A.S);
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
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
            dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
            if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            if (A.home_goals) {
                A.home_goals[(size_t)j * nf + f] = (uint8_t)x;
                A.away_goals[(size_t)j * nf + f] = (uint8_t)y;
            }
        }
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, SEASON_MAX_TEAMS, lane, slot_lane);
        // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
        if constexpr (!H2H) dcr::wave_lds_order();
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int ahead = 0;
        if constexpr (H2H) {
            ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
            dcr::wave_lds_order();
        } else {
            // (written out: in a helper the loop lost its scalar counter, dc_table.hip.h)
            const dctab::Keys K = dctab::rank_keys(row, r0);
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(K.k1, k), o2k = dcr::readlane_u64(K.k2, k);
                ahead += (o1k > K.k1 || (o1k == K.k1 && (o2k > K.k2 || (o2k == K.k2 && k < lane)))) ? 1 : 0;
            }
        }
        if (slot_lane) {
            atomicAdd(&hist[lane * n + ahead], 1u);
            psum += row.pts;
            gdsum += row.gf - row.ga;
            if (A.sim_points) A.sim_points[(size_t)j * n + lane] = row.pts;
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
