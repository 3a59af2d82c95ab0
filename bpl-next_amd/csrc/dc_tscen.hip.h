// dc_tscen.hip.h -- the joint result of a few chosen group fixtures against knockout targets (tournament_scenarios,
// bpl/neutral_dixon_coles.py): every combination of the key fixtures' clipped margins cross-tabulated against every
// team's targets "plays knockout round r", "wins the tournament" and "wins its group", over the SAME simulations
// dc_tournament.hip.h and dc_paths.hip.h play.  Simulation j takes draw j mod S, the threefry blocks, the ranking, the
// bracket and the knockout rule of dc_paths_sim, through the same device functions (dct::play, dck::decide,
// dch::pair_rank, dctab::*), so that under one key every scoreline, position and winner is theirs bit for bit
// (tests/test_gpu_tournament_scenarios.py).  No [N, ...] array exists on the device: the simulations pass through a
// workspace of `chunk` records, two kernels per chunk, as in dc_scenario.hip.h.
//
// The scenario index is dc_scenario.hip.h's: key fixture q with cap c_q has 2 c_q + 1 classes, class = c_q -
//   clip(first-listed goals - second-listed goals, -c_q, c_q) -- the LISTED orientation, as dc_paths_sim's ballots,
//   also when a host listed second plays at home -- and a scenario is one class per key, row-major in the caller's
//   order.  Every group fixture carries one u16 code, stride | cap << dcsc::CODE_CAP_SHIFT, 0 for a fixture that is no
//   key: the keys may sit in any block of 64 and on any lane.
// Stage 1, dc_tscen_sim<H2H, ET>: ONE WAVE PER SIMULATION, dc_paths_sim's body statement for statement for the group
//   matches, the ranking, the bracket fill and the knockout rounds, without its ballots, match words and slot bytes
//   -- a body of its own rather than a flag in dc_paths_sim or dc_tournament_body.hip.inc, so the eight tournament
//   kernels are untouched.  A key lane keeps class x stride of its fixtures in a register over all blocks of the
//   list, and the wave adds the lanes once per simulation (an integer butterfly).  Record of simulation c of the chunk
//   (simulation j0 + c):
//       scen[c]                    u32  the scenario index
//       tset[slot * chunk + c]     u8   bits 0..R = (1 << stage) - 1 (bit k < R: plays knockout round k, bit R: wins
//                                       the tournament), bit R + 1 = first in its group; SLOT-MAJOR as in dc_scenario
//   -- 4 + n bytes per simulation (52 B for a 48-team World Cup against dc_paths_sim's 316).  With ET the
//   [round][kind] histogram of dc_knockout.hip.h is kept as in dc_paths_sim.  Nothing else is counted here.
// Stage 2: dcsc::dc_scenario_count, unchanged, on these records with K = R + 2 targets: it reads nothing but n, K, nc,
//   chunk, M, tile_rows, scen, tset and its two tables.
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_scenario.hip.h"     // dcsc::CODE_CAP_SHIFT, wave_sum_u32
#include "dc_tournament.hip.h"   // dct::TournamentArgs, play and what it includes

namespace dcts {

constexpr int TSCEN_WAVES = 4;
constexpr int TSCEN_BLOCKS_PER_CU = 4;

struct TscenArgs {
    long long j0;                 // first simulation of the chunk
    int nc, chunk;                // simulations in this chunk, the workspace's chunk length
    const uint16_t* fix_code;     // [nf]: stride | cap << dcsc::CODE_CAP_SHIFT of a key fixture, 0 otherwise
    uint32_t* scen;               // [chunk] scenario indices
    uint8_t* tset;                // [n, chunk] target sets by slot
};

// A.n_sims, A.stage_counts, A.pos_counts, A.sim_stage and K.sim_decided are not read: P says which simulations.
// The host launches it with groups and at least one group fixture only (there is nothing to key on otherwise); the
// branches without groups are dc_paths_sim's and leave scenario 0.
template <bool H2H, bool ET>
__global__ __launch_bounds__(64 * TSCEN_WAVES) void dc_tscen_sim(dct::TournamentArgs A, dch::PairArgs H,
                                                                 dck::KnockoutArgs K, TscenArgs P) {
    using namespace dct;
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[TSCEN_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[TSCEN_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[TSCEN_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = H2H ? (int)(blockDim.x >> 6) : TSCEN_WAVES;
    const int n = A.n, nf = A.nf, nb = 1 << A.rounds;
    if constexpr (ET) {
        if (threadIdx.x < dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS) dck::decided_hist()[threadIdx.x] = 0u;
    }
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS; i += blockDim.x) sinfo[i] = i < n ? A.slot_info[i] : 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_CODES; i += blockDim.x)
        code_pos[i] = A.n_groups ? A.code_pos[i] : (uint8_t)0xFF;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    uint8_t* br = bracket[wave];
    uint8_t* stg = stage[wave];
    const bool slot_lane = lane < n;
    const bool groups = A.n_groups > 0;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane && groups);
    const int my_group = slot_lane ? (int)(sinfo[lane] >> 25) : -1;
    const int first_slot = !groups && lane < nb ? (int)A.first_round[lane] : 0;
    const int advance = A.advance;

    const int waves = (int)gridDim.x * nw;
    for (int c = (int)blockIdx.x * nw + wave; c < P.nc; c += waves) {
        const long long j = P.j0 + c;
        const int s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        int my_stage = 1, pos = 0;
        uint32_t cell = 0u;   // class x stride of this lane's key fixtures, over all blocks of the list
        if (groups) {
            // ---- group matches, lane = fixture
            dctab::store_row(table, lane, slot_lane, init);
            if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
            dcr::wave_lds_order();
            for (int base = 0; base < nf; base += 64) {
                const int f = base + lane;
                if (f < nf) {
                    const uint32_t sl = A.fix[f];
                    const int p = (int)(sl & 0xFFu);
                    int hs, as, x, y;
                    play(A, sinfo, s, ju, (uint32_t)f, p, (int)(sl >> 8), &hs, &as, &x, &y);
                    dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                    if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                    // (x, y) is in the home orientation: a host listed second was swapped in
                    const int margin = hs == p ? x - y : y - x;
                    const uint32_t code = P.fix_code[f];
                    const int cap = (int)(code >> dcsc::CODE_CAP_SHIFT);   // (0 for a fixture that is no key)
                    cell += (uint32_t)(cap - min(max(margin, -cap), cap)) * (code & ((1u << dcsc::CODE_CAP_SHIFT) - 1u));
                }
            }
            cell = dcsc::wave_sum_u32(cell);
            dcr::wave_lds_order();
            const dctab::Row row = dctab::load_row(table, TOURNAMENT_MAX_TEAMS, lane, slot_lane);
            if constexpr (!H2H) dcr::wave_lds_order();
            // ---- ranking, lane = slot: dc_tournament's, statement for statement
            uint32_t r0 = 0u, r1;
            if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
            if constexpr (H2H) {
                pos = dch::pair_rank<true>(pair, H.pitch, n, lane, slot_lane, row, r0, my_group);
                dcr::wave_lds_order();
            }
            const dctab::Keys Q = dctab::rank_keys(row, r0);
            if constexpr (!H2H) {
                for (int k = 0; k < n; ++k) {
                    const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
                    const int gk = __builtin_amdgcn_readlane(my_group, k);
                    const bool better = o1k > Q.k1 || (o1k == Q.k1 && (o2k > Q.k2 || (o2k == Q.k2 && k < lane)));
                    pos += (gk == my_group && better) ? 1 : 0;
                }
            }
            const int rest = slot_lane && pos == advance ? 1 : 0;
            int rest_rank = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
                const int rk = __builtin_amdgcn_readlane(rest, k);
                const bool better = o1k > Q.k1 || (o1k == Q.k1 && (o2k > Q.k2 || (o2k == Q.k2 && k < lane)));
                rest_rank += (rk && better) ? 1 : 0;
            }
            int code = -1;
            if (slot_lane && pos < advance) code = TOURNAMENT_MAX_GROUP * my_group + pos;
            else if (rest) code = 128 + rest_rank;
            const int bpos = code >= 0 && code < TOURNAMENT_CODES ? (int)code_pos[code] : 0xFF;
            my_stage = bpos < nb ? 1 : 0;
            if (bpos < nb) br[bpos] = (uint8_t)lane;
        } else if (lane < nb) {
            br[lane] = (uint8_t)first_slot;
        }
        if (slot_lane) stg[lane] = (uint8_t)my_stage;
        dcr::wave_lds_order();
        // ---- knockout rounds, lane = match
        int k0 = 0;
        for (int r = 0; r < A.rounds; ++r) {
            const int M = nb >> (r + 1);
            int win = 0;
            if (lane < M) {
                const int p = br[2 * lane], q = br[2 * lane + 1];
                const uint32_t ctr = KNOCKOUT_COUNTER | ((uint32_t)(k0 + lane) << 5);
                if constexpr (ET) {
                    int how = 0;
                    win = dck::decide(A, K, sinfo, s, ju, ctr, p, q, (K.legs_mask >> r) & 1u, &how);
                    atomicAdd(&dck::decided_hist()[r * dck::DECIDED_KINDS + how], 1u);
                } else {
                    win = p;   // after TOURNAMENT_ATTEMPTS level attempts the first-listed side goes through
                    for (int t = 0; t < TOURNAMENT_ATTEMPTS; ++t) {
                        int hs, as, x, y;
                        play(A, sinfo, s, ju, ctr | (uint32_t)t, p, q, &hs, &as, &x, &y);
                        if (x != y) {
                            win = x > y ? hs : as;
                            break;
                        }
                    }
                }
            }
            dcr::wave_lds_order();   // every lane has read its pair before entry m is overwritten
            if (lane < M) {
                br[lane] = (uint8_t)win;
                stg[win] = (uint8_t)(r + 2);
            }
            dcr::wave_lds_order();
            k0 += M;
        }
        if (lane == 0) P.scen[c] = cell;
        if (slot_lane) {
            const uint32_t st = stg[lane];
            // bits 0..R: the stage's targets; bit R + 1: first in its group
            const uint32_t top = groups && pos == 0 ? 1u << (A.rounds + 1) : 0u;
            P.tset[(size_t)lane * P.chunk + c] = (uint8_t)(((1u << st) - 1u) | top);
        }
        dcr::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
    }
    if constexpr (ET) {
        __syncthreads();
        if (threadIdx.x < A.rounds * dck::DECIDED_KINDS) {
            const uint32_t v = dck::decided_hist()[threadIdx.x];
            if (v) atomicAdd(&K.decided_counts[threadIdx.x], (unsigned long long)v);
        }
    }
}

}  // namespace dcts
