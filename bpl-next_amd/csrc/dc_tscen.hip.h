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
// Stage 1, dc_tscen_sim<H2H, ET>: ONE WAVE PER SIMULATION, dc_paths_sim's group matches, ranking, bracket fill and
//   knockout rounds -- the recording kernels' shared text (dc_tournament_sim.hip.h) -- without its ballots, match
//   words and slot bytes; dc_tournament_body.hip.inc and its four kernels are untouched.  Through the text's
//   callables a key lane keeps class x stride of its fixtures in a register over all blocks of the
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
// On a live matchday (`in_play`, `log_weights`) stage 1 is dctq::cup_scen_live[_table]
//   (dc_tournament_live_queries.hip.h): this file's kernel text with LIVE set.  fix_code then has F + L entries, a key
//   F + m is match m in play, and its class is formed from the FINAL score in the listed orientation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_scenario.hip.h"     // dcsc::CODE_CAP_SHIFT, wave_sum_u32
#include "dc_tournament_sim.hip.h"   // dct::sim_enter, sim_play, sim_leave; dct::TournamentArgs and what it includes

namespace dcts {

constexpr int TSCEN_WAVES = dct::SIM_WAVES;
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
#define DCT_SIM_NAME dc_tscen_sim
#define DCT_SIM_ALLOC false
#include "dc_tscen_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
// the same text under a best-of-rest allocation table (four more instantiations)
#define DCT_SIM_NAME scen_alloc_sim
#define DCT_SIM_ALLOC true
#include "dc_tscen_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC

}  // namespace dcts
