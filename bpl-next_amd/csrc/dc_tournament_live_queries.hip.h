// dc_tournament_live_queries.hip.h -- the three tournament queries on a day with group matches IN PROGRESS, and with
// weighted draws (tournament_paths', tournament_scenarios' and tournament_points' `in_play`, `reweight` and
// `log_weights`): dc_live_queries.hip.h's counterpart for the tournament family.  The weights
// are dc_tournament_live.hip.h's, formed once per call by dctl::live_cup_loglik and dclive::live_weights; what this
// file adds is the recording kernels that play on them.  They are the TEXT of dcpath::dc_paths_sim, dcts::dc_tscen_sim
// and dcgq::dc_gpts_sim and of their *_alloc_sim twins (dc_*_sim_kernel.hip.inc over dc_tournament_sim_*.hip.inc)
// with LIVE set, which changes a simulation in three places (and hands the wave's index to the scalar unit through
// readfirstlane, dc_tournament_sim_enter.hip.inc: held per lane, the wave-uniform simulation index, draw and LDS rows
// cost the vector registers the conditional sampler needs -- section 44):
//   - the draw of simulation j is dct::live_draw(A, V, j, lane): systematic resampling on the scan of the weights, or
//     j mod S without weights; formed again for every simulation, nothing of it is held across the chunk loop;
//   - the group-fixture loop runs over the CONCATENATED list, F fixtures still to kick off and after them the L
//     matches in play: one lane-stride loop over F + L with a per-lane branch.  Lane f < F plays dct::play as before;
//     lane F <= f < F + L plays match m = f - F by dct::play_live from its state on the block (j, F + m).  Both book
//     the final score (dctab::book, dch::pair_book under H2H) and hand it to the kernel's on_fixture with index f and
//     the first-listed slot, so dc_paths_sim's ballot of block f / 64, dc_tscen_sim's class sum and dc_gpts_sim's rows
//     cover the concatenated list at the positions the counting kernels read -- also when F is no multiple of 64 and
//     the first matches in play share a ballot block with the last ordinary fixtures.  One loop and not a second one
//     whose marks are merged: a second loop would ballot the shared block twice and OR two words in the workspace.
//     The price: a block that holds both kinds runs both branches one after the other (at the World Cup's last
//     matchday, F = 48 and L = 24, one trip of play and two of play_live against the simulator's one and one);
//   - when asked, lane 0 stores the draw and play_live the final scores in the listed order, [n_sims] and
//     [n_sims, L]: the only per-simulation arrays that do not pass through the chunk's workspace.
// The ranking, the allocation fill, the knockout rounds under both rules, the ET histogram and each kernel's record
// stores keep their text: they see another draw and a table with L more matches booked.
// The counting kernels (dclev::dc_leverage_count, dcpath::dc_paths_count, dcsc::dc_scenario_count,
// dcgq::dc_gpts_count) are unchanged and launched as they were, with nf = F + L.
// 24 kernels: 3 queries x {overall, head-to-head} x {redraw, extra time} x {ranked, table}, launched only when
// weights are in force or a match is in play; the 24 kick-off kernels read the flag through `if constexpr` only and
// compile to the code they were.  The state, the sides and the scores are per-lane values in vector registers, only
// the draw is wave uniform.  Integer atomics only, vector stores only, no LDS beyond the kick-off twins'.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_group_points.hip.h"      // dcgq::GptsArgs, dc_gpts_sim's text
#include "dc_paths.hip.h"             // dcpath::PathsArgs, dc_paths_sim's text
#include "dc_tournament_live.hip.h"   // dct::live_draw, play_live
#include "dc_tscen.hip.h"             // dcts::TscenArgs, dc_tscen_sim's text

namespace dctq {

using dcgq::GPTS_NO_REST;
using dcgq::GPTS_WAVES;
using dcgq::GptsArgs;
using dcpath::PATHS_WAVES;
using dcpath::PathsArgs;
using dcts::TSCEN_WAVES;
using dcts::TscenArgs;

#define DCT_SIM_LIVE 1
#define DCT_SIM_NAME cup_paths_live
#define DCT_SIM_ALLOC false
#include "dc_paths_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
#define DCT_SIM_NAME cup_paths_live_table
#define DCT_SIM_ALLOC true
#include "dc_paths_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC

#define DCT_SIM_NAME cup_scen_live
#define DCT_SIM_ALLOC false
#include "dc_tscen_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
#define DCT_SIM_NAME cup_scen_live_table
#define DCT_SIM_ALLOC true
#include "dc_tscen_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC

#define DCT_SIM_NAME cup_gpoints_live
#define DCT_SIM_ALLOC false
#include "dc_gpts_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
#define DCT_SIM_NAME cup_gpoints_live_table
#define DCT_SIM_ALLOC true
#include "dc_gpts_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
#undef DCT_SIM_LIVE

}  // namespace dctq
