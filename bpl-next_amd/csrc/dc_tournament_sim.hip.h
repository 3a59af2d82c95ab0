// dc_tournament_sim.hip.h -- what the recording tournament kernels share: dcpath::dc_paths_sim (dc_paths.hip.h),
// dcts::dc_tscen_sim (dc_tscen.hip.h) and dcgq::dc_gpts_sim (dc_group_points.hip.h), twelve instantiations.  They
// play the simulations of dc_tournament.hip.h, one wave per simulation, through the same device functions
// (dct::play, dck::decide, dch::pair_rank, dctab::*), and differ only in what they record of a simulation and where.
// The shared part is TEXT, included into each kernel's body after `using namespace dct;` with the flags H2H, ET,
// GROUPS_ONLY, ALLOC and LIVE and the arguments A, H, K, V in scope (ALLOC: the bracket is filled through a best-of-rest
// allocation table, dct::alloc_slot -- each kernel's text is included twice by its header, as the kernel it was with
// ALLOC false and as its *_alloc_sim twin with ALLOC true, twelve instantiations more.  LIVE: matches in play and
// weighted draws, the same text a third and fourth time as the 24 kernels of dc_tournament_live_queries.hip.h; every
// kernel of the three headers named above has LIVE false and a never-read V):
//   dc_tournament_sim_enter.hip.inc   the per-workgroup scaffold: the LDS arrays sinfo, code_pos, tab, bracket and
//                                     stage and their fill, the ET histogram zeroed, and the wave's constants (lane,
//                                     wave, nw, waves, n, nf, nb, table, pair, br, stg, slot_lane, groups, init,
//                                     my_group, first_slot, advance).  GROUPS_ONLY: the kernel is launched with groups
//                                     only, and neither tests A.n_groups nor has the knockout-only branch
//   dc_tournament_sim_play.hip.inc    one simulation by one wave, inside the kernel's loop over its chunk, with the
//                                     draw `s` and the simulation `ju` in scope.  Leaves the lane's pos, rest, rest_rank
//                                     and row and every slot's stage in stg[].  The kernel's recording is four
//                                     callables in scope:
//       on_fixture(f, p, hs, x, y)      a lane's played group fixture f: the first-listed slot p, the home slot hs and
//                                       the scoreline in the home orientation (a host listed second was swapped in);
//                                       returns the lane's u32 mark for on_block
//       on_block(b, mark)               every lane of the wave, after block b of 64 fixtures; mark = 0 on a lane
//                                       without a fixture
//       on_fixtures_done()              every lane of the wave, after the last block (with groups only)
//       on_match(k, p, q, win, how)     a lane's knockout match k (numbered over the rounds) of p against q; how = 0
//                                       under the redraw rule
//   dc_tournament_sim_leave.hip.inc   the ET histogram's flush
// A kernel keeps its argument record, its loop over the chunk, its callables and its record stores.
// Why text and not a function template: DESIGN.md, "The tournament family's shared paths" -- a force-inlined
// template with the same callables moved the code of nine kernels that are none of the twelve.
// The four dc_tournament / dc_tournament_et kernels do NOT come through here: they keep dc_tournament_body.hip.inc
// (why: see there).  A change of the rules is made in both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_tournament.hip.h"   // dct::TournamentArgs, play and what it includes

namespace dct {

constexpr int SIM_WAVES = 4;   // waves per workgroup in the overall order (H2H: blockDim.x / 64)
// the LIVE instantiations (dc_tournament_live_queries.hip.h) ask for four waves per SIMD, 128 VGPRs, as the dctl
// simulators do: the conditional sampler beside the knockout rules would otherwise cost a wave per SIMD
constexpr int LIVE_SIM_WAVES_PER_SIMD = 4;

}  // namespace dct
