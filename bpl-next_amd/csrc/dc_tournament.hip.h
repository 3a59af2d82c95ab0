// dc_tournament.hip.h -- a group-and-knockout tournament, simulated jointly over the posterior
// (simulate_tournament, bpl/neutral_dixon_coles.py): the venue-form neutral models' counterpart of
// dc_season.hip.h; the sampler, the rate form and the league table are the shared ones.
//
// Simulation j uses posterior draw s = j mod S for EVERY match it plays, in the groups and in the
// knockout rounds.  A match between slots p and q (listed order) is played at the host's venue when
// exactly one of them is a host: the host is the home side (swapped in when listed second) and
// on = 1; every other match keeps the listed order and is neutral, on = 0.  With h / a the model
// indices of the home / away side the log-rates are the venue BRANCH form of dc_posterior.hip.h,
// rho = corr_coef[s], and the scoreline is dcr::sample_scoreline's exact draw (dc_sampler.hip.h,
// which lists the counter space).  Groups are ranked by the shared league table (dc_table.hip.h),
// counting only the slots of the same group; the top `advance`
// qualify, and the teams placed advance + 1 are ranked across the groups by the same keys, the best
// `best_of_rest` of them qualifying as well.  The bracket's first round is resolved from the
// qualifiers' (group, place) or (best, rank) codes; knockout match m of a round pairs entries 2m and
// 2m + 1, its winner becomes entry m of the next round.  A knockout match redraws a level scoreline
// with the next attempt's block until one side wins (the winner is drawn from that posterior draw's
// scoreline distribution conditioned on a winner); after 32 level attempts (probability ~1e-17) the
// first-listed side goes through.  A slot's stage is 0 when it goes out in the groups, else 1 + the
// furthest knockout column it reached (column R = winning the final).  tests/tournament_ref.py
// restates all of this in numpy, operation for operation (contraction off, as in dc_season).
// With ET (knockout_rule="extra_time", the dc_tournament_et kernels) a knockout match is decided by
// dc_knockout.hip.h's ladder instead: one or two legs, away goals, extra time at scaled rates and a
// shoot-out, at most four blocks and no redraw.
//
// Layout: ONE WAVE PER SIMULATION, TOURNAMENT_WAVES per workgroup, grid-stride over the simulations.
//   groups    lane = fixture (f = lane, lane + 64, ...): rates from the float64 tables (L2-resident),
//             the sampler; points / GF / GA into the wave's LDS table with integer LDS atomics.
//   ranking   lane = slot: group position by counting the slots of the same group ahead over
//             wave-uniform readlanes, then the best-of-rest rank among the slots placed advance + 1.
//   bracket   each qualifier writes its slot into the wave's LDS bracket at its code's position.  Under a
//             best-of-rest allocation (ALLOC: the cup_alloc kernels, launched instead when a table is set) the code
//             of a qualifier placed advance + 1 is 128 + its allocation slot, read from the table row that the set
//             of those qualifiers' groups selects (alloc_slot), instead of 128 + its rank.
//   knockout  round by round, lane = match: redraws while level (ET: dck::decide), the winner's slot goes to
//             entry m; ET: how the match was decided into the workgroup's LDS histogram [round][kind] and,
//             when asked, into the simulation's row by the match's lane.
//   counts    per-workgroup u32 LDS histograms [slot][stage] and [slot][group position], flushed
//             once per workgroup with global u64 atomics.  Integer atomics only: bit-identical runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_knockout.hip.h"    // dck::KnockoutArgs, decide, decided_hist
#include "dc_posterior.hip.h"   // dcq::Posterior, log_rates_venue_branch
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dct {

constexpr int TOURNAMENT_WAVES = 4;
constexpr int TOURNAMENT_BLOCKS_PER_CU = 4;
constexpr int TOURNAMENT_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;
constexpr int TOURNAMENT_MAX_GROUP = 8;          // teams per group; also the group-position width
constexpr int TOURNAMENT_MAX_GROUPS = 16;        // groups; also the allocation tables' slot width
constexpr int TOURNAMENT_STAGES = 8;             // stage 0..R+1, R <= 6
constexpr int TOURNAMENT_CODES = 192;            // group g place p: 8 g + p - 1;  best k: 128 + k - 1
constexpr int TOURNAMENT_ATTEMPTS = 32;
constexpr uint32_t KNOCKOUT_COUNTER = 0x40000000u;

struct TournamentArgs {
    // (not an embedded dcq::Posterior: with it 1e3-tournament launches measured 1-4 % slower; play() builds the view)
    int S, T, C;                     // draws, model teams, confederations (0: none)
    int n, nf, n_groups;             // slots, group fixtures, groups (0: knockout only)
    int advance, rounds;             // qualifiers per group, knockout rounds R (bracket 2^R)
    long long n_sims;
    uint32_t key_hi, key_lo;
    int win, draw, loss;
    // the best-of-rest allocation (bplhip_tournament_set_allocation), in the dword that padded the pointers below:
    // no other member moved.  Read by the ALLOC kernels only (0 for every other launch): the byte offset from `fix`
    // of the allocation block (a multiple of 8): slot counts u64 [TOURNAMENT_MAX_GROUPS, TOURNAMENT_MAX_GROUPS]
    // (cup_alloc only; zeroed by the caller), row_of_mask u16
    // [1 << n_groups] (the table row of a mask of qualifying groups, 0 for any other), slots u8 [rows, n_groups] (the
    // 0-based slot of group g's team in that row, 0xFF none)
    uint32_t alloc_off;
    const double* attack;            // [S,T] each
    const double* defence;
    const double* home_attack;
    const double* away_attack;
    const double* home_defence;
    const double* away_defence;
    const double* conf;              // [S,C] or null
    const double* corr;              // [S]
    const uint32_t* slot_info;       // [n]: model index | conf << 16 | host << 24 | group << 25
    const uint16_t* fix;             // [nf]: slot p | slot q << 8 (listed order)
    const int32_t* init;             // [3, n]: points, GF, GA of the current table
    const uint8_t* code_pos;         // [TOURNAMENT_CODES]: bracket position of a qualifier code, 0xFF none
    const uint8_t* first_round;      // [2^R]: slots of the first round when n_groups = 0
    unsigned long long* stage_counts;   // [n, TOURNAMENT_STAGES] (zeroed by the caller)
    unsigned long long* pos_counts;     // [n, TOURNAMENT_MAX_GROUP] (zeroed by the caller)
    uint8_t* sim_stage;              // [n_sims, n] or null
};
static_assert(sizeof(TournamentArgs) == 192 && offsetof(TournamentArgs, alloc_off) == 60 &&
              offsetof(TournamentArgs, attack) == 64 && offsetof(TournamentArgs, loss) == 56,
              "alloc_off sits in the padding: no member moved, the argument blocks after the struct keep their place");
constexpr int ALLOC_COUNT_BYTES = TOURNAMENT_MAX_GROUPS * TOURNAMENT_MAX_GROUPS * 8;
__device__ __forceinline__ unsigned long long* alloc_counts(const TournamentArgs& A) {
    return reinterpret_cast<unsigned long long*>(const_cast<char*>(reinterpret_cast<const char*>(A.fix)) + A.alloc_off);
}

// The LDS of the ALLOC kernels alone, held the way dck::decided_hist() is (only the instantiations that call these
// hold them): a word per wave for the mask of qualifying groups, and cup_alloc's [group][slot] histogram.
__device__ __forceinline__ uint32_t* alloc_words() {
    __shared__ uint32_t words[TOURNAMENT_WAVES];
    return words;
}
__device__ __forceinline__ uint32_t* alloc_hist() {
    __shared__ uint32_t hist[TOURNAMENT_MAX_GROUPS * TOURNAMENT_MAX_GROUPS];
    return hist;
}
// The allocation slot of a lane's team, 0xFF when it has none.  `through`: the lane's slot is one of the best
// best_of_rest placed advance + 1, at most one lane per group, so an integer OR of 1 << group over those lanes is the
// mask of qualifying groups.  The OR goes through `word`, the wave's own word of alloc_words(), and the mask, the row
// and the slot stay in vector registers: these kernels have no scalar register to spare.
// Every lane of the wave calls it.
__device__ __forceinline__ int alloc_slot(const TournamentArgs& A, uint32_t* word, int lane, bool through, int my_group) {
    if (lane == 0) *word = 0u;
    dcr::wave_lds_order();
    if (through) atomicOr(word, 1u << (my_group & (TOURNAMENT_MAX_GROUPS - 1)));
    dcr::wave_lds_order();
    int slot = 0xFF;
    if (through) {
        const uint32_t mask = *word & ((1u << A.n_groups) - 1u);
        const uint16_t* rows = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(alloc_counts(A)) + ALLOC_COUNT_BYTES);
        const uint8_t* slots = reinterpret_cast<const uint8_t*>(rows + (1u << A.n_groups));
        slot = (int)slots[(int)rows[mask] * A.n_groups + my_group];
    }
    dcr::wave_lds_order();   // (the word is read before the next simulation zeroes it)
    return slot;
}

// one match of simulation j on draw s between slots p and q (listed order), venue decided by the
// host flags; returns the scoreline in the (home, away) orientation and the home / away slots
__device__ inline void play(const TournamentArgs& A, const uint32_t* sinfo, int s, uint32_t j, uint32_t ctr, int p,
                           int q, int* hs, int* as, int* x, int* y) {
#pragma clang fp contract(off)
    const uint32_t ip = sinfo[p], iq = sinfo[q];
    const bool hp = (ip >> 24) & 1u, hq = (iq >> 24) & 1u;
    const bool swap = hq && !hp;
    const uint32_t ih = swap ? iq : ip, ia = swap ? ip : iq;
    *hs = swap ? q : p;
    *as = swap ? p : q;
    const int h = (int)(ih & 0xFFFFu), a = (int)(ia & 0xFFFFu);
    double eh, ea;
    const dcq::Posterior<double> P{A.S, A.T, A.C, A.attack, A.defence, nullptr, 0, A.home_attack, A.away_attack,
                                   A.home_defence, A.away_defence, A.conf, A.corr};
    dcq::log_rates_venue_branch(P, s, h, a, hp != hq, &eh, &ea);
    if (P.C) dcq::add_confederations(P, s, (int)((ih >> 16) & 0xFFu), (int)((ia >> 16) & 0xFFu), &eh, &ea);
    const double lh = exp(eh), la = exp(ea), rho = P.corr[s];
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, j, ctr, &o0, &o1);
    dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), x, y);
}

// What the LIVE kernels (dc_tournament_live.hip.h: matches in play and weighted draws) take on
// top of the blocks above; the kernels of this file hold a never-read dummy of it, as the redraw kernels hold `K`.
// A.fix is then the concatenated list, the F fixtures still to kick off (A.nf = F) and after them the L in play.
struct LiveCup {
    int F, L;                   // the ordinary fixtures come first
    const uint32_t* st_goals;   // [L]: a | b << 8, the current score in the LISTED order
    const double* st_t;         // [L] elapsed fraction
    const double* C;            // [S] the scan of the weights, or null: simulation j takes draw j mod S
    int32_t* sim_draw;          // [n_sims] or null
    uint8_t* final_home;        // [n_sims, L] or null: the final scores in the listed order
    uint8_t* final_away;
};
// (defined in dc_tournament_live.hip.h; named by the discarded LIVE statements of the body)
__device__ inline int live_draw(const TournamentArgs& A, const LiveCup& V, long long j, int lane);
__device__ inline void play_live(const TournamentArgs& A, const LiveCup& V, const uint32_t* sinfo, int s, long long j,
                                 int m, int* hs, int* as, int* x, int* y);

// H2H: the groups are ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  The best of the rest, slots of different groups
// with no match between them, keep the overall keys in both modes.
// ET: level knockout matches go to extra time and a shoot-out (dc_knockout.hip.h); `K` is not read otherwise.

// The four kernels share one body, dc_tournament_body.hip.inc (why as text: see there).  The redraw rule keeps its
// kernels' names and arguments; the extra-time rule (ET) adds its own argument block.
template <bool H2H>
__global__ __launch_bounds__(64 * TOURNAMENT_WAVES) void dc_tournament(TournamentArgs A, dch::PairArgs H) {
    constexpr bool ET = false, ALLOC = false, LIVE = false;
    const LiveCup V{};   // (named by the discarded live statements; never read)
    const dck::KnockoutArgs K{};   // (named by the discarded extra-time statements; never read)
#include "dc_tournament_body.hip.inc"
}
template <bool H2H>
__global__ __launch_bounds__(64 * TOURNAMENT_WAVES) void dc_tournament_et(TournamentArgs A, dch::PairArgs H,
                                                                          dck::KnockoutArgs K) {
    constexpr bool ET = true, ALLOC = false, LIVE = false;
    const LiveCup V{};   // (named by the discarded live statements; never read)
#include "dc_tournament_body.hip.inc"
}
// ALLOC: the same body under a best-of-rest allocation table (A.alloc_off), launched instead of the two above when one
// is set.  Kernels of their own and not a runtime branch in the four above: those sit at the 106-SGPR ceiling, and a
// branch they never take still moved their spill code; this way their code is what it was.
template <bool H2H>
__global__ __launch_bounds__(64 * TOURNAMENT_WAVES) void cup_alloc(TournamentArgs A, dch::PairArgs H) {
    constexpr bool ET = false, ALLOC = true, LIVE = false;
    const LiveCup V{};   // (named by the discarded live statements; never read)
    const dck::KnockoutArgs K{};
#include "dc_tournament_body.hip.inc"
}
template <bool H2H>
__global__ __launch_bounds__(64 * TOURNAMENT_WAVES) void cup_alloc_et(TournamentArgs A, dch::PairArgs H, dck::KnockoutArgs K) {
    constexpr bool ET = true, ALLOC = true, LIVE = false;
    const LiveCup V{};   // (named by the discarded live statements; never read)
#include "dc_tournament_body.hip.inc"
}

}  // namespace dct
