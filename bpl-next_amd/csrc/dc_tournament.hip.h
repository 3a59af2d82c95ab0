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
//
// Layout: ONE WAVE PER SIMULATION, TOURNAMENT_WAVES per workgroup, grid-stride over the simulations.
//   groups    lane = fixture (f = lane, lane + 64, ...): rates from the float64 tables (L2-resident),
//             the sampler; points / GF / GA into the wave's LDS table with integer LDS atomics.
//   ranking   lane = slot: group position by counting the slots of the same group ahead over
//             wave-uniform readlanes, then the best-of-rest rank among the slots placed advance + 1.
//   bracket   each qualifier writes its slot into the wave's LDS bracket at its code's position.
//   knockout  round by round, lane = match: redraws while level, the winner's slot goes to entry m.
//   counts    per-workgroup u32 LDS histograms [slot][stage] and [slot][group position], flushed
//             once per workgroup with global u64 atomics.  Integer atomics only: bit-identical runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_posterior.hip.h"   // dcq::Posterior, log_rates_venue_branch
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dct {

constexpr int TOURNAMENT_WAVES = 4;
constexpr int TOURNAMENT_BLOCKS_PER_CU = 4;
constexpr int TOURNAMENT_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;
constexpr int TOURNAMENT_MAX_GROUP = 8;          // teams per group; also the group-position width
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

// H2H: the groups are ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  The best of the rest, slots of different groups
// with no match between them, keep the overall keys in both modes.
template <bool H2H>
__global__ __launch_bounds__(64 * TOURNAMENT_WAVES) void dc_tournament(TournamentArgs A, dch::PairArgs H) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist_stage[TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES];
    __shared__ uint32_t hist_pos[TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP];
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[TOURNAMENT_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[TOURNAMENT_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[TOURNAMENT_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : TOURNAMENT_WAVES;
    const int n = A.n, nf = A.nf, nb = 1 << A.rounds;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES; i += blockDim.x) hist_stage[i] = 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP; i += blockDim.x) hist_pos[i] = 0u;
    if constexpr (H2H) {
        // a two-wave workgroup's 128 threads do not cover the 192 codes
        for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS; i += blockDim.x) sinfo[i] = i < n ? A.slot_info[i] : 0u;
        for (int i = threadIdx.x; i < TOURNAMENT_CODES; i += blockDim.x)
            code_pos[i] = A.n_groups ? A.code_pos[i] : (uint8_t)0xFF;
    } else {
        if (threadIdx.x < TOURNAMENT_MAX_TEAMS) sinfo[threadIdx.x] = threadIdx.x < n ? A.slot_info[threadIdx.x] : 0u;
        if (threadIdx.x < TOURNAMENT_CODES) code_pos[threadIdx.x] = A.n_groups ? A.code_pos[threadIdx.x] : (uint8_t)0xFF;
    }
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;   // (not formed in the overall order: even unused it changed the compiled code)
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    uint8_t* br = bracket[wave];
    uint8_t* stg = stage[wave];
    const bool slot_lane = lane < n;
    const bool groups = A.n_groups > 0;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane && groups);
    const int my_group = slot_lane ? (int)(sinfo[lane] >> 25) : -1;
    const int first_slot = !groups && lane < nb ? (int)A.first_round[lane] : 0;
    const int advance = A.advance;   // (best_of_rest lives in code_pos: ranks beyond it map to no position)

    const long long waves = (long long)gridDim.x * nw;
    for (long long j = (long long)blockIdx.x * nw + wave; j < A.n_sims; j += waves) {
        const int s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        int my_stage = 1;
        if (groups) {
            // ---- group matches, lane = fixture
            dctab::store_row(table, lane, slot_lane, init);
            if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
            dcr::wave_lds_order();
            for (int f = lane; f < nf; f += 64) {
                const uint32_t sl = A.fix[f];
                int hs, as, x, y;
                play(A, sinfo, s, ju, (uint32_t)f, (int)(sl & 0xFFu), (int)(sl >> 8), &hs, &as, &x, &y);
                dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            }
            dcr::wave_lds_order();
            const dctab::Row row = dctab::load_row(table, TOURNAMENT_MAX_TEAMS, lane, slot_lane);
            // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
            if constexpr (!H2H) dcr::wave_lds_order();
            // ---- ranking, lane = slot: the group position, among the slots of the same group
            uint32_t r0 = 0u, r1;
            if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
            int pos = 0;
            if constexpr (H2H) {
                pos = dch::pair_rank<true>(pair, H.pitch, n, lane, slot_lane, row, r0, my_group);
                dcr::wave_lds_order();
            }
            const dctab::Keys K = dctab::rank_keys(row, r0);   // (after pair_rank: the place it compiles the same from)
            if constexpr (!H2H) {
                // (written out: in a helper the loop lost its scalar counter, dc_table.hip.h)
                for (int k = 0; k < n; ++k) {
                    const unsigned long long o1k = dcr::readlane_u64(K.k1, k), o2k = dcr::readlane_u64(K.k2, k);
                    const int gk = __builtin_amdgcn_readlane(my_group, k);
                    const bool better = o1k > K.k1 || (o1k == K.k1 && (o2k > K.k2 || (o2k == K.k2 && k < lane)));
                    pos += (gk == my_group && better) ? 1 : 0;
                }
            }
            // best of the rest: the slots placed advance + 1, ranked across the groups by the overall keys
            const int rest = slot_lane && pos == advance ? 1 : 0;
            int rest_rank = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(K.k1, k), o2k = dcr::readlane_u64(K.k2, k);
                const int rk = __builtin_amdgcn_readlane(rest, k);
                const bool better = o1k > K.k1 || (o1k == K.k1 && (o2k > K.k2 || (o2k == K.k2 && k < lane)));
                rest_rank += (rk && better) ? 1 : 0;
            }
            // ---- bracket resolution: a qualifier's code -> its first-round position
            int code = -1;
            if (slot_lane && pos < advance) code = TOURNAMENT_MAX_GROUP * my_group + pos;
            else if (rest) code = 128 + rest_rank;
            const int bpos = code >= 0 && code < TOURNAMENT_CODES ? (int)code_pos[code] : 0xFF;
            my_stage = bpos < nb ? 1 : 0;
            if (bpos < nb) br[bpos] = (uint8_t)lane;
            if (slot_lane) atomicAdd(&hist_pos[lane * TOURNAMENT_MAX_GROUP + pos], 1u);
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
            dcr::wave_lds_order();   // every lane has read its pair before entry m is overwritten
            if (lane < M) {
                br[lane] = (uint8_t)win;
                stg[win] = (uint8_t)(r + 2);
            }
            dcr::wave_lds_order();
            k0 += M;
        }
        if (slot_lane) {
            const int st = stg[lane];
            atomicAdd(&hist_stage[lane * TOURNAMENT_STAGES + st], 1u);
            if (A.sim_stage) A.sim_stage[(size_t)j * n + lane] = (uint8_t)st;
        }
        dcr::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    for (int i = threadIdx.x; i < n * TOURNAMENT_STAGES; i += blockDim.x) {
        const uint32_t v = hist_stage[i];
        if (v) atomicAdd(&A.stage_counts[i], (unsigned long long)v);
    }
    for (int i = threadIdx.x; i < n * TOURNAMENT_MAX_GROUP; i += blockDim.x) {
        const uint32_t v = hist_pos[i];
        if (v) atomicAdd(&A.pos_counts[i], (unsigned long long)v);
    }
}

}  // namespace dct
