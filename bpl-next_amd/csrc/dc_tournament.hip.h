// dc_tournament.hip.h -- a group-and-knockout tournament, simulated jointly over the posterior
// (simulate_tournament, bpl/neutral_dixon_coles.py): the venue-form neutral models' counterpart of
// dc_season.hip.h, whose sampler and wave helpers it reuses.
//
// Simulation j uses posterior draw s = j mod S for EVERY match it plays, in the groups and in the
// knockout rounds.  A match between slots p and q (listed order) is played at the host's venue when
// exactly one of them is a host: the host is the home side (swapped in when listed second) and
// on = 1; every other match keeps the listed order and is neutral, on = 0.  With h / a the model
// indices of the home / away side (venue-aware rate form of bplhip_predict_score_proba_venue):
//     eh = attack[s,h] - defence[s,a],  ea = attack[s,a] - defence[s,h]
//     on:    eh = eh + (home_attack[s,h] - away_defence[s,a]),  ea = ea + (away_attack[s,a] - home_defence[s,h])
//     confederations: dc = conf[s,c(h)] - conf[s,c(a)],  eh = eh + dc,  ea = ea - dc
//     lh = exp(eh), la = exp(ea), rho = corr_coef[s]
// and the scoreline is dcs::sample_scoreline's exact draw on u = (o + 0.5) 2^-32 from threefry-2x32-20
// blocks under the caller's key:
//     group fixture f                              block (j, f)
//     slot tie-break word                          o0 of block (j, 0x80000000 | slot)
//     knockout match k (over all rounds in order), attempt t < 32     block (j, 0x40000000 | k << 5 | t)
// Groups are ranked as dc_season's table (points, goal difference, goals for, tie-break word, all
// descending, then slot ascending), counting only the slots of the same group; the top `advance`
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

#include "dc_season.hip.h"   // dcs::sample_scoreline, unit_open, readlane_u64, wave_lds_order

namespace dct {

constexpr int TOURNAMENT_WAVES = 4;
constexpr int TOURNAMENT_BLOCKS_PER_CU = 4;
constexpr int TOURNAMENT_MAX_TEAMS = 64;
constexpr int TOURNAMENT_MAX_GROUP = 8;          // teams per group; also the group-position width
constexpr int TOURNAMENT_STAGES = 8;             // stage 0..R+1, R <= 6
constexpr int TOURNAMENT_CODES = 192;            // group g place p: 8 g + p - 1;  best k: 128 + k - 1
constexpr int TOURNAMENT_ATTEMPTS = 32;
constexpr uint32_t KNOCKOUT_COUNTER = 0x40000000u;

struct TournamentArgs {
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
    const size_t r = (size_t)s * A.T;
    double eh = A.attack[r + h] - A.defence[r + a];
    double ea = A.attack[r + a] - A.defence[r + h];
    if (hp != hq) {
        eh = eh + (A.home_attack[r + h] - A.away_defence[r + a]);
        ea = ea + (A.away_attack[r + a] - A.home_defence[r + h]);
    }
    if (A.C) {
        const double* cs = A.conf + (size_t)s * A.C;
        const double dc = cs[(ih >> 16) & 0xFFu] - cs[(ia >> 16) & 0xFFu];
        eh = eh + dc;
        ea = ea - dc;
    }
    const double lh = exp(eh), la = exp(ea), rho = A.corr[s];
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, j, ctr, &o0, &o1);
    dcs::sample_scoreline(lh, la, rho, dcs::unit_open(o0), dcs::unit_open(o1), x, y);
}

__global__ __launch_bounds__(64 * TOURNAMENT_WAVES) void dc_tournament(TournamentArgs A) {
    __shared__ uint32_t hist_stage[TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES];
    __shared__ uint32_t hist_pos[TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP];
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[TOURNAMENT_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[TOURNAMENT_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[TOURNAMENT_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = A.n, nf = A.nf, nb = 1 << A.rounds;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES; i += blockDim.x) hist_stage[i] = 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP; i += blockDim.x) hist_pos[i] = 0u;
    if (threadIdx.x < TOURNAMENT_MAX_TEAMS) sinfo[threadIdx.x] = threadIdx.x < n ? A.slot_info[threadIdx.x] : 0u;
    if (threadIdx.x < TOURNAMENT_CODES) code_pos[threadIdx.x] = A.n_groups ? A.code_pos[threadIdx.x] : (uint8_t)0xFF;
    __syncthreads();

    int32_t* tp = tab[wave][0];
    int32_t* tf = tab[wave][1];
    int32_t* ta = tab[wave][2];
    uint8_t* br = bracket[wave];
    uint8_t* stg = stage[wave];
    const bool slot_lane = lane < n;
    const bool groups = A.n_groups > 0;
    const int32_t p_init = slot_lane && groups ? A.init[lane] : 0;
    const int32_t f_init = slot_lane && groups ? A.init[n + lane] : 0;
    const int32_t a_init = slot_lane && groups ? A.init[2 * n + lane] : 0;
    const int my_group = slot_lane ? (int)(sinfo[lane] >> 25) : -1;
    const int first_slot = !groups && lane < nb ? (int)A.first_round[lane] : 0;
    const int advance = A.advance;   // (best_of_rest lives in code_pos: ranks beyond it map to no position)

    const long long waves = (long long)gridDim.x * TOURNAMENT_WAVES;
    for (long long j = (long long)blockIdx.x * TOURNAMENT_WAVES + wave; j < A.n_sims; j += waves) {
        const int s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        int my_stage = 1;
        if (groups) {
            // ---- group matches, lane = fixture
            if (slot_lane) {
                tp[lane] = p_init;
                tf[lane] = f_init;
                ta[lane] = a_init;
            }
            dcs::wave_lds_order();
            for (int f = lane; f < nf; f += 64) {
                const uint32_t sl = A.fix[f];
                int hs, as, x, y;
                play(A, sinfo, s, ju, (uint32_t)f, (int)(sl & 0xFFu), (int)(sl >> 8), &hs, &as, &x, &y);
                const int ph = x > y ? A.win : x == y ? A.draw : A.loss;
                const int pa = y > x ? A.win : x == y ? A.draw : A.loss;
                atomicAdd(&tp[hs], ph);
                atomicAdd(&tp[as], pa);
                atomicAdd(&tf[hs], x);
                atomicAdd(&tf[as], y);
                atomicAdd(&ta[hs], y);
                atomicAdd(&ta[as], x);
            }
            dcs::wave_lds_order();
            const int32_t pts = slot_lane ? tp[lane] : 0;
            const int32_t gf = slot_lane ? tf[lane] : 0;
            const int32_t ga = slot_lane ? ta[lane] : 0;
            dcs::wave_lds_order();   // (the next simulation's reset comes after these reads)
            // ---- ranking, lane = slot: dc_season's two packed keys
            uint32_t r0 = 0u, r1;
            if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcs::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
            const unsigned long long k1 = ((unsigned long long)(uint32_t)pts << 32) | (uint32_t)((gf - ga) ^ (int32_t)0x80000000);
            const unsigned long long k2 = ((unsigned long long)(uint32_t)gf << 32) | r0;
            int pos = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcs::readlane_u64(k1, k), o2k = dcs::readlane_u64(k2, k);
                const int gk = __builtin_amdgcn_readlane(my_group, k);
                const bool better = o1k > k1 || (o1k == k1 && (o2k > k2 || (o2k == k2 && k < lane)));
                pos += (gk == my_group && better) ? 1 : 0;
            }
            // best of the rest: the slots placed advance + 1, ranked across the groups
            const int rest = slot_lane && pos == advance ? 1 : 0;
            int rest_rank = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcs::readlane_u64(k1, k), o2k = dcs::readlane_u64(k2, k);
                const int rk = __builtin_amdgcn_readlane(rest, k);
                const bool better = o1k > k1 || (o1k == k1 && (o2k > k2 || (o2k == k2 && k < lane)));
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
        dcs::wave_lds_order();
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
            dcs::wave_lds_order();   // every lane has read its pair before entry m is overwritten
            if (lane < M) {
                br[lane] = (uint8_t)win;
                stg[win] = (uint8_t)(r + 2);
            }
            dcs::wave_lds_order();
            k0 += M;
        }
        if (slot_lane) {
            const int st = stg[lane];
            atomicAdd(&hist_stage[lane * TOURNAMENT_STAGES + st], 1u);
            if (A.sim_stage) A.sim_stage[(size_t)j * n + lane] = (uint8_t)st;
        }
        dcs::wave_lds_order();   // (the next simulation's bracket and stage writes come after these reads)
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
