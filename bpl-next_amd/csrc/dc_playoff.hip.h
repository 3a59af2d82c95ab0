// dc_playoff.hip.h -- play-offs after the league table (simulate_season(..., playoffs=...), bpl/base.py): one kernel
// that simulates the rest of a season, ranks the table and then plays ONE knockout bracket seeded by that ranking,
// all from the simulation's one posterior draw.  DESIGN.md section 24.
//
// League phase: dc_season's (dc_season.hip.h), statement for statement, through the same device functions -- the
// same draw j mod S, threefry blocks (j, f), scorelines, table, tie-break word and ranking (both orders), and the
// same position counts, sums and per-simulation outputs.  Under one key a call with play-offs IS the call without
// them as far as the league goes (tests/test_gpu_playoff.py compares every output bit for bit).
//
// Play-off phase.  Slots 0..n-1 are the table's rows, slots n..n+g-1 the guests (teams of the model that are not
// table rows, e.g. the club from the division below); n + g <= 64.  A slot's seed: its finishing position for a
// table row, n + i for guest i (worse than every table row); a winner carries its seed on.  The first round has
// 2^R entries, each a code: a finishing position (< n), PLAYOFF_GUEST | i, or PLAYOFF_BYE.  Entry 2m meets entry
// 2m + 1; a bye sends the other entry through without a match (it keeps its match number and draws nothing).
// In every tie q is the better-seeded side and p the worse-seeded one, and the rule is dc_knockout.hip.h's ladder
// on the same four threefry blocks (j, 0x40000000 | k << 5 | t), k numbered over all 2^R - 1 bracket matches:
//   one leg    t = 0: "seed" venue -- q at home WITH the home advantage; neutral venue (bit r of neutral_mask) --
//              p listed as the home side and the home-advantage term left out (eh = attack[h] - defence[a],
//              ea = attack[a] - defence[h]; the scalar and the per-team form alike).
//   two legs   t = 0 at p's ground, t = 1 at q's ground, both with the home advantage; aggregates and the optional
//              away-goals rule as in dc_knockout.hip.h (the mask is not read).
//   extra time t = 2: the venue of the only leg or of leg 2, both rates times `scale`.
//   shoot-out  t = 3: p is through iff unit_open(o0) < 1 / (1 + exp(-(strength[p] - strength[q]))).
// The leg and the ladder are written out here (team-level rate form, seed-driven orientation) rather than as a
// change to dck::play_leg / dck::decide, whose kernels keep their code; the constants are dck's.  All float64,
// contraction off; tests/playoff_ref.py restates it in numpy, operation for operation.
//
// Layout: dc_season's -- one wave per simulation, SEASON_WAVES per workgroup (H2H: dch::waves_for(n)).
//   ranking    lane = slot writes its slot into the wave's LDS row indexed by position (pos_slot) and its seed.
//   bracket    lane = entry resolves its code: position -> slot, guest -> n + i, or bye.
//   rounds     lane = match, behind dcr::wave_lds_order() fences as in dc_tournament_body.hip.inc.
//   counts     per-workgroup u32 LDS histograms [slot][stage] and [round][kind], flushed ONCE per workgroup with
//              global u64 integer atomics.  No float atomics: the outputs are bit-identical run to run.
// Static LDS: dc_season's 20 KB plus 3.4 KB (stage histogram 2 KB, four waves x four 64-byte rows, the slots'
// model indices, the bracket codes, the decision histogram).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_knockout.hip.h"    // dck::DECIDED_*, BLOCK_*, KNOCKOUT_MAX_ROUNDS
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_season.hip.h"      // dcs::SeasonArgs, SEASON_WAVES
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "dc_tournament.hip.h"  // dct::KNOCKOUT_COUNTER
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dcpo {

constexpr int PLAYOFF_MAX_SLOTS = dctab::TABLE_MAX_TEAMS;   // table rows plus guests
constexpr int PLAYOFF_STAGES = 8;                           // stage 0..R+1, R <= 6
constexpr uint16_t PLAYOFF_GUEST = 0x8000u;                 // code: PLAYOFF_GUEST | guest index
constexpr uint16_t PLAYOFF_BYE = 0xFFFFu;
constexpr int NO_SLOT = 0xFF;                               // a bye in the wave's bracket row
constexpr int DECIDED_BYE = 255;

struct PlayoffArgs {
    int g, rounds;                       // guests, rounds R (bracket 2^R)
    uint32_t legs_mask, neutral_mask;    // bit r: round r has two legs / a single leg of round r is neutral
    int away_goals;                      // 0 / 1
    double scale;                        // extra time: both rates times this, in (0, 1]
    const uint16_t* slot_model;          // [n + g] model index of every slot
    const uint16_t* bracket;             // [2^R] codes
    const double* strength;              // [n + g] shoot-out strength per slot
    unsigned long long* stage_counts;    // [n + g, PLAYOFF_STAGES] (zeroed by the caller)
    unsigned long long* decided_counts;  // [KNOCKOUT_MAX_ROUNDS, DECIDED_KINDS] (zeroed by the caller)
    uint8_t* sim_stage;                  // [n_sims, n + g] or null
    uint8_t* sim_decided;                // [n_sims, 2^R - 1] or null
};

// the largest dynamic part of a head-to-head launch on top of this kernel's static part stays within 64 KB
static_assert(dch::H2H_MAX_WAVES * dch::H2H_SMALL_TEAMS * (dch::H2H_SMALL_TEAMS | 1) * 4 + 24 * 1024 <= 64 * 1024, "four waves");
static_assert(2 * dctab::TABLE_MAX_TEAMS * (dctab::TABLE_MAX_TEAMS | 1) * 4 + 24 * 1024 <= 64 * 1024, "two waves");

// one leg of simulation j on draw s: model team h at home against a, with (on) or without the home advantage,
// both rates times c (1.0: exact) -- dc_season's rate form
__device__ inline void play_leg(const dcs::SeasonArgs& A, int s, uint32_t j, uint32_t ctr, int h, int a, bool on,
                                double c, int* x, int* y) {
#pragma clang fp contract(off)
    const double* att = A.attack + (size_t)s * A.T;
    const double* dfn = A.defence + (size_t)s * A.T;
    double eh = att[h] - dfn[a];
    if (on) eh = eh + (A.ha_stride ? A.home_adv[(size_t)s * A.T + h] : A.home_adv[s]);
    const double lh = exp(eh) * c, la = exp(att[a] - dfn[h]) * c;
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, j, ctr, &o0, &o1);
    dcr::sample_scoreline(lh, la, A.corr[s], dcr::unit_open(o0), dcr::unit_open(o1), x, y);
}

// the ladder of one tie between slot p (the worse seed) and slot q (the better seed); ctr = KNOCKOUT_COUNTER |
// k << 5.  Returns the slot that goes through and how it was decided.  One loop over the blocks 0, (1,) 2: one
// copy of the sampler.
__device__ inline int decide(const dcs::SeasonArgs& A, const PlayoffArgs& P, const uint16_t* model, int s, uint32_t j,
                             uint32_t ctr, int p, int q, bool two, bool neutral, int* how) {
#pragma clang fp contract(off)
    const int mp = model[p], mq = model[q];
    const bool on = two || !neutral;
    int gp = 0, gq = 0, y1 = 0;
    for (uint32_t t = 0; t <= dck::BLOCK_EXTRA_TIME; t = (t == 0 && !two) ? dck::BLOCK_EXTRA_TIME : t + 1) {
        const bool q_home = two ? t >= dck::BLOCK_LEG2 : !neutral;
        int x, y;
        play_leg(A, s, j, ctr | t, q_home ? mq : mp, q_home ? mp : mq, on, t == dck::BLOCK_EXTRA_TIME ? P.scale : 1.0,
                 &x, &y);
        gp += q_home ? y : x;
        gq += q_home ? x : y;
        if (two && t == 0) {
            y1 = y;   // q's away goals
            continue;
        }
        if (gp != gq) {
            *how = t == dck::BLOCK_EXTRA_TIME ? dck::DECIDED_EXTRA_TIME : dck::DECIDED_NORMAL;
            return gp > gq ? p : q;
        }
        // leg 2 has q at home: y is p's away goals
        if (t == dck::BLOCK_LEG2 && P.away_goals && y != y1) {
            *how = dck::DECIDED_AWAY_GOALS;
            return y > y1 ? p : q;
        }
    }
    uint32_t o0, o1;
    nd::tf_block(A.key_hi, A.key_lo, j, ctr | dck::BLOCK_SHOOTOUT, &o0, &o1);
    const double pr = 1.0 / (1.0 + exp(-(P.strength[p] - P.strength[q])));
    *how = dck::DECIDED_SHOOTOUT;
    return dcr::unit_open(o0) < pr ? p : q;
}

// H2H: the table is ordered by the head-to-head rule, launched as dc_season<true> is (blockDim.x = 64 x
// dch::waves_for(n), dch::lds_bytes(n) of dynamic LDS)
template <bool H2H>
__global__ __launch_bounds__(64 * dcs::SEASON_WAVES) void dc_playoff(dcs::SeasonArgs A, dch::PairArgs H, PlayoffArgs P) {
    using dcs::SEASON_MAX_TEAMS;
    using dcs::SEASON_WAVES;
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist[SEASON_MAX_TEAMS * SEASON_MAX_TEAMS];
    __shared__ unsigned long long bsum[2][SEASON_MAX_TEAMS];
    __shared__ int32_t tab[SEASON_WAVES][3][SEASON_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint32_t hist_stage[PLAYOFF_MAX_SLOTS * PLAYOFF_STAGES];
    __shared__ uint32_t hist_decided[dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS];
    __shared__ uint16_t model[PLAYOFF_MAX_SLOTS];                // model index of every slot
    __shared__ uint16_t bcode[PLAYOFF_MAX_SLOTS];                // the first round's codes
    // per wave, one block (one base register): the slot at each position, each slot's seed, the current round's
    // slots, each slot's stage
    __shared__ uint8_t rows[SEASON_WAVES][4][PLAYOFF_MAX_SLOTS];
    // (the wave index as a scalar: the wave's LDS rows then have scalar bases; with it, one block of rows and the
    // codes in LDS the kernels take 110 / 116 VGPRs, without them 130 / 138)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = H2H ? (int)(blockDim.x >> 6) : SEASON_WAVES;
    const int n = A.n, nf = A.nf, nt = A.n + P.g, nb = 1 << P.rounds;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x < 2 * SEASON_MAX_TEAMS) (&bsum[0][0])[threadIdx.x] = 0ull;
    for (int i = threadIdx.x; i < PLAYOFF_MAX_SLOTS * PLAYOFF_STAGES; i += blockDim.x) hist_stage[i] = 0u;
    if (threadIdx.x < dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS) hist_decided[threadIdx.x] = 0u;
    if (threadIdx.x < PLAYOFF_MAX_SLOTS) {
        model[threadIdx.x] = threadIdx.x < nt ? P.slot_model[threadIdx.x] : (uint16_t)0;
        bcode[threadIdx.x] = threadIdx.x < nb ? P.bracket[threadIdx.x] : PLAYOFF_BYE;
    }
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    uint8_t* ps = rows[wave][0];
    uint8_t* sd = rows[wave][1];
    uint8_t* br = rows[wave][2];
    uint8_t* stg = rows[wave][3];
    const bool slot_lane = lane < n, any_lane = lane < nt;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    long long psum = 0, gdsum = 0;   // this lane's slot over the wave's simulations
    // a guest's seed never changes (a table row's is written after every ranking)
    if (any_lane && !slot_lane) sd[lane] = (uint8_t)lane;

    const long long waves = (long long)gridDim.x * nw;
    for (long long j = (long long)blockIdx.x * nw + wave; j < A.n_sims; j += waves) {
        const int s = (int)(j % A.S);
        const uint32_t ju = (uint32_t)j;
        // ---- the league, lane = fixture (dc_season.hip.h)
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
            nd::tf_block(A.key_hi, A.key_lo, ju, (uint32_t)f, &o0, &o1);
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
        if constexpr (!H2H) dcr::wave_lds_order();
        // ---- ranking, lane = slot
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int ahead = 0;
        if constexpr (H2H) {
            ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
            dcr::wave_lds_order();
        } else {
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
            ps[ahead] = (uint8_t)lane;   // the positions are a permutation of 0..n-1: every cell is written
            sd[lane] = (uint8_t)ahead;
        }
        if (any_lane) stg[lane] = (uint8_t)0;
        dcr::wave_lds_order();
        // ---- bracket resolution, lane = entry
        if (lane < nb) {
            const int code = bcode[lane];
            const int slot = code == PLAYOFF_BYE ? NO_SLOT : (code & PLAYOFF_GUEST) ? n + (code & 0xFF) : (int)ps[code];
            br[lane] = (uint8_t)slot;
            if (slot != NO_SLOT) stg[slot] = (uint8_t)1;
        }
        dcr::wave_lds_order();
        // ---- rounds, lane = match
        int k0 = 0;
        for (int r = 0; r < P.rounds; ++r) {
            const int M = nb >> (r + 1);
            int win = NO_SLOT;
            if (lane < M) {
                const int e0 = br[2 * lane], e1 = br[2 * lane + 1];
                int how = DECIDED_BYE;
                if (e0 == NO_SLOT || e1 == NO_SLOT) {
                    win = e0 == NO_SLOT ? e1 : e0;
                } else {
                    const bool first_better = sd[e0] < sd[e1];
                    const int q = first_better ? e0 : e1, p = first_better ? e1 : e0;
                    const uint32_t ctr = dct::KNOCKOUT_COUNTER | ((uint32_t)(k0 + lane) << 5);
                    win = decide(A, P, model, s, ju, ctr, p, q, (P.legs_mask >> r) & 1u, (P.neutral_mask >> r) & 1u, &how);
                    atomicAdd(&hist_decided[r * dck::DECIDED_KINDS + how], 1u);
                }
                if (P.sim_decided) P.sim_decided[(size_t)j * (nb - 1) + k0 + lane] = (uint8_t)how;
            }
            dcr::wave_lds_order();   // every lane has read its pair before entry m is overwritten
            if (lane < M) {
                br[lane] = (uint8_t)win;
                if (win != NO_SLOT) stg[win] = (uint8_t)(r + 2);
            }
            dcr::wave_lds_order();
            k0 += M;
        }
        if (any_lane) {
            const int st = stg[lane];
            atomicAdd(&hist_stage[lane * PLAYOFF_STAGES + st], 1u);
            if (P.sim_stage) P.sim_stage[(size_t)j * nt + lane] = (uint8_t)st;
        }
        dcr::wave_lds_order();   // (the next simulation's rows are written after these reads)
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
    for (int i = threadIdx.x; i < nt * PLAYOFF_STAGES; i += blockDim.x) {
        const uint32_t v = hist_stage[i];
        if (v) atomicAdd(&P.stage_counts[i], (unsigned long long)v);
    }
    if (threadIdx.x < P.rounds * dck::DECIDED_KINDS) {
        const uint32_t v = hist_decided[threadIdx.x];
        if (v) atomicAdd(&P.decided_counts[threadIdx.x], (unsigned long long)v);
    }
}

}  // namespace dcpo
