// dc_h2h.hip.h -- head-to-head tie-breaks (tiebreak="head_to_head" of simulate_season, match_leverage and
// simulate_tournament): the per-pair record of one simulation and the ranking that uses it, then the
// head-to-head forms of dc_season, dc_leverage_sim and dc_tournament.  Under one key simulation j of a kernel
// here IS simulation j of its model kernel up to the ranking: the same draw j mod S, the same threefry blocks
// (j, f), scorelines, points and tie-break word (tests/test_gpu_h2h.py compares them bit for bit).
//
// The pair matrix: pair[i][k] = points i took from k << 16 | goals i scored against k, over every match
// between the two -- those already played (pair_init, from the host) and those of this simulation.  One u32
// per ordered pair, n rows of `pitch` = n | 1 words in DYNAMIC LDS, private to a wave.  The host bounds every
// half to 16 bits before any launch (played + remaining meetings x the largest value of a match), so the goals
// never carry into the points.
//   reset    lane = column: row by row from pair_init (zero without one), at the start of EVERY simulation;
//   booking  lane = fixture: one integer LDS atomic per side per match (a pair can meet twice in a simulation,
//            two lanes can share a cell);
//   ranking  lane = slot i walks the wave-uniform slots k: where k is level on points (and of the same group)
//            it adds pair[i][k]'s halves and pair[k][i]'s goals -- the mini-table over ALL slots level with
//            i, formed once.  pair[i][k] has lane stride = pitch, which is odd: the 64 lanes fall into
//            distinct banks (a pitch of 64 would put them all into one); pair[k][i] has lane stride 1.
// Order: points, head-to-head points, head-to-head goal difference, head-to-head goals, overall goal
// difference, overall goals for (all descending), the tie-break word descending, slot ascending.  Two slots
// compare on the head-to-head keys only when level on points, and then they share the mini-table, so the
// lexicographic compare is a total order.  The callers place dcr::wave_lds_order() between reset, booking and
// reading, as for the table rows.
//
// LDS: a wave's matrix is 4 n (n | 1) bytes -- 1680 B at n = 20, 9408 B at n = 48, 16 640 B at n = 64.  Up to
// H2H_SMALL_TEAMS slots a workgroup has four waves as the model kernels do, above it two, so that the dynamic
// part stays below 38 KB and a workgroup's total below 64 KB (DESIGN.md §21 has the occupancy).
// Integer atomics only, every add commutative: the outputs are bit-identical whatever the schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_leverage.hip.h"    // dclev::LeverageArgs
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order, readlane_u64
#include "dc_season.hip.h"      // dcs::SeasonArgs
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "dc_tournament.hip.h"  // dct::TournamentArgs, play
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dch {

constexpr int H2H_MAX_WAVES = 4;
constexpr int H2H_SMALL_TEAMS = 48;      // more slots than this: two waves per workgroup
constexpr int H2H_BLOCKS_PER_CU = 4;
constexpr uint32_t H2H_HALF = 0xFFFFu;   // a half of a pair record
constexpr int H2H_MAX_GOALS = 255;       // dcr::sample_scoreline's cap

struct PairArgs {
    const uint32_t* init;   // DEVICE u32 [n, n] or null (all zero); the diagonal is never read
    int pitch;              // n | 1
};

inline int waves_for(int n) { return n <= H2H_SMALL_TEAMS ? H2H_MAX_WAVES : 2; }
inline int pitch_for(int n) { return n | 1; }
inline size_t lds_bytes(int n) { return (size_t)waves_for(n) * n * pitch_for(n) * sizeof(uint32_t); }
// the largest dynamic part (n = H2H_SMALL_TEAMS with four waves, n = 64 with two) on top of the largest static
// part (dc_season_h2h: 20 KB) stays within the 64 KB every launch may ask for without an attribute
static_assert(H2H_MAX_WAVES * H2H_SMALL_TEAMS * (H2H_SMALL_TEAMS | 1) * 4 + 20 * 1024 <= 64 * 1024, "four-wave matrices");
static_assert(2 * dctab::TABLE_MAX_TEAMS * (dctab::TABLE_MAX_TEAMS | 1) * 4 + 20 * 1024 <= 64 * 1024, "two-wave matrices");

__device__ __forceinline__ void pair_reset(uint32_t* pair, const PairArgs& H, int n, int lane) {
    if (lane < n)
        for (int i = 0; i < n; ++i) pair[i * H.pitch + lane] = H.init ? H.init[i * n + lane] : 0u;
}
// a match hs v as that ended x : y
__device__ __forceinline__ void pair_book(uint32_t* pair, int pitch, int hs, int as, int x, int y, int win, int draw,
                                          int loss) {
    const uint32_t hp = (uint32_t)(x > y ? win : x == y ? draw : loss), ap = (uint32_t)(y > x ? win : x == y ? draw : loss);
    atomicAdd(&pair[hs * pitch + as], (hp << 16) | (uint32_t)x);
    atomicAdd(&pair[as * pitch + hs], (ap << 16) | (uint32_t)y);
}
// lane = slot: the number of slots ahead of it (GROUPED: of its group) under the eight keys
template <bool GROUPED>
__device__ __forceinline__ int pair_rank(const uint32_t* pair, int pitch, int n, int lane, bool slot_lane,
                                         const dctab::Row& row, uint32_t r0, int group) {
    int32_t hp = 0, hgf = 0, hga = 0;   // against the slots level on points
    for (int k = 0; k < n; ++k) {
        const int32_t pk = __builtin_amdgcn_readlane(row.pts, k);
        const int gk = GROUPED ? __builtin_amdgcn_readlane(group, k) : 0;
        if (slot_lane && k != lane && pk == row.pts && (!GROUPED || gk == group)) {
            const uint32_t w = pair[lane * pitch + k], v = pair[k * pitch + lane];
            hp += (int32_t)(w >> 16);
            hgf += (int32_t)(w & H2H_HALF);
            hga += (int32_t)(v & H2H_HALF);
        }
    }
    // (points, head-to-head points), (head-to-head GD + 2^31, head-to-head goals), (GD + 2^31, GF), word
    const unsigned long long k1 = ((unsigned long long)(uint32_t)row.pts << 32) | (uint32_t)hp;
    const unsigned long long k2 = ((unsigned long long)(uint32_t)((hgf - hga) ^ (int32_t)0x80000000) << 32) | (uint32_t)hgf;
    const unsigned long long k3 =
        ((unsigned long long)(uint32_t)((row.gf - row.ga) ^ (int32_t)0x80000000) << 32) | (uint32_t)row.gf;
    int ahead = 0;
    for (int k = 0; k < n; ++k) {
        const unsigned long long o1 = dcr::readlane_u64(k1, k), o2 = dcr::readlane_u64(k2, k), o3 = dcr::readlane_u64(k3, k);
        const uint32_t ok = (uint32_t)__builtin_amdgcn_readlane((int)r0, k);
        const int gk = GROUPED ? __builtin_amdgcn_readlane(group, k) : 0;
        const bool better =
            o1 > k1 ||
            (o1 == k1 && (o2 > k2 || (o2 == k2 && (o3 > k3 || (o3 == k3 && (ok > r0 || (ok == r0 && k < lane)))))));
        ahead += ((!GROUPED || gk == group) && better) ? 1 : 0;
    }
    return ahead;
}

// ---- dc_season with the head-to-head order (blockDim.x = 64 x dch::waves_for(n), dynamic LDS dch::lds_bytes(n))
__global__ __launch_bounds__(64 * H2H_MAX_WAVES) void dc_season_h2h(dcs::SeasonArgs A, PairArgs H) {
    extern __shared__ uint32_t pairs[];
    __shared__ uint32_t hist[dcs::SEASON_MAX_TEAMS * dcs::SEASON_MAX_TEAMS];
    __shared__ unsigned long long bsum[2][dcs::SEASON_MAX_TEAMS];
    __shared__ int32_t tab[H2H_MAX_WAVES][3][dcs::SEASON_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    const int n = A.n, nf = A.nf;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x < 2 * dcs::SEASON_MAX_TEAMS) (&bsum[0][0])[threadIdx.x] = 0ull;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    long long psum = 0, gdsum = 0;   // this lane's slot over the wave's simulations

    const long long waves = (long long)gridDim.x * nw;
    for (long long j = (long long)blockIdx.x * nw + wave; j < A.n_sims; j += waves) {
        const int s = (int)(j % A.S);
        dctab::store_row(table, lane, slot_lane, init);
        pair_reset(pair, H, n, lane);
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
            pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            if (A.home_goals) {
                A.home_goals[(size_t)j * nf + f] = (uint8_t)x;
                A.away_goals[(size_t)j * nf + f] = (uint8_t)y;
            }
        }
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, dcs::SEASON_MAX_TEAMS, lane, slot_lane);
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        const int ahead = pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
        dcr::wave_lds_order();   // (the next simulation's reset comes after these reads)
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

// ---- dc_leverage_sim with the head-to-head order: the chunk's records are dc_leverage_sim's, and
// dclev::dc_leverage_count reads them as it is
__global__ __launch_bounds__(64 * H2H_MAX_WAVES) void dc_leverage_sim_h2h(dclev::LeverageArgs A, PairArgs H) {
    extern __shared__ uint32_t pairs[];
    __shared__ uint32_t hist[dclev::LEVERAGE_MAX_TEAMS * dclev::LEVERAGE_MAX_TARGETS];
    __shared__ int32_t tab[H2H_MAX_WAVES][3][dclev::LEVERAGE_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    const int n = A.n, nf = A.nf, K = A.K;
    for (int i = threadIdx.x; i < n * K; i += blockDim.x) hist[i] = 0u;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);

    const int waves = (int)gridDim.x * nw;
    for (int c = (int)blockIdx.x * nw + wave; c < A.nc; c += waves) {
        const long long j = A.j0 + c;
        const int s = (int)(j % A.S);
        dctab::store_row(table, lane, slot_lane, init);
        pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
        const double* att = A.attack + (size_t)s * A.T;
        const double* dfn = A.defence + (size_t)s * A.T;
        const double* hadv = A.ha_stride ? A.home_adv + (size_t)s * A.T : A.home_adv + s;
        const double rho = A.corr[s];
        // (the trip count is the wave's, not the lane's: the ballots below take every lane)
        for (int base = 0, b = 0; base < nf; base += 64, ++b) {
            const int f = base + lane;
            bool home_win = false, away_win = false;
            if (f < nf) {
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
                pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                home_win = x > y;
                away_win = y > x;
            }
            const unsigned long long hb = __ballot(home_win), ab = __ballot(away_win);
            if (lane == 0) {
                unsigned long long* rec = A.ball + ((size_t)b * A.chunk + c) * 2;
                rec[0] = hb;
                rec[1] = ab;
            }
        }
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, dclev::LEVERAGE_MAX_TEAMS, lane, slot_lane);
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        const int ahead = pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
        dcr::wave_lds_order();   // (the next simulation's reset comes after these reads)
        if (slot_lane) {
            uint32_t set = 0u;
            for (int k = 0; k < K; ++k) {
                const uint32_t in = (uint32_t)(A.mask[k] >> ahead) & 1u;
                set |= in << k;
                if (in) atomicAdd(&hist[lane * K + k], 1u);
            }
            A.tset[(size_t)c * n + lane] = (uint8_t)set;
        }
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    for (int i = threadIdx.x; i < n * K; i += blockDim.x) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(&A.target[i], (unsigned long long)v);
    }
}

// ---- dc_tournament with the head-to-head order inside the groups; the best of the rest, slots of different
// groups with no match between them, keep dc_tournament's keys
__global__ __launch_bounds__(64 * H2H_MAX_WAVES) void dc_tournament_h2h(dct::TournamentArgs A, PairArgs H) {
    using namespace dct;
    extern __shared__ uint32_t pairs[];
    __shared__ uint32_t hist_stage[TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES];
    __shared__ uint32_t hist_pos[TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP];
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[H2H_MAX_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[H2H_MAX_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[H2H_MAX_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    const int n = A.n, nf = A.nf, nb = 1 << A.rounds;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_STAGES; i += blockDim.x) hist_stage[i] = 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS * TOURNAMENT_MAX_GROUP; i += blockDim.x) hist_pos[i] = 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_MAX_TEAMS; i += blockDim.x) sinfo[i] = i < n ? A.slot_info[i] : 0u;
    for (int i = threadIdx.x; i < TOURNAMENT_CODES; i += blockDim.x) code_pos[i] = A.n_groups ? A.code_pos[i] : (uint8_t)0xFF;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = pairs + (size_t)wave * n * H.pitch;
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
            pair_reset(pair, H, n, lane);
            dcr::wave_lds_order();
            for (int f = lane; f < nf; f += 64) {
                const uint32_t sl = A.fix[f];
                int hs, as, x, y;
                play(A, sinfo, s, ju, (uint32_t)f, (int)(sl & 0xFFu), (int)(sl >> 8), &hs, &as, &x, &y);
                dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            }
            dcr::wave_lds_order();
            const dctab::Row row = dctab::load_row(table, TOURNAMENT_MAX_TEAMS, lane, slot_lane);
            // ---- ranking, lane = slot: the group position under the head-to-head order
            uint32_t r0 = 0u, r1;
            if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, ju, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
            const int pos = pair_rank<true>(pair, H.pitch, n, lane, slot_lane, row, r0, my_group);
            dcr::wave_lds_order();   // (the next simulation's reset comes after these reads)
            // best of the rest: the slots placed advance + 1, ranked across the groups by the overall keys
            const dctab::Keys Q = dctab::rank_keys(row, r0);
            const int rest = slot_lane && pos == advance ? 1 : 0;
            int rest_rank = 0;
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
                const int rk = __builtin_amdgcn_readlane(rest, k);
                const bool better = o1k > Q.k1 || (o1k == Q.k1 && (o2k > Q.k2 || (o2k == Q.k2 && k < lane)));
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

}  // namespace dch
