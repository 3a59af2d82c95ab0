// dc_paths.hip.h -- who meets whom in a tournament (tournament_paths, bpl/neutral_dixon_coles.py): the knockout
// pairings, the group places and the group fixtures' outcomes of the SAME simulations dc_tournament.hip.h plays,
// cross-tabulated on the device.  Simulation j takes draw j mod S, the threefry blocks, the ranking, the bracket and
// the knockout rule of dc_tournament / dc_tournament_et, through the same device functions (dct::play, dck::decide,
// dch::pair_rank, dctab::*), so that under one key every scoreline, position and winner is theirs bit for bit
// (tests/test_gpu_paths.py).  No [N, ...] array exists on the device: the simulations pass through a workspace of
// `chunk` records, as in dc_leverage.hip.h.
//
// Stage 1, dc_paths_sim<H2H, ET>: ONE WAVE PER SIMULATION, dc_tournament's body with its own loop (a chunk, not a
//   grid-stride over all simulations) and records in place of the histograms -- a body of its own rather than a
//   flag in dc_tournament_body.hip.inc, so the four tournament kernels are untouched.  Record of simulation c of the
//   chunk (simulation j0 + c):
//       ball[(b * chunk + c) * 2 + {0, 1}]  u64, group-fixture block b: the first-listed / the second-listed side
//                                           wins (dc_leverage's layout, block-major; dct::play returns the home
//                                           orientation, which is turned back to the listed one here)
//       tset[c * n + slot]                  u8, bit k = stage >= k + 1: plays knockout column k (k = R: wins)
//       slot[c * n + slot]                  u8, stage | group position << 4 (position 0 without groups)
//       match[c * (2^R - 1) + k]            u32, knockout match k (numbered over the rounds):
//                                           first slot | second slot << 8 | winner << 16 | how decided << 24
//   -- 16 B per 64 group fixtures, 2 n bytes and 4 (2^R - 1) bytes: 316 B for a 48-team World Cup.  With ET the
//   [round][kind] histogram of dc_knockout.hip.h is kept as in dc_tournament_et.
// Stage 2: dclev::dc_leverage_count, unchanged, on the ballots and target bytes (K = R + 1 targets); and
//   dc_paths_count, grid (R + 1, shares of the chunk), a thread per simulation:
//     x < R   round x: every match of the round adds 1 to advance[winner][loser] in an LDS table [n][n] of u32;
//     x = R   every slot adds 1 to [slot][position][stage] in the same LDS table, [n][8][8];
//   LDS integer atomics, one flush per workgroup with global u64 atomics.  meet = advance + advance^T, the stage and
//   position counts and the target counts are sums of these tables, taken on the host from the integers.
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_tournament.hip.h"   // dct::TournamentArgs, play and what it includes

namespace dcpath {

constexpr int PATHS_WAVES = 4;
constexpr int PATHS_BLOCKS_PER_CU = 4;
constexpr int PATHS_COUNT_THREADS = 256;
constexpr int PATHS_CELLS = dct::TOURNAMENT_MAX_TEAMS * dct::TOURNAMENT_MAX_TEAMS;   // [n][n] and [n][8][8]
static_assert(dct::TOURNAMENT_MAX_GROUP * dct::TOURNAMENT_STAGES == dct::TOURNAMENT_MAX_TEAMS,
              "one LDS table serves both");

struct PathsArgs {
    long long j0;                    // first simulation of the chunk
    int nc, chunk;                   // simulations in this chunk, the workspace's chunk length
    unsigned long long* ball;        // [blocks, chunk, 2] ballots of the chunk (16-byte aligned)
    uint8_t* tset;                   // [chunk, n] target sets of the chunk
    uint8_t* slot;                   // [chunk, n] stage | position << 4
    uint32_t* match;                 // [chunk, 2^R - 1] knockout matches
    unsigned long long* advance;     // [R, n, n] (zeroed by the caller)
    unsigned long long* pos_stage;   // [n, TOURNAMENT_MAX_GROUP, TOURNAMENT_STAGES] (zeroed by the caller)
};

// A.n_sims, A.stage_counts, A.pos_counts, A.sim_stage and K.sim_decided are not read: P says which simulations
template <bool H2H, bool ET>
__global__ __launch_bounds__(64 * PATHS_WAVES) void dc_paths_sim(dct::TournamentArgs A, dch::PairArgs H,
                                                                 dck::KnockoutArgs K, PathsArgs P) {
    using namespace dct;
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t sinfo[TOURNAMENT_MAX_TEAMS];
    __shared__ uint8_t code_pos[TOURNAMENT_CODES];
    __shared__ int32_t tab[PATHS_WAVES][3][TOURNAMENT_MAX_TEAMS];   // per wave: points, GF, GA
    __shared__ uint8_t bracket[PATHS_WAVES][TOURNAMENT_MAX_TEAMS];  // per wave: the current round's slots
    __shared__ uint8_t stage[PATHS_WAVES][TOURNAMENT_MAX_TEAMS];    // per wave: each slot's stage
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = H2H ? (int)(blockDim.x >> 6) : PATHS_WAVES;
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
        if (groups) {
            // ---- group matches, lane = fixture (the trip count is the wave's: the ballots take every lane)
            dctab::store_row(table, lane, slot_lane, init);
            if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
            dcr::wave_lds_order();
            for (int base = 0, b = 0; base < nf; base += 64, ++b) {
                const int f = base + lane;
                bool first_wins = false, second_wins = false;
                if (f < nf) {
                    const uint32_t sl = A.fix[f];
                    const int p = (int)(sl & 0xFFu);
                    int hs, as, x, y;
                    play(A, sinfo, s, ju, (uint32_t)f, p, (int)(sl >> 8), &hs, &as, &x, &y);
                    dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                    if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                    // (x, y) is in the home orientation: a host listed second was swapped in
                    const bool listed = hs == p;
                    first_wins = listed ? x > y : y > x;
                    second_wins = listed ? y > x : x > y;
                }
                const unsigned long long fb = __ballot(first_wins), sb = __ballot(second_wins);
                if (lane == 0) {
                    unsigned long long* rec = P.ball + ((size_t)b * P.chunk + c) * 2;
                    rec[0] = fb;
                    rec[1] = sb;
                }
            }
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
        uint32_t* rec = P.match + (size_t)c * (nb - 1);
        int k0 = 0;
        for (int r = 0; r < A.rounds; ++r) {
            const int M = nb >> (r + 1);
            int win = 0;
            if (lane < M) {
                const int p = br[2 * lane], q = br[2 * lane + 1];
                const uint32_t ctr = KNOCKOUT_COUNTER | ((uint32_t)(k0 + lane) << 5);
                int how = 0;
                if constexpr (ET) {
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
                rec[k0 + lane] = (uint32_t)p | ((uint32_t)q << 8) | ((uint32_t)win << 16) | ((uint32_t)how << 24);
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
            const uint32_t st = stg[lane];
            P.slot[(size_t)c * n + lane] = (uint8_t)(st | ((uint32_t)pos << 4));
            P.tset[(size_t)c * n + lane] = (uint8_t)((1u << st) - 1u);
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

// grid (R + 1, shares of the chunk): see the head of the file
__global__ __launch_bounds__(PATHS_COUNT_THREADS) void dc_paths_count(PathsArgs P, int n, int rounds) {
    __shared__ uint32_t cell[PATHS_CELLS];
    for (int i = threadIdx.x; i < PATHS_CELLS; i += blockDim.x) cell[i] = 0u;
    __syncthreads();
    const int r = (int)blockIdx.x, nb = 1 << rounds, nm = nb - 1;
    const int stride = (int)(gridDim.y * blockDim.x);
    if (r < rounds) {
        const int M = nb >> (r + 1), k0 = nb - (nb >> r);   // the rounds before hold 2^R - 2^(R - r) matches
        for (int c = (int)(blockIdx.y * blockDim.x + threadIdx.x); c < P.nc; c += stride) {
            const uint32_t* rec = P.match + (size_t)c * nm + k0;
            for (int m = 0; m < M; ++m) {
                const uint32_t w = rec[m];
                const uint32_t p = w & 0xFFu, q = (w >> 8) & 0xFFu, win = (w >> 16) & 0xFFu;
                const uint32_t lose = win == p ? q : p;
                if (win < (uint32_t)n && lose < (uint32_t)n) atomicAdd(&cell[win * n + lose], 1u);
            }
        }
    } else {
        for (int c = (int)(blockIdx.y * blockDim.x + threadIdx.x); c < P.nc; c += stride) {
            const uint8_t* rec = P.slot + (size_t)c * n;
            for (int t = 0; t < n; ++t) {
                const uint32_t b = rec[t];
                const uint32_t place = (b >> 4) & 7u, st = b & 7u;
                atomicAdd(&cell[(t * dct::TOURNAMENT_MAX_GROUP + place) * dct::TOURNAMENT_STAGES + st], 1u);
            }
        }
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    unsigned long long* out = r < rounds ? P.advance + (size_t)r * n * n : P.pos_stage;
    const int cells = r < rounds ? n * n : n * dct::TOURNAMENT_MAX_GROUP * dct::TOURNAMENT_STAGES;
    for (int i = threadIdx.x; i < cells; i += blockDim.x) {
        const uint32_t v = cell[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
}

}  // namespace dcpath
