// dc_leverage.hip.h -- which remaining fixtures decide the table (match_leverage, bpl/base.py): the
// cross-tabulation of every fixture's outcome against every team's finishing-position targets, over the
// SAME simulations dc_season.hip.h plays -- simulation j takes draw j mod S, the threefry blocks (j, f),
// the tie-break block and the ranking of dc_season, operation for operation, so that under one key the
// per-simulation scorelines and positions are dc_season's bit for bit (tests/test_gpu_leverage.py).
// Neither goes to the host, and no [N, F] array exists: the simulations pass through a workspace of
// `chunk` records, two kernels per chunk.
//
// Stage 1, dc_leverage_sim: ONE WAVE PER SIMULATION as in dc_season (lane = fixture for sampling, lane =
//   slot for ranking).  Per 64 fixtures the wave forms two ballots, home win and away win (a draw is
//   neither), and per slot one byte, the set of targets its position falls in (bit k: target_mask[k] has
//   the position's bit).  Record of simulation c of the chunk:
//       ball[(b * chunk + c) * 2 + {0, 1}]  u64, fixture block b (block-major: stage 2 reads one block)
//       tset[c * n + slot]                  u8
//   -- 16 B per 64 fixtures and n bytes, 116 B for 380 fixtures and 20 teams.  The target counts [n, K]
//   are booked here, through a per-workgroup LDS histogram flushed once with integer atomics.
// Stage 2, dc_leverage_count: the one-hot product joint[f, o, (t, k)] += sum_c A[c, (f, o)] B[c, (t, k)],
//   64 simulations per AND + popcount.  A workgroup owns a tile (fixture block b of 64, slot block of
//   COUNT_COLS / K slots with all their targets) over a share of the chunk's simulation groups:
//     transpose  wave w loads the ballots of 64 simulations (lane = simulation) and turns them by 64
//                ballots into lane = fixture words over the simulations (bit i = simulation i), through LDS
//                to all four waves;
//     count      for its columns (slot, k) the wave forms the wave-uniform word over the simulations by one
//                ballot of the slots' bytes, and lane = fixture adds popcount(H & word), popcount(A & word)
//                into its OWN u32 cell of the LDS tile (no atomics: a cell has one writer);
//     flush      once per chunk the tile goes into the global u64 table [F, 3, n, K], rows o = 0 (home
//                win) and o = 2 (away win), consecutive threads on consecutive columns.  The outcome
//                counts are the popcounts of H and A.
//   Row o = 1 (the draw) is what is left: joint[f, 1] = target - joint[f, 0] - joint[f, 2], taken on the
//   host from the integer tables.
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dclev {

constexpr int LEVERAGE_WAVES = 4;
constexpr int LEVERAGE_BLOCKS_PER_CU = 4;
constexpr int LEVERAGE_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;
constexpr int LEVERAGE_MAX_TARGETS = 8;
constexpr int COUNT_COLS = 64;                 // (slot, target) columns of a stage-2 tile
constexpr int COUNT_PITCH = 65;                // tile row pitch in words: the flush reads down a column

struct LeverageArgs {
    int S, T, n, nf, K;              // draws, model teams, table slots, fixtures, targets
    long long j0;                    // first simulation of the chunk
    int nc, chunk;                   // simulations in this chunk, the workspace's chunk length
    uint32_t key_hi, key_lo;
    int win, draw, loss;
    const double* attack;            // [S,T]
    const double* defence;           // [S,T]
    const double* home_adv;          // [S] (ha_stride = 0) or [S,T] (ha_stride = T)
    int ha_stride;
    const double* corr;              // [S]
    const uint32_t* fix;             // [nf]: home | away << 16 (model indices)
    const uint16_t* fix_slot;        // [nf]: home slot | away slot << 8
    const int32_t* init;             // [3, n]: points, GF, GA of the current table
    unsigned long long mask[LEVERAGE_MAX_TARGETS];   // bit p: position p is in target k
    unsigned long long* ball;        // [blocks, chunk, 2] ballots of the chunk (16-byte aligned)
    uint8_t* tset;                   // [chunk, n] target sets of the chunk
    unsigned long long* target;      // [n, K] (zeroed by the caller)
    unsigned long long* outcome;     // [nf, 3], columns 0 and 2 (zeroed by the caller)
    unsigned long long* joint;       // [nf, 3, n, K], rows 0 and 2 (zeroed by the caller)
    int slots_per_tile;              // COUNT_COLS / K
};

// H2H: the table is ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  The chunk's records are the same in both
// modes, and dc_leverage_count reads them as they are.
template <bool H2H>
__global__ __launch_bounds__(64 * LEVERAGE_WAVES) void dc_leverage_sim(LeverageArgs A, dch::PairArgs H) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist[LEVERAGE_MAX_TEAMS * LEVERAGE_MAX_TARGETS];
    __shared__ int32_t tab[LEVERAGE_WAVES][3][LEVERAGE_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : LEVERAGE_WAVES;
    const int n = A.n, nf = A.nf, K = A.K;
    for (int i = threadIdx.x; i < n * K; i += blockDim.x) hist[i] = 0u;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;   // (not formed in the overall order: even unused it changed the compiled code)
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);

    const int waves = (int)gridDim.x * nw;
    for (int c = (int)blockIdx.x * nw + wave; c < A.nc; c += waves) {
        const long long j = A.j0 + c;
        const int s = (int)(j % A.S);
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
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
                if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
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
        const dctab::Row row = dctab::load_row(table, LEVERAGE_MAX_TEAMS, lane, slot_lane);
        // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
        if constexpr (!H2H) dcr::wave_lds_order();
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int ahead = 0;
        if constexpr (H2H) {
            ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
            dcr::wave_lds_order();
        } else {
            // (written out: in a helper the loop lost its scalar counter, dc_table.hip.h)
            const dctab::Keys Q = dctab::rank_keys(row, r0);
            for (int k = 0; k < n; ++k) {
                const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
                ahead += (o1k > Q.k1 || (o1k == Q.k1 && (o2k > Q.k2 || (o2k == Q.k2 && k < lane)))) ? 1 : 0;
            }
        }
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

// lane = simulation holds `w`, bit f = fixture f; returns lane = fixture, bit i = simulation i
__device__ __forceinline__ unsigned long long transpose_bits(unsigned long long w, int lane) {
    unsigned long long out = 0ull;
#pragma unroll
    for (int f = 0; f < 64; ++f) {
        const unsigned long long m = __ballot((int)((w >> f) & 1ull));
        if (lane == f) out = m;
    }
    return out;
}

// grid (fixture blocks, slot tiles, shares of the chunk's simulation groups)
__global__ __launch_bounds__(64 * LEVERAGE_WAVES) void dc_leverage_count(LeverageArgs A) {
    __shared__ uint32_t tile[2][COUNT_COLS][COUNT_PITCH];             // [home | away][column][fixture]
    __shared__ unsigned long long turned[LEVERAGE_WAVES][2][64];       // [group of the round][home | away][fixture]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = A.n, K = A.K, nc = A.nc;
    const int b = (int)blockIdx.x, t0 = (int)blockIdx.y * A.slots_per_tile;
    const int slots = min(A.slots_per_tile, n - t0), cols = slots * K;
    const int groups = (nc + 63) >> 6;
    for (int i = threadIdx.x; i < 2 * COUNT_COLS * COUNT_PITCH; i += blockDim.x) (&tile[0][0][0])[i] = 0u;
    uint32_t home_n = 0u, away_n = 0u;   // wave 0 of the first slot tile: this fixture's outcome counts
    const bool count_outcomes = wave == 0 && blockIdx.y == 0;
    const ulonglong2* ball = reinterpret_cast<const ulonglong2*>(A.ball) + (size_t)b * A.chunk;
    __syncthreads();

    for (int g0 = (int)blockIdx.z * LEVERAGE_WAVES; g0 < groups; g0 += (int)gridDim.z * LEVERAGE_WAVES) {
        {   // transpose: this wave turns group g0 + wave
            const int c = (g0 + wave) * 64 + lane;
            ulonglong2 w = make_ulonglong2(0ull, 0ull);
            if (c < nc) w = ball[c];
            turned[wave][0][lane] = transpose_bits(w.x, lane);
            turned[wave][1][lane] = transpose_bits(w.y, lane);
        }
        __syncthreads();
        for (int q = 0; q < LEVERAGE_WAVES && g0 + q < groups; ++q) {
            const unsigned long long H = turned[q][0][lane], W = turned[q][1][lane];
            if (count_outcomes) {
                home_n += (uint32_t)__popcll(H);
                away_n += (uint32_t)__popcll(W);
            }
            const int c = (g0 + q) * 64 + lane;   // lane = simulation for the target bytes
            const uint8_t* sets = A.tset + (size_t)c * n + t0;
            for (int ti = wave; ti < slots; ti += LEVERAGE_WAVES) {
                const uint32_t set = c < nc ? sets[ti] : 0u;
                for (int k = 0; k < K; ++k) {
                    const unsigned long long in = __ballot((int)((set >> k) & 1u));
                    const int col = ti * K + k;
                    tile[0][col][lane] += (uint32_t)__popcll(H & in);
                    tile[1][col][lane] += (uint32_t)__popcll(W & in);
                }
            }
        }
        __syncthreads();   // (the next round overwrites `turned`)
    }

    // flush: consecutive threads on consecutive columns of one (fixture, outcome) row
    const size_t nK = (size_t)n * K;
    for (int i = threadIdx.x; i < 2 * 64 * cols; i += blockDim.x) {
        const int col = i % cols, r = i / cols, fl = r & 63, o = r >> 6;
        const int f = b * 64 + fl;
        const uint32_t v = tile[o][col][fl];
        if (f < A.nf && v) atomicAdd(&A.joint[((size_t)f * 3 + 2 * o) * nK + (size_t)t0 * K + col], (unsigned long long)v);
    }
    if (count_outcomes) {
        const int f = b * 64 + lane;
        if (f < A.nf) {
            if (home_n) atomicAdd(&A.outcome[(size_t)f * 3], (unsigned long long)home_n);
            if (away_n) atomicAdd(&A.outcome[(size_t)f * 3 + 2], (unsigned long long)away_n);
        }
    }
}

}  // namespace dclev
