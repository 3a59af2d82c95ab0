// dc_points.hip.h -- points totals against finishing targets (points_needed, bpl/base.py): how many points a
// team ends on, cross-tabulated against its finishing-position targets, the points of every finishing position
// and the gap between neighbouring positions, over the SAME simulations dc_season.hip.h plays -- simulation j
// takes draw j mod S, the threefry blocks (j, f), the tie-break block and the ranking of dc_season, operation
// for operation, so that under one key the per-simulation points and positions are dc_season's bit for bit
// (tests/test_gpu_points.py).  Neither goes to the host: the simulations pass through a workspace of `chunk`
// records, two kernels per chunk, as in dc_leverage.hip.h.
//
// Stage 1, dc_points_sim: ONE WAVE PER SIMULATION as in dc_season (lane = fixture for sampling, lane = slot
//   for ranking).  The loop is written out here: a step shared with dc_season or dc_leverage_sim changed their
//   compiled code (dc_season.hip.h).  Record of simulation c of the chunk, v = points - points_min (a u16: the
//   host bounds the axis at POINTS_MAX_BINS), all three arrays SLOT-MAJOR, a row over the chunk -- stage 2 reads one row
//   with consecutive threads on consecutive simulations, stage 1's n two-byte stores per simulation are the
//   scattered side:
//       slot_pts[slot * chunk + c]       u16  v of the slot
//       pos_pts[position * chunk + c]    u16  v of the slot that finished there (the positions are a
//                                             permutation: one writer per cell)
//       tset[slot * chunk + c]           u8   the set of targets its position falls in (bit k: mask[k] has the
//                                             position's bit), as dc_leverage_sim forms it
//   -- 5 n bytes per simulation.  Nothing is counted here.
// Stage 2, dc_points_count: grid (row, share of the chunk), a thread per simulation, a u32 LDS histogram per
//   workgroup, flushed once per chunk with one global u64 atomic per non-zero cell.  The rows:
//       n slot rows      [P][1 + K]: column 0 the points count, column 1 + k "and inside target k"
//       n position rows  [P]
//       n - 1 gap rows   [P]: v of position g minus v of position g + 1 (>= 0: points order the table first
//                        in both tie-break modes); bin 0 = level on points, decided by the tie-break
//   Points cluster in a few dozen bins, so many lanes of a wave hit one LDS word; the adds are plain integer LDS
//   atomics all the same.  (Tried and not kept: a wave-aggregated form, one leader per distinct cell of the wave
//   adding the popcount of a ballot of its equals -- 296 us against 35 us per call at the league shape,
//   DESIGN.md section 28.)
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dcpt {

constexpr int POINTS_WAVES = 4;
constexpr int POINTS_BLOCKS_PER_CU = 4;
constexpr int POINTS_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;
constexpr int POINTS_MAX_TARGETS = 8;
constexpr int POINTS_MAX_BINS = 1024;
constexpr int COUNT_THREADS = 256;

struct PointsArgs {
    int S, T, n, nf, K;              // draws, model teams, table slots, fixtures, targets
    long long j0;                    // first simulation of the chunk
    int nc, chunk;                   // simulations in this chunk, the workspace's chunk length
    uint32_t key_hi, key_lo;
    int win, draw, loss;
    int points_min, P;               // the points axis: bin v = points - points_min, 0 <= v < P
    const double* attack;            // [S,T]
    const double* defence;           // [S,T]
    const double* home_adv;          // [S] (ha_stride = 0) or [S,T] (ha_stride = T)
    int ha_stride;
    const double* corr;              // [S]
    const uint32_t* fix;             // [nf]: home | away << 16 (model indices)
    const uint16_t* fix_slot;        // [nf]: home slot | away slot << 8
    const int32_t* init;             // [3, n]: points, GF, GA of the current table
    unsigned long long mask[POINTS_MAX_TARGETS];   // bit p: position p is in target k
    uint16_t* slot_pts;              // [n, chunk] bins by slot
    uint16_t* pos_pts;               // [n, chunk] bins by finishing position
    uint8_t* tset;                   // [n, chunk] target sets by slot
    unsigned long long* team_points;       // [n, P] (zeroed by the caller)
    unsigned long long* team_target;       // [n, P, K] (zeroed by the caller)
    unsigned long long* position_points;   // [n, P] (zeroed by the caller)
    unsigned long long* gap;               // [n - 1, P] (zeroed by the caller)
};

// H2H: the table is ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  The chunk's records are the same in both
// modes, and dc_points_count reads them as they are.
template <bool H2H>
__global__ __launch_bounds__(64 * POINTS_WAVES) void dc_points_sim(PointsArgs A, dch::PairArgs H) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ int32_t tab[POINTS_WAVES][3][POINTS_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : POINTS_WAVES;
    const int n = A.n, nf = A.nf, K = A.K;

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
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
            if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
        }
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, POINTS_MAX_TEAMS, lane, slot_lane);
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
        // (ahead < n: the ranking is a permutation of the slots; the host has bounded the points axis)
        if (slot_lane && ahead < n) {
            uint32_t set = 0u;
            for (int k = 0; k < K; ++k) set |= ((uint32_t)(A.mask[k] >> ahead) & 1u) << k;
            const uint16_t v = (uint16_t)(row.pts - A.points_min);
            A.slot_pts[(size_t)lane * A.chunk + c] = v;
            A.pos_pts[(size_t)ahead * A.chunk + c] = v;
            A.tset[(size_t)lane * A.chunk + c] = (uint8_t)set;
        }
    }
}

// grid (rows: n slots, n positions, n - 1 gaps; shares of the chunk)
__global__ __launch_bounds__(COUNT_THREADS) void dc_points_count(PointsArgs A) {
    __shared__ uint32_t hist[POINTS_MAX_BINS * (1 + POINTS_MAX_TARGETS)];
    const int n = A.n, K = A.K, P = A.P, nc = A.nc;
    const int r = (int)blockIdx.x;
    const int kind = r < n ? 0 : (r < 2 * n ? 1 : 2), t = r - kind * n;   // slot t, position t, or gap t | t + 1
    const int W = kind == 0 ? 1 + K : 1, cells = P * W;
    for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) hist[i] = 0u;
    __syncthreads();

    const uint16_t* a = (kind == 0 ? A.slot_pts : A.pos_pts) + (size_t)t * A.chunk;
    const uint16_t* b = A.pos_pts + (size_t)(t + 1) * A.chunk;   // (read by the gap rows only: t + 1 < n there)
    const uint8_t* sets = A.tset + (size_t)t * A.chunk;
    const int step = (int)gridDim.y * COUNT_THREADS;
    for (int c0 = (int)blockIdx.y * COUNT_THREADS; c0 < nc; c0 += step) {
        const int c = c0 + (int)threadIdx.x;
        const bool live = c < nc;
        uint32_t v = live ? a[c] : 0u;
        if (kind == 2) v -= live ? b[c] : 0u;
        const bool on = live && v < (uint32_t)P;   // (always, by the host's bounds: keeps the cell inside `hist`)
        if (on) atomicAdd(&hist[v * W], 1u);
        if (kind == 0 && on) {
            const uint32_t set = sets[c];
            for (int k = 0; k < K; ++k)
                if ((set >> k) & 1u) atomicAdd(&hist[v * W + 1 + k], 1u);
        }
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) {
        const uint32_t cnt = hist[i];
        if (!cnt) continue;
        if (kind == 0) {
            const int bin = i / W, col = i - bin * W;
            if (col == 0) atomicAdd(&A.team_points[(size_t)t * P + bin], (unsigned long long)cnt);
            else atomicAdd(&A.team_target[((size_t)t * P + bin) * K + col - 1], (unsigned long long)cnt);
        } else if (kind == 1) {
            atomicAdd(&A.position_points[(size_t)t * P + i], (unsigned long long)cnt);
        } else {
            atomicAdd(&A.gap[(size_t)t * P + i], (unsigned long long)cnt);
        }
    }
}

}  // namespace dcpt
