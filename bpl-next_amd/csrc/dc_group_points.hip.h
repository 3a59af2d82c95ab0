// dc_group_points.hip.h -- group points against qualification targets (tournament_points,
// bpl/neutral_dixon_coles.py): how many points a team ends the group stage on, cross-tabulated against its knockout
// targets and its group place, the points of every group place, the gap between neighbouring places, and the points
// and goal difference of the teams placed advance + 1 ("the rest") against their rank across the groups, over the
// SAME simulations dc_tournament.hip.h, dc_paths.hip.h and dc_tscen.hip.h play.  Simulation j takes draw j mod S, the
// threefry blocks, the ranking, the bracket and the knockout rule of dc_tscen_sim, through the same device functions
// (dct::play, dck::decide, dch::pair_rank, dctab::*), so that under one key every scoreline, position and winner is
// theirs bit for bit (tests/test_gpu_tournament_points.py).  No [N, ...] array exists on the device: the simulations
// pass through a workspace of `chunk` records, two kernels per chunk, as in dc_points.hip.h.
//
// The axes: points bin v = points - points_min, 0 <= v < P <= GPTS_MAX_BINS = 256 (the host bounds the axis, so a bin
//   is a byte); goal-difference bin d = clip(GF - GA, -cap, cap) + cap, 0 <= d < D = 2 cap + 1 <= 17.  K = R + 2
//   targets: bit k < R "plays knockout round k", bit R "wins the tournament", bit R + 1 "first in its group" -- the
//   byte dc_tscen_sim forms.  Z = the largest group, B = the groups with a place advance + 1.
// Stage 1, dc_gpts_sim<H2H, ET>: ONE WAVE PER SIMULATION, dc_tscen_sim's group matches, ranking, bracket fill and
//   knockout rounds -- the recording kernels' shared text (dc_tournament_sim.hip.h) in its groups-only form -- with
//   empty callables: all it records it stores at the end.  The host launches it with groups only.  Record of
//   simulation c of the chunk (simulation j0 + c), every array a row over the chunk, one writer per cell:
//       slot[t * chunk + c]              u32  of slot t: v | place << 8 | d << 11 | target set << 16 | rest << 24,
//                                             rest = its rank among the rest (0 = best), GPTS_NO_REST when it is
//                                             not placed advance + 1
//       place[(g * Z + z) * chunk + c]   u8   v of the slot that finished place z of group g (the places of a group
//                                             are a permutation of its slots; a place a smaller group lacks is never
//                                             written nor read)
//       rank[k * chunk + c]              u16  v | d << 8 of the k-th best of the rest (best_of_rest > 0 only; the
//                                             ranks are a permutation of 0 .. B - 1)
//   -- 4 n + Gn Z + 2 B bytes per simulation (264 B for a 48-team World Cup).  With ET the [round][kind] histogram of
//   dc_knockout.hip.h is kept as in dc_tscen_sim.  Nothing else is counted here.
// Stage 2, dc_gpts_count: grid (row, share of the chunk), a thread per simulation, a u32 LDS histogram per workgroup,
//   flushed once per chunk with one global u64 atomic per non-zero cell.  The rows:
//       n slot rows            [P][1 + K + Z]: column 0 the points count, 1 + k "and inside target k", 1 + K + z "and
//                              place z" -- the largest row, 256 x 17 words = 17 KB of LDS
//       Gn Z place rows        [P]
//       Gn (Z - 1) gap rows    [P]: v of place z minus v of place z + 1 (>= 0: points order a group first in both
//                              tie-break modes); bin 0 = level on points
//     and with best_of_rest > 0
//       2 n pooled rest rows   [P][D], from the SLOT records, two per slot: the slot had a rest rank; it was ranked
//                              < best_of_rest.  All n of a kind flush into one table (a row per slot keeps every
//                              workgroup's share of the chunk the same: one pooled row walking all n slots took 48
//                              times as long as the other rows at the World Cup shape)
//       B rest-rank rows       [P][D], from the rank records
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
// On a live matchday (`in_play`, `log_weights`) stage 1 is dctq::cup_gpoints_live[_table]
//   (dc_tournament_live_queries.hip.h): this file's kernel text with LIVE set.  The matches in play are booked like
//   any fixture, and the host bounds the points axis with them among a slot's matches to come.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_tournament_sim.hip.h"   // dct::sim_enter, sim_play, sim_leave; dct::TournamentArgs and what it includes

namespace dcgq {

constexpr int GPTS_WAVES = dct::SIM_WAVES;
constexpr int GPTS_BLOCKS_PER_CU = 4;
constexpr int GPTS_MAX_BINS = 256;
constexpr int GPTS_MAX_GD_CAP = 8;
constexpr int GPTS_MAX_GROUPS = 16;
constexpr int GPTS_MAX_COLS = 1 + 8 + dct::TOURNAMENT_MAX_GROUP;   // a slot row's columns: 1 + K + Z, K <= 8
constexpr uint32_t GPTS_NO_REST = 0xFFu;
constexpr int COUNT_THREADS = 256;

struct GptsArgs {
    long long j0;                 // first simulation of the chunk
    int nc, chunk;                // simulations in this chunk, the workspace's chunk length
    int n, K, Z, Gn, B;           // slots, targets, the largest group, groups, groups with a place advance + 1
    int best;                     // best_of_rest
    int points_min, P;            // the points axis: bin v = points - points_min, 0 <= v < P
    int cap, D;                   // the goal-difference axis: bin d = clip(gd, -cap, cap) + cap, D = 2 cap + 1
    uint8_t gsize[GPTS_MAX_GROUPS];   // the groups' sizes
    uint32_t* slot;               // [n, chunk] slot records
    uint8_t* place;               // [Gn, Z, chunk] bins by group place
    uint16_t* rank;               // [B, chunk] bins by rest rank (best > 0)
    unsigned long long* team_points;    // [n, P]          (all zeroed by the caller)
    unsigned long long* team_target;    // [n, P, K]
    unsigned long long* team_place;     // [n, P, Z]
    unsigned long long* place_points;   // [Gn, Z, P]
    unsigned long long* place_gap;      // [Gn, Z - 1, P]
    unsigned long long* rest_count;     // [P, D]          (these three with best > 0)
    unsigned long long* rest_through;   // [P, D]
    unsigned long long* rest_rank;      // [B, P, D]
};

// A.n_sims, A.stage_counts, A.pos_counts, A.sim_stage and K.sim_decided are not read: P says which simulations.
// Launched with groups only (A.n_groups > 0); A.nf may be 0, the group stage is then the current table's.
#define DCT_SIM_NAME dc_gpts_sim
#define DCT_SIM_ALLOC false
#include "dc_gpts_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
// the same text under a best-of-rest allocation table (four more instantiations)
#define DCT_SIM_NAME points_alloc_sim
#define DCT_SIM_ALLOC true
#include "dc_gpts_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC

// grid (rows: n slots, Gn Z places, Gn (Z - 1) gaps; with best > 0 also 2 n pooled rest rows and B rest ranks; shares
// of the chunk).  Every cell index is checked against the row's cells before the LDS add.
__global__ __launch_bounds__(COUNT_THREADS) void dc_gpts_count(GptsArgs A) {
    __shared__ uint32_t hist[GPTS_MAX_BINS * GPTS_MAX_COLS];
    const int n = A.n, K = A.K, Z = A.Z, P = A.P, D = A.D, nc = A.nc;
    // the row's kind and its index there: slots, places, gaps, the pooled rest rows (2 per slot), rest ranks
    int r = (int)blockIdx.x, kind = 0;
    const int places = A.Gn * Z, gaps = A.Gn * (Z - 1);
    if (r >= n) {
        r -= n, kind = 1;
        if (r >= places) {
            r -= places, kind = 2;
            if (r >= gaps) {
                r -= gaps, kind = 3;
                if (r >= 2 * n) r -= 2 * n, kind = 4;
            }
        }
    }
    const int W = kind == 0 ? 1 + K + Z : (kind >= 3 ? D : 1), cells = P * W;
    // a place (or a gap's lower place) the group does not have: nothing to count
    if (kind == 1 && r % Z >= (int)A.gsize[r / Z]) return;
    if (kind == 2 && r % (Z - 1) + 1 >= (int)A.gsize[r / (Z - 1)]) return;
    if (kind == 4 && r >= A.B) return;   // (never: the grid has B rows of this kind)
    for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) hist[i] = 0u;
    __syncthreads();

    const int step = (int)gridDim.y * COUNT_THREADS;
    if (kind == 0) {
        const uint32_t* rec = A.slot + (size_t)r * A.chunk;
        for (int c = (int)blockIdx.y * COUNT_THREADS + (int)threadIdx.x; c < nc; c += step) {
            const uint32_t w = rec[c], v = w & 0xFFu, z = (w >> 8) & 7u, set = (w >> 16) & 0xFFu;
            if (v >= (uint32_t)P) continue;   // (never, by the host's bounds: keeps the cell inside `hist`)
            atomicAdd(&hist[v * W], 1u);
            for (int k = 0; k < K; ++k)
                if ((set >> k) & 1u) atomicAdd(&hist[v * W + 1 + k], 1u);
            if (z < (uint32_t)Z) atomicAdd(&hist[v * W + 1 + K + z], 1u);
        }
    } else if (kind == 1 || kind == 2) {
        // place row r = g Z + z; gap row r = g (Z - 1) + z between the places z and z + 1 of group g
        const int g = kind == 1 ? r / Z : r / (Z - 1), z = kind == 1 ? r % Z : r % (Z - 1);
        const uint8_t* a = A.place + ((size_t)g * Z + z) * A.chunk;
        const uint8_t* b = a + A.chunk;   // (read by the gap rows only: place z + 1 exists there)
        for (int c = (int)blockIdx.y * COUNT_THREADS + (int)threadIdx.x; c < nc; c += step) {
            uint32_t v = a[c];
            if (kind == 2) v -= b[c];
            if (v < (uint32_t)P) atomicAdd(&hist[v], 1u);
        }
    } else if (kind == 3) {
        // pooled over the slots, row r = 2 t + which: slot t had a rest rank (which = 0), one among the best `best` (1)
        const uint32_t below = (r & 1) == 0 ? GPTS_NO_REST : (uint32_t)A.best;
        const uint32_t* rec = A.slot + (size_t)(r >> 1) * A.chunk;
        for (int c = (int)blockIdx.y * COUNT_THREADS + (int)threadIdx.x; c < nc; c += step) {
            const uint32_t w = rec[c], v = w & 0xFFu, d = (w >> 11) & 31u;
            if ((w >> 24) < below && v < (uint32_t)P && d < (uint32_t)D) atomicAdd(&hist[v * D + d], 1u);
        }
    } else {
        const uint16_t* rec = A.rank + (size_t)r * A.chunk;
        for (int c = (int)blockIdx.y * COUNT_THREADS + (int)threadIdx.x; c < nc; c += step) {
            const uint32_t w = rec[c], v = w & 0xFFu, d = w >> 8;
            if (v < (uint32_t)P && d < (uint32_t)D) atomicAdd(&hist[v * D + d], 1u);
        }
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) {
        const uint32_t cnt = hist[i];
        if (!cnt) continue;
        unsigned long long* out;
        if (kind == 0) {
            const int bin = i / W, col = i - bin * W;
            if (col == 0) out = &A.team_points[(size_t)r * P + bin];
            else if (col <= K) out = &A.team_target[((size_t)r * P + bin) * K + col - 1];
            else out = &A.team_place[((size_t)r * P + bin) * Z + col - 1 - K];
        } else if (kind == 1) {
            out = &A.place_points[(size_t)r * P + i];
        } else if (kind == 2) {
            out = &A.place_gap[(size_t)r * P + i];
        } else if (kind == 3) {
            out = ((r & 1) == 0 ? A.rest_count : A.rest_through) + i;
        } else {
            out = &A.rest_rank[(size_t)r * P * D + i];
        }
        atomicAdd(out, (unsigned long long)cnt);
    }
}

}  // namespace dcgq
