// dc_paths.hip.h -- who meets whom in a tournament (tournament_paths, bpl/neutral_dixon_coles.py): the knockout
// pairings, the group places and the group fixtures' outcomes of the SAME simulations dc_tournament.hip.h plays,
// cross-tabulated on the device.  Simulation j takes draw j mod S, the threefry blocks, the ranking, the bracket and
// the knockout rule of dc_tournament / dc_tournament_et, through the same device functions (dct::play, dck::decide,
// dch::pair_rank, dctab::*), so that under one key every scoreline, position and winner is theirs bit for bit
// (tests/test_gpu_paths.py).  No [N, ...] array exists on the device: the simulations pass through a workspace of
// `chunk` records, as in dc_leverage.hip.h.
//
// Stage 1, dc_paths_sim<H2H, ET>: ONE WAVE PER SIMULATION, dc_tournament's simulation with its own loop (a chunk, not
//   a grid-stride over all simulations) and records in place of the histograms.  The scaffold and the play of a
//   simulation are the recording kernels' shared text (dc_tournament_sim.hip.h), not a flag in
//   dc_tournament_body.hip.inc, so the four tournament kernels are untouched; the ballots, the match words and the
//   slot bytes are this kernel's callables and stores.  Record of simulation c of the chunk (simulation j0 + c):
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
// On a live matchday (`in_play`, `log_weights`) stage 1 is dctq::cup_paths_live[_table]
//   (dc_tournament_live_queries.hip.h): this file's kernel text with LIVE set.  The ballot blocks then cover the
//   concatenated list, F fixtures to kick off and L matches in play, and stage 2 runs unchanged with nf = F + L.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_tournament_sim.hip.h"   // dct::sim_enter, sim_play, sim_leave; dct::TournamentArgs and what it includes

namespace dcpath {

constexpr int PATHS_WAVES = dct::SIM_WAVES;
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
#define DCT_SIM_NAME dc_paths_sim
#define DCT_SIM_ALLOC false
#include "dc_paths_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC
// the same text under a best-of-rest allocation table (four more instantiations)
#define DCT_SIM_NAME paths_alloc_sim
#define DCT_SIM_ALLOC true
#include "dc_paths_sim_kernel.hip.inc"
#undef DCT_SIM_NAME
#undef DCT_SIM_ALLOC

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
