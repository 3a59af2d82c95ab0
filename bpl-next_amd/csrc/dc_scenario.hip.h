// dc_scenario.hip.h -- the joint result of a few chosen fixtures against finishing targets (match_scenarios,
// bpl/base.py): every combination of the key fixtures' clipped margins cross-tabulated against every team's
// finishing-position targets, over the SAME simulations dc_season.hip.h plays -- simulation j takes draw j mod S, the
// threefry blocks (j, f), the tie-break block and the ranking of dc_season, operation for operation, so that under one
// key the per-simulation scorelines and positions are dc_season's bit for bit (tests/test_gpu_scenarios.py).  Neither
// goes to the host: the simulations pass through a workspace of `chunk` records, two kernels per chunk, as in
// dc_points.hip.h.
//
// The scenario index.  Key fixture q with cap c_q has C_q = 2 c_q + 1 classes, class = c_q - clip(x - y, -c_q, c_q)
//   (0 = home by c_q or more, 2 c_q = away by c_q or more), and a scenario is one class per key fixture, row-major in
//   the caller's order: m = sum_q class_q stride_q, stride_q = prod_{r > q} C_r, M = prod_q C_q <= SCENARIO_MAX_CELLS.
//   Every fixture carries one u16 code uploaded with the fixtures, stride | cap << CODE_CAP_SHIFT, 0 for a fixture
//   that is no key: the key fixtures may sit in any block of 64 and on any lane.
// Stage 1, dc_scenario_sim: ONE WAVE PER SIMULATION as in dc_season (lane = fixture for sampling, lane = slot for
//   ranking).  The loop is written out here: a step shared with dc_season or dc_leverage_sim changed their compiled
//   code (dc_season.hip.h).  A key lane keeps class x stride of its fixtures in a register over all blocks of the
//   list, and the wave adds the lanes once per simulation (an integer butterfly).  Record of simulation c of the chunk:
//       scen[c]                    u32  the scenario index
//       tset[slot * chunk + c]     u8   the set of targets the slot's position falls in (bit k: mask[k] has the
//                                       position's bit), as dc_leverage_sim forms it; SLOT-MAJOR as in dc_points
//   -- 4 + n bytes per simulation.  Nothing is counted here.
// Stage 2, dc_scenario_count: the table [M][W], W = 1 + n K (column 0 the scenario's count, column 1 + slot K + k
//   "and the slot inside target k"), is up to 6561 x 513 cells and does not fit one workgroup.  Grid (scenario tile,
//   share of the chunk): a workgroup owns COUNT_WORDS / W consecutive scenarios in a u32 LDS histogram, scans its
//   share of scen[] with a thread per simulation (consecutive threads on consecutive simulations), books the
//   simulations that fall inside its tile -- the scenario's cell and one cell per set target bit of every slot -- and
//   flushes the tile once per chunk with one global u64 atomic per non-zero cell.  A table that fits one tile has one
//   tile, and the shares carry the parallelism.  The slots' bytes are read eight rows at a time, independent loads,
//   and only their set bits are walked (the first form, one load after the other and a bit test per target, took
//   259.5 us per call at M = 6561 against 191.7 us: DESIGN.md section 34).
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dcsc {

constexpr int SCENARIO_WAVES = 4;
constexpr int SCENARIO_BLOCKS_PER_CU = 4;
constexpr int SCENARIO_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;
constexpr int SCENARIO_MAX_TARGETS = 8;
constexpr int SCENARIO_MAX_KEYS = 8;       // include/bplhip.h BPLHIP_SCENARIO_MAX_KEYS
constexpr int SCENARIO_MAX_CAP = 3;        // include/bplhip.h BPLHIP_SCENARIO_MAX_CAP
constexpr int SCENARIO_MAX_CELLS = 6561;   // include/bplhip.h BPLHIP_SCENARIO_MAX_CELLS = 3^8
constexpr int CODE_CAP_SHIFT = 12;         // a stride is at most SCENARIO_MAX_CELLS / 3 = 2187 < 2^12
constexpr int COUNT_THREADS = 256;
constexpr int COUNT_WORDS = 16384;         // the tile: 64 KB of u32 cells, at least 31 scenarios at W = 513
struct ScenarioArgs {
    int S, T, n, nf, K;              // draws, model teams, table slots, fixtures, targets
    long long j0;                    // first simulation of the chunk
    int nc, chunk;                   // simulations in this chunk, the workspace's chunk length
    uint32_t key_hi, key_lo;
    int win, draw, loss;
    int M, tile_rows;                // scenarios, scenarios of a stage-2 tile (tile_rows (1 + n K) <= COUNT_WORDS)
    const double* attack;            // [S,T]
    const double* defence;           // [S,T]
    const double* home_adv;          // [S] (ha_stride = 0) or [S,T] (ha_stride = T)
    int ha_stride;
    const double* corr;              // [S]
    const uint32_t* fix;             // [nf]: home | away << 16 (model indices)
    const uint16_t* fix_slot;        // [nf]: home slot | away slot << 8
    const uint16_t* fix_code;        // [nf]: stride | cap << CODE_CAP_SHIFT of a key fixture, 0 otherwise
    const int32_t* init;             // [3, n]: points, GF, GA of the current table
    unsigned long long mask[SCENARIO_MAX_TARGETS];   // bit p: position p is in target k
    uint32_t* scen;                  // [chunk] scenario indices
    uint8_t* tset;                   // [n, chunk] target sets by slot
    unsigned long long* scenario;    // [M] (zeroed by the caller)
    unsigned long long* joint;       // [M, n, K] (zeroed by the caller)
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// H2H: the table is ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  The chunk's records are the same in both
// modes, and dc_scenario_count reads them as they are.
template <bool H2H>
__global__ __launch_bounds__(64 * SCENARIO_WAVES) void dc_scenario_sim(ScenarioArgs A, dch::PairArgs H) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ int32_t tab[SCENARIO_WAVES][3][SCENARIO_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : SCENARIO_WAVES;
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
        uint32_t cell = 0u;   // class x stride of this lane's key fixtures, over all blocks of the list
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
            const uint32_t code = A.fix_code[f];
            const int cap = (int)(code >> CODE_CAP_SHIFT);   // (0 for a fixture that is no key: it adds nothing)
            cell += (uint32_t)(cap - min(max(x - y, -cap), cap)) * (code & ((1u << CODE_CAP_SHIFT) - 1u));
        }
        cell = wave_sum_u32(cell);
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, SCENARIO_MAX_TEAMS, lane, slot_lane);
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
        if (lane == 0) A.scen[c] = cell;
        // (ahead < n: the ranking is a permutation of the slots)
        if (slot_lane && ahead < n) {
            uint32_t set = 0u;
            for (int k = 0; k < K; ++k) set |= ((uint32_t)(A.mask[k] >> ahead) & 1u) << k;
            A.tset[(size_t)lane * A.chunk + c] = (uint8_t)set;
        }
    }
}

// grid (scenario tiles of A.tile_rows; shares of the chunk)
__global__ __launch_bounds__(COUNT_THREADS) void dc_scenario_count(ScenarioArgs A) {
    __shared__ uint32_t hist[COUNT_WORDS];
    const int n = A.n, K = A.K, nc = A.nc, W = 1 + n * K;
    const int m0 = (int)blockIdx.x * A.tile_rows;
    const int rows = min(A.tile_rows, A.M - m0), cells = rows * W;   // (cells <= COUNT_WORDS by the host's tile_rows)
    for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) hist[i] = 0u;
    __syncthreads();

    const int step = (int)gridDim.y * COUNT_THREADS;
    for (int c0 = (int)blockIdx.y * COUNT_THREADS; c0 < nc; c0 += step) {
        const int c = c0 + (int)threadIdx.x;
        if (c >= nc) continue;
        const uint32_t r = A.scen[c] - (uint32_t)m0;
        if (r >= (uint32_t)rows) continue;   // another tile's simulation (keeps the cell inside `hist`)
        uint32_t* cell = hist + r * W;
        atomicAdd(cell, 1u);
        ++cell;
        // eight slots at a time: their bytes are eight independent loads (one row each), and the walk is over the
        // set bits only -- a simulation has sum_k |target k| of them over all slots, whatever the table
        for (int t0 = 0; t0 < n; t0 += 8, cell += 8 * K) {
            unsigned long long sets = 0ull;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (t0 + u < n) sets |= (unsigned long long)A.tset[(size_t)(t0 + u) * A.chunk + c] << (8 * u);
            while (sets) {
                const int b = __ffsll((long long)sets) - 1;   // slot t0 + (b >> 3), target b & 7 < K
                sets &= sets - 1ull;
                atomicAdd(cell + (b >> 3) * K + (b & 7), 1u);
            }
        }
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    const size_t nK = (size_t)n * K;
    for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) {
        const uint32_t cnt = hist[i];
        if (!cnt) continue;
        const int r = i / W, col = i - r * W;
        if (col == 0) atomicAdd(&A.scenario[m0 + r], (unsigned long long)cnt);
        else atomicAdd(&A.joint[(size_t)(m0 + r) * nK + col - 1], (unsigned long long)cnt);
    }
}

}  // namespace dcsc
