// dc_trajectory.hip.h -- the table after every remaining matchday (season_trajectory, bpl/base.py): positions,
// targets and points after each matchday, how long a team stays inside a target, from which matchday it is
// inside for good and how often the lead changes hands, over the SAME simulations dc_season.hip.h plays --
// simulation j takes draw j mod S, the threefry block (j, f) of fixture f under its ORIGINAL index whatever
// order it is visited in, the tie-break block and the ranking rule of dc_season, so that the table after the
// last matchday is dc_season's final table position for position (tests/test_gpu_trajectory.py).  Nothing per
// simulation goes to the host: the simulations pass through a workspace of `chunk` records, three kernels per
// chunk, as in dc_points.hip.h.
//
// The host sorts the fixtures by matchday (stable) and passes fix / fix_slot in that order, fix_id [nf] (the
// original index of the fixture now at f) and round_end [R] (matchday r is the fixtures round_end[r-1] <= f <
// round_end[r]; non-decreasing, the last one nf).
//
// Stage 1, dc_trajectory_sim: ONE WAVE PER SIMULATION as in dc_season.  The loop is written out here: a step
//   shared with dc_season, dc_leverage_sim or dc_points_sim changed their compiled code (dc_season.hip.h).  The
//   sorted fixtures are walked in windows of 64, lane = fixture: all 64 are sampled at once, then for every
//   matchday that ends inside the window (a wave-uniform walk over round_end) the matchday's lanes book, the
//   wave ranks (lane = slot) and emits; the lanes of a matchday that runs on into the next window book without
//   a ranking.  The tie-break words are formed once per simulation.  Under the head-to-head rule the pair matrix
//   is booked matchday by matchday too, so the mini-table is over the matches booked so far, `played` included.
//   Record of simulation c of the chunk, rows over the chunk (stage 2 reads one row with consecutive threads on
//   consecutive simulations; stage 1's stores are the scattered side):
//       pos[(r * n + slot) * chunk + c]     u8   the slot's position after matchday r
//       pts[(r * n + slot) * chunk + c]     u16  v = its points - points_min (the host bounds the axis)
//       leader[r * chunk + c]               u8   the slot with nobody ahead
//   -- 3 n R + R bytes per simulation.  Nothing is counted here.
// Stage 2, a thread per simulation, u32 LDS histograms, one global u64 atomic per non-zero cell:
//   dc_trajectory_count  grid (R n rows: matchday, slot; shares of the chunk): position_count, target_count,
//       target_final_count (with the same slot's row of the LAST matchday) and the sums of v and v^2.  The
//       target sets are formed from the position and the masks, as dc_points_sim forms them; the cell of a
//       target is fixed per workgroup, so a wave adds the popcount of a ballot, not a lane at a time.
//   dc_trajectory_paths  grid (n + 1 rows; shares of the chunk): a thread walks its simulation's R positions of
//       the slot and bins, per target, the number of matchdays inside and the first matchday from which it
//       stays inside (R: outside at the end); row n walks `leader` and bins the number of changes.
// Integers only, every add commutative: the tables are bit-identical for any grid, chunk and schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dctr {

constexpr int TRAJECTORY_WAVES = 4;
constexpr int TRAJECTORY_BLOCKS_PER_CU = 4;
constexpr int TRAJECTORY_MAX_TEAMS = dctab::TABLE_MAX_TEAMS;
constexpr int TRAJECTORY_MAX_TARGETS = 8;
constexpr int TRAJECTORY_MAX_ROUNDS = 256;
constexpr int COUNT_THREADS = 256;

struct TrajectoryArgs {
    int S, T, n, nf, K, R;           // draws, model teams, table slots, fixtures, targets, matchdays
    long long j0;                    // first simulation of the chunk
    int nc, chunk;                   // simulations in this chunk, the workspace's chunk length
    uint32_t key_hi, key_lo;
    int win, draw, loss;
    int points_min;                  // v = points - points_min
    const double* attack;            // [S,T]
    const double* defence;           // [S,T]
    const double* home_adv;          // [S] (ha_stride = 0) or [S,T] (ha_stride = T)
    int ha_stride;
    const double* corr;              // [S]
    const uint32_t* fix;             // [nf]: home | away << 16 (model indices), sorted by matchday
    const uint16_t* fix_slot;        // [nf]: home slot | away slot << 8, in the same order
    const uint16_t* fix_id;          // [nf]: the fixture's original index (its threefry counter)
    const int32_t* round_end;        // [R]: one past matchday r's last fixture
    const int32_t* init;             // [3, n]: points, GF, GA of the current table
    unsigned long long mask[TRAJECTORY_MAX_TARGETS];   // bit p: position p is in target k
    uint8_t* pos;                    // [R, n, chunk] positions by matchday and slot
    uint16_t* pts;                   // [R, n, chunk] v by matchday and slot
    uint8_t* leader;                 // [R, chunk] the leading slot
    unsigned long long* position_count;       // [R, n, n]        (all zeroed by the caller)
    unsigned long long* target_count;         // [R, n, K]
    unsigned long long* target_final_count;   // [R, n, K]
    unsigned long long* points_sum;           // [2, R, n]: sums of v, then of v^2
    unsigned long long* rounds_inside;        // [n, K, R + 1]
    unsigned long long* secured;              // [n, K, R + 1]
    unsigned long long* lead_changes;         // [R]
};

// H2H: the tables are ordered by the head-to-head rule (dc_h2h.hip.h) -- blockDim.x = 64 x dch::waves_for(n) and
// dch::lds_bytes(n) of dynamic LDS; `H` is not read otherwise.  The chunk's records are the same in both modes.
template <bool H2H>
__global__ __launch_bounds__(64 * TRAJECTORY_WAVES) void dc_trajectory_sim(TrajectoryArgs A, dch::PairArgs H) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ int32_t tab[TRAJECTORY_WAVES][3][TRAJECTORY_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // waves per workgroup: the head-to-head launch has two above dch::H2H_SMALL_TEAMS slots, so it asks
    const int nw = H2H ? (int)(blockDim.x >> 6) : TRAJECTORY_WAVES;
    const int n = A.n, nf = A.nf, R = A.R;

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
        // one word per slot for every matchday of the simulation
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int r = 0;   // the next matchday to rank (wave-uniform)
        // (`r < R` past the fixtures: a call without fixtures still ranks its matchdays, all empty)
        for (int w0 = 0; w0 < nf || r < R; w0 += 64) {
            const int f = w0 + lane, wend = min(w0 + 64, nf);
            const bool live = f < nf;
            int hs = 0, as = 0, x = 0, y = 0;
            if (live) {
                const uint32_t hw = A.fix[f];
                const int h = (int)(hw & 0xFFFFu), a = (int)(hw >> 16);
                const uint32_t sl = A.fix_slot[f];
                hs = (int)(sl & 0xFFu), as = (int)(sl >> 8);
                double eh = att[h] - dfn[a];
                eh = eh + (A.ha_stride ? hadv[h] : hadv[0]);
                const double lh = exp(eh), la = exp(att[a] - dfn[h]);
                uint32_t o0, o1;
                nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, (uint32_t)A.fix_id[f], &o0, &o1);
                dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            }
            int lo = w0;   // the first fixture of the window not booked yet
            while (r < R) {
                const int e = A.round_end[r];
                if (e > wend) break;
                if (live && f >= lo && f < e) {
                    dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                    if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                }
                lo = max(lo, e);
                dcr::wave_lds_order();
                const dctab::Row row = dctab::load_row(table, TRAJECTORY_MAX_TEAMS, lane, slot_lane);
                int ahead = 0;
                if constexpr (H2H) {
                    ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
                } else {
                    // (written out: in a helper the loop lost its scalar counter, dc_table.hip.h.  dc_season's
                    // predicate with | and & for || and &&: this loop runs R times a simulation, and the short-circuit
                    // form compiles to two nested exec-mask branches per step)
                    const dctab::Keys Q = dctab::rank_keys(row, r0);
                    for (int k = 0; k < n; ++k) {
                        const unsigned long long o1k = dcr::readlane_u64(Q.k1, k), o2k = dcr::readlane_u64(Q.k2, k);
                        const bool tie = (o2k > Q.k2) | ((o2k == Q.k2) & (k < lane));
                        ahead += (int)((o1k > Q.k1) | ((o1k == Q.k1) & tie));
                    }
                }
                // the next matchday's booking, or the next simulation's reset, comes after these reads
                dcr::wave_lds_order();
                // (ahead < n: the ranking is a permutation of the slots; the host has bounded the points axis)
                if (slot_lane && ahead < n) {
                    const size_t at = ((size_t)r * n + lane) * A.chunk + c;
                    A.pos[at] = (uint8_t)ahead;
                    A.pts[at] = (uint16_t)(row.pts - A.points_min);
                    if (ahead == 0) A.leader[(size_t)r * A.chunk + c] = (uint8_t)lane;
                }
                ++r;
            }
            // a matchday that runs on into the next window: booked now, ranked when it ends
            if (live && f >= lo) {
                dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            }
        }
        dcr::wave_lds_order();
    }
}

// grid (rows: matchday r, slot t as r n + t; shares of the chunk)
__global__ __launch_bounds__(COUNT_THREADS) void dc_trajectory_count(TrajectoryArgs A) {
    __shared__ uint32_t hist[TRAJECTORY_MAX_TEAMS];                 // positions of the slot after the matchday
    __shared__ uint32_t inside[2][TRAJECTORY_MAX_TARGETS];          // inside target k; and inside it at the end
    __shared__ unsigned long long vsum[2];                          // sums of v and v^2
    const int n = A.n, K = A.K, nc = A.nc;
    const int row = (int)blockIdx.x, r = row / n, t = row - r * n;
    if (threadIdx.x < TRAJECTORY_MAX_TEAMS) hist[threadIdx.x] = 0u;
    if (threadIdx.x < 2 * TRAJECTORY_MAX_TARGETS) (&inside[0][0])[threadIdx.x] = 0u;
    if (threadIdx.x < 2) vsum[threadIdx.x] = 0ull;
    __syncthreads();

    const uint8_t* now = A.pos + (size_t)row * A.chunk;
    const uint8_t* last = A.pos + ((size_t)(A.R - 1) * n + t) * A.chunk;
    const uint16_t* val = A.pts + (size_t)row * A.chunk;
    unsigned long long s1 = 0ull, s2 = 0ull;
    const int step = (int)gridDim.y * COUNT_THREADS;
    // (the trip count is the workgroup's, not the thread's: the ballots below take every lane)
    for (int c0 = (int)blockIdx.y * COUNT_THREADS; c0 < nc; c0 += step) {
        const int c = c0 + (int)threadIdx.x;
        const bool live = c < nc;
        const uint32_t p = live ? now[c] : 0u, pf = live ? last[c] : 0u;
        const unsigned long long v = live ? val[c] : 0u;
        if (live && p < (uint32_t)n) atomicAdd(&hist[p], 1u);   // (always p < n: keeps the cell inside `hist`)
        s1 += v;
        s2 += v * v;
        for (int k = 0; k < K; ++k) {
            const bool in = live && ((A.mask[k] >> p) & 1ull);
            const unsigned long long b = __ballot((int)in), bf = __ballot((int)(in && ((A.mask[k] >> pf) & 1ull)));
            if ((threadIdx.x & 63) == 0) {
                if (b) atomicAdd(&inside[0][k], (uint32_t)__popcll(b));
                if (bf) atomicAdd(&inside[1][k], (uint32_t)__popcll(bf));
            }
        }
    }
    if (s1) atomicAdd(&vsum[0], s1);
    if (s2) atomicAdd(&vsum[1], s2);
    __syncthreads();
    // one global atomic per touched cell per workgroup
    if ((int)threadIdx.x < n) {
        const uint32_t cnt = hist[threadIdx.x];
        if (cnt) atomicAdd(&A.position_count[(size_t)row * n + threadIdx.x], (unsigned long long)cnt);
    }
    if ((int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + K) {
        const int k = (int)threadIdx.x - 64;
        const uint32_t a = inside[0][k], b = inside[1][k];
        if (a) atomicAdd(&A.target_count[(size_t)row * K + k], (unsigned long long)a);
        if (b) atomicAdd(&A.target_final_count[(size_t)row * K + k], (unsigned long long)b);
    }
    if (threadIdx.x >= 128 && threadIdx.x < 130) {
        const int w = (int)threadIdx.x - 128;
        const unsigned long long sum = vsum[w];
        if (sum) atomicAdd(&A.points_sum[((size_t)w * A.R + r) * n + t], sum);
    }
}

// grid (rows: n slots, then the leader's row; shares of the chunk)
__global__ __launch_bounds__(COUNT_THREADS) void dc_trajectory_paths(TrajectoryArgs A) {
    __shared__ uint32_t hist[2][TRAJECTORY_MAX_TARGETS][TRAJECTORY_MAX_ROUNDS + 1];   // matchdays inside; secured from
    const int n = A.n, K = A.K, R = A.R, nc = A.nc;
    const int t = (int)blockIdx.x;
    const bool lead = t == n;
    uint32_t* flat = &hist[0][0][0];
    for (int i = threadIdx.x; i < 2 * TRAJECTORY_MAX_TARGETS * (TRAJECTORY_MAX_ROUNDS + 1); i += COUNT_THREADS) flat[i] = 0u;
    __syncthreads();

    const int step = (int)gridDim.y * COUNT_THREADS;
    for (int c = (int)blockIdx.y * COUNT_THREADS + (int)threadIdx.x; c < nc; c += step) {
        if (lead) {
            uint32_t before = A.leader[c], changes = 0u;
            for (int r = 1; r < R; ++r) {
                const uint32_t now = A.leader[(size_t)r * A.chunk + c];
                changes += now != before ? 1u : 0u;
                before = now;
            }
            atomicAdd(&hist[0][0][changes], 1u);   // (changes < R)
            continue;
        }
        // per target: the matchdays inside, and one past the last matchday outside (0: inside throughout)
        uint32_t count[TRAJECTORY_MAX_TARGETS], from[TRAJECTORY_MAX_TARGETS];
#pragma unroll
        for (int k = 0; k < TRAJECTORY_MAX_TARGETS; ++k) count[k] = from[k] = 0u;
        uint32_t p = 0u;
        for (int r = 0; r < R; ++r) {
            p = A.pos[((size_t)r * n + t) * A.chunk + c];
#pragma unroll
            for (int k = 0; k < TRAJECTORY_MAX_TARGETS; ++k) {
                const bool in = (A.mask[k] >> p) & 1ull;   // (mask[k] = 0 for k >= K)
                count[k] += in ? 1u : 0u;
                from[k] = in ? from[k] : (uint32_t)(r + 1);
            }
        }
#pragma unroll
        for (int k = 0; k < TRAJECTORY_MAX_TARGETS; ++k)
            if (k < K) {
                atomicAdd(&hist[0][k][count[k]], 1u);   // (count <= R, from <= R: R = outside after the last matchday)
                atomicAdd(&hist[1][k][from[k]], 1u);
            }
    }
    __syncthreads();
    // one global atomic per touched cell per workgroup
    if (lead) {
        for (int i = threadIdx.x; i < R; i += COUNT_THREADS) {
            const uint32_t cnt = hist[0][0][i];
            if (cnt) atomicAdd(&A.lead_changes[i], (unsigned long long)cnt);
        }
        return;
    }
    for (int i = threadIdx.x; i < K * (R + 1); i += COUNT_THREADS) {
        const int k = i / (R + 1), b = i - k * (R + 1);
        const uint32_t cnt = hist[0][k][b], sec = hist[1][k][b];
        if (cnt) atomicAdd(&A.rounds_inside[((size_t)t * K + k) * (R + 1) + b], (unsigned long long)cnt);
        if (sec) atomicAdd(&A.secured[((size_t)t * K + k) * (R + 1) + b], (unsigned long long)sec);
    }
}

}  // namespace dctr
