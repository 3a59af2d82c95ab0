// dc_live_queries.hip.h -- match_leverage, points_needed and match_scenarios on a day with matches IN PROGRESS
// (their `in_play`, `reweight` and `log_weights`).  Three recording kernels, the stage-1 kernels
// of dc_leverage.hip.h, dc_points.hip.h and dc_scenario.hip.h with dc_live.hip.h's live parts added, so that under
// one key simulation j here is simulation j of dc_season_live bit for bit: the same draw, the same threefry blocks
// (j, g) with g the position in the CONCATENATED list (the F fixtures still to kick off, then the matches in play),
// the same final scores of the matches in play, the same tie-break block and ranking
// (tests/test_gpu_live_queries.py).  The loops are written out once more: a step shared with the kick-off kernels
// changed their compiled code (dc_season.hip.h), and those stay as they are.  Each kernel adds to its twin
//   - the draw of simulation j = j0 + c: with weights in force (C non-null) dclive::search_scan on the scan that
//     live_weights left, with U, W and step = W / N formed as dc_season_live forms them from the call's TOTAL
//     simulations N -- never the chunk's nc, so every chunking selects the same draws; otherwise j mod S.  The
//     search is wave wide (a ballot per pass): it stands at the top of the wave-uniform simulation loop;
//   - fixtures g >= F: dclive::sample_conditional from the state (a, b, t) of match g - F instead of
//     dcr::sample_scoreline, on the uniforms of block (j, g).  The lanes stay lane = g mod 64 in ONE loop over the
//     concatenated list -- dc_season_live lanes the matches in play afresh (lane = m), but the random numbers hang on
//     (j, g), not on the lane, so the scorelines are its own, and dc_leverage_count goes on reading bit `lane` of
//     block b as fixture 64 b + lane;
//   - nothing else: the records are the kick-off kernels' (dclev::LeverageArgs, dcpt::PointsArgs, dcsc::ScenarioArgs
//     carry them), and dc_leverage_count, dc_points_count and dc_scenario_count read them unchanged.
// live_loglik and live_weights (dc_live.hip.h) run once per call before the first chunk, on the same stream.
// Integer atomics only, vector stores only: every output is bit-identical run to run and for every chunk length.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_leverage.hip.h"    // dclev::LeverageArgs and the kick-off kernel's constants
#include "dc_live.hip.h"        // dclive::search_scan, sample_conditional, RESAMPLE_COUNTER
#include "dc_points.hip.h"      // dcpt::PointsArgs
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_scenario.hip.h"    // dcsc::ScenarioArgs, wave_sum_u32
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dclq {

// what the three kernels take on top of their twins' records (whose nf counts the F ordinary fixtures AND the L in
// play).  A record of this namespace: the kernels' mangled names carry no dclive type
struct LiveQuery {
    int F;                      // the ordinary fixtures come first
    long long N;                // the call's simulations, all chunks together
    const uint32_t* st_goals;   // [L]: a | b << 8
    const double* st_t;         // [L] elapsed fraction
    const double* C;            // [S] the scan of the weights, or null: simulation j takes draw j mod S
};

// one offset U for the whole call, targets (j + U) W / N: dc_season_live's three values
struct Resample {
    double U, W, step;
};
__device__ __forceinline__ Resample resample_of(const LiveQuery& V, int S, uint32_t key_hi, uint32_t key_lo) {
    Resample R{0.0, 0.0, 0.0};
    if (V.C) {
        uint32_t o0, o1;
        nd::tf_block(key_hi, key_lo, 0u, dclive::RESAMPLE_COUNTER, &o0, &o1);
        R.U = dcr::unit_open(o0);
        R.W = V.C[S - 1];
        R.step = R.W / (double)V.N;
    }
    return R;
}
// the draw of simulation j (wave uniform, all 64 lanes active)
__device__ __forceinline__ int draw_of(const LiveQuery& V, const Resample& R, int S, long long j, int lane) {
    if (V.C) {
        const double target = fmin(((double)j + R.U) * R.step, R.W);
        return min(dclive::search_scan(V.C, S, target, lane), S - 1);
    }
    return (int)(j % S);
}

// dclev::dc_leverage_sim's launch shape and records; fixtures V.F .. A.nf - 1 start from their states
template <bool H2H>
__global__ __launch_bounds__(64 * dclev::LEVERAGE_WAVES) void live_leverage_sim(dclev::LeverageArgs A, dch::PairArgs H,
                                                                                 LiveQuery V) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist[dclev::LEVERAGE_MAX_TEAMS * dclev::LEVERAGE_MAX_TARGETS];
    __shared__ int32_t tab[dclev::LEVERAGE_WAVES][3][dclev::LEVERAGE_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = H2H ? (int)(blockDim.x >> 6) : dclev::LEVERAGE_WAVES;
    const int n = A.n, nf = A.nf, K = A.K, F = V.F;
    for (int i = threadIdx.x; i < n * K; i += blockDim.x) hist[i] = 0u;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    const Resample R = resample_of(V, A.S, A.key_hi, A.key_lo);

    const int waves = (int)gridDim.x * nw;
    for (int c = (int)blockIdx.x * nw + wave; c < A.nc; c += waves) {
        const long long j = A.j0 + c;
        const int s = draw_of(V, R, A.S, j, lane);
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
        const double* att = A.attack + (size_t)s * A.T;
        const double* dfn = A.defence + (size_t)s * A.T;
        const double* hadv = A.ha_stride ? A.home_adv + (size_t)s * A.T : A.home_adv + s;
        const double rho = A.corr[s];
        // (the trip count is the wave's, not the lane's: the ballots below take every lane)
        for (int base = 0, b = 0; base < nf; base += 64, ++b) {
            const int g = base + lane;
            bool home_win = false, away_win = false;
            if (g < nf) {
                const uint32_t hw = A.fix[g];
                const int h = (int)(hw & 0xFFFFu), a = (int)(hw >> 16);
                const uint32_t sl = A.fix_slot[g];
                const int hs = (int)(sl & 0xFFu), as = (int)(sl >> 8);
                double eh = att[h] - dfn[a];
                eh = eh + (A.ha_stride ? hadv[h] : hadv[0]);
                const double lh = exp(eh), la = exp(att[a] - dfn[h]);
                uint32_t o0, o1;
                nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, (uint32_t)g, &o0, &o1);
                int x, y;
                if (g >= F) {
                    const uint32_t st = V.st_goals[g - F];
                    dclive::sample_conditional(lh, la, rho, (int)(st & 0xFFu), (int)(st >> 8), 1.0 - V.st_t[g - F],
                                               dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
                } else {
                    dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
                }
                dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
                if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
                home_win = x > y;   // (a match in play is classified by its FINAL score)
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
        // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
        if constexpr (!H2H) dcr::wave_lds_order();
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int ahead = 0;
        if constexpr (H2H) {
            ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
            dcr::wave_lds_order();
        } else {
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

// dcpt::dc_points_sim's launch shape and records; fixtures V.F .. A.nf - 1 start from their states
template <bool H2H>
__global__ __launch_bounds__(64 * dcpt::POINTS_WAVES) void live_points_sim(dcpt::PointsArgs A, dch::PairArgs H, LiveQuery V) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ int32_t tab[dcpt::POINTS_WAVES][3][dcpt::POINTS_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = H2H ? (int)(blockDim.x >> 6) : dcpt::POINTS_WAVES;
    const int n = A.n, nf = A.nf, K = A.K, F = V.F;

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    const Resample R = resample_of(V, A.S, A.key_hi, A.key_lo);

    const int waves = (int)gridDim.x * nw;
    for (int c = (int)blockIdx.x * nw + wave; c < A.nc; c += waves) {
        const long long j = A.j0 + c;
        const int s = draw_of(V, R, A.S, j, lane);
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
        const double* att = A.attack + (size_t)s * A.T;
        const double* dfn = A.defence + (size_t)s * A.T;
        const double* hadv = A.ha_stride ? A.home_adv + (size_t)s * A.T : A.home_adv + s;
        const double rho = A.corr[s];
        for (int g = lane; g < nf; g += 64) {
            const uint32_t hw = A.fix[g];
            const int h = (int)(hw & 0xFFFFu), a = (int)(hw >> 16);
            const uint32_t sl = A.fix_slot[g];
            const int hs = (int)(sl & 0xFFu), as = (int)(sl >> 8);
            double eh = att[h] - dfn[a];
            eh = eh + (A.ha_stride ? hadv[h] : hadv[0]);
            const double lh = exp(eh), la = exp(att[a] - dfn[h]);
            uint32_t o0, o1;
            nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, (uint32_t)g, &o0, &o1);
            int x, y;
            if (g >= F) {
                const uint32_t st = V.st_goals[g - F];
                dclive::sample_conditional(lh, la, rho, (int)(st & 0xFFu), (int)(st >> 8), 1.0 - V.st_t[g - F],
                                           dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            } else {
                dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            }
            dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
            if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
        }
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, dcpt::POINTS_MAX_TEAMS, lane, slot_lane);
        // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
        if constexpr (!H2H) dcr::wave_lds_order();
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int ahead = 0;
        if constexpr (H2H) {
            ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
            dcr::wave_lds_order();
        } else {
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

// dcsc::dc_scenario_sim's launch shape and records; fixtures V.F .. A.nf - 1 start from their states, and a key
// among them is classed by its FINAL clipped margin
template <bool H2H>
__global__ __launch_bounds__(64 * dcsc::SCENARIO_WAVES) void live_scenario_sim(dcsc::ScenarioArgs A, dch::PairArgs H,
                                                                               LiveQuery V) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ int32_t tab[dcsc::SCENARIO_WAVES][3][dcsc::SCENARIO_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = H2H ? (int)(blockDim.x >> 6) : dcsc::SCENARIO_WAVES;
    const int n = A.n, nf = A.nf, K = A.K, F = V.F;

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    const Resample R = resample_of(V, A.S, A.key_hi, A.key_lo);

    const int waves = (int)gridDim.x * nw;
    for (int c = (int)blockIdx.x * nw + wave; c < A.nc; c += waves) {
        const long long j = A.j0 + c;
        const int s = draw_of(V, R, A.S, j, lane);
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
        const double* att = A.attack + (size_t)s * A.T;
        const double* dfn = A.defence + (size_t)s * A.T;
        const double* hadv = A.ha_stride ? A.home_adv + (size_t)s * A.T : A.home_adv + s;
        const double rho = A.corr[s];
        uint32_t cell = 0u;   // class x stride of this lane's key fixtures, over all blocks of the list
        for (int g = lane; g < nf; g += 64) {
            const uint32_t hw = A.fix[g];
            const int h = (int)(hw & 0xFFFFu), a = (int)(hw >> 16);
            const uint32_t sl = A.fix_slot[g];
            const int hs = (int)(sl & 0xFFu), as = (int)(sl >> 8);
            double eh = att[h] - dfn[a];
            eh = eh + (A.ha_stride ? hadv[h] : hadv[0]);
            const double lh = exp(eh), la = exp(att[a] - dfn[h]);
            uint32_t o0, o1;
            nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, (uint32_t)g, &o0, &o1);
            int x, y;
            if (g >= F) {
                const uint32_t st = V.st_goals[g - F];
                dclive::sample_conditional(lh, la, rho, (int)(st & 0xFFu), (int)(st >> 8), 1.0 - V.st_t[g - F],
                                           dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            } else {
                dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            }
            dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
            if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            const uint32_t code = A.fix_code[g];
            const int cap = (int)(code >> dcsc::CODE_CAP_SHIFT);   // (0 for a fixture that is no key: it adds nothing)
            cell += (uint32_t)(cap - min(max(x - y, -cap), cap)) * (code & ((1u << dcsc::CODE_CAP_SHIFT) - 1u));
        }
        cell = dcsc::wave_sum_u32(cell);
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, dcsc::SCENARIO_MAX_TEAMS, lane, slot_lane);
        // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
        if constexpr (!H2H) dcr::wave_lds_order();
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
        int ahead = 0;
        if constexpr (H2H) {
            ahead = dch::pair_rank<false>(pair, H.pitch, n, lane, slot_lane, row, r0, 0);
            dcr::wave_lds_order();
        } else {
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

}  // namespace dclq
