// dc_live.hip.h -- the rest of a season on a day with matches IN PROGRESS (simulate_season's `in_play`,
// `reweight` and `log_weights`).  dc_season.hip.h plays every fixture from 0-0 with the
// posterior draws at equal weight; here L of the fixtures start from a state (a, b, t) -- current score and elapsed
// fraction, dc_inplay.hip.h's -- and the draws carry weights: the joint likelihood of all the states (section 25's
// l, summed over the matches) and / or the caller's log weights.  Three kernels on one stream, nothing comes back
// to the host between them:
//   live_loglik   lane = draw on the TEAM-major tables, a sequential loop over the L states (wave-uniform
//       operands): l[s, m] = log Pois(a; lh t) + log Pois(b; la t) + log Z exactly as dc_inplay.hip.h forms it
//       (restated here: nothing of that header is shared), lgamma from the 64-entry table in the arguments, a count
//       of 0 takes no logarithm.  L0[s] = sum_m l[s, m] in m order, L[s] = (L0[s] if reweight) + (lw[s] if given).
//   live_weights  ONE workgroup, any S: the block maximum of L, w[s] = exp(L[s] - max L), the inclusive scan C of w
//       in draw order with a FIXED association -- thread i owns the i-th contiguous segment and sums it
//       sequentially, the segment totals are added left to right, C[s] = (the segment's start) + (its own partial
//       sum up to s), as dc_inplay.hip.h's inplay_summary scans -- into global memory; W = C[S-1], ess =
//       W^2 / sum w^2 and log_evidence = max L0 + log(mean exp(L0 - max L0)) from the same segments.
//   dc_season_live<H2H>   dc_season's structure statement for statement (one wave per simulation, the same LDS
//       table, dctab / dch booking and ranking, the same integer-atomic histogram flush), plus
//       - the draw of simulation j: with weights, SYSTEMATIC RESAMPLING on the scan -- U = unit_open(o0) of the
//         threefry block (0, RESAMPLE_COUNTER) under the call's key, step = W / N, target_j = min((j + U) step, W),
//         s_j = #{s : C[s] < target_j} (at most S - 1: C[S-1] = W; a draw with w = 0 repeats its predecessor's C
//         and is never selected) by a wave-uniform 64-ary search of C (L2-resident): every lane probes one split
//         point, the ballot's population count is the number of split points below the target; without weights
//         (C null) s_j = j mod S;
//       - the in-play fixtures, lane = in-play match, after the F ordinary ones (which go through
//         dcr::sample_scoreline itself): sample_conditional below on the block (j, F + m);
//       - the optional outputs: the draw of every simulation; the final scores of the in-play matches are
//         columns F .. F + L - 1 of home_goals / away_goals.
// Integer atomics only, no floating-point atomics, vector stores only: every output is bit-identical run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_h2h.hip.h"         // dch::PairArgs, pair_reset, pair_book, pair_rank
#include "dc_sampler.hip.h"     // dcr::sample_scoreline, unit_open, wave_lds_order
#include "dc_season.hip.h"      // dcs::SeasonArgs, SEASON_WAVES, SEASON_MAX_TEAMS
#include "dc_table.hip.h"       // dctab::load_row, store_row, book, rank_keys
#include "nuts_dev.hip.h"       // nd::tf_block

namespace dclive {

constexpr uint32_t RESAMPLE_COUNTER = 0x20000000u;   // dc_sampler.hip.h's counter table
constexpr int LIVE_MAX_GOALS = 63;                   // a current score (include/bplhip.h BPLHIP_LIVE_MAX_GOALS)
constexpr int LIVE_WAVES = 4;
constexpr int LIVE_THREADS = 64 * LIVE_WAVES;

// the states and the weights: what live_loglik and live_weights read and write
struct LiveArgs {
    int S, L, reweight, ha_stride;
    const double* attack;       // TEAM-major [T, S]
    const double* defence;      // TEAM-major [T, S]
    const double* home_adv;     // [S] (ha_stride = 0) or TEAM-major [T, S]
    const double* corr;         // [S]
    const uint32_t* st_fix;     // [L]: home | away << 16 (model indices)
    const uint32_t* st_goals;   // [L]: a | b << 8
    const double* st_t;         // [L] elapsed fraction
    const double* lw;           // [S] log weights, or null
    double* Lw;                 // [S] L
    double* L0;                 // [S] the state part alone
    double* C;                  // [S] the scan of the weights
    double* stats;              // [3]: W, ess, log_evidence
    double lgf[LIVE_MAX_GOALS + 1];   // lgf[k] = lgamma(k + 1)
};

// what dc_season_live takes on top of dcs::SeasonArgs (whose nf counts the F ordinary fixtures AND the L in play)
struct LiveSim {
    int F;                      // the ordinary fixtures come first
    const uint32_t* st_goals;   // [L]: a | b << 8
    const double* st_t;         // [L]
    const double* C;            // [S] the scan, or null: simulation j takes draw j mod S
    int32_t* sim_draw;          // [n_sims] or null
};

// grid: ceil(S / LIVE_THREADS) workgroups
__global__ __launch_bounds__(LIVE_THREADS) void live_loglik(LiveArgs A) {
#pragma clang fp contract(off)
    const int s = blockIdx.x * LIVE_THREADS + threadIdx.x;
    const size_t S = (size_t)A.S;
    if (s >= A.S) return;   // (no barrier below)
    const double rho = A.corr[s];
    double l0 = 0.0;
#pragma unroll 1
    for (int m = 0; m < A.L; ++m) {
        const uint32_t hw = A.st_fix[m], g = A.st_goals[m];   // (wave uniform)
        const int h = (int)(hw & 0xFFFFu), aw = (int)(hw >> 16);
        const int a = (int)(g & 0xFFu), b = (int)(g >> 8);
        const double t = A.st_t[m], r = 1.0 - t;
        const double ha = A.ha_stride ? A.home_adv[h * S + s] : A.home_adv[s];
        const double eh = A.attack[h * S + s] - A.defence[aw * S + s] + ha;
        const double ea = A.attack[aw * S + s] - A.defence[h * S + s];
        const double lh = exp(eh), la = exp(ea);
        const double lhr = lh * r, lar = la * r;
        const double u0 = exp(-lhr), v0 = exp(-lar);
        const double c00 = rho * -(lh * la), c01 = rho * lh, c10 = rho * la, c11 = rho * -1.0;
        // Z: the tau cells at or beyond (a, b), each (f - 1) u_(x-a) v_(y-b), f - 1 = max(rho c, -1)
        const double u1 = u0 * lhr, v1 = v0 * lar;
        const double hx0 = a == 0 ? u0 : 0.0, hx1 = a == 0 ? u1 : (a == 1 ? u0 : 0.0);
        const double hy0 = b == 0 ? v0 : 0.0, hy1 = b == 0 ? v1 : (b == 1 ? v0 : 0.0);
        const double Z = 1.0 + (((fmax(c00, -1.0) * (hx0 * hy0) + fmax(c01, -1.0) * (hx0 * hy1)) +
                                 fmax(c10, -1.0) * (hx1 * hy0)) + fmax(c11, -1.0) * (hx1 * hy1));
        // a count of 0 takes no logarithm (t = 0 comes with 0-0)
        const double lt = log(t);
        const double pa = (a > 0 ? (double)a * (eh + lt) : 0.0) - lh * t - A.lgf[a];
        const double pb = (b > 0 ? (double)b * (ea + lt) : 0.0) - la * t - A.lgf[b];
        l0 = l0 + ((pa + pb) + log(Z));
    }
    A.L0[s] = l0;
    A.Lw[s] = (A.reweight ? l0 : 0.0) + (A.lw ? A.lw[s] : 0.0);
}

// the workgroup's maximum (commutative: any order gives the same bits); red: [LIVE_WAVES] LDS
__device__ __forceinline__ double live_block_max(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();   // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
// the total of the threads' values added LEFT TO RIGHT (thread 0 first), and what comes before this thread's
__device__ __forceinline__ double live_ordered_total(double part, double* tot, double* before) {
    __syncthreads();   // (tot may still be read from the call before)
    tot[threadIdx.x] = part;
    __syncthreads();
    double w = 0.0;
    for (int i = 0; i < LIVE_THREADS; ++i) {
        if (i == (int)threadIdx.x) *before = w;
        w += tot[i];
    }
    return w;
}

// ONE workgroup of LIVE_THREADS threads
__global__ __launch_bounds__(LIVE_THREADS) void live_weights(LiveArgs A) {
#pragma clang fp contract(off)
    __shared__ double red[LIVE_WAVES];
    __shared__ double tot[LIVE_THREADS];
    const int tid = threadIdx.x, S = A.S;
    double lmax = -INFINITY, m0 = -INFINITY;
    for (int s = tid; s < S; s += LIVE_THREADS) {
        lmax = fmax(lmax, A.Lw[s]);
        m0 = fmax(m0, A.L0[s]);
    }
    lmax = live_block_max(lmax, red);
    m0 = live_block_max(m0, red);
    // thread i owns draws i per .. (i + 1) per - 1
    const int per = (S + LIVE_THREADS - 1) / LIVE_THREADS;
    const int lo = min(tid * per, S), hi = min(lo + per, S);
    double part = 0.0, sq = 0.0, ev = 0.0;
    for (int s = lo; s < hi; ++s) {
        const double o = exp(A.Lw[s] - lmax);
        part += o;
        sq += o * o;
        ev += exp(A.L0[s] - m0);
    }
    double before = 0.0, unused = 0.0;
    const double W = live_ordered_total(part, tot, &before);
    const double sww = live_ordered_total(sq, tot, &unused);
    const double e = live_ordered_total(ev, tot, &unused);
    double p = 0.0;   // (C[s] = before + the segment's own partial sum: C at the segment's end is the next `before`)
    for (int s = lo; s < hi; ++s) {
        p += exp(A.Lw[s] - lmax);
        A.C[s] = before + p;
    }
    if (tid == 0) {
        A.stats[0] = W;
        A.stats[1] = W * W / sww;
        A.stats[2] = m0 + log(e / (double)S);
    }
}

// One FINAL scoreline of a match that stands a : b with the fraction r = 1 - t still to play, from the two
// uniforms: remaining goals Poisson with the thinned rates lh r, la r, tau on the final score with the FULL-MATCH
// rates (dc_inplay.hip.h's law, sampled exactly as dcr::sample_scoreline samples the kick-off law):
//     v0 = exp(-la r), v1 = v0 la r;  c_x = 1 + sum_{y in {0,1}, y >= b} (tau(x, y) - 1) v_(y-b)  (x <= 1; else 1)
//     u0 = exp(-lh r), u1 = u0 lh r;  Z = 1 + sum_{x in {0,1}, x >= a} u_(x-a) (c_x - 1)
//     home: p_k = p_{k-1} lh r / k, the first k with  u1 Z < sum_{i<=k} p_i c_(a+i);        x = a + k (capped at 255)
//     away: p'_k = p'_{k-1} la r / k, the first k with  u2 c_x < sum_{i<=k} p'_i tau(x, b+i);  y = b + k (capped at 255)
// The terms stand in sample_scoreline's order: at a = b = 0, r = 1 this performs the same operations and returns the
// same scoreline bit for bit (tests/test_live_host.py has the restatement do so; contraction off as there).
__device__ inline void sample_conditional(double lh, double la, double rho, int a, int b, double r, double u1,
                                          double u2, int* xo, int* yo) {
#pragma clang fp contract(off)
    const double t00 = fmax(1.0 - lh * la * rho, 0.0);
    const double t01 = fmax(1.0 + lh * rho, 0.0);
    const double t10 = fmax(1.0 + la * rho, 0.0);
    const double t11 = fmax(1.0 - rho, 0.0);
    const double lhr = lh * r, lar = la * r;
    const double q0 = exp(-lar), q1 = q0 * lar;
    double c0 = 1.0, c1 = 1.0;
    if (b == 0) {
        c0 = 1.0 + (t00 - 1.0) * q0 + (t01 - 1.0) * q1;
        c1 = 1.0 + (t10 - 1.0) * q0 + (t11 - 1.0) * q1;
    } else if (b == 1) {
        c0 = 1.0 + (t01 - 1.0) * q0;
        c1 = 1.0 + (t11 - 1.0) * q0;
    }
    const double p0 = exp(-lhr), p1 = p0 * lhr;
    double Z = 1.0;
    if (a == 0) Z = 1.0 + p0 * (c0 - 1.0) + p1 * (c1 - 1.0);
    else if (a == 1) Z = 1.0 + p0 * (c1 - 1.0);
    // home goals: marginal u_(x-a) c_x / Z
    const double th = u1 * Z;
    double p = p0, acc = a == 0 ? p0 * c0 : a == 1 ? p0 * c1 : p0;
    int x = a;
    while (!(th < acc) && x < 255) {
        ++x;
        p = p * lhr / (double)(x - a);
        acc = acc + (x == 1 ? p * c1 : p);
    }
    // away goals given x: tau(x, y) v_(y-b) / c_x
    const double ta = u2 * (x == 0 ? c0 : x == 1 ? c1 : 1.0);
    const double f0 = x == 0 ? t00 : x == 1 ? t10 : 1.0;   // tau(x, 0), tau(x, 1)
    const double f1 = x == 0 ? t01 : x == 1 ? t11 : 1.0;
    const double tau0 = b == 0 ? f0 : b == 1 ? f1 : 1.0;   // tau(x, b), tau(x, b + 1)
    const double tau1 = b == 0 ? f1 : 1.0;
    p = q0;
    acc = q0 * tau0;
    int y = b;
    while (!(ta < acc) && y < 255) {
        ++y;
        p = p * lar / (double)(y - b);
        acc = acc + (y - b == 1 ? p * tau1 : p);
    }
    *xo = x;
    *yo = y;
}

// #{s : C[s] < target} over the non-decreasing C[0 .. S-1], wave uniform (all 64 lanes active): the answer stays in
// [lo, hi]; each pass probes up to 64 split points `step` apart, one per lane, and the probes below the target are a
// prefix of the lanes
__device__ __forceinline__ int search_scan(const double* __restrict__ C, int S, double target, int lane) {
    int lo = 0, hi = S;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int at = lo + (lane + 1) * step - 1;   // (step <= 2^25: no overflow)
        const bool below = at < hi && C[at] < target;
        const int cnt = (int)__popcll(__ballot(below));
        lo += cnt * step;             // C[lo - 1] < target
        hi = min(lo + step - 1, hi);  // C[lo + step - 1] >= target, where it was probed
    }
    return lo;
}

// H2H as for dcs::dc_season: blockDim.x = 64 x dch::waves_for(n) and dch::lds_bytes(n) of dynamic LDS
template <bool H2H>
__global__ __launch_bounds__(64 * dcs::SEASON_WAVES) void dc_season_live(dcs::SeasonArgs A, dch::PairArgs H, LiveSim V) {
    extern __shared__ uint32_t pairs[];   // H2H only: the waves' pair matrices
    __shared__ uint32_t hist[dcs::SEASON_MAX_TEAMS * dcs::SEASON_MAX_TEAMS];
    __shared__ unsigned long long bsum[2][dcs::SEASON_MAX_TEAMS];
    __shared__ int32_t tab[dcs::SEASON_WAVES][3][dcs::SEASON_MAX_TEAMS];   // per wave: points, GF, GA
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = H2H ? (int)(blockDim.x >> 6) : dcs::SEASON_WAVES;
    const int n = A.n, nf = A.nf, F = V.F;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x < 2 * dcs::SEASON_MAX_TEAMS) (&bsum[0][0])[threadIdx.x] = 0ull;
    __syncthreads();

    int32_t* table = &tab[wave][0][0];
    uint32_t* pair = nullptr;
    if constexpr (H2H) pair = pairs + (size_t)wave * n * H.pitch;
    const bool slot_lane = lane < n;
    const dctab::Row init = dctab::load_row(A.init, n, lane, slot_lane);
    long long psum = 0, gdsum = 0;   // this lane's slot over the wave's simulations

    // systematic resampling: one offset U for the whole call, targets (j + U) W / N
    double U = 0.0, W = 0.0, step = 0.0;
    if (V.C) {
        uint32_t o0, o1;
        nd::tf_block(A.key_hi, A.key_lo, 0u, RESAMPLE_COUNTER, &o0, &o1);
        U = dcr::unit_open(o0);
        W = V.C[A.S - 1];
        step = W / (double)A.n_sims;
    }

    const long long waves = (long long)gridDim.x * nw;
    for (long long j = (long long)blockIdx.x * nw + wave; j < A.n_sims; j += waves) {
        int s;
        if (V.C) {
            const double target = fmin(((double)j + U) * step, W);
            s = min(search_scan(V.C, A.S, target, lane), A.S - 1);
        } else {
            s = (int)(j % A.S);
        }
        dctab::store_row(table, lane, slot_lane, init);
        if constexpr (H2H) dch::pair_reset(pair, H, n, lane);
        dcr::wave_lds_order();
        const double* att = A.attack + (size_t)s * A.T;
        const double* dfn = A.defence + (size_t)s * A.T;
        const double* hadv = A.ha_stride ? A.home_adv + (size_t)s * A.T : A.home_adv + s;
        const double rho = A.corr[s];
        // fixture g of the concatenated list: dc_season's fixture step, the sampler chosen by `live`
        auto play = [&](const int g, const bool live) {
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
            if (live) {
                const uint32_t st = V.st_goals[g - F];
                sample_conditional(lh, la, rho, (int)(st & 0xFFu), (int)(st >> 8), 1.0 - V.st_t[g - F],
                                   dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            } else {
                dcr::sample_scoreline(lh, la, rho, dcr::unit_open(o0), dcr::unit_open(o1), &x, &y);
            }
            dctab::book(table, hs, as, x, y, A.win, A.draw, A.loss);
            if constexpr (H2H) dch::pair_book(pair, H.pitch, hs, as, x, y, A.win, A.draw, A.loss);
            if (A.home_goals) {
                A.home_goals[(size_t)j * nf + g] = (uint8_t)x;
                A.away_goals[(size_t)j * nf + g] = (uint8_t)y;
            }
        };
        // the ordinary fixtures first (dc_season's loop), then lane = in-play match
        for (int f = lane; f < F; f += 64) play(f, false);
        for (int m = lane; m < nf - F; m += 64) play(F + m, true);
        dcr::wave_lds_order();
        const dctab::Row row = dctab::load_row(table, dcs::SEASON_MAX_TEAMS, lane, slot_lane);
        // the next simulation's reset comes after the reads of the wave's LDS: here, or after pair_rank's
        if constexpr (!H2H) dcr::wave_lds_order();
        uint32_t r0 = 0u, r1;
        if (slot_lane) nd::tf_block(A.key_hi, A.key_lo, (uint32_t)j, dcr::TIEBREAK_COUNTER | (uint32_t)lane, &r0, &r1);
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
        }
        if (V.sim_draw && lane == 0) V.sim_draw[j] = s;
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

}  // namespace dclive
