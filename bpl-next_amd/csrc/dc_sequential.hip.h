// dc_sequential.hip.h -- sequential (leave-future-out) updating of a fitted posterior on the device: the
// draws are re-weighted by the likelihood of the results seen since the fit, block of fixtures by block
// (a block is usually a gameweek), with Pareto-smoothed importance sampling, and the forecasts of every
// block are scored under the weights of the blocks before it.  Everything in float64; the [draws, fixtures]
// log-likelihood matrix is never stored.  DESIGN.md section 17.
//
// The host entry sorts the fixtures stably by block, packs each into a SeqFixture, and cuts every block into
// chunks of at most SEQ_CHUNK fixtures: chunk c holds the sorted fixtures chunk_begin[c] .. chunk_begin[c + 1] of block chunk_block[c],
// and block b owns the chunks block_chunk[b] .. block_chunk[b + 1].  lane = draw on the TEAM-major tables
// (dc_loglik.hip.h), so a fixture's rows are wave-uniform and the loads coalesce.
//
// Five kernels:
//   block_ll_tiles   A workgroup owns 256 draws (thread = draw) and one chunk: it adds ll (dcl::ll_at) over
//       the chunk's fixtures in sorted order and stores part[chunk][s].
//   block_ll_reduce  A[b, s] = the sum of part[c][s] over the chunks of block b, in chunk order; 0 for a
//       block without fixtures.  One thread per (b, s).
//   psis_rows        ONE WAVE PER BLOCK on a stored row r = R[b, .]: max and min; the first digit's
//       histogram of x = r - max r; dcl::psis_tail (the selection, gather, sort and fit of loglik_summary,
//       the same lines); lse(x) and lse(2 x) over the smoothed row; then lw = x - lse(x) is written with
//       the block's k, ess = exp(-lse(2 lw)) and tail length.  All draws equal: uniform weights, k = 0,
//       no tail.  max r = -inf (a dead block): lw = -inf, k = +inf, ess = 0.
//   weighted_tiles   A wave owns 64 draws (lane = draw) and one chunk; the four waves of a workgroup share
//       the chunk and take neighbouring draw tiles.  The chunk lies in one block, so the lane's log weight
//       and its exp stay in registers.  Per fixture: the outcome probabilities (dcs::outcome_probs, the
//       walk of dc_score.hip.h) times the weight, and the log-sum-exp term lw + ll, summed per lane over
//       its SEQ_D draws, then over the wave with xor butterflies, into
//       w_part[draw tile][n][5]: the three probabilities and the pair (max, sum of exp).
//   weighted_reduce  merges the draw tiles in index order: proba[n, 3] and elpd[n] = max + log(sum).
// No floating-point atomics; every sum has an order fixed by the data and by constants: results are
// bit-identical from run to run.  psis_rows reads its x from memory, so every pass sees the same bits;
// ll is evaluated by dcl::ll_at (contraction off) in both kernels that need it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"    // dcl::Fix, make_fix, ll_at, psis_tail, the wave helpers
#include "dc_outcome.hip.h"   // dcs::outcome_probs

namespace dcu {

constexpr int SEQ_MAX_BLOCKS = 4096;   // include/bplhip.h BPLHIP_SEQ_MAX_BLOCKS
constexpr int SEQ_CHUNK = 64;          // fixtures per chunk (DESIGN.md section 17 says why)
constexpr int SEQ_STRIP = 256;         // draws per workgroup of block_ll_tiles
constexpr int SEQ_D = 1;               // draws per lane of weighted_tiles (2 spills scalar registers in the venue form)
constexpr int SEQ_DRAWS = 64 * SEQ_D;
constexpr int SEQ_WAVES = 4;

// one fixture of the sorted query, packed by the host entry: one wave-uniform 32-byte load per fixture and one
// pointer in scalar registers, where the seven columns of dcq::Queries and the two lgamma values would take nine
// (the venue form of weighted_tiles spilled scalar registers with them).  lgamma comes from the host because the
// device's costs a lane some 90 registers, for two values a fixture has once.
struct SeqFixture {
    double lgx, lgy;            // lgamma(home goals + 1), lgamma(away goals + 1)
    uint16_t h, a, x, y, hc, ac;
    uint8_t neutral, pad[3];
};
static_assert(sizeof(SeqFixture) == 32, "SeqFixture is 32 bytes");

struct SeqArgs {
    dcq::Posterior<double> P;   // TEAM-major
    const SeqFixture* fx;       // [M] the fixtures with their actual goals, sorted by block
    long long M;
    int B, NC, TS, G;           // blocks, chunks, draw tiles ceil(S / SEQ_DRAWS), max_goals
    const int32_t* chunk_block;   // [NC]
    const int32_t* chunk_begin;   // [NC + 1]
    const int32_t* block_chunk;   // [B + 1]
    double* part;               // block_ll: [NC, S]
    double* A;                  // block_ll: [B, S]
    const double* lw;           // weighted: [B, S]
    double* w_part;             // weighted: [TS, M, 5]: the three weighted probabilities, then (max, sum of exp)
    double* proba;              // weighted: [M, 3]
    double* elpd;               // weighted: [M]
    double rk[dcs::SCORE_MAX_GOALS + 1];   // rk[k] = 1 / k (k >= 1)
};

struct PsisArgs {
    const double* R;   // [B, S]
    double* lw;        // [B, S]
    double* pareto_k;  // [B]
    double* ess;       // [B]
    int32_t* tail_len; // [B]
    int S, tail_m;
    double log_dbl_min;
};

// running log-sum-exp (m, s) that takes t = -inf (dcl::lse_add does not: its callers have finite terms)
__device__ __forceinline__ void lse_take(double& m, double& s, double t) {
    if (t > m) {
        s = s * exp(m - t) + 1.0;   // (m = -inf: s is 0 and stays finite)
        m = t;
    } else if (t > -INFINITY) {
        s += exp(t - m);
    }
}
// the pair form of dcl::wave_lse: every lane gets the wave's (max, sum of exp)
__device__ __forceinline__ void wave_lse_pair(double& m, double& s) {
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        const double mm = fmax(m, m2);
        const double a = m == -INFINITY ? 0.0 : s * exp(m - mm), b = m2 == -INFINITY ? 0.0 : s2 * exp(m2 - mm);
        s = a + b;   // (commutative: both lanes of a pair get the same bits)
        m = mm;
    }
}

// dcl::make_fix from the packed fixture
template <bool VENUE>
__device__ __forceinline__ dcl::Fix seq_fix(const SeqArgs& A, long long n) {
    const SeqFixture q = A.fx[n];
    dcl::Fix F = dcl::fix_rows_of<VENUE>(A.P, q.h, q.a, q.neutral, q.hc, q.ac);
    F.x = q.x;
    F.y = q.y;
    F.xd = (double)F.x;
    F.yd = (double)F.y;
    F.lgx = q.lgx;
    F.lgy = q.lgy;
    return F;
}

// ---- block sums
template <bool VENUE>
__global__ __launch_bounds__(SEQ_STRIP) void block_ll_tiles(SeqArgs A) {
    const int c = blockIdx.x;
    const int s = blockIdx.y * SEQ_STRIP + threadIdx.x;
    const int n0 = A.chunk_begin[c], n1 = A.chunk_begin[c + 1];
    double t = 0.0;
#pragma unroll 1
    for (int n = n0; n < n1; ++n) {
        const dcl::Fix F = seq_fix<VENUE>(A, n);
        if (s < A.P.S) t += dcl::ll_at<VENUE>(F, s);   // (-inf stays -inf; nothing here is +inf)
    }
    if (s < A.P.S) A.part[(size_t)c * (size_t)A.P.S + s] = t;
}

__global__ __launch_bounds__(256) void block_ll_reduce(SeqArgs A) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t S = (size_t)A.P.S;
    if (i >= (size_t)A.B * S) return;
    const size_t b = i / S, s = i - b * S;
    double t = 0.0;
    for (int c = A.block_chunk[b]; c < A.block_chunk[b + 1]; ++c) t += A.part[(size_t)c * S + s];
    A.A[i] = t;
}

// ---- PSIS of stored rows
__global__ __launch_bounds__(64) void psis_rows(PsisArgs A) {
    __shared__ unsigned long long tkey[dcl::LOGLIK_MAX_TAIL];   // tail keys, then the tail's z values
    __shared__ uint16_t tidx[dcl::LOGLIK_MAX_TAIL];             // tail draws
    __shared__ uint32_t hist[256];
    __shared__ double cut;
    const int lane = threadIdx.x, S = A.S;
    const size_t b = blockIdx.x;
    const double* r = A.R + b * (size_t)S;
    double* lw = A.lw + b * (size_t)S;

    double mx = -INFINITY, mn = INFINITY;
    for (int s = lane; s < S; s += 64) {
        const double v = r[s];
        mx = fmax(mx, v);
        mn = fmin(mn, v);
    }
    mx = dcl::wave_max(mx);
    mn = dcl::wave_min(mn);
    if (!(mx > -INFINITY) || mx == mn) {
        // a dead block (every draw ruled out), or constant ratios: no tail
        const bool dead = !(mx > -INFINITY);
        const double v = dead ? -INFINITY : 0.0 - log((double)S);   // (S = 1: +0, not -0)
        for (int s = lane; s < S; s += 64) lw[s] = v;
        if (lane == 0) {
            A.pareto_k[b] = dead ? INFINITY : 0.0;
            A.ess[b] = dead ? 0.0 : (double)S;
            A.tail_len[b] = 0;
        }
        return;
    }
    auto xat = [&](int s) { return (r[s] - mx) + 0.0; };   // (+ 0.0: a -0 becomes +0)

    for (int i = lane; i < 256; i += 64) hist[i] = 0u;
    dcl::wave_lds_order();
    for (int s = lane; s < S; s += 64) atomicAdd(&hist[dcl::key_of(xat(s)) >> 56], 1u);
    const dcl::PsisTail T = dcl::psis_tail(xat, S, A.tail_m, A.log_dbl_min, lane, hist, tkey, tidx, &cut);
    const bool smooth = T.kk < INFINITY;

    // lse(x) and lse(2 x) of the smoothed row
    double ma = -INFINITY, sa = 0.0, mb = -INFINITY, sb = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double x = xat(s);
        if (smooth && x > T.cutoff) continue;   // a tail draw: below
        lse_take(ma, sa, x);
        lse_take(mb, sb, 2.0 * x);
    }
    if (smooth) {
        for (int i = lane; i < T.L; i += 64) {
            const double x = dcl::psis_smoothed(T, i);
            lse_take(ma, sa, x);
            lse_take(mb, sb, 2.0 * x);
        }
    }
    const double lse_x = dcl::wave_lse(ma, sa), lse_2x = dcl::wave_lse(mb, sb);
    for (int s = lane; s < S; s += 64) {
        const double x = xat(s);
        if (smooth && x > T.cutoff) continue;
        lw[s] = x - lse_x;
    }
    if (smooth)
        for (int i = lane; i < T.L; i += 64) lw[tidx[T.base + i]] = dcl::psis_smoothed(T, i) - lse_x;
    if (lane == 0) {
        A.pareto_k[b] = T.kk;
        A.ess[b] = exp(-(lse_2x - 2.0 * lse_x));
        A.tail_len[b] = T.L;
    }
}

// ---- weighted scores
template <bool VENUE>
__global__ __launch_bounds__(64 * SEQ_WAVES) void weighted_tiles(SeqArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ts = blockIdx.y * SEQ_WAVES + wave;
    const int S = A.P.S;
    const size_t M = (size_t)A.M;
    if (ts >= A.TS) return;   // (wave uniform; no barrier below)
    const int c = blockIdx.x;
    const int n0 = A.chunk_begin[c], n1 = A.chunk_begin[c + 1];
    const double* lwb = A.lw + (size_t)A.chunk_block[c] * (size_t)S;
    double lw[SEQ_D], w[SEQ_D];
#pragma unroll
    for (int d = 0; d < SEQ_D; ++d) {
        const int s = ts * SEQ_DRAWS + d * 64 + lane;
        lw[d] = s < S ? lwb[s] : -INFINITY;
        w[d] = exp(lw[d]);   // (exp(-inf) = 0)
    }
#pragma unroll 1
    for (int n = n0; n < n1; ++n) {
        const dcl::Fix F = seq_fix<VENUE>(A, n);
        double acc[3] = {0.0, 0.0, 0.0};
        double m = -INFINITY, sm = 0.0;
#pragma unroll
        for (int d = 0; d < SEQ_D; ++d) {
            const int s = ts * SEQ_DRAWS + d * 64 + lane;
            if (s < S) {
                double eh, ea, pH, pD, pA;
                dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
                dcs::outcome_probs(eh, ea, F.corr[s], A.G, A.rk, &pH, &pD, &pA);
                acc[0] += w[d] * pH;
                acc[1] += w[d] * pD;
                acc[2] += w[d] * pA;
                lse_take(m, sm, lw[d] + dcl::ll_at<VENUE>(F, s));   // (-inf + -inf = -inf; nothing is +inf)
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = dcl::wave_sum(acc[k]);
        wave_lse_pair(m, sm);
        const double v = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : (lane == 2 ? acc[2] : (lane == 3 ? m : sm)));
        if (lane < 5) A.w_part[((size_t)ts * M + (size_t)n) * 5 + lane] = v;
    }
}

// one thread per element of proba [M, 3], then of elpd [M]
__global__ __launch_bounds__(256) void weighted_reduce(SeqArgs A) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t M = (size_t)A.M, M3 = M * 3;
    if (i < M3) {
        const size_t n = i / 3, k = i - n * 3;
        double t = 0.0;
        for (int ts = 0; ts < A.TS; ++ts) t += A.w_part[((size_t)ts * M + n) * 5 + k];
        A.proba[i] = t;
    } else if (i < M3 + M) {
        const size_t n = i - M3;
        double m = -INFINITY, s = 0.0;
        for (int ts = 0; ts < A.TS; ++ts) {
            const double m2 = A.w_part[((size_t)ts * M + n) * 5 + 3], s2 = A.w_part[((size_t)ts * M + n) * 5 + 4];
            if (m2 == -INFINITY) continue;
            const double mm = fmax(m, m2);
            s = (m == -INFINITY ? 0.0 : s * exp(m - mm)) + s2 * exp(m2 - mm);
            m = mm;
        }
        A.elpd[n] = m == -INFINITY ? -INFINITY : m + log(s);
    }
}

}  // namespace dcu
