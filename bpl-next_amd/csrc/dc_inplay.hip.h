// dc_inplay.hip.h -- match markets of a match IN PROGRESS: the state is the elapsed fraction t in [0, 1) and the
// current score (a, b); r = 1 - t.  Goal times are exchangeable within a match, so with the full-match rates
// lh, la of a draw (dcl::log_rates_at) the joint law of the state at t and the final score (x, y) factorises:
//     P_s(state, final) = Pois(a; lh t) Pois(b; la t) * tau_s(x, y) Pois(x - a; lh r) Pois(y - b; la r)
// (tau on the FINAL score, with the FULL-MATCH rates).  Per draw s, fixture n and market k:
//     u_i = Pois(i; lh r), v_j = Pois(j; la r)
//     p~(x, y) = f(x, y) u_(x-a) v_(y-b) on a <= x <= G, b <= y <= G; f = max(1 + rho c, 0) on {0,1}^2, else 1
//     Z   = 1 + sum over the tau cells with x >= a, y >= b of (f - 1) u_(x-a) v_(y-b)     (untruncated support)
//     val[s, k, n] = (sum_{x, y <= G} W_k[x, y] p~(x, y)) / Z                             (W by FINAL score)
//     l[s, n]      = log Pois(a; lh t) + log Pois(b; la t) + log Z                        (Pois(0; 0) = 1)
// f - 1 is formed as max(rho c, -1): no cancellation in the factor itself; what is left in Z is bounded in
// section 25.  The draws are then re-weighted per fixture, w[s] = exp(L[s] - max L), L = (l if reweight) +
// (log_weights[s] if given), and summarised with those weights: mean, sd (population form), the weighted inverted
// CDF at each quantile, the effective sample size and the log evidence of the state.
//
// Two kernels:
//   inplay_values   dcm::market_values' structure (lane = draw on the team-major tables, four waves share a
//       fixture and a pass of INPLAY_KPASS markets, weights from the [pass][cell][8] copy through wave-uniform
//       loads, registers only), with the walk started at (a, b) -- wave uniform, from the query's goal columns.
//       The y blocks start at b, so the last block is partial for most b; the tau factors go by FINAL cell.
//       Z and l come once per (draw, fixture) from the same u_0, u_1, v_0, v_1; pass 0 alone writes l.
//   inplay_summary  ONE WORKGROUP PER (fixture, market): keys (dcl::key_of) and draw indices in LDS, the stable
//       LSD radix sort dcg::radix_sort (ties keep the draw order), then the weights are written over the keys
//       (by draw), gathered by sorted position and scanned in a fixed order: thread i owns the i-th segment of
//       the sorted order, sums it sequentially, the segment totals are added left to right (a segment's start;
//       W is the last), C_i is the segment's start plus its own partial sum, and the crossing C_i >= q W of each
//       quantile is read off by the one thread whose segment holds it.  Mean and sd are
//       fixed-order two-pass sums.  The market-0 workgroup of a fixture writes ess and log_evidence.
// No floating-point atomics, no scratch, vector stores only; contraction is off and every fma explicit.  A value's
// accumulation order depends only on its own (draw, fixture, market, a, b): results are bit-identical from run to
// run, under any chunking and under any order of the fixtures.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_diagnostics.hip.h"   // dcg::radix_sort, block_sum
#include "dc_loglik.hip.h"        // dcl::Fix, fix_rows, log_rates_at, key_of, wave_max
#include "dc_market.hip.h"        // the walk this one follows

namespace dcip {

constexpr int INPLAY_MAX_GOALS = dcm::MARKET_MAX_GOALS;
constexpr int INPLAY_MAX_DRAWS = 12288;   // include/bplhip.h BPLHIP_INPLAY_MAX_DRAWS = dcg::DIAG_LDS_DRAWS
constexpr int INPLAY_KPASS = dcm::MARKET_KPASS;
constexpr int INPLAY_YB = dcm::MARKET_YB;
constexpr int INPLAY_WAVES = 4;
constexpr int INPLAY_THREADS = 64 * INPLAY_WAVES;
static_assert(INPLAY_MAX_DRAWS == dcg::DIAG_LDS_DRAWS && INPLAY_WAVES == dcg::DIAG_WAVES, "dcg::radix_sort's shape");

struct InplayArgs {
    dcq::Posterior<double> P;   // TEAM-major
    dcq::Queries Q;             // the fixtures, goals = the current score
    int G, K, NQ, reweight;
    long long n0, nc;           // the chunk: fixtures n0 .. n0 + nc - 1
    const double* w;            // [ceil(K / INPLAY_KPASS)][(G+1)^2][INPLAY_KPASS]
    const double* q;            // [NQ]
    const double* t;            // [M] elapsed fraction
    const double* lw;           // [S] log weights, or null
    double* vals;               // [nc, K, S]
    double* lev;                // [nc, S] log evidence of the state per draw
    double* mean;               // [K, M]
    double* sd;                 // [K, M]
    double* quant;              // [K, NQ, M]
    double* ess;                // [M]
    double* logev;              // [M]
    double rk[INPLAY_MAX_GOALS + 1];    // rk[k] = 1 / k (k >= 1)
    double lgf[INPLAY_MAX_GOALS + 1];   // lgf[k] = lgamma(k + 1)
};

__host__ __device__ inline size_t inplay_summary_lds_bytes(int S) {
    return (size_t)S * 12;   // keys (then weights) 8 B, two index buffers 2 B each
}

// grid: (fixture of the chunk, draw tile group, pass)
template <bool VENUE>
__global__ __launch_bounds__(64 * INPLAY_WAVES) void inplay_values(InplayArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = A.P.S, G = A.G;
    const int s = (blockIdx.y * INPLAY_WAVES + wave) * 64 + lane;
    const long long f = blockIdx.x;
    const int pass = blockIdx.z;
    if (s >= S) return;   // (no barrier below)
    const long long n = A.n0 + f;
    const dcl::Fix F = dcl::fix_rows<VENUE>(A.P, A.Q, n);
    const int a = A.Q.x[n], b = A.Q.y[n];   // (wave uniform; a, b <= G checked by the host entry)
    const double t = A.t[n], r = 1.0 - t;
    double eh, ea;
    dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
    const double rho = F.corr[s];
    const double lh = exp(eh), la = exp(ea);
    const double lhr = lh * r, lar = la * r;   // the thinned rates of what is left (r = 1: the rates themselves)
    const double u0 = exp(-lhr), v0 = exp(-lar);
    // the tau coefficients of the FINAL cells (0,0), (0,1), (1,0), (1,1) with the FULL-MATCH rates (c as in dcl::ll_at)
    const double c00 = rho * -(lh * la), c01 = rho * lh, c10 = rho * la, c11 = rho * -1.0;
    const double t00 = fmax(1.0 + c00, 0.0), t01 = fmax(1.0 + c01, 0.0);
    const double t10 = fmax(1.0 + c10, 0.0), t11 = fmax(1.0 + c11, 0.0);
    // Z: the tau cells at or beyond (a, b), each (f - 1) u_(x-a) v_(y-b); hx0 is u_(0-a), hx1 is u_(1-a) (0 if behind a)
    const double u1 = u0 * lhr, v1 = v0 * lar;
    const double hx0 = a == 0 ? u0 : 0.0, hx1 = a == 0 ? u1 : (a == 1 ? u0 : 0.0);
    const double hy0 = b == 0 ? v0 : 0.0, hy1 = b == 0 ? v1 : (b == 1 ? v0 : 0.0);
    const double Z = 1.0 + (((fmax(c00, -1.0) * (hx0 * hy0) + fmax(c01, -1.0) * (hx0 * hy1)) +
                             fmax(c10, -1.0) * (hx1 * hy0)) + fmax(c11, -1.0) * (hx1 * hy1));
    const double rz = 1.0 / Z;
    if (pass == 0) {
        // log Pois(a; lh t) + log Pois(b; la t) + log Z; a count of 0 takes no logarithm (t = 0 comes with 0-0)
        const double lt = log(t);
        const double pa = (a > 0 ? (double)a * (eh + lt) : 0.0) - lh * t - A.lgf[a];
        const double pb = (b > 0 ? (double)b * (ea + lt) : 0.0) - la * t - A.lgf[b];
        A.lev[(size_t)f * (size_t)S + (size_t)s] = (pa + pb) + log(Z);
    }
    const size_t row = (size_t)(G + 1) * INPLAY_KPASS;
    const double* __restrict__ wp = A.w + (size_t)pass * (size_t)(G + 1) * row;
    double acc[INPLAY_KPASS];
#pragma unroll
    for (int k = 0; k < INPLAY_KPASS; ++k) acc[k] = 0.0;
    double vy = v0;   // Pois(y0 - b; la r) of the block's first count
#pragma unroll 1
    for (int y0 = b; y0 <= G; y0 += INPLAY_YB) {
        const int j0 = y0 - b;   // the block's first remaining-goal count
        double v[INPLAY_YB];
        v[0] = j0 == 0 ? v0 : vy * (lar * A.rk[j0]);
#pragma unroll
        for (int j = 1; j < INPLAY_YB; ++j) v[j] = y0 + j <= G ? v[j - 1] * (lar * A.rk[j0 + j]) : 0.0;
        vy = v[INPLAY_YB - 1];
        const int nj = G - y0 + 1 < INPLAY_YB ? G - y0 + 1 : INPLAY_YB;   // (uniform)
        double u = u0;
#pragma unroll 1
        for (int x = a; x <= G; ++x) {
            if (x > a) u = u * (lhr * A.rk[x - a]);
            const double* __restrict__ wc = wp + (size_t)x * row + (size_t)y0 * INPLAY_KPASS;
            if (y0 <= 1 && x <= 1) {
                // the block with tau cells (y0 = b <= 1): the FINAL columns 0 and 1 carry their factor
                const double f0 = x == 0 ? t00 : t10, f1 = x == 0 ? t01 : t11;
#pragma unroll
                for (int j = 0; j < INPLAY_YB; ++j) {
                    if (j < nj) {
                        double p = u * v[j];
                        if (y0 + j == 0) p = f0 * p;
                        if (y0 + j == 1) p = f1 * p;
#pragma unroll
                        for (int k = 0; k < INPLAY_KPASS; ++k) acc[k] = fma(wc[j * INPLAY_KPASS + k], p, acc[k]);
                    }
                }
            } else if (nj == INPLAY_YB) {
#pragma unroll
                for (int j = 0; j < INPLAY_YB; ++j) {
                    const double p = u * v[j];
#pragma unroll
                    for (int k = 0; k < INPLAY_KPASS; ++k) acc[k] = fma(wc[j * INPLAY_KPASS + k], p, acc[k]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < INPLAY_YB; ++j) {
                    if (j < nj) {
                        const double p = u * v[j];
#pragma unroll
                        for (int k = 0; k < INPLAY_KPASS; ++k) acc[k] = fma(wc[j * INPLAY_KPASS + k], p, acc[k]);
                    }
                }
            }
        }
    }
    const int k0 = pass * INPLAY_KPASS;
    double* out = A.vals + ((size_t)f * (size_t)A.K + (size_t)k0) * (size_t)S + (size_t)s;
#pragma unroll
    for (int k = 0; k < INPLAY_KPASS; ++k)
        if (k0 + k < A.K) out[(size_t)k * (size_t)S] = acc[k] * rz + 0.0;   // (+ 0.0: never -0)
}

// the workgroup's maximum (commutative: any order gives the same bits); red: [INPLAY_WAVES] LDS
__device__ __forceinline__ double block_max(double v, double* red) {
    v = dcl::wave_max(v);
    __syncthreads();   // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// grid: nc * K workgroups, workgroup -> (fixture of the chunk, market); dynamic LDS: inplay_summary_lds_bytes(S).
// It reads stored values only; VENUE names the rate form of the entry that launched it (as dcm::market_summary)
template <bool VENUE>
__global__ __launch_bounds__(INPLAY_THREADS) void inplay_summary(InplayArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ uint32_t hist[INPLAY_WAVES * 256];
    __shared__ uint32_t wtot[INPLAY_WAVES];
    __shared__ double red[INPLAY_WAVES];
    __shared__ double tot[INPLAY_THREADS];   // the segment totals of the scan
    const int tid = threadIdx.x;
    const long long item = blockIdx.x;
    if (item >= A.nc * (long long)A.K) return;   // (workgroup uniform)
    const long long f = item / A.K;
    const int k = (int)(item - f * A.K);
    const int S = A.P.S;
    const size_t M = (size_t)A.Q.M, n = (size_t)(A.n0 + f);
    const double* __restrict__ v = A.vals + (size_t)item * (size_t)S;
    const double* __restrict__ lev = A.lev + (size_t)f * (size_t)S;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(dyn);
    double* om = reinterpret_cast<double*>(dyn);   // the weights, over the keys once the order is known
    uint16_t* ia = reinterpret_cast<uint16_t*>(dyn + (size_t)S * 8);
    uint16_t* ib = ia + S;

    // L[s] = (l if reweight) + (log weight if given), its maximum, and the keys
    double lmax = -INFINITY;
    for (int s = tid; s < S; s += INPLAY_THREADS) {
        const double L = (A.reweight ? lev[s] : 0.0) + (A.lw ? A.lw[s] : 0.0);
        lmax = fmax(lmax, L);
        key[s] = dcl::key_of(v[s]);
        ia[s] = (uint16_t)s;
    }
    lmax = block_max(lmax, red);
    if (A.NQ > 0) dcg::radix_sort(key, ia, ib, S, hist, wtot);   // (ia: the order, ties by draw)
    __syncthreads();
    for (int s = tid; s < S; s += INPLAY_THREADS) {
        const double L = (A.reweight ? lev[s] : 0.0) + (A.lw ? A.lw[s] : 0.0);
        om[s] = exp(L - lmax);
    }
    __syncthreads();

    // mean and sd: two passes, per thread sequential over s = tid, tid + 256, ..., then dcg::block_sum
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int s = tid; s < S; s += INPLAY_THREADS) {
        const double o = om[s];
        s0 += o;
        s1 = fma(o, v[s], s1);
        s2 = fma(o, o, s2);
    }
    const double sw = dcg::block_sum(s0, red);
    const double mean = dcg::block_sum(s1, red) / sw;
    const double sww = dcg::block_sum(s2, red);
    double sq = 0.0;
    for (int s = tid; s < S; s += INPLAY_THREADS) {
        const double d = v[s] - mean;
        sq = fma(om[s], d * d, sq);
    }
    sq = dcg::block_sum(sq, red);
    if (tid == 0) {
        A.mean[(size_t)k * M + n] = mean;
        A.sd[(size_t)k * M + n] = sqrt(sq / sw);
    }

    if (A.NQ > 0) {
        // the scan C of the weights in sorted order: thread i owns positions i per .. (i + 1) per - 1
        const int per = (S + INPLAY_THREADS - 1) / INPLAY_THREADS;
        const int lo = min(tid * per, S), hi = min(lo + per, S);
        double part = 0.0;
        for (int i = lo; i < hi; ++i) part += om[ia[i]];
        tot[tid] = part;
        __syncthreads();
        double before = 0.0, W = 0.0;   // C just before this segment; the scan's last element
        for (int i = 0; i < INPLAY_THREADS; ++i) {
            if (i == tid) before = W;
            W += tot[i];
        }
        const double after = before + part;   // (= the scan at this segment's last position)
        for (int iq = 0; iq < A.NQ; ++iq) {
            const double qq = A.q[iq];
            int at = -1;
            if (qq >= 1.0) {
                if (hi == S && lo < hi) at = S - 1;   // q = 1: the maximum, whatever the last weights are
            } else {
                const double target = qq * W;
                // the first position with C >= target is here iff C before the segment is below it (or nothing
                // is before) and C at the segment's end reaches it
                if (lo < hi && (lo == 0 || before < target) && after >= target) {
                    double p = 0.0;   // (C_i = before + the segment's own partial sum: C at the end is `after`)
                    for (int i = lo; i < hi; ++i) {
                        p += om[ia[i]];
                        if (before + p >= target) {
                            at = i;
                            break;
                        }
                    }
                }
            }
            if (at >= 0) A.quant[((size_t)k * (size_t)A.NQ + (size_t)iq) * M + n] = v[ia[at]];
        }
    }

    if (k == 0) {
        // per fixture: ess of the weights; the log evidence from l alone, whatever the weights are
        double m = -INFINITY;
        for (int s = tid; s < S; s += INPLAY_THREADS) m = fmax(m, lev[s]);
        m = block_max(m, red);
        double e = 0.0;
        for (int s = tid; s < S; s += INPLAY_THREADS) e += exp(lev[s] - m);
        e = dcg::block_sum(e, red);
        if (tid == 0) {
            A.ess[n] = sw * sw / sww;
            A.logev[n] = m + log(e / (double)S);
        }
    }
}

}  // namespace dcip
