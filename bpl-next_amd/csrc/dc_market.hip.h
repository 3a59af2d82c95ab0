// dc_market.hip.h -- match markets of a fitted model on the device: every market is a linear functional of
// one draw's scoreline grid, formed PER DRAW and then summarised over the draws (a quantile of a sum is not
// a sum of quantiles).  Per posterior draw s, fixture n and market k with float64 weights W_k[x, y]:
//     v[s, k, n] = sum_{x, y <= G} W_k[x, y] q(x, y)
//     q(x, y)    = max(1 + rho_s c(x, y), 0) Pois(x; lh) Pois(y; la)       (not renormalised)
// with the rates of dcl::log_rates_at and the tau coefficient c of dcl::ll_at: dc_score.hip.h is the special
// case where W is the three triangles.  Per (k, n), over the S draws: mean, sd (ddof = 1; 0 for one draw) and
// linearly interpolated quantiles of EXACT order statistics.  Everything in float64.
//
// Two kernels:
//   market_values   lane = draw on the team-major tables; the four waves of a workgroup share one fixture and
//       one pass of MARKET_KPASS markets and take neighbouring draw tiles, so the row pointers and the weights
//       are wave-uniform.  A draw's grid is rank one, u_x v_y, apart from the four tau cells.  The walk goes
//       over blocks of MARKET_YB away counts: the block's v_y (Poisson recurrence, 1 / k from a table in the
//       kernel arguments) are held in registers while x walks 0..G with its own recurrence, so a cell costs one
//       multiplication (u_x v_y) and one fma per market, plus 2 / MARKET_YB multiplications for the
//       recurrences.  The weights are read through wave-uniform loads from a [pass][cell][MARKET_KPASS]
//       copy (a cell's MARKET_KPASS weights are contiguous; the tail of the last pass holds zeros).  Nothing
//       per draw is kept but the MARKET_KPASS accumulators.  The four low cells carry their own
//       max(1 + rho c, 0): a clipped cell contributes an exact 0, as in dcs::outcome_probs.  Registers only:
//       no LDS, no scratch, no barrier.  The values go to vals[fixture of the chunk][k][s], draws contiguous.
//   market_summary  ONE WAVE PER (fixture, market) over the S stored values: mean and sd from a two-pass sum
//       (per-lane sequential over a fixed draw order, then xor butterflies), then per quantile q with
//       h = q (S - 1) the order statistic v_(floor h) by radix selection on the order-preserving 64-bit key
//       of a float64, 8 bits per pass, as dcl::loglik_summary does (per-wave LDS histogram with integer LDS
//       atomics, a lane suffix scan; the first digit's histogram is built once per (fixture, market)); when h
//       has a fraction, v_(floor h + 1) is the least value above v_(floor h) unless v_(floor h) is repeated
//       past that rank (one more pass), and the result is v_lo + (h - floor h) (v_hi - v_lo).
// No floating-point atomics; every sum has a fixed order and a value's accumulation order depends on nothing
// but its own (draw, fixture, market): results are bit-identical from run to run, under any chunking of the
// fixtures and under any order of the fixtures.  Contraction is off and every fma is explicit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"   // dcl::Fix, fix_rows, log_rates_at, wave_sum, key_of, wave_lds_order

namespace dcm {

constexpr int MARKET_MAX_GOALS = 63;      // dcs::SCORE_MAX_GOALS
constexpr int MARKET_MAX_MARKETS = 64;    // include/bplhip.h BPLHIP_MARKET_MAX_MARKETS
constexpr int MARKET_MAX_QUANTILES = 16;  // include/bplhip.h BPLHIP_MARKET_MAX_QUANTILES
constexpr int MARKET_KPASS = 8;           // markets per pass: 8 accumulators + 8 block values = 32 of the 70 VGPRs
constexpr int MARKET_YB = 8;              // away counts per block
constexpr int MARKET_WAVES = 4;

struct MarketArgs {
    dcq::Posterior<double> P;   // TEAM-major
    dcq::Queries Q;             // the fixtures (no goals)
    int G, K, NQ;
    long long n0, nc;           // the chunk: fixtures n0 .. n0 + nc - 1
    const double* w;            // [ceil(K / MARKET_KPASS)][(G+1)^2][MARKET_KPASS]
    const double* q;            // [NQ]
    double* vals;               // [nc, K, S]
    double* mean;               // [K, M]
    double* sd;                 // [K, M]
    double* quant;              // [K, NQ, M]
    double rk[MARKET_MAX_GOALS + 1];   // rk[k] = 1 / k (k >= 1)
};

// grid: (fixture of the chunk, draw tile group, pass)
template <bool VENUE>
__global__ __launch_bounds__(64 * MARKET_WAVES) void market_values(MarketArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = A.P.S, G = A.G;
    const int s = (blockIdx.y * MARKET_WAVES + wave) * 64 + lane;
    const long long f = blockIdx.x;
    const int pass = blockIdx.z;
    if (s >= S) return;   // (no barrier below)
    const dcl::Fix F = dcl::fix_rows<VENUE>(A.P, A.Q, A.n0 + f);
    double eh, ea;
    dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
    const double rho = F.corr[s];
    const double lh = exp(eh), la = exp(ea);
    const double u0 = exp(-lh), v0 = exp(-la);
    // the tau factors of (0,0), (0,1), (1,0), (1,1) (c as in dcl::ll_at)
    const double t00 = fmax(1.0 + rho * -(lh * la), 0.0), t01 = fmax(1.0 + rho * lh, 0.0);
    const double t10 = fmax(1.0 + rho * la, 0.0), t11 = fmax(1.0 + rho * -1.0, 0.0);
    const size_t row = (size_t)(G + 1) * MARKET_KPASS;
    const double* __restrict__ wp = A.w + (size_t)pass * (size_t)(G + 1) * row;
    double acc[MARKET_KPASS];
#pragma unroll
    for (int k = 0; k < MARKET_KPASS; ++k) acc[k] = 0.0;
    double vy = v0;   // Pois(y0; la) of the block's first count
#pragma unroll 1
    for (int y0 = 0; y0 <= G; y0 += MARKET_YB) {
        double v[MARKET_YB];
        v[0] = y0 == 0 ? v0 : vy * (la * A.rk[y0]);
#pragma unroll
        for (int j = 1; j < MARKET_YB; ++j) v[j] = y0 + j <= G ? v[j - 1] * (la * A.rk[y0 + j]) : 0.0;
        vy = v[MARKET_YB - 1];
        const int nj = G - y0 + 1 < MARKET_YB ? G - y0 + 1 : MARKET_YB;   // (uniform)
        double u = u0;
#pragma unroll 1
        for (int x = 0; x <= G; ++x) {
            if (x > 0) u = u * (lh * A.rk[x]);
            const double* __restrict__ wc = wp + (size_t)x * row + (size_t)y0 * MARKET_KPASS;
            if (y0 == 0 && x <= 1) {
                // the block with the tau cells: columns 0 and 1 carry their factor
                const double f0 = x == 0 ? t00 : t10, f1 = x == 0 ? t01 : t11;
#pragma unroll
                for (int j = 0; j < MARKET_YB; ++j) {
                    if (j < nj) {
                        double t = u * v[j];
                        if (j == 0) t = f0 * t;
                        if (j == 1) t = f1 * t;
#pragma unroll
                        for (int k = 0; k < MARKET_KPASS; ++k) acc[k] = fma(wc[j * MARKET_KPASS + k], t, acc[k]);
                    }
                }
            } else if (nj == MARKET_YB) {
#pragma unroll
                for (int j = 0; j < MARKET_YB; ++j) {
                    const double t = u * v[j];
#pragma unroll
                    for (int k = 0; k < MARKET_KPASS; ++k) acc[k] = fma(wc[j * MARKET_KPASS + k], t, acc[k]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < MARKET_YB; ++j) {
                    if (j < nj) {
                        const double t = u * v[j];
#pragma unroll
                        for (int k = 0; k < MARKET_KPASS; ++k) acc[k] = fma(wc[j * MARKET_KPASS + k], t, acc[k]);
                    }
                }
            }
        }
    }
    const int k0 = pass * MARKET_KPASS;
    double* out = A.vals + ((size_t)f * (size_t)A.K + (size_t)k0) * (size_t)S + (size_t)s;
#pragma unroll
    for (int k = 0; k < MARKET_KPASS; ++k)
        if (k0 + k < A.K) out[(size_t)k * (size_t)S] = acc[k] + 0.0;   // (+ 0.0: never -0)
}

__device__ __forceinline__ double value_of(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)u);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}

// the digit of the histogram `hw` that holds the r-th largest candidate: (bin, rank left inside it, its count)
__device__ __forceinline__ void pick_digit(const uint32_t* hw, int lane, uint32_t r, int* bin_out, uint32_t* r_out,
                                           uint32_t* cnt_out) {
    uint32_t c[4];
    for (int b = 0; b < 4; ++b) c[b] = hw[4 * lane + b];
    const uint32_t own = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = own;   // candidates in this lane's bins and every higher bin
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_down(incl, o);
        if (lane + o < 64) incl += t;
    }
    const uint32_t excl = incl - own;
    const unsigned long long hit = __ballot(excl < r && r <= incl);
    const int src = hit ? __ffsll((long long)hit) - 1 : 0;   // (always one lane: the candidates hold rank r)
    int bin = 0;
    uint32_t rr = 0, cnt = 0;
    if (lane == src) {
        uint32_t acc = excl;
        for (int b = 3; b >= 0; --b) {
            if (acc + c[b] >= r) {
                bin = 4 * lane + b;
                rr = r - acc;
                cnt = c[b];
                break;
            }
            acc += c[b];
        }
    }
    *bin_out = __shfl(bin, src);
    *r_out = __shfl(rr, src);
    *cnt_out = __shfl(cnt, src);
}

// grid: ceil(nc * K / MARKET_WAVES) workgroups; wave -> (fixture of the chunk, market).  It reads stored values
// only; VENUE names the rate form of the entry that launched it, so that a kernel trace tells the two apart
template <bool VENUE>
__global__ __launch_bounds__(64 * MARKET_WAVES) void market_summary(MarketArgs A) {
#pragma clang fp contract(off)
    __shared__ uint32_t hist0[MARKET_WAVES][256];   // the first digit of all S values
    __shared__ uint32_t hist[MARKET_WAVES][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long item = (long long)blockIdx.x * MARKET_WAVES + w;
    if (item >= A.nc * (long long)A.K) return;   // (wave uniform; no workgroup barrier below)
    const long long f = item / A.K;
    const int k = (int)(item - f * A.K);
    const int S = A.P.S;
    const size_t M = (size_t)A.Q.M, n = (size_t)(A.n0 + f);
    const double* __restrict__ v = A.vals + (size_t)item * (size_t)S;
    uint32_t* h0 = hist0[w];
    uint32_t* hw = hist[w];

    for (int i = lane; i < 256; i += 64) h0[i] = 0u;
    dcl::wave_lds_order();
    double sm = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double x = v[s];
        sm += x;
        if (A.NQ > 0) atomicAdd(&h0[dcl::key_of(x) >> 56], 1u);
    }
    const double mean = dcl::wave_sum(sm) / (double)S;
    double sq = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double d = v[s] - mean;
        sq = fma(d, d, sq);
    }
    sq = dcl::wave_sum(sq);
    if (lane == 0) {
        A.mean[(size_t)k * M + n] = mean;
        A.sd[(size_t)k * M + n] = S > 1 ? sqrt(sq / (double)(S - 1)) : 0.0;
    }

    for (int iq = 0; iq < A.NQ; ++iq) {
        const double h = A.q[iq] * (double)(S - 1);
        const double fl = floor(h);
        const int lo = (int)fl;
        const double frac = h - fl;
        // v_(lo), 0-based from the least: the (S - lo)-th largest key.  `prefix` holds the digits found, `r` the
        // rank left in its bucket
        unsigned long long prefix = 0;
        int shift = 56;
        uint32_t r = (uint32_t)(S - lo), cnt;
        const uint32_t* src = h0;
        for (;;) {
            dcl::wave_lds_order();
            int bin;
            pick_digit(src, lane, r, &bin, &r, &cnt);
            prefix = (prefix << 8) | (unsigned long long)bin;
            if (cnt == 1u || shift == 0) break;
            shift -= 8;
            dcl::wave_lds_order();
            for (int i = lane; i < 256; i += 64) hw[i] = 0u;
            dcl::wave_lds_order();
            for (int s = lane; s < S; s += 64) {
                const unsigned long long key = dcl::key_of(v[s]);
                if ((key >> (shift + 8)) == prefix) atomicAdd(&hw[(key >> shift) & 255u], 1u);
            }
            src = hw;
        }
        unsigned long long klo = prefix;
        if (shift > 0) {
            // one value left in the bucket: read it off
            unsigned long long found = 0;
            for (int s = lane; s < S; s += 64) {
                const unsigned long long key = dcl::key_of(v[s]);
                if ((key >> shift) == prefix) found = key;
            }
            klo = wave_max_u64(found);
        }
        const double vlo = value_of(klo);
        double res = vlo;
        if (frac > 0.0 && lo + 1 < S) {
            // v_(lo + 1): v_(lo) again when it is repeated past rank lo, else the least value above it
            uint32_t le = 0;
            unsigned long long above = ~0ull;
            for (int s = lane; s < S; s += 64) {
                const unsigned long long key = dcl::key_of(v[s]);
                if (key <= klo) ++le;
                else above = key < above ? key : above;
            }
            for (int o = 32; o > 0; o >>= 1) {
                le += __shfl_xor(le, o);
                const unsigned long long t = __shfl_xor(above, o);
                above = t < above ? t : above;
            }
            const double vhi = le > (uint32_t)(lo + 1) ? vlo : value_of(above);
            res = vlo + frac * (vhi - vlo);
        }
        if (lane == 0) A.quant[((size_t)k * (size_t)A.NQ + (size_t)iq) * M + n] = res;
    }
}

}  // namespace dcm
