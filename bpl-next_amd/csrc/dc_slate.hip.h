// dc_slate.hip.h -- the total of several fixtures' legs on the device: accumulators, points totals, counts of
// home wins.  A leg gives every final score (x, y) of its fixture an integer 0..SLATE_VALUES-1; a slate is a list
// of fixtures, and its total is T = sum_i leg_i.  The fixtures share the posterior, so E_draw[prod p_i] is not
// prod E_draw[p_i]: the law of T is formed PER DRAW and only then summarised.  Given one draw the fixtures are
// independent, so that law is exact, a convolution, with no Monte Carlo.  Per posterior draw s:
//     r_i[v]   = sum_{(x, y): leg_i(x, y) = v} q_s(x, y)       q as in dc_market.hip.h (not renormalised)
//     pmf_s    = r_1 * r_2 * ... * r_N                          in list order, t = 0..P
//     at_least[t] = sum_{u >= t} pmf[u] (from the top down),  expected = sum_t t pmf[t] (t ascending),
//     mass     = at_least[0] = prod_i (grid mass of fixture i)
// One kernel, slate_values: lane = draw, ONE WAVE per workgroup, grid (slate of the chunk, 64-draw tile).  The wave
// walks its slate's fixtures in list order.  Per fixture the rank-one walk of dcm::market_values (two Poisson
// recurrences, the four tau cells clipped to an exact 0), where each cell's probability goes into one of
// SLATE_VALUES per-lane accumulators: the leg's table is wave-uniform, eight cells to a 64-bit word read through
// uniform loads, and cell k's "weight" is the uniform (value == k ? 1.0 : 0.0) in an explicit fma, so the
// accumulators stay in registers under static indices (fma(1, t, a) = a + t and fma(0, t, a) = a exactly).  The
// running pmf lives in dynamic LDS as [t][lane] float64 (512 B per t: consecutive lanes, conflict-free 64-bit
// accesses), updated in place with t descending up to the running top: new[t] = sum_v r_v old[t - v], v
// ascending.  A lane reads and writes its own column only, so nothing crosses lanes: no barrier and no fence.
// The statistics go to vals[slate of the chunk][2 (P+1) + 2][S] (pmf, at_least, expected, mass) and the fixture's
// value law to leg_vals[fixture of the chunk][SLATE_VALUES][S], draws contiguous: both are summarised by
// dcm::market_summary.  No floating-point atomics; every sum has a fixed order that depends on nothing but the
// slate's own fixtures: results are bit-identical from run to run, under any chunking of the slates and under
// any reordering that keeps each slate's own order.  Contraction is off and every fma is explicit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"   // dcl::Fix, fix_rows, log_rates_at

namespace dcsl {

constexpr int SLATE_MAX_GOALS = 63;     // dcm::MARKET_MAX_GOALS
constexpr int SLATE_VALUES = 8;         // a leg's values are 0..7: include/bplhip.h BPLHIP_SLATE_VALUES
constexpr int SLATE_MAX_TOTAL = 127;    // include/bplhip.h BPLHIP_SLATE_MAX_TOTAL: (127 + 1) 512 B = 64 KB of LDS
constexpr int SLATE_MAX_LEGS = 1024;    // include/bplhip.h BPLHIP_SLATE_MAX_LEGS
constexpr int SLATE_YB = 8;             // away counts per block: one 64-bit word of the leg's table

struct SlateArgs {
    dcq::Posterior<double> P;   // TEAM-major
    dcq::Queries Q;             // the fixtures (no goals), each slate's contiguous and in list order
    int G, PT;                  // PT = P + 1, the rows of the pmf: the call's largest total plus one
    long long j0, jc;           // the chunk: slates j0 .. j0 + jc - 1
    const int32_t* start;       // [J + 1]: slate j holds the fixtures start[j] .. start[j + 1] - 1
    const int32_t* table;       // [M] the fixture's leg table
    const int32_t* top;         // [tables] the table's largest value m
    const uint64_t* cells;      // [tables][G + 1][ceil((G + 1) / SLATE_YB)]: byte j of word (x, b) is cell (x, 8 b + j); 0 past G
    double* vals;               // [jc, 2 PT + 2, S]
    double* leg_vals;           // [fixtures of the chunk, SLATE_VALUES, S]
    double rk[SLATE_MAX_GOALS + 1];   // rk[k] = 1 / k (k >= 1)
};

// grid: (slate of the chunk, draw tile); dynamic LDS: PT * 64 * 8 bytes
template <bool VENUE>
__global__ __launch_bounds__(64) void slate_values(SlateArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double pmf_lds[];
    const int lane = threadIdx.x;
    const int S = A.P.S, G = A.G;
    const int s = blockIdx.y * 64 + lane;
    if (s >= S) return;   // (no barrier below)
    const long long j = A.j0 + blockIdx.x;
    const int f_begin = A.start[j], f_end = A.start[j + 1], f_chunk = A.start[A.j0];
    const int yblocks = (G + SLATE_YB) / SLATE_YB;
    double* pmf = pmf_lds + lane;   // pmf[64 t]: this lane's column
    pmf[0] = 1.0;
    int top = 0;   // the running largest total (uniform)
#pragma unroll 1
    for (int f = f_begin; f < f_end; ++f) {
        const dcl::Fix F = dcl::fix_rows<VENUE>(A.P, A.Q, f);
        double eh, ea;
        dcl::log_rates_at<VENUE>(F, s, &eh, &ea);
        const double rho = F.corr[s];
        const double lh = exp(eh), la = exp(ea);
        const double u0 = exp(-lh), v0 = exp(-la);
        // the tau factors of (0,0), (0,1), (1,0), (1,1) (c as in dcl::ll_at)
        const double t00 = fmax(1.0 + rho * -(lh * la), 0.0), t01 = fmax(1.0 + rho * lh, 0.0);
        const double t10 = fmax(1.0 + rho * la, 0.0), t11 = fmax(1.0 + rho * -1.0, 0.0);
        const int tab = A.table[f];
        const int m = A.top[tab];
        const uint64_t* __restrict__ cp = A.cells + (size_t)tab * (size_t)(G + 1) * (size_t)yblocks;
        double r[SLATE_VALUES];
#pragma unroll
        for (int k = 0; k < SLATE_VALUES; ++k) r[k] = 0.0;
        double vy = v0;   // Pois(y0; la) of the block's first count
#pragma unroll 1
        for (int b = 0; b < yblocks; ++b) {
            const int y0 = b * SLATE_YB;
            double v[SLATE_YB];
            v[0] = y0 == 0 ? v0 : vy * (la * A.rk[y0]);
#pragma unroll
            for (int jj = 1; jj < SLATE_YB; ++jj) v[jj] = y0 + jj <= G ? v[jj - 1] * (la * A.rk[y0 + jj]) : 0.0;
            vy = v[SLATE_YB - 1];
            double u = u0;
#pragma unroll 1
            for (int x = 0; x <= G; ++x) {
                if (x > 0) u = u * (lh * A.rk[x]);
                const uint64_t word = cp[(size_t)x * (size_t)yblocks + (size_t)b];   // (uniform)
                // a count past G has v = 0 and the value 0: it adds an exact 0 to r[0]
                const bool tau = y0 == 0 && x <= 1;
                const double f0 = x == 0 ? t00 : t10, f1 = x == 0 ? t01 : t11;
#pragma unroll
                for (int jj = 0; jj < SLATE_YB; ++jj) {
                    double t = u * v[jj];
                    if (jj == 0 && tau) t = f0 * t;
                    if (jj == 1 && tau) t = f1 * t;
                    const int val = (int)((word >> (8 * jj)) & 0xFFu);
#pragma unroll
                    for (int k = 0; k < SLATE_VALUES; ++k) r[k] = fma(val == k ? 1.0 : 0.0, t, r[k]);
                }
            }
        }
        double* out = A.leg_vals + (size_t)(f - f_chunk) * (size_t)SLATE_VALUES * (size_t)S + (size_t)s;
#pragma unroll
        for (int k = 0; k < SLATE_VALUES; ++k) out[(size_t)k * (size_t)S] = r[k] + 0.0;   // (+ 0.0: never -0)
        // the convolution, in place: row t is written after the rows t - v it reads, all of them below it
#pragma unroll 1
        for (int t = top + m; t >= 0; --t) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < SLATE_VALUES; ++k)
                if (k <= m && t - k >= 0 && t - k <= top) acc = fma(r[k], pmf[64 * (t - k)], acc);   // (uniform)
            pmf[64 * t] = acc;
        }
        top += m;
    }
    const int PT = A.PT;
    double* out = A.vals + (size_t)blockIdx.x * (size_t)(2 * PT + 2) * (size_t)S + (size_t)s;
    double al = 0.0;
#pragma unroll 1
    for (int t = PT - 1; t >= 0; --t) {
        const double p = t <= top ? pmf[64 * t] : 0.0;
        al = al + p;
        out[(size_t)t * (size_t)S] = p + 0.0;
        out[(size_t)(PT + t) * (size_t)S] = al + 0.0;
    }
    double e = 0.0;
#pragma unroll 1
    for (int t = 0; t <= top; ++t) e = fma((double)t, pmf[64 * t], e);
    out[(size_t)(2 * PT) * (size_t)S] = e + 0.0;
    out[(size_t)(2 * PT + 1) * (size_t)S] = al + 0.0;
}

}  // namespace dcsl
