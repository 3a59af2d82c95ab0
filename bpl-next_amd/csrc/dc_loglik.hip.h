// dc_loglik.hip.h -- pointwise log-likelihood of a fitted model on the device: one value per
// (posterior draw s, fixture n), and the per-fixture summaries WAIC and PSIS-LOO are built from.
//     ll = x log lh - lh - lgamma(x+1) + y log la - la - lgamma(y+1) + [x <= 1, y <= 1] log(max(1 + rho_s c(x,y), 0))
// with the two rate forms of dc_predict.hip.h (template VENUE; log lh, log la are the exponents
// themselves) and the tau coefficient c of dcp::predict_score_proba, so that exp(ll) averaged over
// the draws is predict_score_proba.  A clipped tau gives -inf, never NaN.  Everything in float64.
//
// The posterior is read from TEAM-MAJOR float64 copies ([T][S]: a team's draws contiguous) that the
// host entry builds lazily, with `transpose_f64`, on the first log-likelihood call after an upload:
// lane = draw loads are then coalesced.
//
// Three kernels:
//   transpose_f64   [rows, cols] -> [cols, rows] through a 32 x 33 LDS tile.
//   loglik_matrix   ll as [S, M] float64.  A workgroup owns 64 draws x 64 fixtures: each wave works
//       16 fixtures with lane = draw into an LDS tile [fixture][draw] (row stride 65 doubles), then
//       the workgroup stores the tile row by row (lane = fixture): coalesced on both sides.
//   loglik_summary  ONE WAVE PER FIXTURE; the matrix is never stored.  Passes over the draws, each
//       recomputing ll (two exp per draw, no log outside the four low scorelines):
//         1  max, min and sum of ll (and whether some ll is -inf)
//         2  sum exp(ll - max) (-> lppd), sum (ll - mean)^2 (-> var, 1/(S-1)); with PSIS the first
//            digit histogram of the selection below
//       With PSIS (x = min ll - ll = r - max r for r = -ll, x <= 0):
//         3..  radix selection of the (M+1)-th largest x on the order-preserving 64-bit key of the
//            float64, 8 bits per pass: a per-wave LDS histogram (integer LDS atomics) of the
//            candidates' next digit, a lane suffix scan to find the digit holding the target rank.
//            It stops as soon as that digit's bucket holds one draw (usually after 2 or 3 digits)
//         g  gather: the draws above the target's bucket (at most M <= LOGLIK_MAX_TAIL) go to LDS as
//            (key, draw) by ballot compaction in draw order, and the cutoff x_(S-M) is read off
//            the bucket's own draw.  Only this set is sorted (bitonic, in LDS, by (key, draw))
//         -  the Zhang-Stephens GPD fit of the tail with lane = grid point j (m = 30 + floor(sqrt L)
//            <= 62 points), Pareto smoothing of the tail by rank
//         f  lse(x) and lse(x + ll) over the draws: non-tail draws from a last pass, tail draws from
//            their smoothed values and a recomputed ll; elpd_loo = lse(x + ll) - lse(x)
//       Reductions are per-lane sequential over a fixed draw order, then xor butterflies of
//       commutative operations: results are bit-identical from run to run.
//       ll is evaluated with floating-point contraction off, so every pass computes bit-identical
//       values for a draw (the tail test x > cutoff of the last pass repeats that of the gather).
//       The selection, gather, sort and fit are the device function psis_tail, templated on where a draw's
//       x comes from: dc_sequential.hip.h runs the same lines on rows read from memory.
//   LDS: 4 waves x (8 KB keys + 2 KB draw indices + 1 KB histogram) ~ 44 KB per workgroup; no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_posterior.hip.h"   // dcq::Posterior, the log-rate forms
#include "dc_sampler.hip.h"     // dcr::wave_lds_order (nothing else of it is used here)

namespace dcl {
using dcr::wave_lds_order;

constexpr int LOGLIK_MAX_DRAWS = 65536;   // include/bplhip.h BPLHIP_LOGLIK_MAX_DRAWS (draw index fits u16)
constexpr int LOGLIK_MAX_TAIL = 1024;     // include/bplhip.h BPLHIP_LOGLIK_MAX_TAIL
constexpr int SUM_WAVES = 4;

struct LoglikArgs {
    dcq::Posterior<double> P;   // TEAM-major
    dcq::Queries Q;             // the fixtures
    double* ll;               // loglik_matrix: [S, M]
    double* lppd;             // loglik_summary: [M] each
    double* mean;
    double* var;
    double* elpd_loo;         // with PSIS
    double* pareto_k;
    int32_t* tail_len;        // with PSIS: L, the number of draws in the smoothed tail
    int psis;
    int tail_m;               // M = min(ceil(min(0.2 S, 3 sqrt(S / r_eff))), S - 1), checked on the host
    double log_dbl_min;       // log(DBL_MIN), the floor of the cutoff
};

// one fixture's rows of the team-major tables and its constants
struct Fix {
    const double *ah, *aa, *dh, *da, *ha;
    const double *hat, *adf, *aat, *hdf, *ch, *ca;
    const double* corr;
    double on, xd, yd, lgx, lgy;
    int x, y;
};

// the rows alone, from one fixture's indices (dc_sequential.hip.h has them packed); the goals and their
// constants stay zero
template <bool VENUE>
__device__ __forceinline__ Fix fix_rows_of(const dcq::Posterior<double>& P, int h, int a, int neutral, int hc, int ac) {
    Fix F{};
    const size_t S = (size_t)P.S;
    F.ah = P.attack + h * S;
    F.aa = P.attack + a * S;
    F.dh = P.defence + h * S;
    F.da = P.defence + a * S;
    if constexpr (VENUE) {
        F.hat = P.home_attack + h * S;
        F.adf = P.away_defence + a * S;
        F.aat = P.away_attack + a * S;
        F.hdf = P.home_defence + h * S;
        F.on = neutral ? 0.0 : 1.0;
        if (P.conf) {
            F.ch = P.conf + hc * S;
            F.ca = P.conf + ac * S;
        }
    } else {
        F.ha = P.ha_stride ? P.home_adv + h * S : P.home_adv;
    }
    F.corr = P.corr;
    return F;
}
// ... of fixture n of a query (dc_score.hip.h takes them from here too)
template <bool VENUE>
__device__ __forceinline__ Fix fix_rows(const dcq::Posterior<double>& P, const dcq::Queries& Q, long long n) {
    if constexpr (VENUE) return fix_rows_of<VENUE>(P, Q.h[n], Q.a[n], Q.neutral[n], P.conf ? Q.hc[n] : 0, P.conf ? Q.ac[n] : 0);
    else return fix_rows_of<VENUE>(P, Q.h[n], Q.a[n], 0, 0, 0);
}

template <bool VENUE>
__device__ __forceinline__ Fix make_fix(const dcq::Posterior<double>& P, const dcq::Queries& Q, long long n) {
    Fix F = fix_rows<VENUE>(P, Q, n);
    F.x = Q.x[n];
    F.y = Q.y[n];
    F.xd = (double)F.x;
    F.yd = (double)F.y;
    F.lgx = lgamma(F.xd + 1.0);
    F.lgy = lgamma(F.yd + 1.0);
    return F;
}
template <bool VENUE>
__device__ __forceinline__ Fix make_fix(const LoglikArgs& A, long long n) {
    return make_fix<VENUE>(A.P, A.Q, n);
}

// the log rates of draw s (the product forms of dc_posterior.hip.h)
template <bool VENUE>
__device__ __forceinline__ void log_rates_at(const Fix& F, int s, double* eh, double* ea) {
#pragma clang fp contract(off)
    if constexpr (VENUE) {
        dcq::log_rates_venue_product_v(F.ah[s], F.da[s], F.on, F.hat[s], F.adf[s], F.aa[s], F.dh[s], F.aat[s], F.hdf[s],
                                       eh, ea);
        if (F.ch) dcq::add_confederations(F.ch[s] - F.ca[s], eh, ea);
    } else {
        dcq::log_rates_plain_v(F.ah[s], F.da[s], F.ha[s], F.aa[s], F.dh[s], eh, ea);
    }
}

// ll of draw s, left to right as written above (and as the numpy restatement evaluates it)
template <bool VENUE>
__device__ __forceinline__ double ll_at(const Fix& F, int s) {
#pragma clang fp contract(off)
    double eh, ea;
    log_rates_at<VENUE>(F, s, &eh, &ea);
    const double lh = exp(eh), la = exp(ea);
    double v = F.xd * eh - lh - F.lgx + F.yd * ea - la - F.lgy;
    if (F.x <= 1 && F.y <= 1) {
        const double c = F.x == 0 ? (F.y == 0 ? -(lh * la) : lh) : (F.y == 0 ? la : -1.0);
        v = v + log(fmax(1.0 + F.corr[s] * c, 0.0));
    }
    return v;
}

// ---- team-major copies
__global__ __launch_bounds__(256) void transpose_f64(const double* in, double* out, int rows, int cols) {
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < rows && c < cols) t[k][tx] = in[(size_t)r * cols + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < rows && c < cols) out[(size_t)c * rows + r] = t[tx][k];
    }
}

// ---- the matrix
template <bool VENUE>
__global__ __launch_bounds__(256) void loglik_matrix(LoglikArgs A) {
    __shared__ double tile[64][65];   // [fixture][draw]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s0 = blockIdx.y * 64;
    const long long n0 = (long long)blockIdx.x * 64;
    const int s = s0 + lane;
#pragma unroll 1
    for (int f = wave * 16; f < wave * 16 + 16; ++f) {
        const long long n = n0 + f;
        if (n < A.Q.M && s < A.P.S) {
            const Fix F = make_fix<VENUE>(A, n);
            tile[f][lane] = ll_at<VENUE>(F, s);
        }
    }
    __syncthreads();
    for (int r = wave; r < 64; r += 4) {
        const long long n = n0 + lane;
        if (s0 + r < A.P.S && n < A.Q.M) A.ll[(size_t)(s0 + r) * (size_t)A.Q.M + n] = tile[lane][r];
    }
}

// ---- the summary: wave helpers
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
// running log-sum-exp (m, s): lse = m + log(s)
__device__ __forceinline__ void lse_add(double& m, double& s, double t) {
    if (t > m) {
        s = s * exp(m - t) + 1.0;
        m = t;
    } else {
        s += exp(t - m);
    }
}
__device__ __forceinline__ double wave_lse(double m, double s) {
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        const double mm = fmax(m, m2);
        const double a = m == -INFINITY ? 0.0 : s * exp(m - mm), b = m2 == -INFINITY ? 0.0 : s2 * exp(m2 - mm);
        s = a + b;   // (commutative: both lanes of a pair get the same bits)
        m = mm;
    }
    return m == -INFINITY ? -INFINITY : m + log(s);
}
// order-preserving key of a float64 (x is never -0 here)
__device__ __forceinline__ unsigned long long key_of(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double x_of(double mn, double v) {
    return (mn - v) + 0.0;   // (+ 0.0: a -0 becomes +0)
}

// ---- PSIS of one wave's draws, shared by loglik_summary (x from ll_at) and dc_sequential.hip.h (x from a
// stored row): `xat(s)` gives x_s = r_s - max r (<= 0, never NaN, -0 excluded) and must return bit-identical
// values every time it is called for a draw.  On entry hw[256] holds the histogram of the first digit of
// key_of(x) over the draws.  Runs the selection, the gather, the sort and the fit described above; kw / iw
// (LOGLIK_MAX_TAIL entries each), hw and cut are this wave's LDS.  On return iw[base .. base + L) are the
// tail's draws in ascending (x, draw) order.
struct PsisTail {
    int L, base;            // tail length; the tail's first entry in iw
    double cutoff, ecut;    // max(x_(S-M), log DBL_MIN) and its exp
    double kk, sigma;       // the fit: kk = +inf when nothing is smoothed (L <= 4 or no usable fit)
};

template <class X>
__device__ __forceinline__ PsisTail psis_tail(X xat, int S, int tail_m, double log_dbl_min, int lane, uint32_t* hw,
                                              unsigned long long* kw, uint16_t* iw, double* cut) {
    PsisTail T;
    // selection of the (M+1)-th largest key: `prefix` holds the digits found, `r` the rank left in its bucket
    unsigned long long prefix = 0;
    int shift = 56;
    uint32_t r = (uint32_t)tail_m + 1u;
    for (;;) {
        wave_lds_order();
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
        bin = __shfl(bin, src);
        rr = __shfl(rr, src);
        cnt = __shfl(cnt, src);
        prefix = (prefix << 8) | (unsigned long long)bin;
        r = rr;
        if (cnt == 1u || shift == 0) break;
        shift -= 8;
        wave_lds_order();
        for (int i = lane; i < 256; i += 64) hw[i] = 0u;
        wave_lds_order();
        for (int s = lane; s < S; s += 64) {
            const unsigned long long k = key_of(xat(s));
            if ((k >> (shift + 8)) == prefix) atomicAdd(&hw[(k >> shift) & 255u], 1u);
        }
    }

    // gather the draws above the target's bucket; the bucket's own draw (or, all digits resolved, any
    // of its equal draws) gives the cutoff value
    const unsigned long long thr = shift == 0 ? prefix : (prefix << shift) | ((1ull << shift) - 1ull);
    int ng = 0;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        bool in = false;
        unsigned long long k = 0;
        if (s < S) {
            const double x = xat(s);
            k = key_of(x);
            in = k > thr;
            if ((k >> shift) == prefix) *cut = x;
        }
        const unsigned long long mask = __ballot(in);
        const int pos = ng + (int)__popcll(mask & ((1ull << lane) - 1ull));
        if (in && pos < LOGLIK_MAX_TAIL) {
            kw[pos] = k;
            iw[pos] = (uint16_t)s;
        }
        ng += (int)__popcll(mask);
    }
    ng = min(ng, LOGLIK_MAX_TAIL);   // (at most M by construction)
    wave_lds_order();
    const double cutoff = fmax(*cut, log_dbl_min);
    T.cutoff = cutoff;
    int P = 1;
    while (P < ng) P <<= 1;
    for (int i = ng + lane; i < P; i += 64) {
        kw[i] = ~0ull;
        iw[i] = 0xFFFFu;
    }
    wave_lds_order();
    // bitonic sort of (key, draw), ascending
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int p = i ^ j;
                if (p > i) {
                    const unsigned long long ka = kw[i], kb = kw[p];
                    const uint16_t ia = iw[i], ib = iw[p];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == ((i & k) == 0)) {
                        kw[i] = kb;
                        kw[p] = ka;
                        iw[i] = ib;
                        iw[p] = ia;
                    }
                }
            }
            wave_lds_order();
        }
    // the tail: the sorted entries with x > cutoff (the top L)
    int L = 0;
    for (int i0 = 0; i0 < ng; i0 += 64) {
        const int i = i0 + lane;
        bool above = false;
        if (i < ng) {
            const unsigned long long k = kw[i];
            const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
            above = __longlong_as_double((long long)u) > cutoff;
        }
        L += (int)__popcll(__ballot(above));
    }
    T.L = L;
    T.base = ng - L;
    const int base = T.base;
    const double ecut = exp(cutoff);
    T.ecut = ecut;
    double kk = INFINITY, sigma = 0.0;
    if (L > 4) {
        wave_lds_order();
        for (int i = base + lane; i < ng; i += 64) {
            const unsigned long long k = kw[i];
            const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
            kw[i] = (unsigned long long)__double_as_longlong(exp(__longlong_as_double((long long)u)) - ecut);   // z, as bits
        }
        wave_lds_order();
        auto z = [&](int i) { return __longlong_as_double((long long)kw[base + i]); };
        // Zhang-Stephens: lane j < m is grid point j + 1
        const double Ld = (double)L;
        const int mfit = 30 + (int)sqrt(Ld);
        const double zq = z((int)(Ld / 4.0 + 0.5) - 1), zL = z(L - 1);
        double b = 0.0, lj = 0.0;
        if (lane < mfit) {
            b = 1.0 - sqrt((double)mfit / ((double)(lane + 1) - 0.5));
            b = b / (3.0 * zq);
            b = b + 1.0 / zL;
            double ks = 0.0;
            for (int i = 0; i < L; ++i) ks += log1p(-b * z(i));
            const double kj = ks / Ld;
            lj = Ld * (log(-(b / kj)) - kj - 1.0);
        }
        double wsum = 0.0;
        for (int i = 0; i < mfit; ++i) wsum += exp(__shfl(lj, i) - lj);
        double wj = lane < mfit ? 1.0 / wsum : 0.0;
        if (!(wj >= 10.0 * 2.220446049250313e-16)) wj = 0.0;   // negligible (or NaN) weights dropped
        const double wtot = wave_sum(wj);
        const double bh = wave_sum(wj == 0.0 ? 0.0 : b * (wj / wtot));
        double kh = 0.0;
        for (int i = lane; i < L; i += 64) kh += log1p(-bh * z(i));
        kh = wave_sum(kh) / Ld;
        sigma = -kh / bh;
        kk = (Ld * kh + 5.0) / (Ld + 10.0);
        if (!(fabs(kk) < INFINITY) || !(sigma > 0.0) || !(sigma < INFINITY)) kk = INFINITY;   // no smoothing; never NaN
    }
    T.kk = kk;
    T.sigma = sigma;
    return T;
}

// the i-th smallest of the L tail values after smoothing (kk finite)
__device__ __forceinline__ double psis_smoothed(const PsisTail& T, int i) {
    const double p = ((double)i + 0.5) / (double)T.L;
    double q = fabs(T.kk) < 2.220446049250313e-16 ? -log1p(-p) : expm1(-T.kk * log1p(-p)) / T.kk;
    q = q * T.sigma;
    const double v = log(q + T.ecut);
    return v > 0.0 ? 0.0 : v;
}

template <bool VENUE>
__global__ __launch_bounds__(64 * SUM_WAVES) void loglik_summary(LoglikArgs A) {
    __shared__ unsigned long long tkey[SUM_WAVES][LOGLIK_MAX_TAIL];   // tail keys, then the tail's z values
    __shared__ uint16_t tidx[SUM_WAVES][LOGLIK_MAX_TAIL];             // tail draws
    __shared__ uint32_t hist[SUM_WAVES][256];
    __shared__ double cut[SUM_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long n = (long long)blockIdx.x * SUM_WAVES + w;
    if (n >= A.Q.M) return;   // (wave uniform; no workgroup barrier below)
    const Fix F = make_fix<VENUE>(A, n);
    const int S = A.P.S;

    // pass 1
    double mx = -INFINITY, mn = INFINITY, sm = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double v = ll_at<VENUE>(F, s);
        mx = fmax(mx, v);
        mn = fmin(mn, v);
        sm += v;
    }
    mx = wave_max(mx);
    mn = wave_min(mn);
    sm = wave_sum(sm);
    const bool bad = !(mn > -INFINITY);   // some draw has ll = -inf
    const double mean = sm / (double)S;
    const bool psis = A.psis && !bad;

    // pass 2 (+ the selection's first digit)
    uint32_t* hw = hist[w];
    if (psis) {
        for (int i = lane; i < 256; i += 64) hw[i] = 0u;
        wave_lds_order();
    }
    double se = 0.0, sq = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double v = ll_at<VENUE>(F, s);
        if (mx > -INFINITY) se += exp(v - mx);
        if (!bad) {
            const double d = v - mean;
            sq += d * d;
        }
        if (psis) atomicAdd(&hw[key_of(x_of(mn, v)) >> 56], 1u);
    }
    se = wave_sum(se);
    sq = wave_sum(sq);
    const double lppd = mx > -INFINITY ? mx + log(se / (double)S) : -INFINITY;
    const double var = bad ? INFINITY : (S > 1 ? sq / (double)(S - 1) : 0.0);
    if (lane == 0) {
        A.lppd[n] = lppd;
        A.mean[n] = mean;
        A.var[n] = var;
    }
    if (!A.psis) return;
    if (bad) {
        if (lane == 0) {
            A.elpd_loo[n] = -INFINITY;
            A.pareto_k[n] = INFINITY;
            A.tail_len[n] = 0;
        }
        return;
    }

    // selection, gather, sort and fit (psis_tail above)
    const PsisTail T = psis_tail([&](int s) { return x_of(mn, ll_at<VENUE>(F, s)); }, S, A.tail_m, A.log_dbl_min, lane,
                                 hw, tkey[w], tidx[w], &cut[w]);
    const uint16_t* iw = tidx[w];
    const int L = T.L, base = T.base;
    const double cutoff = T.cutoff, kk = T.kk;
    const bool smooth = kk < INFINITY;   // (L > 4 and a usable fit)
    auto smoothed = [&](int i) { return psis_smoothed(T, i); };
    // pass f: lse(x) and lse(x + ll)
    double ma = -INFINITY, sa = 0.0, mb = -INFINITY, sb = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double v = ll_at<VENUE>(F, s);
        const double x = x_of(mn, v);
        if (smooth && x > cutoff) continue;   // a tail draw: below
        lse_add(ma, sa, x);
        lse_add(mb, sb, x + v);
    }
    if (smooth) {
        for (int i = lane; i < L; i += 64) {
            const double v = ll_at<VENUE>(F, iw[base + i]);
            const double x = smoothed(i);
            lse_add(ma, sa, x);
            lse_add(mb, sb, x + v);
        }
    }
    const double lse_x = wave_lse(ma, sa), lse_xl = wave_lse(mb, sb);
    if (lane == 0) {
        A.elpd_loo[n] = lse_xl - lse_x;
        A.pareto_k[n] = kk;
        A.tail_len[n] = L;
    }
}

}  // namespace dcl
