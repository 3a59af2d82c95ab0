// dc_diagnostics.hip.h -- MCMC convergence diagnostics of posterior draws on the device: the rank-normalised
// split R-hat, bulk / tail / mean effective sample sizes and the Monte Carlo standard error of Vehtari, Gelman,
// Simpson, Carpenter and Buerkner (2021), per scalar quantity, in float64 (definitions: DESIGN.md section 20).
//
// The draws arrive QUANTITY-major ([Q][C N], dcl::transpose_f64 of the host's [C N, Q]).  A quantity's C chains of
// N draws are split into M = 2 C chains of n = N / 2 (the middle draw of an odd N is dropped), S = M n values;
// split position p = m n + i is draw (m >> 1) N + (m & 1) (N - n) + i.
//
// Two kernels, both deterministic (every sum has a fixed order, no floating-point atomics, contraction off):
//   diag_rank   ONE WORKGROUP PER QUANTITY.  mean and sd (ddof = 1) over all C N draws; then twice -- for x and
//       for |x - median x| -- an exact stable LSD radix sort of the draw indices by dcl::key_of (8 bits per pass,
//       passes whose digit is the same for every key are skipped; each wave owns a quarter of the array, counts
//       its digits with integer LDS atomics and scatters its quarter in order, ranks inside a tile of 64 by
//       ballot matching), average ranks of ties from the run around each sorted entry (two binary searches, only
//       where a neighbour is equal), z = Phi^-1((r - 3/8) / (S + 1/4)) by Wichura's AS 241 (PPND16) stored by
//       position, and R-hat of the M x n matrix z.  The median and the requested quantiles (numpy's linear
//       interpolation) are read off the first sorted order.  The keys (8 B) and two index arrays (2 B each) live
//       in LDS when S <= DIAG_LDS_DRAWS (12 B per draw), else in the workspace (same code, other pointers).
//   diag_ess    ONE WAVE PER (quantity, series): series 0 is z (ess_bulk), 1 is x (ess_mean, mcse_mean), 2 walks
//       the indicators x <= q of the quantiles (ess_tail = their minimum).  Chain means first; then the
//       autocovariances directly with lane = lag, 64 lags per block, summed over the chains in chain order, and
//       Geyer's initial positive and monotone sequences consumed pair by pair from the block: the walk stops at
//       the truncation point, so after NUTS one block is the usual cost and n lags the worst case.
// No scratch; vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_loglik.hip.h"   // dcl::key_of, wave_sum, wave_lds_order
#include "dc_market.hip.h"   // dcm::value_of

namespace dcg {
using dcl::wave_lds_order;

constexpr int DIAG_MAX_DRAWS = 65536;      // include/bplhip.h BPLHIP_DIAG_MAX_DRAWS (a split position fits u16)
constexpr int DIAG_MAX_CHAINS = 256;       // include/bplhip.h BPLHIP_DIAG_MAX_CHAINS (M <= 512 chain records in LDS)
constexpr int DIAG_MAX_QUANTILES = 16;     // include/bplhip.h BPLHIP_DIAG_MAX_QUANTILES
constexpr int DIAG_LDS_DRAWS = 12288;      // S up to here sorts in LDS: 12 B per draw = 144 KiB + 12.1 KiB static
constexpr int DIAG_WAVES = 4;
constexpr int DIAG_THREADS = 64 * DIAG_WAVES;
constexpr int DIAG_SERIES = 3;             // bulk, mean, tail
constexpr int DIAG_FLAG_NONFINITE = 1, DIAG_FLAG_CONSTANT = 2;

struct DiagArgs {
    const double* xt;        // [Q][C N] quantity-major draws
    int C, N, n, M, S, CN;
    int NQ;
    const double* q;         // [NQ]
    long long q0, qc;        // the chunk: quantities q0 .. q0 + qc - 1
    // per quantity of the chunk
    double* zb;              // [qc][S] rank-normalised x by split position
    double* zf;              // [qc][S] rank-normalised |x - median| (diag_rank's own)
    unsigned long long* gkey;   // [qc][S] and
    uint16_t* gidx;             // [qc][2 S]: the sort's arrays when S > DIAG_LDS_DRAWS, else unused
    double* qv;              // [qc][NQ] the quantile values
    int32_t* flag;           // [qc]
    // outputs [Q]
    double *mean, *sd, *rhat, *ess_bulk, *ess_tail, *ess_mean, *mcse_mean;
};

__host__ __device__ inline size_t diag_workspace_per_quantity(int S, int NQ) {
    size_t b = (size_t)S * 16 + (size_t)(NQ > 0 ? NQ : 1) * 8 + 8;
    if (S > DIAG_LDS_DRAWS) b += (size_t)S * 12;
    return b;
}
__host__ __device__ inline size_t diag_rank_lds_bytes(int S) {
    return S > DIAG_LDS_DRAWS ? 0 : (size_t)S * 12;
}

// Wichura (1988), Algorithm AS 241, PPND16, without its extreme-tail branch: p stays inside [9.5e-6, 1 - 9.5e-6]
// for S <= 65536, where r = sqrt(-log(min(p, 1 - p))) <= 3.41 < 5
__host__ __device__ inline double inv_phi(double p) {
#pragma clang fp contract(off)
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e0);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                             4.2313330701600911252e+1) * r + 1.0);
        return q * num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r)) - 1.6;
    const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                            1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
                         4.63033784615654529590e0) * r + 1.42343711074968357734e0);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                            1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
                         2.05319162663775882187e0) * r + 1.0);
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// draw index of split position p
__device__ __forceinline__ int split_src(const DiagArgs& A, int p) {
    const int m = p / A.n, i = p - m * A.n;
    return (m >> 1) * A.N + ((m & 1) ? A.N - A.n : 0) + i;
}

// the workgroup's sum in a fixed order: per thread sequential (the caller), lanes by xor butterflies, waves 0..3
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma clang fp contract(off)
    v = dcl::wave_sum(v);
    __syncthreads();   // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Stable LSD radix sort of the S indices in a[] by key[index]; b[] is the second buffer; on return a[] holds
// the order (the pointers are swapped as the passes go).  hist: [DIAG_WAVES][256] LDS words, wtot: [DIAG_WAVES].
// Called by the whole workgroup.
__device__ __forceinline__ void radix_sort(const unsigned long long* key, uint16_t*& a, uint16_t*& b, int S,
                                           uint32_t* hist, uint32_t* wtot) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (S + DIAG_WAVES - 1) / DIAG_WAVES;
    const int lo = min(w * per, S), hi = min(lo + per, S);
    for (int shift = 0; shift < 64; shift += 8) {
        __syncthreads();
        for (int i = tid; i < DIAG_WAVES * 256; i += DIAG_THREADS) hist[i] = 0u;
        __syncthreads();
        for (int i = lo + lane; i < hi; i += 64) atomicAdd(&hist[w * 256 + (int)((key[a[i]] >> shift) & 255u)], 1u);
        __syncthreads();
        // thread = digit: its count per wave, then the exclusive scan of the totals over the 256 digits
        uint32_t c[DIAG_WAVES], total = 0;
        for (int k = 0; k < DIAG_WAVES; ++k) {
            c[k] = hist[k * 256 + tid];
            total += c[k];
        }
        if (__syncthreads_or(total == (uint32_t)S)) continue;   // every key has this digit: nothing moves
        uint32_t incl = total;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        uint32_t base = incl - total;
        for (int k = 0; k < w; ++k) base += wtot[k];
        for (int k = 0; k < DIAG_WAVES; ++k) {
            hist[k * 256 + tid] = base;
            base += c[k];
        }
        __syncthreads();
        // each wave scatters its quarter in order
        uint32_t* off = hist + w * 256;
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int i = i0 + lane;
            const bool valid = i < hi;
            const uint16_t id = valid ? a[i] : (uint16_t)0;
            const uint32_t d = valid ? (uint32_t)((key[id] >> shift) & 255u) : 0u;
            unsigned long long peers = __ballot(valid);
            for (int bit = 0; bit < 8; ++bit) {
                const bool on = (d >> bit) & 1u;
                const unsigned long long bb = __ballot(valid && on);
                peers &= on ? bb : ~bb;
            }
            const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
            const uint32_t cnt = (uint32_t)__popcll(peers);
            if (valid) {
                const uint32_t pos = off[d] + rank;
                if (pos < (uint32_t)S) b[pos] = id;
            }
            wave_lds_order();
            if (valid && rank == 0u) off[d] += cnt;
            wave_lds_order();
        }
        __syncthreads();
        uint16_t* t = a;
        a = b;
        b = t;
    }
    __syncthreads();
}

// z by position from the sorted order: average ranks of ties, then Phi^-1.  Whole workgroup.
__device__ __forceinline__ void rank_normalise(const unsigned long long* key, const uint16_t* ord, int S, double* z) {
#pragma clang fp contract(off)
    for (int r = threadIdx.x; r < S; r += DIAG_THREADS) {
        const uint16_t id = ord[r];
        const unsigned long long k = key[id];
        int first = r, past = r + 1;
        if (r > 0 && key[ord[r - 1]] == k) {   // the run's first entry: the least index whose key is not below k
            int lo = 0, hi = r - 1;            // (key[ord[hi]] == k)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key[ord[mid]] < k) lo = mid + 1;
                else hi = mid;
            }
            first = lo;
        }
        if (r + 1 < S && key[ord[r + 1]] == k) {   // one past the run's last entry
            int lo = r + 1, hi = S;                // (key[ord[lo]] == k; key at hi is above k, or hi = S)
            while (lo + 1 < hi) {
                const int mid = (lo + hi) >> 1;
                if (key[ord[mid]] > k) hi = mid;
                else lo = mid;
            }
            past = lo + 1;
        }
        const double avg = 0.5 * (double)(first + past + 1);   // mean of the 1-based ranks first + 1 .. past
        z[id] = inv_phi((avg - 0.375) / ((double)S + 0.25));
    }
}

// R-hat of the M x n matrix z (row m at z + m n); cm / cv: [M] LDS.  Whole workgroup; every thread gets the result.
__device__ __forceinline__ double rhat_of(const double* z, int M, int n, double* cm, double* cv, double* red) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();   // (z was written by other threads)
    for (int m = w; m < M; m += DIAG_WAVES) {
        const double* row = z + (size_t)m * n;
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += row[i];
        const double mu = dcl::wave_sum(s) / (double)n;
        double q = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double d = row[i] - mu;
            q += d * d;
        }
        q = dcl::wave_sum(q);
        if (lane == 0) {
            cm[m] = mu;
            cv[m] = q / (double)(n - 1);
        }
    }
    __syncthreads();
    double sw = 0.0, sm = 0.0;
    for (int m = threadIdx.x; m < M; m += DIAG_THREADS) {
        sw += cv[m];
        sm += cm[m];
    }
    const double W = block_sum(sw, red) / (double)M;
    const double mm = block_sum(sm, red) / (double)M;
    double sb = 0.0;
    for (int m = threadIdx.x; m < M; m += DIAG_THREADS) {
        const double d = cm[m] - mm;
        sb += d * d;
    }
    const double Bn = block_sum(sb, red) / (double)(M - 1);
    if (W == 0.0) return __longlong_as_double(0x7FF8000000000000ll);
    return sqrt(((double)(n - 1) / (double)n * W + Bn) / W);
}

// grid: the chunk's quantities; dynamic LDS: diag_rank_lds_bytes(S)
__global__ __launch_bounds__(DIAG_THREADS) void diag_rank(DiagArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ uint32_t hist[DIAG_WAVES * 256];
    __shared__ uint32_t wtot[DIAG_WAVES];
    __shared__ double cm[2 * DIAG_MAX_CHAINS], cv[2 * DIAG_MAX_CHAINS];
    __shared__ double red[DIAG_WAVES];
    const int tid = threadIdx.x;
    const long long kq = blockIdx.x;
    if (kq >= A.qc) return;   // (workgroup uniform)
    const size_t k = (size_t)(A.q0 + kq);
    const int S = A.S, n = A.n, M = A.M, CN = A.CN;
    const double* __restrict__ x = A.xt + k * (size_t)CN;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);

    // mean and sd over all draws; is every draw finite?
    double s = 0.0;
    int bad = 0;
    for (int i = tid; i < CN; i += DIAG_THREADS) {
        const double v = x[i];
        s += v;
        bad |= !(fabs(v) < INFINITY);
    }
    const double mean = block_sum(s, red) / (double)CN;
    double sq = 0.0;
    for (int i = tid; i < CN; i += DIAG_THREADS) {
        const double d = x[i] - mean;
        sq += d * d;
    }
    const double sd = sqrt(block_sum(sq, red) / (double)(CN - 1));
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        A.mean[k] = mean;
        A.sd[k] = sd;
    }
    if (bad) {
        if (tid == 0) {
            A.flag[kq] = DIAG_FLAG_NONFINITE;
            A.rhat[k] = nan;
        }
        return;
    }

    unsigned long long* key;
    uint16_t *ia, *ib;
    if (S <= DIAG_LDS_DRAWS) {
        key = reinterpret_cast<unsigned long long*>(dyn);
        ia = reinterpret_cast<uint16_t*>(dyn + (size_t)S * 8);
        ib = ia + S;
    } else {
        key = A.gkey + (size_t)kq * S;
        ia = A.gidx + (size_t)kq * 2 * S;
        ib = ia + S;
    }
    double* zb = A.zb + (size_t)kq * S;
    double* zf = A.zf + (size_t)kq * S;

    // ---- x
    for (int p = tid; p < S; p += DIAG_THREADS) {
        key[p] = dcl::key_of(x[split_src(A, p)] + 0.0);   // (+ 0.0: a -0 ties with +0)
        ia[p] = (uint16_t)p;
    }
    radix_sort(key, ia, ib, S, hist, wtot);
    const double vmin = dcm::value_of(key[ia[0]]), vmax = dcm::value_of(key[ia[S - 1]]);
    if (vmin == vmax) {   // a constant quantity: W = 0 and every var_plus = 0
        if (tid == 0) {
            A.flag[kq] = DIAG_FLAG_CONSTANT;
            A.rhat[k] = nan;
        }
        return;
    }
    // the median (S is even) and the quantiles, numpy's "linear" method and its lerp
    const double med = (dcm::value_of(key[ia[S / 2 - 1]]) + dcm::value_of(key[ia[S / 2]])) / 2.0;
    if (tid < A.NQ) {
        const double qq = A.q[tid];
        const double h = ((double)S * qq + (1.0 + qq * -1.0)) - 1.0;
        double fl = floor(h);
        int lo = (int)fl;
        if (lo < 0) lo = 0;
        if (lo > S - 1) lo = S - 1;
        double g = h - fl;
        if (g < 0.0) g = 0.0;
        const int up = lo + 1 < S ? lo + 1 : S - 1;
        const double a = dcm::value_of(key[ia[lo]]), b = dcm::value_of(key[ia[up]]);
        const double diff = b - a;
        double r = a + diff * g;
        if (g >= 0.5) r = b - diff * (1.0 - g);
        A.qv[(size_t)kq * A.NQ + tid] = r;
    }
    rank_normalise(key, ia, S, zb);
    const double rhat_b = rhat_of(zb, M, n, cm, cv, red);

    // ---- |x - median|
    __syncthreads();
    for (int p = tid; p < S; p += DIAG_THREADS) {
        key[p] = dcl::key_of(fabs(x[split_src(A, p)] - med) + 0.0);
        ia[p] = (uint16_t)p;
    }
    radix_sort(key, ia, ib, S, hist, wtot);
    rank_normalise(key, ia, S, zf);
    const double rhat_f = rhat_of(zf, M, n, cm, cv, red);
    if (tid == 0) {
        A.flag[kq] = 0;
        A.rhat[k] = (rhat_b != rhat_b || rhat_f != rhat_f) ? nan : fmax(rhat_b, rhat_f);
    }
}

// ess of the M x n series val(m, i) by one wave; cm: [M] LDS of this wave.  NaN when var_plus = 0.
template <class V>
__device__ __forceinline__ double ess_wave(V val, int M, int n, int lane, double* cm) {
#pragma clang fp contract(off)
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double nd = (double)n;
    wave_lds_order();
    for (int m = 0; m < M; ++m) {
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += val(m, i);
        s = dcl::wave_sum(s) / nd;
        if (lane == 0) cm[m] = s;
    }
    wave_lds_order();
    double sm = 0.0;
    for (int m = lane; m < M; m += 64) sm += cm[m];
    const double mm = dcl::wave_sum(sm) / (double)M;
    double sb = 0.0;
    for (int m = lane; m < M; m += 64) {
        const double d = cm[m] - mm;
        sb += d * d;
    }
    const double vb = dcl::wave_sum(sb) / (double)(M - 1);

    double mean_var = 0.0, var_plus = 0.0;
    double pe = 1.0, po = 0.0;       // the last pair computed (rho_{t-1}, rho_t)
    double pa = 0.0, pb = 0.0;       // the last pair inside the sequence, after the monotone step
    bool has_prev = false;
    double acc = 0.0;                // sum of rho_0 .. rho_{t-2}
    int t = 1;
    for (int t0 = 0; t0 < n; t0 += 64) {
        // this block's autocovariances, lane = lag
        const int lag = t0 + lane;
        double a = 0.0;
        for (int m = 0; m < M; ++m) {
            const double mu = cm[m];
            double cs = 0.0;
            for (int i = 0; i < n - t0; ++i) {
                const double u = val(m, i) - mu;
                if (i + lag < n) cs = fma(u, val(m, i + lag) - mu, cs);
            }
            a += cs;
        }
        a = a / nd / (double)M;
        if (t0 == 0) {
            const double a0 = __shfl(a, 0);
            mean_var = a0 * nd / (nd - 1.0);
            var_plus = mean_var * (nd - 1.0) / nd + vb;
            if (var_plus == 0.0) return nan;
        }
        const double rho = 1.0 - (mean_var - a) / var_plus;
        int j = 0;
        if (t0 == 0) {
            po = __shfl(rho, 1);
            j = 2;
        }
        bool done = false;
        for (; j < 64; j += 2) {
            if (!(t < n - 3 && pe + po > 0.0)) {
                done = true;
                break;
            }
            double e = pe, o = po;
            if (has_prev && e + o > pa + pb) {
                e = (pa + pb) / 2.0;
                o = e;
            }
            acc += e + o;
            pa = e;
            pb = o;
            has_prev = true;
            pe = __shfl(rho, j);       // lag t + 1 = t0 + j
            po = __shfl(rho, j + 1);
            t += 2;
        }
        if (done) break;
    }
    const double last = (pe > 0.0 || pe + po >= 0.0) ? pe : 0.0;
    double tau = -1.0 + 2.0 * acc + last;
    const double S = (double)M * nd;
    tau = fmax(tau, 1.0 / log10(S));
    return S / tau;
}

// grid: ceil(qc * DIAG_SERIES / DIAG_WAVES) workgroups; wave -> (quantity of the chunk, series)
__global__ __launch_bounds__(DIAG_THREADS) void diag_ess(DiagArgs A) {
#pragma clang fp contract(off)
    __shared__ double cmw[DIAG_WAVES][2 * DIAG_MAX_CHAINS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long item = (long long)blockIdx.x * DIAG_WAVES + w;
    if (item >= A.qc * DIAG_SERIES) return;   // (wave uniform; no workgroup barrier below)
    const long long kq = item / DIAG_SERIES;
    const int ser = (int)(item - kq * DIAG_SERIES);
    const size_t k = (size_t)(A.q0 + kq);
    const int n = A.n, M = A.M, N = A.N;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double* out = ser == 0 ? A.ess_bulk : ser == 1 ? A.ess_mean : A.ess_tail;
    if (A.flag[kq] != 0) {
        if (lane == 0) {
            out[k] = nan;
            if (ser == 1) A.mcse_mean[k] = nan;
        }
        return;
    }
    const double* __restrict__ x = A.xt + k * (size_t)A.CN;
    auto xs = [&](int m, int i) { return x[(m >> 1) * N + ((m & 1) ? N - n : 0) + i]; };
    if (ser == 0) {
        const double* __restrict__ z = A.zb + (size_t)kq * A.S;
        const double e = ess_wave([&](int m, int i) { return z[m * n + i]; }, M, n, lane, cmw[w]);
        if (lane == 0) out[k] = e;
    } else if (ser == 1) {
        const double e = ess_wave(xs, M, n, lane, cmw[w]);
        if (lane == 0) {
            out[k] = e;
            A.mcse_mean[k] = A.sd[k] / sqrt(e);
        }
    } else {
        double least = INFINITY;
        bool any_nan = false;
        for (int iq = 0; iq < A.NQ; ++iq) {
            const double qv = A.qv[(size_t)kq * A.NQ + iq];
            const double e = ess_wave([&](int m, int i) { return xs(m, i) <= qv ? 1.0 : 0.0; }, M, n, lane, cmw[w]);
            if (e != e) any_nan = true;
            else least = fmin(least, e);
        }
        if (lane == 0) out[k] = (any_nan || A.NQ == 0) ? nan : least;
    }
}

}  // namespace dcg
