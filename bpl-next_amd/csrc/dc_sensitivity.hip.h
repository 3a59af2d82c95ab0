// dc_sensitivity.hip.h -- how far the distribution of every scalar quantity of a posterior moves when its draws
// are re-weighted: the symmetrised, normalised cumulative Jensen-Shannon distance of power-scaling sensitivity
// analysis (Kallioinen, Paananen, Buerkner and Vehtari 2023), per quantity and weight row, in float64
// (definitions: DESIGN.md section 33).
//
// The draws arrive QUANTITY-major ([Q][S], dcl::transpose_f64 of the host's [S, Q]); the weight rows are stored
// rows of normalised log weights [R][S] (dcu::psis_rows' output).  Per quantity, with the draws sorted ascending
// (ties by draw), position i = 1 .. S - 1 (1-based) starts the interval d_i = x_(i+1) - x_(i), over which the
// unweighted ECDF is P_i = i / S and the weighted one is Q_i = (w_(1) + .. + w_(i)) / W:
//     JS = sum d_i [P_i log2(P_i / M_i) + Q_i log2(Q_i / M_i)], M_i = (P_i + Q_i) / 2   (a term with Q_i = 0 is 0)
//     B  = sum d_i (P_i + Q_i)                 F = max(JS, 0) / B
// and R is the same with P_i -> 1 - P_i, Q_i -> max(1 - Q_i, 0) (the quantity -x); cjs_sq = max(F, R).
//
// One kernel:
//   shift_summary   ONE WORKGROUP OF 4 WAVES PER QUANTITY.  Keys (dcl::key_of) and draw indices, the stable LSD
//       radix sort dcg::radix_sort, then per weight row: the weights exp(lw) are written over the keys (by draw),
//       mean and sd as two fixed-order passes (dcip::inplay_summary's form), the scan of the weights in sorted
//       order (thread i owns the i-th segment, sums it sequentially, the 256 segment totals are added left to
//       right), and one walk per thread over its segment's intervals -- the interval after a segment's last
//       position reaches into the next segment, position S - 1 starts none -- that accumulates JS and B of both
//       passes; dcg::block_sum reduces the four.  The keys (8 B) and two index arrays (2 B each) live in LDS when
//       S <= SHIFT_LDS_DRAWS, else in the workspace (same code, other pointers).  A quantity with a non-finite
//       draw is not sorted, a quantity whose draws are all equal is not walked: both get mean and sd and a NaN.
// No floating-point atomics, no scratch, vector stores only; contraction is off and every fma explicit.  A value's
// accumulation order depends only on S: results are bit-identical from run to run and under any chunking.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dc_diagnostics.hip.h"   // dcg::radix_sort, block_sum
#include "dc_loglik.hip.h"        // dcl::key_of

namespace dcps {

constexpr int SHIFT_MAX_ROWS = 8;                      // include/bplhip.h BPLHIP_SHIFT_MAX_ROWS
constexpr int SHIFT_MAX_DRAWS = dcg::DIAG_MAX_DRAWS;   // (a draw index fits u16)
constexpr int SHIFT_LDS_DRAWS = dcg::DIAG_LDS_DRAWS;   // S up to here sorts in LDS: 12 B per draw = 144 KiB + 6.2 KiB static
constexpr int SHIFT_WAVES = dcg::DIAG_WAVES;
constexpr int SHIFT_THREADS = 64 * SHIFT_WAVES;

struct ShiftArgs {
    const double* xt;           // [Q][S] quantity-major draws
    const double* lw;           // [R][S] normalised log weights
    int S, R;
    long long Q;
    long long q0, qc;           // the chunk: quantities q0 .. q0 + qc - 1
    unsigned long long* gkey;   // [qc][S] and
    uint16_t* gidx;             // [qc][2 S]: the sort's arrays when S > SHIFT_LDS_DRAWS, else unused
    double *cjs_sq, *mean, *sd; // [R][Q]
};

__host__ __device__ inline size_t shift_workspace_per_quantity(int S) {
    return S > SHIFT_LDS_DRAWS ? (size_t)S * 12 : 0;
}
__host__ __device__ inline size_t shift_summary_lds_bytes(int S) {
    return S > SHIFT_LDS_DRAWS ? 0 : (size_t)S * 12;
}

// one interval's integrand: p log2(p / m) + q log2(q / m), m = (p + q) / 2; a term whose own factor is 0 counts 0
__device__ __forceinline__ double js_term(double p, double q) {
#pragma clang fp contract(off)
    const double m = (p + q) / 2.0;
    const double a = p > 0.0 ? p * log2(p / m) : 0.0;
    const double b = q > 0.0 ? q * log2(q / m) : 0.0;
    return a + b;
}

// grid: the chunk's quantities; dynamic LDS: shift_summary_lds_bytes(S)
__global__ __launch_bounds__(SHIFT_THREADS) void shift_summary(ShiftArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ uint32_t hist[SHIFT_WAVES * 256];
    __shared__ uint32_t wtot[SHIFT_WAVES];
    __shared__ double red[SHIFT_WAVES];
    __shared__ double tot[SHIFT_THREADS];   // the segment totals of the scan
    const int tid = threadIdx.x;
    const long long kq = blockIdx.x;
    if (kq >= A.qc) return;   // (workgroup uniform)
    const size_t k = (size_t)(A.q0 + kq);
    const int S = A.S;
    const size_t Q = (size_t)A.Q;
    const double* __restrict__ x = A.xt + k * (size_t)S;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);

    unsigned long long* key;
    uint16_t *ia, *ib;
    if (S <= SHIFT_LDS_DRAWS) {
        key = reinterpret_cast<unsigned long long*>(dyn);
        ia = reinterpret_cast<uint16_t*>(dyn + (size_t)S * 8);
        ib = ia + S;
    } else {
        key = A.gkey + (size_t)kq * S;
        ia = A.gidx + (size_t)kq * 2 * S;
        ib = ia + S;
    }
    double* om = reinterpret_cast<double*>(key);   // the weights, over the keys once the order is known

    // the keys; is every draw finite?
    int bad = 0;
    for (int s = tid; s < S; s += SHIFT_THREADS) {
        const double v = x[s];
        bad |= !(fabs(v) < INFINITY);
        key[s] = dcl::key_of(v + 0.0);   // (+ 0.0: a -0 ties with +0)
        ia[s] = (uint16_t)s;
    }
    bad = __syncthreads_or(bad);
    bool walk = false;
    if (!bad) {
        dcg::radix_sort(key, ia, ib, S, hist, wtot);   // (ia: the order, ties by draw)
        walk = key[ia[0]] != key[ia[S - 1]];           // all draws equal: B = 0
    }
    __syncthreads();   // (every thread has compared the keys before the weights replace them)

    // thread i owns the sorted positions i per .. (i + 1) per - 1
    const int per = (S + SHIFT_THREADS - 1) / SHIFT_THREADS;
    const int lo = min(tid * per, S), hi = min(lo + per, S);
    const double Sd = (double)S;

    for (int r = 0; r < A.R; ++r) {
        const double* __restrict__ lw = A.lw + (size_t)r * (size_t)S;
        const size_t o = (size_t)r * Q + k;
        __syncthreads();   // (the row before may still read its weights)
        for (int s = tid; s < S; s += SHIFT_THREADS) om[s] = exp(lw[s]);
        __syncthreads();

        // mean and sd: two passes, per thread sequential over s = tid, tid + 256, ..., then dcg::block_sum
        double s0 = 0.0, s1 = 0.0;
        for (int s = tid; s < S; s += SHIFT_THREADS) {
            const double w = om[s];
            s0 += w;
            s1 = fma(w, x[s], s1);
        }
        const double sw = dcg::block_sum(s0, red);
        const double mean = dcg::block_sum(s1, red) / sw;
        double sq = 0.0;
        for (int s = tid; s < S; s += SHIFT_THREADS) {
            const double d = x[s] - mean;
            sq = fma(om[s], d * d, sq);
        }
        sq = dcg::block_sum(sq, red);
        if (tid == 0) {
            A.mean[o] = mean;
            A.sd[o] = sqrt(sq / sw);
        }
        if (!walk) {   // (workgroup uniform)
            if (tid == 0) A.cjs_sq[o] = nan;
            continue;
        }

        // the scan of the weights in sorted order: C just before this segment, and W, its last element
        double part = 0.0;
        for (int i = lo; i < hi; ++i) part += om[ia[i]];
        tot[tid] = part;
        __syncthreads();
        double before = 0.0, W = 0.0;
        for (int i = 0; i < SHIFT_THREADS; ++i) {
            if (i == tid) before = W;
            W += tot[i];
        }

        // the walk: position i (0-based) starts the interval to position i + 1, with P = (i + 1) / S and
        // Q = (before + the segment's own partial sum) / W
        double jf = 0.0, bf = 0.0, js = 0.0, bs = 0.0;
        if (lo < hi) {
            double run = 0.0;
            double xa = x[ia[lo]];
            for (int i = lo; i < hi && i + 1 < S; ++i) {
                run += om[ia[i]];
                const double xb = x[ia[i + 1]];
                const double d = xb - xa;
                xa = xb;
                const double p = (double)(i + 1) / Sd;
                const double q = (before + run) / W;
                const double ps = 1.0 - p, qs = fmax(1.0 - q, 0.0);
                jf += d * js_term(p, q);
                bf += d * (p + q);
                js += d * js_term(ps, qs);
                bs += d * (ps + qs);
            }
        }
        jf = dcg::block_sum(jf, red);
        bf = dcg::block_sum(bf, red);
        js = dcg::block_sum(js, red);
        bs = dcg::block_sum(bs, red);
        if (tid == 0) A.cjs_sq[o] = fmax(fmax(jf, 0.0) / bf, fmax(js, 0.0) / bs);
    }
}

}  // namespace dcps
