// dc_outcome.hip.h -- the per-draw outcome probabilities of one fixture: the O(G) walk that dc_score.hip.h
// describes, in a header of its own so that dc_score.hip.h (means over the draws) and dc_sequential.hip.h
// (importance-weighted sums over the draws) run the same lines.
#pragma once
#include <hip/hip_runtime.h>

namespace dcs {

constexpr int SCORE_MAX_GOALS = 63;   // dcp::GRID_MAX_GOALS

// (p_H, p_D, p_A) of one draw on the grid 0..G
__device__ __forceinline__ void outcome_probs(double eh, double ea, double rho, int G, const double* rk, double* pH,
                                              double* pD, double* pA) {
#pragma clang fp contract(off)
    const double lh = exp(eh), la = exp(ea);
    const double u0 = exp(-lh), v0 = exp(-la);
    // the depths 0 and 1 by hand, each tau cell times its own factor (c as in dcl::ll_at): a clipped cell
    // is exactly 0, not the rounding residue of adding and subtracting it
    double u = u0, v = v0, cu = u0, cv = v0;   // Pois(k), and the sums over the counts up to k
    double H = 0.0, D = fmax(1.0 + rho * -(lh * la), 0.0) * (u0 * v0), A = 0.0;
    if (G >= 1) {
        u = u0 * lh;
        v = v0 * la;
        H = fmax(1.0 + rho * la, 0.0) * (u * v0);            // (1, 0)
        A = fmax(1.0 + rho * lh, 0.0) * (u0 * v);            // (0, 1)
        D = fma(fmax(1.0 + rho * -1.0, 0.0), u * v, D);      // (1, 1)
        cu = cu + u;
        cv = cv + v;
    }
#pragma unroll 1
    for (int k = 2; k <= G; ++k) {
        const double r = rk[k];
        u = u * (lh * r);
        v = v * (la * r);
        H = fma(u, cv, H);   // home k, away below k
        A = fma(v, cu, A);
        D = fma(u, v, D);
        cu = cu + u;
        cv = cv + v;
    }
    // (fmax: a rate beyond float64 gives 0, not NaN)
    *pH = fmax(H, 0.0);
    *pD = fmax(D, 0.0);
    *pA = fmax(A, 0.0);
}

}  // namespace dcs
