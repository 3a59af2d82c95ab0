// dc_posterior.hip.h -- the fitted posterior as the kernels see it, the query columns of the per-fixture
// kernels and the log-rate forms.  dc_predict, dc_loglik and dc_ppc embed the view in their argument
// structs; dc_tournament builds it in the kernel; loglik, tournament and ppc take their rates from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcq {

// S draws of T teams (C confederations, 0: none).  Two layouts, chosen by the host (posterior_view in
// bplhip.hip) and fixed per kernel:
//   row-major   [S,T] tables, conf [S,C]: a draw's teams contiguous (predict_score_proba, season,
//               tournament, ppc: one draw, many teams)
//   team-major  [T,S] tables, conf [C,S]: a team's draws contiguous (loglik: lane = draw)
// corr is [S] in both.  By model family:
//   plain  (predict_set_posterior)        home_adv is [S] (ha_stride = 0) or a per-team table
//          (ha_stride != 0; T in the row-major view); the four venue tables and conf are unused, C = 0
//   venue  (predict_set_posterior_venue)  home_attack, away_attack, home_defence, away_defence are
//          tables; conf is null when C = 0; home_adv is unused, ha_stride = 0
// (member order matters: an argument struct's leading 14 dwords arrive preloaded in SGPRs, csrc/Makefile)
template <class F>
struct Posterior {
    int S, T, C;
    const F* attack;
    const F* defence;
    const F* home_adv;
    int ha_stride;
    const F* home_attack;
    const F* away_attack;
    const F* home_defence;
    const F* away_defence;
    const F* conf;
    const F* corr;
};

// M queries (proba, loglik): model indices, goals as given (may exceed 255); venue: neutral (and confederations)
struct Queries {
    long long M;
    const uint16_t *h, *a, *x, *y;
    const uint8_t* neutral;
    const uint16_t *hc, *ac;
};

// ---- the log-rate forms (eh = log lh, ea = log la of a fixture h v a in one draw; on = 1 - neutral).
// Both venue forms then add / subtract dc = conf[c(h)] - conf[c(a)] when there are confederations.
// There are two venue forms ON PURPOSE.  Each is pinned operation for operation by a numpy restatement
// that the GPU tests compare against bit for bit: the product form by tests/fake_ctx.py::_log_rates and
// tests/loglik_ref.py (log-likelihood), the branch form by tests/tournament_ref.py::rates (tournament,
// ppc).  They differ in the last bit for on = 1, so merging them would change sampled scorelines.
// All are written with contraction off: a rate has the same bits in every kernel and pass.
// dcp::predict_score_proba keeps its own lines (compiled with contraction ON, venue term associated as
// eh + (on hat - on adf)); dcp::predict_score_grid is float32 on the matrix pipe and keeps its lambda.
// (the value forms take their operands in the order the expressions read them: a caller that passes
// loads gets them issued in that order)
template <class F>
__device__ __forceinline__ void log_rates_plain_v(F ah, F da, F ha, F aa, F dh, F* eh, F* ea) {
#pragma clang fp contract(off)
    *eh = ah - da + ha;
    *ea = aa - dh;
}
template <class F>
__device__ __forceinline__ void log_rates_venue_product_v(F ah, F da, F on, F hat, F adf, F aa, F dh, F aat, F hdf,
                                                          F* eh, F* ea) {
#pragma clang fp contract(off)
    *eh = ah - da + on * hat - on * adf;
    *ea = aa - dh + on * aat - on * hdf;
}
template <class F>
__device__ __forceinline__ void add_confederations(F dc, F* eh, F* ea) {
#pragma clang fp contract(off)
    *eh = *eh + dc;
    *ea = *ea - dc;
}
// row-major views: draw s, model indices h, a
template <class F>
__device__ __forceinline__ void log_rates_plain(const Posterior<F>& P, int s, int h, int a, F* eh, F* ea) {
    const size_t r = (size_t)s * P.T;
    log_rates_plain_v(P.attack[r + h], P.defence[r + a], P.ha_stride ? P.home_adv[r + h] : P.home_adv[s],
                      P.attack[r + a], P.defence[r + h], eh, ea);
}
template <class F>
__device__ __forceinline__ void log_rates_venue_branch(const Posterior<F>& P, int s, int h, int a, bool on, F* eh, F* ea) {
#pragma clang fp contract(off)
    const size_t r = (size_t)s * P.T;
    *eh = P.attack[r + h] - P.defence[r + a];
    *ea = P.attack[r + a] - P.defence[r + h];
    if (on) {
        *eh = *eh + (P.home_attack[r + h] - P.away_defence[r + a]);
        *ea = *ea + (P.away_attack[r + a] - P.home_defence[r + h]);
    }
}
// ... followed, when P.C != 0, by the two sides' confederations hc, ac
template <class F>
__device__ __forceinline__ void add_confederations(const Posterior<F>& P, int s, int hc, int ac, F* eh, F* ea) {
    const F* cs = P.conf + (size_t)s * P.C;
    add_confederations(cs[hc] - cs[ac], eh, ea);
}

}  // namespace dcq
