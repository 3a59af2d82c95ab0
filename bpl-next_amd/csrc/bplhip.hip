// bplhip.hip -- C-ABI (include/bplhip.h) over the gfx950 kernels in dc_kernels.hip.h.
// Host side: context, fixture re-layout (sort by (home,away) pair, pad to the wave
// tile, data-only sums), launch sequences, hipGraph replay, and the NUTS driver glue.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/bplhip.h"
#include "dc_dynamic.hip.h"
#include "dc_kernels.hip.h"
#include "dc_loglik.hip.h"
#include "dc_loo.hip.h"
#include "dc_sequential.hip.h"
#include "dc_neutral.hip.h"
#include "dc_ppc.hip.h"
#include "dc_predict.hip.h"
#include "dc_score.hip.h"
#include "dc_market.hip.h"
#include "dc_inplay.hip.h"
#include "dc_period.hip.h"
#include "dc_ratings.hip.h"
#include "dc_slate.hip.h"
#include "dc_diagnostics.hip.h"
#include "dc_sensitivity.hip.h"
#include "dc_playoff.hip.h"
#include "dc_season.hip.h"
#include "dc_live.hip.h"
#include "dc_leverage.hip.h"
#include "dc_points.hip.h"
#include "dc_scenario.hip.h"
#include "dc_live_queries.hip.h"
#include "dc_trajectory.hip.h"
#include "dc_paths.hip.h"
#include "dc_tscen.hip.h"
#include "dc_group_points.hip.h"
#include "dc_tournament.hip.h"
#include "dc_tournament_live.hip.h"
#include "dc_tournament_live_queries.hip.h"
#include "dc_h2h.hip.h"
#include "dc_vec.hip.h"
#include "nuts.hpp"
#include "threefry.hpp"

namespace {

thread_local std::string g_create_error;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

struct GraphKey {
    int count, n_z;
    const void *z, *pot, *grad;
    bool operator<(const GraphKey& o) const {
        return std::tie(count, n_z, z, pot, grad) <
               std::tie(o.count, o.n_z, o.z, o.pot, o.grad);
    }
};

}  // namespace

struct bplhip_ctx {
    int device = 0;
    std::string err;
    bool bound = false;
    dc::Layout L{};
    int64_t n = 0;
    int n_tiles = 0;
    // Launch geometry of dc_eval ("partition"): which waves of a workgroup own tiles, tiles per
    // wave, workgroups, and the sparse-slab structure that follows from it.  Two of them when the
    // stream is short: with idle CUs a chain runs on twice the workgroups with 4 of 8 waves owning
    // tiles (two waves share a SIMD and a tile's lane arithmetic is issue bound: -3 % at N = 1e6,
    // -13 % at 1e5); several chains per launch fill the chip with the 8-wave partition (the
    // 4-wave one cost them 15-25 %).  ep = the one selected for the current launch.
    struct EvalPart {
        int aw = dc::WAVES, tpw = 1, n_wg = 1, total_c = 0;
        bool staged = true;   // the tail stages the compact array in LDS
        DevBuf d_wg_off, d_wg_slots, d_col_off, d_wg_dst;
        DevBuf d_ga_expect;   // contributions every accumulator row receives per evaluation (dc::ga_add)
    } parts[2];
    int n_parts = 1;
    EvalPart* ep = &parts[0];
    int n_cu = 256;
    bool weighted = false;
    int P = 0;
    double lgsum = 0.0;
    // device buffers (library owned)
    DevBuf d_h, d_a, d_x, d_y, d_w, d_pairs, d_xs, d_cA, d_cD, d_cH, d_tickets, d_debug, d_xsf, d_hbuf;
    DevBuf d_gacc;  // accumulator rows of dc_eval's hand-off (dc::GA_ROW)
    DevBuf d_pairw; // per unique pair: sum of weights, of w x, of w y (data only; dc::EvalArgs::pairw)
    DevBuf d_pairc; // per unique pair: weight of its (0,0), (1,0), (0,1) fixtures (dc::ill_pass)
    double w11 = 0.0;  // weight of all (1,1) fixtures
    // fault word: host memory mapped into the device.  A kernel whose bounded wait expires ORs its
    // code in (dc::raise_fault); every entry point looks at it on the way in and on the way out
    // (consume_fault), so a timed-out hand-off becomes BPLHIP_EHIP + a message instead of NaN outputs
    // that a sampler would book as divergences.
    unsigned int* h_fault = nullptr;
    unsigned int* d_fault = nullptr;
    int opt_chunk_graph = 1;
    bool dyn_fused_ok = true;   // cleared when the single-launch dynamic kernel timed out: four launches from then on
    int dyn_fused_blocks_per_cu = -1;  // occupancy of dyn_fused (queried once)
    long long dyn_max_gw = 0;          // fixtures of the largest gameweek (dyn_fused<true> sizes its LDS by it)
    int opt_dyn_big_wgs = 0;           // dyn_fused<true>: workgroups aimed for (0: one per CU)
    int opt_dyn_gather = 1;            // dyn_fused<false>: adjoint records + gather (1) or float64 atomics into the cells (0)
    size_t dyn_big_lds = 0;            // ... the LDS size its cached occupancy belongs to
    int dyn_big_blocks_per_cu = 0;
    bool dyn_big_attr_set = false, neu_big_attr_set = false;
    DevBuf d_zb;    // persistent evaluation kernel: the next position as tagged granules
    unsigned int loop_tag = 0;  // tags handed out so far (a launch of k steps takes k + 1 of them)
    int opt_persistent_kernel = 1;  // 1: a single chain's leapfrogs run inside one resident launch
    int opt_persist_spec = 1;       // ... and the next position is published before the leaf is booked (dc::tail_waves)
    int opt_pair_order = -1;        // fixture layout: 0 (home, away) order, 1 Z-order over (home, away), -1: Z-order past 64 teams
    int opt_dense_pairs = 1;        // 1: complete pair tables take the separable (O(teams)) bounds
    bool pairs_complete = false;
    int opt_fused_small = 1;        // 1: neutral / dynamic evaluations that fit one CU's LDS run as one launch
    bool neu_attr_set = false;
    int slab_chains = 0;
    // tuning options (bplhip_set_option)
    int opt_device_nuts = 1;  // 1: tree builder on the device (nuts_dev.hip.h) when supported
    int opt_max_wg = 255;  // streaming workgroups (+1 prior workgroup = one per CU)
    int opt_active_waves = 0;  // waves per workgroup that own tiles (0 = automatic, see set_fixtures)
    int opt_persistent_nuts = 1;  // bplhip_nuts_run_chains: whole chains on the device (0: lock step)
    int opt_vec_min_chains = 12;  // batched calls with at least this many chains use dc_vec (0: never);
                                  // fewer run as grid.y copies of the single-chain launch (62 workgroups per
                                  // chain at N = 1e6).  Round 4: 12 (was 32) -- with the chain arithmetic done per
                                  // run dc_vec takes 10.5 us for 8 or 16 chains, the copies 9.2 for 8 and 13.8 for 16
    int opt_gridy_max_chains = 8;   // persistent chains: grid.y copies of the NUTS-aware launch up to here (was 32:
                                    // 16 chains 698k -> 921k leapfrogs/s, 32 chains 986k -> 1.22M through dc_vec;
                                    // 8 chains stay with the copies, 582k against 474k: profiles/r04/lockstep_gridy.txt)
    int opt_vec_tpw = 0;         // > 0: force this many tiles per wave for every chain count
    // chain-vectorised partitions (dc_vec.hip.h): fewer, fatter workgroups the more chains
    // share a launch (the per-workgroup prologue builds 8 chains' tables); each has its
    // own sparse-slab structure.  vps[0..2]: 1x / 2x / 3x the single-chain tiles per wave,
    // used for <= 8 / <= 23 / more chains; vp = the one selected for the current launch.
    struct VecPart {
        bool ok = false, staged = true;
        int tpw = 1, n_wg = 1, total_c = 0, slab_chains = 0;
        DevBuf d_wg_off, d_wg_slots, d_col_off, d_wg_dst, d_hbuf;
    } vps[3];
    VecPart* vp = &vps[0];
    bool lds_attr_set = false;
    // NUTS scratch (device): z, potential, grad, aux + pinned host mirror
    DevBuf d_nuts, d_ns;
    // posterior draws for the device predict path (dc_predict.hip.h)
    // (tables 0..7: attack, defence, home_advantage | home_attack, away_attack, home_defence,
    // away_defence, confederation_strength; float64 [S, cols] for the pointwise kernel and float32
    // team-major [cols, S] for the grid kernel)
    DevBuf dp_tab[8], dp_tab32[8], dp_corr, dp_corr32, dp_q;
    DevBuf dp_season;   // simulate_season: fixtures, table, counts, per-simulation outputs (dc_season.hip.h)
    DevBuf dp_leverage; // match_leverage: count tables, fixtures, table and the chunk's records (dc_leverage.hip.h)
    DevBuf dp_points;   // season_points: count tables, fixtures, table and the chunk's records (dc_points.hip.h)
    DevBuf dp_trajectory;   // season_trajectory: the same for dc_trajectory.hip.h
    DevBuf dp_scenario;     // season_scenarios: the same for dc_scenario.hip.h
    DevBuf dp_tournament;   // simulate_tournament: slots, fixtures, bracket tables, counts, stages (dc_tournament.hip.h)
    // log-likelihood path (dc_loglik.hip.h): float64 TEAM-major [cols, S] copies of dp_tab, built on the
    // first loglik call after an upload (pred_tm), and the query / output buffer
    DevBuf dp_tm[8], dp_ll;
    DevBuf dp_mkt;   // market_summary: weights, quantiles, outputs and the per-draw values of a chunk (dc_market.hip.h)
    DevBuf dp_diag, dp_diag_ws;   // mcmc_diagnostics: draws, their transpose, quantiles and outputs; the chunk's workspace (dc_diagnostics.hip.h)
    bool diag_attr_set = false;
    DevBuf dp_shift, dp_shift_ws;   // weighted_shift: ratios, log weights, draws, their transpose and outputs; the chunk's sort arrays (dc_sensitivity.hip.h)
    bool shift_attr_set = false;
    DevBuf dp_inplay;   // inplay_summary: weights, quantiles, states, outputs and a chunk's values and evidence (dc_inplay.hip.h)
    bool inplay_attr_set = false;
    DevBuf dp_period;   // period_summary: weights, quantiles, splits, outputs and the per-draw values of a chunk (dc_period.hip.h)
    DevBuf dp_ratings;   // team_ratings: indices, quantiles, outputs, the ranked statistic [R, S] and a chunk's values (dc_ratings.hip.h)
    DevBuf dp_slate;   // slate_summary: slate starts, leg tables, quantiles, outputs and a chunk's values (dc_slate.hip.h)
    DevBuf dp_ppc;   // posterior_predictive_check: queries, per-replication tallies and scorelines (dc_ppc.hip.h)
    bool pred_tm = false;
    int pred_S = 0, pred_T = 0, pred_C = 0, pred_ha_stride = 0;
    bool pred_venue = false;
    // the best-of-rest allocation of the tournament family (bplhip_tournament_set_allocation): host copies, staged
    // into every tournament call's record while set (alloc_rows = 0: none)
    int alloc_groups = 0, alloc_best = 0, alloc_rows = 0;
    std::vector<uint16_t> alloc_row;
    std::vector<uint8_t> alloc_slot;
    double* h_pinned = nullptr;
    size_t h_pinned_bytes = 0;
    // host copies needed by bplhip_constrain (rho bounds over the unique pairs)
    std::vector<uint32_t> h_pairs;
    std::vector<double> h_xs;
    // dynamic (time-varying) model: separate float64 path (dc_dynamic.hip.h)
    bool dynamic = false;
    dcd::DynLayout DL{};
    int dyn_random_walk = 1;
    bool dyn_scratch_clean = false;  // the single-launch kernel finds (and leaves) its scratch zeroed
    // neutral-venue model (dc_neutral.hip.h): the dynamic model's fixture passes + own z side
    bool neutral = false;
    dcn::NeuLayout NL{};
    DevBuf dd_gw, dd_nv, dd_cells, dd_acc, dd_hyp, dd_hc, dd_ac;
    DevBuf dd_fpack, dd_sched, dd_slot_off;  // single-launch neutral kernel (dcn::neu_fused)
    std::vector<unsigned long long> neu_keys;   // neu_big: the sorted fixtures' run keys (host copy: run counts per wave)
    int neu_runs_nb = -1;                       // ... the grid size the cached answer belongs to
    bool neu_runs_ok = false;
    int opt_neu_runs = 1;                       // neu_big: per-run arithmetic (1) / per-fixture (0)
    int last_eval_path = BPLHIP_PATH_NONE;      // the form the last evaluation was launched in (host bookkeeping only)
    int last_nuts_engine = BPLHIP_ENGINE_NONE;  // the engine the last sampler run was dispatched to (likewise)
    bool neu_fusable = false;
    int neu_slots = 0;
    int opt_debug_stop = 0;         // diagnostic build only
    DevBuf dd_gwoff, dd_tick;  // dynamic model: first fixture of each gameweek; arrival counters
    DevBuf dd_fx8;             // dynamic model: one packed word per fixture (dcd::pack_fixture), dyn_fused<true>
    DevBuf dd_fadj, dd_inc_off, dd_inc;   // dyn_fused<false>: per-fixture adjoint records + the cells' incidence lists
    bool dyn_gather = false;   // every cell's list is short enough for the gathering phase 4
    bool dyn_attr_set = false;
    std::map<GraphKey, hipGraphExec_t> graphs;
    hipStream_t cap_stream = nullptr;
    bool capturing = false;   // between hipStreamBeginCapture and hipStreamEndCapture on cap_stream: nothing
                              // may allocate, free or synchronise (capture_launches)

    ~bplhip_ctx() {
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        if (h_pinned) (void)hipHostFree(h_pinned);
    }
};

namespace {

int fail(bplhip_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIP_TRY(c, expr)                                                            \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess)                                                       \
            return fail((c), BPLHIP_EHIP, "%s failed: %s (%s:%d)", #expr,           \
                        hipGetErrorString(e_), __FILE__, __LINE__);                 \
    } while (0)

constexpr size_t LDS_LIMIT = 160 * 1024;

// the prior workgroup's record: header | gz[D] | eps[3T] | (dc_vec) the ill-conditioned classes' sums [3T + 4]
int zo_stride_of(const dc::Layout& L) { return (dc::zo_ill_off(L.D, L.T) + dc::zo_ill_len(L.T) + 1) & ~1; }

// dc_eval's hand-off buffer holds the prior workgroup's record only (the fixture sums travel
// through the accumulator rows, d_gacc)
int hb_stride_of(const bplhip_ctx* c) { return zo_stride_of(c->L); }
size_t gacc_bytes_of(const bplhip_ctx* c, int chains) {
    return (size_t)chains * 2 * dc::ga_set_words(c->L.T) * sizeof(long long);   // (two sets per chain)
}
// the partition a launch of `chains` chains uses: the short-stream one (part 0 of two) while its
// workgroups still find a CU each
void select_part(bplhip_ctx* c, int chains) {
    int pi = 0;
    if (c->n_parts > 1 && (long long)chains * (c->parts[0].n_wg + 1) > c->n_cu) pi = 1;
    c->ep = &c->parts[pi];
}

void drop_graphs(bplhip_ctx* c);

// Zero the arrival tickets and the accumulator rows.  Every completed launch leaves them zero
// (the last arriver re-arms both), so this matters after a growth and after a launch that did not
// complete (a fault, an aborted run): entry points that start a chain call it stream-ordered.
int reset_handoff(bplhip_ctx* c, hipStream_t s, bool sync) {
    if (c->slab_chains <= 0) return BPLHIP_OK;
    HIP_TRY(c, hipMemsetAsync(c->d_tickets.p, 0, (size_t)c->slab_chains * dc::TK_WORDS * sizeof(unsigned int), s));
    HIP_TRY(c, hipMemsetAsync(c->d_gacc.p, 0, gacc_bytes_of(c, c->slab_chains), s));
    if (sync) HIP_TRY(c, hipDeviceSynchronize());
    return BPLHIP_OK;
}

// Hand-off slabs and tickets for `chains` chains per launch.  Growing them frees the old buffers
// (hipFree waits for the device), so every cached hipGraphExec -- their kernel arguments hold the
// old pointers -- is dropped with them, and the fresh tickets are zeroed before anything can
// launch on any stream.
int ensure_slabs(bplhip_ctx* c, int chains) {
    select_part(c, chains);
    if (chains <= c->slab_chains) return BPLHIP_OK;
    drop_graphs(c);
    HIP_TRY(c, c->d_hbuf.ensure((size_t)chains * hb_stride_of(c) * sizeof(double)));
    HIP_TRY(c, c->d_tickets.ensure((size_t)chains * dc::TK_WORDS * sizeof(unsigned int)));
    HIP_TRY(c, c->d_gacc.ensure(gacc_bytes_of(c, chains)));
    c->slab_chains = chains;
    return reset_handoff(c, nullptr, true);
}

// the same at the start of a chain: also zero the tickets / rows a launch that never completed
// may have left armed
int ensure_slabs_fresh(bplhip_ctx* c, int chains, hipStream_t s) {
    const int rc = ensure_slabs(c, chains);
    return rc != BPLHIP_OK ? rc : reset_handoff(c, s, false);
}

size_t ctx_lds_bytes(const bplhip_ctx* c, bool staged) {
    return dc::eval_lds_bytes(c->L.T, c->L.D, c->L.K, zo_stride_of(c->L), staged);
}

template <bool W, bool C, bool S, bool N>
int launch_eval_n(bplhip_ctx* c, const dc::EvalArgs& A, int chains, hipStream_t s) {
    const dim3 grid(c->ep->n_wg + 1, chains), block(dc::BLOCK);
    const size_t lds = ctx_lds_bytes(c, S);
    if (lds > 48 * 1024) {  // (idempotent; only for large team counts)
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dc::dc_eval<W, C, S, N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    // (the leading arguments are the ones gfx950 preloads into SGPRs: dc_eval)
    hipLaunchKernelGGL((dc::dc_eval<W, C, S, N>), grid, block, lds, s, A.z, A.h, A.a, A.x, A.y,
                       (int)(A.L.T | (A.L.K << 16)), A.n_tiles, (int)(A.tiles_per_wave | (A.active_waves << 16)),
                       A.z_stride, A);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
template <bool W, bool C, bool S>
int launch_eval_s(bplhip_ctx* c, const dc::EvalArgs& A, int chains, hipStream_t s) {
    // the NUTS-aware instantiation is a separate kernel: the plain evaluation carries none
    // of its code (instruction-cache footprint matters at ~11 us per launch)
    return A.nuts ? launch_eval_n<W, C, S, true>(c, A, chains, s)
                  : launch_eval_n<W, C, S, false>(c, A, chains, s);
}
template <bool W, bool C>
int launch_eval_t(bplhip_ctx* c, const dc::EvalArgs& A, int chains, hipStream_t s) {
    return c->ep->staged ? launch_eval_s<W, C, true>(c, A, chains, s)
                     : launch_eval_s<W, C, false>(c, A, chains, s);
}

// Enqueue one (batched) evaluation: ONE launch.  No host sync.
int launch_eval_dynamic(bplhip_ctx* c, int chains, const double* z, double* pot, double* grad,
                        double* aux, hipStream_t s) {
    const dcd::DynLayout& L = c->DL;
    const size_t GT = (size_t)L.G * L.T;
    for (int ch = 0; ch < chains; ++ch) {  // chains run back to back
        dcd::DynArgs A{};
        A.h = c->d_h.as<const uint16_t>();
        A.a = c->d_a.as<const uint16_t>();
        A.x = c->d_x.as<const uint8_t>();
        A.y = c->d_y.as<const uint8_t>();
        A.gw = c->dd_gw.as<const uint16_t>();
        A.nv = c->dd_nv.as<const uint8_t>();
        A.n = c->n;
        A.xs = L.K ? c->d_xs.as<const double>() : nullptr;
        A.lgsum = c->lgsum;
        A.cells = c->dd_cells.as<double>();
        A.acc = c->dd_acc.as<double>();
        A.sc = A.acc + GT * dcd::A_N;
        A.gsum = A.sc + dcd::SC_N;
        A.red = A.gsum + 10 * (size_t)L.G;
        A.cov = A.red + dcd::R_N;
        A.grp = A.cov + 2 * (size_t)L.K;
        A.hyp = c->dd_hyp.as<double>();
        A.z = z + (size_t)ch * L.D;
        A.potential = pot + ch;
        A.grad = grad + (size_t)ch * L.D;
        A.aux = aux ? aux + (size_t)ch * 4 : nullptr;
        A.random_walk = c->dyn_random_walk;
        A.L = L;
        // fixture passes: at most 1024 workgroups of 16 waves (every workgroup ends with same-address
        // global atomics: maxima, U, its private accumulators); pass 2 takes contiguous chunks
        const int fb = c->n >= (1 << 18) ? dcd::FIX_BLOCK : 256;  // threads per workgroup
        const long long nb_all = (c->n + fb - 1) / fb;
        const int nb = (int)std::min<long long>(nb_all, 1024);
        A.chunk = ((c->n + nb - 1) / nb + fb - 1) / fb * fb;
        const int nb2 = (int)((c->n + A.chunk - 1) / A.chunk);
        const int cell_blocks = (L.T + dcd::CELL_BLOCK / 64 - 1) / (dcd::CELL_BLOCK / 64);
        A.scratch_n = dcd::scratch_doubles(L.G, L.T, L.K);
        A.gw_off = c->dd_gwoff.as<const int>();
        A.tickets = c->dd_tick.as<unsigned int>();
        A.fault = c->d_fault;
        A.gather = c->dyn_gather && c->opt_dyn_gather;
        A.fadj = c->dd_fadj.as<double>();
        A.inc_off = c->dd_inc_off.as<const int>();
        A.inc = c->dd_inc.as<const unsigned int>();
        const int team_blocks = (L.T + dcd::BACK_BLOCK / 64 - 1) / (dcd::BACK_BLOCK / 64);
        // one launch when every workgroup is resident and a wave spans all gameweeks
        // (and a workgroup's share of the fixtures is a few rounds of its threads)
        // ... and its workgroups wait for each other inside the launch (flagged cells, two grid barriers):
        // every one of them must be resident at once, on THIS device in its current compute partition
        if (c->dyn_fused_blocks_per_cu < 0) {
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, dcd::dyn_fused<false>, dcd::FUSED_DYN_BLOCK, 0) != hipSuccess)
                per_cu = 0;
            c->dyn_fused_blocks_per_cu = per_cu;
        }
        const bool co_resident = (long long)c->dyn_fused_blocks_per_cu * c->n_cu >= team_blocks;
        const bool fused_shape = c->opt_fused_small && c->dyn_fused_ok && L.G <= dcd::FUSED_DYN_MAX_G &&
                                 L.T <= dcd::FUSED_DYN_MAX_T;
        auto arm_scratch = [&]() -> int {
            if (!c->dyn_scratch_clean) {  // (the four-launch path leaves its scratch and its cells as it ends)
                HIP_TRY(c, hipMemsetAsync(A.acc, 0, A.scratch_n * 8, s));
                HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(A.cells), (int)dcd::CELL_EMPTY_WORD,
                                             GT * dcd::P_N * 2, s));
                c->dyn_scratch_clean = true;
            }
            return BPLHIP_OK;
        };
        if (fused_shape && co_resident && c->opt_dyn_big_wgs <= 0 &&
            c->n <= (long long)team_blocks * dcd::FUSED_DYN_BLOCK * 4) {
            if (int rc = arm_scratch()) return rc;
            hipLaunchKernelGGL(dcd::dyn_fused<false>, dim3(team_blocks), dim3(dcd::FUSED_DYN_BLOCK), 0, s, A);
            HIP_TRY(c, hipGetLastError());
            c->last_eval_path = A.gather ? BPLHIP_PATH_DYN_FUSED_GATHER : BPLHIP_PATH_DYN_FUSED_ATOMICS;
            continue;
        }
        if (fused_shape) {
            // more fixtures: the same single launch with `wpg` workgroups per gameweek, a gameweek's slice
            // of the fixtures each (its cell records, accumulators and rates in LDS) -- when the slices fit
            // and every workgroup is resident
            constexpr size_t STATIC_LDS = 24 * 1024;   // dyn_fused's own arrays (20.7 KB), rounded up
            const int want = c->opt_dyn_big_wgs > 0 ? c->opt_dyn_big_wgs : c->n_cu;
            bool launched = false;
            for (int mult = 1; mult <= 4 && !launched; ++mult) {
                const int wpg = std::max(1, want * mult / L.G);
                const int nbig = std::max(team_blocks, wpg * L.G);
                const long long cap = (c->dyn_max_gw + wpg - 1) / wpg;
                if (cap > (1 << 24)) continue;
                // (the slice's fixture words in LDS too when they fit beside its rates)
                const bool stage = dcd::fused_big_lds_bytes(L.T, (int)cap, true) + STATIC_LDS <= LDS_LIMIT;
                const size_t lds = dcd::fused_big_lds_bytes(L.T, (int)cap, stage);
                if (lds + STATIC_LDS > LDS_LIMIT) continue;
                if (!c->dyn_big_attr_set) {
                    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcd::dyn_fused<true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)(LDS_LIMIT - STATIC_LDS)));
                    c->dyn_big_attr_set = true;
                }
                if (c->dyn_big_lds != lds) {
                    int per_cu = 0;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, dcd::dyn_fused<true>,
                                                                     dcd::FUSED_DYN_BLOCK, lds) != hipSuccess)
                        per_cu = 0;
                    c->dyn_big_lds = lds;
                    c->dyn_big_blocks_per_cu = per_cu;
                }
                if ((long long)c->dyn_big_blocks_per_cu * c->n_cu < nbig) continue;
                if (int rc = arm_scratch()) return rc;
                A.wpg = wpg;
                A.rate_cap = (int)cap;
                A.fx8 = c->dd_fx8.as<const unsigned long long>();
                A.stage_fx = stage ? 1 : 0;
                hipLaunchKernelGGL(dcd::dyn_fused<true>, dim3(nbig), dim3(dcd::FUSED_DYN_BLOCK), lds, s, A);
                HIP_TRY(c, hipGetLastError());
                c->last_eval_path = BPLHIP_PATH_DYN_SLICED;
                launched = true;
            }
            if (launched) continue;
        }
        if (!c->dyn_attr_set) {
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcd::dyn_pass2),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           dcd::PASS2_LDS_CELLS * dcd::A_N * 8));
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcd::dyn_back),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)dcd::back_lds_bytes(dcd::BACK_LDS_G)));
            c->dyn_attr_set = true;
            c->lds_attr_set = true;
        }
        c->dyn_scratch_clean = false;
        hipLaunchKernelGGL(dcd::dyn_cells, dim3(cell_blocks), dim3(dcd::CELL_BLOCK), 0, s, A);
        hipLaunchKernelGGL(dcd::dyn_pass1, dim3(nb), dim3(fb), 0, s, A);
        hipLaunchKernelGGL(dcd::dyn_pass2, dim3(nb2), dim3(fb),
                           (size_t)dcd::PASS2_LDS_CELLS * dcd::A_N * 8, s, A);
        hipLaunchKernelGGL(dcd::dyn_back, dim3(team_blocks), dim3(dcd::BACK_BLOCK),
                           dcd::back_lds_bytes(L.G), s, A);
        HIP_TRY(c, hipGetLastError());
        c->last_eval_path = BPLHIP_PATH_DYN_MULTI;
    }
    return BPLHIP_OK;
}

// the neutral model's single-launch kernel can take the NUTS leaf with it (nuts_state != nullptr)
bool neutral_leaf_fusable(const bplhip_ctx* c) {
    return c->neutral && c->opt_fused_small && c->neu_fusable && c->NL.D <= 64 * nd::LEAF_NE_MAX &&
           (dcn::fused_lds_doubles(c->NL, c->n, c->neu_slots) + dcn::fused_leaf_doubles(c->NL)) * 8 <= LDS_LIMIT;
}
int launch_eval_neutral(bplhip_ctx* c, int chains, const double* z, double* pot, double* grad,
                        double* aux, hipStream_t s, double* nuts_state = nullptr, size_t nuts_stride = 0,
                        int nuts_depth = 0, const nd::Persist* persist = nullptr) {
    const dcn::NeuLayout& L = c->NL;
    if (c->opt_fused_small && c->neu_fusable) {  // one workgroup per chain, one launch for all of them
        dcn::FusedArgs A{};
        A.L = L;
        A.n = (int)c->n;
        A.fx = c->dd_fpack.as<const dcn::FusedFixture>();
        A.n_slots = c->neu_slots;
        A.sched = c->dd_sched.as<const uint32_t>();
        A.slot_off = c->dd_slot_off.as<const int>();
        A.xs = L.K ? c->d_xs.as<const double>() : nullptr;
        A.lgsum = c->lgsum;
        A.z = z;
        A.potential = pot;
        A.grad = grad;
        A.aux = aux;
        A.stop_after = c->opt_debug_stop;
        if (!c->neu_attr_set) {
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcn::neu_fused<false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcn::neu_fused<true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT));
            c->neu_attr_set = true;
        }
        if (nuts_state) {  // persistent chains: one launch evaluates AND books the leapfrog of every chain
            A.nuts = nuts_state;
            A.nuts_stride = nuts_stride;
            A.max_depth = nuts_depth;
            A.persist = *persist;
            hipLaunchKernelGGL(dcn::neu_fused<true>, dim3(chains), dim3(dcn::FUSED_BLOCK),
                               (dcn::fused_lds_doubles(L, c->n, c->neu_slots) + dcn::fused_leaf_doubles(L)) * 8, s, A);
            HIP_TRY(c, hipGetLastError());
            c->last_eval_path = BPLHIP_PATH_NEU_FUSED;
            return BPLHIP_OK;
        }
        hipLaunchKernelGGL(dcn::neu_fused<false>, dim3(chains), dim3(dcn::FUSED_BLOCK),
                           dcn::fused_lds_doubles(L, c->n, c->neu_slots) * 8, s, A);
        HIP_TRY(c, hipGetLastError());
        c->last_eval_path = BPLHIP_PATH_NEU_FUSED;
        return BPLHIP_OK;
    }
    for (int ch = 0; ch < chains; ++ch) {  // multi-launch path: chains run back to back
        dcn::NeuArgs A{};
        dcd::DynArgs& F = A.F;
        F.h = c->d_h.as<const uint16_t>();
        F.a = c->d_a.as<const uint16_t>();
        F.x = c->d_x.as<const uint8_t>();
        F.y = c->d_y.as<const uint8_t>();
        F.gw = nullptr;
        F.nv = c->dd_nv.as<const uint8_t>();
        F.w = c->weighted ? c->d_w.as<const float>() : nullptr;
        F.n = c->n;
        F.xs = L.K ? c->d_xs.as<const double>() : nullptr;
        F.lgsum = c->lgsum;
        F.cells = c->dd_cells.as<double>();
        F.acc = c->dd_acc.as<double>();
        F.sc = F.acc + (size_t)L.T * dcd::A_N;
        F.cacc = F.sc + dcd::SC_N;
        F.n_conf = L.C;
        F.hc = L.C ? c->dd_hc.as<const uint8_t>() : nullptr;
        F.ac = L.C ? c->dd_ac.as<const uint8_t>() : nullptr;
        F.cs = z + (size_t)ch * L.D + L.o_conf;
        F.z = z + (size_t)ch * L.D;
        F.potential = pot + ch;
        F.grad = grad + (size_t)ch * L.D;
        F.aux = aux ? aux + (size_t)ch * 4 : nullptr;
        F.L.G = 1;
        F.L.T = L.T;
        F.L.K = L.K;
        F.L.o_corr = L.o_corr;
        A.L = L;
        F.scratch_n = (size_t)L.T * dcd::A_N + dcd::SC_N + L.C;
        F.tickets = c->dd_tick.as<unsigned int>();
        F.fault = c->d_fault;
        if (c->opt_fused_small && c->dyn_fused_ok && F.tickets) {
            // one launch (dcn::neu_big): a slice of the fixtures per workgroup, one workgroup per CU, when the
            // slice's rates fit the LDS and every workgroup is resident
            constexpr size_t STATIC_LDS = 2 * 1024;
            const int want = c->opt_dyn_big_wgs > 0 ? c->opt_dyn_big_wgs : c->n_cu;
            const int nbig = (int)std::max<long long>(1, std::min<long long>(want, (c->n + dcn::NEU_BIG_BLOCK - 1) / dcn::NEU_BIG_BLOCK));
            const long long cap = (c->n + nbig - 1) / nbig;
            const size_t lds = dcn::big_lds_bytes(L, cap);
            if (lds + STATIC_LDS <= LDS_LIMIT) {
                if (!c->neu_big_attr_set) {
                    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcn::neu_big),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)(LDS_LIMIT - STATIC_LDS)));
                    c->neu_big_attr_set = true;
                }
                if (c->dyn_big_lds != lds) {
                    int per_cu = 0;
                    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, dcn::neu_big, dcn::NEU_BIG_BLOCK, lds) != hipSuccess)
                        per_cu = 0;
                    c->dyn_big_lds = lds;
                    c->dyn_big_blocks_per_cu = per_cu;
                }
                if ((long long)c->dyn_big_blocks_per_cu * c->n_cu >= nbig) {
                    if (!c->dyn_scratch_clean) {  // (the multi-launch path leaves its scratch as it ends)
                        HIP_TRY(c, hipMemsetAsync(F.acc, 0, F.scratch_n * 8 * dcn::NEU_BIG_GROUPS, s));
                        c->dyn_scratch_clean = true;
                    }
                    F.rate_cap = (int)cap;
                    A.fxp = c->dd_fpack.as<const dcn::FusedFixture>();
                    if (c->neu_runs_nb != nbig) {   // per-run arithmetic: every wave's part must fit its run table
                        constexpr int WV = dcn::NEU_BIG_BLOCK / 64;
                        bool ok = (long long)c->neu_keys.size() == c->n &&
                                  (size_t)WV * dcn::NEU_RUNS_MAX * dcn::NEU_RUN_W <= 2 * (size_t)cap;
                        for (int b = 0; ok && b < nbig; ++b) {
                            const long long i_lo = std::min<long long>((long long)b * cap, c->n), i_hi = std::min<long long>(i_lo + cap, c->n);
                            const long long n_mine = i_hi - i_lo, per_wave = (n_mine + WV - 1) / WV;
                            for (int w = 0; ok && w < WV; ++w) {
                                const long long w0 = std::min<long long>(w * per_wave, n_mine), w1 = std::min<long long>(w0 + per_wave, n_mine);
                                int runs = 0;
                                // (a wave counts a run per step-aligned piece as well: one per key change, plus one where a
                                // 64-fixture step that straddles runs ends inside a run -- bounded by twice the key changes + 1)
                                for (long long i = w0; i < w1; ++i)
                                    runs += i == w0 || c->neu_keys[i_lo + i] != c->neu_keys[i_lo + i - 1];
                                ok = 2 * runs + 1 <= dcn::NEU_RUNS_MAX;
                            }
                        }
                        c->neu_runs_ok = ok;
                        c->neu_runs_nb = nbig;
                    }
                    A.runs = c->neu_runs_ok && c->opt_neu_runs;
                    hipLaunchKernelGGL(dcn::neu_big, dim3(nbig), dim3(dcn::NEU_BIG_BLOCK), lds, s, A);
                    HIP_TRY(c, hipGetLastError());
                    c->last_eval_path = A.runs ? BPLHIP_PATH_NEU_BIG_RUNS : BPLHIP_PATH_NEU_BIG_FIXTURE;
                    continue;
                }
            }
        }
        c->dyn_scratch_clean = false;
        const int fb = c->n >= (1 << 18) ? dcd::FIX_BLOCK : 256;  // threads per workgroup
        const long long nb_all = (c->n + fb - 1) / fb;
        const int nb = (int)std::min<long long>(nb_all, 1024);
        F.chunk = ((c->n + nb - 1) / nb + fb - 1) / fb * fb;
        const int nb2 = (int)((c->n + F.chunk - 1) / F.chunk);
        hipLaunchKernelGGL(dcn::neu_cells, dim3((L.T + 255) / 256), dim3(256), 0, s, A);
        if (!c->lds_attr_set) {
            HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcd::dyn_pass2),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           dcd::PASS2_LDS_CELLS * dcd::A_N * 8));
            c->lds_attr_set = true;
        }
        hipLaunchKernelGGL(dcd::dyn_pass1, dim3(nb), dim3(fb), 0, s, F);
        hipLaunchKernelGGL(dcd::dyn_pass2, dim3(nb2), dim3(fb),
                           (size_t)dcd::PASS2_LDS_CELLS * dcd::A_N * 8, s, F);
        hipLaunchKernelGGL(dcn::neu_epilogue, dim3(1), dim3(dcn::NEU_EPI),
                           (size_t)(dcn::NEU_SUMS + 2 * L.K) * 8, s, A);
        HIP_TRY(c, hipGetLastError());
        c->last_eval_path = BPLHIP_PATH_NEU_MULTI;
    }
    return BPLHIP_OK;
}

dc::EvalArgs eval_args(bplhip_ctx* c, int chains, const double* z, double* pot, double* grad,
                       double* aux) {
    dc::EvalArgs A{};
    A.h = c->d_h.as<const uint32_t>();
    A.a = c->d_a.as<const uint32_t>();
    A.x = c->d_x.as<const uint32_t>();
    A.y = c->d_y.as<const uint32_t>();
    A.w = c->weighted ? c->d_w.as<const float>() : nullptr;
    A.n_tiles = c->n_tiles;
    A.active_waves = c->ep->aw;
    A.tiles_per_wave = c->ep->tpw;
    A.pairs = c->d_pairs.as<const uint32_t>();
    A.pairw = c->d_pairw.as<const double>();
    A.pairc = c->d_pairc.as<const double>();
    A.w11 = c->w11;
    A.P = c->P;
    A.dense_pairs = c->opt_dense_pairs && c->pairs_complete && c->P >= dc::DENSE_MIN_PAIRS;
    A.xs = c->L.K ? c->d_xs.as<const double>() : nullptr;
    A.xsf = c->L.K ? c->d_xsf.as<const float>() : nullptr;
    A.cA = c->d_cA.as<const double>();
    A.cD = c->d_cD.as<const double>();
    A.cH = c->d_cH.as<const double>();
    A.lgsum = c->lgsum;
    A.wg_off = c->ep->d_wg_off.as<const int>();
    A.wg_slots = c->ep->d_wg_slots.as<const int>();
    A.col_off = c->ep->d_col_off.as<const int>();
    A.wg_dst = c->ep->d_wg_dst.as<const int>();
    A.total_c = c->ep->total_c;
    A.hbuf = c->d_hbuf.as<double>();
    A.hb_stride = hb_stride_of(c);
    A.n_wg = c->ep->n_wg;
    A.zo_stride = zo_stride_of(c->L);
    A.tickets = c->d_tickets.as<unsigned int>();
    A.gacc = c->d_gacc.as<long long>();
    A.ga_expect = c->ep->d_ga_expect.as<const int>();
    A.chains = chains;
    A.z = z;
    A.potential = pot;
    A.grad = grad;
    A.aux = aux;
    A.z_stride = c->L.D;
    A.g_stride = c->L.D;
    A.p_stride = 1;
    A.aux_stride = 4;
    A.debug = c->d_debug.as<unsigned long long>();
    A.fault = c->d_fault;
    A.L = c->L;
    return A;
}

int launch_eval(bplhip_ctx* c, int chains, const double* z, double* pot, double* grad,
                double* aux, hipStream_t s, double* nuts_state = nullptr, int nuts_depth = 0,
                const nd::Persist* persist = nullptr, int nuts_stride = 0) {
    if (c->neutral) return launch_eval_neutral(c, chains, z, pot, grad, aux, s);
    if (c->dynamic) return launch_eval_dynamic(c, chains, z, pot, grad, aux, s);
    c->last_eval_path = BPLHIP_PATH_LEAGUE;
    select_part(c, chains);
    dc::EvalArgs A = eval_args(c, chains, z, pot, grad, aux);
    A.nuts = nuts_state;
    A.nuts_max_depth = nuts_depth;
    A.persist = persist;
    if (nuts_state && nuts_stride) {  // several chains (grid.y): everything lives in the state buffers
        A.nuts_stride = nuts_stride;
        A.z_stride = A.g_stride = A.p_stride = A.aux_stride = nuts_stride;
    }
    const bool clip = c->L.model == dc::MODEL_EXTENDED;
    if (c->weighted) return clip ? launch_eval_t<true, true>(c, A, chains, s)
                                 : launch_eval_t<true, false>(c, A, chains, s);
    return clip ? launch_eval_t<false, true>(c, A, chains, s)
                : launch_eval_t<false, false>(c, A, chains, s);
}

// ---- persistent evaluation kernel (dc_eval_loop): up to `steps` leapfrogs of ONE device-resident
// chain in one launch.  Needs the leaf in the tail (basic / extended, <= 64 teams) and a grid that
// is co-resident (one workgroup per CU).
bool loop_ok(const bplhip_ctx* c) {
    if (c->dynamic || c->neutral || !c->opt_persistent_kernel) return false;
    const bplhip_ctx::EvalPart& ep = c->parts[0];
    // (the leaf's vectors live in registers / LDS lanes there: two elements per lane at most)
    return ep.staged && ep.n_wg + 1 <= c->n_cu && ctx_lds_bytes(c, true) <= 64 * 1024 && c->L.D <= 128;
}
template <bool W, bool C, int LNE>
int launch_loop_l(bplhip_ctx* c, const dc::EvalArgs& A, hipStream_t s) {
    const size_t lds = ctx_lds_bytes(c, true);
    if (lds > 48 * 1024)
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dc::dc_eval_loop<W, C, LNE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((dc::dc_eval_loop<W, C, LNE>), dim3(c->ep->n_wg + 1, 1), dim3(dc::BLOCK), lds, s, A);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
template <bool W, bool C>
int launch_loop_t(bplhip_ctx* c, const dc::EvalArgs& A, hipStream_t s) {
    // the leaf's vectors in registers: one element per lane up to 64 latent entries, two up to 128
    // (the extended model: 3T + 2K + 7); beyond, the LDS-staged leaf of the one-element kernel
    if (c->L.D > 64) {
        c->last_nuts_engine = BPLHIP_ENGINE_LOOP_LNE2;
        return launch_loop_l<W, C, 2>(c, A, s);
    }
    c->last_nuts_engine = BPLHIP_ENGINE_LOOP_LNE1;
    return launch_loop_l<W, C, 1>(c, A, s);
}
int launch_eval_loop(bplhip_ctx* c, double* ns, int nuts_depth, const nd::Persist* persist, int steps,
                     hipStream_t s) {
    const int D = c->L.D;
    select_part(c, 1);
    if (c->d_zb.bytes < (size_t)D * 8 || c->loop_tag > 0xF0000000u) {  // fresh granules: tag 0 everywhere
        HIP_TRY(c, c->d_zb.ensure((size_t)D * 8));
        HIP_TRY(c, hipMemsetAsync(c->d_zb.p, 0, (size_t)D * 8, s));
        c->loop_tag = 0;
    }
    dc::EvalArgs A = eval_args(c, 1, nd::vec(ns, D, nd::V_ZN), ns + nd::H_LEAF_PE, nd::vec(ns, D, nd::V_GRAD),
                               ns + nd::H_LEAF_AUX0);
    A.tag_base = c->loop_tag;
    c->loop_tag += (unsigned int)steps + 2u;  // steps + the launch's own "finished" tag
    A.nuts = ns;
    A.nuts_max_depth = nuts_depth;
    A.persist = persist;
    A.persist_steps = steps;
    A.persist_spec = c->opt_persist_spec;
    A.zg = c->d_zb.as<unsigned long long>();
    const bool clip = c->L.model == dc::MODEL_EXTENDED;
    if (c->weighted) return clip ? launch_loop_t<true, true>(c, A, s) : launch_loop_t<true, false>(c, A, s);
    return clip ? launch_loop_t<false, true>(c, A, s) : launch_loop_t<false, false>(c, A, s);
}

// ---- chain-vectorised evaluation (dc_vec.hip.h): stream launch + tail launch
int vec_hb_stride(const bplhip_ctx* c) {
    return (zo_stride_of(c->L) + c->vp->n_wg * dc::N_SCAL + c->vp->total_c + 1) & ~1;
}
size_t vec_tail_lds(const bplhip_ctx* c, bool staged) {
    return dc::tail_lds_bytes(c->L.T, c->L.D, c->L.K, zo_stride_of(c->L), c->vp->n_wg, c->vp->total_c, staged);
}
template <bool S, bool N, bool E>
int launch_vec_tail(bplhip_ctx* c, const dc::EvalArgs& A, int chains, hipStream_t s) {
    const size_t tl = vec_tail_lds(c, S);
    if (tl > 48 * 1024)
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dc::dc_vec_tail<S, N, E>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)tl));
    hipLaunchKernelGGL((dc::dc_vec_tail<S, N, E>), dim3(chains), dim3(dc::BLOCK), tl, s, A);
    return BPLHIP_OK;
}
template <bool W, bool C, bool N>
int launch_vec_n(bplhip_ctx* c, const dc::EvalArgs& A, int chains, hipStream_t s) {
    const int groups = (chains + dc::CB - 1) / dc::CB;
    const size_t lds = std::max(dc::vec_stream_lds_bytes(c->L.T), dc::prior_lds_bytes(c->L.T));
    if (lds > 48 * 1024)
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dc::dc_vec_stream<W, C, N>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((dc::dc_vec_stream<W, C, N>), dim3(dc::CB + c->vp->n_wg, groups),
                       dim3(dc::BLOCK), lds, s, A);
    const int rc = c->vp->staged ? launch_vec_tail<true, N, C>(c, A, chains, s)
                                : launch_vec_tail<false, N, C>(c, A, chains, s);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
template <bool W, bool C>
int launch_vec_t(bplhip_ctx* c, const dc::EvalArgs& A, int chains, hipStream_t s) {
    return A.nuts ? launch_vec_n<W, C, true>(c, A, chains, s)
                  : launch_vec_n<W, C, false>(c, A, chains, s);
}
// nuts != nullptr: lock-step device NUTS; chain c's state at nuts + c*nuts_stride, and
// z / pot / grad / aux point into chain 0's state (strides = nuts_stride)
// select the partition for `chains` chains and size its hand-off buffer.  Growing it is a hipMalloc
// (+ hipFree): not allowed while a stream of this thread is capturing -- whoever captures launches of
// the vectorised kernel sizes it first (round 3 did not: every sampler run with more chains than
// gridy_max_chains on a fresh context failed inside the chunk graph's capture).
int prepare_vec(bplhip_ctx* c, int chains) {
    // The thinnest partition whose grid still fits the chip in (about) one round -- groups x workgroups + one
    // prior workgroup per chain <= CUs: tiles per wave set the launch's length as long as nobody queues behind
    // another workgroup (measured, N = 1e6, us per launch at 1x / 2x / 3x / 4x tiles per wave: 8 chains 10.4 /
    // 12.9 / 14.6 / 15.8, 32 chains 12.7 / 13.2 / 14.5 / 16.1, 64 chains 17.0 / 16.3 / 14.9 / 16.3, 128 chains
    // 21.7 / 22.3 / 19.0 / 21.7, 256 chains 32.8 / 30.1 / 30.0 / 31.6: profiles/r04/vec_tiles_per_wave.txt.
    // Round 3 took 1x / 2x / 4x by chain count alone: 4x at 32 and at 64 chains).
    {
        const int groups = (chains + dc::CB - 1) / dc::CB;
        int pi = 2;
        for (int k = 0; k < 3; ++k)
            if ((long long)groups * c->vps[k].n_wg + chains <= c->n_cu + c->n_cu / 8) {   // (a few workgroups over: still one round)
                pi = k;
                break;
            }
        c->vp = &c->vps[pi];
    }
    if (chains > c->vp->slab_chains) {
        if (c->capturing)
            return fail(c, BPLHIP_ESTATE, "dc_vec: hand-off buffer for %d chains not sized before the capture", chains);
        HIP_TRY(c, c->vp->d_hbuf.ensure((size_t)chains * vec_hb_stride(c) * sizeof(double)));
        c->vp->slab_chains = chains;
    }
    return BPLHIP_OK;
}
int launch_eval_vec(bplhip_ctx* c, int chains, const double* z, double* pot, double* grad,
                    double* aux, hipStream_t s, double* nuts = nullptr, int nuts_stride = 0,
                    int nuts_depth = 0, const nd::Persist* persist = nullptr) {
    {
        const int prc = prepare_vec(c, chains);
        if (prc != BPLHIP_OK) return prc;
    }
    dc::EvalArgs A = eval_args(c, chains, z, pot, grad, aux);
    c->last_eval_path = BPLHIP_PATH_LEAGUE;
    if (nuts) {
        A.nuts = nuts;
        A.nuts_stride = nuts_stride;
        A.nuts_max_depth = nuts_depth;
        A.persist = persist;
        A.z_stride = A.g_stride = A.p_stride = A.aux_stride = nuts_stride;
    }
    A.tiles_per_wave = c->vp->tpw;
    A.wg_off = c->vp->d_wg_off.as<const int>();
    A.wg_slots = c->vp->d_wg_slots.as<const int>();
    A.col_off = c->vp->d_col_off.as<const int>();
    A.wg_dst = c->vp->d_wg_dst.as<const int>();
    A.total_c = c->vp->total_c;
    A.hbuf = c->vp->d_hbuf.as<double>();
    A.hb_stride = vec_hb_stride(c);
    A.n_wg = c->vp->n_wg;
    A.tickets = nullptr;
    const bool clip = c->L.model == dc::MODEL_EXTENDED;
    if (c->weighted) return clip ? launch_vec_t<true, true>(c, A, chains, s)
                                 : launch_vec_t<true, false>(c, A, chains, s);
    return clip ? launch_vec_t<false, true>(c, A, chains, s)
                : launch_vec_t<false, false>(c, A, chains, s);
}

bool vec_ok(const bplhip_ctx* c) {
    return !c->dynamic && !c->neutral && c->vps[0].ok && c->vps[1].ok && c->vps[2].ok;
}
bool use_vec(const bplhip_ctx* c, int chains) {
    return vec_ok(c) && c->opt_vec_min_chains > 0 && chains >= c->opt_vec_min_chains;
}

// Static sparse-slab structure: which of the 3T per-team slots each streaming workgroup's
// fixtures touch (att[h], ha[h], def[a], att[a], def[h]), and the transposed (per column,
// workgroup order) position lists for the tail's reduction.
struct SparseSlabs {
    std::vector<int> wg_off, wg_slots, col_off, wg_dst;
};
// tiles_per_wg: contiguous tiles of one workgroup
SparseSlabs build_sparse_slabs(const std::vector<uint16_t>& hs, const std::vector<uint16_t>& as,
                               int64_t n, int T, int tiles_per_wg, int n_wg) {
    SparseSlabs o;
    o.wg_off.assign(n_wg + 1, 0);
    o.col_off.assign(3 * T + 1, 0);
    std::vector<char> touched(3 * (size_t)T);
    const int64_t per_wg = (int64_t)tiles_per_wg * dc::TILE;
    for (int w = 0; w < n_wg; ++w) {
        std::fill(touched.begin(), touched.end(), 0);
        const int64_t r0 = (int64_t)w * per_wg, r1 = std::min<int64_t>(n, r0 + per_wg);
        for (int64_t r = r0; r < r1; ++r) {
            const int hh = hs[r], aa = as[r];
            touched[hh] = touched[2 * T + hh] = touched[T + aa] = 1;
            touched[aa] = touched[T + hh] = 1;
        }
        for (int sidx = 0; sidx < 3 * T; ++sidx)
            if (touched[sidx]) o.wg_slots.push_back(sidx);
        o.wg_off[w + 1] = (int)o.wg_slots.size();
    }
    const int total = (int)o.wg_slots.size();
    for (int k = 0; k < total; ++k) o.col_off[o.wg_slots[k] + 1] += 1;
    for (int cidx = 0; cidx < 3 * T; ++cidx) o.col_off[cidx + 1] += o.col_off[cidx];
    o.wg_dst.resize(std::max(total, 1));
    std::vector<int> fill(o.col_off.begin(), o.col_off.end() - 1);
    for (int k = 0; k < total; ++k) o.wg_dst[k] = fill[o.wg_slots[k]]++;  // k ascending = wg order
    if (o.wg_slots.empty()) o.wg_slots.push_back(0);
    return o;
}

void drop_graphs(bplhip_ctx* c) {  // (declared above ensure_slabs)
    for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second);
    c->graphs.clear();
}

// Capture what `enqueue(stream)` launches into an executable graph.  A capture is an optimisation,
// never a requirement: whatever goes wrong inside it (a launch path that wanted to allocate, an API
// the runtime refuses while capturing, an instantiation failure) ends the capture, clears the
// runtime's error state and returns nullptr with BPLHIP_OK -- the caller then enqueues the same
// launches one by one.  Callers run the launches ONCE un-captured first, so that everything a launch
// path sizes or sets lazily (buffers, function attributes, occupancy queries) is settled.
template <class F>
int capture_launches(bplhip_ctx* c, F&& enqueue, hipGraphExec_t* out) {
    *out = nullptr;
    if (!c->cap_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    if (hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return BPLHIP_OK;
    }
    c->capturing = true;
    const bool dyn_clean = c->dyn_scratch_clean;
    const int crc = enqueue(c->cap_stream);
    c->capturing = false;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(c->cap_stream, &g);
    hipGraphExec_t ge = nullptr;
    if (crc == BPLHIP_OK && e == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
        (void)hipGraphDestroy(g);
        *out = ge;
        return BPLHIP_OK;
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    c->dyn_scratch_clean = dyn_clean;   // (a captured memset never ran)
    return BPLHIP_OK;
}

}  // namespace

// The C-ABI never lets a C++ exception escape (std::bad_alloc from a host buffer, std::system_error
// from a host thread, ...): the entry points that allocate run inside this guard.

// A raised fault word: name it, put the hand-off state back (counters, accumulator rows, the dynamic
// model's scratch) and report.  The device is idle or running work that no longer matters when this
// is called from an entry point; from inside a sampler it is called right after a stream sync.
static int consume_fault(bplhip_ctx* c, const char* where) {
    if (!c || !c->h_fault) return BPLHIP_OK;
    const unsigned int f = __atomic_load_n(c->h_fault, __ATOMIC_RELAXED);
    if (f == 0u) return BPLHIP_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    __atomic_store_n(c->h_fault, 0u, __ATOMIC_RELAXED);
    (void)reset_handoff(c, nullptr, true);
    if (f & dc::FAULT_DYN_BARRIER) {
        c->dyn_fused_ok = false;
        c->dyn_scratch_clean = false;
        if (c->dd_tick.p) (void)hipMemset(c->dd_tick.p, 0, c->dd_tick.bytes);
    }
    return fail(c, BPLHIP_EHIP,
                "%s: a device-side hand-off timed out (fault word 0x%x:%s%s%s%s); outputs of the affected evaluations are "
                "NaN, the hand-off state has been reset%s",
                where, f, (f & dc::FAULT_EVAL_ARRIVALS) ? " dc_eval arrivals" : "",
                (f & dc::FAULT_LOOP_ARRIVALS) ? " dc_eval_loop arrivals" : "",
                (f & dc::FAULT_LOOP_GRANULES) ? " dc_eval_loop granules" : "",
                (f & dc::FAULT_DYN_BARRIER) ? " dyn_fused barrier" : (f & nd::FAULT_LEAF_BARRIER) ? " wide leaf row barrier" : "",
                (f & dc::FAULT_DYN_BARRIER) ? ", the dynamic model uses its four-launch path from now on" : "");
}

template <class F>
static int guarded(bplhip_ctx* c, const char* where, F&& body) {
    try {
        int rc = consume_fault(c, where);   // raised by asynchronous work of an earlier call
        if (rc != BPLHIP_OK) return rc;
        rc = body();
        return rc != BPLHIP_OK ? rc : consume_fault(c, where);
    } catch (const std::bad_alloc&) {
        return c ? fail(c, BPLHIP_ENOMEM, "%s: out of host memory", where) : BPLHIP_ENOMEM;
    } catch (const std::exception& e) {
        return c ? fail(c, BPLHIP_EHIP, "%s: %s", where, e.what()) : BPLHIP_EHIP;
    } catch (...) {
        return c ? fail(c, BPLHIP_EHIP, "%s: unknown C++ exception", where) : BPLHIP_EHIP;
    }
}

extern "C" {

int bplhip_abi_version(void) { return BPLHIP_ABI_VERSION; }

static int bplhip_create_impl(bplhip_ctx** out, int device_id) {
    if (!out) return fail(nullptr, BPLHIP_EINVAL, "bplhip_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, BPLHIP_EHIP, "bplhip_create: no HIP device (%s)",
                    e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev)
        return fail(nullptr, BPLHIP_EINVAL, "bplhip_create: device %d out of range [0,%d)",
                    device_id, ndev);
    e = hipSetDevice(device_id);
    if (e != hipSuccess)
        return fail(nullptr, BPLHIP_EHIP, "hipSetDevice(%d): %s", device_id,
                    hipGetErrorString(e));
    bplhip_ctx* c = new (std::nothrow) bplhip_ctx();
    if (!c) return fail(nullptr, BPLHIP_ENOMEM, "bplhip_create: out of host memory");
    c->device = device_id;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0)
        c->n_cu = cus;
    void* hf = nullptr;
    void* df = nullptr;
    if (hipHostMalloc(&hf, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&df, hf, 0) != hipSuccess) {
        if (hf) (void)hipHostFree(hf);
        delete c;
        return fail(nullptr, BPLHIP_EHIP, "bplhip_create: cannot map the fault word");
    }
    std::memset(hf, 0, 64);
    c->h_fault = static_cast<unsigned int*>(hf);
    c->d_fault = static_cast<unsigned int*>(df);
    *out = c;
    return BPLHIP_OK;
}

void bplhip_destroy(bplhip_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();  // (nothing may write the fault word after it is unmapped)
    if (ctx->h_fault) (void)hipHostFree(ctx->h_fault);
    delete ctx;
}

const char* bplhip_last_error(const bplhip_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

static int bplhip_set_fixtures_impl(bplhip_ctx* c, int model_kind, int64_t n, int32_t n_teams,
                        const uint16_t* home_idx, const uint16_t* away_idx,
                        const uint8_t* home_goals, const uint8_t* away_goals,
                        const float* weights, const double* covariates, int32_t k,
                        void* stream) {
    if (!c) return BPLHIP_EINVAL;
    c->bound = false;
    c->last_eval_path = BPLHIP_PATH_NONE;
    c->last_nuts_engine = BPLHIP_ENGINE_NONE;
    c->dynamic = false;
    c->neutral = false;
    if (model_kind != BPLHIP_MODEL_BASIC && model_kind != BPLHIP_MODEL_EXTENDED)
        return fail(c, BPLHIP_EINVAL, "set_fixtures: unknown model_kind %d", model_kind);
    if (n < 1 || n > (int64_t)1 << 40)
        return fail(c, BPLHIP_EINVAL, "set_fixtures: n=%lld must be >= 1", (long long)n);
    if (n_teams < 1 || n_teams > 65534)
        return fail(c, BPLHIP_EINVAL, "set_fixtures: n_teams=%d out of range [1,65534]", n_teams);
    if (!home_idx || !away_idx || !home_goals || !away_goals)
        return fail(c, BPLHIP_EINVAL, "set_fixtures: null fixture array");
    if (k < 0 || (k > 0 && !covariates) || (k == 0 && covariates))
        return fail(c, BPLHIP_EINVAL, "set_fixtures: covariates/k mismatch (k=%d)", k);
    if (model_kind == BPLHIP_MODEL_BASIC && (k != 0 || weights))
        return fail(c, BPLHIP_EINVAL,
                    "set_fixtures: the basic model takes neither covariates nor weights");
    if (dc::stream_lds_bytes(n_teams) > LDS_LIMIT || dc::prior_lds_bytes(n_teams) > LDS_LIMIT)
        return fail(c, BPLHIP_EUNSUPPORTED,
                    "set_fixtures: n_teams=%d exceeds the LDS-resident table limit", n_teams);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);

    // ---- read the caller's device arrays once
    std::vector<uint16_t> h(n), a(n);
    std::vector<uint8_t> x(n), y(n);
    std::vector<float> w;
    HIP_TRY(c, hipMemcpyAsync(h.data(), home_idx, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(a.data(), away_idx, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(x.data(), home_goals, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(y.data(), away_goals, n, hipMemcpyDeviceToHost, s));
    if (weights) {
        w.resize(n);
        HIP_TRY(c, hipMemcpyAsync(w.data(), weights, n * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    for (int64_t i = 0; i < n; ++i)
        if (h[i] >= n_teams || a[i] >= n_teams)
            return fail(c, BPLHIP_EINVAL, "set_fixtures: team index out of range at fixture %lld",
                        (long long)i);

    // ---- sort by (home, away): runs of equal pairs become contiguous, so a wave-tile
    // reduces to one (or a few) per-pair sums.  Stable, so equal pairs keep input order.
    std::vector<uint64_t> order(n);
    for (int64_t i = 0; i < n; ++i)
        order[i] = ((uint64_t)h[i] << 48) | ((uint64_t)a[i] << 32) | (uint64_t)(uint32_t)i;
    if (n > (int64_t)0xFFFFFFFF) return fail(c, BPLHIP_EUNSUPPORTED, "set_fixtures: n too large");
    std::sort(order.begin(), order.end());

    const int T = n_teams;
    // Leagues of more than 64 teams: the FIXTURES are laid out along the Z-order curve over (home, away)
    // instead (the pair table below keeps the (home, away) order: its index is the tie rule of the bounds).
    // A workgroup's contiguous slice then covers ~sqrt(its pairs) home teams x as many away teams, and adds
    // into that many accumulator rows; in (home, away) order a slice is one home team against everybody --
    // ~3T row adds per workgroup, and every workgroup of the grid adding into the same away-side rows, one
    // after the other at the memory side.  Runs of one pair stay contiguous either way.
    const bool z_order = c->opt_pair_order == 1 || (c->opt_pair_order < 0 && T > 64);
    std::vector<uint64_t> forder;
    if (z_order) {
        auto spread = [](uint32_t v) {  // 16 bits -> every other bit of 32
            v = (v | (v << 8)) & 0x00FF00FFu;
            v = (v | (v << 4)) & 0x0F0F0F0Fu;
            v = (v | (v << 2)) & 0x33333333u;
            v = (v | (v << 1)) & 0x55555555u;
            return v;
        };
        forder.resize(n);
        for (int64_t i = 0; i < n; ++i)
            forder[i] = ((uint64_t)((spread(h[i]) << 1) | spread(a[i])) << 32) | (uint64_t)(uint32_t)i;
        std::sort(forder.begin(), forder.end());
    }
    // Every pair's run is padded to a multiple of LANE_FIX with NULL fixtures (same pair,
    // goals (255, 255), weight 0): a lane never straddles a pair boundary.  Then the whole
    // array is padded to the tile size with the sentinel team T (zero table entries).
    std::vector<uint16_t> hs, as;
    std::vector<uint8_t> xs8, ys8;
    std::vector<uint8_t> is_null;  // padding fixtures (any scoreline is a legal REAL one, 255-255 included)
    std::vector<float> ws;
    hs.reserve(n + n / 8 + dc::TILE); as.reserve(hs.capacity());
    xs8.reserve(hs.capacity()); ys8.reserve(hs.capacity());
    if (weights) ws.reserve(hs.capacity());
    std::vector<uint32_t> pairs;
    std::vector<double> pairw;  // [P][4]: sum w | sum w x | sum w y | 0  (for the prior workgroup's corrections)
    std::vector<double> pairc;  // [P][4]: weight of the pair's (0,0) | (1,0) | (0,1) fixtures | 0  (dc::ill_pass)
    double w11 = 0.0;
    std::vector<double> cA(T, 0.0), cD(T, 0.0), cH(T, 0.0);
    double lgsum = 0.0;
    auto pad_run = [&]() {
        while (hs.size() % dc::LANE_FIX) {
            hs.push_back(hs.back());
            as.push_back(as.back());
            xs8.push_back(255);
            ys8.push_back(255);
            is_null.push_back(1);
            if (weights) ws.push_back(0.0f);
        }
    };
    {   // the fixture arrays, in layout order
        const std::vector<uint64_t>& lay = z_order ? forder : order;
        uint32_t last_pk = 0;
        for (int64_t r = 0; r < n; ++r) {
            const uint32_t i = (uint32_t)lay[r];
            const uint32_t pk = (uint32_t)h[i] | ((uint32_t)a[i] << 16);
            if (r > 0 && pk != last_pk) pad_run();
            last_pk = pk;
            hs.push_back(h[i]);
            as.push_back(a[i]);
            xs8.push_back(x[i]);
            ys8.push_back(y[i]);
            is_null.push_back(0);
            if (weights) ws.push_back(w[i]);
        }
    }
    // the pair table and the host-side sums, in (home, away) order
    for (int64_t r = 0; r < n; ++r) {
        const uint32_t i = (uint32_t)order[r];
        const uint32_t pk = (uint32_t)h[i] | ((uint32_t)a[i] << 16);
        if (pairs.empty() || pairs.back() != pk) {
            pairs.push_back(pk);
            pairw.insert(pairw.end(), {0.0, 0.0, 0.0, 0.0});
            pairc.insert(pairc.end(), {0.0, 0.0, 0.0, 0.0});
        }
        const double wi = weights ? (double)w[i] : 1.0;
        cA[h[i]] += wi * x[i];
        cA[a[i]] += wi * y[i];
        cD[a[i]] += wi * x[i];
        cD[h[i]] += wi * y[i];
        cH[h[i]] += wi * x[i];
        {
            double* pw = &pairw[pairw.size() - 4];
            pw[0] += wi;
            pw[1] += wi * x[i];
            pw[2] += wi * y[i];
            if (x[i] <= 1 && y[i] <= 1) {   // score classes of bpl/_util.py:58-91
                if (x[i] == 1 && y[i] == 1) w11 += wi;
                else pairc[pairc.size() - 4 + (x[i] == 1 ? 1 : (y[i] == 1 ? 2 : 0))] += wi;
            }
        }
        lgsum += wi * (std::lgamma((double)x[i] + 1.0) + std::lgamma((double)y[i] + 1.0));
    }
    pad_run();
    const int64_t n_lanefix = (int64_t)hs.size();  // real + null fixtures
    const int n_tiles = (int)((n_lanefix + dc::TILE - 1) / dc::TILE);
    const int64_t n_pad = (int64_t)n_tiles * dc::TILE;
    hs.resize(n_pad, (uint16_t)T);
    as.resize(n_pad, (uint16_t)T);
    xs8.resize(n_pad, 2);
    ys8.resize(n_pad, 2);
    if (weights) ws.resize(n_pad, 0.0f);

    // ---- launch geometry: 8 waves per workgroup, contiguous tiles per wave
    const int max_wg = c->opt_max_wg;  // one workgroup per CU by default
    // partitions (see EvalPart): part 0 for one chain (or few: while the chip has idle CUs), with
    // 4 of 8 waves owning tiles when that costs no extra tiles per wave; part 1 = all 8 waves
    int aw0 = c->opt_active_waves;
    if (aw0 <= 0 || aw0 > dc::WAVES) aw0 = n_tiles <= max_wg * (dc::WAVES / 2) ? dc::WAVES / 2 : dc::WAVES;
    c->n_parts = aw0 < dc::WAVES && c->opt_active_waves <= 0 ? 2 : 1;
    int tpw = 1;  // of the 8-wave geometry (the chain-vectorised partitions scale it)
    {
        tpw = (n_tiles + max_wg * dc::WAVES - 1) / (max_wg * dc::WAVES);
        if (tpw < 1) tpw = 1;
    }
    // device copies of the indices, run-length encoded: ONE word per lane (all fixtures of a
    // lane share one pair): home | (number of real fixtures of the lane) << 16, and away
    const int64_t n_lanes = n_pad / dc::LANE_FIX;
    std::vector<uint32_t> h_lane(n_lanes), a_lane(n_lanes);
    for (int64_t l = 0; l < n_lanes; ++l) {
        uint32_t cnt = 0;
        for (int j = 0; j < dc::LANE_FIX; ++j) {
            const int64_t r = l * dc::LANE_FIX + j;
            cnt += r < n_lanefix && !is_null[r];
        }
        h_lane[l] = (uint32_t)hs[l * dc::LANE_FIX] | (cnt << 16);
        a_lane[l] = (uint32_t)as[l * dc::LANE_FIX];
    }

    // ---- upload
    for (int pi = 0; pi < c->n_parts; ++pi) {
        bplhip_ctx::EvalPart& ep = c->parts[pi];
        ep.aw = pi == 0 ? aw0 : dc::WAVES;
        ep.tpw = (n_tiles + max_wg * ep.aw - 1) / (max_wg * ep.aw);
        if (ep.tpw < 1) ep.tpw = 1;
        const int waves = (n_tiles + ep.tpw - 1) / ep.tpw;
        ep.n_wg = (waves + ep.aw - 1) / ep.aw;
        const SparseSlabs sp = build_sparse_slabs(hs, as, n_lanefix, T, ep.tpw * ep.aw, ep.n_wg);
        ep.total_c = sp.wg_off[ep.n_wg];
        HIP_TRY(c, ep.d_wg_off.ensure(sp.wg_off.size() * 4));
        HIP_TRY(c, ep.d_wg_slots.ensure(sp.wg_slots.size() * 4));
        HIP_TRY(c, ep.d_col_off.ensure(sp.col_off.size() * 4));
        HIP_TRY(c, ep.d_wg_dst.ensure(sp.wg_dst.size() * 4));
        // (synchronous copies: the host vectors die with this iteration)
        HIP_TRY(c, hipMemcpy(ep.d_wg_off.p, sp.wg_off.data(), sp.wg_off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(ep.d_wg_slots.p, sp.wg_slots.data(), sp.wg_slots.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(ep.d_col_off.p, sp.col_off.data(), sp.col_off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(ep.d_wg_dst.p, sp.wg_dst.data(), sp.wg_dst.size() * 4, hipMemcpyHostToDevice));
        {   // how many workgroups add to each accumulator row per evaluation (the rows count their
            // contributions: dc::ga_add): team row = the workgroups that touch the slot, scalar row
            // (shard sh, scalar j) = the workgroups with index = sh (mod GA_SHARDS)
            const int ncol = 3 * T;
            std::vector<int> expect(dc::ga_rows(T), 0);
            for (int cidx = 0; cidx < ncol; ++cidx) expect[cidx] = sp.col_off[cidx + 1] - sp.col_off[cidx];
            for (int w = 0; w < ep.n_wg; ++w)
                for (int j = 0; j < dc::N_SCAL; ++j) expect[ncol + (w % dc::GA_SHARDS) * dc::N_SCAL + j] += 1;
            for (int e : expect)
                if (e > 255)
                    return fail(c, BPLHIP_EUNSUPPORTED,
                                "set_fixtures: %d workgroups feed one accumulator row (the row's counter holds 255)", e);
            HIP_TRY(c, ep.d_ga_expect.ensure(expect.size() * 4));
            HIP_TRY(c, hipMemcpy(ep.d_ga_expect.p, expect.data(), expect.size() * 4, hipMemcpyHostToDevice));
        }
    }
    HIP_TRY(c, c->d_h.ensure(n_lanes * 4));
    HIP_TRY(c, c->d_a.ensure(n_lanes * 4));
    HIP_TRY(c, c->d_x.ensure(n_pad));
    HIP_TRY(c, c->d_y.ensure(n_pad));
    HIP_TRY(c, hipMemcpyAsync(c->d_h.p, h_lane.data(), n_lanes * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_a.p, a_lane.data(), n_lanes * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_x.p, xs8.data(), n_pad, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_y.p, ys8.data(), n_pad, hipMemcpyHostToDevice, s));
    if (weights) {
        HIP_TRY(c, c->d_w.ensure(n_pad * 4));
        HIP_TRY(c, hipMemcpyAsync(c->d_w.p, ws.data(), n_pad * 4, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, c->d_pairw.ensure(std::max<size_t>(pairw.size(), 4) * 8));
    HIP_TRY(c, hipMemcpy(c->d_pairw.p, pairw.data(), pairw.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, c->d_pairc.ensure(std::max<size_t>(pairc.size(), 4) * 8));
    HIP_TRY(c, hipMemcpy(c->d_pairc.p, pairc.data(), pairc.size() * 8, hipMemcpyHostToDevice));
    c->w11 = w11;
    HIP_TRY(c, c->d_pairs.ensure(pairs.size() * 4));
    HIP_TRY(c, hipMemcpyAsync(c->d_pairs.p, pairs.data(), pairs.size() * 4,
                              hipMemcpyHostToDevice, s));
    HIP_TRY(c, c->d_cA.ensure(T * 8));
    HIP_TRY(c, c->d_cD.ensure(T * 8));
    HIP_TRY(c, c->d_cH.ensure(T * 8));
    HIP_TRY(c, hipMemcpyAsync(c->d_cA.p, cA.data(), T * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_cD.p, cD.data(), T * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_cH.p, cH.data(), T * 8, hipMemcpyHostToDevice, s));
    c->h_xs.clear();
    if (k > 0) {
        c->h_xs.assign(covariates, covariates + (size_t)T * k);
        HIP_TRY(c, c->d_xs.ensure((size_t)T * k * 8));
        HIP_TRY(c, hipMemcpyAsync(c->d_xs.p, c->h_xs.data(), (size_t)T * k * 8,
                                  hipMemcpyHostToDevice, s));
        std::vector<float> xsf(c->h_xs.begin(), c->h_xs.end());
        HIP_TRY(c, c->d_xsf.ensure((size_t)T * k * 4));
        HIP_TRY(c, hipMemcpy(c->d_xsf.p, xsf.data(), (size_t)T * k * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipStreamSynchronize(s));

    drop_graphs(c);
    c->L = dc::make_layout(model_kind, T, k);
    c->lds_attr_set = false;
    c->n = n;
    c->n_tiles = n_tiles;
    c->weighted = weights != nullptr;
    c->P = (int)pairs.size();
    c->lgsum = lgsum;
    // every ordered pair h != a present (and no team against itself): the bounds are separable
    c->pairs_complete = T >= 2 && (long long)pairs.size() == (long long)T * (T - 1) &&
                        std::none_of(pairs.begin(), pairs.end(), [](uint32_t pr) { return (pr & 0xFFFFu) == (pr >> 16); });
    c->h_pairs = std::move(pairs);
    c->slab_chains = 0;
    // staged <=> T <= 64: the tail's one-lane-per-team epilogue (and the device-resident NUTS)
    for (int pi = 0; pi < c->n_parts; ++pi) {
        c->ep = &c->parts[pi];
        c->ep->staged = T <= 64 && ctx_lds_bytes(c, true) <= 96 * 1024;
        if (ctx_lds_bytes(c, c->ep->staged) > LDS_LIMIT)
            return fail(c, BPLHIP_EUNSUPPORTED, "set_fixtures: tail LDS footprint too large");
    }
    select_part(c, 1);
    int rc = ensure_slabs(c, 1);
    if (rc != BPLHIP_OK) return rc;

    // ---- chain-vectorised partition: fewer, fatter workgroups (the per-workgroup prologue
    // of 8 chains' tables is amortised over more tiles)
    for (int pi = 0; pi < 3; ++pi) {
        auto& vp = c->vps[pi];
        c->vp = &vp;  // (the LDS helpers below read the current partition)
        vp.ok = false;
        vp.slab_chains = 0;
        vp.tpw = c->opt_vec_tpw > 0 ? std::max(tpw, c->opt_vec_tpw) : tpw * (pi + 1);   // (1x / 2x / 3x: prepare_vec)
        const int vwaves = (n_tiles + vp.tpw - 1) / vp.tpw;
        vp.n_wg = (vwaves + dc::WAVES - 1) / dc::WAVES;
        const SparseSlabs vs = build_sparse_slabs(hs, as, n_lanefix, T, vp.tpw * dc::WAVES, vp.n_wg);
        vp.total_c = vs.wg_off[vp.n_wg];
        HIP_TRY(c, vp.d_wg_off.ensure(vs.wg_off.size() * 4));
        HIP_TRY(c, vp.d_wg_slots.ensure(vs.wg_slots.size() * 4));
        HIP_TRY(c, vp.d_col_off.ensure(vs.col_off.size() * 4));
        HIP_TRY(c, vp.d_wg_dst.ensure(vs.wg_dst.size() * 4));
        HIP_TRY(c, hipMemcpy(vp.d_wg_off.p, vs.wg_off.data(), vs.wg_off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(vp.d_wg_slots.p, vs.wg_slots.data(), vs.wg_slots.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(vp.d_col_off.p, vs.col_off.data(), vs.col_off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(vp.d_wg_dst.p, vs.wg_dst.data(), vs.wg_dst.size() * 4, hipMemcpyHostToDevice));
        vp.staged = T <= 64 && vec_tail_lds(c, true) <= 96 * 1024;
        vp.ok = dc::vec_stream_lds_bytes(T) <= 64 * 1024 && vec_tail_lds(c, vp.staged) <= LDS_LIMIT;
    }
    c->vp = &c->vps[0];
    c->bound = true;
    return BPLHIP_OK;
}

int bplhip_set_option(bplhip_ctx* c, const char* name, int value) {
    if (!c || !name) return BPLHIP_EINVAL;
    const std::string n(name);
    if (n == "device_nuts") {
        c->opt_device_nuts = value != 0;
        return BPLHIP_OK;
    }
    if (n == "dyn_big_wgs") {  // dynamic model, single launch: > 0 takes the sliced form (dyn_fused<true>) whatever
                               // N is, aiming for that many workgroups; 0: sliced form past 1024 fixtures per
                               // team workgroup, one workgroup per CU
        if (value < 0 || value > 65535) return fail(c, BPLHIP_EINVAL, "set_option: dyn_big_wgs out of range");
        c->opt_dyn_big_wgs = value;
        drop_graphs(c);
        return BPLHIP_OK;
    }
    if (n == "persistent_nuts") {
        c->opt_persistent_nuts = value != 0;
        return BPLHIP_OK;
    }
    if (n == "persistent_kernel") {  // 0: one launch per leapfrog even for a single resident chain
        c->opt_persistent_kernel = value != 0;
        return BPLHIP_OK;
    }
#ifdef DC_STAMPS
    if (n == "debug_stop") {
        c->opt_debug_stop = value;
        drop_graphs(c);
        return BPLHIP_OK;
    }
#endif
    if (n == "debug_raise_fault") {  // test hook: raise the fault word as a timed-out kernel would
        if (c->h_fault) __atomic_fetch_or(c->h_fault, (unsigned int)value, __ATOMIC_RELAXED);
        return BPLHIP_OK;
    }
    if (n == "pair_order") {   // takes effect at the next set_fixtures
        if (value < -1 || value > 1) return fail(c, BPLHIP_EINVAL, "set_option: pair_order is -1, 0 or 1");
        c->opt_pair_order = value;
        return BPLHIP_OK;
    }
    if (n == "dense_pairs") {  // 0: the rho bounds always walk the pair table
        c->opt_dense_pairs = value != 0;
        drop_graphs(c);
        return BPLHIP_OK;
    }
    if (n == "fused_small") {  // 0: neutral / dynamic evaluations always take the multi-launch path
        c->opt_fused_small = value != 0;
        drop_graphs(c);  // (captured launch sequences belong to the other path)
        return BPLHIP_OK;
    }
    if (n == "gridy_max_chains") {
        if (value < 1 || value > 4096) return fail(c, BPLHIP_EINVAL, "gridy_max_chains out of range");
        c->opt_gridy_max_chains = value;
        return BPLHIP_OK;
    }
    if (n == "vec_min_chains") {  // batched calls with >= value chains use the vectorised kernel
        if (value < 0) return fail(c, BPLHIP_EINVAL, "vec_min_chains must be >= 0");
        c->opt_vec_min_chains = value;
        return BPLHIP_OK;
    }
    if (n == "vec_tiles_per_wave") {  // 0 = by chain count; takes effect at the next bplhip_set_fixtures
        if (value < 0 || value > 4096) return fail(c, BPLHIP_EINVAL, "vec_tiles_per_wave out of range");
        c->opt_vec_tpw = value;
        return BPLHIP_OK;
    }
    if (n == "neu_runs") {  // neutral model's sliced single launch: per-run arithmetic (1) / per fixture (0)
        c->opt_neu_runs = value != 0;
        drop_graphs(c);
        return BPLHIP_OK;
    }
    if (n == "dyn_gather") {  // dynamic model's small single launch: per-fixture adjoint records gathered by the cells (1) / atomics (0)
        c->opt_dyn_gather = value != 0;
        drop_graphs(c);
        return BPLHIP_OK;
    }
    if (n == "persist_spec") {  // persistent kernel: the next position before the leaf (1) or after it (0)
        c->opt_persist_spec = value != 0;
        return BPLHIP_OK;
    }
    if (n == "chunk_graph") {  // persistent chains: a chunk of leapfrogs as one replayed hipGraph (1) or launch by launch (0)
        c->opt_chunk_graph = value != 0;
        return BPLHIP_OK;
    }
    if (n == "max_wg") {  // takes effect at the next bplhip_set_fixtures
        // (an accumulator row counts its contributions in 8 bits, dc::GA_COUNT_SHIFT: with few teams every
        // workgroup adds to every row)
        if (value < 1 || value > 255) return fail(c, BPLHIP_EINVAL, "max_wg out of range [1,255]");
        c->opt_max_wg = value;
        return BPLHIP_OK;
    }
    if (n == "active_waves") {  // waves per workgroup that own tiles; 0 = automatic; next set_fixtures
        if (value < 0 || value > dc::WAVES) return fail(c, BPLHIP_EINVAL, "active_waves: 0 (automatic) .. 8");
        c->opt_active_waves = value;
        return BPLHIP_OK;
    }
    return fail(c, BPLHIP_EINVAL, "unknown option '%s'", name);
}

int bplhip_last_eval_path(const bplhip_ctx* c) {
    return c ? c->last_eval_path : BPLHIP_EINVAL;
}
int bplhip_last_nuts_engine(const bplhip_ctx* c) {
    return c ? c->last_nuts_engine : BPLHIP_EINVAL;
}

int bplhip_latent_dim(const bplhip_ctx* c) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound) return BPLHIP_ESTATE;
    return c->neutral ? c->NL.D : (c->dynamic ? c->DL.D : c->L.D);
}

static int bplhip_set_fixtures_neutral_impl(bplhip_ctx* c, int64_t n, int32_t n_teams, const uint16_t* home_idx,
                                const uint16_t* away_idx, const uint8_t* home_goals,
                                const uint8_t* away_goals, const uint8_t* neutral_venue,
                                const uint8_t* home_conf, const uint8_t* away_conf, int32_t n_conf,
                                const float* weights, const double* covariates, int32_t k,
                                void* stream) {
    if (!c) return BPLHIP_EINVAL;
    c->bound = false;
    c->last_eval_path = BPLHIP_PATH_NONE;
    c->last_nuts_engine = BPLHIP_ENGINE_NONE;
    if (n < 1 || n > (int64_t)0xFFFFFFFF || n_teams < 1 || n_teams > 65534)
        return fail(c, BPLHIP_EINVAL, "set_fixtures_neutral: bad sizes");
    if (n_conf < 0 || n_conf > 255 || (n_conf > 0 && (!home_conf || !away_conf)) ||
        (n_conf == 0 && (home_conf || away_conf)))
        return fail(c, BPLHIP_EINVAL, "set_fixtures_neutral: confederation arrays / n_conf mismatch");
    if (!home_idx || !away_idx || !home_goals || !away_goals || !neutral_venue)
        return fail(c, BPLHIP_EINVAL, "set_fixtures_neutral: null fixture array");
    if (k < 0 || (k > 0 && !covariates) || (k == 0 && covariates))
        return fail(c, BPLHIP_EINVAL, "set_fixtures_neutral: covariates/k mismatch");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<uint16_t> h(n), a(n);
    std::vector<uint8_t> x(n), y(n), nv(n);
    std::vector<float> w;
    HIP_TRY(c, hipMemcpyAsync(h.data(), home_idx, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(a.data(), away_idx, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(x.data(), home_goals, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(y.data(), away_goals, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(nv.data(), neutral_venue, n, hipMemcpyDeviceToHost, s));
    if (weights) {
        w.resize(n);
        HIP_TRY(c, hipMemcpyAsync(w.data(), weights, n * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    double lgsum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (h[i] >= n_teams || a[i] >= n_teams || nv[i] > 1)
            return fail(c, BPLHIP_EINVAL, "set_fixtures_neutral: value out of range at fixture %lld",
                        (long long)i);
        const double wi = weights ? (double)w[i] : 1.0;
        lgsum += wi * (std::lgamma((double)x[i] + 1.0) + std::lgamma((double)y[i] + 1.0));
    }
    // sort by (venue, home, away): a wave of dyn_pass2 then usually sits on one pair and adds
    // its 64 contributions with one set of atomics.  (Confederations follow the teams.)
    std::vector<uint32_t> order(n);
    {
        for (int64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) {
            // (last key: the fixtures with a tau term -- both sides <= 1 goal -- first within a run, so that a
            // wave's 64 consecutive fixtures mostly agree on having one: dcn::neu_big)
            const uint64_t kp = ((uint64_t)nv[p] << 33) | ((uint64_t)h[p] << 17) | ((uint64_t)a[p] << 1) |
                                (uint64_t)!(x[p] <= 1 && y[p] <= 1);
            const uint64_t kq = ((uint64_t)nv[q] << 33) | ((uint64_t)h[q] << 17) | ((uint64_t)a[q] << 1) |
                                (uint64_t)!(x[q] <= 1 && y[q] <= 1);
            return kp < kq;
        });
        auto permute = [&](auto& v) {
            auto t = v;
            for (int64_t i = 0; i < n; ++i) t[i] = v[order[i]];
            v.swap(t);
        };
        permute(h); permute(a); permute(x); permute(y); permute(nv);
        if (weights) permute(w);
    }
    HIP_TRY(c, c->d_h.ensure(n * 2));
    HIP_TRY(c, c->d_a.ensure(n * 2));
    HIP_TRY(c, c->d_x.ensure(n));
    HIP_TRY(c, c->d_y.ensure(n));
    HIP_TRY(c, c->dd_nv.ensure(n));
    HIP_TRY(c, hipMemcpyAsync(c->d_h.p, h.data(), n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_a.p, a.data(), n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_x.p, x.data(), n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_y.p, y.data(), n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->dd_nv.p, nv.data(), n, hipMemcpyHostToDevice, s));
    if (weights) {
        HIP_TRY(c, c->d_w.ensure(n * 4));
        HIP_TRY(c, hipMemcpyAsync(c->d_w.p, w.data(), n * 4, hipMemcpyHostToDevice, s));
    }
    std::vector<uint8_t> hcv, acv;
    if (n_conf > 0) {  // (device -> device: the library keeps its own copy)
        hcv.resize(n); acv.resize(n);
        HIP_TRY(c, hipMemcpy(hcv.data(), home_conf, n, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(acv.data(), away_conf, n, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i)
            if (hcv[i] >= n_conf || acv[i] >= n_conf)
                return fail(c, BPLHIP_EINVAL, "set_fixtures_neutral: confederation out of range at fixture %lld",
                            (long long)i);
        {   // same order as the fixtures
            auto t1 = hcv, t2 = acv;
            for (int64_t i = 0; i < n; ++i) { t1[i] = hcv[order[i]]; t2[i] = acv[order[i]]; }
            hcv.swap(t1); acv.swap(t2);
        }
        HIP_TRY(c, c->dd_hc.ensure(n));
        HIP_TRY(c, c->dd_ac.ensure(n));
        HIP_TRY(c, hipMemcpy(c->dd_hc.p, hcv.data(), n, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->dd_ac.p, acv.data(), n, hipMemcpyHostToDevice));
    }
    // single-launch kernel (dcn::neu_fused): packed fixtures and the schedule of its gather step
    const dcn::NeuLayout NL = dcn::make_neu_layout(n_teams, k, n_conf);
    c->neu_fusable = n <= dcn::FUSED_MAX_N && n_teams <= dcn::FUSED_MAX_T && n_conf <= dcn::FUSED_MAX_C;
    if (c->neu_fusable) {
        std::vector<dcn::FusedFixture> pack(n);
        std::vector<int> off(n_teams + 1, 0);
        for (int64_t i = 0; i < n; ++i) {
            dcn::FusedFixture f{};
            f.h = h[i]; f.a = a[i]; f.x = x[i]; f.y = y[i]; f.nv = nv[i];
            f.hc = n_conf ? hcv[i] : 0;
            f.ac = n_conf ? acv[i] : 0;
            f.w = weights ? w[i] : 1.0f;
            pack[i] = f;
            ++off[h[i] + 1];
            ++off[a[i] + 1];
        }
        for (int t = 0; t < n_teams; ++t) off[t + 1] += off[t];
        // team-major incidence entries (fixture order within a team: the sums have a fixed order)
        std::vector<uint32_t> inc(2 * n);
        {
            std::vector<int> fill(off.begin(), off.end() - 1);
            for (int64_t i = 0; i < n; ++i) {
                inc[fill[h[i]]++] = ((uint32_t)i << 2) | ((uint32_t)nv[i] << 1);
                inc[fill[a[i]]++] = ((uint32_t)i << 2) | ((uint32_t)nv[i] << 1) | 1u;
            }
        }
        // slots: <= 64 consecutive entries of one team, taken by one 16-lane row (lane `sub`
        // holds entries sub, sub + 16, ...); row r of the workgroup takes slots r, r + 64, ...
        constexpr int SLOT = 16 * dcn::FUSED_PRE;
        std::vector<int> slot_off(n_teams + 1, 0);
        for (int t = 0; t < n_teams; ++t) slot_off[t + 1] = slot_off[t] + (off[t + 1] - off[t] + SLOT - 1) / SLOT;
        const int n_slots = slot_off[n_teams];
        const int rounds = std::max(1, (n_slots + dcn::FUSED_ROWS - 1) / dcn::FUSED_ROWS);
        std::vector<uint32_t> sched((size_t)rounds * dcn::FUSED_PRE * dcn::FUSED_BLOCK, dcn::INC_NONE);
        for (int t = 0; t < n_teams; ++t)
            for (int sl = slot_off[t]; sl < slot_off[t + 1]; ++sl) {
                const int b0 = off[t] + (sl - slot_off[t]) * SLOT, b1 = std::min(b0 + SLOT, off[t + 1]);
                const int round = sl / dcn::FUSED_ROWS, row = sl % dcn::FUSED_ROWS;
                for (int e = b0; e < b1; ++e) {
                    const int sub = (e - b0) % 16, r = (e - b0) / 16;
                    sched[((size_t)round * dcn::FUSED_PRE + r) * dcn::FUSED_BLOCK + row * 16 + sub] = inc[e];
                }
            }
        c->neu_slots = n_slots;
        c->neu_fusable = dcn::fused_lds_doubles(NL, n, n_slots) * 8 <= LDS_LIMIT;
        if (c->neu_fusable) {
            HIP_TRY(c, c->dd_fpack.ensure(pack.size() * sizeof(dcn::FusedFixture)));
            HIP_TRY(c, c->dd_sched.ensure(sched.size() * 4));
            HIP_TRY(c, c->dd_slot_off.ensure(slot_off.size() * 4));
            HIP_TRY(c, hipMemcpy(c->dd_fpack.p, pack.data(), pack.size() * sizeof(dcn::FusedFixture), hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(c->dd_sched.p, sched.data(), sched.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(c->dd_slot_off.p, slot_off.data(), slot_off.size() * 4, hipMemcpyHostToDevice));
        }
    }
    c->neu_keys.clear();
    c->neu_runs_nb = -1;
    if (!c->neu_fusable) {  // dcn::neu_big streams the same 16-byte records
        std::vector<dcn::FusedFixture> pack(n);
        c->neu_keys.resize(n);
        for (int64_t i = 0; i < n; ++i) {
            dcn::FusedFixture f{};
            f.h = h[i]; f.a = a[i]; f.x = x[i]; f.y = y[i]; f.nv = nv[i];
            f.hc = n_conf ? hcv[i] : 0;
            f.ac = n_conf ? acv[i] : 0;
            f.w = weights ? w[i] : 1.0f;
            pack[i] = f;
            c->neu_keys[i] = ((unsigned long long)f.h << 33) | ((unsigned long long)f.a << 17) |
                             ((unsigned long long)(f.nv != 0) << 16) | ((unsigned long long)f.hc << 8) | (unsigned long long)f.ac;
        }
        HIP_TRY(c, c->dd_fpack.ensure(pack.size() * sizeof(dcn::FusedFixture)));
        HIP_TRY(c, hipMemcpy(c->dd_fpack.p, pack.data(), pack.size() * sizeof(dcn::FusedFixture), hipMemcpyHostToDevice));
    }
    HIP_TRY(c, c->dd_cells.ensure((size_t)n_teams * dcd::P_N * 8));
    // (dcn::neu_big adds into NEU_BIG_GROUPS copies of the scratch; the multi-launch path uses the first)
    const size_t neu_scratch_bytes = ((size_t)n_teams * dcd::A_N + dcd::SC_N + n_conf) * 8 * dcn::NEU_BIG_GROUPS;
    HIP_TRY(c, c->dd_acc.ensure(neu_scratch_bytes));
    // the single-launch kernel for large N (dcn::neu_big) finds its scratch and its counters zeroed, and leaves them so
    HIP_TRY(c, hipMemset(c->dd_acc.p, 0, neu_scratch_bytes));
    HIP_TRY(c, c->dd_tick.ensure(dcd::TICKET_BYTES));
    HIP_TRY(c, hipMemset(c->dd_tick.p, 0, dcd::TICKET_BYTES));
    c->dyn_scratch_clean = true;
    c->dyn_big_lds = 0;   // (the cached occupancy belongs to one kernel and one LDS size)
    c->h_xs.clear();
    if (k > 0) {
        c->h_xs.assign(covariates, covariates + (size_t)n_teams * k);
        HIP_TRY(c, c->d_xs.ensure((size_t)n_teams * k * 8));
        HIP_TRY(c, hipMemcpyAsync(c->d_xs.p, c->h_xs.data(), (size_t)n_teams * k * 8,
                                  hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    drop_graphs(c);
    c->NL = dcn::make_neu_layout(n_teams, k, n_conf);
    c->n = n;
    c->lgsum = lgsum;
    c->weighted = weights != nullptr;
    c->lds_attr_set = false;
    c->dynamic = false;
    c->neutral = true;
    c->bound = true;
    return BPLHIP_OK;
}

static int bplhip_set_fixtures_dynamic_impl(bplhip_ctx* c, int64_t n, int32_t n_teams, int32_t n_gameweeks,
                                const uint16_t* home_idx, const uint16_t* away_idx,
                                const uint8_t* home_goals, const uint8_t* away_goals,
                                const uint16_t* gameweek, const uint8_t* neutral_venue,
                                const double* covariates, int32_t k, int32_t random_walk,
                                void* stream) {
    if (!c) return BPLHIP_EINVAL;
    c->bound = false;
    c->last_eval_path = BPLHIP_PATH_NONE;
    c->last_nuts_engine = BPLHIP_ENGINE_NONE;
    c->neutral = false;
    if (n < 1 || n_teams < 1 || n_teams > 65534 || n_gameweeks < 1 || n_gameweeks > 65535)
        return fail(c, BPLHIP_EINVAL, "set_fixtures_dynamic: bad sizes");
    if (!home_idx || !away_idx || !home_goals || !away_goals || !gameweek || !neutral_venue)
        return fail(c, BPLHIP_EINVAL, "set_fixtures_dynamic: null fixture array");
    if (k < 0 || (k > 0 && !covariates) || (k == 0 && covariates))
        return fail(c, BPLHIP_EINVAL, "set_fixtures_dynamic: covariates/k mismatch");
    if ((int64_t)n_teams * n_gameweeks > (int64_t)1 << 26)
        return fail(c, BPLHIP_EUNSUPPORTED, "set_fixtures_dynamic: too many (gameweek, team) cells");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<uint16_t> h(n), a(n), g(n);
    std::vector<uint8_t> x(n), y(n), nv(n);
    HIP_TRY(c, hipMemcpyAsync(h.data(), home_idx, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(a.data(), away_idx, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(g.data(), gameweek, n * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(x.data(), home_goals, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(y.data(), away_goals, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(nv.data(), neutral_venue, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    double lgsum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (h[i] >= n_teams || a[i] >= n_teams || g[i] >= n_gameweeks || nv[i] > 1)
            return fail(c, BPLHIP_EINVAL, "set_fixtures_dynamic: index out of range at fixture %lld",
                        (long long)i);
        lgsum += std::lgamma((double)x[i] + 1.0) + std::lgamma((double)y[i] + 1.0);
    }
    {   // stable sort by gameweek: a workgroup of dyn_pass2 then spans only a few gameweeks
        std::vector<uint32_t> order(n);
        for (int64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        if (n > (int64_t)0xFFFFFFFF) return fail(c, BPLHIP_EUNSUPPORTED, "set_fixtures_dynamic: n too large");
        std::stable_sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) { return g[p] < g[q]; });
        auto permute = [&](auto& v) {
            auto w = v;
            for (int64_t i = 0; i < n; ++i) w[i] = v[order[i]];
            v.swap(w);
        };
        // ... and inside a gameweek, in blocks of 1024, the fixtures with a tau term (both sides <= 1 goal)
        // first: a wave's 64 consecutive fixtures then mostly agree on whether they have one, and the sliced
        // single launch (dyn_fused<true>) runs its log / reciprocal for a third of the waves, not for all
        for (int64_t b0 = 0; b0 < n;) {
            int64_t b1 = b0;
            while (b1 < n && b1 - b0 < 1024 && g[order[b1]] == g[order[b0]]) ++b1;
            std::stable_partition(order.begin() + b0, order.begin() + b1,
                                  [&](uint32_t p) { return x[p] <= 1 && y[p] <= 1; });
            b0 = b1;
        }
        permute(h); permute(a); permute(x); permute(y); permute(nv); permute(g);
    }
    const size_t GT = (size_t)n_teams * n_gameweeks;
    HIP_TRY(c, c->d_h.ensure(n * 2));
    HIP_TRY(c, c->d_a.ensure(n * 2));
    HIP_TRY(c, c->d_x.ensure(n));
    HIP_TRY(c, c->d_y.ensure(n));
    HIP_TRY(c, c->dd_gw.ensure(n * 2));
    HIP_TRY(c, c->dd_nv.ensure(n));
    HIP_TRY(c, hipMemcpyAsync(c->d_h.p, h.data(), n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_a.p, a.data(), n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_x.p, x.data(), n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->d_y.p, y.data(), n, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->dd_gw.p, g.data(), n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->dd_nv.p, nv.data(), n, hipMemcpyHostToDevice, s));
    std::vector<unsigned long long> fx8(n);   // (kept alive until the stream is synchronised below)
    for (int64_t i = 0; i < n; ++i) fx8[i] = dcd::pack_fixture(h[i], a[i], x[i], y[i], nv[i]);
    HIP_TRY(c, c->dd_fx8.ensure(n * 8));
    HIP_TRY(c, hipMemcpyAsync(c->dd_fx8.p, fx8.data(), n * 8, hipMemcpyHostToDevice, s));
    {   // incidence lists of the cells (gameweek, team) over the sorted fixtures: dyn_fused<false>'s gather
        std::vector<int> off(GT + 1, 0);
        for (int64_t i = 0; i < n; ++i) {
            off[(size_t)g[i] * n_teams + h[i] + 1] += 1;
            off[(size_t)g[i] * n_teams + a[i] + 1] += 1;
        }
        int longest = 0;
        for (size_t cidx = 0; cidx < GT; ++cidx) {
            longest = std::max(longest, off[cidx + 1]);
            off[cidx + 1] += off[cidx];
        }
        c->dyn_gather = longest <= dcd::GATHER_MAX_INCIDENT && n < (1ll << 30);
        if (c->dyn_gather) {
            std::vector<unsigned int> inc(std::max<size_t>(2 * (size_t)n, 1));
            std::vector<int> fill(off.begin(), off.end() - 1);
            for (int64_t i = 0; i < n; ++i) {   // (fixture order within a list: ascending, the summation order)
                const unsigned int venue = nv[i] ? 1u << 30 : 0u;
                inc[fill[(size_t)g[i] * n_teams + h[i]]++] = (unsigned int)i | venue;
                inc[fill[(size_t)g[i] * n_teams + a[i]]++] = (unsigned int)i | venue | (1u << 31);
            }
            HIP_TRY(c, c->dd_inc_off.ensure(off.size() * 4));
            HIP_TRY(c, c->dd_inc.ensure(inc.size() * 4));
            HIP_TRY(c, c->dd_fadj.ensure((size_t)n * 16));
            HIP_TRY(c, hipMemcpy(c->dd_inc_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(c->dd_inc.p, inc.data(), inc.size() * 4, hipMemcpyHostToDevice));
        }
    }
    HIP_TRY(c, c->dd_cells.ensure(GT * dcd::P_N * 8));
    HIP_TRY(c, c->dd_acc.ensure(dcd::scratch_doubles(n_gameweeks, n_teams, k) * 8));
    // the single-launch kernel finds its scratch zeroed and its cell records armed (and leaves them so):
    // done here, so that a launch sequence captured right after this call holds no fills
    HIP_TRY(c, hipMemsetAsync(c->dd_acc.p, 0, dcd::scratch_doubles(n_gameweeks, n_teams, k) * 8, s));
    HIP_TRY(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->dd_cells.p), (int)dcd::CELL_EMPTY_WORD,
                                 GT * dcd::P_N * 2, s));
    c->dyn_scratch_clean = true;
    c->dyn_big_lds = 0;   // (the cached occupancy belongs to one kernel and one LDS size)
    HIP_TRY(c, c->dd_hyp.ensure((size_t)6 * n_gameweeks * 8));
    {   // first fixture of every gameweek (sorted), and the two arrival counters
        std::vector<int> gw_off(n_gameweeks + 1, 0);
        for (int64_t i = 0; i < n; ++i) gw_off[g[i] + 1] += 1;
        c->dyn_max_gw = 0;
        for (int j = 0; j < n_gameweeks; ++j) c->dyn_max_gw = std::max<long long>(c->dyn_max_gw, gw_off[j + 1]);
        for (int j = 0; j < n_gameweeks; ++j) gw_off[j + 1] += gw_off[j];
        HIP_TRY(c, c->dd_gwoff.ensure(gw_off.size() * 4));
        HIP_TRY(c, hipMemcpy(c->dd_gwoff.p, gw_off.data(), gw_off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, c->dd_tick.ensure(dcd::TICKET_BYTES));
        HIP_TRY(c, hipMemset(c->dd_tick.p, 0, dcd::TICKET_BYTES));
        HIP_TRY(c, hipMemset(c->dd_acc.p, 0, dcd::scratch_doubles(n_gameweeks, n_teams, k) * 8));
    }
    c->h_xs.clear();
    if (k > 0) {
        c->h_xs.assign(covariates, covariates + (size_t)n_teams * k);
        HIP_TRY(c, c->d_xs.ensure((size_t)n_teams * k * 8));
        HIP_TRY(c, hipMemcpyAsync(c->d_xs.p, c->h_xs.data(), (size_t)n_teams * k * 8,
                                  hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    drop_graphs(c);
    c->DL = dcd::make_dyn_layout(n_gameweeks, n_teams, k);
    c->dyn_random_walk = random_walk != 0;
    c->n = n;
    c->lgsum = lgsum;
    c->dynamic = true;
    c->bound = true;
    return BPLHIP_OK;
}

static int bplhip_logp_grad_batched_impl(bplhip_ctx* c, int32_t n_chains, const double* z,
                             double* potential, double* grad, double* aux, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound) return fail(c, BPLHIP_ESTATE, "logp_grad: no fixtures bound");
    if (!z || !potential || !grad) return fail(c, BPLHIP_EINVAL, "logp_grad: null pointer");
    if (n_chains < 1 || n_chains > 65535)
        return fail(c, BPLHIP_EINVAL, "logp_grad: n_chains=%d out of range", n_chains);
    HIP_TRY(c, hipSetDevice(c->device));
    if (use_vec(c, n_chains))
        return launch_eval_vec(c, n_chains, z, potential, grad, aux, static_cast<hipStream_t>(stream));
    if (!c->dynamic && !c->neutral) {
        int rc = ensure_slabs(c, n_chains);
        if (rc != BPLHIP_OK) return rc;
    }
    return launch_eval(c, n_chains, z, potential, grad, aux, static_cast<hipStream_t>(stream));
}

int bplhip_logp_grad(bplhip_ctx* c, const double* z, double* potential, double* grad,
                     double* aux, void* stream) {
    return bplhip_logp_grad_batched(c, 1, z, potential, grad, aux, stream);
}

static int bplhip_logp_grad_graph_impl(bplhip_ctx* c, int32_t count, int32_t n_z, const double* z,
                           double* potential, double* grad, int32_t replays, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound) return fail(c, BPLHIP_ESTATE, "logp_grad_graph: no fixtures bound");
    if (!z || !potential || !grad || count < 1 || n_z < 1 || replays < 0)
        return fail(c, BPLHIP_EINVAL, "logp_grad_graph: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const GraphKey key{count, n_z, z, potential, grad};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = bplhip_latent_dim(c);
    auto enqueue = [&](hipStream_t st) -> int {
        int rc = BPLHIP_OK;
        for (int i = 0; i < count && rc == BPLHIP_OK; ++i) {
            const int j = i % n_z;
            rc = launch_eval(c, 1, z + (size_t)j * D, potential + j, grad + (size_t)j * D, nullptr, st);
        }
        return rc;
    };
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
        // one un-captured evaluation first: whatever the launch path sets up lazily happens outside the capture
        int rc = launch_eval(c, 1, z, potential, grad, nullptr, s);
        if (rc != BPLHIP_OK) return rc;
        hipGraphExec_t ge = nullptr;
        rc = capture_launches(c, enqueue, &ge);
        if (rc != BPLHIP_OK) return rc;
        if (!ge) {  // no graph on this runtime: the same launches, one by one
            for (int r = 0; r < replays; ++r) {
                rc = enqueue(s);
                if (rc != BPLHIP_OK) return rc;
            }
            return BPLHIP_OK;
        }
        it = c->graphs.emplace(key, ge).first;
    }
    for (int r = 0; r < replays; ++r) HIP_TRY(c, hipGraphLaunch(it->second, s));
    return BPLHIP_OK;
}

#ifdef DC_STAMPS
// diagnostic build only: allocate / read the per-workgroup timestamp buffer [n_wg][16]
int bplhip_debug_stamps(bplhip_ctx* c, unsigned long long* out, int n_words) {
    if (!c || !c->bound) return BPLHIP_ESTATE;
    const size_t bytes = (size_t)(c->ep->n_wg + 2) * 16 * 8;
    if (!c->d_debug.p) {
        HIP_TRY(c, c->d_debug.ensure(bytes));
        HIP_TRY(c, hipMemset(c->d_debug.p, 0, bytes));
        return c->ep->n_wg + 1;
    }
    HIP_TRY(c, hipDeviceSynchronize());
    const size_t want = std::min(bytes, (size_t)n_words * 8);
    HIP_TRY(c, hipMemcpy(out, c->d_debug.p, want, hipMemcpyDeviceToHost));
    return c->ep->n_wg + 1;
}
#endif

void bplhip_threefry_split(uint32_t key_hi, uint32_t key_lo, int32_t n, uint32_t* out) {
    if (n <= 0 || !out) return;
    std::vector<tf::Key> ks(n);
    tf::split({key_hi, key_lo}, n, ks.data());
    for (int i = 0; i < n; ++i) {
        out[2 * i] = ks[i].hi;
        out[2 * i + 1] = ks[i].lo;
    }
}

void bplhip_threefry_bits(uint32_t key_hi, uint32_t key_lo, int32_t n, uint32_t* out) {
    if (n <= 0 || !out) return;
    tf::random_bits({key_hi, key_lo}, n, out);
}

void bplhip_nuts_default_cfg(bplhip_nuts_cfg* cfg) {
    if (!cfg) return;
    cfg->num_warmup = 500;
    cfg->num_samples = 1000;
    cfg->max_tree_depth = 10;
    cfg->adapt_step_size = 1;
    cfg->adapt_mass_matrix = 1;
    cfg->thinning = 1;
    cfg->step_size = 1.0;
    cfg->target_accept_prob = 0.8;
    cfg->init_radius = 2.0;
    cfg->max_delta_energy = 1000.0;
}

}  // extern "C"

// ------------------------------------------------------------------ NUTS glue + constrain

namespace {

// Potential functor handed to the templated NUTS driver: one launch sequence + one
// pinned-host read-back per evaluation.
struct HipPotential {
    bplhip_ctx* c;
    hipStream_t s;
    int D;
    double *d_z, *d_pot, *d_grad, *d_aux;  // device
    double* hp;                            // pinned: [D grad | pot | aux4]
    int rc = BPLHIP_OK;
    int dim() const { return D; }
    // returns false on a HIP failure (rc holds the code)
    bool operator()(const double* z, double* U, double* grad, double* aux) {
        if (hipMemcpyAsync(d_z, z, (size_t)D * 8, hipMemcpyHostToDevice, s) != hipSuccess) {
            rc = fail(c, BPLHIP_EHIP, "nuts: H2D of z failed");
            return false;
        }
        rc = launch_eval(c, 1, d_z, d_pot, d_grad, d_aux, s);
        if (rc != BPLHIP_OK) return false;
        // d_grad, d_pot, d_aux are contiguous: one D2H
        if (hipMemcpyAsync(hp, d_grad, (size_t)(D + 1 + 4) * 8, hipMemcpyDeviceToHost, s) !=
                hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            rc = fail(c, BPLHIP_EHIP, "nuts: D2H / sync failed: %s",
                      hipGetErrorString(hipGetLastError()));
            return false;
        }
        std::memcpy(grad, hp, (size_t)D * 8);
        *U = hp[D];
        if (aux) std::memcpy(aux, hp + D + 1, 4 * 8);
        return true;
    }
};

}  // namespace

namespace {

// Tree builder on the device: per doubling the host enqueues k_begin, 2^j dc_eval launches
// (leaf bookkeeping in their tails) and k_end, and synchronises once per batch of
// doublings; the first batch of a transition speculates on the previous tree's depth.
struct DeviceEngine {
    bplhip_ctx* c;
    hipStream_t s;
    const nuts::Config& cfg;
    int D, max_depth;
    double* ns;        // device state (nuts_dev.hip.h)
    double* hp;        // pinned: [r: D | hdr: H_N | z: D]
    int64_t evals = 0;
    int last_depth = 1;
    int rc = BPLHIP_OK;
    int dim() const { return D; }
    int64_t leapfrogs() const { return evals; }
    bool hip_ok(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        rc = fail(c, BPLHIP_EHIP, "device nuts: %s: %s", what, hipGetErrorString(e));
        return false;
    }
    bool set_state(const double* z, double* pe_out, bool* finite) {
        std::memcpy(hp, z, (size_t)D * 8);
        double* zn = nd::vec(ns, D, nd::V_ZN);
        double* gr = nd::vec(ns, D, nd::V_GRAD);
        if (!hip_ok(hipMemcpyAsync(zn, hp, (size_t)D * 8, hipMemcpyHostToDevice, s), "H2D z")) return false;
        rc = launch_eval(c, 1, zn, ns + nd::H_LEAF_PE, gr, ns + nd::H_LEAF_AUX0, s);
        if (rc != BPLHIP_OK) return false;
        // adopt as the current state of the chain
        (void)hipMemcpyAsync(nd::vec(ns, D, nd::V_Z), zn, (size_t)D * 8, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(nd::vec(ns, D, nd::V_G), gr, (size_t)D * 8, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(ns + nd::H_CUR_PE, ns + nd::H_LEAF_PE, 8, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(ns + nd::H_T_AUX0, ns + nd::H_LEAF_AUX0, 32, hipMemcpyDeviceToDevice, s);
        double* h_hdr = hp + D;
        (void)hipMemcpyAsync(h_hdr, ns, (size_t)nd::H_N * 8, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(hp + D + nd::H_N, gr, (size_t)D * 8, hipMemcpyDeviceToHost, s);
        if (!hip_ok(hipStreamSynchronize(s), "sync(set_state)")) return false;
        const double pe = h_hdr[nd::H_LEAF_PE];
        bool ok = std::isfinite(pe);
        for (int i = 0; i < D && ok; ++i) ok = std::isfinite(hp[D + nd::H_N + i]);
        *finite = ok;
        *pe_out = pe;
        evals += 1;
        return true;
    }
    bool transition(const double* r, tf::Key key, double step_size, const nuts::vec& inv_mass,
                    bool mass_changed, double* z_out, nuts::TransitionOut* out) {
        double* h_hdr = hp + D;
        if (mass_changed) {
            // (pinned staging reused: the copy is ordered before the momentum copy)
            std::memcpy(hp + D + nd::H_N, inv_mass.data(), (size_t)D * 8);
            if (!hip_ok(hipMemcpyAsync(nd::vec(ns, D, nd::V_INVM), hp + D + nd::H_N, (size_t)D * 8,
                                       hipMemcpyHostToDevice, s), "H2D inv_mass")) return false;
        }
        std::memcpy(hp, r, (size_t)D * 8);
        if (!hip_ok(hipMemcpyAsync(nd::vec(ns, D, nd::V_TL_R), hp, (size_t)D * 8,
                                   hipMemcpyHostToDevice, s), "H2D r")) return false;
        hipLaunchKernelGGL(nd::k_init, dim3(1), dim3(64), 0, s, ns, D, step_size, cfg.max_delta_energy);
        double* zn = nd::vec(ns, D, nd::V_ZN);
        double* gr = nd::vec(ns, D, nd::V_GRAD);
        int depth = 0;
        bool stop = false;
        bool first_batch = true;
        while (!stop && depth < max_depth) {
            int nb = first_batch ? std::max(1, std::min(last_depth, max_depth)) : 1;
            nb = std::min(nb, max_depth - depth);
            for (int j = depth; j < depth + nb; ++j) {
                // numpyro build_tree: key, direction_key, doubling_key = split(key, 3);
                // _double_tree: key, transition_key = split(doubling_key)
                tf::Key k_next, k_dir, k_dbl, k_sub, k_tr;
                tf::split3(key, &k_next, &k_dir, &k_dbl);
                key = k_next;
                const int going_right = tf::bernoulli(k_dir, 0.5) ? 1 : 0;
                tf::split2(k_dbl, &k_sub, &k_tr);
                hipLaunchKernelGGL(nd::k_begin, dim3(1), dim3(64), 0, s, ns, D, j, going_right,
                                   k_sub.hi, k_sub.lo);
                const int leaves = 1 << j;
                for (int l = 0; l < leaves; ++l) {
                    rc = launch_eval(c, 1, zn, ns + nd::H_LEAF_PE, gr, ns + nd::H_LEAF_AUX0, s, ns,
                                     max_depth);
                    if (rc != BPLHIP_OK) return false;
                }
                hipLaunchKernelGGL(nd::k_end, dim3(1), dim3(64), 0, s, ns, D, max_depth, k_tr.hi,
                                   k_tr.lo);
            }
            // one read-back per batch: header + the tree's current proposal (final if STOP)
            (void)hipMemcpyAsync(h_hdr, ns, (size_t)nd::H_N * 8, hipMemcpyDeviceToHost, s);
            (void)hipMemcpyAsync(hp + D + nd::H_N, nd::vec(ns, D, nd::V_TP_Z), (size_t)D * 8,
                                 hipMemcpyDeviceToHost, s);
            if (!hip_ok(hipStreamSynchronize(s), "sync(doubling)")) return false;
            first_batch = false;
            depth = (int)h_hdr[nd::H_T_DEPTH];
            stop = h_hdr[nd::H_STOP] != 0.0;
        }
        // the proposal becomes the chain's current state (no host wait needed)
        hipLaunchKernelGGL(nd::k_finish, dim3(1), dim3(64), 0, s, ns, D);
        if (!hip_ok(hipGetLastError(), "launch")) return false;
        const double num = h_hdr[nd::H_T_NUM];
        out->accept_prob = num > 0 ? h_hdr[nd::H_T_SUMACC] / num : 0.0;
        out->num_steps = (int)num;
        out->diverging = h_hdr[nd::H_T_DIV] != 0.0;
        out->pe = h_hdr[nd::H_T_PE];
        out->aux[0] = h_hdr[nd::H_T_AUX0];
        out->aux[1] = h_hdr[nd::H_T_AUX1];
        out->aux[2] = h_hdr[nd::H_T_AUX2];
        out->aux[3] = h_hdr[nd::H_T_AUX3];
        std::memcpy(z_out, hp + D + nd::H_N, (size_t)D * 8);
        evals += (int64_t)num;
        last_depth = std::max(1, depth);
        return true;
    }
};


// Lock-step chains (numpyro chain_method="vectorized"): all chains' trees are built
// together; every leapfrog of the batch is ONE chain-vectorised evaluation (dc_vec.hip.h)
// whose tail books each chain's leaf.  Chains whose subtree / tree is complete idle.
struct VecDeviceEngine {
    bplhip_ctx* c;
    hipStream_t s;
    const nuts::Config& cfg;
    int D, max_depth, C;
    double* ns;       // device [C][stride]
    size_t stride;
    double* par;      // device [C][par_stride]
    int par_stride;
    // pinned staging: r [C][D] | inv_mass [C][D] | hdr [C][H_N] | prop [C][D] | par [C][par_stride]
    double *h_r, *h_m, *h_hdr, *h_prop, *h_par;
    int last_depth = 1;
    int rc = BPLHIP_OK;
    int dim() const { return D; }
    bool hip_ok(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        rc = fail(c, BPLHIP_EHIP, "lock-step nuts: %s: %s", what, hipGetErrorString(e));
        return false;
    }
    bool set_state(int ch, const double* z, double* pe_out, bool* finite) {
        double* nsc = ns + (size_t)ch * stride;
        std::memcpy(h_r, z, (size_t)D * 8);
        double* zn = nd::vec(nsc, D, nd::V_ZN);
        double* gr = nd::vec(nsc, D, nd::V_GRAD);
        if (!hip_ok(hipMemcpyAsync(zn, h_r, (size_t)D * 8, hipMemcpyHostToDevice, s), "H2D z")) return false;
        rc = launch_eval(c, 1, zn, nsc + nd::H_LEAF_PE, gr, nsc + nd::H_LEAF_AUX0, s);
        if (rc != BPLHIP_OK) return false;
        (void)hipMemcpyAsync(nd::vec(nsc, D, nd::V_Z), zn, (size_t)D * 8, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(nd::vec(nsc, D, nd::V_G), gr, (size_t)D * 8, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(nsc + nd::H_CUR_PE, nsc + nd::H_LEAF_PE, 8, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(nsc + nd::H_T_AUX0, nsc + nd::H_LEAF_AUX0, 32, hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(h_hdr, nsc, (size_t)nd::H_N * 8, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(h_prop, gr, (size_t)D * 8, hipMemcpyDeviceToHost, s);
        if (!hip_ok(hipStreamSynchronize(s), "sync(set_state)")) return false;
        const double pe = h_hdr[nd::H_LEAF_PE];
        bool ok = std::isfinite(pe);
        for (int i = 0; i < D && ok; ++i) ok = std::isfinite(h_prop[i]);
        *finite = ok;
        *pe_out = pe;
        return true;
    }
    bool transition_all(std::vector<nuts::ChainDriver>& cds, std::vector<nuts::TransitionOut>* outs) {
        bool any_mass = false;
        for (int ch = 0; ch < C; ++ch) {
            nuts::ChainDriver& cd = cds[ch];
            std::memcpy(h_r + (size_t)ch * D, cd.r.data(), (size_t)D * 8);
            std::memcpy(h_m + (size_t)ch * D, cd.inv_mass.data(), (size_t)D * 8);
            any_mass = any_mass || cd.mass_changed;
            // numpyro build_tree: key, direction_key, doubling_key = split(key, 3);
            // _double_tree: key, transition_key = split(doubling_key) -- data independent,
            // so all doublings' directions and keys are known up front
            double* p = h_par + (size_t)ch * par_stride;
            p[0] = cd.step_size;
            tf::Key key = cd.k_tr;
            for (int j = 0; j < max_depth; ++j) {
                tf::Key k_next, k_dir, k_dbl, k_sub, k_tr;
                tf::split3(key, &k_next, &k_dir, &k_dbl);
                key = k_next;
                tf::split2(k_dbl, &k_sub, &k_tr);
                double* q = p + 1 + 5 * j;
                q[0] = tf::bernoulli(k_dir, 0.5) ? 1.0 : 0.0;
                q[1] = (double)k_sub.hi; q[2] = (double)k_sub.lo;
                q[3] = (double)k_tr.hi;  q[4] = (double)k_tr.lo;
            }
        }
        const size_t pitch = stride * 8, row = (size_t)D * 8;
        if (any_mass &&
            !hip_ok(hipMemcpy2DAsync(nd::vec(ns, D, nd::V_INVM), pitch, h_m, row, row, C,
                                     hipMemcpyHostToDevice, s), "H2D inv_mass")) return false;
        if (!hip_ok(hipMemcpy2DAsync(nd::vec(ns, D, nd::V_TL_R), pitch, h_r, row, row, C,
                                     hipMemcpyHostToDevice, s), "H2D r")) return false;
        if (!hip_ok(hipMemcpyAsync(par, h_par, (size_t)C * par_stride * 8, hipMemcpyHostToDevice, s),
                    "H2D par")) return false;
        hipLaunchKernelGGL(nd::kv_init, dim3(C), dim3(64), 0, s, ns, stride, D, par, par_stride,
                           cfg.max_delta_energy);
        int depth = 0;
        bool stop = false, first_batch = true;
        while (!stop && depth < max_depth) {
            int nb = first_batch ? std::max(1, std::min(last_depth, max_depth)) : 1;
            nb = std::min(nb, max_depth - depth);
            for (int j = depth; j < depth + nb; ++j) {
                hipLaunchKernelGGL(nd::kv_begin, dim3(C), dim3(64), 0, s, ns, stride, D, j, par,
                                   par_stride);
                const int leaves = 1 << j;
                for (int l = 0; l < leaves; ++l) {
                    rc = launch_eval_vec(c, C, nd::vec(ns, D, nd::V_ZN), ns + nd::H_LEAF_PE,
                                         nd::vec(ns, D, nd::V_GRAD), ns + nd::H_LEAF_AUX0, s, ns,
                                         (int)stride, max_depth);
                    if (rc != BPLHIP_OK) return false;
                }
                hipLaunchKernelGGL(nd::kv_end, dim3(C), dim3(64), 0, s, ns, stride, D, j, max_depth,
                                   par, par_stride);
            }
            // one read-back per batch: every chain's header + current proposal
            (void)hipMemcpy2DAsync(h_hdr, (size_t)nd::H_N * 8, ns, pitch, (size_t)nd::H_N * 8, C,
                                   hipMemcpyDeviceToHost, s);
            (void)hipMemcpy2DAsync(h_prop, row, nd::vec(ns, D, nd::V_TP_Z), pitch, row, C,
                                   hipMemcpyDeviceToHost, s);
            if (!hip_ok(hipStreamSynchronize(s), "sync(doubling)")) return false;
            first_batch = false;
            depth += nb;
            stop = true;
            for (int ch = 0; ch < C; ++ch) stop = stop && h_hdr[(size_t)ch * nd::H_N + nd::H_STOP] != 0.0;
        }
        hipLaunchKernelGGL(nd::kv_finish, dim3(C), dim3(64), 0, s, ns, stride, D);
        if (!hip_ok(hipGetLastError(), "launch")) return false;
        int dmax = 1;
        for (int ch = 0; ch < C; ++ch) {
            const double* hd = h_hdr + (size_t)ch * nd::H_N;
            nuts::TransitionOut& o = (*outs)[ch];
            const double num = hd[nd::H_T_NUM];
            o.accept_prob = num > 0 ? hd[nd::H_T_SUMACC] / num : 0.0;
            o.num_steps = (int)num;
            o.diverging = hd[nd::H_T_DIV] != 0.0;
            o.pe = hd[nd::H_T_PE];
            for (int i = 0; i < 4; ++i) o.aux[i] = hd[nd::H_T_AUX0 + i];
            std::memcpy(cds[ch].z.data(), h_prop + (size_t)ch * D, (size_t)D * 8);
            dmax = std::max(dmax, (int)hd[nd::H_T_DEPTH]);
        }
        last_depth = dmax;
        return true;
    }
};

// Persistent chains (nuts_dev.hip.h): the host finds the initial states, generates every
// chain's random inputs (they are data independent), uploads them, and from then on only
// enqueues evaluations -- C == 1: the single-chain kernel, else the chain-vectorised one --
// checking the chains' "all done" flags once per chunk of launches.

// the leaf can run in dc_eval's tail (nuts_dev.hip.h): the basic / extended models, <= 64 teams
static bool leaf_in_tail(const bplhip_ctx* c) {
    bool staged = true;
    for (int pi = 0; pi < c->n_parts; ++pi) staged = staged && c->parts[pi].staged;
    return !c->neutral && !c->dynamic && c->L.T <= 64 && staged && c->L.D <= 64 * nd::LEAF_NE_MAX;
}
// persistent chains keep all momentum draws of a run on the device: [C][n_iter][D] doubles
// ... and the wide leaf's grid row (kw_leaf: its workgroups poll each other's records and, when a
// subtree is complete, meet at row barriers) must fit the device at once.  Workgroups are dispatched in
// order, so a row never waits for a later one -- but a row that does not fit would wait for itself.
static bool persistent_fits(const bplhip_ctx* c, const bplhip_nuts_cfg* cfg, int C) {
    const double bytes = (double)C * (cfg->num_warmup + cfg->num_samples) * bplhip_latent_dim(c) * 8.0;
    if (nd::kw_workgroups(bplhip_latent_dim(c), nd::KW_NTB) > c->n_cu) return false;
    return bytes <= 16.0 * 1024 * 1024 * 1024;
}

int run_chains_persistent(bplhip_ctx* c, hipStream_t s, const nuts::Config& nc, int C, const double* z0,
                          const tf::Key* keys, double* draws_out, std::vector<nuts::Result>* res) {
    const int D = bplhip_latent_dim(c), md = nc.max_tree_depth;
    // the leaf as its own launch(es) after a plain evaluation: one wave per chain (kp_leaf) up
    // to 256 latent entries, GW workgroups per chain (kw_leaf) beyond
    const bool generic = !leaf_in_tail(c);
    const bool wide = generic && D > 64 * nd::LEAF_NE_MAX;
    const int GWB = nd::kw_workgroups(D, nd::KW_NTB);
    const int n_iter = nc.num_warmup + nc.num_samples;
    const int kept = nc.num_samples / nc.thinning;
    const size_t nsd = (nd::ns_doubles(D, md) + 1) & ~(size_t)1;
    const size_t stride = (nsd + nd::pd_doubles(D) + 1) & ~(size_t)1;
    const std::vector<nuts::Window> sched = nuts::build_adaptation_schedule(nc.num_warmup);
    std::vector<int> win_end;
    for (const auto& w : sched) win_end.push_back(w.end);
    if (win_end.empty()) win_end.push_back(-1);

    DevBuf d_ns, d_norm, d_par, d_win, d_draws, d_stats, d_desc, d_part, d_tick, d_rowpart;
    if (wide) {
        HIP_TRY(c, d_part.ensure((size_t)C * GWB * nd::KW_PW * sizeof(nd::TaggedSum)));
        HIP_TRY(c, hipMemsetAsync(d_part.p, 0, (size_t)C * GWB * nd::KW_PW * sizeof(nd::TaggedSum), s));   // (tag 0: nobody's)
        HIP_TRY(c, d_tick.ensure((size_t)C * nd::RT_WORDS * 4));   // per chain: ticket, row barrier, exit counter
        HIP_TRY(c, hipMemsetAsync(d_tick.p, 0, (size_t)C * nd::RT_WORDS * 4, s));
        HIP_TRY(c, d_rowpart.ensure((size_t)C * nd::row_part_doubles() * 8));
    }
    HIP_TRY(c, d_ns.ensure((size_t)C * stride * 8));
    HIP_TRY(c, hipMemsetAsync(d_ns.p, 0, (size_t)C * stride * 8, s));
    HIP_TRY(c, d_norm.ensure((size_t)C * n_iter * D * 8));
    HIP_TRY(c, d_par.ensure((size_t)C * n_iter * md * 5 * 8));
    HIP_TRY(c, d_win.ensure(win_end.size() * 4));
    HIP_TRY(c, d_draws.ensure((size_t)C * kept * D * 8));
    HIP_TRY(c, d_stats.ensure((size_t)C * kept * 6 * 8));
    HIP_TRY(c, d_desc.ensure(sizeof(nd::Persist)));
    double* ns = d_ns.as<double>();

    // ---- initial states (ChainDriver::init: key plumbing + init_to_uniform with retries)
    res->assign(C, nuts::Result{});
    std::vector<nuts::ChainDriver> cds;
    cds.reserve(C);
    for (int ch = 0; ch < C; ++ch) cds.emplace_back(nc, D, draws_out + (size_t)ch * kept * D, &(*res)[ch]);
    std::vector<double> stage(std::max<size_t>((size_t)D + nd::H_N, 64));
    int rc = BPLHIP_OK;
    for (int ch = 0; ch < C; ++ch) {
        double* nsc = ns + (size_t)ch * stride;
        auto set_state = [&](const double* zz, double* pe, bool* fin) {
            double* zn = nd::vec(nsc, D, nd::V_ZN);
            double* gr = nd::vec(nsc, D, nd::V_GRAD);
            if (hipMemcpyAsync(zn, zz, (size_t)D * 8, hipMemcpyHostToDevice, s) != hipSuccess) return false;
            rc = launch_eval(c, 1, zn, nsc + nd::H_LEAF_PE, gr, nsc + nd::H_LEAF_AUX0, s);
            if (rc != BPLHIP_OK) return false;
            (void)hipMemcpyAsync(nd::vec(nsc, D, nd::V_Z), zn, (size_t)D * 8, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(nd::vec(nsc, D, nd::V_G), gr, (size_t)D * 8, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(nsc + nd::H_CUR_PE, nsc + nd::H_LEAF_PE, 8, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(nsc + nd::H_T_AUX0, nsc + nd::H_LEAF_AUX0, 32, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(stage.data(), nsc + nd::H_LEAF_PE, 8, hipMemcpyDeviceToHost, s);
            (void)hipMemcpyAsync(stage.data() + 1, gr, (size_t)D * 8, hipMemcpyDeviceToHost, s);
            if (hipStreamSynchronize(s) != hipSuccess) return false;
            bool ok = std::isfinite(stage[0]);
            for (int i = 0; i < D && ok; ++i) ok = std::isfinite(stage[1 + i]);
            *fin = ok;
            *pe = stage[0];
            return true;
        };
        const int st = cds[ch].init(set_state, z0 ? z0 + (size_t)ch * D : nullptr, keys[ch]);
        if (st == nuts::ST_EVAL_FAILED) return rc != BPLHIP_OK ? rc : fail(c, BPLHIP_EHIP, "persistent nuts: init failed");
        if (st == nuts::ST_NO_FINITE_INIT) return BPLHIP_ENUMERIC;
    }

    // ---- all random inputs of every chain (sample_kernel / build_tree / _double_tree splits)
    {
        std::vector<double> nrm((size_t)C * n_iter * D), par((size_t)C * n_iter * md * 5);
        std::vector<tf::Key> k_moms((size_t)C * n_iter);
        for (int ch = 0; ch < C; ++ch) {
            tf::Key key_hmc = cds[ch].key_hmc;
            for (int it = 0; it < n_iter; ++it) {
                tf::Key k_mom, k_tr;
                tf::split3(key_hmc, &key_hmc, &k_mom, &k_tr);
                k_moms[(size_t)ch * n_iter + it] = k_mom;
                tf::Key key = k_tr;
                for (int j = 0; j < md; ++j) {
                    tf::Key k_next, k_dir, k_dbl, k_sub, k_t2;
                    tf::split3(key, &k_next, &k_dir, &k_dbl);
                    key = k_next;
                    tf::split2(k_dbl, &k_sub, &k_t2);
                    double* q = par.data() + (((size_t)ch * n_iter + it) * md + j) * 5;
                    q[0] = tf::bernoulli(k_dir, 0.5) ? 1.0 : 0.0;
                    q[1] = (double)k_sub.hi; q[2] = (double)k_sub.lo;
                    q[3] = (double)k_t2.hi;  q[4] = (double)k_t2.lo;
                }
            }
        }
        {   // the momentum draws themselves (C * n_iter * D normals): host threads for long vectors
            const size_t jobs = (size_t)C * n_iter;
            unsigned nthr = nrm.size() > (size_t)1 << 20 ? std::thread::hardware_concurrency() : 1;
            nthr = std::max(1u, std::min(nthr, 32u));
            auto work = [&](unsigned t) {
                for (size_t j = t; j < jobs; j += nthr) tf::normal(k_moms[j], D, nrm.data() + j * D);
            };
            if (nthr == 1) {
                work(0);
            } else {
                std::vector<std::thread> pool;
                for (unsigned t = 0; t < nthr; ++t) pool.emplace_back(work, t);
                for (auto& th : pool) th.join();
            }
        }
        HIP_TRY(c, hipMemcpy(d_norm.p, nrm.data(), nrm.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_par.p, par.data(), par.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d_win.p, win_end.data(), win_end.size() * 4, hipMemcpyHostToDevice));
    }
    nd::Persist P{};
    P.normals = d_norm.as<const double>();
    P.par = d_par.as<const double>();
    P.win_end = d_win.as<const int>();
    P.draws = d_draws.as<double>();
    P.stats = d_stats.as<double>();
    P.n_iter = n_iter; P.kept = kept; P.max_depth = md; P.n_win = (int)win_end.size(); P.D = D;
    P.pd_off = nsd;
    HIP_TRY(c, hipMemcpy(d_desc.p, &P, sizeof P, hipMemcpyHostToDevice));
    {   // PD blocks + identity mass matrices
        std::vector<double> pd(nd::pd_doubles(D), 0.0), ones(D, 1.0);
        pd[nd::P_WARM] = nc.num_warmup; pd[nd::P_TOTAL] = n_iter; pd[nd::P_STEP] = nc.step_size;
        pd[nd::P_DA_PROX] = std::log(10.0 * nc.step_size);
        pd[nd::P_NWIN] = (double)sched.size();
        pd[nd::P_ADAPT_SS] = nc.adapt_step_size; pd[nd::P_ADAPT_MM] = nc.adapt_mass_matrix;
        pd[nd::P_TARGET] = nc.target_accept_prob; pd[nd::P_THIN] = nc.thinning;
        pd[nd::P_START_IDX] = nc.num_warmup + nc.num_samples % nc.thinning;
        pd[nd::P_MAXDE] = nc.max_delta_energy;
        for (int i = 0; i < D; ++i) pd[nd::P_N + 2 * (size_t)D + i] = 1.0;  // mass_sqrt
        for (int ch = 0; ch < C; ++ch) {
            double* nsc = ns + (size_t)ch * stride;
            HIP_TRY(c, hipMemcpy(nsc + nsd, pd.data(), pd.size() * 8, hipMemcpyHostToDevice));
            HIP_TRY(c, hipMemcpy(nd::vec(nsc, D, nd::V_INVM), ones.data(), (size_t)D * 8, hipMemcpyHostToDevice));
        }
    }
    std::vector<double> evals0(C);
    HIP_TRY(c, hipMemcpy2D(evals0.data(), 8, ns + nd::H_EVALS, stride * 8, 8, C, hipMemcpyDeviceToHost));

    // ---- run: first transitions, then blind chunks of evaluations
    if (wide) hipLaunchKernelGGL(nd::kw_start, dim3(GWB, C), dim3(nd::KW_NTB), 0, s, ns, stride, P,
                                 d_tick.as<unsigned int>(), d_rowpart.as<double>(), c->d_fault);
    else hipLaunchKernelGGL(nd::kp_start, dim3(C), dim3(64), 0, s, ns, stride, P);
    const nd::Persist* dP = d_desc.as<const nd::Persist>();
    std::vector<double> flags(C);
    const bool looped = C == 1 && !generic && loop_ok(c);  // one resident launch per chunk
    const int chunk = looped ? 1024 : 256;
    if (generic)
        c->last_nuts_engine = neutral_leaf_fusable(c) ? BPLHIP_ENGINE_PERSIST_NEU_FUSED
                              : wide                  ? BPLHIP_ENGINE_PERSIST_KW_LEAF
                                                      : BPLHIP_ENGINE_PERSIST_KP_LEAF;
    else if (!looped)   // (looped: launch_loop_t names the leaf it takes)
        c->last_nuts_engine = C == 1                         ? BPLHIP_ENGINE_PERSIST_TAIL
                              : C <= c->opt_gridy_max_chains ? BPLHIP_ENGINE_PERSIST_GRIDY
                                                             : BPLHIP_ENGINE_PERSIST_VEC;
    bool all_done = false;
    // every launch advances every unfinished chain by one leapfrog: an upper bound exists
    const double max_steps = (double)n_iter * (double)((1u << md) - 1) + 2.0 * chunk;
    double steps_done = 0.0;
    // one leapfrog of every unfinished chain: the launches a chunk repeats `chunk` times (same arguments
    // every time: everything lives in the chains' state buffers)
    auto enqueue_leapfrogs = [&](hipStream_t st, int count) -> int {
        int erc = BPLHIP_OK;
        for (int k = 0; k < count; ++k) {
            if (generic && neutral_leaf_fusable(c)) {  // evaluation + leaf of every chain in ONE launch
                erc = launch_eval_neutral(c, C, nullptr, nullptr, nullptr, nullptr, st, ns, stride, md, &P);
                if (erc != BPLHIP_OK) return erc;
                continue;
            }
            if (generic) {
                for (int ch = 0; ch < C && erc == BPLHIP_OK; ++ch) {
                    double* nsc = ns + (size_t)ch * stride;
                    erc = launch_eval(c, 1, nd::vec(nsc, D, nd::V_ZN), nsc + nd::H_LEAF_PE,
                                      nd::vec(nsc, D, nd::V_GRAD), nsc + nd::H_LEAF_AUX0, st);
                }
                if (erc != BPLHIP_OK) return erc;
                if (wide) {
                    hipLaunchKernelGGL(nd::kw_leaf, dim3(GWB, C), dim3(nd::KW_NTB), 0, st, ns, stride, D, md,
                                       d_part.as<nd::TaggedSum>(), d_tick.as<unsigned int>(), P, d_rowpart.as<double>(),
                                       c->d_fault);
                } else {
                    hipLaunchKernelGGL(nd::kp_leaf, dim3(C), dim3(64), (size_t)(D + 8) * 8, st, ns, stride, D,
                                       md, P);
                }
                continue;
            }
            // up to `gridy_max_chains` chains run as grid.y copies of the single-chain launch
            // (62 workgroups each at N = 1e6; measured faster than sharing up to ~32 chains);
            // more chains share the chain-vectorised kernel
            erc = C <= c->opt_gridy_max_chains
                      ? launch_eval(c, C, nd::vec(ns, D, nd::V_ZN), ns + nd::H_LEAF_PE, nd::vec(ns, D, nd::V_GRAD),
                                    ns + nd::H_LEAF_AUX0, st, ns, md, dP, C > 1 ? (int)stride : 0)
                      : launch_eval_vec(c, C, nd::vec(ns, D, nd::V_ZN), ns + nd::H_LEAF_PE,
                                        nd::vec(ns, D, nd::V_GRAD), ns + nd::H_LEAF_AUX0, st, ns, (int)stride,
                                        md, dP);
            if (erc != BPLHIP_OK) return erc;
        }
        return BPLHIP_OK;
    };
    // The chunk as ONE hipGraph, captured once per run and replayed (option chunk_graph, default on): the
    // launches of a chunk are identical, and enqueued one by one each of them paid the host's launch
    // path and the XCDs' staggered start of a stand-alone launch (profiles/r03/dispatch_ramp.txt) --
    // dependent launches of a graph pay neither.
    struct ExecGuard {
        hipGraphExec_t e = nullptr;
        ~ExecGuard() { if (e) (void)hipGraphExecDestroy(e); }
    } chunk_graph;
    if (!looped && c->opt_chunk_graph) {
        // one un-captured leapfrog first: the launch path sizes its buffers and sets its function
        // attributes outside the capture (it advances the chains like any other leapfrog)
        rc = enqueue_leapfrogs(s, 1);
        if (rc != BPLHIP_OK) return rc;
        steps_done += 1.0;
        rc = capture_launches(c, [&](hipStream_t st) { return enqueue_leapfrogs(st, chunk); }, &chunk_graph.e);
        if (rc != BPLHIP_OK) return rc;   // (no graph is not an error: the loop below enqueues launch by launch)
    }
    while (!all_done) {
        if (steps_done > max_steps)
            return fail(c, BPLHIP_EHIP, "persistent nuts: chains did not finish within the leapfrog bound");
        steps_done += chunk;
#ifdef DC_STAMPS  // diagnostic build: stop mid-chain so the stamp record is an ordinary leapfrog's
        if (const char* cap = getenv("BPLHIP_DEBUG_MAX_STEPS"))
            if (steps_done > atof(cap)) return fail(c, BPLHIP_EHIP, "debug: step cap reached");
#endif
        if (looped) {  // the whole chunk inside one resident launch
            rc = launch_eval_loop(c, ns, md, dP, chunk, s);
            if (rc != BPLHIP_OK) return rc;
        } else if (chunk_graph.e) {
            HIP_TRY(c, hipGraphLaunch(chunk_graph.e, s));
        } else {
            rc = enqueue_leapfrogs(s, chunk);
            if (rc != BPLHIP_OK) return rc;
        }
        HIP_TRY(c, hipMemcpy2DAsync(flags.data(), 8, ns + nsd + nd::P_ALLDONE, stride * 8, 8, C,
                                    hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        {   // a hand-off that timed out inside the chunk: stop here, not at the leapfrog bound
            const int frc = consume_fault(c, "persistent nuts");
            if (frc != BPLHIP_OK) return frc;
        }
        all_done = true;
        for (int ch = 0; ch < C; ++ch) all_done = all_done && flags[ch] != 0.0;
    }

    // ---- results
    std::vector<double> stats((size_t)C * kept * 6), pd(nd::pd_doubles(D)), hdr(nd::H_N);
    HIP_TRY(c, hipMemcpy(draws_out, d_draws.p, (size_t)C * kept * D * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(stats.data(), d_stats.p, stats.size() * 8, hipMemcpyDeviceToHost));
    for (int ch = 0; ch < C; ++ch) {
        nuts::Result& r = (*res)[ch];
        const double* nsc = ns + (size_t)ch * stride;
        HIP_TRY(c, hipMemcpy(pd.data(), nsc + nsd, pd.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(hdr.data(), nsc, (size_t)nd::H_N * 8, hipMemcpyDeviceToHost));
        r.potential_energy.resize(kept); r.accept_prob.resize(kept); r.step_size.resize(kept);
        r.aux0.resize(kept); r.num_steps.resize(kept); r.diverging.resize(kept);
        for (int i = 0; i < kept; ++i) {
            const double* st = stats.data() + ((size_t)ch * kept + i) * 6;
            r.potential_energy[i] = st[0]; r.accept_prob[i] = st[1]; r.step_size[i] = st[2];
            r.num_steps[i] = (int)st[3]; r.diverging[i] = (int)st[4]; r.aux0[i] = st[5];
        }
        r.final_step_size = pd[nd::P_STEP];
        r.mean_accept_prob = pd[nd::P_MEAN_ACC];
        r.total_divergences = (int64_t)pd[nd::P_NDIV];
        r.total_leapfrogs = (int64_t)(hdr[nd::H_EVALS] - evals0[ch]);
        r.inverse_mass_matrix.resize(D);
        HIP_TRY(c, hipMemcpy(r.inverse_mass_matrix.data(), nd::vec(const_cast<double*>(nsc), D, nd::V_INVM),
                             (size_t)D * 8, hipMemcpyDeviceToHost));
    }
    return BPLHIP_OK;
}

// numpyro's configuration + the latent sites in model execution order (init key order)
nuts::Config make_nuts_config(const bplhip_ctx* c, const bplhip_nuts_cfg* cfg) {
    nuts::Config nc;
    nc.num_warmup = cfg->num_warmup;
    nc.num_samples = cfg->num_samples;
    nc.max_tree_depth = cfg->max_tree_depth;
    nc.adapt_step_size = cfg->adapt_step_size != 0;
    nc.adapt_mass_matrix = cfg->adapt_mass_matrix != 0;
    nc.thinning = cfg->thinning;
    nc.step_size = cfg->step_size;
    nc.target_accept_prob = cfg->target_accept_prob;
    nc.init_radius = cfg->init_radius;
    nc.max_delta_energy = cfg->max_delta_energy;

    if (c->neutral) {  // bpl/neutral_dixon_coles.py:138-261, model execution order
        const dcn::NeuLayout& L = c->NL;
        const int T = L.T;
        nc.sites = {{L.o_md, 1}, {L.o_s_att, 1}, {L.o_s_def, 1}, {L.o_mha, 1}, {L.o_maa, 1},
                    {L.o_mhd, 1}, {L.o_mad, 1}, {L.o_s_ha, 1}, {L.o_s_aa, 1}, {L.o_s_hd, 1},
                    {L.o_s_ad, 1}};
        if (L.C) nc.sites.push_back({L.o_u, 1});  // bpl/neutral_dixon_coles_WC.py:116 (u first)
        if (L.K) {
            nc.sites.push_back({L.o_bA, L.K});
            nc.sites.push_back({L.o_bD, L.K});
        }
        if (!L.C) nc.sites.push_back({L.o_u, 1});
        for (int o : {L.o_sat, L.o_sdt, L.o_hat, L.o_aat, L.o_hdf, L.o_adf}) nc.sites.push_back({o, T});
        if (L.C) nc.sites.push_back({L.o_conf, L.C});
        nc.sites.push_back({L.o_corr, 1});
    } else if (c->dynamic) {  // bpl/dynamic_dixon_coles.py:74-241, model execution order
        const dcd::DynLayout& L = c->DL;
        const int G = L.G, GT = L.G * L.T;
        nc.sites = {{L.o_mha, G}, {L.o_maa, G}, {L.o_mhd, G}, {L.o_mad, G}, {L.o_s_ha, G},
                    {L.o_s_aa, G}, {L.o_s_hd, G}, {L.o_s_ad, G}, {L.o_s_att, G}, {L.o_s_def, G},
                    {L.o_md, 1}};
        if (L.K) {
            nc.sites.push_back({L.o_bA, L.K});
            nc.sites.push_back({L.o_bD, L.K});
        }
        for (int o : {L.o_u, L.o_sat, L.o_sdt, L.o_hat, L.o_aat, L.o_hdf, L.o_adf})
            nc.sites.push_back({o, GT});
        nc.sites.push_back({L.o_corr, 1});
    } else {  // latent sites in MODEL EXECUTION order (seed-handler key order, Appendix B.5)
        const dc::Layout& L = c->L;
        const int T = L.T, K = L.K;
        if (L.model == dc::MODEL_BASIC) {
            // bpl/dixon_coles.py:46-78
            nc.sites = {{L.o_ha, 1}, {L.o_md, 1}, {L.o_sa, 1}, {L.o_sd, 1},
                        {L.o_adec, T}, {L.o_ddec, T}, {L.o_corr, 1}};
        } else {
            // bpl/extended_dixon_coles.py:112-235
            nc.sites = {{L.o_mha, 1}, {L.o_sh, 1}, {L.o_md, 1}, {L.o_sa, 1}, {L.o_sd, 1}};
            if (K) {
                nc.sites.push_back({L.o_bA, K});
                nc.sites.push_back({L.o_bD, K});
            }
            nc.sites.push_back({L.o_u, 1});
            nc.sites.push_back({L.o_sat, T});
            nc.sites.push_back({L.o_sdt, T});
            nc.sites.push_back({L.o_hadec, T});
            nc.sites.push_back({L.o_corr, 1});
        }
    }

    return nc;
}

void fill_stats(bplhip_nuts_stats* stats, const nuts::Result& res, double wall, int D) {
    if (!stats) return;
    const size_t kept = res.potential_energy.size();
    auto cp = [&](double* dst, const std::vector<double>& v) {
        if (dst) std::memcpy(dst, v.data(), kept * 8);
    };
    cp(stats->potential_energy, res.potential_energy);
    cp(stats->accept_prob, res.accept_prob);
    cp(stats->step_size, res.step_size);
    cp(stats->corr_coef, res.aux0);
    if (stats->num_steps) std::memcpy(stats->num_steps, res.num_steps.data(), kept * 4);
    if (stats->diverging) std::memcpy(stats->diverging, res.diverging.data(), kept * 4);
    stats->final_step_size = res.final_step_size;
    stats->mean_accept_prob = res.mean_accept_prob;
    stats->total_leapfrogs = res.total_leapfrogs;
    stats->total_divergences = res.total_divergences;
    stats->wall_seconds = wall;
    if (stats->inverse_mass_matrix)
        std::memcpy(stats->inverse_mass_matrix, res.inverse_mass_matrix.data(), (size_t)D * 8);
}

}  // namespace

static int bplhip_nuts_run_impl(bplhip_ctx* c, const bplhip_nuts_cfg* cfg, const double* z0,
                               uint32_t seed_hi, uint32_t seed_lo, double* draws_out,
                               bplhip_nuts_stats* stats, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound) return fail(c, BPLHIP_ESTATE, "nuts_run: no fixtures bound");
    if (!cfg || !draws_out) return fail(c, BPLHIP_EINVAL, "nuts_run: null cfg/draws_out");
    if (cfg->num_warmup < 0 || cfg->num_samples < 1 || cfg->max_tree_depth < 1 ||
        cfg->max_tree_depth > 20 || cfg->thinning < 1 || !(cfg->step_size > 0))
        return fail(c, BPLHIP_EINVAL, "nuts_run: bad configuration");
    HIP_TRY(c, hipSetDevice(c->device));
    const int D = bplhip_latent_dim(c);
    const size_t nd = (size_t)2 * D + 1 + 4;
    HIP_TRY(c, c->d_nuts.ensure(nd * 8));
    if (c->h_pinned_bytes < nd * 8) {
        if (c->h_pinned) (void)hipHostFree(c->h_pinned);
        c->h_pinned = nullptr;
        HIP_TRY(c, hipHostMalloc((void**)&c->h_pinned, nd * 8, hipHostMallocDefault));
        c->h_pinned_bytes = nd * 8;
    }
    HipPotential pot{c, static_cast<hipStream_t>(stream), D};
    pot.d_z = c->d_nuts.as<double>();
    pot.d_grad = pot.d_z + D;
    pot.d_pot = pot.d_grad + D;
    pot.d_aux = pot.d_pot + 1;
    pot.hp = c->h_pinned;

    nuts::Config nc = make_nuts_config(c, cfg);

    nuts::Result res;
    const auto t0 = std::chrono::steady_clock::now();
    int st;
    int dev_rc = BPLHIP_OK;
    const bool device_tree = c->opt_device_nuts && leaf_in_tail(c);
    const bool generic_persist = c->opt_device_nuts && c->opt_persistent_nuts && !leaf_in_tail(c) &&
                                 persistent_fits(c, cfg, 1);
    if ((device_tree || generic_persist) && c->opt_persistent_nuts) {
        // the whole chain on the device (nuts_dev.hip.h, persistent chains)
        if (!generic_persist) {
            int rc1 = ensure_slabs_fresh(c, 1, static_cast<hipStream_t>(stream));
            if (rc1 != BPLHIP_OK) return rc1;
        }
        const tf::Key k1{seed_hi, seed_lo};
        std::vector<nuts::Result> pres;
        const int prc = run_chains_persistent(c, static_cast<hipStream_t>(stream), nc, 1, z0, &k1,
                                              draws_out, &pres);
        if (prc == BPLHIP_ENUMERIC)
            return fail(c, BPLHIP_ENUMERIC, "nuts_run: no finite initial point after 100 tries");
        if (prc != BPLHIP_OK) return prc;
        res = pres[0];
        st = nuts::ST_OK;
    } else if (device_tree) {
        const size_t nsd = nd::ns_doubles(D, nc.max_tree_depth);
        HIP_TRY(c, c->d_ns.ensure(nsd * 8));
        HIP_TRY(c, hipMemsetAsync(c->d_ns.p, 0, nsd * 8, static_cast<hipStream_t>(stream)));
        const size_t need = ((size_t)2 * D + nd::H_N) * 8;
        if (c->h_pinned_bytes < need) {
            if (c->h_pinned) (void)hipHostFree(c->h_pinned);
            c->h_pinned = nullptr;
            HIP_TRY(c, hipHostMalloc((void**)&c->h_pinned, need, hipHostMallocDefault));
            c->h_pinned_bytes = need;
        }
        int rc1 = ensure_slabs_fresh(c, 1, static_cast<hipStream_t>(stream));
        if (rc1 != BPLHIP_OK) return rc1;
        DeviceEngine E{c, static_cast<hipStream_t>(stream), nc, D, nc.max_tree_depth,
                       c->d_ns.as<double>(), c->h_pinned};
        c->last_nuts_engine = BPLHIP_ENGINE_DEVICE_TREE;
        // identity mass matrix until adapted
        std::vector<double> ones(D, 1.0);
        HIP_TRY(c, hipMemcpy(nd::vec(E.ns, D, nd::V_INVM), ones.data(), (size_t)D * 8, hipMemcpyHostToDevice));
        st = nuts::run_chain_engine(E, nc, z0, tf::Key{seed_hi, seed_lo}, draws_out, &res);
        dev_rc = E.rc;
    } else {
        c->last_nuts_engine = BPLHIP_ENGINE_HOST_TREE;
        st = nuts::run_chain(pot, nc, z0, tf::Key{seed_hi, seed_lo}, draws_out, &res);
        dev_rc = pot.rc;
    }
    const double wall =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st == nuts::ST_EVAL_FAILED) return dev_rc != BPLHIP_OK ? dev_rc : BPLHIP_EHIP;
    if (st == nuts::ST_NO_FINITE_INIT)
        return fail(c, BPLHIP_ENUMERIC, "nuts_run: no finite initial point after 100 tries");
    fill_stats(stats, res, wall, D);
    return BPLHIP_OK;
}

static int bplhip_nuts_run_chains_impl(bplhip_ctx* c, const bplhip_nuts_cfg* cfg, int32_t n_chains,
                                      const double* z0, const uint32_t* seeds, double* draws_out,
                                      bplhip_nuts_stats* stats, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound) return fail(c, BPLHIP_ESTATE, "nuts_run_chains: no fixtures bound");
    if (!cfg || !draws_out || !seeds) return fail(c, BPLHIP_EINVAL, "nuts_run_chains: null argument");
    if (n_chains < 1 || n_chains > 4096) return fail(c, BPLHIP_EINVAL, "nuts_run_chains: bad n_chains");
    if (cfg->num_warmup < 0 || cfg->num_samples < 1 || cfg->max_tree_depth < 1 ||
        cfg->max_tree_depth > 20 || cfg->thinning < 1 || !(cfg->step_size > 0))
        return fail(c, BPLHIP_EINVAL, "nuts_run_chains: bad configuration");
    // every model whose leaf does not fit dc_eval's tail: persistent chains with the leaf as its
    // own launch(es) (kp_leaf / kw_leaf_*)
    const bool generic_ok = !leaf_in_tail(c) && c->opt_persistent_nuts && persistent_fits(c, cfg, n_chains);
    if (!generic_ok &&
        (!leaf_in_tail(c) || !vec_ok(c) || !(c->vps[0].staged && c->vps[1].staged && c->vps[2].staged)))
        return fail(c, BPLHIP_EUNSUPPORTED,
                    "nuts_run_chains: these chains do not fit on the device (momentum draws > 16 GiB, or "
                    "persistent_nuts=0 with a model outside dc_eval's tail)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int D = bplhip_latent_dim(c), C = n_chains;
    const nuts::Config nc = make_nuts_config(c, cfg);
    if (c->opt_persistent_nuts) {
        if (!generic_ok) {
            int rc0 = ensure_slabs_fresh(c, std::max(1, std::min(C, c->opt_gridy_max_chains)), static_cast<hipStream_t>(stream));
            if (rc0 != BPLHIP_OK) return rc0;
        }
        std::vector<tf::Key> pkeys(C);
        for (int ch = 0; ch < C; ++ch) pkeys[ch] = tf::Key{seeds[2 * ch], seeds[2 * ch + 1]};
        std::vector<nuts::Result> pres;
        const auto pt0 = std::chrono::steady_clock::now();
        const int prc = run_chains_persistent(c, s, nc, C, z0, pkeys.data(), draws_out, &pres);
        const double pwall =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - pt0).count();
        if (prc == BPLHIP_ENUMERIC)
            return fail(c, BPLHIP_ENUMERIC, "nuts_run_chains: no finite initial point after 100 tries");
        if (prc != BPLHIP_OK) return prc;
        if (stats)
            for (int ch = 0; ch < C; ++ch) fill_stats(&stats[ch], pres[ch], pwall, D);
        return BPLHIP_OK;
    }
    const size_t stride = (nd::ns_doubles(D, nc.max_tree_depth) + 1) & ~(size_t)1;
    const int par_stride = nd::par_doubles(nc.max_tree_depth);
    DevBuf d_ns, d_par;
    HIP_TRY(c, d_ns.ensure((size_t)C * stride * 8));
    HIP_TRY(c, d_par.ensure((size_t)C * par_stride * 8));
    HIP_TRY(c, hipMemsetAsync(d_ns.p, 0, (size_t)C * stride * 8, s));
    const size_t pinned = ((size_t)C * (3 * D + nd::H_N + par_stride)) * 8;
    double* hp = nullptr;
    HIP_TRY(c, hipHostMalloc((void**)&hp, pinned, hipHostMallocDefault));
    int rc1 = ensure_slabs_fresh(c, 1, static_cast<hipStream_t>(stream));
    if (rc1 != BPLHIP_OK) {
        (void)hipHostFree(hp);
        return rc1;
    }
    VecDeviceEngine E{c, s, nc, D, nc.max_tree_depth, C, d_ns.as<double>(), stride,
                      d_par.as<double>(), par_stride};
    E.h_r = hp;
    E.h_m = E.h_r + (size_t)C * D;
    E.h_hdr = E.h_m + (size_t)C * D;
    E.h_prop = E.h_hdr + (size_t)C * nd::H_N;
    E.h_par = E.h_prop + (size_t)C * D;
    {   // identity mass matrices until adapted
        std::vector<double> ones((size_t)C * D, 1.0);
        hipError_t e = hipMemcpy2D(nd::vec(E.ns, D, nd::V_INVM), stride * 8, ones.data(), (size_t)D * 8,
                                   (size_t)D * 8, C, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipHostFree(hp);
            return fail(c, BPLHIP_EHIP, "nuts_run_chains: H2D mass: %s", hipGetErrorString(e));
        }
    }
    std::vector<tf::Key> keys(C);
    for (int ch = 0; ch < C; ++ch) keys[ch] = tf::Key{seeds[2 * ch], seeds[2 * ch + 1]};
    std::vector<nuts::Result> res;
    const auto t0 = std::chrono::steady_clock::now();
    c->last_nuts_engine = BPLHIP_ENGINE_LOCKSTEP_VEC;
    const int st = nuts::run_chains_lockstep(E, nc, C, z0, keys.data(), draws_out, &res);
    (void)hipStreamSynchronize(s);
    const double wall =
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    (void)hipHostFree(hp);
    if (st == nuts::ST_EVAL_FAILED) return E.rc != BPLHIP_OK ? E.rc : BPLHIP_EHIP;
    if (st == nuts::ST_NO_FINITE_INIT)
        return fail(c, BPLHIP_ENUMERIC, "nuts_run_chains: no finite initial point after 100 tries");
    if (stats)
        for (int ch = 0; ch < C; ++ch) fill_stats(&stats[ch], res[ch], wall, D);
    return BPLHIP_OK;
}

static int bplhip_constrain_impl(bplhip_ctx* c, const double* z_draws, int64_t s,
                                double* attack, double* defence, double* home_advantage,
                                double* corr_coef) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound) return fail(c, BPLHIP_ESTATE, "constrain: no fixtures bound");
    if (c->dynamic) return fail(c, BPLHIP_ESTATE, "constrain: use bplhip_constrain_dynamic");
    if (c->neutral) return fail(c, BPLHIP_ESTATE, "constrain: the neutral model's sites are mapped by the caller");
    if (!z_draws || s < 0) return fail(c, BPLHIP_EINVAL, "constrain: bad argument");
    const dc::Layout& L = c->L;
    const int T = L.T;
    const double* xs = c->h_xs.empty() ? nullptr : c->h_xs.data();
    const bool clip = L.model == dc::MODEL_EXTENDED;
    std::vector<double> att(T), def(T), ha(T);
    for (int64_t i = 0; i < s; ++i) {
        const double* z = z_draws + (size_t)i * L.D;
        for (int t = 0; t < T; ++t) dc::team_params(L, z, xs, t, &att[t], &def[t], &ha[t]);
        if (attack) std::memcpy(attack + (size_t)i * T, att.data(), (size_t)T * 8);
        if (defence) std::memcpy(defence + (size_t)i * T, def.data(), (size_t)T * 8);
        if (home_advantage) {
            if (L.model == dc::MODEL_BASIC) home_advantage[i] = ha[0];
            else std::memcpy(home_advantage + (size_t)i * T, ha.data(), (size_t)T * 8);
        }
        if (corr_coef) {
            // compute_corr_coef_bounds (bpl/_util.py:23-30) over the unique pairs
            double M = 0.0, Lh = 0.0, La = 0.0;
            for (uint32_t pk : c->h_pairs) {
                const int h = pk & 0xFFFFu, a = pk >> 16;
                double lh = std::exp(att[h] - def[a] + ha[h]);
                double la = std::exp(att[a] - def[h]);
                if (clip) {
                    lh = std::fmin(lh, dc::RATE_CLIP);
                    la = std::fmin(la, dc::RATE_CLIP);
                }
                M = std::fmax(M, lh * la);
                Lh = std::fmax(Lh, lh);
                La = std::fmax(La, la);
            }
            const double UB = M > 1.0 ? 1.0 / M : 1.0;
            const double LB = -1.0 / std::fmax(Lh, La);
            double q, dq;
            dc::clipped_sigmoid(z[L.o_corr], &q, &dq);
            corr_coef[i] = LB + q * (UB - LB);
        }
    }
    return BPLHIP_OK;
}

// Dynamic model: constrained / deterministic sites per draw.  HOST in, HOST out; outputs
// [s, G, T] each (any may be NULL): attack, defence (the walk), home_attack, away_attack,
// home_defence, away_defence.  corr_coef comes from the sampler statistics.
static int bplhip_constrain_dynamic_impl(bplhip_ctx* c, const double* z_draws, int64_t s,
                                        double* attack, double* defence, double* home_attack,
                                        double* away_attack, double* home_defence,
                                        double* away_defence) {
    if (!c) return BPLHIP_EINVAL;
    if (!c->bound || !c->dynamic) return fail(c, BPLHIP_ESTATE, "constrain_dynamic: no dynamic model bound");
    if (!z_draws || s < 0) return fail(c, BPLHIP_EINVAL, "constrain_dynamic: bad argument");
    const dcd::DynLayout& L = c->DL;
    const int G = L.G, T = L.T, K = L.K;
    const size_t GT = (size_t)G * T;
    for (int64_t i = 0; i < s; ++i) {
        const double* z = z_draws + (size_t)i * L.D;
        for (int t = 0; t < T; ++t) {
            double att = 0.0, def = z[L.o_md];
            for (int k = 0; k < K; ++k) {
                att += c->h_xs[(size_t)t * K + k] * z[L.o_bA + k];
                def += c->h_xs[(size_t)t * K + k] * z[L.o_bD + k];
            }
            for (int g = 0; g < G; ++g) {
                const size_t cidx = (size_t)g * T + t, o = (size_t)i * GT + cidx;
                double a_ = 0.0, d_ = 0.0;
                if (c->dyn_random_walk) {
                    att += z[L.o_sat + cidx] * std::exp(z[L.o_s_att + g]);
                    def += z[L.o_sdt + cidx] * std::exp(z[L.o_s_def + g]);
                    a_ = att;
                    d_ = def;
                }
                if (attack) attack[o] = a_;
                if (defence) defence[o] = d_;
                if (home_attack) home_attack[o] = z[L.o_mha + g] + std::exp(z[L.o_s_ha + g]) * z[L.o_hat + cidx];
                if (away_attack) away_attack[o] = z[L.o_maa + g] + std::exp(z[L.o_s_aa + g]) * z[L.o_aat + cidx];
                if (home_defence) home_defence[o] = z[L.o_mhd + g] + std::exp(z[L.o_s_hd + g]) * z[L.o_hdf + cidx];
                if (away_defence) away_defence[o] = z[L.o_mad + g] + std::exp(z[L.o_s_ad + g]) * z[L.o_adf + cidx];
            }
        }
    }
    return BPLHIP_OK;
}

// ---- predict path on the device (rows f-2, f-4)
enum { PT_ATT = 0, PT_DEF, PT_HA, PT_HAT, PT_AAT, PT_HDF, PT_ADF, PT_CONF };
// one posterior table: float64 as given + float32 transposed (a column's draws contiguous)
static int predict_upload(bplhip_ctx* c, int which, const double* src, size_t rows, size_t cols) {
    HIP_TRY(c, c->dp_tab[which].ensure(rows * cols * 8));
    HIP_TRY(c, hipMemcpy(c->dp_tab[which].p, src, rows * cols * 8, hipMemcpyHostToDevice));
    std::vector<float> tmp(rows * cols);
    for (size_t r = 0; r < rows; ++r)
        for (size_t q = 0; q < cols; ++q) tmp[q * rows + r] = (float)src[r * cols + q];
    HIP_TRY(c, c->dp_tab32[which].ensure(tmp.size() * 4));
    HIP_TRY(c, hipMemcpy(c->dp_tab32[which].p, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    return BPLHIP_OK;
}
static int predict_upload_corr(bplhip_ctx* c, const double* corr_coef, size_t s) {
    HIP_TRY(c, c->dp_corr.ensure(s * 8));
    HIP_TRY(c, hipMemcpy(c->dp_corr.p, corr_coef, s * 8, hipMemcpyHostToDevice));
    std::vector<float> tmp(s);
    for (size_t r = 0; r < s; ++r) tmp[r] = (float)corr_coef[r];
    HIP_TRY(c, c->dp_corr32.ensure(s * 4));
    HIP_TRY(c, hipMemcpy(c->dp_corr32.p, tmp.data(), s * 4, hipMemcpyHostToDevice));
    return BPLHIP_OK;
}

static int bplhip_predict_set_posterior_impl(bplhip_ctx* c, int32_t s, int32_t t,
                                            const double* attack, const double* defence,
                                            const double* home_advantage,
                                            int32_t home_advantage_per_team,
                                            const double* corr_coef) {
    if (!c) return BPLHIP_EINVAL;
    if (s < 1 || t < 1 || !attack || !defence || !home_advantage || !corr_coef)
        return fail(c, BPLHIP_EINVAL, "predict_set_posterior: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    c->pred_S = 0;
    c->pred_tm = false;
    int rc = predict_upload(c, PT_ATT, attack, (size_t)s, (size_t)t);
    if (rc == BPLHIP_OK) rc = predict_upload(c, PT_DEF, defence, (size_t)s, (size_t)t);
    if (rc == BPLHIP_OK) rc = predict_upload(c, PT_HA, home_advantage, (size_t)s, home_advantage_per_team ? (size_t)t : 1);
    if (rc == BPLHIP_OK) rc = predict_upload_corr(c, corr_coef, (size_t)s);
    if (rc != BPLHIP_OK) return rc;
    c->pred_S = s;
    c->pred_T = t;
    c->pred_C = 0;
    c->pred_ha_stride = home_advantage_per_team ? t : 0;
    c->pred_venue = false;
    return BPLHIP_OK;
}

static int bplhip_predict_set_posterior_venue_impl(bplhip_ctx* c, int32_t s, int32_t t, const double* attack,
                                                  const double* defence, const double* home_attack,
                                                  const double* away_attack, const double* home_defence,
                                                  const double* away_defence, int32_t n_conf,
                                                  const double* confederation_strength,
                                                  const double* corr_coef) {
    if (!c) return BPLHIP_EINVAL;
    if (s < 1 || t < 1 || !attack || !defence || !home_attack || !away_attack || !home_defence ||
        !away_defence || !corr_coef || n_conf < 0 || (n_conf > 0) != (confederation_strength != nullptr))
        return fail(c, BPLHIP_EINVAL, "predict_set_posterior_venue: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    c->pred_S = 0;
    c->pred_tm = false;
    const double* src[6] = {attack, defence, home_attack, away_attack, home_defence, away_defence};
    const int slot[6] = {PT_ATT, PT_DEF, PT_HAT, PT_AAT, PT_HDF, PT_ADF};
    for (int i = 0; i < 6; ++i) {
        const int rc = predict_upload(c, slot[i], src[i], (size_t)s, (size_t)t);
        if (rc != BPLHIP_OK) return rc;
    }
    if (n_conf) {
        const int rc = predict_upload(c, PT_CONF, confederation_strength, (size_t)s, (size_t)n_conf);
        if (rc != BPLHIP_OK) return rc;
    }
    const int rc = predict_upload_corr(c, corr_coef, (size_t)s);
    if (rc != BPLHIP_OK) return rc;
    c->pred_S = s;
    c->pred_T = t;
    c->pred_C = n_conf;
    c->pred_ha_stride = 0;
    c->pred_venue = true;
    return BPLHIP_OK;
}

// argument checks shared by every query entry point (the goal columns are the entry's own to check)
static int predict_check_query(bplhip_ctx* c, const char* what, const bplhip_fixtures* q) {
    if (!q) return fail(c, BPLHIP_EINVAL, "%s: null fixtures record", what);
    const bool venue = q->venue != 0;
    const int64_t m = q->m;
    if (c->pred_S == 0) return fail(c, BPLHIP_ESTATE, "%s: no posterior set", what);
    if (venue != c->pred_venue)
        return fail(c, BPLHIP_ESTATE, "%s: the posterior was set with predict_set_posterior%s", what,
                    c->pred_venue ? "_venue" : "");
    if (m < 0 || m > 0x7FFFFFFF || (m > 0 && (!q->home_idx || !q->away_idx)))
        return fail(c, BPLHIP_EINVAL, "%s: bad argument", what);
    if (venue && m > 0 && (!q->neutral_venue || (c->pred_C > 0) != (q->home_conf != nullptr) || (q->home_conf != nullptr) != (q->away_conf != nullptr)))
        return fail(c, BPLHIP_EINVAL, "%s: neutral_venue is required, confederations exactly when the posterior has them", what);
    for (int64_t i = 0; i < m; ++i) {
        if (q->home_idx[i] >= c->pred_T || q->away_idx[i] >= c->pred_T)
            return fail(c, BPLHIP_EINVAL, "%s: team index out of range at %lld", what, (long long)i);
        if (venue && q->home_conf && (q->home_conf[i] >= c->pred_C || q->away_conf[i] >= c->pred_C))
            return fail(c, BPLHIP_EINVAL, "%s: confederation index out of range at %lld", what, (long long)i);
    }
    return BPLHIP_OK;
}

// the posterior as the float64 kernels see it (dc_posterior.hip.h): the row-major tables as uploaded or the
// team-major copies of loglik_team_major ([S] home advantage: one layout).  Relies on set_posterior leaving pred_C = 0
// (plain) / pred_ha_stride = 0 (venue); the other family's tables may be stale or null: no kernel of this one reads them.
static dcq::Posterior<double> posterior_view(const bplhip_ctx* c, bool team_major) {
    const DevBuf* tab = team_major ? c->dp_tm : c->dp_tab;
    auto t = [&](int which) { return tab[which].as<const double>(); };
    const double* ha = c->pred_ha_stride ? t(PT_HA) : c->dp_tab[PT_HA].as<const double>();
    return {c->pred_S, c->pred_T, c->pred_C, t(PT_ATT), t(PT_DEF), ha, c->pred_ha_stride, t(PT_HAT), t(PT_AAT),
            t(PT_HDF), t(PT_ADF), c->pred_C ? t(PT_CONF) : nullptr, c->dp_corr.as<const double>()};
}

// the query columns of a checked query at the head of `buf`: u16 h, a, (x, y with `goals`,) hc, ac then u8 neutral,
// rounded up to 8 bytes, with room for `out_bytes` of results behind them (*out)
static int stage_queries(bplhip_ctx* c, DevBuf& buf, hipStream_t s, const bplhip_fixtures* fx, bool goals,
                         size_t out_bytes, dcq::Queries* Q, char** out) {
    const size_t m = (size_t)fx->m, cols = goals ? 6 : 4, idx_bytes = (m * (2 * cols + 1) + 7) & ~(size_t)7;
    HIP_TRY(c, buf.ensure(idx_bytes + out_bytes));
    uint16_t* q = buf.as<uint16_t>();
    uint16_t* qc = q + (cols - 2) * m;
    uint8_t* qn = reinterpret_cast<uint8_t*>(q + cols * m);
    *Q = dcq::Queries{(long long)m, q, q + m, goals ? q + 2 * m : nullptr, goals ? q + 3 * m : nullptr, qn, qc, qc + m};
    *out = buf.as<char>() + idx_bytes;
    const bool venue = fx->venue != 0;
    const void* src[7] = {fx->home_idx, fx->away_idx, goals ? fx->home_goals : nullptr, goals ? fx->away_goals : nullptr,
                          venue ? fx->neutral_venue : nullptr, venue ? fx->home_conf : nullptr,
                          venue ? fx->away_conf : nullptr};
    const void* dst[7] = {Q->h, Q->a, Q->x, Q->y, qn, qc, qc + m};
    for (int i = 0; i < 7; ++i)
        if (src[i]) HIP_TRY(c, hipMemcpyAsync(const_cast<void*>(dst[i]), src[i], i == 4 ? m : m * 2, hipMemcpyHostToDevice, s));
    return BPLHIP_OK;
}

// sections of one device buffer, each at an 8-byte-aligned offset (a section of 0 bytes takes no room)
struct Carver {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t at = total; total += (bytes + 7) & ~(size_t)7; return at; }
};

static int predict_score_grid_any(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, void* out, bool f32,
                                  void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = f32 ? "predict_score_grid_f32" : "predict_score_grid";
    if (max_goals < 0 || max_goals > dcp::GRID_MAX_GOALS)
        return fail(c, BPLHIP_EINVAL, "%s: max_goals=%d out of range [0,%d]", what, max_goals, dcp::GRID_MAX_GOALS);
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    if (m > 0 && !out) return fail(c, BPLHIP_EINVAL, "%s: bad argument", what);
    if (m == 0) return BPLHIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cells = (size_t)m * (max_goals + 1) * (max_goals + 1);
    const size_t cell_bytes = f32 ? 4 : 8;
    dcp::GridArgs A{};
    dcq::Queries Q;
    char* q_out;
    rc = stage_queries(c, c->dp_q, s, q, false, cells * cell_bytes, &Q, &q_out);
    if (rc != BPLHIP_OK) return rc;
    double* d_out = reinterpret_cast<double*>(q_out);
    for (int k = 0; k < 64; ++k) A.rk[k] = (float)(1.0 / ((double)k + 1.0));  // the constants of the pmf recurrence
    {
        double fct = 1.0;
        for (int k = 0; k < 16; ++k) {
            A.rfact[k] = 1.0 / fct;
            fct *= (double)(k + 1);
        }
    }
    A.S = c->pred_S;
    A.T = c->pred_T;
    A.attack = c->dp_tab32[PT_ATT].as<const float>();
    A.defence = c->dp_tab32[PT_DEF].as<const float>();
    A.home_adv = c->dp_tab32[PT_HA].as<const float>();
    A.ha_stride = c->pred_ha_stride;
    A.home_attack = c->dp_tab32[PT_HAT].as<const float>();
    A.away_attack = c->dp_tab32[PT_AAT].as<const float>();
    A.home_defence = c->dp_tab32[PT_HDF].as<const float>();
    A.away_defence = c->dp_tab32[PT_ADF].as<const float>();
    A.conf = c->pred_C ? c->dp_tab32[PT_CONF].as<const float>() : nullptr;
    A.corr = c->dp_corr32.as<const float>();
    A.M = (int)m;
    A.G = max_goals;
    A.h = Q.h;
    A.a = Q.a;
    A.neutral = Q.neutral;
    A.hc = Q.hc;
    A.ac = Q.ac;
    A.out = f32 ? nullptr : d_out;
    A.out32 = f32 ? reinterpret_cast<float*>(d_out) : nullptr;
    const dim3 grid((unsigned)((m + dcp::GRID_WAVES - 1) / dcp::GRID_WAVES)), block(64 * dcp::GRID_WAVES);
    if (q->venue) hipLaunchKernelGGL(dcp::predict_score_grid<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcp::predict_score_grid<false>, grid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, cells * cell_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

static int predict_score_proba_any(bplhip_ctx* c, const bplhip_fixtures* q, double* out, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "predict_score_proba";
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    if (m > 0 && (!q->home_goals || !q->away_goals || !out)) return fail(c, BPLHIP_EINVAL, "%s: bad argument", what);
    if (m == 0) return BPLHIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    dcp::PredictArgs A{};
    char* q_out;
    rc = stage_queries(c, c->dp_q, s, q, true, (size_t)m * 8, &A.Q, &q_out);
    if (rc != BPLHIP_OK) return rc;
    double* d_out = reinterpret_cast<double*>(q_out);
    A.P = posterior_view(c, false);
    A.out = d_out;
    const dim3 grid((unsigned)((m + 255) / 256)), block(256);
    if (q->venue) hipLaunchKernelGGL(dcp::predict_score_proba<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcp::predict_score_proba<false>, grid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- pointwise log-likelihood (dc_loglik.hip.h)
// the team-major float64 copies of the current posterior, made once per upload on `s`
static int loglik_team_major(bplhip_ctx* c, hipStream_t s) {
    if (c->pred_tm) return BPLHIP_OK;
    const int S = c->pred_S;
    int slots[8], cols[8], n = 0;
    auto add = [&](int which, int k) { slots[n] = which; cols[n] = k; ++n; };
    add(PT_ATT, c->pred_T);
    add(PT_DEF, c->pred_T);
    if (c->pred_venue) {
        for (int which : {PT_HAT, PT_AAT, PT_HDF, PT_ADF}) add(which, c->pred_T);
        if (c->pred_C) add(PT_CONF, c->pred_C);
    } else if (c->pred_ha_stride) {
        add(PT_HA, c->pred_T);   // (a [S] home advantage is read as uploaded)
    }
    for (int i = 0; i < n; ++i) {
        const size_t bytes = (size_t)S * cols[i] * 8;
        HIP_TRY(c, c->dp_tm[slots[i]].ensure(bytes));
        const dim3 grid((unsigned)((cols[i] + 31) / 32), (unsigned)((S + 31) / 32)), block(256);
        hipLaunchKernelGGL(dcl::transpose_f64, grid, block, 0, s, c->dp_tab[slots[i]].as<const double>(),
                           c->dp_tm[slots[i]].as<double>(), S, cols[i]);
        HIP_TRY(c, hipGetLastError());
    }
    c->pred_tm = true;
    return BPLHIP_OK;
}

// M = min(ceil(min(0.2 S, 3 sqrt(S / r_eff))), S - 1)
static long long loglik_tail_size(int S, double r_eff) {
    const double m = std::ceil(std::min(0.2 * S, 3.0 * std::sqrt((double)S / r_eff)));
    return std::min((long long)m, (long long)S - 1);
}

// matrix (out != nullptr) or summary (lppd != nullptr); every check before any device call
static int loglik_any(bplhip_ctx* c, const bplhip_fixtures* q, bool summary, double* out, double r_eff, int32_t psis,
                      double* lppd, double* mean, double* var, double* elpd_loo, double* pareto_k, int32_t* tail_len,
                      void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = summary ? "loglik_summary" : "loglik_matrix";
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (c->pred_S > BPLHIP_LOGLIK_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: %d posterior draws, at most %d", what, c->pred_S, BPLHIP_LOGLIK_MAX_DRAWS);
    if (m > 0 && (!q->home_goals || !q->away_goals || (!summary && !out) || (summary && (!lppd || !mean || !var || (psis && (!elpd_loo || !pareto_k))))))
        return fail(c, BPLHIP_EINVAL, "%s: bad argument", what);
    long long tail_m = 0;
    if (summary && psis) {
        if (!(std::isfinite(r_eff) && r_eff > 0.0))
            return fail(c, BPLHIP_EINVAL, "%s: r_eff = %g must be finite and > 0", what, r_eff);
        tail_m = loglik_tail_size(c->pred_S, r_eff);
        if (tail_m > BPLHIP_LOGLIK_MAX_TAIL)
            return fail(c, BPLHIP_EINVAL, "%s: the PSIS tail of %lld draws (S = %d, r_eff = %g) exceeds %d", what,
                        tail_m, c->pred_S, r_eff, BPLHIP_LOGLIK_MAX_TAIL);
    }
    if (m == 0) return BPLHIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    const size_t out_bytes = summary ? (size_t)m * (5 * 8 + 4) : (size_t)m * c->pred_S * 8;
    dcl::LoglikArgs A{};
    char* q_out;
    rc = stage_queries(c, c->dp_ll, s, q, true, out_bytes, &A.Q, &q_out);
    if (rc != BPLHIP_OK) return rc;
    double* d_out = reinterpret_cast<double*>(q_out);
    A.P = posterior_view(c, true);
    if (summary) {
        A.lppd = d_out;
        A.mean = d_out + m;
        A.var = d_out + 2 * m;
        A.elpd_loo = d_out + 3 * m;
        A.pareto_k = d_out + 4 * m;
        A.tail_len = reinterpret_cast<int32_t*>(d_out + 5 * m);
        A.psis = psis ? 1 : 0;
        A.tail_m = (int)tail_m;
        A.log_dbl_min = std::log(DBL_MIN);
        const dim3 grid((unsigned)((m + dcl::SUM_WAVES - 1) / dcl::SUM_WAVES)), block(64 * dcl::SUM_WAVES);
        if (venue) hipLaunchKernelGGL(dcl::loglik_summary<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(dcl::loglik_summary<false>, grid, block, 0, s, A);
        HIP_TRY(c, hipGetLastError());
        double* dst[5] = {lppd, mean, var, elpd_loo, pareto_k};
        for (int i = 0; i < (psis ? 5 : 3); ++i)
            HIP_TRY(c, hipMemcpyAsync(dst[i], d_out + i * m, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        if (psis && tail_len)
            HIP_TRY(c, hipMemcpyAsync(tail_len, A.tail_len, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    } else {
        A.ll = d_out;
        const dim3 grid((unsigned)((m + 63) / 64), (unsigned)((c->pred_S + 63) / 64)), block(256);
        if (venue) hipLaunchKernelGGL(dcl::loglik_matrix<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(dcl::loglik_matrix<false>, grid, block, 0, s, A);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- outcome probabilities and scoring rules (dc_score.hip.h); every check before any device call
static int outcome_scores_any(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, double* proba,
                              double* draw_sums, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "outcome_scores";
    if (max_goals < 0 || max_goals > dcs::SCORE_MAX_GOALS)
        return fail(c, BPLHIP_EINVAL, "%s: max_goals=%d out of range [0,%d]", what, max_goals, dcs::SCORE_MAX_GOALS);
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (c->pred_S > BPLHIP_LOGLIK_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: %d posterior draws, at most %d", what, c->pred_S, BPLHIP_LOGLIK_MAX_DRAWS);
    if (m < 1 || !q->home_goals || !q->away_goals || !proba || !draw_sums)
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld below 1 or a null argument", what, (long long)m);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    const size_t M = (size_t)m, S = (size_t)c->pred_S;
    dcs::ScoreArgs A{};
    A.TS = (int)((S + dcs::SCORE_DRAWS - 1) / dcs::SCORE_DRAWS);
    A.TN = (int)((M + dcs::SCORE_NF - 1) / dcs::SCORE_NF);
    Carver cv;
    const size_t o_pp = cv.take((size_t)A.TS * M * 24), o_dp = cv.take((size_t)A.TN * S * 24), o_p = cv.take(M * 24),
                 o_d = cv.take(S * 24);
    char* q_out;
    rc = stage_queries(c, c->dp_ll, s, q, true, cv.total, &A.Q, &q_out);
    if (rc != BPLHIP_OK) return rc;
    A.P = posterior_view(c, true);
    A.G = max_goals;
    A.p_part = reinterpret_cast<double*>(q_out + o_pp);
    A.d_part = reinterpret_cast<double*>(q_out + o_dp);
    A.proba = reinterpret_cast<double*>(q_out + o_p);
    A.draw_sums = reinterpret_cast<double*>(q_out + o_d);
    for (int k = 1; k <= dcs::SCORE_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    const dim3 grid((unsigned)A.TN, (unsigned)((A.TS + dcs::SCORE_WAVES - 1) / dcs::SCORE_WAVES)), block(64 * dcs::SCORE_WAVES);
    if (venue) hipLaunchKernelGGL(dcs::outcome_tiles<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcs::outcome_tiles<false>, grid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(dcs::outcome_reduce, dim3((unsigned)((3 * (M + S) + 255) / 256)), dim3(256), 0, s, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(proba, A.proba, M * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(draw_sums, A.draw_sums, S * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- leave-one-out forecasts (dc_loo.hip.h): loglik_any(summary, psis)'s checks plus max_goals, every one before any
// device call
static int loo_scores_any(bplhip_ctx* c, const bplhip_fixtures* q, double r_eff, int32_t max_goals, double* elpd_loo,
                          double* pareto_k, int32_t* tail_len, double* ess, double* proba, double* proba_in_sample,
                          double* pit, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "loo_scores";
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (max_goals < 0 || max_goals > dcs::SCORE_MAX_GOALS)
        return fail(c, BPLHIP_EINVAL, "%s: max_goals=%d out of range [0,%d]", what, max_goals, dcs::SCORE_MAX_GOALS);
    if (c->pred_S > BPLHIP_LOGLIK_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: %d posterior draws, at most %d", what, c->pred_S, BPLHIP_LOGLIK_MAX_DRAWS);
    if (m > 0 && (!q->home_goals || !q->away_goals || !elpd_loo || !pareto_k || !tail_len || !ess || !proba ||
                  !proba_in_sample || !pit))
        return fail(c, BPLHIP_EINVAL, "%s: bad argument", what);
    if (!(std::isfinite(r_eff) && r_eff > 0.0))
        return fail(c, BPLHIP_EINVAL, "%s: r_eff = %g must be finite and > 0", what, r_eff);
    const long long tail_m = loglik_tail_size(c->pred_S, r_eff);
    if (tail_m > BPLHIP_LOGLIK_MAX_TAIL)
        return fail(c, BPLHIP_EINVAL, "%s: the PSIS tail of %lld draws (S = %d, r_eff = %g) exceeds %d", what, tail_m,
                    c->pred_S, r_eff, BPLHIP_LOGLIK_MAX_TAIL);
    if (m == 0) return BPLHIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    const size_t M = (size_t)m;
    Carver cv;
    const size_t o_e = cv.take(M * 8), o_k = cv.take(M * 8), o_s = cv.take(M * 8), o_p = cv.take(M * 24),
                 o_i = cv.take(M * 24), o_t = cv.take(M * 32), o_l = cv.take(M * 4);
    dcloo::LooArgs A{};
    char* q_out;
    rc = stage_queries(c, c->dp_ll, s, q, true, cv.total, &A.Q, &q_out);
    if (rc != BPLHIP_OK) return rc;
    A.P = posterior_view(c, true);
    A.elpd_loo = reinterpret_cast<double*>(q_out + o_e);
    A.pareto_k = reinterpret_cast<double*>(q_out + o_k);
    A.ess = reinterpret_cast<double*>(q_out + o_s);
    A.proba = reinterpret_cast<double*>(q_out + o_p);
    A.proba_in = reinterpret_cast<double*>(q_out + o_i);
    A.pit = reinterpret_cast<double*>(q_out + o_t);
    A.tail_len = reinterpret_cast<int32_t*>(q_out + o_l);
    A.G = max_goals;
    A.tail_m = (int)tail_m;
    A.log_dbl_min = std::log(DBL_MIN);
    for (int k = 1; k <= dcs::SCORE_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    const dim3 grid((unsigned)((m + dcl::SUM_WAVES - 1) / dcl::SUM_WAVES)), block(64 * dcl::SUM_WAVES);
    if (venue) hipLaunchKernelGGL(dcloo::loo_forecast<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcloo::loo_forecast<false>, grid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    const struct { void* dst; const void* src; size_t bytes; } back[7] = {
        {elpd_loo, A.elpd_loo, M * 8}, {pareto_k, A.pareto_k, M * 8}, {ess, A.ess, M * 8}, {proba, A.proba, M * 24},
        {proba_in_sample, A.proba_in, M * 24}, {pit, A.pit, M * 32}, {tail_len, A.tail_len, M * 4}};
    for (const auto& b : back) HIP_TRY(c, hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- sequential updating (dc_sequential.hip.h); every check before any device call
// the fixtures sorted stably by block and packed, cut into chunks of at most SEQ_CHUNK fixtures of one block
struct SeqPlan {
    std::vector<int64_t> perm;   // sorted position -> position in the query
    std::vector<int32_t> chunk_block, chunk_begin, block_chunk;
    std::vector<dcu::SeqFixture> fx;   // sorted order
};

static int seq_plan(bplhip_ctx* c, const char* what, const bplhip_fixtures* q, const int32_t* block_idx,
                    int32_t n_blocks, SeqPlan* pl) {
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    std::vector<int64_t> start((size_t)n_blocks + 1, 0);
    for (int64_t i = 0; i < m; ++i) {
        if (block_idx[i] < 0 || block_idx[i] >= n_blocks)
            return fail(c, BPLHIP_EINVAL, "%s: block index %d out of range [0,%d) at %lld", what, block_idx[i], n_blocks,
                        (long long)i);
        ++start[(size_t)block_idx[i] + 1];
    }
    for (int32_t b = 0; b < n_blocks; ++b) start[b + 1] += start[b];
    pl->perm.resize((size_t)m);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < m; ++i) pl->perm[(size_t)at[block_idx[i]]++] = i;
    }
    pl->block_chunk.assign((size_t)n_blocks + 1, 0);
    for (int32_t b = 0; b < n_blocks; ++b) {
        for (int64_t n = start[b]; n < start[b + 1]; n += dcu::SEQ_CHUNK) {
            pl->chunk_block.push_back(b);
            pl->chunk_begin.push_back((int32_t)n);
        }
        pl->block_chunk[b + 1] = (int32_t)pl->chunk_block.size();
    }
    pl->chunk_begin.push_back((int32_t)m);
    pl->fx.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t n = pl->perm[i];
        dcu::SeqFixture f{};
        f.lgx = std::lgamma((double)q->home_goals[n] + 1.0);
        f.lgy = std::lgamma((double)q->away_goals[n] + 1.0);
        f.h = q->home_idx[n];
        f.a = q->away_idx[n];
        f.x = q->home_goals[n];
        f.y = q->away_goals[n];
        f.hc = venue && q->home_conf ? q->home_conf[n] : 0;
        f.ac = venue && q->away_conf ? q->away_conf[n] : 0;
        f.neutral = venue ? q->neutral_venue[n] : 0;
        pl->fx[i] = f;
    }
    return BPLHIP_OK;
}

// block sums (out != nullptr) or weighted scores (lw != nullptr)
static int seq_any(bplhip_ctx* c, const bplhip_fixtures* q, const int32_t* block_idx, int32_t n_blocks, double* out,
                   const double* lw, int32_t max_goals, double* elpd, double* proba, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const bool sums = lw == nullptr && elpd == nullptr && proba == nullptr;
    const char* what = sums ? "block_loglik" : "weighted_scores";
    if (!sums && (max_goals < 0 || max_goals > dcs::SCORE_MAX_GOALS))
        return fail(c, BPLHIP_EINVAL, "%s: max_goals=%d out of range [0,%d]", what, max_goals, dcs::SCORE_MAX_GOALS);
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (c->pred_S > BPLHIP_LOGLIK_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: %d posterior draws, at most %d", what, c->pred_S, BPLHIP_LOGLIK_MAX_DRAWS);
    if (m < 1 || !q->home_goals || !q->away_goals || !block_idx || (sums ? !out : (!lw || !elpd || !proba)))
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld below 1 or a null argument", what, (long long)m);
    if (n_blocks < 1 || n_blocks > BPLHIP_SEQ_MAX_BLOCKS)
        return fail(c, BPLHIP_EINVAL, "%s: n_blocks=%d out of range [1,%d]", what, n_blocks, BPLHIP_SEQ_MAX_BLOCKS);
    SeqPlan pl;
    rc = seq_plan(c, what, q, block_idx, n_blocks, &pl);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    const size_t M = (size_t)m, S = (size_t)c->pred_S, B = (size_t)n_blocks, NC = pl.chunk_block.size();
    dcu::SeqArgs A{};
    A.M = (long long)m;
    A.B = n_blocks;
    A.NC = (int)NC;
    A.TS = (int)((S + dcu::SEQ_DRAWS - 1) / dcu::SEQ_DRAWS);
    A.G = max_goals;
    Carver cv;
    const size_t o_fx = cv.take(M * sizeof(dcu::SeqFixture)), o_cb = cv.take(NC * 4), o_cg = cv.take((NC + 1) * 4),
                 o_bc = cv.take((B + 1) * 4);
    const size_t o_part = cv.take(sums ? NC * S * 8 : 0), o_A = cv.take(sums ? B * S * 8 : 0);
    const size_t o_lw = cv.take(sums ? 0 : B * S * 8), o_wp = cv.take(sums ? 0 : (size_t)A.TS * M * 40),
                 o_p = cv.take(sums ? 0 : M * 24), o_e = cv.take(sums ? 0 : M * 8);
    HIP_TRY(c, c->dp_ll.ensure(cv.total));
    char* d = c->dp_ll.as<char>();
    A.P = posterior_view(c, true);
    A.fx = reinterpret_cast<const dcu::SeqFixture*>(d + o_fx);
    A.chunk_block = reinterpret_cast<const int32_t*>(d + o_cb);
    A.chunk_begin = reinterpret_cast<const int32_t*>(d + o_cg);
    A.block_chunk = reinterpret_cast<const int32_t*>(d + o_bc);
    HIP_TRY(c, hipMemcpyAsync(d + o_fx, pl.fx.data(), M * sizeof(dcu::SeqFixture), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_cb, pl.chunk_block.data(), NC * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_cg, pl.chunk_begin.data(), (NC + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_bc, pl.block_chunk.data(), (B + 1) * 4, hipMemcpyHostToDevice, s));
    if (sums) {
        A.part = reinterpret_cast<double*>(d + o_part);
        A.A = reinterpret_cast<double*>(d + o_A);
        const dim3 grid((unsigned)NC, (unsigned)((S + dcu::SEQ_STRIP - 1) / dcu::SEQ_STRIP)), block(dcu::SEQ_STRIP);
        if (venue) hipLaunchKernelGGL(dcu::block_ll_tiles<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(dcu::block_ll_tiles<false>, grid, block, 0, s, A);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(dcu::block_ll_reduce, dim3((unsigned)((B * S + 255) / 256)), dim3(256), 0, s, A);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(out, A.A, B * S * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        return BPLHIP_OK;
    }
    A.lw = reinterpret_cast<const double*>(d + o_lw);
    A.w_part = reinterpret_cast<double*>(d + o_wp);
    A.proba = reinterpret_cast<double*>(d + o_p);
    A.elpd = reinterpret_cast<double*>(d + o_e);
    for (int k = 1; k <= dcs::SCORE_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    HIP_TRY(c, hipMemcpyAsync(d + o_lw, lw, B * S * 8, hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)NC, (unsigned)((A.TS + dcu::SEQ_WAVES - 1) / dcu::SEQ_WAVES)), block(64 * dcu::SEQ_WAVES);
    if (venue) hipLaunchKernelGGL(dcu::weighted_tiles<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcu::weighted_tiles<false>, grid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(dcu::weighted_reduce, dim3((unsigned)((4 * M + 255) / 256)), dim3(256), 0, s, A);
    HIP_TRY(c, hipGetLastError());
    std::vector<double> sorted(4 * M);   // proba [M, 3], then elpd [M], in sorted order
    HIP_TRY(c, hipMemcpyAsync(sorted.data(), A.proba, M * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(sorted.data() + 3 * M, A.elpd, M * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < M; ++i) {
        const size_t n = (size_t)pl.perm[i];
        for (int k = 0; k < 3; ++k) proba[n * 3 + k] = sorted[i * 3 + k];
        elpd[n] = sorted[3 * M + i];
    }
    return BPLHIP_OK;
}

// the device layout of a PSIS call over B rows of S draws (ratios, log weights, k, ess, tail length), and the upload
// and launch of dcu::psis_rows on it: shared by psis_weights and weighted_shift
struct PsisCarve {
    Carver cv;
    size_t o_r = 0, o_w = 0, o_k = 0, o_e = 0, o_t = 0;
    Carver& carve(size_t B, size_t S) {
        o_r = cv.take(B * S * 8);
        o_w = cv.take(B * S * 8);
        o_k = cv.take(B * 8);
        o_e = cv.take(B * 8);
        o_t = cv.take(B * 4);
        return cv;
    }
};
static hipError_t psis_rows_launch(const PsisCarve& pc, char* d, size_t B, int32_t n_draws, long long tail_m,
                                   const double* log_ratios, hipStream_t s, dcu::PsisArgs* out) {
    dcu::PsisArgs A{};
    A.R = reinterpret_cast<const double*>(d + pc.o_r);
    A.lw = reinterpret_cast<double*>(d + pc.o_w);
    A.pareto_k = reinterpret_cast<double*>(d + pc.o_k);
    A.ess = reinterpret_cast<double*>(d + pc.o_e);
    A.tail_len = reinterpret_cast<int32_t*>(d + pc.o_t);
    A.S = n_draws;
    A.tail_m = (int)tail_m;
    A.log_dbl_min = std::log(DBL_MIN);
    *out = A;
    hipError_t e = hipMemcpyAsync(d + pc.o_r, log_ratios, B * (size_t)n_draws * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dcu::psis_rows, dim3((unsigned)B), dim3(64), 0, s, A);
    return hipGetLastError();
}

static int psis_weights_any(bplhip_ctx* c, int32_t n_blocks, int32_t n_draws, const double* log_ratios, double r_eff,
                            double* log_weights, double* pareto_k, double* ess, int32_t* tail_len, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "psis_weights";
    if (n_blocks < 1 || n_blocks > BPLHIP_SEQ_MAX_BLOCKS)
        return fail(c, BPLHIP_EINVAL, "%s: n_blocks=%d out of range [1,%d]", what, n_blocks, BPLHIP_SEQ_MAX_BLOCKS);
    if (n_draws < 1 || n_draws > BPLHIP_LOGLIK_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: n_draws=%d out of range [1,%d]", what, n_draws, BPLHIP_LOGLIK_MAX_DRAWS);
    if (!log_ratios || !log_weights || !pareto_k || !ess || !tail_len)
        return fail(c, BPLHIP_EINVAL, "%s: a null argument", what);
    if (!(std::isfinite(r_eff) && r_eff > 0.0))
        return fail(c, BPLHIP_EINVAL, "%s: r_eff = %g must be finite and > 0", what, r_eff);
    const long long tail_m = loglik_tail_size(n_draws, r_eff);
    if (tail_m > BPLHIP_LOGLIK_MAX_TAIL)
        return fail(c, BPLHIP_EINVAL, "%s: the PSIS tail of %lld draws (S = %d, r_eff = %g) exceeds %d", what, tail_m,
                    n_draws, r_eff, BPLHIP_LOGLIK_MAX_TAIL);
    const size_t B = (size_t)n_blocks, S = (size_t)n_draws;
    for (size_t i = 0; i < B * S; ++i)
        if (!(log_ratios[i] < INFINITY))   // NaN or +inf
            return fail(c, BPLHIP_EINVAL, "%s: log ratio %zu is NaN or +inf", what, i);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PsisCarve pc;
    HIP_TRY(c, c->dp_ll.ensure(pc.carve(B, S).total));
    dcu::PsisArgs A{};
    HIP_TRY(c, psis_rows_launch(pc, c->dp_ll.as<char>(), B, n_draws, tail_m, log_ratios, s, &A));
    HIP_TRY(c, hipMemcpyAsync(log_weights, A.lw, B * S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(pareto_k, A.pareto_k, B * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(ess, A.ess, B * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(tail_len, A.tail_len, B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- the summary queries (markets, periods, in-play, slates, ratings): a value per draw, then statistics over the
// draws.  What the five entries share on the host; each keeps its own checks in its own
// order, its values kernel and what it alone reads back.
static int summary_check_range(bplhip_ctx* c, const char* what, const char* name, int32_t v, int lo, int hi) {
    if (v < lo || v > hi) return fail(c, BPLHIP_EINVAL, "%s: %s=%d out of range [%d,%d]", what, name, v, lo, hi);
    return BPLHIP_OK;
}

// the query record, then the cap on the posterior's draws
static int summary_check_record(bplhip_ctx* c, const char* what, const bplhip_fixtures* q, int draws) {
    const int rc = predict_check_query(c, what, q);
    if (rc == BPLHIP_OK && c->pred_S > draws)
        return fail(c, BPLHIP_EINVAL, "%s: %d posterior draws, at most %d", what, c->pred_S, draws);
    return rc;
}

// the head of the three fixture-by-market entries: the scalar ranges, then the record
static int summary_check_query(bplhip_ctx* c, const char* what, const bplhip_fixtures* q, int32_t max_goals, int goals,
                               int32_t n_markets, int markets, int32_t n_quantiles, int draws) {
    int rc = summary_check_range(c, what, "max_goals", max_goals, 0, goals);
    if (rc == BPLHIP_OK) rc = summary_check_range(c, what, "n_markets", n_markets, 1, markets);
    if (rc == BPLHIP_OK) rc = summary_check_range(c, what, "n_quantiles", n_quantiles, 0, BPLHIP_MARKET_MAX_QUANTILES);
    return rc == BPLHIP_OK ? summary_check_record(c, what, q, draws) : rc;
}

static int summary_check_quantiles(bplhip_ctx* c, const char* what, size_t NQ, const double* quantiles) {
    for (size_t i = 0; i < NQ; ++i)
        if (!(quantiles[i] >= 0.0 && quantiles[i] <= 1.0))
            return fail(c, BPLHIP_EINVAL, "%s: quantile %g outside [0, 1]", what, quantiles[i]);
    return BPLHIP_OK;
}

// the workspace rule: 0 selects `preset`; *chunk = how many of the `n` items (`noun`s) of `per_item` bytes fit
static int summary_chunk(bplhip_ctx* c, const char* what, int64_t workspace_bytes, long long preset, size_t per_item,
                         size_t n, const char* noun, size_t* chunk) {
    const size_t ws = workspace_bytes == 0 ? (size_t)preset : (size_t)workspace_bytes;
    if (workspace_bytes < 0 || ws < per_item)
        return fail(c, BPLHIP_EINVAL, "%s: workspace_bytes=%lld holds no %s (%zu bytes each)", what,
                    (long long)workspace_bytes, noun, per_item);
    *chunk = std::min(n, ws / per_item);
    return BPLHIP_OK;
}

// the weights as a values kernel reads them: [pass][cell][kpass], zeros behind the last market.  walk(k, put) calls
// put(w) for market k's `cells` weights in the kernel's order
template <class Walk>
static std::vector<double> summary_pack_weights(size_t K, size_t cells, size_t kpass, Walk&& walk) {
    std::vector<double> wt((K + kpass - 1) / kpass * cells * kpass, 0.0);
    for (size_t k = 0; k < K; ++k) {
        double* to = wt.data() + (k / kpass) * cells * kpass + k % kpass;
        size_t cell = 0;
        walk(k, [&](double w) { to[kpass * cell++] = w; });
    }
    return wt;
}

// market k's weights on the score grid, every one finite: the cells as they stand
static int summary_grid_weights(bplhip_ctx* c, const char* what, const double* weights, size_t K, size_t cells,
                                size_t kpass, std::vector<double>* wt) {
    for (size_t i = 0; i < K * cells; ++i)
        if (!std::isfinite(weights[i]))
            return fail(c, BPLHIP_EINVAL, "%s: weight %zu of market %zu is not finite", what, i % cells, i / cells);
    *wt = summary_pack_weights(K, cells, kpass, [&](size_t k, auto put) {
        for (size_t i = 0; i < cells; ++i) put(weights[k * cells + i]);
    });
    return BPLHIP_OK;
}

// the sections a summary owns in its entry's buffer: NQ quantile levels and the statistics of K rows ("markets") by M
// columns ("fixtures"); the entry takes its own sections around and between the two
struct Summary {
    size_t K, NQ, M;
    size_t o_q = 0, o_mean = 0, o_sd = 0, o_quant = 0;
    void take_levels(Carver& cv) { o_q = cv.take(NQ * 8); }
    void take_stats(Carver& cv) {
        o_mean = cv.take(K * M * 8);
        o_sd = cv.take(K * M * 8);
        o_quant = cv.take(K * NQ * M * 8);
    }
    // the fields of a dcm::MarketArgs (or the dcip::InplayArgs of the same names) behind the sections at `d`
    template <class Args>
    void point(Args& A, char* d) const {
        A.K = (int)K;
        A.NQ = (int)NQ;
        A.q = reinterpret_cast<const double*>(d + o_q);
        A.mean = reinterpret_cast<double*>(d + o_mean);
        A.sd = reinterpret_cast<double*>(d + o_sd);
        A.quant = reinterpret_cast<double*>(d + o_quant);
    }
    // dcm::market_summary's arguments over values another kernel stored: K "markets" of M "fixtures"
    dcm::MarketArgs over(const dcq::Posterior<double>& P, double* vals, char* d) const {
        dcm::MarketArgs B{};
        B.P = P;
        B.Q.M = (long long)M;
        B.vals = vals;
        point(B, d);
        return B;
    }
    hipError_t upload(hipStream_t s, char* d, const double* quantiles) const {
        return NQ ? hipMemcpyAsync(d + o_q, quantiles, NQ * 8, hipMemcpyHostToDevice, s) : hipSuccess;
    }
    hipError_t read(hipStream_t s, const char* d, double* mean, double* sd, double* quantile) const {
        hipError_t e = hipMemcpyAsync(mean, d + o_mean, K * M * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sd, d + o_sd, K * M * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && NQ) e = hipMemcpyAsync(quantile, d + o_quant, K * NQ * M * 8, hipMemcpyDeviceToHost, s);
        return e;
    }
};

// dcm::market_summary over the `rows` (chunk item, market) rows of stored values
static hipError_t summary_launch(bool venue, size_t rows, hipStream_t s, const dcm::MarketArgs& A) {
    const dim3 grid((unsigned)((rows + dcm::MARKET_WAVES - 1) / dcm::MARKET_WAVES)), block(64 * dcm::MARKET_WAVES);
    if (venue) hipLaunchKernelGGL(dcm::market_summary<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcm::market_summary<false>, grid, block, 0, s, A);
    return hipGetLastError();
}

// the chunks of `n` items, `chunk` at a time, as the boundaries summary_chunks takes
static std::vector<size_t> summary_strides(size_t n, size_t chunk) {
    std::vector<size_t> at;
    for (size_t n0 = 0; n0 < n; n0 += chunk) at.push_back(n0);
    at.push_back(n);
    return at;
}

// the chunk loop over items at[i] .. at[i+1]-1: run(n0, nc) launches the chunk's kernels; with `copy`, out(n0, nc)
// copies the chunk's per-draw values to the host (synchronous: the next chunk overwrites them only after it).  Both
// return their first HIP error
template <class Run, class Out>
static int summary_chunks(bplhip_ctx* c, hipStream_t s, const std::vector<size_t>& at, bool copy, Run&& run, Out&& out) {
    for (size_t i = 0; i + 1 < at.size(); ++i) {
        HIP_TRY(c, run(at[i], at[i + 1] - at[i]));
        if (!copy) continue;
        HIP_TRY(c, out(at[i], at[i + 1] - at[i]));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    return BPLHIP_OK;
}

// ---- match markets (dc_market.hip.h); every check before any device call
static int market_summary_any(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, int32_t n_markets,
                              const double* weights, int32_t n_quantiles, const double* quantiles, double* mean,
                              double* sd, double* quantile, double* draws, int64_t workspace_bytes, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "market_summary";
    int rc = summary_check_query(c, what, q, max_goals, dcm::MARKET_MAX_GOALS, n_markets, BPLHIP_MARKET_MAX_MARKETS,
                                 n_quantiles, BPLHIP_LOGLIK_MAX_DRAWS);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (m < 1 || !weights || !mean || !sd || (n_quantiles > 0 && (!quantiles || !quantile)))
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld below 1 or a null argument", what, (long long)m);
    const size_t M = (size_t)m, S = (size_t)c->pred_S, K = (size_t)n_markets;
    const size_t cells = (size_t)(max_goals + 1) * (size_t)(max_goals + 1), per_fixture = K * S * 8;
    Summary sm{K, (size_t)n_quantiles, M};
    std::vector<double> wt;
    size_t chunk;
    rc = summary_grid_weights(c, what, weights, K, cells, dcm::MARKET_KPASS, &wt);
    if (rc == BPLHIP_OK) rc = summary_check_quantiles(c, what, sm.NQ, quantiles);
    if (rc == BPLHIP_OK)
        rc = summary_chunk(c, what, workspace_bytes, BPLHIP_MARKET_WORKSPACE_BYTES, per_fixture, M, "fixture", &chunk);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    Carver cv;
    const size_t o_w = cv.take(wt.size() * 8);
    sm.take_levels(cv);
    sm.take_stats(cv);
    const size_t o_vals = cv.take(chunk * per_fixture);
    dcm::MarketArgs A{};
    char* d;
    rc = stage_queries(c, c->dp_mkt, s, q, false, cv.total, &A.Q, &d);
    if (rc != BPLHIP_OK) return rc;
    A.P = posterior_view(c, true);
    A.G = max_goals;
    A.w = reinterpret_cast<const double*>(d + o_w);
    A.vals = reinterpret_cast<double*>(d + o_vals);
    sm.point(A, d);
    for (int k = 1; k <= dcm::MARKET_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    HIP_TRY(c, hipMemcpyAsync(d + o_w, wt.data(), wt.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, sm.upload(s, d, quantiles));
    const dim3 block(64 * dcm::MARKET_WAVES);
    const unsigned tiles = (unsigned)((S + block.x - 1) / block.x), passes = (unsigned)(wt.size() / (cells * dcm::MARKET_KPASS));
    rc = summary_chunks(c, s, summary_strides(M, chunk), draws != nullptr, [&](size_t n0, size_t nc) {
        A.n0 = (long long)n0;
        A.nc = (long long)nc;
        const dim3 grid((unsigned)nc, tiles, passes);
        if (venue) hipLaunchKernelGGL(dcm::market_values<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(dcm::market_values<false>, grid, block, 0, s, A);
        const hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : summary_launch(venue, nc * K, s, A);
    }, [&](size_t n0, size_t nc) {
        return hipMemcpyAsync(draws + n0 * K * S, A.vals, nc * per_fixture, hipMemcpyDeviceToHost, s);
    });
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, sm.read(s, d, mean, sd, quantile));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- period markets (dc_period.hip.h): bplhip_market_summary's checks in its order, then the splits and the
// weights of the readable cells; every check before any device call
static int period_summary_any(bplhip_ctx* c, const bplhip_fixtures* q, const double* split, int32_t max_goals,
                              int32_t n_markets, const double* weights, int32_t n_quantiles, const double* quantiles,
                              double* mean, double* sd, double* quantile, double* draws, int64_t workspace_bytes,
                              void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "period_summary";
    int rc = summary_check_query(c, what, q, max_goals, BPLHIP_PERIOD_MAX_GOALS, n_markets, BPLHIP_PERIOD_MAX_MARKETS,
                                 n_quantiles, BPLHIP_LOGLIK_MAX_DRAWS);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (m < 1 || !split || !weights || !mean || !sd || (n_quantiles > 0 && (!quantiles || !quantile)))
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld below 1 or a null argument", what, (long long)m);
    const size_t M = (size_t)m, S = (size_t)c->pred_S, K = (size_t)n_markets, per_fixture = K * S * 8;
    const size_t g1 = (size_t)max_goals + 1, full = g1 * g1 * g1 * g1, T = g1 * (g1 + 1) / 2, cells = T * T;
    Summary sm{K, (size_t)n_quantiles, M};
    rc = summary_check_quantiles(c, what, sm.NQ, quantiles);
    if (rc != BPLHIP_OK) return rc;
    for (size_t i = 0; i < M; ++i)
        if (!(split[i] >= 0.0 && split[i] <= 1.0))   // (NaN fails both)
            return fail(c, BPLHIP_EINVAL, "%s: split %g of fixture %zu outside [0, 1]", what, split[i], i);
    // the readable cells in walk order; the first market with a non-finite weight on one
    size_t bad = K;
    const std::vector<double> wt = summary_pack_weights(K, cells, dcpd::PERIOD_KPASS, [&](size_t k, auto put) {
        dcpd::period_walk(max_goals, [&](int a, int b, int x, int y) {
            const double w = weights[k * full + (((size_t)a * g1 + (size_t)b) * g1 + (size_t)x) * g1 + (size_t)y];
            if (!std::isfinite(w)) bad = std::min(bad, k);
            put(w);
        });
    });
    if (bad < K) return fail(c, BPLHIP_EINVAL, "%s: market %zu has a non-finite weight on a readable cell", what, bad);
    size_t chunk;
    rc = summary_chunk(c, what, workspace_bytes, BPLHIP_MARKET_WORKSPACE_BYTES, per_fixture, M, "fixture", &chunk);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    Carver cv;
    const size_t o_w = cv.take(wt.size() * 8);
    sm.take_levels(cv);
    const size_t o_t = cv.take(M * 8);
    sm.take_stats(cv);
    const size_t o_vals = cv.take(chunk * per_fixture);
    dcpd::PeriodArgs P{};
    dcm::MarketArgs& A = P.M;
    char* d;
    rc = stage_queries(c, c->dp_period, s, q, false, cv.total, &A.Q, &d);
    if (rc != BPLHIP_OK) return rc;
    A.P = posterior_view(c, true);
    A.G = max_goals;
    A.w = reinterpret_cast<const double*>(d + o_w);
    P.split = reinterpret_cast<const double*>(d + o_t);
    A.vals = reinterpret_cast<double*>(d + o_vals);
    sm.point(A, d);
    for (int k = 1; k <= dcm::MARKET_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    HIP_TRY(c, hipMemcpyAsync(d + o_w, wt.data(), wt.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, sm.upload(s, d, quantiles));
    HIP_TRY(c, hipMemcpyAsync(d + o_t, split, M * 8, hipMemcpyHostToDevice, s));
    const dim3 block(64 * dcpd::PERIOD_WAVES);
    const unsigned tiles = (unsigned)((S + block.x - 1) / block.x), passes = (unsigned)(wt.size() / (cells * dcpd::PERIOD_KPASS));
    rc = summary_chunks(c, s, summary_strides(M, chunk), draws != nullptr, [&](size_t n0, size_t nc) {
        A.n0 = (long long)n0;
        A.nc = (long long)nc;
        const dim3 grid((unsigned)nc, tiles, passes);
        if (venue) hipLaunchKernelGGL(dcpd::period_values<true>, grid, block, 0, s, P);
        else hipLaunchKernelGGL(dcpd::period_values<false>, grid, block, 0, s, P);
        const hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : summary_launch(venue, nc * K, s, A);   // dcm::market_summary on the stored values
    }, [&](size_t n0, size_t nc) {
        return hipMemcpyAsync(draws + n0 * K * S, A.vals, nc * per_fixture, hipMemcpyDeviceToHost, s);
    });
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, sm.read(s, d, mean, sd, quantile));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- totals over slates of fixtures (dc_slate.hip.h); every check before any device call
static int slate_summary_any(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, int32_t n_slates,
                             const int32_t* start, int32_t n_tables, const uint8_t* tables, const int32_t* leg_table,
                             int32_t n_quantiles, const double* quantiles, double* mean, double* sd, double* quantile,
                             double* leg_mean, double* draws, int64_t workspace_bytes, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "slate_summary";
    int rc = summary_check_range(c, what, "max_goals", max_goals, 0, dcsl::SLATE_MAX_GOALS);
    if (rc == BPLHIP_OK) rc = summary_check_range(c, what, "n_quantiles", n_quantiles, 0, BPLHIP_MARKET_MAX_QUANTILES);
    if (rc == BPLHIP_OK) rc = summary_check_record(c, what, q, BPLHIP_LOGLIK_MAX_DRAWS);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (m < 1 || !start || !tables || !leg_table || !mean || !sd || !leg_mean ||
        (n_quantiles > 0 && (!quantiles || !quantile)))
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld below 1 or a null argument", what, (long long)m);
    if (n_slates < 1 || n_slates > m) return fail(c, BPLHIP_EINVAL, "%s: n_slates=%d out of range [1,m]", what, n_slates);
    if (n_tables < 1 || n_tables > m) return fail(c, BPLHIP_EINVAL, "%s: n_tables=%d out of range [1,m]", what, n_tables);
    const size_t M = (size_t)m, S = (size_t)c->pred_S, J = (size_t)n_slates, NT = (size_t)n_tables, NQ = (size_t)n_quantiles;
    const size_t g1 = (size_t)max_goals + 1, cells = g1 * g1;
    std::vector<int32_t> top(NT, 0);
    for (size_t t = 0; t < NT; ++t)
        for (size_t i = 0; i < cells; ++i) {
            const int v = tables[t * cells + i];
            if (v >= BPLHIP_SLATE_VALUES)
                return fail(c, BPLHIP_EINVAL, "%s: value %d of cell %zu of leg table %zu, at most %d", what, v, i, t,
                            BPLHIP_SLATE_VALUES - 1);
            top[t] = std::max(top[t], (int32_t)v);
        }
    for (size_t i = 0; i < M; ++i)
        if (leg_table[i] < 0 || leg_table[i] >= n_tables)
            return fail(c, BPLHIP_EINVAL, "%s: leg table index out of range at %zu", what, i);
    if (start[0] != 0 || (int64_t)start[J] != m)
        return fail(c, BPLHIP_EINVAL, "%s: start does not cover the %lld fixtures", what, (long long)m);
    int Pmax = 0;
    size_t legs_max = 0;
    for (size_t j = 0; j < J; ++j) {
        if (start[j + 1] <= start[j] || (int64_t)start[j + 1] > m)
            return fail(c, BPLHIP_EINVAL, "%s: start is not increasing at slate %zu", what, j);
        const size_t legs = (size_t)(start[j + 1] - start[j]);
        if (legs > BPLHIP_SLATE_MAX_LEGS)
            return fail(c, BPLHIP_EINVAL, "%s: slate %zu has %zu legs, at most %d", what, j, legs, BPLHIP_SLATE_MAX_LEGS);
        int total = 0;
        for (int32_t f = start[j]; f < start[j + 1]; ++f) total += top[(size_t)leg_table[f]];
        if (total > BPLHIP_SLATE_MAX_TOTAL)
            return fail(c, BPLHIP_EINVAL, "%s: slate %zu can total %d, at most %d", what, j, total, BPLHIP_SLATE_MAX_TOTAL);
        Pmax = std::max(Pmax, total);
        legs_max = std::max(legs_max, legs);
    }
    rc = summary_check_quantiles(c, what, NQ, quantiles);
    if (rc != BPLHIP_OK) return rc;
    const size_t PT = (size_t)Pmax + 1, K = 2 * PT + 2, V = dcsl::SLATE_VALUES;
    // a slate's share of the workspace: its statistics and its fixtures' value laws
    auto slate_bytes = [&](size_t j) { return (K + V * (size_t)(start[j + 1] - start[j])) * S * 8; };
    const size_t ws = workspace_bytes == 0 ? (size_t)BPLHIP_MARKET_WORKSPACE_BYTES : (size_t)workspace_bytes;
    size_t largest = 0;
    for (size_t j = 0; j < J; ++j) largest = std::max(largest, slate_bytes(j));
    if (workspace_bytes < 0 || ws < largest)
        return fail(c, BPLHIP_EINVAL, "%s: workspace_bytes=%lld does not hold the largest slate (%zu bytes)", what,
                    (long long)workspace_bytes, largest);
    // the chunks: consecutive slates while they fit
    std::vector<size_t> chunk_at{0};
    size_t ws_used = 0;
    for (size_t j = 0, bytes = 0; j < J; ++j) {
        if (bytes + slate_bytes(j) > ws) {
            chunk_at.push_back(j);
            bytes = 0;
        }
        bytes += slate_bytes(j);
        ws_used = std::max(ws_used, bytes);
    }
    chunk_at.push_back(J);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    // the tables as the kernel reads them: a row of ceil((G+1) / 8) words of eight cells, zeros past G
    const size_t yb = (g1 + dcsl::SLATE_YB - 1) / dcsl::SLATE_YB;
    std::vector<uint64_t> packed(NT * g1 * yb, 0);
    for (size_t t = 0; t < NT; ++t)
        for (size_t x = 0; x < g1; ++x)
            for (size_t y = 0; y < g1; ++y)
                packed[(t * g1 + x) * yb + y / dcsl::SLATE_YB] |= (uint64_t)tables[t * cells + x * g1 + y] << (8 * (y % dcsl::SLATE_YB));
    Carver cv;
    const size_t o_start = cv.take((J + 1) * 4), o_tab = cv.take(M * 4), o_top = cv.take(NT * 4),
                 o_cells = cv.take(packed.size() * 8);
    Summary sm{K, NQ, J};
    sm.take_levels(cv);
    sm.take_stats(cv);
    const size_t o_lmean = cv.take(V * M * 8), o_lsd = cv.take(V * M * 8), o_ws = cv.take(ws_used);
    dcsl::SlateArgs A{};
    char* d;
    rc = stage_queries(c, c->dp_slate, s, q, false, cv.total, &A.Q, &d);
    if (rc != BPLHIP_OK) return rc;
    A.P = posterior_view(c, true);
    A.G = max_goals;
    A.PT = (int)PT;
    A.start = reinterpret_cast<const int32_t*>(d + o_start);
    A.table = reinterpret_cast<const int32_t*>(d + o_tab);
    A.top = reinterpret_cast<const int32_t*>(d + o_top);
    A.cells = reinterpret_cast<const uint64_t*>(d + o_cells);
    A.vals = reinterpret_cast<double*>(d + o_ws);
    for (int k = 1; k <= dcsl::SLATE_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    // the summaries are dcm::market_summary on the stored values: K "markets" of J "fixtures" with the quantiles,
    // and the SLATE_VALUES "markets" of the M fixtures without (no levels and no quantiles: L's own few fields)
    dcm::MarketArgs B = sm.over(A.P, A.vals, d), L{};
    L.P = A.P;
    L.Q.M = (long long)M;
    L.K = (int)V;
    L.NQ = 0;
    L.mean = reinterpret_cast<double*>(d + o_lmean);
    L.sd = reinterpret_cast<double*>(d + o_lsd);
    HIP_TRY(c, hipMemcpyAsync(d + o_start, start, (J + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_tab, leg_table, M * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_top, top.data(), NT * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_cells, packed.data(), packed.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, sm.upload(s, d, quantiles));
    const unsigned tiles = (unsigned)((S + 63) / 64);
    // a chunk is a run of slates j0 .. j0+jc-1 and of their fixtures f0 .. f0+fc-1
    rc = summary_chunks(c, s, chunk_at, draws != nullptr, [&](size_t j0, size_t jc) {
        const size_t f0 = (size_t)start[j0], fc = (size_t)start[j0 + jc] - f0;
        A.j0 = B.n0 = (long long)j0;
        A.jc = B.nc = (long long)jc;
        A.leg_vals = A.vals + jc * K * S;
        L.vals = A.leg_vals;
        L.n0 = (long long)f0;
        L.nc = (long long)fc;
        const dim3 grid((unsigned)jc, tiles);
        if (venue) hipLaunchKernelGGL(dcsl::slate_values<true>, grid, dim3(64), PT * 512, s, A);
        else hipLaunchKernelGGL(dcsl::slate_values<false>, grid, dim3(64), PT * 512, s, A);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = summary_launch(venue, jc * K, s, B);
        return e != hipSuccess ? e : summary_launch(venue, fc * V, s, L);
    }, [&](size_t j0, size_t jc) {   // a slate's pmf rows are the head of its block of values
        return hipMemcpy2DAsync(draws + j0 * PT * S, PT * S * 8, A.vals, K * S * 8, PT * S * 8, jc, hipMemcpyDeviceToHost, s);
    });
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, sm.read(s, d, mean, sd, quantile));
    HIP_TRY(c, hipMemcpyAsync(leg_mean, L.mean, V * M * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- team ratings against a field of opponents (dc_ratings.hip.h); every check before any device call
static int team_ratings_any(bplhip_ctx* c, int32_t n_teams, const uint16_t* teams, const uint16_t* team_conf,
                            int32_t n_opponents, const uint16_t* opponents, const uint16_t* opponent_conf, int32_t venue,
                            int32_t max_goals, const double* points, int32_t rank_by, int32_t n_quantiles,
                            const double* quantiles, double* mean, double* sd, double* quantile, int32_t* rank_count,
                            int32_t* better_count, int32_t* matches, double* draws, int64_t workspace_bytes,
                            void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "team_ratings";
    if (n_teams < 1 || n_teams > BPLHIP_RATINGS_MAX_TEAMS || n_opponents < 1 || n_opponents > BPLHIP_RATINGS_MAX_TEAMS)
        return fail(c, BPLHIP_EINVAL, "%s: n_teams=%d or n_opponents=%d out of range [1,%d]", what, n_teams, n_opponents,
                    BPLHIP_RATINGS_MAX_TEAMS);
    int rc = summary_check_range(c, what, "venue", venue, 0, 3);
    if (rc == BPLHIP_OK) rc = summary_check_range(c, what, "max_goals", max_goals, 0, dcs::SCORE_MAX_GOALS);
    if (rc == BPLHIP_OK) rc = summary_check_range(c, what, "rank_by", rank_by, 0, dcr::RATINGS_STATS - 1);
    if (rc == BPLHIP_OK) rc = summary_check_range(c, what, "n_quantiles", n_quantiles, 0, BPLHIP_MARKET_MAX_QUANTILES);
    if (rc != BPLHIP_OK) return rc;
    if (c->pred_S == 0) return fail(c, BPLHIP_ESTATE, "%s: no posterior set", what);
    if (c->pred_S > BPLHIP_LOGLIK_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: %d posterior draws, at most %d", what, c->pred_S, BPLHIP_LOGLIK_MAX_DRAWS);
    if (!teams || !opponents || !points || !mean || !sd || !rank_count || !better_count || !matches ||
        (n_quantiles > 0 && (!quantiles || !quantile)))
        return fail(c, BPLHIP_EINVAL, "%s: a null argument", what);
    const bool venue_form = c->pred_venue;
    if (venue == dcr::RATINGS_NEUTRAL && !venue_form)
        return fail(c, BPLHIP_EINVAL, "%s: venue 3 (neutral) needs a posterior set with predict_set_posterior_venue", what);
    const bool conf = venue_form && c->pred_C > 0;
    if (conf != (team_conf != nullptr) || conf != (opponent_conf != nullptr))
        return fail(c, BPLHIP_EINVAL, "%s: confederations exactly when the posterior has them", what);
    const size_t R = (size_t)n_teams, NO = (size_t)n_opponents, S = (size_t)c->pred_S, NQ = (size_t)n_quantiles;
    const size_t K = dcr::RATINGS_STATS;
    for (int side = 0; side < 2; ++side) {
        const uint16_t* idx = side ? opponents : teams;
        const uint16_t* cf = side ? opponent_conf : team_conf;
        const size_t n = side ? NO : R;
        std::vector<char> seen((size_t)c->pred_T, 0);
        for (size_t i = 0; i < n; ++i) {
            if (idx[i] >= c->pred_T)
                return fail(c, BPLHIP_EINVAL, "%s: %s index out of range at %zu", what, side ? "opponent" : "team", i);
            if (seen[idx[i]]) return fail(c, BPLHIP_EINVAL, "%s: duplicate %s at %zu", what, side ? "opponent" : "team", i);
            seen[idx[i]] = 1;
            if (conf && cf[i] >= c->pred_C)
                return fail(c, BPLHIP_EINVAL, "%s: confederation index out of range at %zu", what, i);
        }
    }
    std::vector<int32_t> n_matches(R);
    for (size_t i = 0; i < R; ++i) {
        int32_t others = 0;
        for (size_t j = 0; j < NO; ++j) others += opponents[j] != teams[i];
        if (others == 0) return fail(c, BPLHIP_EINVAL, "%s: team %zu has no opponent other than itself", what, i);
        n_matches[i] = others * (venue == dcr::RATINGS_BOTH ? 2 : 1);
    }
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(points[i])) return fail(c, BPLHIP_EINVAL, "%s: point value %d is not finite", what, i);
    const size_t per_team = K * S * 8;
    size_t chunk;
    rc = summary_check_quantiles(c, what, NQ, quantiles);
    if (rc == BPLHIP_OK)
        rc = summary_chunk(c, what, workspace_bytes, BPLHIP_RATINGS_WORKSPACE_BYTES, per_team, R, "team", &chunk);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    Carver cv;
    const size_t o_t = cv.take(R * 2), o_tc = cv.take(conf ? R * 2 : 0), o_o = cv.take(NO * 2),
                 o_oc = cv.take(conf ? NO * 2 : 0);
    Summary sm{K, NQ, R};
    sm.take_levels(cv);
    sm.take_stats(cv);
    const size_t o_ranked = cv.take(R * S * 8), o_rank = cv.take(R * R * 4), o_better = cv.take(R * R * 4),
                 o_vals = cv.take(chunk * per_team);
    HIP_TRY(c, c->dp_ratings.ensure(cv.total));
    char* d = c->dp_ratings.as<char>();
    dcr::RatingsArgs A{};
    A.P = posterior_view(c, true);
    A.R = n_teams;
    A.NO = n_opponents;
    A.venue = venue;
    A.G = max_goals;
    A.rank_by = rank_by;
    A.team = reinterpret_cast<const uint16_t*>(d + o_t);
    A.tconf = conf ? reinterpret_cast<const uint16_t*>(d + o_tc) : nullptr;
    A.opp = reinterpret_cast<const uint16_t*>(d + o_o);
    A.oconf = conf ? reinterpret_cast<const uint16_t*>(d + o_oc) : nullptr;
    A.pw = points[0];
    A.pd = points[1];
    A.pl = points[2];
    A.vals = reinterpret_cast<double*>(d + o_vals);
    A.ranked = reinterpret_cast<double*>(d + o_ranked);
    A.rank_count = reinterpret_cast<int32_t*>(d + o_rank);
    A.better_count = reinterpret_cast<int32_t*>(d + o_better);
    for (int k = 1; k <= dcs::SCORE_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    // the summary is dcm::market_summary on the stored values: K = 5 "markets" of M = R "fixtures"
    dcm::MarketArgs B = sm.over(A.P, A.vals, d);
    HIP_TRY(c, hipMemcpyAsync(d + o_t, teams, R * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d + o_o, opponents, NO * 2, hipMemcpyHostToDevice, s));
    if (conf) {
        HIP_TRY(c, hipMemcpyAsync(d + o_tc, team_conf, R * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(d + o_oc, opponent_conf, NO * 2, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, sm.upload(s, d, quantiles));
    const dim3 block(64 * dcr::RATINGS_WAVES);
    const unsigned tiles = (unsigned)((S + block.x - 1) / block.x);
    rc = summary_chunks(c, s, summary_strides(R, chunk), draws != nullptr, [&](size_t t0, size_t tc) {
        A.t0 = B.n0 = (long long)t0;
        A.tc = B.nc = (long long)tc;
        const dim3 grid((unsigned)tc, tiles);
        if (venue_form) hipLaunchKernelGGL(dcr::ratings_values<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(dcr::ratings_values<false>, grid, block, 0, s, A);
        const hipError_t e = hipGetLastError();
        return e != hipSuccess ? e : summary_launch(venue_form, tc * K, s, B);
    }, [&](size_t t0, size_t tc) {
        return hipMemcpyAsync(draws + t0 * K * S, A.vals, tc * per_team, hipMemcpyDeviceToHost, s);
    });
    if (rc != BPLHIP_OK) return rc;
    // the tiles of 64 draws are dealt over up to about 2048 workgroups (rank_count and better_count are adjacent)
    HIP_TRY(c, hipMemsetAsync(d + o_rank, 0, (o_better - o_rank) + R * R * 4, s));
    const size_t rcols = (R + dcr::RATINGS_WAVES - 1) / dcr::RATINGS_WAVES;
    const size_t slices = std::min((S + 63) / 64, std::max((size_t)1, 2048 / rcols));
    const dim3 rgrid((unsigned)rcols, (unsigned)slices);
    if (venue_form) hipLaunchKernelGGL(dcr::ratings_rank<true>, rgrid, block, 0, s, A);
    else hipLaunchKernelGGL(dcr::ratings_rank<false>, rgrid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sm.read(s, d, mean, sd, quantile));
    HIP_TRY(c, hipMemcpyAsync(rank_count, A.rank_count, R * R * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(better_count, A.better_count, R * R * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    std::copy(n_matches.begin(), n_matches.end(), matches);
    return BPLHIP_OK;
}

// ---- markets of a match in progress (dc_inplay.hip.h); every check before any device call
static int inplay_summary_any(bplhip_ctx* c, const bplhip_fixtures* q, const double* elapsed, int32_t max_goals,
                              int32_t n_markets, const double* weights, int32_t n_quantiles, const double* quantiles,
                              int32_t reweight, const double* log_weights, double* mean, double* sd, double* quantile,
                              double* ess, double* log_evidence, double* draws, double* draw_log_evidence,
                              int64_t workspace_bytes, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "inplay_summary";
    int rc = summary_check_query(c, what, q, max_goals, dcip::INPLAY_MAX_GOALS, n_markets, BPLHIP_MARKET_MAX_MARKETS,
                                 n_quantiles, BPLHIP_INPLAY_MAX_DRAWS);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    if (m < 1 || !q->home_goals || !q->away_goals || !elapsed || !weights || !mean || !sd || !ess || !log_evidence ||
        (n_quantiles > 0 && (!quantiles || !quantile)))
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld below 1 or a null argument", what, (long long)m);
    const size_t M = (size_t)m, S = (size_t)c->pred_S, K = (size_t)n_markets;
    const size_t cells = (size_t)(max_goals + 1) * (size_t)(max_goals + 1);
    Summary sm{K, (size_t)n_quantiles, M};
    std::vector<double> wt;
    rc = summary_grid_weights(c, what, weights, K, cells, dcip::INPLAY_KPASS, &wt);
    if (rc == BPLHIP_OK) rc = summary_check_quantiles(c, what, sm.NQ, quantiles);
    if (rc != BPLHIP_OK) return rc;
    for (size_t i = 0; i < M; ++i) {
        if (!(elapsed[i] >= 0.0 && elapsed[i] < 1.0))
            return fail(c, BPLHIP_EINVAL, "%s: elapsed %g of fixture %zu outside [0, 1)", what, elapsed[i], i);
        if (q->home_goals[i] > max_goals || q->away_goals[i] > max_goals)
            return fail(c, BPLHIP_EINVAL, "%s: score %d-%d of fixture %zu beyond max_goals=%d", what,
                        (int)q->home_goals[i], (int)q->away_goals[i], i, max_goals);
        if (elapsed[i] == 0.0 && (q->home_goals[i] != 0 || q->away_goals[i] != 0))
            return fail(c, BPLHIP_EINVAL, "%s: score %d-%d of fixture %zu at elapsed = 0", what, (int)q->home_goals[i],
                        (int)q->away_goals[i], i);
    }
    if (log_weights)
        for (size_t i = 0; i < S; ++i)
            if (!std::isfinite(log_weights[i]))
                return fail(c, BPLHIP_EINVAL, "%s: log weight %zu is not finite", what, i);
    size_t chunk;   // (the values and the evidence; nc K workgroups)
    rc = summary_chunk(c, what, workspace_bytes, BPLHIP_MARKET_WORKSPACE_BYTES, (K + 1) * S * 8, M, "fixture", &chunk);
    if (rc != BPLHIP_OK) return rc;
    chunk = std::min(chunk, (size_t)0x7FFFFFFF / K);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = loglik_team_major(c, s);
    if (rc != BPLHIP_OK) return rc;
    Carver cv;
    const size_t o_w = cv.take(wt.size() * 8);
    sm.take_levels(cv);
    const size_t o_t = cv.take(M * 8), o_lw = cv.take(log_weights ? S * 8 : 0);
    sm.take_stats(cv);
    const size_t o_ess = cv.take(M * 8), o_ev = cv.take(M * 8), o_vals = cv.take(chunk * K * S * 8),
                 o_lev = cv.take(chunk * S * 8);
    dcip::InplayArgs A{};
    char* d;
    rc = stage_queries(c, c->dp_inplay, s, q, true, cv.total, &A.Q, &d);
    if (rc != BPLHIP_OK) return rc;
    A.P = posterior_view(c, true);
    A.G = max_goals;
    A.reweight = reweight != 0;
    A.w = reinterpret_cast<const double*>(d + o_w);
    A.t = reinterpret_cast<const double*>(d + o_t);
    A.lw = log_weights ? reinterpret_cast<const double*>(d + o_lw) : nullptr;
    A.ess = reinterpret_cast<double*>(d + o_ess);
    A.logev = reinterpret_cast<double*>(d + o_ev);
    A.vals = reinterpret_cast<double*>(d + o_vals);
    A.lev = reinterpret_cast<double*>(d + o_lev);
    sm.point(A, d);
    for (int k = 1; k <= dcip::INPLAY_MAX_GOALS; ++k) A.rk[k] = 1.0 / (double)k;
    for (int k = 0; k <= dcip::INPLAY_MAX_GOALS; ++k) A.lgf[k] = std::lgamma((double)k + 1.0);
    HIP_TRY(c, hipMemcpyAsync(d + o_w, wt.data(), wt.size() * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, sm.upload(s, d, quantiles));
    HIP_TRY(c, hipMemcpyAsync(d + o_t, elapsed, M * 8, hipMemcpyHostToDevice, s));
    if (log_weights) HIP_TRY(c, hipMemcpyAsync(d + o_lw, log_weights, S * 8, hipMemcpyHostToDevice, s));
    // (a quantile is stored by the one thread that holds its crossing: NaN where the weights leave none)
    if (sm.NQ) HIP_TRY(c, hipMemsetAsync(A.quant, 0xFF, K * sm.NQ * M * 8, s));
    const size_t lds = dcip::inplay_summary_lds_bytes((int)S);
    if (!c->inplay_attr_set) {
        const int cap = (int)dcip::inplay_summary_lds_bytes(dcip::INPLAY_MAX_DRAWS);
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcip::inplay_summary<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcip::inplay_summary<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, cap));
        c->inplay_attr_set = true;
    }
    const dim3 block(dcip::INPLAY_THREADS);
    const unsigned tiles = (unsigned)((S + block.x - 1) / block.x), passes = (unsigned)(wt.size() / (cells * dcip::INPLAY_KPASS));
    // the summary kernel is in-play's own (weighted draws): one workgroup per (fixture, market)
    rc = summary_chunks(c, s, summary_strides(M, chunk), draws || draw_log_evidence, [&](size_t n0, size_t nc) {
        A.n0 = (long long)n0;
        A.nc = (long long)nc;
        const dim3 grid((unsigned)nc, tiles, passes), sgrid((unsigned)(nc * K));
        if (venue) hipLaunchKernelGGL(dcip::inplay_values<true>, grid, block, 0, s, A);
        else hipLaunchKernelGGL(dcip::inplay_values<false>, grid, block, 0, s, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (venue) hipLaunchKernelGGL(dcip::inplay_summary<true>, sgrid, block, lds, s, A);
        else hipLaunchKernelGGL(dcip::inplay_summary<false>, sgrid, block, lds, s, A);
        return hipGetLastError();
    }, [&](size_t n0, size_t nc) {
        hipError_t e = draws ? hipMemcpyAsync(draws + n0 * K * S, A.vals, nc * K * S * 8, hipMemcpyDeviceToHost, s) : hipSuccess;
        if (e == hipSuccess && draw_log_evidence)
            e = hipMemcpyAsync(draw_log_evidence + n0 * S, A.lev, nc * S * 8, hipMemcpyDeviceToHost, s);
        return e;
    });
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, sm.read(s, d, mean, sd, quantile));
    HIP_TRY(c, hipMemcpyAsync(ess, A.ess, M * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(log_evidence, A.logev, M * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- MCMC convergence diagnostics (dc_diagnostics.hip.h); needs no posterior; every check before any device call
static int mcmc_diagnostics_any(bplhip_ctx* c, int32_t n_chains, int32_t n_draws, int64_t n_quantities,
                                const double* values, int32_t n_quantiles, const double* quantiles,
                                int64_t workspace_bytes, double* mean, double* sd, double* rhat, double* ess_bulk,
                                double* ess_tail, double* ess_mean, double* mcse_mean, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "mcmc_diagnostics";
    if (n_chains < 1 || n_chains > BPLHIP_DIAG_MAX_CHAINS)
        return fail(c, BPLHIP_EINVAL, "%s: n_chains=%d out of range [1,%d]", what, n_chains, BPLHIP_DIAG_MAX_CHAINS);
    if (n_draws < 8) return fail(c, BPLHIP_EINVAL, "%s: n_draws=%d below 8", what, n_draws);
    const int64_t split = 2 * (int64_t)n_chains * (n_draws / 2);
    if (split > BPLHIP_DIAG_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: %lld split draws, at most %d", what, (long long)split, BPLHIP_DIAG_MAX_DRAWS);
    if (n_quantities < 1 || n_quantities > INT32_MAX)
        return fail(c, BPLHIP_EINVAL, "%s: n_quantities=%lld out of range [1,2^31)", what, (long long)n_quantities);
    if (n_quantiles < 0 || n_quantiles > BPLHIP_DIAG_MAX_QUANTILES)
        return fail(c, BPLHIP_EINVAL, "%s: n_quantiles=%d out of range [0,%d]", what, n_quantiles,
                    BPLHIP_DIAG_MAX_QUANTILES);
    if (!values || !mean || !sd || !rhat || !ess_bulk || !ess_tail || !ess_mean || !mcse_mean ||
        (n_quantiles > 0 && !quantiles))
        return fail(c, BPLHIP_EINVAL, "%s: a null argument", what);
    for (int i = 0; i < n_quantiles; ++i)
        if (!(quantiles[i] > 0.0 && quantiles[i] < 1.0))
            return fail(c, BPLHIP_EINVAL, "%s: quantile %g outside (0, 1)", what, quantiles[i]);
    const int S = (int)split;
    const size_t Q = (size_t)n_quantities, CN = (size_t)n_chains * (size_t)n_draws, NQ = (size_t)n_quantiles;
    const size_t per_quantity = dcg::diag_workspace_per_quantity(S, n_quantiles);
    const size_t ws = workspace_bytes == 0 ? (size_t)BPLHIP_DIAG_WORKSPACE_BYTES : (size_t)workspace_bytes;
    if (workspace_bytes < 0 || ws < per_quantity)
        return fail(c, BPLHIP_EINVAL, "%s: workspace_bytes=%lld holds no quantity (%zu bytes each)", what,
                    (long long)workspace_bytes, per_quantity);
    const size_t chunk = std::min(std::min(Q, ws / per_quantity), (size_t)1 << 20);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    Carver cv;
    const size_t o_in = cv.take(CN * Q * 8), o_t = cv.take(CN * Q * 8), o_q = cv.take(NQ * 8);
    size_t o_out[7];
    for (size_t& o : o_out) o = cv.take(Q * 8);
    HIP_TRY(c, c->dp_diag.ensure(cv.total));
    const bool in_lds = S <= dcg::DIAG_LDS_DRAWS;
    Carver cw;
    const size_t w_zb = cw.take(chunk * S * 8), w_zf = cw.take(chunk * S * 8),
                 w_key = cw.take(in_lds ? 0 : chunk * S * 8), w_idx = cw.take(in_lds ? 0 : chunk * S * 4),
                 w_qv = cw.take(chunk * std::max(NQ, (size_t)1) * 8), w_flag = cw.take(chunk * 4);
    HIP_TRY(c, c->dp_diag_ws.ensure(cw.total));
    char* base = c->dp_diag.as<char>();
    char* wb = c->dp_diag_ws.as<char>();
    HIP_TRY(c, hipMemcpyAsync(base + o_in, values, CN * Q * 8, hipMemcpyHostToDevice, s));
    if (NQ) HIP_TRY(c, hipMemcpyAsync(base + o_q, quantiles, NQ * 8, hipMemcpyHostToDevice, s));
    {
        const dim3 grid((unsigned)((Q + 31) / 32), (unsigned)((CN + 31) / 32)), block(256);
        hipLaunchKernelGGL(dcl::transpose_f64, grid, block, 0, s, reinterpret_cast<const double*>(base + o_in),
                           reinterpret_cast<double*>(base + o_t), (int)CN, (int)Q);
        HIP_TRY(c, hipGetLastError());
    }
    dcg::DiagArgs A{};
    A.xt = reinterpret_cast<const double*>(base + o_t);
    A.C = n_chains;
    A.N = n_draws;
    A.n = n_draws / 2;
    A.M = 2 * n_chains;
    A.S = S;
    A.CN = (int)CN;
    A.NQ = n_quantiles;
    A.q = reinterpret_cast<const double*>(base + o_q);
    A.zb = reinterpret_cast<double*>(wb + w_zb);
    A.zf = reinterpret_cast<double*>(wb + w_zf);
    A.gkey = reinterpret_cast<unsigned long long*>(wb + w_key);
    A.gidx = reinterpret_cast<uint16_t*>(wb + w_idx);
    A.qv = reinterpret_cast<double*>(wb + w_qv);
    A.flag = reinterpret_cast<int32_t*>(wb + w_flag);
    double** outs[7] = {&A.mean, &A.sd, &A.rhat, &A.ess_bulk, &A.ess_tail, &A.ess_mean, &A.mcse_mean};
    for (int i = 0; i < 7; ++i) *outs[i] = reinterpret_cast<double*>(base + o_out[i]);
    const size_t lds = dcg::diag_rank_lds_bytes(S);
    if (!c->diag_attr_set) {
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcg::diag_rank),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)dcg::diag_rank_lds_bytes(dcg::DIAG_LDS_DRAWS)));
        c->diag_attr_set = true;
    }
    for (size_t q0 = 0; q0 < Q; q0 += chunk) {
        const size_t qc = std::min(chunk, Q - q0);
        A.q0 = (long long)q0;
        A.qc = (long long)qc;
        hipLaunchKernelGGL(dcg::diag_rank, dim3((unsigned)qc), dim3(dcg::DIAG_THREADS), lds, s, A);
        HIP_TRY(c, hipGetLastError());
        const dim3 egrid((unsigned)((qc * dcg::DIAG_SERIES + dcg::DIAG_WAVES - 1) / dcg::DIAG_WAVES));
        hipLaunchKernelGGL(dcg::diag_ess, egrid, dim3(dcg::DIAG_THREADS), 0, s, A);
        HIP_TRY(c, hipGetLastError());
    }
    double* host[7] = {mean, sd, rhat, ess_bulk, ess_tail, ess_mean, mcse_mean};
    for (int i = 0; i < 7; ++i) HIP_TRY(c, hipMemcpyAsync(host[i], base + o_out[i], Q * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- weighted shift of posterior quantities (dc_sensitivity.hip.h); needs no posterior; every check before any
// device call.  One stream: the PSIS of the ratio rows, the transpose of the draws, shift_summary chunk by chunk
static int weighted_shift_any(bplhip_ctx* c, int32_t n_draws, int64_t n_quantities, const double* values,
                              int32_t n_rows, const double* log_ratios, double r_eff, int64_t workspace_bytes,
                              double* log_weights, double* pareto_k, double* ess, int32_t* tail_len, double* cjs_sq,
                              double* mean, double* sd, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "weighted_shift";
    if (n_rows < 1 || n_rows > BPLHIP_SHIFT_MAX_ROWS)
        return fail(c, BPLHIP_EINVAL, "%s: n_rows=%d out of range [1,%d]", what, n_rows, BPLHIP_SHIFT_MAX_ROWS);
    if (n_draws < 8 || n_draws > BPLHIP_DIAG_MAX_DRAWS)
        return fail(c, BPLHIP_EINVAL, "%s: n_draws=%d out of range [8,%d]", what, n_draws, BPLHIP_DIAG_MAX_DRAWS);
    if (n_quantities < 1 || n_quantities > INT32_MAX)
        return fail(c, BPLHIP_EINVAL, "%s: n_quantities=%lld out of range [1,2^31)", what, (long long)n_quantities);
    if (!values || !log_ratios || !log_weights || !pareto_k || !ess || !tail_len || !cjs_sq || !mean || !sd)
        return fail(c, BPLHIP_EINVAL, "%s: a null argument", what);
    if (!(std::isfinite(r_eff) && r_eff > 0.0))
        return fail(c, BPLHIP_EINVAL, "%s: r_eff = %g must be finite and > 0", what, r_eff);
    const long long tail_m = loglik_tail_size(n_draws, r_eff);
    if (tail_m > BPLHIP_LOGLIK_MAX_TAIL)
        return fail(c, BPLHIP_EINVAL, "%s: the PSIS tail of %lld draws (S = %d, r_eff = %g) exceeds %d", what, tail_m,
                    n_draws, r_eff, BPLHIP_LOGLIK_MAX_TAIL);
    const size_t R = (size_t)n_rows, S = (size_t)n_draws, Q = (size_t)n_quantities;
    for (size_t i = 0; i < R * S; ++i)
        if (!std::isfinite(log_ratios[i]))
            return fail(c, BPLHIP_EINVAL, "%s: log ratio %zu is not finite", what, i);
    const size_t per_quantity = dcps::shift_workspace_per_quantity(n_draws);
    const size_t ws = workspace_bytes == 0 ? (size_t)BPLHIP_SHIFT_WORKSPACE_BYTES : (size_t)workspace_bytes;
    if (workspace_bytes < 0 || ws < per_quantity)
        return fail(c, BPLHIP_EINVAL, "%s: workspace_bytes=%lld holds no quantity (%zu bytes each)", what,
                    (long long)workspace_bytes, per_quantity);
    const size_t chunk = std::min(std::min(Q, per_quantity ? ws / per_quantity : Q), (size_t)1 << 20);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PsisCarve pc;
    Carver& cv = pc.carve(R, S);
    const size_t o_in = cv.take(S * Q * 8), o_x = cv.take(S * Q * 8);
    size_t o_out[3];
    for (size_t& o : o_out) o = cv.take(R * Q * 8);
    HIP_TRY(c, c->dp_shift.ensure(cv.total));
    const bool in_lds = n_draws <= dcps::SHIFT_LDS_DRAWS;
    Carver cw;
    const size_t w_key = cw.take(in_lds ? 0 : chunk * S * 8), w_idx = cw.take(in_lds ? 0 : chunk * S * 4);
    HIP_TRY(c, c->dp_shift_ws.ensure(cw.total));
    char* base = c->dp_shift.as<char>();
    char* wb = c->dp_shift_ws.as<char>();
    dcu::PsisArgs P{};
    HIP_TRY(c, psis_rows_launch(pc, base, R, n_draws, tail_m, log_ratios, s, &P));
    HIP_TRY(c, hipMemcpyAsync(base + o_in, values, S * Q * 8, hipMemcpyHostToDevice, s));
    {
        const dim3 grid((unsigned)((Q + 31) / 32), (unsigned)((S + 31) / 32)), block(256);
        hipLaunchKernelGGL(dcl::transpose_f64, grid, block, 0, s, reinterpret_cast<const double*>(base + o_in),
                           reinterpret_cast<double*>(base + o_x), (int)S, (int)Q);
        HIP_TRY(c, hipGetLastError());
    }
    dcps::ShiftArgs A{};
    A.xt = reinterpret_cast<const double*>(base + o_x);
    A.lw = P.lw;
    A.S = n_draws;
    A.R = n_rows;
    A.Q = (long long)Q;
    A.gkey = reinterpret_cast<unsigned long long*>(wb + w_key);
    A.gidx = reinterpret_cast<uint16_t*>(wb + w_idx);
    A.cjs_sq = reinterpret_cast<double*>(base + o_out[0]);
    A.mean = reinterpret_cast<double*>(base + o_out[1]);
    A.sd = reinterpret_cast<double*>(base + o_out[2]);
    const size_t lds = dcps::shift_summary_lds_bytes(n_draws);
    if (!c->shift_attr_set) {
        HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(dcps::shift_summary),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)dcps::shift_summary_lds_bytes(dcps::SHIFT_LDS_DRAWS)));
        c->shift_attr_set = true;
    }
    for (size_t q0 = 0; q0 < Q; q0 += chunk) {
        const size_t qc = std::min(chunk, Q - q0);
        A.q0 = (long long)q0;
        A.qc = (long long)qc;
        hipLaunchKernelGGL(dcps::shift_summary, dim3((unsigned)qc), dim3(dcps::SHIFT_THREADS), lds, s, A);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(log_weights, P.lw, R * S * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(pareto_k, P.pareto_k, R * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(ess, P.ess, R * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(tail_len, P.tail_len, R * 4, hipMemcpyDeviceToHost, s));
    double* host[3] = {cjs_sq, mean, sd};
    for (int i = 0; i < 3; ++i) HIP_TRY(c, hipMemcpyAsync(host[i], base + o_out[i], R * Q * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- posterior predictive replications (dc_ppc.hip.h); every check before any device call
static int ppc_any(bplhip_ctx* c, const bplhip_fixtures* q, const uint16_t* home_slot, const uint16_t* away_slot,
                   const uint32_t* fixture_id, int32_t n_slots, int32_t max_goals, int64_t n_reps, uint32_t key_hi,
                   uint32_t key_lo, uint32_t* score_counts, uint32_t* outcome_counts, int64_t* goal_sums,
                   uint32_t* team_counts, uint8_t* home_goals, uint8_t* away_goals, void* stream) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "ppc";
    int rc = predict_check_query(c, what, q);
    if (rc != BPLHIP_OK) return rc;
    const int64_t m = q->m;
    const bool venue = q->venue != 0;
    const bool conf = venue && q->home_conf;
    if (m < 1 || m > BPLHIP_PPC_MAX_FIXTURES || !home_slot || !away_slot)
        return fail(c, BPLHIP_EINVAL, "%s: m=%lld out of range [1,%d] or null slots", what, (long long)m,
                    BPLHIP_PPC_MAX_FIXTURES);
    if (n_slots < 1 || n_slots > BPLHIP_PPC_MAX_TEAMS)
        return fail(c, BPLHIP_EINVAL, "%s: n_slots=%d out of range [1,%d]", what, n_slots, BPLHIP_PPC_MAX_TEAMS);
    if (max_goals < 1 || max_goals > BPLHIP_PPC_MAX_GOALS)
        return fail(c, BPLHIP_EINVAL, "%s: max_goals=%d out of range [1,%d]", what, max_goals, BPLHIP_PPC_MAX_GOALS);
    if (n_reps < 1 || n_reps > BPLHIP_PPC_MAX_REPLICATIONS || n_reps * n_slots > BPLHIP_PPC_MAX_TEAM_CELLS)
        return fail(c, BPLHIP_EINVAL, "%s: n_reps=%lld out of range [1,%d] or n_reps x n_slots over %d", what,
                    (long long)n_reps, BPLHIP_PPC_MAX_REPLICATIONS, BPLHIP_PPC_MAX_TEAM_CELLS);
    if (!score_counts || !outcome_counts || !goal_sums || !team_counts)
        return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    if ((home_goals != nullptr) != (away_goals != nullptr))
        return fail(c, BPLHIP_EINVAL, "%s: home_goals and away_goals go together", what);
    if (home_goals && n_reps * m > BPLHIP_PPC_MAX_SCORE_CELLS)
        return fail(c, BPLHIP_EINVAL, "%s: n_reps x m = %lld replicated scorelines, at most %lld", what,
                    (long long)(n_reps * m), (long long)BPLHIP_PPC_MAX_SCORE_CELLS);
    const size_t M = (size_t)m, R = (size_t)n_reps, k = (size_t)n_slots, nb = (size_t)(max_goals + 1) * (max_goals + 1);
    std::vector<uint32_t> pk((conf ? 4 : 3) * M);   // the columns in pairs, one u32 per fixture
    for (size_t i = 0; i < M; ++i) {
        if (home_slot[i] >= n_slots || away_slot[i] >= n_slots)
            return fail(c, BPLHIP_EINVAL, "%s: team slot out of range at %zu", what, i);
        pk[i] = (uint32_t)q->home_idx[i] | ((uint32_t)q->away_idx[i] << 16);
        pk[M + i] = (uint32_t)home_slot[i] | ((uint32_t)away_slot[i] << 16);
        pk[2 * M + i] = fixture_id ? fixture_id[i] : (uint32_t)i;
        if (conf) pk[3 * M + i] = (uint32_t)q->home_conf[i] | ((uint32_t)q->away_conf[i] << 16);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one buffer: queries u32 [3 or 4, m], neutral u8 [m]; then the outputs score u32 [R, nb], outcome u32
    // [R, 3], sums i64 [R, 5], team u32 [R, k, 4], and the scorelines asked for
    Carver cv;
    cv.take(pk.size() * 4);
    const size_t o_nv = cv.take(M), o_score = cv.take(R * nb * 4), o_out = cv.take(R * 3 * 4), o_sums = cv.take(R * 5 * 8),
                 o_team = cv.take(R * k * 16), o_hg = cv.take(home_goals ? R * M : 0), o_ag = cv.take(home_goals ? R * M : 0);
    HIP_TRY(c, c->dp_ppc.ensure(cv.total));
    char* base = c->dp_ppc.as<char>();
    HIP_TRY(c, hipMemcpyAsync(base, pk.data(), pk.size() * 4, hipMemcpyHostToDevice, s));
    if (venue) HIP_TRY(c, hipMemcpyAsync(base + o_nv, q->neutral_venue, M, hipMemcpyHostToDevice, s));
    const uint32_t* dq = reinterpret_cast<const uint32_t*>(base);
    dcppc::PpcArgs A{};
    A.P = posterior_view(c, false);
    A.m = (int)m;
    A.k = n_slots;
    A.G = max_goals;
    A.key_hi = key_hi;
    A.key_lo = key_lo;
    A.fix = dq;
    A.slot = dq + M;
    A.fid = dq + 2 * M;
    A.neutral = reinterpret_cast<const uint8_t*>(base + o_nv);
    A.conf_idx = A.P.C ? dq + 3 * M : nullptr;
    A.score = reinterpret_cast<uint32_t*>(base + o_score);
    A.outcome = reinterpret_cast<uint32_t*>(base + o_out);
    A.sums = reinterpret_cast<long long*>(base + o_sums);
    A.team = reinterpret_cast<uint32_t*>(base + o_team);
    A.home_goals = home_goals ? reinterpret_cast<uint8_t*>(base + o_hg) : nullptr;
    A.away_goals = home_goals ? reinterpret_cast<uint8_t*>(base + o_ag) : nullptr;
    // one workgroup per replication: every row is written whole, nothing to zero
    const dim3 grid((unsigned)R), block(64 * dcppc::PPC_WAVES);
    if (venue) hipLaunchKernelGGL(dcppc::dc_ppc<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(dcppc::dc_ppc<false>, grid, block, 0, s, A);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(score_counts, A.score, R * nb * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(outcome_counts, A.outcome, R * 3 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(goal_sums, A.sums, R * 5 * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(team_counts, A.team, R * k * 16, hipMemcpyDeviceToHost, s));
    if (home_goals) {
        HIP_TRY(c, hipMemcpyAsync(home_goals, A.home_goals, R * M, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(away_goals, A.away_goals, R * M, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- what simulate_season and simulate_tournament share (`what` names the entry point in the messages)
static int sim_check_run(bplhip_ctx* c, const char* what, int64_t n_sims, int32_t win_points, int32_t draw_points,
                         int32_t loss_points) {
    if (n_sims < 1 || n_sims > 0x7FFFFFFF)
        return fail(c, BPLHIP_EINVAL, "%s: n_sims=%lld out of range [1,2^31)", what, (long long)n_sims);
    const int32_t pts[3] = {win_points, draw_points, loss_points};
    for (int32_t p : pts)
        if (p < 0 || p > BPLHIP_SEASON_MAX_MATCH_POINTS) return fail(c, BPLHIP_EINVAL, "%s: bad points", what);
    return BPLHIP_OK;
}
// one wave per simulation, at most blocks_per_cu workgroups per CU (grid-stride beyond)
static unsigned sim_grid(const bplhip_ctx* c, int64_t n_sims, int waves, int blocks_per_cu) {
    const long long want = (n_sims + waves - 1) / waves, cap = (long long)blocks_per_cu * c->n_cu;
    return (unsigned)std::min(want, cap);
}

// ---- head-to-head tie-breaks (dc_h2h.hip.h): what the three *_h2h entry points add to their counterparts
struct H2HRequest {
    bool on = false;
    const uint32_t* pair_init = nullptr;   // HOST u32 [n, n] or null
};
// every half of a pair record stays in 16 bits: what was played plus the remaining meetings (`meet` [n, n],
// symmetric) at the largest value a match can add; `*any` tells whether pair_init has a non-zero entry to upload
static int h2h_check(bplhip_ctx* c, const char* what, int n, const std::vector<int64_t>& meet, int32_t win_points,
                     int32_t draw_points, int32_t loss_points, const uint32_t* pair_init, bool* any) {
    const int64_t top = std::max({win_points, draw_points, loss_points});
    *any = false;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) {
            if (i == k) continue;
            const uint32_t w = pair_init ? pair_init[(size_t)i * n + k] : 0u;
            const int64_t m = meet[(size_t)i * n + k];
            if ((int64_t)(w >> 16) + m * top > (int64_t)dch::H2H_HALF ||
                (int64_t)(w & dch::H2H_HALF) + m * dch::H2H_MAX_GOALS > (int64_t)dch::H2H_HALF)
                return fail(c, BPLHIP_EINVAL, "%s: the pair record of slots %d and %d can pass 16 bits", what, i, k);
            *any = *any || w != 0u;
        }
    return BPLHIP_OK;
}
// the remaining meetings of every ordered pair of slots, [n, n] (for h2h_check); `fix`: slot | slot << 8
static std::vector<int64_t> pair_meetings(const std::vector<uint16_t>& fix, int n) {
    std::vector<int64_t> meet((size_t)n * n, 0);
    for (const uint16_t f : fix) {
        const size_t p = f & 0xFFu, q = f >> 8;
        ++meet[p * n + q];
        ++meet[q * n + p];
    }
    return meet;
}
// the launch shape of a table simulator over n slots: the overall order with the kernel's own waves per
// workgroup and workgroups per CU and no dynamic LDS, the head-to-head order with dch::waves_for(n) waves and
// their pair matrices
struct SimLaunch {
    dim3 grid, block;
    size_t lds;
};
static SimLaunch sim_launch(const bplhip_ctx* c, const H2HRequest& h2h, int n, int64_t n_sims, int waves, int blocks_per_cu) {
    if (h2h.on) {
        waves = dch::waves_for(n);
        blocks_per_cu = dch::H2H_BLOCKS_PER_CU;
    }
    return {dim3(sim_grid(c, n_sims, waves, blocks_per_cu)), dim3(64 * waves), h2h.on ? dch::lds_bytes(n) : 0};
}
// the pair matrix goes last into a call's carved buffer, u32 [n, n], and only when pair_init has an entry to
// upload (h2h_check's `any`): takes its place, sizes `buf` for the whole carve and uploads
static int pair_place(bplhip_ctx* c, Carver& cv, DevBuf& buf, const H2HRequest& h2h, bool any, int n, hipStream_t s,
                      dch::PairArgs* H) {
    const size_t bytes = (size_t)n * n * 4, at = cv.take(any ? bytes : 0);
    HIP_TRY(c, buf.ensure(cv.total));
    if (any) HIP_TRY(c, hipMemcpyAsync(buf.as<char>() + at, h2h.pair_init, bytes, hipMemcpyHostToDevice, s));
    *H = {any ? reinterpret_cast<const uint32_t*>(buf.as<char>() + at) : nullptr, dch::pitch_for(n)};
    return BPLHIP_OK;
}

// ---- the season family: simulate_season (and _h2h, _playoff, _live), match_leverage (and _h2h), season_points and
// season_trajectory.  SeasonCall is what all eight exported symbols take first, as their wrappers hand it on
struct SeasonCall {
    int64_t n_fixtures;
    const uint16_t *home_idx, *away_idx;              // HOST u16 [n_fixtures] model indices
    int32_t n_table;
    const uint16_t* table_idx;                        // HOST u16 [n_table] model indices in slot order
    const int32_t *init_points, *init_gf, *init_ga;   // HOST i32 [n_table]
    int32_t win, draw, loss;
    int64_t n_sims;
    uint32_t key_hi, key_lo;
    void* stream;
    H2HRequest h2h;
};
// every check of bpl/base.py's _season_inputs repeated on the host, then the fixtures, their slots and the current
// table as the kernels read them
struct SeasonSetup {
    std::vector<uint32_t> fix;        // [nf]: home | away << 16 (model indices)
    std::vector<uint16_t> fix_slot;   // [nf]: home slot | away slot << 8
    std::vector<int32_t> init;        // [3, n]: points, GF, GA
};
static int season_setup(bplhip_ctx* c, const char* what, const SeasonCall& q, int64_t max_fixtures, SeasonSetup* out) {
    if (c->pred_S == 0) return fail(c, BPLHIP_ESTATE, "%s: no posterior set", what);
    if (c->pred_venue)
        return fail(c, BPLHIP_ESTATE, "%s: the posterior was set with predict_set_posterior_venue", what);
    if (q.n_fixtures < 0 || q.n_fixtures > max_fixtures || (q.n_fixtures > 0 && (!q.home_idx || !q.away_idx)))
        return fail(c, BPLHIP_EINVAL, "%s: bad fixtures (n_fixtures=%lld)", what, (long long)q.n_fixtures);
    if (q.n_table < 1 || q.n_table > dcs::SEASON_MAX_TEAMS || !q.table_idx || !q.init_points || !q.init_gf || !q.init_ga)
        return fail(c, BPLHIP_EINVAL, "%s: n_table=%d out of range [1,%d] or null table", what, q.n_table,
                    dcs::SEASON_MAX_TEAMS);
    int rc = sim_check_run(c, what, q.n_sims, q.win, q.draw, q.loss);
    if (rc != BPLHIP_OK) return rc;
    std::vector<int> slot_of(c->pred_T, -1);
    for (int i = 0; i < q.n_table; ++i) {
        if (q.table_idx[i] >= c->pred_T || slot_of[q.table_idx[i]] >= 0)
            return fail(c, BPLHIP_EINVAL, "%s: table team %d out of range or repeated", what, (int)q.table_idx[i]);
        slot_of[q.table_idx[i]] = i;
        for (const int32_t v : {q.init_points[i], q.init_gf[i], q.init_ga[i]})
            if (v < 0 || v > BPLHIP_SEASON_MAX_TABLE_VALUE)
                return fail(c, BPLHIP_EINVAL, "%s: table entry of slot %d out of range [0,%d]", what, i,
                            BPLHIP_SEASON_MAX_TABLE_VALUE);
    }
    const size_t nf = (size_t)q.n_fixtures, n = (size_t)q.n_table;
    out->fix.resize(nf);
    out->fix_slot.resize(nf);
    for (size_t f = 0; f < nf; ++f) {
        const int h = q.home_idx[f], a = q.away_idx[f];
        if (h >= c->pred_T || a >= c->pred_T || slot_of[h] < 0 || slot_of[a] < 0)
            return fail(c, BPLHIP_EINVAL, "%s: fixture %zu has a team outside the table", what, f);
        if (h == a) return fail(c, BPLHIP_EINVAL, "%s: fixture %zu is a team playing itself", what, f);
        out->fix[f] = (uint32_t)h | ((uint32_t)a << 16);
        out->fix_slot[f] = (uint16_t)(slot_of[h] | (slot_of[a] << 8));
    }
    out->init.resize(3 * n);
    std::copy(q.init_points, q.init_points + n, out->init.begin());
    std::copy(q.init_gf, q.init_gf + n, out->init.begin() + n);
    std::copy(q.init_ga, q.init_ga + n, out->init.begin() + 2 * n);
    return BPLHIP_OK;
}

// what every entry of the family does between its own checks and its own kernels.  season_begin is an entry's
// last check (the pair records) and selects the device; season_stage follows the entry's carve of its workspace
struct SeasonStage {
    hipStream_t s = nullptr;
    bool pair_any = false;   // pair_init has an entry to upload
    dch::PairArgs H{};
    char* base = nullptr;    // the carved workspace
};
static int season_begin(bplhip_ctx* c, const char* what, const SeasonCall& q, const SeasonSetup& in, SeasonStage* st) {
    if (q.h2h.on) {
        const int rc = h2h_check(c, what, q.n_table, pair_meetings(in.fix_slot, q.n_table), q.win, q.draw, q.loss,
                                 q.h2h.pair_init, &st->pair_any);
        if (rc != BPLHIP_OK) return rc;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    st->s = static_cast<hipStream_t>(q.stream);
    return BPLHIP_OK;
}
// the sections every workspace of the family has: the counts zeroed together end where the fixtures begin
struct SeasonSections {
    size_t zero_from, o_fix, o_slot, o_init;
};
// places the pair matrix after the entry's sections and sizes `buf`, zeroes the counts, uploads the fixtures (the
// entry's own arrays: season_trajectory's are permuted), their slots and the table, and fills the fields that the
// argument records of the family's kernels have in common
template <class Args>
static int season_stage(bplhip_ctx* c, const SeasonCall& q, SeasonStage& st, Carver& cv, DevBuf& buf,
                        const SeasonSections& at, const std::vector<uint32_t>& fix, const std::vector<uint16_t>& fix_slot,
                        const std::vector<int32_t>& init, Args& A) {
    const int rc = pair_place(c, cv, buf, q.h2h, st.pair_any, q.n_table, st.s, &st.H);
    if (rc != BPLHIP_OK) return rc;
    const auto [zero_from, o_fix, o_slot, o_init] = at;
    const size_t nf = fix.size();
    char* base = st.base = buf.as<char>();
    hipStream_t s = st.s;
    HIP_TRY(c, hipMemsetAsync(base + zero_from, 0, o_fix - zero_from, s));
    if (nf) {
        HIP_TRY(c, hipMemcpyAsync(base + o_fix, fix.data(), nf * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(base + o_slot, fix_slot.data(), nf * 2, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, hipMemcpyAsync(base + o_init, init.data(), init.size() * 4, hipMemcpyHostToDevice, s));
    A.S = c->pred_S;
    A.T = c->pred_T;
    A.n = q.n_table;
    A.nf = (int)nf;
    A.key_hi = q.key_hi;
    A.key_lo = q.key_lo;
    A.win = q.win;
    A.draw = q.draw;
    A.loss = q.loss;
    A.attack = c->dp_tab[PT_ATT].as<const double>();
    A.defence = c->dp_tab[PT_DEF].as<const double>();
    A.home_adv = c->dp_tab[PT_HA].as<const double>();
    A.ha_stride = c->pred_ha_stride;
    A.corr = c->dp_corr.as<const double>();
    A.fix = reinterpret_cast<const uint32_t*>(base + o_fix);
    A.fix_slot = reinterpret_cast<const uint16_t*>(base + o_slot);
    A.init = reinterpret_cast<const int32_t*>(base + o_init);
    return BPLHIP_OK;
}

// ---- what match_leverage, season_points and season_trajectory share: finishing targets, counted chunk by chunk
struct TargetRequest {
    int32_t n_targets;
    const uint64_t* target_mask;   // HOST u64 [n_targets]: bit p = finishing position p
    int64_t chunk_sims;            // simulations per pass through the workspace, 0 = chunk_for's choice
};
static int targets_check(bplhip_ctx* c, const char* what, int32_t n_table, const TargetRequest& tg) {
    if (tg.n_targets < 1 || tg.n_targets > BPLHIP_LEVERAGE_MAX_TARGETS || !tg.target_mask)
        return fail(c, BPLHIP_EINVAL, "%s: n_targets=%d out of range [1,%d] or null masks", what, tg.n_targets,
                    BPLHIP_LEVERAGE_MAX_TARGETS);
    const uint64_t table_bits = n_table == 64 ? ~0ull : (1ull << n_table) - 1ull;
    for (int k = 0; k < tg.n_targets; ++k)
        if (tg.target_mask[k] == 0 || (tg.target_mask[k] & ~table_bits))
            return fail(c, BPLHIP_EINVAL, "%s: target %d has no position, or one outside the table", what, k);
    if (tg.chunk_sims < 0) return fail(c, BPLHIP_EINVAL, "%s: chunk_sims=%lld is negative", what, (long long)tg.chunk_sims);
    return BPLHIP_OK;
}
// the simulations of one pass: the caller's, or as many records of `record_bytes` as keep the chunk's rows within
// SEASON_WORKSPACE_BYTES (and a chunk's u32 tile counts far from overflow), in whole groups of 64
constexpr size_t SEASON_WORKSPACE_BYTES = (size_t)64 << 20, SEASON_MAX_CHUNK = 1 << 16;
static size_t chunk_for(int64_t chunk_sims, size_t record_bytes, int64_t n_sims) {
    const size_t fit = std::min(SEASON_MAX_CHUNK, SEASON_WORKSPACE_BYTES / record_bytes) & ~(size_t)63;
    const size_t chunk = chunk_sims ? (size_t)chunk_sims : std::max<size_t>(64, fit);
    return std::min(chunk, (size_t)n_sims);
}
template <class Args>
static void target_args(Args& A, const TargetRequest& tg, size_t chunk) {
    A.K = tg.n_targets;
    A.chunk = (int)chunk;
    for (int k = 0; k < tg.n_targets; ++k) A.mask[k] = tg.target_mask[k];
}
// every total of a slot lies on the points axis [points_min, points_min + n_bins): from init + m * least to init + m *
// (most points of a match), m = the slot's remaining matches; `verb`: what the slot does with those totals
static int axis_check(bplhip_ctx* c, const char* what, const char* verb, const SeasonCall& q, const SeasonSetup& in,
                      int64_t least, int32_t points_min, int32_t n_bins) {
    const int64_t most = std::max({q.win, q.draw, q.loss});
    std::vector<int64_t> matches((size_t)q.n_table, 0);
    for (const uint16_t f : in.fix_slot) {
        ++matches[f & 0xFFu];
        ++matches[f >> 8];
    }
    for (size_t t = 0; t < matches.size(); ++t) {
        const int64_t lo = q.init_points[t] + matches[t] * least, hi = q.init_points[t] + matches[t] * most;
        if (lo < (int64_t)points_min || hi >= (int64_t)points_min + n_bins)
            return fail(c, BPLHIP_EINVAL, "%s: slot %zu %s %lld..%lld points, outside [%d,%lld)", what, t, verb,
                        (long long)lo, (long long)hi, points_min, (long long)points_min + n_bins);
    }
    return BPLHIP_OK;
}
// a counting kernel's grid over a chunk of nc simulations: one row of workgroups per counted row, and shares of the
// chunk: enough workgroups to fill the device, each with at least one pass of its threads
static dim3 count_grid(const bplhip_ctx* c, unsigned rows, int nc, int threads) {
    const long long passes = (nc + threads - 1) / threads, fill = (2ll * c->n_cu + rows - 1) / rows;
    return dim3(rows, (unsigned)std::max(1ll, std::min({passes, fill, 65535ll})));
}

// ---- play-offs after the table (dc_playoff.hip.h): what bplhip_simulate_season_playoff adds
struct PlayoffRequest {
    int32_t head_to_head;
    int32_t n_guests;
    const uint16_t* guest_idx;   // HOST u16 [n_guests] model indices, or null with none
    const uint16_t* bracket;     // HOST u16 [2^rounds] codes
    int32_t rounds;
    uint32_t legs_mask, neutral_mask;
    double scale;
    int32_t away_goals;
    const double* strength;      // HOST f64 [n_table + n_guests] or null (all zero)
    uint64_t* stage_counts;      // HOST u64 [n_table + n_guests, rounds + 2]
    uint64_t* decided_counts;    // HOST u64 [rounds, 4]
    uint8_t* sim_stage;          // u8 [n_sims, n_table + n_guests] or null
    uint8_t* sim_decided;        // u8 [n_sims, 2^rounds - 1] or null
};
// every check of bpl/base.py's playoff_inputs repeated; `slot_model`: the model index of every slot
static int playoff_check(bplhip_ctx* c, const PlayoffRequest& po, int32_t n_table, const uint16_t* table_idx,
                         std::vector<uint16_t>* slot_model) {
    const char* what = "simulate_season_playoff";
    if (po.head_to_head != 0 && po.head_to_head != 1) return fail(c, BPLHIP_EINVAL, "%s: head_to_head is 0 / 1", what);
    if (po.rounds < 1 || po.rounds > dck::KNOCKOUT_MAX_ROUNDS || !po.bracket)
        return fail(c, BPLHIP_EINVAL, "%s: the bracket must have 2^R entries, 1 <= R <= %d", what, dck::KNOCKOUT_MAX_ROUNDS);
    if (po.n_guests < 0 || n_table + (int64_t)po.n_guests > dcpo::PLAYOFF_MAX_SLOTS || (po.n_guests > 0 && !po.guest_idx))
        return fail(c, BPLHIP_EINVAL, "%s: n_guests=%d: table rows plus guests number at most %d", what, po.n_guests,
                    dcpo::PLAYOFF_MAX_SLOTS);
    if (po.legs_mask >> po.rounds || po.neutral_mask >> po.rounds)
        return fail(c, BPLHIP_EINVAL, "%s: legs_mask=0x%x or neutral_mask=0x%x has a bit at or above R=%d", what,
                    po.legs_mask, po.neutral_mask, po.rounds);
    if (!(po.scale > 0.0 && po.scale <= 1.0))
        return fail(c, BPLHIP_EINVAL, "%s: extra_time_scale=%g outside (0,1]", what, po.scale);
    if (po.away_goals != 0 && po.away_goals != 1) return fail(c, BPLHIP_EINVAL, "%s: away_goals is 0 / 1", what);
    if (!po.stage_counts || !po.decided_counts) return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    const int n = n_table, g = po.n_guests, nt = n + g, nb = 1 << po.rounds;
    for (int i = 0; po.strength && i < nt; ++i)
        if (!(std::fabs(po.strength[i]) <= BPLHIP_TOURNAMENT_MAX_STRENGTH))
            return fail(c, BPLHIP_EINVAL, "%s: strength of slot %d is not finite or beyond %d", what, i,
                        BPLHIP_TOURNAMENT_MAX_STRENGTH);
    std::vector<char> seen(c->pred_T, 0);
    slot_model->assign(table_idx, table_idx + n);
    for (int i = 0; i < n; ++i) seen[table_idx[i]] = 1;   // (season_setup has checked the table)
    for (int i = 0; i < g; ++i) {
        if (po.guest_idx[i] >= c->pred_T || seen[po.guest_idx[i]])
            return fail(c, BPLHIP_EINVAL, "%s: guest %d out of range, repeated or a row of the table", what,
                        (int)po.guest_idx[i]);
        seen[po.guest_idx[i]] = 1;
        slot_model->push_back(po.guest_idx[i]);
    }
    std::vector<char> used(nt, 0);
    for (int b = 0; b < nb; ++b) {
        const uint16_t code = po.bracket[b];
        if (code == BPLHIP_PLAYOFF_BYE) {
            if ((b & 1) && po.bracket[b - 1] == BPLHIP_PLAYOFF_BYE)
                return fail(c, BPLHIP_EINVAL, "%s: bracket entries %d and %d are both byes", what, b - 1, b);
            continue;
        }
        const int slot = (code & BPLHIP_PLAYOFF_GUEST) ? ((code & 0x7FFF) < g ? n + (code & 0x7FFF) : -1)
                                                       : (code < n ? (int)code : -1);
        if (slot < 0 || used[slot])
            return fail(c, BPLHIP_EINVAL, "%s: bracket entry %d (code 0x%x) out of range or used twice", what, b, (int)code);
        used[slot] = 1;
    }
    return BPLHIP_OK;
}

// ---- simulate_season (dc_season.hip.h), and what it shares with its live form: the outputs, their sections at the
// head of dp_season, the whole of SeasonArgs and the read-back
struct SeasonOut {
    uint64_t* position_counts;          // HOST u64 [n, n]
    int64_t *points_sum, *gd_sum;       // HOST i64 [n]
    int32_t* sim_points;                // i32 [n_sims, n] or null
    uint8_t* sim_position;              // u8 [n_sims, n] or null
    uint8_t *home_goals, *away_goals;   // u8 [n_sims, nf] or null, together
};
static int season_out_check(bplhip_ctx* c, const char* what, const SeasonOut& out) {
    if (!out.position_counts || !out.points_sum || !out.gd_sum) return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    if ((out.home_goals != nullptr) != (out.away_goals != nullptr))
        return fail(c, BPLHIP_EINVAL, "%s: home_goals and away_goals go together", what);
    return BPLHIP_OK;
}
// counts u64 [n, n] at the base, sums u64 [2, n], fixtures u32 [nf], slots u16 [nf], table i32 [3, n], then the
// per-simulation outputs asked for
struct SeasonCarve {
    size_t o_sums, o_fix, o_slot, o_init, o_pts, o_pos, o_hg, o_ag;
};
static SeasonCarve season_carve(Carver& cv, const SeasonOut& out, size_t n, size_t nf, size_t ns) {
    SeasonCarve at;
    cv.take(n * n * 8);
    at.o_sums = cv.take(2 * n * 8);
    at.o_fix = cv.take(nf * 4);
    at.o_slot = cv.take(nf * 2);
    at.o_init = cv.take(3 * n * 4);
    at.o_pts = cv.take(out.sim_points ? ns * n * 4 : 0);
    at.o_pos = cv.take(out.sim_position ? ns * n : 0);
    at.o_hg = cv.take(out.home_goals ? ns * nf : 0);
    at.o_ag = cv.take(out.home_goals ? ns * nf : 0);
    return at;
}
// after the entry's own sections are carved: season_stage into dp_season, then SeasonArgs' outputs
static int season_args(bplhip_ctx* c, const SeasonCall& q, SeasonStage& st, Carver& cv, const SeasonCarve& at,
                       const SeasonSetup& in, const SeasonOut& out, dcs::SeasonArgs& A) {
    const int rc = season_stage(c, q, st, cv, c->dp_season, {0, at.o_fix, at.o_slot, at.o_init}, in.fix, in.fix_slot, in.init, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    A.n_sims = q.n_sims;
    A.counts = reinterpret_cast<unsigned long long*>(base);
    A.sums = reinterpret_cast<unsigned long long*>(base + at.o_sums);
    A.sim_points = out.sim_points ? reinterpret_cast<int32_t*>(base + at.o_pts) : nullptr;
    A.sim_position = out.sim_position ? reinterpret_cast<uint8_t*>(base + at.o_pos) : nullptr;
    A.home_goals = out.home_goals ? reinterpret_cast<uint8_t*>(base + at.o_hg) : nullptr;
    A.away_goals = out.home_goals ? reinterpret_cast<uint8_t*>(base + at.o_ag) : nullptr;
    return BPLHIP_OK;
}
// enqueues the copies of SeasonOut; `sums` [2, n] is the host's landing place, for season_sums once the stream
// has been synchronised
static int season_read(bplhip_ctx* c, const SeasonStage& st, const SeasonCarve& at, const SeasonOut& out, size_t n, size_t nf,
                       size_t ns, std::vector<int64_t>& sums) {
    const char* base = st.base;
    hipStream_t s = st.s;
    sums.resize(2 * n);
    HIP_TRY(c, hipMemcpyAsync(out.position_counts, base, n * n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(sums.data(), base + at.o_sums, 2 * n * 8, hipMemcpyDeviceToHost, s));
    if (out.sim_points) HIP_TRY(c, hipMemcpyAsync(out.sim_points, base + at.o_pts, ns * n * 4, hipMemcpyDeviceToHost, s));
    if (out.sim_position) HIP_TRY(c, hipMemcpyAsync(out.sim_position, base + at.o_pos, ns * n, hipMemcpyDeviceToHost, s));
    if (out.home_goals && nf) {
        HIP_TRY(c, hipMemcpyAsync(out.home_goals, base + at.o_hg, ns * nf, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(out.away_goals, base + at.o_ag, ns * nf, hipMemcpyDeviceToHost, s));
    }
    return BPLHIP_OK;
}
static void season_sums(const std::vector<int64_t>& sums, const SeasonOut& out) {
    const size_t n = sums.size() / 2;
    std::copy(sums.begin(), sums.begin() + n, out.points_sum);
    std::copy(sums.begin() + n, sums.end(), out.gd_sum);
}

static int simulate_season_impl(bplhip_ctx* c, const SeasonCall& q, const SeasonOut& out, const PlayoffRequest* po = nullptr) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "simulate_season";
    SeasonSetup in;
    int rc = season_setup(c, what, q, BPLHIP_SEASON_MAX_FIXTURES, &in);
    if (rc != BPLHIP_OK) return rc;
    rc = season_out_check(c, what, out);
    if (rc != BPLHIP_OK) return rc;
    std::vector<uint16_t> slot_model;   // play-offs only
    if (po) {
        rc = playoff_check(c, *po, q.n_table, q.table_idx, &slot_model);
        if (rc != BPLHIP_OK) return rc;
    }
    SeasonStage st;
    rc = season_begin(c, what, q, in, &st);
    if (rc != BPLHIP_OK) return rc;
    const size_t nf = in.fix.size(), n = (size_t)q.n_table, ns = (size_t)q.n_sims;
    Carver cv;
    const SeasonCarve at = season_carve(cv, out, n, nf, ns);
    // with play-offs also stage counts u64 [nt, 8] and decided counts u64 [6, 4] (zeroed together), strengths f64
    // [nt], the slots' model indices u16 [nt], the bracket u16 [nb] and the per-simulation records asked for
    const size_t nt = po ? n + (size_t)po->n_guests : 0, nb = po ? (size_t)1 << po->rounds : 0;
    const size_t n_dec = (size_t)dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS;
    const size_t o_stc = cv.take(nt * dcpo::PLAYOFF_STAGES * 8), o_dec = cv.take(po ? n_dec * 8 : 0),
                 o_str = cv.take(nt * 8), o_mod = cv.take(nt * 2), o_br = cv.take(nb * 2),
                 o_sst = cv.take(po && po->sim_stage ? ns * nt : 0),
                 o_sdc = cv.take(po && po->sim_decided ? ns * (nb - 1) : 0);
    dcs::SeasonArgs A{};
    rc = season_args(c, q, st, cv, at, in, out, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    const dch::PairArgs& H = st.H;
    const SimLaunch L = sim_launch(c, q.h2h, q.n_table, q.n_sims, dcs::SEASON_WAVES, dcs::SEASON_BLOCKS_PER_CU);
    std::vector<double> strength;   // (outlives the asynchronous upload: the call synchronises before it returns)
    if (po) {
        strength.assign(nt, 0.0);
        if (po->strength) std::copy(po->strength, po->strength + nt, strength.begin());
        HIP_TRY(c, hipMemsetAsync(base + o_stc, 0, o_str - o_stc, s));
        HIP_TRY(c, hipMemcpyAsync(base + o_str, strength.data(), nt * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(base + o_mod, slot_model.data(), nt * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(base + o_br, po->bracket, nb * 2, hipMemcpyHostToDevice, s));
        dcpo::PlayoffArgs P{};
        P.g = po->n_guests;
        P.rounds = po->rounds;
        P.legs_mask = po->legs_mask;
        P.neutral_mask = po->neutral_mask;
        P.away_goals = po->away_goals;
        P.scale = po->scale;
        P.slot_model = reinterpret_cast<const uint16_t*>(base + o_mod);
        P.bracket = reinterpret_cast<const uint16_t*>(base + o_br);
        P.strength = reinterpret_cast<const double*>(base + o_str);
        P.stage_counts = reinterpret_cast<unsigned long long*>(base + o_stc);
        P.decided_counts = reinterpret_cast<unsigned long long*>(base + o_dec);
        P.sim_stage = po->sim_stage ? reinterpret_cast<uint8_t*>(base + o_sst) : nullptr;
        P.sim_decided = po->sim_decided ? reinterpret_cast<uint8_t*>(base + o_sdc) : nullptr;
        if (q.h2h.on) hipLaunchKernelGGL(dcpo::dc_playoff<true>, L.grid, L.block, L.lds, s, A, H, P);
        else hipLaunchKernelGGL(dcpo::dc_playoff<false>, L.grid, L.block, L.lds, s, A, H, P);
    } else if (q.h2h.on) hipLaunchKernelGGL(dcs::dc_season<true>, L.grid, L.block, L.lds, s, A, H);
    else hipLaunchKernelGGL(dcs::dc_season<false>, L.grid, L.block, L.lds, s, A, H);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint64_t> stage_dev(nt * dcpo::PLAYOFF_STAGES);
    if (po) {
        HIP_TRY(c, hipMemcpyAsync(stage_dev.data(), base + o_stc, stage_dev.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(po->decided_counts, base + o_dec, (size_t)po->rounds * dck::DECIDED_KINDS * 8,
                                  hipMemcpyDeviceToHost, s));
        if (po->sim_stage) HIP_TRY(c, hipMemcpyAsync(po->sim_stage, base + o_sst, ns * nt, hipMemcpyDeviceToHost, s));
        if (po->sim_decided)
            HIP_TRY(c, hipMemcpyAsync(po->sim_decided, base + o_sdc, ns * (nb - 1), hipMemcpyDeviceToHost, s));
    }
    std::vector<int64_t> sums;
    rc = season_read(c, st, at, out, n, nf, ns, sums);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    season_sums(sums, out);
    if (po)   // the device rows are PLAYOFF_STAGES wide, the caller's rounds + 2
        for (size_t i = 0; i < nt; ++i)
            std::copy_n(stage_dev.begin() + i * dcpo::PLAYOFF_STAGES, po->rounds + 2, po->stage_counts + i * (po->rounds + 2));
    return BPLHIP_OK;
}

// ---- simulate_season with matches in progress and weighted draws (dc_live.hip.h): what
// bplhip_simulate_season_live adds.  Every check before any device call
// LiveIn is what the live forms of match_leverage, season_points and season_scenarios take as well
struct LiveIn {
    int32_t n_in_play;
    const uint16_t *home_idx, *away_idx;     // HOST u16 [n_in_play]
    const uint8_t *home_goals, *away_goals;  // HOST u8 [n_in_play] the current score
    const double* elapsed;                   // HOST f64 [n_in_play]
    int32_t reweight;
    const double* log_weights;               // HOST f64 [s] or null
    double *ess, *log_evidence;              // HOST f64 [1]
};
struct LiveRequest {
    LiveIn in;
    int32_t* sim_draw;                       // i32 [n_sims] or null
    double *draw_log_weights, *draw_log_evidence;   // HOST f64 [s] or null
};
// the request's own checks, the first of a live call: the two lists' lengths against `max_fixtures`, the columns, the
// two outputs, the states
// (`fix_cols`, `side_cols`: the two columns of the fixture list and of the matches in play are there -- model indices
// in the season family, slots in simulate_tournament_live)
static int live_check_lists(bplhip_ctx* c, const char* what, int64_t n_fixtures, bool fix_cols, bool side_cols,
                            const LiveIn& lv, int max_fixtures) {
    if (n_fixtures < 0 || n_fixtures > max_fixtures || (n_fixtures > 0 && !fix_cols))
        return fail(c, BPLHIP_EINVAL, "%s: bad fixtures (n_fixtures=%lld)", what, (long long)n_fixtures);
    const int64_t L = lv.n_in_play;
    if (L < 0 || n_fixtures + L > max_fixtures)
        return fail(c, BPLHIP_EINVAL, "%s: n_in_play=%lld: fixtures plus matches in play number at most %d", what,
                    (long long)L, max_fixtures);
    if (L > 0 && (!side_cols || !lv.home_goals || !lv.away_goals || !lv.elapsed))
        return fail(c, BPLHIP_EINVAL, "%s: null in-play column", what);
    if (!lv.ess || !lv.log_evidence) return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    for (int64_t m = 0; m < L; ++m) {
        const double t = lv.elapsed[m];
        if (!(t >= 0.0 && t < 1.0))
            return fail(c, BPLHIP_EINVAL, "%s: elapsed %g of in-play match %lld outside [0, 1)", what, t, (long long)m);
        if (lv.home_goals[m] > BPLHIP_LIVE_MAX_GOALS || lv.away_goals[m] > BPLHIP_LIVE_MAX_GOALS)
            return fail(c, BPLHIP_EINVAL, "%s: score %d-%d of in-play match %lld beyond %d goals", what,
                        (int)lv.home_goals[m], (int)lv.away_goals[m], (long long)m, BPLHIP_LIVE_MAX_GOALS);
        if (t == 0.0 && (lv.home_goals[m] != 0 || lv.away_goals[m] != 0))
            return fail(c, BPLHIP_EINVAL, "%s: score %d-%d of in-play match %lld at elapsed = 0", what,
                        (int)lv.home_goals[m], (int)lv.away_goals[m], (long long)m);
    }
    return BPLHIP_OK;
}
static int live_check(bplhip_ctx* c, const char* what, const SeasonCall& call, const LiveIn& lv, int max_fixtures) {
    return live_check_lists(c, what, call.n_fixtures, call.home_idx && call.away_idx, lv.home_idx && lv.away_idx, lv,
                            max_fixtures);
}
// the concatenated list: the fixtures still to kick off, then the matches in play (after live_check); the call over
// it, whose index arrays `cat` owns
struct LiveList {
    std::vector<uint16_t> home, away;
};
static SeasonCall live_concat(const SeasonCall& call, const LiveIn& lv, LiveList* cat) {
    const size_t F = (size_t)call.n_fixtures, L = (size_t)lv.n_in_play, nf = F + L;
    cat->home.resize(nf);
    cat->away.resize(nf);
    std::copy_n(call.home_idx, F, cat->home.begin());
    std::copy_n(call.away_idx, F, cat->away.begin());
    std::copy_n(lv.home_idx, L, cat->home.begin() + F);
    std::copy_n(lv.away_idx, L, cat->away.begin() + F);
    SeasonCall q = call;
    q.n_fixtures = (int64_t)nf;
    q.home_idx = cat->home.data();
    q.away_idx = cat->away.data();
    return q;
}
// the last of a live call's checks of its inputs (after season_setup: a posterior is set); `lv` null: a kick-off call
static int live_weights_check(bplhip_ctx* c, const char* what, const LiveIn* lv) {
    const size_t S = (size_t)c->pred_S;
    if (lv && lv->log_weights)
        for (size_t i = 0; i < S; ++i)
            if (!std::isfinite(lv->log_weights[i])) return fail(c, BPLHIP_EINVAL, "%s: log weight %zu is not finite", what, i);
    return BPLHIP_OK;
}
// the live sections of a call's carved buffer, after the entry's own: the states (goals u32 [L], elapsed f64 [L]), the
// log weights f64 [S], L, L0 and the scan f64 [S] each, W / ess / log_evidence f64 [3]; the host's side of them
struct LivePlan {
    bool weighted = false;   // weights are in force
    size_t o_stg = 0, o_stt = 0, o_lw = 0, o_L = 0, o_L0 = 0, o_C = 0, o_stats = 0;
    std::vector<uint32_t> st_goals;   // [L]: a | b << 8 (outlives the asynchronous upload: the call synchronises)
    double stats[3] = {0.0, 0.0, 0.0};   // the landing place of W, ess, log_evidence
};
// after season_begin and the entry's own carve: the team-major tables the weight kernels read, then the sections
static int live_plan(bplhip_ctx* c, hipStream_t s, Carver& cv, const LiveIn& lv, LivePlan* P) {
    const size_t L = (size_t)lv.n_in_play, S = (size_t)c->pred_S;
    const bool weighted = P->weighted = lv.log_weights != nullptr || (lv.reweight != 0 && L > 0);
    if (weighted) {
        const int rc = loglik_team_major(c, s);
        if (rc != BPLHIP_OK) return rc;
    }
    P->o_stg = cv.take(L * 4);
    P->o_stt = cv.take(L * 8);
    P->o_lw = cv.take(weighted && lv.log_weights ? S * 8 : 0);
    P->o_L = cv.take(weighted ? S * 8 : 0);
    P->o_L0 = cv.take(weighted ? S * 8 : 0);
    P->o_C = cv.take(weighted ? S * 8 : 0);
    P->o_stats = cv.take(weighted ? 3 * 8 : 0);
    P->st_goals.resize(L);
    for (size_t m = 0; m < L; ++m) P->st_goals[m] = (uint32_t)lv.home_goals[m] | ((uint32_t)lv.away_goals[m] << 8);
    // without weights no kernel runs for them
    P->stats[0] = 0.0;
    P->stats[1] = (double)S;
    P->stats[2] = L > 0 ? std::nan("") : 0.0;
    return BPLHIP_OK;
}
// after season_stage has uploaded the concatenated list (`st_fix`: its device entries from F on): uploads the states
// and, with weights in force, runs live_loglik and live_weights -- once per call, before its simulators
static int live_upload(bplhip_ctx* c, hipStream_t s, char* base, const LiveIn& lv, const LivePlan& P) {
    const size_t L = (size_t)lv.n_in_play, S = (size_t)c->pred_S;
    if (L) {
        HIP_TRY(c, hipMemcpyAsync(base + P.o_stg, P.st_goals.data(), L * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(base + P.o_stt, lv.elapsed, L * 8, hipMemcpyHostToDevice, s));
    }
    if (P.weighted && lv.log_weights)
        HIP_TRY(c, hipMemcpyAsync(base + P.o_lw, lv.log_weights, S * 8, hipMemcpyHostToDevice, s));
    return BPLHIP_OK;
}
// the weight kernels' record with the draw count, the request and the plan's buffers filled (the season's tables and
// fixtures are live_stage's to add; simulate_tournament_live hands it to live_weights alone)
static dclive::LiveArgs live_args(const bplhip_ctx* c, char* base, const LiveIn& lv, const LivePlan& P) {
    dclive::LiveArgs W{};
    W.S = c->pred_S;
    W.L = lv.n_in_play;
    W.reweight = lv.reweight != 0;
    W.corr = c->dp_corr.as<const double>();
    W.st_goals = reinterpret_cast<const uint32_t*>(base + P.o_stg);
    W.st_t = reinterpret_cast<const double*>(base + P.o_stt);
    W.lw = lv.log_weights ? reinterpret_cast<const double*>(base + P.o_lw) : nullptr;
    W.Lw = reinterpret_cast<double*>(base + P.o_L);
    W.L0 = reinterpret_cast<double*>(base + P.o_L0);
    W.C = reinterpret_cast<double*>(base + P.o_C);
    W.stats = reinterpret_cast<double*>(base + P.o_stats);
    for (int k = 0; k <= dclive::LIVE_MAX_GOALS; ++k) W.lgf[k] = std::lgamma((double)k + 1.0);
    return W;
}
static dim3 live_grid(const bplhip_ctx* c) {
    return dim3((unsigned)((c->pred_S + dclive::LIVE_THREADS - 1) / dclive::LIVE_THREADS));
}
static int live_stage(bplhip_ctx* c, hipStream_t s, char* base, const LiveIn& lv, const LivePlan& P, const uint32_t* st_fix) {
    const int rc = live_upload(c, s, base, lv, P);
    if (rc != BPLHIP_OK || !P.weighted) return rc;
    dclive::LiveArgs W = live_args(c, base, lv, P);
    W.ha_stride = c->pred_ha_stride;
    W.attack = c->dp_tm[PT_ATT].as<const double>();
    W.defence = c->dp_tm[PT_DEF].as<const double>();
    W.home_adv = c->pred_ha_stride ? c->dp_tm[PT_HA].as<const double>() : c->dp_tab[PT_HA].as<const double>();
    W.st_fix = st_fix;
    const dim3 block(dclive::LIVE_THREADS);
    hipLaunchKernelGGL(dclive::live_loglik, live_grid(c), block, 0, s, W);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(dclive::live_weights, dim3(1), block, 0, s, W);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
// enqueues the copy of W / ess / log_evidence into the plan; live_finish hands them on once the stream is synchronised
static int live_read(bplhip_ctx* c, hipStream_t s, const char* base, LivePlan& P) {
    if (P.weighted) HIP_TRY(c, hipMemcpyAsync(P.stats, base + P.o_stats, 3 * 8, hipMemcpyDeviceToHost, s));
    return BPLHIP_OK;
}
static void live_finish(const LiveIn& lv, const LivePlan& P) {
    *lv.ess = P.stats[1];
    *lv.log_evidence = P.stats[2];
}
// the per-draw figures a live simulator returns when asked (rq.draw_log_weights / draw_log_evidence, null for the
// queries): queued copies of the draws' log weights and of the states' log likelihood where weights are in force,
// without them what live_plan says of a call that ran no weight kernel -- 0, and NaN with a match in play
static int live_read_draws(bplhip_ctx* c, hipStream_t s, const char* base, const LiveRequest& rq, const LivePlan& P) {
    const size_t S = (size_t)c->pred_S;
    if (P.weighted) {
        if (rq.draw_log_weights)
            HIP_TRY(c, hipMemcpyAsync(rq.draw_log_weights, base + P.o_L, S * 8, hipMemcpyDeviceToHost, s));
        if (rq.draw_log_evidence)
            HIP_TRY(c, hipMemcpyAsync(rq.draw_log_evidence, base + P.o_L0, S * 8, hipMemcpyDeviceToHost, s));
    } else {
        if (rq.draw_log_weights) std::fill_n(rq.draw_log_weights, S, 0.0);
        if (rq.draw_log_evidence) std::fill_n(rq.draw_log_evidence, S, rq.in.n_in_play > 0 ? std::nan("") : 0.0);
    }
    return BPLHIP_OK;
}
// what an entry of the season family does with a live request around its own steps, in one order for the simulator and
// the three queries: the lists checked and concatenated before season_setup, the log weights after the entry's own
// checks (live_weights_check), the live sections carved after the entry's own, after season_stage the states uploaded
// and the two weight kernels run, once per call, and the weights' figures read back.  Without a request (the kick-off
// entries) every step is empty and `q` is the caller's call.  The tournament family's twin is CupLiveQuery
struct SeasonLive {
    const LiveIn* lv = nullptr;
    const char* what = nullptr;   // the entry's name in its messages: the live form's with a request
    SeasonCall q{};               // the call over the concatenated list
    LiveList cat;                 // that list
    size_t F = 0;                 // the fixtures still to kick off
    LivePlan P;
    dclq::LiveQuery V{};          // what the live kernels take on top of their twins' records
};
static int season_live_lists(bplhip_ctx* c, const char* kick_off, const char* live, const SeasonCall& call, const LiveIn* lv,
                             int max_fixtures, SeasonLive* X) {
    X->lv = lv;
    X->what = lv ? live : kick_off;
    X->q = call;
    if (!lv) return BPLHIP_OK;
    const int rc = live_check(c, X->what, call, *lv, max_fixtures);
    if (rc != BPLHIP_OK) return rc;
    X->F = (size_t)call.n_fixtures;
    X->q = live_concat(call, *lv, &X->cat);
    return BPLHIP_OK;
}
// after season_begin and the entry's own carve
static int season_live_plan(bplhip_ctx* c, const SeasonStage& st, Carver& cv, SeasonLive& X) {
    return X.lv ? live_plan(c, st.s, cv, *X.lv, &X.P) : (int)BPLHIP_OK;
}
// after season_stage has uploaded the concatenated list to `fix`
static int season_live_stage(bplhip_ctx* c, const SeasonStage& st, const uint32_t* fix, SeasonLive& X) {
    if (!X.lv) return BPLHIP_OK;
    const LivePlan& P = X.P;
    X.V.F = (int)X.F;
    X.V.N = X.q.n_sims;
    X.V.st_goals = reinterpret_cast<const uint32_t*>(st.base + P.o_stg);
    X.V.st_t = reinterpret_cast<const double*>(st.base + P.o_stt);
    X.V.C = P.weighted ? reinterpret_cast<const double*>(st.base + P.o_C) : nullptr;
    return live_stage(c, st.s, st.base, *X.lv, P, fix + X.F);
}
// after the last kernel: the weights' figures queued; season_live_finish once the stream is synchronised
static int season_live_read(bplhip_ctx* c, const SeasonStage& st, SeasonLive& X) {
    return X.lv ? live_read(c, st.s, st.base, X.P) : (int)BPLHIP_OK;
}
static void season_live_finish(const SeasonLive& X) {
    if (X.lv) live_finish(*X.lv, X.P);
}
static int simulate_season_live_impl(bplhip_ctx* c, const SeasonCall& call, const SeasonOut& out, const LiveRequest& rq) {
    if (!c) return BPLHIP_EINVAL;
    SeasonLive X;
    int rc = season_live_lists(c, nullptr, "simulate_season_live", call, &rq.in, BPLHIP_SEASON_MAX_FIXTURES, &X);
    if (rc != BPLHIP_OK) return rc;
    const char* what = X.what;
    const SeasonCall& q = X.q;
    SeasonSetup in;
    rc = season_setup(c, what, q, BPLHIP_SEASON_MAX_FIXTURES, &in);
    if (rc != BPLHIP_OK) return rc;
    rc = season_out_check(c, what, out);
    if (rc != BPLHIP_OK) return rc;
    rc = live_weights_check(c, what, X.lv);
    if (rc != BPLHIP_OK) return rc;
    SeasonStage st;   // (the matches in play are meetings to come like any fixture)
    rc = season_begin(c, what, q, in, &st);
    if (rc != BPLHIP_OK) return rc;
    hipStream_t s = st.s;
    const size_t nf = in.fix.size(), n = (size_t)q.n_table, ns = (size_t)q.n_sims;
    // one buffer: simulate_season's, then the live sections and the draws i32 [n_sims]
    Carver cv;
    const SeasonCarve at = season_carve(cv, out, n, nf, ns);
    rc = season_live_plan(c, st, cv, X);
    if (rc != BPLHIP_OK) return rc;
    const size_t o_draw = cv.take(rq.sim_draw ? ns * 4 : 0);
    dcs::SeasonArgs A{};
    rc = season_args(c, q, st, cv, at, in, out, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    rc = season_live_stage(c, st, A.fix, X);
    if (rc != BPLHIP_OK) return rc;
    dclive::LiveSim V{};
    V.F = X.V.F;
    V.st_goals = X.V.st_goals;
    V.st_t = X.V.st_t;
    V.C = X.V.C;
    V.sim_draw = rq.sim_draw ? reinterpret_cast<int32_t*>(base + o_draw) : nullptr;
    const SimLaunch LN = sim_launch(c, q.h2h, q.n_table, q.n_sims, dcs::SEASON_WAVES, dcs::SEASON_BLOCKS_PER_CU);
    if (q.h2h.on) hipLaunchKernelGGL(dclive::dc_season_live<true>, LN.grid, LN.block, LN.lds, s, A, st.H, V);
    else hipLaunchKernelGGL(dclive::dc_season_live<false>, LN.grid, LN.block, LN.lds, s, A, st.H, V);
    HIP_TRY(c, hipGetLastError());
    std::vector<int64_t> sums;
    rc = season_read(c, st, at, out, n, nf, ns, sums);
    if (rc != BPLHIP_OK) return rc;
    if (rq.sim_draw) HIP_TRY(c, hipMemcpyAsync(rq.sim_draw, base + o_draw, ns * 4, hipMemcpyDeviceToHost, s));
    rc = season_live_read(c, st, X);
    if (rc != BPLHIP_OK) return rc;
    rc = live_read_draws(c, s, base, rq, X.P);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    season_sums(sums, out);
    season_live_finish(X);
    return BPLHIP_OK;
}

// ---- match_leverage (dc_leverage.hip.h): dc_season's simulations, cross-tabulated on the device chunk by chunk
// `lv` (bplhip_match_leverage_live): the fixtures are the concatenated list, the draws may carry weights and stage 1 is
// dclq::live_leverage_sim (dc_live_queries.hip.h); null: the kick-off call, as it was before the live form existed
static int match_leverage_impl(bplhip_ctx* c, const SeasonCall& call, const TargetRequest& tg, uint64_t* outcome_counts,
                               uint64_t* target_counts, uint64_t* joint_counts, const LiveIn* lv = nullptr) {
    if (!c) return BPLHIP_EINVAL;
    SeasonLive X;
    int rc = season_live_lists(c, "match_leverage", "match_leverage_live", call, lv, BPLHIP_LEVERAGE_MAX_FIXTURES, &X);
    if (rc != BPLHIP_OK) return rc;
    const char* what = X.what;
    const SeasonCall& q = X.q;
    SeasonSetup in;
    rc = season_setup(c, what, q, BPLHIP_LEVERAGE_MAX_FIXTURES, &in);
    if (rc != BPLHIP_OK) return rc;
    rc = targets_check(c, what, q.n_table, tg);
    if (rc != BPLHIP_OK) return rc;
    if (!outcome_counts || !target_counts || !joint_counts) return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    rc = live_weights_check(c, what, lv);
    if (rc != BPLHIP_OK) return rc;
    SeasonStage st;
    rc = season_begin(c, what, q, in, &st);
    if (rc != BPLHIP_OK) return rc;
    const size_t nf = in.fix.size(), n = (size_t)q.n_table, K = (size_t)tg.n_targets, nK = n * K;
    const size_t blocks = (nf + 63) / 64;
    // a simulation's record: 16 B per 64 fixtures and n bytes
    const size_t chunk = chunk_for(tg.chunk_sims, blocks * 16 + n, q.n_sims);
    // one buffer: the ballots first (16-byte records), then joint u64 [nf, 3, n, K], outcome u64 [nf, 3], target
    // u64 [n, K] (zeroed together), fixtures u32 [nf], table i32 [3, n], slots u16 [nf], the target sets u8 [chunk, n]
    Carver cv;
    cv.take((blocks * chunk * 16 + 15) & ~(size_t)15);
    const size_t o_joint = cv.take(nf * 3 * nK * 8), o_out = cv.take(nf * 3 * 8), o_tgt = cv.take(nK * 8),
                 o_fix = cv.take(nf * 4), o_init = cv.take(3 * n * 4), o_slot = cv.take(nf * 2), o_set = cv.take(chunk * n);
    rc = season_live_plan(c, st, cv, X);   // (live only: its sections follow)
    if (rc != BPLHIP_OK) return rc;
    dclev::LeverageArgs A{};
    rc = season_stage(c, q, st, cv, c->dp_leverage, {o_joint, o_fix, o_slot, o_init}, in.fix, in.fix_slot, in.init, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    rc = season_live_stage(c, st, A.fix, X);
    if (rc != BPLHIP_OK) return rc;
    const dclq::LiveQuery& V = X.V;
    target_args(A, tg, chunk);
    A.ball = reinterpret_cast<unsigned long long*>(base);
    A.tset = reinterpret_cast<uint8_t*>(base + o_set);
    A.target = reinterpret_cast<unsigned long long*>(base + o_tgt);
    A.outcome = reinterpret_cast<unsigned long long*>(base + o_out);
    A.joint = reinterpret_cast<unsigned long long*>(base + o_joint);
    A.slots_per_tile = dclev::COUNT_COLS / tg.n_targets;
    const unsigned tiles = (unsigned)((n + A.slots_per_tile - 1) / A.slots_per_tile);
    const dim3 block(64 * dclev::LEVERAGE_WAVES);
    for (int64_t j0 = 0; j0 < q.n_sims; j0 += (int64_t)chunk) {
        A.j0 = j0;
        A.nc = (int)std::min<int64_t>((int64_t)chunk, q.n_sims - j0);
        const SimLaunch L = sim_launch(c, q.h2h, q.n_table, A.nc, dclev::LEVERAGE_WAVES, dclev::LEVERAGE_BLOCKS_PER_CU);
        if (lv && q.h2h.on) hipLaunchKernelGGL(dclq::live_leverage_sim<true>, L.grid, L.block, L.lds, s, A, st.H, V);
        else if (lv) hipLaunchKernelGGL(dclq::live_leverage_sim<false>, L.grid, L.block, L.lds, s, A, st.H, V);
        else if (q.h2h.on) hipLaunchKernelGGL(dclev::dc_leverage_sim<true>, L.grid, L.block, L.lds, s, A, st.H);
        else hipLaunchKernelGGL(dclev::dc_leverage_sim<false>, L.grid, L.block, L.lds, s, A, st.H);
        HIP_TRY(c, hipGetLastError());
        if (nf) {
            // shares of the chunk's 64-simulation groups: enough workgroups to fill the device, each with at
            // least one round of LEVERAGE_WAVES groups
            const long long rounds = ((A.nc + 63) / 64 + dclev::LEVERAGE_WAVES - 1) / dclev::LEVERAGE_WAVES;
            const long long fill = (2ll * c->n_cu + (long long)(blocks * tiles) - 1) / (long long)(blocks * tiles);
            const dim3 cgrid((unsigned)blocks, tiles, (unsigned)std::max(1ll, std::min({rounds, fill, 65535ll})));
            hipLaunchKernelGGL(dclev::dc_leverage_count, cgrid, block, 0, s, A);
            HIP_TRY(c, hipGetLastError());
        }
    }
    HIP_TRY(c, hipMemcpyAsync(joint_counts, base + o_joint, nf * 3 * nK * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(outcome_counts, base + o_out, nf * 3 * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(target_counts, base + o_tgt, nK * 8, hipMemcpyDeviceToHost, s));
    rc = season_live_read(c, st, X);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    season_live_finish(X);
    // the draw is what the wins leave: every simulation gives a fixture exactly one outcome
    for (size_t f = 0; f < nf; ++f) {
        uint64_t* oc = outcome_counts + f * 3;
        oc[1] = (uint64_t)q.n_sims - oc[0] - oc[2];
        uint64_t* jc = joint_counts + f * 3 * nK;
        for (size_t i = 0; i < nK; ++i) jc[nK + i] = target_counts[i] - jc[i] - jc[2 * nK + i];
    }
    return BPLHIP_OK;
}

// ---- season_points (dc_points.hip.h): dc_season's simulations, their points cross-tabulated on the device chunk by chunk
// `lv` (bplhip_season_points_live): as for match_leverage_impl, stage 1 being dclq::live_points_sim; the axis counts the
// matches in play among a slot's remaining matches
static int season_points_impl(bplhip_ctx* c, const SeasonCall& call, const TargetRequest& tg, int32_t points_min,
                              int32_t n_bins, uint64_t* team_points, uint64_t* team_target, uint64_t* position_points,
                              uint64_t* gap, const LiveIn* lv = nullptr) {
    if (!c) return BPLHIP_EINVAL;
    SeasonLive X;
    int rc = season_live_lists(c, "season_points", "season_points_live", call, lv, BPLHIP_LEVERAGE_MAX_FIXTURES, &X);
    if (rc != BPLHIP_OK) return rc;
    const char* what = X.what;
    const SeasonCall& q = X.q;
    SeasonSetup in;
    rc = season_setup(c, what, q, BPLHIP_LEVERAGE_MAX_FIXTURES, &in);
    if (rc != BPLHIP_OK) return rc;
    rc = targets_check(c, what, q.n_table, tg);
    if (rc != BPLHIP_OK) return rc;
    if (n_bins < 1 || n_bins > BPLHIP_POINTS_MAX_BINS)
        return fail(c, BPLHIP_EINVAL, "%s: n_bins=%d out of range [1,%d]", what, n_bins, BPLHIP_POINTS_MAX_BINS);
    if (!team_points || !team_target || !position_points || (!gap && q.n_table > 1))
        return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    // the axis holds every total a simulation can reach: a match gives its least points at the worst
    rc = axis_check(c, what, "can end on", q, in, std::min({q.win, q.draw, q.loss}), points_min, n_bins);
    if (rc != BPLHIP_OK) return rc;
    rc = live_weights_check(c, what, lv);
    if (rc != BPLHIP_OK) return rc;
    SeasonStage st;
    rc = season_begin(c, what, q, in, &st);
    if (rc != BPLHIP_OK) return rc;
    const size_t nf = in.fix.size(), n = (size_t)q.n_table, K = (size_t)tg.n_targets, P = (size_t)n_bins;
    // a simulation's record: 5 n bytes
    const size_t chunk = chunk_for(tg.chunk_sims, 5 * n, q.n_sims);
    // one buffer: team_points u64 [n, P], team_target u64 [n, P, K], position_points u64 [n, P], gap u64 [n - 1, P]
    // (zeroed together), fixtures u32 [nf], table i32 [3, n], slots u16 [nf], then the chunk's rows: bins by slot and
    // by position u16 [n, chunk] each, target sets u8 [n, chunk]
    Carver cv;
    cv.take(n * P * 8);
    const size_t o_tt = cv.take(n * P * K * 8), o_pp = cv.take(n * P * 8), o_gap = cv.take((n - 1) * P * 8),
                 o_fix = cv.take(nf * 4), o_init = cv.take(3 * n * 4), o_slot = cv.take(nf * 2),
                 o_sp = cv.take(n * chunk * 2), o_ps = cv.take(n * chunk * 2), o_set = cv.take(n * chunk);
    rc = season_live_plan(c, st, cv, X);   // (live only: its sections follow)
    if (rc != BPLHIP_OK) return rc;
    dcpt::PointsArgs A{};
    rc = season_stage(c, q, st, cv, c->dp_points, {0, o_fix, o_slot, o_init}, in.fix, in.fix_slot, in.init, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    rc = season_live_stage(c, st, A.fix, X);
    if (rc != BPLHIP_OK) return rc;
    const dclq::LiveQuery& V = X.V;
    target_args(A, tg, chunk);
    A.points_min = points_min;
    A.P = n_bins;
    A.slot_pts = reinterpret_cast<uint16_t*>(base + o_sp);
    A.pos_pts = reinterpret_cast<uint16_t*>(base + o_ps);
    A.tset = reinterpret_cast<uint8_t*>(base + o_set);
    A.team_points = reinterpret_cast<unsigned long long*>(base);
    A.team_target = reinterpret_cast<unsigned long long*>(base + o_tt);
    A.position_points = reinterpret_cast<unsigned long long*>(base + o_pp);
    A.gap = reinterpret_cast<unsigned long long*>(base + o_gap);
    const unsigned rows = (unsigned)(3 * n - 1);
    for (int64_t j0 = 0; j0 < q.n_sims; j0 += (int64_t)chunk) {
        A.j0 = j0;
        A.nc = (int)std::min<int64_t>((int64_t)chunk, q.n_sims - j0);
        const SimLaunch L = sim_launch(c, q.h2h, q.n_table, A.nc, dcpt::POINTS_WAVES, dcpt::POINTS_BLOCKS_PER_CU);
        if (lv && q.h2h.on) hipLaunchKernelGGL(dclq::live_points_sim<true>, L.grid, L.block, L.lds, s, A, st.H, V);
        else if (lv) hipLaunchKernelGGL(dclq::live_points_sim<false>, L.grid, L.block, L.lds, s, A, st.H, V);
        else if (q.h2h.on) hipLaunchKernelGGL(dcpt::dc_points_sim<true>, L.grid, L.block, L.lds, s, A, st.H);
        else hipLaunchKernelGGL(dcpt::dc_points_sim<false>, L.grid, L.block, L.lds, s, A, st.H);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(dcpt::dc_points_count, count_grid(c, rows, A.nc, dcpt::COUNT_THREADS), dim3(dcpt::COUNT_THREADS), 0,
                           s, A);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(team_points, base, n * P * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(team_target, base + o_tt, n * P * K * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(position_points, base + o_pp, n * P * 8, hipMemcpyDeviceToHost, s));
    if (n > 1) HIP_TRY(c, hipMemcpyAsync(gap, base + o_gap, (n - 1) * P * 8, hipMemcpyDeviceToHost, s));
    rc = season_live_read(c, st, X);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    season_live_finish(X);
    return BPLHIP_OK;
}

// ---- the scenario keys, as season_scenarios and tournament_scenarios take them: n_key and the pointers, the positions
// in a list of n_fixtures, the caps, then the number of scenarios into `cells`
static int scenario_keys_check(bplhip_ctx* c, const char* what, int32_t n_key, const int32_t* key_fixture,
                               const int32_t* key_cap, int64_t n_fixtures, int64_t* cells) {
    if (n_key < 1 || n_key > BPLHIP_SCENARIO_MAX_KEYS || !key_fixture || !key_cap)
        return fail(c, BPLHIP_EINVAL, "%s: n_key=%d out of range [1,%d] or null keys", what, n_key, BPLHIP_SCENARIO_MAX_KEYS);
    for (int i = 0; i < n_key; ++i) {
        if (key_fixture[i] < 0 || key_fixture[i] >= n_fixtures)
            return fail(c, BPLHIP_EINVAL, "%s: key fixture %d is %d, outside [0,%lld)", what, i, key_fixture[i],
                        (long long)n_fixtures);
        for (int r = 0; r < i; ++r)
            if (key_fixture[r] == key_fixture[i])
                return fail(c, BPLHIP_EINVAL, "%s: key fixtures %d and %d are both fixture %d", what, r, i, key_fixture[i]);
    }
    *cells = 1;
    for (int i = 0; i < n_key; ++i) {
        if (key_cap[i] < 1 || key_cap[i] > BPLHIP_SCENARIO_MAX_CAP)
            return fail(c, BPLHIP_EINVAL, "%s: the cap of key fixture %d is %d, outside [1,%d]", what, i, key_cap[i],
                        BPLHIP_SCENARIO_MAX_CAP);
        *cells *= 2 * key_cap[i] + 1;   // (at most 7^8: far inside 64 bits)
    }
    if (*cells > BPLHIP_SCENARIO_MAX_CELLS)
        return fail(c, BPLHIP_EINVAL, "%s: %lld scenarios, at most %d", what, (long long)*cells, BPLHIP_SCENARIO_MAX_CELLS);
    return BPLHIP_OK;
}
// a fixture's code: the stride of its class in the scenario index and its cap, 0 when it is no key
static std::vector<uint16_t> scenario_codes(size_t nf, int32_t n_key, const int32_t* key_fixture, const int32_t* key_cap) {
    std::vector<uint16_t> code(nf, 0);
    for (int i = n_key - 1, stride = 1; i >= 0; stride *= 2 * key_cap[i] + 1, --i)
        code[(size_t)key_fixture[i]] = (uint16_t)(stride | (key_cap[i] << dcsc::CODE_CAP_SHIFT));
    return code;
}

// ---- season_scenarios (dc_scenario.hip.h): dc_season's simulations, the joint class of the key fixtures cross-tabulated
// against the targets on the device chunk by chunk
// `lv` (bplhip_season_scenarios_live): as for match_leverage_impl, stage 1 being dclq::live_scenario_sim; key_fixture
// indexes the concatenated list, n_fixtures + m being match m in play
static int season_scenarios_impl(bplhip_ctx* c, const SeasonCall& call, const TargetRequest& tg, int32_t n_key,
                                 const int32_t* key_fixture, const int32_t* key_cap, uint64_t* scenario, uint64_t* joint,
                                 const LiveIn* lv = nullptr) {
    if (!c) return BPLHIP_EINVAL;
    SeasonLive X;
    int rc = season_live_lists(c, "season_scenarios", "season_scenarios_live", call, lv, BPLHIP_LEVERAGE_MAX_FIXTURES, &X);
    if (rc != BPLHIP_OK) return rc;
    const char* what = X.what;
    const SeasonCall& q = X.q;
    SeasonSetup in;
    rc = season_setup(c, what, q, BPLHIP_LEVERAGE_MAX_FIXTURES, &in);
    if (rc != BPLHIP_OK) return rc;
    rc = targets_check(c, what, q.n_table, tg);
    if (rc != BPLHIP_OK) return rc;
    int64_t cells = 1;
    rc = scenario_keys_check(c, what, n_key, key_fixture, key_cap, q.n_fixtures, &cells);
    if (rc != BPLHIP_OK) return rc;
    if (!scenario || !joint) return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    rc = live_weights_check(c, what, lv);
    if (rc != BPLHIP_OK) return rc;
    SeasonStage st;
    rc = season_begin(c, what, q, in, &st);
    if (rc != BPLHIP_OK) return rc;
    const size_t nf = in.fix.size(), n = (size_t)q.n_table, K = (size_t)tg.n_targets, nK = n * K, M = (size_t)cells;
    const std::vector<uint16_t> code = scenario_codes(nf, n_key, key_fixture, key_cap);
    // a simulation's record: 4 + n bytes
    const size_t chunk = chunk_for(tg.chunk_sims, 4 + n, q.n_sims);
    // one buffer: scenario u64 [M], joint u64 [M, n, K] (zeroed together), fixtures u32 [nf], table i32 [3, n], slots
    // u16 [nf], codes u16 [nf], then the chunk's records: scenario indices u32 [chunk], target sets u8 [n, chunk]
    Carver cv;
    cv.take(M * 8);
    const size_t o_joint = cv.take(M * nK * 8), o_fix = cv.take(nf * 4), o_init = cv.take(3 * n * 4),
                 o_slot = cv.take(nf * 2), o_code = cv.take(nf * 2), o_scen = cv.take(chunk * 4),
                 o_set = cv.take(n * chunk);
    rc = season_live_plan(c, st, cv, X);   // (live only: its sections follow)
    if (rc != BPLHIP_OK) return rc;
    dcsc::ScenarioArgs A{};
    rc = season_stage(c, q, st, cv, c->dp_scenario, {0, o_fix, o_slot, o_init}, in.fix, in.fix_slot, in.init, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    rc = season_live_stage(c, st, A.fix, X);
    if (rc != BPLHIP_OK) return rc;
    const dclq::LiveQuery& V = X.V;
    HIP_TRY(c, hipMemcpyAsync(base + o_code, code.data(), nf * 2, hipMemcpyHostToDevice, s));
    target_args(A, tg, chunk);
    A.M = (int)M;
    // a stage-2 tile: as many whole scenarios as its LDS cells hold (at least 31: 1 + n K <= 513)
    A.tile_rows = (int)std::min<size_t>(M, (size_t)dcsc::COUNT_WORDS / (1 + nK));
    A.fix_code = reinterpret_cast<const uint16_t*>(base + o_code);
    A.scen = reinterpret_cast<uint32_t*>(base + o_scen);
    A.tset = reinterpret_cast<uint8_t*>(base + o_set);
    A.scenario = reinterpret_cast<unsigned long long*>(base);
    A.joint = reinterpret_cast<unsigned long long*>(base + o_joint);
    const unsigned tiles = (unsigned)((M + A.tile_rows - 1) / A.tile_rows);
    for (int64_t j0 = 0; j0 < q.n_sims; j0 += (int64_t)chunk) {
        A.j0 = j0;
        A.nc = (int)std::min<int64_t>((int64_t)chunk, q.n_sims - j0);
        const SimLaunch L = sim_launch(c, q.h2h, q.n_table, A.nc, dcsc::SCENARIO_WAVES, dcsc::SCENARIO_BLOCKS_PER_CU);
        if (lv && q.h2h.on) hipLaunchKernelGGL(dclq::live_scenario_sim<true>, L.grid, L.block, L.lds, s, A, st.H, V);
        else if (lv) hipLaunchKernelGGL(dclq::live_scenario_sim<false>, L.grid, L.block, L.lds, s, A, st.H, V);
        else if (q.h2h.on) hipLaunchKernelGGL(dcsc::dc_scenario_sim<true>, L.grid, L.block, L.lds, s, A, st.H);
        else hipLaunchKernelGGL(dcsc::dc_scenario_sim<false>, L.grid, L.block, L.lds, s, A, st.H);
        HIP_TRY(c, hipGetLastError());
        // (shares of at least 4, 8 and 32 passes instead of count_grid's one were measured and were no faster:
        // profiles/scenarios/count_ab.txt)
        hipLaunchKernelGGL(dcsc::dc_scenario_count, count_grid(c, tiles, A.nc, dcsc::COUNT_THREADS),
                           dim3(dcsc::COUNT_THREADS), 0, s, A);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(scenario, base, M * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(joint, base + o_joint, M * nK * 8, hipMemcpyDeviceToHost, s));
    rc = season_live_read(c, st, X);
    if (rc != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    season_live_finish(X);
    return BPLHIP_OK;
}

// ---- season_trajectory (dc_trajectory.hip.h): dc_season's simulations ranked after every matchday, the paths counted
// on the device chunk by chunk
struct TrajectoryOut {
    uint64_t *position_count, *target_count, *target_final_count, *points_sum, *points_sq_sum, *rounds_inside_count,
        *secured_count, *lead_changes_count;
};
static int season_trajectory_impl(bplhip_ctx* c, const SeasonCall& q, const TargetRequest& tg, int32_t points_min,
                                  int32_t n_bins, int32_t n_rounds, const int32_t* round_end, const int32_t* fix_id,
                                  const TrajectoryOut& out) {
    if (!c) return BPLHIP_EINVAL;
    const char* what = "season_trajectory";
    const int64_t n_fixtures = q.n_fixtures;
    SeasonSetup in;
    int rc = season_setup(c, what, q, BPLHIP_LEVERAGE_MAX_FIXTURES, &in);
    if (rc != BPLHIP_OK) return rc;
    rc = targets_check(c, what, q.n_table, tg);
    if (rc != BPLHIP_OK) return rc;
    if (n_bins < 1 || n_bins > BPLHIP_POINTS_MAX_BINS)
        return fail(c, BPLHIP_EINVAL, "%s: n_bins=%d out of range [1,%d]", what, n_bins, BPLHIP_POINTS_MAX_BINS);
    if (n_rounds < 1 || n_rounds > BPLHIP_TRAJECTORY_MAX_ROUNDS || !round_end || (n_fixtures > 0 && !fix_id))
        return fail(c, BPLHIP_EINVAL, "%s: n_rounds=%d out of range [1,%d], or null round_end / fix_id", what, n_rounds,
                    BPLHIP_TRAJECTORY_MAX_ROUNDS);
    if (!out.position_count || !out.target_count || !out.target_final_count || !out.points_sum || !out.points_sq_sum ||
        !out.rounds_inside_count || !out.secured_count || !out.lead_changes_count)
        return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    const size_t nf = in.fix.size(), n = (size_t)q.n_table, K = (size_t)tg.n_targets, R = (size_t)n_rounds;
    for (size_t r = 0; r < R; ++r)
        if (round_end[r] < (r ? round_end[r - 1] : 0) || (int64_t)round_end[r] > n_fixtures)
            return fail(c, BPLHIP_EINVAL, "%s: round_end[%zu]=%d is not non-decreasing within the fixtures", what, r,
                        round_end[r]);
    if ((int64_t)round_end[R - 1] != n_fixtures)
        return fail(c, BPLHIP_EINVAL, "%s: round_end ends at %d, not at n_fixtures=%lld", what, round_end[R - 1],
                    (long long)n_fixtures);
    // the fixtures in the order of fix_id, which must name every fixture once
    std::vector<uint32_t> fix(nf);
    std::vector<uint16_t> fix_slot(nf), ids(nf);
    {
        std::vector<char> seen(nf, 0);
        for (size_t f = 0; f < nf; ++f) {
            const int64_t g = fix_id[f];
            if (g < 0 || g >= n_fixtures || seen[(size_t)g])
                return fail(c, BPLHIP_EINVAL, "%s: fix_id is not a permutation of the fixtures (entry %zu)", what, f);
            seen[(size_t)g] = 1;
            fix[f] = in.fix[(size_t)g];
            fix_slot[f] = in.fix_slot[(size_t)g];
            ids[f] = (uint16_t)g;
        }
    }
    // the axis holds every total a simulation passes through: a match gives no negative points, so the least is
    // the current total
    rc = axis_check(c, what, "can stand on", q, in, 0, points_min, n_bins);
    if (rc != BPLHIP_OK) return rc;
    SeasonStage st;
    rc = season_begin(c, what, q, in, &st);
    if (rc != BPLHIP_OK) return rc;
    // a simulation's record: 3 n R + R bytes
    const size_t chunk = chunk_for(tg.chunk_sims, 3 * n * R + R, q.n_sims);
    // one buffer: position u64 [R, n, n], target and target_final u64 [R, n, K], the sums u64 [2, R, n], rounds_inside
    // and secured u64 [n, K, R + 1], lead_changes u64 [R] (zeroed together), fixtures u32 [nf], table i32 [3, n],
    // round_end i32 [R], slots and ids u16 [nf], then the chunk's rows: v u16 [R, n, chunk], positions u8 [R, n, chunk],
    // leaders u8 [R, chunk]
    Carver cv;
    cv.take(R * n * n * 8);
    const size_t o_tc = cv.take(R * n * K * 8), o_tf = cv.take(R * n * K * 8), o_sum = cv.take(2 * R * n * 8),
                 o_in = cv.take(n * K * (R + 1) * 8), o_sec = cv.take(n * K * (R + 1) * 8), o_lead = cv.take(R * 8),
                 o_fix = cv.take(nf * 4), o_init = cv.take(3 * n * 4), o_end = cv.take(R * 4), o_slot = cv.take(nf * 2),
                 o_id = cv.take(nf * 2), o_pts = cv.take(R * n * chunk * 2), o_pos = cv.take(R * n * chunk),
                 o_ldr = cv.take(R * chunk);
    dctr::TrajectoryArgs A{};
    rc = season_stage(c, q, st, cv, c->dp_trajectory, {0, o_fix, o_slot, o_init}, fix, fix_slot, in.init, A);
    if (rc != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    if (nf) HIP_TRY(c, hipMemcpyAsync(base + o_id, ids.data(), nf * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(base + o_end, round_end, R * 4, hipMemcpyHostToDevice, s));
    target_args(A, tg, chunk);
    A.R = n_rounds;
    A.points_min = points_min;
    A.fix_id = reinterpret_cast<const uint16_t*>(base + o_id);
    A.round_end = reinterpret_cast<const int32_t*>(base + o_end);
    A.pos = reinterpret_cast<uint8_t*>(base + o_pos);
    A.pts = reinterpret_cast<uint16_t*>(base + o_pts);
    A.leader = reinterpret_cast<uint8_t*>(base + o_ldr);
    A.position_count = reinterpret_cast<unsigned long long*>(base);
    A.target_count = reinterpret_cast<unsigned long long*>(base + o_tc);
    A.target_final_count = reinterpret_cast<unsigned long long*>(base + o_tf);
    A.points_sum = reinterpret_cast<unsigned long long*>(base + o_sum);
    A.rounds_inside = reinterpret_cast<unsigned long long*>(base + o_in);
    A.secured = reinterpret_cast<unsigned long long*>(base + o_sec);
    A.lead_changes = reinterpret_cast<unsigned long long*>(base + o_lead);
    const unsigned rows = (unsigned)(R * n), path_rows = (unsigned)(n + 1);
    const dim3 cblock(dctr::COUNT_THREADS);
    for (int64_t j0 = 0; j0 < q.n_sims; j0 += (int64_t)chunk) {
        A.j0 = j0;
        A.nc = (int)std::min<int64_t>((int64_t)chunk, q.n_sims - j0);
        const SimLaunch L = sim_launch(c, q.h2h, q.n_table, A.nc, dctr::TRAJECTORY_WAVES, dctr::TRAJECTORY_BLOCKS_PER_CU);
        if (q.h2h.on) hipLaunchKernelGGL(dctr::dc_trajectory_sim<true>, L.grid, L.block, L.lds, s, A, st.H);
        else hipLaunchKernelGGL(dctr::dc_trajectory_sim<false>, L.grid, L.block, L.lds, s, A, st.H);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(dctr::dc_trajectory_count, count_grid(c, rows, A.nc, dctr::COUNT_THREADS), cblock, 0, s, A);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(dctr::dc_trajectory_paths, count_grid(c, path_rows, A.nc, dctr::COUNT_THREADS), cblock, 0, s, A);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(out.position_count, base, R * n * n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.target_count, base + o_tc, R * n * K * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.target_final_count, base + o_tf, R * n * K * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.points_sum, base + o_sum, R * n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.points_sq_sum, base + o_sum + R * n * 8, R * n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.rounds_inside_count, base + o_in, n * K * (R + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.secured_count, base + o_sec, n * K * (R + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out.lead_changes_count, base + o_lead, R * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return BPLHIP_OK;
}

// ---- the extra-time knockout rule (dc_knockout.hip.h): what bplhip_simulate_tournament_knockout adds
struct KnockoutRequest {
    uint32_t legs_mask;
    double scale;
    int32_t away_goals;
    const double* strength;      // HOST f64 [n] or null (all zero)
    uint64_t* decided_counts;    // HOST u64 [R, 4]
    uint8_t* sim_decided;        // u8 [n_sims, 2^R - 1] or null
};

// ---- tournament_paths (dc_paths.hip.h): what bplhip_tournament_paths adds.  The simulations pass through a workspace
// of `chunk` records; sim_stage and the extra-time rule's sim_decided are then filled chunk by chunk as well
struct PathsRequest {
    int64_t chunk_sims;                // simulations per pass through the workspace, 0 = chunk_for's choice
    uint64_t* advance_counts;          // HOST u64 [R, n, n]
    uint64_t* position_stage_counts;   // HOST u64 [n, 8, 8] (required with groups)
    uint64_t* outcome_counts;          // HOST u64 [nf, 3]      (required with fixtures, as the two below)
    uint64_t* target_counts;           // HOST u64 [n, R + 1]
    uint64_t* joint_counts;            // HOST u64 [nf, 3, n, R + 1]
    uint8_t* sim_position;             // u8 [n_sims, n] or null
    uint8_t* sim_outcome;              // u8 [n_sims, nf] or null
    uint8_t* sim_pair;                 // u8 [n_sims, 2^R - 1, 2] or null
    uint8_t* sim_winner;               // u8 [n_sims, 2^R - 1] or null
};

// ---- tournament_scenarios (dc_tscen.hip.h): what bplhip_tournament_scenarios adds.  The simulations pass through a
// workspace of `chunk` records of 4 + n bytes and are counted by dc_scenario_count; stage_counts,
// group_position_counts and sim_stage are not asked for
struct TscenRequest {
    int64_t chunk_sims;                // simulations per pass through the workspace, 0 = chunk_for's choice
    int32_t n_key;
    const int32_t* key_fixture;        // HOST i32 [n_key] positions in the group-fixture list
    const int32_t* key_cap;            // HOST i32 [n_key] margin caps
    uint64_t* scenario;                // HOST u64 [M]
    uint64_t* joint;                   // HOST u64 [M, n, R + 2]
    uint32_t* sim_scenario;            // u32 [n_sims] or null
    uint8_t* sim_tset;                 // u8 [n_sims, n] or null
};

// ---- tournament_points (dc_group_points.hip.h): what bplhip_tournament_points adds.  The simulations pass through a
// workspace of `chunk` records of 4 n + Gn Z + 2 B bytes and are counted by dc_gpts_count; stage_counts,
// group_position_counts and sim_stage are not asked for
struct GptsRequest {
    int64_t chunk_sims;                // simulations per pass through the workspace, 0 = chunk_for's choice
    int32_t points_min, n_bins;        // the points axis
    int32_t gd_cap;                    // the goal-difference axis: 2 gd_cap + 1 bins
    uint64_t* team_points;             // HOST u64 [n, P]
    uint64_t* team_target;             // HOST u64 [n, P, R + 2]
    uint64_t* team_place;              // HOST u64 [n, P, Z]
    uint64_t* place_points;            // HOST u64 [Gn, Z, P]
    uint64_t* place_gap;               // HOST u64 [Gn, Z - 1, P]
    uint64_t* rest_count;              // HOST u64 [P, D]     (these three with best_of_rest > 0)
    uint64_t* rest_through;            // HOST u64 [P, D]
    uint64_t* rest_rank;               // HOST u64 [B, P, D]
};

// ---- the tournament family: simulate_tournament (and _h2h, _knockout), tournament_paths, tournament_scenarios and
// tournament_points.  TournamentCall is what all six exported symbols take first, as their wrappers hand it on
struct TournamentCall {
    int32_t n_teams;
    const uint16_t *team_idx, *team_conf;             // HOST u16 [n_teams] model indices, confederations (or null)
    const uint8_t* team_host;                         // HOST u8 [n_teams] or null
    int32_t n_groups;
    const uint8_t* team_group;                        // HOST u8 [n_teams] (with groups)
    const int32_t *init_points, *init_gf, *init_ga;   // HOST i32 [n_teams] (with groups)
    int64_t n_fixtures;
    const uint8_t *fix_p, *fix_q;                     // HOST u8 [n_fixtures] slots in the listed order
    int32_t advance, best_of_rest, n_bracket;
    const uint16_t* bracket;                          // HOST u16 [n_bracket]
    int32_t win, draw, loss;
    int64_t n_sims;
    uint32_t key_hi, key_lo;
    void* stream;
    H2HRequest h2h;
};
// what simulate_tournament and tournament_paths return of every slot
struct TournamentOut {
    uint64_t* stage_counts;            // HOST u64 [n, R + 2]
    uint64_t* group_position_counts;   // HOST u64 [n, 8] (required with groups)
    uint8_t* sim_stage;                // u8 [n_sims, n] or null
};
// the knockout-rule checks, the same for every entry
static int knockout_check(bplhip_ctx* c, const KnockoutRequest& ko, int n, int rounds) {
    if (ko.legs_mask >> rounds)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: legs_mask=0x%x has a bit at or above R=%d", ko.legs_mask, rounds);
    if (!(ko.scale > 0.0 && ko.scale <= 1.0))
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: extra_time_scale=%g outside (0,1]", ko.scale);
    if (ko.away_goals != 0 && ko.away_goals != 1)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: away_goals is 0 / 1");
    for (int i = 0; ko.strength && i < n; ++i)
        if (!(std::fabs(ko.strength[i]) <= BPLHIP_TOURNAMENT_MAX_STRENGTH))
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: strength of slot %d is not finite or beyond %d", i,
                        BPLHIP_TOURNAMENT_MAX_STRENGTH);
    if (!ko.decided_counts) return fail(c, BPLHIP_EINVAL, "simulate_tournament: null required output");
    return BPLHIP_OK;
}
// every check of bpl/neutral_dixon_coles.py repeated on the host, in one order for all entries (`out`: the entry
// returns TournamentOut; `ko`: the extra-time rule, checked between the run's and the slots' checks), then the slots,
// the bracket, the fixtures and the current table as the kernels read them
struct TournamentSetup {
    int rounds = 0;
    std::vector<uint32_t> info;          // [n]: model index | conf << 16 | host << 24 | group << 25
    std::vector<uint8_t> code_pos;       // [TOURNAMENT_CODES]: bracket position of a qualifier code, 0xFF none
    std::vector<uint8_t> first_round;    // [n_bracket]: the first round's slots without groups
    std::vector<uint16_t> fix;           // [nf]: slot p | slot q << 8
    std::vector<int32_t> init;           // [3, n]: points, GF, GA (empty without groups)
    std::vector<int> size;               // [n_groups]: the groups' sizes
};
static int tournament_setup(bplhip_ctx* c, const TournamentCall& q, const TournamentOut* out, const KnockoutRequest* ko,
                            TournamentSetup* in) {
    using namespace dct;
    if (c->pred_S == 0) return fail(c, BPLHIP_ESTATE, "simulate_tournament: no posterior set");
    if (!c->pred_venue)
        return fail(c, BPLHIP_ESTATE, "simulate_tournament: the posterior was not set with predict_set_posterior_venue");
    const int n = q.n_teams, n_groups = q.n_groups, n_bracket = q.n_bracket, advance = q.advance, best_of_rest = q.best_of_rest;
    if (n < 2 || n > TOURNAMENT_MAX_TEAMS || !q.team_idx)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: n_teams=%d out of range [2,%d] or null", n, TOURNAMENT_MAX_TEAMS);
    if ((c->pred_C > 0) != (q.team_conf != nullptr))
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: team_conf exactly when the posterior has confederations");
    int rounds = 0;
    while (rounds < 7 && (1 << rounds) < n_bracket) ++rounds;
    if (!q.bracket || rounds < 1 || rounds > 6 || (1 << rounds) != n_bracket)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: the bracket must have 2^R entries, 1 <= R <= 6");
    in->rounds = rounds;
    int rc = sim_check_run(c, "simulate_tournament", q.n_sims, q.win, q.draw, q.loss);
    if (rc != BPLHIP_OK) return rc;
    if (out && (!out->stage_counts || (n_groups > 0 && !out->group_position_counts)))
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: null required output");
    if (ko && (rc = knockout_check(c, *ko, n, rounds)) != BPLHIP_OK) return rc;
    std::vector<char> seen(c->pred_T, 0);
    in->info.resize(n);
    for (int i = 0; i < n; ++i) {
        if (q.team_idx[i] >= c->pred_T || seen[q.team_idx[i]])
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: team %d out of range or repeated", (int)q.team_idx[i]);
        seen[q.team_idx[i]] = 1;
        if (q.team_conf && q.team_conf[i] >= c->pred_C)
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: confederation of slot %d out of range", i);
        if (q.team_host && q.team_host[i] > 1) return fail(c, BPLHIP_EINVAL, "simulate_tournament: host flags are 0 / 1");
        in->info[i] = (uint32_t)q.team_idx[i] | ((uint32_t)(q.team_conf ? q.team_conf[i] : 0) << 16) |
                      ((uint32_t)(q.team_host ? q.team_host[i] : 0) << 24);
    }
    in->code_pos.assign(TOURNAMENT_CODES, 0xFF);
    in->first_round.assign(n_bracket, 0);
    if (n_groups == 0 && c->alloc_rows)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: an allocation is set but there are no groups");
    if (n_groups == 0) {
        // knockout only: the bracket lists every slot once
        if (q.n_fixtures != 0 || n_bracket != n)
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: without groups there are no fixtures and n_bracket = n_teams");
        std::vector<char> used(n, 0);
        for (int b = 0; b < n_bracket; ++b) {
            if (q.bracket[b] >= n || used[q.bracket[b]])
                return fail(c, BPLHIP_EINVAL, "simulate_tournament: bracket entry %d is not a fresh slot", b);
            used[q.bracket[b]] = 1;
            in->first_round[b] = (uint8_t)q.bracket[b];
        }
        return BPLHIP_OK;
    }
    if (n_groups < 1 || n_groups > BPLHIP_TOURNAMENT_MAX_GROUPS || !q.team_group || !q.init_points || !q.init_gf || !q.init_ga)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: n_groups=%d out of range [0,%d] or null group table", n_groups,
                    BPLHIP_TOURNAMENT_MAX_GROUPS);
    if (advance < 1 || advance > TOURNAMENT_MAX_GROUP || best_of_rest < 0)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: advance=%d or best_of_rest=%d out of range", advance, best_of_rest);
    std::vector<int>& size = in->size;
    size.assign(n_groups, 0);
    for (int i = 0; i < n; ++i) {
        if (q.team_group[i] >= n_groups) return fail(c, BPLHIP_EINVAL, "simulate_tournament: group of slot %d out of range", i);
        ++size[q.team_group[i]];
        in->info[i] |= (uint32_t)q.team_group[i] << 25;
        for (const int32_t v : {q.init_points[i], q.init_gf[i], q.init_ga[i]})
            if (v < 0 || v > BPLHIP_SEASON_MAX_TABLE_VALUE)
                return fail(c, BPLHIP_EINVAL, "simulate_tournament: table entry of slot %d out of range [0,%d]", i,
                            BPLHIP_SEASON_MAX_TABLE_VALUE);
    }
    int qualifiers = best_of_rest, rest_groups = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (size[g] < 2 || size[g] > TOURNAMENT_MAX_GROUP)
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: group %d has %d teams, not 2..%d", g, size[g],
                        TOURNAMENT_MAX_GROUP);
        qualifiers += std::min(advance, size[g]);
        rest_groups += size[g] > advance ? 1 : 0;
    }
    if (best_of_rest > rest_groups || qualifiers != n_bracket)
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: %d qualifiers for a bracket of %d (best_of_rest=%d)", qualifiers,
                    n_bracket, best_of_rest);
    for (int b = 0; b < n_bracket; ++b) {
        const int hi = q.bracket[b] >> 8, lo = q.bracket[b] & 0xFF;
        int code = -1;
        if (hi == 0xFF) {
            if (lo >= 1 && lo <= best_of_rest) code = 128 + lo - 1;
        } else if (hi < n_groups && lo >= 1 && lo <= std::min(advance, size[hi])) {
            code = TOURNAMENT_MAX_GROUP * hi + lo - 1;
        }
        if (code < 0 || in->code_pos[code] != 0xFF)
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: bracket entry %d (0x%04x) unresolvable or repeated", b,
                        (unsigned)q.bracket[b]);
        in->code_pos[code] = (uint8_t)b;
    }
    if (c->alloc_rows) {
        // the allocation in force was set for this shape, and has a row for every set of best_of_rest groups with a
        // place advance + 1: the kernels index the tables with nothing else
        if (c->alloc_groups != n_groups || c->alloc_best != best_of_rest)
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: the allocation was set for %d groups and best_of_rest=%d, not %d and %d",
                        c->alloc_groups, c->alloc_best, n_groups, best_of_rest);
        uint32_t eligible = 0u;
        for (int g = 0; g < n_groups; ++g) eligible |= size[g] > advance ? 1u << g : 0u;
        for (uint32_t m = 0; m < (1u << n_groups); ++m) {
            if ((m & ~eligible) || __builtin_popcount(m) != best_of_rest) continue;
            const uint8_t* row = &c->alloc_slot[(size_t)c->alloc_row[m] * n_groups];
            for (int g = 0; g < n_groups; ++g)
                if (((m >> g) & 1u) != (row[g] != 0xFF ? 1u : 0u))
                    return fail(c, BPLHIP_EINVAL, "simulate_tournament: the allocation has no row for the groups 0x%x", m);
        }
    }
    if (q.n_fixtures < 0 || q.n_fixtures > BPLHIP_SEASON_MAX_FIXTURES || (q.n_fixtures > 0 && (!q.fix_p || !q.fix_q)))
        return fail(c, BPLHIP_EINVAL, "simulate_tournament: bad fixtures (n_fixtures=%lld)", (long long)q.n_fixtures);
    in->fix.resize((size_t)q.n_fixtures);
    for (size_t f = 0; f < in->fix.size(); ++f) {
        const int p = q.fix_p[f], o = q.fix_q[f];
        if (p >= n || o >= n || p == o || q.team_group[p] != q.team_group[o])
            return fail(c, BPLHIP_EINVAL, "simulate_tournament: fixture %zu is not two slots of one group", f);
        in->fix[f] = (uint16_t)(p | (o << 8));
    }
    in->init.resize(3 * (size_t)n);
    std::copy(q.init_points, q.init_points + n, in->init.begin());
    std::copy(q.init_gf, q.init_gf + n, in->init.begin() + n);
    std::copy(q.init_ga, q.init_ga + n, in->init.begin() + 2 * n);
    return BPLHIP_OK;
}

// what every entry of the family does between its own checks and its own kernels.  tournament_begin is an entry's last
// check (the pair records); it selects the device and carves the sections every workspace starts with: stage counts
// u64 [n, STAGES], position counts u64 [n, MAX_GROUP], slot info u32 [n], fixtures u16 [nf], table i32 [3, n], code
// positions u8 [CODES], first round u8 [nb], stages u8 [n_sims, n] when `out` asks; with the extra-time rule also
// decided counts u64 [6, 4], strengths f64 [n] and, beside `out`, decided u8 [n_sims, nb - 1] when asked.  The entry
// carves its own region from `cv` after that, and tournament_stage follows
struct TournamentStage {
    hipStream_t s = nullptr;
    bool pair_any = false;   // pair_init has an entry to upload
    bool want_stage = false, want_decided = false;   // the kernels fill sim_stage / sim_decided rows
    Carver cv;
    size_t o_pos = 0, o_info = 0, o_fix = 0, o_init = 0, o_code = 0, o_first = 0, o_stage = 0, o_dec = 0, o_str = 0, o_sdec = 0;
    size_t o_alloc = 0;   // the allocation block: slot counts, row_of_mask, slots (empty without a table)
    std::vector<double> strength;   // (outlives the asynchronous upload: the call synchronises before it returns)
    char* base = nullptr;           // the carved workspace
    dch::PairArgs H{};
    dct::TournamentArgs A{};
    dck::KnockoutArgs K{};
};
constexpr size_t ALLOC_BYTES = dct::ALLOC_COUNT_BYTES;   // the allocation block's slot counts
constexpr size_t DECIDED_BYTES = (size_t)dck::KNOCKOUT_MAX_ROUNDS * dck::DECIDED_KINDS * 8;
static_assert(dct::TOURNAMENT_MAX_GROUPS == BPLHIP_TOURNAMENT_MAX_GROUPS, "the slot counts are [groups, groups]");
static int tournament_begin(bplhip_ctx* c, const TournamentCall& q, const TournamentSetup& in, const TournamentOut* out,
                            const KnockoutRequest* ko, TournamentStage* st) {
    using namespace dct;
    const size_t n = (size_t)q.n_teams, ns = (size_t)q.n_sims;
    if (q.h2h.on) {
        const int rc = h2h_check(c, "simulate_tournament", q.n_teams, pair_meetings(in.fix, q.n_teams), q.win, q.draw, q.loss,
                                 q.h2h.pair_init, &st->pair_any);
        if (rc != BPLHIP_OK) return rc;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    st->s = static_cast<hipStream_t>(q.stream);
    Carver& cv = st->cv;
    cv.take(n * TOURNAMENT_STAGES * 8);
    st->o_pos = cv.take(n * TOURNAMENT_MAX_GROUP * 8), st->o_info = cv.take(n * 4), st->o_fix = cv.take(in.fix.size() * 2),
    st->o_init = cv.take(in.init.size() * 4), st->o_code = cv.take(TOURNAMENT_CODES), st->o_first = cv.take((size_t)q.n_bracket),
    // (before the per-simulation sections: the kernels reach the block by a 32-bit offset from the fixtures)
    st->o_alloc = cv.take(c->alloc_rows ? ALLOC_BYTES + c->alloc_row.size() * 2 + c->alloc_slot.size() : 0);
    st->want_stage = out && out->sim_stage;
    st->want_decided = out && ko && ko->sim_decided;
    st->o_stage = cv.take(st->want_stage ? ns * n : 0);
    st->o_dec = cv.take(ko ? DECIDED_BYTES : 0), st->o_str = cv.take(ko ? n * 8 : 0),
    st->o_sdec = cv.take(st->want_decided ? ns * (size_t)(q.n_bracket - 1) : 0);
    return BPLHIP_OK;
}
// places the pair matrix after the entry's sections and sizes the workspace, zeroes the counts, uploads slot info,
// fixtures, table, codes, first round and strengths, and fills TournamentArgs and KnockoutArgs (sim_stage and
// sim_decided stay null where tournament_begin had no `out`)
static int tournament_stage(bplhip_ctx* c, const TournamentCall& q, const TournamentSetup& in, const KnockoutRequest* ko,
                            TournamentStage& st) {
    using namespace dct;
    const int n = q.n_teams;
    const int rc = pair_place(c, st.cv, c->dp_tournament, q.h2h, st.pair_any, n, st.s, &st.H);
    if (rc != BPLHIP_OK) return rc;
    const size_t nf = in.fix.size();
    char* base = st.base = c->dp_tournament.as<char>();
    hipStream_t s = st.s;
    HIP_TRY(c, hipMemsetAsync(base, 0, st.o_info, s));
    HIP_TRY(c, hipMemcpyAsync(base + st.o_info, in.info.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (nf) HIP_TRY(c, hipMemcpyAsync(base + st.o_fix, in.fix.data(), nf * 2, hipMemcpyHostToDevice, s));
    if (!in.init.empty())
        HIP_TRY(c, hipMemcpyAsync(base + st.o_init, in.init.data(), in.init.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(base + st.o_code, in.code_pos.data(), TOURNAMENT_CODES, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(base + st.o_first, in.first_round.data(), (size_t)q.n_bracket, hipMemcpyHostToDevice, s));
    dck::KnockoutArgs& K = st.K;
    if (ko) {
        st.strength.assign(n, 0.0);
        if (ko->strength) std::copy(ko->strength, ko->strength + n, st.strength.begin());
        HIP_TRY(c, hipMemsetAsync(base + st.o_dec, 0, DECIDED_BYTES, s));
        HIP_TRY(c, hipMemcpyAsync(base + st.o_str, st.strength.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
        K.legs_mask = ko->legs_mask;
        K.away_goals = ko->away_goals;
        K.scale = ko->scale;
        K.strength = reinterpret_cast<const double*>(base + st.o_str);
        K.decided_counts = reinterpret_cast<unsigned long long*>(base + st.o_dec);
        K.sim_decided = st.want_decided ? reinterpret_cast<uint8_t*>(base + st.o_sdec) : nullptr;
    }
    TournamentArgs& A = st.A;
    A.S = c->pred_S;
    A.T = c->pred_T;
    A.C = c->pred_C;
    A.n = n;
    A.nf = (int)nf;
    A.n_groups = q.n_groups;
    A.advance = q.advance;
    A.rounds = in.rounds;
    A.n_sims = q.n_sims;
    A.key_hi = q.key_hi;
    A.key_lo = q.key_lo;
    A.win = q.win;
    A.draw = q.draw;
    A.loss = q.loss;
    A.attack = c->dp_tab[PT_ATT].as<const double>();
    A.defence = c->dp_tab[PT_DEF].as<const double>();
    A.home_attack = c->dp_tab[PT_HAT].as<const double>();
    A.away_attack = c->dp_tab[PT_AAT].as<const double>();
    A.home_defence = c->dp_tab[PT_HDF].as<const double>();
    A.away_defence = c->dp_tab[PT_ADF].as<const double>();
    A.conf = c->pred_C ? c->dp_tab[PT_CONF].as<const double>() : nullptr;
    A.corr = c->dp_corr.as<const double>();
    A.slot_info = reinterpret_cast<const uint32_t*>(base + st.o_info);
    A.fix = reinterpret_cast<const uint16_t*>(base + st.o_fix);
    A.init = reinterpret_cast<const int32_t*>(base + st.o_init);
    A.code_pos = reinterpret_cast<const uint8_t*>(base + st.o_code);
    A.first_round = reinterpret_cast<const uint8_t*>(base + st.o_first);
    A.stage_counts = reinterpret_cast<unsigned long long*>(base);
    A.pos_counts = reinterpret_cast<unsigned long long*>(base + st.o_pos);
    A.sim_stage = st.want_stage ? reinterpret_cast<uint8_t*>(base + st.o_stage) : nullptr;
    if (c->alloc_rows) {
        char* blk = base + st.o_alloc;
        HIP_TRY(c, hipMemsetAsync(blk, 0, ALLOC_BYTES, s));
        HIP_TRY(c, hipMemcpyAsync(blk + ALLOC_BYTES, c->alloc_row.data(), c->alloc_row.size() * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(blk + ALLOC_BYTES + c->alloc_row.size() * 2, c->alloc_slot.data(), c->alloc_slot.size(),
                                  hipMemcpyHostToDevice, s));
        A.alloc_off = (uint32_t)(st.o_alloc - st.o_fix);
    }
    return BPLHIP_OK;
}
constexpr int SIM_BLOCKS_PER_CU = 4;   // workgroups per CU of the recording kernels in the overall order
// one chunk of a recording kernel: the four <H2H, ET> instantiations as kernels[H2H][ET]
template <class P>
using TournamentSimKernel = void (*)(dct::TournamentArgs, dch::PairArgs, dck::KnockoutArgs, P);
template <class P>
static int tournament_sim_launch(bplhip_ctx* c, const TournamentCall& q, const TournamentStage& st, bool et,
                                 TournamentSimKernel<P> const (&kernels)[2][2][2], const P& p) {
    const SimLaunch L = sim_launch(c, q.h2h, q.n_teams, p.nc, dct::SIM_WAVES, SIM_BLOCKS_PER_CU);
    // (st.A.alloc_off: a best-of-rest allocation table is staged; its kernels are the same text with ALLOC set)
    hipLaunchKernelGGL(kernels[st.A.alloc_off != 0][q.h2h.on][et], L.grid, L.block, L.lds, st.s, st.A, st.H, st.K, p);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
#define TOURNAMENT_SIM_KERNELS(P, kernel, alloc_kernel) \
    static constexpr TournamentSimKernel<P> kernels[2][2][2] = { \
        {{kernel<false, false>, kernel<false, true>}, {kernel<true, false>, kernel<true, true>}}, \
        {{alloc_kernel<false, false>, alloc_kernel<false, true>}, {alloc_kernel<true, false>, alloc_kernel<true, true>}}}
static_assert(dcpath::PATHS_BLOCKS_PER_CU == SIM_BLOCKS_PER_CU && dcts::TSCEN_BLOCKS_PER_CU == SIM_BLOCKS_PER_CU &&
              dcgq::GPTS_BLOCKS_PER_CU == SIM_BLOCKS_PER_CU, "one launch shape for the recording kernels");
// how the knockout matches were decided, [R, 4] of the workspace's [6, 4] (queued on the stream)
static int tournament_decided(bplhip_ctx* c, const KnockoutRequest* ko, const TournamentStage& st) {
    if (ko)
        HIP_TRY(c, hipMemcpyAsync(ko->decided_counts, st.base + st.o_dec, (size_t)st.A.rounds * dck::DECIDED_KINDS * 8,
                                  hipMemcpyDeviceToHost, st.s));
    return BPLHIP_OK;
}

// ---- simulate_tournament (dc_tournament.hip.h): the live request, the state words and the simulator kernels
// what bplhip_simulate_tournament_live adds (dc_tournament_live.hip.h): the season's live request with the two sides
// of a match in play as SLOTS in the listed order, and the final scores of those matches in that order
struct CupLiveRequest {
    LiveRequest rq;                        // (rq.in.home_idx / away_idx stay null)
    const uint8_t *side_p, *side_q;        // HOST u8 [n_in_play] slots in the listed order
    uint8_t *final_home, *final_away;      // u8 [n_sims, n_in_play] or null
};
// the states as live_cup_loglik reads them: the venue decided from the host bits as dct::play decides it, the sides'
// model indices and confederations and the score in the home / away orientation
struct CupStateWords {
    std::vector<uint32_t> side, state, conf;
};
static CupStateWords cup_state_words(const TournamentSetup& in, const CupLiveRequest& lr) {
    const size_t L = (size_t)lr.rq.in.n_in_play;
    CupStateWords w{std::vector<uint32_t>(L), std::vector<uint32_t>(L), std::vector<uint32_t>(L)};
    for (size_t m = 0; m < L; ++m) {
        const uint32_t ip = in.info[lr.side_p[m]], iq = in.info[lr.side_q[m]];
        const bool hp = (ip >> 24) & 1u, hq = (iq >> 24) & 1u, swap = hq && !hp;
        const uint32_t ih = swap ? iq : ip, ia = swap ? ip : iq;
        const uint32_t gp = lr.rq.in.home_goals[m], gq = lr.rq.in.away_goals[m];
        w.side[m] = (ih & 0xFFFFu) | ((ia & 0xFFFFu) << 16);
        w.state[m] = (swap ? gq : gp) | ((swap ? gp : gq) << 8) | ((hp != hq ? 1u : 0u) << 16);
        w.conf[m] = ((ih >> 16) & 0xFFu) | (((ia >> 16) & 0xFFu) << 16);
    }
    return w;
}
// the simulator of a call: the kick-off kernels by tie-break, knockout rule and allocation table (ALLOC: the same body
// under a best-of-rest table), and their LIVE twins of dc_tournament_live.hip.h with the live block
static int cup_launch(bplhip_ctx* c, const TournamentCall& q, const TournamentStage& st, bool et, const SimLaunch& L) {
    using namespace dct;
    hipStream_t s = st.s;
    if (st.A.alloc_off) {
        if (et && q.h2h.on) hipLaunchKernelGGL(cup_alloc_et<true>, L.grid, L.block, L.lds, s, st.A, st.H, st.K);
        else if (et) hipLaunchKernelGGL(cup_alloc_et<false>, L.grid, L.block, L.lds, s, st.A, st.H, st.K);
        else if (q.h2h.on) hipLaunchKernelGGL(cup_alloc<true>, L.grid, L.block, L.lds, s, st.A, st.H);
        else hipLaunchKernelGGL(cup_alloc<false>, L.grid, L.block, L.lds, s, st.A, st.H);
    } else if (et && q.h2h.on) hipLaunchKernelGGL(dc_tournament_et<true>, L.grid, L.block, L.lds, s, st.A, st.H, st.K);
    else if (et) hipLaunchKernelGGL(dc_tournament_et<false>, L.grid, L.block, L.lds, s, st.A, st.H, st.K);
    else if (q.h2h.on) hipLaunchKernelGGL(dc_tournament<true>, L.grid, L.block, L.lds, s, st.A, st.H);
    else hipLaunchKernelGGL(dc_tournament<false>, L.grid, L.block, L.lds, s, st.A, st.H);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
static int cup_live_launch(bplhip_ctx* c, const TournamentCall& q, const TournamentStage& st, bool et, const SimLaunch& L,
                           const dct::LiveCup& V) {
    using namespace dctl;
    hipStream_t s = st.s;
    if (st.A.alloc_off) {
        if (et && q.h2h.on) hipLaunchKernelGGL(live_cup_table_et<true>, L.grid, L.block, L.lds, s, st.A, st.H, st.K, V);
        else if (et) hipLaunchKernelGGL(live_cup_table_et<false>, L.grid, L.block, L.lds, s, st.A, st.H, st.K, V);
        else if (q.h2h.on) hipLaunchKernelGGL(live_cup_table<true>, L.grid, L.block, L.lds, s, st.A, st.H, V);
        else hipLaunchKernelGGL(live_cup_table<false>, L.grid, L.block, L.lds, s, st.A, st.H, V);
    } else if (et && q.h2h.on) hipLaunchKernelGGL(live_cup_et<true>, L.grid, L.block, L.lds, s, st.A, st.H, st.K, V);
    else if (et) hipLaunchKernelGGL(live_cup_et<false>, L.grid, L.block, L.lds, s, st.A, st.H, st.K, V);
    else if (q.h2h.on) hipLaunchKernelGGL(live_cup<true>, L.grid, L.block, L.lds, s, st.A, st.H, V);
    else hipLaunchKernelGGL(live_cup<false>, L.grid, L.block, L.lds, s, st.A, st.H, V);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
// ---- the live form of simulate_tournament (dc_tournament_live.hip.h) and of tournament_paths, tournament_scenarios
// and tournament_points (dc_tournament_live_queries.hip.h): what an entry does with a CupLiveRequest around its own
// steps, in one order for all four -- the lists checked and concatenated before tournament_setup, the log weights after
// the entry's own checks (live_weights_check), the live sections carved after the entry's own, after tournament_stage
// the states uploaded and the two weight kernels run, once per call, and the draws, the final scores and the weights'
// figures read back.  Without a request (the kick-off entries) every step is empty and `q` is the caller's call.  The
// season family's twin is SeasonLive
struct CupLiveQuery {
    const CupLiveRequest* lr = nullptr;
    const LiveIn* lv = nullptr;          // the request's inputs (lr->rq.in)
    TournamentCall q{};                  // the call over the concatenated list
    std::vector<uint8_t> cat_p, cat_q;   // that list
    size_t F = 0, L = 0;                 // the fixtures still to kick off, the matches in play
    LivePlan P;
    // the live sections after live_plan's: the states u32 [3, L], the draws i32 [n_sims], the finals u8 [2, n_sims, L]
    size_t o_words = 0, o_draw = 0, o_final = 0;
    CupStateWords words;                 // (outlives the upload: the call synchronises)
    bool kernels = false;                // weights are in force or a match is in play: the dctq kernels record
    dct::LiveCup V{};
};
static int cup_query_lists(bplhip_ctx* c, const char* what, const TournamentCall& q0, const CupLiveRequest* lr,
                           CupLiveQuery* X) {
    X->lr = lr;
    X->q = q0;
    if (!lr) return BPLHIP_OK;
    const LiveIn& lv = lr->rq.in;
    X->lv = &lv;
    const int rc = live_check_lists(c, what, q0.n_fixtures, q0.fix_p && q0.fix_q, lr->side_p && lr->side_q, lv,
                                    BPLHIP_SEASON_MAX_FIXTURES);
    if (rc != BPLHIP_OK) return rc;
    const size_t F = X->F = (size_t)q0.n_fixtures, Lm = X->L = (size_t)lv.n_in_play;
    if (Lm > 0 && q0.n_groups <= 0) return fail(c, BPLHIP_EINVAL, "%s: n_in_play=%lld without groups", what, (long long)Lm);
    if ((lr->final_home != nullptr) != (lr->final_away != nullptr))
        return fail(c, BPLHIP_EINVAL, "%s: the final scores come as a pair", what);
    X->cat_p.assign(q0.fix_p, q0.fix_p + F);
    X->cat_q.assign(q0.fix_q, q0.fix_q + F);
    X->cat_p.insert(X->cat_p.end(), lr->side_p, lr->side_p + Lm);
    X->cat_q.insert(X->cat_q.end(), lr->side_q, lr->side_q + Lm);
    X->q.n_fixtures = (int64_t)(F + Lm);
    X->q.fix_p = X->cat_p.data();
    X->q.fix_q = X->cat_q.data();
    return BPLHIP_OK;
}
// after tournament_begin and the entry's own carve
static int cup_query_plan(bplhip_ctx* c, TournamentStage& st, CupLiveQuery& X) {
    if (!X.lr) return BPLHIP_OK;
    const int rc = live_plan(c, st.s, st.cv, X.lr->rq.in, &X.P);
    if (rc != BPLHIP_OK) return rc;
    const size_t ns = (size_t)X.q.n_sims;
    X.o_words = st.cv.take(X.P.weighted ? 3 * X.L * 4 : 0);
    X.o_draw = st.cv.take(X.lr->rq.sim_draw ? ns * 4 : 0);
    X.o_final = st.cv.take(X.lr->final_home ? 2 * ns * X.L : 0);
    X.kernels = X.P.weighted || X.L > 0;
    return BPLHIP_OK;
}
// after tournament_stage: the ordinary loop's fixture count, the states, the weights, the kernels' live block
static int cup_query_stage(bplhip_ctx* c, const TournamentSetup& in, TournamentStage& st, CupLiveQuery& X) {
    if (!X.lr) return BPLHIP_OK;
    const LiveIn& lv = X.lr->rq.in;
    const LivePlan& P = X.P;
    char* base = st.base;
    hipStream_t s = st.s;
    const size_t Lm = X.L, ns = (size_t)X.q.n_sims;
    st.A.nf = (int)X.F;   // the ordinary fixtures; those in play follow them in A.fix
    int rc = live_upload(c, s, base, lv, P);
    if (rc != BPLHIP_OK) return rc;
    X.words = cup_state_words(in, *X.lr);
    if (P.weighted) {
        uint32_t* dw = reinterpret_cast<uint32_t*>(base + X.o_words);
        if (Lm) {
            HIP_TRY(c, hipMemcpyAsync(dw, X.words.side.data(), Lm * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(dw + Lm, X.words.state.data(), Lm * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(c, hipMemcpyAsync(dw + 2 * Lm, X.words.conf.data(), Lm * 4, hipMemcpyHostToDevice, s));
        }
        const dclive::LiveArgs W = live_args(c, base, lv, P);
        const dcq::Posterior<double> T = posterior_view(c, true);
        dctl::CupStates G{};
        G.S = W.S, G.L = W.L, G.C = T.C, G.reweight = W.reweight;
        G.attack = T.attack, G.defence = T.defence, G.home_attack = T.home_attack, G.away_attack = T.away_attack;
        G.home_defence = T.home_defence, G.away_defence = T.away_defence, G.conf = T.conf, G.corr = T.corr;
        G.st_side = dw, G.st_state = dw + Lm, G.st_conf = dw + 2 * Lm, G.st_t = W.st_t;
        G.lw = W.lw, G.Lw = W.Lw, G.L0 = W.L0;
        std::copy(std::begin(W.lgf), std::end(W.lgf), std::begin(G.lgf));
        const dim3 block(dclive::LIVE_THREADS);
        hipLaunchKernelGGL(dctl::live_cup_loglik, live_grid(c), block, 0, s, G);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(dclive::live_weights, dim3(1), block, 0, s, W);
        HIP_TRY(c, hipGetLastError());
    }
    dct::LiveCup& V = X.V;
    V.F = (int)X.F, V.L = (int)Lm;
    V.st_goals = reinterpret_cast<const uint32_t*>(base + P.o_stg);
    V.st_t = reinterpret_cast<const double*>(base + P.o_stt);
    V.C = P.weighted ? reinterpret_cast<const double*>(base + P.o_C) : nullptr;
    V.sim_draw = X.lr->rq.sim_draw ? reinterpret_cast<int32_t*>(base + X.o_draw) : nullptr;
    V.final_home = X.lr->final_home ? reinterpret_cast<uint8_t*>(base + X.o_final) : nullptr;
    V.final_away = X.lr->final_home ? V.final_home + ns * Lm : nullptr;
    return BPLHIP_OK;
}
// after the last chunk: the draws, the final scores and the weights' figures queued; cup_query_finish after the
// stream is synchronised
static int cup_query_read(bplhip_ctx* c, const TournamentStage& st, CupLiveQuery& X) {
    if (!X.lr) return BPLHIP_OK;
    const CupLiveRequest& lr = *X.lr;
    const size_t ns = (size_t)X.q.n_sims, Lm = X.L, S = (size_t)c->pred_S;
    const char* base = st.base;
    if (X.kernels) {
        if (lr.rq.sim_draw)
            HIP_TRY(c, hipMemcpyAsync(lr.rq.sim_draw, base + X.o_draw, ns * 4, hipMemcpyDeviceToHost, st.s));
        if (lr.final_home && Lm) {
            HIP_TRY(c, hipMemcpyAsync(lr.final_home, base + X.o_final, ns * Lm, hipMemcpyDeviceToHost, st.s));
            HIP_TRY(c, hipMemcpyAsync(lr.final_away, base + X.o_final + ns * Lm, ns * Lm, hipMemcpyDeviceToHost, st.s));
        }
    } else if (lr.rq.sim_draw) {
        for (size_t j = 0; j < ns; ++j) lr.rq.sim_draw[j] = (int32_t)(j % S);   // (no weights: the kick-off kernels)
    }
    const int rc = live_read(c, st.s, base, X.P);
    return rc != BPLHIP_OK ? rc : live_read_draws(c, st.s, base, lr.rq, X.P);
}
static void cup_query_finish(const CupLiveQuery& X) {
    if (X.lr) live_finish(X.lr->rq.in, X.P);
}

// ---- simulate_tournament (dc_tournament.hip.h)
// `lr` (bplhip_simulate_tournament_live): `q0` lists the fixtures still to kick off, the group fixtures are the
// concatenated list, the draws may carry weights and the simulator is one of dctl's when weights are in force or a
// match is in play; null: the kick-off call, as it was before the live form existed
static int simulate_tournament_impl(bplhip_ctx* c, const TournamentCall& q0, const TournamentOut& out,
                                    const KnockoutRequest* ko = nullptr, uint64_t* slot_counts = nullptr,
                                    const CupLiveRequest* lr = nullptr) {
    using namespace dct;
    if (!c) return BPLHIP_EINVAL;
    const char* what = "simulate_tournament_live";
    if (!lr && slot_counts && !c->alloc_rows)
        return fail(c, BPLHIP_ESTATE, "simulate_tournament: slot_counts without an allocation set");
    if (lr && !c->alloc_rows) slot_counts = nullptr;   // (this entry serves both cases)
    CupLiveQuery X;
    int rc = cup_query_lists(c, what, q0, lr, &X);
    if (rc != BPLHIP_OK) return rc;
    const TournamentCall& q = X.q;
    TournamentSetup in;
    rc = tournament_setup(c, q, &out, ko, &in);
    if (rc != BPLHIP_OK) return rc;
    if ((rc = live_weights_check(c, what, X.lv)) != BPLHIP_OK) return rc;
    TournamentStage st;   // (the matches in play are meetings to come like any fixture)
    if ((rc = tournament_begin(c, q, in, &out, ko, &st)) != BPLHIP_OK) return rc;
    const int n = q.n_teams, rounds = in.rounds;
    const size_t ns = (size_t)q.n_sims;
    if ((rc = cup_query_plan(c, st, X)) != BPLHIP_OK) return rc;
    if ((rc = tournament_stage(c, q, in, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_stage(c, in, st, X)) != BPLHIP_OK) return rc;
    hipStream_t s = st.s;
    const SimLaunch L = sim_launch(c, q.h2h, n, q.n_sims, TOURNAMENT_WAVES, TOURNAMENT_BLOCKS_PER_CU);
    // (a live call with weights in force or a match in play launches its dctl kernel in the kick-off kernel's place)
    rc = X.kernels ? cup_live_launch(c, q, st, ko != nullptr, L, X.V) : cup_launch(c, q, st, ko != nullptr, L);
    if (rc != BPLHIP_OK) return rc;
    // stage counts come back as [n, R + 2], position counts as [n, MAX_GROUP]
    std::vector<uint64_t> sc((size_t)n * TOURNAMENT_STAGES);
    HIP_TRY(c, hipMemcpyAsync(sc.data(), st.base, sc.size() * 8, hipMemcpyDeviceToHost, s));
    if (q.n_groups > 0)
        HIP_TRY(c, hipMemcpyAsync(out.group_position_counts, st.base + st.o_pos, (size_t)n * TOURNAMENT_MAX_GROUP * 8,
                                  hipMemcpyDeviceToHost, s));
    if (out.sim_stage) HIP_TRY(c, hipMemcpyAsync(out.sim_stage, st.base + st.o_stage, ns * n, hipMemcpyDeviceToHost, s));
    if ((rc = tournament_decided(c, ko, st)) != BPLHIP_OK) return rc;
    if (st.want_decided)
        HIP_TRY(c, hipMemcpyAsync(ko->sim_decided, st.base + st.o_sdec, ns * (size_t)(q.n_bracket - 1), hipMemcpyDeviceToHost,
                                  s));
    std::vector<uint64_t> ac(slot_counts ? ALLOC_BYTES / 8 : 0);
    if (slot_counts) HIP_TRY(c, hipMemcpyAsync(ac.data(), st.base + st.o_alloc, ALLOC_BYTES, hipMemcpyDeviceToHost, s));
    if ((rc = cup_query_read(c, st, X)) != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    cup_query_finish(X);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < rounds + 2; ++k)
            out.stage_counts[(size_t)i * (rounds + 2) + k] = sc[(size_t)i * TOURNAMENT_STAGES + k];
    // the slot counts come back as [n_groups, best_of_rest] of the block's [16, 16]
    for (int g = 0; slot_counts && g < q.n_groups; ++g)
        for (int k = 0; k < q.best_of_rest; ++k)
            slot_counts[(size_t)g * q.best_of_rest + k] = ac[(size_t)g * TOURNAMENT_MAX_GROUPS + k];
    return BPLHIP_OK;
}
// one chunk of a LIVE recording kernel, as tournament_sim_launch: kernels[ALLOC][H2H][ET]
template <class P>
using TournamentLiveKernel = void (*)(dct::TournamentArgs, dch::PairArgs, dck::KnockoutArgs, P, dct::LiveCup);
template <class P>
static int tournament_live_launch(bplhip_ctx* c, const TournamentCall& q, const TournamentStage& st, bool et,
                                  TournamentLiveKernel<P> const (&kernels)[2][2][2], const P& p, const dct::LiveCup& V) {
    const SimLaunch L = sim_launch(c, q.h2h, q.n_teams, p.nc, dct::SIM_WAVES, SIM_BLOCKS_PER_CU);
    hipLaunchKernelGGL(kernels[st.A.alloc_off != 0][q.h2h.on][et], L.grid, L.block, L.lds, st.s, st.A, st.H, st.K, p, V);
    HIP_TRY(c, hipGetLastError());
    return BPLHIP_OK;
}
#define TOURNAMENT_LIVE_KERNELS(P, kernel, table_kernel) \
    static constexpr TournamentLiveKernel<P> live_kernels[2][2][2] = { \
        {{kernel<false, false>, kernel<false, true>}, {kernel<true, false>, kernel<true, true>}}, \
        {{table_kernel<false, false>, table_kernel<false, true>}, {table_kernel<true, false>, table_kernel<true, true>}}}

// ---- tournament_paths (dc_paths.hip.h): sim_stage and the extra-time rule's sim_decided are filled chunk by chunk
// from the records, as the request's own per-simulation arrays
// `lr` (bplhip_tournament_paths_live): as in simulate_tournament_impl; null: the kick-off call
static int tournament_paths_impl(bplhip_ctx* c, const TournamentCall& q0, const TournamentOut& out,
                                 const KnockoutRequest* ko, const PathsRequest& paths,
                                 const CupLiveRequest* lr = nullptr) {
    using namespace dct;
    if (!c) return BPLHIP_EINVAL;
    CupLiveQuery X;
    int rc = cup_query_lists(c, "tournament_paths_live", q0, lr, &X);
    if (rc != BPLHIP_OK) return rc;
    const TournamentCall& q = X.q;
    TournamentSetup in;
    rc = tournament_setup(c, q, &out, ko, &in);
    if (rc != BPLHIP_OK) return rc;
    const size_t nf = in.fix.size();
    if (paths.chunk_sims < 0)
        return fail(c, BPLHIP_EINVAL, "tournament_paths: chunk_sims=%lld is negative", (long long)paths.chunk_sims);
    if (nf > BPLHIP_LEVERAGE_MAX_FIXTURES)
        return fail(c, BPLHIP_EINVAL, "tournament_paths: at most %d group fixtures", BPLHIP_LEVERAGE_MAX_FIXTURES);
    if (!paths.advance_counts || (q.n_groups > 0 && !paths.position_stage_counts) ||
        (nf && (!paths.outcome_counts || !paths.target_counts || !paths.joint_counts)))
        return fail(c, BPLHIP_EINVAL, "tournament_paths: null required output");
    if ((rc = live_weights_check(c, "tournament_paths_live", X.lv)) != BPLHIP_OK) return rc;
    TournamentStage st;
    if ((rc = tournament_begin(c, q, in, nullptr, ko, &st)) != BPLHIP_OK) return rc;
    // the count tables advance u64 [R, n, n], position x stage u64 [n, 8, 8], joint u64 [nf, 3, n, K], outcome u64
    // [nf, 3] (zeroed together), then the chunk's records: ballots (16-byte records), target sets u8 [chunk, n], slot
    // bytes u8 [chunk, n], matches u32 [chunk, nb - 1]
    const int n = q.n_teams, rounds = in.rounds;
    const int64_t n_sims = q.n_sims;
    const size_t nm = (size_t)q.n_bracket - 1, blocks = (nf + 63) / 64, PK = (size_t)rounds + 1;
    const size_t chunk = chunk_for(paths.chunk_sims, blocks * 16 + 2 * (size_t)n + 4 * nm, n_sims);
    const size_t adv_bytes = (size_t)rounds * n * n * 8, ps_bytes = (size_t)n * TOURNAMENT_MAX_GROUP * TOURNAMENT_STAGES * 8,
                 joint_bytes = nf * 3 * (size_t)n * PK * 8;
    Carver& cv = st.cv;
    const size_t o_adv = cv.take(adv_bytes), o_ps = cv.take(ps_bytes), o_joint = cv.take(joint_bytes),
                 o_out = cv.take(nf * 3 * 8), tables_end = cv.total;
    cv.total = (cv.total + 15) & ~(size_t)15;
    const size_t o_ball = cv.take(blocks * chunk * 16), o_tset = cv.take(chunk * n), o_slot = cv.take(chunk * n),
                 o_match = cv.take(chunk * nm * 4);
    if ((rc = cup_query_plan(c, st, X)) != BPLHIP_OK) return rc;
    if ((rc = tournament_stage(c, q, in, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_stage(c, in, st, X)) != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    HIP_TRY(c, hipMemsetAsync(base + o_adv, 0, tables_end - o_adv, s));
    dcpath::PathsArgs P{};
    P.chunk = (int)chunk;
    P.ball = reinterpret_cast<unsigned long long*>(base + o_ball);
    P.tset = reinterpret_cast<uint8_t*>(base + o_tset);
    P.slot = reinterpret_cast<uint8_t*>(base + o_slot);
    P.match = reinterpret_cast<uint32_t*>(base + o_match);
    P.advance = reinterpret_cast<unsigned long long*>(base + o_adv);
    P.pos_stage = reinterpret_cast<unsigned long long*>(base + o_ps);
    dclev::LeverageArgs V{};   // what dc_leverage_count reads: the shape, the chunk's records and its two tables
    V.n = n;
    V.nf = (int)nf;
    V.K = (int)PK;
    V.chunk = (int)chunk;
    V.ball = P.ball;
    V.tset = P.tset;
    V.outcome = reinterpret_cast<unsigned long long*>(base + o_out);
    V.joint = reinterpret_cast<unsigned long long*>(base + o_joint);
    V.slots_per_tile = dclev::COUNT_COLS / (int)PK;
    const unsigned tiles = (unsigned)((n + V.slots_per_tile - 1) / V.slots_per_tile);
    uint8_t* sim_decided = ko ? ko->sim_decided : nullptr;
    const bool records = out.sim_stage || paths.sim_position || paths.sim_outcome || paths.sim_pair || paths.sim_winner ||
                         sim_decided;
    std::vector<uint64_t> h_ball(records ? blocks * chunk * 2 : 0);
    std::vector<uint8_t> h_slot(records ? chunk * n : 0);
    std::vector<uint32_t> h_match(records ? chunk * nm : 0);
    TOURNAMENT_SIM_KERNELS(dcpath::PathsArgs, dcpath::dc_paths_sim, dcpath::paths_alloc_sim);
    TOURNAMENT_LIVE_KERNELS(dcpath::PathsArgs, dctq::cup_paths_live, dctq::cup_paths_live_table);
    for (int64_t j0 = 0; j0 < n_sims; j0 += (int64_t)chunk) {
        P.j0 = j0;
        P.nc = V.nc = (int)std::min<int64_t>((int64_t)chunk, n_sims - j0);
        rc = X.kernels ? tournament_live_launch(c, q, st, ko != nullptr, live_kernels, P, X.V)
                       : tournament_sim_launch(c, q, st, ko != nullptr, kernels, P);
        if (rc != BPLHIP_OK) return rc;
        // shares of the chunk: enough workgroups to fill the device, each thread with a simulation of its own
        const long long per = (P.nc + dcpath::PATHS_COUNT_THREADS - 1) / dcpath::PATHS_COUNT_THREADS;
        if (nf) {
            const long long groups_of_4 = ((P.nc + 63) / 64 + dclev::LEVERAGE_WAVES - 1) / dclev::LEVERAGE_WAVES;
            const long long fill = (2ll * c->n_cu + (long long)(blocks * tiles) - 1) / (long long)(blocks * tiles);
            const dim3 cgrid((unsigned)blocks, tiles, (unsigned)std::max(1ll, std::min({groups_of_4, fill, 65535ll})));
            hipLaunchKernelGGL(dclev::dc_leverage_count, cgrid, dim3(64 * dclev::LEVERAGE_WAVES), 0, s, V);
            HIP_TRY(c, hipGetLastError());
        }
        const long long share = (2ll * c->n_cu + rounds) / (rounds + 1);
        const dim3 pgrid((unsigned)(rounds + 1), (unsigned)std::max(1ll, std::min({per, share, 65535ll})));
        hipLaunchKernelGGL(dcpath::dc_paths_count, pgrid, dim3(dcpath::PATHS_COUNT_THREADS), 0, s, P, n, rounds);
        HIP_TRY(c, hipGetLastError());
        if (!records) continue;
        // the chunk's records, unpacked into the caller's per-simulation arrays
        if (nf) HIP_TRY(c, hipMemcpyAsync(h_ball.data(), base + o_ball, blocks * chunk * 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_slot.data(), base + o_slot, (size_t)P.nc * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(h_match.data(), base + o_match, (size_t)P.nc * nm * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for (size_t i = 0; i < (size_t)P.nc; ++i) {
            const size_t j = (size_t)j0 + i;
            for (size_t t = 0; t < (size_t)n; ++t) {
                const uint8_t b = h_slot[i * n + t];
                if (out.sim_stage) out.sim_stage[j * n + t] = b & 7u;
                if (paths.sim_position) paths.sim_position[j * n + t] = b >> 4;
            }
            for (size_t f = 0; paths.sim_outcome && f < nf; ++f) {
                const uint64_t* w = &h_ball[((f >> 6) * chunk + i) * 2];
                paths.sim_outcome[j * nf + f] = (uint8_t)((w[0] >> (f & 63)) & 1u ? 0 : (w[1] >> (f & 63)) & 1u ? 2 : 1);
            }
            for (size_t k = 0; k < nm; ++k) {
                const uint32_t w = h_match[i * nm + k];
                if (paths.sim_pair) {
                    paths.sim_pair[(j * nm + k) * 2] = (uint8_t)w;
                    paths.sim_pair[(j * nm + k) * 2 + 1] = (uint8_t)(w >> 8);
                }
                if (paths.sim_winner) paths.sim_winner[j * nm + k] = (uint8_t)(w >> 16);
                if (sim_decided) sim_decided[j * nm + k] = (uint8_t)(w >> 24);
            }
        }
    }
    std::vector<uint64_t> ps((size_t)n * TOURNAMENT_MAX_GROUP * TOURNAMENT_STAGES);
    HIP_TRY(c, hipMemcpyAsync(ps.data(), base + o_ps, ps_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(paths.advance_counts, base + o_adv, adv_bytes, hipMemcpyDeviceToHost, s));
    if (nf) {
        HIP_TRY(c, hipMemcpyAsync(paths.joint_counts, base + o_joint, joint_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(paths.outcome_counts, base + o_out, nf * 3 * 8, hipMemcpyDeviceToHost, s));
    }
    if ((rc = tournament_decided(c, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_read(c, st, X)) != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    cup_query_finish(X);
    // the marginal tables are sums of the position x stage table; `reached` [n, K] is the stage counts' tail sum
    std::vector<uint64_t> reached((size_t)n * PK, 0);
    for (size_t t = 0; t < (size_t)n; ++t) {
        for (size_t k = 0; k < (size_t)rounds + 2; ++k) out.stage_counts[t * (rounds + 2) + k] = 0;
        for (size_t p = 0; p < (size_t)TOURNAMENT_MAX_GROUP; ++p) {
            uint64_t at = 0;
            for (size_t k = 0; k < (size_t)TOURNAMENT_STAGES; ++k) {
                const uint64_t v = ps[(t * TOURNAMENT_MAX_GROUP + p) * TOURNAMENT_STAGES + k];
                at += v;
                if (k < (size_t)rounds + 2) out.stage_counts[t * (rounds + 2) + k] += v;
            }
            if (q.n_groups > 0) out.group_position_counts[t * TOURNAMENT_MAX_GROUP + p] = at;
        }
        uint64_t tail = 0;
        for (size_t k = PK; k >= 1; --k) {
            tail += out.stage_counts[t * (rounds + 2) + k];
            reached[t * PK + k - 1] = tail;
        }
    }
    if (q.n_groups > 0) std::copy(ps.begin(), ps.end(), paths.position_stage_counts);
    if (nf) {
        std::copy(reached.begin(), reached.end(), paths.target_counts);
        // the draw is what the wins leave: every simulation gives a fixture exactly one outcome
        const size_t nK = (size_t)n * PK;
        for (size_t f = 0; f < nf; ++f) {
            uint64_t* oc = paths.outcome_counts + f * 3;
            oc[1] = (uint64_t)n_sims - oc[0] - oc[2];
            uint64_t* jc = paths.joint_counts + f * 3 * nK;
            for (size_t i = 0; i < nK; ++i) jc[nK + i] = reached[i] - jc[i] - jc[2 * nK + i];
        }
    }
    return BPLHIP_OK;
}

// ---- tournament_scenarios (dc_tscen.hip.h): counted by dc_scenario_count
// `lr` (bplhip_tournament_scenarios_live): as in simulate_tournament_impl -- the keys index the concatenated list;
// null: the kick-off call
static int tournament_scenarios_impl(bplhip_ctx* c, const TournamentCall& q0, const KnockoutRequest* ko,
                                     const TscenRequest& scen, const CupLiveRequest* lr = nullptr) {
    if (!c) return BPLHIP_EINVAL;
    CupLiveQuery X;
    int rc = cup_query_lists(c, "tournament_scenarios_live", q0, lr, &X);
    if (rc != BPLHIP_OK) return rc;
    const TournamentCall& q = X.q;
    TournamentSetup in;
    rc = tournament_setup(c, q, nullptr, ko, &in);
    if (rc != BPLHIP_OK) return rc;
    const char* what = "tournament_scenarios";
    const size_t nf = in.fix.size();
    int64_t cells = 1;
    if (scen.chunk_sims < 0) return fail(c, BPLHIP_EINVAL, "%s: chunk_sims=%lld is negative", what, (long long)scen.chunk_sims);
    if (q.n_groups == 0 || nf == 0)
        return fail(c, BPLHIP_EINVAL, "%s: without groups or group fixtures there is nothing to key on", what);
    rc = scenario_keys_check(c, what, scen.n_key, scen.key_fixture, scen.key_cap, q.n_fixtures, &cells);
    if (rc != BPLHIP_OK) return rc;
    if (!scen.scenario || !scen.joint) return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    if ((rc = live_weights_check(c, "tournament_scenarios_live", X.lv)) != BPLHIP_OK) return rc;
    TournamentStage st;
    if ((rc = tournament_begin(c, q, in, nullptr, ko, &st)) != BPLHIP_OK) return rc;
    // scenario u64 [M], joint u64 [M, n, R + 2] (zeroed together), the fixtures' codes u16 [nf], then the chunk's
    // records: scenario indices u32 [chunk], target sets u8 [n, chunk] -- 4 + n bytes a simulation
    const int n = q.n_teams;
    const int64_t n_sims = q.n_sims;
    const size_t M = (size_t)cells, K = (size_t)in.rounds + 2, nK = (size_t)n * K;
    const size_t chunk = chunk_for(scen.chunk_sims, 4 + (size_t)n, n_sims);
    Carver& cv = st.cv;
    const size_t o_scn = cv.take(M * 8), o_joint = cv.take(M * nK * 8), o_code = cv.take(nf * 2), o_idx = cv.take(chunk * 4),
                 o_set = cv.take((size_t)n * chunk);
    if ((rc = cup_query_plan(c, st, X)) != BPLHIP_OK) return rc;
    if ((rc = tournament_stage(c, q, in, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_stage(c, in, st, X)) != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    HIP_TRY(c, hipMemsetAsync(base + o_scn, 0, o_code - o_scn, s));
    const std::vector<uint16_t> code = scenario_codes(nf, scen.n_key, scen.key_fixture, scen.key_cap);
    HIP_TRY(c, hipMemcpyAsync(base + o_code, code.data(), nf * 2, hipMemcpyHostToDevice, s));
    dcts::TscenArgs P{};
    P.chunk = (int)chunk;
    P.fix_code = reinterpret_cast<const uint16_t*>(base + o_code);
    P.scen = reinterpret_cast<uint32_t*>(base + o_idx);
    P.tset = reinterpret_cast<uint8_t*>(base + o_set);
    dcsc::ScenarioArgs V{};   // what dc_scenario_count reads: the shape, the chunk's records and its two tables
    V.n = n;
    V.K = (int)K;
    V.chunk = (int)chunk;
    V.M = (int)M;
    // a stage-2 tile: as many whole scenarios as its LDS cells hold (at least 31: 1 + n K <= 513)
    V.tile_rows = (int)std::min<size_t>(M, (size_t)dcsc::COUNT_WORDS / (1 + nK));
    V.scen = P.scen;
    V.tset = P.tset;
    V.scenario = reinterpret_cast<unsigned long long*>(base + o_scn);
    V.joint = reinterpret_cast<unsigned long long*>(base + o_joint);
    const unsigned tiles = (unsigned)((M + V.tile_rows - 1) / V.tile_rows);
    const bool records = scen.sim_scenario || scen.sim_tset;
    std::vector<uint8_t> h_set(scen.sim_tset ? (size_t)n * chunk : 0);
    TOURNAMENT_SIM_KERNELS(dcts::TscenArgs, dcts::dc_tscen_sim, dcts::scen_alloc_sim);
    TOURNAMENT_LIVE_KERNELS(dcts::TscenArgs, dctq::cup_scen_live, dctq::cup_scen_live_table);
    for (int64_t j0 = 0; j0 < n_sims; j0 += (int64_t)chunk) {
        P.j0 = j0;
        P.nc = V.nc = (int)std::min<int64_t>((int64_t)chunk, n_sims - j0);
        rc = X.kernels ? tournament_live_launch(c, q, st, ko != nullptr, live_kernels, P, X.V)
                       : tournament_sim_launch(c, q, st, ko != nullptr, kernels, P);
        if (rc != BPLHIP_OK) return rc;
        hipLaunchKernelGGL(dcsc::dc_scenario_count, count_grid(c, tiles, V.nc, dcsc::COUNT_THREADS), dim3(dcsc::COUNT_THREADS),
                           0, s, V);
        HIP_TRY(c, hipGetLastError());
        if (!records) continue;
        // the chunk's records into the caller's per-simulation arrays: the target sets turned simulation-major
        if (scen.sim_scenario)
            HIP_TRY(c, hipMemcpyAsync(scen.sim_scenario + j0, base + o_idx, (size_t)P.nc * 4, hipMemcpyDeviceToHost, s));
        if (scen.sim_tset) HIP_TRY(c, hipMemcpyAsync(h_set.data(), base + o_set, (size_t)n * chunk, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        for (size_t t = 0; scen.sim_tset && t < (size_t)n; ++t)
            for (size_t i = 0; i < (size_t)P.nc; ++i) scen.sim_tset[((size_t)j0 + i) * n + t] = h_set[t * chunk + i];
    }
    HIP_TRY(c, hipMemcpyAsync(scen.scenario, base + o_scn, M * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(scen.joint, base + o_joint, M * nK * 8, hipMemcpyDeviceToHost, s));
    if ((rc = tournament_decided(c, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_read(c, st, X)) != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    cup_query_finish(X);
    return BPLHIP_OK;
}

// ---- tournament_points (dc_group_points.hip.h): counted by dc_gpts_count
// `lr` (bplhip_tournament_points_live): as in simulate_tournament_impl -- the matches in play are matches to come on
// the points axis; null: the kick-off call
static int tournament_points_impl(bplhip_ctx* c, const TournamentCall& q0, const KnockoutRequest* ko,
                                  const GptsRequest& gpts, const CupLiveRequest* lr = nullptr) {
    if (!c) return BPLHIP_EINVAL;
    CupLiveQuery X;
    int rc = cup_query_lists(c, "tournament_points_live", q0, lr, &X);
    if (rc != BPLHIP_OK) return rc;
    const TournamentCall& q = X.q;
    TournamentSetup in;
    rc = tournament_setup(c, q, nullptr, ko, &in);
    if (rc != BPLHIP_OK) return rc;
    const char* what = "tournament_points";
    const int n = q.n_teams, best_of_rest = q.best_of_rest;
    if (gpts.chunk_sims < 0) return fail(c, BPLHIP_EINVAL, "%s: chunk_sims=%lld is negative", what, (long long)gpts.chunk_sims);
    if (q.n_groups == 0) return fail(c, BPLHIP_EINVAL, "%s: without groups there are no group points", what);
    if (gpts.n_bins < 1 || gpts.n_bins > BPLHIP_GROUP_POINTS_MAX_BINS)
        return fail(c, BPLHIP_EINVAL, "%s: n_bins=%d out of range [1,%d]", what, gpts.n_bins, BPLHIP_GROUP_POINTS_MAX_BINS);
    if (gpts.gd_cap < 0 || gpts.gd_cap > BPLHIP_GROUP_POINTS_MAX_GD_CAP)
        return fail(c, BPLHIP_EINVAL, "%s: gd_cap=%d out of range [0,%d]", what, gpts.gd_cap, BPLHIP_GROUP_POINTS_MAX_GD_CAP);
    if (!gpts.team_points || !gpts.team_target || !gpts.team_place || !gpts.place_points || !gpts.place_gap ||
        (best_of_rest > 0 && (!gpts.rest_count || !gpts.rest_through || !gpts.rest_rank)))
        return fail(c, BPLHIP_EINVAL, "%s: null required output", what);
    // the largest group Z and the B groups with a place advance + 1
    int gZ = 0, gB = 0;
    for (const int size : in.size) {
        gZ = std::max(gZ, size);
        gB += size > q.advance ? 1 : 0;
    }
    // the axis holds every total a simulation can reach, as axis_check has it for a season
    const int64_t least = std::min({q.win, q.draw, q.loss}), most = std::max({q.win, q.draw, q.loss});
    std::vector<int64_t> matches((size_t)n, 0);
    for (const uint16_t f : in.fix) {
        ++matches[f & 0xFFu];
        ++matches[f >> 8];
    }
    for (int t = 0; t < n; ++t) {
        const int64_t lo = q.init_points[t] + matches[t] * least, hi = q.init_points[t] + matches[t] * most;
        if (lo < (int64_t)gpts.points_min || hi >= (int64_t)gpts.points_min + gpts.n_bins)
            return fail(c, BPLHIP_EINVAL, "%s: slot %d can end on %lld..%lld points, outside [%d,%lld)", what, t, (long long)lo,
                        (long long)hi, gpts.points_min, (long long)gpts.points_min + gpts.n_bins);
    }
    if ((rc = live_weights_check(c, "tournament_points_live", X.lv)) != BPLHIP_OK) return rc;
    TournamentStage st;
    if ((rc = tournament_begin(c, q, in, nullptr, ko, &st)) != BPLHIP_OK) return rc;
    // team_points u64 [n, P], team_target u64 [n, P, R + 2], team_place u64 [n, P, Z], place_points u64 [Gn, Z, P],
    // place_gap u64 [Gn, Z - 1, P] and with best_of_rest > 0 rest_count and rest_through u64 [P, D] and rest_rank u64
    // [B, P, D] (zeroed together), then the chunk's records: slots u32 [n, chunk], places u8 [Gn, Z, chunk], rest ranks
    // u16 [B, chunk] -- 4 n + Gn Z + 2 B bytes a simulation
    static_assert(dcgq::GPTS_MAX_GROUPS >= BPLHIP_TOURNAMENT_MAX_GROUPS && dcgq::GPTS_MAX_BINS == BPLHIP_GROUP_POINTS_MAX_BINS &&
                  dcgq::GPTS_MAX_GD_CAP == BPLHIP_GROUP_POINTS_MAX_GD_CAP, "dc_group_points.hip.h and bplhip.h disagree");
    const int64_t n_sims = q.n_sims;
    const size_t N = (size_t)n, GP = (size_t)gpts.n_bins, GD = 2 * (size_t)gpts.gd_cap + 1, GK = (size_t)in.rounds + 2,
                 GZ = (size_t)gZ, GG = (size_t)q.n_groups, GB = best_of_rest > 0 ? (size_t)gB : 0;
    const size_t chunk = chunk_for(gpts.chunk_sims, 4 * N + GG * GZ + 2 * (size_t)gB, n_sims);
    Carver& cv = st.cv;
    const size_t o_tp = cv.take(N * GP * 8), o_tt = cv.take(N * GP * GK * 8), o_tz = cv.take(N * GP * GZ * 8),
                 o_pp = cv.take(GG * GZ * GP * 8), o_gap = cv.take(GG * (GZ - 1) * GP * 8), o_rc = cv.take(GB ? GP * GD * 8 : 0),
                 o_rt = cv.take(GB ? GP * GD * 8 : 0), o_rr = cv.take(GB * GP * GD * 8), tables_end = cv.total;
    const size_t o_slot = cv.take(N * chunk * 4), o_place = cv.take(GG * GZ * chunk), o_rank = cv.take(GB * chunk * 2);
    if ((rc = cup_query_plan(c, st, X)) != BPLHIP_OK) return rc;
    if ((rc = tournament_stage(c, q, in, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_stage(c, in, st, X)) != BPLHIP_OK) return rc;
    char* base = st.base;
    hipStream_t s = st.s;
    HIP_TRY(c, hipMemsetAsync(base + o_tp, 0, tables_end - o_tp, s));
    dcgq::GptsArgs P{};
    P.chunk = (int)chunk;
    P.n = n;
    P.K = (int)GK;
    P.Z = gZ;
    P.Gn = q.n_groups;
    P.B = (int)GB;
    P.best = best_of_rest;
    P.points_min = gpts.points_min;
    P.P = gpts.n_bins;
    P.cap = gpts.gd_cap;
    P.D = (int)GD;
    std::copy(in.size.begin(), in.size.end(), P.gsize);
    P.slot = reinterpret_cast<uint32_t*>(base + o_slot);
    P.place = reinterpret_cast<uint8_t*>(base + o_place);
    P.rank = reinterpret_cast<uint16_t*>(base + o_rank);
    P.team_points = reinterpret_cast<unsigned long long*>(base + o_tp);
    P.team_target = reinterpret_cast<unsigned long long*>(base + o_tt);
    P.team_place = reinterpret_cast<unsigned long long*>(base + o_tz);
    P.place_points = reinterpret_cast<unsigned long long*>(base + o_pp);
    P.place_gap = reinterpret_cast<unsigned long long*>(base + o_gap);
    P.rest_count = reinterpret_cast<unsigned long long*>(base + o_rc);
    P.rest_through = reinterpret_cast<unsigned long long*>(base + o_rt);
    P.rest_rank = reinterpret_cast<unsigned long long*>(base + o_rr);
    // the rows of stage 2: slots, places, gaps, and with a best of the rest two pooled rows per slot and the ranks
    const unsigned rows = (unsigned)(N + GG * GZ + GG * (GZ - 1) + (GB ? 2 * N + GB : 0));
    TOURNAMENT_SIM_KERNELS(dcgq::GptsArgs, dcgq::dc_gpts_sim, dcgq::points_alloc_sim);
    TOURNAMENT_LIVE_KERNELS(dcgq::GptsArgs, dctq::cup_gpoints_live, dctq::cup_gpoints_live_table);
    for (int64_t j0 = 0; j0 < n_sims; j0 += (int64_t)chunk) {
        P.j0 = j0;
        P.nc = (int)std::min<int64_t>((int64_t)chunk, n_sims - j0);
        rc = X.kernels ? tournament_live_launch(c, q, st, ko != nullptr, live_kernels, P, X.V)
                       : tournament_sim_launch(c, q, st, ko != nullptr, kernels, P);
        if (rc != BPLHIP_OK) return rc;
        hipLaunchKernelGGL(dcgq::dc_gpts_count, count_grid(c, rows, P.nc, dcgq::COUNT_THREADS), dim3(dcgq::COUNT_THREADS), 0,
                           s, P);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(gpts.team_points, base + o_tp, N * GP * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(gpts.team_target, base + o_tt, N * GP * GK * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(gpts.team_place, base + o_tz, N * GP * GZ * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(gpts.place_points, base + o_pp, GG * GZ * GP * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(gpts.place_gap, base + o_gap, GG * (GZ - 1) * GP * 8, hipMemcpyDeviceToHost, s));
    if (GB) {
        HIP_TRY(c, hipMemcpyAsync(gpts.rest_count, base + o_rc, GP * GD * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(gpts.rest_through, base + o_rt, GP * GD * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(gpts.rest_rank, base + o_rr, GB * GP * GD * 8, hipMemcpyDeviceToHost, s));
    }
    if ((rc = tournament_decided(c, ko, st)) != BPLHIP_OK) return rc;
    if ((rc = cup_query_read(c, st, X)) != BPLHIP_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    cup_query_finish(X);
    return BPLHIP_OK;
}
#undef TOURNAMENT_SIM_KERNELS
#undef TOURNAMENT_LIVE_KERNELS

// ---- guarded C-ABI entry points (see `guarded`)
extern "C" int bplhip_create(bplhip_ctx** out, int device_id) {
    return guarded(nullptr, "bplhip_create", [&] { return bplhip_create_impl(out, device_id); });
}
extern "C" int bplhip_set_fixtures(bplhip_ctx* c, int model_kind, int64_t n, int32_t n_teams,
                        const uint16_t* home_idx, const uint16_t* away_idx,
                        const uint8_t* home_goals, const uint8_t* away_goals,
                        const float* weights, const double* covariates, int32_t k,
                        void* stream) {
    return guarded(c, "bplhip_set_fixtures", [&] { return bplhip_set_fixtures_impl(c, model_kind, n, n_teams, home_idx, away_idx, home_goals, away_goals, weights, covariates, k, stream); });
}
extern "C" int bplhip_set_fixtures_neutral(bplhip_ctx* c, int64_t n, int32_t n_teams, const uint16_t* home_idx,
                                const uint16_t* away_idx, const uint8_t* home_goals,
                                const uint8_t* away_goals, const uint8_t* neutral_venue,
                                const uint8_t* home_conf, const uint8_t* away_conf, int32_t n_conf,
                                const float* weights, const double* covariates, int32_t k,
                                void* stream) {
    return guarded(c, "bplhip_set_fixtures_neutral", [&] { return bplhip_set_fixtures_neutral_impl(c, n, n_teams, home_idx, away_idx, home_goals, away_goals, neutral_venue, home_conf, away_conf, n_conf, weights, covariates, k, stream); });
}
extern "C" int bplhip_set_fixtures_dynamic(bplhip_ctx* c, int64_t n, int32_t n_teams, int32_t n_gameweeks,
                                const uint16_t* home_idx, const uint16_t* away_idx,
                                const uint8_t* home_goals, const uint8_t* away_goals,
                                const uint16_t* gameweek, const uint8_t* neutral_venue,
                                const double* covariates, int32_t k, int32_t random_walk,
                                void* stream) {
    return guarded(c, "bplhip_set_fixtures_dynamic", [&] { return bplhip_set_fixtures_dynamic_impl(c, n, n_teams, n_gameweeks, home_idx, away_idx, home_goals, away_goals, gameweek, neutral_venue, covariates, k, random_walk, stream); });
}
extern "C" int bplhip_logp_grad_batched(bplhip_ctx* c, int32_t n_chains, const double* z,
                             double* potential, double* grad, double* aux, void* stream) {
    return guarded(c, "bplhip_logp_grad_batched", [&] { return bplhip_logp_grad_batched_impl(c, n_chains, z, potential, grad, aux, stream); });
}
extern "C" int bplhip_logp_grad_graph(bplhip_ctx* c, int32_t count, int32_t n_z, const double* z,
                           double* potential, double* grad, int32_t replays, void* stream) {
    return guarded(c, "bplhip_logp_grad_graph", [&] { return bplhip_logp_grad_graph_impl(c, count, n_z, z, potential, grad, replays, stream); });
}
extern "C" int bplhip_nuts_run(bplhip_ctx* c, const bplhip_nuts_cfg* cfg, const double* z0,
                               uint32_t seed_hi, uint32_t seed_lo, double* draws_out,
                               bplhip_nuts_stats* stats, void* stream) {
    return guarded(c, "bplhip_nuts_run", [&] { return bplhip_nuts_run_impl(c, cfg, z0, seed_hi, seed_lo, draws_out, stats, stream); });
}
extern "C" int bplhip_nuts_run_chains(bplhip_ctx* c, const bplhip_nuts_cfg* cfg, int32_t n_chains,
                                      const double* z0, const uint32_t* seeds, double* draws_out,
                                      bplhip_nuts_stats* stats, void* stream) {
    return guarded(c, "bplhip_nuts_run_chains", [&] { return bplhip_nuts_run_chains_impl(c, cfg, n_chains, z0, seeds, draws_out, stats, stream); });
}
extern "C" int bplhip_constrain(bplhip_ctx* c, const double* z_draws, int64_t s,
                                double* attack, double* defence, double* home_advantage,
                                double* corr_coef) {
    return guarded(c, "bplhip_constrain", [&] { return bplhip_constrain_impl(c, z_draws, s, attack, defence, home_advantage, corr_coef); });
}
extern "C" int bplhip_constrain_dynamic(bplhip_ctx* c, const double* z_draws, int64_t s,
                                        double* attack, double* defence, double* home_attack,
                                        double* away_attack, double* home_defence,
                                        double* away_defence) {
    return guarded(c, "bplhip_constrain_dynamic", [&] { return bplhip_constrain_dynamic_impl(c, z_draws, s, attack, defence, home_attack, away_attack, home_defence, away_defence); });
}
extern "C" int bplhip_predict_set_posterior(bplhip_ctx* c, int32_t s, int32_t t,
                                            const double* attack, const double* defence,
                                            const double* home_advantage,
                                            int32_t home_advantage_per_team,
                                            const double* corr_coef) {
    return guarded(c, "bplhip_predict_set_posterior", [&] { return bplhip_predict_set_posterior_impl(c, s, t, attack, defence, home_advantage, home_advantage_per_team, corr_coef); });
}
extern "C" int bplhip_predict_score_grid(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, double* out,
                                         void* stream) {
    return guarded(c, "bplhip_predict_score_grid", [&] { return predict_score_grid_any(c, q, max_goals, out, false, stream); });
}
extern "C" int bplhip_predict_score_grid_f32(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, float* out,
                                             void* stream) {
    return guarded(c, "bplhip_predict_score_grid_f32", [&] { return predict_score_grid_any(c, q, max_goals, out, true, stream); });
}
extern "C" int bplhip_predict_set_posterior_venue(bplhip_ctx* c, int32_t s, int32_t t, const double* attack,
                                                  const double* defence, const double* home_attack,
                                                  const double* away_attack, const double* home_defence,
                                                  const double* away_defence, int32_t n_conf,
                                                  const double* confederation_strength,
                                                  const double* corr_coef) {
    return guarded(c, "bplhip_predict_set_posterior_venue", [&] {
        return bplhip_predict_set_posterior_venue_impl(c, s, t, attack, defence, home_attack, away_attack, home_defence,
                                                       away_defence, n_conf, confederation_strength, corr_coef);
    });
}
__global__ void selftest_math_kernel(int which, long long n, const double* in, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    out[i] = which == 0 ? dc::lean::exp(x) : which == 1 ? dc::lean::log(x)
           : which == 2 ? dc::lean::log1p_pos(x) : dc::lean::rcp(x);
}
extern "C" int bplhip_selftest_math(bplhip_ctx* c, int32_t which, int64_t n, const double* in, double* out) {
    return guarded(c, "bplhip_selftest_math", [&] {
        if (!c || which < 0 || which > 3 || n < 1 || !in || !out) return c ? fail(c, BPLHIP_EINVAL, "selftest_math: bad arguments") : BPLHIP_EINVAL;
        HIP_TRY(c, hipSetDevice(c->device));
        DevBuf din, dout;
        HIP_TRY(c, din.ensure((size_t)n * 8));
        HIP_TRY(c, dout.ensure((size_t)n * 8));
        HIP_TRY(c, hipMemcpy(din.p, in, (size_t)n * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(selftest_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, which,
                           (long long)n, din.as<const double>(), dout.as<double>());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpy(out, dout.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        return (int)BPLHIP_OK;
    });
}
// ---- test-only probes of the cross-lane layer and the counted rows (bplhip_selftest_lanes, include/bplhip.h).
// Every probe calls the library's own function and stores what EVERY lane holds afterwards.  A wave owns
// SL_CH channels of 64 lanes of each type; the channels a probe does not name as operands are bystanders: live
// in VGPRs across the call (the written-out reductions of wave_reduce.hip.h pin physical registers) and echoed.
namespace selftest {
constexpr int SL_CH = BPLHIP_SELFTEST_CHANNELS;
constexpr int SL_WAVE = SL_CH * 64;   // elements per wave and type
enum {
    SL_SUM4_F64 = 0, SL_BOUNDS, SL_LANES8, SL_MAX3_F32, SL_SUM1_F64, SL_SUM2_F64, SL_MAX1_F64, SL_MAX1_F32,
    SL_MAX_F64_F32, SL_MAX3_F64, SL_ROW_SUM6,
    SL_SUM_F32, SL_SUM2_F32, SL_PREV_LANE, SL_PREFIX, SL_SUFFIX, SL_SUMN_2, SL_SUMN_7, SL_SUMN_13,
    SL_BLOCK_2, SL_BLOCK_5_LDS, SL_BLOCK_6_LDS, SL_ND_SUM, SL_ND_SUM2, SL_TOP2_F32, SL_TOP2_F64, SL_TOP2_PAIR,
    SL_Q30, SL_EXACT_I64, SL_COUNTED_ROWS, SL_N
};
static_assert(SL_COUNTED_ROWS == BPLHIP_SELFTEST_COUNTED_ROWS, "the probe numbers of include/bplhip.h");
constexpr bool sl_block(int w) { return w == SL_BLOCK_2 || w == SL_BLOCK_5_LDS || w == SL_BLOCK_6_LDS; }
template <int NV>
__device__ __forceinline__ void sl_sumN(double (&d)[SL_CH]) {
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = d[j];
    dc::wave_sumN_f64(v);
#pragma unroll
    for (int j = 0; j < NV; ++j) d[j] = v[j];
}
template <int NV, bool LDS_ONLY>
__device__ __forceinline__ void sl_block_sum(double (&d)[SL_CH], double* scratch) {
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = d[j];
    dc::block_sum<NV, LDS_ONLY>(v, scratch, (int)threadIdx.x);
#pragma unroll
    for (int j = 0; j < NV; ++j) d[j] = v[j];
}
template <int W>
__global__ void __launch_bounds__(sl_block(W) ? dc::BLOCK : 64)
lanes_kernel(const double* in64, const float* in32, const int* ini, double* o64, float* o32, int* oi) {
    __shared__ double scratch[dc::WAVES * 8];
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const size_t base = wave * SL_WAVE + lane;
    double d[SL_CH];
    float f[SL_CH];
    int n[SL_CH];
#pragma unroll
    for (int j = 0; j < SL_CH; ++j) {
        d[j] = in64[base + j * 64];
        f[j] = in32[base + j * 64];
        n[j] = ini[base + j * 64];
    }
#pragma unroll
    for (int j = 0; j < SL_CH; ++j) {   // (in registers BEFORE the call, not loaded behind it)
        asm volatile("" : "+v"(d[j]));
        asm volatile("" : "+v"(f[j]));
        asm volatile("" : "+v"(n[j]));
    }
    if constexpr (W == SL_SUM4_F64) {
        double v[4] = {d[0], d[1], d[2], d[3]};
        dc::wave_sum4_f64(v);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    } else if constexpr (W == SL_BOUNDS) {
        dc::wave_bounds_reduce(f[0], f[1], f[2], d[0], d[1], d[2], d[3]);
    } else if constexpr (W == SL_LANES8) {
        dc::lanes8_max3_sum(d[0], d[1], d[2], d[3], f[0], f[1], f[2]);
    } else if constexpr (W == SL_MAX3_F32) {
        dc::wave_max3_f32(f[0], f[1], f[2]);
    } else if constexpr (W == SL_SUM1_F64) {
        d[0] = dc::wave_sum_f64(d[0]);
    } else if constexpr (W == SL_SUM2_F64) {
        dc::wave_sum2_f64(d[0], d[1]);
    } else if constexpr (W == SL_MAX1_F64) {
        d[0] = dc::wave_max_f64(d[0]);
    } else if constexpr (W == SL_MAX1_F32) {
        f[0] = dc::wave_max_f32(f[0]);
    } else if constexpr (W == SL_MAX_F64_F32) {   // (no wrapper: what every lane holds, the promise is lane 63)
        wr::wave_reduce_max_f64_f32_raw(f[0], d[0]);
    } else if constexpr (W == SL_MAX3_F64) {
        dc::wave_max3_f64(d[0], d[1], d[2]);
    } else if constexpr (W == SL_ROW_SUM6) {
        double v[6] = {d[0], d[1], d[2], d[3], d[4], d[5]};
        dc::row_sum_f64(v);
#pragma unroll
        for (int j = 0; j < 6; ++j) d[j] = v[j];
    } else if constexpr (W == SL_SUM_F32) {
        f[0] = dc::wave_sum_f32(f[0]);
    } else if constexpr (W == SL_SUM2_F32) {
        dc::wave_sum2_f32(f[0], f[1]);
    } else if constexpr (W == SL_PREV_LANE) {
        n[0] = (int)dc::prev_lane_u32((uint32_t)n[0], (uint32_t)n[1]);
    } else if constexpr (W == SL_PREFIX) {
        d[0] = dc::wave_prefix_dpp_f64(d[0]);
    } else if constexpr (W == SL_SUFFIX) {
        d[0] = dc::wave_suffix_dpp_f64(d[0], lane);
    } else if constexpr (W == SL_SUMN_2) {
        sl_sumN<2>(d);
    } else if constexpr (W == SL_SUMN_7) {
        sl_sumN<7>(d);
    } else if constexpr (W == SL_SUMN_13) {
        sl_sumN<13>(d);
    } else if constexpr (W == SL_BLOCK_2) {
        sl_block_sum<2, false>(d, scratch);
    } else if constexpr (W == SL_BLOCK_5_LDS) {
        sl_block_sum<5, true>(d, scratch);
    } else if constexpr (W == SL_BLOCK_6_LDS) {
        sl_block_sum<6, true>(d, scratch);
    } else if constexpr (W == SL_ND_SUM) {
        d[0] = nd::nd_wave_sum(d[0]);
    } else if constexpr (W == SL_ND_SUM2) {
        nd::nd_wave_sum2(d[0], d[1]);
    } else if constexpr (W == SL_TOP2_F32 || W == SL_TOP2_F64 || W == SL_TOP2_PAIR) {
        // the wave's channels read flat as per-team arrays: T (the same in all lanes of i32 channel 0) teams
        const int cap = W == SL_TOP2_PAIR ? SL_WAVE / 2 : SL_WAVE;
        const int T = min(max(__builtin_amdgcn_readfirstlane(n[0]), 1), cap);
        if constexpr (W == SL_TOP2_F64) {
            const double* tab = in64 + wave * SL_WAVE;
            const dc::Top2<double> R = dc::wave_top2<double>(T, lane, [&](int t) { return tab[t]; });
            d[0] = R.m1; d[1] = R.m2; n[1] = R.i1; n[2] = R.i2;
        } else if constexpr (W == SL_TOP2_F32) {
            const float* tab = in32 + wave * SL_WAVE;
            const dc::Top2<float> R = dc::wave_top2<float>(T, lane, [&](int t) { return tab[t]; });
            f[0] = R.m1; f[1] = R.m2; n[1] = R.i1; n[2] = R.i2;
        } else {
            const float* ta = in32 + wave * SL_WAVE;
            const float* tb = ta + SL_WAVE / 2;
            dc::Top2<float> Ra, Rb;
            dc::wave_top2_pair_f32(T, lane, [&](int t, float* va, float* vb) { *va = ta[t]; *vb = tb[t]; }, &Ra, &Rb);
            f[0] = Ra.m1; f[1] = Ra.m2; n[1] = Ra.i1; n[2] = Ra.i2;
            f[2] = Rb.m1; f[3] = Rb.m2; n[3] = Rb.i1; n[4] = Rb.i2;
        }
    } else if constexpr (W == SL_Q30) {
        d[0] = dc::q30(f[0]);
    } else if constexpr (W == SL_EXACT_I64) {
        d[0] = __longlong_as_double(dc::exact_i64(d[0]));
    }
#pragma unroll
    for (int j = 0; j < SL_CH; ++j) {
        asm volatile("" : "+v"(d[j]));
        asm volatile("" : "+v"(f[j]));
        asm volatile("" : "+v"(n[j]));
    }
#pragma unroll
    for (int j = 0; j < SL_CH; ++j) {
        o64[base + j * 64] = d[j];
        o32[base + j * 64] = f[j];
        oi[base + j * 64] = n[j];
    }
}
template <int W>
void launch_lanes(int n_waves, const double* in64, const float* in32, const int* ini, double* o64, float* o32, int* oi) {
    const int per = sl_block(W) ? dc::WAVES : 1;
    hipLaunchKernelGGL(lanes_kernel<W>, dim3((unsigned)(n_waves / per)), dim3(64 * per), 0, 0, in64, in32, ini, o64, o32, oi);
}
template <int W = 0>
void dispatch_lanes(int which, int n_waves, const double* in64, const float* in32, const int* ini, double* o64, float* o32,
                    int* oi) {
    if constexpr (W < SL_COUNTED_ROWS) {
        if (which == W) launch_lanes<W>(n_waves, in64, in32, ini, o64, o32, oi);
        else dispatch_lanes<W + 1>(which, n_waves, in64, in32, ini, o64, o32, oi);
    }
}
// counted rows: one workgroup per contribution, one ga_add per row ...
__global__ void ga_add_kernel(long long* rows, const double* vals, int n_rows) {
    for (int r = threadIdx.x; r < n_rows; r += blockDim.x)
        dc::ga_add(rows + (size_t)r * dc::GA_ROW, vals[(size_t)blockIdx.x * n_rows + r]);
}
// ... ONE workgroup reads every row through every load form, then (behind a barrier: its own loads of the
// neighbouring rows are done) re-arms them; o64: SL_GA_WORDS 64-bit words per row, oi: 4 ints per row
constexpr int SL_GA_WORDS = BPLHIP_SELFTEST_GA_WORDS;
__device__ __forceinline__ void sl_put4(long long* o, const dc::GaWords (&w)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[2 * k] = w[k].lo; o[2 * k + 1] = w[k].hi; }
}
__global__ void ga_read_kernel(long long* rows, int n_rows, long long* o64, int* oi) {
    for (int r = threadIdx.x; r < n_rows; r += blockDim.x) {
        const long long* r0 = rows + (size_t)r * dc::GA_ROW;
        const long long* r1 = rows + (size_t)((r + 1) % n_rows) * dc::GA_ROW;
        const long long* r2 = rows + (size_t)((r + 2) % n_rows) * dc::GA_ROW;
        const long long* r3 = rows + (size_t)((r + 3) % n_rows) * dc::GA_ROW;
        long long* o = o64 + (size_t)r * SL_GA_WORDS;
        const dc::GaWords w0 = dc::ga_load(r0);
        o[0] = w0.lo; o[1] = w0.hi;
        o[2] = __double_as_longlong(dc::ga_value(w0));
        oi[4 * r + 0] = dc::ga_count(w0);
        oi[4 * r + 1] = dc::ga_is_zero(w0) ? 1 : 0;
        dc::GaWords a, b, w[4];
        dc::ga_load2(r0, r1, &a, &b);
        o[3] = a.lo; o[4] = a.hi; o[5] = b.lo; o[6] = b.hi;
        dc::ga_load4(r0, r1, r2, r3, w);
        sl_put4(o + 7, w);
        dc::ga_load3(r0, r1, r2, w);
        sl_put4(o + 15, w);
        dc::ga_load2rows(r0, r1, w);
        sl_put4(o + 23, w);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < n_rows; r += blockDim.x) dc::ga_rearm(rows + (size_t)r * dc::GA_ROW);
}
__global__ void ga_reread_kernel(const long long* rows, int n_rows, long long* o64, int* oi) {
    for (int r = threadIdx.x; r < n_rows; r += blockDim.x) {
        const dc::GaWords w = dc::ga_load(rows + (size_t)r * dc::GA_ROW);
        o64[(size_t)r * SL_GA_WORDS + 31] = w.lo | w.hi;
        oi[4 * r + 2] = dc::ga_is_zero(w) ? 1 : 0;
        oi[4 * r + 3] = dc::ga_count(w);
    }
}
}  // namespace selftest
extern "C" int bplhip_selftest_lanes(bplhip_ctx* c, int32_t which, int32_t n_waves, const double* in_f64,
                                     const float* in_f32, const int32_t* in_i32, double* out_f64, float* out_f32,
                                     int32_t* out_i32) {
    using namespace selftest;
    return guarded(c, "bplhip_selftest_lanes", [&] {
        if (!c) return (int)BPLHIP_EINVAL;
        if (which < 0 || which >= SL_N || n_waves < 1 || n_waves > (1 << 16) || !in_f64 || !in_i32 || !out_f64 || !out_i32)
            return fail(c, BPLHIP_EINVAL, "selftest_lanes: bad arguments");
        HIP_TRY(c, hipSetDevice(c->device));
        DevBuf d64, d32, di, e64, e32, ei;
        if (which == SL_COUNTED_ROWS) {
            const int n_rows = n_waves, n_contrib = in_i32[0];
            if (n_contrib < 1 || n_contrib > 255) return fail(c, BPLHIP_EINVAL, "selftest_lanes: 1..255 contributions");
            const size_t row_bytes = (size_t)n_rows * dc::GA_ROW * 8, val_bytes = (size_t)n_contrib * n_rows * 8;
            const size_t o_bytes = (size_t)n_rows * SL_GA_WORDS * 8;
            HIP_TRY(c, di.ensure(row_bytes));
            HIP_TRY(c, d64.ensure(val_bytes));
            HIP_TRY(c, e64.ensure(o_bytes));
            HIP_TRY(c, ei.ensure((size_t)n_rows * 16));
            HIP_TRY(c, hipMemset(di.p, 0, row_bytes));
            HIP_TRY(c, hipMemset(e64.p, 0, o_bytes));
            HIP_TRY(c, hipMemcpy(d64.p, in_f64, val_bytes, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(ga_add_kernel, dim3((unsigned)n_contrib), dim3(64), 0, 0, di.as<long long>(),
                               d64.as<const double>(), n_rows);
            hipLaunchKernelGGL(ga_read_kernel, dim3(1), dim3(dc::BLOCK), 0, 0, di.as<long long>(), n_rows,
                               e64.as<long long>(), ei.as<int>());
            hipLaunchKernelGGL(ga_reread_kernel, dim3(1), dim3(dc::BLOCK), 0, 0, di.as<const long long>(), n_rows,
                               e64.as<long long>(), ei.as<int>());
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpy(out_f64, e64.p, o_bytes, hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(out_i32, ei.p, (size_t)n_rows * 16, hipMemcpyDeviceToHost));
            return (int)BPLHIP_OK;
        }
        if (!in_f32 || !out_f32) return fail(c, BPLHIP_EINVAL, "selftest_lanes: bad arguments");
        if (sl_block(which) && n_waves % dc::WAVES) return fail(c, BPLHIP_EINVAL, "selftest_lanes: whole workgroups of 8 waves");
        const size_t n = (size_t)n_waves * SL_WAVE;
        HIP_TRY(c, d64.ensure(n * 8)); HIP_TRY(c, e64.ensure(n * 8));
        HIP_TRY(c, d32.ensure(n * 4)); HIP_TRY(c, e32.ensure(n * 4));
        HIP_TRY(c, di.ensure(n * 4));  HIP_TRY(c, ei.ensure(n * 4));
        HIP_TRY(c, hipMemcpy(d64.p, in_f64, n * 8, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(d32.p, in_f32, n * 4, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(di.p, in_i32, n * 4, hipMemcpyHostToDevice));
        dispatch_lanes(which, n_waves, d64.as<const double>(), d32.as<const float>(), di.as<const int>(), e64.as<double>(),
                       e32.as<float>(), ei.as<int>());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpy(out_f64, e64.p, n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(out_f32, e32.p, n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(out_i32, ei.p, n * 4, hipMemcpyDeviceToHost));
        return (int)BPLHIP_OK;
    });
}
extern "C" int bplhip_predict_score_proba(bplhip_ctx* c, const bplhip_fixtures* q, double* out, void* stream) {
    return guarded(c, "bplhip_predict_score_proba", [&] { return predict_score_proba_any(c, q, out, stream); });
}
// the season family's wrappers: every one names its first fifteen parameters and its stream as include/bplhip.h
// does, and the four simulate_season forms their seven outputs; how a symbol asks for the head-to-head order is
// its own (the _h2h suffix, head_to_head == 1, a non-null pair_init)
#define SEASON_CALL(h2h)                                                                                             \
    SeasonCall{n_fixtures, home_idx,    away_idx,    n_table, table_idx, init_points, init_gf, init_ga, win_points, \
               draw_points, loss_points, n_sims,     key_hi,  key_lo,    stream,      h2h}
#define SEASON_OUT SeasonOut{position_counts, points_sum, gd_sum, sim_points, sim_position, home_goals, away_goals}
// the four live forms name the live request's inputs and its two outputs alike
#define LIVE_IN                                                                                                      \
    LiveIn{n_in_play,       in_play_home_idx, in_play_away_idx, in_play_home_goals, in_play_away_goals,              \
           in_play_elapsed, reweight,         log_weights,      ess,                log_evidence}
// the tournament family's wrappers likewise: their first twenty-two parameters and their stream; the three
// simulate_tournament forms and tournament_paths their three outputs
#define TOURNAMENT_CALL(h2h)                                                                                           \
    TournamentCall{n_teams, team_idx,     team_conf,     team_host, n_groups,   team_group,  init_points, init_gf,    \
                   init_ga, n_fixtures,   fix_p,         fix_q,     advance,    best_of_rest, n_bracket,  bracket,    \
                   win_points, draw_points, loss_points, n_sims,    key_hi,     key_lo,      stream,      h2h}
#define TOURNAMENT_H2H (head_to_head ? H2HRequest{true, pair_init} : H2HRequest{})
#define TOURNAMENT_OUT TournamentOut{stage_counts, group_position_counts, sim_stage}
extern "C" int bplhip_simulate_season(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                      const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                      const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                      int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                      uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts,
                                      int64_t* points_sum, int64_t* gd_sum, int32_t* sim_points,
                                      uint8_t* sim_position, uint8_t* home_goals, uint8_t* away_goals, void* stream) {
    return guarded(c, "bplhip_simulate_season", [&] {
        return simulate_season_impl(c, SEASON_CALL(H2HRequest{}), SEASON_OUT);
    });
}
extern "C" int bplhip_match_leverage(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                     const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                     const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                     int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                     uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                     int64_t chunk_sims, uint64_t* outcome_counts, uint64_t* target_counts,
                                     uint64_t* joint_counts, void* stream) {
    return guarded(c, "bplhip_match_leverage", [&] {
        return match_leverage_impl(c, SEASON_CALL(H2HRequest{}), {n_targets, target_mask, chunk_sims}, outcome_counts,
                                   target_counts, joint_counts);
    });
}
extern "C" int bplhip_simulate_tournament(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                          const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                          const uint8_t* team_group, const int32_t* init_points,
                                          const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures,
                                          const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                          int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
                                          int32_t win_points, int32_t draw_points, int32_t loss_points,
                                          int64_t n_sims, uint32_t key_hi, uint32_t key_lo, uint64_t* stage_counts,
                                          uint64_t* group_position_counts, uint8_t* sim_stage, void* stream) {
    return guarded(c, "bplhip_simulate_tournament", [&] {
        return simulate_tournament_impl(c, TOURNAMENT_CALL(H2HRequest{}), TOURNAMENT_OUT);
    });
}
extern "C" int bplhip_simulate_season_h2h(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                          const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                          const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                          int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                          uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts,
                                          int64_t* points_sum, int64_t* gd_sum, int32_t* sim_points,
                                          uint8_t* sim_position, uint8_t* home_goals, uint8_t* away_goals, void* stream,
                                          const uint32_t* pair_init) {
    return guarded(c, "bplhip_simulate_season_h2h", [&] {
        return simulate_season_impl(c, SEASON_CALL((H2HRequest{true, pair_init})), SEASON_OUT);
    });
}
extern "C" int bplhip_simulate_season_playoff(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                              const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                              const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                              int32_t win_points, int32_t draw_points, int32_t loss_points,
                                              int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                              uint64_t* position_counts, int64_t* points_sum, int64_t* gd_sum,
                                              int32_t* sim_points, uint8_t* sim_position, uint8_t* home_goals,
                                              uint8_t* away_goals, void* stream, const uint32_t* pair_init,
                                              int32_t head_to_head, int32_t n_guests, const uint16_t* guest_idx,
                                              const uint16_t* bracket, int32_t rounds, uint32_t legs_mask,
                                              uint32_t neutral_mask, double extra_time_scale, int32_t away_goals_rule,
                                              const double* strength, uint64_t* stage_counts, uint64_t* decided_counts,
                                              uint8_t* sim_stage, uint8_t* sim_decided) {
    return guarded(c, "bplhip_simulate_season_playoff", [&] {
        const PlayoffRequest po{head_to_head, n_guests,     guest_idx,    bracket,        rounds,
                                legs_mask,    neutral_mask, extra_time_scale, away_goals_rule, strength,
                                stage_counts, decided_counts, sim_stage,  sim_decided};
        return simulate_season_impl(c, SEASON_CALL(head_to_head == 1 ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                    SEASON_OUT, &po);
    });
}
extern "C" int bplhip_simulate_season_live(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                           const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                           const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                           int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                           uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts,
                                           int64_t* points_sum, int64_t* gd_sum, int32_t* sim_points,
                                           uint8_t* sim_position, uint8_t* home_goals, uint8_t* away_goals, void* stream,
                                           const uint32_t* pair_init, int32_t head_to_head, int32_t n_in_play,
                                           const uint16_t* in_play_home_idx, const uint16_t* in_play_away_idx,
                                           const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                           const double* in_play_elapsed, int32_t reweight, const double* log_weights,
                                           double* ess, double* log_evidence, int32_t* sim_draw,
                                           double* draw_log_weights, double* draw_log_evidence) {
    return guarded(c, "bplhip_simulate_season_live", [&] {
        if (c && head_to_head != 0 && head_to_head != 1)
            return fail(c, BPLHIP_EINVAL, "simulate_season_live: head_to_head is 0 / 1");
        const LiveRequest lv{LIVE_IN, sim_draw, draw_log_weights, draw_log_evidence};
        return simulate_season_live_impl(c, SEASON_CALL(head_to_head == 1 ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                         SEASON_OUT, lv);
    });
}
extern "C" int bplhip_match_leverage_h2h(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                         const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                         const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                         int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                         uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                         int64_t chunk_sims, uint64_t* outcome_counts, uint64_t* target_counts,
                                         uint64_t* joint_counts, void* stream, const uint32_t* pair_init) {
    return guarded(c, "bplhip_match_leverage_h2h", [&] {
        return match_leverage_impl(c, SEASON_CALL((H2HRequest{true, pair_init})), {n_targets, target_mask, chunk_sims},
                                   outcome_counts, target_counts, joint_counts);
    });
}
extern "C" int bplhip_season_points(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                    const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                    const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                    int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                    uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                    int64_t chunk_sims, int32_t points_min, int32_t n_bins, uint64_t* team_points,
                                    uint64_t* team_target, uint64_t* position_points, uint64_t* gap, void* stream,
                                    const uint32_t* pair_init) {
    return guarded(c, "bplhip_season_points", [&] {
        return season_points_impl(c, SEASON_CALL(pair_init ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                  {n_targets, target_mask, chunk_sims}, points_min, n_bins, team_points, team_target,
                                  position_points, gap);
    });
}
extern "C" int bplhip_season_trajectory(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                        const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                        const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                        int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                        uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                        int64_t chunk_sims, int32_t points_min, int32_t n_bins, int32_t n_rounds,
                                        const int32_t* round_end, const int32_t* fix_id, uint64_t* position_count,
                                        uint64_t* target_count, uint64_t* target_final_count, uint64_t* points_sum,
                                        uint64_t* points_sq_sum, uint64_t* rounds_inside_count, uint64_t* secured_count,
                                        uint64_t* lead_changes_count, void* stream, const uint32_t* pair_init) {
    return guarded(c, "bplhip_season_trajectory", [&] {
        return season_trajectory_impl(c, SEASON_CALL(pair_init ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                      {n_targets, target_mask, chunk_sims}, points_min, n_bins, n_rounds, round_end, fix_id,
                                      TrajectoryOut{position_count, target_count, target_final_count, points_sum,
                                                    points_sq_sum, rounds_inside_count, secured_count, lead_changes_count});
    });
}
extern "C" int bplhip_season_scenarios(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                       const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                       const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                       int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                       uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                       int64_t chunk_sims, int32_t n_key, const int32_t* key_fixture,
                                       const int32_t* key_cap, uint64_t* scenario, uint64_t* joint, void* stream,
                                       const uint32_t* pair_init) {
    return guarded(c, "bplhip_season_scenarios", [&] {
        return season_scenarios_impl(c, SEASON_CALL(pair_init ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                     {n_targets, target_mask, chunk_sims}, n_key, key_fixture, key_cap, scenario, joint);
    });
}
// the live forms of the three queries: the head-to-head form's list, then the live request's inputs and outputs; a
// non-null pair_init asks for the head-to-head order, as bplhip_season_points reads it
extern "C" int bplhip_match_leverage_live(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                          const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                          const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                          int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                          uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                          int64_t chunk_sims, uint64_t* outcome_counts, uint64_t* target_counts,
                                          uint64_t* joint_counts, void* stream, const uint32_t* pair_init,
                                          int32_t n_in_play, const uint16_t* in_play_home_idx,
                                          const uint16_t* in_play_away_idx, const uint8_t* in_play_home_goals,
                                          const uint8_t* in_play_away_goals, const double* in_play_elapsed,
                                          int32_t reweight, const double* log_weights, double* ess, double* log_evidence) {
    return guarded(c, "bplhip_match_leverage_live", [&] {
        const LiveIn lv = LIVE_IN;
        return match_leverage_impl(c, SEASON_CALL(pair_init ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                   {n_targets, target_mask, chunk_sims}, outcome_counts, target_counts, joint_counts, &lv);
    });
}
extern "C" int bplhip_season_points_live(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                         const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                         const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                         int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                         uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                         int64_t chunk_sims, int32_t points_min, int32_t n_bins, uint64_t* team_points,
                                         uint64_t* team_target, uint64_t* position_points, uint64_t* gap, void* stream,
                                         const uint32_t* pair_init, int32_t n_in_play, const uint16_t* in_play_home_idx,
                                         const uint16_t* in_play_away_idx, const uint8_t* in_play_home_goals,
                                         const uint8_t* in_play_away_goals, const double* in_play_elapsed,
                                         int32_t reweight, const double* log_weights, double* ess, double* log_evidence) {
    return guarded(c, "bplhip_season_points_live", [&] {
        const LiveIn lv = LIVE_IN;
        return season_points_impl(c, SEASON_CALL(pair_init ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                  {n_targets, target_mask, chunk_sims}, points_min, n_bins, team_points, team_target,
                                  position_points, gap, &lv);
    });
}
extern "C" int bplhip_season_scenarios_live(bplhip_ctx* c, int64_t n_fixtures, const uint16_t* home_idx,
                                            const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                            const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                            int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                            uint32_t key_hi, uint32_t key_lo, int32_t n_targets,
                                            const uint64_t* target_mask, int64_t chunk_sims, int32_t n_key,
                                            const int32_t* key_fixture, const int32_t* key_cap, uint64_t* scenario,
                                            uint64_t* joint, void* stream, const uint32_t* pair_init, int32_t n_in_play,
                                            const uint16_t* in_play_home_idx, const uint16_t* in_play_away_idx,
                                            const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                            const double* in_play_elapsed, int32_t reweight, const double* log_weights,
                                            double* ess, double* log_evidence) {
    return guarded(c, "bplhip_season_scenarios_live", [&] {
        const LiveIn lv = LIVE_IN;
        return season_scenarios_impl(c, SEASON_CALL(pair_init ? (H2HRequest{true, pair_init}) : H2HRequest{}),
                                     {n_targets, target_mask, chunk_sims}, n_key, key_fixture, key_cap, scenario, joint,
                                     &lv);
    });
}
#undef LIVE_IN
#undef SEASON_CALL
#undef SEASON_OUT
extern "C" int bplhip_simulate_tournament_h2h(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                              const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                              const uint8_t* team_group, const int32_t* init_points,
                                              const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures,
                                              const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                              int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
                                              int32_t win_points, int32_t draw_points, int32_t loss_points,
                                              int64_t n_sims, uint32_t key_hi, uint32_t key_lo, uint64_t* stage_counts,
                                              uint64_t* group_position_counts, uint8_t* sim_stage, void* stream,
                                              const uint32_t* pair_init) {
    return guarded(c, "bplhip_simulate_tournament_h2h", [&] {
        return simulate_tournament_impl(c, TOURNAMENT_CALL((H2HRequest{true, pair_init})), TOURNAMENT_OUT);
    });
}
extern "C" int bplhip_simulate_tournament_knockout(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                                   const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                                   const uint8_t* team_group, const int32_t* init_points,
                                                   const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures,
                                                   const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                                   int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
                                                   int32_t win_points, int32_t draw_points, int32_t loss_points,
                                                   int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                                   uint64_t* stage_counts, uint64_t* group_position_counts,
                                                   uint8_t* sim_stage, void* stream, const uint32_t* pair_init,
                                                   int32_t head_to_head, uint32_t legs_mask, double extra_time_scale,
                                                   int32_t away_goals, const double* strength,
                                                   uint64_t* decided_counts, uint8_t* sim_decided) {
    return guarded(c, "bplhip_simulate_tournament_knockout", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, sim_decided};
        return simulate_tournament_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), TOURNAMENT_OUT, &ko);
    });
}
// bplhip_simulate_tournament_knockout's argument list with the flag extra_time (as bplhip_tournament_paths has it)
// and, last, the slot counts of the allocation in force
extern "C" int bplhip_simulate_tournament_alloc(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                                const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                                const uint8_t* team_group, const int32_t* init_points,
                                                const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures,
                                                const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                                int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
                                                int32_t win_points, int32_t draw_points, int32_t loss_points,
                                                int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                                uint64_t* stage_counts, uint64_t* group_position_counts,
                                                uint8_t* sim_stage, void* stream, const uint32_t* pair_init,
                                                int32_t head_to_head, int32_t extra_time, uint32_t legs_mask,
                                                double extra_time_scale, int32_t away_goals, const double* strength,
                                                uint64_t* decided_counts, uint8_t* sim_decided, uint64_t* slot_counts) {
    return guarded(c, "bplhip_simulate_tournament_alloc", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, sim_decided};
        if (c && !slot_counts) return fail(c, BPLHIP_EINVAL, "simulate_tournament: null required output");
        return simulate_tournament_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), TOURNAMENT_OUT, extra_time ? &ko : nullptr,
                                        slot_counts);
    });
}
// bplhip_simulate_tournament_alloc's argument list, then bplhip_simulate_season_live's request with the sides as slots
// and its outputs, then the final scores of the matches in play
extern "C" int bplhip_simulate_tournament_live(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                               const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                               const uint8_t* team_group, const int32_t* init_points,
                                               const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures,
                                               const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                               int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
                                               int32_t win_points, int32_t draw_points, int32_t loss_points,
                                               int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                               uint64_t* stage_counts, uint64_t* group_position_counts,
                                               uint8_t* sim_stage, void* stream, const uint32_t* pair_init,
                                               int32_t head_to_head, int32_t extra_time, uint32_t legs_mask,
                                               double extra_time_scale, int32_t away_goals, const double* strength,
                                               uint64_t* decided_counts, uint8_t* sim_decided, uint64_t* slot_counts,
                                               int32_t n_in_play, const uint8_t* in_play_p, const uint8_t* in_play_q,
                                               const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                               const double* in_play_elapsed, int32_t reweight,
                                               const double* log_weights, double* ess, double* log_evidence,
                                               int32_t* sim_draw, double* draw_log_weights, double* draw_log_evidence,
                                               uint8_t* in_play_final_home, uint8_t* in_play_final_away) {
    return guarded(c, "bplhip_simulate_tournament_live", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, sim_decided};
        const LiveIn in{n_in_play,       nullptr,  nullptr,     in_play_home_goals, in_play_away_goals,
                        in_play_elapsed, reweight, log_weights, ess,                log_evidence};
        const CupLiveRequest lr{LiveRequest{in, sim_draw, draw_log_weights, draw_log_evidence}, in_play_p, in_play_q,
                                in_play_final_home, in_play_final_away};
        return simulate_tournament_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), TOURNAMENT_OUT, extra_time ? &ko : nullptr,
                                        slot_counts, &lr);
    });
}
extern "C" int bplhip_tournament_paths(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                       const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                       const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                       const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                       const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                       const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                       int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                       uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage,
                                       void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                       int32_t extra_time, uint32_t legs_mask, double extra_time_scale,
                                       int32_t away_goals, const double* strength, uint64_t* decided_counts,
                                       uint8_t* sim_decided, int64_t chunk_sims, uint64_t* advance_counts,
                                       uint64_t* position_stage_counts, uint64_t* outcome_counts,
                                       uint64_t* target_counts, uint64_t* joint_counts, uint8_t* sim_position,
                                       uint8_t* sim_outcome, uint8_t* sim_pair, uint8_t* sim_winner) {
    return guarded(c, "bplhip_tournament_paths", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, sim_decided};
        const PathsRequest paths{chunk_sims, advance_counts, position_stage_counts, outcome_counts, target_counts,
                                 joint_counts, sim_position, sim_outcome, sim_pair, sim_winner};
        return tournament_paths_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), TOURNAMENT_OUT, extra_time ? &ko : nullptr, paths);
    });
}
extern "C" int bplhip_tournament_scenarios(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                           const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                           const uint8_t* team_group, const int32_t* init_points,
                                           const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures,
                                           const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                           int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
                                           int32_t win_points, int32_t draw_points, int32_t loss_points,
                                           int64_t n_sims, uint32_t key_hi, uint32_t key_lo, void* stream,
                                           const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time,
                                           uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                           const double* strength, uint64_t* decided_counts, int64_t chunk_sims,
                                           int32_t n_key, const int32_t* key_fixture, const int32_t* key_cap,
                                           uint64_t* scenario, uint64_t* joint, uint32_t* sim_scenario,
                                           uint8_t* sim_tset) {
    return guarded(c, "bplhip_tournament_scenarios", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, nullptr};
        const TscenRequest scen{chunk_sims, n_key, key_fixture, key_cap, scenario, joint, sim_scenario, sim_tset};
        return tournament_scenarios_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), extra_time ? &ko : nullptr, scen);
    });
}
extern "C" int bplhip_tournament_points(bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx,
                                        const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                        const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                        const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                        const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                        const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                        int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                        void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                        int32_t extra_time, uint32_t legs_mask, double extra_time_scale,
                                        int32_t away_goals, const double* strength, uint64_t* decided_counts,
                                        int64_t chunk_sims, int32_t points_min, int32_t n_bins, int32_t gd_cap,
                                        uint64_t* team_points, uint64_t* team_target, uint64_t* team_place,
                                        uint64_t* place_points, uint64_t* place_gap, uint64_t* rest_count,
                                        uint64_t* rest_through, uint64_t* rest_rank) {
    return guarded(c, "bplhip_tournament_points", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, nullptr};
        const GptsRequest gpts{chunk_sims, points_min, n_bins, gd_cap, team_points, team_target, team_place,
                               place_points, place_gap, rest_count, rest_through, rest_rank};
        return tournament_points_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), extra_time ? &ko : nullptr, gpts);
    });
}
// the three queries' kick-off argument lists, then bplhip_simulate_tournament_live's live block without the outputs
// a query lacks: n_in_play .. log_evidence, and for the two with per-simulation records sim_draw and the final scores
extern "C" int bplhip_tournament_paths_live(
        bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
        const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group, const int32_t* init_points,
        const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
        const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
        int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
        uint32_t key_lo, uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage, void* stream,
        const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time, uint32_t legs_mask,
        double extra_time_scale, int32_t away_goals, const double* strength, uint64_t* decided_counts,
        uint8_t* sim_decided, int64_t chunk_sims, uint64_t* advance_counts, uint64_t* position_stage_counts,
        uint64_t* outcome_counts, uint64_t* target_counts, uint64_t* joint_counts, uint8_t* sim_position,
        uint8_t* sim_outcome, uint8_t* sim_pair, uint8_t* sim_winner, int32_t n_in_play, const uint8_t* in_play_p,
        const uint8_t* in_play_q, const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
        const double* in_play_elapsed, int32_t reweight, const double* log_weights, double* ess,
        double* log_evidence, int32_t* sim_draw, uint8_t* in_play_final_home, uint8_t* in_play_final_away) {
    return guarded(c, "bplhip_tournament_paths_live", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, sim_decided};
        const PathsRequest paths{chunk_sims, advance_counts, position_stage_counts, outcome_counts, target_counts,
                                 joint_counts, sim_position, sim_outcome, sim_pair, sim_winner};
        const LiveIn in{n_in_play,       nullptr,  nullptr,     in_play_home_goals, in_play_away_goals,
                        in_play_elapsed, reweight, log_weights, ess,                log_evidence};
        const CupLiveRequest lr{LiveRequest{in, sim_draw, nullptr, nullptr}, in_play_p, in_play_q, in_play_final_home,
                                in_play_final_away};
        return tournament_paths_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), TOURNAMENT_OUT, extra_time ? &ko : nullptr, paths,
                                     &lr);
    });
}
extern "C" int bplhip_tournament_scenarios_live(
        bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
        const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group, const int32_t* init_points,
        const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
        const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
        int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
        uint32_t key_lo, void* stream, const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time,
        uint32_t legs_mask, double extra_time_scale, int32_t away_goals, const double* strength,
        uint64_t* decided_counts, int64_t chunk_sims, int32_t n_key, const int32_t* key_fixture,
        const int32_t* key_cap, uint64_t* scenario, uint64_t* joint, uint32_t* sim_scenario, uint8_t* sim_tset,
        int32_t n_in_play, const uint8_t* in_play_p, const uint8_t* in_play_q, const uint8_t* in_play_home_goals,
        const uint8_t* in_play_away_goals, const double* in_play_elapsed, int32_t reweight,
        const double* log_weights, double* ess, double* log_evidence, int32_t* sim_draw, uint8_t* in_play_final_home,
        uint8_t* in_play_final_away) {
    return guarded(c, "bplhip_tournament_scenarios_live", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, nullptr};
        const TscenRequest scen{chunk_sims, n_key, key_fixture, key_cap, scenario, joint, sim_scenario, sim_tset};
        const LiveIn in{n_in_play,       nullptr,  nullptr,     in_play_home_goals, in_play_away_goals,
                        in_play_elapsed, reweight, log_weights, ess,                log_evidence};
        const CupLiveRequest lr{LiveRequest{in, sim_draw, nullptr, nullptr}, in_play_p, in_play_q, in_play_final_home,
                                in_play_final_away};
        return tournament_scenarios_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), extra_time ? &ko : nullptr, scen, &lr);
    });
}
extern "C" int bplhip_tournament_points_live(
        bplhip_ctx* c, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
        const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group, const int32_t* init_points,
        const int32_t* init_gf, const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
        const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket,
        int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
        uint32_t key_lo, void* stream, const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time,
        uint32_t legs_mask, double extra_time_scale, int32_t away_goals, const double* strength,
        uint64_t* decided_counts, int64_t chunk_sims, int32_t points_min, int32_t n_bins, int32_t gd_cap,
        uint64_t* team_points, uint64_t* team_target, uint64_t* team_place, uint64_t* place_points,
        uint64_t* place_gap, uint64_t* rest_count, uint64_t* rest_through, uint64_t* rest_rank, int32_t n_in_play,
        const uint8_t* in_play_p, const uint8_t* in_play_q, const uint8_t* in_play_home_goals,
        const uint8_t* in_play_away_goals, const double* in_play_elapsed, int32_t reweight,
        const double* log_weights, double* ess, double* log_evidence) {
    return guarded(c, "bplhip_tournament_points_live", [&] {
        const KnockoutRequest ko{legs_mask, extra_time_scale, away_goals, strength, decided_counts, nullptr};
        const GptsRequest gpts{chunk_sims, points_min, n_bins, gd_cap, team_points, team_target, team_place,
                               place_points, place_gap, rest_count, rest_through, rest_rank};
        const LiveIn in{n_in_play,       nullptr,  nullptr,     in_play_home_goals, in_play_away_goals,
                        in_play_elapsed, reweight, log_weights, ess,                log_evidence};
        const CupLiveRequest lr{LiveRequest{in, nullptr, nullptr, nullptr}, in_play_p, in_play_q, nullptr, nullptr};
        return tournament_points_impl(c, TOURNAMENT_CALL(TOURNAMENT_H2H), extra_time ? &ko : nullptr, gpts, &lr);
    });
}
#undef TOURNAMENT_CALL
#undef TOURNAMENT_H2H
#undef TOURNAMENT_OUT
// ---- the best-of-rest allocation of the tournament family: kept on the context, as the posterior is, and staged
// into the call record of every tournament entry while set.  Checked here for what the kernels index with -- every
// mask's row inside the table, every row's slots a permutation over its own mask's groups -- and in tournament_setup
// against the call's shape
extern "C" int bplhip_tournament_set_allocation(bplhip_ctx* c, int32_t n_groups, int32_t best, int32_t n_rows,
                                                const uint16_t* row_of_mask, const uint8_t* slots) {
    return guarded(c, "bplhip_tournament_set_allocation", [&] {
        if (!c) return (int)BPLHIP_EINVAL;
        if (!row_of_mask || !slots) {
            if (row_of_mask || slots || n_rows != 0)
                return fail(c, BPLHIP_EINVAL, "tournament_set_allocation: both tables and n_rows, or neither");
            c->alloc_groups = c->alloc_best = c->alloc_rows = 0;
            c->alloc_row.clear();
            c->alloc_slot.clear();
            return (int)BPLHIP_OK;
        }
        if (n_groups < 1 || n_groups > BPLHIP_TOURNAMENT_MAX_GROUPS || best < 1 || best > n_groups)
            return fail(c, BPLHIP_EINVAL, "tournament_set_allocation: n_groups=%d out of range [1,%d] or best=%d not in [1,n_groups]",
                        n_groups, BPLHIP_TOURNAMENT_MAX_GROUPS, best);
        if (n_rows < 1 || n_rows > BPLHIP_TOURNAMENT_MAX_ALLOCATION_ROWS)
            return fail(c, BPLHIP_EINVAL, "tournament_set_allocation: n_rows=%d out of range [1,%d]", n_rows,
                        BPLHIP_TOURNAMENT_MAX_ALLOCATION_ROWS);
        const uint32_t n_masks = 1u << n_groups;
        for (uint32_t m = 0; m < n_masks; ++m)
            if (row_of_mask[m] >= n_rows)
                return fail(c, BPLHIP_EINVAL, "tournament_set_allocation: row_of_mask[0x%x]=%d is no row", m, (int)row_of_mask[m]);
        for (int r = 0; r < n_rows; ++r) {
            uint32_t mask = 0u, used = 0u;
            for (int g = 0; g < n_groups; ++g) {
                const uint8_t v = slots[(size_t)r * n_groups + g];
                if (v == 0xFF) continue;
                if (v >= best || ((used >> v) & 1u))
                    return fail(c, BPLHIP_EINVAL, "tournament_set_allocation: row %d is not a permutation of %d slots", r, best);
                used |= 1u << v;
                mask |= 1u << g;
            }
            if (__builtin_popcount(mask) != best || row_of_mask[mask] != r)
                return fail(c, BPLHIP_EINVAL, "tournament_set_allocation: row %d has %d groups, not %d, or its mask 0x%x "
                            "names another row", r, __builtin_popcount(mask), best, mask);
        }
        c->alloc_groups = n_groups;
        c->alloc_best = best;
        c->alloc_rows = n_rows;
        c->alloc_row.assign(row_of_mask, row_of_mask + n_masks);
        c->alloc_slot.assign(slots, slots + (size_t)n_rows * n_groups);
        return (int)BPLHIP_OK;
    });
}
extern "C" int bplhip_ppc(bplhip_ctx* c, const bplhip_fixtures* q, const uint16_t* home_slot, const uint16_t* away_slot,
                          const uint32_t* fixture_id, int32_t n_slots, int32_t max_goals, int64_t n_reps,
                          uint32_t key_hi, uint32_t key_lo, uint32_t* score_counts, uint32_t* outcome_counts,
                          int64_t* goal_sums, uint32_t* team_counts, uint8_t* home_goals, uint8_t* away_goals,
                          void* stream) {
    return guarded(c, "bplhip_ppc", [&] {
        return ppc_any(c, q, home_slot, away_slot, fixture_id, n_slots, max_goals, n_reps, key_hi, key_lo, score_counts,
                       outcome_counts, goal_sums, team_counts, home_goals, away_goals, stream);
    });
}
extern "C" int bplhip_loglik_matrix(bplhip_ctx* c, const bplhip_fixtures* q, double* out, void* stream) {
    return guarded(c, "bplhip_loglik_matrix", [&] {
        return loglik_any(c, q, false, out, 1.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    });
}
extern "C" int bplhip_loglik_summary(bplhip_ctx* c, const bplhip_fixtures* q, double r_eff, int32_t psis, double* lppd,
                                     double* mean, double* var, double* elpd_loo, double* pareto_k, int32_t* tail_len,
                                     void* stream) {
    return guarded(c, "bplhip_loglik_summary", [&] {
        return loglik_any(c, q, true, nullptr, r_eff, psis, lppd, mean, var, elpd_loo, pareto_k, tail_len, stream);
    });
}
extern "C" int bplhip_outcome_scores(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, double* proba,
                                     double* draw_sums, void* stream) {
    return guarded(c, "bplhip_outcome_scores", [&] { return outcome_scores_any(c, q, max_goals, proba, draw_sums, stream); });
}
extern "C" int bplhip_loo_scores(bplhip_ctx* c, const bplhip_fixtures* q, double r_eff, int32_t max_goals, double* elpd_loo,
                                 double* pareto_k, int32_t* tail_len, double* ess, double* proba, double* proba_in_sample,
                                 double* pit, void* stream) {
    return guarded(c, "bplhip_loo_scores", [&] {
        return loo_scores_any(c, q, r_eff, max_goals, elpd_loo, pareto_k, tail_len, ess, proba, proba_in_sample, pit, stream);
    });
}
extern "C" int bplhip_block_loglik(bplhip_ctx* c, const bplhip_fixtures* q, const int32_t* block_idx, int32_t n_blocks,
                                   double* out, void* stream) {
    return guarded(c, "bplhip_block_loglik", [&] {
        return seq_any(c, q, block_idx, n_blocks, out, nullptr, 0, nullptr, nullptr, stream);
    });
}
extern "C" int bplhip_psis_weights(bplhip_ctx* c, int32_t n_blocks, int32_t n_draws, const double* log_ratios,
                                   double r_eff, double* log_weights, double* pareto_k, double* ess,
                                   int32_t* tail_len, void* stream) {
    return guarded(c, "bplhip_psis_weights", [&] {
        return psis_weights_any(c, n_blocks, n_draws, log_ratios, r_eff, log_weights, pareto_k, ess, tail_len, stream);
    });
}
extern "C" int bplhip_weighted_scores(bplhip_ctx* c, const bplhip_fixtures* q, const int32_t* block_idx,
                                      int32_t n_blocks, const double* log_weights, int32_t max_goals, double* elpd,
                                      double* proba, void* stream) {
    return guarded(c, "bplhip_weighted_scores", [&] {
        // (a null output makes the call malformed, not a block-sum call)
        if (c && (!log_weights || !elpd || !proba)) return fail(c, BPLHIP_EINVAL, "weighted_scores: a null argument");
        return seq_any(c, q, block_idx, n_blocks, nullptr, log_weights, max_goals, elpd, proba, stream);
    });
}
extern "C" int bplhip_mcmc_diagnostics(bplhip_ctx* c, int32_t n_chains, int32_t n_draws, int64_t n_quantities,
                                       const double* values, int32_t n_quantiles, const double* quantiles,
                                       int64_t workspace_bytes, double* mean, double* sd, double* rhat,
                                       double* ess_bulk, double* ess_tail, double* ess_mean, double* mcse_mean,
                                       void* stream) {
    return guarded(c, "bplhip_mcmc_diagnostics", [&] {
        return mcmc_diagnostics_any(c, n_chains, n_draws, n_quantities, values, n_quantiles, quantiles, workspace_bytes,
                                    mean, sd, rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, stream);
    });
}
extern "C" int bplhip_weighted_shift(bplhip_ctx* c, int32_t n_draws, int64_t n_quantities, const double* values,
                                     int32_t n_rows, const double* log_ratios, double r_eff, int64_t workspace_bytes,
                                     double* log_weights, double* pareto_k, double* ess, int32_t* tail_len,
                                     double* cjs_sq, double* mean, double* sd, void* stream) {
    return guarded(c, "bplhip_weighted_shift", [&] {
        return weighted_shift_any(c, n_draws, n_quantities, values, n_rows, log_ratios, r_eff, workspace_bytes,
                                  log_weights, pareto_k, ess, tail_len, cjs_sq, mean, sd, stream);
    });
}
extern "C" int bplhip_market_summary(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, int32_t n_markets,
                                     const double* weights, int32_t n_quantiles, const double* quantiles, double* mean,
                                     double* sd, double* quantile, double* draws, int64_t workspace_bytes,
                                     void* stream) {
    return guarded(c, "bplhip_market_summary", [&] {
        return market_summary_any(c, q, max_goals, n_markets, weights, n_quantiles, quantiles, mean, sd, quantile, draws,
                                  workspace_bytes, stream);
    });
}
extern "C" int bplhip_period_summary(bplhip_ctx* c, const bplhip_fixtures* q, const double* split, int32_t max_goals,
                                     int32_t n_markets, const double* weights, int32_t n_quantiles,
                                     const double* quantiles, double* mean, double* sd, double* quantile, double* draws,
                                     int64_t workspace_bytes, void* stream) {
    return guarded(c, "bplhip_period_summary", [&] {
        return period_summary_any(c, q, split, max_goals, n_markets, weights, n_quantiles, quantiles, mean, sd, quantile,
                                  draws, workspace_bytes, stream);
    });
}
extern "C" int bplhip_slate_summary(bplhip_ctx* c, const bplhip_fixtures* q, int32_t max_goals, int32_t n_slates,
                                    const int32_t* start, int32_t n_tables, const uint8_t* tables,
                                    const int32_t* leg_table, int32_t n_quantiles, const double* quantiles, double* mean,
                                    double* sd, double* quantile, double* leg_mean, double* draws,
                                    int64_t workspace_bytes, void* stream) {
    return guarded(c, "bplhip_slate_summary", [&] {
        return slate_summary_any(c, q, max_goals, n_slates, start, n_tables, tables, leg_table, n_quantiles, quantiles,
                                 mean, sd, quantile, leg_mean, draws, workspace_bytes, stream);
    });
}
extern "C" int bplhip_team_ratings(bplhip_ctx* c, int32_t n_teams, const uint16_t* teams, const uint16_t* team_conf,
                                   int32_t n_opponents, const uint16_t* opponents, const uint16_t* opponent_conf,
                                   int32_t venue, int32_t max_goals, const double* points, int32_t rank_by,
                                   int32_t n_quantiles, const double* quantiles, double* mean, double* sd,
                                   double* quantile, int32_t* rank_count, int32_t* better_count, int32_t* matches,
                                   double* draws, int64_t workspace_bytes, void* stream) {
    return guarded(c, "bplhip_team_ratings", [&] {
        return team_ratings_any(c, n_teams, teams, team_conf, n_opponents, opponents, opponent_conf, venue, max_goals,
                                points, rank_by, n_quantiles, quantiles, mean, sd, quantile, rank_count, better_count,
                                matches, draws, workspace_bytes, stream);
    });
}
extern "C" int bplhip_inplay_summary(bplhip_ctx* c, const bplhip_fixtures* q, const double* elapsed, int32_t max_goals,
                                     int32_t n_markets, const double* weights, int32_t n_quantiles,
                                     const double* quantiles, int32_t reweight, const double* log_weights, double* mean,
                                     double* sd, double* quantile, double* ess, double* log_evidence, double* draws,
                                     double* draw_log_evidence, int64_t workspace_bytes, void* stream) {
    return guarded(c, "bplhip_inplay_summary", [&] {
        return inplay_summary_any(c, q, elapsed, max_goals, n_markets, weights, n_quantiles, quantiles, reweight,
                                  log_weights, mean, sd, quantile, ess, log_evidence, draws, draw_log_evidence,
                                  workspace_bytes, stream);
    });
}
