/* bplhip.h -- C-ABI of libbplhip.so: the MI355X (gfx950) Dixon-Coles log-density +
 * gradient path and the NUTS driver around it.
 *
 * The reference (anguswilliams91/bpl-next) is pure Python over numpyro/JAX and has NO
 * FFI layer of its own; the seam this library replaces is numpyro's
 * `value_and_grad(potential_fn)(z)` call made once per leapfrog step by
 * `NUTS(self._model)` / `MCMC(...).run(...)`:
 *     bpl/dixon_coles.py:100-116            (basic model driver)
 *     bpl/extended_dixon_coles.py:293-316   (extended model driver)
 * Each entry point below cites the reference code whose work it takes over.
 *
 * Conventions
 *   - plain C linkage, plain pointers and sizes, no C++/torch types;
 *   - every function returns 0 (BPLHIP_OK) or a negative BPLHIP_E* code; the message
 *     is kept per context (bplhip_last_error); no exception or abort crosses the ABI;
 *   - "device" pointers are HIP device pointers owned by the caller (e.g.
 *     torch.Tensor.data_ptr()); "host" pointers are ordinary host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All device
 *     work is enqueued on it; functions documented "asynchronous" do not synchronise;
 *   - a context is bound to one device and is not thread-safe; distinct contexts may be
 *     used concurrently from distinct host threads;
 *   - a non-finite potential is NOT an error (NUTS treats it as a divergence): it is
 *     returned as +inf / nan.
 *
 * Latent vector layout (flat, numpyro's sorted-site-name order; all float64):
 *   basic    attack_decentered[T], corr_coef_raw, defence_decentered[T], home_advantage,
 *            mean_defence, std_attack, std_defence                         D = 2T+5
 *   extended attack_coefficients[K], corr_coef_raw, defence_coefficients[K],
 *            home_advantage_decentered[T], mean_defence, mean_home_advantage,
 *            standardised_attack[T], standardised_defence[T], std_attack, std_defence,
 *            std_home_advantage, u                                         D = 3T+2K+7
 */
#ifndef BPLHIP_H
#define BPLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPLHIP_ABI_VERSION 2

enum {
    BPLHIP_OK = 0,
    BPLHIP_EINVAL = -1,   /* bad argument (null pointer, size, index out of range) */
    BPLHIP_ESTATE = -2,   /* call out of order (e.g. logp_grad before set_fixtures) */
    BPLHIP_EHIP = -3,     /* a HIP runtime call failed, or a device-side hand-off timed out
                           * (the kernels' waits for each other are bounded; one that expires raises a
                           * host-visible fault word which the NEXT entry point -- or the running
                           * sampler at its next synchronisation -- reports and clears; the affected
                           * evaluations' outputs are NaN); see bplhip_last_error  */
    BPLHIP_ENOMEM = -4,
    BPLHIP_EUNSUPPORTED = -5,
    BPLHIP_ENUMERIC = -6  /* NUTS could not find a finite initial point            */
};

enum {
    BPLHIP_MODEL_BASIC = 0,    /* bpl/dixon_coles.py:39-84           */
    BPLHIP_MODEL_EXTENDED = 1, /* bpl/extended_dixon_coles.py:78-248 */
    BPLHIP_MODEL_DYNAMIC = 2,  /* bpl/dynamic_dixon_coles.py:63-247 (bound through
                                  bplhip_set_fixtures_dynamic)       */
    BPLHIP_MODEL_NEUTRAL = 3   /* bpl/neutral_dixon_coles.py:102-283 (bound through
                                  bplhip_set_fixtures_neutral)       */
};

/* The form an evaluation was launched in (bplhip_last_eval_path).  The host picks it from the bound data
 * and the options; the values of one model all compute the same U and gradient. */
enum {
    BPLHIP_PATH_NONE = 0,              /* nothing evaluated since the fixtures were bound            */
    BPLHIP_PATH_LEAGUE = 1,            /* basic / extended model (dc_eval, dc_vec)                   */
    BPLHIP_PATH_NEU_FUSED = 2,         /* neutral: one workgroup per chain, everything in LDS        */
    BPLHIP_PATH_NEU_BIG_RUNS = 3,      /* neutral: sliced single launch, per-run arithmetic          */
    BPLHIP_PATH_NEU_BIG_FIXTURE = 4,   /* neutral: sliced single launch, per-fixture arithmetic      */
    BPLHIP_PATH_NEU_MULTI = 5,         /* neutral: four launches                                     */
    BPLHIP_PATH_DYN_FUSED_GATHER = 6,  /* dynamic: small single launch, adjoint records + gather     */
    BPLHIP_PATH_DYN_FUSED_ATOMICS = 7, /* dynamic: small single launch, float64 atomics              */
    BPLHIP_PATH_DYN_SLICED = 8,        /* dynamic: sliced single launch                              */
    BPLHIP_PATH_DYN_MULTI = 9          /* dynamic: four launches                                     */
};

/* The engine a sampler run was dispatched to (bplhip_last_nuts_engine).  The host picks it from the bound
 * model's latent size, the chain count and the options; all of them walk the same trajectories. */
enum {
    BPLHIP_ENGINE_NONE = 0,             /* no sampler run since the fixtures were bound                        */
    BPLHIP_ENGINE_HOST_TREE = 1,        /* tree and adaptation on the host, one evaluation per leapfrog        */
    BPLHIP_ENGINE_DEVICE_TREE = 2,      /* tree in dc_eval's tail, one launch per leapfrog, host adaptation    */
    BPLHIP_ENGINE_LOOP_LNE1 = 3,        /* persistent chain, dc_eval_loop, one leaf element per lane           */
    BPLHIP_ENGINE_LOOP_LNE2 = 4,        /* persistent chain, dc_eval_loop, two leaf elements per lane          */
    BPLHIP_ENGINE_PERSIST_TAIL = 5,     /* persistent chain, leaf in dc_eval's tail, one launch per leapfrog   */
    BPLHIP_ENGINE_PERSIST_GRIDY = 6,    /* persistent chains as grid.y copies of the single-chain launch       */
    BPLHIP_ENGINE_PERSIST_VEC = 7,      /* persistent chains in the chain-vectorised kernel                    */
    BPLHIP_ENGINE_PERSIST_KP_LEAF = 8,  /* persistent chains, the leaf as its own one-wave launch (kp_leaf)    */
    BPLHIP_ENGINE_PERSIST_KW_LEAF = 9,  /* persistent chains, the leaf as its own multi-workgroup launch       */
    BPLHIP_ENGINE_LOCKSTEP_VEC = 10,    /* lock-step chains in the chain-vectorised kernel, host adaptation    */
    BPLHIP_ENGINE_PERSIST_NEU_FUSED = 11 /* persistent neutral chains, evaluation and leaf in one launch       */
};

typedef struct bplhip_ctx bplhip_ctx;

/* ABI version of the loaded library (== BPLHIP_ABI_VERSION of the header it was built
 * against). */
int bplhip_abi_version(void);

/* Create / destroy a context on HIP device `device_id`. */
int bplhip_create(bplhip_ctx** out, int device_id);
void bplhip_destroy(bplhip_ctx* ctx);

/* Last error message of this context ("" if none); `ctx` may be NULL for the message of
 * a failed bplhip_create. The pointer stays valid until the next call on the context. */
const char* bplhip_last_error(const bplhip_ctx* ctx);

/* Bind the model arguments.  Replaces the concrete (non-traced) arguments the reference
 * hands to `mcmc.run(...)`: bpl/dixon_coles.py:108-116 (home_ind, away_ind, num_teams,
 * home_goals, away_goals) and bpl/extended_dixon_coles.py:303-316 (+ team_covariates,
 * weights = exp(-epsilon*time_diff), optionally rescaled: :202-205).
 *
 *   home_idx/away_idx  device u16[n]  team indices in [0, n_teams) -- the reference's
 *                                     storage dtype, bpl/base.py:16-22, parse_teams
 *                                     bpl/_util.py:115-135
 *   home_goals/away_goals device u8[n]
 *   weights            device f32[n] or NULL (unweighted)
 *   covariates         HOST f64[n_teams*k] row-major, ALREADY standardised
 *                      (bpl/extended_dixon_coles.py:124-127), or NULL with k = 0;
 *                      must be NULL for the basic model
 *
 * The arrays are read once (synchronously on `stream`) and re-laid-out into a library
 * owned SoA copy (sorted by (home,away) pair, every pair's run padded to the lane width,
 * the whole padded to the tile size); the caller's buffers are not referenced after the
 * call returns.  (The padding fixtures carry goals 255-255 and weight 0; a real 255-255 fixture is
 * legal -- which fixtures of a lane are real is recorded separately.) */
int bplhip_set_fixtures(bplhip_ctx* ctx, int model_kind, int64_t n, int32_t n_teams,
                        const uint16_t* home_idx, const uint16_t* away_idx,
                        const uint8_t* home_goals, const uint8_t* away_goals,
                        const float* weights, const double* covariates, int32_t k,
                        void* stream);

/* Bind the arguments of the dynamic (time-varying, neutral-venue) model,
 * bpl/dynamic_dixon_coles.py:63-247 as run at :286-300: per-gameweek hyper-parameters,
 * [G,T] tables, `gameweek` (0-based, device u16[n]) and `neutral_venue` (device u8[n], 0/1).
 * Latent layout (sorted site names, D = 7GT + 10G + 2 + 2K): attack_coefficients[K],
 * away_attack_decentered[G,T], away_defence_decentered[G,T], corr_coef_raw,
 * defence_coefficients[K], home_attack_decentered[G,T], home_defence_decentered[G,T],
 * mean_away_attack[G], mean_away_defence[G], mean_defence, mean_home_attack[G],
 * mean_home_defence[G], standardised_attack[G,T], standardised_defence[G,T], std_attack[G],
 * std_away_attack[G], std_away_defence[G], std_defence[G], std_home_attack[G],
 * std_home_defence[G], u[G,T].  `random_walk` 1 = the INTENDED model, attack[g] = attack[g-1] +
 * standardised_attack[g]*std_attack[g] (:192-218 discard that update);
 * 0 = the code as written (attack = defence = 0).  After this call logp_grad / nuts_run
 * work on the dynamic model; draws are mapped by bplhip_constrain_dynamic. */
int bplhip_set_fixtures_dynamic(bplhip_ctx* ctx, int64_t n, int32_t n_teams,
                                int32_t n_gameweeks, const uint16_t* home_idx,
                                const uint16_t* away_idx, const uint8_t* home_goals,
                                const uint8_t* away_goals, const uint16_t* gameweek,
                                const uint8_t* neutral_venue, const double* covariates,
                                int32_t k, int32_t random_walk, void* stream);

/* Dynamic model: HOST draws f64[s, D] -> constrained/deterministic sites f64[s, G, T]
 * (any output may be NULL): attack, defence (`attack_j`/`defence_j` of :195-218),
 * home_attack, away_attack, home_defence, away_defence (:142-189). */
int bplhip_constrain_dynamic(bplhip_ctx* ctx, const double* z_draws, int64_t s,
                             double* attack, double* defence, double* home_attack,
                             double* away_attack, double* home_defence,
                             double* away_defence);

/* Bind the arguments of the neutral-venue model, bpl/neutral_dixon_coles.py:102-283 as run
 * at :342-356: `neutral_venue` device u8[n] (0/1), `weights` device f32[n] = the final
 * per-fixture weights (time decay x game weights, :251-257; NULL = all ones), covariates as
 * for the extended model.  Latent layout (sorted site names, D = 6T + 2K + 13):
 * attack_coefficients[K], away_attack_decentered[T], away_defence_decentered[T],
 * corr_coef_raw, defence_coefficients[K], home_attack_decentered[T],
 * home_defence_decentered[T], mean_away_attack, mean_away_defence, mean_defence,
 * mean_home_attack, mean_home_defence, standardised_attack[T], standardised_defence[T],
 * std_attack, std_away_attack, std_away_defence, std_defence, std_home_attack,
 * std_home_defence, u.  World-Cup variant (bpl/neutral_dixon_coles_WC.py:83-232): `home_conf`,
 * `away_conf` device u8[n] confederation indices and n_conf > 0 add the site
 * confederation_strength_decentered[n_conf] (after away_defence_decentered, D += n_conf);
 * NULL, NULL, 0 for the plain neutral model.  After this call logp_grad / nuts_run work on
 * the neutral model. */
int bplhip_set_fixtures_neutral(bplhip_ctx* ctx, int64_t n, int32_t n_teams,
                                const uint16_t* home_idx, const uint16_t* away_idx,
                                const uint8_t* home_goals, const uint8_t* away_goals,
                                const uint8_t* neutral_venue, const uint8_t* home_conf,
                                const uint8_t* away_conf, int32_t n_conf, const float* weights,
                                const double* covariates, int32_t k, void* stream);

/* Tuning knobs (no reference counterpart; defaults are the measured best):
 *   "device_nuts" 1 (default) = NUTS tree builder on the device for every model: leaf
 *            bookkeeping in the tail of the evaluation kernel (basic/extended models,
 *            n_teams <= 64) or in leaf launches after it (everything else);
 *            0 = host tree builder (one read-back per leapfrog; the cross-check engine).
 *   "persistent_nuts" 1 (default) = the whole chain on the device (adaptation included, the
 *            host only enqueues evaluations); 0 = device trees with host-side adaptation
 *            (models of the evaluation kernel's tail only).
 *   "persistent_kernel" 1 (default) = one resident chain of the basic / extended model runs its
 *            leapfrogs INSIDE one launch (the streaming workgroups poll the next position);
 *            0 = one launch per leapfrog.
 *   "persist_spec" 1 (default) = inside that resident launch the next position goes out as soon as
 *            the gradient exists and the leaf is booked beside the next step's prior part (a U-turn or
 *            divergence -- once per transition -- discards one evaluation); 0 = leaf first, then publish
 *   "fused_small" 1 (default) = neutral / dynamic evaluations run as ONE launch: small ones on
 *            one workgroup per chain with everything in LDS (neutral) / one workgroup per four
 *            teams with phases behind grid barriers (dynamic), larger ones sliced over all CUs
 *            (a slice of the fixtures per workgroup, tree barriers) while the slices fit the LDS;
 *            0 = always the multi-launch path.
 *   "dyn_gather" 1 (default) = the dynamic model's small single launch hands the adjoints over as one
 *            16-byte record per fixture and gathers them per cell (host-built incidence lists; taken when no
 *            cell takes part in more than 16 fixtures); 0 = float64 atomics into the cells' accumulators
 *   "neu_runs" 1 (default) = the neutral model's sliced single launch works rates, tau terms and adjoints
 *            out once per (venue, home, away) run from seven sums over the run's fixtures (taken when every
 *            wave's part of the slice holds at most 15 runs); 0 = per fixture
 *   "dyn_big_wgs" 0 (default) = the sliced single launch uses one workgroup per CU, and the
 *            dynamic model takes it past 1024 fixtures per team workgroup; > 0 = that many
 *            workgroups, and the dynamic model takes the sliced form whatever its size.
 *   "dense_pairs" 1 (default) = a complete pair table (every ordered pair h != a present) of 4096
 *            pairs or more -- every complete table past 64 teams -- takes the rho bounds from the
 *            top two table entries per role (O(teams)); 0 = always walk the pair table.
 *   "pair_order" -1 (default) = past 64 teams the fixtures are laid out along the Z-order curve over
 *            (home, away), so that a workgroup's slice touches ~sqrt of its pairs' teams; up to 64
 *            teams in (home, away) order.  0 / 1 = (home, away) / Z-order whatever the league's
 *            size.  Applies at the next bplhip_set_fixtures; results do not depend on it beyond
 *            the order of the float32 run sums.
 *   "max_wg" streaming workgroups per evaluation, 1..255 (default 255: with the prior workgroup
 *            one per CU; an accumulator row counts its contributors in 8 bits); applies at the next
 *            bplhip_set_fixtures
 *   "gridy_max_chains" 8 (default) = bplhip_nuts_run_chains keeps up to this many chains as grid.y
 *            copies of the single-chain NUTS-aware launch; more share the chain-vectorised kernel
 *   "vec_min_chains" 12 (default) = bplhip_logp_grad_batched takes the chain-vectorised kernel
 *            (dc_vec: the fixtures are read once per 8 chains) from this many chains on; 0 = never
 *   "vec_tiles_per_wave" 0 (default) = the chain-vectorised partitions scale with the chain count
 *            (1x / 2x / 3x the single-chain tiles per wave, the thinnest whose grid fits the chip in one round); > 0 = this many; next bplhip_set_fixtures
 *   "chunk_graph" 1 (default) = a persistent sampler replays its chunk of 256 leapfrog launches as
 *            ONE hipGraph (falls back to plain launches by itself if a capture fails); 0 = always
 *            launch by launch
 *   "debug_raise_fault" test hook: ORs `value` into the context's fault word, as a kernel whose
 *            bounded wait expired would (the next entry point returns BPLHIP_EHIP)
 *   "active_waves" waves per workgroup that own tiles: 0 (default) = automatic -- short
 *            streams get a second partition with 4 of 8 waves owning tiles, used while the
 *            launch's workgroups still find a CU each; 1..8 = one fixed partition; applies
 *            at the next bplhip_set_fixtures
 * Which form these knobs and the data selected for the last evaluation: bplhip_last_eval_path. */
int bplhip_set_option(bplhip_ctx* ctx, const char* name, int value);

/* D of the bound model (negative error code if no fixtures are bound). */
int bplhip_latent_dim(const bplhip_ctx* ctx);

/* BPLHIP_PATH_* of the evaluation enqueued last on this context (of its last chain, for a batched call);
 * host bookkeeping only: no device traffic, no synchronisation.  BPLHIP_EINVAL for a NULL context. */
int bplhip_last_eval_path(const bplhip_ctx* ctx);

/* BPLHIP_ENGINE_* of the sampler run dispatched last on this context (bplhip_nuts_run / _chains); set by the
 * host where the dispatch is made, reset where the evaluation path is.  Nothing on the device reads it. */
int bplhip_last_nuts_engine(const bplhip_ctx* ctx);

/* THE HOT PATH.  U(z) = -log p(z, data) in unconstrained space and dU/dz -- what
 * numpyro's `value_and_grad(potential_fn)(z)` computes once per leapfrog from the model
 * declared at bpl/dixon_coles.py:39-84 / bpl/extended_dixon_coles.py:78-248, including
 * compute_corr_coef_bounds (bpl/_util.py:17-31) and dixon_coles_correlation_term
 * (bpl/_util.py:35-93).  Asynchronous, stream ordered.
 *   z          device f64[D]
 *   potential  device f64[1]
 *   grad       device f64[D]
 *   aux        device f64[4] or NULL: {corr_coef (the `deterministic` site of
 *              bpl/dixon_coles.py:80), LB, UB, raw} */
int bplhip_logp_grad(bplhip_ctx* ctx, const double* z, double* potential, double* grad,
                     double* aux, void* stream);

/* The same for `n_chains` independent latent vectors in one launch sequence (numpyro
 * chain_method="vectorized", reachable through mcmc_kwargs at bpl/dixon_coles.py:105).
 *   z [n_chains, D], potential [n_chains], grad [n_chains, D], aux [n_chains, 4] or NULL */
int bplhip_logp_grad_batched(bplhip_ctx* ctx, int32_t n_chains, const double* z,
                             double* potential, double* grad, double* aux, void* stream);

/* Pre-record `count` back-to-back evaluations z[i % n_z] -> (potential[i % n_z],
 * grad[i % n_z]) as one hipGraph and replay it `replays` times on `stream`
 * (asynchronous).  This is how the NUTS driver issues the 2^depth leapfrogs of a tree
 * doubling without a host round trip per launch; it is exposed for the op-level
 * benchmark. */
int bplhip_logp_grad_graph(bplhip_ctx* ctx, int32_t count, int32_t n_z, const double* z,
                           double* potential, double* grad, int32_t replays, void* stream);

/* ---- NUTS driver: numpyro.infer.{NUTS,MCMC} as configured at
 * bpl/dixon_coles.py:100-116 (all NUTS defaults; num_warmup / num_samples forwarded). */
typedef struct bplhip_nuts_cfg {
    int32_t num_warmup;         /* bpl/dixon_coles.py:90 default 500                */
    int32_t num_samples;        /* bpl/dixon_coles.py:91 default 1000               */
    int32_t max_tree_depth;     /* numpyro default 10                               */
    int32_t adapt_step_size;    /* numpyro default 1                                */
    int32_t adapt_mass_matrix;  /* numpyro default 1 (diagonal, regularised)        */
    int32_t thinning;           /* numpyro MCMC default 1                           */
    double step_size;           /* numpyro default 1.0                              */
    double target_accept_prob;  /* numpyro default 0.8                              */
    double init_radius;         /* init_to_uniform(radius=2)                        */
    double max_delta_energy;    /* numpyro default 1000                             */
} bplhip_nuts_cfg;

/* Fill `cfg` with numpyro's defaults as reached from bpl/dixon_coles.py:100-106. */
void bplhip_nuts_default_cfg(bplhip_nuts_cfg* cfg);

typedef struct bplhip_nuts_stats {
    /* per kept draw, HOST arrays of length num_samples/thinning, each may be NULL */
    double* potential_energy;
    double* accept_prob;
    double* step_size;
    int32_t* num_steps;
    int32_t* diverging;
    double* corr_coef;          /* deterministic site `corr_coef` of each draw      */
    /* scalars, filled by the call */
    double final_step_size;
    double mean_accept_prob;
    int64_t total_leapfrogs;    /* potential+gradient evaluations, warm-up included */
    int64_t total_divergences;  /* post warm-up                                     */
    double wall_seconds;
    double* inverse_mass_matrix; /* HOST f64[D] or NULL: adapted diagonal           */
} bplhip_nuts_stats;

/* Run one chain.  `seed_hi:seed_lo` is the 2x32 threefry key (jax.random.PRNGKey(s) ==
 * {0, s} for a 32-bit s; chain c of a multi-chain run uses split(key, num_chains)[c]).
 *   z0         HOST f64[D] or NULL (NULL = init_to_uniform(radius) + retry until finite,
 *              numpyro find_valid_initial_params; non-NULL = run_kwargs init_params,
 *              bpl/dixon_coles.py:115)
 *   draws_out  HOST f64[num_samples/thinning, D] unconstrained draws (post warm-up)
 * Synchronous (returns when the chain has finished). */
int bplhip_nuts_run(bplhip_ctx* ctx, const bplhip_nuts_cfg* cfg, const double* z0,
                    uint32_t seed_hi, uint32_t seed_lo, double* draws_out,
                    bplhip_nuts_stats* stats, void* stream);

/* Run `n_chains` chains together on this GPU (numpyro chain_method="vectorized",
 * MCMC(num_chains=...) at bpl/dixon_coles.py:101-106): persistent chains, every launch
 * advances every unfinished chain by one leapfrog.  Every model; BPLHIP_EUNSUPPORTED only
 * when the run's momentum draws (n_chains * iterations * D doubles) exceed 16 GiB or with
 * "persistent_nuts" 0 outside the basic / extended models with n_teams <= 64 (then run the
 * chains one after another with bplhip_nuts_run).
 *   z0        HOST f64[n_chains, D] or NULL       seeds  HOST u32[n_chains, 2] (hi, lo)
 *   draws_out HOST f64[n_chains, num_samples/thinning, D]
 *   stats     n_chains statistics records, or NULL; wall_seconds is the whole run's.
 * Chain c follows the same key sequence as bplhip_nuts_run with seeds[c]. */
int bplhip_nuts_run_chains(bplhip_ctx* ctx, const bplhip_nuts_cfg* cfg, int32_t n_chains,
                           const double* z0, const uint32_t* seeds, double* draws_out,
                           bplhip_nuts_stats* stats, void* stream);

/* Map unconstrained draws to the constrained / deterministic sites the reference reads
 * from `mcmc.get_samples()` (bpl/dixon_coles.py:118-122,
 * bpl/extended_dixon_coles.py:319-331).  HOST in, HOST out; any output may be NULL.
 *   z_draws f64[s, D]
 *   attack, defence f64[s, T]; home_advantage f64[s] (basic) or f64[s, T] (extended);
 *   corr_coef f64[s]  (needs the rho bounds over all bound fixtures) */
int bplhip_constrain(bplhip_ctx* ctx, const double* z_draws, int64_t s, double* attack,
                     double* defence, double* home_advantage, double* corr_coef);

/* ---- predict path on the device (post-fit).  No fixtures need to be bound.
 * A context holds ONE posterior, in one of two rate forms; per draw, with h / a the home / away team:
 *   plain  (bplhip_predict_set_posterior: the posterior draws the reference keeps as attributes after fit,
 *          bpl/dixon_coles.py:118-122.  HOST pointers: attack/defence f64[s,t], home_advantage f64[s] (basic) or
 *          f64[s,t] (extended, home_advantage_per_team = 1), corr_coef f64[s])
 *     log home rate = attack[h] - defence[a] + home_advantage (h's, when per team)
 *     log away rate = attack[a] - defence[h]
 *   venue  (bplhip_predict_set_posterior_venue: six HOST f64[s,t] tables, confederation_strength HOST
 *          f64[s,n_conf] or NULL with n_conf = 0, corr_coef f64[s]) -- the venue-aware form of the neutral-venue
 *          family: `_calculate_expected_goals` of bpl/neutral_dixon_coles.py:399-423 (four per-team offsets that
 *          are switched off at neutral venues), bpl/neutral_dixon_coles_WC.py:385-424 (plus the difference of the
 *          two sides' confederation strengths) and, for the dynamic class, the rates of its MODEL,
 *          bpl/dynamic_dixon_coles.py:220-231, on the tables of one gameweek:
 *     on = 1 - neutral_venue,  dc = confederation_strength[home_conf] - confederation_strength[away_conf]
 *     log home rate = attack[h] - defence[a] + on (home_attack[h] - away_defence[a]) + dc
 *     log away rate = attack[a] - defence[h] + on (away_attack[a] - home_defence[h]) - dc
 * (A DELIBERATE DEVIATION for the dynamic class: upstream's own predict-time
 * `_calculate_expected_goals`, bpl/dynamic_dixon_coles.py:336-361, differs from the model it was fitted
 * with -- "+ on away_defence[a]" in the home rate, "- on away_attack[a] - on home_defence[h]" in the away
 * rate -- and indexes no gameweek (the class is unfinished upstream).  Predictions
 * here use the rates the likelihood used.) */
int bplhip_predict_set_posterior(bplhip_ctx* ctx, int32_t s, int32_t t, const double* attack,
                                 const double* defence, const double* home_advantage,
                                 int32_t home_advantage_per_team, const double* corr_coef);
int bplhip_predict_set_posterior_venue(bplhip_ctx* ctx, int32_t s, int32_t t, const double* attack,
                                       const double* defence, const double* home_attack,
                                       const double* away_attack, const double* home_defence,
                                       const double* away_defence, int32_t n_conf,
                                       const double* confederation_strength,
                                       const double* corr_coef);

/* The fixtures of a query on that posterior: every query entry point below takes one record, in the form of
 * the posterior.  Every entry checks it in this order before any device call (the score grids, outcome_scores,
 * weighted_scores and market_summary check the ranges of max_goals, n_markets and n_quantiles first, every
 * entry its other arguments afterwards): BPLHIP_ESTATE without a posterior; BPLHIP_ESTATE when `venue` is not
 * the posterior's form (the two forms cannot be mixed, whatever m is); BPLHIP_EINVAL for m outside [0, 2^31), a
 * missing column or an index out of range.  A NULL record is BPLHIP_EINVAL.  The columns are read during the
 * call only. */
typedef struct bplhip_fixtures {
    int64_t m;                               /* fixtures; 0 only where the entry says m >= 0             */
    int32_t venue;                           /* 0: plain form, 1 (nonzero): venue form                   */
    const uint16_t *home_idx, *away_idx;     /* HOST u16[m] team indices < t                             */
    const uint16_t *home_goals, *away_goals; /* HOST u16[m]; not read by entries that take no goals      */
    const uint8_t* neutral_venue;            /* HOST u8[m], nonzero = neutral: the venue form's, required */
    const uint16_t *home_conf, *away_conf;   /* HOST u16[m] < n_conf: the venue form's, exactly when the
                                                posterior has confederations (else NULL)                 */
} bplhip_fixtures;

/* `predict_score_proba` (bpl/dixon_coles.py:139-163, bpl/extended_dixon_coles.py:360-399): out[i] = mean over
 * draws of exp(tau term) * Poisson(x_i; home rate) * Poisson(y_i; away rate).  Fixtures with goals, m >= 0;
 * HOST f64[m] out, synchronous. */
int bplhip_predict_score_proba(bplhip_ctx* ctx, const bplhip_fixtures* q, double* out, void* stream);
/* `predict_score_grid_proba` (bpl/base.py:74-111): for each of the m fixtures the whole
 * (max_goals+1) x (max_goals+1) grid of scoreline probabilities, out[i, x, y] = mean over draws of
 * exp(tau term) * Poisson(x; home rate) * Poisson(y; away rate) -- the primitive the reference's
 * predict_outcome_proba (:113-148), predict_score_n_proba / predict_concede_n_proba (:248-348)
 * and sample_score / sample_outcome (:150-246) are reductions of.  One wave per fixture on the
 * matrix cores (float32 pmf outer products, float64 accumulation across 64-draw blocks).
 * Fixtures without goals, m >= 0; HOST f64[m, max_goals+1, max_goals+1] out, max_goals <= 63, synchronous. */
int bplhip_predict_score_grid(bplhip_ctx* ctx, const bplhip_fixtures* q, int32_t max_goals, double* out,
                              void* stream);
/* ... the same grids as HOST f32[m, max_goals+1, max_goals+1] -- the dtype the reference's
 * predict_score_grid_proba returns (jax float32, bpl/base.py:74-111): the float64 accumulators
 * are rounded once at the store, and half as many bytes come back over PCIe (the copy back is
 * most of a large query: 97 280 grids of 16 x 16 are 199 MB as float64). */
int bplhip_predict_score_grid_f32(bplhip_ctx* ctx, const bplhip_fixtures* q, int32_t max_goals, float* out,
                                  void* stream);

/* ---- the rest of a season, simulated jointly over the posterior (csrc/dc_season.hip.h).
 * Simulation j takes posterior draw j mod s of the posterior set with bplhip_predict_set_posterior
 * (BPLHIP_ESTATE without one, or with a venue-form posterior) and plays every remaining fixture from
 * that one draw: fixture f draws its scoreline exactly from max(tau, 0) Pois(x; lh) Pois(y; la) / Z
 * (the rates and tau of bplhip_predict_score_proba, no max_goals truncation) by two inverse-CDF walks
 * on u = (o + 0.5) 2^-32 from the threefry-2x32-20 block (j, f) under key_hi:key_lo.  The table --
 * init_* plus win / draw / loss points, goals for and against -- is ordered by points, goal
 * difference, goals for (descending), then o0 of block (j, 0x80000000 | slot) descending, then slot;
 * a slot's position is the number of slots ahead of it.
 *   fixtures: home_idx, away_idx HOST u16[n_fixtures] model indices (n_fixtures may be 0), both sides
 *     in the table and distinct;  table: table_idx HOST u16[n_table] distinct model indices
 *     (1 <= n_table <= 64; slot i is table_idx[i]), init_points / init_gf / init_ga HOST i32[n_table]
 *     in [0, BPLHIP_SEASON_MAX_TABLE_VALUE];  points per match in [0, BPLHIP_SEASON_MAX_MATCH_POINTS];
 *     1 <= n_sims < 2^31;  n_fixtures <= BPLHIP_SEASON_MAX_FIXTURES.
 *   required outputs: position_counts HOST u64[n_table, n_table] (slot, position 0 = top), points_sum
 *     and gd_sum HOST i64[n_table] (sums over the simulations);
 *   optional outputs (NULL = not written): sim_points i32[n_sims, n_table], sim_position
 *     u8[n_sims, n_table], home_goals and away_goals u8[n_sims, n_fixtures] (both or neither).
 * Integer accumulation only: the outputs are bit-identical run to run.  Synchronous. */
#define BPLHIP_SEASON_MAX_FIXTURES (1 << 20)
#define BPLHIP_SEASON_MAX_TABLE_VALUE (1 << 24)
#define BPLHIP_SEASON_MAX_MATCH_POINTS 1000
int bplhip_simulate_season(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                           const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                           const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                           int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                           uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts, int64_t* points_sum,
                           int64_t* gd_sum, int32_t* sim_points, uint8_t* sim_position, uint8_t* home_goals,
                           uint8_t* away_goals, void* stream);

/* ---- which remaining fixtures decide the table (csrc/dc_leverage.hip.h): bplhip_simulate_season's simulations,
 * cross-tabulated on the device.  The input arguments up to key_lo are bplhip_simulate_season's, in its order
 * and under its rules (BPLHIP_ESTATE without a posterior, or with a venue-form posterior; BPLHIP_EINVAL
 * for bad arguments), except n_fixtures <= BPLHIP_LEVERAGE_MAX_FIXTURES; simulation j is simulation j of
 * bplhip_simulate_season under the same key: the same draw, threefry blocks, tie-break and ranking.
 *   targets: 1 <= n_targets <= BPLHIP_LEVERAGE_MAX_TARGETS sets of finishing positions, target_mask HOST
 *     u64[n_targets], bit p = position p (0 = top); every mask non-zero and inside the table (bits < n_table);
 *   chunk_sims: the simulations pass through a device workspace of this many records at a time
 *     (16 B per 64 fixtures + n_table bytes each); 0 = the library's choice (at most 65536, within 64 MiB),
 *     negative is BPLHIP_EINVAL.  The results do not depend on it;
 *   required outputs, o = 0 home win, 1 draw, 2 away win: outcome_counts HOST u64[n_fixtures, 3] (the
 *     simulations in which fixture f ended o), target_counts HOST u64[n_table, n_targets] (slot t finished
 *     inside target k), joint_counts HOST u64[n_fixtures, 3, n_table, n_targets] (both at once).
 * Per-simulation scorelines and positions never leave the device.  Integer accumulation only: the outputs
 * are bit-identical run to run and for every chunk_sims.  Synchronous. */
#define BPLHIP_LEVERAGE_MAX_FIXTURES 4096
#define BPLHIP_LEVERAGE_MAX_TARGETS 8
int bplhip_match_leverage(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                          const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                          const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                          int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                          uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                          int64_t chunk_sims, uint64_t* outcome_counts, uint64_t* target_counts,
                          uint64_t* joint_counts, void* stream);

/* ---- a group-and-knockout tournament, simulated jointly over the posterior (csrc/dc_tournament.hip.h).
 * Needs the posterior set with bplhip_predict_set_posterior_venue (BPLHIP_ESTATE without one, or with
 * a plain posterior).  Simulation j takes posterior draw j mod s for every match it plays.  A match
 * between slots p and q (listed order) with exactly one host is played at the host's venue (the host
 * is the home side, on = 1); every other match keeps the listed order and is neutral (on = 0); the
 * rates are the venue form's, with the slots' confederations.  Scorelines are
 * bplhip_simulate_season's exact draw on the threefry-2x32-20 blocks (j, f) for group fixture f,
 * (j, 0x40000000 | k << 5 | t) for knockout match k (numbered over all rounds in order) attempt t < 32.
 * Groups are ranked like bplhip_simulate_season's table within each group (tie-break word: o0 of
 * block (j, 0x80000000 | slot)); the top `advance` of each group qualify, and the slots placed
 * advance + 1 are ranked across the groups by the same keys, the best `best_of_rest` qualifying too.
 * First-round entry 2m meets entry 2m + 1, the winner becomes entry m of the next round; a level
 * scoreline is redrawn from the next attempt's block, and after 32 level attempts the first-listed
 * side goes through.
 *   teams: n_teams in [2, 64]; team_idx HOST u16[n_teams] distinct model indices; team_conf HOST
 *     u16[n_teams] exactly when the posterior has confederations (else NULL); team_host HOST
 *     u8[n_teams] 0 / 1 or NULL (no hosts).
 *   groups: n_groups in [0, BPLHIP_TOURNAMENT_MAX_GROUPS]; with n_groups > 0, team_group HOST
 *     u8[n_teams] (each group 2..8 slots), init_points / init_gf / init_ga HOST i32[n_teams] in
 *     [0, BPLHIP_SEASON_MAX_TABLE_VALUE], fixtures fix_p / fix_q HOST u8[n_fixtures] two slots of one
 *     group (n_fixtures <= BPLHIP_SEASON_MAX_FIXTURES), 1 <= advance <= 8, best_of_rest at most the
 *     number of groups larger than advance, points per match in [0, BPLHIP_SEASON_MAX_MATCH_POINTS].
 *     With n_groups = 0 (knockout only) n_fixtures = 0, and the group arguments are not read.
 *   bracket: HOST u16[n_bracket], n_bracket = 2^R, 1 <= R <= 6.  With groups, entry group << 8 | place
 *     (place 1-based, at most min(advance, group size)) or 0xFF00 | k (the k-th best of the rest, 1-based),
 *     every qualifier exactly once; without groups, a slot, every slot exactly once.
 *   outputs: stage_counts HOST u64[n_teams, R + 2] (stage 0 = out in the groups, r + 1 = reached
 *     knockout column r, column R = won the final); group_position_counts HOST u64[n_teams, 8]
 *     (position 0 = top of the group; required with groups, else not written); sim_stage u8[n_sims,
 *     n_teams] or NULL.  1 <= n_sims < 2^31.
 * Integer accumulation only: the outputs are bit-identical run to run.  Synchronous. */
#define BPLHIP_TOURNAMENT_MAX_GROUPS 16
int bplhip_simulate_tournament(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx,
                               const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                               const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                               const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                               const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                               const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                               int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                               uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage,
                               void* stream);

/* ---- head-to-head tie-breaks (csrc/dc_h2h.hip.h): the three calls above with the table ordered by points, then
 * among the slots level on points (in a tournament: level on points within one group) by the points taken
 * from each other, the goal difference and the goals scored in the matches between them, and only then by
 * overall goal difference, goals for, the tie-break word and the slot.  The mini-table is formed once over all
 * slots level on points (no re-application to a still-tied subset).  The tournament's best of the rest keep
 * bplhip_simulate_tournament's keys: slots of different groups have no match between them.
 * Each call takes the argument list of its counterpart, under its rules and with its outputs, plus
 *   pair_init: HOST u32[n, n] (n = n_table / n_teams), row i column k = the points slot i took from slot k << 16 |
 *     the goals i scored against k in the matches already played; NULL = all zero; the diagonal is ignored.
 *     BPLHIP_EINVAL when, for an ordered pair, points + m max(win, draw, loss points) or goals + 255 m can pass
 *     65535, m = the pair's remaining meetings among the fixtures.
 * Under one key simulation j is simulation j of the counterpart up to the ranking: the same draw, threefry
 * blocks, scorelines, points and tie-break word.  Integer accumulation only; synchronous. */
int bplhip_simulate_season_h2h(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                               const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                               const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                               int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                               uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts, int64_t* points_sum,
                               int64_t* gd_sum, int32_t* sim_points, uint8_t* sim_position, uint8_t* home_goals,
                               uint8_t* away_goals, void* stream, const uint32_t* pair_init);
int bplhip_match_leverage_h2h(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                              const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                              const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                              int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                              uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                              int64_t chunk_sims, uint64_t* outcome_counts, uint64_t* target_counts,
                              uint64_t* joint_counts, void* stream, const uint32_t* pair_init);
int bplhip_simulate_tournament_h2h(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx,
                                   const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                   const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                   const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                   const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                   const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                   int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                   uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage,
                                   void* stream, const uint32_t* pair_init);

/* ---- extra time, shoot-outs and two-legged ties (csrc/dc_knockout.hip.h): bplhip_simulate_tournament_h2h's
 * argument list, under its rules and with its outputs (pair_init is read only when head_to_head != 0; with 0 the
 * groups are ordered as by bplhip_simulate_tournament), but a knockout match is no longer redrawn while level.
 * Match k (numbered over all rounds) between entries p (2m) and q (2m + 1) reads at most four blocks
 * (j, 0x40000000 | k << 5 | t):
 *   t = 0  the only leg, at the venue and in the orientation the host flags give; or leg 1 of a two-legged round
 *          (bit r of legs_mask set for round r, first round = bit 0): p at home, on = 1, host flags not read;
 *   t = 1  leg 2: q at home, on = 1.  The higher aggregate (x1 + y2 for p, y1 + x2 for q) goes through; level,
 *          and with away_goals = 1, the higher away goals (y2 for p, y1 for q);
 *   t = 2  extra time when still level: the venue and orientation of the only leg or of leg 2, both rates times
 *          extra_time_scale in (0, 1], the same rho and sampler; the goals are added and the higher total goes
 *          through (away goals are not applied again);
 *   t = 3  the shoot-out when still level: p goes through iff (o0 + 0.5) 2^-32 < 1 / (1 + exp(-(strength[p] -
 *          strength[q]))); strength HOST f64[n_teams], finite, |strength| <= BPLHIP_TOURNAMENT_MAX_STRENGTH, or
 *          NULL (all zero: exactly one half).
 * Under one key, a single-leg match that is not level after block 0 has bplhip_simulate_tournament's winner.
 *   outputs: decided_counts HOST u64[R, 4] (required): round r's matches decided in normal time / by away goals /
 *     in extra time / by the shoot-out; sim_decided u8[n_sims, 2^R - 1] or NULL: the same 0..3 per match.
 * BPLHIP_EINVAL also for a legs_mask bit at or above R, a scale outside (0, 1], away_goals not 0 / 1 and a
 * non-finite or too large strength; BPLHIP_ESTATE as the counterpart.  Integer accumulation only; synchronous. */
#define BPLHIP_TOURNAMENT_MAX_STRENGTH 20
int bplhip_simulate_tournament_knockout(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx,
                                        const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                        const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                        const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                        const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                        const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                        int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                        uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage,
                                        void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                        uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                        const double* strength, uint64_t* decided_counts, uint8_t* sim_decided);

/* ---- who meets whom (csrc/dc_paths.hip.h): bplhip_simulate_tournament_knockout's argument list with one flag more,
 * extra_time (0: a level knockout match is redrawn as by bplhip_simulate_tournament and the five rule arguments
 * after it are not read; 1: the extra-time rule), under the same checks, which speak in simulate_tournament's name.
 * Under one key simulation j is simulation j of the counterpart: the same draw, blocks, ranking, bracket and winners
 * in all four modes, so stage_counts, group_position_counts, decided_counts, sim_stage and sim_decided are the
 * counterpart's.  The simulations pass through a device workspace of chunk_sims records (0: the library's choice,
 * >= 0; no result depends on it) and are cross-tabulated there; with K = R + 1 targets, target k < R = "plays
 * knockout column k", k = R = "wins the tournament":
 *   advance_counts HOST u64[R, n, n] (required): [r, t, u] = t went through against u in knockout round r (a
 *     two-legged tie is one meeting); the meetings are advance + its transpose;
 *   position_stage_counts HOST u64[n, 8, 8] (required with groups, else not written): group position x stage;
 *   outcome_counts HOST u64[n_fixtures, 3], target_counts HOST u64[n, K], joint_counts HOST u64[n_fixtures, 3, n, K]
 *     (required when n_fixtures > 0, else not written): bplhip_match_leverage's tables for the group fixtures, the
 *     outcome in the LISTED order of the fixture (0 = fix_p's side wins, 1 = draw, 2 = fix_q's side wins), whichever
 *     side the host flags put at home; n_fixtures <= BPLHIP_LEVERAGE_MAX_FIXTURES;
 *   optional per-simulation records, NULL or: sim_position u8[n_sims, n] (group position, 0 without groups),
 *     sim_outcome u8[n_sims, n_fixtures] (0 / 1 / 2 as above), sim_pair u8[n_sims, 2^R - 1, 2] (the two slots of
 *     every knockout match in listed order, matches numbered over the rounds as sim_decided numbers them),
 *     sim_winner u8[n_sims, 2^R - 1].
 * BPLHIP_EINVAL and BPLHIP_ESTATE as the counterparts, and BPLHIP_EINVAL for a negative chunk_sims, too many
 * fixtures and a null required output.  Integer accumulation only: bit-identical run to run and for any chunk_sims.
 * Synchronous. */
int bplhip_tournament_paths(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
                            const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group,
                            const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                            int64_t n_fixtures, const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                            int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket, int32_t win_points,
                            int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                            uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage, void* stream,
                            const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time, uint32_t legs_mask,
                            double extra_time_scale, int32_t away_goals, const double* strength,
                            uint64_t* decided_counts, uint8_t* sim_decided, int64_t chunk_sims,
                            uint64_t* advance_counts, uint64_t* position_stage_counts, uint64_t* outcome_counts,
                            uint64_t* target_counts, uint64_t* joint_counts, uint8_t* sim_position,
                            uint8_t* sim_outcome, uint8_t* sim_pair, uint8_t* sim_winner);

/* ---- play-offs after the league table (csrc/dc_playoff.hip.h): bplhip_simulate_season_h2h's argument list, under
 * its rules and with its outputs (pair_init is read only when head_to_head != 0; with 0 the table is ordered as by
 * bplhip_simulate_season), and under one key the same league simulation for simulation: the blocks (j, f), the
 * tie-break words, the ranking and every output.  After the ranking simulation j plays one knockout bracket from the
 * same posterior draw j mod s.  Slots 0..n_table-1 are the table's rows, slots n_table + i the guests:
 *   guest_idx: HOST u16[n_guests] distinct model indices outside the table (NULL with n_guests = 0);
 *     n_table + n_guests <= 64;
 *   bracket: HOST u16[2^rounds] first-round codes, 1 <= rounds <= 6: a finishing position (0 = top, < n_table),
 *     BPLHIP_PLAYOFF_GUEST | i (guest i < n_guests) or BPLHIP_PLAYOFF_BYE; every position and guest at most once;
 *     entry 2m meets entry 2m + 1 (a bye sends the other entry through without a match; two byes may not be
 *     paired), the winners of matches 2m and 2m + 1 meet next.
 * A table row's seed is its finishing position, guest i's seed is n_table + i, a winner carries its seed on.  In every
 * tie q is the better-seeded and p the worse-seeded side, and match k (numbered over all 2^rounds - 1 bracket
 * matches, byes included) reads at most four blocks (j, 0x40000000 | k << 5 | t):
 *   t = 0  the only leg: q at home with the home advantage, or -- bit r of neutral_mask set for round r -- p listed
 *          as the home side and the home-advantage term left out of the rates; or leg 1 of a two-legged round (bit r
 *          of legs_mask; the neutral bit is then not read): at p's ground, with the home advantage;
 *   t = 1  leg 2 at q's ground.  Aggregates and away_goals as in bplhip_simulate_tournament_knockout;
 *   t = 2  extra time at the venue of the only leg or of leg 2, both rates times extra_time_scale in (0, 1];
 *   t = 3  the shoot-out: p goes through iff (o0 + 0.5) 2^-32 < 1 / (1 + exp(-(strength[p] - strength[q])));
 *          strength HOST f64[n_table + n_guests] per slot, finite, at most BPLHIP_TOURNAMENT_MAX_STRENGTH in size, or
 *          NULL (all zero).
 *   required outputs: stage_counts HOST u64[n_table + n_guests, rounds + 2] (stage 0 = not in the bracket, r + 1 =
 *     the furthest round entered was r, by a match or a bye, rounds + 1 = won the bracket); decided_counts HOST
 *     u64[rounds, 4] (the matches played in round r decided in normal time / by away goals / in extra time / by the
 *     shoot-out; byes are not counted);
 *   optional outputs: sim_stage u8[n_sims, n_table + n_guests]; sim_decided u8[n_sims, 2^rounds - 1], 0..3 per
 *     match and 255 for a bye.
 * BPLHIP_EINVAL also for rounds outside 1..6, a code out of range or used twice, two byes paired, a guest out of
 * range, repeated or in the table, mask bits at or above rounds, a scale outside (0, 1], head_to_head or away_goals
 * not 0 / 1, a non-finite or too large strength, n_table + n_guests > 64 and a null required output; BPLHIP_ESTATE
 * as the counterpart.  Integer accumulation only: bit-identical run to run.  Synchronous. */
#define BPLHIP_PLAYOFF_GUEST 0x8000
#define BPLHIP_PLAYOFF_BYE 0xFFFF
int bplhip_simulate_season_playoff(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                                   const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                   const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                   int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                   uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts, int64_t* points_sum,
                                   int64_t* gd_sum, int32_t* sim_points, uint8_t* sim_position, uint8_t* home_goals,
                                   uint8_t* away_goals, void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                   int32_t n_guests, const uint16_t* guest_idx, const uint16_t* bracket,
                                   int32_t rounds, uint32_t legs_mask, uint32_t neutral_mask,
                                   double extra_time_scale, int32_t away_goals_rule, const double* strength,
                                   uint64_t* stage_counts, uint64_t* decided_counts, uint8_t* sim_stage,
                                   uint8_t* sim_decided);

/* ---- the rest of a season with matches IN PROGRESS and weighted posterior draws (csrc/dc_live.hip.h):
 * bplhip_simulate_season_h2h's argument list (pair_init is read only when head_to_head != 0; with 0 the table is
 * ordered as by bplhip_simulate_season), under its rules and with its outputs, over the CONCATENATED list of the
 * n_fixtures fixtures still to kick off and then the n_in_play matches in progress: match m is fixture n_fixtures + m
 * (its threefry block is (j, n_fixtures + m), it is booked into the table and the pair matrix like any fixture and
 * counts as a meeting to come in pair_init's 16-bit bound), and home_goals / away_goals are u8[n_sims, n_fixtures +
 * n_in_play] FINAL scores.  The table (init_*) and pair_init do NOT contain the matches in progress.
 *   in_play_home_idx, in_play_away_idx   HOST u16[n_in_play] model indices, both in the table and distinct
 *   in_play_home_goals, in_play_away_goals   HOST u8[n_in_play] the current score, each at most BPLHIP_LIVE_MAX_GOALS
 *   in_play_elapsed   HOST f64[n_in_play], each in [0, 1) (not NaN); 0 only with the score 0-0
 *   reweight     nonzero: the joint likelihood of all states enters the draw weights (read only when n_in_play > 0)
 *   log_weights  NULL, or HOST f64[s], all finite
 * With l[s, m] = log Pois(a; lh t) + log Pois(b; la t) + log Z of bplhip_inplay_summary (the base form's full-match
 * rates), in float64:  L0[s] = sum_m l[s, m] in m order;  L[s] = (L0[s] if reweight) + (log_weights[s] if given);
 * w[s] = exp(L[s] - max L);  C the inclusive scan of w in draw order (fixed association: 256 contiguous segments summed
 * sequentially, their totals left to right, C[s] = segment start + own partial sum);  W = C[s-1].
 * Weights are IN FORCE when log_weights is given or (reweight and n_in_play > 0).  Then simulation j takes the draw
 *     s_j = #{s : C[s] < min((j + U) W / n_sims, W)},   U = (o0 + 0.5) 2^-32 of the threefry block (0, 0x20000000)
 * (systematic resampling: draw s is used floor or ceil of n_sims w[s] / W times, a draw with w = 0 never); otherwise
 * j mod s as bplhip_simulate_season, and no weight is computed.  A match in progress at a : b with r = 1 - t to play
 * draws its FINAL score from tau(x, y) Pois(x - a; lh r) Pois(y - b; la r) / Z on x >= a, y >= b (tau on the final
 * score with the full-match rates) by bplhip_simulate_season's two walks started at the current score (each side
 * capped at 255); at 0-0, t = 0 the scoreline is bit for bit the one bplhip_simulate_season draws from that block.
 *   ess          HOST f64[1]: (sum w)^2 / sum w^2; s without weights in force
 *   log_evidence HOST f64[1]: max L0 + log mean_s exp(L0 - max L0); 0 with n_in_play = 0; NaN when n_in_play > 0
 *                and no weights are in force (the states' likelihood is then not evaluated)
 *   sim_draw     NULL, or i32[n_sims]: s_j
 *   draw_log_weights, draw_log_evidence   NULL, or HOST f64[s]: L and L0 (zeros / as log_evidence without weights)
 * BPLHIP_EINVAL, before any device call, for everything bplhip_simulate_season_h2h refuses and for an elapsed outside
 * [0, 1) or NaN, elapsed = 0 with a score other than 0-0, a current goal count above BPLHIP_LIVE_MAX_GOALS, an
 * in-play team outside the table or playing itself, n_fixtures + n_in_play > BPLHIP_SEASON_MAX_FIXTURES, a non-finite
 * log weight.  Integer accumulation only and a fixed-order scan: bit-identical run to run.  Synchronous. */
#define BPLHIP_LIVE_MAX_GOALS 63
int bplhip_simulate_season_live(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                                const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                uint32_t key_hi, uint32_t key_lo, uint64_t* position_counts, int64_t* points_sum,
                                int64_t* gd_sum, int32_t* sim_points, uint8_t* sim_position, uint8_t* home_goals,
                                uint8_t* away_goals, void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                int32_t n_in_play, const uint16_t* in_play_home_idx, const uint16_t* in_play_away_idx,
                                const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                const double* in_play_elapsed, int32_t reweight, const double* log_weights,
                                double* ess, double* log_evidence, int32_t* sim_draw, double* draw_log_weights,
                                double* draw_log_evidence);

/* ---- points totals against finishing targets (csrc/dc_points.hip.h): bplhip_simulate_season's simulations, the
 * points a slot ends on cross-tabulated on the device against its finishing-position targets, the points of every
 * finishing position and the gap between neighbouring positions.  The arguments up to chunk_sims are
 * bplhip_match_leverage's, in its order and under its rules and error codes (BPLHIP_ESTATE without a posterior, or
 * with a venue-form posterior; n_fixtures <= BPLHIP_LEVERAGE_MAX_FIXTURES; 1 <= n_targets <=
 * BPLHIP_LEVERAGE_MAX_TARGETS); simulation j is simulation j of bplhip_simulate_season under the same key.
 *   chunk_sims: the simulations pass through a device workspace of this many records at a time (5 n_table bytes
 *     each); 0 = the library's choice (at most 65536, within 64 MiB), negative is BPLHIP_EINVAL.  The results do
 *     not depend on it;
 *   the points axis: bin b = points_min + b points, 1 <= n_bins <= BPLHIP_POINTS_MAX_BINS.  BPLHIP_EINVAL when a
 *     simulated total could fall outside [points_min, points_min + n_bins): slot t with m remaining matches ends on
 *     init_points[t] + m min(win, draw, loss points) .. init_points[t] + m max(win, draw, loss points);
 *   required outputs: team_points HOST u64[n_table, n_bins] (slot t ended on bin b), team_target HOST
 *     u64[n_table, n_bins, n_targets] (and inside target k), position_points HOST u64[n_table, n_bins] (the slot
 *     finishing in position p, 0 = top, had bin b), gap HOST u64[n_table - 1, n_bins] (the points of position p minus
 *     those of position p + 1, bin 0 = level on points; may be NULL only when n_table = 1);
 *   pair_init: NULL = the overall order of bplhip_simulate_season; non-NULL = the head-to-head order, read as
 *     bplhip_match_leverage_h2h reads it (HOST u32[n_table, n_table]; all zero for no matches played).
 * Per-simulation points and positions never leave the device.  Integer accumulation only: the outputs are
 * bit-identical run to run and for every chunk_sims.  Synchronous. */
#define BPLHIP_POINTS_MAX_BINS 1024
int bplhip_season_points(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx, const uint16_t* away_idx,
                         int32_t n_table, const uint16_t* table_idx, const int32_t* init_points,
                         const int32_t* init_gf, const int32_t* init_ga, int32_t win_points, int32_t draw_points,
                         int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo, int32_t n_targets,
                         const uint64_t* target_mask, int64_t chunk_sims, int32_t points_min, int32_t n_bins,
                         uint64_t* team_points, uint64_t* team_target, uint64_t* position_points, uint64_t* gap,
                         void* stream, const uint32_t* pair_init);

/* ---- the joint result of chosen fixtures against finishing targets (csrc/dc_scenario.hip.h):
 * bplhip_simulate_season's simulations, every combination of the key fixtures' clipped margins cross-tabulated on
 * the device against the slots' finishing-position targets.  The arguments up to chunk_sims are
 * bplhip_season_points', in its order and under its rules and error codes (BPLHIP_ESTATE without a posterior, or with
 * a venue-form posterior; n_fixtures <= BPLHIP_LEVERAGE_MAX_FIXTURES; 1 <= n_targets <= BPLHIP_LEVERAGE_MAX_TARGETS;
 * chunk_sims as there, a record being 4 + n_table bytes); simulation j is simulation j of bplhip_simulate_season
 * under the same key.
 *   the keys: 1 <= n_key <= BPLHIP_SCENARIO_MAX_KEYS; key_fixture HOST i32[n_key], distinct positions in
 *     0..n_fixtures-1; key_cap HOST i32[n_key], each in 1..BPLHIP_SCENARIO_MAX_CAP.  Key q with cap c has C_q = 2 c + 1
 *     classes, class = c - clip(home goals - away goals, -c, c): 0 = home by c or more, 2 c = away by c or more.  A
 *     scenario is one class per key, m = sum_q class_q prod_{r > q} C_r (row-major in the order given), and
 *     M = prod_q C_q <= BPLHIP_SCENARIO_MAX_CELLS.  BPLHIP_EINVAL otherwise, checked in this order: n_key and the
 *     pointers, the positions, the caps, M;
 *   required outputs: scenario HOST u64[M] (the simulations of scenario m), joint HOST u64[M, n_table, n_targets]
 *     (of those, slot t finished inside target k);
 *   pair_init: as for bplhip_season_points.
 * Per-simulation scorelines and positions never leave the device.  Integer accumulation only: the outputs are
 * bit-identical run to run and for every chunk_sims.  Synchronous. */
#define BPLHIP_SCENARIO_MAX_KEYS 8
#define BPLHIP_SCENARIO_MAX_CAP 3
#define BPLHIP_SCENARIO_MAX_CELLS 6561
int bplhip_season_scenarios(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx, const uint16_t* away_idx,
                            int32_t n_table, const uint16_t* table_idx, const int32_t* init_points,
                            const int32_t* init_gf, const int32_t* init_ga, int32_t win_points, int32_t draw_points,
                            int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo, int32_t n_targets,
                            const uint64_t* target_mask, int64_t chunk_sims, int32_t n_key, const int32_t* key_fixture,
                            const int32_t* key_cap, uint64_t* scenario, uint64_t* joint, void* stream,
                            const uint32_t* pair_init);

/* ---- the three queries on a day with matches IN PROGRESS and with weighted posterior draws
 * (csrc/dc_live_queries.hip.h): bplhip_match_leverage_h2h's, bplhip_season_points' and bplhip_season_scenarios'
 * argument lists, each followed by bplhip_simulate_season_live's request (n_in_play .. log_weights) and its outputs ess
 * and log_evidence, with that symbol's meaning throughout:
 *   the fixture list is the CONCATENATED one, the n_fixtures fixtures still to kick off and then the n_in_play matches
 *     in progress; match m is fixture n_fixtures + m: its threefry block is (j, n_fixtures + m), it is booked into the
 *     table and the pair matrix like any fixture, it counts as a meeting to come in pair_init's 16-bit bound and as a
 *     remaining match on bplhip_season_points' axis, and n_fixtures + n_in_play <= BPLHIP_LEVERAGE_MAX_FIXTURES.  The
 *     table (init_*) and pair_init do NOT contain the matches in progress;
 *   under one key simulation j is simulation j of bplhip_simulate_season_live with the same request: the same draw
 *     (systematic resampling over all n_sims simulations with one offset per call when weights are in force, j mod s
 *     otherwise -- whatever chunk_sims is), the same scorelines, FINAL scores of the matches in progress included, the
 *     same tie-break and ranking;
 *   ess and log_evidence are that symbol's, bit for bit (the same two kernels on the same inputs);
 *   pair_init: NULL = the overall order; non-NULL = the head-to-head order (all zero for no matches played), for all
 *     three symbols, as bplhip_season_points reads it.
 * bplhip_match_leverage_live: outcome_counts is u64[n_fixtures + n_in_play, 3] and joint_counts u64[n_fixtures +
 *   n_in_play, 3, n_table, n_targets], the matches in progress last, each classified by its FINAL score.
 * bplhip_season_points_live: the outputs of bplhip_season_points.
 * bplhip_season_scenarios_live: key_fixture holds distinct positions in 0..n_fixtures + n_in_play - 1 of the
 *   concatenated list; a key in progress is classed by its final clipped margin, so a class the current score has ruled
 *   out has count 0.
 * BPLHIP_EINVAL, before any device call, for everything the kick-off symbol refuses and everything
 * bplhip_simulate_season_live refuses of its request, checked in that symbol's order: the lengths of the two lists,
 * null in-play columns, null ess / log_evidence, the states; then the kick-off symbol's own checks over the
 * concatenated list; last a non-finite log weight.  Integer accumulation only and a fixed-order scan: bit-identical run
 * to run and for every chunk_sims.  Synchronous. */
int bplhip_match_leverage_live(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                               const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                               const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                               int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                               uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                               int64_t chunk_sims, uint64_t* outcome_counts, uint64_t* target_counts,
                               uint64_t* joint_counts, void* stream, const uint32_t* pair_init, int32_t n_in_play,
                               const uint16_t* in_play_home_idx, const uint16_t* in_play_away_idx,
                               const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                               const double* in_play_elapsed, int32_t reweight, const double* log_weights, double* ess,
                               double* log_evidence);
int bplhip_season_points_live(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                              const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                              const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                              int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                              uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                              int64_t chunk_sims, int32_t points_min, int32_t n_bins, uint64_t* team_points,
                              uint64_t* team_target, uint64_t* position_points, uint64_t* gap, void* stream,
                              const uint32_t* pair_init, int32_t n_in_play, const uint16_t* in_play_home_idx,
                              const uint16_t* in_play_away_idx, const uint8_t* in_play_home_goals,
                              const uint8_t* in_play_away_goals, const double* in_play_elapsed, int32_t reweight,
                              const double* log_weights, double* ess, double* log_evidence);
int bplhip_season_scenarios_live(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx,
                                 const uint16_t* away_idx, int32_t n_table, const uint16_t* table_idx,
                                 const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                 int32_t win_points, int32_t draw_points, int32_t loss_points, int64_t n_sims,
                                 uint32_t key_hi, uint32_t key_lo, int32_t n_targets, const uint64_t* target_mask,
                                 int64_t chunk_sims, int32_t n_key, const int32_t* key_fixture, const int32_t* key_cap,
                                 uint64_t* scenario, uint64_t* joint, void* stream, const uint32_t* pair_init,
                                 int32_t n_in_play, const uint16_t* in_play_home_idx, const uint16_t* in_play_away_idx,
                                 const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                 const double* in_play_elapsed, int32_t reweight, const double* log_weights,
                                 double* ess, double* log_evidence);

/* ---- the joint result of chosen group fixtures against knockout targets (csrc/dc_tscen.hip.h):
 * bplhip_tournament_paths' simulations, every combination of the key group fixtures' clipped margins cross-tabulated
 * on the device against K = R + 2 targets per slot: target k < R = "plays knockout column k", k = R = "wins the
 * tournament", k = R + 1 = "finishes first in its group".  The inputs through key_lo are bplhip_simulate_tournament's,
 * in its order; stream .. decided_counts are bplhip_tournament_paths' (extra_time 0: the five rule arguments after
 * it are not read), under the same checks, which speak in simulate_tournament's name; under one key simulation j is
 * simulation j of both, in all four modes, and decided_counts is theirs.
 *   chunk_sims: the simulations pass through a device workspace of this many records at a time (4 + n bytes each);
 *     0 = the library's choice, negative is BPLHIP_EINVAL.  The results do not depend on it;
 *   BPLHIP_EINVAL with n_groups = 0 or n_fixtures = 0: there is nothing to key on;
 *   the keys: n_key, key_fixture (positions in the group-fixture list), key_cap and the scenario index as for
 *     bplhip_season_scenarios, checked in its order, with class = c - clip(fix_p's goals - fix_q's goals, -c, c): the
 *     LISTED order of the fixture, whichever side the host flags put at home;
 *   required outputs: scenario HOST u64[M], joint HOST u64[M, n, K];
 *   optional per-simulation records, NULL or: sim_scenario u32[n_sims] (the scenario index), sim_tset u8[n_sims, n]
 *     (bit k: the slot is inside target k).
 * BPLHIP_ESTATE without a venue-form posterior.  Integer accumulation only: the outputs are bit-identical run to run
 * and for every chunk_sims.  Synchronous. */
int bplhip_tournament_scenarios(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
                                const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group,
                                const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                int64_t n_fixtures, const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket, int32_t win_points,
                                int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
                                uint32_t key_lo, void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                int32_t extra_time, uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                const double* strength, uint64_t* decided_counts, int64_t chunk_sims, int32_t n_key,
                                const int32_t* key_fixture, const int32_t* key_cap, uint64_t* scenario,
                                uint64_t* joint, uint32_t* sim_scenario, uint8_t* sim_tset);

/* ---- group points against qualification targets (csrc/dc_group_points.hip.h): bplhip_tournament_scenarios'
 * simulations, every slot's group-stage points cross-tabulated on the device against its K = R + 2 targets (those of
 * bplhip_tournament_scenarios) and its group place, the points of every group place, the gap between neighbouring
 * places, and the points and clipped goal difference of the slots placed advance + 1 ("the rest") against their rank
 * across the groups.  The inputs through chunk_sims are bplhip_tournament_scenarios', in its order and under the
 * same checks, which speak in simulate_tournament's name; under one key simulation j is simulation j of
 * bplhip_simulate_tournament, bplhip_tournament_paths and bplhip_tournament_scenarios, in all four modes, and
 * decided_counts is theirs.
 *   chunk_sims: the simulations pass through a device workspace of this many records at a time (4 n + n_groups Z +
 *     2 B bytes each, Z the largest group, B the groups with a place advance + 1); 0 = the library's choice, negative
 *     is BPLHIP_EINVAL.  The results do not depend on it;
 *   BPLHIP_EINVAL with n_groups = 0: there are no group points.  n_fixtures = 0 is allowed: the group stage is then the
 *     current table's, in every simulation;
 *   the points axis: bin b = points_min + b points, 1 <= n_bins <= BPLHIP_GROUP_POINTS_MAX_BINS.  BPLHIP_EINVAL when a
 *     simulated total could leave it, by bplhip_season_points' rule: unless init_points[t] + m min(win, draw, loss
 *     points) >= points_min and init_points[t] + m max(...) < points_min + n_bins for slot t with m group fixtures;
 *   the goal-difference axis: 0 <= gd_cap <= BPLHIP_GROUP_POINTS_MAX_GD_CAP, D = 2 gd_cap + 1 bins, bin d =
 *     clip(goals for - goals against, -gd_cap, gd_cap) + gd_cap over the current table plus the simulated matches;
 *   required outputs, HOST u64: team_points [n, n_bins] (slot t ended the groups on bin b), team_target [n, n_bins, K]
 *     (and inside target k), team_place [n, n_bins, Z] (and on place z of its group, 0 = top), place_points
 *     [n_groups, Z, n_bins] (the slot on place z of group g had bin b; zero for a place the group lacks), place_gap
 *     [n_groups, Z - 1, n_bins] (the points of place z minus those of place z + 1; bin 0 = level on points);
 *   the rest outputs, HOST u64, required with best_of_rest > 0 and not written (they may be NULL) with best_of_rest
 *     = 0: rest_count [n_bins, D] (the slots placed advance + 1, pooled over groups and simulations), rest_through
 *     [n_bins, D] (those of them among the best best_of_rest), rest_rank [B, n_bins, D] (the k-th best of the rest,
 *     ranked as the bracket ranks them).
 * Per-simulation tables never leave the device.  BPLHIP_ESTATE without a venue-form posterior.  Integer accumulation
 * only: the outputs are bit-identical run to run and for every chunk_sims.  Synchronous. */
#define BPLHIP_GROUP_POINTS_MAX_BINS 256
#define BPLHIP_GROUP_POINTS_MAX_GD_CAP 8
int bplhip_tournament_points(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
                             const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group,
                             const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                             int64_t n_fixtures, const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                             int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket, int32_t win_points,
                             int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
                             uint32_t key_lo, void* stream, const uint32_t* pair_init, int32_t head_to_head,
                             int32_t extra_time, uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                             const double* strength, uint64_t* decided_counts, int64_t chunk_sims, int32_t points_min,
                             int32_t n_bins, int32_t gd_cap, uint64_t* team_points, uint64_t* team_target,
                             uint64_t* team_place, uint64_t* place_points, uint64_t* place_gap, uint64_t* rest_count,
                             uint64_t* rest_through, uint64_t* rest_rank);

/* ---- best-of-rest allocation tables: where in the bracket a qualifier placed advance + 1 goes by WHICH groups
 * those qualifiers come from (the Euros since 2016, the World Cup from 2026), not by its rank among them.  Kept on
 * the context, as the posterior is: while a table is set, every entry of the tournament family (the three
 * simulate_tournament forms, tournament_paths, tournament_scenarios, tournament_points) reads the bracket code
 * 0xFF00 | k as "allocation slot k" instead of "the k-th best of the rest".  Which slots qualify does not change,
 * nor any random number: a simulation differs only in the bracket positions of those qualifiers and in what follows.
 *   n_groups, best: the n_groups and best_of_rest of the calls to come, 1 <= best <= n_groups; a call with other
 *     values while the table is set, or one without groups, is BPLHIP_EINVAL;
 *   slots HOST u8 [n_rows, n_groups], 1 <= n_rows <= BPLHIP_TOURNAMENT_MAX_ALLOCATION_ROWS: in row r, the 0-based
 *     slot of the qualifier from group g, 0xFF for a group outside the row's set; the entries that are not 0xFF are
 *     a permutation of 0 .. best - 1;
 *   row_of_mask HOST u16 [1 << n_groups]: the row of the set of groups with bits m; every entry is below n_rows (0
 *     for a mask that is no row's), and the mask of row r maps back to r.  A call is BPLHIP_EINVAL unless every set of
 *     `best` groups with a place advance + 1 has its row;
 *   row_of_mask = slots = NULL with n_rows = 0 clears the table (n_groups and best are not read).
 * Both tables are copied.  The set and clear calls touch no device. */
#define BPLHIP_TOURNAMENT_MAX_ALLOCATION_ROWS 12870
int bplhip_tournament_set_allocation(bplhip_ctx* ctx, int32_t n_groups, int32_t best, int32_t n_rows,
                                     const uint16_t* row_of_mask, const uint8_t* slots);
/* simulate_tournament under the allocation in force, with its slot counts: bplhip_simulate_tournament_knockout's
 * argument list with the flag extra_time after head_to_head (as bplhip_tournament_paths has it: 0 = the redraw rule,
 * the five rule arguments, decided_counts and sim_decided are not read) and, last, the required output slot_counts
 * HOST u64 [n_groups, best_of_rest]: how often the qualifier from group g took allocation slot k, counted on the
 * device with integer atomics (bit-identical run to run).  BPLHIP_ESTATE without an allocation set. */
int bplhip_simulate_tournament_alloc(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx,
                                     const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                     const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                     const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                     const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                     const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                     int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                     uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage,
                                     void* stream, const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time,
                                     uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                     const double* strength, uint64_t* decided_counts, uint8_t* sim_decided,
                                     uint64_t* slot_counts);

/* ---- a tournament with group matches IN PROGRESS and weighted posterior draws (csrc/dc_tournament_live.hip.h):
 * bplhip_simulate_tournament_alloc's argument list, under its rules and with its outputs, with one difference:
 * slot_counts is read only while an allocation is set (NULL or not; without one it is ignored, there is no
 * BPLHIP_ESTATE: this entry serves both cases).  Then bplhip_simulate_season_live's request, the two sides of a match
 * in play as SLOTS in the listed order (as fix_p / fix_q) in place of model indices, then that symbol's outputs, then
 * the final scores.  The group fixtures are the CONCATENATED list of the n_fixtures fixtures still to kick off and then
 * the n_in_play matches in progress: match m is fixture n_fixtures + m (its threefry block is (j, n_fixtures + m), it
 * is booked once into the table and the pair matrix like any fixture and counts as a meeting to come in pair_init's
 * 16-bit bound).  The table (init_*) and pair_init do NOT contain the matches in progress.
 *   in_play_p, in_play_q   HOST u8[n_in_play] slots, two different slots of one group, in the listed order
 *   in_play_home_goals, in_play_away_goals   HOST u8[n_in_play] the current score of the LISTED sides (p, q), each at
 *                most BPLHIP_LIVE_MAX_GOALS
 *   in_play_elapsed, reweight, log_weights   as for bplhip_simulate_season_live
 * The venue of a match in play is decided as for any group fixture: with exactly one host among p and q the host is the
 * home side (on = 1), and when it is listed second the sides swap and the two goal counts of the state swap with them.
 * With l[s, m] as bplhip_simulate_season_live forms it from the state in the home / away orientation and the rates of
 * this symbol's matches (the venue branch form plus the confederations, in float64), L0, L, w, the scan C and W are
 * that symbol's, by the same kernel.  Weights are IN FORCE when log_weights is given or (reweight and n_in_play > 0).
 * Then simulation j plays EVERY match, in the groups and in the knockout rounds, on the draw
 *     s_j = #{s : C[s] < min((j + U) W / n_sims, W)},   U = (o0 + 0.5) 2^-32 of the threefry block (0, 0x20000000)
 * (capped at s - 1); otherwise on j mod s, and no weight is computed.  A match in progress draws its FINAL score from
 * that symbol's conditional law with these rates, by the same two walks; at 0-0, t = 0 it is bit for bit group fixture
 * n_fixtures + m of bplhip_simulate_tournament_alloc.  With n_in_play = 0 and log_weights = NULL the kernels and the
 * results are that symbol's.
 *   ess, log_evidence, sim_draw, draw_log_weights, draw_log_evidence   as for bplhip_simulate_season_live
 *   in_play_final_home, in_play_final_away   both NULL, or u8[n_sims, n_in_play]: the final scores of the LISTED sides
 * BPLHIP_EINVAL, before any device call, for everything bplhip_simulate_tournament_alloc refuses (a match in play is
 * checked like a group fixture: two different slots of one group) and for an elapsed outside [0, 1) or NaN, elapsed = 0
 * with a score other than 0-0, a current goal count above BPLHIP_LIVE_MAX_GOALS, n_fixtures + n_in_play >
 * BPLHIP_SEASON_MAX_FIXTURES, n_in_play > 0 without groups, a non-finite log weight, one final-score output without the
 * other.  Integer accumulation only and a fixed-order scan: bit-identical run to run.  Synchronous. */
int bplhip_simulate_tournament_live(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx,
                                    const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                    const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                    const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                    const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                    const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                    int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                    uint64_t* stage_counts, uint64_t* group_position_counts, uint8_t* sim_stage,
                                    void* stream, const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time,
                                    uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                    const double* strength, uint64_t* decided_counts, uint8_t* sim_decided,
                                    uint64_t* slot_counts, int32_t n_in_play, const uint8_t* in_play_p,
                                    const uint8_t* in_play_q, const uint8_t* in_play_home_goals,
                                    const uint8_t* in_play_away_goals, const double* in_play_elapsed, int32_t reweight,
                                    const double* log_weights, double* ess, double* log_evidence, int32_t* sim_draw,
                                    double* draw_log_weights, double* draw_log_evidence, uint8_t* in_play_final_home,
                                    uint8_t* in_play_final_away);

/* ---- the three tournament queries with group matches IN PROGRESS and weighted posterior draws
 * (csrc/dc_tournament_live_queries.hip.h).  Each takes the argument list of its kick-off entry, in its order and under
 * its rules, and then the live block of bplhip_simulate_tournament_live from n_in_play on, without the outputs the query
 * lacks: n_in_play, in_play_p, in_play_q, in_play_home_goals, in_play_away_goals, in_play_elapsed, reweight,
 * log_weights, ess, log_evidence, and -- the two entries with per-simulation records -- sim_draw, in_play_final_home,
 * in_play_final_away.  Their meaning, the checks and BPLHIP_EINVAL are that symbol's, by the same host code; the weights
 * are formed once per call by its two kernels, and simulation j here is simulation j there: the draw s_j, the ordinary
 * fixtures, the final score of match m on the block (j, n_fixtures + m), the ranking, the allocation fill and the
 * knockout.  The group-fixture axis of every output and every per-simulation array is the CONCATENATED list, the
 * n_fixtures fixtures still to kick off and then the n_in_play matches in progress, nf = n_fixtures + n_in_play:
 *   paths       nf <= BPLHIP_LEVERAGE_MAX_FIXTURES; outcome_counts [nf, 3], joint_counts [nf, 3, n, R + 1] and
 *               sim_outcome [n_sims, nf] class a match in progress by its FINAL score in the listed order;
 *   scenarios   key_fixture indexes the concatenated list (n_fixtures + m names match m in progress), the class is
 *               formed from the final score in the listed order;
 *   points      the axis must hold every total a slot can reach with the matches in progress among its matches to come.
 * sim_draw i32[n_sims] and the final scores u8[n_sims, n_in_play] are kept on the device for the whole call when asked
 * for; everything else passes through the chunked workspace as in the kick-off entries.  With n_in_play = 0 and
 * log_weights = NULL the kick-off kernels run and every output is the kick-off entry's; ess is then the number of
 * draws and log_evidence 0.  Integer accumulation only and a fixed-order scan: bit-identical run to run and for every
 * chunk_sims.  Synchronous. */
int bplhip_tournament_paths_live(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
                                 const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group,
                                 const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                 int64_t n_fixtures, const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                 int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket, int32_t win_points,
                                 int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
                                 uint32_t key_lo, uint64_t* stage_counts, uint64_t* group_position_counts,
                                 uint8_t* sim_stage, void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                 int32_t extra_time, uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                 const double* strength, uint64_t* decided_counts, uint8_t* sim_decided,
                                 int64_t chunk_sims, uint64_t* advance_counts, uint64_t* position_stage_counts,
                                 uint64_t* outcome_counts, uint64_t* target_counts, uint64_t* joint_counts,
                                 uint8_t* sim_position, uint8_t* sim_outcome, uint8_t* sim_pair, uint8_t* sim_winner,
                                 int32_t n_in_play, const uint8_t* in_play_p, const uint8_t* in_play_q,
                                 const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                 const double* in_play_elapsed, int32_t reweight, const double* log_weights,
                                 double* ess, double* log_evidence, int32_t* sim_draw, uint8_t* in_play_final_home,
                                 uint8_t* in_play_final_away);
int bplhip_tournament_scenarios_live(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx,
                                     const uint16_t* team_conf, const uint8_t* team_host, int32_t n_groups,
                                     const uint8_t* team_group, const int32_t* init_points, const int32_t* init_gf,
                                     const int32_t* init_ga, int64_t n_fixtures, const uint8_t* fix_p,
                                     const uint8_t* fix_q, int32_t advance, int32_t best_of_rest, int32_t n_bracket,
                                     const uint16_t* bracket, int32_t win_points, int32_t draw_points,
                                     int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo,
                                     void* stream, const uint32_t* pair_init, int32_t head_to_head, int32_t extra_time,
                                     uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                     const double* strength, uint64_t* decided_counts, int64_t chunk_sims,
                                     int32_t n_key, const int32_t* key_fixture, const int32_t* key_cap,
                                     uint64_t* scenario, uint64_t* joint, uint32_t* sim_scenario, uint8_t* sim_tset,
                                     int32_t n_in_play, const uint8_t* in_play_p, const uint8_t* in_play_q,
                                     const uint8_t* in_play_home_goals, const uint8_t* in_play_away_goals,
                                     const double* in_play_elapsed, int32_t reweight, const double* log_weights,
                                     double* ess, double* log_evidence, int32_t* sim_draw,
                                     uint8_t* in_play_final_home, uint8_t* in_play_final_away);
int bplhip_tournament_points_live(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* team_idx, const uint16_t* team_conf,
                                  const uint8_t* team_host, int32_t n_groups, const uint8_t* team_group,
                                  const int32_t* init_points, const int32_t* init_gf, const int32_t* init_ga,
                                  int64_t n_fixtures, const uint8_t* fix_p, const uint8_t* fix_q, int32_t advance,
                                  int32_t best_of_rest, int32_t n_bracket, const uint16_t* bracket, int32_t win_points,
                                  int32_t draw_points, int32_t loss_points, int64_t n_sims, uint32_t key_hi,
                                  uint32_t key_lo, void* stream, const uint32_t* pair_init, int32_t head_to_head,
                                  int32_t extra_time, uint32_t legs_mask, double extra_time_scale, int32_t away_goals,
                                  const double* strength, uint64_t* decided_counts, int64_t chunk_sims,
                                  int32_t points_min, int32_t n_bins, int32_t gd_cap, uint64_t* team_points,
                                  uint64_t* team_target, uint64_t* team_place, uint64_t* place_points,
                                  uint64_t* place_gap, uint64_t* rest_count, uint64_t* rest_through,
                                  uint64_t* rest_rank, int32_t n_in_play, const uint8_t* in_play_p,
                                  const uint8_t* in_play_q, const uint8_t* in_play_home_goals,
                                  const uint8_t* in_play_away_goals, const double* in_play_elapsed, int32_t reweight,
                                  const double* log_weights, double* ess, double* log_evidence);

/* ---- the table after every remaining matchday (csrc/dc_trajectory.hip.h): bplhip_simulate_season's simulations,
 * ranked after each matchday by the rule of the final table (points, not points per game; under the head-to-head
 * rule the mini-table over the matches booked so far; one tie-break word per slot for all matchdays), and the paths
 * counted on the device.  The arguments up to n_bins are bplhip_season_points', in its order and under its rules
 * and error codes (BPLHIP_ESTATE without a posterior, or with a venue-form posterior; n_fixtures <=
 * BPLHIP_LEVERAGE_MAX_FIXTURES; 1 <= n_targets <= BPLHIP_LEVERAGE_MAX_TARGETS; chunk_sims as there, a record being
 * 3 n_table n_rounds + n_rounds bytes), except that the axis must hold every total a slot PASSES THROUGH:
 * BPLHIP_EINVAL unless init_points[t] >= points_min and init_points[t] + m max(win, draw, loss points) < points_min +
 * n_bins for slot t with m remaining matches.  home_idx / away_idx are in the caller's order: fixture f takes the
 * random block (simulation, f) of bplhip_simulate_season whatever its matchday, so simulation j is simulation j
 * there and the table after the last matchday is its final table.
 *   the matchdays: 1 <= n_rounds <= BPLHIP_TRAJECTORY_MAX_ROUNDS; fix_id HOST i32[n_fixtures], the fixtures' indices
 *     sorted by matchday (a permutation of 0..n_fixtures-1); round_end HOST i32[n_rounds], non-decreasing and ending
 *     at n_fixtures: matchday r is fix_id[round_end[r-1] .. round_end[r]) (an empty matchday repeats the table before
 *     it).  The table after matchday r is the current table plus every fixture of matchdays 0..r.  BPLHIP_EINVAL
 *     otherwise;
 *   required outputs, HOST u64, n = n_table, K = n_targets, R = n_rounds:
 *     position_count [R, n, n] (slot t is in position p after matchday r), target_count [R, n, K] (inside target k),
 *     target_final_count [R, n, K] (inside after matchday r AND after the last), points_sum and points_sq_sum [R, n]
 *     (the sums over the simulations of v = points - points_min and of v^2), rounds_inside_count [n, K, R + 1] (the
 *     number of matchdays after which slot t was inside target k), secured_count [n, K, R + 1] (bin r < R: the first
 *     matchday from which t is inside k after that and every later matchday; bin R: outside at the end),
 *     lead_changes_count [R] (the number of matchdays r >= 1 whose leader differs from matchday r - 1's);
 *   pair_init: as for bplhip_season_points.
 * Per-simulation tables never leave the device.  Integer accumulation only: the outputs are bit-identical run to run
 * and for every chunk_sims.  Synchronous. */
#define BPLHIP_TRAJECTORY_MAX_ROUNDS 256
int bplhip_season_trajectory(bplhip_ctx* ctx, int64_t n_fixtures, const uint16_t* home_idx, const uint16_t* away_idx,
                             int32_t n_table, const uint16_t* table_idx, const int32_t* init_points,
                             const int32_t* init_gf, const int32_t* init_ga, int32_t win_points, int32_t draw_points,
                             int32_t loss_points, int64_t n_sims, uint32_t key_hi, uint32_t key_lo, int32_t n_targets,
                             const uint64_t* target_mask, int64_t chunk_sims, int32_t points_min, int32_t n_bins,
                             int32_t n_rounds, const int32_t* round_end, const int32_t* fix_id,
                             uint64_t* position_count, uint64_t* target_count, uint64_t* target_final_count,
                             uint64_t* points_sum, uint64_t* points_sq_sum, uint64_t* rounds_inside_count,
                             uint64_t* secured_count, uint64_t* lead_changes_count, void* stream,
                             const uint32_t* pair_init);

/* ---- pointwise log-likelihood of the uploaded posterior (csrc/dc_loglik.hip.h), for WAIC and PSIS-LOO.
 * Per draw s and fixture n, in float64:
 *     ll[s, n] = x log lh - lh - lgamma(x+1) + y log la - la - lgamma(y+1)
 *                + [x <= 1 and y <= 1] log(max(1 + corr_coef[s] c(x, y), 0))
 * with the rates and tau coefficient of bplhip_predict_score_proba: the mean over the draws of exp(ll) is
 * that entry's output.  A clipped tau gives -inf.  Unweighted: fit-time weights play no part.  Fixtures with
 * goals, m >= 0.  The posterior's draws must number at most BPLHIP_LOGLIK_MAX_DRAWS (the upload itself has no
 * such limit).  The first call after an upload builds team-major copies of the tables on the device.
 * Synchronous; bit-identical run to run.
 *   matrix:  out HOST f64[s, m] (row = draw).
 *   summary: per fixture, HOST f64[m] each: lppd = log mean_s exp(ll), mean and var (1/(S-1); 0 for
 *     S = 1) of ll over the draws.  With psis != 0 also elpd_loo and pareto_k (PSIS-LOO with the
 *     tail size M = min(ceil(min(0.2 S, 3 sqrt(S / r_eff))), S - 1), which must not exceed
 *     BPLHIP_LOGLIK_MAX_TAIL; r_eff finite and > 0) and, when not NULL, tail_len HOST i32[m], the
 *     number of draws in the smoothed tail; the definition is DESIGN.md section 12.  A fixture with
 *     ll = -inf in some draw has mean = elpd_loo = -inf, var = pareto_k = +inf, tail_len = 0.  No
 *     output is NaN for finite posterior tables.  Without psis, elpd_loo, pareto_k and tail_len are
 *     not read (may be NULL) and r_eff is not checked. */
#define BPLHIP_LOGLIK_MAX_DRAWS 65536
#define BPLHIP_LOGLIK_MAX_TAIL 1024
int bplhip_loglik_matrix(bplhip_ctx* ctx, const bplhip_fixtures* q, double* out, void* stream);
int bplhip_loglik_summary(bplhip_ctx* ctx, const bplhip_fixtures* q, double r_eff, int32_t psis, double* lppd,
                          double* mean, double* var, double* elpd_loo, double* pareto_k, int32_t* tail_len,
                          void* stream);

/* ---- outcome probabilities and proper scoring rules of the uploaded posterior on fixtures with known
 * results (csrc/dc_score.hip.h).  Per draw s and fixture n, in float64, on the grid 0 <= x, y <= max_goals
 * (0..63), NOT renormalised:
 *     q(x, y) = max(1 + corr_coef[s] c(x, y), 0) Pois(x; lh) Pois(y; la)
 *     p_H, p_D, p_A = the sums of q over x > y, x = y, x < y
 * with the rates and the tau coefficient c of the log-likelihood above, in O(max_goals) per (s, n).  The
 * observed class o of a fixture is home (0) for home_goals > away_goals, draw (1) for equal goals, else
 * away (2); the goals themselves may exceed max_goals.  Fixtures with goals, m >= 1 (BPLHIP_EINVAL
 * otherwise); at most BPLHIP_LOGLIK_MAX_DRAWS draws.
 *   proba      HOST f64[m, 3]: the mean over the draws of (p_H, p_D, p_A), the average that
 *              bplhip_predict_score_grid's triangles approximate in float32
 *   draw_sums  HOST f64[s, 3]: per draw, the sums over the m fixtures of log p_o,
 *              sum_k (p_k - [k = o])^2 and ((p_H - o_H)^2 + (p_H + p_D - o_H - o_D)^2) / 2 of that draw's
 *              own probabilities.  A zero p_o gives -inf; no output is NaN.
 * The [s, m, 3] array is never stored.  Synchronous; bit-identical run to run (fixed summation orders,
 * no floating-point atomics). */
int bplhip_outcome_scores(bplhip_ctx* ctx, const bplhip_fixtures* q, int32_t max_goals, double* proba,
                          double* draw_sums, void* stream);

/* ---- leave-one-out forecasts of fixtures the fit has seen (csrc/dc_loo.hip.h): each
 * fixture's own PSIS-LOO weights applied to its per-draw forecasts.  Per fixture, the log ratios r = -ll over the
 * draws are Pareto smoothed exactly as bplhip_loglik_summary smooths them with psis != 0 (the same tail size from
 * r_eff, order, fit and cap; raw ratios where nothing is smoothed) and normalised to weights w_s.  With p_s and q_s
 * the per-draw outcome probabilities and grid of bplhip_outcome_scores on 0..max_goals (0..63), and x, y the
 * fixture's actual goals (they may exceed max_goals), HOST outputs:
 *   elpd_loo, pareto_k  f64[m], tail_len i32[m]: what bplhip_loglik_summary gives
 *   ess                 f64[m] = 1 / sum_s w_s^2
 *   proba               f64[m, 3] = sum_s w_s p_s, the leave-one-out forecast
 *   proba_in_sample     f64[m, 3] = mean_s p_s, the proba of bplhip_outcome_scores
 *   pit                 f64[m, 4]: home lower = sum_s w_s sum_{a < x} sum_b q_s(a, b) and upper (a <= x), then the
 *                       away pair on the other marginal with y; a, b on 0..max_goals, so a count above max_goals
 *                       gives lower = upper = the weighted grid mass
 * A fixture with ll = -inf in some draw takes the limit: uniform weights over those draws, 0 elsewhere; elpd_loo =
 * -inf, pareto_k = +inf, tail_len = 0, ess = their number, every probability finite.  No output is NaN for finite
 * posterior tables.  Fixtures with goals, m >= 0 (m = 0 writes nothing); the checks and codes are those of
 * bplhip_loglik_summary with psis != 0 plus max_goals, every one before any device call; no output may be NULL for
 * m > 0.  Synchronous; bit-identical run to run, and a fixture's outputs do not depend on where it stands in the
 * query (fixed summation orders, no floating-point atomics). */
int bplhip_loo_scores(bplhip_ctx* ctx, const bplhip_fixtures* q, double r_eff, int32_t max_goals, double* elpd_loo,
                      double* pareto_k, int32_t* tail_len, double* ess, double* proba, double* proba_in_sample,
                      double* pit, void* stream);

/* ---- sequential updating of the uploaded posterior by the results of fixtures seen since the fit
 * (csrc/dc_sequential.hip.h): PSIS leave-future-out.  The fixtures carry a block index (a
 * gameweek, say) in 0..n_blocks-1, in any order; 1 <= n_blocks <= BPLHIP_SEQ_MAX_BLOCKS.  ll[s, n] is the
 * log-likelihood of bplhip_loglik_matrix.  The caller forms the log ratios between the two steps: R[b, s] = sum
 * of A[b', s] over b' < b (R[0, .] = 0), adding the A of several calls first when the fixtures are spread over
 * several posteriors.
 *   bplhip_block_loglik  fixtures with goals, m >= 1, plus HOST i32 block_idx[m].  out HOST f64[n_blocks, s]:
 *       A[b, s] = the sum of ll[s, n] over the fixtures of block b (fixtures in query order, in chunks of 64: a
 *       fixed order), 0 for a block without fixtures.  A clipped tau gives -inf.  At most
 *       BPLHIP_LOGLIK_MAX_DRAWS draws.
 *   bplhip_psis_weights  needs no posterior.  log_ratios HOST f64[n_blocks, n_draws], every value finite or
 *       -inf; 1 <= n_draws <= BPLHIP_LOGLIK_MAX_DRAWS; r_eff finite and > 0 with a tail size within
 *       BPLHIP_LOGLIK_MAX_TAIL, as bplhip_loglik_summary.  Per block, the row is Pareto smoothed over the
 *       draws exactly as bplhip_loglik_summary smooths r = -ll and normalised:
 *       log_weights HOST f64[n_blocks, n_draws] (each row's exp sums to one), pareto_k, ess =
 *       exp(-lse(2 log_weights)) HOST f64[n_blocks], tail_len HOST i32[n_blocks].  A row of equal values has
 *       uniform weights, pareto_k = 0, tail_len = 0; a row of -inf only (a dead block) has log_weights =
 *       -inf, pareto_k = +inf, ess = 0, tail_len = 0; a single -inf among finite values is a weight of 0.
 *   bplhip_weighted_scores  fixtures and block_idx as bplhip_block_loglik, log_weights HOST
 *       f64[n_blocks, s], max_goals in 0..63.  Per fixture n of block b: elpd HOST f64[m] =
 *       lse_s(log_weights[b, s] + ll[s, n]) and proba HOST f64[m, 3] = sum_s exp(log_weights[b, s])
 *       (p_H, p_D, p_A)(s, n), the per-draw outcome probabilities of bplhip_outcome_scores.  Output in query
 *       order.  A dead block gives elpd = -inf and proba = 0.
 * BPLHIP_EINVAL for m < 1, n_blocks, n_draws, max_goals or a block index out of range, a bad r_eff, a NaN or
 * +inf log ratio, or a null argument; every check before any device call.  No output is NaN.  Synchronous;
 * bit-identical run to run (fixed summation orders, no floating-point atomics). */
#define BPLHIP_SEQ_MAX_BLOCKS 4096
int bplhip_block_loglik(bplhip_ctx* ctx, const bplhip_fixtures* q, const int32_t* block_idx, int32_t n_blocks,
                        double* out, void* stream);
int bplhip_psis_weights(bplhip_ctx* ctx, int32_t n_blocks, int32_t n_draws, const double* log_ratios, double r_eff,
                        double* log_weights, double* pareto_k, double* ess, int32_t* tail_len, void* stream);
int bplhip_weighted_scores(bplhip_ctx* ctx, const bplhip_fixtures* q, const int32_t* block_idx, int32_t n_blocks,
                           const double* log_weights, int32_t max_goals, double* elpd, double* proba, void* stream);

/* ---- match markets with credible intervals, of the uploaded posterior (csrc/dc_market.hip.h).  A market k is
 * a linear functional of one draw's scoreline grid, with weights W_k[x, y] (x = home goals), any finite values.
 * Per draw s and fixture n, in float64, on the grid 0 <= x, y <= max_goals (0..63), NOT renormalised:
 *     v[s, k, n] = sum_{x, y} W_k[x, y] q(x, y),   q as in bplhip_outcome_scores
 * (the three triangles as W give its p_H, p_D, p_A).  Per (k, n), over the s draws: the mean, the standard
 * deviation (ddof = 1; 0 for one draw) and, for each requested q in [0, 1], the linearly interpolated
 * quantile: with h = q (s - 1), v_(floor h) + (h - floor h) (v_(floor h + 1) - v_(floor h)) on the EXACT order
 * statistics v_(0) <= v_(1) <= ... of the per-draw values (numpy's default "linear" method).
 * Fixtures without goals, m >= 1; at most BPLHIP_LOGLIK_MAX_DRAWS draws.
 *   n_markets    1..BPLHIP_MARKET_MAX_MARKETS; weights HOST f64[n_markets, (max_goals+1)^2], all finite
 *   n_quantiles  0..BPLHIP_MARKET_MAX_QUANTILES; quantiles HOST f64[n_quantiles], each in [0, 1] (not NaN);
 *                may be NULL for n_quantiles = 0, and then quantile may be NULL too
 *   mean, sd     HOST f64[n_markets, m]
 *   quantile     HOST f64[n_markets, n_quantiles, m]
 *   draws        NULL, or HOST f64[m, n_markets, s]: every per-draw value (a fixture's draws contiguous)
 *   workspace_bytes  caps the device memory held beyond the inputs and outputs: the per-draw values of a
 *                chunk of fixtures, f64[chunk, n_markets, s]; the fixtures are walked in chunks that fit.
 *                0 = BPLHIP_MARKET_WORKSPACE_BYTES.  Negative, or too small for one fixture
 *                (n_markets x s x 8 bytes): BPLHIP_EINVAL.
 * BPLHIP_EINVAL also for max_goals, n_markets, n_quantiles or m out of range, a quantile outside [0, 1] or NaN,
 * a non-finite weight or a null argument; every check before any device call.  Synchronous; bit-identical run
 * to run, for any workspace_bytes and any order of the fixtures (fixed summation orders, no floating-point
 * atomics). */
#define BPLHIP_MARKET_MAX_MARKETS 64
#define BPLHIP_MARKET_MAX_QUANTILES 16
#define BPLHIP_MARKET_WORKSPACE_BYTES (256ll << 20)
int bplhip_market_summary(bplhip_ctx* ctx, const bplhip_fixtures* q, int32_t max_goals, int32_t n_markets,
                          const double* weights, int32_t n_quantiles, const double* quantiles, double* mean,
                          double* sd, double* quantile, double* draws, int64_t workspace_bytes, void* stream);

/* ---- period markets with credible intervals, of the uploaded posterior (csrc/dc_period.hip.h; DESIGN.md section
 * 39): markets on the score at a SPLIT of the match together with the final score -- the half-time result,
 * half-time/full-time, win both halves, a goal in the first ten minutes.  Goal times are exchangeable within a match
 * (the assumption of bplhip_inplay_summary), so with f = split[fixture] the share of the match's scoring before the
 * split, per draw s and fixture n, in float64, over 0 <= a <= x <= max_goals, 0 <= b <= y <= max_goals:
 *     p(a, b, x, y) = F(x, y) Pois(a; f lh) Pois(x - a; (1 - f) lh) Pois(b; f la) Pois(y - b; (1 - f) la)
 *     v[s, k, n]    = sum W_k[a, b, x, y] p(a, b, x, y)
 * (a, b) the score at the split, (x, y) the final score, F = max(1 + rho c, 0) on the final scores {0, 1}^2 with the
 * full-match rates (the tau of bplhip_outcome_scores; a clipped cell contributes an exact 0) and 1 elsewhere;
 * Pois(0; 0) = 1, Pois(k > 0; 0) = 0.  NOT renormalised, truncated by the final score only: sum_{a, b} p is the q of
 * bplhip_market_summary for every f.  Per (k, n), over the s draws: mean, sd and quantiles exactly as
 * bplhip_market_summary defines them.  Fixtures without goals, m >= 1; at most BPLHIP_LOGLIK_MAX_DRAWS draws.
 *   split        HOST f64[m], each finite and in [0, 1]
 *   max_goals    0..BPLHIP_PERIOD_MAX_GOALS
 *   n_markets    1..BPLHIP_PERIOD_MAX_MARKETS; weights HOST f64[n_markets, (max_goals+1)^4] indexed [a, b, x, y];
 *                the cells with a > x or b > y are never read, every other weight is finite
 *   n_quantiles, quantiles, mean, sd, quantile, draws, workspace_bytes   as for bplhip_market_summary
 * The checks follow bplhip_market_summary's order and codes, then BPLHIP_EINVAL for a split outside [0, 1] or NaN
 * and for a non-finite weight on a cell that is read; every check before any device call.  Synchronous; bit-identical
 * run to run, for any workspace_bytes and any order of the fixtures. */
#define BPLHIP_PERIOD_MAX_GOALS 31
#define BPLHIP_PERIOD_MAX_MARKETS 32
int bplhip_period_summary(bplhip_ctx* ctx, const bplhip_fixtures* q, const double* split, int32_t max_goals,
                          int32_t n_markets, const double* weights, int32_t n_quantiles, const double* quantiles,
                          double* mean, double* sd, double* quantile, double* draws, int64_t workspace_bytes,
                          void* stream);

/* ---- totals over SLATES of fixtures, of the uploaded posterior (csrc/dc_slate.hip.h): an
 * accumulator, the number of home wins of a matchday, the points of a prediction-league entry.  A leg table gives
 * every final score (x, y) on the grid 0 <= x, y <= max_goals (0..63) an integer value 0..BPLHIP_SLATE_VALUES-1;
 * fixture i plays under table leg_table[i], with m_i the table's largest value.  Slate j holds the fixtures
 * start[j] .. start[j+1]-1 of the record, in the order given, and its total is T_j = sum_i value_i.  Per draw s, in
 * float64, with q as in bplhip_market_summary (NOT renormalised):
 *     r_i[v]  = sum_{(x, y): table(x, y) = v} q(x, y)                       the fixture's value law
 *     pmf     = r_1 * r_2 * ... (convolution, in list order), t = 0..P      P = the largest sum m_i of the call's slates
 *     at_least[t] = sum_{u >= t} pmf[u];  expected = sum_t t pmf[t];  mass = at_least[0] = prod_i (grid mass of i)
 * The fixtures are independent GIVEN the draw, so a draw's pmf is exact; they share the posterior, so the statistics
 * are formed per draw and then summarised over the s draws exactly as bplhip_market_summary defines mean, sd and
 * quantiles.  The K = 2 (P + 1) + 2 statistics of a slate are ordered pmf[0..P], at_least[0..P], expected, mass;
 * beyond a slate's own sum m_i every pmf and at_least entry is an exact 0.
 * Fixtures without goals, m >= 1; at most BPLHIP_LOGLIK_MAX_DRAWS draws.
 *   n_slates     1..m; start HOST i32[n_slates + 1], start[0] = 0 < ... < start[n_slates] = m; at most
 *                BPLHIP_SLATE_MAX_LEGS fixtures and sum m_i <= BPLHIP_SLATE_MAX_TOTAL per slate
 *   n_tables     1..m; tables HOST u8[n_tables, (max_goals+1)^2] (x major), every value below BPLHIP_SLATE_VALUES;
 *                leg_table HOST i32[m], each in [0, n_tables)
 *   n_quantiles, quantiles   as for bplhip_market_summary
 *   mean, sd     HOST f64[K, n_slates];  quantile HOST f64[K, n_quantiles, n_slates]
 *   leg_mean     HOST f64[BPLHIP_SLATE_VALUES, m]: the mean over the draws of r_i[v]
 *   draws        NULL, or HOST f64[n_slates, P + 1, s]: every per-draw pmf
 *   workspace_bytes  caps the device memory for the per-draw values of a chunk of consecutive slates: a slate takes
 *                (K + BPLHIP_SLATE_VALUES x its fixtures) x s x 8 bytes.  0 = BPLHIP_MARKET_WORKSPACE_BYTES.  Negative,
 *                or too small for the largest slate: BPLHIP_EINVAL.
 * The checks follow bplhip_market_summary's order and codes (max_goals and n_quantiles, the fixtures record, then
 * the rest: BPLHIP_EINVAL); every check before any device call.  Synchronous; bit-identical run to run, for any
 * workspace_bytes and under any reordering of the record that keeps each slate's own order (fixed summation
 * orders, no floating-point atomics). */
#define BPLHIP_SLATE_VALUES 8
#define BPLHIP_SLATE_MAX_TOTAL 127
#define BPLHIP_SLATE_MAX_LEGS 1024
int bplhip_slate_summary(bplhip_ctx* ctx, const bplhip_fixtures* q, int32_t max_goals, int32_t n_slates,
                         const int32_t* start, int32_t n_tables, const uint8_t* tables, const int32_t* leg_table,
                         int32_t n_quantiles, const double* quantiles, double* mean, double* sd, double* quantile,
                         double* leg_mean, double* draws, int64_t workspace_bytes, void* stream);

/* ---- team ratings: how a team does against a FIELD of opponents, of the uploaded posterior
 * (csrc/dc_ratings.hip.h).  Per draw s and rated team t, over the n_t matches t plays against
 * the opponents other than itself, walked in the order given, in float64:
 *   venue 0 "both": per opponent t hosts, then t visits; 1 "home": t hosts; 2 "away": t visits; 3 "neutral": t listed
 *   first on neutral ground (a posterior set with predict_set_posterior_venue only).  Under 0..2 a venue posterior
 *   plays at the home side's ground (neutral_venue = 0).
 *   per match (p_H, p_D, p_A) as in bplhip_outcome_scores at depth max_goals (0..63, not renormalised), seen from t:
 *     k = 0 points           sum (points[0] p_win + points[1] p_draw + points[2] p_loss) / n_t
 *     k = 1 win              sum p_win / n_t
 *     k = 2 goals_for        sum (t's scoring rate) / n_t      the rates are the marginal means of the unclipped
 *     k = 3 goals_against    sum (the opponent's rate) / n_t   law, NOT truncated at max_goals
 *     k = 4 goal_difference  (sum goals_for - sum goals_against) / n_t
 * Over the s draws, per (k, t): mean, sd and quantiles exactly as bplhip_market_summary defines them.  Per draw the
 * rated teams are ranked by statistic rank_by, larger better: the rank of t is the number of rated teams with a
 * strictly larger value plus the number with an equal value listed earlier, so a draw's ranks are a permutation.
 *   n_teams, n_opponents   1..BPLHIP_RATINGS_MAX_TEAMS; teams, opponents HOST u16 model indices, no duplicates within
 *                either list; every rated team needs an opponent other than itself
 *   team_conf, opponent_conf   HOST u16 confederation indices, exactly when the posterior has confederations; else NULL
 *   points       HOST f64[3] (win, draw, loss), all finite;  rank_by 0..4
 *   n_quantiles, quantiles   as for bplhip_market_summary
 *   mean, sd     HOST f64[5, n_teams];  quantile HOST f64[5, n_quantiles, n_teams]
 *   rank_count   HOST i32[n_teams, n_teams]: [t, r] the draws in which t held rank r (0 the best)
 *   better_count HOST i32[n_teams, n_teams]: [t, u] the draws with value_t > value_u, strictly
 *   matches      HOST i32[n_teams]: n_t
 *   draws        NULL, or HOST f64[n_teams, 5, s]: every per-draw value (a statistic's draws contiguous)
 *   workspace_bytes  caps the per-draw values of a chunk of rated teams, f64[chunk, 5, s]; the teams are walked in
 *                chunks that fit.  0 = BPLHIP_RATINGS_WORKSPACE_BYTES.  Negative, or too small for one team
 *                (5 x s x 8 bytes): BPLHIP_EINVAL.  The ranked statistic of ALL rated teams, f64[n_teams, s], stays
 *                resident across the chunks: an input-sized buffer of its own, not counted here.
 * BPLHIP_ESTATE without a posterior.  BPLHIP_EINVAL for a count, venue, max_goals, rank_by or n_quantiles out of
 * range, more than BPLHIP_LOGLIK_MAX_DRAWS draws, a null argument, venue 3 on a plain posterior, confederations
 * missing or superfluous, an index out of range, a duplicate, a team whose only opponent is itself, a non-finite
 * point value, a bad quantile or workspace; every check before any device call.  Synchronous; bit-identical run to
 * run and for any workspace_bytes (fixed summation orders, integer counts, no floating-point atomics). */
#define BPLHIP_RATINGS_MAX_TEAMS 1024
#define BPLHIP_RATINGS_WORKSPACE_BYTES (256ll << 20)
int bplhip_team_ratings(bplhip_ctx* ctx, int32_t n_teams, const uint16_t* teams, const uint16_t* team_conf,
                        int32_t n_opponents, const uint16_t* opponents, const uint16_t* opponent_conf, int32_t venue,
                        int32_t max_goals, const double* points, int32_t rank_by, int32_t n_quantiles,
                        const double* quantiles, double* mean, double* sd, double* quantile, int32_t* rank_count,
                        int32_t* better_count, int32_t* matches, double* draws, int64_t workspace_bytes, void* stream);

/* ---- markets of a match IN PROGRESS, of the uploaded posterior (csrc/dc_inplay.hip.h).
 * The fixtures record carries the CURRENT score in its goal columns; elapsed[i] in [0, 1) is the fraction of the
 * match played, r = 1 - elapsed.  With goal times exchangeable within a match, per draw s and fixture n, in float64:
 *     u_i = Pois(i; lh r), v_j = Pois(j; la r)               lh, la the FULL-MATCH rates of the draw
 *     p~(x, y) = f(x, y) u_(x-a) v_(y-b)                     a <= x <= max_goals, b <= y <= max_goals; f the clipped
 *                                                            tau factor of the FINAL cell on {0,1}^2, else 1
 *     Z = 1 + sum over the tau cells with x >= a, y >= b of (f - 1) u_(x-a) v_(y-b)      (untruncated support)
 *     v[s, k, n] = (sum_{x, y} W_k[x, y] p~(x, y)) / Z       W indexed by the FINAL score; mass beyond max_goals dropped
 *     l[s, n]    = log Pois(a; lh t) + log Pois(b; la t) + log Z                          (Pois(0; 0) = 1)
 * The draws are re-weighted PER FIXTURE: w[s, n] = exp(L - max_s L), L = (l if reweight) + (log_weights[s] if given).
 * Per (k, n): mean = sum w v / sum w; sd = sqrt(sum w (v - mean)^2 / sum w) (population form); for each q the
 * weighted inverted CDF: the draws sorted by v (ties by draw), C the scan of w in that order and W its last element,
 * the order statistic at the first i with C_i >= q W; no interpolation; q = 0 is the minimum and q = 1 the maximum.
 * Per fixture: ess = (sum w)^2 / sum w^2 and log_evidence = log mean_s exp(l), from l alone whatever reweight is.
 * NOT modelled: goal intensity that varies over the match, red cards and game state, stoppage time (the caller maps
 * the clock to elapsed), a joint update over several matches in progress (each fixture is updated on its own).
 * Fixtures with goals, m >= 1; at most BPLHIP_INPLAY_MAX_DRAWS draws (the sort of a (fixture, market) lives in LDS).
 *   elapsed      HOST f64[m], each in [0, 1) (not NaN); 0 only with the score 0-0
 *   max_goals, n_markets, weights, n_quantiles, quantiles    as for bplhip_market_summary; no goal count above max_goals
 *   reweight     nonzero: l enters the weights
 *   log_weights  NULL, or HOST f64[s], all finite (a row of bplhip_psis_weights' log_weights, say)
 *   mean, sd     HOST f64[n_markets, m];  quantile HOST f64[n_markets, n_quantiles, m]
 *   ess, log_evidence   HOST f64[m]
 *   draws        NULL, or HOST f64[m, n_markets, s];  draw_log_evidence NULL, or HOST f64[m, s]
 *   workspace_bytes  as for bplhip_market_summary; a fixture takes (n_markets + 1) x s x 8 bytes
 * The checks follow bplhip_market_summary's order and codes, then BPLHIP_EINVAL for an elapsed outside [0, 1) or
 * NaN, a goal count above max_goals, elapsed = 0 with a score other than 0-0, a non-finite log weight; more than
 * BPLHIP_INPLAY_MAX_DRAWS draws is BPLHIP_EINVAL where bplhip_market_summary checks its own limit.  Every check before
 * any device call.  Synchronous; bit-identical run to run, for any workspace_bytes and any order of the fixtures. */
#define BPLHIP_INPLAY_MAX_DRAWS 12288
int bplhip_inplay_summary(bplhip_ctx* ctx, const bplhip_fixtures* q, const double* elapsed, int32_t max_goals,
                          int32_t n_markets, const double* weights, int32_t n_quantiles, const double* quantiles,
                          int32_t reweight, const double* log_weights, double* mean, double* sd, double* quantile,
                          double* ess, double* log_evidence, double* draws, double* draw_log_evidence,
                          int64_t workspace_bytes, void* stream);

/* ---- MCMC convergence diagnostics of posterior draws (csrc/dc_diagnostics.hip.h): the rank-normalised split
 * R-hat, the bulk, tail and mean effective sample sizes and the Monte Carlo standard error of the mean of Vehtari,
 * Gelman, Simpson, Carpenter and Buerkner (2021), per scalar quantity, in float64.  Needs no fixtures and no
 * posterior.  values HOST f64[n_chains * n_draws, n_quantities], chain-major rows (chain c's draws are rows
 * c n_draws .. (c + 1) n_draws - 1); every column is one quantity.  Each chain is split into its first and its
 * last n = n_draws / 2 draws: M = 2 n_chains chains, S = M n values, S <= BPLHIP_DIAG_MAX_DRAWS.  The definitions
 * are DESIGN.md section 20.
 *   n_chains     1..BPLHIP_DIAG_MAX_CHAINS; n_draws >= 8; n_quantities >= 1
 *   n_quantiles  0..BPLHIP_DIAG_MAX_QUANTILES; quantiles HOST f64[n_quantiles], each strictly inside (0, 1):
 *                ess_tail is the least ess of the indicators x <= (that quantile of the S split values); NaN
 *                for n_quantiles = 0
 *   mean, sd     HOST f64[n_quantities] over all n_chains * n_draws draws (sd with ddof = 1)
 *   rhat, ess_bulk, ess_tail, ess_mean, mcse_mean   HOST f64[n_quantities]; NaN for a quantity with a
 *                non-finite draw or whose S split values are all equal; rhat NaN for W = 0, an ess NaN for
 *                var_plus = 0, mcse_mean = sd / sqrt(ess_mean) NaN with ess_mean
 *   workspace_bytes  caps the device memory held beyond the draws and the outputs: per quantity of a chunk
 *                16 S bytes (+ 12 S when S > 12288: the sort then runs through the workspace instead of LDS)
 *                and 8 per quantile; the quantities are walked in chunks that fit.
 *                0 = BPLHIP_DIAG_WORKSPACE_BYTES.  Negative, or too small for one quantity: BPLHIP_EINVAL.
 * BPLHIP_EINVAL also for any argument out of range, a quantile outside (0, 1) or NaN, or a null argument; every
 * check before any device call.  Synchronous; bit-identical run to run and for any workspace_bytes (fixed
 * summation orders, an exact sort, no floating-point atomics). */
#define BPLHIP_DIAG_MAX_DRAWS 65536
#define BPLHIP_DIAG_MAX_CHAINS 256
#define BPLHIP_DIAG_MAX_QUANTILES 16
#define BPLHIP_DIAG_WORKSPACE_BYTES (256ll << 20)
int bplhip_mcmc_diagnostics(bplhip_ctx* ctx, int32_t n_chains, int32_t n_draws, int64_t n_quantities,
                            const double* values, int32_t n_quantiles, const double* quantiles,
                            int64_t workspace_bytes, double* mean, double* sd, double* rhat, double* ess_bulk,
                            double* ess_tail, double* ess_mean, double* mcse_mean, void* stream);

/* ---- weighted shift of posterior quantities (csrc/dc_sensitivity.hip.h): how far the distribution of every
 * scalar quantity moves when the draws are re-weighted by rows of importance ratios -- the symmetrised, normalised
 * cumulative Jensen-Shannon distance of power-scaling sensitivity analysis (Kallioinen, Paananen, Buerkner and
 * Vehtari 2023), squared, with the weighted mean and sd, in float64.  Needs no fixtures and no posterior.  The
 * rows are Pareto-smoothed exactly as bplhip_psis_weights smooths them; the definitions are DESIGN.md section 33.
 *   n_draws      8..BPLHIP_DIAG_MAX_DRAWS; n_quantities >= 1
 *   values       HOST f64[n_draws, n_quantities]; every column is one quantity
 *   n_rows       1..BPLHIP_SHIFT_MAX_ROWS; log_ratios HOST f64[n_rows, n_draws], all finite
 *   r_eff        as in bplhip_psis_weights
 *   log_weights  HOST f64[n_rows, n_draws]; pareto_k, ess HOST f64[n_rows]; tail_len HOST i32[n_rows]: what
 *                bplhip_psis_weights returns for these rows
 *   cjs_sq, mean, sd   HOST f64[n_rows, n_quantities]; sd = sqrt(sum w (x - mean)^2) with the normalised weights.
 *                cjs_sq is NaN for a quantity with a non-finite draw or whose draws are all equal; both keep
 *                mean and sd
 *   workspace_bytes  caps the device memory held beyond the draws and the outputs: 12 n_draws bytes per
 *                quantity of a chunk when n_draws > 12288 (the sort then runs through the workspace instead of
 *                LDS), nothing otherwise; the quantities are walked in chunks that fit.
 *                0 = BPLHIP_SHIFT_WORKSPACE_BYTES.  Negative, or too small for one quantity: BPLHIP_EINVAL.
 * BPLHIP_EINVAL also for any argument out of range, a non-finite ratio, a PSIS tail over BPLHIP_LOGLIK_MAX_TAIL
 * or a null argument; every check before any device call.  Synchronous; bit-identical run to run and for any
 * workspace_bytes (fixed summation orders, an exact sort, no floating-point atomics). */
#define BPLHIP_SHIFT_MAX_ROWS 8
#define BPLHIP_SHIFT_WORKSPACE_BYTES (256ll << 20)
int bplhip_weighted_shift(bplhip_ctx* ctx, int32_t n_draws, int64_t n_quantities, const double* values,
                          int32_t n_rows, const double* log_ratios, double r_eff, int64_t workspace_bytes,
                          double* log_weights, double* pareto_k, double* ess, int32_t* tail_len,
                          double* cjs_sq, double* mean, double* sd, void* stream);

/* ---- posterior predictive replications of observed fixtures (csrc/dc_ppc.hip.h), for posterior
 * predictive checks.  Replication r (0 <= r < n_reps) takes posterior draw r mod s for every fixture; fixture i
 * draws its scoreline with bplhip_simulate_season's exact sampler (no max_goals truncation, goals capped at 255)
 * on the threefry-2x32-20 block (r, f) under key_hi:key_lo, f = fixture_id[i] (NULL: f = i).  Rates: those of
 * bplhip_simulate_season (plain form), or of bplhip_simulate_tournament with on = 1 - neutral_venue[i] and the
 * fixture's confederations (venue form).  Each replication is reduced on the device; nothing per fixture is
 * stored unless home_goals / away_goals are given.
 *   fixtures without goals, 1 <= m <= BPLHIP_PPC_MAX_FIXTURES; home_slot, away_slot HOST u16[m] team slots
 *     < n_slots (1 <= n_slots <= BPLHIP_PPC_MAX_TEAMS: the caller's numbering, so calls on parts of one
 *     dataset add up); fixture_id HOST u32[m] or NULL.  1 <= max_goals <= BPLHIP_PPC_MAX_GOALS; 1 <= n_reps <=
 *     BPLHIP_PPC_MAX_REPLICATIONS and n_reps x n_slots <= BPLHIP_PPC_MAX_TEAM_CELLS.
 *   outputs, per replication row (HOST, all written):  score_counts u32[n_reps, max_goals+1, max_goals+1]
 *     (row min(x, max_goals), column min(y, max_goals)); outcome_counts u32[n_reps, 3] (home wins, draws,
 *     away wins); goal_sums i64[n_reps, 5] (sum x, sum y, sum x^2, sum y^2, sum x y); team_counts
 *     u32[n_reps, n_slots, 4] (goals for, goals against, wins, draws); home_goals and away_goals
 *     u8[n_reps, m] (both or neither; n_reps x m <= BPLHIP_PPC_MAX_SCORE_CELLS).
 * The fixture limit keeps every u32 tally below 2^32 (255 x BPLHIP_PPC_MAX_FIXTURES).  Integer
 * accumulation only: the outputs are bit-identical run to run.  Synchronous. */
#define BPLHIP_PPC_MAX_FIXTURES (1 << 22)
#define BPLHIP_PPC_MAX_TEAMS 1024
#define BPLHIP_PPC_MAX_GOALS 15
#define BPLHIP_PPC_MAX_REPLICATIONS (1 << 20)
#define BPLHIP_PPC_MAX_TEAM_CELLS (1 << 26)
#define BPLHIP_PPC_MAX_SCORE_CELLS (1LL << 30)
int bplhip_ppc(bplhip_ctx* ctx, const bplhip_fixtures* q, const uint16_t* home_slot, const uint16_t* away_slot,
               const uint32_t* fixture_id, int32_t n_slots, int32_t max_goals, int64_t n_reps, uint32_t key_hi,
               uint32_t key_lo, uint32_t* score_counts, uint32_t* outcome_counts, int64_t* goal_sums,
               uint32_t* team_counts, uint8_t* home_goals, uint8_t* away_goals, void* stream);

/* Self-test of the library's own float64 device math (csrc/dc_kernels.hip.h, namespace
 * dc::lean -- the short exp / log / log1p / reciprocal the float64 kernels use on their critical
 * paths; no reference counterpart).  which: 0 exp(x), 1 log(x), 2 log(1 + x) for x >= 0, 3 1/x for
 * normal x.  HOST f64[n] in and out, synchronous. */
int bplhip_selftest_math(bplhip_ctx* ctx, int32_t which, int64_t n, const double* in, double* out);

/* Self-test of the library's cross-lane layer and counted accumulator rows (csrc/wave_reduce.hip.h, the wave
 * helpers, wave_top2* and ga_* of csrc/dc_kernels.hip.h, nd_wave_sum* of csrc/nuts_dev.hip.h; no reference
 * counterpart).  Test-only; HOST arrays, synchronous.
 * which < BPLHIP_SELFTEST_COUNTED_ROWS: n_waves independent waves, each owning BPLHIP_SELFTEST_CHANNELS channels
 * of 64 lanes in each of the three arrays ([n_waves][CHANNELS][64]).  The probe takes its operands from the
 * leading channels of the matching type, calls the library function with all 64 lanes active and writes back
 * what EVERY lane holds afterwards; all other channels are held in registers across the call and come back
 * unchanged.  In the order of `which` from 0 (operands: d = f64, f = f32, i = i32 channels):
 *   wave_sum4_f64 d0..3 | wave_bounds_reduce f0..2 d0..3 | lanes8_max3_sum f0..2 d0..3 | wave_max3_f32 f0..2 |
 *   wave_sum_f64 d0 | wave_sum2_f64 d0..1 | wave_max_f64 d0 | wave_max_f32 f0 |
 *   wr::wave_reduce_max_f64_f32_raw f0 d0 (raw: lane 63 is promised) | wave_max3_f64 d0..2 | row_sum_f64<6> d0..5 |
 *   wave_sum_f32 f0 | wave_sum2_f32 f0..1 | prev_lane_u32 i0 (i1 = fill) | wave_prefix_dpp_f64 d0 |
 *   wave_suffix_dpp_f64 d0 | wave_sumN_f64<2>, <7>, <13> d0.. | block_sum<2>, <5, true>, <6, true> d0.. (512-thread
 *   workgroups: n_waves a multiple of 8) | nd_wave_sum d0 | nd_wave_sum2 d0..1 |
 *   wave_top2<float>, wave_top2<double>, wave_top2_pair_f32: the wave's f32 / f64 channels read flat as a per-team
 *   array (the pair: the two halves of the f32 channels), T in every lane of i0; out m1, m2 in f0, f1 (d0, d1), i1,
 *   i2 in i1, i2, the pair's second array in f2, f3, i3, i4 |
 *   q30 f0 -> d0 | exact_i64 d0 -> d0 (the int64 as bits).
 * which == BPLHIP_SELFTEST_COUNTED_ROWS: n_waves is the number of rows, in_i32[0] the number of contributions
 * (1..255), in_f64[contribution][row] the addends in units of 2^-30.  One workgroup per contribution calls ga_add
 * once per row; a second launch reads every row r into out_f64 as BPLHIP_SELFTEST_GA_WORDS 64-bit words:
 * {lo, hi} of ga_load, ga_value, {lo, hi} x 2 of ga_load2(r, r+1), x 4 of ga_load4(r .. r+3), x 4 of
 * ga_load3(r .. r+2), x 4 of ga_load2rows(r, r+1) (row numbers modulo the row count), and into out_i32[row][4]
 * ga_count and ga_is_zero, then re-arms the rows; a third launch re-reads them: lo | hi in word 31, ga_is_zero
 * and ga_count in out_i32[row][2..3].  in_f32 / out_f32 are not used. */
#define BPLHIP_SELFTEST_CHANNELS 16
#define BPLHIP_SELFTEST_COUNTED_ROWS 29
#define BPLHIP_SELFTEST_GA_WORDS 32
int bplhip_selftest_lanes(bplhip_ctx* ctx, int32_t which, int32_t n_waves, const double* in_f64, const float* in_f32,
                          const int32_t* in_i32, double* out_f64, float* out_f32, int32_t* out_i32);

/* threefry2x32 helpers with jax.random semantics (jax 0.4.24, non-partitionable
 * threefry): used by the Python host for key plumbing (random.split for multi-chain
 * runs, bpl/dixon_coles.py:107).  out has 2*n words: n keys (hi, lo). */
void bplhip_threefry_split(uint32_t key_hi, uint32_t key_lo, int32_t n, uint32_t* out);
/* n raw 32-bit draws, jax.random.bits(key, (n,), uint32). */
void bplhip_threefry_bits(uint32_t key_hi, uint32_t key_lo, int32_t n, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* BPLHIP_H */
