/*
 * tpe_engine.h -- C ABI of the MI355X (gfx950) TPE suggestion engine.
 *
 * Drop-in boundary.  The reference (pminervini/hyperopt, pure Python/numpy)
 * has no FFI of its own; its hot path is a set of pyll `scope` operators
 * evaluated per hyperparameter inside `tpe.suggest`.  Each entry point below
 * replaces one of those operators (operator level, host buffers, synchronous)
 * or the whole evaluation of the posterior graph (plan level, device
 * resident).  The Python binding is hyperopt_amd/_engine.py (ctypes); see
 * INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions: all functions return TPE_OK (0) or a negative TPE_E_* code;
 * tpe_last_error() gives the message.  No exception or abort crosses the ABI.
 * Inputs are never mutated.  One handle must be used by one thread at a
 * time; distinct handles are independent (no global mutable state).
 */
#ifndef TPE_ENGINE_H
#define TPE_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPE_ENGINE_ABI_VERSION 1

/* Candidate-range alignment of bit-identical sharding: tpe_plan_suggest over
 * [0, n) and over any split of [0, n) into ranges whose boundaries are
 * multiples of TPE_SHARD_ALIGN (merged with tpe_plan_merge) give the same
 * results byte for byte, as long as every part takes the same draw path (the
 * large-draw value-bucketed path runs at >= 2^22 draws per call).  Large
 * draws are value-bucketed in blocks of this many consecutive global
 * candidate indices (of 4096 for suggestions of <= 2^18 candidates, whose
 * block boundaries are among these), and a candidate's pruned log-sum-exp
 * depends on its block.  Unaligned splits still agree under the north-star tie rule. */
#define TPE_SHARD_ALIGN 8192

/* ---- status codes ---------------------------------------------------- */
#define TPE_OK 0
#define TPE_E_INVALID (-1)   /* bad argument / shape  -> TypeError/ValueError     */
#define TPE_E_BOUNDS (-2)    /* low >= high           (tpe.py:80-81, 237-238)     */
#define TPE_E_NEGATIVE (-3)  /* negative lognormal_cdf argument (tpe.py:181-182) */
#define TPE_E_NOMEM (-4)     /* device allocation failed                         */
#define TPE_E_HIP (-5)       /* HIP runtime error                                */
#define TPE_E_NODEVICE (-6)  /* no gfx950 device                                 */
#define TPE_E_INDEX (-7)     /* categorical sample out of range (IndexError)     */

/* ---- posterior families ---------------------------------------------- */
#define TPE_GMM 0  /* GMM1 / GMM1_lpdf          hyperopt/tpe.py:62-166  */
#define TPE_LGMM 1 /* LGMM1 / LGMM1_lpdf        hyperopt/tpe.py:216-301 */
#define TPE_CAT 2  /* categorical / _lpdf       hyperopt/tpe.py:50-57, 573-607 */

/* ---- flags (which optional lpdf / sampler arguments are not None) ----- */
#define TPE_HAS_LOW 1u
#define TPE_HAS_HIGH 2u
#define TPE_HAS_Q 4u
#define TPE_PCHOICE 8u /* categorical with a prior p (hp.pchoice) */

/* ---- observation transform applied before the Parzen fit --------------
 * hyperopt/tpe.py:485-568 (ap_*_sampler).                                  */
#define TPE_OBS_IDENT 0          /* uniform, quniform, normal, qnormal        */
#define TPE_OBS_LOG 1            /* loguniform, lognormal: log(obs)           */
#define TPE_OBS_LOG_CLIP_EXPLOW 2/* qloguniform: log(max(obs, max(EPS, e^low))) */
#define TPE_OBS_LOG_CLIP_EPS 3   /* qlognormal: log(max(obs, EPS))            */

typedef struct tpe_engine *tpe_handle_t;
typedef struct tpe_plan *tpe_plan_t;

/* One hyperparameter of a compiled search space (descriptor
 * table).  For TPE_LGMM, low/high are the log-space bounds exactly as the
 * reference passes them to LGMM1/LGMM1_lpdf. */
typedef struct {
  int32_t family;        /* TPE_GMM / TPE_LGMM / TPE_CAT                  */
  uint32_t flags;        /* TPE_HAS_* / TPE_PCHOICE                       */
  int32_t obs_transform; /* TPE_OBS_*                                     */
  int32_t upper;         /* categorical: number of categories             */
  double prior_mu;       /* Parzen prior (continuous families)            */
  double prior_sigma;
  double low, high, q;   /* sampler / lpdf arguments (valid per flags)    */
  int32_t cond_begin;    /* activity: OR over [cond_begin, +cond_count) of */
  int32_t cond_count;    /*   (parent active && parent value == branch)    */
  int64_t pprior_begin;  /* TPE_PCHOICE: upper probabilities in pprior[]   */
} tpe_hp;

typedef struct {
  int32_t n_hp;
  const tpe_hp *hp;
  int32_t n_cond;
  const int32_t *cond_parent; /* hp index of the controlling choice   */
  const int32_t *cond_branch; /* option index that activates the hp   */
  int64_t n_pprior;
  const double *pprior;
} tpe_space;

/* Per (suggestion, hp) outcome of broadcast_best (tpe.py:749-759). */
typedef struct {
  double score;  /* below_llik - above_llik of the winner (NaN allowed)   */
  double value;  /* the winning candidate                                 */
  int64_t index; /* its global candidate index (-1: hp inactive)          */
  int32_t active;/* 1 if the hp is active in this suggestion              */
  int32_t pad;
} tpe_result;

/* ---- engine ------------------------------------------------------------ */
const char *tpe_version(void);
int tpe_device_count(int32_t *n);
int tpe_create(int32_t device, tpe_handle_t *out);
int tpe_destroy(tpe_handle_t h);
const char *tpe_last_error(tpe_handle_t h);
int tpe_synchronize(tpe_handle_t h);

/* ---- operator level: host buffers, synchronous -------------------------
 * Each mirrors one pyll scope operator of the reference.                   */

/* ap_filter_trials loss ranking (tpe.py:613-641): marks the n_below lowest
 * losses (ties: lowest position first) with 1 in below_mask[n].           */
int tpe_split(tpe_handle_t h, const double *losses, int64_t n, double gamma,
              int32_t gamma_cap, uint8_t *below_mask);

/* adaptive_parzen_normal (tpe.py:398-475): K = n + 1 outputs.             */
int tpe_parzen_fit(tpe_handle_t h, const double *obs, int64_t n,
                   double prior_weight, double prior_mu, double prior_sigma,
                   int32_t lf, double *w, double *mu, double *sigma);

/* categorical posterior (tpe.py:573-607): p[upper].  pprior may be NULL.  */
int tpe_categorical_posterior(tpe_handle_t h, const int64_t *obs, int64_t n,
                              int32_t upper, double prior_weight,
                              const double *pprior, int32_t lf, double *p);

/* GMM1_lpdf / LGMM1_lpdf (tpe.py:104-166, 259-301) of one mixture.  For
 * TPE_CAT, w holds p (k = upper) and mu/sigma are ignored.                */
int tpe_lpdf(tpe_handle_t h, int32_t family, const double *x, int64_t n,
             const double *w, const double *mu, const double *sigma, int64_t k,
             double low, double high, double q, uint32_t flags, double *out);

/* Fused below/above lpdf + broadcast_best argmax (tpe.py:684-698, 749-759).
 * llik_b / llik_a may be NULL (argmax only).                               */
int tpe_score(tpe_handle_t h, int32_t family, const double *x, int64_t n,
              const double *wb, const double *mb, const double *sb, int64_t kb,
              const double *wa, const double *ma, const double *sa, int64_t ka,
              double low, double high, double q, uint32_t flags,
              double *llik_b, double *llik_a, int64_t *best_index,
              double *best_score);

/* GMM1 / LGMM1 / categorical candidate draws (tpe.py:62-93, 216-250,
 * pyll/stochastic.py:104-142) with counter-based Philox4x32-10: draw i uses
 * counter (offset + i, stream), key seed, so any sharding of [0, n) yields
 * the same values.                                                        */
int tpe_sample(tpe_handle_t h, int32_t family, const double *w,
               const double *mu, const double *sigma, int64_t k, double low,
               double high, double q, uint32_t flags, uint64_t seed,
               uint64_t stream, int64_t offset, int64_t n, double *out);

/* ---- plan level: whole tpe.suggest posterior evaluation on device -------
 * A plan holds one compiled space and a device-resident trial history.     */
int tpe_plan_create(tpe_handle_t h, const tpe_space *space, int64_t max_trials,
                    tpe_plan_t *out);
int tpe_plan_destroy(tpe_plan_t p);
int tpe_plan_num_levels(tpe_plan_t p, int32_t *n_levels);

/* History in tid order (tpe.py:820-848): losses[n] (+inf for unfinished),
 * vals[n_hp][n], active[n_hp][n].  on_device != 0: pointers are device
 * memory (e.g. torch tensors); stream: hipStream_t or NULL (the engine's).
 * History updates are stream-ordered, not synchronous: the host buffers may
 * be reused on return, but the device rows change in `stream`'s order, so a
 * fit / suggest on another stream must be ordered after it by the caller
 * (the same stream, or an event).  The same holds for every plan call. */
int tpe_plan_set_history(tpe_plan_t p, const double *losses,
                         const double *vals, const uint8_t *active, int64_t n,
                         int32_t on_device, void *stream);

/* Incremental history update (the columnar trial store appends rows): copy
 * rows [row0, row0 + n_rows) of every hp from vals / active (source layout
 * [n_hp][src_ld]: row r of hp i at vals[i * src_ld + (r - row0)]) and
 * losses [loss0, n) from losses[0 .. n - loss0); the history length becomes
 * n.  Rows outside [row0, row0 + n_rows) keep their device contents.
 * tpe_plan_set_history(n) == update_history(n, 0, n, vals, active, n, 0,
 * losses).  Replaces the per-call re-walk of hyperopt/tpe.py:820-848.      */
int tpe_plan_update_history(tpe_plan_t p, int64_t n, int64_t row0, int64_t n_rows,
                            const double *vals, const uint8_t *active, int64_t src_ld,
                            int64_t loss0, const double *losses, int32_t on_device,
                            void *stream);

/* split + Parzen fit of every hp, both sides (tpe.py:613-641, 398-607).    */
int tpe_plan_fit(tpe_plan_t p, double gamma, int32_t gamma_cap,
                 double prior_weight, int32_t lf, void *stream);

/* Below-side mixture of one hp after tpe_plan_fit (host copy; k = K).     */
int tpe_plan_get_mixture(tpe_plan_t p, int32_t hp, int32_t side, double *w,
                         double *mu, double *sigma, int64_t cap, int64_t *k);

/* Diagnostics / table parity tests: the raw scoring table of slot (hp,
 * side) as written by the last fit -- which 0: the per-component coefficient
 * table (32 B per component, field-major blocks of 8, envelopes in the
 * w-rows), 1: the block-local fp32 table (128 B per block of 8), 2: the
 * moment table of 16-component chunks (64 B each), 3: the 8-wide moment
 * table (128 B per block of 8; written instead of 2 for mixtures of ~1e3
 * components, the other one is then stale), 4: the degree-15 copy of 2's
 * chunks (128 B each, 3's layout; read where a wave's window is too wide
 * for degree 9).  *bytes = the table's
 * size; out may be NULL (size query).  The layouts are internal
 * (tpe_internal.hpp) and may change between versions.                      */
int tpe_plan_get_table(tpe_plan_t p, int32_t hp, int32_t side, int32_t which, void *out,
                       int64_t cap_bytes, int64_t *bytes);

/* Sample + score + argmax for n_suggest suggestions (seeds[s]) on the
 * candidate range [cand_begin, cand_begin + n_cand) of each suggestion, for
 * the hps of one level (level < 0: all levels, single device).  Results for
 * [n_suggest][n_hp] are kept in the plan; out (host or device, may be NULL)
 * receives a copy.                                                         */
int tpe_plan_suggest(tpe_plan_t p, const uint64_t *seeds, int64_t n_suggest,
                     int64_t n_cand, int64_t cand_begin, int32_t level,
                     tpe_result *out, int32_t out_on_device, void *stream);
/* The same for a shard of a larger suggestion: the candidates [cand_begin,
 * cand_begin + n_cand) of an n_total-candidate suggestion (n_total >=
 * cand_begin + n_cand).  n_total picks the scoring tiles (one-row wave tiles
 * up to 2^18 candidates), so the shards of one suggestion score every
 * candidate exactly as the unsharded call does (parallel.ShardedSuggest);
 * tpe_plan_suggest is this with n_total = cand_begin + n_cand.             */
int tpe_plan_suggest_shard(tpe_plan_t p, const uint64_t *seeds, int64_t n_sug, int64_t n_total,
                           int64_t cand_begin, int64_t n_cand, int32_t level, tpe_result *out,
                           int32_t out_on_device, void *stream);

/* tpe_plan_fit + tpe_plan_suggest (all levels, cand_begin 0) in one call:
 * the tpe.suggest posterior evaluation for one history.  Repeated calls of
 * one shape (prior_weight, lf, n_suggest <= 8, n_candidates, stream) may
 * replay a captured hipGraph of the whole step, patched with this call's
 * history length and seeds (opt-in: TPE_GRAPH=1 in the environment; the
 * default enqueues the step's kernels back to back).                      */
int tpe_plan_fit_suggest(tpe_plan_t p, double gamma, int32_t gamma_cap,
                         double prior_weight, int32_t lf, const uint64_t *seeds,
                         int64_t n_suggest, int64_t n_cand, tpe_result *out,
                         int32_t out_on_device, void *stream);

/* Results [n_suggest][n_hp] of the last tpe_plan_suggest (copy), and the
 * device address where the plan keeps them (valid until the next call).   */
int tpe_plan_get_results(tpe_plan_t p, tpe_result *out, int32_t out_on_device,
                         void *stream);
const tpe_result *tpe_plan_results_device(tpe_plan_t p);

/* Multi-device: combine world copies of one level's results ([world][S][P],
 * device memory, e.g. an RCCL all-gather) with numpy argmax semantics and
 * make them the plan's state.  out_on_device 2: `out` is a device buffer
 * that already holds the records the level's tpe_plan_suggest_shard copied
 * out (out_on_device 1); only the level's merged slots are stored into it,
 * by the merge kernel itself (no copy launch after the merge).             */
int tpe_plan_merge(tpe_plan_t p, const tpe_result *gathered, int32_t world,
                   int32_t level, tpe_result *out, int32_t out_on_device,
                   void *stream);

/* Score given candidates of one hp with the plan's fitted mixtures
 * (parity path for reference-sampled candidates).                          */
int tpe_plan_score_candidates(tpe_plan_t p, int32_t hp, const double *x,
                              int64_t n, double *llik_b, double *llik_a,
                              int64_t *best_index, double *best_score);

/* The same, through the production scoring form of large draws: the given
 * candidates are value-bucketed in blocks of TPE_SHARD_ALIGN exactly as
 * k_draw_sorted buckets its draws, then scored on the same tiles with
 * log-sum-exp prune mode `mode` (tpe_plan_set_prune: 0 every pair, 1 block
 * skip, 2 block skip + one exponent per wave, 3 the same in block-local
 * fp32; 4: mode 3's tiles scored from the hp's certified Chebyshev tables of
 * both mixtures alone, as suggestions of more than 2^18 candidates score a
 * bounded continuous hp -- TPE_E_INVALID when the hp takes no table or a
 * side's table is not certified).  Outputs are in the given
 * order.  The parity path of tpe.py:139-144 / 253-256 as the suggest
 * computes it at config 4.                                                 */
int tpe_plan_score_candidates_sorted(tpe_plan_t p, int32_t hp, int32_t mode,
                                     const double *x, int64_t n, double *llik_b,
                                     double *llik_a, int64_t *best_index,
                                     double *best_score);

/* EI of M whole configurations under the last tpe_plan_fit: vals[n_hp][ld]
 * (the history's layout).  total[M]; terms[n_hp][ld] and active[n_hp][ld]
 * may be NULL.  on_device != 0: all pointers are device memory and the call
 * is stream-ordered like every plan call; else host buffers, synchronous.
 * A configuration's active set follows the space's condition tables from its
 * own values (an hp is active iff it has no condition, or some condition's
 * parent is active with value == branch); values of inactive hps are ignored.
 * terms[i][c] = below_llik - above_llik of hp i at its value (the score
 * broadcast_best ranks, tpe.py:749-759), +0.0 where inactive; total[c] = the
 * terms of c added in ascending hp index.  Non-finite lpdfs propagate as IEEE
 * arithmetic does; an active categorical value that is not an integer in
 * [0, upper) gives a NaN term and total and activates no child.
 * TPE_E_INVALID: m < 0, ld < m, null vals / total with m > 0, or a plan that
 * has not been fitted; m == 0 touches nothing.  The results of the last
 * suggest and the history are not disturbed.                               */
int tpe_plan_score_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                          double *total, double *terms, uint8_t *active,
                          int32_t on_device, void *stream);

/* Draw m whole configurations from the below mixtures of the last
 * tpe_plan_fit and score them: vals[n_hp][ld], total[m], and optional
 * terms[n_hp][ld] / active[n_hp][ld], laid out as tpe_plan_score_points lays
 * them out (entries m..ld of a row are not touched).  Configuration j has
 * index c = begin + j.  The hps are visited parents first; an hp is active iff
 * it has no condition, or some condition's parent is active with a drawn value
 * equal to the branch.  An active hp takes, bit for bit, the value tpe_sample
 * returns for its below mixture with Philox key `seed`, stream = the hp's
 * index and offset c; an inactive one is NaN, so vals is a pool array for
 * tpe_plan_score_points.  total, terms and active are what
 * tpe_plan_score_points returns for the drawn vals, bit for bit.  The draws
 * depend on (seed, hp, c) only: any split of [begin, begin + m) into calls
 * gives the same numbers.  on_device != 0: device pointers, stream-ordered, no
 * host synchronisation; else host buffers, synchronous.  TPE_E_INVALID: m < 0,
 * ld < m, begin < 0, null vals / total with m > 0, or a plan that has not
 * been fitted; m == 0 touches nothing.  The history, a pending history update
 * and the results of the last suggest are not disturbed.                    */
int tpe_plan_sample_points(tpe_plan_t p, uint64_t seed, int64_t begin, int64_t m,
                           int64_t ld, double *vals, double *total, double *terms,
                           uint8_t *active, int32_t on_device, void *stream);

/* idx[0..k): the k eligible entries of total[m] that rank first -- highest
 * total first, ties to the lower index (-0.0 == +0.0), +inf above and -inf
 * below every finite total, NaN last (NaN entries by index).  eligible[m]
 * (bytes, non-zero = eligible) may be NULL: every entry.  1 <= k <= 4096,
 * m <= 2^31 - 1.  The selection is a radix select on integer keys: the same
 * result for every launch shape, no floating-point atomics.  TPE_E_INVALID:
 * k or m out of range, null total / idx, or fewer than k eligible entries
 * (with a mask the call waits for the device's count of them, in device mode
 * too).  on_device as above.                                                */
int tpe_plan_topk_points(tpe_plan_t p, const double *total, const uint8_t *eligible,
                         int64_t m, int32_t k, int32_t *idx, int32_t on_device,
                         void *stream);

/* out[n_hp][k] = the columns idx[0..k) of vals[n_hp][ld].  on_device as above;
 * host mode fails with TPE_E_INDEX on an index outside [0, ld), device mode
 * writes NaN for it.  k == 0 touches nothing.                               */
int tpe_plan_gather_points(tpe_plan_t p, const double *vals, int64_t ld,
                           const int32_t *idx, int32_t k, double *out,
                           int32_t on_device, void *stream);

/* Multivariate TPE: a joint Parzen model over the root hps -- those without a
 * condition, in ascending index; they must be active in every history row
 * (not checked).  The sides are the split of the last tpe_plan_fit, each kept
 * in row order.  Side s with n_s rows has n_s + 1 components: component 0 is
 * the prior, component k >= 1 the side's k-th row, with weight w_0 =
 * prior_weight / (S + prior_weight), w_k = lw[k - 1] / (S + prior_weight), lw
 * the linear-forgetting weights of the side's rows (ones unless lf < n_s) and
 * S their sum.  A component's density is the product over the root hps of a
 * kernel: for a continuous hp the (mu, sigma) the marginal fit of that hp
 * gave the row's observation (the prior's for component 0), as the q = None
 * log-density or, with q, log(cdf(ub) - cdf(lb)) on the reference's bounds,
 * without truncation normaliser; for a categorical hp with observation o,
 * kappa(c) = ((c == o ? 1 : 0) + a pi[c]) / (1 + a), a = prior_weight
 * (upper - 1) / (S + prior_weight), pi the prior over the options (component
 * 0: pi itself).  J_s(c) = logsumexp_k [log w_k + sum_d log kappa_dk(c_d)],
 * joint(c) = J_below(c) - J_above(c).
 * tpe_plan_joint_fit builds the model's tables from the last tpe_plan_fit
 * (TPE_E_INVALID before one); a later fit invalidates them.  Stream-ordered. */
int tpe_plan_joint_fit(tpe_plan_t p, void *stream);
/* The joint model's components of a root hp in component order, k of them
 * (cap >= k): w, mu, sigma are the entries of the hp's marginal mixture
 * (tpe_plan_get_mixture) that row rows[j] owns, bit for bit -- sorted by (mu,
 * row) they are that mixture -- and rows[0] = -1 (the prior).  A categorical
 * hp: w = the component weight, mu = the observed option (-1 for component
 * 0), sigma = a.  hp = -1: the component weights themselves in w (the draw's
 * pick distribution); mu and sigma are not written.  Any output may be NULL.
 * TPE_E_INVALID for a conditional hp or without a joint fit.  Synchronizes
 * the device.                                                               */
int tpe_plan_joint_get_mixture(tpe_plan_t p, int32_t hp, int32_t side, double *w,
                               double *mu, double *sigma, int32_t *rows, int64_t cap,
                               int64_t *k);
/* tpe_plan_score_points under the joint model: joint[M] (may be NULL) as
 * above from the root values; terms[i][c] of a conditional hp is what
 * tpe_plan_score_points returns, of a root hp +0.0; total[c] = joint[c] plus
 * the terms in ascending hp index, added in float64 in that order.  Activity,
 * layouts, on_device, the NULL outputs, m == 0 and the errors are
 * tpe_plan_score_points'; a root value that is NaN, or a root choice that is
 * not an integer in [0, upper), gives NaN joint and total and activates no
 * child.  A configuration's numbers depend on its own values and the fit
 * alone.  TPE_E_INVALID without a joint fit.                                */
int tpe_plan_joint_score_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                                double *total, double *joint, double *terms,
                                uint8_t *active, int32_t on_device, void *stream);
/* Debug: J_below and J_above (either may be NULL) of the first m
 * configurations of the plan's last tpe_plan_joint_score_points or
 * tpe_plan_joint_sample_points call.  Synchronizes the device.              */
int tpe_plan_joint_sides(tpe_plan_t p, double *below, double *above, int64_t m);
/* tpe_plan_sample_points under the joint model.  Configuration c = begin + j
 * picks one below component, comp[j] (may be NULL) = tpe_sample(TPE_CAT, the
 * below component weights, stream 2^29 | n_hp, offset c).  A continuous root
 * hp d takes, bit for bit, tpe_sample of the one-component mixture (1.0,
 * mu_d,comp, sigma_d,comp) with the hp's family, bounds, q and flags, stream
 * 2^29 | d, offset c; a categorical one tpe_sample(TPE_CAT, kappa_d,comp,
 * stream 2^29 | d, offset c).  Conditional hps are drawn and routed as
 * tpe_plan_sample_points draws them.  total, joint, terms and active are what
 * tpe_plan_joint_score_points returns for the drawn vals, bit for bit.  The
 * draws depend on (seed, c) only.  TPE_E_INVALID as tpe_plan_sample_points,
 * without a joint fit, or with more than 2048 below components or options of
 * a root choice.                                                            */
int tpe_plan_joint_sample_points(tpe_plan_t p, uint64_t seed, int64_t begin, int64_t m,
                                 int64_t ld, double *vals, int32_t *comp, double *total,
                                 double *joint, double *terms, uint8_t *active,
                                 int32_t on_device, void *stream);

/* Multivariate TPE over conditional spaces: one joint Parzen model per group
 * of hps that are always active together.  A group is a maximal set of hps
 * with the same set of immediate (parent, branch) condition alternatives;
 * group 0 holds the hps without a condition, the other groups follow in
 * ascending order of their smallest hp index, and inside a group the hps keep
 * ascending index.  tpe_plan_group_info writes each hp's group and the number
 * of groups G (either output may be NULL; needs no fit).
 * Group g's side s holds the rows of the last tpe_plan_fit's split side in
 * which the group is active (the activity column of its hps, which must agree:
 * not checked; group 0 takes every row, as the root model does), in row order, n_gs of them, and K_gs = n_gs + 1 components:
 * component 0 the prior, component k that side's k-th such row, w_0 =
 * prior_weight / (S + prior_weight), w_k = lw[k - 1] / (S + prior_weight) with
 * lw the linear-forgetting weights over the n_gs rows (ones unless lf < n_gs)
 * and S their sum; an empty side is the prior alone.  Per hp of the group the
 * component's kernel is the root model's above: for a continuous hp the
 * (mu, sigma) its marginal fit gave the row's observation, for a categorical
 * hp kappa with a = prior_weight (upper - 1) / (S + prior_weight) on the
 * group's own S; no truncation normaliser.
 * J_gs(c) = logsumexp_k [log w_k + sum_{d in g} log kappa_dk(c_d)],
 * joint_g(c) = J_g,below(c) - J_g,above(c), and EI(c) = the float64 sum, in
 * ascending group order from +0.0, of joint_g(c) over the groups active in c
 * (an inactive group adds +0.0).  A group is active in c when one of its
 * (parent, branch) alternatives holds with the parent active; group 0 always.
 * The root model of tpe_plan_joint_* is group 0 of this one, bit for bit.
 * tpe_plan_group_fit builds every group's tables from the last tpe_plan_fit
 * (TPE_E_INVALID before one, or for a space without an unconditional hp); a
 * later fit invalidates them.  Stream-ordered.                              */
int tpe_plan_group_info(tpe_plan_t p, int32_t *group_of_hp, int32_t *n_groups);
int tpe_plan_group_fit(tpe_plan_t p, void *stream);
/* tpe_plan_joint_get_mixture for hp `hp` of group `group`: its k = K_gs
 * components in component order, rows[0] = -1; w, mu, sigma are the entries of
 * the hp's marginal mixture that row owns, bit for bit (categorical: w = the
 * component weight, mu = the observed option, sigma = a).  hp = -1: the
 * group's component weights in w.  TPE_E_INVALID for an hp of another group
 * or without a group fit.  Synchronizes the device.                          */
int tpe_plan_group_get_mixture(tpe_plan_t p, int32_t group, int32_t hp, int32_t side,
                               double *w, double *mu, double *sigma, int32_t *rows,
                               int64_t cap, int64_t *k);
/* EI of m whole configurations under the group models: total[m], and optional
 * joint[G][ld] (joint_g per configuration, +0.0 where the group is inactive)
 * and active[n_hp][ld].  Layouts, on_device, the NULL outputs, m == 0 and the
 * errors are tpe_plan_joint_score_points'; there are no per-hp terms.  A NaN
 * value, or a choice that is not an integer in [0, upper), inside an active
 * group gives NaN joint_g and total and activates no child.  A
 * configuration's numbers depend on its own values and the fit alone.
 * TPE_E_INVALID without a group fit.                                        */
int tpe_plan_group_score_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                                double *total, double *joint, uint8_t *active,
                                int32_t on_device, void *stream);
/* Debug: J_g,below and J_g,above (either may be NULL) of group `group` for the
 * first m configurations of the plan's last tpe_plan_group_score_points or
 * tpe_plan_group_sample_points call, NaN where the group was inactive.
 * TPE_E_INVALID without a group fit (a later tpe_plan_fit drops the sides) or
 * for more entries than that call held.  Synchronizes the device.           */
int tpe_plan_group_sides(tpe_plan_t p, int32_t group, double *below, double *above,
                         int64_t m);
/* tpe_plan_sample_points under the group models.  The hps are visited parents
 * first.  Where configuration c = begin + j activates group g, comp[g][j]
 * (comp[G][ld], may be NULL) = tpe_sample(TPE_CAT, the group's below component
 * weights, stream 2^29 | (n_hp + g), offset c), and every hp d of the group
 * draws from that component as tpe_plan_joint_sample_points draws a root: a
 * continuous hp tpe_sample of the one-component mixture (1.0, mu_d,comp,
 * sigma_d,comp), a categorical one tpe_sample(TPE_CAT, kappa_d,comp), stream
 * 2^29 | d, offset c.  Where the group is inactive its hps are NaN and comp is
 * -1.  total, joint and active are what tpe_plan_group_score_points returns
 * for the drawn vals, bit for bit.  The draws depend on (seed, c) only.
 * TPE_E_INVALID as tpe_plan_sample_points, without a group fit, or with more
 * than 2048 below components of a group or options of a choice.             */
int tpe_plan_group_sample_points(tpe_plan_t p, uint64_t seed, int64_t begin, int64_t m,
                                 int64_t ld, double *vals, int32_t *comp, double *total,
                                 double *joint, uint8_t *active, int32_t on_device,
                                 void *stream);

/* A batch for parallel workers: k greedy picks with a pending-trial penalty
 * (the constant liar inside one call).  The input is the m configurations
 * vals[n_hp][ld] of the plan's last tpe_plan_group_score_points or
 * tpe_plan_group_sample_points call -- the same values, the same m -- whose
 * per-group sides J_g,below(c), J_g,above(c) the plan still holds.
 * With W_g = S_g,above + prior_weight (the unnormalised mass of group g's
 * above side) and Ja_g^(0) = J_g,above, round t = 0..k-1 scores every
 * configuration, score_t(c) = the float64 sum, in ascending group order from
 * +0.0, of J_g,below(c) - Ja_g^(t)(c) over the groups active in c (score_0 is
 * the call's total, bit for bit), and picks the first selectable
 * configuration in tpe_plan_topk_points' order (highest score, ties to the
 * lower index, -0.0 == +0.0, NaN last) with one tier above it: a
 * configuration is selectable when eligible[c] != 0 (NULL: all) and it has
 * not been taken; it is a duplicate when its activity and active values equal
 * a taken one's (the sign of zero ignored), and every non-duplicate ranks
 * above every duplicate.  After a pick p every group g active in p gets one
 * pending component of unnormalised weight 1 (the linear-forgetting weight of
 * a newest row): for each c with g active
 *   Ja_g^(t+1)(c) = logaddexp(Ja_g^(t)(c) + log(W_g + n_g),
 *                             sum_{d in g} log kappa_d(c_d; p_d))
 *                   - log(W_g + n_g + 1),
 * n_g the earlier picks that activated g; groups inactive in p or in c keep
 * their value.  kappa_d is the kernel a refit would give the pick's value
 * appended to hp d's above observations with every fitted component frozen.
 * Continuous hp: mu = the transformed value; in the hp's sorted above mixture
 * (tpe_plan_get_mixture, side 1, K components with the prior) the left
 * neighbour is the last mu_k <= mu and the right one the first mu_k > mu
 * (fitted components only, never earlier picks), sigma = the larger of the
 * two gaps (one-sided at an end) clipped to [prior_sigma / min(100, 2 + K),
 * prior_sigma], and prior_sigma / 2 when the prior is alone; the log kernel is
 * the group model's form (the q = None log-density, or log(cdf(ub) - cdf(lb))
 * with q; no truncation normaliser).  Categorical hp with picked option o:
 * kappa(c) = ((c == o) + a pi[c]) / (1 + a) with the above side's a.
 * idx[k]: the picks; gain[k] (may be NULL): gain[t] = score_t(idx[t]);
 * trace[k][ld] (may be NULL, for tests): trace[t][c] = score_t(c) for every
 * configuration, selectable or not.  1 <= k <= 1024, m <= 2^31 - 1.
 * TPE_E_INVALID: no group fit, an m other than the last group score's or
 * draw's since that fit, k or m out of range, ld < m, null vals / idx, or
 * fewer than k selectable configurations -- a short batch, found after the
 * rounds: idx[t] = -1 from the first round without one.  on_device as above,
 * except that the call ends with one 4-byte read-back for the short batch.
 * The history, the fit, the sides and the last suggest's results are not
 * disturbed.  The same picks for every launch shape: all comparisons are on
 * integers, there is no floating-point atomic.                             */
int tpe_plan_group_batch_points(tpe_plan_t p, const double *vals, int64_t m, int64_t ld,
                                const uint8_t *eligible, int32_t k, int32_t *idx,
                                double *gain, double *trace, int32_t on_device,
                                void *stream);

/* ---- multi-objective TPE: the history ranked by Pareto dominance ----------
 * (DESIGN 5.17).  Every objective is minimised.  A row is complete when none
 * of its n_obj objectives is NaN or +inf, pending otherwise.  For complete
 * rows, j dominates i when y_j[m] <= y_i[m] for every m and y_j[m] < y_i[m]
 * for some m (IEEE comparison: -0.0 == +0.0, -inf an ordinary value).
 *   dominated_by[i] = #{complete j : j dominates i}   (0: nondominated)
 *   dominates[i]    = #{complete j : i dominates j}
 *   s[i] = dominated_by[i] (n + 1) + (n - dominates[i]),  +inf if i is pending
 * (counts 0 / 0 for a pending row).  s is an exact integer; a dominates b
 * implies s[a] < s[b]; with one objective and distinct losses s sorts as the
 * loss does.
 *
 * tpe_plan_set_objectives copies rows [obj0, n) of every objective from Y
 * (row r of objective m at Y[m * ld + (r - obj0)]) into the plan's objective
 * matrix (allocated by the first call, at the plan's trial capacity; rows
 * below obj0 are those of the last call, which must have had the same n_obj
 * and at least obj0 rows), counts over all rows [0, n) and overwrites the loss
 * column of rows [0, n) with s: the fits, the joint and group models, the
 * batch and the draws then rank the history by Pareto dominance with no other
 * change.  n must be the plan's history length.  Stream-ordered like every
 * plan call; a deferred tpe_plan_update_history is written first, so none of
 * its losses can land on s -- a later history update that carries losses
 * overwrites s in its turn.  The fit, the joint fit and the group fit are
 * invalidated.  The counts use integer atomics only: they depend on Y alone,
 * not on the launch shape.  TPE_E_INVALID: n_obj outside [1, TPE_MAX_OBJ], n
 * other than the history length, (n + 1)^2 >= 2^53, obj0 outside [0, n] or
 * above the rows held, ld < n - obj0, or a null Y.  An empty history (n = 0)
 * is accepted and ranks nothing.                                            */
#define TPE_MAX_OBJ 8
int tpe_plan_set_objectives(tpe_plan_t p, const double *Y, int32_t n_obj, int64_t n,
                            int64_t ld, int64_t obj0, int32_t on_device, void *stream);

/* Host copies of the last tpe_plan_set_objectives' results: dominated_by[n],
 * dominates[n] and the loss column s[n] as the device holds it now (each may
 * be NULL).  n must be that call's.  Waits for the device.                   */
int tpe_plan_pareto_get(tpe_plan_t p, int32_t *dominated_by, int32_t *dominates,
                        double *loss, int64_t n);

/* The launch the ranking takes for n rows of n_obj objectives, and a test
 * hook: out[0] = rows per tile, out[1] = TPE_MAX_OBJ, out[2] = the j-splits
 * (blocks that share a tile of rows i and split the rows j), out[3] = the
 * tiles.  force_splits > 0: plan with that many j-splits, in this call and in
 * this plan's later tpe_plan_set_objectives calls (at most one per tile; the
 * plan rounds to a count without an empty split); 0: back to the default;
 * < 0: leave the plan's setting.  TPE_E_INVALID when (n, n_obj) is out of
 * range.                                                                     */
int tpe_plan_pareto_shape(tpe_plan_t p, int64_t n, int32_t n_obj, int64_t force_splits,
                          int64_t *out);

/* ---- hypervolume subset selection inside the Pareto front ----
 * Off by default.  With mode 1 the next tpe_plan_set_objectives (and every
 * later one, until mode 0) orders the nondominated rows by a greedy
 * hypervolume subset selection against the reference point ref[n_obj] after
 * the counts, and writes the loss column from it.  A row takes part when it is
 * complete, has dominated_by = 0, is finite in every objective and has
 * w[m] = ref[m] - y[m] > 0 for every m; vol = w[0] * ... * w[n_obj - 1].  In
 * round t = 0 .. n_pick - 1 the row of largest key is pick t (ties to the
 * lower row); a key that is not > 0 ends the selection with R = t picks.
 *   exact (two objectives): key = (right - y[0]) * (top - y[1]), right the
 *     smallest y_p[0] > y[0] over the picks p (ref[0] without one), top the
 *     same in objective 1; 0 once a pick equals the row in both objectives.
 *   Monte-Carlo: key = vol * alive, alive the number of the row's n_samples
 *     samples z[m] = y[m] + u[s][m] * w[m] with no pick p below them
 *     (y_p[m] <= z[m] for every m); u[s][m] is uniform m % 4 of the Philox
 *     draw (seed, counter s, stream 0x60000000, block pair m / 4), the same
 *     table for every row.  No division by n_samples.
 * Picked rows and rows with a zero count have key 0.  The loss column becomes
 *   s[i] = dominated_by[i] (n + 1) + sec[i]
 * with sec = t for pick t, max(R, n - dominates[i]) for every other row with
 * dominated_by = 0, n - dominates[i] elsewhere; +inf for a pending row.  sec
 * stays in [0, n]: a dominates b still implies s[a] < s[b].  Every value is a
 * function of (Y, ref, n_pick, n_samples, seed, method) alone: products and
 * differences as written, no fused multiply-add, keys compared as integers.
 * method: 0 exact with two objectives and Monte-Carlo with more, 1 exact,
 * 2 Monte-Carlo.  With n_obj = 1 the setting is accepted and ignored (the
 * ranking is total).  TPE_E_INVALID: a mode other than 0 / 1, a null or
 * non-finite ref, n_obj outside [1, TPE_MAX_OBJ], n_pick outside [1, 256],
 * n_samples not a multiple of 64 in [64, 4096], an unknown method, method 1
 * with n_obj != 2; a tpe_plan_set_objectives with another n_obj fails with
 * TPE_E_INVALID while the mode is on.  Mode 0 ignores the other arguments,
 * adds no launch and allocates nothing.                                      */
int tpe_plan_set_hv(tpe_plan_t p, int32_t mode, const double *ref, int32_t n_obj,
                    int32_t n_pick, int32_t n_samples, uint64_t seed, int32_t method);

/* Host copies of the last ranking's selection: the first min(cap, n_pick)
 * entries of picks (row indices in pick order, -1 from round R on), keys (the
 * key of each pick; 0 from round R on) and counts (the pick's alive samples;
 * -1 on the exact path and from round R on), each may be NULL; *n_picked = R,
 * 0 when that ranking ran no selection.  Waits for the device.              */
int tpe_plan_hv_get(tpe_plan_t p, int32_t *picks, double *keys, int32_t *counts,
                    int32_t *n_picked, int32_t cap);

/* Device time (ms) of the last tpe_plan_suggest, from HIP events on the
 * plan's stream (recorded only while tpe_plan_profile is on, else NaN: an
 * event record drains the pipeline between launches); and the (candidate,
 * component) pairs it evaluated.                                           */
int tpe_plan_last_stats(tpe_plan_t p, double *score_ms, double *pairs);

/* Per-kernel profiling: record HIP events around each of the next `capacity`
 * scoring launches (one per level and candidate chunk; every lpdf kind of the
 * level), then read their average device duration and, for one lpdf kind
 * (0 LSE-GMM, 1 LSE-LGMM, 2 ERF-GMM, 3 ERF-LGMM, 4 categorical), the
 * (candidate, component) pairs per launch of that kind's active hps; kind 5
 * reads the value-lattice launches instead (their average duration and
 * lattice points x components per launch).
 * tpe_plan_profile also clears the ring (capacity 0: off).                  */
int tpe_plan_profile(tpe_plan_t p, int32_t capacity);
int tpe_plan_profile_read(tpe_plan_t p, int32_t kind, double *avg_ms,
                          int64_t *launches, double *pairs_per_launch);

/* Bounded quantized hps (quniform / qloguniform with finite bounds) are by
 * default scored on their value lattice: each distinct value j * q a drawn
 * candidate can take is scored once per suggest call and looked up by every
 * candidate (bit-identical lpdfs; chosen when the lattice is no larger than
 * the candidate count).  enable = 0 scores every candidate on its own (the
 * tpe.py:146-160 / 284-299 work as written), for A/B measurement and tests. */
int tpe_plan_set_lattice(tpe_plan_t p, int32_t enable);

/* Roofline accounting: read (counts may be NULL) and clear the census of the
 * scoring work since the last call -- counts[0] valid quantized (candidate,
 * component) pairs, [1] live ones (not an exact zero), [2] quantized pairs
 * evaluated (live for some lane of their wave), [3] valid log-sum-exp pairs,
 * [4] of [5] the ones evaluated in the one-exponent-per-wave form, [5]
 * log-sum-exp pairs evaluated (outside the component blocks skipped as exact
 * zeros; a wave's retried pass counts again) -- and switch the census on (enable != 0)
 * or off for the following suggests.  counts has 6 entries.               */
int tpe_plan_census(tpe_plan_t p, int32_t enable, int64_t *counts);
/* The same with n_counts entries (up to 13; [12]: the pairs credited to
 * candidates scored from the Chebyshev tables, also counted in [3], while
 * the table build's (node, component) pairs go into [3] and [5]): [6] of [5] the log-sum-exp pairs
 * evaluated in the block-local fp32 per-group-lift form (prune mode 3 on
 * mixtures below the one-exponent size), [7] of [4] the one-exponent pairs
 * evaluated again by a wave's second attempt (its exponent re-centred),
 * [8] of [4] the one-exponent pairs of wide blocks (mode 3's fp64 loop),
 * [9] of [4] the one-exponent pairs evaluated in the moment form of their
 * 16-component chunk (one exp2 + a degree-9 polynomial per chunk) or, [10]
 * of [9], of their 8-component block (one exp2 + a degree-15 polynomial),
 * [11] of [9] the 16-component chunks read at degree 15 (table 4).         */
int tpe_plan_census_n(tpe_plan_t p, int32_t enable, int64_t *counts, int32_t n_counts);

/* Debug: counts[s * n_hp + hp], s < n_suggest (at most the last call's), the
 * wave tiles (128 candidates each) the direct pass behind the Chebyshev
 * tables scored for hp in the plan's last scoring launch that took them: the
 * tiles within the tie window of a slot whose two tables are certified, every
 * tile of any other slot, 0 for an inactive hp, -1 for an hp no such launch
 * has scored.  Synchronizes the device.                                     */
int tpe_plan_tie_counts(tpe_plan_t p, int32_t n_suggest, int32_t *counts);
/* Debug: out[(s * n_hp + hp) * W + t], s < n_suggest (at most the last
 * call's), the best table score of wave tile t (candidates 128 t .. 128 t +
 * 127 of the sorted draw) of hp as the table pass of the plan's last scoring
 * launch that took the tables left it; W = 8 * the launch's tiles per slot
 * holds every wave tile of its candidate count.  Entries of hps without two
 * certified tables, of inactive hps and of wave tiles no such launch has
 * written are unspecified.  -inf: a wave tile the prefilter ruled out, in
 * the map or -- unless TPE_DRAW_PRUNE=0 -- already in the sorted draw, which
 * then neither ranked nor wrote its candidates (tpe_plan_cand_dump).
 * out == NULL: returns W (0: no such launch yet)
 * and copies nothing.  Synchronizes the device.                              */
int tpe_plan_tab_wmax(tpe_plan_t p, int32_t n_suggest, double *out);
/* Debug: out[c], c < 4096, the bound lattice of hp as the last fit left it:
 * an upper bound of the table score (the EI score the table pass computes)
 * over cell c of 4096 equal cells of [low, high] in the fitted domain, +inf
 * where no bound holds.  Builds the tables of the current fit if no launch
 * has yet.  out == NULL: returns the cell count and copies nothing.
 * TPE_E_INVALID when the hp takes no table, either side's table is not
 * certified or the prefilter is off (no lattice).  Synchronizes the device.  */
int tpe_plan_tab_bound(tpe_plan_t p, int32_t hp, double *out);
/* Debug: the Chebyshev table of (hp, side) -- side 0 the below mixture, 1 the
 * above one -- as the last fit left it: *y_lo and *inv_w of its header,
 * *ncert its certified panels (the table is used when ncert equals the panel
 * count) and panels[i], i < P, the panels as raw 144-byte records (16
 * coefficients, the exponent M, one unused double).  Any pointer may be NULL;
 * panels holds up to 64 records.  Builds the tables of the current fit if no
 * launch has yet.  Returns P (0: no table), or a negative status.
 * Synchronizes the device.                                                  */
int tpe_plan_tab_panels(tpe_plan_t p, int32_t hp, int32_t side, double *y_lo, double *inv_w,
                        int32_t *ncert, void *panels);
/* Debug: out[3 i + ...] = le, lr, lg of panel i < P of (hp, side): the log2 of
 * the interpolation bound, of the rounding bound and of the lower bound of the
 * mixture on the panel -- the panel is certified when max(le, lr) + 1 <= lg -
 * 28 (and everything is finite) -- as the last build computed them.  The first
 * call allocates the record and builds the tables again; later builds fill it
 * as they go.  out may be NULL.  Returns P, or a negative status.
 * Synchronizes the device.                                                  */
int tpe_plan_tab_cert(tpe_plan_t p, int32_t hp, int32_t side, double *out);
/* Debug: out[i], i < n, the wave tiles of (suggestion s, hp) the direct pass
 * of the plan's last scoring launch that took the tables was given, in list
 * order; n is that launch's tpe_plan_tie_counts entry (0 where it is -1).
 * out may be NULL (n alone); it holds up to the W of tpe_plan_tab_wmax
 * entries.  Adds no launch; synchronizes the device.  Returns n, or a
 * negative status.                                                          */
int tpe_plan_tie_list(tpe_plan_t p, int32_t s, int32_t hp, int32_t *out);
/* Debug: out[(s * n_hp + hp) * 18 + ...] = y_lo, y_hi, lo[8], hi[8], s <
 * n_suggest (at most the last call's): the hot intervals of hp -- closed
 * intervals [lo[i], hi[i]] of the centred fitted-domain value, an unused one
 * (+inf, -inf), outside of which no wave tile is table-scored -- and the range
 * [y_lo, y_hi] candidates are clamped into, as the plan's last scoring launch
 * that ran the prefilter's pilot left them.  Entries of hps without two
 * certified tables, of inactive hps and of hps no such launch has scored are
 * unspecified.  Synchronizes the device.                                    */
int tpe_plan_tab_hot(tpe_plan_t p, int32_t n_suggest, double *out);
/* Debug: the value-bucketed candidates of (suggestion s, hp) as the plan's
 * last sorted draw left them in the candidate buffer: values[i] and
 * positions[i] (the candidate's index within the launch's chunk), i < n, the
 * launch's candidates per slot.  Either pointer may be NULL; both NULL:
 * returns n and copies nothing.  Behind the pruning draw (TPE_DRAW_PRUNE, on
 * by default) the wave tiles it dropped -- -inf in tpe_plan_tab_wmax -- were
 * never written: their entries are unspecified.  Adds no launch; synchronizes
 * the device.  Returns n, or a negative status.                             */
int64_t tpe_plan_cand_dump(tpe_plan_t p, int32_t s, int32_t hp, double *values,
                           int32_t *positions);
/* Debug: the screened pruning draw's counters since the last read (reset on
 * read): out[0] sort blocks composed from the screened candidates, out[1]
 * sort blocks that fell back to the full draw, out[2] candidates whose CDF was
 * inverted in the blocks of out[0] (of up to 8192 each).  Slots that are not
 * screened count nowhere.  TPE_DRAW_SCREEN=0: all zero.  The counters take
 * one atomic add per sort block and wrap (2^24 blocks, 2^40 candidates).
 * Adds no launch; synchronizes the device.                                  */
int tpe_plan_draw_screen_stats(tpe_plan_t p, int64_t *out);

/* Prior draws of n_suggest whole suggestions (rand.suggest, the TPE startup
 * phase: hyperopt/rand.py:14-33, pyll/stochastic.py:30-142): every active hp
 * drawn from its prior, conditional hps routed by their parents' draws;
 * results[s][hp] = (0, value, 0, active=1) or (NaN, NaN, -1, 0) inactive.
 * Counter-based Philox keyed by seeds[s] (stream disjoint from candidate
 * draws); the history is not read.                                          */
int tpe_plan_sample_prior(tpe_plan_t p, const uint64_t *seeds, int64_t n_suggest,
                          tpe_result *out, int32_t out_on_device, void *stream);

/* Annealing suggestions (anneal.suggest, hyperopt/anneal.py:43-408): each of
 * n_suggest independent annealers (seeds[s]) walks the hps in hp_order -- set
 * once per plan with tpe_plan_set_anneal_order: the reference interpreter's
 * node-evaluation order, a permutation of the hp ids in which every hp comes
 * after the choices that lead to it (else TPE_E_INVALID; so does
 * tpe_plan_anneal before an order is set).  An
 * active hp with T > 0 history rows in which it is active (pending / failed
 * rows, loss +inf, count) takes an anchor row -- the first row of the
 * suggestion's anchor list that has the hp active, else a fresh one: rank
 * r = clip(g - 1, 0, T - 1), g geometric(1 / avg_best_idx), in ascending
 * (loss, row) order among the hp's rows, appended to the list -- and draws its
 * value from the prior narrowed around the anchor's value by shrink = 1 /
 * (1 + T shrink_coef); T = 0 draws from the prior.  results[s][hp] = (score:
 * the anchor's loss, value, index: the anchor row, active = 1), (0, value, 0,
 * 1) for a prior draw, (NaN, NaN, -1, 0) inactive.  Counter-based Philox keyed
 * by seeds[s], stream 2^30 | hp (candidate draws: hp, prior draws: 2^31 | hp),
 * counter 0, one draw4: u0 the rank draw (consumed only by a fresh anchor), u1
 * the value draw of bounded and categorical kinds, (u2, u3) the Box-Muller
 * pair of the normal kinds.  Reads the history (a pending update is flushed
 * first); stream-ordered; results are kept in the plan.
 * TPE_E_INVALID: avg_best_idx < 1, shrink_coef < 0, either non-finite,
 * n_suggest <= 0.                                                          */
int tpe_plan_set_anneal_order(tpe_plan_t p, const int32_t *hp_order, int32_t n_hp);
int tpe_plan_anneal(tpe_plan_t p, double avg_best_idx, double shrink_coef,
                    const uint64_t *seeds, int64_t n_suggest,
                    tpe_result *out, int32_t out_on_device, void *stream);

/* Debug: out[s * n_hp + hp], s < n_suggest (at most the last tpe_plan_anneal
 * call's): row -- the anchor row (-1: prior draw or inactive hp); rank -- the
 * clipped rank r of a fresh anchor (-1: the anchor was reused, or none);
 * u[0] the rank draw when one was made, then the value draws in the order
 * above (one for bounded / categorical kinds, two for normal kinds); unused
 * slots NaN.  Synchronizes the device.                                      */
typedef struct { int32_t row; int32_t rank; double u[4]; } tpe_anneal_trace;
int tpe_plan_anneal_trace(tpe_plan_t p, int32_t n_suggest, tpe_anneal_trace *out);

/* Large draws score log-sum-exp candidates on value-bucketed tiles.  mode 1
 * skips the blocks of 8 mixture components whose every term is below
 * 2^-(27 + log2 K) of each candidate's largest one (lpdf moved by <= 2^-26
 * ~ 1.5e-8 relative); mode 2 also gives each wave one exponent instead of a
 * per-group max (terms 2^(t - M), M an upper bound of the wave's terms),
 * guarded so no term's fp32 argument exceeds ~|4| where it matters (<= 3e-7
 * relative; else the wave falls back to mode 1); mode 3 (default) computes
 * mode 2's t - M in fp32 about each component block's own centre (packed
 * fp32 FMAs instead of fp64 ones; the exponent difference is exact, the
 * rest O(1), so the error stays at mode 2's level).  mode 0 evaluates every
 * (candidate, component) pair -- A/B measurement, tests.                    */
int tpe_plan_set_prune(tpe_plan_t p, int32_t mode);

/* Register-only microbenchmarks for the roofline: which = 0 v_exp_f32
 * (results/s), 1 fp64 FMA (flop/s), 2 OCML fp64 erf (results/s), 3 the
 * log-sum-exp (candidate, component) pair of the scoring kernel (pairs/s),
 * 4 a live quantized pair (2 fp64 erf; pairs/s), 5 the log-sum-exp pair of
 * the one-exponent-per-wave loop (tpe_plan_set_prune mode 2; pairs/s), 6 the
 * same pair in block-local fp32 (mode 3; pairs/s), 7 the per-group-lift pair
 * in block-local fp32 (mode 3 below the one-exponent size; pairs/s), 8 the
 * moment form of a 16-component chunk (one exp2 + a degree-9 polynomial per
 * candidate and chunk; pairs/s, 16 per chunk evaluation), 9 the 8-wide moment
 * form (one exp2 + a degree-15 polynomial per candidate and block of 8;
 * pairs/s, 8 per block evaluation).                                         */
int tpe_microbench(tpe_handle_t h, int32_t which, double *per_second);

/* Test probe of the device math helpers: out[i] = f(x[i]), i < n (host
 * pointers), with f = 0 fast_log, 1 fast_log2, 2 erfcinv_fast, 3 the library
 * erfc the draw table and the draw screen's zones call.  One element per
 * thread in 256-thread blocks, so wave j holds x[64 j .. 64 j + 63].  Another
 * `which` is TPE_E_INVALID.                                                 */
int tpe_math_probe(tpe_handle_t h, int32_t which, const double *x, int64_t n, double *out);

#ifdef __cplusplus
}
#endif
#endif /* TPE_ENGINE_H */
