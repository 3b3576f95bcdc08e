/*
 * phylo_hip.h -- C ABI of libphylo_hip.so, the MI355X (gfx950) Felsenstein
 * pruning engine behind phylo_utils' likelihood-engine seam.
 *
 * The reference selects its engine by module import
 * (phylo_utils/tree_model.py:1 `from phylo_utils.likelihood.numba_likelihood_engine
 * import clv, lnl_node`).  Every entry point below replaces one reference
 * interface; the citation is given on each declaration (paths relative to the
 * reference repository root).
 *
 * Conventions
 *   - plain pointers and sizes; no C++ types, no exceptions cross this ABI;
 *   - every int-returning call returns PU_OK (0) or a negative PU_E* code and
 *     records a message readable with pu_last_error();
 *   - host buffers are caller-owned and copied in/out; device buffers are
 *     owned by the context;
 *   - a context is bound to one device and one HIP stream and is not
 *     thread-safe (one host thread per context);
 *   - layouts are the reference's C-contiguous fp64 layouts:
 *       partials [site][category][state], scalers [site][category],
 *       P matrices [category][parent state][child state];
 *   - state rows (the simulator) are uint8 [row][site], one state index in [0, K) per byte,
 *     row-major with a row stride in bytes; a row is a tip slot or a node.
 */
#ifndef PHYLO_HIP_H
#define PHYLO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PU_OK 0
#define PU_E_ARG (-1)     /* bad argument / shape (numba raises on shape mismatch)     */
#define PU_E_HIP (-2)     /* HIP runtime error                                          */
#define PU_E_STATE (-3)   /* call order violated (e.g. run before set_schedule)         */
#define PU_E_SCHED (-4)   /* schedule is not a valid post-order over the declared tips  */
#define PU_E_NOMEM (-5)   /* device allocation failed                                   */
#define PU_E_COMM (-6)    /* RCCL error                                                 */

/* context flags */
#define PU_KEEP_PARTIALS 0x0 /* default: every internal CLV kept in HBM (tree_model.py:117-124) */
#define PU_LNL_ONLY 0x1      /* internal CLVs live only as long as needed (buffer reuse)        */
#define PU_NO_REORDER 0x2    /* evaluate ops in the caller's order (default: register-aware)    */

typedef struct pu_ctx pu_ctx;

/* ---- library / errors ------------------------------------------------------------- */
const char *pu_version(void);
/* Last error of ctx, or the process-wide last error when ctx is NULL. */
const char *pu_last_error(const pu_ctx *ctx);
int pu_device_count(int *n);

/* ---- stateless engine seam: exactly the numba engine's gufuncs --------------------- */
/* numba `clv`, phylo_utils/likelihood/numba_likelihood_engine.py:10-46.
 * p1,p2 [C][K][K]; clv1,clv2,out [S][C][K]; scaler_a,scaler_b,cml_scaler [S][C].
 * cml_scaler is written in place (numba_likelihood_engine.py:40,44). */
int pu_clv(int device, int n_states, int n_cat, int64_t n_sites, const double *p1,
           const double *p2, const double *clv1, const double *clv2, const double *scaler_a,
           const double *scaler_b, double *cml_scaler, double *out);
/* numba `lnl_node`, numba_likelihood_engine.py:82-87: out[s][c] = log(sum_i pi_i *
 * partials[s][c][i]) + scale[s][c], or -inf when the sum is <= 0. */
int pu_lnl_node(int device, int n_states, int n_cat, int64_t n_sites, const double *pi,
                const double *partials, const double *scale, double *out);

/* ---- discrete gamma: phylo_utils.discrete_gamma.discrete_gamma ---------------------- */
/* src/discrete_gamma.pyx:30-47 -> src/c_discrete_gamma.c:285-321 (alpha == beta).
 * Host routine (AS91 / AS32 / AS70 / Pike-Hill), no device involved. */
int pu_discrete_gamma(double alpha, int n_cat, int median_rates, double *rates_out);

/* ---- TreeModel-equivalent context ---------------------------------------------------- */
/* TreeModel.initialise allocation, tree_model.py:101-124.  n_nodes = 2N-2 node
 * indices as numbered by Traversal (traversal.py:16-21); n_patterns = S.
 * 1 <= n_cat <= 64, otherwise PU_E_ARG.  The traversal (pu_run) runs every n_cat up to 64
 * for n_states 2, 4 and 20.  The edge operations keep their matrices in the LDS of one
 * workgroup (160 KiB) and return PU_E_ARG, before any launch, above: pu_edge_derivs and the
 * optimisers n_cat 64 / 60 / 10 for n_states 2 / 4 / 20; pu_edge_lnl 64 / 64 / 21;
 * pu_update_partials 64 / 64 / 23.  The context stays usable after such a refusal. */
int pu_ctx_create(pu_ctx **out, int device, int n_nodes, int n_tips, int64_t n_patterns,
                  int n_cat, int n_states, int flags);
void pu_ctx_destroy(pu_ctx *ctx);

/* Tip partials for node `node` ([S][K]); tree_model.py:142-148 copies these into
 * every category -- the engine stores them once and broadcasts. */
int pu_set_tip_partials(pu_ctx *ctx, int node, const double *partials);
/* Compact tips (the same information as charmap partial vectors,
 * alignment/charmaps.py:8-86, alignment.py:26-37): one code table
 * [n_codes][K] per context (n_codes <= 256), then codes[S] per tip node.
 * A context whose tips are all coded streams 1 byte per tip site instead of
 * K doubles; mixing with pu_set_tip_partials is allowed (coded tips are then
 * expanded on the host). */
int pu_set_code_table(pu_ctx *ctx, int n_codes, const double *code_table);
int pu_set_tip_codes(pu_ctx *ctx, int node, const uint8_t *codes);
/* Pattern counts from alignment_to_numpy (alignment/alignment.py:47-51); default 1. */
int pu_set_pattern_weights(pu_ctx *ctx, const double *weights);
/* All tips at once (SURVEY 8(b) B2 `pu_set_tips`; tree_model.py:142-148): tip i is node
 * nodes[i]; exactly one of codes [n_tips][S] (with code_table [n_codes][K]) or partials
 * [n_tips][S][K]; pattern_weights [S] or NULL (all 1). */
int pu_set_tips(pu_ctx *ctx, int n_tips, const int32_t *nodes, int n_codes,
                const double *code_table, const uint8_t *codes, const double *partials,
                const double *pattern_weights);

/* A new topology over the same taxa (many trees on one alignment): tip
 * slot i -- the i-th tip node given to pu_set_tips / pu_set_tip_* -- becomes node
 * nodes[i] of the new numbering (Traversal, traversal.py:16-21).  No tip data move; the
 * next pu_set_schedule describes the new tree (tree_model.py:87-89 set_tree). */
int pu_set_tip_nodes(pu_ctx *ctx, int n_tips, const int32_t *nodes);

/* One resident alignment for many contexts (r06, SURVEY 8(e) G2: "the same (replicated)
 * alignment" per GPU; the reference holds one alignment and swaps trees,
 * tree_model.py:42-50, 87-89).  ctx -- fresh: no tips set yet -- reads owner's coded tips,
 * code table and pattern weights in place instead of holding its own copies; owner's tip
 * slot i is node nodes[i] of ctx's numbering (as pu_set_tip_nodes).  Both contexts must be
 * on one device with equal n_tips, S and K, and every owner tip must be coded.  From then on
 * the shared tips, table and weights are frozen in every context that holds them
 * (pu_set_tip_*, pu_set_code_table, pu_set_pattern_weights return PU_E_STATE); the storage
 * lives until the last context holding it is destroyed, in any order. */
int pu_share_tips(pu_ctx *ctx, pu_ctx *owner, int n_tips, const int32_t *nodes);

/* Model.p inputs (substitution_models/abstract.py:49-59, 99-105): evecs [K][K],
 * evals [K], ivecs [K][K] row-major; freqs [K] (lnl_node pi); rate-model rates and
 * weights [C] (rate_models.py:15-47). */
int pu_set_model(pu_ctx *ctx, const double *evecs, const double *evals, const double *ivecs,
                 const double *freqs, const double *rates, const double *weights);

/* Models without a real eigen-decomposition -- the non-reversible DNANonReversibleModel
 * family (Strsym, Unrest: P(t) = expm(Q r t), substitution_models/abstract.py:163-180):
 * pu_set_model_p sets freqs (lnl_node pi; q_to_freqs for these models), rates and weights,
 * and the context then skips its own P computation.  After every pu_set_schedule /
 * pu_set_branch_lengths the caller supplies the matrices with pu_set_pmatrices:
 * P [n_ops + 1][2][C][K][K] in the caller's op and child order (the row after the last op:
 * root_a's P(0), root_b's P(root_len); the layout pu_get_pmatrices returns); until then
 * pu_enqueue / pu_run fail with PU_E_STATE.  Edge operations (pu_edge_*, pu_update_partials,
 * pu_optimise_*) need pu_set_model and fail with PU_E_STATE on such a context.
 * pu_set_model switches back to device-computed P. */
int pu_set_model_p(pu_ctx *ctx, const double *freqs, const double *rates, const double *weights);
int pu_set_pmatrices(pu_ctx *ctx, const double *P);
/* Matrix provider of a context on host transition matrices (pu_set_model_p), for the
 * operations whose lengths are chosen on the device side of the ABI -- the edge lnL /
 * derivatives, partial updates and the Newton optimisers (pu_edge_*, pu_update_partials,
 * pu_optimise_*), and the traversal after they move a length.  fn(user, order, n, t, out)
 * fills out[n][C][K][K] with d^order/dt^order P(t[i] r_c), order 0, 1 or 2, the chain-rule
 * factor r_c included (for the non-reversible models r Q expm(Q r t) and r^2 Q^2 expm(Q r t);
 * the reference's DNANonReversibleModel.dp_dt / d2p_dt2, abstract.py:180-192, return
 * Q expm(Q r t) and Q^2 expm(Q r t)).  Returns 0, non-zero on failure.  NULL removes it. */
typedef int (*pu_pmat_provider)(void *user, int order, int n, const double *t, double *out);
int pu_set_pmatrix_provider(pu_ctx *ctx, pu_pmat_provider fn, void *user);

/* Traversal.postorder_traversal (traversal.py:28,36; utils.py:127-134): ops[n_ops][3]
 * = (parent, child1, child2); brlens[n_ops][2] = lengths of (parent,child1) and
 * (parent,child2) (Traversal.brlens); root edge (root_a, root_b, root_len) as in
 * compute_partials_at_edge (tree_model.py:178-198): P(0) on root_a, P(len) on root_b. */
int pu_set_schedule(pu_ctx *ctx, int n_ops, const int32_t *ops, const double *brlens,
                    int root_a, int root_b, double root_len);
/* New branch lengths for the current topology (same layout as pu_set_schedule). */
int pu_set_branch_lengths(pu_ctx *ctx, const double *brlens, double root_len);

/* compute_partials + compute_likelihood_at_edge + sum (tree_model.py:160-217,
 * bin/phy.py:146).  Synchronous: lnl_out = sum_s weight[s] * site_lnl[s]; sitewise_out
 * [S] (nullable) = the per-pattern lnL (tree_model.py:216, before the inverse-index
 * expansion). */
int pu_run(pu_ctx *ctx, double *lnl_out, double *sitewise_out);
/* Asynchronous form for timing loops: enqueue on the context stream only. */
int pu_enqueue(pu_ctx *ctx);
int pu_synchronize(pu_ctx *ctx, double *lnl_out);
/* Per-pattern log-likelihood (compute_likelihood_at_edge before the inverse-index
 * expansion, tree_model.py:216). */
int pu_get_site_lnl(pu_ctx *ctx, double *out);
/* Read back TreeModel.partials[node] / scale[node] (tips are expanded per category)
 * and root_partials / root_scale.  Requires PU_KEEP_PARTIALS for internal nodes; the root
 * after the context's own last run (not a pu_batch_enqueue, PU_E_STATE). */
int pu_get_partials(pu_ctx *ctx, int node, double *partials_out, double *scale_out);
int pu_get_root(pu_ctx *ctx, double *root_partials_out, double *root_scale_out);
/* Transition matrices the last run used: [n_ops+1][2][C][K][K] (last row = root). */
int pu_get_pmatrices(pu_ctx *ctx, double *out);

/* Lewis ascertainment-bias correction (TreeModel.set_ascertainment_bias_correction,
 * tree_model.py:92-98; dummy sites :151-156; correction :209-214).  The caller appends K
 * dummy invariant patterns [first_dummy, S) -- at dummy pattern first_dummy + k every tip
 * is the one-hot vector of state k -- with pattern weight 0.  After every evaluation
 * (pu_run / pu_enqueue / pu_edge_lnl): corr = log(1 - exp(x)), site_lnl[s] -= corr for
 * s < first_dummy, lnl -= corr * sum of their weights.  mode 1 (the reference): x =
 * logsumexp over the K x C lnl_node values of the dummy sites, unweighted over categories
 * (so NaN for Gamma rates with C > 1, as the reference); mode 2 (weighted Lewis): x =
 * logsumexp_k of the dummy sites' mixture lnL.  mode 0: off. */
int pu_set_ascertainment(pu_ctx *ctx, int mode, int64_t first_dummy);
/* The correction (log(1 - P(invariant))) the last evaluation applied. */
int pu_get_ascertainment_correction(pu_ctx *ctx, double *corr_out);

/* ---- edge operations on the resident CLVs (need PU_KEEP_PARTIALS) ------ */
/* Category limits (one workgroup's LDS holds the per-(category, site) values): edge lnL
 * C <= 194 (K = 4) / 21 (K = 20); derivatives and the optimisers C <= 72 (K = 2), 60 (K = 4),
 * 10 (K = 20).  Beyond them the call fails with PU_E_ARG. */
/* compute_partials_at_edge + compute_likelihood_at_edge (tree_model.py:178-217) with the
 * root on ANY edge (a, b) of the current topology, on the nodes' CURRENT partials (the
 * reference's "only valid if the CLVs at a and b are valid", tree_model.py:181-182): P(0) on
 * a, P(length of (a,b)) on b.  Writes the root partials (pu_get_root) and sitewise lnL;
 * PU_E_ARG "There is no edge connecting nodes a and b" as tree_model.py:184-187. */
int pu_edge_lnl(pu_ctx *ctx, int node_a, int node_b, double *lnl_out, double *sitewise_out);
/* out3 = {lnL, dlnL/dt, d2lnL/dt2} at edge length t = length (< 0: the current length) for
 * the pattern-weighted sum over sites of log sum_c w_c f_c, f_c as in lnl_branch_derivs
 * (numba_likelihood_engine.py:49-57) with dP/dt = evecs diag(l r e^{l t r}) ivecs -- the
 * exact derivative of P(t r); Model.dp_dt (abstract.py:61-77) omits the factor r. */
int pu_edge_derivs(pu_ctx *ctx, int node_a, int node_b, double length, double *out3);
/* In-place partials updates on any nodes, in order: partials[par] = clv(P(len1), P(len2),
 * partials[ch1], partials[ch2]) for ops[n][3] = (par, ch1, ch2), brlens[n][2] -- the
 * re-orientation and restore rows of the optimising traversal (utils.py:137-188). */
int pu_update_partials(pu_ctx *ctx, int n_ops, const int32_t *ops, const double *brlens);
/* Newton-Raphson (monotone safeguard) on the length of edge (a, b), all evaluations on the
 * device with the current partials of a and b; lengths are kept in [1e-8, 100].  The new
 * length is stored (pu_get_branch_lengths) and returned. */
int pu_optimise_edge(pu_ctx *ctx, int node_a, int node_b, double tol, int max_iter,
                     double *length_out, double *lnl_out);
/* One pass of the optimising traversal (Traversal.optimising_traversal, traversal.py:29,34-35;
 * utils.py:137-188): rows[n_rows][5]; a row (p, s, g, n, p) re-orients p towards n from s and
 * g, then optimises edge (n, p); (n, c1, c2, -1, -1) restores n; (-1, -1, -1, a, b) optimises
 * edge (a, b).  Ends with a full traversal at the new lengths: lnl_out; evals_out = Newton
 * iterations taken.  An error in mid-pass (a row that names no edge, a failed launch) runs that
 * traversal too, at the lengths reached so far, before the first error is returned. */
int pu_optimise_sweep(pu_ctx *ctx, int n_rows, const int32_t *rows, double tol, int max_iter,
                      double *lnl_out, int *evals_out);
/* The reference's own 1-D minimisers on the length of edge (a, b) (r06): method 1 = brent
 * (src/optimisation.pyx:86-177), 2 = dbrent (:179-297), over the objective f(t) = -lnL(t) (and
 * f'(t) = -dlnL/dt for dbrent) with the current partials of a and b: brent(lo, t0, hi, f, tol,
 * out) -- the bracket spanned by lo and hi, the search from t0 -- with the reference's steps,
 * tolerances, iteration limits and quirks (phylo_utils_amd/optimisation.py documents them).
 * out3 = the reference's out: {x, f(x), iterations}.  DNA contexts of up to 4 categories on
 * the device eigen-system run the whole minimisation in one persistent launch (the
 * k_edge_newton machinery); others one k_edge launch per evaluation, with the same state
 * machine.  The length x is stored (pu_get_branch_lengths). */
int pu_minimise_edge(pu_ctx *ctx, int node_a, int node_b, int method, double lo, double t0,
                     double hi, double tol, double *out3);
/* ---- nearest-neighbour interchange on resident partials ------------------ */
/* The largest category count the quartet kernel takes for n_states = 2, 4 or 20 (its LDS use
 * of one workgroup against the 160 KiB of a CU: 25, 24, 19); PU_E_ARG for other n_states.
 * Host only. */
int pu_quartet_max_cat(int n_states);
/* out9[3][3] = {lnL, d1, d2} of arrangements 0..2 at central lengths t[3] (t NULL: all three at
 * lens[4]); nodes[4] pairwise distinct; lens[5] = pendant lengths of nodes 0..3, then the
 * standing central length.  Arrangement 0 is (x0,x1 | x2,x3), the standing one; 1 is
 * (x0,x2 | x1,x3); 2 is (x0,x3 | x1,x2).  For (a,b | c,d): L = clv(P(l_a), P(l_b), a, b) and
 * R = clv(P(l_c), P(l_d), c, d) with the engine's rescale rule, then what pu_edge_derivs
 * defines for ends L, R at length t[k].  On the nodes' CURRENT partials, like pu_edge_lnl.
 * Changes nothing in the context.  PU_KEEP_PARTIALS contexts on the device eigen-system
 * without an ascertainment correction (else PU_E_STATE); PU_E_ARG: a null buffer, a node out
 * of range, repeated nodes, a non-positive or non-finite length, more categories than
 * pu_quartet_max_cat. */
int pu_quartet_derivs(pu_ctx *ctx, const int32_t nodes[4], const double lens[5],
                      const double *t, double *out9);
/* One scoring pass over the optimising traversal (rows as pu_optimise_sweep takes them, lengths
 * the context's current ones).  Every re-orientation / restore row is applied.  At every
 * optimise row (.., NOD, PAR) whose NOD is internal, and at row 0 when both ends are internal,
 * the quartet (children of NOD | SIB, GPA) is scored (row 0: the children of its second end
 * for SIB, GPA).  For each arrangement the central length is optimised from the standing one
 * with the library's own Newton rule (pu_optimise_edge's: safeguards, bounds [1e-8, 100],
 * stopping rule), the three arrangements advancing together, one k_quartet launch per
 * iteration.  scores_out [n_scored][3][4] = {t*, lnL(t*), lnL'(t*), evaluations}.
 * quartets_out [n_scored][6] = {NOD, PAR, x0, x1, x2, x3}.  *n_scored_out <= n_tips - 3; the
 * buffers hold n_tips - 3 entries.  No length is stored.  The pass ends with a full traversal,
 * so the context's partials, lnL and sitewise lnL are bitwise those of pu_run before the call.
 * An error in mid-pass (a row that names no edge, a failed launch) runs that traversal too before
 * the first error is returned.  PU_E_ARG also for tol <= 0 and max_iter < 0. */
int pu_nni_sweep(pu_ctx *ctx, int n_rows, const int32_t *rows, double tol, int max_iter,
                 double *scores_out, int32_t *quartets_out, int *n_scored_out);
/* HIP-event time (ms) of the last k_quartet launch made while pu_ctx_profile was on. */
int pu_quartet_kernel_ms(pu_ctx *ctx, double *ms_out);
/* ---- branch support on the quartet kernel: aLRT, aBayes, SH-aLRT ----------- */
/* site_out[3][S]: the unweighted per-pattern lnL of arrangements 0..2 at t[3] (NULL: lens[4]),
 * -inf where no rate category gives the pattern a positive likelihood; out9 (nullable) as
 * pu_quartet_derivs, bitwise equal to it.  Changes nothing in the context.  Refusals as
 * pu_quartet_derivs. */
int pu_quartet_site_lnl(pu_ctx *ctx, const int32_t nodes[4], const double lens[5],
                        const double *t, double *site_out, double *out9);
/* RELL sums: out[n_rep][n_vec] = B(W[r], L[v]) = sum_p W[r][p] L[v][p]; L fp64 [n_vec][n_sites],
 * W uint32 [n_rep][n_sites] (the device form: row strides ldl, ldw >= n_sites, ldo >= n_vec,
 * queued on `stream`).  A pattern with W[r][p] == 0 adds nothing, whatever L[v][p] is, -inf and
 * NaN included.  The order of the sum is a function of n_sites alone (segments of 2048 patterns
 * added serially, the segment sums added serially): out[r][v] does not depend on the other
 * replicates or vectors of the call, on their number or position, or on the strides.  Stateless.
 * PU_E_ARG, before any device is touched: a null buffer, n_vec, n_rep or n_sites < 1, a row
 * stride below its row. */
int pu_rell_sums(int device, int n_vec, int64_t n_sites, const double *L, int n_rep,
                 const uint32_t *W, double *out);
int pu_rell_sums_device(int device, void *stream, int n_vec, int64_t n_sites, const double *d_L,
                        int64_t ldl, int n_rep, const uint32_t *d_W, int64_t ldw, double *d_out,
                        int64_t ldo);
/* pu_nni_sweep's pass with supports: scores_out / quartets_out / *n_scored_out exactly as
 * pu_nni_sweep (bitwise).  At every scored edge one more k_quartet launch leaves the
 * per-pattern lnL s_k of the three arrangements at their optimised lengths on the device; after
 * the walk l_k = B(w, s_k) for the pattern weights w, and B(W[r], s_k) for replicates r =
 * first_rep .. first_rep + n_rep - 1 of pu_boot_weights' rule on (seed, r, w), come from
 * pu_rell_sums_device.  With d = l_0 - max(l_1, l_2), c_k = B(W[r], s_k) - l_k (-inf for an
 * l_k that is not finite) and g_r the gap between the largest and the second largest c_k:
 * support_out[n_scored][4] = {lrt = 2 max(d, 0), alrt_chi2 = erf(sqrt(lrt / 2)),
 * abayes = 1 / sum_k exp(l_k - l_0), sh_alrt = #{r : d > g_r + epsilon} / n_rep}, all NaN where
 * l_0 is not finite; rell_out (nullable) [n_scored][n_rep + 1][3] = B of row w (index 0) and of
 * every replicate.  The context is left as pu_nni_sweep leaves it, after an error in mid-pass
 * too; no length is stored.
 * Refusals as pu_nni_sweep, and PU_E_ARG, before the first launch, for n_rep < 1, a replicate
 * outside [0, 2^32), epsilon negative or non-finite, pattern weights that are negative,
 * non-integer or sum outside [1, 2^31 - 1].  PU_E_NOMEM (the message names the bytes) where the
 * site buffer [n_tips - 3][3][S] does not fit; the context stays usable. */
int pu_branch_support(pu_ctx *ctx, int n_rows, const int32_t *rows, double tol, int max_iter,
                      uint64_t seed, int64_t first_rep, int n_rep, double epsilon,
                      double *scores_out, int32_t *quartets_out, double *support_out,
                      double *rell_out, int *n_scored_out);
/* ---- impossible patterns on the resident-partials calls ---------------------
 * A pattern that no state explains (a dense tip row of zeros) has Z = 0 in every kernel that
 * mixes the categories (pu_edge_lnl, the quartet, ancestral, counts, placement and regraft
 * kernels).  What they write there:
 *   - the pattern's own lnL (sitewise lnL, pu_quartet_site_lnl) is -inf;
 *   - a lnL summed over the patterns is -inf if the pattern's weight is not 0, and does not see
 *     the pattern if it is 0: weight 0 adds exactly 0, never 0 x -inf (the traversal's own lnL,
 *     pu_run / pu_synchronize, included);
 *   - the per-pattern quotients post, map_prob, cat_post and mean_rate are 0 / 0 = NaN at that
 *     pattern, whatever its weight, and map_state there is unspecified; every other pattern is
 *     unaffected;
 *   - the count matrices take coef = pw w_c e^{..} / Z: exactly 0 for weight 0, NaN otherwise
 *     (gradient.edge_counts refuses a lnL that is not finite);
 *   - placement and regraft scores are sums over patterns and follow the second rule. */
/* ---- marginal ancestral states and site-rate posteriors -------------------- */
/* The largest category count the ancestral kernel takes for n_states = 2, 4 or 20: its LDS use
 * of one workgroup against the 160 KiB of a CU, and no more than a context holds (64, 50, 10);
 * PU_E_ARG for other n_states.  Host only. */
int pu_ancestral_max_cat(int n_states);
/* The marginal posterior of `node`'s state at every pattern, from the current partials of
 * `node` (the subtree on its side of the edge) and of `other` (everything else), the two ends
 * of one edge, at `length` (< 0: the edge's current length), like pu_edge_lnl on the nodes'
 * CURRENT partials: map_state[S] the most probable state (the lowest index on a tie),
 * map_prob[S] its posterior, post[S][K] all posteriors (NULL: not wanted), *lnl_out the
 * pattern-weighted lnL.  Changes nothing in the context.  PU_KEEP_PARTIALS contexts on the
 * device eigen-system (a reversible model) without an ascertainment correction (else
 * PU_E_STATE); PU_E_ARG: a null buffer, a node out of range, nodes not joined by an edge, a tip
 * as `node`, a zero or non-finite length, more categories than pu_ancestral_max_cat. */
int pu_ancestral_edge(pu_ctx *ctx, int node, int other, double length, uint8_t *map_state,
                      double *map_prob, double *post, double *lnl_out);
/* Every internal node in one pass over the optimising traversal (rows as pu_optimise_sweep
 * takes them, lengths the context's current ones).  Every re-orientation / restore row is
 * applied.  Row 0 reconstructs each end of the root edge from the other, every later row
 * (PAR, SIB, GPA, NOD, PAR) reconstructs NOD from PAR -- internal nodes only, each once, in that
 * order: nodes_out[n], map_state_out[n][S], map_prob_out[n][S], post_out[n][S][K] (NULL: not
 * wanted), node_lnl_out[n] (every entry the tree's lnL, by the pulley principle), *n_nodes_out
 * = n <= n_tips - 2; the buffers hold n_tips - 2 entries, more internal nodes in the rows are
 * PU_E_ARG.  The results stay on the device during the pass and are copied once per array.
 * The pass ends with a full traversal, so the context's partials, lnL and sitewise lnL are
 * bitwise those of pu_run before the call.  An error in mid-pass (a row that names no edge, a
 * failed launch) runs that traversal too before the first error is returned.  Refusals as
 * pu_ancestral_edge. */
int pu_ancestral_sweep(pu_ctx *ctx, int n_rows, const int32_t *rows, int32_t *nodes_out,
                       uint8_t *map_state_out, double *map_prob_out, double *post_out,
                       double *node_lnl_out, int *n_nodes_out);
/* Posterior of the rate category of every pattern, cat_post_out[S][C] (NULL: not wanted), and
 * its mean rate sum_c r(c) rate_c, mean_rate_out[S]: one launch on the root edge, on the
 * partials a traversal leaves.  Refusals as pu_ancestral_edge. */
int pu_site_rates(pu_ctx *ctx, double *cat_post_out, double *mean_rate_out);
/* HIP-event time (ms) of the last k_ancestral launch made while pu_ctx_profile was on. */
int pu_ancestral_kernel_ms(pu_ctx *ctx, double *ms_out);
/* ---- per-edge joint count matrices (the reference has none) ------------------- */
/* The largest category count the counts kernel takes for n_states = 2, 4 or 20: its LDS use of
 * one workgroup against the 160 KiB of a CU, no more than a context holds and, for 20 states,
 * one category per wave (64, 64, 6); PU_E_ARG for other n_states.  Host only.  (The reference
 * has none) */
int pu_counts_max_cat(int n_states);
/* The joint count matrices of one edge from the current partials of `node` (the subtree on its
 * side of the edge; it may be a tip) and of `other` (everything else), at `length` (< 0: the
 * edge's current length), like pu_edge_lnl on the nodes' CURRENT partials:
 *   counts_out[c][i][j] = sum_s pw_s (w_c e^{sigma_sc - m_s} / Z_s) A_sc(i) B_sc(j),
 * i the state at `node`, j the state at `other`, A and B their vectors, sigma the sum of their
 * scalers, m its maximum over the categories, Z the mixed site likelihood, pw the pattern
 * weight: the derivative of lnL in every entry of pi_j P_c(length)[j][i].  *lnl_out is the
 * pattern-weighted lnL.  A pattern of weight 0 adds exactly nothing; a pattern of non-zero
 * weight and likelihood 0 makes *lnl_out -inf and leaves the matrices unspecified.  Bitwise
 * reproducible; changes nothing in the context.  PU_KEEP_PARTIALS contexts on the device
 * eigen-system (a reversible model) without an ascertainment correction (else PU_E_STATE);
 * PU_E_ARG: a null buffer, a node out of range, nodes not joined by an edge, a zero or
 * non-finite length, more categories than pu_counts_max_cat.  (The reference has none; DESIGN
 * 4.18.) */
int pu_edge_counts(pu_ctx *ctx, int node, int other, double length, double *counts_out,
                   double *lnl_out);
/* Every edge in one pass over the optimising traversal (rows as pu_optimise_sweep takes them,
 * lengths the context's current ones).  Every re-orientation / restore row is applied; every
 * row with NOD >= 0 yields the matrices of edge (NOD, PAR), tip edges included, each edge once
 * and in that order: edges_out[n][2] = (NOD, PAR), lengths_out[n], counts_out[n][C][K][K] (i
 * the state at NOD, j at PAR, the end towards the root edge), edge_lnl_out[n] (every entry the
 * tree's lnL, by the pulley principle), *n_edges_out = n <= 2 n_tips - 3; the buffers hold
 * 2 n_tips - 3 entries, more edges in the rows are PU_E_ARG.  The results stay on the device
 * during the pass and are copied once per array.  The pass ends with a full traversal, so the
 * context's partials, lnL and sitewise lnL are bitwise those of pu_run before the call.  An
 * error in mid-pass (a row that names no edge, a failed launch) runs that traversal too before
 * the first error is returned.  Refusals as pu_edge_counts.  (The reference has none; DESIGN
 * 4.18.) */
int pu_counts_sweep(pu_ctx *ctx, int n_rows, const int32_t *rows, int32_t *edges_out,
                    double *lengths_out, double *counts_out, double *edge_lnl_out,
                    int *n_edges_out);
/* HIP-event time (ms) of the last k_counts launch made while pu_ctx_profile was on.  (The
 * reference has none) */
int pu_counts_kernel_ms(pu_ctx *ctx, double *ms_out);
/* ---- phylogenetic placement of query sequences (the reference has none) ------- */
/* A query q joins edge (n, o) of length t at its midpoint on a pendant branch of length l.  With
 * A, B the current vectors of the two ends at (pattern p, category c), sA, sB their scalers and
 * z the query's tip vector at a site, a row of code_table[n_codes][K]:
 *   a_pc(i)    = pi_i [P_c(t/2) A_pc](i) [P_c(t/2) B_pc](i)
 *   sigma_pc   = sA_pc + sB_pc,  m_p = max_c sigma_pc (categories with sum_i a_pc(i) > 0)
 *   F_p(l, z)  = sum_c w_c e^{sigma_pc - m_p} sum_i a_pc(i) [P_c(l) z](i)
 *   lnL(q,e,l) = sum_s sw_s (m_p(s) + log F_p(s)(l, z_qs))
 * the lnL of the tree with e split into halves and q hung from the new node (pulley principle).
 * Queries: query_codes[n_query][n_sites] uint8 into code_table (n_codes <= 32); site_pattern
 * [n_sites] the context pattern of every query column (NULL: the identity, n_sites = the
 * context's patterns); site_weight[n_sites] (NULL: 1).  A site of weight 0 adds nothing; one of
 * non-zero weight and F <= 0 makes the sum -inf.  Every call is bitwise reproducible, and a
 * query's numbers do not depend on the other queries of the call.
 * Common refusals, all before any launch: PU_KEEP_PARTIALS contexts on the device eigen-system
 * (a reversible model) without an ascertainment correction (else PU_E_STATE); PU_E_ARG: a null
 * buffer, n_query or n_sites < 1, n_codes outside [1, 32], a code >= n_codes, a site_pattern
 * entry outside [0, patterns), n_sites != patterns with a NULL map, l0 not finite or <= 0, tol
 * negative, max_iter < 0, more categories than pu_place_max_cat. */
/* The largest category count the placement kernels take for n_states = 2, 4 or 20: the table
 * kernel's LDS use of one workgroup against the 160 KiB of a CU, and no more than a context
 * holds; PU_E_ARG for other n_states.  Host only. */
int pu_place_max_cat(int n_states);
/* All queries at one edge, on the CURRENT partials of `node` and `other` (like pu_edge_counts)
 * at `length` (finite and > 0, else PU_E_ARG): score_out[Q] = lnL(q, e, l0), the pre-score;
 * then, from l0, pu_optimise_edge's Newton rule on l (bounds [1e-8, 100], `tol`, at most
 * max_iter steps) in the kernel: pendant_out[Q] = l*, lnl_out[Q] = lnL(l*), derivs_out[Q][2] =
 * dlnL/dl and d2lnL/dl2 at l*.  max_iter = 0 gives the pre-score alone: lnl_out = score_out,
 * pendant_out = l0, derivs_out NaN.  Changes nothing in the context. */
int pu_place_edge(pu_ctx *ctx, int node, int other, double length, int n_query, int64_t n_sites,
                  const uint8_t *query_codes, const int32_t *site_pattern,
                  const double *site_weight, int n_codes, const double *code_table, double l0,
                  double tol, int max_iter, double *score_out, double *pendant_out,
                  double *lnl_out, double *derivs_out);
/* The pre-score of every query at every edge in one pass over the optimising traversal (rows
 * and edge order as pu_counts_sweep: every row with NOD >= 0, tip edges included, each edge
 * once): edges_out[E][2] = (NOD, PAR), lengths_out[E], score_out[E][Q] = lnL(q, e, l0),
 * *n_edges_out = E <= 2 n_tips - 3; the buffers hold 2 n_tips - 3 edges, more in the rows are
 * PU_E_ARG.  The queries are uploaded once; the scores stay on the device during the pass and
 * are copied once.  The pass ends with a full traversal, so the context's partials, lnL and
 * sitewise lnL are bitwise those of pu_run before the call.  An error in mid-pass (a row that
 * names no edge, a failed launch) runs that traversal too before the first error is returned. */
int pu_place_prescore(pu_ctx *ctx, int n_rows, const int32_t *rows, int n_query, int64_t n_sites,
                      const uint8_t *query_codes, const int32_t *site_pattern,
                      const double *site_weight, int n_codes, const double *code_table, double l0,
                      int32_t *edges_out, double *lengths_out, double *score_out,
                      int *n_edges_out);
/* The same pass with the Newton rule of pu_place_edge for chosen (edge, query) pairs: at edge
 * number n of the pass (pu_place_prescore's order) the queries cand_query[cand_off[n] ..
 * cand_off[n + 1]) are optimised from l0; cand_off[n_edges + 1] starts at 0 and does not
 * decrease.  Per candidate: pendant_out, lnl_out, derivs_out[.][2], iters_out (Newton steps).
 * An edge with an empty list launches nothing beyond the pass's own rows.  PU_E_ARG also for a
 * candidate query outside [0, n_query) and for more edges in the rows than n_edges.  Ends with a
 * full traversal, as pu_place_prescore. */
int pu_place_refine(pu_ctx *ctx, int n_rows, const int32_t *rows, int n_query, int64_t n_sites,
                    const uint8_t *query_codes, const int32_t *site_pattern,
                    const double *site_weight, int n_codes, const double *code_table, double l0,
                    double tol, int max_iter, int n_edges, const int64_t *cand_off,
                    const int32_t *cand_query, double *pendant_out, double *lnl_out,
                    double *derivs_out, int32_t *iters_out);
/* HIP-event times (ms) of the last k_place_table, k_place_prescore and k_place_newton launches
 * made while pu_ctx_profile was on. */
int pu_place_kernel_ms(pu_ctx *ctx, double *table_ms, double *prescore_ms, double *newton_ms);
/* ---- subtree pruning and regrafting (the reference has no tree search) -------- */
/* Pruning the subtree on n's side of edge (n, o), o internal, dissolves o: its other neighbours
 * are joined by one edge of the sum of their two lengths, which leaves the rest tree R.  With A,
 * B the directed vectors of R at the ends of an edge of length t (neither holds the subtree), S
 * the vector at n pointing at o, sA, sB, sS their scalers and l = len(n, o):
 *   g_pc     = sum_i pi_i [P_c(t/2) A_pc](i) [P_c(t/2) B_pc](i) [P_c(l) S_pc](i)
 *   sigma_pc = sA_pc + sB_pc + sS_pc,  m_p = max_c sigma_pc (categories with g_pc > 0)
 *   score    = sum_p w_p (m_p + log sum_c w_c e^{sigma_pc - m_p} g_pc)
 * the lnL of the tree with the subtree regrafted at the edge's midpoint, every other length
 * unchanged (pulley principle).  A pattern of weight 0 adds nothing; one of non-zero weight and
 * a non-positive inner sum makes the score -inf.  A score is bitwise reproducible and depends
 * only on (A, B, S, t, l) and the pattern count.
 * Common refusals, before any launch: PU_KEEP_PARTIALS contexts on the device eigen-system (a
 * reversible model) without an ascertainment correction (else PU_E_STATE); PU_E_ARG: more
 * categories than pu_regraft_max_cat, a node outside [0, n_nodes), a repeated node among the
 * three scored, a length that is not finite or not > 0. */
/* The largest category count k_regraft takes for n_states = 2, 4 or 20: its LDS use of one
 * workgroup against the 160 KiB of a CU, and no more than a context holds; PU_E_ARG for other
 * n_states.  Host only. */
int pu_regraft_max_cat(int n_states);
/* One score on the CURRENT partials of nodes a, b (the edge's ends) and s (the subtree), tips
 * or kept internal nodes, at edge length t and pendant length l: *score_out.  Changes nothing
 * in the context. */
int pu_regraft_edge(pu_ctx *ctx, int a, int b, int s, double t, double l, double *score_out);
/* One pass over the optimising traversal (rows[n_rows][5], as pu_counts_sweep); while it stands
 * on the edge of row r it runs the inner rows inner_off[r] .. inner_off[r + 1] (inner_off
 * [n_rows + 1] starts at 0 and does not decrease; a row that names no edge has none).  Inner row
 * i is inner_rows[i][6] = (x0, x1, x2, A, B, S) with inner_len[i][4] = (len1, len2, t, l): if
 * x0 >= 0, node x0 is updated in place from x1 at len1 and x2 at len2 (pu_update_partials: a
 * re-orientation or a restore at explicit lengths); then, if A >= 0, scores_out[i] = the score
 * of (A, B, S, t, l); a row with A < 0 gets NaN.  The library knows nothing about trees: the
 * caller's rows of one edge must end with the restores that put back every node they
 * re-oriented.  Before the pass every kept partial is rewritten by the update kernel from its
 * children, so that a restore reproduces the bits it replaces.  The scores stay on the device
 * during the pass and are copied once.  PU_E_ARG also for inner_off[0] != 0 or decreasing,
 * inner rows on a row without an edge, and x0 equal to A, B or S of a scoring row; all rows are
 * checked before any launch.  The pass ends with a full traversal (its lnL to *lnl_out,
 * nullable), so the context's partials, lnL and sitewise lnL are bitwise those of pu_run before
 * the call.  An error in mid-pass (an update of a tip, a failed launch) runs that traversal too
 * before the first error is returned. */
int pu_spr_sweep(pu_ctx *ctx, int n_rows, const int32_t *rows, const int64_t *inner_off,
                 const int32_t *inner_rows, const double *inner_len, double *scores_out,
                 double *lnl_out);
/* HIP-event time (ms) of the last k_regraft launch made while pu_ctx_profile was on. */
int pu_spr_kernel_ms(pu_ctx *ctx, double *regraft_ms);
/* Current lengths in pu_set_schedule's layout: brlens_out[n_ops][2], root length. */
int pu_get_branch_lengths(pu_ctx *ctx, double *brlens_out, double *root_len_out);

/* ---- stateless branch likelihoods: the numba engine's lnl_branch / lnl_branch_derivs ---- */
/* numba_likelihood_engine.py:60-79 / :49-57 over E items (broadcast flattened by the caller):
 * item e uses probs[pidx ? pidx[e] : e % n_p] ([n_p][K][K], or [n_p][3][K][K] = P, dP, d2P
 * for the derivs); partials_a, partials_b [E][K]; scale_a, scale_b [E]; pi [K].
 * lnl_branch: out[E] = log(f) + sa + sb, f = sum((P . a) * b * pi);
 * lnl_branch_derivs: out[E][3] = {log f + sa + sb, f'/f, (f'' f - f'^2) / f^2}. */
int pu_lnl_branch(int device, int n_states, int64_t n_items, int n_p, const int32_t *pidx,
                  const double *probs, const double *pi, const double *partials_a,
                  const double *partials_b, const double *scale_a, const double *scale_b,
                  double *out);
int pu_lnl_branch_derivs(int device, int n_states, int64_t n_items, int n_p,
                         const int32_t *pidx, const double *probs, const double *pi,
                         const double *partials_a, const double *partials_b,
                         const double *scale_a, const double *scale_b, double *out);

/* ---- site-pattern compression --------------------------------------- */
/* Replaces np.unique(alignment, return_inverse=True, return_counts=True, axis=1) in
 * alignment_to_numpy (phylo_utils/alignment/alignment.py:40-57), on tip codes.
 * codes: [n_taxa][n_sites] uint8, row-major, each < n_codes (<= 256), numbered in the
 * lexicographic order of their partial vectors (then the byte order of code columns is the
 * order np.unique gives the float columns).  Outputs: *n_unique = U; unique_out [n_taxa][U]
 * (compact rows; the buffer holds n_taxa * n_sites bytes), counts_out [U], inverse_out
 * [n_sites] -- np.unique's three results, patterns in lexicographic order.  n_sites < 2^32,
 * n_taxa <= 65000.
 * Host buffers (copied in and out). */
int pu_compress_patterns(int device, const uint8_t *codes, int n_taxa, int64_t n_sites,
                         int n_codes, uint8_t *unique_out, int64_t *counts_out,
                         int64_t *inverse_out, int64_t *n_unique_out);
/* The same on device buffers, on the caller's HIP stream (hipStream_t as void*).  Row t of
 * the unique columns is written at d_unique + t * ld_unique (ld_unique >= n_sites; 0: U,
 * compact; an even ld_unique and base take 2-byte stores).  Returns when the result is
 * complete (U is read back between phases). */
int pu_compress_patterns_device(int device, void *stream, const uint8_t *d_codes, int n_taxa,
                                int64_t n_sites, int n_codes, uint8_t *d_unique,
                                int64_t ld_unique, int64_t *d_counts, int64_t *d_inverse,
                                int64_t *n_unique_out);

/* ---- simulation down the tree (the reference's src/simulation.pyx) -------------------- */
/* Replaces set_seed / weighted_choice(s) / evolve_states (src/simulation.pyx:13-19, 22-60,
 * 63-87).  The reference draws from libc rand(), one sequential stream; here every draw has
 * an address -- (seed, global site g, draw d) -- and is a pure function of it:
 *   (x0, x1, x2, x3) = Philox4x32-10(counter = (g lo, g hi, d, 0), key = (seed lo, seed hi)),
 *   u = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53 in [0, 1);
 *   pick(w[0..n), u): cum_j = cum_{j-1} + w_j (fp64 adds in index order), r = u * cum_{n-1},
 *   the first j with cum_j > r, else n - 1 (weighted_choice's comparison, :35-41; the
 *   reference returns 0 in that unreachable-in-practice case).
 * So results do not depend on the launch, the chunking, the op order or the site range of the
 * call: column g is the same in every call that covers it. */
/* src/simulation.pyx:63-87 evolve_states over one branch: child[s] = pick(probs[rate_class[s]]
 * [parent[s]][.], u(seed, first_site + s, draw)); probs [C][K][K] (the project layout; the
 * reference's is [K][K][C]).  K, C <= 256; rate_class may be NULL when C = 1.  PU_E_ARG:
 * n_sites <= 0, first_site < 0, a null buffer, a parent state >= K or a class >= C. */
int pu_evolve_states(int device, int n_states, int n_cat, int64_t n_sites, uint64_t seed,
                     int64_t first_site, uint32_t draw, const double *probs,
                     const uint8_t *parent_states, const uint8_t *rate_class,
                     uint8_t *child_states_out);
/* evolve_states down the whole tree (src/simulation.pyx:63-87 per branch, driven in the
 * reference by the caller's loop over the tree): ctx's current schedule oriented away from
 * root_a, its current lengths (those pu_get_branch_lengths returns, after pu_optimise_* /
 * pu_minimise_edge too) and model.  Site g = first_site + column draws d = 0: its rate category,
 * pick(weights); d = 1: the state of root_a, pick(freqs); d = 2 + v: the state of every other
 * node v, pick(P_v[category][state of v's parent][.]), P_v = P(len_v * rate) and root_b hanging
 * from root_a with root_len.  P comes from the model's eigen-system on the device, or -- on a
 * context on host matrices (pu_set_model_p) -- from its pu_pmat_provider (order 0).  Needs no
 * tip data beyond the tip declarations the schedule required and changes no result of the
 * context.  tips_out [n_tips][n_sites] in tip-slot order; nullable: cats_out [n_sites],
 * nodes_out [n_nodes][n_sites] (every node's state), cum_out [n_nodes][C][K][K] (the cumulative
 * rows the draws used: row v is the edge above v, row root_a is zero).  Sites are processed
 * in chunks (a node-major uint8 workspace of at most 256 MiB; PU_SIM_CHUNK=<sites>, read at each
 * call, overrides the chunk).  PU_E_STATE: before pu_set_model* / pu_set_schedule, or host
 * matrices without a provider; PU_E_ARG: n_sites <= 0, first_site < 0, null tips_out. */
int pu_simulate(pu_ctx *ctx, uint64_t seed, int64_t first_site, int64_t n_sites,
                uint8_t *tips_out, uint8_t *cats_out, uint8_t *nodes_out, double *cum_out);
/* The same into device buffers on the context's stream, rows ld bytes apart (ld >= n_sites,
 * ld_nodes >= n_sites, else PU_E_ARG), ready for pu_compress_patterns_device; asynchronous
 * (a repeated call on an unchanged tree only queues kernels).  d_cats, d_nodes nullable. */
int pu_simulate_device(pu_ctx *ctx, uint64_t seed, int64_t first_site, int64_t n_sites,
                       uint8_t *d_tips, int64_t ld, uint8_t *d_cats, uint8_t *d_nodes,
                       int64_t ld_nodes);

/* ---- pairwise ML distances (the reference's phylo_utils/likelihood.py:226-236) --------- */
/* Replaces optimise(model, partials_a, partials_b, min_brlen, max_brlen) (likelihood.py:226-236,
 * with brent_optimise / scipy_optimise beside it), which returns (t, -1 / lnL''(t)) for two
 * sequences, for every requested pair of a coded alignment at once, with no context (DESIGN
 * 4.11, normative).  codes: uint8 [n_taxa][n_sites], row-major, each < n_codes <= 32, rows of
 * code_table [n_codes][K]; site_weights [n_sites] (NULL: 1; pattern counts after compression).
 * pairs [n_pairs][2] taxon indices in any order, repeats allowed; NULL: all i < j in row-major
 * order, and n_pairs must then be n_taxa (n_taxa - 1) / 2.
 *   lnL_ab(t) = sum_{u,v} N_ab[u][v] log F_uv(t), N_ab[u][v] = sum_s w_s [a_s = u][b_s = v],
 *   F_uv(t) = sum_m L[u][m] R[v][m] g_m(t), L[u][m] = sum_i pi_i x_u[i] evecs[i][m],
 *   R[v][m] = sum_j ivecs[m][j] x_v[j], g_m(t) = sum_c q_c exp(evals_m r_c t); derivatives in t
 *   with the factor r_c included, as pu_edge_derivs; F' = F'' = 0 for a bin whose code u or v
 *   has a constant tip vector (a gap: F does not depend on t).
 * Pairs are processed in chunks (count matrices and their per-segment slabs within 256 MiB;
 * PU_DIST_CHUNK=<pairs>, read at each call, lowers the chunk); no result depends on the chunk.
 * PU_E_ARG, before any device is touched: a null buffer, n_taxa < 2, n_sites <= 0, n_codes
 * outside [1, 32], n_states not 2, 4 or 20, n_cat outside [1, PU_PAIR_MAX_CAT] (the kernel
 * keeps rates and weights in LDS), !(0 < lo < hi), tol <= 0, max_iter < 0, a pair index out of
 * range or i == j, n_pairs < 1, ld < n_sites, a t0 outside [lo, hi], and -- host forms -- a code
 * >= n_codes. */
#define PU_PAIR_MAX_CAT 64
/* likelihood.py:226-236's sufficient statistic: counts_out [n_pairs][n_codes][n_codes], the
 * weighted pair count matrices N_ab (row: the code of the pair's first taxon).  A bin's adds run
 * in site order within a segment of the sites and the segments are added in order; the
 * segmentation depends on n_sites alone.  With integer weights the counts are exact. */
int pu_pair_counts(int device, const uint8_t *codes, int n_taxa, int64_t n_sites, int n_codes,
                   const double *site_weights, int64_t n_pairs, const int32_t *pairs,
                   double *counts_out);
/* likelihood.py:226-236 for every pair: out5 [n_pairs][5] = {t, lnL(t), lnL'(t), lnL''(t),
 * evaluations} -- the variance is -1 / lnL''(t).  A safeguarded Newton iteration on lnL'(t) = 0
 * in [lo, hi], one wave per pair in one launch per chunk: lnL'(lo) <= 0 gives t = lo (one
 * evaluation; a pair without an informative site lands here with zero derivatives), lnL'(hi)
 * >= 0 gives t = hi (two); otherwise, from t0 (NULL, or not inside: sqrt(lo hi)), a bracket
 * lnL'(a) > 0 > lnL'(b) is kept, the Newton step is taken when lnL'' < 0 and it stays inside the
 * bracket, else the bracket is halved; a step below tol is taken and the result evaluated where
 * it lands; after max_iter iterations without such a step the last evaluated point is returned
 * (evaluations = 2 + max_iter: not converged).  max_iter = 0: one evaluation at t0.  A bin with
 * N > 0 and F <= 0 gives lnL = -inf and t = lnL' = lnL'' = NaN.  Results are bitwise repeatable. */
int pu_pair_distances(int device, int n_states, int n_cat, int n_codes, const double *code_table,
                      const double *evecs, const double *evals, const double *ivecs,
                      const double *freqs, const double *rates, const double *cat_weights,
                      const uint8_t *codes, int n_taxa, int64_t n_sites,
                      const double *site_weights, int64_t n_pairs, const int32_t *pairs,
                      const double *t0, double lo, double hi, double tol, int max_iter,
                      double *out5);
/* likelihood.py:226-236 on device buffers -- the output of pu_simulate_device or
 * pu_compress_patterns_device with no copy: d_codes rows ld bytes apart (ld >= n_sites),
 * d_site_weights (nullable) and d_out5 in device memory; the model, pairs and t0 are host
 * buffers, copied before the call returns.  Asynchronous on the caller's stream (hipStream_t as
 * void*).  Precondition: every code < n_codes (a larger code is counted nowhere). */
int pu_pair_distances_device(int device, void *stream, int n_states, int n_cat, int n_codes,
                             const double *code_table, const double *evecs, const double *evals,
                             const double *ivecs, const double *freqs, const double *rates,
                             const double *cat_weights, const uint8_t *d_codes, int64_t ld,
                             int n_taxa, int64_t n_sites, const double *d_site_weights,
                             int64_t n_pairs, const int32_t *pairs, const double *t0, double lo,
                             double hi, double tol, int max_iter, double *d_out5);
/* Event timing of the pair kernels (scripts/time_distances.py): with pu_pair_profile(device, 1)
 * every pair call records events around its launches; pu_pair_kernel_ms waits for the last
 * call's and returns the time of its count launches (k_pair_counts and the slab merge) and of
 * its k_pair_newton launches, in ms, summed over the chunks. */
int pu_pair_profile(int device, int on);
int pu_pair_kernel_ms(int device, double *counts_ms, double *newton_ms);

/* ---- neighbour joining and BIONJ from a distance matrix (normative) -------- */
/* A tree from a distance matrix, or one per matrix of a batch: classic neighbour joining
 * (method 0; Saitou-Nei in the Studier-Keppler form) or BIONJ (method 1; Gascuel 1997, variances
 * initialised to the distances).  D [n_mat][n][n], row-major; only the upper triangle is read
 * and the diagonal is ignored.  Tips are clusters 0..n-1 and join m creates cluster n + m:
 *   joins_out [n_mat][n-2][2]  the child ids of cluster n + m, smaller id first
 *   lens_out  [n_mat][n-2][2]  their branch lengths, raw (they may be negative)
 *   root_out  [n_mat][2], root_len_out [n_mat]  the root edge (2n-3, the last other cluster) and
 *             its length: 2n-2 nodes with the root on an edge, the shape pu_set_schedule takes
 *   q_out     [n_mat][n-3], nullable  the criterion Q of every chosen pair but the last
 * While r > 3 clusters are live the pair a < b with the smallest Q_ab = (r-2) D_ab - R_a - R_b
 * is joined (R: row sums, taken once in index order and updated after; ties to the
 * lexicographically smallest (a, b)); the last three are joined without a criterion.  Every
 * result is bitwise repeatable and does not depend on the tier.
 * Tier A keeps the matrix in the LDS of one workgroup (n up to the n pu_nj_max_lds_n returns,
 * one workgroup per matrix, one launch); tier B keeps it in device memory (two launches per
 * join, all queued without a host read-back; matrices one after another).
 * PU_NJ_TIER=A|B, read at each call, forces a tier where n allows it.
 * PU_E_ARG, before any device is touched: a null buffer other than q_out, n < 3,
 * n > PU_NJ_MAX_N (the working copies are n^2 doubles), n_mat < 1, method outside {0, 1},
 * ld < n and -- host form -- a negative or non-finite entry of an upper triangle. */
#define PU_NJ_MAX_N 8192
int pu_nj(int device, int method, int n_mat, int n, const double *D, int32_t *joins_out,
          double *lens_out, int32_t *root_out, double *root_len_out, double *q_out);
/* The same on device buffers: matrix b starts at d_D + b n ld, its rows ld doubles apart
 * (ld >= n); the outputs are device buffers.  Asynchronous on the caller's stream (hipStream_t
 * as void*). */
int pu_nj_device(int device, void *stream, int method, int n_mat, int n, const double *d_D,
                 int64_t ld, int32_t *d_joins, double *d_lens, int32_t *d_root,
                 double *d_root_len, double *d_q);
/* The largest n whose matrix (method 1: matrices) fits the 160 KiB of LDS of one workgroup
 * (tier A); host only. */
int pu_nj_max_lds_n(int method);
/* The t column of pu_pair_distances_device's rows d_out5 [n_pairs][5] as a matrix d_D (rows ld
 * doubles apart, ld >= n_taxa), so that a distance run feeds pu_nj_device with no host copy.
 * pairs NULL (n_pairs = n_taxa (n_taxa - 1) / 2, all i < j row-major): the whole symmetric
 * matrix with a zero diagonal is written.  With a pair list (host buffer [n_pairs][2], copied
 * before the call returns) both entries of every listed pair are written and nothing else.
 * Asynchronous on the caller's stream.  PU_E_ARG as for the pair calls. */
int pu_pair_matrix_device(int device, void *stream, int n_taxa, int64_t n_pairs,
                          const int32_t *pairs, const double *d_out5, double *d_D, int64_t ld);

/* ---- bootstrap support of distance trees (normative) ------------------------ */
/* The nonparametric bootstrap (Felsenstein 1985) of a neighbour-joining or BIONJ tree, with no
 * host copy between its steps.  The resampling rule: S site patterns with non-negative integer
 * weights w_s (fp64; NULL: all 1), N = sum_s w_s in [1, 2^31 - 1].  Replicate r -- a global
 * number, r = first_rep + its row, so that a call continues a series -- draws N columns
 * j = 0..N-1:
 *   (x0, x1, ..) = philox4x32_10(counter = (j lo, j hi, r, 1), key = (seed lo, seed hi))
 *   u = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53     (the simulator's u; counter word 3 = 1)
 *   c = min(floor(u * N), N - 1)                    (one fp64 multiply)
 *   s = the first pattern whose inclusive integer prefix sum of w exceeds c;  W[r][s] += 1
 * w_out uint32 [n_rep][n_sites]: every row sums to N, a pattern of weight 0 is never drawn, and
 * a row depends on (seed, r, w) alone.
 * PU_E_ARG, before any device is touched: a null output, n_rep < 1, n_sites < 1, replicate
 * numbers outside [0, 2^32), N outside [1, 2^31 - 1] and -- host form -- a weight that is
 * negative, non-integer or non-finite. */
int pu_boot_weights(int device, uint64_t seed, int64_t first_rep, int n_rep, int64_t n_sites,
                    const double *site_weights, uint32_t *w_out);
/* The same on device buffers: d_site_weights (nullable) and d_w, its rows ldw words apart
 * (ldw >= n_sites; the words between n_sites and ldw are left alone).  Asynchronous on the
 * caller's stream (hipStream_t as void*).  Precondition: the device weights obey the rule (with
 * N outside its range W is all zero). */
int pu_boot_weights_device(int device, void *stream, uint64_t seed, int64_t first_rep, int n_rep,
                           int64_t n_sites, const double *d_site_weights, uint32_t *d_w,
                           int64_t ldw);
/* Scaled resampling (normative; the multiscale bootstrap of the AU test): the rule
 * above with j = 0..n_draw-1 -- c = min(floor(u * N), N - 1) still uses N --, so every row sums
 * to n_draw, a pattern of weight 0 is never drawn, and with n_draw = N a row is pu_boot_weights'
 * row bit for bit.  n_draws (nullable, int64 [n_rep]) gives every row its own number of columns
 * and n_draw is then not read by the rule: one call fills rows of different scales.
 * PU_E_ARG as pu_boot_weights, and for n_draw (without n_draws) or -- host form -- an entry of
 * n_draws outside [1, 2^31 - 1]. */
int pu_boot_weights_scaled(int device, uint64_t seed, int64_t first_rep, int n_rep,
                           int64_t n_sites, const double *site_weights, int64_t n_draw,
                           const int64_t *n_draws, uint32_t *w_out);
/* The same on device buffers, as pu_boot_weights_device; d_n_draws (nullable) is a device
 * buffer, and with it a positive n_draw only sizes the launch (the longest row).  Precondition:
 * every entry of d_n_draws lies in [1, 2^31 - 1] (a row whose entry does not stays zero). */
int pu_boot_weights_scaled_device(int device, void *stream, uint64_t seed, int64_t first_rep,
                                  int n_rep, int64_t n_sites, const double *d_site_weights,
                                  int64_t n_draw, const int64_t *d_n_draws, uint32_t *d_w,
                                  int64_t ldw);
/* The pair count matrices of every replicate in one pass over the alignment: counts_out
 * [n_rep][n_pairs][n_codes][n_codes] fp64, N[r][p][u][v] = the sum of W[r][s] over the sites
 * where pairs[p]'s first taxon shows code u and its second code v.  W uint32 [n_rep][n_sites];
 * codes, pairs and n_codes as in pu_pair_counts.  The sums are integers: the result is exact,
 * does not depend on the tiling, the segments or the chunks (PU_DIST_CHUNK caps the pairs of a
 * chunk here too), and equals pu_pair_counts with site_weights = W[r] bit for bit.
 * PU_E_ARG as for pu_pair_counts, and for n_rep < 1, a null W and a row of W whose sum is
 * outside [1, 2^31 - 1]. */
int pu_boot_pair_counts(int device, const uint8_t *codes, int n_taxa, int64_t n_sites, int n_codes,
                        const uint32_t *W, int n_rep, int64_t n_pairs, const int32_t *pairs,
                        double *counts_out);
/* pu_pair_distances for every replicate: out5_out [n_rep][n_pairs][5], the rows of replicate r
 * bitwise equal to pu_pair_distances(..., site_weights = W[r], t0 = NULL, ...).  The counts of
 * all replicates are taken in one pass (above) and all replicates x pairs go through the pair
 * calls' Newton kernel as one list.  PU_E_ARG as for pu_pair_distances and pu_boot_pair_counts. */
int pu_boot_distances(int device, int n_states, int n_cat, int n_codes, const double *code_table,
                      const double *evecs, const double *evals, const double *ivecs,
                      const double *freqs, const double *rates, const double *cat_weights,
                      const uint8_t *codes, int n_taxa, int64_t n_sites, const uint32_t *W,
                      int n_rep, int64_t n_pairs, const int32_t *pairs, double lo, double hi,
                      double tol, int max_iter, double *out5_out);
/* The same on device buffers (d_codes rows ld bytes apart, d_W rows ldw words apart, d_out5); the
 * model and pairs are host buffers, copied before the call returns.  With d_D non-null (all
 * pairs only: pairs NULL) the t column of every replicate is also written as the symmetric
 * matrices d_D [n_rep][n_taxa][ldd] with a zero diagonal, the entries pu_pair_matrix_device
 * writes, ready for pu_nj_device.  Asynchronous on the caller's stream. */
int pu_boot_distances_device(int device, void *stream, int n_states, int n_cat, int n_codes,
                             const double *code_table, const double *evecs, const double *evals,
                             const double *ivecs, const double *freqs, const double *rates,
                             const double *cat_weights, const uint8_t *d_codes, int64_t ld,
                             int n_taxa, int64_t n_sites, const uint32_t *d_W, int64_t ldw,
                             int n_rep, int64_t n_pairs, const int32_t *pairs, double lo, double hi,
                             double tol, int max_iter, double *d_out5, double *d_D, int64_t ldd);
/* Split support.  The reference and the n_rep replicates are trees in pu_nj's join form over
 * the same n tips (ref_joins [n-2][2], ref_root [2]; joins [n_rep][n-2][2], roots [n_rep][2]).
 * The nontrivial splits of a tree are the tip sets of its clusters n + m, m = 0..n-4 (cluster
 * 2n-3 shares the root edge's split with root[1], or is trivial), each a bitset of
 * ceil(n / 64) words, complemented when it holds tip 0.  support_out [n-3]: support[m] = the
 * number of ok replicates whose tree holds a split equal, word for word, to the reference's
 * split m, divided by n_ok; n_ok_out [1] = the number of replicates with ok[r] != 0 (ok int32
 * [n_rep], NULL: all).  n_ok = 0 gives NaN.
 * PU_E_ARG, before any device is touched: a null buffer other than ok, n < 3, n > PU_NJ_MAX_N,
 * n_rep < 1 and -- host form -- a join of a cluster that is not live. */
int pu_split_support(int device, int n, int n_rep, const int32_t *ref_joins,
                     const int32_t *ref_root, const int32_t *joins, const int32_t *roots,
                     const int32_t *ok, double *support_out, int32_t *n_ok_out);
int pu_split_support_device(int device, void *stream, int n, int n_rep, const int32_t *d_ref_joins,
                            const int32_t *d_ref_root, const int32_t *d_joins,
                            const int32_t *d_roots, const int32_t *d_ok, double *d_support,
                            int32_t *d_n_ok);
/* The whole bootstrap on one stream, only the outputs coming back: the reference tree (method 0
 * NJ, 1 BIONJ) of the distances under site_weights, then replicates 0..n_rep-1 of (seed,
 * site_weights): their W, distances, matrices, ok[r] = every upper-triangle distance of
 * replicate r is finite, trees and the support of the reference tree's splits over the ok
 * replicates (a replicate with ok = 0 has an unspecified tree).  ref_*_out as pu_nj's outputs
 * for one matrix, support_out [n-3], n_ok_out [1], rep_joins_out [n_rep][n-2][2] and
 * rep_roots_out [n_rep][2] nullable.  Every result equals the composition of the separate calls
 * above, pu_pair_distances, pu_pair_matrix_device and pu_nj, bit for bit.
 * The call holds the out5 rows, matrices and join arrays of all replicates on the device at once,
 * (1 + n_rep) (5 n (n - 1) / 2 + n^2 + 2 (n - 2) + 1) doubles, and W (n_rep n_sites words); only
 * the count matrices are chunked.  Where that does not fit it returns PU_E_NOMEM, and the
 * separate calls over ranges of replicates (first_rep) still run.  The split comparison is
 * written for trees of up to a few hundred taxa (n^2 n_rep ceil(n / 64) word compares, no hash
 * prefilter); it is correct, but has not been timed, in the thousands.
 * PU_E_ARG: n_taxa < 3, and as for those calls. */
int pu_bootstrap_nj(int device, int method, int n_states, int n_cat, int n_codes,
                    const double *code_table, const double *evecs, const double *evals,
                    const double *ivecs, const double *freqs, const double *rates,
                    const double *cat_weights, const uint8_t *codes, int n_taxa, int64_t n_sites,
                    const double *site_weights, uint64_t seed, int n_rep, double lo, double hi,
                    double tol, int max_iter, int32_t *ref_joins_out, double *ref_lens_out,
                    int32_t *ref_root_out, double *ref_root_len_out, double *support_out,
                    int32_t *n_ok_out, int32_t *rep_joins_out, int32_t *rep_roots_out);
/* Event timing of the two hot stages (scripts/time_bootstrap.py), as pu_pair_profile does for
 * the pair calls: with pu_boot_profile(device, 1) every pu_boot_pair_counts / pu_boot_distances*
 * call records events around its launches; pu_boot_kernel_ms waits for the last call's and
 * returns the time of its count launches (k_boot_pair_counts and the slab merge) and of its
 * k_pair_newton launches, in ms, summed over the chunks.  PU_BOOT_REP_CHUNK, read at each call,
 * caps the replicates of a chunk as PU_DIST_CHUNK caps the pairs; no result depends on either. */
int pu_boot_profile(int device, int on);
int pu_boot_kernel_ms(int device, double *counts_ms, double *newton_ms);

/* ---- topology tests of candidate trees (normative) ----------------------------
 * The replicate counts behind RELL bootstrap proportions (Kishino et al. 1990), the KH test
 * (Kishino & Hasegawa 1989), the SH test (Shimodaira & Hasegawa 1999), expected likelihood
 * weights (Strimmer & Rambaut 2002) and the multiscale bootstrap of the AU test (Shimodaira
 * 2002).  The reference has no topology test: the rule is DESIGN 4.24's and
 * tests/topotest_reference.py restates it.
 * L fp64 [T][S]: the unweighted per-pattern lnL of T trees; site_weights [S]: non-negative
 * integers, N = their sum in [1, 2^31 - 1]; scales [K]: r_1 .. r_K.  Block 0 draws n_0 = N
 * columns, block k >= 1 n_k = floor(r_k N + 0.5) (two fp64 roundings); replicate i < R of block k
 * is replicate first_rep + k R + i of pu_boot_weights_scaled's rule with n_draw = n_k, so block 0
 * holds pu_boot_weights' rows.  B[r][t] = pu_rell_sums(W[r], L[t]), l_t = B(w, L[t]) with w the
 * weights as a uint32 row.  A tree whose l_t is not finite is excluded: it enters no argmax or
 * max (its l and c count as -inf) and all its counts are 0.  c_t[r] = B[r][t] - l_t.
 *   counts_out uint32 [K + 1][3][T]:
 *     [k][0][t] = #{r of block k : t = argmax_u B[r][u], ties to the lowest t}
 *     [0][1][t] = #{r of block 0 : c_u*[r] - c_t[r] >= l_u* - l_t},  u* = argmax_{u != t} l_u,
 *                 ties to the lowest u                                               (KH)
 *     [0][2][t] = #{r of block 0 : max_u c_u[r] - c_t[r] >= max_u l_u - l_t}         (SH)
 *     [k][1], [k][2] = 0 for k > 0
 *   lnl_out [T] = l;  n_draw_out int64 [K + 1] = n;  rell_out (nullable) [K + 1][R][T] = B.
 * Every compared value is a single fp64 subtraction and the counts are integers, so no result
 * depends on the launch shape or on the ranges of rows the call walks (256 MiB of W at most;
 * PU_TOPO_REP_CHUNK, read at each call, caps the rows of a range).  Stateless; everything is
 * freed on return.
 * PU_E_ARG, before any device is touched, the message naming the argument: a null buffer, T
 * outside [2, 1024], S < 1, R < 1, K < 0, a scale that is not finite and positive or whose n_k
 * is outside [1, 2^31 - 1], a weight that is negative, non-integer or non-finite, N outside
 * [1, 2^31 - 1], first_rep < 0 or first_rep + (K + 1) R > 2^32.  PU_E_NOMEM (the message names
 * the bytes) where a buffer does not fit. */
int pu_topology_tests(int device, int T, int64_t S, const double *L, const double *site_weights,
                      uint64_t seed, int64_t first_rep, int R, int K, const double *scales,
                      uint32_t *counts_out, double *lnl_out, int64_t *n_draw_out,
                      double *rell_out);
/* Event timing of its three stages (scripts/time_topotest.py), as pu_boot_profile: with
 * pu_topotest_profile(device, 1) every pu_topology_tests call records events round the stages of
 * each range; pu_topotest_kernel_ms waits for the last call's and returns the time of its weight
 * launches, of its RELL sums and of its k_topo_counts launches, in ms, summed over the ranges. */
int pu_topotest_profile(int device, int on);
int pu_topotest_kernel_ms(int device, double *weights_ms, double *rell_ms, double *counts_ms);

/* ---- Fitch parsimony (normative) ---------------------------------------------
 * The reference has no parsimony, so there is no reference interface to cite: the rule is
 * DESIGN 4.22's and tests/parsimony_reference.py restates it.  Every result is an integer and
 * does not depend on the launch shape, the summation order or the chunking.
 * The alignment: codes [n_taxa][n_pat] into code_table [n_codes][n_states]; the state set of a
 * code is bit k for every k with code_table[code][k] > 0.  weights [n_pat] are non-negative
 * integers, NULL: all 1.  Node ids: a tip is its alignment row (< n_taxa), the internal nodes
 * are n_taxa .. 2 n_taxa - 3.  A tree is a post-order op list ops [n_taxa - 2][3] = (parent,
 * left, right) and its root edge [2], the two nodes left without a parent; its 2 n_taxa - 3
 * edges in op order are 2 i = (left_i, parent_i), 2 i + 1 = (right_i, parent_i) and, last, the
 * root edge.
 * PU_E_ARG, before any device is touched: a null buffer other than weights and the optional
 * outputs, n_taxa < 3 or > PU_PARS_MAX_TAXA (a workgroup keeps one 64-bit counter per edge in
 * LDS), n_pat < 1, n_states outside [1, 32], n_codes outside [1, 32], a code >= n_codes, a
 * code that allows no state, a negative weight or weights that sum past 2^63 / (2 n_taxa), an
 * op list that is not a post-order of a binary tree over exactly the alignment's rows, an
 * order that is not a permutation, n_trees, n_query or n_rep < 1.
 * The node sets of one launch live in a device workspace of at most 256 MiB, laid out
 * [node][pattern]; a call is cut into chunks of trees (or replicates) and, where one tree
 * alone is larger, of patterns.  PU_PARS_CHUNK=n, read at each call, caps the trees or
 * replicates of a chunk. */
#define PU_PARS_MAX_TAXA 4000
/* The lengths of n_trees trees (ops [n_trees][n_taxa-2][3], root_edges [n_trees][2]) in one
 * launch per chunk: lengths_out [n_trees]; pattern_changes_out [n_trees][n_pat], nullable,
 * the unweighted changes of every pattern; edge_changes_out [n_trees][2 n_taxa - 3], nullable,
 * per edge in op order the weighted count of patterns whose two directional sets are disjoint. */
int pu_fitch_lengths(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                     const uint8_t *codes, const double *code_table, const int64_t *weights,
                     int n_trees, const int32_t *ops, const int32_t *root_edges,
                     uint64_t *lengths_out, uint32_t *pattern_changes_out,
                     uint64_t *edge_changes_out);
/* The exact length of the tree with query row q (query_codes [n_query][n_pat]) attached on
 * edge e, for every q and e: lengths_out [n_query][2 n_taxa - 3], edges in op order.  The edge
 * sets are computed once ([edge][pattern], not chunked); the scoring is a grid over pattern
 * tiles, edges and query tiles. */
int pu_fitch_insert_lengths(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                            const uint8_t *codes, const double *code_table,
                            const int64_t *weights, const int32_t *ops, const int32_t *root_edge,
                            int n_query, const uint8_t *query_codes, uint64_t *lengths_out);
/* Stepwise addition for n_rep addition orders [n_rep][n_taxa], each a permutation of the rows:
 * edges_out [n_rep][2 n_taxa - 3][2] in DESIGN 4.22's numbering, step_lengths_out
 * [n_rep][n_taxa - 2] (entry 0: the three-taxon star) and lengths_out [n_rep], the length of
 * the finished tree scored once more from scratch.  The host drives the steps (one read-back
 * per step: the per-edge sums, then the argmin and the topology update); all replicates of a
 * chunk go through the same launch of a step. */
int pu_parsimony_stepwise(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                          const uint8_t *codes, const double *code_table, const int64_t *weights,
                          int n_rep, const int32_t *orders, int32_t *edges_out,
                          uint64_t *step_lengths_out, uint64_t *lengths_out);
/* ---- Parsimony SPR (normative; tests/parsimony_spr_reference.py restates it) ----
 * A tree is an edge list edges [2 n_taxa - 3][2] in DESIGN 4.22's form, as pu_parsimony_stepwise
 * returns it: tips 0 .. n_taxa - 1, internal nodes n_taxa .. 2 n_taxa - 3, each on exactly
 * three edges.  Prune direction d = 2 e + side prunes the subtree on s's side of edge e, (s, u) =
 * edges[e] for side 0 and reversed for side 1; it is valid iff u is internal.  u's other two
 * edges are ea < eb with far ends a, b; the rest tree T' has the merged edge (a, b) under id ea.
 * Every other edge f of T' is a target, named by its id, at dist(f) = 1 next to the merged edge
 * and one more per edge further away; radius = 0 is no limit, else only dist(f) <= radius.
 *   score[d][f] = L(T) - miss(ea) + miss(f),  miss(g) = sum_p w[p] [D(s->u)(p) & E'(g)(p) = 0]
 * is the exact length of the tree after the move (E'(g): the edge set of g in T', derived from
 * the directional sets of T by a walk outward from the merged edge); every entry that is not a
 * (valid direction, target) pair holds UINT64_MAX.  Applying (d, f), (x, y) = edges[f]:
 * edges[ea] = (a, b), edges[f] = (x, u), edges[eb] = (u, y); edges[e] and all node ids stay.
 * PU_E_ARG: everything pu_fitch_lengths refuses, an edge list that is not a binary tree over
 * the rows, radius < 0, max_rounds < 0.  n_taxa = 3 is valid and has no move.
 * Workspace and scores obey the 256 MiB rule above, chunked over trees, then directions, then
 * patterns (PU_PARS_CHUNK, PU_PARS_WS); PU_PARS_LDS=bytes lowers the LDS the walk's arriving
 * sets may use before they go to the workspace.  No result depends on any of them. */
/* lengths_out [n_trees] = L(T); scores_out [n_trees][2 (2 n_taxa - 3)][2 n_taxa - 3]. */
int pu_fitch_spr_scores(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                        const uint8_t *codes, const double *code_table, const int64_t *weights,
                        int n_trees, const int32_t *edges, int radius, uint64_t *lengths_out,
                        uint64_t *scores_out);
/* The search, per tree: score the tree; best = the smallest score, ties to the lowest d, then
 * the lowest f; stop if there is no target or best >= L; else apply the move, L = best, count a
 * round; stop after max_rounds rounds (0: no limit).  edges_inout [n_trees][2 n_taxa - 3][2]
 * (unchanged when the call fails), lengths_out [n_trees] the final lengths, rounds_out
 * [n_trees]; moves_out, nullable, [n_trees][max_rounds][3] = (d, f, length after), rows past a
 * tree's rounds zero -- refused when non-NULL with max_rounds = 0.  The host drives the
 * rounds: one scoring pass per round for all unconverged trees, three numbers read back per
 * tree and direction chunk (k_spr_argmin), the move applied on the host. */
int pu_parsimony_spr(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                     const uint8_t *codes, const double *code_table, const int64_t *weights,
                     int n_trees, int32_t *edges_inout, int radius, int max_rounds,
                     uint64_t *lengths_out, int32_t *rounds_out, uint64_t *moves_out);
/* Event timing (scripts/time_parsimony.py): with pu_parsimony_profile(device, 1) every call
 * above records events around its launches; pu_parsimony_kernel_ms returns the last call's
 * kernel time in ms, summed over its chunks and steps. */
int pu_parsimony_profile(int device, int on);
int pu_parsimony_kernel_ms(int device, double *ms);

/* ---- Sets of trees: splits, RF matrix, split counts (normative;
 * tests/treeset_reference.py restates it) ----
 * T = n_trees binary trees over the same n tips, tips 0 .. n - 1, internal nodes n .. 2n - 3.
 * Each tree's 2n - 3 edges are numbered in the form's own edge order (below).  The split of an
 * edge is the set of tips on the side of the edge that does not hold tip 0: a bitset of
 * nw = ceil(n / 64) words, tip i at bit i & 63 of word i >> 6.  A split of 1 or n - 1 tips (a
 * pendant edge) is trivial and has no id; every binary tree has exactly n - 3 others, one per
 * internal edge.  The split table U holds the distinct non-trivial splits of all T trees in
 * ascending order as unsigned integers of 64 nw bits, word nw - 1 the most significant; the id
 * of a split is its index in U, and count[u] is the number of trees that hold split u (a tree
 * holds a split at most once).  Two splits are equal only if all nw words are equal: no hash
 * decides equality or order.  RF(a, b) = 2 (n - 3) - 2 |ids(a) & ids(b)|.  n = 3 is valid: no
 * split, U = 0, every RF 0.
 * form selects the encoding of `trees`:
 *   PU_TREES_OPS    ops [T][n-2][3] = (parent, left, right) and roots [T][2], pu_fitch_lengths'
 *                   form; edges 2 i = (left_i, parent_i), 2 i + 1 = (right_i, parent_i), then the
 *                   root edge.
 *   PU_TREES_JOINS  joins [T][n-2][2] and roots [T][2], pu_nj's form: op m is
 *                   (n + m, joins[m][0], joins[m][1]); the edge order is the ops form's.
 *   PU_TREES_EDGES  edges [T][2n-3][2], roots NULL, pu_parsimony_stepwise's form; the edge order
 *                   is the list's own.
 * Outputs: edge_ids_out [T][2n-3], the split id per edge, -1 on a pendant edge; n_unique_out
 * [1] = U; uniq_bits_out (nullable) with room for T (n - 3) rows of nw words, the first U
 * written; uniq_count_out (nullable) with room for T (n - 3), the first U written; rf_out
 * (nullable) [n_rows][T], trees 0 .. n_rows - 1 against all.  A nullable output that is NULL
 * changes no other.
 * PU_E_ARG, before any device is touched: a null trees, edge_ids_out or n_unique_out; null roots
 * with the ops or joins form; n < 3 or n > PU_NJ_MAX_N; n_trees < 1 or T (n - 3) >= 2^31; n_rows
 * outside [0, T]; an unknown form; a tree that is not a binary tree over exactly tips 0 .. n - 1
 * (pu_fitch_lengths' refusals for the ops and joins forms, pu_fitch_spr_scores' for an edge
 * list; the message names the tree).
 * The call is not chunked: the bitsets [T][n-3][nw], the sort's keys and permutations and the
 * id arrays, T (n - 3) (8 nw + 44) bytes and rocPRIM's temporaries, are on the device at once;
 * PU_E_NOMEM where they do not fit, or where the host cannot hold the converted trees. */
#define PU_TREES_OPS 0
#define PU_TREES_JOINS 1
#define PU_TREES_EDGES 2
int pu_treeset_compare(int device, int n, int n_trees, int form, const int32_t *trees,
                       const int32_t *roots, int n_rows, int32_t *edge_ids_out,
                       int64_t *n_unique_out, uint64_t *uniq_bits_out, int32_t *uniq_count_out,
                       int32_t *rf_out);
/* Event timing (scripts/time_treeset.py): with pu_treeset_profile(device, 1) every call above
 * records events between its stages; pu_treeset_kernel_ms returns the last call's times in ms:
 * the split kernel, the ids (sort, scan, table, counts, edge ids) and the RF stage (the
 * per-tree sorted lists and the tile kernel). */
int pu_treeset_profile(int device, int on);
int pu_treeset_kernel_ms(int device, double *splits_ms, double *ids_ms, double *rf_ms);

/* ---- Sets of trees with branch lengths: weighted RF, branch score, path distances, length
 * sums (normative; tests/treedist_reference.py restates it) ----
 * The trees, forms, edge orders, splits and ids are pu_treeset_compare's.  lengths [T][2n-3],
 * fp64, holds every tree's edge lengths in its form's own edge order.  A tree's lengths are
 * indexed by key: pendant key i is the edge at tip i, split key u the edge whose non-trivial
 * split has id u; a key the tree does not hold has length 0.
 *   wRF(a, b)   = sum over keys of |l_a - l_b|; KF2(a, b) = sum over keys of (l_a - l_b)^2 (the
 *                 branch score is its square root, left to the caller).  Sum order of both: the
 *                 pendant keys 0 .. n - 1, then the split keys of a or b in ascending id; one
 *                 serial fp64 sum from 0.0; the square is rounded on its own, then added (no fma).
 *   Path2(a, b) = sum over i < j of (e_a(i, j) - e_b(i, j))^2, e(i, j) the number of edges between
 *                 tips i and j; unsigned 64-bit integers, exact.
 *   WPath2(a, b): the same with p(i, j) in fp64.  Root the tree at tip 0 and let l be the node of
 *                 the path i .. j nearest tip 0 (tip 0 itself for i = 0); h(i -> l) is the sum of
 *                 the edge lengths from tip i up to l, added serially from i's pendant edge (0.0
 *                 for no edge); p(i, j) = h(i -> l) + h(j -> l).  The squares of p_a - p_b are
 *                 rounded on their own and summed over the pairs in row-major order (i, then j)
 *                 by DESIGN 4.17's segment rule: segments of 2048 consecutive pairs added serially
 *                 from 0.0, the segment sums added serially in segment order.
 *   split_len_sum[u] = the lengths of the edges that carry split u, added serially over the trees
 *                 in ascending tree index; tip_len_sum[i] = tip i's pendant lengths likewise.
 * Outputs, all nullable, a NULL one is not computed and changes no other: wrf_out, kf2_out,
 * wpath2_out fp64 [n_rows][T] and path2_out uint64 [n_rows][T], trees 0 .. n_rows - 1 against
 * all; n_unique_out [1] = U; split_len_sum_out with room for T (n - 3), the first U written;
 * tip_len_sum_out [n].  n = 3 is valid: no split keys, three pendant keys, e = 2 for every pair.
 * PU_E_ARG, before any device is touched: everything pu_treeset_compare refuses in its inputs; a
 * null lengths; a length that is negative, NaN or infinite (the message names tree and edge);
 * n_rows outside [0, T].
 * Memory, beside pu_treeset_compare's T (n - 3) (8 nw + 44) bytes, nothing chunked: the keyed
 * lengths and sorted ids T (28 n - 60) bytes; for path2_out or wpath2_out T (2n - 2) 16 bytes of
 * rooted-tree arrays and T ceil4(n (n - 1) / 2) 2 bytes of integer paths (ceil4: rounded up to a
 * multiple of 4); for wpath2_out T n (n - 1) / 2 8 bytes more; the output matrices.  PU_E_NOMEM
 * where they do not fit. */
int pu_treedist(int device, int n, int n_trees, int form, const int32_t *trees,
                const int32_t *roots, const double *lengths, int n_rows, double *wrf_out,
                double *kf2_out, uint64_t *path2_out, double *wpath2_out, int64_t *n_unique_out,
                double *split_len_sum_out, double *tip_len_sum_out);
/* Event timing (scripts/time_treedist.py): with pu_treedist_profile(device, 1) every call above
 * records events between its stages; pu_treedist_kernel_ms returns the last call's times in ms:
 * pu_treeset_compare's stages (splits and ids), the weighted stage (keyed lengths, per-tree sort,
 * the merge kernel, the length sums), the paths per tree (rooting and the pair walk), the
 * integer path reduction and the fp64 path reduction. */
int pu_treedist_profile(int device, int on);
int pu_treedist_kernel_ms(int device, double *ids_ms, double *weighted_ms, double *paths_ms,
                          double *path2_ms, double *wpath2_ms);

/* ---- Site concordance factors (normative; tests/concordance_reference.py
 * restates it) ----
 * The reference has no concordance factors; the rule is this project's own.  The alignment
 * arguments are pu_fitch_lengths'; the tree is an edge list edges [2 n_taxa - 3][2] in DESIGN
 * 4.22's form (tips 0 .. n_taxa - 1 are the alignment's rows, internal nodes n_taxa ..
 * 2 n_taxa - 3), 4 <= n_taxa <= PU_PARS_MAX_TAXA.
 * Edge e = (x, y) is internal iff both ends are internal nodes.  x's other two edges, in
 * increasing edge id, lead away from e to clades A and B, y's to C and D; a clade is the set of
 * tips beyond its edge, in ascending row order.  With Q = n_quartets and m = |A||B||C||D| (64
 * bits): if m <= Q the branch has nq[e] = m quartets, all of them, quartet q the mixed-radix
 * number (ia, ib, ic, id), id fastest, of the tips' indices in their clades; else nq[e] = Q and
 * clade k = 0..3 (A, B, C, D) of quartet q takes the tip at index min(floor(u |X|), |X| - 1) of
 * its clade X, u = philox_u(seed, g = q, c2 = 4 e + k, c3 = 2): Philox4x32-10 as DESIGN 4.10
 * defines u, counter word 3 = 2 (the simulator uses 0, the bootstrap 1).  Tips are drawn with
 * replacement across quartets; quartet q of branch e depends on (seed, e, q, the clades) alone.
 * A pattern p of weight w_p is decisive for a quartet (a, b, c, d) iff the state sets of all four
 * codes are singletons (a gap and every ambiguity code is not); with s the four states,
 *   n1 += w_p where sa = sb, sc = sd, sa != sc   (ab|cd, the branch itself)
 *   n2 += w_p where sa = sc, sb = sd, sa != sb   (ac|bd)
 *   n3 += w_p where sa = sd, sb = sc, sa != sb   (ad|bc)
 * counts_out [2 n_taxa - 3][Q][3] = (n1, n2, n3), nq_out [2 n_taxa - 3], taxa_out (nullable)
 * [2 n_taxa - 3][Q][4] the picks; rows of edges that are not internal and slots q >= nq[e] are
 * zero, their taxa -1.  Every sum is an unsigned 64-bit integer: no result depends on the launch
 * shape, on PU_SCF_FEED or on the chunking.  The finish (sCF = 100 mean(n1 / (n1 + n2 + n3))
 * over the quartets with a decisive pattern, and so on) is the caller's, in float64
 * (phylo_utils_amd/concordance.py).
 * PU_E_ARG, before any device is touched: everything pu_fitch_lengths refuses of the alignment,
 * n_taxa < 4, a null edges, counts_out or nq_out, n_quartets < 1, an edge list that is not a
 * binary tree over the rows (pu_fitch_spr_scores' refusals), and an n_quartets whose counts and
 * picks of one branch alone (40 bytes per quartet) pass half the workspace.
 * The workspace obeys the 256 MiB rule of the parsimony calls (PU_SCF_WS=bytes lowers it): half
 * for the counts and picks of a chunk of branches, half for the state bytes [taxon][pattern]
 * of a chunk of patterns; the call is cut into chunks of branches and, inside each, of
 * patterns.  PU_SCF_CHUNK=n, read at each call, caps the branches of a chunk.  A chunk of
 * patterns is never less than one tile of 2048: a PU_SCF_WS below 2 * 2048 n_taxa bytes is
 * exceeded by that much and no further.
 * PU_SCF_FEED=lds|global, read at each call, selects how k_scf_counts is fed: the pattern tile
 * of all rows staged in LDS (tiles of 2048, 1024 or 512 patterns for n_taxa <= 74, 148 or 296;
 * beyond, as global), or the rows read from memory. */
int pu_scf_counts(int device, int n_taxa, int64_t n_pat, int n_codes, int n_states,
                  const uint8_t *codes, const double *code_table, const int64_t *weights,
                  const int32_t *edges, int n_quartets, uint64_t seed, uint64_t *counts_out,
                  int32_t *nq_out, int32_t *taxa_out);
/* Event timing (scripts/time_concordance.py): with pu_scf_profile(device, 1) the call above
 * records events around its launches; pu_scf_kernel_ms returns the last call's times in ms,
 * summed over its chunks: the pick kernel, the state-byte kernel and k_scf_counts. */
int pu_scf_profile(int device, int on);
int pu_scf_kernel_ms(int device, double *picks_ms, double *states_ms, double *counts_ms);

/* ---- likelihood mapping -------------------------------------------------- */
/* The reference has no likelihood mapping (Strimmer & von Haeseler 1997); the rule is this
 * project's own.  Alignment and model as in pu_pair_distances: codes [n_taxa][n_sites] below
 * n_codes <= 32, rows of code_table [n_codes][K], K in {2, 4, 20}, pattern weights (NULL: 1), a
 * reversible model's eigen-system and 1 <= n_cat <= PU_PAIR_MAX_CAT categories (a zero rate is
 * an ordinary category).  quartets [Q][4] are four distinct taxa (a, b, c, d).  Topology tau has
 * tips (p, q | r, s) = (a, b | c, d), (a, c | b, d), (a, d | b, c) for tau = 0, 1, 2 and lengths
 * (l_p, l_q, l_r, l_s, l_i), l_i the internal edge; with P_c(t) = E diag(e^{lambda r_c t}) E^-1
 *   L_s = sum_c q_c sum_i pi_i (P_c(l_p) x_p)_i (P_c(l_q) x_q)_i
 *                   sum_j P_c(l_i)[i][j] (P_c(l_r) x_r)_j (P_c(l_s) x_s)_j
 *   lnL = sum_s w_s log L_s        (no scaler; w_s > 0 and L_s <= 0 give -inf; w_s >= 0)
 * and derivatives in one length as pu_edge_derivs defines them (the factor r_c included).
 * The optimiser: the start is t0[5] (NULL: 0.1 each) and one evaluation there; a round takes the
 * edges in the order p, q, r, s, i, each by the Newton rule of pu_optimise_edge (tol, max_iter,
 * the bounds 1e-8 and 100) from its current length with the others fixed; after a round it stops
 * at round == max_rounds or, where min_gain >= 0, at lnL_after - lnL_before_round <= min_gain
 * (min_gain < 0: never early); max_rounds = 0 is the one evaluation; a non-finite lnL ends the
 * topology at once.
 * out [Q][3][8] = (lnL, l_p, l_q, l_r, l_s, l_i, rounds, evaluations), the evaluations being the
 * start's and those of the Newton rule; derivs (nullable) [Q][3][5][2] = (lnL', lnL'') in each
 * length at the final lengths, in the order p, q, r, s, i (NaN after a non-finite lnL).
 * Results are bitwise repeatable and do not depend on the chunking of the quartets, on the grid
 * or on the other quartets of the call; no floating-point atomics (DESIGN 4.30 states the order
 * of every sum).
 * Two feeds of the optimiser, PU_LMAP_FEED=bins|patterns read at each call: `patterns` walks the
 * four code rows; `bins` first counts per quartet the weighted 4-tuples of the codes in use in
 * unsigned 64-bit integers and runs over the non-zero bins.  The bins need n_used^4 <= 4096 and
 * non-negative integer weights below 2^53: the host form checks both and takes the patterns
 * otherwise; the device form takes n_codes^4 <= 4096 and, for integer weights, the caller's word:
 * without weights it defaults to the bins, with weights to the patterns unless PU_LMAP_FEED=bins
 * states them integer.  The bins of a chunk of quartets stay within 256 MiB;
 * PU_LMAP_CHUNK=<quartets>, read at each call, lowers the chunk.
 * PU_E_ARG, before any device is touched: a null buffer, n_taxa < 4, n_sites <= 0, n_codes
 * outside [1, 32], n_states not 2, 4 or 20, n_cat outside [1, PU_PAIR_MAX_CAT], tables past the
 * 160 KiB of LDS of one workgroup (8 (2 K^2 + 2 K + 2 C + n K + 6 C n K + C K^2 + 3 C K + 24)
 * bytes, n the codes), Q < 1, a quartet index out of range or repeated within a quartet,
 * tol <= 0, max_iter < 0, max_rounds < 0, a NaN min_gain, a t0 outside [1e-8, 100], and -- host
 * forms -- a code >= n_codes and a weight that is negative or not finite.  The device form
 * cannot look at its buffers: codes below n_codes and weights >= 0 are its preconditions, and
 * the result of a call that breaks them is not defined (the patterns feed gives -inf for a code
 * >= n_codes, the bins feed does not count the pattern). */
int pu_lmap_scores(int device, int n_states, int n_cat, int n_codes, const double *code_table,
                   const double *evecs, const double *evals, const double *ivecs,
                   const double *freqs, const double *rates, const double *cat_weights,
                   const uint8_t *codes, int n_taxa, int64_t n_sites, const double *site_weights,
                   int64_t n_quartets, const int32_t *quartets, const double *t0, double tol,
                   int max_iter, int max_rounds, double min_gain, double *out, double *derivs);
/* The same on device buffers -- the output of pu_simulate_device or pu_compress_patterns_device
 * with no copy: d_codes rows ld bytes apart (ld >= n_sites), d_site_weights (nullable), d_out
 * and d_derivs (nullable) on the device; quartets and the model on the host.  Asynchronous on
 * the caller's stream. */
int pu_lmap_scores_device(int device, void *stream, int n_states, int n_cat, int n_codes,
                          const double *code_table, const double *evecs, const double *evals,
                          const double *ivecs, const double *freqs, const double *rates,
                          const double *cat_weights, const uint8_t *d_codes, int64_t ld,
                          int n_taxa, int64_t n_sites, const double *d_site_weights,
                          int64_t n_quartets, const int32_t *quartets, const double *t0,
                          double tol, int max_iter, int max_rounds, double min_gain,
                          double *d_out, double *d_derivs);
/* The statistic of the bins feed: bins_out [Q][n_used^4], entry ((u_a n_used + u_b) n_used +
 * u_c) n_used + u_d = the sum of the weights of the patterns where the quartet's taxa show the
 * codes used[u_a], used[u_b], used[u_c], used[u_d].  `used` lists n_used ascending codes (NULL:
 * all n_codes).  Exact.  PU_E_ARG as above, and for n_used^4 > 4096, a weight that is no
 * non-negative integer below 2^53, a `used` that is not ascending, and a code outside it. */
int pu_lmap_bins(int device, const uint8_t *codes, int n_taxa, int64_t n_sites, int n_codes,
                 const double *site_weights, int64_t n_quartets, const int32_t *quartets,
                 int n_used, const uint8_t *used, uint64_t *bins_out);
/* The quartets of a mapping, Philox as DESIGN 4.10 defines u, counter word 3 = 3.  Without
 * clusters (cluster NULL), m = C(n_taxa, 4): m <= n_quartets gives all a < b < c < d in
 * lexicographic order; else quartet g draws r_k = min(floor(u_k (n - k)), n - k - 1), u_k =
 * philox_u(seed, g, k, 3), k = 0..3, and its taxon k is r_k raised by one for each earlier taxon
 * of the quartet <= it, those taken in ascending order; (a, b, c, d) is the draw order.  With
 * cluster [n_taxa] in {-1, 0, 1, 2, 3}: a from cluster 0, b from 1, c from 2, d from 3, m the
 * product of the sizes; m <= n_quartets gives all, mixed radix with d fastest over the
 * ascending members; else the member at index min(floor(u |X|), |X| - 1), u = philox_u(seed, g,
 * 4 + k, 3).  quartets_out [min(m, n_quartets)][4] (room for n_quartets), *n_out their number.
 * PU_E_ARG: n_taxa < 4, n_quartets < 1, a null output, a cluster value outside -1..3, an empty
 * cluster. */
int pu_lmap_quartets(int device, int n_taxa, const int32_t *cluster, int64_t n_quartets,
                     uint64_t seed, int32_t *quartets_out, int64_t *n_out);
/* Event timing (scripts/time_lmap.py), as pu_pair_profile / pu_pair_kernel_ms: the bin launches
 * and the optimiser launches of the last pu_lmap_scores* call, summed over its chunks. */
int pu_lmap_profile(int device, int on);
int pu_lmap_kernel_ms(int device, double *bins_ms, double *opt_ms);

/* ---- multi-device / stream interop (site sharding) ------------------- */
/* Launch on the caller's HIP stream (hipStream_t as void*), e.g.
 * torch.cuda.current_stream().cuda_stream, so the RCCL all-reduce of the lnL is
 * stream-ordered after the traversal with no host synchronisation.  NULL is the HIP null
 * stream (torch's default stream: handle 0); PU_OWN_STREAM returns to the context's own
 * non-blocking stream, which is NOT ordered with the null stream. */
#define PU_OWN_STREAM ((void *)(intptr_t)-1)
int pu_ctx_set_stream(pu_ctx *ctx, void *hip_stream);
/* Also write each run's lnL (one double) to this DEVICE pointer (NULL = off); when set,
 * pu_enqueue skips its device->host copy and pu_synchronize reads it from here. */
int pu_set_lnl_device_output(pu_ctx *ctx, double *device_ptr);

/* ---- several trees per launch ------------------------------------
 * Replaces the reference's loop over trees -- set_tree, compute_partials, likelihood per tree
 * (tree_model.py:87-89, 160-176) -- for trees on one alignment (bootstrap replicates,
 * candidate trees: BASELINE cfg5).  A batch evaluates the lnL of n contexts with one P launch,
 * one traversal launch and one reduction for all of them, on the batch's stream; each
 * context keeps its own schedule, branch lengths and buffers, and each tree's lnL and sitewise
 * lnL are bitwise those of pu_enqueue on that context.  Accepted at pu_batch_enqueue (else
 * PU_E_ARG, and pu_enqueue per context is the way): contexts on one device, created with
 * PU_LNL_ONLY, K = 2 or 4, coded tips, the model's eigen-system (no host matrices), no
 * ascertainment correction, equal K, C and S.  The contexts must outlive the batch; work a
 * context queued on its own stream is ordered before the batch's launches, and the batch's
 * results are complete after pu_batch_synchronize (or on the batch's stream). */
typedef struct pu_batch pu_batch;
int pu_batch_create(pu_batch **out, int n, pu_ctx *const *ctxs);
void pu_batch_destroy(pu_batch *b);
const char *pu_batch_last_error(const pu_batch *b);
/* stream of the batch's launches: NULL the HIP null stream, PU_OWN_STREAM its own (default) */
int pu_batch_set_stream(pu_batch *b, void *stream);
/* tree i's lnL into lnl_dev[i] (device memory, n doubles); lnl_dev NULL: into each context's
 * own output (its pu_set_lnl_device_output, or pu_synchronize(ctx, &lnl) after
 * pu_batch_synchronize).  With lnl_dev, pu_synchronize(ctx_i, &lnl) until ctx_i's next own
 * evaluation reads lnl_dev[i] (which must then still be allocated).  Work later queued on a
 * context's own stream is ordered after the batch's launches (an event the stream waits on).
 * Refused (PU_E_ARG): a category count other than 1, 2 or 4.  The root partials are not
 * written (r06: nothing of a batched lnL-only tree reads them): pu_get_root on a context
 * refuses (PU_E_STATE) until its next own pu_enqueue / pu_run. */
int pu_batch_enqueue(pu_batch *b, double *lnl_dev);
int pu_batch_synchronize(pu_batch *b);
/* profiling (bench.py): on = 1 records hipEvents around each enqueue's traversal launch (and
 * its P and reduction launches) from here on; pu_batch_kernel_times returns up to cap
 * per-enqueue times in ms (trav: the traversal launch, total: P + traversal + reduction) */
int pu_batch_profile(pu_batch *b, int on);
int pu_batch_kernel_times(pu_batch *b, double *trav, double *total, int cap, int *n);

/* ---- one process, several devices (SURVEY 8(b) B2 pu_group_create, 8(e) G1) ----------- */
/* One context per device over contiguous pattern shards of an n_patterns alignment (shard
 * sizes differ by at most one) and an RCCL communicator over the devices
 * (ncclCommInitAll).  devices = NULL: 0 .. n_dev-1.  On failure *out is still set for
 * pu_group_last_error and must be destroyed. */
typedef struct pu_group pu_group;
int pu_group_create(pu_group **out, int n_dev, const int *devices, int n_nodes, int n_tips,
                    int64_t n_patterns, int n_cat, int n_states, int flags);
void pu_group_destroy(pu_group *g);
const char *pu_group_last_error(const pu_group *g);
int pu_group_size(const pu_group *g);
/* pattern range [first, first + count) of device i, and its context */
int pu_group_shard(const pu_group *g, int i, int64_t *first, int64_t *count);
pu_ctx *pu_group_ctx(pu_group *g, int i);
/* the pu_set_tips / pu_set_model / pu_set_schedule / pu_set_branch_lengths of every shard;
 * tips, codes and weights are given for all n_patterns and sliced per device */
int pu_group_set_tips(pu_group *g, int n_tips, const int32_t *nodes, int n_codes,
                      const double *code_table, const uint8_t *codes, const double *partials,
                      const double *pattern_weights);
int pu_group_set_model(pu_group *g, const double *evecs, const double *evals,
                       const double *ivecs, const double *freqs, const double *rates,
                       const double *weights);
int pu_group_set_schedule(pu_group *g, int n_ops, const int32_t *ops, const double *brlens,
                          int root_a, int root_b, double root_len);
int pu_group_set_branch_lengths(pu_group *g, const double *brlens, double root_len);
/* pu_set_model_p / pu_set_pmatrices of every shard (the same matrices on every device) */
int pu_group_set_model_p(pu_group *g, const double *freqs, const double *rates,
                         const double *weights);
int pu_group_set_pmatrices(pu_group *g, const double *P);
/* every shard's traversal, then ncclAllReduce(sum) of the per-device lnL on the shards'
 * streams (8 bytes, the only collective); sitewise_out [n_patterns] (nullable) gathers
 * the shards' per-pattern lnL */
int pu_group_run(pu_group *g, double *lnl_out, double *sitewise_out);

/* ---- planner introspection (host only, no device) -------------------------------------- */
/* Run the schedule planner of pu_set_schedule for a tree whose leaves are the nodes no op
 * produces, with L LDS stash slots and R = the split target (PU_SPLIT; 0: one task).
 * stats_out[8] = {n_mem, n_chains, n_lds, n_tip, n_store, max_live, n_cur, n_top}: children
 * read back from HBM, chain tasks of a split plan (0: not split), children from the LDS
 * stash / tips, HBM slots allocated, peak number of values waiting for a later consumer,
 * children taken straight from the previous op's result, ops of the top task. */
int pu_plan_stats(int n_nodes, int n_ops, const int32_t *ops, int root_a, int root_b, int R,
                  int L, int flags, int32_t *stats_out);

/* ---- measurement hooks (bench.py) ----------------------------------------------------- */
/* HIP stream the context launches on (hipStream_t as void*). */
void *pu_ctx_stream(pu_ctx *ctx);
/* Bytes resident on the device for this context. */
int64_t pu_ctx_device_bytes(const pu_ctx *ctx);
/* Device-side Newton (pu_optimise_edge / pu_optimise_sweep, r06): the persistent launches
 * made and the evaluations they ran since the context's edge buffers were set up. */
int pu_ctx_newton_stats(pu_ctx *ctx, int *launches, int *evaluations);
/* The device's write-stream ceiling for a traversal's store stream (r06, bench.py's
 * roofline.ceiling_GBps): hipMemsetAsync of `bytes` into a fresh buffer, `reps` times after 3
 * warm-ups, on a stream of its own; ms_out = the median time (ms).  The fastest write stream
 * measured on this hardware (6.4-6.6 TB/s, against 5.0-5.7 for k_prune-shaped
 * probes), so box-to-box spread shows in it as in the kernel. */
int pu_write_ceiling(int device, int64_t bytes, int reps, double *ms_out);
/* Event timing on the launch stream: with pu_ctx_profile(ctx, 1) every pu_enqueue
 * records events around its kernels (up to 4096 runs); pu_ctx_kernel_ms waits for them
 * and returns the mean time of the traversal launch alone and the mean P + traversal +
 * reduction time (ms) over the recorded runs.  pu_ctx_profile(ctx, 0|1) also clears the
 * record. */
int pu_ctx_profile(pu_ctx *ctx, int enable);
int pu_ctx_kernel_ms(pu_ctx *ctx, double *traverse_ms_avg, double *total_ms_avg, int *n);
/* The per-run times behind pu_ctx_kernel_ms, in launch order: up to `cap` runs into
 * traverse_ms[] (the traversal launch alone) and total_ms[] (P + traversal + reduction);
 * *n = the number written.  bench.py takes medians of these. */
int pu_ctx_kernel_times(pu_ctx *ctx, double *traverse_ms, double *total_ms, int cap, int *n);
/* The traversal's compulsory HBM bytes per launch for the current plan, after a run:
 * out[0] parents written (CLVs of every storing op and the root), out[1] scalers written
 * (in steady state: only the non-zero wave tiles under TV_SKIP_ZERO_SCALE), out[2] tip data
 * read, out[3] parents read back from HBM (stash overflow, CLV + scaler), out[4] sitewise
 * lnL written + pattern weights read.  bench.py checks its PMC traffic against the sum. */
int pu_ctx_traffic(pu_ctx *ctx, int64_t out[5]);
/* The traversal plan of the current schedule (r05): out[10] = {launch grid, k_prune build
 * (1 default, 7 the 7-wave build, -1 chosen at enqueue), kernel variant bits (pu_internal.h
 * TV_*), LDS stash slots, staging chunks, LDS pad bytes, 64-site tiles, blocks, unused tiles
 * per layout row (PU_PITCH_EXTRA), tiles per layout row}. */
int pu_ctx_plan_info(const pu_ctx *ctx, int32_t out[10]);
/* With pu_ctx_profile(ctx, 1), also the mean kernel time of the edge reductions
 * (pu_edge_lnl / pu_edge_derivs / the Newton evaluations of pu_optimise_*), in ms. */
int pu_ctx_edge_kernel_ms(pu_ctx *ctx, double *kernel_ms_avg, int *n);
/* The same, plus the mean time of the k_edge launch alone (before its reduction launch). */
int pu_ctx_edge_kernel_ms2(pu_ctx *ctx, double *kernel_ms_avg, double *edge_ms_avg, int *n);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_H */
