/*
 * ce.h -- C-ABI of the MI355X consensus-entropy query-selection engine (libce_amd.so).
 *
 * The reference (juansgomez87/consensus-entropy) has no plugin/FFI interface: the
 * selection path is ~60 lines of NumPy/SciPy inline in AMG_Tester.run
 * (amg_test.py:425-489).  This header defines the drop-in seam at exactly that
 * place; each entry point names the reference lines it replaces.  The Python
 * mirror of the reference interface (consensus-entropy_amd/ce_amd) binds it with
 * ctypes; INTEGRATION.md shows the binding a maintainer of the reference adds.
 *
 * Conventions (all entry points):
 *   - every pointer is caller-owned DEVICE memory unless stated otherwise;
 *   - every call is stream-ordered on `stream` (a hipStream_t; NULL = legacy
 *     default stream) and asynchronous: nothing is read back to the host;
 *   - nothing allocates: scratch comes from the caller's `ws`, sized by the
 *     matching *_workspace_bytes() function (pure host arithmetic).  A
 *     workspace must be ZERO-FILLED before its first use (e.g. hipMemsetAsync
 *     once after allocating it): its 64 KiB header holds the arrival counters
 *     of the tiled kernels (a block that finishes last merges its problem's
 *     tiles), and every call leaves them zero again, so one workspace serves
 *     any sequence of calls on one stream;
 *   - return 0 (CE_OK) or a negative CE_E* code; ce_last_error() gives a
 *     thread-local message.  Nothing throws across the ABI;
 *   - strides are in ELEMENTS.  Element (n, m, c) of a committee tensor lives at
 *     p[n*sN + m*sM + c*sC]: the reference's member-major stack np.array(pred_prob)
 *     ([M,N,C], amg_test.py:441) is sN=C, sM=N*C, sC=1; the item-major [N,M,C]
 *     tensor is sN=M*C, sM=C, sC=1;
 *   - arithmetic contract (BASELINE.json north_star): inputs are loaded as
 *     f32/f64/bf16 and every sum, mean, normalisation and entropy is computed in
 *     f64 in the reference's order (member-sequential mean, numpy pairwise row
 *     sums, scipy.special.entr);
 *   - selection order: NaN entropies first, then entropy descending, then lowest
 *     index (the reference's argsort()[::-1] with its unspecified tie order
 *     tightened to lowest-index-first; -0.0 == +0.0).  Selected outputs are q
 *     slots, best first; slots beyond the number of candidates hold idx = -1 and
 *     val = NaN;
 *   - q is any integer >= 0, as the reference's -q (amg_test.py:547-553;
 *     argsort()[::-1][:q] returns min(q, N) positions, none for q = 0): q = 0
 *     writes nothing; q <= CE_MAX_Q runs on the list kernels (workspace of a few
 *     KB-MB); a larger q runs on a device radix sort of the pool's order keys
 *     (ce_sort.hpp; its workspace grows with N: ~40 B per item) -- the
 *     *_workspace_bytes functions size either.
 */
#ifndef CE_AMD_CE_H
#define CE_AMD_CE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *ce_stream_t; /* hipStream_t */

typedef enum { CE_F32 = 0, CE_F64 = 1, CE_BF16 = 2 } ce_dtype;

enum {
    CE_OK = 0,
    CE_EINVAL = -1,       /* bad argument (shape, q, stride, null pointer) */
    CE_EWORKSPACE = -2,   /* ws too small */
    CE_ELAUNCH = -3,      /* HIP runtime error on launch */
    CE_EUNSUPPORTED = -4  /* shape outside what this build implements */
};

#define CE_MAX_Q 2048 /* the list kernels' largest q; larger q: the sort path */

const char *ce_last_error(void);
const char *ce_version(void);
/* The main kernel the last selection call on this thread launched, as
 * rocprofv3 names it without "void " and the argument list (e.g.
 * "ce::k_stream_nmc<0, 4, 16, 2, false, 2>"); "" when that call launched none
 * of the noted kernels.  Lets a benchmark tie a profiled figure to the kernel
 * it actually ran.  The ce_*_score_users entry points note their kernel too. */
const char *ce_last_kernel(void);

/*
 * Per-item committee consensus entropy -- replaces amg_test.py:441 + :443:
 *   consensus_prob = np.mean(np.array(pred_prob), axis=0)
 *   ent = scipy.stats.entropy(consensus_prob, axis=1)
 * p: [N items x M members x C classes] via strides; ent: [N] f64 out.
 * mean_or_null: optional [N, C] f64 out (the consensus_prob matrix).
 */
int ce_committee_entropy(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                         int64_t sM, int64_t sC, double *mean_or_null, double *ent,
                         ce_stream_t stream);

/*
 * Human-consensus table -- replaces amg_test.py:109-117 (+ :451's entropy):
 *   per row, count votes per class (votes[n*ld + a] in [0, C) is a vote, any
 *   other value e.g. -1 is missing), freq = np.round(count / n_votes, 3),
 *   ent = scipy.stats.entropy(freq).  A row with no vote gives NaN.
 * votes: [N, A] int8 with row stride ld (bytes).  freq_or_null: [N, C] f64 out.
 * C in [1, 8].  N = 0 does nothing; A = 0 reads no vote (every row NaN), so
 * votes may be NULL there.
 */
int ce_vote_entropy(const int8_t *votes, int64_t N, int32_t A, int32_t C, int64_t ld,
                    double *freq_or_null, double *ent, ce_stream_t stream);

/*
 * Same as ce_vote_entropy from the raw AMG1608 annotation array
 * (amg_test.py:88-106): va[(n*A + a)*2 + 0] = valence, [.. + 1] = arousal, f64,
 * NaN = missing (dropped as dropna() at :101); quadrant rule of :69-78; C = 4.
 */
int ce_va_entropy(const double *va, int64_t N, int32_t A, double *freq_or_null, double *ent,
                  ce_stream_t stream);

/*
 * Frame -> song segment mean of one committee member -- replaces
 *   pd.DataFrame(y_probs, index=X_train.index).groupby(['s_id']).mean()
 * (amg_test.py:437, :469) with pandas 1.1.5 group_mean semantics (the
 * reference pins pandas==1.1.5): per (song, class) an f64 sequential sum over
 * the song's frames in row order, NaN skipped, divided by the non-NaN count
 * (no frame -> NaN); float32 input gives the float32-rounded mean.
 * frames: [F, C] (dt F32|F64, row stride ld elements).  Song n owns the rows
 * perm[offsets[n]] .. perm[offsets[n+1]-1] (perm_or_null == NULL: rows
 * offsets[n] .. offsets[n+1]-1), in their original order; songs are in sorted
 * s_id order as groupby returns them.  out: [N, C] (out_dt F32|F64, row stride
 * ld_out) -- e.g. member m's slice of an [M, N, C] committee stack.
 */
int ce_segment_mean(const void *frames, ce_dtype dt, int64_t F, int32_t C, int64_t ld,
                    const int64_t *perm_or_null, const int64_t *offsets, int64_t N, void *out,
                    ce_dtype out_dt, int64_t ld_out, ce_stream_t stream);

/*
 * Frames -> committee entropy -> top-q in ONE pass --
 * replaces amg_test.py:426-445 from the members' FRAME-level outputs on: per
 * member, pd.DataFrame(y_probs, index=X_train.index).groupby(['s_id']).mean()
 * (:437; pandas 1.1.5 group_mean, as ce_segment_mean), then
 * np.mean(np.array(pred_prob), 0), scipy.stats.entropy and argsort[::-1][:q]
 * (:441-445) -- without materialising the [M, N, C] stack.
 * members: HOST array of M (<= 32) descriptors, in mod_list order; a member is
 * frame-level (rows of X_train: song n owns rows perm[offsets[n]] ..
 * perm[offsets[n+1]-1], perm_or_null == NULL: offsets[n] .. offsets[n+1]-1)
 * or song-level (song_level != 0: row n, e.g. the CNN member, :430-433).
 * Every member is f32/f64 [*, C] with row stride ld; a float32 member's song
 * means are rounded to float32 (the groupby result keeps the dtype) and the
 * stack is accumulated in f64 (north star: fp32 load, fp64 accumulate).
 * C in {2, 3, 4, 8}; any q (q <= 64 in one pass; larger q through the per-song
 * entropies); output as ce_select_mc (positions base_idx + n of the sorted songs).
 */
typedef struct {
    const void *p;
    int32_t dtype;      /* CE_F32 | CE_F64 */
    int32_t song_level; /* 0: frame rows, 1: one row per song */
    int64_t ld;         /* row stride, elements */
} ce_member;

size_t ce_select_frames_workspace_bytes(int64_t N, int32_t q);
int ce_select_frames(const ce_member *members, int32_t M, int32_t C, const int64_t *offsets,
                     const int64_t *perm_or_null, int64_t N, int32_t q, int64_t base_idx, void *ws,
                     size_t ws_bytes, double *val_out, int64_t *idx_out, ce_stream_t stream);

/*
 * The same pass for a multi-epoch session (SURVEY.md §8(f)3 over §8(f)1) --
 * replaces amg_test.py:425-447 of every epoch after the first, where the
 * reference predicts on the frame rows of what is LEFT of X_train (:521-531
 * removed the queried songs): the full pool stays on the device and the
 * exclusion bitmap is tested inside the frames kernels.  excl: ce_excl_words(N)
 * words, the layout of ce_select_mc_excl -- bit n of word n / 32 set = song n
 * (its position in sorted s_id order, WITHOUT base_idx) is already queried.
 * An excluded song reads no frame row, no perm entry and no song-level row and
 * is never selected; slots past the remaining songs are padding (idx -1, val
 * NaN).  A song's mean depends on its own frames only and sorted order
 * survives a subset, so the selection equals the reference's groupby on the
 * shrunken X_train.  Any q, the routes and the workspace
 * (ce_select_frames_workspace_bytes) of ce_select_frames.  excl == NULL with
 * N > 0 is CE_EINVAL.
 */
int ce_select_frames_excl(const ce_member *members, int32_t M, int32_t C, const int64_t *offsets,
                          const int64_t *perm_or_null, int64_t N, const uint32_t *excl, int32_t q,
                          int64_t base_idx, void *ws, size_t ws_bytes, double *val_out,
                          int64_t *idx_out, ce_stream_t stream);

/*
 * The committee mean itself from frame-level members -- replaces
 * amg_test.py:426-441 (:458-471 in the mix branch): the groupby means of
 * :437 / :469 and consensus_prob = np.mean(np.array(pred_prob), axis=0), as
 * f64 rows out[n * ld_out + c] (ld_out >= C), without the [M, N, C] stack.
 * It feeds the selections that need more than one global top-q (ce_select_mix,
 * ce_select_batched_excl, ce_select_batched_mix) as a one-member f64 committee:
 * (+0.0 + x) / 1 is x, so those selections stay the reference's.  Members and
 * C as ce_select_frames.  excl_or_null: rows of excluded songs are NOT written
 * (the caller's buffer keeps what it held) and their frames are not read.  No
 * workspace.
 */
int ce_frames_consensus(const ce_member *members, int32_t M, int32_t C, const int64_t *offsets,
                        const int64_t *perm_or_null, int64_t N, const uint32_t *excl_or_null,
                        double *out, int64_t ld_out, ce_stream_t stream);

/*
 * Committee member inference on the device -- the
 * predict_proba of the reference's linear members (amg_test.py:435, :467;
 * deam_classifier.py:211-218) over frames X [F, D] f64 (row stride ld),
 * written to out [F, C] f64 (row stride ld_out), e.g. the input of
 * ce_segment_mean.  D <= 512 features (the reference: 260; GaussianNB needs
 * D >= 8, CE_EUNSUPPORTED below), C <= 8 classes.
 *   ce_gnb_predict_proba  GaussianNB (sklearn 0.24.1): theta / var [C, D]
 *                         (theta_, sigma_), log_prior [C] = log(class_prior_);
 *                         numpy's pairwise sums over features, scipy's logsumexp
 *   ce_sgd_predict_proba  SGDClassifier(loss='log'): coef [K, D], intercept [K];
 *                         expit(X coef^T + b), OvR-normalised for K = C > 2,
 *                         [1-p, p] for a binary model (K = 1, C = 2)
 */
int ce_gnb_predict_proba(const double *X, int64_t F, int32_t D, int64_t ld, const double *theta,
                         const double *var, const double *log_prior, int32_t C, double *out,
                         int64_t ld_out, ce_stream_t stream);
int ce_sgd_predict_proba(const double *X, int64_t F, int32_t D, int64_t ld, const double *coef,
                         const double *intercept, int32_t K, int32_t C, double *out, int64_t ld_out,
                         ce_stream_t stream);

/*
 * The users form of the two entry points above: after the
 * partial_fit entry points below every user has a model of their own, and one
 * launch predicts every frame row with the model of the user who owns it.
 * theta / var [U, C, D], log_prior [U, C] (coef [U, K, D], intercept [U, K]):
 * model u's parameters at u * C * D (u * K * D).  The geometry is the
 * sessions': stacked song g owns the CSR positions frame_offsets[g] ..
 * frame_offsets[g+1], position p being row frame_perm[p] of X (row p when
 * frame_perm is NULL); user u owns the stacked songs item_offsets[u] ..
 * item_offsets[u+1] (DEVICE arrays, [T + 1], [>= frame_offsets[T]], [U + 1];
 * non-decreasing offsets, item_offsets[U] <= T).  A row of X that no song owns
 * is not touched in out; a position whose row is outside [0, F) is skipped
 * (neither read nor written).  excl_or_null: an exclusion bitmap over the T
 * stacked songs (ce_excl_words(T) words): the rows of an excluded song are
 * never written, and their frames are not read where eight consecutive
 * positions are excluded.  Per row the arithmetic is that of the one-model
 * entry points, bit for bit.  Shapes as there (GaussianNB: D >= 8); U >= 1;
 * F == 0 launches nothing.  One launch, no workspace, nothing synchronised.
 */
int ce_gnb_predict_proba_users(const double *X, int64_t F, int32_t D, int64_t ld, const double *theta,
                               const double *var, const double *log_prior, int32_t C, int32_t U,
                               const int64_t *item_offsets, const int64_t *frame_offsets,
                               const int64_t *frame_perm_or_null, const uint32_t *excl_or_null,
                               double *out, int64_t ld_out, ce_stream_t stream);
int ce_sgd_predict_proba_users(const double *X, int64_t F, int32_t D, int64_t ld, const double *coef,
                               const double *intercept, int32_t K, int32_t C, int32_t U,
                               const int64_t *item_offsets, const int64_t *frame_offsets,
                               const int64_t *frame_perm_or_null, const uint32_t *excl_or_null,
                               double *out, int64_t ld_out, ce_stream_t stream);

/*
 * GaussianNB.partial_fit on the device -- replaces
 * amg_test.py:509, mod.partial_fit(X_batch.values, y_batch_enc), the retrain
 * step of an epoch, for U already-fitted models (priors=None) in one launch,
 * one workgroup per model.  Model u's batch is the rows
 * rows[row_offsets[u] .. row_offsets[u+1]) of X [F, D] f64 (row stride ld),
 * row i of class labels[i]; theta / var [U, C, D] and class_count [U, C] are
 * updated IN PLACE, class_prior [U, C] and epsilon [U] are written.  sklearn's
 * steps, operation for operation (read from sklearn 1.7.2; parity with the
 * reference's pinned 0.24.1, where var_ is sigma_, is unpinned):
 *   1. epsilon = var_smoothing * np.var(X_batch, axis=0).max(), over the whole
 *      batch (NaN if any cell of it is);
 *   2. var -= epsilon (the NEW batch's epsilon, as sklearn does);
 *   3. per class c in the batch, new_mu = np.mean(X_c, 0), new_var =
 *      np.var(X_c, 0) (rows summed one after the other in the order given,
 *      onto +0.0; true divides, no FMA): taken as they are when
 *      class_count[c] == 0, else merged (_update_mean_variance):
 *        total_mu  = (n_new * new_mu + n_past * mu) / n_total
 *        total_var = ((n_past * var + n_new * new_var)
 *                     + (n_new * n_past / n_total) * (mu - new_mu)**2) / n_total
 *      and class_count[c] += n_new; a class absent from the batch keeps theta
 *      and class_count, its var still goes through - epsilon + epsilon;
 *   4. var += epsilon;
 *   5. class_prior = class_count / class_count.sum() (whole numbers: exact in any order).
 * Bit-identical to sklearn for 2 <= D <= 512 and 2 <= C <= 8; D = 1 is
 * CE_EUNSUPPORTED (numpy sums a single column pairwise, not row by row).
 * A model with an empty batch is left untouched, its epsilon and class_prior
 * slots included.  Preconditions (not checked on the device): every row in
 * [0, F), every label in [0, C), and the rows of a batch in the order of
 * X_train (ascending frame row: X_train[X_train.index.isin(q_songs)], :491) --
 * the sums follow the order given.  rows, labels, row_offsets [U + 1]: DEVICE
 * memory.  No workspace, no allocation; stream-ordered and capturable.
 */
int ce_gnb_partial_fit(const double *X, int64_t F, int32_t D, int64_t ld, const int64_t *rows,
                       const int32_t *labels, const int64_t *row_offsets, int32_t U, int32_t C,
                       double var_smoothing, double *theta, double *var, double *class_count,
                       double *class_prior, double *epsilon, ce_stream_t stream);

/*
 * SGDClassifier.partial_fit on the device -- replaces
 * amg_test.py:509, mod.partial_fit(X_batch.values, y_batch_enc), for the
 * reference's 'classifier_sgd' member (deam_classifier.py:214-217: loss='log',
 * penalty='l2', learning_rate='optimal', fit_intercept, shuffle, no averaging,
 * no class or sample weights), U models in one launch, one workgroup per model,
 * one wave per binary problem.  Model u's batch is the rows
 * rows[row_offsets[u] .. row_offsets[u+1]) of X [F, D] f64 (row stride ld),
 * row i of class labels[i]; coef [U, K, D], intercept [U, K] and t [U] (f64:
 * coef_, intercept_, t_) are updated IN PLACE.  K = C one-vs-rest problems for
 * C > 2 (problem k: class k positive), K = 1 for C = 2 (class 1 positive), as
 * in ce_sgd_predict_proba.  One epoch of sklearn's _plain_sgd64 per problem,
 * operation for operation (read from sklearn 1.7.2):
 *   1. the visiting order: the identity over the model's n rows, then for i in
 *      0 .. n-2: j = i + our_rand_r(&seed) % (n - i), swap ind[i], ind[j];
 *      our_rand_r is the xorshift (13, 17, 5) on a uint32 (0 becomes 1), taken
 *      modulo 2^31.  seed = shuffle_seeds[u * K + k] (DEVICE memory), which the
 *      host derives from random_state (ce_amd.ops.sgd_chain_seeds): the K
 *      problems visit the same batch in K different orders;
 *   2. per visited row x of class y (1.0 if positive, else 0.0), with wscale = 1
 *      at the start and t = the model's t at entry:
 *        p = (sum_j w[j] * x[j]) * wscale + b, the products added one after the
 *            other in feature order onto +0.0 (no FMA, no pairwise sum);
 *        eta = 1 / (alpha * (optimal_init + t - 1)); optimal_init is the host
 *            constant of learning_rate='optimal' (ce_amd.ops.sgd_optimal_init);
 *        g = the gradient: grad 0 (sklearn >= 1.x, cgradient_half_binomial):
 *            p > -37 ? ((1 - y) - y * exp(-p)) / (1 + exp(-p)) : exp(p) - y;
 *            grad 1 (sklearn 0.24.1, Log.dloss on labels ys = +-1, z = p * ys):
 *            z > 18 ? exp(-z) * -ys : z < -18 ? -ys : -ys / (exp(z) + 1);
 *            exp is glibc's; g is clipped to +-1e12; update = -eta * g;
 *        wscale *= max(0, 1 - eta * alpha); if wscale < 1e-9: w *= wscale,
 *            wscale = 1 (before the add);
 *        if update != 0: w += x * (update / wscale), b += update;
 *        t += 1;
 *   3. w *= wscale after the last row; the model's t += n, once per model.
 * Bit-identical to sklearn 1.7.2 with grad 0 for 1 <= D <= 512, 2 <= C <= 8;
 * parity of grad 1 with the reference's pinned 0.24.1 is unpinned.  A model
 * with an empty batch is left untouched, its t included.
 * status [U] int32 is only ever SET: to 1 where a model's intercept or any
 * weight is non-finite after the update (where sklearn raises ValueError; the
 * parameters are left as the arithmetic produced them), to 2 where a model
 * was not run (a batch of 2^31 rows or more, or one whose permutations need a
 * workspace the call did not get); zero it before the call.
 * The K permutations of a model stay in shared memory while K * n <= 8192;
 * a larger batch keeps them in `workspace` (4-byte aligned, may be NULL when no
 * batch is that large), ce_sgd_partial_fit_workspace_bytes(R, C) bytes for R
 * rows in all (0: no batch can need it).  Preconditions as ce_gnb_partial_fit:
 * every row in [0, F), every label in [0, C), row order = X_train's (the
 * shuffle starts from the order given).  rows, labels, row_offsets [U + 1],
 * shuffle_seeds: DEVICE memory.  Bad shapes, alpha or optimal_init not positive
 * and finite, an unknown grad or a null pointer: CE_EINVAL; D > 512 or C > 8:
 * CE_EUNSUPPORTED -- before any launch.  No allocation; stream-ordered and
 * capturable.
 */
size_t ce_sgd_partial_fit_workspace_bytes(int64_t R, int32_t C);
int ce_sgd_partial_fit(const double *X, int64_t F, int32_t D, int64_t ld, const int64_t *rows,
                       const int32_t *labels, const int64_t *row_offsets, int32_t U, int32_t C,
                       double alpha, double optimal_init, const uint32_t *shuffle_seeds, int32_t grad,
                       double *coef, double *intercept, double *t, int32_t *status, void *workspace,
                       size_t workspace_bytes, ce_stream_t stream);

/*
 * The evaluate step of an epoch for the linear members --
 * replaces amg_test.py:513-515 (and :411-413 before epoch 0) for U models in
 * one launch per member:
 *   this_mod_pred = mod.predict(X_test.values)
 *   f1_score(y_test_enc.values, this_mod_pred, average='weighted')
 * ce_*_score_users label every TEST frame row with the model of the user who
 * owns it and count (true class, predicted class) per user.  Models as in
 * ce_*_predict_proba_users (theta / var [U, C, D], log_prior [U, C]; coef
 * [U, K, D], intercept [U, K]); the geometry is theirs too, here over the test
 * songs of every user: item_offsets [U + 1], frame_offsets [T + 1],
 * frame_perm_or_null, excl_or_null, with the same skips (a position whose row
 * is outside [0, F), the rows of an excluded song).  Per row the scores are the
 * ones the predict_proba kernels form, bit for bit: GaussianNB the joint
 * log-likelihood jll[c] (before the logsumexp), SGD the decision value
 * x . coef_c + intercept_c (before expit).  The predicted class is sklearn's:
 * np.argmax over the C scores (the FIRST maximum; a NaN wins at its first
 * occurrence), and for a binary SGD model (K = 1) score > 0 ? 1 : 0 (NaN: 0) --
 * not the argmax of the rounded probabilities.
 *   y               [F] int32 by ROW of X: the encoded class 0 .. C-1.  A row
 *                   whose label is outside [0, C) is not counted and nothing
 *                   is written for it.
 *   cm              [U, C, C] int64, cm[u, y, pred] = counted rows of user u.
 *                   ZERO-FILLED by the entry point with one stream-ordered
 *                   memset before the launch (under stream capture: one memset
 *                   node), then added to with integer atomics: the same on
 *                   every run.
 *   pred_or_null    [F] int32 by row of X; rows that are not owned, excluded,
 *                   out of range or whose label is are not written.
 *   scores_or_null  [F, C] f64, row pitch ld_scores (>= C; >= 1 for a binary
 *                   SGD model, which writes column 0 only); the same rows.
 * Shapes and refusals as ce_*_predict_proba_users (GaussianNB: 8 <= D <= 512;
 * SGD: 1 <= D <= 512), 2 <= C <= 8, U >= 1; y or cm NULL: CE_EINVAL.  F == 0
 * zero-fills cm and launches nothing.  No workspace, nothing synchronised.
 * ce_last_kernel() names the score kernel launched ("" when none was).
 *
 * ce_f1_weighted_users: cm [U, C, C] -> f1 [U] f64, sklearn 1.7.2's
 * f1_score(average='weighted') restated (bit-identical; parity with the
 * reference's pinned 0.24.1, which forms 2pr/(p+r), is unpinned):
 *   true_c = sum_p cm[c, p], pred_c = sum_y cm[y, c], tp_c = cm[c, c];
 *   class c is present iff true_c + pred_c > 0 (unique_labels(y_true, y_pred));
 *   f_c = (2.0 * tp_c) / ((double)true_c + (double)pred_c);
 *   s = the sum of f_c * true_c over the present classes in ascending c, added
 *       one after the other onto 0.0 for fewer than 8 terms, by numpy's tree
 *       ((t0+t1)+(t2+t3)) + ((t4+t5)+(t6+t7)) for 8;
 *   f1 = s / sum_c true_c.
 * A user without a counted row gets NaN (sklearn has no value there).
 * prf_or_null [U, C, 4] f64: precision tp_c/pred_c, recall tp_c/true_c, f_c
 * and the support true_c of every class (classification_report, :514), 0.0 on
 * a zero denominator and for an absent class.  U >= 1, 2 <= C <= 8.
 */
int ce_gnb_score_users(const double *X, int64_t F, int32_t D, int64_t ld, const double *theta,
                       const double *var, const double *log_prior, int32_t C, int32_t U,
                       const int64_t *item_offsets, const int64_t *frame_offsets,
                       const int64_t *frame_perm_or_null, const uint32_t *excl_or_null,
                       const int32_t *y, int64_t *cm, int32_t *pred_or_null, double *scores_or_null,
                       int64_t ld_scores, ce_stream_t stream);
int ce_sgd_score_users(const double *X, int64_t F, int32_t D, int64_t ld, const double *coef,
                       const double *intercept, int32_t K, int32_t C, int32_t U,
                       const int64_t *item_offsets, const int64_t *frame_offsets,
                       const int64_t *frame_perm_or_null, const uint32_t *excl_or_null,
                       const int32_t *y, int64_t *cm, int32_t *pred_or_null, double *scores_or_null,
                       int64_t ld_scores, ce_stream_t stream);
int ce_f1_weighted_users(const int64_t *cm, int32_t U, int32_t C, double *f1, double *prf_or_null,
                         ce_stream_t stream);

/*
 * XGBClassifier.predict_proba on the device (the
 * 'classifier_xgb' member; amg_test.py:435/:467 -> xgboost/sklearn.py:991-1029
 * -> libxgboost 1.3.3 CPU predictor, restated in csrc/ce_xgb.hpp and
 * csrc/ce_xgb_walk.hpp; csrc/ce_xgb.hip holds these entries).
 * X [F, D] (x_dt F32|F64, row stride ld; cast to float32 like DMatrix, NaN =
 * missing), D <= 512.  The forest is packed by ce_amd.xgb.XgbForest: every tree
 * padded to a perfect tree of depth `depth` (<= 10), stored group-major --
 * group g owns trees [group_offsets[g], group_offsets[g+1]) in model order:
 *   nodes  [T][2^depth - 1][2] u32 {feature | default_left << 31, split_cond bits}
 *   leaves [T][2^depth] f32
 * Every feature index must be < D.  G = C groups -> multi:softprob (softmax),
 * G = 1 and C = 2 -> binary:logistic ([1 - p, p]); C <= 8.  base_margin is the
 * margin every group starts from (base_score for softprob, -logf(1/b - 1) for
 * logistic).  out [F, C] (out_dt F32 = what xgboost returns, F64 = its exact
 * upcast, e.g. a committee stack), row stride ld_out.  Bit-identical to the
 * restated predictor, including glibc's expf in the softmax.
 *   ce_xgb_lds_bytes  dynamic LDS one block uses (host arithmetic)
 *   ce_xgb_expf       the restated glibc expf over x [n] -> y [n] (verification)
 * Forests of depth <= 5 (the reference's XGBClassifier(max_depth=5)) run
 * faster from prebuilt lane tables: ce_xgb_lane_table turns (nodes, leaves)
 * of T trees into table [2][T][64][2] u32 (T * 1024 bytes, device memory) for
 * X with D columns, once per forest; ce_xgb_predict_proba_lanes then takes the
 * table and T in place of nodes / leaves and must be given the same D.  Same
 * results as ce_xgb_predict_proba, bit for bit.
 */
int ce_xgb_predict_proba(const void *X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                         const uint32_t *nodes, const float *leaves, const int32_t *group_offsets,
                         int32_t G, int32_t depth, float base_margin, int32_t C, void *out,
                         ce_dtype out_dt, int64_t ld_out, ce_stream_t stream);
int ce_xgb_lane_table(const uint32_t *nodes, const float *leaves, int32_t T, int32_t depth, int32_t D,
                      uint32_t *table, ce_stream_t stream);
int ce_xgb_predict_proba_lanes(const void *X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                               const uint32_t *table, int32_t T, const int32_t *group_offsets, int32_t G,
                               int32_t depth, float base_margin, int32_t C, void *out, ce_dtype out_dt,
                               int64_t ld_out, ce_stream_t stream);
size_t ce_xgb_lds_bytes(int32_t D, int32_t G);
int ce_xgb_expf(const float *x, int64_t n, float *y, ce_stream_t stream);

/*
 * The users form of the XGBoost member (SURVEY.md §8(f)5b / 5c;
 * csrc/ce_xgb_users.hpp, entries in csrc/ce_xgb_users.hip): after epoch 0 every
 * user's forest is the shared pretrained trees plus the rounds that user's own
 * mod.fit(xgb_model=) appended (amg_test.py:507; ce_xgb_fit_users grows them),
 * and one launch has every frame row of X predicted by the forest of the user
 * who owns it.  Depth <= 5 only (lane tables).
 *   table         [2][TT][64][2] u32: TT perfect trees of one common `depth`,
 *                 built by ce_xgb_lane_table for X with D columns -- the shared
 *                 base trees once, then every user's own trees
 *   tree_ids      [L] int32: the row of `table` of every logical tree
 *   group_offsets [U * G + 1] int32, a CSR over tree_ids: user u's group g owns
 *                 tree_ids[group_offsets[u G + g] .. group_offsets[u G + g + 1]),
 *                 in the order the reference adds them to preds[g] (the base
 *                 model's trees of group g in model order, then the user's
 *                 appended ones); a group may own no tree (the base margin)
 * base_margin, G, C, D and depth are common to all users.  The geometry
 * (item_offsets [U + 1], frame_offsets, frame_perm_or_null, excl_or_null) is
 * that of ce_gnb_predict_proba_users: a position whose row is outside [0, F)
 * is neither read nor written, the rows of an excluded song are never written
 * (a 64-frame tile without a row to write is skipped before its loads), a row
 * no song owns is not touched.  out [F, C] out_dt F32 | F64 (the exact upcast),
 * row stride ld_out.  Per row the bits are ce_xgb_predict_proba_lanes' with
 * that user's forest.
 * ce_xgb_score_users: the evaluate step (amg_test.py:513) -- the same float32
 * probabilities, labelled by XGBClassifier.predict's rule
 * (xgboost/sklearn.py:981-985: np.argmax of the PROBABILITIES for
 * multi:softprob, the first maximum, a NaN at its first occurrence; p > 0.5 for
 * binary:logistic) and counted in cm [U, C, C] int64 (zero-filled here by one
 * stream-ordered memset), cm[u, y, pred]; y [F] by ROW of X, a label outside
 * [0, C) is not counted and nothing is written for that row.  pred_or_null
 * [F] int32 and proba_or_null [F, C] f32 (row stride ld_proba) by row of X.
 * ce_f1_weighted_users turns cm into every user's weighted F1.
 * CE_EINVAL: bad shapes, G / C other than G == C or (G == 1, C == 2), dtypes
 * other than F32 / F64, a null pointer with F > 0, U < 1, L < 0;
 * CE_EUNSUPPORTED: depth > 5.  F == 0 launches nothing (cm is zero-filled).
 * Preconditions, checked in the debug build alone: ids in [0, TT), offsets
 * non-decreasing and <= L, table built for this D.  One launch (and the
 * memset), no workspace, nothing read back: capturable.  ce_last_kernel()
 * names the kernel launched.
 */
int ce_xgb_predict_proba_users(const void *X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld,
                               const uint32_t *table, int32_t TT, const int32_t *tree_ids, int64_t L,
                               const int32_t *group_offsets, int32_t G, int32_t depth, float base_margin,
                               int32_t C, int32_t U, const int64_t *item_offsets, const int64_t *frame_offsets,
                               const int64_t *frame_perm_or_null, const uint32_t *excl_or_null, void *out,
                               ce_dtype out_dt, int64_t ld_out, ce_stream_t stream);
int ce_xgb_score_users(const void *X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld, const uint32_t *table,
                       int32_t TT, const int32_t *tree_ids, int64_t L, const int32_t *group_offsets, int32_t G,
                       int32_t depth, float base_margin, int32_t C, int32_t U, const int64_t *item_offsets,
                       const int64_t *frame_offsets, const int64_t *frame_perm_or_null,
                       const uint32_t *excl_or_null, const int32_t *y, int64_t *cm, int32_t *pred_or_null,
                       float *proba_or_null, int64_t ld_proba, ce_stream_t stream);

/*
 * The XGBoost member's refit on the device (csrc/ce_xgb_fit.hpp, entries in
 * csrc/ce_xgb_fit.hip) -- replaces amg_test.py:507 for U users in one call:
 *   mod.fit(X_batch.values, y_batch_enc, xgb_model=mod.get_booster())
 * `rounds` boosting rounds of XGBClassifier(max_depth) are grown on every
 * user's batch on top of that user's current forest: objective multi:softprob,
 * tree_method exact (grow_colmaker on dense columns, one thread), gamma = alpha
 * = 0, max_delta_step 0, no subsampling, no sample weights.  xgboost's C++ core
 * is in no image of this project: the arithmetic below, restated row by row in
 * tests/xgb_fit_ref.py, is the contract (matched bit for bit); parity with
 * xgboost 1.3.3 itself is unpinned.
 *   batch      user u's rows are rows[row_offsets[u] .. row_offsets[u + 1]) of
 *              X [F, D] (x_dt F32 | F64, cast to float32 like DMatrix), of class
 *              labels[i] in [0, G); R = row_offsets[U] rows in all, none of a
 *              user more than n_max (HOST numbers).  DEVICE memory.
 *   forests    table, TT, tree_ids, L, group_offsets, G, depth, base_margin: the
 *              users' current stacked forests, as ce_xgb_predict_proba_users
 *              takes them (G = C groups).
 *   margins    m[i][k], float32: base_margin plus the leaves of the user's trees
 *              of group k, by the users walk itself;
 *   per round  every row's G gradients from the round's starting margins:
 *              p = Softmax(m[i]) (fmaxf, glibc expf, a double wsum, / (float)
 *              wsum), g = p[k] - (y == k), h = fmaxf(2.0f * p * (1.0f - p), 1e-16f);
 *              then G trees, tree k from its own (g, h):
 *   node       G, H: double sums of the float g, h over its rows in batch order;
 *              weight = (float)(-G / (H + lambda)), root_gain = (float)(G * G /
 *              (H + lambda));
 *   search     per level, per feature in feature order, the rows sorted by the
 *              feature ascending (stable by batch position) and scanned from
 *              the high end; every open node keeps e = {double G, H; float last}.
 *              For a row of node nid with value fv: when the node has seen a
 *              row, fv != e.last and e.H >= min_child_weight, c = node - e and,
 *              when c.H >= min_child_weight, loss_chg = (float)(gain(c) + gain(e)
 *              - root_gain), gain(s) = s.G * s.G / (s.H + lambda) in double; the
 *              candidate (loss_chg, f, (fv + e.last) * 0.5f) has c left, e
 *              right.  Then the row is added to e and e.last = fv.  A candidate
 *              replaces the node's best only when its loss_chg is finite and
 *              strictly greater (the best starts at 0): the lower feature wins
 *              an exact tie, within a feature the first of the scan.
 *   expand     open nodes in id order: best loss_chg > 1e-6f splits the node
 *              (children take the next two ids, left then right; rows with
 *              x < cond go left; default_left set); otherwise, and for every
 *              node still open after max_depth levels, a leaf of weight * eta;
 *   update     m[i][k] += the leaf of the row, in float.
 * Outputs, for tree (u * rounds + r) * G + k (round r, group k of user u), T =
 * U * rounds * G slots in all -- a user without rows, or one flagged in
 * status, leaves its slots unwritten:
 *   nodes_out  [T][max(2^depth - 1, 1)][2] u32, leaves_out [T][2^depth] f32: the
 *              packed perfect-tree form ce_xgb_lane_table reads, at the stack's
 *              common `depth` (>= max_depth);
 *   left_out, right_out, split_out [T][63] int32, cond_out [T][63] f32 (the leaf
 *              value at a leaf), default_left_out [T][63] u8, num_nodes_out [T]:
 *              the model's own node arrays (entries past num_nodes: -1, -1, 0,
 *              0.0, 0);
 *   margins_out_or_null [R, G] f32: the batch's final margins, by position.
 *   status     [U] int32, only ever SET: 1 where a user's batch holds a value
 *              that is not finite as float32, a row outside [0, F) or a label
 *              outside [0, G) (its forest gets no tree), 2 where a batch holds
 *              more than n_max rows (not run).  Zero it before the call.
 * workspace: ce_xgb_fit_workspace_bytes(R, n_max, D, G, rounds) bytes, 16-byte
 * aligned (the margins and every feature's sorted column: about 6 R D bytes).
 * Before any launch -- CE_EINVAL: bad shapes, rounds or max_depth < 1, depth <
 * max_depth, n_max > R, eta / lambda / min_child_weight out of range, a null
 * pointer; CE_EUNSUPPORTED: D > 512, G > 8, G == 1 (binary:logistic), max_depth
 * > 5, depth > 5, n_max > 4096 rows per user; CE_EWORKSPACE.  R == 0 launches
 * nothing.  No allocation; stream-ordered, nothing read back.
 */
size_t ce_xgb_fit_workspace_bytes(int64_t R, int64_t n_max, int32_t D, int32_t G, int32_t rounds);
int ce_xgb_fit_users(const void *X, ce_dtype x_dt, int64_t F, int32_t D, int64_t ld, const int64_t *rows,
                     const int32_t *labels, const int64_t *row_offsets, int32_t U, int64_t R, int64_t n_max,
                     const uint32_t *table, int32_t TT, const int32_t *tree_ids, int64_t L,
                     const int32_t *group_offsets, int32_t G, int32_t depth, float base_margin,
                     int32_t rounds, int32_t max_depth, float eta, float lambda, float min_child_weight,
                     uint32_t *nodes_out, float *leaves_out, int32_t *left_out, int32_t *right_out,
                     int32_t *split_out, float *cond_out, uint8_t *default_left_out, int32_t *num_nodes_out,
                     float *margins_out_or_null, int32_t *status, void *workspace, size_t workspace_bytes,
                     ce_stream_t stream);

/*
 * glibc's f64 log as the engine evaluates it inside every entropy
 * (scipy.special.entr's log, amg_test.py:443; csrc/ce_glibc_log.hpp), exposed
 * for verification against the C library:
 *   ce_log_f64       y[i] = log(x[i]) on the device (x, y device memory)
 *   ce_log_f64_host  the same restatement on the host CPU (x, y HOST memory;
 *                    synchronous, no GPU needed)
 */
int ce_log_f64(const double *x, int64_t n, double *y, ce_stream_t stream);
/* y[i] = x[i] / s[i] as every entropy divides its row by the row sum (one
 * reciprocal per row, ce_device.hpp RowDivisor) -- verification against IEEE
 * division (device memory, stream-ordered). */
int ce_row_div_f64(const double *x, const double *s, int64_t n, double *y, ce_stream_t stream);
int ce_log_f64_host(const double *x, int64_t n, double *y);
/* glibc's f64 exp restated (csrc/ce_glibc_exp.hpp; the exp of the GaussianNB
 * member's logsumexp): device (stream-ordered) and host
 * (synchronous, no GPU) builds, for verification against the C library. */
int ce_exp_f64(const double *x, int64_t n, double *y, ce_stream_t stream);
int ce_exp_f64_host(const double *x, int64_t n, double *y);
/* The single-block pools' approximate entropy (f32, hardware rcp / log2; the
 * prefilter of csrc/ce_small.hpp) of n exact consensus rows [n, C] (C in
 * {2, 3, 4, 8}), in log2 units, and whether each row is special (taken by the
 * exact path): verification of the error bound the prefilter's floor relies on. */
int ce_approx_entropy(const double *rows, int64_t n, int32_t C, float *h2, uint8_t *special, ce_stream_t stream);
/* The wide stream's approximate prefilter (csrc/ce_wide.hpp wave_approx_entropy:
 * f32 copies, one v_rcp_f32, a hardware log2 per class) of n rows [n, C] f64 --
 * member sums or means, laid out as k_stream_wide2 holds a dt committee's rows
 * in registers (C a multiple of 4 / 2 / 8 for f32 / f64 / bf16, C <= 2048) --
 * in log2 units, and whether each row is special (taken by the exact path):
 * verification of the kWideApproxErr2 margin the chunked C5 job skips by. */
int ce_wide_approx_entropy(const double *rows, int64_t n, int32_t C, ce_dtype dt, float *h2,
                           uint8_t *special, ce_stream_t stream);

/*
 * Top-q of an entropy vector -- replaces np.argsort(ent)[::-1][:q]
 * (amg_test.py:445, :452, :480).  Positions are reported as base_idx + i.
 * val_out: [q] f64, idx_out: [q] int64.
 */
size_t ce_topq_workspace_bytes(int64_t N, int32_t q);
int ce_topq(const double *ent, int64_t N, int32_t q, int64_t base_idx, void *ws, size_t ws_bytes,
            double *val_out, int64_t *idx_out, ce_stream_t stream);

/*
 * Merge of nlists candidate lists of q slots each (vals/idx: [nlists*q], every
 * list best-first as the ce_* outputs are; idx < 0 = empty slot) into the
 * global top-q.  Used after the RCCL all-gather of per-GPU top-q lists.  No
 * workspace: q > CE_MAX_Q merges by rank (a binary search per candidate and list).
 */
int ce_topq_merge(const double *vals, const int64_t *idx, int32_t nlists, int32_t q,
                  double *val_out, int64_t *idx_out, ce_stream_t stream);

/*
 * Fused mc selection -- replaces amg_test.py:441-445 in one pass over the
 * committee tensor (entropies never reach HBM): scores each item and keeps a
 * per-block top-q, then merges the blocks' candidates -- for q <= 64 inside
 * the same launch (the last block to finish merges), so the whole selection
 * is one kernel.
 * ce_select_mc_partial + ce_select_finish are the same two stages exposed
 * separately (q <= CE_MAX_Q; the bench times them apart).
 */
size_t ce_select_mc_workspace_bytes(int64_t N, int32_t q);
int ce_select_mc(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                 int64_t sM, int64_t sC, int32_t q, int64_t base_idx, void *ws, size_t ws_bytes,
                 double *val_out, int64_t *idx_out, ce_stream_t stream);
int ce_select_mc_partial(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                         int64_t sM, int64_t sC, int32_t q, int64_t base_idx, void *ws,
                         size_t ws_bytes, ce_stream_t stream);
/* Stage 2 of ce_select_mc / ce_select_mix / ce_topq on a filled workspace. */
int ce_select_finish(int64_t N, int32_t q, void *ws, size_t ws_bytes, double *val_out,
                     int64_t *idx_out, ce_stream_t stream);

/*
 * Exchange records for the multi-GPU merge (BASELINE.json north_star: "each GPU
 * computes its local top-q, an RCCL allgather over xGMI collects the
 * candidates, and a merge produces the final q").  A ce_cand is 16 bytes of
 * plain data: `key` is an order key monotone in the selection order (NaN first,
 * entropy descending; compare as unsigned), `idx` the global position, -1 for
 * an empty slot.  A list is q records, best first.
 *   ce_select_finish_cands  stage 2 of ce_select_mc_partial, writing the rank's
 *                           q records to `out` (the all-gather send buffer)
 *   ce_merge_cands          merge nlists such lists (the all-gather receive
 *                           buffer, rank-major) into the final top-q
 * Any q (ce_select_finish_cands: q <= CE_MAX_Q, a stage 2 of
 * ce_select_mc_partial) and 16-byte aligned record buffers.
 */
typedef struct {
    uint64_t key;
    int64_t idx;
} ce_cand;

int ce_select_finish_cands(int64_t N, int32_t q, void *ws, size_t ws_bytes, ce_cand *out,
                           ce_stream_t stream);
/* ce_select_mc writing the pool's q records to `out` in ONE launch (stage 2
 * folded into stage 1's last block; ws sized by ce_select_mc_workspace_bytes). */
int ce_select_mc_cands(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                       int64_t sM, int64_t sC, int32_t q, int64_t base_idx, void *ws, size_t ws_bytes,
                       ce_cand *out, ce_stream_t stream);
int ce_merge_cands(const ce_cand *c, int32_t nlists, int32_t q, double *val_out, int64_t *idx_out,
                   ce_stream_t stream);

/*
 * Chunked mc selection for a pool larger than HBM (BASELINE configs[4]: 50M
 * items x 32 members x 1000 classes bf16 = 3.2 TB) -- amg_test.py:441-445 over
 * a pool that arrives in chunks.  Each call scores one resident chunk (pool
 * items base_idx .. base_idx + N - 1, positions reported as pool positions)
 * and merges its top-q with the caller's running list `running` (q ce_cand
 * records, best first, 16-byte aligned device memory) in place; first != 0
 * starts a job (running's content is ignored and overwritten).  After the
 * last chunk ce_merge_cands(running, 1, q, ...) returns the selection -- the
 * same as ce_select_mc over the whole pool, ties included.  Any q.
 */
size_t ce_select_mc_chunk_workspace_bytes(int64_t N, int32_t q);
int ce_select_mc_chunk(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                       int64_t sM, int64_t sC, int32_t q, int64_t base_idx, ce_cand *running,
                       int32_t first, void *ws, size_t ws_bytes, ce_stream_t stream);

/*
 * Device-resident multi-epoch selection (amg_test.py:396-397
 * epochs, :455/:484 hc-pool shrink, :521-531 X_train shrink): instead of
 * rebuilding the pool every epoch, the caller keeps the full pool on the device
 * with an exclusion bitmap (bit i of word i/32 set = item i already queried).
 *   ce_excl_words      uint32 words of a bitmap for N items (host arithmetic)
 *   ce_select_mc_excl  ce_select_mc over the items whose bit is clear (any q;
 *                      ws sized by ce_select_mc_workspace_bytes)
 *   ce_mark_selected   set the bits of the n positions idx[0..n) (minus
 *                      base_idx; negative / out-of-range entries ignored) --
 *                      fed the previous call's idx_out, nothing leaves the GPU
 */
size_t ce_excl_words(int64_t N);
int ce_select_mc_excl(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                      int64_t sM, int64_t sC, const uint32_t *excl, int32_t q, int64_t base_idx,
                      void *ws, size_t ws_bytes, double *val_out, int64_t *idx_out,
                      ce_stream_t stream);
int ce_mark_selected(uint32_t *excl, int64_t N, const int64_t *idx, int32_t n, int64_t base_idx,
                     ce_stream_t stream);

/*
 * Fused mix selection -- replaces amg_test.py:473-480: the ROW stack
 * [mc consensus (N rows); hc table (N_h rows)], entropy, top-q over the union.
 * Positions in [0, N) are committee items, [N, N + N_h) hc rows.
 * hc: [N_h, C] f64 with row stride ld_hc (elements).
 */
size_t ce_select_mix_workspace_bytes(int64_t N, int64_t N_h, int32_t q);
int ce_select_mix(const void *p, ce_dtype dt, int64_t N, int32_t M, int32_t C, int64_t sN,
                  int64_t sM, int64_t sC, const double *hc, int64_t N_h, int64_t ld_hc, int32_t q,
                  void *ws, size_t ws_bytes, double *val_out, int64_t *idx_out,
                  ce_stream_t stream);

/*
 * Batched personalization -- replaces the per-user loop (amg_test.py:345) around
 * :441-445: U independent pools in one launch.  User u owns items
 * [offsets[u], offsets[u+1]) of the committee tensor (offsets: [U+1] int64,
 * DEVICE memory; total_items = offsets[U] is passed for workspace sizing).
 * Output slots [u*q, (u+1)*q); positions are user-local (0-based in the pool).
 */
size_t ce_select_batched_workspace_bytes(int64_t total_items, int32_t U, int32_t q);
int ce_select_batched(const void *p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C,
                      int64_t sN, int64_t sM, int64_t sC, const int64_t *offsets, int32_t U,
                      int32_t q, void *ws, size_t ws_bytes, double *val_out, int64_t *idx_out,
                      ce_stream_t stream);

/*
 * Batched multi-epoch selection -- the per-user loop (amg_test.py:345) around
 * the epochs (:396-397) with each user's shrinking pool (:521-531) kept on the
 * device: ce_select_batched over the items whose bit is clear.  excl is a
 * bitmap over the GLOBAL item index offsets[u] + i (ce_excl_words(total_items)
 * words, so words straddle users); NULL = ce_select_batched.  Output as
 * ce_select_batched (user-local positions; -1 / NaN past a user's alive
 * items); any q, the sort path's limits as there.  Workspace:
 * ce_select_batched_workspace_bytes.
 */
int ce_select_batched_excl(const void *p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C,
                           int64_t sN, int64_t sM, int64_t sC, const int64_t *offsets, int32_t U,
                           const uint32_t *excl, int32_t q, void *ws, size_t ws_bytes, double *val_out,
                           int64_t *idx_out, ce_stream_t stream);

/*
 * Batched mix -- replaces amg_test.py:473-480 for U users at once (the loop of
 * :345 around it): user u's problem is the row stack [mc_u (N_u committee
 * items offsets[u] .. offsets[u+1]); hc_u (Nh_u rows offsets_h[u] ..
 * offsets_h[u+1] of the stacked tables)] over the rows still alive.
 * hc: [total_h, C] f64 with row stride ld_hc (elements), the users' tables one
 * after the other; offsets_h: [U+1] int64, DEVICE memory.  excl / excl_h:
 * optional bitmaps over the global item index / the global hc row index
 * (ce_excl_words(total_items) / ce_excl_words(total_h) words), NULL = none.
 * Output slots [u*q, (u+1)*q), user-local positions: i in [0, N_u) is
 * committee item i, N_u + j is hc row j of that user; order and padding as
 * everywhere (on an exact tie the lower position wins: the committee item
 * before the hc row).  A user may have N_u = 0, Nh_u = 0 or both.
 * One launch, for C = 4 and 1 <= q <= 64 (q = 0 writes nothing); any other
 * shape returns CE_EUNSUPPORTED: compose it from ce_select_batched_excl over
 * either part and ce_topq_merge per user.
 */
size_t ce_select_batched_mix_workspace_bytes(int64_t total_items, int64_t total_h, int32_t U, int32_t q);
int ce_select_batched_mix(const void *p, ce_dtype dt, int64_t total_items, int32_t M, int32_t C,
                          int64_t sN, int64_t sM, int64_t sC, const int64_t *offsets, const double *hc,
                          int64_t total_h, int64_t ld_hc, const int64_t *offsets_h, int32_t U,
                          const uint32_t *excl, const uint32_t *excl_h, int32_t q, void *ws,
                          size_t ws_bytes, double *val_out, int64_t *idx_out, ce_stream_t stream);

/*
 * Marks the picks of a batched selection -- amg_test.py:484 (the hc frame
 * drops the queried songs) and :521-531 (X_train does) for U users: idx [U, q]
 * as ce_select_batched_excl / ce_select_batched_mix wrote it.  Slot (u, k)
 * with p = idx[u*q + k] >= 0:
 *   p < N_u:  sets bit g = offsets[u] + p of excl and, when m2h is given and
 *             m2h[g] >= 0, bit m2h[g] of excl_h;
 *   else j = p - N_u < Nh_u: sets bit h = offsets_h[u] + j of excl_h and, when
 *             h2m is given and h2m[h] >= 0, bit h2m[h] of excl.
 * Other slots are ignored.  m2h [total_items] / h2m [total_h] hold GLOBAL
 * indices (-1: no twin): a song leaves both pools whichever part picked it.
 * offsets_h, excl_h, m2h, h2m may be NULL (offsets_h and excl_h together; the
 * maps need both).
 */
int ce_mark_selected_batched(const int64_t *idx, int32_t U, int32_t q, const int64_t *offsets,
                             uint32_t *excl, const int64_t *offsets_h, uint32_t *excl_h,
                             const int64_t *m2h, const int64_t *h2m, ce_stream_t stream);

/*
 * The short-chunk CNN member, inference (the 'short_cnn' member of
 * amg_test.py:430 / :462: predict_cnn, :173-201, over short_cnn.py:278-349 in
 * eval mode), f32 throughout as the reference runs it:
 *   waveform [L] -> power spectrogram (n_fft = window = 512, hop 256, periodic
 *   Hann, centred with reflect padding: T = L / 256 + 1 frames, 257 bins)
 *   -> filter bank fb [257, 128] -> 10 log10(max(x, 1e-10))          (ce_cnn_logmel)
 *   -> spec_bn -> 7 x (conv 3x3, pad 1, bias -> BatchNorm -> ReLU -> max-pool
 *   2x2, floor), channels 1 -> nc, nc, 2nc, 2nc, 2nc, 2nc, 4nc -> max over the
 *   width left -> dense1 -> BatchNorm1d -> ReLU -> dense2 -> sigmoid: [4] per
 *   excerpt, un-normalised                                    (ce_cnn_forward_users)
 * BatchNorm uses the running statistics; the caller folds them (and the conv /
 * dense1 bias) into a per-channel scale and shift, in double, so that a
 * normalised value is fma(scale, sum, shift).
 *
 * ce_cnn_logmel: wave [S, L] f32, row pitch ld_wave >= L (512 <= L < 8 * 65535 * 256) -> mel
 * [S, 128, T] f32 (dB).  basis [2, 512, 257] f32: plane 0 w[n] cos(2 pi f n /
 * 512), plane 1 w[n] sin(2 pi f n / 512), w the periodic Hann window -- the DFT
 * is a product with it, not an FFT.  fb [257, 128] f32 (the state dict's
 * spec.mel_scale.fb).  The max is torch.clamp(min = 1e-10): a band without
 * power (an empty band of the bank, digital silence) is -100 dB, and a NaN
 * stays a NaN -- every band of the frames that cover a NaN sample is NaN, and
 * the network carries it to that excerpt's four outputs (ReLU, the pools and
 * the global max pass a NaN on as torch's do).  One launch.
 *
 * Weights: one packed f32 record per model, ce_cnn_weights_floats(nc) floats,
 * the records stacked [Uw, floats] (256-B aligned).  In order, every part a
 * multiple of 16 floats:
 *   spec [16]                scale, shift of spec_bn, zeros
 *   per block i = 1 .. 7     w [9 Cin, Cout] (row (ky 3 + kx) Cin + ci), scale [Cout], shift [Cout]
 *   W1 [4nc, 4nc]            dense1.weight TRANSPOSED (input-major)
 *   s1 [4nc], t1 [4nc]       BatchNorm1d over dense1 (its bias folded into t1)
 *   W2 [4, 4nc]              dense2.weight
 *   b2 [16]                  dense2.bias, zeros
 *
 * ce_cnn_forward_users: mel [n, 128, T] holds the excerpts s_base .. s_base +
 * n - 1 of the stacked pool (a batch: n <= 65535); item_offsets [U + 1]
 * (DEVICE), excl_or_null (a bitmap, ce_excl_words), y_or_null and out are
 * indexed by the pool position s.  Excerpt s belongs to the user u with
 * item_offsets[u] <= s < item_offsets[u+1] and runs through record u (Uw == U)
 * or record 0 (Uw == 1: one shared model).  An excerpt that is excluded or that
 * no user owns is neither computed nor written.  out [*, 4] f32, row pitch
 * ld_out >= 4.  y / cm (both or neither): y [*] int32 the class of excerpt s,
 * cm [U, 4, 4] int64; the predicted class is np.argmax of the four outputs (the
 * first maximum; a NaN wins at its first occurrence) and cm[u, y, pred] is
 * bumped with an integer atomic (a label outside [0, 4) is not counted).  cm is
 * NOT zero-filled here: a pool is walked in batches that add to one cm.
 * ws: ce_cnn_workspace_bytes(n, T, nc) bytes, two ping-pong activation buffers
 * (not zero-filled, no header).  Every output is one ordered f32 fma chain (no
 * split-K, no float atomic): its bits depend on neither n, s_base, U nor Uw.
 * CE_EINVAL: n_mels != 128, T < 128, nc not a positive multiple of 16 (<= 1024),
 * Uw neither 1 nor U, bad shapes, a null pointer; CE_EWORKSPACE: a short ws.
 * All checked before any device call.  8 launches, nothing read back.
 *
 * ce_cnn_activations: what block `block` (1 .. 7) of one model writes, for
 * tests and diagnosis: the forward's own launch sequence (the same kernels,
 * grids and ping-pong order) over blocks 1 .. block, then a device-to-device
 * copy on the stream of that block's output into act [n, 128 >> block,
 * T >> block, C] f32, channel-innermost, C = nc, nc, 2nc, 2nc, 2nc, 2nc, 4nc
 * (after BatchNorm, ReLU and the pool).  weights: ONE record; no exclusion;
 * item_offsets [2] (DEVICE) = {0, any value >= n}, the one owner's range as the
 * forward takes it.  mel, n, n_mels, T, nc, ws as above, and the same errors;
 * CE_EINVAL also for a block outside 1 .. 7.  block launches and one copy.
 */
size_t ce_cnn_weights_floats(int32_t nc);
size_t ce_cnn_workspace_bytes(int64_t batch, int32_t T, int32_t nc);
int ce_cnn_logmel(const float *wave, int64_t S, int64_t L, int64_t ld_wave, const float *basis,
                  const float *fb, float *mel, ce_stream_t stream);
int ce_cnn_forward_users(const float *mel, int64_t n, int32_t n_mels, int32_t T, const float *weights,
                         int32_t nc, int32_t Uw, const int64_t *item_offsets, int32_t U,
                         int64_t s_base, const uint32_t *excl_or_null, const int32_t *y_or_null,
                         int64_t *cm_or_null, float *out, int64_t ld_out, void *ws, size_t ws_bytes,
                         ce_stream_t stream);
int ce_cnn_activations(const float *mel, int64_t n, int32_t n_mels, int32_t T, const float *weights,
                       int32_t nc, const int64_t *item_offsets, int32_t block, float *act, void *ws,
                       size_t ws_bytes, ce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CE_AMD_CE_H */
