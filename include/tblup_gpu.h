/*
 * tblup_gpu.h — C ABI of the MI355X GBLUP fitness evaluator (libtblup_gpu.so).
 *
 * Drop-in boundary for the reference's fitness-evaluation hot path
 * (ianwhale/tblup).  The reference has no native FFI; its boundary is the
 * Python evaluator plugin API, whose compute leg is the multiprocessing
 * worker pool:
 *
 *   ParallelEvaluator.__enter__/__exit__   tblup/evaluator.py:120-135  -> tblup_ctx_create / tblup_ctx_destroy
 *   BlupParallelEvaluator.__init__ split   tblup/evaluator.py:188-203  -> tblup_set_split
 *   worker() + enqueue() + blup()          tblup/evaluator.py:205-263  -> tblup_eval_batch
 *     gblup()    evaluator.py:265-286   (branch TBLUP_BRANCH_GBLUP)
 *     snp_blup() evaluator.py:288-314   (branch TBLUP_BRANCH_SNP)
 *     dispatch   evaluator.py:257       (branch TBLUP_BRANCH_AUTO: k > n -> gblup)
 *   make_grm()                             tblup/utils.py:7-18          -> tblup_debug_grm (block readback)
 *
 * The ctypes binding a maintainer adds on the reference side is shown in
 * INTEGRATION.md.  All functions return 0 on success and a negative status
 * otherwise; tblup_last_error() returns a thread-local message.  Host buffers
 * are borrowed for the duration of the call only.  A NaN fitness (constant
 * prediction, degenerate panel) is returned as NaN, never raised.
 */
#ifndef TBLUP_GPU_H
#define TBLUP_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tblup_ctx tblup_ctx;

enum {
  TBLUP_OK = 0,
  TBLUP_ERR_ARG = -1,      /* invalid argument (shape, index range, unknown split) */
  TBLUP_ERR_HIP = -2,      /* HIP runtime error (no device, launch or copy failure) */
  TBLUP_ERR_OOM = -3,      /* device allocation failed */
  TBLUP_ERR_STATE = -4,    /* call out of order */
  TBLUP_ERR_INDEX = -5     /* SNP index outside [-n_snps, n_snps): numpy's IndexError for data[:, indices] */
};

enum {
  TBLUP_BRANCH_AUTO = 0,   /* evaluator.py:257: len(indices) > n_animals -> GBLUP else SNP-BLUP */
  TBLUP_BRANCH_GBLUP = 1,  /* evaluator.py:265-286: p over all n animals, no phenotype centring */
  TBLUP_BRANCH_SNP = 2     /* evaluator.py:288-314: p over train animals, ridge intercept = mean(y_T) */
};

enum {
  TBLUP_LAYOUT_ANIMAL_MAJOR = 0, /* n_animals x n_snps, row-major (the .npy the reference loads) */
  TBLUP_LAYOUT_SNP_MAJOR = 1     /* n_snps x n_animals, row-major */
};

/* Last error message of the calling thread ("" if none). */
const char* tblup_last_error(void);

/* Library version string. */
const char* tblup_version(void);

/* Number of visible HIP devices (0 when none). */
int tblup_device_count(int* out_count);

/*
 * Create a context on HIP device `device`: uploads the {0,1,2} genotype
 * matrix (int8) and the phenotype vector (float64, length n_animals).
 * Replaces the per-worker np.load of evaluator.py:215-216.
 * tblup_ctx_create(NULL, 0, 0, layout, NULL, device, &ctx) creates a context
 * without a panel, for the DE step and genome decode only (no split can be set).
 */
int tblup_ctx_create(const int8_t* geno, int64_t n_animals, int64_t n_snps, int layout,
                     const double* pheno, int device, tblup_ctx** out_ctx);

int tblup_ctx_destroy(tblup_ctx* ctx);

/*
 * Register a train/validation split under `split_id` (replacing any split
 * with that id).  train/valid are animal row ids in the reference's order
 * (evaluator.py:196-203, 316-322, 485-491, 555-561, 413).
 */
int tblup_set_split(tblup_ctx* ctx, int split_id, const int64_t* train, int64_t n_train,
                    const int64_t* valid, int64_t n_valid);

int tblup_drop_split(tblup_ctx* ctx, int split_id);

/*
 * Multi-trait evaluation (BASELINE config 5; build-defined, the reference is
 * single-trait): replace the context's phenotypes with an n_animals x n_traits
 * row-major matrix, 1 <= n_traits <= TBLUP_MAX_TRAITS.  Independent traits with
 * a shared G decouple (G (x) I + lambda I), so one Cholesky per individual
 * serves every trait's right-hand side; each trait's EBVs are exactly the
 * single-trait blup() of that phenotype column (evaluator.py:244-314), and
 * fitness = mean over traits of |pearson(EBV_V,t, y_V,t)|; ebv outputs become
 * batch x n_traits x n_valid.  Drops every registered split (they hold
 * per-trait phenotype vectors): call tblup_set_split again afterwards.
 */
#define TBLUP_MAX_TRAITS 4
int tblup_set_traits(tblup_ctx* ctx, const double* pheno, int64_t n_traits);
int tblup_get_traits(tblup_ctx* ctx, int64_t* n_traits);

/*
 * Evaluate `batch` individuals (one blup() call each, evaluator.py:244-314).
 *   idx      : concatenated selected SNP column indices (duplicates allowed,
 *              any order), length offsets[batch].  numpy fancy-index rules, as the
 *              reference's data[:, indices] (evaluator.py:275/298) applies them to an
 *              IndexIndividual genome (individual.py:93-95, unclipped DE can go
 *              negative): -n_snps <= i < 0 addresses column i + n_snps; any index
 *              outside [-n_snps, n_snps) fails the whole call with TBLUP_ERR_INDEX
 *   offsets  : batch+1 prefix offsets into idx; an individual may have k >= 1
 *   h2       : heritability, lambda = (1-h2)/h2
 *   branch   : TBLUP_BRANCH_*
 *   fitness  : out, batch doubles, |pearson(EBV_V, y_V)| (NaN when undefined)
 *   ebv      : optional out (may be NULL), batch x n_valid predicted breeding values
 *              (batch x n_traits x n_valid after tblup_set_traits)
 * Synchronous; host pointers.  A chained solve (SNP form, small chunks) whose bounded hand-off
 * wait expires does not fail the call: the chunk's factor is solved again by the one-workgroup
 * back substitution, bit-identical to an unexpired run, and counted (tblup_chain_recoveries).
 */
int tblup_eval_batch(tblup_ctx* ctx, int split_id, const int64_t* idx, const int64_t* offsets,
                     int64_t batch, double h2, int branch, double* fitness, double* ebv);

/*
 * Taking the fitted model out.  The reference ends a blup() call with one number; the model it
 * fitted on the way is the clf of snp_blup (evaluator.py:311-312: coef_, intercept_, and the 2p it
 * subtracted, :304-309) or, under gblup, the all-animal `prediction` of evaluator.py:284 that it
 * indexes by the validation rows and drops (:286).  Both are, for selected columns idx[0..k)
 * (duplicates kept, each occurrence its own column, as data[:, indices]),
 *   EBV_t(a) = intercept[t] + sum_j (x[a, idx_j] - center[j]) * effects[t][j]
 * with center[j] = 2 p_j, the exact allele count of column j over the branch's reference rows (all
 * n animals for gblup, utils.py:7-18; the train rows for snp, evaluator.py:304) divided once by
 * their number; effects = the solved beta (SNP form: Ridge's primal coef_) or W_T^T alpha / d
 * (kernel form: gblup, and the snp branch's dual Ridge when k > n_T), W = A - 2p, d = 2 sum p(1-p),
 * (K_TT + lambda I) alpha = y_T - mu; intercept = 0 (gblup) or the split's mean(y_T) (snp).
 *
 * tblup_fit_batch: tblup_eval_batch plus the model of every individual.  idx / offsets / h2 /
 * branch, the index rules and errors and the chunking by TBLUP_WORKSPACE_MB are tblup_eval_batch's.
 *   fitness   : optional out (may be NULL), batch doubles, bit-identical to tblup_eval_batch's
 *   intercept : out, batch x n_traits
 *   center    : out, offsets[batch] doubles, indexed like idx
 *   effects   : out, n_traits x offsets[batch], trait-major planes each indexed like idx
 * An individual whose solve yields NaN (a monomorphic panel: d = 0) gets NaN effects; that is not
 * an error.  The effects are the same bits under every TBLUP_SOLVE_CHAIN / TBLUP_SOLVE_PULL
 * setting.  Host pointers, synchronous.
 */
int tblup_fit_batch(tblup_ctx* ctx, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch,
                    double h2, int branch, double* fitness, double* intercept, double* center, double* effects);

/*
 * Reliabilities of the predicted breeding values: tblup_fit_batch plus, for each of `n_pred` animals
 * of the context's panel under each of the `batch` models, the squared accuracy of its genomic value
 * g_a = w_a . beta (r^2 = 1 - PEV / (sigma_g^2 K_aa)).  With A the gathered columns idx[0..k)
 * (duplicates kept), c = 2p the exact allele count over the branch's N reference rows divided once by
 * N (all n animals for gblup -- the reference's make_grm centres over every row, candidates included
 * -- and the train rows for snp), d = 2 sum p(1-p), lambda = (1-h2)/h2, w_a = A[a] - c, K = W W^T / d:
 *   rel(a) = k_aT^T (K_TT + lambda I)^{-1} k_Ta / K_aa,  k_Ta = W_T w_a / d, K_aa = w_a.w_a / d   (kernel form)
 *   rel(a) = 1 - lambda w_a^T (C + lambda I)^{-1} w_a / (w_a.w_a),  C = W_T^T W_T / d            (SNP form)
 * -- equal by the Woodbury identity; the library evaluates whichever form the batch's systems were
 * factored in.  The model is the reference's own: beta ~ N(0, sigma_g^2 / d I), e ~ N(0, sigma_e^2 I),
 * sigma_e^2 / sigma_g^2 = lambda; the snp branch's intercept mean(y_T) is taken as known (its
 * uncertainty is not in the PEV).  No phenotype and no variance component enters: with several traits
 * (one factor, shared h2) it is one number per (model, animal).
 *   animals     : n_pred row ids in [0, n), any order, repeats allowed, any or no split role
 *                 (TBLUP_ERR_ARG outside the range)
 *   fitness     : optional out (may be NULL), bit-identical to tblup_eval_batch's
 *   intercept / center / effects : optional as a triple -- all NULL: reliabilities only; all given:
 *                 tblup_fit_batch's outputs, bit for bit; anything else is TBLUP_ERR_ARG
 *   reliability : out, batch x n_pred
 * n_pred == 0 or batch == 0 returns 0 and writes nothing; a context without a panel gives
 * TBLUP_ERR_STATE; idx / offsets / h2 / branch, the index rules (TBLUP_ERR_INDEX) and the chunking are
 * tblup_eval_batch's.  d = 0 (a monomorphic panel) or K_aa = 0 gives NaN, not an error.
 * The Cholesky factor (k x k or n_T x n_T doubles per model) is not portable and is dropped with the
 * chunk, so reliabilities are produced here, at fit time: for newly genotyped candidates use a context
 * whose panel holds them as extra rows (they need not be in any split).
 * An animal's value depends neither on n_pred, nor on its position in `animals`, nor on the chunking
 * (TBLUP_WORKSPACE_MB), and the same call gives the same bits twice.  Host pointers, synchronous.
 */
int tblup_reliability_batch(tblup_ctx* ctx, int split_id, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                            const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                            double* intercept, double* center, double* effects, double* reliability);

/*
 * Leave-one-out cross-validation of each of `batch` fitted models: every training animal t of the split (in
 * the split's `train` order) predicted by the model fitted without it, in closed form from the factor that one
 * evaluation leaves behind -- the k -> n_T limit of k-fold cross-validation at the cost of one pass.  Notation is
 * tblup_reliability_batch's; c = 0 and mu = 0 under gblup, c = 1 / n_T and mu = mean(y_T) under snp:
 *   SNP form     h_tt = c + w_t^T (W_T^T W_T + lambda d I)^{-1} w_t,  e_t = y_t - mu - w_t . beta,
 *                e_loo,t = e_t / (1 - h_tt)
 *   kernel form  V = K_TT + lambda I, alpha = V^{-1} (y_T - mu):
 *                e_loo,t = lambda alpha_t / (lambda (V^{-1})_tt - c),  h_tt = 1 + c - lambda (V^{-1})_tt
 *   y^_loo,t = y_t - e_loo,t
 * -- equal by the Woodbury identity; the library evaluates whichever form the batch's systems were factored in.
 * gblup branch: y^_loo,t is the reference's gblup prediction of animal t from a model trained on T \ {t} (K the
 * GRM over all n animals, as the reference centres it).  snp branch: ridge regression with the fitted model's own
 * penalty lambda d kept -- d and the centre come from the full training set, the intercept and the centring are
 * refitted on T \ {t}.  This is not the reference pipeline re-run with t removed: that re-run would also change
 * p and d.
 *   fitness      : out, batch: |pearson(y^_loo, y_T)| over the n_T animals, the mean over traits for several
 *                  traits (tblup_eval_batch's convention and NaN rules)
 *   loo_pred     : out, batch x n_traits x n_train
 *   leverage     : optional out (may be NULL), batch x n_train: h_tt, one number per (model, animal) whatever
 *                  the number of traits
 *   press        : optional out (may be NULL), batch x n_traits: sum_t e_loo,t^2
 *   eval_fitness : optional out (may be NULL), batch: the pass's own validation fitness, bit-identical to
 *                  tblup_eval_batch's
 * batch == 0 returns 0 and writes nothing; a context without a panel gives TBLUP_ERR_STATE; idx / offsets / h2 /
 * branch, the index rules (TBLUP_ERR_INDEX) and the chunking are tblup_eval_batch's.  d = 0 (a monomorphic
 * panel) gives NaN, not an error.  The error of the closed form grows as 1 / (1 - h_tt): near h2 = 1 in the
 * kernel form, where 1 - h_tt approaches 0, digits are lost in proportion.  LOO under fixed-effect covariates or
 * a class factor is not built.  An animal's values depend neither on the batch nor on the chunking
 * (TBLUP_WORKSPACE_MB), and the same call gives the same bits twice.  Host pointers, synchronous.
 */
int tblup_loo_batch(tblup_ctx* ctx, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch,
                    double h2, int branch, double* fitness, double* loo_pred, double* leverage, double* press,
                    double* eval_fitness);

/*
 * Profile (restricted) log-likelihood of h2 for each of `batch` models, at `n_h2` values each: the
 * evaluation's pipeline once per row of `h2`, plus one reduction over the factor it leaves behind.
 * The model is the reference's own, the one tblup_reliability_batch documents: beta ~ N(0, sigma2_g / d I),
 * e ~ N(0, sigma2_e I), sigma2_e / sigma2_g = lambda = (1-h2)/h2.  With N = n_T, A the gathered columns
 * (duplicates kept), W_T = A_T - c (c the branch's centre), K = W W^T / d, V = K_TT + lambda I, and
 * sigma2_g profiled out:
 *   gblup branch (no mean is fitted, as the reference fits none; r = 0):
 *     q = y_T^T V^{-1} y_T,   l = -1/2 [ N (log 2pi + 1 + log(q / N)) + log|V| ]
 *   snp branch (intercept mean(y_T), centre over the train rows, so V 1 = lambda 1; r = 1):
 *     q = yc^T V^{-1} yc, yc = y_T - mean(y_T); the restricted likelihood of the N - 1 error contrasts
 *     A^T y_T (A orthonormal, A^T 1 = 0):
 *     l_R = -1/2 [ (N-1)(log 2pi + 1 + log(q / (N-1))) + log|V| - log lambda ]
 *     (log|A^T V A| = log|V| - log lambda: 1/sqrt(N) is an eigenvector of V with eigenvalue lambda)
 *   sigma2_g = q / (N - r); the caller derives sigma2_e = lambda sigma2_g.
 * From the factor M = L L^T of the form the batch's systems take: log|M| = -2 sum log(1 / L_ii) over the
 * real rows; kernel form M = V and q = |z|^2 (z = L^{-1} rhs); SNP form M = W_T^T W_T / d + lambda I_k,
 * rhs = W_T^T yc / d, and by Sylvester and Woodbury log|V| = (N - k) log lambda + log|M|,
 * q = (yc^T yc - d |z|^2) / lambda.  Several traits share log|V|; q, l and sigma2_g are per trait.
 *   h2       : n_h2 x batch, row g holds every model's h2 of pass g (a shared grid: constant rows);
 *              each in (0, 1) -- lambda = 0 makes the snp branch's V singular, so h2 = 1 is
 *              TBLUP_ERR_ARG here (and only here), as are h2 <= 0 and NaN
 *   fitness  : optional out (may be NULL), n_h2 x batch; row g is bit-identical to tblup_eval_batch at
 *              that h2 when row g of `h2` is constant
 *   loglik   : out, n_h2 x batch x n_traits
 *   sigma2_g : optional out (may be NULL), the same shape
 * d = 0 (a monomorphic panel) or a quadratic form that is not positive and finite gives NaN, not an
 * error.  n_h2 == 0 or batch == 0 returns 0 and writes nothing; a context without a panel gives
 * TBLUP_ERR_STATE; idx / offsets / branch, the index rules (TBLUP_ERR_INDEX), the chunking and the
 * chained solve's recovery are tblup_eval_batch's.  Per chunk the index lists are uploaded once and
 * the n_h2 passes run back to back on the context's stream, the results copied out after the last.
 * A model's values depend neither on the batch around it, nor on the other rows of `h2`, nor on the
 * chunking (fixed-order sums, no atomics), and the same call gives the same bits twice.
 * Host pointers, synchronous.
 */
int tblup_loglik_batch(tblup_ctx* ctx, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch,
                       const double* h2, int64_t n_h2, int branch, double* fitness, double* loglik,
                       double* sigma2_g);

/*
 * Mixed-model score statistics of `n_cand` SNPs of the context's panel against each of `batch` fitted
 * panels (the score test of EMMAX / GRAMMAR-gamma): the evaluation's pipeline plus one forward
 * substitution per listed SNP against the factor it leaves behind.  The model is the reference's own, as
 * tblup_reliability_batch and tblup_loglik_batch document it.  For model b: A the gathered columns
 * idx[0..k) (duplicates kept), c the branch's centre (all n animals for gblup, the train rows for snp),
 * d = 2 sum p(1-p), lambda = (1-h2)/h2, W_T = A_T - c, K = W W^T / d, V = K_TT + lambda I,
 * r_t = y_T,t - mu_t (mu = 0 for gblup, mean(y_T) for snp), N = n_T.  For a listed column j of the panel,
 * whether or not it is in the model: w_j = x_T,j - c_j with the same centring rule (c_j the exact allele
 * count of column j over the branch's reference rows, divided once by their number), and
 *   score[b][t][j] = u = w_j^T V^{-1} r_t
 *   info[b][j]     = v = w_j^T V^{-1} w_j      (trait-independent: one factor, shared h2)
 *   q[b][t]        = r_t^T V^{-1} r_t          (what tblup_loglik_batch profiles sigma2_g from)
 * Under snp w_j is orthogonal to 1 and V 1 = lambda 1, so these are also the REML (P-matrix) forms with
 * the intercept fitted; under gblup no mean is fitted, as in the reference.  u / d is the SNP's
 * back-solved BLUP effect to first order: for a SNP of the model it is tblup_fit_batch's effect.
 * From the factor M = L L^T of the form the batch's systems take, z = L^{-1} rhs:
 *   kernel form (M = V):  s_j = L^{-1} w_j;  u = s_j.z_t,  v = s_j.s_j,  q = |z_t|^2
 *   SNP form (M = W_T^T W_T / d + lambda I_k, rhs = W_T^T r / d):  g_j = W_T^T w_j (exact integer counts
 *     (A_T^T x_j)_i minus sT_i sT_j / n_T), s_j = L^{-1} g_j;  u = (w_j.r_t - s_j.z_t) / lambda,
 *     v = (w_j.w_j - s_j.s_j / d) / lambda,  q = (r^T r - d |z|^2) / lambda
 *   snps    : n_cand column indices with idx's rules -- negatives wrap, anything outside
 *             [-n_snps, n_snps) is TBLUP_ERR_INDEX; any order, repeats allowed
 *   h2      : in (0, 1): lambda = 0 makes the snp branch's V singular (TBLUP_ERR_ARG, as tblup_loglik_batch)
 *   fitness : optional out (may be NULL), bit-identical to tblup_eval_batch's
 *   score   : out, batch x n_traits x n_cand
 *   info    : out, batch x n_cand
 *   q       : optional out (may be NULL), batch x n_traits
 * n_cand == 0 or batch == 0 returns 0 and writes nothing; a context without a panel gives
 * TBLUP_ERR_STATE; idx / offsets / branch, the index rules, the chunking and the chained solve's recovery
 * are tblup_eval_batch's.  d = 0 (a monomorphic model panel) gives NaN for every output of that model,
 * not an error; a listed column that is constant over the reference rows has w_j = 0 and gives
 * u = v = 0 exactly.
 * A (model, SNP) value depends neither on n_cand, nor on the SNP's position in `snps`, nor on the other
 * models of the batch (beyond the form they choose together), nor on the chunking (TBLUP_WORKSPACE_MB):
 * independent workgroups, fixed-order sums, no atomics; the same call gives the same bits twice.
 * Host pointers, synchronous.
 */
int tblup_snp_score_batch(tblup_ctx* ctx, int split_id, const int64_t* snps, int64_t n_cand, const int64_t* idx,
                          const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                          double* score, double* info, double* q);

/*
 * Fixed-effect covariates in the fitted model: tblup_fit_batch with `n_cov` covariates (sex, herd, batch,
 * ancestry PCs ..) fitted beside the genomic effects by generalised least squares on the same factor.
 * cov is n x n_cov, row-major, one row per animal of the panel, 1 <= n_cov <= 16.  Per model b and trait t,
 * with V, W_T, d, lambda and the branch's mu as tblup_snp_score_batch documents them,
 *   y_T = mu 1 + Q~_T b + g + e,   Q~ = Q - 1 m^T
 * with m_j the mean of column j over the train rows in split order under snp (then Q~_T^T 1 = 0 and
 * V 1 = lambda 1: the intercept stays mean(y_T) and decouples) and m = 0 under gblup: no mean is fitted
 * there unless the caller passes a column of ones, which is the way to fit one.  r_t = y_T,t - mu_t,
 *   b_t = (Q~_T^T V^{-1} Q~_T)^{-1} Q~_T^T V^{-1} r_t      (the GLS estimate)
 * and the genomic model is the branch's own model of the adjusted phenotype y*_t = y_t - Q~ b_t (every
 * animal, train and validation alike):
 *   fitness     : optional out (may be NULL), batch: the mean over traits of |pearson(ebv_V, y*_V)|, the
 *                 predictive ability on phenotypes corrected for the fitted fixed effects
 *   ebv         : optional out (may be NULL), batch x n_traits x n_valid: tblup_eval_batch's for phenotype y*
 *   cov_effects : out, batch x n_traits x n_cov: b
 *   cov_center  : out, batch x n_cov: m (all zero for a gblup model)
 *   intercept / center / effects : optional as a triple (all NULL or none): tblup_fit_batch's for phenotype y*
 * so that the value of an animal with genotype x and covariates q is
 *   intercept[t] + sum_j (x[idx_j] - center[j]) effects[t][j] + sum_i (q_i - cov_center[i]) cov_effects[t][i].
 * From the factor M = L L^T, S = L^{-1} R (one forward substitution with the covariates as one slab of 16
 * right-hand sides), G = Q~^T V^{-1} Q~, h_t = Q~^T V^{-1} r_t:
 *   kernel form (M = V):  R = Q~_T;  G = S^T S,  h_t = S^T z_t,  corrected z_t - S b_t
 *   SNP form (M = W_T^T W_T / d + lambda I_k):  R = W_T^T Q~_T;  G = (Q~_T^T Q~_T - S^T S / d) / lambda,
 *     h_t = (Q~_T^T r_t - S^T z_t) / lambda,  corrected z_t - S b_t / d
 * b_t = G^{-1} h_t by an n_cov x n_cov Cholesky; then the back substitution, the prediction and the effects
 * run a second time on the corrected z.  A pivot of G that is not positive (above 1e-12 of its own diagonal
 * entry of G: a repeated column leaves rounding noise of either sign) and finite (collinear covariates;
 * a column that is constant over the train rows under snp; h2 = 1 in the SNP form) gives NaN for every output
 * of that model, as d = 0 does: not an error.  A NaN or Inf in cov, or n_cov outside [1, 16], is TBLUP_ERR_ARG.
 * idx / offsets / h2 / branch, the index rules and errors and the chunking are tblup_fit_batch's; batch == 0
 * returns 0 and writes nothing; a context without a panel gives TBLUP_ERR_STATE.  The call keeps no state in
 * the context.  A model's bits depend neither on the other models of the batch (beyond the form they
 * choose together), nor on the chunking, nor on where the right-hand sides live (TBLUP_SCORE_LDS): fixed-order
 * sums, no atomics.  Host pointers, synchronous.
 */
#define TBLUP_MAX_COV 16
int tblup_fit_cov_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness, double* ebv,
                        double* cov_effects, double* cov_center, double* intercept, double* center, double* effects);

/*
 * A class fixed effect (herd, herd-year-season, batch, pen, sex x farm ..) beside the covariates:
 * tblup_fit_cov_batch with the fixed design F = [Q, Z], Q the n_cov dense covariates (0 <= n_cov <= 16; cov may be
 * NULL when n_cov is 0) and Z the one-hot columns of one factor.  group is int64 [n]: every animal's level code in
 * [0, n_levels), or -1 for an animal without one, which is allowed only outside the split's train and validation
 * rows.  The branch's centring rule applies to Z as it does to Q:
 *   gblup : nothing is centred and no mean is fitted.  Z has one column per level, in ascending code order; the
 *           level effects are the group means of the model (a column of ones in Q is then collinear: a NaN model).
 *           n_cov + n_levels columns.
 *   snp   : every column is centred by its mean over the train rows, the intercept stays mean(y_T).  Z drops the
 *           lowest level, the reference level, whose effect is exactly 0; the centre of level l is its share
 *           n_l / n_T of the train rows.  n_cov + n_levels - 1 columns.
 * With F~ the centred design, b_t = (F~_T^T V^{-1} F~_T)^{-1} F~_T^T V^{-1} r_t and y*_t = y_t - F~ b_t exactly as
 * tblup_fit_cov_batch has them for Q~; which level is the reference changes the reported effects and nothing else.
 * A model has at most TBLUP_MAX_FIXED = 128 columns.
 *   group_effects : out, batch x n_traits x n_levels: the level effects (0 at the reference level under snp)
 *   group_center  : out, batch x n_levels: the levels' shares of the train rows under snp, all zero for a gblup model
 *   cov_effects / cov_center : out, as tblup_fit_cov_batch (may be NULL when n_cov is 0)
 *   fitness / ebv / intercept / center / effects : tblup_fit_cov_batch's, for phenotype y*
 * so that the value of an animal of level g is tblup_fit_cov_batch's plus
 *   sum_l ([g == l] - group_center[l]) group_effects[t][l].
 * A model of 1 .. 16 columns runs tblup_fit_cov_batch's own kernels on the expanded design: its outputs are that
 * entry's on [Q, Z] bit for bit.  A wider one runs the same GLS step in 16-column slabs: S = L^{-1} R slab by slab
 * (a level's right-hand side in the SNP form is the allele count of each selected SNP over the level's train animals
 * minus s_i n_l / n_T: exact integers, one fp64 combination), G and h_t on fp64 MFMA (SNP form: F~_T^T F~_T and
 * F~_T^T r_t once per call, on the host in long double), a blocked Cholesky of G in 16 x 16 blocks under
 * tblup_fit_cov_batch's pivot rule, the two triangular solves, the corrected z and the second pass.
 * TBLUP_ERR_ARG: n_cov outside [0, 16]; n_levels < 1; a code outside [-1, n_levels); -1 on a split row; a level
 * with no train row; more than 128 columns for a model of the batch; NaN or Inf in cov.  A degenerate model (d = 0,
 * a flagged index, a pivot of G failing the rule: a covariate equal to a level's indicator, a column of ones beside
 * gblup levels) is NaN in every output of that model: not an error.  Everything else -- idx / offsets / h2 / branch,
 * the empty batch, the context without a panel, the chunking, the bits' independence of the batch, the chunking
 * and TBLUP_SCORE_LDS -- is tblup_fit_cov_batch's.  Host pointers, synchronous.
 */
#define TBLUP_MAX_FIXED 128
int tblup_fit_group_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                          int64_t n_levels, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                          int branch, double* fitness, double* ebv, double* cov_effects, double* cov_center,
                          double* group_effects, double* group_center, double* intercept, double* center,
                          double* effects);

/*
 * The score statistics of tblup_snp_score_batch and the likelihood of tblup_loglik_batch for the model with
 * fixed-effect covariates that tblup_fit_cov_batch fits: cov, n_cov, Q~, G = Q~_T^T V^{-1} Q~_T = C C^T,
 * h_t = Q~_T^T V^{-1} r_t and b_t = G^{-1} h_t as documented there, and with
 *   P = V^{-1} - V^{-1} Q~_T G^{-1} Q~_T^T V^{-1},   c = n_cov,   dof = N - r - c.
 *
 * tblup_snp_score_cov_batch: for listed column j, w_j as tblup_snp_score_batch defines it, a_j = Q~_T^T V^{-1} w_j:
 *   score : out, batch x n_traits x n_cand: u_P = w_j^T P r_t = u - (C^{-1} a_j).(C^{-1} h_t)
 *   info  : out, batch x n_cand:            v_P = w_j^T P w_j = v - |C^{-1} a_j|^2
 *   q     : optional out, batch x n_traits:  q_P = r_t^T P r_t = q - h_t^T b_t
 *   cov_effects : optional out, batch x n_traits x n_cov: tblup_fit_cov_batch's b at this h2, bit for bit
 *   fitness : optional out, batch: tblup_eval_batch's value, bit for bit (the model without covariates)
 * u_P / v_P is the GLS effect of the SNP fitted as one more covariate beside Q; u_P^2 / (v_P q_P / dof) the
 * score test.  From the factor, with S = L^{-1} R the covariates' slab (tblup_fit_cov_batch) and s_j the SNP's
 * solved column (tblup_snp_score_batch):
 *   kernel form:  a_j = S^T s_j          SNP form:  a_j = (Q~_T^T x_T,j - S^T s_j / d) / lambda
 * (Q~_T sums to zero over the train rows there, so the centre of w_j drops out).  A listed SNP with
 * v_P <= 1e-12 v -- constant over the reference rows, or in the span of the covariates -- gives u_P = v_P = 0
 * exactly.
 *
 * tblup_loglik_cov_batch: the restricted likelihood of the N - r - c error contrasts A^T y_T (A orthonormal,
 * A^T [1 Q~_T] = 0 under snp, A^T Q_T = 0 under gblup, where a mean is fitted only by a column of ones in Q),
 * sigma2_g profiled out:
 *   log|A^T V A| = log|V| - r log lambda + log|G| - log|Q~_T^T Q~_T|
 *   loglik   : out, n_h2 x batch x n_traits: -1/2 [ dof (log 2 pi + 1 + log(q_P / dof)) + log|A^T V A| ]
 *   sigma2_g : optional out, same shape: q_P / dof
 *   cov_effects : optional out, n_h2 x batch x n_traits x n_cov: b at each h2
 *   fitness  : optional out, n_h2 x batch: tblup_eval_batch's value at each h2
 * log|Q~_T^T Q~_T| does not depend on h2: once per call on the host, in long double; a plane (branch) whose
 * Q~_T is not of full rank by the pivot rule gives NaN for the models of that branch.
 *
 * Both: a model whose G has a pivot that is not positive (tblup_fit_cov_batch's rule) and finite, d = 0, a
 * flagged index or dof <= 0 gives NaN in score / info / q / loglik / sigma2_g (and cov_effects, except for
 * dof <= 0): not an error.  cov / n_cov and their errors are tblup_fit_cov_batch's; every other argument, the
 * index rules, h2 in (0, 1), the empty-call rules, the chunking and the chained-solve recovery are
 * tblup_snp_score_batch's / tblup_loglik_batch's.  A (model, SNP) value depends neither on the list, the
 * slab, the batch, the chunking nor TBLUP_SCORE_LDS: fixed-order sums, no atomics.  Host pointers, synchronous.
 */
int tblup_snp_score_cov_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* snps,
                              int64_t n_cand, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                              int branch, double* fitness, double* score, double* info, double* q,
                              double* cov_effects);
int tblup_loglik_cov_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                           const int64_t* offsets, int64_t batch, const double* h2, int64_t n_h2, int branch,
                           double* fitness, double* loglik, double* sigma2_g, double* cov_effects);

/*
 * The same two for the model with a class fixed effect that tblup_fit_group_batch fits: cov, n_cov, group, n_levels
 * and the design F = [Q, Z] as documented there (gblup: nothing centred, every level a column; snp: every column
 * centred by its train mean, the lowest level dropped), C_m = n_cov + n_levels - [snp] columns for a model, at most
 * TBLUP_MAX_FIXED.  With F~_T in place of Q~_T and C_m in place of c the statistics and the likelihood are exactly
 * tblup_snp_score_cov_batch's and tblup_loglik_cov_batch's:
 *   G = F~_T^T V^{-1} F~_T = C C^T,  h_t = F~_T^T V^{-1} r_t,  P = V^{-1} - V^{-1} F~_T G^{-1} F~_T^T V^{-1},
 *   dof = N - r - C_m,  log|A^T V A| = log|V| - r log lambda + log|G| - log|F~_T^T F~_T|.
 * C_m, so dof and log|F~_T^T F~_T|, differ between the gblup and the snp models of one batch.
 * Under gblup with a class factor, or with a column of ones in Q, q_P = q - |C^{-1} h_t|^2, sigma2_g and the likelihood
 * lose as many digits as the squared phenotype mean exceeds its variance: centre the phenotype first.
 *   score / info / q, loglik / sigma2_g, fitness : as the covariate entries have them
 *   cov_effects   : optional out, [n_h2 x] batch x n_traits x n_cov
 *   group_effects : optional out, [n_h2 x] batch x n_traits x n_levels: tblup_fit_group_batch's at this h2, bit
 *                   for bit (NaN throughout for a model that entry gives NaN)
 * A batch model of 1 .. 16 columns runs the covariate entries' own kernels on the expanded design: its outputs are
 * tblup_snp_score_cov_batch's / tblup_loglik_cov_batch's on [Q, Z] bit for bit.  A wider one runs
 * tblup_fit_group_batch's GLS step and keeps it -- S = L^{-1} R in 16-column slabs, C, C^{-1} h_t,
 * {log|G|, h_t^T b_t} -- and behind it
 *   the score statistics: T = S^T s_j (C_m x 16 per slab of listed SNPs) on fp64 MFMA, one wave per column slab over
 *     the real rows in order; SNP form a_j = (F~_T^T x_T,j - T / d) / lambda, a level's row of F~_T^T x_T,j being the
 *     exact allele count of SNP j over the level's train animals minus its share of the SNP's train sum; C y = a_j
 *     column by column with |y|^2 and y.(C^{-1} h_t) on the way; v_P <= 1e-12 v gives exact zeros;
 *   the likelihood: k_loglik with the model's own C_m and log|F~_T^T F~_T| of its plane, once per call on the host
 *     in long double under the pivot rule (NaN for a plane that is not of full rank).
 * Argument errors are tblup_fit_group_batch's (a code outside [-1, n_levels), -1 on a split row, a level without a
 * train row, more than 128 columns for a model of the batch, NaN in cov); everything else -- the empty calls, h2 in
 * (0, 1), the chunking, NaN and no error for a degenerate model or dof <= 0, the bits' independence of the list,
 * the slab, the batch, the chunking, TBLUP_SCORE_LDS and TBLUP_WORKSPACE_MB -- is the covariate entries'.
 * Host pointers, synchronous.
 */
int tblup_snp_score_group_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                                int64_t n_levels, const int64_t* snps, int64_t n_cand, const int64_t* idx,
                                const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                                double* score, double* info, double* q, double* cov_effects, double* group_effects);
int tblup_loglik_group_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                             int64_t n_levels, const int64_t* idx, const int64_t* offsets, int64_t batch,
                             const double* h2, int64_t n_h2, int branch, double* fitness, double* loglik,
                             double* sigma2_g, double* cov_effects, double* group_effects);

/*
 * Uncertainty under the model with fixed-effect covariates that tblup_fit_cov_batch fits: the reliabilities of
 * tblup_reliability_batch with the covariates' effects estimated, not known, the error variance of a predicted
 * value and the sampling covariance of the covariates' effects.  Notation is tblup_reliability_batch's and
 * tblup_fit_cov_batch's: V = K_TT + lambda I, k_Ta, K_aa, Q~ (centred by the train means m under snp, as given
 * under gblup), G = Q~_T^T V^{-1} Q~_T = C C^T.  Under snp the intercept mean(y_T) is still taken as known; under
 * gblup a mean is fitted only through a column of ones in Q.  For a listed animal a (any row of the panel, in any
 * or no split role), with P as tblup_snp_score_cov_batch defines it:
 *   a_a          = Q~_T^T V^{-1} k_Ta                                           (n_cov values)
 *   reliability  : out, batch x n_pred:  (k_Ta^T V^{-1} k_Ta - |C^{-1} a_a|^2) / K_aa = k_Ta^T P k_Ta / K_aa
 *                  = 1 - PEV(g^_a - g_a) / (sigma2_g K_aa) with b estimated; never above tblup_reliability_batch's
 *   pev_total    : optional out, batch x n_pred:  K_aa - k_Ta^T V^{-1} k_Ta + |C^{-1} (q~_a - a_a)|^2, q~_a = q_a - m:
 *                  the error variance of q~_a^T b^ + g^_a as a predictor of q~_a^T b + g_a, in units of sigma2_g
 *   cov_cov      : optional out, batch x n_cov x n_cov (compact, row-major):  G^{-1}, in units of sigma2_g:
 *                  Var(b^_t) = sigma2_g,t G^{-1}, sigma2_g,t being tblup_loglik_cov_batch's
 *   fitness      : optional out, batch: tblup_fit_cov_batch's, bit for bit
 *   cov_effects / cov_center / intercept / center / effects : optional as a group (all NULL or none):
 *                  tblup_fit_cov_batch's, bit for bit
 * From the factor, with s_a the animal's solved column (tblup_reliability_batch) and S = L^{-1} R the covariates'
 * slab (tblup_fit_cov_batch):
 *   kernel form (M = V, R = Q~_T):  a_a = S^T s_a,  k_Ta^T V^{-1} k_Ta = |s_a|^2
 *   SNP form (M = W_T^T W_T / d + lambda I_k, R = W_T^T Q~_T; V^{-1} W_T = W_T M^{-1}, k_Ta = W_T w_a / d):
 *     a_a = S^T s_a / d,  k_Ta^T V^{-1} k_Ta = K_aa - lambda |s_a|^2 / d
 * No phenotype enters reliability, pev_total or cov_cov: with several traits one value per (model, animal).
 * A model whose G has a pivot that is not positive (tblup_fit_cov_batch's rule) and finite, d = 0 or a flagged
 * index gives NaN in every output of that model; K_aa = 0 gives NaN for that animal: not errors.  cov / n_cov
 * and their errors are tblup_fit_cov_batch's; animals and theirs tblup_reliability_batch's; idx / offsets / h2 /
 * branch, the index rules and the chunking tblup_fit_batch's.  batch == 0 returns 0 and writes nothing, as does
 * n_pred == 0 when none of cov_cov, fitness and the model group is asked for; n_pred == 0 with one of them given
 * still fills it.  The second solve behind the model group and fitness runs only when one of them is given.
 * A (model, animal) value depends neither on the list, the slab, the batch, the chunking nor on where the
 * right-hand sides live (TBLUP_RELIAB_LDS, TBLUP_SCORE_LDS): fixed-order sums, no atomics.  Host pointers,
 * synchronous.
 */
int tblup_reliability_cov_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov,
                                const int64_t* animals, int64_t n_pred, const int64_t* idx, const int64_t* offsets,
                                int64_t batch, double h2, int branch, double* fitness, double* cov_effects,
                                double* cov_center, double* intercept, double* center, double* effects,
                                double* reliability, double* pev_total, double* cov_cov);

/*
 * The same for the model with a class fixed effect that tblup_fit_group_batch fits: cov, n_cov, group, n_levels and
 * the design F = [Q, Z] as documented there, C_m = n_cov + n_levels - [snp] columns for a model, at most
 * TBLUP_MAX_FIXED.  With F~ in place of Q~ the three statistics are exactly tblup_reliability_cov_batch's:
 * G = F~_T^T V^{-1} F~_T = C C^T and, for a listed animal a (any row of the panel, in any split role or none) with
 * design row f~_a,
 *   a_a          = F~_T^T V^{-1} k_Ta                                           (C_m values)
 *   reliability  : out, batch x n_pred:  (k_Ta^T V^{-1} k_Ta - |C^{-1} a_a|^2) / K_aa: the level effects estimated,
 *                  not known; never above tblup_reliability_cov_batch's on Q alone
 *   pev_total    : optional out, batch x n_pred:  K_aa - k_Ta^T V^{-1} k_Ta + |C^{-1} (f~_a - a_a)|^2: the error variance
 *                  of a predicted record of the animal in its own level, in units of sigma2_g
 *   fixed_cov    : optional out, batch x (n_cov + n_levels) x (n_cov + n_levels), covariates then levels:  G^{-1}, in
 *                  units of sigma2_g.  Under snp the row and the column of the reference level (the lowest) are exact
 *                  zeros: its effect is 0 by construction
 *   fitness      : optional out, batch: tblup_fit_group_batch's, bit for bit
 *   cov_effects / cov_center / group_effects / group_center / intercept / center / effects : optional as a group
 *                  (all NULL or none; cov_effects / cov_center only with n_cov > 0): tblup_fit_group_batch's, bit for bit
 * f~_a: a covariate's entry is tblup_reliability_cov_batch's q~_a; a level's is [code_a == level] under gblup and
 * [code_a == level] - share_level under snp, the lowest level dropped.  A listed animal whose code is -1 (a label that
 * no train animal has) is not an argument error: its reliability needs no design row and is defined, its pev_total is
 * NaN.  On a row of the split -1 stays the argument error it is in tblup_fit_group_batch.
 * From the factor, with s_a the animal's solved column and S = L^{-1} R in 16-column slabs (tblup_fit_group_batch):
 *   kernel form:  a_a = S^T s_a          SNP form:  a_a = S^T s_a / d
 * (no allele counts per level are needed, unlike tblup_snp_score_group_batch's SNP form).  A batch model of 1 .. 16
 * columns runs tblup_reliability_cov_batch's own kernels on the expanded design: its outputs are that entry's on
 * [Q, Z] bit for bit, fixed_cov scattered to the layout above.  A wider one keeps tblup_fit_group_batch's GLS step --
 * S, C, the bad flag -- and behind it T = S^T s_a (C_m x 16 per slab of listed animals) on fp64 MFMA, one wave per
 * column slab over the real rows in order; C y = a_a and C x = f~_a - a_a together, column by column, with |y|^2 and
 * |x|^2 on the way; and G^{-1} from C^{-1}, formed in place in LDS, G^{-1}(i, j) one chain over k >= max(i, j) in order
 * (the same bits at (i, j) and (j, i)).
 * NaN in every output of a model whose design is collinear over the train rows (a covariate equal to a level's
 * indicator, a column of ones beside gblup levels), with d = 0 or a flagged index; K_aa = 0 gives NaN for the
 * animal: not errors.  Argument errors are tblup_fit_group_batch's and, for animals, tblup_reliability_batch's; the
 * empty-call rules, the second solve only when fitness or the model group is given, the chunking and the bits'
 * independence of the list, the slab, the batch, the chunking, TBLUP_RELIAB_LDS, TBLUP_SCORE_LDS and
 * TBLUP_WORKSPACE_MB are tblup_reliability_cov_batch's.  Host pointers, synchronous.
 */
int tblup_reliability_group_batch(tblup_ctx* ctx, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                                  int64_t n_levels, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                                  const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                                  double* cov_effects, double* cov_center, double* group_effects,
                                  double* group_center, double* intercept, double* center, double* effects,
                                  double* reliability, double* pev_total, double* fixed_cov);

/*
 * EBVs of `n_pred` animals of the context's panel under `batch` fitted models (the formula above
 * on the device panel): ebv is batch x n_traits x n_pred.  `animals` are row ids in any order, may
 * repeat and need not belong to any split; no split is needed, only a panel (TBLUP_ERR_STATE on a
 * DE / decode-only context).  Models are portable between contexts: predicting newly genotyped
 * candidates means a context on their genotype matrix (same SNP columns) and the same model.
 * idx follows tblup_eval_batch's index rules (negative indices wrap, TBLUP_ERR_INDEX outside
 * [-n_snps, n_snps)); intercept / center / effects are laid out as tblup_fit_batch writes them.
 * Every animal's sum over j runs in list order in one chain, so the same call gives the same bits
 * twice and an animal's EBV depends neither on n_pred nor on its position in `animals`.
 * Host pointers, synchronous.
 */
int tblup_predict_batch(tblup_ctx* ctx, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, const double* intercept, const double* center,
                        const double* effects, int64_t n_traits, double* ebv);

/*
 * tblup_eval_batch's computation on device-resident inputs/outputs, enqueued on `stream`
 * (a hipStream_t; NULL = the context's own stream) without synchronising.
 * d_idx / d_offsets / d_fitness / d_ebv are device pointers on the
 * context's device; h_offsets is the same batch+1 offsets on the host (used
 * for workspace sizing).  The workspace is shared with other calls on the
 * context: calls must be serialised on one stream.  Negative indices wrap as in
 * tblup_eval_batch; an individual with an index outside [-n_snps, n_snps) gets a NaN
 * fitness and raises the context's index-error flag (read it with tblup_index_error).
 */
int tblup_eval_batch_device(tblup_ctx* ctx, int split_id, const int64_t* d_idx,
                            const int64_t* d_offsets, const int64_t* h_offsets, int64_t batch,
                            double h2, int branch, double* d_fitness, double* d_ebv, void* stream);

/*
 * Every individual against each of n_splits registered splits (IntraGCVBlupParallelEvaluator's
 * k folds, tblup/evaluator.py:509-537, whose fitness is the mean over folds; or any split set):
 * fitness is n_splits x batch row-major (row f = split_ids[f]).  The splits' evaluations are
 * enqueued back to back on one stream with one upload of the index lists and one
 * synchronisation, instead of one tblup_eval_batch round trip per fold.  When the splits partition
 * one animal set (IntraGCV's folds), the exact genotype products are shared: in the SNP-space form
 * C_{T_f} = C_{T_all} - C_{V_f}, in the kernel (GRM) form one A_R A_R^T per individual that every
 * fold's system reads its counts from.  Same numbers as tblup_eval_batch per split, bit for bit.
 * Host pointers, synchronous.
 */
int tblup_eval_folds(tblup_ctx* ctx, const int* split_ids, int n_splits, const int64_t* idx, const int64_t* offsets,
                     int64_t batch, double h2, int branch, double* fitness);

/* Same on device-resident inputs / outputs (d_fitness: n_splits x batch), enqueued on `stream`
 * (NULL = the context's stream) without synchronising; h_offsets as in tblup_eval_batch_device. */
int tblup_eval_folds_device(tblup_ctx* ctx, const int* split_ids, int n_splits, const int64_t* d_idx,
                            const int64_t* d_offsets, const int64_t* h_offsets, int64_t batch, double h2, int branch,
                            double* d_fitness, void* stream);

/*
 * RandomKeyIndividual / CoevolutionIndividual genome decode
 * (tblup/individual.py:154-156, `np.argsort(keys)[-int(length):]`): for each of
 * `batch` key rows of length d, the indices of its k_b = offsets[b+1]-offsets[b]
 * largest keys in ascending key order, written to idx_out[offsets[b] ...] — the
 * (idx, offsets) pair tblup_eval_batch takes.  Equal keys are ordered by index (a
 * stable argsort), so a tie straddling the k-th position selects its largest
 * indices; with continuous keys this is the set numpy's default sort returns.
 * Keys compare as numpy compares them: -0.0 equals +0.0, and every NaN (either
 * sign bit, any payload) is equal to every other NaN and sorts above +inf.
 * 1 <= k_b <= min(d, 8192).  Host pointers, synchronous.
 */
int tblup_decode_topk(tblup_ctx* ctx, const double* keys, int64_t batch, int64_t d, const int64_t* offsets,
                      int64_t* idx_out);

/*
 * Same on device-resident keys (row stride ld >= d doubles), offsets and output,
 * enqueued on `stream` (NULL = the context's stream); h_offsets is the host copy
 * (validation).  The output feeds tblup_eval_batch_device directly.
 */
int tblup_decode_topk_device(tblup_ctx* ctx, const double* d_keys, int64_t batch, int64_t d, int64_t ld,
                             const int64_t* d_offsets, const int64_t* h_offsets, int64_t* d_idx_out,
                             void* stream);

/*
 * Per-kernel-class timing with HIP events on the launch stream.
 * tblup_set_profiling(ctx, 1) enables recording; tblup_get_profile returns
 * accumulated milliseconds, launch counts and algorithmic flops per class
 * since the last reset (classes: 0 stats, 1 gather, 2 grm, 3 chol_diag,
 * 4 chol_offdiag, 5 solve).  Arrays must hold TBLUP_N_KCLASS entries.
 */
#define TBLUP_N_KCLASS 6
int tblup_set_profiling(tblup_ctx* ctx, int enable);
int tblup_get_profile(tblup_ctx* ctx, double* ms, int64_t* launches, double* flops, double* bytes);
int tblup_reset_profile(tblup_ctx* ctx);

/*
 * Workgroup trace (profiling; enabled by TBLUP_WG_TRACE=1 at tblup_ctx_create): after an
 * evaluation, the Cholesky launches of its last chunk left one record per workgroup,
 * 4 x uint64 {start, end, kind << 56 | I << 40 | individual, J} with s_memrealtime
 * timestamps (100 MHz) and kind 1 diagonal tile, 2 off-diagonal tile (I, J), 3 preparation
 * of diagonal tile I, 4 K_II build.  *n_records = records available; copies min(cap, that).
 */
int tblup_get_wg_trace(tblup_ctx* ctx, uint64_t* out, int64_t cap, int64_t* n_records);

/*
 * Debug / parity readback for ONE individual: runs the pipeline up to
 * `stage` (1 = GRM block K_{RT} incl. lambda on the TT diagonal,
 * 2 = after the tile Cholesky: L in the TT lower triangle) and copies the
 * (n_train + n_valid) x n_train block to `out` (row-major, R = train then
 * valid order), plus z = L^{-1}(y_T - mu) to `z_out` (may be NULL).
 */
int tblup_debug_grm(tblup_ctx* ctx, int split_id, const int64_t* idx, int64_t k, double h2,
                    int branch, int stage, double* out, double* z_out);

/*
 * VanRaden GRM of the selected columns over ALL animals, make_grm(data[:, idx])
 * (tblup/utils.py:7-18): G = W W^T / (2 sum p(1-p)), W = Z - 2p, p = column mean / 2.
 * Exact-integer A A^T on int8 MFMA (2-bit packed rows unpacked into LDS) plus the fp64 rank-1
 * centring (k_grm).  `G` is
 * n_animals x n_animals row-major (host).  Used by the PCA splitter
 * (pca_splitter, evaluator.py:641-663, with idx = every SNP).  Synchronous.
 */
int tblup_grm(tblup_ctx* ctx, const int64_t* idx, int64_t k, double* G);

/*
 * Per-SNP sums over the animal rows `rows` (n_rows ids, any order): sx = sum x,
 * sxx = sum x^2 (exact), sxy = sum x * yc (fp64; yc = the caller's centred phenotypes
 * of those rows), for every SNP of the panel (outputs of length n_snps, host).  The data
 * pass of the seeder's GWAS metric (sklearn f_regression over X[train],
 * tblup/seeder.py:144-160, 202-210).  Synchronous.
 */
int tblup_snp_scan(tblup_ctx* ctx, const int64_t* rows, int64_t n_rows, const double* yc, int64_t* sx,
                   int64_t* sxx, double* sxy);

/*
 * One differential-evolution generation (mutation + binary crossover + clip) for a
 * population of `pop` internal genomes of length L, bit-exact to the reference:
 *   TBLUP_DE_RAND_1            DERandOneEvolver.de_rand_one   tblup/evolver.py:103-138
 *                              donors[i] = (a, b, c):   mutant = a + F (b - c)
 *   TBLUP_DE_CURRENT_TO_BEST_1 DECurrentToBestOneEvolver.de_currenttobest_one  evolver.py:179-221
 *                              donors[i] = (best, a, b): mutant = x + F (best - x) + F (a - b)
 *   crossover (evolver.py:63-82): child_j = mutant_j where u_j < cr or j == fixed[i], else x_j,
 *   u = numpy's legacy np.random.rand(L) for individual i; clip (np.clip(., 0, clip_hi)) when clip.
 * The donors and `fixed` are the caller's python-`random` draws (exclusive_randrange,
 * random.randrange: utils.py:21-36, evolver.py:76).  mt_key / mt_pos hold numpy's global
 * MT19937 state (np.random.get_state()[1:3]) before the generation's first
 * np.random.rand call; on return they hold the state after all pop x 2L outputs, in
 * numpy's own representation (np.random.set_state continues the stream exactly).
 * Host pointers (parents/children: pop x L doubles), synchronous.
 */
enum { TBLUP_DE_RAND_1 = 0, TBLUP_DE_CURRENT_TO_BEST_1 = 1 };
int tblup_de_step(tblup_ctx* ctx, int strategy, const double* parents, int64_t pop, int64_t L,
                  const int32_t* donors, const int64_t* fixed, double F, double cr, int clip, double clip_hi,
                  uint32_t* mt_key, int32_t* mt_pos, double* children);

/* Same with device-resident parents / children (row strides ld, ldc >= L doubles) enqueued on
 * `stream` (NULL = the context's stream); donors, fixed and the MT state are host arrays.
 * Synchronises `stream` before returning (the new MT state is read back). */
int tblup_de_step_device(tblup_ctx* ctx, int strategy, const double* d_parents, int64_t pop, int64_t L, int64_t ld,
                         const int32_t* donors, const int64_t* fixed, double F, double cr, int clip, double clip_hi,
                         uint32_t* mt_key, int32_t* mt_pos, double* d_children, int64_t ldc, void* stream);

/* tblup_de_step_device in two halves: the step and the copy of the new MT state into a
 * page-locked context buffer are enqueued on `stream` without waiting (mt_key is read before
 * returning; mt_pos is passed by value), and tblup_de_state_wait waits for that copy only and
 * writes the state out.  Between the two the caller may enqueue work on the children (the
 * evaluator's decode and evaluation, their copy to the host); one step may be pending at a time.
 * tblup_de_step_device is the two calls back to back. */
int tblup_de_step_device_async(tblup_ctx* ctx, int strategy, const double* d_parents, int64_t pop, int64_t L,
                               int64_t ld, const int32_t* donors, const int64_t* fixed, double F, double cr, int clip,
                               double clip_hi, const uint32_t* mt_key, int32_t mt_pos, double* d_children,
                               int64_t ldc, void* stream);
int tblup_de_state_wait(tblup_ctx* ctx, uint32_t* mt_key, int32_t* mt_pos);

/* tblup_de_step_device_async with a strategy, mutation factor and crossover rate per individual
 * (host arrays of pop): the adaptive evolvers' generation -- SaDE (tblup/evolver.py:407-547) draws
 * each individual's strategy (DE/rand/1 or DE/current-to-best/1, python's random.random() < p)
 * and its crossover rate, with one F per generation.  Same numpy stream layout (one
 * np.random.rand(L) per individual, in order); completed by tblup_de_state_wait. */
int tblup_de_step_device_async_mix(tblup_ctx* ctx, const int32_t* strategies, const double* F, const double* cr,
                                   const double* d_parents, int64_t pop, int64_t L, int64_t ld, const int32_t* donors,
                                   const int64_t* fixed, int clip, double clip_hi, const uint32_t* mt_key,
                                   int32_t mt_pos, double* d_children, int64_t ldc, void* stream);

/* Enqueue dst row i (L doubles, row stride ldd) = the device row d_src_rows[i] (a host array of
 * n device pointers, each to L doubles on this context's device) on `stream` (NULL = the
 * context's stream): one launch per 128 rows.  The DE step's parents gathered from the rows
 * where earlier generations' children still sit on the device (tblup_amd.keystore), as the
 * reference's evolver reads population[i].get_internal_genome() (evolver.py:130-140). */
int tblup_gather_rows(tblup_ctx* ctx, double* d_dst, int64_t n, int64_t L, int64_t ldd, const double* const* d_src_rows,
                      void* stream);

/* Host-only: advance numpy's MT19937 (key[624], pos) state by n_words 32-bit outputs
 * (GF(2) jump-ahead; used to check the DE step's stream arithmetic without a GPU). */
int tblup_mt19937_jump(const uint32_t* key, int32_t pos, uint64_t n_words, uint32_t* key_out, int32_t* pos_out);

/* Host-only: one DE generation's python-`random` draws, the loops of DERandOneEvolver /
 * DECurrentToBestOneEvolver.evolve that feed tblup_de_step: per individual i the donors
 * (exclusive_randrange, utils.py:21-36; rand/1: a, b, c, evolver.py:118-121; current-to-best/1:
 * a, b beside `best`, evolver.py:199-203, donors[i] = (best, a, b)) and then fixed[i] =
 * random.randrange(0, L) (evolver.py:76).  py_mt / py_index hold CPython's MT19937 state
 * (random.getstate()[1]: 624 words, then the index) and are advanced in place exactly as the
 * python loop advances it (random.setstate continues the stream).  best = -1 for rand/1.
 * Needs 4 <= pop (smaller populations raise the reference's assertion: keep those in python). */
int tblup_de_donors(int strategy, int64_t pop, int64_t L, int32_t best, uint32_t* py_mt, int32_t* py_index,
                    int32_t* donors, int64_t* fixed);

/*
 * One MDE_pBX generation (MDE_pBX.evolve, tblup/evolver.py:550-687) in two device halves with a
 * host resolve between them.  Per individual i the reference draws
 *   best = population[np.random.choice(q_best, 1)], parent = np.random.choice(p_best, 1)
 * and then runs de_currenttobest_one on population[parent] (exclusive_randrange twice, randrange,
 * np.random.rand(L)).  Legacy np.random.choice(arr, 1) takes no MT19937 word for a single-entry
 * array and otherwise one word per attempt of `word & mask <= n - 1` (mask = 2^bit_length(n-1) - 1),
 * so individual i's uniforms start at word 2 L i + C_i of the generation's numpy stream, C_i = the
 * words the choices of individuals 0..i took.
 *
 * tblup_mde_windows (host-only): the stream offsets past 2 L i that a choice of individual i can
 * read, [lo[i], hi[i]) -- lo[i] the certain minimum of C_{i-1}, hi[i] the expected C_i plus slack
 * (slack < 0: six standard deviations + 16 words; slack >= 0: that many words and no deviation
 * term, for tests that force an overflow) -- and off[i] (pop + 1 entries), where that run starts in
 * the compact word buffer of *n_words = off[pop] words.  lo / hi / off may be NULL.
 *
 * tblup_mde_draws: enqueues on `stream` (NULL = the context's) the jump to every individual's
 * window and the expansion of those runs, copies the tempered words into `words` (host, n_words as
 * tblup_mde_windows gives for the same pop, nq, np, slack) and waits for them.  mt_key / mt_pos:
 * numpy's state before the generation's first choice; it is not advanced.
 *
 * tblup_mde_resolve (host-only, no context): sequentially over i, the two choices from `words`
 * (q_best[.] / p_best[.]: the population indices of the nq group bests and np parents to choose
 * from), C_i into c_words[i], and python's draws on (py_mt, py_index) as tblup_de_donors makes
 * them, with exclusions [parent_i, best_i] then a: donors[i] = (best_i, a, b), fixed[i],
 * parent[i].  *overflow = 1 when a rejection run left its window: the outputs are then undefined
 * and (py_mt, py_index) untouched -- the caller runs the generation on the host instead.
 *
 * tblup_mde_step_device_async: the step for the resolved draws, asynchronous like
 * tblup_de_step_device_async and completed by tblup_de_state_wait (numpy's state after all
 * 2 L pop + C_pop words): child i = DE/current-to-best/1 on row parent[i] with F[i], cr[i]
 * (host arrays of pop), uniforms from word 2 L i + c_words[i].  It continues the last
 * tblup_mde_draws of the same context, which must have been given the same pop, L and MT state
 * (TBLUP_ERR_STATE otherwise); c_words must be non-decreasing and within those draws' windows
 * (c_words[pop-1] <= hi[pop-1], as tblup_mde_resolve guarantees); one step may be pending at a
 * time.  Needs 4 <= pop.
 */
int tblup_mde_windows(int64_t pop, int64_t nq, int64_t np, int32_t slack, int32_t* lo, int32_t* hi, int64_t* off,
                      int64_t* n_words);
int tblup_mde_draws(tblup_ctx* ctx, int64_t pop, int64_t L, int64_t nq, int64_t np, int32_t slack,
                    const uint32_t* mt_key, int32_t mt_pos, uint32_t* words, int64_t n_words, void* stream);
int tblup_mde_resolve(int64_t pop, int64_t L, const int32_t* q_best, int64_t nq, const int32_t* p_best, int64_t np,
                      int32_t slack, const uint32_t* words, int64_t n_words, uint32_t* py_mt, int32_t* py_index,
                      int32_t* parent, int32_t* donors, int64_t* fixed, int64_t* c_words, int32_t* overflow);
int tblup_mde_step_device_async(tblup_ctx* ctx, const double* F, const double* cr, const double* d_parents,
                                int64_t pop, int64_t L, int64_t ld, const int32_t* parent, const int32_t* donors,
                                const int64_t* fixed, const int64_t* c_words, int clip, double clip_hi,
                                const uint32_t* mt_key, int32_t mt_pos, double* d_children, int64_t ldc,
                                void* stream);

/* Index-error flag of the device entry points: synchronises `stream` (NULL = the context's
 * stream), sets *flag = 1 if any individual evaluated since the last call had an index
 * outside [-n_snps, n_snps) (its fitness is NaN), and clears the flag. */
int tblup_index_error(tblup_ctx* ctx, void* stream, int* flag);

/* Solve-error flag: the chained back substitution (SNP form, small batches) hands block rows
 * between workgroups and bounds every wait; a wait that gives up leaves the batch's fitnesses
 * invalid.  The synchronous entries (tblup_eval_batch, tblup_eval_folds) recover by themselves
 * (the chunk's solve re-run through k_solve; tblup_chain_recoveries counts it) and never raise
 * this flag; after device entries read it here: synchronises `stream` (NULL = the context's
 * stream), *flag = 1 if a wait expired since the last read, clears it -- the caller re-evaluates
 * through a synchronous entry (the drop-in evaluator does).  (The reference has no such failure
 * mode -- a dead worker hangs its parent, tblup/evaluator.py:397-398; here it is an error or a
 * recovery, never a silent NaN.) */
int tblup_solve_error(tblup_ctx* ctx, void* stream, int* flag);

/* Number of chunks the synchronous entries re-solved after an expired chained-solve wait since
 * the context was created (each one cost one extra back substitution). */
int tblup_chain_recoveries(tblup_ctx* ctx, int64_t* count);

/* Both status words without synchronising: enqueues on `stream` (NULL = the context's stream) a
 * copy of {index error, solve error} (2 x int32, nonzero = raised) into `host_status`
 * (page-locked host memory) and clears them on the device; valid once the stream has passed
 * that point (the caller's event). */
int tblup_status_async(tblup_ctx* ctx, void* stream, int32_t* host_status);

/* Page-lock `bytes` of existing host memory at `ptr` for DMA (hipHostRegister) / release it.  The
 * multi-rank generation path registers the node-shared memory segments the ranks' shards of the
 * children's genomes are copied into (tblup_amd/shmrows.py), so each rank's device-to-host copy of
 * its shard runs as a DMA straight into the shared rows. */
int tblup_host_register(void* ptr, int64_t bytes);
int tblup_host_unregister(void* ptr);

/* Device memory currently held by the context (bytes). */
int tblup_mem_info(tblup_ctx* ctx, int64_t* bytes_in_use);

#ifdef __cplusplus
}
#endif

#endif /* TBLUP_GPU_H */
