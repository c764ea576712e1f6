// C ABI of libtblup_gpu.so (include/tblup_gpu.h), the host entries that read the factor the evaluation's
// pipeline leaves in the workspace, each one function on the host-batch driver of capi_ctx.h.  Its body carves
// the entry's buffers (a *Bufs struct below; the chunker measures the same carve), runs the pipeline and then:
//   tblup_fit_batch          k_effects
//   tblup_reliability_batch  k_reliab's launches, k_effects when the model is wanted too
//   tblup_loo_batch          k_effects for the solution alone, k_loo's launches, k_loo_fitness
//   tblup_snp_score_batch    k_snpscore's launches
//   tblup_loglik_batch       the pipeline once per h2 row, k_loglik behind each
//   tblup_fit_cov_batch      k_covar, a second solve, k_cov_fitness, k_effects when the model is wanted
//   tblup_snp_score_cov_batch  k_covar in keep mode, k_snpscore's covariate-adjusted launches
//   tblup_loglik_cov_batch     the pipeline once per h2 row, k_covar in keep mode and k_loglik behind each
//   tblup_reliability_cov_batch  k_covar in keep mode, k_reliab's covariate-adjusted launches, k_cov_cov;
//                                tblup_fit_cov_batch's second pass when the model or its fitness is wanted
//   tblup_fit_group_batch      models of up to 16 columns: tblup_fit_cov_batch on the expanded design; wider ones:
//                              k_fixed_subst, k_fixed_gls, a second solve, k_fixed_fitness, k_effects when wanted
//   tblup_snp_score_group_batch  models of up to 16 columns: tblup_snp_score_cov_batch on the expanded design; wider
//                              ones: k_fixed_subst, k_fixed_gls in keep mode, k_snpscore's wide-design launches
//   tblup_loglik_group_batch   the same routes: tblup_loglik_cov_batch, or per h2 row k_fixed_subst, k_fixed_gls in
//                              keep mode and k_loglik with the model's own column count
//   tblup_reliability_group_batch  the same routes: tblup_reliability_cov_batch, or k_fixed_subst, k_fixed_gls in keep
//                              mode, k_reliab's wide-design launches and k_fixed_cov; tblup_fit_group_batch's second
//                              pass when the model or its fitness is wanted
// tblup_predict_batch (k_predict) runs no pipeline: its own chunks, of PredictBufs alone.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "capi_ctx.h"

using namespace tblup;
using namespace tblup_capi;

namespace {

// The fitted model of a chunk (the reliabilities and the covariates carve it first if their caller wants it)
struct ModelBufs {
  double *cen, *eff;   // centres [sum_k], effects [nt][sum_k]
  static ModelBufs carve(Carve& cv, const HostBatch& hb, int64_t sum_k, bool wanted = true) {
    if (!wanted) return {};
    return {cv.take<double>((size_t)sum_k), cv.take<double>((size_t)hb.d.nt * sum_k)};
  }
  // k_effects on cl's factor and z, then the chunk's stretch of center and of every trait plane of effects
  int enqueue(const HostBatch& hb, const Chunk& ck, const CholLaunch& cl, double* center, double* effects) const {
    const hipStream_t s = hb.c->stream;
    const int64_t at = hb.offsets[ck.b0], total = hb.offsets[hb.batch];
    HIPCHK(launch_effects(cl, (const int32_t*)hb.c->colsum_all.p, cen, eff, ck.sum_k, s));
    HIPCHK(hipMemcpyAsync(center + at, cen, (size_t)ck.sum_k * 8, hipMemcpyDeviceToHost, s));
    for (int t = 0; t < hb.d.nt; ++t)
      HIPCHK(hipMemcpyAsync(effects + (int64_t)t * total + at, eff + (int64_t)t * ck.sum_k, (size_t)ck.sum_k * 8,
                            hipMemcpyDeviceToHost, s));
    return 0;
  }
};

// intercept [batch][nt]: the split's mean(y_T) the evaluation uses under snp, 0 under gblup
void fill_intercepts(const HostBatch& hb, double* intercept) {
  const int nt = hb.d.nt;
  for (int64_t b = 0; b < hb.batch; ++b) {
    const int mode = branch_of(hb.c, hb.offsets[b + 1] - hb.offsets[b], hb.branch);
    for (int t = 0; t < nt; ++t) intercept[b * nt + t] = mode == 2 ? hb.sp->meanyT[t] : 0.0;
  }
}

// A list's slab plan: the slices of a launch aim at a quarter of the workspace budget, RELIAB_SCRATCH at most
SlabPlan plan_slabs(const HostBatch& hb, int64_t B, int64_t n_items, int lds_knob) {
  return slab_plan(hb.sd, B, n_items, lds_knob != 0, std::min<int64_t>(RELIAB_SCRATCH, (int64_t)(hb.c->budget / 4)));
}
double* carve_slices(Carve& cv, const SlabPlan& p) { return p.lds ? nullptr : cv.take<double>(p.scratch()); }

struct ReliabBufs {   // tblup_reliability_batch
  ModelBufs m;
  SlabPlan plan;
  int32_t* an;          // the animal list [n_rel]
  double *rel, *vscr;   // reliabilities [B][n_rel]; the slices of one launch's slabs
  static ReliabBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t n_rel, bool model) {
    const SlabPlan p = plan_slabs(hb, B, n_rel, hb.c->reliab_lds);
    return {ModelBufs::carve(cv, hb, sum_k, model), p, cv.take<int32_t>((size_t)n_rel),
            cv.take<double>((size_t)B * n_rel), carve_slices(cv, p)};
  }
};

struct LooBufs {   // tblup_loo_batch
  SlabPlan plan;        // an n_T-item list; the knob is k_reliab's, TBLUP_RELIAB_LDS
  int32_t* tr;          // the train animals' rows of the panel [n_T]
  double* alpha;        // the solution k_effects leaves [B][nt][ns]
  double *pred, *lev;   // y^_loo [B][nt][n_T]; leverages [B][n_T]
  double *rfit, *press; // |r| and PRESS per (model, trait) [B][nt]
  double* vscr;         // the slices of one launch's slabs
  static LooBufs carve(Carve& cv, const HostBatch& hb, int64_t B) {
    const EvalDims& d = hb.d;
    const SlabPlan p = plan_slabs(hb, B, d.nT, hb.c->reliab_lds);
    const size_t Bt = (size_t)B * d.nt;
    return {p, cv.take<int32_t>((size_t)d.nT), cv.take<double>(Bt * hb.sd.ns), cv.take<double>(Bt * d.nT),
            cv.take<double>((size_t)B * d.nT), cv.take<double>(Bt), cv.take<double>(Bt), carve_slices(cv, p)};
  }
};

struct ScoreBufs {   // tblup_snp_score_batch
  SlabPlan plan;
  int32_t* cand;                    // the SNP list [n_cand]
  double *sco, *inf, *q, *vscr;     // score [B][nt][n_cand], info [B][n_cand], q [B][nt]; the slices
  static ScoreBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_cand) {
    const SlabPlan p = plan_slabs(hb, B, n_cand, hb.c->score_lds);
    const size_t nt = (size_t)hb.d.nt;
    return {p, cv.take<int32_t>((size_t)n_cand), cv.take<double>(B * nt * n_cand), cv.take<double>((size_t)B * n_cand),
            cv.take<double>(B * nt), carve_slices(cv, p)};
  }
};

struct LogLikBufs {   // tblup_loglik_batch, every pass of the chunk
  double *h2, *fits, *ll, *s2;   // h2 rows and fitnesses [n_h2][B]; log-likelihoods and sigma2_g [n_h2][B][nt]
  static LogLikBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_h2) {
    const size_t n = (size_t)n_h2 * B;
    return {cv.take<double>(n), cv.take<double>(n), cv.take<double>(n * hb.d.nt), cv.take<double>(n * hb.d.nt)};
  }
};

struct CovBufs {   // tblup_fit_cov_batch
  ModelBufs m;
  SlabPlan plan;       // one slab per model: a COVAR_W-item list; the knob is k_snpscore's, TBLUP_SCORE_LDS
  double *qT, *qV;     // the covariates of the train and of the validation rows, both planes
  double *b, *z2;      // their fitted effects [B][nt][n_cov]; z of the adjusted phenotype [B][nt][ns]
  double *fit0, *ebv2, *vscr;   // the first pass's fitness (not returned); the second solve's EBVs; the slices
  static CovBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t n_cov, bool model) {
    const EvalDims& d = hb.d;
    const SlabPlan p = plan_slabs(hb, B, COVAR_W, hb.c->score_lds);
    const size_t Bt = (size_t)B * d.nt;
    return {ModelBufs::carve(cv, hb, sum_k, model), p, cv.take<double>((size_t)2 * COVAR_W * d.nTp),
            cv.take<double>((size_t)2 * COVAR_W * d.nV), cv.take<double>(Bt * n_cov), cv.take<double>(Bt * hb.sd.ns),
            cv.take<double>((size_t)B), cv.take<double>(Bt * d.nV), carve_slices(cv, p)};
  }
};

struct FixedBufs {   // tblup_fit_group_batch, the models of more than COVAR_W columns (k_fixed.hip)
  ModelBufs m;
  SlabPlan plan;            // a Cw-item list; the slices of a plan without LDS are S's own slabs
  double *qT, *qV;          // CovBufs'
  int32_t *gT, *gV, *lst, *lpos;   // level codes of the train / validation rows; the train rows by level
  double *share, *ff, *fr;  // FixedDesign's
  double* S;                // [B][Cw / 16][ns][16]
  double *b, *z2;           // the fitted effects [B][nt][Cw]; z of the adjusted phenotype [B][nt][ns]
  double *fit0, *ebv2;      // CovBufs'
  static FixedBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t L, int64_t Cw, bool model) {
    const EvalDims& d = hb.d;
    const size_t Bt = (size_t)B * d.nt;
    FixedBufs f{ModelBufs::carve(cv, hb, sum_k, model), plan_slabs(hb, B, Cw, hb.c->score_lds)};
    f.qT = cv.take<double>((size_t)2 * COVAR_W * d.nTp);
    f.qV = cv.take<double>((size_t)2 * COVAR_W * d.nV);
    f.gT = cv.take<int32_t>((size_t)d.nTp);
    f.gV = cv.take<int32_t>((size_t)d.nV);
    f.lst = cv.take<int32_t>((size_t)L + 1);
    f.lpos = cv.take<int32_t>((size_t)d.nT);
    f.share = cv.take<double>((size_t)L);
    f.ff = cv.take<double>((size_t)Cw * Cw);
    f.fr = cv.take<double>((size_t)MAXT * Cw);
    f.S = cv.take<double>((size_t)B * Cw * hb.sd.ns);
    f.b = cv.take<double>(Bt * Cw);
    f.z2 = cv.take<double>(Bt * hb.sd.ns);
    f.fit0 = cv.take<double>((size_t)B);
    f.ebv2 = cv.take<double>(Bt * d.nV);
    return f;
  }
};

// What k_covar keeps of a chunk's GLS step for the covariate-adjusted score statistics and likelihood
// (CovKeep): one slab per model, planned as CovBufs plans it.  passes: the h2 rows whose effects are kept.
struct CovKeepBufs {
  SlabPlan plan;
  double* qT;            // the covariates of the train rows, both planes
  double* b;             // their fitted effects [passes][B][nt][n_cov]
  CovKeep keep;          // keep.sq doubles as the slices of a plan without LDS
  double* lqq;           // log|Q~_T^T Q~_T| of the two planes
  static CovKeepBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_cov, int64_t passes) {
    const SlabPlan p = plan_slabs(hb, B, COVAR_W, hb.c->score_lds);
    CovKeepBufs k{p, cv.take<double>((size_t)2 * COVAR_W * hb.d.nTp),
                  cv.take<double>((size_t)passes * B * hb.d.nt * n_cov), {}, nullptr};
    k.keep.sq = cv.take<double>((size_t)B * hb.sd.ns * COVAR_W);
    k.keep.cf = cv.take<double>((size_t)B * COVAR_W * COVAR_W);
    k.keep.ch = cv.take<double>((size_t)B * MAXT * COVAR_W);
    k.keep.ks = cv.take<double>((size_t)B * COVAR_KS);
    k.lqq = cv.take<double>(2);
    return k;
  }
  double* vscr() const { return plan.lds ? nullptr : keep.sq; }
};

struct ScoreCovBufs {   // tblup_snp_score_cov_batch
  ScoreBufs s;
  CovKeepBufs k;
  static ScoreCovBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_cand, int64_t n_cov) {
    const ScoreBufs s = ScoreBufs::carve(cv, hb, B, n_cand);
    return {s, CovKeepBufs::carve(cv, hb, B, n_cov, 1)};
  }
};

struct LogLikCovBufs {   // tblup_loglik_cov_batch
  LogLikBufs l;
  CovKeepBufs k;
  static LogLikCovBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_h2, int64_t n_cov) {
    const LogLikBufs l = LogLikBufs::carve(cv, hb, B, n_h2);
    return {l, CovKeepBufs::carve(cv, hb, B, n_cov, n_h2)};
  }
};

struct ReliabCovBufs {   // tblup_reliability_cov_batch
  ReliabBufs r;
  CovKeepBufs k;
  double *qa, *pev, *cc;            // the listed animals' covariates, both planes [2][n_rel][COVAR_W]; pev_total
                                    // [B][n_rel] and cov_cov [B][n_cov][n_cov] where wanted
  double *qV, *z2, *fit0, *ebv2;    // tblup_fit_cov_batch's second pass (CovBufs'), where wanted
  static ReliabCovBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t n_rel, int64_t n_cov,
                             bool model, bool full, bool pev, bool cc) {
    const EvalDims& d = hb.d;
    const size_t Bt = (size_t)B * d.nt;
    ReliabCovBufs b{ReliabBufs::carve(cv, hb, B, sum_k, n_rel, model), CovKeepBufs::carve(cv, hb, B, n_cov, 1)};
    b.qa = cv.take<double>((size_t)2 * n_rel * COVAR_W);
    b.pev = pev ? cv.take<double>((size_t)B * n_rel) : nullptr;
    b.cc = cc ? cv.take<double>((size_t)B * n_cov * n_cov) : nullptr;
    if (full) {
      b.qV = cv.take<double>((size_t)2 * COVAR_W * d.nV);
      b.z2 = cv.take<double>(Bt * hb.sd.ns);
      b.fit0 = cv.take<double>((size_t)B);
      b.ebv2 = cv.take<double>(Bt * d.nV);
    }
    return b;
  }
};

// The argument checks every covariate entry shares (tblup_fit_cov_batch's)
int check_cov(const tblup_ctx* c, const double* cov, int64_t n_cov) {
  if (n_cov < 1 || n_cov > COVAR_W) return fail(TBLUP_ERR_ARG, "need 1 <= n_cov <= 16");
  if (!cov) return fail(TBLUP_ERR_ARG, "null cov");
  for (int64_t i = 0; i < c->n * n_cov; ++i)
    if (!std::isfinite(cov[i])) return fail(TBLUP_ERR_ARG, "covariates must be finite");
  return 0;
}

// The covariates of the split's rows gathered once per call, covariate-major and zero-padded, as given
// (plane 0: gblup models) and centred by the column means over the train rows in split order (plane 1:
// snp models): m [n_cov], qT [2][COVAR_W][nTp], qV [2][COVAR_W][nV] (valid: wanted).
struct CovPlanes {
  std::vector<double> m, qT, qV;
};
CovPlanes gather_cov(const HostBatch& hb, const double* cov, int64_t n_cov, bool valid) {
  const EvalDims& d = hb.d;
  CovPlanes cp{std::vector<double>((size_t)n_cov), std::vector<double>((size_t)2 * COVAR_W * d.nTp, 0.0),
               std::vector<double>(valid ? (size_t)2 * COVAR_W * d.nV : 0, 0.0)};
  for (int64_t j = 0; j < n_cov; ++j) {
    long double acc = 0.0L;
    for (int64_t i = 0; i < d.nT; ++i) acc += cov[hb.sp->train[i] * n_cov + j];
    const double m = cp.m[j] = (double)(acc / (long double)d.nT);
    const auto planes = [&](const std::vector<int64_t>& rows, int64_t n_rows, int64_t ld, std::vector<double>& q) {
      for (int64_t i = 0; i < n_rows; ++i) {
        const double v = cov[rows[i] * n_cov + j];
        q[j * ld + i] = v;
        q[(COVAR_W + j) * ld + i] = v - m;
      }
    };
    planes(hb.sp->train, d.nT, d.nTp, cp.qT);
    if (valid) planes(hb.sp->valid, d.nV, d.nV, cp.qV);
  }
  return cp;
}

// log|Q~_T^T Q~_T| of a plane of qT in long double, by Cholesky under k_covar's pivot rule (COVAR_PIV_RTOL of
// the pivot's own diagonal entry); NaN for a plane that is not of full rank
double log_det_chol(long double* a, int64_t n);
double log_det_qq(const double* q, int64_t nT, int64_t nTp, int64_t n_cov) {
  long double a[COVAR_W * COVAR_W];
  for (int64_t i = 0; i < n_cov; ++i)
    for (int64_t j = 0; j <= i; ++j) {
      long double acc = 0.0L;
      for (int64_t r = 0; r < nT; ++r) acc += (long double)q[i * nTp + r] * (long double)q[j * nTp + r];
      a[i * n_cov + j] = acc;
    }
  return log_det_chol(a, n_cov);
}
// log|A| of a symmetric n x n matrix given by its lower triangle (row-major, stride n; overwritten by the factor),
// under the pivot rule above; NaN for one that is not of full rank
double log_det_chol(long double* a, int64_t n) {
  long double ld = 0.0L;
  for (int64_t k = 0; k < n; ++k) {
    const long double gkk = a[k * n + k];
    long double p = gkk;
    for (int64_t m = 0; m < k; ++m) p -= a[k * n + m] * a[k * n + m];
    if (!(p > (long double)COVAR_PIV_RTOL * gkk) || !std::isfinite((double)p)) return std::nan("");
    const long double ckk = std::sqrt(p);
    ld += 2.0L * std::log(ckk);
    for (int64_t i = k + 1; i < n; ++i) {
      long double v = a[i * n + k];
      for (int64_t m = 0; m < k; ++m) v -= a[i * n + m] * a[k * n + m];
      a[i * n + k] = v / ckk;
    }
    a[k * n + k] = ckk;
  }
  return (double)ld;
}

// The class factor of a tblup_fit_group_batch call on the host: the split rows' codes, the train rows by level,
// the levels' shares, and the snp design's cross products F~_T^T F~_T and F~_T^T r_t (long double, once per call:
// a row has n_cov + 1 non-zeros before centring, so they cost n_T (n_cov + 1)^2, not n_T C^2).
struct GroupDesign {
  int nc, L, Cw;
  CovPlanes cp;
  std::vector<int32_t> gT, gV, lst, lpos;
  std::vector<double> share, ff, fr;
};
GroupDesign gather_group(const HostBatch& hb, const double* cov, int64_t n_cov, const int64_t* group, int64_t L,
                         int64_t Cw) {
  const EvalDims& d = hb.d;
  const std::vector<int64_t>& T = hb.sp->train;
  const int nt = d.nt;
  GroupDesign g{(int)n_cov, (int)L, (int)Cw, gather_cov(hb, cov, n_cov, true)};
  g.gT.assign((size_t)d.nTp, -1);
  g.gV.assign((size_t)d.nV, -1);
  g.lst.assign((size_t)L + 1, 0);
  g.lpos.resize((size_t)d.nT);
  g.share.resize((size_t)L);
  for (int64_t i = 0; i < d.nT; ++i) ++g.lst[(g.gT[i] = (int32_t)group[T[i]]) + 1];
  for (int64_t i = 0; i < d.nV; ++i) g.gV[i] = (int32_t)group[hb.sp->valid[i]];
  for (int64_t l = 0; l < L; ++l) {
    g.share[l] = (double)((long double)g.lst[l + 1] / (long double)d.nT);
    g.lst[l + 1] += g.lst[l];
  }
  std::vector<int32_t> at(g.lst.begin(), g.lst.end() - 1);
  for (int64_t i = 0; i < d.nT; ++i) g.lpos[at[g.gT[i]]++] = (int32_t)i;
  // the snp design: columns 0 .. n_cov - 1 the covariates centred by their train means, then levels 1 .. L - 1
  // centred by their shares.  U = F_T^T F_T uncentred, F~^T F~ = U - n_T m m^T with m the train means.
  const int64_t C = n_cov + L - 1;
  std::vector<long double> U((size_t)C * C, 0.0L), m((size_t)C, 0.0L), fr((size_t)nt * C, 0.0L), sr((size_t)nt, 0.0L);
  for (int64_t j = 0; j < n_cov; ++j) m[j] = g.cp.m[j];
  for (int64_t l = 1; l < L; ++l) m[n_cov + l - 1] = g.share[l];
  for (int64_t i = 0; i < d.nT; ++i) {
    const double* q = cov + T[i] * n_cov;   // (not read when n_cov is 0)
    const int64_t zl = g.gT[i] >= 1 ? n_cov + g.gT[i] - 1 : -1;
    for (int64_t a = 0; a < n_cov; ++a) {
      for (int64_t e = 0; e <= a; ++e) U[a * C + e] += (long double)q[a] * (long double)q[e];
      if (zl >= 0) U[zl * C + a] += q[a];
    }
    if (zl >= 0) U[zl * C + zl] += 1.0L;
    for (int t = 0; t < nt; ++t) {
      const long double r = (long double)(hb.c->pheno[T[i] * nt + t] - hb.sp->meanyT[t]);
      sr[t] += r;
      for (int64_t a = 0; a < n_cov; ++a) fr[t * C + a] += (long double)q[a] * r;
      if (zl >= 0) fr[t * C + zl] += r;
    }
  }
  g.ff.assign((size_t)Cw * Cw, 0.0);
  g.fr.assign((size_t)MAXT * Cw, 0.0);
  if (C <= Cw) {
    for (int64_t a = 0; a < C; ++a)
      for (int64_t e = 0; e <= a; ++e)
        g.ff[a * Cw + e] = g.ff[e * Cw + a] = (double)(U[a * C + e] - (long double)d.nT * m[a] * m[e]);
    for (int t = 0; t < nt; ++t)
      for (int64_t a = 0; a < C; ++a) g.fr[t * Cw + a] = (double)(fr[t * C + a] - m[a] * sr[t]);
  }
  return g;
}

// log|F~_T^T F~_T| of the gblup design (plane 0: [Q, Z] as given, every level) and of the snp design (plane 1:
// centred, the lowest level dropped) in long double under log_det_qq's rule, once per call; NaN for a plane that
// is not of full rank, and for one that no model of the call has (need).  A row has n_cov + 1 non-zeros.  The snp
// plane sums the covariates centred, as log_det_qq does on gather_cov's centred plane, so a covariate whose mean is
// far above its spread loses nothing: Q~^T Z~ = Q~^T Z because Q~_T sums to zero, and Z~^T Z~ = diag(n_l) - n_l n_e / n_T
// from the integer counts.
void group_log_dets(const HostBatch& hb, const double* cov, const GroupDesign& g, const bool (&need)[2],
                    double (&lqq)[2]) {
  const std::vector<int64_t>& T = hb.sp->train;
  const int64_t nT = hb.d.nT, nc = g.nc, L = g.L;
  lqq[0] = lqq[1] = std::nan("");
  for (int plane = 0; plane < 2; ++plane) {
    if (!need[plane]) continue;
    const int64_t l0 = plane, C = nc + L - l0;   // the first level with a column; the plane's columns
    std::vector<long double> A((size_t)C * C, 0.0L), q((size_t)nc);
    for (int64_t i = 0; i < nT; ++i) {
      for (int64_t a = 0; a < nc; ++a)
        q[a] = (long double)cov[T[i] * nc + a] - (plane ? (long double)g.cp.m[a] : 0.0L);
      const int64_t zl = g.gT[i] >= l0 ? nc + g.gT[i] - l0 : -1;
      for (int64_t a = 0; a < nc; ++a) {
        for (int64_t e = 0; e <= a; ++e) A[a * C + e] += q[a] * q[e];
        if (zl >= 0) A[zl * C + a] += q[a];
      }
      if (zl >= 0) A[zl * C + zl] += 1.0L;
    }
    if (plane)
      for (int64_t a = nc; a < C; ++a)
        for (int64_t e = nc; e <= a; ++e) {
          const long double na = g.lst[a - nc + l0 + 1] - g.lst[a - nc + l0], ne = g.lst[e - nc + l0 + 1] - g.lst[e - nc + l0];
          A[a * C + e] -= na * ne / (long double)nT;
        }
    lqq[plane] = log_det_chol(A.data(), C);
  }
}

// What k_fixed_subst and k_fixed_gls in keep mode leave of a chunk's wide GLS step for the score statistics and the
// likelihood under the class factor (FixedBufs without the second pass).  passes: the h2 rows whose effects are kept.
struct FixedKeepBufs {
  SlabPlan plan;            // FixedBufs'
  double* qT;
  int32_t *gT, *lst, *lpos;
  double *share, *ff, *fr;
  double* S;                // [B][Cw / 16][ns][16]
  double* b;                // the fitted effects [passes][B][nt][Cw]
  FixedKeep keep;
  double* lqq;              // log|F~_T^T F~_T| of the two planes
  static FixedKeepBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t L, int64_t Cw, int64_t passes) {
    const EvalDims& d = hb.d;
    FixedKeepBufs f{plan_slabs(hb, B, Cw, hb.c->score_lds)};
    f.qT = cv.take<double>((size_t)2 * COVAR_W * d.nTp);
    f.gT = cv.take<int32_t>((size_t)d.nTp);
    f.lst = cv.take<int32_t>((size_t)L + 1);
    f.lpos = cv.take<int32_t>((size_t)d.nT);
    f.share = cv.take<double>((size_t)L);
    f.ff = cv.take<double>((size_t)Cw * Cw);
    f.fr = cv.take<double>((size_t)MAXT * Cw);
    f.S = cv.take<double>((size_t)B * Cw * hb.sd.ns);
    f.b = cv.take<double>((size_t)passes * B * d.nt * Cw);
    f.keep.cf = cv.take<double>((size_t)B * Cw * Cw);
    f.keep.ch = cv.take<double>((size_t)B * MAXT * Cw);
    f.keep.ks = cv.take<double>((size_t)B * COVAR_KS);
    f.lqq = cv.take<double>(2);
    return f;
  }
  FixedDesign design(const GroupDesign& g) const {
    return {qT, nullptr, gT, nullptr, lst, lpos, share, ff, fr, g.nc, g.L, g.Cw};
  }
  int upload(const GroupDesign& g, hipStream_t s) const {
    const auto up = [&](void* dst, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(up(qT, g.cp.qT.data(), g.cp.qT.size() * 8));
    HIPCHK(up(gT, g.gT.data(), g.gT.size() * 4));
    HIPCHK(up(lst, g.lst.data(), g.lst.size() * 4));
    HIPCHK(up(lpos, g.lpos.data(), g.lpos.size() * 4));
    HIPCHK(up(share, g.share.data(), g.share.size() * 8));
    HIPCHK(up(ff, g.ff.data(), g.ff.size() * 8));
    HIPCHK(up(fr, g.fr.data(), g.fr.size() * 8));
    return 0;
  }
};

// The models of more than COVAR_W fixed columns of a tblup_fit_group_batch call, as a batch of their own:
// bout [batch][nt][Cw] the fitted effects by column (zero past a model's own), everything else
// tblup_fit_cov_batch's.  A model whose effects are NaN is NaN in intercept and center too.
int fit_fixed_wide(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group, int64_t L,
                   int64_t Cw, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2, int branch,
                   double* fitness, double* ebv, double* bout, double* intercept, double* center, double* effects) {
  const bool model = intercept != nullptr;
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  if (!hb.sp) return 0;
  const EvalDims& d = hb.d;
  const int nt = d.nt;
  const GroupDesign g = gather_group(hb, cov, n_cov, group, L, Cw);
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) { return FixedBufs::carve(cv, hb, B, sk, L, Cw, model); };
  // per chunk: tblup_fit_cov_batch's, with k_fixed's three kernels in place of k_covar and k_cov_fitness
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const FixedBufs fb = carve(cv, B, ck.sum_k);
    if (int rc = ws_check(c, cv)) return rc;
    const auto up = [&](void* dst, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(up(fb.qT, g.cp.qT.data(), g.cp.qT.size() * 8));
    HIPCHK(up(fb.qV, g.cp.qV.data(), g.cp.qV.size() * 8));
    HIPCHK(up(fb.gT, g.gT.data(), g.gT.size() * 4));
    HIPCHK(up(fb.gV, g.gV.data(), g.gV.size() * 4));
    HIPCHK(up(fb.lst, g.lst.data(), g.lst.size() * 4));
    HIPCHK(up(fb.lpos, g.lpos.data(), g.lpos.size() * 4));
    HIPCHK(up(fb.share, g.share.data(), g.share.size() * 8));
    HIPCHK(up(fb.ff, g.ff.data(), g.ff.size() * 8));
    HIPCHK(up(fb.fr, g.fr.data(), g.fr.size() * 8));
    const FixedDesign fd{fb.qT, fb.qV, fb.gT, fb.gV, fb.lst, fb.lpos, fb.share, fb.ff, fb.fr, g.nc, g.L, g.Cw};
    double* d_fit = rq.d_fit;
    Carve cvp = cv;
    rq.mode = ChunkMode::NoChain;
    rq.d_fit = fb.fit0;
    ChunkRes res;
    if (int rc = run_chunk(c, rq, cvp, res)) return rc;
    HIPCHK(launch_fixed_subst(res.cl, fd, fb.plan, fb.S, s));
    HIPCHK(launch_fixed_gls(res.cl, fd, fb.S, fb.b, fb.z2, FixedKeep{}, s));
    CholLaunch cl2 = res.cl;
    cl2.z = fb.z2;
    HIPCHK(launch_solve(cl2, nullptr, fb.fit0, fb.ebv2, s));
    HIPCHK(launch_fixed_fitness(cl2, fd, fb.ebv2, fb.b, d_fit, s));
    if (model)
      if (int rc = fb.m.enqueue(hb, ck, cl2, center, effects)) return rc;
    HIPCHK(hipMemcpyAsync(bout + b0 * nt * Cw, fb.b, (size_t)B * nt * Cw * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fitness + b0, d_fit, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    if (ebv) HIPCHK(hipMemcpyAsync(ebv + b0 * nt * d.nV, fb.ebv2, (size_t)B * nt * d.nV * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
    return 0;
  });
  if (rc || !model) return rc;
  fill_intercepts(hb, intercept);
  const double nan = std::nan("");
  for (int64_t b = 0; b < batch; ++b) {
    // (a model without a fixed column has no effect to tell by: its fitness tells)
    const bool gblup = branch_of(c, offsets[b + 1] - offsets[b], branch) == 1;
    bool dead = fixed_cols(gblup, (int)n_cov, (int)L) == 0 && std::isnan(fitness[b]);
    for (int64_t i = 0; i < nt * Cw; ++i) dead = dead || std::isnan(bout[b * nt * Cw + i]);
    if (!dead) continue;
    for (int t = 0; t < nt; ++t) intercept[b * nt + t] = nan;
    for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i) center[i] = nan;
  }
  return 0;
}

// The argument checks the class-factor entries share (tblup_fit_group_batch's), before the split is known
int check_group(const tblup_ctx* c, const double* cov, int64_t n_cov, const int64_t* group, int64_t n_levels) {
  if (n_cov < 0 || n_cov > COVAR_W) return fail(TBLUP_ERR_ARG, "need 0 <= n_cov <= 16");
  if (n_cov > 0)
    if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (n_levels < 1) return fail(TBLUP_ERR_ARG, "need n_levels >= 1");
  if (!group) return fail(TBLUP_ERR_ARG, "null group");
  for (int64_t i = 0; i < c->n; ++i)
    if (group[i] < -1 || group[i] >= n_levels) return fail(TBLUP_ERR_ARG, "a level code lies outside [-1, n_levels)");
  return 0;
}

// ... and against the split: every animal of the split has a level and every level a train row.  share [L] the
// levels' shares n_l / n_T, cov_m the covariates' means over the train rows (gather_cov's).
struct GroupSplit {
  std::vector<long double> share;
  std::vector<double> cov_m;
  int64_t nT = 0, nV = 0;
  int nt = 1;
};
int check_group_split(const HostBatch& hb, const double* cov, int64_t nc, const int64_t* group, int64_t L,
                      GroupSplit& gs) {
  const int64_t nT = gs.nT = hb.d.nT, nV = gs.nV = hb.d.nV;
  gs.nt = hb.d.nt;
  gs.share.assign((size_t)std::min<int64_t>(L, hb.c->n + 1), 0.0L);
  gs.cov_m.resize((size_t)nc);
  if (L > nT) return fail(TBLUP_ERR_ARG, "a level has no train row");
  for (int64_t i = 0; i < nT; ++i) {
    if (group[hb.sp->train[i]] < 0) return fail(TBLUP_ERR_ARG, "an animal of the split has no level (-1)");
    gs.share[group[hb.sp->train[i]]] += 1.0L;
  }
  for (int64_t i = 0; i < nV; ++i)
    if (group[hb.sp->valid[i]] < 0) return fail(TBLUP_ERR_ARG, "an animal of the split has no level (-1)");
  for (int64_t l = 0; l < L; ++l) {
    if (gs.share[l] == 0.0L) return fail(TBLUP_ERR_ARG, "a level has no train row");
    gs.share[l] /= (long double)nT;
  }
  for (int64_t j = 0; j < nc; ++j) {
    long double acc = 0.0L;
    for (int64_t i = 0; i < nT; ++i) acc += cov[hb.sp->train[i] * nc + j];
    gs.cov_m[j] = (double)(acc / (long double)nT);
  }
  return 0;
}

// A model's columns follow its branch: n_cov + L under gblup, one less under snp (the reference level).
// Routes: 0 / 1 the gblup / snp models of 1 .. 16 columns, which run the covariate entry on the expanded design;
// 2 the others, one batch of both branches through k_fixed.
struct GroupRoutes {
  int64_t cols[2] = {0, 0};
  std::vector<int64_t> of[3];
  int64_t wide_cols = 0;
  // the column stride of a route's effects
  int64_t width(int route) const {
    return route == 2 ? std::max<int64_t>(COVAR_W, round_up(wide_cols, COVAR_W)) : cols[route];
  }
};
int route_group(const tblup_ctx* c, const int64_t* offsets, int64_t batch, int branch, int64_t nc, int64_t L,
                GroupRoutes& gr) {
  gr.cols[0] = fixed_cols(true, (int)nc, (int)L);
  gr.cols[1] = fixed_cols(false, (int)nc, (int)L);
  for (int64_t b = 0; b < batch; ++b) {
    const int br = branch_of(c, offsets[b + 1] - offsets[b], branch) == 1 ? 0 : 1;
    if (gr.cols[br] > FIXED_MAX)
      return fail(TBLUP_ERR_ARG, "more than 128 fixed columns (n_cov + levels; one less under snp)");
    const bool narrow = gr.cols[br] >= 1 && gr.cols[br] <= COVAR_W;
    gr.of[narrow ? br : 2].push_back(b);
    if (!narrow) gr.wide_cols = std::max(gr.wide_cols, gr.cols[br]);
  }
  return 0;
}

// a route's models as a batch of their own
struct SubBatch {
  std::vector<int64_t> so, si;
};
SubBatch sub_batch(const int64_t* idx, const int64_t* offsets, const std::vector<int64_t>& mb) {
  SubBatch sb{std::vector<int64_t>(mb.size() + 1, 0), {}};
  for (size_t i = 0; i < mb.size(); ++i) {
    sb.si.insert(sb.si.end(), idx + offsets[mb[i]], idx + offsets[mb[i] + 1]);
    sb.so[i + 1] = (int64_t)sb.si.size();
  }
  return sb;
}

// the expanded design [Q, Z] of route 0 / 1, [n][Cw]: every level under gblup, all but the lowest under snp; an
// animal without a level (outside the split) has a row of zeros in Z
std::vector<double> expand_design(const tblup_ctx* c, const double* cov, int64_t nc, const int64_t* group, int64_t Cw,
                                  int route) {
  std::vector<double> x((size_t)c->n * Cw, 0.0);
  for (int64_t a = 0; a < c->n; ++a) {
    for (int64_t j = 0; j < nc; ++j) x[a * Cw + j] = cov[a * nc + j];
    const int64_t z = group[a] - route;
    if (z >= 0) x[a * Cw + nc + z] = 1.0;
  }
  return x;
}

// a model's fitted effects by column (bt [nt][Cw]) as the covariates' and the levels' (0 at the reference level
// under snp, br = 1); either output may be null
void put_effects(const double* bt, int nt, int64_t Cw, int64_t nc, int64_t L, int br, bool dead, double* cov_eff,
                 double* grp_eff) {
  const double nan = std::nan("");
  for (int t = 0; t < nt; ++t) {
    if (cov_eff)
      for (int64_t j = 0; j < nc; ++j) cov_eff[t * nc + j] = dead ? nan : bt[t * Cw + j];
    if (grp_eff)
      for (int64_t l = 0; l < L; ++l) grp_eff[t * L + l] = dead ? nan : (l - br < 0 ? 0.0 : bt[t * Cw + nc + l - br]);
  }
}

struct ScoreFixedBufs {   // tblup_snp_score_group_batch, the models of more than COVAR_W columns
  ScoreBufs s;
  FixedKeepBufs k;
  static ScoreFixedBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_cand, int64_t L, int64_t Cw) {
    const ScoreBufs s = ScoreBufs::carve(cv, hb, B, n_cand);
    return {s, FixedKeepBufs::carve(cv, hb, B, L, Cw, 1)};
  }
};

struct LogLikFixedBufs {   // tblup_loglik_group_batch, the models of more than COVAR_W columns
  LogLikBufs l;
  FixedKeepBufs k;
  static LogLikFixedBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_h2, int64_t L, int64_t Cw) {
    const LogLikBufs l = LogLikBufs::carve(cv, hb, B, n_h2);
    return {l, FixedKeepBufs::carve(cv, hb, B, L, Cw, n_h2)};
  }
};

// The models of more than COVAR_W fixed columns of a tblup_snp_score_group_batch call, as a batch of their own:
// tblup_snp_score_cov_batch's chunk with k_fixed_subst and k_fixed_gls (keep mode) in place of k_covar and
// k_snpscore's FIX instances behind them.  bout [batch][nt][Cw]: fit_fixed_wide's.
int score_fixed_wide(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group, int64_t L,
                     int64_t Cw, const std::vector<int32_t>& s32, const int64_t* idx, const int64_t* offsets,
                     int64_t batch, double h2, int branch, double* fitness, double* score, double* info, double* q,
                     double* bout) {
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  if (!hb.sp) return 0;
  const int nt = hb.d.nt;
  const int64_t n_cand = (int64_t)s32.size();
  const GroupDesign g = gather_group(hb, cov, n_cov, group, L, Cw);
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return ScoreFixedBufs::carve(cv, hb, B, n_cand, L, Cw); };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ScoreFixedBufs sb = carve(cv, B, ck.sum_k);
    const FixedKeepBufs& kb = sb.k;
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpyAsync(sb.s.cand, s32.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
    if (int rc = kb.upload(g, s)) return rc;
    const FixedDesign fd = kb.design(g);
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      HIPCHK(launch_fixed_subst(cl, fd, kb.plan, kb.S, s));
      HIPCHK(launch_fixed_gls(cl, fd, kb.S, kb.b, nullptr, kb.keep, s));
      const ScoreFixed sf{kb.S, kb.keep.cf, kb.keep.ch, kb.keep.ks, fd};
      HIPCHK(launch_snpscore_fixed(cl, (const int32_t*)c->colsum_all.p, sb.s.cand, n_cand, sb.s.plan, sb.s.vscr, sf,
                                   sb.s.sco, sb.s.inf, sb.s.q, s));
      HIPCHK(hipMemcpyAsync(score + b0 * nt * n_cand, sb.s.sco, (size_t)B * nt * n_cand * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(info + b0 * n_cand, sb.s.inf, (size_t)B * n_cand * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(q + b0 * nt, sb.s.q, (size_t)B * nt * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(bout + b0 * nt * Cw, kb.b, (size_t)B * nt * Cw * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
}

// The same of a tblup_loglik_group_batch call: tblup_loglik_cov_batch's passes with k_fixed_subst and k_fixed_gls
// (keep mode, no z*) between the pipeline and k_loglik.  h2 [n_h2][batch]; bout [n_h2][batch][nt][Cw].
int loglik_fixed_wide(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group, int64_t L,
                      int64_t Cw, const int64_t* idx, const int64_t* offsets, int64_t batch, const double* h2,
                      int64_t n_h2, int branch, double* fitness, double* loglik, double* sigma2_g, double* bout) {
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2[0], branch, true)) return rc;
  if (!hb.sp) return 0;
  const int nt = hb.d.nt;
  const GroupDesign g = gather_group(hb, cov, n_cov, group, L, Cw);
  const int cols[2] = {fixed_cols(true, (int)n_cov, (int)L), fixed_cols(false, (int)n_cov, (int)L)};
  // log|F~_T^T F~_T| does not depend on h2: once per call, for the planes that the batch has models of
  bool need[2] = {false, false};
  for (int64_t b = 0; b < batch; ++b) need[branch_of(c, offsets[b + 1] - offsets[b], branch) == 1 ? 0 : 1] = true;
  double lqq[2];
  group_log_dets(hb, cov, g, need, lqq);
  // (a plane without a model is not read; its count only has to pass the launcher's range check)
  const int kcols[2] = {need[0] ? cols[0] : 0, need[1] ? cols[1] : 0};
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return LogLikFixedBufs::carve(cv, hb, B, n_h2, L, Cw); };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const size_t row = (size_t)B * 8, rowt = row * nt, pitch = (size_t)batch * 8;
    const LogLikFixedBufs lf = carve(cv, B, ck.sum_k);
    const LogLikBufs& lb = lf.l;
    const FixedKeepBufs& kb = lf.k;
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpy2DAsync(lb.h2, row, h2 + b0, pitch, row, (size_t)n_h2, hipMemcpyHostToDevice, s));
    if (int rc = kb.upload(g, s)) return rc;
    HIPCHK(hipMemcpyAsync(kb.lqq, lqq, sizeof(lqq), hipMemcpyHostToDevice, s));
    const FixedDesign fd = kb.design(g);
    return run_recovering(c, [&](bool redo, std::vector<int32_t>& seqs) -> int {
      for (int64_t gi = 0; gi < n_h2; ++gi) {
        Carve cvp = cv;
        rq.mode = redo ? ChunkMode::NoChain : ChunkMode::Full;
        rq.d_h2 = lb.h2 + gi * B;
        rq.d_fit = lb.fits + gi * B;
        ChunkRes res;
        if (int rc = run_chunk(c, rq, cvp, res)) return rc;
        seqs.push_back(res.chain_seq);
        if (redo) continue;
        HIPCHK(launch_fixed_subst(res.cl, fd, kb.plan, kb.S, s));
        HIPCHK(launch_fixed_gls(res.cl, fd, kb.S, kb.b + gi * B * nt * Cw, nullptr, kb.keep, s));
        HIPCHK(launch_loglik_fixed(res.cl, kb.keep.ks, kb.lqq, kcols, lb.ll + gi * B * nt, lb.s2 + gi * B * nt, s));
      }
      const auto out = [&](double* host, size_t hpitch, const double* dev, size_t drow) {   // n_h2 rows to the host
        return hipMemcpy2DAsync(host, hpitch, dev, drow, drow, (size_t)n_h2, hipMemcpyDeviceToHost, s);
      };
      HIPCHK(out(fitness + b0, pitch, lb.fits, row));
      if (redo) return 0;
      HIPCHK(out(loglik + b0 * nt, pitch * nt, lb.ll, rowt));
      HIPCHK(out(sigma2_g + b0 * nt, pitch * nt, lb.s2, rowt));
      HIPCHK(out(bout + b0 * nt * Cw, pitch * nt * Cw, kb.b, rowt * Cw));
      return 0;
    });
  });
}

struct ReliabFixedBufs {   // tblup_reliability_group_batch, the models of more than COVAR_W columns
  ReliabBufs r;
  FixedKeepBufs k;
  double* qa;                       // ReliabCovBufs'
  int32_t* ga;                      // the listed animals' level codes [n_rel]
  double *pev, *fc;                 // pev_total [B][n_rel] and fixed_cov [B][n_cov + L][n_cov + L] where wanted
  double* qV;                       // tblup_fit_group_batch's second pass (FixedBufs'), where wanted
  int32_t* gV;
  double *z2, *fit0, *ebv2;
  static ReliabFixedBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t n_rel, int64_t n_cov,
                               int64_t L, int64_t Cw, bool model, bool full, bool pev, bool fc) {
    const EvalDims& d = hb.d;
    const size_t Bt = (size_t)B * d.nt, Co = (size_t)(n_cov + L);
    ReliabFixedBufs b{ReliabBufs::carve(cv, hb, B, sum_k, n_rel, model), FixedKeepBufs::carve(cv, hb, B, L, Cw, 1)};
    b.qa = cv.take<double>((size_t)2 * n_rel * COVAR_W);
    b.ga = cv.take<int32_t>((size_t)n_rel);
    b.pev = pev ? cv.take<double>((size_t)B * n_rel) : nullptr;
    b.fc = fc ? cv.take<double>((size_t)B * Co * Co) : nullptr;
    if (full) {
      b.qV = cv.take<double>((size_t)2 * COVAR_W * d.nV);
      b.gV = cv.take<int32_t>((size_t)d.nV);
      b.z2 = cv.take<double>(Bt * hb.sd.ns);
      b.fit0 = cv.take<double>((size_t)B);
      b.ebv2 = cv.take<double>(Bt * d.nV);
    }
    return b;
  }
};

// The models of more than COVAR_W fixed columns of a tblup_reliability_group_batch call, as a batch of their own:
// tblup_reliability_cov_batch's chunk with k_fixed_subst and k_fixed_gls (keep mode) in place of k_covar, k_reliab's
// FIX instances and k_fixed_cov behind them, and fit_fixed_wide's second pass when the model or its fitness is wanted
// (full).  a32 / animals: the list; rel / pev [batch][n_pred], fc [batch][(n_cov + L)^2] (pev, fc: null when not
// wanted); bout [batch][nt][Cw] and intercept / center / effects: fit_fixed_wide's, with model.
int reliab_fixed_wide(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group, int64_t L,
                      int64_t Cw, const std::vector<int32_t>& a32, const int64_t* animals, const int64_t* idx,
                      const int64_t* offsets, int64_t batch, double h2, int branch, bool full, double* fitness,
                      double* rel, double* pev, double* fc, double* bout, double* intercept, double* center,
                      double* effects) {
  const bool model = intercept != nullptr;
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  if (!hb.sp) return 0;
  fitness = hb.fitness_or_own(fitness);
  const EvalDims& d = hb.d;
  const int nt = d.nt;
  const int64_t n_pred = (int64_t)a32.size(), Co = n_cov + L;
  const GroupDesign g = gather_group(hb, cov, n_cov, group, L, Cw);
  // f~_a of the listed animals: the covariates as tblup_reliability_cov_batch lays them out, the level codes
  std::vector<double> h_qa((size_t)2 * n_pred * COVAR_W, 0.0);
  std::vector<int32_t> h_ga((size_t)n_pred);
  for (int64_t v = 0; v < n_pred; ++v) {
    for (int64_t j = 0; j < n_cov; ++j) {
      const double q = cov[animals[v] * n_cov + j];
      h_qa[v * COVAR_W + j] = q;
      h_qa[(n_pred + v) * COVAR_W + j] = q - g.cp.m[j];
    }
    h_ga[v] = (int32_t)group[animals[v]];
  }
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) {
    return ReliabFixedBufs::carve(cv, hb, B, sk, n_pred, n_cov, L, Cw, model, full, pev != nullptr, fc != nullptr);
  };
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ReliabFixedBufs rb = carve(cv, B, ck.sum_k);
    const FixedKeepBufs& kb = rb.k;
    if (int rc = ws_check(c, cv)) return rc;
    if (n_pred > 0) {
      HIPCHK(hipMemcpyAsync(rb.r.an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(rb.qa, h_qa.data(), h_qa.size() * 8, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(rb.ga, h_ga.data(), h_ga.size() * 4, hipMemcpyHostToDevice, s));
    }
    if (int rc = kb.upload(g, s)) return rc;
    FixedDesign fd = kb.design(g);
    if (full) {
      HIPCHK(hipMemcpyAsync(rb.qV, g.cp.qV.data(), g.cp.qV.size() * 8, hipMemcpyHostToDevice, s));
      if (!g.gV.empty()) HIPCHK(hipMemcpyAsync(rb.gV, g.gV.data(), g.gV.size() * 4, hipMemcpyHostToDevice, s));
      fd.qV = rb.qV;
      fd.gV = rb.gV;
    }
    const auto after = [&](const CholLaunch& cl) -> int {
      HIPCHK(launch_fixed_subst(cl, fd, kb.plan, kb.S, s));
      HIPCHK(launch_fixed_gls(cl, fd, kb.S, kb.b, rb.z2, kb.keep, s));
      const ReliabFixed rf{kb.S, kb.keep.cf, kb.keep.ks, rb.qa, rb.ga, fd, rb.pev};
      HIPCHK(launch_reliab_fixed(cl, (const int8_t*)c->geno_sm.p, (const int32_t*)c->colsum_all.p, rb.r.an, n_pred,
                                 rb.r.plan, rb.r.vscr, rf, rb.r.rel, s));
      if (n_pred > 0) {
        HIPCHK(hipMemcpyAsync(rel + b0 * n_pred, rb.r.rel, (size_t)B * n_pred * 8, hipMemcpyDeviceToHost, s));
        if (pev) HIPCHK(hipMemcpyAsync(pev + b0 * n_pred, rb.pev, (size_t)B * n_pred * 8, hipMemcpyDeviceToHost, s));
      }
      if (fc) {
        HIPCHK(launch_fixed_cov(cl, fd, kb.keep.cf, kb.keep.ks, rb.fc, s));
        HIPCHK(hipMemcpyAsync(fc + b0 * Co * Co, rb.fc, (size_t)B * Co * Co * 8, hipMemcpyDeviceToHost, s));
      }
      return 0;
    };
    if (!full) return factor_pass(hb, ck, cv, rq, fitness, nullptr, after);
    // fit_fixed_wide's chunk: the pipeline with the one-workgroup solve, then the second pass on z*
    double* d_fit = rq.d_fit;
    Carve cvp = cv;
    rq.mode = ChunkMode::NoChain;
    rq.d_fit = rb.fit0;
    ChunkRes res;
    if (int rc = run_chunk(c, rq, cvp, res)) return rc;
    if (int rc = after(res.cl)) return rc;
    CholLaunch cl2 = res.cl;
    cl2.z = rb.z2;
    HIPCHK(launch_solve(cl2, nullptr, rb.fit0, rb.ebv2, s));
    HIPCHK(launch_fixed_fitness(cl2, fd, rb.ebv2, kb.b, d_fit, s));
    if (model) {
      if (int rc = rb.r.m.enqueue(hb, ck, cl2, center, effects)) return rc;
      HIPCHK(hipMemcpyAsync(bout + b0 * nt * Cw, kb.b, (size_t)B * nt * Cw * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(fitness + b0, d_fit, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
    return 0;
  });
  if (rc || !model) return rc;
  // fit_fixed_wide's post-pass
  fill_intercepts(hb, intercept);
  const double nan = std::nan("");
  for (int64_t b = 0; b < batch; ++b) {
    const bool gblup = branch_of(c, offsets[b + 1] - offsets[b], branch) == 1;
    bool dead = fixed_cols(gblup, (int)n_cov, (int)L) == 0 && std::isnan(fitness[b]);
    for (int64_t i = 0; i < nt * Cw; ++i) dead = dead || std::isnan(bout[b * nt * Cw + i]);
    if (!dead) continue;
    for (int t = 0; t < nt; ++t) intercept[b * nt + t] = nan;
    for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i) center[i] = nan;
  }
  return 0;
}

struct PredictBufs {   // tblup_predict_batch: no pipeline, these are the chunk
  int32_t* an;                      // the animal list [n_pred]
  int64_t *idx, *off;               // the models' index lists and offsets
  double *icpt, *cen, *eff, *ebv;   // intercepts [B][nt], centres [sum_k], effects [nt][sum_k]; EBVs [B][nt][n_pred]
  static PredictBufs carve(Carve& cv, int64_t B, int64_t sum_k, int64_t n_pred, int nt) {
    const size_t sk = (size_t)sum_k, Bt = (size_t)B * nt;
    return {cv.take<int32_t>((size_t)n_pred), cv.take<int64_t>(sk), cv.take<int64_t>((size_t)B + 1),
            cv.take<double>(Bt), cv.take<double>(sk), cv.take<double>(nt * sk), cv.take<double>(Bt * n_pred)};
  }
};

}  // namespace

extern "C" {

int tblup_fit_batch(tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                    int branch, double* fitness, double* intercept, double* center, double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (batch > 0 && (!intercept || !center || !effects)) return fail(TBLUP_ERR_ARG, "null intercept/center/effects");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  if (!hb.sp) return 0;
  fitness = hb.fitness_or_own(fitness);
  const auto carve = [&](Carve& cv, int64_t, int64_t sum_k) { return ModelBufs::carve(cv, hb, sum_k); };
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const ModelBufs mb = carve(cv, ck.B, ck.sum_k);
    return factor_pass(hb, ck, cv, rq, fitness, nullptr,
                       [&](const CholLaunch& cl) { return mb.enqueue(hb, ck, cl, center, effects); });
  });
  if (!rc) fill_intercepts(hb, intercept);
  return rc;
}

int tblup_reliability_batch(tblup_ctx* c, int split_id, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                            const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                            double* intercept, double* center, double* effects, double* reliability) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  const bool model = intercept || center || effects;
  if (model && !(intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "intercept/center/effects are given together or not at all");
  if (n_pred > 0 && !animals) return fail(TBLUP_ERR_ARG, "null animals");
  std::vector<int32_t> a32((size_t)n_pred);
  for (int64_t i = 0; i < n_pred; ++i) {
    if (animals[i] < 0 || animals[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    a32[i] = (int32_t)animals[i];
  }
  if (batch == 0 || n_pred == 0) return 0;
  if (!reliability) return fail(TBLUP_ERR_ARG, "null reliability");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) { return ReliabBufs::carve(cv, hb, B, sk, n_pred, model); };
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const ReliabBufs rb = carve(cv, ck.B, ck.sum_k);
    HIPCHK(hipMemcpyAsync(rb.an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      if (model)
        if (int rc = rb.m.enqueue(hb, ck, cl, center, effects)) return rc;
      HIPCHK(launch_reliab(cl, (const int8_t*)c->geno_sm.p, (const int32_t*)c->colsum_all.p, rb.an, n_pred, rb.plan,
                           rb.vscr, nullptr, rb.rel, s));
      HIPCHK(hipMemcpyAsync(reliability + ck.b0 * n_pred, rb.rel, (size_t)ck.B * n_pred * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
  if (!rc && model) fill_intercepts(hb, intercept);
  return rc;
}

int tblup_loo_batch(tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                    int branch, double* fitness, double* loo_pred, double* leverage, double* press,
                    double* eval_fitness) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (batch > 0 && !loo_pred) return fail(TBLUP_ERR_ARG, "null loo_pred");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, fitness != nullptr)) return rc;
  if (!hb.sp) return 0;
  const EvalDims& d = hb.d;
  const int nt = d.nt;
  const int64_t nT = d.nT;
  std::vector<int32_t> t32((size_t)nT);
  for (int64_t i = 0; i < nT; ++i) t32[i] = (int32_t)hb.sp->train[i];
  std::vector<double> rfit((size_t)batch * nt), own_press(press ? 0 : (size_t)batch * nt);
  if (!press) press = own_press.data();
  eval_fitness = hb.fitness_or_own(eval_fitness);
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return LooBufs::carve(cv, hb, B); };
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const LooBufs lb = carve(cv, B, ck.sum_k);
    HIPCHK(hipMemcpyAsync(lb.tr, t32.data(), (size_t)nT * 4, hipMemcpyHostToDevice, s));
    return factor_pass(hb, ck, cv, rq, eval_fitness, nullptr, [&](const CholLaunch& cl) -> int {
      // neither solve path keeps the solution: k_effects' back substitution does, with nothing else asked of it
      HIPCHK(launch_effects(cl, (const int32_t*)c->colsum_all.p, nullptr, nullptr, 0, s, lb.alpha));
      HIPCHK(launch_loo(cl, (const int8_t*)c->geno_sm.p, lb.tr, lb.alpha, lb.plan, lb.vscr, lb.pred, lb.lev, s));
      HIPCHK(launch_loo_fitness(cl, lb.pred, lb.rfit, lb.press, s));
      HIPCHK(hipMemcpyAsync(loo_pred + b0 * nt * nT, lb.pred, (size_t)B * nt * nT * 8, hipMemcpyDeviceToHost, s));
      if (leverage) HIPCHK(hipMemcpyAsync(leverage + b0 * nT, lb.lev, (size_t)B * nT * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(rfit.data() + b0 * nt, lb.rfit, (size_t)B * nt * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(press + b0 * nt, lb.press, (size_t)B * nt * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
  if (rc) return rc;
  // the evaluation's convention: the mean of the traits' |r|, added in trait order
  for (int64_t b = 0; b < batch; ++b) {
    double fsum = 0.0;
    for (int t = 0; t < nt; ++t) fsum += rfit[b * nt + t];
    fitness[b] = nt == 1 ? fsum : fsum / (double)nt;
  }
  return 0;
}

int tblup_reliability_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* animals,
                                int64_t n_pred, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                                int branch, double* fitness, double* cov_effects, double* cov_center,
                                double* intercept, double* center, double* effects, double* reliability,
                                double* pev_total, double* cov_cov) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  const bool model = cov_effects || cov_center || intercept || center || effects;
  if (model && !(cov_effects && cov_center && intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "cov_effects/cov_center/intercept/center/effects are given together or not at all");
  if (n_pred > 0 && !animals) return fail(TBLUP_ERR_ARG, "null animals");
  std::vector<int32_t> a32((size_t)n_pred);
  for (int64_t i = 0; i < n_pred; ++i) {
    if (animals[i] < 0 || animals[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    a32[i] = (int32_t)animals[i];
  }
  // the second solve (the model of the adjusted phenotype and its fitness) runs only for a caller who wants it
  const bool full = model || fitness;
  if (batch == 0 || (n_pred == 0 && !full && !cov_cov)) return 0;
  if (n_pred > 0 && !reliability) return fail(TBLUP_ERR_ARG, "null reliability");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const EvalDims& d = hb.d;
  const int nt = d.nt, nc = (int)n_cov;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, full);
  // q~_a of the listed animals: plane 0 as given, plane 1 centred by the train means, zero past n_cov
  std::vector<double> h_qa((size_t)2 * n_pred * COVAR_W, 0.0);
  for (int64_t v = 0; v < n_pred; ++v)
    for (int64_t j = 0; j < n_cov; ++j) {
      const double q = cov[animals[v] * n_cov + j];
      h_qa[v * COVAR_W + j] = q;
      h_qa[(n_pred + v) * COVAR_W + j] = q - cp.m[j];
    }
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) {
    return ReliabCovBufs::carve(cv, hb, B, sk, n_pred, n_cov, model, full, pev_total != nullptr, cov_cov != nullptr);
  };
  // per chunk, behind the pipeline: k_covar keeps the model's GLS step, k_reliab's covariate-adjusted launches
  // and k_cov_cov read it; a caller who wants the model or its fitness gets tblup_fit_cov_batch's own second
  // pass (the one-workgroup solve on z*, k_cov_fitness, k_effects) behind them
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ReliabCovBufs rb = carve(cv, B, ck.sum_k);
    const CovKeepBufs& kb = rb.k;
    if (int rc = ws_check(c, cv)) return rc;
    if (n_pred > 0) {
      HIPCHK(hipMemcpyAsync(rb.r.an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(rb.qa, h_qa.data(), h_qa.size() * 8, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(kb.qT, cp.qT.data(), cp.qT.size() * 8, hipMemcpyHostToDevice, s));
    if (full) HIPCHK(hipMemcpyAsync(rb.qV, cp.qV.data(), cp.qV.size() * 8, hipMemcpyHostToDevice, s));
    const auto after = [&](const CholLaunch& cl) -> int {
      HIPCHK(launch_covar(cl, kb.qT, nc, kb.plan, kb.vscr(), kb.b, rb.z2, kb.keep, s));
      const ReliabCov rcv{kb.keep.sq, kb.keep.cf, kb.keep.ks, rb.qa, nc, rb.pev};
      HIPCHK(launch_reliab(cl, (const int8_t*)c->geno_sm.p, (const int32_t*)c->colsum_all.p, rb.r.an, n_pred,
                           rb.r.plan, rb.r.vscr, &rcv, rb.r.rel, s));
      if (n_pred > 0) {
        HIPCHK(hipMemcpyAsync(reliability + b0 * n_pred, rb.r.rel, (size_t)B * n_pred * 8, hipMemcpyDeviceToHost, s));
        if (pev_total)
          HIPCHK(hipMemcpyAsync(pev_total + b0 * n_pred, rb.pev, (size_t)B * n_pred * 8, hipMemcpyDeviceToHost, s));
      }
      if (cov_cov) {
        HIPCHK(launch_cov_cov(kb.keep.cf, kb.keep.ks, B, nc, rb.cc, s));
        HIPCHK(hipMemcpyAsync(cov_cov + b0 * nc * nc, rb.cc, (size_t)B * nc * nc * 8, hipMemcpyDeviceToHost, s));
      }
      return 0;
    };
    if (!full) return factor_pass(hb, ck, cv, rq, fitness, nullptr, after);
    // tblup_fit_cov_batch's chunk: the pipeline with the one-workgroup solve, then the second pass on z*
    double* d_fit = rq.d_fit;
    Carve cvp = cv;
    rq.mode = ChunkMode::NoChain;
    rq.d_fit = rb.fit0;
    ChunkRes res;
    if (int rc = run_chunk(c, rq, cvp, res)) return rc;
    if (int rc = after(res.cl)) return rc;
    CholLaunch cl2 = res.cl;
    cl2.z = rb.z2;
    HIPCHK(launch_solve(cl2, nullptr, rb.fit0, rb.ebv2, s));
    HIPCHK(launch_cov_fitness(cl2, rb.ebv2, rb.qV, kb.b, nc, d_fit, s));
    if (model) {
      if (int rc = rb.r.m.enqueue(hb, ck, cl2, center, effects)) return rc;
      HIPCHK(hipMemcpyAsync(cov_effects + b0 * nt * nc, kb.b, (size_t)B * nt * nc * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(fitness + b0, d_fit, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
    return 0;
  });
  if (rc || !model) return rc;
  // tblup_fit_cov_batch's post-pass: intercepts, cov_center, and NaN throughout for a model whose covariate
  // effects are NaN
  fill_intercepts(hb, intercept);
  const double nan = std::nan("");
  for (int64_t b = 0; b < batch; ++b) {
    const int mode = branch_of(c, offsets[b + 1] - offsets[b], branch);
    bool dead = false;
    for (int64_t i = 0; i < nt * n_cov; ++i) dead = dead || std::isnan(cov_effects[b * nt * n_cov + i]);
    for (int64_t j = 0; j < n_cov; ++j) cov_center[b * n_cov + j] = dead ? nan : (mode == 2 ? cp.m[j] : 0.0);
    if (dead) {
      for (int t = 0; t < nt; ++t) intercept[b * nt + t] = nan;
      for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i) center[i] = nan;
    }
  }
  return 0;
}

int tblup_snp_score_batch(tblup_ctx* c, int split_id, const int64_t* snps, int64_t n_cand, const int64_t* idx,
                          const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness, double* score,
                          double* info, double* q) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (batch < 0 || n_cand < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_cand");
  if (n_cand > 0 && !snps) return fail(TBLUP_ERR_ARG, "null snps");
  if (int rc = check_indices(c, snps, n_cand)) return rc;
  if (batch == 0 || n_cand == 0) return 0;
  // lambda = 0 makes the snp branch's V singular: (0, 1), as tblup_loglik_batch
  if (!(h2 > 0.0) || !(h2 < 1.0)) return fail(TBLUP_ERR_ARG, "h2 must be in (0, 1)");
  if (!score || !info) return fail(TBLUP_ERR_ARG, "null score/info");
  std::vector<int32_t> s32((size_t)n_cand);
  for (int64_t i = 0; i < n_cand; ++i) s32[i] = (int32_t)snp_col(snps[i], c->P);
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const int nt = hb.d.nt;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return ScoreBufs::carve(cv, hb, B, n_cand); };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ScoreBufs sb = carve(cv, B, ck.sum_k);
    HIPCHK(hipMemcpyAsync(sb.cand, s32.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      HIPCHK(launch_snpscore(cl, (const int32_t*)c->colsum_all.p, sb.cand, n_cand, sb.plan, sb.vscr, nullptr, sb.sco,
                             sb.inf, sb.q, s));
      HIPCHK(hipMemcpyAsync(score + b0 * nt * n_cand, sb.sco, (size_t)B * nt * n_cand * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(info + b0 * n_cand, sb.inf, (size_t)B * n_cand * 8, hipMemcpyDeviceToHost, s));
      if (q) HIPCHK(hipMemcpyAsync(q + b0 * nt, sb.q, (size_t)B * nt * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
}

int tblup_loglik_batch(tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch,
                       const double* h2, int64_t n_h2, int branch, double* fitness, double* loglik,
                       double* sigma2_g) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (batch < 0 || n_h2 < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_h2");
  if (batch == 0 || n_h2 == 0) return 0;
  if (!h2 || !loglik) return fail(TBLUP_ERR_ARG, "null h2/loglik");
  // lambda = 0 makes the snp branch's V singular: (0, 1) here, not tblup_eval_batch's (0, 1]
  for (int64_t i = 0; i < n_h2 * batch; ++i)
    if (!(h2[i] > 0.0) || !(h2[i] < 1.0)) return fail(TBLUP_ERR_ARG, "every h2 must be in (0, 1)");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2[0], branch, true)) return rc;
  const int nt = hb.d.nt;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return LogLikBufs::carve(cv, hb, B, n_h2); };
  // per chunk: its h2 columns up front, the n_h2 passes back to back (each the pipeline at its row of
  // per-system h2, then k_loglik on the factor it leaves, without waiting for the solve), the results of
  // every pass copied out behind the last
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const size_t row = (size_t)B * 8, rowt = row * nt, pitch = (size_t)batch * 8;
    const LogLikBufs lb = carve(cv, B, ck.sum_k);
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpy2DAsync(lb.h2, row, h2 + b0, pitch, row, (size_t)n_h2, hipMemcpyHostToDevice, s));
    return run_recovering(c, [&](bool redo, std::vector<int32_t>& seqs) -> int {
      // redo: a chained solve of some pass gave up a wait -- the factors of all but the last pass are
      // gone, so every pass runs again whole with the one-workgroup k_solve (the same bits), for the
      // fitnesses only
      for (int64_t g = 0; g < n_h2; ++g) {
        Carve cvp = cv;
        rq.mode = redo ? ChunkMode::NoChain : ChunkMode::Full;
        rq.d_h2 = lb.h2 + g * B;
        rq.d_fit = lb.fits + g * B;
        ChunkRes res;
        if (int rc = run_chunk(c, rq, cvp, res)) return rc;
        seqs.push_back(res.chain_seq);
        if (!redo) HIPCHK(launch_loglik(res.cl, nullptr, nullptr, 0, lb.ll + g * B * nt, lb.s2 + g * B * nt, s));
      }
      const auto out = [&](double* host, size_t hpitch, const double* dev, size_t drow) {   // n_h2 rows to the host
        return hipMemcpy2DAsync(host, hpitch, dev, drow, drow, (size_t)n_h2, hipMemcpyDeviceToHost, s);
      };
      if (fitness) HIPCHK(out(fitness + b0, pitch, lb.fits, row));
      if (redo) return 0;
      HIPCHK(out(loglik + b0 * nt, pitch * nt, lb.ll, rowt));
      if (sigma2_g) HIPCHK(out(sigma2_g + b0 * nt, pitch * nt, lb.s2, rowt));
      return 0;
    });
  });
}

int tblup_fit_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness, double* ebv,
                        double* cov_effects, double* cov_center, double* intercept, double* center, double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  const bool model = intercept || center || effects;
  if (model && !(intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "intercept/center/effects are given together or not at all");
  if (batch > 0 && (!cov_effects || !cov_center)) return fail(TBLUP_ERR_ARG, "null cov_effects/cov_center");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  if (!hb.sp) return 0;
  fitness = hb.fitness_or_own(fitness);
  const EvalDims& d = hb.d;
  const int nt = d.nt, nc = (int)n_cov;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, true);
  const std::vector<double>&cov_m = cp.m, &h_qT = cp.qT, &h_qV = cp.qV;
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) { return CovBufs::carve(cv, hb, B, sk, n_cov, model); };
  // per chunk: the pipeline with the one-workgroup solve (nothing to recover; its EBVs are not wanted),
  // k_covar on the factor and z it leaves, then the solve, the fitness and the effects of the adjusted
  // phenotype from the corrected z in a buffer of its own
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const CovBufs cb = carve(cv, B, ck.sum_k);
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpyAsync(cb.qT, h_qT.data(), h_qT.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(cb.qV, h_qV.data(), h_qV.size() * 8, hipMemcpyHostToDevice, s));
    double* d_fit = rq.d_fit;
    Carve cvp = cv;
    rq.mode = ChunkMode::NoChain;
    rq.d_fit = cb.fit0;
    ChunkRes res;
    if (int rc = run_chunk(c, rq, cvp, res)) return rc;
    HIPCHK(launch_covar(res.cl, cb.qT, nc, cb.plan, cb.vscr, cb.b, cb.z2, CovKeep{}, s));
    CholLaunch cl2 = res.cl;
    cl2.z = cb.z2;
    HIPCHK(launch_solve(cl2, nullptr, cb.fit0, cb.ebv2, s));
    HIPCHK(launch_cov_fitness(cl2, cb.ebv2, cb.qV, cb.b, nc, d_fit, s));
    if (model)
      if (int rc = cb.m.enqueue(hb, ck, cl2, center, effects)) return rc;
    HIPCHK(hipMemcpyAsync(cov_effects + b0 * nt * nc, cb.b, (size_t)B * nt * nc * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(fitness + b0, d_fit, (size_t)B * 8, hipMemcpyDeviceToHost, s));
    if (ebv) HIPCHK(hipMemcpyAsync(ebv + b0 * nt * d.nV, cb.ebv2, (size_t)B * nt * d.nV * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
    return 0;
  });
  if (rc) return rc;
  if (model) fill_intercepts(hb, intercept);
  // cov_center: the train rows' column means under snp, 0 under gblup; a model whose covariate effects are
  // NaN (d = 0, collinear covariates) is NaN in every output
  const double nan = std::nan("");
  for (int64_t b = 0; b < batch; ++b) {
    const int mode = branch_of(c, offsets[b + 1] - offsets[b], branch);
    bool dead = false;
    for (int64_t i = 0; i < nt * n_cov; ++i) dead = dead || std::isnan(cov_effects[b * nt * n_cov + i]);
    for (int64_t j = 0; j < n_cov; ++j) cov_center[b * n_cov + j] = dead ? nan : (mode == 2 ? cov_m[j] : 0.0);
    if (dead && model) {
      for (int t = 0; t < nt; ++t) intercept[b * nt + t] = nan;
      for (int64_t i = offsets[b]; i < offsets[b + 1]; ++i) center[i] = nan;
    }
  }
  return 0;
}

int tblup_fit_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                          int64_t n_levels, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                          int branch, double* fitness, double* ebv, double* cov_effects, double* cov_center,
                          double* group_effects, double* group_center, double* intercept, double* center,
                          double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  const bool model = intercept || center || effects;
  if (model && !(intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "intercept/center/effects are given together or not at all");
  if (batch > 0 && (!group_effects || !group_center)) return fail(TBLUP_ERR_ARG, "null group_effects/group_center");
  if (batch > 0 && n_cov > 0 && (!cov_effects || !cov_center))
    return fail(TBLUP_ERR_ARG, "null cov_effects/cov_center");
  const int64_t L = n_levels, nc = n_cov;
  GroupSplit gs;
  {
    HostBatch hb;
    if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
    if (!hb.sp) return 0;
    if (int rc = check_group_split(hb, cov, nc, group, L, gs)) return rc;
  }
  const std::vector<long double>& share = gs.share;
  const std::vector<double>& cov_m = gs.cov_m;
  const int64_t nV = gs.nV;
  const int nt = gs.nt;
  // Routes 0 / 1 through tblup_fit_cov_batch on the expanded design (the same bits as that entry gives); 2 through
  // k_fixed.
  GroupRoutes gr;
  if (int rc = route_group(c, offsets, batch, branch, nc, L, gr)) return rc;
  const int64_t(&cols)[2] = gr.cols;
  const int64_t total = offsets[batch];
  const double nan = std::nan("");
  for (int route = 0; route < 3; ++route) {
    const std::vector<int64_t>& mb = gr.of[route];
    const int64_t Bs = (int64_t)mb.size();
    if (!Bs) continue;
    const SubBatch sub = sub_batch(idx, offsets, mb);
    const std::vector<int64_t>&so = sub.so, &si = sub.si;
    const int64_t st = so[Bs];
    const int64_t Cw = gr.width(route);
    std::vector<double> fit((size_t)Bs), ev(ebv ? (size_t)Bs * nt * nV : 0), bo((size_t)Bs * nt * Cw);
    std::vector<double> icpt(model ? (size_t)Bs * nt : 0), cen(model ? (size_t)st : 0), eff(model ? (size_t)nt * st : 0);
    double* evp = ebv ? ev.data() : nullptr;
    double *ip = model ? icpt.data() : nullptr, *cp = model ? cen.data() : nullptr, *ep = model ? eff.data() : nullptr;
    int rc;
    if (route == 2) {
      rc = fit_fixed_wide(c, split_id, cov, nc, group, L, Cw, si.data(), so.data(), Bs, h2, branch, fit.data(), evp,
                          bo.data(), ip, cp, ep);
    } else {
      const std::vector<double> x = expand_design(c, cov, nc, group, Cw, route);
      std::vector<double> xc((size_t)Bs * Cw);   // that entry's centres (cov_m, share)
      rc = tblup_fit_cov_batch(c, split_id, x.data(), Cw, si.data(), so.data(), Bs, h2, branch, fit.data(), evp,
                               bo.data(), xc.data(), ip, cp, ep);
    }
    if (rc) return rc;
    for (int64_t i = 0; i < Bs; ++i) {
      const int64_t b = mb[i];
      const int br = branch_of(c, offsets[b + 1] - offsets[b], branch) == 1 ? 0 : 1;
      const int64_t k = offsets[b + 1] - offsets[b];
      bool dead = cols[br] == 0 && std::isnan(fit[i]);
      for (int64_t e = 0; e < nt * Cw; ++e) dead = dead || std::isnan(bo[i * nt * Cw + e]);
      if (fitness) fitness[b] = fit[i];
      if (ebv) std::copy(evp + i * nt * nV, evp + (i + 1) * nt * nV, ebv + b * nt * nV);
      for (int64_t j = 0; j < nc; ++j)
        cov_center[b * nc + j] = dead ? nan : (br == 1 ? cov_m[j] : 0.0);
      for (int64_t l = 0; l < L; ++l) group_center[b * L + l] = dead ? nan : (br == 1 ? (double)share[l] : 0.0);
      put_effects(bo.data() + i * nt * Cw, nt, Cw, nc, L, br, dead, nc ? cov_effects + b * nt * nc : nullptr,
                  group_effects + b * nt * L);
      for (int t = 0; t < nt; ++t) {
        if (model) {
          intercept[b * nt + t] = ip[i * nt + t];
          std::copy(ep + t * st + so[i], ep + t * st + so[i] + k, effects + t * total + offsets[b]);
        }
      }
      if (model) std::copy(cp + so[i], cp + so[i] + k, center + offsets[b]);
    }
  }
  return 0;
}

int tblup_snp_score_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* snps,
                              int64_t n_cand, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                              int branch, double* fitness, double* score, double* info, double* q,
                              double* cov_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (batch < 0 || n_cand < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_cand");
  if (n_cand > 0 && !snps) return fail(TBLUP_ERR_ARG, "null snps");
  if (int rc = check_indices(c, snps, n_cand)) return rc;
  if (batch == 0 || n_cand == 0) return 0;
  if (!(h2 > 0.0) || !(h2 < 1.0)) return fail(TBLUP_ERR_ARG, "h2 must be in (0, 1)");
  if (!score || !info) return fail(TBLUP_ERR_ARG, "null score/info");
  std::vector<int32_t> s32((size_t)n_cand);
  for (int64_t i = 0; i < n_cand; ++i) s32[i] = (int32_t)snp_col(snps[i], c->P);
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const int nt = hb.d.nt, nc = (int)n_cov;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, false);
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return ScoreCovBufs::carve(cv, hb, B, n_cand, n_cov); };
  // per chunk, behind the pipeline: k_covar keeps the model's GLS step, k_snpscore's launches read it
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ScoreCovBufs sb = carve(cv, B, ck.sum_k);
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpyAsync(sb.s.cand, s32.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sb.k.qT, cp.qT.data(), cp.qT.size() * 8, hipMemcpyHostToDevice, s));
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      HIPCHK(launch_covar(cl, sb.k.qT, nc, sb.k.plan, sb.k.vscr(), sb.k.b, nullptr, sb.k.keep, s));
      const ScoreCov sc{sb.k.keep.sq, sb.k.keep.cf, sb.k.keep.ch, sb.k.keep.ks, sb.k.qT, nc};
      HIPCHK(launch_snpscore(cl, (const int32_t*)c->colsum_all.p, sb.s.cand, n_cand, sb.s.plan, sb.s.vscr, &sc,
                             sb.s.sco, sb.s.inf, sb.s.q, s));
      HIPCHK(hipMemcpyAsync(score + b0 * nt * n_cand, sb.s.sco, (size_t)B * nt * n_cand * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(info + b0 * n_cand, sb.s.inf, (size_t)B * n_cand * 8, hipMemcpyDeviceToHost, s));
      if (q) HIPCHK(hipMemcpyAsync(q + b0 * nt, sb.s.q, (size_t)B * nt * 8, hipMemcpyDeviceToHost, s));
      if (cov_effects)
        HIPCHK(hipMemcpyAsync(cov_effects + b0 * nt * nc, sb.k.b, (size_t)B * nt * nc * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
}

int tblup_loglik_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                           const int64_t* offsets, int64_t batch, const double* h2, int64_t n_h2, int branch,
                           double* fitness, double* loglik, double* sigma2_g, double* cov_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (batch < 0 || n_h2 < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_h2");
  if (batch == 0 || n_h2 == 0) return 0;
  if (!h2 || !loglik) return fail(TBLUP_ERR_ARG, "null h2/loglik");
  for (int64_t i = 0; i < n_h2 * batch; ++i)
    if (!(h2[i] > 0.0) || !(h2[i] < 1.0)) return fail(TBLUP_ERR_ARG, "every h2 must be in (0, 1)");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2[0], branch, true)) return rc;
  const int nt = hb.d.nt, nc = (int)n_cov;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, false);
  // log|Q~_T^T Q~_T| does not depend on h2: once per call, one value per plane
  const double lqq[2] = {log_det_qq(cp.qT.data(), hb.d.nT, hb.d.nTp, n_cov),
                         log_det_qq(cp.qT.data() + (size_t)COVAR_W * hb.d.nTp, hb.d.nT, hb.d.nTp, n_cov)};
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return LogLikCovBufs::carve(cv, hb, B, n_h2, n_cov); };
  // tblup_loglik_batch's passes, each with k_covar (keep mode, no z*) between the pipeline and k_loglik
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const size_t row = (size_t)B * 8, rowt = row * nt, pitch = (size_t)batch * 8;
    const LogLikCovBufs lc = carve(cv, B, ck.sum_k);
    const LogLikBufs& lb = lc.l;
    const CovKeepBufs& kb = lc.k;
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpy2DAsync(lb.h2, row, h2 + b0, pitch, row, (size_t)n_h2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(kb.qT, cp.qT.data(), cp.qT.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(kb.lqq, lqq, sizeof(lqq), hipMemcpyHostToDevice, s));
    return run_recovering(c, [&](bool redo, std::vector<int32_t>& seqs) -> int {
      for (int64_t g = 0; g < n_h2; ++g) {
        Carve cvp = cv;
        rq.mode = redo ? ChunkMode::NoChain : ChunkMode::Full;
        rq.d_h2 = lb.h2 + g * B;
        rq.d_fit = lb.fits + g * B;
        ChunkRes res;
        if (int rc = run_chunk(c, rq, cvp, res)) return rc;
        seqs.push_back(res.chain_seq);
        if (redo) continue;
        HIPCHK(launch_covar(res.cl, kb.qT, nc, kb.plan, kb.vscr(), kb.b + g * B * nt * nc, nullptr, kb.keep, s));
        HIPCHK(launch_loglik(res.cl, kb.keep.ks, kb.lqq, nc, lb.ll + g * B * nt, lb.s2 + g * B * nt, s));
      }
      const auto out = [&](double* host, size_t hpitch, const double* dev, size_t drow) {   // n_h2 rows to the host
        return hipMemcpy2DAsync(host, hpitch, dev, drow, drow, (size_t)n_h2, hipMemcpyDeviceToHost, s);
      };
      if (fitness) HIPCHK(out(fitness + b0, pitch, lb.fits, row));
      if (redo) return 0;
      HIPCHK(out(loglik + b0 * nt, pitch * nt, lb.ll, rowt));
      if (sigma2_g) HIPCHK(out(sigma2_g + b0 * nt, pitch * nt, lb.s2, rowt));
      if (cov_effects) HIPCHK(out(cov_effects + b0 * nt * nc, pitch * nt * nc, kb.b, rowt * nc));
      return 0;
    });
  });
}

int tblup_snp_score_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                                int64_t n_levels, const int64_t* snps, int64_t n_cand, const int64_t* idx,
                                const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                                double* score, double* info, double* q, double* cov_effects, double* group_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  if (batch < 0 || n_cand < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_cand");
  if (n_cand > 0 && !snps) return fail(TBLUP_ERR_ARG, "null snps");
  if (int rc = check_indices(c, snps, n_cand)) return rc;
  if (batch == 0 || n_cand == 0) return 0;
  if (!(h2 > 0.0) || !(h2 < 1.0)) return fail(TBLUP_ERR_ARG, "h2 must be in (0, 1)");
  if (!score || !info) return fail(TBLUP_ERR_ARG, "null score/info");
  const int64_t L = n_levels, nc = n_cov;
  GroupSplit gs;
  {
    HostBatch hb;
    if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
    if (int rc = check_group_split(hb, cov, nc, group, L, gs)) return rc;
  }
  const int nt = gs.nt;
  GroupRoutes gr;
  if (int rc = route_group(c, offsets, batch, branch, nc, L, gr)) return rc;
  std::vector<int32_t> s32((size_t)n_cand);
  for (int64_t i = 0; i < n_cand; ++i) s32[i] = (int32_t)snp_col(snps[i], c->P);
  for (int route = 0; route < 3; ++route) {
    const std::vector<int64_t>& mb = gr.of[route];
    const int64_t Bs = (int64_t)mb.size();
    if (!Bs) continue;
    const SubBatch sub = sub_batch(idx, offsets, mb);
    const int64_t Cw = gr.width(route);
    std::vector<double> fit((size_t)Bs), sco((size_t)Bs * nt * n_cand), inf((size_t)Bs * n_cand), qs((size_t)Bs * nt),
        bo((size_t)Bs * nt * Cw);
    int rc;
    if (route == 2) {
      rc = score_fixed_wide(c, split_id, cov, nc, group, L, Cw, s32, sub.si.data(), sub.so.data(), Bs, h2, branch,
                            fit.data(), sco.data(), inf.data(), qs.data(), bo.data());
    } else {
      const std::vector<double> x = expand_design(c, cov, nc, group, Cw, route);
      rc = tblup_snp_score_cov_batch(c, split_id, x.data(), Cw, snps, n_cand, sub.si.data(), sub.so.data(), Bs, h2,
                                     branch, fit.data(), sco.data(), inf.data(), qs.data(), bo.data());
    }
    if (rc) return rc;
    for (int64_t i = 0; i < Bs; ++i) {
      const int64_t b = mb[i];
      const int br = branch_of(c, offsets[b + 1] - offsets[b], branch) == 1 ? 0 : 1;
      bool dead = gr.cols[br] == 0 && std::isnan(fit[i]);
      for (int64_t e = 0; e < nt * Cw; ++e) dead = dead || std::isnan(bo[i * nt * Cw + e]);
      if (fitness) fitness[b] = fit[i];
      std::copy(sco.begin() + i * nt * n_cand, sco.begin() + (i + 1) * nt * n_cand, score + b * nt * n_cand);
      std::copy(inf.begin() + i * n_cand, inf.begin() + (i + 1) * n_cand, info + b * n_cand);
      if (q) std::copy(qs.begin() + i * nt, qs.begin() + (i + 1) * nt, q + b * nt);
      put_effects(bo.data() + i * nt * Cw, nt, Cw, nc, L, br, dead, cov_effects ? cov_effects + b * nt * nc : nullptr,
                  group_effects ? group_effects + b * nt * L : nullptr);
    }
  }
  return 0;
}

int tblup_loglik_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                             int64_t n_levels, const int64_t* idx, const int64_t* offsets, int64_t batch,
                             const double* h2, int64_t n_h2, int branch, double* fitness, double* loglik,
                             double* sigma2_g, double* cov_effects, double* group_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  if (batch < 0 || n_h2 < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_h2");
  if (batch == 0 || n_h2 == 0) return 0;
  if (!h2 || !loglik) return fail(TBLUP_ERR_ARG, "null h2/loglik");
  for (int64_t i = 0; i < n_h2 * batch; ++i)
    if (!(h2[i] > 0.0) || !(h2[i] < 1.0)) return fail(TBLUP_ERR_ARG, "every h2 must be in (0, 1)");
  const int64_t L = n_levels, nc = n_cov;
  GroupSplit gs;
  {
    HostBatch hb;
    if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2[0], branch, true)) return rc;
    if (int rc = check_group_split(hb, cov, nc, group, L, gs)) return rc;
  }
  const int nt = gs.nt;
  GroupRoutes gr;
  if (int rc = route_group(c, offsets, batch, branch, nc, L, gr)) return rc;
  for (int route = 0; route < 3; ++route) {
    const std::vector<int64_t>& mb = gr.of[route];
    const int64_t Bs = (int64_t)mb.size();
    if (!Bs) continue;
    const SubBatch sub = sub_batch(idx, offsets, mb);
    const int64_t Cw = gr.width(route);
    // the route's h2 columns; its results [n_h2][Bs][..]
    std::vector<double> hs((size_t)n_h2 * Bs), fit(hs.size()), ll(hs.size() * nt), s2(ll.size()), bo(ll.size() * Cw);
    for (int64_t g = 0; g < n_h2; ++g)
      for (int64_t i = 0; i < Bs; ++i) hs[g * Bs + i] = h2[g * batch + mb[i]];
    int rc;
    if (route == 2) {
      rc = loglik_fixed_wide(c, split_id, cov, nc, group, L, Cw, sub.si.data(), sub.so.data(), Bs, hs.data(), n_h2,
                             branch, fit.data(), ll.data(), s2.data(), bo.data());
    } else {
      const std::vector<double> x = expand_design(c, cov, nc, group, Cw, route);
      rc = tblup_loglik_cov_batch(c, split_id, x.data(), Cw, sub.si.data(), sub.so.data(), Bs, hs.data(), n_h2, branch,
                                  fit.data(), ll.data(), s2.data(), bo.data());
    }
    if (rc) return rc;
    for (int64_t g = 0; g < n_h2; ++g)
      for (int64_t i = 0; i < Bs; ++i) {
        const int64_t b = mb[i], at = g * Bs + i, to = g * batch + b;
        const int br = branch_of(c, offsets[b + 1] - offsets[b], branch) == 1 ? 0 : 1;
        bool dead = gr.cols[br] == 0 && std::isnan(fit[at]);
        for (int64_t e = 0; e < nt * Cw; ++e) dead = dead || std::isnan(bo[at * nt * Cw + e]);
        if (fitness) fitness[to] = fit[at];
        std::copy(ll.begin() + at * nt, ll.begin() + (at + 1) * nt, loglik + to * nt);
        if (sigma2_g) std::copy(s2.begin() + at * nt, s2.begin() + (at + 1) * nt, sigma2_g + to * nt);
        put_effects(bo.data() + at * nt * Cw, nt, Cw, nc, L, br, dead,
                    cov_effects ? cov_effects + to * nt * nc : nullptr,
                    group_effects ? group_effects + to * nt * L : nullptr);
      }
  }
  return 0;
}

int tblup_reliability_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                                  int64_t n_levels, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                                  const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                                  double* cov_effects, double* cov_center, double* group_effects, double* group_center,
                                  double* intercept, double* center, double* effects, double* reliability,
                                  double* pev_total, double* fixed_cov) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  // (without covariates cov_effects / cov_center are not looked at, as tblup_fit_group_batch)
  const bool cov_out = n_cov > 0 && (cov_effects || cov_center);
  const bool model = cov_out || group_effects || group_center || intercept || center || effects;
  if (model && !(group_effects && group_center && intercept && center && effects &&
                 (n_cov == 0 || (cov_effects && cov_center))))
    return fail(TBLUP_ERR_ARG,
                "cov_effects/cov_center/group_effects/group_center/intercept/center/effects are given together or not "
                "at all");
  if (n_pred > 0 && !animals) return fail(TBLUP_ERR_ARG, "null animals");
  std::vector<int32_t> a32((size_t)n_pred);
  for (int64_t i = 0; i < n_pred; ++i) {
    if (animals[i] < 0 || animals[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    a32[i] = (int32_t)animals[i];
  }
  // the second solve (the model of the adjusted phenotype and its fitness) runs only for a caller who wants it
  const bool full = model || fitness;
  if (batch == 0 || (n_pred == 0 && !full && !fixed_cov)) return 0;
  if (n_pred > 0 && !reliability) return fail(TBLUP_ERR_ARG, "null reliability");
  const int64_t L = n_levels, nc = n_cov, Co = nc + L;
  GroupSplit gs;
  {
    HostBatch hb;
    if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
    if (int rc = check_group_split(hb, cov, nc, group, L, gs)) return rc;
  }
  const int nt = gs.nt;
  GroupRoutes gr;
  if (int rc = route_group(c, offsets, batch, branch, nc, L, gr)) return rc;
  const int64_t total = offsets[batch];
  const double nan = std::nan("");
  for (int route = 0; route < 3; ++route) {
    const std::vector<int64_t>& mb = gr.of[route];
    const int64_t Bs = (int64_t)mb.size();
    if (!Bs) continue;
    const SubBatch sub = sub_batch(idx, offsets, mb);
    const std::vector<int64_t>& so = sub.so;
    const int64_t st = so[Bs], Cw = gr.width(route), Cm = gr.cols[route == 2 ? 0 : route];
    // A route that is the whole batch (its models are then in batch order) writes the per-animal outputs, and the
    // wide route fixed_cov, straight into the caller's arrays: at 128 columns fixed_cov is 128 KiB a model.  Else the
    // route's own: fixed_cov compact [Cm][Cm] from the covariate entry, in the caller's layout from k_fixed_cov.
    const bool whole = Bs == batch, fc_own = fixed_cov && !(whole && route == 2);
    const size_t fc_model = (size_t)(route == 2 ? Co * Co : Cm * Cm);
    std::vector<double> fit(fitness ? (size_t)Bs : 0), rel(whole ? 0 : (size_t)Bs * n_pred),
        pev(pev_total && !whole ? (size_t)Bs * n_pred : 0), fc(fc_own ? (size_t)Bs * fc_model : 0),
        bo(model ? (size_t)Bs * nt * Cw : 0), xc(model ? (size_t)Bs * Cw : 0), icpt(model ? (size_t)Bs * nt : 0),
        cen(model ? (size_t)st : 0), eff(model ? (size_t)nt * st : 0);
    const auto opt = [](std::vector<double>& v, bool on) { return on ? v.data() : nullptr; };
    double *fp = opt(fit, fitness), *bp = opt(bo, model), *ip = opt(icpt, model), *np = opt(cen, model);
    double *ep = opt(eff, model), *rp = whole ? reliability : rel.data();
    double *pp = whole ? pev_total : opt(pev, pev_total), *cp = fc_own ? fc.data() : fixed_cov;
    int rc;
    if (route == 2) {
      rc = reliab_fixed_wide(c, split_id, cov, nc, group, L, Cw, a32, animals, sub.si.data(), so.data(), Bs, h2,
                             branch, full, fp, rp, pp, cp, bp, ip, np, ep);
    } else {
      const std::vector<double> x = expand_design(c, cov, nc, group, Cw, route);
      rc = tblup_reliability_cov_batch(c, split_id, x.data(), Cw, animals, n_pred, sub.si.data(), so.data(), Bs, h2,
                                       branch, fp, bp, opt(xc, model), ip, np, ep, rp, pp, cp);
    }
    if (rc) return rc;
    for (int64_t i = 0; i < Bs; ++i) {
      const int64_t b = mb[i], k = offsets[b + 1] - offsets[b];
      const int br = branch_of(c, k, branch) == 1 ? 0 : 1;
      if (fitness) fitness[b] = fit[i];
      for (int64_t v = 0; v < n_pred; ++v) {
        reliability[b * n_pred + v] = rp[i * n_pred + v];
        // an animal whose label no train animal has: no design row, so no predicted record (PanelModel.predict's rule)
        if (pev_total) pev_total[b * n_pred + v] = group[animals[v]] < 0 ? nan : pp[i * n_pred + v];
      }
      if (fc_own) {
        double* out = fixed_cov + b * Co * Co;
        if (route == 2) {
          std::copy(cp + i * Co * Co, cp + (i + 1) * Co * Co, out);
        } else {
          // the compact G^-1 of the expanded design at the caller's columns: level l is column nc + l - br, and the
          // reference level of an snp model keeps its zeros (NaN throughout for a model that is NaN)
          const double* in = cp + i * Cm * Cm;
          const bool dead = std::isnan(in[0]);
          for (int64_t oi = 0; oi < Co; ++oi)
            for (int64_t oj = 0; oj < Co; ++oj) {
              const int64_t mi = oi < nc ? oi : oi - br, mj = oj < nc ? oj : oj - br;
              const bool ref = br == 1 && (oi == nc || oj == nc);
              out[oi * Co + oj] = dead ? nan : (ref ? 0.0 : in[mi * Cm + mj]);
            }
        }
      }
      if (!model) continue;
      bool dead = gr.cols[br] == 0 && std::isnan(fit[i]);
      for (int64_t e = 0; e < nt * Cw; ++e) dead = dead || std::isnan(bo[i * nt * Cw + e]);
      for (int64_t j = 0; j < nc; ++j) cov_center[b * nc + j] = dead ? nan : (br == 1 ? gs.cov_m[j] : 0.0);
      for (int64_t l = 0; l < L; ++l) group_center[b * L + l] = dead ? nan : (br == 1 ? (double)gs.share[l] : 0.0);
      put_effects(bo.data() + i * nt * Cw, nt, Cw, nc, L, br, dead, nc ? cov_effects + b * nt * nc : nullptr,
                  group_effects + b * nt * L);
      for (int t = 0; t < nt; ++t) {
        intercept[b * nt + t] = ip[i * nt + t];
        std::copy(ep + t * st + so[i], ep + t * st + so[i] + k, effects + t * total + offsets[b]);
      }
      std::copy(np + so[i], np + so[i] + k, center + offsets[b]);
    }
  }
  return 0;
}

int tblup_predict_batch(tblup_ctx* c, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, const double* intercept, const double* center,
                        const double* effects, int64_t n_traits, double* ebv) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (n_traits < 1 || n_traits > MAXT) return fail(TBLUP_ERR_ARG, "need 1 <= n_traits <= 4");
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  if (batch == 0 || n_pred == 0) return 0;
  if (!animals || !idx || !offsets || !intercept || !center || !effects || !ebv)
    return fail(TBLUP_ERR_ARG, "null predict arguments");
  if (offsets[0] != 0) return fail(TBLUP_ERR_ARG, "offsets[0] must be 0");
  if (int rc = check_counts(offsets, batch, "model")) return rc;
  const int64_t total = offsets[batch];
  if (int rc = check_indices(c, idx, total)) return rc;
  std::vector<int32_t> a32((size_t)n_pred);
  for (int64_t i = 0; i < n_pred; ++i) {
    if (animals[i] < 0 || animals[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    a32[i] = (int32_t)animals[i];
  }
  HIPCHK(hipSetDevice(c->device));
  const int nt = (int)n_traits;
  const ChunkBytes bytes_of = [&](const int64_t*, int64_t B, int64_t sum_k) {
    return measure([&](Carve& cv) { PredictBufs::carve(cv, B, sum_k, n_pred, nt); });
  };
  // models per chunk: within the workspace budget (TBLUP_WORKSPACE_MB) and one launch's grid,
  // B * nblk <= 0x7fffffff
  const int64_t nblk = (n_pred + 255) / 256;
  return for_each_chunk(c, offsets, batch, 0x7fffffff / nblk, bytes_of, [&](const Chunk& ck) -> int {
    const int64_t b0 = ck.b0, B = ck.B, sum_k = ck.sum_k;
    Carve cv{(char*)c->ws.p};
    const PredictBufs pb = PredictBufs::carve(cv, B, sum_k, n_pred, nt);
    if (int rc = ws_check(c, cv)) return rc;
    if (int rc = upload_chunk(c, idx, offsets, ck, pb.idx, pb.off)) return rc;
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(pb.an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(pb.icpt, intercept + b0 * nt, (size_t)B * nt * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(pb.cen, center + offsets[b0], (size_t)sum_k * 8, hipMemcpyHostToDevice, s));
    for (int t = 0; t < nt; ++t)
      HIPCHK(hipMemcpyAsync(pb.eff + (int64_t)t * sum_k, effects + (int64_t)t * total + offsets[b0], (size_t)sum_k * 8,
                            hipMemcpyHostToDevice, s));
    HIPCHK(launch_predict((const int8_t*)c->geno_sm.p, c->n, c->P, pb.an, n_pred, pb.idx, pb.off, B, pb.icpt, pb.cen,
                          pb.eff, sum_k, nt, pb.ebv, s));
    HIPCHK(hipMemcpyAsync(ebv + b0 * nt * n_pred, pb.ebv, (size_t)B * nt * n_pred * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
    return 0;
  });
}

}  // extern "C"
