// C ABI of libtblup_gpu.so (include/tblup_gpu.h), the host entries that read the factor the evaluation's
// pipeline leaves in the workspace, each one function on the host-batch driver of capi_ctx.h.  Its body carves
// the entry's buffers (a *Bufs struct below; the chunker measures the same carve), runs the pipeline and then:
//   tblup_fit_batch          k_effects
//   tblup_reliability_batch  k_reliab's launches, k_effects when the model is wanted too
//   tblup_loo_batch          k_effects for the solution alone, k_loo's launches, k_loo_fitness
//   tblup_snp_score_batch    k_snpscore's launches
//   tblup_loglik_batch       the pipeline once per h2 row, k_loglik behind each
// and under fixed effects, with the model's GLS step in front (CovGls: k_covar, the narrow step of up to 16 columns;
// FixedGls: k_fixed_subst and k_fixed_gls, the wide one of up to 128):
//   tblup_fit_cov_batch / fit_fixed_wide                the step, then the second pass: a solve on the adjusted
//                                                       phenotype, the step's fitness kernel, k_effects when wanted
//   tblup_snp_score_cov_batch / score_fixed_wide        the step in keep mode, k_snpscore's adjusted launches
//   tblup_loglik_cov_batch / loglik_fixed_wide          per h2 row the step in keep mode and k_loglik
//   tblup_reliability_cov_batch / reliab_fixed_wide     the step in keep mode, k_reliab's adjusted launches, k_cov_cov /
//                                                       k_fixed_cov; the second pass when the model or its fitness is
//                                                       wanted
// What the variants share is written once: the two GLS steps' buffers, uploads, launches and consumer views (CovGls,
// FixedGls), the second pass and its host post-pass (second_pass, finish_second, post_model), the h2-grid loop
// (h2_grid) and the argument checks (check_*).  The narrow and the wide step run different kernels on different
// layouts, so an entry keeps one body for each.
// tblup_*_group_batch route a batch by its models' column counts (for_each_route): the narrow ones through the
// covariate entry on the expanded design, the wide ones through the *_fixed_wide function, results scattered back.
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
  // the chunk's stretch of the statistics to the host (q null: not wanted)
  int copy_out(const HostBatch& hb, const Chunk& ck, int64_t n_cand, double* score, double* info, double* q_out) const {
    const hipStream_t s = hb.c->stream;
    const int64_t b0 = ck.b0, B = ck.B, nt = hb.d.nt;
    HIPCHK(hipMemcpyAsync(score + b0 * nt * n_cand, sco, (size_t)(B * nt * n_cand) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(info + b0 * n_cand, inf, (size_t)(B * n_cand) * 8, hipMemcpyDeviceToHost, s));
    if (q_out) HIPCHK(hipMemcpyAsync(q_out + b0 * nt, q, (size_t)(B * nt) * 8, hipMemcpyDeviceToHost, s));
    return 0;
  }
};

struct LogLikBufs {   // tblup_loglik_batch, every pass of the chunk
  double *h2, *fits, *ll, *s2;   // h2 rows and fitnesses [n_h2][B]; log-likelihoods and sigma2_g [n_h2][B][nt]
  static LogLikBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_h2) {
    const size_t n = (size_t)n_h2 * B;
    return {cv.take<double>(n), cv.take<double>(n), cv.take<double>(n * hb.d.nt), cv.take<double>(n * hb.d.nt)};
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

// The second pass's device buffers, held by a GLS step carved with `second`: the covariates of the validation rows
// (both planes), z of the adjusted phenotype [B][nt][ns], the first pass's fitness (not returned), the second
// solve's EBVs [B][nt][nV]
struct Second {
  double *qV = nullptr, *z2 = nullptr, *fit0 = nullptr, *ebv2 = nullptr;
  static Second carve(Carve& cv, const HostBatch& hb, int64_t B, bool wanted) {
    if (!wanted) return {};
    const size_t Bt = (size_t)B * hb.d.nt;
    return {cv.take<double>((size_t)2 * COVAR_W * hb.d.nV), cv.take<double>(Bt * hb.sd.ns), cv.take<double>((size_t)B),
            cv.take<double>(Bt * hb.d.nV)};
  }
};

// The narrow GLS step of a chunk (k_covar): one slab per model, a COVAR_W-item list; the knob is k_snpscore's,
// TBLUP_SCORE_LDS.  keep: what k_covar leaves for the adjusted score statistics, likelihood and reliabilities
// (CovKeep) and log|Q~_T^T Q~_T|; keep.sq then doubles as the slices of a plan without LDS.  passes: the h2 rows
// whose effects are kept.  second: the second pass's buffers.
struct CovGls {
  SlabPlan plan;
  int nc;
  double *qT, *b;       // the covariates of the train rows, both planes; their fitted effects [passes][B][nt][nc]
  CovKeep keep;
  double *lqq, *vscr;   // log|Q~_T^T Q~_T| of the two planes (keep); the slices
  Second p2;
  static CovGls carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t n_cov, bool keep, int64_t passes,
                      bool second) {
    CovGls g{plan_slabs(hb, B, COVAR_W, hb.c->score_lds), (int)n_cov};
    g.qT = cv.take<double>((size_t)2 * COVAR_W * hb.d.nTp);
    g.b = cv.take<double>((size_t)passes * B * hb.d.nt * n_cov);
    if (keep) {
      g.keep.sq = cv.take<double>((size_t)B * hb.sd.ns * COVAR_W);
      g.keep.cf = cv.take<double>((size_t)B * COVAR_W * COVAR_W);
      g.keep.ch = cv.take<double>((size_t)B * MAXT * COVAR_W);
      g.keep.ks = cv.take<double>((size_t)B * COVAR_KS);
      g.lqq = cv.take<double>(2);
      g.vscr = g.plan.lds ? nullptr : g.keep.sq;
    } else {
      g.vscr = carve_slices(cv, g.plan);
    }
    g.p2 = Second::carve(cv, hb, B, second);
    return g;
  }
  int upload(const CovPlanes& cp, hipStream_t s) const {
    HIPCHK(hipMemcpyAsync(qT, cp.qT.data(), cp.qT.size() * 8, hipMemcpyHostToDevice, s));
    if (p2.qV) HIPCHK(hipMemcpyAsync(p2.qV, cp.qV.data(), cp.qV.size() * 8, hipMemcpyHostToDevice, s));
    return 0;
  }
  // the step on cl's factor and z: the effects into row `pass`, z* where the second pass's buffers were carved
  int enqueue(const CholLaunch& cl, int64_t pass, hipStream_t s) const {
    HIPCHK(launch_covar(cl, qT, nc, plan, vscr, b + pass * cl.B * cl.d.nt * nc, p2.z2, keep, s));
    return 0;
  }
  // the second pass's fitness, on the launch whose z is z*
  hipError_t fitness(const CholLaunch& cl2, double* d_fit, hipStream_t s) const {
    return launch_cov_fitness(cl2, p2.ebv2, p2.qV, b, nc, d_fit, s);
  }
  ScoreCov score() const { return {keep.sq, keep.cf, keep.ch, keep.ks, qT, nc}; }
  ReliabCov reliab(const double* qa, double* pev) const { return {keep.sq, keep.cf, keep.ks, qa, nc, pev}; }
};

// The wide GLS step of a chunk (k_fixed_subst, k_fixed_gls): a Cw-item list; S's own slabs serve as the slices of
// a plan without LDS.  keep / passes / second: CovGls's.
struct FixedGls {
  SlabPlan plan;
  int nc, L, Cw;
  double* qT;                      // CovGls's
  int32_t *gT, *gV, *lst, *lpos;   // level codes of the train / validation (second) rows; the train rows by level
  double *share, *ff, *fr;         // FixedDesign's
  double *S, *b;                   // [B][Cw / 16][ns][16]; the fitted effects [passes][B][nt][Cw]
  FixedKeep keep;
  double* lqq;                     // log|F~_T^T F~_T| of the two planes (keep)
  Second p2;
  static FixedGls carve(Carve& cv, const HostBatch& hb, int64_t B, const GroupDesign& g, bool keep, int64_t passes,
                        bool second) {
    const EvalDims& d = hb.d;
    const size_t L = (size_t)g.L, Cw = (size_t)g.Cw;
    FixedGls f{plan_slabs(hb, B, g.Cw, hb.c->score_lds), g.nc, g.L, g.Cw};
    f.qT = cv.take<double>((size_t)2 * COVAR_W * d.nTp);
    f.gT = cv.take<int32_t>((size_t)d.nTp);
    f.gV = second ? cv.take<int32_t>((size_t)d.nV) : nullptr;
    f.lst = cv.take<int32_t>(L + 1);
    f.lpos = cv.take<int32_t>((size_t)d.nT);
    f.share = cv.take<double>(L);
    f.ff = cv.take<double>(Cw * Cw);
    f.fr = cv.take<double>((size_t)MAXT * Cw);
    f.S = cv.take<double>((size_t)B * Cw * hb.sd.ns);
    f.b = cv.take<double>((size_t)passes * B * d.nt * Cw);
    if (keep) {
      f.keep.cf = cv.take<double>((size_t)B * Cw * Cw);
      f.keep.ch = cv.take<double>((size_t)B * MAXT * Cw);
      f.keep.ks = cv.take<double>((size_t)B * COVAR_KS);
      f.lqq = cv.take<double>(2);
    }
    f.p2 = Second::carve(cv, hb, B, second);
    return f;
  }
  int upload(const GroupDesign& g, hipStream_t s) const {
    const auto up = [&](void* dst, const void* src, size_t bytes) {
      return bytes && dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(up(qT, g.cp.qT.data(), g.cp.qT.size() * 8));
    HIPCHK(up(p2.qV, g.cp.qV.data(), g.cp.qV.size() * 8));
    HIPCHK(up(gT, g.gT.data(), g.gT.size() * 4));
    HIPCHK(up(gV, g.gV.data(), g.gV.size() * 4));
    HIPCHK(up(lst, g.lst.data(), g.lst.size() * 4));
    HIPCHK(up(lpos, g.lpos.data(), g.lpos.size() * 4));
    HIPCHK(up(share, g.share.data(), g.share.size() * 8));
    HIPCHK(up(ff, g.ff.data(), g.ff.size() * 8));
    HIPCHK(up(fr, g.fr.data(), g.fr.size() * 8));
    return 0;
  }
  FixedDesign design() const { return {qT, p2.qV, gT, gV, lst, lpos, share, ff, fr, nc, L, Cw}; }
  // CovGls::enqueue's, in two launches
  int enqueue(const CholLaunch& cl, int64_t pass, hipStream_t s) const {
    const FixedDesign fd = design();
    HIPCHK(launch_fixed_subst(cl, fd, plan, S, s));
    HIPCHK(launch_fixed_gls(cl, fd, S, b + pass * cl.B * cl.d.nt * Cw, p2.z2, keep, s));
    return 0;
  }
  hipError_t fitness(const CholLaunch& cl2, double* d_fit, hipStream_t s) const {
    return launch_fixed_fitness(cl2, design(), p2.ebv2, b, d_fit, s);
  }
  ScoreFixed score() const { return {S, keep.cf, keep.ch, keep.ks, design()}; }
  ReliabFixed reliab(const double* qa, const int32_t* ga, double* pev) const {
    return {S, keep.cf, keep.ks, qa, ga, design(), pev};
  }
};

// An entry's own buffers with its GLS step's behind them (braces: carved left to right)
template <class Own, class Gls>
struct WithGls {
  Own o;
  Gls k;
};

struct ReliabCovBufs {   // tblup_reliability_cov_batch
  ReliabBufs r;
  CovGls k;
  double *qa, *pev, *cc;   // the listed animals' covariates, both planes [2][n_rel][COVAR_W]; pev_total [B][n_rel]
                           // and cov_cov [B][n_cov][n_cov] where wanted
  static ReliabCovBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t n_rel, int64_t n_cov,
                             bool model, bool full, bool pev, bool cc) {
    ReliabCovBufs b{ReliabBufs::carve(cv, hb, B, sum_k, n_rel, model), CovGls::carve(cv, hb, B, n_cov, true, 1, full)};
    b.qa = cv.take<double>((size_t)2 * n_rel * COVAR_W);
    b.pev = pev ? cv.take<double>((size_t)B * n_rel) : nullptr;
    b.cc = cc ? cv.take<double>((size_t)B * n_cov * n_cov) : nullptr;
    return b;
  }
};

struct ReliabFixedBufs {   // tblup_reliability_group_batch, the models of more than COVAR_W columns
  ReliabBufs r;
  FixedGls k;
  double* qa;         // ReliabCovBufs'
  int32_t* ga;        // the listed animals' level codes [n_rel]
  double *pev, *fc;   // pev_total [B][n_rel] and fixed_cov [B][n_cov + L][n_cov + L] where wanted
  static ReliabFixedBufs carve(Carve& cv, const HostBatch& hb, int64_t B, int64_t sum_k, int64_t n_rel,
                               const GroupDesign& g, bool model, bool full, bool pev, bool fc) {
    const size_t Co = (size_t)(g.nc + g.L);
    ReliabFixedBufs b{ReliabBufs::carve(cv, hb, B, sum_k, n_rel, model), FixedGls::carve(cv, hb, B, g, true, 1, full)};
    b.qa = cv.take<double>((size_t)2 * n_rel * COVAR_W);
    b.ga = cv.take<int32_t>((size_t)n_rel);
    b.pev = pev ? cv.take<double>((size_t)B * n_rel) : nullptr;
    b.fc = fc ? cv.take<double>((size_t)B * Co * Co) : nullptr;
    return b;
  }
};

// ---- the second pass on the adjusted phenotype ----
// What a second pass copies to the host, the chunk's stretch of each
struct SecondOut {
  const ModelBufs* m;          // k_effects' model into center / effects; null: not wanted
  double *center, *effects;
  double* b;                   // the GLS effects [batch][nt][cols] from d_b; null: not wanted
  const double* d_b;
  int64_t cols;
  double *fitness, *ebv;       // ebv [batch][nt][nV]; null: not wanted
};
// One chunk of tblup_fit_cov_batch and of every entry that runs its second pass: the pipeline with the
// one-workgroup solve (nothing to recover; its fitness goes to fit0 and its EBVs are not wanted), after(cl) on the
// factor and z it leaves -- the GLS step, which writes z*, and whatever else reads the kept step -- then the solve,
// fitness_launch(cl2, d_fit) and the model of the adjusted phenotype on z*; the copies out, and the host waits.
int second_pass(const HostBatch& hb, const Chunk& ck, const Carve& cv, ChunkReq& rq, const Second& p2,
                const std::function<int(const CholLaunch&)>& after,
                const std::function<hipError_t(const CholLaunch&, double*)>& fitness_launch, const SecondOut& o) {
  const hipStream_t s = hb.c->stream;
  const int64_t b0 = ck.b0, B = ck.B, nt = hb.d.nt, nV = hb.d.nV;
  double* d_fit = rq.d_fit;
  Carve cvp = cv;
  rq.mode = ChunkMode::NoChain;
  rq.d_fit = p2.fit0;
  ChunkRes res;
  if (int rc = run_chunk(hb.c, rq, cvp, res)) return rc;
  if (int rc = after(res.cl)) return rc;
  CholLaunch cl2 = res.cl;
  cl2.z = p2.z2;
  HIPCHK(launch_solve(cl2, nullptr, p2.fit0, p2.ebv2, s));
  HIPCHK(fitness_launch(cl2, d_fit));
  if (o.m)
    if (int rc = o.m->enqueue(hb, ck, cl2, o.center, o.effects)) return rc;
  if (o.b) HIPCHK(hipMemcpyAsync(o.b + b0 * nt * o.cols, o.d_b, (size_t)(B * nt * o.cols) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.fitness + b0, d_fit, (size_t)B * 8, hipMemcpyDeviceToHost, s));
  if (o.ebv) HIPCHK(hipMemcpyAsync(o.ebv + b0 * nt * nV, p2.ebv2, (size_t)(B * nt * nV) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
  return 0;
}

// The host post-pass of one model fitted under fixed effects: bt [nt][stride] its effects by column (zero past
// its own `cols`), fit its fitness.  A model whose effects are NaN (d = 0, a flagged index, a collinear design) is
// dead; one without a fixed column has no effect to tell by: its NaN fitness tells.  A dead model is NaN in
// intercept [nt] and center [k] (null: not wanted).  Returns dead.
bool post_model(const double* bt, int nt, int64_t stride, int64_t cols, double fit, double* intercept, double* center,
                int64_t k) {
  bool dead = cols == 0 && std::isnan(fit);
  for (int64_t i = 0; i < nt * stride; ++i) dead = dead || std::isnan(bt[i]);
  if (dead && intercept) std::fill(intercept, intercept + nt, std::nan(""));
  if (dead && center) std::fill(center, center + k, std::nan(""));
  return dead;
}
// ... and the centres of n of its fixed columns: the train means m under snp, 0 under gblup, NaN for a dead model
void put_centres(double* out, const double* m, int64_t n, bool snp, bool dead) {
  for (int64_t j = 0; j < n; ++j) out[j] = dead ? std::nan("") : (snp ? m[j] : 0.0);
}
// The post-pass of a second-pass entry over its batch: the intercepts, then post_model on every model's effects
// b [batch][nt][stride] (cols: the fixed columns of a gblup / an snp model), and put_centres on ctr [batch][stride]
// from m where the entry returns centres.  intercept and center come together (null: no model wanted).
void finish_second(const HostBatch& hb, const double* fitness, const double* b, int64_t stride, int64_t cols_gblup,
                   int64_t cols_snp, const double* m, double* ctr, double* intercept, double* center) {
  const int nt = hb.d.nt;
  if (intercept) fill_intercepts(hb, intercept);
  for (int64_t i = 0; i < hb.batch; ++i) {
    const int64_t k = hb.offsets[i + 1] - hb.offsets[i];
    const bool snp = branch_of(hb.c, k, hb.branch) == 2;
    const bool dead = post_model(b + i * nt * stride, nt, stride, snp ? cols_snp : cols_gblup, fitness[i],
                                 intercept ? intercept + i * nt : nullptr, intercept ? center + hb.offsets[i] : nullptr, k);
    if (ctr) put_centres(ctr + i * stride, m, stride, snp, dead);
  }
}

// ---- the h2-grid loop of the likelihood entries ----
// One chunk of tblup_loglik_batch and its variants: the chunk's h2 columns up front, the n_h2 passes back to back
// (each the pipeline at its row of per-system h2, then per_pass(cl, g) on the factor it leaves, without waiting for
// the solve: the entry's launches up to k_loglik into row g of lb.ll / lb.s2), the results of every pass copied out
// behind the last.  redo: a chained solve of some pass gave up a wait -- the factors of all but the last pass are
// gone, so every pass runs again whole with the one-workgroup k_solve (the same bits), for the fitnesses only.
// fitness behind either pass, the rest behind pass 0 only; a null output is skipped.  extra [n_h2][batch][row]
// from d_extra: the entry's per-pass effects (xrow doubles a model).
int h2_grid(const HostBatch& hb, const Chunk& ck, const Carve& cv, ChunkReq& rq, const LogLikBufs& lb, const double* h2,
            int64_t n_h2, const std::function<int(const CholLaunch& cl, int64_t g)>& per_pass, double* fitness,
            double* loglik, double* sigma2_g, double* extra = nullptr, const double* d_extra = nullptr,
            int64_t xrow = 0) {
  tblup_ctx* c = hb.c;
  const hipStream_t s = c->stream;
  const int64_t b0 = ck.b0, B = ck.B, nt = hb.d.nt;
  const size_t row = (size_t)B * 8, pitch = (size_t)hb.batch * 8;
  HIPCHK(hipMemcpy2DAsync(lb.h2, row, h2 + b0, pitch, row, (size_t)n_h2, hipMemcpyHostToDevice, s));
  return run_recovering(c, [&](bool redo, std::vector<int32_t>& seqs) -> int {
    for (int64_t g = 0; g < n_h2; ++g) {
      Carve cvp = cv;
      rq.mode = redo ? ChunkMode::NoChain : ChunkMode::Full;
      rq.d_h2 = lb.h2 + g * B;
      rq.d_fit = lb.fits + g * B;
      ChunkRes res;
      if (int rc = run_chunk(c, rq, cvp, res)) return rc;
      seqs.push_back(res.chain_seq);
      if (!redo)
        if (int rc = per_pass(res.cl, g)) return rc;
    }
    // n_h2 rows of `per` doubles a model to the host
    const auto out = [&](double* host, const double* dev, int64_t per) {
      return host ? hipMemcpy2DAsync(host + b0 * per, pitch * per, dev, row * per, row * per, (size_t)n_h2,
                                     hipMemcpyDeviceToHost, s)
                  : hipSuccess;
    };
    HIPCHK(out(fitness, lb.fits, 1));
    if (redo) return 0;
    HIPCHK(out(loglik, lb.ll, nt));
    HIPCHK(out(sigma2_g, lb.s2, nt));
    HIPCHK(out(extra, d_extra, xrow));
    return 0;
  });
}

// ---- argument checks the entries share ----
int check_panel(const tblup_ctx* c) {
  return c->n == 0 ? fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)") : 0;
}
// the animal list as rows of the panel: a32
int check_animals(const tblup_ctx* c, const int64_t* animals, int64_t n_pred, std::vector<int32_t>& a32) {
  if (n_pred > 0 && !animals) return fail(TBLUP_ERR_ARG, "null animals");
  a32.resize((size_t)n_pred);
  for (int64_t i = 0; i < n_pred; ++i) {
    if (animals[i] < 0 || animals[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    a32[i] = (int32_t)animals[i];
  }
  return 0;
}
// the SNP list as columns of the panel: s32
int check_snps(const tblup_ctx* c, const int64_t* snps, int64_t n_cand, std::vector<int32_t>& s32) {
  if (n_cand > 0 && !snps) return fail(TBLUP_ERR_ARG, "null snps");
  if (int rc = check_indices(c, snps, n_cand)) return rc;
  s32.resize((size_t)n_cand);
  for (int64_t i = 0; i < n_cand; ++i) s32[i] = (int32_t)snp_col(snps[i], c->P);
  return 0;
}
// lambda = 0 makes the snp branch's V singular: (0, 1) for the entries that need V's inverse, not
// tblup_eval_batch's (0, 1]
int check_h2_open(double h2) {
  return !(h2 > 0.0) || !(h2 < 1.0) ? fail(TBLUP_ERR_ARG, "h2 must be in (0, 1)") : 0;
}
int check_h2_grid(const double* h2, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!(h2[i] > 0.0) || !(h2[i] < 1.0)) return fail(TBLUP_ERR_ARG, "every h2 must be in (0, 1)");
  return 0;
}
// k_effects' outputs are given together or not at all; model: given
int check_model_out(const double* intercept, const double* center, const double* effects, bool& model) {
  model = intercept || center || effects;
  if (model && !(intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "intercept/center/effects are given together or not at all");
  return 0;
}
// The fixed-design rows of the listed animals: qa [2][n_pred][COVAR_W] their covariates, plane 0 as given, plane 1
// centred by the train means m, zero past n_cov; with group, ga [n_pred] their level codes
std::vector<double> gather_listed(const double* cov, int64_t n_cov, const std::vector<double>& m, const int64_t* animals,
                                  int64_t n_pred, const int64_t* group = nullptr, std::vector<int32_t>* ga = nullptr) {
  std::vector<double> qa((size_t)2 * n_pred * COVAR_W, 0.0);
  if (ga) ga->resize((size_t)n_pred);
  for (int64_t v = 0; v < n_pred; ++v) {
    for (int64_t j = 0; j < n_cov; ++j) {
      const double q = cov[animals[v] * n_cov + j];
      qa[v * COVAR_W + j] = q;
      qa[(n_pred + v) * COVAR_W + j] = q - m[j];
    }
    if (ga) (*ga)[v] = (int32_t)group[animals[v]];
  }
  return qa;
}

// ---- the class factor: its checks, and the routes of a batch ----
// The arguments a class-factor entry passes on to its routes
struct GroupCall {
  tblup_ctx* c;
  int split_id;
  const double* cov;
  int64_t nc;
  const int64_t* group;
  int64_t L;
  const int64_t *idx, *offsets;
  int64_t batch;
  int branch;
};

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
  std::vector<double> share, cov_m;
  int64_t nT = 0, nV = 0;
  int nt = 1;
};
int check_group_split(const HostBatch& hb, const double* cov, int64_t nc, const int64_t* group, int64_t L,
                      GroupSplit& gs) {
  const int64_t nT = gs.nT = hb.d.nT, nV = gs.nV = hb.d.nV;
  gs.nt = hb.d.nt;
  std::vector<long double> count((size_t)std::min<int64_t>(L, hb.c->n + 1), 0.0L);
  gs.cov_m.resize((size_t)nc);
  if (L > nT) return fail(TBLUP_ERR_ARG, "a level has no train row");
  for (int64_t i = 0; i < nT; ++i) {
    if (group[hb.sp->train[i]] < 0) return fail(TBLUP_ERR_ARG, "an animal of the split has no level (-1)");
    count[group[hb.sp->train[i]]] += 1.0L;
  }
  for (int64_t i = 0; i < nV; ++i)
    if (group[hb.sp->valid[i]] < 0) return fail(TBLUP_ERR_ARG, "an animal of the split has no level (-1)");
  gs.share.resize((size_t)L);
  for (int64_t l = 0; l < L; ++l) {
    if (count[l] == 0.0L) return fail(TBLUP_ERR_ARG, "a level has no train row");
    gs.share[l] = (double)(count[l] / (long double)nT);
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

// One non-empty route of a call, as for_each_route hands it to the entry: its models as a batch of their own
// (idx / off, Bs of them, route model i is batch model mb[i] of branch br[i]: 0 gblup, 1 snp), the column stride
// Cw of its effects and, routes 0 / 1, the expanded design x [n][Cw] = [Q, Z]: every level under gblup, all but
// the lowest under snp; an animal without a level (outside the split) has a row of zeros in Z.
struct Route {
  const GroupCall& a;
  const GroupSplit& gs;
  int id;
  const std::vector<int64_t>& mb;
  int64_t Bs, Cw;
  int64_t cols[2];   // the fixed columns of a gblup / an snp model
  std::vector<int64_t> so, si;
  std::vector<int> br;
  std::vector<double> x;
  const int64_t* idx() const { return si.data(); }
  const int64_t* off() const { return so.data(); }
  // a row-shaped output of the route, src [n_h2][Bs][len], into the batch's dst [n_h2][batch][len] (null: not wanted)
  void scatter(const double* src, int64_t len, double* dst, int64_t n_h2 = 1) const {
    if (!dst) return;
    for (int64_t g = 0; g < n_h2; ++g)
      for (int64_t i = 0; i < Bs; ++i)
        std::copy(src + (g * Bs + i) * len, src + (g * Bs + i + 1) * len, dst + (g * a.batch + mb[i]) * len);
  }
  // its fitted effects bo [n_h2][Bs][nt][Cw] (fit [n_h2][Bs]: the fitnesses, for post_model) as the batch's
  // cov_effects [n_h2][batch][nt][nc] and group_effects [n_h2][batch][nt][L], and with centres (n_h2 = 1) those of
  // the covariates [batch][nc] and of the levels [batch][L]; a null output is skipped
  void put_fixed(const double* bo, const double* fit, double* cov_eff, double* grp_eff, int64_t n_h2 = 1,
                 double* cov_center = nullptr, double* group_center = nullptr) const {
    const int64_t nt = gs.nt, nc = a.nc, L = a.L;
    for (int64_t g = 0; g < n_h2; ++g)
      for (int64_t i = 0; i < Bs; ++i) {
        const int64_t b = mb[i], at = g * Bs + i, to = g * a.batch + b;
        const double* bt = bo + at * nt * Cw;
        const bool dead = post_model(bt, (int)nt, Cw, cols[br[i]], fit[at], nullptr, nullptr, 0);
        put_effects(bt, (int)nt, Cw, nc, L, br[i], dead, cov_eff ? cov_eff + to * nt * nc : nullptr,
                    grp_eff ? grp_eff + to * nt * L : nullptr);
        if (cov_center) put_centres(cov_center + b * nc, gs.cov_m.data(), nc, br[i] == 1, dead);
        if (group_center) put_centres(group_center + b * L, gs.share.data(), L, br[i] == 1, dead);
      }
  }
};
// A route's k_effects model where wanted (null pointers else): intercept [Bs][nt], center [st], effects [nt][st]
struct RouteModel {
  std::vector<double> icpt, cen, eff;
  double *ip = nullptr, *cp = nullptr, *ep = nullptr;
  RouteModel(const Route& r, bool wanted) {
    if (!wanted) return;
    const int64_t st = r.so[r.Bs];
    icpt.resize((size_t)r.Bs * r.gs.nt);
    cen.resize((size_t)st);
    eff.resize((size_t)r.gs.nt * st);
    ip = icpt.data();
    cp = cen.data();
    ep = eff.data();
  }
  void scatter(const Route& r, double* intercept, double* center, double* effects) const {
    const int64_t *offsets = r.a.offsets, st = r.so[r.Bs], total = offsets[r.a.batch];
    r.scatter(ip, r.gs.nt, intercept);
    for (int64_t i = 0; i < r.Bs; ++i) {
      const int64_t b = r.mb[i], k = offsets[b + 1] - offsets[b];
      std::copy(cp + r.so[i], cp + r.so[i] + k, center + offsets[b]);
      for (int t = 0; t < r.gs.nt; ++t)
        std::copy(ep + t * st + r.so[i], ep + t * st + r.so[i] + k, effects + t * total + offsets[b]);
    }
  }
};

// The class-factor entries' driver: the batch's checks against the split (h2: any of the call's, for the batch's
// validation), its routes, and `body` on each non-empty one in turn.  An empty batch is no route.
int for_each_route(const GroupCall& a, double h2, const std::function<int(const Route&)>& body) {
  GroupSplit gs;
  {
    HostBatch hb;
    if (int rc = open_host_batch(hb, a.c, a.split_id, a.idx, a.offsets, a.batch, h2, a.branch, true)) return rc;
    if (!hb.sp) return 0;
    if (int rc = check_group_split(hb, a.cov, a.nc, a.group, a.L, gs)) return rc;
  }
  GroupRoutes gr;
  if (int rc = route_group(a.c, a.offsets, a.batch, a.branch, a.nc, a.L, gr)) return rc;
  for (int route = 0; route < 3; ++route) {
    const std::vector<int64_t>& mb = gr.of[route];
    if (mb.empty()) continue;
    Route r{a, gs, route, mb, (int64_t)mb.size(), gr.width(route), {gr.cols[0], gr.cols[1]}};
    r.so.assign(mb.size() + 1, 0);
    for (size_t i = 0; i < mb.size(); ++i) {
      const int64_t lo = a.offsets[mb[i]], hi = a.offsets[mb[i] + 1];
      r.si.insert(r.si.end(), a.idx + lo, a.idx + hi);
      r.so[i + 1] = (int64_t)r.si.size();
      r.br.push_back(branch_of(a.c, hi - lo, a.branch) == 1 ? 0 : 1);
    }
    if (route < 2) {
      r.x.assign((size_t)a.c->n * r.Cw, 0.0);
      for (int64_t an = 0; an < a.c->n; ++an) {
        for (int64_t j = 0; j < a.nc; ++j) r.x[an * r.Cw + j] = a.cov[an * a.nc + j];
        const int64_t z = a.group[an] - route;
        if (z >= 0) r.x[an * r.Cw + a.nc + z] = 1.0;
      }
    }
    if (int rc = body(r)) return rc;
  }
  return 0;
}

// ---- the wide route of the class-factor entries: a route's models through k_fixed ----
// Opens the route's batch and gathers its design
int open_wide(const Route& r, double h2, HostBatch& hb, GroupDesign& g) {
  const GroupCall& a = r.a;
  if (int rc = open_host_batch(hb, a.c, a.split_id, r.idx(), r.off(), r.Bs, h2, a.branch, true)) return rc;
  g = gather_group(hb, a.cov, a.nc, a.group, a.L, r.Cw);
  return 0;
}

// tblup_fit_group_batch's: tblup_fit_cov_batch's chunk and post-pass with FixedGls in place of CovGls.
// bout [Bs][nt][Cw] the fitted effects by column (zero past a model's own), everything else that entry's.
int fit_fixed_wide(const Route& r, double h2, double* fitness, double* ebv, double* bout, double* intercept,
                   double* center, double* effects) {
  const bool model = intercept != nullptr;
  HostBatch hb;
  GroupDesign g;
  if (int rc = open_wide(r, h2, hb, g)) return rc;
  using Bufs = WithGls<ModelBufs, FixedGls>;
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) {
    return Bufs{ModelBufs::carve(cv, hb, sk, model), FixedGls::carve(cv, hb, B, g, false, 1, true)};
  };
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = hb.c->stream;
    const Bufs fb = carve(cv, ck.B, ck.sum_k);
    if (int rc = ws_check(hb.c, cv)) return rc;
    if (int rc = fb.k.upload(g, s)) return rc;
    return second_pass(
        hb, ck, cv, rq, fb.k.p2, [&](const CholLaunch& cl) { return fb.k.enqueue(cl, 0, s); },
        [&](const CholLaunch& cl2, double* d_fit) { return fb.k.fitness(cl2, d_fit, s); },
        {model ? &fb.o : nullptr, center, effects, bout, fb.k.b, r.Cw, fitness, ebv});
  });
  if (rc || !model) return rc;
  finish_second(hb, fitness, bout, r.Cw, r.cols[0], r.cols[1], nullptr, nullptr, intercept, center);
  return 0;
}

// tblup_snp_score_group_batch's: tblup_snp_score_cov_batch's chunk with FixedGls in place of CovGls and
// k_snpscore's FIX instances behind it.  bout: fit_fixed_wide's.
int score_fixed_wide(const Route& r, const std::vector<int32_t>& s32, double h2, double* fitness, double* score,
                     double* info, double* q, double* bout) {
  HostBatch hb;
  GroupDesign g;
  if (int rc = open_wide(r, h2, hb, g)) return rc;
  tblup_ctx* c = hb.c;
  const int64_t nt = hb.d.nt, n_cand = (int64_t)s32.size(), Cw = r.Cw;
  using Bufs = WithGls<ScoreBufs, FixedGls>;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) {
    return Bufs{ScoreBufs::carve(cv, hb, B, n_cand), FixedGls::carve(cv, hb, B, g, true, 1, false)};
  };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const Bufs bufs = carve(cv, B, ck.sum_k);
    const ScoreBufs& sb = bufs.o;
    const FixedGls& kb = bufs.k;
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpyAsync(sb.cand, s32.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
    if (int rc = kb.upload(g, s)) return rc;
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      if (int rc = kb.enqueue(cl, 0, s)) return rc;
      HIPCHK(launch_snpscore_fixed(cl, (const int32_t*)c->colsum_all.p, sb.cand, n_cand, sb.plan, sb.vscr, kb.score(),
                                   sb.sco, sb.inf, sb.q, s));
      if (int rc = sb.copy_out(hb, ck, n_cand, score, info, q)) return rc;
      HIPCHK(hipMemcpyAsync(bout + b0 * nt * Cw, kb.b, (size_t)(B * nt * Cw) * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
}

// tblup_loglik_group_batch's: tblup_loglik_cov_batch's passes with FixedGls in place of CovGls and k_loglik with
// the model's own column count.  h2 [n_h2][Bs]; bout [n_h2][Bs][nt][Cw].
int loglik_fixed_wide(const Route& r, const double* h2, int64_t n_h2, double* fitness, double* loglik,
                      double* sigma2_g, double* bout) {
  HostBatch hb;
  GroupDesign g;
  if (int rc = open_wide(r, h2[0], hb, g)) return rc;
  const int64_t nt = hb.d.nt;
  // log|F~_T^T F~_T| does not depend on h2: once per call, for the planes that the batch has models of
  bool need[2] = {false, false};
  for (int b : r.br) need[b] = true;
  double lqq[2];
  group_log_dets(hb, r.a.cov, g, need, lqq);
  // (a plane without a model is not read; its count only has to pass the launcher's range check)
  const int kcols[2] = {need[0] ? (int)r.cols[0] : 0, need[1] ? (int)r.cols[1] : 0};
  using Bufs = WithGls<LogLikBufs, FixedGls>;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) {
    return Bufs{LogLikBufs::carve(cv, hb, B, n_h2), FixedGls::carve(cv, hb, B, g, true, n_h2, false)};
  };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = hb.c->stream;
    const int64_t B = ck.B;
    const Bufs bufs = carve(cv, B, ck.sum_k);
    const LogLikBufs& lb = bufs.o;
    const FixedGls& kb = bufs.k;
    if (int rc = ws_check(hb.c, cv)) return rc;
    if (int rc = kb.upload(g, s)) return rc;
    HIPCHK(hipMemcpyAsync(kb.lqq, lqq, sizeof(lqq), hipMemcpyHostToDevice, s));
    const auto per_pass = [&](const CholLaunch& cl, int64_t gi) -> int {
      if (int rc = kb.enqueue(cl, gi, s)) return rc;
      HIPCHK(launch_loglik_fixed(cl, kb.keep.ks, kb.lqq, kcols, lb.ll + gi * B * nt, lb.s2 + gi * B * nt, s));
      return 0;
    };
    return h2_grid(hb, ck, cv, rq, lb, h2, n_h2, per_pass, fitness, loglik, sigma2_g, bout, kb.b, nt * r.Cw);
  });
}

// tblup_reliability_group_batch's: tblup_reliability_cov_batch's chunk with FixedGls in place of CovGls, k_reliab's
// FIX instances and k_fixed_cov behind it, and fit_fixed_wide's second pass when the model or its fitness is wanted
// (full).  a32 / animals: the list; rel / pev [Bs][n_pred], fc [Bs][(n_cov + L)^2] (pev, fc: null when not
// wanted); bout [Bs][nt][Cw] and intercept / center / effects: fit_fixed_wide's, with model.
int reliab_fixed_wide(const Route& r, const std::vector<int32_t>& a32, const int64_t* animals, double h2, bool full,
                      double* fitness, double* rel, double* pev, double* fc, double* bout, double* intercept,
                      double* center, double* effects) {
  const bool model = intercept != nullptr;
  HostBatch hb;
  GroupDesign g;
  if (int rc = open_wide(r, h2, hb, g)) return rc;
  tblup_ctx* c = hb.c;
  fitness = hb.fitness_or_own(fitness);
  const int64_t n_pred = (int64_t)a32.size(), Co = r.a.nc + r.a.L;
  std::vector<int32_t> h_ga;
  const std::vector<double> h_qa = gather_listed(r.a.cov, r.a.nc, g.cp.m, animals, n_pred, r.a.group, &h_ga);
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) {
    return ReliabFixedBufs::carve(cv, hb, B, sk, n_pred, g, model, full, pev != nullptr, fc != nullptr);
  };
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ReliabFixedBufs rb = carve(cv, B, ck.sum_k);
    const FixedGls& kb = rb.k;
    if (int rc = ws_check(c, cv)) return rc;
    if (n_pred > 0) {
      HIPCHK(hipMemcpyAsync(rb.r.an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(rb.qa, h_qa.data(), h_qa.size() * 8, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(rb.ga, h_ga.data(), h_ga.size() * 4, hipMemcpyHostToDevice, s));
    }
    if (int rc = kb.upload(g, s)) return rc;
    const auto after = [&](const CholLaunch& cl) -> int {
      if (int rc = kb.enqueue(cl, 0, s)) return rc;
      HIPCHK(launch_reliab_fixed(cl, (const int8_t*)c->geno_sm.p, (const int32_t*)c->colsum_all.p, rb.r.an, n_pred,
                                 rb.r.plan, rb.r.vscr, kb.reliab(rb.qa, rb.ga, rb.pev), rb.r.rel, s));
      if (n_pred > 0) {
        HIPCHK(hipMemcpyAsync(rel + b0 * n_pred, rb.r.rel, (size_t)(B * n_pred) * 8, hipMemcpyDeviceToHost, s));
        if (pev) HIPCHK(hipMemcpyAsync(pev + b0 * n_pred, rb.pev, (size_t)(B * n_pred) * 8, hipMemcpyDeviceToHost, s));
      }
      if (fc) {
        HIPCHK(launch_fixed_cov(cl, kb.design(), kb.keep.cf, kb.keep.ks, rb.fc, s));
        HIPCHK(hipMemcpyAsync(fc + b0 * Co * Co, rb.fc, (size_t)(B * Co * Co) * 8, hipMemcpyDeviceToHost, s));
      }
      return 0;
    };
    if (!full) return factor_pass(hb, ck, cv, rq, fitness, nullptr, after);
    return second_pass(
        hb, ck, cv, rq, kb.p2, after, [&](const CholLaunch& cl2, double* d_fit) { return kb.fitness(cl2, d_fit, s); },
        {model ? &rb.r.m : nullptr, center, effects, bout, kb.b, r.Cw, fitness, nullptr});
  });
  if (rc || !model) return rc;
  finish_second(hb, fitness, bout, r.Cw, r.cols[0], r.cols[1], nullptr, nullptr, intercept, center);
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
  if (int rc = check_panel(c)) return rc;
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  bool model;
  if (int rc = check_model_out(intercept, center, effects, model)) return rc;
  std::vector<int32_t> a32;
  if (int rc = check_animals(c, animals, n_pred, a32)) return rc;
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
  if (int rc = check_panel(c)) return rc;
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
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  const bool model = cov_effects || cov_center || intercept || center || effects;
  if (model && !(cov_effects && cov_center && intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "cov_effects/cov_center/intercept/center/effects are given together or not at all");
  std::vector<int32_t> a32;
  if (int rc = check_animals(c, animals, n_pred, a32)) return rc;
  // the second solve (the model of the adjusted phenotype and its fitness) runs only for a caller who wants it
  const bool full = model || fitness;
  if (batch == 0 || (n_pred == 0 && !full && !cov_cov)) return 0;
  if (n_pred > 0 && !reliability) return fail(TBLUP_ERR_ARG, "null reliability");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const int nc = (int)n_cov;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, full);
  const std::vector<double> h_qa = gather_listed(cov, n_cov, cp.m, animals, n_pred);
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) {
    return ReliabCovBufs::carve(cv, hb, B, sk, n_pred, n_cov, model, full, pev_total != nullptr, cov_cov != nullptr);
  };
  // per chunk, behind the pipeline: k_covar keeps the model's GLS step, k_reliab's covariate-adjusted launches
  // and k_cov_cov read it; a caller who wants the model or its fitness gets tblup_fit_cov_batch's second pass
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const ReliabCovBufs rb = carve(cv, B, ck.sum_k);
    const CovGls& kb = rb.k;
    if (int rc = ws_check(c, cv)) return rc;
    if (n_pred > 0) {
      HIPCHK(hipMemcpyAsync(rb.r.an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(rb.qa, h_qa.data(), h_qa.size() * 8, hipMemcpyHostToDevice, s));
    }
    if (int rc = kb.upload(cp, s)) return rc;
    const auto after = [&](const CholLaunch& cl) -> int {
      if (int rc = kb.enqueue(cl, 0, s)) return rc;
      const ReliabCov rcv = kb.reliab(rb.qa, rb.pev);
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
    return second_pass(
        hb, ck, cv, rq, kb.p2, after, [&](const CholLaunch& cl2, double* d_fit) { return kb.fitness(cl2, d_fit, s); },
        {model ? &rb.r.m : nullptr, center, effects, cov_effects, kb.b, n_cov, fitness, nullptr});
  });
  if (rc || !model) return rc;
  finish_second(hb, fitness, cov_effects, n_cov, n_cov, n_cov, cp.m.data(), cov_center, intercept, center);
  return 0;
}

int tblup_snp_score_batch(tblup_ctx* c, int split_id, const int64_t* snps, int64_t n_cand, const int64_t* idx,
                          const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness, double* score,
                          double* info, double* q) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (batch < 0 || n_cand < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_cand");
  std::vector<int32_t> s32;
  if (int rc = check_snps(c, snps, n_cand, s32)) return rc;
  if (batch == 0 || n_cand == 0) return 0;
  if (int rc = check_h2_open(h2)) return rc;
  if (!score || !info) return fail(TBLUP_ERR_ARG, "null score/info");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return ScoreBufs::carve(cv, hb, B, n_cand); };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const ScoreBufs sb = carve(cv, ck.B, ck.sum_k);
    HIPCHK(hipMemcpyAsync(sb.cand, s32.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      HIPCHK(launch_snpscore(cl, (const int32_t*)c->colsum_all.p, sb.cand, n_cand, sb.plan, sb.vscr, nullptr, sb.sco,
                             sb.inf, sb.q, s));
      return sb.copy_out(hb, ck, n_cand, score, info, q);
    });
  });
}

int tblup_loglik_batch(tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch,
                       const double* h2, int64_t n_h2, int branch, double* fitness, double* loglik,
                       double* sigma2_g) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (batch < 0 || n_h2 < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_h2");
  if (batch == 0 || n_h2 == 0) return 0;
  if (!h2 || !loglik) return fail(TBLUP_ERR_ARG, "null h2/loglik");
  if (int rc = check_h2_grid(h2, n_h2 * batch)) return rc;
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2[0], branch, true)) return rc;
  const int64_t nt = hb.d.nt;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) { return LogLikBufs::carve(cv, hb, B, n_h2); };
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const int64_t B = ck.B;
    const LogLikBufs lb = carve(cv, B, ck.sum_k);
    if (int rc = ws_check(c, cv)) return rc;
    const auto per_pass = [&](const CholLaunch& cl, int64_t g) -> int {
      HIPCHK(launch_loglik(cl, nullptr, nullptr, 0, lb.ll + g * B * nt, lb.s2 + g * B * nt, c->stream));
      return 0;
    };
    return h2_grid(hb, ck, cv, rq, lb, h2, n_h2, per_pass, fitness, loglik, sigma2_g);
  });
}

int tblup_fit_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness, double* ebv,
                        double* cov_effects, double* cov_center, double* intercept, double* center, double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  bool model;
  if (int rc = check_model_out(intercept, center, effects, model)) return rc;
  if (batch > 0 && (!cov_effects || !cov_center)) return fail(TBLUP_ERR_ARG, "null cov_effects/cov_center");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  if (!hb.sp) return 0;
  fitness = hb.fitness_or_own(fitness);
  const CovPlanes cp = gather_cov(hb, cov, n_cov, true);
  using Bufs = WithGls<ModelBufs, CovGls>;
  const auto carve = [&](Carve& cv, int64_t B, int64_t sk) {
    return Bufs{ModelBufs::carve(cv, hb, sk, model), CovGls::carve(cv, hb, B, n_cov, false, 1, true)};
  };
  // per chunk: the second pass behind k_covar, see second_pass
  const int rc = run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const Bufs cb = carve(cv, ck.B, ck.sum_k);
    if (int rc = ws_check(c, cv)) return rc;
    if (int rc = cb.k.upload(cp, s)) return rc;
    return second_pass(
        hb, ck, cv, rq, cb.k.p2, [&](const CholLaunch& cl) { return cb.k.enqueue(cl, 0, s); },
        [&](const CholLaunch& cl2, double* d_fit) { return cb.k.fitness(cl2, d_fit, s); },
        {model ? &cb.o : nullptr, center, effects, cov_effects, cb.k.b, n_cov, fitness, ebv});
  });
  if (rc) return rc;
  // cov_center: the train rows' column means under snp, 0 under gblup; a model whose covariate effects are
  // NaN (d = 0, collinear covariates) is NaN in every output
  finish_second(hb, fitness, cov_effects, n_cov, n_cov, n_cov, cp.m.data(), cov_center, intercept, center);
  return 0;
}

int tblup_fit_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                          int64_t n_levels, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                          int branch, double* fitness, double* ebv, double* cov_effects, double* cov_center,
                          double* group_effects, double* group_center, double* intercept, double* center,
                          double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  bool model;
  if (int rc = check_model_out(intercept, center, effects, model)) return rc;
  if (batch > 0 && (!group_effects || !group_center)) return fail(TBLUP_ERR_ARG, "null group_effects/group_center");
  if (batch > 0 && n_cov > 0 && (!cov_effects || !cov_center))
    return fail(TBLUP_ERR_ARG, "null cov_effects/cov_center");
  // Routes 0 / 1 through tblup_fit_cov_batch on the expanded design (the same bits as that entry gives); 2 through
  // k_fixed.
  const GroupCall a{c, split_id, cov, n_cov, group, n_levels, idx, offsets, batch, branch};
  return for_each_route(a, h2, [&](const Route& r) -> int {
    const int64_t Bs = r.Bs, Cw = r.Cw, nt = r.gs.nt;
    std::vector<double> fit((size_t)Bs), ev(ebv ? (size_t)Bs * nt * r.gs.nV : 0), bo((size_t)Bs * nt * Cw);
    RouteModel rm(r, model);
    double* evp = ebv ? ev.data() : nullptr;
    int rc;
    if (r.id == 2) {
      rc = fit_fixed_wide(r, h2, fit.data(), evp, bo.data(), rm.ip, rm.cp, rm.ep);
    } else {
      std::vector<double> xc((size_t)Bs * Cw);   // that entry's centres (cov_m, share)
      rc = tblup_fit_cov_batch(c, split_id, r.x.data(), Cw, r.idx(), r.off(), Bs, h2, branch, fit.data(), evp,
                               bo.data(), xc.data(), rm.ip, rm.cp, rm.ep);
    }
    if (rc) return rc;
    r.scatter(fit.data(), 1, fitness);
    r.scatter(evp, nt * r.gs.nV, ebv);
    r.put_fixed(bo.data(), fit.data(), cov_effects, group_effects, 1, cov_center, group_center);
    if (model) rm.scatter(r, intercept, center, effects);
    return 0;
  });
}

int tblup_snp_score_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* snps,
                              int64_t n_cand, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                              int branch, double* fitness, double* score, double* info, double* q,
                              double* cov_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (batch < 0 || n_cand < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_cand");
  std::vector<int32_t> s32;
  if (int rc = check_snps(c, snps, n_cand, s32)) return rc;
  if (batch == 0 || n_cand == 0) return 0;
  if (int rc = check_h2_open(h2)) return rc;
  if (!score || !info) return fail(TBLUP_ERR_ARG, "null score/info");
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, true)) return rc;
  fitness = hb.fitness_or_own(fitness);
  const int nt = hb.d.nt, nc = (int)n_cov;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, false);
  using Bufs = WithGls<ScoreBufs, CovGls>;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) {
    return Bufs{ScoreBufs::carve(cv, hb, B, n_cand), CovGls::carve(cv, hb, B, n_cov, true, 1, false)};
  };
  // per chunk, behind the pipeline: k_covar keeps the model's GLS step, k_snpscore's launches read it
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t b0 = ck.b0, B = ck.B;
    const Bufs bufs = carve(cv, B, ck.sum_k);
    const ScoreBufs& sb = bufs.o;
    const CovGls& kb = bufs.k;
    if (int rc = ws_check(c, cv)) return rc;
    HIPCHK(hipMemcpyAsync(sb.cand, s32.data(), (size_t)n_cand * 4, hipMemcpyHostToDevice, s));
    if (int rc = kb.upload(cp, s)) return rc;
    return factor_pass(hb, ck, cv, rq, fitness, nullptr, [&](const CholLaunch& cl) -> int {
      if (int rc = kb.enqueue(cl, 0, s)) return rc;
      const ScoreCov sc = kb.score();
      HIPCHK(launch_snpscore(cl, (const int32_t*)c->colsum_all.p, sb.cand, n_cand, sb.plan, sb.vscr, &sc, sb.sco,
                             sb.inf, sb.q, s));
      if (int rc = sb.copy_out(hb, ck, n_cand, score, info, q)) return rc;
      if (cov_effects)
        HIPCHK(hipMemcpyAsync(cov_effects + b0 * nt * nc, kb.b, (size_t)B * nt * nc * 8, hipMemcpyDeviceToHost, s));
      return 0;
    });
  });
}

int tblup_loglik_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                           const int64_t* offsets, int64_t batch, const double* h2, int64_t n_h2, int branch,
                           double* fitness, double* loglik, double* sigma2_g, double* cov_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_cov(c, cov, n_cov)) return rc;
  if (batch < 0 || n_h2 < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_h2");
  if (batch == 0 || n_h2 == 0) return 0;
  if (!h2 || !loglik) return fail(TBLUP_ERR_ARG, "null h2/loglik");
  if (int rc = check_h2_grid(h2, n_h2 * batch)) return rc;
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2[0], branch, true)) return rc;
  const int64_t nt = hb.d.nt;
  const CovPlanes cp = gather_cov(hb, cov, n_cov, false);
  // log|Q~_T^T Q~_T| does not depend on h2: once per call, one value per plane
  const double lqq[2] = {log_det_qq(cp.qT.data(), hb.d.nT, hb.d.nTp, n_cov),
                         log_det_qq(cp.qT.data() + (size_t)COVAR_W * hb.d.nTp, hb.d.nT, hb.d.nTp, n_cov)};
  using Bufs = WithGls<LogLikBufs, CovGls>;
  const auto carve = [&](Carve& cv, int64_t B, int64_t) {
    return Bufs{LogLikBufs::carve(cv, hb, B, n_h2), CovGls::carve(cv, hb, B, n_cov, true, n_h2, false)};
  };
  // tblup_loglik_batch's passes, each with k_covar (keep mode, no z*) between the pipeline and k_loglik
  return run_host_batch(hb, false, carve, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) -> int {
    const hipStream_t s = c->stream;
    const int64_t B = ck.B;
    const Bufs bufs = carve(cv, B, ck.sum_k);
    const LogLikBufs& lb = bufs.o;
    const CovGls& kb = bufs.k;
    if (int rc = ws_check(c, cv)) return rc;
    if (int rc = kb.upload(cp, s)) return rc;
    HIPCHK(hipMemcpyAsync(kb.lqq, lqq, sizeof(lqq), hipMemcpyHostToDevice, s));
    const auto per_pass = [&](const CholLaunch& cl, int64_t g) -> int {
      if (int rc = kb.enqueue(cl, g, s)) return rc;
      HIPCHK(launch_loglik(cl, kb.keep.ks, kb.lqq, kb.nc, lb.ll + g * B * nt, lb.s2 + g * B * nt, s));
      return 0;
    };
    return h2_grid(hb, ck, cv, rq, lb, h2, n_h2, per_pass, fitness, loglik, sigma2_g, cov_effects, kb.b, nt * n_cov);
  });
}

int tblup_snp_score_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                                int64_t n_levels, const int64_t* snps, int64_t n_cand, const int64_t* idx,
                                const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                                double* score, double* info, double* q, double* cov_effects, double* group_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  if (batch < 0 || n_cand < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_cand");
  std::vector<int32_t> s32;
  if (int rc = check_snps(c, snps, n_cand, s32)) return rc;
  if (batch == 0 || n_cand == 0) return 0;
  if (int rc = check_h2_open(h2)) return rc;
  if (!score || !info) return fail(TBLUP_ERR_ARG, "null score/info");
  const GroupCall a{c, split_id, cov, n_cov, group, n_levels, idx, offsets, batch, branch};
  return for_each_route(a, h2, [&](const Route& r) -> int {
    const int64_t Bs = r.Bs, Cw = r.Cw, nt = r.gs.nt;
    std::vector<double> fit((size_t)Bs), sco((size_t)Bs * nt * n_cand), inf((size_t)Bs * n_cand), qs((size_t)Bs * nt),
        bo((size_t)Bs * nt * Cw);
    int rc;
    if (r.id == 2) {
      rc = score_fixed_wide(r, s32, h2, fit.data(), sco.data(), inf.data(), qs.data(), bo.data());
    } else {
      rc = tblup_snp_score_cov_batch(c, split_id, r.x.data(), Cw, snps, n_cand, r.idx(), r.off(), Bs, h2, branch,
                                     fit.data(), sco.data(), inf.data(), qs.data(), bo.data());
    }
    if (rc) return rc;
    r.scatter(fit.data(), 1, fitness);
    r.scatter(sco.data(), nt * n_cand, score);
    r.scatter(inf.data(), n_cand, info);
    r.scatter(qs.data(), nt, q);
    r.put_fixed(bo.data(), fit.data(), cov_effects, group_effects);
    return 0;
  });
}

int tblup_loglik_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                             int64_t n_levels, const int64_t* idx, const int64_t* offsets, int64_t batch,
                             const double* h2, int64_t n_h2, int branch, double* fitness, double* loglik,
                             double* sigma2_g, double* cov_effects, double* group_effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (int rc = check_group(c, cov, n_cov, group, n_levels)) return rc;
  if (batch < 0 || n_h2 < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_h2");
  if (batch == 0 || n_h2 == 0) return 0;
  if (!h2 || !loglik) return fail(TBLUP_ERR_ARG, "null h2/loglik");
  if (int rc = check_h2_grid(h2, n_h2 * batch)) return rc;
  const GroupCall a{c, split_id, cov, n_cov, group, n_levels, idx, offsets, batch, branch};
  return for_each_route(a, h2[0], [&](const Route& r) -> int {
    const int64_t Bs = r.Bs, Cw = r.Cw, nt = r.gs.nt;
    // the route's h2 columns; its results [n_h2][Bs][..]
    std::vector<double> hs((size_t)n_h2 * Bs), fit(hs.size()), ll(hs.size() * nt), s2(ll.size()), bo(ll.size() * Cw);
    for (int64_t g = 0; g < n_h2; ++g)
      for (int64_t i = 0; i < Bs; ++i) hs[g * Bs + i] = h2[g * batch + r.mb[i]];
    int rc;
    if (r.id == 2) {
      rc = loglik_fixed_wide(r, hs.data(), n_h2, fit.data(), ll.data(), s2.data(), bo.data());
    } else {
      rc = tblup_loglik_cov_batch(c, split_id, r.x.data(), Cw, r.idx(), r.off(), Bs, hs.data(), n_h2, branch,
                                  fit.data(), ll.data(), s2.data(), bo.data());
    }
    if (rc) return rc;
    r.scatter(fit.data(), 1, fitness, n_h2);
    r.scatter(ll.data(), nt, loglik, n_h2);
    r.scatter(s2.data(), nt, sigma2_g, n_h2);
    r.put_fixed(bo.data(), fit.data(), cov_effects, group_effects, n_h2);
    return 0;
  });
}

int tblup_reliability_group_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* group,
                                  int64_t n_levels, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                                  const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                                  double* cov_effects, double* cov_center, double* group_effects, double* group_center,
                                  double* intercept, double* center, double* effects, double* reliability,
                                  double* pev_total, double* fixed_cov) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
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
  std::vector<int32_t> a32;
  if (int rc = check_animals(c, animals, n_pred, a32)) return rc;
  // the second solve (the model of the adjusted phenotype and its fitness) runs only for a caller who wants it
  const bool full = model || fitness;
  if (batch == 0 || (n_pred == 0 && !full && !fixed_cov)) return 0;
  if (n_pred > 0 && !reliability) return fail(TBLUP_ERR_ARG, "null reliability");
  const int64_t nc = n_cov, Co = nc + n_levels;
  const double nan = std::nan("");
  const GroupCall a{c, split_id, cov, n_cov, group, n_levels, idx, offsets, batch, branch};
  return for_each_route(a, h2, [&](const Route& r) -> int {
    const int64_t Bs = r.Bs, Cw = r.Cw, nt = r.gs.nt, Cm = r.cols[r.id == 2 ? 0 : r.id];
    // A route that is the whole batch (its models are then in batch order) writes the per-animal outputs, and the
    // wide route fixed_cov, straight into the caller's arrays: at 128 columns fixed_cov is 128 KiB a model.  Else the
    // route's own: fixed_cov compact [Cm][Cm] from the covariate entry, in the caller's layout from k_fixed_cov.
    const bool whole = Bs == batch, fc_own = fixed_cov && !(whole && r.id == 2);
    const size_t fc_model = (size_t)(r.id == 2 ? Co * Co : Cm * Cm);
    // (the fitness also tells post_model of a model without a fixed column)
    std::vector<double> fit(full ? (size_t)Bs : 0), rel(whole ? 0 : (size_t)Bs * n_pred),
        pev(pev_total && !whole ? (size_t)Bs * n_pred : 0), fc(fc_own ? (size_t)Bs * fc_model : 0),
        bo(model ? (size_t)Bs * nt * Cw : 0), xc(model ? (size_t)Bs * Cw : 0);
    RouteModel rm(r, model);
    const auto opt = [](std::vector<double>& v, bool on) { return on ? v.data() : nullptr; };
    double *fp = opt(fit, full), *bp = opt(bo, model), *rp = whole ? reliability : rel.data();
    double *pp = whole ? pev_total : opt(pev, pev_total), *cp = fc_own ? fc.data() : fixed_cov;
    int rc;
    if (r.id == 2) {
      rc = reliab_fixed_wide(r, a32, animals, h2, full, fp, rp, pp, cp, bp, rm.ip, rm.cp, rm.ep);
    } else {
      rc = tblup_reliability_cov_batch(c, split_id, r.x.data(), Cw, animals, n_pred, r.idx(), r.off(), Bs, h2, branch,
                                       fp, bp, opt(xc, model), rm.ip, rm.cp, rm.ep, rp, pp, cp);
    }
    if (rc) return rc;
    if (fitness) r.scatter(fp, 1, fitness);
    if (!whole) r.scatter(rp, n_pred, reliability);
    if (!whole) r.scatter(pp, n_pred, pev_total);
    // an animal whose label no train animal has: no design row, so no predicted record (PanelModel.predict's rule)
    for (int64_t i = 0; pev_total && i < Bs; ++i)
      for (int64_t v = 0; v < n_pred; ++v)
        if (group[animals[v]] < 0) pev_total[r.mb[i] * n_pred + v] = nan;
    if (fc_own && r.id == 2) r.scatter(cp, Co * Co, fixed_cov);
    for (int64_t i = 0; fc_own && r.id != 2 && i < Bs; ++i) {
      // the compact G^-1 of the expanded design at the caller's columns: level l is column nc + l - br, and the
      // reference level of an snp model keeps its zeros (NaN throughout for a model that is NaN)
      const int br = r.br[i];
      const double* in = cp + i * Cm * Cm;
      double* out = fixed_cov + r.mb[i] * Co * Co;
      const bool dead = std::isnan(in[0]);
      for (int64_t oi = 0; oi < Co; ++oi)
        for (int64_t oj = 0; oj < Co; ++oj) {
          const int64_t mi = oi < nc ? oi : oi - br, mj = oj < nc ? oj : oj - br;
          const bool ref = br == 1 && (oi == nc || oj == nc);
          out[oi * Co + oj] = dead ? nan : (ref ? 0.0 : in[mi * Cm + mj]);
        }
    }
    if (!model) return 0;
    r.put_fixed(bp, fp, cov_effects, group_effects, 1, cov_center, group_center);
    rm.scatter(r, intercept, center, effects);
    return 0;
  });
}

int tblup_predict_batch(tblup_ctx* c, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, const double* intercept, const double* center,
                        const double* effects, int64_t n_traits, double* ebv) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_panel(c)) return rc;
  if (n_traits < 1 || n_traits > MAXT) return fail(TBLUP_ERR_ARG, "need 1 <= n_traits <= 4");
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  if (batch == 0 || n_pred == 0) return 0;
  if (!animals || !idx || !offsets || !intercept || !center || !effects || !ebv)
    return fail(TBLUP_ERR_ARG, "null predict arguments");
  if (offsets[0] != 0) return fail(TBLUP_ERR_ARG, "offsets[0] must be 0");
  if (int rc = check_counts(offsets, batch, "model")) return rc;
  const int64_t total = offsets[batch];
  if (int rc = check_indices(c, idx, total)) return rc;
  std::vector<int32_t> a32;
  if (int rc = check_animals(c, animals, n_pred, a32)) return rc;
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
