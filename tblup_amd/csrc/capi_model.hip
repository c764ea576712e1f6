// C ABI of libtblup_gpu.so, taking the fitted model out (include/tblup_gpu.h): tblup_fit_batch
// (the evaluation's chunks plus one k_effects launch each), tblup_predict_batch (k_predict),
// tblup_loglik_batch (the chunks once per h2 row plus one k_loglik launch each),
// tblup_snp_score_batch (the chunks plus k_snpscore's launches each) and tblup_fit_cov_batch (the chunks plus
// k_covar, a second solve, k_cov_fitness and k_effects each).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "capi_ctx.h"

using namespace tblup;
using namespace tblup_capi;

extern "C" {

int tblup_fit_batch(tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch, double h2,
                    int branch, double* fitness, double* intercept, double* center, double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (batch > 0 && (!intercept || !center || !effects)) return fail(TBLUP_ERR_ARG, "null intercept/center/effects");
  std::vector<double> fit_local;
  if (!fitness && batch > 0) {
    fit_local.resize((size_t)batch);
    fitness = fit_local.data();
  }
  const FitOut fo{intercept, center, effects};
  return eval_batch_host(c, split_id, idx, offsets, batch, h2, branch, fitness, nullptr, &fo);
}

int tblup_fit_cov_batch(tblup_ctx* c, int split_id, const double* cov, int64_t n_cov, const int64_t* idx,
                        const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness, double* ebv,
                        double* cov_effects, double* cov_center, double* intercept, double* center, double* effects) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (n_cov < 1 || n_cov > COVAR_W) return fail(TBLUP_ERR_ARG, "need 1 <= n_cov <= 16");
  if (!cov) return fail(TBLUP_ERR_ARG, "null cov");
  for (int64_t i = 0; i < c->n * n_cov; ++i)
    if (!std::isfinite(cov[i])) return fail(TBLUP_ERR_ARG, "covariates must be finite");
  const bool any = intercept || center || effects;
  if (any && !(intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "intercept/center/effects are given together or not at all");
  if (batch > 0 && (!cov_effects || !cov_center)) return fail(TBLUP_ERR_ARG, "null cov_effects/cov_center");
  std::vector<double> fit_local;
  if (!fitness && batch > 0) {
    fit_local.resize((size_t)batch);
    fitness = fit_local.data();
  }
  const FitOut fo{intercept, center, effects};
  const CovOut co{cov, n_cov, cov_effects, cov_center};
  return eval_batch_host(c, split_id, idx, offsets, batch, h2, branch, fitness, ebv, any ? &fo : nullptr, nullptr,
                         nullptr, nullptr, &co);
}

int tblup_reliability_batch(tblup_ctx* c, int split_id, const int64_t* animals, int64_t n_pred, const int64_t* idx,
                            const int64_t* offsets, int64_t batch, double h2, int branch, double* fitness,
                            double* intercept, double* center, double* effects, double* reliability) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (batch < 0 || n_pred < 0) return fail(TBLUP_ERR_ARG, "negative batch / n_pred");
  const bool any = intercept || center || effects;
  if (any && !(intercept && center && effects))
    return fail(TBLUP_ERR_ARG, "intercept/center/effects are given together or not at all");
  if (n_pred > 0 && !animals) return fail(TBLUP_ERR_ARG, "null animals");
  std::vector<int32_t> a32((size_t)n_pred);
  for (int64_t i = 0; i < n_pred; ++i) {
    if (animals[i] < 0 || animals[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    a32[i] = (int32_t)animals[i];
  }
  if (batch == 0 || n_pred == 0) return 0;
  if (!reliability) return fail(TBLUP_ERR_ARG, "null reliability");
  std::vector<double> fit_local;
  if (!fitness) {
    fit_local.resize((size_t)batch);
    fitness = fit_local.data();
  }
  const FitOut fo{intercept, center, effects};
  const RelOut ro{a32.data(), n_pred, reliability};
  return eval_batch_host(c, split_id, idx, offsets, batch, h2, branch, fitness, nullptr, any ? &fo : nullptr, &ro);
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
  const LogLikOut lo{h2, n_h2, loglik, sigma2_g};
  return eval_batch_host(c, split_id, idx, offsets, batch, h2[0], branch, fitness, nullptr, nullptr, nullptr, &lo);
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
  std::vector<double> fit_local;
  if (!fitness) {
    fit_local.resize((size_t)batch);
    fitness = fit_local.data();
  }
  const ScoreOut so{s32.data(), n_cand, score, info, q};
  return eval_batch_host(c, split_id, idx, offsets, batch, h2, branch, fitness, nullptr, nullptr, nullptr, nullptr, &so);
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
  // device bytes of models [b0, b1) (every buffer rounded up to 256 B)
  const ChunkBytes bytes_of = [&](const int64_t*, int64_t B, int64_t sum_k) {
    size_t s = 0;
    auto add = [&](size_t x) { s = (size_t)round_up((int64_t)(s + x), 256); };
    add((size_t)n_pred * 4);
    add((size_t)sum_k * 8);
    add((size_t)(B + 1) * 8);
    add((size_t)B * nt * 8);
    add((size_t)sum_k * 8);
    add((size_t)nt * sum_k * 8);
    add((size_t)B * nt * n_pred * 8);
    return s + 256;
  };
  // models per chunk: within the workspace budget (TBLUP_WORKSPACE_MB) and one launch's grid,
  // B * nblk <= 0x7fffffff
  const int64_t nblk = (n_pred + 255) / 256;
  return for_each_chunk(c, offsets, batch, 0x7fffffff / nblk, bytes_of, [&](const Chunk& ck) -> int {
    const int64_t b0 = ck.b0, B = ck.B, sum_k = ck.sum_k;
    Carve cv{(char*)c->ws.p};
    int32_t* d_an = cv.take<int32_t>((size_t)n_pred);
    int64_t *d_idx, *d_off;
    if (int rc = upload_chunk(c, cv, idx, offsets, ck, &d_idx, &d_off)) return rc;
    double* d_int = cv.take<double>((size_t)B * nt);
    double* d_cen = cv.take<double>((size_t)sum_k);
    double* d_eff = cv.take<double>((size_t)nt * sum_k);
    double* d_ebv = cv.take<double>((size_t)B * nt * n_pred);
    if (ws_check(c, cv)) return fail(TBLUP_ERR_STATE, "internal error: predict buffers overrun the workspace");
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(d_an, a32.data(), (size_t)n_pred * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_int, intercept + b0 * nt, (size_t)B * nt * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_cen, center + offsets[b0], (size_t)sum_k * 8, hipMemcpyHostToDevice, s));
    for (int t = 0; t < nt; ++t)
      HIPCHK(hipMemcpyAsync(d_eff + (int64_t)t * sum_k, effects + (int64_t)t * total + offsets[b0], (size_t)sum_k * 8,
                            hipMemcpyHostToDevice, s));
    HIPCHK(launch_predict((const int8_t*)c->geno_sm.p, c->n, c->P, d_an, n_pred, d_idx, d_off, B, d_int, d_cen, d_eff,
                          sum_k, nt, d_ebv, s));
    HIPCHK(hipMemcpyAsync(ebv + b0 * nt * n_pred, d_ebv, (size_t)B * nt * n_pred * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // the chunk's offsets and the host buffers are borrowed until here
    return 0;
  });
}

}  // extern "C"
