// Profile (restricted) log-likelihood of every model of a chunk, from what the chunk's pipeline left in
// the workspace: the factor's pivots (the diagonals of Dinv = L_JJ^{-1}), z = L^{-1} rhs and the scalars.
//
// Model (the reference's own): beta ~ N(0, sigma2_g / d I), e ~ N(0, sigma2_e I), sigma2_e / sigma2_g =
// lambda; N = n_T, W_T = A_T - c, V = W_T W_T^T / d + lambda I, profiled over sigma2_g.
//   gblup (no mean fitted, r = 0):  q = y_T^T V^{-1} y_T
//   snp (intercept mean(y_T), train centre, V 1 = lambda 1, r = 1):  q = yc^T V^{-1} yc, yc = y_T - mean(y_T)
//   l = -1/2 [ (N - r)(log 2 pi + 1 + log(q / (N - r))) + log|V| - r log lambda ],  sigma2_g = q / (N - r)
// What is read, per form (M the factorised system, log|M| = -2 sum over the real rows of log Dinv_ii):
//   kernel form (M = V, rhs = y_T - mu):                    log|V| = log|M|,  q = |z|^2
//   SNP form (M = W_T^T W_T / d + lambda I_k, rhs = W_T^T yc / d), by Sylvester and Woodbury:
//                                   log|V| = (N - k) log lambda + log|M|,  q = (yc^T yc - d |z|^2) / lambda
// One workgroup per system; several traits share log|V|.  Every lane sums a fixed strided subset of the
// rows, the wave sum is a fixed-order xor butterfly, the waves' partials meet in LDS and are added in
// wave order: no atomics, so a system's bits do not depend on the batch around it.
//
// With fixed-effect covariates Q~ (ks non-null: what k_covar kept of the model's GLS step at the same h2), the
// restricted likelihood of the N - r - c error contrasts A^T y (A^T [1 Q~_T] = 0):
//   q_P = q - h_t^T b_t,  dof = N - r - c,  log|A^T V A| = log|V| - r log lambda + log|G| - log|Q~_T^T Q~_T|
//   l_R = -1/2 [ dof (log 2 pi + 1 + log(q_P / dof)) + log|A^T V A| ],  sigma2_g = q_P / dof
// log|Q~_T^T Q~_T| does not depend on h2: the host's, one value per branch (lqq; NaN: not of full rank).
// c is a count per branch (nc_gblup, nc_snp): the covariate entries pass the same count twice, the wide design
// [Q, Z] of tblup_loglik_group_batch has one column less under snp (launch_loglik_fixed).
#include "tblup_internal.h"

namespace tblup {

constexpr int LL_THREADS = 256;
constexpr int LL_WAVES = LL_THREADS / 64;
constexpr int LL_SUMS = 1 + 2 * MAXT;   // sum log Dinv_ii, |z_t|^2, yc_t^T yc_t

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(LL_THREADS) void k_loglik(CholLaunch c, const double* __restrict__ ks,
                                                       const double* __restrict__ lqq, int nc_gblup, int nc_snp,
                                                       double* __restrict__ loglik, double* __restrict__ sigma2) {
  __shared__ double part[LL_WAVES][LL_SUMS];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t ns = c.sd.ns, nT = c.d.nT, nTp = c.d.nTp;
  const int nt = c.d.nt;
  const double* sc = c.scal + b * SCAL;
  const int64_t pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const bool primal = c.sd.form == FORM_PRIMAL;
  const double* Db = c.Dinv + b * (int64_t)c.sd.NT * NPACK * BLKD;
  const double* zb = c.z + b * nt * ns;
  double acc[LL_SUMS];
#pragma unroll
  for (int e = 0; e < LL_SUMS; ++e) acc[e] = 0.0;
  // system rows: the pivot 1 / L_rr is element (r % 16, r % 16) of diagonal block r / 16 of tile r / 128
  for (int64_t r = t; r < ns; r += LL_THREADS) {
    if (!sys_real(r, pad, nrow)) continue;   // identity padding
    const int i = (int)(r % TILE), qb = i / NB, ii = i % NB;
    acc[0] += log(Db[(r / TILE) * (int64_t)NPACK * BLKD + pk(qb, qb) + bo(ii, ii)]);
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr)
      if (tr < nt) {
        const double zv = zb[tr * ns + r];
        acc[1 + tr] = __builtin_fma(zv, zv, acc[1 + tr]);
      }
  }
  if (primal) {
    // yc^T yc over the train rows of the system's split
    const int fo = fold_of(c.ft, b);
    const double* yT = c.ft.yT[fo];
    const double* ymu = c.ft.ymu[fo];
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr)
      if (tr < nt) {
        const double mu = ymu[tr];
        for (int64_t r = t; r < nT; r += LL_THREADS) {
          const double yc = yT[tr * nTp + r] - mu;
          acc[1 + MAXT + tr] = __builtin_fma(yc, yc, acc[1 + MAXT + tr]);
        }
      }
  }
#pragma unroll
  for (int e = 0; e < LL_SUMS; ++e) {
    const double v = wave_sum(acc[e]);
    if ((t & 63) == 0) part[t >> 6][e] = v;
  }
  __syncthreads();
  if (t >= nt) return;
  double slog = 0.0, zz = 0.0, yy = 0.0;
  for (int w = 0; w < LL_WAVES; ++w) {
    slog += part[w][0];
    zz += part[w][1 + t];
    yy += part[w][1 + MAXT + t];
  }
  const double lam = sc[SC_LAM], d = sc[SC_D], r = sc[SC_MUF];
  const double N = (double)nT;
  double df = N - r;
  const double loglam = log(lam);
  const double logM = -2.0 * slog;
  const double logV = primal ? (N - (double)nrow) * loglam + logM : logM;
  double q = primal ? (yy - d * zz) / lam : zz;
  double ldg = 0.0;   // log|G| - log|Q~_T^T Q~_T|
  bool ok = d > 0.0 && sc[SC_BAD] == 0.0;
  if (ks) {
    const double* kb = ks + b * COVAR_KS;
    const bool gblup = (int)sc[SC_MODE] == 1;
    const double lq = lqq[gblup ? 0 : 1];
    df = df - (double)(gblup ? nc_gblup : nc_snp);
    q = q - kb[KS_HB + t];
    ldg = kb[KS_LOGG] - lq;
    ok = ok && kb[KS_BAD] == 0.0 && lq == lq;
  }
  ok = ok && q > 0.0 && q < __builtin_inf() && df > 0.0;
  const double two_pi = 6.283185307179586476925286766559;
  double m2l = df * (log(two_pi) + 1.0 + log(q / df)) + logV - r * loglam;
  if (ks) m2l = m2l + ldg;
  const double l = -0.5 * m2l;
  const double nan = __builtin_nan("");
  loglik[b * nt + t] = ok && l == l ? l : nan;
  sigma2[b * nt + t] = ok ? q / df : nan;
}

hipError_t launch_loglik(const CholLaunch& c, const double* ks, const double* lqq, int n_cov, double* loglik,
                         double* sigma2, hipStream_t s) {
  if (c.d.nt < 1 || c.d.nt > MAXT) return hipErrorInvalidValue;
  if (ks && (!lqq || n_cov < 1 || n_cov > COVAR_W)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_loglik, dim3((unsigned)c.B), dim3(LL_THREADS), 0, s, c, ks, lqq, n_cov, n_cov, loglik, sigma2);
  return hipGetLastError();
}

hipError_t launch_loglik_fixed(const CholLaunch& c, const double* ks, const double* lqq, const int (&cols)[2],
                               double* loglik, double* sigma2, hipStream_t s) {
  if (c.d.nt < 1 || c.d.nt > MAXT || !ks || !lqq) return hipErrorInvalidValue;
  for (int n : cols)
    if (n < 0 || n > FIXED_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_loglik, dim3((unsigned)c.B), dim3(LL_THREADS), 0, s, c, ks, lqq, cols[0], cols[1], loglik,
                     sigma2);
  return hipGetLastError();
}

}  // namespace tblup
