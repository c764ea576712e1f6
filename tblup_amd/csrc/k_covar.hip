// Fixed-effect covariates in the fitted model (tblup_fit_cov_batch): the GLS estimate of their effects and
// the phenotype adjusted for them, from the Cholesky factor M = L L^T, the inverted diagonal tiles
// X_J = L_JJ^{-1} and z = L^{-1} rhs that the chunk's pipeline left in the workspace (what k_snpscore reads;
// neither solve kernel writes them).  With Q~ = Q - 1 m^T the n x c covariates (c <= COVAR_W = 16) centred
// by the branch's rule (snp: m the column means over the train rows; gblup: m = 0 -- a column of ones
// fits the mean), V = W_T W_T^T / d + lambda I and r_t = y_T,t - mu_t as k_snpscore has them,
//   b_t = (Q~_T^T V^{-1} Q~_T)^{-1} Q~_T^T V^{-1} r_t = G^{-1} h_t,      y*_t = y_t - Q~ b_t,
// and the genomic model is the branch's own model of y*.  With S = L^{-1} R:
//   kernel form (M = V, rhs = r):   R = Q~_T;          G = S^T S,  h_t = S^T z_t,  z*_t = z_t - S b_t
//   SNP form (M = W_T^T W_T / d + lambda I_k, rhs = W_T^T r / d; snp batches only, choose_sys):
//     R = g = W_T^T Q~_T = A_T^T Q~_T (Q~_T sums to zero over the train rows),
//     G = (Q~_T^T Q~_T - S^T S / d) / lambda,  h_t = (Q~_T^T r_t - S^T z_t) / lambda,  z*_t = z_t - S b_t / d
// z* = L^{-1} rhs(y*) goes to a buffer of its own; the second pass of k_solve and k_effects on it give the
// EBVs and the effects of y*'s model.  It is k_snpscore with dense columns in place of SNP columns.
//
// k_covar: one 512-thread workgroup per model (no flags, no atomics, every loop bounded by the system's shape).
//   phase 1: R [ns][16] into V (columns past c and padding rows zero), from the call's centred covariates of
//     the train rows in split order (qT: plane 0 uncentred for gblup models, plane 1 centred for snp
//     models; zero at padding rows and columns).  SNP form: g_ij one fma chain per (system row i,
//     covariate j) over the train animals in order, the genotypes unpacked from the split's 2-bit packed
//     row of SNP i on the way -- a thread per (row, 8 covariates), a wave's covariate values uniform; and
//     Q~_T^T Q~_T, Q~_T^T r_t: one chain over the train rows in order per entry.
//   phase 2 (fwd_subst.h): the blocked forward substitution of k_reliab / k_snpscore, unchanged, in place.
//   phase 3: S^T S (thread (i, j, half): the real rows of its parity in order) and S^T z_t (thread
//     (j, t, wave): rows wave, wave + 8, ..); the partial sums meet in LDS and are added in a fixed order.
//   phase 4: wave 0 -- lane (t, i) holds row i of G -- factors G = C C^T (right-looking, the pivots
//     and columns passed by lane shuffles), solves for b_t and writes it.  A pivot that is not positive and
//     finite (collinear covariates; a column constant over the train rows under snp), d = 0 or a flagged index:
//     NaN for b and for z*, so for everything the model's second pass produces.  Positive means above
//     COVAR_PIV_RTOL of the pivot's own diagonal entry of G: the pivot of a column that repeats another is
//     rounding noise of either sign, some 1e-16 of that entry.
//   phase 5: z* for every trait by all threads; the pipeline's z is left as it is.  Skipped when z2 is null.
// Keep mode (CovKeep non-null, the entries that adjust the score statistics and the likelihood for the
// covariates): what phases 2 - 4 compute stays in the workspace -- S [ns][16] (copied out of LDS when V
// lives there; else V is that buffer), C (row-major, identity past c), C^{-1} h_t per trait, and per model
// {log|G| = 2 sum log C_ii, the bad flag, h_t^T b_t = |C^{-1} h_t|^2 per trait}.  b and z* are the same bits
// with or without it.
// So a model's bits are a function of the model, the covariates and the system alone: not of the batch, the
// chunking or where V lives (LDS when ns x 16 doubles fit, SlabPlan::lds; else a workspace slice of its own).
//
// k_cov_fitness: one 512-thread workgroup per model; y*_V = y_V - Q~_V b_t (one chain over the covariates in
// order) and the mean over traits of |pearson(ebv_V, y*_V)| through the solve kernels' own restatement
// (pearson_dev.h), from the second solve's EBVs.
#include <algorithm>

#include "fwd_subst.h"
#include "pearson_dev.h"

namespace tblup {

namespace {

constexpr int CTHR = FWD_TH;
constexpr int CW = COVAR_W;
constexpr int CHALF = CW / 2;   // covariates per thread in the SNP form's count products
static_assert(COVAR_W == FWD_W, "the covariates are one slab of the substitution's 16 right-hand sides");
static_assert(COVAR_W * MAXT == 64, "phase 4: one wave, one lane per (trait, covariate)");
static_assert(CTHR == 2 * CW * CW, "phase 3: two threads per entry of S^T S");

template <int FORM, bool VLDS, bool KEEP>
__global__ __launch_bounds__(CTHR) void k_covar(CholLaunch c, const double* __restrict__ qT, int nc,
                                                double* __restrict__ vscr, double* __restrict__ bhat,
                                                double* __restrict__ z2, CovKeep keep) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  __shared__ double pss[2][CW * CW];          // S^T S partial sums by row parity
  __shared__ double psz[CTHR / 64][64];       // S^T z_t partial sums by wave: [wave][16 t + j]
  __shared__ double qq_s[CW * CW];            // SNP form: Q~_T^T Q~_T
  __shared__ double qr_s[MAXT * CW];          // SNP form: Q~_T^T r_t
  __shared__ double b_s[MAXT][CW];
  __shared__ int bad_s;
  constexpr int W = CW;
  const int t = threadIdx.x, l = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6), lc = l & 15, lg = l >> 4;
  const int64_t b = blockIdx.x;
  const int64_t ns = c.sd.ns, nT = c.d.nT, nTp = c.d.nTp;
  const int NT = c.sd.NT, nt = c.d.nt;
  double* V;
  if constexpr (VLDS) V = dyn;
  else V = vscr + b * ns * W;
  const double* sc = c.scal + b * SCAL;
  const double lam = sc[SC_LAM], dd = sc[SC_D];
  const int64_t pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const bool gblup = (int)sc[SC_MODE] == 1;
  const int fo = fold_of(c.ft, b);
  const double* qt = qT + (gblup ? 0 : (int64_t)W * nTp);   // the model's plane [16][nTp]
  // block rows that hold real system rows (the rest is identity padding with zero right-hand sides)
  const int J0 = (int)(pad / TILE), J1 = (int)((pad + nrow + TILE - 1) / TILE);

  if constexpr (FORM == FORM_DUAL) {
    // rows = the train animals in split order
    for (int64_t i = t; i < ns * W; i += CTHR) {
      const int64_t r = i / W;
      V[i] = r < nrow ? qt[(i % W) * nTp + r] : 0.0;
    }
  } else {
    // g: work item (half h of the covariates, row) -- a wave's 64 items share h, so its covariate values
    // are uniform; a padding row reads the zero row P
    const int64_t o0 = c.off[b], P = c.d.P;
    const uint8_t* gp = c.ft.gpk[fo];
    const int64_t r0 = (int64_t)J0 * TILE, nspan = (int64_t)(J1 - J0) * TILE;
    for (int64_t w0 = 64 * q; w0 < 2 * nspan; w0 += CTHR) {
      const int h = (int)(w0 / nspan);
      const int64_t row = r0 + w0 % nspan + l;
      const bool real = sys_real(row, pad, nrow);
      double acc[CHALF];
#pragma unroll
      for (int j = 0; j < CHALF; ++j) acc[j] = 0.0;
      if (CHALF * h < nc) {
        const int64_t col = real ? snp_col(c.idx[o0 + row - pad], P) : P;
        const uint32_t* xr = reinterpret_cast<const uint32_t*>(gp + col * c.gpk_row);   // 16 animals per dword
        const double* qh = qt + (int64_t)CHALF * h * nTp;
        for (int64_t g = 0; g < nTp / 16; ++g) {
          const uint32_t x = xr[g];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const double xv = (double)((x >> (2 * e)) & 3u);
#pragma unroll
            for (int j = 0; j < CHALF; ++j) acc[j] = __builtin_fma(xv, qh[(int64_t)j * nTp + 16 * g + e], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < CHALF; ++j) V[row * W + CHALF * h + j] = real ? acc[j] : 0.0;
    }
    // Q~_T^T Q~_T and Q~_T^T r_t: one chain over the train rows in order per entry
    if (t < W * W) {
      const double* qi = qt + (int64_t)(t >> 4) * nTp;
      const double* qj = qt + (int64_t)(t & 15) * nTp;
      double acc = 0.0;
#pragma unroll 8
      for (int64_t r = 0; r < nT; ++r) acc = __builtin_fma(qi[r], qj[r], acc);
      qq_s[t] = acc;
    } else if (t < W * W + MAXT * W) {
      const int tr = (t - W * W) >> 4, j = t & 15;
      double acc = 0.0;
      if (tr < nt) {
        const double* y = c.ft.yT[fo] + (int64_t)tr * nTp;
        const double mu = c.ft.ymu[fo][tr];
        const double* qj = qt + (int64_t)j * nTp;
#pragma unroll 8
        for (int64_t r = 0; r < nT; ++r) acc = __builtin_fma(qj[r], y[r] - mu, acc);
      }
      qr_s[t - W * W] = acc;
    }
  }
  __syncthreads();

  // phase 2: V_J = X_J (R_J - sum_{L<J} L_JL V_L)
  const double* Lb = c.L + b * l_stride(NT);
  const double* Db = c.Dinv + b * (int64_t)NT * NPACK * BLKD;
  const double* zb = c.z + b * nt * ns;
  fwd_subst16(Lb, Db, V, NT, J0, J1, pad, q, lc, lg, [](int, double) {});

  if constexpr (VLDS && KEEP) {
    {
      double* sq = keep.sq + b * ns * W;
      for (int64_t i = t; i < ns * W; i += CTHR) sq[i] = V[i];
    }
  }

  // phase 3: S^T S and S^T z_t over the real rows
  {
    const int i = (t >> 4) & 15, j = t & 15, hp = t >> 8;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t r = pad + hp; r < pad + nrow; r += 2) acc = __builtin_fma(V[r * W + i], V[r * W + j], acc);
    pss[hp][t & 255] = acc;
    const int tr = (l >> 4);
    double za = 0.0;
    if (tr < nt) {
#pragma unroll 4
      for (int64_t r = pad + q; r < pad + nrow; r += CTHR / 64) za = __builtin_fma(V[r * W + j], zb[(int64_t)tr * ns + r], za);
    }
    psz[q][l] = za;
  }
  __syncthreads();

  // phase 4: wave 0, lane (trait lg, covariate lc): row lc of G in registers
  const bool dead = !(dd > 0.0) || sc[SC_BAD] != 0.0;
  const double nan = __builtin_nan("");
  if (t < 64) {
    const int i = lc, tr = lg;
    double g[W], col[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double ss = pss[0][i * W + j] + pss[1][i * W + j];
      double v;
      if constexpr (FORM == FORM_PRIMAL) v = (qq_s[i * W + j] - ss / dd) / lam;
      else v = ss;
      g[j] = (i < nc && j < nc) ? v : (i == j ? 1.0 : 0.0);   // columns past c: kept out of G
      col[j] = 0.0;
    }
    double sz = 0.0;
    for (int w = 0; w < CTHR / 64; ++w) sz += psz[w][l];
    double h;
    if constexpr (FORM == FORM_PRIMAL) h = (qr_s[l] - sz) / lam;
    else h = sz;
    if (i >= nc || tr >= nt) h = 0.0;
    double gii = 0.0;   // this lane's diagonal entry of G
#pragma unroll
    for (int j = 0; j < W; ++j) gii = (j == i) ? g[j] : gii;
    // G = C C^T, right-looking: after step k, g[k] of lane i >= k is C[i][k]; lane k keeps column k of C
    bool ok = true;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double pkk = __shfl(g[k], k, W);
      ok = ok && pkk > COVAR_PIV_RTOL * __shfl(gii, k, W) && pkk < __builtin_inf();
      const double ckk = sqrt(pkk);
      const double cik = (i == k) ? ckk : g[k] / ckk;
      g[k] = cik;
#pragma unroll
      for (int j = k + 1; j < W; ++j) {
        const double cjk = __shfl(cik, j, W);
        g[j] = __builtin_fma(-cik, cjk, g[j]);
        if (i == k) col[j] = cjk;
      }
    }
    // C y = h, then C^T b = y
    double rhs = h, y = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double yk = __shfl(rhs / g[k], k, W);
      if (i == k) y = yk;
      rhs = __builtin_fma(-g[k], yk, rhs);
    }
    const double ych = y;   // (C^{-1} h_t)_i
    double bsol = 0.0;
#pragma unroll
    for (int k = W - 1; k >= 0; --k) {
      const double bk = __shfl(y / g[k], k, W);
      if (i == k) bsol = bk;
      y = __builtin_fma(-col[k], bk, y);
    }
    const bool bad = dead || !ok;
    const double bv = bad ? nan : (i < nc ? bsol : 0.0);
    b_s[tr][i] = bv;
    if (tr < nt && i < nc) bhat[(b * nt + tr) * nc + i] = bv;
    if (t == 0) bad_s = bad ? 1 : 0;
    if constexpr (KEEP) {
      // h_t^T b_t = |C^{-1} h_t|^2: one chain over the covariates in order
      double hb = 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double yk = __shfl(ych, k, W);
        hb = __builtin_fma(yk, yk, hb);
      }
      // sum log C_kk (C_kk = 1 past c): every lane the log of its own diagonal entry, added in order
      double cii = 1.0;
#pragma unroll
      for (int k = 0; k < W; ++k) cii = (k == i) ? g[k] : cii;
      const double lci = log(cii);
      double slog = 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) slog += __shfl(lci, k, W);
      if (tr == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) keep.cf[(b * W + i) * W + k] = k <= i ? g[k] : 0.0;
      }
      keep.ch[(b * MAXT + tr) * W + i] = ych;
      double* ks = keep.ks + b * COVAR_KS;
      if (i == 0) ks[KS_HB + tr] = hb;
      if (t == 0) {
        ks[KS_LOGG] = 2.0 * slog;
        ks[KS_BAD] = bad ? 1.0 : 0.0;
      }
    }
  }
  if constexpr (KEEP) {
    if (!z2) return;
  }
  __syncthreads();

  // phase 5: z* = z - S b (SNP form: / d) at the real rows, z elsewhere
  const bool bad = bad_s != 0;
  for (int64_t i = t; i < (int64_t)nt * ns; i += CTHR) {
    const int64_t tr = i / ns, r = i % ns;
    double zv = zb[i];
    if (sys_real(r, pad, nrow)) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < W; ++j) acc = __builtin_fma(V[r * W + j], b_s[tr][j], acc);
      if constexpr (FORM == FORM_PRIMAL) zv = zv - acc / dd;
      else zv = zv - acc;
      if (bad) zv = nan;
    }
    z2[b * nt * ns + i] = zv;
  }
}

__global__ __launch_bounds__(CTHR) void k_cov_fitness(CholLaunch c, const double* __restrict__ ebv,
                                                      const double* __restrict__ qV, const double* __restrict__ bhat,
                                                      int nc, double* __restrict__ fit) {
  extern __shared__ double ys[];   // y*_V of one trait
  __shared__ double red[4 * 16];
  __shared__ double b_s[MAXT][CW];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x, nV = c.d.nV;
  const int nt = c.d.nt;
  const double* sc = c.scal + b * SCAL;
  const int fo = fold_of(c.ft, b);
  const double* qv = qV + ((int)sc[SC_MODE] == 1 ? 0 : (int64_t)CW * nV);   // the model's plane [16][nV]
  if (t < MAXT * CW) {
    const int tr = t >> 4, j = t & 15;
    b_s[tr][j] = (tr < nt && j < nc) ? bhat[(b * nt + tr) * nc + j] : 0.0;
  }
  __syncthreads();
  double fsum = 0.0;
  for (int tr = 0; tr < nt; ++tr) {
    const double* yV = c.ft.yV[fo] + (int64_t)tr * nV;
    for (int64_t v = t; v < nV; v += CTHR) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < CW; ++j) acc = __builtin_fma(qv[(int64_t)j * nV + v], b_s[tr][j], acc);
      ys[v] = yV[v] - acc;
    }
    __syncthreads();
    fsum += pearson_abs<CTHR>(ebv + (b * nt + tr) * nV, ys, nV, red);
    __syncthreads();
  }
  if (t == 0) fit[b] = sc[SC_BAD] != 0.0 ? __builtin_nan("") : (nt == 1) ? fsum : fsum / (double)nt;
}

}  // namespace

hipError_t launch_covar(const CholLaunch& c, const double* qT, int n_cov, const SlabPlan& p, double* vscr,
                        double* bhat, double* z2, const CovKeep& keep, hipStream_t s) {
  if (c.B < 1) return hipSuccess;
  if (c.d.nt < 1 || c.d.nt > MAXT || n_cov < 1 || n_cov > COVAR_W || p.S != 1) return hipErrorInvalidValue;
  // keep mode: every buffer or none; without LDS the slices are S themselves
  const bool kp = keep.sq || keep.cf || keep.ch || keep.ks;
  if (kp && !(keep.sq && keep.cf && keep.ch && keep.ks && (p.lds || vscr == keep.sq))) return hipErrorInvalidValue;
  if (!kp && !z2) return hipErrorInvalidValue;
  using Kern = decltype(&k_covar<FORM_DUAL, false, false>);
  const Kern plain[4] = {k_covar<FORM_DUAL, false, false>, k_covar<FORM_DUAL, true, false>,
                         k_covar<FORM_PRIMAL, false, false>, k_covar<FORM_PRIMAL, true, false>};
  const Kern kept[4] = {k_covar<FORM_DUAL, false, true>, k_covar<FORM_DUAL, true, true>,
                        k_covar<FORM_PRIMAL, false, true>, k_covar<FORM_PRIMAL, true, true>};
  return launch_slabs(kp ? kept : plain, c, p, vscr, 1, [&](Kern k, dim3 grid, size_t shm, int64_t, int64_t) {
    hipLaunchKernelGGL(k, grid, dim3(CTHR), shm, s, c, qT, n_cov, vscr, bhat, z2, keep);
  });
}

hipError_t launch_cov_fitness(const CholLaunch& c, const double* ebv, const double* qV, const double* bhat, int n_cov,
                              double* fit, hipStream_t s) {
  if (c.B < 1) return hipSuccess;
  if (c.d.nt < 1 || c.d.nt > MAXT || n_cov < 1 || n_cov > COVAR_W) return hipErrorInvalidValue;
  const size_t shm = (size_t)c.d.nV * 8;
  if (shm > 150 * 1024) return hipErrorInvalidValue;   // (k_solve's own LDS bound on n_V is tighter)
  if (shm > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_cov_fitness, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cov_fitness, dim3((unsigned)c.B), dim3(CTHR), shm, s, c, ebv, qV, bhat, n_cov, fit);
  return hipGetLastError();
}

}  // namespace tblup
