// A wide fixed design in the fitted model (tblup_fit_group_batch): k_covar's GLS step for up to FIXED_MAX = 128
// columns F = [Q, Z] -- n_cov dense covariates and the one-hot columns of a class factor (herd, batch, ..) --
// from the Cholesky factor M = L L^T, the inverted diagonal tiles and z = L^{-1} rhs that the chunk's pipeline left
// in the workspace.  The model, the two forms and the NaN rule are k_covar's (its header has them) with F~ in place
// of Q~; a model's column j is covariate j for j < nc, else a level: level j - nc as given under gblup, level
// j - nc + 1 minus its share of the train rows under snp (the lowest level is the reference, its effect 0).
// k_covar holds G in one wave's registers, so it ends at 16 columns; here:
//
// k_fixed_subst: one 512-thread workgroup per (model, slab of 16 columns), k_snpscore's walk of a SNP list.
//   phase 1: R [ns][16] into V.  Kernel form: the train rows of F~ -- a level column is a comparison of the row's
//     code.  SNP form: R = A_T^T F~_T: a covariate is k_covar's fma chain over the train animals in order (its
//     thread map: a row and 8 covariates, a wave's covariate values uniform); a level, thread (system row i,
//     column j), is the allele count of SNP i over the level's train animals (lst / lpos: each
//     train animal belongs to one level, so a model's level columns cost ns x n_T together) minus s_i m_l -- exact
//     integers and one fp64 combination.
//   phase 2 (fwd_subst.h): the blocked forward substitution, unchanged.  V is the slab's own slice of S
//     [B][Cw / 16][ns][16], or LDS copied there at the end: the same arithmetic.
// k_fixed_gls: one 512-thread workgroup per model, G in LDS (128 x 128 doubles at the limit).
//   G = S^T S and h_t = S^T z_t in 16 x 16 blocks on v_mfma_f64_16x16x4_f64, a block one chain over the 4-row groups
//     of the real rows in order (the blocks go round the waves); SNP form: G = (ff - S^T S / d) / lambda,
//     h = (fr - S^T z) / lambda.  Columns past the model's own are identity.
//   G = C C^T right-looking in 16 x 16 blocks: wave 0 factors the diagonal block (k_covar's lane scheme, the pivot
//     rule COVAR_PIV_RTOL against the pivot's own diagonal entry of G), a thread per row solves the panel, all
//     threads update the trailing lower triangle, one fma chain over the block's 16 columns per entry.
//   C y = h_t, C^T b_t = y: thread (trait, row), a column per step.  z* = z - S b (SNP form: / d), one chain over the
//     model's columns in order.
//   Keep mode (FixedKeep non-null: tblup_snp_score_group_batch, tblup_loglik_group_batch), what k_covar's keep mode is
//     for 16 columns: C (row-major with the call's stride, identity past the model's columns), C^{-1} h_t and
//     {log|G| = 2 sum log C_kk, the bad flag, h_t^T b_t = |C^{-1} h_t|^2 per trait} go to the workspace, the sums one
//     chain over the model's columns in order; S is already there.  z* is skipped when z2 is null.  b and z* are
//     the same bits with or without it.
// k_fixed_fitness: k_cov_fitness with a level column as a lookup: y*_V = y_V - (q~_V b_Q + b_level - sum_l m_l b_l).
// k_fixed_cov (tblup_reliability_group_batch): G^{-1} from the kept C, one workgroup per model, C^{-1} in place in LDS.
// No flags, no atomics, every loop bounded by the system's shape and the model's own column count, every sum in a
// fixed order: a model's bits are a function of the model, the design and the system alone.
#include <algorithm>

#include "fwd_subst.h"
#include "pearson_dev.h"

namespace tblup {

namespace {

constexpr int XTH = FWD_TH;
constexpr int XW = FWD_W;
static_assert(FIXED_MAX % XW == 0 && MAXT * FIXED_MAX == XTH, "the solves: one thread per (trait, column)");

// (the host sizes Cw for the call's widest model; the bound only keeps a mistake there inside the buffers)
__device__ __forceinline__ int cols_of(const FixedDesign& f, bool gblup) {
  const int n = fixed_cols(gblup, f.nc, f.L);
  return n < f.Cw ? n : f.Cw;
}
// the level of column j >= nc
__device__ __forceinline__ int level_of(const FixedDesign& f, bool gblup, int j) { return j - f.nc + (gblup ? 0 : 1); }

template <int FORM, bool VLDS>
__global__ __launch_bounds__(XTH) void k_fixed_subst(CholLaunch c, FixedDesign f, int64_t slab0, int64_t nslab,
                                                     double* __restrict__ sbuf) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  constexpr int W = XW;
  const int t = threadIdx.x, l = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6), lc = l & 15, lg = l >> 4;
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t b = blk / nslab, sl = slab0 + blk % nslab;
  const int64_t ns = c.sd.ns, nTp = c.d.nTp;
  const int NT = c.sd.NT;
  const double* sc = c.scal + b * SCAL;
  const int64_t pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const bool gblup = (int)sc[SC_MODE] == 1;
  const int Cm = cols_of(f, gblup);
  if (W * sl >= Cm) return;   // the model has fewer slabs than the call's widest
  double* Vg = sbuf + (b * (f.Cw / W) + sl) * ns * W;
  double* V;
  if constexpr (VLDS) V = dyn;
  else V = Vg;
  const int fo = fold_of(c.ft, b);
  const double* qt = f.qT + (gblup ? 0 : (int64_t)COVAR_W * nTp);
  const int J0 = (int)(pad / TILE), J1 = (int)((pad + nrow + TILE - 1) / TILE);
  // thread (row t / 16 of 32, column t % 16 of the slab)
  const int jj = t & (W - 1), col = W * (int)sl + jj;
  const int lev = level_of(f, gblup, col);
  const double ml = (col >= f.nc && col < Cm && !gblup) ? f.share[lev] : 0.0;

  if constexpr (FORM == FORM_DUAL) {
    for (int64_t r = t / W; r < ns; r += XTH / W) {
      double v = 0.0;
      if (r < nrow && col < Cm) {
        if (col < f.nc) v = qt[(int64_t)col * nTp + r];
        else v = (f.gT[r] == lev ? 1.0 : 0.0) - ml;
      }
      V[r * W + jj] = v;
    }
  } else {
    const int64_t o0 = c.off[b], P = c.d.P;
    const uint8_t* gp = c.ft.gpk[fo];
    const double* ub = c.u + b * c.sd.prow;   // s_i at system row i
    const int64_t r0 = (int64_t)J0 * TILE, nspan = (int64_t)(J1 - J0) * TILE;
    if (sl == 0 && f.nc > 0) {
      // the covariates (columns < nc, all in slab 0) over the block rows that hold real rows: k_covar's chains --
      // work item (half h of the slab's columns, row); a wave's 64 items share h, so its covariate values are
      // uniform; a padding row reads the zero row P
      constexpr int CH = W / 2;
      for (int64_t w0 = 64 * q; w0 < 2 * nspan; w0 += XTH) {
        const int h = (int)(w0 / nspan);
        const int64_t row = r0 + w0 % nspan + l;
        const bool real = sys_real(row, pad, nrow);
        double acc[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[j] = 0.0;
        if (CH * h < f.nc) {
          const int64_t xc = real ? snp_col(c.idx[o0 + row - pad], P) : P;
          const uint32_t* xr = reinterpret_cast<const uint32_t*>(gp + xc * c.gpk_row);   // 16 animals per dword
          const double* qh = qt + (int64_t)CH * h * nTp;
          for (int64_t g = 0; g < nTp / 16; ++g) {
            const uint32_t x = xr[g];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const double xv = (double)((x >> (2 * e)) & 3u);
#pragma unroll
              for (int j = 0; j < CH; ++j) acc[j] = __builtin_fma(xv, qh[(int64_t)j * nTp + 16 * g + e], acc[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j)
          if (CH * h + j < f.nc) V[row * W + CH * h + j] = real ? acc[j] : 0.0;
      }
    }
    // the levels: thread (row, column), the count over the level's train animals four at a time (integers: any
    // order); a covariate column only gets its zeros outside the block rows above
    const bool lcol = col >= f.nc && col < Cm;
    const int p0 = lcol ? f.lst[lev] : 0, p1 = lcol ? f.lst[lev + 1] : 0;
    for (int64_t r = t / W; r < ns; r += XTH / W) {
      double v = 0.0;
      if (lcol && sys_real(r, pad, nrow)) {
        const uint8_t* xb = gp + snp_col(c.idx[o0 + r - pad], P) * c.gpk_row;
        int cnt = 0, p = p0;
        for (; p + 4 <= p1; p += 4) {
          int a[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) a[e] = f.lpos[p + e];
#pragma unroll
          for (int e = 0; e < 4; ++e) cnt += (xb[a[e] >> 2] >> (2 * (a[e] & 3))) & 3;
        }
        for (; p < p1; ++p) {
          const int a = f.lpos[p];
          cnt += (xb[a >> 2] >> (2 * (a & 3))) & 3;
        }
        v = (double)cnt - ub[r] * ml;
      }
      if (col >= f.nc || (uint64_t)(r - r0) >= (uint64_t)nspan) V[r * W + jj] = v;
    }
  }
  __syncthreads();

  const double* Lb = c.L + b * l_stride(NT);
  const double* Db = c.Dinv + b * (int64_t)NT * NPACK * BLKD;
  fwd_subst16(Lb, Db, V, NT, J0, J1, pad, q, lc, lg, [](int, double) {});
  if constexpr (VLDS) {
    for (int64_t i = t; i < ns * W; i += XTH) Vg[i] = V[i];
  }
}

template <int FORM, bool KEEP>
__global__ __launch_bounds__(XTH) void k_fixed_gls(CholLaunch c, FixedDesign f, const double* __restrict__ sbuf,
                                                   double* __restrict__ bhat, double* __restrict__ z2,
                                                   FixedKeep keep) {
  extern __shared__ __attribute__((aligned(16))) double G[];   // [GS][GS], the model's columns rounded up to 16
  __shared__ double gd[FIXED_MAX];            // the diagonal of G before the factorisation
  __shared__ double hs[MAXT][FIXED_MAX];      // h_t
  __shared__ double ys[MAXT][FIXED_MAX];      // C^{-1} h_t
  __shared__ double bs[MAXT][FIXED_MAX];      // b_t
  __shared__ int ok_s;
  constexpr int W = XW;
  const int t = threadIdx.x, l = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6), lc = l & 15, lg = l >> 4;
  const int64_t b = blockIdx.x;
  const int64_t ns = c.sd.ns;
  const int nt = c.d.nt;
  const double* sc = c.scal + b * SCAL;
  const double lam = sc[SC_LAM], dd = sc[SC_D];
  const int64_t pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const bool gblup = (int)sc[SC_MODE] == 1;
  const int Cm = cols_of(f, gblup), nb = (Cm + W - 1) / W, GS = nb * W;
  const double* Sb = sbuf + b * (f.Cw / W) * ns * W;   // the model's slabs [ns][16] back to back
  const double* zb = c.z + b * nt * ns;
  if (t == 0) ok_s = 1;

  // S^T S (blocks I >= J) and S^T z_t (block I against the traits as columns): item w of the waves' round
  {
    const int ntri = nb * (nb + 1) / 2;
    const int64_t g0 = pad / 4, g1 = (pad + nrow + 3) / 4;
    constexpr int TK = 8;   // 4-row groups per step, their loads issued together
    for (int w = q; w < ntri + nb; w += XTH / 64) {
      int I = 0, J = 0;
      const bool hz = w >= ntri;
      if (hz) I = w - ntri;
      else {
        while ((I + 1) * (I + 2) / 2 <= w) ++I;
        J = w - I * (I + 1) / 2;
      }
      const double* sa = Sb + (int64_t)I * ns * W + lc;
      const double* sb = hz ? zb + (int64_t)(lc < nt ? lc : 0) * ns : Sb + (int64_t)J * ns * W + lc;
      const int64_t bstr = hz ? 1 : W;
      const bool bon = !hz || lc < nt;
      v4d acc = {0.0, 0.0, 0.0, 0.0};
      for (int64_t gs = g0; gs < g1; gs += TK) {
        double av[TK], bv[TK];
#pragma unroll
        for (int e = 0; e < TK; ++e) {
          const int64_t r = 4 * (gs + e) + lg;
          const bool on = gs + e < g1 && sys_real(r, pad, nrow);
          av[e] = on ? sa[r * W] : 0.0;
          bv[e] = on && bon ? sb[r * bstr] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < TK; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e], bv[e], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = W * I + lg + 4 * r;
        if (hz) {
          if (lc < MAXT) hs[lc][m] = acc[r];
        } else {
          G[m * GS + W * J + lc] = acc[r];
        }
      }
    }
  }
  __syncthreads();
  // G and h in the model's form; columns past its own: kept out as identity
  for (int e = t; e < GS * GS; e += XTH) {
    const int i = e / GS, j = e % GS;
    if (j > i) continue;
    double v = G[e];
    if constexpr (FORM == FORM_PRIMAL) v = (f.ff[(int64_t)i * f.Cw + j] - v / dd) / lam;
    G[e] = (i < Cm && j < Cm) ? v : (i == j ? 1.0 : 0.0);
  }
  for (int e = t; e < MAXT * GS; e += XTH) {
    const int tr = e / GS, i = e % GS;
    double v = hs[tr][i];
    if constexpr (FORM == FORM_PRIMAL) v = (f.fr[(int64_t)tr * f.Cw + i] - v) / lam;
    hs[tr][i] = (i < Cm && tr < nt) ? v : 0.0;
  }
  __syncthreads();
  if (t < GS) gd[t] = G[t * GS + t];
  __syncthreads();

  // G = C C^T in place (lower), right-looking over the 16-column blocks
  for (int K = 0; K < nb; ++K) {
    const int k0 = W * K;
    if (t < 64) {
      // the diagonal block: lane (copy lg, row lc) holds row lc; after step k its g[k] is C[lc][k]
      const int i = lc;
      double g[W];
#pragma unroll
      for (int j = 0; j < W; ++j) g[j] = j <= i ? G[(k0 + i) * GS + k0 + j] : 0.0;
      bool ok = true;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double pkk = __shfl(g[k], k, W);
        ok = ok && pkk > COVAR_PIV_RTOL * gd[k0 + k] && pkk < __builtin_inf();
        const double ckk = sqrt(pkk);
        const double cik = (i == k) ? ckk : g[k] / ckk;
        g[k] = cik;
#pragma unroll
        for (int j = k + 1; j < W; ++j) {
          const double cjk = __shfl(cik, j, W);
          g[j] = __builtin_fma(-cik, cjk, g[j]);
        }
      }
      if (lg == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (k <= i) G[(k0 + i) * GS + k0 + k] = g[k];
      }
      if (t == 0 && !ok) ok_s = 0;
    }
    __syncthreads();
    const int n0 = k0 + W, m = GS - n0;
    if (t < m) {
      // the panel: row n0 + t of C against the diagonal block, column by column
      double* row = G + (n0 + t) * GS + k0;
      double x[W];
#pragma unroll
      for (int k = 0; k < W; ++k) x[k] = row[k];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double xk = x[k] / G[(k0 + k) * GS + k0 + k];
        x[k] = xk;
#pragma unroll
        for (int j = k + 1; j < W; ++j) x[j] = __builtin_fma(-xk, G[(k0 + j) * GS + k0 + k], x[j]);
      }
#pragma unroll
      for (int k = 0; k < W; ++k) row[k] = x[k];
    }
    __syncthreads();
    for (int e = t; e < m * m; e += XTH) {
      const int i = n0 + e / m, j = n0 + e % m;
      if (j > i) continue;
      const double* ri = G + i * GS + k0;
      const double* rj = G + j * GS + k0;
      double acc = G[i * GS + j];
#pragma unroll
      for (int k = 0; k < W; ++k) acc = __builtin_fma(-ri[k], rj[k], acc);
      G[i * GS + j] = acc;
    }
    __syncthreads();
  }

  // C y = h_t, then C^T b_t = y: thread (trait tr, row i), a column of C per step
  {
    const int tr = t / FIXED_MAX, i = t % FIXED_MAX;
    double rhs = i < GS ? hs[tr][i] : 0.0;
    for (int k = 0; k < GS; ++k) {
      if (i == k) ys[tr][k] = rhs / G[k * GS + k];
      __syncthreads();
      if (i > k && i < GS) rhs = __builtin_fma(-G[i * GS + k], ys[tr][k], rhs);
    }
    double y = i < GS ? ys[tr][i] : 0.0;
    for (int k = GS - 1; k >= 0; --k) {
      if (i == k) bs[tr][k] = y / G[k * GS + k];
      __syncthreads();
      if (i < k) y = __builtin_fma(-G[k * GS + i], bs[tr][k], y);
    }
    __syncthreads();
    const bool bad = !(dd > 0.0) || sc[SC_BAD] != 0.0 || ok_s == 0;
    const double bv = bad ? __builtin_nan("") : (i < Cm ? bs[tr][i] : 0.0);
    __syncthreads();
    if (i < GS) bs[tr][i] = bv;
    if (tr < nt && i < f.Cw) bhat[(b * nt + tr) * f.Cw + i] = bv;
    if constexpr (KEEP) {
      // C^{-1} h_t; h_t^T b_t = |C^{-1} h_t|^2 and log|G| = 2 sum log C_kk, each one chain over the model's columns
      if (i < f.Cw) keep.ch[(b * MAXT + tr) * f.Cw + i] = i < GS ? ys[tr][i] : 0.0;
      double* ks = keep.ks + b * COVAR_KS;
      if (i == 0) {
        double hb = 0.0;
        for (int k = 0; k < Cm; ++k) hb = __builtin_fma(ys[tr][k], ys[tr][k], hb);
        ks[KS_HB + tr] = hb;
      }
      if (t == 1) {
        double slog = 0.0;
        for (int k = 0; k < Cm; ++k) slog += log(G[k * GS + k]);
        ks[KS_LOGG] = 2.0 * slog;
        ks[KS_BAD] = bad ? 1.0 : 0.0;
      }
    }
  }
  if constexpr (KEEP) {
    // C, row-major with the call's stride: identity past the model's blocks
    double* cf = keep.cf + b * (int64_t)f.Cw * f.Cw;
    for (int e = t; e < f.Cw * f.Cw; e += XTH) {
      const int i = e / f.Cw, j = e % f.Cw;
      cf[e] = (i < GS && j <= i) ? G[i * GS + j] : (i == j ? 1.0 : 0.0);
    }
    if (!z2) return;
  }
  __syncthreads();

  // z* = z - S b (SNP form: / d) at the real rows, z elsewhere
  const bool bad = !(dd > 0.0) || sc[SC_BAD] != 0.0 || ok_s == 0;
  for (int64_t e = t; e < (int64_t)nt * ns; e += XTH) {
    const int64_t tr = e / ns, r = e % ns;
    double zv = zb[e];
    if (sys_real(r, pad, nrow)) {
      double acc = 0.0;
      for (int j = 0; j < Cm; ++j) acc = __builtin_fma(Sb[((int64_t)(j / W) * ns + r) * W + j % W], bs[tr][j], acc);
      if constexpr (FORM == FORM_PRIMAL) zv = zv - acc / dd;
      else zv = zv - acc;
      if (bad) zv = __builtin_nan("");
    }
    z2[b * nt * ns + e] = zv;
  }
}

__global__ __launch_bounds__(XTH) void k_fixed_fitness(CholLaunch c, FixedDesign f, const double* __restrict__ ebv,
                                                       const double* __restrict__ bhat, double* __restrict__ fit) {
  extern __shared__ double ysv[];   // y*_V of one trait
  __shared__ double red[4 * 16];
  __shared__ double b_s[MAXT][FIXED_MAX];
  __shared__ double cm_s[MAXT];     // sum_l m_l b_l over the model's level columns in order
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x, nV = c.d.nV;
  const int nt = c.d.nt;
  const double* sc = c.scal + b * SCAL;
  const bool gblup = (int)sc[SC_MODE] == 1;
  const int Cm = cols_of(f, gblup);
  const int fo = fold_of(c.ft, b);
  const double* qv = f.qV + (gblup ? 0 : (int64_t)COVAR_W * nV);
  {
    const int tr = t / FIXED_MAX, j = t % FIXED_MAX;
    b_s[tr][j] = (tr < nt && j < Cm) ? bhat[(b * nt + tr) * f.Cw + j] : 0.0;
  }
  __syncthreads();
  if (t < MAXT) {
    double acc = 0.0;
    if (!gblup)
      for (int j = f.nc; j < Cm; ++j) acc = __builtin_fma(f.share[level_of(f, gblup, j)], b_s[t][j], acc);
    cm_s[t] = acc;
  }
  __syncthreads();
  double fsum = 0.0;
  for (int tr = 0; tr < nt; ++tr) {
    const double* yV = c.ft.yV[fo] + (int64_t)tr * nV;
    for (int64_t v = t; v < nV; v += XTH) {
      double acc = 0.0;
      for (int j = 0; j < f.nc; ++j) acc = __builtin_fma(qv[(int64_t)j * nV + v], b_s[tr][j], acc);
      const int jl = f.nc + f.gV[v] - (gblup ? 0 : 1);   // the level's column; nc - 1: the reference level
      const double bl = jl >= f.nc ? b_s[tr][jl] : 0.0;
      ysv[v] = yV[v] - (acc + (bl - cm_s[tr]));
    }
    __syncthreads();
    fsum += pearson_abs<XTH>(ebv + (b * nt + tr) * nV, ysv, nV, red);
    __syncthreads();
  }
  if (t == 0) fit[b] = sc[SC_BAD] != 0.0 ? __builtin_nan("") : (nt == 1) ? fsum : fsum / (double)nt;
}

// fixed_cov = G^{-1} = C^{-T} C^{-1} of every model from the factor k_fixed_gls keeps (k_cov_cov for the wide
// design): one workgroup per model, C in LDS.  C^{-1} in place, thread j its column j: the column-by-column solve of
// C x = e_j with x kept in column j itself -- at step k the threads j < k take x_k = x[k] / C_kk and update their
// rows below k with column k of C, then thread k turns column k into its own x (x_k = 1 / C_kk, -C_ik x_k below).
// G^{-1}(i, j) is one chain over k = max(i, j) .. Cm - 1 in order, the same bits at (i, j) and (j, i), written at the
// caller's [nc + L][nc + L]: covariates then levels, zeros in the row and the column of the level that an snp model
// drops.  NaN throughout for a model whose ks is flagged.
__global__ __launch_bounds__(XTH) void k_fixed_cov(CholLaunch c, FixedDesign f, const double* __restrict__ cf,
                                                   const double* __restrict__ ks, double* __restrict__ fc) {
  extern __shared__ __attribute__((aligned(16))) double M[];   // [Cw][Cw]
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int Cw = f.Cw;
  const bool gblup = (int)c.scal[b * SCAL + SC_MODE] == 1;
  const int Cm = cols_of(f, gblup);
  const double* C = cf + b * (int64_t)Cw * Cw;
  for (int e = t; e < Cw * Cw; e += XTH) M[e] = C[e];
  __syncthreads();
  for (int k = 0; k < Cm; ++k) {
    const double ckk = M[k * Cw + k];
    if (t < k) {
      const double xk = M[k * Cw + t] / ckk;
      for (int i = k + 1; i < Cm; ++i) M[i * Cw + t] = __builtin_fma(-M[i * Cw + k], xk, M[i * Cw + t]);
      M[k * Cw + t] = xk;
    }
    __syncthreads();
    if (t == k) {
      const double xk = 1.0 / ckk;
      for (int i = k + 1; i < Cm; ++i) M[i * Cw + k] = -M[i * Cw + k] * xk;
      M[k * Cw + k] = xk;
    }
    __syncthreads();
  }
  const int Co = f.nc + f.L, drop = gblup ? 0 : 1;
  const bool bad = ks[b * COVAR_KS + KS_BAD] != 0.0;
  double* out = fc + b * (int64_t)Co * Co;
  for (int e = t; e < Co * Co; e += XTH) {
    const int oi = e / Co, oj = e % Co;
    // the model's column of an output index; the reference level of an snp model has none
    const int i = oi < f.nc ? oi : oi - drop, j = oj < f.nc ? oj : oj - drop;
    const bool ref = drop && (oi == f.nc || oj == f.nc);
    double acc = 0.0;
    if (!ref && i < Cm && j < Cm)
      for (int k = i > j ? i : j; k < Cm; ++k) acc = __builtin_fma(M[k * Cw + i], M[k * Cw + j], acc);
    out[e] = bad ? __builtin_nan("") : acc;
  }
}

bool design_ok(const CholLaunch& c, const FixedDesign& f) {
  return c.d.nt >= 1 && c.d.nt <= MAXT && f.nc >= 0 && f.nc <= COVAR_W && f.L >= 1 && f.Cw >= XW && f.Cw <= FIXED_MAX &&
         f.Cw % XW == 0;
}

}  // namespace

hipError_t launch_fixed_subst(const CholLaunch& c, const FixedDesign& f, const SlabPlan& p, double* sbuf,
                              hipStream_t s) {
  if (c.B < 1) return hipSuccess;
  if (!design_ok(c, f) || !sbuf) return hipErrorInvalidValue;
  using Kern = decltype(&k_fixed_subst<FORM_DUAL, false>);
  const Kern kern[4] = {k_fixed_subst<FORM_DUAL, false>, k_fixed_subst<FORM_DUAL, true>,
                        k_fixed_subst<FORM_PRIMAL, false>, k_fixed_subst<FORM_PRIMAL, true>};
  return launch_slabs(kern, c, p, sbuf, f.Cw / XW, [&](Kern k, dim3 grid, size_t shm, int64_t s0, int64_t sn) {
    hipLaunchKernelGGL(k, grid, dim3(XTH), shm, s, c, f, s0, sn, sbuf);
  });
}

hipError_t launch_fixed_gls(const CholLaunch& c, const FixedDesign& f, const double* sbuf, double* bhat, double* z2,
                            const FixedKeep& keep, hipStream_t s) {
  if (c.B < 1) return hipSuccess;
  // keep mode: every buffer or none
  const bool kp = keep.cf || keep.ch || keep.ks;
  if (kp && !(keep.cf && keep.ch && keep.ks)) return hipErrorInvalidValue;
  if (!design_ok(c, f) || !sbuf || !bhat || (!kp && !z2)) return hipErrorInvalidValue;
  const bool primal = c.sd.form == FORM_PRIMAL;
  const auto k = kp ? (primal ? k_fixed_gls<FORM_PRIMAL, true> : k_fixed_gls<FORM_DUAL, true>)
                    : (primal ? k_fixed_gls<FORM_PRIMAL, false> : k_fixed_gls<FORM_DUAL, false>);
  const size_t shm = (size_t)f.Cw * f.Cw * 8;
  hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3((unsigned)c.B), dim3(XTH), shm, s, c, f, sbuf, bhat, z2, keep);
  return hipGetLastError();
}

hipError_t launch_fixed_cov(const CholLaunch& c, const FixedDesign& f, const double* cf, const double* ks, double* fc,
                            hipStream_t s) {
  if (c.B < 1) return hipSuccess;
  if (!design_ok(c, f) || !cf || !ks || !fc || c.B > 0x7fffffff) return hipErrorInvalidValue;
  const size_t shm = (size_t)f.Cw * f.Cw * 8;
  hipError_t e = hipFuncSetAttribute((const void*)k_fixed_cov, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_fixed_cov, dim3((unsigned)c.B), dim3(XTH), shm, s, c, f, cf, ks, fc);
  return hipGetLastError();
}

hipError_t launch_fixed_fitness(const CholLaunch& c, const FixedDesign& f, const double* ebv, const double* bhat,
                                double* fit, hipStream_t s) {
  if (c.B < 1) return hipSuccess;
  if (!design_ok(c, f)) return hipErrorInvalidValue;
  const size_t shm = (size_t)c.d.nV * 8;
  if (shm > 140 * 1024) return hipErrorInvalidValue;   // (k_solve's own LDS bound on n_V is tighter)
  if (shm > 48 * 1024) {
    hipError_t e =
        hipFuncSetAttribute((const void*)k_fixed_fitness, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_fixed_fitness, dim3((unsigned)c.B), dim3(XTH), shm, s, c, f, ebv, bhat, fit);
  return hipGetLastError();
}

}  // namespace tblup
