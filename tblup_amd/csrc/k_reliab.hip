// Reliabilities of predicted breeding values (tblup_reliability_batch): for every listed animal a of
// the panel, from the Cholesky factor L L^T and the inverted diagonal tiles X_J = L_JJ^{-1} that the
// chunk's pipeline left in the workspace (what k_effects reads; neither solve kernel writes them),
//   kernel form  rel(a) = |L^{-1} k_Ta|^2 / K_aa,            k_Ta = W_T w_a / d, K_aa = w_a.w_a / d
//   SNP form     rel(a) = 1 - lambda |L^{-1} w_a|^2 / (w_a.w_a)
// with w_a = A[a] - c the animal's centred row over the model's SNPs (the two are equal by the
// Woodbury identity).  No phenotype and no variance component enters.
//
// One 512-thread workgroup per (model, slab of RW = 16 listed animals); workgroups are independent
// (no flags, no hand-offs, every loop bounded by the system's shape).
//   phase 1: the slab's right-hand sides R [ns][16] into V.  SNP form: gathered from the SNP-major
//     int8 panel and centred with the centre k_effects writes; w_a.w_a in one fma chain in list order.
//     Kernel form: the exact counts (A_T A_a^T)_ta on int8 MFMA (v_mfma_i32_16x16x64_i8) -- the train
//     rows from the chunk's 2-bit packed panel (unpack16), the animals' genotypes gathered into LDS in
//     the same byte order -- then (G_ta - (u_t + u_a)/N + q/N^2)/d in fp64; u_a and G_aa are exact
//     integer sums.
//   phase 2 (fwd_subst.h): blocked forward substitution with 16 right-hand sides on fp64 MFMA
//     (v_mfma_f64_16x16x4_f64), block row by block row: V_J = X_J (R_J - sum_{L<J} L_JL V_L); wave q
//     owns rows 16q .. 16q+15 of the block row, one accumulator chain over L = J0 .. J-1 and the rows
//     of each tile in order (L read once per slab, from L2: a model's slabs run on one XCD), then
//     over the blocks s = 0 .. q of X_J.  Every lane adds the squares of
//     its four rows of V_J to one running sum; the 32 partial sums of an animal are added in a fixed
//     order at the end.
// So an animal's value is a function of its genotypes and the system alone: not of n_pred, of its
// place in the list, of its slab or of the chunking.
// V lives in LDS when ns x 16 doubles fit beside the staging buffers (ns <= 1024), else in a
// workspace slice of the workgroup's own -- the same arithmetic in the same order.
//
// COV instances (tblup_reliability_cov_batch): the reliabilities under the model with fixed-effect covariates
// Q~ that k_covar fits, from what its keep mode left in the workspace -- S = L^{-1} R of the covariates, the
// factor C of G = Q~_T^T V^{-1} Q~_T and the bad flag.  With s_a the animal's solved column and
// kVk = k_Ta^T V^{-1} k_Ta (kernel form |s_a|^2; SNP form K_aa - lambda |s_a|^2 / d, K_aa = w_a.w_a / d):
//   a_a = Q~_T^T V^{-1} k_Ta:  kernel form S^T s_a;  SNP form S^T s_a / d   (V^{-1} W_T = W_T M^{-1}, R = W_T^T Q~_T)
//   rel_cov = (kVk - |C^{-1} a_a|^2) / K_aa,   pev_total = K_aa - kVk + |C^{-1} (q~_a - a_a)|^2
// behind phase 2, with the same sum for |s_a|^2 as the plain instances:
//   T = S^T s for the slab's 16 animals on fp64 MFMA, k_snpscore's cross product (wave q over the 4-row groups
//     pad / 4 + q, + 8, .. of the real rows in order, S from global / L2); the 8 tiles are staged in the head of V
//     itself, which is done with by then, and added in wave order: no LDS beyond the plain instances';
//   thread (animal, covariate) of the first four waves: a_a, q~_a - a_a (q~_a from the call's [n_pred][16] array of
//     the model's branch), the two substitutions C y = a_a and C x = q~_a - a_a column by column by lane shuffles.
// NaN also for a model whose G has no positive pivot.  k_cov_cov inverts C into G^{-1} per model.
//
// FIX instances (tblup_reliability_group_batch): the same two values for the wide fixed design F~ = [Q~, Z~] of up to
// FIXED_MAX = 128 columns that k_fixed.hip fits, from what k_fixed_subst and k_fixed_gls (keep mode) left in the
// workspace -- S slab-major [Cw / 16][ns][16], C [Cw][Cw] and the bad flag.  Phase 1, the substitution and the sum
// for |s_a|^2 are the plain instances'; behind them, for the model's own Cm columns:
//   T = S^T s, Cm x 16, on fp64 MFMA: wave q takes the design's column slab q over all real 4-row groups in order, so
//     the waves' tiles are T itself and nothing is summed across waves; T is staged in the head of V;
//   thread (animal, r of 32) holds a_a and f~_a - a_a at the columns r, r + 32, ..: a covariate's entry of f~_a from
//     the call's array, a level's from the animal's code and the levels' shares;
//   C y = a_a and C x = f~_a - a_a together, column by column: the owner of row k hands y_k and x_k to the animal's
//     32 threads through a double-buffered LDS slot (one barrier a column), every thread updates its rows below k
//     with its column of C streamed from global / L2 a step ahead; thread (animal, 0) takes |y|^2 and |x|^2 on the
//     way, each one chain over the model's columns in order.
// 512 bytes of static LDS (the column slot) come on top, in these instances only.  k_fixed_cov (k_fixed.hip) inverts
// C into G^{-1} per model.
#include <algorithm>
#include <type_traits>

#include "fwd_subst.h"
#include "i8_tile.h"

namespace tblup {

namespace {

constexpr int RTH = FWD_TH;       // 8 waves
constexpr int RKC = 1024;         // kernel form: SNPs per LDS stage of the animals' genotypes
constexpr int RKS = RKC + 16;     // its row stride (bytes): 16 animals' 16-B reads on distinct banks
constexpr int RPARTS = RTH / RELIAB_W;
static_assert(RELIAB_W == FWD_W, "k_reliab's slab is the substitution's 16 right-hand sides");

// ADJ: the fixed effects the reliabilities are adjusted for, and the struct that carries them (k_snpscore's modes)
constexpr int ADJ_NONE = 0, ADJ_COV = 1, ADJ_FIX = 2;
template <int ADJ>
using ReliabAdj = std::conditional_t<ADJ == ADJ_FIX, ReliabFixed, ReliabCov>;

template <int FORM, bool VLDS, int ADJ>
__global__ __launch_bounds__(RTH) void k_reliab(CholLaunch c, const int8_t* __restrict__ geno,
                                                const int32_t* __restrict__ csA,
                                                const int32_t* __restrict__ animals, int64_t n_pred, int64_t slab0,
                                                int64_t nslab, double* __restrict__ vscr, ReliabAdj<ADJ> cv,
                                                double* __restrict__ rel) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  __shared__ double nrm[RTH];
  __shared__ double den[RELIAB_W];   // SNP form: w_a.w_a; kernel form: K_aa
  constexpr int W = RELIAB_W;
  const int t = threadIdx.x, l = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6), lc = l & 15, lg = l >> 4;
  // consecutive slabs of a model on one XCD, so that its L tiles are shared in that XCD's L2 (speed only)
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t b = blk / nslab, sl = slab0 + blk % nslab;
  const int64_t ns = c.sd.ns, n = c.d.n, P = c.d.P;
  const int NT = c.sd.NT;
  double* V;
  if constexpr (VLDS) V = dyn;
  else V = vscr + (int64_t)blockIdx.x * ns * W;
  const double* sc = c.scal + b * SCAL;
  const double lam = sc[SC_LAM], dd = sc[SC_D], invd = sc[SC_INVD];
  const int64_t kk = (int64_t)sc[SC_K], pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const bool gblup = (int)sc[SC_MODE] == 1;
  const int fo = fold_of(c.ft, b);
  const int32_t* cs = gblup ? csA : c.ft.csT[fo];
  const double N = gblup ? (double)n : (double)c.d.nT;
  const int64_t o0 = c.off[b];
  // block rows that hold real system rows (the rest is identity padding with zero right-hand sides)
  const int J0 = (int)(pad / TILE), J1 = (int)((pad + nrow + TILE - 1) / TILE);
  // phase 1 thread map: animal ta of the slab, part tp of RPARTS
  const int ta = t & (W - 1), tp = t / W;
  const int64_t va = sl * W + ta;
  const int64_t an = va < n_pred ? animals[va] : animals[0];

  if constexpr (FORM == FORM_PRIMAL) {
    // (every row loads -- a padding row the first SNP's values, then dropped -- so that the unrolled
    // loop's loads are in flight together)
#pragma unroll 8
    for (int64_t r = (int64_t)J0 * TILE + tp; r < (int64_t)J1 * TILE; r += RPARTS) {
      const bool real = sys_real(r, pad, nrow);
      const int64_t col = snp_col(c.idx[o0 + (real ? r - pad : 0)], P);
      const double x = (double)geno[col * n + an] - (double)cs[col] / N;
      V[r * W + ta] = real ? x : 0.0;
    }
    __syncthreads();
    if (t < W) {
      double ww = 0.0;
#pragma unroll 8
      for (int64_t j = 0; j < kk; ++j) {
        const double x = V[(pad + j) * W + t];
        ww = __builtin_fma(x, x, ww);
      }
      den[t] = ww;
    }
  } else {
    __shared__ __attribute__((aligned(16))) int8_t ab[W * RKS];
    __shared__ long long ired[2][W][RPARTS];
    __shared__ double ua_s[W];
    const uint8_t* pb = c.panel + b * c.pstride;
    const int64_t pk_row = (c.sd.cblk + 3) / 4 * 64;   // dual_pk_row
    const int64_t nrb = (int64_t)J1 * (TILE / 16);   // 16-row blocks of the real block rows
    long long iu = 0, ig = 0;
    for (int64_t k0 = 0; k0 < kk; k0 += RKC) {
      const int kc = (int)min((int64_t)RKC, kk - k0);
      const int kc64 = (kc + KBLK - 1) / KBLK * KBLK;
      for (int jj = tp; jj < kc64; jj += RPARTS) {
        int g = 0;
        if (jj < kc) {
          const int64_t col = snp_col(c.idx[o0 + k0 + jj], P);
          g = geno[col * n + an];
          iu += (long long)g * cs[col];
          ig += (long long)g * g;
        }
        // unpack16's order: byte m of dword e of a 16-SNP group is its SNP 4m + e
        const int e16 = jj & 15;
        ab[ta * RKS + (jj & ~15) + 4 * (e16 & 3) + (e16 >> 2)] = (int8_t)g;
      }
      __syncthreads();
      for (int64_t rb = q; rb < nrb; rb += RTH / 64) {
        v4i acc = {0, 0, 0, 0};
        const uint8_t* prow = pb + (16 * rb + lc) * pk_row + k0 / 4 + 4 * lg;
        for (int kb = 0; kb < kc64 / KBLK; ++kb) {
          const v4i a = unpack16(*reinterpret_cast<const uint32_t*>(prow + 16 * kb));
          const v4i bv = *reinterpret_cast<const v4i*>(ab + lc * RKS + KBLK * kb + 16 * lg);
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t vi = (16 * rb + 4 * lg + r) * W + lc;
          V[vi] = (k0 == 0 ? 0.0 : V[vi]) + (double)acc[r];   // exact integers
        }
      }
      __syncthreads();
    }
    ired[0][ta][tp] = iu;
    ired[1][ta][tp] = ig;
    __syncthreads();
    const double sa = sc[SC_SA], cN = sc[SC_CN];
    if (t < W) {
      long long su = 0, sg = 0;
      for (int p = 0; p < RPARTS; ++p) {
        su += ired[0][t][p];
        sg += ired[1][t][p];
      }
      const double ua = (double)su;
      ua_s[t] = ua;
      den[t] = ((double)sg - (ua + ua) * sa + cN) * invd;
    }
    __syncthreads();
    const double* ub = c.u + b * c.sd.prow;
    const double ua = ua_s[lc];
    for (int64_t rb = q; rb < nrb; rb += RTH / 64) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = 16 * rb + 4 * lg + r;
        const int64_t vi = row * W + lc;
        V[vi] = row < nrow ? (V[vi] - (ub[row] + ua) * sa + cN) * invd : 0.0;
      }
    }
  }
  __syncthreads();

  // phase 2: V_J = X_J (R_J - sum_{L<J} L_JL V_L)
  const double* Lb = c.L + b * l_stride(NT);
  const double* Db = c.Dinv + b * (int64_t)NT * NPACK * BLKD;
  double nacc = 0.0;
  fwd_subst16(Lb, Db, V, NT, J0, J1, pad, q, lc, lg, [&](int, double v) { nacc = __builtin_fma(v, v, nacc); });
  nrm[t] = nacc;
  if constexpr (ADJ == ADJ_COV) {
    // The covariates' share: a_a = Q~_T^T V^{-1} k_Ta from T = S^T s_a (S = L^{-1} R of the covariates, k_covar's
    // keep mode) -- k_snpscore's cross product: rows of S (global / L2) against the same rows of the solved V on
    // fp64 MFMA, wave q over the 4-row groups pad / 4 + q, + 8, .. of the real rows in order (a function of the
    // system alone); a row outside them counts as zero.
    const double* sq = cv.sq + b * ns * W;
    v4d tacc = {0.0, 0.0, 0.0, 0.0};
    const int64_t g1 = (pad + nrow + 3) / 4;
    constexpr int TKC = 8;   // groups per step, their loads issued together (16 spills beside the substitution's ring)
    for (int64_t g0 = pad / 4 + q; g0 < g1; g0 += TKC * (RTH / 64)) {
      double sa[TKC], sv[TKC];
#pragma unroll
      for (int e = 0; e < TKC; ++e) {
        const int64_t g = g0 + e * (RTH / 64), r = 4 * g + lg;
        sa[e] = g < g1 && sys_real(r, pad, nrow) ? sq[r * W + lc] : 0.0;
        sv[e] = g < g1 ? V[r * W + lc] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < TKC; ++e) tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa[e], sv[e], tacc, 0, 0, 0);
    }
    // the solved V is done with: its first 8 x 256 doubles (ns >= TILE rows of 16) stage the waves' tiles,
    // element [covariate][animal] -- no LDS beyond the plain instances'
    static_assert((RTH / 64) * W * W <= TILE * W, "the waves' tiles fit the smallest V");
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) V[q * W * W + (lg + 4 * r) * W + lc] = tacc[r];
    __syncthreads();
    // thread (animal an = t / 16, covariate i = t % 16) of the first four waves: a_a (SNP form: S^T s_a / d) and
    // e_a = q~_a - a_a, the tiles added in wave order; then C y = a_a and C x = e_a column by column
    // (k_covar's own substitution, the solved entries passed by lane shuffles), y.y and x.x on the way
    if (t < W * W) {
      const int i = t & (W - 1), an = t >> 4;
      const int64_t va = sl * W + an;
      const bool live = va < n_pred;
      double T = 0.0;
      for (int w = 0; w < RTH / 64; ++w) T += V[w * W * W + i * W + an];
      if constexpr (FORM == FORM_PRIMAL) T = T / dd;
      const bool in = i < cv.nc;
      const double qv = live && in ? cv.qa[((gblup ? 0 : n_pred) + va) * W + i] : 0.0;
      double a = in ? T : 0.0, e = in ? qv - T : 0.0;
      double crow[W];   // row i of C
#pragma unroll
      for (int k = 0; k < W; ++k) crow[k] = cv.cf[(b * W + i) * W + k];
      double cii = 1.0;
#pragma unroll
      for (int k = 0; k < W; ++k) cii = (k == i) ? crow[k] : cii;
      double yy = 0.0, xx = 0.0;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double yk = __shfl(a / cii, k, W), xk = __shfl(e / cii, k, W);
        if (i > k) {
          a = __builtin_fma(-crow[k], yk, a);
          e = __builtin_fma(-crow[k], xk, e);
        }
        yy = __builtin_fma(yk, yk, yy);
        xx = __builtin_fma(xk, xk, xx);
      }
      if (i == 0 && live) {
        double s2 = 0.0;
        for (int w = 0; w < RTH / 64; ++w)
          for (int g = 0; g < 4; ++g) s2 += nrm[64 * w + 16 * g + an];
        // kVk = k_Ta^T V^{-1} k_Ta and K_aa; SNP form: K_aa - kVk = lambda |s_a|^2 / d
        const double dn = den[an];
        double r, pv;
        if constexpr (FORM == FORM_PRIMAL) {
          const double kaa = dn / dd, gap = lam * s2 / dd;
          r = ((kaa - gap) - yy) / kaa;
          pv = gap + xx;
        } else {
          r = (s2 - yy) / dn;
          pv = (dn - s2) + xx;
        }
        if (dd == 0.0 || dn == 0.0 || sc[SC_BAD] != 0.0 || cv.ks[b * COVAR_KS + KS_BAD] != 0.0)
          r = pv = __builtin_nan("");
        rel[b * n_pred + va] = r;
        if (cv.pev) cv.pev[b * n_pred + va] = pv;
      }
    }
    return;
  } else if constexpr (ADJ == ADJ_FIX) {
    // The wide design's share: a_a = F~_T^T V^{-1} k_Ta for the model's Cm columns from T = S^T s_a, Cm x 16, on fp64
    // MFMA -- k_snpscore's FIX cross product: wave q takes the design's column slab q (S slab-major: the slab's
    // [ns][16] from global / L2) over all 4-row groups of the real rows in order, so its tile is rows 16 q .. 16 q + 15
    // of T itself and nothing is summed across waves; a row outside the real ones counts as zero.
    const FixedDesign& f = cv.f;
    const int Cw = f.Cw;
    const int Cm = std::min(fixed_cols(gblup, f.nc, f.L), Cw), nb = (Cm + W - 1) / W;
    v4d tacc = {0.0, 0.0, 0.0, 0.0};
    if (q < nb) {
      const double* sq = cv.sbuf + (b * (Cw / W) + q) * ns * W;
      const int64_t g1 = (pad + nrow + 3) / 4;
      constexpr int TKC = 8;   // groups per step, their loads issued together (the COV instances' count)
      for (int64_t g0 = pad / 4; g0 < g1; g0 += TKC) {
        double sa[TKC], sv[TKC];
#pragma unroll
        for (int e = 0; e < TKC; ++e) {
          const int64_t g = g0 + e, r = 4 * g + lg;
          sa[e] = g < g1 && sys_real(r, pad, nrow) ? sq[r * W + lc] : 0.0;
          sv[e] = g < g1 ? V[r * W + lc] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < TKC; ++e) tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa[e], sv[e], tacc, 0, 0, 0);
      }
    }
    // the solved V is done with: its first Cw x 16 doubles (ns >= TILE >= Cw rows of 16) stage T, element
    // [column][animal] -- no dynamic LDS beyond the plain instances'
    static_assert(FIXED_MAX <= TILE && (RTH / 64) * W >= FIXED_MAX && FIXED_MAX % RPARTS == 0,
                  "T fits the smallest V; a wave per column slab; the solve's rows go round the animal's threads");
    __shared__ double ycol[2][2][W];   // the solves' current column of y and of x, double-buffered
    __syncthreads();
    if (q < nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) V[(W * q + lg + 4 * r) * W + lc] = tacc[r];
    }
    __syncthreads();
    // Thread (animal ta, tp of 32) holds a_a (SNP form: T / d) and e_a = f~_a - a_a at the columns tp, tp + 32, ..: a
    // covariate's entry of f~_a from the call's array of the model's branch, a level's [code == level] minus, under
    // snp, the level's share (an animal without a level: the centre alone).
    constexpr int NR = FIXED_MAX / RPARTS;
    const bool live = va < n_pred;
    const int code = live ? cv.ga[va] : -1;
    double a[NR], e[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      const int i = tp + RPARTS * m;
      double T = i < Cm ? V[i * W + ta] : 0.0;
      if constexpr (FORM == FORM_PRIMAL) T = T / dd;
      double fv = 0.0;
      if (i < f.nc) {
        fv = live ? cv.qa[((gblup ? 0 : n_pred) + va) * COVAR_W + i] : 0.0;
      } else if (i < Cm) {
        const int lev = i - f.nc + (gblup ? 0 : 1);
        fv = (code == lev ? 1.0 : 0.0) - (gblup ? 0.0 : f.share[lev]);
      }
      a[m] = i < Cm ? T : 0.0;
      e[m] = i < Cm ? fv - T : 0.0;
    }
    // C y = a_a and C x = e_a together, column by column (k_snpscore's FIX solve): one column of C streamed from
    // global / L2 a step ahead serves both; the owner of row k hands y_k and x_k to the animal's threads through LDS
    // (one barrier a column), every thread updates its rows below k; thread (ta, 0) takes y.y and x.x on the way, each
    // one chain over the model's columns in order
    const double* Cb = cv.cf + b * (int64_t)Cw * Cw;
    double yy = 0.0, xx = 0.0;
    double cn[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      const int i = tp + RPARTS * m;
      cn[m] = i < Cm ? Cb[(int64_t)i * Cw] : 0.0;
    }
    for (int k = 0; k < Cm; ++k) {
      double cc[NR];
#pragma unroll
      for (int m = 0; m < NR; ++m) {
        const int i = tp + RPARTS * m;
        cc[m] = cn[m];
        cn[m] = (i > k && i < Cm) ? Cb[(int64_t)i * Cw + k + 1] : 0.0;
      }
      if (tp == k % RPARTS) {
        double ak = 0.0, ek = 0.0, ckk = 1.0;
#pragma unroll
        for (int m = 0; m < NR; ++m)
          if (m == k / RPARTS) ak = a[m], ek = e[m], ckk = cc[m];
        ycol[k & 1][0][ta] = ak / ckk;
        ycol[k & 1][1][ta] = ek / ckk;
      }
      __syncthreads();
      const double yk = ycol[k & 1][0][ta], xk = ycol[k & 1][1][ta];
#pragma unroll
      for (int m = 0; m < NR; ++m) {
        const int i = tp + RPARTS * m;
        if (i > k && i < Cm) {
          a[m] = __builtin_fma(-cc[m], yk, a[m]);
          e[m] = __builtin_fma(-cc[m], xk, e[m]);
        }
      }
      if (tp == 0) {
        yy = __builtin_fma(yk, yk, yy);
        xx = __builtin_fma(xk, xk, xx);
      }
    }
    if (tp == 0 && live) {
      double s2 = 0.0;
      for (int w = 0; w < RTH / 64; ++w)
        for (int g = 0; g < 4; ++g) s2 += nrm[64 * w + 16 * g + ta];
      // the COV instances' end, with the model's own columns behind yy and xx
      const double dn = den[ta];
      double r, pv;
      if constexpr (FORM == FORM_PRIMAL) {
        const double kaa = dn / dd, gap = lam * s2 / dd;
        r = ((kaa - gap) - yy) / kaa;
        pv = gap + xx;
      } else {
        r = (s2 - yy) / dn;
        pv = (dn - s2) + xx;
      }
      if (dd == 0.0 || dn == 0.0 || sc[SC_BAD] != 0.0 || cv.ks[b * COVAR_KS + KS_BAD] != 0.0)
        r = pv = __builtin_nan("");
      rel[b * n_pred + va] = r;
      if (cv.pev) cv.pev[b * n_pred + va] = pv;
    }
    return;
  }
  __syncthreads();
  if (t < W && sl * W + t < n_pred) {
    double s2 = 0.0;
    for (int w = 0; w < RTH / 64; ++w)
      for (int g = 0; g < 4; ++g) s2 += nrm[64 * w + 16 * g + t];
    double r;
    if constexpr (FORM == FORM_PRIMAL) r = 1.0 - lam * s2 / den[t];
    else r = s2 / den[t];
    if (dd == 0.0 || den[t] == 0.0 || sc[SC_BAD] != 0.0) r = __builtin_nan("");
    rel[b * n_pred + sl * W + t] = r;
  }
}

// cov_cov = G^{-1} = C^{-T} C^{-1} of every model from the factor k_covar keeps (identity past nc): thread j < 16
// solves C x = e_j (column j of C^{-1}), thread (i, j) one chain over k = max(i, j) .. nc - 1 in order -- the
// same bits at (i, j) and (j, i).  NaN for a model whose ks is flagged.
__global__ __launch_bounds__(COVAR_W* COVAR_W) void k_cov_cov(const double* __restrict__ cf,
                                                               const double* __restrict__ ks, int nc,
                                                               double* __restrict__ cc) {
  constexpr int W = COVAR_W;
  __shared__ double ci[W][W];   // C^{-1}, row-major
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* C = cf + b * W * W;
  if (t < W) {
    double x[W];
#pragma unroll
    for (int i = 0; i < W; ++i) x[i] = i == t ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const double xk = x[k] / C[k * W + k];
#pragma unroll
      for (int i = k + 1; i < W; ++i) x[i] = __builtin_fma(-C[i * W + k], xk, x[i]);
      ci[k][t] = xk;
    }
  }
  __syncthreads();
  const int i = t >> 4, j = t & 15;
  if (i < nc && j < nc) {
    double acc = 0.0;
    for (int k = i > j ? i : j; k < nc; ++k) acc = __builtin_fma(ci[k][i], ci[k][j], acc);
    cc[(b * nc + i) * nc + j] = ks[b * COVAR_KS + KS_BAD] != 0.0 ? __builtin_nan("") : acc;
  }
}

}  // namespace

SlabPlan slab_plan(const SysDims& sd, int64_t B, int64_t n_items, bool lds_knob, int64_t aim) {
  const bool lds = lds_knob && sd.ns * FWD_W * 8 <= RELIAB_LDS_V;
  int64_t S = (n_items + FWD_W - 1) / FWD_W;
  if (!lds) S = std::min(S, std::max<int64_t>(1, aim / (B * sd.ns * FWD_W * 8)));
  S = std::max<int64_t>(1, std::min(S, (int64_t)0x7fffffff / std::max<int64_t>(B, 1)));
  return {lds, S, B * S, sd.ns};
}

hipError_t launch_reliab(const CholLaunch& c, const int8_t* geno_sm, const int32_t* csA, const int32_t* animals,
                         int64_t n_pred, const SlabPlan& p, double* vscr, const ReliabCov* cov, double* rel,
                         hipStream_t s) {
  if (c.B < 1 || n_pred < 1) return hipSuccess;
  if (cov && (!cov->sq || !cov->cf || !cov->ks || !cov->qa || cov->nc < 1 || cov->nc > COVAR_W))
    return hipErrorInvalidValue;
  using Kern = decltype(&k_reliab<FORM_DUAL, false, ADJ_NONE>);
  const Kern plain[4] = {k_reliab<FORM_DUAL, false, ADJ_NONE>, k_reliab<FORM_DUAL, true, ADJ_NONE>,
                         k_reliab<FORM_PRIMAL, false, ADJ_NONE>, k_reliab<FORM_PRIMAL, true, ADJ_NONE>};
  const Kern adj[4] = {k_reliab<FORM_DUAL, false, ADJ_COV>, k_reliab<FORM_DUAL, true, ADJ_COV>,
                       k_reliab<FORM_PRIMAL, false, ADJ_COV>, k_reliab<FORM_PRIMAL, true, ADJ_COV>};
  const ReliabCov cv = cov ? *cov : ReliabCov{};
  const auto launch = [&](Kern k, dim3 grid, size_t shm, int64_t s0, int64_t sn) {
    hipLaunchKernelGGL(k, grid, dim3(RTH), shm, s, c, geno_sm, csA, animals, n_pred, s0, sn, vscr, cv, rel);
  };
  return launch_slabs(cov ? adj : plain, c, p, vscr, (n_pred + RELIAB_W - 1) / RELIAB_W, launch);
}

hipError_t launch_reliab_fixed(const CholLaunch& c, const int8_t* geno_sm, const int32_t* csA, const int32_t* animals,
                               int64_t n_pred, const SlabPlan& p, double* vscr, const ReliabFixed& fx, double* rel,
                               hipStream_t s) {
  if (c.B < 1 || n_pred < 1) return hipSuccess;
  const FixedDesign& f = fx.f;
  if (!fx.sbuf || !fx.cf || !fx.ks || !fx.qa || !fx.ga || !f.share || f.nc < 0 || f.nc > COVAR_W || f.L < 1 ||
      f.Cw < RELIAB_W || f.Cw > FIXED_MAX || f.Cw % RELIAB_W != 0)
    return hipErrorInvalidValue;
  using Kern = decltype(&k_reliab<FORM_DUAL, false, ADJ_FIX>);
  const Kern kern[4] = {k_reliab<FORM_DUAL, false, ADJ_FIX>, k_reliab<FORM_DUAL, true, ADJ_FIX>,
                        k_reliab<FORM_PRIMAL, false, ADJ_FIX>, k_reliab<FORM_PRIMAL, true, ADJ_FIX>};
  const auto launch = [&](Kern k, dim3 grid, size_t shm, int64_t s0, int64_t sn) {
    hipLaunchKernelGGL(k, grid, dim3(RTH), shm, s, c, geno_sm, csA, animals, n_pred, s0, sn, vscr, fx, rel);
  };
  return launch_slabs(kern, c, p, vscr, (n_pred + RELIAB_W - 1) / RELIAB_W, launch);
}

hipError_t launch_cov_cov(const double* cf, const double* ks, int64_t B, int n_cov, double* cc, hipStream_t s) {
  if (B < 1) return hipSuccess;
  if (!cf || !ks || !cc || n_cov < 1 || n_cov > COVAR_W || B > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cov_cov, dim3((unsigned)B), dim3(COVAR_W * COVAR_W), 0, s, cf, ks, n_cov, cc);
  return hipGetLastError();
}

}  // namespace tblup
