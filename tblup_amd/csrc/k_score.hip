// Mixed-model score statistics of candidate SNPs (tblup_snp_score_batch): for every listed column j of
// the panel, in or out of the model, from the Cholesky factor M = L L^T, the inverted diagonal tiles
// X_J = L_JJ^{-1} and z = L^{-1} rhs that the chunk's pipeline left in the workspace (what k_reliab and
// k_loglik read; neither solve kernel writes them),
//   score u = w_j^T V^{-1} r_t,   info v = w_j^T V^{-1} w_j,   q = r_t^T V^{-1} r_t,
// V = W_T W_T^T / d + lambda I, w_j = x_T,j - c_j (c_j the exact allele count of column j over the
// branch's reference rows -- all n animals for gblup, the train rows for snp -- divided once by their
// number), r_t = y_T,t - mu_t (mu = 0 for gblup, mean(y_T) for snp).
//   kernel form (M = V, rhs = r):                      s_j = L^{-1} w_j;  u = s_j.z_t,  v = s_j.s_j,  q = |z_t|^2
//   SNP form (M = W_T^T W_T / d + lambda I_k, rhs = W_T^T r / d; snp batches only, choose_sys):
//     g_j = W_T^T w_j,  s_j = L^{-1} g_j;  u = (w_j.r_t - s_j.z_t) / lambda,
//     v = (w_j.w_j - s_j.s_j / d) / lambda,  q = (r^T r - d |z|^2) / lambda   (Woodbury)
// It is k_reliab transposed: SNP columns as right-hand sides in the kernel form, their products with the
// model's columns in the SNP form.
//
// One 512-thread workgroup per (model, slab of SCORE_W = 16 listed SNPs); workgroups are independent
// (no flags, no atomics, every loop bounded by the system's shape).
//   phase 1: the slab's right-hand sides R [ns][16] into V, from the split's 2-bit packed SNP-major rows
//     (a column over the train rows is contiguous).  Kernel form: the 16 columns unpacked and centred,
//     zero at padding rows.  SNP form: the exact counts (A_T^T x_j)_i on int8 MFMA
//     (v_mfma_i32_16x16x64_i8), both operands unpacked from 16-B reads of the packed rows on the way
//     (unpack16: the same animal order in every row), then cnt_ij - sT_i sT_j / n_T in fp64; w_j.w_j from exact integer
//     sums (popcounts of the packed row); w_j.r_t one fma chain over the train rows in order, per trait.
//   phase 2 (fwd_subst.h): k_reliab's blocked forward substitution on fp64 MFMA, the same ring and tile
//     order.  Every lane adds s^2 of its four rows of every block row to a running sum; s.z_t is one pass
//     over the solved V, 32 lanes per SNP, each over a fixed strided subset of the rows in order.  The 32
//     partial sums of a SNP are added in a fixed order at the end.
// So a (model, SNP) value is a function of the column and the system alone: not of n_cand, of its place
// in the list, of its slab, of the batch or of the chunking.  q is written by the model's first slab.
// V lives in LDS when ns x 16 doubles fit (SlabPlan::lds: ns <= 1024), else in a workspace slice of the
// workgroup's own -- the same arithmetic in the same order.
// NaN for every output of a model with d = 0 or a flagged index; a column that is constant over the
// reference rows has w_j = 0 and gives u = v = 0 exactly.
//
// COV instances (tblup_snp_score_cov_batch): the statistics of the model with fixed-effect covariates Q~ that
// k_covar fits, from what its keep mode left in the workspace -- S = L^{-1} R of the covariates, the factor C of
// G = Q~_T^T V^{-1} Q~_T, C^{-1} h_t and {log|G|, bad flag, h_t^T b_t}:
//   a_j = Q~_T^T V^{-1} w_j:  kernel form S^T s_j;  SNP form (Q~_T^T x_T,j - S^T s_j / d) / lambda
//   u_P = u - (C^{-1} a_j).(C^{-1} h_t),  v_P = v - |C^{-1} a_j|^2,  q_P = q - h_t^T b_t
// behind phase 2, with the same sums for u, v, q as the plain instances:
//   T = S^T s for the slab's 16 SNPs on fp64 MFMA, wave q over the 4-row groups pad / 4 + q, + 8, .. of the real
//     rows in order (S from global / L2: a model's slabs share an XCD), the 8 tiles added in wave order in LDS;
//   SNP form: Q~_T^T x_T,j one fma chain over the train rows in order per (covariate, SNP), 256 threads;
//   one lane per SNP: a_j, C y = a_j column by column, u_P and v_P; v_P <= COVAR_PIV_RTOL v gives exact zeros.
// The staging reuses part (tiles, Q~^T x) and ired (C, C^{-1} h_t): no static LDS beyond the plain instances'.
// NaN also for a model whose G has no positive pivot and for N - r - c <= 0.
//
// FIX instances (tblup_snp_score_group_batch): the same statistics for the wide fixed design F~ = [Q~, Z~] of up to
// FIXED_MAX = 128 columns that k_fixed.hip fits, from what k_fixed_subst and k_fixed_gls (keep mode) left in the
// workspace -- S slab-major [Cw / 16][ns][16], C [Cw][Cw], C^{-1} h_t and {log|G|, bad flag, h_t^T b_t}.  Phase 1,
// the substitution and the sums for u, v, q are the plain instances'; behind them, for the model's own Cm columns:
//   T = S^T s, Cm x 16, on fp64 MFMA: wave q takes the design's column slab q over all real 4-row groups in order, so
//     the waves' tiles are T itself and nothing is summed across waves;
//   thread (SNP, r of 32) holds a_j at the columns r, r + 32, ..; SNP form: its own entries of F~_T^T x_T,j -- a
//     covariate's the COV chain, a level's the exact allele count of SNP j over the level's train animals (lst /
//     lpos) minus the level's share of the SNP's train sum, integers and one fp64 combination: all levels together
//     one pass over n_T per SNP;
//   C y = a_j column by column: the owner of row k hands y_k to the SNP's 32 threads through a double-buffered LDS
//     slot (one barrier a column), every thread updates its rows below k with its column of C streamed from
//     global / L2 a step ahead; thread (SNP, 0) takes y.y and y.(C^{-1} h_t) on the way, one chain over the model's
//     columns in order; v_P <= COVAR_PIV_RTOL v gives exact zeros.
// The staging reuses part (T) and ired (C^{-1} h_t); 256 bytes of static LDS (the column slot) come on top, in these
// instances only.  NaN as the COV instances, with Cm in place of c.
#include <algorithm>
#include <type_traits>

#include "fwd_subst.h"
#include "i8_tile.h"

namespace tblup {

namespace {

constexpr int STH = FWD_TH;
constexpr int SPARTS = STH / SCORE_W;   // threads per listed SNP in phase 1
constexpr int SKC = 8;                  // SNP form: 16-B loads per operand in flight in the count products
static_assert(SCORE_W == FWD_W, "a slab is the substitution's 16 right-hand sides");
static_assert(SCORE_W * MAXT == 64, "w.r chains: one wave, one lane per (SNP, trait)");

// ADJ: the fixed effects the statistics are adjusted for, and the struct that carries them
// (plain ints: an unnamed enum in the kernel's signature is mangled differently by the host and the device pass)
constexpr int ADJ_NONE = 0, ADJ_COV = 1, ADJ_FIX = 2;
template <int ADJ>
using ScoreAdj = std::conditional_t<ADJ == ADJ_FIX, ScoreFixed, ScoreCov>;

template <int FORM, bool VLDS, int ADJ>
__global__ __launch_bounds__(STH) void k_snpscore(CholLaunch c, const int32_t* __restrict__ csA,
                                                  const int32_t* __restrict__ cand, int64_t n_cand, int64_t slab0,
                                                  int64_t nslab, double* __restrict__ vscr, ScoreAdj<ADJ> cv,
                                                  double* __restrict__ score, double* __restrict__ info,
                                                  double* __restrict__ qout) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  __shared__ double part[1 + MAXT][STH];   // s.s and s.z_t partial sums (row 0 again for q's wave sums)
  __shared__ long long ired[SCORE_W][SPARTS];
  __shared__ double ww_s[SCORE_W];             // SNP form: w_j.w_j
  __shared__ double wr_s[MAXT][SCORE_W];       // SNP form: w_j.r_t
  __shared__ int32_t col_s[SCORE_W];
  constexpr int W = SCORE_W;
  const int t = threadIdx.x, l = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6), lc = l & 15, lg = l >> 4;
  // consecutive slabs of a model on one XCD, so that its L tiles are shared in that XCD's L2 (speed only)
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t b = blk / nslab, sl = slab0 + blk % nslab;
  const int64_t ns = c.sd.ns, nT = c.d.nT, nTp = c.d.nTp;
  const int NT = c.sd.NT, nt = c.d.nt;
  double* V;
  if constexpr (VLDS) V = dyn;
  else V = vscr + (int64_t)blockIdx.x * ns * W;
  const double* sc = c.scal + b * SCAL;
  const double lam = sc[SC_LAM], dd = sc[SC_D];
  const int64_t pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const bool gblup = (int)sc[SC_MODE] == 1;
  const int fo = fold_of(c.ft, b);
  const int32_t* cs = gblup ? csA : c.ft.csT[fo];
  const double N = gblup ? (double)c.d.n : (double)nT;
  const uint8_t* gp = c.ft.gpk[fo];
  // block rows that hold real system rows (the rest is identity padding with zero right-hand sides)
  const int J0 = (int)(pad / TILE), J1 = (int)((pad + nrow + TILE - 1) / TILE);
  // phase 1 thread map: SNP ta of the slab, part tp of SPARTS (a slot past the list repeats its first SNP)
  const int ta = t & (W - 1), tp = t / W;
  const int64_t va = sl * W + ta;
  const int64_t col = cand[va < n_cand ? va : 0];
  const uint32_t* crow = reinterpret_cast<const uint32_t*>(gp + col * c.gpk_row);   // 16 animals per dword
  const double cj = (double)cs[col] / N;

  if constexpr (FORM == FORM_DUAL) {
    // rows = the train animals in split order: dword g of the packed row holds rows 16g .. 16g+15
    for (int64_t g = (int64_t)J0 * (TILE / 16) + tp; g < (int64_t)J1 * (TILE / 16); g += SPARTS) {
      const uint32_t x = crow[g];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t r = 16 * g + e;
        V[r * W + ta] = r < nrow ? (double)((x >> (2 * e)) & 3u) - cj : 0.0;
      }
    }
  } else {
    if (tp == 0) col_s[ta] = (int32_t)col;
    // x_j.x_j over the train rows (the padding animals are zero): genotype g = lo + 2 hi, g^2 = lo + 4 hi
    long long sxx = 0;
    for (int64_t g = tp; g < nTp / 16; g += SPARTS) {
      const uint32_t x = crow[g];
      sxx += __builtin_popcount(x & 0x55555555u) + 4 * __builtin_popcount((x >> 1) & 0x55555555u);
    }
    ired[ta][tp] = sxx;
    __syncthreads();
    if (t < W) {
      long long s = 0;
      for (int p = 0; p < SPARTS; ++p) s += ired[t][p];
      const double sT = (double)cs[col];
      ww_s[t] = (double)s - sT * sT / N;
    }
    if (q == STH / 64 - 1) {
      // w_j.r_t: lane (SNP lc, trait lg) of the last wave, one chain over the train rows in order
      const int64_t cl = col_s[lc];
      const uint32_t* row = reinterpret_cast<const uint32_t*>(gp + cl * c.gpk_row);
      const double cc = (double)cs[cl] / N;
      const int tr = lg < nt ? lg : 0;
      const double* y = c.ft.yT[fo] + (int64_t)tr * nTp;
      const double mu = c.ft.ymu[fo][tr];
      // (16 rows per step, the next step's loads in flight under the step's chain; y is zero-padded to
      // nTp, and a padding row adds nothing)
      double acc = 0.0;
      double ya[16], yb[16];
      uint32_t xa, xb;
      auto ld = [&](double (&yv)[16], uint32_t& x, int64_t g) {
        x = row[g];
#pragma unroll
        for (int e = 0; e < 16; ++e) yv[e] = y[16 * g + e];
      };
      auto use = [&](const double (&yv)[16], uint32_t x, int ne) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const double a = __builtin_fma((double)((x >> (2 * e)) & 3u) - cc, yv[e] - mu, acc);
          acc = e < ne ? a : acc;
        }
      };
      const int64_t nfull = nT / 16, ngr = (nT + 15) / 16;
      const int tail = (int)(nT % 16);
      ld(ya, xa, 0);
      for (int64_t g = 0; g < nfull; g += 2) {
        if (g + 1 < ngr) ld(yb, xb, g + 1);
        use(ya, xa, 16);
        if (g + 1 < nfull) {
          if (g + 2 < ngr) ld(ya, xa, g + 2);
          use(yb, xb, 16);
        }
      }
      if (tail) {   // the last, partial step sits in the buffer its parity names
        if (nfull & 1) use(yb, xb, tail);
        else use(ya, xa, tail);
      }
      wr_s[lg][lc] = acc;
    }
    // counts: system rows 16 rb .. 16 rb + 15 (the model's columns; a padding row reads the zero row P)
    // against the slab's 16 columns, 64 train animals per MFMA
    const int64_t o0 = c.off[b], P = c.d.P;
    const double* ub = c.u + b * c.sd.prow;   // sT_i at system row i
    const double sTj = (double)cs[col_s[lc]];
    const uint8_t* brow = gp + (int64_t)col_s[lc] * c.gpk_row + 16 * lg;
    // Lane (lc, lg) loads 16 B of its row per step: bytes 64 k + 16 lg .. + 15 of the packed row, i.e. four
    // dwords of 16 animals each, and MFMA i of the step contracts dword i of every lane -- 64 animals per
    // MFMA, 256 per step, both operands in the same animal order (integer sums: any order, the same
    // bits).  A row block's loads are issued together; the next block's column index is fetched under
    // the current block's products.  The last step of a train part of 128 x odd animals covers only
    // 32 B of it: its lanes lg >= 2 (which would read the validation animals) contribute zero.
    auto col_of = [&](int64_t rb) -> int64_t {
      const int64_t ar = 16 * rb + lc;
      return sys_real(ar, pad, nrow) ? snp_col(c.idx[o0 + ar - pad], P) : P;
    };
    const int nst = (int)((nTp / 4 + 63) / 64);           // 64-B steps of the train part
    const bool cut = (nTp / 4) % 64 != 0 && lg >= 2;       // this lane is past the train part in the last step
    const v4i zero4 = {0, 0, 0, 0};
    const int64_t rb1 = (int64_t)J1 * (TILE / 16);
    // (the row blocks go round the waves that do not run the w.r chains)
    constexpr int CW = STH / 64 - 1;
    int64_t rb = q < CW ? (int64_t)J0 * (TILE / 16) + q : rb1;
    int64_t acol = rb < rb1 ? col_of(rb) : P;
    for (; rb < rb1; rb += CW) {
      const uint8_t* arow = gp + acol * c.gpk_row + 16 * lg;
      if (rb + CW < rb1) acol = col_of(rb + CW);
      v4i acc = {0, 0, 0, 0};
      for (int k0 = 0; k0 < nst; k0 += SKC) {
        v4i aq[SKC], bq[SKC];
#pragma unroll
        for (int e = 0; e < SKC; ++e) {
          const int k = k0 + e < nst ? k0 + e : k0;   // (a slot past the end repeats step k0, then dropped)
          aq[e] = *reinterpret_cast<const v4i*>(arow + 64 * k);
          bq[e] = *reinterpret_cast<const v4i*>(brow + 64 * k);
        }
#pragma unroll
        for (int e = 0; e < SKC; ++e)
          if (k0 + e < nst) {
            const bool drop = cut && k0 + e == nst - 1;
            const v4i av = drop ? zero4 : aq[e];
#pragma unroll
            for (int i = 0; i < 4; ++i)
              acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(unpack16((uint32_t)av[i]), unpack16((uint32_t)bq[e][i]), acc, 0,
                                                          0, 0);
          }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = 16 * rb + 4 * lg + r;
        V[row * W + lc] = sys_real(row, pad, nrow) ? (double)acc[r] - ub[row] * sTj / N : 0.0;
      }
    }
  }
  __syncthreads();

  // phase 2: V_J = X_J (R_J - sum_{L<J} L_JL V_L), with s.s on the way
  const double* Lb = c.L + b * l_stride(NT);
  const double* Db = c.Dinv + b * (int64_t)NT * NPACK * BLKD;
  const double* zb = c.z + b * nt * ns;
  double nacc = 0.0;
  fwd_subst16(Lb, Db, V, NT, J0, J1, pad, q, lc, lg, [&](int, double v) { nacc = __builtin_fma(v, v, nacc); });
  // s.z_t over the real rows from the solved V (thread (ta, tp): rows pad + tp, pad + tp + 32, .. in order)
  double zacc[MAXT] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int64_t r = pad + tp; r < pad + nrow; r += SPARTS) {
    const double v = V[r * W + ta];
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr)
      if (tr < nt) zacc[tr] = __builtin_fma(v, zb[(int64_t)tr * ns + r], zacc[tr]);
  }
  part[0][t] = nacc;
#pragma unroll
  for (int tr = 0; tr < MAXT; ++tr) part[1 + tr][t] = zacc[tr];
  __syncthreads();
  bool dead = !(dd > 0.0) || sc[SC_BAD] != 0.0;
  const double nan = __builtin_nan("");
  const bool fin = t < W && sl * W + t < n_cand;   // this lane finishes a listed SNP
  if constexpr (ADJ == ADJ_NONE) {
    if (fin) {
      double s2 = 0.0, sz[MAXT] = {0.0, 0.0, 0.0, 0.0};
      for (int w = 0; w < STH / 64; ++w)
        for (int g = 0; g < 4; ++g) {
          s2 += part[0][64 * w + 16 * g + t];
#pragma unroll
          for (int tr = 0; tr < MAXT; ++tr) sz[tr] += part[1 + tr][64 * w + 16 * g + t];
        }
      double v;
      if constexpr (FORM == FORM_PRIMAL) v = (ww_s[t] - s2 / dd) / lam;
      else v = s2;
      info[b * n_cand + sl * W + t] = dead ? nan : v;
      for (int tr = 0; tr < nt; ++tr) {
        double u;
        if constexpr (FORM == FORM_PRIMAL) u = (wr_s[tr][t] - sz[tr]) / lam;
        else u = sz[tr];
        score[(b * nt + tr) * n_cand + sl * W + t] = dead ? nan : u;
      }
    }
  } else if constexpr (ADJ == ADJ_COV) {
    // the plain statistics of this lane's SNP, the same sums
    double v = 0.0, u[MAXT] = {0.0, 0.0, 0.0, 0.0};
    if (fin) {
      double s2 = 0.0, sz[MAXT] = {0.0, 0.0, 0.0, 0.0};
      for (int w = 0; w < STH / 64; ++w)
        for (int g = 0; g < 4; ++g) {
          s2 += part[0][64 * w + 16 * g + t];
#pragma unroll
          for (int tr = 0; tr < MAXT; ++tr) sz[tr] += part[1 + tr][64 * w + 16 * g + t];
        }
      if constexpr (FORM == FORM_PRIMAL) v = (ww_s[t] - s2 / dd) / lam;
      else v = s2;
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr) {
        if constexpr (FORM == FORM_PRIMAL) u[tr] = (wr_s[tr][t] - sz[tr]) / lam;
        else u[tr] = sz[tr];
      }
    }
    // The covariates' share: a_j = Q~_T^T V^{-1} w_j from T = S^T s_j (S = L^{-1} R of the covariates, k_covar's),
    // then C y = a_j and v_P = v - y.y, u_P = u - y.(C^{-1} h_t).
    // T for the slab's 16 SNPs on fp64 MFMA, rows of S (global / L2) against the same rows of the solved V:
    // wave q takes the 4-row groups pad / 4 + q, + 8, .. of the real rows in order (a function of the
    // system alone); a row outside them counts as zero.
    const double* ks = cv.ks + b * COVAR_KS;
    dead = dead || ks[KS_BAD] != 0.0 || !((double)nT - sc[SC_MUF] - (double)cv.nc > 0.0);
    const double* sq = cv.sq + b * ns * W;
    v4d tacc = {0.0, 0.0, 0.0, 0.0};
    const int64_t g1 = (pad + nrow + 3) / 4;
    // (TKC groups per step, their loads issued together; a slot past the last group multiplies zeros)
    constexpr int TKC = 16;
    for (int64_t g0 = pad / 4 + q; g0 < g1; g0 += TKC * (STH / 64)) {
      double sa[TKC], sv[TKC];
#pragma unroll
      for (int e = 0; e < TKC; ++e) {
        const int64_t g = g0 + e * (STH / 64), r = 4 * g + lg;
        sa[e] = g < g1 && sys_real(r, pad, nrow) ? sq[r * W + lc] : 0.0;
        sv[e] = g < g1 ? V[r * W + lc] : 0.0;
      }
#pragma unroll
      for (int e = 0; e < TKC; ++e) tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa[e], sv[e], tacc, 0, 0, 0);
    }
    // SNP form: (Q~_T^T x_T,j)_i, thread (covariate i = t / 16, SNP ta): one chain over the train rows in
    // order, the genotypes unpacked from the packed row (Q~_T sums to zero there: w_j's centre drops out)
    double qx = 0.0;
    if constexpr (FORM == FORM_PRIMAL) {
      if (t < W * W && tp < cv.nc) {
        const double* qi = cv.qT + (gblup ? 0 : (int64_t)W * nTp) + (int64_t)tp * nTp;
        // (16 rows per step, the next step's loads in flight under the step's chain, as the w.r chains of
        // phase 1; a padding row has genotype and covariate zero and adds nothing)
        double qa[16], qb[16];
        uint32_t xa, xb;
        auto ld = [&](double (&qv)[16], uint32_t& x, int64_t g) {
          x = crow[g];
#pragma unroll
          for (int e = 0; e < 16; ++e) qv[e] = qi[16 * g + e];
        };
        auto use = [&](const double (&qv)[16], uint32_t x) {
#pragma unroll
          for (int e = 0; e < 16; ++e) qx = __builtin_fma((double)((x >> (2 * e)) & 3u), qv[e], qx);
        };
        const int64_t ng = nTp / 16;
        ld(qa, xa, 0);
        for (int64_t g = 0; g < ng; g += 2) {
          if (g + 1 < ng) ld(qb, xb, g + 1);
          use(qa, xa);
          if (g + 1 < ng) {
            if (g + 2 < ng) ld(qa, xa, g + 2);
            use(qb, xb);
          }
        }
      }
    }
    // staging in the buffers the sums above are done with: the waves' tiles and Q~^T x in part, C and
    // C^{-1} h_t in ired
    double* tps = &part[0][0];
    double* cfs = reinterpret_cast<double*>(&ired[0][0]);
    static_assert(sizeof(part) >= (STH / 64 + 1) * W * W * 8 && sizeof(ired) >= (W * W + MAXT * W) * 8,
                  "the covariates' staging fits part / ired");
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) tps[q * W * W + (lg + 4 * r) * W + lc] = tacc[r];   // tile element [covariate][SNP]
    if (t < W * W) {
      tps[(STH / 64) * W * W + t] = qx;
      cfs[t] = cv.cf[b * W * W + t];
    } else if (t < W * W + MAXT * W) {
      cfs[t] = cv.ch[b * MAXT * W + t - W * W];
    }
    __syncthreads();
    if (fin) {
      double a[W];
#pragma unroll
      for (int i = 0; i < W; ++i) {
        double T = 0.0;
        for (int w = 0; w < STH / 64; ++w) T += tps[w * W * W + i * W + t];
        if constexpr (FORM == FORM_PRIMAL) a[i] = (tps[(STH / 64) * W * W + i * W + t] - T / dd) / lam;
        else a[i] = T;
        if (i >= cv.nc) a[i] = 0.0;
      }
      // C y = a_j (k_covar's own substitution: column by column), y.y and y.(C^{-1} h_t) on the way
      double yy = 0.0, yh[MAXT] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double yk = a[k] / cfs[k * W + k];
#pragma unroll
        for (int i = k + 1; i < W; ++i) a[i] = __builtin_fma(-cfs[i * W + k], yk, a[i]);
        yy = __builtin_fma(yk, yk, yy);
#pragma unroll
        for (int tr = 0; tr < MAXT; ++tr) yh[tr] = __builtin_fma(yk, cfs[W * W + tr * W + k], yh[tr]);
      }
      // a SNP in the span of the covariates (or constant over the reference rows): exact zeros
      const double vp = v - yy;
      const bool span = !(vp > COVAR_PIV_RTOL * v);
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr) u[tr] = span ? 0.0 : u[tr] - yh[tr];
      v = span ? 0.0 : vp;
      info[b * n_cand + sl * W + t] = dead ? nan : v;
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr)
        if (tr < nt) score[(b * nt + tr) * n_cand + sl * W + t] = dead ? nan : u[tr];
    }
  } else {
    // the plain statistics of this lane's SNP, the same sums
    double v = 0.0, u[MAXT] = {0.0, 0.0, 0.0, 0.0};
    if (fin) {
      double s2 = 0.0, sz[MAXT] = {0.0, 0.0, 0.0, 0.0};
      for (int w = 0; w < STH / 64; ++w)
        for (int g = 0; g < 4; ++g) {
          s2 += part[0][64 * w + 16 * g + t];
#pragma unroll
          for (int tr = 0; tr < MAXT; ++tr) sz[tr] += part[1 + tr][64 * w + 16 * g + t];
        }
      if constexpr (FORM == FORM_PRIMAL) v = (ww_s[t] - s2 / dd) / lam;
      else v = s2;
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr) {
        if constexpr (FORM == FORM_PRIMAL) u[tr] = (wr_s[tr][t] - sz[tr]) / lam;
        else u[tr] = sz[tr];
      }
    }
    // The wide design's share: a_j = F~_T^T V^{-1} w_j for the model's Cm columns, C y = a_j, and the COV
    // instances' u_P, v_P.
    const FixedDesign& f = cv.f;
    const int Cw = f.Cw;
    const int Cm = std::min(fixed_cols(gblup, f.nc, f.L), Cw), nb = (Cm + W - 1) / W;
    const double* ks = cv.ks + b * COVAR_KS;
    dead = dead || ks[KS_BAD] != 0.0 || !((double)nT - sc[SC_MUF] - (double)Cm > 0.0);
    // T = S^T s, Cm x 16, on fp64 MFMA: wave q takes the design's column slab q (S slab-major: the slab's [ns][16]
    // from global / L2) over all 4-row groups of the real rows in order, so its tile is rows 16 q .. 16 q + 15 of T
    // itself; a row outside the real ones counts as zero.
    v4d tacc = {0.0, 0.0, 0.0, 0.0};
    if (q < nb) {
      const double* sq = cv.sbuf + (b * (Cw / W) + q) * ns * W;
      const int64_t g1 = (pad + nrow + 3) / 4;
      // (TKC groups per step, their loads issued together; a slot past the last group multiplies zeros)
      constexpr int TKC = 16;
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
    // staging in the buffers the sums above are done with: T in part, C^{-1} h_t in ired
    __shared__ double ycol[2][W];   // the solve's current column of y, double-buffered
    double* tps = &part[0][0];
    double* chs = reinterpret_cast<double*>(&ired[0][0]);
    static_assert(sizeof(part) >= FIXED_MAX * W * 8 && sizeof(ired) >= MAXT * FIXED_MAX * 8 &&
                      STH == MAXT * FIXED_MAX && STH / 64 * W >= FIXED_MAX,
                  "the wide design's staging fits part / ired; a wave per column slab");
    __syncthreads();
    if (q < nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) tps[(W * q + lg + 4 * r) * W + lc] = tacc[r];   // T[column][SNP]
    }
    {
      const int tr = t / FIXED_MAX, i = t % FIXED_MAX;
      chs[t] = i < Cw ? cv.ch[(b * MAXT + tr) * Cw + i] : 0.0;
    }
    __syncthreads();
    // Thread (SNP ta, tp) holds a_j at the columns tp, tp + 32, .. (FIXED_MAX / SPARTS of them).  SNP form:
    // a = (F~_T^T x_T,j - T / d) / lambda with F~_T^T x_T,j the thread's own: a covariate's (tp < nc, the COV
    // instances' chain over the train rows in order), a level's the exact allele count of SNP j over the level's
    // train animals (lst / lpos; integers: any order) minus the level's share of the SNP's train sum -- k_fixed_subst's
    // right-hand side.  F~_T sums to zero over the train rows there: w_j's centre drops out.
    constexpr int NR = FIXED_MAX / SPARTS;
    double a[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      const int i = tp + SPARTS * m;
      a[m] = i < Cm ? tps[i * W + ta] : 0.0;
    }
    if constexpr (FORM == FORM_PRIMAL) {
      double qx = 0.0;
      if (tp < f.nc) {
        const double* qi = f.qT + (gblup ? 0 : (int64_t)COVAR_W * nTp) + (int64_t)tp * nTp;
        double qa[16], qb[16];
        uint32_t xa, xb;
        auto ld = [&](double (&qv)[16], uint32_t& x, int64_t g) {
          x = crow[g];
#pragma unroll
          for (int e = 0; e < 16; ++e) qv[e] = qi[16 * g + e];
        };
        auto use = [&](const double (&qv)[16], uint32_t x) {
#pragma unroll
          for (int e = 0; e < 16; ++e) qx = __builtin_fma((double)((x >> (2 * e)) & 3u), qv[e], qx);
        };
        const int64_t ng = nTp / 16;
        ld(qa, xa, 0);
        for (int64_t g = 0; g < ng; g += 2) {
          if (g + 1 < ng) ld(qb, xb, g + 1);
          use(qa, xa);
          if (g + 1 < ng) {
            if (g + 2 < ng) ld(qa, xa, g + 2);
            use(qb, xb);
          }
        }
      }
      const uint8_t* xb8 = reinterpret_cast<const uint8_t*>(crow);
      const double sTj = (double)cs[col];
#pragma unroll
      for (int m = 0; m < NR; ++m) {
        const int i = tp + SPARTS * m;
        double fx = qx;   // (a covariate's column has m = 0)
        if (i >= f.nc && i < Cm) {
          const int lev = i - f.nc + (gblup ? 0 : 1);
          const int p1 = f.lst[lev + 1];
          int cnt = 0, p = f.lst[lev];
          for (; p + 4 <= p1; p += 4) {
            int an[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) an[e] = f.lpos[p + e];
#pragma unroll
            for (int e = 0; e < 4; ++e) cnt += (xb8[an[e] >> 2] >> (2 * (an[e] & 3))) & 3;
          }
          for (; p < p1; ++p) {
            const int an = f.lpos[p];
            cnt += (xb8[an >> 2] >> (2 * (an & 3))) & 3;
          }
          fx = (double)cnt - sTj * (gblup ? 0.0 : f.share[lev]);
        }
        a[m] = i < Cm ? (fx - a[m] / dd) / lam : 0.0;
      }
    }
    // C y = a_j column by column (k_fixed_gls's substitution), C streamed from global / L2 a column ahead: the owner
    // of row k hands y_k to the SNP's other threads through LDS, every thread updates its rows below k; thread
    // (SNP ta, 0) takes y.y and y.(C^{-1} h_t) on the way, one chain over the model's columns in order
    const double* Cb = cv.cf + b * (int64_t)Cw * Cw;
    double yy = 0.0, yh[MAXT] = {0.0, 0.0, 0.0, 0.0};
    double cn[NR];
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      const int i = tp + SPARTS * m;
      cn[m] = i < Cm ? Cb[(int64_t)i * Cw] : 0.0;
    }
    for (int k = 0; k < Cm; ++k) {
      double cc[NR];
#pragma unroll
      for (int m = 0; m < NR; ++m) {
        const int i = tp + SPARTS * m;
        cc[m] = cn[m];
        cn[m] = (i > k && i < Cm) ? Cb[(int64_t)i * Cw + k + 1] : 0.0;
      }
      if (tp == k % SPARTS) {
        double ak = 0.0, ckk = 1.0;
#pragma unroll
        for (int m = 0; m < NR; ++m)
          if (m == k / SPARTS) ak = a[m], ckk = cc[m];
        ycol[k & 1][ta] = ak / ckk;
      }
      __syncthreads();
      const double yk = ycol[k & 1][ta];
#pragma unroll
      for (int m = 0; m < NR; ++m) {
        const int i = tp + SPARTS * m;
        if (i > k && i < Cm) a[m] = __builtin_fma(-cc[m], yk, a[m]);
      }
      if (tp == 0) {
        yy = __builtin_fma(yk, yk, yy);
#pragma unroll
        for (int tr = 0; tr < MAXT; ++tr) yh[tr] = __builtin_fma(yk, chs[tr * FIXED_MAX + k], yh[tr]);
      }
    }
    if (fin) {
      // a SNP in the span of the design (or constant over the reference rows): exact zeros
      const double vp = v - yy;
      const bool span = !(vp > COVAR_PIV_RTOL * v);
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr) u[tr] = span ? 0.0 : u[tr] - yh[tr];
      v = span ? 0.0 : vp;
      info[b * n_cand + sl * W + t] = dead ? nan : v;
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr)
        if (tr < nt) score[(b * nt + tr) * n_cand + sl * W + t] = dead ? nan : u[tr];
    }
  }
  if (sl != 0 || !qout) return;

  // q of the model, by its first slab: |z_t|^2 over the real rows (SNP form: and r_t.r_t over the train rows)
  __syncthreads();
  double zz[MAXT] = {0.0, 0.0, 0.0, 0.0}, yy[MAXT] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = pad + t; r < pad + nrow; r += STH)
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr)
      if (tr < nt) {
        const double zv = zb[(int64_t)tr * ns + r];
        zz[tr] = __builtin_fma(zv, zv, zz[tr]);
      }
  if constexpr (FORM == FORM_PRIMAL) {
    for (int64_t r = t; r < nT; r += STH)
#pragma unroll
      for (int tr = 0; tr < MAXT; ++tr)
        if (tr < nt) {
          const double yc = c.ft.yT[fo][(int64_t)tr * nTp + r] - c.ft.ymu[fo][tr];
          yy[tr] = __builtin_fma(yc, yc, yy[tr]);
        }
  }
  // every lane a fixed strided subset of the rows, the wave sum a fixed-order xor butterfly, the waves'
  // partials added in wave order (k_loglik's reduction)
#pragma unroll
  for (int tr = 0; tr < MAXT; ++tr) {
    double a = zz[tr], y = yy[tr];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o);
      y += __shfl_xor(y, o);
    }
    if (l == 0) {
      part[0][2 * MAXT * q + tr] = a;
      part[0][2 * MAXT * q + MAXT + tr] = y;
    }
  }
  __syncthreads();
  if (t < nt) {
    double szz = 0.0, syy = 0.0;
    for (int w = 0; w < STH / 64; ++w) {
      szz += part[0][2 * MAXT * w + t];
      syy += part[0][2 * MAXT * w + MAXT + t];
    }
    double qv;
    if constexpr (FORM == FORM_PRIMAL) qv = (syy - dd * szz) / lam;
    else qv = szz;
    if constexpr (ADJ != ADJ_NONE) qv = qv - cv.ks[b * COVAR_KS + KS_HB + t];   // q_P = q - h_t^T b_t
    qout[b * nt + t] = dead ? nan : qv;
  }
}

// the list's slabs through the <FORM, VLDS> instance of mode ADJ that the chunk and the plan select
template <int ADJ>
hipError_t launch_adj(const CholLaunch& c, const int32_t* csA, const int32_t* cand, int64_t n_cand, const SlabPlan& p,
                      double* vscr, const ScoreAdj<ADJ>& cv, double* score, double* info, double* q, hipStream_t s) {
  using Kern = decltype(&k_snpscore<FORM_DUAL, false, ADJ>);
  const Kern kern[4] = {k_snpscore<FORM_DUAL, false, ADJ>, k_snpscore<FORM_DUAL, true, ADJ>,
                        k_snpscore<FORM_PRIMAL, false, ADJ>, k_snpscore<FORM_PRIMAL, true, ADJ>};
  const auto launch = [&](Kern k, dim3 grid, size_t shm, int64_t s0, int64_t sn) {
    hipLaunchKernelGGL(k, grid, dim3(STH), shm, s, c, csA, cand, n_cand, s0, sn, vscr, cv, score, info, q);
  };
  return launch_slabs(kern, c, p, vscr, (n_cand + SCORE_W - 1) / SCORE_W, launch);
}

}  // namespace

hipError_t launch_snpscore(const CholLaunch& c, const int32_t* csA, const int32_t* cand, int64_t n_cand,
                           const SlabPlan& p, double* vscr, const ScoreCov* cov, double* score, double* info,
                           double* q, hipStream_t s) {
  if (c.B < 1 || n_cand < 1) return hipSuccess;
  if (c.d.nt < 1 || c.d.nt > MAXT) return hipErrorInvalidValue;
  if (cov && (!cov->sq || !cov->cf || !cov->ch || !cov->ks || !cov->qT || cov->nc < 1 || cov->nc > COVAR_W))
    return hipErrorInvalidValue;
  if (cov) return launch_adj<ADJ_COV>(c, csA, cand, n_cand, p, vscr, *cov, score, info, q, s);
  return launch_adj<ADJ_NONE>(c, csA, cand, n_cand, p, vscr, ScoreCov{}, score, info, q, s);
}

hipError_t launch_snpscore_fixed(const CholLaunch& c, const int32_t* csA, const int32_t* cand, int64_t n_cand,
                                 const SlabPlan& p, double* vscr, const ScoreFixed& fx, double* score, double* info,
                                 double* q, hipStream_t s) {
  if (c.B < 1 || n_cand < 1) return hipSuccess;
  if (c.d.nt < 1 || c.d.nt > MAXT) return hipErrorInvalidValue;
  const FixedDesign& f = fx.f;
  if (!fx.sbuf || !fx.cf || !fx.ch || !fx.ks || !f.qT || !f.lst || !f.lpos || !f.share || f.nc < 0 || f.nc > COVAR_W ||
      f.L < 1 || f.Cw < SCORE_W || f.Cw > FIXED_MAX || f.Cw % SCORE_W != 0)
    return hipErrorInvalidValue;
  return launch_adj<ADJ_FIX>(c, csA, cand, n_cand, p, vscr, fx, score, info, q, s);
}

}  // namespace tblup
