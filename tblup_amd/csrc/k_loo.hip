// Leave-one-out cross-validation of fitted models (tblup_loo_batch): every training animal t of the split
// predicted by the model fitted without it, from the Cholesky factor L L^T, the inverted diagonal tiles
// X_J = L_JJ^{-1} and the solution alpha = L^{-T} z that the chunk's pipeline and k_effects left in the
// workspace.  With lambda = (1 - h2) / h2, c = 0 under gblup and 1 / n_T under snp (the refitted intercept),
// mu = 0 under gblup and mean(y_T) under snp:
//   SNP form     L L^T = W_T^T W_T / d + lambda I:   h_tt = c + |L^{-1} w_t|^2 / d,  e_t = y_t - mu - w_t . beta,
//                e_loo,t = e_t / (1 - h_tt)
//   kernel form  L L^T = V = K_TT + lambda I:        (V^{-1})_tt = |L^{-1} e_t|^2 (e_t the unit vector),
//                e_loo,t = lambda alpha_t / (lambda (V^{-1})_tt - c),  h_tt = 1 + c - lambda (V^{-1})_tt
//   y^_loo,t = y_t - e_loo,t
// (the two are equal by the Woodbury identity).  The snp branch keeps the fitted model's penalty lambda d and its
// centre; the intercept and the centring are refitted without t (that is what c carries).
//
// k_loo: one 512-thread workgroup per (model, slab of LOO_W = 16 training animals in `train` order); workgroups
// are independent (no flags, no hand-offs, every loop bounded by the system's shape).
//   SNP form: phase 1 is k_reliab's -- the animals' centred rows gathered from the SNP-major int8 panel into
//     V [ns][16]; thread (animal) then takes w_t . beta in one fma chain over j = 0 .. k-1 per trait, before the
//     substitution overwrites V in place.
//   Kernel form: the right-hand sides are the unit columns of the slab's own system rows r0 + i, r0 = 16 slab,
//     so the substitution starts at block row r0 / 128 and skips the leading zero rows in whole 64-row steps
//     (exact: the skipped products are zeros).  No genotype is read.
//   Both: fwd_subst16 (fwd_subst.h) with the running sum of squares in its callback; the 32 partial sums of an
//     animal are added in a fixed order, and the animal's own thread finishes h_tt, e_loo and y^_loo.
// So an animal's values are a function of its genotypes, the phenotypes and the system alone: not of the batch,
// the chunking or the animal's slab.  V lives in LDS when ns x 16 doubles fit (ns <= 1024), else in a workspace
// slice of the workgroup's own -- the same arithmetic in the same order.
//
// k_loo_fitness: one workgroup per (model, trait): PRESS = sum_t e_loo,t^2 and |pearson(y^_loo, y_T)|
// (pearson_dev.h's restatement, the evaluation's NaN rules) over the n_T values in `train` order, fixed-order sums.
#include "fwd_subst.h"
#include "pearson_dev.h"

namespace tblup {

namespace {

constexpr int LTH = FWD_TH;         // 8 waves
constexpr int LPARTS = LTH / LOO_W;
constexpr int LFTH = 256;           // k_loo_fitness
static_assert(LOO_W == FWD_W, "k_loo's slab is the substitution's 16 right-hand sides");

template <int FORM, bool VLDS, int NTR>
__global__ __launch_bounds__(LTH) void k_loo(CholLaunch c, const int8_t* __restrict__ geno,
                                             const int32_t* __restrict__ train, const double* __restrict__ alpha,
                                             int64_t slab0, int64_t nslab, double* __restrict__ vscr,
                                             double* __restrict__ pred, double* __restrict__ lev) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  __shared__ double nrm[LTH];
  __shared__ double wb[MAXT][LOO_W];   // SNP form: w_t . beta per trait
  constexpr int W = LOO_W;
  const int t = threadIdx.x, l = t & 63, q = __builtin_amdgcn_readfirstlane(t >> 6), lc = l & 15, lg = l >> 4;
  // consecutive slabs of a model on one XCD, so that its L tiles are shared in that XCD's L2 (speed only)
  const int64_t blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t b = blk / nslab, sl = slab0 + blk % nslab;
  const int64_t ns = c.sd.ns, n = c.d.n, P = c.d.P, nT = c.d.nT, nTp = c.d.nTp;
  const int NT = c.sd.NT;
  double* V;
  if constexpr (VLDS) V = dyn;
  else V = vscr + (int64_t)blockIdx.x * ns * W;
  const double* sc = c.scal + b * SCAL;
  const double lam = sc[SC_LAM], dd = sc[SC_D], muf = sc[SC_MUF];
  const int64_t kk = (int64_t)sc[SC_K], pad = (int64_t)sc[SC_PAD], nrow = (int64_t)sc[SC_NROW];
  const int fo = fold_of(c.ft, b);
  const double* al = alpha + b * NTR * ns;
  const int J1 = (int)((pad + nrow + TILE - 1) / TILE);
  const int ta = t & (W - 1), tp = t / W;
  const int64_t r0 = sl * W;   // the slab's first animal, by position in `train`
  int J0;
  int64_t lead;   // leading rows of V that are zero

  if constexpr (FORM == FORM_PRIMAL) {
    J0 = (int)(pad / TILE);
    lead = pad;
    const int64_t an = r0 + ta < nT ? train[r0 + ta] : train[0];
    const int32_t* cs = c.ft.csT[fo];
    const double N = (double)nT;
    const int64_t o0 = c.off[b];
    // k_reliab's phase 1 (every row loads -- a padding row the first SNP's values, then dropped -- so that the
    // unrolled loop's loads are in flight together)
#pragma unroll 8
    for (int64_t r = (int64_t)J0 * TILE + tp; r < (int64_t)J1 * TILE; r += LPARTS) {
      const bool real = sys_real(r, pad, nrow);
      const int64_t col = snp_col(c.idx[o0 + (real ? r - pad : 0)], P);
      const double x = (double)geno[col * n + an] - (double)cs[col] / N;
      V[r * W + ta] = real ? x : 0.0;
    }
    __syncthreads();
    if (t < W) {
      double acc[NTR] = {};
#pragma unroll 4
      for (int64_t j = 0; j < kk; ++j) {
        const double x = V[(pad + j) * W + t];
#pragma unroll
        for (int tr = 0; tr < NTR; ++tr) acc[tr] = __builtin_fma(x, al[tr * ns + pad + j], acc[tr]);
      }
#pragma unroll
      for (int tr = 0; tr < NTR; ++tr) wb[tr][t] = acc[tr];
    }
  } else {
    // unit columns: one at system row r0 + i of right-hand side i (none past the train rows)
    J0 = (int)(r0 / TILE);
    lead = r0;
    for (int64_t r = (int64_t)J0 * TILE + tp; r < (int64_t)J1 * TILE; r += LPARTS)
      V[r * W + ta] = (r == r0 + ta && r < nT) ? 1.0 : 0.0;
  }
  __syncthreads();

  const double* Lb = c.L + b * l_stride(NT);
  const double* Db = c.Dinv + b * (int64_t)NT * NPACK * BLKD;
  double nacc = 0.0;
  fwd_subst16(Lb, Db, V, NT, J0, J1, lead, q, lc, lg, [&](int, double v) { nacc = __builtin_fma(v, v, nacc); });
  nrm[t] = nacc;
  __syncthreads();
  if (t < W && r0 + t < nT) {
    const int64_t ti = r0 + t;
    double s2 = 0.0;
    for (int w = 0; w < LTH / 64; ++w)
      for (int g = 0; g < 4; ++g) s2 += nrm[64 * w + 16 * g + t];
    const double cc = muf / (double)nT;
    const bool dead = dd == 0.0 || sc[SC_BAD] != 0.0;
    const double nan = __builtin_nan("");
    // e_loo = num / den.  Every product below is an explicit fma or stands alone, so that no instance (form,
    // traits) contracts what another does not: a trait's bits are the single-trait call's
    double h, den;
    if constexpr (FORM == FORM_PRIMAL) {
      h = cc + s2 / dd;
      den = 1.0 - h;
    } else {
      den = __builtin_fma(lam, s2, -cc);
      h = __builtin_fma(-lam, s2, 1.0 + cc);
    }
    lev[b * nT + ti] = dead ? nan : h;
#pragma unroll
    for (int tr = 0; tr < NTR; ++tr) {
      const double y = c.ft.yT[fo][(int64_t)tr * nTp + ti];
      double num;
      if constexpr (FORM == FORM_PRIMAL) num = (y - c.ft.ymu[fo][tr]) - wb[tr][t];
      else num = lam * al[tr * ns + ti];
      pred[(b * NTR + tr) * nT + ti] = dead ? nan : y - num / den;
    }
  }
}

__global__ __launch_bounds__(LFTH) void k_loo_fitness(CholLaunch c, const double* __restrict__ pred, int nt,
                                                      double* __restrict__ rfit, double* __restrict__ press) {
  __shared__ double red[4 * 16];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / nt;
  const int tr = (int)(blockIdx.x % nt);
  const int64_t nT = c.d.nT;
  const double* p = pred + (b * nt + tr) * nT;
  const double* y = c.ft.yT[fold_of(c.ft, b)] + (int64_t)tr * c.d.nTp;
  double pa = 0.0;
  for (int64_t v = t; v < nT; v += LFTH) {
    const double e = y[v] - p[v];
    pa = __builtin_fma(e, e, pa);
  }
  const double ps = block_sum<LFTH>(pa, red);
  __syncthreads();
  const double r = pearson_abs<LFTH>(p, y, nT, red);
  if (t == 0) {
    const bool bad = c.scal[b * SCAL + SC_BAD] != 0.0;
    rfit[b * nt + tr] = bad ? __builtin_nan("") : r;
    press[b * nt + tr] = bad ? __builtin_nan("") : ps;
  }
}

template <int NTR>
hipError_t launch_loo_nt(const CholLaunch& c, const int8_t* geno_sm, const int32_t* train, const double* alpha,
                         const SlabPlan& p, double* vscr, double* pred, double* lev, hipStream_t s) {
  using Kern = decltype(&k_loo<FORM_DUAL, false, NTR>);
  const Kern kern[4] = {k_loo<FORM_DUAL, false, NTR>, k_loo<FORM_DUAL, true, NTR>, k_loo<FORM_PRIMAL, false, NTR>,
                        k_loo<FORM_PRIMAL, true, NTR>};
  const auto launch = [&](Kern k, dim3 grid, size_t shm, int64_t s0, int64_t sn) {
    hipLaunchKernelGGL(k, grid, dim3(LTH), shm, s, c, geno_sm, train, alpha, s0, sn, vscr, pred, lev);
  };
  return launch_slabs(kern, c, p, vscr, (c.d.nT + LOO_W - 1) / LOO_W, launch);
}

}  // namespace

hipError_t launch_loo(const CholLaunch& c, const int8_t* geno_sm, const int32_t* train, const double* alpha,
                      const SlabPlan& p, double* vscr, double* pred, double* lev, hipStream_t s) {
  if (c.B < 1 || c.d.nT < 1) return hipSuccess;
  if (!train || !alpha || !pred || !lev) return hipErrorInvalidValue;
  switch (c.d.nt) {
    case 1: return launch_loo_nt<1>(c, geno_sm, train, alpha, p, vscr, pred, lev, s);
    case 2: return launch_loo_nt<2>(c, geno_sm, train, alpha, p, vscr, pred, lev, s);
    case 3: return launch_loo_nt<3>(c, geno_sm, train, alpha, p, vscr, pred, lev, s);
    case 4: return launch_loo_nt<4>(c, geno_sm, train, alpha, p, vscr, pred, lev, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_loo_fitness(const CholLaunch& c, const double* pred, double* rfit, double* press, hipStream_t s) {
  if (c.B < 1 || c.d.nT < 1) return hipSuccess;
  if (!pred || !rfit || !press || c.B * c.d.nt > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_loo_fitness, dim3((unsigned)(c.B * c.d.nt)), dim3(LFTH), 0, s, c, pred, c.d.nt, rfit, press);
  return hipGetLastError();
}

}  // namespace tblup
