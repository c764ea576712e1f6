// Prediction from fitted models (tblup_predict_batch): the EBV of any animal of the panel,
//   EBV_t(a) = intercept[t] + sum_j (x[a, idx_j] - center[j]) effects[t][j],
// the formula both reference branches reduce to (gblup: W W_T^T alpha / d, tblup/evaluator.py:284,
// intercept 0; snp: clf.predict of the 2p-centred rows, evaluator.py:308-314, intercept mean(y_T)).
//
// A batched gather-and-dot over the SNP-major int8 panel, bound by the k rows of n bytes each model
// reads.  One 256-thread workgroup per (model, block of 256 listed animals), one animal per thread:
// the model's rows, centres and effects are staged through LDS 256 SNPs at a time (broadcast reads),
// and a thread walks them in list order with one byte load per SNP -- consecutive listed animals
// make a wave's loads one 64-B run of the row, whatever n is (no alignment of the rows is assumed).
// Every animal's sum runs j = 0 .. k-1 in one fma chain per trait, so its bits depend neither on
// n_pred nor on where it stands in the list.
#include "tblup_internal.h"

namespace tblup {

namespace {

constexpr int PTH = 256;   // animals per workgroup
constexpr int PJ = 256;    // SNPs per LDS stage

template <int NTR>
__global__ __launch_bounds__(PTH) void k_predict(const int8_t* __restrict__ geno, int64_t n, int64_t P,
                                                 const int32_t* __restrict__ animals, int64_t n_pred, int64_t nblk,
                                                 const int64_t* __restrict__ idx, const int64_t* __restrict__ off,
                                                 const double* __restrict__ intercept,
                                                 const double* __restrict__ center,
                                                 const double* __restrict__ effects, int64_t plane,
                                                 double* __restrict__ ebv) {
  __shared__ int64_t rowo[PJ];
  __shared__ double cen[PJ];
  __shared__ double eff[NTR][PJ];
  const int t = threadIdx.x;
  const int64_t m = blockIdx.x / nblk, v = (blockIdx.x % nblk) * PTH + t;
  const bool live = v < n_pred;
  const int64_t a = live ? animals[v] : 0;
  const int64_t o0 = off[m], k = off[m + 1] - o0;
  double acc[NTR] = {};
  for (int64_t j0 = 0; j0 < k; j0 += PJ) {
    const int nj = (int)min((int64_t)PJ, k - j0);
    __syncthreads();
    if (t < nj) {
      rowo[t] = snp_col(idx[o0 + j0 + t], P) * n;
      cen[t] = center[o0 + j0 + t];
#pragma unroll
      for (int tr = 0; tr < NTR; ++tr) eff[tr][t] = effects[tr * plane + o0 + j0 + t];
    }
    __syncthreads();
    if (live) {
#pragma unroll 8
      for (int j = 0; j < nj; ++j) {
        const double xc = (double)geno[rowo[j] + a] - cen[j];
#pragma unroll
        for (int tr = 0; tr < NTR; ++tr) acc[tr] = __builtin_fma(xc, eff[tr][j], acc[tr]);
      }
    }
  }
  if (live) {
#pragma unroll
    for (int tr = 0; tr < NTR; ++tr) ebv[(m * NTR + tr) * n_pred + v] = intercept[m * NTR + tr] + acc[tr];
  }
}

}  // namespace

hipError_t launch_predict(const int8_t* geno_sm, int64_t n, int64_t P, const int32_t* animals, int64_t n_pred,
                          const int64_t* idx, const int64_t* off, int64_t B, const double* intercept,
                          const double* center, const double* effects, int64_t plane, int nt, double* ebv,
                          hipStream_t s) {
  if (B < 1 || n_pred < 1) return hipSuccess;
  const int64_t nblk = (n_pred + PTH - 1) / PTH;
  if (B * nblk > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(B * nblk));
  auto launch = [&](auto kernel) -> hipError_t {
    hipLaunchKernelGGL(kernel, grid, dim3(PTH), 0, s, geno_sm, n, P, animals, n_pred, nblk, idx, off, intercept, center,
                       effects, plane, ebv);
    return hipGetLastError();
  };
  switch (nt) {
    case 1: return launch(k_predict<1>);
    case 2: return launch(k_predict<2>);
    case 3: return launch(k_predict<3>);
    case 4: return launch(k_predict<4>);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace tblup
