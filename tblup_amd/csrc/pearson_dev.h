// Workgroup reductions and the Pearson restatement of the fitness, shared by the solve kernels
// (k_solve.hip) and the covariate model's fitness epilogue (k_covar.hip): one code, so |r| of the same
// numbers is the same bits in either.
//   fitness = |pearsonr(EBV_V, y_V)|       evaluator.py:286 / :314, scipy 1.15.3 pearsonr:
//            exact-equality constant input -> NaN; mean-centre; max-abs scaled
//            norms; clip to [-1, 1]; round when n == 2.
#pragma once
#include "tblup_internal.h"

namespace tblup {

template <int NTH_>
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NTH_ / 64; ++i) s += red[i];
  return s;
}

template <int NTH_>
__device__ __forceinline__ double block_max(double v, double* red) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < NTH_ / 64; ++i) s = fmax(s, red[i]);
  return s;
}

// N sums (max: N maxima) in one pass: each component reduced exactly as block_sum / block_max
// reduce it alone (red: N x 16 slots)
template <int NTH_, int N, bool MAX>
__device__ __forceinline__ void block_reduce(double (&v)[N], double* red) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = MAX ? fmax(v[k], __shfl_xor(v[k], o)) : v[k] + __shfl_xor(v[k], o);
  __syncthreads();
  if (l == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) red[k * 16 + w] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double s = MAX ? red[k * 16] : 0.0;
#pragma unroll
    for (int i = MAX ? 1 : 0; i < NTH_ / 64; ++i) s = MAX ? fmax(s, red[k * 16 + i]) : s + red[k * 16 + i];
    v[k] = s;
  }
}

// (NTH_ may be below the block size: the threads past it hold no elements; red needs a slot per wave)
template <int NTH_>
__device__ __forceinline__ double pearson_abs(const double* e, const double* yV, int64_t nV, double* red) {
  const int t = threadIdx.x < NTH_ ? (int)threadIdx.x : (int)nV;
  const double yb = yV[0], eb = e[0];
  // red: 4 x 16 slots; four reductions (sums and non-constant counts, maxima, squares, products)
  double m4[4] = {0.0, 0.0, 0.0, 0.0};   // sx, sy, ncx, ncy
  for (int64_t v = t; v < nV; v += NTH_) {
    m4[0] += e[v];
    m4[1] += yV[v];
    m4[2] += (e[v] != eb) ? 1.0 : 0.0;
    m4[3] += (yV[v] != yb) ? 1.0 : 0.0;
  }
  block_reduce<NTH_, 4, false>(m4, red);
  const double mx = m4[0] / (double)nV, my = m4[1] / (double)nV;
  const double nonconst_x = m4[2], nonconst_y = m4[3];
  double a2[2] = {0.0, 0.0};
  for (int64_t v = t; v < nV; v += NTH_) {
    a2[0] = fmax(a2[0], fabs(e[v] - mx));
    a2[1] = fmax(a2[1], fabs(yV[v] - my));
  }
  block_reduce<NTH_, 2, true>(a2, red);
  const double xmax = a2[0], ymax = a2[1];
  double q2[2] = {0.0, 0.0};
  for (int64_t v = t; v < nV; v += NTH_) {
    const double a = (e[v] - mx) / xmax, c = (yV[v] - my) / ymax;
    q2[0] = __builtin_fma(a, a, q2[0]);
    q2[1] = __builtin_fma(c, c, q2[1]);
  }
  block_reduce<NTH_, 2, false>(q2, red);
  const double nx = xmax * sqrt(q2[0]);
  const double ny = ymax * sqrt(q2[1]);
  double r1[1] = {0.0};
  for (int64_t v = t; v < nV; v += NTH_) r1[0] = __builtin_fma((e[v] - mx) / nx, (yV[v] - my) / ny, r1[0]);
  block_reduce<NTH_, 1, false>(r1, red);
  double r = r1[0];
  if (r == r) r = fmin(fmax(r, -1.0), 1.0);  // np.clip keeps NaN (fmin/fmax would drop it)
  if (nonconst_x == 0.0 || nonconst_y == 0.0) r = __builtin_nan("");
  if (nV == 2) r = rint(r);
  return fabs(r);
}

}  // namespace tblup
