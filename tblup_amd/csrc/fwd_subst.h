// Blocked forward substitution with 16 right-hand sides on fp64 MFMA (v_mfma_f64_16x16x4_f64), shared
// by k_reliab (k_reliab.hip), k_snpscore (k_score.hip) and k_covar (k_covar.hip), and the host side of their
// slab launches (launch_slabs): one 512-thread workgroup solves
//   V_J = X_J (R_J - sum_{L<J} L_JL V_L),  J = J0 .. J1-1,
// in place in V [ns][16] (LDS or a workspace slice of the workgroup's own), from a model's Lt tiles and
// the inverted diagonal tiles X_J = L_JJ^{-1} that the chunk's pipeline left in the workspace.
// Wave q owns rows 16q .. 16q+15 of the block row: one accumulator chain over L = J0 .. J-1 and the rows
// of each tile in order, then over the blocks s = 0 .. q of X_J.  Both kernels run this one chain, so a
// right-hand side's solution is the same bits in either.
#pragma once
#include <algorithm>

#include "tblup_internal.h"

namespace tblup {

constexpr int FWD_TH = 512;     // 8 waves
constexpr int FWD_W = 16;       // right-hand sides per workgroup
constexpr int FWD_STEP = 64;    // rows of L per step of the substitution's chain (16 MFMAs)

// Every thread calls it after a __syncthreads() behind the last write of R into V; q = wave, lc = lane & 15,
// lg = lane >> 4.  Lb / Db: the model's Lt tiles and packed X.  pad: leading rows of V that are zero (skipped
// in whole steps).  done(row, v): called once for each of the thread's four solved values of every block
// row, in row order (row = 128 J + 16 q + lg + 4 r, r = 0 .. 3; right-hand side lc), after V holds them.
template <class Done>
__device__ __forceinline__ void fwd_subst16(const double* __restrict__ Lb, const double* __restrict__ Db, double* V,
                                            int NT, int J0, int J1, int64_t pad, int q, int lc, int lg, Done&& done) {
  constexpr int W = FWD_W;
  // The tiles (J, Lc), Lc = 0 .. J-1, lie back to back and each holds L_JL^T (element [cc][r] =
  // L_JL[r][cc]), so row kx = 128 Lc + cc of that run holds column kx of block row J: one chain over
  // kx in order, FWD_STEP rows per step, through a ring of three register sets -- two steps' L values are
  // in flight while a step's MFMAs run, and the first two steps of block row J + 1 (which need no V)
  // are issued before block row J's barriers.  The zero rows of V that lead the system are skipped in
  // whole steps.
  constexpr int NA = FWD_STEP / 4;
  const double* lrow = Lb + 16 * q + lc;
  const double* vcol = V + lc;
  const int ks = (int)(pad / FWD_STEP) * FWD_STEP;
  double a0[NA], a1[NA], a2[NA];
  auto lda = [&](double (&a)[NA], int k) {
#pragma unroll
    for (int e = 0; e < NA; ++e) a[e] = lrow[(int64_t)(k + 4 * e + lg) * TILE];
  };
  auto prime = [&](int Jn) {
    lrow = Lb + (int64_t)Jn * NT * TILE * TILE + 16 * q + lc;
    if (ks < Jn * TILE) lda(a0, ks);
    if (ks + FWD_STEP < Jn * TILE) lda(a1, ks + FWD_STEP);
  };
  prime(J0);
  for (int J = J0; J < J1; ++J) {
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    // X_J's blocks (q, s), s = 0 .. q, of this wave through a ring of four register sets, the first
    // four in flight under the chain below: stored block (q, s) element [r][cc] = X[16q + cc][16s + r]
    const double* xq = Db + (int64_t)J * NPACK * BLKD + pk(q, 0);
    double xr[4][4];
    auto ldx = [&](double (&x)[4], int s) {
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) x[k4] = xq[s * BLKD + bo(4 * k4 + lg, lc)];
    };
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i <= q) ldx(xr[i], i);
    {
      const int ke = J * TILE;
      auto mm = [&](const double (&a)[NA], int k) {
#pragma unroll
        for (int e = 0; e < NA; ++e)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], vcol[(int64_t)(k + 4 * e + lg) * W], acc, 0, 0, 0);
      };
      for (int k = ks; k < ke; k += 3 * FWD_STEP) {
        if (k + 2 * FWD_STEP < ke) lda(a2, k + 2 * FWD_STEP);
        mm(a0, k);
        if (k + FWD_STEP < ke) {
          if (k + 3 * FWD_STEP < ke) lda(a0, k + 3 * FWD_STEP);
          mm(a1, k + FWD_STEP);
        }
        if (k + 2 * FWD_STEP < ke) {
          if (k + 4 * FWD_STEP < ke) lda(a1, k + 4 * FWD_STEP);
          mm(a2, k + 2 * FWD_STEP);
        }
      }
    }
    if (J + 1 < J1) prime(J + 1);
    double* vj = V + ((int64_t)J * TILE) * W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = (16 * q + lg + 4 * r) * W + lc;
      vj[i] = vj[i] - acc[r];
    }
    __syncthreads();
    v4d acc2 = {0.0, 0.0, 0.0, 0.0};
    for (int s0 = 0; s0 <= q; s0 += 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = s0 + i;
        if (s <= q) {
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4)
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[i][k4], vj[(16 * s + 4 * k4 + lg) * W + lc], acc2, 0, 0, 0);
          if (s + 4 <= q) ldx(xr[i], s + 4);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      vj[(16 * q + lg + 4 * r) * W + lc] = acc2[r];
      done(J * TILE + 16 * q + lg + 4 * r, acc2[r]);
    }
    __syncthreads();
  }
}

// Host side of the slab kernels.  kern: a kernel's four <FORM, VLDS> instances at [2 * (SNP form) + lds];
// the one that the chunk and the plan select runs over the list's nslab slabs, p.S of them per launch
// (B x sn workgroups of FWD_TH threads): launch(kernel, grid, shm, s0, sn) enqueues slabs [s0, s0 + sn).
// With p.lds the right-hand sides are dynamic LDS; the attribute that allows them is set whenever shm > 0.
template <class Kern, class Launch>
hipError_t launch_slabs(const Kern (&kern)[4], const CholLaunch& c, const SlabPlan& p, const double* vscr,
                        int64_t nslab, Launch&& launch) {
  const size_t shm = p.lds ? (size_t)c.sd.ns * FWD_W * 8 : 0;
  if (shm > (size_t)RELIAB_LDS_V || (!p.lds && !vscr)) return hipErrorInvalidValue;
  if (p.S < 1 || c.B * p.S > 0x7fffffff || p.slices != c.B * p.S || p.ns != c.sd.ns) return hipErrorInvalidValue;
  const Kern k = kern[(c.sd.form == FORM_PRIMAL ? 2 : 0) + (p.lds ? 1 : 0)];
  if (shm > 0) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e != hipSuccess) return e;
  }
  for (int64_t s0 = 0; s0 < nslab; s0 += p.S) {
    const int64_t sn = std::min(p.S, nslab - s0);
    launch(k, dim3((unsigned)(c.B * sn)), shm, s0, sn);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace tblup
