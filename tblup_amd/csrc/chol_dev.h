// Device-side declarations shared by the column loop of the tile Cholesky (k_chol.hip) and the
// launches that form the system tiles' exact counts before it (k_systiles.hip): the kernels'
// argument block, the packed rows they contract over, and the layout of the count tiles that the
// second writes and the first reads.
#pragma once
#include "i8_tile.h"

namespace tblup {

// Per-launch arguments shared by the Cholesky and the system-tile kernels.
struct CholArgs {
  double* L;                // Lt tiles [B][NT][NT][128*128]
  double* Dinv;             // [B][NT][36 packed 16x16 blocks] X = L_JJ^{-1}
  double* z;                // [B][nt][ns]
  double* w;                // [B][nt][ns] forward-substitution partial sums
  double* S;                // [B][2][36*256] K_JJ - sum_{L<J-1} L_JL L_JL^T, slot J&1
  double* Kd;               // [B][NT][36*256] GRM diagonal tiles (k_diag_grm)
  const double* yT;         // [nt][ytp] dual right-hand sides (y_T - mu, on the fly)
  const double* rhs;        // [B][nt][ns] primal right-hand sides
  const uint8_t* panel;     // [B] x pstride: kernel form, prow packed animal rows of pstride / prow bytes
  int64_t pstride;
  const double* u;          // [B][prow]
  const double* scal;       // [B][SCAL]
  int64_t ns, prow;         // padded system size, panel rows per contraction block
  int form;
  // primal form: rows read in place from the split's 2-bit packed SNP-major matrix
  // (row P is zero; ft.gpk of the system's split)
  const int64_t* idx;
  const int64_t* off;
  int64_t gs_row, P;
  int64_t ytp;              // yT stride (nTp)
  int nt;                   // traits (right-hand sides)
  int NT, J;
  int skip;                 // diagnostic ablation mask (TBLUP_DBG_SKIP); 0 in production
  uint64_t* wgt;            // workgroup trace records (TBLUP_WG_TRACE), null in production
  uint64_t* dtr;            // diagonal launch: phase timestamps of workgroup 0 (TBLUP_WG_TRACE), else null
  const int16_t* kc;        // off-diagonal system-tile counts (k_sys_tiles, either form), else null
  double* part;             // [2][B][NT][128*128] off-diagonal partial sums K - sum_{L<J-1} (acc layout), slot J&1
  double* q;                // last-term mode: [B][NPACK*BLKD] L_{J,J-1} L_{J,J-1}^T, from launch J-1's tile (J, J-1)
  int64_t B;                // individuals in the chunk
  FoldTab ft;               // each system's split (ymu, packed rows)
  int padskip;              // contractions over block column 0 skip the leading padding rows (SNP form)
  int padfirst;             // SNP form: padding rows lead (SC_PAD = ns - k)
  int16_t* kd;              // with k_sys_tiles: the diagonal tiles' exact counts for J >= 2 (KD_TILE
                            // each; the D-units form K_JJ + lambda I where they read it, kd_block); Kd then
                            // holds J < 2 only (the diagonal kernel's direct reads)
};

inline CholArgs make_args(const CholLaunch& c, int J) {
  CholArgs a{c.L, c.Dinv, c.z, c.w, c.S, c.Kd, c.yT, c.rhs, c.panel, c.pstride, c.u, c.scal, c.sd.ns,
             c.sd.prow, c.sd.form, c.idx, c.off, c.gpk_row, c.d.P, c.d.nTp, c.d.nt, c.sd.NT, J, c.skip,
             c.wgt, nullptr, c.kc, c.part, c.q, c.B, c.ft, c.padskip,
             (c.sd.form == FORM_PRIMAL && c.sd.pad_first) ? 1 : 0, c.kd};
  return a;
}

// ---- the count tiles: written once by the system-tile kernels, read once by the unit that forms
// their K (tblup_internal.h: KC_TILE, KD_TILE).  int16 offsets of system s's tiles in kc / kd ----
// off-diagonal tile (I, J), I > J
__device__ __forceinline__ int64_t kc_tile(int NT, int64_t s, int I, int J) {
  return ((s * (NT * (NT - 1) / 2)) + I * (I - 1) / 2 + J) * KC_TILE;
}
// diagonal tile J
__device__ __forceinline__ int64_t kd_tile(int NT, int64_t s, int J) { return (s * NT + J) * KD_TILE; }
// Non-temporal accesses, so that 235 MB of them a step do not push the Lt tiles out of the caches
__device__ __forceinline__ int2 nt_load2(const int16_t* p) {
  const long long v = __builtin_nontemporal_load(reinterpret_cast<const long long*>(p));
  return int2{(int)(unsigned)(v & 0xffffffffll), (int)(v >> 32)};
}
__device__ __forceinline__ void nt_store2(int16_t* p, int2 v) {
  __builtin_nontemporal_store((long long)(((unsigned long long)(unsigned)v.y << 32) | (unsigned)v.x),
                              reinterpret_cast<long long*>(p));
}
// a lane's four int16 counts of one 16 x 16 block (accumulator elements r = 0 .. 3)
__device__ __forceinline__ v4i unpack_counts4(int2 p) {
  return v4i{(int32_t)(int16_t)(p.x & 0xffff), (int32_t)(int16_t)(p.x >> 16), (int32_t)(int16_t)(p.y & 0xffff),
             (int32_t)(int16_t)(p.y >> 16)};
}

// row I and column J <= I of element t = I (I + 1) / 2 + J of a row-major lower triangle
__device__ __forceinline__ void tri_decode(int t, int& I, int& J) {
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  J = t - I * (I + 1) / 2;
}

// ---- operand images of a 64-B stage of packed rows, [128 rows][64 B] ----
// The loader lane of 16-B chunk pos of a row reads source chunk pos ^ swizzle(row): A rows swizzle by
// (row >> 2) & 3, B rows by (row >> 2) & 2, which keeps both ds_read_b128 patterns conflict-free.
__device__ __forceinline__ int pk_swz_a(int row, int pos) { return 16 * (pos ^ ((row >> 2) & 3)); }
__device__ __forceinline__ int pk_swz_b(int row, int pos) { return 16 * (pos ^ ((row >> 2) & 2)); }
__device__ __forceinline__ int i8off_a(int row, int c) { return row * 64 + pk_swz_a(row, c); }
__device__ __forceinline__ int i8off_b(int row, int c) { return row * 64 + pk_swz_b(row, c); }

// Packed panel row of system row r of individual b (kernel form: the gathered animal rows,
// dual_pk_row = pstride / prow bytes each; stage kb at + 16 kb, as row_packed's)
__device__ __forceinline__ const uint8_t* row_dpk(const CholArgs& a, int64_t b, int64_t r) {
  return a.panel + b * a.pstride + r * (a.pstride / a.prow);
}
// Packed split row of system row r (primal: row r holds selected SNP r - pad; padding rows -> the
// zero row P; stage kb at + 16 kb).
__device__ __forceinline__ const uint8_t* row_packed(const CholArgs& a, int64_t b, int64_t r) {
  const int64_t o0 = a.off[b], k = a.off[b + 1] - o0;
  const int64_t pad = a.padfirst ? a.ns - k : 0;   // = SC_PAD, without a dependent scal load
  int64_t p = a.P;
  if (sys_real(r, pad, k)) {
    p = snp_col(a.idx[o0 + r - pad], a.P);
  }
  return a.ft.gpk[fold_of(a.ft, b)] + p * a.gs_row;
}

// Profiling only: workgroup start / end timestamps (s_memrealtime, 100 MHz) of a launch.
struct WgTrace {
  uint64_t* rec;
  uint64_t t0;
  uint64_t ph;   // up to three phase marks of wave 0 (10-ns ticks from the start, 16 bits each)
  __device__ __forceinline__ explicit WgTrace(uint64_t* base) : rec(nullptr), t0(0), ph(0) {
    if (base) {
      rec = base + (int64_t)blockIdx.x * WGT_REC;
      t0 = __builtin_amdgcn_s_memrealtime();
    }
  }
  __device__ __forceinline__ void mark(int k) {
    if (!rec) return;
    const uint64_t d = __builtin_amdgcn_s_memrealtime() - t0;
    ph |= (d < 0xffff ? d : 0xffff) << (16 * k);
  }
  __device__ __forceinline__ void done(int kind, int J, int I, int64_t b) {
    if (!rec) return;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
      rec[0] = t0;
      rec[1] = t1;
      rec[2] = ((uint64_t)kind << 56) | ((uint64_t)I << 40) | (uint64_t)b;
      rec[3] = (uint64_t)J | (ph << 16);
    }
  }
};

}  // namespace tblup
