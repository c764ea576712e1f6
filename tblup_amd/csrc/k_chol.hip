// Batched left-looking tile Cholesky of (K_TT + lambda I), fp64, 128x128 tiles,
// with the GRM tiles from exact integer counts (K is never stored in fp64).
//
// Replaces the reference's per-individual dense solves
//   gblup:    G_inv = np.linalg.inv(G_TT + lambda I)          (tblup/evaluator.py:280-284)
//   snp_blup: Ridge(alpha).fit -> scipy.linalg.solve(assume_a="pos") (evaluator.py:311-312,
//             scikit-learn 1.7.2 _ridge.py _solve_cholesky[_kernel])
// by one Cholesky factorisation per individual, batched over the population.
// For each tile column J:
//   k_chol_diag    (one WG per individual): K_JJ - sum_L L_JL L_JL^T (fp64 MFMA SYRK on the
//                  lower blocks), blocked 16x16 factorisation, blocked inverse
//                  X_J = L_JJ^{-1}, forward-substitution block z_J = X_J (y_J - mu - w_J)
//   k_chol_offdiag (one WG per individual x tile row I > J), all transposes in registers:
//                  T^T = K_JI - sum_L L_JL L_IL^T  (fp64 MFMA, acc = T^T)
//                  L_IJ^T = X_J T^T               (acc of T^T is the B operand directly)
//                  w_I += L_IJ z_J                (forward-substitution partial sums)
// Where K comes from: by default the exact integer counts of every system tile are formed on FP4
// MFMA before the column loop (k_systiles.hip) and the units here only turn them into fp64 K where
// they read them (kc_issue / k_acc, kd_load / kd_block; layout: chol_dev.h).  Without those counts
// (one tile, counts past int16, the kernel form with TBLUP_DUAL_ST=0 or with shared fold counts) the
// int8 MFMA rings of this file form them: k_diag_grm8 and diag_grm_tile for K_JJ, k_acc's own int8
// phase for K_JI, k_gshare for the shared counts.
//
// Storage of L ("Lt"): tile-contiguous and transposed.  Tile (I, J), I >= J, of matrix b
// is 128x128 doubles at L + ((b*NT + I)*NT + J)*128*128 with Lt[j][i] = L[128I+i][128J+j],
// so a 16-k-row stage of any operand is 16 KiB contiguous and every tile write coalesces.
//
// MFMA layouts (verified on gfx950 by tools/mfma_probe*.hip):
//   f64 16x16x4 : A[i=l&15][k=l>>4], B[k=l>>4][j=l&15], C row=(l>>4)+4r, col=l&15
//   i8 16x16x64 : A row l&15, B col l&15, 16 B of k per lane, C row=4(l>>4)+r, col=l&15
//   i8 32x32x32 : C row=(r&3)+8(r>>2)+4(l>>5), col=l&31
// Reading the i8 16x16x64 A rows through the permutation pi(rho) = (rho>>2) + 4(rho&3)
// makes its accumulator land in the f64 C layout, so the exact integer GRM counts
// become the fp64 accumulators of the Cholesky GEMM without any data movement.
#include "chol_dev.h"
#include <algorithm>
#include <type_traits>

namespace tblup {

namespace {

constexpr int BKD = 16;                // k rows per fp64 stage
constexpr int LTS = BKD * TILE;        // doubles in one 16-row stage of an Lt tile (16 KiB)
constexpr int TT = TILE * TILE;        // doubles per tile

__device__ __forceinline__ v4d mfma64(double a, double b, v4d c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// c - a*b: for f64 MFMA the BLGP field is the operand-negate mask (neg:[1,0,0] = -A)
__device__ __forceinline__ v4d mfma64_nega(double a, double b, v4d c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 1);
}

constexpr int NSLOT = TBLUP_NSLOT;

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// (glds16_asm, the stage rings' LDS-DMA as inline asm -- the SYRK, GEMM1 and integer-count rings all
// use it: tblup_internal.h)
// Non-temporal result stores (round 5): the L tiles of the T-units, the partial sums (P- / E-units),
// the diagonal targets S and last terms Q -- each read by a later launch, none by this one (the
// last-term read-back aside), and every line a kernel leaves dirty in L2 is written back at its
// end (the kernel boundary).  Interleaved A/B at config 2 (profiles/r05_nt_store_ab.txt): both on
// +0.9% at pop 256 (off-diagonal 1.611 -> 1.594 ms), +1.0% at 128, +0.9% at 64 (the L tiles alone:
// -0.3% at 64).  The partial sums' and S's loads are non-temporal too (each read once; A/B: +0.7% at
// pop 128, +0.15% at 256, same file).  The diagonal kernel's X_J (Dinv) stores and the system-tile
// epilogue's K_JJ + lambda I tiles J < 2 stay plain stores.  (Where a store's address goes into a
// local `d` first, that is the evaluation order of the measured builds: address, then value.)

// Stage image [16 k][128 x] of an Lt tile: 16-B chunk p of row k holds source chunk
// p ^ 8(k&1), so the fragment pattern (16 x in one k row, the next k in lanes 16-31)
// covers all 64 banks.  One LDS-DMA instruction moves one 1 KiB k row.
__device__ __forceinline__ int lt_off(int k, int x) { return k * TILE + 2 * ((x >> 1) ^ (8 * (k & 1))) + (x & 1); }

// ---- int8 GRM tile in the f64 accumulator layout (offdiag) ----
// cnt[cb][ib] = sum_s A[16cb + pi-row][s] B[32w + 16ib + col][s] with A = panel rows of tile J
// (c) and B = panel rows of tile I (i).  Panel tiles [128 rows][64 B], chunks swizzled (i8off_a /
// i8off_b, chol_dev.h).

// ---- SYRK restricted to the 36 lower 16x16 blocks (diag kernel), A = Lt tiles (J, L) ----
__host__ __device__ constexpr int tri_q(int e) {
  int q = 0;
  while ((q + 1) * (q + 2) / 2 <= e) ++q;
  return q;
}
__host__ __device__ constexpr int tri_s(int e) { return e - tri_q(e) * (tri_q(e) + 1) / 2; }
// runtime row of packed lower block e (e < 36)
__device__ __forceinline__ int tri_q_rt(int e) {
  int q = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  if ((q + 1) * (q + 2) / 2 <= e) ++q;
  if (q * (q + 1) / 2 > e) --q;
  return q;
}


// acc (16x16, f64 MFMA C layout) += A(16x16) * B(16x16)^T, both blocks in LDS
__device__ __forceinline__ v4d mma_abt(const double* A, const double* Bt, v4d acc, int l) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int k = 4 * kk + (l >> 4);
    acc = mfma64(A[bo(l & 15, k)], Bt[bo(l & 15, k)], acc);
  }
  return acc;
}

// Factor the 16x16 SPD block D with ONE wave (no barriers): X <- L^{-1} (lower, zeros above),
// and L into D's lower triangle on the debug path.  Right-looking elimination with unscaled
// pivots; E = L'^{-1} is built by row operations on I alongside (L = L' D^{1/2}, X = D^{-1/2} E):
//   c > j : T_ic -= (T_ij / piv_j) T_jc
//   i > j : E_ic -= (T_ij / piv_j) E_jc (c < j),  E_ij = -T_ij / piv_j
// Column scaling by 1/sqrt(piv) is deferred to the end.
__device__ __forceinline__ double recip(double p) {
  double r = __builtin_amdgcn_rcp(p);
  double e = __builtin_fma(-p, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-p, r, 1.0);
  return __builtin_fma(r, e, r);
}

__device__ __forceinline__ double rdlane(double x, int lane) {
  const long long bits = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)bits, lane);
  const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// x += x[lane J of this 16-lane row] * m in one instruction (DPP64 row_newbcast on src0).  The
// compiler does not see inside asm, so hazards are handled here: NOP = the DPP read-after-VALU-
// write wait for a register the previous instruction may have written (the next pivot's
// column); the others are volatile so they keep their order, in which no fmac reads a
// register the one before it wrote.  That the compiler places no other VALU write of an fmac's
// src0 within 2 wait states of it is checked on the built library by tools/check_dpp_hazards.py
// (tests/test_abi.py); an s_nop on every fmac instead would lengthen factor16's pivot chain.
template <int J, bool NOP>
__device__ __forceinline__ void fmac_row(double& x, double m) {
  if constexpr (NOP)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf"
                 : "+v"(x) : "v"(m), "i"(J));
  else
    asm volatile("v_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(x) : "v"(m), "i"(J));
}

// Rows 0 and 2 of the wave to rows 1 and 3 (v_permlane16_swap on each 32-bit half).
__device__ __forceinline__ double even_rows_to_odd(double x) {
  const long long bits = __double_as_longlong(x);
  const unsigned lo = (unsigned)bits, hi = (unsigned)(bits >> 32);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __longlong_as_double(((long long)b[0] << 32) | (unsigned)a[0]);
}

// v on lanes whose row (lane & 15) is below J, +0 elsewhere: the lane mask is a constant in
// SGPRs (no compare on the pivot chain)
template <int J>
__device__ __forceinline__ double rows_below(double v) {
  constexpr unsigned long long r = (0xFFFFull << (J + 1)) & 0xFFFFull;
  constexpr unsigned long long msk = r | (r << 16) | (r << 32) | (r << 48);
  const long long bits = __double_as_longlong(v);
  int lo = (int)bits, hi = (int)(bits >> 32);
  asm("v_cndmask_b32_e64 %0, 0, %0, %2\n\tv_cndmask_b32_e64 %1, 0, %1, %2" : "+v"(lo), "+v"(hi) : "s"(msk));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// 16x16 factor and inverse.  Lane l = i + 16 g: even groups hold row i of T in x[0..15]
// (column c in register c), odd groups row i of E (the Gauss-Jordan inverse, starting at I)
// with column c in register 15 - c.  Pivot j: T_jj by v_readlane, l_i = T_ij / T_jj from the
// lane's own register j (zero for i <= j), handed from the T rows to the E rows by a
// permlane16 swap, then every register the two halves still need -- T columns > j, E columns
// <= j, the same registers thanks to E's reversed order -- takes x += x[row j] * (-l_i) in one
// DPP64 fmac.  Registers outside those sets only ever receive x += 0 or hold finished columns,
// so no per-element masks.  The next pivot's column goes first; for j < 7 it is an E column
// above the diagonal (E_jc = 0) for the odd groups, so it takes the multiplier before the swap
// and the swap leaves the pivot chain.  Same operations in the same order per element as the
// factor / elimination T_ic -= l_i T_jc, E_ic -= l_i E_jc, so the factor and its inverse are
// unchanged.  Row i of T is final after pivot i - 1 (later multipliers are 0 there), so T_ii,
// the pivot, is still in register i at the end.
template <int J, int R>
__device__ __forceinline__ void f16_upd(double (&x)[NB], double m) {
  if constexpr (R < NB) {
    if constexpr (R != J + 1) fmac_row<J, false>(x[R], m);
    f16_upd<J, R + 1>(x, m);
  }
}

template <int J, bool WL>
__device__ __forceinline__ void f16_steps(double (&x)[NB], double (&ls)[NB]) {
  if constexpr (J + 1 < NB) {
    const double piv = rdlane(x[J], J);
    if constexpr (WL) ls[J] = x[J];
    const double mt = rows_below<J>(-(x[J] * recip(piv)));
    const double m = even_rows_to_odd(mt);
    fmac_row<J, true>(x[J + 1], (J < 7) ? mt : m);   // next pivot's column first
    constexpr int R0 = (J + 1 < NB - 1 - J) ? J + 1 : NB - 1 - J;
    f16_upd<J, R0>(x, m);
    f16_steps<J + 1, WL>(x, ls);
  } else if constexpr (WL) {
    ls[J] = x[J];
  }
}

template <int C>
__device__ __forceinline__ void f16_store_l(double* D, const double (&ls)[NB], double rs_own, int l) {
  if constexpr (C < NB) {
    const double rc = __builtin_amdgcn_mov_dpp(rs_own, 0x150 + C, 0xF, 0xF, true);  // lane C's 1/sqrt(piv_C)
    if (l < 16 && l >= C) D[bo(l, C)] = ls[C] * rc;
    f16_store_l<C + 1>(D, ls, rs_own, l);
  }
}

__device__ __forceinline__ void fstamp(uint64_t* st, int slot) {
  if (st && (threadIdx.x & 63) == 0) st[slot] = __builtin_amdgcn_s_memrealtime();
}

// D: symmetric 16x16 block (both triangles) -> X = L^{-1} (and, WL, L into D's lower triangle;
// the diagonal L blocks are read back only by the debug path).  X must hold the reversed
// identity (X_{i,15-i} = 1) on entry: the E rows load it as their starting point.
template <bool WL>
__device__ __forceinline__ void factor16(double* D, double* X, int l, uint64_t* st) {
  const int i = l & 15;
  fstamp(st, 50);
  const bool t_row = ((l >> 4) & 1) == 0;
  const double* src = t_row ? D : X;
  double x[NB], ls[NB];
#pragma unroll
  for (int k = 0; k < NB / 2; ++k) {
    const v2d v = *reinterpret_cast<const v2d*>(src + bo(i, 2 * k));
    x[2 * k] = v[0];
    x[2 * k + 1] = v[1];
  }
  fstamp(st, 51);
  f16_steps<0, WL>(x, ls);
  fstamp(st, 52);
  // the pivot of row i from register i of the T rows, to the E rows by the same swap
  double own = x[0];
#pragma unroll
  for (int c = 1; c < NB; ++c) own = (i == c) ? x[c] : own;
  own = even_rows_to_odd(own);
  // deferred scaling: X_ic = E_ic / sqrt(piv_i) (E_ic = +0 above the diagonal); L_ic = T_ic / sqrt(piv_c)
  const double rs_own = 1.0 / sqrt(own);
  if (l >= 16 && l < 32) {
#pragma unroll
    for (int k = 0; k < NB / 2; ++k)
      *reinterpret_cast<v2d*>(X + bo(i, 2 * k)) = v2d{x[NB - 1 - 2 * k] * rs_own, x[NB - 2 - 2 * k] * rs_own};
  }
  if constexpr (WL) f16_store_l<0>(D, ls, rs_own, l);
  fstamp(st, 53);
}


}  // namespace

// K_JJ + lambda I (identity on padding rows) of packed lower block e of individual b's diagonal tile J,
// from its exact counts (the system-tile launches, k_systiles.hip), minus sub (may be null), into the packed-block image dst: the
// f64 MFMA C layout, element (16 q + (l >> 4) + 4 r, 16 s + (l & 15)) of the tile at
// dst[pk(q, s) + bo((l >> 4) + 4 r, l & 15)], q / s the block's row / column.  cv: the block's
// counts (int2 load issued by the caller).  (v - 0.0 == v exactly, so sub = 0 stores K itself.)
__device__ __forceinline__ void kd_block(const CholArgs& a, int64_t b, int J, int e, int2 cv, v4d sub,
                                         double* dst) {
  const int l = threadIdx.x & 63;
  const double* sc = a.scal + b * SCAL;
  const double sa = sc[SC_SA], cN = sc[SC_CN], invd = sc[SC_INVD], lam = sc[SC_LAM], sm = sc[SC_SM];
  const int64_t nrow = (int64_t)sc[SC_NROW], pad = (int64_t)sc[SC_PAD];
  int q, sb;
  tri_decode(e, q, sb);
  const int64_t j0 = (int64_t)J * TILE;
  const double* ub = a.u + b * a.prow + j0;
  const int il = 16 * sb + (l & 15);
  const int64_t gj = j0 + il;
  const double uj = ub[il];
  const v4i c4 = unpack_counts4(cv);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int cl = 16 * q + (l >> 4) + 4 * r;
    const int64_t gi = j0 + cl;
    const double kv = grm_value(c4[r], ub[cl], uj, sa, cN, invd, sm);
    const double v = (sys_real(gi, pad, nrow) && sys_real(gj, pad, nrow)) ? kv + ((gi == gj) ? lam : 0.0)
                                                                         : ((gi == gj) ? 1.0 : 0.0);
    double* d = dst + pk(q, sb) + bo((l >> 4) + 4 * r, l & 15);
    __builtin_nontemporal_store(v - sub[r], d);
  }
}
__device__ __forceinline__ int2 kd_load(const CholArgs& a, int64_t b, int J, int e) {
  const int l = threadIdx.x & 63;
  return nt_load2(a.kd + kd_tile(a.NT, b, J) + (e * 64 + l) * 4);
}

// Leading contraction rows of block column 0 that a GEMM1 / SYRK run starting at L = 0 skips:
// individual b's leading padding rows (SC_PAD), rounded down to the MFMA's 4-row k-step.
__device__ __forceinline__ int skip_rows(const CholArgs& a, int64_t b) {
  return a.padskip ? ((int)a.scal[b * SCAL + SC_PAD] & ~3) : 0;
}

// st: profiling only (phase stamps of one factorisation in diagonal workgroup 0), else null
template <bool LJJ = true>   // LJJ false: a kernel that never runs the debug path (its launcher sees to it)
__device__ __forceinline__ void factor16_any(const CholArgs& a, double* D, double* X, int l, uint64_t* st = nullptr) {
  if (LJJ && (a.skip & FLAG_WRITE_LJJ))
    factor16<true>(D, X, l, st);
  else
    factor16<false>(D, X, l, st);
}

// Profiling only: lane 0 of each wave of diagonal workgroup 0 stamps phase boundaries
// (s_memrealtime) into dtr[wave * 64 + slot].
__device__ __forceinline__ void dstamp(const CholArgs& a, int slot) {
  if (a.dtr && blockIdx.x == 0 && (threadIdx.x & 63) == 0)
    a.dtr[(threadIdx.x >> 6) * 64 + slot] = __builtin_amdgcn_s_memrealtime();
}

// Kernel form, folds sharing one animal set (FoldTab::gsh): the exact count A_r . A_c of system
// rows r, c (< n_Tp) of system s, from its individual's A_R A_R^T (k_gshare); padding rows count 0,
// as their zero panel rows do
__device__ __forceinline__ int32_t gsh_count(const CholArgs& a, int64_t s, int64_t r, int64_t c) {
  const FoldTab& ft = a.ft;
  const int32_t* mp = ft.gmap + (int64_t)fold_of(ft, s) * ft.gmap_ld;
  const int32_t mr = mp[r], mc = mp[c];
  return (mr >= 0 && mc >= 0) ? ft.gsh[((s % ft.bpf) * ft.gsh_ld + mr) * ft.gsh_ld + mc] : 0;
}

// ---------------------------------------------------------------------------
// Diagonal tile T_J = K_JJ - sum_{L<J} L_JL L_JL^T is assembled from pieces that are
// computed OFF the column-to-column critical path:
//   K_JJ            k_diag_grm, all J of the batch in one launch up front
//   L < J-1 terms   extra workgroups of the off-diagonal launch of column J-1
//   L = J-1 term    k_diag_prep right before the diagonal kernel (split over k)
// Each piece is written in the packed block layout the diagonal kernel factorises in,
// so the diagonal kernel sums them with a linear sweep.
// ---------------------------------------------------------------------------
constexpr int DW = 8;            // waves per diagonal workgroup: phase A (S load, SYRK map), and the whole
                                 // workgroup in the launches that carry D- / E-units
constexpr int DTHR = 64 * DW;
// waves of the diagonal workgroups in launches without D- / E-units (k_chol_diag_w): the extra
// waves join at the factorisation windows as workers (diag_tile)
constexpr int DWX = DIAG_WAVES_WIDE;
static_assert(DWX > DW && DWX % 4 == 0 && DWX <= 16, "wide diagonal workgroup: 12 or 16 waves");
// diag z: four lanes per row, so one wave forms the z of one 16-row block row (diag_z), whatever
// the workgroup's wave count
static_assert(64 == 4 * NB && DW >= NBLK, "diag z: four lanes per row, one wave per block row");



// ===========================================================================
// Off-diagonal launch, 8 waves (512 threads) per workgroup, two workgroups per CU:
// wave w owns the 16 columns i in [16w, 16w+16) of its tile; 16 waves per CU hide the
// operand latency better than 8 (GEMM1 microbenchmark: 62 vs 58 TFLOP/s).
// ===========================================================================
constexpr int OW = 8;            // waves per off-diagonal workgroup
constexpr int OTH = 64 * OW;     // threads

// Packed rows (the SNP form's split rows, the kernel form's gathered panel), 64-B stages: stage st
// = 256 contraction elements = 64 B of each packed row (rows of 4 swizzled 16-B chunks; every
// 128-B line of a row is consumed by two consecutive stages).
// Lane (rho, ch) reads one 16-B chunk = 4 packed dwords and feeds dword s to k-step s, so
// the four lane groups x four k-steps cover the 16 dwords once (animal order inside a
// stage is immaterial to the counts; A and B use the same order).  A stage past the
// training block (nblk = 64-animal blocks, nblk % 4 != 0) zeroes chunks ch >= nblk % 4.
template <int D, int WCL = -1>
__device__ __forceinline__ void i8_tt8_pk64(const uint8_t* sa, const uint8_t* sb, int64_t nblk, uint8_t* lds,
                                            v4i (&cnt)[8]) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wc = (WCL < 0) ? w : WCL;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) cnt[cb] = v4i{0, 0, 0, 0};
  if (nblk <= 0) return;
  const int64_t nst = (nblk + 3) >> 2;
  constexpr int TB = TILE * 64;
  auto issue = [&](int64_t st) {
    uint8_t* slot = lds + (int)(st % D) * 2 * TB;
    glds16_asm(sa + st * 64, slot + w * 1024);
    glds16_asm(sb + st * 64, slot + TB + w * 1024);
  };
  for (int64_t st = 0; st < D - 1 && st < nst; ++st) issue(st);
  const int rho = l & 15, prow = (rho >> 2) + 4 * (rho & 3), ch = l >> 4;
  const int tail_ch = (int)(nblk & 3);
  for (int64_t st = 0; st < nst; ++st) {
    if (st + D - 2 < nst) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 2) * 2) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (st + D - 1 < nst) issue(st + D - 1);
    const uint8_t* As = lds + (int)(st % D) * 2 * TB;
    const uint8_t* Bs = As + TB;
    uint4 bq = *reinterpret_cast<const uint4*>(Bs + i8off_b(16 * wc + rho, ch));
    if (st == nst - 1 && tail_ch != 0 && ch >= tail_ch) bq = uint4{0u, 0u, 0u, 0u};
    uint4 aq[8];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
      if (cb >= WCL) aq[cb] = *reinterpret_cast<const uint4*>(As + i8off_a(16 * cb + prow, ch));
    const uint32_t bw[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const v4i bv = unpack16(bw[s4]);
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        if (cb >= WCL) {
          const uint32_t aw = s4 == 0 ? aq[cb].x : s4 == 1 ? aq[cb].y : s4 == 2 ? aq[cb].z : aq[cb].w;
          cnt[cb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(unpack16(aw), bv, cnt[cb], 0, 0, 0);
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// Off-diagonal SNP-form tile with a 2-D wave split: the stages are loaded exactly as in
// i8_tt8_pk64, but wave w = (wr, wc) = (w >> 2, w & 3) computes row blocks 4wr..4wr+3 x
// column blocks 2wc, 2wc+1, so each k-step unpacks 4 A + 2 B dwords for 8 MFMAs (instead of
// 8 + 1).  The counts then go through LDS (64 blocks x 1 KiB, lane-linear 16-B slots) so
// that wave w ends up with column block w for all 8 row blocks -- the layout GEMM1/GEMM2 use
// (the MFMA lane mapping inside a block is the same in both layouts).
template <int D>
__device__ __forceinline__ void i8_tt2d_pk64(const uint8_t* sa, const uint8_t* sb, int64_t nblk, uint8_t* lds,
                                             v4i (&cnt)[8]) {
  // D is unused: two 128-B super-stages (each = two of i8_tt8_pk64's 64-B stages, 32 KiB)
  // alternate in the 64 KiB ring, one barrier per 512 animals
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w >> 2, wc = w & 3;
  v4i c2[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) c2[m][ib] = v4i{0, 0, 0, 0};
  if (nblk > 0) {
    const int64_t nh = (nblk + 3) >> 2;   // 64-B half stages
    const int64_t nst = (nh + 1) >> 1;
    constexpr int TB = TILE * 64;
    auto issue = [&](int64_t st) {
      uint8_t* slot = lds + (int)(st & 1) * 4 * TB;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t hs = 2 * st + h;
        if (hs < nh) {
          glds16_asm(sa + hs * 64, slot + h * 2 * TB + w * 1024);
          glds16_asm(sb + hs * 64, slot + h * 2 * TB + TB + w * 1024);
        }
      }
    };
    issue(0);
    const int rho = l & 15, prow = (rho >> 2) + 4 * (rho & 3), ch = l >> 4;
    const int tail_ch = (int)(nblk & 3);
    for (int64_t st = 0; st < nst; ++st) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (st + 1 < nst) issue(st + 1);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t hs = 2 * st + h;
        if (hs < nh) {
          const uint8_t* As = lds + (int)(st & 1) * 4 * TB + h * 2 * TB;
          const uint8_t* Bs = As + TB;
          const bool ztail = (hs == nh - 1 && tail_ch != 0 && ch >= tail_ch);
          uint4 bq[2], aq[4];
#pragma unroll
          for (int ib = 0; ib < 2; ++ib) {
            bq[ib] = *reinterpret_cast<const uint4*>(Bs + i8off_b(16 * (2 * wc + ib) + rho, ch));
            if (ztail) bq[ib] = uint4{0u, 0u, 0u, 0u};
          }
#pragma unroll
          for (int m = 0; m < 4; ++m)
            aq[m] = *reinterpret_cast<const uint4*>(As + i8off_a(16 * (4 * wr + m) + prow, ch));
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            v4i bv[2];
#pragma unroll
            for (int ib = 0; ib < 2; ++ib)
              bv[ib] = unpack16(s4 == 0 ? bq[ib].x : s4 == 1 ? bq[ib].y : s4 == 2 ? bq[ib].z : bq[ib].w);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              const v4i av = unpack16(s4 == 0 ? aq[m].x : s4 == 1 ? aq[m].y : s4 == 2 ? aq[m].z : aq[m].w);
#pragma unroll
              for (int ib = 0; ib < 2; ++ib)
                c2[m][ib] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv[ib], c2[m][ib], 0, 0, 0);
            }
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }
  // exchange: block (row cb, column ib) at slot ib * 8 + cb, lane l's 16 B at l
  v4i* xs = reinterpret_cast<v4i*>(lds);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) xs[((2 * wc + ib) * 8 + 4 * wr + m) * 64 + l] = c2[m][ib];
  __syncthreads();
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) cnt[cb] = xs[(w * 8 + cb) * 64 + l];
  __syncthreads();
}

// GEMM1: acc[cb] -= sum_k L_J[c][k] L_I[i][k] over the nL Lt tiles starting at ltJ / ltI (k < 128 nL)
// for the wave's 16 columns i and the NCB row blocks cb0 .. cb0+NCB-1, on 32-row stages: only A
// (the Lt_J stage every wave reads) goes through the LDS ring (2 x 32 KiB); each wave's B operand
// (its own 16 columns of Lt_I) is loaded straight into registers: k-step kk of stage s, once its
// MFMAs are issued, reloads bc[kk] for stage s + 1.  (A 16-row A+B ring has twice the barriers and
// measured 2% slower.)  Every accumulator element's chain of MFMAs is the same whatever NCB / cb0 and
// wherever the L range is split, so partial sums handed from one launch to the next reproduce the
// one-workgroup result bit for bit.
//
// Waits.  The vector-memory queue of a wave completes in order.  At the top of stage s it holds,
// oldest first, A(s) x 4 (LDS-DMA, inline asm: the compiler does not count them) and B(s) x 8; the
// stage's own wait is vmcnt(8): the four A ops, nothing younger.  A(s + 1) x 4 follows the barrier,
// and k-step kk waits for bc[kk] with the compiler's vmcnt(7) -- it counts the 8 B loads it sees; the
// 4 A ops it does not see make that stricter than needed (exact: 11), never laxer -- so a B load has
// 3 to 4 k-steps (24 to 32 MFMAs of its wave) in flight before anything waits on it.  For the count
// to hold the B loads are unconditional and pinned behind their k-step by scheduling barriers:
// under `if (more)` the wait-count pass may not count a load as issued and emitted vmcnt(7 - kk),
// which from k-step 2 on waited for the loads just issued and drained the queue at k-step 7; left
// free, max-ILP bunches the loads at the stage's end and spills, and the scratch reloads bring
// vmcnt(0) into the loop (tools/stage_waits.py --check guards both).  The last stage therefore
// reloads its own B rows (address clamped to stage s): 8 loads per call, L2 hits, never read -- the
// compiler tracks them as pending writes of bc[], so no later use of those registers can pass them,
// and a later counted wait only finds older ops in the queue, which makes it wait for more.
//
// r0 (a multiple of 4): leading contraction rows skipped -- the SNP form's leading padding rows,
// whose columns of block column 0 are exact zeros (sys_real), so only a range that starts at L = 0
// passes r0 > 0: whole 32-row stages, then the first stage computed from k-step (r0 & 31) / 4 (a
// peeled stage: the main loop stays the branch-free one; a short LAST stage instead, or a per-k-step
// bound inside the loop, made the compiler spill or split the MFMA chains).  The MFMAs skipped would
// only have added exact zeros, so the result is the same bit for bit.
template <int NCB>
__device__ __forceinline__ void gemm1_a32(const double* __restrict__ ltJ, const double* __restrict__ ltI, int nL,
                                          int cb0, double* lds, v4d (&acc)[NCB], int r0 = 0) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int AS = 32 * TILE;   // doubles per 32-row stage
  const int s0 = r0 >> 5;         // whole leading stages skipped
  const int kf = (r0 & 31) >> 2;  // leading k-steps skipped in the first stage computed
  const int nst = 4 * nL;
  if (nst <= s0) return;
  auto src_of = [&](int s) { return (int64_t)(s >> 2) * TT + (s & 3) * AS; };
  auto issue_a = [&](int s) {
    double* slot = lds + (s & 1) * AS;
    const int64_t src = src_of(s);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * w + e;
      glds16_asm(ltJ + src + k * TILE + 2 * (l ^ (8 * (k & 1))), slot + k * TILE);
    }
  };
  const double* bcol = ltI + 16 * w + (l & 15) + (l >> 4) * TILE;
  double bc[8];
  issue_a(s0);
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) bc[kk] = bcol[src_of(s0) + 4 * kk * TILE];
  int s = s0;
  if (kf > 0) {   // the first stage from k-step kf
    // the next stage's A issued before this short stage's wait, not after it.  The queue is then
    // A(s) x 4, B(s) x 8, A(s + 1) x 4, and only A(s) has to be complete: vmcnt(12) leaves this stage's
    // 8 B loads (the compiler's own waits cover them) and the next stage's 4 LDS-DMA ops outstanding;
    // without a next stage the queue is A(s) x 4, B(s) x 8 and vmcnt(8) leaves the 8 B loads.
    const bool more = s + 1 < nst;
    if (more) {
      issue_a(s + 1);
      asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const double* bs = bcol + src_of(more ? s + 1 : s);
    const double* As = lds + (s & 1) * AS;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + (l >> 4);
      if (kk >= kf) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          acc[cb] = mfma64_nega(As[lt_off(k, 16 * (cb0 + cb) + (l & 15))], bc[kk], acc[cb]);
      }
      // conditional here (once per call, not in the loop): unconditional loads in this stage, pinned
      // or not, spill (scratch 28 -> 208 B per lane)
      if (more) bc[kk] = bs[4 * kk * TILE];
    }
    ++s;
  }
  for (; s < nst; ++s) {
    // the queue here, oldest first: A(s) x 4, B(s) x 8 -- only the LDS-DMA ops have to be complete
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more = s + 1 < nst;
    if (more) issue_a(s + 1);
    const double* bs = bcol + src_of(more ? s + 1 : s);
    const double* As = lds + (s & 1) * AS;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + (l >> 4);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        acc[cb] = mfma64_nega(As[lt_off(k, 16 * (cb0 + cb) + (l & 15))], bc[kk], acc[cb]);
      // B of the next stage into the register this k-step has consumed: unconditional and pinned
      // behind its k-step (see above)
      __builtin_amdgcn_sched_barrier(0);
      bc[kk] = bs[4 * kk * TILE];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// The 36 lower blocks over 8 waves, by block-row pairs (q, 7 - q), q = W & 3: the pair's 9 blocks
// (7-q, 0 .. 7-q), (q, 0 .. q) in that order, the first 5 to wave q, the other 4 to wave q + 4 -- a
// wave's blocks share their rows, so it reads 4-6 of the 8 A fragments per k-step instead of all 8
// (round 4: the D-units' LDS reads per MFMA 1.78 -> 1.08; each block keeps its MFMA chain, so the
// sums are unchanged bit for bit).  syrk_e(W, i): packed index of wave W's i-th block, i < syrk_nb(W).
__host__ __device__ constexpr int syrk_nb(int W) { return W < 4 ? 5 : 4; }
__host__ __device__ constexpr int syrk_e(int W, int i) {
  const int q = W & 3, j = (W < 4) ? i : 5 + i, r1 = 8 - q;   // r1: blocks in row 7 - q
  return (j < r1) ? (7 - q) * (8 - q) / 2 + j : q * (q + 1) / 2 + (j - r1);
}
// every lower block exactly once
constexpr bool syrk_map_ok() {
  int seen[NPACK] = {};
  for (int W = 0; W < 8; ++W)
    for (int i = 0; i < syrk_nb(W); ++i) {
      const int e = syrk_e(W, i);
      if (e < 0 || e >= NPACK || seen[e]++) return false;
    }
  for (int e = 0; e < NPACK; ++e)
    if (seen[e] != 1) return false;
  return true;
}
static_assert(syrk_map_ok(), "SYRK block map must cover the 36 lower blocks once");

// SYRK of Lt stages restricted to the 36 lower blocks, 8 waves: wave W takes blocks syrk_e(W, i),
// i < syrk_nb(W); only the i in MASK (a diagonal-target slice).
// PART: from k-step ks on (the first stage of a run that starts past padding rows).
template <int W, int MASK, bool PART = false>
__device__ __forceinline__ void syrk_stage8(const double* As, v4d (&acc)[5], int l, int ks = 0) {
  constexpr int NBW = syrk_nb(W);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    if (PART && kk < ks) continue;
    const int k = 4 * kk + (l >> 4);
    double a8[8];   // the fragments no block of this wave uses are never loaded (dead)
#pragma unroll
    for (int q = 0; q < 8; ++q) a8[q] = As[lt_off(k, 16 * q + (l & 15))];
#pragma unroll
    for (int i = 0; i < NBW; ++i)
      if ((MASK >> i) & 1) acc[i] = mfma64(a8[tri_q(syrk_e(W, i))], a8[tri_s(syrk_e(W, i))], acc[i]);
  }
}

// block masks of the diagonal-target slices: all blocks; even i; odd i
__host__ __device__ constexpr int slice_mask(int sl) { return sl == 0 ? 0x1F : sl == 1 ? 0x15 : 0x0A; }

// SYRK of Lt rows restricted to the 36 lower blocks, 8 waves (wave W takes blocks syrk_e(W, i), i in
// slice_mask(sl)), on 32-row stages through a 2 x 32 KiB LDS-DMA ring: one barrier per 32 k rows.
// r0 (a multiple of 4): leading rows skipped, as in gemm1_a32 (zero padding columns of block
// column 0): whole stages, then the first stage computed from k-step (r0 & 31) / 4.
__device__ __forceinline__ void syrk_lower8_32(const double* __restrict__ src, int nst16, double* lds, v4d (&acc)[5],
                                               int sl = 0, int r0 = 0) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int AS = 32 * TILE;
  const int nst = nst16 >> 1;   // 8 x (number of Lt tiles): always even
  const int s0 = r0 >> 5, kf = (r0 & 31) >> 2;
  if (nst <= s0) return;
  auto issue = [&](int s) {
    double* slot = lds + (s & 1) * AS;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 4 * w + e;
      glds16_asm(src + (int64_t)s * AS + k * TILE + 2 * (l ^ (8 * (k & 1))), slot + k * TILE);
    }
  };
  issue(s0);
  const int ws = w + 8 * sl;   // wave-uniform (wave, slice) instantiation
#define SYRK_CASE(W, SL)                                    \
  case W + 8 * SL:                                          \
    syrk_stage8<W, slice_mask(SL)>(As, acc, l);             \
    syrk_stage8<W, slice_mask(SL)>(As + LTS, acc, l);       \
    break;
#define SYRK_PCASE(W, SL)                                                             \
  case W + 8 * SL:                                                                    \
    if (kf < 4) syrk_stage8<W, slice_mask(SL), true>(As, acc, l, kf);                 \
    syrk_stage8<W, slice_mask(SL), true>(As + LTS, acc, l, kf < 4 ? 0 : kf - 4);      \
    break;
#define SYRK_CASES(C, SL) C(0, SL) C(1, SL) C(2, SL) C(3, SL) C(4, SL) C(5, SL) C(6, SL) C(7, SL)
  int s = s0;
  if (kf > 0) {   // the next stage issued before this short stage's wait (as in gemm1_a32)
    if (s + 1 < nst) {
      issue(s + 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const double* As = lds + (s & 1) * AS;
    switch (ws) {
      SYRK_CASES(SYRK_PCASE, 0)
      SYRK_CASES(SYRK_PCASE, 1)
      SYRK_CASES(SYRK_PCASE, 2)
      default: break;
    }
    ++s;
  }
  for (; s < nst; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (s + 1 < nst) issue(s + 1);
    const double* As = lds + (s & 1) * AS;
    switch (ws) {
      SYRK_CASES(SYRK_CASE, 0)
      SYRK_CASES(SYRK_CASE, 1)
      SYRK_CASES(SYRK_CASE, 2)
      default: break;
    }
  }
#undef SYRK_CASES
#undef SYRK_PCASE
#undef SYRK_CASE
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// Packed-block store of a wave's SYRK accumulators (blocks W + 8i, i in the slice):
// dst[o] = base[o] - acc (base null: dst[o] = acc).
__device__ __forceinline__ void store_syrk_blocks(double* dst, const double* base, const v4d (&acc)[5], int sl) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int e = syrk_e(w, i);
    if (i < syrk_nb(w) && ((slice_mask(sl) >> i) & 1)) {
      const int q = tri_q_rt(e), sb = e - q * (q + 1) / 2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = pk(q, sb) + bo((l >> 4) + 4 * r, l & 15);
        double* d = dst + o;
        __builtin_nontemporal_store(base ? base[o] - acc[i][r] : acc[i][r], d);
      }
    }
  }
}

// S[b][Jt&1] = K_{Jt,Jt} - sum_{L < nterm} L_{Jt,L} L_{Jt,L}^T (packed blocks; the blocks of slice
// sl only), 8 waves: the diagonal target's partial sum.  K_{Jt,Jt} from Kd, or formed from the
// exact counts (kd: their loads issued before the SYRK, whose first wait covers them).
__device__ __forceinline__ void syrk_partial8(const CholArgs& a, int64_t b, int Jt, int nterm, double* lds, int sl) {
  const int w = threadIdx.x >> 6;
  v4d acc[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
  int2 kv[5];
  if (a.kd) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int e = syrk_e(w, i);
      kv[i] = (i < syrk_nb(w) && ((slice_mask(sl) >> i) & 1)) ? kd_load(a, b, Jt, e) : int2{0, 0};
    }
  }
  if (!(a.skip & 2)) syrk_lower8_32(a.L + b * l_stride(a.NT) + (int64_t)Jt * a.NT * TT, 8 * nterm, lds, acc, sl, skip_rows(a, b));
  double* dst = a.S + (b * NSLOT + (Jt & 1)) * (int64_t)NPACK * BLKD;
  if (!a.kd) {
    store_syrk_blocks(dst, a.Kd + (b * a.NT + Jt) * (int64_t)NPACK * BLKD, acc, sl);
    return;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int e = syrk_e(w, i);
    if (i < syrk_nb(w) && ((slice_mask(sl) >> i) & 1)) kd_block(a, b, Jt, e, kv[i], acc[i], dst);
  }
}

// ---------------------------------------------------------------------------
// diagonal tile
//   A. T = K_JJ - sum_{L<J} L_JL L_JL^T = Kd + partials; r = y_J - mu - w_J
//   C. for panel p: one wave factors T_pp (-> L_pp, X_pp = L_pp^{-1});
//      all waves: L_qp = T_qp X_pp^T (q > p); T_qs -= L_qp L_sp^T (q >= s > p)   [MFMA]
//   D. blocked inverse X = L^{-1}: X_{j+d,j} = -X_{j+d,j+d} sum_{l=j}^{j+d-1} L_{j+d,l} X_{l,j}
//      (off-diagonal X blocks written to / re-read from Dinv, diagonal ones stay in LDS)
//   E. write L_JJ^T (Lt tile), X_J^T (Dinv, zeros below its diagonal), z_J = X_J r
// ---------------------------------------------------------------------------
// X block (q, jb), q > jb, of X = L^{-1}: X_{q,jb} = -X_qq sum_{lb=jb}^{q-1} L_{q,lb} X_{lb,jb}
// (needs L row q and X rows jb..q-1, X_qq); one wave.
__device__ __forceinline__ void xinv_block(const double* Tp, double* Xp, int q, int jb, int l) {
  // two independent MFMA chains (even / odd lb) halve the dependent-accumulator latency
  v4d s0 = {0.0, 0.0, 0.0, 0.0}, s1 = {0.0, 0.0, 0.0, 0.0};
  int lb = jb;
  for (; lb + 1 < q; lb += 2) {
    const double* A0 = Tp + pk(q, lb);
    const double* B0 = Xp + pk(lb, jb);
    const double* A1 = Tp + pk(q, lb + 1);
    const double* B1 = Xp + pk(lb + 1, jb);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = 4 * kk + (l >> 4);
      s0 = mfma64(A0[bo(l & 15, k)], B0[bo(k, l & 15)], s0);
      s1 = mfma64(A1[bo(l & 15, k)], B1[bo(k, l & 15)], s1);
    }
  }
  if (lb < q) {
    const double* A0 = Tp + pk(q, lb);
    const double* B0 = Xp + pk(lb, jb);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = 4 * kk + (l >> 4);
      s0 = mfma64(A0[bo(l & 15, k)], B0[bo(k, l & 15)], s0);
    }
  }
  const v4d sacc = s0 + s1;
  v4d xo = {0.0, 0.0, 0.0, 0.0};
  const double* Xqq = Xp + pk(q, q);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) xo = mfma64_nega(Xqq[bo(l & 15, 4 * kk + (l >> 4))], sacc[kk], xo);
  double* dst = Xp + pk(q, jb);
#pragma unroll
  for (int r = 0; r < 4; ++r) dst[bo((l >> 4) + 4 * r, l & 15)] = xo[r];
}

// z_J[i] = sum_{c <= i} X[i][c] r[c] for the NTR right-hand sides: four lanes per row
// (c = q mod 4), shuffle-reduced.  One wave covers the 16 rows of block row qr (lane l: row
// 16 qr + (l >> 2), q = l & 3), so a block row's z can be formed as soon as its X blocks are final.
template <int NTR>
__device__ __forceinline__ void diag_z(const CholArgs& a, const double* Xp, const double (*rsh)[TILE], int64_t b,
                                       int64_t j0, int qr) {
  const int l = threadIdx.x & 63, ii = l >> 2, i = 16 * qr + ii, q = l & 3;
  double acc[NTR];
#pragma unroll
  for (int tr = 0; tr < NTR; ++tr) acc[tr] = 0.0;
  // c = q, q + 4, ... <= i in this order, one block (four c) per pass: the block's X and r loads
  // are in flight together instead of one LDS round trip per term (the lane's fma chain is
  // unchanged).  Blocks left of the diagonal hold only c <= i; the diagonal block's c > i are skipped.
#pragma unroll 1
  for (int cb = 0; cb < qr; ++cb) {
    const double* xb = Xp + pk(qr, cb);
    double xc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xc[j] = xb[bo(ii, q + 4 * j)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int tr = 0; tr < NTR; ++tr) acc[tr] += xc[j] * rsh[tr][16 * cb + q + 4 * j];
    }
  }
  for (int c = 16 * qr + q; c <= i; c += 4) {
    const double xc = Xp[pk(qr, qr) + bo(ii, c & 15)];
#pragma unroll
    for (int tr = 0; tr < NTR; ++tr) acc[tr] += xc * rsh[tr][c];
  }
#pragma unroll
  for (int tr = 0; tr < NTR; ++tr) {
    double v = acc[tr];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    if (q == 0) a.z[(b * NTR + tr) * a.ns + j0 + i] = v;
  }
}
__device__ __forceinline__ void diag_z_row(const CholArgs& a, const double* Xp, const double (*rsh)[TILE], int64_t b,
                                           int64_t j0, int qr) {
  if (a.skip & (1 << 15)) return;
  switch (a.nt) {
    case 1: diag_z<1>(a, Xp, rsh, b, j0, qr); break;
    case 2: diag_z<2>(a, Xp, rsh, b, j0, qr); break;
    case 3: diag_z<3>(a, Xp, rsh, b, j0, qr); break;
    default: diag_z<4>(a, Xp, rsh, b, j0, qr); break;
  }
}

// Block row qr of X into Dinv, each block transposed (block (q, jb) holds X_{q,jb}^T in the bo()
// layout): thread tid of nthr writes the 16-B pairs k = first pair of the row + tid, + nthr, ...,
// i.e. elements (r, c0), (r, c0 + 1) of block blk's transpose, read from X at bo(c0, r), bo(c0 + 1, r)
// (coalesced; the packed blocks of one row are contiguous).
__device__ __forceinline__ void dinv_store_row(const CholArgs& a, const double* Xp, double* Xg, int qr, int tid,
                                               int nthr) {
  if (a.skip & (1 << 14)) return;
  const int k0 = pk(qr, 0) / 2, k1 = pk(qr, qr + 1) / 2;
  for (int k = k0 + tid; k < k1; k += nthr) {
    const int g = 2 * k, blk = g >> 8, o = g & 255, r = o >> 4;
    const int c0 = 2 * (((o & 15) >> 1) ^ ((r >> 1) & 7));
    const double* xb = Xp + blk * BLKD;
    *reinterpret_cast<v2d*>(Xg + g) = v2d{xb[bo(c0, r)], xb[bo(c0 + 1, r)]};
  }
}

// Waves of a diagonal workgroup beyond the SYRK's eight: the barriers of syrk_lower8_32 (same
// arguments), nothing else.
__device__ __forceinline__ void syrk_lower8_32_bystander(int nst16, int r0 = 0) {
  const int nst = nst16 >> 1, s0 = r0 >> 5, kf = (r0 & 31) >> 2;
  if (nst <= s0) return;
  int s = s0;
  if (kf > 0) {
    __builtin_amdgcn_s_barrier();
    ++s;
  }
  for (; s < nst; ++s) __builtin_amdgcn_s_barrier();
  __syncthreads();
}

// Rank of worker wave w (1 .. NW-1) of a diagonal workgroup: 8 waves in wave order; more waves:
// the waves off wave 0's SIMD first (w & 3 != 0), then its SIMD mates 4, 8, ...
template <int NW>
__device__ __forceinline__ int diag_rank(int w) {
  if constexpr (NW == DW) return w - 1;
  return (w & 3) ? 3 * (w >> 2) + (w & 3) - 1 : 3 * (NW / 4) + (w >> 2) - 1;
}

// Diagonal tile J of individual b.  T = S - sum_{L0 <= L < J} L_JL L_JL^T where S is
// K_JJ - sum_{L < L0} (the buffer slot J&1 left by an earlier off-diagonal launch) when
// L0 > 0, else k_diag_grm's K_JJ.
// LDS (lds >= 2 * NPACK * BLKD doubles = 144 KiB): Tp = T -> L (packed lower 16x16 blocks),
// Xp = X = L^{-1} in the same packed layout; before the factorisation Xp's space is the
// 64 KiB SYRK stage ring.  X never round-trips through global memory: Dinv receives X^T
// block row by block row, as the rows become final.
//
// NW waves (DW, or DWX in the launches without D- / E-units).  Phase A runs on waves < DW whatever
// NW; the factorisation windows spread their off-chain work over the workers, waves 1 .. NW-1 in
// rank order (diag_rank: wave 0's SIMD mates last).  Window p (block (p, p) factored, X_pp in LDS):
//   wave 0  : L_{p+1,p} = T_{p+1,p} X_pp^T                                        | barrier a_p |
//             T_{p+1,p+1} -= L_{p+1,p} L_{p+1,p}^T, factor16 of block (p+1, p+1)  | barrier w_p
//   workers : L_qp, q > p+1                                                       | barrier a_p |
//             trailing blocks T_qs -= L_qp L_sp^T; X block row p (xinv_block);
//             block row p-1 of X^T into Dinv and its 16 rows of z                 | barrier w_p
// so the pivot chain is one L block, one update and factor16 per window, and after the last window
// only the last block row of X, its store and its z remain (row NBLK-2's store and z beside them).
// Every block keeps its MFMA chain and every z row its fma order whichever wave takes it, so the
// results do not depend on NW.
template <int NW>
__device__ __forceinline__ void diag_tile(const CholArgs& a, int64_t b, int J, int L0, double* lds,
                                          double (*rsh)[TILE]) {
  constexpr int NTHR = 64 * NW;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  // the wave's role from a scalar: those branches are then scalar too, so every wave meets each
  // barrier in exactly one of them
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const int64_t ns = a.ns;
  const int NT = a.NT;
  const int64_t j0 = (int64_t)J * TILE;
  const double* sc = a.scal + b * SCAL;
  const double muf = sc[SC_MUF];
  const int64_t nrow = (int64_t)sc[SC_NROW], pad = (int64_t)sc[SC_PAD];
  const int nt = a.nt;
  double* Tp = lds;
  double* Xp = lds + NPACK * BLKD;
  dstamp(a, 0);

  // forward-substitution right-hand side r = rhs_J - w_J: loads issued first so that their
  // latency overlaps the S load and the SYRK
  double rv[MAXT] = {0.0, 0.0, 0.0, 0.0};
  const int64_t gi = j0 + t;
  if (t < TILE) {
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr) {
      if (tr < nt) {
        const int64_t o = (b * nt + tr) * ns + gi;
        const double wv = (J > 0) ? a.w[o] : 0.0;
        const int fo = fold_of(a.ft, b);   // the system's split (fold-fused batches)
        rv[tr] = ((a.form == FORM_PRIMAL) ? a.rhs[o] : a.ft.yT[fo][tr * a.ytp + gi] - muf * a.ft.ymu[fo][tr]) - wv;
      }
    }
  }

  // T = S - sum_{L0 <= L < J} L_JL L_JL^T: S by LDS-DMA, the SYRK through the stage ring.
  // (Streaming the whole Lt tile in one burst, or 4 stages in flight, measured slower: the
  // launch's loads are HBM-bound and the SYRK at 2 waves per SIMD then runs after them.)
  const double* src = (L0 == 0) ? a.Kd + (b * NT + J) * (int64_t)NPACK * BLKD
                                : a.S + (b * NSLOT + (J & 1)) * (int64_t)NPACK * BLKD;
  const bool aw = NW == DW || wu < DW;   // phase A's loads and SYRK: the first DW waves
  {
    if (aw) {
#pragma unroll
      for (int e = 0; e < NPACK * BLKD / 2 / DTHR; ++e) {   // 9 x 16 B per thread
        const int chunk = (e * DW + w) * 64;
        __builtin_amdgcn_global_load_lds(src + 2 * (chunk + l), (lds_ptr_t)(Tp + 2 * chunk), 16, 0, 2);   // aux 2: non-temporal
      }
    }
    if (J > L0 && a.q != nullptr) {
      // last-term mode: Q = L_{J,J-1} L_{J,J-1}^T came with launch J-1's tile (J, J-1)
      const double* qg = a.q + b * (int64_t)NPACK * BLKD;
      if (aw) {
#pragma unroll
        for (int e = 0; e < NPACK * BLKD / 2 / DTHR; ++e) {
          const int chunk = (e * DW + w) * 64;
          __builtin_amdgcn_global_load_lds(qg + 2 * (chunk + l), (lds_ptr_t)(Xp + 2 * chunk), 16, 0, 0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      for (int e = t; e < NPACK * BLKD; e += NTHR) Tp[e] -= Xp[e];
      __syncthreads();
    } else if (J > L0 && !(a.skip & 2)) {
      if (aw) {
        v4d acc[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
        // waits for all its stages (and the older S loads) and ends in a barrier
        // (no padding skip here: at J = 1 only, and it keeps the peeled stage out of this kernel)
        syrk_lower8_32(a.L + b * l_stride(NT) + ((int64_t)J * NT + L0) * TT, 8 * (J - L0), Xp, acc);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const int e = syrk_e(w, i);
          if (i < syrk_nb(w)) {
            const int q = tri_q_rt(e);
            double* blk = Tp + pk(q, e - q * (q + 1) / 2);
#pragma unroll
            for (int r = 0; r < 4; ++r) blk[bo((l >> 4) + 4 * r, l & 15)] -= acc[i][r];
          }
        }
      } else {
        syrk_lower8_32_bystander(8 * (J - L0));
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  // X's diagonal blocks start as the reversed identity (factor16's inverse rows load it); the
  // SYRK ring that shared their space is drained
#pragma unroll
  for (int e = t; e < NBLK * BLKD; e += NTHR) {
    const int p = e >> 8, o = e & 255, r = o >> 4;
    const int c = 2 * (((o & 15) >> 1) ^ ((r >> 1) & 7)) + (o & 1);   // bo(r, c) == o
    Xp[pk(p, p) + o] = (c == NB - 1 - r) ? 1.0 : 0.0;
  }
  if (t < TILE) {
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr) rsh[tr][t] = (tr < nt && sys_real(gi, pad, nrow)) ? rv[tr] : 0.0;
  }
  dstamp(a, 1);
  __syncthreads();
  dstamp(a, 2);

  // C. blocked right-looking factorisation over 16-column panels.  Wave 0 is the pivot chain: it
  //    forms the one L block the next pivot block needs, updates that block and factors it; the
  //    workers take the rest of panel p's L column, the trailing update and the X rows.
  const int rk = diag_rank<NW>(wu);
  constexpr int NWK = NW - 1;                                   // workers
  constexpr int ZR = NW == DW ? NWK - 1 : 3 * (NW / 4) - 1;     // wave NW-1's rank: rows of X^T and z
  double* Xg = a.Dinv + (b * NT + J) * (int64_t)NPACK * BLKD;
  constexpr int LR = NBLK - 1;
  auto upd_next = [&](int p) {   // T_{p+1,p+1} -= L_{p+1,p} L_{p+1,p}^T
    v4d x = {0.0, 0.0, 0.0, 0.0};
    x = mma_abt(Tp + pk(p + 1, p), Tp + pk(p + 1, p), x, l);
    double* dst = Tp + pk(p + 1, p + 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[bo((l >> 4) + 4 * r, l & 15)] -= x[r];
  };
  if (!(a.skip & 4)) {
    if (wu == 0 && !(a.skip & 256)) factor16_any<NW == DW>(a, Tp + pk(0, 0), Xp + pk(0, 0), l);
    __syncthreads();
  }
  for (int p = 0; p + 1 < ((a.skip & 4) ? 0 : NBLK); ++p) {
    // L column of panel p: block (p+1, p) on wave 0, block (p+2+r, p) on the worker of rank r
    const int qc = (wu == 0) ? p + 1 : p + 2 + rk;
    if (qc < ((a.skip & 512) ? 0 : NBLK)) {
      v4d x = {0.0, 0.0, 0.0, 0.0};
      x = mma_abt(Tp + pk(qc, p), Xp + pk(p, p), x, l);
#pragma unroll
      for (int r = 0; r < 4; ++r) Tp[pk(qc, p) + bo((l >> 4) + 4 * r, l & 15)] = x[r];
    }
    dstamp(a, 3 + 3 * p);
    __syncthreads();   // a_p: L column p complete (the workers read L_{p+1,p} too)
    const int nb = NBLK - 1 - p;
    if (wu == 0) {
      uint64_t* st = (a.dtr && blockIdx.x == 0 && p == 3) ? a.dtr : nullptr;
      fstamp(st, 54);
      // (after the barrier: its own L block is back in LDS, and the workers start their trailing
      // blocks an update earlier; before the barrier measured even)
      if (!(a.skip & 512)) upd_next(p);
      if (!(a.skip & 256)) factor16_any<NW == DW>(a, Tp + pk(p + 1, p + 1), Xp + pk(p + 1, p + 1), l, st);
    } else {
      // trailing blocks e = 1 .. nb(nb+1)/2 - 1 (e = 0 is block (p+1, p+1)).  8 waves: over all
      // seven workers, which then take the X blocks and the finished row.  More waves: ranks < p
      // build X row p, the ranks from p up to ZR take the trailing blocks; wave 0's SIMD mates (the
      // ranks past ZR) run no MFMA beside factor16 (with trailing blocks on them: +0.7% per step).
      int ti = rk, ntw = NWK;
      if constexpr (NW != DW) {
        ntw = ZR - p;
        ti = (rk < ZR) ? rk - p : -1;
      }
      // two blocks per pass: independent MFMA chains and LDS traffic overlap
      const int ne = (a.skip & 512) ? 0 : nb * (nb + 1) / 2;
      for (int e = ti + 1; ti >= 0 && e < ne; e += 2 * ntw) {
        const int e2 = e + ntw;
        int qq = 0;
        while ((qq + 1) * (qq + 2) / 2 <= e) ++qq;
        const int q = p + 1 + qq, sb = p + 1 + (e - qq * (qq + 1) / 2);
        const bool two = e2 < ne;
        int qq2 = qq;
        while ((qq2 + 1) * (qq2 + 2) / 2 <= e2) ++qq2;
        const int q2 = two ? p + 1 + qq2 : q, sb2 = two ? p + 1 + (e2 - qq2 * (qq2 + 1) / 2) : sb;
        const double* A = Tp + pk(q, p);
        const double* B = Tp + pk(sb, p);
        const double* A2 = Tp + pk(q2, p);
        const double* B2 = Tp + pk(sb2, p);
        v4d x = {0.0, 0.0, 0.0, 0.0}, x2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int k = 4 * kk + (l >> 4);
          x = mfma64(A[bo(l & 15, k)], B[bo(l & 15, k)], x);
          x2 = mfma64(A2[bo(l & 15, k)], B2[bo(l & 15, k)], x2);
        }
        double* dst = Tp + pk(q, sb);
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[bo((l >> 4) + 4 * r, l & 15)] -= x[r];
        if (two) {
          double* dst2 = Tp + pk(q2, sb2);
#pragma unroll
          for (int r = 0; r < 4; ++r) dst2[bo((l >> 4) + 4 * r, l & 15)] -= x2[r];
        }
      }
      // D (overlapped). block row p of X = L^{-1}: L row p and X rows < p are final and
      // X_pp came out of the previous window's factor16
      if (!(a.skip & 8) && rk < p) xinv_block(Tp, Xp, p, rk, l);
      // E (overlapped). block row p-1 of X is final since barrier w_{p-1}: into Dinv, and its z.
      // z (fp64 VALU) on rank ZR, off wave 0's SIMD; the store there too, or (wide workgroup)
      // over wave 0's mates, which it costs LDS reads and stores only
      if (p >= 1 && !(a.skip & 8)) {
        if (NW == DW && rk == ZR) dinv_store_row(a, Xp, Xg, p - 1, l, 64);
        if (NW != DW && rk > ZR) dinv_store_row(a, Xp, Xg, p - 1, 64 * (rk - ZR - 1) + l, 64 * (NWK - 1 - ZR));
        if (rk == ZR) diag_z_row(a, Xp, rsh, b, j0, p - 1);
      }
    }
    dstamp(a, 4 + 3 * p);
    __syncthreads();
    dstamp(a, 5 + 3 * p);
  }
  if (a.skip & 16) return;

  // D. last block row of X (rows < NBLK-1 were built inside the factorisation windows), beside it
  //    block row NBLK-2 into Dinv
  if (!(a.skip & 4) && !(a.skip & 8)) {
    const int jb = (NW == DW) ? wu : (wu == 0 ? LR : rk);
    if (jb < LR) xinv_block(Tp, Xp, LR, jb, l);
    // (8 waves: the one wave without an X block; wide: wave 0 and the ranks past the X blocks')
    if (NW == DW && wu == NW - 1) dinv_store_row(a, Xp, Xg, LR - 1, l, 64);
    if (NW != DW && (wu == 0 || rk >= LR))
      dinv_store_row(a, Xp, Xg, LR - 1, 64 * (wu == 0 ? 0 : rk - LR + 1) + l, 64 * (NW - LR));
    dstamp(a, 26);
    __syncthreads();
    dstamp(a, 27);
  }

  // E. X into Dinv as packed lower blocks, each block transposed (block (q, jb) holds
  //    X_{q,jb}^T in the bo() layout), z_J = X r, and L_JJ^T only for the debug readback.
  if (NW == DW && (a.skip & FLAG_WRITE_LJJ)) {   // (the debug path runs the 8-wave kernel: launch_chol_diag)
    double* Ld = a.L + b * l_stride(NT) + ((int64_t)J * NT + J) * TT;
    for (int e = t; e < TT; e += NTHR) {
      const int rr = e >> 7, cc = e & 127;
      Ld[e] = (cc >= rr) ? Tp[pk(cc >> 4, rr >> 4) + bo(cc & 15, rr & 15)] : 0.0;
    }
  }
  // what is left: z of block rows NBLK-2 and NBLK-1 on the last two waves (two SIMDs, neither
  // wave 0's), the last row's eight blocks of X^T over the others
  if (wu == NW - 1)
    diag_z_row(a, Xp, rsh, b, j0, LR - 1);
  else if (wu == NW - 2)
    diag_z_row(a, Xp, rsh, b, j0, LR);
  else
    dinv_store_row(a, Xp, Xg, LR, t, 64 * (NW - 2));
  dstamp(a, 28);
}

// ---------------------------------------------------------------------------
// Off-diagonal launch of column J: one 8-wave workgroup per unit, two per CU (LDS <= 72 KiB).
//   T-unit, tile (I, J), I > J:
//     0. acc = K_JI in the f64 accumulator layout: from the system-tile launches' counts (either form) or int8
//        MFMA here (rows permuted so the counts land in the f64 layout) -- or, when launch J-1 ran
//        ahead, its partial sum K_JI - sum_{L<J-1} L_JL L_IL^T
//     1. acc -= sum_{L} L_JL L_IL^T over the L < J not summed yet   (acc = T^T, wave w: its 16 i)
//     2. out^T[jb] = sum_{cb<=jb} X[jb][cb] T^T[cb]   (X = inv(L_JJ); acc is the B operand)
//        -> Lt tile (I, J); w_I += L_IJ z_J
//   P-unit (ahead), tile (I, J+1), I >= J+2, row blocks of slice rs: acc = K - sum_{L<J} (steps 0-1
//     of launch J+1's T-unit, which continues the same MFMA chains: bit-identical results)
//   D-unit, diagonal tile J+1, block slice: S = K - sum_{L<J} L_{J+1,L} L_{J+1,L}^T (packed blocks)
// ---------------------------------------------------------------------------

// K_{I,Jt} (the T^T layout of tile (I, Jt)) for the NCB row blocks from cb0: exact counts of
// the system-tile launches (loads issued by kc_issue) or, NCB = 8 only, the int8 tile here.
template <int NCB>
__device__ __forceinline__ void kc_issue(const CholArgs& a, int64_t b, int I, int Jt, int cb0, int2 (&kcv)[NCB]) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int16_t* kt = a.kc + kc_tile(a.NT, b, I, Jt) + w * 8 * 64 * 4;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) kcv[cb] = nt_load2(kt + ((cb0 + cb) * 64 + l) * 4);
}

// K_ij = (c - (u_i + u_j) sa - u_i u_j sm + cN) / d regrouped around the column j: c / d + P_j u_i +
// Q_j, P_j = -(sa + sm u_j) / d, Q_j = (cN - sa u_j) / d, with P_j = Q_j = 0 on padding columns (whose
// counts are 0): per element an LDS pair, a conversion and two fmas, where the plain formula took
// seven fp64 ops and a 64-bit compare -- an fp64 VALU op waits for the matrix pipe while the CU's
// other waves stream MFMAs (gfx950 does not dual-issue them).  Only the off-diagonal tiles' K comes
// from here (T-, P- and E-units alike), so every schedule agrees.  k_stage (threads t < TILE, before
// the unit's barrier): the column pairs of tile Jt and the row sums u_i of tile I.
__device__ __forceinline__ void k_stage(const CholArgs& a, int64_t b, int64_t i0, int64_t j0, double* pq_sh,
                                        double* ui_sh) {
  const int t = threadIdx.x;
  if (t < TILE) {
    const double* sc = a.scal + b * SCAL;
    const double sa = sc[SC_SA], cN = sc[SC_CN], invd = sc[SC_INVD], sm = sc[SC_SM];
    const int64_t nrow = (int64_t)sc[SC_NROW], pad = (int64_t)sc[SC_PAD];
    const double uj = a.u[b * a.prow + j0 + t];
    const bool rj = sys_real(j0 + t, pad, nrow);
    reinterpret_cast<v2d*>(pq_sh)[t] = rj ? v2d{-invd * (sa + sm * uj), invd * (cN - sa * uj)} : v2d{0.0, 0.0};
    ui_sh[t] = a.u[b * a.prow + i0 + t];
  }
}

// GSH: the kernel-form path may read shared fold counts (FoldTab::gsh); the diagonal kernel's E-units
// are built without it (E-units are not planned for such chunks: run_chunk), which keeps that
// latency-bound kernel's code as it was
template <int NCB, bool GSH = true>
__device__ __forceinline__ void k_acc(const CholArgs& a, int64_t b, int I, int Jt, int cb0, const int2 (&kcv)[NCB],
                                      uint8_t* lds8, const double* pq_sh, const double* ui_sh, v4d (&acc)[NCB]) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)Jt * TILE;
  const double* sc = a.scal + b * SCAL;
  const double invd = sc[SC_INVD];
  const int64_t nrow = (int64_t)sc[SC_NROW], pad = (int64_t)sc[SC_PAD];
  const int il = 16 * w + (l & 15);
  const bool ireal = sys_real(i0 + il, pad, nrow);
  const double ui = ui_sh[il];
  const v2d* pq = reinterpret_cast<const v2d*>(pq_sh);
  if (a.kc) {
    // counts issued before the u / z loads landed; exact ints -> fp64 K
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      // (written out, not unpack_counts4: with it the compiler reorders k_chol_diag's register setup)
      const int32_t c4[4] = {(int32_t)(int16_t)(kcv[cb].x & 0xffff), (int32_t)(int16_t)(kcv[cb].x >> 16),
                             (int32_t)(int16_t)(kcv[cb].y & 0xffff), (int32_t)(int16_t)(kcv[cb].y >> 16)};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cl = 16 * (cb0 + cb) + (l >> 4) + 4 * r;
        const v2d q = pq[cl];
        const double v = __builtin_fma((double)c4[r], invd, __builtin_fma(q[0], ui, q[1]));
        acc[cb][r] = ireal ? v : 0.0;
      }
    }
    return;
  }
  if constexpr (NCB == 8) {
    v4i cnt[8];
    const int64_t nblk = (int64_t)sc[SC_CBLK];
    if (GSH && !(a.skip & 32) && a.form != FORM_PRIMAL && a.ft.gsh) {
      // kernel-form folds: the counts of the individual's shared A_R A_R^T (same integers)
#pragma unroll
      for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt[cb][r] = gsh_count(a, b, j0 + 16 * cb + (l >> 4) + 4 * r, i0 + il);
    } else if (!(a.skip & 32)) {
      // 2-bit packed rows of either form: the SNP form's split rows, the kernel form's gathered panel
      const int row = 16 * w + (l >> 2), pos = l & 3;
      const bool pf = a.form == FORM_PRIMAL;
      const uint8_t* sa = (pf ? row_packed(a, b, j0 + row) : row_dpk(a, b, j0 + row)) + pk_swz_a(row, pos);
      const uint8_t* sb = (pf ? row_packed(a, b, i0 + row) : row_dpk(a, b, i0 + row)) + pk_swz_b(row, pos);
      i8_tt2d_pk64<4>(sa, sb, nblk, lds8, cnt);
    } else {
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) cnt[cb] = v4i{0, 0, 0, 0};
    }
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cl = 16 * cb + (l >> 4) + 4 * r;
        const v2d q = pq[cl];
        const double v = __builtin_fma((double)cnt[cb][r], invd, __builtin_fma(q[0], ui, q[1]));
        acc[cb][r] = ireal ? v : 0.0;
      }
    }
  }
}

// Partial sums of launch J+1's tiles, acc layout: [slot Jt&1][b][I][wave][cb][lane][4]
__device__ __forceinline__ double* part_ptr(const CholArgs& a, int64_t b, int I, int Jt) {
  return a.part + (((int64_t)(Jt & 1) * a.B + b) * a.NT + I) * TT + (threadIdx.x >> 6) * 8 * 64 * 4;
}

// P-unit: acc = K_{I,J+1} - sum_{L<J} L_{J+1,L} L_{I,L}^T for row blocks [cb0, cb0 + NCB).
template <int NCB>
__device__ __forceinline__ void part_unit(const CholArgs& a, int64_t b, int I, int rs, double* lds, double* uj_sh,
                                          double* ui_sh) {
  const int t = threadIdx.x, l = t & 63;
  const int J = a.J, Jt = J + 1, NT = a.NT, cb0 = rs * NCB;
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)Jt * TILE;
  int2 kcv[NCB];
  if (a.kc) kc_issue<NCB>(a, b, I, Jt, cb0, kcv);
  k_stage(a, b, i0, j0, uj_sh, ui_sh);
  __syncthreads();
  v4d acc[NCB];
  k_acc<NCB>(a, b, I, Jt, cb0, kcv, reinterpret_cast<uint8_t*>(lds), uj_sh, ui_sh, acc);
  const double* Lb = a.L + b * l_stride(NT);
  if (!(a.skip & 64))
    gemm1_a32<NCB>(Lb + (int64_t)Jt * NT * TT, Lb + (int64_t)I * NT * TT, J, cb0, lds, acc, skip_rows(a, b));
  double* pd = part_ptr(a, b, I, Jt);
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    v2d* d = reinterpret_cast<v2d*>(pd + ((cb0 + cb) * 64 + l) * 4);
    __builtin_nontemporal_store(v2d{acc[cb][0], acc[cb][1]}, d);
    __builtin_nontemporal_store(v2d{acc[cb][2], acc[cb][3]}, d + 1);
  }
}

// T-unit: tile (I, J).
template <int NTR>   // traits the w update runs over: 1, or MAXT (the zero traits' FMAs wait on the matrix pipe too)
__device__ __forceinline__ void tile_unit(const CholArgs& a, int64_t b, int I, int ahead_cur, int edone, double* lds,
                                          double* uj_sh, double* ui_sh, double (*zj_sh)[TILE], WgTrace& tr) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int J = a.J, NT = a.NT;
  const int64_t ns = a.ns;
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)J * TILE;
  const double* Lb = a.L + b * l_stride(NT);
  v4d acc[8];
  int2 kcv[8];
  const bool from_part = ahead_cur || edone;
  if (from_part) {
    const double* pd = part_ptr(a, b, I, J);
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      const v2d* s2 = reinterpret_cast<const v2d*>(pd + (cb * 64 + l) * 4);
      const v2d lo = __builtin_nontemporal_load(s2), hi = __builtin_nontemporal_load(s2 + 1);
      acc[cb] = v4d{lo[0], lo[1], hi[0], hi[1]};
    }
  } else if (a.kc) {
    kc_issue<8>(a, b, I, J, 0, kcv);
  }
  if (!from_part) k_stage(a, b, i0, j0, uj_sh, ui_sh);
  if (t < TILE) {
#pragma unroll
    for (int tr = 0; tr < MAXT; ++tr)
      zj_sh[tr][t] = (tr < a.nt) ? a.z[(b * a.nt + tr) * ns + j0 + t] : 0.0;
  }
  __syncthreads();
  if (!from_part) k_acc<8>(a, b, I, J, 0, kcv, reinterpret_cast<uint8_t*>(lds), uj_sh, ui_sh, acc);
  tr.mark(0);

  // 1. T^T = K_JI - sum_L L_JL L_IL^T over the L not summed by launch J-1 or this tile's E-unit
  const int Ls = (ahead_cur ? J - 1 : 0) + edone;
  if (J > Ls && !(a.skip & 64))
    gemm1_a32<8>(Lb + (int64_t)J * NT * TT + (int64_t)Ls * TT, Lb + (int64_t)I * NT * TT + (int64_t)Ls * TT, J - Ls, 0,
                 lds, acc, Ls == 0 ? skip_rows(a, b) : 0);
  tr.mark(1);

  // 2. L_IJ^T = X T^T by 16-row blocks of X (X[j][c] = 0 for c > j).  Dinv holds X in the
  //    packed block layout (blocks transposed): all 36 blocks (72 KiB) land in LDS in one
  //    LDS-DMA burst, then the 8 block rows run without further waits.
  double* Lout = const_cast<double*>(Lb) + ((int64_t)I * NT + J) * TT;
  double* xl = lds;
  {
    const double* Xg = a.Dinv + (b * NT + J) * (int64_t)NPACK * BLKD;
#pragma unroll
    for (int e = 0; e < NPACK * BLKD / 2 / OTH; ++e) {   // 9 x 16 B per thread
      const int chunk = (e * OW + w) * 64;
      __builtin_amdgcn_global_load_lds(Xg + 2 * (chunk + l), (lds_ptr_t)(xl + 2 * chunk), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  tr.mark(2);
  double wacc[MAXT] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int jb = 0; jb < NBLK; ++jb) {
    v4d o = {0.0, 0.0, 0.0, 0.0};
    if (!(a.skip & 128)) {
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        if (cb <= jb) {
          const double* xb = xl + pk(jb, cb);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) o = mfma64(xb[bo(4 * kk + (l >> 4), l & 15)], acc[cb][kk], o);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jl = 16 * jb + (l >> 4) + 4 * r, il = 16 * w + (l & 15);
      double* d = Lout + jl * TILE + il;
      __builtin_nontemporal_store(o[r], d);
#pragma unroll
      for (int tr = 0; tr < NTR; ++tr) wacc[tr] += o[r] * zj_sh[tr][jl];
    }
  }
  // w_I[i] += sum_j L_IJ[i][j] z_J[j]: reduce the 4 lane groups that share a column i
#pragma unroll
  for (int tr = 0; tr < NTR; ++tr) {
    if (tr < a.nt) {
      double v = wacc[tr];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if ((l >> 4) == 0) {
        const int64_t gi = (b * a.nt + tr) * ns + i0 + 16 * w + l;
        a.w[gi] = (J == 0) ? v : a.w[gi] + v;
      }
    }
  }
  // last-term mode: the diagonal tile J+1's last SYRK term L_{J+1,J} L_{J+1,J}^T from the tile
  // just stored (read back through the same stage ring and MFMA chains the diagonal kernel would
  // run, so its T = S - Q is bit-identical)
  if (a.q != nullptr && I == J + 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    v4d qa[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) qa[i] = v4d{0.0, 0.0, 0.0, 0.0};
    syrk_lower8_32(Lout, 8, lds, qa, 0, J == 0 ? skip_rows(a, b) : 0);
    store_syrk_blocks(a.q + b * (int64_t)NPACK * BLKD, nullptr, qa, 0);
  }
}

// E-unit (diagonal launch J, on a CU its other workgroups leave idle): the GEMM1 term L = ls0 of tile
// (I, J) -- from K_JI (ls0 = 0) or from launch J-1's partial over L < J-1 (ls0 = J-1) -- into the
// partial-sum slot J&1, where launch J's T-unit picks it up (OffPlan::ne).  The same k_acc start and
// gemm1_a32 MFMA chains as the T-unit, split after the term: bit-identical.
__device__ __forceinline__ void e_unit(const CholArgs& a, int64_t b, int I, int ls0, double* lds) {
  const int t = threadIdx.x, l = t & 63;
  const int J = a.J, NT = a.NT;
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)J * TILE;
  double* uj_sh = lds + NPACK * BLKD;   // past the GEMM1 ring (2 x 32 KiB) and k_acc's int8 ring
  double* ui_sh = uj_sh + 2 * TILE;
  double* pd = part_ptr(a, b, I, J);
  v4d acc[8];
  if (ls0 > 0) {
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      const v2d* s2 = reinterpret_cast<const v2d*>(pd + (cb * 64 + l) * 4);
      const v2d lo = __builtin_nontemporal_load(s2), hi = __builtin_nontemporal_load(s2 + 1);
      acc[cb] = v4d{lo[0], lo[1], hi[0], hi[1]};
    }
  } else {
    int2 kcv[8];
    if (a.kc) kc_issue<8>(a, b, I, J, 0, kcv);
    k_stage(a, b, i0, j0, uj_sh, ui_sh);
    __syncthreads();
    k_acc<8, false>(a, b, I, J, 0, kcv, reinterpret_cast<uint8_t*>(lds), uj_sh, ui_sh, acc);
  }
  const double* Lb = a.L + b * l_stride(NT);
  if (!(a.skip & 64))
    gemm1_a32<8>(Lb + (int64_t)J * NT * TT + (int64_t)ls0 * TT, Lb + (int64_t)I * NT * TT + (int64_t)ls0 * TT, 1, 0, lds,
                 acc, ls0 == 0 ? skip_rows(a, b) : 0);
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    v2d* d = reinterpret_cast<v2d*>(pd + (cb * 64 + l) * 4);
    __builtin_nontemporal_store(v2d{acc[cb][0], acc[cb][1]}, d);
    __builtin_nontemporal_store(v2d{acc[cb][2], acc[cb][3]}, d + 1);
  }
}

// Diagonal tile J of every individual: for J >= 2 the previous off-diagonal launch left
// K_JJ - sum_{L < J-1} in S[J&1], and the L = J-1 term is subtracted here.  Grid: the B diagonal
// workgroups, then nd D-units, then ne E-units (OffPlan).
__global__ __launch_bounds__(DTHR) void k_chol_diag(CholArgs a, int64_t ne, int ls0) {
  __shared__ __attribute__((aligned(16))) double lds[2 * NPACK * BLKD];   // 144 KiB: T/L and X
  __shared__ double rsh[MAXT][TILE];
  WgTrace tr(a.wgt);
  if ((int64_t)blockIdx.x >= a.B) {
    const int64_t x = blockIdx.x - a.B, nd = gridDim.x - a.B - ne;
    if (x < nd) {
      // OffPlan::ndd: the D-unit of diagonal target J+1 (S = K - sum_{L<J}), on a CU the diagonal
      // workgroups (dispatched first) leave idle; blocks B + x and x share an XCD when 8 | B
      const int64_t b = xcd_remap(x, nd);
      syrk_partial8(a, b, a.J + 1, a.J, lds, 0);
      tr.done(WGT_DPREP, a.J, a.J + 1, b);
    } else {
      const int64_t lg = xcd_remap(x - nd, ne);
      const int64_t b = lg % a.B;
      const int I = a.J + 1 + (int)(lg / a.B);
      e_unit(a, b, I, ls0, lds);
      tr.done(WGT_EPART, a.J, I, b);
    }
    return;
  }
  // individual b on the XCD that runs its off-diagonal tiles (same L2 for L, S, X, w)
  const int64_t b = xcd_remap(blockIdx.x, a.B);
  diag_tile<DW>(a, b, a.J, a.J >= 2 ? a.J - 1 : 0, lds, rsh);
  tr.done(WGT_DIAG, a.J, a.J, b);
}

// The same diagonal tile on NW waves, for the launches with no D- or E-units beside the B diagonal
// workgroups (every launch at B >= the CU count): the workgroup has its CU to itself (LDS), and the
// extra waves give the windows' off-chain work slack (diag_tile).
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_chol_diag_w(CholArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[2 * NPACK * BLKD];   // 144 KiB: T/L and X
  __shared__ double rsh[MAXT][TILE];
  WgTrace tr(a.wgt);
  const int64_t b = xcd_remap(blockIdx.x, a.B);
  diag_tile<NW>(a, b, a.J, a.J >= 2 ? a.J - 1 : 0, lds, rsh);
  tr.done(WGT_DIAG, a.J, a.J, b);
}

// K_JJ for every (individual, J) with the off-diagonal kernel's 8-wave int8 tile (A = B =
// the rows of tile J, output in the f64 accumulator layout: a wave holds the 16 columns of
// one column block, MFMAs only for the lower row blocks), exact counts + fp64 centring,
// + lambda I, identity on padded rows; packed lower 16x16 blocks into Kd[b][J].  J = 0, 1 run in
// k_diag_grm8 before the column loop; J >= 2 are extra workgroups at the end of the column-0
// off-diagonal launch (they fill its last round; the first reader is column 1's preparation).
__device__ __forceinline__ void diag_grm_tile(const CholArgs& a, int64_t b, int J, uint8_t* lds, double* u_sh) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int NT = a.NT;
  const int64_t j0 = (int64_t)J * TILE;
  const double* sc = a.scal + b * SCAL;
  const double sa = sc[SC_SA], cN = sc[SC_CN], invd = sc[SC_INVD], lam = sc[SC_LAM], sm = sc[SC_SM];
  const int64_t nrow = (int64_t)sc[SC_NROW], nblk = (int64_t)sc[SC_CBLK], pad = (int64_t)sc[SC_PAD];
  if (t < TILE) u_sh[t] = a.u[b * a.prow + j0 + t];
  double* Kd = a.Kd + (b * NT + J) * (int64_t)NPACK * BLKD;
  v4i cnt[8];
  const int row = 16 * w + (l >> 2), pos = l & 3;
  // lower blocks only; waves w and w+4 share a SIMD, so they take column blocks w and 7-w
  // (8-w and w+1 row blocks: 9 per SIMD)
  const int wc = (w < 4) ? w : 11 - w;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) cnt[cb] = v4i{0, 0, 0, 0};
  if (a.skip & 1) {
    __syncthreads();
  } else if (a.ft.gsh) {
    // kernel-form folds: the lower blocks' counts from the individual's shared A_R A_R^T
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
      if (cb >= wc)
#pragma unroll
        for (int r = 0; r < 4; ++r) cnt[cb][r] = gsh_count(a, b, j0 + 16 * cb + (l >> 4) + 4 * r, j0 + 16 * wc + (l & 15));
  } else {
    // 2-bit packed rows: the SNP form's split rows, the kernel form's gathered panel
    const uint8_t* rp = a.form == FORM_PRIMAL ? row_packed(a, b, j0 + row) : row_dpk(a, b, j0 + row);
    const uint8_t* sa = rp + pk_swz_a(row, pos);
    const uint8_t* sb = rp + pk_swz_b(row, pos);
    switch (wc) {   // wave-uniform: one instantiation per column block
      case 0: i8_tt8_pk64<4, 0>(sa, sb, nblk, lds, cnt); break;
      case 1: i8_tt8_pk64<4, 1>(sa, sb, nblk, lds, cnt); break;
      case 2: i8_tt8_pk64<4, 2>(sa, sb, nblk, lds, cnt); break;
      case 3: i8_tt8_pk64<4, 3>(sa, sb, nblk, lds, cnt); break;
      case 4: i8_tt8_pk64<4, 4>(sa, sb, nblk, lds, cnt); break;
      case 5: i8_tt8_pk64<4, 5>(sa, sb, nblk, lds, cnt); break;
      case 6: i8_tt8_pk64<4, 6>(sa, sb, nblk, lds, cnt); break;
      default: i8_tt8_pk64<4, 7>(sa, sb, nblk, lds, cnt); break;
    }
  }
  __syncthreads();
  const int il = 16 * wc + (l & 15);
  const int64_t gj = j0 + il;
  const double uj = u_sh[il];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) {
    if (cb >= wc) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cl = 16 * cb + (l >> 4) + 4 * r;
        const int64_t gi = j0 + cl;
        const double kv = grm_value(cnt[cb][r], u_sh[cl], uj, sa, cN, invd, sm);
        const double v = (sys_real(gi, pad, nrow) && sys_real(gj, pad, nrow)) ? kv + ((gi == gj) ? lam : 0.0)
                                                                              : ((gi == gj) ? 1.0 : 0.0);
        Kd[pk(cb, wc) + bo(cl & 15, il & 15)] = v;
      }
    }
  }
}

// Off-diagonal launch of column J (see OffPlan).  The grid holds the unit classes longest first
// -- every P-unit, then every D-unit, then every T-unit (a class's units dispatched after
// another class's have started cannot hide behind them: with the D-units after the T-units of
// their own individual, as one list per individual, the launches ran 9% longer) -- each class
// XCD-remapped so that one XCD's L2 serves an individual's Lt block rows; and, column 0 of the
// kernel form only, the K_JJ workgroups for J >= 2 at the end.
// NTRK: the traits the T-units' w update runs over (1, or MAXT for several traits) -- one kernel per
// case, so the single-trait kernel's registers are allocated for its own path
template <int NTRK>
__global__ __launch_bounds__(OTH, 4) void k_chol_offdiag(CholArgs a, OffPlan p) {
  __shared__ __attribute__((aligned(16))) double lds[NPACK * BLKD];   // 72 KiB: rings, then packed X
  __shared__ __attribute__((aligned(16))) double uj_sh[2 * TILE];   // k_stage's column pairs (P_j, Q_j)
  __shared__ double ui_sh[TILE], zj_sh[MAXT][TILE];
  const int64_t npu = (int64_t)p.nP * p.nrs;
  const int64_t n_p = a.B * npu, n_d = a.B * p.nds, n_t = a.B * p.nI;
  int64_t bid = blockIdx.x;
  WgTrace tr(a.wgt);
  if (bid < n_p) {
    const int64_t lg = xcd_remap(bid, n_p);
    const int64_t b = lg / npu;
    const int u = (int)(lg % npu);
    const int I = a.J + 2 + u / p.nrs, rs = u % p.nrs;
    switch (p.nrs) {
      case 1: part_unit<8>(a, b, I, rs, lds, uj_sh, ui_sh); break;
      case 2: part_unit<4>(a, b, I, rs, lds, uj_sh, ui_sh); break;
      default: part_unit<2>(a, b, I, rs, lds, uj_sh, ui_sh); break;
    }
    tr.done(WGT_PART, a.J, I, b);
    return;
  }
  bid -= n_p;
  if (bid < n_d) {
    const int64_t lg = xcd_remap(bid, n_d);
    const int64_t b = lg / p.nds;
    const int u = (int)(lg % p.nds);
    syrk_partial8(a, b, a.J + 1, a.J, lds, p.nds == 1 ? 0 : 1 + u);
    tr.done(WGT_PREP, a.J, a.J + 1, b);
    return;
  }
  bid -= n_d;
  if (bid < n_t) {
    int64_t b;
    int I;
    if (a.q != nullptr) {   // last-term mode: the B tiles (J+1, J) first, then the rest
      if (bid < a.B) {
        b = xcd_remap(bid, a.B);
        I = a.J + 1;
      } else {
        const int64_t lg = xcd_remap(bid - a.B, n_t - a.B);
        b = lg / (p.nI - 1);
        I = a.J + 2 + (int)(lg % (p.nI - 1));
      }
    } else if (p.ne > 0 && p.ne < n_t) {
      // some tiles started by E-units: the others first, those last (with the dispatcher's
      // round-robin a CU then pairs a whole tile with a shortened one or with a lighter class),
      // each class in the E-units' own order (tile e, I-major: its E-unit's XCD)
      const int64_t nne = n_t - p.ne;
      const int64_t e = bid < nne ? p.ne + xcd_remap(bid, nne) : xcd_remap(bid - nne, p.ne);
      b = e % a.B;
      I = a.J + 1 + (int)(e / a.B);
    } else {
      const int64_t lg = xcd_remap(bid, n_t);
      b = lg / p.nI;
      I = a.J + 1 + (int)(lg % p.nI);
    }
    // an E-unit of the diagonal launch summed the term L = Ls0 of the first ne tiles (I-major)
    const int ed = (int64_t)(I - a.J - 1) * a.B + b < p.ne ? 1 : 0;
    tile_unit<NTRK>(a, b, I, p.ahead_cur, ed, lds, uj_sh, ui_sh, zj_sh, tr);
    tr.done(WGT_TILE, a.J, I, b);
    return;
  }
  // column 0, kernel form: K_JJ for J >= 2
  const int64_t lg = xcd_remap(bid - n_t, p.n_kd);
  const int nJ = a.NT - 2;
  diag_grm_tile(a, lg / nJ, 2 + (int)(lg % nJ), reinterpret_cast<uint8_t*>(lds), uj_sh);
  tr.done(WGT_KJJ, a.J, 2 + (int)(lg % nJ), lg / nJ);
}

int cu_count() {
  static int n = 0;
  if (n <= 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
  }
  return n;
}

__global__ __launch_bounds__(OTH, 2) void k_diag_grm8(CholArgs a, int nJ) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[4 * 2 * TILE * 64];
  __shared__ double u_sh[TILE];
  const int64_t lg = xcd_remap(blockIdx.x, gridDim.x);   // an individual's tiles on one XCD
  diag_grm_tile(a, lg / nJ, (int)(lg % nJ), lds, u_sh);
}

hipError_t launch_diag_grm(const CholLaunch& c, hipStream_t s) {
  CholArgs a = make_args(c, 0);
  a.wgt = nullptr;
  const int nJ = std::min(c.sd.NT, 2);
  hipLaunchKernelGGL(k_diag_grm8, dim3((unsigned)(c.B * nJ)), dim3(OTH), 0, s, a, nJ);
  return hipGetLastError();
}

// Kernel-form folds sharing one animal set: A_R A_R^T of individual b over fold 0's split rows (its
// panel, system b), every 128 x 128 tile pair I >= J of the n_Rp rows on int8 MFMA from the packed
// rows (i8_tt8_pk64), stored both ways into a full n_Rp x n_Rp int32 matrix (FoldTab::gsh)
__global__ __launch_bounds__(OTH, 2) void k_gshare(CholArgs a, int NR) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[4 * 2 * TILE * 64];
  const int64_t ntp = (int64_t)NR * (NR + 1) / 2;
  const int64_t lg = xcd_remap(blockIdx.x, gridDim.x);   // an individual's tiles on one XCD
  const int64_t b = lg / ntp;
  int I, J;
  tri_decode((int)(lg % ntp), I, J);
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)J * TILE;
  const int row = 16 * w + (l >> 2), pos = l & 3;
  const int64_t nblk = (int64_t)a.scal[b * SCAL + SC_CBLK];
  v4i cnt[8];
  i8_tt8_pk64<4>(row_dpk(a, b, j0 + row) + pk_swz_a(row, pos), row_dpk(a, b, i0 + row) + pk_swz_b(row, pos), nblk, lds,
                 cnt);
  const int64_t ld = a.ft.gsh_ld;
  int32_t* G = a.ft.gsh + b * ld * ld;
  const int64_t ic = i0 + 16 * w + (l & 15);
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t jr = j0 + 16 * cb + (l >> 4) + 4 * r;
      G[jr * ld + ic] = cnt[cb][r];
      G[ic * ld + jr] = cnt[cb][r];
    }
}

hipError_t launch_gshare(const CholLaunch& c, hipStream_t s) {
  const FoldTab& ft = c.ft;
  if (!ft.gsh || c.sd.form != FORM_DUAL || c.d.nRp % TILE) return hipErrorInvalidValue;
  CholArgs a = make_args(c, 0);
  a.wgt = nullptr;
  const int NR = (int)(c.d.nRp / TILE);
  hipLaunchKernelGGL(k_gshare, dim3((unsigned)(ft.bpf * NR * (NR + 1) / 2)), dim3(OTH), 0, s, a, NR);
  return hipGetLastError();
}

hipError_t launch_chol_diag(const CholLaunch& c, int J, const OffPlan& p, hipStream_t s) {
  CholArgs a = make_args(c, J);
  const int64_t nwg = c.B * (1 + p.ndd) + p.ne;
  // E-units need the partial-sum slots and a tile below the diagonal, and are built without the
  // shared fold counts (k_acc<8, false>)
  if (p.ne > 0 && (c.part == nullptr || J < 1 || p.ne > c.B * p.nI || c.ft.gsh)) return hipErrorInvalidValue;
  // profiling: the phase stamps of this launch follow its workgroup records
  if (c.wgt) a.dtr = c.wgt + nwg * WGT_REC;
  if (diag_waves(p, c.diag_waves) == DWX && !(a.skip & FLAG_WRITE_LJJ))
    hipLaunchKernelGGL(k_chol_diag_w<DWX>, dim3((unsigned)nwg), dim3(64 * DWX), 0, s, a);
  else
    hipLaunchKernelGGL(k_chol_diag, dim3((unsigned)nwg), dim3(DTHR), 0, s, a, p.ne, p.ahead_cur ? J - 1 : 0);
  return hipGetLastError();
}

hipError_t launch_chol_offdiag(const CholLaunch& c, int J, const OffPlan& p, hipStream_t s) {
  if (p.nI <= 0) return hipSuccess;
  CholArgs a = make_args(c, J);
  if (c.d.nt == 1)
    hipLaunchKernelGGL(k_chol_offdiag<1>, dim3((unsigned)offdiag_grid(p, c.B)), dim3(OTH), 0, s, a, p);
  else
    hipLaunchKernelGGL(k_chol_offdiag<MAXT>, dim3((unsigned)offdiag_grid(p, c.B)), dim3(OTH), 0, s, a, p);
  return hipGetLastError();
}

}  // namespace tblup
