// Internal declarations shared by the HIP translation units of libtblup_gpu.so.
//
// Data layout in HBM (per context = one GPU):
//   geno_sm   int8  [P][n]        SNP-major genotypes, built once (transpose of the .npy)
//   colsum_all int32 [P]          per-SNP allele count over all n animals (gblup p)
//   per split s (train T, valid V; nTp/nVp = sizes rounded up to 128):
//     gpk       uint8 [P+1][nRp/4] SNP-major rows permuted to [T | 0-pad | V | 0-pad], nRp = nTp+nVp,
//                                 2-bit packed (animal 4j+i at bits 2i of byte j); row P is all zero
//                                 (padding rows of the primal form)
//     colsum_T  int32 [P]         allele counts over T (snp p)
//     xty       f64  [nt][P]      sum_t (x_tp - c_p)(y_t - mean y_T): the primal right-hand side, per SNP and trait
//     yT        f64 [nTp]         phenotypes of T (0 in padding), yV f64 [nV]
//   per evaluation chunk of B individuals (workspace):
//   Two equivalent forms of the per-individual system (chosen per chunk, see SysDims):
//     kernel (dual) form   rows = train animals (ns = nTp), contraction over the k SNPs
//     SNP (primal) form    rows = the k selected SNPs (ns = round_up(k)), contraction over
//                          the train animals -- sklearn Ridge's own choice when k <= n_T
//     panel  uint8 [b][nRp][dual_pk_row]  kernel form only: each system's animal rows 2-bit packed
//                                      over its k SNPs (the primal form reads gpk rows in place)
//     u      f64  [B][prow]            centring sums (dual: u_i = sum_s m_s a_is; primal: s_a)
//     scal   f64  [B][16]              see SC_* below
//     L      f64  [B][NT][NT][128^2]   Lt tiles (tile (I,J) holds L_IJ^T)
//     Dinv   f64  [B][NT][36][16x16]   X = L_JJ^{-1} of each diagonal tile, packed lower blocks
//     z      f64  [B][ns]              L^{-1} rhs
//     fit    f64  [B]
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace tblup {

constexpr int TILE = 128;      // output tile edge of the GRM and Cholesky kernels
constexpr int TBLUP_NSLOT = 2; // diagonal-tile preparation buffers per individual (slot J&1)
constexpr int KBLK = 64;       // SNPs per panel block (int8 MFMA K step)
constexpr int MAXT = 4;        // traits per context (multi-trait: one Cholesky, MAXT right-hand sides)
constexpr int GATHER_ROWS = 128;

// per-individual scalars scal[b][SCAL]
constexpr int SCAL = 16;
enum {
  SC_SA = 0,    // additive centring coefficient (dual 1/N, primal 0)
  SC_CN = 1,    // constant centring term (dual q/N^2, primal 0)
  SC_INVD = 2,  // 1/d
  SC_MUF = 3,   // intercept flag: 1 = snp branch (intercept mean(y_T) of each trait), 0 = gblup
  SC_LAM = 4,   // lambda = (1-h2)/h2
  SC_D = 5,     // d = 2 sum p(1-p)
  SC_MODE = 6,  // branch: 1 gblup, 2 snp
  SC_K = 7,     // selected SNPs
  SC_SM = 8,    // multiplicative centring coefficient (dual 0, primal 1/n_T)
  SC_NROW = 9,  // real system rows (dual n_T, primal k); the rest is identity padding
  SC_CBLK = 10, // contraction blocks of 64 for the system matrix
  SC_BAD = 11,  // 1 when an index lies outside [-P, P) (numpy would raise IndexError): fitness NaN
  SC_PAD = 12,  // leading padding rows (SNP form: ns - k, see SysDims::pad_first; kernel form 0)
};
// System row r is real (not identity padding) when pad <= r < pad + nrow.  SNP form: real row r
// holds selected SNP r - pad.  The padding leads so that its exact-zero rows and columns fall at
// the START of block column 0, where the Cholesky's contractions over L = 0 skip them
// (gemm1_a32 / syrk_lower8_32 start at row pad); trailing padding would sit in the output rows of
// the last tile row instead, split unevenly over the waves.
__host__ __device__ __forceinline__ bool sys_real(int64_t r, int64_t pad, int64_t nrow) {
  return (uint64_t)(r - pad) < (uint64_t)nrow;
}
enum { FORM_DUAL = 0, FORM_PRIMAL = 1 };

// Panel column of a selected-SNP index with numpy's fancy-index rule (the reference's
// data[:, indices], evaluator.py:275/298): -P <= p < 0 addresses column p + P.  Indices
// outside [-P, P) are rejected on the host (tblup_eval_batch) or flagged by k_indiv_stats
// (device entry); the clamp below only keeps such a flagged individual's loads in bounds.
__host__ __device__ __forceinline__ int64_t snp_col(int64_t p, int64_t P) {
  p = p < 0 ? p + P : p;
  return p < 0 ? 0 : (p >= P ? P - 1 : p);
}
// CholLaunch::skip: also store L_JJ (debug readback only).  Bits 0-18 of the mask are the ablation
// bits of TBLUP_DBG_SKIP (bits 16-18: k_sys_tiles stores nothing); this flag must stay clear of them.
constexpr int FLAG_WRITE_LJJ = 1 << 24;

// System dimensions of one chunk.
struct SysDims {
  int form;          // FORM_DUAL / FORM_PRIMAL
  int64_t ns;        // padded system size (multiple of TILE)
  int NT;            // ns / TILE
  int64_t prow;      // panel rows per contraction block
  int64_t cblk;      // contraction blocks per individual in the panel (max over the chunk)
  int pad_first = 0; // SNP form: padding rows lead (SC_PAD = ns - k; TBLUP_PAD_FIRST, default on)
};
// Kernel form: the gathered panel holds each system's prow (= n_Rp) animal rows 2-bit packed over its
// selected SNPs -- byte j of a row holds SNPs 4j..4j+3 at bits 2i, the SNP-form split rows' code --
// in whole 64-B (256-SNP) stages: bytes per row
inline int64_t dual_pk_row(const SysDims& sd) { return (sd.cblk + 3) / 4 * 64; }

typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct EvalDims {
  int64_t n;        // animals in the panel
  int64_t P;        // SNPs in the panel
  int64_t nT, nV;   // split sizes
  int64_t nTp, nVp; // padded to TILE
  int64_t nRp;      // nTp + nVp
  int NT;           // nTp / TILE
  int NR;           // nRp / TILE
  int nt;           // traits
};

// LDS-DMA of 16 B per lane (lane i -> lds + 16 i) as inline asm, for the stage rings.  The compiler
// sees __builtin_amdgcn_global_load_lds as an LDS write in flight and waits vmcnt(0) before the
// next LDS read of ANY address (ROCm 7.2, checked in the emitted code): in a ring that issues
// stage s + 1 and then reads stage s, that wait drained the prefetch, so every stage's load
// latency was exposed.  Hidden from the compiler, the DMA is ordered by the ring's own counted
// s_waitcnt + barrier, which every reader of a stage sits behind (the compiler's own counted waits
// on its loads stay correct: an extra outstanding DMA only makes them wait for more).  m0 is saved
// and restored around the DMA (its LDS address is sampled at issue), so the asm leaves m0 as the
// compiler last set it: builtin LDS-DMAs beside these rings keep whatever m0 setup the compiler
// hoisted or merged for them, by construction.  (m0 is a reserved register, so it cannot be
// declared clobbered: clang warns that the clobber is not honoured.)
__device__ __forceinline__ void glds16_asm(const void* g, const void* lds) {
  const uint32_t la = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds);
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(la)
      : "memory");
}

// ---- packed lower-triangular 16x16 block storage of a 128x128 tile (LDS and Dinv) ----
constexpr int NB = 16;                       // base block edge
constexpr int NBLK = TILE / NB;              // 8 block rows
constexpr int NPACK = NBLK * (NBLK + 1) / 2; // 36 lower blocks
constexpr int BLKD = NB * NB;                // doubles per block

__host__ __device__ __forceinline__ int pk(int q, int s) { return (q * (q + 1) / 2 + s) * BLKD; }
// element (r, c) of a 16x16 block; 16-B chunk swizzle makes the fragment reads conflict-free
__host__ __device__ __forceinline__ int bo(int r, int c) { return r * NB + 2 * ((c >> 1) ^ ((r >> 1) & 7)) + (c & 1); }

// Per-split device data of the systems of one launch sequence.  One split: nf = 1.  Fold-fused
// evaluation (tblup_eval_folds*: IntraGCV's k folds as one batch of F x B systems, system
// s = f * bpf + b against split f; every split of equal dimensions): one entry per fold.
constexpr int MAXF = 16;
struct FoldTab {
  int64_t bpf;                 // systems per fold (the chunk's B when nf = 1)
  int nf;
  int share;                   // every fold's train + valid rows are one multiset (k_sys_tiles_folds)
  const uint8_t* gpk[MAXF];    // 2-bit packed split rows [P+1][nRp/4]
  const int32_t* csT[MAXF];    // train allele counts [P]
  const double* xty[MAXF];     // [nt][P]
  const double* yV[MAXF];      // [nt][nV]
  const double* yT[MAXF];      // [nt][nTp] (kernel form: the right-hand sides y_T - mu on the fly)
  const double* ymu[MAXF];     // [nt]
  // kernel form with shared counts (IntraGCV, share): every system's int8 count A_r . A_c is read
  // from its individual's A_R A_R^T over fold 0's split rows (k_gshare), system row r of fold f at
  // row gmap[f][r] (-1: padding) -- one int8 GEMM per individual instead of one per fold
  int32_t* gsh;                // [bpf][gsh_ld][gsh_ld] (null: counts per system, int8 MFMA in the units)
  const int32_t* gmap;         // [nf][gmap_ld]
  int64_t gsh_ld, gmap_ld;     // nRp, nTp
};
__host__ __device__ __forceinline__ int fold_of(const FoldTab& ft, int64_t s) { return (int)(s / ft.bpf); }

// ---- launchers (k_prep.hip) ----
hipError_t launch_transpose_geno(const int8_t* src, int8_t* dst, int64_t n, int64_t P, hipStream_t s);
hipError_t launch_colsum_all(const int8_t* geno_sm, int32_t* colsum, int64_t n, int64_t P, hipStream_t s);
// yres[t] = sum over T of the doubles y_t - ymu[t] (each rounded as the kernel rounds it; only their sum is taken
// in long double)
struct YResidual { double v[MAXT]; };
hipError_t launch_build_split(const int8_t* geno_sm, int64_t n, int64_t P, const int32_t* rowmap,
                              int64_t nRp, int64_t nT, const double* yT, const double* ymu, YResidual yres, int nt,
                              uint8_t* geno_packed, int32_t* colsum_T, double* xty,
                              hipStream_t s);
// fused offsets of F copies of a B-individual index list (sum_k indices each): out[F * B + 1]
hipError_t launch_fold_offsets(const int64_t* off, int64_t B, int64_t F, int64_t sum_k, int64_t* out, hipStream_t s);
// primal form (sd.form): also u[b][a] = s_a and rhs[b][t][a] = xty[t][p_a] / d over the ns rows
// (colsum_T / xty of system b: ft's fold of b); h2v != null: [B] on the device, system b's own h2
hipError_t launch_indiv_stats(const int64_t* idx, const int64_t* off, int64_t B, const FoldTab& ft,
                              const int32_t* colsum_all, const EvalDims& d, const SysDims& sd,
                              int branch, double h2, const double* h2v, double* scal, double* u, double* rhs,
                              int32_t* err, hipStream_t s);
// kernel form: each system's 2-bit packed animal rows (dual_pk_row bytes each) from its split's rows
// (ft: fold of system b)
hipError_t launch_gather(const FoldTab& ft, const int64_t* idx, const int64_t* off, int64_t panel_stride, int64_t B,
                         const int32_t* colsum_all, const double* scal, const EvalDims& d, int64_t pk_row,
                         uint8_t* panel, double* u, hipStream_t s);

// ---- launchers (k_grm.hip) ----
hipError_t launch_grm(const uint8_t* panel, int64_t panel_stride, int64_t pk_row, const int64_t* off, const double* u,
                      const double* scal, const EvalDims& d, int64_t B, double* K, hipStream_t s);

// ---- launchers (k_chol.hip, k_systiles.hip, k_solve.hip) ----
// SNP form with k_sys_tiles_st (which reads no scalar): k_indiv_stats' inputs and outputs, when the
// scalars are formed in the launch after the system tiles (k_stats_diag_counts, fused with the
// K_JJ + lambda I epilogue of the tiles J < 2) instead of in a launch of their own before them
struct StatsFuse {
  const int32_t* csA;    // allele counts over all n animals (gblup p)
  int64_t n, nT;
  int branch;
  double h2;
  const double* h2v;     // [B] per-system h2 on the device, null: h2
  int32_t* err;          // the context's index-error status word
  double* scal;          // [B][SCAL]
  double* u;             // [B][ns]
  double* rhs;           // [B][nt][ns]
};
// 4 KiB between individuals' Lt tiles, so the same tile of different individuals does not start on the
// same HBM channel offset: off-diagonal -5 us at pop 128, solve -1% (A/B, profiles/r06_lpad_ab.txt;
// 64 KiB was slower, 260 KiB even)
constexpr int64_t L_PAD = 512;   // doubles of padding between individuals' L
// doubles from one individual's Lt tiles to the next's
__host__ __device__ inline int64_t l_stride(int NT) { return (int64_t)NT * NT * TILE * TILE + L_PAD; }
struct CholLaunch {
  EvalDims d;
  SysDims sd;
  int64_t B;
  double* L;             // Lt tiles [B][NT][NT][128*128] (tile (I,J) holds L_IJ^T)
  double* Dinv;          // [B][NT][NPACK*BLKD] X = L_JJ^{-1}, packed lower 16x16 blocks
  double* z;             // [B][nt][ns]
  double* w;             // [B][nt][ns] forward-substitution partial sums
  const double* rhs;     // [B][nt][ns] primal right-hand sides (dual: y_T - mu on the fly)
  double* S;             // [B][2][36*256] diagonal-tile preparation, slot J&1
  double* Kd;            // [B][NT][36*256] GRM diagonal tiles K_JJ + lambda I (kernel form / no system tiles)
  const double* yT;      // split phenotypes [nt][nTp] (kernel form: one split)
  const uint8_t* panel;  // kernel form: the gathered 2-bit packed animal rows (dual_pk_row bytes each)
  int64_t pstride;       // panel bytes per individual
  const int64_t* off;    // [B+1] device offsets
  const int64_t* idx;    // device SNP indices of the chunk
  int64_t gs_row;        // bytes per int8 split row (nRp): split SNP-major matrix, row P zero
  int64_t gpk_row;       // bytes per 2-bit packed split row (nRp / 4)
  FoldTab ft;            // split rows, counts, right-hand sides and phenotypes of each system's split
  const double* u;       // [B][prow]
  const double* scal;    // [B][SCAL]
  int skip;              // diagnostic ablation mask (env TBLUP_DBG_SKIP), 0 in production
  uint64_t* wgt;         // per-workgroup timestamp records of this launch (env TBLUP_WG_TRACE), else null
  int16_t* kc;           // exact off-diagonal system-tile counts from k_sys_tiles (either form), else null
  double* part;          // [2][B][NT][128*128] partial sums of the next column's tiles (ahead schedule)
  double* q;             // last-term mode: [B][36*256] diagonal tile J's last SYRK term, from launch J-1
  int padskip;           // contractions over block column 0 skip the leading padding rows (SC_PAD)
  int16_t* kd;           // with k_sys_tiles: the diagonal tiles' exact counts instead of Kd,
                         // [B][NT][36 packed lower blocks][64 lanes][4] (KD_TILE int16 per tile); the
                         // consumers form K_JJ + lambda I from them (kd_block, k_chol.hip)
  int sys_st = -1;       // k_sys_tiles_st: -1 auto, 0 never, 1 whenever it applies (TBLUP_SYS_ST)
  int diag_waves = 0;    // diagonal workgroup waves where the launch has no D- / E-units: 0 auto (TBLUP_DIAG_WAVES)
  const StatsFuse* stats = nullptr;   // launch_sys_tiles: form the scalars after k_sys_tiles_st
};
// k_sys_tiles output: per individual NT(NT-1)/2 off-diagonal tiles (I > J, t = I(I-1)/2 + J) of
// 128 x 128 int16 counts, in the order the off-diagonal kernel's lanes read them:
// [column block ib][row block cb][lane][4].  Exact while n_T <= 8191 (counts <= 4 n_T).
// (Tile offsets, both sides: kc_tile / kd_tile, chol_dev.h.)
constexpr int64_t KC_TILE = (int64_t)TILE * TILE;
constexpr int64_t KD_TILE = (int64_t)NPACK * BLKD;   // diagonal tile counts: the 36 lower 16x16 blocks
constexpr int64_t KC_MAX_NT = 8191;
// workgroup trace record (profiling only): {start, end, kind << 56 | I << 40 | b, J},
// s_memrealtime ticks (100 MHz); kinds below
constexpr int WGT_REC = 4;
// a diagonal launch's records are followed by DTR_RECS records holding the phase stamps of
// its workgroup 0 (up to 16 waves x 64 uint64), written as kind-0 records
constexpr int DTR_RECS = 16 * 64 / WGT_REC;
enum { WGT_DIAG = 1, WGT_TILE = 2, WGT_PREP = 3, WGT_KJJ = 4, WGT_SYS = 5, WGT_PART = 6, WGT_DPREP = 9, WGT_EPART = 10 };   // 7 / 8: the chained solve (k_solve.hip)
// Work units of the off-diagonal launch of column J, per individual (k_chol.hip):
//   nI  T-units: tiles (I, J), I > J
//   nP  x nrs P-units (ahead schedule): partial sums K - sum_{L<J} of tiles (I, J+1), I >= J+2, in
//       nrs row slices -- launch J+1's T-units then start from them (ahead_cur) and sum one L
//   nds D-units: the diagonal tile J+1's partial sum over L < J (1 or 2 block slices)
//   n_kd K_JJ workgroups (column 0 of the kernel form only)
//   ndd: the D-units run in the DIAGONAL launch J instead (whole, one per individual; nds = 0), on
//   the CUs its B workgroups leave idle -- they need only the columns L < J, complete before it
//   ne  E-units, also in the DIAGONAL launch J (after its D-units), one per CU still idle: the GEMM1
//       term L = Ls0 (Ls0 = J-1 after an ahead launch, else 0) of column J's tiles e < ne in
//       I-major order (tile (J+1 + e / B, J) of individual e % B), into the partial-sum slot J&1;
//       such a tile's T-unit starts from that partial and sums from Ls0 + 1 (its MFMA chains
//       unchanged: bit-identical)
struct OffPlan {
  int nI, nP, nrs, nds, ahead_cur;
  int ndd;
  int64_t n_kd;
  int64_t ne;
  __host__ __device__ int64_t units() const { return (int64_t)nP * nrs + nds + nI; }
};
// Schedule policy (host, per chunk: a function of B and the system shape only, so the results
// are bit-identical for any policy -- every accumulator keeps its MFMA chain):
//   ahead: -1 auto (launch j ahead when B * (NT - 2 - j) < AHEAD_SLOTS; measured at config 2 against
//   the classic schedule: +14% at B = 32, +2.3% at B = 128, even at 256; a whole-chunk B < 64 rule
//   and thresholds 512 / 1024 were slower at 128), 0 never, 1 always; nrs: 0 auto (fill >= 2 units per CU
//   slot pair), else fixed 1 / 2 / 4; without k_sys_tiles counts (int8 K in-tile) nrs = 1
constexpr int64_t AHEAD_SLOTS = 256;
// diag_d: D-units in the diagonal launch, -1 auto (DD_MIN_B < B <= DD_MAX_B and J <= DD_MAX_J), 0 never,
// 1 always.  Measured (config 2, A/B): pop 128 +2.4% (off-diagonal -49 us, diagonal +11 us per step);
// pop 64 -0.8%, pop 32 -1.5% (their off-diagonal launches are bound by other units, and the diagonal
// launches still grow); every J (TBLUP_DIAG_D=1): diagonal +100 us at pop 128
constexpr int64_t DD_MIN_B = 64;
constexpr int64_t DD_MAX_B = 128;
constexpr int DD_MAX_J = 3;
// diag_e: E-units in the diagonal launch, -1 auto (one per CU the launch's other workgroups leave
// idle, ncu - B (1 + ndd), up to the column's tiles; so none at B >= ncu), 0 never, 1 every tile of
// the column (tests), 2 only columns covered whole
OffPlan off_plan(int64_t B, int NT, int J, bool sys_tiles, int ahead, int nrs, int64_t slots = AHEAD_SLOTS,
                 int diag_d = 0, int dd_maxj = DD_MAX_J, int diag_e = 0, int64_t ncu = 0);
// Waves of launch J's diagonal workgroups.  A launch with D- or E-units keeps the 8-wave kernel (its
// units are 8-wave code); the others run the wide workgroup, DIAG_WAVES_WIDE waves, whose extra
// waves shorten the factorisation windows (k_chol.hip diag_tile).  knob: 0 auto, else 8 or the wide
// count forces the choice for the launches without units (a count that is not built: auto).
constexpr int DIAG_WAVES_WIDE = 16;
inline int diag_waves(const OffPlan& p, int knob) {
  if (p.ndd > 0 || p.ne > 0) return 8;
  return knob == 8 ? 8 : DIAG_WAVES_WIDE;
}
// multiprocessor count of the current device (256 when the query fails)
int cu_count();
inline int64_t offdiag_grid(const OffPlan& p, int64_t B) { return p.nI > 0 ? B * p.units() + p.n_kd : 0; }
// Fused GRM + tile Cholesky, column by column (k_chol.hip): diagonal tile J (k_chol_diag),
// then the off-diagonal tiles (I > J, J) plus the preparation of diagonal tile J+1.
hipError_t launch_chol_diag(const CholLaunch& c, int J, const OffPlan& p, hipStream_t s);
hipError_t launch_chol_offdiag(const CholLaunch& c, int J, const OffPlan& p, hipStream_t s);
// all diagonal GRM tiles K_JJ of the batch (one launch, before the column loop)
hipError_t launch_diag_grm(const CholLaunch& c, hipStream_t s);
// kernel form, shared fold counts: A_R A_R^T of every individual (FoldTab::gsh) from fold 0's panels
hipError_t launch_gshare(const CholLaunch& c, hipStream_t s);
// k_systiles.hip, either form: every (I >= J) system tile of the batch on FP4 MFMA in one launch -- off-diagonal
// counts into c.kc, diagonal tiles' counts into c.kd (replaces launch_diag_grm and the int8 phase
// of the off-diagonal tiles)
hipError_t launch_sys_tiles(const CholLaunch& c, hipStream_t s);
// its grid: > 0 the persistent super-tile kernel's workgroups (k_sys_tiles_st), else minus the
// per-tile kernel's
int64_t sys_tiles_grid(const CholLaunch& c);
constexpr int SP_ROWTAB = 4096;   // k_sys_tiles_st: rows of its LDS row table (ns <= SP_ROWTAB)
// the same for a fold-fused chunk whose folds share their train + valid rows (FoldTab::share):
// C_{R_f} = C_{T_all} - C_{V_f}, one workgroup per (individual, tile) for all F folds
hipError_t launch_sys_tiles_folds(const CholLaunch& c, hipStream_t s);
// Back substitution, prediction and fitness.  ch == null: one workgroup per individual
// (k_solve); else (SNP form) the chained solve (k_solve_chain): an individual's block rows and
// tile products spread over the chip, handing beta_J and the partial products on through
// per-call flags (SolveChain).
struct SolveChain {
  int32_t* flags;   // [B][chain_flags(NT)], compared with seq (never reset)
  double* beta;     // [B][nt][ns]: beta_J, published by the pull units (flags [0, NT) of an individual)
  double* cpart;    // [B][NT (row I)][NT (tile J)][nt][128]: L_JI^T beta_J
  double* epart;    // [B][NT][nt][nV]: block J's share of X_V beta
  double* mbpart;   // [B][NT][nt]: block J's share of sum_a s_a beta_a
  int32_t* err;     // this call's slot of the expiry ring (CHAIN_ERR_RING words, slot seq % CHAIN_ERR_RING):
                    // = seq once a wait of the call gave up -- the call's later waits give up at once,
                    // and the host entries read it to re-run that chunk's solve through k_solve
  int32_t* expired; // device entries: the context's sticky solve-status word (set to 1 by a unit whose
                    // wait gave up; tblup_solve_error / tblup_status_async); host entries: a scratch
                    // word (they recover from their own ring slot instead)
  int32_t seq;      // this call's flag value
  int32_t mode;     // TBLUP_CHAIN_SYNC (k_solve.hip)
  int32_t spin_max; // polls before a wait gives up (CHAIN_SPIN_MAX; lowered only by the debug knob)
  int32_t pull;     // 1: pull units (block column J: beta_K, K > J, and the tiles (K, J)); 0: push units
  int32_t delay;    // debug knob only: U(0, NT-1) sleeps this many s_sleep(127) rounds before
                    // publishing, so its consumers' waits expire (0 in production)
};
// Bound on a hand-off wait: 2^20 polls (an sc1 load round trip each plus s_sleep 2: ~0.5-1 s).
// Progress does not need the bound (see k_solve.hip); it turns a broken dispatch assumption into
// an error the host reports instead of a hang.
constexpr int32_t CHAIN_SPIN_MAX = 1 << 20;
// expiry records, one slot per call sequence number modulo the ring size (after the flags)
constexpr int CHAIN_ERR_RING = 64;
// the context's device status words (tblup_index_error / tblup_solve_error / tblup_status_async)
enum { ST_INDEX = 0, ST_SOLVE = 1, ST_WORDS = 2 };
__host__ __device__ inline int64_t chain_flags(int NT) { return (int64_t)NT * (NT + 2); }
hipError_t launch_solve(const CholLaunch& c, const SolveChain* ch, double* fitness, double* ebv, hipStream_t s);
// The fitted model of every individual of a chunk (k_effects, k_solve.hip), from the factor, the
// diagonal inverses and z that the chunk's pipeline left in the workspace (what launch_solve reads):
// center[off[b] + j] = 2 p_j of selected SNP j (the exact allele count over the branch's reference
// rows -- csA over all n animals for gblup, the split's counts for snp -- divided once by their
// number) and effects[t * plane + off[b] + j], trait-major planes.  SNP form: the solved beta without
// its padding rows; kernel form: W_T^T alpha / d over the split's 2-bit packed rows.
// alpha (may be null): also the solution itself, [B][nt][ns] in z's layout (SNP form: beta at rows pad .. pad + k - 1;
// kernel form: alpha_t = (V^-1 (y_T - mu))_t at the train rows); with center null only alpha is written.
hipError_t launch_effects(const CholLaunch& c, const int32_t* csA, double* center, double* effects, int64_t plane,
                          hipStream_t s, double* alpha = nullptr);

// ---- the slab kernels behind a chunk's factor: k_reliab, k_snpscore, k_covar (fwd_subst.h) ----
// Each walks a list (animals, SNPs, covariates) in slabs of 16 right-hand sides, one workgroup per (model,
// slab).  How one call does so, decided in one place: lds -- a slab's ns x 16 right-hand sides live in LDS
// (the entry's knob allows it and they fit RELIAB_LDS_V), else in a workspace slice of the workgroup's own;
// S -- slabs of the list per launch: all of them, or without LDS what `aim` bytes hold of the B x S slices
// of one launch, never less than one slab per model and never a grid beyond 2^31 - 1; scratch() -- the
// doubles of those slices (vscr; 0 with LDS).  The same bits either way.
// tblup_reliability_batch plans with TBLUP_RELIAB_LDS, tblup_snp_score_batch with TBLUP_SCORE_LDS;
// tblup_fit_cov_batch's covariates are one slab per model (n_items = COVAR_W) and its plan keeps reading
// TBLUP_SCORE_LDS.
constexpr int64_t RELIAB_LDS_V = 128 * 1024;          // bytes of LDS for V beside the staging buffers
constexpr int64_t RELIAB_SCRATCH = 64ll << 20;        // aim of the workspace slices' size (>= one slab per model)
struct SlabPlan {
  bool lds = false;
  int64_t S = 1;
  int64_t slices = 0;   // B x S
  int64_t ns = 0;
  size_t scratch() const { return lds ? 0 : (size_t)(slices * ns * 16); }
};
SlabPlan slab_plan(const SysDims& sd, int64_t B, int64_t n_items, bool lds_knob, int64_t aim);

// ---- launcher (k_reliab.hip): reliabilities of any animals of the panel from a chunk's factor ----
// rel[b * n_pred + v] for animal animals[v] (a row of geno_sm, int8 [P][n]) under model b of the chunk
// whose pipeline left L, Dinv, u, scal (and, kernel form, the packed panel) in c: one workgroup per
// (model, slab of RELIAB_W listed animals), a blocked forward substitution on fp64 MFMA.  p / vscr: the
// list's slab_plan and its scratch() doubles (null with LDS).
// The same bits either way, and for an animal wherever it stands in the list.
// With covariates (cov non-null: sq / cf / ks launch_covar's keep buffers of the same chunk; qa [2][n_pred][16]
// the listed animals' covariates, plane 0 as given (gblup models), plane 1 centred by the train means (snp
// models), zero past nc): rel holds (k_Ta^T V^-1 k_Ta - |C^-1 a_a|^2) / K_aa and pev (may be null)
// K_aa - k_Ta^T V^-1 k_Ta + |C^-1 (q~_a - a_a)|^2, with a_a = Q~_T^T V^-1 k_Ta from the cross product S^T s_a on
// fp64 MFMA (SNP form: / d); NaN also for a model whose ks is flagged.  Without: the plain reliabilities, the
// same bits as before.  launch_cov_cov: cc [B][n_cov][n_cov] = G^-1 = C^-T C^-1 from the kept factor.
constexpr int RELIAB_W = 16;
struct ReliabCov {
  const double *sq, *cf, *ks, *qa;
  int nc;
  double* pev;
};
hipError_t launch_reliab(const CholLaunch& c, const int8_t* geno_sm, const int32_t* csA, const int32_t* animals,
                         int64_t n_pred, const SlabPlan& p, double* vscr, const ReliabCov* cov, double* rel,
                         hipStream_t s);
hipError_t launch_cov_cov(const double* cf, const double* ks, int64_t B, int n_cov, double* cc, hipStream_t s);

// ---- launchers (k_loo.hip): leave-one-out cross-validation of a chunk's models from its factor ----
// For training animal ti (position in the split's `train` order; train [n_T] its rows of geno_sm) under model b of the
// chunk whose pipeline left L, Dinv, u, scal in c and whose solution launch_effects left in alpha [B][nt][ns]:
// lev[b * n_T + ti] = h_tt and pred[(b * nt + t) * n_T + ti] = y_t - e_loo,t, the prediction of the animal by the
// model fitted without it (the snp branch keeps the penalty lambda d and refits the intercept and the centring).
// One workgroup per (model, slab of LOO_W training animals) through fwd_subst.h; p / vscr: as launch_reliab, the
// plan of an n_T-item list.  The same bits either way, whatever the batch and the chunking.  NaN for a model with
// d = 0 or a flagged index.  launch_loo_fitness: rfit[b * nt + t] = |pearson(pred, y_T)| (pearson_dev.h) and
// press[b * nt + t] = sum_t e_loo,t^2 over the n_T values in order, one workgroup per (model, trait).
constexpr int LOO_W = 16;
hipError_t launch_loo(const CholLaunch& c, const int8_t* geno_sm, const int32_t* train, const double* alpha,
                      const SlabPlan& p, double* vscr, double* pred, double* lev, hipStream_t s);
hipError_t launch_loo_fitness(const CholLaunch& c, const double* pred, double* rfit, double* press, hipStream_t s);

// ---- launcher (k_score.hip): mixed-model score statistics of listed SNPs from a chunk's factor ----
// score[(b * nt + t) * n_cand + v] = w_j^T V^-1 r_t, info[b * n_cand + v] = w_j^T V^-1 w_j for column
// j = cand[v] (already wrapped to [0, P)) under model b of the chunk whose pipeline left L, Dinv, z, u and
// scal in c, and q[b * nt + t] = r_t^T V^-1 r_t (q may be null): one workgroup per (model, slab of SCORE_W
// listed SNPs), right-hand sides from the split's 2-bit packed rows, then k_reliab's forward substitution
// (fwd_subst.h).  p / vscr: as launch_reliab.  The same bits either way, and for a SNP wherever it stands in
// the list.  NaN for a model with d = 0 or a flagged index.
// With covariates (cov non-null: launch_covar's keep buffers of the same chunk, qT and n_cov as launch_covar
// has them): score / info / q hold u_P = u - (C^-1 a_j).(C^-1 h_t), v_P = v - |C^-1 a_j|^2 and
// q_P = q - h_t^T b_t with a_j = Q~_T^T V^-1 w_j from the cross product S^T s_j on fp64 MFMA; u_P = v_P = 0
// exactly where v_P <= COVAR_PIV_RTOL v; NaN also for a model whose ks is flagged and for N - r - n_cov <= 0.
// Without: the plain statistics, the same bits as before.
constexpr int SCORE_W = 16;
struct ScoreCov {
  const double *sq, *cf, *ch, *ks, *qT;
  int nc;
};
hipError_t launch_snpscore(const CholLaunch& c, const int32_t* csA, const int32_t* cand, int64_t n_cand,
                           const SlabPlan& p, double* vscr, const ScoreCov* cov, double* score, double* info,
                           double* q, hipStream_t s);

// ---- launchers (k_covar.hip): fixed-effect covariates fitted by GLS from a chunk's factor ----
// qT [2][COVAR_W][nTp] / qV [2][COVAR_W][nV]: the call's covariates of the split's train / validation rows,
// covariate-major, plane 0 as given (gblup models), plane 1 centred by the column means over the train rows
// (snp models); zero at padding rows and at columns past n_cov.  launch_covar: bhat[(b * nt + t) * n_cov + j]
// the GLS effects under model b of the chunk whose pipeline left L, Dinv, z, u and scal in c, and
// z2 [B][nt][ns] = L^-1 rhs of the adjusted phenotype (c.z is not written) -- one workgroup per model,
// k_reliab's forward substitution (fwd_subst.h) on the covariates as one slab.  p / vscr: as launch_reliab,
// the plan of a COVAR_W-item list.  NaN for a model with d = 0, a flagged
// index or covariates that are collinear over the train rows.  launch_cov_fitness: fit[b] = the mean over
// traits of |pearson(ebv_V, y_V - Q~_V b)| from ebv [B][nt][nV] (the solve on z2).
constexpr int COVAR_W = 16;
// a pivot of the covariates' Cholesky counts as positive above this fraction of its diagonal entry of
// Q~^T V^-1 Q~ (1 - R^2 of the column on the earlier ones): below it the effects have no digit left at the
// tests' 1e-9, and an exactly repeated column leaves rounding noise of either sign, ~1e-16 of the entry
constexpr double COVAR_PIV_RTOL = 1e-12;
// Keep mode of launch_covar (all four pointers or none): what the model's GLS step computed stays on the
// device for launch_snpscore's and launch_loglik's covariate adjustment.  sq [B][ns][COVAR_W] = S = L^-1 R
// (zero at padding rows and at columns past n_cov; without LDS it is vscr itself, the model's slice),
// cf [B][COVAR_W][COVAR_W] the factor C of G = C C^T (row-major, lower, identity past n_cov),
// ch [B][MAXT][COVAR_W] = C^-1 h_t, ks [B][COVAR_KS] = {log|G|, bad flag, h_t^T b_t per trait}.  With keep,
// z2 may be null: z* is then not formed.
struct CovKeep {
  double *sq = nullptr, *cf = nullptr, *ch = nullptr, *ks = nullptr;
};
enum { KS_LOGG = 0, KS_BAD = 1, KS_HB = 2, COVAR_KS = KS_HB + MAXT };
hipError_t launch_covar(const CholLaunch& c, const double* qT, int n_cov, const SlabPlan& p, double* vscr,
                        double* bhat, double* z2, const CovKeep& keep, hipStream_t s);
hipError_t launch_cov_fitness(const CholLaunch& c, const double* ebv, const double* qV, const double* bhat, int n_cov,
                              double* fit, hipStream_t s);

// ---- launchers (k_fixed.hip): a wide fixed design [Q, Z] fitted by GLS from a chunk's factor ----
// tblup_fit_group_batch's models of more than COVAR_W columns: n_cov dense covariates and the one-hot
// columns Z of a class factor of L levels, FIXED_MAX columns at most.  Column j of a model's design: covariate
// j for j < nc (qT / qV, launch_covar's planes), else level j - nc under gblup (as given) and level
// j - nc + 1 under snp (the lowest level is the reference; centred by the level's share of the train rows).
//   gT [nTp] / gV [nV]  level codes of the split's train / validation rows (-1 at padding rows)
//   lst [L + 1], lpos [n_T]  the train rows' positions by level, ascending inside a level (CSR)
//   share [L]           n_l / n_T
//   ff [Cw][Cw], fr [MAXT][Cw]  SNP form: F~_T^T F~_T and F~_T^T r_t of the snp design, once per call
// Cw: the column stride of the call's buffers, a multiple of 16 that holds every model's columns.
// launch_fixed_subst: S = L^-1 R into sbuf [B][Cw / 16][ns][16], one workgroup per (model, slab of 16 columns);
// p: the plan of a Cw-item list, its slices being sbuf's own slabs.  launch_fixed_gls: G, its blocked Cholesky,
// bhat [B][nt][Cw] (zero past the model's columns) and z2 [B][nt][ns], one workgroup per model.
// launch_fixed_fitness: launch_cov_fitness for this design.  NaN as launch_covar.
constexpr int FIXED_MAX = 128;
struct FixedDesign {
  const double *qT, *qV;
  const int32_t *gT, *gV, *lst, *lpos;
  const double *share, *ff, *fr;
  int nc, L, Cw;
};
__host__ __device__ __forceinline__ int fixed_cols(bool gblup, int nc, int L) { return nc + L - (gblup ? 0 : 1); }
hipError_t launch_fixed_subst(const CholLaunch& c, const FixedDesign& f, const SlabPlan& p, double* sbuf,
                              hipStream_t s);
// Keep mode of launch_fixed_gls (all three pointers or none), CovKeep for the wide design: cf [B][Cw][Cw] the
// factor C of G = C C^T (row-major, lower, identity past the model's columns), ch [B][MAXT][Cw] = C^-1 h_t,
// ks [B][COVAR_KS] = {log|G| summed over the model's own columns in order, bad flag, h_t^T b_t per trait}; S stays
// in sbuf as launch_fixed_subst left it.  With keep, z2 may be null: z* is then not formed.  bhat and z2 are the
// same bits with or without it.
struct FixedKeep {
  double *cf = nullptr, *ch = nullptr, *ks = nullptr;
};
hipError_t launch_fixed_gls(const CholLaunch& c, const FixedDesign& f, const double* sbuf, double* bhat, double* z2,
                            const FixedKeep& keep, hipStream_t s);
hipError_t launch_fixed_fitness(const CholLaunch& c, const FixedDesign& f, const double* ebv, const double* bhat,
                                double* fit, hipStream_t s);
// launch_snpscore for a model with the wide design (k_score.hip's FIX instances): u_P, v_P, q_P as its covariate
// form has them with F~ in place of Q~, from sbuf (launch_fixed_subst's) and launch_fixed_gls's keep buffers of the
// same chunk; f as those two launches had it (qV / gV / ff / fr are not read).  NaN also for N - r - C_m <= 0.
struct ScoreFixed {
  const double *sbuf, *cf, *ch, *ks;
  FixedDesign f;
};
hipError_t launch_snpscore_fixed(const CholLaunch& c, const int32_t* csA, const int32_t* cand, int64_t n_cand,
                                 const SlabPlan& p, double* vscr, const ScoreFixed& fx, double* score, double* info,
                                 double* q, hipStream_t s);
// launch_reliab for a model with the wide design (k_reliab.hip's FIX instances): rel and pev as its covariate form
// has them with F~ in place of Q~, from sbuf (launch_fixed_subst's) and launch_fixed_gls's keep buffers of the same
// chunk; f as those two launches had it (only share, nc, L and Cw are read).  qa [2][n_pred][16]: ReliabCov's;
// ga [n_pred]: the listed animals' level codes (-1: no level, every level entry of the design row is then its
// centre alone).  launch_fixed_cov: fc [B][nc + L][nc + L] = G^-1 = C^-T C^-1 from the kept factor, covariates then
// levels; the reference level's row and column of an snp model are zeros; NaN throughout for a flagged model.
struct ReliabFixed {
  const double *sbuf, *cf, *ks, *qa;
  const int32_t* ga;
  FixedDesign f;
  double* pev;
};
hipError_t launch_reliab_fixed(const CholLaunch& c, const int8_t* geno_sm, const int32_t* csA, const int32_t* animals,
                               int64_t n_pred, const SlabPlan& p, double* vscr, const ReliabFixed& fx, double* rel,
                               hipStream_t s);
hipError_t launch_fixed_cov(const CholLaunch& c, const FixedDesign& f, const double* cf, const double* ks, double* fc,
                            hipStream_t s);

// ---- launcher (k_loglik.hip): profile (restricted) log-likelihood of every model of a chunk ----
// loglik[b * nt + t] and sigma2[b * nt + t] (the profiled sigma2_g) from the pivots on Dinv's diagonals,
// z and the scalars that the chunk's pipeline left in c (SNP form: also the split's yT / ymu); one
// workgroup per model, fixed-order sums, so a model's bits do not depend on the chunk around it.
// NaN for d = 0, a flagged index or a quadratic form that is not positive and finite.
// With covariates (ks non-null: launch_covar's keep.ks of the same chunk at the same h2; lqq [2] =
// log|Q~_T^T Q~_T| of the gblup and of the snp plane, NaN for a plane that is not of full rank):
// q_P = q - h_t^T b_t, dof = N - r - n_cov, log|A^T V A| = log|V| - r log lambda + log|G| - lqq.  NaN also
// for a model whose ks is flagged and for dof <= 0.  With ks null: the plain likelihood, the same bits.
hipError_t launch_loglik(const CholLaunch& c, const double* ks, const double* lqq, int n_cov, double* loglik,
                         double* sigma2, hipStream_t s);
// The same with a column count per plane (the wide design: ks launch_fixed_gls's keep.ks, lqq [2] =
// log|F~_T^T F~_T|): dof = N - r - cols[0] for a gblup model, N - r - cols[1] for an snp model, each in
// [0, FIXED_MAX].
hipError_t launch_loglik_fixed(const CholLaunch& c, const double* ks, const double* lqq, const int (&cols)[2],
                               double* loglik, double* sigma2, hipStream_t s);

// ---- launcher (k_model.hip): EBVs of any animals of the panel from fitted models ----
// ebv[(m * nt + t) * n_pred + v] = intercept[m * nt + t] + sum_j (x[animals[v], idx_j] - center_j)
// effects[t * plane + j], j = off[m] .. off[m + 1] in that order for every animal (the same bits
// wherever the animal stands in the list).  geno_sm: int8 [P][n]; indices wrap as snp_col.
hipError_t launch_predict(const int8_t* geno_sm, int64_t n, int64_t P, const int32_t* animals, int64_t n_pred,
                          const int64_t* idx, const int64_t* off, int64_t B, const double* intercept,
                          const double* center, const double* effects, int64_t plane, int nt, double* ebv,
                          hipStream_t s);

// ---- launcher (k_decode.hip): RandomKey genome decode, top-k of each key row ----
hipError_t launch_decode_topk(const double* keys, int64_t B, int64_t d, int64_t ld, const int64_t* off, int64_t* out,
                              hipStream_t s);

// ---- launchers (k_de.hip): one DE generation (mutation + binary crossover + clip) per individual ----
// The request, and the kernels' by-value argument: every pointer is device memory.  The caller
// value-initialises it and fills what its form reads by name; dbg, keep_end and MDE_pBX's strategy
// are the launchers'.
struct DeArgs {
  const uint32_t* key;     // numpy key[624] at the generation's first draw
  int pos0;                // numpy pos (0..624)
  const uint32_t* polys;   // [pop][624]: row i-1 -> individual i >= 1; row pop-1 -> end state
  int end_jump;            // end window by polys[pop-1] (else the base key itself)
  int end_s, end_pos;      // numpy key = end ring words [end_s, end_s + 624), pos = end_pos
  const double* parent;    // [pop][ldp]
  int64_t ldp;
  const int32_t* donors;   // [pop][3]
  const int64_t* fixed;    // [pop]
  int strategy;            // 0 rand/1, 1 current-to-best/1
  double F, cr;
  int clip;
  double hi;               // clip upper bound (dimensionality - 1)
  int64_t L;               // genome length
  int pop;
  double* child;           // [pop][ldc]
  int64_t ldc;
  uint32_t* key_out;       // [624]
  int32_t* pos_out;
  int dbg;                 // phase-ablation timing only (env TBLUP_DE_DBG, diagnostic builds; results wrong):
                           // 1 no jump correlation, 2 no mask recurrence, 4 no stream
  // per-individual strategy / F / crossover rate ([pop] each; null: the scalars above) -- SaDE
  // (evolver.py:407-547): each individual's strategy by python's random.random() < p, its own cr
  const int32_t* strat_i;
  const double* F_i;
  const double* cr_i;
  // MDE_pBX (evolver.py:550-687; the kernels' general form): individual i's uniforms start at word
  // f_i[i] of its window (any offset: its np.random.choice draws come first), its target and the
  // child's base are row target_i[i]; keep_end: k_de_jump leaves the end window in gwin row pop
  const int64_t* f_i;
  const int32_t* target_i;
  int keep_end;
};
// scratch (null: one launch): DE_SEQ_SCRATCH words for the base sequence, then 624 per window (pop of
// them; MDE_pBX pop + 1) -- the three-launch form for populations larger than the CU count
constexpr int64_t DE_SEQ_SCRATCH = 624 + 19937 + 624 + 64;
// the classic step: everything above f_i
hipError_t launch_de_step(const DeArgs& a, uint32_t* scratch, hipStream_t s);
// MDE_pBX in two halves.  The draws read key, pos0, polys, end_jump and pop: every individual's
// window, then the tempered words [tab[2i], tab[2i+1]) past 2Li of its stream into words + woff[i]
// (what its np.random.choice draws can read).  The step, once the host has resolved them: F_i, cr_i,
// f_i and target_i per individual, the end state end_s words into the end window; with scratch it
// reads the windows the draws' launch left there.
hipError_t launch_mde_draws(const DeArgs& a, const int32_t* tab, const int64_t* woff, uint32_t* words,
                            uint32_t* scratch, hipStream_t s);
hipError_t launch_mde_step(const DeArgs& a, uint32_t* scratch, hipStream_t s);

// ---- launcher (k_de.hip): rows from scattered device rows into one matrix (up to ROWPTRS rows
//      per launch, source pointers in the kernel arguments) ----
constexpr int ROWPTRS = 128;
struct RowPtrs {
  const double* p[ROWPTRS];
};
hipError_t launch_gather_rows(double* dst, int64_t ldd, int64_t L, const RowPtrs& src, int nr, hipStream_t s);

// ---- launcher (k_scan.hip): per-SNP sums over a set of animals (seeder GWAS metric) ----
hipError_t launch_snp_scan(const int8_t* geno_sm, int64_t n, int64_t P, const int32_t* rows, int64_t nr,
                           const double* yc, int64_t* sx, int64_t* sxx, double* sxy, hipStream_t s);

// XCD-aware bijective remap of a 1-D block id (blocks b and b+8 share an XCD
// under the observed round-robin placement; speed only, never correctness).
__device__ __forceinline__ int64_t xcd_remap(int64_t orig, int64_t nwg) {
  if (nwg <= 8) return orig;
  int64_t q = nwg / 8, r = nwg % 8, xcd = orig % 8;
  int64_t base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + orig / 8;
}

}  // namespace tblup
