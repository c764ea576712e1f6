// ===========================================================================
// SNP form: every system tile (I >= J) of the batch in one launch, before the column loop:
// C = A B^T over the n_T train animals on FP4 MFMA (16x16x128, e2m1 operands, fp32 accumulate),
// 2-bit packed split rows read in place.  Genotype code g read as an e2m1 nibble is g / 2 (0, 0.5,
// 1.0), so a packed dword's even fields become nibbles by x & 0x33333333 and its odd fields by
// (x >> 2) & 0x33333333 -- 3 VALU ops per 16 animals into 2 operand dwords (the int8 form spent 7
// per 16 animals) -- and both operands carry the E8M0 scale 2.0; the counts (<= 4 n_T < 2^24)
// accumulate exactly in fp32 at twice the int8 rate.  The animals' order inside k is the same for A and B, so A B^T is unchanged.
// 4 waves per workgroup; wave (qr, qc) computes a 64 x 64 quadrant = 4 x 4 blocks; 256-animal
// stages through a 3-deep LDS-DMA ring (48 KiB, three workgroups per CU).  A rows are read
// through pi(rho) so the counts land in the f64 accumulator layout.  Off-diagonal tiles store
// the exact counts as int16 where the off-diagonal kernel's lanes read them (kc, see
// tblup_internal.h); diagonal tiles store the exact counts of their 36 lower blocks the same way
// (kd: 18 KiB a tile instead of 72 KiB of fp64 K_JJ + lambda I -- the diagonal kernel and the
// D-units form those values where they read them, kd_block in k_chol.hip).  (Rows stored as nibbles --
// twice the bytes, no unpack -- measured no faster: those loads then bound the launch.)
// ===========================================================================
#include "chol_dev.h"
#include "k_stats.h"
#include <algorithm>

namespace tblup {

constexpr int STW = 4;   // waves per system-tile workgroup

// K_JJ + lambda I (identity on padding rows) from a diagonal tile's accumulators (exact counts in
// fp32) as packed fp64 blocks into Kd: the tiles J < 2, which the diagonal kernel reads directly
// (sc / ub: the system's scalars and tile J's centring sums -- scal / u, or their LDS copies)
__device__ __forceinline__ void sys_diag_epilogue_src(const CholArgs& a, const v4f (&cnt)[4][4], int64_t b, int J, int qr,
                                                      int qc, int l, const double* sc, const double* ub) {
  const int64_t j0 = (int64_t)J * TILE;
  const double sa_ = sc[SC_SA], cN = sc[SC_CN], invd = sc[SC_INVD], lam = sc[SC_LAM], sm = sc[SC_SM];
  const int64_t nrow = (int64_t)sc[SC_NROW], pad = (int64_t)sc[SC_PAD];
  double* Kd = a.Kd + (b * a.NT + J) * (int64_t)NPACK * BLKD;
  // every centring sum this lane needs, loaded before the first store (Kd and u are both double
  // pointers: loads interleaved with the stores were issued one after another, ~47 us a launch)
  double ur[4][4], uc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) ur[m][r] = ub[16 * (4 * qr + m) + (l >> 4) + 4 * r];
#pragma unroll
  for (int n = 0; n < 4; ++n) uc[n] = ub[16 * (4 * qc + n) + (l & 15)];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int cb = 4 * qr + m, ib = 4 * qc + n;
      if (cb < ib) continue;
      const int il = 16 * ib + (l & 15);
      const int64_t gj = j0 + il;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cl = 16 * cb + (l >> 4) + 4 * r;
        const int64_t gi = j0 + cl;
        const double kv = grm_value((int32_t)cnt[m][n][r], ur[m][r], uc[n], sa_, cN, invd, sm);
        const double v = (sys_real(gi, pad, nrow) && sys_real(gj, pad, nrow)) ? kv + ((gi == gj) ? lam : 0.0)
                                                                              : ((gi == gj) ? 1.0 : 0.0);
        double* d = Kd + pk(cb, ib) + bo(cl & 15, il & 15);
        *d = v;
      }
    }
}
// the same from scal / u
__device__ __forceinline__ void sys_diag_epilogue_inl(const CholArgs& a, const v4f (&cnt)[4][4], int64_t b, int J, int qr,
                                                      int qc, int l) {
  sys_diag_epilogue_src(a, cnt, b, J, qr, qc, l, a.scal + b * SCAL, a.u + b * a.prow + (int64_t)J * TILE);
}
// k_sys_tiles' call: a plain function, which the compiler inlines late, where _inl is inlined at once.
// No register reason is left for it: with _inl called directly the kernel builds to the same
// registers (55 / 63 SGPRs, 160 VGPRs, 3 waves per SIMD) and the same number of instructions, and only
// the operand order of the epilogue's address ORs changes (so does k_sys_diag_counts' when it calls
// this one instead of _inl).  Both calls stay as they were measured, so that a rebuild can be checked
// against that code instruction for instruction (tools/asm_kernel_diff.py).
__device__ void sys_diag_epilogue(const CholArgs& a, const v4f (&cnt)[4][4], int64_t b, int J, int qr, int qc, int l) {
  sys_diag_epilogue_inl(a, cnt, b, J, qr, qc, l);
}

// a diagonal tile's counts as int16 (diag): its 36 lower blocks (cb >= ib) only, packed block
// e = cb (cb + 1) / 2 + ib, lane order of the f64 C layout (kd_load / kd_block read them); an
// off-diagonal tile's: store_counts16's layout
// The super-tile kernel's counted ring waits (k_sys_tiles_st) leave the VMEM ops younger than the
// stage they wait for outstanding: ST_STAGE_OPS LDS-DMA loads per lane for each later stage (issue():
// two rows x A and B) and, after a unit of two off-diagonal tiles, this function's stores -- one 8-B
// store per 16 x 16 block of the wave's 4 x 4 quadrant (all 16 off the diagonal: addresses 512 B
// apart within a lane, never merged).  A count above the real number only waits for more.
constexpr int ST_STAGE_OPS = 4;
constexpr int ST_TILE_STORES = 4 * 4;
constexpr int ST_UNIT_STORES = 2 * ST_TILE_STORES;
static_assert(2 * ST_STAGE_OPS + ST_UNIT_STORES < 64, "vmcnt holds 6 bits");
__device__ __forceinline__ void store_counts16_any(int16_t* kt, const v4f (&cnt)[4][4], int qr, int qc, int l,
                                                   bool diag) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int cb = 4 * qr + m, ib = 4 * qc + n;
      if (diag && cb < ib) continue;
      const v4f c = cnt[m][n];
      const int2 packed = {(int)((uint32_t)((int)c[0] & 0xffff) | ((uint32_t)(int)c[1] << 16)),
                           (int)((uint32_t)((int)c[2] & 0xffff) | ((uint32_t)(int)c[3] << 16))};
      nt_store2(kt + ((diag ? cb * (cb + 1) / 2 + ib : ib * 8 + cb) * 64 + l) * 4, packed);
    }
}
// two packed dwords (32 animals) -> one fp4 MFMA operand (even fields, odd fields of each): the
// 2-bit code g lands in the low half of a nibble, e2m1 value g / 2 (0, 0.5 subnormal, 1.0), and
// the E8M0 operand scales 2.0 (128) restore g -- 3 VALU ops per packed dword instead of 4
__device__ __forceinline__ v4i fp4_operand(uint32_t x0, uint32_t x1) {
  constexpr uint32_t M = 0x33333333u;
  return v4i{(int)(x0 & M), (int)((x0 >> 2) & M), (int)(x1 & M), (int)((x1 >> 2) & M)};
}
// the scaled f8f6f4 MFMA with fp4 operands in 4 VGPRs each (the clang builtin types them as 8 VGPRs,
// the upper half unused by fp4 -- 32 more VGPRs and a zeroing move per operand)
__device__ v4f mfma_fp4_16x16x128(v4i a, v4i b, v4f c, int cbsz, int blgp, int opsel_a, int scale_a, int opsel_b,
                                  int scale_b) __asm("llvm.amdgcn.mfma.scale.f32.16x16x128.f8f6f4.v4i32.v4i32");

template <bool DUAL>   // kernel form: the gathered panel's packed animal rows
__global__ __launch_bounds__(64 * STW, 2) void k_sys_tiles(CholArgs a, int16_t* kc, int ntri) {
  constexpr int D = 3;                 // 64-B stages (256 animals) in the LDS ring (48 KiB: 3 workgroups per CU)
  constexpr int TB = TILE * 64;        // one operand image of a stage: 8 KiB
  __shared__ __attribute__((aligned(16))) uint8_t lds[D * 2 * TB];   // 64 KiB
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, qr = w >> 1, qc = w & 1;
  WgTrace tr(a.wgt);
  const int64_t lg = xcd_remap(blockIdx.x, gridDim.x);   // an individual's tiles on one XCD
  const int64_t b = lg / ntri;
  const int t = (int)(lg % ntri);   // tri_decode(t, I, J), written out: this kernel's instruction order
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  const int J = t - I * (I + 1) / 2;
  const bool compute = (I != J) || (qr >= qc);   // diagonal tile: the upper quadrant is never read
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)J * TILE;
  const double* sc = a.scal + b * SCAL;
  const int64_t nblk = (int64_t)sc[SC_CBLK];
  const int64_t nst = (nblk + 3) >> 2;
  const int tail_ch = (int)(nblk & 3);
  // loader: wave w fills rows 16 (2w + h) + (l >> 2), h = 0, 1, of both operand images
  const uint8_t* sa[2];
  const uint8_t* sb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 16 * (2 * w + h) + (l >> 2), pos = l & 3;
    sa[h] = (DUAL ? row_dpk(a, b, j0 + row) : row_packed(a, b, j0 + row)) + pk_swz_a(row, pos);
    sb[h] = (DUAL ? row_dpk(a, b, i0 + row) : row_packed(a, b, i0 + row)) + pk_swz_b(row, pos);
  }
  auto issue = [&](int64_t st) {
    uint8_t* slot = lds + (int)(st % D) * 2 * TB;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      glds16_asm(sa[h] + st * 64, slot + (2 * w + h) * 1024);
      glds16_asm(sb[h] + st * 64, slot + TB + (2 * w + h) * 1024);
    }
  };
  v4f cnt[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) cnt[m][n] = v4f{0.f, 0.f, 0.f, 0.f};
  for (int64_t st = 0; st < D - 1 && st < nst; ++st) issue(st);
  const int rho = l & 15, prow = (rho >> 2) + 4 * (rho & 3), ch = l >> 4;
  for (int64_t st = 0; st < nst; ++st) {
    if (st + D - 2 < nst) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 2) * 4) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (st + D - 1 < nst) issue(st + D - 1);
    if (compute && !(a.skip & (1 << 18))) {
      const uint8_t* As = lds + (int)(st % D) * 2 * TB;
      const uint8_t* Bs = As + TB;
      const bool ztail = (st == nst - 1 && tail_ch != 0 && ch >= tail_ch);   // past the training animals
      uint4 aq[4], bq[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        aq[m] = *reinterpret_cast<const uint4*>(As + i8off_a(16 * (4 * qr + m) + prow, ch));
        bq[m] = *reinterpret_cast<const uint4*>(Bs + i8off_b(16 * (4 * qc + m) + rho, ch));
        if (ztail) bq[m] = uint4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        v4i av[4], bv[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          av[m] = s2 == 0 ? fp4_operand(aq[m].x, aq[m].y) : fp4_operand(aq[m].z, aq[m].w);
          bv[m] = s2 == 0 ? fp4_operand(bq[m].x, bq[m].y) : fp4_operand(bq[m].z, bq[m].w);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)   // cbsz = blgp = 4: A, B in fp4; E8M0 scales 128 = 2.0
            cnt[m][n] = mfma_fp4_16x16x128(av[m], bv[n], cnt[m][n], 4, 4, 0, 128, 0, 128);
      }
    }
  }
  if (compute && I == J && J < 2 && !(a.skip & (1 << 17)))
    sys_diag_epilogue(a, cnt, b, J, qr, qc, l);   // read directly by the diagonal kernel
  else if (compute && !(a.skip & (I != J ? 1 << 16 : 1 << 17)))
    store_counts16_any(I != J ? kc + kc_tile(a.NT, b, I, J) : a.kd + kd_tile(a.NT, b, J), cnt, qr, qc, l, I == J);
  tr.done(WGT_SYS, J, I, b);
}

// Persistent super-tile form of k_sys_tiles (large batches, sys_tiles_grid): one 8-wave workgroup
// per CU walks a contiguous run of units, a unit being a 256 x 256 super-tile = the 2 x 2 tiles
// (I0 + ti, J0 + tj), I0 = 2 SI, J0 = 2 SJ, SI >= SJ, of one individual (10 units at NT = 8 instead
// of 36 tile workgroups).  Per 256-animal stage a unit loads 2 x 256 rows (32 KiB: half the bytes
// per tile of the single-tile form) and runs 64 MFMAs per wave: wave (tj, qr, qc) accumulates
// quadrant (qr, qc) of tiles (I0, J0 + tj) and (I0 + 1, J0 + tj) (A fragments shared).  The
// 3-deep LDS-DMA ring runs on across unit boundaries (the next unit's first stages load while
// this one's last stage computes and its counts are stored), so the per-tile prologue and store
// latency of 36 short workgroups is paid once per run.  Row addresses come from a per-individual
// row table in LDS (no global load whose use would drain the ring).  The same exact fp32 counts as
// k_sys_tiles (every partial sum an integer below 2^24), stored to the same places.
constexpr int SPW = 8;                 // waves per super-tile workgroup
constexpr int SP_MAXIND = 64;          // individuals in one workgroup's run (sys_tiles_grid checks)
constexpr int64_t SYS_ST_MIN = 4;      // auto: at least this many units per CU

template <bool DUAL>   // kernel form: the gathered panel's packed animal rows
__global__ __launch_bounds__(64 * SPW, 1) void k_sys_tiles_st(CholArgs a, int16_t* kc, int nsu, int nunits) {
  constexpr int D = 3;                 // stages in the ring (the waits are written for 1-2 stages ahead: D <= 4)
  constexpr int TB2 = 2 * TILE * 64;   // one 256-row operand image of a stage: 16 KiB
  __shared__ __attribute__((aligned(16))) uint8_t lds[D * 2 * TB2];   // 96 KiB
  __shared__ int32_t rowtab[SP_ROWTAB];
  __shared__ int32_t cblk_tab[SP_MAXIND];   // contraction blocks of the run's individuals (SNP form:
                                            // n_Tp / 64 each, SC_CBLK -- not read from scal, so this
                                            // launch may precede the scalars' k_stats_diag_counts)
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int tj = w >> 2, qr = (w >> 1) & 1, qc = w & 1;
  const int NT = a.NT;
  WgTrace tr(a.wgt);
  const int u0 = (int)((int64_t)blockIdx.x * nunits / gridDim.x), u1 = (int)((int64_t)(blockIdx.x + 1) * nunits / gridDim.x);
  const int b_first = u0 / nsu;
  const int rho = l & 15, prow = (rho >> 2) + 4 * (rho & 3), ch = l >> 4;
  const int pos = l & 3;
  // super-tile s of the lower triangle (row-major): SI, SJ
  auto unit_tiles = [&](int u, int& b, int& I0, int& J0) __attribute__((always_inline)) {
    b = __builtin_amdgcn_readfirstlane(u / nsu);
    const int s = __builtin_amdgcn_readfirstlane(u % nsu);   // (tri_decode written out, as above)
    int SI = 0;
    while ((SI + 1) * (SI + 2) / 2 <= s) ++SI;
    I0 = 2 * SI;
    J0 = 2 * (s - SI * (SI + 1) / 2);
  };
  // the row table of individual b: packed row index of each of its ns system rows (row P: zero)
  int tab_b = -1;
  auto load_rowtab = [&](int b) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int64_t o0 = a.off[b], k = a.off[b + 1] - o0;
    const int64_t pad = a.padfirst ? a.ns - k : 0;
    const int nrt = 2 * TILE * ((NT + 1) / 2);   // rows a super-tile reads (ns rounded up to 256)
    if constexpr (!DUAL) {
      for (int r = t; r < nrt; r += 64 * SPW)
        rowtab[r] = (int32_t)(r < a.ns && sys_real(r, pad, k) ? snp_col(a.idx[o0 + r - pad], a.P) : a.P);
    } else {   // kernel form: the panel's own rows (past ns: any row -- those tiles are not stored)
      for (int r = t; r < nrt; r += 64 * SPW) rowtab[r] = r < a.ns ? r : 0;
    }
    __syncthreads();
    tab_b = b;
  };
  // issue cursor: the unit and stage whose loads go out next, and its row pointers
  int iu = u0, ib = 0;
  int ist = 0, inst = 0;
  int ra[2], rb[2];                    // packed rows of this lane's A / B loads (h = 0, 1)
  const uint8_t* gbase = nullptr;
  const int64_t gsr = DUAL ? a.pstride / a.prow : a.gs_row;   // packed row bytes
  // (pk_swz_a / pk_swz_b of rows l >> 2 and 16 + (l >> 2), written out: this kernel's registers)
  const int offa[2] = {16 * (pos ^ (((l >> 2) >> 2) & 3)), 16 * (pos ^ (((16 + (l >> 2)) >> 2) & 3))};
  const int offb[2] = {16 * (pos ^ (((l >> 2) >> 2) & 2)), 16 * (pos ^ (((16 + (l >> 2)) >> 2) & 2))};
  auto setup_issue = [&]() __attribute__((always_inline)) {
    int I0, J0;
    unit_tiles(iu, ib, I0, J0);
    if (ib != tab_b) load_rowtab(ib);
    inst = (cblk_tab[ib - b_first] + 3) >> 2;
    gbase = DUAL ? a.panel + ib * a.pstride : a.ft.gpk[fold_of(a.ft, ib)];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 16 * (2 * w + h) + (l >> 2);
      ra[h] = rowtab[J0 * TILE + row];
      rb[h] = rowtab[I0 * TILE + row];
    }
    ist = 0;
  };
  // issue one stage into ring slot g % D and advance the cursor (false: nothing left)
  auto issue = [&](int g) __attribute__((always_inline)) {
    if (iu >= u1) return;
    uint8_t* slot = lds + (g % D) * 2 * TB2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      glds16_asm(gbase + (int64_t)ra[h] * gsr + (offa[h] + ist * 64), slot + (2 * w + h) * 1024);
      glds16_asm(gbase + (int64_t)rb[h] * gsr + (offb[h] + ist * 64), slot + TB2 + (2 * w + h) * 1024);
    }
    if (++ist == inst && ++iu < u1) setup_issue();
  };
  if (u0 >= u1) return;
  const int nind = (u1 - 1) / nsu - b_first + 1;
  if (t < nind) {   // kernel form: the individual's k SNPs
    const int64_t bt = b_first + t;
    cblk_tab[t] = (int32_t)(DUAL ? (a.off[bt + 1] - a.off[bt] + KBLK - 1) / KBLK : a.ytp / KBLK);
  }
  __syncthreads();
  setup_issue();
  // total stages of the run (the units of one individual share its stage count)
  int nstages = 0;
  for (int u = u0; u < u1;) {
    const int b = u / nsu, ue = min(u1, (b + 1) * nsu);
    nstages += (ue - u) * ((cblk_tab[b - b_first] + 3) >> 2);
    u = ue;
  }
  for (int g = 0; g < D - 1; ++g) issue(g);

  v4f cnt[2][4][4];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) cnt[ti][m][n] = v4f{0.f, 0.f, 0.f, 0.f};
  // compute cursor
  int cu = u0, cb_ = 0;
  int cI0 = 0, cJ0 = 0, cst = 0;
  unit_tiles(cu, cb_, cI0, cJ0);
  int cnblk = cblk_tab[cb_ - b_first];
  int cnst = (int)((cnblk + 3) >> 2);
  bool stored_full = false;   // the previous stage ended a unit whose every wave stored 32 count pairs
  for (int g = 0; g < nstages; ++g) {
    // stage g's loads done: the younger ops are the 4 loads of each stage issued after it (up to
    // D - 2) and the stores of the unit that ended last stage (32 per wave after a full
    // off-diagonal super-tile: 16 8-B stores per tile whose addresses lie 512 B apart within a
    // lane, so none can be merged; any other unit: waited for)
    const int ahead = min(D - 2, nstages - 1 - g);   // stages issued after stage g
    if (ahead >= 2) {
      if (stored_full)
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * ST_STAGE_OPS + ST_UNIT_STORES) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * ST_STAGE_OPS) : "memory");
    } else if (ahead == 1) {
      if (stored_full)
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(ST_STAGE_OPS + ST_UNIT_STORES) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(ST_STAGE_OPS) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    issue(g + D - 1);
    const int J0t = cJ0 + tj;
    bool comp[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
      const int I = cI0 + ti;
      comp[ti] = I < NT && J0t < NT && (I > J0t || (I == J0t && qr >= qc));
    }
    if ((comp[0] || comp[1]) && !(a.skip & (1 << 18))) {
      const uint8_t* As = lds + (g % D) * 2 * TB2;
      const uint8_t* Bs = As + TB2;
      const int tail_ch = (int)(cnblk & 3);
      const bool ztail = (cst == cnst - 1 && tail_ch != 0 && ch >= tail_ch);   // past the training animals
      uint4 aq[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) aq[m] = *reinterpret_cast<const uint4*>(As + i8off_a(TILE * tj + 16 * (4 * qr + m) + prow, ch));
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        if (!comp[ti]) continue;
        uint4 bq[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          bq[n] = *reinterpret_cast<const uint4*>(Bs + i8off_b(TILE * ti + 16 * (4 * qc + n) + rho, ch));
          if (ztail) bq[n] = uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          v4i av[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) av[m] = s2 == 0 ? fp4_operand(aq[m].x, aq[m].y) : fp4_operand(aq[m].z, aq[m].w);
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const v4i bv = s2 == 0 ? fp4_operand(bq[n].x, bq[n].y) : fp4_operand(bq[n].z, bq[n].w);
#pragma unroll
            for (int m = 0; m < 4; ++m)   // cbsz = blgp = 4: A, B in fp4; E8M0 scales 128 = 2.0
              cnt[ti][m][n] = mfma_fp4_16x16x128(av[m], bv, cnt[ti][m][n], 4, 4, 0, 128, 0, 128);
          }
        }
      }
    }
    stored_full = false;
    if (++cst == cnst) {
      // the unit's epilogue: its tiles' counts (diagonal tiles J < 2 too: k_sys_diag_counts forms
      // their K_JJ + lambda I afterwards -- the fp64 epilogue here would spill the accumulators)
      stored_full = cI0 != cJ0 && cI0 + 1 < NT && !(a.skip & (1 << 16));
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        const int I = cI0 + ti;
        if (!comp[ti]) continue;
        if (!(a.skip & (I != J0t ? 1 << 16 : 1 << 17))) {
          store_counts16_any(I != J0t ? kc + kc_tile(NT, cb_, I, J0t) : a.kd + kd_tile(NT, cb_, J0t), cnt[ti], qr, qc, l,
                             I == J0t);
        }
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n) cnt[ti][m][n] = v4f{0.f, 0.f, 0.f, 0.f};
      if (++cu < u1) {
        unit_tiles(cu, cb_, cI0, cJ0);
        cnblk = cblk_tab[cb_ - b_first];
        cnst = (int)((cnblk + 3) >> 2);
      }
      cst = 0;
    }
  }
  tr.done(WGT_SYS, 0, 0, u0 / nsu);
}

// Fold-fused evaluation with shared counts (IntraGCV's folds, tblup_eval_folds*): when every fold's
// training rows R_f and validation rows V_f make up the same multiset T_all, C_{R_f} = C_{T_all} -
// C_{V_f}.  One workgroup per (individual b, tile) accumulates C_{T_all} over fold 0's rows
// [0, nRp) (train, zero padding, validation, zero padding), then for f = 0 .. F-1 adds C_{V_{f-1}}
// back (f > 0) and subtracts C_{V_f} -- the A operand negated through the e2m1 sign bits -- and
// stores system f * B + b's tile after each subtraction.  The stage sequence runs through one
// 3-deep LDS-DMA ring across these segments.  Every partial sum is an exact integer in fp32, so
// the tiles equal k_sys_tiles' per-fold ones bit for bit; contraction (nRp + (2F - 1) nVp) / (F nTp)
// of the per-fold launch's (config 2, 5 folds of 256: 14 stages of 256 animals instead of 20).
__global__ __launch_bounds__(64 * STW, 2) void k_sys_tiles_folds(CholArgs a, int16_t* kc, int ntri) {
  constexpr int D = 3;
  constexpr int TB = TILE * 64;
  __shared__ __attribute__((aligned(16))) uint8_t lds[D * 2 * TB];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, qr = w >> 1, qc = w & 1;
  WgTrace tr(a.wgt);
  const int64_t lg = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t b = lg / ntri;   // individual: system b of fold 0
  const int t = (int)(lg % ntri);   // tri_decode(t, I, J), written out: this kernel's instruction order
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  const int J = t - I * (I + 1) / 2;
  const bool compute = (I != J) || (qr >= qc);
  const int64_t i0 = (int64_t)I * TILE, j0 = (int64_t)J * TILE;
  const int F = a.ft.nf;
  const int64_t bpf = a.ft.bpf;
  const int64_t vbyte = a.ytp / 4;                           // validation rows start (nTp animals)
  const int64_t nblkA = a.gs_row / 16, nsA = (nblkA + 3) >> 2;   // all nRp animals, 64 per block
  const int64_t nblkV = nblkA - a.ytp / 64, nsV = (nblkV + 3) >> 2;
  const int64_t nst = nsA + (2 * F - 1) * nsV;
  // the same SNP rows in every fold's layout: per-lane row offsets, fold bases per stage
  int64_t oa[2], ob[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 16 * (2 * w + h) + (l >> 2), pos = l & 3;
    oa[h] = (row_packed(a, b, j0 + row) - a.ft.gpk[0]) + pk_swz_a(row, pos);
    ob[h] = (row_packed(a, b, i0 + row) - a.ft.gpk[0]) + pk_swz_b(row, pos);
  }
  // stage g -> segment k (0: T_all of fold 0, 2f + 1: minus V_f, 2f + 2: plus V_f) and its stage
  auto seg_of = [&](int64_t g, int& k, int64_t& st) {
    if (g < nsA) {
      k = 0;
      st = g;
    } else {
      k = 1 + (int)((g - nsA) / nsV);
      st = (g - nsA) % nsV;
    }
  };
  auto issue = [&](int64_t g) __attribute__((always_inline)) {
    int k;
    int64_t st;
    seg_of(g, k, st);
    const uint8_t* base = a.ft.gpk[k == 0 ? 0 : (k - 1) >> 1] + (k == 0 ? 0 : vbyte) + st * 64;
    uint8_t* slot = lds + (int)(g % D) * 2 * TB;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      glds16_asm(base + oa[h], slot + (2 * w + h) * 1024);
      glds16_asm(base + ob[h], slot + TB + (2 * w + h) * 1024);
    }
  };
  v4f cnt[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) cnt[m][n] = v4f{0.f, 0.f, 0.f, 0.f};
  for (int64_t g = 0; g < D - 1 && g < nst; ++g) issue(g);
  const int rho = l & 15, prow = (rho >> 2) + 4 * (rho & 3), ch = l >> 4;
  int64_t g = 0;
  for (int k = 0; k < 2 * F; ++k) {
    const int64_t ns_k = k == 0 ? nsA : nsV;
    const int tail_ch = (int)((k == 0 ? nblkA : nblkV) & 3);
    const int neg = (k & 1) ? (int)0x88888888u : 0;   // e2m1 sign bits: subtract this segment
    for (int64_t st = 0; st < ns_k; ++st, ++g) {
      if (g + D - 2 < nst) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 2) * 4) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      if (g + D - 1 < nst) issue(g + D - 1);
      if (compute) {
        const uint8_t* As = lds + (int)(g % D) * 2 * TB;
        const uint8_t* Bs = As + TB;
        const bool ztail = (st == ns_k - 1 && tail_ch != 0 && ch >= tail_ch);   // past the segment's rows
        uint4 aq[4], bq[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          aq[m] = *reinterpret_cast<const uint4*>(As + i8off_a(16 * (4 * qr + m) + prow, ch));
          bq[m] = *reinterpret_cast<const uint4*>(Bs + i8off_b(16 * (4 * qc + m) + rho, ch));
          if (ztail) bq[m] = uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          v4i av[4], bv[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            av[m] = s2 == 0 ? fp4_operand(aq[m].x, aq[m].y) : fp4_operand(aq[m].z, aq[m].w);
            av[m] |= neg;
            bv[m] = s2 == 0 ? fp4_operand(bq[m].x, bq[m].y) : fp4_operand(bq[m].z, bq[m].w);
          }
#pragma unroll
          for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n)
              cnt[m][n] = mfma_fp4_16x16x128(av[m], bv[n], cnt[m][n], 4, 4, 0, 128, 0, 128);
        }
      }
    }
    if (!(k & 1) || !compute) continue;
    const int64_t s = (int64_t)((k - 1) >> 1) * bpf + b;   // C_{T_all} - C_{V_f}: system f * B + b
    store_counts16_any(I != J ? kc + kc_tile(a.NT, s, I, J) : a.kd + kd_tile(a.NT, s, J), cnt, qr, qc, l, I == J);
  }
  tr.done(WGT_SYS, J, I, b);
}

// fold-fused chunks (k_sys_tiles_folds stores every diagonal tile's counts): K_JJ + lambda I of the
// tiles J < 2 into Kd, one 4-wave workgroup per (system, J)
__global__ __launch_bounds__(64 * STW) void k_sys_diag_counts(CholArgs a) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, qr = w >> 1, qc = w & 1;
  const int64_t s = blockIdx.x >> 1;
  const int J = (int)(blockIdx.x & 1);
  if (qr < qc || J >= a.NT) return;   // the upper quadrant is never read
  v4f cnt[4][4];   // the inverse of store_counts16_any(..., diag = true)
  const int16_t* kt = a.kd + kd_tile(a.NT, s, J);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int cb = 4 * qr + m, ib = 4 * qc + n;
      int2 p = {0, 0};
      if (cb >= ib) p = *reinterpret_cast<const int2*>(kt + ((cb * (cb + 1) / 2 + ib) * 64 + l) * 4);
      cnt[m][n] = v4f{(float)(int16_t)(p.x & 0xffff), (float)(int16_t)(p.x >> 16), (float)(int16_t)(p.y & 0xffff),
                      (float)(int16_t)(p.y >> 16)};
    }
  sys_diag_epilogue_inl(a, cnt, s, J, qr, qc, l);
}

// k_sys_tiles_st chunks: k_sys_diag_counts with the per-individual scalars formed here (the same
// stats_wg code as k_indiv_stats) instead of in a launch before the system tiles -- one launch less
// on the chain.  Workgroup (b, J < 2): stats_wg (workgroup J = 0 also stores scal), tile
// J's centring sums into LDS, then the epilogue from the LDS copies; the u / rhs rows are split
// between the two workgroups.
__global__ __launch_bounds__(64 * STW) void k_stats_diag_counts(CholArgs a, StatsFuse x) {
  static_assert(64 * STW == STATS_THREADS, "stats_wg runs on the workgroup's 256 threads");
  __shared__ StatsShared sh;
  __shared__ double u_sh[TILE];
  const int t = threadIdx.x, l = t & 63, w = t >> 6, qr = w >> 1, qc = w & 1;
  const int64_t b = blockIdx.x >> 1;
  const int J = (int)(blockIdx.x & 1);
  const bool tile = qr >= qc && J < a.NT;   // the upper quadrant is never read
  // the counts first: their loads overlap the scalars' reduction
  v4f cnt[4][4];
  const int16_t* kt = a.kd + (b * a.NT + J) * KD_TILE;   // kd_tile(a.NT, b, J), written out: this kernel's registers
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int cb = 4 * qr + m, ib = 4 * qc + n;
      int2 p = {0, 0};
      if (tile && cb >= ib) p = *reinterpret_cast<const int2*>(kt + ((cb * (cb + 1) / 2 + ib) * 64 + l) * 4);
      cnt[m][n] = v4f{(float)(int16_t)(p.x & 0xffff), (float)(int16_t)(p.x >> 16), (float)(int16_t)(p.y & 0xffff),
                      (float)(int16_t)(p.y >> 16)};
    }
  // u_a = s_a of tile J's rows (stats_wg's u values, gathered here before its reduction so that
  // these loads overlap it)
  if (t < TILE) {
    const int64_t o0 = a.off[b], k = a.off[b + 1] - o0;
    const int64_t pad = a.padfirst ? a.ns - k : 0;
    const int64_t r = (int64_t)J * TILE + t;
    const int32_t* csT = a.ft.csT[fold_of(a.ft, b)];
    u_sh[t] = (r < a.ns && sys_real(r, pad, k)) ? (double)csT[snp_col(a.idx[o0 + r - pad], a.P)] : 0.0;
  }
  // (stats_wg's barriers also publish u_sh)
  stats_wg(a.idx, a.off, a.ft, x.csA, x.n, x.nT, a.ytp, a.P, a.form, a.ns, a.padfirst, a.nt, x.branch, x.h2, x.h2v, b,
           J == 0 ? x.scal : nullptr, x.err, sh);
  if (tile) sys_diag_epilogue_src(a, cnt, b, J, qr, qc, l, sh.sc, u_sh);
  // then the u / rhs rows, split between the individual's two workgroups (their stores overlap the
  // epilogue's)
  const int64_t half = (a.ns / 2 + 63) & ~(int64_t)63;
  stats_rows(a.idx, a.off, a.ft, a.P, a.ns, a.padfirst, a.nt, b, x.u, x.rhs, sh, J == 0 ? 0 : half,
             J == 0 ? half : a.ns);
}

int64_t sys_tiles_grid(const CholLaunch& c) {
  const int64_t ntri = (int64_t)c.sd.NT * (c.sd.NT + 1) / 2;
  const int64_t NS = (c.sd.NT + 1) / 2, units = c.B * (NS * (NS + 1) / 2);
  const int64_t cus = cu_count();
  const bool st = c.sys_st > 0 || (c.sys_st < 0 && units >= SYS_ST_MIN * cus);
  const int64_t grid = std::min(units, cus);
  const int64_t nsu = NS * (NS + 1) / 2, per = (units + grid - 1) / grid;
  if (!st || c.sd.ns > SP_ROWTAB || per / nsu + 2 > SP_MAXIND) return -(c.B * ntri);
  return grid;
}

// after a launch that stored the diagonal tiles' counts: K_JJ + lambda I of the tiles J < 2, and with
// c.stats the scalars (neither is traced)
static hipError_t launch_diag_counts(const CholLaunch& c, CholArgs a, hipStream_t s) {
  if (hipError_t e = hipGetLastError()) return e;
  a.wgt = nullptr;
  if (c.stats)
    hipLaunchKernelGGL(k_stats_diag_counts, dim3((unsigned)(c.B * 2)), dim3(64 * STW), 0, s, a, *c.stats);
  else
    hipLaunchKernelGGL(k_sys_diag_counts, dim3((unsigned)(c.B * 2)), dim3(64 * STW), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sys_tiles(const CholLaunch& c, hipStream_t s) {
  const CholArgs a = make_args(c, 0);
  const bool primal = c.sd.form == FORM_PRIMAL;
  const int64_t grid = sys_tiles_grid(c);
  if (grid > 0) {
    const int NS = (c.sd.NT + 1) / 2, nsu = NS * (NS + 1) / 2;
    hipLaunchKernelGGL(primal ? k_sys_tiles_st<false> : k_sys_tiles_st<true>, dim3((unsigned)grid), dim3(64 * SPW), 0, s,
                       a, c.kc, nsu, (int)(c.B * nsu));
    return launch_diag_counts(c, a, s);
  }
  if (c.stats) return hipErrorInvalidValue;   // the per-tile kernel reads the scalars
  const int ntri = c.sd.NT * (c.sd.NT + 1) / 2;
  hipLaunchKernelGGL(primal ? k_sys_tiles<false> : k_sys_tiles<true>, dim3((unsigned)(c.B * ntri)), dim3(64 * STW), 0, s,
                     a, c.kc, ntri);
  return hipGetLastError();
}

hipError_t launch_sys_tiles_folds(const CholLaunch& c, hipStream_t s) {
  const CholArgs a = make_args(c, 0);
  const int ntri = c.sd.NT * (c.sd.NT + 1) / 2;
  hipLaunchKernelGGL(k_sys_tiles_folds, dim3((unsigned)(c.ft.bpf * ntri)), dim3(64 * STW), 0, s, a, c.kc, ntri);
  return launch_diag_counts(c, a, s);   // k_sys_tiles_folds reads no scalar either
}

}  // namespace tblup
