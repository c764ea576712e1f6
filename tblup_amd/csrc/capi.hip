// C ABI of libtblup_gpu.so (see include/tblup_gpu.h): context, splits, workspace,
// batched evaluation pipeline and per-kernel-class event timing.
//
// Pipeline per chunk of B individuals (run_chunk: one HIP stream, no host syncs inside):
//   k_indiv_stats -> k_gather -> k_grm -> for J: (k_chol_diag, k_chol_offdiag) -> k_solve
// The host entries' driver (capi_ctx.h) and tblup_eval_batch are here; the entries that read the factor the
// pipeline leaves are in capi_model.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "capi_ctx.h"
#include "mt_jump.h"

using namespace tblup;

namespace tblup_capi {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

void clear_error() { g_err.clear(); }

int dev_alloc(tblup_ctx* c, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return 0;
  if (b.p) c->mem_in_use -= (int64_t)b.bytes;
  b.release();
  if (bytes == 0) return 0;
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    return fail(TBLUP_ERR_OOM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  }
  b.bytes = bytes;
  c->mem_in_use += (int64_t)bytes;
  return 0;
}

void dev_free(tblup_ctx* c, DevBuf& b) {
  if (b.p) c->mem_in_use -= (int64_t)b.bytes;
  b.release();
}

void Split::release(tblup_ctx* c) {
  for (DevBuf* b : {&gpk, &colsumT, &xty, &yT, &yV, &ymu}) dev_free(c, *b);
}

int check_ctx(tblup_ctx* c) {
  if (!c) return fail(TBLUP_ERR_ARG, "null context");
  return 0;
}

int ws_check(const tblup_ctx* c, const Carve& cv) {
  if (cv.base >= (char*)c->ws.p && cv.base + cv.used <= (char*)c->ws.p + c->ws.bytes) return 0;
  return fail(TBLUP_ERR_STATE, "internal error: workspace carve of " + std::to_string(cv.used) +
                                   " bytes overruns the " + std::to_string(c->ws.bytes) + "-byte workspace");
}

int check_indices(const tblup_ctx* c, const int64_t* idx, int64_t count) {
  for (int64_t i = 0; i < count; ++i)
    if (idx[i] < -c->P || idx[i] >= c->P)
      return fail(TBLUP_ERR_INDEX, "index " + std::to_string(idx[i]) + " is out of bounds for axis 1 with size " +
                                       std::to_string(c->P));
  return 0;
}

int check_counts(const int64_t* offsets, int64_t batch, const char* who) {
  for (int64_t b = 0; b < batch; ++b)
    if (offsets[b + 1] - offsets[b] < 1) return fail(TBLUP_ERR_ARG, std::string("every ") + who + " needs k >= 1 indices");
  return 0;
}

int for_each_chunk(tblup_ctx* c, const int64_t* offsets, int64_t batch, int64_t max_B, const ChunkBytes& bytes,
                   const std::function<int(const Chunk&)>& body) {
  std::vector<int64_t> hoff;
  int64_t b0 = 0;
  while (b0 < batch) {
    // grow the chunk while it fits the workspace budget and one launch's grid
    int64_t b1 = b0, sum_k = 0;
    hoff.assign(1, 0);
    while (b1 < batch) {
      const int64_t k = offsets[b1 + 1] - offsets[b1];
      hoff.push_back(sum_k + k);
      if (b1 > b0 && (bytes(hoff.data(), b1 + 1 - b0, sum_k + k) > c->budget || b1 + 1 - b0 > max_B)) {
        hoff.pop_back();
        break;
      }
      sum_k += k;
      ++b1;
    }
    const int64_t B = b1 - b0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int rc = dev_alloc(c, c->ws, bytes(hoff.data(), B, sum_k))) return rc;
    if (int rc = body(Chunk{b0, B, sum_k, hoff.data()})) return rc;
    b0 = b1;
  }
  return 0;
}

int upload_chunk(tblup_ctx* c, const int64_t* idx, const int64_t* offsets, const Chunk& ck, int64_t* d_idx,
                 int64_t* d_off) {
  HIPCHK(hipMemcpyAsync(d_idx, idx + offsets[ck.b0], (size_t)ck.sum_k * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_off, ck.hoff, (size_t)(ck.B + 1) * 8, hipMemcpyHostToDevice, c->stream));
  return 0;
}

}  // namespace tblup_capi

using namespace tblup_capi;

namespace {

hipEvent_t get_event(tblup_ctx* c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

int drain_events(tblup_ctx* c) {
  for (auto& p : c->pending) {
    HIPCHK(hipEventSynchronize(p.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
    c->ms[p.cls] += ms;
    c->event_pool.push_back(p.a);
    c->event_pool.push_back(p.b);
  }
  c->pending.clear();
  return 0;
}

// Launch wrapper: records an event pair around the launch when profiling.
template <typename F>
int timed(tblup_ctx* c, hipStream_t s, int cls, double flops, double bytes, F&& launch) {
  hipEvent_t a = nullptr, b = nullptr;
  if (c->profiling) {
    a = get_event(c);
    b = get_event(c);
    if (a) (void)hipEventRecord(a, s);
  }
  hipError_t e = launch();
  if (e != hipSuccess) return fail(TBLUP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  if (c->profiling && a && b) {
    (void)hipEventRecord(b, s);
    c->pending.push_back({cls, a, b});
    c->launches[cls] += 1;
    c->flops[cls] += flops;
    c->bytes[cls] += bytes;
  }
  return 0;
}

// TBLUP_DBG_SKIP (phase ablation, results wrong when set): honoured by diagnostic builds only
// (tools/ab_build_defs.sh 'diag=-DTBLUP_DIAG_BUILD'); the production library ignores it
inline int dbg_skip(const tblup_ctx* c) {
#ifdef TBLUP_DIAG_BUILD
  return c->dbg_skip;
#else
  (void)c;
  return 0;
#endif
}

// The batched system-tile launch (k_sys_tiles) builds every exact tile up front; int16 counts stay
// exact while the contraction -- n_T animals (SNP form), k SNPs (kernel form: every k <= 64 cblk) --
// is <= KC_MAX_NT (beyond it, and for one-tile systems, the in-tile int8 products of the
// off-diagonal kernel).  Kernel form: TBLUP_DUAL_ST=0 keeps the in-tile products (A/B timing).
bool sys_tiles(const tblup_ctx* c, const EvalDims& d, const SysDims& sd) {
  if (sd.NT < 2) return false;
  if (sd.form == FORM_PRIMAL) return d.nT <= KC_MAX_NT;
  return c->dual_st && sd.cblk * KBLK <= KC_MAX_NT;
}

}  // namespace

// Makespan of greedy list scheduling, in order, of classes {duration, count} on `slots` identical
// slots (slot free times kept as {time: free slots} groups).
static double list_makespan(std::initializer_list<std::pair<double, int64_t>> classes, int64_t slots) {
  std::map<double, int64_t> fr{{0.0, slots}};
  double end = 0.0;
  for (const auto& cl : classes) {
    int64_t n = cl.second;
    while (n > 0) {
      auto it = fr.begin();
      const double t = it->first;
      const int64_t use = std::min(n, it->second);
      if ((it->second -= use) == 0) fr.erase(it);
      fr[t + cl.first] += use;
      end = std::max(end, t + cl.first);
      n -= use;
    }
  }
  return end;
}

OffPlan tblup::off_plan(int64_t B, int NT, int J, bool st, int ahead, int nrs_pol, int64_t slots, int diag_d,
                        int dd_maxj, int diag_e, int64_t ncu) {
  OffPlan p{};
  p.nI = NT - J - 1;
  if (p.nI <= 0) {
    p.nI = 0;
    return p;
  }
  // launch j computes the partial sums of column j + 1's tiles; auto: when the launch's P-units
  // (B x (NT - 2 - j)) fit in AHEAD_SLOTS workgroup slots, i.e. run beside its T-units in one wave
  auto ahead_at = [&](int j) {
    const bool on = ahead == 1 || (ahead < 0 && B * (NT - 2 - j) < slots);
    return on && j >= 1 && j + 2 <= NT - 1;
  };
  p.nP = ahead_at(J) ? NT - 2 - J : 0;
  p.ahead_cur = (J >= 2 && ahead_at(J - 1)) ? 1 : 0;
  int dt = (J >= 1 && J + 1 < NT) ? 1 : 0;   // diagonal target J + 1 (its partial over L < J)
  // small batches: the D-units in the diagonal launch J (its B workgroups leave 256 - B CUs idle
  // for ~45 us; a D-unit alone on a CU sums J / 2 SYRK terms, so J <= DD_MAX_J keeps it shorter)
  if (dt && (diag_d == 1 || (diag_d < 0 && B > DD_MIN_B && B <= DD_MAX_B && J <= dd_maxj))) {
    p.ndd = 1;
    dt = 0;
  }
  // E-units: column J's GEMM1 term L = Ls0 of its first tiles, on the CUs the diagonal launch J
  // leaves idle (its B diagonal workgroups and D-units take one CU each: 144 KiB of LDS).  One term
  // (29 us alone on a CU, measured) ends inside the ~45 us diagonal launch.  Auto: one per idle CU.
  // The off-diagonal launch dispatches the tiles they started last, so that (the dispatcher filling
  // every CU's first slot, then its second) a CU pairs a whole tile with a shortened one or with a
  // lighter unit class -- an off-diagonal launch of one round lasts as long as its busiest CU.  (In
  // the tiles' plain order, columns covered only in part gained nothing: A/B, profiles/r05_epol_ab.txt,
  // r05_eord_ab.txt -- with the order pop 96 +1.9%, 160 +0.3%, 128 +0.2%.)  2: only whole columns.
  if (J >= 1 && (diag_e == 1 || (diag_e != 0 && ncu > 0))) {
    const int64_t idle = std::max<int64_t>(0, ncu - B * (1 + p.ndd));
    p.ne = diag_e == 1 ? B * p.nI : std::min<int64_t>(B * p.nI, idle);
    if (diag_e == 2 && p.ne < B * p.nI) p.ne = 0;
  }
  p.nrs = 1;
  p.nds = dt;
  // Row slices of the P-units (they need k_sys_tiles' counts: the int8 K is a whole-tile
  // product) and block slices of the D-unit: the pair whose greedy list schedule -- grid order
  // P, D, T on 512 slots (two workgroups per CU), unit work in 2*128^3-flop GEMM units plus a
  // fixed 0.25 -- ends first (ties: fewer units).  T-unit: the GEMM1 terms it still sums (1 after
  // an ahead launch, else J) + 0.5 (GEMM2); P-unit: J / nrs; D-unit: J / 2 / nds.
  // A slicing other than (1, 1) must gain 10%: the model ignores that tiles sharing a CU with
  // tiles (not with the lighter D-units) slow each other down (round 2: D split in two at pop 256
  // measured slower although such a model predicted -90 us).
  const double jt = J, tw = (p.ahead_cur ? 1.0 : jt) + 0.5, c0 = 0.25;
  const int64_t nT = B * p.nI;
  auto span = [&](int nrs, int nds) {
    return list_makespan({{c0 + jt / nrs, B * p.nP * nrs}, {c0 + 0.5 * jt / nds, B * dt * nds}, {c0 + tw, nT}}, 512);
  };
  const bool slice_p = p.nP > 0 && st;
  double best = (nrs_pol > 1 && slice_p) ? 1e300 : 0.9 * span(1, 1);
  for (int nrs : {1, 2, 4}) {
    if (nrs > 1 && !slice_p) break;
    if (nrs_pol > 0 && nrs != nrs_pol && slice_p) continue;
    for (int nds = 1; nds <= (dt ? 2 : 1); ++nds) {
      if (nrs == 1 && nds == 1) continue;
      const double ms = span(nrs, nds);
      if (ms < best) {
        best = ms;
        p.nrs = slice_p ? nrs : 1;
        p.nds = dt * nds;
      }
    }
  }
  p.n_kd = (J == 0 && NT > 2 && !st) ? B * (NT - 2) : 0;
  return p;
}

namespace {

OffPlan plan_of(const tblup_ctx* c, int64_t B, int NT, int J, bool st) {
  return off_plan(B, NT, J, st, c->ahead, c->nrs, AHEAD_SLOTS, c->diag_d, DD_MAX_J, c->diag_e, cu_count());
}

// the chunk's launches hand partial sums of off-diagonal tiles on (P-units or E-units)
bool uses_part(const tblup_ctx* c, int64_t B, int NT, bool st) {
  for (int J = 0; J < NT; ++J) {
    const OffPlan p = plan_of(c, B, NT, J, st);
    if (p.nP > 0 || p.ne > 0) return true;
  }
  return false;
}

// SNP-form solve: the chained kernel up to CHAIN_MAX_B individuals (measured at config 2: solve
// 0.175 -> 0.071 ms at B = 32, 0.184 -> 0.092 at 64, 0.199 -> 0.151 at 128 (round 4's block-row
// units; round 3's tile units: 0.078 / 0.102 / 0.162), even at 192 (round 3), 0.238 -> 0.274 at
// 256, where one workgroup per individual already streams L near the HBM rate).  Round 5's pull
// units (one trait; profiles/r05_solve_pull_ab.txt): 0.061 -> 0.049 ms at 32, 0.079 -> 0.068 at 64,
// 0.128 -> 0.125 at 128, even at 160, 0.188 (k_solve) -> 0.180 at 192, even at 256 -- bound 192
constexpr int64_t CHAIN_MAX_B = 160;
constexpr int64_t CHAIN_PULL_MAX_B = 192;
bool use_chain(const tblup_ctx* c, const SysDims& sd, int64_t B, int64_t nt) {
  const bool pull = c->solve_pull == 1 || (c->solve_pull < 0 && nt == 1);
  return sd.form == FORM_PRIMAL &&
         (c->solve_chain == 1 || (c->solve_chain < 0 && B <= (pull ? CHAIN_PULL_MAX_B : CHAIN_MAX_B)));
}

// Last-term mode: the diagonal tile's last SYRK term computed by the previous launch's tile
// (J, J-1) workgroup (dispatched first) instead of inside the diagonal launch, where one
// workgroup per individual runs it on one CU.  Bit-identical either way.  Measured (config 2,
// A/B): the diagonal launches lose ~8 us each at every B (0.349 -> 0.282 ms per step at B = 32,
// 0.394 -> 0.331 at 256) but the off-diagonal launches gain 42 (B = 32) to 97 us (256): +3.3% at
// 32, +2.0% at 64, -1.3% at 128, -1% at 192 and 256.
// Per diagonal launch (bit J: diagonal J takes its last term from launch J-1), round 5: at
// 64 < B <= 160 only diagonal launches 1 and 3 -- the workgroup traces of round 4 (pop 128,
// profiles/r04_wg_trace_pop128_auto.txt / _lastterm.txt) give, per launch, the off-diagonal launch's
// extra time against the next diagonal launch's saving: J = 0: -1.1 / -9.1 us, J = 2: +0.5 / -5.6;
// every other launch loses.  Late in round 5 (pull-unit solve, non-temporal stores; traces
// profiles/r05i_wg_trace_pop128.txt: tiles (7, 6) and (6, 5) done 20 / 40 us before their launches
// end) diagonal launches 6 and 7 too up to 128: pop 128 +0.8%, 96 +1.5%, 112 even, 160 -0.2%
// (profiles/r05_lt_mask4_ab.txt).
constexpr int64_t LT_MAX_B = 64;
constexpr int64_t LT_LATE_MAX_B = 128;
constexpr int64_t LT_PART_MAX_B = 160;
uint32_t last_term_mask(const tblup_ctx* c, const SysDims& sd, int64_t B) {
  if (sd.NT < 2 || c->last_term == 0) return 0;
  if (c->lt_mask >= 0) return (uint32_t)c->lt_mask;
  if (c->last_term == 1 || B <= LT_MAX_B) return ~1u;   // every diagonal launch J >= 1
  if (B <= LT_LATE_MAX_B) return (1u << 1) | (1u << 3) | (1u << 6) | (1u << 7);
  return B <= LT_PART_MAX_B ? (1u << 1) | (1u << 3) : 0u;
}
bool use_last_term(const tblup_ctx* c, const SysDims& sd, int64_t B) { return last_term_mask(c, sd, B) != 0; }
// bit J of a last-term mask; a kernel-form system can have NT > 32 tile columns (n_T > 4096), and
// there the all-launches mask (~1u, J >= 1) keeps its meaning while a sparse mask names none
inline bool lt_bit(uint32_t m, int J) { return J < 32 ? ((m >> J) & 1u) != 0 : m == ~1u; }

EvalDims dims_of(const tblup_ctx* c, const Split& sp) {
  EvalDims d;
  d.n = c->n;
  d.P = c->P;
  d.nT = sp.nT;
  d.nV = sp.nV;
  d.nTp = sp.nTp;
  d.nVp = sp.nVp;
  d.nRp = sp.nRp;
  d.NT = (int)(sp.nTp / TILE);
  d.NR = (int)(sp.nRp / TILE);
  d.nt = c->nt;
  return d;
}

// Form of the per-individual system for a batch.  The SNP-space (primal) form is what
// sklearn's Ridge solves when k <= n_T (_ridge.py _solve_cholesky: X^T X + alpha I); it is
// used when every individual takes the snp branch and it gives no more 128-row tiles than the
// kernel form.  pref: 0 auto, 1 force dual, 2 force primal (snp batches only).
SysDims choose_sys(const tblup_ctx* c, const EvalDims& d, const int64_t* h_off, int64_t B, int branch, int pref) {
  int64_t max_k = 1;
  bool all_snp = true;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t k = h_off[b + 1] - h_off[b];
    max_k = std::max(max_k, k);
    if (branch_of(c, k, branch) != 2) all_snp = false;
  }
  const int64_t kp = round_up(max_k, TILE);
  // equal tile counts (kp == nTp, e.g. k = 1000 against a 1024-animal CV fold) also take the SNP
  // form: its system tiles come from k_sys_tiles' FP4 counts instead of the in-tile int8 products
  const bool primal = all_snp && pref != 1 && (pref == 2 || kp <= d.nTp);
  SysDims sd;
  if (primal) {
    sd.form = FORM_PRIMAL;
    sd.pad_first = c->pad_first;
    sd.ns = kp;
    sd.prow = kp;
    sd.cblk = d.nRp / KBLK;
  } else {
    sd.form = FORM_DUAL;
    sd.ns = d.nTp;
    sd.prow = d.nRp;
    sd.cblk = round_up(max_k, KBLK) / KBLK;
  }
  sd.NT = (int)(sd.ns / TILE);
  return sd;
}

void set_fold(FoldTab& ft, int64_t f, const Split& sp) {
  ft.gpk[f] = (const uint8_t*)sp.gpk.p;
  ft.csT[f] = (const int32_t*)sp.colsumT.p;
  ft.xty[f] = (const double*)sp.xty.p;
  ft.yV[f] = (const double*)sp.yV.p;
  ft.yT[f] = (const double*)sp.yT.p;
  ft.ymu[f] = (const double*)sp.ymu.p;
}

FoldTab single_fold(const Split& sp, int64_t B) {
  FoldTab ft{};
  ft.bpf = std::max<int64_t>(B, 1);
  ft.nf = 1;
  set_fold(ft, 0, sp);
  return ft;
}

// Host entries, after the chunk's stream synchronisation: whether one of the chained solves `seqs`
// (0: none) gave up a wait.  Its ring slot holds seq exactly then (slots of other calls hold their own seqs).
int chain_expired(tblup_ctx* c, const std::vector<int32_t>& seqs, bool* out) {
  *out = false;
  for (int32_t seq : seqs) {
    if (seq <= 0 || !c->chain.p) continue;
    const int32_t* ring = (const int32_t*)c->chain.p + (c->chain.bytes / 4 - CHAIN_ERR_RING - 1);
    int32_t v = 0;
    HIPCHK(hipMemcpyAsync(&v, ring + seq % CHAIN_ERR_RING, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = *out || v == seq;
  }
  return 0;
}

// What a host entry carves first: the chunk's index list and offsets, n_fit fitnesses, n_ebv EBVs (0: none)
struct HeadBufs {
  int64_t *idx, *off;
  double *fit, *ebv;
  static HeadBufs carve(Carve& cv, int64_t B, int64_t sum_k, int64_t n_fit, int64_t n_ebv) {
    return {cv.take<int64_t>((size_t)sum_k), cv.take<int64_t>((size_t)B + 1), cv.take<double>((size_t)n_fit),
            n_ebv ? cv.take<double>((size_t)n_ebv) : nullptr};
  }
};

// The pipeline's buffers of a chunk of B systems.  A new one is one line of this carve: run_chunk lays the
// chunk out with it and every entry measures its workspace with it.
struct PipeBufs {
  bool use_st, chain;   // system tiles from k_sys_tiles; the mode runs the chained solve
  uint8_t* panel;
  double *u, *scal, *L, *Dinv, *z, *w, *rhs, *Sp, *Kdg;
  int16_t *kdb, *kcb;
  double *Pp, *Qb, *K, *beta, *cpart, *epart, *mbpart;
  // gsh: a kernel-form fold chunk that reads its counts from the shared A_R A_R^T instead of system tiles
  static PipeBufs carve(Carve& cv, const tblup_ctx* c, const EvalDims& d, const SysDims& sd, int64_t B, ChunkMode mode,
                        bool gsh) {
    PipeBufs p{};
    const size_t nB = (size_t)B, vec = nB * d.nt * sd.ns, dg = nB * sd.NT * NPACK * BLKD;
    p.use_st = sys_tiles(c, d, sd) && mode != ChunkMode::DebugK && !gsh;
    p.chain = mode == ChunkMode::Full && use_chain(c, sd, B, d.nt);
    p.panel = cv.take<uint8_t>(sd.form == FORM_DUAL ? nB * sd.prow * dual_pk_row(sd) : 0);   // packed (kernel form)
    p.u = cv.take<double>(nB * sd.prow); p.scal = cv.take<double>(nB * SCAL);
    p.L = cv.take<double>(nB * l_stride(sd.NT));   // Lt tiles
    p.Dinv = cv.take<double>(dg);                  // packed X
    p.z = cv.take<double>(vec); p.w = cv.take<double>(vec); p.rhs = cv.take<double>(vec);
    p.Sp = cv.take<double>(nB * TBLUP_NSLOT * 36 * 256);   // next diagonal tile (minus its last SYRK term)
    // diagonal system tiles: fp64 K_JJ + lambda I (with k_sys_tiles: J < 2 only, the diagonal kernel's direct
    // reads) and, with k_sys_tiles, the exact int16 counts of J >= 2 (the D-units') and of the off-diagonal tiles
    p.Kdg = cv.take<double>(dg);
    if (p.use_st) p.kdb = cv.take<int16_t>(nB * sd.NT * KD_TILE);
    if (p.use_st) p.kcb = cv.take<int16_t>(nB * sd.NT * (sd.NT - 1) / 2 * KC_TILE);
    // the off-diagonal tiles' partial sums; the diagonal tiles' last SYRK terms
    if (uses_part(c, B, sd.NT, sys_tiles(c, d, sd))) p.Pp = cv.take<double>(2 * nB * sd.NT * TILE * TILE);
    if (use_last_term(c, sd, B)) p.Qb = cv.take<double>(nB * NPACK * BLKD);
    if (mode == ChunkMode::DebugK) p.K = cv.take<double>(nB * d.nRp * d.nTp);   // the full K_{R,T} block
    if (p.chain) {   // beta, c_{J->I}, EBV shares
      p.beta = cv.take<double>(vec); p.cpart = cv.take<double>(nB * sd.NT * sd.NT * d.nt * TILE);
      p.epart = cv.take<double>(nB * sd.NT * d.nt * d.nV); p.mbpart = cv.take<double>(nB * sd.NT * d.nt);
    }
    return p;
  }
};

// The chained solve's launch arguments: the context's flags (grown and zeroed when too small: a host
// synchronisation), the next seq and its ring slot, the chunk's buffers, the debug knob's shots
int chain_args(tblup_ctx* c, const ChunkReq& rq, const PipeBufs& pb, SolveChain& ch) {
  const size_t fbytes = ((size_t)rq.B * chain_flags(rq.sd.NT) + CHAIN_ERR_RING + 1) * 4;
  if (c->chain.bytes < fbytes || c->chain_seq >= INT32_MAX - 1) {
    HIPCHK(hipStreamSynchronize(rq.s));   // the flags may still be read by an earlier chained solve
    if (int rc = dev_alloc(c, c->chain, fbytes)) return rc;
    HIPCHK(hipMemsetAsync(c->chain.p, 0, c->chain.bytes, rq.s));
    c->chain_seq = 0;
  }
  ch.flags = (int32_t*)c->chain.p;
  int32_t* ring = ch.flags + (c->chain.bytes / 4 - CHAIN_ERR_RING - 1);
  ch.beta = pb.beta; ch.cpart = pb.cpart; ch.epart = pb.epart; ch.mbpart = pb.mbpart;
  ch.seq = ++c->chain_seq;
  ch.err = ring + ch.seq % CHAIN_ERR_RING;
  // host entries recover from their ring slot (chain_expired); device entries raise the status word
  ch.expired = c->host_entry ? ring + CHAIN_ERR_RING : (int32_t*)c->status.p + ST_SOLVE;
  ch.mode = c->chain_sync;
  // pull units for one trait (several traits: their registers spill at two units per CU)
  ch.pull = c->solve_pull == 1 || (c->solve_pull < 0 && rq.d.nt == 1);
  ch.spin_max = CHAIN_SPIN_MAX;
  if (c->chain_dbg_shots > 0) {
    --c->chain_dbg_shots;
    ch.spin_max = c->chain_dbg_spin;
    ch.delay = c->chain_dbg_delay;
  }
  return 0;
}

}  // namespace

// Enqueue the pipeline for one chunk (no host synchronisation unless the chain flags must grow).
int tblup_capi::run_chunk(tblup_ctx* c, const ChunkReq& rq, Carve& cv, ChunkRes& res) {
  const EvalDims& d = rq.d;
  const SysDims& sd = rq.sd;
  const hipStream_t s = rq.s;
  const int64_t *d_idx = rq.d_idx, *d_off = rq.d_off, *h_off = rq.h_off, B = rq.B;
  res = ChunkRes{};
  CholLaunch& cl = res.cl;
  cl.ft = rq.ft ? *rq.ft : single_fold(*rq.sp, B);
  const FoldTab& ft = cl.ft;
  const bool redo = rq.mode == ChunkMode::SolveOnly;
  const PipeBufs pb = PipeBufs::carve(cv, c, d, sd, B, rq.mode, ft.gsh != nullptr);
  if (int rc = ws_check(c, cv)) return rc;
  const bool use_st = pb.use_st;
  double grm_flops = 0.0, gather_bytes = 0.0, stats_bytes = 0.0;
  const double tri = (double)d.nT * (d.nT + 1) / 2.0 + (double)d.nV * d.nT;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t k = h_off[b + 1] - h_off[b];
    grm_flops += 2.0 * (double)k * tri;
    gather_bytes += 0.5 * (double)k * (double)(d.nT + d.nV);   // 2-bit split rows in, 2-bit rows out
    stats_bytes += 16.0 * (double)k;
  }
  const int64_t pk_row = (sd.form == FORM_DUAL) ? dual_pk_row(sd) : 0;
  const int64_t pstride = sd.prow * pk_row;
  double *const u = pb.u, *const scal = pb.scal, *const rhs = pb.rhs, *const Qb = pb.Qb;
  const bool fold_share = use_st && sd.form == FORM_PRIMAL && ft.nf > 1 && ft.share;   // k_sys_tiles_folds
  // the launches' arguments, by name (cl.ft above; wgt, q and stats change from launch to launch)
  cl.d = d; cl.sd = sd; cl.B = B; cl.off = rq.d_off; cl.idx = rq.d_idx;
  cl.L = pb.L; cl.Dinv = pb.Dinv; cl.z = pb.z; cl.w = pb.w; cl.rhs = rhs; cl.S = pb.Sp; cl.u = u; cl.scal = scal;
  cl.Kd = pb.Kdg; cl.kd = pb.kdb; cl.kc = pb.kcb; cl.part = pb.Pp; cl.q = Qb;
  cl.yT = (const double*)rq.sp->yT.p; cl.panel = pb.panel; cl.pstride = pstride; cl.gs_row = d.nRp; cl.gpk_row = d.nRp / 4;
  cl.skip = dbg_skip(c) | (rq.mode == ChunkMode::DebugL ? FLAG_WRITE_LJJ : 0);
  cl.padskip = (sd.form == FORM_PRIMAL && sd.pad_first) ? 1 : 0;
  cl.sys_st = c->sys_st;
  cl.diag_waves = c->diag_waves;
  std::vector<OffPlan> plan(sd.NT);
  for (int J = 0; J < sd.NT; ++J) {
    plan[J] = plan_of(c, B, sd.NT, J, use_st);
    if (ft.gsh) plan[J].ne = 0;   // the diagonal kernel's E-units do not read shared fold counts
  }
  const int32_t* csA = (const int32_t*)c->colsum_all.p;
  // the scalars formed after k_sys_tiles_st / k_sys_tiles_folds, in their K_JJ epilogue launch (one
  // launch less; neither reads a scalar), else by k_indiv_stats first
  const bool fuse_stats = !redo && use_st && sd.form == FORM_PRIMAL && (fold_share || sys_tiles_grid(cl) > 0);
  const StatsFuse sf{csA, d.n, d.nT, rq.branch, rq.h2, rq.d_h2, (int32_t*)c->status.p + ST_INDEX, scal, u, rhs};
  int rc = 0;
  if (!redo && !fuse_stats)
    rc = timed(c, s, KC_STATS, 2.0 * (double)h_off[B], stats_bytes, [&] {
      return launch_indiv_stats(d_idx, d_off, B, ft, csA, d, sd, rq.branch, rq.h2, rq.d_h2, scal, u, rhs,
                                (int32_t*)c->status.p + ST_INDEX, s);
    });
  if (rc) return rc;
  if (sd.form == FORM_DUAL && !redo) {
    // primal rows are read in place from the split matrix: no gather
    rc = timed(c, s, KC_GATHER, 0.0, gather_bytes, [&] {
      return launch_gather(ft, d_idx, d_off, pstride, B, csA, scal, d, pk_row, pb.panel, u, s);
    });
    if (rc) return rc;
  }
  res.z = pb.z;
  if (rq.mode == ChunkMode::DebugK) {
    // parity readback only: the full K_{R,T} block of the unified form (k_grm); the
    // production path never materialises K (the Cholesky kernels rebuild each tile)
    res.K = pb.K;
    const double kbytes = (double)B * ((double)d.nT * d.nT / 2.0 + (double)d.nV * d.nT) * 8.0;
    return timed(c, s, KC_GRM, grm_flops, kbytes + gather_bytes / 2.0,
                 [&] { return launch_grm(pb.panel, pstride, pk_row, d_off, u, scal, d, B, pb.K, s); });
  }
  res.K = pb.L;
  const double T3 = (double)TILE * TILE * TILE;
  // profiling only: room for one record per Cholesky workgroup of this chunk
  uint64_t* wgt = nullptr;
  if (c->wg_trace && !redo) {
    int64_t nwg = 0;
    for (int J = 0; J < sd.NT; ++J) nwg += B * (1 + plan[J].ndd) + plan[J].ne + DTR_RECS + offdiag_grid(plan[J], B);
    if (use_st) nwg += B * sd.NT * (sd.NT + 1) / 2;
    if (pb.chain) nwg += B * sd.NT;   // chained solve units
    if (int rc = dev_alloc(c, c->wgt, (size_t)nwg * WGT_REC * 8)) return rc;
    HIPCHK(hipMemsetAsync(c->wgt.p, 0, (size_t)nwg * WGT_REC * 8, s));
    wgt = (uint64_t*)c->wgt.p;
    c->wgt_used = 0;
  }
  auto trace = [&](int64_t n) {   // the next launch writes its n records behind those so far
    cl.wgt = wgt + c->wgt_used * WGT_REC;
    c->wgt_used += n;
  };
  const double kbar = B > 0 ? (double)h_off[B] / (double)B : 0.0;
  const double cbar = (sd.form == FORM_PRIMAL) ? (double)d.nT : kbar;   // contraction length
  if (!redo && use_st) {
    // every system tile (I >= J) in one int8 launch: int ops 2 x 128^2 x n_T per tile
    const double ntri = (double)sd.NT * (sd.NT + 1) / 2.0;
    const double fg = (double)B * ntri * 2.0 * 128.0 * 128.0 * cbar;
    const double nd8 = std::min(sd.NT, 2);   // diagonal tiles stored as fp64 (the rest as int16 counts)
    const double bg = (double)B * ((ntri - sd.NT) * KC_TILE * 2.0 + (sd.NT - nd8) * KD_TILE * 2.0 + nd8 * KD_TILE * 8.0);
    if (wgt) trace(fold_share ? B * sd.NT * (sd.NT + 1) / 2 : std::abs(sys_tiles_grid(cl)));
    cl.stats = fuse_stats ? &sf : nullptr;
    rc = timed(c, s, KC_GRM, fg, bg + (fuse_stats ? stats_bytes : 0.0), [&] {
      return fold_share ? launch_sys_tiles_folds(cl, s) : launch_sys_tiles(cl, s);
    });
    cl.stats = nullptr;
    if (rc) return rc;
  } else if (!redo) {
    if (ft.gsh) {
      // kernel-form folds: every individual's A_R A_R^T once (int ops 2 x nRp^2 x k / 2 + the diagonal tiles)
      const double NR = (double)(d.nRp / TILE);
      const double fgs = (double)ft.bpf * NR * (NR + 1) / 2.0 * 2.0 * 128.0 * 128.0 * kbar;
      rc = timed(c, s, KC_GRM, fgs, (double)ft.bpf * d.nRp * d.nRp * 4.0, [&] { return launch_gshare(cl, s); });
      if (rc) return rc;
    }
    // int ops of the diagonal GRM tiles J < 2 (J >= 2 run inside the column-0 off-diagonal launch)
    const double nJ = (double)std::min(sd.NT, 2);
    const double fg = (double)B * nJ * 128.0 * 129.0 * cbar;
    rc = timed(c, s, KC_GRM, fg, (double)B * nJ * 36 * 256 * 8.0, [&] { return launch_diag_grm(cl, s); });
    if (rc) return rc;
  }
  // Column loop.  (A look-ahead schedule -- tile (J+1, J) and diagonal tile J+1 on a
  // high-priority stream beside the rest of column J -- measured slower on MI355X: the
  // chip is already full during the off-diagonal launches, and sharing CUs slows the
  // critical path more than it hides.)
  const double Bd = (double)B;
  const uint32_t ltm = last_term_mask(c, sd, B);
  for (int J = 0; !redo && J < sd.NT; ++J) {
    const double jt = (double)J;
    const OffPlan& p = plan[J];
    // algorithmic fp64 work: the L = J-1 SYRK term of the diagonal tile, potrf + trtri,
    // forward-substitution GEMV (the exact system tiles are counted under KC_GRM)
    const bool qd = Qb && lt_bit(ltm, J), qo = Qb && lt_bit(ltm, J + 1);
    const double lt_d = qd ? 0.0 : std::min(jt, 1.0);   // the last SYRK term's share of this launch
    // (+ the D-units when they run in this launch: 128^3 per L < J, as in the off-diagonal launch)
    // (+ the E-units: one 2*128^3 GEMM1 term each, moved out of launch J's T-units)
    const double fd = Bd * (T3 * lt_d + 2.0 * T3 / 3.0 + 2.0 * TILE * TILE * jt) + (p.ndd ? Bd * T3 * jt : 0.0) +
                      (double)p.ne * 2.0 * T3;
    const double bd = Bd * (TILE * TILE * lt_d * 8.0 + 2.0 * TILE * TILE * 8.0) +
                      (p.ndd ? 2.0 * Bd * TILE * TILE * jt * 8.0 : 0.0) + (double)p.ne * 3.0 * TILE * TILE * 8.0;
    if (wgt) trace(B * (1 + p.ndd) + p.ne + DTR_RECS);
    cl.q = qd ? Qb : nullptr;   // diagonal J: its last term from launch J-1
    rc = timed(c, s, KC_DIAG, fd, bd, [&] { return launch_chol_diag(cl, J, p, s); });
    cl.q = qo ? Qb : nullptr;   // off-diagonal J: the last term of diagonal J+1
    if (rc) return rc;
    if (p.nI > 0) {
      // T-units: GEMM1 over the L not summed ahead (2*128^3 each) + the triangular solve 128^3;
      // P-units: 2*128^3 per L < J; D-unit: 128^3 per L < J (lower half); the fused int8 GRM
      // tiles' int-ops are excluded
      const double lt = p.ahead_cur ? 1.0 : jt;
      const double fo = Bd * p.nI * (2.0 * T3 * lt + T3) + Bd * p.nP * 2.0 * T3 * jt + (p.nds ? Bd * T3 * jt : 0.0) +
                        (qo ? Bd * T3 : 0.0) - (double)p.ne * 2.0 * T3;
      const double bo = Bd * p.nI * (TILE * TILE * lt * 8.0 + TILE * TILE * 8.0) +
                        Bd * p.nP * (2.0 * TILE * TILE * jt * 8.0 + TILE * TILE * 8.0) +
                        (p.nds ? 2.0 * Bd * TILE * TILE * jt * 8.0 : 0.0);
      if (wgt) trace(offdiag_grid(p, B));
      rc = timed(c, s, KC_OFFDIAG, fo, bo, [&] { return launch_chol_offdiag(cl, J, p, s); });
      if (rc) return rc;
    }
  }
  if (rq.mode == ChunkMode::DebugL) return 0;
  const double fs = (double)B * (2.0 * (double)sd.ns * sd.ns / 2.0 + 2.0 * kbar * (double)(d.nT + d.nV) + 10.0 * d.nV);
  const double bs = (double)B * (((double)sd.ns * sd.ns / 2.0 + (double)sd.NT * TILE * TILE) * 8.0 +
                                 kbar * (double)(d.nT + d.nV));
  SolveChain ch{};
  const SolveChain* chp = nullptr;
  if (pb.chain) {
    if (int rc2 = chain_args(c, rq, pb, ch)) return rc2;
    res.chain_seq = ch.seq;
    chp = &ch;
    if (wgt) trace(B * sd.NT);
  }
  return timed(c, s, KC_SOLVE, fs, bs, [&] { return launch_solve(cl, chp, rq.d_fit, rq.d_ebv, s); });
}

int tblup_capi::run_recovering(tblup_ctx* c, const std::function<int(bool, std::vector<int32_t>&)>& enqueue) {
  std::vector<int32_t> seqs;
  for (int pass = 0;; ++pass) {
    seqs.clear();
    if (int rc = enqueue(pass != 0, seqs)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    bool any = false;
    if (int rc = chain_expired(c, seqs, &any)) return rc;
    if (!any) return 0;
    ++c->chain_recoveries;
  }
}

namespace {

// Device entries: the workspace grown to `need` bytes.  Large enough already: no synchronisation (the
// entries are asynchronous); else it may still be in use by earlier work on either stream.
int ensure_ws(tblup_ctx* c, hipStream_t s, size_t need) {
  if (need <= c->ws.bytes) return 0;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipStreamSynchronize(c->stream));
  return dev_alloc(c, c->ws, need);
}

// Marks a synchronous entry for its duration: its chained solves write their expiry to the ring
// only (the entry re-runs the affected chunk's solve through k_solve and counts it), not to the
// context's sticky status word that the device entries' callers read.
struct HostEntry {
  tblup_ctx* c;
  explicit HostEntry(tblup_ctx* cc) : c(cc) { c->host_entry = true; }
  ~HostEntry() { c->host_entry = false; }
};

Split* find_split(tblup_ctx* c, int id) {
  auto it = c->splits.find(id);
  return it == c->splits.end() ? nullptr : it->second.get();
}

}  // namespace

extern "C" {

const char* tblup_last_error(void) { return tblup_capi::g_err.c_str(); }

const char* tblup_version(void) { return "tblup_gpu 0.1.0 (gfx950)"; }

int tblup_device_count(int* out) {
  if (!out) return fail(TBLUP_ERR_ARG, "null out");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *out = n;
  return 0;
}

int tblup_ctx_create(const int8_t* geno, int64_t n, int64_t P, int layout, const double* pheno, int device,
                     tblup_ctx** out) {
  g_err.clear();
  if (!out) return fail(TBLUP_ERR_ARG, "null out_ctx");
  *out = nullptr;
  const bool panel = geno || pheno || n || P;   // (NULL, 0, 0, NULL): DE / decode-only context
  if (panel && (!geno || !pheno || n < 2 || P < 1)) return fail(TBLUP_ERR_ARG, "bad genotype/phenotype arguments");
  if (layout != TBLUP_LAYOUT_ANIMAL_MAJOR && layout != TBLUP_LAYOUT_SNP_MAJOR) return fail(TBLUP_ERR_ARG, "bad layout");
  if (n > (int64_t)1 << 30) return fail(TBLUP_ERR_ARG, "too many animals");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(TBLUP_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(TBLUP_ERR_ARG, "device id out of range");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<tblup_ctx> c(new tblup_ctx());
  c->device = device;
  c->n = n;
  c->P = P;
  if (panel) c->pheno.assign(pheno, pheno + n);
  c->nt = 1;
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const char* env = getenv("TBLUP_WORKSPACE_MB");
  c->budget = (size_t)(env ? atoll(env) : 32768) << 20;
#ifdef TBLUP_DIAG_BUILD
  const char* dbg = getenv("TBLUP_DBG_SKIP");
  c->dbg_skip = dbg ? atoi(dbg) : 0;
#endif
  const char* wt = getenv("TBLUP_WG_TRACE");
  c->wg_trace = wt && atoi(wt) != 0;
  const char* fp = getenv("TBLUP_FORM");
  c->form_pref = fp ? std::max(0, std::min(2, atoi(fp))) : 0;
  if (const char* e = getenv("TBLUP_AHEAD")) c->ahead = std::max(-1, std::min(1, atoi(e)));
  if (const char* e = getenv("TBLUP_SOLVE_CHAIN")) c->solve_chain = std::max(-1, std::min(1, atoi(e)));
  if (const char* e = getenv("TBLUP_SOLVE_PULL")) c->solve_pull = std::max(-1, std::min(1, atoi(e)));
  if (const char* e = getenv("TBLUP_CHAIN_SYNC")) c->chain_sync = atoi(e);
  if (const char* e = getenv("TBLUP_LAST_TERM")) c->last_term = std::max(-1, std::min(1, atoi(e)));
  if (const char* e = getenv("TBLUP_LT_MASK")) c->lt_mask = (int)strtol(e, nullptr, 0);
  if (const char* e = getenv("TBLUP_FOLD_FUSE")) c->fold_fuse = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_FOLD_SHARE")) c->fold_share = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_SYS_ST")) c->sys_st = std::max(-1, std::min(1, atoi(e)));
  if (const char* e = getenv("TBLUP_FOLD_GSHARE")) c->fold_gshare = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_DUAL_ST")) c->dual_st = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_DIAG_D")) c->diag_d = std::max(-1, std::min(1, atoi(e)));
  if (const char* e = getenv("TBLUP_DIAG_E")) c->diag_e = std::max(-1, std::min(2, atoi(e)));
  if (const char* e = getenv("TBLUP_DIAG_WAVES")) c->diag_waves = (atoi(e) == 8 || atoi(e) == 12 || atoi(e) == 16) ? atoi(e) : 0;
  if (const char* e = getenv("TBLUP_PAD_FIRST")) c->pad_first = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_RELIAB_LDS")) c->reliab_lds = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_SCORE_LDS")) c->score_lds = atoi(e) != 0;
  if (const char* e = getenv("TBLUP_NRS")) c->nrs = (atoi(e) == 1 || atoi(e) == 2 || atoi(e) == 4) ? atoi(e) : 0;
  if (const char* e = getenv("TBLUP_CHAIN_DEBUG")) {
    int sp = 0, dl = 0, sh = 0;
    if (sscanf(e, "%d,%d,%d", &sp, &dl, &sh) == 3 && sp > 0 && dl >= 0 && sh > 0) {
      c->chain_dbg_spin = sp;
      c->chain_dbg_delay = dl;
      c->chain_dbg_shots = sh;
    }
  }
  if (!panel) {
    *out = c.release();
    return 0;
  }
  const size_t gbytes = (size_t)n * (size_t)P;
  if (int rc = dev_alloc(c.get(), c->geno_sm, gbytes)) return rc;
  if (int rc = dev_alloc(c.get(), c->colsum_all, (size_t)P * 4)) return rc;
  if (int rc = dev_alloc(c.get(), c->status, ST_WORDS * 4)) return rc;
  HIPCHK(hipMemsetAsync(c->status.p, 0, ST_WORDS * 4, c->stream));
  if (layout == TBLUP_LAYOUT_SNP_MAJOR) {
    HIPCHK(hipMemcpyAsync(c->geno_sm.p, geno, gbytes, hipMemcpyHostToDevice, c->stream));
  } else {
    if (int rc = dev_alloc(c.get(), c->scratch, gbytes)) return rc;
    HIPCHK(hipMemcpyAsync(c->scratch.p, geno, gbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_transpose_geno((const int8_t*)c->scratch.p, (int8_t*)c->geno_sm.p, n, P, c->stream));
  }
  HIPCHK(launch_colsum_all((const int8_t*)c->geno_sm.p, (int32_t*)c->colsum_all.p, n, P, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  dev_free(c.get(), c->scratch);
  *out = c.release();
  return 0;
}

int tblup_ctx_destroy(tblup_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& p : c->pending) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  for (auto e : c->event_pool) (void)hipEventDestroy(e);
  for (auto& kv : c->splits) kv.second->release(c);
  for (DevBuf* b : {&c->geno_sm, &c->colsum_all, &c->status, &c->scratch, &c->ws, &c->wgt, &c->chain, &c->dec_keys,
                    &c->dec_idx, &c->de_polys, &c->de_small, &c->de_par, &c->de_chi, &c->mde_dev})
    b->release();
  if (c->de_ev) (void)hipEventDestroy(c->de_ev);
  if (c->de_host) (void)hipHostFree(c->de_host);
  if (c->de_stage) (void)hipHostFree(c->de_stage);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int tblup_set_split(tblup_ctx* c, int split_id, const int64_t* train, int64_t nT, const int64_t* valid,
                    int64_t nV) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (!train || !valid || nT < 1 || nV < 2) return fail(TBLUP_ERR_ARG, "split needs >= 1 train and >= 2 valid rows");
  for (int64_t i = 0; i < nT; ++i)
    if (train[i] < 0 || train[i] >= c->n) return fail(TBLUP_ERR_ARG, "train index out of range");
  for (int64_t i = 0; i < nV; ++i)
    if (valid[i] < 0 || valid[i] >= c->n) return fail(TBLUP_ERR_ARG, "valid index out of range");
  HIPCHK(hipSetDevice(c->device));
  auto sp = std::make_unique<Split>();
  sp->nT = nT;
  sp->nV = nV;
  sp->nTp = round_up(nT, TILE);
  sp->nVp = round_up(nV, TILE);
  sp->nRp = sp->nTp + sp->nVp;
  sp->rows.assign(train, train + nT);
  sp->rows.insert(sp->rows.end(), valid, valid + nV);
  sp->train.assign(train, train + nT);
  sp->valid.assign(valid, valid + nV);
  std::sort(sp->rows.begin(), sp->rows.end());
  std::vector<int32_t> rowmap(sp->nRp, -1);
  for (int64_t i = 0; i < nT; ++i) rowmap[i] = (int32_t)train[i];
  for (int64_t i = 0; i < nV; ++i) rowmap[sp->nTp + i] = (int32_t)valid[i];
  const int nt = c->nt;
  std::vector<double> yT((size_t)nt * sp->nTp, 0.0), yV((size_t)nt * nV);
  sp->meanyT.assign(nt, 0.0);
  YResidual yres{};
  for (int t = 0; t < nt; ++t) {
    // mean(y_T) as numpy computes it for Ridge's y_offset (pairwise summation differs only in rounding)
    long double acc = 0.0L;
    for (int64_t i = 0; i < nT; ++i) {
      const double y = c->pheno[train[i] * nt + t];
      yT[t * sp->nTp + i] = y;
      acc += y;
    }
    sp->meanyT[t] = (double)(acc / (long double)nT);
    long double res = 0.0L;   // what the rounded mean leaves: sum of the doubles y - mean
    for (int64_t i = 0; i < nT; ++i) res += (long double)(yT[t * sp->nTp + i] - sp->meanyT[t]);
    yres.v[t] = (double)res;
    for (int64_t i = 0; i < nV; ++i) yV[t * nV + i] = c->pheno[valid[i] * nt + t];
  }
  if (int rc = dev_alloc(c, sp->gpk, (size_t)(c->P + 1) * (sp->nRp / 4) + 64)) return rc;
  if (int rc = dev_alloc(c, sp->colsumT, (size_t)c->P * 4)) return rc;
  if (int rc = dev_alloc(c, sp->xty, (size_t)nt * c->P * 8)) return rc;
  if (int rc = dev_alloc(c, sp->yT, yT.size() * 8)) return rc;
  if (int rc = dev_alloc(c, sp->yV, yV.size() * 8)) return rc;
  if (int rc = dev_alloc(c, sp->ymu, (size_t)nt * 8)) return rc;
  DevBuf rm;
  if (int rc = dev_alloc(c, rm, rowmap.size() * 4)) return rc;
  HIPCHK(hipMemcpyAsync(rm.p, rowmap.data(), rowmap.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sp->yT.p, yT.data(), yT.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sp->yV.p, yV.data(), yV.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(sp->ymu.p, sp->meanyT.data(), (size_t)nt * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(launch_build_split((const int8_t*)c->geno_sm.p, c->n, c->P, (const int32_t*)rm.p, sp->nRp, nT,
                            (const double*)sp->yT.p, (const double*)sp->ymu.p, yres, nt, (uint8_t*)sp->gpk.p, (int32_t*)sp->colsumT.p, (double*)sp->xty.p, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  dev_free(c, rm);
  if (Split* old = find_split(c, split_id)) old->release(c);
  c->splits[split_id] = std::move(sp);
  return 0;
}

int tblup_set_traits(tblup_ctx* c, const double* pheno, int64_t n_traits) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel (DE / decode-only context)");
  if (!pheno || n_traits < 1 || n_traits > MAXT) return fail(TBLUP_ERR_ARG, "need 1 <= n_traits <= 4 and phenotypes");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& kv : c->splits) kv.second->release(c);   // splits hold per-trait phenotype vectors
  c->splits.clear();
  c->nt = (int)n_traits;
  c->pheno.assign(pheno, pheno + c->n * n_traits);
  return 0;
}

int tblup_get_traits(tblup_ctx* c, int64_t* n_traits) {
  if (int rc = check_ctx(c)) return rc;
  if (n_traits) *n_traits = c->nt;
  return 0;
}

int tblup_drop_split(tblup_ctx* c, int split_id) {
  if (int rc = check_ctx(c)) return rc;
  auto it = c->splits.find(split_id);
  if (it == c->splits.end()) return fail(TBLUP_ERR_ARG, "unknown split id");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  it->second->release(c);
  c->splits.erase(it);
  return 0;
}

static int validate_batch(tblup_ctx* c, int branch, double h2, const int64_t* offsets, int64_t batch) {
  if (branch < 0 || branch > 2) return fail(TBLUP_ERR_ARG, "bad branch");
  if (!(h2 > 0.0) || !(h2 <= 1.0)) return fail(TBLUP_ERR_ARG, "h2 must be in (0, 1]");
  if (batch < 0) return fail(TBLUP_ERR_ARG, "negative batch");
  if (batch > 0 && !offsets) return fail(TBLUP_ERR_ARG, "null offsets");
  if (int rc = check_counts(offsets, batch, "individual")) return rc;
  if (batch > 0 && offsets[0] != 0) return fail(TBLUP_ERR_ARG, "offsets[0] must be 0");
  return 0;
}

}  // extern "C"

int tblup_capi::open_host_batch(HostBatch& hb, tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets,
                                int64_t batch, double h2, int branch, bool have_fitness) {
  hb = HostBatch{};
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_batch(c, branch, h2, offsets, batch)) return rc;
  if (batch == 0) return 0;
  if (!idx || !have_fitness) return fail(TBLUP_ERR_ARG, "null idx/fitness");
  Split* sp = find_split(c, split_id);
  if (!sp) return fail(TBLUP_ERR_ARG, "unknown split id");
  if (int rc = check_indices(c, idx, offsets[batch])) return rc;
  HIPCHK(hipSetDevice(c->device));
  const EvalDims d = dims_of(c, *sp);
  hb = HostBatch{c, sp, d, choose_sys(c, d, offsets, batch, branch, c->form_pref), idx, offsets, batch, h2, branch};
  return 0;
}

int tblup_capi::run_host_batch(const HostBatch& hb, bool with_ebv, const ChunkCarve& carve, const ChunkBody& body) {
  tblup_ctx* c = hb.c;
  HostEntry he(c);
  ChunkReq rq{hb.sp, hb.d, hb.sd, c->stream, hb.h2, hb.branch};
  const int64_t ebv_row = with_ebv ? hb.d.nt * hb.d.nV : 0;
  const auto head = [&](Carve& cv, int64_t B, int64_t sum_k) { return HeadBufs::carve(cv, B, sum_k, B, B * ebv_row); };
  const ChunkBytes bytes = [&](const int64_t*, int64_t B, int64_t sum_k) {   // one form for the whole call
    return measure([&](Carve& cv) {
      head(cv, B, sum_k);
      if (carve) carve(cv, B, sum_k);
      PipeBufs::carve(cv, c, hb.d, hb.sd, B, ChunkMode::Full, false);
    });
  };
  const int rc = for_each_chunk(c, hb.offsets, hb.batch, 65535, bytes, [&](const Chunk& ck) -> int {
    Carve cv{(char*)c->ws.p};
    const HeadBufs h = head(cv, ck.B, ck.sum_k);
    if (int rc = upload_chunk(c, hb.idx, hb.offsets, ck, h.idx, h.off)) return rc;
    rq.d_idx = h.idx; rq.d_off = h.off; rq.h_off = ck.hoff; rq.B = ck.B;
    rq.d_fit = h.fit; rq.d_ebv = h.ebv;
    rq.mode = ChunkMode::Full;
    return body(ck, cv, rq);
  });
  if (rc) return rc;
  return c->profiling ? drain_events(c) : 0;
}

int tblup_capi::factor_pass(const HostBatch& hb, const Chunk& ck, const Carve& cv, ChunkReq& rq, double* fitness,
                            double* ebv, const std::function<int(const CholLaunch&)>& after) {
  tblup_ctx* c = hb.c;
  const size_t ebv_row = (size_t)hb.d.nt * hb.d.nV;
  return run_recovering(c, [&](bool redo, std::vector<int32_t>& seqs) -> int {
    Carve cvp = cv;
    rq.mode = redo ? ChunkMode::SolveOnly : ChunkMode::Full;
    ChunkRes res;
    if (int rc = run_chunk(c, rq, cvp, res)) return rc;
    seqs.push_back(res.chain_seq);
    if (after && !redo)
      if (int rc = after(res.cl)) return rc;
    HIPCHK(hipMemcpyAsync(fitness + ck.b0, rq.d_fit, (size_t)ck.B * 8, hipMemcpyDeviceToHost, c->stream));
    if (ebv)
      HIPCHK(hipMemcpyAsync(ebv + ck.b0 * ebv_row, rq.d_ebv, (size_t)ck.B * ebv_row * 8, hipMemcpyDeviceToHost,
                            c->stream));
    return 0;
  });
}

extern "C" {

// Fitness and, if wanted, the validation EBVs: the chunks through the pipeline, nothing behind it
int tblup_eval_batch(tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets, int64_t batch,
                     double h2, int branch, double* fitness, double* ebv) {
  g_err.clear();
  HostBatch hb;
  if (int rc = open_host_batch(hb, c, split_id, idx, offsets, batch, h2, branch, fitness != nullptr)) return rc;
  if (!hb.sp) return 0;
  return run_host_batch(hb, ebv != nullptr, nullptr, [&](const Chunk& ck, Carve& cv, ChunkReq& rq) {
    return factor_pass(hb, ck, cv, rq, fitness, ebv, nullptr);
  });
}

int tblup_eval_batch_device(tblup_ctx* c, int split_id, const int64_t* d_idx, const int64_t* d_offsets,
                            const int64_t* h_offsets, int64_t batch, double h2, int branch, double* d_fitness,
                            double* d_ebv, void* stream) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_batch(c, branch, h2, h_offsets, batch)) return rc;
  if (batch == 0) return 0;
  if (!d_idx || !d_offsets || !d_fitness) return fail(TBLUP_ERR_ARG, "null device pointers");
  if (batch > 65535) return fail(TBLUP_ERR_ARG, "device batch limited to 65535 individuals per call");
  Split* sp = find_split(c, split_id);
  if (!sp) return fail(TBLUP_ERR_ARG, "unknown split id");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const EvalDims d = dims_of(c, *sp);
  const SysDims sd = choose_sys(c, d, h_offsets, batch, branch, c->form_pref);
  const auto pipe = [&](Carve& cv) { PipeBufs::carve(cv, c, d, sd, batch, ChunkMode::Full, false); };
  if (int rc = ensure_ws(c, s, measure(pipe))) return rc;
  Carve cv{(char*)c->ws.p};
  ChunkReq rq{sp, d, sd, s, h2, branch};
  rq.d_idx = d_idx; rq.d_off = d_offsets; rq.h_off = h_offsets; rq.B = batch;
  rq.d_fit = d_fitness; rq.d_ebv = d_ebv;
  ChunkRes res;
  return run_chunk(c, rq, cv, res);
}

// IntraGCV's k folds (evaluator.py:509-537) or any set of splits: every individual against every
// split in one call, one host round trip for the whole set.  Fold-fused (the default whenever
// the splits have equal dimensions and the batch takes the SNP form with k_sys_tiles): the
// F x B systems (s = f * B + b: individual b against split f) run as ONE batch through one
// launch sequence -- 18 launches instead of 18 F, each filling the chip F times over, the
// system's split picked per workgroup from the FoldTab.  Otherwise the folds' batches run back to
// back on one stream, reusing one workspace in stream order.  Results are bit-identical either
// way (every system's arithmetic is independent of the batch it runs in).

// Whether a chunk can run fused: 2..MAXF splits of equal dimensions, one launch's grid (sd: their common shape)
static bool fold_fusable(const tblup_ctx* c, const std::vector<Split*>& sps, const int64_t* h_off, int64_t B,
                         int branch, SysDims& sd) {
  const int64_t F = (int64_t)sps.size();
  if (!c->fold_fuse || F < 2 || F > MAXF || F * B > 65535 || B < 1) return false;
  for (const Split* sp : sps)
    if (sp->nT != sps[0]->nT || sp->nV != sps[0]->nV || sp->nTp != sps[0]->nTp || sp->nRp != sps[0]->nRp) return false;
  const EvalDims d = dims_of(c, *sps[0]);
  sd = choose_sys(c, d, h_off, B, branch, c->form_pref);
  return true;   // either form: every system reads its own split through the FoldTab
}

// Kernel form, folds partitioning one animal set (IntraGCV): the systems' int8 counts come from one
// A_R A_R^T per individual over fold 0's split rows (k_gshare; FoldTab::gsh) -- the fold systems'
// training rows are all rows of fold 0's split -- instead of one int8 GEMM per system.  The counts
// are the same exact integers, so the results are bit-identical (TBLUP_FOLD_GSHARE=0 for A/B).
// (only where the systems would form their counts in-tile: FP4 system tiles per fold system beat the
// shared int32 counts' row-mapped reads -- config-4-shaped 5 folds 21.9 vs 22.5 ms)
static bool fold_gshare(const tblup_ctx* c, const std::vector<Split*>& sps, const SysDims& sd) {
  if (sd.form != FORM_DUAL || !c->fold_share || !c->fold_gshare || sps.size() < 2) return false;
  if (sys_tiles(c, dims_of(c, *sps[0]), sd)) return false;
  for (const Split* sp : sps)
    if (sp->rows != sps[0]->rows || (int64_t)sp->train.size() != sp->nT || (int64_t)sp->valid.size() != sp->nV)
      return false;
  return true;
}
struct FoldBufs {   // run_folds_fused's own buffers, ahead of the pipeline's
  int64_t *idx_f, *off_f;   // the index lists replicated per fold [F][sum_k]; the fused offsets [F B + 1]
  int32_t *gsh, *dmap;      // under fold_gshare: the shared counts [B][nRp][nRp], the fold row maps [F][nTp]
  static FoldBufs carve(Carve& cv, const tblup_ctx* c, const std::vector<Split*>& sps, const SysDims& sd, int64_t B,
                        int64_t sum_k) {
    const size_t F = sps.size(), nRp = (size_t)sps[0]->nRp;
    const bool g = fold_gshare(c, sps, sd);
    return {cv.take<int64_t>(F * sum_k), cv.take<int64_t>(F * B + 1), g ? cv.take<int32_t>(B * nRp * nRp) : nullptr,
            g ? cv.take<int32_t>(F * sps[0]->nTp) : nullptr};
  }
};

// The fused chunk: the index lists replicated per fold (F x sum_k, device to device), the fused
// offsets built on the device, then run_chunk over F x B systems.  rq: the chunk of B individuals as
// for fold 0 alone (sd: the folds' common shape; d_fit: [F][B]).
static int run_folds_fused(tblup_ctx* c, const std::vector<Split*>& sps, ChunkReq rq, Carve& cv, ChunkRes& res) {
  const int64_t B = rq.B, F = (int64_t)sps.size(), FB = F * B, sum_k = rq.h_off[B];
  const int64_t *d_idx = rq.d_idx, *d_off = rq.d_off, *h_off = rq.h_off;
  const hipStream_t s = rq.s;
  const FoldBufs fb = FoldBufs::carve(cv, c, sps, rq.sd, B, sum_k);
  if (int rc = ws_check(c, cv)) return rc;
  std::vector<int64_t>& ho = c->fold_hoff;   // host copy (run_chunk's work accounting and shapes)
  ho.assign((size_t)FB + 1, 0);
  for (int64_t f = 0; f < F; ++f)
    for (int64_t b = 0; b < B; ++b) ho[f * B + b] = f * sum_k + h_off[b];
  ho[FB] = F * sum_k;
  for (int64_t f = 0; f < F; ++f)
    HIPCHK(hipMemcpyAsync(fb.idx_f + f * sum_k, d_idx, (size_t)sum_k * 8, hipMemcpyDeviceToDevice, s));
  HIPCHK(launch_fold_offsets(d_off, B, F, sum_k, fb.off_f, s));
  FoldTab ft{};
  ft.bpf = B;
  ft.nf = (int)F;
  ft.share = c->fold_share;
  for (int64_t f = 1; f < F; ++f) ft.share = ft.share && sps[f]->rows == sps[0]->rows;
  if (fb.gsh && rq.mode != ChunkMode::SolveOnly) {   // (the solve-only re-run does not read the counts again)
    const int64_t nRp = sps[0]->nRp, nTp = sps[0]->nTp, nT = sps[0]->nT;
    // the fold row maps: system row r of fold f -> fold 0's split row of the same animal
    std::unordered_map<int64_t, int32_t> pos0;
    pos0.reserve((size_t)(sps[0]->nT + sps[0]->nV) * 2);
    for (int64_t i = 0; i < sps[0]->nT; ++i) pos0[sps[0]->train[i]] = (int32_t)i;
    for (int64_t j = 0; j < sps[0]->nV; ++j) pos0[sps[0]->valid[j]] = (int32_t)(nTp + j);
    std::vector<int32_t>& hm = c->gmap_host;
    HIPCHK(hipStreamSynchronize(s));   // the previous chunk's map copy may still read hm
    hm.assign((size_t)(F * nTp), -1);
    for (int64_t f = 0; f < F; ++f)
      for (int64_t r = 0; r < nT; ++r) {
        const auto it = pos0.find(sps[f]->train[r]);
        if (it == pos0.end()) return fail(TBLUP_ERR_STATE, "internal error: fold rows are not one animal set");
        hm[(size_t)(f * nTp + r)] = it->second;
      }
    HIPCHK(hipMemcpyAsync(fb.dmap, hm.data(), hm.size() * 4, hipMemcpyHostToDevice, s));
    ft.gsh = fb.gsh; ft.gmap = fb.dmap; ft.gsh_ld = nRp; ft.gmap_ld = nTp;
  }
  for (int64_t f = 0; f < F; ++f) set_fold(ft, f, *sps[f]);
  rq.d_idx = fb.idx_f; rq.d_off = fb.off_f; rq.h_off = ho.data(); rq.B = FB;
  rq.ft = &ft;
  return run_chunk(c, rq, cv, res);
}

// Workspace of a fold chunk (off: its offsets), behind the host entry's head where there is one: the fused
// layout (0: not fusable) and the largest split-by-split pipeline.  The host entry's chunks fit the larger;
// the device entry runs fused where that fits the budget, else split by split.
struct FoldBytes {
  size_t fused, split;
  SysDims fsd;   // fusable: the folds' common shape
};
static FoldBytes fold_chunk_bytes(const tblup_ctx* c, const std::vector<Split*>& sps, const int64_t* off, int64_t B,
                                  int branch, bool host) {
  const int64_t F = (int64_t)sps.size(), sum_k = off[B];
  const auto bytes = [&](const Split& sp, const SysDims& sd, bool fused) {
    return measure([&](Carve& cv) {
      if (host) HeadBufs::carve(cv, B, sum_k, F * B, 0);
      if (fused) FoldBufs::carve(cv, c, sps, sd, B, sum_k);
      PipeBufs::carve(cv, c, dims_of(c, sp), sd, fused ? F * B : B, ChunkMode::Full, fused && fold_gshare(c, sps, sd));
    });
  };
  FoldBytes fb{};
  for (const Split* sp : sps)
    fb.split = std::max(fb.split, bytes(*sp, choose_sys(c, dims_of(c, *sp), off, B, branch, c->form_pref), false));
  if (fold_fusable(c, sps, off, B, branch, fb.fsd)) fb.fused = bytes(*sps[0], fb.fsd, true);
  return fb;
}

static int validate_splits(tblup_ctx* c, const int* split_ids, int n_splits, std::vector<Split*>& sps) {
  if (!split_ids || n_splits < 1) return fail(TBLUP_ERR_ARG, "need n_splits >= 1 split ids");
  sps.resize(n_splits);
  for (int f = 0; f < n_splits; ++f) {
    sps[f] = find_split(c, split_ids[f]);
    if (!sps[f]) return fail(TBLUP_ERR_ARG, "unknown split id " + std::to_string(split_ids[f]));
  }
  return 0;
}

// One chunk against every split on rq's stream: fused (fsd: the folds' common shape) through one launch
// sequence, else split by split, every split reusing the workspace after `head` in stream order.
// rq: the chunk, its mode and d_fit [F][B]; seqs: the chained solves enqueued.
static int run_folds(tblup_ctx* c, const std::vector<Split*>& sps, ChunkReq rq, bool fused, const SysDims& fsd,
                     const Carve& head, std::vector<int32_t>& seqs) {
  double* const d_fit = rq.d_fit;
  for (size_t f = 0; f < (fused ? 1 : sps.size()); ++f) {
    Carve cv = head;
    ChunkRes res;
    rq.sp = sps[f];
    rq.d = dims_of(c, *sps[f]);
    rq.sd = fused ? fsd : choose_sys(c, rq.d, rq.h_off, rq.B, rq.branch, c->form_pref);
    rq.d_fit = d_fit + (int64_t)f * rq.B;
    if (int rc = fused ? run_folds_fused(c, sps, rq, cv, res) : run_chunk(c, rq, cv, res)) return rc;
    seqs.push_back(res.chain_seq);
  }
  return 0;
}

int tblup_eval_folds_device(tblup_ctx* c, const int* split_ids, int n_splits, const int64_t* d_idx,
                            const int64_t* d_offsets, const int64_t* h_offsets, int64_t batch, double h2, int branch,
                            double* d_fitness, void* stream) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_batch(c, branch, h2, h_offsets, batch)) return rc;
  std::vector<Split*> sps;
  if (int rc = validate_splits(c, split_ids, n_splits, sps)) return rc;
  if (batch == 0) return 0;
  if (!d_idx || !d_offsets || !d_fitness) return fail(TBLUP_ERR_ARG, "null device pointers");
  if (batch > 65535) return fail(TBLUP_ERR_ARG, "device batch limited to 65535 individuals per call");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const FoldBytes need = fold_chunk_bytes(c, sps, h_offsets, batch, branch, false);
  const bool fused = need.fused > 0 && need.fused <= c->budget;   // else split by split: the largest split's chunk
  if (int rc = ensure_ws(c, s, fused ? need.fused : need.split)) return rc;
  ChunkReq rq{nullptr, {}, {}, s, h2, branch};   // run_folds sets the split, its dims and the system shape
  rq.d_idx = d_idx; rq.d_off = d_offsets; rq.h_off = h_offsets; rq.B = batch;
  rq.d_fit = d_fitness;
  std::vector<int32_t> seqs;   // device entry: an expiry raises the status word instead
  return run_folds(c, sps, rq, fused, need.fsd, Carve{(char*)c->ws.p}, seqs);
}

int tblup_eval_folds(tblup_ctx* c, const int* split_ids, int n_splits, const int64_t* idx, const int64_t* offsets,
                     int64_t batch, double h2, int branch, double* fitness) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_batch(c, branch, h2, offsets, batch)) return rc;
  std::vector<Split*> sps;
  if (int rc = validate_splits(c, split_ids, n_splits, sps)) return rc;
  if (batch == 0) return 0;
  if (!idx || !fitness) return fail(TBLUP_ERR_ARG, "null idx/fitness");
  if (int rc = check_indices(c, idx, offsets[batch])) return rc;
  HIPCHK(hipSetDevice(c->device));
  HostEntry he(c);
  // the form is chosen per chunk, from the candidate's own offsets
  const ChunkBytes fold_bytes = [&](const int64_t* off, int64_t B, int64_t) {
    const FoldBytes fb = fold_chunk_bytes(c, sps, off, B, branch, true);
    return std::max(fb.fused, fb.split);
  };
  ChunkReq rq{nullptr, {}, {}, c->stream, h2, branch};   // run_folds sets the split, its dims and the system shape
  const int rc = for_each_chunk(c, offsets, batch, 65535, fold_bytes, [&](const Chunk& ck) -> int {
    const int64_t B = ck.B;
    Carve head{(char*)c->ws.p};
    const HeadBufs h = HeadBufs::carve(head, B, ck.sum_k, n_splits * B, 0);
    if (int rc = upload_chunk(c, idx, offsets, ck, h.idx, h.off)) return rc;
    double* const d_fit = rq.d_fit = h.fit;
    rq.d_idx = h.idx; rq.d_off = h.off; rq.h_off = ck.hoff; rq.B = B;
    SysDims fsd{};
    const bool fused = fold_fusable(c, sps, ck.hoff, B, branch, fsd);
    return run_recovering(c, [&](bool redo, std::vector<int32_t>& seqs) -> int {
      // redo, after a chained solve gave up a wait: fused, the same factor solved by k_solve; split
      // by split (the folds reuse one workspace, so the earlier folds' factors are gone), every fold
      // again with the chained solve off -- bit-identical either way
      rq.mode = !redo ? ChunkMode::Full : fused ? ChunkMode::SolveOnly : ChunkMode::NoChain;
      if (int rc = run_folds(c, sps, rq, fused, fsd, head, seqs)) return rc;
      for (int f = 0; f < n_splits; ++f)
        HIPCHK(hipMemcpyAsync(fitness + (int64_t)f * batch + ck.b0, d_fit + (int64_t)f * B, (size_t)B * 8,
                              hipMemcpyDeviceToHost, c->stream));
      return 0;
    });
  });
  if (rc) return rc;
  return c->profiling ? drain_events(c) : 0;
}

int tblup_set_profiling(tblup_ctx* c, int enable) {
  if (int rc = check_ctx(c)) return rc;
  c->profiling = enable != 0;
  return 0;
}

int tblup_get_profile(tblup_ctx* c, double* ms, int64_t* launches, double* flops, double* bytes) {
  if (int rc = check_ctx(c)) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = drain_events(c)) return rc;
  for (int i = 0; i < TBLUP_N_KCLASS; ++i) {
    if (ms) ms[i] = c->ms[i];
    if (launches) launches[i] = c->launches[i];
    if (flops) flops[i] = c->flops[i];
    if (bytes) bytes[i] = c->bytes[i];
  }
  return 0;
}

int tblup_reset_profile(tblup_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = drain_events(c)) return rc;
  for (int i = 0; i < TBLUP_N_KCLASS; ++i) {
    c->ms[i] = 0;
    c->launches[i] = 0;
    c->flops[i] = 0;
    c->bytes[i] = 0;
  }
  return 0;
}

int tblup_debug_grm(tblup_ctx* c, int split_id, const int64_t* idx, int64_t k, double h2, int branch, int stage,
                    double* out, double* z_out) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (!idx || k < 1 || !out) return fail(TBLUP_ERR_ARG, "bad debug arguments");
  if (stage != 1 && stage != 2) return fail(TBLUP_ERR_ARG, "stage must be 1 or 2");
  int64_t offs[2] = {0, k};
  if (int rc = validate_batch(c, branch, h2, offs, 1)) return rc;
  if (int rc = check_indices(c, idx, k)) return rc;
  Split* sp = find_split(c, split_id);
  if (!sp) return fail(TBLUP_ERR_ARG, "unknown split id");
  HIPCHK(hipSetDevice(c->device));
  const EvalDims d = dims_of(c, *sp);
  const SysDims sd = choose_sys(c, d, offs, 1, branch, 1);   // readback is of the kernel (dual) form
  HIPCHK(hipStreamSynchronize(c->stream));
  const ChunkMode mode = stage == 1 ? ChunkMode::DebugK : ChunkMode::DebugL;
  const auto carve = [&](Carve& cv) { HeadBufs::carve(cv, 1, k, 1, 0); PipeBufs::carve(cv, c, d, sd, 1, mode, false); };
  if (int rc = dev_alloc(c, c->ws, measure(carve))) return rc;
  Carve cv{(char*)c->ws.p};
  const HeadBufs h = HeadBufs::carve(cv, 1, k, 1, 0);
  if (int rc = upload_chunk(c, idx, offs, Chunk{0, 1, k, offs}, h.idx, h.off)) return rc;
  ChunkReq rq{sp, d, sd, c->stream, h2, branch};
  rq.d_idx = h.idx; rq.d_off = h.off; rq.h_off = offs; rq.B = 1;
  rq.d_fit = h.fit;
  rq.mode = mode;
  ChunkRes res;
  if (int rc = run_chunk(c, rq, cv, res)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t rows = (stage == 1) ? d.nRp : d.nTp;
  std::vector<double> full((size_t)rows * d.nTp);
  HIPCHK(hipMemcpy(full.data(), res.K, full.size() * 8, hipMemcpyDeviceToHost));
  const int64_t nR = d.nT + d.nV;
  if (stage == 2) {
    // Lt tiles: tile (I, J) at ((I*NT + J) * 128*128), element [j][i] = L[128I+i][128J+j]
    std::memset(out, 0, (size_t)nR * d.nT * 8);   // upper triangle and V rows are zero
    const int64_t TT = (int64_t)TILE * TILE;
    for (int64_t r = 0; r < d.nT; ++r)
      for (int64_t cc = 0; cc <= r; ++cc) {
        const int64_t I = r / TILE, Jt = cc / TILE;
        out[r * d.nT + cc] = full[(I * d.NT + Jt) * TT + (cc % TILE) * TILE + (r % TILE)];
      }
  } else {
    for (int64_t r = 0; r < nR; ++r) {
      const int64_t src = r < d.nT ? r : d.nTp + (r - d.nT);
      std::memcpy(out + r * d.nT, full.data() + src * d.nTp, (size_t)d.nT * 8);
    }
  }
  if (z_out) {
    std::vector<double> zz(d.nTp);   // trait 0
    HIPCHK(hipMemcpy(zz.data(), res.z, (size_t)d.nTp * 8, hipMemcpyDeviceToHost));
    std::memcpy(z_out, zz.data(), (size_t)d.nT * 8);
  }
  return c->profiling ? drain_events(c) : 0;
}

int tblup_grm(tblup_ctx* c, const int64_t* idx, int64_t k, double* G) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel");
  if (!idx || k < 1 || !G) return fail(TBLUP_ERR_ARG, "bad grm arguments");
  const int64_t n = c->n;
  // G = K_TT of the gblup-branch kernel form with T = every animal (p over all rows, as
  // make_grm) and lambda = 0 (h2 = 1); V is a placeholder the solve never reaches
  std::vector<int64_t> T(n);
  for (int64_t i = 0; i < n; ++i) T[i] = i;
  const int64_t V[2] = {0, 1};
  const int sid = -0x7ffffff0;   // reserved id, dropped before returning
  if (int rc = tblup_set_split(c, sid, T.data(), n, V, 2)) return rc;
  std::vector<double> K((size_t)(n + 2) * n);
  const int rc = tblup_debug_grm(c, sid, idx, k, 1.0, TBLUP_BRANCH_GBLUP, 1, K.data(), nullptr);
  const std::string err = g_err;
  tblup_drop_split(c, sid);
  if (rc) return fail(rc, err);
  for (int64_t r = 0; r < n; ++r)   // lower-triangle tiles are computed; mirror the upper triangle
    for (int64_t cc = 0; cc < n; ++cc) G[r * n + cc] = cc <= r ? K[(size_t)r * n + cc] : K[(size_t)cc * n + r];
  return 0;
}

int tblup_get_wg_trace(tblup_ctx* c, uint64_t* out, int64_t cap, int64_t* n_records) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (!n_records) return fail(TBLUP_ERR_ARG, "null n_records");
  *n_records = c->wg_trace ? c->wgt_used : 0;
  if (!c->wg_trace || !out || cap <= 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipDeviceSynchronize());
  const int64_t n = std::min(cap, c->wgt_used);
  HIPCHK(hipMemcpy(out, c->wgt.p, (size_t)n * WGT_REC * 8, hipMemcpyDeviceToHost));
  return 0;
}

static int read_status_word(tblup_ctx* c, void* stream, int* flag, int word) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (!flag) return fail(TBLUP_ERR_ARG, "null flag");
  *flag = 0;
  if (!c->status.p) return 0;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  int32_t h = 0;
  int32_t* w = (int32_t*)c->status.p + word;
  HIPCHK(hipMemcpyAsync(&h, w, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemsetAsync(w, 0, 4, s));
  HIPCHK(hipStreamSynchronize(s));
  *flag = h != 0;
  return 0;
}

int tblup_index_error(tblup_ctx* c, void* stream, int* flag) { return read_status_word(c, stream, flag, ST_INDEX); }

int tblup_solve_error(tblup_ctx* c, void* stream, int* flag) { return read_status_word(c, stream, flag, ST_SOLVE); }

int tblup_status_async(tblup_ctx* c, void* stream, int32_t* host_status) {
  g_err.clear();
  if (int rc = check_ctx(c)) return rc;
  if (!host_status) return fail(TBLUP_ERR_ARG, "null host_status");
  if (!c->status.p) return fail(TBLUP_ERR_STATE, "context has no genotype panel");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  HIPCHK(hipMemcpyAsync(host_status, c->status.p, ST_WORDS * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemsetAsync(c->status.p, 0, ST_WORDS * 4, s));
  return 0;
}

int tblup_chain_recoveries(tblup_ctx* c, int64_t* count) {
  if (int rc = check_ctx(c)) return rc;
  if (!count) return fail(TBLUP_ERR_ARG, "null count");
  *count = c->chain_recoveries;
  return 0;
}

int tblup_mem_info(tblup_ctx* c, int64_t* bytes) {
  if (int rc = check_ctx(c)) return rc;
  if (bytes) *bytes = c->mem_in_use;
  return 0;
}

}  // extern "C"
