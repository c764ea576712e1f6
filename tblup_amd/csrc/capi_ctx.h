// Internal to libtblup_gpu.so's C-ABI translation units (capi.hip, capi_aux.hip, capi_model.hip): the context
// (struct tblup_ctx of include/tblup_gpu.h), its device buffers, the error / allocation helpers, the
// evaluation pipeline of one chunk and the host entries' chunk driver.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tblup_gpu.h"
#include "tblup_internal.h"

struct tblup_ctx;

namespace tblup_capi {

int fail(int code, const std::string& msg);   // sets the calling thread's tblup_last_error()

#define HIPCHK(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return fail(TBLUP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct Split {
  int64_t nT = 0, nV = 0, nTp = 0, nVp = 0, nRp = 0;
  std::vector<int64_t> rows;   // train + valid animals, sorted (fold sets: shared counts)
  std::vector<int64_t> train, valid;   // the split's animal lists in system-row order
  std::vector<double> meanyT;   // [nt]
  DevBuf gpk, colsumT, xty, yT, yV, ymu;
  void release(tblup_ctx* c);   // frees the six device buffers (dev_free: the context's memory accounting)
};

enum { KC_STATS = 0, KC_GATHER, KC_GRM, KC_DIAG, KC_OFFDIAG, KC_SOLVE };

struct EventPair {
  int cls;
  hipEvent_t a, b;
};

}  // namespace tblup_capi

using tblup_capi::DevBuf;
using tblup_capi::EventPair;
using tblup_capi::Split;

struct tblup_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t n = 0, P = 0;
  DevBuf geno_sm, colsum_all, scratch;
  DevBuf status;               // int32 [ST_WORDS] device status words: ST_INDEX an index outside
                               // [-P, P) reached k_indiv_stats; ST_SOLVE a chained-solve wait expired
  std::vector<double> pheno;   // [n][nt] animal-major
  int nt = 1;                  // traits (tblup_set_traits)
  std::map<int, std::unique_ptr<Split>> splits;
  DevBuf ws;
  DevBuf dec_keys, dec_idx;   // host-pointer decode staging
  DevBuf de_polys, de_small, de_par, de_chi;   // DE step: jump polynomials, per-call args, host-path staging
  int64_t de_L = -1, de_pop = -1;              // (L, pop) of the uploaded polynomials
  bool de_end_jump = false;
  uint32_t* de_host = nullptr;   // page-locked: the MT state after the last step (624 words + pos)
  char* de_stage = nullptr;      // page-locked: the per-call arguments on their way to de_small
  size_t de_stage_bytes = 0;
  hipEvent_t de_ev = nullptr;    // recorded behind that state's copy
  bool de_pending = false;       // tblup_de_step_device_async issued, tblup_de_state_wait not yet called
  // MDE_pBX (tblup_mde_draws -> tblup_mde_step_device_async): the draws' device buffer (base key,
  // window tables, draw words, the three-launch form's sequence and windows) and what it was made for
  DevBuf mde_dev;
  std::vector<uint32_t> mde_key;   // the base key of the last tblup_mde_draws (empty: none to continue)
  int32_t mde_pos = -1;
  int64_t mde_cmax = 0;   // hi[pop - 1] of those draws' windows: no resolved C_i can exceed it
  int64_t mde_pop = -1, mde_L = -1, mde_scr = 0;   // mde_scr: byte offset of the scratch in mde_dev, 0 = one-launch form
  size_t budget = 0;
  // profiling
  bool profiling = false;
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> event_pool;
  double ms[TBLUP_N_KCLASS] = {0};
  int64_t launches[TBLUP_N_KCLASS] = {0};
  double flops[TBLUP_N_KCLASS] = {0};
  double bytes[TBLUP_N_KCLASS] = {0};
  int64_t mem_in_use = 0;

  // TBLUP_WG_TRACE: per-workgroup start/end records of the Cholesky launches of the last chunk
  bool wg_trace = false;
  DevBuf wgt;
  int64_t wgt_used = 0;
  int dbg_skip = 0;   // TBLUP_DBG_SKIP, read only by diagnostic builds (-DTBLUP_DIAG_BUILD): phase
                      // ablation, results wrong when set; the production library never reads it
  int form_pref = 0;  // TBLUP_FORM: 0 auto, 1 kernel (dual) form only, 2 SNP (primal) form for snp batches
  // Cholesky schedule (results are bit-identical under every setting; see OffPlan):
  int ahead = -1;     // TBLUP_AHEAD: -1 auto (per launch: B * (NT - 2 - j) < AHEAD_SLOTS), 0 never, 1 always
  int nrs = 0;        // TBLUP_NRS: partial-sum row slices, 0 auto, else 1 / 2 / 4
  int diag_d = -1;    // TBLUP_DIAG_D: D-units in the diagonal launch (-1 auto, 0 never, 1 always)
  int diag_e = -1;    // TBLUP_DIAG_E: E-units in the diagonal launch (-1 auto, 0 never, 1 every tile)
  int diag_waves = 0; // TBLUP_DIAG_WAVES: waves of the diagonal workgroups in launches without D- / E-units
                      // (0 auto, 8, 12, 16: diag_waves(), tblup_internal.h)
  int chain_sync = 0;    // TBLUP_CHAIN_SYNC (k_solve.hip)
  int last_term = -1;    // TBLUP_LAST_TERM: -1 auto (last_term_mask), 0 never, 1 always (see use_last_term)
  int lt_mask = -1;      // TBLUP_LT_MASK: the diagonal launches in last-term mode by bit (A/B timing; -1 auto)
  int solve_chain = -1;  // TBLUP_SOLVE_CHAIN: SNP-form back substitution spread over the chip (k_solve_chain):
                         // -1 auto (B <= CHAIN_MAX_B), 0 never, 1 always -- bit-identical results either way
  int solve_pull = -1;   // TBLUP_SOLVE_PULL: the chained solve's units pull beta_K and the tiles of their block
                         // column (1; -1 auto: one trait) or push the tile products of their block row (0)
                         // -- the same bits
  int fold_fuse = 1;     // TBLUP_FOLD_FUSE: 0 evaluates a fold set split by split (A/B timing)
  int fold_share = 1;    // TBLUP_FOLD_SHARE: 0 builds every fold's system tiles from its own rows
  int fold_gshare = 1;   // TBLUP_FOLD_GSHARE: kernel-form folds read their counts from one A_R A_R^T
  int dual_st = 1;       // TBLUP_DUAL_ST: kernel-form system tiles from k_sys_tiles (0: in-tile products)
  std::vector<int32_t> gmap_host;   // the fold row maps of the last fused kernel-form chunk (H2D source)
  int sys_st = -1;       // TBLUP_SYS_ST: system tiles by the persistent super-tile kernel (k_sys_tiles_st):
                         // -1 auto (sys_tiles_grid), 0 never, 1 whenever it applies -- the same exact counts
  // SNP form: the padding rows (ns - k) lead the system, so the contractions over block column 0
  // skip them (TBLUP_PAD_FIRST=0: trailing padding, equal up to rounding -- a test knob).
  int pad_first = 1;
  // TBLUP_RELIAB_LDS=0: k_reliab keeps its right-hand sides in the workspace at every system size (what
  // it does above 1024 rows anyway; the same bits -- a test knob)
  int reliab_lds = 1;
  // TBLUP_SCORE_LDS=0: the same for k_snpscore's right-hand sides (tblup_snp_score_batch)
  int score_lds = 1;
  std::vector<int64_t> fold_hoff;   // host offsets of the last fold-fused chunk (host-side shapes only)
  DevBuf chain;          // its flags [B][chain_flags(NT)], the expiry ring [CHAIN_ERR_RING] and one
                         // scratch word (zeroed when allocated)
  int32_t chain_seq = 0; // flag value of the last chained solve
  bool host_entry = false;      // a synchronous entry is running: its chained solves recover on expiry
  int64_t chain_recoveries = 0; // chunks whose expired chained solve was re-run through k_solve
  // debug knob (TBLUP_CHAIN_DEBUG="spin,delay,shots"): the next `shots` chained solves poll at
  // most `spin` times and delay one producer by `delay` sleep rounds -- forces an expiry (tests)
  int32_t chain_dbg_spin = 0, chain_dbg_delay = 0, chain_dbg_shots = 0;
};

namespace tblup_capi {
int dev_alloc(tblup_ctx* c, DevBuf& b, size_t bytes);
void dev_free(tblup_ctx* c, DevBuf& b);
int check_ctx(tblup_ctx* c);
void clear_error();

// Buffers of a chunk, taken in order from the workspace (each starts on a 256-byte boundary).  A Carve
// without a base only measures: it hands out null pointers and `used` is what the same takes need.
struct Carve {
  char* base;
  size_t used = 0;
  template <typename T>
  T* take(size_t count) {
    used = round_up((int64_t)used, 256);
    T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += count * sizeof(T);
    return p;
  }
};
// The bytes a carve function takes: the one place a workspace size comes from (no slack on top)
template <typename F>
size_t measure(F&& carve) {
  Carve cv{nullptr};
  carve(cv);
  return (size_t)round_up((int64_t)cv.used, 256);
}
// Every buffer carved so far lies inside the workspace (checked before the launches that use
// them: a sizing mistake fails the call instead of faulting the GPU)
int ws_check(const tblup_ctx* c, const Carve& cv);
// numpy's fancy-index bound (the reference's data[:, indices], evaluator.py:275/298):
// -P <= i < P is valid (negatives wrap, on the device); anything else is numpy's IndexError.
int check_indices(const tblup_ctx* c, const int64_t* idx, int64_t count);
// every one of the batch's index lists is non-empty ("every <who> needs k >= 1 indices")
int check_counts(const int64_t* offsets, int64_t batch, const char* who);
// the branch an individual of k SNPs takes (evaluator.py:257): 1 gblup, 2 snp; branch 0 = auto
inline int branch_of(const tblup_ctx* c, int64_t k, int branch) { return branch ? branch : (k > c->n ? 1 : 2); }

// The host entries' chunk loop.  Individuals [b0, b0 + B) of the batch: sum_k indices, hoff their
// B + 1 offsets rebased to 0 (valid until the body returns).
struct Chunk {
  int64_t b0, B, sum_k;
  const int64_t* hoff;
};
// workspace bytes of a candidate chunk (its rebased offsets, B, sum_k)
using ChunkBytes = std::function<size_t(const int64_t* hoff, int64_t B, int64_t sum_k)>;
// Runs `body` on each chunk of the batch in turn.  A chunk grows while its bytes fit the context's
// budget (TBLUP_WORKSPACE_MB) and max_B individuals (one launch's grid); its first individual always
// fits.  Before the body: the context's stream synchronised, the workspace grown to the chunk's bytes.
int for_each_chunk(tblup_ctx* c, const int64_t* offsets, int64_t batch, int64_t max_B, const ChunkBytes& bytes,
                   const std::function<int(const Chunk&)>& body);
// The chunk's index list and offsets on their way to d_idx [sum_k] / d_off [B + 1] on the context's stream
int upload_chunk(tblup_ctx* c, const int64_t* idx, const int64_t* offsets, const Chunk& ck, int64_t* d_idx,
                 int64_t* d_off);

// ---- the evaluation pipeline of one chunk (capi.hip) ----
enum class ChunkMode {
  Full,        // the whole pipeline
  DebugK,      // debug readback: the pipeline up to the full K block (k_grm)
  DebugL,      // debug readback: the pipeline up to the factor L and z
  SolveOnly,   // the solve only, through the one-workgroup k_solve, on the factor an earlier run_chunk
               // of the same chunk left in the same carve (host entries, after that run's chained
               // solve gave up a wait: bit-identical results)
  NoChain,     // the whole pipeline with the one-workgroup k_solve instead of the chained solve (a
               // per-call choice: the context's policy is not touched)
};

// One chunk whose idx/off already sit in device memory, as run_chunk enqueues it.  An entry fixes the
// first six members once (ChunkReq rq{sp, d, sd, s, h2, branch}: six distinct types); the chunk's
// pointers, B and the mode are set by name.
struct ChunkReq {
  const Split* sp;
  tblup::EvalDims d;
  tblup::SysDims sd;
  hipStream_t s;
  double h2;
  int branch;
  const int64_t *d_idx = nullptr, *d_off = nullptr;
  const int64_t* h_off = nullptr;   // host copy of the offsets (work accounting and shapes)
  int64_t B = 0;
  double* d_fit = nullptr;       // [B] fitness
  double* d_ebv = nullptr;       // [B][nt][nV], if wanted
  const tblup::FoldTab* ft = nullptr;   // the systems' splits when they are not all sp (fold-fused evaluation;
                                        // sp is then fold 0)
  ChunkMode mode = ChunkMode::Full;
  const double* d_h2 = nullptr;  // [B] per-system h2 on the device (tblup_loglik_batch); null: h2
};

struct ChunkRes {
  int32_t chain_seq = 0;    // seq of the chained solve this run enqueued, 0 if none
  double* K = nullptr;      // debug readbacks: the K block (DebugK), else the factor L
  double* z = nullptr;
  tblup::CholLaunch cl{};   // the chunk's buffers, for a launch after the pipeline (launch_effects)
};

// Enqueue the pipeline for one chunk (no host synchronisation unless the chain flags must grow); its
// buffers (PipeBufs, capi.hip) are carved next from cv and the lot checked against the workspace.
int run_chunk(tblup_ctx* c, const ChunkReq& rq, Carve& cv, ChunkRes& res);
// A host entry's chunk with recovery.  enqueue(redo, seqs) enqueues one pass on the context's stream --
// its launches and the copies of the results to the host -- and lists the chained solves it enqueued.
// Pass 0 (redo false) is the chunk as usual; when one of its chained solves gave up a wait, the pass
// is enqueued once more with redo set (the entry solves through k_solve then) and the chunk counted.
int run_recovering(tblup_ctx* c, const std::function<int(bool redo, std::vector<int32_t>& seqs)>& enqueue);

// ---- the host entries' driver (capi.hip) ----
// tblup_eval_batch (capi.hip) and the entries that read the factor it leaves (capi_model.hip) are each one
// function: its argument checks, open_host_batch, run_host_batch with its body as a lambda, its host-side
// post-pass.  The driver owns the batch's validation, the split, the system shape, the chunking, idx / off /
// fitness / EBVs and ChunkReq's per-chunk members.  An entry writes its own buffers down once, as a carve
// function: the body calls it on the chunk's Carve, the chunker on a measuring one.
struct HostBatch {
  tblup_ctx* c;
  Split* sp;                 // null: an empty batch, nothing to run
  tblup::EvalDims d;
  tblup::SysDims sd;         // one form for the whole call
  const int64_t *idx, *offsets;
  int64_t batch;
  double h2;
  int branch;
  std::vector<double> own_fitness;   // fitness_or_own: room for the batch's where the caller wants none
  double* fitness_or_own(double* fitness) {
    if (!fitness) own_fitness.resize((size_t)batch);
    return fitness ? fitness : own_fitness.data();
  }
};
// Validates in order: context, branch / h2 / offsets, the empty batch (0, hb.sp null), idx and `have_fitness`,
// the split, the indices; then selects the device and fills hb.
int open_host_batch(HostBatch& hb, tblup_ctx* c, int split_id, const int64_t* idx, const int64_t* offsets,
                    int64_t batch, double h2, int branch, bool have_fitness);
// The entry's own buffers of a chunk of B individuals and sum_k indices, taken from cv (a result is ignored)
using ChunkCarve = std::function<void(Carve& cv, int64_t B, int64_t sum_k)>;
// A chunk, the Carve behind its idx / off / fitness / EBVs, the request with every per-chunk member set
using ChunkBody = std::function<int(const Chunk& ck, Carve& cv, ChunkReq& rq)>;
// Runs the batch chunk by chunk as a synchronous entry (its chained solves recover on expiry), a chunk's
// bytes measured on the head's, `carve`'s (null: nothing) and the pipeline's takes; then collects the events.
int run_host_batch(const HostBatch& hb, bool with_ebv, const ChunkCarve& carve, const ChunkBody& body);
// One pass of a chunk's pipeline with recovery (redo: the same factor solved by k_solve, for the fitness and
// the EBVs only).  after(cl) (null: nothing) is enqueued behind pass 0 on the factor it leaves: neither solve
// kernel writes L, the diagonal inverses, z, u or the scalars, so it does not wait for the chained solve's
// verdict.  Behind either pass the chunk's fitness and, ebv non-null, EBVs [batch][nt][nV] are copied out.
int factor_pass(const HostBatch& hb, const Chunk& ck, const Carve& cv, ChunkReq& rq, double* fitness, double* ebv,
                const std::function<int(const tblup::CholLaunch& cl)>& after);
}  // namespace tblup_capi
