// C ABI of libtblup_gpu.so, the entry points beside the evaluation pipeline (include/tblup_gpu.h):
// RandomKey genome decode, the seeder's SNP scan, the GPU DE generation step (numpy's MT19937
// stream jumped per individual, mt_jump.cpp) and its helpers, host memory registration.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "capi_ctx.h"
#include "mt_jump.h"

using namespace tblup;
using namespace tblup_capi;

extern "C" {

static int validate_decode(int64_t batch, int64_t d, const int64_t* offsets) {
  if (batch < 0 || d < 1 || d > 0x7fffffff) return fail(TBLUP_ERR_ARG, "decode needs batch >= 0, 1 <= d < 2^31");
  if (batch > 0 && (!offsets || offsets[0] != 0)) return fail(TBLUP_ERR_ARG, "offsets must start at 0");
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t k = offsets[b + 1] - offsets[b];
    if (k < 1 || k > d || k > 8192) return fail(TBLUP_ERR_ARG, "every k must be in [1, min(d, 8192)]");
  }
  return 0;
}

int tblup_decode_topk_device(tblup_ctx* c, const double* d_keys, int64_t batch, int64_t d, int64_t ld,
                             const int64_t* d_offsets, const int64_t* h_offsets, int64_t* d_idx_out, void* stream) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_decode(batch, d, h_offsets)) return rc;
  if (ld < d) return fail(TBLUP_ERR_ARG, "ld < d");
  if (batch == 0) return 0;
  if (!d_keys || !d_offsets || !d_idx_out) return fail(TBLUP_ERR_ARG, "null device pointers");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  HIPCHK(launch_decode_topk(d_keys, batch, d, ld, d_offsets, d_idx_out, s));
  return 0;
}

int tblup_decode_topk(tblup_ctx* c, const double* keys, int64_t batch, int64_t d, const int64_t* offsets,
                      int64_t* idx_out) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_decode(batch, d, offsets)) return rc;
  if (batch == 0) return 0;
  if (!keys || !idx_out) return fail(TBLUP_ERR_ARG, "null keys/idx_out");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t total = offsets[batch];
  if (int rc = dev_alloc(c, c->dec_keys, (size_t)batch * d * 8)) return rc;
  if (int rc = dev_alloc(c, c->dec_idx, (size_t)(total + batch + 1) * 8)) return rc;
  int64_t* d_idx = (int64_t*)c->dec_idx.p;
  int64_t* d_off = d_idx + total;
  HIPCHK(hipMemcpyAsync(c->dec_keys.p, keys, (size_t)batch * d * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_off, offsets, (size_t)(batch + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(launch_decode_topk((const double*)c->dec_keys.p, batch, d, d, d_off, d_idx, c->stream));
  HIPCHK(hipMemcpyAsync(idx_out, d_idx, (size_t)total * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int tblup_snp_scan(tblup_ctx* c, const int64_t* rows, int64_t n_rows, const double* yc, int64_t* sx, int64_t* sxx,
                   double* sxy) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->n == 0) return fail(TBLUP_ERR_STATE, "context has no genotype panel");
  if (!rows || n_rows < 1 || !yc || !sx || !sxx || !sxy) return fail(TBLUP_ERR_ARG, "bad scan arguments");
  std::vector<int32_t> r32((size_t)n_rows);
  for (int64_t i = 0; i < n_rows; ++i) {
    if (rows[i] < 0 || rows[i] >= c->n) return fail(TBLUP_ERR_ARG, "animal row out of range");
    r32[i] = (int32_t)rows[i];
  }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t P = (size_t)c->P;
  DevBuf buf;
  const size_t o_y = round_up(4 * (size_t)n_rows, 16), o_sx = o_y + 8 * (size_t)n_rows, o_sxx = o_sx + 8 * P,
               o_sxy = o_sxx + 8 * P, bytes = o_sxy + 8 * P;
  if (int rc = dev_alloc(c, buf, bytes)) return rc;
  char* b = (char*)buf.p;
  int rc = 0;
  auto run = [&]() -> int {
    HIPCHK(hipMemcpyAsync(b, r32.data(), 4 * (size_t)n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_y, yc, 8 * (size_t)n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_snp_scan((const int8_t*)c->geno_sm.p, c->n, c->P, (const int32_t*)b, n_rows,
                           (const double*)(b + o_y), (int64_t*)(b + o_sx), (int64_t*)(b + o_sxx),
                           (double*)(b + o_sxy), c->stream));
    HIPCHK(hipMemcpyAsync(sx, b + o_sx, 8 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sxx, b + o_sxx, 8 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sxy, b + o_sxy, 8 * P, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
  };
  rc = run();
  dev_free(c, buf);
  return rc;
}

// ---- differential-evolution step (k_de.hip; jump polynomials from mt_jump.cpp) ----

int tblup_mt19937_jump(const uint32_t* key, int32_t pos, uint64_t n_words, uint32_t* key_out, int32_t* pos_out) {
  clear_error();
  if (!key || !key_out || !pos_out) return fail(TBLUP_ERR_ARG, "null key/key_out/pos_out");
  if (pos < 0 || pos > 624) return fail(TBLUP_ERR_ARG, "pos must be in [0, 624]");
  int po = 0;
  tblup_mt::jump_state(key, pos, n_words, key_out, &po);
  *pos_out = po;
  return 0;
}

int tblup_de_donors(int strategy, int64_t pop, int64_t L, int32_t best, uint32_t* py_mt, int32_t* py_index,
                    int32_t* donors, int64_t* fixed) {
  clear_error();
  if (strategy != TBLUP_DE_RAND_1 && strategy != TBLUP_DE_CURRENT_TO_BEST_1)
    return fail(TBLUP_ERR_ARG, "unknown DE strategy");
  if (pop < 4 || pop > 65535 || L < 1 || L >= ((int64_t)1 << 32))
    return fail(TBLUP_ERR_ARG, "need 4 <= pop <= 65535 and 1 <= L < 2^32");
  if (!py_mt || !py_index || !donors || !fixed) return fail(TBLUP_ERR_ARG, "null py_mt/py_index/donors/fixed");
  if (*py_index < 0 || *py_index > 624) return fail(TBLUP_ERR_ARG, "py_index must be in [0, 624]");
  if (strategy == TBLUP_DE_CURRENT_TO_BEST_1 ? (best < 0 || best >= pop) : best != -1)
    return fail(TBLUP_ERR_ARG, "best must be in [0, pop) for current-to-best/1 and -1 for rand/1");
  tblup_mt::py_random_donors(py_mt, py_index, pop, L, best, donors, fixed);
  return 0;
}

static int validate_de(int strategy, int64_t pop, int64_t L, const int32_t* donors, const int64_t* fixed, double cr,
                       const uint32_t* mt_key, const int32_t* mt_pos) {
  if (strategy != TBLUP_DE_RAND_1 && strategy != TBLUP_DE_CURRENT_TO_BEST_1)
    return fail(TBLUP_ERR_ARG, "unknown DE strategy");
  if (pop < 1 || pop > 65535 || L < 1 || L > ((int64_t)1 << 31)) return fail(TBLUP_ERR_ARG, "need 1 <= pop <= 65535, 1 <= L <= 2^31");
  if (!donors || !fixed || !mt_key || !mt_pos) return fail(TBLUP_ERR_ARG, "null donors/fixed/mt_key/mt_pos");
  if (*mt_pos < 0 || *mt_pos > 624) return fail(TBLUP_ERR_ARG, "mt_pos must be in [0, 624]");
  if (!(cr == cr)) return fail(TBLUP_ERR_ARG, "crossover rate is NaN");
  for (int64_t i = 0; i < 3 * pop; ++i)
    if (donors[i] < 0 || donors[i] >= pop) return fail(TBLUP_ERR_ARG, "donor index out of range");
  for (int64_t i = 0; i < pop; ++i)
    if (fixed[i] < 0 || fixed[i] >= L) return fail(TBLUP_ERR_ARG, "fixed crossover position out of range");
  return 0;
}

// the jump polynomials of (L, pop) on the device (kept until another shape is asked for)
static int de_upload_polys(tblup_ctx* c, int64_t L, int64_t pop, hipStream_t s) {
  if (c->de_L == L && c->de_pop == pop) return 0;
  const tblup_mt::DePolys dp = tblup_mt::de_polys(L, pop);
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (int rc = dev_alloc(c, c->de_polys, dp.words.size() * 4)) return rc;
  HIPCHK(hipMemcpy(c->de_polys.p, dp.words.data(), dp.words.size() * 4, hipMemcpyHostToDevice));
  c->de_L = L;
  c->de_pop = pop;
  c->de_end_jump = dp.end_jump;
  return 0;
}

// the copy of the new MT state to the host behind a step, and the event tblup_de_state_wait waits for
static int de_state_fetch(tblup_ctx* c, const void* d_state, hipStream_t s) {
  if (!c->de_host) HIPCHK(hipHostMalloc((void**)&c->de_host, 625 * 4, hipHostMallocDefault));
  if (!c->de_ev) HIPCHK(hipEventCreateWithFlags(&c->de_ev, hipEventDisableTiming));
  HIPCHK(hipMemcpyAsync(c->de_host, d_state, 624 * 4 + 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(c->de_ev, s));
  c->de_pending = true;
  return 0;
}

// smallest population the three-launch forms take (TBLUP_DE_SPLIT; default: more individuals than CUs)
static int64_t de_split_min() {
  static const int64_t v = getenv("TBLUP_DE_SPLIT") ? atoll(getenv("TBLUP_DE_SPLIT")) : cu_count() + 1;
  return v;
}

// What every entry that runs DE kernels on the context checks first.
static int de_enter(tblup_ctx* c) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (c->de_pending) return fail(TBLUP_ERR_STATE, "the previous DE step's state was not fetched (tblup_de_state_wait)");
  return 0;
}

// ... and what the two step entries check last, behind their own arguments (the reports keep their order)
static int check_de_rows(int64_t L, int64_t ld, int64_t ldc, const double* d_parents, const double* d_children) {
  if (ld < L || ldc < L) return fail(TBLUP_ERR_ARG, "ld/ldc < L");
  if (!d_parents || !d_children) return fail(TBLUP_ERR_ARG, "null device pointers");
  return 0;
}

// Byte layout of a step's per-call block, staged page-locked and copied to de_small in one piece:
// key in, key out, pos out, donors, fixed, then the arrays of pop elements that the form take()s.
struct DeStage {
  static constexpr size_t key_out = 624 * 4, pos_out = 2 * 624 * 4, donors = pos_out + 16;
  size_t fixed, end;
  char *dev = nullptr, *host = nullptr;   // de_stage_open
  explicit DeStage(int64_t pop) : fixed(donors + (size_t)round_up(12 * pop, 16)), end(fixed + 8 * (size_t)pop) {}
  size_t take(size_t bytes) {
    const size_t o = end;
    end += bytes;
    return o;
  }
};

// de_small of at least dev_bytes (the stream waits only when it grows) and the page-locked stage of
// st.end bytes, the common prefix in it and in the request; the caller adds its arrays to st.host and
// copies st.end bytes to st.dev.  The stage outlives the call (the copy is asynchronous); the previous
// call's copy from it finished before that call's state was fetched (one step pending at a time).
static int de_stage_open(tblup_ctx* c, DeStage& st, size_t dev_bytes, int64_t pop, const uint32_t* mt_key,
                         const int32_t* donors, const int64_t* fixed, DeArgs& a, hipStream_t s) {
  if (dev_bytes > c->de_small.bytes) {
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = dev_alloc(c, c->de_small, dev_bytes)) return rc;
  }
  if (st.end > c->de_stage_bytes) {
    HIPCHK(hipStreamSynchronize(s));
    if (c->de_stage) HIPCHK(hipHostFree(c->de_stage));
    c->de_stage = nullptr;
    c->de_stage_bytes = 0;
    HIPCHK(hipHostMalloc((void**)&c->de_stage, st.end, hipHostMallocDefault));
    c->de_stage_bytes = st.end;
  }
  st.dev = (char*)c->de_small.p;
  st.host = c->de_stage;
  std::memcpy(st.host, mt_key, 624 * 4);
  std::memcpy(st.host + st.donors, donors, 12 * pop);
  std::memcpy(st.host + st.fixed, fixed, 8 * pop);
  a.key = (const uint32_t*)st.dev;
  a.donors = (const int32_t*)(st.dev + st.donors);
  a.fixed = (const int64_t*)(st.dev + st.fixed);
  a.key_out = (uint32_t*)(st.dev + st.key_out);
  a.pos_out = (int32_t*)(st.dev + st.pos_out);
  a.polys = (const uint32_t*)c->de_polys.p;
  a.end_jump = c->de_end_jump ? 1 : 0;
  return 0;
}

// The asynchronous step.  strat_i / F_i / cr_i: host arrays of pop, all three (tblup_de_step_device_async_mix)
// or none (the scalars).
static int de_step_async(tblup_ctx* c, int strategy, const int32_t* strat_i, const double* F_i, const double* cr_i,
                         const double* d_parents, int64_t pop, int64_t L, int64_t ld, const int32_t* donors,
                         const int64_t* fixed, double F, double cr, int clip, double clip_hi, const uint32_t* mt_key,
                         int32_t mt_pos, double* d_children, int64_t ldc, void* stream) {
  if (int rc = de_enter(c)) return rc;
  DeArgs a = {};
  a.strategy = strategy, a.F = F, a.cr = cr;
  // With per-individual arrays no kernel reads the scalars: element 0 stands in them so that
  // validate_de sees something valid (read only for a non-empty population; it rejects pop < 1).
  if (strat_i) {
    const bool any = pop >= 1;
    a.strategy = any ? strat_i[0] : TBLUP_DE_RAND_1, a.F = any ? F_i[0] : 0.0, a.cr = any ? cr_i[0] : 0.0;
  }
  if (int rc = validate_de(a.strategy, pop, L, donors, fixed, a.cr, mt_key, &mt_pos)) return rc;
  for (int64_t i = 0; strat_i && i < pop; ++i)
    if (strat_i[i] != TBLUP_DE_RAND_1 && strat_i[i] != TBLUP_DE_CURRENT_TO_BEST_1)
      return fail(TBLUP_ERR_ARG, "unknown DE strategy");
  for (int64_t i = 0; cr_i && i < pop; ++i)
    if (!(cr_i[i] == cr_i[i])) return fail(TBLUP_ERR_ARG, "crossover rate is NaN");
  if (int rc = check_de_rows(L, ld, ldc, d_parents, d_children)) return rc;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (int rc = de_upload_polys(c, L, pop, s)) return rc;
  DeStage st(pop);
  const size_t o_str = st.take((size_t)round_up(4 * pop, 16)), o_F = st.take(8 * (size_t)pop),
               o_cr = st.take(8 * (size_t)pop);
  // device-only scratch of the three-launch form (large populations): base sequence + windows
  // (from more individuals than CUs: both forms need a second round of jump workgroups there, and the
  // split form's mask and stream run several per CU; TBLUP_DE_SPLIT = the smallest split population)
  const bool split = pop >= de_split_min();
  const size_t o_scr = (size_t)round_up((int64_t)st.end, 256);
  if (int rc = de_stage_open(c, st, split ? o_scr + 4 * (size_t)(DE_SEQ_SCRATCH + 624 * pop) : st.end, pop, mt_key,
                             donors, fixed, a, s))
    return rc;
  if (strat_i) {
    std::memcpy(st.host + o_str, strat_i, 4 * pop);
    std::memcpy(st.host + o_F, F_i, 8 * pop);
    std::memcpy(st.host + o_cr, cr_i, 8 * pop);
    a.strat_i = (const int32_t*)(st.dev + o_str);
    a.F_i = (const double*)(st.dev + o_F), a.cr_i = (const double*)(st.dev + o_cr);
  }
  HIPCHK(hipMemcpyAsync(st.dev, st.host, st.end, hipMemcpyHostToDevice, s));
  const tblup_mt::EndState e = tblup_mt::end_state(mt_pos, 2 * (uint64_t)L * (uint64_t)pop);
  a.pos0 = mt_pos, a.end_s = e.s, a.end_pos = e.pos;
  a.parent = d_parents, a.ldp = ld;
  a.child = d_children, a.ldc = ldc;
  a.clip = clip ? 1 : 0, a.hi = clip_hi;
  a.L = L, a.pop = (int)pop;
  HIPCHK(launch_de_step(a, split ? (uint32_t*)(st.dev + o_scr) : nullptr, s));
  return de_state_fetch(c, st.dev + st.key_out, s);
}

int tblup_de_step_device_async(tblup_ctx* c, int strategy, const double* d_parents, int64_t pop, int64_t L,
                               int64_t ld, const int32_t* donors, const int64_t* fixed, double F, double cr, int clip,
                               double clip_hi, const uint32_t* mt_key, int32_t mt_pos, double* d_children,
                               int64_t ldc, void* stream) {
  return de_step_async(c, strategy, nullptr, nullptr, nullptr, d_parents, pop, L, ld, donors, fixed, F, cr, clip,
                       clip_hi, mt_key, mt_pos, d_children, ldc, stream);
}

int tblup_de_step_device_async_mix(tblup_ctx* c, const int32_t* strategies, const double* F, const double* cr,
                                   const double* d_parents, int64_t pop, int64_t L, int64_t ld, const int32_t* donors,
                                   const int64_t* fixed, int clip, double clip_hi, const uint32_t* mt_key,
                                   int32_t mt_pos, double* d_children, int64_t ldc, void* stream) {
  if (!strategies || !F || !cr) {
    clear_error();
    return fail(TBLUP_ERR_ARG, "null strategies/F/cr");
  }
  return de_step_async(c, TBLUP_DE_RAND_1, strategies, F, cr, d_parents, pop, L, ld, donors, fixed, 0.0, 0.0, clip,
                       clip_hi, mt_key, mt_pos, d_children, ldc, stream);
}

int tblup_de_state_wait(tblup_ctx* c, uint32_t* mt_key, int32_t* mt_pos) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (!mt_key || !mt_pos) return fail(TBLUP_ERR_ARG, "null mt_key/mt_pos");
  if (!c->de_pending) return fail(TBLUP_ERR_STATE, "no DE step pending (tblup_de_step_device_async)");
  HIPCHK(hipSetDevice(c->device));
  c->de_pending = false;
  HIPCHK(hipEventSynchronize(c->de_ev));
  std::memcpy(mt_key, c->de_host, 624 * 4);
  std::memcpy(mt_pos, c->de_host + 624, 4);
  return 0;
}

int tblup_de_step_device(tblup_ctx* c, int strategy, const double* d_parents, int64_t pop, int64_t L, int64_t ld,
                         const int32_t* donors, const int64_t* fixed, double F, double cr, int clip, double clip_hi,
                         uint32_t* mt_key, int32_t* mt_pos, double* d_children, int64_t ldc, void* stream) {
  if (!mt_key || !mt_pos) {
    clear_error();
    return fail(TBLUP_ERR_ARG, "null donors/fixed/mt_key/mt_pos");
  }
  if (int rc = tblup_de_step_device_async(c, strategy, d_parents, pop, L, ld, donors, fixed, F, cr, clip, clip_hi,
                                          mt_key, *mt_pos, d_children, ldc, stream))
    return rc;
  return tblup_de_state_wait(c, mt_key, mt_pos);
}

int tblup_de_step(tblup_ctx* c, int strategy, const double* parents, int64_t pop, int64_t L, const int32_t* donors,
                  const int64_t* fixed, double F, double cr, int clip, double clip_hi, uint32_t* mt_key,
                  int32_t* mt_pos, double* children) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (int rc = validate_de(strategy, pop, L, donors, fixed, cr, mt_key, mt_pos)) return rc;
  if (!parents || !children) return fail(TBLUP_ERR_ARG, "null parents/children");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t bytes = (size_t)pop * L * 8;
  if (int rc = dev_alloc(c, c->de_par, bytes)) return rc;
  if (int rc = dev_alloc(c, c->de_chi, bytes)) return rc;
  HIPCHK(hipMemcpyAsync(c->de_par.p, parents, bytes, hipMemcpyHostToDevice, c->stream));
  if (int rc = tblup_de_step_device(c, strategy, (const double*)c->de_par.p, pop, L, L, donors, fixed, F, cr, clip,
                                    clip_hi, mt_key, mt_pos, (double*)c->de_chi.p, L, nullptr))
    return rc;
  HIPCHK(hipMemcpy(children, c->de_chi.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// ---- MDE_pBX generation (evolver.py:550-687): draws, host resolve, step ----

static const int64_t MDE_WORDS_MAX = (int64_t)1 << 26;   // draw words of one generation (256 MiB)

static int validate_mde_shape(int64_t pop, int64_t L, int64_t nq, int64_t np) {
  if (pop < 4 || pop > 65535 || L < 1 || L > ((int64_t)1 << 31))
    return fail(TBLUP_ERR_ARG, "need 4 <= pop <= 65535 and 1 <= L <= 2^31");
  if (nq < 1 || nq > pop || np < 1 || np > pop) return fail(TBLUP_ERR_ARG, "choice-array sizes must be in [1, pop]");
  return 0;
}

int tblup_mde_windows(int64_t pop, int64_t nq, int64_t np, int32_t slack, int32_t* lo, int32_t* hi, int64_t* off,
                      int64_t* n_words) {
  clear_error();
  if (int rc = validate_mde_shape(pop, 1, nq, np)) return rc;
  if (!n_words) return fail(TBLUP_ERR_ARG, "null n_words");
  *n_words = tblup_mt::mde_windows(pop, nq, np, slack, lo, hi, off);
  return 0;
}

int tblup_mde_draws(tblup_ctx* c, int64_t pop, int64_t L, int64_t nq, int64_t np, int32_t slack,
                    const uint32_t* mt_key, int32_t mt_pos, uint32_t* words, int64_t n_words, void* stream) {
  if (int rc = de_enter(c)) return rc;
  if (int rc = validate_mde_shape(pop, L, nq, np)) return rc;
  if (!mt_key || !words) return fail(TBLUP_ERR_ARG, "null mt_key/words");
  if (mt_pos < 0 || mt_pos > 624) return fail(TBLUP_ERR_ARG, "mt_pos must be in [0, 624]");
  std::vector<int32_t> lo((size_t)pop), hi((size_t)pop);
  std::vector<int64_t> off((size_t)pop + 1);
  const int64_t total = tblup_mt::mde_windows(pop, nq, np, slack, lo.data(), hi.data(), off.data());
  if (n_words != total) return fail(TBLUP_ERR_ARG, "n_words is not the size tblup_mde_windows gives");
  if (total > MDE_WORDS_MAX) return fail(TBLUP_ERR_ARG, "more than 2^26 draw words: keep this generation on the host");
  c->mde_key.clear();
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (int rc = de_upload_polys(c, L, pop, s)) return rc;
  const bool split = pop >= de_split_min();
  const size_t o_tab = 624 * 4, o_off = o_tab + (size_t)round_up(8 * pop, 16), o_words = o_off + 8 * (size_t)pop;
  const size_t o_scr = (size_t)round_up((int64_t)(o_words + 4 * (size_t)total), 256);
  const size_t need = split ? o_scr + 4 * (size_t)(DE_SEQ_SCRATCH + 624 * (pop + 1)) : o_scr;
  if (need > c->mde_dev.bytes) {
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = dev_alloc(c, c->mde_dev, need)) return rc;
  }
  char* base = (char*)c->mde_dev.p;
  std::vector<char> host(o_words);
  std::memcpy(host.data(), mt_key, 624 * 4);
  int32_t* tab = (int32_t*)(host.data() + o_tab);
  for (int64_t i = 0; i < pop; ++i) tab[2 * i] = lo[i], tab[2 * i + 1] = hi[i];
  std::memcpy(host.data() + o_off, off.data(), 8 * (size_t)pop);
  // `host` is pageable and local: the stream is synchronised below, before it goes away
  HIPCHK(hipMemcpyAsync(base, host.data(), o_words, hipMemcpyHostToDevice, s));
  DeArgs a = {};
  a.key = (const uint32_t*)base, a.pos0 = mt_pos, a.pop = (int)pop;
  a.polys = (const uint32_t*)c->de_polys.p, a.end_jump = c->de_end_jump ? 1 : 0;
  HIPCHK(launch_mde_draws(a, (const int32_t*)(base + o_tab), (const int64_t*)(base + o_off),
                          (uint32_t*)(base + o_words), split ? (uint32_t*)(base + o_scr) : nullptr, s));
  if (total > 0) HIPCHK(hipMemcpyAsync(words, base + o_words, 4 * (size_t)total, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->mde_key.assign(mt_key, mt_key + 624);
  c->mde_pos = mt_pos;
  c->mde_pop = pop;
  c->mde_L = L;
  c->mde_scr = split ? (int64_t)o_scr : 0;
  c->mde_cmax = hi[(size_t)pop - 1];
  return 0;
}

int tblup_mde_resolve(int64_t pop, int64_t L, const int32_t* q_best, int64_t nq, const int32_t* p_best, int64_t np,
                      int32_t slack, const uint32_t* words, int64_t n_words, uint32_t* py_mt, int32_t* py_index,
                      int32_t* parent, int32_t* donors, int64_t* fixed, int64_t* c_words, int32_t* overflow) {
  clear_error();
  if (int rc = validate_mde_shape(pop, 1, nq, np)) return rc;
  if (L < 1 || L >= ((int64_t)1 << 32)) return fail(TBLUP_ERR_ARG, "need 1 <= L < 2^32");
  if (!q_best || !p_best || !words || !py_mt || !py_index || !parent || !donors || !fixed || !c_words || !overflow)
    return fail(TBLUP_ERR_ARG, "null argument");
  if (*py_index < 0 || *py_index > 624) return fail(TBLUP_ERR_ARG, "py_index must be in [0, 624]");
  for (int64_t k = 0; k < nq; ++k)
    if (q_best[k] < 0 || q_best[k] >= pop) return fail(TBLUP_ERR_ARG, "best index out of range");
  for (int64_t k = 0; k < np; ++k)
    if (p_best[k] < 0 || p_best[k] >= pop) return fail(TBLUP_ERR_ARG, "parent index out of range");
  if (n_words != tblup_mt::mde_windows(pop, nq, np, slack, nullptr, nullptr, nullptr))
    return fail(TBLUP_ERR_ARG, "n_words is not the size tblup_mde_windows gives");
  *overflow = tblup_mt::mde_resolve(pop, L, q_best, nq, p_best, np, slack, words, py_mt, py_index, parent, donors,
                                    fixed, c_words)
                  ? 0
                  : 1;
  return 0;
}

int tblup_mde_step_device_async(tblup_ctx* c, const double* F, const double* cr, const double* d_parents, int64_t pop,
                                int64_t L, int64_t ld, const int32_t* parent, const int32_t* donors,
                                const int64_t* fixed, const int64_t* c_words, int clip, double clip_hi,
                                const uint32_t* mt_key, int32_t mt_pos, double* d_children, int64_t ldc, void* stream) {
  if (int rc = de_enter(c)) return rc;
  if (!F || !cr || !parent || !c_words) return fail(TBLUP_ERR_ARG, "null F/cr/parent/c_words");
  if (pop < 4) return fail(TBLUP_ERR_ARG, "need 4 <= pop <= 65535 and 1 <= L <= 2^31");
  if (int rc = validate_de(TBLUP_DE_CURRENT_TO_BEST_1, pop, L, donors, fixed, 0.0, mt_key, &mt_pos)) return rc;
  for (int64_t i = 0; i < pop; ++i) {
    if (!(cr[i] == cr[i])) return fail(TBLUP_ERR_ARG, "crossover rate is NaN");
    if (parent[i] < 0 || parent[i] >= pop) return fail(TBLUP_ERR_ARG, "parent index out of range");
    if (c_words[i] < (i ? c_words[i - 1] : 0)) return fail(TBLUP_ERR_ARG, "c_words must be non-negative and non-decreasing");
  }
  if (int rc = check_de_rows(L, ld, ldc, d_parents, d_children)) return rc;
  if (c->mde_key.empty() || c->mde_pop != pop || c->mde_L != L || c->mde_pos != mt_pos || c->de_pop != pop ||
      c->de_L != L || std::memcmp(c->mde_key.data(), mt_key, 624 * 4) != 0)
    return fail(TBLUP_ERR_STATE, "no tblup_mde_draws of this population, length and MT state to continue");
  // every workgroup walks c_words / 624 blocks forward: no more than the draws' windows can give
  if (c_words[pop - 1] > c->mde_cmax) return fail(TBLUP_ERR_ARG, "c_words exceeds the windows of tblup_mde_draws");
  c->mde_key.clear();   // the draws are used up, whatever happens below
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  DeStage st(pop);   // + F, cr, the uniforms' window offsets, targets
  const size_t o_F = st.take(8 * (size_t)pop), o_cr = st.take(8 * (size_t)pop), o_f = st.take(8 * (size_t)pop),
               o_tgt = st.take(4 * (size_t)pop);
  DeArgs a = {};
  if (int rc = de_stage_open(c, st, st.end, pop, mt_key, donors, fixed, a, s)) return rc;
  std::memcpy(st.host + o_F, F, 8 * pop);
  std::memcpy(st.host + o_cr, cr, 8 * pop);
  int64_t* f_i = (int64_t*)(st.host + o_f);
  for (int64_t i = 0; i < pop; ++i) f_i[i] = c_words[i] + (i ? 2 : 0);   // windows 1.. start two words early
  std::memcpy(st.host + o_tgt, parent, 4 * pop);
  HIPCHK(hipMemcpyAsync(st.dev, st.host, st.end, hipMemcpyHostToDevice, s));
  // numpy's state after 2 L pop + C_pop words, counted from where the end window starts
  const uint64_t fixed_words = 2 * (uint64_t)L * (uint64_t)pop;
  const tblup_mt::EndState e = tblup_mt::end_state(mt_pos, fixed_words + (uint64_t)c_words[pop - 1]);
  const uint64_t o_win = c->de_end_jump ? (uint64_t)mt_pos + fixed_words - 625 : 0;
  a.pos0 = mt_pos, a.end_s = (int)((uint64_t)e.s + e.o_rel - o_win), a.end_pos = e.pos;
  a.parent = d_parents, a.ldp = ld;
  a.child = d_children, a.ldc = ldc;
  a.clip = clip ? 1 : 0, a.hi = clip_hi;
  a.L = L, a.pop = (int)pop;
  a.F_i = (const double*)(st.dev + o_F), a.cr_i = (const double*)(st.dev + o_cr);
  a.f_i = (const int64_t*)(st.dev + o_f), a.target_i = (const int32_t*)(st.dev + o_tgt);
  HIPCHK(launch_mde_step(a, c->mde_scr ? (uint32_t*)((char*)c->mde_dev.p + c->mde_scr) : nullptr, s));
  return de_state_fetch(c, st.dev + st.key_out, s);
}

int tblup_gather_rows(tblup_ctx* c, double* d_dst, int64_t n, int64_t L, int64_t ldd, const double* const* d_src_rows,
                      void* stream) {
  clear_error();
  if (int rc = check_ctx(c)) return rc;
  if (n < 0 || L < 0 || ldd < L) return fail(TBLUP_ERR_ARG, "need n >= 0, 0 <= L <= ldd");
  if (n == 0 || L == 0) return 0;
  if (!d_dst || !d_src_rows) return fail(TBLUP_ERR_ARG, "null destination / source table");
  for (int64_t i = 0; i < n; ++i)
    if (!d_src_rows[i]) return fail(TBLUP_ERR_ARG, "null source row");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  for (int64_t r0 = 0; r0 < n; r0 += ROWPTRS) {
    const int nr = (int)std::min<int64_t>(ROWPTRS, n - r0);
    RowPtrs t{};
    for (int k = 0; k < nr; ++k) t.p[k] = d_src_rows[r0 + k];
    HIPCHK(launch_gather_rows(d_dst + r0 * ldd, ldd, L, t, nr, s));
  }
  return 0;
}

int tblup_host_register(void* ptr, int64_t bytes) {
  clear_error();
  if (!ptr || bytes <= 0) return fail(TBLUP_ERR_ARG, "null pointer or non-positive size");
  HIPCHK(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault));
  return 0;
}

int tblup_host_unregister(void* ptr) {
  clear_error();
  if (!ptr) return fail(TBLUP_ERR_ARG, "null pointer");
  HIPCHK(hipHostUnregister(ptr));
  return 0;
}

}  // extern "C"
