// Occupancy microbenchmark of the off-diagonal GEMM1 loop (k_chol.hip gemm1_a32: 32-row Lt_J stages
// through a 2 x 32 KiB LDS-DMA ring, each wave's Lt_I columns straight into registers): how fast does
// ONE 8-wave workgroup alone on a CU run it, against two per CU (production), and against one
// 16-wave workgroup whose waves split the tile's row blocks (wave w: columns 16 (w & 7), row blocks
// 4 (w >> 3) .. +3)?
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-sched-strategy=max-ilp -I tblup_amd/csrc
//         tools/occ_bench.hip -o tools/occ_bench          (k_chol.hip's scheduler option, csrc/Makefile)
//   tools/occ_bench [nL]   -> one JSON line per variant (TFLOP/s over the launch, fp64); the *_pin
//   rows run the production form of the stage loop's waits, the others the form before it; then one
//   JSON line per traced launch (shader-clock cycles per stage in the wait, the barrier and the body)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tblup_internal.h"

using namespace tblup;

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int TT = TILE * TILE;

__device__ __forceinline__ v4d mfma64_nega(double a, double b, v4d c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 1);
}
__device__ __forceinline__ int lt_off(int k, int x) { return k * TILE + 2 * ((x >> 1) ^ (8 * (k & 1))) + (x & 1); }

// PIN: the stage loop as gemm1_a32 has it now (top wait vmcnt(8): only the LDS-DMA ops; B loads
// unconditional and pinned behind their k-step); !PIN: the earlier form (top wait vmcnt(0), B loads
// under `if (more)`: the compiler's waits drain the prefetch within the stage), kept to measure against
//
// TRACE: lane 0 of every wave stamps the shader clock (s_memtime) three times per stage -- before the
// stage's wait, after it, after the barrier -- into its own LDS row past the ring (tr; an LDS write
// is no vector-memory op, so the counted waits see the queue they see without it).
template <int NW, int NCB, bool PIN, bool TRACE = false>
__device__ __forceinline__ void gemm1(const double* __restrict__ ltJ, const double* __restrict__ ltI, int nL, double* lds,
                                      v4d (&acc)[NCB], uint64_t* tr = nullptr) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wc = w & 7, cb0 = (w >> 3) * NCB;
  constexpr int AS = 32 * TILE;
  constexpr int RPW = 32 / NW;   // stage rows issued per wave
  const int nst = 4 * nL;
  auto src_of = [&](int s) { return (int64_t)(s >> 2) * TT + (s & 3) * AS; };
  auto issue_a = [&](int s) {
    double* slot = lds + (s & 1) * AS;
    const int64_t src = src_of(s);
#pragma unroll
    for (int e = 0; e < RPW; ++e) {
      const int k = RPW * w + e;
      glds16_asm(ltJ + src + k * TILE + 2 * (l ^ (8 * (k & 1))), slot + k * TILE);
    }
  };
  const double* bcol = ltI + 16 * wc + (l & 15) + (l >> 4) * TILE;
  double bc[8];
  issue_a(0);
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) bc[kk] = bcol[4 * kk * TILE];
  for (int s = 0; s < nst; ++s) {
    if (TRACE && l == 0) tr[3 * s] = __builtin_readcyclecounter();
    if (PIN)   // queue: A(s) x RPW, B(s) x 8
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (TRACE && l == 0) tr[3 * s + 1] = __builtin_readcyclecounter();
    __builtin_amdgcn_s_barrier();
    if (TRACE && l == 0) tr[3 * s + 2] = __builtin_readcyclecounter();
    const bool more = s + 1 < nst;
    if (more) issue_a(s + 1);
    const double* bs = bcol + src_of(more ? s + 1 : s);
    const double* As = lds + (s & 1) * AS;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + (l >> 4);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma64_nega(As[lt_off(k, 16 * (cb0 + cb) + (l & 15))], bc[kk], acc[cb]);
      if (PIN) {
        __builtin_amdgcn_sched_barrier(0);
        bc[kk] = bs[4 * kk * TILE];
        __builtin_amdgcn_sched_barrier(0);
      } else if (more) {
        bc[kk] = bs[4 * kk * TILE];
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// T-unit pair: 8 waves, one workgroup per CU (256 VGPRs), wave w holds the 16 columns w of TWO tiles
// (Lt_I and Lt_I2 in registers) against one shared Lt_J stage: 16 MFMAs per 8 LDS A reads
__device__ __forceinline__ void gemm1_pair(const double* __restrict__ ltJ, const double* __restrict__ ltI,
                                           const double* __restrict__ ltI2, int nL, double* lds, v4d (&acc)[8],
                                           v4d (&acc2)[8]) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int AS = 32 * TILE;
  const int nst = 4 * nL;
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
  const double* bcol2 = ltI2 + 16 * w + (l & 15) + (l >> 4) * TILE;
  double bc[8], bd[8];
  issue_a(0);
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    bc[kk] = bcol[4 * kk * TILE];
    bd[kk] = bcol2[4 * kk * TILE];
  }
  for (int s = 0; s < nst; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more = s + 1 < nst;
    if (more) issue_a(s + 1);
    const int64_t so = src_of(more ? s + 1 : s);
    const double* As = lds + (s & 1) * AS;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + (l >> 4);
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        const double a = As[lt_off(k, 16 * cb + (l & 15))];
        acc[cb] = mfma64_nega(a, bc[kk], acc[cb]);
        acc2[cb] = mfma64_nega(a, bd[kk], acc2[cb]);
      }
      if (more) {
        bc[kk] = bcol[so + 4 * kk * TILE];
        bd[kk] = bcol2[so + 4 * kk * TILE];
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

__global__ __launch_bounds__(512, 1) void k_pair(const double* L, int rows, int nL, double* out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  v4d acc[8], acc2[8];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) acc[cb] = acc2[cb] = v4d{0.0, 0.0, 0.0, 0.0};
  const int g = blockIdx.x;
  const double* ltJ = L + (int64_t)(g % rows) * 8 * TT;
  const double* ltI = L + (int64_t)((g * 7 + 3) % rows) * 8 * TT;
  const double* ltI2 = L + (int64_t)((g * 11 + 5) % rows) * 8 * TT;
  gemm1_pair(ltJ, ltI, ltI2, nL, lds, acc, acc2);
  double s = 0.0;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) s += acc[cb][0] + acc[cb][1] + acc[cb][2] + acc[cb][3] + acc2[cb][0] + acc2[cb][3];
  if (s == 12345.678) out[g] = s;
}

// every workgroup: GEMM1 of nL terms for one tile, rows of 8 tiles in L (row r = tiles r*8 .. r*8+7)
template <int NW, int NCB, int MINB, bool PIN>
__global__ __launch_bounds__(64 * NW, MINB) void k_bench(const double* L, int rows, int nL, double* out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  v4d acc[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) acc[cb] = v4d{0.0, 0.0, 0.0, 0.0};
  const int g = blockIdx.x;
  const double* ltJ = L + (int64_t)(g % rows) * 8 * TT;
  const double* ltI = L + (int64_t)((g * 7 + 3) % rows) * 8 * TT;
  gemm1<NW, NCB, PIN>(ltJ, ltI, nL, lds, acc);
  double s = 0.0;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) s += acc[cb][0] + acc[cb][1] + acc[cb][2] + acc[cb][3];
  if (s == 12345.678) out[g] = s;
}

// The stage loop traced: workgroup tb copies its waves' stamps (8 x 3 x 4 nL) to tro
constexpr int TRACE_MAX_STAGES = 64;
template <bool PIN>
__global__ __launch_bounds__(512, 4) void k_trace(const double* L, int rows, int nL, double* out, int tb, uint64_t* tro) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  v4d acc[8];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) acc[cb] = v4d{0.0, 0.0, 0.0, 0.0};
  const int g = blockIdx.x, w = threadIdx.x >> 6;
  uint64_t* tr = reinterpret_cast<uint64_t*>(lds + 2 * 32 * TILE) + w * 3 * TRACE_MAX_STAGES;
  const double* ltJ = L + (int64_t)(g % rows) * 8 * TT;
  const double* ltI = L + (int64_t)((g * 7 + 3) % rows) * 8 * TT;
  gemm1<8, 8, PIN, true>(ltJ, ltI, nL, lds, acc, tr);
  if (g == tb && (threadIdx.x & 63) == 0)
    for (int i = 0; i < 12 * nL; ++i) tro[w * 3 * TRACE_MAX_STAGES + i] = tr[i];
  double s = 0.0;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb) s += acc[cb][0] + acc[cb][1] + acc[cb][2] + acc[cb][3];
  if (s == 12345.678) out[g] = s;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s\n", hipGetErrorString(e_)); exit(1); } } while (0)

template <int NW, int NCB, int MINB, bool PIN = false>
void run(const char* name, const double* L, int rows, int nL, int grid, size_t lds_bytes, double* out) {
  auto k = k_bench<NW, NCB, MINB, PIN>;
  CK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k, dim3(grid), dim3(64 * NW), lds_bytes, 0, L, rows, nL, out);
  CK(hipDeviceSynchronize());
  const int reps = 10;
  CK(hipEventRecord(a));
  for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k, dim3(grid), dim3(64 * NW), lds_bytes, 0, L, rows, nL, out);
  CK(hipEventRecord(b));
  CK(hipEventSynchronize(b));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, a, b));
  const double tiles = (double)grid * (NW == 16 ? 1.0 : 1.0);
  const double flops = tiles * nL * 2.0 * 128.0 * 128.0 * 128.0 * reps;
  printf("{\"variant\": \"%s\", \"grid\": %d, \"lds_kb\": %zu, \"nL\": %d, \"ms_per_launch\": %.4f, \"tflops\": %.2f}\n", name,
         grid, lds_bytes / 1024, nL, ms / reps, flops / (ms * 1e-3) / 1e12);
}

void run_pair(const double* L, int rows, int nL, int grid, double* out) {
  const size_t lds_bytes = 64 * 1024;
  CK(hipFuncSetAttribute((const void*)k_pair, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_pair, dim3(grid), dim3(512), lds_bytes, 0, L, rows, nL, out);
  CK(hipDeviceSynchronize());
  const int reps = 10;
  CK(hipEventRecord(a));
  for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_pair, dim3(grid), dim3(512), lds_bytes, 0, L, rows, nL, out);
  CK(hipEventRecord(b));
  CK(hipEventSynchronize(b));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, a, b));
  const double flops = 2.0 * grid * nL * 2.0 * 128.0 * 128.0 * 128.0 * reps;
  printf("{\"variant\": \"w8_pair_one_per_cu\", \"grid\": %d, \"nL\": %d, \"ms_per_launch\": %.4f, \"tflops\": %.2f}\n", grid,
         nL, ms / reps, flops / (ms * 1e-3) / 1e12);
}

// One traced launch (after a warm-up launch): per stage s >= 1 of workgroup tb, averaged over its 8
// waves, the shader-clock cycles in the stage's wait, in its barrier, and from the barrier to the
// next stage's top (the body: LDS-DMA issue, 64 MFMAs, 8 B loads and the compiler's waits on them).
template <bool PIN>
void run_trace(const char* name, const double* L, int rows, int nL, int grid, int tb, double* out) {
  const size_t lds_bytes = 64 * 1024 + 8 * 3 * TRACE_MAX_STAGES * 8;
  const int nst = 4 * nL;
  if (nst > TRACE_MAX_STAGES) return;
  auto k = k_trace<PIN>;
  CK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  uint64_t* tro;
  CK(hipMalloc(&tro, 8 * 3 * TRACE_MAX_STAGES * 8));
  for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(k, dim3(grid), dim3(512), lds_bytes, 0, L, rows, nL, out, tb, tro);
  CK(hipDeviceSynchronize());
  std::vector<uint64_t> h(8 * 3 * TRACE_MAX_STAGES);
  CK(hipMemcpy(h.data(), tro, h.size() * 8, hipMemcpyDeviceToHost));
  double wait = 0, bar = 0, body = 0, wait_max = 0;
  int n = 0;
  for (int w = 0; w < 8; ++w)
    for (int s = 1; s + 1 < nst; ++s) {
      const uint64_t* r = h.data() + w * 3 * TRACE_MAX_STAGES + 3 * s;
      wait += (double)(r[1] - r[0]);
      bar += (double)(r[2] - r[1]);
      body += (double)(r[3] - r[2]);
      if ((double)(r[1] - r[0]) > wait_max) wait_max = (double)(r[1] - r[0]);
      ++n;
    }
  printf("{\"trace\": \"%s\", \"grid\": %d, \"workgroup\": %d, \"nL\": %d, \"stages\": %d, \"wait_cycles\": %.0f, "
         "\"wait_max_cycles\": %.0f, \"barrier_cycles\": %.0f, \"body_cycles\": %.0f}\n",
         name, grid, tb, nL, n, wait / n, wait_max, bar / n, body / n);
  CK(hipFree(tro));
}

int main(int argc, char** argv) {
  const int nL = argc > 1 ? atoi(argv[1]) : 6;
  const int rows = 512;   // 512 x 8 tiles x 128 KiB = 512 MiB of Lt tiles (beyond the MALL: HBM-served)
  double *L, *out;
  CK(hipMalloc(&L, (size_t)rows * 8 * TT * 8));
  CK(hipMalloc(&out, 1 << 20));
  std::vector<double> h((size_t)8 * TT);
  for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3 * (double)((i * 2654435761u) % 1000);
  for (int r = 0; r < rows; ++r) CK(hipMemcpy(L + (size_t)r * 8 * TT, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  const size_t base = 64 * 1024;   // the 2 x 32 KiB ring
  for (int rounds : {1, 4}) {
    // production: 8 waves, 72 KiB-class LDS, two workgroups per CU when the grid allows
    run<8, 8, 4>("w8_two_per_cu", L, rows, nL, 512 * rounds, base, out);
    run<8, 8, 4, true>("w8_two_per_cu_pin", L, rows, nL, 512 * rounds, base, out);
    // one 8-wave workgroup per CU (LDS beyond half the CU)
    run<8, 8, 4>("w8_one_per_cu", L, rows, nL, 256 * rounds, 96 * 1024, out);
    // one 16-wave workgroup per CU: waves split the row blocks (4 per wave)
    run<16, 4, 1>("w16_one_per_cu", L, rows, nL, 256 * rounds, base, out);
    run<16, 4, 1>("w16_lds96", L, rows, nL, 256 * rounds, 96 * 1024, out);
    run_pair(L, rows, nL, 256 * rounds, out);
  }
  // L2-resident operands (an individual's Lt rows shared by its tiles): 8 rows only
  for (int rounds : {4}) {
    run<8, 8, 4>("w8_two_per_cu_l2", L, 8, nL, 512 * rounds, base, out);
    run<8, 8, 4, true>("w8_two_per_cu_l2_pin", L, 8, nL, 512 * rounds, base, out);
    run<16, 4, 1>("w16_one_per_cu_l2", L, 8, nL, 256 * rounds, base, out);
    run_pair(L, 8, nL, 256 * rounds, out);
  }
  // stage-boundary trace of one workgroup of the third round (its CU shared with another), both forms
  run_trace<false>("w8_two_per_cu", L, rows, nL, 2048, 1200, out);
  run_trace<true>("w8_two_per_cu_pin", L, rows, nL, 2048, 1200, out);
  run_trace<false>("w8_two_per_cu_l2", L, 8, nL, 2048, 1200, out);
  run_trace<true>("w8_two_per_cu_l2_pin", L, 8, nL, 2048, 1200, out);
  return 0;
}
