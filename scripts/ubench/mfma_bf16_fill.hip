// Micro-benchmark: do NON-packed vector instructions hide under v_mfma_f32_32x32x16_bf16 on gfx950 -- issued by the same
// wave between its MFMAs, or by the other wave of the SIMD (the chain / helper pairing of K3p)?  mfma_overlap.hip asked the
// same with v_pk_fma_f32 and f32 MFMAs as the partner and found the sum; packed f32 is the case the platform documents as
// not hiding, so this file measures the non-packed instructions the bf16 kernels issue: v_fma_f32, v_add_f32,
// v_cvt_pk_bf16_f32, v_permlane32_swap, ds_read_b128 (and v_pk_fma_f32 for contrast).
//
// 512-thread workgroups, 256 of them; waves 0..3 and 4..7 share SIMDs pairwise.  Per iteration role A issues 48 bf16 MFMAs
// (four independent accumulators).  Modes (ticks of s_memtime = shader cycles, per iteration, mean over workgroups of
// first start .. last end):
//   same wave : waves 0..3 issue F fillers after every MFMA (waves 4..7 idle)      vs  the MFMAs alone and the fillers alone
//   two waves : waves 0..3 the MFMAs, waves 4..7 the 48 F fillers as one stream   vs  each role alone
// Fillers are inline asm (the compiler neither packs nor reorders them) and independent of each other and of the MFMAs.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

enum { FMA = 0, ADD, CVT, PERM, DSR, PKFMA, NKIND };
static const char* kind_name[NKIND] = {"v_fma_f32", "v_add_f32", "v_cvt_pk_bf16_f32", "v_permlane32_swap", "ds_read_b128",
                                       "v_pk_fma_f32"};

struct Fill {
  float x[8];
  f32x2 p[4];
  unsigned u[8];
  u32x4 q[4];
};

// filler number j (0..7 rotating destinations)
template <int KIND>
__device__ __forceinline__ void filler(Fill& s, int j, float a, float b, const void* lds_addr) {
  if constexpr (KIND == FMA) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(s.x[j]) : "v"(a), "v"(b));
  else if constexpr (KIND == ADD) asm volatile("v_add_f32 %0, %1, %0" : "+v"(s.x[j]) : "v"(a));
  else if constexpr (KIND == CVT) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(s.u[j]) : "v"(s.x[j]), "v"(b));
  else if constexpr (KIND == PERM) asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(s.x[j]), "+v"(s.x[(j + 1) & 7]));
  else if constexpr (KIND == DSR) {
    // four destinations; the read that last wrote q[j & 3] (four reads ago) must be done
    asm volatile("s_waitcnt lgkmcnt(3)\n\tds_read_b128 %0, %1" : "=v"(s.q[j & 3]) : "v"((unsigned)(uintptr_t)lds_addr) : "memory");
  } else asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(s.p[j & 3]) : "v"(f32x2{a, b}), "v"(f32x2{b, a}));
}

// what: bit 0 = MFMAs in waves 0..3, bit 1 = fillers in waves 4..7 (48 F per iteration), bit 2 = F fillers after each MFMA
// in waves 0..3 (the fillers alone when bit 0 is clear)
template <int KIND, int F>
__global__ __launch_bounds__(512) void k(float* out, long long* span, int iters, float seed, int what) {
  __shared__ __attribute__((aligned(16))) float lds[64 * 4 * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e = threadIdx.x; e < 64 * 4 * 8; e += 512) lds[e] = seed * e;
  const void* my_lds = lds + (wave & 7) * 256 + lane * 4;
  const bool roleA = wave < 4;
  bf16x8 pa, pb;
  for (int e = 0; e < 8; ++e) { pa[e] = (__bf16)(seed * (lane + e)); pb[e] = (__bf16)(seed + e); }
  f32x16 c0, c1, c2, c3;
  for (int r = 0; r < 16; ++r) { c0[r] = 0.f; c1[r] = 0.f; c2[r] = 0.f; c3[r] = 0.f; }
  Fill s;
  for (int i = 0; i < 8; ++i) { s.x[i] = seed + i + lane; s.u[i] = 0; }
  for (int i = 0; i < 4; ++i) { s.p[i] = f32x2{seed + i, seed - i}; s.q[i] = u32x4{0u, 0u, 0u, 0u}; }
  const float fa = 1.0001f, fb = seed * lane;
  __syncthreads();
  const long long t0 = __builtin_amdgcn_s_memtime();
  if (roleA && (what & 5)) {
    const bool mf = what & 1, fill = what & 4;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 12; ++i) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          if (mf) {
            f32x16& c = m == 0 ? c0 : m == 1 ? c1 : m == 2 ? c2 : c3;
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, pb, c, 0, 0, 0);
          }
          if (fill) {
#pragma unroll
            for (int j = 0; j < F; ++j) filler<KIND>(s, (4 * m + j) & 7, fa, fb, my_lds);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  if (!roleA && (what & 2)) {
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int i = 0; i < 48 * F; ++i) filler<KIND>(s, i & 7, fa, fb, my_lds);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
  const long long t1 = __builtin_amdgcn_s_memtime();
  float r = c0[0] + c1[1] + c2[2] + c3[3];
  for (int i = 0; i < 8; ++i) r += s.x[i] + __uint_as_float(s.u[i]);
  for (int i = 0; i < 4; ++i) r += s.p[i][0] + s.p[i][1] + __uint_as_float(s.q[i][0] ^ s.q[i][3]);
  out[blockIdx.x * 512 + threadIdx.x] = r;
  if (lane == 0) { span[(blockIdx.x * 8 + wave) * 2] = t0; span[(blockIdx.x * 8 + wave) * 2 + 1] = t1; }
}

constexpr int BLOCKS = 256;

template <int KIND, int F>
static double run(int what, int iters) {
  float* out; long long* span;
  if (hipMalloc(&out, BLOCKS * 512 * sizeof(float)) != hipSuccess) return -1;
  if (hipMalloc(&span, BLOCKS * 16 * sizeof(long long)) != hipSuccess) return -1;
  hipMemset(span, 0, BLOCKS * 16 * sizeof(long long));
  k<KIND, F><<<BLOCKS, 512>>>(out, span, 10, 1.0f, what);
  k<KIND, F><<<BLOCKS, 512>>>(out, span, iters, 1.0f, what);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  std::vector<long long> h(BLOCKS * 16);
  hipMemcpy(h.data(), span, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
  hipFree(out); hipFree(span);
  // waves that did nothing still stamp; the span of a workgroup covers all eight
  double sum = 0;
  for (int b = 0; b < BLOCKS; ++b) {
    long long lo = h[b * 16], hi = h[b * 16 + 1];
    for (int w = 0; w < 8; ++w) {
      lo = h[b * 16 + 2 * w] < lo ? h[b * 16 + 2 * w] : lo;
      hi = h[b * 16 + 2 * w + 1] > hi ? h[b * 16 + 2 * w + 1] : hi;
    }
    sum += (double)(hi - lo);
  }
  return sum / BLOCKS / iters;
}

template <int KIND, int F>
static void row(int iters) {
  const double a = run<KIND, F>(1, iters);
  const double same_fill = run<KIND, F>(4, iters), same = run<KIND, F>(5, iters);
  const double pair_fill = run<KIND, F>(2, iters), pair = run<KIND, F>(3, iters);
  printf("%-18s F=%d | MFMAs alone %7.1f | same wave: fillers alone %7.1f  both %7.1f  (+%5.1f%% over MFMAs, %5.1f per filler)"
         " | two waves: fillers alone %7.1f  both %7.1f  (+%5.1f%%)\n",
         kind_name[KIND], F, a, same_fill, same, 100.0 * (same - a) / a, (same - a) / (48.0 * F), pair_fill, pair,
         100.0 * (pair - a) / a);
}

template <int KIND>
static void kind_rows(int iters) {
  row<KIND, 2>(iters);
  row<KIND, 4>(iters);
  row<KIND, 6>(iters);
  row<KIND, 8>(iters);
}

int main() {
  const int iters = 1000;
  printf("s_memtime ticks per iteration of 48 x v_mfma_f32_32x32x16_bf16; F fillers per MFMA gap\n");
  kind_rows<FMA>(iters);
  kind_rows<ADD>(iters);
  kind_rows<CVT>(iters);
  kind_rows<PERM>(iters);
  kind_rows<DSR>(iters);
  kind_rows<PKFMA>(iters);
  return 0;
}
