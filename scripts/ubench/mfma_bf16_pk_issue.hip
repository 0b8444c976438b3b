// Micro-benchmark: what does PACKED f32 (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32) cost beside bf16 MFMAs on gfx950 when the
// SIMD is ISSUE-bound, not MFMA-bound?  mfma_bf16_fill.hip asked it with 48 MFMAs per iteration and the fillers squeezed
// into their gaps (the matrix pipe was the limit, and packed f32 did not hide).  K3p's bf16 form is the opposite case: two
// waves per SIMD issue ~3,000 instructions per stage between them, and the 195 MFMAs of a stage keep the matrix pipe busy
// less than half of that time.  A packed instruction does two FMAs in one issue slot; this file measures whether the slot
// it saves is worth the pipe time it takes, in that kernel's shape:
//   wave A (waves 0..3, the chain's shape): 33 rows of three dependent v_mfma_f32_32x32x16_bf16, issued one row ahead of the
//           row's consume as the kernel issues them (issue Jo, consume Je, issue Je, consume Jo); a consume is 32 FMAs --
//           16 into four partial sums (p0, p1, q0, q1), 16 into the vs accumulators -- or, packed, 16 v_pk_fma_f32 on the
//           adjacent register pairs (the second operand of the vs half broadcast by op_sel).  PK_ROWS of the 32 consumed
//           rows take the packed form, spread evenly: 0 -> 1,024 scalar; 8 -> 768 + 128 packed; 16 -> 512 + 256; 32 -> 512 packed;
//   wave B (waves 4..7, the helper's shape): 16 blocks of six dependent MFMAs (eight accumulators, 96 MFMAs) behind 75
//           non-packed vector instructions each (8 v_mul, an 8-long v_fma chain, 12 v_cvt_pk_bf16_f32, 16 v_sub, 8 shifts,
//           8 ands, 15 v_add: the products, the dL/db chain and the three-piece splits; 1,200 per iteration).
//           B_FORM 1: the 8 v_mul as 4 v_pk_mul_f32; B_FORM 2: also the 16 v_sub as 8 v_pk_add_f32 with a negated operand.
// Both waves meet in one s_barrier per iteration (the stage barrier).  One workgroup per CU (the LDS request sees to it), so
// every SIMD holds exactly one A and one B wave.  All arithmetic is inline asm: the compiler neither packs nor reorders it.
// As compiled, B's loop is 1,606 / 1,544 / 1,416 instructions in forms 0 / 1 / 2 and A's 1,298 / 1,170 / 1,042 / 786: only the
// named instructions change, the packed operands sit in aligned pairs without copies (two or three v_mov_b64 per iteration
// in every form), and the compiler's s_nop 0 between adjacent dependent asm statements are the same in every form (301, 164).
// Output: s_memtime ticks per iteration, mean over workgroups of first start .. last end, each role alone and both together.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

struct ChainState {
  f32x2 y[8], vs[8], p, q;
};

__device__ __forceinline__ void issue_row(f32x16& J, const u32x4& m0, const u32x4& m1, const u32x4& m2, const u32x4& b01,
                                          const u32x4& b2) {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 1\n\t"
               "v_mfma_f32_32x32x16_bf16 %0, %3, %5, 0\n\t"
               "v_mfma_f32_32x32x16_bf16 %0, %2, %4, %0\n\t"
               "v_mfma_f32_32x32x16_bf16 %0, %1, %4, %0"
               : "=&v"(J) : "v"(m0), "v"(m1), "v"(m2), "v"(b01), "v"(b2));
  __builtin_amdgcn_sched_barrier(0);
}

// (`packed` is a constant once the row loop is unrolled)
__device__ __forceinline__ void consume_row(bool packed, const f32x16& J, float ah, ChainState& s) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (packed) {
      const f32x2 Jp = {J[2 * j], J[2 * j + 1]};
      const f32x2 ah2 = {ah, ah};
      if (j & 1) asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(s.q) : "v"(Jp), "v"(s.y[j]));
      else asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(s.p) : "v"(Jp), "v"(s.y[j]));
      asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(s.vs[j]) : "v"(Jp), "v"(ah2));
    } else {
      f32x2& acc = (j & 1) ? s.q : s.p;
      asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[0]) : "v"(J[2 * j]), "v"(s.y[j][0]));
      asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(acc[1]) : "v"(J[2 * j + 1]), "v"(s.y[j][1]));
      asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(s.vs[j][0]) : "v"(J[2 * j]), "v"(ah));
      asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(s.vs[j][1]) : "v"(J[2 * j + 1]), "v"(ah));
    }
  }
}

// consumed row number i of 32: packed when it is one of the PK_ROWS evenly spread ones
template <int PK_ROWS>
__host__ __device__ constexpr bool row_packed(int i) { return PK_ROWS > 0 && i % (32 / (PK_ROWS > 0 ? PK_ROWS : 1)) == 0; }

template <int B_FORM>
__device__ __forceinline__ void helper_block(f32x16& acc, float (&x)[16], unsigned (&u)[12], float& chain, const u32x4& pa,
                                             const u32x4& pb, float fa) {
  // products
  if constexpr (B_FORM >= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x2 r;
      asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(f32x2{x[2 * i], x[2 * i + 1]}), "v"(f32x2{fa, fa}));
      x[8 + 2 * i] = r[0]; x[8 + 2 * i + 1] = r[1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("v_mul_f32 %0, %1, %2" : "=v"(x[8 + i]) : "v"(x[i]), "v"(fa));
  }
  // the dL/db chain (one dependent chain) and the three-piece splits of the four product pairs -- cvt, then twice (shift,
  // and, 2 sub, cvt) -- level by level across the pairs, as a scheduler would lay the independent pairs out
  float r0[4], r1[4];
  unsigned h0[4], h1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r0[i] = x[8 + 2 * i]; r1[i] = x[8 + 2 * i + 1];
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u[3 * i]) : "v"(r0[i]), "v"(r1[i]));
    asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(chain) : "v"(x[i]), "v"(fa));
  }
#pragma unroll
  for (int level = 0; level < 2; ++level) {
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(h0[i]) : "v"(u[3 * i + level]));
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(h1[i]) : "v"(u[3 * i + level]));
#pragma unroll
    for (int i = 0; i < 2; ++i) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(chain) : "v"(x[4 + 2 * level + i]), "v"(fa));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (B_FORM >= 2) {
        f32x2 r;
        asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]"
                     : "=v"(r) : "v"(f32x2{r0[i], r1[i]}), "v"(f32x2{__uint_as_float(h0[i]), __uint_as_float(h1[i])}));
        r0[i] = r[0]; r1[i] = r[1];
      } else {
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(r0[i]) : "v"(r0[i]), "v"(__uint_as_float(h0[i])));
        asm volatile("v_sub_f32 %0, %1, %2" : "=v"(r1[i]) : "v"(r1[i]), "v"(__uint_as_float(h1[i])));
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(u[3 * i + level + 1]) : "v"(r0[i]), "v"(r1[i]));
  }
  // bookkeeping
#pragma unroll
  for (int i = 0; i < 15; ++i) asm volatile("v_add_f32 %0, %1, %0" : "+v"(x[i & 7]) : "v"(fa));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int m = 0; m < 6; ++m) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(pa), "v"(pb));
  __builtin_amdgcn_sched_barrier(0);
}

// what: bit 0 = wave A works, bit 1 = wave B works (an idle role still meets the barrier)
template <int PK_ROWS, int B_FORM>
__global__ __launch_bounds__(512) void k(float* out, long long* span, int iters, float seed, int what) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x == 0) lds[0] = seed;
  u32x4 pa, pb;
  for (int e = 0; e < 4; ++e) { pa[e] = 0x3f803f80u + lane; pb[e] = 0x3c003c00u + e; }
  float r = 0.f;
  __syncthreads();
  const long long t0 = __builtin_amdgcn_s_memtime();
  if (wave < 4) {
    ChainState s;
    for (int j = 0; j < 8; ++j) { s.y[j] = f32x2{seed + j, seed - j}; s.vs[j] = f32x2{0.f, 0.f}; }
    s.p = f32x2{0.f, 0.f}; s.q = f32x2{0.f, 0.f};
    const float ah = seed * 1e-3f;
    const bool work = what & 1;
    for (int it = 0; it < iters; ++it) {
      if (work) {
        f32x16 Je, Jo;
        issue_row(Je, pa, pb, pa, pb, pa);
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          issue_row(Jo, pa, pb, pa, pb, pa);
          asm volatile("" : "+v"(Je));
          consume_row(row_packed<PK_ROWS>(2 * rr), Je, ah, s);
          issue_row(Je, pa, pb, pa, pb, pa);
          asm volatile("" : "+v"(Jo));
          consume_row(row_packed<PK_ROWS>(2 * rr + 1), Jo, ah, s);
        }
        asm volatile("s_nop 15\n\ts_nop 7" : "+v"(Je));
        s.p[0] += Je[0];
      }
      asm volatile("s_barrier" ::: "memory");
    }
    r = s.p[0] + s.p[1] + s.q[0] + s.q[1];
    for (int j = 0; j < 8; ++j) r += s.vs[j][0] + s.vs[j][1];
  } else {
    f32x16 acc[8];
    for (int c = 0; c < 8; ++c)
      for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
    float x[16], chain = 0.f;
    unsigned u[12];
    for (int i = 0; i < 16; ++i) x[i] = seed + i + lane;
    for (int i = 0; i < 12; ++i) u[i] = 0;
    const float fa = 1.0001f;
    const bool work = what & 2;
    for (int it = 0; it < iters; ++it) {
      if (work) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
#pragma unroll
          for (int c = 0; c < 8; ++c) helper_block<B_FORM>(acc[c], x, u, chain, pa, pb, fa);
        }
      }
      asm volatile("s_barrier" ::: "memory");
    }
    r = chain;
    for (int c = 0; c < 8; ++c) r += acc[c][c];
    for (int i = 0; i < 16; ++i) r += x[i];
    for (int i = 0; i < 12; ++i) r += __uint_as_float(u[i]);
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  const long long t1 = __builtin_amdgcn_s_memtime();
  out[blockIdx.x * 512 + threadIdx.x] = r + lds[0];
  if (lane == 0) { span[(blockIdx.x * 8 + wave) * 2] = t0; span[(blockIdx.x * 8 + wave) * 2 + 1] = t1; }
}

constexpr int BLOCKS = 256;
constexpr size_t LDS_BYTES = 96 * 1024;      // more than half of a CU's 160 KB: one workgroup per CU

template <int PK_ROWS, int B_FORM>
static double run(int what, int iters) {
  float* out; long long* span;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k<PK_ROWS, B_FORM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)LDS_BYTES) != hipSuccess) return -1;
  if (hipMalloc(&out, BLOCKS * 512 * sizeof(float)) != hipSuccess) return -1;
  if (hipMalloc(&span, BLOCKS * 16 * sizeof(long long)) != hipSuccess) return -1;
  hipMemset(span, 0, BLOCKS * 16 * sizeof(long long));
  k<PK_ROWS, B_FORM><<<BLOCKS, 512, LDS_BYTES>>>(out, span, 10, 1.0f, what);
  k<PK_ROWS, B_FORM><<<BLOCKS, 512, LDS_BYTES>>>(out, span, iters, 1.0f, what);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  std::vector<long long> h(BLOCKS * 16);
  hipMemcpy(h.data(), span, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
  hipFree(out); hipFree(span);
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

template <int PK_ROWS, int B_FORM>
static void row(int iters) {
  const double a = run<PK_ROWS, B_FORM>(1, iters), b = run<PK_ROWS, B_FORM>(2, iters), both = run<PK_ROWS, B_FORM>(3, iters);
  const double again = run<PK_ROWS, B_FORM>(3, iters);
  printf("A: %4d v_fma_f32 + %3d v_pk_fma_f32 | B form %d | A alone %8.1f | B alone %8.1f | both %8.1f  (repeat %8.1f)\n",
         (32 - PK_ROWS) * 32, PK_ROWS * 16, B_FORM, a, b, both, again);
}

template <int B_FORM>
static void rows(int iters) {
  row<0, B_FORM>(iters);
  row<8, B_FORM>(iters);
  row<16, B_FORM>(iters);
  row<32, B_FORM>(iters);
}

int main() {
  const int iters = 1000;
  printf("s_memtime ticks per iteration; A: 99 v_mfma_f32_32x32x16_bf16 in 33 dependent groups of three + the FMAs of 32 row "
         "consumes; B: 96 MFMAs + 16 x 75 vector instructions\n"
         "B form 0: non-packed; 1: 128 v_mul_f32 as 64 v_pk_mul_f32; 2: also 256 v_sub_f32 as 128 v_pk_add_f32\n");
  rows<0>(iters);
  rows<1>(iters);
  rows<2>(iters);
  return 0;
}
