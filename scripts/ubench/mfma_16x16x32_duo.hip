// Micro-benchmark: can K2b's stage (rk4_forward_bf16x3: one wave per SIMD, 96 v_mfma_f32_32x32x16_bf16 and ~390 vector
// instructions that depend on them and feed the next stage's MFMAs) be shortened by cutting the wave's 32 series into two
// groups of 16 that run half a stage apart in one instruction stream -- each group's field on v_mfma_f32_16x16x32_bf16, its
// contraction / 3/8-rule update / operand split issued in the gaps of the OTHER group's MFMAs?  Two streams are timed:
//   shape A (K2b as it is): per iteration four tile pairs of 24 MFMAs 32x32x16 (two accumulators of 16 registers, twelve
//           dependent products each, SrcA in AGPRs), each pair followed by its contraction with dX (2 v_mul + 30 v_fma in
//           four 8-long chains, reading the pair's accumulators), then the tail: update (72), bookkeeping (102 v_add / v_mul),
//           the three-piece split of 16 values (88: 24 v_cvt_pk_bf16_f32, 32 v_sub, 16 shifts, 16 ands) whose pieces are the
//           next iteration's B operands.  96 MFMAs + 390 vector instructions, one dependency chain.
//   shape B (the proposal): per iteration two phases.  A phase is 96 MFMAs 16x16x32 of one group (16 accumulator tiles of 4
//           registers, six dependent products each, SrcA in AGPRs, B = that group's pieces) and the other group's 176 vector
//           instructions (contraction 64, update 36, split of 8 values 44, bookkeeping 32: the same mix), PER_GAP of them
//           behind every MFMA until they are used up.  They read that group's accumulators of the previous phase and write
//           the pieces its MFMAs read in the next.  192 MFMAs + 352 vector instructions.
// MFMA time is 96 x 32 = 192 x 16 = 3,072 cycles in both.  MODE 0: as described; 1: the MFMAs alone; 2 (shape B): the same
// instructions with the interleave off, a phase's vector block behind its MFMAs; 3: the vector instructions alone.
// One workgroup of four waves per CU (the LDS request sees to it), one wave per SIMD.  The MFMAs are builtins and the vector
// instructions plain C++, one instruction per statement, each behind a scheduling barrier: the order is the source's, the
// wait states are the compiler's (s_nop 10 between a tile pair's last MFMA and its contraction in shape A; shape B reads an
// accumulator tile no sooner than 24 MFMAs after its last write and needs none).  Adjacent statements are independent
// wherever the work allows (chains interleaved in pairs, split levels across the pairs), as a scheduler would lay them out.
// First product of every accumulator takes C = 0 (the kernel's bias reads from LDS are not part of either stream).
// Build (K2b's flag; no fused, packed or re-vectorised forms of what is written here; check the loops with --save-temps):
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form -mllvm -disable-vector-combine -ffp-contract=off
//         -fno-slp-vectorize scripts/ubench/mfma_16x16x32_duo.hip -o scripts/ubench/mfma_16x16x32_duo
// As compiled: shape A's loop 96 MFMAs + 390 vector instructions + 4 s_nop 10, longest bare MFMA run 24; shape B's 192 + 352
// + 6 s_nop, "MFMA, vector, vector" 88 times per phase and 8 bare MFMAs at its end; SrcA of every MFMA in a[..]; 143 / 194
// VGPRs + 192 AGPRs, no scratch.
// Output: s_memtime ticks per iteration, mean over workgroups of first start .. last end.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <type_traits>
#include <vector>
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// a loop whose index is a constant in the body, whatever the unroller thinks of its size
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

constexpr int IMG = 48;                      // the weight image: 48 uint4 per lane, 192 AGPRs, in both shapes

// One vector instruction each, in plain C++ behind a scheduling barrier (as inline asm every statement that reads its
// neighbour's result gets an s_nop 0 in front on gfx950 -- ~95 per stream here, which the kernels do not carry)
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
#define VSTEP(expr) do { expr; __builtin_amdgcn_sched_barrier(0); } while (0)
__device__ __forceinline__ void v_mul(float& d, float a, float b) { VSTEP(d = a * b); }
__device__ __forceinline__ void v_add(float& d, float a, float b) { VSTEP(d = a + b); }
__device__ __forceinline__ void v_sub(float& d, float a, float b) { VSTEP(d = a - b); }
__device__ __forceinline__ void v_fma(float& d, float a, float b) { VSTEP(d = __builtin_fmaf(a, b, d)); }
__device__ __forceinline__ void v_fma3(float& d, float a, float b, float c) { VSTEP(d = __builtin_fmaf(a, b, c)); }
__device__ __forceinline__ void v_cvt(unsigned& d, float a, float b) {
  VSTEP(d = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2)));
}
__device__ __forceinline__ void v_shl(float& d, unsigned u) { VSTEP(d = __uint_as_float(u << 16)); }
__device__ __forceinline__ void v_and(float& d, unsigned u) { VSTEP(d = __uint_as_float(u & 0xffff0000u)); }

// the six piece products of a tile, smallest first: a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1 (0-based piece indices)
__host__ __device__ constexpr int piece_a(int p) { return p == 0 ? 2 : (p == 1 || p == 3) ? 1 : 0; }
__host__ __device__ constexpr int piece_b(int p) { return p == 0 ? 0 : p == 1 ? 1 : p == 2 ? 2 : p == 3 ? 0 : p == 4 ? 1 : 0; }

// the MFMAs: builtins between scheduling barriers
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
__device__ __forceinline__ void mfma16(bool first, f32x4& acc, const u32x4& a, const u32x4& b) {
  __builtin_amdgcn_sched_barrier(0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                first ? f32x4{0.f, 0.f, 0.f, 0.f} : acc, 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void mfma32(bool first, f32x16& acc, const u32x4& a, const u32x4& b) {
  f32x16 zero;
  for (int e = 0; e < 16; ++e) zero[e] = 0.f;
  __builtin_amdgcn_sched_barrier(0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), first ? zero : acc, 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
}

// level-by-level three-piece split of NP pairs (x[2 i], x[2 i + 1]) into pc[piece][i]; step j of 11 NP
// (get / set: a piece's dword e -- a vector element cannot be bound to a reference)
template <int NP, typename Get, typename Set>
__device__ __forceinline__ void split_step(int j, const float* x, float* r0, float* r1, float* h0, float* h1, Get get, Set set) {
  unsigned d;
  if (j < NP) { v_cvt(d, x[2 * j], x[2 * j + 1]); set(0, j, d); return; }
  const int level = (j - NP) / (5 * NP), q = (j - NP) % (5 * NP);
  if (q < NP) v_shl(h0[q], get(level, q));
  else if (q < 2 * NP) v_and(h1[q - NP], get(level, q - NP));
  else if (q < 4 * NP) {
    const int p = (q - 2 * NP) >> 1, odd = (q - 2 * NP) & 1;
    if (odd) v_sub(r1[p], level == 0 ? x[2 * p + 1] : r1[p], h1[p]);
    else v_sub(r0[p], level == 0 ? x[2 * p] : r0[p], h0[p]);
  } else { v_cvt(d, r0[q - 4 * NP], r1[q - 4 * NP]); set(level + 1, q - 4 * NP, d); }
}

// update, NU units, step j: four levels across the units (v_mul, v_sub, v_fma, v_add), then `extra` v_mul of bookkeeping
template <int NU>
__device__ __forceinline__ void update_step(int j, float* x, float* k, float* f, float* m, float dt, float third) {
  const int level = j / NU, u = j % NU;
  if (level == 0) v_mul(f[u], f[u], third);
  else if (level == 1) v_sub(f[u], k[u], f[u]);
  else if (level == 2) v_fma3(x[u], dt, f[u], k[u]);
  else if (level == 3) v_add(k[u], k[u], f[u]);
  else v_mul(m[u & 3], m[u & 3], third);
}
__device__ __forceinline__ void misc_step(int j, float* m, float dt, float third) {
  if (j % 8 < 5) v_add(m[j & 3], m[j & 3], dt);
  else v_mul(m[j & 3], m[j & 3], third);
}

// ------------------------------------------------------------------------------------------------ shape B: one group
struct Grp {
  f32x4 acc[16];
  float x[8], k[8], f[8], r0[4], r1[4], h0[4], h1[4], m[4];
  u32x4 pc[3];
};
constexpr int DUO_V = 64 + 36 + 44 + 32;     // 176 vector instructions per group and stage

__device__ __forceinline__ void duo_vstep(int i, Grp& s, const float (&dX)[8], float dt, float third) {
  if (i < 64) {                              // contraction: unit m's channels 0..3 in tile 2 m, 4..7 in tile 2 m + 1; two chains at a time
    const int j = i & 15, c = j >> 1, m = 2 * (i >> 4) + (j & 1);
    const float a = s.acc[2 * m + (c >> 2)][c & 3];
    if (c == 0) v_mul(s.f[m], a, dX[0]);
    else v_fma(s.f[m], a, dX[c]);
  } else if (i < 100) update_step<8>(i - 64, s.x, s.k, s.f, s.m, dt, third);
  else if (i < 144) split_step<4>(i - 100, s.x, s.r0, s.r1, s.h0, s.h1, [&](int p, int e) { return s.pc[p][e]; },
                                 [&](int p, int e, unsigned d) { s.pc[p][e] = d; });
  else if (i < DUO_V) misc_step(i - 144, s.m, dt, third);
}

template <int MODE, int PER_GAP>
__device__ __forceinline__ void duo_phase(Grp& mg, Grp& vg, const u32x4 (&w)[IMG], const float (&dX)[8], float dt, float third) {
  if constexpr (MODE == 3) {                                   // (nobody writes them in this mode)
#pragma unroll
    for (int t = 0; t < 16; ++t) asm volatile("" : "+v"(vg.acc[t]));
  }
  static_for<0, 96>([&](auto S) {                               // tile pair tp, product p, tile u of the pair
    constexpr int slot = S(), tp = slot / 12, p = (slot % 12) / 2, u = slot & 1, t = 2 * tp + u;
    if constexpr (MODE != 3) mfma16(p == 0, mg.acc[t], w[t * 3 + piece_a(p)], mg.pc[piece_b(p)]);
    if constexpr (MODE == 1 && p == 5) asm volatile("" : "+v"(mg.acc[t]));     // (nobody reads it in this mode)
    if constexpr (MODE == 0 || MODE == 3)
      static_for<0, PER_GAP>([&](auto E) {
        if constexpr (slot * PER_GAP + E() < DUO_V) duo_vstep(slot * PER_GAP + E(), vg, dX, dt, third);
      });
  });
  if constexpr (MODE == 3) asm volatile("" :: "v"(vg.pc[0]), "v"(vg.pc[1]), "v"(vg.pc[2]));   // (no MFMA reads them in this mode)
  if constexpr (MODE == 2) static_for<0, DUO_V>([&](auto I) { duo_vstep(I(), vg, dX, dt, third); });
}

// ------------------------------------------------------------------------------------------------ shape A
struct One {
  f32x16 acc[2];
  float x[16], k[16], f[16], r0[8], r1[8], h0[8], h1[8], m[4];
  u32x4 pc[2][3];
};
constexpr int ONE_TAIL = 72 + 102 + 88;      // + 4 x 32 of contraction = 390

template <int MODE>
__device__ __forceinline__ void one_stage(One& s, const u32x4 (&w)[IMG], const float (&dX)[8], float dt, float third) {
  static_for<0, 4>([&](auto TP) {
    constexpr int tp = TP();
    if constexpr (MODE != 3)
      static_for<0, 24>([&](auto S) {                           // K step ks, product p, tile u of the pair
        constexpr int ks = S() / 12, p = (S() % 12) / 2, u = S() & 1;
        mfma32(ks == 0 && p == 0, s.acc[u], w[((2 * tp + u) * 2 + ks) * 3 + piece_a(p)], s.pc[ks][piece_b(p)]);
        if constexpr (MODE == 1 && ks == 1 && p == 5) asm volatile("" : "+v"(s.acc[u]));     // (nobody reads it in this mode)
      });
    if constexpr (MODE != 1) {
      if constexpr (MODE == 3) asm volatile("" : "+v"(s.acc[0]), "+v"(s.acc[1]));   // (nobody writes them in this mode)
      static_for<0, 32>([&](auto S) {                           // registers 2 c, 2 c + 1: the tile's two units at channel c
        constexpr int u = S() / 16, j = S() % 16, c = j >> 1, unit = 2 * (2 * tp + u) + (j & 1);
        if constexpr (c == 0) v_mul(s.f[unit], s.acc[u][j], dX[0]);
        else v_fma(s.f[unit], s.acc[u][j], dX[c]);
      });
    }
  });
  if constexpr (MODE != 1)
    static_for<0, ONE_TAIL>([&](auto I) {
      constexpr int i = I();
      if constexpr (i < 72) update_step<16>(i, s.x, s.k, s.f, s.m, dt, third);
      else if constexpr (i < 174) misc_step(i - 72, s.m, dt, third);
      else split_step<8>(i - 174, s.x, s.r0, s.r1, s.h0, s.h1, [&](int p, int e) { return s.pc[e >> 2][p][e & 3]; },
                         [&](int p, int e, unsigned d) { s.pc[e >> 2][p][e & 3] = d; });
    });
  if constexpr (MODE == 3) {                                    // (no MFMA reads them in this mode)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) asm volatile("" :: "v"(s.pc[ks][0]), "v"(s.pc[ks][1]), "v"(s.pc[ks][2]));
  }
}

// ------------------------------------------------------------------------------------------------ kernel
template <int SHAPE, int MODE, int PER_GAP>
__global__ __launch_bounds__(256, 1) void k(float* out, long long* span, int iters, float seed) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x == 0) lds[0] = seed;
  u32x4 w[IMG];
#pragma unroll
  for (int i = 0; i < IMG; ++i) {
    for (int e = 0; e < 4; ++e) w[i][e] = 0x3c003c00u + 0x00010001u * ((lane + 5 * i + e) & 63);
    asm volatile("" : "+a"(w[i]));
  }
  float dX[8];
  for (int c = 0; c < 8; ++c) dX[c] = seed * 0.01f * (c + 1);
  const float dt = seed * 1e-3f, third = (float)(1.0 / 3.0);
  float r = 0.f;
  __syncthreads();
  const long long t0 = __builtin_amdgcn_s_memtime();
  if constexpr (SHAPE == 0) {
    One s;
    for (int u = 0; u < 2; ++u)
      for (int e = 0; e < 16; ++e) s.acc[u][e] = 0.f;
    for (int i = 0; i < 16; ++i) { s.x[i] = seed + 0.01f * (i + lane); s.k[i] = 0.f; s.f[i] = 0.f; }
    for (int i = 0; i < 8; ++i) { s.r0[i] = 0.f; s.r1[i] = 0.f; s.h0[i] = 0.f; s.h1[i] = 0.f; }
    for (int i = 0; i < 4; ++i) s.m[i] = seed + i;
    for (int ks = 0; ks < 2; ++ks)
      for (int p = 0; p < 3; ++p)
        for (int e = 0; e < 4; ++e) s.pc[ks][p][e] = (0x3f803f80u >> (8 * p)) + ks + lane;
    for (int it = 0; it < iters; ++it) one_stage<MODE>(s, w, dX, dt, third);
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    for (int i = 0; i < 16; ++i) r += s.x[i] + s.k[i] + s.f[i] + s.acc[0][i] + s.acc[1][i];
    for (int i = 0; i < 4; ++i) r += s.m[i];
  } else {
    Grp g[2];
    for (int gi = 0; gi < 2; ++gi) {
      Grp& s = g[gi];
      for (int t = 0; t < 16; ++t)
        for (int e = 0; e < 4; ++e) s.acc[t][e] = 0.f;
      for (int i = 0; i < 8; ++i) { s.x[i] = seed + 0.01f * (i + lane + 8 * gi); s.k[i] = 0.f; s.f[i] = 0.f; }
      for (int i = 0; i < 4; ++i) { s.r0[i] = 0.f; s.r1[i] = 0.f; s.h0[i] = 0.f; s.h1[i] = 0.f; s.m[i] = seed + i; }
      for (int p = 0; p < 3; ++p)
        for (int e = 0; e < 4; ++e) s.pc[p][e] = (0x3f803f80u >> (8 * p)) + gi + lane;
    }
    for (int it = 0; it < iters; ++it) {
      duo_phase<MODE, PER_GAP>(g[0], g[1], w, dX, dt, third);     // [M_A(s) || V_B(s)]
      duo_phase<MODE, PER_GAP>(g[1], g[0], w, dX, dt, third);     // [M_B(s + 1) || V_A(s)]
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    for (int gi = 0; gi < 2; ++gi) {
      for (int i = 0; i < 8; ++i) r += g[gi].x[i] + g[gi].k[i] + g[gi].f[i];
      for (int t = 0; t < 16; ++t) r += g[gi].acc[t][t & 3];
      for (int i = 0; i < 4; ++i) r += g[gi].m[i];
    }
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  out[blockIdx.x * 256 + threadIdx.x] = r + lds[0];
  if (lane == 0) { span[(blockIdx.x * 4 + wave) * 2] = t0; span[(blockIdx.x * 4 + wave) * 2 + 1] = t1; }
}

constexpr int BLOCKS = 256;
constexpr size_t LDS_BYTES = 96 * 1024;      // more than half of a CU's 160 KB: one workgroup per CU

template <int SHAPE, int MODE, int PER_GAP>
static double run(int iters) {
  float* out; long long* span;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k<SHAPE, MODE, PER_GAP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)LDS_BYTES) != hipSuccess) return -1;
  if (hipMalloc(&out, BLOCKS * 256 * sizeof(float)) != hipSuccess) return -1;
  if (hipMalloc(&span, BLOCKS * 8 * sizeof(long long)) != hipSuccess) return -1;
  (void)hipMemset(span, 0, BLOCKS * 8 * sizeof(long long));
  k<SHAPE, MODE, PER_GAP><<<BLOCKS, 256, LDS_BYTES>>>(out, span, 10, 1.0f);
  k<SHAPE, MODE, PER_GAP><<<BLOCKS, 256, LDS_BYTES>>>(out, span, iters, 1.0f);
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  std::vector<long long> h(BLOCKS * 8);
  (void)hipMemcpy(h.data(), span, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
  (void)hipFree(out); (void)hipFree(span);
  double sum = 0;
  for (int b = 0; b < BLOCKS; ++b) {
    long long lo = h[b * 8], hi = h[b * 8 + 1];
    for (int wv = 0; wv < 4; ++wv) {
      lo = h[b * 8 + 2 * wv] < lo ? h[b * 8 + 2 * wv] : lo;
      hi = h[b * 8 + 2 * wv + 1] > hi ? h[b * 8 + 2 * wv + 1] : hi;
    }
    sum += (double)(hi - lo);
  }
  return sum / BLOCKS / iters;
}

template <int SHAPE, int MODE, int PER_GAP>
static double row(const char* what, int iters) {
  const double a = run<SHAPE, MODE, PER_GAP>(iters), again = run<SHAPE, MODE, PER_GAP>(iters);
  printf("%-92s %8.1f  (repeat %8.1f)\n", what, a, again);
  return a < again ? again : a;
}

int main() {
  const int iters = 1000;
  printf("s_memtime ticks per iteration (= one stage of 32 series per wave); one wave per SIMD, 256 workgroups, %d iterations\n", iters);
  const double a = row<0, 0, 0>("(a) K2b's shape: 96 MFMA 32x32x16 + 390 dependent vector instructions", iters);
  row<0, 1, 0>("(a) its 96 MFMAs alone", iters);
  row<0, 3, 0>("(a) its 390 vector instructions alone", iters);
  const double b = row<1, 0, 2>("(b) two groups: 2 x [96 MFMA 16x16x32 || 176 vector instructions of the other group], 2 per gap", iters);
  row<1, 1, 2>("(b) its 192 MFMAs alone", iters);
  row<1, 3, 2>("(b) its 352 vector instructions alone", iters);
  row<1, 2, 2>("(b) interleave off: each phase's 176 vector instructions behind its 96 MFMAs", iters);
  row<1, 0, 3>("(b) 3 per gap (59 gaps filled, 37 bare)", iters);
  row<1, 0, 4>("(b) 4 per gap (44 gaps filled, 52 bare)", iters);
  printf("(b) / (a) = %.3f (the slower of each pair of launches); go at <= 0.85\n", b / a);
  return 0;
}
