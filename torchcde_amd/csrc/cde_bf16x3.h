// cde_bf16x3.h -- what K2b (rk4_bf16x3.hip) and K3b (rk4_bf16x3_adjoint.hip) share: the exact three-piece bf16 operand
// split, the weight images in LDS, and the field / vjp evaluations on the bf16 matrix pipe.  The field evaluation has two
// forms that compute the same values through the same MFMAs: bx_field reads the weight pieces from the LDS image in every
// stage (K3b: its accumulators live in AGPRs, so it has no registers to spare and is built without -amdgpu-mfma-vgpr-form);
// bx_load_resident + bx_field_resident keep them in AGPRs for the whole solve (K2b: one wave per SIMD, AGPRs otherwise empty).
//
// Idea ("bf16x3").  gfx950 has no xf32 / TF32 mode; its exact-f32 MFMA runs at the vector rate, 1/16 of the bf16 rate
// (MI355X_MICROARCH.md).  A float32 value splits exactly into three bf16 pieces x = x1 + x2 + x3 (8 + 8 + 8 mantissa
// bits), and a product a b is recovered to ~2^-24 relative from the six piece products a_i b_j with i + j <= 4, each a
// v_mfma_f32_32x32x16_bf16 accumulating in float32 (smallest terms first).  Six bf16 MFMAs of 32 cycles replace eight
// f32 MFMAs of 64-66 cycles per 32 x 32 x 16 block: 2.7x less matrix-pipe time.  scripts/ubench/bf16x3_gemm.hip measured
// it in isolation (profiles/r03_bf16x3_ubench.txt): 3381 against 8393 cycles per evaluation INCLUDING the operand split,
// error 1.45e-7 of max|Y| against the f32 MFMA's 1.94e-7.
//
// What makes the split cheap here is the PRE-ACTIVATION form of the field (the one the tanh kernels use):
//     f_h = sum_c (W z + b)_(h,c) dX_c          the GEMM's B operand is the state z itself: 16 values per lane and stage,
// not the 264 products z_m dX_c of K2 / K3's product form.  Likewise for the adjoint
//     (a^T df/dz)_k = sum_c dX_c (W_c^T a)_k    eight 32 x 32 blocks W_c, B operand = a: 16 values per lane and stage.
// The weight pieces are split ONCE per launch into LDS images.  The third GEMM of the adjoint, dL/dW += (a (x) dX)^T z,
// stays on the exact-f32 pipe as in K3: its 256-row operand changes every stage and splitting it (128 values per lane)
// costs what the bf16 MFMAs save.
//
// Ownership = K3's: one wave owns 32 series for the whole solve, lane (n = l & 31, half = l >> 5) keeps hidden units
// 2 r + half (r = 0..15) in registers.  Tilings are chosen so that nothing ever moves between lanes:
//   MFMA K index kappa = 16 ks + 8 half + e  <->  unit 2 (8 ks + e) + half : the lane's own register 8 ks + e
//   Y tile t (4 units x 8 channels), row rho = 8 g + 4 hf + e  <->  unit 4 t + 2 (e & 1) + hf, channel 2 g + (e >> 1) :
//       D register r of lane (n, half) = Y[unit 4 t + 2 (r & 1) + half][channel r >> 1] -- both of the lane's units of the
//       tile with all their channels: f_(2(2t)+half), f_(2(2t+1)+half) are two in-lane dot products with dX.  The two
//       units sit in ADJACENT registers (2 c, 2 c + 1), so the pair that one packed FMA multiplies by dX_c needs no gather
//   W_c^T tile (channel c), row rho = 8 g + 4 hf + e  <->  output unit 2 (4 g + e) + hf : D register r = output unit 2 r + half
#pragma once
#include "cde_mfma.h"

namespace cde {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int BX_IMG_PER_LANE = 8 * 2 * 3;                // one lane's uint4 entries of a piece image
constexpr int BX_IMG_U4 = BX_IMG_PER_LANE * 64;           // uint4 entries of one piece image: [tile 8][ks 2][piece 3][lane 64]
constexpr int BX_BIAS_FLOATS = 8 * 2 * 16;                // [tile][half][register]
constexpr int BX_FWD_LDS_BYTES = BX_IMG_U4 * 16 + BX_BIAS_FLOATS * 4;
constexpr int BX_ADJ_LDS_BYTES = 2 * BX_IMG_U4 * 16 + BX_BIAS_FLOATS * 4 + 4 * SCR_FLOATS * 4;

__device__ __forceinline__ void bx_wave_lds_sync() {           // rk4_mfma.hip: wave_lds_sync
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void bx_split3(float x, __bf16& a, __bf16& b, __bf16& c) {
  a = (__bf16)x;
  const float r1 = x - (float)a;
  b = (__bf16)r1;
  const float r2 = r1 - (float)b;
  c = (__bf16)r2;
}

// the three pieces of 8 consecutive registers as MFMA B operands
__device__ __forceinline__ void bx_split8(const f32x16& v, int base, bf16x8 (&p)[3]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    __bf16 a, b, c;
    bx_split3(v[base + e], a, b, c);
    p[0][e] = a; p[1][e] = b; p[2][e] = c;
  }
}

// images into LDS: `which` 0 = Y tiles (rows (unit, channel), K = input unit), 1 = W_c^T tiles (rows = output unit, K = unit)
__device__ __forceinline__ void bx_stage_image(const float* __restrict__ W, u32x4* img, int which, Dims d, int tid, int nthreads) {
  for (int e4 = tid; e4 < BX_IMG_U4; e4 += nthreads) {
    const int l = e4 & 63, piece = (e4 >> 6) % 3, tk = (e4 >> 6) / 3, ks = tk & 1, t = tk >> 1;
    const int rho = l & 31, hfA = l >> 5;
    const int g = rho >> 3, hf = (rho >> 2) & 1, ee = rho & 3;
    bf16x8 out;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int uin = 2 * (8 * ks + e) + hfA;                     // the unit K index kappa = 16 ks + 8 hfA + e stands for
      float w;
      if (which == 0) {
        const int uo = 4 * t + 2 * (ee & 1) + hf, c = 2 * g + (ee >> 1);
        w = (uo < d.H && c < d.C && uin < d.H) ? W[(uo * d.C + c) * d.H + uin] : 0.f;
      } else {
        const int ko = 2 * (4 * g + ee) + hf, c = t;              // tile index = channel
        w = (uin < d.H && c < d.C && ko < d.H) ? W[(uin * d.C + c) * d.H + ko] : 0.f;
      }
      __bf16 a, b, c3;
      bx_split3(w, a, b, c3);
      out[e] = piece == 0 ? a : piece == 1 ? b : c3;
    }
    img[e4] = __builtin_bit_cast(u32x4, out);
  }
}

__device__ __forceinline__ void bx_stage_bias(const float* __restrict__ bias, float* tab, Dims d, int tid, int nthreads) {
  for (int e = tid; e < BX_BIAS_FLOATS; e += nthreads) {
    const int r = e & 15, half = (e >> 4) & 1, t = e >> 5;
    const int u = 4 * t + 2 * (r & 1) + half, c = r >> 1;
    tab[e] = (u < d.H && c < d.C) ? bias[u * d.C + c] : 0.f;
  }
}

// six piece products of one 32 x 32 x 16 block for TWO independent accumulators (two tiles), interleaved so that no MFMA
// waits on its own accumulator; smallest terms first: a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1.  w / w_other: the A operand's
// three pieces (largest first), wherever they live
__device__ __forceinline__ void bx_block2_pieces(const u32x4* w, const u32x4* w_other, const bf16x8 (&b)[3], f32x16& acc,
                                                 f32x16& acc_other) {
  const bf16x8 a1 = __builtin_bit_cast(bf16x8, w[0]), a2 = __builtin_bit_cast(bf16x8, w[1]), a3 = __builtin_bit_cast(bf16x8, w[2]);
  const bf16x8 o1 = __builtin_bit_cast(bf16x8, w_other[0]), o2 = __builtin_bit_cast(bf16x8, w_other[1]),
               o3 = __builtin_bit_cast(bf16x8, w_other[2]);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b[0], acc, 0, 0, 0);
  acc_other = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o3, b[0], acc_other, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b[1], acc, 0, 0, 0);
  acc_other = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o2, b[1], acc_other, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b[2], acc, 0, 0, 0);
  acc_other = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o1, b[2], acc_other, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b[0], acc, 0, 0, 0);
  acc_other = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o2, b[0], acc_other, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b[1], acc, 0, 0, 0);
  acc_other = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o1, b[1], acc_other, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b[0], acc, 0, 0, 0);
  acc_other = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o1, b[0], acc_other, 0, 0, 0);
}

// the same with the pieces read from an LDS image (a, a_other: the lane's entry of piece 0; pieces are 64 entries apart)
__device__ __forceinline__ void bx_block2(const u32x4* a, const u32x4* a_other, const bf16x8 (&b)[3], f32x16& acc,
                                          f32x16& acc_other) {
  const u32x4 w[3] = {a[0], a[64], a[128]}, w_other[3] = {a_other[0], a_other[64], a_other[128]};
  bx_block2_pieces(w, w_other, b, acc, acc_other);
}

// f (register r <-> unit 2 r + half) of the affine field at state z
__device__ __forceinline__ f32x16 bx_field(const u32x4* imgY, const float* btab, int lane, int half, const f32x16& z,
                                           const float (&dX)[MC]) {
  // the images are loop invariant: without this the compiler hoists all 48 LDS reads (192 registers) out of the time loop
  int opaque = 0;
  asm volatile("" : "+v"(opaque));
  imgY += opaque;
  bf16x8 zp0[3], zp1[3];
  bx_split8(z, 0, zp0);
  bx_split8(z, 8, zp1);
  f32x16 f;
  const float4* b4 = reinterpret_cast<const float4*>(btab) + half * 4 + opaque;
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {                                // two tiles at a time: 32 accumulator registers live
    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 bb = b4[(2 * tp + u) * 8 + q4];
        acc[u][4 * q4] = bb.x; acc[u][4 * q4 + 1] = bb.y; acc[u][4 * q4 + 2] = bb.z; acc[u][4 * q4 + 3] = bb.w;
      }
    const u32x4* a0 = imgY + (((2 * tp) * 2) * 3) * 64 + lane;    // tile 2 tp, K step 0; K step 1 is 3 * 64 further on
    const u32x4* a1 = imgY + (((2 * tp + 1) * 2) * 3) * 64 + lane;
    bx_block2(a0, a1, zp0, acc[0], acc[1]);
    bx_block2(a0 + 3 * 64, a1 + 3 * 64, zp1, acc[0], acc[1]);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s0 = acc[u][0] * dX[0], s1 = acc[u][1] * dX[0];
#pragma unroll
      for (int c = 1; c < MC; ++c) { s0 = __builtin_fmaf(acc[u][2 * c], dX[c], s0); s1 = __builtin_fmaf(acc[u][2 * c + 1], dX[c], s1); }
      f[2 * (2 * tp + u)] = s0; f[2 * (2 * tp + u) + 1] = s1;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return f;
}

// K2b's form of bx_field: the weight pieces stay in the wave's registers for the whole solve.  K2b runs one wave per SIMD, so
// beside its 256 VGPRs the wave owns 256 accumulator registers that -amdgpu-mfma-vgpr-form leaves empty; an MFMA reads SrcA
// straight from them.  bx_load_resident reads the lane's 48 entries of the staged image once and pins each to an AGPR (the
// empty asm only fixes the register class: the MFMAs stay builtins and their hazards the compiler's business).
__device__ __forceinline__ void bx_load_resident(const u32x4* imgY, int lane, u32x4 (&w)[BX_IMG_PER_LANE]) {
#pragma unroll
  for (int i = 0; i < BX_IMG_PER_LANE; ++i) {
    w[i] = imgY[i * 64 + lane];
    asm volatile("" : "+a"(w[i]));
  }
}

// bx_field with the image in registers (w[(2 t + ks) * 3 + piece]): the same bias, MFMAs and fmaf chains in the same order.
// Only the 1 KB bias table is read from LDS in the time loop.
__device__ __forceinline__ f32x16 bx_field_resident(const u32x4 (&w)[BX_IMG_PER_LANE], const float* btab, int half, const f32x16& z,
                                                    const float (&dX)[MC]) {
  // the bias table is loop invariant too: without this the compiler hoists its 32 LDS reads (128 registers) out of the time loop
  int opaque = 0;
  asm volatile("" : "+v"(opaque));
  bf16x8 zp0[3], zp1[3];
  bx_split8(z, 0, zp0);
  bx_split8(z, 8, zp1);
  f32x16 f;
  const float4* b4 = reinterpret_cast<const float4*>(btab) + half * 4 + opaque;
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {                                // two tiles at a time: 32 accumulator registers live
    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 bb = b4[(2 * tp + u) * 8 + q4];
        acc[u][4 * q4] = bb.x; acc[u][4 * q4 + 1] = bb.y; acc[u][4 * q4 + 2] = bb.z; acc[u][4 * q4 + 3] = bb.w;
      }
    const u32x4* a0 = w + (2 * tp) * 2 * 3;                       // tile 2 tp, K step 0; K step 1 is 3 entries further on
    const u32x4* a1 = w + (2 * tp + 1) * 2 * 3;
    bx_block2_pieces(a0, a1, zp0, acc[0], acc[1]);
    bx_block2_pieces(a0 + 3, a1 + 3, zp1, acc[0], acc[1]);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float s0 = acc[u][0] * dX[0], s1 = acc[u][1] * dX[0];
#pragma unroll
      for (int c = 1; c < MC; ++c) { s0 = __builtin_fmaf(acc[u][2 * c], dX[c], s0); s1 = __builtin_fmaf(acc[u][2 * c + 1], dX[c], s1); }
      f[2 * (2 * tp + u)] = s0; f[2 * (2 * tp + u) + 1] = s1;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return f;
}

// a^T df/dz (register r <-> unit 2 r + half)
__device__ __forceinline__ f32x16 bx_vjp(const u32x4* imgV, int lane, const f32x16& a, const float (&dX)[MC]) {
  int opaque = 0;
  asm volatile("" : "+v"(opaque));
  imgV += opaque;
  bf16x8 ap0[3], ap1[3];
  bx_split8(a, 0, ap0);
  bx_split8(a, 8, ap1);
  f32x16 va;
#pragma unroll
  for (int r = 0; r < 16; ++r) va[r] = 0.f;
#pragma unroll
  for (int cp = 0; cp < MC / 2; ++cp) {                           // two channels at a time
    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
    const u32x4* a0 = imgV + (((2 * cp) * 2) * 3) * 64 + lane;
    const u32x4* a1 = imgV + (((2 * cp + 1) * 2) * 3) * 64 + lane;
    bx_block2(a0, a1, ap0, acc[0], acc[1]);
    bx_block2(a0 + 3 * 64, a1 + 3 * 64, ap1, acc[0], acc[1]);
#pragma unroll
    for (int r = 0; r < 16; ++r) va[r] = __builtin_fmaf(acc[1][r], dX[2 * cp + 1], __builtin_fmaf(acc[0][r], dX[2 * cp], va[r]));
    __builtin_amdgcn_sched_barrier(0);
  }
  return va;
}

}  // namespace cde
