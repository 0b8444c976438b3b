// cde_bf16x3_duo.h -- the pieces of K2bd (rk4_bf16x3_duo.hip): K2b's field (cde_bf16x3.h: three exact bf16 pieces per f32
// operand, six piece products per block, f32 accumulation) on v_mfma_f32_16x16x32_bf16, for a wave whose 32 series are two
// groups of 16 that run half a stage apart in one instruction stream.  One MFMA covers the whole K = 32 of a 16-row tile for
// one group's 16 series, so a group's field is 16 tiles x 6 products = 96 MFMAs of 16 cycles: the matrix time of K2b's 96
// MFMAs of 32 cycles per two groups, and every vector instruction of one group has MFMAs of the other to issue beside
// (scripts/ubench/mfma_16x16x32_duo.hip, profiles/NOTES.md round 13).
//
// Layout -- nothing moves between lanes.  Lane l: n = l & 15, q = l >> 4; group g holds series 16 g + n of the tile.
//   state   lane (n, q) keeps units 8 q + j, j = 0..7, of its series: the lane's B-operand K indices 8 q + j
//   image   [tile 16][piece 3][lane 64] uint4 (BX_IMG_U4 entries, as K2b's, so bx_load_resident pins it to 192 AGPRs):
//           tile t, row rho = l & 15 stands for unit 8 (rho >> 2) + (t >> 1), channel 4 (t & 1) + (rho & 3); element j of
//           lane (rho, q) is W[(unit, channel)][8 q + j], zero beyond H / C
//   result  D register i of tile t on lane (n, q) is row 4 q + i: unit 8 q + (t >> 1), channel 4 (t & 1) + i -- tiles 2 m and
//           2 m + 1 give the lane all eight channels of its own unit 8 q + m; f is an in-lane fmaf chain in bx_field's order
//   bias    table [tile 16][q 4] float4: the accumulator's initial value, one ds_read_b128 per tile and group
//   control lane q holds the coefficient row of channels 2 q, 2 q + 1 of its series only, forms those two slopes and the
//           four lanes of a series exchange them through a per-wave LDS strip: one ds_write_b64, two ds_read_b128
#pragma once
#include "cde_bf16x3.h"

namespace cde {

constexpr int BXD_BIAS_FLOATS = 16 * 4 * 4;                    // [tile][q][register]
constexpr int BXD_STRIP_FLOATS = 2 * 16 * 8;                   // per wave: [group][series][channel]
constexpr int BXD_FWD_LDS_BYTES = BX_IMG_U4 * 16 + BXD_BIAS_FLOATS * 4 + 4 * BXD_STRIP_FLOATS * 4;

__device__ __forceinline__ void bxd_stage_image(const float* __restrict__ W, u32x4* img, Dims d, int tid, int nthreads) {
  for (int e4 = tid; e4 < BX_IMG_U4; e4 += nthreads) {
    const int l = e4 & 63, piece = (e4 >> 6) % 3, t = (e4 >> 6) / 3;
    const int rho = l & 15, q = l >> 4;
    const int u = 8 * (rho >> 2) + (t >> 1), c = 4 * (t & 1) + (rho & 3);
    bf16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * q + j;
      const float w = (u < d.H && c < d.C && k < d.H) ? W[(u * d.C + c) * d.H + k] : 0.f;
      __bf16 a, b, c3;
      bx_split3(w, a, b, c3);
      out[j] = piece == 0 ? a : piece == 1 ? b : c3;
    }
    img[e4] = __builtin_bit_cast(u32x4, out);
  }
}

__device__ __forceinline__ void bxd_stage_bias(const float* __restrict__ bias, float* tab, Dims d, int tid, int nthreads) {
  for (int e = tid; e < BXD_BIAS_FLOATS; e += nthreads) {
    const int i = e & 3, q = (e >> 2) & 3, t = e >> 4;
    const int u = 8 * q + (t >> 1), c = 4 * (t & 1) + i;
    tab[e] = (u < d.H && c < d.C) ? bias[u * d.C + c] : 0.f;
  }
}

// the three pieces of the lane's eight values as MFMA B operands; two values per v_cvt_pk_bf16_f32, the roundings of
// bx_split3.  A vector conversion, not inline asm: the compiler sees the VALU write and keeps the MFMA's wait states
// (rk4_adjoint_pair.hip: kp_split3x2)
using bxd_bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
__device__ __forceinline__ unsigned bxd_cvt_pk(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bxd_bf16x2));
}
__device__ __forceinline__ void bxd_split8(const float (&z)[8], bf16x8 (&p)[3]) {
  u32x4 w[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float x0 = z[2 * i], x1 = z[2 * i + 1];
    const unsigned a = bxd_cvt_pk(x0, x1);
    const float r0 = x0 - __uint_as_float(a << 16), r1 = x1 - __uint_as_float(a & 0xffff0000u);
    const unsigned b = bxd_cvt_pk(r0, r1);
    const unsigned c = bxd_cvt_pk(r0 - __uint_as_float(b << 16), r1 - __uint_as_float(b & 0xffff0000u));
    w[0][i] = a; w[1][i] = b; w[2][i] = c;
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) p[m] = __builtin_bit_cast(bf16x8, w[m]);
}

// a group's 96 MFMAs: W z + b for its 16 series, every accumulator tile started from the bias table.  Tile pairs, the six
// piece products smallest first (bx_block2_pieces), the two tiles of a pair alternating
__device__ __forceinline__ void bxd_field_mfma(const u32x4 (&w)[BX_IMG_PER_LANE], const float4* b4, const bf16x8 (&zp)[3],
                                               f32x4 (&acc)[16]) {
#pragma unroll
  for (int tp = 0; tp < 8; ++tp) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float4 bb = b4[(2 * tp + u) * 4];
      acc[2 * tp + u] = f32x4{bb.x, bb.y, bb.z, bb.w};
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int pa = p == 0 ? 2 : (p == 1 || p == 3) ? 1 : 0;     // a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1
      const int pb = p == 0 ? 0 : p == 1 ? 1 : p == 2 ? 2 : p == 3 ? 0 : p == 4 ? 1 : 0;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = 2 * tp + u;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w[t * 3 + pa]), zp[pb], acc[t], 0, 0, 0);
      }
    }
  }
}

// f (register m <-> unit 8 q + m) from a group's accumulators: bx_field's fmaf chain over the channels
__device__ __forceinline__ void bxd_contract(const f32x4 (&acc)[16], const float (&dX)[MC], float (&f)[8]) {
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    float s = acc[2 * m][0] * dX[0];
#pragma unroll
    for (int c = 1; c < MC; ++c) s = __builtin_fmaf(acc[2 * m + (c >> 2)][c & 3], dX[c], s);
    f[m] = s;
  }
}

// the lane's share of a control row: channels 2 q, 2 q + 1 (zeros beyond C); cubic b, 2c, 3d; linear x[idx], x[idx + 1]
template <int DEGREE>
struct BxdRow {
  float v[DEGREE == CDE_PATH_CUBIC ? 6 : 4];
};
template <int DEGREE>
__device__ __forceinline__ BxdRow<DEGREE> bxd_load_row(const float* __restrict__ coeffs, int64_t series, int64_t n_intervals,
                                                       int64_t idx, int C, int q) {
  BxdRow<DEGREE> r;
  constexpr int PARTS = DEGREE == CDE_PATH_CUBIC ? 3 : 2;
  const float* p = DEGREE == CDE_PATH_CUBIC ? coeffs + (series * n_intervals + idx) * 4 * C + C
                                            : coeffs + (series * (n_intervals + 1) + idx) * C;
#pragma unroll
  for (int part = 0; part < PARTS; ++part)
#pragma unroll
    for (int k = 0; k < 2; ++k) r.v[2 * part + k] = 2 * q + k < C ? p[part * C + 2 * q + k] : 0.f;
  return r;
}
// the lane's two slopes into the strip row of its series (control_slope's arithmetic)
template <int DEGREE>
__device__ __forceinline__ void bxd_write_slopes(const BxdRow<DEGREE>& r, float frac, float width, float* strip_row, int q) {
  float2 s;
  if (DEGREE == CDE_PATH_CUBIC) {
    s.x = cubic_derivative(r.v[0], r.v[2], r.v[4], frac);
    s.y = cubic_derivative(r.v[1], r.v[3], r.v[5], frac);
  } else {
    s.x = (r.v[2] - r.v[0]) / width;
    s.y = (r.v[3] - r.v[1]) / width;
  }
  *reinterpret_cast<float2*>(strip_row + 2 * q) = s;
}
__device__ __forceinline__ void bxd_read_slopes(const float* strip_row, float (&dX)[MC]) {
  const float4 lo = *reinterpret_cast<const float4*>(strip_row), hi = *reinterpret_cast<const float4*>(strip_row + 4);
  dX[0] = lo.x; dX[1] = lo.y; dX[2] = lo.z; dX[3] = lo.w;
  dX[4] = hi.x; dX[5] = hi.y; dX[6] = hi.z; dX[7] = hi.w;
}

}  // namespace cde
