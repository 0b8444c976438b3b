// cde_mlp_tallh.h -- the two-layer vector field on hidden states of 33 .. 64 channels (rk4_mlp_tallh.hip; C entry points in api.hip)
//   f(z) = reshape_{HxC}( act( W2 hid(W1 z + b1) + b2 ) ) dX,   float32, 32 < H <= 64, C <= 64 with H CP <= 2048, width <= 128
// (CP = C rounded up to 4).  K2mc / K3mc (cde_mlp_widec.h) with twice the state: one wave per 16 series, lane (n, q) owns
// units q, 4 + q, .., 60 + q of every state vector -- four f32x4, vector v register i = unit 16 v + 4 i + q.  The output
// layer is worked as in cde_mlp_widec.h: ceil(H / 4) <= 16 unit groups P x CP / 4 tiles, read through L2 (forward: from the
// caller's W2; sweep: from the padded copies), the control slope through that header's per-wave LDS slab at every C.
//   layer 1   K = 64: 16 K steps per tile, s = 0 .. 15 IN ORDER, step s feeding unit 4 s + kq; the LDS image is
//             [tile T1][K group sg][lane][4] (32 KiB), element j of group sg = step 4 sg + j, then b1 [tile][q][r]
//   va        W1^T g1 has 64 outputs: four accumulator tiles T, register r of lane (n, q) = unit 4 (4 T + r) + q, 32 K
//             steps (T1, r) in order; image [T][T1][lane][4] (32 KiB, read from the workspace)
//   sweep image  [layer-1 image | b1 | W1^T image | b2 [TH_ROWS] | W2 plain [TH_ROWS][128] | W2 for gu [TH_ROWS][8 n + T1]]
//             rows h CP + c.  TH_ROWS = 2048 + 3 * 64: the last unit group's tiles run to unit 4 ceil(H / 4) - 1 >= H - 1,
//             up to 3 CP rows of zeros past H CP.
// Factor rows: U, G1 and the G2 blocks exactly as K3mc (H CP <= 2048: at most 8 blocks).  Z is two [rows][36] halves --
// Z: units 0 .. 31 | 1, Z_hi: units 32 .. 63 | 1 (columns H - 32 .. 31 never written: the caller zeroes it once) -- each
// reduced against G1 by the layer-1 form of cde_mlp_grad_reduce into its own [128][36] image.
#pragma once
#include "cde_mlp_widec.h"

namespace cde {

constexpr int TH_MIN_H = 33, TH_MAX_H = 64, TH_MAX_C = 64;
constexpr int TH_OUT_ROWS = 2048;                            // H CP at most: the G2 blocks, the host's gather
constexpr int TH_ROWS = TH_OUT_ROWS + 3 * TH_MAX_C;          // rows of the padded output-layer copies
constexpr int TH_W1_FLOATS = 8 * 4 * 64 * 4;                 // layer 1: 8 tiles x 4 groups of 4 K steps
constexpr int TH_L1_FLOATS = TH_W1_FLOATS + B1M_FLOATS;      // the LDS images: layer 1 and its bias
constexpr int TH_W1T_FLOATS = 4 * 8 * 64 * 4;                // [tile T][T1][lane][4]
constexpr int TH_IMAGE_FLOATS = TH_L1_FLOATS + TH_W1T_FLOATS + TH_ROWS + 2 * TH_ROWS * MW;
constexpr int TH_W1T_AT = TH_L1_FLOATS, TH_B2_AT = TH_W1T_AT + TH_W1T_FLOATS, TH_W2P_AT = TH_B2_AT + TH_ROWS,
              TH_W2T_AT = TH_W2P_AT + TH_ROWS * MW;
static_assert(TH_W1T_AT % 4 == 0 && TH_B2_AT % 4 == 0 && TH_W2P_AT % 4 == 0 && TH_W2T_AT % 4 == 0, "float4 reads of the image parts");

// steps [k_begin, k_end) of the tall-state sweep (continuous adjoint only)
struct TallSweepIO {
  const float* image; int act;
  void* y_state; void* a_state; const void* grid; int64_t k_begin, k_end;
  void* U; void* G2; void* G1; void* Z; void* Z_hi;
};

bool mlp_tallh_shape_ok(int64_t C, int64_t H, int64_t width);
size_t mlp_tallh_adjoint_image_bytes();
int launch_mlp_tallh_adjoint_images(const TwoLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s);
template <typename TT>
int launch_forward_mlp_tallh(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                             hipStream_t s);
template <typename TT>
int launch_mlp_tallh_adjoint_sweep(const Control& x, const TallSweepIO& io, const Shape& n, const StageTable& st, hipStream_t s);

// value of [layer-1 image | b1] at flat index e
__device__ __forceinline__ float th_l1_image(const float* __restrict__ W1, const float* __restrict__ b1, int e, MlpDims d) {
  if (e < TH_W1_FLOATS) {
    const int j = e & 3, l = (e >> 2) & 63, g = e >> 8;              // g = 4 T1 + sg
    const int row = 16 * (g >> 2) + (l & 15), k = 4 * (4 * (g & 3) + j) + (l >> 4);
    return (row < d.width && k < d.H) ? W1[row * d.H + k] : 0.f;
  }
  e -= TH_W1_FLOATS;
  const int unit = 16 * (e >> 4) + 4 * ((e >> 2) & 3) + (e & 3);
  return unit < d.width ? b1[unit] : 0.f;
}
// value of the W1^T image at flat index e: tile T, K step (T1, r = j); lane quarter kq feeds hidden-layer unit 16 T1 + 4 kq + j,
// row i is state unit 4 (4 T + (i & 3)) + (i >> 2)
__device__ __forceinline__ float th_w1t_image(const float* __restrict__ W1, int e, MlpDims d) {
  const int j = e & 3, l = (e >> 2) & 63, i = l & 15, kq = l >> 4;
  const int g = e >> 8, T = g >> 3, T1 = g & 7;
  const int unit = 16 * T1 + 4 * kq + j, k = 4 * (4 * T + (i & 3)) + (i >> 2);
  return (unit < d.width && k < d.H) ? W1[unit * d.H + k] : 0.f;
}

// layer 1 from the LDS image (w1 = image + lane, bb1 = bias image + q): u[4 T1 + r] = hid(pre) of unit 16 T1 + 4 q + r, `mask`
// bit 4 T1 + r = (pre > 0).  One accumulator chain per tile, bias first, the 16 K steps in order; two tiles side by side.
template <int ACT>
__device__ __forceinline__ void th_layer1(const float4* w1, const float4* bb1, const float (&zs)[16], float (&u)[32],
                                          unsigned& mask) {
  mask = 0;
#pragma unroll
  for (int TP = 0; TP < 4; ++TP) {
    const float4 c0 = bb1[8 * TP], c1 = bb1[8 * TP + 4];
    f32x4 y0 = {c0.x, c0.y, c0.z, c0.w}, y1 = {c1.x, c1.y, c1.z, c1.w};
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) {
      const float4 g0 = w1[(8 * TP + sg) * 64], g1 = w1[(8 * TP + 4 + sg) * 64];
      y0 = mfma16(g0.x, zs[4 * sg], y0);     y1 = mfma16(g1.x, zs[4 * sg], y1);
      y0 = mfma16(g0.y, zs[4 * sg + 1], y0); y1 = mfma16(g1.y, zs[4 * sg + 1], y1);
      y0 = mfma16(g0.z, zs[4 * sg + 2], y0); y1 = mfma16(g1.z, zs[4 * sg + 2], y1);
      y0 = mfma16(g0.w, zs[4 * sg + 3], y0); y1 = mfma16(g1.w, zs[4 * sg + 3], y1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u[8 * TP + r] = hidden_activate<ACT>(y0[r]);
      u[8 * TP + 4 + r] = hidden_activate<ACT>(y1[r]);
      mask |= (y0[r] > 0.f ? 1u : 0u) << (8 * TP + r);
      mask |= (y1[r] > 0.f ? 1u : 0u) << (8 * TP + 4 + r);
    }
  }
}
}  // namespace cde
