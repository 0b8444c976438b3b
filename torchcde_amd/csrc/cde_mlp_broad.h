// cde_mlp_broad.h -- the two-layer vector field with an inner layer of 129 .. 256 units ("broad inner layer": K2mb / K3mb,
// rk4_mlp_broad.hip; C entry points in api.hip)
//   f(z) = reshape_{HxC}( act( W2 hid(W1 z + b1) + b2 ) ) dX,   float32, 128 < width <= 256, H <= 32, C <= 64, H CP <= 1024
// The wide-control form of cde_mlp_tiled.h (NV = 2: one wave per 16 series, lane (n, q) owns units q, 4 + q, .., 28 + q of the
// two state vectors, the output layer worked tile (P, tb) by tile from L2, the dX slab per wave) with the inner layer in two
// HALVES of 128 units: units 0 .. 127 and 128 .. 255.  Every per-half object has the layout the 128-unit kernels give it, so
// tl_tile_mfma, mlp3_layer1 and -- on the host's side -- cde_mlp_grad_reduce serve a half each, unchanged.
//   layer 1   K = 32 over 16 output tiles: the image is K2m's twice over, [tile T1 < 16][K group sg < 2][lane][4] (32 KiB),
//             then b1 [tile][q][r] (1 KiB), in LDS.  u_lo / u_hi [32]: register 4 T + r of half s = unit 128 s + 16 T + 4 q + r.
//   output    tile (P, tb) has 16 K groups: the lower 8 on u_lo, then the upper 8 on u_hi, into the same accumulator (K steps
//             ascending, one chain, bias first).  Two operand sets of 8 float4: a half's operands are requested while the MFMAs of
//             the half before it run.
//   forward   the float4 of K group g straight from the caller's W2: columns 16 g + 4 q .. + 3 of row (4 P + (n >> 2),
//             4 tb + (n & 3)); rows >= H C and columns >= width read as zero, never dereferenced
//   sweep     from the zero-padded copies cde_rk4_adjoint_mlp_broad_prepare leaves in the workspace, rows h CP + c:
//             [layer-1 image | b1 | W1^T image | b2 [ROWS] | W2 plain [ROWS][256] | W2 for gu [ROWS][16 n + T1] = W2[row][16 T1 + n]]
//             ROWS = 1024 + 3 * 64: the last unit group's tiles run to unit 4 ceil(H / 4) - 1 >= H - 1, up to 3 CP rows of
//             zeros past H CP (as the tall-state form has them).
//   gu        gu += W2^T dL/dY2 per tile: 16 accumulators, the lower 8 (units 0 .. 127) from the first two float4 of the lane's
//             gu row, the upper 8 from the last two -- the same two operand sets, alternating with the Y2 halves.
//   va        W1^T g1 over 64 K steps (T1 < 16, r) in order on the two state tiles; image [T < 2][T1 < 16][lane][4], read from
//             the workspace.
// Factor rows per (stage, series), for cde_mlp_grad_reduce as it is:
//   U_lo, U_hi    [rows][132]: units 0 .. 127 and 128 .. 255 (all 128 columns of both are written; a unit >= width carries
//                 hid(0), which meets only columns of dW2 the caller drops).  The caller writes the "1" of column 128.
//   G1_lo, G1_hi  [rows][128], quadrature-weighted.  The columns of units >= width are exact zeros: the gu copy's columns beyond
//                 the width are zero, so gu is, and 0 * hid' = 0 (relu: the pre-activation 0 is not > 0).
//   G2, Z         as K3mc: ceil(H CP / 256) <= 4 blocks of 256 columns; [rows][36].
#pragma once
#include "cde_mlp_tiled.h"

namespace cde {

constexpr int BR_WIDTH = 2 * MW;                              // inner-layer units the tiles are built for
constexpr int BR_OUT_ROWS = 1024;                             // H CP at most
constexpr int BR_ROWS = BR_OUT_ROWS + 3 * TL_MAX_C;           // rows of the padded output-layer copies
constexpr int BR_W1_FLOATS = 2 * W1M_FLOATS;                  // the layer-1 image; b1 follows it
constexpr int BR_B1_FLOATS = 2 * B1M_FLOATS;
constexpr int BR_L1_FLOATS = BR_W1_FLOATS + BR_B1_FLOATS;     // the LDS images
constexpr int BR_W1T_FLOATS = 2 * 16 * 64 * 4;                // [tile T][T1][lane][4]
constexpr int BR_IMAGE_FLOATS = BR_L1_FLOATS + BR_W1T_FLOATS + BR_ROWS + 2 * BR_ROWS * BR_WIDTH;
constexpr int BR_W1T_AT = BR_L1_FLOATS, BR_B2_AT = BR_W1T_AT + BR_W1T_FLOATS, BR_W2P_AT = BR_B2_AT + BR_ROWS,
              BR_W2T_AT = BR_W2P_AT + BR_ROWS * BR_WIDTH;
static_assert(BR_W1T_AT % 4 == 0 && BR_B2_AT % 4 == 0 && BR_W2P_AT % 4 == 0 && BR_W2T_AT % 4 == 0, "float4 reads of the image parts");

inline bool mlp_broad_shape_ok(int64_t C, int64_t H, int64_t width) {
  return width > MW && width <= BR_WIDTH && H >= 1 && H <= MH && C >= 1 && C <= TL_MAX_C && H * ((C + 3) / 4 * 4) <= BR_OUT_ROWS;
}

// value of [layer-1 image | b1] at flat index e < BR_L1_FLOATS (mlp16_image's first two parts over 16 tiles)
__device__ __forceinline__ float br_l1_image(const float* __restrict__ W1, const float* __restrict__ b1, int e, MlpDims d) {
  if (e < BR_W1_FLOATS) {
    const int j = e & 3, l = (e >> 2) & 63, g = e >> 8;              // g = 2 T1 + sg
    const int row = 16 * (g >> 1) + (l & 15), k = 4 * (4 * (g & 1) + j) + (l >> 4);
    return (row < d.width && k < d.H) ? W1[row * d.H + k] : 0.f;
  }
  e -= BR_W1_FLOATS;
  const int unit = 16 * (e >> 4) + 4 * ((e >> 2) & 3) + (e & 3);
  return unit < d.width ? b1[unit] : 0.f;
}
// value of the W1^T image at flat index e < BR_W1T_FLOATS: tile T, K step (T1, r = j); lane quarter kq feeds inner-layer unit
// 16 T1 + 4 kq + j, row i is state unit 4 (4 T + (i & 3)) + (i >> 2)
__device__ __forceinline__ float br_w1t_image(const float* __restrict__ W1, int e, MlpDims d) {
  const int j = e & 3, l = (e >> 2) & 63, i = l & 15, kq = l >> 4;
  const int g = e >> 8, T = g >> 4, T1 = g & 15;
  const int unit = 16 * T1 + 4 * kq + j, k = 4 * (4 * T + (i & 3)) + (i >> 2);
  return (unit < d.width && k < d.H) ? W1[unit * d.H + k] : 0.f;
}

// steps [k_begin, k_end) of the sweep (continuous adjoint only)
struct BroadSweepIO {
  const float* image; int act;
  void* y_state; void* a_state; const void* grid; int64_t k_begin, k_end;
  void* U_lo; void* U_hi; void* G2; void* G1_lo; void* G1_hi; void* Z;
};

inline size_t mlp_broad_adjoint_image_bytes() { return (size_t)BR_IMAGE_FLOATS * sizeof(float); }
int launch_mlp_broad_adjoint_images(const TwoLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s);
template <typename TT>
int launch_forward_mlp_broad(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                             hipStream_t s);
template <typename TT>
int launch_mlp_broad_adjoint_sweep(const Control& x, const BroadSweepIO& io, const Shape& n, const StageTable& st, hipStream_t s);
}  // namespace cde
