// cde_affine_tiled.h -- the one-layer vector field on controls of 17 .. 64 channels, worked tile by tile through L2
// (rk4_affine_tiled.hip: K2c forward, K3c sweep; reached through cde_rk4_forward_linear / cde_rk4_adjoint_linear under
// CDE_VARIANT_AUTO)
//   f(z) = reshape_{HxC}( act( W z + b ) ) dX,   float32, 1 <= H <= 32, 17 <= C <= 64, act = identity or tanh
// This is the output layer of cde_mlp_tiled.h with z in the place of the hidden vector: K = H <= 32 instead of width <= 128,
// up to H CP = 2048 rows (h, c) (CP = C rounded up to 4; 256 KiB at H = 32, C = 64: no LDS holds it, an XCD's L2 does).
// One wave per 16 series, v_mfma_f32_16x16x4_f32, lane (n = l & 15, q = l >> 4).
//   ownership  lane (n, q) owns units 8 q .. 8 q + 7 of series n (field16's): two f32x4, vector v register i = unit 8 q + 4 v + i.
//   Y tiles    W is worked in unit groups j < min(H, 8) of the 4 units {j, 8 + j, 16 + j, 24 + j} x CP channels; a group has
//              CP / 4 tiles, tile (j, tb) holds rows i <-> (h = 8 (i >> 2) + j, c = 4 tb + (i & 3)).  K step s < 8 feeds unit
//              8 q + s: the lane's B operand is its OWN state register s, its A operands of a tile are columns 8 q .. 8 q + 7
//              of row (8 (n >> 2) + j, 4 tb + (n & 3)) -- two float4 of a row of W -- and its D registers r are
//              (unit 8 q + j, channel 4 tb + r): a unit it owns.  Nothing is transposed between the evaluation and the RK
//              bookkeeping.
//   forward    the two float4 straight from the caller's W (VEC: H % 4 == 0 and W 16-byte aligned; else eight guarded scalar
//              loads); rows >= H C and columns >= H read as zero, never dereferenced.
//   sweep      from the zero-padded image launch_adjoint_affine_tiled builds in its workspace, AT_ROWS rows h CP + c:
//                [ W plain [AT_ROWS][32] | b [AT_ROWS] | W for va [AT_ROWS / 4][16][4][2] ]
//              va = W^T g has 32 outputs: two accumulator tiles T, row i <-> unit 8 (i >> 2) + 4 T + (i & 3), so lane (n, q)
//              receives units 8 q + 4 T + r -- its own.  K step (j, tb, r) takes rows (8 kq + j, 4 tb + r), kq = 0 .. 3: the lane's
//              B operand is its own g register r of the tile, and its eight A operands of the tile -- (r, T) -- are the 32
//              contiguous bytes  [(h CP + 4 tb) / 4][i][r][T] = W[(h, 4 tb + r)][8 (i >> 2) + 4 T + (i & 3)]  at h = 8 q + j, i = n.
// The control slope of the tile goes through cde_mlp_tiled.h's per-wave LDS slab [series][TL_SLAB_STRIDE].
// f_h = sum_c act(Y_hc) dX_c is kept as two partial sums per unit, even and odd channels (one packed FMA per channel pair, as
// rk4_wide.hip), added once per unit group; both kernels sum in this order.
// The sweep keeps no parameter gradients; like rk4_wide.hip it streams the factors per row = (step, stage, series), series
// padded to a multiple of 16 (the padding lanes carry a = 0 and write zeros),
//     G [row][MP]   w ds dL/dY, column h CP + c; MP = H CP rounded up to 256.  Every column below H CP is written on every
//                   row (channels C .. CP - 1 as zeros: their dX is zero); columns H CP .. MP - 1 are never written -- the
//                   launcher zeroes the chunk once when MP > H CP
//     Z [row][32]   the stage value of z (units >= H as zeros)
// and launch_wide_grad_reduce (mlp_grad_reduce.hip) turns each chunk into acc (MP, 33) += G^T [Z | 1]; a gather kernel leaves
// grad_W (H C, H) and grad_b.  Workspace behind the stage tables, every part 256-byte aligned:
//     [ y (B, H) | a (B, H) | acc (MP, 33) | reduction partials | image | G chunk | Z chunk ]
// CDE_OPT_WIDE_SCRATCH_BYTES is the budget of G chunk + Z chunk (at least one RK step).
#pragma once
#include "cde_mlp_tiled.h"

namespace cde {

constexpr int AT_MAX_H = 32;
constexpr int AT_MIN_C = 17;
constexpr int AT_ROWS = TL_OUT_ROWS;                          // H CP at most
constexpr int AT_WP_AT = 0, AT_B_AT = AT_ROWS * AT_MAX_H, AT_WT_AT = AT_B_AT + AT_ROWS;
constexpr int AT_IMAGE_FLOATS = AT_WT_AT + AT_ROWS * AT_MAX_H;
static_assert(AT_B_AT % 4 == 0 && AT_WT_AT % 4 == 0, "float4 reads of the image parts");

// a lane's eight units 8 q .. 8 q + 7 of one series' row (units >= H: zero / not stored)
__device__ __forceinline__ void at_load_units8(const float* __restrict__ row, int q, int H, f32x4 (&v)[2]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) v[s >> 2][s & 3] = 8 * q + s < H ? row[8 * q + s] : 0.f;
}
__device__ __forceinline__ void at_store_units8(float* __restrict__ row, int q, int H, const f32x4 (&v)[2]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) if (8 * q + s < H) row[8 * q + s] = v[s >> 2][s & 3];
}
// one Y tile: y += A z over the 8 K steps in order, one accumulator chain
__device__ __forceinline__ f32x4 at_tile_mfma(const float4 (&a)[2], const float (&z)[8], f32x4 y) {
  y = mfma16(a[0].x, z[0], y); y = mfma16(a[0].y, z[1], y); y = mfma16(a[0].z, z[2], y); y = mfma16(a[0].w, z[3], y);
  y = mfma16(a[1].x, z[4], y); y = mfma16(a[1].y, z[5], y); y = mfma16(a[1].z, z[6], y); y = mfma16(a[1].w, z[7], y);
  return y;
}

}  // namespace cde
