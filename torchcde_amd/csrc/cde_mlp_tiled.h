// cde_mlp_tiled.h -- the two-layer vector field with its output layer worked tile by tile through L2 (rk4_mlp_tiled.hip; C
// entry points in api.hip)
//   f(z) = reshape_{HxC}( act( W2 hid(W1 z + b1) + b2 ) ) dX,   float32, width <= 128, in two forms of one source:
//   NV = 2  "wide control" (K2mc / K3mc)   H <= 32, 16 < C <= 64
//   NV = 4  "tall state"   (K2mh / K3mh)   32 < H <= 64, C <= 64 with H CP <= 2048        (CP = C rounded up to 4)
// NV is the number of f32x4 state vectors a lane owns: one wave per 16 series as in cde_mlp3.h, lane (n, q) owns units q,
// 4 + q, .., 16 NV - 4 + q of every state vector, vector v register i = unit 16 v + 4 i + q.  MlpTiled<NV> below states what
// else differs between the forms; everything not named there is the same code.
// The output layer has up to 2048 rows x 128 columns (1 MiB): no LDS holds it, an XCD's L2 does.  It is worked in unit groups
// P of 4 hidden units x CP channels: a group has CP / 4 tiles, tile (P, tb) holds rows (h = 4 P + (i >> 2), c = 4 tb + (i & 3)),
// so lane (n, q) receives unit 4 P + q at channels 4 tb + r -- the tiling of field_mlp16 with a run-time number of channel
// blocks.  The lane's A operand of K group T1 is one float4: columns 16 T1 + 4 q .. + 3 of row (4 P + (n >> 2), 4 tb + (n & 3)).
//   forward   the float4 straight from the caller's W2 (rows >= H C and columns >= width read as zero, never dereferenced)
//   sweep     from the zero-padded copies cde_rk4_adjoint_mlp_{wide,tall}_prepare leave in the workspace, rows h CP + c:
//             [layer-1 image | b1 | W1^T image | b2 [ROWS] | W2 plain [ROWS][128] | W2 for gu [ROWS][8 n + T1] = W2[row][16 T1 + n]]
//             NV = 2: ROWS = 2048.  NV = 4: 2048 + 3 * 64 -- the last unit group's tiles run to unit 4 ceil(H / 4) - 1 >= H - 1,
//             up to 3 CP rows of zeros past H CP.
//   layer 1   NV = 2: K = 32, K2m's image and mlp3_layer1.  NV = 4: K = 64, 16 K steps per tile, s = 0 .. 15 IN ORDER, step
//             s feeding unit 4 s + kq; the LDS image is [tile T1][K group sg][lane][4] (32 KiB), element j of group sg = step
//             4 sg + j, then b1 [tile][q][r]
//   va        W1^T g1 has 16 NV outputs: NV accumulator tiles T, register r of lane (n, q) = unit 4 (4 T + r) + q, 32 K steps
//             (T1, r) in order; image [T][T1][lane][4] (NV = 2: K3m's; read from the workspace)
// The control slope of a tile's 16 series x CP channels does not fit the registers (a cubic row of 64 channels is 256
// floats): every stage writes it to a per-wave LDS slab [series][TL_SLAB_STRIDE] and reads one float4 per tile back.
// The sweep streams K3m's factor rows per (stage, series): U, G1 as K3m, and G2 as ceil(H CP / 256) blocks of 256 columns,
// block b = columns 256 b .. 256 b + 255 of the padded (h, c) -> h CP + c layout, 4 (k_end - k_begin) B rows apart; the
// caller reduces each block with cde_mlp_grad_reduce (layer 2) into its own [256][132] image.  Only rows h < H are written:
// the caller zeroes G2 once.  Z is NV / 2 halves of [rows][36] -- Z: units 0 .. 31 | 1, Z_hi (NV = 4): units 32 .. 63 | 1 --
// each reduced against G1 by the layer-1 form of cde_mlp_grad_reduce into its own [128][36] image.  Columns H .. of the last
// half are never written: the caller zeroes it once.
#pragma once
#include "cde_mlp3.h"

namespace cde {

constexpr int TL_MAX_C = 64;
constexpr int TL_OUT_ROWS = 2048;                            // H CP at most: the G2 blocks, the host's gather
constexpr int TL_SLAB_STRIDE = TL_MAX_C + 4;                 // floats per series of the dX slab (16-byte rows, banks apart)
constexpr int TL_SLAB_FLOATS = 16 * TL_SLAB_STRIDE;

// a wave's LDS writes before its own reads of other lanes' words, and the reads before the next writes (revheun.hip)
__device__ __forceinline__ void tl_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// dX of the wave's 16 series at one stage into its slab: lane (n, q) writes channels q, 4 + q, .. of series n (zero from C on)
template <int DEGREE>
__device__ __forceinline__ void tl_control_slope(float* slab, const float* __restrict__ coeffs, int64_t series,
                                                 int64_t n_intervals, int64_t idx, float frac, float width, int n, int q, int C,
                                                 int CP) {
  tl_wave_lds_sync();                                     // the previous stage's reads are done
  const float* p = DEGREE == CDE_PATH_CUBIC ? coeffs + (series * n_intervals + idx) * 4 * C
                                            : coeffs + (series * (n_intervals + 1) + idx) * C;
#pragma clang loop unroll(disable)
  for (int c = q; c < CP; c += 4) {
    float v = 0.f;
    if (c < C) {
      if (DEGREE == CDE_PATH_CUBIC) v = cubic_derivative(p[C + c], p[2 * C + c], p[3 * C + c], frac);
      else v = (p[C + c] - p[c]) / width;
    }
    slab[n * TL_SLAB_STRIDE + c] = v;
  }
  tl_wave_lds_sync();
}

// one tile of the output layer: y += A u over the 32 K steps, one accumulator chain, K steps in order
__device__ __forceinline__ f32x4 tl_tile_mfma(const float4 (&a)[8], const float (&u)[32], f32x4 y) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    y = mfma16(a[g].x, u[4 * g], y);
    y = mfma16(a[g].y, u[4 * g + 1], y);
    y = mfma16(a[g].z, u[4 * g + 2], y);
    y = mfma16(a[g].w, u[4 * g + 3], y);
  }
  return y;
}

// ---------------------------------------------------------------- layer 1 over K = 64 (NV = 4 alone)
constexpr int TL_W1_K64_FLOATS = 8 * 4 * 64 * 4;             // 8 tiles x 4 groups of 4 K steps
// value of [layer-1 image | b1] at flat index e
__device__ __forceinline__ float tl_l1_image_k64(const float* __restrict__ W1, const float* __restrict__ b1, int e, MlpDims d) {
  if (e < TL_W1_K64_FLOATS) {
    const int j = e & 3, l = (e >> 2) & 63, g = e >> 8;              // g = 4 T1 + sg
    const int row = 16 * (g >> 2) + (l & 15), k = 4 * (4 * (g & 3) + j) + (l >> 4);
    return (row < d.width && k < d.H) ? W1[row * d.H + k] : 0.f;
  }
  e -= TL_W1_K64_FLOATS;
  const int unit = 16 * (e >> 4) + 4 * ((e >> 2) & 3) + (e & 3);
  return unit < d.width ? b1[unit] : 0.f;
}
// value of the W1^T image at flat index e: tile T, K step (T1, r = j); lane quarter kq feeds hidden-layer unit 16 T1 + 4 kq + j,
// row i is state unit 4 (4 T + (i & 3)) + (i >> 2)
__device__ __forceinline__ float tl_w1t_image_k64(const float* __restrict__ W1, int e, MlpDims d) {
  const int j = e & 3, l = (e >> 2) & 63, i = l & 15, kq = l >> 4;
  const int g = e >> 8, T = g >> 3, T1 = g & 7;
  const int unit = 16 * T1 + 4 * kq + j, k = 4 * (4 * T + (i & 3)) + (i >> 2);
  return (unit < d.width && k < d.H) ? W1[unit * d.H + k] : 0.f;
}
// cde_mlp3.h's mlp3_layer1 for the 16 K steps of this image -- the kernels call either by the size of `zs` (w1 = image + lane,
// bb1 = bias image + q): u[4 T1 + r] = hid(pre) of unit 16 T1 + 4 q + r, `mask` bit 4 T1 + r = (pre > 0).  One accumulator
// chain per tile, bias first, the 16 K steps in order; two tiles side by side.
template <int ACT>
__device__ __forceinline__ void mlp3_layer1(const float4* w1, const float4* bb1, const float (&zs)[16], float (&u)[32],
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

// ---------------------------------------------------------------- what differs between the two forms
template <int NV>
struct MlpTiled {
  static_assert(NV == 2 || NV == 4, "two or four state vectors per lane");
  static constexpr int ROWS = NV == 2 ? TL_OUT_ROWS : TL_OUT_ROWS + 3 * TL_MAX_C;     // rows of the padded output-layer copies
  static constexpr int W1_FLOATS = NV == 2 ? W1M_FLOATS : TL_W1_K64_FLOATS;           // the layer-1 image; b1 follows it
  static constexpr int L1_FLOATS = W1_FLOATS + B1M_FLOATS;                            // the LDS images: layer 1 and its bias
  static constexpr int W1T_FLOATS = NV * 8 * 64 * 4;                                  // [tile T][T1][lane][4]
  static constexpr int IMAGE_FLOATS = L1_FLOATS + W1T_FLOATS + ROWS + 2 * ROWS * MW;
  static constexpr int W1T_AT = L1_FLOATS, B2_AT = W1T_AT + W1T_FLOATS, W2P_AT = B2_AT + ROWS, W2T_AT = W2P_AT + ROWS * MW;
  static_assert(W1T_AT % 4 == 0 && B2_AT % 4 == 0 && W2P_AT % 4 == 0 && W2T_AT % 4 == 0, "float4 reads of the image parts");

  static bool shape_ok(int64_t C, int64_t H, int64_t width) {
    if (width < 1 || width > MW) return false;
    if constexpr (NV == 2) return H >= 1 && H <= MH && C >= 17 && C <= TL_MAX_C;
    else return H >= 33 && H <= 64 && C >= 1 && C <= TL_MAX_C && H * ((C + 3) / 4 * 4) <= TL_OUT_ROWS;
  }
  // value of [layer-1 image | b1] at flat index e < L1_FLOATS (NV = 2: K2m's)
  static __device__ __forceinline__ float l1_image(const float* __restrict__ W1, const float* __restrict__ b1,
                                                   const float* __restrict__ W2, const float* __restrict__ b2, int e, MlpDims d) {
    if constexpr (NV == 2) return mlp16_image(W1, b1, W2, b2, e, d);
    else return tl_l1_image_k64(W1, b1, e, d);
  }
  // value of the W1^T image at flat index e < W1T_FLOATS (NV = 2: K3m's)
  static __device__ __forceinline__ float w1t_image(const float* __restrict__ W1, const float* __restrict__ b1,
                                                    const float* __restrict__ W2, const float* __restrict__ b2, int e, MlpDims d) {
    if constexpr (NV == 2) return mlp_adj_image(W1, b1, W2, b2, ADJ_LDS_FLOATS + e, d, 2);
    else return tl_w1t_image_k64(W1, e, d);
  }
};
static_assert(MlpTiled<2>::W1T_FLOATS == W1T_FLOATS, "NV = 2 reads K3m's W1^T image");

// steps [k_begin, k_end) of the sweep (continuous adjoint only); `Z_hi`: null for NV = 2
struct TiledSweepIO {
  const float* image; int act;
  void* y_state; void* a_state; const void* grid; int64_t k_begin, k_end;
  void* U; void* G2; void* G1; void* Z; void* Z_hi;
};

template <int NV>
size_t mlp_tiled_adjoint_image_bytes() { return (size_t)MlpTiled<NV>::IMAGE_FLOATS * sizeof(float); }
template <int NV>
int launch_mlp_tiled_adjoint_images(const TwoLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s);
template <int NV, typename TT>
int launch_forward_mlp_tiled(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                             hipStream_t s);
template <int NV, typename TT>
int launch_mlp_tiled_adjoint_sweep(const Control& x, const TiledSweepIO& io, const Shape& n, const StageTable& st, hipStream_t s);
}  // namespace cde
