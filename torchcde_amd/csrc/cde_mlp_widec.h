// cde_mlp_widec.h -- the two-layer vector field on controls of 17 .. 64 channels (rk4_mlp_widec.hip; C entry points in api.hip)
//   f(z) = reshape_{HxC}( act( W2 hid(W1 z + b1) + b2 ) ) dX,   float32, H <= 32, 16 < C <= 64, width <= 128
// One wave per 16 series as in cde_mlp3.h.  The output layer has up to 2048 rows x 128 columns (1 MiB): no LDS holds it, an
// XCD's L2 does.  It is worked in unit groups P of 4 hidden units x CP channels (CP = C rounded up to 4): a group has CP / 4
// tiles, tile (P, tb) holds rows (h = 4 P + (i >> 2), c = 4 tb + (i & 3)), so lane (n, q) receives unit 4 P + q at channels
// 4 tb + r -- the tiling of field_mlp16 with a run-time number of channel blocks.  The lane's A operand of K group T1 is one
// float4: columns 16 T1 + 4 q .. + 3 of row (4 P + (n >> 2), 4 tb + (n & 3)).
//   forward   the float4 straight from the caller's W2 (rows >= H C and columns >= width read as zero, never dereferenced)
//   sweep     from the zero-padded copies cde_rk4_adjoint_mlp_wide_prepare leaves in the workspace, rows h CP + c:
//             [layer-1 image | b1 | W1^T image | b2 [2048] | W2 plain [2048][128] | W2 for gu [2048][8 n + T1] = W2[row][16 T1 + n]]
// The control slope of a tile's 16 series x CP channels does not fit the registers (a cubic row of 64 channels is 256
// floats): every stage writes it to a per-wave LDS slab [series][WC_SLAB_STRIDE] and reads one float4 per tile back.
// The sweep streams K3m's factor rows per (stage, series): U, G1, Z as K3m, and G2 as ceil(H CP / 256) blocks of 256 columns,
// block b = columns 256 b .. 256 b + 255 of the padded (h, c) -> h CP + c layout, 4 (k_end - k_begin) B rows apart; the
// caller reduces each block with cde_mlp_grad_reduce (layer 2) into its own [256][132] image.  Only rows h < H are written:
// the caller zeroes G2 once.
#pragma once
#include "cde_mlp3.h"

namespace cde {

constexpr int WC_MIN_C = 17, WC_MAX_C = 64;
constexpr int WC_ROWS = MH * WC_MAX_C;                       // rows of the padded output-layer copies
constexpr int WC_SLAB_STRIDE = WC_MAX_C + 4;                 // floats per series of the dX slab (16-byte rows, banks apart)
constexpr int WC_SLAB_FLOATS = 16 * WC_SLAB_STRIDE;
constexpr int WC_L1_FLOATS = W1M_FLOATS + B1M_FLOATS;        // the LDS images: layer 1 and its bias
constexpr int WC_IMAGE_FLOATS = WC_L1_FLOATS + W1T_FLOATS + WC_ROWS + 2 * WC_ROWS * MW;
constexpr int WC_W1T_AT = WC_L1_FLOATS, WC_B2_AT = WC_W1T_AT + W1T_FLOATS, WC_W2P_AT = WC_B2_AT + WC_ROWS,
              WC_W2T_AT = WC_W2P_AT + WC_ROWS * MW;
static_assert(WC_B2_AT % 4 == 0 && WC_W2P_AT % 4 == 0 && WC_W2T_AT % 4 == 0, "float4 reads of the image parts");

// steps [k_begin, k_end) of the wide-control sweep (continuous adjoint only)
struct WideSweepIO {
  const float* image; int act;
  void* y_state; void* a_state; const void* grid; int64_t k_begin, k_end;
  void* U; void* G2; void* G1; void* Z;
};

bool mlp_widec_shape_ok(int64_t C, int64_t H, int64_t width);
size_t mlp_widec_adjoint_image_bytes();
int launch_mlp_widec_adjoint_images(const TwoLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s);
template <typename TT>
int launch_forward_mlp_widec(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                             hipStream_t s);
template <typename TT>
int launch_mlp_widec_adjoint_sweep(const Control& x, const WideSweepIO& io, const Shape& n, const StageTable& st, hipStream_t s);

// a wave's LDS writes before its own reads of other lanes' words, and the reads before the next writes (revheun.hip)
__device__ __forceinline__ void wc_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// dX of the wave's 16 series at one stage into its slab: lane (n, q) writes channels q, 4 + q, .. of series n (zero from C on)
template <int DEGREE>
__device__ __forceinline__ void wc_control_slope(float* slab, const float* __restrict__ coeffs, int64_t series,
                                                 int64_t n_intervals, int64_t idx, float frac, float width, int n, int q, int C,
                                                 int CP) {
  wc_wave_lds_sync();                                     // the previous stage's reads are done
  const float* p = DEGREE == CDE_PATH_CUBIC ? coeffs + (series * n_intervals + idx) * 4 * C
                                            : coeffs + (series * (n_intervals + 1) + idx) * C;
#pragma clang loop unroll(disable)
  for (int c = q; c < CP; c += 4) {
    float v = 0.f;
    if (c < C) {
      if (DEGREE == CDE_PATH_CUBIC) v = cubic_derivative(p[C + c], p[2 * C + c], p[3 * C + c], frac);
      else v = (p[C + c] - p[c]) / width;
    }
    slab[n * WC_SLAB_STRIDE + c] = v;
  }
  wc_wave_lds_sync();
}

// one tile of the output layer: y += A u over the 32 K steps, one accumulator chain, K steps in order
__device__ __forceinline__ f32x4 wc_tile_mfma(const float4 (&a)[8], const float (&u)[32], f32x4 y) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    y = mfma16(a[g].x, u[4 * g], y);
    y = mfma16(a[g].y, u[4 * g + 1], y);
    y = mfma16(a[g].z, u[4 * g + 2], y);
    y = mfma16(a[g].w, u[4 * g + 3], y);
  }
  return y;
}
}  // namespace cde
