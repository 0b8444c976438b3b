// cde_mlp3.h -- the three-layer vector field (rk4_mlp3.hip; its C entry points are in api.hip)
//   f(z) = reshape_{HxC}( act( W2 hid( Wm hid(W1 z + b1) + bm ) + b2 ) ) dX,   hid = relu | softplus for both hidden layers
// on the tiles of the two-layer kernels (cde_mfma.h: field_mlp16; cde_mlp_adj.h): float32, H <= 32, C <= 8, both hidden
// widths <= 128, one wave per 16 series.  Layer 1's C/D fragment -- lane (n, q) holds units 16 T1 + 4 q + r of series n -- is
// the B operand of the middle layer's K step (T1, r), whose own C/D fragment is in turn the B operand of layer 2's K steps, so
// neither hidden state leaves the registers.  The middle layer is 8 output tiles x 32 K steps = 256 MFMAs; its transpose
// (dL/du1 = Wm^T dL/dpre2, the adjoint sweep) another 256.
//   forward image      A[i][kq] of (output tile T', K step (T1, r)) = Wm[16 T' + i][16 T1 + 4 kq + r]
//   transposed image   A[i][kq] of (output tile T1, K step (T', r)) = Wm[16 T' + 4 kq + r][16 T1 + i]
// both [output tile][K tile][lane][r] (one float4 per lane and tile pair), zero outside the real (width2, width1); the bias
// is the accumulator's initial value ([tile][q][r], as layer 1's).  The two 64 KB images do not fit the LDS beside the other
// layers' (149 / 153 KB of 160): the sweep reads them from the prepared workspace (L2-resident, one float4 per lane and
// 4 MFMAs, like the W1^T image), the forward kernel -- which has no workspace -- the same float4 straight from the caller's
// Wm (rows of 16 bytes when width1 is a multiple of 4 and Wm is aligned; element by element otherwise).
#pragma once
#include "cde_mlp_adj.h"
#include "cde_launch.h"

namespace cde {

constexpr int WMM_FLOATS = 8 * 8 * 64 * 4;              // one middle-layer image
constexpr int BMM_FLOATS = B1M_FLOATS;                  // its bias image [tile][q][r]
constexpr int MLP3_FWD_LDS_FLOATS = MLP16_LDS_FLOATS + BMM_FLOATS;       // K2m's images | bm
constexpr int MLP3_ADJ_LDS_FLOATS = ADJ_LDS_FLOATS + BMM_FLOATS;         // K3m's LDS images | bm
// the prepared workspace image: [LDS part | W1^T | Wm forward | Wm transposed]
constexpr int MLP3_ADJ_IMAGE_FLOATS = MLP3_ADJ_LDS_FLOATS + W1T_FLOATS + 2 * WMM_FLOATS;
constexpr int GM_COLS = 256;                            // row stride of the streamed dL/dpre2 rows (128 written; see api.hip)

struct ThreeLayerField {
  const void* W1; const void* bias1; int64_t width1;
  const void* Wm; const void* biasm; int64_t width2;
  const void* W2; const void* bias2; int act;
};
struct Mlp3Dims { int H, C, w1, w2; };
// steps [k_begin, k_end) of the three-layer sweep (continuous adjoint only)
struct Sweep3IO {
  const float* image; int act;
  void* y_state; void* a_state; const void* grid; int64_t k_begin, k_end;
  void* U; void* U1; void* G2; void* Gm; void* G1; void* Z;
};

bool mlp3_shape_ok(int64_t C, int64_t H, int64_t width1, int64_t width2);
size_t mlp3_adjoint_image_bytes();
int launch_mlp3_adjoint_images(const ThreeLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s);
template <typename TT>
int launch_forward_mlp3(const Control& x, const ThreeLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                        hipStream_t s);
template <typename TT>
int launch_mlp3_adjoint_sweep(const Control& x, const Sweep3IO& io, const Shape& n, const StageTable& st, hipStream_t s);

__device__ __forceinline__ float wm_image(const float* __restrict__ Wm, int e, int w1, int w2, bool transposed) {
  const int r = e & 3, l = (e >> 2) & 63, i = l & 15, kq = l >> 4, g = e >> 8, To = g >> 3, Tk = g & 7;
  const int row = transposed ? 16 * Tk + 4 * kq + r : 16 * To + i;
  const int col = transposed ? 16 * To + i : 16 * Tk + 4 * kq + r;
  return (row < w2 && col < w1) ? Wm[row * w1 + col] : 0.f;
}
__device__ __forceinline__ float bm_image(const float* __restrict__ bm, int e, int w2) {
  const int unit = 16 * (e >> 4) + 4 * ((e >> 2) & 3) + (e & 3);
  return unit < w2 ? bm[unit] : 0.f;
}

// One tile pair of a middle-layer product (forward or transposed): its 16 float4 of A operands, and the 64 MFMAs that consume
// them -- two accumulator chains, K steps in order, so that no MFMA waits for its own predecessor.
struct WmPair { float4 a0[8], a1[8]; };
template <typename LoadA>
__device__ __forceinline__ WmPair wm_pair_load(int TP, LoadA&& loadA) {
  WmPair p;
#pragma unroll
  for (int Tk = 0; Tk < 8; ++Tk) { p.a0[Tk] = loadA(2 * TP, Tk); p.a1[Tk] = loadA(2 * TP + 1, Tk); }
  return p;
}
__device__ __forceinline__ void wm_pair_mfma(const WmPair& p, const float (&b)[32], f32x4& y0, f32x4& y1) {
#pragma unroll
  for (int Tk = 0; Tk < 8; ++Tk) {
    y0 = mfma16(p.a0[Tk].x, b[4 * Tk], y0);     y1 = mfma16(p.a1[Tk].x, b[4 * Tk], y1);
    y0 = mfma16(p.a0[Tk].y, b[4 * Tk + 1], y0); y1 = mfma16(p.a1[Tk].y, b[4 * Tk + 1], y1);
    y0 = mfma16(p.a0[Tk].z, b[4 * Tk + 2], y0); y1 = mfma16(p.a1[Tk].z, b[4 * Tk + 2], y1);
    y0 = mfma16(p.a0[Tk].w, b[4 * Tk + 3], y0); y1 = mfma16(p.a1[Tk].w, b[4 * Tk + 3], y1);
  }
}

// u2 = hid(Wm u1 + bm) for the lane's 32 units of the second hidden layer (u2[4 T' + r] = unit 16 T' + 4 q + r), `mask` bit
// 4 T' + r = (its pre-activation > 0).  ONE accumulator chain per tile, bias first, K steps in order -- in the forward
// kernel and in the sweep alike.
// bbm: bias image + q;  loadA(T', T1): the lane's float4 of the forward image
// AHEAD (the sweep, which has the registers: one wave per SIMD): the next tile pair's operands are requested before the
// MFMAs of the pair at hand, so that their L2 latency passes behind 64 MFMAs instead of in front of them.
template <int ACT, bool AHEAD, typename LoadA>
__device__ __forceinline__ void mlp3_middle(const float4* bbm, const float (&u1)[32], float (&u2)[32], unsigned& mask,
                                            LoadA&& loadA) {
  mask = 0;
  WmPair cur = wm_pair_load(0, loadA);
#pragma unroll
  for (int TP = 0; TP < 4; ++TP) {
    const float4 c0 = bbm[8 * TP], c1 = bbm[8 * TP + 4];
    f32x4 y0 = {c0.x, c0.y, c0.z, c0.w}, y1 = {c1.x, c1.y, c1.z, c1.w};
    WmPair next = cur;
    if constexpr (AHEAD) {
      if (TP < 3) next = wm_pair_load(TP + 1, loadA);
      __builtin_amdgcn_sched_barrier(0);
    }
    wm_pair_mfma(cur, u1, y0, y1);
    if constexpr (AHEAD) __builtin_amdgcn_sched_barrier(0);
    else if (TP < 3) next = wm_pair_load(TP + 1, loadA);
    cur = next;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u2[8 * TP + r] = hidden_activate<ACT>(y0[r]);
      u2[8 * TP + 4 + r] = hidden_activate<ACT>(y1[r]);
      mask |= (y0[r] > 0.f ? 1u : 0u) << (8 * TP + r);
      mask |= (y1[r] > 0.f ? 1u : 0u) << (8 * TP + 4 + r);
    }
  }
}

// gu1 = Wm^T gm, tile T1 of the result in gu1[T1] (register r: unit 16 T1 + 4 q + r, the fragment form of u1);
// loadT(T1, T'): the lane's float4 of the transposed image.  The sweep only: operands one tile pair ahead, as above.
template <typename LoadT>
__device__ __forceinline__ void mlp3_middle_transposed(const float (&gm)[32], f32x4 (&gu1)[8], LoadT&& loadT) {
  WmPair cur = wm_pair_load(0, loadT);
#pragma unroll
  for (int TP = 0; TP < 4; ++TP) {
    f32x4 y0 = {0.f, 0.f, 0.f, 0.f}, y1 = y0;
    WmPair next = cur;
    if (TP < 3) next = wm_pair_load(TP + 1, loadT);
    __builtin_amdgcn_sched_barrier(0);
    wm_pair_mfma(cur, gm, y0, y1);
    __builtin_amdgcn_sched_barrier(0);
    cur = next;
    gu1[2 * TP] = y0; gu1[2 * TP + 1] = y1;
  }
}

// layer 1 of the two-layer kernels, from the LDS image (w1 = image + lane, bb1 = bias image + q)
template <int ACT>
__device__ __forceinline__ void mlp3_layer1(const float4* w1, const float4* bb1, const float (&zs)[8], float (&u)[32],
                                            unsigned& mask) {
  mask = 0;
#pragma unroll
  for (int TP = 0; TP < 4; ++TP) {
    const float4 c0 = bb1[8 * TP], c1 = bb1[8 * TP + 4];
    f32x4 y0 = {c0.x, c0.y, c0.z, c0.w}, y1 = {c1.x, c1.y, c1.z, c1.w};
    const float4 g00 = w1[(4 * TP) * 64], g01 = w1[(4 * TP + 1) * 64], g10 = w1[(4 * TP + 2) * 64], g11 = w1[(4 * TP + 3) * 64];
    const float a0[8] = {g00.x, g00.y, g00.z, g00.w, g01.x, g01.y, g01.z, g01.w};
    const float a1[8] = {g10.x, g10.y, g10.z, g10.w, g11.x, g11.y, g11.z, g11.w};
#pragma unroll
    for (int s = 0; s < 8; ++s) { y0 = mfma16(a0[s], zs[s], y0); y1 = mfma16(a1[s], zs[s], y1); }
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
