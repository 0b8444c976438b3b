// rk4_mlp_broad.hip -- K2mb / K3mb: the fused RK4 (3/8 rule) solve and continuous-adjoint sweep of the two-layer vector field
//   f(z) = reshape_{HxC}( act( W2 hid(W1 z + b1) + b2 ) ) dX
// with an inner layer of 129 .. 256 units (H <= 32, C <= 64, H CP <= 1024): cde_mlp_broad.h.  K2mc / K3mc (rk4_mlp_tiled.hip,
// NV = 2) with the inner layer in two halves of 128 units -- one wave per 16-series tile, float32, the output layer as
// ceil(H / 4) unit groups x CP / 4 tiles read from L2, every tile as two K halves into one accumulator:
//   forward   128 + 64 ceil(H / 4) CP / 4 MFMAs per evaluation (1152 at H = 32, C = 8; 4224 at H = 32, C = 32)
//   sweep     128 + 128 ceil(H / 4) CP / 4 + 128 (2304; 8448): each tile's Y2 product and its share of gu = W2^T dL/dY2
// A half's operands are requested while the MFMAs of the half before it run (two operand sets of 8 float4, no copies).
#include "cde_mlp_broad.h"

namespace cde {

// ============================================================================================ forward
// VEC: width is a multiple of 4 and W2 16-byte aligned -- the lane's four K steps of a tile's K group are one float4 of W2's
// row (h, c) at column 16 g + 4 q; otherwise four guarded scalar loads.
template <typename TT, int DEGREE, int ACT, bool VEC>
__global__ __launch_bounds__(512, 2) void rk4_forward_mlp_broad(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W1, const float* __restrict__ bias1, const float* __restrict__ W2,
    const float* __restrict__ bias2, const float* __restrict__ z0, const TT* __restrict__ grid, int64_t n_grid,
    const TT* __restrict__ t_out, int64_t n_out, float* __restrict__ z_out, int64_t B,
    const int64_t* __restrict__ stage_index, const float* __restrict__ stage_frac, MlpDims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int e = threadIdx.x; e < BR_L1_FLOATS; e += blockDim.x) lds[e] = br_l1_image(W1, bias1, e, dims);
  __syncthreads();
  const int Hr = dims.H, Cr = dims.C, wr = dims.width;
  const int CP = (Cr + 3) & ~3, NPr = (Hr + 3) >> 2, NBr = CP >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 16 >= B) return;                                        // (no workgroup barrier from here on)
  float* slab = lds + BR_L1_FLOATS + wave * TL_SLAB_FLOATS;
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  f32x4 y[2];                                                        // this lane's units: y[v][i] = unit 16 v + 4 i + q
#pragma unroll
  for (int v = 0; v < 2; ++v) y[v] = load_units4<4>(z0 + sc * Hr, 16 * v + q, Hr);
  auto store = [&](int64_t j, const f32x4 (&a)[2]) {
    if (valid) {
      float* row = z_out + (series * n_out + j) * Hr;
#pragma unroll
      for (int v = 0; v < 2; ++v) store_units4<4>(row, 16 * v + q, Hr, a[v]);
    }
  };
  store(0, y);
  int64_t jout = 1;
  const int64_t n_steps = n_grid - 1;
  if (n_steps <= 0) return;

  // K half `half` of tile (P, tb): the lane's A operands (row (4 P + (n >> 2), 4 tb + (n & 3)), columns 128 half + 16 g + 4 q
  // .. + 3).  Beyond the real (H, C, width) -- a tile past the last one included -- zeros, nothing is read.
  auto load_half = [&](int P, int tb, int half, float4 (&a)[8]) {
    const int h = 4 * P + (n >> 2), c = 4 * tb + (n & 3);
    const bool ok = h < Hr && c < Cr;
    const int col0 = MW * half + 4 * q;
    const float* p = W2 + ((int64_t)(ok ? h * Cr + c : 0) * wr + col0);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int col = col0 + 16 * g;
      if constexpr (VEC) {
        a[g] = (ok && col < wr) ? *reinterpret_cast<const float4*>(p + 16 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        a[g] = make_float4(ok && col < wr ? p[16 * g] : 0.f, ok && col + 1 < wr ? p[16 * g + 1] : 0.f,
                           ok && col + 2 < wr ? p[16 * g + 2] : 0.f, ok && col + 3 < wr ? p[16 * g + 3] : 0.f);
      }
    }
  };
  // the bias of the lane's D rows (4 P + q, 4 tb + r): the accumulator's initial value
  auto load_bias = [&](int P, int tb, f32x4& bias) {
    const int hb = 4 * P + q;
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (hb < Hr && 4 * tb + r < Cr) ? bias2[hb * Cr + 4 * tb + r] : 0.f;
  };

  int64_t idx = stage_index[0];
  float frac = stage_frac[0];

  for (int64_t k = 0; k < n_steps; ++k) {
    const TT t0 = grid[k], t1 = grid[k + 1];
    const float dt = (float)(t1 - t0);
    f32x4 k1[2], k2[2], pq[2], z[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) z[v] = y[v];
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      tl_control_slope<DEGREE>(slab, coeffs, sc, n_intervals, idx, frac, width, n, q, Cr, CP);
      const int64_t e_next = 4 * k + stage + 1;
      const bool more = e_next < 4 * n_steps;
      const int64_t nidx = more ? stage_index[e_next] : idx;
      const float nfrac = more ? stage_frac[e_next] : frac;

      // ---- the field: layer 1 (LDS), the output layer tile by tile (L2) + activation + contraction with dX (LDS slab)
      f32x4 f4[2];
#pragma unroll
      for (int v = 0; v < 2; ++v) f4[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      {
        int opaque = 0;                         // keeps the LDS reads inside the evaluation (cde_mfma.h: field_act16)
        asm volatile("" : "+v"(opaque));
        const float4* w1 = reinterpret_cast<const float4*>(lds) + lane + opaque;
        const float4* bb1 = reinterpret_cast<const float4*>(lds + BR_W1_FLOATS) + q + opaque;
        const float4* dxs = reinterpret_cast<const float4*>(slab + n * TL_SLAB_STRIDE) + opaque;
        float zs[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) zs[s] = z[s >> 2][s & 3];
        float u_lo[32], u_hi[32];
        unsigned unused;
        mlp3_layer1<ACT>(w1, bb1, zs, u_lo, unused);                         // tiles 0 .. 7
        mlp3_layer1<ACT>(w1 + 16 * 64, bb1 + 32, zs, u_hi, unused);          // tiles 8 .. 15
        __builtin_amdgcn_sched_barrier(0);
        float4 alo[8], ahi[8];
        f32x4 cb;
        load_half(0, 0, 0, alo);
        load_bias(0, 0, cb);
#pragma clang loop unroll(disable)
        for (int P = 0; P < NPr; ++P) {          // unit group P: 4 hidden units x CP channels = NBr tiles
          float f = 0.f;
#pragma clang loop unroll(disable)
          for (int tb = 0; tb < NBr; ++tb) {
            load_half(P, tb, 1, ahi);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 yv = tl_tile_mfma(alo, u_lo, cb);
            __builtin_amdgcn_sched_barrier(0);
            const bool wrap = tb + 1 >= NBr;
            load_half(wrap ? P + 1 : P, wrap ? 0 : tb + 1, 0, alo);          // (past the last tile: zeros)
            load_bias(wrap ? P + 1 : P, wrap ? 0 : tb + 1, cb);
            __builtin_amdgcn_sched_barrier(0);
            yv = tl_tile_mfma(ahi, u_hi, yv);
            const f32x2 t01 = activate2<ACT>(yv[0], yv[1]), t23 = activate2<ACT>(yv[2], yv[3]);
            const float4 dx = dxs[tb];
            f = __builtin_fmaf(t01[0], dx.x, f); f = __builtin_fmaf(t01[1], dx.y, f);
            f = __builtin_fmaf(t23[0], dx.z, f); f = __builtin_fmaf(t23[1], dx.w, f);
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int s = 0; s < 8; ++s) f4[s >> 2][s & 3] = P == s ? f : f4[s >> 2][s & 3];
        }
      }

      // torchdiffeq rk4_alt_step_func (3/8 rule), association order preserved
      const float third = (float)(1.0 / 3.0);
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const f32x4 fv = f4[v];
        if (stage == 0) {
          k1[v] = fv;
          z[v] = y[v] + dt * k1[v] * third;
        } else if (stage == 1) {
          k2[v] = fv;
          z[v] = y[v] + dt * (k2[v] - k1[v] * third);
        } else if (stage == 2) {
          z[v] = y[v] + dt * (k1[v] - k2[v] + fv);
          pq[v] = k1[v] + 3.f * (k2[v] + fv);
        } else {
          z[v] = y[v] + (pq[v] + fv) * dt * 0.125f;
        }
      }
      idx = nidx; frac = nfrac;
    }
    while (jout < n_out && t1 >= t_out[jout]) {
      const TT tj = t_out[jout];
      if (tj == t0) store(jout, y);
      else if (tj == t1) store(jout, z);
      else {
        const float slope = (float)((tj - t0) / (t1 - t0));
        f32x4 mid[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) mid[v] = y[v] + slope * (z[v] - y[v]);
        store(jout, mid);
      }
      ++jout;
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) y[v] = z[v];
  }
}

// ============================================================================================ adjoint sweep
__global__ void mlp_broad_adj_image_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                           const float* __restrict__ W2, const float* __restrict__ b2, float* __restrict__ img,
                                           MlpDims d) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= BR_IMAGE_FLOATS) return;
  const int at = e, CP = (d.C + 3) & ~3;
  if (e < BR_L1_FLOATS) { img[at] = br_l1_image(W1, b1, e, d); return; }                                // layer 1 | b1 (the forward's)
  e -= BR_L1_FLOATS;
  if (e < BR_W1T_FLOATS) { img[at] = br_w1t_image(W1, e, d); return; }
  e -= BR_W1T_FLOATS;
  if (e < BR_ROWS) {                                                                                    // b2 at h CP + c
    const int h = e / CP, c = e - h * CP;
    img[at] = (h < d.H && c < d.C) ? b2[h * d.C + c] : 0.f;
    return;
  }
  e -= BR_ROWS;
  const bool for_gu = e >= BR_ROWS * BR_WIDTH;
  if (for_gu) e -= BR_ROWS * BR_WIDTH;
  const int row = e >> 8, j = e & 255, col = for_gu ? 16 * (j & 15) + (j >> 4) : j;     // gu copy: [row][16 n + T1] = W2[row][16 T1 + n]
  const int h = row / CP, c = row - h * CP;
  img[at] = (h < d.H && c < d.C && col < d.width) ? W2[(h * d.C + c) * d.width + col] : 0.f;
}

// K3mc with the inner layer in two halves: per stage  u_lo, u_hi and their masks (layer 1) -> per tile (P, tb): Y2 (two K
// halves), activation, f, g2 = a_h dX_c act'(Y2) (streamed, quadrature-weighted), gu_lo, gu_hi += W2^T g2 -> g1 = gu hid'(pre1)
// -> va = W1^T g1 (64 K steps).  Two operand sets A and B alternate through the four products of a tile:
//   request Y2-upper (B) | Y2-lower MFMAs (A) | request gu-lower (A) | Y2-upper MFMAs (B) | request gu-upper (B) |
//   gu-lower MFMAs (A) | request the next tile's Y2-lower (A) | gu-upper MFMAs (B)
// One wave per SIMD (at most 256 threads, as K3mc): u, gu, g1's inputs and the RK state of z and a need more than 256 registers.
template <typename TT, int DEGREE, int ACT>
__global__ __launch_bounds__(256, 1) void rk4_adjoint_mlp_broad_sweep(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ img, float* __restrict__ y_state, float* __restrict__ a_state,
    const TT* __restrict__ sgrid, int64_t k_begin, int64_t k_end, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, float* __restrict__ U_lo, float* __restrict__ U_hi, float* __restrict__ G2,
    float* __restrict__ G1_lo, float* __restrict__ G1_hi, float* __restrict__ Z, int64_t B, Dims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  {
    const float4* src = reinterpret_cast<const float4*>(img);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < BR_L1_FLOATS / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int Hr = dims.H, Cr = dims.C;
  const int CP = (Cr + 3) & ~3, NPr = (Hr + 3) >> 2, NBr = CP >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 16 >= B) return;                                        // (no workgroup barrier from here on)
  float* slab = lds + BR_L1_FLOATS + wave * TL_SLAB_FLOATS;
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  const int64_t block_rows = (k_end - k_begin) * 4 * B;              // rows between two blocks of G2
  const float4* w1t_base = reinterpret_cast<const float4*>(img + BR_W1T_AT) + lane;
  // lane offsets into the padded copies: Y2 rows (h & 3 = n >> 2, c & 3 = n & 3) at columns 4 q; the lane's own rows
  // (h & 3 = q) for the bias, the G2 columns and -- at 16 n -- the gu copy
  const int y_off = ((n >> 2) * CP + (n & 3)) * BR_WIDTH + 4 * q;
  const int own_off = q * CP;

  f32x4 y[2], a[2];                                                  // this lane's units: [v][i] = unit 16 v + 4 i + q
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    y[v] = load_units4<4>(y_state + sc * Hr, 16 * v + q, Hr);
    a[v] = load_units4<4>(a_state + sc * Hr, 16 * v + q, Hr);
    if (!valid) a[v] = f32x4{0.f, 0.f, 0.f, 0.f};                    // a == 0 stays 0: padded lanes contribute nothing
  }

  int64_t idx = stage_index[4 * k_begin];
  float frac = stage_frac[4 * k_begin];

  for (int64_t k = k_begin; k < k_end; ++k) {
    const float ds = (float)(sgrid[k + 1] - sgrid[k]);
    f32x4 ky1[2], ky2[2], ka1[2], ka2[2], z[2], sa[2];               // the RK temporaries; stage values of z and a
#pragma unroll
    for (int v = 0; v < 2; ++v) { z[v] = y[v]; sa[v] = a[v]; }
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      tl_control_slope<DEGREE>(slab, coeffs, sc, n_intervals, idx, frac, width, n, q, Cr, CP);
      const int64_t e_next = 4 * k + stage + 1;
      const bool more = e_next < 4 * k_end;
      const int64_t nidx = more ? stage_index[e_next] : idx;
      const float nfrac = more ? stage_frac[e_next] : frac;
      const float wq = ((stage == 0 || stage == 3) ? 0.125f : 0.375f) * ds;      // 3/8-rule quadrature weight
      const int64_t out_row = ((k - k_begin) * 4 + stage) * B + series;          // (stage, series)

      int opaque = 0;                                                // keeps the LDS / image reads inside the stage
      asm volatile("" : "+v"(opaque));
      const float4* w1 = reinterpret_cast<const float4*>(lds) + lane + opaque;
      const float4* bb1 = reinterpret_cast<const float4*>(lds + BR_W1_FLOATS) + q + opaque;
      const float4* dxs = reinterpret_cast<const float4*>(slab + n * TL_SLAB_STRIDE) + opaque;
      const float4* w1t = w1t_base + opaque;
      const float* b2p = img + BR_B2_AT + own_off + opaque;
      const float* w2y = img + BR_W2P_AT + y_off + opaque;
      const float* w2g = img + BR_W2T_AT + own_off * BR_WIDTH + 16 * n + opaque;
      float zs[8], as[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) { zs[s] = z[s >> 2][s & 3]; as[s] = sa[s >> 2][s & 3]; }

      // ---- layer 1: u and its masks, half by half (softplus: the slope is re-derived from the value)
      float u_lo[32], u_hi[32];
      unsigned mask_lo, mask_hi;
      mlp3_layer1<ACT>(w1, bb1, zs, u_lo, mask_lo);                            // tiles 0 .. 7
      mlp3_layer1<ACT>(w1 + 16 * 64, bb1 + 32, zs, u_hi, mask_hi);             // tiles 8 .. 15
      if (valid) {
        float* ulo = U_lo + out_row * U_COLS + 4 * q;                // units 16 T1 + 4 q + r and 128 + the same
        float* uhi = U_hi + out_row * U_COLS + 4 * q;
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1) {
          stream_store4(ulo + 16 * T1, u_lo[4 * T1], u_lo[4 * T1 + 1], u_lo[4 * T1 + 2], u_lo[4 * T1 + 3]);
          stream_store4(uhi + 16 * T1, u_hi[4 * T1], u_hi[4 * T1 + 1], u_hi[4 * T1 + 2], u_hi[4 * T1 + 3]);
        }
        float* zrow = Z + out_row * Z_COLS;
#pragma unroll
        for (int m = 0; m < 8; ++m) if (4 * m + q < Hr) zrow[4 * m + q] = zs[m];
      }
      __builtin_amdgcn_sched_barrier(0);

      // ---- the output layer tile by tile: Y2, activation, contraction, dL/dY2, gu += W2^T dL/dY2
      f32x4 gu_lo[8], gu_hi[8];
#pragma unroll
      for (int T1 = 0; T1 < 8; ++T1) gu_lo[T1] = gu_hi[T1] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 f4[2];
#pragma unroll
      for (int v = 0; v < 2; ++v) f4[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      // Tile (P, tb) of the padded copies starts 4 P CP + 4 tb rows in, and group P's tiles end at row 4 (P + 1) CP - 1.  No
      // request may read past the copies' BR_ROWS rows: groups P < NPr stay inside 4 NPr CP <= (H + 3) CP <= 1024 + 3 * 64 at
      // every shape of the envelope.  The request after the last tile asks for group NPr, which could end past them; its
      // operands are never consumed, so it reads row 0 instead.
      float4 sA[8], sB[8];
      f32x4 cy;
      auto load_y = [&](int rows, int half, float4 (&s)[8]) {
        const float* p = w2y + rows * BR_WIDTH + MW * half;
#pragma unroll
        for (int g = 0; g < 8; ++g) s[g] = *reinterpret_cast<const float4*>(p + 16 * g);
      };
      auto load_g = [&](int rows, int half, float4 (&s)[8]) {        // rows (4 P + q, 4 tb + r): [16 n + T1], T1 = 8 half ..
        const float4* p = reinterpret_cast<const float4*>(w2g + rows * BR_WIDTH) + 2 * half;
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[2 * r] = p[r * (BR_WIDTH / 4)]; s[2 * r + 1] = p[r * (BR_WIDTH / 4) + 1]; }
      };
      auto gu_mfma = [&](const float4 (&s)[8], const float (&g2)[4], f32x4 (&gu)[8]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // K step (P, c = 4 tb + r); 8 independent accumulator chains
          const float rv[8] = {s[2 * r].x, s[2 * r].y, s[2 * r].z, s[2 * r].w,
                               s[2 * r + 1].x, s[2 * r + 1].y, s[2 * r + 1].z, s[2 * r + 1].w};
#pragma unroll
          for (int T1 = 0; T1 < 8; ++T1) gu[T1] = mfma16(rv[T1], g2[r], gu[T1]);
        }
      };
      load_y(0, 0, sA);
      {
        const float4 c0 = *reinterpret_cast<const float4*>(b2p);
        cy = f32x4{c0.x, c0.y, c0.z, c0.w};
      }
#pragma clang loop unroll(disable)
      for (int P = 0; P < NPr; ++P) {            // unit group P: 4 hidden units x CP channels = NBr tiles
        float as_P = as[0];
#pragma unroll
        for (int kk = 1; kk < 8; ++kk) as_P = P == kk ? as[kk] : as_P;
        const bool own = valid && 4 * P + q < Hr;                    // the lane's row (4 P + q, .) exists
        float f = 0.f;
#pragma clang loop unroll(disable)
        for (int tb = 0; tb < NBr; ++tb) {
          const int rows = 4 * P * CP + 4 * tb;
          load_y(rows, 1, sB);
          __builtin_amdgcn_sched_barrier(0);
          f32x4 yv = tl_tile_mfma(sA, u_lo, cy);
          __builtin_amdgcn_sched_barrier(0);
          load_g(rows, 0, sA);
          __builtin_amdgcn_sched_barrier(0);
          yv = tl_tile_mfma(sB, u_hi, yv);
          const f32x2 t01 = activate2<ACT>(yv[0], yv[1]), t23 = activate2<ACT>(yv[2], yv[3]);
          const float tv[4] = {t01[0], t01[1], t23[0], t23[1]};
          const float4 dx4 = dxs[tb];
          const float dx[4] = {dx4.x, dx4.y, dx4.z, dx4.w};
          float g2[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = tv[r];
            f = __builtin_fmaf(t, dx[r], f);
            const float slope = final_tanh(ACT) ? __builtin_fmaf(-t, t, 1.f) : 1.f;
            g2[r] = as_P * (dx[r] * slope);
          }
          if (own) {
            const int at = (4 * P + q) * CP + 4 * tb;                // column of the padded layout: block at >> 8, column at & 255
            float* grow = G2 + ((int64_t)(at >> 8) * block_rows + out_row) * G2_COLS + (at & 255);
            stream_store4(grow, g2[0] * wq, g2[1] * wq, g2[2] * wq, g2[3] * wq);
          }
          __builtin_amdgcn_sched_barrier(0);
          load_g(rows, 1, sB);
          __builtin_amdgcn_sched_barrier(0);
          gu_mfma(sA, g2, gu_lo);
          __builtin_amdgcn_sched_barrier(0);
          {
            const bool wrap = tb + 1 >= NBr;
            const int Pn = wrap ? P + 1 : P, tbn = wrap ? 0 : tb + 1;
            const int rn = Pn < NPr ? 4 * Pn * CP + 4 * tbn : 0;
            load_y(rn, 0, sA);
            const float4 c0 = *reinterpret_cast<const float4*>(b2p + rn);
            cy = f32x4{c0.x, c0.y, c0.z, c0.w};
          }
          __builtin_amdgcn_sched_barrier(0);
          gu_mfma(sB, g2, gu_hi);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) f4[s >> 2][s & 3] = P == s ? f : f4[s >> 2][s & 3];
      }

      // ---- dL/dpre1 = gu * hid'(pre1);  va = W1^T dL/dpre1
      float g1_lo[32], g1_hi[32];
#pragma unroll
      for (int s2 = 0; s2 < 32; ++s2) {
        g1_lo[s2] = hidden_backward<ACT>(gu_lo[s2 >> 2][s2 & 3], (mask_lo >> s2) & 1u, u_lo[s2]);
        g1_hi[s2] = hidden_backward<ACT>(gu_hi[s2 >> 2][s2 & 3], (mask_hi >> s2) & 1u, u_hi[s2]);
      }
      if (valid) {
        float* glo = G1_lo + out_row * G1_COLS + 4 * q;
        float* ghi = G1_hi + out_row * G1_COLS + 4 * q;
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1) {
          stream_store4(glo + 16 * T1, g1_lo[4 * T1] * wq, g1_lo[4 * T1 + 1] * wq, g1_lo[4 * T1 + 2] * wq, g1_lo[4 * T1 + 3] * wq);
          stream_store4(ghi + 16 * T1, g1_hi[4 * T1] * wq, g1_hi[4 * T1 + 1] * wq, g1_hi[4 * T1 + 2] * wq, g1_hi[4 * T1 + 3] * wq);
        }
      }
      f32x4 va[2];
#pragma unroll
      for (int v = 0; v < 2; ++v) va[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      auto va_half = [&](const float (&g1)[32], int half) {          // K steps (T1, r) in order, two independent accumulator chains
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1) {
          float4 at[2];
#pragma unroll
          for (int v = 0; v < 2; ++v) at[v] = w1t[(16 * v + 8 * half + T1) * 64];
#pragma unroll
          for (int v = 0; v < 2; ++v) va[v] = mfma16(at[v].x, g1[4 * T1], va[v]);
#pragma unroll
          for (int v = 0; v < 2; ++v) va[v] = mfma16(at[v].y, g1[4 * T1 + 1], va[v]);
#pragma unroll
          for (int v = 0; v < 2; ++v) va[v] = mfma16(at[v].z, g1[4 * T1 + 2], va[v]);
#pragma unroll
          for (int v = 0; v < 2; ++v) va[v] = mfma16(at[v].w, g1[4 * T1 + 3], va[v]);
        }
      };
      va_half(g1_lo, 0);
      va_half(g1_hi, 1);

      __builtin_amdgcn_sched_barrier(0);
      // ---- reverse-time dynamics: dz/ds = -f, da/ds = +a^T df/dz; torchdiffeq 3/8 rule, association preserved
      const float third = (float)(1.0 / 3.0);
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const f32x4 ky = -f4[v], ka = va[v];
        if (stage == 0) {
          ky1[v] = ky; ka1[v] = ka;
          z[v] = y[v] + ds * ky1[v] * third;
          sa[v] = a[v] + ds * ka1[v] * third;
        } else if (stage == 1) {
          ky2[v] = ky; ka2[v] = ka;
          z[v] = y[v] + ds * (ky2[v] - ky1[v] * third);
          sa[v] = a[v] + ds * (ka2[v] - ka1[v] * third);
        } else if (stage == 2) {
          z[v] = y[v] + ds * (ky1[v] - ky2[v] + ky);
          sa[v] = a[v] + ds * (ka1[v] - ka2[v] + ka);
          ky1[v] = ky1[v] + 3.f * (ky2[v] + ky);
          ka1[v] = ka1[v] + 3.f * (ka2[v] + ka);
        } else {
          z[v] = y[v] + (ky1[v] + ky) * ds * 0.125f;
          sa[v] = a[v] + (ka1[v] + ka) * ds * 0.125f;
        }
      }
      idx = nidx; frac = nfrac;
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) { y[v] = z[v]; a[v] = sa[v]; }
  }
  if (valid) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      store_units4<4>(y_state + series * Hr, 16 * v + q, Hr, y[v]);
      store_units4<4>(a_state + series * Hr, 16 * v + q, Hr, a[v]);
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
static size_t broad_lds_bytes(unsigned waves) { return (size_t)(BR_L1_FLOATS + waves * TL_SLAB_FLOATS) * sizeof(float); }

int launch_mlp_broad_adjoint_images(const TwoLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s) {
  mlp_broad_adj_image_kernel<<<(BR_IMAGE_FLOATS + 255) / 256, 256, 0, s>>>(
      f32(f.W1), f32(f.bias1), f32(f.W2), f32(f.bias2), img, MlpDims{(int)H, (int)C, (int)f.width});
  return check_launch();
}

template <typename TT>
int launch_forward_mlp_broad(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                             hipStream_t s) {
  if (!mlp_broad_shape_ok(n.C, n.H, f.width)) return CDE_ERR_UNSUPPORTED;
  const MlpDims dims{(int)n.H, (int)n.C, (int)f.width};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 8), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = broad_lds_bytes(waves);
  const bool vec = (f.width & 3) == 0 && ((uintptr_t)f.W2 & 15) == 0;
  const int rc = dispatch_degree_field(x.degree, f.act, [&](auto D, auto A) {
    auto launch = [&](auto V) {
      auto kernel = rk4_forward_mlp_broad<TT, D(), A(), V()>;
      allow_lds(kernel, lds);
      kernel<<<blocks, 64 * waves, lds, s>>>(f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W1), f32(f.bias1), f32(f.W2),
                                      f32(f.bias2), f32(io.z0), (const TT*)io.grid, io.n_grid, (const TT*)io.t_out, io.n_out,
                                      f32(io.z_out), n.B, st.index, f32(st.frac), dims);
    };
    if (vec) launch(std::true_type{}); else launch(std::false_type{});
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

template <typename TT>
int launch_mlp_broad_adjoint_sweep(const Control& x, const BroadSweepIO& io, const Shape& n, const StageTable& st, hipStream_t s) {
  if (io.k_end <= io.k_begin) return CDE_OK;
  if (!mlp_broad_shape_ok(n.C, n.H, BR_WIDTH)) return CDE_ERR_UNSUPPORTED;
  const Dims dims{(int)n.H, (int)n.C};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 4), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = broad_lds_bytes(waves);
  const int rc = dispatch_degree_field(x.degree, io.act, [&](auto D, auto A) {
    auto kernel = rk4_adjoint_mlp_broad_sweep<TT, D(), A()>;
    allow_lds(kernel, lds);
    kernel<<<blocks, 64 * waves, lds, s>>>(f32(x.coeffs), f32(x.knots), x.n_intervals, io.image, f32(io.y_state), f32(io.a_state),
                                    (const TT*)io.grid, io.k_begin, io.k_end, st.index, f32(st.frac), f32(io.U_lo), f32(io.U_hi),
                                    f32(io.G2), f32(io.G1_lo), f32(io.G1_hi), f32(io.Z), n.B, dims);
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

#define CDE_INST(TT)                                                                                                    \
  template int launch_forward_mlp_broad<TT>(const Control&, const TwoLayerField&, const ForwardIO&, const Shape&,      \
                                            const StageTable&, hipStream_t);                                           \
  template int launch_mlp_broad_adjoint_sweep<TT>(const Control&, const BroadSweepIO&, const Shape&, const StageTable&, \
                                                  hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
