// rk4_mlp_tiled.hip -- K2mc / K3mc (NV = 2) and K2mh / K3mh (NV = 4): the fused RK4 (3/8 rule) solve and continuous-adjoint
// sweep of the two-layer vector field
//   f(z) = reshape_{HxC}( act( W2 hid(W1 z + b1) + b2 ) ) dX
// on controls of 17 .. 64 channels (NV = 2, H <= 32) and on hidden states of 33 .. 64 channels (NV = 4, C <= 64 with
// H CP <= 2048): cde_mlp_tiled.h.  One wave per 16-series tile, float32, width <= 128; no shared-tile forms.  Both kernels are
// K2m3 / K3m3 (rk4_mlp3.hip) without the middle layer, with NV state vectors per lane (layer 1 over K = 16 NV, va = W1^T g1
// on NV tiles) and with the output layer as ceil(H / 4) unit groups x CP / 4 tiles read from L2:
//   forward   32 NV + 32 ceil(H / 4) CP / 4 MFMAs per evaluation (4160 at H = 32, C = 64; 4224 at H = 64, C = 32)
//   sweep     32 NV + 64 ceil(H / 4) CP / 4 + 32 NV (8320; 8448): each tile's Y2 product and its share of gu = W2^T dL/dY2
// A tile's operands are requested while the MFMAs of the tile before it run (two operand sets in registers, no copies).
#include "cde_mlp_tiled.h"

namespace cde {

// ============================================================================================ forward
// VEC: width is a multiple of 4 and W2 16-byte aligned -- the lane's four K steps of a tile's K group are one float4 of W2's
// row (h, c) at column 16 T1 + 4 q; otherwise four guarded scalar loads.
template <int NV, typename TT, int DEGREE, int ACT, bool VEC>
__global__ __launch_bounds__(512, 2) void rk4_forward_mlp_tiled(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W1, const float* __restrict__ bias1, const float* __restrict__ W2,
    const float* __restrict__ bias2, const float* __restrict__ z0, const TT* __restrict__ grid, int64_t n_grid,
    const TT* __restrict__ t_out, int64_t n_out, float* __restrict__ z_out, int64_t B,
    const int64_t* __restrict__ stage_index, const float* __restrict__ stage_frac, MlpDims dims) {
  using Form = MlpTiled<NV>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int e = threadIdx.x; e < Form::L1_FLOATS; e += blockDim.x) lds[e] = Form::l1_image(W1, bias1, W2, bias2, e, dims);
  __syncthreads();
  const int Hr = dims.H, Cr = dims.C, wr = dims.width;
  const int CP = (Cr + 3) & ~3, NPr = (Hr + 3) >> 2, NBr = CP >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 16 >= B) return;                                        // (no workgroup barrier from here on)
  float* slab = lds + Form::L1_FLOATS + wave * TL_SLAB_FLOATS;
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  f32x4 y[NV];                                                       // this lane's units: y[v][i] = unit 16 v + 4 i + q
#pragma unroll
  for (int v = 0; v < NV; ++v) y[v] = load_units4<4>(z0 + sc * Hr, 16 * v + q, Hr);
  auto store = [&](int64_t j, const f32x4 (&a)[NV]) {
    if (valid) {
      float* row = z_out + (series * n_out + j) * Hr;
#pragma unroll
      for (int v = 0; v < NV; ++v) store_units4<4>(row, 16 * v + q, Hr, a[v]);
    }
  };
  store(0, y);
  int64_t jout = 1;
  const int64_t n_steps = n_grid - 1;
  if (n_steps <= 0) return;

  // tile (P, tb): the lane's A operands (row (4 P + (n >> 2), 4 tb + (n & 3)), columns 16 g + 4 q .. + 3) and the bias of its
  // D rows (4 P + q, 4 tb + r).  Beyond the real (H, C, width) -- a tile past the last one included -- zeros, nothing is read.
  auto load_tile = [&](int P, int tb, float4 (&a)[8], f32x4& bias) {
    const int h = 4 * P + (n >> 2), c = 4 * tb + (n & 3);
    const bool ok = h < Hr && c < Cr;
    const float* p = W2 + ((int64_t)(ok ? h * Cr + c : 0) * wr + 4 * q);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int col = 16 * g + 4 * q;
      if constexpr (VEC) {
        a[g] = (ok && col < wr) ? *reinterpret_cast<const float4*>(p + 16 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        a[g] = make_float4(ok && col < wr ? p[16 * g] : 0.f, ok && col + 1 < wr ? p[16 * g + 1] : 0.f,
                           ok && col + 2 < wr ? p[16 * g + 2] : 0.f, ok && col + 3 < wr ? p[16 * g + 3] : 0.f);
      }
    }
    const int hb = 4 * P + q;
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (hb < Hr && 4 * tb + r < Cr) ? bias2[hb * Cr + 4 * tb + r] : 0.f;
  };

  int64_t idx = stage_index[0];
  float frac = stage_frac[0];

  for (int64_t k = 0; k < n_steps; ++k) {
    const TT t0 = grid[k], t1 = grid[k + 1];
    const float dt = (float)(t1 - t0);
    f32x4 k1[NV], k2[NV], pq[NV], z[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) z[v] = y[v];
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      tl_control_slope<DEGREE>(slab, coeffs, sc, n_intervals, idx, frac, width, n, q, Cr, CP);
      const int64_t e_next = 4 * k + stage + 1;
      const bool more = e_next < 4 * n_steps;
      const int64_t nidx = more ? stage_index[e_next] : idx;
      const float nfrac = more ? stage_frac[e_next] : frac;

      // ---- the field: layer 1 (LDS), the output layer tile by tile (L2) + activation + contraction with dX (LDS slab)
      f32x4 f4[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) f4[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      {
        int opaque = 0;                         // keeps the LDS reads inside the evaluation (cde_mfma.h: field_act16)
        asm volatile("" : "+v"(opaque));
        const float4* w1 = reinterpret_cast<const float4*>(lds) + lane + opaque;
        const float4* bb1 = reinterpret_cast<const float4*>(lds + Form::W1_FLOATS) + q + opaque;
        const float4* dxs = reinterpret_cast<const float4*>(slab + n * TL_SLAB_STRIDE) + opaque;
        float zs[4 * NV];
#pragma unroll
        for (int s = 0; s < 4 * NV; ++s) zs[s] = z[s >> 2][s & 3];
        float u[32];
        unsigned unused;
        mlp3_layer1<ACT>(w1, bb1, zs, u, unused);
        __builtin_amdgcn_sched_barrier(0);
        auto finish = [&](const f32x4& yv, int tb, float f) {      // activation and the tile's four channels of f
          const f32x2 t01 = activate2<ACT>(yv[0], yv[1]), t23 = activate2<ACT>(yv[2], yv[3]);
          const float4 dx = dxs[tb];
          f = __builtin_fmaf(t01[0], dx.x, f); f = __builtin_fmaf(t01[1], dx.y, f);
          f = __builtin_fmaf(t23[0], dx.z, f); f = __builtin_fmaf(t23[1], dx.w, f);
          return f;
        };
        float4 a0[8], a1[8];
        f32x4 c0, c1;
        load_tile(0, 0, a0, c0);
#pragma clang loop unroll(disable)
        for (int P = 0; P < NPr; ++P) {          // unit group P: 4 hidden units x CP channels = NBr tiles, two per round
          float f = 0.f;
#pragma clang loop unroll(disable)
          for (int tb = 0; tb < NBr; tb += 2) {
            const bool pair = tb + 1 < NBr;
            load_tile(P, tb + 1, a1, c1);        // (past the group's last tile: zeros)
            __builtin_amdgcn_sched_barrier(0);
            f = finish(tl_tile_mfma(a0, u, c0), tb, f);
            __builtin_amdgcn_sched_barrier(0);
            const bool wrap = tb + 2 >= NBr;
            load_tile(wrap ? P + 1 : P, wrap ? 0 : tb + 2, a0, c0);
            __builtin_amdgcn_sched_barrier(0);
            if (pair) f = finish(tl_tile_mfma(a1, u, c1), tb + 1, f);
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int s = 0; s < 4 * NV; ++s) f4[s >> 2][s & 3] = P == s ? f : f4[s >> 2][s & 3];
        }
      }

      // torchdiffeq rk4_alt_step_func (3/8 rule), association order preserved
      const float third = (float)(1.0 / 3.0);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
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
        f32x4 mid[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) mid[v] = y[v] + slope * (z[v] - y[v]);
        store(jout, mid);
      }
      ++jout;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) y[v] = z[v];
  }
}

// ============================================================================================ adjoint sweep
template <int NV>
__global__ void mlp_tiled_adj_image_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                           const float* __restrict__ W2, const float* __restrict__ b2, float* __restrict__ img,
                                           MlpDims d) {
  using Form = MlpTiled<NV>;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Form::IMAGE_FLOATS) return;
  const int at = e, CP = (d.C + 3) & ~3;
  if (e < Form::L1_FLOATS) { img[at] = Form::l1_image(W1, b1, W2, b2, e, d); return; }                  // layer 1 | b1 (the forward's)
  e -= Form::L1_FLOATS;
  if (e < Form::W1T_FLOATS) { img[at] = Form::w1t_image(W1, b1, W2, b2, e, d); return; }
  e -= Form::W1T_FLOATS;
  if (e < Form::ROWS) {                                                                                 // b2 at h CP + c
    const int h = e / CP, c = e - h * CP;
    img[at] = (h < d.H && c < d.C) ? b2[h * d.C + c] : 0.f;
    return;
  }
  e -= Form::ROWS;
  const bool for_gu = e >= Form::ROWS * MW;
  if (for_gu) e -= Form::ROWS * MW;
  const int row = e >> 7, j = e & 127, col = for_gu ? 16 * (j & 7) + (j >> 3) : j;      // gu copy: [row][8 n + T1] = W2[row][16 T1 + n]
  const int h = row / CP, c = row - h * CP;
  img[at] = (h < d.H && c < d.C && col < d.width) ? W2[(h * d.C + c) * d.width + col] : 0.f;
}

// K3m3's one-wave-per-tile sweep without the middle layer: per stage  u, mask (layer 1) -> per tile (P, tb): Y2, activation,
// f, g2 = a_h dX_c act'(Y2) (streamed, quadrature-weighted), gu += W2^T g2 -> g1 = gu hid'(pre1) -> va = W1^T g1 (NV tiles).
// The tile's gu operands are requested before its Y2 MFMAs, the next tile's Y2 operands before its gu MFMAs.
// One wave per SIMD (at most 256 threads, as K3m3): under 512-thread bounds the stage body of NV = 2 -- u, gu, two operand sets
// and the RK state of z and a -- spilled 164 bytes per lane, and NV = 4 needs more than 256 registers.
template <int NV, typename TT, int DEGREE, int ACT>
__global__ __launch_bounds__(256, 1) void rk4_adjoint_mlp_tiled_sweep(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ img, float* __restrict__ y_state, float* __restrict__ a_state,
    const TT* __restrict__ sgrid, int64_t k_begin, int64_t k_end, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, float* __restrict__ U, float* __restrict__ G2, float* __restrict__ G1,
    float* __restrict__ Z, float* __restrict__ Z_hi, int64_t B, Dims dims) {
  using Form = MlpTiled<NV>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  {
    const float4* src = reinterpret_cast<const float4*>(img);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < Form::L1_FLOATS / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int Hr = dims.H, Cr = dims.C;
  const int CP = (Cr + 3) & ~3, NPr = (Hr + 3) >> 2, NBr = CP >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 16 >= B) return;                                        // (no workgroup barrier from here on)
  float* slab = lds + Form::L1_FLOATS + wave * TL_SLAB_FLOATS;
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  const int64_t block_rows = (k_end - k_begin) * 4 * B;              // rows between two blocks of G2
  const float4* w1t_base = reinterpret_cast<const float4*>(img + Form::W1T_AT) + lane;
  // lane offsets into the padded copies: Y2 rows (h & 3 = n >> 2, c & 3 = n & 3) at columns 4 q; the lane's own rows
  // (h & 3 = q) for the bias, the G2 columns and -- at 8 n -- the gu copy
  const int y_off = ((n >> 2) * CP + (n & 3)) * MW + 4 * q;
  const int own_off = q * CP;

  f32x4 y[NV], a[NV];                                                // this lane's units: [v][i] = unit 16 v + 4 i + q
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    y[v] = load_units4<4>(y_state + sc * Hr, 16 * v + q, Hr);
    a[v] = load_units4<4>(a_state + sc * Hr, 16 * v + q, Hr);
    if (!valid) a[v] = f32x4{0.f, 0.f, 0.f, 0.f};                    // a == 0 stays 0: padded lanes contribute nothing
  }

  int64_t idx = stage_index[4 * k_begin];
  float frac = stage_frac[4 * k_begin];

  for (int64_t k = k_begin; k < k_end; ++k) {
    const float ds = (float)(sgrid[k + 1] - sgrid[k]);
    f32x4 ky1[NV], ky2[NV], ka1[NV], ka2[NV], z[NV], sa[NV];         // the RK temporaries; stage values of z and a
#pragma unroll
    for (int v = 0; v < NV; ++v) { z[v] = y[v]; sa[v] = a[v]; }
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
      const float4* bb1 = reinterpret_cast<const float4*>(lds + Form::W1_FLOATS) + q + opaque;
      const float4* dxs = reinterpret_cast<const float4*>(slab + n * TL_SLAB_STRIDE) + opaque;
      const float4* w1t = w1t_base + opaque;
      const float* b2p = img + Form::B2_AT + own_off + opaque;
      const float* w2y = img + Form::W2P_AT + y_off + opaque;
      const float* w2g = img + Form::W2T_AT + own_off * MW + 8 * n + opaque;
      float zs[4 * NV], as[4 * NV];
#pragma unroll
      for (int s = 0; s < 4 * NV; ++s) { zs[s] = z[s >> 2][s & 3]; as[s] = sa[s >> 2][s & 3]; }

      // ---- layer 1: u and its mask (softplus: the slope is re-derived from the value)
      float u[32];
      unsigned mask;
      mlp3_layer1<ACT>(w1, bb1, zs, u, mask);
      if (valid) {
        float* urow = U + out_row * U_COLS + 4 * q;                  // hidden-layer units 16*T1 + 4q + r
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1) stream_store4(urow + 16 * T1, u[4 * T1], u[4 * T1 + 1], u[4 * T1 + 2], u[4 * T1 + 3]);
        float* zrow = Z + out_row * Z_COLS;                          // units 0 .. 31; NV = 4: 32 .. 63 into the second half
#pragma unroll
        for (int m = 0; m < 8; ++m) if (NV == 4 || 4 * m + q < Hr) zrow[4 * m + q] = zs[m];      // (H > 32: all of them exist)
        if constexpr (NV == 4) {
          float* zhrow = Z_hi + out_row * Z_COLS;
#pragma unroll
          for (int m = 8; m < 16; ++m) if (4 * m + q < Hr) zhrow[4 * (m - 8) + q] = zs[m];
        }
      }
      __builtin_amdgcn_sched_barrier(0);

      // ---- the output layer tile by tile: Y2, activation, contraction, dL/dY2, gu += W2^T dL/dY2
      f32x4 gu[8];
#pragma unroll
      for (int T1 = 0; T1 < 8; ++T1) gu[T1] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 f4[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) f4[v] = f32x4{0.f, 0.f, 0.f, 0.f};
      // Tile (P, tb) of the padded copies starts 4 P CP + 4 tb rows in, and group P's tiles end at row 4 (P + 1) CP - 1.  No
      // request may read past the copies' Form::ROWS rows: groups P < NPr stay inside 4 NPr CP <= Form::ROWS at every shape
      // of the envelope (NV = 2: 4 * 8 * 64; NV = 4: (H + 3) CP <= 2048 + 3 * 64).  The request after the last tile asks for
      // group NPr, which could end past them; its operands are never consumed, so it reads row 0 instead.
      float4 ay[8], ag[8];
      f32x4 cy;
      auto load_y = [&](int P, int tb) {
        const int rows = P < NPr ? 4 * P * CP + 4 * tb : 0;
        const float* p = w2y + rows * MW;
#pragma unroll
        for (int g = 0; g < 8; ++g) ay[g] = *reinterpret_cast<const float4*>(p + 16 * g);
        const float4 c0 = *reinterpret_cast<const float4*>(b2p + rows);
        cy = f32x4{c0.x, c0.y, c0.z, c0.w};
      };
      load_y(0, 0);
#pragma clang loop unroll(disable)
      for (int P = 0; P < NPr; ++P) {            // unit group P: 4 hidden units x CP channels = NBr tiles
        float as_P = as[0];
#pragma unroll
        for (int kk = 1; kk < 4 * NV; ++kk) as_P = P == kk ? as[kk] : as_P;
        const bool own = valid && 4 * P + q < Hr;                    // the lane's row (4 P + q, .) exists
        float f = 0.f;
#pragma clang loop unroll(disable)
        for (int tb = 0; tb < NBr; ++tb) {
          const int rows = 4 * P * CP + 4 * tb;
          {
            const float4* p = reinterpret_cast<const float4*>(w2g + rows * MW);      // rows (4 P + q, 4 tb + r): [8 n + T1]
#pragma unroll
            for (int r = 0; r < 4; ++r) { ag[2 * r] = p[r * (MW / 4)]; ag[2 * r + 1] = p[r * (MW / 4) + 1]; }
          }
          __builtin_amdgcn_sched_barrier(0);
          const f32x4 yv = tl_tile_mfma(ay, u, cy);
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
          {
            const bool wrap = tb + 1 >= NBr;
            load_y(wrap ? P + 1 : P, wrap ? 0 : tb + 1);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {                              // K step (P, c = 4 tb + r); 8 independent accumulator chains
            const float rv[8] = {ag[2 * r].x, ag[2 * r].y, ag[2 * r].z, ag[2 * r].w,
                                 ag[2 * r + 1].x, ag[2 * r + 1].y, ag[2 * r + 1].z, ag[2 * r + 1].w};
#pragma unroll
            for (int T1 = 0; T1 < 8; ++T1) gu[T1] = mfma16(rv[T1], g2[r], gu[T1]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < 4 * NV; ++s) f4[s >> 2][s & 3] = P == s ? f : f4[s >> 2][s & 3];
      }

      // ---- dL/dpre1 = gu * hid'(pre1);  va = W1^T dL/dpre1
      float g1[32];
#pragma unroll
      for (int s2 = 0; s2 < 32; ++s2) g1[s2] = hidden_backward<ACT>(gu[s2 >> 2][s2 & 3], (mask >> s2) & 1u, u[s2]);
      if (valid) {
        float* grow = G1 + out_row * G1_COLS + 4 * q;
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1)
          stream_store4(grow + 16 * T1, g1[4 * T1] * wq, g1[4 * T1 + 1] * wq, g1[4 * T1 + 2] * wq, g1[4 * T1 + 3] * wq);
      }
      f32x4 va[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) va[v] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int T1 = 0; T1 < 8; ++T1) {           // K steps (T1, r) in order, NV independent accumulator chains
        float4 at[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) at[v] = w1t[(8 * v + T1) * 64];
#pragma unroll
        for (int v = 0; v < NV; ++v) va[v] = mfma16(at[v].x, g1[4 * T1], va[v]);
#pragma unroll
        for (int v = 0; v < NV; ++v) va[v] = mfma16(at[v].y, g1[4 * T1 + 1], va[v]);
#pragma unroll
        for (int v = 0; v < NV; ++v) va[v] = mfma16(at[v].z, g1[4 * T1 + 2], va[v]);
#pragma unroll
        for (int v = 0; v < NV; ++v) va[v] = mfma16(at[v].w, g1[4 * T1 + 3], va[v]);
      }

      __builtin_amdgcn_sched_barrier(0);
      // ---- reverse-time dynamics: dz/ds = -f, da/ds = +a^T df/dz; torchdiffeq 3/8 rule, association preserved
      const float third = (float)(1.0 / 3.0);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
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
    for (int v = 0; v < NV; ++v) { y[v] = z[v]; a[v] = sa[v]; }
  }
  if (valid) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      store_units4<4>(y_state + series * Hr, 16 * v + q, Hr, y[v]);
      store_units4<4>(a_state + series * Hr, 16 * v + q, Hr, a[v]);
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
template <int NV>
static size_t tiled_lds_bytes(unsigned waves) { return (size_t)(MlpTiled<NV>::L1_FLOATS + waves * TL_SLAB_FLOATS) * sizeof(float); }

template <int NV>
int launch_mlp_tiled_adjoint_images(const TwoLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s) {
  mlp_tiled_adj_image_kernel<NV><<<(MlpTiled<NV>::IMAGE_FLOATS + 255) / 256, 256, 0, s>>>(
      f32(f.W1), f32(f.bias1), f32(f.W2), f32(f.bias2), img, MlpDims{(int)H, (int)C, (int)f.width});
  return check_launch();
}

template <int NV, typename TT>
int launch_forward_mlp_tiled(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                             hipStream_t s) {
  if (!MlpTiled<NV>::shape_ok(n.C, n.H, f.width)) return CDE_ERR_UNSUPPORTED;
  const MlpDims dims{(int)n.H, (int)n.C, (int)f.width};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 8), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = tiled_lds_bytes<NV>(waves);
  const bool vec = (f.width & 3) == 0 && ((uintptr_t)f.W2 & 15) == 0;
  const int rc = dispatch_degree_field(x.degree, f.act, [&](auto D, auto A) {
    auto launch = [&](auto V) {
      auto kernel = rk4_forward_mlp_tiled<NV, TT, D(), A(), V()>;
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

template <int NV, typename TT>
int launch_mlp_tiled_adjoint_sweep(const Control& x, const TiledSweepIO& io, const Shape& n, const StageTable& st, hipStream_t s) {
  if (io.k_end <= io.k_begin) return CDE_OK;
  if (!MlpTiled<NV>::shape_ok(n.C, n.H, 1)) return CDE_ERR_UNSUPPORTED;
  const Dims dims{(int)n.H, (int)n.C};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 4), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = tiled_lds_bytes<NV>(waves);
  const int rc = dispatch_degree_field(x.degree, io.act, [&](auto D, auto A) {
    auto kernel = rk4_adjoint_mlp_tiled_sweep<NV, TT, D(), A()>;
    allow_lds(kernel, lds);
    kernel<<<blocks, 64 * waves, lds, s>>>(f32(x.coeffs), f32(x.knots), x.n_intervals, io.image, f32(io.y_state), f32(io.a_state),
                                    (const TT*)io.grid, io.k_begin, io.k_end, st.index, f32(st.frac), f32(io.U), f32(io.G2),
                                    f32(io.G1), f32(io.Z), f32(io.Z_hi), n.B, dims);
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

#define CDE_INST(NV, TT)                                                                                                   \
  template int launch_forward_mlp_tiled<NV, TT>(const Control&, const TwoLayerField&, const ForwardIO&, const Shape&,      \
                                                const StageTable&, hipStream_t);                                           \
  template int launch_mlp_tiled_adjoint_sweep<NV, TT>(const Control&, const TiledSweepIO&, const Shape&, const StageTable&, \
                                                      hipStream_t);
CDE_INST(2, float)
CDE_INST(2, double)
CDE_INST(4, float)
CDE_INST(4, double)
#undef CDE_INST
template int launch_mlp_tiled_adjoint_images<2>(const TwoLayerField&, int64_t, int64_t, float*, hipStream_t);
template int launch_mlp_tiled_adjoint_images<4>(const TwoLayerField&, int64_t, int64_t, float*, hipStream_t);

}  // namespace cde
