// rk4_affine_tiled.hip -- K2c / K3c: the fused RK4 (3/8 rule) solve and continuous-adjoint sweep of the one-layer vector field
//   f(z) = reshape_{HxC}( act( W z + b ) ) dX,   act = identity or tanh
// on controls of 17 .. 64 channels (float32, H <= 32): cde_affine_tiled.h states the tiling and every layout.  Until these
// kernels such calls fell to the one-lane-per-hidden-unit VALU kernels of rk4_generic.hip.  One wave per 16-series tile; both
// kernels are rk4_mlp_tiled.hip's (NV = 2) without the first layer, with the state itself as the B operand:
//   forward   8 min(H, 8) CP / 4 MFMAs per evaluation (1024 at H = 32, C = 64)
//   sweep     16 min(H, 8) CP / 4 (2048): each tile's Y product and its share of va = W^T dL/dY
// A tile's operands are requested while the MFMAs of the tile before it run (two operand sets in registers, no copies).
#include "cde_affine_tiled.h"

namespace cde {

// ============================================================================================ forward
// VEC: H is a multiple of 4 and W 16-byte aligned -- the lane's eight K steps of a tile are two float4 of W's row (h, c) at
// column 8 q; otherwise eight guarded scalar loads.
template <typename TT, int DEGREE, int ACT, bool VEC>
__global__ __launch_bounds__(512, 2) void rk4_forward_affine_tiled(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ z0,
    const TT* __restrict__ grid, int64_t n_grid, const TT* __restrict__ t_out, int64_t n_out,
    float* __restrict__ z_out, int64_t B, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, Dims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int Hr = dims.H, Cr = dims.C;
  const int CP = (Cr + 3) & ~3, NJr = Hr < 8 ? Hr : 8, NBr = CP >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 16 >= B) return;                                        // (no workgroup barrier in this kernel)
  float* slab = lds + wave * TL_SLAB_FLOATS;
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  f32x4 y[2];                                                        // this lane's units: y[v][i] = unit 8 q + 4 v + i
  at_load_units8(z0 + sc * Hr, q, Hr, y);
  auto store = [&](int64_t j, const f32x4 (&a)[2]) {
    if (valid) at_store_units8(z_out + (series * n_out + j) * Hr, q, Hr, a);
  };
  store(0, y);
  int64_t jout = 1;
  const int64_t n_steps = n_grid - 1;
  if (n_steps <= 0) return;

  // tile (j, tb): the lane's A operands (row (8 (n >> 2) + j, 4 tb + (n & 3)), columns 8 q .. 8 q + 7) and the bias of its D
  // rows (8 q + j, 4 tb + r).  Beyond the real (H, C) -- a tile past the last one included -- zeros, nothing is read.
  auto load_tile = [&](int j, int tb, float4 (&a)[2], f32x4& c4) {
    const int h = 8 * (n >> 2) + j, c = 4 * tb + (n & 3);
    const bool ok = j < NJr && h < Hr && c < Cr;
    const float* p = W + ((int64_t)(ok ? h * Cr + c : 0) * Hr + 8 * q);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int col = 8 * q + 4 * g;
      if constexpr (VEC) {
        a[g] = (ok && col < Hr) ? *reinterpret_cast<const float4*>(p + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        a[g] = make_float4(ok && col < Hr ? p[4 * g] : 0.f, ok && col + 1 < Hr ? p[4 * g + 1] : 0.f,
                           ok && col + 2 < Hr ? p[4 * g + 2] : 0.f, ok && col + 3 < Hr ? p[4 * g + 3] : 0.f);
      }
    }
    const int hb = 8 * q + j;
#pragma unroll
    for (int r = 0; r < 4; ++r) c4[r] = (j < NJr && hb < Hr && 4 * tb + r < Cr) ? bias[hb * Cr + 4 * tb + r] : 0.f;
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

      // ---- the field: W z + b tile by tile (L2) + activation + contraction with dX (LDS slab)
      f32x4 f4[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      {
        int opaque = 0;                         // keeps the LDS reads inside the evaluation (cde_mfma.h: field_act16)
        asm volatile("" : "+v"(opaque));
        const float4* dxs = reinterpret_cast<const float4*>(slab + n * TL_SLAB_STRIDE) + opaque;
        float zs[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) zs[s] = z[s >> 2][s & 3];
        // activation and the tile's four channels of f: even and odd channels in two partial sums (packed FMAs, as Kw)
        auto finish = [&](const f32x4& yv, int tb, f32x2 fp) {
          const f32x2 t01 = activate2<ACT>(yv[0], yv[1]), t23 = activate2<ACT>(yv[2], yv[3]);
          const float4 dx = dxs[tb];
          fp = __builtin_elementwise_fma(t01, f32x2{dx.x, dx.y}, fp);
          return __builtin_elementwise_fma(t23, f32x2{dx.z, dx.w}, fp);
        };
        float4 a0[2], a1[2];
        f32x4 c0, c1;
        load_tile(0, 0, a0, c0);
#pragma clang loop unroll(disable)
        for (int j = 0; j < NJr; ++j) {          // unit group j: 4 hidden units x CP channels = NBr tiles, two per round
          f32x2 fp = {0.f, 0.f};
#pragma clang loop unroll(disable)
          for (int tb = 0; tb < NBr; tb += 2) {
            const bool pair = tb + 1 < NBr;
            load_tile(j, tb + 1, a1, c1);        // (past the group's last tile: zeros)
            __builtin_amdgcn_sched_barrier(0);
            fp = finish(at_tile_mfma(a0, zs, c0), tb, fp);
            __builtin_amdgcn_sched_barrier(0);
            const bool wrap = tb + 2 >= NBr;
            load_tile(wrap ? j + 1 : j, wrap ? 0 : tb + 2, a0, c0);
            __builtin_amdgcn_sched_barrier(0);
            if (pair) fp = finish(at_tile_mfma(a1, zs, c1), tb + 1, fp);
            __builtin_amdgcn_sched_barrier(0);
          }
          const float f = fp[0] + fp[1];
#pragma unroll
          for (int s = 0; s < 8; ++s) f4[s >> 2][s & 3] = j == s ? f : f4[s >> 2][s & 3];
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
// the zero-padded image of cde_affine_tiled.h: [W plain | b | W for va]
__global__ void affine_tiled_image_kernel(const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ img,
                                          Dims d) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= AT_IMAGE_FLOATS) return;
  const int at = e, CP = (d.C + 3) & ~3;
  if (e < AT_B_AT) {                                                 // [row h CP + c][k]
    const int row = e >> 5, k = e & 31, h = row / CP, c = row - h * CP;
    img[at] = (h < d.H && c < d.C && k < d.H) ? W[(h * d.C + c) * d.H + k] : 0.f;
    return;
  }
  e -= AT_B_AT;
  if (e < AT_ROWS) {
    const int h = e / CP, c = e - h * CP;
    img[at] = (h < d.H && c < d.C) ? bias[h * d.C + c] : 0.f;
    return;
  }
  e -= AT_ROWS;                                                      // [four rows (h, 4 tb ..)][i][r][T]
  const int T = e & 1, r = (e >> 1) & 3, i = (e >> 3) & 15, row = 4 * (e >> 7) + r;
  const int h = row / CP, c = row - h * CP, out = 8 * (i >> 2) + 4 * T + (i & 3);
  img[at] = (h < d.H && c < d.C && out < d.H) ? W[(h * d.C + c) * d.H + out] : 0.f;
}

// One chunk of RK steps [k_begin, k_end) of one output interval, reversed time: (z, a) of every series come from and go back
// to y_state / a_state (B x H); the per-stage factors go to Gout [row][MP] / Zout [row][32], row = ((step - k_begin) * 4 +
// stage) * B16 + series.  Per stage and tile (j, tb): Y, activation, f, g = a_h dX_c act'(Y) (streamed, quadrature-weighted),
// va += W^T g.  The tile's va operands are requested before its Y MFMAs, the next tile's Y operands before its va MFMAs.
// One wave per SIMD (256-thread bounds), as K3mc.
template <typename TT, int DEGREE, int ACT>
__global__ __launch_bounds__(256, 1) void rk4_adjoint_affine_tiled_sweep(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ img, float* __restrict__ y_state, float* __restrict__ a_state,
    const TT* __restrict__ sgrid, int64_t k_begin, int64_t k_end, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, float* __restrict__ Gout, float* __restrict__ Zout, int64_t B, int64_t B16, int MP,
    Dims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int Hr = dims.H, Cr = dims.C;
  const int CP = (Cr + 3) & ~3, NJr = Hr < 8 ? Hr : 8, NBr = CP >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 16 >= B) return;                                        // (no workgroup barrier in this kernel)
  float* slab = lds + wave * TL_SLAB_FLOATS;
  const int64_t series = tile * 16 + n;                              // < B16: the padding lanes have rows of their own
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  // lane offsets into the image: Y rows (h = 8 (n >> 2) + j, c & 3 = n & 3) at columns 8 q; the lane's own rows (h = 8 q + j)
  // for the bias, the G columns and -- at 8 n floats -- the va copy
  const int y_off = (8 * (n >> 2) * CP + (n & 3)) * AT_MAX_H + 8 * q;
  const int own_off = 8 * q * CP;

  f32x4 y[2], a[2];                                                  // this lane's units: [v][i] = unit 8 q + 4 v + i
  at_load_units8(y_state + sc * Hr, q, Hr, y);
  at_load_units8(a_state + sc * Hr, q, Hr, a);
  if (!valid) { a[0] = f32x4{0.f, 0.f, 0.f, 0.f}; a[1] = a[0]; }     // a == 0 stays 0: padded lanes contribute nothing

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
      const int64_t out_row = ((k - k_begin) * 4 + stage) * B16 + series;        // (stage, series)

      int opaque = 0;                                                // keeps the LDS / image reads inside the stage
      asm volatile("" : "+v"(opaque));
      const float4* dxs = reinterpret_cast<const float4*>(slab + n * TL_SLAB_STRIDE) + opaque;
      const float* bp = img + AT_B_AT + own_off + opaque;
      const float* wy = img + AT_WP_AT + y_off + opaque;
      const float* wv = img + AT_WT_AT + own_off * AT_MAX_H + 8 * n + opaque;
      float zs[8], as[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) { zs[s] = z[s >> 2][s & 3]; as[s] = sa[s >> 2][s & 3]; }
      {
        float* zrow = Zout + out_row * AT_MAX_H + 8 * q;             // units >= H are zero in z
        stream_store4(zrow, zs[0], zs[1], zs[2], zs[3]);
        stream_store4(zrow + 4, zs[4], zs[5], zs[6], zs[7]);
      }
      __builtin_amdgcn_sched_barrier(0);

      f32x4 va[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      f32x4 f4[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      // Tile (j, tb) of the image starts (8 (n >> 2) + j) CP + 4 tb rows in: below 32 CP <= AT_ROWS for every j < 8.  The
      // request after the last tile is never consumed; it reads tile (0, 0) again.
      float4 ay[2], ag[2];
      f32x4 cy;
      auto load_y = [&](int j, int tb) {
        const int rows = j < NJr ? j * CP + 4 * tb : 0;
        const float* p = wy + rows * AT_MAX_H;
        ay[0] = *reinterpret_cast<const float4*>(p);
        ay[1] = *reinterpret_cast<const float4*>(p + 4);
        const float4 c0 = *reinterpret_cast<const float4*>(bp + rows);
        cy = f32x4{c0.x, c0.y, c0.z, c0.w};
      };
      load_y(0, 0);
#pragma clang loop unroll(disable)
      for (int j = 0; j < NJr; ++j) {            // unit group j: 4 hidden units x CP channels = NBr tiles
        float as_j = as[0];
#pragma unroll
        for (int kk = 1; kk < 8; ++kk) as_j = j == kk ? as[kk] : as_j;
        const bool own = 8 * q + j < Hr;                             // the lane's row (8 q + j, .) exists
        f32x2 fp = {0.f, 0.f};                                       // even and odd channels, as the forward kernel
#pragma clang loop unroll(disable)
        for (int tb = 0; tb < NBr; ++tb) {
          const int rows = j * CP + 4 * tb;
          {
            const float4* p = reinterpret_cast<const float4*>(wv + rows * AT_MAX_H);   // rows (8 q + j, 4 tb + r): [n][r][T]
            ag[0] = p[0]; ag[1] = p[1];
          }
          __builtin_amdgcn_sched_barrier(0);
          const f32x4 yv = at_tile_mfma(ay, zs, cy);
          const f32x2 t01 = activate2<ACT>(yv[0], yv[1]), t23 = activate2<ACT>(yv[2], yv[3]);
          const float tv[4] = {t01[0], t01[1], t23[0], t23[1]};
          const float4 dx4 = dxs[tb];
          const float dx[4] = {dx4.x, dx4.y, dx4.z, dx4.w};
          fp = __builtin_elementwise_fma(t01, f32x2{dx4.x, dx4.y}, fp);
          fp = __builtin_elementwise_fma(t23, f32x2{dx4.z, dx4.w}, fp);
          float g[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = tv[r];
            const float slope = final_tanh(ACT) ? __builtin_fmaf(-t, t, 1.f) : 1.f;
            g[r] = as_j * (dx[r] * slope);
          }
          if (own) {
            float* grow = Gout + out_row * MP + own_off + rows;      // column (8 q + j) CP + 4 tb
            stream_store4(grow, g[0] * wq, g[1] * wq, g[2] * wq, g[3] * wq);
          }
          __builtin_amdgcn_sched_barrier(0);
          {
            const bool wrap = tb + 1 >= NBr;
            load_y(wrap ? j + 1 : j, wrap ? 0 : tb + 1);
          }
          __builtin_amdgcn_sched_barrier(0);
          // K steps (j, c = 4 tb + r); two accumulator chains
          va[0] = mfma16(ag[0].x, g[0], va[0]); va[1] = mfma16(ag[0].y, g[0], va[1]);
          va[0] = mfma16(ag[0].z, g[1], va[0]); va[1] = mfma16(ag[0].w, g[1], va[1]);
          va[0] = mfma16(ag[1].x, g[2], va[0]); va[1] = mfma16(ag[1].y, g[2], va[1]);
          va[0] = mfma16(ag[1].z, g[3], va[0]); va[1] = mfma16(ag[1].w, g[3], va[1]);
          __builtin_amdgcn_sched_barrier(0);
        }
        const float f = fp[0] + fp[1];
#pragma unroll
        for (int s = 0; s < 8; ++s) f4[s >> 2][s & 3] = j == s ? f : f4[s >> 2][s & 3];
      }

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
    at_store_units8(y_state + series * Hr, q, Hr, y);
    at_store_units8(a_state + series * Hr, q, Hr, a);
  }
}

// (z, a) at an output time, torchdiffeq's adjoint: z is re-seeded from the stored forward solution, the incoming gradient of
// that output is added to a (first: a starts from it)
__global__ void affine_tiled_seed_kernel(float* __restrict__ y_state, float* __restrict__ a_state,
                                         const float* __restrict__ z_saved, const float* __restrict__ grad_out, int64_t j,
                                         int64_t n_out, int64_t B, int H, int first) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * H) return;
  const int64_t b = e / H;
  const int h = (int)(e - b * H);
  const int64_t src = (b * n_out + j) * H + h;
  y_state[e] = z_saved[src];
  a_state[e] = first ? grad_out[src] : a_state[e] + grad_out[src];
}

// acc [m = h CP + c][33] = [dW (units 0 .. 31) | db]  ->  grad_W (H C, H), grad_b (H C)
__global__ void affine_tiled_gather_kernel(const float* __restrict__ acc, float* __restrict__ grad_W,
                                           float* __restrict__ grad_b, int H, int C, int CP) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= H * C * (H + 1)) return;
  const int m = e / (H + 1), k = e - m * (H + 1);
  const int h = m / C, c = m - h * C;
  const float v = acc[(h * CP + c) * (AT_MAX_H + 1) + (k < H ? k : AT_MAX_H)];
  if (k < H) grad_W[m * H + k] = v; else grad_b[m] = v;
}

// ------------------------------------------------------------------------------------------ host side
bool affine_tiled_applicable(int64_t C, int64_t H, int dtype, int act) {
  const bool act_ok = act == CDE_ACT_NONE || act == CDE_ACT_TANH;
  return dtype == CDE_F32 && act_ok && H >= 1 && H <= AT_MAX_H && C >= AT_MIN_C && C <= TL_MAX_C;
}

template <typename TT>
int launch_forward_affine_tiled(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                                hipStream_t s) {
  if (!affine_tiled_applicable(n.C, n.H, CDE_F32, f.act)) return CDE_ERR_UNSUPPORTED;
  const Dims dims{(int)n.H, (int)n.C};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 8), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = (size_t)waves * TL_SLAB_FLOATS * sizeof(float);
  const bool vec = (n.H & 3) == 0 && ((uintptr_t)f.W & 15) == 0;
  const int rc = dispatch_degree_act(x.degree, f.act, [&](auto D, auto A) {
    auto launch = [&](auto V) {
      rk4_forward_affine_tiled<TT, D(), A(), V()><<<blocks, 64 * waves, lds, s>>>(
          f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.z0), (const TT*)io.grid, io.n_grid,
          (const TT*)io.t_out, io.n_out, f32(io.z_out), n.B, st.index, f32(st.frac), dims);
    };
    if (vec) launch(std::true_type{}); else launch(std::false_type{});
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

// workspace of the backward pass behind the stage tables (cde_affine_tiled.h)
struct AffineTiledLayout {
  size_t off_y, off_a, off_acc, off_partial, off_image, off_G, off_Z, total, G_bytes;
  int64_t chunk_steps, B16;
  int MP, CP;
};
constexpr size_t AT_SCRATCH_BYTES = (size_t)4 << 30;                  // factor chunk: at most 4 GB (288 GB of HBM per GPU)

static AffineTiledLayout affine_tiled_layout(int64_t B, int64_t C, int64_t H, int64_t n_steps) {
  AffineTiledLayout L;
  L.CP = (int)((C + 3) / 4 * 4);
  L.MP = (int)((H * L.CP + 255) / 256 * 256);
  L.B16 = (B + 15) / 16 * 16;                                         // the sweep writes rows for the padding lanes too
  const int64_t opt = option(CDE_OPT_WIDE_SCRATCH_BYTES);             // (tests: tiny chunks)
  const size_t budget = opt > 0 ? (size_t)opt : AT_SCRATCH_BYTES;
  const size_t row_bytes = (size_t)(L.MP + AT_MAX_H) * sizeof(float);
  int64_t steps = (int64_t)(budget / (row_bytes * 4 * (size_t)(L.B16 > 0 ? L.B16 : 1)));
  steps = steps < 1 ? 1 : steps;
  steps = steps > n_steps ? (n_steps > 0 ? n_steps : 1) : steps;
  L.chunk_steps = steps;
  const size_t rows = (size_t)steps * 4 * (size_t)L.B16;
  L.G_bytes = rows * L.MP * sizeof(float);
  L.off_y = 0;
  L.off_a = L.off_y + align256((size_t)B * H * sizeof(float));
  L.off_acc = L.off_a + align256((size_t)B * H * sizeof(float));
  L.off_partial = L.off_acc + align256((size_t)L.MP * (AT_MAX_H + 1) * sizeof(float));
  L.off_image = L.off_partial + align256(wide_grad_reduce_partial_bytes(L.MP, AT_MAX_H));
  L.off_G = L.off_image + align256((size_t)AT_IMAGE_FLOATS * sizeof(float));
  L.off_Z = L.off_G + align256(L.G_bytes);
  L.total = L.off_Z + align256(rows * AT_MAX_H * sizeof(float));
  return L;
}
size_t affine_tiled_adjoint_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t n_steps) {
  return affine_tiled_layout(B, C, H, n_steps).total;
}

template <typename TT>
int launch_adjoint_affine_tiled(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                                void* scratch, hipStream_t s) {
  const int64_t B = n.B, H = n.H, C = n.C;
  const Dims dims{(int)H, (int)C};
  if (x.degree != CDE_PATH_CUBIC && x.degree != CDE_PATH_LINEAR) return CDE_ERR_UNSUPPORTED;
  if (!affine_tiled_applicable(C, H, CDE_F32, f.act)) return CDE_ERR_UNSUPPORTED;
  // the chunk loop runs on the host and reads the segment offsets from the caller's HOST copy, as launch_adjoint_wide does
  if (io.n_out > 1 && !io.seg_off_host) return CDE_ERR_NULL;
  const AffineTiledLayout L = affine_tiled_layout(B, C, H, io.n_sgrid - 1);
  unsigned char* base = (unsigned char*)scratch;
  float* y_state = (float*)(base + L.off_y);
  float* a_state = (float*)(base + L.off_a);
  float* acc = (float*)(base + L.off_acc);
  float* partial = (float*)(base + L.off_partial);
  float* img = (float*)(base + L.off_image);
  float* Gbuf = (float*)(base + L.off_G);
  float* Zbuf = (float*)(base + L.off_Z);
  const int64_t tiles = (B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 4), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = (size_t)waves * TL_SLAB_FLOATS * sizeof(float);
  const unsigned seed_blocks = (unsigned)((B * H + 255) / 256);
  zero_async(acc, (size_t)L.MP * (AT_MAX_H + 1) * sizeof(float), s);
  if (L.MP > H * L.CP && io.n_out > 1) zero_async(Gbuf, L.G_bytes, s);                 // the columns no lane writes
  affine_tiled_image_kernel<<<(AT_IMAGE_FLOATS + 255) / 256, 256, 0, s>>>(f32(f.W), f32(f.bias), img, dims);
  affine_tiled_seed_kernel<<<seed_blocks, 256, 0, s>>>(y_state, a_state, f32(io.z_saved), f32(io.grad_out), io.n_out - 1,
                                                       io.n_out, B, (int)H, 1);
  int rc = check_launch();
  if (rc != CDE_OK) return rc;
  auto sweep = [&](int64_t k, int64_t ke) {              // steps [k, ke) of the reversed grid
    return dispatch_degree_act(x.degree, f.act, [&](auto D, auto A) {
      rk4_adjoint_affine_tiled_sweep<TT, D(), A()><<<blocks, 64 * waves, lds, s>>>(
          f32(x.coeffs), f32(x.knots), x.n_intervals, img, y_state, a_state, (const TT*)io.sgrid, k, ke, st.index,
          f32(st.frac), Gbuf, Zbuf, B, L.B16, L.MP, dims);
      return CDE_OK;
    });
  };
  for (int64_t p = 0; p + 1 < io.n_out; ++p) {
    int64_t k = io.seg_off_host[p];
    const int64_t k_end = io.seg_off_host[p + 1] - 1;
    while (k < k_end) {
      const int64_t ke = k + L.chunk_steps < k_end ? k + L.chunk_steps : k_end;
      rc = sweep(k, ke);
      if (rc != CDE_OK) return rc;
      rc = check_launch();
      if (rc != CDE_OK) return rc;
      rc = launch_wide_grad_reduce(Gbuf, Zbuf, 4 * (ke - k) * L.B16, L.MP, AT_MAX_H, acc, partial, s);
      if (rc != CDE_OK) return rc;
      k = ke;
    }
    affine_tiled_seed_kernel<<<seed_blocks, 256, 0, s>>>(y_state, a_state, f32(io.z_saved), f32(io.grad_out),
                                                         io.n_out - 2 - p, io.n_out, B, (int)H, 0);
  }
  if (hipMemcpyAsync(io.grad_z0, a_state, (size_t)B * H * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return CDE_ERR_LAUNCH;
  affine_tiled_gather_kernel<<<(unsigned)((H * C * (H + 1) + 255) / 256), 256, 0, s>>>(acc, f32(io.grad_W), f32(io.grad_b),
                                                                                      (int)H, (int)C, L.CP);
  return check_launch();
}

#define CDE_INST(TT)                                                                                                          \
  template int launch_forward_affine_tiled<TT>(const Control&, const AffineField&, const ForwardIO&, const Shape&,            \
                                               const StageTable&, hipStream_t);                                               \
  template int launch_adjoint_affine_tiled<TT>(const Control&, const AffineField&, const AdjointIO&, const Shape&,            \
                                               const StageTable&, void*, hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
