// revheun.hip -- the reversible Heun method (Kidger et al., arXiv 2105.13493, Algorithms 1 and 2) for the one-layer
// fields f(z) = reshape_{HxC}(act(W z + b)) dX, f32, H <= 32, C <= 8, cubic and linear controls:
// cdeint(..., backend="torchsde", method="reversible_heun").
//
// The carried state is (y, zh, f) with zh_0 = y_0 = z0, f_0 = F(t_0, z0), and a step over dt = grid[k+1] - grid[k] is
//     zh_{k+1} = 2 y_k - zh_k + f_k dt        f_{k+1} = F(t_{k+1}, zh_{k+1})        y_{k+1} = y_k + (f_k + f_{k+1}) dt/2
// -- ONE field evaluation per step.  The step is algebraically invertible, so the backward pass keeps nothing but
// (y_N, zh_N): it walks the nodes N .. 0, rebuilds (y, zh) as it goes and differentiates the steps themselves -- the exact
// gradient of the discrete solve (what autograd through the recurrences gives) from one evaluation-and-VJP per node.
//
//   RHf  forward: K2's skeleton (rk4_mfma.hip) -- one wave per 16 series, two waves per SIMD, the weight image resident as
//        in field16 (identity, registers) / field_act16 (tanh, LDS); three state vectors per lane; also writes zh_N.
//   RHa  backward: one wave per 32 series, five carried vectors (y, zh, ybar, zbar, fbar -- f_{k+1} is folded into y, see
//        below; no scratch: tests/test_kernel_reversible_heun.py); every node is K3a's
//        stage (rk4_mfma.hip: rk4_adjoint_act_mfma) with quadrature weight 1 -- the pre-activation GEMM, the in-lane
//        slope, W^T g, and dL/dW with the batch as MFMA K through the transposed scratch tile.  Per-wave partial
//        parameter gradients in K3's layout, summed in a fixed order by launch_reduce_partials (deterministic).
//        Output gradients arrive as K3d's node lists (the transpose of the linear output interpolation).
// The interval index / fractional part of every grid node comes from the node table (api.hip: node_table_kernel, the
// stage table's `locate`), so X.derivative at a knot means what CubicSpline._interpret_t means.
#include "cde_mfma.h"
#include "cde_launch.h"

namespace cde {

__device__ __forceinline__ void rh_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void rh_swap32(float& x, float& y) {   // x[lanes 32..63] <-> y[lanes 0..31]
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  x = __uint_as_float(r[0]);
  y = __uint_as_float(r[1]);
}

// ============================================================================================ forward
// RHf.  Lane l = (n = l & 15, q = l >> 4) of a wave keeps 8 hidden units of series n (identity: 8q .. 8q+7; tanh:
// q, 4+q, .., 28+q -- the ownership of field16 / field_act16) of y, zh and f.
constexpr int RH_FWD_THREADS = 512;

template <typename TT, int DEGREE, int ACT>
__global__ __launch_bounds__(RH_FWD_THREADS, 2) void revheun_forward_mfma(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ z0,
    const TT* __restrict__ grid, int64_t n_grid, const TT* __restrict__ t_out, int64_t n_out,
    float* __restrict__ z_out, float* __restrict__ zhat_out, int64_t B, const int64_t* __restrict__ node_index,
    const float* __restrict__ node_frac, Dims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool PRODUCT = ACT == CDE_ACT_NONE;
  constexpr int STRIDE = PRODUCT ? 1 : 4;          // distance between a lane's consecutive hidden units
  float4 wA[PRODUCT ? W16_GROUPS : 1], wB[PRODUCT ? W16_GROUPS : 1];
  if constexpr (PRODUCT) load_w16(W, bias, lds, wA, wB, dims);
  else stage_wy16(W, bias, lds, dims);
  const int Hr = dims.H, Cr = dims.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (RH_FWD_THREADS / 64) + wave;
  if (tile * 16 >= B) return;
  // (waves w and w + 4 share a SIMD: half an evaluation of head start for one of them, as in K2)
  if (__builtin_amdgcn_readfirstlane(wave) >= 4) __builtin_amdgcn_s_sleep(FWD_STAGGER_SLEEP);
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;

  const int ua = PRODUCT ? 8 * q : q, ub = PRODUCT ? 8 * q + 4 : 16 + q;
  const float4* wy = reinterpret_cast<const float4*>(lds) + lane;              // activation form: LDS images
  const float4* by = reinterpret_cast<const float4*>(lds + WY_FLOATS) + q;
  f32x4 ya = load_units4<STRIDE>(z0 + sc * Hr, ua, Hr), yb = load_units4<STRIDE>(z0 + sc * Hr, ub, Hr);
  auto store = [&](int64_t j, const f32x4& a, const f32x4& b) {
    if (valid) {
      float* row = z_out + (series * n_out + j) * Hr;
      store_units4<STRIDE>(row, ua, Hr, a);
      store_units4<STRIDE>(row, ub, Hr, b);
    }
  };
  store(0, ya, yb);
  f32x4 zha = ya, zhb = yb;
  const int64_t n_steps = n_grid - 1;
  if (n_steps > 0) {
    int64_t idx = node_index[0];
    float frac = node_frac[0];
    Row<DEGREE> row = load_row<DEGREE>(coeffs, sc, n_intervals, idx, Cr);
    auto field = [&](const f32x4& za, const f32x4& zb, f32x4& fa, f32x4& fb) {
      float dX[MC];
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      control_slope<DEGREE>(row, frac, width, dX);
      if constexpr (PRODUCT) field16(wA, wB, za, zb, dX, q, fa, fb);
      else field_act16<ACT>(wy, by, za, zb, dX, fa, fb);
    };
    f32x4 fa, fb;
    field(zha, zhb, fa, fb);                                      // f_0 = F(t_0, z0)
    int64_t jout = 1;
    for (int64_t k = 0; k < n_steps; ++k) {
      const TT t0 = grid[k], t1 = grid[k + 1];
      const float dt = (float)(t1 - t0);
      const int64_t nidx = node_index[k + 1];
      frac = node_frac[k + 1];
      if (nidx != idx) row = load_row<DEGREE>(coeffs, sc, n_intervals, nidx, Cr);
      idx = nidx;
      zha = 2.f * ya - zha + fa * dt;
      zhb = 2.f * yb - zhb + fb * dt;
      f32x4 ga, gb;
      field(zha, zhb, ga, gb);                                    // f_{k+1} = F(t_{k+1}, zh_{k+1})
      const float half_dt = 0.5f * dt;
      const f32x4 y1a = ya + (fa + ga) * half_dt, y1b = yb + (fb + gb) * half_dt;
      while (jout < n_out && t1 >= t_out[jout]) {                 // outputs: linear between grid points, as K2
        const TT tj = t_out[jout];
        if (tj == t0) store(jout, ya, yb);
        else if (tj == t1) store(jout, y1a, y1b);
        else {
          const float slope = (float)((tj - t0) / (t1 - t0));
          store(jout, ya + slope * (y1a - ya), yb + slope * (y1b - yb));
        }
        ++jout;
      }
      ya = y1a; yb = y1b; fa = ga; fb = gb;
    }
  }
  if (valid) {
    store_units4<STRIDE>(zhat_out + series * Hr, ua, Hr, zha);
    store_units4<STRIDE>(zhat_out + series * Hr, ub, Hr, zhb);
  }
}

// ============================================================================================ backward
// RHa.  Ownership as K3 / K3a: one wave = 32 series, lane (n = l & 31, half = l >> 5) keeps hidden units 2r + half.
// With dt = grid[k] - grid[k-1] the node k (k = N .. 1) does
//     a    = fbar_k + ybar_k dt/2                       (cotangent of f_k)
//     f_k  = F(t_k, zh_k),  v = (dF/dz)^T a,  dL/dtheta += (dF/dtheta)^T a        -- K3a's stage
//     y_k  = (y_{k+1} - f_{k+1} dt_k/2) - f_k dt_k/2    (k < N: y lags one node, it needs f_k)
//     zt   = zbar_k + v
//     fbar_{k-1} = ybar_k dt/2 + zt dt,   ybar_{k-1} = ybar_k + 2 zt + (output gradients on node k-1),   zbar_{k-1} = -zt
//     zh_{k-1}   = 2 y_k - zh_k - f_k dt
// and node 0 evaluates at zh_0 (= y_0 = z0) with cotangent fbar_0:  dL/dz0 = ybar_0 + zbar_0 + v.
constexpr int RH_WV32_FLOATS = 8 * 16 * 64;          // one 32x32x2 image: 8 tiles x 16 K steps x 64 lanes
constexpr int RH_BY32_FLOATS = 8 * 2 * 16;           // bias image [tile][half][register]
constexpr int RH_SCRA_FLOATS = 2 * 64 * 20;          // per wave: z^T and one transposed g tile
constexpr int RH_ADJ_LDS_FLOATS = 2 * RH_WV32_FLOATS + RH_BY32_FLOATS + 4 * RH_SCRA_FLOATS;
constexpr int64_t RH_PARTIAL_FLOATS = MH * MC * MH + MH * MC;      // K3's per-wave layout (launch_reduce_partials)

__device__ __forceinline__ float rh_wy32_image(const float* __restrict__ W, int T, int s, int l, Dims d) {
  const int i = l & 31, hk = l >> 5;
  const int h = 4 * T + (i >> 3), c = i & 7, k = 2 * s + hk;
  return (h < d.H && c < d.C && k < d.H) ? W[(h * d.C + c) * d.H + k] : 0.f;
}
__device__ __forceinline__ float rh_wv32_image(const float* __restrict__ W, int T, int r, int l, Dims d) {
  const int k = rho(l & 31), hk = l >> 5;
  const int h = 4 * T + (r >> 2), c = (r & 3) + 4 * hk;
  return (h < d.H && c < d.C && k < d.H) ? W[(h * d.C + c) * d.H + k] : 0.f;
}
template <int ACT>
__device__ __forceinline__ float rh_slope(float t) { return ACT == CDE_ACT_TANH ? __builtin_fmaf(-t, t, 1.f) : 1.f; }

template <typename TT, int DEGREE, int ACT>
__global__ __launch_bounds__(256, 1) void revheun_adjoint_mfma(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ y_final,
    const float* __restrict__ zhat_final, const float* __restrict__ grad_out, const TT* __restrict__ grid, int64_t n_grid,
    const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ node_out, const float* __restrict__ node_weight,
    int64_t n_out, float* __restrict__ grad_z0, float* __restrict__ partial, int64_t B,
    const int64_t* __restrict__ node_index, const float* __restrict__ node_frac, Dims dims) {
  const int Hr = dims.H, Cr = dims.C;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wyf = lds;
  float* wvf = lds + RH_WV32_FLOATS;
  float* byf = lds + 2 * RH_WV32_FLOATS;
  for (int e = threadIdx.x; e < RH_WV32_FLOATS; e += 256) {
    const int j = e & 3, l = (e >> 2) & 63, g = e >> 8;             // g = 4T + (step >> 2)
    wyf[e] = rh_wy32_image(W, g >> 2, 4 * (g & 3) + j, l, dims);
    wvf[e] = rh_wv32_image(W, g >> 2, 4 * (g & 3) + j, l, dims);
  }
  for (int e = threadIdx.x; e < RH_BY32_FLOATS; e += 256) {
    const int r = e & 15, hf = (e >> 4) & 1, T = e >> 5;
    const int h = 4 * T + (r >> 2), c = (r & 3) + 4 * hf;
    byf[e] = (h < Hr && c < Cr) ? bias[h * Cr + c] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, half = lane >> 5;
  const float4* wy = reinterpret_cast<const float4*>(wyf) + lane;
  const float4* wv = reinterpret_cast<const float4*>(wvf) + lane;
  const float4* by = reinterpret_cast<const float4*>(byf) + 4 * half;
  float* scr_zt = lds + 2 * RH_WV32_FLOATS + RH_BY32_FLOATS + wave * RH_SCRA_FLOATS;   // 64 rows x 20
  float* scr_g = scr_zt + 64 * 20;                                                     // 64 rows x 20

  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  float* my_partial = partial + tile * RH_PARTIAL_FLOATS;
  if (tile * 32 >= B) return;   // the host sizes `partial` by the number of live tiles only
  const int64_t series = tile * 32 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;

  f32x16 accW[8];
  float gb[8];
#pragma unroll
  for (int T = 0; T < 8; ++T) {
    gb[T] = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) accW[T][r] = 0.f;
  }
  // the output gradients that land on grid node m (padded lanes keep a zero cotangent: they add nothing to dL/dW)
  auto add_outputs = [&](int64_t m, f32x16& g) {
    const float* go = grad_out + sc * n_out * Hr + half;
    for (int64_t e = node_ptr[m]; e < node_ptr[m + 1]; ++e) {
      const int64_t j = node_out[e];
      const float wgt = node_weight[e];
      if (valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (2 * r + half < Hr) g[r] = __builtin_fmaf(wgt, go[j * Hr + 2 * r], g[r]);
      }
    }
  };

  const int64_t n_steps = n_grid - 1;
  // five carried vectors: yh = y_{k+1} - f_{k+1} dt_k/2 (y_N at the start; y_k follows once f_k is known), zh, ybar, zbar,
  // and `ast`, which holds fbar_k between two nodes and the cotangent of f_k inside one
  f32x16 yh, zh, ybar, zbar, ast;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int u = 2 * r + half;
    const bool on = u < Hr;
    yh[r] = on ? y_final[sc * Hr + u] : 0.f;
    zh[r] = on ? zhat_final[sc * Hr + u] : 0.f;
    ybar[r] = 0.f; zbar[r] = 0.f; ast[r] = 0.f;
  }
  add_outputs(n_steps, ybar);

  int64_t idx = node_index[n_steps];
  float frac = node_frac[n_steps];
  Row<DEGREE> row = load_row<DEGREE>(coeffs, sc, n_intervals, idx, Cr);
  float dt_next = 0.f;                                   // grid[k+1] - grid[k]
  for (int64_t k = n_steps; k >= 0; --k) {
    const float dt = k > 0 ? (float)(grid[k] - grid[k - 1]) : 0.f;
    const float half_dt = 0.5f * dt;
    float dX[MC];
    const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
    control_slope<DEGREE>(row, frac, width, dX);
    // this half's 4 channels
    const float dh[4] = {half ? dX[4] : dX[0], half ? dX[5] : dX[1], half ? dX[6] : dX[2], half ? dX[7] : dX[3]};
    if (k > 0) ast = ast + ybar * half_dt;               // cotangent of f_k

    // z^T for the dL/dW products (K3's layout): scr_zt[(par*32 + u)*20 + s] = z_u of series 2s+par
    {
      float* wz = scr_zt + ((n & 1) * 32 + half) * 20 + (n >> 1);
#pragma unroll
      for (int r = 0; r < 16; ++r) wz[r * 40] = zh[r];
      rh_wave_lds_sync();
    }
    f32x16 f, va = zbar;                      // the W^T g products accumulate onto zbar: va ends as zt = zbar + v
    int opaque = 0;
    asm volatile("" : "+v"(opaque));          // keeps the image reads inside the node (no hoisting)
    const float4* wys = wy + opaque;
    const float4* wvs = wv + opaque;
    const float4* bys = by + opaque;
#pragma unroll
    for (int T = 0; T < 8; ++T) {
      // ---- Y tile = W_T zh + b_T: lane (n, half) register r = Y[h = 4T + (r>>2)][c = (r&3) + 4 half]
      f32x16 yt;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 b4 = bys[T * 8 + g4];
        yt[4 * g4] = b4.x; yt[4 * g4 + 1] = b4.y; yt[4 * g4 + 2] = b4.z; yt[4 * g4 + 3] = b4.w;
      }
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 a4 = wys[(4 * T + g4) * 64];
        yt = mfma(a4.x, zh[4 * g4], yt);
        yt = mfma(a4.y, zh[4 * g4 + 1], yt);
        yt = mfma(a4.z, zh[4 * g4 + 2], yt);
        yt = mfma(a4.w, zh[4 * g4 + 3], yt);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- activation, contraction with dX, dL/dY.  The cotangent of units 4T..4T+3 in every lane: swap32 of two copies
      // broadcasts both halves' values
      float ae0 = ast[2 * T], ao0 = ast[2 * T], ae1 = ast[2 * T + 1], ao1 = ast[2 * T + 1];
      rh_swap32(ae0, ao0);
      rh_swap32(ae1, ao1);
      const float a4u[4] = {ae0, ao0, ae1, ao1};
      float ps[4], g[16];
#pragma unroll
      for (int hl = 0; hl < 4; ++hl) {
        float acc = 0.f;
        const f32x2 tp[2] = {activate2<ACT>(yt[4 * hl], yt[4 * hl + 1]), activate2<ACT>(yt[4 * hl + 2], yt[4 * hl + 3])};
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) {
          const float t = tp[cl >> 1][cl & 1];
          acc = cl == 0 ? t * dh[0] : __builtin_fmaf(t, dh[cl], acc);
          g[4 * hl + cl] = a4u[hl] * (dh[cl] * rh_slope<ACT>(t));
        }
        ps[hl] = acc;
      }
      rh_swap32(ps[0], ps[1]);
      rh_swap32(ps[2], ps[3]);
      f[2 * T] = ps[0] + ps[1];
      f[2 * T + 1] = ps[2] + ps[3];
      __builtin_amdgcn_sched_barrier(0);
      // ---- va += W_T^T g
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 a4 = wvs[(4 * T + g4) * 64];
        va = mfma(a4.x, g[4 * g4], va);
        va = mfma(a4.y, g[4 * g4 + 1], va);
        va = mfma(a4.z, g[4 * g4 + 2], va);
        va = mfma(a4.w, g[4 * g4 + 3], va);
      }
      // ---- dW_T += g^T zh through the transposed scratch tile; dL/db is the row sum of the same tile
      {
        float* wg = scr_g + ((n & 1) * 32 + 4 * half) * 20 + (n >> 1);     // + row(r) * 20, row = (r&3) + 8*(r>>2)
#pragma unroll
        for (int r = 0; r < 16; ++r) wg[((r & 3) + 8 * (r >> 2)) * 20] = g[r];
        rh_wave_lds_sync();
        const float4* g4p = reinterpret_cast<const float4*>(scr_g + (half * 32 + n) * 20);
        float gA[16];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 v = g4p[g4];
          gA[4 * g4] = v.x; gA[4 * g4 + 1] = v.y; gA[4 * g4 + 2] = v.z; gA[4 * g4 + 3] = v.w;
        }
        rh_wave_lds_sync();                      // reads retired before the next tile overwrites the scratch
        float zB[16];                            // zh^T of this lane's K steps (re-read per tile: 4 b128 against 16 live registers)
        const float4* zt4 = reinterpret_cast<const float4*>(scr_zt + (half * 32 + n) * 20) + opaque;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 v = zt4[g4];
          zB[4 * g4] = v.x; zB[4 * g4 + 1] = v.y; zB[4 * g4 + 2] = v.z; zB[4 * g4 + 3] = v.w;
        }
        float rs = 0.f;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          accW[T] = mfma(gA[s2], zB[s2], accW[T]);
          rs += gA[s2];
        }
        gb[T] += rs;
        asm volatile("" : "+v"(gb[T]));          // (only read after the solve: left alone, the optimiser sinks the row sums
                                                 //  below the last tile and keeps every tile's 16 values alive until then)
      }
      __builtin_amdgcn_sched_barrier(0);       // one tile at a time: bounds the live registers
    }

    if (k == 0) {                              // dL/dz0 = ybar_0 + zbar_0 + (dF/dz)^T fbar_0
      ybar = ybar + va;
      break;
    }
    const f32x16 y = yh - f * (0.5f * dt_next);          // y_k (dt_next = 0 at node N: yh is y_N itself)
    ast = ybar * half_dt + va * dt;                      // fbar_{k-1}
    ybar = ybar + 2.f * va;
    add_outputs(k - 1, ybar);
    zbar = -va;
    zh = 2.f * y - zh - f * dt;
    yh = y - f * half_dt;
    dt_next = dt;
    // the next node's table entry and (if the interval changes) its control row -- after the stage, which is register-bound
    const int64_t nidx = node_index[k - 1];
    frac = node_frac[k - 1];
    if (nidx != idx) row = load_row<DEGREE>(coeffs, sc, n_intervals, nidx, Cr);
    idx = nidx;
  }

  if (valid) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (2 * r + half < Hr) grad_z0[series * Hr + 2 * r + half] = ybar[r];
  }
  // per-wave partials in the K3 layout: tile T register r of lane (n, half) is dW[h = 4T + (r>>2)][c = (r&3) + 4 half][k = n]
#pragma unroll
  for (int T = 0; T < 8; ++T) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int h = 4 * T + (r >> 2), c = (r & 3) + 4 * half;
      my_partial[(h * MC + c) * MH + n] = accW[T][r];
    }
    // row sums: lane (i = n, half) summed row i = (h = 4T + (n>>3), c = n&7) over the series of its parity
    const float other = __shfl_xor(gb[T], 32, 64);
    if (half == 0) my_partial[MH * MC * MH + 32 * T + n] = gb[T] + other;
  }
}

// ------------------------------------------------------------------------------------------ host side
bool revheun_applicable(int64_t C, int64_t H, int dtype, int act) { return mfma_applicable(C, H, dtype, act); }

template <typename TT>
int launch_revheun_forward(const Control& x, const AffineField& f, const ForwardIO& io, void* zhat_out, const Shape& n,
                           const StageTable& nodes, hipStream_t s) {
  const Dims dims{(int)n.H, (int)n.C};
  const int rc = dispatch_degree_act(x.degree, f.act, [&](auto D, auto A) {
    revheun_forward_mfma<TT, D(), A()>
        <<<(unsigned)((n.B + RH_FWD_THREADS / 4 - 1) / (RH_FWD_THREADS / 4)), RH_FWD_THREADS,
           (A() == CDE_ACT_NONE ? W16_FLOATS : ACT16_LDS_FLOATS) * sizeof(float), s>>>(
            f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.z0), (const TT*)io.grid, io.n_grid,
            (const TT*)io.t_out, io.n_out, f32(io.z_out), f32(zhat_out), n.B, nodes.index, f32(nodes.frac), dims);
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

template <typename TT>
int launch_revheun_adjoint(const Control& x, const AffineField& f, const ReversibleIO& io, const Shape& n,
                           const StageTable& nodes, float* partial, hipStream_t s) {
  const Dims dims{(int)n.H, (int)n.C};
  const unsigned blocks = (unsigned)((n.B + 127) / 128);
  const size_t lds = (size_t)RH_ADJ_LDS_FLOATS * sizeof(float);
  int rc = dispatch_degree_act(x.degree, f.act, [&](auto D, auto A) {
    auto kernel = revheun_adjoint_mfma<TT, D(), A()>;
    allow_lds(kernel, lds);
    kernel<<<blocks, 256, lds, s>>>(f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.y_final),
                                    f32(io.zhat_final), f32(io.grad_out), (const TT*)io.grid, io.n_grid, io.node_ptr,
                                    io.node_out, io.node_weight, io.n_out, f32(io.grad_z0), partial, n.B, nodes.index,
                                    f32(nodes.frac), dims);
    return CDE_OK;
  });
  if (rc == CDE_OK) rc = check_launch();
  if (rc != CDE_OK) return rc;
  return launch_reduce_partials(partial, (n.B + 31) / 32, io.grad_W, io.grad_b, (int)n.H, (int)n.C, s);
}

#define CDE_INST(TT)                                                                                                  \
  template int launch_revheun_forward<TT>(const Control&, const AffineField&, const ForwardIO&, void*, const Shape&,   \
                                          const StageTable&, hipStream_t);                                            \
  template int launch_revheun_adjoint<TT>(const Control&, const AffineField&, const ReversibleIO&, const Shape&,       \
                                          const StageTable&, float*, hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
