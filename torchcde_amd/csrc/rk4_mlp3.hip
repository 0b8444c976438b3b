// rk4_mlp3.hip -- K2m3 / K3m3: the fused RK4 (3/8 rule) solve and continuous-adjoint sweep of the three-layer vector field
//   f(z) = reshape_{HxC}( act( W2 hid( Wm hid(W1 z + b1) + bm ) + b2 ) ) dX       (cde_mlp3.h)
// one wave per 16-series tile, float32, H <= 32, C <= 8, both hidden widths <= 128; no shared-tile forms (a 32-series call
// runs two waves), no 16-channel layout.  Both kernels are K2m / K3m (rk4_mfma.hip, rk4_mlp_adjoint.hip) with the middle
// layer between their layer 1 and layer 2:
//   forward   64 + 256 + 512 = 832 MFMAs per evaluation (K2m: 576)
//   sweep     64 + 256 + 512 + 512 + 256 + 64 = 1664 (K3m: 1152): the middle layer, and its transpose for dL/du1
// Layer 1, layer 2 and their biases read K2m's / K3m's LDS images (layer 1 built for width1, layer 2 for width2); the middle
// layer's A operands come from L2 -- the sweep's from the two images cde_rk4_adjoint_mlp3_prepare leaves in the workspace,
// the forward kernel's straight from the caller's Wm (cde_mlp3.h).
// The sweep streams, per (stage, series), the factor rows of K3m with two more:
//     U1 [132]  hid(W1 z + b1) | 1 | 0 0 0       Gm [256]  w ds dL/dpre2 in columns 0..127 (128..255: the caller's zeros)
//     U  [132]  hid(Wm u1 + bm) | 1 | 0 0 0      G2, G1, Z as K3m
// and the caller reduces  dW2 | db2 = G2^T U,  dWm | dbm = Gm^T U1,  dW1 | db1 = G1^T Z  (cde_mlp_grad_reduce: layer 2, layer 2,
// layer 1 -- Gm is padded to the 256 columns of the existing form, so the reduction's two forms stay as they are).
#include "cde_mlp3.h"

namespace cde {

// ============================================================================================ forward
// VEC: width1 is a multiple of 4 and Wm 16-byte aligned -- the lane's four K steps of a middle-layer tile are one float4 of
// Wm's row 16 T' + i at column 16 T1 + 4 kq; otherwise four guarded scalar loads.  Rows beyond width2 and columns beyond
// width1 read as zero either way (what the sweep's padded image holds: the same bits in u2).
template <typename TT, int DEGREE, int ACT, bool VEC>
__global__ __launch_bounds__(512, 2) void rk4_forward_mlp3(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W1, const float* __restrict__ bias1, const float* __restrict__ Wm,
    const float* __restrict__ biasm, const float* __restrict__ W2, const float* __restrict__ bias2,
    const float* __restrict__ z0, const TT* __restrict__ grid, int64_t n_grid, const TT* __restrict__ t_out, int64_t n_out,
    float* __restrict__ z_out, int64_t B, const int64_t* __restrict__ stage_index, const float* __restrict__ stage_frac,
    Mlp3Dims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  {
    const MlpDims d1{dims.H, dims.C, dims.w1}, d2{dims.H, dims.C, dims.w2};
    for (int e = threadIdx.x; e < MLP16_LDS_FLOATS; e += blockDim.x)
      lds[e] = mlp16_image(W1, bias1, W2, bias2, e, e < W1M_FLOATS + B1M_FLOATS ? d1 : d2);
    for (int e = threadIdx.x; e < BMM_FLOATS; e += blockDim.x) lds[MLP16_LDS_FLOATS + e] = bm_image(biasm, e, dims.w2);
    __syncthreads();
  }
  const int Hr = dims.H, Cr = dims.C, w1r = dims.w1, w2r = dims.w2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // (1 .. 8 waves per workgroup: cde_launch.h, waves_per_workgroup)
  if (tile * 16 >= B) return;
  // (waves w and w + 4 share a SIMD: half a stage of head start for one of them, as in K2)
  if (__builtin_amdgcn_readfirstlane(wave) >= 4) __builtin_amdgcn_s_sleep(FWD_STAGGER_SLEEP);
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  const int ua = q, ub = 16 + q;                                   // this lane's units: q, 4+q, .., 28+q
  f32x4 ya = load_units4<4>(z0 + sc * Hr, ua, Hr), yb = load_units4<4>(z0 + sc * Hr, ub, Hr);
  auto store = [&](int64_t j, const f32x4& a, const f32x4& b) {
    if (valid) {
      float* row = z_out + (series * n_out + j) * Hr;
      store_units4<4>(row, ua, Hr, a);
      store_units4<4>(row, ub, Hr, b);
    }
  };
  store(0, ya, yb);
  int64_t jout = 1;
  const int64_t n_steps = n_grid - 1;
  if (n_steps <= 0) return;

  // the lane's A operand of the middle layer: row 16 T' + n of Wm, columns 16 T1 + 4 q .. + 3
  const float* wm_lane = Wm + n * w1r + 4 * q;
  auto load_wm = [&](int Tp, int T1) -> float4 {
    const int row = 16 * Tp + n, col = 16 * T1 + 4 * q;
    const float* p = wm_lane + 16 * Tp * w1r + 16 * T1;
    if constexpr (VEC) {
      return (row < w2r && col < w1r) ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const bool ok = row < w2r;
      return make_float4(ok && col < w1r ? p[0] : 0.f, ok && col + 1 < w1r ? p[1] : 0.f, ok && col + 2 < w1r ? p[2] : 0.f,
                         ok && col + 3 < w1r ? p[3] : 0.f);
    }
  };

  int64_t idx = stage_index[0];
  float frac = stage_frac[0];
  Row<DEGREE, MC> row = load_row<DEGREE, MC>(coeffs, sc, n_intervals, idx, Cr);

  for (int64_t k = 0; k < n_steps; ++k) {
    const TT t0 = grid[k], t1 = grid[k + 1];
    const float dt = (float)(t1 - t0);
    f32x4 k1a, k1b, k2a, k2b, pqa, pqb, za = ya, zb = yb;
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      float dX[MC];
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      control_slope<DEGREE, MC>(row, frac, width, dX);
      const int64_t e_next = 4 * k + stage + 1;
      const bool more = e_next < 4 * n_steps;
      const int64_t nidx = more ? stage_index[e_next] : idx;
      const float nfrac = more ? stage_frac[e_next] : frac;

      // ---- the field: layer 1 (LDS), middle layer (L2), layer 2 + activation + contraction (LDS)
      f32x4 fa = {0.f, 0.f, 0.f, 0.f}, fb = fa;
      {
        int opaque = 0;                         // keeps the LDS reads inside the evaluation (cde_mfma.h: field_act16)
        asm volatile("" : "+v"(opaque));
        const float4* w1 = reinterpret_cast<const float4*>(lds) + lane + opaque;
        const float4* bb1 = reinterpret_cast<const float4*>(lds + W1M_FLOATS) + q + opaque;
        const float4* w2 = reinterpret_cast<const float4*>(lds + W1M_FLOATS + B1M_FLOATS) + lane + opaque;
        const float4* bb2 = reinterpret_cast<const float4*>(lds + W1M_FLOATS + B1M_FLOATS + W2M_FLOATS) + q + opaque;
        const float4* bbm = reinterpret_cast<const float4*>(lds + MLP16_LDS_FLOATS) + q + opaque;
        const float zs[8] = {za[0], za[1], za[2], za[3], zb[0], zb[1], zb[2], zb[3]};
        float u1[32], u2[32];
        unsigned unused;
        mlp3_layer1<ACT>(w1, bb1, zs, u1, unused);
        mlp3_middle<ACT, false>(bbm, u1, u2, unused, load_wm);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int P = 0; P < 8; ++P) {            // unit group P: 4 hidden units x 8 channels = tiles 2P, 2P + 1
          const float4 c0 = bb2[8 * P], c1 = bb2[8 * P + 4];
          f32x4 y0 = {c0.x, c0.y, c0.z, c0.w}, y1 = {c1.x, c1.y, c1.z, c1.w};
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            const float4 a0 = w2[(16 * P + g) * 64], a1 = w2[(16 * P + 8 + g) * 64];
            y0 = mfma16(a0.x, u2[4 * g], y0);     y1 = mfma16(a1.x, u2[4 * g], y1);
            y0 = mfma16(a0.y, u2[4 * g + 1], y0); y1 = mfma16(a1.y, u2[4 * g + 1], y1);
            y0 = mfma16(a0.z, u2[4 * g + 2], y0); y1 = mfma16(a1.z, u2[4 * g + 2], y1);
            y0 = mfma16(a0.w, u2[4 * g + 3], y0); y1 = mfma16(a1.w, u2[4 * g + 3], y1);
          }
          const f32x2 t01 = activate2<ACT>(y0[0], y0[1]), t23 = activate2<ACT>(y0[2], y0[3]);
          const f32x2 t45 = activate2<ACT>(y1[0], y1[1]), t67 = activate2<ACT>(y1[2], y1[3]);
          float f = t01[0] * dX[0];
          f = __builtin_fmaf(t01[1], dX[1], f); f = __builtin_fmaf(t23[0], dX[2], f); f = __builtin_fmaf(t23[1], dX[3], f);
          f = __builtin_fmaf(t45[0], dX[4], f); f = __builtin_fmaf(t45[1], dX[5], f);
          f = __builtin_fmaf(t67[0], dX[6], f); f = __builtin_fmaf(t67[1], dX[7], f);
          if (P < 4) fa[P] = f; else fb[P - 4] = f;
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (nidx != idx) row = load_row<DEGREE, MC>(coeffs, sc, n_intervals, nidx, Cr);

      // torchdiffeq rk4_alt_step_func (3/8 rule), association order preserved
      const float third = (float)(1.0 / 3.0);
      if (stage == 0) {
        k1a = fa; k1b = fb;
        za = ya + dt * k1a * third; zb = yb + dt * k1b * third;
      } else if (stage == 1) {
        k2a = fa; k2b = fb;
        za = ya + dt * (k2a - k1a * third); zb = yb + dt * (k2b - k1b * third);
      } else if (stage == 2) {
        za = ya + dt * (k1a - k2a + fa); zb = yb + dt * (k1b - k2b + fb);
        pqa = k1a + 3.f * (k2a + fa); pqb = k1b + 3.f * (k2b + fb);
      } else {
        za = ya + (pqa + fa) * dt * 0.125f; zb = yb + (pqb + fb) * dt * 0.125f;
      }
      idx = nidx; frac = nfrac;
    }
    const f32x4 y1a = za, y1b = zb;
    while (jout < n_out && t1 >= t_out[jout]) {
      const TT tj = t_out[jout];
      if (tj == t0) store(jout, ya, yb);
      else if (tj == t1) store(jout, y1a, y1b);
      else {
        const float slope = (float)((tj - t0) / (t1 - t0));
        store(jout, ya + slope * (y1a - ya), yb + slope * (y1b - yb));
      }
      ++jout;
    }
    ya = y1a; yb = y1b;
  }
}

// ============================================================================================ adjoint sweep
__global__ void mlp3_adj_image_kernel(const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ Wm,
                                      const float* __restrict__ bm, const float* __restrict__ W2, const float* __restrict__ b2,
                                      float* __restrict__ img, Mlp3Dims d) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= MLP3_ADJ_IMAGE_FLOATS) return;
  const int at = e;
  const MlpDims d1{d.H, d.C, d.w1}, d2{d.H, d.C, d.w2};
  if (e < ADJ_LDS_FLOATS) {                     // K3m's LDS images: layer 1 (and its bias) for width1, the plain W2 copy for width2
    img[at] = mlp_adj_image(W1, b1, W2, b2, e, e < W1M_FLOATS + B1M_FLOATS ? d1 : d2, 2);
    return;
  }
  e -= ADJ_LDS_FLOATS;
  if (e < BMM_FLOATS) { img[at] = bm_image(bm, e, d.w2); return; }
  e -= BMM_FLOATS;
  if (e < W1T_FLOATS) { img[at] = mlp_adj_image(W1, b1, W2, b2, ADJ_LDS_FLOATS + e, d1, 2); return; }     // K3m's W1^T image
  e -= W1T_FLOATS;
  img[at] = e < WMM_FLOATS ? wm_image(Wm, e, d.w1, d.w2, false) : wm_image(Wm, e - WMM_FLOATS, d.w1, d.w2, true);
}

// K3m's one-wave-per-tile sweep (rk4_mlp_adjoint.hip: same lane layout, same LDS reads, same RK bookkeeping) with the middle
// layer: per stage  u1, mask1 (layer 1) -> u2, mask2 (middle) -> layer 2 / dL/dY2 / gu = dL/du2 per unit group ->
// gm = gu hid'(pre2) -> gu1 = Wm^T gm -> g1 = gu1 hid'(pre1) -> va = W1^T g1.
// One wave per SIMD (at most 256 threads): with u2, the second mask and the dL/dpre2 temporaries beside K3m's live set, and the
// middle layer's operands requested a tile pair ahead (cde_mlp3.h), the stage body needs 450 .. 512 registers -- under K3m's
// 512-thread, two-waves-per-SIMD bounds it spilled 216 .. 344 bytes per lane; under these 256 VGPRs + 193 .. 256 AGPRs and
// no scratch but for the relu field without tanh on a cubic control (44 bytes per lane; profiles/NOTES.md).
template <typename TT, int DEGREE, int ACT>
__global__ __launch_bounds__(256, 1) void rk4_adjoint_mlp3_sweep(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ img, float* __restrict__ y_state, float* __restrict__ a_state,
    const TT* __restrict__ sgrid, int64_t k_begin, int64_t k_end, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, float* __restrict__ U, float* __restrict__ U1, float* __restrict__ G2,
    float* __restrict__ Gm, float* __restrict__ G1, float* __restrict__ Z, int64_t B, Dims dims) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  {
    const float4* src = reinterpret_cast<const float4*>(img);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int i = threadIdx.x; i < MLP3_ADJ_LDS_FLOATS / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  constexpr int CT = MC, NB = 2, NP = 8;
  const int Hr = dims.H, Cr = dims.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;     // (1 .. 4 waves per workgroup: cde_launch.h, waves_per_workgroup)
  if (tile * 16 >= B) return;
  const int64_t series = tile * 16 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  const float4* w1t_base = reinterpret_cast<const float4*>(img + MLP3_ADJ_LDS_FLOATS) + lane;
  const float4* wmf_base = reinterpret_cast<const float4*>(img + MLP3_ADJ_LDS_FLOATS + W1T_FLOATS) + lane;
  const float4* wmt_base = wmf_base + WMM_FLOATS / 4;
  // lane offsets into the plain W2 copy (rk4_mlp_adjoint.hip): Y2 rows (h&3 = n>>2, c&3 = n&3), gu rows (h&3 = q, c&3 = cl)
  const int w2y_off = ((n >> 3) * 8 + w2p_residue(n >> 2, n & 3)) * W2P_STRIDE + 4 * q;
  int w2g_off[4];
#pragma unroll
  for (int cl = 0; cl < 4; ++cl) w2g_off[cl] = ((q >> 1) * 8 + w2p_residue(q, cl)) * W2P_STRIDE + n;

  const int ua = q, ub = 16 + q;                                     // this lane's units: q, 4+q, .., 28+q
  f32x4 ya = load_units4<4>(y_state + sc * Hr, ua, Hr), yb = load_units4<4>(y_state + sc * Hr, ub, Hr);
  f32x4 aa = load_units4<4>(a_state + sc * Hr, ua, Hr), ab = load_units4<4>(a_state + sc * Hr, ub, Hr);
  if (!valid) { aa = f32x4{0.f, 0.f, 0.f, 0.f}; ab = aa; }          // a == 0 stays 0: padded lanes contribute nothing

  int64_t idx = stage_index[4 * k_begin];
  float frac = stage_frac[4 * k_begin];
  Row<DEGREE, CT> row = load_row<DEGREE, CT>(coeffs, sc, n_intervals, idx, Cr);

  for (int64_t k = k_begin; k < k_end; ++k) {
    const float ds = (float)(sgrid[k + 1] - sgrid[k]);
    f32x4 ky1a, ky1b, ky2a, ky2b, ka1a, ka1b, ka2a, ka2b;
    f32x4 za = ya, zb = yb, sa = aa, sb = ab;                        // stage values of z and a
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      float dX[CT];
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      control_slope<DEGREE, CT>(row, frac, width, dX);
      const int64_t e_next = 4 * k + stage + 1;
      const bool more = e_next < 4 * k_end;
      const int64_t nidx = more ? stage_index[e_next] : idx;
      const float nfrac = more ? stage_frac[e_next] : frac;
      // (`row` is dead from here to the end of the stage: the next stage's row is reloaded before the va phase)
      const float wq = ((stage == 0 || stage == 3) ? 0.125f : 0.375f) * ds;      // 3/8-rule quadrature weight
      const int64_t out_row = ((k - k_begin) * 4 + stage) * B + series;          // (stage, series)

      int opaque = 0;                                                // keeps the LDS / image reads inside the stage
      asm volatile("" : "+v"(opaque));
      const float4* w1 = reinterpret_cast<const float4*>(lds) + lane + opaque;
      const float4* bb1 = reinterpret_cast<const float4*>(lds + W1M_FLOATS) + q + opaque;
      const float* w2p = lds + W1M_FLOATS + B1M_FLOATS + opaque;
      const float4* bb2 = reinterpret_cast<const float4*>(lds + W1M_FLOATS + B1M_FLOATS + W2P_FLOATS) + q + opaque;
      const float4* bbm = reinterpret_cast<const float4*>(lds + ADJ_LDS_FLOATS) + q + opaque;
      const float* w2y = w2p + w2y_off;
      const float* w2g[4] = {w2p + w2g_off[0], w2p + w2g_off[1], w2p + w2g_off[2], w2p + w2g_off[3]};
      const float4* w1t = w1t_base + opaque;
      const float4* wmf = wmf_base + opaque;
      const float4* wmt = wmt_base + opaque;
      const float zs[8] = {za[0], za[1], za[2], za[3], zb[0], zb[1], zb[2], zb[3]};
      const float as[8] = {sa[0], sa[1], sa[2], sa[3], sb[0], sb[1], sb[2], sb[3]};

      // ---- layer 1 and the middle layer: u1, u2 and their masks (softplus: the slopes are re-derived from the values)
      float u1[32], u2[32];
      unsigned mask1, mask2;
      mlp3_layer1<ACT>(w1, bb1, zs, u1, mask1);
      if (valid) {
        float* urow = U1 + out_row * U_COLS + 4 * q;                 // first hidden layer's units 16*T1 + 4q + r
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1) stream_store4(urow + 16 * T1, u1[4 * T1], u1[4 * T1 + 1], u1[4 * T1 + 2], u1[4 * T1 + 3]);
        float* zrow = Z + out_row * Z_COLS;
#pragma unroll
        for (int m = 0; m < 8; ++m) if (4 * m + q < Hr) zrow[4 * m + q] = zs[m];
      }
      mlp3_middle<ACT, true>(bbm, u1, u2, mask2, [&](int Tp, int T1) { return wmf[(8 * Tp + T1) * 64]; });
      if (valid) {
        float* urow = U + out_row * U_COLS + 4 * q;                  // second hidden layer's units
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1) stream_store4(urow + 16 * T1, u2[4 * T1], u2[4 * T1 + 1], u2[4 * T1 + 2], u2[4 * T1 + 3]);
      }

      __builtin_amdgcn_sched_barrier(0);
      // ---- layer 2, activation, contraction, dL/dY2, and gu += W2^T dL/dY2, one tile pair at a time (K3m's body on u2)
      f32x4 gu[8];
#pragma unroll
      for (int T1 = 0; T1 < 8; ++T1) gu[T1] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 fa = {0.f, 0.f, 0.f, 0.f}, fb = fa;
#pragma unroll
      for (int P = 0; P < NP; ++P) {                                 // unit group P: 4 hidden units x 8 channels = 2 tiles
        const float as_P = as[P];
        f32x4 y[NB];
        const float* tp_[NB];
#pragma unroll
        for (int tb = 0; tb < NB; ++tb) {
          const float4 c0 = bb2[4 * (NB * P + tb)];
          y[tb] = f32x4{c0.x, c0.y, c0.z, c0.w};
          tp_[tb] = w2y + 2 * (NB * P + tb) * 8 * W2P_STRIDE;        // tile T = 2P + tb: physical rows (2T + hb)*8 + r8
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          float4 a[NB];
#pragma unroll
          for (int tb = 0; tb < NB; ++tb) a[tb] = *reinterpret_cast<const float4*>(tp_[tb] + 16 * g);
#pragma unroll
          for (int tb = 0; tb < NB; ++tb) y[tb] = mfma16(a[tb].x, u2[4 * g], y[tb]);
#pragma unroll
          for (int tb = 0; tb < NB; ++tb) y[tb] = mfma16(a[tb].y, u2[4 * g + 1], y[tb]);
#pragma unroll
          for (int tb = 0; tb < NB; ++tb) y[tb] = mfma16(a[tb].z, u2[4 * g + 2], y[tb]);
#pragma unroll
          for (int tb = 0; tb < NB; ++tb) y[tb] = mfma16(a[tb].w, u2[4 * g + 3], y[tb]);
        }
        float g2[CT];
        float f = 0.f;
#pragma unroll
        for (int tb = 0; tb < NB; ++tb) {
          const f32x2 t01 = activate2<ACT>(y[tb][0], y[tb][1]), t23 = activate2<ACT>(y[tb][2], y[tb][3]);
          const float tv[4] = {t01[0], t01[1], t23[0], t23[1]};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 4 * tb + r;
            const float t = tv[r];
            f = c == 0 ? t * dX[0] : __builtin_fmaf(t, dX[c], f);
            const float slope = final_tanh(ACT) ? __builtin_fmaf(-t, t, 1.f) : 1.f;
            g2[c] = as_P * (dX[c] * slope);
          }
        }
        if (P < 4) fa[P] = f; else fb[P - 4] = f;
        if (valid) {
          float* grow = G2 + out_row * G2_COLS + 4 * CT * P + CT * q;      // rows (h = 4P+q, c = 0..7) of the padded layout
          stream_store4(grow, g2[0] * wq, g2[1] * wq, g2[2] * wq, g2[3] * wq);
          stream_store4(grow + 4, g2[4] * wq, g2[5] * wq, g2[6] * wq, g2[7] * wq);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {                               // K step (P, c); 8 independent accumulator chains
          const float* rowp = w2g[c & 3] + 2 * (NB * P + (c >> 2)) * 8 * W2P_STRIDE;
#pragma unroll
          for (int T1 = 0; T1 < 8; ++T1) gu[T1] = mfma16(rowp[16 * T1], g2[c], gu[T1]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }

      // ---- dL/dpre2 = gu * hid'(pre2);  gu1 = Wm^T dL/dpre2 (K step (T', r): the lane feeds its own register)
      float gm[32];
#pragma unroll
      for (int s2 = 0; s2 < 32; ++s2) gm[s2] = hidden_backward<ACT>(gu[s2 >> 2][s2 & 3], (mask2 >> s2) & 1u, u2[s2]);
      if (valid) {
        float* grow = Gm + out_row * GM_COLS + 4 * q;
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1)
          stream_store4(grow + 16 * T1, gm[4 * T1] * wq, gm[4 * T1 + 1] * wq, gm[4 * T1 + 2] * wq, gm[4 * T1 + 3] * wq);
      }
      f32x4 gu1[8];
      mlp3_middle_transposed(gm, gu1, [&](int T1, int Tp) { return wmt[(8 * T1 + Tp) * 64]; });
      __builtin_amdgcn_sched_barrier(0);
      row = load_row<DEGREE, CT>(coeffs, sc, n_intervals, nidx, Cr);     // for the next stage; lands during the va phase
      // ---- dL/dpre1 = gu1 * hid'(pre1);  va = W1^T dL/dpre1
      float g1[32];
#pragma unroll
      for (int s2 = 0; s2 < 32; ++s2) g1[s2] = hidden_backward<ACT>(gu1[s2 >> 2][s2 & 3], (mask1 >> s2) & 1u, u1[s2]);
      if (valid) {
        float* grow = G1 + out_row * G1_COLS + 4 * q;
#pragma unroll
        for (int T1 = 0; T1 < 8; ++T1)
          stream_store4(grow + 16 * T1, g1[4 * T1] * wq, g1[4 * T1 + 1] * wq, g1[4 * T1 + 2] * wq, g1[4 * T1 + 3] * wq);
      }
      f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = va;
#pragma unroll
      for (int T1 = 0; T1 < 8; ++T1) {
        const float4 a0 = w1t[T1 * 64], a1 = w1t[(8 + T1) * 64];
        va = mfma16(a0.x, g1[4 * T1], va);     vb = mfma16(a1.x, g1[4 * T1], vb);
        va = mfma16(a0.y, g1[4 * T1 + 1], va); vb = mfma16(a1.y, g1[4 * T1 + 1], vb);
        va = mfma16(a0.z, g1[4 * T1 + 2], va); vb = mfma16(a1.z, g1[4 * T1 + 2], vb);
        va = mfma16(a0.w, g1[4 * T1 + 3], va); vb = mfma16(a1.w, g1[4 * T1 + 3], vb);
      }

      __builtin_amdgcn_sched_barrier(0);
      // ---- reverse-time dynamics: dz/ds = -f, da/ds = +a^T df/dz; torchdiffeq 3/8 rule, association preserved
      const f32x4 kya = -fa, kyb = -fb, kaa = va, kab = vb;
      const float third = (float)(1.0 / 3.0);
      if (stage == 0) {
        ky1a = kya; ky1b = kyb; ka1a = kaa; ka1b = kab;
        za = ya + ds * ky1a * third; zb = yb + ds * ky1b * third;
        sa = aa + ds * ka1a * third; sb = ab + ds * ka1b * third;
      } else if (stage == 1) {
        ky2a = kya; ky2b = kyb; ka2a = kaa; ka2b = kab;
        za = ya + ds * (ky2a - ky1a * third); zb = yb + ds * (ky2b - ky1b * third);
        sa = aa + ds * (ka2a - ka1a * third); sb = ab + ds * (ka2b - ka1b * third);
      } else if (stage == 2) {
        za = ya + ds * (ky1a - ky2a + kya); zb = yb + ds * (ky1b - ky2b + kyb);
        sa = aa + ds * (ka1a - ka2a + kaa); sb = ab + ds * (ka1b - ka2b + kab);
        ky1a = ky1a + 3.f * (ky2a + kya); ky1b = ky1b + 3.f * (ky2b + kyb);
        ka1a = ka1a + 3.f * (ka2a + kaa); ka1b = ka1b + 3.f * (ka2b + kab);
      } else {
        za = ya + (ky1a + kya) * ds * 0.125f; zb = yb + (ky1b + kyb) * ds * 0.125f;
        sa = aa + (ka1a + kaa) * ds * 0.125f; sb = ab + (ka1b + kab) * ds * 0.125f;
      }
      idx = nidx; frac = nfrac;
      __builtin_amdgcn_sched_barrier(0);
    }
    ya = za; yb = zb; aa = sa; ab = sb;
  }
  if (valid) {
    store_units4<4>(y_state + series * Hr, ua, Hr, ya);
    store_units4<4>(y_state + series * Hr, ub, Hr, yb);
    store_units4<4>(a_state + series * Hr, ua, Hr, aa);
    store_units4<4>(a_state + series * Hr, ub, Hr, ab);
  }
}

// ------------------------------------------------------------------------------------------ host side
bool mlp3_shape_ok(int64_t C, int64_t H, int64_t width1, int64_t width2) {
  return H >= 1 && H <= MH && C >= 1 && C <= MC && width1 >= 1 && width1 <= MW && width2 >= 1 && width2 <= MW;
}

size_t mlp3_adjoint_image_bytes() { return (size_t)MLP3_ADJ_IMAGE_FLOATS * sizeof(float); }

int launch_mlp3_adjoint_images(const ThreeLayerField& f, int64_t C, int64_t H, float* img, hipStream_t s) {
  mlp3_adj_image_kernel<<<(MLP3_ADJ_IMAGE_FLOATS + 255) / 256, 256, 0, s>>>(
      f32(f.W1), f32(f.bias1), f32(f.Wm), f32(f.biasm), f32(f.W2), f32(f.bias2), img,
      Mlp3Dims{(int)H, (int)C, (int)f.width1, (int)f.width2});
  return check_launch();
}

template <typename TT>
int launch_forward_mlp3(const Control& x, const ThreeLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                        hipStream_t s) {
  if (!mlp3_shape_ok(n.C, n.H, f.width1, f.width2)) return CDE_ERR_UNSUPPORTED;
  const Mlp3Dims dims{(int)n.H, (int)n.C, (int)f.width1, (int)f.width2};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 8), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = (size_t)MLP3_FWD_LDS_FLOATS * sizeof(float);
  const bool vec = (f.width1 & 3) == 0 && ((uintptr_t)f.Wm & 15) == 0;
  const int rc = dispatch_degree_field(x.degree, f.act, [&](auto D, auto A) {
    auto launch = [&](auto V) {
      auto kernel = rk4_forward_mlp3<TT, D(), A(), V()>;
      allow_lds(kernel, lds);
      kernel<<<blocks, 64 * waves, lds, s>>>(f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W1), f32(f.bias1), f32(f.Wm),
                                      f32(f.biasm), f32(f.W2), f32(f.bias2), f32(io.z0), (const TT*)io.grid, io.n_grid,
                                      (const TT*)io.t_out, io.n_out, f32(io.z_out), n.B, st.index, f32(st.frac), dims);
    };
    if (vec) launch(std::true_type{}); else launch(std::false_type{});
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

template <typename TT>
int launch_mlp3_adjoint_sweep(const Control& x, const Sweep3IO& io, const Shape& n, const StageTable& st, hipStream_t s) {
  if (io.k_end <= io.k_begin) return CDE_OK;
  const Dims dims{(int)n.H, (int)n.C};
  const int64_t tiles = (n.B + 15) / 16;
  const unsigned waves = waves_per_workgroup(tiles, 4), blocks = (unsigned)((tiles + waves - 1) / waves);
  const size_t lds = (size_t)MLP3_ADJ_LDS_FLOATS * sizeof(float);
  const int rc = dispatch_degree_field(x.degree, io.act, [&](auto D, auto A) {
    auto kernel = rk4_adjoint_mlp3_sweep<TT, D(), A()>;
    allow_lds(kernel, lds);
    kernel<<<blocks, 64 * waves, lds, s>>>(f32(x.coeffs), f32(x.knots), x.n_intervals, io.image, f32(io.y_state), f32(io.a_state),
                                    (const TT*)io.grid, io.k_begin, io.k_end, st.index, f32(st.frac), f32(io.U), f32(io.U1),
                                    f32(io.G2), f32(io.Gm), f32(io.G1), f32(io.Z), n.B, dims);
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

#define CDE_INST(TT)                                                                                                       \
  template int launch_forward_mlp3<TT>(const Control&, const ThreeLayerField&, const ForwardIO&, const Shape&,             \
                                       const StageTable&, hipStream_t);                                                    \
  template int launch_mlp3_adjoint_sweep<TT>(const Control&, const Sweep3IO&, const Shape&, const StageTable&, hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
