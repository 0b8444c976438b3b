// rk4_bf16x3_adjoint.hip -- K3b: the one-wave adjoint of the headline solve on the bf16 matrix pipe (csrc/cde_bf16x3.h),
// `k3_form = product` under variant "bf16x3".  A translation unit of its own: K2b's file takes a compiler flag that would
// more than double this kernel's scratch.
#include "cde_bf16x3.h"
#include "cde_launch.h"

namespace cde {

// ============================================================================================ adjoint (K3b)
// K3 (rk4_mfma.hip: rk4_adjoint_mfma) with its two weight GEMMs on the bf16 pipe; the dL/dW product, the scratch
// transposes, the RK bookkeeping and the per-wave partial layout are K3's.
constexpr int64_t BX_PARTIAL_FLOATS = MH * MC * MH + MH * MC;

template <typename TT, int DEGREE>
__global__ __launch_bounds__(256, 1) void rk4_adjoint_bf16x3(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ z_saved,
    const float* __restrict__ grad_out, const TT* __restrict__ sgrid, const int64_t* __restrict__ seg_off,
    int64_t n_out, float* __restrict__ grad_z0, float* __restrict__ partial, int64_t B,
    const int64_t* __restrict__ stage_index, const float* __restrict__ stage_frac, Dims dims) {
  const int Hr = dims.H, Cr = dims.C;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  u32x4* imgY = reinterpret_cast<u32x4*>(lds_raw);
  u32x4* imgV = imgY + BX_IMG_U4;
  float* btab = reinterpret_cast<float*>(lds_raw + 2 * BX_IMG_U4 * 16);
  float* scr_base = btab + BX_BIAS_FLOATS;
  bx_stage_image(W, imgY, 0, dims, threadIdx.x, 256);
  bx_stage_image(W, imgV, 1, dims, threadIdx.x, 256);
  bx_stage_bias(bias, btab, dims, threadIdx.x, 256);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, half = lane >> 5;
  float* scr_y = scr_base + wave * SCR_FLOATS;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  float* my_partial = partial + tile * BX_PARTIAL_FLOATS;
  if (tile * 32 >= B) return;
  const int64_t series = tile * 32 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;

  f32x16 accW[MC];
  f32x2 gbp[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
#pragma unroll
  for (int c = 0; c < MC; ++c) {
#pragma unroll
    for (int r = 0; r < 16; ++r) accW[c][r] = 0.f;
  }
  f32x16 y0, a0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int u = 2 * r + half;
    const bool on = u < Hr;
    y0[r] = on ? z_saved[(sc * n_out + (n_out - 1)) * Hr + u] : 0.f;
    a0[r] = (valid && on) ? grad_out[(sc * n_out + (n_out - 1)) * Hr + u] : 0.f;
  }
  float* scr_zt = scr_y;                    // 64 rows x 20   (see rk4_adjoint_mfma)
  float* scr_at = scr_y + 64 * 20;
  float* scr_dw = scr_y + 2 * 64 * 20;      // 32 x 8

  for (int64_t p = 0; p + 1 < n_out; ++p) {
    const int64_t i_out = n_out - 1 - p;
    const int64_t k_begin = seg_off[p], k_end = seg_off[p + 1] - 1;
    if (k_end > k_begin) {
      int64_t idx = stage_index[4 * k_begin];
      float frac = stage_frac[4 * k_begin];
      Row<DEGREE> row = load_row<DEGREE>(coeffs, sc, n_intervals, idx, Cr);
      for (int64_t k = k_begin; k < k_end; ++k) {
        const float ds = (float)(sgrid[k + 1] - sgrid[k]);
        f32x16 ky1, ky2, ka1, ka2, yst = y0, ast = a0;
        // (NOT unrolled: with four stage bodies in one block the register allocator spilled 700 dwords; one body: 74)
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
          float dX[MC];
          const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
          control_slope<DEGREE>(row, frac, width, dX);
          const int64_t e_next = 4 * k + stage + 1;
          const bool more = e_next < 4 * k_end;
          const int64_t nidx = more ? stage_index[e_next] : idx;
          const float nfrac = more ? stage_frac[e_next] : frac;
          if (nidx != idx) row = load_row<DEGREE>(coeffs, sc, n_intervals, nidx, Cr);

          const f32x2 d01 = {dX[0], dX[1]}, d23 = {dX[2], dX[3]}, d45 = {dX[4], dX[5]}, d67 = {dX[6], dX[7]};
          // ---- stage state -> scratch (transposed), weighted control derivative (for the dL/dW product)
          {
            const float wq = ((stage == 0 || stage == 3) ? 0.125f : 0.375f) * ds;
            float* wz = scr_zt + ((n & 1) * 32 + half) * 20 + (n >> 1);
            float* wa = scr_at + ((n & 1) * 32 + half) * 20 + (n >> 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) { wz[r * 40] = yst[r]; wa[r * 40] = ast[r]; }
            const f32x2 w0 = (half ? d45 : d01) * wq, w1 = (half ? d67 : d23) * wq;
            *reinterpret_cast<float4*>(scr_dw + n * 8 + 4 * half) = make_float4(w0[0], w0[1], w1[0], w1[1]);
            bx_wave_lds_sync();
          }
          // ---- f and a^T df/dz on the bf16 pipe
          const f32x16 f = bx_field(imgY, btab, lane, half, yst, dX);
          const f32x16 va = bx_vjp(imgV, lane, ast, dX);
          // ---- dL/dW tile c: D[h][k] += sum_series (w ds a_h dX_c)[series] * z_k[series] on the exact-f32 pipe (K3's block)
          {
            const float4* zt4 = reinterpret_cast<const float4*>(scr_zt + (half * 32 + n) * 20);
            const float4* at4 = reinterpret_cast<const float4*>(scr_at + (half * 32 + n) * 20);
            const float4* dw4 = reinterpret_cast<const float4*>(scr_dw + half * 8);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const float4 zq = zt4[g4], aq = at4[g4];
              const f32x2 ap0 = {aq.x, aq.y}, ap1 = {aq.z, aq.w};
              const float zs[4] = {zq.x, zq.y, zq.z, zq.w};
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int s2 = 4 * g4 + i;
                const float4 e0 = dw4[s2 * 4], e1 = dw4[s2 * 4 + 1];
                const f32x2 e01 = {e0.x, e0.y}, e23 = {e0.z, e0.w}, e45 = {e1.x, e1.y}, e67 = {e1.z, e1.w};
                const f32x2 asrc = i < 2 ? ap0 : ap1;
                f32x2 v01, v23, v45, v67;
                if (i & 1) {
                  v01 = pk_mul_hi(e01, asrc); v23 = pk_mul_hi(e23, asrc); v45 = pk_mul_hi(e45, asrc); v67 = pk_mul_hi(e67, asrc);
                  pk_fma_hi(gbp[0], e01, asrc); pk_fma_hi(gbp[1], e23, asrc); pk_fma_hi(gbp[2], e45, asrc); pk_fma_hi(gbp[3], e67, asrc);
                } else {
                  v01 = pk_mul_lo(e01, asrc); v23 = pk_mul_lo(e23, asrc); v45 = pk_mul_lo(e45, asrc); v67 = pk_mul_lo(e67, asrc);
                  pk_fma_lo(gbp[0], e01, asrc); pk_fma_lo(gbp[1], e23, asrc); pk_fma_lo(gbp[2], e45, asrc); pk_fma_lo(gbp[3], e67, asrc);
                }
                __builtin_amdgcn_sched_barrier(0);
                const float zb = zs[i];
                accW[0] = mfma(v01[0], zb, accW[0]); accW[1] = mfma(v01[1], zb, accW[1]);
                accW[2] = mfma(v23[0], zb, accW[2]); accW[3] = mfma(v23[1], zb, accW[3]);
                accW[4] = mfma(v45[0], zb, accW[4]); accW[5] = mfma(v45[1], zb, accW[5]);
                accW[6] = mfma(v67[0], zb, accW[6]); accW[7] = mfma(v67[1], zb, accW[7]);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
          }
          bx_wave_lds_sync();
          // ---- reverse-time dynamics: dy/ds = -f, da/ds = +a^T df/dz (3/8 rule, torchdiffeq's association)
          const f32x16 ky = -f, ka = va;
          const float third = (float)(1.0 / 3.0);
          if (stage == 0) {
            ky1 = ky; ka1 = ka;
            yst = y0 + ds * ky1 * third;
            ast = a0 + ds * ka1 * third;
          } else if (stage == 1) {
            ky2 = ky; ka2 = ka;
            yst = y0 + ds * (ky2 - ky1 * third);
            ast = a0 + ds * (ka2 - ka1 * third);
          } else if (stage == 2) {
            yst = y0 + ds * (ky1 - ky2 + ky);
            ast = a0 + ds * (ka1 - ka2 + ka);
            ky1 = ky1 + 3.f * (ky2 + ky);
            ka1 = ka1 + 3.f * (ka2 + ka);
          } else {
            yst = y0 + (ky1 + ky) * ds * 0.125f;
            ast = a0 + (ka1 + ka) * ds * 0.125f;
          }
          idx = nidx; frac = nfrac;
        }
        y0 = yst; a0 = ast;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 2 * r + half;
      if (u < Hr) {
        y0[r] = z_saved[(sc * n_out + (i_out - 1)) * Hr + u];
        if (valid) a0[r] += grad_out[(sc * n_out + (i_out - 1)) * Hr + u];
      }
    }
  }
  if (valid) {
#pragma unroll
    for (int r = 0; r < 16; ++r) if (2 * r + half < Hr) grad_z0[series * Hr + 2 * r + half] = a0[r];
  }
#pragma unroll
  for (int c = 0; c < MC; ++c) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int h = (r & 3) + 8 * (r >> 2) + 4 * half;
      my_partial[(h * MC + c) * MH + n] = accW[c][r];
    }
    const float mine_gb = gbp[c >> 1][c & 1];
    const float other = __shfl_xor(mine_gb, 32, 64);
    if (half == 0) my_partial[MH * MC * MH + n * MC + c] = mine_gb + other;
  }
}

// ------------------------------------------------------------------------------------------ host side
template <typename TT>
int launch_adjoint_bf16x3(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                          float* partial, hipStream_t s) {
  const Dims dims{(int)n.H, (int)n.C};
  const unsigned blocks = (unsigned)((n.B + 127) / 128);
  int rc = dispatch_degree(x.degree, [&](auto D) {
    allow_lds(rk4_adjoint_bf16x3<TT, D()>, BX_ADJ_LDS_BYTES);
    rk4_adjoint_bf16x3<TT, D()><<<blocks, 256, BX_ADJ_LDS_BYTES, s>>>(
        f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.z_saved), f32(io.grad_out),
        (const TT*)io.sgrid, io.seg_off, io.n_out, f32(io.grad_z0), partial, n.B, st.index, f32(st.frac), dims);
    return CDE_OK;
  });
  if (rc == CDE_OK) rc = check_launch();
  if (rc != CDE_OK) return rc;
  return launch_reduce_partials(partial, (n.B + 31) / 32, io.grad_W, io.grad_b, (int)n.H, (int)n.C, s);
}


#define CDE_INST(TT)                                                                                                  \
  template int launch_adjoint_bf16x3<TT>(const Control&, const AffineField&, const AdjointIO&, const Shape&, const StageTable&, float*, hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
