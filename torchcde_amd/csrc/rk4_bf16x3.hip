// rk4_bf16x3.hip -- K2b: the forward of the headline solve (f32 state, H <= 32, C <= 8, affine field) with its weight GEMM
// on the BF16 matrix pipe at float32 accuracy (csrc/cde_bf16x3.h).  Since round 13 `variant = CDE_VARIANT_BF16X3` and AUTO's
// bf16 form run K2bd (rk4_bf16x3_duo.hip: the same solve as two interleaved 16-series groups per wave); this kernel is what
// tuning option k2b_groups = 1 selects, kept for A/B timing and as the reference the new one is tested beside (api.hip).  The one-wave adjoint K3b is rk4_bf16x3_adjoint.hip: this file is
// built with -amdgpu-mfma-vgpr-form (torchcde_amd/_lib.py), which keeps K2b's accumulators out of AGPRs and would cost K3b scratch.
// The AGPRs hold the weights instead: the piece image is staged in LDS as in K3b, then every wave reads its lane's 48 entries
// once (bx_load_resident) and the time loop evaluates the field with bx_field_resident -- the MFMAs take SrcA from a[...] and
// the only LDS reads left in a stage are the 32 of the bias table.  K3b keeps the LDS form (bx_field): see cde_bf16x3.h.
#include "cde_bf16x3.h"
#include "cde_launch.h"

namespace cde {

// ============================================================================================ forward (K2b)
template <typename TT, int DEGREE>
__global__ __launch_bounds__(256, 1) void rk4_forward_bf16x3(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ z0,
    const TT* __restrict__ grid, int64_t n_grid, const TT* __restrict__ t_out, int64_t n_out,
    float* __restrict__ z_out, int64_t B, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, Dims dims) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  u32x4* imgY = reinterpret_cast<u32x4*>(lds_raw);
  float* btab = reinterpret_cast<float*>(lds_raw + BX_IMG_U4 * 16);
  bx_stage_image(W, imgY, 0, dims, threadIdx.x, 256);
  bx_stage_bias(bias, btab, dims, threadIdx.x, 256);
  __syncthreads();
  const int Hr = dims.H, Cr = dims.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 31, half = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  if (tile * 32 >= B) return;
  u32x4 wY[BX_IMG_PER_LANE];                                     // 192 AGPRs: the image is not read again
  bx_load_resident(imgY, lane, wY);
  const int64_t series = tile * 32 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  f32x16 y;
#pragma unroll
  for (int r = 0; r < 16; ++r) y[r] = 2 * r + half < Hr ? z0[sc * Hr + 2 * r + half] : 0.f;
  auto store = [&](int64_t j, const f32x16& v) {
    if (valid) {
      float* row = z_out + (series * n_out + j) * Hr;
#pragma unroll
      for (int r = 0; r < 16; ++r) if (2 * r + half < Hr) row[2 * r + half] = v[r];
    }
  };
  store(0, y);
  int64_t jout = 1;
  const int64_t n_steps = n_grid - 1;
  if (n_steps <= 0) return;
  int64_t idx = stage_index[0];
  float frac = stage_frac[0];
  Row<DEGREE> row = load_row<DEGREE>(coeffs, sc, n_intervals, idx, Cr);
  for (int64_t k = 0; k < n_steps; ++k) {
    const TT t0 = grid[k], t1 = grid[k + 1];
    const float dt = (float)(t1 - t0);
    f32x16 k1, k2, pq, z = y;
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      float dX[MC];
      const float width = DEGREE == CDE_PATH_LINEAR ? knots[idx + 1] - knots[idx] : 1.f;
      control_slope<DEGREE>(row, frac, width, dX);
      const int64_t e_next = 4 * k + stage + 1;
      const bool more = e_next < 4 * n_steps;
      const int64_t nidx = more ? stage_index[e_next] : idx;
      const float nfrac = more ? stage_frac[e_next] : frac;
      if (nidx != idx) row = load_row<DEGREE>(coeffs, sc, n_intervals, nidx, Cr);
      const f32x16 f = bx_field_resident(wY, btab, half, z, dX);
      // torchdiffeq rk4_alt_step_func (3/8 rule), association order preserved
      const float third = (float)(1.0 / 3.0);
      if (stage == 0) { k1 = f; z = y + dt * k1 * third; }
      else if (stage == 1) { k2 = f; z = y + dt * (k2 - k1 * third); }
      else if (stage == 2) { z = y + dt * (k1 - k2 + f); pq = k1 + 3.f * (k2 + f); }
      else z = y + (pq + f) * dt * 0.125f;
      idx = nidx; frac = nfrac;
    }
    const f32x16 y1 = z;
    while (jout < n_out && t1 >= t_out[jout]) {
      const TT tj = t_out[jout];
      if (tj == t0) store(jout, y);
      else if (tj == t1) store(jout, y1);
      else {
        const float slope = (float)((tj - t0) / (t1 - t0));
        store(jout, y + slope * (y1 - y));
      }
      ++jout;
    }
    y = y1;
  }
}

// ------------------------------------------------------------------------------------------ host side
template <typename TT>
int launch_forward_bf16x3(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                          hipStream_t s) {
  const Dims dims{(int)n.H, (int)n.C};
  const unsigned blocks = (unsigned)((n.B + 127) / 128);
  const int rc = dispatch_degree(x.degree, [&](auto D) {
    allow_lds(rk4_forward_bf16x3<TT, D()>, BX_FWD_LDS_BYTES);
    rk4_forward_bf16x3<TT, D()><<<blocks, 256, BX_FWD_LDS_BYTES, s>>>(
        f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.z0), (const TT*)io.grid, io.n_grid,
        (const TT*)io.t_out, io.n_out, f32(io.z_out), n.B, st.index, f32(st.frac), dims);
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

#define CDE_INST(TT)                                                                                                  \
  template int launch_forward_bf16x3<TT>(const Control&, const AffineField&, const ForwardIO&, const Shape&, const StageTable&, hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
