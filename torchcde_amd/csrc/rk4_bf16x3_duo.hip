// rk4_bf16x3_duo.hip -- K2bd: K2b (rk4_bf16x3.hip) with the wave's 32 series cut into two groups of 16, A and B, that run
// half a stage apart in ONE instruction stream (cde_bf16x3_duo.h: layout, v_mfma_f32_16x16x32_bf16 field, control exchange).
// K2b's stage is one dependency chain -- z -> split -> 96 MFMAs -> contraction -> 3/8-rule update -> next z -- and its ~390
// vector instructions issue with no MFMA in flight (~1,900 of ~4,960 cycles).  Here the time loop is written phase by phase,
//     [M_B(s) || V_A(s)]   [M_A(s + 1) || V_B(s)]   ...
// M_g(s): group g's 96 MFMAs of stage s; V_g(s): its contraction, update, split into the operands of M_g(s + 1), and the
// control slopes of stage s + 1.  The two halves of a phase are independent.  A phase is written as 96 slots -- one MFMA,
// two single-instruction steps of V -- with a scheduling barrier behind every slot and an empty asm on every step's result
// (bxd_phase, bxd_vstep); __builtin_amdgcn_sched_group_barrier over a phase written as M then V did not hold the order: the
// compiler emitted V whole, then 96 bare MFMAs (profiles/NOTES.md, round 13).  -DBXD_INTERLEAVE=0 builds the same source
// with V behind M.  M_A(0) runs alone before the loop and one M_A past the last step is computed and dropped.
// The control: a phase opens with the slopes of vg's stage s + 1 from the row in its registers and, where the interval index
// changes, requests the row of stage s + 2 into the same registers right there, in front of the phase's 96 MFMAs.  The
// wave's global loads share one in-order counter and the request sits behind branches, so the next read of any row
// register -- the next phase's first instruction, on the other group's row -- waits for every load in flight: requested
// behind V, as first built (-DBXD_ROW_AT_TAIL=1), the row was drained where it was issued
// (tests/test_kernel_forward_row_request.py holds the distance from request to wait).  Weights
// resident in AGPRs, built with -amdgpu-mfma-vgpr-form, one wave per SIMD, as K2b; dead series clamp to series B - 1 and
// store nothing, a tile beyond B returns before the loop.  `variant = "bf16x3"` and AUTO's bf16 form take this kernel;
// tuning option k2b_groups = 1 selects K2b (api.hip).  The values differ from K2b's in the last bits: K = 32 is summed
// inside one MFMA, not in two K = 16 steps.
#include "cde_bf16x3_duo.h"
#include "cde_launch.h"

#ifndef BXD_INTERLEAVE
#define BXD_INTERLEAVE 1
#endif
#ifndef BXD_ROW_AT_TAIL
#define BXD_ROW_AT_TAIL 0                    // 1: the row request behind V, as first built (A/B timing: profiles/NOTES.md, round 14)
#endif

namespace cde {

template <int DEGREE>
struct BxdGroup {
  float y[8], z[8], k1[8], k2[8];            // z: the state of the group's next field evaluation (y1 behind the last stage)
  bf16x8 zp[3];                              // its pieces
  f32x4 acc[16];
  float dX[MC];
  BxdRow<DEGREE> row;                        // the coefficient row of the stage whose slopes are formed next
  float* strip;                              // strip row of the lane's series
  int64_t series, sc;
  bool valid;
};

struct BxdStages {
  const int64_t* __restrict__ index;
  const float* __restrict__ frac;
  const float* __restrict__ knots;
  int64_t last;                              // 4 n_steps - 1
  __device__ __forceinline__ int64_t at(int64_t e) const { return e < last ? e : last; }
};

// the stage table's entries of one RK step (global stages e .. e + 5; both groups read them), loaded once per step: a
// scalar load at the head of every phase leaves its round trip in front of the phase's first MFMA
template <int DEGREE>
struct BxdStepT {
  int64_t idx[6];
  float frac[6], width[6];
  __device__ __forceinline__ void load(const BxdStages& st, int64_t e) {
#pragma unroll
    for (int j = 1; j < 6; ++j) {
      idx[j] = st.index[st.at(e + j)];
      frac[j] = st.frac[st.at(e + j)];
    }
#pragma unroll
    for (int j = 1; j < 5; ++j) width[j] = DEGREE == CDE_PATH_LINEAR ? st.knots[idx[j] + 1] - st.knots[idx[j]] : 1.f;
  }
};

// a loop whose index is a constant in the body
template <int I, int N, typename F>
__device__ __forceinline__ void bxd_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    bxd_static_for<I + 1, N>(f);
  }
}

// V_g(s) as a list of single vector instructions: step i of BXD_V_STEPS<STAGE>.  Contraction (64: bxd_contract's chains, two
// units at a time), 3/8-rule update (operation by operation across the units; association order of rk4_bf16x3.hip), split
// (44: bxd_split8's arithmetic level by level across the four pairs).  Adjacent steps are independent of each other.
__host__ __device__ constexpr int bxd_update_ops(int stage) { return stage == 0 ? 3 : stage == 2 ? 7 : 4; }
template <int STAGE>
constexpr int BXD_V_STEPS = 64 + 8 * bxd_update_ops(STAGE) + 44;

struct BxdTemps {
  float f[8], ta[8], tb[8], r0[4], r1[4];
  unsigned pw[3][4];
};

// (an empty asm on a step's result: no instruction, but the step can neither sink below its slot's scheduling barrier nor
// -- through the results it reads -- rise far above it.  Without these every step of V is emitted ahead of the first MFMA.)
#define BXD_PIN(x) asm volatile("" : "+v"(x))
template <int STAGE, int I, int DEGREE>
__device__ __forceinline__ void bxd_vstep(BxdGroup<DEGREE>& g, BxdTemps& t, float dt) {
  constexpr int NU = 8 * bxd_update_ops(STAGE);
  const float third = (float)(1.0 / 3.0);
  if constexpr (I < 64) {
    constexpr int j = I & 15, c = j >> 1, m = 2 * (I >> 4) + (j & 1);
    if constexpr (c == 0) { t.f[m] = g.acc[2 * m][0] * g.dX[0]; BXD_PIN(t.f[m]); }
    else { t.f[m] = __builtin_fmaf(g.acc[2 * m + (c >> 2)][c & 3], g.dX[c], t.f[m]); BXD_PIN(t.f[m]); }
  } else if constexpr (I < 64 + NU) {
    constexpr int op = (I - 64) / 8, m = (I - 64) % 8;
    if constexpr (STAGE == 0) {                                  // k1 = f; z = y + dt * k1 * third
      if constexpr (op == 0) { { g.k1[m] = t.f[m]; BXD_PIN(g.k1[m]); } { t.ta[m] = dt * g.k1[m]; BXD_PIN(t.ta[m]); } }
      else if constexpr (op == 1) { t.ta[m] = t.ta[m] * third; BXD_PIN(t.ta[m]); }
      else { g.z[m] = g.y[m] + t.ta[m]; BXD_PIN(g.z[m]); }
    } else if constexpr (STAGE == 1) {                           // k2 = f; z = y + dt * (k2 - k1 * third)
      if constexpr (op == 0) { g.k2[m] = t.f[m]; { t.ta[m] = g.k1[m] * third; BXD_PIN(t.ta[m]); } }
      else if constexpr (op == 1) { t.ta[m] = g.k2[m] - t.ta[m]; BXD_PIN(t.ta[m]); }
      else if constexpr (op == 2) { t.ta[m] = dt * t.ta[m]; BXD_PIN(t.ta[m]); }
      else { g.z[m] = g.y[m] + t.ta[m]; BXD_PIN(g.z[m]); }
    } else if constexpr (STAGE == 2) {                           // z = y + dt * (k1 - k2 + f); pq = k1 + 3 * (k2 + f), kept in k1
      if constexpr (op == 0) { t.ta[m] = g.k1[m] - g.k2[m]; BXD_PIN(t.ta[m]); }
      else if constexpr (op == 1) { t.ta[m] = t.ta[m] + t.f[m]; BXD_PIN(t.ta[m]); }
      else if constexpr (op == 2) { t.ta[m] = dt * t.ta[m]; BXD_PIN(t.ta[m]); }
      else if constexpr (op == 3) { g.z[m] = g.y[m] + t.ta[m]; BXD_PIN(g.z[m]); }
      else if constexpr (op == 4) { t.tb[m] = g.k2[m] + t.f[m]; BXD_PIN(t.tb[m]); }
      else if constexpr (op == 5) { t.tb[m] = 3.f * t.tb[m]; BXD_PIN(t.tb[m]); }
      else { g.k1[m] = g.k1[m] + t.tb[m]; BXD_PIN(g.k1[m]); }
    } else {                                                     // z = y + (pq + f) * dt * 0.125
      if constexpr (op == 0) { t.ta[m] = g.k1[m] + t.f[m]; BXD_PIN(t.ta[m]); }
      else if constexpr (op == 1) { t.ta[m] = t.ta[m] * dt; BXD_PIN(t.ta[m]); }
      else if constexpr (op == 2) { t.ta[m] = t.ta[m] * 0.125f; BXD_PIN(t.ta[m]); }
      else { g.z[m] = g.y[m] + t.ta[m]; BXD_PIN(g.z[m]); }
    }
  } else {
    constexpr int j = I - 64 - NU;
    if constexpr (j < 4) { t.pw[0][j] = bxd_cvt_pk(g.z[2 * j], g.z[2 * j + 1]); BXD_PIN(t.pw[0][j]); }
    else {
      constexpr int level = (j - 4) / 20, r = (j - 4) % 20;      // per level: 4 shifts, 4 ands, 8 subtractions, 4 conversions
      if constexpr (r < 4) { t.ta[r] = __uint_as_float(t.pw[level][r] << 16); BXD_PIN(t.ta[r]); }
      else if constexpr (r < 8) { t.tb[r - 4] = __uint_as_float(t.pw[level][r - 4] & 0xffff0000u); BXD_PIN(t.tb[r - 4]); }
      else if constexpr (r < 16) {
        constexpr int p = (r - 8) >> 1, odd = (r - 8) & 1;
        if constexpr (odd) { t.r1[p] = (level == 0 ? g.z[2 * p + 1] : t.r1[p]) - t.tb[p]; BXD_PIN(t.r1[p]); }
        else { t.r0[p] = (level == 0 ? g.z[2 * p] : t.r0[p]) - t.ta[p]; BXD_PIN(t.r0[p]); }
      } else { t.pw[level + 1][r - 16] = bxd_cvt_pk(t.r0[r - 16], t.r1[r - 16]); BXD_PIN(t.pw[level + 1][r - 16]); }
    }
  }
}

// One phase: M of `mg` (96 MFMAs) beside V of `vg`, which is at stage STAGE of its step (global stage number e).  Written
// slot by slot -- one MFMA, then two steps of V -- with a scheduling barrier behind every slot: the order is the source's.
// The bias tiles of a pair are requested 12 slots ahead of its first MFMA; those of mg's first pair were requested in the
// phase before, behind the contraction that last read those registers, and this phase does the same for vg.
template <int STAGE, int DEGREE>
__device__ __forceinline__ void bxd_phase(BxdGroup<DEGREE>& mg, BxdGroup<DEGREE>& vg, const u32x4 (&w)[BX_IMG_PER_LANE],
                                          const float4* b4, float dt, const BxdStepT<DEGREE>& sp, const float* __restrict__ coeffs,
                                          int64_t n_intervals, int Cr, int q) {
  bx_wave_lds_sync();                        // the slopes `mg` wrote in the last phase are read in this one
  const int64_t idx1 = sp.idx[STAGE + 1];
  bxd_write_slopes<DEGREE>(vg.row, sp.frac[STAGE + 1], sp.width[STAGE + 1], vg.strip, q);  // of vg's next stage
  // the row of the stage after that, into the registers just read, where the interval index changes.  Requested here, not
  // behind V: the wait for a row is the next phase's first instruction and, behind these branches, one for every load in
  // flight (vmcnt counts in order and the compiler cannot tell which loads were issued) -- this request included, so it
  // has to be a phase old by then
  const int64_t idx2 = sp.idx[STAGE + 2];
  if constexpr (!BXD_ROW_AT_TAIL)
    if (idx2 != idx1) vg.row = bxd_load_row<DEGREE>(coeffs, vg.sc, n_intervals, idx2, Cr, q);
  auto bias = [&](f32x4& acc, int t) { const float4 bb = b4[t * 4]; acc = f32x4{bb.x, bb.y, bb.z, bb.w}; };
  BxdTemps t;
  __builtin_amdgcn_sched_barrier(0);
  bxd_static_for<0, 96>([&](auto S) {
    constexpr int slot = S(), tp = slot / 12, p = (slot % 12) / 2, u = slot & 1, tile = 2 * tp + u;
    constexpr int pa = p == 0 ? 2 : (p == 1 || p == 3) ? 1 : 0;   // a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1 (bx_block2_pieces)
    constexpr int pb = p == 0 ? 0 : p == 1 ? 1 : p == 2 ? 2 : p == 3 ? 0 : p == 4 ? 1 : 0;
    if constexpr (slot % 12 == 0 && tp < 7) { bias(mg.acc[tile + 2], tile + 2); bias(mg.acc[tile + 3], tile + 3); }
    mg.acc[tile] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w[tile * 3 + pa]), mg.zp[pb], mg.acc[tile], 0, 0, 0);
    if constexpr (BXD_INTERLEAVE) {
      if constexpr (2 * slot < BXD_V_STEPS<STAGE>) bxd_vstep<STAGE, 2 * slot>(vg, t, dt);
      if constexpr (2 * slot + 1 < BXD_V_STEPS<STAGE>) bxd_vstep<STAGE, 2 * slot + 1>(vg, t, dt);
      if constexpr (slot == 12) { bias(vg.acc[0], 0); bias(vg.acc[1], 1); }       // its contraction is through with them
    }
    if constexpr (slot == 64) bxd_read_slopes(mg.strip, mg.dX);  // of mg's stage: the MFMAs behind it cover the round trip
    __builtin_amdgcn_sched_barrier(0);
  });
  if constexpr (!BXD_INTERLEAVE) {
    bxd_static_for<0, BXD_V_STEPS<STAGE>>([&](auto I) { bxd_vstep<STAGE, I()>(vg, t, dt); __builtin_amdgcn_sched_barrier(0); });
    bias(vg.acc[0], 0); bias(vg.acc[1], 1);
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) vg.zp[m] = __builtin_bit_cast(bf16x8, u32x4{t.pw[m][0], t.pw[m][1], t.pw[m][2], t.pw[m][3]});
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (BXD_ROW_AT_TAIL)
    if (idx2 != idx1) vg.row = bxd_load_row<DEGREE>(coeffs, vg.sc, n_intervals, idx2, Cr, q);
}

template <typename TT, int DEGREE>
__global__ __launch_bounds__(256, 1) void rk4_forward_bf16x3_duo(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ z0,
    const TT* __restrict__ grid, int64_t n_grid, const TT* __restrict__ t_out, int64_t n_out,
    float* __restrict__ z_out, int64_t B, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, Dims dims) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  u32x4* imgY = reinterpret_cast<u32x4*>(lds_raw);
  float* btab = reinterpret_cast<float*>(lds_raw + BX_IMG_U4 * 16);
  float* strips = btab + BXD_BIAS_FLOATS;
  bxd_stage_image(W, imgY, dims, threadIdx.x, 256);
  bxd_stage_bias(bias, btab, dims, threadIdx.x, 256);
  __syncthreads();
  const int Hr = dims.H, Cr = dims.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  if (tile * 32 >= B) return;
  u32x4 wY[BX_IMG_PER_LANE];                                     // 192 AGPRs: the image is not read again
  bx_load_resident(imgY, lane, wY);
  // the bias table is loop invariant: without this the compiler hoists its 16 LDS reads out of the time loop (bx_field_resident)
  int opaque = 0;
  asm volatile("" : "+v"(opaque));
  const float4* b4 = reinterpret_cast<const float4*>(btab) + q + opaque;

  const int64_t n_steps = n_grid - 1;
  const BxdStages st{stage_index, stage_frac, knots, n_steps > 0 ? 4 * n_steps - 1 : 0};
  BxdGroup<DEGREE> g[2];
  auto store = [&](const BxdGroup<DEGREE>& s, int64_t j, const float (&v)[8]) {
    if (s.valid) {
      float* row = z_out + (s.series * n_out + j) * Hr;
      store_units4<1>(row, 8 * q, Hr, f32x4{v[0], v[1], v[2], v[3]});
      store_units4<1>(row, 8 * q + 4, Hr, f32x4{v[4], v[5], v[6], v[7]});
    }
  };
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {
    BxdGroup<DEGREE>& s = g[gi];
    s.series = tile * 32 + 16 * gi + n;
    s.valid = s.series < B;
    s.sc = s.valid ? s.series : B - 1;
    s.strip = strips + ((wave * 2 + gi) * 16 + n) * 8;
    const f32x4 lo = load_units4<1>(z0 + s.sc * Hr, 8 * q, Hr), hi = load_units4<1>(z0 + s.sc * Hr, 8 * q + 4, Hr);
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.y[j] = lo[j]; s.y[4 + j] = hi[j]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) { s.z[j] = s.y[j]; s.k1[j] = 0.f; s.k2[j] = 0.f; }
    store(s, 0, s.y);
  }
  if (n_steps <= 0) return;
#pragma unroll
  for (int gi = 0; gi < 2; ++gi) {
    BxdGroup<DEGREE>& s = g[gi];
    bxd_split8(s.z, s.zp);
    const int64_t idx0 = stage_index[0];
    const float width0 = DEGREE == CDE_PATH_LINEAR ? knots[idx0 + 1] - knots[idx0] : 1.f;
    s.row = bxd_load_row<DEGREE>(coeffs, s.sc, n_intervals, idx0, Cr, q);
    bxd_write_slopes<DEGREE>(s.row, stage_frac[0], width0, s.strip, q);
    s.row = bxd_load_row<DEGREE>(coeffs, s.sc, n_intervals, stage_index[st.at(1)], Cr, q);
  }
  bx_wave_lds_sync();
  bxd_field_mfma(wY, b4, g[0].zp, g[0].acc);                     // M_A(0)
  bxd_read_slopes(g[0].strip, g[0].dX);
#pragma unroll
  for (int u = 0; u < 2; ++u) {                                  // M_B(0)'s first bias tiles (bxd_phase requests them a phase ahead)
    const float4 bb = b4[u * 4];
    g[1].acc[u] = f32x4{bb.x, bb.y, bb.z, bb.w};
  }
  __builtin_amdgcn_sched_barrier(0);

  int64_t jout = 1;
  for (int64_t k = 0; k < n_steps; ++k) {
    const TT t0 = grid[k], t1 = grid[k + 1];
    const float dt = (float)(t1 - t0);
    BxdStepT<DEGREE> sp;
    sp.load(st, 4 * k);
    bxd_phase<0, DEGREE>(g[1], g[0], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<0, DEGREE>(g[0], g[1], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<1, DEGREE>(g[1], g[0], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<1, DEGREE>(g[0], g[1], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<2, DEGREE>(g[1], g[0], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<2, DEGREE>(g[0], g[1], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<3, DEGREE>(g[1], g[0], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);
    bxd_phase<3, DEGREE>(g[0], g[1], wY, b4, dt, sp, coeffs, n_intervals, Cr, q);   // M_A of the next step's first stage
    while (jout < n_out && t1 >= t_out[jout]) {
      const TT tj = t_out[jout];
#pragma unroll
      for (int gi = 0; gi < 2; ++gi) {
        const BxdGroup<DEGREE>& s = g[gi];
        if (tj == t0) store(s, jout, s.y);
        else if (tj == t1) store(s, jout, s.z);
        else {
          const float slope = (float)((tj - t0) / (t1 - t0));
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = s.y[j] + slope * (s.z[j] - s.y[j]);
          store(s, jout, v);
        }
      }
      ++jout;
    }
#pragma unroll
    for (int gi = 0; gi < 2; ++gi)
#pragma unroll
      for (int j = 0; j < 8; ++j) g[gi].y[j] = g[gi].z[j];
  }
}

// ------------------------------------------------------------------------------------------ host side
template <typename TT>
int launch_forward_bf16x3_duo(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                              hipStream_t s) {
  const Dims dims{(int)n.H, (int)n.C};
  const unsigned blocks = (unsigned)((n.B + 127) / 128);
  const int rc = dispatch_degree(x.degree, [&](auto D) {
    allow_lds(rk4_forward_bf16x3_duo<TT, D()>, BXD_FWD_LDS_BYTES);
    rk4_forward_bf16x3_duo<TT, D()><<<blocks, 256, BXD_FWD_LDS_BYTES, s>>>(
        f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.z0), (const TT*)io.grid, io.n_grid,
        (const TT*)io.t_out, io.n_out, f32(io.z_out), n.B, st.index, f32(st.frac), dims);
    return CDE_OK;
  });
  return rc != CDE_OK ? rc : check_launch();
}

#define CDE_INST(TT)                                                                                                  \
  template int launch_forward_bf16x3_duo<TT>(const Control&, const AffineField&, const ForwardIO&, const Shape&, const StageTable&, hipStream_t);
CDE_INST(float)
CDE_INST(double)
#undef CDE_INST

}  // namespace cde
