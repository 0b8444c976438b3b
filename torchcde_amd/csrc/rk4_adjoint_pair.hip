// rk4_adjoint_pair.hip -- K3p: K3j (rk4_mfma.hip: the continuous-adjoint sweep of the affine field through the shared
// Jacobian) as TWO waves per 32-series tile that share a SIMD.
//
// Why.  K3j runs one wave per SIMD (its 128 dL/dW accumulators and the eight state vectors of the 3/8 rule do not fit
// 256 registers) and a wave overlaps nothing with its own f32 MFMAs (scripts/ubench/mfma_issue.hip): per stage
// 260 MFMAs x 64 cycles + ~1000 vector / LDS instructions x ~4.5 cycles = 21.3 k cycles, of which the matrix pipe is
// busy 16.6 k (0.76 of the f32 peak, profiles/r04_bench_kernel_stats.csv).  The same micro-benchmark shows a second wave
// on the SIMD taking over more than half of the non-MFMA slots (84 -> 74 cycles per [v_mul, MFMA] pair).  So the stage
// is cut along its one loose dependency -- dL/dW, dL/db only CONSUME (z, a, dX) of a stage, nothing reads them back:
//   chain wave  (waves 0..3 of the workgroup, priority 3): the 33 Jacobian rows (132 MFMAs, results in vector registers),
//               f = J z + b dX and a^T J on the vector pipe, the 3/8 rule; at the START of a stage it leaves (z, a)
//               transposed in one of two LDS buffers of its tile and picks up the stage's control derivative;
//   helper wave (waves 4..7; wave w + 4 shares a SIMD with wave w): one stage behind with dL/dW += (w ds a (x) dX)^T z
//               (128 MFMAs, batch = MFMA K) and dL/db -- 136 accumulators, kept in VECTOR registers
//               (-mllvm -amdgpu-mfma-vgpr-form for this file: the allocation of a kernel is max VGPR + max AGPR over both
//               roles, and only <= 256 in total leaves room for two waves per SIMD) -- and two stages AHEAD with the
//               control: it owns the stage table, the coefficient rows and the knot widths, forms dX/dt of every stage
//               and leaves it (plain for the chain wave, weighted by the quadrature weight for itself) in a three-slot LDS
//               ring.  That takes 30 registers and ~50 vector instructions per stage off the chain wave, which then fits
//               256 registers without scratch.
// One s_barrier per stage orders everything: the chain wave writes (z, a) buffer s & 1 and reads ring slot s % 3 before
// barrier s; the helper reads both between barriers s and s + 1 and writes slot (s + 2) % 3; the chain wave's next write to
// buffer s & 1 comes after barrier s + 1.  The matrix pipe sees the chain wave's dependent row chains and the helper's
// eight independent accumulator chains interleaved.
// Measured (profiles/r05_k3_pair_b.log, 32768 series): 5.26 -> 5.01 ms.  Chain / helper priorities make no difference
// (CDE_K3P_FLAGS), nor does, in the f32 form, requesting the helper's LDS operands a K step ahead (the bf16 form's helper
// does gain from it: 0.05 ms per launch, profiles/NOTES.md round 11): what is left is arithmetic -- on gfx950
// the f32 MFMA runs on the vector ALUs (157.3 TFLOP/s is the VECTOR peak), so the other wave's packed FMAs take matrix-pipe
// time too; the second wave only removes the ISSUE gaps a single wave leaves (~5 cycles per instruction down to its ~4 of
// ALU time): 260 MFMAs x 64 + ~950 vector instructions x ~4 = 20.4 k cycles per stage, measured ~21 k.
// Arithmetic: K3j's, operation for operation (same rows, same consume order, same transposes, same dL/dW K order), so
// results are bitwise K3j's; the per-wave partials keep K3j's layout and go through reduce_mfma_partials.
#include "cde_mfma.h"
#include "cde_launch.h"

namespace cde {

namespace {

constexpr int64_t KP_PARTIAL_FLOATS = MH * MC * MH + MH * MC;      // == PARTIAL_FLOATS of rk4_mfma.hip
constexpr int KP_WJ_ROWS = MH + 1;                                 // 32 rows of J + the bias rows
constexpr int KP_WJ_FLOATS = KP_WJ_ROWS * 64 * 4;
constexpr int KP_ZA_FLOATS = 2 * 64 * 20;                          // one stage's transposed (z, a): 64 rows x 20 each
constexpr int KP_TILE_FLOATS = 2 * KP_ZA_FLOATS + 3 * 256 + 3 * 256;   // per tile: 2 x (z^T | a^T), 3 x dX, 3 x weighted dX
constexpr int KP_LDS_FLOATS = KP_WJ_FLOATS + 4 * KP_TILE_FLOATS;
// BX: the weight image as bf16 pieces, [row][piece][k slot] of 8 channels (16 B), stored once per k slot (the two half-lanes
// that read one slot take the same entry; the third MFMA's lower half-lanes read piece 1 again): 50.7 KB, so that with the
// four tiles' buffers the workgroup fits the 160 KB of LDS.
constexpr int KP_WJB_U4 = KP_WJ_ROWS * 3 * 32;
constexpr int KP_WJB_FLOATS = KP_WJB_U4 * 4;
constexpr int KP_LDS_FLOATS_BX = KP_WJB_FLOATS + 4 * KP_TILE_FLOATS;
static_assert(KP_LDS_FLOATS_BX * 4 <= 160 * 1024, "BX workgroup exceeds the LDS of a CU");
using kp_bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using kp_u32x4 = __attribute__((ext_vector_type(4))) unsigned;

__device__ __forceinline__ void kp_swap32(float& x, float& y) {    // x[lanes 32..63] <-> y[lanes 0..31]
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  x = __uint_as_float(r[0]);
  y = __uint_as_float(r[1]);
}
__device__ __forceinline__ float kp_wj_image(const float* __restrict__ W, const float* __restrict__ bias, int h, int s, int l,
                                             Dims d) {
  const int k = rho(l & 31), c = 2 * s + (l >> 5);
  if (c >= d.C || k >= d.H) return 0.f;
  if (h < MH) return h < d.H ? W[(h * d.C + c) * d.H + k] : 0.f;
  return bias[k * d.C + c];
}
// x = a + b + c in bf16 pieces (each the round-to-nearest bf16 of what the larger ones leave)
__device__ __forceinline__ void kp_split3(float x, __bf16& a, __bf16& b, __bf16& c) {
  a = (__bf16)x;
  const float r1 = x - (float)a;
  b = (__bf16)r1;
  c = (__bf16)(r1 - (float)b);
}
// kp_split3 of two values at once, the pieces already packed as the MFMA operands take them: word m holds piece m + 1 of
// x0 in its low and of x1 in its high half.  One v_cvt_pk_bf16_f32 per piece pair (the same rounding as the scalar cast,
// which converts one value per instruction and then needs a second instruction to pack two pieces into a word).  A vector
// conversion, not inline asm: the compiler then sees the VALU write and gives the MFMA that reads the word its wait states.
using kp_bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
__device__ __forceinline__ unsigned kp_cvt_pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, kp_bf16x2));
}
__device__ __forceinline__ void kp_split3x2(float x0, float x1, unsigned& a, unsigned& b, unsigned& c) {
  a = kp_cvt_pk_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(a << 16), r1 = x1 - __uint_as_float(a & 0xffff0000u);
  b = kp_cvt_pk_bf16(r0, r1);
  c = kp_cvt_pk_bf16(r0 - __uint_as_float(b << 16), r1 - __uint_as_float(b & 0xffff0000u));
}
// piece m of the 8 channel weights of row h at k slot j (hidden unit k = rho(j)); row MH: the bias rows
__device__ __forceinline__ kp_u32x4 kp_wjb_image(const float* __restrict__ W, const float* __restrict__ bias, int h, int m, int j,
                                                 Dims d) {
  const int k = rho(j);
  kp_bf16x8 out;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float w = 0.f;
    if (c < d.C && k < d.H) w = h < MH ? (h < d.H ? W[(h * d.C + c) * d.H + k] : 0.f) : bias[k * d.C + c];
    __bf16 p1, p2, p3;
    kp_split3(w, p1, p2, p3);
    out[c] = m == 0 ? p1 : m == 1 ? p2 : p3;
  }
  return __builtin_bit_cast(kp_u32x4, out);
}
// Packed f32 in the chain wave of the bf16 form (BX): the number of J rows of a stage whose consume is v_pk_fma_f32 -- 0,
// 16 (the odd rows) or 32 -- is a compile-time constant (-DKP_PACK_CHAIN_ROWS=.. for A/B builds); the f32 form and
// rk4_backprop_jacobian_pair never take this path.  What packed f32 costs beside the partner wave's bf16 MFMAs, and the parts
// that were built and not kept, are in the BX comment below and in profiles/NOTES.md (round 12).
#ifndef KP_PACK_CHAIN_ROWS
#define KP_PACK_CHAIN_ROWS 32
#endif
constexpr int KP_PK_CHAIN_ROWS = KP_PACK_CHAIN_ROWS;
static_assert(KP_PK_CHAIN_ROWS == 0 || KP_PK_CHAIN_ROWS == 16 || KP_PK_CHAIN_ROWS == 32, "KP_PACK_CHAIN_ROWS: 0, 16 or 32");

// the stage barrier: this wave's LDS traffic done, then all eight waves meet
__device__ __forceinline__ void kp_stage_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// METHOD (CDE_METHOD_*): the 3/8 rule, or torchdiffeq's midpoint / euler on the same augmented system -- two stages / one
// stage per step, quadrature weights (0, ds) / (ds) for the parameter gradients (a zero-weight stage costs the helper nothing).
// BX: both GEMMs on the bf16 matrix pipe.  The J rows as K3bj forms them (rk4_mfma.hip): three v_mfma_f32_32x32x16_bf16
// per row take the six piece products W_i dX_j with i + j <= 4, float32 accumulation, in K3bj's order -- so dL/dz0 and the
// trajectories are bitwise K3bj's.  The helper's dL/dW: 12 bf16 MFMAs per channel tile (six piece products x two K blocks
// of 16 series) instead of 16 f32 ones, its operands split on the helper itself with non-packed vector instructions, which
// hide in the chain wave's MFMA gaps (scripts/ubench/mfma_bf16_fill.hip).  dL/db keeps the f32 form's fma order.
// Packed f32 beside bf16 MFMAs (round 12, scripts/ubench/mfma_bf16_pk_issue.hip, profiles/NOTES.md).  This kernel is bound
// by the instruction issue of its two waves (~3,000 instructions per stage and SIMD at ~4 cycles, the matrix pipe busy 0.43),
// and a v_pk_* f32 instruction costs MORE than a non-packed one -- it is no free pair -- but less than the two it replaces.
// So what is written packed is what halves a large instruction count: the chain's J-row consume (32 v_fma_f32 -> 16
// v_pk_fma_f32 per row: 3.42 -> 3.33 ms per launch).  A packed instruction that replaces ONE scalar one loses (the sum of a
// row's two partial-sum halves is kept scalar by a fence: 0.02 ms); the 3/8-rule update as packed arithmetic gained 0.014 ms
// on the kernel and nothing that the step's timing resolves, and is not kept; packing the helper's products and split
// remainders (64 v_pk_mul_f32 + 128 v_pk_add_f32 for 384 scalar ones per stage) made the launch slower than no packing at
// all, 3.33 -> 3.44 ms -- the helper's vector work is what hides under the chain's MFMAs, and packed f32 does not hide.
// Every packed operation rounds element for element as the scalar one it replaces: all results are bitwise the same.
template <typename TT, int DEGREE, int METHOD = CDE_METHOD_RK4, bool BX = false>
__global__ __launch_bounds__(512, 2) void rk4_adjoint_jacobian_pair(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ z_saved,
    const float* __restrict__ grad_out, const TT* __restrict__ sgrid, const int64_t* __restrict__ seg_off,
    int64_t n_out, float* __restrict__ grad_z0, float* __restrict__ partial, int64_t B,
    const int64_t* __restrict__ stage_index, const float* __restrict__ stage_frac, Dims dims, int flags) {
  const int Hr = dims.H, Cr = dims.C;
  constexpr int NS = METHOD == CDE_METHOD_RK4 ? 4 : METHOD == CDE_METHOD_MIDPOINT ? 2 : 1;     // stages per step
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(!BX || METHOD == CDE_METHOD_RK4, "BX: rk4 only");
  if constexpr (BX) {
    kp_u32x4* img = reinterpret_cast<kp_u32x4*>(lds);
    for (int e = threadIdx.x; e < KP_WJB_U4; e += 512) img[e] = kp_wjb_image(W, bias, e / 96, (e >> 5) % 3, e & 31, dims);
  } else {
    for (int e = threadIdx.x; e < KP_WJ_FLOATS; e += 512) lds[e] = kp_wj_image(W, bias, e >> 8, e & 3, (e >> 2) & 63, dims);
  }
  const float4* wj = reinterpret_cast<const float4*>(lds);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int slot = wave & 3;                                       // the tile of this wave within the workgroup
  const bool helper = wave >= 4;
  const int n = lane & 31, half = lane >> 5;
  // per tile: [2 x (z^T | a^T)] [3 x dX] [3 x weighted dX]          (KP_TILE_FLOATS)
  float* tile_lds = lds + (BX ? KP_WJB_FLOATS : KP_WJ_FLOATS) + slot * KP_TILE_FLOATS;
  float* ring_dx = tile_lds + 2 * KP_ZA_FLOATS;                      // + (stage % 3) * 256: dX_c of series n at [n*8 + c]
  float* ring_dw = ring_dx + 3 * 256;                                // + (stage % 3) * 256: (quadrature weight * ds) * dX_c

  const int64_t tile = (int64_t)blockIdx.x * 4 + slot;
  const bool live = tile * 32 < B;                                  // (dead tiles keep pace with the barriers, store nothing)
  const int64_t series = tile * 32 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;

  if (helper) {
    // ------------------------------------------------------------------------------------------ helper wave
    f32x16 accW[MC];
    f32x2 gbp[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};   // dL/db partials, channel pairs
#pragma unroll
    for (int c = 0; c < MC; ++c) {
#pragma unroll
      for (int r = 0; r < 16; ++r) accW[c][r] = 0.f;
    }
    // the stages in sweep order: entry e = 4 k + stage of the stage table, k over the steps of segment p = 0, 1, ..
    int64_t n_stages = 0;
    for (int64_t p = 0; p + 1 < n_out; ++p) {
      const int64_t k_begin = seg_off[p], k_end = seg_off[p + 1] - 1;
      if (k_end > k_begin) n_stages += NS * (k_end - k_begin);
    }
    if (flags & 2) __builtin_amdgcn_s_setprio(3);
    // A cursor over those entries runs THREE stages ahead of the dL/dW work: the control derivative of stage st + 2 is
    // published (LDS ring of three slots; the chain wave reads slot st % 3 at the start of stage st, this wave's dL/dW of
    // stage st reads the weighted copy) from a row / fraction / step size requested one iteration earlier, and the
    // interval index of the stage after that is requested one iteration before its row -- no dependent global load is
    // waited for where it was issued.
    int64_t cur_p = -1, cur_e = 0, cur_end = 0;
    bool cur_ok = false;
    auto advance = [&]() {                     // (the table keeps four slots per step; a method uses the first NS of them)
      if (cur_ok && (cur_e & 3) + 1 < NS) { ++cur_e; return; }
      if (cur_ok && (cur_e | 3) + 1 < cur_end) { cur_e = (cur_e | 3) + 1; return; }
      cur_ok = false;
      for (int64_t p = cur_p + 1; p + 1 < n_out; ++p) {
        const int64_t k_begin = seg_off[p], k_end = seg_off[p + 1] - 1;
        if (k_end > k_begin) { cur_p = p; cur_e = 4 * k_begin; cur_end = 4 * k_end; cur_ok = true; return; }
      }
    };
    Row<DEGREE> row;
    int64_t row_idx = -1, idx_ahead = -1;
    float p_frac = 0.f, p_wq = 0.f, p_width = 1.f;
    bool p_ok = false;
    auto fetch = [&]() {                       // cursor's stage -> (row, p_*); then the cursor moves on and its index is requested
      p_ok = cur_ok;
      if (cur_ok) {
        if (idx_ahead != row_idx) { row = load_row<DEGREE>(coeffs, sc, n_intervals, idx_ahead, Cr); row_idx = idx_ahead; }
        p_frac = stage_frac[cur_e];
        if (DEGREE == CDE_PATH_LINEAR) p_width = knots[idx_ahead + 1] - knots[idx_ahead];
        const int64_t k = cur_e >> 2;
        const int stage = (int)(cur_e & 3);
        const float ds = (float)(sgrid[k + 1] - sgrid[k]);
        if constexpr (METHOD == CDE_METHOD_RK4) p_wq = ((stage == 0 || stage == 3) ? 0.125f : 0.375f) * ds;   // 3/8-rule quadrature weight
        else if constexpr (METHOD == CDE_METHOD_MIDPOINT) p_wq = stage == 1 ? ds : 0.f;                        // the midpoint evaluation alone
        else p_wq = ds;
      }
      advance();
      if (cur_ok) idx_ahead = stage_index[cur_e];
    };
    auto publish = [&](int which) {             // dX of the fetched stage -> ring slot `which` (plain and weighted)
      if (!p_ok) return;
      float dX[MC];
      control_slope<DEGREE>(row, p_frac, p_width, dX);
      const f32x2 d0 = half ? f32x2{dX[4], dX[5]} : f32x2{dX[0], dX[1]}, d1 = half ? f32x2{dX[6], dX[7]} : f32x2{dX[2], dX[3]};
      *reinterpret_cast<float4*>(ring_dx + which * 256 + n * 8 + 4 * half) = make_float4(d0[0], d0[1], d1[0], d1[1]);
      const f32x2 w0 = d0 * p_wq, w1 = d1 * p_wq;
      if constexpr (BX) {                      // channel-major [c][series parity][series >> 1]: the K order of the bf16 MFMAs
        float* wr = ring_dw + which * 256 + 4 * half * 32 + (n & 1) * 16 + (n >> 1);
        wr[0] = w0[0]; wr[32] = w0[1]; wr[64] = w1[0]; wr[96] = w1[1];
      } else {
        *reinterpret_cast<float4*>(ring_dw + which * 256 + n * 8 + 4 * half) = make_float4(w0[0], w0[1], w1[0], w1[1]);
      }
    };
    advance();
    if (cur_ok) idx_ahead = stage_index[cur_e];
    fetch(); publish(0);                                            // stages 0 and 1 before the first barrier
    fetch(); publish(1);
    fetch();                                                        // stage 2: in flight
    __syncthreads();                                                // (also: the weight image is staged)
    int par = 0, rs = 0, cs = 0;                                    // (z, a) buffer, ring slot and stage-in-step of stage st
    for (int64_t st = 0; st < n_stages; ++st) {
      kp_stage_barrier();                                           // barrier `st`: buffer `par` holds (z, a) of stage `st`
      // (BX) the operands of the stage's first block, requested in front of publish / fetch: buffer `par` and ring slot `rs`
      // are complete at barrier `st`, and publish writes another slot
      float4 hz0, hz1, ha0, ha1, he0, he1;
      if constexpr (BX) {
        const float* base = tile_lds + par * KP_ZA_FLOATS;
        const float4* zt4 = reinterpret_cast<const float4*>(base + (half * 32 + n) * 20);
        const float4* at4 = reinterpret_cast<const float4*>(base + 64 * 20 + (half * 32 + n) * 20);
        const float4* dw4 = reinterpret_cast<const float4*>(ring_dw + rs * 256 + half * 16);
        hz0 = zt4[0]; hz1 = zt4[1]; ha0 = at4[0]; ha1 = at4[1]; he0 = dw4[0]; he1 = dw4[1];
      }
      publish(rs >= 1 ? rs - 1 : 2);                                // stage st + 2 -> slot (st + 2) % 3
      fetch();                                                      // stage st + 3: requested, used next iteration
      const bool weighted = METHOD != CDE_METHOD_MIDPOINT || cs == 1;      // midpoint: the first evaluation carries no weight
      cs = cs + 1 == NS ? 0 : cs + 1;
      if (weighted && BX) {
      // (BX) dL/dW tile c on the bf16 pipe: D[h][k] += sum_series v_c[h] z_k with v_c = (w ds dX_c) a_h, both operands split
      // into three bf16 pieces and the six piece products with i + j <= 4 taken, smallest first.  MFMA K = 16 series:
      // this lane supplies K index 8 * half + j = series 2 (8 g + j) + half, row h = n (A: v of a_n), column k = n (B: z_n);
      // two K blocks g per tile.  dL/db as before: sum_series (w ds dX_c) a_n, the same fma order (bitwise the f32 form's).
      // The operands of block (g, c + 1) -- after c = 7, of block (g + 1, 0) with the next K block's z / a rows -- are
      // requested from LDS before the MFMAs of block (g, c) are issued, as the f32 form does for its K steps: the wave then
      // starts a block's splits on operands that have had six MFMAs to arrive, not on a round trip it has just begun.
      const float* base = tile_lds + par * KP_ZA_FLOATS;
      const float4* zt4 = reinterpret_cast<const float4*>(base + (half * 32 + n) * 20);
      const float4* at4 = reinterpret_cast<const float4*>(base + 64 * 20 + (half * 32 + n) * 20);
      const float4* dw4 = reinterpret_cast<const float4*>(ring_dw + rs * 256 + half * 16);   // + c * 8 + g * 2: 8 series
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const float4 z0 = hz0, z1 = hz1, a0 = ha0, a1 = ha1;
        const float zv[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        kp_u32x4 zw1, zw2, zw3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned p1, p2, p3;
          kp_split3x2(zv[2 * i], zv[2 * i + 1], p1, p2, p3);
          zw1[i] = p1; zw2[i] = p2; zw3[i] = p3;
        }
        const kp_bf16x8 zp1 = __builtin_bit_cast(kp_bf16x8, zw1), zp2 = __builtin_bit_cast(kp_bf16x8, zw2),
                        zp3 = __builtin_bit_cast(kp_bf16x8, zw3);
#pragma unroll
        for (int c = 0; c < MC; ++c) {
          const float4 e0 = he0, e1 = he1;
          const float ev[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
          kp_u32x4 vw1, vw2, vw3;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            unsigned p1, p2, p3;
            kp_split3x2(ev[2 * i] * av[2 * i], ev[2 * i + 1] * av[2 * i + 1], p1, p2, p3);
            vw1[i] = p1; vw2[i] = p2; vw3[i] = p3;
            gbp[c >> 1][c & 1] = __builtin_fmaf(ev[2 * i], av[2 * i], gbp[c >> 1][c & 1]);
            gbp[c >> 1][c & 1] = __builtin_fmaf(ev[2 * i + 1], av[2 * i + 1], gbp[c >> 1][c & 1]);
          }
          const kp_bf16x8 vp1 = __builtin_bit_cast(kp_bf16x8, vw1), vp2 = __builtin_bit_cast(kp_bf16x8, vw2),
                          vp3 = __builtin_bit_cast(kp_bf16x8, vw3);
          __builtin_amdgcn_sched_barrier(0);       // the requests stay behind this block's waits and in front of its MFMAs
          if (c < MC - 1) {
            he0 = dw4[(c + 1) * 8 + 2 * g]; he1 = dw4[(c + 1) * 8 + 2 * g + 1];
          } else if (g == 0) {
            he0 = dw4[2]; he1 = dw4[3];
            hz0 = zt4[2]; hz1 = zt4[3]; ha0 = at4[2]; ha1 = at4[3];
          }
          __builtin_amdgcn_sched_barrier(0);
          f32x16 acc = accW[c];
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vp3, zp1, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vp1, zp3, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vp2, zp2, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vp2, zp1, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vp1, zp2, acc, 0, 0, 0);
          accW[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vp1, zp1, acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      } else if (weighted) {
      // dL/dW tile c: D[h][k] += sum_series (w ds a_h dX_c)[series] * z_k[series]; this lane feeds MFMA K index `half`
      // of K-step s2, i.e. series 2*s2 + half, row h = n, column k = n.  Operands of K-step s2 + 1 are requested from LDS
      // before the MFMAs of K-step s2 are issued (their issue blocks this wave for as long as they take).
      const float* base = tile_lds + par * KP_ZA_FLOATS;
      const float4* zt4 = reinterpret_cast<const float4*>(base + (half * 32 + n) * 20);
      const float4* at4 = reinterpret_cast<const float4*>(base + 64 * 20 + (half * 32 + n) * 20);
      const float4* dw4 = reinterpret_cast<const float4*>(ring_dw + rs * 256 + half * 8);      // + s2*4 (16 floats per s2)
      float4 zq = zt4[0], aq = at4[0], e0 = dw4[0], e1 = dw4[1];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int i = s2 & 3;
        const f32x2 e01 = {e0.x, e0.y}, e23 = {e0.z, e0.w}, e45 = {e1.x, e1.y}, e67 = {e1.z, e1.w};
        const f32x2 asrc = i < 2 ? f32x2{aq.x, aq.y} : f32x2{aq.z, aq.w};
        const float zb = i == 0 ? zq.x : i == 1 ? zq.y : i == 2 ? zq.z : zq.w;
        f32x2 v01, v23, v45, v67;
        if (i & 1) {
          v01 = pk_mul_hi(e01, asrc); v23 = pk_mul_hi(e23, asrc); v45 = pk_mul_hi(e45, asrc); v67 = pk_mul_hi(e67, asrc);
          pk_fma_hi(gbp[0], e01, asrc); pk_fma_hi(gbp[1], e23, asrc); pk_fma_hi(gbp[2], e45, asrc); pk_fma_hi(gbp[3], e67, asrc);
        } else {
          v01 = pk_mul_lo(e01, asrc); v23 = pk_mul_lo(e23, asrc); v45 = pk_mul_lo(e45, asrc); v67 = pk_mul_lo(e67, asrc);
          pk_fma_lo(gbp[0], e01, asrc); pk_fma_lo(gbp[1], e23, asrc); pk_fma_lo(gbp[2], e45, asrc); pk_fma_lo(gbp[3], e67, asrc);
        }
        if (s2 < 15) {
          e0 = dw4[(s2 + 1) * 4]; e1 = dw4[(s2 + 1) * 4 + 1];
          if (i == 3) { zq = zt4[(s2 + 1) >> 2]; aq = at4[(s2 + 1) >> 2]; }
        }
        __builtin_amdgcn_sched_barrier(0);
        accW[0] = mfma(v01[0], zb, accW[0]); accW[1] = mfma(v01[1], zb, accW[1]);
        accW[2] = mfma(v23[0], zb, accW[2]); accW[3] = mfma(v23[1], zb, accW[3]);
        accW[4] = mfma(v45[0], zb, accW[4]); accW[5] = mfma(v45[1], zb, accW[5]);
        accW[6] = mfma(v67[0], zb, accW[6]); accW[7] = mfma(v67[1], zb, accW[7]);
        __builtin_amdgcn_sched_barrier(0);
      }
      }
      par ^= 1;
      rs = rs == 2 ? 0 : rs + 1;
    }
    if (live) {
      // per-wave partial parameter gradients (summed in tile order by reduce_mfma_partials), K3j's layout
      float* my_partial = partial + tile * KP_PARTIAL_FLOATS;
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
    return;
  }

  // -------------------------------------------------------------------------------------------- chain wave
  if (flags & 1) __builtin_amdgcn_s_setprio(3);  // the critical path: the helper's MFMAs fill the pipe while this wave is on the vector pipe
  f32x16 y0, a0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int u = 2 * r + half;
    const bool on = u < Hr;
    y0[r] = on ? z_saved[(sc * n_out + (n_out - 1)) * Hr + u] : 0.f;
    a0[r] = (valid && on) ? grad_out[(sc * n_out + (n_out - 1)) * Hr + u] : 0.f;   // a == 0 stays 0: padded lanes add nothing to dL/dW
  }
  __syncthreads();                               // the weight image and the helper's first two control derivatives are in LDS
  int par = 0, rs = 0;                           // (z, a) buffer and control-derivative slot of the current stage
  for (int64_t p = 0; p + 1 < n_out; ++p) {
    const int64_t i_out = n_out - 1 - p;
    const int64_t k_begin = seg_off[p], k_end = seg_off[p + 1] - 1;   // steps k_begin .. k_end-1
    for (int64_t k = k_begin; k < k_end; ++k) {
      const float ds = (float)(sgrid[k + 1] - sgrid[k]);
      f32x16 ky1, ky2, ka1, ka2, yst = y0, ast = a0;
#pragma unroll
      for (int stage = 0; stage < NS; ++stage) {
        // ---- this stage's control derivative (the helper wave left it two stages ago), the stage state -> this stage's
        // buffer (transposed); then the stage barrier
        float bs0, bs1, bs2, bs3;
        kp_u32x4 b01, b2;                        // (BX) bf16 pieces of the 8 channel values: lower half-lanes d1 | d3, upper d2 | d1
        {
          const float4 dA = *reinterpret_cast<const float4*>(ring_dx + rs * 256 + n * 8);
          const float4 dB = *reinterpret_cast<const float4*>(ring_dx + rs * 256 + n * 8 + 4);
          if constexpr (BX) {
            const float dx[8] = {dA.x, dA.y, dA.z, dA.w, dB.x, dB.y, dB.z, dB.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {                // channels 2i, 2i + 1 per word
              unsigned p1, p2, p3;
              kp_split3x2(dx[2 * i], dx[2 * i + 1], p1, p2, p3);
              b01[i] = half ? p2 : p1;
              b2[i] = half ? p1 : p3;
            }
          } else {
            bs0 = half ? dA.y : dA.x; bs1 = half ? dA.w : dA.z; bs2 = half ? dB.y : dB.x; bs3 = half ? dB.w : dB.z;
          }
          float* base = tile_lds + par * KP_ZA_FLOATS;
          float* wz = base + ((n & 1) * 32 + half) * 20 + (n >> 1);                // + 2r*20
          float* wa = base + 64 * 20 + ((n & 1) * 32 + half) * 20 + (n >> 1);
#pragma unroll
          for (int r = 0; r < 16; ++r) { wz[r * 40] = yst[r]; wa[r * 40] = ast[r]; }
          kp_stage_barrier();
          par ^= 1;
          rs = rs == 2 ? 0 : rs + 1;
        }

        // ---- J = sum_c dX_c W_c one row (hidden unit h) at a time: 4 MFMAs leave J[h][k] of this lane's series in
        // the lane, k = the 16 units it owns; f_h += J[h][.] . z and va += a_h J[h][.] follow on the vector pipe
        // (K3j's code: rows issued one ahead of their use, explicit wait states after the last issue).
        f32x16 f, va;
        {
          // a^T J: the f32 form keeps it in `vs` and sums with `consume`; the bf16 form keeps it on register pairs
          // (vs[2j], vs[2j + 1]) in `vs2` and sums with `consume2`.  Each instantiation uses one of the two and the other is
          // dead code; `consume` is the reference for the order of operations, `consume2` must match it element for element.
          float vs[16];
          f32x2 vs2[8];
          if constexpr (BX) {
#pragma unroll
            for (int j = 0; j < 8; ++j) vs2[j] = f32x2{0.f, 0.f};
          } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) vs[j] = 0.f;
          }
          int opaque = 0;                               // the image reads are loop invariant: keep them inside the stage
          asm volatile("" : "+v"(opaque));
          const float4* wp = wj + lane + opaque;
          // (BX) row h's pieces: [3h][j], [3h + 1][j] and, for the third MFMA, [3h][j] (lower half-lanes) / [3h + 2][j]
          const kp_u32x4* wpb = reinterpret_cast<const kp_u32x4*>(lds) + (lane & 31) + opaque;
          const int third = half ? 64 : 0;
          struct RowImage { float4 a; kp_u32x4 m0, m1, m2; };
          auto image = [&](int h) {
            RowImage r;
            if constexpr (BX) { r.m0 = wpb[h * 96]; r.m1 = wpb[h * 96 + 32]; r.m2 = wpb[h * 96 + third]; }
            else r.a = wp[h * 64];
            return r;
          };
          auto issue = [&](f32x16& J, const RowImage& a) {
            __builtin_amdgcn_sched_barrier(0);           // everything that still reads the old J stays above
            if constexpr (BX) {
              asm volatile("s_nop 1\n\t"                                     // (operands may be fresh VALU results)
                           "v_mfma_f32_32x32x16_bf16 %0, %3, %5, 0\n\t"      // smallest terms first (K3bj's order)
                           "v_mfma_f32_32x32x16_bf16 %0, %2, %4, %0\n\t"
                           "v_mfma_f32_32x32x16_bf16 %0, %1, %4, %0"
                           : "=&v"(J) : "v"(a.m0), "v"(a.m1), "v"(a.m2), "v"(b01), "v"(b2));
            } else {
              asm volatile("s_nop 1\n\t"                                     // (operands may be fresh VALU results)
                           "v_mfma_f32_32x32x2_f32 %0, %1, %5, 0\n\t"
                           "v_mfma_f32_32x32x2_f32 %0, %2, %6, %0\n\t"
                           "v_mfma_f32_32x32x2_f32 %0, %3, %7, %0\n\t"
                           "v_mfma_f32_32x32x2_f32 %0, %4, %8, %0"
                           : "=&v"(J) : "v"(a.a.x), "v"(a.a.y), "v"(a.a.z), "v"(a.a.w), "v"(bs0), "v"(bs1), "v"(bs2), "v"(bs3));
            }
            __builtin_amdgcn_sched_barrier(0);
          };
          // f_h's share: four partial sums (even / odd register pairs, low / high element), (p0 + q0) + (p1 + q1) -- the
          // packed form's order, element by element, so the sums are bitwise K3j's / K3bj's
          auto consume = [&](const f32x16& J, float ah) {
            float p0 = 0.f, p1 = 0.f, q0 = 0.f, q1 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (j & 1) {
                q0 = __builtin_fmaf(J[2 * j], yst[2 * j], q0);
                q1 = __builtin_fmaf(J[2 * j + 1], yst[2 * j + 1], q1);
              } else {
                p0 = __builtin_fmaf(J[2 * j], yst[2 * j], p0);
                p1 = __builtin_fmaf(J[2 * j + 1], yst[2 * j + 1], p1);
              }
              vs[2 * j] = __builtin_fmaf(J[2 * j], ah, vs[2 * j]);
              vs[2 * j + 1] = __builtin_fmaf(J[2 * j + 1], ah, vs[2 * j + 1]);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) asm volatile("" : "+v"(vs[j]));
            return (p0 + q0) + (p1 + q1);
          };
          // (BX) the same sums on register pairs: p = (p0, p1), q = (q0, q1) and vs2[j] each take one v_pk_fma_f32 per pair
          // of J (element for element the scalar form's operations, so the same bits); a_h is the low (hi = false) or high
          // element of `aeo`, broadcast by op_sel.  Rows that are not packed (KP_PK_CHAIN_ROWS) run the scalar form on the
          // same registers.
          auto consume2 = [&](const f32x16& J, f32x2 aeo, bool hi, bool packed) {
            const float ah = hi ? aeo[1] : aeo[0];
            float s;
            if (packed) {
              f32x2 p = {0.f, 0.f}, q = {0.f, 0.f};
              const f32x2 ah2 = {ah, ah};
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const f32x2 Jp = {J[2 * j], J[2 * j + 1]}, yp = {yst[2 * j], yst[2 * j + 1]};
                if (j & 1) q = __builtin_elementwise_fma(Jp, yp, q);
                else p = __builtin_elementwise_fma(Jp, yp, p);
                vs2[j] = __builtin_elementwise_fma(Jp, ah2, vs2[j]);
              }
              const f32x2 pq = p + q;                      // (p0 + q0, p1 + q1)
              float s0 = pq[0], s1 = pq[1];
              asm volatile("" : "+v"(s0), "+v"(s1));       // or the compiler adds the two halves with a second v_pk_add_f32
              s = s0 + s1;
            } else {
              float p0 = 0.f, p1 = 0.f, q0 = 0.f, q1 = 0.f;
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                if (j & 1) {
                  q0 = __builtin_fmaf(J[2 * j], yst[2 * j], q0);
                  q1 = __builtin_fmaf(J[2 * j + 1], yst[2 * j + 1], q1);
                } else {
                  p0 = __builtin_fmaf(J[2 * j], yst[2 * j], p0);
                  p1 = __builtin_fmaf(J[2 * j + 1], yst[2 * j + 1], p1);
                }
                vs2[j][0] = __builtin_fmaf(J[2 * j], ah, vs2[j][0]);
                vs2[j][1] = __builtin_fmaf(J[2 * j + 1], ah, vs2[j][1]);
              }
              s = (p0 + q0) + (p1 + q1);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(vs2[j]));
            return s;
          };
          f32x16 Je, Jo;                                 // rows 2r / 2r + 1 in flight
          if constexpr (BX) {
            // one row image in flight (12 registers): requested right after the previous row's issue, a consume ahead
            // of its own (the chain wave has no room for two).  Hazards: the ds_read that overwrites the image registers
            // follows the three MFMAs that read them as SrcA.  gfx950 has a write-after-read hazard only on an MFMA's SrcC
            // (read over its passes); SrcA / SrcB are read when the MFMA issues, so the overwrite needs no wait states.
            // SrcC here is J, which nothing else writes until its consume; the consume reads J after the next row's
            // MFMAs have issued behind it in the in-order pipe, as in the f32 form.
            RowImage img = image(0);
            issue(Je, img);
            img = image(1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              issue(Jo, img);
              img = image(2 * r + 2);                    // row 2r + 2 (r = 15: the bias rows)
              asm volatile("" : "+v"(Je));
              float ae = ast[r], ao = ast[r];
              kp_swap32(ae, ao);
              const f32x2 aeo = {ae, ao};
              float X = consume2(Je, aeo, false, KP_PK_CHAIN_ROWS == 32);
              issue(Je, img);
              if (r < 15) img = image(2 * r + 3);
              asm volatile("" : "+v"(Jo));
              float Y = consume2(Jo, aeo, true, KP_PK_CHAIN_ROWS >= 16);
              kp_swap32(X, Y);
              f[r] = X + Y;
            }
          } else {
          RowImage a_cur = image(0), a_nxt = image(1);
          issue(Je, a_cur);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            a_cur = image(2 * r + 2);                    // image of row 2r + 2 (r = 15: the bias rows)
            issue(Jo, a_nxt);
            asm volatile("" : "+v"(Je));
            float ae = ast[r], ao = ast[r];
            kp_swap32(ae, ao);
            float X = consume(Je, ae);
            if (r < 15) a_nxt = image(2 * r + 3);
            issue(Je, a_cur);
            asm volatile("" : "+v"(Jo));
            float Y = consume(Jo, ao);
            kp_swap32(X, Y);                             // ... and each half-lane collects the f of the unit it owns
            f[r] = X + Y;
          }
          }
          // Je: (b dX)_h for the units this lane owns.  16-pass MFMA result -> VALU read: wait states
          asm volatile("s_nop 15\n\ts_nop 7" : "+v"(Je));
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            f[r] += Je[r];
            va[r] = BX ? vs2[r >> 1][r & 1] : vs[r];
          }
        }

        // ---- reverse-time dynamics: dy/ds = -f, da/ds = +a^T df/dz.  3/8 rule in two slots per variable; element by
        // element in scalar (non-packed) instructions, each expression in its original order
        const float third = (float)(1.0 / 3.0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ky = -f[r], ka = va[r];
          if constexpr (METHOD == CDE_METHOD_EULER) {                  // y1 = y0 + ds * k
            yst[r] = y0[r] + ds * ky;
            ast[r] = a0[r] + ds * ka;
          } else if constexpr (METHOD == CDE_METHOD_MIDPOINT) {        // mid = y0 + k1 * half_ds; y1 = y0 + ds * k(mid)
            const float half_ds = 0.5f * ds;
            if (stage == 0) { yst[r] = y0[r] + ky * half_ds; ast[r] = a0[r] + ka * half_ds; }
            else { yst[r] = y0[r] + ds * ky; ast[r] = a0[r] + ds * ka; }
          } else if (stage == 0) {
            ky1[r] = ky; ka1[r] = ka;
            yst[r] = y0[r] + ds * ky * third;
            ast[r] = a0[r] + ds * ka * third;
          } else if (stage == 1) {
            ky2[r] = ky; ka2[r] = ka;
            yst[r] = y0[r] + ds * (ky - ky1[r] * third);
            ast[r] = a0[r] + ds * (ka - ka1[r] * third);
          } else if (stage == 2) {
            yst[r] = y0[r] + ds * (ky1[r] - ky2[r] + ky);
            ast[r] = a0[r] + ds * (ka1[r] - ka2[r] + ka);
            ky1[r] = ky1[r] + 3.f * (ky2[r] + ky);
            ka1[r] = ka1[r] + 3.f * (ka2[r] + ka);
          } else {
            yst[r] = y0[r] + (ky1[r] + ky) * ds * 0.125f;
            ast[r] = a0[r] + (ka1[r] + ka) * ds * 0.125f;
          }
        }
      }
      y0 = yst; a0 = ast;
    }
    // torchdiffeq adjoint: re-seed y from the stored forward value, add the incoming gradient
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
}


// ------------------------------------------------------------------------------------------ K3d as a pair (adjoint=False)
// rk4_backprop.hip's reverse-mode sweep (identity-activation affine field) with the same cut: the chain wave reads the stored
// stage state s_i, forms the 32 Jacobian rows, v_i = J_i^T kb_i on the vector pipe and the kb bookkeeping; the helper wave
// runs dL/dW += (kb_i (x) dX_i)^T s_i one stage behind and the control derivative two stages ahead (the FORWARD stage table,
// walked backwards; one ring: the products carry no quadrature weight).  Same arithmetic as rk4_backprop_jacobian.
template <int DEGREE>
__global__ __launch_bounds__(512, 2) void rk4_backprop_jacobian_pair(
    const float* __restrict__ coeffs, const float* __restrict__ knots, int64_t n_intervals,
    const float* __restrict__ W, const float* __restrict__ stages, const float* __restrict__ grad_out, int64_t n_out,
    const float* __restrict__ step_dt, int64_t n_steps, const int64_t* __restrict__ node_ptr,
    const int64_t* __restrict__ node_out, const float* __restrict__ node_weight, float* __restrict__ grad_z0,
    float* __restrict__ partial, int64_t B, const int64_t* __restrict__ stage_index,
    const float* __restrict__ stage_frac, Dims dims) {
  const int Hr = dims.H, Cr = dims.C;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int e = threadIdx.x; e < KP_WJ_FLOATS; e += 512) lds[e] = kp_wj_image(W, W, e >> 8, e & 3, (e >> 2) & 63, dims);   // (row 32 unused)
  const float4* wj = reinterpret_cast<const float4*>(lds);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int slot = wave & 3;
  const bool helper = wave >= 4;
  const int n = lane & 31, half = lane >> 5;
  float* tile_lds = lds + KP_WJ_FLOATS + slot * KP_TILE_FLOATS;
  float* ring_dx = tile_lds + 2 * KP_ZA_FLOATS;                      // + (stage counter % 3) * 256: dX_c of series n at [n*8 + c]
  const int64_t tile = (int64_t)blockIdx.x * 4 + slot;
  const bool live = tile * 32 < B;
  const int64_t series = tile * 32 + n;
  const bool valid = series < B;
  const int64_t sc = valid ? series : B - 1;
  const int64_t n_stages = 4 * n_steps;

  if (helper) {
    f32x16 accW[MC];
    f32x2 gbp[4] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
#pragma unroll
    for (int c = 0; c < MC; ++c) {
#pragma unroll
      for (int r = 0; r < 16; ++r) accW[c][r] = 0.f;
    }
    // cursor over the forward table's entries, last first; the interval index of the entry after the fetched one is requested
    // one iteration before its row (as in the adjoint's helper)
    int64_t cur_e = n_stages;                                       // entry whose data `fetch` takes next is cur_e - 1
    Row<DEGREE> row;
    int64_t row_idx = -1, idx_ahead = -1;
    float p_frac = 0.f, p_width = 1.f;
    bool p_ok = false;
    auto fetch = [&]() {
      --cur_e;
      p_ok = cur_e >= 0;
      if (p_ok) {
        if (idx_ahead != row_idx) { row = load_row<DEGREE>(coeffs, sc, n_intervals, idx_ahead, Cr); row_idx = idx_ahead; }
        p_frac = stage_frac[cur_e];
        if (DEGREE == CDE_PATH_LINEAR) p_width = knots[idx_ahead + 1] - knots[idx_ahead];
      }
      if (cur_e >= 1) idx_ahead = stage_index[cur_e - 1];
    };
    auto publish = [&](int which) {
      if (!p_ok) return;
      float dX[MC];
      control_slope<DEGREE>(row, p_frac, p_width, dX);
      const f32x2 d0 = half ? f32x2{dX[4], dX[5]} : f32x2{dX[0], dX[1]}, d1 = half ? f32x2{dX[6], dX[7]} : f32x2{dX[2], dX[3]};
      *reinterpret_cast<float4*>(ring_dx + which * 256 + n * 8 + 4 * half) = make_float4(d0[0], d0[1], d1[0], d1[1]);
    };
    if (n_stages > 0) idx_ahead = stage_index[n_stages - 1];
    fetch(); publish(0);
    fetch(); publish(1);
    fetch();
    __syncthreads();
    int par = 0, rs = 0;
    for (int64_t st = 0; st < n_stages; ++st) {
      kp_stage_barrier();
      // dL/dW of stage st first (its ring slot is rs), THEN stage st + 2's derivative into slot (st + 2) % 3 -- one ring
      // serves the chain wave and this wave, so the slot this stage reads must not be the one written: (st + 2) % 3 != st % 3
      publish(rs >= 1 ? rs - 1 : 2);
      fetch();
      const float* base = tile_lds + par * KP_ZA_FLOATS;
      const float4* zt4 = reinterpret_cast<const float4*>(base + (half * 32 + n) * 20);
      const float4* at4 = reinterpret_cast<const float4*>(base + 64 * 20 + (half * 32 + n) * 20);
      const float4* dw4 = reinterpret_cast<const float4*>(ring_dx + rs * 256 + half * 8);
      float4 zq = zt4[0], aq = at4[0], e0 = dw4[0], e1 = dw4[1];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const int i = s2 & 3;
        const f32x2 e01 = {e0.x, e0.y}, e23 = {e0.z, e0.w}, e45 = {e1.x, e1.y}, e67 = {e1.z, e1.w};
        const f32x2 asrc = i < 2 ? f32x2{aq.x, aq.y} : f32x2{aq.z, aq.w};
        const float zb = i == 0 ? zq.x : i == 1 ? zq.y : i == 2 ? zq.z : zq.w;
        f32x2 v01, v23, v45, v67;
        if (i & 1) {
          v01 = pk_mul_hi(e01, asrc); v23 = pk_mul_hi(e23, asrc); v45 = pk_mul_hi(e45, asrc); v67 = pk_mul_hi(e67, asrc);
          pk_fma_hi(gbp[0], e01, asrc); pk_fma_hi(gbp[1], e23, asrc); pk_fma_hi(gbp[2], e45, asrc); pk_fma_hi(gbp[3], e67, asrc);
        } else {
          v01 = pk_mul_lo(e01, asrc); v23 = pk_mul_lo(e23, asrc); v45 = pk_mul_lo(e45, asrc); v67 = pk_mul_lo(e67, asrc);
          pk_fma_lo(gbp[0], e01, asrc); pk_fma_lo(gbp[1], e23, asrc); pk_fma_lo(gbp[2], e45, asrc); pk_fma_lo(gbp[3], e67, asrc);
        }
        if (s2 < 15) {
          e0 = dw4[(s2 + 1) * 4]; e1 = dw4[(s2 + 1) * 4 + 1];
          if (i == 3) { zq = zt4[(s2 + 1) >> 2]; aq = at4[(s2 + 1) >> 2]; }
        }
        __builtin_amdgcn_sched_barrier(0);
        accW[0] = mfma(v01[0], zb, accW[0]); accW[1] = mfma(v01[1], zb, accW[1]);
        accW[2] = mfma(v23[0], zb, accW[2]); accW[3] = mfma(v23[1], zb, accW[3]);
        accW[4] = mfma(v45[0], zb, accW[4]); accW[5] = mfma(v45[1], zb, accW[5]);
        accW[6] = mfma(v67[0], zb, accW[6]); accW[7] = mfma(v67[1], zb, accW[7]);
        __builtin_amdgcn_sched_barrier(0);
      }
      par ^= 1;
      rs = rs == 2 ? 0 : rs + 1;
    }
    if (live) {
      float* my_partial = partial + tile * KP_PARTIAL_FLOATS;
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
    return;
  }

  // -------------------------------------------------------------------------------------------- chain wave
  __builtin_amdgcn_s_setprio(3);
  auto add_outputs = [&](int64_t m, f32x16& g) {
    for (int64_t e = node_ptr[m]; e < node_ptr[m + 1]; ++e) {
      const int64_t j = node_out[e];
      const float wgt = node_weight[e];
      if (valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int u = 2 * r + half;
          if (u < Hr) g[r] = __builtin_fmaf(wgt, grad_out[(sc * n_out + j) * Hr + u], g[r]);
        }
      }
    }
  };
  f32x16 gy;
#pragma unroll
  for (int r = 0; r < 16; ++r) gy[r] = 0.f;
  add_outputs(n_steps, gy);
  const float* srow = stages + (sc * n_steps * 4) * 32 + half * 16;
  auto load_state = [&](int64_t e) {
    f32x16 v16;
    const float4* sp = reinterpret_cast<const float4*>(srow + e * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = sp[i];
      v16[4 * i] = v.x; v16[4 * i + 1] = v.y; v16[4 * i + 2] = v.z; v16[4 * i + 3] = v.w;
    }
    return v16;
  };
  f32x16 snext = gy;
  if (n_steps > 0) snext = load_state(4 * n_steps - 1);
  __syncthreads();
  int par = 0, rs = 0;
  for (int64_t k = n_steps - 1; k >= 0; --k) {
    const float dt = step_dt[k];
    const float third = (float)(1.0 / 3.0);
    const float c8 = dt * 0.125f, dt3 = dt * third;
    f32x16 kb1 = gy * c8, kb2 = gy * (3.f * c8), kb3 = kb2, kbc = kb1;
    f32x16 yb = gy;
#pragma unroll
    for (int stage = 3; stage >= 0; --stage) {
      const f32x16 sst = snext;
      const int64_t e_next = 4 * k + stage - 1;
      if (e_next >= 0) snext = load_state(e_next);
      float bs0, bs1, bs2, bs3;
      {
        const float4 dA = *reinterpret_cast<const float4*>(ring_dx + rs * 256 + n * 8);
        const float4 dB = *reinterpret_cast<const float4*>(ring_dx + rs * 256 + n * 8 + 4);
        bs0 = half ? dA.y : dA.x; bs1 = half ? dA.w : dA.z; bs2 = half ? dB.y : dB.x; bs3 = half ? dB.w : dB.z;
        float* base = tile_lds + par * KP_ZA_FLOATS;
        float* wz = base + ((n & 1) * 32 + half) * 20 + (n >> 1);
        float* wa = base + 64 * 20 + ((n & 1) * 32 + half) * 20 + (n >> 1);
#pragma unroll
        for (int r = 0; r < 16; ++r) { wz[r * 40] = sst[r]; wa[r * 40] = kbc[r]; }
        kp_stage_barrier();
        par ^= 1;
        rs = rs == 2 ? 0 : rs + 1;
      }
      f32x16 v;
      {
        f32x2 v2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v2[j] = f32x2{0.f, 0.f};
        int opaque = 0;
        asm volatile("" : "+v"(opaque));
        const float4* wp = wj + lane + opaque;
        auto issue = [&](f32x16& J, const float4& a) {
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("s_nop 1\n\t"
                       "v_mfma_f32_32x32x2_f32 %0, %1, %5, 0\n\t"
                       "v_mfma_f32_32x32x2_f32 %0, %2, %6, %0\n\t"
                       "v_mfma_f32_32x32x2_f32 %0, %3, %7, %0\n\t"
                       "v_mfma_f32_32x32x2_f32 %0, %4, %8, %0"
                       : "=&v"(J) : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(bs0), "v"(bs1), "v"(bs2), "v"(bs3));
          __builtin_amdgcn_sched_barrier(0);
        };
        auto consume = [&](const f32x16& J, float ah) {
          const f32x2 ah2 = {ah, ah};
#pragma unroll
          for (int j = 0; j < 8; ++j) v2[j] = __builtin_elementwise_fma(f32x2{J[2 * j], J[2 * j + 1]}, ah2, v2[j]);
#pragma unroll
          for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(v2[j]));
        };
        f32x16 Je, Jo;
        float4 a_cur = wp[0], a_nxt = wp[64];
        issue(Je, a_cur);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r < 15) a_cur = wp[(2 * r + 2) * 64];
          issue(Jo, a_nxt);
          asm volatile("" : "+v"(Je));
          float ae = kbc[r], ao = kbc[r];
          kp_swap32(ae, ao);
          consume(Je, ae);
          if (r < 15) {
            a_nxt = wp[(2 * r + 3) * 64];
            issue(Je, a_cur);
            asm volatile("" : "+v"(Jo));
          } else {
            asm volatile("s_nop 15\n\ts_nop 7" : "+v"(Jo));
          }
          consume(Jo, ao);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = v2[r >> 1][r & 1];
      }
      yb = yb + v;
      if (stage == 3) {
        kb1 = kb1 + dt * v;
        kb2 = kb2 - dt * v;
        kb3 = kb3 + dt * v;
        kbc = kb3;
      } else if (stage == 2) {
        kb2 = kb2 + dt * v;
        kb1 = kb1 - dt3 * v;
        kbc = kb2;
      } else if (stage == 1) {
        kb1 = kb1 + dt3 * v;
        kbc = kb1;
      }
    }
    gy = yb;
    add_outputs(k, gy);
  }
  if (valid) {
#pragma unroll
    for (int r = 0; r < 16; ++r) if (2 * r + half < Hr) grad_z0[series * Hr + 2 * r + half] = gy[r];
  }
}

}  // namespace

// K3d's pair form (identity activation); CDE_K3D_WAVES=1 keeps the one-wave kernel of rk4_backprop.hip
int launch_backprop_jacobian_pair(const Control& x, const AffineField& f, const BackpropIO& io, const Shape& n,
                                  const StageTable& st, float* partial, hipStream_t s) {
  const Dims dims{(int)n.H, (int)n.C};
  const unsigned blocks = (unsigned)((n.B + 127) / 128);
  const size_t lds = (size_t)KP_LDS_FLOATS * sizeof(float);
  int rc = dispatch_degree(x.degree, [&](auto D) {
    allow_lds(rk4_backprop_jacobian_pair<D()>, lds);
    rk4_backprop_jacobian_pair<D()><<<blocks, 512, lds, s>>>(
        f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(io.stages), f32(io.grad_out), io.n_out, io.step_dt,
        io.n_steps, io.node_ptr, io.node_out, io.node_weight, f32(io.grad_z0), partial, n.B, st.index, f32(st.frac), dims);
    return CDE_OK;
  });
  if (rc == CDE_OK) rc = check_launch();
  if (rc != CDE_OK) return rc;
  return launch_reduce_partials(partial, (n.B + 31) / 32, io.grad_W, io.grad_b, (int)n.H, (int)n.C, s);
}

template <typename TT>
int launch_adjoint_jacobian_pair(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n,
                                 const StageTable& st, float* partial, hipStream_t s, PairForm form) {
  const Dims dims{(int)n.H, (int)n.C};
  const unsigned blocks = (unsigned)((n.B + 127) / 128);
  const bool bx = form.rows == PairRows::bf16;
  const size_t lds = (size_t)(bx ? KP_LDS_FLOATS_BX : KP_LDS_FLOATS) * sizeof(float);
  // bit 0: priority 3 for the chain waves, bit 1: for the helper waves (the trace build reads CDE_K3P_FLAGS once: experiments)
#ifdef CDE_PHASE_TRACE
  static const int flags = [] { const char* e = getenv("CDE_K3P_FLAGS"); return e ? atoi(e) : 1; }();
#else
  constexpr int flags = 1;
#endif
  if (bx && form.method != CDE_METHOD_RK4) return CDE_ERR_UNSUPPORTED;
  int rc = dispatch_degree(x.degree, [&](auto D) -> int {
    auto launch = [&](auto M, auto X) {
      allow_lds(rk4_adjoint_jacobian_pair<TT, D(), M(), X()>, lds);
      rk4_adjoint_jacobian_pair<TT, D(), M(), X()><<<blocks, 512, lds, s>>>(
          f32(x.coeffs), f32(x.knots), x.n_intervals, f32(f.W), f32(f.bias), f32(io.z_saved), f32(io.grad_out),
          (const TT*)io.sgrid, io.seg_off, io.n_out, f32(io.grad_z0), partial, n.B, st.index, f32(st.frac), dims, flags);
      return CDE_OK;
    };
    if (bx) return launch(Const<CDE_METHOD_RK4>{}, std::true_type{});           // (the bf16 rows: rk4 only)
    if (form.method == CDE_METHOD_RK4) return launch(Const<CDE_METHOD_RK4>{}, std::false_type{});
    if (form.method == CDE_METHOD_MIDPOINT) return launch(Const<CDE_METHOD_MIDPOINT>{}, std::false_type{});
    if (form.method == CDE_METHOD_EULER) return launch(Const<CDE_METHOD_EULER>{}, std::false_type{});
    return CDE_ERR_UNSUPPORTED;
  });
  if (rc == CDE_OK) rc = check_launch();
  if (rc != CDE_OK) return rc;
  return launch_reduce_partials(partial, (n.B + 31) / 32, io.grad_W, io.grad_b, (int)n.H, (int)n.C, s);
}
template int launch_adjoint_jacobian_pair<float>(const Control&, const AffineField&, const AdjointIO&, const Shape&, const StageTable&, float*, hipStream_t, PairForm);
template int launch_adjoint_jacobian_pair<double>(const Control&, const AffineField&, const AdjointIO&, const Shape&, const StageTable&, float*, hipStream_t, PairForm);

}  // namespace cde
