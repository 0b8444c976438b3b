// api.hip -- C-ABI entry points of the fused solvers: argument checks, stage table, kernel dispatch.
// Every entry point checks its arguments, names each pointer once in the structs of cde_launch.h and hands those on.
#include "cde_common.h"
#include "cde_launch.h"
#include "cde_mlp3.h"
#include "cde_mlp_tiled.h"
#include "cde_mlp_broad.h"

namespace cde {

static bool bf16x3_applicable(int64_t C, int64_t H, int dtype, int act) {
  return dtype == CDE_F32 && act == CDE_ACT_NONE && H >= 1 && H <= 32 && C >= 1 && C <= 8;
}
// AUTO takes the bf16x3 kernels (K2b forward, K3p's bf16 form backward) for the headline field on the wave-per-tile
// batches: float32, identity activation, H <= 32, C <= 8, more than CDE_SPLIT_MAX_BATCH series, no control gradients.
// variant = "mfma" keeps the exact-f32 kernels.
static bool auto_bf16x3(int variant, int64_t B, int64_t C, int64_t H, int dtype, int act) {
  return variant == CDE_VARIANT_AUTO && B > CDE_SPLIT_MAX_BATCH && bf16x3_applicable(C, H, dtype, act);
}

// Stage table: for solver step k over [grid[k], grid[k+1]] and RK stage j, the control interval
// and fractional part at the stage time -- what CubicSpline._interpret_t (interpolation_cubic.py:
// 315-322) returns when torchdiffeq's rk4 evaluates the vector field there.  One lane per entry.
// `negate`: the reverse sweep integrates in s = -t and evaluates the field at t = -s.
// `method` (CDE_METHOD_*): rk4's 3/8-rule times; midpoint: t0, t0 + 0.5 dt (torchdiffeq's `half_dt = 0.5 * dt`); euler: t0.
// The table keeps four slots per step whatever the method (unused slots repeat t0).
template <typename T, typename TT>
__global__ void stage_table_kernel(const T* __restrict__ knots, int64_t n_intervals, const TT* __restrict__ grid,
                                   int64_t n_steps, int negate, int64_t* __restrict__ index_out,
                                   T* __restrict__ frac_out, int method) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 4 * n_steps) return;
  const int64_t k = e >> 2;
  const StageClock<TT> clk(grid[k], grid[k + 1]);
  const int stage = (int)(e & 3);
  TT tt = clk.time(stage);
  if (method == CDE_METHOD_MIDPOINT) tt = stage == 1 ? clk.t0 + (TT)0.5 * clk.dt : clk.t0;
  else if (method == CDE_METHOD_EULER) tt = clk.t0;
  T ts = (T)tt;
  if (negate) ts = -ts;
  T frac;
  index_out[e] = locate(knots, n_intervals, ts, frac);
  frac_out[e] = frac;
}

// Node table of the reversible Heun solves (revheun.hip): the control interval and fractional part at every GRID NODE --
// the method evaluates the field at grid points only -- one slot per node, by the same `locate` as the stage table.
template <typename T, typename TT>
__global__ void node_table_kernel(const T* __restrict__ knots, int64_t n_intervals, const TT* __restrict__ grid,
                                  int64_t n_grid, int64_t* __restrict__ index_out, T* __restrict__ frac_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_grid) return;
  T frac;
  index_out[e] = locate(knots, n_intervals, (T)grid[e], frac);
  frac_out[e] = frac;
}

// A solve's stage table and what follows it in one allocation: [index: 4 n_steps int64 | frac: 4 n_steps elem | tail],
// every part 256-byte aligned.  `n_grid` grid points are n_grid - 1 steps (none for an empty grid).
struct StageBuffers {
  int64_t* index; void* frac;
  operator StageTable() const { return StageTable{index, frac}; }
};
struct StageWorkspace {
  int64_t n_steps; size_t elem;
  StageWorkspace(int64_t n_grid, size_t elem_bytes) : n_steps(n_grid > 1 ? n_grid - 1 : 0), elem(elem_bytes) {}
  size_t frac_offset() const { return align256((size_t)(4 * n_steps) * sizeof(int64_t)); }
  size_t tail_offset() const { return frac_offset() + align256((size_t)(4 * n_steps) * elem); }
  size_t total(size_t tail_bytes) const { return tail_offset() + tail_bytes; }
  StageBuffers table(const void* ws) const { return StageBuffers{(int64_t*)ws, (unsigned char*)ws + frac_offset()}; }
  void* tail(const void* ws) const { return (unsigned char*)ws + tail_offset(); }
};
struct Dtypes { int state, time; };

template <typename T, typename TT>
static int fill_stage_table(const Control& x, const void* grid, int64_t n_steps, int negate, int method, StageBuffers to,
                            hipStream_t s) {
  if (n_steps <= 0) return CDE_OK;
  stage_table_kernel<T, TT><<<(unsigned)((4 * n_steps + 255) / 256), 256, 0, s>>>(
      (const T*)x.knots, x.n_intervals, (const TT*)grid, n_steps, negate, to.index, (T*)to.frac, method);
  return check_launch();
}

// The state and time dtypes as types together: `f(Type<T>{}, Type<TT>{})`
template <typename F>
static int with_types(Dtypes d, F&& f) {
  return dispatch_dtype(d.state, [&](auto t) { return dispatch_dtype(d.time, [&](auto tt) -> int { return f(t, tt); }); });
}

// The forward direction of every solver: the stage table of `io.grid` into the caller's buffers, then `launch(T, TT)`.
template <typename F>
static int forward_solve(Dtypes d, const Control& x, const ForwardIO& io, int method, StageBuffers to, hipStream_t s,
                         F&& launch) {
  return with_types(d, [&](auto t, auto tt) -> int {
    using T = typename decltype(t)::type;
    using TT = typename decltype(tt)::type;
    const int rc = fill_stage_table<T, TT>(x, io.grid, io.n_grid - 1, 0, method, to, s);
    return rc != CDE_OK ? rc : launch(t, tt);
  });
}

// Do the MFMA kernels (rk4_mfma.hip and its relatives) take the solve?  `unsupported`: the variant asks for them and the
// shape does not fit, or the variant is unknown.
enum class Mfma { no, yes, unsupported };
static Mfma pick_mfma(int variant, int64_t C, int64_t H, int dtype, int act) {
  const bool ok = mfma_applicable(C, H, dtype, act);
  if (variant == CDE_VARIANT_MFMA || variant == CDE_VARIANT_SPLIT) return ok ? Mfma::yes : Mfma::unsupported;
  if (variant == CDE_VARIANT_GENERIC) return Mfma::no;
  if (variant != CDE_VARIANT_AUTO) return Mfma::unsupported;
  return ok ? Mfma::yes : Mfma::no;
}

// Among the MFMA kernels: the one-wave-per-series-tile kernels (K2/K3) need B/16 (B/32) waves to fill 1024 SIMDs twice
// (once); below CDE_SPLIT_MAX_BATCH series the workgroup-per-tile kernels of rk4_split.hip finish sooner.
// The tanh field is VALU-co-limited in the one-wave-per-tile kernels (K3a: 46 % MFMA-busy); the 8-wave tile kernel
// overlaps the activation work of its chain waves with the helper waves' dW products and wins at EVERY batch size
// (32768 series, forward + adjoint: 12.9 ms against 15.0 ms).
static bool pick_split(int variant, int64_t B, bool control_grad, int act = CDE_ACT_NONE) {
  if (control_grad) return false;                  // dL/dcoeffs lives in the pre-activation K3 kernel only
  if (variant == CDE_VARIANT_SPLIT) return true;
  return variant == CDE_VARIANT_AUTO && (B <= CDE_SPLIT_MAX_BATCH || act == CDE_ACT_TANH);
}

// Shapes beyond the 32 x 8 tiles (H <= 64, C <= 8 or H <= 32, C <= 16): the wide tile kernels under AUTO
static bool pick_wide(int variant, int64_t C, int64_t H, int dtype, int act) {
  return variant == CDE_VARIANT_AUTO && !mfma_applicable(C, H, dtype, act) && wide_applicable(C, H, dtype, act);
}

// Controls of 17 .. 64 channels on H <= 32 (rk4_affine_tiled.hip): the tiled kernels K2c / K3c under AUTO
static bool pick_affine_tiled(int variant, int64_t C, int64_t H, int dtype, int act) {
  return variant == CDE_VARIANT_AUTO && !mfma_applicable(C, H, dtype, act) && !wide_applicable(C, H, dtype, act) &&
         affine_tiled_applicable(C, H, dtype, act);
}
// ... whose backward pass reserves the larger of its own and the generic kernels' need (cde_rk4_adjoint_workspace_bytes
// answers before it knows the activation)
static size_t affine_tiled_reserve(int64_t B, int64_t C, int64_t H, int64_t n_steps, size_t elem) {
  const size_t a = affine_tiled_adjoint_workspace_bytes(B, C, H, n_steps), b = generic_adjoint_workspace_bytes(B, C, H, elem);
  return a > b ? a : b;
}

template <typename T, typename TT>
static int forward_typed(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, int dtype, int variant,
                         const StageTable& st, hipStream_t s) {
  if (variant == CDE_VARIANT_BF16X3 || auto_bf16x3(variant, n.B, n.C, n.H, dtype, f.act)) {
    if (!bf16x3_applicable(n.C, n.H, dtype, f.act)) return CDE_ERR_UNSUPPORTED;
    if (option(CDE_OPT_K2B_GROUPS) == 1) return launch_forward_bf16x3<TT>(x, f, io, n, st, s);      // K2b, for A/B timing
    return launch_forward_bf16x3_duo<TT>(x, f, io, n, st, s);
  }
  const Mfma mfma = pick_mfma(variant, n.C, n.H, dtype, f.act);
  if (mfma == Mfma::unsupported) return CDE_ERR_UNSUPPORTED;
  if (mfma == Mfma::yes && pick_split(variant, n.B, false, f.act)) return launch_forward_split<TT>(x, f, io, n, st, s);
  if (mfma == Mfma::yes) return launch_forward_mfma<TT>(x, f, io, n, st, s);
  if (pick_wide(variant, n.C, n.H, dtype, f.act)) return launch_forward_wide<TT>(x, f, io, n, st, s);
  if (pick_affine_tiled(variant, n.C, n.H, dtype, f.act)) return launch_forward_affine_tiled<TT>(x, f, io, n, st, s);
  return launch_forward_generic<T, TT>(x, f, io, n, st, s);
}

// workspace: [stage_index: 4*(n_sgrid-1) int64][stage_frac: 4*(n_sgrid-1) T][partials]
template <typename T, typename TT>
static int adjoint_typed(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, int dtype, int variant,
                         Workspace ws, hipStream_t s) {
  const bool bx = variant == CDE_VARIANT_BF16X3 || (auto_bf16x3(variant, n.B, n.C, n.H, dtype, f.act) && !io.grad_coeffs);
  bool use_split = false, use_mfma = true, use_wide = false, use_tiled = false;
  if (bx) {
    if (!bf16x3_applicable(n.C, n.H, dtype, f.act) || io.grad_coeffs) return CDE_ERR_UNSUPPORTED;
  } else {
    const Mfma mfma = pick_mfma(variant, n.C, n.H, dtype, f.act);
    if (mfma == Mfma::unsupported) return CDE_ERR_UNSUPPORTED;
    use_mfma = mfma == Mfma::yes;
    if (io.grad_coeffs && !use_mfma) return CDE_ERR_UNSUPPORTED;      // control gradients: MFMA kernels only
    use_split = use_mfma && pick_split(variant, n.B, io.grad_coeffs != nullptr, f.act);
    if (variant == CDE_VARIANT_SPLIT && !use_split) return CDE_ERR_UNSUPPORTED;
    use_wide = !use_mfma && pick_wide(variant, n.C, n.H, dtype, f.act);
    use_tiled = !use_mfma && !use_wide && pick_affine_tiled(variant, n.C, n.H, dtype, f.act);
  }
  const StageWorkspace layout(io.n_sgrid, sizeof(T));
  const size_t part_bytes = use_split ? split_adjoint_partial_bytes(n.B)
                            : use_mfma ? mfma_adjoint_partial_bytes(n.B)
                            : use_wide ? wide_adjoint_workspace_bytes(n.B, n.C, n.H, io.n_sgrid - 1)
                            : use_tiled ? affine_tiled_reserve(n.B, n.C, n.H, layout.n_steps, sizeof(T))
                                       : generic_adjoint_workspace_bytes(n.B, n.C, n.H, sizeof(T));
  if (ws.bytes < layout.total(part_bytes)) return CDE_ERR_WORKSPACE;
  const StageBuffers st = layout.table(ws.base);
  void* partial = layout.tail(ws.base);
  const int rc = fill_stage_table<T, TT>(x, io.sgrid, io.n_sgrid - 1, 1, CDE_METHOD_RK4, st, s);
  if (rc != CDE_OK) return rc;
  if (bx) {
    // the reverse sweep: K3p with its J rows on the bf16 pipe (rk4_adjoint_pair.hip); CDE_OPT_K3_WAVES = 1 keeps the
    // one-wave form K3bj (rk4_mfma.hip, bitwise the same results), CDE_OPT_K3_FORM = 1 K3b (three GEMMs, two of them on the
    // bf16 pipe)
    if (option(CDE_OPT_K3_FORM) == 1) return launch_adjoint_bf16x3<TT>(x, f, io, n, st, (float*)partial, s);
    if (option(CDE_OPT_K3_WAVES) == 1) return launch_adjoint_jacobian_bx<TT>(x, f, io, n, st, (float*)partial, s);
    return launch_adjoint_jacobian_pair<TT>(x, f, io, n, st, (float*)partial, s, PairForm{CDE_METHOD_RK4, PairRows::bf16});
  }
  if (use_split) return launch_adjoint_split<TT>(x, f, io, n, st, (float*)partial, s);
  if (use_mfma) return launch_adjoint_mfma<TT>(x, f, io, n, st, (float*)partial, s);
  if (use_wide) return launch_adjoint_wide<TT>(x, f, io, n, st, partial, s);
  if (use_tiled) return launch_adjoint_affine_tiled<TT>(x, f, io, n, st, partial, s);
  return launch_adjoint_generic<T, TT>(x, f, io, n, st, partial, s);
}

}  // namespace cde

using namespace cde;

// which arithmetic an rk4 solve of the affine field takes (1: the bf16x3 kernels, 0: the exact-f32 / other kernels) --
// the rule of forward_typed / adjoint_typed, for the host's dispatch record
extern "C" int cde_rk4_bf16x3_form(int64_t B, int64_t C, int64_t H, int dtype, int act, int variant) {
  if (variant == CDE_VARIANT_BF16X3) return bf16x3_applicable(C, H, dtype, act) ? 1 : 0;
  return auto_bf16x3(variant, B, C, H, dtype, act) ? 1 : 0;
}

extern "C" int cde_rk4_supported(int64_t C, int64_t H, int dtype, int act, int adjoint, int variant) {
  if (C < 1 || H < 1 || (dtype != CDE_F32 && dtype != CDE_F64)) return 0;
  if (act != CDE_ACT_NONE && act != CDE_ACT_TANH) return 0;
  if (variant == CDE_VARIANT_BF16X3) return bf16x3_applicable(C, H, dtype, act) ? 1 : 0;
  const Mfma mfma = pick_mfma(variant, C, H, dtype, act);
  if (mfma != Mfma::no) return mfma == Mfma::yes ? 1 : 0;
  if (pick_wide(variant, C, H, dtype, act)) return 1;
  if (pick_affine_tiled(variant, C, H, dtype, act)) return 1;
  return generic_applicable(C, H, dtype == CDE_F64 ? 8 : 4, adjoint != 0) ? 1 : 0;
}

// the rule of pick_affine_tiled under CDE_VARIANT_AUTO, for the host's dispatch record
extern "C" int cde_rk4_affine_tiled_supported(int64_t C, int64_t H, int dtype, int act) {
  return pick_affine_tiled(CDE_VARIANT_AUTO, C, H, dtype, act) ? 1 : 0;
}

extern "C" int cde_rk4_forward_linear(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                      const void* W, const void* bias, int act, const void* z0, const void* grid,
                                      int64_t n_grid, const void* t_out, int64_t n_out, void* z_out, int64_t B,
                                      int64_t C, int64_t H, int dtype, int time_dtype, int variant,
                                      int64_t* stage_index, void* stage_frac, void* stream) {
  if (B < 0 || C < 1 || H < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (act != CDE_ACT_NONE && act != CDE_ACT_TANH) return CDE_ERR_UNSUPPORTED;
  if (B == 0) return CDE_OK;
  if (!coeffs || !knots || !W || !bias || !z0 || !grid || !t_out || !z_out) return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac)) return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const AffineField f{W, bias, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, nullptr};
  const Shape n{B, C, H};
  const StageBuffers st{stage_index, stage_frac};
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(Dtypes{dtype, time_dtype}, x, io, CDE_METHOD_RK4, st, s, [&](auto t, auto tt) {
    return forward_typed<typename decltype(t)::type, typename decltype(tt)::type>(x, f, io, n, dtype, variant, st, s);
  });
}

extern "C" int cde_rk4_forward_mlp(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                   const void* W1, const void* bias1, int64_t width, const void* W2, const void* bias2,
                                   int act, const void* z0, const void* grid, int64_t n_grid, const void* t_out,
                                   int64_t n_out, void* z_out, int64_t B, int64_t C, int64_t H, int dtype,
                                   int time_dtype, int64_t* stage_index, void* stage_frac, void* stream) {
  if (B < 0 || C < 1 || H < 1 || width < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!field_act_known(act)) return CDE_ERR_UNSUPPORTED;
  if (B == 0) return CDE_OK;
  if (!coeffs || !knots || !W1 || !bias1 || !W2 || !bias2 || !z0 || !grid || !t_out || !z_out) return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac)) return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const TwoLayerField f{W1, bias1, width, W2, bias2, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, nullptr};
  const Shape n{B, C, H};
  const StageBuffers st{stage_index, stage_frac};
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(Dtypes{dtype, time_dtype}, x, io, CDE_METHOD_RK4, st, s, [&](auto, auto tt) {
    return launch_forward_mlp<typename decltype(tt)::type>(x, f, io, n, st, s);
  });
}

extern "C" size_t cde_rk4_adjoint_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t n_sgrid, int dtype,
                                                  int variant) {
  const size_t elem = dtype == CDE_F64 ? 8 : 4;
  const StageWorkspace layout(n_sgrid, elem);
  if (variant == CDE_VARIANT_BF16X3) return layout.total(mfma_adjoint_partial_bytes(B));
  const bool use_mfma = pick_mfma(variant, C, H, dtype, CDE_ACT_NONE) == Mfma::yes;
  // AUTO may resolve to either kernel depending on the activation: reserve the larger need
  size_t a = mfma_adjoint_partial_bytes(B);
  if (variant != CDE_VARIANT_MFMA && variant != CDE_VARIANT_GENERIC) {    // AUTO may resolve to the tile kernels (tanh: at any B)
    const size_t sp = split_adjoint_partial_bytes(B);
    a = sp > a ? sp : a;
  }
  size_t b = generic_adjoint_workspace_bytes(B, C, H, elem);
  if (!use_mfma && (pick_wide(variant, C, H, dtype, CDE_ACT_NONE))) {
    const size_t wb = wide_adjoint_workspace_bytes(B, C, H, layout.n_steps);
    b = wb > b ? wb : b;
  }
  if (!use_mfma && pick_affine_tiled(variant, C, H, dtype, CDE_ACT_NONE)) b = affine_tiled_reserve(B, C, H, layout.n_steps, elem);
  if (variant == CDE_VARIANT_MFMA || variant == CDE_VARIANT_SPLIT) return layout.total(a);
  if (variant == CDE_VARIANT_GENERIC || !use_mfma) return layout.total(b);
  return layout.total(a > b ? a : b);
}

static int adjoint_linear_impl(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, Dtypes d,
                               int variant, Workspace ws, void* stream) {
  if (n.B < 1 || n.C < 1 || n.H < 1 || x.n_intervals < 1 || io.n_out < 1 || io.n_sgrid < 0) return CDE_ERR_SHAPE;
  if (f.act != CDE_ACT_NONE && f.act != CDE_ACT_TANH) return CDE_ERR_UNSUPPORTED;
  if (!x.coeffs || !x.knots || !f.W || !f.bias || !io.z_saved || !io.grad_out || !io.grad_z0 || !io.grad_W || !io.grad_b ||
      !ws.base)
    return CDE_ERR_NULL;
  if (io.n_out > 1 && (!io.sgrid || !io.seg_off)) return CDE_ERR_NULL;
  return with_types(d, [&](auto t, auto tt) {
    return adjoint_typed<typename decltype(t)::type, typename decltype(tt)::type>(x, f, io, n, d.state, variant, ws,
                                                                                  (hipStream_t)stream);
  });
}

extern "C" int cde_rk4_adjoint_linear(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                      const void* W, const void* bias, int act, const void* z_saved,
                                      const void* grad_out, const void* sgrid, int64_t n_sgrid, const int64_t* seg_off,
                                      const int64_t* seg_off_host, int64_t n_out, void* grad_z0, void* grad_W,
                                      void* grad_b, int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                      int variant, void* workspace, size_t workspace_bytes, void* stream) {
  return adjoint_linear_impl(Control{coeffs, knots, n_intervals, degree}, AffineField{W, bias, act},
                             AdjointIO{z_saved, grad_out, sgrid, n_sgrid, seg_off, seg_off_host, n_out, grad_z0, grad_W,
                                       grad_b, nullptr},
                             Shape{B, C, H}, Dtypes{dtype, time_dtype}, variant, Workspace{workspace, workspace_bytes}, stream);
}

extern "C" int cde_rk4_adjoint_linear_dcontrol(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                               const void* W, const void* bias, int act, const void* z_saved,
                                               const void* grad_out, const void* sgrid, int64_t n_sgrid,
                                               const int64_t* seg_off, int64_t n_out, void* grad_z0, void* grad_W,
                                               void* grad_b, void* grad_coeffs, int64_t B, int64_t C, int64_t H,
                                               int dtype, int time_dtype, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  if (!grad_coeffs) return CDE_ERR_NULL;
  return adjoint_linear_impl(Control{coeffs, knots, n_intervals, degree}, AffineField{W, bias, act},
                             AdjointIO{z_saved, grad_out, sgrid, n_sgrid, seg_off, nullptr, n_out, grad_z0, grad_W, grad_b,
                                       grad_coeffs},
                             Shape{B, C, H}, Dtypes{dtype, time_dtype}, CDE_VARIANT_MFMA, Workspace{workspace, workspace_bytes},
                             stream);
}

// ---------------------------------------------------------------------------------------------- midpoint / euler
extern "C" int cde_fixed_supported(int method, int64_t C, int64_t H, int dtype, int act) {
  if (method != CDE_METHOD_MIDPOINT && method != CDE_METHOD_EULER) return 0;
  return (dtype == CDE_F32 && act == CDE_ACT_NONE && mfma_applicable(C, H, dtype, act)) ? 1 : 0;
}

extern "C" int cde_fixed_forward_linear(int method, const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                        const void* W, const void* bias, const void* z0, const void* grid, int64_t n_grid,
                                        const void* t_out, int64_t n_out, void* z_out, int64_t B, int64_t C, int64_t H,
                                        int dtype, int time_dtype, int64_t* stage_index, void* stage_frac, void* stream) {
  if (B < 0 || C < 1 || H < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!cde_fixed_supported(method, C, H, dtype, CDE_ACT_NONE)) return CDE_ERR_UNSUPPORTED;
  if (B == 0) return CDE_OK;
  if (!coeffs || !knots || !W || !bias || !z0 || !grid || !t_out || !z_out) return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac)) return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const AffineField f{W, bias, CDE_ACT_NONE};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, nullptr};
  const Shape n{B, C, H};
  const StageBuffers st{stage_index, stage_frac};
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(Dtypes{dtype, time_dtype}, x, io, method, st, s, [&](auto, auto tt) {
    return launch_forward_mfma_method<typename decltype(tt)::type>(method, x, f, io, n, st, s);
  });
}

// workspace: [stage_index: 4*(n_sgrid-1) int64][stage_frac: 4*(n_sgrid-1) f32][per-wave partial parameter gradients]
extern "C" size_t cde_fixed_adjoint_workspace_bytes(int64_t B, int64_t n_sgrid) {
  return StageWorkspace(n_sgrid, sizeof(float)).total(B > 0 ? mfma_adjoint_partial_bytes(B) : 0);
}

extern "C" int cde_fixed_adjoint_linear(int method, const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                        const void* W, const void* bias, const void* z_saved, const void* grad_out,
                                        const void* sgrid, int64_t n_sgrid, const int64_t* seg_off, int64_t n_out,
                                        void* grad_z0, void* grad_W, void* grad_b, int64_t B, int64_t C, int64_t H, int dtype,
                                        int time_dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || C < 1 || H < 1 || n_intervals < 1 || n_out < 1 || n_sgrid < 0) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!cde_fixed_supported(method, C, H, dtype, CDE_ACT_NONE)) return CDE_ERR_UNSUPPORTED;
  if (!coeffs || !knots || !W || !bias || !z_saved || !grad_out || !grad_z0 || !grad_W || !grad_b || !workspace)
    return CDE_ERR_NULL;
  if (n_out > 1 && (!sgrid || !seg_off)) return CDE_ERR_NULL;
  if (workspace_bytes < cde_fixed_adjoint_workspace_bytes(B, n_sgrid)) return CDE_ERR_WORKSPACE;
  const Control x{coeffs, knots, n_intervals, degree};
  const AffineField f{W, bias, CDE_ACT_NONE};
  const AdjointIO io{z_saved, grad_out, sgrid, n_sgrid, seg_off, nullptr, n_out, grad_z0, grad_W, grad_b, nullptr};
  const Shape n{B, C, H};
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const StageBuffers st = layout.table(workspace);
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(time_dtype, [&](auto tt) -> int {
    using TT = typename decltype(tt)::type;
    const int rc = fill_stage_table<float, TT>(x, sgrid, layout.n_steps, 1, method, st, s);
    if (rc != CDE_OK) return rc;
    return launch_adjoint_jacobian_pair<TT>(x, f, io, n, st, (float*)layout.tail(workspace), s, PairForm{method, PairRows::f32});
  });
}

// ---------------------------------------------------------------------------------------------- reversible Heun
// node table [index: n_grid int64 | frac: n_grid f32], then the per-wave partial parameter gradients
namespace cde {
struct NodeWorkspace {
  int64_t n_grid;
  explicit NodeWorkspace(int64_t n) : n_grid(n > 0 ? n : 0) {}
  size_t frac_offset() const { return align256((size_t)n_grid * sizeof(int64_t)); }
  size_t tail_offset() const { return frac_offset() + align256((size_t)n_grid * sizeof(float)); }
  StageBuffers table(const void* ws) const { return StageBuffers{(int64_t*)ws, (unsigned char*)ws + frac_offset()}; }
  void* tail(const void* ws) const { return (unsigned char*)ws + tail_offset(); }
};
template <typename TT>
static int fill_node_table(const Control& x, const void* grid, int64_t n_grid, StageBuffers to, hipStream_t s) {
  node_table_kernel<float, TT><<<(unsigned)((n_grid + 255) / 256), 256, 0, s>>>(f32(x.knots), x.n_intervals, (const TT*)grid,
                                                                                n_grid, to.index, f32(to.frac));
  return check_launch();
}
}  // namespace cde

extern "C" int cde_revheun_supported(int64_t C, int64_t H, int dtype, int act) {
  return revheun_applicable(C, H, dtype, act) ? 1 : 0;
}

extern "C" int cde_revheun_forward_linear(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                          const void* W, const void* bias, int act, const void* z0, const void* grid,
                                          int64_t n_grid, const void* t_out, int64_t n_out, void* z_out, void* zhat_out,
                                          int64_t B, int64_t C, int64_t H, int dtype, int time_dtype, int64_t* node_index,
                                          void* node_frac, void* stream) {
  if (B < 0 || C < 1 || H < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if ((dtype != CDE_F32 && dtype != CDE_F64) || (time_dtype != CDE_F32 && time_dtype != CDE_F64)) return CDE_ERR_DTYPE;
  if (B == 0) return CDE_OK;
  if (!cde_revheun_supported(C, H, dtype, act)) return CDE_ERR_UNSUPPORTED;
  if (degree != CDE_PATH_CUBIC && degree != CDE_PATH_LINEAR) return CDE_ERR_UNSUPPORTED;
  if (!coeffs || !knots || !W || !bias || !z0 || !grid || !t_out || !z_out || !zhat_out || !node_index || !node_frac)
    return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const AffineField f{W, bias, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, nullptr};
  const Shape n{B, C, H};
  const StageBuffers nodes{node_index, node_frac};
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(time_dtype, [&](auto tt) -> int {
    using TT = typename decltype(tt)::type;
    const int rc = fill_node_table<TT>(x, grid, n_grid, nodes, s);
    return rc != CDE_OK ? rc : launch_revheun_forward<TT>(x, f, io, zhat_out, n, nodes, s);
  });
}

extern "C" size_t cde_revheun_adjoint_workspace_bytes(int64_t B, int64_t n_grid) {
  return NodeWorkspace(n_grid).tail_offset() + (B > 0 ? mfma_adjoint_partial_bytes(B) : 0);
}

extern "C" int cde_revheun_adjoint_linear(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                          const void* W, const void* bias, int act, const void* y_final,
                                          const void* zhat_final, const void* grad_out, const void* grid, int64_t n_grid,
                                          const int64_t* node_ptr, const int64_t* node_out, const float* node_weight,
                                          int64_t n_out, void* grad_z0, void* grad_W, void* grad_b, int64_t B, int64_t C,
                                          int64_t H, int dtype, int time_dtype, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (B < 1 || C < 1 || H < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if ((dtype != CDE_F32 && dtype != CDE_F64) || (time_dtype != CDE_F32 && time_dtype != CDE_F64)) return CDE_ERR_DTYPE;
  if (!cde_revheun_supported(C, H, dtype, act)) return CDE_ERR_UNSUPPORTED;
  if (degree != CDE_PATH_CUBIC && degree != CDE_PATH_LINEAR) return CDE_ERR_UNSUPPORTED;
  if (!coeffs || !knots || !W || !bias || !y_final || !zhat_final || !grad_out || !grid || !node_ptr || !node_out ||
      !node_weight || !grad_z0 || !grad_W || !grad_b || !workspace)
    return CDE_ERR_NULL;
  if (workspace_bytes < cde_revheun_adjoint_workspace_bytes(B, n_grid)) return CDE_ERR_WORKSPACE;
  const Control x{coeffs, knots, n_intervals, degree};
  const AffineField f{W, bias, act};
  const ReversibleIO io{y_final, zhat_final, grad_out, grid, n_grid, node_ptr, node_out, node_weight, n_out,
                        grad_z0, grad_W, grad_b};
  const Shape n{B, C, H};
  const NodeWorkspace layout(n_grid);
  const StageBuffers nodes = layout.table(workspace);
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtype(time_dtype, [&](auto tt) -> int {
    using TT = typename decltype(tt)::type;
    const int rc = fill_node_table<TT>(x, grid, n_grid, nodes, s);
    return rc != CDE_OK ? rc : launch_revheun_adjoint<TT>(x, f, io, n, nodes, (float*)layout.tail(workspace), s);
  });
}

// ---------------------------------------------------------------------------------------------- K3d (adjoint=False)
extern "C" int cde_rk4_backprop_supported(int64_t C, int64_t H, int dtype, int act) {
  return (dtype == CDE_F32 && (act == CDE_ACT_NONE || act == CDE_ACT_TANH) && mfma_applicable(C, H, dtype, act)) ? 1 : 0;
}

extern "C" int cde_rk4_forward_linear_stages(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                             const void* W, const void* bias, int act, const void* z0, const void* grid,
                                             int64_t n_grid, const void* t_out, int64_t n_out, void* z_out, void* stages,
                                             int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                             int64_t* stage_index, void* stage_frac, void* stream) {
  if (B < 0 || C < 1 || H < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!cde_rk4_backprop_supported(C, H, dtype, act)) return CDE_ERR_UNSUPPORTED;
  if (B == 0) return CDE_OK;
  if (!coeffs || !knots || !W || !bias || !z0 || !grid || !t_out || !z_out) return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac || !stages)) return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const AffineField f{W, bias, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, stages};
  const Shape n{B, C, H};
  const StageBuffers st{stage_index, stage_frac};
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(Dtypes{dtype, time_dtype}, x, io, CDE_METHOD_RK4, st, s, [&](auto, auto tt) {
    return launch_forward_mfma_stages<typename decltype(tt)::type>(x, f, io, n, st, s);
  });
}

extern "C" size_t cde_rk4_backprop_workspace_bytes(int64_t B) { return B > 0 ? backprop_workspace_bytes(B) : 0; }

static int rk4_backprop_linear_impl(const Control& x, const AffineField& f, const BackpropIO& io, const Shape& n, int dtype,
                                    const StageTable& st, Workspace ws, void* stream) {
  if (n.B < 1 || n.C < 1 || n.H < 1 || x.n_intervals < 1 || io.n_out < 1 || io.n_steps < 0) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!cde_rk4_backprop_supported(n.C, n.H, dtype, f.act)) return CDE_ERR_UNSUPPORTED;
  if (!x.coeffs || !x.knots || !f.W || !f.bias || !io.grad_out || !io.node_ptr || !io.node_out || !io.node_weight ||
      !io.grad_z0 || !io.grad_W || !io.grad_b || !ws.base)
    return CDE_ERR_NULL;
  if (io.n_steps > 0 && (!io.stages || !io.step_dt || !st.index || !st.frac)) return CDE_ERR_NULL;
  if (ws.bytes < cde_rk4_backprop_workspace_bytes(n.B)) return CDE_ERR_WORKSPACE;
  return launch_backprop_jacobian(x, f, io, n, st, (float*)ws.base, (hipStream_t)stream);
}

extern "C" int cde_rk4_backprop_linear(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                       const void* W, const void* bias, int act, const void* stages, const void* grad_out,
                                       int64_t n_out,
                                       const float* step_dt, int64_t n_steps, const int64_t* node_ptr,
                                       const int64_t* node_out, const float* node_weight, void* grad_z0, void* grad_W,
                                       void* grad_b, int64_t B, int64_t C, int64_t H, int dtype,
                                       const int64_t* stage_index, const void* stage_frac, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return rk4_backprop_linear_impl(Control{coeffs, knots, n_intervals, degree}, AffineField{W, bias, act},
                                  BackpropIO{stages, grad_out, n_out, step_dt, n_steps, node_ptr, node_out, node_weight,
                                             grad_z0, grad_W, grad_b, nullptr},
                                  Shape{B, C, H}, dtype, StageTable{stage_index, stage_frac},
                                  Workspace{workspace, workspace_bytes}, stream);
}

// ... and with the gradient w.r.t. the control's coefficient tensor (`grad_coeffs`: layout of `coeffs`, ZEROED by the caller,
// accumulated): under adjoint=False autograd reaches the control through X.derivative at every stage.
extern "C" int cde_rk4_backprop_linear_dcontrol(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                                const void* W, const void* bias, int act, const void* stages,
                                                const void* grad_out, int64_t n_out, const float* step_dt, int64_t n_steps,
                                                const int64_t* node_ptr, const int64_t* node_out, const float* node_weight,
                                                void* grad_z0, void* grad_W, void* grad_b, void* grad_coeffs, int64_t B,
                                                int64_t C, int64_t H, int dtype, const int64_t* stage_index,
                                                const void* stage_frac, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  if (!grad_coeffs) return CDE_ERR_NULL;
  return rk4_backprop_linear_impl(Control{coeffs, knots, n_intervals, degree}, AffineField{W, bias, act},
                                  BackpropIO{stages, grad_out, n_out, step_dt, n_steps, node_ptr, node_out, node_weight,
                                             grad_z0, grad_W, grad_b, grad_coeffs},
                                  Shape{B, C, H}, dtype, StageTable{stage_index, stage_frac},
                                  Workspace{workspace, workspace_bytes}, stream);
}

// ---------------------------------------------------------------------------------------------- K3m
// workspace: [stage_index: 4*(n_sgrid-1) int64][stage_frac: 4*(n_sgrid-1) f32][weight images]
extern "C" size_t cde_rk4_adjoint_mlp_workspace_bytes(int64_t n_sgrid) {
  return StageWorkspace(n_sgrid, sizeof(float)).total(align256(mlp_adjoint_image_bytes()));
}

// the stage table of `grid` (`negate`: the reversed grid of the continuous adjoint) and the weight images, once per solve
static int mlp_prepare_impl(int negate, const Control& x, const void* grid, int64_t n_grid, const TwoLayerField& f,
                            const Shape& n, Dtypes d, Workspace ws, void* stream) {
  if (n.C < 1 || n.H < 1 || f.width < 1 || x.n_intervals < 1 || n_grid < 0) return CDE_ERR_SHAPE;
  if (d.state != CDE_F32) return d.state == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!mlp_shape_ok(n.C, n.H, f.width) && !mlp_shape_upper(n.C, n.H, f.width)) return CDE_ERR_UNSUPPORTED;
  if (!x.knots || !f.W1 || !f.bias1 || !f.W2 || !f.bias2 || !ws.base || (n_grid > 1 && !grid)) return CDE_ERR_NULL;
  if (ws.bytes < cde_rk4_adjoint_mlp_workspace_bytes(n_grid)) return CDE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const StageWorkspace layout(n_grid, sizeof(float));
  const int rc = dispatch_dtype(d.time, [&](auto tt) {
    return fill_stage_table<float, typename decltype(tt)::type>(x, grid, layout.n_steps, negate, CDE_METHOD_RK4,
                                                                layout.table(ws.base), s);
  });
  if (rc != CDE_OK) return rc;
  return launch_mlp_adjoint_images(f.W1, f.bias1, f.width, f.W2, f.bias2, n.C, n.H, (float*)layout.tail(ws.base), s);
}

extern "C" int cde_rk4_adjoint_mlp_prepare(const void* knots, int64_t n_intervals, const void* sgrid, int64_t n_sgrid,
                                           const void* W1, const void* bias1, int64_t width, const void* W2,
                                           const void* bias2, int64_t C, int64_t H, int dtype, int time_dtype,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return mlp_prepare_impl(1, Control{nullptr, knots, n_intervals, 0}, sgrid, n_sgrid,
                          TwoLayerField{W1, bias1, width, W2, bias2, CDE_ACT_NONE}, Shape{0, C, H}, Dtypes{dtype, time_dtype},
                          Workspace{workspace, workspace_bytes}, stream);
}

// ---------------------------------------------------------------------------------------------- K3m, reverse mode (adjoint=False)
extern "C" int cde_rk4_forward_mlp_stages(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                          const void* W1, const void* bias1, int64_t width, const void* W2,
                                          const void* bias2, int act, const void* z0, const void* grid, int64_t n_grid,
                                          const void* t_out, int64_t n_out, void* z_out, void* stages, int64_t B, int64_t C,
                                          int64_t H, int dtype, int time_dtype, int64_t* stage_index, void* stage_frac,
                                          void* stream) {
  if (B < 0 || C < 1 || H < 1 || width < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!field_act_known(act)) return CDE_ERR_UNSUPPORTED;
  if (B == 0) return CDE_OK;
  if (!coeffs || !knots || !W1 || !bias1 || !W2 || !bias2 || !z0 || !grid || !t_out || !z_out) return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac || !stages)) return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const TwoLayerField f{W1, bias1, width, W2, bias2, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, stages};
  const Shape n{B, C, H};
  const StageBuffers st{stage_index, stage_frac};
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(Dtypes{dtype, time_dtype}, x, io, CDE_METHOD_RK4, st, s, [&](auto, auto tt) {
    return launch_forward_mlp_stages<typename decltype(tt)::type>(x, f, io, n, st, s);
  });
}

extern "C" int cde_rk4_backprop_mlp_prepare(const void* knots, int64_t n_intervals, const void* grid, int64_t n_grid,
                                            const void* W1, const void* bias1, int64_t width, const void* W2,
                                            const void* bias2, int64_t C, int64_t H, int dtype, int time_dtype,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  return mlp_prepare_impl(0, Control{nullptr, knots, n_intervals, 0}, grid, n_grid,
                          TwoLayerField{W1, bias1, width, W2, bias2, CDE_ACT_NONE}, Shape{0, C, H}, Dtypes{dtype, time_dtype},
                          Workspace{workspace, workspace_bytes}, stream);
}

// One chunk of a two-layer sweep over the table and images its *_prepare call left in `ws`.  `io` arrives without its image;
// `backprop`: the reverse-mode sweep over the stored stages, else the continuous adjoint.
static int mlp_sweep_impl(bool backprop, const Control& x, SweepIO io, int64_t n_grid, const Shape& n, Dtypes d, Workspace ws,
                          void* stream) {
  if (n.B < 1 || n.C < 1 || n.H < 1 || x.n_intervals < 1 || io.k_begin < 0 || io.k_end < io.k_begin || io.k_end > n_grid - 1)
    return CDE_ERR_SHAPE;
  if (d.state != CDE_F32) return d.state == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!mlp_shape_ok(n.C, n.H, 1) && !mlp_shape_upper(n.C, n.H, 1)) return CDE_ERR_UNSUPPORTED;
  if (!field_act_known(io.act)) return CDE_ERR_UNSUPPORTED;
  if (!x.coeffs || !x.knots || !(backprop ? io.stages : io.y_state) || !io.a_state || !io.grid || !io.U || !io.G2 || !io.G1 ||
      !io.Z || !ws.base)
    return CDE_ERR_NULL;
  if (ws.bytes < cde_rk4_adjoint_mlp_workspace_bytes(n_grid)) return CDE_ERR_WORKSPACE;
  const StageWorkspace layout(n_grid, sizeof(float));
  const StageTable st = layout.table(ws.base);
  io.image = (const float*)layout.tail(ws.base);
  io.n_steps = n_grid - 1;
  return dispatch_dtype(d.time, [&](auto tt) {
    using TT = typename decltype(tt)::type;
    return backprop ? launch_mlp_backprop_sweep<TT>(x, io, n, st, (hipStream_t)stream)
                    : launch_mlp_adjoint_sweep<TT>(x, io, n, st, (hipStream_t)stream);
  });
}

extern "C" int cde_rk4_backprop_mlp_sweep(const void* coeffs, const void* knots, int64_t n_intervals, int degree, int act,
                                          const void* stages, void* g_state, const void* grid, int64_t n_grid,
                                          int64_t k_begin, int64_t k_end, void* U, void* G2, void* G1, void* Z, int64_t B,
                                          int64_t C, int64_t H, int dtype, int time_dtype, const void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return mlp_sweep_impl(true, Control{coeffs, knots, n_intervals, degree},
                        SweepIO{nullptr, act, nullptr, g_state, stages, 0, grid, k_begin, k_end, U, G2, G1, Z, nullptr}, n_grid,
                        Shape{B, C, H}, Dtypes{dtype, time_dtype}, Workspace{(void*)workspace, workspace_bytes}, stream);
}

// ... and with the gradient w.r.t. the control's coefficient tensor (`grad_coeffs` zeroed by the caller before the first chunk,
// accumulated by every chunk's launch)
extern "C" int cde_rk4_backprop_mlp_sweep_dcontrol(const void* coeffs, const void* knots, int64_t n_intervals, int degree,
                                                   int act, const void* stages, void* g_state, const void* grid,
                                                   int64_t n_grid, int64_t k_begin, int64_t k_end, void* U, void* G2, void* G1,
                                                   void* Z, void* grad_coeffs, int64_t B, int64_t C, int64_t H, int dtype,
                                                   int time_dtype, const void* workspace, size_t workspace_bytes,
                                                   void* stream) {
  if (!grad_coeffs) return CDE_ERR_NULL;
  return mlp_sweep_impl(true, Control{coeffs, knots, n_intervals, degree},
                        SweepIO{nullptr, act, nullptr, g_state, stages, 0, grid, k_begin, k_end, U, G2, G1, Z, grad_coeffs},
                        n_grid, Shape{B, C, H}, Dtypes{dtype, time_dtype}, Workspace{(void*)workspace, workspace_bytes}, stream);
}

extern "C" int cde_rk4_adjoint_mlp_sweep(const void* coeffs, const void* knots, int64_t n_intervals, int degree, int act,
                                         void* y_state, void* a_state, const void* sgrid, int64_t n_sgrid,
                                         int64_t k_begin, int64_t k_end, void* U, void* G2, void* G1, void* Z,
                                         void* grad_coeffs, int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                         const void* workspace, size_t workspace_bytes, void* stream) {
  return mlp_sweep_impl(false, Control{coeffs, knots, n_intervals, degree},
                        SweepIO{nullptr, act, y_state, a_state, nullptr, 0, sgrid, k_begin, k_end, U, G2, G1, Z, grad_coeffs},
                        n_sgrid, Shape{B, C, H}, Dtypes{dtype, time_dtype}, Workspace{(void*)workspace, workspace_bytes}, stream);
}

// ---------------------------------------------------------------------------------------------- K2m3 / K3m3 (three layers)
// argument checks in the siblings' order, all before the first HIP call: sizes, dtype, (forward) the empty batch, the
// envelope of rk4_mlp3.hip, pointers, workspace
static int mlp3_envelope(int64_t C, int64_t H, int64_t width1, int64_t width2, int dtype, int act, bool with_act) {
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  if (!mlp3_shape_ok(C, H, width1, width2)) return CDE_ERR_UNSUPPORTED;
  if (with_act && !field_act_known(act)) return CDE_ERR_UNSUPPORTED;
  return CDE_OK;
}

extern "C" int cde_rk4_forward_mlp3(const void* coeffs, const void* knots, int64_t n_intervals, int degree, const void* W1,
                                    const void* bias1, int64_t width1, const void* Wm, const void* biasm, int64_t width2,
                                    const void* W2, const void* bias2, int act, const void* z0, const void* grid,
                                    int64_t n_grid, const void* t_out, int64_t n_out, void* z_out, int64_t B, int64_t C,
                                    int64_t H, int dtype, int time_dtype, int64_t* stage_index, void* stage_frac,
                                    void* stream) {
  if (B < 0 || C < 1 || H < 1 || width1 < 1 || width2 < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32 && dtype != CDE_F64) return CDE_ERR_DTYPE;
  if (B == 0) return CDE_OK;
  const int rc = mlp3_envelope(C, H, width1, width2, dtype, act, true);
  if (rc != CDE_OK) return rc;
  if (!coeffs || !knots || !W1 || !bias1 || !Wm || !biasm || !W2 || !bias2 || !z0 || !grid || !t_out || !z_out)
    return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac)) return CDE_ERR_NULL;
  const Control x{coeffs, knots, n_intervals, degree};
  const ThreeLayerField f{W1, bias1, width1, Wm, biasm, width2, W2, bias2, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, nullptr};
  const Shape n{B, C, H};
  const StageBuffers st{stage_index, stage_frac};
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(Dtypes{dtype, time_dtype}, x, io, CDE_METHOD_RK4, st, s, [&](auto, auto tt) {
    return launch_forward_mlp3<typename decltype(tt)::type>(x, f, io, n, st, s);
  });
}

// workspace: [stage_index: 4*(n_sgrid-1) int64][stage_frac: 4*(n_sgrid-1) f32][weight images]
extern "C" size_t cde_rk4_adjoint_mlp3_workspace_bytes(int64_t n_sgrid) {
  return StageWorkspace(n_sgrid, sizeof(float)).total(align256(mlp3_adjoint_image_bytes()));
}

extern "C" int cde_rk4_adjoint_mlp3_prepare(const void* knots, int64_t n_intervals, const void* sgrid, int64_t n_sgrid,
                                            const void* W1, const void* bias1, int64_t width1, const void* Wm,
                                            const void* biasm, int64_t width2, const void* W2, const void* bias2, int64_t C,
                                            int64_t H, int dtype, int time_dtype, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  if (C < 1 || H < 1 || width1 < 1 || width2 < 1 || n_intervals < 1 || n_sgrid < 0) return CDE_ERR_SHAPE;
  const int rc = mlp3_envelope(C, H, width1, width2, dtype, 0, false);
  if (rc != CDE_OK) return rc;
  if (!knots || !W1 || !bias1 || !Wm || !biasm || !W2 || !bias2 || !workspace || (n_sgrid > 1 && !sgrid)) return CDE_ERR_NULL;
  if (workspace_bytes < cde_rk4_adjoint_mlp3_workspace_bytes(n_sgrid)) return CDE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Control x{nullptr, knots, n_intervals, 0};
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const int table = dispatch_dtype(time_dtype, [&](auto tt) {
    return fill_stage_table<float, typename decltype(tt)::type>(x, sgrid, layout.n_steps, 1, CDE_METHOD_RK4,
                                                                layout.table(workspace), s);
  });
  if (table != CDE_OK) return table;
  return launch_mlp3_adjoint_images(ThreeLayerField{W1, bias1, width1, Wm, biasm, width2, W2, bias2, CDE_ACT_NONE}, C, H,
                                    (float*)layout.tail(workspace), s);
}

extern "C" int cde_rk4_adjoint_mlp3_sweep(const void* coeffs, const void* knots, int64_t n_intervals, int degree, int act,
                                          void* y_state, void* a_state, const void* sgrid, int64_t n_sgrid, int64_t k_begin,
                                          int64_t k_end, void* U, void* U1, void* G2, void* Gm, void* G1, void* Z, int64_t B,
                                          int64_t C, int64_t H, int dtype, int time_dtype, const void* workspace,
                                          size_t workspace_bytes, void* stream) {
  if (B < 1 || C < 1 || H < 1 || n_intervals < 1 || k_begin < 0 || k_end < k_begin || k_end > n_sgrid - 1) return CDE_ERR_SHAPE;
  const int rc = mlp3_envelope(C, H, 1, 1, dtype, act, true);
  if (rc != CDE_OK) return rc;
  if (!coeffs || !knots || !y_state || !a_state || !sgrid || !U || !U1 || !G2 || !Gm || !G1 || !Z || !workspace)
    return CDE_ERR_NULL;
  if (workspace_bytes < cde_rk4_adjoint_mlp3_workspace_bytes(n_sgrid)) return CDE_ERR_WORKSPACE;
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const StageTable st = layout.table(workspace);
  const Control x{coeffs, knots, n_intervals, degree};
  const Sweep3IO io{(const float*)layout.tail(workspace), act, y_state, a_state, sgrid, k_begin, k_end, U, U1, G2, Gm, G1, Z};
  return dispatch_dtype(time_dtype, [&](auto tt) {
    return launch_mlp3_adjoint_sweep<typename decltype(tt)::type>(x, io, Shape{B, C, H}, st, (hipStream_t)stream);
  });
}

// ------------------------------------------------------ K2mc / K3mc (17 .. 64 channels), K2mh / K3mh (33 .. 64 hidden channels)
// One implementation over the state vectors per lane (rk4_mlp_tiled.hip: NV = 2 behind *_mlp_wide_*, NV = 4 behind
// *_mlp_tall_*).  Argument checks in the siblings' order, all before the first HIP call: sizes, dtype, (forward) the empty
// batch, the envelope of the form, pointers, workspace
template <int NV>
static int mlp_tiled_supported(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  return (dtype == CDE_F32 && field_act_known(act) && MlpTiled<NV>::shape_ok(C, H, width)) ? 1 : 0;
}

template <int NV>
static int mlp_tiled_envelope(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  return mlp_tiled_supported<NV>(C, H, width, dtype, act) ? CDE_OK : CDE_ERR_UNSUPPORTED;
}

template <int NV>
static int mlp_tiled_forward(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, Dtypes dt,
                             const StageBuffers& st, void* stream) {
  if (n.B < 0 || n.C < 1 || n.H < 1 || f.width < 1 || x.n_intervals < 1 || io.n_grid < 1 || io.n_out < 1) return CDE_ERR_SHAPE;
  if (dt.state != CDE_F32 && dt.state != CDE_F64) return CDE_ERR_DTYPE;
  if (n.B == 0) return CDE_OK;
  const int rc = mlp_tiled_envelope<NV>(n.C, n.H, f.width, dt.state, f.act);
  if (rc != CDE_OK) return rc;
  if (!x.coeffs || !x.knots || !f.W1 || !f.bias1 || !f.W2 || !f.bias2 || !io.z0 || !io.grid || !io.t_out || !io.z_out)
    return CDE_ERR_NULL;
  if (io.n_grid > 1 && (!st.index || !st.frac)) return CDE_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(dt, x, io, CDE_METHOD_RK4, st, s, [&](auto, auto tt) {
    return launch_forward_mlp_tiled<NV, typename decltype(tt)::type>(x, f, io, n, st, s);
  });
}

// workspace: [stage_index: 4*(n_sgrid-1) int64][stage_frac: 4*(n_sgrid-1) f32][layer-1 images and the padded output-layer copies]
template <int NV>
static size_t mlp_tiled_workspace_bytes(int64_t n_sgrid) {
  return StageWorkspace(n_sgrid, sizeof(float)).total(align256(mlp_tiled_adjoint_image_bytes<NV>()));
}

template <int NV>
static int mlp_tiled_prepare(const void* knots, int64_t n_intervals, const void* sgrid, int64_t n_sgrid, const TwoLayerField& f,
                             int64_t C, int64_t H, Dtypes dt, Workspace ws, void* stream) {
  if (C < 1 || H < 1 || f.width < 1 || n_intervals < 1 || n_sgrid < 0) return CDE_ERR_SHAPE;
  const int rc = mlp_tiled_envelope<NV>(C, H, f.width, dt.state, CDE_ACT_NONE);
  if (rc != CDE_OK) return rc;
  if (!knots || !f.W1 || !f.bias1 || !f.W2 || !f.bias2 || !ws.base || (n_sgrid > 1 && !sgrid)) return CDE_ERR_NULL;
  if (ws.bytes < mlp_tiled_workspace_bytes<NV>(n_sgrid)) return CDE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Control x{nullptr, knots, n_intervals, 0};
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const int table = dispatch_dtype(dt.time, [&](auto tt) {
    return fill_stage_table<float, typename decltype(tt)::type>(x, sgrid, layout.n_steps, 1, CDE_METHOD_RK4,
                                                                layout.table(ws.base), s);
  });
  if (table != CDE_OK) return table;
  return launch_mlp_tiled_adjoint_images<NV>(f, C, H, (float*)layout.tail(ws.base), s);
}

// `io.image` is filled in here; `io.Z_hi` is read by NV = 4 alone
template <int NV>
static int mlp_tiled_sweep(const Control& x, TiledSweepIO io, int64_t n_sgrid, const Shape& n, Dtypes dt, Workspace ws,
                           void* stream) {
  if (n.B < 1 || n.C < 1 || n.H < 1 || x.n_intervals < 1 || io.k_begin < 0 || io.k_end < io.k_begin || io.k_end > n_sgrid - 1)
    return CDE_ERR_SHAPE;
  const int rc = mlp_tiled_envelope<NV>(n.C, n.H, 1, dt.state, io.act);
  if (rc != CDE_OK) return rc;
  if (!x.coeffs || !x.knots || !io.y_state || !io.a_state || !io.grid || !io.U || !io.G2 || !io.G1 || !io.Z ||
      (NV == 4 && !io.Z_hi) || !ws.base)
    return CDE_ERR_NULL;
  if (ws.bytes < mlp_tiled_workspace_bytes<NV>(n_sgrid)) return CDE_ERR_WORKSPACE;
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const StageTable st = layout.table(ws.base);
  io.image = (const float*)layout.tail(ws.base);
  return dispatch_dtype(dt.time, [&](auto tt) {
    return launch_mlp_tiled_adjoint_sweep<NV, typename decltype(tt)::type>(x, io, n, st, (hipStream_t)stream);
  });
}

extern "C" int cde_rk4_mlp_wide_supported(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  return mlp_tiled_supported<2>(C, H, width, dtype, act);
}

extern "C" int cde_rk4_forward_mlp_wide(const void* coeffs, const void* knots, int64_t n_intervals, int degree, const void* W1,
                                        const void* bias1, int64_t width, const void* W2, const void* bias2, int act,
                                        const void* z0, const void* grid, int64_t n_grid, const void* t_out, int64_t n_out,
                                        void* z_out, int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                        int64_t* stage_index, void* stage_frac, void* stream) {
  return mlp_tiled_forward<2>(Control{coeffs, knots, n_intervals, degree}, TwoLayerField{W1, bias1, width, W2, bias2, act},
                              ForwardIO{z0, grid, n_grid, t_out, n_out, z_out, nullptr}, Shape{B, C, H},
                              Dtypes{dtype, time_dtype}, StageBuffers{stage_index, stage_frac}, stream);
}

extern "C" size_t cde_rk4_adjoint_mlp_wide_workspace_bytes(int64_t n_sgrid) { return mlp_tiled_workspace_bytes<2>(n_sgrid); }

extern "C" int cde_rk4_adjoint_mlp_wide_prepare(const void* knots, int64_t n_intervals, const void* sgrid, int64_t n_sgrid,
                                                const void* W1, const void* bias1, int64_t width, const void* W2,
                                                const void* bias2, int64_t C, int64_t H, int dtype, int time_dtype,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  return mlp_tiled_prepare<2>(knots, n_intervals, sgrid, n_sgrid, TwoLayerField{W1, bias1, width, W2, bias2, CDE_ACT_NONE}, C, H,
                              Dtypes{dtype, time_dtype}, Workspace{workspace, workspace_bytes}, stream);
}

extern "C" int cde_rk4_adjoint_mlp_wide_sweep(const void* coeffs, const void* knots, int64_t n_intervals, int degree, int act,
                                              void* y_state, void* a_state, const void* sgrid, int64_t n_sgrid,
                                              int64_t k_begin, int64_t k_end, void* U, void* G2, void* G1, void* Z, int64_t B,
                                              int64_t C, int64_t H, int dtype, int time_dtype, const void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return mlp_tiled_sweep<2>(Control{coeffs, knots, n_intervals, degree},
                            TiledSweepIO{nullptr, act, y_state, a_state, sgrid, k_begin, k_end, U, G2, G1, Z, nullptr}, n_sgrid,
                            Shape{B, C, H}, Dtypes{dtype, time_dtype}, Workspace{(void*)workspace, workspace_bytes}, stream);
}

extern "C" int cde_rk4_mlp_tall_supported(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  return mlp_tiled_supported<4>(C, H, width, dtype, act);
}

extern "C" int cde_rk4_forward_mlp_tall(const void* coeffs, const void* knots, int64_t n_intervals, int degree, const void* W1,
                                        const void* bias1, int64_t width, const void* W2, const void* bias2, int act,
                                        const void* z0, const void* grid, int64_t n_grid, const void* t_out, int64_t n_out,
                                        void* z_out, int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                        int64_t* stage_index, void* stage_frac, void* stream) {
  return mlp_tiled_forward<4>(Control{coeffs, knots, n_intervals, degree}, TwoLayerField{W1, bias1, width, W2, bias2, act},
                              ForwardIO{z0, grid, n_grid, t_out, n_out, z_out, nullptr}, Shape{B, C, H},
                              Dtypes{dtype, time_dtype}, StageBuffers{stage_index, stage_frac}, stream);
}

extern "C" size_t cde_rk4_adjoint_mlp_tall_workspace_bytes(int64_t n_sgrid) { return mlp_tiled_workspace_bytes<4>(n_sgrid); }

extern "C" int cde_rk4_adjoint_mlp_tall_prepare(const void* knots, int64_t n_intervals, const void* sgrid, int64_t n_sgrid,
                                                const void* W1, const void* bias1, int64_t width, const void* W2,
                                                const void* bias2, int64_t C, int64_t H, int dtype, int time_dtype,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  return mlp_tiled_prepare<4>(knots, n_intervals, sgrid, n_sgrid, TwoLayerField{W1, bias1, width, W2, bias2, CDE_ACT_NONE}, C, H,
                              Dtypes{dtype, time_dtype}, Workspace{workspace, workspace_bytes}, stream);
}

extern "C" int cde_rk4_adjoint_mlp_tall_sweep(const void* coeffs, const void* knots, int64_t n_intervals, int degree, int act,
                                              void* y_state, void* a_state, const void* sgrid, int64_t n_sgrid,
                                              int64_t k_begin, int64_t k_end, void* U, void* G2, void* G1, void* Z, void* Z_hi,
                                              int64_t B, int64_t C, int64_t H, int dtype, int time_dtype, const void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return mlp_tiled_sweep<4>(Control{coeffs, knots, n_intervals, degree},
                            TiledSweepIO{nullptr, act, y_state, a_state, sgrid, k_begin, k_end, U, G2, G1, Z, Z_hi}, n_sgrid,
                            Shape{B, C, H}, Dtypes{dtype, time_dtype}, Workspace{(void*)workspace, workspace_bytes}, stream);
}

// ------------------------------------------------------ K2mb / K3mb (inner layer of 129 .. 256 units; rk4_mlp_broad.hip)
// Argument checks in the order of *_mlp_wide_*, all before the first HIP call: sizes, dtype, (forward) the empty batch, the
// envelope, pointers, workspace.  The sweep is not told the width: it checks the rest of the envelope at the widest.
static int mlp_broad_supported(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  return (dtype == CDE_F32 && field_act_known(act) && mlp_broad_shape_ok(C, H, width)) ? 1 : 0;
}

static int mlp_broad_envelope(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  if (dtype != CDE_F32) return dtype == CDE_F64 ? CDE_ERR_UNSUPPORTED : CDE_ERR_DTYPE;
  return mlp_broad_supported(C, H, width, dtype, act) ? CDE_OK : CDE_ERR_UNSUPPORTED;
}

// workspace: [stage_index: 4*(n_sgrid-1) int64][stage_frac: 4*(n_sgrid-1) f32][layer-1 images and the padded output-layer copies]
static size_t mlp_broad_workspace_bytes(int64_t n_sgrid) {
  return StageWorkspace(n_sgrid, sizeof(float)).total(align256(mlp_broad_adjoint_image_bytes()));
}

extern "C" int cde_rk4_mlp_broad_supported(int64_t C, int64_t H, int64_t width, int dtype, int act) {
  return mlp_broad_supported(C, H, width, dtype, act);
}

extern "C" int cde_rk4_forward_mlp_broad(const void* coeffs, const void* knots, int64_t n_intervals, int degree, const void* W1,
                                         const void* bias1, int64_t width, const void* W2, const void* bias2, int act,
                                         const void* z0, const void* grid, int64_t n_grid, const void* t_out, int64_t n_out,
                                         void* z_out, int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                         int64_t* stage_index, void* stage_frac, void* stream) {
  const Control x{coeffs, knots, n_intervals, degree};
  const TwoLayerField f{W1, bias1, width, W2, bias2, act};
  const ForwardIO io{z0, grid, n_grid, t_out, n_out, z_out, nullptr};
  const Shape n{B, C, H};
  const Dtypes dt{dtype, time_dtype};
  const StageBuffers st{stage_index, stage_frac};
  if (B < 0 || C < 1 || H < 1 || width < 1 || n_intervals < 1 || n_grid < 1 || n_out < 1) return CDE_ERR_SHAPE;
  if (dtype != CDE_F32 && dtype != CDE_F64) return CDE_ERR_DTYPE;
  if (B == 0) return CDE_OK;
  const int rc = mlp_broad_envelope(C, H, width, dtype, act);
  if (rc != CDE_OK) return rc;
  if (!coeffs || !knots || !W1 || !bias1 || !W2 || !bias2 || !z0 || !grid || !t_out || !z_out) return CDE_ERR_NULL;
  if (n_grid > 1 && (!stage_index || !stage_frac)) return CDE_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  return forward_solve(dt, x, io, CDE_METHOD_RK4, st, s, [&](auto, auto tt) {
    return launch_forward_mlp_broad<typename decltype(tt)::type>(x, f, io, n, st, s);
  });
}

extern "C" size_t cde_rk4_adjoint_mlp_broad_workspace_bytes(int64_t n_sgrid) { return mlp_broad_workspace_bytes(n_sgrid); }

extern "C" int cde_rk4_adjoint_mlp_broad_prepare(const void* knots, int64_t n_intervals, const void* sgrid, int64_t n_sgrid,
                                                 const void* W1, const void* bias1, int64_t width, const void* W2,
                                                 const void* bias2, int64_t C, int64_t H, int dtype, int time_dtype,
                                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (C < 1 || H < 1 || width < 1 || n_intervals < 1 || n_sgrid < 0) return CDE_ERR_SHAPE;
  const int rc = mlp_broad_envelope(C, H, width, dtype, CDE_ACT_NONE);
  if (rc != CDE_OK) return rc;
  if (!knots || !W1 || !bias1 || !W2 || !bias2 || !workspace || (n_sgrid > 1 && !sgrid)) return CDE_ERR_NULL;
  if (workspace_bytes < mlp_broad_workspace_bytes(n_sgrid)) return CDE_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Control x{nullptr, knots, n_intervals, 0};
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const int table = dispatch_dtype(time_dtype, [&](auto tt) {
    return fill_stage_table<float, typename decltype(tt)::type>(x, sgrid, layout.n_steps, 1, CDE_METHOD_RK4,
                                                                layout.table(workspace), s);
  });
  if (table != CDE_OK) return table;
  return launch_mlp_broad_adjoint_images(TwoLayerField{W1, bias1, width, W2, bias2, CDE_ACT_NONE}, C, H,
                                         (float*)layout.tail(workspace), s);
}

extern "C" int cde_rk4_adjoint_mlp_broad_sweep(const void* coeffs, const void* knots, int64_t n_intervals, int degree, int act,
                                               void* y_state, void* a_state, const void* sgrid, int64_t n_sgrid,
                                               int64_t k_begin, int64_t k_end, void* U_lo, void* U_hi, void* G2, void* G1_lo,
                                               void* G1_hi, void* Z, int64_t B, int64_t C, int64_t H, int dtype, int time_dtype,
                                               const void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 1 || C < 1 || H < 1 || n_intervals < 1 || k_begin < 0 || k_end < k_begin || k_end > n_sgrid - 1) return CDE_ERR_SHAPE;
  const int rc = mlp_broad_envelope(C, H, BR_WIDTH, dtype, act);
  if (rc != CDE_OK) return rc;
  if (!coeffs || !knots || !y_state || !a_state || !sgrid || !U_lo || !U_hi || !G2 || !G1_lo || !G1_hi || !Z || !workspace)
    return CDE_ERR_NULL;
  if (workspace_bytes < mlp_broad_workspace_bytes(n_sgrid)) return CDE_ERR_WORKSPACE;
  const StageWorkspace layout(n_sgrid, sizeof(float));
  const StageTable st = layout.table((void*)workspace);
  const Control x{coeffs, knots, n_intervals, degree};
  const BroadSweepIO io{(const float*)layout.tail((void*)workspace), act, y_state, a_state, sgrid, k_begin, k_end,
                        U_lo, U_hi, G2, G1_lo, G1_hi, Z};
  return dispatch_dtype(time_dtype, [&](auto tt) {
    return launch_mlp_broad_adjoint_sweep<typename decltype(tt)::type>(x, io, Shape{B, C, H}, st, (hipStream_t)stream);
  });
}
