// cde_launch.h -- host side of the fused solvers: the argument structs the launchers take, the prototype of every launcher
// and helper that crosses a translation unit, the degree / activation dispatch and the adaptive families' launch loop.
// Host code only: declarations, and the two templates that touch the runtime for the kernel they are handed (allow_lds,
// launch_attempts -- the latter holds a <<<>>> launch, so only .hip files include this header).  Fixed grid (rk4 / midpoint / euler): api.hip fills the structs where the C ABI's pointers enter,
// the rk4_*.hip files define the launchers.  Adaptive (dopri5): the entry points of the dopri5*.hip files fill them.
// Interpolation, fills, log-signature windows (interp_kernels.hip, logsig_kernels.hip): the dtype dispatch and the small
// things their entry points share.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cde_mi355x.h"

namespace cde {

// ---------------------------------------------------------------- what always travels together
struct Control { const void* coeffs; const void* knots; int64_t n_intervals; int degree; };
struct AffineField { const void* W; const void* bias; int act; };
struct TwoLayerField { const void* W1; const void* bias1; int64_t width; const void* W2; const void* bias2; int act; };
struct Shape { int64_t B, C, H; };
// control interval and fractional part at every stage time (api.hip: stage_table_kernel), four slots per step
struct StageTable { const int64_t* index; const void* frac; };
// `stages`: where the kernels of adjoint=False store their stage states (null otherwise)
struct ForwardIO { const void* z0; const void* grid; int64_t n_grid; const void* t_out; int64_t n_out; void* z_out; void* stages; };
// `seg_off_host`: the host copy of `seg_off` (the wide kernels' chunk loop); `grad_coeffs`: null without control gradients
struct AdjointIO {
  const void* z_saved; const void* grad_out; const void* sgrid; int64_t n_sgrid;
  const int64_t* seg_off; const int64_t* seg_off_host; int64_t n_out;
  void* grad_z0; void* grad_W; void* grad_b; void* grad_coeffs;
};
// reverse mode through the stored stage states of the affine field (adjoint=False)
struct BackpropIO {
  const void* stages; const void* grad_out; int64_t n_out;
  const float* step_dt; int64_t n_steps; const int64_t* node_ptr; const int64_t* node_out; const float* node_weight;
  void* grad_z0; void* grad_W; void* grad_b; void* grad_coeffs;
};
// the reconstructing backward pass of the reversible Heun method (revheun.hip): the final (y, zh) of the forward solve, the
// forward grid, and the output gradients as BackpropIO's node lists
struct ReversibleIO {
  const void* y_final; const void* zhat_final; const void* grad_out; const void* grid; int64_t n_grid;
  const int64_t* node_ptr; const int64_t* node_out; const float* node_weight; int64_t n_out;
  void* grad_z0; void* grad_W; void* grad_b;
};
// steps [k_begin, k_end) of a two-layer sweep.  Continuous adjoint: `y_state`, `a_state` over `grid` = the reversed grid;
// reverse mode: `a_state` alone (the running gradient) over the forward grid, with the `stages` of all `n_steps` steps.
struct SweepIO {
  const float* image; int act;
  void* y_state; void* a_state; const void* stages; int64_t n_steps;
  const void* grid; int64_t k_begin, k_end;
  void* U; void* G2; void* G1; void* Z; void* grad_coeffs;
};
struct Workspace { void* base; size_t bytes; };
static inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }        // every part of a workspace starts on one
// K3p's form: the solver's stage count and whether the J rows run on the bf16 pipe (rk4 only)
enum class PairRows { f32, bf16 };
struct PairForm { int method; PairRows rows; };

static inline const float* f32(const void* p) { return (const float*)p; }
static inline float* f32(void* p) { return (float*)p; }

// ---------------------------------------------------------------- the adaptive protocol (dopri5*.hip)
struct StepControl { double rtol, atol, safety, ifactor, dfactor; };
struct Jumps { const double* t; int64_t n; };                  // ascending; the adjoint solves: in reversed time
struct DopriIO { const void* z0; const double* t_out; int64_t n_out; void* z_out; };
// one output interval [s0, s1] of a backward pass, in reversed time
struct AdjInterval { const void* y_init; const void* a_init; double s0, s1; void* a_out; int first_interval, norm_kind; };
// a call queues launches [first, first + n) of its solve; launch i works on controller block i & 1 (`parity`)
struct LaunchWindow { int64_t first, n; };
// one step controller for a batch sharded over GPUs: the pending sums added up over all shards, the global batch size
struct Sharding {
  const double* reduced_sums; int64_t B_global;
  bool on() const { return reduced_sums != nullptr || B_global > 0; }
};
// adjoint_params naming the control: `coeffs` null without control gradients, `knots` null without the knot-time block
struct ControlGrads { void* coeffs; int64_t numel; void* knots; };

// ---------------------------------------------------------------- degree / activation as compile-time constants
// `f(std::integral_constant<int, V>{})` for the run-time value; CDE_ERR_UNSUPPORTED for any other.  `f` launches and
// returns a code, so each launcher names its kernel's arguments once.
template <int V> using Const = std::integral_constant<int, V>;
template <typename F>
int dispatch_degree(int degree, F&& f) {
  if (degree == CDE_PATH_CUBIC) return f(Const<CDE_PATH_CUBIC>{});
  if (degree == CDE_PATH_LINEAR) return f(Const<CDE_PATH_LINEAR>{});
  return CDE_ERR_UNSUPPORTED;
}
template <typename F>
int dispatch_act(int act, F&& f) {
  if (act == CDE_ACT_NONE) return f(Const<CDE_ACT_NONE>{});
  if (act == CDE_ACT_TANH) return f(Const<CDE_ACT_TANH>{});
  return CDE_ERR_UNSUPPORTED;
}
template <typename F>
int dispatch_degree_act(int degree, int act, F&& f) {
  return dispatch_degree(degree, [&](auto D) { return dispatch_act(act, [&](auto A) { return f(D, A); }); });
}
// the two-layer fields: `act` = CDE_FIELD_ACT(final, hidden), handed to the kernels whole (cde_mfma.h: final_tanh, hidden_softplus)
constexpr int FIELD_SOFTPLUS_NONE = CDE_FIELD_ACT(CDE_ACT_NONE, CDE_HIDDEN_SOFTPLUS);
constexpr int FIELD_SOFTPLUS_TANH = CDE_FIELD_ACT(CDE_ACT_TANH, CDE_HIDDEN_SOFTPLUS);
static inline bool field_act_known(int act) {
  return (act & ~0xff) == 0 && (CDE_FIELD_FINAL(act) == CDE_ACT_NONE || CDE_FIELD_FINAL(act) == CDE_ACT_TANH) &&
         (CDE_FIELD_HIDDEN(act) == CDE_HIDDEN_RELU || CDE_FIELD_HIDDEN(act) == CDE_HIDDEN_SOFTPLUS);
}
template <typename F>
int dispatch_degree_field(int degree, int act, F&& f) {
  if (!field_act_known(act)) return CDE_ERR_UNSUPPORTED;
  return dispatch_degree(degree, [&](auto D) -> int {
    if (CDE_FIELD_HIDDEN(act) == CDE_HIDDEN_RELU) return dispatch_act(act, [&](auto A) { return f(D, A); });
    if (act == FIELD_SOFTPLUS_NONE) return f(D, Const<FIELD_SOFTPLUS_NONE>{});
    return f(D, Const<FIELD_SOFTPLUS_TANH>{});
  });
}
// a dtype code as a type: `f(Type<float>{})` / `f(Type<double>{})` (`using T = typename decltype(tag)::type;`),
// CDE_ERR_DTYPE for anything else
template <typename T> struct Type { using type = T; };
template <typename F>
int dispatch_dtype(int dtype, F&& f) {
  if (dtype == CDE_F32) return f(Type<float>{});
  if (dtype == CDE_F64) return f(Type<double>{});
  return CDE_ERR_DTYPE;
}
// `kernel`'s dynamic LDS limit, raised to what the launch asks for
template <typename K>
void allow_lds(K kernel, size_t bytes) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// Waves (16-series tiles) per workgroup of the one-wave-per-tile kernels (rk4_mlp3.hip, rk4_mlp_tiled.hip).  Their LDS images
// allow one workgroup per CU, and there is one tile form only, so a small batch is spread over the 256 CUs first: one wave
// per workgroup up to 256 tiles, then two, .. up to `most`.
static inline unsigned waves_per_workgroup(int64_t tiles, unsigned most) {
  const int64_t per_cu = (tiles + 255) / 256;
  return per_cu < 1 ? 1u : per_cu > most ? most : (unsigned)per_cu;
}
// the launch loop of every adaptive family: per launch of the window the attempt kernel on its parity, then `after(parity)`
// (the kernels that digest what the attempt left); a code other than CDE_OK from `after` ends the loop
template <typename K, typename Args, typename After>
int launch_attempts(K kernel, unsigned grid, unsigned block, size_t lds, hipStream_t s, const Args& g, LaunchWindow w,
                    After&& after) {
  for (int64_t i = 0; i < w.n; ++i) {
    const int parity = (int)((w.first + i) & 1);
    kernel<<<grid, block, lds, s>>>(g, parity);
    const int rc = after(parity);
    if (rc != CDE_OK) return rc;
  }
  return CDE_OK;
}

// ---------------------------------------------------------------- interp_kernels.hip, logsig_kernels.hip (f32 / f64)
template <typename F>
int dispatch_what(int what, F&& f) {
  if (what == CDE_EVAL_DERIVATIVE) return f(Const<CDE_EVAL_DERIVATIVE>{});
  if (what == CDE_EVAL_VALUE) return f(Const<CDE_EVAL_VALUE>{});
  return CDE_ERR_UNSUPPORTED;
}
template <typename F>
int dispatch_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
// a batch of series (B, L, C); `ok`: the size check of every entry point that takes one (the fills accept L = 1)
struct Series {
  int64_t B, L, C;
  bool ok(int64_t min_L = 2) const { return B >= 0 && L >= min_L && C >= 1; }
};
// workgroups for one lane per item; `grid_stride_blocks`: for the kernels that loop, at most 65536
static inline unsigned blocks_for(int64_t items, int per_block = 256) { return (unsigned)((items + per_block - 1) / per_block); }
static inline unsigned grid_stride_blocks(int64_t items) {
  const int64_t g = (items + 255) / 256;
  return (unsigned)(g > 65536 ? 65536 : g);
}

// ---------------------------------------------------------------- rk4_generic.hip (any shape, f32 / f64)
bool generic_applicable(int64_t C, int64_t H, size_t elem, bool adjoint);
size_t generic_adjoint_workspace_bytes(int64_t B, int64_t C, int64_t H, size_t elem);
template <typename T, typename TT>
int launch_forward_generic(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                           hipStream_t s);
template <typename T, typename TT>
int launch_adjoint_generic(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                           void* partial, hipStream_t s);

// ---------------------------------------------------------------- rk4_mfma.hip (f32, H <= 32, C <= 8; the two-layer field)
bool mfma_applicable(int64_t C, int64_t H, int dtype, int act);
size_t mfma_adjoint_partial_bytes(int64_t B);
bool mlp_shape_ok(int64_t C, int64_t H, int64_t width);        // (cde_mfma.h declares these three for the kernel files)
bool mlp_shape_hi(int64_t C, int64_t H, int64_t width);
bool mlp_shape_upper(int64_t C, int64_t H, int64_t width);
// fixed-order sum of the per-tile partial parameter gradients
int launch_reduce_partials(const float* partial, int64_t n_tiles, void* grad_W, void* grad_b, int H, int C, hipStream_t s);
template <typename TT>
int launch_forward_mfma(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                        hipStream_t s);
template <typename TT>
int launch_forward_mlp(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                       hipStream_t s);
// ... storing the stage states (`io.stages`) for adjoint=False
template <typename TT>
int launch_forward_mfma_stages(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n,
                               const StageTable& st, hipStream_t s);
template <typename TT>
int launch_forward_mlp_stages(const Control& x, const TwoLayerField& f, const ForwardIO& io, const Shape& n,
                              const StageTable& st, hipStream_t s);
// midpoint / euler (identity activation)
template <typename TT>
int launch_forward_mfma_method(int method, const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n,
                               const StageTable& st, hipStream_t s);
template <typename TT>
int launch_adjoint_mfma(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                        float* partial, hipStream_t s);
template <typename TT>
int launch_adjoint_jacobian_bx(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n,
                               const StageTable& st, float* partial, hipStream_t s);

// ---------------------------------------------------------------- revheun.hip (reversible Heun: f32, H <= 32, C <= 8)
// `nodes`: control interval and fractional part at every GRID NODE, one slot per node (api.hip: node_table_kernel)
bool revheun_applicable(int64_t C, int64_t H, int dtype, int act);
template <typename TT>
int launch_revheun_forward(const Control& x, const AffineField& f, const ForwardIO& io, void* zhat_out, const Shape& n,
                           const StageTable& nodes, hipStream_t s);
template <typename TT>
int launch_revheun_adjoint(const Control& x, const AffineField& f, const ReversibleIO& io, const Shape& n,
                           const StageTable& nodes, float* partial, hipStream_t s);

// ---------------------------------------------------------------- rk4_adjoint_pair.hip (chain wave + helper wave per tile)
template <typename TT>
int launch_adjoint_jacobian_pair(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n,
                                 const StageTable& st, float* partial, hipStream_t s, PairForm form);
int launch_backprop_jacobian_pair(const Control& x, const AffineField& f, const BackpropIO& io, const Shape& n,
                                  const StageTable& st, float* partial, hipStream_t s);

// ---------------------------------------------------------------- rk4_backprop.hip (adjoint=False of the affine field)
size_t backprop_workspace_bytes(int64_t B);
int launch_backprop_jacobian(const Control& x, const AffineField& f, const BackpropIO& io, const Shape& n, const StageTable& st,
                             float* partial, hipStream_t s);

// ------------------------------------ rk4_bf16x3.hip, rk4_bf16x3_adjoint.hip (exact operand splits on the bf16 pipe)
template <typename TT>
int launch_forward_bf16x3(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                          hipStream_t s);
// rk4_bf16x3_duo.hip: the same solve with the wave's 32 series as two interleaved groups of 16 (the default forward)
template <typename TT>
int launch_forward_bf16x3_duo(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                              hipStream_t s);
template <typename TT>
int launch_adjoint_bf16x3(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                          float* partial, hipStream_t s);

// ---------------------------------------------------------------- rk4_split.hip (one workgroup per 16 series: small batches)
size_t split_adjoint_partial_bytes(int64_t B);
template <typename TT>
int launch_forward_split(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                         hipStream_t s);
template <typename TT>
int launch_adjoint_split(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                         float* partial, hipStream_t s);

// ---------------------------------------------------------------- rk4_wide.hip (H <= 64, C <= 8 or H <= 32, C <= 16)
bool wide_applicable(int64_t C, int64_t H, int dtype, int act);
size_t wide_adjoint_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t n_steps);
template <typename TT>
int launch_forward_wide(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                        hipStream_t s);
template <typename TT>
int launch_adjoint_wide(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                        void* scratch, hipStream_t s);
// mlp_grad_reduce.hip: acc (M, N + 1) += G^T [Z | 1] over `rows` rows, G (rows, M), Z (rows, N)
size_t wide_grad_reduce_partial_bytes(int M, int N);
int launch_wide_grad_reduce(const float* G, const float* Z, int64_t rows, int M, int N, float* acc, float* partial,
                            hipStream_t s);

// ---------------------------------------------------------------- rk4_affine_tiled.hip (H <= 32, 17 <= C <= 64)
bool affine_tiled_applicable(int64_t C, int64_t H, int dtype, int act);
size_t affine_tiled_adjoint_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t n_steps);
template <typename TT>
int launch_forward_affine_tiled(const Control& x, const AffineField& f, const ForwardIO& io, const Shape& n, const StageTable& st,
                                hipStream_t s);
template <typename TT>
int launch_adjoint_affine_tiled(const Control& x, const AffineField& f, const AdjointIO& io, const Shape& n, const StageTable& st,
                                void* scratch, hipStream_t s);

// ---------------------------------------------------------------- rk4_mlp_adjoint.hip (sweeps of the two-layer field)
size_t mlp_adjoint_image_bytes();                              // (cde_mlp_adj.h declares these two for the kernel files)
int launch_mlp_adjoint_images(const void* W1, const void* b1, int64_t width, const void* W2, const void* b2, int64_t C,
                              int64_t H, float* img, hipStream_t s, float b1_pad = 0.f);
template <typename TT>
int launch_mlp_adjoint_sweep(const Control& x, const SweepIO& io, const Shape& n, const StageTable& st, hipStream_t s);
template <typename TT>
int launch_mlp_backprop_sweep(const Control& x, const SweepIO& io, const Shape& n, const StageTable& st, hipStream_t s);

// ---------------------------------------------------------------- dopri5_adjoint.hip (for K4a and K4am alike)
// the ADJ_NS pending state sums of `n_wg` workgroups -> sums; and, under "seminorm", vjp_t at the end of an interval redone
// from the reduced sums (neither asks for the launch status)
void launch_adjoint_state_sums(const double* partial, int n_wg, double* sums, hipStream_t s);
void launch_adjoint_carry(const unsigned char* ctrl, int p2, const double* reduced, double* carry, hipStream_t s);

}  // namespace cde
