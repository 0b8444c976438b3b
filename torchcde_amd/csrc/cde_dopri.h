// cde_dopri.h -- controller state and Dormand-Prince tableau shared by the adaptive kernels (dopri5.hip,
// dopri5_adjoint.hip).
#pragma once
#include "cde_mfma.h"

namespace cde {

struct DopriCtrl {
  double t_lo, t_hi, dt;        // dense-output interval of the last accepted step, next step size
  double t1_try, dt_try;        // the attempt whose partial sums are pending
  double h0;                    // Hairer initial step, phase 1 -> 2
  int64_t i_out, i_jump;        // next output index, next jump index
  int64_t n_accept, n_reject;
  int32_t phase;                // 0 start, 1 after f0 norms, 2 after f1 norm, 3 stepping, 4 done
  int32_t on_jump;              // pending attempt was clipped to a jump time
  int32_t refresh;              // k0 must be recomputed just after t_hi (we stepped onto a jump)
  int32_t pad;
  int32_t slot;                 // MFMA attempt kernel: which of the two (y, k) state slots holds the step's start
  int32_t stored;               // ... and what the pending attempt left in the other one: bit 0 k6, bit 1 the midpoint
  int32_t hint_lo, hint_hi;     // ... and the knot intervals of the pending attempt's first and last stage times: the next
                                // launch requests the control rows of its two likely intervals BEFORE it knows the decision
};
static_assert(sizeof(DopriCtrl) == 112, "cde_dopri5_status (include/cde_mi355x.h) and _lib.DopriStatus mirror this layout");

// torchdiffeq's remaining step-size options (first_step, step_t, min_step, max_step; oracle/odeint.py: _Dopri5.integrate),
// for the forward and the backward controller alike.  The kernels get ONE pointer for them (null: none of them is set and
// the controllers take exactly the path they took before these existed) to a device block of the caller's
// (cde_dopri5_step_options::state): the option values, which the first call of a solve copies there, and what the
// controller carries from launch to launch, which ping-pongs with the launch parity like the controller blocks -- every
// workgroup reads state[parity], one lane of workgroup 0 writes state[parity ^ 1].
struct StepState {
  int64_t i_step;               // next step time, counted from `first`
  int32_t on_step;              // pending attempt was clipped onto a step time (and no jump time took over)
  int32_t first;                // offset of the first kept step time (those >= the solve's start)
};
struct StepBlock {              // the device block: cde_dopri5_step_state_bytes() bytes
  double first_step;            // NaN: Hairer's rule
  double min_step, max_step;
  const double* step_t; int64_t n_step;    // ascending; the adjoint solves: in reversed time
  int64_t reserved;
  StepState state[2];
};
// The controllers' view of the block.  Every value is read where it is used and nothing of it is kept in registers: the
// attempt kernels have none to spare, and a solve without the options must not pay for them.
struct StepOptions {
  const StepBlock* b;           // null: none of the options is set
  __device__ __forceinline__ bool on() const { return b != nullptr; }
  // torchdiffeq: `if not isfinite(dt): dt = min_step; dt = dt.clamp(min_step, max_step)`
  __device__ __forceinline__ double clamp(double dt) const {
    const double min_step = b->min_step, max_step = b->max_step;
    if (!(dt - dt == 0.0)) dt = min_step;
    dt = dt < min_step ? min_step : dt;
    return dt > max_step ? max_step : dt;
  }
  __device__ __forceinline__ double first_step(double hairer) const {
    const double given = b->first_step;
    return given == given ? given : hairer;
  }
  __device__ __forceinline__ int64_t kept(const StepState& st) const { return b->n_step - st.first; }
  // phase 0: keep the step times >= t_start, start at min(bisect_right(kept, t_start), len - 1)
  __device__ __forceinline__ void begin(StepState& st, double t_start) const {
    const double* step_t = b->step_t;
    const int64_t n_step = b->n_step;
    int64_t j = 0;
    while (j < n_step && step_t[j] < t_start) ++j;
    const int64_t first = j;
    while (j < n_step && step_t[j] <= t_start) ++j;
    st.i_step = j - first;
    if (n_step - first > 0 && st.i_step > n_step - first - 1) st.i_step = n_step - first - 1;
    st.first = (int32_t)first; st.on_step = 0;
  }
  // the overrides on the decision of an attempt of length dt: longer than max_step is rejected, at most min_step accepted
  __device__ __forceinline__ bool decide(bool accept, double dt) const {
    if (dt > b->max_step) accept = false;
    if (dt <= b->min_step) accept = true;
    return accept;
  }
  // an accepted attempt that was clipped onto a step time moves on to the next one (the last one stays)
  __device__ __forceinline__ void accepted(StepState& st) const {
    if (st.on_step && st.i_step != kept(st) - 1) st.i_step++;
  }
  // a new attempt [t0, t0 + dt]: clipped onto the next step time when that lies strictly inside
  __device__ __forceinline__ void clip(StepState& st, double t0, double& t1, double& dt) const {
    st.on_step = 0;
    const int64_t at = st.first + st.i_step;
    if (at >= 0 && at < b->n_step) {                               // (begin() leaves it there whenever a time is kept)
      const double nxt = b->step_t[at];
      if (t0 < nxt && nxt < t0 + dt) { st.on_step = 1; t1 = nxt; dt = t1 - t0; }
    }
  }
  __device__ __forceinline__ void publish(const StepState& st, int parity) const {
    if (blockIdx.x == 0 && threadIdx.x == 0) const_cast<StepBlock*>(b)->state[parity ^ 1] = st;
  }
};

// host: what a caller's cde_dopri5_step_options must satisfy (checked before any HIP call; `sharded`: one controller across
// shards has no form of these options), and the kernels' view of it (null: absent)
static inline int step_options_check(const cde_dopri5_step_options* o, bool sharded) {
  if (!o) return CDE_OK;
  if (sharded) return CDE_ERR_UNSUPPORTED;
  if (!(o->min_step >= 0.0) || !(o->max_step >= o->min_step) || o->n_step < 0) return CDE_ERR_SHAPE;
  if ((o->n_step > 0 && !o->step_t) || !o->state) return CDE_ERR_NULL;
  return CDE_OK;
}
static inline const StepBlock* step_block(const cde_dopri5_step_options* o) { return o ? (const StepBlock*)o->state : nullptr; }
// the first call of a solve: the option values into the block (the struct is the caller's and may be gone when the launches run)
static inline int step_block_fill(const cde_dopri5_step_options* o, hipStream_t s) {
  if (!o) return CDE_OK;
  struct { double first_step, min_step, max_step; const double* step_t; int64_t n_step; int64_t reserved; } head = {
      o->first_step, o->min_step, o->max_step, o->step_t, o->n_step, 0};
  static_assert(sizeof(head) == offsetof(StepBlock, state), "the block's head");
  return hipMemcpyAsync(o->state, &head, sizeof(head), hipMemcpyHostToDevice, s) == hipSuccess ? CDE_OK : CDE_ERR_LAUNCH;
}

// wave-uniform copies: the controller's outputs derive from LDS reads (the block sums), so the compiler keeps them --
// and everything computed from them -- in vector registers; read back through lane 0 they live in scalar registers
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }
__device__ __forceinline__ double uni(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ int64_t uni(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Sums of NV doubles over the workgroup, the result in every thread.  Fixed order (xor-shuffle tree inside each wave,
// then the waves in index order): bit-identical in every workgroup that sums the same values, and run to run.
// `red`: NV * (blockDim.x / 64) doubles of LDS.
template <int NV>
__device__ __forceinline__ void block_total(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  __syncthreads();                                               // `red` may still be in use by an earlier call
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k * nw + wave] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += red[k * nw + w];
    v[k] = s;
  }
}

// what the previous launch left for the step options, as wave-uniform values (scalar registers: the controllers run where
// the attempt kernels have no vector register to spare)
__device__ __forceinline__ StepState step_state(const StepOptions& so, int parity) {
  StepState st{};
  if (so.on()) {
    const StepState in = so.b->state[parity];
    st.i_step = uni(in.i_step); st.on_step = uni(in.on_step); st.first = uni(in.first);
  }
  return st;
}

__device__ __forceinline__ float next_toward(float x, float dir) { return nextafterf(x, x + dir); }
__device__ __forceinline__ double next_toward(double x, double dir) { return nextafter(x, x + dir); }

// Dormand-Prince tableau (identical numbers to oracle/odeint.py)
__device__ constexpr double DP_ALPHA[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__device__ constexpr double DP_BETA[6][6] = {
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
__device__ constexpr double DP_CERR[7] = {35.0 / 384 - 1951.0 / 21600, 0, 500.0 / 1113 - 22642.0 / 50085,
                                          125.0 / 192 - 451.0 / 720, -2187.0 / 6784 - -12231.0 / 42400,
                                          11.0 / 84 - 649.0 / 6300, -1.0 / 60};
__device__ constexpr double DP_CMID[7] = {6025192743.0 / 30085553152.0 / 2, 0, 51252292925.0 / 65400821598.0 / 2,
                                          -2691868925.0 / 45128329728.0 / 2, 187940372067.0 / 1594534317056.0 / 2,
                                          -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2};

}  // namespace cde
