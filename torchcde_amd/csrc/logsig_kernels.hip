// logsig_kernels.hip -- K5: log-signature windows of the log-ODE method (forward and backward).
#include "cde_common.h"
#include "cde_launch.h"

namespace cde {

// ------------------------------------------------------------------------------------------ K5 log-ODE windows
// logsig_windows / logsignature_windows (reference log_ode.py:15-133) after the host has merged the window
// boundaries into the series and filled them linearly: for every window the logsignature (depth <= 4) of the
// piecewise-linear path between two boundary rows, optionally scaled, accumulated along the windows.
// The arithmetic the reference gets from the `signatory` package (absent here; see oracle/logsig.py): signature by
// Chen's identity  S <- S (x) exp(d)  over the increments, tensor-algebra logarithm, coefficients of the Lyndon words
// (`words`: (level, flat index) pairs in signatory's order, built by the host).
// The signature levels live in per-lane arrays, so the kernel is instantiated for the (channels, depth) envelopes that
// occur: up to 8 channels to depth 3 (config 5 and the examples), up to 5 channels to depth 4 (the reference's test
// runs depth 1-4 on 1-3 channels), up to 32 channels to depth 2.
template <int N, int P> struct IPow { static constexpr int value = N * IPow<N, P - 1>::value; };
template <int N> struct IPow<N, 0> { static constexpr int value = 1; };

// pass 1: one lane per (series, window) -- the windows of a series are independent until the running sum
template <typename T, int MAXC, int MAXD>
__global__ __launch_bounds__(64) void logsig_windows_kernel(const T* __restrict__ x, const int64_t* __restrict__ rows,
                                                            const T* __restrict__ scale, const int32_t* __restrict__ words,
                                                            T* __restrict__ out, int64_t B, int64_t L, int C, int depth,
                                                            int64_t n_windows, int n_words) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * n_windows) return;
  const int64_t b = id / n_windows, win = id - b * n_windows;
  const T* src = x + b * L * C;
  T* dst = out + (b * (n_windows + 1) + win + 1) * n_words;
  T S1[MAXC], S2[MAXD >= 2 ? IPow<MAXC, 2>::value : 1], S3[MAXD >= 3 ? IPow<MAXC, 3>::value : 1],
      S4[MAXD >= 4 ? IPow<MAXC, 4>::value : 1];
  const int C2 = C * C, C3 = C2 * C;
  for (int i = 0; i < C; ++i) S1[i] = (T)0;
  if (MAXD >= 2 && depth >= 2) for (int i = 0; i < C2; ++i) S2[i] = (T)0;
  if (MAXD >= 3 && depth >= 3) for (int i = 0; i < C3; ++i) S3[i] = (T)0;
  if (MAXD >= 4 && depth >= 4) for (int i = 0; i < C3 * C; ++i) S4[i] = (T)0;
  for (int64_t r = rows[win]; r < rows[win + 1]; ++r) {
    T d[MAXC];
    for (int i = 0; i < C; ++i) d[i] = src[(r + 1) * C + i] - src[r * C + i];
    // levels of S (x) exp(d), highest first (they read the old lower levels); exp(d): e1 = d, e2 = e1 (x) d / 2, ...
    // level k = S_k + e_k + S_1 (x) e_(k-1) + ... + S_(k-1) (x) e_1, added in that order (oracle/logsig.py)
    if (MAXD >= 4 && depth >= 4)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
          const T e2ij = d[i] * d[j] / (T)2;
          for (int k = 0; k < C; ++k) {
            const T e3ijk = e2ij * d[k] / (T)3;
            const T e2jk = d[j] * d[k] / (T)2;
            for (int l = 0; l < C; ++l) {
              const int at = ((i * C + j) * C + k) * C + l;
              T acc = S4[at] + e3ijk * d[l] / (T)4;
              acc = acc + S1[i] * (e2jk * d[l] / (T)3);
              acc = acc + S2[i * C + j] * (d[k] * d[l] / (T)2);
              acc = acc + S3[(i * C + j) * C + k] * d[l];
              S4[at] = acc;
            }
          }
        }
    if (MAXD >= 3 && depth >= 3)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
          const T e2 = d[i] * d[j] / (T)2;
          for (int k = 0; k < C; ++k) {
            T acc = S3[(i * C + j) * C + k] + e2 * d[k] / (T)3;
            acc = acc + S1[i] * (d[j] * d[k] / (T)2);
            acc = acc + S2[i * C + j] * d[k];
            S3[(i * C + j) * C + k] = acc;
          }
        }
    if (MAXD >= 2 && depth >= 2)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) S2[i * C + j] = (S2[i * C + j] + d[i] * d[j] / (T)2) + S1[i] * d[j];
    for (int i = 0; i < C; ++i) S1[i] = S1[i] + d[i];
  }
  // logarithm: log(1 + S) = S - S^2/2 + S^3/3 - S^4/4, level by level, then the Lyndon-word coordinates
  const T sc = scale[win];
  for (int w = 0; w < n_words; ++w) {
    const int level = words[2 * w], flat = words[2 * w + 1];
    T value;
    if (level == 1) value = S1[flat];
    else if (level == 2) {
      const int i = flat / C, j = flat - i * C;
      value = S2[flat] + (-(S1[i] * S1[j])) / (T)2;
    } else if (level == 3) {
      const int i = flat / C2, jk = flat - i * C2, j = jk / C, k = jk - j * C;
      const T p2 = (S1[i] * S2[j * C + k]) + S2[i * C + j] * S1[k];          // (S^2)_3
      const T p3 = (S1[i] * S1[j]) * S1[k];                                   // (S^3)_3
      value = (S3[flat] + (-p2) / (T)2) + p3 / (T)3;
    } else {
      const int i = flat / C3, jkl = flat - i * C3, j = jkl / C2, kl = jkl - j * C2, k = kl / C, l = kl - k * C;
      const int ij = i * C + j, ijk = ij * C + k;
      const T p2 = ((S1[i] * S3[jkl]) + S2[ij] * S2[kl]) + S3[ijk] * S1[l];                      // (S^2)_4
      const T s2_3 = (S1[i] * S2[j * C + k]) + S2[ij] * S1[k];                                   // (S^2)_3 at ijk
      const T p3 = ((S1[i] * S1[j]) * S2[kl]) + s2_3 * S1[l];                                    // (S^3)_4
      const T p4 = ((S1[i] * S1[j]) * S1[k]) * S1[l];                                            // (S^4)_4
      value = ((S4[flat] + (-p2) / (T)2) + p3 / (T)3) + (-p4) / (T)4;
    }
    dst[w] = value * sc;
  }
}

// pass 2: the running sum of log_ode.py:63 (sequential, like torch.cumsum on the CPU), one lane per (series, coordinate);
// row 0 = the first observation padded with zeros (log_ode.py:50-52)
template <typename T>
__global__ __launch_bounds__(256) void logsig_accumulate_kernel(const T* __restrict__ x, T* __restrict__ out, int64_t B,
                                                                int64_t L, int C, int64_t n_windows, int n_words) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * n_words) return;
  const int64_t b = id / n_words;
  const int w = (int)(id - b * n_words);
  T* col = out + b * (n_windows + 1) * n_words + w;
  T run = w < C ? x[b * L * C + w] : (T)0;
  col[0] = run;
  for (int64_t win = 1; win <= n_windows; ++win) { run = run + col[win * n_words]; col[win * n_words] = run; }
}

// ---- K5 backward (autograd through signatory's logsignature and the running sum of log_ode.py:53-63)
// pass 1: the running sum transposed -- suffix sums of grad_out along the windows, one lane per (series, coordinate);
// row k of `gsum` = sum of the rows >= k.  Row 0 is the gradient of the first observation (first C coordinates).
template <typename T>
__global__ __launch_bounds__(256) void logsig_suffix_kernel(const T* __restrict__ grad_out, T* __restrict__ gsum,
                                                            T* __restrict__ grad_x, int64_t B, int64_t L, int C,
                                                            int64_t n_windows, int n_words) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * n_words) return;
  const int64_t b = id / n_words;
  const int w = (int)(id - b * n_words);
  const T* src = grad_out + b * (n_windows + 1) * n_words + w;
  T* dst = gsum + b * (n_windows + 1) * n_words + w;
  T run = (T)0;
  for (int64_t win = n_windows; win >= 0; --win) { run = run + src[win * n_words]; dst[win * n_words] = run; }
  if (w < C) grad_x[b * L * C + w] = run;                  // grad_x was zeroed by the caller; pass 2 adds to it
}

// pass 2: one lane per (series, window).  The signature levels below the top one are rebuilt (the logarithm's and the
// Chen step's derivatives never read the top level), the word coordinates and the logarithm are differentiated into
// gS, and the Chen recursion is walked BACKWARDS: before increment r is differentiated the signature is stepped back
// with  S <- S (x) exp(-d_r)  (the reversibility signatory's own backward relies on), then
//   new_k = S_k + e_k(d) + sum_j S_j (x) e_(k-j)(d),  e_m(d) = d^(x m) / m!
// is transposed level by level, LOWEST level first (level k reads gS_k of the new signature, which the lower levels'
// updates have not touched, and adds to the lower gS).  No atomics, fixed summation order: rows interior to a window get
// both of their increments' contributions from this lane (one plain store); of a boundary row's two contributions the
// one from the window BELOW it (that window's last increment) is parked in the first C slots of the window's own `gsum`
// row -- dead once the lane has read it -- and the one from the window above it is added in place by that window's lane,
// the row's only writer in this pass; pass 3 then adds the parked values window by window.
template <typename T, int MAXC, int MAXD>
__global__ __launch_bounds__(64) void logsig_windows_backward_kernel(T* gsum, const T* __restrict__ x,
                                                                     const int64_t* __restrict__ rows,
                                                                     const T* __restrict__ scale,
                                                                     const int32_t* __restrict__ words,
                                                                     T* __restrict__ grad_x, int64_t B, int64_t L, int C,
                                                                     int depth, int64_t n_windows, int n_words) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * n_windows) return;
  const int64_t b = id / n_windows, win = id - b * n_windows;
  const T* src = x + b * L * C;
  T* gx = grad_x + b * L * C;
  T* gw = gsum + (b * (n_windows + 1) + win + 1) * n_words;
  T S1[MAXC], S2[MAXD >= 3 ? IPow<MAXC, 2>::value : 1], S3[MAXD >= 4 ? IPow<MAXC, 3>::value : 1];
  T g1[MAXC], g2[MAXD >= 2 ? IPow<MAXC, 2>::value : 1], g3[MAXD >= 3 ? IPow<MAXC, 3>::value : 1],
      g4[MAXD >= 4 ? IPow<MAXC, 4>::value : 1];
  const int C2 = C * C, C3 = C2 * C;
  for (int i = 0; i < C; ++i) { S1[i] = (T)0; g1[i] = (T)0; }
  if (MAXD >= 2 && depth >= 2) for (int i = 0; i < C2; ++i) g2[i] = (T)0;
  if (MAXD >= 3 && depth >= 3) for (int i = 0; i < C2; ++i) S2[i] = (T)0;
  if (MAXD >= 3 && depth >= 3) for (int i = 0; i < C3; ++i) g3[i] = (T)0;
  if (MAXD >= 4 && depth >= 4) for (int i = 0; i < C3; ++i) S3[i] = (T)0;
  if (MAXD >= 4 && depth >= 4) for (int i = 0; i < C3 * C; ++i) g4[i] = (T)0;
  const int64_t r_lo = rows[win], r_hi = rows[win + 1];
  // ---- the signature of the window, levels 1 .. depth-1 (same operations as the forward kernel)
  for (int64_t r = r_lo; r < r_hi; ++r) {
    T d[MAXC];
    for (int i = 0; i < C; ++i) d[i] = src[(r + 1) * C + i] - src[r * C + i];
    if (MAXD >= 4 && depth >= 4)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
          const T e2 = d[i] * d[j] / (T)2;
          for (int k = 0; k < C; ++k) {
            T acc = S3[(i * C + j) * C + k] + e2 * d[k] / (T)3;
            acc = acc + S1[i] * (d[j] * d[k] / (T)2);
            acc = acc + S2[i * C + j] * d[k];
            S3[(i * C + j) * C + k] = acc;
          }
        }
    if (MAXD >= 3 && depth >= 3)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) S2[i * C + j] = (S2[i * C + j] + d[i] * d[j] / (T)2) + S1[i] * d[j];
    for (int i = 0; i < C; ++i) S1[i] = S1[i] + d[i];
  }
  // ---- word coordinates and logarithm, transposed
  const T sc = scale[win];
  for (int w = 0; w < n_words; ++w) {
    const int level = words[2 * w], flat = words[2 * w + 1];
    const T g = gw[w] * sc;
    if (level == 1) g1[flat] += g;
    else if (level == 2) {
      if (MAXD >= 2) {
        const int i = flat / C, j = flat - i * C;
        g2[flat] += g;
        const T h = -g / (T)2;
        const T si = S1[i], sj = S1[j];
        g1[i] += h * sj; g1[j] += h * si;
      }
    } else if (level == 3) {
      if (MAXD >= 3) {
        const int i = flat / C2, jk = flat - i * C2, j = jk / C, k = jk - j * C, ij = i * C + j;
        g3[flat] += g;
        const T h2 = -g / (T)2, h3 = g / (T)3;
        const T si = S1[i], sj = S1[j], sk = S1[k], sjk = S2[jk], sij = S2[ij];
        g1[i] += h2 * sjk + h3 * sj * sk;
        g1[j] += h3 * si * sk;
        g1[k] += h2 * sij + h3 * si * sj;
        g2[jk] += h2 * si;
        g2[ij] += h2 * sk;
      }
    } else {
      if (MAXD >= 4) {
        const int i = flat / C3, jkl = flat - i * C3, j = jkl / C2, kl = jkl - j * C2, k = kl / C, l = kl - k * C;
        const int ij = i * C + j, jk = j * C + k, ijk = ij * C + k;
        g4[flat] += g;
        const T h2 = -g / (T)2, h3 = g / (T)3, h4 = -g / (T)4;
        const T si = S1[i], sj = S1[j], sk = S1[k], sl = S1[l];
        const T sij = S2[ij], sjk = S2[jk], skl = S2[kl], sijk = S3[ijk], sjkl = S3[jkl];
        // (S^2)_4 = S1_i S3_jkl + S2_ij S2_kl + S3_ijk S1_l
        g1[i] += h2 * sjkl; g3[jkl] += h2 * si;
        g2[ij] += h2 * skl; g2[kl] += h2 * sij;
        g3[ijk] += h2 * sl; g1[l] += h2 * sijk;
        // (S^3)_4 = S1_i S1_j S2_kl + (S1_i S2_jk + S2_ij S1_k) S1_l
        const T s23 = si * sjk + sij * sk, hs = h3 * sl;
        g1[i] += h3 * sj * skl + hs * sjk;
        g1[j] += h3 * si * skl;
        g2[kl] += h3 * si * sj;
        g1[l] += h3 * s23;
        g2[jk] += hs * si;
        g2[ij] += hs * sk;
        g1[k] += hs * sij;
        // (S^4)_4 = S1_i S1_j S1_k S1_l
        g1[i] += h4 * sj * sk * sl; g1[j] += h4 * si * sk * sl; g1[k] += h4 * si * sj * sl; g1[l] += h4 * si * sj * sk;
      }
    }
  }
  // ---- Chen's recursion backwards
  T carry[MAXC];                                            // -(dL/dd) of the increment above: what row r+1 still owes
  for (int i = 0; i < C; ++i) carry[i] = (T)0;
  for (int64_t r = r_hi - 1; r >= r_lo; --r) {
    T d[MAXC], gd[MAXC];
    for (int i = 0; i < C; ++i) d[i] = src[(r + 1) * C + i] - src[r * C + i];
    // step the signature back: S <- S (x) exp(-d), highest level first
    if (MAXD >= 4 && depth >= 4)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
          const T e2 = d[i] * d[j] / (T)2;
          for (int k = 0; k < C; ++k)
            S3[(i * C + j) * C + k] = ((S3[(i * C + j) * C + k] - e2 * d[k] / (T)3) + S1[i] * (d[j] * d[k] / (T)2)) - S2[i * C + j] * d[k];
        }
    if (MAXD >= 3 && depth >= 3)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) S2[i * C + j] = (S2[i * C + j] + d[i] * d[j] / (T)2) - S1[i] * d[j];
    if (depth >= 2) for (int i = 0; i < C; ++i) S1[i] = S1[i] - d[i];
    // transposed step, lowest level first
    for (int i = 0; i < C; ++i) gd[i] = g1[i];
    if (MAXD >= 2 && depth >= 2)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) {
          const T G = g2[i * C + j];
          gd[i] += G * d[j] / (T)2;
          gd[j] += G * (d[i] / (T)2 + S1[i]);
          g1[i] += G * d[j];
        }
    if (MAXD >= 3 && depth >= 3)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j)
          for (int k = 0; k < C; ++k) {
            const T G = g3[(i * C + j) * C + k];
            const T s1 = S1[i], s2 = S2[i * C + j];
            gd[i] += G * d[j] * d[k] / (T)6;
            gd[j] += G * (d[i] * d[k] / (T)6 + s1 * d[k] / (T)2);
            gd[k] += G * (d[i] * d[j] / (T)6 + s1 * d[j] / (T)2 + s2);
            g1[i] += G * d[j] * d[k] / (T)2;
            g2[i * C + j] += G * d[k];
          }
    if (MAXD >= 4 && depth >= 4)
      for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j)
          for (int k = 0; k < C; ++k)
            for (int l = 0; l < C; ++l) {
              const T G = g4[((i * C + j) * C + k) * C + l];
              const T s1 = S1[i], s2 = S2[i * C + j], s3 = S3[(i * C + j) * C + k];
              gd[i] += G * d[j] * d[k] * d[l] / (T)24;
              gd[j] += G * (d[i] * d[k] * d[l] / (T)24 + s1 * d[k] * d[l] / (T)6);
              gd[k] += G * (d[i] * d[j] * d[l] / (T)24 + s1 * d[j] * d[l] / (T)6 + s2 * d[l] / (T)2);
              gd[l] += G * (d[i] * d[j] * d[k] / (T)24 + s1 * d[j] * d[k] / (T)6 + s2 * d[k] / (T)2 + s3);
              g1[i] += G * d[j] * d[k] * d[l] / (T)6;
              g2[i * C + j] += G * d[k] * d[l] / (T)2;
              g3[(i * C + j) * C + k] += G * d[l];
            }
    // d = x_{r+1} - x_r
    if (r == r_hi - 1) for (int i = 0; i < C; ++i) { gw[i] = gd[i]; carry[i] = -gd[i]; }       // boundary row above: parked
    else for (int i = 0; i < C; ++i) { gx[(r + 1) * C + i] = gd[i] + carry[i]; carry[i] = -gd[i]; }
  }
  if (r_hi > r_lo) for (int i = 0; i < C; ++i) gx[r_lo * C + i] += carry[i];
  else for (int i = 0; i < C; ++i) gw[i] = (T)0;           // empty window: nothing parked
}

// pass 3: the parked boundary contributions, one lane per (series, channel), windows in order (several empty windows may
// share a row)
template <typename T>
__global__ __launch_bounds__(256) void logsig_boundary_kernel(const T* __restrict__ gsum, const int64_t* __restrict__ rows,
                                                              T* __restrict__ grad_x, int64_t B, int64_t L, int C,
                                                              int64_t n_windows, int n_words) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * C) return;
  const int64_t b = id / C;
  const int i = (int)(id - b * C);
  T* gx = grad_x + b * L * C + i;
  const T* parked = gsum + b * (n_windows + 1) * n_words + i;
  for (int64_t win = 0; win < n_windows; ++win) gx[rows[win + 1] * C] += parked[(win + 1) * n_words];
}

// the envelopes of the per-lane signature arrays, the one place the code lists them: `f(Const<MAXC>{}, Const<MAXD>{})` for the
// first one that holds (C channels, depth); CDE_ERR_UNSUPPORTED when none does
template <typename F>
static int dispatch_envelope(int64_t C, int depth, F&& f) {
  if (depth >= 1 && depth <= 3 && C <= 8) return f(Const<8>{}, Const<3>{});
  if (depth == 4 && C <= 5) return f(Const<5>{}, Const<4>{});
  if (depth >= 1 && depth <= 2 && C <= 32) return f(Const<32>{}, Const<2>{});
  return CDE_ERR_UNSUPPORTED;
}

}  // namespace cde

// ================================================================================================ C ABI
// The order of the checks: the sizes, the envelope, the empty batch (a no-op), the pointers, the dtype
// (tests/rejected_calls.py pins it).
using namespace cde;

extern "C" int cde_logsig_windows(const void* x, const int64_t* rows, const void* scale, const int32_t* words, void* out,
                                  int64_t B, int64_t L, int64_t C, int depth, int64_t n_windows, int n_words, int dtype,
                                  void* stream) {
  if (B < 0 || L < 1 || C < 1 || n_windows < 0 || n_words < 1) return CDE_ERR_SHAPE;
  return dispatch_envelope(C, depth, [&](auto MAXC, auto MAXD) -> int {
    if (B == 0) return CDE_OK;
    if (!x || !rows || !scale || !words || !out) return CDE_ERR_NULL;
    return dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipStream_t s = (hipStream_t)stream;
      if (n_windows > 0)
        logsig_windows_kernel<T, MAXC(), MAXD()><<<blocks_for(B * n_windows, 64), 64, 0, s>>>(
            (const T*)x, rows, (const T*)scale, words, (T*)out, B, L, (int)C, depth, n_windows, n_words);
      logsig_accumulate_kernel<T><<<blocks_for(B * n_words), 256, 0, s>>>(
          (const T*)x, (T*)out, B, L, (int)C, n_windows, n_words);
      return check_launch();
    });
  });
}

// grad_out (B, n_windows + 1, n_words) -> grad_x (B, L, C) w.r.t. the filled series the forward call was given;
// `workspace` has the size of grad_out.
extern "C" int cde_logsig_windows_backward(const void* grad_out, const void* x, const int64_t* rows, const void* scale,
                                           const int32_t* words, void* grad_x, void* workspace, int64_t B, int64_t L,
                                           int64_t C, int depth, int64_t n_windows, int n_words, int dtype, void* stream) {
  if (B < 0 || L < 1 || C < 1 || n_windows < 0 || n_words < 1) return CDE_ERR_SHAPE;
  return dispatch_envelope(C, depth, [&](auto MAXC, auto MAXD) -> int {
    if (B == 0) return CDE_OK;
    if (!grad_out || !x || !rows || !scale || !words || !grad_x || !workspace) return CDE_ERR_NULL;
    return dispatch_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipStream_t s = (hipStream_t)stream;
      zero_async(grad_x, (size_t)(B * L * C) * sizeof(T), s);
      logsig_suffix_kernel<T><<<blocks_for(B * n_words), 256, 0, s>>>(
          (const T*)grad_out, (T*)workspace, (T*)grad_x, B, L, (int)C, n_windows, n_words);
      if (n_windows > 0) {
        logsig_windows_backward_kernel<T, MAXC(), MAXD()><<<blocks_for(B * n_windows, 64), 64, 0, s>>>(
            (T*)workspace, (const T*)x, rows, (const T*)scale, words, (T*)grad_x, B, L, (int)C, depth, n_windows, n_words);
        logsig_boundary_kernel<T><<<blocks_for(B * C), 256, 0, s>>>(
            (const T*)workspace, rows, (T*)grad_x, B, L, (int)C, n_windows, n_words);
      }
      return check_launch();
    });
  });
}
