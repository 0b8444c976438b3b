// library.hip -- what the library exports about itself: the ABI version, the error strings and the tuning table that
// every solver's layout functions and launchers read through cde::option (declared in cde_common.h).  Host code only: it
// includes no header that defines a kernel.
#include <atomic>
#include <stdint.h>

#include "../../include/cde_mi355x.h"

namespace cde {
int64_t option(int key);
static constexpr int64_t OPTION_DEFAULTS[] = {
    /* K3_FORM */ 0, /* K3_WAVES */ 0, /* K3D_WAVES */ 0, /* K2M_NO_SPLIT */ 0, /* K3M_NO_SPLIT */ 0, /* K3M_SPLIT4 */ 0,
    /* K3M_S8_TILES */ -1, /* K4_NO_SPLIT */ 0, /* K4M_NO_SPLIT */ 0, /* K4M_SPLIT_TILES */ -1, /* K4AM_WAVES */ 0,
    /* K4AM_S8_TILES */ -1, /* K4AM_SPLIT4 */ 0, /* K4AM_NO_SPLIT */ 0, /* K4AM_NO_SMALL_REDUCE */ 0, /* K4AM_SPS */ 0,
    /* K4AM_NO_FSAL */ 0, /* WIDE_SCRATCH_BYTES */ 0, /* K2B_GROUPS */ 0};
static_assert(sizeof(OPTION_DEFAULTS) / sizeof(OPTION_DEFAULTS[0]) == CDE_OPT_COUNT, "one default per CDE_OPT_* key");
// the live table: it starts out as cde_reset_options leaves it
static struct Options {
  std::atomic<int64_t> value[CDE_OPT_COUNT];
  Options() { reset(); }
  void reset() {
    for (int k = 0; k < CDE_OPT_COUNT; ++k) value[k].store(OPTION_DEFAULTS[k], std::memory_order_relaxed);
  }
} g_options;
int64_t option(int key) { return g_options.value[key].load(std::memory_order_relaxed); }
}  // namespace cde

extern "C" int cde_abi_version(void) { return CDE_ABI_VERSION; }

extern "C" int cde_set_option(int key, int64_t value) {
  if (key < 0 || key >= CDE_OPT_COUNT) return CDE_ERR_SHAPE;
  cde::g_options.value[key].store(value, std::memory_order_relaxed);
  return CDE_OK;
}
extern "C" int64_t cde_get_option(int key) {
  if (key < 0 || key >= CDE_OPT_COUNT) return INT64_MIN;
  return cde::option(key);
}
extern "C" int cde_reset_options(void) {
  cde::g_options.reset();
  return CDE_OK;
}

extern "C" const char* cde_error_string(int code) {
  switch (code) {
    case CDE_OK: return "ok";
    case CDE_ERR_NULL: return "a required pointer argument is NULL";
    case CDE_ERR_DTYPE: return "unknown dtype enum (expected CDE_F32 or CDE_F64)";
    case CDE_ERR_SHAPE: return "a size argument is out of range";
    case CDE_ERR_UNSUPPORTED: return "this (dtype, shape, activation, variant) combination is not implemented";
    case CDE_ERR_WORKSPACE: return "workspace smaller than cde_rk4_adjoint_workspace_bytes()";
    case CDE_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown error code";
  }
}
