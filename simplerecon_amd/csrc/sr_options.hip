// sr_options.hip -- the library's run-time switches as an explicit, thread-safe option table (r05).
//
// r01-r04 read tuning / ablation switches -- and the two fenced split-precision modes, which change the NUMERICS of every call
// -- with getenv() inside the entry points, several of them per launch; hosts flipped them by mutating the process
// environment (setenv vs getenv is a data race in glibc, leaks to child processes, costs an environ scan per launch).
// Now every switch is an entry of this table: atomically readable (sr_option_get), explicitly settable (sr_option_set), and
// initialised ONCE, at the first access, from the environment variable of the same name (so `SR_WINO_XCD=0 python ...` keeps
// working for tuning runs).  After that first access the environment is never read again.  The table is process-wide: an option
// set while another thread launches affects that thread's next launch (documented in include/simplerecon_hip.h).
#include <atomic>
#include <map>
#include <mutex>
#include <utility>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sr_common.h"

namespace {

struct OptDef { const char* name; int dflt; int kind; };   // kind 0: integer, 1: split-precision mode string, 2: MLP tile shape
const OptDef kDefs[SR_OPT_COUNT] = {
    {"SR_MLP_SPLIT", 0, 1},       {"SR_WINO_SPLIT", 0, 1},     {"SR_WINO_XCD", 1, 0},        {"SR_WINO_NT", 0, 0},
    {"SR_WINO_KSPLIT", 0, 0},     {"SR_CONV_WINO", 1, 0},      {"SR_CONV_TILE", 0, 0},       {"SR_CONV_KSPLIT", 1, 0},
    {"SR_PW_NT", 0, 0},           {"SR_PW_KS", 0, 0},          {"SR_PT_CFG", -1, 0},         {"SR_PT_KS", 0, 0},
    {"SR_DOT_LDS", 1, 0},         {"SR_DOT_LDS_G", 0, 0},      {"SR_DOT_LDS_CULL", 1, 0},    {"SR_DOT_LDS_CAP", 634, 0},
    {"SR_UPSAMPLE_QUAD", 1, 0},   {"SR_POOL_STREAM", 1, 0},    {"SR_MLP_TILE", 0, 2},
};
std::atomic<int> g_val[SR_OPT_COUNT];
std::once_flag g_once;

int parse(const OptDef& d, const char* e) {
  if (d.kind == 1) {
    if (!e || !*e || !strcmp(e, "0") || !strcmp(e, "off") || !strcmp(e, "fp32")) return 0;
    if (!strcmp(e, "bf16")) return 1;
    if (!strcmp(e, "f16") || !strcmp(e, "fp16")) return 2;
    return -1;   // unknown: the entry points that honour the mode refuse to run (SR_ERR_INVALID_ARGUMENT)
  }
  if (d.kind == 2) {   // sr_mlp_volume_tile_shape
    static const char* const names[] = {"auto", "flat", "2x32", "4x16", "8x8"};
    if (!e || !*e) return d.dflt;
    for (int i = 0; i < 5; ++i)
      if (!strcmp(e, names[i])) return i;
    return -1;   // unknown: the sweep refuses to run
  }
  return (e && *e) ? atoi(e) : d.dflt;
}

void init() {
  for (int i = 0; i < SR_OPT_COUNT; ++i) {
    const char* e = getenv(kDefs[i].name);
    g_val[i].store(e ? parse(kDefs[i], e) : kDefs[i].dflt, std::memory_order_relaxed);
  }
}

}  // namespace

int sr_opt(int id) {
  std::call_once(g_once, init);
  return g_val[id].load(std::memory_order_relaxed);
}

extern "C" int sr_option_count(void) { return SR_OPT_COUNT; }

extern "C" const char* sr_option_name(int id) { return (id >= 0 && id < SR_OPT_COUNT) ? kDefs[id].name : nullptr; }

extern "C" int sr_option_id(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < SR_OPT_COUNT; ++i)
    if (!strcmp(kDefs[i].name, name)) return i;
  return -1;
}

extern "C" int sr_option_get(int id, int* value) {
  if (id < 0 || id >= SR_OPT_COUNT || !value) return SR_ERR_INVALID_ARGUMENT;
  *value = sr_opt(id);
  return SR_OK;
}

extern "C" int sr_option_set(int id, int value, int* previous) {
  if (id < 0 || id >= SR_OPT_COUNT) return SR_ERR_INVALID_ARGUMENT;
  std::call_once(g_once, init);
  const int old = g_val[id].exchange(value, std::memory_order_relaxed);
  if (previous) *previous = old;
  return SR_OK;
}

extern "C" int sr_option_default(int id, int* value) {
  if (id < 0 || id >= SR_OPT_COUNT || !value) return SR_ERR_INVALID_ARGUMENT;
  *value = kDefs[id].dflt;
  return SR_OK;
}

// CU count of the current device, cached per device index (launch plans of every translation unit ask this; ADVICE r05: a
// process-wide static answered with the first device's count for all of them)
int sr_device_cus() {
  constexpr int kMaxDevices = 64;
  static std::atomic<int> cus[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
  int v = cus[dev].load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cus[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

// The kernel the calling thread's last launcher call issued, as its launch site noted it (sr_common.h).  Nothing is formatted
// and no floating point is touched until somebody asks: sr_last_launch below, only under a profiling bracket.
static thread_local SrLaunchNote t_note = {SR_K_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};

void sr_note_launch(const SrLaunchNote& note) { t_note = note; }

extern "C" int sr_last_launch(char* name, int name_capacity, double* executed_flops) {
  const SrLaunchNote n = t_note;
  t_note.kernel = SR_K_NONE;
  if (n.kernel == SR_K_NONE || !name || name_capacity <= 0 || !executed_flops) return SR_ERR_INVALID_ARGUMENT;
  const char* const tf[2] = {"false", "true"};
  // the template arguments chosen per launch, in the kernel's order (trailing ones that a launcher fixes, such as the I/O format,
  // are left out); the tiled pointwise kernel by its workgroup tile and K split, not by the <WM, WN, NTW> the tile follows from
  switch (n.kernel) {
    case SR_K_CONV: snprintf(name, name_capacity, "sr_conv_kernel<%d, %d, %d, %d, %d, %s>", n.a, n.b, n.c, n.d, n.e, tf[n.f != 0]); break;
    case SR_K_WINO: snprintf(name, name_capacity, "sr_wino_kernel<%d, %s, %s>", n.a, tf[n.b != 0], tf[n.c != 0]); break;
    case SR_K_WINO_SPLIT: snprintf(name, name_capacity, "sr_wino_split_kernel<%d, %d>", n.a, n.b); break;
    case SR_K_WINO4: snprintf(name, name_capacity, "%s", n.a == 3 ? "sr_wino4ws_kernel" : n.a == 2 ? "sr_wino4pp_kernel" : "sr_wino4_kernel"); break;
    case SR_K_PW: snprintf(name, name_capacity, "sr_pw_kernel<%d, %d, %s>", n.a, n.b, tf[n.c != 0]); break;
    case SR_K_PW_TILED: snprintf(name, name_capacity, "sr_pw_tiled_kernel<%dx%d, ks %d, %s>", n.a, n.b, n.c, tf[n.d != 0]); break;
    case SR_K_STEM: snprintf(name, name_capacity, "sr_stem_kernel"); break;
    case SR_K_C1S: snprintf(name, name_capacity, "sr_conv1x1_stats_kernel"); break;
    case SR_K_T16: snprintf(name, name_capacity, "sr_t16_kernel"); break;
    default: return SR_ERR_INVALID_ARGUMENT;
  }
  *executed_flops = n.m > 0 ? 2.0 * (double)n.m * (double)n.n * (double)n.k : -1.0;
  return SR_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize once per (kernel, device) instead of once per launch: the largest
// size granted is remembered under the kernel's host pointer, and the runtime is asked again only for a larger one (the MLP
// sweep's LDS grows with its view count).  A refusal is returned and not remembered.
hipError_t sr_allow_lds(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> granted;
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev)) return e;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[{kernel, dev}];
  if (bytes <= have) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) return e;
  have = bytes;
  return hipSuccess;
}
