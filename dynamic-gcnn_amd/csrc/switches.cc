// switches.cc -- the one table of process-wide switches (switches.h) and its two C entries, dgcnn_switch_get / dgcnn_switch_set.
//
// A row: the name, whether the environment is read (and under which variable), the default, `text` (environment string -> int;
// null = atoi) and `fix` (int -> the value the parse keeps; null = every value).  The environment parse is fix(text(string));
// a value is valid for dgcnn_switch_set and for the switch's own setter exactly when fix leaves it alone, so every quirk of a
// row is written once.  The environment is read once, by the constructor of the function-local table; values are
// std::atomic<int> and a read is one relaxed load.  Plain C++17, no HIP header.
#include "switches.h"
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/dgcnn_hip.h"

#ifndef DGCNN_GEMM_ARITH_DEFAULT
#define DGCNN_GEMM_ARITH_DEFAULT 6
#endif

namespace dg {
void set_error(const char* fmt, ...);        // api.cc

namespace {

struct Row {
  const char* name;
  const char* env;                           // null: the environment is not read
  int def;
  int (*text)(const char*);
  int (*fix)(int);
};

int text_bf16f(const char* e) { return e[0] == 'a' ? 2 : atoi(e); }                 // 0 | 1 | auto
int text_not0(const char* e) { return e[0] == '0' ? 0 : 1; }                         // only a leading 0 switches it off
int text_npr(const char* e, int which) {                                             // "<lx>,<big>"
  int v[2] = {1, 1};
  sscanf(e, "%d,%d", &v[0], &v[1]);
  return v[which];
}
int text_npr_lx(const char* e) { return text_npr(e, 0); }
int text_npr_big(const char* e) { return text_npr(e, 1); }
int text_arith(const char* e) {                                                      // f32 | bf16x6 | bf16x9 | bf16x1, or 0 | 6 | 9 | 1
  return (e[0] == 'f' || e[0] == '0') ? 0 : ((e[0] == '9' || (e[0] == 'b' && e[5] == '9')) ? 9 : ((e[0] == '1' || (e[0] == 'b' && e[5] == '1')) ? 1 : 6));
}
int text_flags(const char* e) { return (int)(unsigned)strtoul(e, nullptr, 0); }      // decimal, 0x..., 0...: the unsigned's bits

int fix_bool(int v) { return v ? 1 : 0; }
int fix_tighten(int v) { return (v < 0 || (v & (v - 1))) ? 1 : v; }                  // a power of two; 0 = the per-form default
int fix_big_k(int v) { return (v < 1 || v > SW_KNN_BIG_ONLY_K) ? SW_KNN_BIG_ONLY_K : v; }
int fix_npr(int v) { return v == 3 ? 3 : 1; }
int fix_hist(int v) { return (v == 0 || v == 1 || v == 2 || v == 4) ? v : 2; }
int fix_wide_c(int v) { return (v < 5 || v > SW_KNN_WIDE_ONLY_C) ? SW_KNN_WIDE_ONLY_C : v; }
int fix_grid(int v) { return v == 2 ? 2 : (v ? 1 : 0); }
int fix_mix(int v) { return v < 0 ? 0 : v; }
int fix_arith(int v) { return (v == 0 || v == 1 || v == 6 || v == 9) ? v : DGCNN_GEMM_ARITH_DEFAULT; }
int fix_tile(int v) { return (v == 128 || v == 256 || v == 512 || v == 448) ? v : 0; }   // 512: 256 x 256, 448: 192 x 256

// hipEventDisableTiming | hipEventDisableSystemFence (plan.cc checks the literal against the HIP header)
constexpr int EVENT_FLAGS_DEFAULT = 0x2 | 0x20000000;
static_assert(SW_UNSET == DGCNN_SWITCH_UNSET, "include/dgcnn_hip.h: the unset value of DGCNN_KNN_GRID_MIN_N");

const Row ROWS[SW_COUNT] = {
    /* SW_KNN_BF16F          */ {"DGCNN_KNN_BF16F", "DGCNN_KNN_BF16F", 2, text_bf16f, nullptr},
    /* SW_KNN_FORCE_VALU     */ {"DGCNN_KNN_FORCE_VALU", nullptr, 0, nullptr, fix_bool},
    /* SW_KNN_TIGHTEN_EVERY  */ {"DGCNN_KNN_TIGHTEN_EVERY", "DGCNN_KNN_TIGHTEN_EVERY", 0, nullptr, fix_tighten},
    /* SW_KNN_BIG_K_MIN      */ {"DGCNN_KNN_BIG_K_MIN", "DGCNN_KNN_BIG_K_MIN", SW_KNN_BIG_ONLY_K, nullptr, fix_big_k},
    /* SW_KNN_SEED_MIN_N     */ {"DGCNN_KNN_SEED_MIN_N", "DGCNN_KNN_SEED_MIN_N", -1, nullptr, nullptr},
    /* SW_KNN_APPEND         */ {"DGCNN_KNN_APPEND", "DGCNN_KNN_APPEND", 1, nullptr, fix_bool},
    /* SW_KNN_APPEND_NPR_LX  */ {"DGCNN_KNN_APPEND_NPR_LX", "DGCNN_KNN_APPEND_NPR", 1, text_npr_lx, fix_npr},
    /* SW_KNN_APPEND_NPR_BIG */ {"DGCNN_KNN_APPEND_NPR_BIG", "DGCNN_KNN_APPEND_NPR", 1, text_npr_big, fix_npr},
    /* SW_KNN_HIST           */ {"DGCNN_KNN_HIST", "DGCNN_KNN_HIST", 2, nullptr, fix_hist},
    /* SW_KNN_WIDE_MIN_C     */ {"DGCNN_KNN_WIDE_MIN_C", "DGCNN_KNN_WIDE_MIN_C", SW_KNN_WIDE_ONLY_C, nullptr, fix_wide_c},
    /* SW_KNN_GRID           */ {"DGCNN_KNN_GRID", "DGCNN_KNN_GRID", 1, text_not0, fix_grid},
    /* SW_KNN_GRID_MIN_N     */ {"DGCNN_KNN_GRID_MIN_N", "DGCNN_KNN_GRID_MIN_N", SW_UNSET, nullptr, nullptr},
    /* SW_KNN_MIX_MIN_N      */ {"DGCNN_KNN_MIX_MIN_N", "DGCNN_KNN_MIX_MIN_N", 0, nullptr, fix_mix},
    /* SW_EDGE_VALU          */ {"DGCNN_EDGE_VALU", "DGCNN_EDGE_VALU", 1, text_not0, fix_bool},
    /* SW_GEMM_ARITH         */ {"DGCNN_GEMM_ARITH", "DGCNN_GEMM_ARITH", DGCNN_GEMM_ARITH_DEFAULT, text_arith, fix_arith},
    /* SW_GEMM_X3_TILE       */ {"DGCNN_GEMM_X3_TILE", nullptr, 0, nullptr, fix_tile},
    /* SW_EVENT_FLAGS        */ {"DGCNN_EVENT_FLAGS", "DGCNN_EVENT_FLAGS", EVENT_FLAGS_DEFAULT, text_flags, nullptr},
};

int fixed(const Row& r, int v) { return r.fix ? r.fix(v) : v; }

struct Table {
  std::atomic<int> v[SW_COUNT];
  int initial[SW_COUNT];
  Table() {
    for (int s = 0; s < SW_COUNT; ++s) {
      const Row& r = ROWS[s];
      const char* e = r.env ? getenv(r.env) : nullptr;
      initial[s] = e ? fixed(r, r.text ? r.text(e) : atoi(e)) : r.def;
      v[s].store(initial[s], std::memory_order_relaxed);
    }
  }
};

Table& table() {
  static Table t;
  return t;
}

int find(const char* name) {
  for (int s = 0; name && s < SW_COUNT; ++s)
    if (strcmp(name, ROWS[s].name) == 0) return s;
  return -1;
}

int unknown(const char* what, const char* name) {
  char names[640] = "";
  for (int s = 0; s < SW_COUNT; ++s) {
    strncat(names, s ? ", " : "", sizeof(names) - strlen(names) - 1);
    strncat(names, ROWS[s].name, sizeof(names) - strlen(names) - 1);
  }
  set_error("%s: no switch named %s (known: %s)", what, name ? name : "(null)", names);
  return DGCNN_EINVAL;
}

}  // namespace

int sw_get(Switch s) { return table().v[s].load(std::memory_order_relaxed); }
int sw_initial(Switch s) { return table().initial[s]; }
bool sw_valid(Switch s, int v) { return fixed(ROWS[s], v) == v; }
int sw_exchange(Switch s, int v) { return table().v[s].exchange(v, std::memory_order_relaxed); }

}  // namespace dg

extern "C" int dgcnn_switch_get(const char* name, int* value) {
  const int s = dg::find(name);
  if (s < 0) return dg::unknown("dgcnn_switch_get", name);
  if (!value) {
    dg::set_error("dgcnn_switch_get: value is null");
    return DGCNN_EINVAL;
  }
  *value = dg::sw_get((dg::Switch)s);
  return DGCNN_OK;
}

extern "C" int dgcnn_switch_set(const char* name, int value) {
  const int s = dg::find(name);
  if (s < 0) return dg::unknown("dgcnn_switch_set", name);
  if (!dg::sw_valid((dg::Switch)s, value)) {
    dg::set_error("dgcnn_switch_set: %d is not a value of %s (the environment parse would read it as %d)", value, name,
                  dg::fixed(dg::ROWS[s], value));
    return DGCNN_EINVAL;
  }
  dg::sw_exchange((dg::Switch)s, value);
  return DGCNN_OK;
}
