// switches.h -- the process-wide A/B switches of libdgcnn_hip.so: one table (switches.cc), filled from the environment when it is
// first touched, read with one relaxed atomic load.  Plain C++17, no HIP header: switches.cc also builds on its own
// (switch_threads_check.cc).  The rules that read a switch stay where they are (knn.hip, knn_grid.hip, bn.hip, gemm_x3.hip,
// plan.cc); only the state lives here.  include/dgcnn_hip.h lists the names dgcnn_switch_get / dgcnn_switch_set know.
#pragma once
#include <limits.h>

namespace dg {

enum Switch {
  SW_KNN_BF16F,
  SW_KNN_FORCE_VALU,
  SW_KNN_TIGHTEN_EVERY,
  SW_KNN_BIG_K_MIN,
  SW_KNN_SEED_MIN_N,
  SW_KNN_APPEND,
  SW_KNN_APPEND_NPR_LX,       // the two halves of $DGCNN_KNN_APPEND_NPR="<lx>,<big>"
  SW_KNN_APPEND_NPR_BIG,
  SW_KNN_HIST,
  SW_KNN_WIDE_MIN_C,
  SW_KNN_GRID,
  SW_KNN_GRID_MIN_N,
  SW_KNN_MIX_MIN_N,
  SW_EDGE_VALU,
  SW_GEMM_ARITH,
  SW_GEMM_X3_TILE,
  SW_EVENT_FLAGS,
  SW_COUNT
};

constexpr int SW_UNSET = INT_MIN;            // DGCNN_KNN_GRID_MIN_N: not given (it overrides two different defaults)
constexpr int SW_KNN_BIG_ONLY_K = 65;        // the defaults (and upper ends) of DGCNN_KNN_BIG_K_MIN and DGCNN_KNN_WIDE_MIN_C
constexpr int SW_KNN_WIDE_ONLY_C = 129;

int sw_get(Switch s);                        // the value in force
int sw_initial(Switch s);                    // what the environment (or the default) gave
bool sw_valid(Switch s, int v);              // v is a value the row's parse would have kept
int sw_exchange(Switch s, int v);            // store v (the caller has validated it); returns the previous value
// the shape of a switch's own setter: store v where the setter accepts it, only query otherwise; returns the previous value
inline int sw_set_or_query(Switch s, bool accepted, int v) { return accepted ? sw_exchange(s, v) : sw_get(s); }

}  // namespace dg
