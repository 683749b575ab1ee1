// switch_threads_check.cc -- a program of its own (make switch_threads_check): the switch table of switches.cc under
// ThreadSanitizer.  Eight threads are released together and each does 10^5 operations on every row -- reads, the generic setter
// with valid and refused values, unknown names, the setters' exchange -- so that the table's first touch (the environment parse)
// is raced by all of them.  Exit status 0 and no report: no data race, and every value read was one some thread had stored or
// the row's initial one.  Host code only: no HIP, nothing of the library beyond switches.cc.
#include "switches.h"
#include <atomic>
#include <stdarg.h>
#include <stdio.h>
#include <thread>
#include <vector>
#include "../../include/dgcnn_hip.h"

namespace dg {
static thread_local char g_err[1024];
void set_error(const char* fmt, ...) {       // api.cc's, which this program does not link
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace dg

namespace {

struct Name {
  const char* name;
  int a, b;                                  // two valid values; the initial one is a third or one of them
  int refused;                               // a value the row's parse would replace (a == refused: the row keeps every value)
};
const Name NAMES[dg::SW_COUNT] = {
    {"DGCNN_KNN_BF16F", 0, 1, 0},
    {"DGCNN_KNN_FORCE_VALU", 0, 1, 2},
    {"DGCNN_KNN_TIGHTEN_EVERY", 2, 8, 3},
    {"DGCNN_KNN_BIG_K_MIN", 20, 40, 99},
    {"DGCNN_KNN_SEED_MIN_N", 0, 4096, 0},
    {"DGCNN_KNN_APPEND", 0, 1, 2},
    {"DGCNN_KNN_APPEND_NPR_LX", 1, 3, 2},
    {"DGCNN_KNN_APPEND_NPR_BIG", 1, 3, 2},
    {"DGCNN_KNN_HIST", 1, 4, 3},
    {"DGCNN_KNN_WIDE_MIN_C", 65, 100, 4},
    {"DGCNN_KNN_GRID", 0, 2, 3},
    {"DGCNN_KNN_GRID_MIN_N", 1024, 2048, 1024},
    {"DGCNN_KNN_MIX_MIN_N", 100, 400, -1},
    {"DGCNN_EDGE_VALU", 0, 1, 2},
    {"DGCNN_GEMM_ARITH", 0, 9, 2},
    {"DGCNN_GEMM_X3_TILE", 128, 448, 64},
    {"DGCNN_EVENT_FLAGS", 2, 0, 2},
};

std::atomic<int> g_go{0};
std::atomic<long> g_bad{0};

void worker(int t, int ops) {
  while (!g_go.load(std::memory_order_acquire)) {
  }
  unsigned r = 12345u + 977u * (unsigned)t;
  for (int i = 0; i < ops; ++i) {
    for (int s = 0; s < dg::SW_COUNT; ++s) {
      const Name& n = NAMES[s];
      r = r * 1664525u + 1013904223u;
      int v = 0;
      switch ((r >> 16) & 7) {
        case 0:
        case 1:
          if (dgcnn_switch_get(n.name, &v) != DGCNN_OK) ++g_bad;
          break;
        case 2:
          if (dgcnn_switch_set(n.name, (r >> 20) & 1 ? n.a : n.b) != DGCNN_OK) ++g_bad;
          break;
        case 3:
          if (n.refused != n.a && dgcnn_switch_set(n.name, n.refused) != DGCNN_EINVAL) ++g_bad;
          break;
        case 4:
          v = dg::sw_exchange((dg::Switch)s, (r >> 20) & 1 ? n.a : n.b);
          break;
        case 5:
          v = dg::sw_set_or_query((dg::Switch)s, (r >> 21) & 1, n.a);
          break;
        case 6:
          v = dg::sw_get((dg::Switch)s);
          break;
        default:
          if (dgcnn_switch_get("DGCNN_NO_SUCH_SWITCH", &v) != DGCNN_EINVAL) ++g_bad;
          v = dg::sw_initial((dg::Switch)s);
          break;
      }
      const int now = dg::sw_get((dg::Switch)s);
      if (now != n.a && now != n.b && now != dg::sw_initial((dg::Switch)s)) ++g_bad;
    }
  }
}

}  // namespace

int main() {
  const int threads = 8, ops = 100000;
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t) pool.emplace_back(worker, t, ops);
  g_go.store(1, std::memory_order_release);  // nothing has touched the table yet: its first touch is raced
  for (std::thread& th : pool) th.join();
  printf("switch_threads_check: %d threads x %d operations x %d rows, %ld inconsistencies\n", threads, ops, (int)dg::SW_COUNT,
         g_bad.load());
  return g_bad.load() == 0 ? 0 : 1;
}
