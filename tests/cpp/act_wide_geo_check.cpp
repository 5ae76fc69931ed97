// tests/cpp/act_wide_geo_check.cpp -- the window geometry of the device window calls (smarties_amd/csrc/act_win_geo.h: the code
// lstm_tm_prepare_acts_dev_kernel runs per agent) on the CPU, against the formula include/smarties_hip_dev.h states and against the rows
// act_stack_window (act_host.h) builds for the host route from the same window.  tests/test_act_wide_dev_cpu.py builds this with the
// address and undefined-behaviour sanitizers and runs it: every buffer lives on the heap at exactly the size of the rows an agent may
// read, so a row computed outside its window is reported.
#include "../../smarties_amd/csrc/act_host.h"
#include "../../smarties_amd/csrc/act_win_geo.h"

#include <cstdio>
#include <memory>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <typename T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

// the header's window rule, and the split of the states read into context and window
static void checkFormula() {
  for (int recWin = 1; recWin <= 5; ++recWin) for (int nApp = 0; nApp <= 3; ++nApp) for (int len = -3; len <= 40; ++len) {
    const ActWinGeo g = act_win_geo(len, recWin, nApp);
    const int ns = std::max(1, std::min(len, recWin + nApp)), skip = std::max(len, 1) - ns;
    CHECK(g.ns == ns && g.skip == skip, "recWin %d nApp %d len %d: ns %d skip %d, the header gives %d %d", recWin, nApp, len, g.ns, g.skip, ns, skip);
    CHECK(g.win == std::min(ns, recWin) && g.ctx == ns - g.win, "recWin %d nApp %d len %d: win %d ctx %d", recWin, nApp, len, g.win, g.ctx);
    CHECK(g.win >= 1 && g.win <= recWin && g.ctx >= 0 && g.ctx <= nApp && g.skip >= 0, "recWin %d nApp %d len %d: out of range", recWin, nApp, len);
    // every state an element may ask for lies among the ns read: rows skip .. skip + ns - 1 of the agent, the newest being its last
    for (int k = 0; k < g.win; ++k) for (int e : {0, nApp}) {
      const int s = act_win_state(g, k, e, 1);
      CHECK(s >= 0 && s < g.ns, "recWin %d nApp %d len %d step %d back %d: state %d of %d", recWin, nApp, len, k, e, s, g.ns);
    }
    CHECK(act_win_state(g, g.win - 1, 0, 1) == g.ns - 1, "recWin %d nApp %d len %d: the last step does not read the newest state", recWin, nApp, len);
    CHECK(act_win_row(g, 7, 3, g.ns - 1) == 7 + 3ll * (std::max(len, 1) - 1), "recWin %d nApp %d len %d: the newest state's row", recWin, nApp, len);
  }
  // rows in 64 bits
  const ActWinGeo g = act_win_geo(3, 3, 0);
  CHECK(act_win_row(g, 1ll << 40, 1ll << 31, 2) == (1ll << 40) + (2ll << 31), "64-bit row arithmetic");
}

// one agent's stacked rows gathered as the kernel gathers them -- element by element through act_win_state / act_win_row -- from a packed
// buffer (row_stride 1) and from column `env` of a [T][nEnv] buffer (row_stride nEnv, first_row = t0 nEnv + env), against act_stack_window
// on the agent's newest ns states laid out back to back
static void checkGather() {
  const int dS = 3, recWin = 3;
  for (int nApp : {0, 2}) for (int len : {-2, 0, 1, 2, 3, 4, 5, 6, 9}) for (int layout = 0; layout < 2; ++layout) {
    const int dIn = dS * (1 + nApp), given = std::max(len, 1);
    const int nEnv = layout ? 3 : 1, env = layout ? 2 : 0, t0 = layout ? 1 : 0;
    const long long stride = nEnv, first = (long long)t0 * nEnv + env;
    // exactly the rows up to the agent's newest state: a row behind it is outside the block
    const size_t rows = (size_t)(first + (long long)(given - 1) * stride + 1);
    auto buf = exact<float>(rows * dS);
    for (size_t i = 0; i < rows * dS; ++i) buf[i] = -7.f;      // cells of other agents
    for (int s = 0; s < given; ++s) for (int i = 0; i < dS; ++i) buf[(size_t)(first + s * stride) * dS + i] = 100.f * (s + 1) + i;
    const ActWinGeo g = act_win_geo(len, recWin, nApp);
    auto newest = exact<float>((size_t)g.ns * dS);
    for (int s = 0; s < g.ns; ++s) for (int i = 0; i < dS; ++i) newest[(size_t)s * dS + i] = 100.f * (given - g.ns + s + 1) + i;
    auto want = exact<float>((size_t)g.win * dIn);
    act_stack_window(want.get(), newest.get(), g.ns, recWin, g.win, nApp, dS);
    for (int k = 0; k < g.win; ++k) for (int e = 0; e < dIn; ++e) {
      const long long row = act_win_row(g, first, stride, act_win_state(g, k, e, dS));
      CHECK(row >= 0 && (size_t)row < rows, "nApp %d len %d layout %d step %d element %d: row %lld of %zu", nApp, len, layout, k, e, row, rows);
      if (row < 0 || (size_t)row >= rows) continue;
      const float got = buf[(size_t)row * dS + e % dS];
      CHECK(got == want[(size_t)k * dIn + e], "nApp %d len %d layout %d step %d element %d: %g, act_stack_window gives %g", nApp, len, layout, k, e, got, want[(size_t)k * dIn + e]);
    }
  }
}

int main() {
  checkFormula();
  checkGather();
  if (failures) { std::printf("act_wide_geo_check: %d failures\n", failures); return 1; }
  std::printf("act_wide_geo_check: ok\n");
  return 0;
}
