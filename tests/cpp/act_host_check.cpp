// tests/cpp/act_host_check.cpp -- the host arithmetic of rollout inference (smarties_amd/csrc/act_host.h) against a naive re-statement of
// its contract, on the CPU.  tests/test_act_host_cpu.py builds this with the address and undefined-behaviour sanitizers and runs it: every
// buffer below lives on the heap at exactly the size its caller in learner_act.h gives it, so an index one past its end is reported.
// The expectations are written per output float from the wording of include/smarties_hip_act.h -- "steps before the first given state
// repeating it", "the rows of steps a window lacks repeating its last one" --, not from the helpers' own loops.
#include "../../smarties_amd/csrc/act_host.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a heap array of exactly n elements (n may be 0)
template <typename T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }
// state s, component i of a window: every float distinct
static float stateValue(int s, int i) { return 100.f * (s + 1) + i; }
static std::unique_ptr<float[]> window(int nSteps, int dS) {
  auto st = exact<float>((size_t)nSteps * dS);
  for (int s = 0; s < nSteps; ++s) for (int i = 0; i < dS; ++i) st[(size_t)s * dS + i] = stateValue(s, i);
  return st;
}
// float f of the input row of step t: the row is the state of step t, then of t - 1, ... t - nApp; a step before the first given state is the first
static float rowValue(int t, int f, int dS) {
  const int back = f / dS, comp = f % dS;
  const int step = t - back;
  return stateValue(step < 0 ? 0 : step, comp);
}

static void checkStackRow() {
  const int dS = 3;
  for (int nApp : {0, 2}) for (int t : {0, 1, nApp, nApp + 3}) {
    const int dIn = dS * (1 + nApp);
    auto st = window(t + 1, dS);      // the caller holds the states up to step t
    auto dst = exact<float>(dIn);
    for (int f = 0; f < dIn; ++f) dst[f] = -1.f;
    act_stack_row(dst.get(), st.get(), t, nApp, dS);
    for (int f = 0; f < dIn; ++f) CHECK(dst[f] == rowValue(t, f, dS), "act_stack_row nApp %d t %d float %d: %g, expected %g", nApp, t, f, dst[f], rowValue(t, f, dS));
  }
}

static void checkStackWindow() {
  const int dS = 3, recWin = 3;
  for (int nApp : {0, 2}) for (int nSteps : {1, 2, 3, 3 + nApp, 2 + nApp}) for (int padded : {1, 0}) {
    const int dIn = dS * (1 + nApp);
    const int win = nSteps < recWin ? nSteps : recWin;      // the window: the last recWin of the given steps, or all of them
    const int K = padded ? 3 : win;                         // the conv chain's recK rows per agent / hl_forward_sequence's win rows
    auto st = window(nSteps, dS);
    auto dst = exact<float>((size_t)K * dIn);
    for (int f = 0; f < K * dIn; ++f) dst[f] = -1.f;
    act_stack_window(dst.get(), st.get(), nSteps, recWin, K, nApp, dS);
    for (int k = 0; k < K; ++k) {
      const int stepOfWindow = k < win ? k : win - 1;       // a row of a step the window lacks repeats its last one
      const int t = (nSteps - win) + stepOfWindow;          // ... which is this one of the given steps
      for (int f = 0; f < dIn; ++f)
        CHECK(dst[(size_t)k * dIn + f] == rowValue(t, f, dS), "act_stack_window nApp %d nSteps %d K %d row %d float %d: %g, expected %g", nApp, nSteps, K, k, f,
              dst[(size_t)k * dIn + f], rowValue(t, f, dS));
    }
  }
}

static void checkChunkTables() {
  const int32_t lens[7] = {1, 2, 4, 3, 1, 4, 2};
  const int n = 7, cap = 3, recWin = 3;
  auto off = exact<int>(cap + 2);      // the chunk stage's tables: cap + 2 offsets, cap counts
  auto cnt = exact<int>(cap);
  long long first = 0;                 // as the chunk driver keeps it: states in front of the chunk
  for (int i0 = 0; i0 < n; i0 += cap) {
    const int m = n - i0 < cap ? n - i0 : cap;
    int sum = -1, winMax = -1;
    act_chunk_tables(lens + i0, m, recWin, off.get(), cnt.get(), &sum, &winMax);
    long long before = 0; for (int i = 0; i < i0; ++i) before += lens[i];
    CHECK(first == before, "chunk at %d: its states start at %lld, %lld states lie in front of it", i0, first, before);
    int longest = 0, all = 0;
    for (int i = 0; i < m; ++i) {
      int inFront = 0; for (int j = i0; j < i0 + i; ++j) inFront += lens[j];
      CHECK(off[i] == inFront, "chunk at %d: off[%d] = %d, expected %d", i0, i, off[i], inFront);
      CHECK(cnt[i] == lens[i0 + i], "chunk at %d: cnt[%d] = %d, expected %d", i0, i, cnt[i], lens[i0 + i]);
      const int w = lens[i0 + i] < recWin ? lens[i0 + i] : recWin;
      if (w > longest) longest = w;
      all += lens[i0 + i];
    }
    CHECK(off[m] == all, "chunk at %d: the closing off[%d] = %d, expected %d", i0, m, off[m], all);
    CHECK(sum == all && winMax == longest, "chunk at %d: sum %d winMax %d, expected %d %d", i0, sum, winMax, all, longest);
    first += sum;
  }
}

// one carve: every region written over its whole length inside a heap block of exactly c.bytes, aligned for its type, none overlapping another
static void checkCarve(const char* what, size_t cap, size_t nOut, size_t inFloats, size_t nDone, bool tables, size_t allocationBytes) {
  const ActCarve c = act_carve(cap, nOut, inFloats, nDone, tables);
  CHECK(c.bytes == allocationBytes, "%s cap %zu nOut %zu: the carve ends at %zu, the block has %zu bytes", what, cap, nOut, c.bytes, allocationBytes);
  auto block = exact<unsigned char>(c.bytes);      // (operator new[]: aligned for every type here, as the pinned blocks are and the chunk stage's multiple of 256)
  const ActStage s = act_stage(block.get(), c);
  CHECK((uintptr_t)s.out % alignof(double) == 0 && (uintptr_t)s.in % alignof(float) == 0 && (uintptr_t)s.done % alignof(unsigned) == 0 &&
        (uintptr_t)s.off % alignof(int) == 0 && (uintptr_t)s.cnt % alignof(int) == 0, "%s cap %zu nOut %zu: a region is not aligned for its type", what, cap, nOut);
  const size_t nOff = tables ? cap + 2 : 0, nCnt = tables ? cap : 0;
  for (size_t i = 0; i < cap * nOut; ++i) s.out[i] = 1.0;
  for (size_t i = 0; i < inFloats; ++i) s.in[i] = 2.f;
  for (size_t i = 0; i < nDone; ++i) s.done[i] = 3u;
  for (size_t i = 0; i < nOff; ++i) s.off[i] = 4;
  for (size_t i = 0; i < nCnt; ++i) s.cnt[i] = 5;
  bool intact = true;
  for (size_t i = 0; i < cap * nOut; ++i) intact = intact && s.out[i] == 1.0;
  for (size_t i = 0; i < inFloats; ++i) intact = intact && s.in[i] == 2.f;
  for (size_t i = 0; i < nDone; ++i) intact = intact && s.done[i] == 3u;
  for (size_t i = 0; i < nOff; ++i) intact = intact && s.off[i] == 4;
  for (size_t i = 0; i < nCnt; ++i) intact = intact && s.cnt[i] == 5;
  CHECK(intact, "%s cap %zu nOut %zu: two regions overlap", what, cap, nOut);
}
static void checkCarves() {
  const size_t dS = 3, nApp = 2, recWin = 3, dIn = dS * (1 + nApp), recK = recWin;
  for (size_t cap : {1, 16, 512}) for (size_t nOut : {1, 7}) {
    // the byte counts are those the blocks have had since the routes were added, spelt out: outputs and a stamp per row or agent, ...
    const size_t states = cap * (recWin + nApp) * dS, stacked = cap * recK * dIn, blocks = (cap + 15) / 16;
    checkCarve("rows or a window", cap, nOut, cap * dIn, cap, false, cap * (nOut * sizeof(double) + sizeof(unsigned)) + cap * dIn * sizeof(float));
    checkCarve("windows", cap, nOut, states, cap, true, cap * (nOut * sizeof(double) + sizeof(unsigned)) + (2 * cap + 2) * sizeof(int) + states * sizeof(float));
    checkCarve("stacked windows", cap, nOut, stacked, cap, true, cap * (nOut * sizeof(double) + sizeof(unsigned)) + (2 * cap + 2) * sizeof(int) + stacked * sizeof(float));
    checkCarve("row blocks", cap, nOut, cap * dIn, blocks, false, cap * nOut * sizeof(double) + cap * dIn * sizeof(float) + blocks * sizeof(unsigned));
  }
}

int main() {
  checkStackRow();
  checkStackWindow();
  checkChunkTables();
  checkCarves();
  if (failures) { std::printf("act_host_check: %d failures\n", failures); return 1; }
  std::printf("act_host_check: ok\n");
  return 0;
}
