// smarties_amd/csrc/act_host.h -- the host arithmetic of rollout inference (learner_act.h) that needs no device: the layout of a staged chunk in a pinned
// block, the rows of appended observations, the tables of a chunk of ragged windows.  Plain pointers and ints only: tests/cpp/act_host_check.cpp runs it on the CPU
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

// One staged chunk of `cap` rows or agents: [outputs, nOut doubles each | inputs, inFloats floats | nDone completion stamps], the inputs on a multiple of
// 16 bytes where cap is even (actconv.hip's row loads); a chunk of windows (`tables`) keeps its small regions together in front of the inputs:
// [outputs | nDone stamps | cap + 2 window offsets | cap state counts | inputs]
struct ActCarve { size_t out, in, done, off, cnt, bytes; };      // byte offsets from the chunk's start; bytes: its end
inline ActCarve act_carve(size_t cap, size_t nOut, size_t inFloats, size_t nDone, bool tables) {
  ActCarve c{};
  const size_t outEnd = cap * nOut * sizeof(double), inBytes = inFloats * sizeof(float);
  c.done = tables ? outEnd : outEnd + inBytes;
  c.off = c.done + nDone * sizeof(unsigned);
  c.cnt = c.off + (tables ? cap + 2 : 0) * sizeof(int);
  c.in = tables ? c.cnt + cap * sizeof(int) : outEnd;
  c.bytes = tables ? c.in + inBytes : c.cnt;
  return c;
}
struct ActStage { double* out; float* in; volatile unsigned* done; int* off; int* cnt; };
inline ActStage act_stage(unsigned char* base, const ActCarve& c) {
  return ActStage{reinterpret_cast<double*>(base + c.out), reinterpret_cast<float*>(base + c.in), reinterpret_cast<volatile unsigned*>(base + c.done),
                  reinterpret_cast<int*>(base + c.off), reinterpret_cast<int*>(base + c.cnt)};
}

// the network's input row of step t with nApp appended observations: the state of step t followed by those of t-1 .. t-nApp
// (Episode::standardizedState, Episode.h:172-183); steps before the first given state repeat it.  dst: (1 + nApp) dS floats
inline void act_stack_row(float* dst, const float* st, int t, int nApp, int dS) {
  for (int j = 0; j <= nApp; ++j) std::memcpy(dst + (size_t)j * dS, st + (size_t)std::max(t - j, 0) * dS, (size_t)dS * sizeof(float));
}
// the K stacked rows of a window of nSteps given states: the last win = min(nSteps, recWin) steps are the window's, the ctx = nSteps - win
// in front of them only feed appended observations; rows win .. K - 1 -- steps the window lacks -- repeat its last one
inline void act_stack_window(float* dst, const float* st, int nSteps, int recWin, int K, int nApp, int dS) {
  const int win = std::min(nSteps, recWin), ctx = nSteps - win;
  const size_t dIn = (size_t)dS * (1 + nApp);
  for (int k = 0; k < win; ++k) act_stack_row(dst + k * dIn, st, ctx + k, nApp, dS);
  for (int k = win; k < K; ++k) std::memcpy(dst + k * dIn, dst + (win - 1) * dIn, dIn * sizeof(float));
}
// m windows back to back: off[i] = states in front of window i, off[m] = *sum = all of them (act_seq_kernel reads off[i + 1]),
// cnt[i] = its states, *winMax = the longest window, none beyond recWin steps
inline void act_chunk_tables(const int32_t* nSteps, int m, int recWin, int* off, int* cnt, int* sum, int* winMax) {
  int s = 0, w = 0;
  for (int i = 0; i < m; ++i) { off[i] = s; cnt[i] = nSteps[i]; s += nSteps[i]; w = std::max(w, std::min((int)nSteps[i], recWin)); }
  off[m] = s; *sum = s; *winMax = w;
}
