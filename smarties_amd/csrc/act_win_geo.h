// smarties_amd/csrc/act_win_geo.h -- the window of one agent of the device window calls (include/smarties_hip_dev.h), written once for the kernel that
// gathers it (rectm.hip: lstm_tm_prepare_acts_dev_kernel) and for the CPU (tests/cpp/act_wide_geo_check.cpp).  Plain ints only, beside act_host.h
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define ACT_GEO_HD __host__ __device__
#else
#define ACT_GEO_HD
#endif

// An agent gives len = dNSteps[i] states from row dFirstRow[i] on, recWin = nnBPTTseq + 1, nApp = nAppendedObs:
//   ns    states read: the newest recWin + nApp of them, one where len < 1
//   skip  older states left out in front of them
//   win   steps of the recurrent window: the newest recWin of the ns
//   ctx   states in front of the window, which only feed appended observations
struct ActWinGeo { int ns, skip, win, ctx; };
ACT_GEO_HD inline ActWinGeo act_win_geo(int len, int recWin, int nApp) {
  ActWinGeo g;
  const int top = recWin + nApp, have = len < top ? len : top;
  g.ns = have > 1 ? have : 1;
  g.skip = (len > 1 ? len : 1) - g.ns;
  g.win = g.ns < recWin ? g.ns : recWin;
  g.ctx = g.ns - g.win;
  return g;
}
// the state (0 = oldest of the ns) whose component e % dS is element e of the stacked input [dS (1 + nApp)] of window step k: the step's own
// state followed by the ones before it, steps before the first state read repeating it (act_stack_row)
ACT_GEO_HD inline int act_win_state(const ActWinGeo& g, int k, int e, int dS) {
  const int s = g.ctx + k - e / dS;
  return s > 0 ? s : 0;
}
// ... and its row of the caller's [rows][dS] array, in 64 bits
ACT_GEO_HD inline long long act_win_row(const ActWinGeo& g, long long firstRow, long long rowStride, int s) {
  return firstRow + (long long)(g.skip + s) * rowStride;
}
