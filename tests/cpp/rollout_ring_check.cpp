// tests/cpp/rollout_ring_check.cpp -- the staging ring's arithmetic (smarties_amd/csrc/rollout_ring.h) against a brute-force restatement
// that keeps an owner per row: random episode tables, capacities from 2 maxSteps up.  Built with the address and undefined-behaviour
// sanitizers by tests/test_rollout_staged_cpu.py; prints "rollout_ring_check: ok".
#include "../../smarties_amd/csrc/rollout_ring.h"

#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(x) do { if (!(x)) { std::printf("rollout_ring_check: %s fails at line %d (capacity %lld, call %d)\n", #x, __LINE__, (long long)capacity, call); std::exit(1); } } while (0)

int main() {
  std::mt19937_64 gen(20240917);
  long long nBatches = 0, nWraps = 0, nReleased = 0, nCalls = 0;
  for (int trial = 0; trial < 120; ++trial) {
    const int maxSteps = 2 + (int)(gen() % 30);
    // the lower bound itself, one above it, odd sizes, rings of many episodes
    const int64_t capacity = trial % 4 == 0 ? 2 * maxSteps : trial % 4 == 1 ? 2 * maxSteps + 1 : 2 * maxSteps + (int64_t)(gen() % (40 * maxSteps));
    hl::RolloutRing ring; ring.capacity = capacity;
    std::vector<int> owner((size_t)capacity, -1);      // brute force: the region that owns each row (-1: free)
    int64_t head = 0, wraps = 0, myWraps = 0;
    int nextRegion = 0, oldestLive = 0;
    long long nextEpisode = 0;
    int call = 0;
    for (; call < 30; ++call) {
      const int nEnded = (int)(gen() % 201);      // up to 200 ended episodes per call
      std::vector<int32_t> ns((size_t)nEnded);
      for (int32_t& x : ns) x = 2 + (int32_t)(gen() % (maxSteps - 1));      // 2 .. maxSteps
      ++nCalls;
      for (int k0 = 0; k0 < nEnded;) {
        int64_t rows = 0;
        const int m = hl::ringBatch(ns.data() + k0, nEnded - k0, capacity, &rows);
        // the batch: at least one episode, the two bounds, and the LONGEST such prefix
        CHECK(m >= 1 && m <= 64 && m <= nEnded - k0);
        int64_t sum = 0; for (int k = 0; k < m; ++k) sum += ns[(size_t)(k0 + k)];
        CHECK(sum == rows && rows <= capacity / 2);
        CHECK(k0 + m == nEnded || m == 64 || rows + ns[(size_t)(k0 + m)] > capacity / 2);
        // the placement, restated: at the head where it fits, else at row 0
        const bool wantWrap = head + rows > capacity;
        const int64_t wantBegin = wantWrap ? 0 : head;
        bool wrapped = false; std::vector<hl::RingRegion> released;
        const int64_t begin = ring.place(rows, nextRegion, &wrapped, &released);
        CHECK(begin == wantBegin && wrapped == wantWrap && begin >= 0 && begin + rows <= capacity);
        head = wantBegin + rows; wraps += wantWrap ? 1 : 0; myWraps += wrapped ? 1 : 0;
        // first in, first out: the released regions are the oldest live ones, in order
        for (const hl::RingRegion& g : released) {
          CHECK(g.event == oldestLive); ++oldestLive; ++nReleased;
          for (int64_t i = g.begin; i < g.begin + g.rows; ++i) { CHECK(owner[(size_t)i] == g.event); owner[(size_t)i] = -1; }
        }
        // no row of the new region belongs to a region that was not released
        for (int64_t i = begin; i < begin + rows; ++i) { CHECK(owner[(size_t)i] == -1); owner[(size_t)i] = nextRegion; }
        // every live region of the ring owns exactly its rows; they are the ones not yet released, oldest first
        CHECK((int)ring.live.size() == nextRegion + 1 - oldestLive);
        for (size_t j = 0; j < ring.live.size(); ++j) {
          const hl::RingRegion& g = ring.live[j];
          CHECK(g.event == oldestLive + (int)j);
          for (int64_t i = g.begin; i < g.begin + g.rows; ++i) CHECK(owner[(size_t)i] == g.event);
        }
        long long owned = 0; for (int o : owner) owned += o >= 0;
        long long liveRows = 0; for (const hl::RingRegion& g : ring.live) liveRows += g.rows;
        CHECK(owned == liveRows);
        // every episode once, in order: episode k of the batch at the rows behind the ones before it
        int64_t at = begin;
        for (int k = 0; k < m; ++k) { CHECK(at + ns[(size_t)(k0 + k)] <= begin + rows); at += ns[(size_t)(k0 + k)]; ++nextEpisode; }
        CHECK(at == begin + rows);
        ++nextRegion; ++nBatches;
        k0 += m;
      }
      CHECK(ring.head == head);
    }
    CHECK(wraps == myWraps);
    nWraps += wraps;
  }
  // the table of tests/test_hip_rollout_staged.py's order test: 70 episodes of 2 states on 96 rows
  {
    const int64_t capacity = 96; const int call = 0;
    std::vector<int32_t> ns(70, 2);
    hl::RolloutRing ring; ring.capacity = capacity;
    int sizes[3] = {0, 0, 0}, nb = 0, w = 0; int64_t total = 0;
    for (int k0 = 0; k0 < 70;) {
      int64_t rows = 0; bool wrapped = false; std::vector<hl::RingRegion> rel;
      const int m = hl::ringBatch(ns.data() + k0, 70 - k0, capacity, &rows);
      CHECK(nb < 3);
      ring.place(rows, nb, &wrapped, &rel);
      sizes[nb++] = m; w += wrapped; total += rows; k0 += m;
    }
    CHECK(nb == 3 && sizes[0] == 24 && sizes[1] == 24 && sizes[2] == 22 && total == 140 && w == 1);
  }
  std::printf("rollout_ring_check: ok (%lld calls, %lld batches, %lld wraps, %lld regions released)\n", nCalls, nBatches, nWraps, nReleased);
  return 0;
}
