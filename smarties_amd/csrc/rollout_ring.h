// smarties_amd/csrc/rollout_ring.h -- the arithmetic of the rollout's staging ring (include/smarties_hip_rollout.h: hl_rollout_staging), host
// only and free of HIP types, so that tests/cpp/rollout_ring_check.cpp drives it on the CPU.
//
// The ring has `capacity` rows.  The ended episodes of a call leave their slabs in BATCHES: a batch is the longest prefix of the episodes
// left that holds at most RING_BATCH_EP episodes (one ingest launch) and at most capacity / 2 rows; capacity >= 2 maxSteps, so one episode
// always fits.  A batch takes one contiguous REGION at the head; one that does not fit between the head and the ring's end starts again at
// row 0 (a wrap: the rows behind the head stay unused this time round).  Regions are released first in, first out: a new region releases
// every older one up to the newest whose rows it covers -- their readers run in that order on one stream, so the newest one's event stands
// for all of them -- and the caller makes the writer wait for the events of the released regions that have not completed.  A region is at
// most half the ring, so it never meets itself.
#pragma once
#include <cstddef>
#include <cstdint>
#include <deque>
#include <vector>

namespace hl {

constexpr int RING_BATCH_EP = 64;      // == INGEST_DEV_MAX_EP (learner_rollout.h asserts it)

// the episodes of the next batch: the longest prefix of nsteps[0 .. left) within the two bounds; *rows: the rows it holds
inline int ringBatch(const int32_t* nsteps, int left, int64_t capacity, int64_t* rows) {
  int m = 0; int64_t sum = 0;
  while (m < left && m < RING_BATCH_EP && sum + nsteps[m] <= capacity / 2) sum += nsteps[m++];
  *rows = sum;
  return m;
}

struct RingRegion { int64_t begin, rows; int event; };      // event: the caller's handle of the region's `consumed` event

struct RolloutRing {
  int64_t capacity = 0, head = 0;
  std::deque<RingRegion> live;      // oldest first

  // a region of `rows` rows (1 .. capacity / 2) that carries `event`: where it begins; *wrapped: it started again at row 0; `released`
  // receives, oldest first, the regions whose rows it takes over
  int64_t place(int64_t rows, int event, bool* wrapped, std::vector<RingRegion>* released) {
    *wrapped = head + rows > capacity;
    const int64_t begin = *wrapped ? 0 : head, end = begin + rows;
    released->clear();
    std::size_t last = 0;      // one past the newest live region the new one covers
    for (std::size_t i = 0; i < live.size(); ++i)
      if (live[i].begin < end && begin < live[i].begin + live[i].rows) last = i + 1;
    for (std::size_t i = 0; i < last; ++i) { released->push_back(live.front()); live.pop_front(); }
    live.push_back(RingRegion{begin, rows, event});
    head = end;
    return begin;
  }
};

}  // namespace hl
