// The slot rotation of the entries that stream frames through the device in batches (camera_maps.hip, rolling_shutter.hip,
// board.hip): two staging slots, so that one batch's copies and kernels overlap the other's.  No HIP here, so that
// tests/frame_batches_driver.cpp can drive it with recording callables.
#pragma once
#include <algorithm>

namespace oicc {

// a second staging slot only when a second batch exists
inline int frame_batch_slots(int num_frames, int batch) { return num_frames > batch ? 2 : 1; }

// enqueue(slot, first, num): queue the frames [first, first + num) on the slot (asynchronous).
// complete(slot, first, num): wait for that batch and take its results; the slot is free afterwards.
// Batches are enqueued in ascending frame order and complete in that order, alternating between the slots; at most two are in
// flight, and a slot takes its next batch right after its own completion.  Returns the first non-zero code of either callable
// and calls neither again after it.  batch >= 1.
template <class Enqueue, class Complete>
int run_frame_batches(int num_frames, int batch, Enqueue&& enqueue, Complete&& complete) {
  batch = std::min(batch, std::max(num_frames, 1));
  const int nslots = frame_batch_slots(num_frames, batch);
  struct { int first, num; } in_flight[2] = {{0, 0}, {0, 0}};
  int next = 0;
  auto push = [&](int q) -> int {
    in_flight[q].first = next; in_flight[q].num = std::min(batch, num_frames - next);
    next += in_flight[q].num;
    return enqueue(q, in_flight[q].first, in_flight[q].num);
  };
  for (int q = 0; q < nslots && next < num_frames; ++q)
    if (const int rc = push(q)) return rc;
  for (int k = 0; in_flight[k % nslots].num > 0; ++k) {
    const int q = k % nslots;
    if (const int rc = complete(q, in_flight[q].first, in_flight[q].num)) return rc;
    in_flight[q].num = 0;
    if (next < num_frames)
      if (const int rc = push(q)) return rc;
  }
  return 0;
}

}  // namespace oicc
