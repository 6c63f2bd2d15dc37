// Drives run_frame_batches (csrc/frame_batches.h), the slot rotation of the frame entries, with recording callables.
// test_frame_batches.py compiles it plain and with -fsanitize=address,undefined and runs it:
//   frame_batches_driver            every check for the (num_frames, batch) pairs below; prints one line per pair, exit code 0 or 1
#include <cstdio>
#include <vector>
#include "frame_batches.h"

namespace {

struct Call { bool enqueue; int slot, first, num; };

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// One run.  fail_enqueue / fail_complete: the 1-based call of that kind that returns `code` (0: none fails).
int run(int num_frames, int batch, int fail_enqueue, int fail_complete, int code, std::vector<Call>* calls) {
  int enqueues = 0, completes = 0;
  return oicc::run_frame_batches(
      num_frames, batch,
      [&](int slot, int first, int num) { calls->push_back(Call{true, slot, first, num}); return ++enqueues == fail_enqueue ? code : 0; },
      [&](int slot, int first, int num) { calls->push_back(Call{false, slot, first, num}); return ++completes == fail_complete ? code : 0; });
}

// What holds for every run, failed or not, as far as it got.  Returns the number of batches enqueued.
int check_order(int num_frames, int batch, const std::vector<Call>& calls, const char* what) {
  const int eff = batch < num_frames ? batch : num_frames;
  int next_frame = 0, in_flight = 0, max_in_flight = 0, enq = 0, done = 0;
  bool busy[2] = {false, false};
  std::vector<Call> queue;      // enqueued, not yet completed
  for (const Call& c : calls) {
    CHECK(c.slot == 0 || c.slot == 1, "%s: slot %d", what, c.slot);
    if (c.slot != 0 && c.slot != 1) return enq;
    if (c.enqueue) {
      CHECK(c.first == next_frame, "%s: batch starts at %d, expected %d", what, c.first, next_frame);      // ascending, no gap, no repeat
      CHECK(c.num >= 1 && c.num <= eff && c.first + c.num <= num_frames, "%s: batch [%d, +%d)", what, c.first, c.num);
      CHECK(c.num == eff || c.first + c.num == num_frames, "%s: a short batch [%d, +%d) that is not the last", what, c.first, c.num);
      CHECK(!busy[c.slot], "%s: slot %d enqueued before its own completion", what, c.slot);
      busy[c.slot] = true;
      next_frame = c.first + c.num;
      queue.push_back(c);
      ++enq; ++in_flight;
      if (in_flight > max_in_flight) max_in_flight = in_flight;
    } else {
      CHECK(size_t(done) < queue.size(), "%s: a completion with nothing in flight", what);
      if (size_t(done) >= queue.size()) return enq;
      const Call& f = queue[size_t(done)];      // batches complete in the order they were enqueued
      CHECK(f.slot == c.slot && f.first == c.first && f.num == c.num, "%s: completion (%d, %d, %d) out of order", what, c.slot, c.first, c.num);
      CHECK(busy[c.slot], "%s: slot %d completed twice", what, c.slot);
      busy[c.slot] = false;
      ++done; --in_flight;
    }
    if (num_frames <= batch) CHECK(c.slot == 0, "%s: slot 1 touched though one batch covers all frames", what);
  }
  CHECK(max_in_flight <= 2, "%s: %d batches in flight", what, max_in_flight);
  return enq;
}

void check_pair(int num_frames, int batch) {
  char what[64];
  std::snprintf(what, sizeof(what), "(%d, %d)", num_frames, batch);
  const int eff = batch < num_frames ? batch : num_frames;
  const int batches = (num_frames + eff - 1) / eff;
  std::vector<Call> calls;
  CHECK(run(num_frames, batch, 0, 0, 0, &calls) == 0, "%s", what);
  CHECK(check_order(num_frames, batch, calls, what) == batches, "%s: batches", what);
  CHECK(int(calls.size()) == 2 * batches, "%s: %d calls, expected %d", what, int(calls.size()), 2 * batches);      // every batch completed
  int frames = 0;
  for (const Call& c : calls) if (c.enqueue) frames += c.num;
  CHECK(frames == num_frames, "%s: %d frames enqueued", what, frames);
  // the n-th enqueue / the n-th completion fails: its code comes back, it is the last call, and what ran before it kept the order
  for (int kind = 0; kind < 2; ++kind)
    for (int nth = 1; nth <= batches; ++nth) {
      std::snprintf(what, sizeof(what), "(%d, %d) %s %d fails", num_frames, batch, kind == 0 ? "enqueue" : "complete", nth);
      const int code = -3 - nth;
      calls.clear();
      CHECK(run(num_frames, batch, kind == 0 ? nth : 0, kind == 1 ? nth : 0, code, &calls) == code, "%s: code", what);
      check_order(num_frames, batch, calls, what);
      int seen = 0;
      for (const Call& c : calls) seen += c.enqueue == (kind == 0);
      CHECK(seen == nth && !calls.empty() && calls.back().enqueue == (kind == 0), "%s: %d calls of the kind, the failing one not last", what, seen);
    }
  std::printf("pair %d %d batches %d\n", num_frames, batch, batches);
}

}  // namespace

int main() {
  const int pairs[][2] = {{1, 1}, {1, 4}, {2, 1}, {3, 1}, {3, 3}, {4, 2}, {5, 2}, {7, 3}};
  for (const auto& p : pairs) check_pair(p[0], p[1]);
  std::printf("failures %d\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
