// The producer side of a round, once: which rows of a worker's dataset shard are
// due, where they land in its ring, how a delivery that wraps the shard's epoch
// is split (ShardFeed) -- and the wait in front of a BSP round (RoundGate).
//
// Reference: WorkerSamplingProcessor.java:50-113 through the host runtime's
// SlidingWindow.  Worker k of N reads dataset rows k, k + N, ... `epochs` times
// over; a delivery is the rows due now (per_iter_rows per call, or the producer
// clock's due_rows), inserted into the window, of which the last `cap` survive
// in the ring.  What a loop does with a contiguous run of them -- a launch, a
// slot in its round kernel's arguments, a pending release -- is the loop's.
//
// No HIP here: BspLoop, KeyRangeLoop, LanesLoop (csrc/runtime) and
// AsyncLanesProtocol (lanes_protocol.h) call this; csrc/tests/host_selftest.cc
// pins it with real windows and a scripted clock.
#pragma once
#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "capi.h"

namespace psx {

// Wall clock (epoch ms: the producer clock and the deadlines), a steady clock, idle sleep.
class HostClock {
 public:
  virtual ~HostClock() = default;
  virtual double now_ms() {
    using namespace std::chrono;
    return (double)duration_cast<microseconds>(system_clock::now().time_since_epoch()).count() / 1000.0;
  }
  virtual int64_t mono_ns() {
    using namespace std::chrono;
    return duration_cast<nanoseconds>(steady_clock::now().time_since_epoch()).count();
  }
  virtual void idle_sleep(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }
};

class ShardFeed {
 public:
  struct Cfg {
    int k = 0, N = 1;
    int64_t ds_rows = 0, epochs = 1;
    int per_iter_rows = 0;  // > 0: rows per delivery; 0: the producer clock p_ms
    double p_ms = 0.0;
    uintptr_t window = 0;  // SlidingWindow*
    int64_t cap = 0;       // rows of the worker's ring
    const HostApi* api = nullptr;
    const char* who = "";  // prefix of the error messages ("BspLoop: ")
  };
  struct Window {
    int64_t size = 0, start = 0, seen = 0;
  };

  ShardFeed() = default;
  explicit ShardFeed(const Cfg& c)
      : c_(c), local_total_(c.N > 0 && c.ds_rows > c.k ? (c.ds_rows - c.k + c.N - 1) / c.N : 0) {}

  int64_t local_total() const { return local_total_; }  // rows of the shard (0: the worker has none)
  int64_t cap() const { return c_.cap; }
  int64_t next_local() const { return next_local_; }  // the producer cursor: local rows delivered so far
  void set_next_local(int64_t v) { next_local_ = v; }
  // tuples seen when the worker's last solve started (the cadence's origin)
  int64_t seen_at_solve() const { return seen_at_solve_; }
  void set_seen_at_solve(int64_t v) { seen_at_solve_ = v; }
  bool exhausted() const { return next_local_ >= local_total_ * c_.epochs; }

  // Deliver the rows due at now_ms (producer time) into the window.  before(keep) once
  // if any are, keep = the rows that survive in the ring; then on_run(src_first, step,
  // n, slot) for each contiguous run of those (dataset rows src_first, src_first +
  // step, ... into ring slots slot, slot + 1, ... modulo cap; a run ends at the shard's
  // epoch boundary).  Returns the rows delivered.
  template <class Before, class OnRun>
  int64_t deliver(double now_ms, Before&& before, OnRun&& on_run) {
    if (exhausted()) return 0;
    const int64_t lt = local_total_;
    const int64_t limit = lt * c_.epochs - next_local_;
    int64_t n;
    if (c_.per_iter_rows > 0) {
      n = c_.per_iter_rows < limit ? c_.per_iter_rows : limit;
      times_.assign((size_t)n, now_ms);
    } else {
      const int64_t cur = next_local_ % lt;
      int64_t mx = limit < lt - cur ? limit : lt - cur;
      if (mx > (int64_t(1) << 22)) mx = int64_t(1) << 22;
      times_.resize(mx > 0 ? (size_t)mx : 1);
      n = c_.api->due_rows(c_.k, c_.N, c_.p_ms, c_.ds_rows, cur, now_ms, mx, times_.data());
      check(n, "due_rows");
    }
    if (n <= 0) return 0;
    const int64_t first = c_.api->window_insert_many(reinterpret_cast<void*>(c_.window), times_.data(), n);
    check(first, "window insert");
    const int64_t cap = c_.cap;
    const int64_t keep = n < cap ? n : cap;  // only the last cap rows can survive in the window
    const int64_t skip = n - keep;
    before(keep);
    int64_t slot = (first + skip) % cap, pos = next_local_ + skip, remaining = keep;
    while (remaining > 0) {  // split at the shard's epoch boundaries
      const int64_t cur = pos % lt;
      const int64_t run = remaining < lt - cur ? remaining : lt - cur;
      on_run(c_.k + cur * (int64_t)c_.N, (int64_t)c_.N, run, slot);
      slot = (slot + run) % cap;
      pos += run;
      remaining -= run;
    }
    next_local_ += n;
    return n;
  }
  template <class OnRun>
  int64_t deliver(double now_ms, OnRun&& on_run) {
    return deliver(now_ms, [](int64_t) {}, on_run);
  }

  Window window() const {
    Window v;
    check(c_.api->window_state(reinterpret_cast<void*>(c_.window), &v.size, &v.start, &v.seen), "window state");
    return v;
  }
  // The cadence: a window with rows solves once it saw `need` new tuples since its last
  // solve (need <= 0: at once) or nothing more will come.
  bool solve_due(const Window& v, int64_t need) const {
    return v.size > 0 && (need <= 0 || v.seen - seen_at_solve_ >= need || exhausted());
  }
  void mark_solved(int64_t seen) { seen_at_solve_ = seen; }

 private:
  void check(int64_t rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string(c_.who) + what + ": " + c_.api->last_error());
  }
  Cfg c_;
  int64_t local_total_ = 0, next_local_ = 0, seen_at_solve_ = 0;
  std::vector<double> times_;  // arrival stamps of one delivery
};

// The wait in front of a BSP round: deliver and look at every lane's window until each
// has rows and its cadence lets it solve.
struct RoundGate {
  HostClock* clock = nullptr;
  double t0_ms = 0.0;        // producer start (epoch ms): deliveries get the time since
  double max_wait_s = 0.0;   // how long a lane may have no rows at all ...
  const char* starved = "";  // ... before this is thrown
  double deadline_ms = 0.0;  // > 0 (epoch ms): the run ends when a round still waits then

  // deliver(now_ms): the caller's delivery for every lane; need(size): new tuples a
  // window of `size` rows waits for.  True: the round runs on views[0..L); false: the
  // run ends (a lane with an empty window and nothing left to come, or the deadline).
  template <class Deliver, class Need>
  bool wait(ShardFeed* feeds, int L, ShardFeed::Window* views, Deliver&& deliver, Need&& need) const {
    const double wait0 = clock->now_ms();
    for (;;) {
      deliver(clock->now_ms() - t0_ms);
      bool ready = true, rows = true, end = false;
      for (int l = 0; l < L; ++l) {
        views[l] = feeds[l].window();
        rows &= views[l].size > 0;
        ready &= feeds[l].solve_due(views[l], need(views[l].size));
        end |= views[l].size <= 0 && feeds[l].exhausted();
      }
      if (ready) return true;
      if (end || (deadline_ms > 0.0 && clock->now_ms() >= deadline_ms)) return false;
      // (only while some lane has no rows at all, not while waiting for the cadence)
      if (!rows && clock->now_ms() - wait0 > max_wait_s * 1000.0) throw std::runtime_error(starved);
      clock->idle_sleep(500);
    }
  }
  // no cadence: a window with rows solves at once
  template <class Deliver>
  bool wait(ShardFeed* feeds, int L, ShardFeed::Window* views, Deliver&& deliver) const {
    return wait(feeds, L, views, deliver, [](int64_t) { return int64_t(0); });
  }
};

}  // namespace psx
