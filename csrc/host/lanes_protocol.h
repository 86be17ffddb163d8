// The host protocol of the asynchronous lanes (SSP / ASP), once: everything the
// loops of LanesLoop::run_async and run_async_remote (csrc/runtime/lanes_loop.h)
// decide, and none of how it reaches the GPU.
//
// Reference: the worker side of ServerProcessor.java:143-183 -- which worker may
// start, with which clock and weights (MessageTracker.java:47-87), what it trains
// on (WorkerSamplingProcessor.java:50-113), which rows its delta logs
// (ServerProcessor.java:154-165) -- plus the budgets, the stream-driven cadence,
// injected crashes / clean leaves, the deadline and the watchdogs.
//
// No HIP here: the tracker, the windows, the metrics sink and the control queues
// are driven through the host runtime's C ABI (capi.h), the persistent launch
// through the hooks of AsyncLanesPlane.  LanesLoop implements the hooks (pinned
// records, events, the transport) and launches / drains around the two loops;
// csrc/tests/host_selftest.cc pins the protocol with a scripted plane and clock.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../kernels/lanes_records.h"
#include "capi.h"
#include "shard_feed.h"

namespace psx {

// The host-side part of the lanes configuration (LanesLoopCfg adds the device part).
struct LanesHostCfg {
  // producer: worker k of N reads dataset rows k, k + N, ... (`epochs` passes)
  int64_t ds_rows = 0;
  int N = 1;              // logical workers in the whole job
  int per_iter_rows = 0;  // > 0: rows per round; 0: the producer clock p_ms
  double p_ms = 0.0;
  int64_t epochs = 1;
  double t0_ms = 0.0;
  // lanes of this process
  int L = 0;
  std::vector<int> k;             // worker ids
  std::vector<uintptr_t> window;  // SlidingWindow*
  uintptr_t sink = 0;       // MetricsSink* (0: no rows)
  bool log_server = true;   // server rows on this rank
  bool log_workers = true;  // worker rows on this rank
  uintptr_t tracker = 0;    // VectorClockTracker* (0: none)
  uintptr_t api = 0;        // HostApi*
  // stream-driven cadence (the CLI's --iter_new_rows / --iter_new_frac / --iter_new_cap,
  // psx/runtime/config.py:new_tuples_needed): a round starts once every lane saw at
  // least max(new_rows, min(ceil(new_frac * window), new_cap)) new tuples since its
  // last solve (or its stream ended); 0 / 0.0: every round solves at once
  int new_rows = 0;
  double new_frac = 0.0;
  int new_cap = 0;
  // ... capped at new_ramp << (the lane's completed solves) for its first solves (0: off)
  int new_ramp = 0;
  // asynchronous consistency (run_async): the worker whose deltas produce the
  // server rows (ServerProcessor.java:154: worker 0, or the lowest live one;
  // -1: none) and injected straggler delays per lane (us, tests / fault injection)
  int log_worker = 0;
  std::vector<int> delay_us;

  // new tuples a window of `size` rows waits for (0: no cadence); updates < 0: no ramp
  int64_t new_tuples_needed(int64_t size, int64_t updates = -1) const {
    int64_t k = (int64_t)std::ceil(new_frac * (double)size);  // as math.ceil in config.py
    if (k < 0) k = 0;
    if (new_cap > 0 && k > new_cap) k = new_cap;
    if (new_ramp > 0 && updates >= 0 && updates < 30) {  // the first solves come early
      const int64_t r = (int64_t)new_ramp << updates;
      if (k > r) k = r;
    }
    return k > new_rows ? k : new_rows;
  }
};

// What the protocol needs of the persistent launch and of the machine (the clocks and the
// idle sleep: HostClock).
class AsyncLanesPlane : public HostClock {
 public:
  // lane `lane`'s release record number `tag` (its count of records so far)
  virtual void write_release(int lane, const RelRec& q, unsigned tag) = 0;
  // the token ring's slot of ticket n (the token is there once its tag == (unsigned)n)
  virtual AsyncToken read_token(uint64_t n) = 0;
  // throws when a lane reported a device error
  virtual void poll_errors() = 0;
  // (failure messages) how far the persistent launch got
  virtual std::string progress_report() = 0;
  // remote over a host transport only: receive the server's weights into lane l's slot;
  // have they landed; send lane l's delta to the server
  virtual void begin_pull(int lane) = 0;
  virtual bool pull_done(int lane) = 0;
  virtual void send_delta(int lane) = 0;
};

class AsyncLanesProtocol {
 public:
  enum LaneState {
    kIdle = 0,      // no release due
    kWant = 1,      // released by the tracker (or its pull landed): starts once its rows allow
    kRunning = 2,   // a release record written, its token not seen yet
    kWaitPull = 3,  // remote: waits for the server's reply token
    kPulling = 4,   // remote, host transport: its weights are on the way
    kDone = 5,      // remote: sent its FINAL delta
    kGone = 6,      // its worker crashed or left: stopped, never starts again
  };
  // the release that a lane's running solve was started with
  struct RunRec {
    int64_t vc = 0, nseen = 0;
    int slot_w = -1, slot_s = -1;
    uint64_t seq_w = 0, seq_s = 0;
    int64_t snap = 0;  // the pulled snapshot's ticket
    LaneRound r{};     // the window + new rows of the release
  };

  // Once, before the first run.  cfg stays the caller's (the sink and log_worker change
  // between runs; lane_leave writes log_worker back); peer: releases carry the lane's pull
  // tag; feeds: every lane's producer, the caller's (its BSP loop delivers from them too).
  void bind(LanesHostCfg* cfg, bool peer, AsyncLanesPlane* plane, std::vector<ShardFeed>* feeds) {
    cfg_ = cfg;
    api_ = reinterpret_cast<const HostApi*>(cfg->api);
    peer_ = peer;
    plane_ = plane;
    feeds_ = feeds;
    const int L = cfg->L;
    relc_.assign(L, 0);
    pend_r_.assign(L, LaneRound{});
    state_.assign(L, kIdle);
    want_vc_.assign(L, 0);
    runrec_.assign(L, RunRec{});
    lane_stopped_.assign(L, 0);
    pull_tag_.assign(L, 0u);
    lane_of_.assign(cfg->N, -1);
    for (int l = 0; l < L; ++l) lane_of_.at(cfg->k[l]) = l;
  }

  // ---- stop records: one per lane per launch ----
  void on_launch() { lane_stopped_.assign(cfg_->L, 0); }
  void stop_lane(int l) {
    if (lane_stopped_[l]) return;  // (an unread second stop record would end the lane's next launch at once)
    RelRec q;
    std::memset(&q, 0, sizeof(q));
    q.stop = 1;
    plane_->write_release(l, q, (unsigned)(++relc_[l]));
    lane_stopped_[l] = 1;
  }
  void stop_lanes() {
    for (int l = 0; l < cfg_->L; ++l) stop_lane(l);
  }

  // ---- the in-process loop (run_async): before the launch, then with it running ----
  // Where this run starts: the lanes the tracker has dispatched (bootstrap: all, vc 0,
  // MessageTracker.java:47-53), the others wait for a release.
  void begin_local(double max_wait_s) {
    const int L = cfg_->L;
    void* trk = reinterpret_cast<void*>(cfg_->tracker);
    log_lane_ = (cfg_->log_worker >= 0 && cfg_->log_worker < cfg_->N) ? lane_of_[cfg_->log_worker] : -1;
    for (int l = 0; l < L; ++l) {
      // a worker the tracker retired (it crashed or left in an earlier call: its `sent` bit
      // stays set) never starts again -- its lane stays gone and gets a stop record at the end
      const int live = api().tracker_is_live(trk, cfg_->k[l]);
      check(live, "tracker state");
      const int sent = api().tracker_is_sent(trk, cfg_->k[l]);
      check(sent, "tracker state");
      state_[l] = !live ? kGone : (sent ? kWant : kIdle);
      want_vc_[l] = api().tracker_clock(trk, cfg_->k[l]);
      check(want_vc_[l], "tracker clock");
    }
    // the lanes' release waits (the device) and the row-starved waits below are idle waits:
    // bounded by the idle limit, not by the in-flight watchdog max_wait_s
    rel_wait_s_ = std::max(max_wait_s, idle_wait_s_);
    // fault injection of this run (set_injection), consumed here
    crash_ = std::move(inj_crash_);
    stop_ = std::move(inj_stop_);
    inj_crash_.clear();
    inj_stop_.clear();
    crashed_.clear();
    left_.clear();
  }
  // Consume tokens in ticket order until `updates` solves ran, the streams ended or the
  // deadline passed; returns the updates applied.  lane_budget[l]: the most solves lane l
  // starts (empty: no per-lane bound).
  int64_t run_local(int64_t updates, double max_wait_s, double deadline_ms, const std::vector<int64_t>& lane_budget) {
    const int L = cfg_->L;
    void* trk = reinterpret_cast<void*>(cfg_->tracker);
    updates_ = updates;
    budget_ = &lane_budget;
    started_ = done_ = 0;
    lane_started_.assign((size_t)L, 0);
    running_ = 0;
    stopping_ = updates <= 0;
    ks_.resize((size_t)cfg_->N);
    vs_.resize((size_t)cfg_->N);
    double wait0 = plane_->now_ms();
    start_ready(plane_->now_ms() - cfg_->t0_ms);
    uint64_t next = aticket_ + 1;
    int64_t idle_spins = 0;
    for (;;) {
      const AsyncToken tk = plane_->read_token(next);
      if (tk.tag == (unsigned)next) {
        const int64_t tk0 = plane_->mono_ns();
        int64_t vc = 0;
        const int l = take_token(tk, &next, &vc, true);
        // the rows of the iteration: server row first (ServerProcessor.java:154-165), then the worker row
        const RunRec& rr = runrec_[l];
        if (log_on_)
          alog_.push_back({(int64_t)aticket_, l, cfg_->k[l], vc, rr.snap, rr.r.B, rr.r.start, rr.r.first, rr.r.step,
                           rr.r.n, rr.r.first2, rr.r.n2});
        SinkRecord rec[2];
        int nr = 0;
        if (rr.slot_s >= 0) rec[nr++] = SinkRecord{rr.slot_s, 1 | kSinkTagged, rr.seq_s, -1, -1, vc, 0};
        if (rr.slot_w >= 0) rec[nr++] = SinkRecord{rr.slot_w, kSinkTagged, rr.seq_w, -1, cfg_->k[l], vc, rr.nseen};
        if (nr) check(api().sink_submit_many(reinterpret_cast<void*>(cfg_->sink), nr, rec), "metrics sink submit");
        state_[l] = kIdle;
        const int n = api().tracker_on_delta(trk, cfg_->k[l], vc, ks_.data(), vs_.data(), cfg_->N);
        check(n, "tracker");
        want_released(n);
        if (!stop_.empty() && stop_[l] >= 0 && lane_started_[l] >= stop_[l]) lane_leave(l, false);
        if (deadline_ms > 0.0 && plane_->now_ms() >= deadline_ms) stopping_ = true;
        start_ready(plane_->now_ms() - cfg_->t0_ms);
        idle_spins = 0;
        wait0 = plane_->now_ms();
        ++tok_n_;
        tok_ns_ += (double)(plane_->mono_ns() - tk0);
        continue;
      }
      if (running_ > 0) {  // solves in flight: spin for their tokens
        if ((++idle_spins & 1023) == 0) {
          plane_->poll_errors();
          const double now = plane_->now_ms();
          if (deadline_ms > 0.0 && now >= deadline_ms) stopping_ = true;
          if (now - wait0 > max_wait_s * 1000.0)
            throw std::runtime_error("LanesLoop: no delta from the device for " + std::to_string(max_wait_s) + " s");
        } else {
          cpu_relax();
        }
        continue;
      }
      // nothing in flight: is the run over?
      if (stopping_ || started_ >= updates_) break;
      bool any_want = false, end = false;
      for (int l = 0; l < L; ++l)
        if (state_[l] == kWant && !at_budget(l)) {
          if (window_empty(l) && exhausted(l)) end = true;  // a worker with no rows left: the run ends
          any_want = true;
        }
      if (end || !any_want) break;
      const double now = plane_->now_ms();
      if (deadline_ms > 0.0 && now >= deadline_ms) break;
      start_ready(now - cfg_->t0_ms);  // every dispatched lane waits for rows (producer clock / cadence)
      if (running_ == 0) {
        if (now - wait0 > idle_wait_s_ * 1000.0) throw std::runtime_error("LanesLoop: no rows for a worker");
        plane_->idle_sleep(200);
      } else {
        wait0 = plane_->now_ms();
      }
    }
    return done_;
  }

  // ---- the worker-rank loop of multi-rank SSP / ASP (run_async_remote) ----
  void begin_remote(double max_wait_s) {
    for (int l = 0; l < cfg_->L; ++l) state_[l] = kWaitPull;  // the server's begin() sends everybody its clock
    rel_wait_s_ = std::max(max_wait_s, idle_wait_s_);
  }
  // Answer the server's reply tokens (queue `reply`: which worker the next weights are
  // for) by pulling the weights and releasing the lane; forward every lane's token to
  // the server (queue `ctrl`: worker, vc, aux = tuples seen, FINAL on the lane's last
  // solve) behind its delta.  peer: the lanes move weights and deltas themselves (the
  // peer data plane), else through begin_pull / pull_done / send_delta.  Returns the
  // solves run (every lane's FINAL token sent).
  int64_t run_remote(bool peer, uintptr_t ctrl, uintptr_t reply, int64_t iters, double max_wait_s,
                     double deadline_ms) {
    const int L = cfg_->L;
    std::vector<int64_t> it(L, 0);
    done_ = 0;
    running_ = 0;
    int finished = 0;
    void* rq = reinterpret_cast<void*>(reply);
    void* cq = reinterpret_cast<void*>(ctrl);
    double wait0 = plane_->now_ms();
    uint64_t next = aticket_ + 1;
    int64_t spins = 0;
    while (finished < L || running_ > 0) {
      bool progress = false;
      // the server's releases, in its send order to this rank
      CtrlToken rt{};
      while (api().ctrl_pop(rq, &rt, 0.0) == 1) {
        const int j = rt.worker >= 0 && rt.worker < cfg_->N ? lane_of_[rt.worker] : -1;
        if (j < 0 || state_[j] != kWaitPull)
          throw std::logic_error("LanesLoop: reply for worker " + std::to_string(rt.worker) + " not waiting");
        want_vc_[j] = rt.vc;
        progress = true;
        if (peer) {  // the server GPU writes the weights into slot j itself: the lane waits for tag aux
          pull_tag_[j] = (unsigned)rt.aux;
          state_[j] = kWant;
          continue;
        }
        plane_->begin_pull(j);
        state_[j] = kPulling;
      }
      const double now = plane_->now_ms();
      for (int l = 0; l < L; ++l) {
        if (state_[l] == kPulling && plane_->pull_done(l)) state_[l] = kWant;
        if (state_[l] == kWant && try_release(l, want_vc_[l], now - cfg_->t0_ms, l)) {
          state_[l] = kRunning;
          ++running_;
          progress = true;
        }
      }
      // the lanes' pushes, in their push (ticket) order
      const AsyncToken tk = plane_->read_token(next);
      if (tk.tag == (unsigned)next) {
        int64_t vc = 0;
        const int l = take_token(tk, &next, &vc, false);
        const bool fin = ++it[l] >= iters || (deadline_ms > 0.0 && now >= deadline_ms) ||
                         (exhausted(l) && window_empty(l));
        // push: the delta to the server, then its token (WorkerTrainingProcessor.java:95-97);
        // peer data plane: the lane already wrote it into the server's inbox (tagged)
        if (!peer) plane_->send_delta(l);
        CtrlToken ct{};
        ct.worker = cfg_->k[l];
        ct.kind = fin ? 1 : 0;
        ct.vc = vc;
        ct.aux = runrec_[l].nseen;
        if (api().ctrl_push(cq, &ct, max_wait_s) != 1) throw std::runtime_error("LanesLoop: control queue full");
        const RunRec& rr = runrec_[l];
        if (rr.slot_w >= 0) {
          SinkRecord rec{rr.slot_w, kSinkTagged, rr.seq_w, -1, cfg_->k[l], vc, rr.nseen};
          check(api().sink_submit_many(reinterpret_cast<void*>(cfg_->sink), 1, &rec), "metrics sink submit");
        }
        state_[l] = fin ? kDone : kWaitPull;
        finished += fin ? 1 : 0;
        progress = true;
      }
      if (progress) {
        wait0 = plane_->now_ms();
        spins = 0;
        continue;
      }
      if ((++spins & 1023) == 0) {
        plane_->poll_errors();
        if (plane_->now_ms() - wait0 > max_wait_s * 1000.0) {
          std::string m = "LanesLoop: no progress with the server for " + std::to_string(max_wait_s) +
                          " s; lanes (state 1 want / 2 running / 3 wait pull / 4 pulling / 5 done, vc, pull tag):";
          for (int l = 0; l < L; ++l)
            m += " [" + std::to_string(state_[l]) + " " + std::to_string((long long)want_vc_[l]) + " " +
                 std::to_string(peer ? pull_tag_[l] : 0u) + " it " + std::to_string((long long)it[l]) + "]";
          m += "; tokens pushed " + std::to_string((long long)done_) + "; " + plane_->progress_report();
          throw std::runtime_error(m);
        }
        if (running_ == 0) plane_->idle_sleep(100);
      } else {
        cpu_relax();
      }
    }
    return done_;
  }

  // Fault injection for the next run_local: crash[l] >= 0 -- lane l fails when released
  // after crash[l] more solves (`drop`: the tracker retires its worker and the run goes
  // on, else the run stops at once); stop[l] >= 0 -- lane l leaves cleanly after stop[l]
  // more solves.  Empty: none; else one entry per lane.
  void set_injection(const std::vector<int64_t>& crash, const std::vector<int64_t>& stop, bool drop) {
    inj_crash_ = crash;
    inj_stop_ = stop;
    inj_drop_ = drop;
  }
  const std::vector<int>& crashed() const { return crashed_; }  // workers, in the last run_local
  const std::vector<int>& left() const { return left_; }
  // idle waits (a row-starved stream, a lane waiting for its release): this bound, never
  // below the in-flight watchdog max_wait_s
  void set_idle_wait(double s) { idle_wait_s_ = s > 0.0 ? s : 600.0; }
  double rel_wait_s() const { return rel_wait_s_; }  // the lanes' wait budget of the current run (device)
  int log_lane() const { return log_lane_; }
  int state(int lane) const { return state_.at(lane); }
  uint64_t tickets() const { return aticket_; }  // last ticket applied (device counter mirror)
  // a host log per applied ticket of what the release that solved it carried: {ticket, lane,
  // worker, vc, snapshot ticket, B, start, first, step, n, first2, n2}
  void set_log(bool on) { log_on_ = on; }
  const std::vector<std::vector<int64_t>>& log() const { return alog_; }
  // a whole call (launch to drain) served `updates`
  void account(int64_t updates, double ns) {
    async_updates_ += updates;
    async_ns_ += ns;
  }
  double host_us_per_update() const { return async_updates_ ? async_ns_ / 1000.0 / (double)async_updates_ : 0.0; }
  // host time spent per consumed token (token seen -> its rows handed over, tracker, the
  // releases it triggers written): the host loop's share of an asynchronous update
  double host_busy_us_per_token() const { return tok_n_ ? tok_ns_ / 1000.0 / (double)tok_n_ : 0.0; }

 private:
  const HostApi& api() const { return *api_; }
  void check(int64_t rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string("LanesLoop: ") + what + ": " + api().last_error());
  }
  static void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
  }
  ShardFeed& feed(int lane) const { return (*feeds_)[lane]; }
  bool exhausted(int lane) const { return feed(lane).exhausted(); }
  bool window_empty(int l) const { return feed(l).window().size <= 0; }
  bool at_budget(int l) const { return !budget_->empty() && lane_started_[l] >= (*budget_)[l]; }

  // the pending new rows of a lane as <= 2 contiguous runs (LaneRound n / n2)
  static void drop_front(LaneRound& r, int64_t d, int64_t cap) {
    while (d > 0 && r.n > 0) {
      const int64_t k = d < r.n ? d : r.n;
      r.first += k * r.step;
      r.dst = (int)((r.dst + k) % cap);
      r.n -= (int)k;
      d -= k;
      if (r.n == 0 && r.n2 > 0) {
        r.first = r.first2;
        r.n = r.n2;
        r.n2 = 0;
      }
    }
  }
  static void append_run(LaneRound& r, long long src_first, long long step, int64_t slot, int64_t run, int64_t cap) {
    if (r.n == 0) {
      r.first = src_first;
      r.step = step;
      r.n = (int)run;
      r.dst = (int)slot;
      r.n2 = 0;
      return;
    }
    if ((r.dst + r.n + r.n2) % cap != slot)
      throw std::logic_error("LanesLoop: ring slots of a delivery not contiguous");
    if (r.n2 == 0 && src_first == r.first + (long long)r.n * r.step)
      r.n += (int)run;
    else if (r.n2 > 0 && src_first == r.first2 + (long long)r.n2 * r.step)
      r.n2 += (int)run;
    else if (r.n2 == 0) {
      r.first2 = src_first;
      r.n2 = (int)run;
    } else {
      throw std::logic_error("LanesLoop: pending rows of a release span three runs");
    }
  }

  // Deliver lane `lane`'s due rows into its window (WorkerSamplingProcessor.java:50-113
  // through the host runtime's SlidingWindow) and add them to the lane's pending runs.
  int64_t poll_async(int lane, double now_ms) {
    LaneRound& r = pend_r_[lane];
    const int64_t cap = feed(lane).cap();
    return feed(lane).deliver(
        now_ms,
        [&](int64_t keep) {  // rows the ring overwrites before the next solve
          const int64_t tot = (int64_t)r.n + r.n2 + keep;
          if (tot > cap) drop_front(r, tot - cap, cap);
        },
        [&](int64_t src_first, int64_t step, int64_t run, int64_t slot) {
          append_run(r, src_first, step, slot, run, cap);
        });
  }

  // Start lane `lane` at clock vc if the cadence lets it go: its release record (window,
  // pending rows, snapshot, the metrics slots of its rows).  snap < 0: the weights right
  // after the latest applied update; remote: the lane's receive slot.
  bool try_release(int lane, int64_t vc, double now_ms, int64_t snap = -1) {
    poll_async(lane, now_ms);
    const ShardFeed::Window v = feed(lane).window();
    // (vc: the worker's completed pushes)
    if (!feed(lane).solve_due(v, cfg_->new_tuples_needed(v.size, vc))) return false;
    feed(lane).mark_solved(v.seen);
    RelRec q;
    std::memset(&q, 0, sizeof(q));
    q.vc = vc;
    q.snap = snap >= 0 ? (long long)snap : (long long)aticket_;
    q.r = pend_r_[lane];
    q.r.B = (int)v.size;
    q.r.start = (int)v.start;
    if (q.r.n == 0) q.r.step = cfg_->N;
    pend_r_[lane] = LaneRound{};
    RunRec& rr = runrec_[lane];
    rr = RunRec{};
    rr.vc = vc;
    rr.nseen = v.seen;
    rr.snap = q.snap;
    rr.r = q.r;
    if (cfg_->sink) {
      const bool w = cfg_->log_workers, sv = cfg_->log_server && lane == log_lane_;
      const int n = (w ? 1 : 0) + (sv ? 1 : 0);
      if (n) {
        int sl[2];
        uint64_t sq[2];
        uintptr_t ad[2];
        check(api().sink_acquire_many(reinterpret_cast<void*>(cfg_->sink), n, sl, sq, ad), "metrics sink acquire");
        int i = 0;
        if (w) {
          rr.slot_w = sl[i];
          rr.seq_w = sq[i];
          q.slot_w = ad[i];
          q.seq_w = (unsigned)sq[i];
          ++i;
        }
        if (sv) {
          rr.slot_s = sl[i];
          rr.seq_s = sq[i];
          q.slot_s = ad[i];
          q.seq_s = (unsigned)sq[i];
        }
      }
    }
    q.delay_us = lane < (int)cfg_->delay_us.size() ? cfg_->delay_us[lane] : 0;
    q.pull_tag = peer_ ? pull_tag_[lane] : 0u;
    plane_->write_release(lane, q, (unsigned)(++relc_[lane]));
    return true;
  }

  // The token of ticket *next, validated against its lane's running release: the ticket is
  // applied, the lane no longer running.  Returns the lane, its clock in *vc.
  int take_token(const AsyncToken& tk, uint64_t* next, int64_t* vc, bool local) {
    const int l = (int)tk.a;
    *vc = (int64_t)(((uint64_t)tk.c << 32) | tk.b);
    if (l < 0 || l >= cfg_->L || state_[l] != kRunning || runrec_[l].vc != *vc)
      throw std::logic_error("LanesLoop: unexpected token (lane " + std::to_string(l) +
                             (local ? ", vc " + std::to_string((long long)*vc) : std::string()) + ")");
    aticket_ = (*next)++;
    --running_;
    ++done_;
    return l;
  }

  // the first n entries of the tracker's release list (ks_, vs_): those workers' lanes want
  // the weights of that clock
  void want_released(int n) {
    for (int i = 0; i < n; ++i) {
      const int j = ks_[i] >= 0 && ks_[i] < cfg_->N ? lane_of_[ks_[i]] : -1;
      if (j < 0) throw std::logic_error("LanesLoop: the tracker released a worker this loop does not host");
      if (state_[j] == kGone) continue;
      state_[j] = kWant;
      want_vc_[j] = vs_[i];
    }
  }
  // a lane whose worker crashed / left: it gets its stop record now (its workgroups
  // leave the launch), the tracker retires the worker (the others are no longer held
  // back by its clock) and the lanes that releases are dispatched
  void lane_leave(int l, bool crashed) {
    const int k = cfg_->k[l];
    state_[l] = kGone;
    stop_lane(l);
    (crashed ? crashed_ : left_).push_back(k);
    if (crashed && !inj_drop_) {  // --on_worker_failure fail: the run ends here
      stopping_ = true;
      return;
    }
    if (l == log_lane_) {  // server rows follow the lowest surviving worker's deltas
      int nl = -1;
      for (int j = 0; j < cfg_->L; ++j)
        if (state_[j] != kGone && (nl < 0 || cfg_->k[j] < cfg_->k[nl])) nl = j;
      log_lane_ = nl;
      if (nl >= 0) cfg_->log_worker = cfg_->k[nl];
    }
    const int n =
        api().tracker_retire(reinterpret_cast<void*>(cfg_->tracker), k, ks_.data(), vs_.data(), cfg_->N);
    check(n, "tracker retire");
    want_released(n);
  }
  void start_ready(double now) {
    for (int l = 0; l < cfg_->L; ++l) {
      if (state_[l] != kWant || stopping_ || started_ >= updates_) continue;
      if (!crash_.empty() && crash_[l] >= 0 && lane_started_[l] >= crash_[l]) {
        lane_leave(l, true);  // released, and fails before its solve (roles.py WorkerRole.compute)
        l = -1;               // (a retirement may have released a lane already passed)
        continue;
      }
      if (at_budget(l)) continue;
      if (try_release(l, want_vc_[l], now)) {
        state_[l] = kRunning;
        ++started_;
        ++lane_started_[l];
        ++running_;
      }
    }
  }

  LanesHostCfg* cfg_ = nullptr;
  const HostApi* api_ = nullptr;
  AsyncLanesPlane* plane_ = nullptr;
  bool peer_ = false;
  std::vector<ShardFeed>* feeds_ = nullptr;
  uint64_t aticket_ = 0;                // last ticket applied
  std::vector<uint64_t> relc_;          // release records written per lane
  std::vector<LaneRound> pend_r_;       // new stream rows not yet in the lane's ring
  std::vector<int> state_;              // LaneState
  std::vector<int64_t> want_vc_;
  std::vector<RunRec> runrec_;
  std::vector<uint8_t> lane_stopped_;   // lanes already sent their stop record (this launch)
  std::vector<int> lane_of_;            // worker id -> lane (-1: not on this loop)
  int log_lane_ = -1;
  std::vector<unsigned> pull_tag_;      // peer data plane: the pull tag of each lane's pending release
  std::vector<int64_t> inj_crash_, inj_stop_;  // set_injection (consumed by the next run_local)
  bool inj_drop_ = true;
  std::vector<int> crashed_, left_;
  double rel_wait_s_ = 60.0;
  double idle_wait_s_ = 600.0;
  bool log_on_ = false;
  std::vector<std::vector<int64_t>> alog_;
  // the current run
  int64_t updates_ = 0, started_ = 0, done_ = 0;
  int running_ = 0;
  bool stopping_ = false;
  const std::vector<int64_t>* budget_ = nullptr;
  std::vector<int64_t> lane_started_, crash_, stop_;
  std::vector<int> ks_;
  std::vector<int64_t> vs_;
  int64_t async_updates_ = 0, tok_n_ = 0;
  double async_ns_ = 0.0, tok_ns_ = 0.0;
};

}  // namespace psx
