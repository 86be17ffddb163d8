// The server protocol of the asynchronous consistency models (SSP, ASP), once.
//
// Reference: ServerProcessor.java:75-87 (bootstrap: every worker gets the
// weights of its clock) and 143-183 (one partition: a delta is applied, the
// tracker says whom to answer, those workers get the weights).  On top of it:
// a watchdog for workers that hold weights and stay silent, retirement of a
// worker on its final delta or on failure, and a stop every checkpoint_every
// updates.
//
// No HIP here: the tracker and the token queue are driven through the host
// runtime's C ABI (capi.h), the data plane through the hooks below.
// AsyncServer (csrc/runtime/async_server.h: RCCL / host / same-process
// point-to-point) and PeerServer (csrc/runtime/peer_server.h: the persistent
// server kernel over the peer data plane) derive from it and implement only the
// hooks; csrc/tests/host_selftest.cc pins the protocol with a scripted plane.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi.h"

namespace psx {

// CtrlToken::kind of the tokens the workers push (ctrl.h)
constexpr int kKindDelta = 0, kKindFinal = 1, kKindError = 2;

enum AsyncCode : int {
  kAsyncDone = 0,        // every worker sent its final delta (or failed)
  kAsyncErrorToken = 1,  // `worker` reported an error: caller decides (retire via fail(), or abort)
  kAsyncWatchdog = 2,    // `worker` busy and silent longer than the timeout
  kAsyncCheckpoint = 3,  // `updates` reached a multiple of checkpoint_every
};

struct AsyncStatus {
  int code = kAsyncDone;
  int worker = -1;
  int64_t updates = 0;
};

class ServerProtocol {
 public:
  virtual ~ServerProtocol() = default;
  // New run: workers that finished the previous run rejoin (failed ones stay
  // retired), every live worker gets the weights of its current clock (the
  // bootstrap: vc 0 on a fresh tracker).
  void begin() {
    start(true);
    std::fill(finished_.begin(), finished_.end(), 0);
    std::fill(failed_.begin(), failed_.end(), 0);
    std::fill(busy_since_.begin(), busy_since_.end(), -1.0);
    int n = 0;
    for (int j = 0; j < n_; ++j) {
      int live = api().tracker_is_live(tracker_, j);
      check_api(live, "tracker is_live");
      if (!live && !dead_[j]) {  // retired because it finished the previous run: rejoins
        check_api(api().tracker_revive(tracker_, j), "tracker revive");
        live = 1;
      }
      if (!live) {  // failed in an earlier run (or retired in a resumed checkpoint)
        failed_[j] = finished_[j] = dead_[j] = 1;
        continue;
      }
      const int64_t u = api().tracker_clock(tracker_, j);
      if (u > 0) api().tracker_sent(tracker_, j, u);  // a later run resumes at the tracked clocks
      rel_k_[n] = j;
      rel_v_[n] = u;
      ++n;
    }
    answer(-1, 0, n);  // the bootstrap (ServerProcessor.java:75-87)
  }

  // Serve tokens until every worker finished (or a code that needs the caller).
  AsyncStatus run(int64_t checkpoint_every) {
    AsyncStatus st;
    start(false);
    const double poll = timeout_s_ < 1.0 ? timeout_s_ : 1.0;
    for (;;) {
      int open = 0;
      for (int j = 0; j < n_; ++j) open += !finished_[j];
      if (open == 0) break;
      CtrlToken t;
      // pending work of the plane takes the tokens already queued, then goes out
      const bool held = pending();
      const int got = api().ctrl_pop(ctrl_, &t, held ? 0.0 : poll);
      check_api(got, "token pop");
      if (held && !got) {
        flush();
        continue;
      }
      check_plane();
      if (!got) {  // watchdog: a worker holding weights that stays silent has failed
        const double now = now_s();
        for (int j = 0; j < n_; ++j)
          if (!finished_[j] && busy_since_[j] >= 0.0 && now - busy_since_[j] > timeout_s_) {
            st.code = kAsyncWatchdog;
            st.worker = j;
            st.updates = updates_;
            return st;
          }
        continue;
      }
      const auto h0 = std::chrono::steady_clock::now();
      ++tokens_;
      const int k = t.worker;
      if (k < 0 || k >= n_) throw std::runtime_error(name_ + ": token from an unknown worker");
      if (t.kind == kKindError) {
        flush();
        st.code = kAsyncErrorToken;
        st.worker = k;
        st.updates = updates_;
        return st;
      }
      if (finished_[k]) throw std::runtime_error(name_ + ": delta from a finished worker " + std::to_string(k));
      busy_since_[k] = -1.0;
      apply(t);
      on_delta(k, t.vc, t.kind == kKindFinal);
      ++updates_;
      ++updates_run_;
      host_ns_ += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - h0).count();
      if (checkpoint_every > 0 && updates_ % checkpoint_every == 0) {
        end();  // (the caller reads the weights)
        st.code = kAsyncCheckpoint;
        st.updates = updates_;
        return st;
      }
    }
    end();
    st.code = kAsyncDone;
    st.updates = updates_;
    return st;
  }

  // Retire worker k (failed): the tracker stops waiting for it; the workers it
  // held back are answered.
  void fail(int k) {
    if (k < 0 || k >= n_) throw std::out_of_range(name_ + "::fail: worker id");
    start(false);
    failed_[k] = finished_[k] = dead_[k] = 1;
    busy_since_[k] = -1.0;
    const int n = api().tracker_retire(tracker_, k, rel_k_.data(), rel_v_.data(), (int)rel_k_.size());
    check_api(n, "tracker retire");
    if (n) answer(-1, 0, n);
  }

  int64_t updates() const { return updates_; }
  void set_updates(int64_t u) { updates_ = u; }
  int64_t tokens() const { return tokens_; }
  double host_us_per_update() const { return updates_run_ ? host_ns_ / 1000.0 / (double)updates_run_ : 0.0; }
  std::vector<int> failed() const {
    std::vector<int> out;
    for (int j = 0; j < n_; ++j)
      if (failed_[j]) out.push_back(j);
    return out;
  }

 protected:
  // `name` prefixes every error text ("AsyncServer", "PeerServer")
  explicit ServerProtocol(const char* name) : name_(name) {}
  // the host runtime's table and handles (once, from the constructor, after the
  // server validated its configuration)
  void bind(uintptr_t api, uintptr_t tracker, uintptr_t ctrl, int nworkers, double worker_timeout_s) {
    api_ = reinterpret_cast<const HostApi*>(api);
    if (api_->version != kHostApiVersion) throw std::runtime_error(name_ + ": host runtime C ABI version mismatch");
    tracker_ = reinterpret_cast<void*>(tracker);
    ctrl_ = reinterpret_cast<void*>(ctrl);
    n_ = nworkers;
    timeout_s_ = worker_timeout_s;
    finished_.assign(n_, 0);
    failed_.assign(n_, 0);
    dead_.assign(n_, 0);
    busy_since_.assign(n_, -1.0);
    rel_k_.resize(n_ + 1);
    rel_v_.resize(n_ + 1);
  }

  // ---- the data plane ----
  // begin() (new_run), run() and fail() are about to use the plane
  virtual void start(bool new_run) { (void)new_run; }
  // run() returns done or a checkpoint (not before a watchdog / error-token return)
  virtual void end() {}
  // the delta of token t, before the tracker hears of it
  virtual void apply(const CtrlToken& t) = 0;
  // answer the n workers (ks[i], at clock vs[i]) released by worker k's delta at clock vc
  // (k = -1: by the bootstrap or a retirement); none of them has finished
  virtual void release(int k, int64_t vc, const int* ks, const int64_t* vs, int n) = 0;
  // work held back for the tokens already queued; flush() sends it out
  virtual bool pending() const { return false; }
  virtual void flush() {}
  // after every pop: throws when the plane has failed
  virtual void check_plane() {}

  // A delta of worker k at clock vc arrived (applied or about to be, the plane's
  // business): the tracker's releases, plus -- on a final delta -- those of k's
  // retirement (its frozen clock would stall an SSP worker D ahead forever), go out.
  void on_delta(int k, int64_t vc, bool final) {
    int n = api().tracker_on_delta(tracker_, k, vc, rel_k_.data(), rel_v_.data(), (int)rel_k_.size());
    check_api(n, "tracker on_delta");
    if (final) {
      finished_[k] = 1;
      const int m = api().tracker_retire(tracker_, k, rel_k_.data() + n, rel_v_.data() + n, (int)rel_k_.size() - n);
      check_api(m, "tracker retire");
      n += m;
    }
    answer(k, vc, n);
  }
  // every worker is open again without a bootstrap (stand-in workers)
  void reopen() { std::fill(finished_.begin(), finished_.end(), 0); }
  // server rows follow the deltas of worker 0 (ServerProcessor.java:154-165), or of
  // the lowest surviving worker once 0 has failed
  int log_worker() const {
    for (int j = 0; j < n_; ++j)
      if (!failed_[j]) return j;
    return -1;
  }
  const HostApi& api() const { return *api_; }
  void check_api(int rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(name_ + ": " + what + ": " + api_->last_error());
  }
  static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  }

 private:
  // the first n entries of the release list, less the finished workers, are busy from
  // now on and go to the plane
  void answer(int k, int64_t vc, int n) {
    const double t = now_s();
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const int j = rel_k_[i];
      if (j < 0 || j >= n_) throw std::logic_error(name_ + ": release of an unknown worker");
      if (finished_[j]) continue;
      busy_since_[j] = t;
      rel_k_[m] = j;
      rel_v_[m] = rel_v_[i];
      ++m;
    }
    release(k, vc, rel_k_.data(), rel_v_.data(), m);
  }

  const std::string name_;
  const HostApi* api_ = nullptr;
  void* tracker_ = nullptr;
  void* ctrl_ = nullptr;
  int n_ = 0;
  double timeout_s_ = 600.0;
  std::vector<uint8_t> finished_, failed_;  // this run
  std::vector<uint8_t> dead_;               // failed in any run: never revived
  std::vector<double> busy_since_;          // < 0: not busy (weights not sent / delta back)
  std::vector<int> rel_k_;
  std::vector<int64_t> rel_v_;
  int64_t updates_ = 0, tokens_ = 0, updates_run_ = 0;
  double host_ns_ = 0.0;
};

}  // namespace psx
