// Host-runtime self-test, built with -fsanitize=address,undefined by
// tests/test_host_sanitizers.py (sanitizer builds of the host
// C++; GPU sanitizers are not available on this pool).  Exercises every host
// component with real threads and shared memory:
//   VectorClockTracker (BSP / SSP / ASP golden cases),
//   SlidingWindow + RateEstimator (cases I/II/III, ring wrap),
//   CtrlQueue (POSIX-shm MPSC: 4 producer threads, 1 consumer),
//   csv_probe / csv_load (header detection, multithreaded parse, bf16),
//   CsvLogger + MetricsSink (producer thread publishing EvalSlots),
//   tracker fault handling (retire / bsp_round),
//   libsvm_save / libsvm_load round trip (multithreaded mmap parser),
//   ServerProtocol (the SSP / ASP server loop of AsyncServer and PeerServer) over a
//   real tracker and token queue with a scripted data plane,
//   AsyncLanesProtocol (the host logic of LanesLoop::run_async / run_async_remote) over
//   a real tracker, real windows, a real metrics sink and real token queues with a
//   scripted plane (release records, tokens) and a scripted clock,
//   ShardFeed + RoundGate (the producer feed and the BSP round wait of the native loops)
//   over real windows with a scripted clock,
//   FitLoop + fit_update_body (the controller loop of the full-batch fitters and their
//   vector update) on a quadratic: every termination reason, stepping, the lifecycle errors.
// Exit status 0 = all checks passed.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../host/ctrl.h"
#include "../host/dataset.h"
#include "../host/lanes_protocol.h"
#include "../host/libsvm.h"
#include "../host/logger.h"
#include "../host/metrics_sink.h"
#include "../host/sampling.h"
#include "../host/server_protocol.h"
#include "../host/tracker.h"
#include "../kernels/dispatch.h"
#include "../solver/fit_loop.h"

using namespace psx;

static int g_fail = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

static void test_tracker() {
  // BSP: nobody is released until every worker's delta for round v arrived.
  VectorClockTracker bsp(3, 0);
  CHECK(bsp.on_delta(0, 0).empty());
  CHECK(bsp.on_delta(1, 0).empty());
  auto rel = bsp.on_delta(2, 0);
  CHECK(rel.size() == 3);
  for (auto& p : rel) CHECK(p.second == 1);
  // ASP: the sender alone is answered, immediately.
  VectorClockTracker asp(2, -1);
  auto r1 = asp.on_delta(1, 0);
  CHECK(r1.size() == 1 && r1[0].first == 1 && r1[0].second == 1);
  // SSP(1): a worker may run ahead of the slowest by the bound only.
  VectorClockTracker ssp(2, 1);
  int64_t v0 = 0;
  int released = 0;
  for (int it = 0; it < 6; ++it) {
    auto r = ssp.on_delta(0, v0);
    released += (int)r.size();
    bool again = false;
    for (auto& p : r)
      if (p.first == 0) again = true, v0 = p.second;
    if (!again) break;
  }
  CHECK(ssp.max_gap() <= 2);
  CHECK(released >= 1);
  // invariant violations are hard errors
  bool threw = false;
  try {
    VectorClockTracker t(2, 0);
    t.received(0, 5);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
}

static void test_tracker_faults() {
  // BSP with 3 workers: 0 and 1 wait for worker 2, which then fails; retiring
  // it releases the two waiting workers with the next version.
  VectorClockTracker bsp(3, 0);
  CHECK(bsp.on_delta(0, 0).empty());
  CHECK(bsp.on_delta(1, 0).empty());
  auto rel = bsp.retire(2);
  CHECK(rel.size() == 2);
  for (auto& p : rel) CHECK(p.first != 2 && p.second == 1);
  CHECK(!bsp.is_live(2) && bsp.num_live() == 2);
  CHECK(bsp.min_clock() == 1);  // the dead worker's clock no longer counts
  // later rounds involve the live workers only
  CHECK(bsp.on_delta(0, 1).empty());
  CHECK(bsp.on_delta(1, 1).size() == 2);
  // SSP(0 slack = 1): a retired straggler stops holding the fast worker back
  VectorClockTracker ssp(2, 1);
  auto r = ssp.on_delta(0, 0);
  CHECK(r.size() == 1 && r[0].second == 1);
  CHECK(ssp.on_delta(0, 1).empty());  // 2 ahead of worker 1 -> held
  auto r2 = ssp.retire(1);
  CHECK(r2.size() == 1 && r2[0].first == 0 && r2[0].second == 2);
  // whole BSP rounds in one call (the collective schedules)
  VectorClockTracker b2(4, 0);
  for (int64_t v = 0; v < 5; ++v) b2.bsp_round(v);
  for (int k = 0; k < 4; ++k) CHECK(b2.clock(k) == 5 && b2.is_sent(k));
  CHECK(b2.max_gap() <= 1);  // same as applying the deltas one by one
}

static void test_libsvm() {
  char path[] = "/tmp/psx_selftest_svm_XXXXXX";
  int fd = mkstemp(path);
  CHECK(fd >= 0);
  close(fd);
  const int64_t rows = 5000;
  std::vector<int64_t> indptr(1, 0);
  std::vector<int32_t> idx;
  std::vector<uint16_t> val;
  std::vector<int32_t> y(rows);
  for (int64_t r = 0; r < rows; ++r) {
    const int n = (int)(r % 7);
    for (int j = 0; j < n; ++j) {
      idx.push_back((int32_t)((r * 131 + j * 977) % 100000 + j));
      val.push_back(f32_to_bf16(0.25f * (float)(j + 1) * ((r & 1) ? -1.f : 1.f)));
    }
    indptr.push_back((int64_t)idx.size());
    y[r] = (int32_t)(r % 5 + 1);
  }
  for (int zb = 0; zb < 2; ++zb) {
    libsvm_save(path, indptr.data(), idx.data(), val.data(), y.data(), rows, zb != 0);
    SparseRows s = libsvm_load(path, zb != 0, 4);
    CHECK((int64_t)s.y.size() == rows && s.indptr == indptr && s.idx == idx && s.val == val && s.y == y);
    int32_t mx = -1;
    for (auto i : idx) mx = i > mx ? i : mx;
    CHECK(s.max_feature == mx);
  }
  unlink(path);
}

static void test_window() {
  SlidingWindow w(2, 8, 100.0, 500, 16);
  std::vector<double> t(40);
  for (int i = 0; i < 40; ++i) t[i] = i;  // 1 ms apart -> target clamps to max
  std::vector<int64_t> slots(40);
  w.insert_many(t.data(), 40, slots.data());
  CHECK(w.size() == 8);
  CHECK(w.head() == 39 % 16);
  CHECK(w.start() == ((39 - 8 + 1) % 16));
  for (int i = 1; i < 40; ++i) CHECK(slots[i] == (slots[i - 1] + 1) % 16);
  CHECK(w.tuples_seen() == 40);
  // slow arrivals shrink the target (case III) down to min
  SlidingWindow s(2, 8, 0.3, 500);
  for (int i = 0; i < 20; ++i) s.insert(i * 60000.0);
  CHECK(s.size() == 2);
  RateEstimator r(4);
  CHECK(std::fabs(r.mean_interarrival_ms() - 1000.0) < 1e-12);
  for (int i = 0; i < 10; ++i) r.arrival(i * 10.0);
  CHECK(std::fabs(r.mean_interarrival_ms() - 10.0) < 1e-12);
}

static void test_ctrl_queue() {
  const std::string name = "/psx_selftest_" + std::to_string(getpid());
  CtrlQueue q(name, 64, true);
  constexpr int kProducers = 4, kPer = 500;
  std::vector<std::thread> th;
  for (int p = 0; p < kProducers; ++p)
    th.emplace_back([&, p] {
      CtrlQueue qp(name, 64, false);
      for (int i = 0; i < kPer; ++i) {
        CtrlToken t{p, 0, i, 0, 0};
        if (!qp.push(t, 10.0)) std::abort();
      }
    });
  std::vector<int64_t> last(kProducers, -1);
  int got = 0;
  while (got < kProducers * kPer) {
    CtrlToken t;
    if (!q.pop(&t, 10.0)) break;
    CHECK(t.worker >= 0 && t.worker < kProducers);
    CHECK(t.vc == last[t.worker] + 1);  // per-producer FIFO
    last[t.worker] = t.vc;
    ++got;
  }
  for (auto& x : th) x.join();
  CHECK(got == kProducers * kPer);
  q.unlink();
}

static void test_csv() {
  char path[] = "/tmp/psx_selftest_XXXXXX";
  int fd = mkstemp(path);
  CHECK(fd >= 0);
  std::string body = "a,b,c,Score\n";
  for (int r = 0; r < 1000; ++r) body += std::to_string(r * 0.5) + ",0," + std::to_string(-r) + "," +
                                         std::to_string(r % 5 + 1) + "\n";
  CHECK(write(fd, body.data(), body.size()) == (ssize_t)body.size());
  close(fd);
  CsvInfo info = csv_probe(path, 0);
  CHECK(info.header && info.rows == 1000 && info.cols == 4);
  const int64_t stride = 8;
  std::vector<float> xf(info.rows * stride, -7.f);
  std::vector<uint16_t> xb(info.rows * stride);
  std::vector<int32_t> y(info.rows);
  csv_load(path, info, -1, stride, xf.data(), xb.data(), y.data(), 4);
  for (int r = 0; r < 1000; ++r) {
    CHECK(xf[r * stride + 0] == (float)(r * 0.5));
    CHECK(xf[r * stride + 2] == (float)(-r));
    CHECK(xf[r * stride + 3] == 0.f);  // padding zeroed
    CHECK(y[r] == r % 5 + 1);
    CHECK(xb[r * stride + 0] == f32_to_bf16(xf[r * stride + 0]));
  }
  unlink(path);
}

static void test_metrics_sink() {
  char path[] = "/tmp/psx_selftest_log_XXXXXX";
  int fd = mkstemp(path);
  close(fd);
  CsvLogger wlog(path, true, true);
  constexpr int kSlots = 3, kRecs = 200;
  std::vector<EvalSlot> slots(kSlots);
  std::memset(slots.data(), 0, sizeof(EvalSlot) * kSlots);
  MetricsSink sink(reinterpret_cast<uintptr_t>(slots.data()), kSlots, 2, &wlog, nullptr, true);
  // the "device": fills slots asynchronously, publishing seq last
  std::atomic<int> produced{0};
  for (int i = 0; i < kRecs; ++i) {
    uint64_t seq = 0;
    const int s = sink.acquire(&seq);
    std::thread([&, s, seq, i] {
      EvalSlot& e = slots[s];
      std::memset(e.conf, 0, sizeof(e.conf));
      e.conf[0] = 3 + (i % 2);  // true 0 -> pred 0
      e.conf[1] = 1;            // true 0 -> pred 1
      e.conf[17] = 4;           // true 1 -> pred 1
      e.loss = 0.5f;
      __atomic_store_n(&e.seq, seq, __ATOMIC_RELEASE);
      produced.fetch_add(1);
    }).detach();
    sink.submit(s, seq, 0, 1000 + i, 0, i, 10 * i);
  }
  CHECK(sink.flush(30.0));
  auto rows = sink.worker_rows();
  CHECK((int)rows.size() == kRecs);
  for (int i = 0; i < kRecs && i < (int)rows.size(); ++i) {
    const double tp0 = 3 + (i % 2), tot = tp0 + 5;
    CHECK(rows[i].vc == i);
    CHECK(std::fabs(rows[i].acc - (tp0 + 4) / tot) < 1e-12);
  }
  while (produced.load() < kRecs) std::this_thread::yield();
  sink.close();
  wlog.close();
  FILE* f = std::fopen(path, "r");
  int lines = 0;
  char buf[512];
  while (f && std::fgets(buf, sizeof buf, f)) ++lines;
  if (f) std::fclose(f);
  CHECK(lines == kRecs + 1);
  unlink(path);
}

// ---- ServerProtocol ---------------------------------------------------------
// Everything the protocol does to the tracker, the token queue and its data plane,
// in order, as one line of words:
//   B / S    plane start (B: of begin(), S: of run() and fail())      E   plane end
//   p / p0   token pop, blocking (<= 1 s poll) / non-blocking         c   plane health check
//   aK@V     plane apply of worker K's delta at clock V               F   plane flush
//   dK@V     tracker on_delta        rK   tracker retire       vK   tracker revive
//   RK@V[..] plane release after worker K's delta at clock V (R-: bootstrap / retirement),
//            [..]: the released workers as J@clock
// The expected lines are the bodies of AsyncServer / PeerServer begin(), run() and fail()
// as they were before the protocol became one class, written out by hand.
static std::vector<std::string>* g_trace = nullptr;
static void say(const std::string& w) {
  if (g_trace) g_trace->push_back(w);
}
static std::string at(int k, int64_t v) { return std::to_string(k) + "@" + std::to_string((long long)v); }

static int traced_pop(void* q, CtrlToken* out, double timeout_s) {
  say(timeout_s == 0.0 ? "p0" : "p");
  return host_api()->ctrl_pop(q, out, timeout_s);
}
static int traced_on_delta(void* t, int k, int64_t v, int* ks, int64_t* vs, int cap) {
  say("d" + at(k, v));
  return host_api()->tracker_on_delta(t, k, v, ks, vs, cap);
}
static int traced_retire(void* t, int k, int* ks, int64_t* vs, int cap) {
  say("r" + std::to_string(k));
  return host_api()->tracker_retire(t, k, ks, vs, cap);
}
static int traced_revive(void* t, int k) {
  say("v" + std::to_string(k));
  return host_api()->tracker_revive(t, k);
}
static const HostApi* traced_api() {
  static HostApi a = [] {
    HostApi x = *host_api();
    x.ctrl_pop = traced_pop;
    x.tracker_on_delta = traced_on_delta;
    x.tracker_retire = traced_retire;
    x.tracker_revive = traced_revive;
    return x;
  }();
  return &a;
}

// The scripted plane.  batching: an applied delta stays pending until a flush (or the
// end of the run), like PeerServer's open batch; otherwise nothing is ever pending,
// like AsyncServer.
class FakeServer : public ServerProtocol {
 public:
  FakeServer(const char* name, VectorClockTracker* t, CtrlQueue* q, int n, double timeout_s, bool batching = false)
      : ServerProtocol(name), batching_(batching) {
    bind(reinterpret_cast<uintptr_t>(traced_api()), reinterpret_cast<uintptr_t>(t), reinterpret_cast<uintptr_t>(q), n,
         timeout_s);
    g_trace = &trace_;
  }
  ~FakeServer() override { g_trace = nullptr; }
  using ServerProtocol::log_worker;
  // the words since the last call
  std::string take() {
    std::string out;
    for (const auto& w : trace_) out += (out.empty() ? "" : " ") + w;
    trace_.clear();
    return out;
  }

 protected:
  void start(bool new_run) override { say(new_run ? "B" : "S"); }
  void end() override {
    held_ = false;
    say("E");
  }
  void apply(const CtrlToken& t) override {
    held_ = batching_;
    say("a" + at(t.worker, t.vc));
  }
  void release(int k, int64_t vc, const int* ks, const int64_t* vs, int n) override {
    std::string w = k < 0 ? "R-[" : "R" + at(k, vc) + "[";
    for (int i = 0; i < n; ++i) w += (i ? "," : "") + at(ks[i], vs[i]);
    say(w + "]");
  }
  bool pending() const override { return held_; }
  void flush() override {
    held_ = false;
    say("F");
  }
  void check_plane() override { say("c"); }

 private:
  bool batching_, held_ = false;
  std::vector<std::string> trace_;
};

#define CHECK_TRACE(srv, want)                                                                        \
  do {                                                                                                \
    const std::string got_ = (srv).take();                                                            \
    if (got_ != (want)) {                                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: trace\n  got  %s\n  want %s\n", __FILE__, __LINE__, got_.c_str(), \
                   std::string(want).c_str());                                                        \
      ++g_fail;                                                                                       \
    }                                                                                                 \
  } while (0)

static void push(CtrlQueue& q, int worker, int kind, int64_t vc) {
  CtrlToken t{};
  t.worker = worker;
  t.kind = kind;
  t.vc = vc;
  if (!q.push(t, 10.0)) std::abort();
}
static bool is_status(const AsyncStatus& st, int code, int worker, int64_t updates) {
  return st.code == code && st.worker == worker && st.updates == updates;
}
// `s` = `prefix` followed by empty polls ("p c") only
static bool then_only_polls(const std::string& s, const std::string& prefix) {
  if (s.compare(0, prefix.size(), prefix) != 0) return false;
  size_t i = prefix.size();
  while (s.compare(i, 4, " p c") == 0) i += 4;
  return i == s.size() && i > prefix.size();
}
static std::string run_error(FakeServer& s) {
  try {
    s.run(0);
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

static void test_server_protocol() {
  const std::string name = "/psx_selftest_proto_" + std::to_string(getpid());
  CtrlQueue q(name, 64, true);
  const int D = kKindDelta, FIN = kKindFinal;
  {  // 1. ASP, 2 workers, 2 deltas each: a delta releases its sender, a final one nobody
    VectorClockTracker trk(2, -1);
    FakeServer s("AsyncServer", &trk, &q, 2, 5.0);
    s.begin();
    CHECK_TRACE(s, "B R-[0@0,1@0]");
    push(q, 0, D, 0), push(q, 1, D, 0), push(q, 0, FIN, 1), push(q, 1, FIN, 1);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 4));
    CHECK_TRACE(s, "S p c a0@0 d0@0 R0@0[0@1] p c a1@0 d1@0 R1@0[1@1]"
                   " p c a0@1 d0@1 r0 R0@1[] p c a1@1 d1@1 r1 R1@1[] E");
    CHECK(s.updates() == 4 && s.tokens() == 4 && s.failed().empty() && s.host_us_per_update() > 0.0);
  }
  {  // 2. BSP, 3 workers, one round then the final one: the third delta releases all at clock 1
    VectorClockTracker trk(3, 0);
    FakeServer s("AsyncServer", &trk, &q, 3, 5.0);
    s.begin();
    CHECK_TRACE(s, "B R-[0@0,1@0,2@0]");
    for (int k = 0; k < 3; ++k) push(q, k, D, 0);
    for (int k = 0; k < 3; ++k) push(q, k, FIN, 1);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 6));
    CHECK_TRACE(s, "S p c a0@0 d0@0 R0@0[] p c a1@0 d1@0 R1@0[] p c a2@0 d2@0 R2@0[0@1,1@1,2@1]"
                   " p c a0@1 d0@1 r0 R0@1[] p c a1@1 d1@1 r1 R1@1[] p c a2@1 d2@1 r2 R2@1[] E");
  }
  {  // 3. SSP(1), 2 workers: worker 0 runs ahead until it is held (clock 2); worker 1's final
     // delta answers worker 0 and not the finished worker 1 (the tracker releases both)
    VectorClockTracker trk(2, 1);
    FakeServer s("AsyncServer", &trk, &q, 2, 5.0);
    s.begin();
    CHECK_TRACE(s, "B R-[0@0,1@0]");
    push(q, 0, D, 0), push(q, 0, D, 1), push(q, 1, FIN, 0), push(q, 0, FIN, 2);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 4));
    CHECK_TRACE(s, "S p c a0@0 d0@0 R0@0[0@1] p c a0@1 d0@1 R0@1[] p c a1@0 d1@0 r1 R1@0[0@2]"
                   " p c a0@2 d0@2 r0 R0@2[] E");
  }
  {  // 3b. the same with worker 0 three clocks ahead (a restored tracker; no bootstrap): worker
     // 1's final delta alone leaves it held, the retirement's list appended behind on_delta's
     // releases it
    VectorClockTracker trk(2, 1);
    trk.restore({3, 0}, {0, 1});
    FakeServer s("AsyncServer", &trk, &q, 2, 5.0);
    push(q, 1, FIN, 0), push(q, 0, FIN, 3);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 2));
    CHECK_TRACE(s, "S p c a1@0 d1@0 r1 R1@0[0@3] p c a0@3 d0@3 r0 R0@3[] E");
  }
  {  // 4. SSP(1), 3 workers: worker 0 held at clock 2 by the silent worker 1, which then
     // reports an error; fail(1) answers worker 0; the run goes on to done
    VectorClockTracker trk(3, 1);
    FakeServer s("AsyncServer", &trk, &q, 3, 5.0);
    s.begin();
    CHECK_TRACE(s, "B R-[0@0,1@0,2@0]");
    push(q, 0, D, 0), push(q, 0, D, 1), push(q, 2, D, 0), push(q, 1, kKindError, 0);
    push(q, 0, FIN, 2), push(q, 2, FIN, 1);
    CHECK(is_status(s.run(0), kAsyncErrorToken, 1, 3));
    CHECK_TRACE(s, "S p c a0@0 d0@0 R0@0[0@1] p c a0@1 d0@1 R0@1[] p c a2@0 d2@0 R2@0[2@1] p c F");
    s.fail(1);
    CHECK_TRACE(s, "S r1 R-[0@2]");
    CHECK(s.failed() == std::vector<int>{1} && s.log_worker() == 0);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 5));
    CHECK_TRACE(s, "S p c a0@2 d0@2 r0 R0@2[] p c a2@1 d2@1 r2 R2@1[] E");
    CHECK(s.failed() == std::vector<int>{1} && s.log_worker() == 0 && s.tokens() == 6);
    // 8. second begin(): the finished workers 0 and 2 rejoin at their tracked clocks, the
    // failed worker 1 stays dead
    s.begin();
    CHECK_TRACE(s, "B v0 v2 R-[0@3,2@2]");
    CHECK(s.failed() == std::vector<int>{1} && trk.is_live(0) && !trk.is_live(1) && trk.is_live(2));
    CHECK(trk.is_sent(0) && trk.is_sent(2));
    push(q, 0, FIN, 3), push(q, 2, FIN, 2);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 7));
    CHECK_TRACE(s, "S p c a0@3 d0@3 r0 R0@3[] p c a2@2 d2@2 r2 R2@2[] E");
    bool threw = false;
    try {
      s.fail(3);
    } catch (const std::out_of_range& e) {
      threw = std::string(e.what()) == "AsyncServer::fail: worker id";
    }
    CHECK(threw);
    CHECK_TRACE(s, "");
  }
  {  // 5. worker 0 fails: the server rows follow worker 1
    VectorClockTracker trk(2, -1);
    FakeServer s("AsyncServer", &trk, &q, 2, 5.0);
    s.begin();
    CHECK(s.log_worker() == 0);
    s.take();
    s.fail(0);
    CHECK_TRACE(s, "S r0");  // (nobody released: no release)
    CHECK(s.log_worker() == 1 && s.failed() == std::vector<int>{0});
    push(q, 1, FIN, 0);
    CHECK(is_status(s.run(0), kAsyncDone, -1, 1));
    CHECK_TRACE(s, "S p c a1@0 d1@0 r1 R1@0[] E");
  }
  {  // 6. watchdog (BSP, 2 workers): worker 0 answered and waits for the round (not busy),
     // worker 1 holds the bootstrap weights and stays silent
    VectorClockTracker trk(2, 0);
    FakeServer s("AsyncServer", &trk, &q, 2, 0.05);
    s.begin();
    s.take();
    push(q, 0, D, 0);
    const auto t0 = std::chrono::steady_clock::now();
    CHECK(is_status(s.run(0), kAsyncWatchdog, 1, 1));
    CHECK(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 1.0);
    CHECK(then_only_polls(s.take(), "S p c a0@0 d0@0 R0@0[]"));  // (and no E)
  }
  {  // 7. checkpoint every 2 updates (ASP, 2 workers): the stop comes after the update's
     // releases, also when that update was the last one; run() again continues
    VectorClockTracker trk(2, -1);
    FakeServer s("AsyncServer", &trk, &q, 2, 5.0);
    s.begin();
    s.take();
    push(q, 0, D, 0), push(q, 1, D, 0), push(q, 0, FIN, 1), push(q, 1, FIN, 1);
    CHECK(is_status(s.run(2), kAsyncCheckpoint, -1, 2));
    CHECK_TRACE(s, "S p c a0@0 d0@0 R0@0[0@1] p c a1@0 d1@0 R1@0[1@1] E");
    CHECK(is_status(s.run(2), kAsyncCheckpoint, -1, 4));
    CHECK_TRACE(s, "S p c a0@1 d0@1 r0 R0@1[] p c a1@1 d1@1 r1 R1@1[] E");
    CHECK(is_status(s.run(2), kAsyncDone, -1, 4));
    CHECK_TRACE(s, "S E");
    s.set_updates(10);
    CHECK(s.updates() == 10);
  }
  {  // 9. protocol violations carry the server's name
    VectorClockTracker trk(2, -1);
    FakeServer s("AsyncServer", &trk, &q, 2, 5.0);
    s.begin();
    s.take();
    push(q, 5, D, 0), push(q, 0, FIN, 0), push(q, 0, D, 1);
    CHECK(run_error(s) == "AsyncServer: token from an unknown worker");
    CHECK_TRACE(s, "S p c");
    CHECK(run_error(s) == "AsyncServer: delta from a finished worker 0");
    CHECK_TRACE(s, "S p c a0@0 d0@0 r0 R0@0[] p c");
    VectorClockTracker trk2(2, -1);
    FakeServer s2("PeerServer", &trk2, &q, 2, 5.0);
    s2.begin();
    push(q, -1, D, 0), push(q, 1, D, 7);
    CHECK(run_error(s2) == "PeerServer: token from an unknown worker");
    // (the tracker's own complaint comes through the C ABI with the same prefix)
    CHECK(run_error(s2).rfind("PeerServer: tracker on_delta: worker 1 pushed vc 7", 0) == 0);
  }
  {  // 10. a plane with pending work (ASP, 3 workers), three tokens queued at once: the first
     // pop waits, the others and the one that finds the queue empty do not; then one flush;
     // nobody answers after that: watchdog, without the end of the run
    VectorClockTracker trk(3, -1);
    FakeServer s("PeerServer", &trk, &q, 3, 0.05, true);
    s.begin();
    CHECK_TRACE(s, "B R-[0@0,1@0,2@0]");
    for (int k = 0; k < 3; ++k) push(q, k, D, 0);
    CHECK(is_status(s.run(0), kAsyncWatchdog, 0, 3));
    CHECK(then_only_polls(s.take(), "S p c a0@0 d0@0 R0@0[0@1] p0 c a1@0 d1@0 R1@0[1@1]"
                                    " p0 c a2@0 d2@0 R2@0[2@1] p0 F"));
    // the open batch goes out before an error token is reported
    push(q, 0, D, 1), push(q, 1, kKindError, 0);
    CHECK(is_status(s.run(0), kAsyncErrorToken, 1, 4));
    CHECK_TRACE(s, "S p c a0@1 d0@1 R0@1[0@2] p0 c F");
    s.fail(1);
    CHECK_TRACE(s, "S r1");
    // the end of the run on a checkpoint and on done
    push(q, 0, FIN, 2), push(q, 2, FIN, 1);
    CHECK(is_status(s.run(5), kAsyncCheckpoint, -1, 5));
    CHECK_TRACE(s, "S p c a0@2 d0@2 r0 R0@2[] E");
    CHECK(is_status(s.run(5), kAsyncDone, -1, 6));
    CHECK_TRACE(s, "S p c a2@1 d2@1 r2 R2@1[] E");
  }
  q.unlink();
}

// ---- AsyncLanesProtocol -------------------------------------------------------
// Everything the protocol does to its plane, the tracker, the sink and the control
// queue, in order, as one line of words:
//   r(lane,tag,vc,snap,B,start,n,dst,first,step,first2,n2,w,s,pull)   a release record
//        (w / s: 1 = a worker-row / server-row slot was acquired)     x(lane,tag)  a stop record
//   dK@V / rK    tracker on_delta / retire (as above)
//   m[..]        rows handed to the sink, in order: s@vc server row, wK@vc:seen worker row
//   c[k,kind,vc,aux]   control token pushed (remote)
//   bpL / pdL / sdL    begin-pull, pull landed, send-delta of lane L (remote, host transport)
// The expected lines are what LanesLoop::run_async / run_async_remote, poll_async and
// try_release did before they became this class, written out by hand.  The standard rig:
// rows arrive 4 per release attempt (per_iter_rows), the windows hold at most 8 rows in a
// ring of 16 (their target stays at the maximum), the ring of a lane has 16 slots.
static std::string rel_word(int l, unsigned tag, long long vc, long long snap, int B, int start, int n, int dst,
                            long long first, long long step, long long first2, int n2, int w, int s, unsigned pull) {
  const long long v[] = {l, tag, vc, snap, B, start, n, dst, first, step, first2, n2, w, s, pull};
  std::string o = "r(";
  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o += (i ? "," : "") + std::to_string(v[i]);
  return o + ")";
}
#define R rel_word

class LanesRig;
static LanesRig* g_rig = nullptr;
static int lanes_traced_submit(void* sink, int n, const SinkRecord* recs) {
  std::string w = "m[";
  for (int i = 0; i < n; ++i) {
    w += i ? "," : "";
    if (recs[i].kind & 1)
      w += "s@" + std::to_string((long long)recs[i].vc);
    else
      w += "w" + at((int)recs[i].partition, recs[i].vc) + ":" + std::to_string((long long)recs[i].nseen);
  }
  say(w + "]");
  return host_api()->sink_submit_many(sink, n, recs);
}
static int lanes_traced_push(void* q, const CtrlToken* t, double timeout_s);
static const HostApi* lanes_api() {
  static HostApi a = [] {
    HostApi x = *host_api();
    x.tracker_on_delta = traced_on_delta;
    x.tracker_retire = traced_retire;
    x.sink_submit_many = lanes_traced_submit;
    x.ctrl_push = lanes_traced_push;
    return x;
  }();
  return &a;
}

struct LanesRigOpt {
  int N = 3;
  std::vector<int> k = {0, 1, 2};  // the lanes' workers
  int c = -1;                      // consistency (ASP)
  int per_iter_rows = 4;
  double p_ms = 0.0;
  int64_t ds_rows = 3000, epochs = 1;
  bool peer = false;
};

class LanesRig : public AsyncLanesPlane {
 public:
  // a scripted token: lane `lane` pushes (vc < 0: at the clock of its release); the clock
  // advances by adv_ms first; force: also when the lane has no solve in flight;
  // empty_window: the lane's window is emptied first
  struct Tok {
    int lane;
    int64_t vc = -1;
    double adv_ms = 0.0;
    bool force = false, empty_window = false;
  };
  explicit LanesRig(const LanesRigOpt& o = LanesRigOpt())
      : trk(o.N, o.c), slots_(16),
        qname_("/psx_selftest_lanes_" + std::to_string(getpid()) + "_" + std::to_string(++rigs_)) {
    std::memset(slots_.data(), 0, sizeof(EvalSlot) * slots_.size());
    sink.reset(new MetricsSink(reinterpret_cast<uintptr_t>(slots_.data()), (int)slots_.size(), 2, nullptr, nullptr,
                               true));
    ctrl.reset(new CtrlQueue(qname_ + "_c", 64, true));
    reply.reset(new CtrlQueue(qname_ + "_r", 64, true));
    const int L = (int)o.k.size();
    cfg.N = o.N;
    cfg.L = L;
    cfg.k = o.k;
    cfg.per_iter_rows = o.per_iter_rows;
    cfg.p_ms = o.p_ms;
    cfg.ds_rows = o.ds_rows;
    cfg.epochs = o.epochs;
    cfg.sink = reinterpret_cast<uintptr_t>(sink.get());
    cfg.tracker = reinterpret_cast<uintptr_t>(&trk);
    cfg.api = reinterpret_cast<uintptr_t>(lanes_api());
    for (int l = 0; l < L; ++l) {
      win.emplace_back(new SlidingWindow(1, 8, 100.0, 500, 16));
      cfg.window.push_back(reinterpret_cast<uintptr_t>(win.back().get()));
      feeds.emplace_back(ShardFeed::Cfg{o.k[l], o.N, o.ds_rows, o.epochs, o.per_iter_rows, o.p_ms, cfg.window[l], 16,
                                        lanes_api(), "LanesLoop: "});
    }
    last_.assign(L, RelRec{});
    inflight_.assign(L, 0);
    pull_left_.assign(L, 0);
    p.bind(&cfg, o.peer, this, &feeds);
    g_trace = &trace_;
    g_rig = this;
  }
  ~LanesRig() override {
    g_trace = nullptr;
    g_rig = nullptr;
    sink->close();
    ctrl->unlink();
    reply->unlink();
  }
  // one call of LanesLoop::run_async / run_async_remote without the GPU: the launch resets the
  // stop bookkeeping, the drain gives every lane its stop record -- also behind an exception
  int64_t local(int64_t updates, double max_wait_s = 0.5, double deadline_ms = 0.0,
                const std::vector<int64_t>& budget = std::vector<int64_t>()) {
    p.begin_local(max_wait_s);
    p.on_launch();
    return drained([&] { return p.run_local(updates, max_wait_s, deadline_ms, budget); });
  }
  int64_t remote(bool peer, int64_t iters, double max_wait_s = 0.5, double deadline_ms = 0.0) {
    p.begin_remote(max_wait_s);
    p.on_launch();
    return drained([&] {
      return p.run_remote(peer, reinterpret_cast<uintptr_t>(ctrl.get()), reinterpret_cast<uintptr_t>(reply.get()),
                          iters, max_wait_s, deadline_ms);
    });
  }
  void feed(std::initializer_list<int> lanes) {
    for (int l : lanes) script.push_back(Tok{l});
  }
  void push_reply(int worker, int64_t vc, int64_t aux) {
    CtrlToken t{};
    t.worker = worker;
    t.vc = vc;
    t.aux = aux;
    if (!reply->push(t, 10.0)) std::abort();
  }
  // the words since the last call; brief: the releases as rL@vc and the stops as xL only
  std::string take() {
    std::string out;
    for (const auto& w : trace_) out += (out.empty() ? "" : " ") + w;
    trace_.clear();
    brief_.clear();
    return out;
  }
  std::string take_brief() {
    const std::string out = brief_;
    take();
    return out;
  }

  LanesHostCfg cfg;
  AsyncLanesProtocol p;
  VectorClockTracker trk;
  std::unique_ptr<MetricsSink> sink;
  std::unique_ptr<CtrlQueue> ctrl, reply;
  std::vector<std::unique_ptr<SlidingWindow>> win;
  std::vector<ShardFeed> feeds;
  std::deque<Tok> script;
  double t_ms = 1000.0;         // the scripted wall clock
  double idle_step_ms = 1.0;    // ... advances by this on every look at an empty token slot
  double sleep_step_ms = -1.0;  // ... and by this per idle sleep (< 0: the sleep's length)
  int sleeps = 0, polls = 0;
  int pull_delay = 0;           // pull_done answers false this often per pull
  bool auto_reply = false;      // a pushed delta token is answered like the server would

 protected:
  void write_release(int lane, const RelRec& q, unsigned tag) override {
    TagChunk ch[kRelChunks];
    pack_release(q, tag, ch);
    RelRec u;
    std::memset(&u, 0, sizeof(u));
    unpack_release(ch, u);
    for (int i = 0; i < kRelChunks; ++i) CHECK(ch[i].tag == tag);
    CHECK(u.stop == q.stop && u.vc == q.vc && u.snap == q.snap && u.r.B == q.r.B && u.r.first2 == q.r.first2 &&
          u.slot_w == q.slot_w && u.slot_s == q.slot_s && u.seq_s == q.seq_s && u.pull_tag == q.pull_tag);
    if (q.stop) {
      say("x(" + std::to_string(lane) + "," + std::to_string(tag) + ")");
      brief_ += (brief_.empty() ? "x" : " x") + std::to_string(lane);
      return;
    }
    say(rel_word(lane, tag, q.vc, q.snap, q.r.B, q.r.start, q.r.n, q.r.dst, q.r.first, q.r.step, q.r.first2, q.r.n2,
                 q.slot_w != 0, q.slot_s != 0, q.pull_tag));
    brief_ += (brief_.empty() ? "r" : " r") + at(lane, q.vc);
    last_[lane] = q;
    inflight_[lane] = 1;
    // the "device": the rows' slots are complete before the token (tagged chunks, K = 2)
    publish(q.slot_w, q.seq_w);
    publish(q.slot_s, q.seq_s);
  }
  AsyncToken read_token(uint64_t n) override {
    if (script.empty() || (!script.front().force && !inflight_[script.front().lane])) {
      t_ms += idle_step_ms;
      return AsyncToken{0u, 0u, 0u, 0u};
    }
    const Tok t = script.front();
    script.pop_front();
    t_ms += t.adv_ms;
    if (t.empty_window) win[t.lane]->restore(-1, 0, win[t.lane]->tuples_seen());
    const uint64_t vc = (uint64_t)(t.vc >= 0 ? t.vc : (int64_t)last_[t.lane].vc);
    inflight_[t.lane] = 0;
    return AsyncToken{(unsigned)n, (unsigned)t.lane, (unsigned)vc, (unsigned)(vc >> 32)};
  }
  void poll_errors() override { ++polls; }
  std::string progress_report() override { return "launch 1: scripted"; }
  void begin_pull(int lane) override {
    say("bp" + std::to_string(lane));
    pull_left_[lane] = pull_delay;
  }
  bool pull_done(int lane) override {
    if (pull_left_[lane] > 0) {
      --pull_left_[lane];
      return false;
    }
    say("pd" + std::to_string(lane));
    return true;
  }
  void send_delta(int lane) override { say("sd" + std::to_string(lane)); }
  double now_ms() override { return t_ms; }
  int64_t mono_ns() override { return ns_ += 1000; }
  void idle_sleep(int us) override {
    ++sleeps;
    t_ms += sleep_step_ms >= 0.0 ? sleep_step_ms : us / 1000.0;
  }

 private:
  template <class F>
  int64_t drained(F f) {
    int64_t done = 0;
    try {
      done = f();
    } catch (...) {
      p.stop_lanes();
      throw;
    }
    p.stop_lanes();
    return done;
  }
  static void publish(unsigned long long addr, unsigned seq) {
    if (!addr) return;
    uint32_t* w = reinterpret_cast<uint32_t*>(addr);
    for (int i = 0; i < 3; ++i) {  // 1 + (K * K + 2) / 3 chunks
      w[4 * i + 1] = w[4 * i + 2] = w[4 * i + 3] = 0u;
      w[4 * i] = seq | 0x80000000u;
    }
  }
  std::vector<EvalSlot> slots_;
  std::string qname_;
  std::vector<std::string> trace_;
  std::string brief_;
  std::vector<RelRec> last_;
  std::vector<uint8_t> inflight_;
  std::vector<int> pull_left_;
  int64_t ns_ = 0;
  static int rigs_;  // (queue names: several rigs live at once)
};
int LanesRig::rigs_ = 0;

static int lanes_traced_push(void* q, const CtrlToken* t, double timeout_s) {
  say("c[" + std::to_string(t->worker) + "," + std::to_string(t->kind) + "," + std::to_string((long long)t->vc) +
      "," + std::to_string((long long)t->aux) + "]");
  const int rc = host_api()->ctrl_push(q, t, timeout_s);
  if (g_rig && g_rig->auto_reply && t->kind == kKindDelta)  // the server: the next weights, tagged
    g_rig->push_reply(t->worker, t->vc + 1, 100 + 10 * t->worker + t->vc + 1);
  return rc;
}

template <class E, class F>
static std::string error_of(F f) {
  try {
    f();
  } catch (const E& e) {
    return e.what();
  } catch (const std::exception& e) {
    return std::string("(another exception) ") + e.what();
  }
  return "(none)";
}

static void test_lanes_protocol() {
  LanesRigOpt ssp3;  // 3 lanes, workers 0..2, SSP(1)
  ssp3.c = 1;
  const LanesRigOpt asp3;  // the same under ASP
  LanesRigOpt one;         // 1 lane, worker 0 of 1, ASP
  one.N = 1;
  one.k = {0};
  one.ds_rows = 1000;
  {  // 1. bootstrap, SSP(1), fresh tracker: everybody at clock 0 with the snapshot of the current
     // ticket; the tokens come in the order 2, 0, 1 and release their senders in that order with
     // the snapshot of their own ticket; server row first, and on the log lane (worker 0) only;
     // every release carries the 4 rows delivered for it (rows k, k + 3, ...)
    LanesRig g(ssp3);
    g.feed({2, 0, 1, 2, 0, 1});
    CHECK(g.local(6) == 6);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " " + R(1, 1, 0, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 0, 0) +
                       " " + R(2, 1, 0, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) + " m[w2@0:4] d2@0 " +
                       R(2, 2, 1, 1, 8, 0, 4, 4, 14, 3, 0, 0, 1, 0, 0) + " m[s@0,w0@0:4] d0@0 " +
                       R(0, 2, 1, 2, 8, 0, 4, 4, 12, 3, 0, 0, 1, 1, 0) + " m[w1@0:4] d1@0 " +
                       R(1, 2, 1, 3, 8, 0, 4, 4, 13, 3, 0, 0, 1, 0, 0) +
                       " m[w2@1:8] d2@1 m[s@1,w0@1:8] d0@1 m[w1@1:8] d1@1 x(0,3) x(1,3) x(2,3)");
    CHECK(g.p.tickets() == 6 && g.p.log_lane() == 0 && g.p.crashed().empty() && g.p.left().empty());
    CHECK(g.p.host_busy_us_per_token() == 1.0);  // (the scripted steady clock: 1 us per reading)
    CHECK(g.sink->flush(30.0));
    const auto srows = g.sink->server_rows();
    CHECK(srows.size() == 2 && srows[0].vc == 0 && srows[1].vc == 1 && g.sink->worker_rows().size() == 6);
  }
  {  // 2. the SSP gap: worker 1's token is withheld; workers 0 and 2 stop one clock ahead (their
     // second delta releases nobody) and resume, with worker 1, when it arrives; `updates` = 7
     // leaves lane 2's release for the next call
    LanesRig g(ssp3);
    g.feed({0, 2, 0, 2, 1, 0, 1});
    CHECK(g.local(7) == 7);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " " + R(1, 1, 0, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 0, 0) +
                       " " + R(2, 1, 0, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) + " m[s@0,w0@0:4] d0@0 " +
                       R(0, 2, 1, 1, 8, 0, 4, 4, 12, 3, 0, 0, 1, 1, 0) + " m[w2@0:4] d2@0 " +
                       R(2, 2, 1, 2, 8, 0, 4, 4, 14, 3, 0, 0, 1, 0, 0) +
                       " m[s@1,w0@1:8] d0@1 m[w2@1:8] d2@1 m[w1@0:4] d1@0 " +
                       R(0, 3, 2, 5, 8, 4, 4, 8, 24, 3, 0, 0, 1, 1, 0) + " " +
                       R(1, 2, 1, 5, 8, 0, 4, 4, 13, 3, 0, 0, 1, 0, 0) +
                       " m[s@2,w0@2:12] d0@2 m[w1@1:8] d1@1 x(0,4) x(1,3) x(2,3)");
    CHECK(g.p.state(2) == AsyncLanesProtocol::kWant && g.trk.is_sent(2) && g.trk.clock(2) == 2);
  }
  {  // 3. ASP: a delta releases its sender and nobody else
    LanesRig g(asp3);
    g.feed({1, 1, 0, 1, 2});
    CHECK(g.local(5) == 5);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " " + R(1, 1, 0, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 0, 0) +
                       " " + R(2, 1, 0, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) + " m[w1@0:4] d1@0 " +
                       R(1, 2, 1, 1, 8, 0, 4, 4, 13, 3, 0, 0, 1, 0, 0) + " m[w1@1:8] d1@1 " +
                       R(1, 3, 2, 2, 8, 4, 4, 8, 25, 3, 0, 0, 1, 0, 0) +
                       " m[s@0,w0@0:4] d0@0 m[w1@2:12] d1@2 m[w2@0:4] d2@0 x(0,2) x(1,4) x(2,2)");
  }
  {  // 4. token validation: a token of a lane without a solve in flight, a token at another
     // clock than the lane's release; every lane has exactly one stop record afterwards
    LanesRig g(asp3);
    LanesRig::Tok idle{1};
    idle.force = true;
    g.script.push_back(idle);
    CHECK(error_of<std::logic_error>([&] { g.local(1); }) == "LanesLoop: unexpected token (lane 1, vc 0)");
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " x(0,2) x(1,1) x(2,1)");
    LanesRig h(asp3);
    LanesRig::Tok wrong{0};
    wrong.vc = 5;
    h.script.push_back(wrong);
    CHECK(error_of<std::logic_error>([&] { h.local(3); }) == "LanesLoop: unexpected token (lane 0, vc 5)");
    CHECK(h.take_brief() == "r0@0 r1@0 r2@0 x0 x1 x2");
    CHECK(h.p.tickets() == 0);
  }
  {  // 5. budgets under ASP: per lane {2, 1, 3} -- no lane starts more than its share, the run
     // ends when every wanting lane is at its budget; the scalar form (2 each) with updates = 5:
     // reached exactly
    LanesRig g(asp3);
    g.feed({0, 0, 1, 2, 2, 2});
    CHECK(g.local(100, 0.5, 0.0, {2, 1, 3}) == 6);
    CHECK(g.take_brief() == "r0@0 r1@0 r2@0 r0@1 r2@1 r2@2 x0 x1 x2");
    LanesRig h(asp3);
    h.feed({0, 0, 1, 2, 1});
    CHECK(h.local(5, 0.5, 0.0, std::vector<int64_t>(3, 2)) == 5);
    CHECK(h.take_brief() == "r0@0 r1@0 r2@0 r0@1 r1@1 x0 x1 x2");
  }
  {  // 6. injected crash, drop policy, SSP(1): lanes 0, 1, 2 host workers 1, 0, 2; worker 0 (lane
     // 1, the log lane) holds the weights of clock 0, workers 1 and 2 are held at clock 2; lane 1
     // fails when released: its stop record before any solve, the retirement releases lane 2 and
     // lane 0 (behind the scan position: the scan restarts), the server rows move to worker 1
    LanesRigOpt o = ssp3;
    o.k = {1, 0, 2};
    LanesRig g(o);
    g.trk.restore({0, 2, 2}, {1, 0, 0});
    g.p.set_injection({-1, 0, -1}, {}, true);
    g.feed({0, 2});
    CHECK(g.local(2) == 2);
    CHECK_TRACE(g, "x(1,1) r0 " + R(0, 1, 2, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 1, 0) + " " +
                       R(2, 1, 2, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) +
                       " m[s@2,w1@2:4] d1@2 m[w2@2:4] d2@2 x(0,2) x(2,2)");
    CHECK(g.p.crashed() == std::vector<int>{0} && g.p.left().empty() && !g.trk.is_live(0));
    CHECK(g.p.log_lane() == 0 && g.cfg.log_worker == 1 && g.p.state(1) == AsyncLanesProtocol::kGone);
  }
  {  // 7. injected crash, fail policy: lane 1 fails when released after its first solve; nothing
     // new starts, the two solves in flight are still consumed, the worker is not retired
    LanesRig g(asp3);
    g.p.set_injection({-1, 1, -1}, {}, false);
    g.feed({1, 0, 2});
    CHECK(g.local(10) == 3);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " " + R(1, 1, 0, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 0, 0) +
                       " " + R(2, 1, 0, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) +
                       " m[w1@0:4] d1@0 x(1,2) m[s@0,w0@0:4] d0@0 m[w2@0:4] d2@0 x(0,2) x(2,2)");
    CHECK(g.p.crashed() == std::vector<int>{1} && g.trk.is_live(1) && g.cfg.log_worker == 0);
  }
  {  // 8. injected clean leave: lane 0 (the log lane) leaves after 2 solves -- its second delta is
     // applied and logged, then its stop record and its retirement; the server rows move to
     // worker 1 with lane 1's next release
    LanesRig g(asp3);
    g.p.set_injection({}, {2, -1, -1}, true);
    g.feed({0, 0, 1, 2, 1});
    CHECK(g.local(5) == 5);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " " + R(1, 1, 0, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 0, 0) +
                       " " + R(2, 1, 0, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) + " m[s@0,w0@0:4] d0@0 " +
                       R(0, 2, 1, 1, 8, 0, 4, 4, 12, 3, 0, 0, 1, 1, 0) + " m[s@1,w0@1:8] d0@1 x(0,3) r0 m[w1@0:4] d1@0 " +
                       R(1, 2, 1, 3, 8, 0, 4, 4, 13, 3, 0, 0, 1, 1, 0) +
                       " m[w2@0:4] d2@0 m[s@1,w1@1:8] d1@1 x(1,3) x(2,2)");
    CHECK(g.p.left() == std::vector<int>{0} && g.p.crashed().empty() && g.cfg.log_worker == 1);
    // 9. carry-over into the next call: the retired worker's lane is gone and only gets its stop
    // record; the releases wanted but not started (1@2, 2@1) start at once; a stop record is
    // written once per launch, and again in the next launch
    g.feed({1, 2});
    CHECK(g.local(2) == 2);
    CHECK_TRACE(g, R(1, 4, 2, 5, 8, 4, 4, 8, 25, 3, 0, 0, 1, 1, 0) + " " + R(2, 3, 1, 5, 8, 0, 4, 4, 14, 3, 0, 0, 1, 0, 0) +
                       " m[s@2,w1@2:12] d1@2 m[w2@1:8] d2@1 x(0,4) x(1,5) x(2,4)");
    CHECK(g.p.left().empty() && g.p.state(0) == AsyncLanesProtocol::kGone && g.p.tickets() == 7);
    g.p.stop_lanes();
    CHECK_TRACE(g, "");
    g.p.on_launch();
    g.p.stop_lane(1);
    g.p.stop_lanes();
    CHECK_TRACE(g, "x(1,6) x(0,5) x(2,5)");
  }
  {  // 10a. rows on the producer clock (2 workers, p_ms = 2000: rows 0..255 at 0 ms, row 256 at
     // 2000 ms, row 257 at 4000 ms): at 0 ms each worker has 128 rows due, the ring keeps the
     // last 16 (rows 224 + k, step 2), the window its last 8; at 2500 ms worker 0 gets row 256
     // and worker 1 nothing new (an empty run with the step filled in)
    LanesRigOpt o;
    o.N = 2;
    o.k = {0, 1};
    o.per_iter_rows = 0;
    o.p_ms = 2000.0;
    o.ds_rows = 600;
    LanesRig g(o);
    g.t_ms = 0.0;
    LanesRig::Tok late{0};
    late.adv_ms = 2500.0;
    g.script.push_back(late);
    g.feed({1, 0, 1});
    CHECK(g.local(4) == 4);
    CHECK_TRACE(g, R(0, 1, 0, 0, 8, 8, 16, 0, 224, 2, 0, 0, 1, 1, 0) + " " +
                       R(1, 1, 0, 0, 8, 8, 16, 0, 225, 2, 0, 0, 1, 0, 0) + " m[s@0,w0@0:128] d0@0 " +
                       R(0, 2, 1, 1, 8, 9, 1, 0, 256, 2, 0, 0, 1, 1, 0) + " m[w1@0:128] d1@0 " +
                       R(1, 2, 1, 2, 8, 8, 0, 0, 0, 2, 0, 0, 1, 0, 0) +
                       " m[s@1,w0@1:129] d0@1 m[w1@1:128] d1@1 x(0,3) x(1,3)");
  }
  {  // 10b. a delivery across the shard's epoch wrap (18 rows, 2 epochs): the fifth release
     // carries rows 16, 17 and, as its second run, rows 0, 1
    LanesRigOpt o = one;
    o.ds_rows = 18;
    o.epochs = 2;
    LanesRig g(o);
    g.feed({0, 0, 0, 0, 0});
    CHECK(g.local(5) == 5);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 1, 0, 0, 1, 1, 0) + " m[s@0,w0@0:4] d0@0 " +
                       R(0, 2, 1, 1, 8, 0, 4, 4, 4, 1, 0, 0, 1, 1, 0) + " m[s@1,w0@1:8] d0@1 " +
                       R(0, 3, 2, 2, 8, 4, 4, 8, 8, 1, 0, 0, 1, 1, 0) + " m[s@2,w0@2:12] d0@2 " +
                       R(0, 4, 3, 3, 8, 8, 4, 12, 12, 1, 0, 0, 1, 1, 0) + " m[s@3,w0@3:16] d0@3 " +
                       R(0, 5, 4, 4, 8, 12, 2, 0, 16, 1, 0, 2, 1, 1, 0) + " m[s@4,w0@4:20] d0@4 x(0,6)");
  }
  {  // 10c. the cadence new_rows = 24 holds the lane back for six deliveries (four idle sleeps);
     // 24 rows are more than the ring's 16: the front 8 are dropped and dst advanced
    LanesRig g(one);
    g.cfg.new_rows = 24;
    g.feed({0});
    CHECK(g.local(1) == 1);
    CHECK_TRACE(g, R(0, 1, 0, 0, 8, 0, 16, 8, 8, 1, 0, 0, 1, 1, 0) + " m[s@0,w0@0:24] d0@0 x(0,2)");
    CHECK(g.sleeps == 4);
  }
  {  // 10d. pending rows in a third non-contiguous run (a shard of 6 rows wraps twice)
    LanesRigOpt o = one;
    o.ds_rows = 6;
    o.epochs = 5;
    LanesRig g(o);
    g.cfg.new_rows = 100;
    CHECK(error_of<std::logic_error>([&] { g.local(1); }) == "LanesLoop: pending rows of a release span three runs");
    CHECK_TRACE(g, "x(0,1)");
  }
  {  // 10e. new_frac = 2 (16 new rows for a window of 8): four deliveries; capped by new_cap = 6: two
    LanesRig g(one);
    g.cfg.new_frac = 2.0;
    g.feed({0});
    CHECK(g.local(1) == 1);
    CHECK_TRACE(g, R(0, 1, 0, 0, 8, 8, 16, 0, 0, 1, 0, 0, 1, 1, 0) + " m[s@0,w0@0:16] d0@0 x(0,2)");
    CHECK(g.sleeps == 2);
    LanesRig h(one);
    h.cfg.new_frac = 2.0;
    h.cfg.new_cap = 6;
    h.feed({0});
    CHECK(h.local(1) == 1);
    CHECK_TRACE(h, R(0, 1, 0, 0, 8, 0, 8, 0, 0, 1, 0, 0, 1, 1, 0) + " m[s@0,w0@0:8] d0@0 x(0,2)");
    CHECK(h.sleeps == 0);
  }
  {  // 10f. new_ramp = 4 on top of new_frac = 2: the lane's solves wait for 4, 8, 16 new rows
     // (one, two, four deliveries)
    LanesRig g(one);
    g.cfg.new_frac = 2.0;
    g.cfg.new_ramp = 4;
    g.feed({0, 0, 0});
    CHECK(g.local(3) == 3);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 1, 0, 0, 1, 1, 0) + " m[s@0,w0@0:4] d0@0 " +
                       R(0, 2, 1, 1, 8, 4, 8, 4, 4, 1, 0, 0, 1, 1, 0) + " m[s@1,w0@1:12] d0@1 " +
                       R(0, 3, 2, 2, 8, 4, 16, 12, 12, 1, 0, 0, 1, 1, 0) + " m[s@2,w0@2:28] d0@2 x(0,4)");
    CHECK(g.sleeps == 2);
  }
  {  // 10g. an exhausted stream (16 rows, one epoch) releases whatever the cadence asks for: after
     // the fourth delivery, and again without any new row
    LanesRigOpt o = one;
    o.ds_rows = 16;
    LanesRig g(o);
    g.cfg.new_rows = 100;
    g.feed({0, 0});
    CHECK(g.local(2) == 2);
    CHECK_TRACE(g, R(0, 1, 0, 0, 8, 8, 16, 0, 0, 1, 0, 0, 1, 1, 0) + " m[s@0,w0@0:16] d0@0 " +
                       R(0, 2, 1, 1, 8, 8, 0, 0, 0, 1, 0, 0, 1, 1, 0) + " m[s@1,w0@1:16] d0@1 x(0,3)");
    CHECK(g.sleeps == 2);
  }
  {  // 11. watchdogs.  Solves in flight and no token: the scripted clock (1 ms per look at the
     // empty slot) is past max_wait_s = 0.5 at the first check (every 1,024 looks)
    LanesRig g(asp3);
    CHECK(error_of<std::runtime_error>([&] { g.local(3, 0.5); }) ==
          "LanesLoop: no delta from the device for 0.500000 s");
    CHECK(g.take_brief() == "r0@0 r1@0 r2@0 x0 x1 x2");
    CHECK(g.polls == 1 && g.sleeps == 0);
    // nothing in flight and no rows (the producer clock has not started): the idle limit of 2 s,
    // not max_wait_s, ends the run -- after 21 sleeps of 100 scripted ms; the lanes' wait budget
    // on the device is the larger of the two
    LanesRigOpt o = one;
    o.per_iter_rows = 0;
    o.p_ms = 2000.0;
    LanesRig h(o);
    h.cfg.t0_ms = 1e9;
    h.idle_step_ms = 0.0;
    h.sleep_step_ms = 100.0;
    h.p.set_idle_wait(2.0);
    CHECK(error_of<std::runtime_error>([&] { h.local(3, 0.5); }) == "LanesLoop: no rows for a worker");
    CHECK_TRACE(h, "x(0,1)");
    CHECK(h.sleeps == 21 && h.p.rel_wait_s() == 2.0);
    h.p.begin_local(5.0);
    CHECK(h.p.rel_wait_s() == 5.0);
  }
  {  // 12. the deadline (5000 ms; the clock starts at 1000) passes before lane 1's token: nothing
     // new starts, the solves in flight are consumed, the count is returned
    LanesRig g(asp3);
    g.feed({0});
    LanesRig::Tok late{1};
    late.adv_ms = 5000.0;
    g.script.push_back(late);
    g.feed({2, 0});
    CHECK(g.local(100, 0.5, 5000.0) == 4);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 0, 3, 0, 0, 1, 1, 0) + " " + R(1, 1, 0, 0, 4, 0, 4, 0, 1, 3, 0, 0, 1, 0, 0) +
                       " " + R(2, 1, 0, 0, 4, 0, 4, 0, 2, 3, 0, 0, 1, 0, 0) + " m[s@0,w0@0:4] d0@0 " +
                       R(0, 2, 1, 1, 8, 0, 4, 4, 12, 3, 0, 0, 1, 1, 0) +
                       " m[w1@0:4] d1@0 m[w2@0:4] d2@0 m[s@1,w0@1:8] d0@1 x(0,3) x(1,2) x(2,2)");
  }
  LanesRigOpt rank;  // a worker rank: lanes 0, 1 host workers 2, 3 of 4
  rank.N = 4;
  rank.k = {2, 3};
  rank.ds_rows = 4000;
  {  // 13. remote over the peer plane, 2 solves per lane: a reply token gives the clock and the pull
     // tag, the release carries them with snap = the lane; the control token has worker, vc and
     // aux = tuples seen, FINAL exactly on the second solve; worker rows only; the loop ends when
     // both lanes are done
    LanesRigOpt o = rank;
    o.peer = true;
    LanesRig g(o);
    g.auto_reply = true;
    g.push_reply(2, 0, 7);
    g.push_reply(3, 0, 9);
    g.feed({1, 0, 1, 0});
    CHECK(g.remote(true, 2) == 4);
    CHECK_TRACE(g, R(0, 1, 0, 0, 4, 0, 4, 0, 2, 4, 0, 0, 1, 0, 7) + " " + R(1, 1, 0, 1, 4, 0, 4, 0, 3, 4, 0, 0, 1, 0, 9) +
                       " c[3,0,0,4] m[w3@0:4] " + R(1, 2, 1, 1, 8, 0, 4, 4, 19, 4, 0, 0, 1, 0, 131) +
                       " c[2,0,0,4] m[w2@0:4] " + R(0, 2, 1, 0, 8, 0, 4, 4, 18, 4, 0, 0, 1, 0, 121) +
                       " c[3,1,1,8] m[w3@1:8] c[2,1,1,8] m[w2@1:8] x(0,3) x(1,3)");
    CHECK(g.p.state(0) == AsyncLanesProtocol::kDone && g.p.state(1) == AsyncLanesProtocol::kDone);
    CHECK(g.p.tickets() == 4 && g.ctrl->enqueued() == 4);
    // a reply for a lane that is not waiting for one
    LanesRig h(o);
    h.push_reply(2, 0, 7);
    h.push_reply(2, 0, 8);
    CHECK(error_of<std::logic_error>([&] { h.remote(true, 2); }) == "LanesLoop: reply for worker 2 not waiting");
    CHECK_TRACE(h, "x(0,1) x(1,1)");
    // FINAL at the deadline (5000 ms): the clock passes it with lane 0's first token, which was
    // judged at the time read before it; every token after that is FINAL
    LanesRig d(o);
    d.auto_reply = true;
    d.push_reply(2, 0, 7);
    d.push_reply(3, 0, 9);
    LanesRig::Tok late{0};
    late.adv_ms = 5000.0;
    d.script.push_back(late);
    d.feed({1, 0});
    CHECK(d.remote(true, 10, 0.5, 5000.0) == 3);
    CHECK_TRACE(d, R(0, 1, 0, 0, 4, 0, 4, 0, 2, 4, 0, 0, 1, 0, 7) + " " + R(1, 1, 0, 1, 4, 0, 4, 0, 3, 4, 0, 0, 1, 0, 9) +
                       " c[2,0,0,4] m[w2@0:4] " + R(0, 2, 1, 0, 8, 0, 4, 4, 18, 4, 0, 0, 1, 0, 121) +
                       " c[3,1,0,4] m[w3@0:4] c[2,1,1,8] m[w2@1:8] x(0,3) x(1,2)");
    // FINAL with the stream exhausted (4 rows per worker) and the window empty -- not with rows
    // still in the window (lane 1's first token)
    LanesRigOpt e = o;
    e.ds_rows = 16;
    LanesRig x(e);
    x.auto_reply = true;
    x.push_reply(2, 0, 7);
    x.push_reply(3, 0, 9);
    LanesRig::Tok empty0{0}, empty1{1};
    empty0.empty_window = empty1.empty_window = true;
    x.script.push_back(empty0);
    x.feed({1});
    x.script.push_back(empty1);
    CHECK(x.remote(true, 10) == 3);
    CHECK_TRACE(x, R(0, 1, 0, 0, 4, 0, 4, 0, 2, 4, 0, 0, 1, 0, 7) + " " + R(1, 1, 0, 1, 4, 0, 4, 0, 3, 4, 0, 0, 1, 0, 9) +
                       " c[2,1,0,4] m[w2@0:4] c[3,0,0,4] m[w3@0:4] " +
                       R(1, 2, 1, 1, 4, 0, 0, 0, 0, 4, 0, 0, 1, 0, 131) + " c[3,1,1,4] m[w3@1:4] x(0,2) x(1,3)");
  }
  {  // 14. remote over a host transport: the pulls begin in reply order (worker 3 first), a lane is
     // released once its pull has landed (the third time it is asked), the delta goes out before
     // its control token; no pull tags
    LanesRig g(rank);
    g.pull_delay = 2;
    g.push_reply(3, 0, 0);
    g.push_reply(2, 0, 0);
    g.feed({1, 0});
    CHECK(g.remote(false, 1) == 2);
    CHECK_TRACE(g, "bp1 bp0 pd0 " + R(0, 1, 0, 0, 4, 0, 4, 0, 2, 4, 0, 0, 1, 0, 0) + " pd1 " +
                       R(1, 1, 0, 1, 4, 0, 4, 0, 3, 4, 0, 0, 1, 0, 0) +
                       " sd1 c[3,1,0,4] m[w3@0:4] sd0 c[2,1,0,4] m[w2@0:4] x(0,2) x(1,2)");
    // no progress: lane 0 never hears from the server, lane 1's pull (clock 5) never lands
    LanesRig h(rank);
    h.pull_delay = 1 << 30;
    h.push_reply(3, 5, 0);
    CHECK(error_of<std::runtime_error>([&] { h.remote(false, 1, 0.5); }) ==
          "LanesLoop: no progress with the server for 0.500000 s; lanes (state 1 want / 2 running / 3 wait pull / 4 "
          "pulling / 5 done, vc, pull tag): [3 0 0 it 0] [4 5 0 it 0]; tokens pushed 0; launch 1: scripted");
    CHECK_TRACE(h, "bp1 x(0,1) x(1,1)");
    CHECK(h.polls == 1);
  }
  {  // 15. the release record's 16-B chunks: 64-bit fields above 2^32, a negative first
    RelRec q;
    std::memset(&q, 0, sizeof(q));
    q.stop = 1;
    q.vc = (5ll << 32) + 7;
    q.snap = (9ll << 32) + 1;
    q.r = LaneRound{1024, 17, 300, 4000, -5, (3ll << 32) + 2, (1ll << 40) + 3, 11, 0};
    q.slot_w = 0x7f12345678abcdefull;
    q.slot_s = 0x00007fffdeadbee0ull;
    q.seq_w = 0xfffffff0u;
    q.seq_s = 0x80000001u;
    q.delay_us = 250;
    q.pull_tag = 0xdeadbeefu;
    TagChunk ch[kRelChunks];
    pack_release(q, 0xabcd0123u, ch);
    RelRec u;
    std::memset(&u, 0xff, sizeof(u));
    unpack_release(ch, u);
    for (int i = 0; i < kRelChunks; ++i) CHECK(ch[i].tag == 0xabcd0123u);
    CHECK(u.stop == 1 && u.vc == q.vc && u.snap == q.snap && u.r.B == 1024 && u.r.start == 17 && u.r.n == 300 &&
          u.r.dst == 4000 && u.r.first == -5 && u.r.step == q.r.step && u.r.first2 == q.r.first2 && u.r.n2 == 11 &&
          u.r.delay_us == 0 && u.slot_w == q.slot_w && u.slot_s == q.slot_s && u.seq_w == q.seq_w &&
          u.seq_s == q.seq_s && u.delay_us == 250 && u.pull_tag == q.pull_tag);
  }
}
#undef R

// ---- ShardFeed + RoundGate (shard_feed.h) ----
// A feed over a real window (at most 8 rows in a ring of 16, its target stays at the
// maximum) and a ring of 16 slots.  The standard shard must wrap: worker 1 of 2 over 11
// rows reads dataset rows 1, 3, 5, 7, 9 (5 local rows).  take(): what one deliver() did,
// as k<keep> (src_first,step,n,slot)...  The expected lines are what the four polls
// (BspLoop, LanesLoop, KeyRangeLoop, AsyncLanesProtocol::poll_async) computed before they
// became this class, written out by hand.
struct FeedRig {
  explicit FeedRig(int per_iter_rows, int64_t epochs, double p_ms = 0.0, int64_t ds_rows = 11,
                   const HostApi* api = host_api(), const char* who = "LanesLoop: ")
      : win(1, 8, 100.0, 500, 16),
        feed(ShardFeed::Cfg{1, 2, ds_rows, epochs, per_iter_rows, p_ms, reinterpret_cast<uintptr_t>(&win), 16, api,
                            who}) {}
  int64_t deliver(double now_ms) {
    return feed.deliver(
        now_ms, [&](int64_t keep) { trace += "k" + std::to_string((long long)keep); },
        [&](int64_t src_first, int64_t step, int64_t n, int64_t slot) {
          trace += " (" + std::to_string((long long)src_first) + "," + std::to_string((long long)step) + "," +
                   std::to_string((long long)n) + "," + std::to_string((long long)slot) + ")";
        });
  }
  std::string take() {
    std::string o;
    o.swap(trace);
    return o;
  }
  // the cursor and the window: next_local size start seen
  std::string at() const {
    const ShardFeed::Window v = feed.window();
    return std::to_string((long long)feed.next_local()) + " " + std::to_string((long long)v.size) + " " +
           std::to_string((long long)v.start) + " " + std::to_string((long long)v.seen);
  }
  SlidingWindow win;
  ShardFeed feed;
  std::string trace;
};

static void test_shard_feed() {
  {  // a, b, c: 4 rows per delivery, 2 epochs of 5 rows -- inside the first epoch; across its end
     // (two runs, the second from the shard's first row again); the last delivery cut at the limit
    FeedRig g(4, 2);
    CHECK(g.feed.local_total() == 5 && g.feed.cap() == 16 && !g.feed.exhausted() && g.at() == "0 0 0 0");
    CHECK(g.deliver(7.0) == 4);
    CHECK_TRACE(g, "k4 (1,2,4,0)");
    CHECK(g.at() == "4 4 0 4");
    CHECK(g.deliver(7.0) == 4);
    CHECK_TRACE(g, "k4 (9,2,1,4) (1,2,3,5)");
    CHECK(g.at() == "8 8 0 8" && !g.feed.exhausted());
    CHECK(g.deliver(8.0) == 2);
    CHECK_TRACE(g, "k2 (7,2,2,8)");
    CHECK(g.at() == "10 8 2 10" && g.feed.exhausted());
    CHECK(g.deliver(9.0) == 0);  // exhausted: nothing, not even the keep hook
    CHECK_TRACE(g, "");
    CHECK(g.at() == "10 8 2 10");
  }
  {  // d: a delivery larger than the ring -- 20 rows, the first 4 are never emitted (the ring
     // would overwrite them), the first surviving row is local row 4 in slot (0 + 4) % 16; the
     // last run wraps the ring (slots 15, 0, 1, 2, 3); 20 is what deliver() returns
    FeedRig g(20, 10);
    CHECK(g.deliver(1.0) == 20);
    CHECK_TRACE(g, "k16 (9,2,1,4) (1,2,5,5) (1,2,5,10) (1,2,5,15)");
    CHECK(g.at() == "20 8 12 20");
  }
  {  // e: the ring slot wraps inside a run (the third delivery's second run: slots 15, 0, 1)
    FeedRig g(6, 100);
    CHECK(g.deliver(1.0) == 6);
    CHECK_TRACE(g, "k6 (1,2,5,0) (1,2,1,5)");
    CHECK(g.at() == "6 6 0 6");
    CHECK(g.deliver(1.0) == 6);
    CHECK_TRACE(g, "k6 (3,2,4,6) (1,2,2,10)");
    CHECK(g.at() == "12 8 4 12");
    CHECK(g.deliver(1.0) == 6);
    CHECK_TRACE(g, "k6 (5,2,3,12) (1,2,3,15)");
    CHECK(g.at() == "18 8 10 18");
  }
  {  // f: the producer clock (2 rows per second after a burst of 128 rows per worker).  The small
     // shard lies inside the burst: nothing is due before its arrival time 0, then the whole
     // epoch -- and no more than the epoch in one call, though the next epoch is due as well
    FeedRig g(0, 2, 500.0);
    CHECK(g.deliver(-1.0) == 0);
    CHECK_TRACE(g, "");
    CHECK(g.at() == "0 0 0 0");
    CHECK(host_api()->due_rows(1, 2, 500.0, 11, 0, 0.0, 10, nullptr) == 5);
    CHECK(g.deliver(0.0) == 5);
    CHECK_TRACE(g, "k5 (1,2,5,0)");
    CHECK(g.at() == "5 5 0 5");
    CHECK(g.deliver(0.0) == 5);
    CHECK_TRACE(g, "k5 (1,2,5,5)");
    CHECK(g.at() == "10 8 2 10" && g.feed.exhausted());
    // 300 local rows: the burst (local rows 0..127) at 0 -- more than the ring holds --, local
    // row 128 (dataset row 257) at 1000 ms, row 129 at 2000 ms, row 130 at 3000 ms
    FeedRig h(0, 1, 500.0, 600);
    CHECK(h.feed.local_total() == 300);
    CHECK(host_api()->due_rows(1, 2, 500.0, 600, 0, 0.0, 300, nullptr) == 128);
    CHECK(h.deliver(0.0) == 128);
    CHECK_TRACE(h, "k16 (225,2,16,0)");
    CHECK(h.at() == "128 8 8 128");
    CHECK(h.deliver(999.0) == 0);
    CHECK_TRACE(h, "");
    CHECK(host_api()->due_rows(1, 2, 500.0, 600, 128, 2000.0, 172, nullptr) == 2);
    CHECK(h.deliver(2000.0) == 2);
    CHECK_TRACE(h, "k2 (257,2,2,0)");
    CHECK(h.at() == "130 8 10 130");
  }
  {  // g: a resume mid-epoch -- the window restored (3 rows, newest in slot 2), the cursor set
    FeedRig g(4, 2);
    g.win.restore(2, 3, 3);
    g.feed.set_next_local(3);
    CHECK(g.feed.next_local() == 3 && g.at() == "3 3 0 3");
    CHECK(g.deliver(1.0) == 4);
    CHECK_TRACE(g, "k4 (7,2,2,3) (1,2,2,5)");
    CHECK(g.at() == "7 7 0 7");
    g.feed.set_next_local(10);
    CHECK(g.feed.exhausted() && g.deliver(1.0) == 0);
    g.feed.set_seen_at_solve(5);
    CHECK(g.feed.seen_at_solve() == 5);
  }
  {  // errors of the C ABI carry the loop's prefix; the cursor stays
    static HostApi bad = [] {
      HostApi x = *host_api();
      x.window_insert_many = [](void*, const double*, int64_t) -> int64_t { return -1; };
      x.last_error = []() -> const char* { return "boom"; };
      return x;
    }();
    for (const char* who : {"BspLoop: ", "LanesLoop: ", "KeyRangeLoop: "}) {
      FeedRig g(4, 2, 0.0, 11, &bad, who);
      CHECK(error_of<std::runtime_error>([&] { g.deliver(1.0); }) == std::string(who) + "window insert: boom");
      CHECK(g.feed.next_local() == 0 && g.take().empty());
    }
  }
  {  // the cadence: new_rows 2, new_frac 0.5, new_cap 3, ramp 1 -- the first solves need
     // max(2, min(ceil(size / 2), 3, 1 << solves)) new tuples; rows arrive one per delivery
    LanesHostCfg c;
    c.new_rows = 2;
    c.new_frac = 0.5;
    c.new_cap = 3;
    c.new_ramp = 1;
    FeedRig g(1, 4);
    CHECK(!g.feed.solve_due(g.feed.window(), 0));  // no rows: never
    // deliveries until solve 0, 1, ... is due: 2 of windows of 1-2 and 3-4 rows (new_rows), then
    // ceil(size / 2) capped at 3 (new_cap; the ramp's 4 no longer binds)
    const int want[] = {2, 2, 3, 3, 3};
    const int64_t seen_then[] = {2, 4, 7, 10, 13};
    for (int solve = 0; solve < 5; ++solve) {
      int n = 0;
      ShardFeed::Window v = g.feed.window();
      CHECK(solve == 0 || !g.feed.solve_due(v, c.new_tuples_needed(v.size, solve)));
      CHECK(solve == 0 || g.feed.solve_due(v, 0));  // (no cadence: at once)
      while (!g.feed.solve_due(v, c.new_tuples_needed(v.size, solve)) && n < 10) {
        g.deliver(1.0);
        v = g.feed.window();
        ++n;
      }
      CHECK(n == want[solve] && v.seen == seen_then[solve]);
      g.feed.mark_solved(v.seen);
      CHECK(g.feed.seen_at_solve() == v.seen);
    }
    CHECK(c.new_tuples_needed(8) == 3 && c.new_tuples_needed(8, 0) == 2 && c.new_tuples_needed(8, 2) == 3);
    // a stream that ended solves on what it has
    ShardFeed::Window v = g.feed.window();
    CHECK(!g.feed.solve_due(v, 3));
    g.feed.set_next_local(20);
    CHECK(g.feed.exhausted() && g.feed.solve_due(v, 3));
  }
}

struct GateClock : HostClock {
  double now_ms() override { return t_ms; }
  int64_t mono_ns() override { return 0; }
  void idle_sleep(int us) override {
    ++sleeps;
    slept_us += us;
    t_ms += sleep_step_ms >= 0.0 ? sleep_step_ms : us / 1000.0;
  }
  double t_ms = 999.0;
  double sleep_step_ms = -1.0;  // the clock advances by this per sleep (< 0: the sleep's length)
  int sleeps = 0;
  int64_t slept_us = 0;
};

static void test_round_gate() {
  const char* const starved[] = {"BspLoop: no rows for 600 s", "LanesLoop: no rows for a worker",
                                 "KeyRangeLoop: no rows"};
  // the caller's hook: deliver for every lane, as the loops do; the times it was given
  std::vector<double> nows;
  auto deliver_all = [&](std::vector<FeedRig*> rigs) {
    return [&nows, rigs](double now) {
      nows.push_back(now);
      for (FeedRig* g : rigs) g->deliver(now);
    };
  };
  {  // ready at once: one delivery at the time since t0, no sleep, the window handed back
    GateClock clk;
    FeedRig g(4, 2);
    ShardFeed::Window v;
    const RoundGate gate{&clk, 900.0, 600.0, starved[0]};
    CHECK(gate.wait(&g.feed, 1, &v, deliver_all({&g})));
    CHECK(clk.sleeps == 0 && nows == std::vector<double>({99.0}));
    CHECK(v.size == 4 && v.start == 0 && v.seen == 4);
    CHECK_TRACE(g, "k4 (1,2,4,0)");
  }
  {  // waits for rows: the producer (clock mode) starts at 1000 ms, the round at 999 ms -- two
     // sleeps of 500 us, a delivery per try, ready on the third
    GateClock clk;
    FeedRig g(0, 2, 500.0);
    ShardFeed::Window v;
    nows.clear();
    const RoundGate gate{&clk, 1000.0, 600.0, starved[0]};
    CHECK(gate.wait(&g.feed, 1, &v, deliver_all({&g})));
    CHECK(clk.sleeps == 2 && clk.slept_us == 1000 && nows == std::vector<double>({-1.0, -0.5, 0.0}));
    CHECK(v.size == 5 && v.start == 0 && v.seen == 5);
    CHECK_TRACE(g, "k5 (1,2,5,0)");
  }
  {  // two lanes: lane 1's stream ended and its window is empty -- the run ends at once, lane 0's
     // rows of this try delivered (the caller flushes them)
    GateClock clk;
    FeedRig g0(4, 2), g1(4, 2);
    g1.feed.set_next_local(10);
    ShardFeed feeds[2] = {g0.feed, g1.feed};
    ShardFeed::Window v[2];
    int tries = 0;
    const RoundGate gate{&clk, 0.0, 600.0, starved[1]};
    CHECK(!gate.wait(feeds, 2, v, [&](double) {
      ++tries;
      for (ShardFeed& f : feeds) f.deliver(1.0, [](int64_t, int64_t, int64_t, int64_t) {});
    }));
    CHECK(tries == 1 && clk.sleeps == 0 && v[0].size == 4 && v[1].size == 0 && feeds[0].next_local() == 4);
    // ... but an ended stream whose window still has rows goes on solving
    g1.win.restore(2, 3, 3);
    CHECK(gate.wait(feeds, 2, v, [](double) {}) && v[1].size == 3 && v[1].seen == 3);
  }
  {  // the deadline: nothing is due (the producer starts at 5000 ms); the round that still waits
     // at 1000 ms is not run -- two sleeps from 999 ms
    GateClock clk;
    FeedRig g(0, 2, 500.0);
    ShardFeed::Window v;
    nows.clear();
    const RoundGate gate{&clk, 5000.0, 600.0, starved[1], 1000.0};
    CHECK(!gate.wait(&g.feed, 1, &v, deliver_all({&g})));
    CHECK(clk.sleeps == 2 && clk.t_ms == 1000.0 && nows.size() == 3 && v.size == 0);
    // no deadline (0): the same wait runs into the row timeout instead, below
  }
  for (const char* msg : starved) {  // no rows for longer than the budget (2 ms): the caller's message,
                                     // after the tries at 999, 999.5, ... 1001 ms (5 sleeps)
    GateClock clk;
    FeedRig g(0, 2, 500.0);
    ShardFeed::Window v;
    const RoundGate gate{&clk, 5000.0, 0.002, msg};
    CHECK(error_of<std::runtime_error>([&] { gate.wait(&g.feed, 1, &v, deliver_all({&g})); }) == msg);
    CHECK(clk.sleeps == 5 && clk.t_ms == 1001.5);
  }
  {  // the cadence alone holds the round back far beyond the row budget (2 ms): no timeout.  128
     // rows at 0, one more at 1000 ms and at 2000 ms; the round needs 130 tuples; the scripted
     // sleep takes 500 ms
    GateClock clk;
    clk.t_ms = 1000.0;
    clk.sleep_step_ms = 500.0;
    FeedRig g(0, 1, 500.0, 600);
    ShardFeed::Window v;
    nows.clear();
    int64_t asked = 0;
    const RoundGate gate{&clk, 1000.0, 0.002, starved[1]};
    CHECK(gate.wait(&g.feed, 1, &v, deliver_all({&g}), [&](int64_t size) {
      asked = size;
      return int64_t(130);
    }));
    CHECK(clk.sleeps == 4 && nows == std::vector<double>({0.0, 500.0, 1000.0, 1500.0, 2000.0}));
    CHECK(asked == 8 && v.size == 8 && v.seen == 130 && g.feed.next_local() == 130);
    CHECK_TRACE(g, "k16 (225,2,16,0)k1 (257,2,1,0)k1 (259,2,1,1)");
    // the next round counts from this solve: 130 seen, none new
    g.feed.mark_solved(v.seen);
    CHECK(!g.feed.solve_due(g.feed.window(), 1) && g.feed.solve_due(g.feed.window(), 0));
  }
}

// ---- FitLoop (csrc/solver/fit_loop.h): the controller loop of a full-batch fit ----
// A fitter in miniature on f(x) = 0.5 * sum a_i (x_i - c_i)^2: fp32 vectors as the
// kernels keep them (stride nv > n, history 2), "evaluate" fills the result block in
// fp64 as the reductions do, "apply" runs fit_update_body of fit_step.h per element.
struct QuadFit {
  int n = 3, nv = 4, H = 2;  // (the names fit_update_body reads)
  float xs[4] = {}, ds[4] = {}, gcs[4] = {}, gts[4] = {}, bts[4] = {}, Ss[8] = {}, Ys[8] = {};
  float *x = xs, *d = ds, *g_c = gcs, *g_t = gts, *beta_t = bts, *S = Ss, *Y = Ys;
  double a[3] = {1e-5, 1e-4, 1e-3}, c[3] = {1.0, -2.0, 0.5};
  double pin[kFitOutWords] = {};
  bool nan_objective = false;
  FitLoop loop;
  QuadFit() = default;
  QuadFit(const QuadFit&) = delete;

  void begin(double off, const FitOpts& o) {  // start at c + off * (1, -1, 1)
    for (int i = 0; i < n; ++i) x[i] = beta_t[i] = (float)(c[i] + (i == 1 ? -off : off));
    loop.start(o, H);
  }
  void evaluate(double reg) {
    double f = 0.0, bb = 0.0;
    for (int i = 0; i < n; ++i) {
      const double r = (double)beta_t[i] - c[i];
      f += 0.5 * a[i] * r * r;
      bb += (double)beta_t[i] * beta_t[i];
      g_t[i] = (float)(a[i] * r + reg * beta_t[i]);
    }
    double* dots = pin + kFitOutDots;  // num_dots(H) dots, then ||beta||^2
    for (int k = 0; k <= num_dots(H); ++k) dots[k] = 0.0;
    for (int i = 0; i < n; ++i) {
      const double g = g_t[i];
      dots[0] += g * g;
      dots[1] += g * d[i];
      dots[2] += g * g_c[i];
      for (int h = 0; h < H; ++h) {
        dots[3 + h] += (double)S[h * nv + i] * g;
        dots[3 + H + h] += (double)Y[h * nv + i] * g;
      }
    }
    dots[num_dots(H)] = bb;
    pin[kFitOutLoss] = f;
    pin[kFitOutF] = nan_objective ? std::nan("") : f + 0.5 * reg * bb;
  }
  bool run(int max_accept) {
    return loop.run(
        max_accept, pin, [&](double reg) { evaluate(reg); },
        [&](const FitStep& st) {
          for (int e = 0; e < n; ++e) fit_update_body(*this, st, e, [&](int i, float bt) { beta_t[i] = bt; });
        });
  }
};

static void test_fit_loop() {
  FitOpts o;
  o.max_iter = 50;
  o.tol = 1e-3;
  std::vector<double> whole;
  {  // a converging run: ends by a tolerance test within the budget, the objective falls at every accepted step
    QuadFit q;
    q.begin(1000.0, o);
    CHECK(q.run(1 << 30) && q.loop.done() && q.loop.reason() == "tol");
    const Ctrl& k = q.loop.ctrl();
    const std::vector<double>& h = q.loop.history();
    CHECK(k.nacc > q.H + 1 && k.nacc < o.max_iter && k.evals >= k.nacc + 1);  // the ring of 2 pairs wrapped
    CHECK((int)h.size() == k.nacc + 1 && h.back() == k.f_c);
    for (size_t i = 1; i < h.size(); ++i) CHECK(h[i] < h[i - 1]);
    // "tol" is ctrl_accept's done = gnorm <= tol * fscale || |f_prev - f_t| <= tol * fscale with
    // fscale = max(1, |f_t|), gnorm^2 = dots[0] = sum g_t_i^2 over the fp32 gradient the evaluation
    // stored.  The inputs are chosen so that the gradient test is the one that fires (a_i <= tol: near the
    // minimum f = 0.5 sum g_i^2 / a_i still falls by more than tol a step when |g| is already below it);
    // both tests are re-evaluated here.  The accepted x is exactly the evaluated point,
    // so g_t is still the gradient at x: |g_t_i| <= gnorm <= tol * fscale.  g_t_i is the fp32 rounding of
    // a_i (x_i - c_i) formed in fp64, hence a_i |x_i - c_i| <= |g_t_i| (1 + 2^-23) (the fp32 rounding is
    // 2^-24 relative, the two fp64 roundings 2^-53 each), and
    //   |x_i - c_i| <= tol * fscale * (1 + 2^-23) / a_i.
    const double fscale = std::fabs(h.back()) > 1.0 ? std::fabs(h.back()) : 1.0, lim = (double)(float)o.tol * fscale;
    double tt = 0.0;
    for (int i = 0; i < q.n; ++i) tt += (double)q.g_t[i] * q.g_t[i];
    CHECK(std::sqrt(tt) <= lim && !(std::fabs(h[h.size() - 2] - h.back()) <= lim));
    for (int i = 0; i < q.n; ++i) {
      CHECK(q.x[i] == q.beta_t[i]);
      CHECK(std::fabs((double)q.x[i] - q.c[i]) <= lim * (1.0 + std::ldexp(1.0, -23)) / q.a[i]);
    }
    whole = h;
  }
  {  // the same fit one accepted step per call: false until the last call, which returns true
    QuadFit q;
    q.begin(1000.0, o);
    const int last = (int)whole.size() - 1;
    for (int it = 1; it <= last; ++it) {
      CHECK(q.run(1) == (it == last));
      CHECK(q.loop.ctrl().nacc == it && q.loop.done() == (it == last));
    }
    CHECK(q.loop.reason() == "tol" && q.loop.history() == whole);
    CHECK(q.run(1) && q.loop.ctrl().nacc == last);  // an ended fit evaluates nothing more
  }
  {  // no iteration allowed: the start is evaluated once and is the result
    QuadFit q;
    FitOpts z = o;
    z.max_iter = 0;
    q.begin(1000.0, z);
    CHECK(q.run(1 << 30) && q.loop.reason() == "max_iter");
    CHECK(q.loop.ctrl().evals == 1 && q.loop.ctrl().nacc == 0 && q.loop.history().size() == 1);
  }
  {  // one iteration allowed: exactly one accepted step
    QuadFit q;
    FitOpts z = o;
    z.max_iter = 1;
    q.begin(1000.0, z);
    CHECK(q.run(1 << 30) && q.loop.reason() == "max_iter");
    CHECK(q.loop.ctrl().nacc == 1 && q.loop.history().size() == 2 && q.loop.history()[1] < q.loop.history()[0]);
  }
  {  // a NaN objective at the start
    QuadFit q;
    q.nan_objective = true;
    q.begin(1000.0, o);
    CHECK(q.run(1 << 30) && q.loop.reason() == "no_descent");
    CHECK(q.loop.ctrl().evals == 1 && q.loop.ctrl().nacc == 0);
  }
  {  // a line search of one evaluation whose first trial overshoots.  The first step is x - g / ||g||, of
    // length 1; 0.001 away from c in every coordinate that is far past the minimum along -g: phi(t) =
    // f - t ||g||^2 + 0.5 t^2 g'Ag rises at t = 1 / ||g|| once 0.5 g'Ag / ||g||^2 (>= 0.5 a_min = 5e-6)
    // exceeds ||g|| (<= a_max * 0.001 * sqrt(3) < 2e-6), so sufficient decrease fails
    QuadFit q;
    FitOpts z = o;
    z.ls_max = 1;
    q.begin(0.001, z);
    CHECK(q.run(1 << 30) && q.loop.reason() == "line_search");
    CHECK(q.loop.ctrl().evals == 2 && q.loop.ctrl().nacc == 0 && q.loop.ctrl().ls_fail == 1);
    CHECK(q.loop.history().size() == 1);
  }
  {  // run without a fit in progress: before start, and after stop (a new dataset, a single evaluation)
    QuadFit q;
    CHECK(error_of<std::runtime_error>([&] { q.run(1); }) == "fit: begin() first");
    q.begin(1000.0, o);
    CHECK(!q.run(1) && !q.loop.done());
    q.loop.stop();
    CHECK(q.loop.done() && !q.loop.begun());
    CHECK(error_of<std::runtime_error>([&] { q.run(1); }) == "fit: begin() first");
    CHECK(error_of<std::invalid_argument>([&] {
            FitOpts bad = o;
            bad.ls_max = 0;
            q.loop.start(bad, q.H);
          }) == "fit: bad max_iter / ls_max / tol");
  }
}

// dispatch.h: a run-time value reaches the functor as the matching compile-time
// constant exactly once; a value outside the list throws and calls nothing.
static void test_dispatch() {
  const int list[] = {128, 256, 512, 1024, 2048};
  for (int v : list) {  // every listed value, the first, a middle one and the last among them
    int calls = 0, got = 0;
    dispatch_int<128, 256, 512, 1024, 2048>("width", v, [&](auto c) {
      static_assert(std::is_same<decltype(c), std::integral_constant<int, c()>>::value, "a constant, not an int");
      ++calls;
      got = c();
    });
    CHECK(calls == 1 && got == v);
    calls = got = 0;
    dispatch_fp("width", v, [&](auto c) {
      ++calls;
      got = c();
    });
    CHECK(calls == 1 && got == v);
  }
  for (int kp : {1, 2, 4, 8, 16}) {  // nested: the pair arrives together
    int calls = 0, gf = 0, gk = 0;
    dispatch_fp("width", 512, [&](auto fp) {
      dispatch_wide_kp("classes", kp, [&](auto k) {
        constexpr int product = fp() * k();  // both usable as template arguments in there
        ++calls;
        gf = fp();
        gk = product / fp();
      });
    });
    CHECK(calls == 1 && gf == 512 && gk == kp);
  }
  for (int v : {0, -1, 3, 127, 192, 2047, 4096}) {
    int calls = 0;
    const std::string e =
        error_of<std::invalid_argument>([&] { dispatch_fp("fit: padded width", v, [&](auto) { ++calls; }); });
    CHECK(calls == 0);
    CHECK(e.find("fit: padded width") != std::string::npos && e.find(std::to_string(v)) != std::string::npos);
  }
  {  // an inner value outside its list: the outer functor ran, the inner did not
    int outer = 0, inner = 0;
    const std::string e = error_of<std::invalid_argument>([&] {
      dispatch_fp("width", 128, [&](auto) {
        ++outer;
        dispatch_int<2, 4, 8>("classes", 16, [&](auto) { ++inner; });
      });
    });
    CHECK(outer == 1 && inner == 0 && e.find("classes") != std::string::npos && e.find("16") != std::string::npos);
  }
  std::vector<int> seen;
  for_each_int<2, 4, 8, 16>([&](auto c) { seen.push_back(c()); });
  CHECK((seen == std::vector<int>{2, 4, 8, 16}));
  seen.clear();
  for_each_fp([&](auto c) { seen.push_back(c()); });
  CHECK((seen == std::vector<int>(list, list + 5)));
  seen.clear();
  for_each_wide_kp([&](auto c) { seen.push_back(c()); });
  CHECK((seen == std::vector<int>{1, 2, 4, 8, 16}));
  // the wide solver's quarter-waves per ring row
  const int nz[] = {1, 64, 65, 129, 256, 257, 512}, nq[] = {1, 1, 2, 4, 4, 8, 8};
  for (int i = 0; i < 7; ++i) CHECK(wide_quarters(nz[i]) == nq[i]);
  CHECK(wide_quarters(128) == 2 && wide_quarters(513) == 16);  // (past the widest ring: no listed value)
}

int main() {
  test_dispatch();
  test_tracker();
  test_tracker_faults();
  test_libsvm();
  test_window();
  test_ctrl_queue();
  test_csv();
  test_metrics_sink();
  test_server_protocol();
  test_lanes_protocol();
  test_shard_feed();
  test_round_gate();
  test_fit_loop();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("host selftest: all checks passed\n");
  return 0;
}
