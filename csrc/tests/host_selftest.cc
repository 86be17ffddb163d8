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
//   real tracker and token queue with a scripted data plane.
// Exit status 0 = all checks passed.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../host/ctrl.h"
#include "../host/dataset.h"
#include "../host/libsvm.h"
#include "../host/logger.h"
#include "../host/metrics_sink.h"
#include "../host/sampling.h"
#include "../host/server_protocol.h"
#include "../host/tracker.h"

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

int main() {
  test_tracker();
  test_tracker_faults();
  test_libsvm();
  test_window();
  test_ctrl_queue();
  test_csv();
  test_metrics_sink();
  test_server_protocol();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("host selftest: all checks passed\n");
  return 0;
}
