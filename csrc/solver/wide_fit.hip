#include "wide_fit.h"

#include <chrono>
#include <climits>
#include <stdexcept>

#include "solver.h"

namespace psx {

static size_t wfit_align(size_t v) { return (v + 255) / 256 * 256; }

WideBatchFitter::WideBatchFitter(int K, int KP, int hist, int max_wg) : max_wg_(max_wg) {
  if (K < 1 || K > 16) throw std::invalid_argument("num classes must be in [1,16]");
  if (KP < K || (KP != 1 && KP != 2 && KP != 4 && KP != 8 && KP != 16))
    throw std::invalid_argument("padded classes must be 1, 2, 4, 8 or 16 and >= K");
  if (hist < 1 || hist > kMaxHist) throw std::invalid_argument("history must be in [1,16]");
  if (max_wg_ <= 0) {
    int dev = 0;
    hipDeviceProp_t p;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    hip_check(hipGetDeviceProperties(&p, dev), "hipGetDeviceProperties");
    max_wg_ = 8 * p.multiProcessorCount;  // the row pass is a gather: every wave slot of a CU taken
  }
  dv_.K = K;
  dv_.KP = KP;
  dv_.H = hist;
  hip_check(hipHostMalloc(reinterpret_cast<void**>(&pin_), kFitOutWords * sizeof(double), hipHostMallocDefault),
            "hipHostMalloc(fit result block)");
}

WideBatchFitter::~WideBatchFitter() {
  if (ws_) (void)hipFree(ws_);
  if (pin_) (void)hipHostFree(pin_);
}

void WideBatchFitter::set_data(const WideFitData& d, hipStream_t s) {
  if (d.N < 1 || d.N >= INT_MAX - 64) throw std::invalid_argument("row count must be in [1, 2^31 - 64)");
  if (d.U < 0 || (d.U + 1) * (int64_t)dv_.KP >= INT_MAX)
    throw std::invalid_argument("touched features * padded classes must stay below 2^31");
  if (d.F < 1 || d.n_items < d.U || d.n_items >= INT_MAX || d.n_short < 0 || d.n_long < 0 ||
      d.n_short + d.n_long != d.n_items)
    throw std::invalid_argument("inconsistent work-item list");
  if (!d.indptr || !d.y || (d.U > 0 && (!d.col || !d.val || !d.uniq || !d.colptr || !d.crow || !d.cval ||
                                        !d.item_begin || !d.item_end || !d.col_item0)) ||
      (d.n_short > 0 && !d.short_items) || (d.n_long > 0 && !d.long_items))
    throw std::invalid_argument("null dataset pointer");
  loop_.stop();
  if (ws_) {
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    hip_check(hipFree(ws_), "hipFree(wide fit workspace)");
    ws_ = nullptr;
  }
  const int K = dv_.K, KP = dv_.KP, H = dv_.H;
  dv_ = WideFitDev{};
  dv_.K = K;
  dv_.KP = KP;
  dv_.H = H;
  static_cast<WideFitData&>(dv_) = d;
  dv_.n = (int)((d.U + 1) * KP);
  dv_.nv = (int)(((int64_t)dv_.n + 63) / 64 * 64);
  const int64_t nwg = (d.N + 3) / 4;
  G_ = (int)(nwg < max_wg_ ? nwg : max_wg_);
  dv_.W = 4 * G_;
  const size_t nv = dv_.nv, U1 = (size_t)d.U + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = wfit_align(off + bytes);
    return o;
  };
  const size_t o_x = take(nv * 4), o_d = take(nv * 4), o_gc = take(nv * 4), o_gt = take(nv * 4), o_bt = take(nv * 4);
  const size_t o_S = take(H * nv * 4), o_Y = take(H * nv * 4), o_wfix = take(nv * 4), o_weff = take(nv * 4);
  const size_t o_std = take(U1 * 4), o_istd = take(U1 * 4);
  const size_t o_R = take((size_t)d.N * KP * 4), o_gitem = take(((size_t)d.n_items + 1) * KP * 4);
  const size_t o_part = take((size_t)dv_.W * 32 * 4), o_bsum = take(16 * 4);
  const size_t o_dpart = take((size_t)wide_fit_reduce_grid(dv_.n) * kFitDotStride * 8);
  const size_t o_out = take((size_t)kFitOutWords * 8);
  hip_check(hipMalloc(&ws_, off), "hipMalloc(wide fit workspace)");
  hip_check(hipMemsetAsync(ws_, 0, off, s), "hipMemsetAsync(wide fit workspace)");
  char* b = static_cast<char*>(ws_);
  dv_.x = reinterpret_cast<float*>(b + o_x);
  dv_.d = reinterpret_cast<float*>(b + o_d);
  dv_.g_c = reinterpret_cast<float*>(b + o_gc);
  dv_.g_t = reinterpret_cast<float*>(b + o_gt);
  dv_.beta_t = reinterpret_cast<float*>(b + o_bt);
  dv_.S = reinterpret_cast<float*>(b + o_S);
  dv_.Y = reinterpret_cast<float*>(b + o_Y);
  dv_.wfix = reinterpret_cast<float*>(b + o_wfix);
  dv_.weff = reinterpret_cast<float*>(b + o_weff);
  dv_.std_ = reinterpret_cast<float*>(b + o_std);
  dv_.inv_std = reinterpret_cast<float*>(b + o_istd);
  dv_.R = reinterpret_cast<float*>(b + o_R);
  dv_.gitem = reinterpret_cast<float*>(b + o_gitem);
  dv_.part = reinterpret_cast<float*>(b + o_part);
  dv_.bsum = reinterpret_cast<float*>(b + o_bsum);
  dv_.dpart = reinterpret_cast<double*>(b + o_dpart);
  dv_.out = reinterpret_cast<double*>(b + o_out);
  launch_wide_fit_stats(dv_, s);
  hip_check(hipGetLastError(), "wide_fit_stats launch");
}

void WideBatchFitter::evaluate(double reg, int raw, hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  launch_wide_fit_rows(dv_, G_, s);
  launch_wide_fit_cols(dv_, s);
  launch_wide_fit_reduce(dv_, reg, raw, s);
  hip_check(hipGetLastError(), "wide fit evaluation launch");
  hip_check(hipMemcpyAsync(pin_, dv_.out, kFitOutWords * sizeof(double), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(fit result block)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(wide fit evaluation)");
  eval_s_.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

double WideBatchFitter::loss_grad(const float* w, float* grad, hipStream_t s) {
  if (!ws_) throw std::runtime_error("loss_grad: no dataset (set_data first)");
  if (!w || !grad) throw std::invalid_argument("loss_grad: null weights or gradient buffer");
  loop_.stop();  // the trial weights are overwritten
  launch_wide_fit_begin(dv_, w, 1, /*raw=*/1, s);
  evaluate(0.0, /*raw=*/1, s);
  eval_s_.pop_back();
  hip_check(hipMemsetAsync(grad, 0, ((size_t)dv_.F + 1) * dv_.KP * 4, s), "hipMemsetAsync(gradient)");
  launch_wide_fit_scatter(dv_, dv_.g_t, grad, s);
  hip_check(hipGetLastError(), "wide_fit_scatter launch");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(loss_grad)");
  return pin_[kFitOutLoss];
}

void WideBatchFitter::begin(const float* w0, const FitOpts& o, hipStream_t s) {
  if (!ws_) throw std::runtime_error("fit: no dataset (set_data first)");
  if (dv_.N < 2) throw std::invalid_argument("fit: at least 2 rows are needed");
  loop_.start(o, dv_.H);
  eval_s_.clear();
  launch_wide_fit_begin(dv_, w0, o.zero_const, /*raw=*/0, s);
  hip_check(hipGetLastError(), "wide_fit_begin launch");
}

bool WideBatchFitter::run(int max_accept, hipStream_t s) {
  return loop_.run(
      max_accept, pin_, [&](double reg) { evaluate(reg, 0, s); },
      [&](const FitStep& st) {
        launch_wide_fit_update(dv_, st, s);
        hip_check(hipGetLastError(), "wide_fit_update launch");
      });
}

void WideBatchFitter::current(float* w_out, hipStream_t s) {
  if (!loop_.begun()) throw std::runtime_error("fit: begin() first");
  if (!w_out) throw std::invalid_argument("fit: null output buffer");
  launch_wide_fit_finalize(dv_, loop_.opts().reg_param == 0.0, w_out, s);
  hip_check(hipGetLastError(), "wide_fit_finalize launch");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(wide_fit_finalize)");
}

namespace {
struct StageEvents {  // four events, destroyed whatever happens in between
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  StageEvents() {
    for (auto& e : ev) hip_check(hipEventCreate(&e), "hipEventCreate");
  }
  ~StageEvents() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  StageEvents(const StageEvents&) = delete;
  StageEvents& operator=(const StageEvents&) = delete;
};
}  // namespace

std::vector<float> WideBatchFitter::stage_ms(int raw, hipStream_t s) {
  if (!ws_) throw std::runtime_error("stage_ms: no dataset (set_data first)");
  StageEvents t;
  hip_check(hipEventRecord(t.ev[0], s), "hipEventRecord");
  launch_wide_fit_rows(dv_, G_, s);
  hip_check(hipEventRecord(t.ev[1], s), "hipEventRecord");
  launch_wide_fit_cols(dv_, s);
  hip_check(hipEventRecord(t.ev[2], s), "hipEventRecord");
  launch_wide_fit_reduce(dv_, 0.0, raw, s);
  hip_check(hipEventRecord(t.ev[3], s), "hipEventRecord");
  hip_check(hipEventSynchronize(t.ev[3]), "hipEventSynchronize");
  std::vector<float> ms(3);
  for (int i = 0; i < 3; ++i) hip_check(hipEventElapsedTime(&ms[i], t.ev[i], t.ev[i + 1]), "hipEventElapsedTime");
  return ms;
}

void WideBatchFitter::read_std(float* std_out, hipStream_t s) {
  if (!ws_) throw std::runtime_error("read_std: no dataset (set_data first)");
  hip_check(hipMemcpyAsync(std_out, dv_.std_, (size_t)dv_.U * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(std)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(std)");
}

void WideBatchFitter::read_state(float* x, float* d, float* g_c, float* g_t, float* beta_t, float* wfix, float* S,
                                 float* Y, hipStream_t s) {
  if (!ws_) throw std::runtime_error("read_state: no dataset (set_data first)");
  const size_t nv = (size_t)dv_.nv, H = (size_t)dv_.H;
  const struct {
    float* dst;
    const float* src;
    size_t words;
  } parts[] = {{x, dv_.x, nv},           {d, dv_.d, nv},       {g_c, dv_.g_c, nv}, {g_t, dv_.g_t, nv},
               {beta_t, dv_.beta_t, nv}, {wfix, dv_.wfix, nv}, {S, dv_.S, H * nv}, {Y, dv_.Y, H * nv}};
  for (const auto& p : parts)
    if (p.dst)
      hip_check(hipMemcpyAsync(p.dst, p.src, p.words * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(fit state)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit state)");
}

}  // namespace psx
