#include "wide_fit.h"

#include <climits>
#include <stdexcept>

#include "solver.h"

namespace psx {

// the row pass is a gather: every wave slot of a CU taken
WideBatchFitter::WideBatchFitter(int K, int KP, int hist, int max_wg) : FitDriver(max_wg, 8) {
  if (K < 1 || K > 16) throw std::invalid_argument("num classes must be in [1,16]");
  if (KP < K || (KP != 1 && KP != 2 && KP != 4 && KP != 8 && KP != 16))
    throw std::invalid_argument("padded classes must be 1, 2, 4, 8 or 16 and >= K");
  if (hist < 1 || hist > kMaxHist) throw std::invalid_argument("history must be in [1,16]");
  dv_.K = K;
  dv_.KP = KP;
  dv_.H = hist;
}

WideBatchFitter::~WideBatchFitter() {
  if (ws_) (void)hipFree(ws_);
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
  end_fit();
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
  const size_t U1 = (size_t)d.U + 1;
  auto layout = [&](Carver& c) {
    carve_fit_vectors(c, dv_, wide_fit_reduce_grid(dv_.n));
    c.take(dv_.weff, (size_t)dv_.nv), c.take(dv_.std_, U1), c.take(dv_.inv_std, U1);
    c.take(dv_.R, (size_t)d.N * KP), c.take(dv_.gitem, ((size_t)d.n_items + 1) * KP);
    c.take(dv_.part, (size_t)dv_.W * 32), c.take(dv_.bsum, 16);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&ws_, size.off), "hipMalloc(wide fit workspace)");
  hip_check(hipMemsetAsync(ws_, 0, size.off, s), "hipMemsetAsync(wide fit workspace)");
  Carver place{static_cast<char*>(ws_)};
  layout(place);
  launch_wide_fit_stats(dv_, s);
  hip_check(hipGetLastError(), "wide_fit_stats launch");
}

FitVectors WideBatchFitter::vectors() const {
  return {dv_.n, dv_.nv, dv_.H, dv_.x, dv_.d, dv_.g_c, dv_.g_t, dv_.beta_t, dv_.S, dv_.Y, dv_.wfix, dv_.out};
}

void WideBatchFitter::launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) {
  launch_wide_fit_begin(dv_, w0, zero_const, raw, s);
}

void WideBatchFitter::launch_eval(double reg, int raw, hipStream_t s) {
  launch_wide_fit_rows(dv_, G_, s);
  launch_wide_fit_cols(dv_, s);
  launch_wide_fit_reduce(dv_, reg, raw, s);
}

void WideBatchFitter::launch_update(const FitStep& st, hipStream_t s) { launch_wide_fit_update(dv_, st, s); }

void WideBatchFitter::launch_finalize(int center, float* w_out, hipStream_t s) {
  launch_wide_fit_finalize(dv_, center, w_out, s);
}

void WideBatchFitter::export_grad(float* grad, hipStream_t s) {
  hip_check(hipMemsetAsync(grad, 0, ((size_t)dv_.F + 1) * dv_.KP * 4, s), "hipMemsetAsync(gradient)");
  launch_wide_fit_scatter(dv_, dv_.g_t, grad, s);
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

}  // namespace psx
