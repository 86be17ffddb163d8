// Run-time value -> template argument, written once.  No HIP in here: the host
// self-test includes it under g++.
//
//   dispatch_int<128, 256, 512>("fit: padded width", fp, [&](auto FP) {
//     kernel<FP()><<<G, 256, lb, s>>>(...);
//   });
//
// calls the functor with std::integral_constant<int, V> for the one listed V equal to
// the value and throws std::invalid_argument for any other: a launch site cannot
// return as if it had launched.  for_each_int visits every listed value in order, so
// an attribute list ranges over the same text as the launches it prepares.
// Two-parameter sites nest two calls.  Flags (scope, LE, MT, HIST, PAIR) keep an if.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

namespace psx {

template <int... Vs, class F>
void dispatch_int(const char* what, int v, F&& f) {
  const bool hit = ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  if (!hit) throw std::invalid_argument(std::string(what) + ": unsupported value " + std::to_string(v));
}

template <int... Vs, class F>
void for_each_int(F&& f) {
  (f(std::integral_constant<int, Vs>{}), ...);
}

// The lists several families share: the five padded row widths ...
template <class F>
void dispatch_fp(const char* what, int fp, F&& f) {
  dispatch_int<128, 256, 512, 1024, 2048>(what, fp, std::forward<F>(f));
}
template <class F>
void for_each_fp(F&& f) {
  for_each_int<128, 256, 512, 1024, 2048>(std::forward<F>(f));
}
// ... and the wide (sparse) model's five padded class counts.
template <class F>
void dispatch_wide_kp(const char* what, int kp, F&& f) {
  dispatch_int<1, 2, 4, 8, 16>(what, kp, std::forward<F>(f));
}
template <class F>
void for_each_wide_kp(F&& f) {
  for_each_int<1, 2, 4, 8, 16>(std::forward<F>(f));
}

// Bucketed values are computed by one small function and then dispatched exactly.
// The wide solver's NQ: quarter-waves per ring row, ceil(NZ / 64) rounded up to a
// power of two (1/2/4/8 for NZ <= 512, the widest ring WideSolver accepts).
inline int wide_quarters(int NZ) {
  const int q = NZ > 64 ? (NZ - 1) / 64 + 1 : 1;
  int nq = 1;
  while (nq < q) nq *= 2;
  return nq;
}

}  // namespace psx
