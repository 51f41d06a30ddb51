// Host-side helpers of the launchers: alignment, grid clamps, carving a workspace, and turning a runtime width or flag into
// a compile-time constant handed to a generic lambda (the `if constexpr` guards at the call sites keep the combinations
// that have no kernel from being instantiated).  No device code.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace {

// x rounded up to a multiple of a (a power of two), in x's own integer type
template <class T>
constexpr T gcr_align(T x, int64_t a) { return (x + (T)(a - 1)) & ~(T)(a - 1); }

// workgroups to launch: `want` clamped to [floor, cap]
constexpr int64_t gcr_grid(int64_t want, int64_t cap, int64_t floor = 1) {
  return want > cap ? cap : (want < floor ? floor : want);
}

// every pointer 16-byte aligned (NULL counts as aligned)
template <class... P>
bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// Consecutive regions of one workspace: take() returns the offset of the next region and moves `at` past it, the region
// padded to a multiple of `align`.  Offsets, counts and `at` share one unit (bytes or 4-byte words: the layout says which);
// the total is `at` after the last take().
struct WsCarve {
  int64_t at = 0;
  int64_t take(int64_t count, int64_t align = 64) {
    const int64_t offset = at;
    at += gcr_align(count, align);
    return offset;
  }
};

// f(std::integral_constant<int, V>{}) for the first V equal to v; the last V also takes every other v (the callers have
// refused unsupported values before they dispatch)
template <int V0, int... V, class F>
auto dispatch_value(int v, F&& f) {
  if constexpr (sizeof...(V) == 0) {
    return f(std::integral_constant<int, V0>{});
  } else {
    if (v == V0) return f(std::integral_constant<int, V0>{});
    return dispatch_value<V...>(v, std::forward<F>(f));
  }
}

// the same for kernels templated on NV = the 64-column groups a lane owns: the first NV with d <= 64 NV, else the last
template <int NV0, int... NV, class F>
auto dispatch_columns(int d, F&& f) {
  if constexpr (sizeof...(NV) == 0) {
    return f(std::integral_constant<int, NV0>{});
  } else {
    if (d <= 64 * NV0) return f(std::integral_constant<int, NV0>{});
    return dispatch_columns<NV...>(d, std::forward<F>(f));
  }
}

template <class F>
void dispatch_bool(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }

}  // namespace
