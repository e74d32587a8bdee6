// How a launcher turns run-time facts (dtype code, flags, chunk counts, rank) into template arguments: each helper picks a
// tag type and calls a generic lambda with it, so a launcher names its kernel once and casts each argument once.
//   by_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type; ... });
//   by_bool(flag, [&](auto on) { ... kernel<T, on> ... });
//   by_ceil<1, 2, 4, 8, 16>(n, [&](auto nch) { ... kernel<T, nch> ... });
// A launcher must not instantiate a kernel that no path can launch: where a ladder is not rectangular, the lambda says so
// with `if constexpr`.  Host-only, plain C++17 (no HIP).
#pragma once
#include <stdint.h>
#include <type_traits>
#include "../../include/dalm_hip.h"
#include "bf16.hpp"

namespace dalm {

// every pointer 16-byte aligned (NULL counts as aligned: optional tensors pass through)
template <typename... P>
inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t{0}) & 15) == 0; }

// f32 rows of stride `ld` elements that 16-byte loads can walk
inline bool rows_aligned16(const float* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

inline int64_t round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }

template <typename T> struct type_tag { using type = T; };

// DALM_F32 -> float, anything else (DALM_BF16: the entry points have checked the code) -> bf16_t
template <typename F>
inline auto by_dtype(int dtype, F&& f) { return dtype == DALM_F32 ? f(type_tag<float>{}) : f(type_tag<bf16_t>{}); }

template <typename F>
inline auto by_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// the first listed value >= n, else the last: chunk ladders such as 1, 2, 4, 8, 16
template <int V, int... Rest, typename F>
inline auto by_ceil(int n, F&& f) {
  if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
  else return n <= V ? f(std::integral_constant<int, V>{}) : by_ceil<Rest...>(n, f);
}

// the listed value equal to n, else the last: case 1 / 2 / 3 / default 4, rank 8 / 16
template <int V, int... Rest, typename F>
inline auto by_exact(int n, F&& f) {
  if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
  else return n == V ? f(std::integral_constant<int, V>{}) : by_exact<Rest...>(n, f);
}

}  // namespace dalm
