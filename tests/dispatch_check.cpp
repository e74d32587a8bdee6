// Stand-alone host check of dalm_amd/csrc/dispatch.hpp (built and run by tests/test_abi.py with a plain C++17 compiler under
// -fsanitize=address,undefined; no HIP, no GPU): the selection rules at their edges, the dtype and bool tags, aligned16, round_up.
#include <stdio.h>
#include <type_traits>

#include "dispatch.hpp"

static int failures = 0;
#define CHECK(cond) \
  do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static int ceil_chunks(int n) { return dalm::by_ceil<1, 2, 4, 8, 16>(n, [](auto v) { return static_cast<int>(v); }); }
static int exact_chunks(int n) { return dalm::by_exact<1, 2, 3, 4>(n, [](auto v) { return static_cast<int>(v); }); }
static int exact_rank(int n) { return dalm::by_exact<8, 16>(n, [](auto v) { return static_cast<int>(v); }); }
static int dtype_size(int code) {
  return dalm::by_dtype(code, [](auto t) { return static_cast<int>(sizeof(typename decltype(t)::type)); });
}

int main() {
  // "first listed value >= n, else the last"
  const int n_ceil[] = {0, 1, 2, 3, 8, 9, 16, 17}, want_ceil[] = {1, 1, 2, 4, 8, 16, 16, 16};
  for (int i = 0; i < 8; ++i) CHECK(ceil_chunks(n_ceil[i]) == want_ceil[i]);
  CHECK(ceil_chunks(4) == 4 && ceil_chunks(5) == 8 && ceil_chunks(-3) == 1);
  CHECK((dalm::by_ceil<7>(100, [](auto v) { return static_cast<int>(v); }) == 7));   // a ladder of one value
  // "exact match, else the last"
  const int n_exact[] = {1, 3, 4, 7}, want_exact[] = {1, 3, 4, 4};
  for (int i = 0; i < 4; ++i) CHECK(exact_chunks(n_exact[i]) == want_exact[i]);
  CHECK(exact_chunks(2) == 2 && exact_chunks(0) == 4);
  CHECK(exact_rank(8) == 8 && exact_rank(16) == 16 && exact_rank(12) == 16);
  // the tag is a compile-time constant inside the lambda
  dalm::by_ceil<1, 2, 4>(3, [](auto v) {
    static_assert(std::is_same_v<decltype(v), std::integral_constant<int, 1>> || std::is_same_v<decltype(v), std::integral_constant<int, 2>> ||
                  std::is_same_v<decltype(v), std::integral_constant<int, 4>>);
    CHECK((std::integral_constant<int, v>::value == 4));                            // usable as a template argument, as launchers do
  });
  // dtype codes and flags
  CHECK(dtype_size(DALM_F32) == 4 && dtype_size(DALM_BF16) == 2);
  CHECK(dalm::by_bool(true, [](auto b) { return std::is_same_v<decltype(b), std::true_type>; }));
  CHECK(dalm::by_bool(false, [](auto b) { return std::is_same_v<decltype(b), std::false_type>; }));
  int launched = 0;
  dalm::by_bool(true, [&](auto b) { launched += b ? 1 : 100; });                    // a lambda that returns nothing
  CHECK(launched == 1);
  // aligned16: NULL counts as aligned, one misaligned pointer among aligned ones does not
  alignas(16) static float buf[8];
  const float* null_f = nullptr;
  const void* null_v = nullptr;
  CHECK(dalm::aligned16(buf) && dalm::aligned16(buf + 4) && dalm::aligned16(null_f) && dalm::aligned16(null_v));
  CHECK(!dalm::aligned16(buf + 1) && !dalm::aligned16(buf + 2) && !dalm::aligned16(reinterpret_cast<const char*>(buf) + 8));
  CHECK(dalm::aligned16(buf, null_f, buf + 4) && !dalm::aligned16(buf, null_f, buf + 3) && !dalm::aligned16(buf + 1, buf));
  CHECK(dalm::rows_aligned16(buf, 8) && !dalm::rows_aligned16(buf, 6) && !dalm::rows_aligned16(buf + 1, 8));
  CHECK(dalm::round_up(0, 4) == 0 && dalm::round_up(1, 4) == 4 && dalm::round_up(4, 4) == 4 && dalm::round_up(33, 32) == 64);
  if (failures) return 1;
  puts("dispatch ok");
  return 0;
}
