// grow.h -- the size of a buffer that grows on demand (DevBuf::reserve,
// host.h).  The sizes are behaviour, so the arithmetic is written once, here.
// Nothing from HIP: a CPU program compiles it (tests/test_host_growth.py).
#pragma once
#include <cstdint>

namespace avh {

// need + need / 4, raised to `floor`, then cut to `ceil`, then rounded up to
// `align` (a power of two)
struct Growth {
  int64_t floor = 0, ceil = INT64_MAX, align = 1;
};
constexpr int64_t grown_capacity(int64_t need, const Growth& g = {}) {
  int64_t want = need + need / 4;
  if (want < g.floor) want = g.floor;
  if (want > g.ceil) want = g.ceil;
  return (want + g.align - 1) & ~(g.align - 1);
}

}  // namespace avh
