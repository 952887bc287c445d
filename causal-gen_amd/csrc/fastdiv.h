// Division by a run-time constant without v_rcp/loops, for the per-lane address generation of every kernel family:
//   q = (umulhi(n, mul) + n) >> shift,  exact for 0 <= n < 2^31
// (round-up method: mul = ceil(2^(32+shift) / d) - 2^32 with shift = ceil(log2 d); the "add" variant keeps mul in 32 bits).
// Built on the host, carried in kernel-argument structs, used on the device.  Plain C++: compiles without any HIP include
// (tests/test_fastdiv_host.py checks the contract with g++ alone).
#pragma once
#include <stdint.h>

namespace cgen {

struct Div32 {
  uint32_t mul, shift;
};
static_assert(sizeof(Div32) == 8, "Div32 sits inside kernel-argument structs");

static inline Div32 mk_div32(uint32_t d) {
  Div32 f;
  f.mul = 0; f.shift = 0;
  if (d <= 1) return f;  // identity form: div32 gives n back (no branch on the device)
  uint32_t sh = 0;
  while ((1u << sh) < d) ++sh;  // ceil(log2 d)
  f.shift = sh;
  f.mul = (uint32_t)((((uint64_t)1 << (32 + sh)) + d - 1) / d - ((uint64_t)1 << 32));
  return f;
}

#ifdef __HIPCC__
__device__ __forceinline__ int div32(int n, const Div32& f) {
  return (int)(((uint64_t)__umulhi((uint32_t)n, f.mul) + (uint32_t)n) >> f.shift);
}
#else  // host compile: the same high word
static inline int div32(int n, const Div32& f) {
  return (int)(((((uint64_t)(uint32_t)n * f.mul) >> 32) + (uint32_t)n) >> f.shift);
}
#endif

}  // namespace cgen
