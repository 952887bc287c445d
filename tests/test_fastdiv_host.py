"""csrc/fastdiv.h on the host: every per-lane address of the hot kernels goes through div32, so its contract -- div32(n, mk_div32(d))
== n / d exactly for 0 <= n < 2^31 -- is checked with g++ alone (the header needs no HIP include).  Divisors: every d in 1..4096
and {4097, 6000, 36864, 65535, 65536, 2^20 + 1, 2^30, 2^31 - 1}; per divisor n in {0, 1, d - 1, d, d + 1, 2d - 1, 2^31 - d,
2^31 - 1} plus 64 values spread evenly over [0, 2^31).  Nothing is skipped: for d = 2^31 - 1 the two values d + 1 and 2d - 1 lie
past 2^31 and are checked all the same, as 32-bit unsigned numbers (n is cast to uint32_t inside div32)."""
import os
import subprocess
import tempfile

from conftest import ROOT

PROG = r'''
#include <stdio.h>
#include <stdint.h>
#include "fastdiv.h"
using namespace cgen;
int main() {
  static_assert(sizeof(Div32) == 8, "layout");
  const uint32_t extra[8] = {4097u, 6000u, 36864u, 65535u, 65536u, (1u << 20) + 1u, 1u << 30, (1u << 31) - 1u};
  long checked = 0, bad = 0, divisors = 0;
  for (int k = 0; k < 4096 + 8; ++k) {
    const uint32_t d = k < 4096 ? (uint32_t)(k + 1) : extra[k - 4096];
    const Div32 f = mk_div32(d);
    uint32_t ns[8 + 64] = {0u, 1u, d - 1u, d, d + 1u, 2u * d - 1u, (1u << 31) - d, (1u << 31) - 1u};
    for (uint32_t j = 0; j < 64; ++j) ns[8 + j] = j << 25;  // step 2^31 / 64
    for (uint32_t n : ns) {
      const uint32_t q = (uint32_t)div32((int)n, f);
      ++checked;
      if (q != n / d) {
        if (++bad <= 10) printf("MISMATCH d=%u n=%u got %u want %u\n", d, n, q, n / d);
      }
    }
    ++divisors;
  }
  for (uint32_t d = 0; d <= 1; ++d) {  // identity form
    const Div32 f = mk_div32(d);
    if (f.mul != 0 || f.shift != 0 || div32(0, f) != 0 || div32(12345, f) != 12345 || div32(0x7fffffff, f) != 0x7fffffff) {
      ++bad;
      printf("IDENTITY d=%u mul=%u shift=%u\n", d, f.mul, f.shift);
    }
  }
  printf("divisors %ld checked %ld bad %ld\n", divisors, checked, bad);
  return bad ? 1 : 0;
}
'''


def test_div32_is_exact_on_the_host():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "fd.cpp")
        open(src, "w").write(PROG)
        exe = os.path.join(d, "fd")
        # g++ alone: no HIP include path, no HIP macro
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "causal-gen_amd", "csrc"), src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().splitlines()[-1] == "divisors %d checked %d bad 0" % (4096 + 8, (4096 + 8) * 72)
