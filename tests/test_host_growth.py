"""The size policy of the buffers that grow on demand (avida_amd/csrc/grow.h;
DESIGN.md 1): need + need/4 under a floor, a ceiling and an alignment.  The
allocation sizes are behaviour, so the seven buffers' policies (floor, ceiling
and alignment as their call sites in csrc/capi*.hip pass them) are held to
literals.  grow.h includes nothing from HIP: a stand-alone C++ program
compiles it with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "grow.h"
using namespace avh;
int main() {
  // genotype rows (cells, m), the arbiter (cells, r)
  const long long rows[][2] = {{1 << 20, 1}, {1 << 20, 1024}, {1 << 20, 1025}, {1100, 1030}};
  for (auto& q : rows) std::printf("gt %lld %lld %lld\n", q[0], q[1], (long long)grown_capacity(q[1], {1024, q[0]}));
  const long long arb[][2] = {{1 << 20, 1}, {1 << 20, 1024}, {1 << 20, 1025}, {1100, 1030}, {0, 1}};
  for (auto& q : arb) std::printf("arb %lld %lld %lld\n", q[0], q[1], (long long)grown_capacity(q[1], {1024, q[0] > 1 ? q[0] : 1}));
  // the lineage store: rows (hint, r), arena (hint, b), scratch
  const long long lr[][2] = {{1, 1}, {1, 5}, {1024, 1}, {1024, 1025}};
  for (auto& q : lr) std::printf("lrows %lld %lld %lld\n", q[0], q[1], (long long)grown_capacity(q[1], {q[0] > 1 ? q[0] : 1}));
  const long long la[][2] = {{16, 16}, {16, 17}, {16, 100}, {0, 1}};
  for (auto& q : la) std::printf("arena %lld %lld %lld\n", q[0], q[1], (long long)grown_capacity(q[1], {q[0] > 16 ? q[0] : 16, INT64_MAX, 16}));
  for (long long n : {0, 64}) std::printf("scratch %lld %lld\n", n, (long long)grown_capacity(n, {64}));
  // a call's inputs and outputs: distances, population events
  for (long long n : {3, 4, 1000}) std::printf("call %lld %lld\n", n, (long long)grown_capacity(n));
  return 0;
}
"""

EXPECTED = """\
gt 1048576 1 1024
gt 1048576 1024 1280
gt 1048576 1025 1281
gt 1100 1030 1100
arb 1048576 1 1024
arb 1048576 1024 1280
arb 1048576 1025 1281
arb 1100 1030 1100
arb 0 1 1
lrows 1 1 1
lrows 1 5 6
lrows 1024 1 1024
lrows 1024 1025 1281
arena 16 16 32
arena 16 17 32
arena 16 100 128
arena 0 1 16
scratch 0 64
scratch 64 80
call 3 3
call 4 5
call 1000 1250
"""


def test_growth_policies(tmp_path):
    src, exe = tmp_path / "growth.cc", tmp_path / "growth"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "avida_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    assert subprocess.check_output([str(exe)], text=True) == EXPECTED
