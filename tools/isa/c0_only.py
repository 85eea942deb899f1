"""Write a source that instantiates only the class-0 world kernel of the bench
(REC, C0W, SIMPLE, DEF) from interp_launch.h, for fast ISA / register-count
experiments:

  python tools/isa/c0_only.py /tmp/isa/c0.hip [extra #define lines...]
  hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off \
      -I avida_amd/csrc --offload-device-only -S -o /tmp/isa/c0.s /tmp/isa/c0.hip
"""
import sys

text = """#include "interp_launch.h"

void c0_entry(const DevWorld* dW) {
  hipLaunchKernelGGL((k_interpret<CLASS0_SIZE, true, true, true, true, false>), dim3(1), dim3(64), 0, 0, dW, 0, 0,
                     (int)AVGPU_MODE_WORLD, (int64_t)0, (int64_t)0, 1, 64, 0);
}
"""
defs = "".join("#define %s\n" % d.replace("=", " ", 1) for d in sys.argv[2:])
open(sys.argv[1], "w").write(defs + text)
