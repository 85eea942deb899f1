// Host check of avida_amd/csrc/stack_rot.h (tests/test_stack_shift.py compiles
// and runs it): for every pair of pointer values of the two stacks
//  - ring -> depth puts ring slot (sp + d) mod 10 at depth d, of its own stack only;
//  - depth -> ring is its inverse;
//  - a push / pop done as a shift in depth order, rotated back, equals
//    cCPUStack's push / pop on the ring (the slot overwritten, the slot cleared,
//    the pointer), through more than a full turn of the ring either way.
#include <cstdio>
#include <cstring>

#include "stack_rot.h"

static const int N = 10;

struct Ring {
  int32_t s[N];
  int sp;
  void push(int32_t v) { sp = (sp == 0) ? N - 1 : sp - 1; s[sp] = v; }
  int32_t pop() { const int32_t v = s[sp]; s[sp] = 0; sp = (sp + 1 == N) ? 0 : sp + 1; return v; }
};

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)

int main() {
  for (int sp0 = 0; sp0 < N; sp0++) {
    for (int sp1 = 0; sp1 < N; sp1++) {
      int32_t ring[2 * N], sv[2 * N];
      for (int i = 0; i < 2 * N; i++) ring[i] = 1000 * (i / N + 1) + i % N;
      std::memcpy(sv, ring, sizeof sv);
      stack_ring_to_depth<0, N>(sv, (uint32_t)sp0);
      stack_ring_to_depth<1, N>(sv, (uint32_t)sp1);
      for (int d = 0; d < N; d++) {
        CHECK(sv[d] == ring[(sp0 + d) % N]);
        CHECK(sv[N + d] == ring[N + (sp1 + d) % N]);
      }
      stack_depth_to_ring<0, N>(sv, (uint32_t)sp0);
      stack_depth_to_ring<1, N>(sv, (uint32_t)sp1);
      CHECK(std::memcmp(sv, ring, sizeof sv) == 0);
    }
  }
  // pushes and pops in depth order against the ring, from every pointer value
  for (int sp = 0; sp < N; sp++) {
    for (int pass = 0; pass < 2; pass++) {
      Ring r;
      for (int i = 0; i < N; i++) r.s[i] = 500 + i;
      r.sp = sp;
      int32_t sv[2 * N] = {0};
      for (int i = 0; i < N; i++) sv[i] = r.s[i];
      stack_ring_to_depth<0, N>(sv, (uint32_t)sp);
      int dsp = sp;
      for (int step = 0; step < 2 * N + 5; step++) {
        // pass 0: 13 pushes, then pops; pass 1: 13 pops (the last on an empty stack), then pushes
        const bool push = (step < 13) == (pass == 0);
        if (push) {
          const int32_t v = 7000 + step;
          r.push(v);
          for (int d = N - 1; d > 0; d--) sv[d] = sv[d - 1];
          sv[0] = v;
          dsp = (dsp == 0) ? N - 1 : dsp - 1;
        } else {
          const int32_t want = r.pop();
          const int32_t got = sv[0];
          for (int d = 0; d < N - 1; d++) sv[d] = sv[d + 1];
          sv[N - 1] = 0;
          dsp = (dsp + 1 == N) ? 0 : dsp + 1;
          CHECK(got == want);
        }
        CHECK(dsp == r.sp);
        int32_t back[2 * N];
        std::memcpy(back, sv, sizeof back);
        stack_depth_to_ring<0, N>(back, (uint32_t)dsp);
        CHECK(std::memcmp(back, r.s, sizeof r.s) == 0);
      }
    }
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
