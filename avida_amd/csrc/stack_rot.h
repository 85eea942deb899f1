// Class 0's register stacks in depth order (interp_core.h VSTK).
//
// The execution record keeps each stack as cCPUStack's ring of
// AVGPU_STACK_SIZE words and a pointer sp (push: sp = sp-1 mod 10, s[sp] = v;
// pop: v = s[sp], s[sp] = 0, sp = sp+1 mod 10).  Seen by depth from the top
// (depth d = ring slot (sp + d) mod 10) a push moves every entry one deeper and
// drops the deepest -- the slot the ring overwrites -- and a pop moves every
// entry one shallower and lets a 0 in at the bottom -- the slot the ring just
// cleared.  A kernel that holds the stacks in registers therefore keeps them in
// depth order: a pop or push is 10 register moves with no index compare.  The
// two rotations here convert at stage-in and at write-back; everything outside
// such a kernel sees the ring.
//
// Both are barrel rotates on the bits of sp (amounts 1, 2, 4, 8 mod 10; 10
// selects per stage), so that a wave whose lanes differ in sp runs one
// instruction stream.  __host__ __device__: tests/host/stack_rot_check.cc runs
// them on the CPU at every pointer value.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

// ring -> depth order of stack K of sv[2 * N]: depth[d] = ring[(sp + d) mod N]
template <int K, int N>
__host__ __device__ inline void stack_ring_to_depth(int32_t (&sv)[2 * N], uint32_t sp) {
#pragma unroll
  for (int b = 1; b < 16; b <<= 1) {
    const bool on = (sp & (uint32_t)b) != 0u;
    int32_t t[N];
#pragma unroll
    for (int d = 0; d < N; d++) t[d] = sv[K * N + (d + b) % N];
#pragma unroll
    for (int d = 0; d < N; d++) sv[K * N + d] = on ? t[d] : sv[K * N + d];
  }
}

// depth order -> ring: ring[p] = depth[(p - sp) mod N]
template <int K, int N>
__host__ __device__ inline void stack_depth_to_ring(int32_t (&sv)[2 * N], uint32_t sp) {
#pragma unroll
  for (int b = 1; b < 16; b <<= 1) {
    const bool on = (sp & (uint32_t)b) != 0u;
    int32_t t[N];
#pragma unroll
    for (int d = 0; d < N; d++) t[d] = sv[K * N + (d + N - b % N) % N];
#pragma unroll
    for (int d = 0; d < N; d++) sv[K * N + d] = on ? t[d] : sv[K * N + d];
  }
}
