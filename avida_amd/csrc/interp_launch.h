// interp_launch.h -- k_interpret, the kernel around interpret_chunk
// (interp_core.h), and launch_interpret, which launches one of its
// instantiations.  Each launch_interpret<S, REC, C0W, NB> of the library, with
// the kernels it launches, is compiled in exactly one unit (INTERP_CLASS0:
// interp_c0.hip, interp_c0_rec.hip; INTERP_LISTS: interp_lists.hip,
// interp_lists_rec.hip; INTERP_CLASS3: serial.hip); interp.hip chooses among
// them.
#pragma once
#include "interp_core.h"

// The k_interpret instantiation of a launch (interp.hip interp_of)
enum Interp { IP_GENERIC, IP_SIMPLE, IP_DEF, IP_DEF_RES };

namespace {

// class 0 must keep 2 waves per SIMD (its LDS admits 7 blocks per CU): the
// second bound caps it at 256 registers (VGPR + AGPR)
// The mixed class-0 launch (nmix > 0, world updates): its first nmix blocks
// run the list classes 1 / 2 / 3 in class-0 blocks (MIX_B1 / MIX_B2 / MIX_B3
// blocks, each a grid-stride over its list in chunks of 64 / kslot
// organisms), the rest are class 0 -- one launch on the world's one stream.
#define MIX_B1 512
#define MIX_B2 16
#define MIX_B3 8
#define MIX_BLOCKS (MIX_B1 + MIX_B2 + MIX_B3)
static_assert(MIX_BLOCKS % 8 == 0, "class 0's XCD mapping needs whole rounds of 8 blocks");
// `sorted_arg`: KI_SORTED the class-0 sweep follows the budget-sorted windows,
// KI_PRED a world update's main pass (its slices add the sub-step predictor);
// NB: the newborn pass (class 0 over list row LIST_NEWBORN, a grid-stride)
template <int S, bool REC, bool C0W = false, bool SIMPLE = false, bool DEF = false, bool RES = false, bool NB = false>
__global__ __launch_bounds__(64, (S == CLASS0_SIZE) ? 2 : 1) void k_interpret(const DevWorld* __restrict__ Wp, int cls, int row, int mode,
                                                  int64_t first, int64_t count, int sorted_arg, int lpw, int nmix = 0) {
  // class 0: stacks in VGPRs, tables in global memory -- only the tapes in LDS
  constexpr int STK = (S == CLASS0_SIZE) ? 0 : STK_LDS_WORDS;
  constexpr int TAB = (S == CLASS0_SIZE) ? 0 : TAB_WORDS;
  __shared__ __attribute__((aligned(16))) uint32_t lds32[64 * tape_stride(S) / 4 + STK + TAB];
  const int sorted = sorted_arg & KI_SORTED;
  const bool pred = (sorted_arg & KI_PRED) != 0;
  if (cls == 0) {
    if (S == CLASS0_SIZE && C0W && (int)blockIdx.x < nmix) {
      const int b = blockIdx.x;
      const int lc = b < MIX_B1 ? 1 : (b < MIX_B1 + MIX_B2 ? 2 : 3);
      const int b0 = lc == 1 ? 0 : (lc == 2 ? MIX_B1 : MIX_B1 + MIX_B2);
      const int nb = lc == 1 ? MIX_B1 : (lc == 2 ? MIX_B2 : MIX_B3);
      const int kslot = lc == 1 ? 3 : (lc == 2 ? 5 : 7);      // 960 / 1600 / 2240 B >= 768 / 1536 / 2048 sites
      const int per = 64 / kslot;
      const int lcount = Wp->class_count[lc];
      for (int64_t chunk = b - b0; chunk * per < lcount; chunk += nb) {
        // (Wp, cls, mode, first, count, chunk, lds32, sorted, row, lpw, serial, kslot, direct, pred)
        interpret_chunk<S, REC, false, SIMPLE, DEF, RES, true, NB>(Wp, lc, mode, first, count, chunk, lds32, false, lc,
                                                                    per, 0, kslot, -2, pred);
        __syncthreads();
      }
      return;
    }
    const int64_t bx = (int64_t)blockIdx.x - nmix, gx = (int64_t)gridDim.x - nmix;
    // one class-0 chunk, then (world slices) the wave's own spills
    auto run_chunk = [&](int64_t chunk) {
      // (Wp, cls, mode, first, count, chunk, lds32, sorted, row, lpw, serial, kslot, direct, pred)
      const int sp = interpret_chunk<S, REC, C0W, SIMPLE, DEF, RES, false, NB>(Wp, 0, mode, first, count, chunk, lds32,
                                                                               sorted, 0, 64, 0, 1, -2, pred) - 1;
      if (S == CLASS0_SIZE && C0W) {
        // Organisms whose h-alloc (or copy) outgrew their 320-site slot: this
        // wave continues them at once in 3-slot (960-site) lanes of its own
        // block's LDS -- their state was written back by this wave, so a
        // workgroup-scope fence makes it visible to the re-staging -- instead of
        // a spill row after class 0 (~55 organisms per update, 66 us after
        // class 0, latency-bound on the longest).  A slice that outgrows 960
        // sites goes on to the class-2 spill row.
        uint64_t m = __ballot(sp >= 0);
        if (m) {
          const int nsp = __popcll(m);
          int mine = -1;
          for (int j = 0; m; j++, m &= m - 1) {
            const int c = __shfl(sp, __ffsll((long long)m) - 1);
            if ((int)threadIdx.x == j) mine = c;
          }
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          __syncthreads();
          constexpr int PER3 = 64 / 3;
          for (int g = 0; g < nsp; g += PER3) {
            const int d = __shfl(mine, (g + (int)threadIdx.x) & 63);
            const int direct = ((int)threadIdx.x < PER3 && g + (int)threadIdx.x < nsp) ? d : -1;
            // (Wp, cls, mode, first, count, chunk, lds32, sorted, row, lpw, serial, kslot, direct, pred):
            // as class 0's spill row (4), which continues the slice, in 3 slots
            interpret_chunk<S, REC, false, SIMPLE, DEF, RES, true, NB>(Wp, 1, mode, first, count, 0, lds32, false, 4,
                                                                        PER3, 0, 3, direct, pred);
            __syncthreads();
          }
        }
      }
    };
    if (NB) {
      // the newborn pass: a grid-stride over list row LIST_NEWBORN
      const int ncount = Wp->class_count[LIST_NEWBORN];
      for (int64_t chunk = bx; chunk * 64 < ncount; chunk += gx) {
        run_chunk(chunk);
        __syncthreads();
      }
      return;
    }
    // sorted windows: the 32 chunks of a window run on one XCD (blocks are
    // dealt to the 8 XCDs round robin), so its state lines meet in one L2
    int64_t chunk = bx;
    if (sorted && (gx & 7) == 0) chunk = (bx & 7) * (gx >> 3) + (bx >> 3);
    run_chunk(chunk);
    return;
  }
  if (C0W) return;
  // list classes: grid-stride over the list (its length is known on device
  // only); with cls < 0, rows row and row + 1 in one launch (their organisms
  // fit this class's tape slots: classes 2 + 3 beside class 0, spill rows 5 + 6)
  const int nrows = cls < 0 ? 2 : 1;
  for (int r = row; r < row + nrows; r++) {
    const int rc = cls >= 0 ? cls : (r <= 3 ? r : r - 3);
    const int lcount = Wp->class_count[r];
    for (int64_t chunk = blockIdx.x; chunk * lpw < lcount; chunk += gridDim.x) {
      // (Wp, cls, mode, first, count, chunk, lds32, sorted, row, lpw, serial, kslot, direct, pred)
      interpret_chunk<S, REC, false, SIMPLE, DEF, RES, false, NB>(Wp, rc, mode, first, count, chunk, lds32, false, r,
                                                                   lpw, 0, 1, -2, pred);
      __syncthreads();
    }
  }
}

}  // namespace

// Launches the k_interpret<S, REC, C0W, ..., NB> that `v` names.
// C0W: class 0 of a world-mode launch; outside world mode class 0 has the
// generic kernel only
template <int S, bool REC, bool C0W, bool NB>
void launch_interpret(Interp v, unsigned grid, hipStream_t s, const DevWorld* dW, int cls, int row, int mode,
                      int64_t first, int64_t count, int srt, int lpw, int nmix) {
#define LAUNCH(SIMPLE, DEF, RES) \
  hipLaunchKernelGGL((k_interpret<S, REC, C0W, SIMPLE, DEF, RES, NB>), dim3(grid), dim3(64), 0, s, dW, cls, row, \
                     mode, first, count, srt, lpw, nmix)
  if constexpr (C0W || S != CLASS0_SIZE) {
    if (v == IP_DEF_RES) { LAUNCH(true, true, true); return; }
    if (v == IP_DEF) { LAUNCH(true, true, false); return; }
  }
  if constexpr (C0W) {
    if (v == IP_SIMPLE) { LAUNCH(true, false, false); return; }
  }
  LAUNCH(false, false, false);
#undef LAUNCH
}

// Every launch_interpret of the library, as X(S, REC, C0W, NB): class 0 of a
// world-mode launch in the main and the newborn pass, class 0 outside world
// mode; the list classes' sizes, of which the newborn pass launches only the
// largest (interp.hip launch_classes).  Class 3's main-pass kernels use the
// interpret_chunk<CLASS3_SIZE, REC> that k_serial_update uses, and the
// compiler's code for either depends on whether the other is beside it: they
// stay in one unit, serial.hip.  A unit instantiates its share with
// INTERP_DEFINE; every other unit sees INTERP_EXTERN and compiles no kernel.
#define INTERP_CLASS0(X, REC) \
  X(CLASS0_SIZE, REC, true, false) X(CLASS0_SIZE, REC, true, true) X(CLASS0_SIZE, REC, false, false)
#define INTERP_LISTS(X, REC) \
  X(CLASS1_SIZE, REC, false, false) X(CLASS2_SIZE, REC, false, false) X(CLASS3_SIZE, REC, false, true)
#define INTERP_CLASS3(X, REC) X(CLASS3_SIZE, REC, false, false)
#define INTERP_SIGNATURE \
  (Interp, unsigned, hipStream_t, const DevWorld*, int, int, int, int64_t, int64_t, int, int, int)
#define INTERP_EXTERN(S, REC, C0W, NB) extern template void launch_interpret<S, REC, C0W, NB> INTERP_SIGNATURE;
#define INTERP_DEFINE(S, REC, C0W, NB) template void launch_interpret<S, REC, C0W, NB> INTERP_SIGNATURE;
INTERP_CLASS0(INTERP_EXTERN, false)
INTERP_CLASS0(INTERP_EXTERN, true)
INTERP_LISTS(INTERP_EXTERN, false)
INTERP_LISTS(INTERP_EXTERN, true)
INTERP_CLASS3(INTERP_EXTERN, false)
INTERP_CLASS3(INTERP_EXTERN, true)
