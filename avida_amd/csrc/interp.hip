// interp.hip -- the host side of the interpreter's launches: which k_interpret
// instantiations a step or a world update launches, in which order and over
// which grids.  It compiles no kernel: the interpreter is interp_core.h, the
// kernel and launch_interpret are interp_launch.h, and the instantiations are
// compiled in interp_c0.hip, interp_c0_rec.hip, interp_lists.hip and
// interp_lists_rec.hip (the serial world's kernel in serial.hip).
//
// A launch sequence (launch_classes): class 0 -- in a world
// update or newborn pass with the list classes 1..3 in its leading blocks and
// its own spills continued by the wave that spilled them --, otherwise the
// list classes and class 0's spill row after it on the same stream, then the
// spill rows of classes 1 and 2 in one launch of class 3's slots.
#include <algorithm>

#include "interp_launch.h"

// lanes per wave of the spill rows (AVGPU_SPILL_LPW overrides for sweeps)
static int spill_lpw() {
  static const int v = env_int("AVGPU_SPILL_LPW", 1, 1, 64);
  return v;
}

// timing events around class 0 only (default) or after every class
// (AVGPU_CLASS_TIMING=1, diagnostics): each timed event record costs ~10 us
// of queue time, and the three spill-row launches sit on the update's
// critical path
bool class_timing_all() {
  static const int v = env_int("AVGPU_CLASS_TIMING", 0, 0, 1);
  return v == 1;
}

// the knobs the DEF instantiation fixes, at the reference's defaults
// (avgpu_cfg_defaults; main/cAvidaConfig.h)
static bool def_knobs(const DevWorld& W) {
  return W.alloc_method != 2 && W.require_allocate == 1 && W.max_label_exe == 1 && W.cfg_min_genome == 0 &&
         W.cfg_max_genome == 0 && W.merit_default_bonus == 0.0 && W.inherit_merit == 1 &&
         W.base_merit_method == 4 && W.th_div_uni == 0 && !W.seg_any && W.th_par_site == 0 && W.th_par_ins == 0 &&
         W.th_par_del == 0 && W.size_range == 2.0 && W.min_exe_lines == 0.5 &&
         W.min_copied_lines == 0.5 && W.required_bonus == 0.0 && W.default_bonus == 1.0 && W.rand_total <= 256 &&
         !W.copy_ext && !W.track_age && W.no_mut_mask == 0 && !W.div_req;
}

// The k_interpret instantiation of a launch (Interp, interp_launch.h), chosen
// once per launch_classes call for its class-0 launch and its rows alike.
// IP_DEF: a world update (main pass or newborn pass) at the simple environment
// and default knobs runs the specialised interpreter (SIMPLE, DEF) in its list
// classes and spill rows as in class 0 -- the spill rows run alone after
// class 0, latency-bound on their longest slice, so every instruction of the
// generic paths is on the update's critical path
// (DEF defers the divide's phenotype work to placement round 0: only world
// updates run placement -- avgpu_step(MODE_WORLD) takes the general path)
// IP_DEF_RES: the same with finite resources behind the simple reactions, configs[4]
// IP_SIMPLE: class 0 of any other world-mode launch at the simple environment
// without resources (the rows have no such kernel: they run the generic one)
static Interp interp_of(const DevWorld& W, int mode, bool update) {
  if (mode != AVGPU_MODE_WORLD) return IP_GENERIC;
  const bool res = W.env_res_mask != 0u;
  if (update && W.env_simple && def_knobs(W)) return res ? IP_DEF_RES : IP_DEF;
  return (W.env_simple && !res) ? IP_SIMPLE : IP_GENERIC;
}

// NB: the newborn pass of a world update (launch_newborns): the same launches
// over the organisms k_activate listed -- class 0 from list row 0 by a
// grid-stride of NB_BLOCKS blocks, the list classes in its leading blocks,
// then the spill rows.  A world update's main pass (sorted) adds the sub-step
// predictor (KI_PRED of the kernels' `sorted_arg`).
#define NB_BLOCKS 2048
template <bool REC, bool NB>
static void launch_classes(const DevWorld& W, const DevWorld* dW, int mode, hipStream_t s,
                           int64_t first, int64_t count, int* launches, hipEvent_t* after_class, bool sorted) {
  const bool c0w = mode == AVGPU_MODE_WORLD;
  const int pfl = (!NB && sorted && c0w) ? KI_PRED : 0;
  const int srt = ((!NB && sorted && first == 0 && count == W.n) ? KI_SORTED : 0) | pfl;
  const bool tall = class_timing_all();
  const unsigned blocks = NB ? (unsigned)NB_BLOCKS : (unsigned)((count + 63) / 64);
  if (blocks == 0) {
    if (after_class)
      for (int k = 0; k < 4; k++) hipEventRecord(after_class[k], s);
    return;
  }
  // the list classes inside class 0's launch (MIX_BLOCKS leading blocks): the
  // newborn pass, or a sorted world update
  const bool mix = NB || (sorted && c0w);
  const int nmix = mix ? MIX_BLOCKS : 0;
  const Interp v = interp_of(W, mode, mix);
#define ROW(SZ, grid, cls, r, lpw) \
  launch_interpret<SZ, REC, false, NB>(v, grid, s, dW, cls, r, mode, first, count, pfl, lpw, 0)
  if (c0w)
    launch_interpret<CLASS0_SIZE, REC, true, NB>(v, blocks + (unsigned)nmix, s, dW, 0, 0, mode, first, count, srt, 64,
                                                 nmix);
  else if constexpr (!NB)
    launch_interpret<CLASS0_SIZE, REC, false, false>(v, blocks, s, dW, 0, 0, mode, first, count, srt, 64, 0);
  if (after_class) hipEventRecord(after_class[0], s);
  // Spill rows run after class 0, alone on the chip and latency-bound on their
  // longest remaining slice; spread over waves (spill_lpw lanes each), a
  // wave's iterations no longer pay for its other lanes' divergent paths.
  const int slpw = spill_lpw();
  const unsigned lb_small = std::min(blocks, 256u);
  // The newborn pass always mixes: its list classes run inside class 0's
  // launch and its class-0 waves continue their own spills, so rows 5 + 6
  // below, in class 3's slots, are its only launch of a list size -- classes
  // 1 and 2 have no newborn kernel (interp_launch.h INTERP_LISTS).
  if constexpr (!NB) {
    if (!mix) {
      // avgpu_step: the list classes follow class 0 on the stream.  A capped
      // grid strides over each list (length known on the device only).  The
      // caps follow the blocks a CU holds (LDS: 3 of class 1, 1 of classes
      // 2 / 3) and the lists' usual lengths (class 1 ~1 %, classes 2 / 3 and the
      // spill rows tens of organisms): a 2048-block grid of 132-KiB class-3
      // blocks costs 8 dispatch rounds even when its list is empty.
      ROW(CLASS1_SIZE, std::min(blocks, 768u), 1, 1, 64);
      ROW(CLASS2_SIZE, std::min(blocks, 8u), 2, 2, 64);
      ROW(CLASS3_SIZE, std::min(blocks, 4u), 3, 3, 64);
      // row 4 (class 0's spills): a world launch's class-0 waves continue their
      // own spills (k_interpret, C0W), other launches run the row
      if (!c0w) ROW(CLASS1_SIZE, lb_small, 1, 4, slpw);
    }
  }
  if (after_class && tall) hipEventRecord(after_class[1], s);
  // spill rows 5 + 6 (beyond classes 1 / 2) in one launch of class 3's slots
  // (all three spill rows in one class-3 launch measured 8 us slower per
  // update than these two launches: row 4's organisms ran slower in class 3's
  // slots than the saved launch gap)
  ROW(CLASS3_SIZE, std::min(lb_small, 64u), -1, 5, slpw);
#undef ROW
  if (after_class && tall) { hipEventRecord(after_class[2], s); hipEventRecord(after_class[3], s); }
  if (launches) *launches += 5;
}

// RECORDED streams launch the REC instantiations (device.h DevWorld::rec)
void launch_interpret_classes(const DevWorld& W, const DevWorld* dW, int mode, hipStream_t s,
                              int64_t first, int64_t count, int* launches, hipEvent_t* after_class, bool sorted) {
  if (W.rec)
    launch_classes<true, false>(W, dW, mode, s, first, count, launches, after_class, sorted);
  else
    launch_classes<false, false>(W, dW, mode, s, first, count, launches, after_class, sorted);
}

// the newborn pass of a world update's batch step (after k_activate)
void launch_newborns(const DevWorld& W, const DevWorld* dW, hipStream_t s) {
  if (W.rec)
    launch_classes<true, true>(W, dW, AVGPU_MODE_WORLD, s, 0, W.n, nullptr, nullptr, false);
  else
    launch_classes<false, true>(W, dW, AVGPU_MODE_WORLD, s, 0, W.n, nullptr, nullptr, false);
}
