// capi.hip -- host side of the C-ABI declared in include/avida_gpu.h: world
// creation and destruction, the instruction set and the environment, organisms
// in, the batch update loop, statistics, the timing ring and the counters.
// The other subsystems' entry points are in capi_*.hip; host.h holds what the
// files share.
//
// The world object owns every device allocation (SoA organism state, tapes,
// birth queue, scratch) on one HIP device and one HIP stream.  Each entry
// point names the reference interface it replaces in the header.  There is no
// CPU execution path in this library: every state transition of the hot path
// runs in the interpreter's kernels (interp_launch.h, serial.hip) and in those
// of state.hip, sched.hip, place.hip, activate.hip and stats.hip around them.
#include "host.h"

using namespace avh;

namespace avh {

int setup_world(avgpu_world* w, int64_t n, bool test_buffers) {
  DevWorld& W = w->W;
  memset(&W, 0, sizeof(W));
  W.n = n;
  const avgpu_cfg& c = w->cfg;
  int rc = 0;
#define A(ptr, cnt) if ((rc = w->alloc(&W.ptr, (size_t)(cnt))) < 0) return rc
  A(xs, (size_t)n * XS_WORDS); A(ctl, n); A(mem_size, n); A(max_exec, n); A(age, n); A(birth_len, n); A(gkey, n); A(pkey, n); A(rng, 3 * n);
  A(budget, n); A(aclass, n); A(tape, (size_t)n * TAPE_SLOT);
  A(inputs, 3 * n); A(last_task, AVGPU_MAX_REACTIONS * n);
  A(cur_react, AVGPU_MAX_REACTIONS * n);
  A(merit, n); A(fitness, n); A(credit, n); A(gest_time, n); A(num_div, n);
  A(generation, n); A(copied, n); A(child_copied, n); A(executed, n);
  HIPCHK(hipMemsetAsync(W.aclass, ACLASS_NONE, n, w->stream));   // no slice allotted yet
  A(class_list, NUM_LISTS * n); A(order, n); A(sub_hist, (size_t)((n + 4095) / 4096) * SORT_BUCKETS); A(class_count, CLASS_COUNT_WORDS); A(counters, CNT_WORDS);
  // birth records: one primary record per cell + overflow for further
  // offspring of one slice (device.h); test worlds never enqueue births
  W.rcap = n + (test_buffers ? 16 : std::max<int64_t>(4096, n / 4));
  const int64_t R = W.rcap;
  A(b_count, BQ_WORDS); A(b_list, n); A(b_len0, R); A(b_edit, 5 * R);
  // DIV_MUT_PROB arena: three times the largest expected substitutions per
  // record plus 16 (offsets are int32); a fill past it is counted
  // (AVGPU_CNT_SUB_OVERFLOW), never written
  const double pmeans[5] = {c.divide_poisson_slip_mean, c.divide_poisson_mut_mean,
                            c.divide_poisson_ins_mean, c.divide_poisson_del_mean, c.divide_poisson_trans_mean};
  const double psite[6] = {c.div_mut_prob, c.div_ins_prob, c.div_del_prob, c.div_uniform_prob, c.div_slip_prob,
                           c.div_trans_prob};
  // data fills (SLIP_FILL_MODE 2 / 3, TRANS_FILL_MODE 1) keep their draws in
  // the arena, and the one-shot slip then goes there as a segment
  const bool sdata = c.slip_fill_mode == 2 || c.slip_fill_mode == 3, tdata = c.trans_fill_mode == 1;
  const double eslip = c.divide_slip_prob + c.divide_poisson_slip_mean + c.div_slip_prob * AVGPU_MAX_GENOME;
  const double etrans = c.divide_trans_prob + c.divide_poisson_trans_mean + c.div_trans_prob * AVGPU_MAX_GENOME;
  bool pois = false, site = c.divide_trans_prob > 0.0 || (sdata && eslip > 0.0);
  for (int q = 0; q < 5; q++) pois = pois || pmeans[q] > 0.0;
  for (int q = 0; q < 6; q++) site = site || psite[q] > 0.0;
  if (pois || site) {
    // arena words per record: 3x the largest expected count of each kind
    // (per site: a 2048-site offspring) + 16 each; offsets are int32
    const int tw = tdata ? 3 : 2, sw = sdata ? 2 : 1;
    int64_t k = 16 + tw + sw;    // + the one-shot translocation's and slip's words
    for (int q = 0; q < 6; q++)
      if (psite[q] > 0.0)
        k += (q == 5 ? tw : (q == 4 ? sw : 1)) * ((int64_t)std::ceil(AVGPU_MAX_GENOME * std::min(1.0, psite[q]) * 3.0) + 16);
    for (int q = 0; q < 5; q++)
      if (pmeans[q] > 0.0) k += (q == 4 ? tw : (q == 0 ? sw : 1)) * ((int64_t)std::ceil(3.0 * std::min(pmeans[q], 4096.0)) + 16);
    // fill words: a slip or translocation of an L-site insertion keeps L words
    // + L/32 of bit set; E[L] <= a sixth of the offspring (from, to uniform),
    // sized at 3x for an offspring of AVGPU_MAX_GENOME / 4 sites
    const double efill = (AVGPU_MAX_GENOME / 4.0) / 6.0 * (1.0 + 1.0 / 32.0) + 2.0;
    if (sdata && eslip > 0.0) k += (int64_t)std::ceil(3.0 * std::min(eslip, 4096.0) * efill) + 16;
    if (tdata && etrans > 0.0) k += (int64_t)std::ceil(3.0 * std::min(etrans, 4096.0) * efill) + 16;
    k = std::min<int64_t>(k, (int64_t)INT32_MAX / R);
    W.scap = R * k;
    A(b_subs, W.scap); A(b_pofs, NSEG * R); A(b_pcnt, NSEG * R);
  }
  W.seg_any = (pois || site) ? 1 : 0;
  W.pois_any = pois ? 1 : 0;
  for (int q = 0; q < 5; q++) W.pois_L[q] = pmeans[q] > 0.0 ? std::exp(-pmeans[q]) : 0.0;
  A(b_inh, (size_t)BI_WORDS * R); A(b_genome, (size_t)R * TAPE_SLOT);
  // placement scratch with two ghost rows (strip tiles)
  // occupancy, owners and the four placement rounds' claims, each with the two
  // ghost rows a strip tile keeps after its n cells
  const int64_t ng = n + 2 * (int64_t)c.world_x;
  A(occ, ng); A(claim, ng); A(claim2, ng); A(owner, ng); A(killt, n); A(sdone, n); A(ran, n); A(sched, SCHED_WORDS); A(pacc, NSHARD * PACC_STRIDE);
  W.claim_r[0] = W.claim; W.claim_r[1] = W.claim2;
  A(claim_r[2], ng); A(claim_r[3], ng); A(b_tgt, 4 * R);
  if (c.birth_method == 4) {
    A(e_list, n); A(e_blk, (n + 255) / 256 + 1); A(soup_perm, n);
    std::vector<int32_t> iota((size_t)n);
    for (int64_t i = 0; i < n; i++) iota[(size_t)i] = (int32_t)i;
    // on the world's stream, after alloc's zeroing memset (a plain hipMemcpy
    // runs on the null stream, which does not wait for the non-blocking one)
    HIPCHK(hipMemcpyAsync(W.soup_perm, iota.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice,
                          w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
  }
  if (test_buffers) {
    A(t_flags, (size_t)n * TAPE_SLOT); A(t_flags_len, n); A(t_child, (size_t)n * TAPE_SLOT);
    A(t_child_len, n);
  }
  A(rand_cum, 64); A(rand_code, 64); A(task_lut, 256); A(rand_lut, 256);
  A(react_tab, AVGPU_MAX_REACTIONS * RT_STRIDE); A(task_tab, 32);
  A(react_res, AVGPU_MAX_REACTIONS * RR_STRIDE); A(res_param, AVGPU_MAX_RESOURCES);
  A(res_global, AVGPU_MAX_RESOURCES); A(res_cons, AVGPU_MAX_RESOURCES);
  if ((rc = w->alloc(&w->d_Wv[0], 1)) || (rc = w->alloc(&w->d_Wv[1], 1))) return rc;
  w->d_W = w->d_Wv[0];
  w->validv[0] = w->validv[1] = false;
  const int64_t nb = (n + 255) / 256;
  if ((rc = w->alloc(&w->d_totals, (size_t)totals_words(nb)))) return rc;
  W.totals = w->d_totals;
  // the scheduler's tree: block counts, the top tree's levels (a strip tile
  // regrows them for the whole world at avgpu_tile_begin)
  if ((rc = w->alloc(&W.blk_count, (size_t)nb))) return rc;
  W.tree_cap = 1;
  while (W.tree_cap < nb) W.tree_cap <<= 1;
  if ((rc = w->alloc(&W.tree_scr, (size_t)(2 * W.tree_cap)))) return rc;
  if ((rc = w->alloc(&W.tree_cnt, (size_t)(2 * W.tree_cap)))) return rc;
  if ((rc = w->alloc(&w->d_stats, (size_t)stats_words(nb)))) return rc;
#undef A
  w->has_test_buffers = test_buffers;
  // config scalars
  W.world_x = c.world_x; W.world_y = c.world_y; W.geometry = c.world_geometry;
  W.ave_time_slice = c.ave_time_slice; W.slicing = c.slicing_method;
  W.base_merit_method = c.base_merit_method; W.base_const_merit = c.base_const_merit;
  W.default_bonus = c.default_bonus; W.size_range = c.offspring_size_range;
  W.min_copied_lines = c.min_copied_lines; W.min_exe_lines = c.min_exe_lines;
  W.merit_default_bonus = c.merit_default_bonus; W.required_bonus = c.required_bonus;
  W.inherit_merit = c.inherit_merit; W.require_allocate = c.require_allocate;
  W.alloc_method = c.alloc_method; W.max_label_exe = c.max_label_exe_size;
  W.cfg_min_genome = c.min_genome_size; W.cfg_max_genome = c.max_genome_size;
  W.max_genome = (!c.max_genome_size || c.max_genome_size > AVGPU_MAX_GENOME) ? AVGPU_MAX_GENOME : c.max_genome_size;
  W.min_genome = (!c.min_genome_size || c.min_genome_size < AVGPU_MIN_GENOME) ? AVGPU_MIN_GENOME : c.min_genome_size;
  W.death_method = c.death_method; W.age_limit = c.age_limit;
  W.prefer_empty = c.prefer_empty; W.allow_parent = c.allow_parent; W.birth_method = c.birth_method;
  // P(p) = u < p: a 32-bit counter draw x hits iff x < ceil(p 2^32)
  auto th = [](double p) -> uint64_t {
    if (!(p > 0.0)) return 0;
    if (p >= 1.0) return 1ull << 32;
    return (uint64_t)std::ceil(p * 4294967296.0);
  };
  W.th_copy_mut = th(c.copy_mut_prob);
  W.th_copy_ins = th(c.copy_ins_prob); W.p_copy_ins = c.copy_ins_prob;
  W.th_copy_del = th(c.copy_del_prob); W.p_copy_del = c.copy_del_prob;
  W.th_copy_uni = th(c.copy_uniform_prob); W.p_copy_uni = c.copy_uniform_prob;
  W.th_copy_slip = th(c.copy_slip_prob); W.p_copy_slip = c.copy_slip_prob;
  W.copy_ext = (W.th_copy_ins || W.th_copy_del || W.th_copy_uni || W.th_copy_slip) ? 1 : 0;
  W.th_div_mut = th(c.divide_mut_prob);
  W.th_div_ins = th(c.divide_ins_prob);
  W.th_div_del = th(c.divide_del_prob);
  W.th_div_slip = th(c.divide_slip_prob);
  W.th_div_uni = th(c.divide_uniform_prob);
  W.p_copy_mut = c.copy_mut_prob; W.p_div_mut = c.divide_mut_prob; W.p_div_ins = c.divide_ins_prob;
  W.p_div_del = c.divide_del_prob; W.p_div_slip = c.divide_slip_prob; W.p_div_uni = c.divide_uniform_prob;
  W.th_div_site = th(c.div_mut_prob);
  W.p_div_site = c.div_mut_prob;
  W.th_dsite[0] = th(c.div_ins_prob); W.p_dsite[0] = c.div_ins_prob;
  W.th_dsite[1] = th(c.div_del_prob); W.p_dsite[1] = c.div_del_prob;
  W.th_dsite[2] = th(c.div_uniform_prob); W.p_dsite[2] = c.div_uniform_prob;
  W.th_dsite[3] = th(c.div_slip_prob); W.p_dsite[3] = c.div_slip_prob;
  W.th_dsite[4] = th(c.div_trans_prob); W.p_dsite[4] = c.div_trans_prob;
  W.th_dtrans = th(c.divide_trans_prob); W.p_dtrans = c.divide_trans_prob;
  W.th_par_site = th(c.parent_mut_prob);
  W.p_par_site = c.parent_mut_prob;
  W.th_par_ins = th(c.parent_ins_prob); W.p_par_ins = c.parent_ins_prob;
  W.th_par_del = th(c.parent_del_prob); W.p_par_del = c.parent_del_prob;
  W.slip_fill_mode = c.slip_fill_mode;
  W.trans_fill_mode = c.trans_fill_mode;
  W.slip_copy_mode = c.slip_copy_mode;
  W.track_age = (c.birth_method == 1 || c.birth_method == 2) ? 1 : 0;
  W.rec = nullptr; W.rec_n = 0; W.rec_off = nullptr;
  W.seed_lo = (uint32_t)c.seed;
  W.seed_hi = (uint32_t)(c.seed >> 32);
  // interpreter slow-op batching (interp_core.h); AVGPU_SLOW_BATCH overrides
  // (tuning).  Class 0 runs pop and push without parking (its register stacks
  // are in depth order), so with three quarters of the parks gone the same wait
  // fills a smaller batch: 6 against 8 against 12 in the resource environment,
  // whose IO still parks (profiles/stack_shift_ab.txt)
  W.slow_batch = env_int("AVGPU_SLOW_BATCH", 6, 1, 64);
  // the newborn pass's own: 1 -- its duration is its longest newborn's, and a
  // parked lane waiting for a batch lengthens exactly that path (1.344 ->
  // 1.323 ms per update, profiles/r06g_ab_nbsb.txt)
  W.nb_slow_batch = env_int("AVGPU_NB_SLOW_BATCH", 1, 1, 64);
  // the kernels that queue their IO task checks (interp_core.h IOQ): there IO
  // parks only on a full queue and (class 0) pop and push not at all -- what
  // still parks is h-alloc, h-search, h-divide and long labels, a few percent
  // of the instructions, and a lane waiting for company costs more than a slow
  // phase for one lane (1 against 2 / 3 / 4 / 6 / 8: profiles/stack_shift_ab.txt)
  W.ioq_slow_batch = env_int("AVGPU_IOQ_SLOW_BATCH", 1, 1, 64);
  W.row0 = 0;
  W.global_rows = c.world_y;
  W.rows = c.world_y;
  W.tiled = 0;
  W.cell0 = 0;
  // logic id -> task bitmask (main/cTaskLib.cc:511-575)
  static const int sets[9][6] = {
      {15, 51, 85, -1, -1, -1}, {63, 95, 119, -1, -1, -1}, {136, 160, 192, -1, -1, -1},
      {175, 187, 207, 221, 243, 245}, {238, 250, 252, -1, -1, -1}, {10, 12, 34, 48, 68, 80},
      {3, 5, 17, -1, -1, -1}, {60, 90, 102, -1, -1, -1}, {153, 165, 195, -1, -1, -1}};
  uint16_t lut[256] = {0};
  for (int t = 0; t < 9; t++)
    for (int k = 0; k < 6; k++)
      if (sets[t][k] >= 0) lut[sets[t][k]] |= (uint16_t)(1u << t);
  HIPCHK(hipMemcpyAsync(W.task_lut, lut, sizeof(lut), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

// The avida.cfg values this path cannot run with the reference's semantics
// (main/cAvidaConfig.h): an empty string when the configuration is on the
// path, else the reason avgpu_create refuses it (AVGPU_EUNSUPPORTED).
static std::string unsupported_cfg(const avgpu_cfg& c) {
  auto nz = [](double v) { return v != 0.0; };
  const bool slips = nz(c.divide_slip_prob) || nz(c.divide_poisson_slip_mean) || nz(c.div_slip_prob);
  if (slips && (c.slip_fill_mode < 0 || c.slip_fill_mode == 1 || c.slip_fill_mode > 4))
    return "SLIP_FILL_MODE 1 (nop-X) or an unknown mode";
  if (nz(c.copy_slip_prob) && c.slip_copy_mode != 0 && c.slip_copy_mode != 1)
    return "SLIP_COPY_MODE other than 0 (read-head jump) and 1 (memory slip)";
  if (nz(c.copy_slip_prob) && c.slip_copy_mode == 1 && c.slip_fill_mode != 0 && c.slip_fill_mode != 2 &&
      c.slip_fill_mode != 4)
    return "SLIP_COPY_MODE 1 with SLIP_FILL_MODE other than 0 (duplication), 2 (random), 4 (nop-C)";
  if ((nz(c.divide_trans_prob) || nz(c.divide_poisson_trans_mean) || nz(c.div_trans_prob)) &&
      (c.trans_fill_mode < 0 || c.trans_fill_mode > 1))
    return "TRANS_FILL_MODE other than 0 (duplication) / 1 (scrambled)";
  if (c.divide_poisson_slip_mean > 700.0 || c.divide_poisson_mut_mean > 700.0 ||
      c.divide_poisson_ins_mean > 700.0 || c.divide_poisson_del_mean > 700.0 ||
      c.divide_poisson_trans_mean > 700.0)
    return "DIVIDE_POISSON_*_MEAN above 700 (exp(-mean) underflows)";
  if (c.divide_method != 1) return "DIVIDE_METHOD other than 1 (split)";
  if (c.sub_updates < 0 || c.sub_updates > 64) return "sub_updates outside 0..64";
  if (c.sub_updates > 1 && c.slicing_method != 1) return "sub_updates > 1 with SLICING_METHOD other than 1";
  if (c.world_geometry != 1 && c.world_geometry != 2) return "WORLD_GEOMETRY other than 1 (grid) or 2 (torus)";
  if (c.slicing_method < 0 || c.slicing_method > 2) return "SLICING_METHOD other than 0, 1, 2";
  if (c.base_merit_method < 0 || c.base_merit_method > 5) return "BASE_MERIT_METHOD other than 0..5";
  if (c.birth_method < 0 || c.birth_method > 5)
    return "BIRTH_METHOD other than 0 (random neighbour), 1 (oldest), 2 (highest age / merit), 3 (empty only), "
           "4 (whole-world soup), 5 (eldest, serial world)";
  if ((c.birth_method == 1 || c.birth_method == 2) && !c.prefer_empty)
    return "BIRTH_METHOD 1 / 2 without PREFER_EMPTY (the reference reads the organism of an empty cell)";
  if (c.death_method < 0 || c.death_method > 2) return "DEATH_METHOD other than 0, 1, 2";
  if (c.alloc_method != 0 && c.alloc_method != 2) return "ALLOC_METHOD other than 0 (default) and 2 (random)";
  if (nz(c.point_mut_prob) || nz(c.point_ins_prob) || nz(c.point_del_prob) || nz(c.inst_point_mut_prob))
    return "POINT_MUT_PROB / POINT_INS_PROB / POINT_DEL_PROB / INST_POINT_MUT_PROB (cosmic-ray mutations)";
  if (nz(c.div_lgt_prob) || nz(c.divide_lgt_prob) || nz(c.divide_poisson_lgt_mean))
    return "DIV_LGT_PROB / DIVIDE_LGT_PROB / DIVIDE_POISSON_LGT_MEAN (lateral gene transfer)";
  if (nz(c.inject_mut_prob) || nz(c.inject_ins_prob) || nz(c.inject_del_prob)) return "INJECT_*_PROB";
  if (nz(c.meta_copy_mut) || nz(c.meta_std_dev)) return "META_COPY_MUT / META_STD_DEV";
  if (nz(c.death_prob)) return "DEATH_PROB";
  if (c.age_deviation != 0) return "AGE_DEVIATION";
  if (c.divide_failure_resets != 0) return "DIVIDE_FAILURE_RESETS";
  if (c.special_mut_line >= 0) return "SPECIAL_MUT_LINE";
  if (c.population_cap > 0) return "POPULATION_CAP";
  if (c.generation_inc_method != 1) return "GENERATION_INC_METHOD other than 1";
  if (c.reset_inputs_on_divide != 0) return "RESET_INPUTS_ON_DIVIDE";
  if (c.epigenetic_method != 0) return "EPIGENETIC_METHOD";
  if (c.min_cycles != 0) return "MIN_CYCLES";
  if (c.required_task < -1 || c.immunity_task < -1 || c.required_reaction < -1 || c.immunity_reaction < -1 ||
      c.required_task >= AVGPU_MAX_REACTIONS || c.immunity_task >= AVGPU_MAX_REACTIONS ||
      c.required_reaction >= 12 || c.immunity_reaction >= 12)
    return "REQUIRED_TASK / IMMUNITY_TASK outside the task library, REQUIRED_REACTION / IMMUNITY_REACTION "
           "beyond reaction 11";
  if (c.require_exact_copy != 0) return "REQUIRE_EXACT_COPY";
  if (c.fitness_method != 0) return "FITNESS_METHOD other than 0";
  if (c.juv_period != 0) return "JUV_PERIOD";
  if (c.no_mut_insts_len < 0 || c.no_mut_insts_len > 63 ||
      (size_t)c.no_mut_insts_len != strnlen(c.no_mut_insts, sizeof(c.no_mut_insts)))
    return "NO_MUT_INSTS longer than 63 symbols, or no_mut_insts_len not its length";
  if (c.test_fitness_measures != 0) return "REVERT_* / STERILIZE_* (Divide_TestFitnessMeasures1)";
  return std::string();
}

avgpu_world* create_world(const avgpu_cfg* cfg, int device, int64_t n, bool test_buffers) {
  if (!cfg) { fail(AVGPU_EINVAL, "cfg is NULL"); return nullptr; }
  {
    const std::string why = unsupported_cfg(*cfg);
    if (!why.empty()) {
      fail(AVGPU_EUNSUPPORTED, why + " is not on the GPU path");
      return nullptr;
    }
  }
  if (hipSetDevice(device) != hipSuccess) { fail(AVGPU_EHIP, "hipSetDevice failed"); return nullptr; }
  avgpu_world* w = new avgpu_world();
  w->cfg = *cfg;
  w->device = device;
  if (n <= 0) n = (int64_t)cfg->world_x * cfg->world_y;
  // every failure from here ends in avgpu_destroy: the owners free what was made
  auto give_up = [&](int code, const char* msg) -> avgpu_world* {
    avgpu_destroy(w);
    if (msg) fail(code, msg);     // (else the failing call's own message stands)
    return nullptr;
  };
  if (n <= 0 || n > (1ll << 30)) return give_up(AVGPU_EINVAL, "bad cell count");
  if (w->own_stream.create(hipStreamNonBlocking) < 0 ||
      w->h_pred.alloc(PRED_WORDS, hipHostMallocMapped | hipHostMallocCoherent) < 0 ||
      w->h_stage.alloc(2, hipHostMallocDefault) < 0 ||
      w->ev_stage[0].create(hipEventDisableTiming) < 0 || w->ev_stage[1].create(hipEventDisableTiming) < 0 ||
      hipHostGetDevicePointer((void**)&w->d_pred, w->h_pred.get(), 0) != hipSuccess)
    return give_up(AVGPU_EHIP, "stream/event creation failed");
  for (int k = 0; k < PRED_WORDS; k++) w->h_pred.get()[k] = 0;
  w->stream = w->own_stream.get();
  for (int i = 0; i < avgpu_world::RING; i++)
    for (int k = 0; k <= NUM_CLASSES; k++)
      if (w->ring[i][k].create() < 0) return give_up(AVGPU_EHIP, "event creation failed");
  for (int i = 0; i < 64; i++) w->code2op[i] = -1;
  if (setup_world(w, n, test_buffers) < 0) return give_up(0, nullptr);
  return w;
}

int copy_tables(avgpu_world* dst, const avgpu_world* src) {
  DevWorld& D = dst->W;
  const DevWorld& S = src->W;
  D.n_ops = S.n_ops; D.rand_total = S.rand_total; D.fill_code = S.fill_code;
  D.n_react = S.n_react;
  D.env_simple = S.env_simple; D.env_react_mask = S.env_react_mask; D.env_once_mask = S.env_once_mask;
  D.no_mut_mask = S.no_mut_mask;                       // (load_instset / load_env derive these)
  D.req_task = S.req_task; D.imm_task = S.imm_task; D.req_react = S.req_react; D.imm_react = S.imm_react;
  D.single_react = S.single_react; D.max_task_cnt = S.max_task_cnt; D.div_req = S.div_req;
  // the source's tables as its stream leaves them, into the destination on its own
  HIPCHK(hipStreamSynchronize(src->stream));
  HIPCHK(hipMemcpyAsync(D.task_tab, S.task_tab, 32 * sizeof(double), hipMemcpyDeviceToDevice, dst->stream));
  HIPCHK(hipMemcpyAsync(D.react_tab, S.react_tab, AVGPU_MAX_REACTIONS * RT_STRIDE * sizeof(int32_t),
                        hipMemcpyDeviceToDevice, dst->stream));
  HIPCHK(hipMemcpyAsync(D.rand_lut, S.rand_lut, 256, hipMemcpyDeviceToDevice, dst->stream));
  HIPCHK(hipMemcpyAsync(D.rand_cum, S.rand_cum, 64 * sizeof(int32_t), hipMemcpyDeviceToDevice, dst->stream));
  HIPCHK(hipMemcpyAsync(D.rand_code, S.rand_code, 64, hipMemcpyDeviceToDevice, dst->stream));
  HIPCHK(hipStreamSynchronize(dst->stream));
  dst->n_ops = src->n_ops;
  memcpy(dst->op2code, src->op2code, sizeof(dst->op2code));
  memcpy(dst->code2op, src->code2op, sizeof(dst->code2op));
  dst->instset_loaded = src->instset_loaded;
  dst->env_loaded = src->env_loaded;
  return 0;
}

int ready(avgpu_world* w) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (!w->instset_loaded) return fail(AVGPU_ESTATE, "avgpu_load_instset not called");
  if (!w->env_loaded) return fail(AVGPU_ESTATE, "avgpu_load_env not called");
  return 0;
}

// ready for a batch update (avgpu_run_update, avgpu_update_run)
int batch_ready(avgpu_world* w) {
  const int rc = ready(w);
  if (rc < 0) return rc;
  if (w->cfg.birth_method == 5)
    return fail(AVGPU_EUNSUPPORTED, "BIRTH_METHOD 5 (the reaper queue) runs on the serial world only");
  return 0;
}

int translate_genomes(avgpu_world* w, const uint8_t* genomes, const int32_t* lens, int64_t count,
                      std::vector<uint8_t>& codes, std::vector<int32_t>& offsets) {
  codes.clear();
  offsets.resize(count);
  size_t off = 0;
  for (int64_t i = 0; i < count; i++) {
    const int len = lens[i];
    if (len < 1 || len > AVGPU_MAX_GENOME) return fail(AVGPU_EINVAL, "genome length out of range");
    offsets[i] = (int32_t)codes.size();
    for (int k = 0; k < len; k++) {
      const uint8_t op = genomes[off + k];
      if (op >= w->n_ops) return fail(AVGPU_EINVAL, "genome op outside instruction set");
      codes.push_back(w->op2code[op]);
    }
    off += len;
    while (codes.size() & 3) codes.push_back(0);
  }
  if (codes.empty()) codes.push_back(0);
  return 0;
}
int set_orgs_impl(avgpu_world* w, int64_t first, int64_t count, const uint8_t* genomes,
                  const int32_t* lens, const double* merits, const int32_t* inputs, int det) {
  if (first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  // a serial BIRTH_METHOD 5 world whose reaper queue exists: the injections'
  // queue entries (oracle reaper_inject; InjectGenome main/cPopulation.cc:
  // 6964-6968, ActivateOrganism :1358-1361), on the host (injection is rare)
  if (w->W.reaper && w->cfg.birth_method == 5 && !w->reaper_rebuild) {
    std::vector<uint32_t> ctl((size_t)count);
    COPY_SYNC(w, ctl.data(), w->W.ctl + first, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost);
    std::vector<int32_t> q;
    int qrc = reaper_read(w, q);
    if (qrc < 0) return qrc;
    for (int64_t i = 0; i < count; i++) {
      const int32_t c = (int32_t)(first + i);
      if (ctl[(size_t)i] & CTL_ALIVE) {
        for (size_t k = q.size(); k-- > 0;)      // the first entry from the front (the newest end)
          if (q[k] == c) { q.erase(q.begin() + (std::ptrdiff_t)k); break; }
      }
      q.push_back(c);
    }
    if ((qrc = reaper_write(w, q)) < 0) return qrc;
  }
  std::vector<uint8_t> codes;
  std::vector<int32_t> offsets;
  int rc = translate_genomes(w, genomes, lens, count, codes, offsets);
  if (rc < 0) return rc;
  DevBuf<uint8_t> d_codes(w->stream);
  DevBuf<int32_t> d_off(w->stream), d_len(w->stream), d_in(w->stream);
  DevBuf<double> d_m(w->stream);
  if ((rc = d_codes.alloc(codes.size())) < 0 || (rc = d_off.alloc(count)) < 0 || (rc = d_len.alloc(count)) < 0)
    return rc;
  HIPCHK(hipMemcpyAsync(d_codes.get(), codes.data(), codes.size(), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(d_off.get(), offsets.data(), count * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(d_len.get(), lens, count * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  if (merits) {
    if ((rc = d_m.alloc(count)) < 0) return rc;
    HIPCHK(hipMemcpyAsync(d_m.get(), merits, count * sizeof(double), hipMemcpyHostToDevice, w->stream));
  }
  if (inputs) {
    if ((rc = d_in.alloc(3 * count)) < 0) return rc;
    HIPCHK(hipMemcpyAsync(d_in.get(), inputs, 3 * count * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  }
  launch_set_orgs(w->W, w->stream, first, count, d_codes.get(), d_off.get(), d_len.get(), d_m.get(), d_in.get(), det);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int drain_ring(avgpu_world* w, int keep) {
  while (w->ring_count > keep) {
    const int i = (w->ring_head - w->ring_count + avgpu_world::RING) % avgpu_world::RING;
    const int nk = class_timing_all() ? NUM_CLASSES : 1;   // class 0 only: 2 events
    HIPCHK(hipEventSynchronize(w->ring[i][nk]));
    for (int k = 0; k < nk; k++) {
      float f = 0.f;
      HIPCHK(hipEventElapsedTime(&f, w->ring[i][k], w->ring[i][k + 1]));
      w->acc_class_ms[k] += f;
      w->acc_ms += f;
    }
    w->acc_phases++;
    w->ring_count--;
  }
  return 0;
}

// point d_W at a device copy of the world descriptor equal to the host copy,
// uploading it into the other slot when neither holds it.  Only launches on
// the world's own stream read a slot, and the upload is queued on that stream
// behind them, so stream order alone makes it safe (avgpu_set_stream
// synchronises before the stream changes).  It comes from pinned staging
// whose last upload is waited for -- no stream synchronisation on the update
// path (it cost ~30 us of idle GPU per configs[4] update, whose resource
// buffers swap every update).
int push_world(avgpu_world* w) {
  for (int k = 0; k < 2; k++)
    if (w->validv[k] && memcmp(&w->pushedv[k], &w->W, sizeof(DevWorld)) == 0) {
      w->cur_w = k;
      w->d_W = w->d_Wv[k];
      return 0;
    }
  const int k = 1 - w->cur_w;
  HIPCHK(hipEventSynchronize(w->ev_stage[k]));
  memcpy(w->h_stage.get() + k, &w->W, sizeof(DevWorld));
  HIPCHK(hipMemcpyAsync(w->d_Wv[k], w->h_stage.get() + k, sizeof(DevWorld), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipEventRecord(w->ev_stage[k], w->stream));
  memcpy(&w->pushedv[k], &w->W, sizeof(DevWorld));
  w->validv[k] = true;
  w->cur_w = k;
  w->d_W = w->d_Wv[k];
  return 0;
}

int interpret(avgpu_world* w, int mode, int64_t first, int64_t count, bool sorted) {
  int launches = 0;
  {
    const int prc = push_world(w);
    if (prc < 0) return prc;
  }
  int rc = drain_ring(w, avgpu_world::RING - 1);
  if (rc < 0) return rc;
  const bool timed = w->time_every > 0 && (w->interp_calls++ % w->time_every) == 0;
  const int i = w->ring_head;
  hipEvent_t after[NUM_CLASSES];               // the launcher's view of the ring's row
  for (int k = 0; k < NUM_CLASSES; k++) after[k] = w->ring[i][k + 1];
  if (timed) HIPCHK(hipEventRecord(w->ring[i][0], w->stream));
  launch_interpret_classes(w->W, w->d_W, mode, w->stream, first, count, &launches, timed ? after : nullptr, sorted);
  HIPCHK(hipGetLastError());
  if (timed) {
    w->ring_head = (i + 1) % avgpu_world::RING;
    w->ring_count++;
  }
  w->last_launches = launches;
  return 0;
}

// An update's batch steps (oracle choose_k): avgpu_cfg.sub_updates
// when set; else the more of two rules over the last step's predictor: with E
// its weight term in mean weights per organism (the total weight's expected
// move within the update), ceil(E / 0.05) steps above E = 0.1; with D the
// fraction of organisms it expects to divide within the densest quarter of
// the update (a cohort in lock step; a steady state spreads its divides over
// the four), ceil(D / 0.15) steps above D = 0.3; one step otherwise, at most
// ADAPT_KMAX.
constexpr int ADAPT_KMAX = 16;
int choose_k(const avgpu_cfg& c, long long pred, long long n, bool handed_in, long long cnt) {
  if (c.sub_updates > 0) return c.sub_updates;
  if (handed_in || c.slicing_method != AVGPU_SLICE_PROBABILISTIC || n <= 0) return 1;
  const double a = (double)(pred < 0 ? -pred : pred), dn = (double)n;
  int k = 1;
  if (a > 104857.6 * dn) k = std::max(k, (int)std::ceil(a / (52428.8 * dn)));
  if ((double)cnt > 0.3 * dn) k = std::max(k, (int)std::ceil((double)cnt / (0.15 * dn)));
  return std::min(k, ADAPT_KMAX);
}

// after an update's first launch_world_begin / launch_tile_pre: the spatial
// step wrote res_amount_alt; later launches read the new amounts
void after_resources_begin(avgpu_world* w) {
  DevWorld& W = w->W;
  if (res_stepped(W)) std::swap(W.res_amount, W.res_amount_alt);
  W.res_first = 0;
}

// the scheduler's key of batch step `sub` of the current update's K
uint32_t step_key(const avgpu_world* w, int sub, int K) {
  return (uint32_t)w->update * (uint32_t)K + (uint32_t)sub;
}

}  // namespace avh

// ===========================================================================
extern "C" {

const char* avgpu_last_error(void) { return last_error().c_str(); }

int64_t avgpu_live_objects(void) { return g_live.load(); }

void avgpu_cfg_defaults(avgpu_cfg* c) {
  memset(c, 0, sizeof(*c));
  c->world_x = 60; c->world_y = 60; c->world_geometry = 2;
  c->ave_time_slice = 30; c->slicing_method = 1; c->base_merit_method = 4;
  c->base_const_merit = 100; c->default_bonus = 1.0;
  c->copy_mut_prob = 0.0075; c->divide_ins_prob = 0.05; c->divide_del_prob = 0.05;
  c->offspring_size_range = 2.0; c->min_copied_lines = 0.5; c->min_exe_lines = 0.5;
  c->require_allocate = 1; c->death_method = 2; c->age_limit = 20; c->alloc_method = 0;
  c->divide_method = 1; c->max_label_exe_size = 1; c->birth_method = 0; c->prefer_empty = 1;
  c->allow_parent = 1; c->test_cpu_time_mod = 20; c->inherit_merit = 1;
  c->seed = 101;
  // main/cAvidaConfig.h defaults of the refused knobs that are not 0
  c->special_mut_line = -1; c->generation_inc_method = 1;
  c->required_task = -1; c->immunity_task = -1;
  c->required_reaction = -1; c->immunity_reaction = -1;
  c->max_unique_task_count = -1;
}

avgpu_world* avgpu_create(const avgpu_cfg* cfg, int device, int64_t num_cells) {
  return create_world(cfg, device, num_cells, false);
}

int avgpu_check_cfg(const avgpu_cfg* cfg) {
  if (!cfg) return fail(AVGPU_EINVAL, "cfg is NULL");
  const std::string why = unsupported_cfg(*cfg);
  if (!why.empty()) return fail(AVGPU_EUNSUPPORTED, why + " is not on the GPU path");
  return 0;
}

int avgpu_destroy(avgpu_world* w) {
  if (!w) return 0;
  if (w->stream) hipStreamSynchronize(w->stream);
  if (w->own_stream.get()) hipStreamSynchronize(w->own_stream.get());
  if (w->land.world) avgpu_destroy(w->land.world);
  delete w;
  return 0;
}

int avgpu_set_stream(avgpu_world* w, void* hip_stream) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  HIPCHK(hipStreamSynchronize(w->stream));
  // NULL is the HIP null stream -- the stream PyTorch's default current
  // stream reports as 0 -- not the handle's own stream
  w->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return 0;
}

int avgpu_sync(avgpu_world* w) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int avgpu_load_instset(avgpu_world* w, int n, const uint8_t* handler_id, const int32_t* redundancy) {
  if (!w || n <= 0 || n > AVGPU_MAX_INST) return fail(AVGPU_EINVAL, "instruction set size");
  int32_t cum[64] = {0};
  uint8_t code[64] = {0};
  bool used[64] = {false};
  int32_t total = 0;
  for (int i = 0; i < 64; i++) w->code2op[i] = -1;
  for (int i = 0; i < n; i++) {
    const int h = handler_id[i];
    if (h < 0 || h >= AVGPU_H_COUNT) return fail(AVGPU_EINVAL, "unknown handler id");
    if (used[h]) return fail(AVGPU_EUNSUPPORTED, "handler mapped twice (non-injective instset)");
    if (h < 3 && h != i) return fail(AVGPU_EUNSUPPORTED, "nops must be ops 0..2 in A,B,C order");
    used[h] = true;
    total += redundancy ? redundancy[i] : 1;
    cum[i] = total;
    code[i] = (uint8_t)h;
    w->op2code[i] = (uint8_t)h;
    w->code2op[h] = (int16_t)i;
  }
  if (total <= 0) return fail(AVGPU_EINVAL, "zero total redundancy");
  // NO_MUT_INSTS over the handler codes the tapes hold (op i's symbol:
  // Instruction::GetSymbol, core/InstructionSequence.cc:69-106, its first
  // character -- '+', '-', '~', '?' past op 61)
  uint64_t nomut = 0;
  for (int i = 0; i < n; i++) {
    const int k = i % 62;
    const char sym = i >= 62 ? "+-~?"[std::min(i / 62, 4) - 1]
                             : (char)(k < 26 ? 'a' + k : (k < 52 ? 'A' + k - 26 : '0' + k - 52));
    if (memchr(w->cfg.no_mut_insts, sym, (size_t)w->cfg.no_mut_insts_len)) nomut |= 1ull << code[i];
  }
  w->W.no_mut_mask = nomut;
  w->n_ops = n;
  w->W.n_ops = n;
  w->W.rand_total = total;
  w->W.fill_code = code[0];
  HIPCHK(hipMemcpyAsync(w->W.rand_cum, cum, sizeof(cum), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(w->W.rand_code, code, sizeof(code), hipMemcpyHostToDevice, w->stream));
  // GetRandomInst as one table lookup when the weights fit (cpu/cInstSet.cc:83-88)
  uint8_t rlut[256];
  memset(rlut, 0, sizeof(rlut));
  if (total <= 256)
    for (int v = 0, i = 0; v < total; v++) {
      while (i < n - 1 && cum[i] <= v) i++;
      rlut[v] = code[i];
    }
  HIPCHK(hipMemcpyAsync(w->W.rand_lut, rlut, sizeof(rlut), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  w->instset_loaded = true;
  return 0;
}

int avgpu_load_env(avgpu_world* w, int nreact, const avgpu_reaction* r) {
  if (!w || nreact < 0 || nreact > AVGPU_MAX_REACTIONS) return fail(AVGPU_EINVAL, "reaction count");
  DevWorld& W = w->W;
  int32_t tab[AVGPU_MAX_REACTIONS * RT_STRIDE];
  memset(tab, 0, sizeof(tab));
  for (int i = 0; i < nreact; i++) {
    if (r[i].task < 0 || r[i].task >= AVGPU_NUM_LOGIC_TASKS) return fail(AVGPU_EINVAL, "task id");
    int32_t* t = tab + i * RT_STRIDE;
    t[RT_TASK] = r[i].task;
    t[RT_TYPE] = r[i].type;
    t[RT_MIN] = r[i].min_count;
    t[RT_MAX] = r[i].max_count;
    t[RT_HASREQ] = r[i].has_requisite;
    t[RT_USED] = 1;
    const double bonus = r[i].max_number * r[i].value;  // DoProcesses: consumed * value
    const double mult = (r[i].type == AVGPU_PROC_POW) ? std::pow(2.0, bonus) : bonus;
    memcpy(t + RT_MULT, &mult, 8);
    memcpy(t + RT_ADD, &bonus, 8);
  }
  W.n_react = nreact;
  // cOrganism::Divide_CheckViable's requirements (main/cOrganism.cc:788-919):
  // REQUIRED_TASK / IMMUNITY_TASK index the task library -- the distinct
  // tasks in the order of their first REACTION line (cTaskLib::AddTask) --,
  // the reaction knobs the reactions in environment order
  {
    int lib[AVGPU_MAX_REACTIONS], nlib = 0;
    for (int i = 0; i < nreact; i++) {
      bool seen = false;
      for (int k = 0; k < nlib; k++) seen = seen || lib[k] == r[i].task;
      if (!seen) lib[nlib++] = r[i].task;
    }
    const avgpu_cfg& c = w->cfg;
    auto task_of = [&](int t) { return t >= 0 && t < nlib ? lib[t] : -2; };
    W.req_task = c.required_task >= 0 ? task_of(c.required_task) : -1;
    W.imm_task = c.immunity_task >= 0 ? task_of(c.immunity_task) : -1;
    if (W.req_task == -2 || W.imm_task == -2)
      return fail(AVGPU_EUNSUPPORTED, "REQUIRED_TASK / IMMUNITY_TASK past the environment's task library");
    if (c.required_reaction >= nreact || c.immunity_reaction >= nreact)
      return fail(AVGPU_EUNSUPPORTED, "REQUIRED_REACTION / IMMUNITY_REACTION past the environment's reactions");
    if (c.require_single_reaction && nreact > 12)
      return fail(AVGPU_EUNSUPPORTED, "REQUIRE_SINGLE_REACTION with more than 12 reactions");
    W.req_react = c.required_reaction;
    W.imm_react = c.immunity_reaction;
    W.single_react = c.require_single_reaction ? 1 : 0;
    W.max_task_cnt = c.max_unique_task_count;
    W.div_req = (W.req_task >= 0 || (!W.single_react && W.req_react >= 0) || W.single_react ||
                 W.max_task_cnt > 0) ? 1 : 0;
  }
  // simple-environment fast path of the IO task check (interp_core.h)
  double ttab[32];
  for (int t = 0; t < 16; t++) { ttab[t] = 1.0; ttab[16 + t] = 0.0; }
  bool simple = true;
  uint32_t rmask = 0, omask = 0;
  for (int i = 0; i < nreact; i++) {
    const int32_t* t = tab + i * RT_STRIDE;
    if (t[RT_TASK] != i) simple = false;
    if (t[RT_HASREQ]) {
      if (t[RT_MIN] > 0) simple = false;
      else if (t[RT_MAX] == 1) omask |= 1u << i;
      else if (t[RT_MAX] != INT32_MAX) simple = false;
    }
    rmask |= 1u << i;
    double m, a;
    memcpy(&m, t + RT_MULT, 8);
    memcpy(&a, t + RT_ADD, 8);
    if (t[RT_TYPE] == AVGPU_PROC_ADD) ttab[16 + i] = a; else ttab[i] = m;
  }
  // resource-bound processes (cEnvironment::DoProcesses): the general path
  double rr[AVGPU_MAX_REACTIONS * RR_STRIDE];
  memset(rr, 0, sizeof(rr));
  int uses = 0;
  uint32_t res_seen = 0, res_mask = 0;
  for (int i = 0; i < nreact; i++) {
    const int res = r[i].resource;       // 1 + index, 0 = infinite
    if (res == 0) continue;
    if (res < 0 || res > W.n_res) return fail(AVGPU_EINVAL, "reaction names an unknown resource");
    if (res_seen & (1u << (res - 1)))
      return fail(AVGPU_EUNSUPPORTED, "a resource consumed by two reactions is not on the GPU path");
    res_seen |= 1u << (res - 1);
    double* q = rr + i * RR_STRIDE;
    q[RR_RES] = (double)res;
    q[RR_SPATIAL] = w->res_geom[res - 1] != AVGPU_RES_GLOBAL ? 1.0 : 0.0;
    q[RR_DEPL] = r[i].depletable ? 1.0 : 0.0;
    q[RR_TYPE] = (double)r[i].type;
    q[RR_FRAC] = r[i].max_fraction > 1.0 ? 1.0 : r[i].max_fraction;
    q[RR_MIN] = r[i].min_number;
    q[RR_MAX] = r[i].max_number;
    q[RR_VALUE] = r[i].value;
    uses++;
    res_mask |= 1u << i;
  }
  W.env_resources = uses ? 1 : 0;
  W.env_res_mask = simple ? res_mask : 0u;   // the simple path indexes reactions by task
  HIPCHK(hipMemcpyAsync(W.react_res, rr, sizeof(rr), hipMemcpyHostToDevice, w->stream));
  W.env_simple = simple ? 1 : 0;
  W.env_react_mask = rmask;
  W.env_once_mask = omask;
  HIPCHK(hipMemcpyAsync(W.task_tab, ttab, sizeof(ttab), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(W.react_tab, tab, sizeof(tab), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  w->env_loaded = true;
  return 0;
}

int avgpu_set_org(avgpu_world* w, int64_t cell, const uint8_t* genome, int len, double merit,
                  const int32_t* inputs) {
  int rc = ready(w);
  if (rc < 0) return rc;
  const int32_t l = len;
  return set_orgs_impl(w, cell, 1, genome, &l, merit > 0 ? &merit : nullptr, inputs, 0);
}

int avgpu_set_orgs(avgpu_world* w, int64_t first, int64_t count, const uint8_t* genomes,
                   const int32_t* lens, const double* merits, const int32_t* inputs, int det) {
  int rc = ready(w);
  if (rc < 0) return rc;
  return set_orgs_impl(w, first, count, genomes, lens, merits, inputs, det);
}

int avgpu_kill(avgpu_world* w, int64_t cell) {
  if (!w || cell < 0 || cell >= w->W.n) return fail(AVGPU_EINVAL, "cell");
  uint32_t ctl = 0;
  COPY_SYNC(w, &ctl, w->W.ctl + cell, 4, hipMemcpyDeviceToHost);
  ctl &= ~CTL_ALIVE;
  COPY_SYNC(w, w->W.ctl + cell, &ctl, 4, hipMemcpyHostToDevice);
  return 0;
}

int avgpu_step(avgpu_world* w, int64_t first, int64_t count, const int32_t* budget,
               int32_t budget_uniform, int mode) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (mode < 0 || mode > 2) return fail(AVGPU_EINVAL, "mode");
  if (mode == AVGPU_MODE_TEST && !w->has_test_buffers)
    return fail(AVGPU_ESTATE, "TEST mode needs a test world (avgpu_test_genomes)");
  if (count == 0) return 0;
  // budgets are below 2^30 (bit 30 tags spilled slices on device, device.h)
  if (!budget && (budget_uniform < 0 || budget_uniform >= BUDGET_PRIM))
    return fail(AVGPU_EINVAL, "budget out of range [0, 2^30)");
  if (budget)
    for (int64_t i = 0; i < count; i++)
      if (budget[i] < 0 || budget[i] >= BUDGET_PRIM) return fail(AVGPU_EINVAL, "budget out of range [0, 2^30)");
  DevBuf<int32_t> d_b(w->stream);     // (freed once the stream has run the interpretation)
  if (budget) {
    if ((rc = d_b.alloc(count)) < 0) return rc;
    HIPCHK(hipMemcpyAsync(d_b.get(), budget, count * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  }
  // the update's counters and queue lengths cleared -- an earlier update run
  // without statistics has its counts folded into the running sums first
  launch_reset_counts(w->W, w->stream);
  launch_classify_uniform(w->W, w->stream, first, count, d_b.get(), budget_uniform);
  HIPCHK(hipGetLastError());
  return interpret(w, mode, first, count);
}

// One update of a single world in K batch steps, each: total
// merit, allotment, class lists and the class-0 order; interpretation;
// placement; the newborn pass.  own_totals: the picks come from the world's
// own totals, and the last step's placement publishes the predictor; else
// from the totals handed in in d_totals' first TOT_HANDED slots (K = 1).
static int run_steps(avgpu_world* w, int K, bool own_totals, avgpu_update_stats* out) {
  for (int sub = 0; sub < K; sub++) {
    const uint32_t key = step_key(w, sub, K);
    launch_world_begin(w->W, w->stream, w->d_totals, w->d_totals + TOT_WORDS, key, sub, K, own_totals);
    if (sub == 0) after_resources_begin(w);
    HIPCHK(hipGetLastError());
    const int rc = interpret(w, AVGPU_MODE_WORLD, 0, w->W.n, true);
    if (rc < 0) return rc;
    const bool last = sub == K - 1, pred = last && own_totals;
    if (pred) w->pred_seq++;
    launch_world_post(w->W, w->stream, key, sub, K, pred ? w->d_pred : nullptr, w->pred_seq);
    launch_newborns(w->W, w->d_W, w->stream);
    // statistics only when asked for: a run without them (out == NULL) leaves
    // the reduction to avgpu_get_stats / avgpu_stats_vector, or skips it
    launch_world_end(w->W, w->stream, w->d_stats, out != nullptr && last);
    HIPCHK(hipGetLastError());
  }
  w->pred_pending = own_totals;
  w->last_k = K;
  w->stats_stale = out == nullptr;
  w->update++;
  if (out) return avgpu_get_stats(w, out);
  return 0;
}

int avgpu_update_totals(avgpu_world* w, double* dev_totals) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (!dev_totals) return fail(AVGPU_EINVAL, "dev_totals is NULL");
  launch_merit_total(w->W, w->stream, dev_totals, w->d_totals + TOT_WORDS);
  HIPCHK(hipGetLastError());
  return 0;
}

int avgpu_update_run(avgpu_world* w, const double* dev_totals, avgpu_update_stats* out) {
  const int rc = batch_ready(w);
  if (rc < 0) return rc;
  if (!dev_totals) return fail(AVGPU_EINVAL, "dev_totals is NULL");
  if (w->cfg.sub_updates > 1)
    return fail(AVGPU_EUNSUPPORTED, "sub_updates > 1 needs the world's own totals (no handed-in totals)");
  // every world's {total weight, organisms} -> this world's share of the
  // picks (cMultiProcessWorld::CalculateUpdateSize) and its allotment; one
  // batch step (choose_k: handed-in totals)
  if (dev_totals != w->d_totals)
    HIPCHK(hipMemcpyAsync(w->d_totals, dev_totals, TOT_HANDED * sizeof(double), hipMemcpyDeviceToDevice, w->stream));
  w->pred_pending = false;
  return run_steps(w, 1, false, out);
}

int avgpu_run_update(avgpu_world* w, avgpu_update_stats* out) {
  const int rc = batch_ready(w);
  if (rc < 0) return rc;
  if (w->use_global) {                 // totals handed in (avgpu_update_totals / tiles)
    w->use_global = false;
    return avgpu_update_run(w, w->d_totals, out);
  }
  // K batch steps (run_steps; choose_k: avgpu_cfg.sub_updates, or the last
  // update's predictor).  The predictor comes back by mapped memory from the
  // last step's placement: the host waits for it (here, at the next update)
  // while the GPU runs the rest of that update.
  if (w->pred_pending) {
    // the last step's placement launch published the predictor into
    // coherent mapped memory, then its sequence number (k_place_claim0): the
    // host polls that instead of an event on the stream (an event record
    // there left ~6 us of dead time per update before the next launch)
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(w->h_pred.get() + PRED_SEQ, __ATOMIC_ACQUIRE) != w->pred_seq) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
        HIPCHK(hipStreamSynchronize(w->stream));   // a fault surfaces here
        if (__atomic_load_n(w->h_pred.get() + PRED_SEQ, __ATOMIC_ACQUIRE) != w->pred_seq)
          return fail(AVGPU_EHIP, "the batch-step predictor was never published");
      }
    }
    w->pred_acc = __atomic_load_n(w->h_pred.get() + PRED_ACC, __ATOMIC_ACQUIRE);
    w->pred_n = __atomic_load_n(w->h_pred.get() + PRED_ORGS, __ATOMIC_ACQUIRE);
    w->pred_cnt = __atomic_load_n(w->h_pred.get() + PRED_DENSEST, __ATOMIC_ACQUIRE);
    w->pred_pending = false;
  }
  const int K = choose_k(w->cfg, w->pred_acc, w->pred_n, false, w->pred_cnt);
  return run_steps(w, K, true, out);
}

int avgpu_run_updates(avgpu_world* w, int n, avgpu_update_stats* last) {
  for (int i = 0; i < n; i++) {
    int rc = avgpu_run_update(w, nullptr);
    if (rc < 0) return rc;
  }
  if (last) return avgpu_get_stats(w, last);
  return 0;
}

int avgpu_get_stats(avgpu_world* w, avgpu_update_stats* out) {
  if (!w || !out) return fail(AVGPU_EINVAL, "args");
  double v[NSTAT];
  if (w->stats_stale) {
    launch_stats(w->W, w->stream, w->d_stats);
    HIPCHK(hipGetLastError());
    w->stats_stale = false;
  }
  HIPCHK(hipMemcpyAsync(v, w->d_stats, sizeof(v), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  memset(out, 0, sizeof(*out));
  out->update = w->update - 1;
  out->num_organisms = (int64_t)v[ST_ORGS];
  out->sum_merit = v[ST_MERIT];
  out->sum_fitness = v[ST_FITNESS];
  out->sum_gestation = v[ST_GESTATION];
  out->sum_genome_length = v[ST_GENOME_LEN];
  out->max_fitness = v[ST_MAX_FITNESS];
  out->ave_generation = v[ST_ORGS] > 0 ? v[ST_GENERATION] / v[ST_ORGS] : 0.0;
  for (int t = 0; t < AVGPU_NUM_LOGIC_TASKS; t++) out->task_orgs[t] = (int64_t)v[ST_TASK0 + t];
  out->insts_executed = (int64_t)v[ST_INSTS];
  out->deaths = (int64_t)v[ST_DEATHS];
  out->divides = (int64_t)v[ST_DIVIDES];
  out->births = (int64_t)v[ST_BIRTHS];
  out->births_dropped = (int64_t)v[ST_DROPPED];
  out->sum_mem_size = v[ST_MEM_SIZE];
  out->cum_insts_executed = (int64_t)v[ST_CUM_INSTS];
  out->cum_births = (int64_t)v[ST_CUM_BIRTHS];
  out->slices = (int64_t)v[ST_SLICES];
  out->lane_steps = (int64_t)v[ST_LANESTEPS];
  out->births_overwritten = (int64_t)v[ST_OVERWRITTEN];
  out->births_cancelled = (int64_t)v[ST_CANCELLED];
  out->seed = w->cfg.seed;
  out->insts_wasted = (int64_t)v[ST_WASTED];
  memcpy(&out->sched_pred, v + ST_PRED, 8);        // (int64 bits)
  memcpy(&out->sched_carry, v + ST_CARRY, 8);
  out->sched_pred_n = (int64_t)v[ST_PRED_ORGS];
  memcpy(&out->sched_pred_cnt, v + ST_PRED_DENSEST, 8);
  for (int q = 0; q < 4; q++) memcpy(&out->sched_pred_bins[q], v + ST_QUARTER0 + q, 8);
  out->sub_steps = w->last_k;
  return 0;
}

int avgpu_stats_vector(avgpu_world* w, void** dev_ptr) {
  if (!w || !dev_ptr) return fail(AVGPU_EINVAL, "args");
  if (w->stats_stale) {           // the vector is complete once this stream reaches it
    launch_stats(w->W, w->stream, w->d_stats);
    HIPCHK(hipGetLastError());
    w->stats_stale = false;
  }
  *dev_ptr = w->d_stats;
  return 0;
}

int avgpu_set_global_totals(avgpu_world* w, double total_merit, int64_t total_orgs) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  double v[TOT_HANDED];
  v[TOT_WEIGHT] = total_merit;
  v[TOT_ORGS] = (double)total_orgs;
  HIPCHK(hipMemcpyAsync(w->d_totals, v, sizeof(v), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  w->use_global = true;
  return 0;
}

int avgpu_last_step_insts(avgpu_world* w, int64_t* insts) {
  if (!w || !insts) return fail(AVGPU_EINVAL, "args");
  std::vector<unsigned long long> v(NSHARD * CNT_STRIDE);
  HIPCHK(hipMemcpyAsync(v.data(), w->W.counters, v.size() * 8, hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  unsigned long long s = 0;
  for (int sh = 0; sh < NSHARD; sh++) s += v[sh * CNT_STRIDE + AVGPU_CNT_INSTS];
  *insts = (int64_t)s;
  return 0;
}

int avgpu_last_kernel_ms(avgpu_world* w, double* ms, int64_t* launches) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  int rc = drain_ring(w, 0);
  if (rc < 0) return rc;
  if (ms) *ms = w->acc_ms;
  if (launches) *launches = w->acc_phases;
  w->acc_ms = 0.0;
  w->acc_phases = 0;
  for (int k = 0; k < NUM_CLASSES; k++) w->acc_class_ms[k] = 0.0;
  return 0;
}

int avgpu_set_timing(avgpu_world* w, int every) {
  if (!w || every < 0) return fail(AVGPU_EINVAL, "every < 0");
  w->time_every = every;
  w->interp_calls = 0;
  return 0;
}

int avgpu_kernel_times(avgpu_world* w, double* class_ms, int64_t* phases) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  int rc = drain_ring(w, 0);
  if (rc < 0) return rc;
  if (class_ms)
    for (int k = 0; k < NUM_CLASSES; k++) class_ms[k] = w->acc_class_ms[k];
  if (phases) *phases = w->acc_phases;
  w->acc_ms = 0.0;
  w->acc_phases = 0;
  for (int k = 0; k < NUM_CLASSES; k++) w->acc_class_ms[k] = 0.0;
  return 0;
}

int avgpu_counters(avgpu_world* w, int cumulative, int64_t* out, int n) {
  if (!w || !out || n < 0) return fail(AVGPU_EINVAL, "args");
  if (n > AVGPU_NUM_COUNTERS) n = AVGPU_NUM_COUNTERS;
  std::vector<unsigned long long> v(CNT_WORDS);
  HIPCHK(hipMemcpyAsync(v.data(), w->W.counters, v.size() * 8, hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  for (int k = 0; k < n; k++) {
    unsigned long long s = 0;
    // (an update run without statistics has its counts still in the shards)
    if (!cumulative || v[CNT_CUM_FLAG] == 0ull)
      for (int sh = 0; sh < NSHARD; sh++) s += v[sh * CNT_STRIDE + k];
    if (cumulative) s += v[CNT_CUM_BASE + k];
    out[k] = (int64_t)s;
  }
  return 0;
}

}  // extern "C"
