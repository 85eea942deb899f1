// capi_landscape.hip -- the test CPU and the mutational landscapes.
#include "host.h"

using namespace avh;

extern "C" {

int avgpu_test_genomes(avgpu_world* w, int n, const uint8_t* genomes, const int32_t* lens,
                       avgpu_test_result* results, char* executed_flags, int flags_cap,
                       uint8_t* offspring) {
  RCCHK(ready(w));
  if (n <= 0) return 0;
  avgpu_cfg tc = w->cfg;
  tc.copy_mut_prob = 0; tc.divide_mut_prob = 0; tc.divide_ins_prob = 0; tc.divide_del_prob = 0;
  avgpu_world* t = create_world(&tc, w->device, n, true);
  if (!t) return AVGPU_ENOMEM;
  struct Destroy { avgpu_world* t; ~Destroy() { avgpu_destroy(t); } } destroy{t};   // on every return
  RCCHK(copy_tables(t, w));
  RCCHK(set_orgs_impl(t, 0, n, genomes, lens, nullptr, nullptr, 1));
  std::vector<int32_t> budget(n);
  for (int i = 0; i < n; i++) budget[i] = w->cfg.test_cpu_time_mod * lens[i];
  RCCHK(avgpu_step(t, 0, n, budget.data(), 0, AVGPU_MODE_TEST));
  std::vector<avgpu_cpu_state> st(n);
  std::vector<uint8_t> ops((size_t)n * AVGPU_MAX_GENOME), fl((size_t)n * AVGPU_MAX_GENOME);
  RCCHK(avgpu_get_states(t, 0, n, st.data(), ops.data(), fl.data(), AVGPU_MAX_GENOME));
  std::vector<uint8_t> tflags((size_t)n * TAPE_SLOT), tchild((size_t)n * TAPE_SLOT);
  std::vector<int32_t> tflen(n), tclen(n);
  // (checked: a failed copy would hand back uninitialised flags and offspring)
  const hipError_t ce[4] = {
      hipMemcpyAsync(tflags.data(), t->W.t_flags, tflags.size(), hipMemcpyDeviceToHost, t->stream),
      hipMemcpyAsync(tchild.data(), t->W.t_child, tchild.size(), hipMemcpyDeviceToHost, t->stream),
      hipMemcpyAsync(tflen.data(), t->W.t_flags_len, n * 4, hipMemcpyDeviceToHost, t->stream),
      hipMemcpyAsync(tclen.data(), t->W.t_child_len, n * 4, hipMemcpyDeviceToHost, t->stream)};
  const hipError_t se = hipStreamSynchronize(t->stream);
  for (hipError_t e : {ce[0], ce[1], ce[2], ce[3], se})
    if (e != hipSuccess) return fail(AVGPU_EHIP, std::string("test_genomes copy: ") + hipGetErrorString(e));
  size_t off = 0;
  for (int i = 0; i < n; i++) {
    avgpu_test_result& r = results[i];
    const avgpu_cpu_state& s = st[i];
    memset(&r, 0, sizeof(r));
    r.divided = s.num_divides > 0;
    r.copied_size = s.copied_size;
    r.executed_size = s.executed_size;
    r.gestation_time = s.gestation_time;
    r.genome_length = s.genome_length;
    r.time_used = s.time_used;
    r.merit = s.merit;
    r.fitness = s.fitness;
    for (int k = 0; k < AVGPU_MAX_REACTIONS; k++) r.task_count[k] = s.last_task_count[k];
    r.offspring_len = r.divided ? tclen[i] : 0;
    bool same = r.divided && tclen[i] == lens[i];
    for (int k = 0; same && k < lens[i]; k++)
      same = (w->code2op[tchild[(size_t)i * TAPE_SLOT + k]] == genomes[off + k]);
    r.copy_true = same;
    if (executed_flags && flags_cap > 0) {
      char* dst = executed_flags + (size_t)i * flags_cap;
      memset(dst, 0, flags_cap);
      if (r.divided) {
        const int m = std::min(tflen[i], flags_cap - 1);
        memcpy(dst, tflags.data() + (size_t)i * TAPE_SLOT, m);
      } else {
        const int m = std::min(s.mem_size, flags_cap - 1);
        for (int k = 0; k < m; k++) dst[k] = (fl[(size_t)i * AVGPU_MAX_GENOME + k] & 0x04) ? '+' : '-';
      }
    }
    if (offspring) {
      uint8_t* d = offspring + (size_t)i * AVGPU_MAX_GENOME;
      memset(d, 0, AVGPU_MAX_GENOME);
      for (int k = 0; k < r.offspring_len; k++)
        d[k] = (uint8_t)w->code2op[tchild[(size_t)i * TAPE_SLOT + k]];
    }
    off += lens[i];
  }
  return 0;
}

// ---- mutational landscapes (landscape.hip) ----
// the scratch test world and the view's per-chunk scratch, for the current chunk
static int land_alloc(avgpu_world* w) {
  Landscapes& D = w->land;
  if (D.world && D.view.chunk == D.chunk) return 0;
  if (D.world) {
    avgpu_destroy(D.world);
    D.world = nullptr;
  }
  avgpu_cfg tc = w->cfg;     // the test CPU: mutations off (as avgpu_test_genomes)
  tc.copy_mut_prob = 0; tc.divide_mut_prob = 0; tc.divide_ins_prob = 0; tc.divide_del_prob = 0;
  const int64_t n = D.chunk;
  avgpu_world* t = create_world(&tc, w->device, n, true);
  if (!t) return AVGPU_ENOMEM;
  t->time_every = 0;         // its interpreter phases are not bracketed: the call times itself
  LandScratch S = {};
  S.chunk = n;
  int rc = t->alloc(&S.budget, (size_t)n);
  if (rc == 0) rc = t->alloc(&S.fit, (size_t)n);
  if (rc == 0) rc = t->alloc(&S.dep, (size_t)n);
  if (rc == 0) rc = t->alloc(&S.count, 2);
  for (int d = 0; d < 2 && rc == 0; d++) {
    if ((rc = t->alloc(&S.src[d], (size_t)n)) < 0) break;
    if ((rc = t->alloc(&S.glen[d], (size_t)n)) < 0) break;
    rc = t->alloc(&S.gen[d], (size_t)n * TAPE_SLOT);
  }
  if (rc == 0 && hipStreamSynchronize(t->stream) != hipSuccess) rc = fail(AVGPU_EHIP, "landscape scratch");
  if (rc == 0) rc = D.timer.create();  // (once: it outlives the scratch world)
  if (rc < 0) {
    avgpu_destroy(t);                  // (leaves the error string alone)
    return rc;
  }
  D.world = t;
  D.view = S;
  return 0;
}

int avgpu_set_landscape_chunk(avgpu_world* w, int64_t cells) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (cells <= 0 || cells % LAND_TILE != 0 || cells > (1ll << 30))
    return fail(AVGPU_EINVAL, "landscape chunk: a positive multiple of 256 cells, at most 2^30");
  w->land.chunk = cells;      // the scratch world follows at the next avgpu_landscapes
  return 0;
}

int avgpu_last_landscape_ms(avgpu_world* w, double* device_ms, int64_t* mutants, int64_t* gestations) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (device_ms) *device_ms = w->land.ms;
  if (mutants) *mutants = w->land.mutants;
  if (gestations) *gestations = w->land.runs;
  return 0;
}

// mutants of a genome of L sites (K = num_insts - 1); `viable`: its base fitness is not 0
static int64_t land_count(int mode, int64_t L, int64_t K, bool viable) {
  switch (mode) {
    case LAND_SUB1: return viable ? L * K : 0;
    case LAND_SUB2: return viable ? L * (L - 1) / 2 * K * K : 0;
    case LAND_INS: return (L + 1) * (K + 1);
    case LAND_DEL: return L;
  }
  return 0;
}

// The one body of the three landscape calls.  mode LAND_SUB1 / LAND_SUB2
// (avgpu_landscapes), LAND_INS / LAND_DEL (avgpu_landscapes_indel); epi: the
// all-pairs test (avgpu_landscape_pairs), a LAND_SUB1 pass with the chart kept
// on the device and a LAND_SUB2 pass classified against it.
static int land_call(avgpu_world* w, const char* who, int n, const uint8_t* genomes, const int32_t* lens, int mode,
                     avgpu_landscape* out, int32_t* site_count, double* fitness_chart, avgpu_epistasis* epi) {
  auto refuse = [&](const char* what) { return fail(AVGPU_EINVAL, (std::string(who) + ": " + what).c_str()); };
  int rc = ready(w);
  if (rc < 0) return rc;
  if (n <= 0 || !genomes || !lens || !out) return refuse("n <= 0 or a NULL argument");
  const int I = w->n_ops;
  const int64_t K = I - 1;
  if (I < 2) return refuse("an instruction set of one instruction has no mutants");
  if (w->cfg.test_cpu_time_mod < 0 || w->cfg.test_cpu_time_mod > (BUDGET_PRIM - 1) / AVGPU_MAX_GENOME)
    return refuse("TEST_CPU_TIME_MOD x genome length outside [0, 2^30)");
  const int distance = mode == LAND_SUB2 ? 2 : 1;   // (the rows of an indel landscape report 1: the actions' m_dist)
  // the mutants of the n genomes back to back, their tiles, their sites
  // (the all-pairs test lays its mutants out once the base fitnesses are known)
  std::vector<int64_t> base_off((size_t)n), mut_off((size_t)n + 1), tile_off((size_t)n + 1), site_off((size_t)n);
  std::vector<uint8_t> base_op, base_code;
  int64_t sites = 0;
  auto lay_out = [&](int md, const double* base_fit) -> int {
    int64_t m = 0, t = 0;
    for (int g = 0; g < n; g++) {
      const int64_t cnt = land_count(md, lens[g], K, !base_fit || base_fit[g] != 0.0);
      mut_off[g] = m; tile_off[g] = t;
      if (__builtin_add_overflow(m, cnt, &m)) return refuse("the mutant count overflows int64");
      t += (cnt + LAND_TILE - 1) / LAND_TILE;
    }
    mut_off[n] = m; tile_off[n] = t;
    return 0;
  };
  {
    size_t in = 0;
    for (int g = 0; g < n; g++) {
      const int64_t L = lens[g];
      if (L < 1 || L > AVGPU_MAX_GENOME) return refuse("genome length out of range");
      if (mode == LAND_INS && L == AVGPU_MAX_GENOME) return refuse("an insertion mutant would exceed AVGPU_MAX_GENOME sites");
      if (mode == LAND_DEL && L == 1) return refuse("a one-site genome has no deletion mutants");
      if (epi && L == 1) return refuse("a one-site genome has no pairs of sites");
      base_off[g] = (int64_t)base_op.size();
      site_off[g] = sites;
      sites += mode == LAND_INS ? L + 1 : L;     // Reset (main/cLandscape.cc:49-95): site_count has size + 1 entries
      for (int64_t k = 0; k < L; k++) {
        const uint8_t op = genomes[in + (size_t)k];
        if (op >= I) return refuse("genome op outside the instruction set");
        base_op.push_back(op);
        base_code.push_back(w->op2code[op]);
      }
      in += (size_t)L;
      while (base_op.size() & 15) { base_op.push_back(0); base_code.push_back(0); }   // 16-B groups
    }
    // one zero group behind the last genome: a length-changing edit looks one
    // site past a genome that fills its last group
    base_op.insert(base_op.end(), 16, 0);
    base_code.insert(base_code.end(), 16, 0);
  }
  // (pairs: every base taken as viable bounds the tiles and checks the count)
  int64_t tiles2 = 0;
  if (epi) {
    if ((rc = lay_out(LAND_SUB2, nullptr)) < 0) return rc;
    tiles2 = tile_off[n];
  }
  if ((rc = lay_out(mode, nullptr)) < 0) return rc;
  int64_t total = mut_off[n], tiles = tile_off[n];
  if ((rc = land_alloc(w)) < 0) return rc;
  avgpu_world* t = w->land.world;
  LandScratch S = w->land.view;
  // the scratch world runs in this world's stream order, with its tables
  t->stream = w->stream;
  struct Restore { avgpu_world* t; ~Restore() { t->stream = t->own_stream.get(); } } restore{t};
  if ((rc = copy_tables(t, w)) < 0) return rc;
  std::vector<DevBuf<uint8_t>> bufs;     // the call's buffers: each waits for w->stream before it goes
  auto dev = [&](auto** p, size_t count, const void* src) -> int {
    const size_t bytes = std::max<size_t>(count * sizeof(**p), 16);
    bufs.emplace_back(w->stream);
    const int arc = bufs.back().alloc(bytes);
    if (arc < 0) return arc;
    void* q = bufs.back().get();
    *p = reinterpret_cast<std::remove_reference_t<decltype(*p)>>(q);
    if (src) HIPCHK(hipMemcpyAsync(q, src, count * sizeof(**p), hipMemcpyHostToDevice, w->stream));
    else HIPCHK(hipMemsetAsync(q, 0, bytes, w->stream));
    return 0;
  };
  uint8_t *d_op = nullptr, *d_code = nullptr, *d_o2c = nullptr;
  int64_t *d_boff = nullptr, *d_moff = nullptr, *d_toff = nullptr, *d_soff = nullptr;
  int32_t* d_len = nullptr;
  const bool want_chart = fitness_chart || epi;          // the pairs are classified against it on the device
  S.n = n; S.num_insts = I; S.time_mod = w->cfg.test_cpu_time_mod;
  if ((rc = dev(&d_op, base_op.size(), base_op.data())) < 0 || (rc = dev(&d_code, base_code.size(), base_code.data())) < 0 ||
      (rc = dev(&d_boff, (size_t)n, base_off.data())) < 0 || (rc = dev(&d_len, (size_t)n, lens)) < 0 ||
      (rc = dev(&d_moff, (size_t)n + 1, nullptr)) < 0 || (rc = dev(&d_toff, (size_t)n + 1, nullptr)) < 0 ||
      (rc = dev(&d_soff, (size_t)n, site_off.data())) < 0 || (rc = dev(&d_o2c, AVGPU_MAX_INST, w->op2code)) < 0 ||
      (rc = dev(&S.base_fit, (size_t)n, nullptr)) < 0 || (rc = dev(&S.base_merit, (size_t)n, nullptr)) < 0 ||
      (rc = dev(&S.base_gest, (size_t)n, nullptr)) < 0 || (rc = dev(&S.parts, (size_t)tiles, nullptr)) < 0 ||
      (rc = dev(&S.rows, (size_t)n, nullptr)) < 0 ||
      (!epi && (rc = dev(&S.site_count, (size_t)sites, nullptr)) < 0) ||
      (want_chart && (rc = dev(&S.chart, (size_t)sites * I, nullptr)) < 0) ||
      (epi && ((rc = dev(&S.eparts, (size_t)tiles2, nullptr)) < 0 || (rc = dev(&S.erows, (size_t)n, nullptr)) < 0)))
    return rc;
  S.base_op = d_op; S.base_code = d_code; S.base_off = d_boff; S.len = d_len;
  S.mut_off = d_moff; S.tile_off = d_toff; S.site_off = d_soff; S.op2code = d_o2c;
  int64_t runs = 0;
  // cells [0, cnt) run mutants m0 .. m0 + cnt - 1 (LAND_BASE: base genomes)
  // through the recursion: depth d's survivors are depth d + 1's cells.  The
  // organisms are classified by their own length (an insertion mutant of a
  // 320-site genome leaves the interpreter's first size class).
  auto run_chunk = [&](int md, int64_t m0, int cnt) -> int {
    HIPCHK(hipMemsetAsync(S.count, 0, 2 * sizeof(int32_t), w->stream));
    launch_land_seed(t->W, S, w->stream, md, m0, cnt);
    int cntd = cnt;
    for (int depth = 0; depth < 3 && cntd > 0; depth++) {
      if (depth > 0) launch_land_seed_next(t->W, S, w->stream, depth, cntd);
      launch_reset_counts(t->W, w->stream);
      launch_classify_uniform(t->W, w->stream, 0, cntd, S.budget, 0);
      HIPCHK(hipGetLastError());
      const int irc = interpret(t, AVGPU_MODE_TEST, 0, cntd);
      if (irc < 0) return irc;
      launch_land_judge(t->W, S, w->stream, md, depth, m0, cntd);
      HIPCHK(hipGetLastError());
      runs += cntd;
      if (depth == 2) break;
      int32_t next = 0;
      COPY_SYNC(w, &next, S.count + depth, sizeof(next), hipMemcpyDeviceToHost);
      cntd = next;
    }
    return 0;
  };
  // every mutant of the layout in mut_off / tile_off, chunk by chunk, each
  // chunk's tiles reduced behind it (pairs: by TestMutPair's classification)
  auto run_pass = [&](int md, bool pairs) -> int {
    COPY_SYNC(w, d_moff, mut_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    COPY_SYNC(w, d_toff, tile_off.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    const int64_t tot = mut_off[n], nt = tile_off[n];
    int g = 0;                               // the genome holding the chunk's end
    int64_t m0 = 0, t0 = 0;
    while (m0 < tot) {
      // the chunk ends at the last tile boundary within S.chunk mutants
      int64_t m1 = tot, t1 = nt;
      if (m0 + S.chunk < tot) {
        while (mut_off[(size_t)g + 1] <= m0 + S.chunk) g++;
        const int64_t full = (m0 + S.chunk - mut_off[g]) / LAND_TILE;
        m1 = mut_off[g] + full * LAND_TILE;
        t1 = tile_off[g] + full;
      }
      const int crc = run_chunk(md, m0, (int)(m1 - m0));
      if (crc < 0) return crc;
      if (pairs) launch_land_epi_reduce(S, w->stream, m0, t0, t1);
      else launch_land_reduce(S, w->stream, md, m0, t0, t1);
      HIPCHK(hipGetLastError());
      m0 = m1; t0 = t1;
    }
    return 0;
  };
  RCCHK(w->land.timer.start(w->stream));
  for (int64_t m0 = 0; m0 < n; m0 += S.chunk)
    if ((rc = run_chunk(LAND_BASE, m0, (int)std::min<int64_t>(S.chunk, n - m0))) < 0) return rc;
  runs = 0;                                  // (the base genomes' runs are not the landscape's)
  std::vector<double> base_fit;
  if (epi) {
    // TestAllPairs (main/cLandscape.cc:792-793): a base of fitness 0 stops
    // there -- no one-step pass, no pairs.  8 B per genome cross to the host.
    base_fit.resize((size_t)n);
    COPY_SYNC(w, base_fit.data(), S.base_fit, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
    if ((rc = lay_out(LAND_SUB1, base_fit.data())) < 0) return rc;
    total = mut_off[n];
  }
  if ((rc = run_pass(mode, false)) < 0) return rc;
  // the rows of the all-pairs test report Reset's distance 0 (it never calls Process)
  launch_land_rows(S, w->stream, epi ? 0 : distance);
  HIPCHK(hipGetLastError());
  if (epi) {
    if ((rc = lay_out(LAND_SUB2, base_fit.data())) < 0) return rc;
    total += mut_off[n];
    if ((rc = run_pass(LAND_SUB2, true)) < 0) return rc;
    launch_land_epi_rows(S, w->stream);
    HIPCHK(hipGetLastError());
  }
  RCCHK(w->land.timer.stop(w->stream));
  std::vector<avgpu_landscape> rows((size_t)n);
  std::vector<avgpu_epistasis> erows(epi ? (size_t)n : 0);
  std::vector<int32_t> sc(epi ? 0 : (size_t)sites);
  std::vector<double> chart(fitness_chart ? (size_t)sites * I : 0);
  HIPCHK(hipMemcpyAsync(rows.data(), S.rows, rows.size() * sizeof(avgpu_landscape), hipMemcpyDeviceToHost, w->stream));
  if (!epi) HIPCHK(hipMemcpyAsync(sc.data(), S.site_count, sc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
  if (epi)
    HIPCHK(hipMemcpyAsync(erows.data(), S.erows, erows.size() * sizeof(avgpu_epistasis), hipMemcpyDeviceToHost, w->stream));
  if (fitness_chart)
    HIPCHK(hipMemcpyAsync(chart.data(), S.chart, chart.size() * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  RCCHK(w->land.timer.elapsed(&w->land.ms));
  w->land.mutants = total;
  w->land.runs = runs;
  // cLandscape::Process (main/cLandscape.cc:158-169): a site's entropy is the
  // log of its legal states, the unmutated one included (ProcessInsert,
  // ProcessDelete and TestAllPairs compute none); ProcessDump's and
  // BuildFitnessChart's chart holds the base fitness at the original instruction
  const bool entropy = !epi && (mode == LAND_SUB1 || mode == LAND_SUB2);
  const double max_ent = std::log((double)I);
  for (int g = 0; g < n; g++) {
    avgpu_landscape& r = rows[(size_t)g];
    double ent = 0.0;
    for (int64_t k = 0; k < lens[g] && (entropy || fitness_chart); k++) {
      const size_t site = (size_t)(site_off[g] + k);
      if (entropy) ent += std::log((double)sc[site] + 1) / max_ent;
      if (fitness_chart) chart[site * I + base_op[(size_t)(base_off[g] + k)]] = r.base_fitness;
    }
    r.total_entropy = entropy ? ent : 0.0;
    r.complexity = entropy ? (double)lens[g] - ent : 0.0;
  }
  memcpy(out, rows.data(), rows.size() * sizeof(avgpu_landscape));
  if (epi) memcpy(epi, erows.data(), erows.size() * sizeof(avgpu_epistasis));
  if (site_count) memcpy(site_count, sc.data(), sc.size() * sizeof(int32_t));
  if (fitness_chart) memcpy(fitness_chart, chart.data(), chart.size() * sizeof(double));
  return 0;
}

int avgpu_landscapes(avgpu_world* w, int n, const uint8_t* genomes, const int32_t* lens, int distance,
                     avgpu_landscape* out, int32_t* site_count, double* fitness_chart) {
  if (distance != 1 && distance != 2) return fail(AVGPU_EINVAL, "avgpu_landscapes: distance must be 1 or 2");
  if (fitness_chart && distance != 1) return fail(AVGPU_EINVAL, "avgpu_landscapes: the fitness chart is distance 1 only");
  return land_call(w, "avgpu_landscapes", n, genomes, lens, distance == 1 ? LAND_SUB1 : LAND_SUB2, out, site_count,
                   fitness_chart, nullptr);
}

int avgpu_landscapes_indel(avgpu_world* w, int n, const uint8_t* genomes, const int32_t* lens, int kind,
                           avgpu_landscape* out, int32_t* site_count) {
  if (kind != AVGPU_LAND_INSERT && kind != AVGPU_LAND_DELETE)
    return fail(AVGPU_EINVAL, "avgpu_landscapes_indel: kind must be AVGPU_LAND_INSERT or AVGPU_LAND_DELETE");
  return land_call(w, "avgpu_landscapes_indel", n, genomes, lens, kind == AVGPU_LAND_INSERT ? LAND_INS : LAND_DEL, out,
                   site_count, nullptr, nullptr);
}

int avgpu_landscape_pairs(avgpu_world* w, int n, const uint8_t* genomes, const int32_t* lens, avgpu_landscape* out,
                          avgpu_epistasis* epi, double* fitness_chart) {
  if (!epi) return fail(AVGPU_EINVAL, "avgpu_landscape_pairs: a NULL argument");
  return land_call(w, "avgpu_landscape_pairs", n, genomes, lens, LAND_SUB1, out, nullptr, fitness_chart, epi);
}

}  // extern "C"
