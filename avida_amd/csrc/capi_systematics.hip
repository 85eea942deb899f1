// capi_systematics.hip -- the census, the genotype table, the genotype arbiter, genotype keys.
#include "host.h"

using namespace avh;

extern "C" {

int avgpu_get_census(avgpu_world* w, int64_t first, int64_t count, avgpu_census* out) {
  if (!w || !out || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  DevBuf<avgpu_census> d(w->stream);
  const int rc = d.alloc(count);
  if (rc < 0) return rc;
  launch_get_census(w->W, w->stream, first, count, d.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d.get(), count * sizeof(avgpu_census), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

// room for m rows in gt_rows (the stream is idle), grown to the largest table seen
static int genotype_rows_reserve(avgpu_world* w, int64_t m) {
  if (w->gt_rows_cap >= m) return 0;
  w->gt_rows_cap = 0;
  const int64_t want = std::min<int64_t>(w->gt.n, std::max<int64_t>(m + m / 4, 1024));
  const int rc = w->gt_rows.alloc((size_t)want);
  if (rc < 0) return rc;
  w->gt_rows_cap = want;
  return 0;
}

// the grouping's scratch: 24 B per cell for the two (key, cell) buffers of
// the sort, the per-tile histograms and segment tiles on top (under 1 B per cell)
static int genotypes_alloc(avgpu_world* w) {
  if (w->gt_ready) return 0;
  GtScratch& S = w->gt;
  S.n = w->W.n;
  S.nblk = (S.n + GT_SORT_TILE - 1) / GT_SORT_TILE;
  S.ntile = (S.n + GT_SEG_TILE - 1) / GT_SEG_TILE;
  int rc = 0;
  for (int k = 0; k < 2 && rc == 0; k++) {
    if ((rc = w->alloc(&S.key[k], (size_t)S.n)) < 0) break;
    rc = w->alloc(&S.cell[k], (size_t)S.n);
  }
  if (rc == 0) rc = w->alloc(&S.hist, (size_t)256 * S.nblk);
  if (rc == 0) rc = w->alloc(&S.dtot, 256);
  if (rc == 0) rc = w->alloc(&S.tile_agg, (size_t)S.ntile);
  if (rc == 0) rc = w->alloc(&S.carry, (size_t)S.ntile);
  if (rc == 0) rc = w->alloc(&S.tile_flag, (size_t)S.ntile);
  if (rc == 0) rc = w->alloc(&S.tile_tails, (size_t)S.ntile);
  if (rc == 0) rc = w->alloc(&S.row_off, (size_t)S.ntile);
  if (rc == 0) rc = w->alloc(&S.totals, 1);
  if (rc < 0) return rc;
  for (Event& e : w->ev_gt)
    if ((rc = e.create()) < 0) return rc;
  w->gt_ready = true;
  return 0;
}

int avgpu_get_genotypes(avgpu_world* w, avgpu_genotype* out, int64_t cap, avgpu_genotype_totals* totals) {
  if (!w || cap < 0) return fail(AVGPU_EINVAL, "avgpu_get_genotypes: NULL world or negative cap");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype table on strip tiles");
  if (w->W.n >= (1ll << 31) - GT_SORT_TILE) return fail(AVGPU_EUNSUPPORTED, "genotype table of 2^31 cells or more");
  int rc = genotypes_alloc(w);
  if (rc < 0) return rc;
  const GtScratch& S = w->gt;
  HIPCHK(hipMemsetAsync(S.totals, 0, sizeof(avgpu_genotype_totals), w->stream));
  HIPCHK(hipEventRecord(w->ev_gt[0], w->stream));
  launch_genotype_group(w->W, S, w->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev_gt[1], w->stream));
  avgpu_genotype_totals t;
  COPY_SYNC(w, &t, S.totals, sizeof(t), hipMemcpyDeviceToHost);
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, w->ev_gt[0], w->ev_gt[1]));
  w->gt_ms = ms;
  w->gt_bytes = sizeof(t);
  if (totals) *totals = t;
  if (!out || cap == 0) return 0;
  if (cap < t.num_genotypes)
    return fail(AVGPU_EINVAL, "avgpu_get_genotypes: cap " + std::to_string(cap) + " rows, the table has " +
                                  std::to_string(t.num_genotypes));
  if (t.num_genotypes == 0) return 0;
  if ((rc = genotype_rows_reserve(w, t.num_genotypes)) < 0) return rc;   // the stream is idle (COPY_SYNC above)
  HIPCHK(hipEventRecord(w->ev_gt[2], w->stream));
  launch_genotype_rows(w->W, S, w->gt_rows.get(), w->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev_gt[3], w->stream));
  COPY_SYNC(w, out, w->gt_rows.get(), (size_t)t.num_genotypes * sizeof(avgpu_genotype), hipMemcpyDeviceToHost);
  HIPCHK(hipEventElapsedTime(&ms, w->ev_gt[2], w->ev_gt[3]));
  w->gt_ms += ms;
  w->gt_bytes += t.num_genotypes * (int64_t)sizeof(avgpu_genotype);
  return (int)t.num_genotypes;
}

int avgpu_last_genotypes_ms(avgpu_world* w, double* device_ms, int64_t* bytes_copied) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (device_ms) *device_ms = w->gt_ms;
  if (bytes_copied) *bytes_copied = w->gt_bytes;
  return 0;
}

// ---- the device-resident genotype arbiter (arbiter.hip) ----
static void arbiter_fresh_summary(avgpu_arbiter_summary* s) {
  memset(s, 0, sizeof(*s));
  s->next_id = 1;
  s->dominant_row = -1;
}

// the fixed-size part: state, counters, name counters, the pinned summary
static int arbiter_alloc(avgpu_world* w) {
  if (w->arb_ready) return 0;
  ArbScratch& A = w->arb;
  int rc = w->alloc(&A.state, 1);
  if (rc == 0) rc = w->alloc(&A.work, 1);
  if (rc == 0) rc = w->alloc(&A.sz_count, AVGPU_MAX_GENOME + 1);
  if (rc < 0) return rc;
  if (w->arb_sum.alloc(1, hipHostMallocMapped | hipHostMallocCoherent) < 0 ||
      hipHostGetDevicePointer((void**)&A.d_sum, w->arb_sum.get(), 0) != hipSuccess)
    return fail(AVGPU_ENOMEM, "pinned arbiter summary");
  A.h_sum = w->arb_sum.get();
  memset(A.h_sum, 0, sizeof(avgpu_arbiter_summary));
  ArbState st = {1, 0, 0, 0ull};
  COPY_SYNC(w, A.state, &st, sizeof(st), hipMemcpyHostToDevice);
  for (Event& e : w->ev_arb)
    if ((rc = e.create()) < 0) return rc;
  arbiter_fresh_summary(&w->arb_last);
  w->arb_n = 0;
  w->arb_ready = true;
  return 0;
}

// room for `rows` rows (the stream is idle); keep: the current state survives
static int arbiter_reserve(avgpu_world* w, int64_t rows, bool keep) {
  ArbScratch& A = w->arb;
  if (rows <= A.cap) return 0;
  const int64_t want = std::min<int64_t>(std::max<int64_t>(w->W.n, 1), std::max<int64_t>(rows + rows / 4, 1024));
  // into locals (the copies wait for w->stream before a failure frees them),
  // swapped in on success: the old buffers go with the locals
  DevBuf<avgpu_arbiter_row> row[2] = {DevBuf<avgpu_arbiter_row>(w->stream), DevBuf<avgpu_arbiter_row>(w->stream)};
  DevBuf<uint64_t> key[2] = {DevBuf<uint64_t>(w->stream), DevBuf<uint64_t>(w->stream)};
  DevBuf<avgpu_genotype> table(w->stream);
  int rc = table.alloc((size_t)want);
  for (int k = 0; k < 2 && rc == 0; k++)
    if ((rc = row[k].alloc((size_t)want)) == 0) rc = key[k].alloc((size_t)want);
  if (rc < 0) return rc;
  if (keep && w->arb_n > 0) {
    hipError_t e = hipMemcpyAsync(row[A.cur].get(), A.row[A.cur], (size_t)w->arb_n * sizeof(avgpu_arbiter_row),
                                  hipMemcpyDeviceToDevice, w->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(key[A.cur].get(), A.key[A.cur], (size_t)w->arb_n * sizeof(uint64_t),
                         hipMemcpyDeviceToDevice, w->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(table.get(), A.table, (size_t)w->arb_n * sizeof(avgpu_genotype), hipMemcpyDeviceToDevice,
                         w->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
    if (e != hipSuccess) return fail(AVGPU_ENOMEM, std::string("arbiter rows: ") + hipGetErrorString(e));
  }
  for (int k = 0; k < 2; k++) {
    w->arb_row[k] = std::move(row[k]);
    w->arb_key[k] = std::move(key[k]);
    A.row[k] = w->arb_row[k].get();
    A.key[k] = w->arb_key[k].get();
  }
  w->arb_table = std::move(table);
  A.table = w->arb_table.get();
  A.cap = want;
  return 0;
}

// ---- the lineage store (lineage.hip) ----
// room for `rows` rows (the stream is idle): 1.25x growth, the held rows kept
static int lineage_reserve_rows(avgpu_world* w, int64_t rows) {
  LinScratch& L = w->lin;
  if (rows <= L.cap) return 0;
  const int64_t want = std::max<int64_t>(rows + rows / 4, std::max<int64_t>(w->lin_rows_hint, 1));
  DevBuf<avgpu_lineage_row> nb(w->stream);
  int rc = nb.alloc((size_t)want);
  if (rc < 0) return rc;
  if (L.n > 0)
    COPY_SYNC(w, nb.get(), L.rows, (size_t)L.n * sizeof(avgpu_lineage_row), hipMemcpyDeviceToDevice);
  w->lin_rows = std::move(nb);
  L.rows = w->lin_rows.get();
  L.cap = want;
  return 0;
}
static int lineage_reserve_arena(avgpu_world* w, int64_t bytes) {
  LinScratch& L = w->lin;
  if (bytes <= L.arena_cap) return 0;
  const int64_t want = (std::max<int64_t>(bytes + bytes / 4, std::max<int64_t>(w->lin_arena_hint, 16)) + 15) & ~15ll;
  DevBuf<uint8_t> nb(w->stream);
  int rc = nb.alloc((size_t)want);
  if (rc < 0) return rc;
  if (L.arena_bytes > 0) COPY_SYNC(w, nb.get(), L.arena, (size_t)L.arena_bytes, hipMemcpyDeviceToDevice);
  w->lin_arena = std::move(nb);
  L.arena = w->lin_arena.get();
  L.arena_cap = want;
  return 0;
}
// the scratch rows of a classification (its new rows) or a prune (every row)
static int lineage_reserve_scratch(avgpu_world* w, int64_t n) {
  LinScratch& L = w->lin;
  if (n <= L.scap) return 0;
  const int64_t want = std::max<int64_t>(n + n / 4, 64);
  HIPCHK(hipStreamSynchronize(w->stream));
  int rc = w->lin_idx.alloc((size_t)want);
  if (rc == 0) rc = w->lin_asz.alloc((size_t)want);
  if (rc == 0) rc = w->lin_mark.alloc((size_t)want);
  if (rc == 0) rc = w->lin_newcell.alloc((size_t)want);
  L.idx = w->lin_idx.get(); L.asz = w->lin_asz.get(); L.mark = w->lin_mark.get(); L.newcell = w->lin_newcell.get();
  L.scap = rc == 0 ? want : 0;
  return rc;
}
static int lineage_clear(avgpu_world* w) {
  LinScratch& L = w->lin;
  L.n = 0;
  L.arena_bytes = 0;
  w->lin_dropped = 0;
  if (L.ctr) SET_SYNC(w, L.ctr, 0, LIN_CTR_WORDS * sizeof(unsigned long long));
  return 0;
}
static int lineage_summary(avgpu_world* w, avgpu_lineage_summary* s) {
  LinScratch& L = w->lin;
  unsigned long long c[LIN_CTR_WORDS];
  HIPCHK(hipMemsetAsync(L.ctr + LIN_MAXDEPTH, 0, sizeof(unsigned long long), w->stream));
  launch_lineage_max_depth(L, w->stream);
  HIPCHK(hipGetLastError());
  COPY_SYNC(w, c, L.ctr, sizeof(c), hipMemcpyDeviceToHost);
  memset(s, 0, sizeof(*s));
  s->rows = L.n;
  s->active_rows = w->arb_ready ? w->arb_n : 0;
  s->arena_bytes = L.arena_bytes;
  s->num_orphans = (int64_t)c[LIN_ORPHANS];
  s->num_unsequenced = (int64_t)c[LIN_UNSEQ];
  s->max_depth = (int64_t)c[LIN_MAXDEPTH];
  s->dropped_last_prune = w->lin_dropped;
  return 0;
}
// one classification's store maintenance (the stream is idle; the arbiter's
// buffers are swapped): n_prev rows and next id id0 before, m rows after
static int lineage_step(avgpu_world* w, int64_t n_prev, int64_t id0, int64_t m, int64_t update) {
  LinScratch& L = w->lin;
  const int64_t n_new = w->arb_last.next_id - id0;
  if (n_new < 0 || n_new > m) return fail(AVGPU_ESTATE, "lineage: new ids outside the classification");
  int rc = lineage_reserve_rows(w, L.n + n_new);
  if (rc == 0) rc = lineage_reserve_scratch(w, n_new);
  if (rc < 0) return rc;
  HIPCHK(hipEventRecord(w->ev_lin[0], w->stream));
  launch_lineage_classify(L, w->arb, w->W, n_prev, m, id0, n_new, update, w->stream);
  HIPCHK(hipGetLastError());
  if (n_new > 0) {
    unsigned long long total = 0;
    COPY_SYNC(w, &total, L.ctr + LIN_TOTAL_A, sizeof(total), hipMemcpyDeviceToHost);
    if ((int64_t)total < L.arena_bytes) return fail(AVGPU_ESTATE, "lineage: arena total went down");
    if ((rc = lineage_reserve_arena(w, (int64_t)total)) < 0) return rc;
    launch_lineage_copy(L, w->W, n_new, w->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(w->ev_lin[1], w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    L.n += n_new;
    L.arena_bytes = (int64_t)total;
  } else {
    HIPCHK(hipEventRecord(w->ev_lin[1], w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
  }
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, w->ev_lin[0], w->ev_lin[1]));
  w->lin_ms = ms;
  return 0;
}

int avgpu_classify_genotypes(avgpu_world* w, int64_t update, int32_t threshold, avgpu_arbiter_summary* out) {
  if (!w || !out || threshold < 1)
    return fail(AVGPU_EINVAL, "avgpu_classify_genotypes: NULL world, NULL out or threshold < 1");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter on strip tiles");
  if (w->W.n >= (1ll << 31) - GT_SORT_TILE) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter of 2^31 cells or more");
  int rc = genotypes_alloc(w);
  if (rc == 0) rc = arbiter_alloc(w);
  if (rc < 0) return rc;
  const GtScratch& S = w->gt;
  ArbScratch& A = w->arb;
  const int64_t lin_prev = w->arb_n, lin_id0 = w->arb_last.next_id;
  // the first part: the grouping; its totals are the summary's first fields
  HIPCHK(hipMemsetAsync(S.totals, 0, sizeof(avgpu_genotype_totals), w->stream));
  HIPCHK(hipEventRecord(w->ev_arb[0], w->stream));
  launch_genotype_group(w->W, S, w->stream);
  launch_arbiter_begin(A, S, update, w->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev_arb[1], w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  const int64_t m = __atomic_load_n(&A.h_sum->num_genotypes, __ATOMIC_ACQUIRE);
  if (m < 0 || m > S.n) return fail(AVGPU_ESTATE, "genotype arbiter: row count outside the world");
  if ((rc = genotype_rows_reserve(w, m)) < 0) return rc;   // the stream is idle
  if ((rc = arbiter_reserve(w, std::max<int64_t>(m, 1), true)) < 0) return rc;
  // every id of the new state is below next_id + m
  int id_bits = 1;
  while (id_bits < 50 && ((w->arb_last.next_id + m) >> id_bits) != 0) id_bits++;
  if (((w->arb_last.next_id + m) >> id_bits) != 0) return fail(AVGPU_EUNSUPPORTED, "genotype ids of 2^50 or more");
  HIPCHK(hipEventRecord(w->ev_arb[2], w->stream));
  if (m > 0) {
    launch_genotype_rows(w->W, S, w->gt_rows.get(), w->stream);
    HIPCHK(hipMemcpyAsync(A.table, w->gt_rows.get(), (size_t)m * sizeof(avgpu_genotype), hipMemcpyDeviceToDevice,
                          w->stream));
  }
  launch_arbiter_classify(A, S, A.table, m, w->arb_n, update, threshold, id_bits, w->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev_arb[3], w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  A.cur ^= 1;
  w->arb_n = m;
  memcpy(&w->arb_last, A.h_sum, sizeof(avgpu_arbiter_summary));
  *out = w->arb_last;
  float ms0 = 0.f, ms1 = 0.f;
  HIPCHK(hipEventElapsedTime(&ms0, w->ev_arb[0], w->ev_arb[1]));
  HIPCHK(hipEventElapsedTime(&ms1, w->ev_arb[2], w->ev_arb[3]));
  w->arb_ms = (double)ms0 + (double)ms1;
  w->arb_bytes = sizeof(avgpu_arbiter_summary);
  if (w->lin_on) return lineage_step(w, lin_prev, lin_id0, m, update);
  return 0;
}

int avgpu_get_arbiter(avgpu_world* w, avgpu_arbiter_row* rows, avgpu_genotype* table, int64_t cap,
                      avgpu_arbiter_summary* summary, int64_t* sz_count) {
  if (!w || cap < 0) return fail(AVGPU_EINVAL, "avgpu_get_arbiter: NULL world or negative cap");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter on strip tiles");
  if (!w->arb_ready) {                          // never classified or set: a new world's state, nothing allocated
    if (summary) arbiter_fresh_summary(summary);
    if (sz_count) memset(sz_count, 0, (AVGPU_MAX_GENOME + 1) * sizeof(int64_t));
    return 0;
  }
  const ArbScratch& A = w->arb;
  const int64_t m = w->arb_n;
  const bool want_rows = (rows || table) && cap > 0;
  if (want_rows && cap < m)
    return fail(AVGPU_EINVAL, "avgpu_get_arbiter: cap " + std::to_string(cap) + " rows, the arbiter has " +
                                  std::to_string(m));
  if (summary) *summary = w->arb_last;
  if (sz_count)
    HIPCHK(hipMemcpyAsync(sz_count, A.sz_count, (AVGPU_MAX_GENOME + 1) * sizeof(int64_t), hipMemcpyDeviceToHost,
                          w->stream));
  if (want_rows && m > 0) {
    if (rows)
      HIPCHK(hipMemcpyAsync(rows, A.row[A.cur], (size_t)m * sizeof(avgpu_arbiter_row), hipMemcpyDeviceToHost,
                            w->stream));
    if (table)
      HIPCHK(hipMemcpyAsync(table, A.table, (size_t)m * sizeof(avgpu_genotype), hipMemcpyDeviceToHost, w->stream));
  }
  HIPCHK(hipStreamSynchronize(w->stream));
  return want_rows ? (int)m : 0;
}

int avgpu_set_arbiter(avgpu_world* w, int64_t n, const avgpu_arbiter_row* rows,
                      const avgpu_arbiter_summary* summary, const int64_t* sz_count) {
  if (!w || n < 0 || (n > 0 && !rows) || !summary)
    return fail(AVGPU_EINVAL, "avgpu_set_arbiter: NULL world, rows or summary, or negative n");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter on strip tiles");
  if (n > w->W.n) return fail(AVGPU_EINVAL, "avgpu_set_arbiter: more rows than cells");
  if (summary->next_id < 1) return fail(AVGPU_EINVAL, "avgpu_set_arbiter: next_id < 1");
  for (int64_t j = 0; j < n; j++)
    if (rows[j].genotype_key == 0 || (j > 0 && rows[j].genotype_key <= rows[j - 1].genotype_key))
      return fail(AVGPU_EINVAL, "avgpu_set_arbiter: row " + std::to_string(j) +
                                    ": keys must be non-zero and strictly ascending");
  for (int64_t j = 0; j < n; j++) {
    const avgpu_arbiter_row& r = rows[j];
    if (r.genome_length < 0 || r.genome_length > AVGPU_MAX_GENOME || r.name_no < 0 || r.num_units < 0 ||
        r.total_units < 0 || r.id < 1 || r.id >= summary->next_id)
      return fail(AVGPU_EINVAL, "avgpu_set_arbiter: row " + std::to_string(j) +
                                    ": genome_length outside 0..AVGPU_MAX_GENOME, a negative name_no, num_units "
                                    "or total_units, or an id outside 1..next_id-1");
  }
  if (sz_count)
    for (int q = 0; q <= AVGPU_MAX_GENOME; q++)
      if (sz_count[q] < 0) return fail(AVGPU_EINVAL, "avgpu_set_arbiter: negative sz_count");
  int rc = arbiter_alloc(w);
  if (rc < 0) return rc;
  HIPCHK(hipStreamSynchronize(w->stream));
  if ((rc = arbiter_reserve(w, std::max<int64_t>(n, 1), false)) < 0) return rc;
  ArbScratch& A = w->arb;
  std::vector<uint64_t> keys((size_t)n);
  int64_t dom = -1;
  const uint64_t dom_key = summary->dominant_row >= 0 ? summary->dominant_state.genotype_key : 0ull;
  int64_t thr = 0;
  for (int64_t j = 0; j < n; j++) {
    keys[j] = rows[j].genotype_key;
    if (keys[j] == dom_key) dom = j;
    thr += rows[j].threshold != 0;
  }
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(A.row[A.cur], rows, (size_t)n * sizeof(avgpu_arbiter_row), hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(A.key[A.cur], keys.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipMemsetAsync(A.table, 0, (size_t)n * sizeof(avgpu_genotype), w->stream));
  }
  ArbState st = {summary->next_id, summary->tot_genotypes, summary->tot_threshold, dom >= 0 ? dom_key : 0ull};
  HIPCHK(hipMemcpyAsync(A.state, &st, sizeof(st), hipMemcpyHostToDevice, w->stream));
  if (sz_count)
    HIPCHK(hipMemcpyAsync(A.sz_count, sz_count, (AVGPU_MAX_GENOME + 1) * sizeof(int64_t), hipMemcpyHostToDevice,
                          w->stream));
  else
    HIPCHK(hipMemsetAsync(A.sz_count, 0, (AVGPU_MAX_GENOME + 1) * sizeof(int64_t), w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  if (w->lin_on && (rc = lineage_clear(w)) < 0) return rc;   // (a resume fills it again: avgpu_set_lineage)
  w->arb_n = n;
  w->arb_last = *summary;
  w->arb_last.num_genotypes = n;
  w->arb_last.num_threshold = thr;
  w->arb_last.dominant_row = dom;
  if (dom >= 0) w->arb_last.dominant_state = rows[dom];
  else memset(&w->arb_last.dominant_state, 0, sizeof(avgpu_arbiter_row));
  if (dom < 0) memset(&w->arb_last.dominant, 0, sizeof(avgpu_genotype));
  return 0;
}

int avgpu_reset_arbiter(avgpu_world* w) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  avgpu_arbiter_summary s;
  arbiter_fresh_summary(&s);
  return avgpu_set_arbiter(w, 0, nullptr, &s, nullptr);
}

int avgpu_last_arbiter_ms(avgpu_world* w, double* device_ms, int64_t* bytes_copied) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (device_ms) *device_ms = w->arb_ms;
  if (bytes_copied) *bytes_copied = w->arb_bytes;
  return 0;
}

int avgpu_set_genotype_keys(avgpu_world* w, int64_t first, int64_t count, const uint64_t* keys) {
  if (!w || !keys || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  HIPCHK(hipMemcpyAsync(w->W.gkey + first, keys, count * sizeof(uint64_t), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int avgpu_enable_lineage(avgpu_world* w, int on, int64_t rows_hint, int64_t arena_hint) {
  if (!w || rows_hint < 0 || arena_hint < 0) return fail(AVGPU_EINVAL, "avgpu_enable_lineage: NULL world or a negative hint");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  HIPCHK(hipStreamSynchronize(w->stream));
  if (!on) {
    w->lin_on = false;
    w->lin_rows.reset(); w->lin_arena.reset(); w->lin_ctr.reset(); w->lin_idx.reset(); w->lin_asz.reset();
    w->lin_mark.reset(); w->lin_newcell.reset();
    w->lin = LinScratch{};
    return 0;
  }
  if (w->arb_ready && (w->arb_n != 0 || w->arb_last.next_id != 1))
    return fail(AVGPU_ESTATE, "avgpu_enable_lineage: the arbiter holds genotypes (avgpu_reset_arbiter first)");
  if (w->lin_on) return 0;
  int rc = w->lin_ctr.alloc(LIN_CTR_WORDS);
  if (rc < 0) return rc;
  w->lin = LinScratch{};
  w->lin.ctr = w->lin_ctr.get();
  w->lin_rows_hint = rows_hint > 0 ? rows_hint : 1024;
  w->lin_arena_hint = arena_hint > 0 ? arena_hint : 65536;
  for (Event& e : w->ev_lin)
    if ((rc = e.create()) < 0) return rc;
  w->lin_on = true;
  w->lin_ms = w->lin_prune_ms = 0.0;
  return lineage_clear(w);
}

int avgpu_get_lineage(avgpu_world* w, avgpu_lineage_row* rows, int64_t cap, uint8_t* genomes, int64_t genome_cap,
                      avgpu_lineage_summary* summary) {
  if (!w || cap < 0 || genome_cap < 0) return fail(AVGPU_EINVAL, "avgpu_get_lineage: NULL world or a negative cap");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  if (!w->lin_on) return fail(AVGPU_ESTATE, "avgpu_get_lineage: the store is off (avgpu_enable_lineage)");
  const LinScratch& L = w->lin;
  if ((rows && cap < L.n) || (genomes && genome_cap < L.arena_bytes))
    return fail(AVGPU_EINVAL, "avgpu_get_lineage: the store has " + std::to_string(L.n) + " rows and " +
                                  std::to_string(L.arena_bytes) + " arena bytes");
  if (summary) {
    const int rc = lineage_summary(w, summary);
    if (rc < 0) return rc;
  }
  if (rows && L.n > 0)
    HIPCHK(hipMemcpyAsync(rows, L.rows, (size_t)L.n * sizeof(avgpu_lineage_row), hipMemcpyDeviceToHost, w->stream));
  if (genomes && L.arena_bytes > 0)
    HIPCHK(hipMemcpyAsync(genomes, L.arena, (size_t)L.arena_bytes, hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return (int)L.n;
}

int avgpu_set_lineage(avgpu_world* w, int64_t n, const avgpu_lineage_row* rows, const uint8_t* genomes, int64_t bytes,
                      const avgpu_lineage_summary* summary) {
  if (!w || n < 0 || bytes < 0 || (n > 0 && !rows) || (bytes > 0 && !genomes) || !summary || (bytes & 15))
    return fail(AVGPU_EINVAL, "avgpu_set_lineage: NULL world, rows, genomes or summary, a negative count, or bytes "
                              "not a multiple of 16");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  if (!w->lin_on) return fail(AVGPU_ESTATE, "avgpu_set_lineage: the store is off (avgpu_enable_lineage)");
  if (summary->num_orphans < 0 || summary->num_unsequenced < 0)
    return fail(AVGPU_EINVAL, "avgpu_set_lineage: negative counters");
  auto find = [&](int64_t id) -> int64_t {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (rows[mid].id < id) lo = mid + 1; else hi = mid; }
    return (lo < n && rows[lo].id == id) ? lo : -1;
  };
  const int64_t next_id = w->arb_ready ? w->arb_last.next_id : 1;
  int64_t at = 0, active = 0;
  for (int64_t j = 0; j < n; j++) {
    const avgpu_lineage_row& r = rows[j];
    if (r.id < 1 || r.id >= next_id || (j > 0 && r.id <= rows[j - 1].id))
      return fail(AVGPU_EINVAL, "avgpu_set_lineage: row " + std::to_string(j) + ": ids must ascend strictly inside 1..next_id-1");
    if (r.parent_id >= r.id || r.parent_id < -1 || (r.parent_id > 0 && find(r.parent_id) < 0))
      return fail(AVGPU_EINVAL, "avgpu_set_lineage: row " + std::to_string(j) + ": parent_id must be below id and present, 0 or -1");
    if (r.genome_length < 0 || r.genome_length > AVGPU_MAX_GENOME || r.depth < 0)
      return fail(AVGPU_EINVAL, "avgpu_set_lineage: row " + std::to_string(j) + ": genome_length or depth out of range");
    if (r.seq_off != -1) {                         // in id order, 16-B aligned, back to back
      if (r.seq_off != at) return fail(AVGPU_EINVAL, "avgpu_set_lineage: row " + std::to_string(j) + ": seq_off out of order");
      at += ((int64_t)r.genome_length + 15) & ~15ll;
      if (at > bytes) return fail(AVGPU_EINVAL, "avgpu_set_lineage: row " + std::to_string(j) + ": genome past the arena");
    }
    active += r.update_deactivated < 0;
  }
  if (at != bytes) return fail(AVGPU_EINVAL, "avgpu_set_lineage: the genomes do not fill the arena");
  // every active arbiter id present as an active row, and no other active row
  const int64_t m = w->arb_ready ? w->arb_n : 0;
  std::vector<avgpu_arbiter_row> arows((size_t)m);
  if (m > 0) COPY_SYNC(w, arows.data(), w->arb.row[w->arb.cur], (size_t)m * sizeof(avgpu_arbiter_row), hipMemcpyDeviceToHost);
  for (int64_t j = 0; j < m; j++) {
    const int64_t q = find(arows[(size_t)j].id);
    if (q < 0 || rows[q].update_deactivated >= 0 || rows[q].genotype_key != arows[(size_t)j].genotype_key)
      return fail(AVGPU_EINVAL, "avgpu_set_lineage: active genotype " + std::to_string(arows[(size_t)j].id) + " has no active row");
  }
  if (active != m) return fail(AVGPU_EINVAL, "avgpu_set_lineage: an active row without an active genotype");
  HIPCHK(hipStreamSynchronize(w->stream));
  LinScratch& L = w->lin;
  const int64_t keep_n = L.n, keep_b = L.arena_bytes;
  L.n = 0; L.arena_bytes = 0;                      // (nothing to carry over when a buffer grows)
  int rc = lineage_reserve_rows(w, std::max<int64_t>(n, 1));
  if (rc == 0) rc = lineage_reserve_arena(w, std::max<int64_t>(bytes, 16));
  if (rc < 0) { L.n = keep_n; L.arena_bytes = keep_b; return rc; }
  if (n > 0) HIPCHK(hipMemcpyAsync(L.rows, rows, (size_t)n * sizeof(avgpu_lineage_row), hipMemcpyHostToDevice, w->stream));
  if (bytes > 0) HIPCHK(hipMemcpyAsync(L.arena, genomes, (size_t)bytes, hipMemcpyHostToDevice, w->stream));
  unsigned long long c[LIN_CTR_WORDS] = {};
  c[LIN_ORPHANS] = (unsigned long long)summary->num_orphans;
  c[LIN_UNSEQ] = (unsigned long long)summary->num_unsequenced;
  COPY_SYNC(w, L.ctr, c, sizeof(c), hipMemcpyHostToDevice);
  L.n = n;
  L.arena_bytes = bytes;
  w->lin_dropped = summary->dropped_last_prune;
  return 0;
}

int avgpu_prune_lineage(avgpu_world* w, avgpu_lineage_summary* summary) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  if (!w->lin_on) return fail(AVGPU_ESTATE, "avgpu_prune_lineage: the store is off (avgpu_enable_lineage)");
  LinScratch& L = w->lin;
  w->lin_dropped = 0;
  w->lin_prune_ms = 0.0;
  if (L.n > 0) {
    int rc = lineage_reserve_scratch(w, L.n);
    if (rc < 0) return rc;
    HIPCHK(hipEventRecord(w->ev_lin[2], w->stream));
    launch_lineage_mark(L, w->stream);
    HIPCHK(hipGetLastError());
    unsigned long long c[LIN_CTR_WORDS];
    COPY_SYNC(w, c, L.ctr, sizeof(c), hipMemcpyDeviceToHost);
    const int64_t kept = (int64_t)c[LIN_TOTAL_A], kbytes = (int64_t)c[LIN_TOTAL_B];
    if (kept < 0 || kept > L.n || kbytes < 0 || kbytes > L.arena_bytes)
      return fail(AVGPU_ESTATE, "lineage prune: totals outside the store");
    // compacted into new buffers of the store's capacities, then swapped in
    DevBuf<avgpu_lineage_row> nr(w->stream);
    DevBuf<uint8_t> na(w->stream);
    if ((rc = nr.alloc((size_t)L.cap)) < 0 || (rc = na.alloc((size_t)L.arena_cap)) < 0) return rc;
    launch_lineage_compact(L, nr.get(), L.cap, na.get(), L.arena_cap, w->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(w->ev_lin[3], w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    w->lin_rows = std::move(nr);
    w->lin_arena = std::move(na);
    L.rows = w->lin_rows.get();
    L.arena = w->lin_arena.get();
    w->lin_dropped = L.n - kept;
    L.n = kept;
    L.arena_bytes = kbytes;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, w->ev_lin[2], w->ev_lin[3]));
    w->lin_prune_ms = ms;
  }
  return summary ? lineage_summary(w, summary) : 0;
}

int avgpu_last_lineage_ms(avgpu_world* w, double* classify_ms, double* prune_ms) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (classify_ms) *classify_ms = w->lin_ms;
  if (prune_ms) *prune_ms = w->lin_prune_ms;
  return 0;
}

int avgpu_get_parent_keys(avgpu_world* w, int64_t first, int64_t count, uint64_t* out) {
  if (!w || !out || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  DevBuf<uint64_t> d(w->stream);                  // (a dead cell's row is stale: masked on the device)
  const int rc = d.alloc((size_t)count);
  if (rc < 0) return rc;
  launch_get_parent_keys(w->W, w->stream, first, count, d.get());
  HIPCHK(hipGetLastError());
  COPY_SYNC(w, out, d.get(), (size_t)count * sizeof(uint64_t), hipMemcpyDeviceToHost);
  return 0;
}

int avgpu_set_parent_keys(avgpu_world* w, int64_t first, int64_t count, const uint64_t* keys) {
  if (!w || !keys || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  COPY_SYNC(w, w->W.pkey + first, keys, (size_t)count * sizeof(uint64_t), hipMemcpyHostToDevice);
  return 0;
}

}  // extern "C"
