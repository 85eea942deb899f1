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

}  // extern "C"
