// capi_systematics.hip -- the census, the genotype table, the genotype arbiter,
// genotype keys.  (The lineage store beside the arbiter: capi_lineage.hip.)
#include "host.h"

using namespace avh;

extern "C" {

int avgpu_get_census(avgpu_world* w, int64_t first, int64_t count, avgpu_census* out) {
  if (!w || !out || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  DevBuf<avgpu_census> d(w->stream);
  RCCHK(d.alloc(count));
  launch_get_census(w->W, w->stream, first, count, d.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d.get(), count * sizeof(avgpu_census), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

// the grouping's scratch: 24 B per cell for the two (key, cell) buffers of
// the sort, the per-tile histograms and segment tiles on top (under 1 B per cell)
static int genotypes_alloc(avgpu_world* w) {
  if (w->gt.ready) return 0;
  GtScratch& S = w->gt.view;
  S.n = w->W.n;
  S.nblk = (S.n + GT_SORT_TILE - 1) / GT_SORT_TILE;
  S.ntile = (S.n + GT_SEG_TILE - 1) / GT_SEG_TILE;
  for (int k = 0; k < 2; k++) { RCCHK(w->alloc(&S.key[k], (size_t)S.n)); RCCHK(w->alloc(&S.cell[k], (size_t)S.n)); }
  RCCHK(w->alloc(&S.hist, (size_t)256 * S.nblk));
  RCCHK(w->alloc(&S.dtot, 256));
  RCCHK(w->alloc(&S.tile_agg, (size_t)S.ntile));
  RCCHK(w->alloc(&S.carry, (size_t)S.ntile));
  RCCHK(w->alloc(&S.tile_flag, (size_t)S.ntile));
  RCCHK(w->alloc(&S.tile_tails, (size_t)S.ntile));
  RCCHK(w->alloc(&S.row_off, (size_t)S.ntile));
  RCCHK(w->alloc(&S.totals, 1));
  RCCHK(w->gt.t_group.create());
  RCCHK(w->gt.t_rows.create());
  w->gt.ready = true;
  return 0;
}

int avgpu_get_genotypes(avgpu_world* w, avgpu_genotype* out, int64_t cap, avgpu_genotype_totals* totals) {
  if (!w || cap < 0) return fail(AVGPU_EINVAL, "avgpu_get_genotypes: NULL world or negative cap");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype table on strip tiles");
  if (w->W.n >= (1ll << 31) - GT_SORT_TILE) return fail(AVGPU_EUNSUPPORTED, "genotype table of 2^31 cells or more");
  RCCHK(genotypes_alloc(w));
  GenotypeTable& G = w->gt;
  const GtScratch& S = G.view;
  HIPCHK(hipMemsetAsync(S.totals, 0, sizeof(avgpu_genotype_totals), w->stream));
  RCCHK(G.t_group.start(w->stream));
  launch_genotype_group(w->W, S, w->stream);
  HIPCHK(hipGetLastError());
  RCCHK(G.t_group.stop(w->stream));
  avgpu_genotype_totals t;
  COPY_SYNC(w, &t, S.totals, sizeof(t), hipMemcpyDeviceToHost);
  RCCHK(G.t_group.elapsed(&G.ms));
  G.bytes = sizeof(t);
  if (totals) *totals = t;
  if (!out || cap == 0) return 0;
  if (cap < t.num_genotypes)
    return fail(AVGPU_EINVAL, "avgpu_get_genotypes: cap " + std::to_string(cap) + " rows, the table has " +
                                  std::to_string(t.num_genotypes));
  if (t.num_genotypes == 0) return 0;
  RCCHK(G.rows.reserve(w->stream, t.num_genotypes, {1024, S.n}));
  RCCHK(G.t_rows.start(w->stream));
  launch_genotype_rows(w->W, S, G.rows.get(), w->stream);
  HIPCHK(hipGetLastError());
  RCCHK(G.t_rows.stop(w->stream));
  COPY_SYNC(w, out, G.rows.get(), (size_t)t.num_genotypes * sizeof(avgpu_genotype), hipMemcpyDeviceToHost);
  double rows_ms = 0.0;
  RCCHK(G.t_rows.elapsed(&rows_ms));
  G.ms += rows_ms;
  G.bytes += t.num_genotypes * (int64_t)sizeof(avgpu_genotype);
  return (int)t.num_genotypes;
}

int avgpu_last_genotypes_ms(avgpu_world* w, double* device_ms, int64_t* bytes_copied) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (device_ms) *device_ms = w->gt.ms;
  if (bytes_copied) *bytes_copied = w->gt.bytes;
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
  if (w->arb.ready) return 0;
  ArbScratch& A = w->arb.view;
  RCCHK(w->alloc(&A.state, 1));
  RCCHK(w->alloc(&A.work, 1));
  RCCHK(w->alloc(&A.sz_count, AVGPU_MAX_GENOME + 1));
  if (w->arb.sum.alloc(1, hipHostMallocMapped | hipHostMallocCoherent) < 0 ||
      hipHostGetDevicePointer((void**)&A.d_sum, w->arb.sum.get(), 0) != hipSuccess)
    return fail(AVGPU_ENOMEM, "pinned arbiter summary");
  A.h_sum = w->arb.sum.get();
  memset(A.h_sum, 0, sizeof(avgpu_arbiter_summary));
  ArbState st = {1, 0, 0, 0ull};
  COPY_SYNC(w, A.state, &st, sizeof(st), hipMemcpyHostToDevice);
  RCCHK(w->arb.t_group.create());
  RCCHK(w->arb.t_classify.create());
  arbiter_fresh_summary(&w->arb.last);
  w->arb.n = 0;
  w->arb.ready = true;
  return 0;
}

// the view's rows, keys, table and capacity from the owners (the rest: arbiter_alloc)
static void arbiter_view(Arbiter& S) {
  ArbScratch& A = S.view;
  for (int k = 0; k < 2; k++) { A.row[k] = S.row[k].get(); A.key[k] = S.key[k].get(); }
  A.table = S.table.get();
  A.cap = S.table.capacity();
}

// room for `rows` rows in the five buffers, all of them or none (DevBuf::reserve's
// steps by hand); keep: the current state survives
static int arbiter_reserve(avgpu_world* w, int64_t rows, bool keep) {
  Arbiter& S = w->arb;
  const ArbScratch& A = S.view;
  if (rows <= S.table.capacity()) return 0;
  const size_t want = (size_t)grown_capacity(rows, {1024, std::max<int64_t>(w->W.n, 1)});
  DevBuf<avgpu_arbiter_row> row[2] = {DevBuf<avgpu_arbiter_row>(w->stream), DevBuf<avgpu_arbiter_row>(w->stream)};
  DevBuf<uint64_t> key[2] = {DevBuf<uint64_t>(w->stream), DevBuf<uint64_t>(w->stream)};
  DevBuf<avgpu_genotype> table(w->stream);
  RCCHK(table.alloc(want));
  for (int k = 0; k < 2; k++) { RCCHK(row[k].alloc(want)); RCCHK(key[k].alloc(want)); }
  if (keep && S.n > 0) {
    const size_t n = (size_t)S.n;
    auto copy = [&](void* d, const void* s, size_t b) { return hipMemcpyAsync(d, s, b, hipMemcpyDeviceToDevice, w->stream); };
    hipError_t e = copy(row[A.cur].get(), A.row[A.cur], n * sizeof(avgpu_arbiter_row));
    if (e == hipSuccess) e = copy(key[A.cur].get(), A.key[A.cur], n * sizeof(uint64_t));
    if (e == hipSuccess) e = copy(table.get(), A.table, n * sizeof(avgpu_genotype));
    if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
    if (e != hipSuccess) return fail(AVGPU_ENOMEM, std::string("arbiter rows: ") + hipGetErrorString(e));
  }
  for (int k = 0; k < 2; k++) { S.row[k] = std::move(row[k]); S.key[k] = std::move(key[k]); }
  S.table = std::move(table);
  arbiter_view(S);
  return 0;
}

int avgpu_classify_genotypes(avgpu_world* w, int64_t update, int32_t threshold, avgpu_arbiter_summary* out) {
  if (!w || !out || threshold < 1)
    return fail(AVGPU_EINVAL, "avgpu_classify_genotypes: NULL world, NULL out or threshold < 1");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter on strip tiles");
  if (w->W.n >= (1ll << 31) - GT_SORT_TILE) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter of 2^31 cells or more");
  RCCHK(genotypes_alloc(w));
  RCCHK(arbiter_alloc(w));
  const GtScratch& S = w->gt.view;
  Arbiter& R = w->arb;
  ArbScratch& A = R.view;
  const int64_t lin_prev = R.n, lin_id0 = R.last.next_id;
  // the first part: the grouping; its totals are the summary's first fields
  HIPCHK(hipMemsetAsync(S.totals, 0, sizeof(avgpu_genotype_totals), w->stream));
  RCCHK(R.t_group.start(w->stream));
  launch_genotype_group(w->W, S, w->stream);
  launch_arbiter_begin(A, S, update, w->stream);
  HIPCHK(hipGetLastError());
  RCCHK(R.t_group.stop(w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  const int64_t m = __atomic_load_n(&A.h_sum->num_genotypes, __ATOMIC_ACQUIRE);
  if (m < 0 || m > S.n) return fail(AVGPU_ESTATE, "genotype arbiter: row count outside the world");
  RCCHK(w->gt.rows.reserve(w->stream, m, {1024, S.n}));
  RCCHK(arbiter_reserve(w, std::max<int64_t>(m, 1), true));
  // every id of the new state is below next_id + m
  int id_bits = 1;
  while (id_bits < 50 && ((R.last.next_id + m) >> id_bits) != 0) id_bits++;
  if (((R.last.next_id + m) >> id_bits) != 0) return fail(AVGPU_EUNSUPPORTED, "genotype ids of 2^50 or more");
  RCCHK(R.t_classify.start(w->stream));
  if (m > 0) {
    launch_genotype_rows(w->W, S, w->gt.rows.get(), w->stream);
    HIPCHK(hipMemcpyAsync(A.table, w->gt.rows.get(), (size_t)m * sizeof(avgpu_genotype), hipMemcpyDeviceToDevice,
                          w->stream));
  }
  launch_arbiter_classify(A, S, A.table, m, R.n, update, threshold, id_bits, w->stream);
  HIPCHK(hipGetLastError());
  RCCHK(R.t_classify.stop(w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  A.cur ^= 1;
  R.n = m;
  memcpy(&R.last, A.h_sum, sizeof(avgpu_arbiter_summary));
  *out = R.last;
  double ms0 = 0.0, ms1 = 0.0;
  RCCHK(R.t_group.elapsed(&ms0));
  RCCHK(R.t_classify.elapsed(&ms1));
  R.ms = ms0 + ms1;
  R.bytes = sizeof(avgpu_arbiter_summary);
  if (w->lin.on) return lineage_step(w, lin_prev, lin_id0, m, update);
  return 0;
}

int avgpu_get_arbiter(avgpu_world* w, avgpu_arbiter_row* rows, avgpu_genotype* table, int64_t cap,
                      avgpu_arbiter_summary* summary, int64_t* sz_count) {
  if (!w || cap < 0) return fail(AVGPU_EINVAL, "avgpu_get_arbiter: NULL world or negative cap");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genotype arbiter on strip tiles");
  if (!w->arb.ready) {                          // never classified or set: a new world's state, nothing allocated
    if (summary) arbiter_fresh_summary(summary);
    if (sz_count) memset(sz_count, 0, (AVGPU_MAX_GENOME + 1) * sizeof(int64_t));
    return 0;
  }
  const ArbScratch& A = w->arb.view;
  const int64_t m = w->arb.n;
  const bool want_rows = (rows || table) && cap > 0;
  if (want_rows && cap < m)
    return fail(AVGPU_EINVAL, "avgpu_get_arbiter: cap " + std::to_string(cap) + " rows, the arbiter has " +
                                  std::to_string(m));
  if (summary) *summary = w->arb.last;
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
  RCCHK(arbiter_alloc(w));
  HIPCHK(hipStreamSynchronize(w->stream));
  RCCHK(arbiter_reserve(w, std::max<int64_t>(n, 1), false));
  ArbScratch& A = w->arb.view;
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
  if (w->lin.on) RCCHK(lineage_clear(w));                   // (a resume fills it again: avgpu_set_lineage)
  w->arb.n = n;
  w->arb.last = *summary;
  w->arb.last.num_genotypes = n;
  w->arb.last.num_threshold = thr;
  w->arb.last.dominant_row = dom;
  if (dom >= 0) w->arb.last.dominant_state = rows[dom];
  else memset(&w->arb.last.dominant_state, 0, sizeof(avgpu_arbiter_row));
  if (dom < 0) memset(&w->arb.last.dominant, 0, sizeof(avgpu_genotype));
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
  if (device_ms) *device_ms = w->arb.ms;
  if (bytes_copied) *bytes_copied = w->arb.bytes;
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
