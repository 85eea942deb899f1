// capi_lineage.hip -- the lineage store beside the arbiter (lineage.hip;
// DESIGN.md 10.6), parent keys.
#include "host.h"

using namespace avh;

namespace {

// the view's pointers and capacities from the owners (after any reserve or swap)
void lineage_view(Lineage& S) {
  LinScratch& L = S.view;
  L.rows = S.rows.get(); L.cap = S.rows.capacity();
  L.arena = S.arena.get(); L.arena_cap = S.arena.capacity();
  L.ctr = S.ctr.get();
  L.idx = S.idx.get(); L.asz = S.asz.get(); L.mark = S.mark.get(); L.newcell = S.newcell.get();
  L.scap = S.idx.capacity();
}

// the scratch rows of a classification (its new rows) or a prune (every row):
// four buffers, all of them or none
int lineage_reserve_scratch(avgpu_world* w, int64_t n) {
  Lineage& S = w->lin;
  if (n <= S.idx.capacity()) return 0;
  const size_t want = (size_t)grown_capacity(n, {64});
  DevBuf<int64_t> idx(w->stream), asz(w->stream);
  DevBuf<uint32_t> mark(w->stream);
  DevBuf<int32_t> newcell(w->stream);
  RCCHK(idx.alloc(want)); RCCHK(asz.alloc(want));
  RCCHK(mark.alloc(want)); RCCHK(newcell.alloc(want));
  S.idx = std::move(idx); S.asz = std::move(asz); S.mark = std::move(mark); S.newcell = std::move(newcell);
  lineage_view(S);
  return 0;
}

int lineage_summary(avgpu_world* w, avgpu_lineage_summary* s) {
  LinScratch& L = w->lin.view;
  unsigned long long c[LIN_CTR_WORDS];
  HIPCHK(hipMemsetAsync(L.ctr + LIN_MAXDEPTH, 0, sizeof(unsigned long long), w->stream));
  launch_lineage_max_depth(L, w->stream);
  HIPCHK(hipGetLastError());
  COPY_SYNC(w, c, L.ctr, sizeof(c), hipMemcpyDeviceToHost);
  memset(s, 0, sizeof(*s));
  s->rows = L.n;
  s->active_rows = w->arb.ready ? w->arb.n : 0;
  s->arena_bytes = L.arena_bytes;
  s->num_orphans = (int64_t)c[LIN_ORPHANS];
  s->num_unsequenced = (int64_t)c[LIN_UNSEQ];
  s->max_depth = (int64_t)c[LIN_MAXDEPTH];
  s->dropped_last_prune = w->lin.dropped;
  return 0;
}

}  // namespace

int avh::lineage_clear(avgpu_world* w) {
  LinScratch& L = w->lin.view;
  L.n = 0;
  L.arena_bytes = 0;
  w->lin.dropped = 0;
  if (L.ctr) SET_SYNC(w, L.ctr, 0, LIN_CTR_WORDS * sizeof(unsigned long long));
  return 0;
}

// (the stream is idle; the arbiter's buffers are swapped): n_prev rows and
// next id id0 before, m rows after
int avh::lineage_step(avgpu_world* w, int64_t n_prev, int64_t id0, int64_t m, int64_t update) {
  Lineage& S = w->lin;
  LinScratch& L = S.view;
  const int64_t n_new = w->arb.last.next_id - id0;
  if (n_new < 0 || n_new > m) return fail(AVGPU_ESTATE, "lineage: new ids outside the classification");
  RCCHK(S.rows.reserve(w->stream, L.n + n_new, {S.rows_hint}, L.n));
  lineage_view(S);
  RCCHK(lineage_reserve_scratch(w, n_new));
  RCCHK(S.t_classify.start(w->stream));
  launch_lineage_classify(L, w->arb.view, w->W, n_prev, m, id0, n_new, update, w->stream);
  HIPCHK(hipGetLastError());
  unsigned long long total = (unsigned long long)L.arena_bytes;
  if (n_new > 0) {
    COPY_SYNC(w, &total, L.ctr + LIN_TOTAL_A, sizeof(total), hipMemcpyDeviceToHost);
    if ((int64_t)total < L.arena_bytes) return fail(AVGPU_ESTATE, "lineage: arena total went down");
    RCCHK(S.arena.reserve(w->stream, (int64_t)total, {S.arena_hint, INT64_MAX, 16}, L.arena_bytes));
    lineage_view(S);
    launch_lineage_copy(L, w->W, n_new, w->stream);
    HIPCHK(hipGetLastError());
  }
  RCCHK(S.t_classify.stop(w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  L.n += n_new;
  L.arena_bytes = (int64_t)total;
  return S.t_classify.elapsed(&S.classify_ms);
}

extern "C" {

int avgpu_enable_lineage(avgpu_world* w, int on, int64_t rows_hint, int64_t arena_hint) {
  if (!w || rows_hint < 0 || arena_hint < 0) return fail(AVGPU_EINVAL, "avgpu_enable_lineage: NULL world or a negative hint");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  HIPCHK(hipStreamSynchronize(w->stream));
  Lineage& S = w->lin;
  if (!on) {
    S.on = false;
    S.rows.reset(); S.arena.reset(); S.ctr.reset(); S.idx.reset(); S.asz.reset(); S.mark.reset(); S.newcell.reset();
    S.view.n = S.view.arena_bytes = 0;
    lineage_view(S);
    return 0;
  }
  if (w->arb.ready && (w->arb.n != 0 || w->arb.last.next_id != 1))
    return fail(AVGPU_ESTATE, "avgpu_enable_lineage: the arbiter holds genotypes (avgpu_reset_arbiter first)");
  if (S.on) return 0;
  RCCHK(S.ctr.alloc(LIN_CTR_WORDS));
  lineage_view(S);
  S.rows_hint = rows_hint > 0 ? rows_hint : 1024;      // the buffers' floors: at least 1 row, 16 B
  S.arena_hint = arena_hint > 0 ? std::max<int64_t>(arena_hint, 16) : 65536;
  RCCHK(S.t_classify.create());
  RCCHK(S.t_prune.create());
  S.on = true;
  S.classify_ms = S.prune_ms = 0.0;
  return lineage_clear(w);
}

int avgpu_get_lineage(avgpu_world* w, avgpu_lineage_row* rows, int64_t cap, uint8_t* genomes, int64_t genome_cap,
                      avgpu_lineage_summary* summary) {
  if (!w || cap < 0 || genome_cap < 0) return fail(AVGPU_EINVAL, "avgpu_get_lineage: NULL world or a negative cap");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  if (!w->lin.on) return fail(AVGPU_ESTATE, "avgpu_get_lineage: the store is off (avgpu_enable_lineage)");
  const LinScratch& L = w->lin.view;
  if ((rows && cap < L.n) || (genomes && genome_cap < L.arena_bytes))
    return fail(AVGPU_EINVAL, "avgpu_get_lineage: the store has " + std::to_string(L.n) + " rows and " +
                                  std::to_string(L.arena_bytes) + " arena bytes");
  if (summary) RCCHK(lineage_summary(w, summary));
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
  if (!w->lin.on) return fail(AVGPU_ESTATE, "avgpu_set_lineage: the store is off (avgpu_enable_lineage)");
  if (summary->num_orphans < 0 || summary->num_unsequenced < 0)
    return fail(AVGPU_EINVAL, "avgpu_set_lineage: negative counters");
  auto find = [&](int64_t id) -> int64_t {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (rows[mid].id < id) lo = mid + 1; else hi = mid; }
    return (lo < n && rows[lo].id == id) ? lo : -1;
  };
  const int64_t next_id = w->arb.ready ? w->arb.last.next_id : 1;
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
  const int64_t m = w->arb.ready ? w->arb.n : 0;
  std::vector<avgpu_arbiter_row> arows((size_t)m);
  if (m > 0)
    COPY_SYNC(w, arows.data(), w->arb.view.row[w->arb.view.cur], (size_t)m * sizeof(avgpu_arbiter_row), hipMemcpyDeviceToHost);
  for (int64_t j = 0; j < m; j++) {
    const int64_t q = find(arows[(size_t)j].id);
    if (q < 0 || rows[q].update_deactivated >= 0 || rows[q].genotype_key != arows[(size_t)j].genotype_key)
      return fail(AVGPU_EINVAL, "avgpu_set_lineage: active genotype " + std::to_string(arows[(size_t)j].id) + " has no active row");
  }
  if (active != m) return fail(AVGPU_EINVAL, "avgpu_set_lineage: an active row without an active genotype");
  HIPCHK(hipStreamSynchronize(w->stream));
  Lineage& S = w->lin;
  LinScratch& L = S.view;
  // (nothing to carry over when a buffer grows: the store is replaced)
  int rc = S.rows.reserve(w->stream, std::max<int64_t>(n, 1), {S.rows_hint});
  if (rc == 0) rc = S.arena.reserve(w->stream, std::max<int64_t>(bytes, 16), {S.arena_hint, INT64_MAX, 16});
  lineage_view(S);
  if (rc < 0) return rc;
  if (n > 0) HIPCHK(hipMemcpyAsync(L.rows, rows, (size_t)n * sizeof(avgpu_lineage_row), hipMemcpyHostToDevice, w->stream));
  if (bytes > 0) HIPCHK(hipMemcpyAsync(L.arena, genomes, (size_t)bytes, hipMemcpyHostToDevice, w->stream));
  unsigned long long c[LIN_CTR_WORDS] = {};
  c[LIN_ORPHANS] = (unsigned long long)summary->num_orphans;
  c[LIN_UNSEQ] = (unsigned long long)summary->num_unsequenced;
  COPY_SYNC(w, L.ctr, c, sizeof(c), hipMemcpyHostToDevice);
  L.n = n;
  L.arena_bytes = bytes;
  S.dropped = summary->dropped_last_prune;
  return 0;
}

int avgpu_prune_lineage(avgpu_world* w, avgpu_lineage_summary* summary) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "lineage store on strip tiles");
  if (!w->lin.on) return fail(AVGPU_ESTATE, "avgpu_prune_lineage: the store is off (avgpu_enable_lineage)");
  Lineage& S = w->lin;
  LinScratch& L = S.view;
  S.dropped = 0;
  S.prune_ms = 0.0;
  if (L.n > 0) {
    RCCHK(lineage_reserve_scratch(w, L.n));
    RCCHK(S.t_prune.start(w->stream));
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
    RCCHK(nr.alloc((size_t)L.cap));
    RCCHK(na.alloc((size_t)L.arena_cap));
    launch_lineage_compact(L, nr.get(), L.cap, na.get(), L.arena_cap, w->stream);
    HIPCHK(hipGetLastError());
    RCCHK(S.t_prune.stop(w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    S.rows = std::move(nr);
    S.arena = std::move(na);
    lineage_view(S);
    S.dropped = L.n - kept;
    L.n = kept;
    L.arena_bytes = kbytes;
    RCCHK(S.t_prune.elapsed(&S.prune_ms));
  }
  return summary ? lineage_summary(w, summary) : 0;
}

int avgpu_last_lineage_ms(avgpu_world* w, double* classify_ms, double* prune_ms) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (classify_ms) *classify_ms = w->lin.classify_ms;
  if (prune_ms) *prune_ms = w->lin.prune_ms;
  return 0;
}

int avgpu_get_parent_keys(avgpu_world* w, int64_t first, int64_t count, uint64_t* out) {
  if (!w || !out || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  DevBuf<uint64_t> d(w->stream);                  // (a dead cell's row is stale: masked on the device)
  RCCHK(d.alloc((size_t)count));
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
