// capi_serial.hip -- the serial world: its state, its two streams, the reaper queue.
#include "host.h"

using namespace avh;

namespace avh {

// the serial world's reaper queue (W.reaper: a ring of reaper_cap cells,
// positions [reaper_ix[0], reaper_ix[1]) from the rear), rear first
int reaper_read(avgpu_world* w, std::vector<int32_t>& q) {
  const DevWorld& W = w->W;
  int64_t ix[2];
  COPY_SYNC(w, ix, W.reaper_ix, sizeof(ix), hipMemcpyDeviceToHost);
  std::vector<int32_t> ring((size_t)W.reaper_cap);
  COPY_SYNC(w, ring.data(), W.reaper, ring.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (ix[1] < ix[0] || ix[1] - ix[0] > W.reaper_cap) return fail(AVGPU_ESTATE, "reaper queue indices");
  q.clear();
  for (int64_t p = ix[0]; p < ix[1]; p++) q.push_back(ring[(size_t)(p % W.reaper_cap)]);
  return 0;
}
int reaper_write(avgpu_world* w, const std::vector<int32_t>& q) {
  const DevWorld& W = w->W;
  if ((int64_t)q.size() > W.reaper_cap) return fail(AVGPU_EUNSUPPORTED, "reaper queue longer than 2n + 64");
  std::vector<int32_t> ring((size_t)W.reaper_cap, 0);
  std::copy(q.begin(), q.end(), ring.begin());
  const int64_t ix[2] = {W.reaper_cap, W.reaper_cap + (int64_t)q.size()};   // position cap + k = slot k
  COPY_SYNC(w, W.reaper, ring.data(), ring.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  COPY_SYNC(w, W.reaper_ix, ix, sizeof(ix), hipMemcpyHostToDevice);
  return 0;
}

// the queue as the reference has it after Setup and the injections of the
// living cells (oracle reaper_setup): cells 0..N-1 pushed, then every living
// cell in ascending order
int reaper_build(avgpu_world* w) {
  const DevWorld& W = w->W;
  std::vector<uint32_t> ctl((size_t)W.n);
  COPY_SYNC(w, ctl.data(), W.ctl, (size_t)W.n * sizeof(uint32_t), hipMemcpyDeviceToHost);
  std::vector<int32_t> q;
  for (int64_t c = 0; c < W.n; c++) q.push_back((int32_t)c);
  for (int64_t c = 0; c < W.n; c++) if (ctl[(size_t)c] & CTL_ALIVE) q.push_back((int32_t)c);
  w->reaper_rebuild = false;
  return reaper_write(w, q);
}

}  // namespace avh

extern "C" {

// the serial world's state, allocated on first use: merit sum tree,
// speculative credits, connection-list facings, the scheduler's and the
// context's counter streams (keyed by the seed, as the oracle's)
static int serial_alloc(avgpu_world* w) {
  DevWorld& W = w->W;
  if (W.stree) return 0;
  int rc;
  int64_t size = 1;
  while (size < W.n) size <<= 1;
  W.stree_size = size;
  if ((rc = w->alloc(&W.stree, (size_t)(2 * size))) < 0) return rc;
  if ((rc = w->alloc(&W.spec, (size_t)W.n)) < 0) return rc;
  if ((rc = w->alloc(&W.face, (size_t)W.n)) < 0) return rc;
  if ((rc = w->alloc(&W.grng, 3)) < 0) return rc;
  if ((rc = w->alloc(&W.sctx, 3)) < 0) return rc;
  if (w->cfg.birth_method == 5) {
    // the reaper queue (oracle reaper_setup): Setup's cells 0..N-1, then the
    // living cells in ascending order, each pushed at the front
    const int64_t cap = 2 * W.n + 64;
    if ((rc = w->alloc(&W.reaper, (size_t)cap)) < 0) return rc;
    if ((rc = w->alloc(&W.reaper_ix, 2)) < 0) return rc;
    W.reaper_cap = cap;
    if ((rc = reaper_build(w)) < 0) return rc;
  }
  uint32_t g[3] = {0, 0, 0}, x[3] = {0, 0, 0};
  const uint64_t seed = (uint64_t)w->cfg.seed;
  derive_key((uint32_t)seed, (uint32_t)(seed >> 32), 0x5CEDu, 0xC0FFEEu, g[0], g[1]);
  derive_key((uint32_t)seed, (uint32_t)(seed >> 32), 0xC7C7u, 0x5EED5u, x[0], x[1]);
  HIPCHK(hipMemcpyAsync(W.grng, g, sizeof(g), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(W.sctx, x, sizeof(x), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int avgpu_set_serial_streams(avgpu_world* w, const double* sched, int64_t n_sched, const double* ctx,
                             int64_t n_ctx) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if ((sched && n_sched <= 0) || (ctx && n_ctx <= 0)) return fail(AVGPU_EINVAL, "empty stream");
  int rc = serial_alloc(w);
  if (rc < 0) return rc;
  DevWorld& W = w->W;
  HIPCHK(hipStreamSynchronize(w->stream));   // no queued serial update still reads them
  w->srec_buf[0].reset(); w->srec_buf[1].reset();
  W.srec_sched = nullptr; W.srec_sched_n = 0; W.srec_ctx = nullptr; W.srec_ctx_n = 0;
  if (sched) {
    if ((rc = w->srec_buf[0].alloc((size_t)n_sched)) < 0) return rc;
    COPY_SYNC(w, w->srec_buf[0].get(), sched, (size_t)n_sched * sizeof(double), hipMemcpyHostToDevice);
    W.srec_sched = w->srec_buf[0].get(); W.srec_sched_n = n_sched;
  }
  if (ctx) {
    if ((rc = w->srec_buf[1].alloc((size_t)n_ctx)) < 0) return rc;
    COPY_SYNC(w, w->srec_buf[1].get(), ctx, (size_t)n_ctx * sizeof(double), hipMemcpyHostToDevice);
    W.srec_ctx = w->srec_buf[1].get(); W.srec_ctx_n = n_ctx;
  }
  // both positions restart at 0 (counter streams: their counters)
  HIPCHK(hipMemsetAsync(W.grng + 2, 0, 4, w->stream));
  HIPCHK(hipMemsetAsync(W.sctx + 2, 0, 4, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int avgpu_get_serial_state(avgpu_world* w, avgpu_serial_state* st, int32_t* spec, uint8_t* face,
                           int32_t* soup_perm, int32_t* reaper, int64_t reaper_cap) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  const DevWorld& W = w->W;
  const int64_t n = W.n;
  const bool started = W.stree != nullptr;     // serial_alloc ran (a serial update, or a set state)
  uint32_t g[3] = {0, 0, 0}, x[3] = {0, 0, 0};
  if (started) {
    COPY_SYNC(w, g, W.grng, sizeof(g), hipMemcpyDeviceToHost);
    COPY_SYNC(w, x, W.sctx, sizeof(x), hipMemcpyDeviceToHost);
  }
  std::vector<int32_t> q;
  const bool have_q = W.reaper && !w->reaper_rebuild;
  if (have_q) {
    int rc = reaper_read(w, q);
    if (rc < 0) return rc;
  }
  if (st) {
    memset(st, 0, sizeof(*st));
    st->sched_pos = g[2];
    st->ctx_pos = x[2];
    st->reaper_len = have_q ? (int64_t)q.size() : -1;
    st->started = started ? 1 : 0;
  }
  if (spec) {
    std::vector<uint32_t> ctl((size_t)n);
    COPY_SYNC(w, ctl.data(), W.ctl, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (started) COPY_SYNC(w, spec, W.spec, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    for (int64_t c = 0; c < n; c++)
      spec[c] = (started ? (spec[c] & 0xFFFF) : 0) | ((ctl[(size_t)c] & CTL_SPECDIE) ? 1 << 16 : 0);
  }
  if (face) {
    if (started) COPY_SYNC(w, face, W.face, (size_t)n, hipMemcpyDeviceToHost);
    else memset(face, 0, (size_t)n);
  }
  if (soup_perm) {
    if (W.soup_perm) COPY_SYNC(w, soup_perm, W.soup_perm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    else for (int64_t c = 0; c < n; c++) soup_perm[c] = (int32_t)c;
  }
  if (reaper && !q.empty()) {
    if (reaper_cap < (int64_t)q.size()) return fail(AVGPU_EINVAL, "reaper buffer too small");
    std::copy(q.begin(), q.end(), reaper);
  }
  return 0;
}

int avgpu_set_serial_state(avgpu_world* w, const avgpu_serial_state* st, const int32_t* spec, const uint8_t* face,
                           const int32_t* soup_perm, const int32_t* reaper) {
  if (!w || !st) return fail(AVGPU_EINVAL, "serial state");
  if (!st->started) return 0;
  DevWorld& W = w->W;
  const int64_t n = W.n, len = st->reaper_len;
  if (soup_perm) {
    std::vector<char> seen((size_t)n, 0);
    for (int64_t c = 0; c < n; c++) {
      if (soup_perm[c] < 0 || soup_perm[c] >= n || seen[(size_t)soup_perm[c]])
        return fail(AVGPU_EINVAL, "soup_perm is not a permutation of the cells");
      seen[(size_t)soup_perm[c]] = 1;
    }
  }
  if (len > 2 * n + 64) return fail(AVGPU_EINVAL, "reaper queue longer than 2n + 64");
  if (len > 0 && !reaper) return fail(AVGPU_EINVAL, "reaper queue");
  for (int64_t k = 0; k < len; k++)
    if (reaper[k] < 0 || reaper[k] >= n) return fail(AVGPU_EINVAL, "reaper queue cell out of range");
  int rc = serial_alloc(w);
  if (rc < 0) return rc;
  const uint32_t gp = (uint32_t)st->sched_pos, xp = (uint32_t)st->ctx_pos;
  COPY_SYNC(w, W.grng + 2, &gp, 4, hipMemcpyHostToDevice);
  COPY_SYNC(w, W.sctx + 2, &xp, 4, hipMemcpyHostToDevice);
  if (spec) {
    std::vector<int32_t> cr((size_t)n);
    std::vector<uint32_t> ctl((size_t)n);
    COPY_SYNC(w, ctl.data(), W.ctl, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    for (int64_t c = 0; c < n; c++) {
      cr[(size_t)c] = spec[c] & 0xFFFF;
      ctl[(size_t)c] = (ctl[(size_t)c] & ~CTL_SPECDIE) | (((spec[c] >> 16) & 1) ? CTL_SPECDIE : 0u);
    }
    COPY_SYNC(w, W.spec, cr.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    COPY_SYNC(w, W.ctl, ctl.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  if (face) COPY_SYNC(w, W.face, face, (size_t)n, hipMemcpyHostToDevice);
  if (soup_perm && W.soup_perm) COPY_SYNC(w, W.soup_perm, soup_perm, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
  if (W.reaper) {
    if (len < 0) {
      w->reaper_rebuild = true;                      // built again at the next serial update
    } else {
      w->reaper_rebuild = false;
      if ((rc = reaper_write(w, std::vector<int32_t>(reaper, reaper + len))) < 0) return rc;
    }
  }
  return 0;
}

int avgpu_run_serial_updates(avgpu_world* w, int n, avgpu_update_stats* last) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (n < 0) return fail(AVGPU_EINVAL, "n_updates < 0");
  DevWorld& W = w->W;
  if (W.rec) return fail(AVGPU_EUNSUPPORTED, "the serial world takes its own two streams (avgpu_set_serial_streams), "
                                             "not per-organism recorded streams");
  if (W.tiled) return fail(AVGPU_EUNSUPPORTED, "the serial world runs single worlds, not strip tiles");
  if (W.birth_method == 1 || W.birth_method == 2)
    return fail(AVGPU_EUNSUPPORTED, "BIRTH_METHOD 1 / 2 run on the batch world, not the serial world");
  if ((rc = serial_alloc(w)) < 0) return rc;
  if (w->reaper_rebuild && (rc = reaper_build(w)) < 0) return rc;
  for (int u = 0; u < n; u++) {
    launch_reset_counts(W, w->stream);
    launch_age_tick(W, w->stream);
    launch_resources_begin(W, w->stream);
    after_resources_begin(w);
    if ((rc = push_world(w)) < 0) return rc;
    launch_serial_update(W, w->d_W, w->stream);
    launch_serial_post(W, w->stream, w->d_stats);
    HIPCHK(hipGetLastError());
    w->stats_stale = false;
    w->update++;
  }
  if (last) return avgpu_get_stats(w, last);
  return 0;
}

}  // extern "C"
