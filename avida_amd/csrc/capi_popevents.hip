// capi_popevents.hip -- population events (popevents.hip).
#include "host.h"

using namespace avh;

namespace {

// What every call checks first: nothing is queued before it passes.
// indexed: the call draws per cell or indexes a cell by 32 bits.
int ev_check(avgpu_world* w, const char* who, bool indexed) {
  if (!w) return fail(AVGPU_EINVAL, std::string(who) + ": NULL world");
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, std::string(who) + " on a strip tile");
  if (indexed && w->W.n >= (1ll << 32)) return fail(AVGPU_EUNSUPPORTED, std::string(who) + " on 2^32 cells or more");
  return 0;
}

int ev_prob(const char* who, double p, uint64_t* th) {
  if (!(p >= 0.0 && p <= 1.0)) return fail(AVGPU_EINVAL, std::string(who) + ": p outside [0, 1]");
  *th = (uint64_t)std::ceil(std::ldexp(p, 32));     // u < p  <=>  h < ceil(p 2^32), exactly
  return 0;
}

// What every call does once its list is uploaded: the scratch (first call), the
// view from the owners (the scratch's three parts, the list under both its
// types), the scratch zeroed in stream order, the timer started
int ev_begin(avgpu_world* w) {
  PopEvents& P = w->pev;
  static_assert(EV_ZERO_BYTES % 8 == 0, "the scratch is a vector of 8-B words");
  if (!P.ctr.get()) RCCHK(P.ctr.alloc(EV_ZERO_BYTES / 8));
  uint8_t* d = reinterpret_cast<uint8_t*>(P.ctr.get());
  P.view.killed = P.ctr.get();
  P.view.sel = reinterpret_cast<EvSelect*>(d + 16);
  P.view.hist = reinterpret_cast<uint32_t*>(d + 16 + sizeof(EvSelect));
  P.view.cells = reinterpret_cast<const int64_t*>(P.in.get());
  P.view.keys = P.in.get();
  RCCHK(P.timer.create());
  HIPCHK(hipMemsetAsync(P.view.killed, 0, EV_ZERO_BYTES, w->stream));
  return P.timer.start(w->stream);
}

// `count` 8-byte words into pev.in, in stream order, from pinned words the call
// owns until the copy has run: the caller's array is free on return, and
// nobody waits for the queued updates (unless the list outgrows its buffers)
int ev_upload(avgpu_world* w, const void* src, int64_t count) {
  PopEvents& P = w->pev;
  RCCHK(P.uploaded.create());
  HIPCHK(hipEventSynchronize(P.uploaded));          // the previous upload has left the pinned words
  if (count > P.in.capacity()) {
    // the device words and their pinned twin, both or neither (DevBuf::reserve's steps by hand)
    const size_t want = (size_t)grown_capacity(count);
    DevBuf<uint64_t> in(w->stream);
    PinnedBuf<uint64_t> host;
    RCCHK(in.alloc(want));
    RCCHK(host.alloc(want, hipHostMallocDefault));
    P.in = std::move(in);
    P.host = std::move(host);
  }
  memcpy(P.host.get(), src, (size_t)count * 8);
  HIPCHK(hipMemcpyAsync(P.in.get(), P.host.get(), (size_t)count * 8, hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipEventRecord(P.uploaded, w->stream));
  return 0;
}

// after the kernels: the timer stopped; the count, if asked for
int ev_end(avgpu_world* w, int64_t cells, int64_t* killed) {
  HIPCHK(hipGetLastError());
  RCCHK(w->pev.timer.stop(w->stream));
  w->pev.timed = true;
  w->pev.cells = cells;
  if (killed) {
    unsigned long long k = 0;
    COPY_SYNC(w, &k, w->pev.view.killed, 8, hipMemcpyDeviceToHost);
    *killed = (int64_t)k;
  }
  return 0;
}

int clampi(int v, int dim) { return v < 0 ? 0 : (v > dim - 1 ? dim - 1 : v); }

}  // namespace

extern "C" {

int avgpu_kill_cells(avgpu_world* w, const int64_t* cells, int64_t n, int64_t* killed) {
  RCCHK(ev_check(w, "avgpu_kill_cells", false));
  if (n < 0 || n > (1ll << 31) || (n > 0 && !cells)) return fail(AVGPU_EINVAL, "avgpu_kill_cells: n or a NULL list");
  for (int64_t i = 0; i < n; i++)
    if (cells[i] < 0 || cells[i] >= w->W.n) return fail(AVGPU_EINVAL, "avgpu_kill_cells: a cell outside the world");
  if (n > 0) RCCHK(ev_upload(w, cells, n));
  RCCHK(ev_begin(w));
  if (n > 0) launch_kill_cells(w->W, w->pev.view, w->stream, n);
  return ev_end(w, n, killed);
}

int avgpu_kill_prob(avgpu_world* w, double p, uint64_t key, int64_t* killed) {
  uint64_t th;
  int rc = ev_check(w, "avgpu_kill_prob", true);
  if (rc < 0 || (rc = ev_prob("avgpu_kill_prob", p, &th)) < 0 || (rc = ev_begin(w)) < 0) return rc;
  launch_kill_prob(w->W, w->pev.view, w->stream, event_base(w->W.seed_lo, w->W.seed_hi, key), th, -1);
  return ev_end(w, w->W.n, killed);
}

int avgpu_kill_rect(avgpu_world* w, int x1, int y1, int x2, int y2, int64_t* killed) {
  RCCHK(ev_check(w, "avgpu_kill_rect", true));
  const int X = w->W.world_x, Y = w->W.world_y;
  if ((int64_t)X * Y != w->W.n) return fail(AVGPU_ESTATE, "avgpu_kill_rect: the world is not WORLD_X x WORLD_Y cells");
  // cActionKillRectangle's constructor (actions/PopulationActions.cc:1770-1798)
  x1 = clampi(x1, X); x2 = clampi(x2, X);
  y1 = clampi(y1, Y); y2 = clampi(y2, Y);
  if (x2 < x1) x2 += X;
  if (y2 < y1) y2 += Y;
  RCCHK(ev_begin(w));
  launch_kill_rect(w->W, w->pev.view, w->stream, x1, y1, x2, y2);
  return ev_end(w, (int64_t)(y2 - y1 + 1) * X, killed);
}

int avgpu_kill_genotypes(avgpu_world* w, const uint64_t* keys, int64_t nkeys, double p, uint64_t key, int64_t* killed) {
  uint64_t th;
  int rc = ev_check(w, "avgpu_kill_genotypes", true);
  if (rc < 0 || (rc = ev_prob("avgpu_kill_genotypes", p, &th)) < 0) return rc;
  if (nkeys < 0 || (nkeys > 0 && !keys)) return fail(AVGPU_EINVAL, "avgpu_kill_genotypes: nkeys or a NULL list");
  // a sorted copy without duplicates: the device searches it per cell
  std::vector<uint64_t> sorted(keys, keys + nkeys);
  std::sort(sorted.begin(), sorted.end());
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  if (nkeys > 0 && (rc = ev_upload(w, sorted.data(), (int64_t)sorted.size())) < 0) return rc;
  if ((rc = ev_begin(w)) < 0) return rc;
  if (nkeys > 0)
    launch_kill_prob(w->W, w->pev.view, w->stream, event_base(w->W.seed_lo, w->W.seed_hi, key), th, (int64_t)sorted.size());
  return ev_end(w, nkeys > 0 ? w->W.n : 0, killed);
}

int avgpu_keep_sample(avgpu_world* w, int64_t keep, uint64_t key, int64_t* killed) {
  RCCHK(ev_check(w, "avgpu_keep_sample", true));
  if (keep < 0) return fail(AVGPU_EINVAL, "avgpu_keep_sample: keep < 0");
  RCCHK(ev_begin(w));
  const uint32_t base = event_base(w->W.seed_lo, w->W.seed_hi, key);
  if (keep == 0) {                                  // nobody survives: every word is below 2^32
    launch_kill_prob(w->W, w->pev.view, w->stream, base, 1ull << 32, -1);
    return ev_end(w, w->W.n, killed);
  }
  launch_keep_sample(w->W, w->pev.view, w->stream, base, keep);
  return ev_end(w, (EV_PASSES + 1) * w->W.n, killed);
}

int avgpu_last_event_ms(avgpu_world* w, double* device_ms, int64_t* cells_scanned) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  double ms = 0.0;
  if (w->pev.timed) RCCHK(w->pev.timer.wait_elapsed(&ms));   // (the call's kernels may still be queued)
  if (device_ms) *device_ms = ms;
  if (cells_scanned) *cells_scanned = w->pev.timed ? w->pev.cells : 0;
  return 0;
}

}  // extern "C"
