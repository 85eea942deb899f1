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

// the scratch (first call), zeroed in stream order; the first timing event
int ev_begin(avgpu_world* w) {
  int rc;
  static_assert(EV_ZERO_BYTES % 8 == 0, "the scratch is a vector of 8-B words");
  if (!w->pev_ctr.get()) {
    if ((rc = w->pev_ctr.alloc(EV_ZERO_BYTES / 8)) < 0) return rc;
    uint8_t* d = reinterpret_cast<uint8_t*>(w->pev_ctr.get());
    w->pev.killed = w->pev_ctr.get();
    w->pev.sel = reinterpret_cast<EvSelect*>(d + 16);
    w->pev.hist = reinterpret_cast<uint32_t*>(d + 16 + sizeof(EvSelect));
  }
  for (Event& e : w->ev_pev)
    if ((rc = e.create()) < 0) return rc;
  HIPCHK(hipMemsetAsync(w->pev.killed, 0, EV_ZERO_BYTES, w->stream));
  HIPCHK(hipEventRecord(w->ev_pev[0], w->stream));
  return 0;
}

// `count` 8-byte words into pev_in, in stream order, from pinned words the call
// owns until the copy has run: the caller's array is free on return, and
// nobody waits for the queued updates
int ev_upload(avgpu_world* w, const void* src, int64_t count) {
  int rc;
  if ((rc = w->ev_pev_up.create()) < 0) return rc;
  HIPCHK(hipEventSynchronize(w->ev_pev_up));        // the previous upload has left the pinned words
  if (count > w->pev_in_cap) {
    HIPCHK(hipStreamSynchronize(w->stream));        // no kernel of an earlier call still reads the old buffer
    const int64_t want = count + count / 4;
    w->pev_in_cap = 0;
    if ((rc = w->pev_in.alloc((size_t)want)) < 0 || (rc = w->pev_host.alloc((size_t)want, hipHostMallocDefault)) < 0)
      return rc;
    w->pev_in_cap = want;
  }
  memcpy(w->pev_host.get(), src, (size_t)count * 8);
  HIPCHK(hipMemcpyAsync(w->pev_in.get(), w->pev_host.get(), (size_t)count * 8, hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipEventRecord(w->ev_pev_up, w->stream));
  return 0;
}

// after the kernels: the second timing event; the count, if asked for
int ev_end(avgpu_world* w, int64_t cells, int64_t* killed) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev_pev[1], w->stream));
  w->pev_timed = true;
  w->pev_cells = cells;
  if (killed) {
    unsigned long long k = 0;
    COPY_SYNC(w, &k, w->pev.killed, 8, hipMemcpyDeviceToHost);
    *killed = (int64_t)k;
  }
  return 0;
}

int clampi(int v, int dim) { return v < 0 ? 0 : (v > dim - 1 ? dim - 1 : v); }

}  // namespace

extern "C" {

int avgpu_kill_cells(avgpu_world* w, const int64_t* cells, int64_t n, int64_t* killed) {
  int rc = ev_check(w, "avgpu_kill_cells", false);
  if (rc < 0) return rc;
  if (n < 0 || n > (1ll << 31) || (n > 0 && !cells)) return fail(AVGPU_EINVAL, "avgpu_kill_cells: n or a NULL list");
  for (int64_t i = 0; i < n; i++)
    if (cells[i] < 0 || cells[i] >= w->W.n) return fail(AVGPU_EINVAL, "avgpu_kill_cells: a cell outside the world");
  if (n > 0 && (rc = ev_upload(w, cells, n)) < 0) return rc;
  if ((rc = ev_begin(w)) < 0) return rc;
  w->pev.cells = reinterpret_cast<const int64_t*>(w->pev_in.get());
  if (n > 0) launch_kill_cells(w->W, w->pev, w->stream, n);
  return ev_end(w, n, killed);
}

int avgpu_kill_prob(avgpu_world* w, double p, uint64_t key, int64_t* killed) {
  uint64_t th;
  int rc = ev_check(w, "avgpu_kill_prob", true);
  if (rc < 0 || (rc = ev_prob("avgpu_kill_prob", p, &th)) < 0 || (rc = ev_begin(w)) < 0) return rc;
  launch_kill_prob(w->W, w->pev, w->stream, event_base(w->W.seed_lo, w->W.seed_hi, key), th, -1);
  return ev_end(w, w->W.n, killed);
}

int avgpu_kill_rect(avgpu_world* w, int x1, int y1, int x2, int y2, int64_t* killed) {
  int rc = ev_check(w, "avgpu_kill_rect", true);
  if (rc < 0) return rc;
  const int X = w->W.world_x, Y = w->W.world_y;
  if ((int64_t)X * Y != w->W.n) return fail(AVGPU_ESTATE, "avgpu_kill_rect: the world is not WORLD_X x WORLD_Y cells");
  // cActionKillRectangle's constructor (actions/PopulationActions.cc:1770-1798)
  x1 = clampi(x1, X); x2 = clampi(x2, X);
  y1 = clampi(y1, Y); y2 = clampi(y2, Y);
  if (x2 < x1) x2 += X;
  if (y2 < y1) y2 += Y;
  if ((rc = ev_begin(w)) < 0) return rc;
  launch_kill_rect(w->W, w->pev, w->stream, x1, y1, x2, y2);
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
  w->pev.keys = w->pev_in.get();
  if (nkeys > 0)
    launch_kill_prob(w->W, w->pev, w->stream, event_base(w->W.seed_lo, w->W.seed_hi, key), th, (int64_t)sorted.size());
  return ev_end(w, nkeys > 0 ? w->W.n : 0, killed);
}

int avgpu_keep_sample(avgpu_world* w, int64_t keep, uint64_t key, int64_t* killed) {
  int rc = ev_check(w, "avgpu_keep_sample", true);
  if (rc < 0) return rc;
  if (keep < 0) return fail(AVGPU_EINVAL, "avgpu_keep_sample: keep < 0");
  if ((rc = ev_begin(w)) < 0) return rc;
  const uint32_t base = event_base(w->W.seed_lo, w->W.seed_hi, key);
  if (keep == 0) {                                  // nobody survives: every word is below 2^32
    launch_kill_prob(w->W, w->pev, w->stream, base, 1ull << 32, -1);
    return ev_end(w, w->W.n, killed);
  }
  launch_keep_sample(w->W, w->pev, w->stream, base, keep);
  return ev_end(w, (EV_PASSES + 1) * w->W.n, killed);
}

int avgpu_last_event_ms(avgpu_world* w, double* device_ms, int64_t* cells_scanned) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  float ms = 0.f;
  if (w->pev_timed) {
    HIPCHK(hipEventSynchronize(w->ev_pev[1]));
    HIPCHK(hipEventElapsedTime(&ms, w->ev_pev[0], w->ev_pev[1]));
  }
  if (device_ms) *device_ms = ms;
  if (cells_scanned) *cells_scanned = w->pev_timed ? w->pev_cells : 0;
  return 0;
}

}  // extern "C"
