// host.h -- what the C-API translation units (capi*.hip) share.  Host only:
// nothing that holds a kernel includes it.
//
// Ownership: locals and members own, through the scoped types below; the
// structs a launch takes by value (DevWorld, the *Scratch views: device.h) only
// view.  Each on-demand subsystem keeps its state in one struct (GenotypeTable
// .. PopEvents), and one function per subsystem writes its view from the
// owners.  avgpu_world::alloc makes the arrays that live as long as the world.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "device.h"
#include "grow.h"

// (hidden: the helpers cross the library's files, not its boundary)
namespace avh __attribute__((visibility("hidden"))) {

// avgpu_last_error's string: one object per thread for every C-API file
inline std::string& last_error() {
  thread_local std::string e;
  return e;
}

inline int fail(int code, const std::string& msg) {
  last_error() = msg;
  return code;
}

#define HIPCHK(x)                                                                   \
  do {                                                                              \
    hipError_t _e = (x);                                                            \
    if (_e != hipSuccess) return fail(AVGPU_EHIP, std::string(#x ": ") + hipGetErrorString(_e)); \
  } while (0)
// (a call that returns one of the library's own codes)
#define RCCHK(x) do { const int _rc = (x); if (_rc < 0) return _rc; } while (0)
// A copy / fill of an API call on the world's stream, complete on return.  The
// world's streams are non-blocking: a null-stream hipMemcpy / hipMemset would
// neither wait for the kernels queued on them nor be waited for by them.
#define COPY_SYNC(ww, dst, src, bytes, kind)                                        \
  do {                                                                              \
    HIPCHK(hipMemcpyAsync((dst), (src), (bytes), (kind), (ww)->stream));           \
    HIPCHK(hipStreamSynchronize((ww)->stream));                                     \
  } while (0)
#define SET_SYNC(ww, dst, val, bytes)                                               \
  do {                                                                              \
    HIPCHK(hipMemsetAsync((dst), (val), (bytes), (ww)->stream));                    \
    HIPCHK(hipStreamSynchronize((ww)->stream));                                     \
  } while (0)

// what the library owns right now: device and pinned buffers, events, streams
// (avgpu_live_objects)
inline std::atomic<int64_t> g_live{0};

// One hipMalloc, and the elements it has room for.  A temporary that queued
// work reads is made with that work's stream: the stream is synchronised before
// the buffer is freed, so no return path, an early one included, frees under a
// running kernel.  A member is made without one and grows by reserve.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(hipStream_t s) : stream_(s), sync_(true) {}
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_), stream_(o.stream_), sync_(o.sync_) { o.p_ = nullptr; o.cap_ = 0; }
  // the buffers change hands, each side keeps its stream: what this held goes with o
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
  ~DevBuf() { reset(); }
  int alloc(size_t count) {
    reset();
    hipError_t e = hipMalloc((void**)&p_, std::max<size_t>(count * sizeof(T), 16));
    if (e != hipSuccess) { p_ = nullptr; return fail(AVGPU_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    g_live++;
    cap_ = (int64_t)count;
    return 0;
  }
  // Room for `need` elements: a buffer of grown_capacity(need, g), the first
  // `keep` copied over on `s`.  The new buffer is the local nb until it is
  // complete; after the swap nb holds the old one, and nb's destructor
  // synchronises `s` before it frees it (work queued on `s` may still read it).
  // On a failure nothing has changed.  Buffers that grow together follow the
  // same steps by hand (arbiter_reserve).
  int reserve(hipStream_t s, int64_t need, const Growth& g = {}, int64_t keep = 0) {
    if (need <= cap_) return 0;
    DevBuf nb(s);
    RCCHK(nb.alloc((size_t)grown_capacity(need, g)));
    if (keep > 0) {
      HIPCHK(hipMemcpyAsync(nb.p_, p_, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    *this = std::move(nb);
    return 0;
  }
  T* get() const { return p_; }
  int64_t capacity() const { return cap_; }
  void reset() {
    if (!p_) return;
    if (sync_) hipStreamSynchronize(stream_);
    hipFree(p_);
    g_live--;
    p_ = nullptr;
    cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  int64_t cap_ = 0;
  hipStream_t stream_ = nullptr;
  bool sync_ = false;
};

// One hipHostMalloc.
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }
  ~PinnedBuf() { reset(); }
  int alloc(size_t count, unsigned flags) {
    reset();
    hipError_t e = hipHostMalloc((void**)&p_, count * sizeof(T), flags);
    if (e != hipSuccess) { p_ = nullptr; return fail(AVGPU_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    g_live++;
    return 0;
  }
  T* get() const { return p_; }
  void reset() {
    if (!p_) return;
    hipHostFree(p_);
    g_live--;
    p_ = nullptr;
  }

 private:
  T* p_ = nullptr;
};

// One hipEvent_t.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
  ~Event() { if (e_) { hipEventDestroy(e_); g_live--; } }
  int create(unsigned flags = hipEventDefault) {
    if (e_) return 0;
    if (hipEventCreateWithFlags(&e_, flags) != hipSuccess) { e_ = nullptr; return fail(AVGPU_EHIP, "event creation failed"); }
    g_live++;
    return 0;
  }
  hipEvent_t get() const { return e_; }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// The event pair around a call's kernels, and the device time between them.
class EventTimer {
 public:
  int create() { RCCHK(t0_.create()); return t1_.create(); }   // (once, like Event::create)
  int start(hipStream_t s) { HIPCHK(hipEventRecord(t0_, s)); return 0; }
  int stop(hipStream_t s) { HIPCHK(hipEventRecord(t1_, s)); return 0; }
  // the stream has been synchronised since stop ...
  int elapsed(double* ms) const {
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, t0_, t1_));
    *ms = f;
    return 0;
  }
  // ... or has not: waits for the stop event alone
  int wait_elapsed(double* ms) const { HIPCHK(hipEventSynchronize(t1_)); return elapsed(ms); }

 private:
  Event t0_, t1_;
};

// One hipStream_t.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { std::swap(s_, o.s_); return *this; }
  ~Stream() { if (s_) { hipStreamDestroy(s_); g_live--; } }
  int create(unsigned flags) {
    if (hipStreamCreateWithFlags(&s_, flags) != hipSuccess) { s_ = nullptr; return fail(AVGPU_EHIP, "stream creation failed"); }
    g_live++;
    return 0;
  }
  hipStream_t get() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// ---- the on-demand subsystems: view, buffers, timers,
// counters.  Nothing is allocated before a subsystem's first call. ----
struct GenotypeTable {                 // avgpu_get_genotypes; the view's scratch is in the world's allocs
  GtScratch view = {};
  bool ready = false;
  DevBuf<avgpu_genotype> rows;
  EventTimer t_group, t_rows;
  double ms = 0.0;
  int64_t bytes = 0;
};
struct Arbiter {                       // avgpu_classify_genotypes: n rows of state, the last summary
  ArbScratch view = {};
  bool ready = false;
  DevBuf<avgpu_arbiter_row> row[2];    // these five grow together (arbiter_reserve)
  DevBuf<uint64_t> key[2];
  DevBuf<avgpu_genotype> table;
  PinnedBuf<avgpu_arbiter_summary> sum;   // view.h_sum: host-mapped
  int64_t n = 0;
  avgpu_arbiter_summary last = {};
  EventTimer t_group, t_classify;
  double ms = 0.0;
  int64_t bytes = 0;
};
struct Lineage {                       // avgpu_enable_lineage
  LinScratch view = {};
  bool on = false;
  DevBuf<avgpu_lineage_row> rows;
  DevBuf<uint8_t> arena;
  DevBuf<unsigned long long> ctr;
  DevBuf<int64_t> idx, asz;            // the scratch: these four grow together
  DevBuf<uint32_t> mark;
  DevBuf<int32_t> newcell;
  int64_t rows_hint = 0, arena_hint = 0, dropped = 0;
  EventTimer t_classify, t_prune;
  double classify_ms = 0.0, prune_ms = 0.0;
};
struct Landscapes {                    // avgpu_landscapes: the scratch test world of `chunk` cells
  LandScratch view = {};
  int64_t chunk = 65536;
  avgpu_world* world = nullptr;        // made by the first call, again when chunk changes; avgpu_destroy frees it
  EventTimer timer;
  double ms = 0.0;
  int64_t mutants = 0, runs = 0;
};
struct Distances {                     // avgpu_genome_distances .. avgpu_site_histogram
  DistScratch view = {};
  DevBuf<uint8_t> in;                  // the call's inputs: genomes, offsets, lengths, pairs
  DevBuf<int32_t> out;                 // its results: hamming, then edit
  DevBuf<int32_t> hist;                // the histogram, then the living count (8-B aligned)
  EventTimer timer;
  double ms = 0.0;
  int64_t pairs = 0, cells = 0;
};
struct PopEvents {                     // avgpu_kill_cells .. avgpu_keep_sample
  EvScratch view = {};
  DevBuf<unsigned long long> ctr;      // the killed count, the select's state and histograms (EV_ZERO_BYTES)
  DevBuf<uint64_t> in;                 // a call's cell ids or genotype keys ...
  PinnedBuf<uint64_t> host;            // ... and the pinned words they are uploaded from: the two grow together
  Event uploaded;                      // the last upload from host
  EventTimer timer;                    // around the last call's kernels
  bool timed = false;
  int64_t cells = 0;
};

}  // namespace avh

// Deleted by avgpu_destroy alone, which destroys the scratch world `land.world`
// first.  Then the destructor's body frees the allocs, and the members go in
// reverse order of declaration: the buffers and events, own_stream last.
struct avgpu_world {
  avh::Stream own_stream;
  hipStream_t stream = nullptr;      // current stream (own or external)
  avgpu_cfg cfg;
  int device = 0;
  // event ring around interpreter phases (avgpu_last_kernel_ms,
  // avgpu_kernel_times): ev[i][0] before class 0, ev[i][k+1] after class k
  static const int RING = 512;
  avh::Event ring[RING][NUM_CLASSES + 1];
  int ring_head = 0, ring_count = 0;
  // avgpu_set_timing: bracket every time_every-th interpretation (0: none)
  int time_every = 1;
  int64_t interp_calls = 0;
  double acc_ms = 0.0;
  double acc_class_ms[NUM_CLASSES] = {};
  int64_t acc_phases = 0;
  DevWorld W;
  DevWorld* d_W = nullptr;      // device copy of W read by k_interpret: one of d_Wv
  // two device copies (a world whose resources swap their buffers every
  // update alternates between two descriptors: after two updates neither
  // is uploaded again), uploaded in stream order from pinned staging
  DevWorld* d_Wv[2] = {};
  DevWorld pushedv[2];          // what d_Wv[k] holds
  bool validv[2] = {false, false};
  int cur_w = 0;
  avh::PinnedBuf<DevWorld> h_stage;   // [2]
  avh::Event ev_stage[2];             // the last upload from h_stage[k]
  std::vector<void*> allocs;          // what alloc made
  // instruction set translation
  int n_ops = 0;
  uint8_t op2code[256];
  int16_t code2op[64];
  bool instset_loaded = false;
  int res_geom[AVGPU_MAX_RESOURCES] = {};
  std::vector<avgpu_resource> res_spec;       // avgpu_load_resources input (re-seeded by set_tile)
  std::vector<avgpu_cell_resource> cell_spec;
  avh::DevBuf<avgpu_cell_resource> res_cells;   // W.res_cells, replaced by every load with CELL entries
  bool env_loaded = false;
  // device scratch
  double* d_totals = nullptr;   // [totals_words(nb)] the step totals, then k_merit_partial's scratch (device.h TOT_*)
  double* d_stats = nullptr;    // [stats_words(nb)] the statistics vector, then k_stats_partial's rows (device.h ST_*)
  bool stats_stale = false;     // the last update ran without statistics (out == NULL)
  bool use_global = false;
  int64_t update = 0;
  float last_kernel_ms = 0.f;
  int64_t last_launches = 0;
  bool has_test_buffers = false;
  avh::DevBuf<double> rec_buf;       // RECORDED mode stream (avgpu_set_rng_mode)
  avh::DevBuf<double> srec_buf[2];   // the serial world's recorded streams
  // strip tiles
  int ntiles_last = 0;
  bool tile_buffers = false;
  // batch steps: the last update's predictor and organisms
  // (coherent mapped host memory the update's last step writes, then pred_seq), the
  // host's copy, the steps the last update ran; strips: the current step
  avh::PinnedBuf<long long> h_pred;
  long long* d_pred = nullptr;   // its device address
  bool pred_pending = false;
  long long pred_seq = 0;       // the sequence number k_place_claim0 publishes with the predictor
  bool reaper_rebuild = false;  // the serial reaper queue is built again at the next serial update
  long long pred_acc = 0, pred_n = 0, pred_cnt = 0;
  int last_k = 1;
  int tile_sub = 0, tile_k = 1, tile_sub_next = 0;
  uint32_t tile_key = 0;
  // the on-demand subsystems (above)
  avh::GenotypeTable gt;
  avh::Arbiter arb;
  avh::Lineage lin;
  avh::Landscapes land;
  avh::Distances dist;
  avh::PopEvents pev;
  // the one way to make an array that lives as long as the world: zero-filled
  // in stream order, freed with the world
  template <typename T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return avh::fail(AVGPU_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    hipMemsetAsync(q, 0, bytes, stream);
    allocs.push_back(q);
    avh::g_live++;
    *p = reinterpret_cast<T*>(q);
    return 0;
  }

  ~avgpu_world() {               // (avgpu_destroy: streams idle, land gone)
    for (void* p : allocs) hipFree(p);
    avh::g_live -= (int64_t)allocs.size();
  }
};

namespace avh __attribute__((visibility("hidden"))) {

// capi.hip
avgpu_world* create_world(const avgpu_cfg* cfg, int device, int64_t n, bool test_buffers);
int setup_world(avgpu_world* w, int64_t n, bool test_buffers);
int copy_tables(avgpu_world* dst, const avgpu_world* src);
int ready(avgpu_world* w);
int batch_ready(avgpu_world* w);      // ready for a batch update (avgpu_run_update, avgpu_update_run)
int translate_genomes(avgpu_world* w, const uint8_t* genomes, const int32_t* lens, int64_t count,
                      std::vector<uint8_t>& codes, std::vector<int32_t>& offsets);
int set_orgs_impl(avgpu_world* w, int64_t first, int64_t count, const uint8_t* genomes,
                  const int32_t* lens, const double* merits, const int32_t* inputs, int det);
int push_world(avgpu_world* w);
int interpret(avgpu_world* w, int mode, int64_t first, int64_t count, bool sorted = false);
int drain_ring(avgpu_world* w, int keep);
void after_resources_begin(avgpu_world* w);
uint32_t step_key(const avgpu_world* w, int sub, int K);
int choose_k(const avgpu_cfg& c, long long pred, long long n, bool handed_in, long long cnt);
// capi_lineage.hip
int lineage_step(avgpu_world* w, int64_t n_prev, int64_t id0, int64_t m, int64_t update);
int lineage_clear(avgpu_world* w);
// capi_serial.hip
int reaper_read(avgpu_world* w, std::vector<int32_t>& q);
int reaper_write(avgpu_world* w, const std::vector<int32_t>& q);
int reaper_build(avgpu_world* w);
// capi_resources.hip
int res_seed(avgpu_world* w);

}  // namespace avh
