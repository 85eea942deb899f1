// host.h -- what the C-API translation units (capi*.hip) share.  Host only:
// nothing that holds a kernel includes it.
//
// Ownership: locals and members own, through the four scoped types below; the
// structs a launch takes by value (DevWorld, GtScratch, ArbScratch,
// LandScratch: device.h) only view, and are assigned from the owners where a
// buffer is (re)allocated.  avgpu_world::alloc makes the arrays that live as
// long as the world.
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

// One hipMalloc.  A temporary that queued work reads is made with that work's
// stream: the stream is synchronised before the buffer is freed, so no return
// path, an early one included, frees under a running kernel.  A member is made
// without one: whoever replaces it, and avgpu_destroy, synchronise first.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(hipStream_t s) : stream_(s), sync_(true) {}
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), stream_(o.stream_), sync_(o.sync_) { o.p_ = nullptr; }
  // the buffers change hands, each side keeps its stream: what this held goes with o
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }
  ~DevBuf() { reset(); }
  int alloc(size_t count) {
    reset();
    hipError_t e = hipMalloc((void**)&p_, std::max<size_t>(count * sizeof(T), 16));
    if (e != hipSuccess) { p_ = nullptr; return fail(AVGPU_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
    g_live++;
    return 0;
  }
  T* get() const { return p_; }
  void reset() {
    if (!p_) return;
    if (sync_) hipStreamSynchronize(stream_);
    hipFree(p_);
    g_live--;
    p_ = nullptr;
  }

 private:
  T* p_ = nullptr;
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

}  // namespace avh

// Deleted by avgpu_destroy alone, which destroys the scratch world `land`
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
  // the genotype table (avgpu_get_genotypes): scratch allocated at the first
  // call (in allocs), the row buffer grown to the largest table seen
  GtScratch gt = {};
  bool gt_ready = false;
  avh::DevBuf<avgpu_genotype> gt_rows;
  int64_t gt_rows_cap = 0;
  avh::Event ev_gt[4];
  double gt_ms = 0.0;
  int64_t gt_bytes = 0;
  // the device-resident genotype arbiter (avgpu_classify_genotypes): buffers
  // allocated at the first use, grown with the row buffer's policy (arb views
  // them); arb_n rows of state, arb_last the summary of the last
  // classification (or set / reset)
  ArbScratch arb = {};
  avh::DevBuf<avgpu_arbiter_row> arb_row[2];
  avh::DevBuf<uint64_t> arb_key[2];
  avh::DevBuf<avgpu_genotype> arb_table;
  avh::PinnedBuf<avgpu_arbiter_summary> arb_sum;   // arb.h_sum: host-mapped
  bool arb_ready = false;
  int64_t arb_n = 0;
  avgpu_arbiter_summary arb_last = {};
  avh::Event ev_arb[4];
  double arb_ms = 0.0;
  int64_t arb_bytes = 0;
  // the lineage store (avgpu_enable_lineage; lineage.hip): lin is the view the
  // launches take, assigned where a buffer is (re)allocated
  bool lin_on = false;
  LinScratch lin = {};
  avh::DevBuf<avgpu_lineage_row> lin_rows;
  avh::DevBuf<uint8_t> lin_arena;
  avh::DevBuf<unsigned long long> lin_ctr;
  avh::DevBuf<int64_t> lin_idx, lin_asz;
  avh::DevBuf<uint32_t> lin_mark;
  avh::DevBuf<int32_t> lin_newcell;
  int64_t lin_rows_hint = 0, lin_arena_hint = 0, lin_dropped = 0;
  avh::Event ev_lin[4];
  double lin_ms = 0.0, lin_prune_ms = 0.0;
  // mutational landscapes (avgpu_landscapes): the scratch test world of
  // land_chunk cells the mutants run through and the per-chunk scratch (in its
  // allocs), created by the first call, re-created when land_chunk changes
  LandScratch land_s = {};
  int64_t land_chunk = 65536;
  avh::Event ev_land[2];
  double land_ms = 0.0;
  int64_t land_mutants = 0, land_runs = 0;
  avgpu_world* land = nullptr;
  // genetic distances and the consensus histogram (avgpu_genome_distances,
  // avgpu_cell_distances, avgpu_site_histogram; distance.hip): dist views the
  // buffers, each allocated at its first use and grown by 1.25x
  DistScratch dist = {};
  avh::DevBuf<uint8_t> dist_in;        // the call's inputs: genomes, offsets, lengths, pairs
  avh::DevBuf<int32_t> dist_out;       // its results: hamming, then edit
  avh::DevBuf<int32_t> dist_hist;      // the histogram, then the living count (8-B aligned)
  int64_t dist_in_cap = 0, dist_out_cap = 0;
  avh::Event ev_dist[2];
  double dist_ms = 0.0;
  int64_t dist_pairs = 0, dist_cells = 0;
  // population events (avgpu_kill_cells .. avgpu_keep_sample; popevents.hip):
  // pev views the buffers, each allocated at its first use
  EvScratch pev = {};
  avh::DevBuf<unsigned long long> pev_ctr;  // the killed count, the select's state and histograms (EV_ZERO_BYTES)
  avh::DevBuf<uint64_t> pev_in;             // a call's cell ids or genotype keys, grown by 1.25x
  avh::PinnedBuf<uint64_t> pev_host;        // ... and the pinned words they are uploaded from
  int64_t pev_in_cap = 0;
  avh::Event ev_pev[2];                     // around the last call's kernels
  avh::Event ev_pev_up;                     // the last upload from pev_host
  bool pev_timed = false;
  int64_t pev_cells = 0;

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
// capi_serial.hip
int reaper_read(avgpu_world* w, std::vector<int32_t>& q);
int reaper_write(avgpu_world* w, const std::vector<int32_t>& q);
int reaper_build(avgpu_world* w);
// capi_resources.hip
int res_seed(avgpu_world* w);

}  // namespace avh
