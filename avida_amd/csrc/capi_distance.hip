// capi_distance.hip -- genetic distances and the consensus histogram
// (distance.hip).
#include "host.h"

using namespace avh;

namespace {

const size_t HIST_WORDS = (size_t)AVGPU_MAX_GENOME * (AVGPU_MAX_INST + 1);

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// What every call does first: room for its inputs and for `n` results of each
// kind, the timer, and the view from the owners -- the input buffer's sections
// at the call's offsets, the results, the histogram with the living count
// behind it.  A section the call does not have (offset 0) aliases gen, and a
// buffer not yet made is NULL: the call's kernels read neither.
int dist_prepare(avgpu_world* w, int64_t in_bytes, int64_t n, size_t o_off = 0, size_t o_len = 0, size_t o_pa = 0,
                 size_t o_pb = 0) {
  Distances& D = w->dist;
  RCCHK(D.in.reserve(w->stream, in_bytes));
  RCCHK(D.out.reserve(w->stream, 2 * n));
  RCCHK(D.timer.create());
  DistScratch& S = D.view;
  uint8_t* d = D.in.get();
  S.gen = d;
  S.off = reinterpret_cast<int64_t*>(d + o_off);
  S.len = reinterpret_cast<int32_t*>(d + o_len);
  S.pair_a = reinterpret_cast<int32_t*>(d + o_pa);
  S.pair_b = reinterpret_cast<int32_t*>(d + o_pb);
  S.ham = D.out.get();
  S.edit = S.ham + n;
  S.hist = D.hist.get();
  static_assert(HIST_WORDS % 2 == 0, "the living count behind the histogram is 8-B aligned");
  S.living = S.hist ? reinterpret_cast<unsigned long long*>(S.hist + HIST_WORDS) : nullptr;
  return 0;
}

// after a distance kernel: the timer stopped, the `n` results of each kind
// asked for (through a buffer of the call's own: a failed copy leaves the
// outputs untouched), the call's device time and counts
int dist_results(avgpu_world* w, int64_t n, bool pairs, int32_t* hamming, int32_t* edit) {
  const DistScratch& S = w->dist.view;
  const size_t bytes = (size_t)n * sizeof(int32_t);
  HIPCHK(hipGetLastError());
  RCCHK(w->dist.timer.stop(w->stream));
  std::vector<int32_t> res(2 * (size_t)n);
  if (hamming) HIPCHK(hipMemcpyAsync(res.data(), S.ham, bytes, hipMemcpyDeviceToHost, w->stream));
  if (edit) HIPCHK(hipMemcpyAsync(res.data() + n, S.edit, bytes, hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  RCCHK(w->dist.timer.elapsed(&w->dist.ms));
  w->dist.pairs = pairs ? n : 0;
  w->dist.cells = pairs ? 0 : n;
  if (hamming) memcpy(hamming, res.data(), bytes);
  if (edit) memcpy(edit, res.data() + n, bytes);
  return 0;
}

int check_range(const avgpu_world* w, const char* who, int64_t first, int64_t count) {
  if (first < 0 || count <= 0 || first > w->W.n || count > w->W.n - first)
    return fail(AVGPU_EINVAL, std::string(who) + ": cell range outside the world");
  return 0;
}

}  // namespace

extern "C" {

int avgpu_genome_distances(avgpu_world* w, int n, const uint8_t* genomes, const int32_t* lens, int64_t npairs,
                           const int32_t* pair_a, const int32_t* pair_b, int32_t* hamming, int32_t* edit) {
  auto refuse = [](const char* what) { return fail(AVGPU_EINVAL, std::string("avgpu_genome_distances: ") + what); };
  RCCHK(ready(w));
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genetic distances on strip tiles");
  if (n <= 0 || npairs <= 0 || npairs > (1ll << 30) || !genomes || !lens || !pair_a || !pair_b)
    return refuse("n or npairs <= 0, more than 2^30 pairs, or a NULL argument");
  if (!hamming && !edit) return refuse("both outputs NULL");
  // the genomes at 16-B aligned offsets, zero padded: the kernel reads whole 16-B groups
  std::vector<int64_t> off((size_t)n);
  size_t bytes = 0, in = 0;
  for (int g = 0; g < n; g++) {
    if (lens[g] < 1 || lens[g] > AVGPU_MAX_GENOME) return refuse("genome length out of range");
    off[g] = (int64_t)bytes;
    bytes += align16((size_t)lens[g]);
  }
  std::vector<uint8_t> packed(bytes, 0);
  for (int g = 0; g < n; g++) {
    for (int k = 0; k < lens[g]; k++) {
      const uint8_t op = genomes[in + (size_t)k];
      if (op >= w->n_ops) return refuse("genome op outside the instruction set");
      packed[(size_t)off[g] + k] = op;
    }
    in += (size_t)lens[g];
  }
  for (int64_t p = 0; p < npairs; p++)
    if (pair_a[p] < 0 || pair_a[p] >= n || pair_b[p] < 0 || pair_b[p] >= n) return refuse("pair index outside 0..n-1");
  // one input buffer: genomes | offsets | lengths | pair_a | pair_b
  const size_t o_off = align16(bytes), o_len = o_off + align16((size_t)n * sizeof(int64_t));
  const size_t o_pa = o_len + align16((size_t)n * sizeof(int32_t));
  const size_t o_pb = o_pa + align16((size_t)npairs * sizeof(int32_t));
  const size_t total = o_pb + align16((size_t)npairs * sizeof(int32_t));
  RCCHK(dist_prepare(w, (int64_t)total, npairs, o_off, o_len, o_pa, o_pb));
  const DistScratch& S = w->dist.view;
  HIPCHK(hipMemcpyAsync(S.gen, packed.data(), bytes, hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(S.off, off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(S.len, lens, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(S.pair_a, pair_a, (size_t)npairs * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(S.pair_b, pair_b, (size_t)npairs * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  RCCHK(w->dist.timer.start(w->stream));
  launch_pair_dist(S, w->stream, (int)npairs, hamming != nullptr, edit != nullptr);
  return dist_results(w, npairs, true, hamming, edit);
}

int avgpu_cell_distances(avgpu_world* w, int64_t first_cell, int64_t count, const uint8_t* ref, int32_t ref_len,
                         int32_t* hamming, int32_t* edit) {
  auto refuse = [](const char* what) { return fail(AVGPU_EINVAL, std::string("avgpu_cell_distances: ") + what); };
  RCCHK(ready(w));
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "genetic distances on strip tiles");
  RCCHK(check_range(w, "avgpu_cell_distances", first_cell, count));
  if (!ref || ref_len < 1 || ref_len > AVGPU_MAX_GENOME) return refuse("reference length out of range, or a NULL reference");
  if (!hamming && !edit) return refuse("both outputs NULL");
  // the tapes hold canonical codes: the reference is compared as such
  std::vector<uint8_t> codes(align16((size_t)ref_len), 0);
  for (int k = 0; k < ref_len; k++) {
    if (ref[k] >= w->n_ops) return refuse("reference op outside the instruction set");
    codes[k] = w->op2code[ref[k]];
  }
  RCCHK(dist_prepare(w, (int64_t)codes.size(), count));
  const DistScratch& S = w->dist.view;
  HIPCHK(hipMemcpyAsync(S.gen, codes.data(), codes.size(), hipMemcpyHostToDevice, w->stream));
  RCCHK(w->dist.timer.start(w->stream));
  launch_cell_dist(w->W, S, w->stream, first_cell, count, ref_len, hamming != nullptr, edit != nullptr);
  return dist_results(w, count, false, hamming, edit);
}

int avgpu_site_histogram(avgpu_world* w, int64_t first_cell, int64_t count, int32_t* hist, int64_t* num_living) {
  RCCHK(ready(w));
  if (w->W.tiled) return fail(AVGPU_EUNSUPPORTED, "site histogram on strip tiles");
  if (w->W.n >= (1ll << 31)) return fail(AVGPU_EUNSUPPORTED, "site histogram of 2^31 cells or more");
  RCCHK(check_range(w, "avgpu_site_histogram", first_cell, count));
  if (!hist) return fail(AVGPU_EINVAL, "avgpu_site_histogram: NULL hist");
  if (!w->dist.hist.get()) RCCHK(w->dist.hist.alloc(HIST_WORDS + 2));    // (+ the living count, 8 B)
  RCCHK(dist_prepare(w, 0, 0));
  const DistScratch& S = w->dist.view;
  HIPCHK(hipMemsetAsync(S.hist, 0, (HIST_WORDS + 2) * sizeof(int32_t), w->stream));
  RCCHK(w->dist.timer.start(w->stream));
  launch_site_hist(w->W, S, w->stream, first_cell, count);
  HIPCHK(hipGetLastError());
  RCCHK(w->dist.timer.stop(w->stream));
  std::vector<int32_t> dev(HIST_WORDS + 2);
  COPY_SYNC(w, dev.data(), S.hist, dev.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
  RCCHK(w->dist.timer.elapsed(&w->dist.ms));
  w->dist.pairs = 0;
  w->dist.cells = count;
  // the device counts by handler; the caller gets op columns
  const int cols = AVGPU_MAX_INST + 1;
  for (int h = 0; h < AVGPU_MAX_INST; h++) {
    if (w->code2op[h] >= 0 && w->code2op[h] < AVGPU_MAX_INST) continue;
    for (int j = 0; j < AVGPU_MAX_GENOME; j++)
      if (dev[(size_t)j * cols + 1 + h])
        return fail(AVGPU_ESTATE, "avgpu_site_histogram: a genome holds a handler outside the instruction set");
  }
  memset(hist, 0, HIST_WORDS * sizeof(int32_t));
  for (int j = 0; j < AVGPU_MAX_GENOME; j++) {
    const int32_t* src = dev.data() + (size_t)j * cols;
    int32_t* dst = hist + (size_t)j * cols;
    dst[0] = src[0];
    for (int h = 0; h < AVGPU_MAX_INST; h++)
      if (src[1 + h]) dst[1 + w->code2op[h]] += src[1 + h];
  }
  if (num_living) {
    unsigned long long living;
    memcpy(&living, dev.data() + HIST_WORDS, sizeof(living));
    *num_living = (int64_t)living;
  }
  return 0;
}

int avgpu_last_distance_ms(avgpu_world* w, double* device_ms, int64_t* pairs, int64_t* cells) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  if (device_ms) *device_ms = w->dist.ms;
  if (pairs) *pairs = w->dist.pairs;
  if (cells) *cells = w->dist.cells;
  return 0;
}

}  // extern "C"
