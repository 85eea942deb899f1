// genotypes.hip -- the genotype table (include/avida_gpu.h avgpu_get_genotypes;
// DESIGN.md section 10): one row per distinct non-zero genome key among the
// living cells, rows ascending by key.
//
//   k_gt_init      sort key per cell (key - 1; an empty cell or a zero key
//                  becomes 2^64-1 and sorts behind every genotype) + the totals
//   8 x { k_gt_hist, k_gt_scan, k_gt_scatter }
//                  stable LSD radix sort of (key, cell), 8 bits a pass: cells
//                  ascend within a key
//   k_gt_tiles<0>  per 256 sorted positions: segmented scan, the tile's open
//                  tail part, its head flag and its number of segment ends
//   k_gt_carry     one block: segmented scan over the tiles (a segment may
//                  span any number of them) + the row offset of every tile
//   k_gt_tiles<1>  the same in-tile scan again; the lane holding a segment's
//                  last position joins the carry and writes the row
//
// Every double sum has one fixed shape, a function of the sorted positions
// alone (hence of the (key, cell) set): Hillis-Steele inside a 256-position
// tile, Hillis-Steele over 512 tiles, 512-tile chunks in ascending order.
// Nothing is added with floating-point atomics.
#include <hip/hip_runtime.h>

#include "device.h"

namespace {

constexpr int RS_THREADS = 256;                    // radix sort block
constexpr int RS_ROUNDS = 16;                      // keys per thread
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_SLOTS = RS_ROUNDS * RS_WAVES;     // (round, wave) groups of 64 keys, in tile order
static_assert(RS_THREADS * RS_ROUNDS == GT_SORT_TILE, "sort tile");
constexpr int CARRY_THREADS = 512;
constexpr uint64_t KEY_NONE = ~0ull;

__device__ __forceinline__ GtAgg gt_identity() {
  GtAgg a;
  a.n = 0; a.ng = 0;
  a.sm = 0.0; a.sf = 0.0; a.sr = 0.0; a.mx = -__builtin_inf();
  a.sg = 0; a.sc = 0;
  a.first = 0x7fffffff; a.pad = 0;
  return a;
}

// a: the earlier positions, b: the later ones
__device__ __forceinline__ GtAgg gt_join(const GtAgg& a, const GtAgg& b) {
  GtAgg r;
  r.n = a.n + b.n; r.ng = a.ng + b.ng;
  r.sm = __dadd_rn(a.sm, b.sm); r.sf = __dadd_rn(a.sf, b.sf); r.sr = __dadd_rn(a.sr, b.sr);
  r.mx = a.mx > b.mx ? a.mx : b.mx;
  r.sg = a.sg + b.sg; r.sc = a.sc + b.sc;
  r.first = a.first < b.first ? a.first : b.first; r.pad = 0;
  return r;
}

// LDS image of B aggregates, one array per field (8-byte strides: no bank
// conflicts between neighbouring lanes)
template <int B>
struct GtLds {
  int2 cnt[B];
  double sm[B], sf[B], sr[B], mx[B];
  long long sg[B], sc[B];
  int first[B], flag[B];
  __device__ __forceinline__ void store(int t, const GtAgg& a, int f) {
    cnt[t] = make_int2(a.n, a.ng);
    sm[t] = a.sm; sf[t] = a.sf; sr[t] = a.sr; mx[t] = a.mx;
    sg[t] = a.sg; sc[t] = a.sc; first[t] = a.first; flag[t] = f;
  }
  __device__ __forceinline__ GtAgg load(int t) const {
    GtAgg a;
    const int2 c = cnt[t];
    a.n = c.x; a.ng = c.y;
    a.sm = sm[t]; a.sf = sf[t]; a.sr = sr[t]; a.mx = mx[t];
    a.sg = sg[t]; a.sc = sc[t]; a.first = first[t]; a.pad = 0;
    return a;
  }
};

// Inclusive segmented scan over the block's B elements (Hillis-Steele, a
// fixed shape): f = 1 starts a segment; on return a is the join of the
// elements from the element's segment start (or the block's first element)
// up to it, f tells whether a start lies in [0, t].
template <int B>
__device__ __forceinline__ void gt_seg_scan(GtLds<B>& L, GtAgg& a, int& f) {
  const int t = threadIdx.x;
  for (int off = 1; off < B; off <<= 1) {
    L.store(t, a, f);
    __syncthreads();
    if (t >= off) {
      if (!f) a = gt_join(L.load(t - off), a);
      f |= L.flag[t - off];
    }
    __syncthreads();
  }
}

// ---- sort keys + totals --------------------------------------------------
__global__ __launch_bounds__(256) void k_gt_init(const uint32_t* __restrict__ ctl, const uint64_t* __restrict__ gkey,
                                                 const int32_t* __restrict__ copied,
                                                 const int32_t* __restrict__ executed, int64_t n,
                                                 uint64_t* __restrict__ key, avgpu_genotype_totals* tot) {
  __shared__ long long s_red[3][4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  long long alive = 0, c = 0, e = 0;
  if (i < n) {
    const bool a = (ctl[i] & CTL_ALIVE) != 0;
    key[i] = (a ? gkey[i] : 0ull) - 1ull;
    if (a) { alive = 1; c = copied[i]; e = executed[i]; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    alive += __shfl_down(alive, off);
    c += __shfl_down(c, off);
    e += __shfl_down(e, off);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { s_red[0][wv] = alive; s_red[1][wv] = c; s_red[2][wv] = e; }
  __syncthreads();
  if (threadIdx.x < 3) {                // integer atomics: exact in any order
    const long long v = s_red[threadIdx.x][0] + s_red[threadIdx.x][1] + s_red[threadIdx.x][2] + s_red[threadIdx.x][3];
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(
        threadIdx.x == 0 ? &tot->num_organisms : threadIdx.x == 1 ? &tot->sum_copied_size : &tot->sum_executed_size);
    if (v) atomicAdd(dst, (unsigned long long)v);
  }
}

// ---- LSD radix sort, one 8-bit digit a pass ---------------------------------
// hist[d * nblk + b]: keys of tile b with digit d
__global__ __launch_bounds__(RS_THREADS) void k_gt_hist(const uint64_t* __restrict__ key, int64_t n, int shift,
                                                        uint32_t* __restrict__ hist, int nblk) {
  __shared__ uint32_t h[256];
  const int t = threadIdx.x;
  h[t] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * GT_SORT_TILE;
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; r++) {
    const int64_t i = base + r * RS_THREADS + t;
    if (i < n) atomicAdd(&h[(uint32_t)(key[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)t * nblk + blockIdx.x] = h[t];
}

// one wave per digit: hist row -> exclusive prefix over the tiles, dtot[d] = the digit's total
__global__ __launch_bounds__(64) void k_gt_scan(uint32_t* __restrict__ hist, int nblk, uint32_t* __restrict__ dtot) {
  const int lane = threadIdx.x;
  uint32_t* row = hist + (size_t)blockIdx.x * nblk;
  uint32_t run = 0;
  for (int b0 = 0; b0 < nblk; b0 += 64) {
    const int b = b0 + lane;
    const uint32_t v = b < nblk ? row[b] : 0u;
    uint32_t x = v;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (b < nblk) row[b] = run + x - v;
    run += __shfl(x, 63);
  }
  if (lane == 0) dtot[blockIdx.x] = run;
}

// Stable scatter of tile b.  The tile's keys are taken in (round, wave, lane)
// order = ascending position; a key's place is
//   (keys of smaller digits) + (same digit in earlier tiles)
//   + (same digit in earlier 64-key groups of this tile) + (same digit in lower lanes).
__global__ __launch_bounds__(RS_THREADS) void k_gt_scatter(const uint64_t* __restrict__ kin,
                                                           const int32_t* __restrict__ cin,
                                                           uint64_t* __restrict__ kout, int32_t* __restrict__ cout,
                                                           int64_t n, int shift, const uint32_t* __restrict__ hist,
                                                           int nblk, const uint32_t* __restrict__ dtot,
                                                           int first_pass) {
  __shared__ uint16_t cnt[RS_SLOTS][256];
  __shared__ uint32_t s_base[256];
  __shared__ uint32_t s_wt[RS_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  {
    uint32_t* z = reinterpret_cast<uint32_t*>(&cnt[0][0]);
    for (int k = t; k < RS_SLOTS * 256 / 2; k += RS_THREADS) z[k] = 0u;
  }
  // exclusive prefix of the digit totals (thread t = digit t)
  const uint32_t tot = dtot[t];
  uint32_t x = tot;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) s_wt[wv] = x;
  __syncthreads();
  uint32_t before = x - tot;
  for (int k = 0; k < wv; k++) before += s_wt[k];
  s_base[t] = before + hist[(size_t)t * nblk + blockIdx.x];

  const int64_t base = (int64_t)blockIdx.x * GT_SORT_TILE;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint64_t k[RS_ROUNDS];
  uint32_t rank[RS_ROUNDS];
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; r++) {
    const int64_t i = base + r * RS_THREADS + t;
    const bool valid = i < n;
    k[r] = valid ? kin[i] : 0ull;
    const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; bit++) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    rank[r] = (uint32_t)__popcll(peers & below);
    if (valid && rank[r] == 0) cnt[r * RS_WAVES + wv][d] = (uint16_t)__popcll(peers);
  }
  __syncthreads();
  {
    uint32_t run = 0;
#pragma unroll 8
    for (int s = 0; s < RS_SLOTS; s++) {
      const uint32_t c = cnt[s][t];
      cnt[s][t] = (uint16_t)run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; r++) {
    const int64_t i = base + r * RS_THREADS + t;
    if (i < n) {
      const uint32_t d = (uint32_t)(k[r] >> shift) & 255u;
      const uint32_t pos = s_base[d] + cnt[r * RS_WAVES + wv][d] + rank[r];
      kout[pos] = k[r];
      cout[pos] = first_pass ? (int32_t)i : cin[i];
    }
  }
}

// ---- segments -----------------------------------------------------------------
struct GtCells {            // the per-cell values of k_census (state.hip)
  const double* merit;
  const double* fitness;
  const int32_t* gest_time;
  const int32_t* copied;
  const int32_t* birth_len;
};

template <bool EMIT>
__global__ __launch_bounds__(GT_SEG_TILE) void k_gt_tiles(GtCells in, const uint64_t* __restrict__ key,
                                                          const int32_t* __restrict__ cell, int64_t n,
                                                          GtAgg* __restrict__ tile_agg, int32_t* __restrict__ tile_flag,
                                                          int32_t* __restrict__ tile_tails,
                                                          const GtAgg* __restrict__ carry,
                                                          const int64_t* __restrict__ row_off,
                                                          avgpu_genotype* __restrict__ out) {
  __shared__ GtLds<GT_SEG_TILE> L;
  __shared__ int s_wt[GT_SEG_TILE / 64];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * GT_SEG_TILE + t;
  uint64_t k = KEY_NONE, kp = KEY_NONE, kn = KEY_NONE;
  if (i < n) {
    k = key[i];
    if (i > 0) kp = key[i - 1];
    if (i + 1 < n) kn = key[i + 1];
  }
  const bool valid = k != KEY_NONE;
  // positions behind the genotypes are starts holding the identity: they
  // carry nothing into a later tile and end no segment
  int f = (!valid || kp != k) ? 1 : 0;
  const bool tail = valid && kn != k;
  GtAgg a = gt_identity();
  if (valid) {
    const int c = cell[i];
    a.n = 1;
    a.first = c;
    const int g = in.gest_time[c];
    if (g > 0) {
      const double fit = in.fitness[c];
      a.ng = 1;
      a.sm = in.merit[c]; a.sf = fit; a.sr = 1.0 / (double)g; a.mx = fit;
      a.sg = g; a.sc = in.copied[c];
    }
  }
  gt_seg_scan<GT_SEG_TILE>(L, a, f);
  if (!EMIT) {
    const int tails = __syncthreads_count(tail);
    if (t == GT_SEG_TILE - 1) { tile_agg[blockIdx.x] = a; tile_flag[blockIdx.x] = f; }
    if (t == 0) tile_tails[blockIdx.x] = tails;
  } else {
    const unsigned long long m = __ballot(tail);
    const int lane = t & 63, wv = t >> 6;
    if (lane == 0) s_wt[wv] = __popcll(m);
    __syncthreads();
    int r = __popcll(m & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; q++) r += s_wt[q];
    if (tail) {
      // no start in [tile begin, i]: the segment began in an earlier tile
      const GtAgg s = f ? a : gt_join(carry[blockIdx.x], a);
      avgpu_genotype g;
      g.genotype_key = k + 1ull;
      g.first_cell = s.first;
      g.num_units = s.n;
      g.genome_length = in.birth_len[s.first];
      g.num_gestated = s.ng;
      g.reserved = 0;
      g.sum_merit = s.sm; g.sum_fitness = s.sf; g.sum_repro_rate = s.sr;
      g.max_fitness = s.ng ? s.mx : 0.0;
      g.sum_gestation = s.sg; g.sum_copied = s.sc;
      out[row_off[blockIdx.x] + r] = g;
    }
  }
}

// One block.  carry[t]: the join of the open segment's parts in the tiles
// before t (what tile t's leading part continues); row_off[t]: segments ending
// before tile t.  Chunks of 512 tiles, ascending, the running carry joined in
// front of each.
__global__ __launch_bounds__(CARRY_THREADS) void k_gt_carry(const GtAgg* __restrict__ tile_agg,
                                                            const int32_t* __restrict__ tile_flag,
                                                            const int32_t* __restrict__ tile_tails, int64_t ntile,
                                                            GtAgg* __restrict__ carry, int64_t* __restrict__ row_off,
                                                            avgpu_genotype_totals* tot) {
  __shared__ GtLds<CARRY_THREADS> L;
  __shared__ long long s_cnt[CARRY_THREADS];
  const int t = threadIdx.x;
  GtAgg run = gt_identity();            // uniform over the block
  long long rows = 0;
  for (int64_t base = 0; base < ntile; base += CARRY_THREADS) {
    const int64_t tt = base + t;
    GtAgg a = gt_identity();
    int f = 1;
    long long nt = 0;
    if (tt < ntile) { a = tile_agg[tt]; f = tile_flag[tt]; nt = tile_tails[tt]; }
    gt_seg_scan<CARRY_THREADS>(L, a, f);
    L.store(t, a, f);
    long long x = nt;
    s_cnt[t] = x;
    __syncthreads();
    GtAgg cin = run;
    if (t > 0) {
      const GtAgg p = L.load(t - 1);
      cin = L.flag[t - 1] ? p : gt_join(run, p);
    }
    const GtAgg last = L.load(CARRY_THREADS - 1);
    run = L.flag[CARRY_THREADS - 1] ? last : gt_join(run, last);
    for (int off = 1; off < CARRY_THREADS; off <<= 1) {
      const long long y = t >= off ? s_cnt[t - off] : 0;
      __syncthreads();
      x += y;
      s_cnt[t] = x;
      __syncthreads();
    }
    if (tt < ntile) { carry[tt] = cin; row_off[tt] = rows + x - nt; }
    rows += s_cnt[CARRY_THREADS - 1];
    __syncthreads();
  }
  if (t == 0) tot->num_genotypes = rows;
}

GtCells cells_of(const DevWorld& W) {
  GtCells c;
  c.merit = W.merit; c.fitness = W.fitness; c.gest_time = W.gest_time;
  c.copied = W.copied; c.birth_len = W.birth_len;
  return c;
}

}  // namespace

// S.totals is zero on entry (stream order); on completion it holds the four
// totals and key[0] / cell[0] the sorted (key - 1, cell) pairs
void launch_genotype_group(const DevWorld& W, const GtScratch& S, hipStream_t s) {
  const int64_t n = S.n;
  k_gt_init<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(W.ctl, W.gkey, W.copied, W.executed, n, S.key[0], S.totals);
  const int nblk = (int)S.nblk;
  for (int p = 0; p < 8; p++) {
    const int a = p & 1, b = a ^ 1;
    k_gt_hist<<<nblk, RS_THREADS, 0, s>>>(S.key[a], n, 8 * p, S.hist, nblk);
    k_gt_scan<<<256, 64, 0, s>>>(S.hist, nblk, S.dtot);
    k_gt_scatter<<<nblk, RS_THREADS, 0, s>>>(S.key[a], S.cell[a], S.key[b], S.cell[b], n, 8 * p, S.hist, nblk,
                                             S.dtot, p == 0);
  }
  k_gt_tiles<false><<<(unsigned)S.ntile, GT_SEG_TILE, 0, s>>>(cells_of(W), S.key[0], S.cell[0], n, S.tile_agg,
                                                              S.tile_flag, S.tile_tails, nullptr, nullptr, nullptr);
  k_gt_carry<<<1, CARRY_THREADS, 0, s>>>(S.tile_agg, S.tile_flag, S.tile_tails, S.ntile, S.carry, S.row_off,
                                         S.totals);
}

// the same sort over the first m entries of key[0] (the arbiter's orderings,
// arbiter.hip): the payload is the entry's position before the sort
void launch_genotype_sort(const GtScratch& S, int64_t m, int passes, hipStream_t s) {
  const int nblk = (int)((m + GT_SORT_TILE - 1) / GT_SORT_TILE);
  for (int p = 0; p < passes; p++) {
    const int a = p & 1, b = a ^ 1;
    k_gt_hist<<<nblk, RS_THREADS, 0, s>>>(S.key[a], m, 8 * p, S.hist, nblk);
    k_gt_scan<<<256, 64, 0, s>>>(S.hist, nblk, S.dtot);
    k_gt_scatter<<<nblk, RS_THREADS, 0, s>>>(S.key[a], S.cell[a], S.key[b], S.cell[b], m, 8 * p, S.hist, nblk,
                                             S.dtot, p == 0);
  }
}

// after launch_genotype_group on the same stream: totals->num_genotypes rows into d_out
void launch_genotype_rows(const DevWorld& W, const GtScratch& S, avgpu_genotype* d_out, hipStream_t s) {
  k_gt_tiles<true><<<(unsigned)S.ntile, GT_SEG_TILE, 0, s>>>(cells_of(W), S.key[0], S.cell[0], S.n, S.tile_agg,
                                                             S.tile_flag, S.tile_tails, S.carry, S.row_off, d_out);
}
