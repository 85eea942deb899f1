// sched.hip -- the start of an update, before k_interpret:
//   k_merit_partial  deterministic total merit (scheduler input); block 0 also
//                    resets the update's counters and queue lengths
//   k_block_counts, k_tree_up, k_tree_down, k_allot  the scheduler (cScheduler
//                    restated): the update's picks split down a binary tree of
//                    the cells; budgets, class tags and lists, occupancy
//   k_window_order   the class-0 order: each window's cells sorted by budget
//   k_reset_counts, k_age_tick  the serial world's share of the above
// Paths are relative to avida-core/source/ of the reference.
#include "device.h"

#pragma clang fp contract(off)

namespace {

// ---- deterministic total merit: 256-cell blocks, fixed pairwise tree ----
// (strip tiles hold whole 256-cell blocks, so the block partials of a tiled
// world are the single world's partials; alive_d: alive counts as doubles
// after the merits, the layout tiles exchange)
// Before the shards are cleared, an update whose statistics were never asked
// for (lazy: run with out == NULL, CNT_CUM_FLAG still 0) has its counts added
// to the running sums here instead of in k_stats_final.  One block, >= 256
// threads; the caller's condition is block-uniform.
__device__ __forceinline__ void reset_queues_block(const DevWorld& W) {
  if (threadIdx.x < BQ_WORDS) W.b_count[threadIdx.x] = 0;
  if (threadIdx.x < CLASS_COUNT_WORDS) W.class_count[threadIdx.x] = 0;
}
__device__ __forceinline__ void reset_counts_block(const DevWorld& W) {
  constexpr int NG = 256 / CNT_STRIDE;
  __shared__ unsigned long long cs[NG][CNT_STRIDE];
  const bool fold = W.counters[CNT_CUM_FLAG] == 0ull;
  if (threadIdx.x < 256) {
    const int slot = threadIdx.x & (CNT_STRIDE - 1), g = threadIdx.x / CNT_STRIDE;
    unsigned long long a = 0;
    if (fold && slot != CNT_STRIDE - 1) {
      unsigned long long v[NSHARD / NG];         // all loads in flight together (this block is
#pragma unroll                                   // the launch's long pole: ~16 L2 round trips)
      for (int k = 0; k < NSHARD / NG; k++) v[k] = W.counters[(g + k * NG) * CNT_STRIDE + slot];
#pragma unroll
      for (int k = 0; k < NSHARD / NG; k++) a += v[k];
    }
    cs[g][slot] = a;
  }
  __syncthreads();
  if (threadIdx.x < CNT_STRIDE) {
    unsigned long long t = 0;
    for (int g = 0; g < NG; g++) t += cs[g][threadIdx.x];
    if (threadIdx.x == CNT_STRIDE - 1) W.counters[CNT_CUM_FLAG] = 0ull;
    else if (t) W.counters[CNT_CUM_BASE + threadIdx.x] += t;
  }
  for (int i = threadIdx.x; i < NSHARD * CNT_STRIDE; i += blockDim.x) W.counters[i] = 0ull;
  if (threadIdx.x < BQ_WORDS) W.b_count[threadIdx.x] = 0;
  if (threadIdx.x < CLASS_COUNT_WORDS) W.class_count[threadIdx.x] = 0;
}

// RESET_COUNTS: block 0 also zeroes the update's counters, birth-queue and class-list
// lengths (k_reset_counts' work; the previous update's statistics have read them);
// RESET_QUEUES (a later sub-update): the queue and list lengths only, the counters
// go on adding up the update
// One wave per 256-cell block b (partial[b]): the pairwise tree of strides
// 128, 64, ..., 1 (s[t] += s[t + stride]), the oracle's tree_merit_sum order.
// Lane l loads cells l, l+64, l+128, l+192 and forms the stride-128 and -64
// sums itself; strides 32 .. 1 are lane shuffles -- the same additions in the
// same order, without the LDS tree's 8 barriers.  Four blocks per workgroup.
__global__ __launch_bounds__(256) void k_merit_partial(DevWorld W, double* partial, int32_t* alive_partial,
                                                       double* alive_d, int reset) {
  if (reset == RESET_COUNTS && blockIdx.x == 0) reset_counts_block(W);
  if (reset == RESET_QUEUES && blockIdx.x == 0) reset_queues_block(W);
  // a strip's partials end with its last step's predictor, pick carry and
  // divide counts by quarter (the TAIL_* words; the oracle's orc_tile_partials;
  // summed on every strip after the gather)
  if (alive_d && blockIdx.x == 0 && threadIdx.x < TAIL_WORDS) {
    const int64_t nbl = (W.n + 255) / 256;
    const long long v = threadIdx.x == TAIL_PRED ? pacc_sum(W, PACC_WEIGHT)
                        : (threadIdx.x == TAIL_CARRY ? W.sched[SCHED_CARRY]
                                                     : quarter_count(W, (int)threadIdx.x - TAIL_QUARTER0));
    partial[tile_tail_off(nbl) + threadIdx.x] = __longlong_as_double(v);
  }
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nb = (W.n + 255) / 256;
  if (b >= nb) return;
  double m[4];
  int a = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t c = b * 256 + lane + 64 * k;
    const uint32_t ctl = c < W.n ? W.ctl[c] : 0u;
    const bool live = (ctl & CTL_ALIVE) != 0;
    m[k] = live ? sched_weight(W.merit[c], ctl) : 0.0;   // the scheduler weight (oracle block_levels)
    a += live ? 1 : 0;
  }
  double z = __dadd_rn(__dadd_rn(m[0], m[2]), __dadd_rn(m[1], m[3]));
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_down(z, off);
    z = __dadd_rn(z, o);                       // lanes < off hold the tree's s[t]
    a += __shfl_down(a, off);
  }
  if (lane == 0) {
    partial[b] = z;
    if (alive_partial) alive_partial[b] = a;
    if (alive_d) alive_d[b] = (double)a;
  }
}

// ---- the scheduler: PROBABILISTIC slicing as the reference's picks ----
// (oracle/oracle.cc block_levels / top_tree / block_split) The
// update's UD = AVE_TIME_SLICE x N picks are split down a fixed binary tree
// with a Binomial at every node: the top tree over the 256-cell blocks'
// partials (k_block_counts, one workgroup), then each block's stride tree
// down to its cells (k_allot).
//
// k_block_counts: heap-ordered top tree in scr (node h = (1 << l) + i,
// children 2h, 2h + 1; leaves at P + block, zero-padded to P = 2^L), built
// bottom up, split top down in cnt.  BC_OWN: this world's partials
// (part doubles, alive int32); BC_GATHERED: a strip's gathered vector (tile
// k's block j at gathered[k * tile_part_stride(nb) + j], its alive count nb
// after); BC_HANDED_IN: this world's partials with the totals of every world
// handed in (TOT_WEIGHT, TOT_ORGS: cMultiProcessWorld::CalculateUpdateSize,
// main/cMultiProcessWorld.cc:396-405 -- this world's picks = (int)((local /
// total) * AVE_TIME_SLICE * N_total)); BC_TOTALS_ONLY: TOT_WEIGHT = root and
// TOT_ORGS = N out, nothing else written.  The other modes also leave TOT_DIV
// = the weight total INTEGRATED divides by and TOT_UD = UD.
// The whole tree is in the workgroup's LDS (P <= TREE_LDS_P: 2 x 4096 doubles
// + counts = 128 KiB of gfx950's 160).  A larger tree (strips of a world of
// more than 4096 blocks: the weak-scaling bench at N >= 2, configs[3]) is
// cut at the level of its 4096-block subtrees ("chunks"): k_tree_up builds
// every chunk's sums (a workgroup each), k_block_counts runs the tree above
// the chunk roots (chunked = 1: its leaves are the chunk roots, its output
// the chunk roots' counts), k_tree_down splits each chunk over this world's
// blocks (a workgroup each).  The same pairwise sums, the same draws at the
// same heap nodes: the same counts as one tree (oracle top_tree).  (One
// workgroup over a 65536-block tree in global memory took 124 us.)
#define TREE_LDS_P 4096
#define TREE_C_LOG 12

// leaf g of the block level (0 past the blocks); alive count into a
__device__ __forceinline__ double tree_leaf(const double* part, const int32_t* alive_part, int64_t nb, int64_t nbt,
                                            int mode, int64_t g, long long& a) {
  if (g >= nbt) return 0.0;
  if (mode == BC_GATHERED) {
    const int64_t k = g / nb, j = g - k * nb;
    a += (long long)part[k * tile_part_stride(nb) + nb + j];
    return part[k * tile_part_stride(nb) + j];
  }
  a += alive_part[g];
  return part[g];
}
__global__ __launch_bounds__(1024) void k_block_counts(DevWorld W, const double* part, const int32_t* alive_part,
                                                       int64_t nb, int ntiles, int L, double* totals,
                                                       uint32_t update, int mode, int chunked, int sub,
                                                       int nsub) {
  __shared__ long long s_cnt[1024];
  __shared__ double scr[2 * TREE_LDS_P];
  __shared__ long long cnt[2 * TREE_LDS_P];
  const int tid = threadIdx.x;
  const int64_t P = (int64_t)1 << L, nbt = mode == BC_GATHERED ? nb * ntiles : nb;
  long long a = 0;
  for (int64_t g = tid; g < P; g += 1024) {
    double v;
    if (chunked) {                              // the chunk roots of k_tree_up
      v = W.tree_scr[g];
      a += W.tree_cnt[g];
    } else {
      v = tree_leaf(part, alive_part, nb, nbt, mode, g, a);
    }
    scr[P + g] = v;
  }
  s_cnt[tid] = a;
  __syncthreads();
  for (int st = 512; st >= 1; st >>= 1) {      // living organisms (integer: any order)
    if (tid < st) s_cnt[tid] += s_cnt[tid + st];
    __syncthreads();
  }
  for (int l = L - 1; l >= 0; l--) {
    const int64_t w0 = (int64_t)1 << l;
    for (int64_t i = tid; i < w0; i += 1024) scr[w0 + i] = __dadd_rn(scr[2 * (w0 + i)], scr[2 * (w0 + i) + 1]);
    __syncthreads();
  }
  if (tid == 0) {
    const long long n = s_cnt[0];
    const double root = scr[1];
    const double ave = (double)W.ave_time_slice;
    // the update's UD = AVE_TIME_SLICE x the organisms at its start
    // (cAvidaDriver's update loop; SCHED_UD), a step's share of that
    if (sub == 0 && mode != BC_HANDED_IN) W.sched[SCHED_UD] = (long long)W.ave_time_slice * n;
    long long nroot = sub_share(W.sched[SCHED_UD], sub, nsub);
    if (mode == BC_HANDED_IN) {
      const double tot = totals[TOT_WEIGHT];
      nroot = tot > 0.0 ? (long long)__dmul_rn(__dmul_rn(__ddiv_rn(root, tot), ave), totals[TOT_ORGS]) : 0;
      totals[TOT_DIV] = tot;
      totals[TOT_UD] = __dmul_rn(ave, totals[TOT_ORGS]);
    } else {
      totals[TOT_WEIGHT] = root;
      totals[TOT_ORGS] = (double)n;
      if (mode != BC_TOTALS_ONLY) {   // (a caller's buffer ends after TOT_HANDED slots)
        totals[TOT_DIV] = root;
        totals[TOT_UD] = (double)W.sched[SCHED_UD];
      }
    }
    if (mode != BC_TOTALS_ONLY) {
      // the picks the last steps' newborns ran beyond their victims'
      // leftovers come out of an update's first step (oracle take_carry): a
      // strip sums every strip's carry from the gathered partials
      long long fresh = W.sched[SCHED_CARRY];
      if (mode == BC_GATHERED) {
        fresh = 0;
        for (int k = 0; k < ntiles; k++)
          fresh += __double_as_longlong(part[k * tile_part_stride(nb) + tile_tail_off(nb) + TAIL_CARRY]);
      }
      long long rem = W.sched[SCHED_CARRY_REM] + fresh;
      if (sub == 0) {
        const long long take = min(max(rem, -nroot), nroot);
        rem -= take;
        nroot -= take;
      }
      W.sched[SCHED_CARRY] = 0;
      W.sched[SCHED_CARRY_REM] = rem;
      count_add(W, AVGPU_CNT_STEPS, 1ull);
    }
    cnt[1] = nroot;
  }
  __syncthreads();
  if (mode == BC_TOTALS_ONLY) return;
  for (int i = tid; i < NSHARD * PACC_STRIDE; i += 1024) W.pacc[i] = 0;   // this step's predictor (interp_core.h pred_term)
  // top down, only the nodes over this world's blocks [b0, b0 + nloc) (a
  // node's count depends on its ancestors' alone): a strip of T splits its
  // own subtree and the path to it, not the whole gathered world's tree
  // (chunked: the leaves are chunks, the range in chunks)
  const int sh = chunked ? TREE_C_LOG : 0;
  const int64_t b0 = mode == BC_GATHERED ? W.cell0 / 256 : 0;
  const int64_t nloc = (W.n + 255) / 256;
  const int64_t lo = b0 >> sh, hi = (b0 + nloc - 1) >> sh;
  for (int l = 0; l < L; l++) {
    const int64_t w0 = (int64_t)1 << l;
    const int64_t ilo = lo >> (L - l), ihi = hi >> (L - l);
    for (int64_t i = ilo + tid; i <= ihi; i += 1024) {
      const int64_t h = w0 + i;
      const long long n = cnt[h];
      const long long left = binom_draw(n, __ddiv_rn(scr[2 * h], scr[h]),
                                        node_draw(W.seed_lo, W.seed_hi, update, SALT_TOP, (uint64_t)h));
      cnt[2 * h] = left;
      cnt[2 * h + 1] = n - left;
    }
    __syncthreads();
  }
  if (chunked) {
    for (int64_t j = lo + tid; j <= hi; j += 1024) W.tree_cnt[P + j] = cnt[P + j];
  } else {
    for (int64_t j = tid; j < nloc; j += 1024) W.blk_count[j] = cnt[P + b0 + j];
  }
}

// a chunk's subtree sums in LDS (t[1 .. 2 C), leaves at C + i), its alive count
__device__ __forceinline__ long long chunk_sums(double* t, long long* s_cnt, const double* part,
                                                const int32_t* alive_part, int64_t nb, int64_t nbt, int mode,
                                                int64_t k) {
  constexpr int C = 1 << TREE_C_LOG;
  const int tid = threadIdx.x;
  long long a = 0;
  for (int i = tid; i < C; i += 1024) t[C + i] = tree_leaf(part, alive_part, nb, nbt, mode, k * C + i, a);
  s_cnt[tid] = a;
  __syncthreads();
  for (int st = 512; st >= 1; st >>= 1) {
    if (tid < st) s_cnt[tid] += s_cnt[tid + st];
    __syncthreads();
  }
  for (int l = TREE_C_LOG - 1; l >= 0; l--) {
    const int w0 = 1 << l;
    for (int i = tid; i < w0; i += 1024) t[w0 + i] = __dadd_rn(t[2 * (w0 + i)], t[2 * (w0 + i) + 1]);
    __syncthreads();
  }
  return s_cnt[0];
}
// chunk k = blockIdx.x: its root's sum -> tree_scr[k], its organisms -> tree_cnt[k]
__global__ __launch_bounds__(1024) void k_tree_up(DevWorld W, const double* part, const int32_t* alive_part,
                                                  int64_t nb, int ntiles, int mode) {
  __shared__ double t[2 << TREE_C_LOG];
  __shared__ long long s_cnt[1024];
  const int64_t nbt = mode == BC_GATHERED ? nb * ntiles : nb;
  const long long a = chunk_sums(t, s_cnt, part, alive_part, nb, nbt, mode, blockIdx.x);
  if (threadIdx.x == 0) {
    W.tree_scr[blockIdx.x] = t[1];
    W.tree_cnt[blockIdx.x] = a;
  }
}
// chunk k = k0 + blockIdx.x of this world's range: its count (tree_cnt[K + k],
// k_block_counts chunked) split down its subtree over this world's blocks;
// node i of local level l is heap node (K + k) 2^l + i
__global__ __launch_bounds__(1024) void k_tree_down(DevWorld W, const double* part, const int32_t* alive_part,
                                                    int64_t nb, int ntiles, int mode, int64_t K, uint32_t update) {
  constexpr int C = 1 << TREE_C_LOG;
  __shared__ double t[2 * C];
  __shared__ long long c[2 * C];
  __shared__ long long s_cnt[1024];
  const int tid = threadIdx.x;
  const int64_t nbt = mode == BC_GATHERED ? nb * ntiles : nb;
  const int64_t b0 = mode == BC_GATHERED ? W.cell0 / 256 : 0;
  const int64_t nloc = (W.n + 255) / 256;
  const int64_t k = (b0 >> TREE_C_LOG) + blockIdx.x;
  chunk_sums(t, s_cnt, part, alive_part, nb, nbt, mode, k);
  if (tid == 0) c[1] = W.tree_cnt[K + k];
  __syncthreads();
  // this world's blocks inside the chunk: local leaves [lo, hi]
  const int64_t g0 = k * C;
  const int lo = (int)(max(b0, g0) - g0), hi = (int)(min(b0 + nloc, g0 + C) - 1 - g0);
  for (int l = 0; l < TREE_C_LOG; l++) {
    const int w0 = 1 << l;
    const int ilo = lo >> (TREE_C_LOG - l), ihi = hi >> (TREE_C_LOG - l);
    for (int i = ilo + tid; i <= ihi; i += 1024) {
      const int h = w0 + i;
      const long long n = c[h];
      const uint64_t H = (uint64_t)(K + k) * (uint64_t)w0 + (uint64_t)i;
      const long long left = binom_draw(n, __ddiv_rn(t[2 * h], t[h]),
                                        node_draw(W.seed_lo, W.seed_hi, update, SALT_TOP, H));
      c[2 * h] = left;
      c[2 * h + 1] = n - left;
    }
    __syncthreads();
  }
  for (int i = lo + tid; i <= hi; i += 1024) W.blk_count[g0 + i - b0] = c[C + i];
}

__device__ __forceinline__ void occ_init_cell(const DevWorld& W, int64_t c) {
  W.occ[c] = (c < W.n && (W.ctl[c] & CTL_ALIVE)) ? 1 : 0;
  W.owner[c] = -1;
}

// k_allot's cells into their size-class lists (rows 1..3; class 0 is swept
// densely), as state.hip's enqueue_class but for CPT cells per thread
// (cells[j], j-major order inside the block): one global atomic per class and
// block for all of them, the waves' offsets in wave order.  blockDim.x = 64 * WAVES.
template <int WAVES, int CPT>
__device__ __forceinline__ void enqueue_class_multi(const DevWorld& W, const int* cell, const bool* want,
                                                    const int* cls) {
  __shared__ int s_pc[NUM_CLASSES][WAVES], s_base[NUM_CLASSES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long masks[NUM_CLASSES][CPT];
  __syncthreads();                             // s_pc / s_base free (repeat calls)
#pragma unroll
  for (int k = 1; k < NUM_CLASSES; k++) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < CPT; j++) {
      masks[k][j] = __ballot(want[j] && cls[j] == k);
      n += __popcll(masks[k][j]);
    }
    if (lane == 0) s_pc[k][wv] = n;
  }
  __syncthreads();
  if (threadIdx.x > 0 && threadIdx.x < NUM_CLASSES) {
    const int k = threadIdx.x;
    int tot = 0;
    for (int w = 0; w < WAVES; w++) tot += s_pc[k][w];
    s_base[k] = tot ? atomicAdd(&W.class_count[k], tot) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 1; k < NUM_CLASSES; k++) {
    int woff = 0;
    for (int w = 0; w < wv; w++) woff += s_pc[k][w];
    int jbase = 0;
#pragma unroll
    for (int j = 0; j < CPT; j++) {
      if (want[j] && cls[j] == k) {
        const int rank = __popcll(masks[k][j] & ((1ull << lane) - 1ull));
        W.class_list[(int64_t)k * W.n + s_base[k] + woff + jbase + rank] = cell[j];
      }
      jbase += __popcll(masks[k][j]);
    }
  }
}

// a cell's bucket of the class-0 order: class-0 slices by budget, descending
// (clamped both ways: a bucket outside the histogram would place the cell
// outside its window of W.order), every other cell in the last bucket
__device__ __forceinline__ int window_bucket(bool c0, int budget) {
  return c0 ? SORT_BUCKETS - 2 - min(max(budget, 0), SORT_BUCKETS - 2) : SORT_BUCKETS - 1;
}
// k_allot: one wave per 256-cell block, 16 blocks per workgroup.  Lane l
// holds cells l, l + 64, l + 128, l + 192.  The block's stride tree over its
// cells' weights (node (k, t) = the cells = t mod 2^k, the additions of
// k_merit_partial): levels 7 and 6 in the lane, levels 5..0 by shuffles; then
// its count blk_count[b] split top down (PROBABILISTIC): levels 0..5 across
// the lanes (lane t holds node (k, t), the right child's count goes to lane
// t + 2^k by shuffle), levels 6 and 7 in the lane -- no barrier, no LDS.
// INTEGRATED: lambda = UD * weight / total with a credit carry; CONSTANT (or
// no weight at all): AVE_TIME_SLICE.  Each cell's head start is consumed here.
// Also the cell's budget and class tag, the placement occupancy of this
// update (living cells occupied; an organism that dies in its slice clears
// its cell at write-back), its kill time, the previous update's round-3
// claim, and the class lists.
__global__ __launch_bounds__(1024) void k_allot(DevWorld W, const double* totals, uint32_t update, int tick) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 6);
  const int64_t nb = (W.n + 255) / 256;
  const double total = totals[TOT_DIV];
  const bool consts = W.slicing == AVGPU_SLICE_CONSTANT || !(total > 0.0);
  const bool prob = !consts && W.slicing != AVGPU_SLICE_INTEGRATED;
  uint32_t ctl[4];
  double wt[4];
  bool alive[4];
  int msz[4];                                  // loaded ahead of the tree (the class needs it)
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int64_t c = b * 256 + lane + 64 * j;
    ctl[j] = (b < nb && c < W.n) ? W.ctl[c] : 0u;
    alive[j] = (ctl[j] & CTL_ALIVE) != 0;
    msz[j] = alive[j] ? W.mem_size[c] : 0;
    const double m = alive[j] ? W.merit[c] : 0.0;
    if (alive[j] && !merit_ok(m)) count_add(W, AVGPU_CNT_BAD_RECORD, 1ull);   // counted; sched_weight gives it 0
    wt[j] = alive[j] ? sched_weight(m, ctl[j]) : 0.0;
  }
  long long cnt[4] = {0, 0, 0, 0};
  if (prob && b < nb) {                        // wave-uniform
    const uint64_t gb = (uint64_t)(W.cell0 / 256 + b);
    const uint32_t slo = W.seed_lo, shi = W.seed_hi;
    // bottom up: L7[l] = x[l] + x[l+128], L7[l+64] = x[l+64] + x[l+192], L6[l] = L7[l] + L7[l+64]
    const double l7a = __dadd_rn(wt[0], wt[2]), l7b = __dadd_rn(wt[1], wt[3]);
    const double l6 = __dadd_rn(l7a, l7b);
    double lv[7];                                // lv[k] = L_k[lane] (k = 0..6; lanes >= 2^k: unused)
    lv[6] = l6;
#pragma unroll
    for (int k = 5; k >= 0; k--) {
      const double o = __shfl_down(lv[k + 1], 1 << k);
      lv[k] = __dadd_rn(lv[k + 1], o);
    }
    // top down: lane t < 2^k holds count(k, t)
    long long c = lane == 0 ? (long long)W.blk_count[b] : 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      long long left = 0;
      const bool act = lane < (1 << k);
      if (act)
        left = binom_draw(c, __ddiv_rn(lv[k + 1], lv[k]),
                          node_draw(slo, shi, update, SALT_BLOCK, (gb << 9) | (uint64_t)((1 << k) + lane)));
      const long long right = c - left;
      const long long got = __shfl_up(right, 1 << k);   // lane t + 2^k takes node (k, t)'s right child
      if (act) c = left;
      else if (lane < (2 << k)) c = got;
    }
    // level 6 (node (6, l) -> (7, l), (7, l + 64)) and level 7 (-> the cells)
    const long long l6l = binom_draw(c, __ddiv_rn(l7a, l6),
                                     node_draw(slo, shi, update, SALT_BLOCK, (gb << 9) | (uint64_t)(64 + lane)));
    const long long c7a = l6l, c7b = c - l6l;
    const long long x0 = binom_draw(c7a, __ddiv_rn(wt[0], l7a),
                                    node_draw(slo, shi, update, SALT_BLOCK, (gb << 9) | (uint64_t)(128 + lane)));
    const long long x1 = binom_draw(c7b, __ddiv_rn(wt[1], l7b),
                                    node_draw(slo, shi, update, SALT_BLOCK, (gb << 9) | (uint64_t)(192 + lane)));
    cnt[0] = x0; cnt[2] = c7a - x0; cnt[1] = x1; cnt[3] = c7b - x1;
  }
  bool want[4] = {false, false, false, false};
  int cls[4] = {0, 0, 0, 0}, buds[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int64_t c = b * 256 + lane + 64 * j;
    if (b >= nb || c >= W.n) continue;
    int bud = 0;
    if (alive[j]) {
      if (consts) {
        bud = W.ave_time_slice;
      } else if (prob) {
        bud = (int)min(cnt[j], (long long)(BUDGET_PRIM - 1));   // budgets are < 2^30 (device.h)
      } else {
        double lam = __ddiv_rn(__dmul_rn(totals[TOT_UD], wt[j]), total);
        if (lam > 1.0e8) lam = 1.0e8;
        const double cr = __dadd_rn(W.credit[c], lam);
        const double fl = floor(cr);
        bud = (int)fl;
        W.credit[c] = __dsub_rn(cr, fl);
      }
      if (ctl[j] & CTL_HS_MASK) W.ctl[c] = ctl[j] & ~CTL_HS_MASK;   // the head start is used up
      if (tick && W.track_age) W.age[c] += 1;   // cPhenotype::IncAge at the previous update's end (oracle age_tick)
      want[j] = bud > 0;
      if (want[j]) cls[j] = class_of(need_of(msz[j], ctl[j], W.size_range));   // need_of_cell
    }
    buds[j] = bud;
    W.budget[c] = bud;
    W.aclass[c] = want[j] ? (uint8_t)cls[j] : (uint8_t)ACLASS_NONE;
    W.ran[c] = 0;
    if (W.env_resources)
      for (int r = 0; r < W.n_res; r++) W.cons[(int64_t)r * W.n + c] = 0.0;
    occ_init_cell(W, c);
    W.killt[c] = 0u;
    W.claim_r[3][c] = 0ull;   // the previous update's round-3 claims (k_activate read them last)
  }
  unsigned long long ns = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) ns += (unsigned long long)__popcll(__ballot(want[j]));
  if (lane == 0 && ns) count_add(W, AVGPU_CNT_SLICES, ns);
  int cells[4];
#pragma unroll
  for (int j = 0; j < 4; j++) cells[j] = (int)(b * 256 + lane + 64 * j);
  enqueue_class_multi<16, 4>(W, cells, want, cls);
  // this 4096-cell sub-window's histogram of the class-0 order's buckets
  // (k_window_order; the bucket rule of window_bucket)
  __shared__ int sh[SORT_BUCKETS];
  for (int i = threadIdx.x; i < SORT_BUCKETS; i += 1024) sh[i] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int64_t c = b * 256 + lane + 64 * j;
    if (b < nb && c < W.n) atomicAdd(&sh[window_bucket(want[j] && cls[j] == 0, buds[j])], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SORT_BUCKETS; i += 1024) W.sub_hist[(int64_t)blockIdx.x * SORT_BUCKETS + i] = sh[i];
}

// exclusive scan of the SORT_BUCKETS counts in h, in place, by one wave
__device__ __forceinline__ void bucket_scan(int* h) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    constexpr int PER = (SORT_BUCKETS + 63) / 64;
    int loc[PER], t = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int i = tid * PER + k;
      loc[k] = i < SORT_BUCKETS ? h[i] : 0;
      t += loc[k];
    }
    int incl = t;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off);
      if (tid >= off) incl += o;
    }
    int run = incl - t;
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const int i = tid * PER + k;
      if (i < SORT_BUCKETS) h[i] = run;
      run += loc[k];
    }
  }
}

// The class-0 order: each SORT_WIN window's class-0 cells by budget
// (descending), a counting sort.  Which cell runs in which wave changes no
// organism's result (per-organism streams, placement by birth time and key),
// it only groups similar slices, so the order inside a budget is free (LDS
// atomics).  A wave loses about (window's budget range) / (2 x its waves) per
// lane to the spread of its budgets: 8192-cell windows (128 waves) took the
// lane efficiency of the multinomial budgets from 0.94 to 0.98
// (tools/budget_spread.py), 32768 cells measured fastest (HISTORY.md,
// profiles/r04w_ab.txt).
// One 1024-thread block per 4096-cell sub-window (the blocks of k_allot,
// which left each sub-window's bucket histogram in sub_hist): the window's
// bucket starts plus the counts of its earlier sub-windows, then this
// sub-window's cells by LDS atomics.  (One block per 32768-cell window, all
// of its 32768 LDS atomics on ~25 busy buckets, took 33 us: the list classes
// used that as their head start before they ran inside class 0's launch.)
__global__ __launch_bounds__(1024) void k_window_order(DevWorld W) {
  constexpr int SUBS = SORT_WIN / 4096;
  __shared__ int start[SORT_BUCKETS];
  const int tid = threadIdx.x;
  const int64_t sub = blockIdx.x;
  const int64_t s0 = (sub / SUBS) * SUBS, nsub = (W.n + 4095) / 4096;
  int before = 0;
  if (tid < SORT_BUCKETS) {
    int tot = 0;
    for (int64_t k = s0; k < s0 + SUBS && k < nsub; k++) {
      const int v = W.sub_hist[k * SORT_BUCKETS + tid];
      tot += v;
      if (k < sub) before += v;
    }
    start[tid] = tot;
  }
  __syncthreads();
  bucket_scan(start);
  __syncthreads();
  if (tid < SORT_BUCKETS) start[tid] += before;
  __syncthreads();
  const int64_t wbase = (sub / SUBS) * SORT_WIN;
#pragma unroll
  for (int h = 0; h < 4; h++) {
    const int64_t c = sub * 4096 + h * 1024 + tid;
    if (c < W.n) {
      const int pos = atomicAdd(&start[window_bucket(W.aclass[c] == 0, W.budget[c])], 1);
      W.order[wbase + pos] = (int32_t)c;
    }
  }
}

}  // namespace

// ---- two kernels outside the allotment (their names are external) ----
// the update's counters, birth-queue and class-list lengths, zeroed by one
// launch instead of three fill packets (~10 us each on the queue)
__global__ __launch_bounds__(256) void k_reset_counts(DevWorld W) { reset_counts_block(W); }

// the serial world's cPhenotype::IncAge tick (k_allot's, for the batch update)
__global__ void k_age_tick(DevWorld W) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < W.n && W.track_age && (W.ctl[c] & CTL_ALIVE)) W.age[c] += 1;
}

// ---------------------------------------------------------------------------
static void launch_block_counts(const DevWorld& W, hipStream_t s, const double* part, const int32_t* alive,
                                int64_t nb, int ntiles, int L, double* totals, uint32_t update, int mode,
                                int sub = 0, int nsub = 1) {
  if (((int64_t)1 << L) <= TREE_LDS_P) {
    hipLaunchKernelGGL(k_block_counts, dim3(1), dim3(1024), 0, s, W, part, alive, nb, ntiles, L, totals, update,
                       mode, 0, sub, nsub);
    return;
  }
  const int Lt = L - TREE_C_LOG;
  const int64_t K = (int64_t)1 << Lt;
  hipLaunchKernelGGL(k_tree_up, dim3((unsigned)K), dim3(1024), 0, s, W, part, alive, nb, ntiles, mode);
  // the K chunk roots' tree in LDS: K <= 4096 for any world of < 2^31 cells
  // (2^23 blocks at most, so K <= 2^11)
  hipLaunchKernelGGL(k_block_counts, dim3(1), dim3(1024), 0, s, W, part, alive, nb, ntiles, Lt, totals,
                     update, mode, 1, sub, nsub);
  if (mode == BC_TOTALS_ONLY) return;
  const int64_t b0 = mode == BC_GATHERED ? W.cell0 / 256 : 0, nloc = (W.n + 255) / 256;
  const int64_t nk = ((b0 + nloc - 1) >> TREE_C_LOG) - (b0 >> TREE_C_LOG) + 1;
  hipLaunchKernelGGL(k_tree_down, dim3((unsigned)nk), dim3(1024), 0, s, W, part, alive, nb, ntiles, mode, K, update);
}

static int tree_levels(int64_t nbt) {
  int L = 0;
  while (((int64_t)1 << L) < nbt) L++;
  return L;
}

// totals: TOT_WEIGHT and TOT_ORGS, a buffer of TOT_HANDED doubles
// (k_block_counts BC_TOTALS_ONLY).
// scratch: (n+255)/256 doubles + as many int32 partials
void launch_merit_total(const DevWorld& W, hipStream_t s, double* totals, double* scratch) {
  const int64_t nb = (W.n + 255) / 256;
  int32_t* alive_partial = reinterpret_cast<int32_t*>(scratch + nb);
  hipLaunchKernelGGL(k_merit_partial, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, W, scratch, alive_partial,
                     (double*)nullptr, RESET_NONE);
  launch_block_counts(W, s, scratch, alive_partial, nb, 1, tree_levels(nb), totals, 0u, BC_TOTALS_ONLY);
}

// the allotment of a world whose block counts are in W.blk_count: budgets,
// class lists, occupancy; then the class-0 order
static void launch_allot(const DevWorld& W, hipStream_t s, const double* totals, uint32_t update, int tick) {
  // (16 blocks per workgroup: the class lists take one global atomic per
  // class and 4096 cells -- with 1024-cell workgroups those atomics on three
  // addresses serialised to ~50 us per update, profiles/r04c_tail_per_update.txt)
  hipLaunchKernelGGL(k_allot, dim3(nblk(W.n, 4096)), dim3(1024), 0, s, W, totals, update, tick);
  hipLaunchKernelGGL(k_window_order, dim3(nblk(W.n, 4096)), dim3(1024), 0, s, W);
}

// single world: block partials (k_merit_partial also zeroes the update's
// counters), the scheduler's top tree, the allotment, the class-0 order.
// The picks come from the world's own totals (k_block_counts BC_OWN) or from
// totals handed in (BC_HANDED_IN; device.h)
void launch_world_begin(const DevWorld& W, hipStream_t s, double* totals, double* scratch, uint32_t update,
                        int sub, int nsub, bool own_totals) {
  const int64_t nb = (W.n + 255) / 256;
  int32_t* alive_partial = reinterpret_cast<int32_t*>(scratch + nb);
  if (sub == 0) launch_resources_begin(W, s);   // ProcessPreUpdate + the update's first DoUpdates
  hipLaunchKernelGGL(k_merit_partial, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, W, scratch, alive_partial,
                     (double*)nullptr, sub == 0 ? RESET_COUNTS : RESET_QUEUES);
  launch_block_counts(W, s, scratch, alive_partial, nb, 1, tree_levels(nb), totals, update,
                      own_totals ? BC_OWN : BC_HANDED_IN, sub, nsub);
  launch_allot(W, s, totals, update, sub == 0 ? 1 : 0);
}

// a strip tile: the top tree over every strip's gathered partials (BC_GATHERED),
// then the allotment (its partials' launch cleared the counters)
void launch_tile_pre(const DevWorld& W, hipStream_t s, const double* gathered, int ntiles, double* totals,
                     uint32_t update, int sub, int nsub) {
  const int64_t nb = (W.n + 255) / 256;
  if (sub == 0) launch_resources_begin(W, s);
  launch_block_counts(W, s, gathered, nullptr, nb, ntiles, tree_levels(nb * ntiles), totals, update, BC_GATHERED, sub,
                      nsub);
  launch_allot(W, s, totals, update, sub == 0 ? 1 : 0);
}

// (a strip tile's partials start its update: block 0 also clears the counters)
void launch_tile_partials(const DevWorld& W, hipStream_t s, double* out, int reset) {
  const int64_t nb = (W.n + 255) / 256;
  hipLaunchKernelGGL(k_merit_partial, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, W, out, (int32_t*)nullptr,
                     out + nb, reset);
}

void launch_age_tick(const DevWorld& W, hipStream_t s) {
  hipLaunchKernelGGL(k_age_tick, dim3(nblk(W.n, 256)), dim3(256), 0, s, W);
}

void launch_reset_counts(const DevWorld& W, hipStream_t s) {
  hipLaunchKernelGGL(k_reset_counts, dim3(1), dim3(256), 0, s, W);
}
