// popevents.hip -- population events decided on the device:
//   k_ev_kill_cells   a list of cells (a loop of cPopulation::KillOrganism)
//   k_ev_kill_prob    every living cell with u < p (KillProb / KillRate, actions/PopulationActions.cc:1166-1187),
//                     optionally only the cells of listed genotypes (KillDominantGenotype :1226-1258,
//                     KillProbSequence :1261-1299, the "ignore deads" leg of SerialTransfer)
//   k_ev_kill_rect    a rectangle of the torus (KillRectangle :1754-1815)
//   k_ev_hist, k_ev_pick, k_ev_kill_above   a uniform sample of `keep` survivors (cPopulation::SerialTransfer,
//                     main/cPopulation.cc:7553-7585; ApplyBottleneck, actions/PopulationActions.cc:1195-1224)
// A killed cell loses CTL_ALIVE and nothing else, as avgpu_kill leaves it.  The
// draws are event_draw (device.h): no organism's stream moves.  The scans own
// their cells (one thread per four consecutive control words, a 16-B load and
// store where the words are aligned), so they clear the bit with plain stores;
// the cell list may name a cell twice and clears it with an atomic.  Only
// integer atomics: the result depends neither on arrival order nor on the grid.
// Paths are relative to avida-core/source/ of the reference.
#include "device.h"

namespace {

#define EV_BLOCK 256
#define EV_MAX_BLOCKS 4096          // grid-stride beyond 4 M cells

// `k` of every thread of the block summed into *dst: one atomic per block that killed anyone
__device__ __forceinline__ void add_killed(unsigned long long* dst, int k) {
  __shared__ int s_killed;
  if (threadIdx.x == 0) s_killed = 0;
  __syncthreads();
  for (int d = 32; d > 0; d >>= 1) k += __shfl_down(k, d);
  if ((threadIdx.x & 63) == 0 && k) atomicAdd(&s_killed, k);
  __syncthreads();
  if (threadIdx.x == 0 && s_killed) atomicAdd(dst, (unsigned long long)s_killed);
}

// dies(cell, ctl) for every living cell of the quads [0, nq) x stride, quad q
// holding the control words at base + 4 q .. (at most `limit` words exist past
// base); wide: base + 4 q is 16-B aligned.  Returns the thread's kills.
template <typename F>
__device__ __forceinline__ int visit_quad(uint32_t* ctl, int64_t c0, int64_t limit, bool wide, F dies) {
  int killed = 0;
  if (wide && c0 + 4 <= limit) {
    uint4 v = *reinterpret_cast<const uint4*>(ctl + c0);
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((w[j] & CTL_ALIVE) && dies(c0 + j, w[j])) { w[j] &= ~CTL_ALIVE; killed++; }
    if (killed) *reinterpret_cast<uint4*>(ctl + c0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (int j = 0; j < 4 && c0 + j < limit; j++) {
      const uint32_t w = ctl[c0 + j];
      if ((w & CTL_ALIVE) && dies(c0 + j, w)) { ctl[c0 + j] = w & ~CTL_ALIVE; killed++; }
    }
  }
  return killed;
}
// the whole control row
template <typename F>
__device__ __forceinline__ int visit_world(const DevWorld& W, F dies) {
  const int64_t nq = (W.n + 3) / 4;
  int killed = 0;
  for (int64_t q = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x; q < nq; q += (int64_t)gridDim.x * EV_BLOCK)
    killed += visit_quad(W.ctl, 4 * q, W.n, true, dies);
  return killed;
}

// the old value the atomic returns says who was alive: a cell named twice counts once
__global__ __launch_bounds__(EV_BLOCK) void k_ev_kill_cells(DevWorld W, EvScratch S, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x;
  int k = 0;
  if (i < n) k = (atomicAnd(&W.ctl[S.cells[i]], ~CTL_ALIVE) & CTL_ALIVE) ? 1 : 0;
  add_killed(S.killed, k);
}

template <bool KEYED>
__global__ __launch_bounds__(EV_BLOCK) void k_ev_kill_prob(DevWorld W, EvScratch S, uint32_t base, uint64_t th,
                                                           int64_t nkeys) {
  const int k = visit_world(W, [&](int64_t c, uint32_t) {
    if (KEYED) {
      const uint64_t g = W.gkey[c];
      int64_t lo = 0, hi = nkeys;                   // the first key >= g
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (S.keys[mid] < g) lo = mid + 1; else hi = mid;
      }
      if (lo >= nkeys || S.keys[lo] != g) return false;
    }
    return (uint64_t)event_draw(base, (uint64_t)(W.cell0 + c)) < th;
  });
  add_killed(S.killed, k);
}

// item = (row r of the rectangle, quad q of that world row): the columns of the
// quad inside x1 .. x2 (mod X) die
__global__ __launch_bounds__(EV_BLOCK) void k_ev_kill_rect(DevWorld W, EvScratch S, int x1, int y1, int x2, int y2) {
  const int64_t X = W.world_x, Y = W.world_y, qpr = (X + 3) / 4;
  const int64_t items = (int64_t)(y2 - y1 + 1) * qpr;
  const bool wide = (X & 3) == 0;                   // every row starts 16-B aligned
  const int span = x2 - x1;
  int killed = 0;
  for (int64_t it = (int64_t)blockIdx.x * EV_BLOCK + threadIdx.x; it < items; it += (int64_t)gridDim.x * EV_BLOCK) {
    const int64_t r = it / qpr, q = it - r * qpr;
    const int64_t row = ((y1 + r) % Y) * X;
    killed += visit_quad(W.ctl + row, 4 * q, X, wide, [&](int64_t x, uint32_t) {
      int d = (int)x - x1;
      if (d < 0) d += (int)X;
      return d <= span;
    });
  }
  add_killed(S.killed, killed);
}

// Radix select of the keep-th smallest word among the living, most significant
// digit first.  Pass p counts digit p of the words whose higher digits equal
// the prefix chosen so far: in LDS, then one add per populated bin and block.
__global__ __launch_bounds__(EV_BLOCK) void k_ev_hist(DevWorld W, EvScratch S, uint32_t base, int pass) {
  __shared__ uint32_t s_hist[EV_BINS];
  static_assert(EV_BINS <= EV_BLOCK, "a thread per bin");
  const EvSelect sel = *S.sel;
  if (pass > 0 && sel.rank == 0) return;            // keep >= living: no threshold to find
  if (threadIdx.x < EV_BINS) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int low = 32 - EV_DIGIT_BITS * (pass + 1);  // the digit's lowest bit
  visit_world(W, [&](int64_t c, uint32_t) {
    const uint32_t h = event_draw(base, (uint64_t)(W.cell0 + c));
    if (pass == 0 || (h >> (low + EV_DIGIT_BITS)) == sel.prefix) atomicAdd(&s_hist[(h >> low) & (EV_BINS - 1)], 1u);
    return false;
  });
  __syncthreads();
  if (threadIdx.x < EV_BINS && s_hist[threadIdx.x])
    atomicAdd(&S.hist[pass * EV_BINS + threadIdx.x], s_hist[threadIdx.x]);
}

// One block: the bin the rank falls in becomes the prefix's next digit, the
// rank becomes the rank inside that bin.  Pass 0 sets the rank: keep, or 0
// when at most keep organisms live.  (256 bins: thread 0 walks them.)
__global__ __launch_bounds__(EV_BINS) void k_ev_pick(EvScratch S, int pass, int64_t keep) {
  __shared__ uint32_t s_cnt[EV_BINS];
  s_cnt[threadIdx.x] = S.hist[pass * EV_BINS + threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  EvSelect sel = *S.sel;
  if (pass == 0) {
    uint64_t living = 0;
    for (int b = 0; b < EV_BINS; b++) living += s_cnt[b];
    sel.prefix = 0;
    sel.rank = (uint64_t)keep < living ? (uint64_t)keep : 0;
  }
  if (sel.rank) {
    uint64_t before = 0;
    for (int b = 0; b < EV_BINS; b++) {
      if (before + s_cnt[b] >= sel.rank) {
        sel.prefix = (sel.prefix << EV_DIGIT_BITS) | (uint32_t)b;
        sel.rank -= before;
        break;
      }
      before += s_cnt[b];
    }
  }
  *S.sel = sel;
}

// after the last pass the prefix is the keep-th smallest word itself: T
__global__ __launch_bounds__(EV_BLOCK) void k_ev_kill_above(DevWorld W, EvScratch S, uint32_t base) {
  const EvSelect sel = *S.sel;
  int k = 0;
  if (sel.rank)
    k = visit_world(W, [&](int64_t c, uint32_t) { return event_draw(base, (uint64_t)(W.cell0 + c)) > sel.prefix; });
  add_killed(S.killed, k);
}

unsigned scan_blocks(int64_t quads) {
  const unsigned b = nblk(quads, EV_BLOCK);
  return b < 1 ? 1 : (b > EV_MAX_BLOCKS ? EV_MAX_BLOCKS : b);
}

}  // namespace

void launch_kill_cells(const DevWorld& W, const EvScratch& S, hipStream_t s, int64_t n) {
  hipLaunchKernelGGL(k_ev_kill_cells, dim3(nblk(n, EV_BLOCK)), dim3(EV_BLOCK), 0, s, W, S, n);
}

void launch_kill_prob(const DevWorld& W, const EvScratch& S, hipStream_t s, uint32_t base, uint64_t th, int64_t nkeys) {
  const dim3 grid(scan_blocks((W.n + 3) / 4));
  if (nkeys >= 0) hipLaunchKernelGGL(k_ev_kill_prob<true>, grid, dim3(EV_BLOCK), 0, s, W, S, base, th, nkeys);
  else hipLaunchKernelGGL(k_ev_kill_prob<false>, grid, dim3(EV_BLOCK), 0, s, W, S, base, th, nkeys);
}

void launch_kill_rect(const DevWorld& W, const EvScratch& S, hipStream_t s, int x1, int y1, int x2, int y2) {
  const int64_t items = (int64_t)(y2 - y1 + 1) * ((W.world_x + 3) / 4);
  hipLaunchKernelGGL(k_ev_kill_rect, dim3(scan_blocks(items)), dim3(EV_BLOCK), 0, s, W, S, x1, y1, x2, y2);
}

void launch_keep_sample(const DevWorld& W, const EvScratch& S, hipStream_t s, uint32_t base, int64_t keep) {
  const dim3 grid(scan_blocks((W.n + 3) / 4));
  for (int pass = 0; pass < EV_PASSES; pass++) {
    hipLaunchKernelGGL(k_ev_hist, grid, dim3(EV_BLOCK), 0, s, W, S, base, pass);
    hipLaunchKernelGGL(k_ev_pick, dim3(1), dim3(EV_BINS), 0, s, S, pass, keep);
  }
  hipLaunchKernelGGL(k_ev_kill_above, grid, dim3(EV_BLOCK), 0, s, W, S, base);
}
