// distance.hip -- genetic distances and the consensus histogram:
//   k_pair_dist   Hamming and Levenshtein distance of pairs of host-supplied genomes
//   k_cell_dist   the same of every cell's birth-genome prefix against one reference genome
//   k_site_hist   per-site instruction histogram of the living cells (CalcConsensus)
//   k_site_fill   its "no site" column
// InstructionSequence::FindHammingDistance (core/InstructionSequence.cc:488-504,
// offset 0) and FindEditDistance (:547-613) restated: one wave per pair, 32-bit
// integers only.  Paths are relative to avida-core/source/ of the reference.
#include "device.h"

namespace {

#define DIST_WAVES 4                 // pairs (cells) per block, one wave each
#define DIST_PAD 0x100               // a pad site of the systolic row: equal to no symbol

// lane i takes lane i - 1's v; lane 0 takes `first` (DPP wave_shr:1, every lane active)
__device__ __forceinline__ int lane_shr1(int first, int v) {
  return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false);
}

// The Levenshtein distance of a[0 .. m) and b[0 .. n) (both in LDS, m, n >= 1,
// m <= 64 C) by a systolic wave: lane L keeps columns L C + 1 .. (L + 1) C of
// the DP row in cur[], and works on row t - L + 1 at step t.  At the start of
// a step lane L - 1 has finished the row lane L is about to work on: its last
// column's value is the left neighbour of lane L's first column, the value
// before it the diagonal.  Lane 0 takes the row numbers themselves (column 0).
// Every index into a[] and cur[] is a constant of the unrolled loops: no scratch.
template <int C>
__device__ __forceinline__ int edit_systolic(const uint8_t* sa, int m, const uint8_t* sb, int n, int lane) {
  int a[C], cur[C];
#pragma unroll
  for (int k = 0; k < C; k++) {
    const int j = lane * C + k;
    a[k] = j < m ? (int)sa[j] : DIST_PAD;
    cur[k] = j + 1;                       // row 0
  }
  int last = cur[C - 1], last_prev = last;
  const int last_lane = (m - 1) / C;      // the lane holding column m
  const int steps = n + last_lane;        // (at most n + 63)
  int bnext = sb[min(max(-lane, 0), n - 1)];
  for (int t = 0; t < steps; t++) {
    const int r = t - lane;               // this lane's row, less 1
    int left = lane_shr1(r + 1, last);
    int diag = lane_shr1(r, last_prev);
    const int bs = bnext;
    bnext = sb[min(max(r + 1, 0), n - 1)];
    if ((unsigned)r < (unsigned)n) {
#pragma unroll
      for (int k = 0; k < C; k++) {
        const int up = cur[k];
        const int v = a[k] == bs ? diag : min(min(diag, up), left) + 1;
        diag = up;
        left = v;
        cur[k] = v;
      }
      last_prev = diag;
      last = left;
    }
  }
  const int km = (m - 1) & (C - 1);
  int res = 0;
#pragma unroll
  for (int k = 0; k < C; k++)
    if (k == km) res = cur[k];
  return __shfl(res, last_lane);
}

// Both distances of sa[0 .. la) and sb[0 .. lb) (LDS, symbols masked), by one
// wave.  Hamming: the length difference plus the mismatches of the overlap,
// lane-strided, counted by ballots.  Levenshtein: the common prefix (found by
// the same pass) and the common suffix of what is left are cut off -- the
// distance of the middles is the distance of the whole -- and the middles go
// through the systolic wave.
__device__ __forceinline__ void wave_distance(const uint8_t* sa, int la, const uint8_t* sb, int lb, int lane,
                                              bool want_edit, int& ham, int& edit) {
  la = __builtin_amdgcn_readfirstlane(la);
  lb = __builtin_amdgcn_readfirstlane(lb);
  const int mn = min(la, lb);
  int mism = 0, front = mn;
  for (int base = 0; base < mn; base += 64) {
    const int p = base + lane;
    const unsigned long long bal = __ballot(p < mn && sa[p] != sb[p]);
    if (bal != 0ull && front == mn) front = base + __ffsll((long long)bal) - 1;
    mism += __popcll(bal);
  }
  ham = la + lb - 2 * mn + mism;
  edit = 0;
  if (!want_edit) return;
  const int room = mn - front;
  int back = room;
  for (int base = 0; base < room; base += 64) {
    const int q = base + lane;
    const unsigned long long bal = __ballot(q < room && sa[la - 1 - q] != sb[lb - 1 - q]);
    if (bal != 0ull) {
      back = base + __ffsll((long long)bal) - 1;
      break;
    }
  }
  // (wave-uniform values, said so: the loops over them stay scalar)
  const int m = __builtin_amdgcn_readfirstlane(la - front - back), n = __builtin_amdgcn_readfirstlane(lb - front - back);
  if (m == 0 || n == 0) {
    edit = m + n;
    return;
  }
  const uint8_t* ta = sa + front;
  const uint8_t* tb = sb + front;
  const int c = (m + 63) >> 6;
  if (c <= 1) edit = edit_systolic<1>(ta, m, tb, n, lane);
  else if (c <= 2) edit = edit_systolic<2>(ta, m, tb, n, lane);
  else if (c <= 4) edit = edit_systolic<4>(ta, m, tb, n, lane);
  else if (c <= 8) edit = edit_systolic<8>(ta, m, tb, n, lane);
  else if (c <= 16) edit = edit_systolic<16>(ta, m, tb, n, lane);
  else edit = edit_systolic<32>(ta, m, tb, n, lane);
}

// len sites from g (16-B aligned, readable up to the next multiple of 16) into
// dst (LDS, 16-B aligned, TAPE_SLOT bytes), bits 0-5 of each; `tid` of `nthr` threads.
// Sites from `valid` on take `fill` (a tape prefix past the organism's memory).
__device__ __forceinline__ void stage_sites(uint8_t* dst, const uint8_t* g, int len, int valid, uint32_t fill,
                                            int tid, int nthr) {
  const uint4* src = reinterpret_cast<const uint4*>(g);
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint32_t f4 = fill * 0x01010101u;
  for (int q = tid; q < (len + 15) / 16; q += nthr) {
    uint4 v = src[q];
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int keep = valid - (16 * q + 4 * k);         // sites of this word inside the memory
      uint32_t x = w[k] & 0x3F3F3F3Fu;
      if (keep < 4) {
        const uint32_t msk = keep <= 0 ? 0u : (1u << (8 * keep)) - 1u;
        x = (x & msk) | (f4 & ~msk);
      }
      w[k] = x;
    }
    d[q] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// pair p = (pair_a[p], pair_b[p]) of the n genomes packed in `gen` (genome g
// at off[g], 16-B aligned and padded): one wave per pair
__global__ __launch_bounds__(64 * DIST_WAVES) void k_pair_dist(const uint8_t* gen, const int64_t* off,
                                                               const int32_t* len, const int32_t* pair_a,
                                                               const int32_t* pair_b, int npairs, int32_t* ham,
                                                               int32_t* edit) {
  __shared__ __attribute__((aligned(16))) uint8_t s_seq[DIST_WAVES][2][TAPE_SLOT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p = blockIdx.x * DIST_WAVES + wv;
  int la = 0, lb = 0;
  if (p < npairs) {
    const int ga = pair_a[p], gb = pair_b[p];
    la = len[ga]; lb = len[gb];
    stage_sites(s_seq[wv][0], gen + off[ga], la, la, 0u, lane, 64);
    stage_sites(s_seq[wv][1], gen + off[gb], lb, lb, 0u, lane, 64);
  }
  __syncthreads();
  if (p >= npairs) return;
  int h, e;
  wave_distance(s_seq[wv][0], la, s_seq[wv][1], lb, lane, edit != nullptr, h, e);
  if (lane == 0) {
    if (ham) ham[p] = h;
    if (edit) edit[p] = e;
  }
}

// cell first + i: its tape prefix of birth_len sites (a site past the
// organism's memory reads as op 0, as avgpu_get_states hands it out) against
// ref[0 .. ref_len) in canonical codes; an empty cell answers -1
__global__ __launch_bounds__(64 * DIST_WAVES) void k_cell_dist(DevWorld W, int64_t first, int64_t count,
                                                               const uint8_t* ref, int ref_len, int32_t* ham,
                                                               int32_t* edit) {
  __shared__ __attribute__((aligned(16))) uint8_t s_ref[TAPE_SLOT];
  __shared__ __attribute__((aligned(16))) uint8_t s_seq[DIST_WAVES][TAPE_SLOT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * DIST_WAVES + wv;
  stage_sites(s_ref, ref, ref_len, ref_len, 0u, threadIdx.x, 64 * DIST_WAVES);
  int la = -1;
  if (i < count) {
    const int64_t c = first + i;
    if (W.ctl[c] & CTL_ALIVE) {
      la = min(max(W.birth_len[c], 0), TAPE_SLOT);
      stage_sites(s_seq[wv], W.tape + c * TAPE_SLOT, la, min(max(W.mem_size[c], 0), la), W.fill_code, lane, 64);
    }
  }
  __syncthreads();
  if (i >= count) return;
  int h = -1, e = -1;
  if (la >= 0) wave_distance(s_seq[wv], la, s_ref, ref_len, lane, edit != nullptr, h, e);
  if (lane == 0) {
    if (ham) ham[i] = h;
    if (edit) edit[i] = la >= 0 ? e : -1;
  }
}

// ---------------------------------------------------------------------------
// The consensus histogram.  A block owns HIST_WIN sites (one per thread) and
// `chunk` cells: thread t alone counts site t's handlers in its own LDS row,
// then adds the non-zero counts to hist with integer atomics.  Only real sites
// are counted here; column 0 ("no site") is what is left of the living cells
// (k_site_fill).
#define HIST_WIN 128
#define HIST_COLS (AVGPU_MAX_INST + 1)
static_assert(TAPE_SLOT % HIST_WIN == 0 && CODE_MASK < AVGPU_MAX_INST, "site windows; a column per handler");

__global__ __launch_bounds__(HIST_WIN) void k_site_hist(DevWorld W, int64_t first, int64_t count, int64_t chunk,
                                                        int32_t* hist, unsigned long long* living) {
  __shared__ int32_t s_hist[HIST_WIN * HIST_COLS];
  __shared__ int32_t s_len[HIST_WIN], s_mem[HIST_WIN];
  const int t = threadIdx.x;
  const int j0 = blockIdx.x * HIST_WIN, j = j0 + t;
  for (int k = 0; k < HIST_COLS; k++) s_hist[t * HIST_COLS + k] = 0;
  const int64_t c0 = first + (int64_t)blockIdx.y * chunk;
  const int64_t c1 = min(first + count, c0 + chunk);
  unsigned long long alive = 0;
  for (int64_t g = c0; g < c1; g += HIST_WIN) {
    __syncthreads();                       // the group before is read
    const int64_t c = g + t;
    int len = 0, mem = 0;
    if (c < c1 && (W.ctl[c] & CTL_ALIVE)) {
      len = min(max(W.birth_len[c], 0), TAPE_SLOT);
      mem = W.mem_size[c];
      alive++;
    }
    s_len[t] = len;
    s_mem[t] = mem;
    __syncthreads();
    const int ng = (int)min<int64_t>(HIST_WIN, c1 - g);
    for (int i = 0; i < ng; i++) {
      const int len_i = s_len[i];
      if (j0 >= len_i) continue;           // (the same in every thread)
      if (j < len_i) {
        const int code = j < s_mem[i] ? (W.tape[(g + i) * TAPE_SLOT + j] & CODE_MASK) : (int)W.fill_code;
        s_hist[t * HIST_COLS + 1 + code]++;
      }
    }
  }
  for (int k = 1; k < HIST_COLS; k++) {
    const int v = s_hist[t * HIST_COLS + k];
    if (v) atomicAdd(&hist[(int64_t)j * HIST_COLS + k], v);
  }
  if (blockIdx.x == 0 && alive) atomicAdd(living, alive);
}

__global__ void k_site_fill(int32_t* hist, const unsigned long long* living) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= TAPE_SLOT) return;
  int sum = 0;
  for (int k = 1; k < HIST_COLS; k++) sum += hist[(int64_t)j * HIST_COLS + k];
  hist[(int64_t)j * HIST_COLS] = (int)*living - sum;
}

}  // namespace

void launch_pair_dist(const DistScratch& S, hipStream_t s, int npairs, bool want_ham, bool want_edit) {
  hipLaunchKernelGGL(k_pair_dist, dim3(nblk(npairs, DIST_WAVES)), dim3(64 * DIST_WAVES), 0, s, S.gen, S.off, S.len,
                     S.pair_a, S.pair_b, npairs, want_ham ? S.ham : nullptr, want_edit ? S.edit : nullptr);
}

void launch_cell_dist(const DevWorld& W, const DistScratch& S, hipStream_t s, int64_t first, int64_t count,
                      int ref_len, bool want_ham, bool want_edit) {
  hipLaunchKernelGGL(k_cell_dist, dim3(nblk(count, DIST_WAVES)), dim3(64 * DIST_WAVES), 0, s, W, first, count, S.gen,
                     ref_len, want_ham ? S.ham : nullptr, want_edit ? S.edit : nullptr);
}

void launch_site_hist(const DevWorld& W, const DistScratch& S, hipStream_t s, int64_t first, int64_t count) {
  // at most 256 chunks of at least 256 cells: a block's flush is worth its cells
  const int64_t chunk = count > 65536 ? (count + 255) / 256 : 256;
  const unsigned nchunk = (unsigned)((count + chunk - 1) / chunk);
  hipLaunchKernelGGL(k_site_hist, dim3(TAPE_SLOT / HIST_WIN, nchunk), dim3(HIST_WIN), 0, s, W, first, count, chunk,
                     S.hist, S.living);
  hipLaunchKernelGGL(k_site_fill, dim3(TAPE_SLOT / 256), dim3(256), 0, s, S.hist, S.living);
}
