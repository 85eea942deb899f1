// landscape.hip -- mutational landscapes on the device:
//   k_land_seed       a cell's organism straight from its mutant rank (depth 0)
//   k_land_seed_next  ... or from the stored offspring of the depth before
//   k_land_judge      cTestCPU::TestGenome_Body's verdict on a gestated cell
//                     (cpu/cTestCPU.cc:233-326): fitness, or on to the next depth
//   k_land_reduce     cLandscape::ProcessGenome's classification and sums over
//                     one tile of ranks (main/cLandscape.cc:97-123, :204)
//   k_land_rows       a genome's tiles combined into its avgpu_landscape row
//   k_land_epi_reduce cLandscape::TestMutPair's classification of one tile of
//                     pair mutants against the one-step chart (:909-949)
//   k_land_epi_rows   a genome's tiles combined into its avgpu_epistasis row
// A mutant is an edit of its base genome, made from its rank alone (LandEdit):
// one or two substitutions (Process_Body :177-213), one insertion
// (ProcessInsert :297-330) or one deletion (ProcessDelete :265-295).
// The gestations between seed and judge are the TEST-mode k_interpret launches
// of an ordinary avgpu_step (capi.hip).  Paths are relative to
// avida-core/source/ of the reference.
#include "device.h"

#pragma clang fp contract(off)

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the genome holding mutant m: the last g with off[g] <= m
__device__ __forceinline__ int land_find(const int64_t* off, int n, int64_t m) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= m) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the edit that makes a mutant of its base genome.  shift 0: site s1 takes op k1
// (s1 < 0: none), site s2 > s1 op k2 (s2 < 0: none); shift +1: op k1 is
// inserted before site s1 (s1 = L: behind the last); shift -1: site s1 is removed
struct LandEdit { int s1, k1, s2, k2, shift; };

// mutants whose first site is below s1 at distance 2, K = num_insts - 1
__device__ __forceinline__ int64_t land_before(int64_t L, int64_t K, int64_t s1) {
  return K * K * (s1 * (L - 1) - s1 * (s1 - 1) / 2);
}

// rank -> edit (avida_gpu.h "Mutant ranks"); ops: the base genome's op codes
__device__ __forceinline__ LandEdit land_decode(const uint8_t* ops, int L, int num_insts, int mode, int64_t r) {
  LandEdit u = {-1, 0, -1, 0, 0};
  const int64_t K = num_insts - 1;
  if (mode == LAND_SUB1) {
    u.s1 = (int)(r / K);
    const int j = (int)(r % K);
    u.k1 = j + (j >= (int)ops[u.s1] ? 1 : 0);
  } else if (mode == LAND_SUB2) {
    int lo = 0, hi = L - 2;                     // the last s1 with land_before(s1) <= r
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (land_before(L, K, mid) <= r) lo = mid; else hi = mid - 1;
    }
    u.s1 = lo;
    const int64_t q = r - land_before(L, K, lo);
    const int64_t per = K * (L - 1 - lo);       // mutants per op at the first site
    const int j1 = (int)(q / per);
    const int64_t q2 = q % per;
    u.k1 = j1 + (j1 >= (int)ops[u.s1] ? 1 : 0);
    u.s2 = lo + 1 + (int)(q2 / K);
    const int j2 = (int)(q2 % K);
    u.k2 = j2 + (j2 >= (int)ops[u.s2] ? 1 : 0);
  } else if (mode == LAND_INS) {                // line * num_insts + op, no op skipped
    u.s1 = (int)(r / num_insts);
    u.k1 = (int)(r % num_insts);
    u.shift = 1;
  } else if (mode == LAND_DEL) {
    u.s1 = (int)r;
    u.shift = -1;
  }
  return u;
}

// the site the reference counts the mutant under (Process_Body:204: the
// innermost; ProcessInsert :324, ProcessDelete :290: line_num)
__device__ __forceinline__ int land_site(const LandEdit& u) { return u.s2 >= 0 ? u.s2 : u.s1; }

// word `v` of sites base .. base + 3 with site s set to code c
__device__ __forceinline__ uint32_t land_patch(uint32_t v, int base, int s, uint32_t c) {
  const unsigned d = (unsigned)(s - base);
  if (d < 4u) v = (v & ~(0xFFu << (8u * d))) | (c << (8u * d));
  return v;
}
// the bytes of a word of sites base .. base + 3 that lie below len
__device__ __forceinline__ uint32_t land_mask(int base, int len) {
  const int keep = len - base;
  return keep >= 4 ? 0xFFFFFFFFu : (keep <= 0 ? 0u : (1u << (8 * keep)) - 1u);
}
// word w of a base genome of L sites, zero outside it (an insertion's first
// word has no word before it; a deletion reads the site behind the last)
__device__ __forceinline__ uint32_t land_base_word(const uint32_t* base32, int w, int L) {
  return (w >= 0 && 4 * w < L) ? base32[w] : 0u;
}

// The one word builder (seed and judge both go through it): the canonical codes of a mutant's sites 4w .. 4w + 3
// (sites past the mutant's length zero) from the base genome's word w (`lo`)
// and, for a length change, the word beside it (`nb`: w - 1 for an insertion,
// w + 1 for a deletion).  From the edit site on the mutant is the base
// shifted by one site: a byte funnel of the two words.
__device__ __forceinline__ uint32_t land_word(uint32_t lo, uint32_t nb, int w, int L, const LandEdit& u, uint32_t c1,
                                              uint32_t c2) {
  if (u.shift == 0) {
    uint32_t v = land_patch(lo, 4 * w, u.s1, c1);
    v = land_patch(v, 4 * w, u.s2, c2);
    return v & land_mask(4 * w, L);
  }
  const uint32_t sh = u.shift > 0 ? (lo << 8) | (nb >> 24) : (lo >> 8) | (nb << 24);
  const uint32_t below = land_mask(4 * w, u.s1);                   // the sites before the edit
  uint32_t v = (lo & below) | (sh & ~below);
  if (u.shift > 0) v = land_patch(v, 4 * w, u.s1, c1);
  return v & land_mask(4 * w, L + u.shift);
}

__global__ void k_land_seed(DevWorld W, LandScratch S, int mode, int64_t m0, int cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const int64_t m = m0 + i;
  const int g = mode == LAND_BASE ? (int)m : land_find(S.mut_off, S.n, m);
  const int64_t r = mode == LAND_BASE ? 0 : m - S.mut_off[g];
  const int L = S.len[g];
  const LandEdit u = land_decode(S.base_op + S.base_off[g], L, S.num_insts, mode, r);
  const uint32_t c1 = u.s1 >= 0 ? S.op2code[u.k1] : 0u, c2 = u.s2 >= 0 ? S.op2code[u.k2] : 0u;
  const uint32_t* b32 = reinterpret_cast<const uint32_t*>(S.base_code + S.base_off[g]);
  uint32_t* t = reinterpret_cast<uint32_t*>(W.tape + (int64_t)i * TAPE_SLOT);
  const int M = L + u.shift;                  // the mutant's length: its size class, its budget
  for (int w = 0; 4 * w < M; w++)
    t[w] = land_word(land_base_word(b32, w, L), u.shift ? land_base_word(b32, w - u.shift, L) : 0u, w, L, u, c1, c2);
  inject_org(W, i, M, 0.0, nullptr, 1);
  S.budget[i] = S.time_mod * M;
}

__global__ void k_land_seed_next(DevWorld W, LandScratch S, int depth, int cnt) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cnt) return;
  const int src = S.src[depth - 1][j];
  int L = W.t_child_len[src];
  L = L < 1 ? 1 : (L > AVGPU_MAX_GENOME ? AVGPU_MAX_GENOME : L);   // (a divide's offspring is in range)
  const uint32_t* ch = reinterpret_cast<const uint32_t*>(W.t_child + (int64_t)src * TAPE_SLOT);
  uint32_t* t = reinterpret_cast<uint32_t*>(W.tape + (int64_t)j * TAPE_SLOT);
  uint32_t* keep = reinterpret_cast<uint32_t*>(S.gen[depth - 1] + (int64_t)j * TAPE_SLOT);
  // whole 16-B groups, zero past the genome: the judge compares 16 B at a time
  for (int w = 0; 4 * w < ((L + 15) & ~15); w++) {
    const uint32_t v = ch[w] & 0x3F3F3F3Fu & land_mask(4 * w, L);
    if (4 * w < L) t[w] = v;
    keep[w] = v;
  }
  S.glen[depth - 1][j] = L;
  inject_org(W, j, L, 0.0, nullptr, 1);
  S.budget[j] = S.time_mod * L;
}

// does the wave's offspring `ch` (clen sites) equal the stored genome `g`
// (glen sites, zero to the end of its last 16-B group)?  Wave-uniform.
__device__ __forceinline__ bool land_eq_stored(const uint8_t* ch, int clen, const uint8_t* g, int glen, int lane) {
  if (clen != glen) return false;
  bool diff = false;
  for (int o = lane * 16; o < clen; o += 64 * 16) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(ch + o);
    const u32x4 b = *reinterpret_cast<const u32x4*>(g + o);
#pragma unroll
    for (int q = 0; q < 4; q++) diff = diff || (((a[q] & 0x3F3F3F3Fu) ^ b[q]) & land_mask(o + 4 * q, clen)) != 0u;
  }
  return __ballot(diff) == 0ull;
}
// ... equal the mutant itself, recomputed from its rank?  The groups run
// over the mutant's length, which is the base's +- 1 for an indel.
__device__ __forceinline__ bool land_eq_mutant(const uint8_t* ch, int clen, const uint8_t* base_code, int L,
                                               const LandEdit& u, uint32_t c1, uint32_t c2, int lane) {
  if (clen != L + u.shift) return false;
  const uint32_t* b32 = reinterpret_cast<const uint32_t*>(base_code);
  bool diff = false;
  for (int o = lane * 16; o < clen; o += 64 * 16) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(ch + o);
    // (an insertion's last group may start behind the base's last: zero)
    const u32x4 b = o < L ? *reinterpret_cast<const u32x4*>(base_code + o) : u32x4{0u, 0u, 0u, 0u};
    const int w0 = o >> 2;
    const uint32_t side = u.shift > 0 ? land_base_word(b32, w0 - 1, L) : u.shift < 0 ? land_base_word(b32, w0 + 4, L) : 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      // the word beside word q: inside the group, or the one fetched from outside it
      const uint32_t nb = u.shift > 0 ? (q == 0 ? side : b[q > 0 ? q - 1 : 0]) : (q == 3 ? side : b[q < 3 ? q + 1 : 3]);
      const uint32_t e = land_word(b[q], nb, w0 + q, L, u, c1, c2);
      diff = diff || (((a[q] & 0x3F3F3F3Fu) ^ e) & land_mask(o + 4 * q, clen)) != 0u;
    }
  }
  return __ballot(diff) == 0ull;
}

// One wave per gestated cell c of depth `depth`.  The chunk's mutant it
// descends from is i (c itself at depth 0).
__global__ void k_land_judge(DevWorld W, LandScratch S, int mode, int depth, int64_t m0, int cnt) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= cnt) return;
  const int c1cell = depth == 2 ? S.src[1][c] : c;                  // the depth-1 cell on the way
  const int i = depth == 0 ? c : S.src[0][c1cell];
  double fit = 0.0;
  bool verdict = true, colony = false;      // colony: this depth's organism is the colony's
  if (W.num_div[c] > 0) {
    const int64_t m = m0 + i;
    const int g = mode == LAND_BASE ? (int)m : land_find(S.mut_off, S.n, m);
    const int64_t r = mode == LAND_BASE ? 0 : m - S.mut_off[g];
    const int L = S.len[g];
    const LandEdit u = land_decode(S.base_op + S.base_off[g], L, S.num_insts, mode, r);
    const uint32_t k1 = u.s1 >= 0 ? S.op2code[u.k1] : 0u, k2 = u.s2 >= 0 ? S.op2code[u.k2] : 0u;
    const uint8_t* ch = W.t_child + (int64_t)c * TAPE_SLOT;
    const int clen = W.t_child_len[c];
    // copy-true, or the offspring is a genome of a depth below (GetColonyOrganism,
    // cpu/cCPUTestInfo.h:133-138): this depth's organism is the colony's
    bool same = land_eq_mutant(ch, clen, S.base_code + S.base_off[g], L, u, k1, k2, lane);
    if (!same && depth >= 1)
      same = land_eq_stored(ch, clen, S.gen[0] + (int64_t)c1cell * TAPE_SLOT, S.glen[0][c1cell], lane);
    if (!same && depth == 2)
      same = land_eq_stored(ch, clen, S.gen[1] + (int64_t)c * TAPE_SLOT, S.glen[1][c], lane);
    colony = same;
    if (same) fit = W.fitness[c];
    else verdict = depth == 2;                                      // past the last depth: fitness 0
  }
  if (lane != 0) return;
  if (!verdict) {
    S.src[depth][atomicAdd(&S.count[depth], 1)] = c;               // on to depth + 1
    return;
  }
  if (mode == LAND_BASE) {                                          // ProcessBase (main/cLandscape.cc:125-142)
    S.base_fit[m0 + i] = fit;
    S.base_merit[m0 + i] = colony ? W.merit[c] : 0.0;
    S.base_gest[m0 + i] = colony ? W.gest_time[c] : 0;
  } else {
    S.fit[i] = fit;
    S.dep[i] = (uint8_t)depth;
  }
}

__device__ __forceinline__ void land_peak(double& f, int64_t& r, double f2, int64_t r2) {
  if (f2 > f || (f2 == f && r2 < r)) { f = f2; r = r2; }
}
__device__ __forceinline__ void land_add(LandPart& a, const LandPart& b) {
  a.sf = a.sf + b.sf; a.sq = a.sq + b.sq; a.sp = a.sp + b.sp; a.sn = a.sn + b.sn;
  land_peak(a.pf, a.pr, b.pf, b.pr);
  a.dead += b.dead; a.neg += b.neg; a.neut += b.neut; a.pos += b.pos; a.run1 += b.run1; a.run2 += b.run2;
}
__device__ __forceinline__ LandPart land_shfl_down(const LandPart& a, int off) {
  LandPart b;
  b.sf = __shfl_down(a.sf, off); b.sq = __shfl_down(a.sq, off); b.sp = __shfl_down(a.sp, off);
  b.sn = __shfl_down(a.sn, off); b.pf = __shfl_down(a.pf, off);
  b.pr = (int64_t)__shfl_down((long long)a.pr, off);
  b.dead = __shfl_down(a.dead, off); b.neg = __shfl_down(a.neg, off); b.neut = __shfl_down(a.neut, off);
  b.pos = __shfl_down(a.pos, off); b.run1 = __shfl_down(a.run1, off); b.run2 = __shfl_down(a.run2, off);
  b.pad = 0;
  return b;
}
// The 256 threads' parts added up in one fixed tree (lane + 32, + 16 .. + 1
// inside a wave, then (w0 + w1) + (w2 + w3)): thread 0 returns the total.
__device__ __forceinline__ LandPart land_block_sum(LandPart a) {
  __shared__ LandPart s_w[4];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const LandPart b = land_shfl_down(a, off);
    land_add(a, b);
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    LandPart lo = s_w[0], hi = s_w[2];
    land_add(lo, s_w[1]);
    land_add(hi, s_w[3]);
    land_add(lo, hi);
    a = lo;
  }
  return a;
}
__device__ __forceinline__ LandPart land_zero() {
  LandPart a;
  a.sf = a.sq = a.sp = a.sn = 0.0;
  a.pf = -1.0;
  a.pr = INT64_MAX;
  a.dead = a.neg = a.neut = a.pos = a.run1 = a.run2 = 0;
  a.pad = 0;
  return a;
}

// One block per tile: ranks 256 t .. of genome g, thread k its rank 256 t + k.
__global__ void __launch_bounds__(LAND_TILE) k_land_reduce(LandScratch S, int mode, int64_t m0, int64_t t0) {
  const int64_t T = t0 + blockIdx.x;
  const int g = land_find(S.tile_off, S.n, T);
  const int64_t r = (T - S.tile_off[g]) * LAND_TILE + threadIdx.x;
  LandPart a = land_zero();
  if (r < S.mut_off[g + 1] - S.mut_off[g]) {
    const int64_t i = S.mut_off[g] + r - m0;
    const double f = S.fit[i], base = S.base_fit[g];
    const int d = S.dep[i];
    a.sf = f;
    a.sq = f * f;
    a.run1 = d >= 1; a.run2 = d >= 2;
    if (f == 0.0) a.dead = 1;                 // ProcessGenome (main/cLandscape.cc:106-120), neutral range 0
    else if (f < base) { a.neg = 1; a.sn = f; }
    else if (f <= base) a.neut = 1;
    else { a.pos = 1; a.sp = f; a.pf = f; a.pr = r; }
    if (S.site_count || S.chart) {
      const LandEdit u = land_decode(S.base_op + S.base_off[g], S.len[g], S.num_insts, mode, r);
      const int64_t site = S.site_off[g] + land_site(u);
      if (S.site_count && f >= base) atomicAdd(&S.site_count[site], 1);
      if (S.chart) S.chart[site * S.num_insts + u.k1] = f;
    }
  }
  a = land_block_sum(a);
  if (threadIdx.x == 0) S.parts[T] = a;
}

// One block per genome: thread k adds tiles k, k + 256, .. in that order, then
// the block's fixed tree -- a shape that depends on the genome's mutant count alone.
__global__ void __launch_bounds__(LAND_TILE) k_land_rows(LandScratch S, int distance) {
  const int g = blockIdx.x;
  const int64_t nt = S.tile_off[g + 1] - S.tile_off[g];
  LandPart a = land_zero();
  for (int64_t t = threadIdx.x; t < nt; t += LAND_TILE) land_add(a, S.parts[S.tile_off[g] + t]);
  a = land_block_sum(a);
  if (threadIdx.x != 0) return;
  avgpu_landscape& o = S.rows[g];
  o.total_count = S.mut_off[g + 1] - S.mut_off[g];
  o.dead_count = a.dead; o.neg_count = a.neg; o.neut_count = a.neut; o.pos_count = a.pos;
  o.gestations[0] = o.total_count; o.gestations[1] = a.run1; o.gestations[2] = a.run2;
  o.base_fitness = S.base_fit[g]; o.base_merit = S.base_merit[g]; o.base_gestation = S.base_gest[g];
  const bool peak = a.pos > 0;               // ProcessBase: the base is the peak until a mutant beats it
  o.peak_fitness = peak ? a.pf : o.base_fitness;
  o.peak_rank = peak ? a.pr : -1;
  o.total_fitness = a.sf; o.total_sqr_fitness = a.sq; o.pos_size = a.sp; o.neg_size = a.sn;
  o.total_entropy = 0.0; o.complexity = 0.0;   // the host's (log)
  o.distance = distance; o.genome_length = S.len[g]; o.num_insts = S.num_insts;
}

// ---- all-pairs epistasis (cLandscape::TestAllPairs, main/cLandscape.cc:788-825) ----
__device__ __forceinline__ LandEpiPart epi_zero() {
  LandEpiPart a;
  a.sn = a.sp = a.s0 = 0.0;
  a.dead = a.neg = a.pos = a.none = a.run1 = a.run2 = 0;
  return a;
}
__device__ __forceinline__ void epi_add(LandEpiPart& a, const LandEpiPart& b) {
  a.sn = a.sn + b.sn; a.sp = a.sp + b.sp; a.s0 = a.s0 + b.s0;
  a.dead += b.dead; a.neg += b.neg; a.pos += b.pos; a.none += b.none; a.run1 += b.run1; a.run2 += b.run2;
}
__device__ __forceinline__ int64_t epi_shfl(int64_t v, int off) { return (int64_t)__shfl_down((long long)v, off); }
// the same fixed tree as land_block_sum: thread 0 returns the total
__device__ __forceinline__ LandEpiPart epi_block_sum(LandEpiPart a) {
  __shared__ LandEpiPart s_e[4];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    LandEpiPart b;
    b.sn = __shfl_down(a.sn, off); b.sp = __shfl_down(a.sp, off); b.s0 = __shfl_down(a.s0, off);
    b.dead = epi_shfl(a.dead, off); b.neg = epi_shfl(a.neg, off); b.pos = epi_shfl(a.pos, off);
    b.none = epi_shfl(a.none, off); b.run1 = epi_shfl(a.run1, off); b.run2 = epi_shfl(a.run2, off);
    epi_add(a, b);
  }
  if ((threadIdx.x & 63) == 0) s_e[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    LandEpiPart lo = s_e[0], hi = s_e[2];
    epi_add(lo, s_e[1]);
    epi_add(hi, s_e[3]);
    epi_add(lo, hi);
    a = lo;
  }
  return a;
}

// One block per tile of pair mutants (distance-2 ranks), thread k its rank
// 256 t + k: TestMutPair's verdict (:925-946) from the pair's colony fitness,
// the two one-step chart entries and the base fitness (> 0: TestAllPairs :793).
__global__ void __launch_bounds__(LAND_TILE) k_land_epi_reduce(LandScratch S, int64_t m0, int64_t t0) {
  const int64_t T = t0 + blockIdx.x;
  const int g = land_find(S.tile_off, S.n, T);
  const int64_t r = (T - S.tile_off[g]) * LAND_TILE + threadIdx.x;
  LandEpiPart a = epi_zero();
  if (r < S.mut_off[g + 1] - S.mut_off[g]) {
    const int64_t i = S.mut_off[g] + r - m0;
    const double base = S.base_fit[g];
    const int d = S.dep[i];
    const LandEdit u = land_decode(S.base_op + S.base_off[g], S.len[g], S.num_insts, LAND_SUB2, r);
    const double* chart = S.chart + S.site_off[g] * S.num_insts;
    const double combo = S.fit[i] / base;
    const double m1 = chart[(int64_t)u.s1 * S.num_insts + u.k1] / base;
    const double m2 = chart[(int64_t)u.s2 * S.num_insts + u.k2] / base;
    const double mult = m1 * m2;
    a.run1 = d >= 1; a.run2 = d >= 2;
    if ((m1 == 0.0 || m2 == 0.0) && combo == 0.0) a.dead = 1;
    else if (combo < mult) { a.neg = 1; a.sn = combo; }
    else if (combo > mult) { a.pos = 1; a.sp = combo; }
    else { a.none = 1; a.s0 = combo; }
  }
  a = epi_block_sum(a);
  if (threadIdx.x == 0) S.eparts[T] = a;
}

// One block per genome, shaped as k_land_rows
__global__ void __launch_bounds__(LAND_TILE) k_land_epi_rows(LandScratch S) {
  const int g = blockIdx.x;
  const int64_t nt = S.tile_off[g + 1] - S.tile_off[g];
  LandEpiPart a = epi_zero();
  for (int64_t t = threadIdx.x; t < nt; t += LAND_TILE) epi_add(a, S.eparts[S.tile_off[g] + t]);
  a = epi_block_sum(a);
  if (threadIdx.x != 0) return;
  avgpu_epistasis& o = S.erows[g];
  o.total_epi_count = S.mut_off[g + 1] - S.mut_off[g];
  o.dead_epi_count = a.dead; o.neg_epi_count = a.neg; o.pos_epi_count = a.pos; o.no_epi_count = a.none;
  o.gestations[0] = o.total_epi_count; o.gestations[1] = a.run1; o.gestations[2] = a.run2;
  o.neg_epi_size = a.sn; o.pos_epi_size = a.sp; o.no_epi_size = a.s0;
}

}  // namespace

static inline unsigned land_nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_land_seed(const DevWorld& W, const LandScratch& S, hipStream_t s, int mode, int64_t m0, int cnt) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(k_land_seed, dim3(land_nblk(cnt, 64)), dim3(64), 0, s, W, S, mode, m0, cnt);
}
void launch_land_seed_next(const DevWorld& W, const LandScratch& S, hipStream_t s, int depth, int cnt) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(k_land_seed_next, dim3(land_nblk(cnt, 64)), dim3(64), 0, s, W, S, depth, cnt);
}
void launch_land_judge(const DevWorld& W, const LandScratch& S, hipStream_t s, int mode, int depth, int64_t m0,
                       int cnt) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(k_land_judge, dim3(land_nblk(cnt, 4)), dim3(256), 0, s, W, S, mode, depth, m0, cnt);
}
void launch_land_reduce(const LandScratch& S, hipStream_t s, int mode, int64_t m0, int64_t t0, int64_t t1) {
  if (t1 <= t0) return;
  hipLaunchKernelGGL(k_land_reduce, dim3((unsigned)(t1 - t0)), dim3(LAND_TILE), 0, s, S, mode, m0, t0);
}
void launch_land_rows(const LandScratch& S, hipStream_t s, int distance) {
  hipLaunchKernelGGL(k_land_rows, dim3((unsigned)S.n), dim3(LAND_TILE), 0, s, S, distance);
}
void launch_land_epi_reduce(const LandScratch& S, hipStream_t s, int64_t m0, int64_t t0, int64_t t1) {
  if (t1 <= t0) return;
  hipLaunchKernelGGL(k_land_epi_reduce, dim3((unsigned)(t1 - t0)), dim3(LAND_TILE), 0, s, S, m0, t0);
}
void launch_land_epi_rows(const LandScratch& S, hipStream_t s) {
  hipLaunchKernelGGL(k_land_epi_rows, dim3((unsigned)S.n), dim3(LAND_TILE), 0, s, S);
}
