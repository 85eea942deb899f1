// lineage.hip -- the lineage store kept beside the device-resident genotype
// arbiter (include/avida_gpu.h avgpu_enable_lineage):
// one avgpu_lineage_row per genotype ever classified, ascending by id, and an
// arena of the captured birth genomes (canonical codes, 16-B aligned, in id
// order).  avida_amd/systematics.py LineageStore is the specification.
//
// One classification at update u, after arbiter.hip has fixed the ids
// (prev: the state before it, cur: the state after it, both sorted by key):
//   k_lin_deactivate  a thread per prev row: absent from cur -> update_deactivated = u
//   k_lin_append      a thread per cur row with a new id: its store row at
//                     n_old + (id - id0); the parent from pkey[first_cell]
//                     looked up among the prev keys, depth = the parent's + 1
//   k_lin_check       a wave per new row: the key of first_cell's tape prefix;
//                     equal -> its arena size, else unsequenced
//   k_lin_scan        exclusive scan of the sizes (one block) -> arena offsets
//   k_lin_copy        a wave per new row: 16-B copies of the masked codes
// Prune: k_lin_mark_init, k_lin_mark_walk (upward from every active row with an
// integer atomic exchange on the mark word, stopping at a marked row),
// k_lin_flags, two scans, k_lin_compact (a wave per kept row).
// Integers only; the kept set is a closure and ids fix every position, so the
// result does not depend on thread order.
#include <hip/hip_runtime.h>

#include "device.h"

namespace {

constexpr int LB = 256;

__device__ __forceinline__ int64_t lin_find_id(const avgpu_lineage_row* __restrict__ r, int64_t n, int64_t id) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (r[mid].id < id) lo = mid + 1; else hi = mid;
  }
  return (lo < n && r[lo].id == id) ? lo : -1;
}
__device__ __forceinline__ int64_t lin_find_key(const uint64_t* __restrict__ a, int64_t n, uint64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return (lo < n && a[lo] == v) ? lo : -1;
}
__device__ __forceinline__ int64_t lin_align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

__global__ __launch_bounds__(LB) void k_lin_deactivate(const avgpu_arbiter_row* __restrict__ prow,
                                                       const uint64_t* __restrict__ pkey, int64_t np,
                                                       const uint64_t* __restrict__ nkey, int64_t m,
                                                       avgpu_lineage_row* rows, int64_t n, int64_t update) {
  const int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (j >= np) return;
  if (lin_find_key(nkey, m, pkey[j]) >= 0) return;
  const int64_t r = lin_find_id(rows, n, prow[j].id);
  if (r >= 0) rows[r].update_deactivated = update;
}

// (rows[0 .. n_old) are read for the parents' depths while rows[n_old ..) are
// written: no chains among the rows of one classification are resolved)
__global__ __launch_bounds__(LB) void k_lin_append(const avgpu_arbiter_row* __restrict__ nrow,
                                                   const avgpu_genotype* __restrict__ tab, int64_t m,
                                                   const avgpu_arbiter_row* __restrict__ prow,
                                                   const uint64_t* __restrict__ pkey, int64_t np,
                                                   avgpu_lineage_row* rows, int64_t n_old, int64_t id0,
                                                   int64_t n_new, const uint64_t* __restrict__ cell_pkey,
                                                   const int32_t* __restrict__ generation, int64_t ncells,
                                                   int64_t update, unsigned long long* ctr,
                                                   int32_t* __restrict__ newcell) {
  const int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (j >= m) return;
  const int64_t id = nrow[j].id;
  const int64_t slot = id - id0;
  if (slot < 0 || slot >= n_new) return;
  int64_t fc = tab[j].first_cell;
  if (fc < 0 || fc >= ncells) fc = 0;             // (never: the table's cells are the world's)
  const uint64_t key = nrow[j].genotype_key;
  const uint64_t pk = cell_pkey[fc];
  int64_t parent = 0;
  int32_t depth = 0;
  if (pk != 0ull) {
    const int64_t p = lin_find_key(pkey, np, pk);
    const int64_t r = p >= 0 ? lin_find_id(rows, n_old, prow[p].id) : -1;
    if (r >= 0) {
      parent = rows[r].id;
      depth = rows[r].depth + 1;
    } else {
      parent = -1;
      atomicAdd(ctr + LIN_ORPHANS, 1ull);
    }
  }
  avgpu_lineage_row o;
  o.genotype_key = key; o.id = id; o.parent_id = parent; o.seq_off = -1;
  o.update_born = update; o.update_deactivated = -1;
  o.depth = depth; o.genome_length = nrow[j].genome_length; o.gen_born = generation[fc]; o.reserved = 0;
  rows[n_old + slot] = o;
  newcell[slot] = (int32_t)fc;
}

// one wave per new row: does first_cell's tape prefix still hash to the key?
__global__ __launch_bounds__(64) void k_lin_check(const uint8_t* __restrict__ tape, avgpu_lineage_row* nrows,
                                                  int64_t n_new, const int32_t* __restrict__ newcell,
                                                  int64_t* __restrict__ sizes, unsigned long long* ctr) {
  const int64_t s = blockIdx.x;
  if (s >= n_new) return;
  const int lane = threadIdx.x;
  const int len = nrows[s].genome_length;
  const uint64_t key = nrows[s].genotype_key;
  bool ok = len >= 0 && len <= AVGPU_MAX_GENOME;
  uint64_t sum = 0;
  if (ok) {
    const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tape + (int64_t)newcell[s] * TAPE_SLOT);
    for (int w = lane; w < (len + 3) / 4; w += 64) sum += gk_word(t32[w], w, len);
  }
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  ok = ok && gk_final(sum, len) == key;
  if (lane == 0) {
    sizes[s] = ok ? lin_align16(len) : 0;
    nrows[s].seq_off = ok ? 0 : -1;
    if (!ok) atomicAdd(ctr + LIN_UNSEQ, 1ull);
  }
}

// exclusive scan of a[0 .. n) in place, starting at base; *total = base + the sum
__global__ __launch_bounds__(1024) void k_lin_scan(int64_t* a, int64_t n, int64_t base, unsigned long long* total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t lo = min(n, per * t), hi = min(n, lo + per);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; i++) s += a[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = base;
    for (int q = 0; q < 1024; q++) { const int64_t v = part[q]; part[q] = run; run += v; }
    *total = (unsigned long long)run;
  }
  __syncthreads();
  int64_t run = part[t];
  for (int64_t i = lo; i < hi; i++) { const int64_t v = a[i]; a[i] = run; run += v; }
}

// 16-B quads of canonical codes: the flag bits masked, the sites past len zero
__device__ __forceinline__ uint4 lin_codes(uint4 v, int q, int len) {
  uint32_t x[4] = {v.x & 0x3F3F3F3Fu, v.y & 0x3F3F3F3Fu, v.z & 0x3F3F3F3Fu, v.w & 0x3F3F3F3Fu};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int keep = len - 16 * q - 4 * j;
    if (keep <= 0) x[j] = 0u;
    else if (keep < 4) x[j] &= (1u << (8 * keep)) - 1u;
  }
  return make_uint4(x[0], x[1], x[2], x[3]);
}

__global__ __launch_bounds__(64) void k_lin_copy(const uint8_t* __restrict__ tape, avgpu_lineage_row* nrows,
                                                 int64_t n_new, const int32_t* __restrict__ newcell,
                                                 const int64_t* __restrict__ offs, uint8_t* arena,
                                                 int64_t arena_cap) {
  const int64_t s = blockIdx.x;
  if (s >= n_new) return;
  if (nrows[s].seq_off < 0) return;                // wave-uniform
  const int len = nrows[s].genome_length;
  const int64_t off = offs[s];
  if (off < 0 || (off & 15) || off + lin_align16(len) > arena_cap) return;   // (never: the host reserved the total)
  const uint4* src = reinterpret_cast<const uint4*>(tape + (int64_t)newcell[s] * TAPE_SLOT);
  uint4* dst = reinterpret_cast<uint4*>(arena + off);
  for (int q = threadIdx.x; q < (len + 15) / 16; q += 64) dst[q] = lin_codes(src[q], q, len);
  __syncthreads();
  if (threadIdx.x == 0) nrows[s].seq_off = off;
}

__global__ __launch_bounds__(LB) void k_lin_mark_init(const avgpu_lineage_row* __restrict__ rows, int64_t n,
                                                      uint32_t* mark) {
  const int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (j < n) mark[j] = rows[j].update_deactivated < 0 ? 1u : 0u;
}
__global__ __launch_bounds__(LB) void k_lin_mark_walk(const avgpu_lineage_row* __restrict__ rows, int64_t n,
                                                      uint32_t* mark) {
  const int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (j >= n || rows[j].update_deactivated >= 0) return;
  int64_t p = rows[j].parent_id, child = rows[j].id;
  while (p > 0 && p < child) {                     // (parent_id < id: the walk ends)
    const int64_t q = lin_find_id(rows, n, p);
    if (q < 0) break;
    if (atomicExch(mark + q, 1u) != 0u) break;     // marked: its chain is, or will be
    child = p;
    p = rows[q].parent_id;
  }
}
__global__ __launch_bounds__(LB) void k_lin_flags(const avgpu_lineage_row* __restrict__ rows, int64_t n,
                                                  const uint32_t* __restrict__ mark, int64_t* __restrict__ idx,
                                                  int64_t* __restrict__ asz) {
  const int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (j >= n) return;
  const bool k = mark[j] != 0u;
  idx[j] = k ? 1 : 0;
  asz[j] = (k && rows[j].seq_off >= 0) ? lin_align16(rows[j].genome_length) : 0;
}
__global__ __launch_bounds__(64) void k_lin_compact(const avgpu_lineage_row* __restrict__ rows, int64_t n,
                                                    const uint32_t* __restrict__ mark,
                                                    const int64_t* __restrict__ idx, const int64_t* __restrict__ aoff,
                                                    const uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                    avgpu_lineage_row* out, int64_t out_cap, uint8_t* out_arena,
                                                    int64_t out_arena_cap) {
  const int64_t j = blockIdx.x;
  if (j >= n || mark[j] == 0u) return;
  const int64_t d = idx[j];
  if (d < 0 || d >= out_cap) return;
  avgpu_lineage_row r = rows[j];
  if (r.seq_off >= 0) {
    const int64_t sz = lin_align16(r.genome_length), no = aoff[j];
    if (r.seq_off + sz <= arena_bytes && no >= 0 && no + sz <= out_arena_cap) {
      const uint4* src = reinterpret_cast<const uint4*>(arena + r.seq_off);
      uint4* dst = reinterpret_cast<uint4*>(out_arena + no);
      for (int q = threadIdx.x; q < (int)(sz / 16); q += 64) dst[q] = src[q];
      r.seq_off = no;
    } else {
      r.seq_off = -1;                              // (never: offsets are the store's own)
    }
  }
  if (threadIdx.x == 0) out[d] = r;
}
__global__ __launch_bounds__(LB) void k_lin_max_depth(const avgpu_lineage_row* __restrict__ rows, int64_t n,
                                                      unsigned long long* ctr) {
  const int64_t j = (int64_t)blockIdx.x * LB + threadIdx.x;
  if (j < n && rows[j].depth > 0) atomicMax(ctr + LIN_MAXDEPTH, (unsigned long long)rows[j].depth);
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + LB - 1) / LB); }

}  // namespace

void launch_lineage_classify(const LinScratch& L, const ArbScratch& A, const DevWorld& W, int64_t n_prev, int64_t m,
                             int64_t id0, int64_t n_new, int64_t update, hipStream_t s) {
  const int cur = A.cur, prv = A.cur ^ 1;          // (after the classification's swap)
  if (n_prev > 0 && L.n > 0)
    k_lin_deactivate<<<blocks_of(n_prev), LB, 0, s>>>(A.row[prv], A.key[prv], n_prev, A.key[cur], m, L.rows, L.n,
                                                      update);
  if (n_new <= 0 || m <= 0) return;
  k_lin_append<<<blocks_of(m), LB, 0, s>>>(A.row[cur], A.table, m, A.row[prv], A.key[prv], n_prev, L.rows, L.n, id0,
                                           n_new, W.pkey, W.generation, W.n, update, L.ctr, L.newcell);
  k_lin_check<<<(unsigned)n_new, 64, 0, s>>>(W.tape, L.rows + L.n, n_new, L.newcell, L.idx, L.ctr);
  k_lin_scan<<<1, 1024, 0, s>>>(L.idx, n_new, L.arena_bytes, L.ctr + LIN_TOTAL_A);
}
void launch_lineage_copy(const LinScratch& L, const DevWorld& W, int64_t n_new, hipStream_t s) {
  if (n_new <= 0) return;
  k_lin_copy<<<(unsigned)n_new, 64, 0, s>>>(W.tape, L.rows + L.n, n_new, L.newcell, L.idx, L.arena, L.arena_cap);
}
void launch_lineage_mark(const LinScratch& L, hipStream_t s) {
  if (L.n <= 0) return;
  k_lin_mark_init<<<blocks_of(L.n), LB, 0, s>>>(L.rows, L.n, L.mark);
  k_lin_mark_walk<<<blocks_of(L.n), LB, 0, s>>>(L.rows, L.n, L.mark);
  k_lin_flags<<<blocks_of(L.n), LB, 0, s>>>(L.rows, L.n, L.mark, L.idx, L.asz);
  k_lin_scan<<<1, 1024, 0, s>>>(L.idx, L.n, 0, L.ctr + LIN_TOTAL_A);
  k_lin_scan<<<1, 1024, 0, s>>>(L.asz, L.n, 0, L.ctr + LIN_TOTAL_B);
}
void launch_lineage_compact(const LinScratch& L, avgpu_lineage_row* out, int64_t out_cap, uint8_t* out_arena,
                            int64_t out_arena_cap, hipStream_t s) {
  if (L.n <= 0) return;
  k_lin_compact<<<(unsigned)L.n, 64, 0, s>>>(L.rows, L.n, L.mark, L.idx, L.asz, L.arena, L.arena_bytes, out, out_cap,
                                             out_arena, out_arena_cap);
}
void launch_lineage_max_depth(const LinScratch& L, hipStream_t s) {
  if (L.n > 0) k_lin_max_depth<<<blocks_of(L.n), LB, 0, s>>>(L.rows, L.n, L.ctr);
}
