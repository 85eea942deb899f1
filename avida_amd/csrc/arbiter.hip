// arbiter.hip -- the device-resident genotype arbiter (include/avida_gpu.h
// avgpu_classify_genotypes): the genotype table of
// genotypes.hip classified against the previous update's state, both sorted by
// key.
//
//   k_arb_begin    the grouping's totals into the summary; the counters reset
//   k_arb_match    one thread per table row: binary search among the previous
//                  keys, the carried (or new) state row, the total; the sort
//                  key of the id ranking (first_cell of a new row)
//   sort           launch_genotype_sort, 4 passes: new rows ascending by first cell
//   k_arb_ids      new row of rank r takes id next_id + r
//   k_arb_best     the lowest id among the rows at the top abundance
//   k_arb_stay     one thread: does the previous dominant stay?
//   k_arb_cross    the dominant's row; the crossing rows' sort key
//                  (genome_length, id)
//   sort           launch_genotype_sort over (genome_length, id)
//   k_arb_name<0>  name_no = the size's counter + the place within the size's run + 1
//   k_arb_name<1>  the run's last row advances the size's counter
//   k_arb_finish   one thread: the world-level state and the summary
//
// Integers only: sums and counts go through integer atomics (exact in any
// order), ranks come from sorts over distinct keys, so the state is a
// function of the table sequence alone.
#include <hip/hip_runtime.h>

#include "device.h"

namespace {

constexpr int AB = 256;
constexpr uint64_t SORT_LAST = ~0ull;              // sorts behind every ranked row
constexpr unsigned long long ID_NONE = ~0ull;

// first position in a[0 .. n) whose value is not below v
__device__ __forceinline__ int64_t arb_lower_bound(const uint64_t* __restrict__ a, int64_t n, uint64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ unsigned long long arb_wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}

__global__ __launch_bounds__(64) void k_arb_begin(const avgpu_genotype_totals* __restrict__ tot, ArbWork* wk,
                                                  avgpu_arbiter_summary* out, int64_t update) {
  if (threadIdx.x != 0) return;
  wk->top = 0; wk->pad = 0;
  wk->best_id = ID_NONE;
  wk->num_new = 0; wk->num_matched = 0; wk->num_crossed = 0; wk->num_thr = 0;
  wk->stay_row = -1; wk->dom_row = -1;
  out->update = update;
  out->num_organisms = tot->num_organisms;
  out->num_genotypes = tot->num_genotypes;
  out->sum_copied_size = tot->sum_copied_size;
  out->sum_executed_size = tot->sum_executed_size;
}

__global__ __launch_bounds__(AB) void k_arb_match(const avgpu_genotype* __restrict__ tab, int64_t m,
                                                  const uint64_t* __restrict__ pkey,
                                                  const avgpu_arbiter_row* __restrict__ prow, int64_t np,
                                                  int64_t update, uint64_t* __restrict__ nkey,
                                                  avgpu_arbiter_row* __restrict__ nrow, uint64_t* __restrict__ skey,
                                                  ArbWork* wk) {
  __shared__ int s_top[AB / 64];
  __shared__ unsigned long long s_new[AB / 64], s_old[AB / 64];
  const int64_t j = (int64_t)blockIdx.x * AB + threadIdx.x;
  int units = 0;
  unsigned long long fresh = 0, old = 0;
  if (j < m) {
    const uint64_t k = tab[j].genotype_key;
    units = tab[j].num_units;
    const int64_t p = arb_lower_bound(pkey, np, k);
    avgpu_arbiter_row r;
    int prev = 0;
    if (p < np && pkey[p] == k) {
      r = prow[p];
      prev = r.num_units;
      old = 1;
    } else {
      r.genotype_key = k;
      r.id = 0; r.update_born = update; r.total_units = 0;
      r.genome_length = tab[j].genome_length;
      r.name_no = 0; r.threshold = 0;
      fresh = 1;
    }
    r.num_units = units;
    r.total_units += units > prev ? units - prev : 0;
    nrow[j] = r;
    nkey[j] = k;
    skey[j] = fresh ? (uint64_t)tab[j].first_cell : 0xFFFFFFFFull;
  }
  int top = units;
  for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_down(top, off));
  fresh = arb_wave_sum(fresh);
  old = arb_wave_sum(old);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { s_top[wv] = top; s_new[wv] = fresh; s_old[wv] = old; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < AB / 64; q++) { top = max(top, s_top[q]); fresh += s_new[q]; old += s_old[q]; }
    atomicMax(&wk->top, top);
    if (fresh) atomicAdd(&wk->num_new, fresh);
    if (old) atomicAdd(&wk->num_matched, old);
  }
}

// sidx[r]: the table row of the new genotype with the r-th lowest first cell
__global__ __launch_bounds__(AB) void k_arb_ids(const int32_t* __restrict__ sidx, int64_t m,
                                                const ArbWork* __restrict__ wk, const ArbState* __restrict__ st,
                                                avgpu_arbiter_row* __restrict__ nrow) {
  const int64_t r = (int64_t)blockIdx.x * AB + threadIdx.x;
  if (r >= m || (unsigned long long)r >= wk->num_new) return;
  const int64_t j = sidx[r];
  if (j >= 0 && j < m) nrow[j].id = st->next_id + r;
}

__global__ __launch_bounds__(AB) void k_arb_best(const avgpu_arbiter_row* __restrict__ nrow, int64_t m,
                                                 ArbWork* wk) {
  const int64_t j = (int64_t)blockIdx.x * AB + threadIdx.x;
  unsigned long long v = ID_NONE;
  if (j < m && nrow[j].num_units == wk->top) v = (unsigned long long)nrow[j].id;
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long y = __shfl_down(v, off);
    v = y < v ? y : v;
  }
  if ((threadIdx.x & 63) == 0 && v != ID_NONE) atomicMin(&wk->best_id, v);
}

__global__ __launch_bounds__(64) void k_arb_stay(const uint64_t* __restrict__ nkey,
                                                 const avgpu_arbiter_row* __restrict__ nrow, int64_t m,
                                                 const ArbState* __restrict__ st, ArbWork* wk) {
  if (threadIdx.x != 0) return;
  int64_t stay = -1;
  const uint64_t k = st->best_key;
  if (k != 0) {
    const int64_t p = arb_lower_bound(nkey, m, k);
    if (p < m && nkey[p] == k && nrow[p].num_units == wk->top) stay = p;
  }
  wk->stay_row = stay;
}

__global__ __launch_bounds__(AB) void k_arb_cross(const avgpu_arbiter_row* __restrict__ nrow, int64_t m,
                                                  int32_t threshold, int id_bits, ArbWork* wk,
                                                  uint64_t* __restrict__ skey) {
  __shared__ unsigned long long s_cross[AB / 64], s_thr[AB / 64];
  const int64_t j = (int64_t)blockIdx.x * AB + threadIdx.x;
  unsigned long long cross = 0, thr = 0;
  if (j < m) {
    const int units = nrow[j].num_units;
    const int64_t id = nrow[j].id;
    const int64_t stay = wk->stay_row;
    const bool dom = stay >= 0 ? j == stay : (units == wk->top && (unsigned long long)id == wk->best_id);
    if (dom) wk->dom_row = j;
    const bool had = nrow[j].threshold != 0;
    const bool c = !had && (units >= threshold || dom);
    skey[j] = c ? ((uint64_t)(uint32_t)nrow[j].genome_length << id_bits) | (uint64_t)id : SORT_LAST;
    cross = c ? 1 : 0;
    thr = (c || had) ? 1 : 0;
  }
  cross = arb_wave_sum(cross);
  thr = arb_wave_sum(thr);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { s_cross[wv] = cross; s_thr[wv] = thr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < AB / 64; q++) { cross += s_cross[q]; thr += s_thr[q]; }
    if (cross) atomicAdd(&wk->num_crossed, cross);
    if (thr) atomicAdd(&wk->num_thr, thr);
  }
}

// skey[0 .. num_crossed): the crossing rows ascending by (genome_length, id)
template <bool COMMIT>
__global__ __launch_bounds__(AB) void k_arb_name(const uint64_t* __restrict__ skey, const int32_t* __restrict__ sidx,
                                                 int64_t m, int id_bits, const ArbWork* __restrict__ wk,
                                                 int64_t* __restrict__ sz_count,
                                                 avgpu_arbiter_row* __restrict__ nrow) {
  const int64_t r = (int64_t)blockIdx.x * AB + threadIdx.x;
  const int64_t nc = (int64_t)wk->num_crossed;
  if (r >= m || r >= nc) return;
  const uint64_t len = skey[r] >> id_bits;
  if (len > AVGPU_MAX_GENOME) return;
  const int64_t start = arb_lower_bound(skey, nc, len << id_bits);
  if (!COMMIT) {
    const int64_t j = sidx[r];
    if (j < 0 || j >= m) return;
    nrow[j].threshold = 1;
    nrow[j].name_no = (int32_t)(sz_count[len] + (r - start) + 1);
  } else if (r + 1 == nc || (skey[r + 1] >> id_bits) != len) {
    sz_count[len] += r - start + 1;
  }
}

__global__ __launch_bounds__(64) void k_arb_finish(const avgpu_genotype* __restrict__ tab,
                                                   const avgpu_arbiter_row* __restrict__ nrow, int64_t m,
                                                   int64_t np, ArbState* st, const ArbWork* __restrict__ wk,
                                                   avgpu_arbiter_summary* out) {
  if (threadIdx.x != 0) return;
  const int64_t fresh = (int64_t)wk->num_new, crossed = (int64_t)wk->num_crossed;
  st->next_id += fresh;
  st->tot_genotypes += fresh;
  st->tot_threshold += crossed;
  const int64_t dom = m > 0 ? wk->dom_row : -1;
  st->best_key = dom >= 0 ? nrow[dom].genotype_key : 0ull;
  out->num_threshold = (int64_t)wk->num_thr;
  out->tot_genotypes = st->tot_genotypes;
  out->tot_threshold = st->tot_threshold;
  out->next_id = st->next_id;
  out->num_new = fresh;
  out->num_gone = np - (int64_t)wk->num_matched;
  out->num_crossed = crossed;
  out->dominant_row = dom;
  uint64_t* ds = reinterpret_cast<uint64_t*>(&out->dominant_state);
  uint64_t* dt = reinterpret_cast<uint64_t*>(&out->dominant);
  const uint64_t* ss = dom >= 0 ? reinterpret_cast<const uint64_t*>(nrow + dom) : nullptr;
  const uint64_t* ts = dom >= 0 ? reinterpret_cast<const uint64_t*>(tab + dom) : nullptr;
  for (int q = 0; q < (int)(sizeof(avgpu_arbiter_row) / 8); q++) ds[q] = ss ? ss[q] : 0ull;
  for (int q = 0; q < (int)(sizeof(avgpu_genotype) / 8); q++) dt[q] = ts ? ts[q] : 0ull;
}

}  // namespace

void launch_arbiter_begin(const ArbScratch& A, const GtScratch& S, int64_t update, hipStream_t s) {
  k_arb_begin<<<1, 64, 0, s>>>(S.totals, A.work, A.d_sum, update);
}

void launch_arbiter_classify(const ArbScratch& A, const GtScratch& S, const avgpu_genotype* d_tab, int64_t m,
                             int64_t n_prev, int64_t update, int32_t threshold, int id_bits, hipStream_t s) {
  const int nxt = A.cur ^ 1;
  avgpu_arbiter_row* nrow = A.row[nxt];
  if (m > 0) {
    const unsigned nb = (unsigned)((m + AB - 1) / AB);
    k_arb_match<<<nb, AB, 0, s>>>(d_tab, m, A.key[A.cur], A.row[A.cur], n_prev, update, A.key[nxt], nrow, S.key[0],
                                  A.work);
    launch_genotype_sort(S, m, 4, s);             // first cells are below 2^31
    k_arb_ids<<<nb, AB, 0, s>>>(S.cell[0], m, A.work, A.state, nrow);
    k_arb_best<<<nb, AB, 0, s>>>(nrow, m, A.work);
    k_arb_stay<<<1, 64, 0, s>>>(A.key[nxt], nrow, m, A.state, A.work);
    k_arb_cross<<<nb, AB, 0, s>>>(nrow, m, threshold, id_bits, A.work, S.key[0]);
    // genome_length takes 12 bits above the id
    int passes = (id_bits + 12 + 7) / 8;
    passes += passes & 1;
    launch_genotype_sort(S, m, passes, s);
    k_arb_name<false><<<nb, AB, 0, s>>>(S.key[0], S.cell[0], m, id_bits, A.work, A.sz_count, nrow);
    k_arb_name<true><<<nb, AB, 0, s>>>(S.key[0], S.cell[0], m, id_bits, A.work, A.sz_count, nrow);
  }
  k_arb_finish<<<1, 64, 0, s>>>(d_tab, nrow, m, n_prev, A.state, A.work, A.d_sum);
}
