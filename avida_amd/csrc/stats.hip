// stats.hip -- the update's statistics (cStats reduction inputs):
//   k_stats_partial  per-256-cell-block partials of the population's sums
//   k_stats_final    one block per slot over the partials; the counter shards
#include "device.h"

#pragma clang fp contract(off)

namespace {

// wave reductions: every lane gets the result
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// (the slots: device.h ST_*; the first NUSED of them have a partial row; part
// layout [NPART][nb] so that k_stats_final reads it coalesced)
// Integer-valued slots (organisms, gestation, genome length, generation,
// memory, task organisms) reduce as integers: their double sums are exact in
// any order, so the partials are the same numbers at a third of the shuffle
// work; the nine task flags go as one u64 of 7-bit lanes (<= 64 per wave).
__global__ __launch_bounds__(256) void k_stats_partial(DevWorld W, double* part) {
  __shared__ double s[4][NPART];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double merit = 0.0, fit = 0.0;
  int iv[5] = {0, 0, 0, 0, 0};                 // ST_ORGS, _GESTATION, _GENOME_LEN, _GENERATION, _MEM_SIZE
  unsigned long long tasks = 0;
  if (c < W.n && (W.ctl[c] & CTL_ALIVE)) {
    merit = W.merit[c];
    fit = W.fitness[c];
    iv[0] = 1;
    iv[1] = W.gest_time[c];
    iv[2] = W.birth_len[c];
    iv[3] = W.generation[c];
    iv[4] = W.mem_size[c];
#pragma unroll
    for (int t = 0; t < AVGPU_NUM_LOGIC_TASKS; t++)
      tasks |= (W.last_task[t * W.n + c] > 0 ? 1ull : 0ull) << (7 * t);
  }
  const double rm = wave_sum(merit), rf = wave_sum(fit), rx = wave_max(fit);
  int ri[5];
#pragma unroll
  for (int k = 0; k < 5; k++) ri[k] = wave_sum(iv[k]);
  const unsigned long long rt = wave_sum(tasks);
  if (lane == 0) {
    s[wv][ST_ORGS] = (double)ri[0]; s[wv][ST_MERIT] = rm; s[wv][ST_FITNESS] = rf;
    s[wv][ST_GESTATION] = (double)ri[1]; s[wv][ST_GENOME_LEN] = (double)ri[2]; s[wv][ST_MAX_FITNESS] = rx;
    s[wv][ST_GENERATION] = (double)ri[3]; s[wv][ST_MEM_SIZE] = (double)ri[4];
#pragma unroll
    for (int t = 0; t < AVGPU_NUM_LOGIC_TASKS; t++) s[wv][ST_TASK0 + t] = (double)((rt >> (7 * t)) & 127ull);
  }
  __syncthreads();
  // only the NUSED slots carry data (the rest of the NPART rows are never
  // written and k_stats_final reports them as 0)
  if (threadIdx.x < NUSED) {
    const int k = threadIdx.x;
    double r = s[0][k];
    for (int q = 1; q < 4; q++) r = (k == ST_MAX_FITNESS) ? fmax(r, s[q][k]) : r + s[q][k];
    part[(int64_t)k * gridDim.x + blockIdx.x] = r;
  }
}

// out: the statistics vector's NSTAT slots (device.h ST_*).
// Block k < NPART reduces partial row k (256 lanes, fixed order: lane t sums
// entries t, t+256, ..., then a pairwise tree); block NPART sums the counter
// shards.
__global__ __launch_bounds__(256) void k_stats_final(DevWorld W, const double* part, int64_t nb,
                                                     double* out) {
  __shared__ double sd[256];
  constexpr int NG = 256 / CNT_STRIDE;          // groups of shards the block sums in parallel
  __shared__ unsigned long long cs[NG][CNT_STRIDE];
  const int tid = threadIdx.x;
  const int k = blockIdx.x;
  if (k >= NUSED && k < NPART) {
    if (tid == 0) out[k] = 0.0;
    return;
  }
  if (k < NPART) {
    const bool mx = k == ST_MAX_FITNESS;
    double acc = 0.0;
    for (int64_t b = tid; b < nb; b += 256) {
      const double o = part[(int64_t)k * nb + b];
      acc = mx ? fmax(acc, o) : acc + o;
    }
    sd[tid] = acc;
    __syncthreads();
    for (int stride = 128; stride >= 1; stride >>= 1) {
      if (tid < stride) sd[tid] = mx ? fmax(sd[tid], sd[tid + stride]) : sd[tid] + sd[tid + stride];
      __syncthreads();
    }
    if (tid == 0) out[k] = sd[0];
    return;
  }
  {
    const int slot = tid & (CNT_STRIDE - 1), g = tid / CNT_STRIDE;
    unsigned long long a = 0;
    for (int sh = g; sh < NSHARD; sh += NG) a += W.counters[sh * CNT_STRIDE + slot];
    cs[g][slot] = a;
  }
  __syncthreads();
  // the running sums take this update's counts once: here, or (statistics
  // never asked for) in the next reset_counts_block
  const bool fold = W.counters[CNT_CUM_FLAG] == 0ull;
  __syncthreads();
  if (tid < CNT_STRIDE) {
    unsigned long long t = 0;
    for (int g = 0; g < NG; g++) t += cs[g][tid];
    cs[0][tid] = t;
    if (tid == CNT_STRIDE - 1) W.counters[CNT_CUM_FLAG] = 1ull;
    else if (fold) W.counters[CNT_CUM_BASE + tid] += t;
  }
  __syncthreads();
  if (tid == 0) {
    out[ST_INSTS] = (double)cs[0][AVGPU_CNT_INSTS];
    out[ST_DEATHS] = (double)cs[0][AVGPU_CNT_DEATHS];
    out[ST_DIVIDES] = (double)cs[0][AVGPU_CNT_DIVIDES];
    out[ST_BIRTHS] = (double)cs[0][AVGPU_CNT_BIRTHS];
    out[ST_DROPPED] = (double)cs[0][AVGPU_CNT_DROPPED];
    out[ST_SPILLS] = (double)cs[0][AVGPU_CNT_SPILLS];
    out[ST_CUM_INSTS] = (double)W.counters[CNT_CUM_INSTS];
    out[ST_CUM_BIRTHS] = (double)W.counters[CNT_CUM_BIRTHS];
    out[ST_SLICES] = (double)cs[0][AVGPU_CNT_SLICES];
    out[ST_LANESTEPS] = (double)cs[0][AVGPU_CNT_LANESTEPS];
    out[ST_OVERWRITTEN] = (double)cs[0][AVGPU_CNT_OVERWRITTEN];
    out[ST_CANCELLED] = (double)cs[0][AVGPU_CNT_CANCELLED];
    out[ST_WASTED] = (double)cs[0][AVGPU_CNT_WASTED];
    out[ST_PRED] = __longlong_as_double(pacc_sum(W, PACC_WEIGHT));
    out[ST_CARRY] = __longlong_as_double(W.sched[SCHED_CARRY] + W.sched[SCHED_CARRY_REM]);
    out[ST_PRED_ORGS] = W.totals[TOT_ORGS];
    out[ST_PRED_DENSEST] = __longlong_as_double(densest_quarter(W));
    for (int q = 0; q < 4; q++) out[ST_QUARTER0 + q] = __longlong_as_double(quarter_count(W, q));
  }
}

}  // namespace

// ---------------------------------------------------------------------------
void launch_stats(const DevWorld& W, hipStream_t s, double* stats) {
  const int64_t nb = (W.n + 255) / 256;
  double* part = stats + NSTAT;
  hipLaunchKernelGGL(k_stats_partial, dim3((unsigned)nb), dim3(256), 0, s, W, part);
  hipLaunchKernelGGL(k_stats_final, dim3(NPART + 1), dim3(256), 0, s, W, part, nb, stats);
}
