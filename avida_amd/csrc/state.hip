// state.hip -- organisms and their state in and out of a world:
//   k_set_orgs       cPopulation::Inject / ActivateOrganism + cPhenotype::SetupInject
//   k_get_states     cHardwareBase inspection API (trace tuple gather)
//   k_set_states     checkpoint restore, its inverse
//   k_state_digest   the per-cell digest of that tuple and the tape
//   k_census, k_parent_keys  the systematics census rows and the parent keys
//   k_classify_uniform  budget + LDS size-class lists for k_interpret
// Paths are relative to avida-core/source/ of the reference.
#include "device.h"

#pragma clang fp contract(off)

namespace {

// Append `cell` to its size-class list (rows 1..3).  Class 0 is not listed:
// k_interpret<CLASS0_SIZE> sweeps the cells densely.  Block-aggregated: one
// global atomic per class and block (a per-wave atomic on three addresses
// serialised ~16K waves in L2), lanes then write at block base + wave offset
// + rank.  blockDim.x must be 64 * WAVES.
template <int WAVES = 4>
__device__ __forceinline__ void enqueue_class(const DevWorld& W, int cell, bool want, int cls) {
  __shared__ int s_pc[NUM_CLASSES][WAVES], s_base[NUM_CLASSES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long masks[NUM_CLASSES];
  __syncthreads();                             // s_pc / s_base free (repeat calls)
#pragma unroll
  for (int k = 1; k < NUM_CLASSES; k++) {
    masks[k] = __ballot(want && cls == k);
    if (lane == 0) s_pc[k][wv] = __popcll(masks[k]);
  }
  __syncthreads();
  // waves take their offsets in wave order (deterministic list order)
  if (threadIdx.x > 0 && threadIdx.x < NUM_CLASSES) {
    const int k = threadIdx.x;
    int tot = 0;
    for (int w = 0; w < WAVES; w++) tot += s_pc[k][w];
    s_base[k] = tot ? atomicAdd(&W.class_count[k], tot) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 1; k < NUM_CLASSES; k++) {
    if (want && cls == k) {
      int woff = 0;
      for (int w = 0; w < wv; w++) woff += s_pc[k][w];
      const int rank = __popcll(masks[k] & ((1ull << lane) - 1ull));
      W.class_list[(int64_t)k * W.n + s_base[k] + woff + rank] = cell;
    }
  }
}

__device__ __forceinline__ int need_of_cell(const DevWorld& W, int cell) {
  return ::need_of(W.mem_size[cell], W.ctl[cell], W.size_range);
}

// ---------------------------------------------------------------------------
__global__ void k_set_orgs(DevWorld W, int64_t first, int64_t count, const uint8_t* codes,
                           const int32_t* offsets, const int32_t* lens, const double* merits,
                           const int32_t* inputs, int deterministic) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t c = first + i;
  const int len = lens[i];
  const uint8_t* g = codes + offsets[i];
  uint8_t* t = W.tape + c * TAPE_SLOT;
  for (int k = 0; k < len; k++) t[k] = g[k] & CODE_MASK;
  inject_org(W, c, len, merits ? merits[i] : 0.0, inputs ? inputs + 3 * i : nullptr, deterministic);
}

// the cHardwareBase inspection tuple of cell c (zero padding: the digest below
// hashes its bytes)
__device__ void build_state(const DevWorld& W, int64_t c, avgpu_cpu_state& s) {
  const int64_t N = W.n;
  memset(&s, 0, sizeof(s));
  const bool fresh = (W.ctl[c] & CTL_FRESH) != 0;   // birth values implied (setup_child)
  const int32_t* x = W.xs + c * XS_WORDS;
  if (!fresh) {
  for (int k = 0; k < 3; k++) s.reg[k] = x[XS_REG + k];
  for (int k = 0; k < 4; k++) s.head[k] = x[XS_HEAD + k];
  for (int k = 0; k < 2; k++)
    for (int j = 0; j < AVGPU_STACK_SIZE; j++) s.stack[k][j] = x[XS_STACK + k * AVGPU_STACK_SIZE + j];
  }
  const uint32_t ctl = W.ctl[c];
  s.stack_ptr[0] = CTL_SP0(ctl); s.stack_ptr[1] = CTL_SP1(ctl);
  s.cur_stack = (ctl & CTL_CURSTK) ? 1 : 0;
  s.mal_active = (ctl & CTL_MAL) ? 1 : 0;
  s.alive = (ctl & CTL_ALIVE) ? 1 : 0;
  const uint32_t rl = fresh ? 0u : (uint32_t)x[XS_RLABEL];
  s.read_label_len = rl & 15;
  for (int k = 0; k < (int)(rl & 15); k++) s.read_label[k] = (int8_t)((rl >> (4 + 2 * k)) & 3);
  s.mem_size = W.mem_size[c];
  s.cpu_cycles_used = fresh ? 0 : x[XS_CYCLES];
  s.time_used = fresh ? 0 : x[XS_TIME];
  s.gestation_start = fresh ? 0 : x[XS_GEST];
  s.gestation_time = W.gest_time[c];
  s.num_divides = fresh ? 0 : W.num_div[c];
  s.generation = W.generation[c];
  s.genome_length = W.birth_len[c];
  s.copied_size = W.copied[c];
  s.child_copied_size = fresh ? 0 : W.child_copied[c];
  s.executed_size = W.executed[c];
  s.max_executed = W.max_exec[c];
  s.birth_length = W.birth_len[c];
  s.input_ptr = fresh ? 0 : x[XS_INPTR];
  const int tot = fresh ? 0 : x[XS_INTOT];
  for (int k = 0; k < 3; k++) s.input_buf[k] = (k < tot) ? x[XS_INBUF + k] : 0;
  s.input_total = tot;
  s.output_total = fresh ? 0 : x[XS_OUTTOT];
  s.output_buf = s.output_total ? x[XS_OUTBUF] : 0;
  for (int k = 0; k < 3; k++) s.inputs[k] = W.inputs[k * N + c];
  // task counts past the logic-9 tasks stay 0 (no reaction can count them)
  for (int k = 0; k < AVGPU_MAX_REACTIONS && !fresh; k++) {
    s.cur_task_count[k] = k < AVGPU_NUM_LOGIC_TASKS ? x[XS_TASK + k] : 0;
    s.cur_reaction_count[k] = k < XS_NREACT ? x[XS_REACT + k] : W.cur_react[k * N + c];
  }
  for (int k = 0; k < AVGPU_MAX_REACTIONS; k++)   // a fresh offspring's were set at activation
    s.last_task_count[k] = (fresh && k >= AVGPU_NUM_LOGIC_TASKS) ? 0 : W.last_task[k * N + c];
  s.rng_key_lo = W.rng[c]; s.rng_key_hi = W.rng[N + c]; s.rng_counter = W.rng[2 * N + c];
  s.errors = fresh ? 0 : x[XS_ERRORS];
  s.cur_bonus = fresh ? W.default_bonus : *reinterpret_cast<const double*>(x + XS_BONUS);
  s.merit = W.merit[c];
  s.fitness = W.fitness[c];
  s.credit = W.credit[c];
  s.head_start = CTL_HS(ctl);
  s.age = W.track_age ? W.age[c] + 1 : 0;   // as UpdateOrganismStats leaves it at the update's end
}

__global__ void k_get_states(DevWorld W, int64_t first, int64_t count, avgpu_cpu_state* out,
                             uint8_t* codes, int cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t c = first + i;
  avgpu_cpu_state s;
  build_state(W, c, s);
  out[i] = s;
  if (codes) {
    const uint8_t* t = W.tape + c * TAPE_SLOT;
    uint8_t* d = codes + i * cap;
    const int m = s.mem_size < cap ? s.mem_size : cap;
    for (int k = 0; k < m; k++) d[k] = t[k];
  }
}

// Per-cell state digest (include/avida_gpu.h avgpu_state_digests): a chained
// 64-bit mix over the 32-bit words of the inspection tuple, then over the
// memory tape in canonical bytes (handler id | copied << 6 | executed << 7, 4
// sites per word, sites >= mem_size zero).  oracle/oracle.cc restates it on its
// own state, so GPU and oracle worlds of any size compare digest for digest.
__global__ void k_state_digest(DevWorld W, int64_t first, int64_t count, uint64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t c = first + i;
  avgpu_cpu_state s;
  build_state(W, c, s);
  if (s.birth_length == 0) { out[i] = 0; return; }   // never occupied
  uint32_t w[sizeof(s) / 4];
  memcpy(w, &s, sizeof(s));              // the record's bytes (no type-punned loads)
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int k = 0; k < (int)(sizeof(s) / 4); k++) h = gk_mix(h ^ ((uint64_t)k << 32 | w[k]));
  const uint32_t* t = reinterpret_cast<const uint32_t*>(W.tape + c * TAPE_SLOT);
  const int m = min(max(s.mem_size, 0), TAPE_SLOT);
  for (int k = 0; k < (m + 3) / 4; k++) {
    uint32_t v = t[k];
    const int keep = m - 4 * k;
    if (keep < 4) v &= (1u << (8 * keep)) - 1u;
    h = gk_mix(h ^ ((uint64_t)(0x10000 + k) << 32 | v));
  }
  out[i] = h;
}

// checkpoint restore: the inverse of k_get_states; `codes` holds device codes
// with the TF_* flag bits, cap bytes per cell
__global__ void k_set_states(DevWorld W, int64_t first, int64_t count, const avgpu_cpu_state* in,
                             const uint8_t* codes, int cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t N = W.n;
  const int64_t c = first + i;
  const avgpu_cpu_state s = in[i];
  if (W.track_age) W.age[c] = s.age - 1;
  int32_t* x = W.xs + c * XS_WORDS;
  for (int k = 0; k < XS_WORDS; k++) x[k] = 0;
  for (int k = 0; k < 3; k++) x[XS_REG + k] = s.reg[k];
  for (int k = 0; k < 4; k++) x[XS_HEAD + k] = s.head[k];
  for (int k = 0; k < 2; k++)
    for (int j = 0; j < AVGPU_STACK_SIZE; j++) x[XS_STACK + k * AVGPU_STACK_SIZE + j] = s.stack[k][j];
  W.ctl[c] = (uint32_t)(s.stack_ptr[0] & 0xF) | ((uint32_t)(s.stack_ptr[1] & 0xF) << 4) |
             (s.cur_stack ? CTL_CURSTK : 0u) | (s.mal_active ? CTL_MAL : 0u) | (s.alive ? CTL_ALIVE : 0u) |
             ((s.head_start & 0x1FFFFu) << CTL_HS_SHIFT);
  uint32_t rl = (uint32_t)(s.read_label_len & 15);
  for (int k = 0; k < (s.read_label_len & 15) && k < AVGPU_MAX_LABEL; k++)
    rl |= (uint32_t)(s.read_label[k] & 3) << (4 + 2 * k);
  x[XS_RLABEL] = (int32_t)rl;
  W.mem_size[c] = s.mem_size;
  x[XS_CYCLES] = s.cpu_cycles_used; x[XS_TIME] = s.time_used; x[XS_GEST] = s.gestation_start;
  W.gest_time[c] = s.gestation_time; W.num_div[c] = s.num_divides; W.generation[c] = s.generation;
  W.birth_len[c] = s.birth_length;
  W.copied[c] = s.copied_size; W.child_copied[c] = s.child_copied_size; W.executed[c] = s.executed_size;
  W.max_exec[c] = s.max_executed;
  x[XS_INPTR] = s.input_ptr;
  for (int k = 0; k < 3; k++) x[XS_INBUF + k] = s.input_buf[k];
  x[XS_INTOT] = s.input_total;
  x[XS_OUTBUF] = s.output_buf; x[XS_OUTTOT] = s.output_total;
  for (int k = 0; k < 3; k++) W.inputs[k * N + c] = s.inputs[k];
  for (int k = 0; k < AVGPU_MAX_REACTIONS; k++) {
    if (k < AVGPU_NUM_LOGIC_TASKS) x[XS_TASK + k] = s.cur_task_count[k];
    W.last_task[k * N + c] = s.last_task_count[k];
    if (k < XS_NREACT) x[XS_REACT + k] = s.cur_reaction_count[k];
    else W.cur_react[k * N + c] = s.cur_reaction_count[k];
  }
  W.rng[c] = s.rng_key_lo; W.rng[N + c] = s.rng_key_hi; W.rng[2 * N + c] = s.rng_counter;
  if (W.rec_off) W.rec_off[c] = -1;   // restored organisms draw from counter streams
  x[XS_ERRORS] = s.errors;
  *reinterpret_cast<double*>(x + XS_BONUS) = s.cur_bonus;
  W.merit[c] = s.merit; W.fitness[c] = s.fitness; W.credit[c] = s.credit;
  W.budget[c] = 0;
  uint8_t* t = W.tape + c * TAPE_SLOT;
  const uint8_t* src = codes + i * cap;
  const int m = s.mem_size < cap ? s.mem_size : cap;
  for (int k = 0; k < m; k++) t[k] = src[k];
  // the birth genome is the tape prefix (as the oracle restores it)
  uint64_t gs = 0;
  const int bl = s.birth_length < m ? s.birth_length : m;
  for (int w = 0; w < (bl + 3) / 4; w++) {
    uint32_t v = 0;
    for (int j = 0; j < 4 && 4 * w + j < bl; j++) v |= (uint32_t)(t[4 * w + j] & CODE_MASK) << (8 * j);
    gs += gk_word(v, w, s.birth_length);
  }
  W.gkey[c] = gk_final(gs, s.birth_length);
  W.pkey[c] = 0ull;   // (a checkpoint sets the parent keys after the states: avgpu_set_parent_keys)
}

// systematics census (include/avida_gpu.h avgpu_census): one row per cell,
// written as one coalesced 48-B struct per lane
__global__ void k_census(DevWorld W, int64_t first, int64_t count, avgpu_census* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t c = first + i;
  const uint32_t ctl = W.ctl[c];
  avgpu_census r;
  memset(&r, 0, sizeof(r));
  if (ctl & CTL_ALIVE) {
    r.genotype_key = W.gkey[c];
    r.merit = W.merit[c];
    r.fitness = W.fitness[c];
    r.genome_length = W.birth_len[c];
    r.gestation_time = W.gest_time[c];
    r.copied_size = W.copied[c];
    r.executed_size = W.executed[c];
    r.generation = W.generation[c];
    r.num_divides = (ctl & CTL_FRESH) ? 0 : W.num_div[c];
  }
  out[i] = r;
}

// the parent keys of a cell range, a dead cell's (stale) word masked to 0
__global__ void k_parent_keys(DevWorld W, int64_t first, int64_t count, uint64_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t c = first + i;
  out[i] = (W.ctl[c] & CTL_ALIVE) ? W.pkey[c] : 0ull;
}

// budget = uniform or per-cell array, all live cells of [first, first+count)
__global__ void k_classify_uniform(DevWorld W, int64_t first, int64_t count, const int32_t* budget,
                                   int32_t uniform) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < count;
  const int cell = in ? (int)(first + i) : 0;
  int b = 0;
  bool want = false;
  int cls = 0;
  if (in) {
    b = budget ? budget[i] : uniform;
    W.budget[cell] = b;
    want = (W.ctl[cell] & CTL_ALIVE) && b > 0;
    if (want) cls = class_of(need_of_cell(W, cell));
    W.aclass[cell] = want ? (uint8_t)cls : (uint8_t)ACLASS_NONE;
  }
  enqueue_class(W, cell, want, cls);
}

}  // namespace

// ---------------------------------------------------------------------------
void launch_set_orgs(const DevWorld& W, hipStream_t s, int64_t first, int64_t count,
                     const uint8_t* codes, const int32_t* offsets, const int32_t* lens,
                     const double* merits, const int32_t* inputs, int deterministic) {
  hipLaunchKernelGGL(k_set_orgs, dim3(nblk(count, 64)), dim3(64), 0, s, W, first, count, codes,
                     offsets, lens, merits, inputs, deterministic);
}

void launch_get_states(const DevWorld& W, hipStream_t s, int64_t first, int64_t count,
                       avgpu_cpu_state* states, uint8_t* codes, int cap) {
  hipLaunchKernelGGL(k_get_states, dim3(nblk(count, 64)), dim3(64), 0, s, W, first, count, states,
                     codes, cap);
}

void launch_state_digest(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, uint64_t* d_out) {
  if (count <= 0) return;
  k_state_digest<<<(unsigned)((count + 127) / 128), 128, 0, s>>>(W, first, count, d_out);
}

void launch_get_census(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, avgpu_census* d_out) {
  if (count <= 0) return;
  k_census<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(W, first, count, d_out);
}
void launch_get_parent_keys(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, uint64_t* d_out) {
  if (count <= 0) return;
  k_parent_keys<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(W, first, count, d_out);
}
void launch_set_states(const DevWorld& W, hipStream_t s, int64_t first, int64_t count, const avgpu_cpu_state* in,
                       const uint8_t* codes, int cap) {
  hipLaunchKernelGGL(k_set_states, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, s, W, first, count, in,
                     codes, cap);
}

void launch_classify_uniform(const DevWorld& W, hipStream_t s, int64_t first, int64_t count,
                             const int32_t* budget, int32_t uniform) {
  hipMemsetAsync(W.class_count, 0, sizeof(int32_t) * CLASS_COUNT_WORDS, s);
  hipLaunchKernelGGL(k_classify_uniform, dim3(nblk(count, 256)), dim3(256), 0, s, W, first, count,
                     budget, uniform);
}
