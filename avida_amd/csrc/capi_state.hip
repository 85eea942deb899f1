// capi_state.hip -- organism state in and out, digests, the RNG mode, the clock.
#include "host.h"

using namespace avh;

extern "C" {

int avgpu_get_states(avgpu_world* w, int64_t first, int64_t count, avgpu_cpu_state* states,
                     uint8_t* mem_ops, uint8_t* mem_flags, int mem_cap) {
  if (!w || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  DevBuf<avgpu_cpu_state> d_s(w->stream);
  DevBuf<uint8_t> d_c(w->stream);
  const bool want_mem = mem_ops && mem_flags && mem_cap > 0;
  int rc = d_s.alloc(count);
  if (rc < 0) return rc;
  if (want_mem) {
    if ((rc = d_c.alloc((size_t)count * mem_cap)) < 0) return rc;
    HIPCHK(hipMemsetAsync(d_c.get(), 0, (size_t)count * mem_cap, w->stream));
  }
  launch_get_states(w->W, w->stream, first, count, d_s.get(), d_c.get(), mem_cap);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(states, d_s.get(), count * sizeof(avgpu_cpu_state), hipMemcpyDeviceToHost, w->stream));
  std::vector<uint8_t> codes;
  if (want_mem) {
    codes.resize((size_t)count * mem_cap);
    HIPCHK(hipMemcpyAsync(codes.data(), d_c.get(), codes.size(), hipMemcpyDeviceToHost, w->stream));
  }
  HIPCHK(hipStreamSynchronize(w->stream));
  if (want_mem) {
    for (int64_t i = 0; i < count; i++) {
      const int m = std::min(states[i].mem_size, mem_cap);
      for (int k = 0; k < mem_cap; k++) {
        const size_t o = (size_t)i * mem_cap + k;
        if (k < m) {
          const uint8_t b = codes[o];
          const int op = w->code2op[b & CODE_MASK];
          mem_ops[o] = (uint8_t)(op < 0 ? 255 : op);
          mem_flags[o] = (uint8_t)(((b & TF_COPIED) ? 0x01 : 0) | ((b & TF_EXEC) ? 0x04 : 0));
        } else {
          mem_ops[o] = 0;
          mem_flags[o] = 0;
        }
      }
    }
  }
  return 0;
}

int avgpu_set_states(avgpu_world* w, int64_t first, int64_t count, const avgpu_cpu_state* states,
                     const uint8_t* mem_ops, const uint8_t* mem_flags, int mem_cap) {
  int rc = ready(w);
  if (rc < 0) return rc;
  if (first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (!states || !mem_ops || !mem_flags || mem_cap <= 0) return fail(AVGPU_EINVAL, "states / memory");
  if (count == 0) return 0;
  std::vector<uint8_t> codes((size_t)count * mem_cap, 0);
  for (int64_t i = 0; i < count; i++) {
    const avgpu_cpu_state& st = states[i];
    if (st.mem_size < 0 || st.mem_size > AVGPU_MAX_GENOME || st.mem_size > mem_cap)
      return fail(AVGPU_EINVAL, "memory size outside the tape / mem_cap");
    for (int k = 0; k < st.mem_size; k++) {
      const size_t o = (size_t)i * mem_cap + k;
      if (mem_ops[o] >= w->n_ops) return fail(AVGPU_EINVAL, "op code outside the instruction set");
      codes[o] = (uint8_t)(w->op2code[mem_ops[o]] | ((mem_flags[o] & 0x01) ? TF_COPIED : 0) |
                           ((mem_flags[o] & 0x04) ? TF_EXEC : 0));
    }
  }
  DevBuf<avgpu_cpu_state> d_s(w->stream);
  DevBuf<uint8_t> d_c(w->stream);
  if ((rc = d_s.alloc(count)) < 0 || (rc = d_c.alloc(codes.size())) < 0) return rc;
  HIPCHK(hipMemcpyAsync(d_s.get(), states, count * sizeof(avgpu_cpu_state), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(d_c.get(), codes.data(), codes.size(), hipMemcpyHostToDevice, w->stream));
  launch_set_states(w->W, w->stream, first, count, d_s.get(), d_c.get(), mem_cap);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int avgpu_state_digests(avgpu_world* w, int64_t first, int64_t count, uint64_t* out) {
  if (!w || !out || first < 0 || count < 0 || first + count > w->W.n) return fail(AVGPU_EINVAL, "cell range");
  if (count == 0) return 0;
  DevBuf<uint64_t> d(w->stream);
  const int rc = d.alloc(count);
  if (rc < 0) return rc;
  launch_state_digest(w->W, w->stream, first, count, d.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d.get(), count * sizeof(uint64_t), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

int avgpu_set_rng_mode(avgpu_world* w, int mode, const double* stream, int64_t n, const int64_t* offsets) {
  if (!w) return fail(AVGPU_EINVAL, "NULL world");
  DevWorld& W = w->W;
  HIPCHK(hipStreamSynchronize(w->stream));
  if (mode == AVGPU_RNG_COUNTER) {
    W.rec = nullptr;
    W.rec_n = 0;
    if (W.rec_off) SET_SYNC(w, W.rec_off, 0xFF, W.n * sizeof(int64_t));   // -1: counter streams
    return 0;
  }
  if (mode != AVGPU_RNG_RECORDED || !stream || n <= 0) return fail(AVGPU_EINVAL, "rng mode / stream");
  std::vector<int64_t> off(W.n, 0);
  if (offsets)
    for (int64_t c = 0; c < W.n; c++) {
      if (offsets[c] < 0 || offsets[c] > n) return fail(AVGPU_EINVAL, "stream offset outside the stream");
      off[c] = offsets[c];
    }
  int rc = w->rec_buf.alloc(n);            // (the stream is idle: the last one goes)
  if (rc < 0) return rc;
  COPY_SYNC(w, w->rec_buf.get(), stream, n * sizeof(double), hipMemcpyHostToDevice);
  if (!W.rec_off && (rc = w->alloc(&W.rec_off, (size_t)W.n)) < 0) return rc;
  COPY_SYNC(w, W.rec_off, off.data(), W.n * sizeof(int64_t), hipMemcpyHostToDevice);
  W.rec = w->rec_buf.get();
  W.rec_n = n;
  // every organism's position in its segment starts at 0
  SET_SYNC(w, W.rng + 2 * W.n, 0, W.n * sizeof(uint32_t));
  return 0;
}

int avgpu_set_clock(avgpu_world* w, const avgpu_update_stats* last) {
  if (!w || !last) return fail(AVGPU_EINVAL, "args");
  double v[2] = {(double)last->cum_insts_executed, (double)last->cum_births};   // ST_CUM_INSTS, ST_CUM_BIRTHS
  HIPCHK(hipMemcpyAsync(w->d_stats + ST_CUM_INSTS, v, sizeof(v), hipMemcpyHostToDevice, w->stream));
  // the running sums k_stats_final adds each update to
  const unsigned long long ci = (unsigned long long)last->cum_insts_executed;
  const unsigned long long cb = (unsigned long long)last->cum_births;
  HIPCHK(hipMemcpyAsync(w->W.counters + CNT_CUM_INSTS, &ci, sizeof(ci), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipMemcpyAsync(w->W.counters + CNT_CUM_BIRTHS, &cb, sizeof(cb), hipMemcpyHostToDevice, w->stream));
  // the sums given are complete: the current shards are not folded in again
  static const unsigned long long one = 1ull;
  HIPCHK(hipMemcpyAsync(w->W.counters + CNT_CUM_FLAG, &one, sizeof(one), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  w->update = last->update + 1;
  // the scheduler's key (the world's RANDOM_SEED) comes with the clock; a
  // zero seed (stats from an older checkpoint, or not from avgpu_get_stats)
  // keeps the configured one
  if (last->seed != 0) {
    w->cfg.seed = last->seed;
    w->W.seed_lo = (uint32_t)last->seed;
    w->W.seed_hi = (uint32_t)(last->seed >> 32);
    // the serial world's two streams are keyed by the seed too (serial_alloc;
    // their positions stay)
    if (w->W.grng) {
      uint32_t g[2], x[2];
      derive_key((uint32_t)last->seed, (uint32_t)(last->seed >> 32), 0x5CEDu, 0xC0FFEEu, g[0], g[1]);
      derive_key((uint32_t)last->seed, (uint32_t)(last->seed >> 32), 0xC7C7u, 0x5EED5u, x[0], x[1]);
      HIPCHK(hipMemcpyAsync(w->W.grng, g, sizeof(g), hipMemcpyHostToDevice, w->stream));
      HIPCHK(hipMemcpyAsync(w->W.sctx, x, sizeof(x), hipMemcpyHostToDevice, w->stream));
      HIPCHK(hipStreamSynchronize(w->stream));
    }
  }
  // the batch-step predictor and the pick carry
  w->pred_acc = last->sched_pred;
  w->pred_n = last->sched_pred_n;
  w->pred_cnt = std::max(std::max(last->sched_pred_bins[0], last->sched_pred_bins[1]),
                          std::max(last->sched_pred_bins[2], last->sched_pred_bins[3]));
  w->pred_pending = false;
  long long sv[SCHED_UD + 1] = {};            // no step's carry, no UD yet
  sv[SCHED_CARRY_REM] = last->sched_carry;
  HIPCHK(hipMemcpyAsync(w->W.sched, sv, sizeof(sv), hipMemcpyHostToDevice, w->stream));
  // the predictor into shard 0 (device.h pacc_sum), the other shards zero
  std::vector<long long> pa(NSHARD * PACC_STRIDE, 0);
  pa[PACC_WEIGHT] = last->sched_pred;
  pa[PACC_Q01] = (long long)((uint64_t)last->sched_pred_bins[0] | ((uint64_t)last->sched_pred_bins[1] << 32));
  pa[PACC_Q23] = (long long)((uint64_t)last->sched_pred_bins[2] | ((uint64_t)last->sched_pred_bins[3] << 32));
  HIPCHK(hipMemcpyAsync(w->W.pacc, pa.data(), pa.size() * sizeof(long long), hipMemcpyHostToDevice, w->stream));
  const double nv = (double)last->sched_pred_n;
  HIPCHK(hipMemcpyAsync(w->d_totals + TOT_ORGS, &nv, sizeof(nv), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return 0;
}

}  // extern "C"
