// serial.hip -- k_serial_update: the serial world (oracle
// orc_run_serial_updates).  The unit also compiles class 3's main-pass
// k_interpret kernels (at the end of the file).
// Avida2Driver::Run's update with the reference's own schedule: UD = 30 x
// living organisms picks, each a merit-weighted draw of one cell from the
// scheduler's stream (cPopulation::ScheduleOrganism over a cWeightedIndex sum
// tree, tools/cWeightedIndex.cc:49-115); a picked organism with speculative
// credit spends one, otherwise it runs ProcessStepSpeculative
// (main/cPopulation.cc:5740-5788, interpret_chunk serial step) and an
// offspring is placed at once (ActivateOffspring / PositionOffspring,
// main/cPopulation.cc:621-952, :5185-5414) into a neighbour drawn from the
// same stream.  One wave per world: the picks are sequential by definition;
// the wave shares the tree walks, genome copies and the interpreter's staging.
#include "interp_launch.h"

#pragma clang fp contract(off)

namespace {

// the sum tree's leaf for x: the binary descent of SerialSched::find, five
// levels per round -- lanes fetch the 62 nodes below p in parallel, then the
// walk runs in registers (same comparisons and subtractions, same order)
__device__ __forceinline__ int64_t stree_find(const double* tree, int64_t size, double x) {
  const int lane = threadIdx.x & 63;
  int depth = 0;
  for (int64_t s = size; s > 1; s >>= 1) depth++;
  int64_t p = 1;
  int dp = 0;
  while (dp < depth) {
    const int lv = min(5, depth - dp);
    const int h = lane + 2;                     // subtree heap index of this lane's node
    const int d = 31 - __clz(h);
    double v = 0.0;
    if (h < (2 << lv) && d <= lv) v = tree[(p << d) + (h - (1 << d))];
    int k = 1;
    for (int l = 0; l < lv; l++) {
      const double left = __shfl(v, 2 * k - 2);
      if (x < left) {
        k = 2 * k;
      } else {
        x = __dsub_rn(x, left);
        k = 2 * k + 1;
      }
    }
    p = (p << lv) + (k - (1 << lv));
    dp += lv;
  }
  return p - size;
}

// SerialSched::set: leaf = v, then every node on its path to the root as the
// sum of its two children (left + right); the siblings are fetched at once
__device__ __forceinline__ void stree_set(double* tree, int64_t size, int64_t i, double v) {
  const int lane = threadIdx.x & 63;
  int depth = 0;
  for (int64_t s = size; s > 1; s >>= 1) depth++;
  const int64_t leaf = size + i;
  double sib = 0.0;
  if (lane < depth) sib = tree[(leaf >> lane) ^ 1];
  double cur = v, mine = 0.0;
  for (int k = 0; k < depth; k++) {
    const double sk = __shfl(sib, k);
    cur = ((leaf >> k) & 1) ? __dadd_rn(sk, cur) : __dadd_rn(cur, sk);
    if (lane == k) mine = cur;
  }
  if (lane == 0) tree[leaf] = v;
  if (lane < depth) tree[leaf >> (lane + 1)] = mine;
  __threadfence_block();
}

// The reference's connection list of a cell (oracle conn_base;
// tools/cTopology.h:40-55: Push() prepends, so the list runs W, SW, S, SE, E,
// NE, N, NW; build_grid drops the wrapped entries, keeping the order)
__device__ __forceinline__ int conn_base(const DevWorld& W, int cell, int* out) {
  constexpr int DX[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, DY[8] = {0, 1, 1, 1, 0, -1, -1, -1};
  const int X = W.world_x, Y = W.world_y;
  const int x = cell % X, y = cell / X;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int nx = x + DX[k], ny = y + DY[k];
    if (W.geometry == 1 && (nx < 0 || nx >= X || ny < 0 || ny >= Y)) continue;
    out[n++] = ((ny + Y) % Y) * X + (nx + X) % X;
  }
  return n;
}

// the serial world's context stream: GetUInt(n) of its next draw (counter, or
// the recorded srec_ctx); ct is its position
__device__ __forceinline__ uint32_t sctx_below(const DevWorld& W, uint32_t& ct, uint32_t n, bool& over) {
  if (W.srec_ctx) {
    double u = 0.0;
    if ((int64_t)ct < W.srec_ctx_n) u = W.srec_ctx[ct]; else over = true;
    ct++;
    const uint32_t v = (uint32_t)(u * (double)n);
    return v < n ? v : n - 1u;
  }
  return rng_below(W.sctx[0], W.sctx[1], ct, n);
}

template <int S, bool REC>
__global__ __launch_bounds__(64, 1) void k_serial_update(const DevWorld* __restrict__ Wp) {
  __shared__ __attribute__((aligned(16))) uint32_t lds32[64 * tape_stride(S) / 4 + STK_LDS_WORDS + TAB_WORDS];
  __shared__ __attribute__((aligned(16))) uint8_t child[TAPE_SLOT + 16];
  const DevWorld& W = *Wp;
  const int lane = threadIdx.x;
  const int64_t n = W.n, size = W.stree_size;
  double* tree = W.stree;
  // the tree over this update's merits (every cell's SerialSched::set)
  int na = 0;
  for (int64_t c = lane; c < size; c += 64) {
    const bool live = c < n && (W.ctl[c] & CTL_ALIVE);
    tree[size + c] = live ? W.merit[c] : 0.0;
    na += live ? 1 : 0;
  }
  __threadfence_block();
  for (int64_t lo = size >> 1; lo >= 1; lo >>= 1) {
    for (int64_t q = lo + lane; q < 2 * lo; q += 64) tree[q] = __dadd_rn(tree[2 * q], tree[2 * q + 1]);
    __threadfence_block();
  }
  for (int off = 32; off > 0; off >>= 1) na += __shfl_xor(na, off);
  const int64_t ud = (int64_t)W.ave_time_slice * na;   // cWorld::CalculateUpdateSize
  const uint32_t glo = W.grng[0], ghi = W.grng[1];
  uint32_t gct = W.grng[2];
  unsigned long long picks = 0, deaths = 0, divides = 0, births = 0, dropped = 0, over = 0;
  for (int64_t i = 0; i < ud; i++) {
    const double tot = tree[1];
    if (!(tot > 0.0)) break;
    // the scheduler's draw (its own stream: main/cPopulation.cc:7341-7346)
    double u;
    if (W.srec_sched) {
      u = (int64_t)gct < W.srec_sched_n ? W.srec_sched[gct] : 0.0;
      over += (int64_t)gct < W.srec_sched_n ? 0 : 1;
      gct++;
    } else {
      u = __dmul_rn((double)rng_next(glo, ghi, gct), 1.0 / 4294967296.0);
    }
    const int64_t c = stree_find(tree, size, __dmul_rn(u, tot));
    const uint32_t ctl = W.ctl[c];
    if (!(ctl & CTL_ALIVE)) continue;
    picks++;
    const int sp = W.spec[c];
    if (sp > 0) {                                 // a speculatively executed step
      if (lane == 0) W.spec[c] = sp - 1;
      __threadfence_block();
      continue;
    }
    if (ctl & CTL_SPECDIE) {                      // SingleProcess: m_spec_die -> Die (cpu/cHardwareCPU.cc:917-921)
      if (lane == 0) W.ctl[c] = ctl & ~(CTL_ALIVE | CTL_SPECDIE);
      __threadfence_block();
      stree_set(tree, size, c, 0.0);
      deaths++;
      continue;
    }
    // the one non-speculative SingleProcess
    // (Wp, cls, mode, first, count, chunk, lds32, sorted, row, lpw, serial)
    const int r = __shfl(interpret_chunk<S, REC>(Wp, 1, AVGPU_MODE_WORLD, c, 1, 0, lds32, false, 0, 64, 1), 0);
    __builtin_amdgcn_s_waitcnt(0);              // the step's stores (some outside the compiler's view)
    __threadfence_block();
    divides += (r >> 16) & 0xFF;
    bool replaced = false;
    if ((r >> 24) & 1) {
      // ActivateOffspring inside the h-divide (main/cPopulation.cc:621-960)
      apply_edits_wave(W, c, child);
      int t = -1, face_t = -1;
      int32_t in3[3] = {0, 0, 0};
      int alive_n = 0;
      if (W.birth_method == 4 && W.prefer_empty) {   // num_organisms, for FindRandEmptyCell
        int a = 0;
        for (int64_t q = lane; q < W.n; q += 64) a += (W.ctl[q] & CTL_ALIVE) ? 1 : 0;
        alive_n = wave_sum_i32(a);
      }
      if (lane == 0) {
        uint32_t ct = W.sctx[2];
        bool ov = false;
        if (W.birth_method == 4) {
          // FULL_SOUP_RANDOM (oracle serial_soup): FindRandEmptyCell on the
          // persistent empty_cell_id_array, else GetUInt(size)
          const uint32_t n = (uint32_t)W.n;
          t = -1;
          if (W.prefer_empty) {
            if (alive_n < (int)n) {
              uint32_t ws = n;
              uint32_t idx = sctx_below(W, ct, ws, ov);
              int cc = W.soup_perm[idx];
              bool found = true;
              while (W.ctl[cc] & CTL_ALIVE) {
                --ws;
                const int sw = W.soup_perm[ws];
                W.soup_perm[ws] = cc;
                W.soup_perm[idx] = sw;
                if (ws == 1) { found = false; break; }
                idx = sctx_below(W, ct, ws, ov);
                cc = W.soup_perm[idx];
              }
              if (found) t = cc;
            }
            if (t < 0) t = (int)sctx_below(W, ct, n, ov);
          } else {
            t = (int)sctx_below(W, ct, n, ov);
            while (!W.allow_parent && n > 1u && t == (int)c) t = (int)sctx_below(W, ct, n, ov);
          }
        } else if (W.birth_method == 5) {
          // FULL_SOUP_ELDEST (oracle serial_eldest): the reaper queue's rear
          // cell; the parent's, without ALLOW_PARENT, goes back to the rear
          const int64_t C = W.reaper_cap;
          int64_t R = W.reaper_ix[0];
          t = W.reaper[R % C];
          R++;
          if (!W.allow_parent && t == (int)c && R < W.reaper_ix[1]) {
            t = W.reaper[R % C];                                  // PopRear, then PushRear(parent)
            W.reaper[R % C] = (int)c;                             // into the slot it freed
          }
          W.reaper_ix[0] = R;
        } else {
          // PositionOffspring on the rotated connection list (oracle serial_target)
          int base[8], conn[8], found[9];
          const int nb = conn_base(W, (int)c, base);
          const int f = nb ? W.face[c] % nb : 0;
          for (int k = 0; k < nb; k++) conn[k] = base[(f + k) % nb];
          int nf = 0;
          if (W.prefer_empty)
            for (int k = 0; k < nb; k++)
              if (!(W.ctl[conn[k]] & CTL_ALIVE)) { for (int q = nf; q > 0; q--) found[q] = found[q - 1]; found[0] = conn[k]; nf++; }
          if (nf == 0 && W.birth_method == 0) {
            if (W.allow_parent) found[nf++] = (int)c;
            for (int k = 0; k < nb; k++) found[nf++] = conn[k];
          }
          t = nf == 0 ? (int)c : found[sctx_below(W, ct, (uint32_t)nf, ov)];
        }
        if (t == (int)c && !W.allow_parent) t = -1;            // target_cells[i] = -1 (:706-712)
        if (t >= 0) {
          // ActivateOrganism -> SetupInputs random (main/cEnvironment.cc:1268-1271)
          in3[0] = (15 << 24) + (int)sctx_below(W, ct, 1u << 24, ov);
          in3[1] = (51 << 24) + (int)sctx_below(W, ct, 1u << 24, ov);
          in3[2] = (85 << 24) + (int)sctx_below(W, ct, 1u << 24, ov);
          // Rotate(parent_cell) (:935-944), for the local birth methods only
          // (birth_method < NUM_LOCAL_POSITION_OFFSPRING = 4, :938)
          if (t != (int)c && W.birth_method < 4) {
            int tb[8];                                          // (not adjacent: a full turn, no change)
            const int ntb = conn_base(W, t, tb);
            for (int k = 0; k < ntb; k++) if (tb[k] == (int)c && face_t < 0) face_t = k;
          }
        }
        W.sctx[2] = ct;
        over += ov ? 1 : 0;
      }
      t = __shfl(t, 0);
#pragma unroll
      for (int k = 0; k < 3; k++) in3[k] = __shfl(in3[k], 0);
      if (t < 0) {
        dropped++;
      } else {
        const bool parent_alive = t != (int)c;
        const bool killed = (W.ctl[t] & CTL_ALIVE) != 0;
        if (parent_alive) stree_set(tree, size, c, W.merit[c]);   // AdjustSchedule(parent) :933
        Child b = child_of_record(W, c);
        b.inputs = in3;                                          // from the context stream (lane 0's)
        b.hs = 0;                                                // placed at once: no head start
        const uint64_t pk = W.gkey[c];                           // the parent's genotype key (t may be c)
        setup_child<64>(W, t, b, reinterpret_cast<const uint32_t*>(W.b_genome + c * TAPE_SLOT), lane);
        __threadfence_block();
        if (lane == 0) {
          W.pkey[t] = pk;
          W.spec[t] = 0;                                         // InsertOrganism resets the credit
          if (parent_alive && face_t >= 0) W.face[t] = (uint8_t)face_t;
          if (W.birth_method == 5) {                             // ActivateOrganism: Push(target) (:1358-1361)
            const int64_t F = W.reaper_ix[1];
            W.reaper[F % W.reaper_cap] = t;
            W.reaper_ix[1] = F + 1;
          }
        }
        __threadfence_block();
        stree_set(tree, size, t, b.merit);
        births++;
        deaths += killed ? 1 : 0;
        replaced = !parent_alive;
      }
    }
    if (replaced) continue;                       // the parent died in its own step: no speculation
    if (!(W.ctl[c] & CTL_ALIVE)) { stree_set(tree, size, c, 0.0); deaths++; continue; }
    // the speculative run (ProcessStepSpeculative, main/cPopulation.cc:5758-5766);
    // (Wp, cls, mode, first, count, chunk, lds32, sorted, row, lpw, serial)
    const int r2 = __shfl(interpret_chunk<S, REC>(Wp, 1, AVGPU_MODE_WORLD, c, 1, 0, lds32, false, 0, 64, 2), 0);
    __builtin_amdgcn_s_waitcnt(0);
    __threadfence_block();
    if (lane == 0) W.spec[c] = r2 & 0xFFFF;
    __threadfence_block();
  }
  if (lane == 0) {
    W.grng[2] = gct;
    count_add(W, AVGPU_CNT_INSTS, picks);
    if (deaths) count_add(W, AVGPU_CNT_DEATHS, deaths);
    if (divides) count_add(W, AVGPU_CNT_DIVIDES, divides);
    if (births) count_add(W, AVGPU_CNT_BIRTHS, births);
    if (dropped) count_add(W, AVGPU_CNT_DROPPED, dropped);
    if (over) count_add(W, AVGPU_CNT_REC_EXHAUSTED, over);
  }
}

}  // namespace

// one serial-world update (launch_world_post's statistics follow it)
void launch_serial_update(const DevWorld& W, const DevWorld* dW, hipStream_t s) {
  if (W.srec_ctx) hipLaunchKernelGGL((k_serial_update<CLASS3_SIZE, true>), dim3(1), dim3(64), 0, s, dW);
  else hipLaunchKernelGGL((k_serial_update<CLASS3_SIZE, false>), dim3(1), dim3(64), 0, s, dW);
}

// class 3's main-pass kernels, which share interpret_chunk<CLASS3_SIZE, REC>
// with k_serial_update (interp_launch.h INTERP_CLASS3)
INTERP_CLASS3(INTERP_DEFINE, true)
INTERP_CLASS3(INTERP_DEFINE, false)
