// activate.hip -- the placed births into their cells:
//   k_activate       cPopulation::ActivateOrganism + cPhenotype::SetupOffspring
//                    of the records that own their cell (a single world also
//                    resolves placement round 3 here), each newborn's budget
//                    and its entry in the newborn pass's lists
//   k_halo_pack      a strip's winners of ghost-row cells into the record
//                    buffers that travel to the neighbouring strips
//   k_activate_remote  the records received from them
// Paths are relative to avida-core/source/ of the reference.
#include "device.h"
#include "births.h"

#pragma clang fp contract(off)

namespace {

// ---- the batch step's newborns (oracle newborn_pass) ----
// An activated offspring first gives back (1 - t) of what its cell's replaced
// organism consumed in the step's main pass, then runs its own share of the
// step's remaining picks: Binomial(round(UD_s (1 - t)), merit / total) from a
// stateless draw of its global cell, in the newborn pass (interp.hip NB).
// The picks beyond what the replaced organism had left ((1 - t) of the
// instructions it ran) are the step's carry, taken from the next allotment.
__device__ __forceinline__ double nb_frac(uint32_t t) { return __dmul_rn((double)(0x10000u - t), 1.0 / 65536.0); }
__device__ __forceinline__ long long newborn_budget(const DevWorld& W, int64_t c, uint32_t t, double merit,
                                                    uint32_t key, long long uds, double total) {
  if (!(total > 0.0) || uds <= 0) return 0;
  const long long n = (long long)floor(__dadd_rn(__dmul_rn((double)uds, nb_frac(t)), 0.5));
  const double p = __ddiv_rn(sched_weight(merit, 0u), total);   // (oracle: sched_weight, no head start)
  const long long b = binom_draw(n, p, node_draw(W.seed_lo, W.seed_hi, key, SALT_NEWBORN, (uint64_t)(W.cell0 + c)));
  return min(b, (long long)(BUDGET_PRIM - 1));
}
__device__ __forceinline__ void newborn_credit(const DevWorld& W, int64_t c, uint32_t t) {
  const double f = nb_frac(t);
  for (int r = 0; r < W.n_res; r++) {
    const double v = W.cons[(int64_t)r * W.n + c];
    if (v == 0.0) continue;
    const double back = __dmul_rn(v, f);
    const ResParam& q = W.res_param[r];
    if (q.geometry != AVGPU_RES_GLOBAL) {
      double* p = W.res_amount + (int64_t)q.slot * W.n + c;
      *p = __dadd_rn(*p, back);
    } else {
      atomicAdd(W.res_cons + r, 0ull - (unsigned long long)__dmul_rn(back, RES_FIX));
    }
  }
}
// one newborn in cell c: credit, budget, carry; returns its list row (-1: no slice)
// (ran: W.ran[c], loaded by the caller ahead of the offspring's stores -- a
// load behind them would wait for all of them)
__device__ __forceinline__ int newborn_setup(const DevWorld& W, int64_t c, uint32_t t, double merit, int len,
                                             uint32_t key, long long uds, double total, long long& carry,
                                             unsigned long long& wasted, int ran) {
  if (W.env_resources) newborn_credit(W, c, t);
  const long long left = (long long)__dmul_rn((double)ran, nb_frac(t));
  const long long bud = newborn_budget(W, c, t, merit, key, uds, total);
  carry += bud - left;
  wasted += (unsigned long long)left;
  W.budget[c] = (int32_t)bud;
  return bud > 0 ? class_of(::need_of(len, CTL_ALIVE, W.size_range)) : -1;
}
// the wave's newborns into the newborn pass's lists (row 0: class 0, rows
// 1..3 the list classes), one atomic per row and wave
__device__ __forceinline__ void newborn_enqueue(const DevWorld& W, int cell, int row) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NUM_CLASSES; k++) {
    const unsigned long long m = __ballot(row == k);
    if (!m) continue;
    int base = 0;
    if (lane == 0) base = atomicAdd(&W.class_count[k], (int)__popcll(m));
    base = __shfl(base, 0);
    if (row == k) W.class_list[(int64_t)k * W.n + base + (int)__popcll(m & ((1ull << lane) - 1ull))] = cell;
  }
}

// One lane per queued birth: the owners of cells inside this world are
// activated (ActivateOrganism + SetupOffspring; owners of ghost-row cells were
// shipped by k_halo_pack), with the head start 2^16 - t for their first
// allotment.  The record's fields are loaded before the ownership test
// (independent loads in flight together instead of a chain behind it).
// fused ACT_WORLD (single world): round 3 is resolved here -- a round-3 winner owns
// its cell unless the owner from an earlier round is later in time; an
// earlier round's owner keeps it unless a round-3 winner (necessarily a
// kill claim: the cell was taken) is not earlier than it.  ACT_STRIP (strip
// tiles): the owners are final (k_tile_round resolved round 3).  Either way
// each record clears the claims it made (round 3's, which this launch reads,
// are cleared by k_allot).  A record that does not own its cell was placed
// and overwritten (AVGPU_CNT_OVERWRITTEN), unless it was cancelled
// (AVGPU_CNT_CANCELLED: its parent died first) or found no cell (AVGPU_CNT_DROPPED).
#ifndef ACT_PRE
#define ACT_PRE 8    // 16-B quads of the offspring's genome k_activate loads ahead
#endif
__global__ __launch_bounds__(64) void k_activate(DevWorld W, int fused, uint32_t key, int sub, int nsub) {
  const int lane = threadIdx.x & 63;
  int64_t le = list_entry(W, (int64_t)blockIdx.x * 64 + lane);   // loaded ahead, with the lengths (list_entry)
  const int64_t np = W.b_count[BQ_PRIMARY];
  const int nb = queue_len(W);
  const int64_t ncell = W.n + (W.tiled ? 2 * (int64_t)W.world_x : 0);
  const double total = W.totals[TOT_DIV];
  const long long uds = sub_share((long long)W.totals[TOT_UD], sub, nsub);
  unsigned long long born = 0, over = 0, canc = 0, nocell = 0, bad = 0, wasted = 0, nbs = 0;
  long long carry = 0;
  for (int64_t q0 = (int64_t)blockIdx.x * 64; q0 < nb; q0 += (int64_t)gridDim.x * 64) {
    const int64_t q = q0 + lane;
    const int64_t i = rec_from(W, q, np, le);
    le = q + (int64_t)gridDim.x * 64 < nb ? list_entry(W, q + (int64_t)gridDim.x * 64) : 0;
    int nrow = -1, ncell_nb = 0;
    do {
      if (q >= nb) break;
      // the genome's first 128 B, loaded before the claims decide whether the
      // record won (a dependent round trip less for the ~95 % that do; the
      // whole class-0 genome, 20 quads, measured no faster)
      const uint4* g4 = reinterpret_cast<const uint4*>(W.b_genome + i * TAPE_SLOT);
      uint4 pre[ACT_PRE];
#pragma unroll
      for (int u = 0; u < ACT_PRE; u++) pre[u] = g4[u];
      // the whole row with them: the phenotype, the parent's task counts and
      // the placement words (target, state, claim key, length)
      static_assert(BI_LTASK == 12 && AVGPU_NUM_LOGIC_TASKS <= 12 && BI_STATE == 27 && BI_TARGET == 28 && BI_PRIO == 30,
                    "row quads");
      const int4* rq = reinterpret_cast<const int4*>(W.b_inh + i * BI_WORDS);
      const int4 q0 = rq[0], q1 = rq[1], q2 = rq[2], q3 = rq[3], q4 = rq[4], q5 = rq[5], q6 = rq[6], q7 = rq[7];
      const int tgt = q7.x;
      const int st = q6.w;
      const unsigned long long prio = (unsigned long long)(uint32_t)q7.z | ((unsigned long long)(uint32_t)q7.w << 32);
      Child b = child_of_row(W, i, q0, q1, q2, q6);
      const int lt[12] = {q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w};
      // the second hop, everything the target addresses: the replaced
      // organism's instructions, round 3's claim on the cell and its owner
      // (a target out of range reads cell 0; it is never used)
      const bool tin = tgt >= 0 && (int64_t)tgt < ncell;
      const int64_t tl = tin ? tgt : 0;
      const int ran = (tin && (int64_t)tgt < W.n) ? W.ran[tl] : 0;
      const unsigned long long c3 = W.claim_r[3][tl];
      const int own = W.owner[tl];
      const int lastr = last_claim_round(st);
      // the record's claims, round k's at b_tgt[k] (the last one its target);
      // a target out of range is a corrupt record: counted, never written
      bool ok = true;
      for (int k = 0; k <= lastr && k < 3; k++) {
        const int tk = (k == lastr && tgt >= 0) ? tgt : W.b_tgt[(int64_t)k * W.rcap + i];
        if (tk >= 0 && (int64_t)tk < ncell) W.claim_r[k][tk] = 0ull;
        else ok = false;
      }
      if (st == BS_CANCELLED) { canc++; break; }
      if (st <= BS_NO_CELL) { nocell++; break; }
      if (!ok || tgt < 0 || (int64_t)tgt >= ncell) { bad++; break; }
      const uint32_t t = 0x10000u - b.hs;
      bool won = false;
      if (fused == ACT_STRIP) {
        won = st >= BS_WON && st < BS_WON + 4 && own == (int)i;
      } else if (st == BS_PENDING) {           // (the owner's time: the one further dependent load)
        won = c3 == prio && takes_cell(W, own, t);
      } else if (st >= BS_WON && st < BS_WON + 4) {
        won = own == (int)i && !(c3 != 0ull && key_time(c3) >= t);
      }
      if (!won) { over++; break; }
      if (b.len < 0 || b.len > AVGPU_MAX_GENOME) { bad++; break; }   // (k_halo_pack skips it too)
      if (tgt >= W.n) break;                   // sent to the neighbouring tile
      born++;
      b.hs = 0;                                // it runs its share of this step instead (newborn pass)
      setup_child_lane<ACT_PRE>(W, tgt, b, W.b_genome + i * TAPE_SLOT, pre, lt);
      static_assert(BI_PKEY == 22, "the parent's key: the last two words of q5");
      W.pkey[tgt] = (uint64_t)(uint32_t)q5.z | ((uint64_t)(uint32_t)q5.w << 32);
      nrow = newborn_setup(W, tgt, t, b.merit, b.len, key, uds, total, carry, wasted, ran);
      ncell_nb = tgt;
    } while (0);
    nbs += nrow >= 0 ? 1ull : 0ull;
    newborn_enqueue(W, ncell_nb, nrow);
  }
  for (int off = 32; off > 0; off >>= 1) {
    born += __shfl_xor(born, off);
    over += __shfl_xor(over, off);
    canc += __shfl_xor(canc, off);
    nocell += __shfl_xor(nocell, off);
    bad += __shfl_xor(bad, off);
    wasted += __shfl_xor(wasted, off);
    nbs += __shfl_xor(nbs, off);
    carry += __shfl_xor(carry, off);
  }
  if (threadIdx.x == 0) {
    if (born) count_add(W, AVGPU_CNT_BIRTHS, born);
    if (over) count_add(W, AVGPU_CNT_OVERWRITTEN, over);
    if (canc) count_add(W, AVGPU_CNT_CANCELLED, canc);
    if (nocell) count_add(W, AVGPU_CNT_DROPPED, nocell);
    if (bad) count_add(W, AVGPU_CNT_BAD_RECORD, bad);
    if (wasted) count_add(W, AVGPU_CNT_WASTED, wasted);
    if (nbs) count_add(W, AVGPU_CNT_SLICES, nbs);
    if (carry) atomicAdd(reinterpret_cast<unsigned long long*>(W.sched + SCHED_CARRY), (unsigned long long)carry);
  }
}

// Winners of ghost-row cells -> record buffer of that direction (one wave per
// queued birth; one record per ghost cell at most: its last winner here).
// The lanes of a wave test 64 queued births at once; the wave then packs the
// few that won a ghost cell one after the other (a wave per queued birth
// spent ~40 us per update on the test alone).
__global__ __launch_bounds__(64) void k_halo_pack(DevWorld W) {
  const int nb = queue_len(W);
  const int lane = threadIdx.x;
  const int X = W.world_x;
  unsigned long long sent = 0, lost = 0;
  for (int64_t q0 = (int64_t)blockIdx.x * 64; q0 < nb; q0 += (int64_t)gridDim.x * 64) {
    const int64_t q = q0 + lane;
    int64_t mine = -1;
    if (q < nb) {
      const int64_t i = rec_of(W, q);
      const PlaceRow p = place_row(W, i);
      const int tgt = p.target, st = p.state;
      // (a target past the ghost rows or a length out of range is a corrupt
      // record: counted in k_activate, which sees the same fields, never sent)
      if (st >= BS_WON && st < BS_WON + 4 && tgt >= W.n && (int64_t)tgt < W.n + 2 * (int64_t)X &&
          p.len >= 0 && p.len <= AVGPU_MAX_GENOME && W.owner[tgt] == (int)i)
        mine = i;
    }
    for (unsigned long long m = __ballot(mine >= 0); m; m &= m - 1ull) {
    const int64_t i = (int64_t)__shfl((long long)mine, __ffsll((long long)m) - 1);
    const PlaceRow pi = place_row(W, i);
    const int tgt = pi.target;
    const int d = (tgt - (int)W.n) / X, col = (tgt - (int)W.n) - d * X;
    const int len = pi.len;
    HaloHdr* hdr = reinterpret_cast<HaloHdr*>(W.r_send[d]);
    HaloRec* recs = reinterpret_cast<HaloRec*>(W.r_send[d] + sizeof(HaloHdr));
    uint8_t* arena = W.r_send[d] + sizeof(HaloHdr) + (int64_t)X * sizeof(HaloRec);
    int slot = 0, off = 0;
    if (lane == 0) {
      slot = atomicAdd(&hdr->count, 1);
      off = atomicAdd(&hdr->arena_used, (len + 3) & ~3);
    }
    slot = __shfl(slot, 0);
    off = __shfl(off, 0);
    const bool fits = (int64_t)off + len <= W.r_arena;
    if (lane == 0) {
      HaloRec r;
      r.col = col; r.round = pi.state - BS_WON; r.len = fits ? len : -1;
      const Child b = child_of_record(W, i);
      r.gen = b.gen; r.ccopied = b.ccopied; r.exec = b.exec; r.gest = b.gest;
      r.rng_lo = b.lo; r.rng_hi = b.hi; r.rng_ctr = b.ctr;
      r.off = off; r.t = 0x10000u - b.hs; r.merit = b.merit; r.fitness = b.fitness;
#pragma unroll
      for (int t = 0; t < AVGPU_NUM_LOGIC_TASKS; t++) r.last_task[t] = b.ltask[t];
      r.pad2[0] = W.b_inh[i * BI_WORDS + BI_PKEY];       // the parent's genotype key
      r.pad2[1] = W.b_inh[i * BI_WORDS + BI_PKEY + 1];
      r.pad2[2] = 0;
      recs[slot] = r;
      if (!fits) atomicAdd(&hdr->overflow, 1);
    }
    if (fits) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(W.b_genome + i * TAPE_SLOT);
      uint32_t* dst = reinterpret_cast<uint32_t*>(arena + off);
      for (int w = lane; w < (len + 3) / 4; w += 64) dst[w] = src[w];
      sent++;
    } else {
      lost++;
    }
    }
  }
  if (lane == 0) {
    if (sent) count_add(W, AVGPU_CNT_HALO_SENT, sent);
    if (lost) { count_add(W, AVGPU_CNT_HALO_LOST, lost); count_add(W, AVGPU_CNT_DROPPED, lost); }
  }
}

// Records received from direction d: the offspring owns its target cell when
// it was that cell's last winner (owner == REMOTE_OWNER(its round)).
__global__ __launch_bounds__(64) void k_activate_remote(DevWorld W, uint32_t key, int sub, int nsub) {
  const int lane = threadIdx.x;
  const double total = W.totals[TOT_DIV];
  const long long uds = sub_share((long long)W.totals[TOT_UD], sub, nsub);
  long long carry = 0;
  unsigned long long wasted = 0, nbs = 0;
  const int X = W.world_x;
  // blocks [0, G/2) take the records from above, the rest those from below
  const int half = gridDim.x >> 1;
  const int d = (int)blockIdx.x >= half ? 1 : 0;
  const int b0 = (int)blockIdx.x - d * half;
  const HaloHdr* hdr = reinterpret_cast<const HaloHdr*>(W.r_recv[d]);
  const HaloRec* recs = reinterpret_cast<const HaloRec*>(W.r_recv[d] + sizeof(HaloHdr));
  const uint8_t* arena = W.r_recv[d] + sizeof(HaloHdr) + (int64_t)X * sizeof(HaloRec);
  const int nrec = min(hdr->count, X);
  unsigned long long born = 0, lost = 0;
  for (int q = b0; q < nrec; q += half) {
    const HaloRec r = recs[q];
    if (r.len < 0) continue;                  // lost at the sender (counted there)
    // fields used as indices / lengths are checked: a record the exchange
    // delivered damaged is counted (AVGPU_CNT_BAD_RECORD), never followed
    if (r.col < 0 || r.col >= X || r.len > AVGPU_MAX_GENOME || r.off < 0 || (r.off & 3) ||
        (int64_t)r.off + r.len > W.r_arena || r.round < 0 || r.round > 3) {
      if (lane == 0) count_add(W, AVGPU_CNT_BAD_RECORD, 1ull);
      continue;
    }
    const int64_t c = edge_cell(W, d, r.col);
    if (W.owner[c] != REMOTE_OWNER(r.round, r.t)) { lost++; continue; }   // overwritten by a later winner
    born++;
    Child b;
    b.len = r.len; b.gen = r.gen; b.ccopied = r.ccopied; b.exec = r.exec; b.gest = r.gest;
    b.hs = 0;                                  // it runs its share of this step (newborn pass)
    b.merit = r.merit; b.fitness = r.fitness; b.lo = r.rng_lo; b.hi = r.rng_hi; b.ctr = r.rng_ctr;
    b.ltask = recs[q].last_task; b.lstride = 1;
    const int ran = W.ran[c];
    setup_child<64>(W, c, b, reinterpret_cast<const uint32_t*>(arena + r.off), lane);
    if (lane == 0) {
      W.pkey[c] = (uint64_t)(uint32_t)r.pad2[0] | ((uint64_t)(uint32_t)r.pad2[1] << 32);
      const int row = newborn_setup(W, c, r.t, r.merit, r.len, key, uds, total, carry, wasted, ran);
      if (row >= 0) {
        nbs++;
        const int slot = atomicAdd(&W.class_count[row], 1);
        W.class_list[(int64_t)row * W.n + slot] = (int)c;
      }
    }
  }
  if (lane == 0) {
    if (born) count_add(W, AVGPU_CNT_BIRTHS, born);
    if (lost) count_add(W, AVGPU_CNT_OVERWRITTEN, lost);
    if (wasted) count_add(W, AVGPU_CNT_WASTED, wasted);
    if (nbs) count_add(W, AVGPU_CNT_SLICES, nbs);
    if (carry) atomicAdd(reinterpret_cast<unsigned long long*>(W.sched + SCHED_CARRY), (unsigned long long)carry);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// k_activate: a lane per birth; 2048 waves cover 131k queued births per pass
static unsigned lane_grid(const DevWorld& W) { return (unsigned)std::min<int64_t>(nblk(W.rcap, 64), 2048); }

void launch_activate(const DevWorld& W, hipStream_t s, int fused, uint32_t key, int sub, int nsub) {
  hipLaunchKernelGGL(k_activate, dim3(lane_grid(W)), dim3(64), 0, s, W, fused, key, sub, nsub);
}

void launch_halo_pack(const DevWorld& W, hipStream_t s) {
  hipLaunchKernelGGL(k_halo_pack, dim3(lane_grid(W)), dim3(64), 0, s, W);
}

// G / 2 blocks per direction (k_activate_remote)
void launch_activate_remote(const DevWorld& W, hipStream_t s, uint32_t key, int sub, int nsub) {
  const unsigned rb = (unsigned)std::max(1, std::min(W.world_x, 4096));
  hipLaunchKernelGGL(k_activate_remote, dim3(2 * rb), dim3(64), 0, s, W, key, sub, nsub);
}
