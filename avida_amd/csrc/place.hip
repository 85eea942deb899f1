// place.hip -- cPopulation::PositionOffspring in conflict-resolving rounds,
// for a single world and for strip tiles, side by side:
//   k_place_pick_mut / k_tile_prep + k_tile_round(0)  round 0's picks, the
//                    deferred divides' phenotype, the divide mutations
//   k_place_claim0 / k_tile_claim0  the cancellations and round 0's claims
//   k_place_round / k_tile_round    round m - 1 resolved, round m picked
//   k_empty_*        BIRTH_METHOD 4's list of empty cells (single worlds)
// and, at the end, the launchers that state the order of a step after
// interpretation (placement, activation, resources, statistics).
// Paths are relative to avida-core/source/ of the reference.
#include "device.h"
#include "births.h"

#pragma clang fp contract(off)

namespace {

// ---- strip-tile halo (DESIGN.md "Multi-GPU") ----
// Halo buffer (one per direction): per round parity p = round & 1, [X u64]
// the sender's claims on the receiver's edge row (its ghost row, k = 0) and
// [X u64] the sender's own claims on its edge row (the receiver's ghost row,
// k = 1); then [X u8] the sender's edge-row occupancy after interpretation.
// A cell of an edge row is claimed only from the two strips it touches, so
// after ONE exchange per placement round both strips know every claim on
// both rows and resolve them alike; the parities let round m + 1's claims
// go out while round m's are still being read (DESIGN.md "Multi-GPU").
__device__ __forceinline__ unsigned long long* halo_cl(uint8_t* b, int X, int p, int k) {
  return reinterpret_cast<unsigned long long*>(b) + (int64_t)(2 * p + k) * X;
}
__device__ __forceinline__ uint8_t* halo_occ(uint8_t* b, int X) { return b + (int64_t)X * 32; }
// round 0's kill times of the sender's picks on the receiver's edge row
__device__ __forceinline__ uint32_t* halo_kt(uint8_t* b, int X) { return reinterpret_cast<uint32_t*>(b + halo_kt_off(X)); }
// which halo slot a cell maps to: d = direction, x = column, k = 0 for a
// ghost cell (my claims on the neighbour's edge), 1 for an edge cell
__device__ __forceinline__ bool halo_slot(const DevWorld& W, int64_t c, int& d, int& x, bool& ghost) {
  const int X = W.world_x;
  if (c >= W.n) { const int64_t k = c - W.n; d = (int)(k / X); x = (int)(k - (int64_t)d * X); ghost = true; return true; }
  ghost = false;
  if (c < X) { d = 0; x = (int)c; return true; }
  if (c >= W.n - X) { d = 1; x = (int)(c - (W.n - X)); return true; }
  return false;
}
// a tile's cell is taken for round m's pick: occupied before round m - 1's
// resolve, or claimed in round m - 1 -- here, or by the neighbour on my edge
// row / on its own edge row (my ghost row): every claimed cell gets a winner,
// so this is the occupancy round m - 1's resolve leaves, read before that
// resolve (in the same launch) has written it.  Round 0 reads the ghost
// rows' occupancy straight from the received halo.
__device__ __forceinline__ bool tile_taken(const DevWorld& W, int64_t c, int m) {
  int d, x;
  bool ghost;
  const bool h = halo_slot(W, c, d, x, ghost);
  if (m == 0) return (h && ghost) ? halo_occ(W.h_recv[d], W.world_x)[x] != 0 : W.occ[c] != 0;
  if (W.occ[c] || W.claim_r[m - 1][c] != 0ull) return true;
  return h && halo_cl(W.h_recv[d], W.world_x, (m - 1) & 1, ghost ? 1 : 0)[x] != 0ull;
}
// round m's merged claim on cell t: mine, the neighbour's
__device__ __forceinline__ unsigned long long tile_merged(const DevWorld& W, int64_t t, int m) {
  unsigned long long v = W.claim_r[m][t];
  int d, x;
  bool ghost;
  if (halo_slot(W, t, d, x, ghost)) {
    const unsigned long long o = halo_cl(W.h_recv[d], W.world_x, m & 1, ghost ? 1 : 0)[x];
    if (o > v) v = o;
  }
  return v;
}

// The rest of a deferred divide (interp_core.h, BI_FINAL), in two halves that
// run side by side in placement round 0's launch.  The offspring's RNG key
// (derived from the parent's key and divide count) is the pick's, which draws
// from it (finalize_key); the offspring's fitness (cPhenotype::DivideReset,
// merit / gestation time) and -- from the record of the parent's last divide
// of the update, the one whose sequence number is its final num_div -- the
// parent's merit, fitness, gestation time, copied / executed sizes and last
// task counts (main/cPhenotype.cc:824-1000) are the extra blocks'
// (finalize_phenotype), off the pick's dependency chain.  BI_FINAL stays set
// (a row is rewritten whole by its next divide): both halves test it.
// (rlo, rhi: the parent's RNG key words, loaded by the caller with the pick's
// other second-hop loads; the derived key is stored for activation and left
// in p for the pick's draws)
__device__ __forceinline__ void finalize_key(const DevWorld& W, int64_t r, PlaceRow& p, uint32_t rlo, uint32_t rhi) {
  if ((p.fin & 1u) == 0u) return;
  int32_t* row = W.b_inh + r * BI_WORDS;
  derive_key(rlo, rhi, p.seq, 0x1B873593U, p.lo, p.hi);
  row[BI_RLO] = (int32_t)p.lo;
  row[BI_RHI] = (int32_t)p.hi;
}
// (every load it needs is issued before the first test: the record's row with
// its parent and sequence number, then the parent's divide count -- a chain
// of two dependent loads after the queue entry)
__device__ __forceinline__ void finalize_phenotype(const DevWorld& W, int64_t r) {
  static_assert(BI_LTASK == 12 && BI_FINAL == 11 && AVGPU_NUM_LOGIC_TASKS <= 12 && BI_PARENT == 24 && BI_SEQ == 25,
                "row quads");
  int32_t* row = W.b_inh + r * BI_WORDS;
  const int4* q = reinterpret_cast<const int4*>(row);
  // (q5's last two words, BI_PKEY, are being written by this launch's pick
  // blocks: loaded with the quad, never used -- lt[] is read up to
  // AVGPU_NUM_LOGIC_TASKS = 9 only)
  const int4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5], q6 = q[6];
  const int parent = q6.x;
  const int seq = q6.y;
  if ((q2.w & 1) == 0) return;                 // BI_FINAL
  const int nd = W.num_div[parent];
  const double merit = __hiloint2double(q0.y, q0.x);
  const int gt = q1.w;
  const double fit = __ddiv_rn(merit, (double)gt);
  const long long fb = __double_as_longlong(fit);
  row[BI_FITNESS] = (int32_t)fb;
  row[BI_FITNESS + 1] = (int32_t)(fb >> 32);
  if (seq == nd) {
    W.merit[parent] = merit;
    W.fitness[parent] = fit;
    W.gest_time[parent] = gt;
    W.child_copied[parent] = q1.y;
    W.executed[parent] = q1.z;
    const int lt[12] = {q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w};
#pragma unroll
    for (int k = 0; k < AVGPU_NUM_LOGIC_TASKS; k++) W.last_task[(int64_t)k * W.n + parent] = lt[k];
  }
}

// ---- time-ordered placement (oracle/oracle.cc "3. Time-ordered placement";
// DESIGN.md 5): a round's pick ----
// (the record's row in registers, its claim key and its BS_* states: births.h)
// BIRTH_METHOD 1: the cell's organism's age; 2: cOrganism::CalcMeritRatio
// (main/cOrganism.cc:703-708, age / merit, or the age without a positive
// merit); an empty cell (a newborn's to be) 0 (oracle position_value)
__device__ __forceinline__ double position_value(const DevWorld& W, int c) {
  if (c >= W.n || !(W.ctl[c] & CTL_ALIVE)) return 0.0;
  const double age = (double)W.age[c];
  if (W.birth_method == 1) return age;
  const double m = W.merit[c];
  return m > 0.0 ? __ddiv_rn(age, m) : age;
}
// BIRTH_METHOD 4 (POSITION_OFFSPRING_FULL_SOUP_RANDOM, main/cPopulation.cc:
// 5297-5310; oracle soup_target): with PREFER_EMPTY one draw among the cells
// empty at placement start that this round has not taken (e_list, compacted
// before every round by k_empty_*: FindRandEmptyCell, :5650-5668, draws
// uniformly among the empty cells), else -- a full world, or every empty cell
// claimed by earlier births -- GetUInt(size); without PREFER_EMPTY
// GetUInt(size), redrawn while it is the parent and ALLOW_PARENT is 0.
// Single worlds only (capi refuses strip tiles).
// What a pick reads beyond the record's row, all of it addressed by the
// row's parent alone and so loaded in one batch (one round trip): the
// parent's RNG key words (round 0: finalize_key), and the occupancy -- for
// m > 0 also round m - 1's claims -- of the eight neighbour cells and of the
// parent's own cell.  The candidate list and the chosen cell's taken bit then
// come from registers.  (A tile's taken() is tile_taken, which reads the halo
// for edge and ghost cells: it keeps its own loads, one cell after the other.)
struct PickIn {
  uint32_t rlo, rhi;     // the parent's RNG key words
  uint64_t pk;           // round 0: the parent cell's genotype key (the record's BI_PKEY words)
  int nbr[8];            // births.h neighbours_mask
  uint32_t valid, tk;    // bit k: slot k exists / is taken (slot 8: the parent's cell)
};
template <bool TILE>
__device__ __forceinline__ PickIn pick_loads(const DevWorld& W, int parent, int m) {
  PickIn in;
  in.rlo = in.rhi = 0u;
  in.valid = in.tk = 0u;
  in.pk = 0ull;
  if (m == 0) { in.rlo = W.rng[parent]; in.rhi = W.rng[W.n + parent]; in.pk = W.gkey[parent]; }
  if (!TILE && W.birth_method == 4) {          // the soup draws its cell: no neighbourhood
#pragma unroll
    for (int k = 0; k < 8; k++) in.nbr[k] = parent;
    return in;
  }
  in.valid = neighbours_mask(W, parent, in.nbr);
  if (TILE) {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if ((in.valid >> k) & 1u) in.tk |= (tile_taken(W, in.nbr[k], m) ? 1u : 0u) << k;
    in.tk |= (tile_taken(W, parent, m) ? 1u : 0u) << 8;
    return in;
  }
  uint8_t o[9];
  unsigned long long c[9];
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = W.occ[in.nbr[k]];
  o[8] = W.occ[parent];
#pragma unroll
  for (int k = 0; k < 9; k++) c[k] = 0ull;
  if (m > 0) {
    const unsigned long long* prev = W.claim_r[m - 1];
#pragma unroll
    for (int k = 0; k < 8; k++) c[k] = prev[in.nbr[k]];
    c[8] = prev[parent];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) in.tk |= ((o[k] != 0 || c[k] != 0ull) ? 1u : 0u) << k;
  return in;
}
// PositionOffspring for record r in round m (main/cPopulation.cc:5353-5413):
// an empty neighbour (not taken) when PREFER_EMPTY, else any of the eight
// neighbours or the parent (ALLOW_PARENT); BIRTH_METHOD 3 with no empty
// neighbour: the parent's cell without a draw (:5407), placed only if
// ALLOW_PARENT (ActivateOffspring :706-713), else never (BS_NO_CELL).  The
// key records whether the target is taken (a kill).  taken(c): the round's
// occupancy -- round 0 occ (tiles: the ghost rows' received occupancy), round
// m > 0 also every cell claimed in round m - 1 (tile_m >= 0: here or by the
// neighbour, tile_taken).  Returns false for no cell.
// p: the record's row, in: pick_loads of its parent.  A pick leaves its target
// and claim key in p (and in the row, one 16-B store) for the caller's atomics.
template <bool TILE>
__device__ __forceinline__ bool place_pick_one(const DevWorld& W, int64_t r, int m, PlaceRow& p, const PickIn& in) {
  int32_t* const row = W.b_inh + r * BI_WORDS;
  const int parent = p.parent;
  if (m == 0) {
    finalize_key(W, r, p, in.rlo, in.rhi);             // round 0: the record's first draws
    // the parent's genotype key, while its cell still holds it (no activation
    // of this step has run: a later one may overwrite that cell)
    *reinterpret_cast<uint64_t*>(row + BI_PKEY) = in.pk;
  }
  const uint32_t lo = p.lo, hi = p.hi;
  uint32_t ctr = p.ctr;
  auto no_cell = [&]() {
    p.target = -1;
    p.state = BS_NO_CELL - m;
    row[BI_TARGET] = -1;
    row[BI_STATE] = p.state;
  };
  int t = parent;
  bool tkn = false;
  if (!TILE && W.birth_method == 4) {
    const uint32_t n = (uint32_t)W.n;
    if (W.prefer_empty) {
      const uint32_t ne = (uint32_t)W.e_blk[(W.n + 255) / 256];
      t = ne > 0u ? W.e_list[rng_below(lo, hi, ctr, ne)] : (int)rng_below(lo, hi, ctr, n);
    } else {
      t = (int)rng_below(lo, hi, ctr, n);
      while (!W.allow_parent && n > 1u && t == parent) t = (int)rng_below(lo, hi, ctr, n);
    }
    if (t == parent && !W.allow_parent) {              // ActivateOffspring drops it (:706-713)
      p.ctr = ctr;
      row[BI_RCTR] = (int32_t)ctr;
      no_cell();
      return false;
    }
    tkn = W.occ[t] != 0 || (m > 0 && W.claim_r[m - 1][t] != 0ull);
  } else {
    const uint32_t nbrs = in.valid & 0xFFu;
    uint32_t cm = W.prefer_empty ? nbrs & ~in.tk : 0u;   // candidate slots, in list order
    int sel = 8;
    if (cm == 0u && (W.birth_method == 1 || W.birth_method == 2)) {
      // PositionAge / PositionMerit (main/cPopulation.cc:5416-5470): the parent
      // first, valued -1 without ALLOW_PARENT; a neighbour of a larger value
      // replaces the list, one of an equal value joins it (oracle place_pick)
      int cs[9];
      int nc = 0;
      double best = W.allow_parent ? position_value(W, parent) : -1.0;
      cs[nc++] = 8;
      for (int k = 0; k < 8; k++) {
        if (!((nbrs >> k) & 1u)) continue;
        const double v = position_value(W, in.nbr[k]);
        if (v > best) { best = v; nc = 0; cs[nc++] = k; }
        else if (v == best) cs[nc++] = k;
      }
      sel = cs[rng_below(lo, hi, ctr, (uint32_t)nc)];
    } else {
      if (cm == 0u && W.birth_method != 3) cm = nbrs | (W.allow_parent ? 0x100u : 0u);
      if (cm == 0u) {                          // the parent's cell, without a draw
        if (!W.allow_parent) { no_cell(); return false; }
      } else {
        const int j = (int)rng_below(lo, hi, ctr, (uint32_t)__popc(cm));
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 9; k++)
          if ((cm >> k) & 1u) { if (cnt == j) sel = k; cnt++; }
      }
    }
    tkn = ((in.tk >> 8) & 1u) != 0u;
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (sel == k) { t = in.nbr[k]; tkn = ((in.tk >> k) & 1u) != 0u; }
  }
  const unsigned long long key = claim_key(BI_TIME(p.fin), tkn, rng_next(lo, hi, ctr), W.cell0 + parent, p.seq);
  p.ctr = ctr;
  p.target = t;
  p.prio = key;
  row[BI_RCTR] = (int32_t)ctr;
  *reinterpret_cast<int4*>(row + BI_TARGET) = make_int4(t, 0, (int)(uint32_t)key, (int)(uint32_t)(key >> 32));
  W.b_tgt[(int64_t)m * W.rcap + r] = t;
  return true;
}

// BIRTH_METHOD 4 + PREFER_EMPTY: round m's candidates, ascending -- the cells
// empty at placement start (after the slices' deaths) and, for m > 0, not
// claimed in round m - 1 (FindRandEmptyCell's; oracle place_reset /
// soup_round_cells): per-256-cell counts, one block's exclusive scan over them
// (e_blk[nb]: the total), the scatter.  (Before round m's launch, occ holds
// the winners up to round m - 2; round m - 1's are in its claims.)
__device__ __forceinline__ bool soup_free(const DevWorld& W, int64_t c, int m) {
  return c < W.n && W.occ[c] == 0 && (m == 0 || W.claim_r[m - 1][c] == 0ull);
}
// (round m >= 2 of a launch k_place_round skips -- nobody picked in round
// m - 1 -- has no pick to serve: the three kernels return at once)
__device__ __forceinline__ bool soup_round_skipped(const DevWorld& W, int m) {
  return m > 1 && W.b_count[BQ_PICKED + m - 1] == 0;
}
__global__ __launch_bounds__(256) void k_empty_count(DevWorld W, int m) {
  __shared__ int ws[4];
  if (soup_round_skipped(W, m)) return;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool e = soup_free(W, c, m);
  const int cnt = __popcll(__ballot(e));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) W.e_blk[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(1024) void k_empty_scan(DevWorld W, int nb, int m) {
  __shared__ int part[1024];
  if (soup_round_skipped(W, m)) return;
  const int per = (nb + 1023) / 1024;
  const int b0 = (int)threadIdx.x * per, b1 = min(nb, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; b++) sum += W.e_blk[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {          // inclusive scan of the runs' sums
    const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = threadIdx.x > 0 ? part[threadIdx.x - 1] : 0;
  for (int b = b0; b < b1; b++) {
    const int v = W.e_blk[b];
    W.e_blk[b] = run;
    run += v;
  }
  if (threadIdx.x == 1023) W.e_blk[nb] = part[1023];
}
__global__ __launch_bounds__(256) void k_empty_scatter(DevWorld W, int m) {
  __shared__ int ws[4];
  if (soup_round_skipped(W, m)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool e = soup_free(W, c, m);
  const unsigned long long bm = __ballot(e);
  if (lane == 0) ws[wv] = __popcll(bm);
  __syncthreads();
  int base = W.e_blk[blockIdx.x];
  for (int k = 0; k < wv; k++) base += ws[k];
  if (e) W.e_list[base + __popcll(bm & ((1ull << lane) - 1ull))] = (int)c;
}

// The divide mutations (k_place_pick_mut, k_tile_prep), by 256-thread blocks:
// block blk of nblocks scans MUT_PER_BLOCK queue entries at a time -- lane k of each
// wave loads one entry's five edit words and both lengths -- and lists the
// ~10 % that have edits in LDS; the block's four waves then apply the list
// round robin, each genome from the words in hand (apply_edits_core).  A
// wave that applied its own 8 entries' edits ran up to ~5 genomes one after
// the other (the launch's longest wave, 36 us: profiles/r04f_split_*); the
// block's pool of 32 caps a wave at ~2.  (One entry per wave over 65536
// waves instead: 71 us for the fused launch, profiles/r04g_*.)
#define MUT_PER_WAVE 8
#define MUT_PER_BLOCK (4 * MUT_PER_WAVE)
__device__ __forceinline__ void mutation_block(const DevWorld& W, int64_t blk, int64_t nblocks,
                                               uint8_t (*child)[TAPE_SLOT + 16]) {
  __shared__ int ml[MUT_PER_BLOCK][8];   // record (2 words), e0..e4, len0 | len << 16
  __shared__ int mn;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // (the lane's list entry is loaded ahead, with the queue's lengths: list_entry)
  int64_t le = lane < MUT_PER_WAVE ? list_entry(W, blk * MUT_PER_BLOCK + wv * MUT_PER_WAVE + lane) : 0;
  const int64_t np = W.b_count[BQ_PRIMARY];
  const int nb = queue_len(W);
  for (int64_t q0 = blk * MUT_PER_BLOCK; q0 < nb; q0 += nblocks * MUT_PER_BLOCK) {   // block-uniform
    if (threadIdx.x == 0) mn = 0;
    __syncthreads();
    const int64_t q = q0 + wv * MUT_PER_WAVE + lane;
    const int64_t r = rec_from(W, q, np, le);
    const int64_t qx = q + nblocks * MUT_PER_BLOCK;
    le = (lane < MUT_PER_WAVE && qx < nb) ? list_entry(W, qx) : 0;
    if (lane < MUT_PER_WAVE && q < nb) {
      int e[5];
#pragma unroll
      for (int k = 0; k < 5; k++) e[k] = W.b_edit[(int64_t)k * W.rcap + r];
      const int l0 = W.b_len0[r], l1 = W.b_inh[r * BI_WORDS + BI_LEN];
      int x = e[0] | e[1] | e[2] | e[3] | e[4];
      if (W.seg_any)
        for (int k = 0; k < NSEG; k++) x |= W.b_pcnt[(int64_t)k * W.rcap + r];
      if (x) {
        const int i = atomicAdd(&mn, 1);
        ml[i][0] = (int)(uint32_t)r; ml[i][1] = (int)(r >> 32);
#pragma unroll
        for (int k = 0; k < 5; k++) ml[i][2 + k] = e[k];
        ml[i][7] = l0 | (l1 << 16);
      }
    }
    __syncthreads();
    const int n = mn;
    for (int i = wv; i < n; i += 4) {
      const int64_t r = (int64_t)(uint32_t)ml[i][0] | ((int64_t)ml[i][1] << 32);
      const int e[5] = {ml[i][2], ml[i][3], ml[i][4], ml[i][5], ml[i][6]};
      apply_edits_core(W, r, e, ml[i][7] & 0xFFFF, ml[i][7] >> 16, child[wv]);
    }
    __syncthreads();
  }
}

// A single world's placement launch m = 1..3: round m - 1 resolved and round m
// picked (oracle run_update_impl).  Each round has its own claim array, so
// round m - 1's claims stay intact for the whole launch: a record whose key is
// the maximum won -- it occupies its cell and owns it unless the cell's owner
// from an earlier round is later in time; a lost kill claim was placed and
// overwritten by the later winner; a lost empty claim picks again, treating
// every cell claimed in round m - 1 as taken (each has a winner).
// A record is still BS_PENDING at launch m only if it picked in round m - 1:
// each launch counts its pickers (b_count[BQ_PICKED + m], one atomic per
// wave), and the next launch returns at once when that count is 0 -- in a
// full world every claim is a kill claim, nothing picks again, and launches 2
// and 3 have no record to look at.  (Round 0's pickers are the whole queue:
// launch 1 always runs.)
// Per record: the row (one hop), then round m - 1's claim on its target and
// that cell's owner together, then the owner's time where there is one.
__global__ void k_place_round(DevWorld W, int m) {
  if (m > 1 && W.b_count[BQ_PICKED + m - 1] == 0) return;
  const unsigned long long* prev = W.claim_r[m - 1];
  unsigned long long* cur = W.claim_r[m];
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t le = list_entry(W, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);   // loaded ahead (list_entry)
  const int64_t np = W.b_count[BQ_PRIMARY];
  for (int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane, qn = queue_len(W); q0 < qn;
       q0 += stride) {                            // wave-uniform: the ballot below takes every lane
    const int64_t q = q0 + lane;
    const int64_t r = rec_from(W, q, np, le);
    le = q + stride < qn ? list_entry(W, q + stride) : 0;
    bool picked = false;
    do {
      if (q >= qn) break;
      PlaceRow p = place_row(W, r);
      const bool pend = p.state == BS_PENDING;
      // (a record that is not pending may have no target: its loads read cell 0)
      const int t = pend && p.target >= 0 ? p.target : 0;
      const unsigned long long pv = prev[t];
      const int own = W.owner[t];
      if (!pend) break;
      const unsigned long long key = p.prio;
      if (pv == key) {                           // won round m-1
        set_state(W, r, BS_WON + m - 1);
        W.occ[t] = 1;
        if (takes_cell(W, own, BI_TIME(p.fin))) W.owner[t] = (int)r;
        break;
      }
      if (key_kill(key)) { set_state(W, r, BS_KILL_LOST + m - 1); break; }
      const PickIn in = pick_loads<false>(W, p.parent, m);
      if (place_pick_one<false>(W, r, m, p, in)) {
        atomicMax(&cur[p.target], p.prio);
        picked = true;
      }
    } while (0);
    const unsigned long long bm = __ballot(picked);
    if (bm && lane == 0) atomicAdd(&W.b_count[BQ_PICKED + m], (int)__popcll(bm));
  }
}
// Launch 0b of a single world: a record whose parent's cell was killed before
// its own birth time (a round-0 pick of an earlier birth landed there:
// killt[parent] > 2^16 - t) is cancelled -- the reference would have killed
// its parent before this divide; the others claim their round-0 targets.
__global__ void k_place_claim0(DevWorld W, long long* pred_out, long long pred_seq) {
  // the list rows are free after the main pass: the newborn pass's (k_activate)
  if (blockIdx.x == 0 && threadIdx.x < NUM_LISTS) W.class_count[threadIdx.x] = 0;
  // the update's last step: its predictor and organisms to the host (mapped
  // memory), which chooses the next update's steps from them
  if (pred_out && blockIdx.x == 0 && threadIdx.x == 0) {
    pred_out[PRED_ACC] = pacc_sum(W, PACC_WEIGHT);
    pred_out[PRED_ORGS] = (long long)W.totals[TOT_ORGS];
    pred_out[PRED_DENSEST] = densest_quarter(W);
    // then its sequence number, after them at system scope: the host polls it
    __threadfence_system();
    __hip_atomic_store(pred_out + PRED_SEQ, pred_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // entry, row, the parent's kill time, the atomic: four hops
  QUEUE_LOOP(q, r) {
    const PlaceRow p = place_row(W, r);
    const uint32_t kt = W.killt[p.parent];
    if (p.state != BS_PENDING) continue;
    if (kt > 0x10000u - BI_TIME(p.fin)) { set_state(W, r, BS_CANCELLED); continue; }
    atomicMax(&W.claim_r[0][p.target], p.prio);
  }
}
// Launch 0 of a single world's placement with the divide mutations beside it:
// blocks [0, pblocks) pick round 0 (a pick whose target is occupied is a kill:
// the cell's kill time, atomicMax of 2^16 - t); the next fblocks finalize the
// deferred divides' phenotype; the rest apply the edits (a wave per 8 queue
// entries, rewriting the ~10 % of genomes that have edits one after the
// other; 4 waves per block) -- placement reads no genome, so they are
// independent and share one launch instead of several latency-bound ones.
// (boff / nblocks: the launch's first logical block and the logical grid, for
// the AVGPU_SPLIT_PICK_MUT diagnostic build that times the three parts apart)
__global__ __launch_bounds__(256) void k_place_pick_mut(DevWorld W, int pblocks, int fblocks, int boff, int nblocks) {
  __shared__ uint8_t child[4][TAPE_SLOT + 16];
  const int bid = (int)blockIdx.x + boff;
  if (bid < pblocks) {
    QUEUE_RECS(i, r, (int64_t)bid * 256 + threadIdx.x, (int64_t)pblocks * 256) {
      // the queue entry, the row, the parent's RNG words with the nine cells'
      // occupancy, then the stores and the atomic: four hops
      PlaceRow p = place_row(W, r);
      const PickIn in = pick_loads<false>(W, p.parent, 0);
      if (!place_pick_one<false>(W, r, 0, p, in)) continue;
      if (key_kill(p.prio)) atomicMax(&W.killt[p.target], 0x10000u - key_time(p.prio));
    }
    return;
  }
  if (bid < pblocks + fblocks) {               // deferred divides' phenotype half
    QUEUE_RECS(i, r, (int64_t)(bid - pblocks) * 256 + threadIdx.x, (int64_t)fblocks * 256)
      finalize_phenotype(W, r);
    return;
  }
  pblocks += fblocks;
  mutation_block(W, bid - pblocks, nblocks - pblocks, child);
}


// ---- strip tiles' placement: one launch per round (DESIGN.md "Multi-GPU") ----
// k_tile_prep, after interpretation: blocks [0, mblocks) apply the divide
// mutations (as k_place_pick_mut's extra blocks); the rest walk the 2 x X
// halo cells: the ghost rows empty (occ, owner, every round's claims), the
// edge rows' occupancy into the send buffers and both parities' claim slots
// zeroed; fblocks more run the deferred divides' phenotype half
// (finalize_phenotype).  (k_allot initialised the tile's own cells.)
__global__ __launch_bounds__(256) void k_tile_prep(DevWorld W, int mblocks, int fblocks) {
  __shared__ uint8_t child[4][TAPE_SLOT + 16];
  if ((int)blockIdx.x >= mblocks && (int)blockIdx.x < mblocks + fblocks) {
    QUEUE_RECS(i, r, (int64_t)(blockIdx.x - mblocks) * 256 + threadIdx.x, (int64_t)fblocks * 256)
      finalize_phenotype(W, r);
    return;
  }
  if ((int)blockIdx.x < mblocks) {
    mutation_block(W, blockIdx.x, mblocks, child);
    return;
  }
  const int X = W.world_x;
  const int g = (blockIdx.x - mblocks - fblocks) * blockDim.x + threadIdx.x;
  if (g >= 2 * X) return;
  const int d = g / X, x = g - d * X;
  const int64_t gc = ghost_cell(W, d, x);
  W.occ[gc] = 0;
  W.owner[gc] = -1;
#pragma unroll
  for (int k = 0; k < 4; k++) W.claim_r[k][gc] = 0ull;
  uint8_t* b = W.h_send[d];
  halo_occ(b, X)[x] = W.occ[edge_cell(W, d, x)];
#pragma unroll
  for (int k = 0; k < 4; k++) halo_cl(b, X, k >> 1, k & 1)[x] = 0ull;
  halo_kt(b, X)[x] = 0u;
}

// Launch m of a tile's placement (oracle orc_tile_place / tile_launch), after
// the previous exchange: blocks [0, rblocks) take the records, the rest walk
// the 2 x X halo cells.
// m = 0: round 0's picks with their kill times (own cells: killt; ghost
//   cells: the halo's kill-time slots, read by the neighbour's launch 0b);
//   the halo cells import the ghost rows' occupancy.
// m = 1..3: round m - 1 resolved against the merged claims -- a halo cell
//   whose maximum came from the neighbour (an edge cell: its claims on my edge
//   row; a ghost cell: its own claims on its edge row) is that round's remote
//   winner's (owner REMOTE_OWNER(m - 1, t), by the time rule) and occupied;
//   a claimed ghost cell is occupied; a record that won takes its cell by the
//   time rule, a lost kill claim was placed and overwritten, a lost empty
//   claim picks round m (tile_taken: the occupancy that resolve leaves) --
//   and the send parity of round m + 1 is cleared (its last contents, round
//   m - 1's, went out before this launch).
// m = 4: the last resolve only, and the record buffers' headers cleared for
//   k_halo_pack.
__global__ __launch_bounds__(256) void k_tile_round(DevWorld W, int m, int rblocks) {
  const int X = W.world_x;
  if ((int)blockIdx.x < rblocks) {
    QUEUE_RECS(q, r, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)rblocks * blockDim.x) {
      PlaceRow p = place_row(W, r);
      if (p.state != BS_PENDING) continue;
      if (m == 0) {
        const PickIn in = pick_loads<true>(W, p.parent, 0);
        if (!place_pick_one<true>(W, r, 0, p, in)) continue;
        const unsigned long long key = p.prio;
        if (!key_kill(key)) continue;
        const int t = p.target;
        const uint32_t kv = 0x10000u - key_time(key);
        if (t >= W.n) {
          const int64_t k = t - W.n;
          const int d = (int)(k / X), x = (int)(k - (int64_t)d * X);
          atomicMax(&halo_kt(W.h_send[d], X)[x], kv);
        } else {
          atomicMax(&W.killt[t], kv);
        }
        continue;
      }
      const int t = p.target;
      const unsigned long long key = p.prio;
      const int own = W.owner[t];              // (with the merged claim's loads)
      if (tile_merged(W, t, m - 1) == key) {   // won round m - 1
        set_state(W, r, BS_WON + m - 1);
        W.occ[t] = 1;
        if (takes_cell(W, own, BI_TIME(p.fin))) W.owner[t] = (int)r;
        continue;
      }
      if (key_kill(key)) { set_state(W, r, BS_KILL_LOST + m - 1); continue; }
      if (m >= 4) continue;
      const PickIn in = pick_loads<true>(W, p.parent, m);
      if (place_pick_one<true>(W, r, m, p, in)) {
        const int nt = p.target;
        const unsigned long long nk = p.prio;
        atomicMax(&W.claim_r[m][nt], nk);
        int d, x;
        bool ghost;
        if (halo_slot(W, nt, d, x, ghost)) atomicMax(&halo_cl(W.h_send[d], X, m & 1, ghost ? 0 : 1)[x], nk);
      }
    }
    return;
  }
  const int g = (blockIdx.x - rblocks) * blockDim.x + threadIdx.x;
  if (m == 4 && g < 2) {
    HaloHdr* hdr = reinterpret_cast<HaloHdr*>(W.r_send[g]);
    hdr->count = 0;
    hdr->arena_used = 0;
    hdr->overflow = 0;
  }
  if (g >= 2 * X) return;
  const int d = g / X, x = g - d * X;
  const int64_t gc = ghost_cell(W, d, x);
  if (m == 0) {
    W.occ[gc] = halo_occ(W.h_recv[d], X)[x];
    return;
  }
  const int p = (m - 1) & 1;
  const int64_t c = edge_cell(W, d, x);
  const unsigned long long rc = halo_cl(W.h_recv[d], X, p, 0)[x], rg = halo_cl(W.h_recv[d], X, p, 1)[x];
  const unsigned long long lg = W.claim_r[m - 1][gc];
  if (rc != 0ull && rc > W.claim_r[m - 1][c]) {
    const uint32_t tr = key_time(rc);
    if (takes_cell(W, W.owner[c], tr)) W.owner[c] = REMOTE_OWNER(m - 1, tr);
    W.occ[c] = 1;
  }
  if (rg != 0ull && rg > lg) {
    const uint32_t tr = key_time(rg);
    if (takes_cell(W, W.owner[gc], tr)) W.owner[gc] = REMOTE_OWNER(m - 1, tr);
  }
  if (lg != 0ull || rg != 0ull) W.occ[gc] = 1;
  if (m == 1 || m == 2) {                      // round m + 1's send parity = round m - 1's
    uint8_t* b = W.h_send[d];
    halo_cl(b, X, p, 0)[x] = 0ull;
    halo_cl(b, X, p, 1)[x] = 0ull;
  }
}
// Launch 0b of a tile (after the kill times' exchange): a record whose
// parent's cell was killed earlier -- by a pick here or, on an edge row, by
// the neighbour's (the halo's kill-time slot) -- is cancelled; the others
// claim their round-0 targets (and the halo send slots of parity 0).
__global__ __launch_bounds__(256) void k_tile_claim0(DevWorld W) {
  const int X = W.world_x;
  if (blockIdx.x == 0 && threadIdx.x < NUM_LISTS) W.class_count[threadIdx.x] = 0;
  QUEUE_LOOP(q, r) {
    const PlaceRow pr = place_row(W, r);
    const int p = pr.parent;
    uint32_t kt = W.killt[p];
    if (pr.state != BS_PENDING) continue;
    int d, x;
    bool ghost;
    if (halo_slot(W, p, d, x, ghost)) kt = max(kt, halo_kt(W.h_recv[d], X)[x]);
    if (kt > 0x10000u - BI_TIME(pr.fin)) { set_state(W, r, BS_CANCELLED); continue; }
    const int t = pr.target;
    const unsigned long long key = pr.prio;
    atomicMax(&W.claim_r[0][t], key);
    if (halo_slot(W, t, d, x, ghost)) atomicMax(&halo_cl(W.h_send[d], X, 0, ghost ? 0 : 1)[x], key);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// placement kernels stride over the queue; 8 blocks of 256 per CU cover it
// (AVGPU_PLACE_GRID overrides the cap for sweeps)
static unsigned place_grid(const DevWorld& W) {
  static const int cap = env_int("AVGPU_PLACE_GRID", 2048, 1, INT32_MAX);
  return (unsigned)std::min<int64_t>(nblk(W.rcap, 256), cap);
}

static bool has_divide_mutations(const DevWorld& W) {
  return (W.th_div_mut | W.th_div_ins | W.th_div_del | W.th_div_slip | W.th_div_uni) != 0 || W.seg_any;
}
static unsigned mut_grid(const DevWorld& W) { return (unsigned)std::min<int64_t>(nblk(W.rcap, MUT_PER_WAVE), 8192); }

// ---- the order of a step after interpretation ----
// Placement round k claims into its own array claim_r[k] (device.h): no
// clearing launch per round.  Each record clears the claims it made when it
// is activated; round 3's, which k_activate reads, are cleared by k_allot.
void launch_world_post(const DevWorld& W, hipStream_t s, uint32_t key, int sub, int nsub, long long* pred_out,
                       long long pred_seq) {
  // the occupancy was initialised by k_allot; the divide mutations
  // ride in round 0's pick launch
  // round 0's pick (with the divide mutations beside it), then three launches
  // of resolve(m-1) + pick(m), then activation with round 3's resolve: 5
  // launches instead of 9 (k_place_round)
  const unsigned bb = place_grid(W);
  const int pm = has_divide_mutations(W) ? (int)((mut_grid(W) + 3) / 4) : 0;
  const int pf = (int)std::min<unsigned>(bb, 256u);   // finalize_phenotype blocks
  const int nbk = (int)bb + pf + pm;
  const bool soup = W.birth_method == 4 && W.prefer_empty;
  auto soup_cells = [&](int m) {                    // the soup's candidates of round m (k_empty_*)
    const int eb = (int)nblk(W.n, 256);
    hipLaunchKernelGGL(k_empty_count, dim3(eb), dim3(256), 0, s, W, m);
    hipLaunchKernelGGL(k_empty_scan, dim3(1), dim3(1024), 0, s, W, eb, m);
    hipLaunchKernelGGL(k_empty_scatter, dim3(eb), dim3(256), 0, s, W, m);
  };
  if (soup) soup_cells(0);
#ifdef AVGPU_SPLIT_PICK_MUT
  hipLaunchKernelGGL(k_place_pick_mut, dim3(bb), dim3(256), 0, s, W, (int)bb, pf, 0, nbk);
  hipLaunchKernelGGL(k_place_pick_mut, dim3(pf), dim3(256), 0, s, W, (int)bb, pf, (int)bb, nbk);
  if (pm) hipLaunchKernelGGL(k_place_pick_mut, dim3(pm), dim3(256), 0, s, W, (int)bb, pf, (int)bb + pf, nbk);
#else
  hipLaunchKernelGGL(k_place_pick_mut, dim3(nbk), dim3(256), 0, s, W, (int)bb, pf, 0, nbk);
#endif
  hipLaunchKernelGGL(k_place_claim0, dim3(bb), dim3(256), 0, s, W, pred_out, pred_seq);
  for (int m = 1; m < 4; m++) {
    if (soup) soup_cells(m);
    hipLaunchKernelGGL(k_place_round, dim3(bb), dim3(256), 0, s, W, m);
  }
  launch_activate(W, s, ACT_WORLD, key, sub, nsub);
}

// after the newborn pass (interp.hip): the step's global consumption settled,
// then (eager) the update's statistics
void launch_world_end(const DevWorld& W, hipStream_t s, double* stats, bool eager) {
  launch_resources_end(W, s);
  if (eager) launch_stats(W, s, stats);
}

// after a serial-world update (its births are placed): resources, statistics
void launch_serial_post(const DevWorld& W, hipStream_t s, double* stats) {
  launch_resources_end(W, s);
  launch_stats(W, s, stats);
}

// ---- strip tiles: the same step split around the halo exchanges ----
// after interpretation: the divide mutations, the ghost rows emptied and the
// edge-row occupancy out (one launch, k_tile_prep)
void launch_tile_after_interpret(const DevWorld& W, hipStream_t s) {
  const unsigned hb = nblk(2 * (int64_t)W.world_x, 256);
  const int mb = has_divide_mutations(W) ? (int)((mut_grid(W) + 3) / 4) : 0;
  const int fb = (int)std::min<unsigned>(place_grid(W), 256u);   // finalize_phenotype blocks
  hipLaunchKernelGGL(k_tile_prep, dim3(mb + fb + hb), dim3(256), 0, s, W, mb, fb);
}

// TP_ROUND:    round 0's picks and kill times, or (round 1..3) k_tile_round:
//              resolve round - 1, pick round
// TP_CLAIM0:   (round 0) the cancellations and round 0's claims (k_tile_claim0)
// TP_PACK:     (round 3) the last resolve, then the ghost-row winners packed
//              into the record buffers
// TP_ACTIVATE: (round 3) this tile's own winners activated -- while the records
//              travel; avgpu_tile_finish then activates the received ones
void launch_tile_place(const DevWorld& W, hipStream_t s, int round, int phase, uint32_t key, int sub, int nsub) {
  const unsigned bb = place_grid(W);
  const unsigned hb = nblk(2 * (int64_t)W.world_x, 256);
  if (phase == TP_ROUND) {
    hipLaunchKernelGGL(k_tile_round, dim3(bb + hb), dim3(256), 0, s, W, round, (int)bb);
  } else if (phase == TP_CLAIM0) {
    hipLaunchKernelGGL(k_tile_claim0, dim3(bb), dim3(256), 0, s, W);
  } else if (phase == TP_PACK) {
    hipLaunchKernelGGL(k_tile_round, dim3(bb + hb), dim3(256), 0, s, W, 4, (int)bb);
    launch_halo_pack(W, s);
  } else {
    launch_activate(W, s, ACT_STRIP, key, sub, nsub);
  }
}

void launch_tile_finish(const DevWorld& W, hipStream_t s, uint32_t key, int sub, int nsub) {
  launch_activate_remote(W, s, key, sub, nsub);
}
